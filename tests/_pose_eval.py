"""What tests/test_pose_eval_f64.py (GPU) and tests/test_pose_eval_bound.py (CPU) share: the inputs of one loop-closure evaluation
(mode 2: PoseEstimator::calcRes + calcGSSSE), the float64 reference's estimator and the poses."""
import numpy as np

from _gn_checks import motion_3x
from _pose_jobs import loop_inputs
from _scenes import make_scene
from direct_stereo_slam_amd import synth as S
from oracle import numpy_ref as N


class PoseInputs:
    """points, per-level colours, target pyramid, intrinsics and exposures: the arguments of dsm_pose_estimator_estimate"""

    def __init__(self, sc, xyz, cols, ref_exposure=1.0, new_exposure=1.0, dIp=None):
        self.sc, self.w, self.h, self.nl, self.K = sc, sc.w, sc.h, sc.nl, sc.K
        self.xyz, self.cols = np.ascontiguousarray(xyz, np.float64), [np.ascontiguousarray(c, np.float32) for c in cols]
        self.ref_exposure, self.new_exposure = ref_exposure, new_exposure
        self.dIp = sc.new_p if dIp is None else dIp

    def args(self):
        return self.xyz, self.cols, self.ref_exposure, self.dIp, self.new_exposure, self.K

    def cut(self, n):
        """the first n points"""
        return PoseInputs(self.sc, self.xyz[:n], [c[:n] for c in self.cols], self.ref_exposure, self.new_exposure, self.dIp)

    def with_points(self, xyz, cols=None):
        return PoseInputs(self.sc, xyz, self.cols if cols is None else cols, self.ref_exposure, self.new_exposure, self.dIp)


def scene_inputs(size, seed, n, aff=(0.0, 0.0), ref_exposure=1.0, new_exposure=1.0):
    """loop_inputs of a scene whose new frame is rendered with the brightness map that AffLight::fromToVecExposure gives for the
    affine pair `aff` and the two exposures against the estimator's reference pair (0, 0): at `aff` the photometry is consistent"""
    import math

    from _scenes import aff_from_to

    a, b = aff_from_to(ref_exposure, new_exposure, (0.0, 0.0), aff)
    sc = make_scene(size, seed=seed, a=math.log(a), b=b)
    xyz, cols = loop_inputs(sc, n=n, seed=seed)
    return PoseInputs(sc, xyz, cols, ref_exposure, new_exposure)


def numpy_estimator(inp):
    npe = N.NumpyPoseEstimator(inp.w, inp.h, inp.nl)
    npe.load(*inp.args())
    return npe


def three_poses(sc):
    return [S.IDENTITY_POSE, sc.gt_pose, motion_3x(sc.gt_pose)]


def matrix(pose):
    return N.pose_to_matrix(np.asarray(pose, np.float64))
