"""GPU parity tests proper: the HIP path through the C ABI against the CPU oracle on the same
seeded inputs.

Bars:
  * integer outputs (numTermsInE, numSaturated -> rs[5], warped count) bit-exact;
  * float sums (E, H, b, flow indicators): relative 2e-5 of the largest entry -- the device
    reduces in a different (fixed) order than the reference's SSE lanes, nothing else differs;
  * LM results (pose, affine, scale): the tolerance SURVEY.md section 8d states, per-frame pose
    difference <= 1e-4 relative on fixtures.
"""
import numpy as np
import pytest

from direct_stereo_slam_amd import synth as S
from oracle import oracle as O

from _scenes import hip_tracker, make_affine_scene, make_scene, oracle_tracker, regrad

pytestmark = pytest.mark.gpu

FLOAT_RTOL = 2e-5


def assert_eval_pose_equal(orc, trk, lvl, pose, aff, cutoff):
    rs_o = orc.calc_res_pose(lvl, pose, aff, cutoff)
    H_o, b_o = orc.calc_gs_pose(lvl, pose, aff)
    E64 = orc.last_energy_f64()
    rs_g, H_g, b_g, n_g = trk.calcResPose(lvl, pose, aff, cutoff)
    assert rs_g[1] == rs_o[1], "numTermsInE differs"
    assert n_g == orc.pose_warped_n(), "warped count differs"
    if rs_o[1] > 0:
        assert np.float32(rs_g[5]) == np.float32(rs_o[5]), "saturated ratio differs"
        np.testing.assert_allclose(rs_g[0], E64, rtol=2e-6)
        assert abs(rs_o[0] - E64) <= max(2e-5, rs_o[1] * 2.0 ** -24) * E64  # quirk Q1 error bound
    np.testing.assert_allclose(rs_g[2:5], rs_o[2:5], rtol=FLOAT_RTOL, atol=1e-9)
    if n_g > 0:
        np.testing.assert_allclose(H_g, H_o, rtol=0, atol=FLOAT_RTOL * np.abs(H_o).max())
        np.testing.assert_allclose(b_g, b_o, rtol=0, atol=FLOAT_RTOL * max(np.abs(b_o).max(), 1e-3 * np.sqrt(np.abs(H_o).max())))
    return rs_g


def assert_eval_scale_equal(orc, trk, lvl, scale, cutoff):
    rs_o = orc.calc_res_scale(lvl, scale, cutoff)
    H_o, b_o = orc.calc_gs_scale(lvl, scale)
    E64 = orc.last_energy_f64()
    rs_g, H_g, b_g, n_g = trk.calcResScale(lvl, scale, cutoff)
    assert rs_g[1] == rs_o[1] and n_g == orc.scale_warped_n()
    if rs_o[1] > 0:
        assert np.float32(rs_g[5]) == np.float32(rs_o[5])
        np.testing.assert_allclose(rs_g[0], E64, rtol=2e-6)
        assert abs(rs_o[0] - E64) <= max(2e-5, rs_o[1] * 2.0 ** -24) * E64
    np.testing.assert_allclose(rs_g[2:5], rs_o[2:5], rtol=FLOAT_RTOL, atol=1e-9)
    if n_g > 0:
        assert abs(H_g - H_o) <= 5e-5 * abs(H_o)
        assert abs(b_g - b_o) <= 5e-5 * max(abs(b_o), 1e-3 * abs(H_o))


@pytest.mark.parametrize("size,template", [("tiny", "dense"), ("small", "dense"), ("small", "sparse"), ("medium", "dense")])
def test_eval_pose_parity_all_levels(ctx, size, template):
    sc = make_scene(size, seed=11, template=template, n0=3000)
    orc, trk = oracle_tracker(sc), hip_tracker(ctx, sc)
    for lvl in range(sc.nl):
        for pose, aff in [(S.IDENTITY_POSE, [0.0, 0.0]), (sc.gt_pose, sc.gt_aff)]:
            for cutoff in (20.0, 5.0):
                assert_eval_pose_equal(orc, trk, lvl, pose, aff, cutoff)


@pytest.mark.parametrize("size", ["tiny", "small", "medium"])
def test_eval_scale_parity_all_levels(ctx, size):
    sc = make_scene(size, seed=12)
    orc, trk = oracle_tracker(sc), hip_tracker(ctx, sc)
    for lvl in range(sc.nl):
        for scale in (1.0, 0.8, 5.0):
            for cutoff in (20.0, 40.0):
                assert_eval_scale_equal(orc, trk, lvl, scale, cutoff)


def test_eval_parity_kitti_full_size(ctx):
    """BASELINE config S1: 1232x368, 5 levels, dense template (446,992 points at level 0)."""
    sc = make_scene("kitti", seed=21)
    orc, trk = oracle_tracker(sc), hip_tracker(ctx, sc)
    assert len(sc.tpl[0][0]) == 1228 * 364
    for lvl in range(sc.nl):
        assert_eval_pose_equal(orc, trk, lvl, S.IDENTITY_POSE, [0.0, 0.0], 20.0)
        assert_eval_scale_equal(orc, trk, lvl, 1.0, 20.0)
    assert_eval_pose_equal(orc, trk, 0, sc.gt_pose, sc.gt_aff, 20.0)


@pytest.mark.parametrize("size,seed", [("kitti6", 0x5EED0000), ("hd6", 0x5EED0001)])
def test_eval_and_track_parity_six_level_configs_full_size(ctx, size, seed):
    """The metric's own configuration (S2: 1248x384, six levels) and BASELINE.json configs[3] at FULL size (S3: 1920x1080,
    six floor-halved levels, 2,057,696 template points at level 0): fused evaluation vs oracle at the finest, a middle and
    the coarsest level (levels 4-5 of S3 have odd sizes: 120x67, 60x33), then the full LM of track and optimize_scale with
    the six-entry iteration table -- same evaluation counts per level as the oracle."""
    sc = make_scene(size, seed=seed, noise=2.0)
    assert sc.nl == 6
    orc, trk = oracle_tracker(sc), hip_tracker(ctx, sc)
    assert len(sc.tpl[0][0]) == (sc.w - 4) * (sc.h - 4) and len(sc.tpl[0][5]) == ((sc.w >> 5) - 4) * ((sc.h >> 5) - 4)
    for lvl in (0, 3, 5):
        assert_eval_pose_equal(orc, trk, lvl, S.IDENTITY_POSE, [0.0, 0.0], 20.0)
        assert_eval_pose_equal(orc, trk, lvl, sc.gt_pose, sc.gt_aff, 20.0)
        assert_eval_scale_equal(orc, trk, lvl, 1.0, 20.0)
    good_o, pose_o, aff_o, last_o, _ = orc.track(S.IDENTITY_POSE, [0, 0], sc.nl - 1)
    good_g, pose_g, aff_g, last_g = trk.trackNewestCoarse(S.IDENTITY_POSE, [0, 0], sc.nl - 1)
    assert good_g == good_o
    np.testing.assert_allclose(pose_g, pose_o, atol=1e-4)
    assert list(ctx.stats().evals)[:sc.nl] == orc.eval_counts()[0][:sc.nl]
    err_o, s_o = orc.optimize_scale(1.0, sc.nl - 1)
    err_g, s_g = trk.optimizeScale(1.0, sc.nl - 1)
    assert abs(s_g - s_o) < 1e-4
    # err = sqrt(E / N) of the last accepted level-0 evaluation.  The reference (and the oracle) accumulate E sequentially in
    # float (quirk Q1), good to n * 2^-24 -- 12 % of E in the worst case at 2 M points -- so the device's value is held
    # against the EXACT sum of the oracle's per-point float terms at the final scale instead (2e-5), and the oracle's own
    # float sum only against its rounding bound
    rs = orc.calc_res_scale(0, s_o, 20.0)
    assert rs[5] < 0.6  # the level ran at the base cut-off (no cut-off repeat)
    err_exact = np.sqrt(orc.last_energy_f64() / rs[1])
    assert abs(err_g - err_exact) < 2e-5 * err_exact
    assert abs(err_o - err_exact) < 0.5 * rs[1] * 2.0 ** -24 * err_exact


@pytest.mark.parametrize("size", ["kitti04", "malaga"])
def test_eval_and_track_parity_other_baseline_shapes(ctx, size):
    """BASELINE.json configs[0] (KITTI 04, 1216x368) and configs[2] (Malaga, 1024x768) working sizes with their own
    intrinsics and stereo baselines: fused evaluation vs oracle at the finest and coarsest level, then the full LM."""
    sc = make_scene(size, seed=23)
    orc, trk = oracle_tracker(sc), hip_tracker(ctx, sc)
    for lvl in (0, sc.nl - 1):
        assert_eval_pose_equal(orc, trk, lvl, sc.gt_pose, sc.gt_aff, 20.0)
        assert_eval_scale_equal(orc, trk, lvl, 1.0, 20.0)
    good_o, pose_o, aff_o, last_o, _ = orc.track(S.IDENTITY_POSE, [0, 0], sc.nl - 1)
    good_g, pose_g, aff_g, last_g = trk.trackNewestCoarse(S.IDENTITY_POSE, [0, 0], sc.nl - 1)
    assert good_g == good_o
    np.testing.assert_allclose(pose_g, pose_o, atol=1e-4)
    assert list(ctx.stats().evals)[:sc.nl] == orc.eval_counts()[0][:sc.nl]
    err_o, s_o = orc.optimize_scale(1.0, sc.nl - 1)
    err_g, s_g = trk.optimizeScale(1.0, sc.nl - 1)
    # err = sqrt(E / N) at level 0: the oracle's E is the reference's sequential float sum (quirk Q1), good to ~n * 2^-24
    assert abs(s_g - s_o) < 1e-4 and abs(err_g - err_o) < 5e-4 * err_o


def test_edge_cases(ctx):
    sc = make_scene("small", seed=13)
    # ragged sizes (not multiples of 4 / 64 / 256), an empty level, and a single point
    for lvl, n in [(0, 1001), (1, 0), (2, 1)]:
        for a in sc.tpl:
            a[lvl] = a[lvl][:n].copy()
    # non-finite texels in the target (the isfinite test, TrackerAndScaler.cpp:791) and non-finite /
    # non-positive inverse depths in the template
    sc.new_p[0][40:44, 100:140, 0] = np.nan
    sc.new_p[0][50, 60:70, 0] = np.inf
    sc.new_p[0] = regrad(sc.new_p[0])  # makeImages zeroes the non-finite gradients around them
    sc.tpl[2][0][5] = np.nan
    sc.tpl[2][0][6] = -0.1
    sc.tpl[2][0][7] = 0.0
    orc, trk = oracle_tracker(sc), hip_tracker(ctx, sc)
    for lvl in range(sc.nl):
        rs = assert_eval_pose_equal(orc, trk, lvl, sc.gt_pose, sc.gt_aff, 20.0)
        assert_eval_scale_equal(orc, trk, lvl, 1.0, 20.0)
        if lvl == 1:
            assert rs[1] == 0 and np.isnan(rs[5])  # 0/0 as in the reference (:849)
    # everything projects out of the image
    far = S.pose_from_Rt(np.eye(3), [50.0, 0, 0])
    rs = assert_eval_pose_equal(orc, trk, 0, far, [0, 0], 20.0)
    assert rs[1] == 0
    # everything saturated
    rs = assert_eval_pose_equal(orc, trk, 0, sc.gt_pose, [0.0, 200.0], 20.0)
    assert rs[5] == 1.0


def test_template_roundtrip_and_scale_depth(ctx):
    sc = make_scene("small", seed=14)
    orc, trk = oracle_tracker(sc), hip_tracker(ctx, sc)
    for lvl in range(sc.nl):
        for a, b in zip(trk.get_template(lvl), [t[lvl] for t in sc.tpl]):
            np.testing.assert_array_equal(a, b)
    trk.scaleCoarseDepthL0(1.7)
    orc.scale_depth(1.7)
    for lvl in range(sc.nl):
        for a, b in zip(trk.get_template(lvl), orc.get_template(lvl)):
            np.testing.assert_array_equal(a, b)  # IEEE division on both sides: bit exact


@pytest.mark.parametrize("size", ["small", "odd"])
def test_device_pyramid_matches_make_images(ctx, size):
    """N1: makeImages on the device is bit-exact with the oracle restatement (also for floor-halved odd sizes, S3)"""
    sc = make_scene(size, seed=15)
    trk = hip_tracker(ctx, sc)
    trk.upload_image(0, sc.new_img, 1.0)
    for lvl in range(sc.nl):
        np.testing.assert_array_equal(trk.get_frame(0, lvl), sc.new_p[lvl])


def test_smallest_pyramid(ctx):
    """the library wants a coarsest level of at least 8 x 8 (a tap fetch spans a 4 x 4 neighbourhood inside the
    2 < u < w - 3 window); at exactly that size -- 16 interior template points, one partly filled wave -- evaluations and the
    whole LM loop agree with the oracle, and a deeper pyramid of the same image is refused"""
    from direct_stereo_slam_amd._lib import DsmError
    from direct_stereo_slam_amd.tracker import TrackerAndScaler

    sc = make_scene("mini4", seed=21)
    assert sc.new_p[-1].shape[:2] == (8, 8) and len(sc.tpl[0][-1]) == 16
    orc, trk = oracle_tracker(sc), hip_tracker(ctx, sc)
    for lvl in range(sc.nl):
        assert_eval_pose_equal(orc, trk, lvl, sc.gt_pose, sc.gt_aff, 20.0)
        assert_eval_scale_equal(orc, trk, lvl, 1.0, 20.0)
    good_o, pose_o, aff_o, last_o, _ = orc.track(S.IDENTITY_POSE, [0.0, 0.0], sc.nl - 1)
    good_g, pose_g, aff_g, last_g = trk.trackNewestCoarse(S.IDENTITY_POSE, [0.0, 0.0], sc.nl - 1)
    assert good_g == good_o
    np.testing.assert_allclose(pose_g, pose_o, atol=1e-4)
    assert list(ctx.stats().evals)[:sc.nl] == orc.eval_counts()[0][:sc.nl]
    with pytest.raises(DsmError, match="too small"):
        TrackerAndScaler(ctx, sc.w, sc.h, sc.nl + 1, sc.T, sc.K)


def test_upload_frame_keeps_intensities_and_checks_gradients(ctx):
    """The device stores channel 0 of the reference's (I, dx, dy) texels only and forms the gradients where they are used:
    dsm_tracker_upload_frame therefore insists that channels 1 and 2 are makeImages' central differences of channel 0
    (rows 1 .. h-2; the first and last row are left unset by makeImages and never read), and dsm_tracker_get_frame
    hands the full texels back"""
    from direct_stereo_slam_amd._lib import DsmError

    sc = make_scene("small", seed=16)
    trk = hip_tracker(ctx, sc)
    for ch in (1, 2):
        bad = [p.copy() for p in sc.new_p]
        bad[1][5, 7, ch] = np.nextafter(bad[1][5, 7, ch], np.float32(np.inf))  # one ulp off, one texel
        with pytest.raises(DsmError, match="central differences"):
            trk.upload_frame(0, bad)
    with pytest.raises(DsmError):  # the slot holds no frame after a refused hand-over
        trk.calcResPose(0, sc.gt_pose, sc.gt_aff, 20.0)
    ok = [p.copy() for p in sc.new_p]
    ok[0][0, :, 1:] = 7.0
    ok[0][-1, :, 1:] = -3.0
    trk.upload_frame(0, ok)
    for lvl in range(sc.nl):
        np.testing.assert_array_equal(trk.get_frame(0, lvl), sc.new_p[lvl])


@pytest.mark.parametrize("size,template,seed", [("tiny", "dense", 1), ("small", "dense", 2), ("small", "sparse", 3), ("medium", "dense", 4), ("odd", "dense", 5)])
def test_track_parity(ctx, size, template, seed):
    sc = make_scene(size, seed=seed, template=template, n0=4000)
    orc, trk = oracle_tracker(sc), hip_tracker(ctx, sc)
    good_o, pose_o, aff_o, last_o, flow_o = orc.track(S.IDENTITY_POSE, [0, 0], sc.nl - 1)
    good_g, pose_g, aff_g, last_g = trk.trackNewestCoarse(S.IDENTITY_POSE, [0, 0], sc.nl - 1)
    assert good_g == good_o
    np.testing.assert_allclose(pose_g, pose_o, rtol=0, atol=1e-4 * max(1.0, np.abs(pose_o[4:]).max()))
    np.testing.assert_allclose(aff_g, aff_o, rtol=1e-3, atol=1e-3)
    np.testing.assert_allclose(last_g[:sc.nl], last_o[:sc.nl], rtol=1e-4)
    assert np.all(np.isnan(last_g[sc.nl:]))
    np.testing.assert_allclose(trk.lastFlowIndicators, flow_o, rtol=1e-3)
    # and both are at the ground truth
    np.testing.assert_allclose(pose_g[4:], sc.gt_pose[4:], atol=5e-3)
    # same LM trajectory: identical evaluation counts per level
    st = ctx.stats()
    assert list(st.evals)[:sc.nl] == orc.eval_counts()[0][:sc.nl]


def test_track_abort_and_affine_checks(ctx):
    sc = make_scene("small", seed=5)
    orc, trk = oracle_tracker(sc), hip_tracker(ctx, sc)
    # minResForAbort so small that the coarsest level aborts (:598): outputs untouched
    mr = np.full(6, 1e-3)
    good_o, pose_o, aff_o, last_o, _ = orc.track(S.IDENTITY_POSE, [0, 0], sc.nl - 1, mr)
    good_g, pose_g, aff_g, last_g = trk.trackNewestCoarse(S.IDENTITY_POSE, [0, 0], sc.nl - 1, mr)
    assert not good_o and not good_g
    np.testing.assert_array_equal(pose_g, S.IDENTITY_POSE)
    np.testing.assert_allclose(last_g[sc.nl - 1], last_o[sc.nl - 1], rtol=1e-4)
    assert np.isnan(last_g[0]) and np.isnan(last_o[0])
    # implausible affine result (:624-626): brightness offset beyond 200
    sc2 = make_scene("small", seed=6, b=240.0)
    orc2, trk2 = oracle_tracker(sc2), hip_tracker(ctx, sc2)
    good_o, pose_o, aff_o, _, _ = orc2.track(S.IDENTITY_POSE, [0, 0], sc2.nl - 1)
    good_g, pose_g, aff_g, _ = trk2.trackNewestCoarse(S.IDENTITY_POSE, [0, 0], sc2.nl - 1)
    assert good_g == good_o
    np.testing.assert_allclose(pose_g, pose_o, atol=2e-4)


# The photometric model of a REAL sequence: every keyframe carries a nonzero affine brightness (a, b) and the two
# frames have different exposure times.  AffLight::fromToVecExposure(lastRef->ab_exposure, new_frame_->ab_exposure, lastRef_aff_g2l,
# aff_g2l) (TrackerAndScaler.cpp:717-720, :647-649), J6 = a (b0 - refColor) (:673-676) with b0 = lastRef_aff_g2l.b (:646), the
# "either exposure 0 => both 1" rule of fromToVecExposure, and the plausibility checks on the RELATIVE affine at the end (:615-626).
AFFINE_CASES = {
    "dark_keyframe_longer_exposure": dict(ref_aff=(-0.3, 12.0), ref_exposure=0.8, new_exposure=1.3, new_aff=(-0.25, 20.0)),
    "bright_keyframe_shorter_exposure": dict(ref_aff=(0.15, -6.0), ref_exposure=1.3, new_exposure=0.8, new_aff=(0.2, -2.0)),
    "zero_reference_exposure": dict(ref_aff=(-0.3, 12.0), ref_exposure=0.0, new_exposure=1.3, new_aff=(-0.25, 20.0)),
    "zero_new_exposure": dict(ref_aff=(-0.3, 12.0), ref_exposure=0.8, new_exposure=0.0, new_aff=(-0.25, 20.0)),
    "relief_family": dict(ref_aff=(-0.3, 12.0), ref_exposure=0.8, new_exposure=1.3, new_aff=(-0.25, 20.0), family="relief"),
}


def assert_affine_row(orc, trk, lvl, pose, aff, cutoff):
    """row / column 6 of H and b[6] -- the only entries J6 = a (b0 - refColor) reaches -- each against ITS OWN scale (the whole-matrix bar
    of assert_eval_pose_equal is relative to max |H|, which the SCALE_B = 1000 entry H[7][7] dominates)"""
    rs_o = orc.calc_res_pose(lvl, pose, aff, cutoff)
    H_o, b_o = orc.calc_gs_pose(lvl, pose, aff)
    rs_g, H_g, b_g, n_g = trk.calcResPose(lvl, pose, aff, cutoff)
    if n_g == 0:
        return
    assert H_o[6, 6] > 0
    for c in range(8):  # |H[6][c]| <= sqrt(H[6][6] H[c][c]) (Cauchy-Schwarz on the weighted sums): the natural scale of the entry
        tol = FLOAT_RTOL * np.sqrt(H_o[6, 6] * H_o[c, c])
        assert abs(H_g[6, c] - H_o[6, c]) <= tol and abs(H_g[c, 6] - H_o[c, 6]) <= tol, (lvl, c, H_g[6, c], H_o[6, c])
    assert abs(b_g[6] - b_o[6]) <= FLOAT_RTOL * max(abs(b_o[6]), np.sqrt(H_o[6, 6] * rs_o[0] / max(rs_o[1], 1.0))), (lvl, b_g[6], b_o[6])


@pytest.mark.parametrize("case", sorted(AFFINE_CASES))
def test_affine_and_exposure_branch_all_levels_track_and_stream(ctx, case):
    from direct_stereo_slam_amd.tracker import Stream

    sc = make_affine_scene("small", seed=31, **AFFINE_CASES[case])
    orc, trk = oracle_tracker(sc), hip_tracker(ctx, sc)
    # ---- fused evaluations, every level: the keyframe's own affine (what FrontEnd hands over as the guess), the truth, and (0, 0) ----
    for lvl in range(sc.nl):
        for pose in (S.IDENTITY_POSE, sc.gt_pose):
            for aff in (list(sc.ref_aff), list(sc.gt_aff), [0.0, 0.0]):
                for cutoff in (20.0, 5.0):
                    assert_eval_pose_equal(orc, trk, lvl, pose, aff, cutoff)
                assert_affine_row(orc, trk, lvl, pose, aff, 20.0)
    # the branch really is exercised: the same images and template under the photometry every other test uses -- reference affine (0, 0),
    # exposures 1 -- give another residual and another affine row
    import copy

    plain = copy.copy(sc)
    plain.ref_aff, plain.ref_exposure, plain.new_exposure = (0.0, 0.0), 1.0, 1.0
    orc_plain = oracle_tracker(plain)
    rs_p, rs_a = orc_plain.calc_res_pose(0, sc.gt_pose, list(sc.gt_aff), 20.0), orc.calc_res_pose(0, sc.gt_pose, list(sc.gt_aff), 20.0)
    H_p, H_a = orc_plain.calc_gs_pose(0, sc.gt_pose, list(sc.gt_aff))[0], orc.calc_gs_pose(0, sc.gt_pose, list(sc.gt_aff))[0]
    assert abs(rs_p[0] - rs_a[0]) > 0.05 * rs_a[0] and not np.allclose(H_p[6], H_a[6], rtol=1e-2)
    # ---- the LM loop ----
    good_o, pose_o, aff_o, last_o, flow_o = orc.track(S.IDENTITY_POSE, list(sc.ref_aff), sc.nl - 1)
    good_g, pose_g, aff_g, last_g = trk.trackNewestCoarse(S.IDENTITY_POSE, list(sc.ref_aff), sc.nl - 1)
    assert good_g == good_o and good_o
    np.testing.assert_allclose(pose_g, pose_o, rtol=0, atol=1e-4)
    np.testing.assert_allclose(aff_g, aff_o, rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(last_g[:sc.nl], last_o[:sc.nl], rtol=1e-4)
    np.testing.assert_allclose(trk.lastFlowIndicators, flow_o, rtol=1e-3)
    np.testing.assert_allclose(pose_g[4:], sc.gt_pose[4:], atol=5e-3)  # and it is the scene's motion
    assert list(ctx.stats().evals)[:sc.nl] == orc.eval_counts()[0][:sc.nl]
    # ---- the tick engine (what bench.py's step runs): the same bits as the direct call ----
    st = Stream(ctx, 2, 1)
    tk = st.submit_track([trk], [S.IDENTITY_POSE], np.array([sc.ref_aff]), sc.nl - 1)[0]
    st.drain()
    got = {r.ticket: r for r in st.results()}
    st.close()
    assert np.array_equal(np.array(got[tk].pose), pose_g) and np.array_equal(np.array(got[tk].aff), aff_g) and bool(got[tk].good) == bool(good_g)
    assert list(got[tk].evals)[:sc.nl] == orc.eval_counts()[0][:sc.nl]


def test_implausible_relative_affine_fails_the_track_like_the_reference(ctx):
    """:615-626: |log(relative a)| > 1.5 -- here an exposure ratio of 6.5 -- returns false AFTER lastToNew_out / aff_g2l_out were written
    (:612-613); the pose is the tracked one"""
    sc = make_affine_scene("small", seed=31, ref_aff=(-0.3, 12.0), ref_exposure=0.2, new_exposure=1.3, new_aff=(-0.25, 20.0))
    orc, trk = oracle_tracker(sc), hip_tracker(ctx, sc)
    good_o, pose_o, aff_o, last_o, _ = orc.track(S.IDENTITY_POSE, list(sc.ref_aff), sc.nl - 1)
    good_g, pose_g, aff_g, last_g = trk.trackNewestCoarse(S.IDENTITY_POSE, list(sc.ref_aff), sc.nl - 1)
    assert not good_o and not good_g
    np.testing.assert_allclose(pose_g, pose_o, rtol=0, atol=1e-4)
    np.testing.assert_allclose(aff_g, aff_o, rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(pose_g[4:], sc.gt_pose[4:], atol=5e-3)
    assert list(ctx.stats().evals)[:sc.nl] == orc.eval_counts()[0][:sc.nl]


@pytest.mark.parametrize("modes", [(-1.0, -1.0), (0.0, -1.0), (-1.0, 0.0)])
def test_track_fixed_affine_modes(ctx, modes):
    """the 6/7-dim sub-solves of TrackerAndScaler.cpp:511-534"""
    sc = make_scene("small", seed=8, a=0.0, b=0.0)
    po, pg = O.default_params(), None
    po.affine_opt_mode_a, po.affine_opt_mode_b = modes
    from direct_stereo_slam_amd.tracker import default_params
    pg = default_params()
    pg.affine_opt_mode_a, pg.affine_opt_mode_b = modes
    orc, trk = oracle_tracker(sc, po), hip_tracker(ctx, sc, pg)
    good_o, pose_o, aff_o, last_o, _ = orc.track(S.IDENTITY_POSE, [0, 0], sc.nl - 1)
    good_g, pose_g, aff_g, last_g = trk.trackNewestCoarse(S.IDENTITY_POSE, [0, 0], sc.nl - 1)
    assert good_g == good_o
    np.testing.assert_allclose(pose_g, pose_o, atol=1e-4)
    np.testing.assert_allclose(aff_g, aff_o, rtol=1e-3, atol=1e-3)
    if modes[0] < 0:
        assert aff_g[0] == 0
    if modes[1] < 0:
        assert aff_g[1] == 0


@pytest.mark.parametrize("s0", [0.1, 1.0, 5.0, 10.0, 50.0])
def test_optimize_scale_parity(ctx, s0):
    """the initial guesses FrontEnd::optimizeScale tries (FrontEnd.cpp:995)"""
    sc = make_scene("small", seed=9, idepth_scale=1.1)
    orc, trk = oracle_tracker(sc), hip_tracker(ctx, sc)
    err_o, s_o = orc.optimize_scale(s0, sc.nl - 1)
    err_g, s_g = trk.optimizeScale(s0, sc.nl - 1)
    # far-off initial guesses end in flat, ill-conditioned regions (the caller rejects them by their
    # error, FrontEnd.cpp:999-1002): there only the error is compared tightly
    converged = abs(s_o - 1.1) < 0.05
    assert abs(s_g - s_o) <= (1e-4 if converged else 2e-3) * abs(s_o)
    assert abs(err_g - err_o) <= 1e-3 * abs(err_o)
    if converged:
        assert list(ctx.stats().evals)[:sc.nl] == orc.eval_counts()[0][:sc.nl]


def test_cutoff_repeat_and_level_repeat(ctx):
    """levelCutoffRepeat doubling (:477-485) and the single level repeat (:601-604): start far
    from the optimum with a large brightness offset so that > 60 % of the residuals saturate."""
    sc = make_scene("small", seed=10, b=60.0)
    orc, trk = oracle_tracker(sc), hip_tracker(ctx, sc)
    rs = orc.calc_res_pose(sc.nl - 1, S.IDENTITY_POSE, [0, 0], 20.0)
    assert rs[5] > 0.6, "scene does not trigger the cut-off doubling"
    good_o, pose_o, aff_o, last_o, _ = orc.track(S.IDENTITY_POSE, [0, 0], sc.nl - 1)
    good_g, pose_g, aff_g, last_g = trk.trackNewestCoarse(S.IDENTITY_POSE, [0, 0], sc.nl - 1)
    assert good_g == good_o
    np.testing.assert_allclose(pose_g, pose_o, atol=2e-4)
    np.testing.assert_allclose(aff_g, aff_o, rtol=2e-3, atol=2e-3)
    assert list(ctx.stats().evals)[:sc.nl] == orc.eval_counts()[0][:sc.nl]


def test_batch_equals_single_and_is_deterministic(ctx):
    scs = [make_scene("small", seed=30 + i, template="dense" if i % 2 == 0 else "sparse", n0=3000) for i in range(5)]
    trks = [hip_tracker(ctx, sc) for sc in scs]
    singles = [t.trackNewestCoarse(S.IDENTITY_POSE, [0, 0], 2) for t in trks]
    poses0 = np.tile(S.IDENTITY_POSE, (5, 1))
    r1 = ctx.track_batch(trks, poses0, np.zeros((5, 2)), 2)
    r2 = ctx.track_batch(trks, poses0, np.zeros((5, 2)), 2)
    for i in range(5):
        assert r1[0][i] == singles[i][0]
        np.testing.assert_array_equal(r1[1][i], singles[i][1])  # bit identical: fixed reduction order
        np.testing.assert_array_equal(r1[2][i], singles[i][2])
    np.testing.assert_array_equal(r1[1], r2[1])
    np.testing.assert_array_equal(r1[3], r2[3])
    e1, s1 = ctx.optimize_scale_batch(trks, np.ones(5), 2)
    for i in range(5):
        e, s = trks[i].optimizeScale(1.0, 2)
        assert e == e1[i] and s == s1[i]


def test_launch_schedule_does_not_change_results(ctx):
    from direct_stereo_slam_amd.tracker import default_params

    sc = make_scene("small", seed=40)
    out = []
    for adaptive in (0, 1, 1, 1):  # worst-case single pass, then adaptive passes with a learning schedule
        p = default_params()
        p.adaptive_schedule = adaptive
        trk = hip_tracker(ctx, sc, p)
        out.append(trk.trackNewestCoarse(S.IDENTITY_POSE, [0, 0], sc.nl - 1))
    for o in out[1:]:
        np.testing.assert_array_equal(o[1], out[0][1])
        np.testing.assert_array_equal(o[3], out[0][3])


def test_track_parity_kitti_full_size(ctx):
    sc = make_scene("kitti", seed=22)
    orc, trk = oracle_tracker(sc), hip_tracker(ctx, sc)
    good_o, pose_o, aff_o, last_o, flow_o = orc.track(S.IDENTITY_POSE, [0, 0], sc.nl - 1)
    good_g, pose_g, aff_g, last_g = trk.trackNewestCoarse(S.IDENTITY_POSE, [0, 0], sc.nl - 1)
    assert good_g and good_o
    np.testing.assert_allclose(pose_g, pose_o, atol=1e-4)
    np.testing.assert_allclose(last_g[:5], last_o[:5], rtol=1e-4)
    np.testing.assert_allclose(pose_g[4:], sc.gt_pose[4:], atol=3e-3)
    err_o, s_o = orc.optimize_scale(1.0, sc.nl - 1)
    err_g, s_g = trk.optimizeScale(1.0, sc.nl - 1)
    assert abs(s_g - s_o) < 1e-4 and abs(err_g - err_o) < 1e-4 * err_o


def test_six_level_extension(ctx):
    """S2 of SURVEY.md section 8d: 1248x384 padded size with a 6-level pyramid (max_iterations[5])"""
    w, h, nl = 1248 // 4, 384 // 4, 4  # quarter-size stand-in keeps every level >= 39x12
    assert (w >> (nl - 1)) >= 8
    sc = make_scene("small", seed=41)
    # full S2 geometry is exercised by bench.py; here only the nlevels=6 plumbing on a small frame
    from direct_stereo_slam_amd.tracker import TrackerAndScaler
    K = S.level_K(S.kitti_K_work(), 0)
    w6, h6 = 1248, 384
    scene = S.PlaneScene(seed=1)
    rng = np.random.default_rng(0)
    ref = scene.render(K, w6, h6, noise=1.0, rng=rng)
    R, t = S.random_motion(rng)
    new = scene.render(K, w6, h6, R, t, noise=1.0, rng=rng)
    ref_p, new_p = O.make_images(ref, 6), O.make_images(new, 6)
    tpl = S.dense_template(scene, K, w6, h6, 6, ref_p)
    orc = O.OracleTracker(w6, h6, 6, S.KITTI_T_STEREO, K)
    orc.make_k(*K); orc.set_ref(0, 0, 0, 1.0, *tpl); orc.set_frame(0, new_p, 1.0)
    trk = TrackerAndScaler(ctx, w6, h6, 6, S.KITTI_T_STEREO, K)
    trk.makeK(*K); trk.setCoarseTrackingRef(0, (0, 0), 1.0, *tpl); trk.upload_frame(0, new_p, 1.0)
    go, po, ao, lo, _ = orc.track(S.IDENTITY_POSE, [0, 0], 5)
    gg, pg, ag, lg = trk.trackNewestCoarse(S.IDENTITY_POSE, [0, 0], 5)
    assert gg == go
    np.testing.assert_allclose(pg, po, atol=1e-4)
    np.testing.assert_allclose(lg, lo, rtol=1e-4)


def test_call_order_errors(ctx):
    from direct_stereo_slam_amd._lib import DsmError
    from direct_stereo_slam_amd.tracker import TrackerAndScaler

    sc = make_scene("tiny", seed=1)
    trk = TrackerAndScaler(ctx, sc.w, sc.h, sc.nl, sc.T, sc.K)
    with pytest.raises(DsmError):
        trk.trackNewestCoarse(S.IDENTITY_POSE, [0, 0], 1)  # before makeK / setCoarseTrackingRef
    trk.makeK(*sc.K)
    trk.setCoarseTrackingRef(0, (0, 0), 1.0, *sc.tpl)
    with pytest.raises(DsmError):
        trk.optimizeScale(1.0, 1)  # right frame missing
    trk.upload_frame(0, sc.new_p)
    with pytest.raises(DsmError):
        trk.trackNewestCoarse(S.IDENTITY_POSE, [0, 0], sc.nl)  # coarsestLvl >= pyrLevelsUsed (:457)


@pytest.mark.parametrize("geometry,n_cut,expect", [(1, 65535, (256, 4, 64)), (0, 4095, (256, 16, 1))])
def test_sparse_template_just_below_a_chunking_threshold(ctx, geometry, n_cut, expect):
    """points-per-thread grows with n, so under the latency table the chunk count is not monotone in n: n = 65535 uses 4 points
    per thread and 64 chunks although the level holds up to 113k points (8 per thread, 56 chunks).  The partial-sum workspace must be
    sized for the worst n of either table, not for the largest.  Under the throughput table a level of at most 4096 points is ONE chunk
    (round 6): n = 4095 is one chunk of 16 points per thread, n = 4097 two."""
    from direct_stereo_slam_amd.tracker import default_params

    sc = make_scene("medium", seed=50)
    assert len(sc.tpl[0][0]) > n_cut
    for a in sc.tpl:
        a[0] = a[0][:n_cut].copy()
    prm = default_params()
    assert prm.chunk_geometry == 0  # the library default: the throughput table
    prm.chunk_geometry = geometry
    orc, trk = oracle_tracker(sc), hip_tracker(ctx, sc, prm)
    assert trk.reduction_geometry(0, n_cut) == expect
    if geometry == 1:
        assert trk.reduction_geometry(0, n_cut + 1)[2] < expect[2]
    else:  # the metric's small levels: 280 / 1480 / 6688 points (levels 5 / 4 / 3 of 1248 x 384)
        assert [trk.reduction_geometry(0, n)[1:] for n in (280, 1480, 6688, 4096, 4097)] == [(2, 1), (8, 1), (16, 2), (16, 1), (16, 2)]
    assert_eval_pose_equal(orc, trk, 0, sc.gt_pose, sc.gt_aff, 20.0)
    good_o, pose_o, _, _, _ = orc.track(S.IDENTITY_POSE, [0, 0], sc.nl - 1)
    good_g, pose_g, _, _ = trk.trackNewestCoarse(S.IDENTITY_POSE, [0, 0], sc.nl - 1)
    assert good_g == good_o
    np.testing.assert_allclose(pose_g, pose_o, atol=1e-4)


@pytest.mark.gpu
def test_chunk_geometries_agree(ctx):
    """dsm_params.chunk_geometry picks the summation tree only: both tables give the oracle's result within the float-sum tolerance,
    equal integer outputs, and a batch of the two kinds of tracker mixed gives each tracker what it gets alone."""
    from direct_stereo_slam_amd.tracker import default_params

    scs = [make_scene("medium", seed=60 + i) for i in range(4)]
    prm = [default_params() for _ in range(2)]
    prm[1].chunk_geometry = 1
    trks = [hip_tracker(ctx, sc, prm[i & 1]) for i, sc in enumerate(scs)]
    alone = [t.trackNewestCoarse(S.IDENTITY_POSE, [0, 0], scs[0].nl - 1) for t in trks]
    good, poses = ctx.track_batch(trks, np.tile(S.IDENTITY_POSE, (4, 1)), np.zeros((4, 2)), scs[0].nl - 1)[:2]
    for i, (sc, t) in enumerate(zip(scs, trks)):
        assert bool(good[i]) == bool(alone[i][0])
        np.testing.assert_array_equal(poses[i], alone[i][1])
        good_o, pose_o, _, _, _ = oracle_tracker(sc).track(S.IDENTITY_POSE, [0, 0], sc.nl - 1)
        assert bool(good[i]) == good_o
        np.testing.assert_allclose(poses[i], pose_o, atol=1e-4)
    # one scene under both tables: single evaluations agree in the integer outputs exactly
    a, b = hip_tracker(ctx, scs[0], prm[0]), hip_tracker(ctx, scs[0], prm[1])
    p2 = default_params()
    p2.chunk_geometry = 2  # the latency table above 4096 points, one chunk below (round 6: one frame in flight with chained small levels)
    c = hip_tracker(ctx, scs[0], p2)
    differ = 0
    for lvl in range(scs[0].nl):
        (rsa, Ha, ba, na), (rsb, Hb, bb, nb), (rsc, Hc, bc, nc) = (t.calcResPose(lvl, scs[0].gt_pose, scs[0].gt_aff, 20.0) for t in (a, b, c))
        assert rsa[1] == rsb[1] and rsa[5] == rsb[5] and na == nb  # numTermsInE, saturated share, warped count
        assert rsa[1] == rsc[1] and rsa[5] == rsc[5] and na == nc
        np.testing.assert_allclose(rsa[0], rsb[0], rtol=1e-5)
        np.testing.assert_allclose(rsa[0], rsc[0], rtol=1e-5)
        np.testing.assert_allclose(Ha, Hb, rtol=0, atol=1e-5 * np.abs(Ha).max())
        np.testing.assert_allclose(Ha, Hc, rtol=0, atol=1e-5 * np.abs(Ha).max())
        n_l = len(scs[0].tpl[lvl][0])
        differ += a.reduction_geometry(lvl, n_l)[2] != b.reduction_geometry(lvl, n_l)[2]
        assert c.reduction_geometry(lvl, n_l)[2] == (a if n_l <= 4096 else b).reduction_geometry(lvl, n_l)[2]
    assert differ > 0  # (the tables do cut this scene's levels differently)


def test_stream_groups_do_not_change_results(ctx):
    scs = [make_scene("small", seed=90 + i) for i in range(7)]
    trks = [hip_tracker(ctx, sc) for sc in scs]
    poses0 = np.tile(S.IDENTITY_POSE, (7, 1))
    ref = ctx.track_batch(trks, poses0, np.zeros((7, 2)), 2)
    try:
        for ns in (2, 3, 16):
            ctx.set_streams(ns)
            got = ctx.track_batch(trks, poses0, np.zeros((7, 2)), 2)
            for a, b in zip(ref, got):
                np.testing.assert_array_equal(a, b)
            e1, s1 = ctx.optimize_scale_batch(trks, np.ones(7), 2)
            ctx.set_streams(1)
            e0, s0 = ctx.optimize_scale_batch(trks, np.ones(7), 2)
            np.testing.assert_array_equal(e0, e1)
            np.testing.assert_array_equal(s0, s1)
    finally:
        ctx.set_streams(1)


@pytest.mark.parametrize("size,template", [("small", "dense"), ("medium", "dense"), ("medium", "sparse"), ("kitti", "dense")])
def test_retired_persistent_coarse_value_changes_nothing(ctx, size, template):
    """persistent_coarse > 0 selected a retired small-level form: the value is still accepted and runs the launch-per-step path,
    so every output must be bit-identical to persistent_coarse = 0, the evaluation counts equal and no small-level kernel launched."""
    from direct_stereo_slam_amd.tracker import default_params

    sc = make_scene(size, seed=60, template=template, n0=12000)
    out, evals, coarse = [], [], []
    for max_pts in (0, 32768, 8192, 2000):
        p = default_params()
        p.persistent_coarse = max_pts
        trk = hip_tracker(ctx, sc, p)
        r = trk.trackNewestCoarse(S.IDENTITY_POSE, [0, 0], sc.nl - 1)
        st = ctx.stats()
        evals.append(list(st.evals))
        coarse.append(st.coarse_launches)
        s = trk.optimizeScale(1.3, sc.nl - 1)
        evals.append(list(ctx.stats().evals))
        out.append((r, s))
    assert coarse == [0, 0, 0, 0]
    (r0, s0) = out[0]
    for k in range(1, 4):
        assert evals[2 * k] == evals[0] and evals[2 * k + 1] == evals[1]
        r1, s1 = out[k]
        assert r0[0] == r1[0]
        for a, b in zip(r0[1:], r1[1:]):
            np.testing.assert_array_equal(a, b)
        assert s0 == s1


@pytest.mark.parametrize("size,template", [("small", "dense"), ("medium", "dense"), ("medium", "sparse"), ("kitti", "dense")])
@pytest.mark.parametrize("geometry", [0, 2])
def test_chain_kernel_is_bit_identical(ctx, size, template, geometry):
    """persistent_coarse < 0: the levels whose evaluation is ONE chunk run their LM loop in one launch per problem (chain_kernel: the
    tick engine's chain as a launch of its own; TrackerAndScaler.cpp:505-593 in place) and the launch-per-step schedule takes over at the
    first level of several chunks.  Same chunk, partial and reduction order: every output bit-identical to the launch form under the
    same chunk table, the evaluation counts equal -- for the throughput table and for table 2 (latency table above 4096 points, one chunk
    below: what the replay adaptors select; its single evaluations against the other tables: test_chunk_geometries_agree)."""
    from direct_stereo_slam_amd.tracker import default_params

    sc = make_scene(size, seed=63, template=template, n0=12000)
    out, evals, coarse = [], [], []
    for chain in (0, -1):
        p = default_params()
        p.chunk_geometry = geometry
        p.persistent_coarse = chain
        trk = hip_tracker(ctx, sc, p)
        r = trk.trackNewestCoarse(S.IDENTITY_POSE, [0, 0], sc.nl - 1)
        st = ctx.stats()
        evals.append(list(st.evals))
        coarse.append(st.coarse_launches)
        s = trk.optimizeScale(1.3, sc.nl - 1)
        evals.append(list(ctx.stats().evals))
        out.append((r, s))
        # a batch of several problems through the same path (stream groups, the companion segment of track + scale)
        if chain:
            trks = [hip_tracker(ctx, make_scene(size, seed=64 + i, template=template, n0=12000), p) for i in range(3)]
            p0 = default_params()
            p0.chunk_geometry = geometry
            refs = [hip_tracker(ctx, make_scene(size, seed=64 + i, template=template, n0=12000), p0) for i in range(3)]
            a = ctx.track_and_scale_batch(trks, np.tile(S.IDENTITY_POSE, (3, 1)), np.zeros((3, 2)), sc.nl - 1, trks[:2], np.array([1.0, 1.2], np.float32))
            b = ctx.track_and_scale_batch(refs, np.tile(S.IDENTITY_POSE, (3, 1)), np.zeros((3, 2)), sc.nl - 1, refs[:2], np.array([1.0, 1.2], np.float32))
            for x, y in zip(a, b):
                np.testing.assert_array_equal(np.asarray(x), np.asarray(y))
    n_coarsest = len(sc.tpl[0][sc.nl - 1])  # (tpl = [pc_u, pc_v, pc_idepth, pc_color], each a list over the levels)
    assert coarse == [0, 1 if n_coarsest <= 4096 else 0], (coarse, n_coarsest)
    (r0, s0), (r1, s1) = out
    assert evals[2] == evals[0] and evals[3] == evals[1]
    assert r0[0] == r1[0]
    for a, b in zip(r0[1:], r1[1:]):
        np.testing.assert_array_equal(a, b)
    assert s0 == s1


@pytest.mark.parametrize("size,template", [("small", "dense"), ("medium", "sparse"), ("kitti", "dense")])
def test_fused_lm_step_is_bit_identical(ctx, size, template):
    """fuse_lm: at levels >= 1 the last-arriving workgroup of the eval kernel performs the LM step; it
    reads the same partials in the same order as the separate LM kernel: bit-identical results."""
    from direct_stereo_slam_amd.tracker import default_params

    sc = make_scene(size, seed=61, template=template, n0=12000)
    assert default_params().fuse_lm == 1
    out = []
    for fuse in (0, 2, 1):
        p = default_params()
        p.fuse_lm = fuse
        trk = hip_tracker(ctx, sc, p)
        r = trk.trackNewestCoarse(S.IDENTITY_POSE, [0, 0], sc.nl - 1)
        ev = list(ctx.stats().evals)
        s = trk.optimizeScale(1.3, sc.nl - 1)
        out.append((r, ev, s, list(ctx.stats().evals)))
    for o in out[1:]:
        assert o[1] == out[0][1] and o[3] == out[0][3] and o[2] == out[0][2]
        assert o[0][0] == out[0][0][0]
        for a, b in zip(o[0][1:], out[0][0][1:]):
            np.testing.assert_array_equal(a, b)


def test_fused_lm_step_batched(ctx):
    """the fused eval+LM kernels with many problems in one launch (fuse_lm = 2 forces them for any batch
    size) and two stream groups: bit-identical to the two-kernel form"""
    from direct_stereo_slam_amd.tracker import default_params

    scs = [make_scene("small", seed=70 + i, template="dense" if i % 3 else "sparse", n0=2500) for i in range(12)]
    poses0 = np.tile(S.IDENTITY_POSE, (12, 1))
    out = []
    try:
        for fuse, ns in ((0, 1), (2, 1), (2, 2)):
            p = default_params()
            p.fuse_lm = fuse
            trks = [hip_tracker(ctx, sc, p) for sc in scs]
            ctx.set_streams(ns)
            r = ctx.track_batch(trks, poses0, np.zeros((12, 2)), 2)
            e = ctx.optimize_scale_batch(trks, np.ones(12), 2)
            out.append((r, e))
    finally:
        ctx.set_streams(1)
    for r, e in out[1:]:
        for a, b in zip(r, out[0][0]):
            np.testing.assert_array_equal(a, b)
        for a, b in zip(e, out[0][1]):
            np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("size,template", [("tiny", "dense"), ("small", "dense"), ("medium", "sparse"), ("kitti", "dense")])
def test_work_queue_kernel_is_bit_identical(ctx, size, template):
    """work_queue: the whole call in one launch of persistent workgroups pulling (problem, chunk) items; same chunks,
    same partials, same reduction order -> bit-identical results, evaluation counts included.  Also with an empty
    pyramid level (no template points there: the level still needs its LM step)."""
    from direct_stereo_slam_amd.tracker import default_params

    sc = make_scene(size, seed=63, template=template, n0=12000)
    assert default_params().work_queue == 1
    out = []
    for queue in (0, 2, 2):
        p = default_params()
        p.work_queue = queue
        trk = hip_tracker(ctx, sc, p)
        r = trk.trackNewestCoarse(S.IDENTITY_POSE, [0, 0], sc.nl - 1)
        st = ctx.stats()
        ev, qb = list(st.evals), st.queue_blocks
        s = trk.optimizeScale(1.3, sc.nl - 1)
        out.append((r, ev, s, list(ctx.stats().evals), qb))
    assert out[0][4] == 0 and out[1][4] > 0
    for o in out[1:]:
        assert o[1] == out[0][1] and o[3] == out[0][3] and o[2] == out[0][2]
        assert o[0][0] == out[0][0][0]
        for a, b in zip(o[0][1:], out[0][0][1:]):
            np.testing.assert_array_equal(a, b)


def test_work_queue_kernel_batched_with_empty_level(ctx):
    from direct_stereo_slam_amd.tracker import default_params

    scs = [make_scene("small", seed=170 + i, template="dense" if i % 3 else "sparse", n0=2500) for i in range(40)]
    for sc in scs[::7]:  # a few problems without any template point at the coarsest level
        sc.tpl = [[a[l] if l < sc.nl - 1 else a[l][:0] for l in range(sc.nl)] for a in sc.tpl]
    poses0 = np.tile(S.IDENTITY_POSE, (40, 1))
    out = []
    for queue in (0, 1, 2):  # 1 = automatic rule (batches >= 32)
        p = default_params()
        p.work_queue = queue
        trks = [hip_tracker(ctx, sc, p) for sc in scs]
        r = ctx.track_batch(trks, poses0, np.zeros((40, 2)), 2)
        qb = ctx.stats().queue_blocks
        e = ctx.optimize_scale_batch(trks, np.ones(40), 2)
        out.append((r, e, qb))
    assert out[0][2] == 0 and out[1][2] > 0 and out[2][2] > 0
    for r, e, _ in out[1:]:
        for a, b in zip(r, out[0][0]):
            np.testing.assert_array_equal(a, b)
        for a, b in zip(e, out[0][1]):
            np.testing.assert_array_equal(a, b)


def test_upload_image_from_pinned_memory(ctx):
    """dsm_host_alloc: a pinned caller buffer is handed over by DMA; same pyramid as from pageable memory, and the buffer may be
    overwritten as soon as upload_image has returned (the call waits for the copy, not for the pyramid kernels)"""
    from direct_stereo_slam_amd.tracker import pinned_array

    sc = make_scene("small", seed=16)
    trk = hip_tracker(ctx, sc)
    buf = pinned_array(sc.new_img.shape)
    buf[...] = sc.new_img
    trk.upload_image(0, buf, 1.0)
    buf[...] = -1.0  # must not affect the pyramid being built
    for lvl in range(sc.nl):
        np.testing.assert_array_equal(trk.get_frame(0, lvl), sc.new_p[lvl])


def test_scale_guess_list_as_one_batch_equals_the_sequential_loop(ctx):
    """FrontEnd::optimizeScale, untrapped branch (FrontEnd.cpp:995-1003): the eight initial guesses as ONE batched call on the
    same tracker vs the reference's sequential loop on the oracle -- same winner, same scale and error"""
    for idepth_scale in (1.0, 7.0):  # template depths off by a factor: the winner is no longer the guess 1
        sc = make_scene("small", seed=41, idepth_scale=idepth_scale)
        orc, trk = oracle_tracker(sc), hip_tracker(ctx, sc)
        guesses = [0.1, 1, 5, 10, 15, 25, 30, 50]
        new_scale, scale_error, all_o = 1.0, -1.0, []
        for g in guesses:
            err, s = orc.optimize_scale(g, sc.nl - 1)
            all_o.append((err, s))
            if err > 0 and (scale_error < 0 or scale_error > err):
                scale_error, new_scale = err, s
        err_g, s_g, errs, scales = trk.optimizeScaleGuesses(guesses, sc.nl - 1)
        for (eo, so), eg, sg in zip(all_o, errs, scales):
            assert abs(sg - so) < 1e-4 * max(1.0, abs(so)) and (abs(eg - eo) < 1e-3 * eo or (np.isnan(eo) and np.isnan(eg)))
        assert abs(s_g - new_scale) < 1e-4 * max(1.0, new_scale) and abs(err_g - scale_error) < 1e-3 * scale_error
        # (which guess wins is decided by the last bits when several guesses reach the same minimum -- here 5, 10 and 15 end at
        # the same scale with errors equal to 1e-6; the winner's scale and error are what FrontEnd uses)


def test_fixed_schedule_runs_one_plus_k_evaluations_per_level_like_the_oracle(ctx):
    """dsm_params.fixed_schedule (SURVEY.md 8d's benchmark schedule): exactly 1 + K evaluations per level, every step taken --
    on the device and on the oracle alike, so the two end at the same pose / scale"""
    from direct_stereo_slam_amd.tracker import default_params

    sc = make_scene("medium", seed=77)
    p, op = default_params(), O.default_params()
    p.fixed_schedule = op.fixed_schedule = 3
    orc, trk = oracle_tracker(sc, op), hip_tracker(ctx, sc, p)
    good_o, pose_o, aff_o, last_o, _ = orc.track(S.IDENTITY_POSE, [0, 0], sc.nl - 1)
    assert orc.eval_counts()[0][:sc.nl] == [4] * sc.nl
    r = trk.trackNewestCoarse(S.IDENTITY_POSE, [0, 0], sc.nl - 1)
    assert list(ctx.stats().evals)[:sc.nl] == [4] * sc.nl
    assert r[0] == good_o
    np.testing.assert_allclose(r[1], pose_o, atol=1e-4)
    np.testing.assert_allclose(r[2], aff_o, rtol=1e-3, atol=1e-3)
    np.testing.assert_allclose(r[3][:sc.nl], last_o[:sc.nl], rtol=1e-3)
    err_o, s_o = orc.optimize_scale(1.2, sc.nl - 1)
    assert orc.eval_counts()[0][:sc.nl] == [4] * sc.nl
    err_g, s_g = trk.optimizeScale(1.2, sc.nl - 1)
    assert list(ctx.stats().evals)[:sc.nl] == [4] * sc.nl
    assert abs(s_g - s_o) < 1e-4 * abs(s_o) and abs(err_g - err_o) < 1e-3 * err_o
    # ... whatever the scheduling form
    for coarse, queue in ((-1, 0), (0, 2)):
        p2 = default_params()
        p2.fixed_schedule, p2.persistent_coarse, p2.work_queue = 3, coarse, queue
        r2 = hip_tracker(ctx, sc, p2).trackNewestCoarse(S.IDENTITY_POSE, [0, 0], sc.nl - 1)
        assert list(ctx.stats().evals)[:sc.nl] == [4] * sc.nl
        for a, b in zip(r[1:], r2[1:]):
            np.testing.assert_array_equal(a, b)


def test_frame_hand_over_checks_and_the_intensity_only_form(ctx):
    """dsm_tracker_upload_frame verifies the caller's gradient channels (the device keeps channel 0 only) and names the first
    offending texel; dsm_params.frame_check / frame_grad_tol relax it; dsm_tracker_upload_intensity hands over channel 0 alone"""
    from direct_stereo_slam_amd._lib import DsmError
    from direct_stereo_slam_amd.tracker import default_params

    sc = make_scene("small", seed=5)
    trk = hip_tracker(ctx, sc)
    ref = trk.trackNewestCoarse(S.IDENTITY_POSE, [0, 0], sc.nl - 1)
    # intensity planes alone: same frame on the device, same result
    trk2 = hip_tracker(ctx, sc)
    trk2.upload_intensity(0, [np.ascontiguousarray(l[..., 0]) for l in sc.new_p], 1.0)
    for l in range(sc.nl):
        np.testing.assert_array_equal(trk2.get_frame(0, l)[1:-1], sc.new_p[l][1:-1])
    for a, b in zip(ref, trk2.trackNewestCoarse(S.IDENTITY_POSE, [0, 0], sc.nl - 1)):
        np.testing.assert_array_equal(a, b)
    # a gradient texel that is not makeImages': refused, with the level and the texel in the message
    bad = [l.copy() for l in sc.new_p]
    w1 = sc.w >> 1
    bad[1][7, 11, 1] *= np.float32(1.0 + 3e-5)
    with pytest.raises(DsmError, match=rf"level 1: 1 texel.*index {7 * w1 + 11} \(x = 11, y = 7\)"):
        trk.upload_frame(0, bad, 1.0)
    with pytest.raises(DsmError):  # the slot is unusable until a good frame arrives
        trk.trackNewestCoarse(S.IDENTITY_POSE, [0, 0], sc.nl - 1)
    # ... accepted to a tolerance, or unchecked: channel 0 is what is used either way
    for check, tol in ((1, 1e-3), (0, 0.0)):
        p = default_params()
        p.frame_check, p.frame_grad_tol = check, tol
        t3 = hip_tracker(ctx, sc, p)
        t3.upload_frame(0, bad, 1.0)
        for a, b in zip(ref, t3.trackNewestCoarse(S.IDENTITY_POSE, [0, 0], sc.nl - 1)):
            np.testing.assert_array_equal(a, b)
    p = default_params()
    p.frame_grad_tol = 1e-6
    with pytest.raises(DsmError, match="level 1"):
        hip_tracker(ctx, sc, p).upload_frame(0, bad, 1.0)
    # a parameter block of another header version is refused
    p = default_params()
    p.struct_size -= 4
    with pytest.raises(DsmError, match="struct_size"):
        hip_tracker(ctx, sc, p)
