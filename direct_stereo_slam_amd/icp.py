"""ICP fallback of loop closure on the device: `icp()` of src/loop_closure/pose_estimation/icp.h:44-71 (PCL's IterativeClosestPoint with the
reference's settings) through dsm_icp_batch, one call for a batch of independent matches.  Semantics: DESIGN.md section 10 (P1-P9, D1-D5).
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import c_double_p, c_float_p, c_int_p, check

MAX_ITERATIONS = 5               # icp.h:58
TRANSFORMATION_EPSILON = 0.01    # icp.h:59
MAX_CORRESPONDENCE_DISTANCE = 2.0  # icp.h:60
ICP_THRES = 1.5                  # icp.h:20
ITERATIONS_LIMIT = 64
STATES = {0: "not converged", 1: "iterations", 2: "transform", 3: "absolute MSE", 5: "no correspondences", 6: "empty"}
# dsm_diag_icp_stages (test aid): the stages of the launch sequence, the "no neighbour" key and dsm_icp_state
STAGE_PREP, STAGE_SEARCH, STAGE_STEP, STAGE_FITNESS_PREP, STAGE_FITNESS_SEARCH, STAGE_FITNESS = range(6)
NO_KEY = 0xFFFFFFFFFFFFFFFF
STATE_DTYPE = np.dtype([("final_tf", np.float32, (4, 4)), ("prev_mse", np.float64), ("fitness", np.float64), ("state", np.int32),
                        ("iterations", np.int32), ("searches", np.int32), ("pad", np.int32), ("corr", np.int32, ITERATIONS_LIMIT)])


class IcpBatch:
    """The ctypes job table of dsm_icp_batch and its output arrays, built once: `run()` is the C call alone (tools/icp_timing.py times
    it), `results()` unpacks.  jobs: list of (pts_source, pts_target, tfm_target_source) with the meaning of icp.h: source = the matched
    keyframe's pts_spherical (n x 3), target = the current keyframe's, tfm = the 4x4 guess."""

    def __init__(self, ctx, jobs, max_iterations=MAX_ITERATIONS, transformation_epsilon=TRANSFORMATION_EPSILON,
                 max_corr_dist=MAX_CORRESPONDENCE_DISTANCE, score_thres=ICP_THRES):
        self.ctx, self.L = ctx, ctx.L
        self.params = (int(max_iterations), float(transformation_epsilon), float(max_corr_dist), float(score_thres))
        self.arr = (_lib.IcpJob * len(jobs))()
        self.keep, self.outs = [], []
        for j, (src, tgt, tfm) in enumerate(jobs):
            src = np.ascontiguousarray(src, np.float64).reshape(-1, 3)
            tgt = np.ascontiguousarray(tgt, np.float64).reshape(-1, 3)
            guess = np.ascontiguousarray(tfm, np.float64).reshape(4, 4)
            o = dict(tfm=guess.copy(), score=np.zeros(1, np.float32), ok=np.zeros(1, np.int32), iterations=np.zeros(1, np.int32),
                     state=np.zeros(1, np.int32), corr=np.zeros(max(1, int(max_iterations)), np.int32))
            self.keep.append((src, tgt, guess))
            self.outs.append(o)
            J = self.arr[j]
            J.n_src, J.src_xyz = len(src), src.ctypes.data_as(c_double_p)
            J.n_tgt, J.tgt_xyz = len(tgt), tgt.ctypes.data_as(c_double_p)
            J.tfm_target_source, J.score = o["tfm"].ctypes.data_as(c_double_p), o["score"].ctypes.data_as(c_float_p)
            J.ok, J.iterations = o["ok"].ctypes.data_as(c_int_p), o["iterations"].ctypes.data_as(c_int_p)
            J.state, J.corr_counts = o["state"].ctypes.data_as(c_int_p), o["corr"].ctypes.data_as(c_int_p)

    def run(self):
        """one dsm_icp_batch call; tfm_target_source starts from each job's guess every time"""
        for (_, _, guess), o in zip(self.keep, self.outs):
            o["tfm"][...] = guess
        check(self.L.dsm_icp_batch(self.ctx.h, len(self.arr), self.arr, *self.params))

    def results(self):
        res = []
        for o in self.outs:
            it, state = int(o["iterations"][0]), int(o["state"][0])
            n_search = it + (1 if state == 5 else 0)
            res.append(dict(ok=bool(o["ok"][0]), tfm=o["tfm"].copy(), score=np.float32(o["score"][0]), iterations=it, state=state,
                            corr_counts=[int(c) for c in o["corr"][:n_search]]))
        return res


def icp_batch(ctx, jobs, **params):
    """dsm_icp_batch over jobs = [(pts_source, pts_target, tfm_target_source), ...]; per job a dict with ok, tfm (the updated
    tfm_target_source), score (float32 icp_score), iterations, state (key of STATES) and corr_counts (pairs kept per search)"""
    b = IcpBatch(ctx, jobs, **params)
    b.run()
    return b.results()


def icp(ctx, pts_source, pts_target, tfm_target_source, **params):
    """icp(pts_source, pts_target, tfm_target_source, icp_score) of icp.h for one match: the same dict as icp_batch"""
    return icp_batch(ctx, [(pts_source, pts_target, tfm_target_source)], **params)[0]


def icp_stages(ctx, jobs, stop_stage, stop_iteration=0, want_slices=0, **params):
    """Test aid (dsm_diag_icp_stages): dsm_icp_batch's own launch sequence over `jobs`, stopped after stop_stage (STAGE_*; for the
    search and the step, of the 0-based iteration stop_iteration), the target of every job cut into want_slices slices (0: the
    production rule).  Per job a dict of what the device holds there: orig, work (n_src x 4 float32: x, y, z, 0), target (n_tgt x 4),
    keys (n_src uint64: float bits of dist2 << 32 | target index, NO_KEY for none) and state (a STATE_DTYPE record)."""
    b = IcpBatch(ctx, jobs, **params)
    n_src = [len(src) for src, _, _ in b.keep]
    n_tgt = [len(tgt) for _, tgt, _ in b.keep]
    orig, work = np.full((sum(n_src), 4), np.nan, np.float32), np.full((sum(n_src), 4), np.nan, np.float32)
    target, keys = np.full((sum(n_tgt), 4), np.nan, np.float32), np.zeros(sum(n_src), np.uint64)
    states = np.zeros(len(jobs), STATE_DTYPE)
    check(ctx.L.dsm_diag_icp_stages(ctx.h, len(b.arr), b.arr, *b.params[:3], int(want_slices), int(stop_stage), int(stop_iteration),
                                    orig.ctypes.data_as(c_float_p), work.ctypes.data_as(c_float_p), target.ctypes.data_as(c_float_p),
                                    keys.ctypes.data_as(C.POINTER(C.c_uint64)), states.ctypes.data_as(C.c_void_p)))
    s0 = np.concatenate([[0], np.cumsum(n_src)])
    t0 = np.concatenate([[0], np.cumsum(n_tgt)])
    return [dict(orig=orig[s0[j]:s0[j + 1]], work=work[s0[j]:s0[j + 1]], target=target[t0[j]:t0[j + 1]], keys=keys[s0[j]:s0[j + 1]],
                 state=states[j]) for j in range(len(jobs))]
