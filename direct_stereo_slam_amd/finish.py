"""The end of FrontEnd::optimize behind its loop (dso_helpers/FrontEndOptimize.cpp:455-486, :39-72, :145-176, :504-523) in the same
device call as the loop -- the ctypes mirror of dsm_window_finish_batch and of the host form dsm_window_finish_host.  Semantics:
DESIGN.md section 22 (Z1-Z8, V).

A job is an optimize job (direct_stereo_slam_amd.optimize; its is_new is read here) with, on top: n_good_residuals_in (n_pts ints),
max_rel_baseline_in (n_pts floats), last_res (n_pts x 2 ints, -1: none) and last_state_in (n_pts x 2 bytes)."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import c_double_p, c_float_p, c_int_p, check
from .linearize import J_FLOATS, PRE, default_params
from .optimize import OptimizeBatch, default_optimize_params
from .step import OPTIONAL as STEP_OPTIONAL
from .step import default_step_params

c_ubyte_p = C.POINTER(C.c_ubyte)
FILL = -7.0
POINT_IN = (("n_good_residuals_in", np.int32, 1, c_int_p), ("max_rel_baseline_in", np.float32, 1, c_float_p), ("last_res", np.int32, 2, c_int_p),
            ("last_state_in", np.uint8, 2, c_ubyte_p))
FRAME_OUT = ("world_to_cam_eval_out", "state_zero_out", "state_out", "ad_host_out", "ad_target_out", "ad_ht_delta_out", "c_delta_out", "delta_x_out",
             "cam_out") + tuple(k + "_out" for k, _ in PRE)
RES_OUT = ("new_state", "new_energy", "new_energy_with_outlier", "keep", "rel_bs", "res_index_out")
POINT_OUT = ("n_good_residuals_out", "max_rel_baseline_out", "last_res_out", "last_state_out", "n_res_kept", "point_dropped", "point_index_out")
SCALAR_OUT = ("energy", "frame_energy_th_out", "n_res_out", "n_pts_out", "rmse", "lost")
FINISH_OPTIONAL = ("cam_to_world_out", "J_out")
FINISH_OUT = FRAME_OUT + RES_OUT + POINT_OUT + SCALAR_OUT + FINISH_OPTIONAL
_PTR = {np.dtype(np.float64): c_double_p, np.dtype(np.float32): c_float_p, np.dtype(np.int32): c_int_p, np.dtype(np.uint8): c_ubyte_p}


class FinishBatch:
    """The ctypes job table of dsm_window_finish_batch and its output arrays, built once: `run()` is the C call alone
    (tools/finish_timing.py times it), `results()` unpacks.  outputs: as OptimizeBatch's; finish_outputs: which of FINISH_OPTIONAL the
    jobs ask for; omit: names of FINISH_OUT (or of the finish's inputs) whose pointer stays NULL."""

    def __init__(self, jobs, outputs=STEP_OPTIONAL, finish_outputs=FINISH_OPTIONAL, omit=()):
        self.opt = OptimizeBatch(jobs, outputs)
        self.arr = (_lib.FinishJob * max(1, len(jobs)))()
        self.n = len(jobs)
        self.keep, self.outs = [], []
        for j, (G, job) in enumerate(zip(self.arr, jobs)):
            G.opt = self.opt.arr[j]
            n, m, nr = len(np.asarray(job["frame_ids"]).reshape(-1)), len(np.asarray(job["host"]).reshape(-1)), len(np.asarray(job["point"]).reshape(-1))
            N, mp, mr = 4 + 8 * n, max(1, m), max(1, nr)
            ins = {}
            for k, dtype, width, ptr in POINT_IN:
                a = np.ascontiguousarray(job[k], dtype).reshape(-1) if job.get(k) is not None else None
                if a is not None and len(a) != width * m:
                    raise ValueError(f"finish job: {k} has {len(a)} entries, not {width * m}")
                setattr(G, k, a.ctypes.data_as(ptr) if a is not None and k not in omit else None)
                ins[k] = a
            f64, f32, i32, u8 = np.float64, np.float32, np.int32, np.uint8
            out = dict(world_to_cam_eval_out=np.full((n, 7), FILL), state_zero_out=np.full((n, 8), FILL), state_out=np.full((n, 8), FILL),
                       ad_host_out=np.full((n, n, 8, 8), FILL), ad_target_out=np.full((n, n, 8, 8), FILL), ad_ht_delta_out=np.full((n, n, 8), FILL, f32),
                       c_delta_out=np.full(4, FILL, f32), delta_x_out=np.full(N, FILL), cam_out=np.full(6, FILL, f32),
                       new_state=np.full(mr, 77, u8), new_energy=np.full(mr, FILL, f32), new_energy_with_outlier=np.full(mr, FILL, f32),
                       keep=np.full(mr, 77, u8), rel_bs=np.full(mr, FILL, f32), res_index_out=np.full(mr, -77, i32),
                       n_good_residuals_out=np.full(mp, -77, i32), max_rel_baseline_out=np.full(mp, FILL, f32), last_res_out=np.full((mp, 2), -77, i32),
                       last_state_out=np.full((mp, 2), 77, u8), n_res_kept=np.full(mp, -77, i32), point_dropped=np.full(mp, 77, u8),
                       point_index_out=np.full(mp, -77, i32), energy=np.full(1, FILL, f64), frame_energy_th_out=np.full(1, FILL, f32),
                       n_res_out=np.full(1, -77, i32), n_pts_out=np.full(1, -77, i32), rmse=np.full(1, FILL, f32), lost=np.full(1, -77, i32),
                       cam_to_world_out=np.full((n, 7), FILL), J_out=np.full((mr, J_FLOATS), FILL, f32))
            out.update({k + "_out": np.full((n, n, w), FILL, f32) for k, w in PRE})
            for k, a in out.items():
                given = k not in omit and (k not in FINISH_OPTIONAL or k in finish_outputs)
                setattr(G, k, a.ctypes.data_as(_PTR[a.dtype]) if given else None)
            self.keep.append(ins)
            self.outs.append((out, m, nr))

    def _params(self, params, step_params, optimize_params):
        return (params if params is not None else default_params(), step_params if step_params is not None else default_step_params(),
                optimize_params if optimize_params is not None else default_optimize_params())

    def run(self, ctx, params=None, step_params=None, optimize_params=None):
        """one dsm_window_finish_batch call"""
        p, sp, op = self._params(params, step_params, optimize_params)
        check(ctx.L.dsm_window_finish_batch(ctx.h, self.n, self.arr, C.byref(p), C.byref(sp), C.byref(op)))

    def run_host(self, w, h, j, frames, params=None, step_params=None, optimize_params=None):
        """dsm_window_finish_host on job j; frames: the level-0 planes in frame_ids order"""
        p, sp, op = self._params(params, step_params, optimize_params)
        planes = [np.ascontiguousarray(f, np.float32) for f in frames]
        ptrs = (c_float_p * max(1, len(planes)))(*[a.ctypes.data_as(c_float_p) for a in planes])
        check(_lib.load().dsm_window_finish_host(int(w), int(h), C.byref(self.arr[j]), ptrs, C.byref(p), C.byref(sp), C.byref(op)))

    def all_outputs(self):
        """per job every output array itself: the optimize call's under their names, the finish's under "fin." + name"""
        return [dict(oo, **{"fin." + k: v for k, v in out.items()}) for oo, (out, _, _) in zip(self.opt.all_outputs(), self.outs)]

    def results(self):
        """per job a pair: OptimizeBatch.results' dict (the loop's last pass and log) and the finish's dict: the arrays of FINISH_OUT cut to
        the job's points and residuals, the one-word outputs as scalars; what was not asked for keeps the mirror's fill value"""
        res = []
        for o, (out, m, nr) in zip(self.opt.results(), self.outs):
            d = {}
            for k, v in out.items():
                d[k] = v[:nr].copy() if k in RES_OUT + ("J_out",) else v[:m].copy() if k in POINT_OUT else v[0] if k in SCALAR_OUT else v.copy()
            res.append((o, d))
        return res


def window_finish_batch(ctx, jobs, params=None, step_params=None, optimize_params=None, **kw):
    """dsm_window_finish_batch: per job the pair of FinishBatch.results"""
    b = FinishBatch(jobs, **kw)
    b.run(ctx, params, step_params, optimize_params)
    return b.results()


def window_finish_host(w, h, job, frames, params=None, step_params=None, optimize_params=None, **kw):
    """dsm_window_finish_host (no device): the same pair for one job"""
    b = FinishBatch([job], **kw)
    b.run_host(w, h, 0, frames, params, step_params, optimize_params)
    return b.results()[0]
