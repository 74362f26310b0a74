"""What FrontEnd::solveSystem builds before every solve (dso_helpers/FrontEndOptimize.cpp:488-494): getNullspaces (:525-574) with the
frames' numeric nullspaces in front of it and the basis with its pseudo-inverse behind it -- the ctypes mirror of
dsm_window_nullspace_batch and of the host form dsm_window_nullspace_host.  Semantics: DESIGN.md section 23 (G1-G7, V).

A job is a dict: world_to_cam_eval (n x 7, what dsm_window_finish_batch returns as world_to_cam_eval), state_zero (n x 8), exposure (n)
and optionally frame_null_in (n x 42).  A result dict passes straight into direct_stereo_slam_amd.solve.window_solve_batch:
dict(solve_job, **{k: res[k] for k in ("null_basis", "null_pinv", "n_null")})."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import c_double_p, c_float_p, c_int_p, check

FILL = -7777.0
OPTIONAL = ("frame_null", "null_x0_pre")
N_NULL = 7


def default_nullspace_params(**kw):
    """dsm_nullspace_params with the upstream defaults, then the given fields"""
    p = _lib.NullspaceParams()
    if _lib.load().dsm_nullspace_params_default(C.byref(p)) != 0:
        raise _lib.DsmError("dsm_nullspace_params_default failed")
    for k, v in kw.items():
        if not hasattr(p, k):
            raise ValueError(f"dsm_nullspace_params has no field {k}")
        setattr(p, k, v)
    return p


class NullspaceBatch:
    """The ctypes job table of dsm_window_nullspace_batch and its output arrays, built once: `run()` is the C call alone
    (tools/nullspace_timing.py times it), `results()` unpacks.  outputs: which of the optional outputs the jobs ask for.  A job may
    carry n_frames (otherwise the rows of world_to_cam_eval) and drop: the name of a required output to leave NULL (the tests of V)."""

    def __init__(self, jobs, outputs=OPTIONAL):
        self.arr = (_lib.NullspaceJob * max(1, len(jobs)))()
        self.n = len(jobs)
        self.keep, self.outs = [], []
        for S, job in zip(self.arr, jobs):
            rows = [np.asarray(job[k]).reshape(-1, w).shape[0] for k, w in (("world_to_cam_eval", 7), ("state_zero", 8)) if job.get(k) is not None]
            n = rows[0] if rows else 1
            N = 4 + 8 * n
            ins = {}

            def take(k, dtype, size, ptr):
                a = np.ascontiguousarray(job[k], dtype).reshape(-1) if job.get(k) is not None else None
                if a is not None and len(a) != size:
                    raise ValueError(f"nullspace job: {k} has {len(a)} entries, not {size}")
                setattr(S, k, a.ctypes.data_as(ptr) if a is not None else None)
                ins[k] = a

            take("world_to_cam_eval", np.float64, 7 * n, c_double_p), take("state_zero", np.float64, 8 * n, c_double_p)
            take("exposure", np.float32, n, c_float_p), take("frame_null_in", np.float64, 42 * n, c_double_p)
            S.n_frames = int(job.get("n_frames", n))
            out = dict(null_basis=np.full((N, 7), FILL), null_pinv=np.full((7, N), FILL), sing=np.full(7, FILL), rank=np.full(1, 77, np.int32),
                       flags=np.full(1, 77, np.int32), frame_null=np.full((n, 42), FILL), null_x0_pre=np.full((N, 9), FILL))
            drop = job.get("drop")
            for k in ("null_basis", "null_pinv", "sing"):
                setattr(S, k, out[k].ctypes.data_as(c_double_p) if k != drop else None)
            for k in ("rank", "flags"):
                setattr(S, k, out[k].ctypes.data_as(c_int_p) if k != drop else None)
            S.frame_null_out = out["frame_null"].ctypes.data_as(c_double_p) if "frame_null" in outputs else None
            S.null_x0_pre = out["null_x0_pre"].ctypes.data_as(c_double_p) if "null_x0_pre" in outputs else None
            self.keep.append(ins)
            self.outs.append(out)

    def run(self, ctx, params=None):
        """one dsm_window_nullspace_batch call; params None: the C side's defaults (a NULL pointer)"""
        check(ctx.L.dsm_window_nullspace_batch(ctx.h, self.n, self.arr, C.byref(params) if params is not None else None))

    def run_host(self, params=None):
        """dsm_window_nullspace_host on every job"""
        check(_lib.load().dsm_window_nullspace_host(self.n, self.arr, C.byref(params) if params is not None else None))

    def all_outputs(self):
        """per job every output array itself"""
        return self.outs

    def results(self):
        """per job a dict: null_basis (N x 7), null_pinv (7 x N), n_null = 7, sing, rank and flags (ints), frame_null (n x 42),
        null_x0_pre (N x 9); what was not asked for, or not written, keeps the mirror's fill value"""
        return [dict({k: int(v[0]) if k in ("rank", "flags") else v.copy() for k, v in out.items()}, n_null=N_NULL) for out in self.outs]


def window_nullspace_batch(ctx, jobs, params=None, outputs=OPTIONAL):
    """dsm_window_nullspace_batch: per job the dict of NullspaceBatch.results"""
    b = NullspaceBatch(jobs, outputs)
    b.run(ctx, params)
    return b.results()


def window_nullspace_host(jobs, params=None, outputs=OPTIONAL):
    """dsm_window_nullspace_host (no device): the same dicts"""
    b = NullspaceBatch(jobs, outputs)
    b.run_host(params)
    return b.results()
