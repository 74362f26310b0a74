"""One trial step of FrontEnd::optimize (dso_helpers/FrontEndOptimize.cpp:332-486) between backupState and doStepFromBackup on the
device: linearisation, Hessian and Schur accumulation, stitch, damping, solve and back-substitution -- the ctypes mirror of
dsm_window_solve_batch and of the host form dsm_window_solve_host.  Semantics: DESIGN.md section 18 (T1d, F1-F8, R1-R3, V).

A job is a hessian job (direct_stereo_slam_amd.hessian) with, on top: H_L (N x N doubles), b_L (N), the optional H_M, b_M, delta_x,
lambda (default 0), and the optional null_basis (N x n_null) with null_pinv (n_null x N); N = 4 + 8 n_frames."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import c_double_p, c_float_p, c_int_p, check
from .hessian import FILL, HessianBatch
from .hessian import OPTIONAL as HES_OPTIONAL
from .linearize import KeyframeWindow, default_params  # noqa: F401  (the window type and the settings of this call)

STITCHED = ("H_A", "b_A", "H_sc", "b_sc")
LAST = ("last_HS", "last_bS")
OPTIONAL = STITCHED + LAST + HES_OPTIONAL
X_NOT_FINITE, STEP_NOT_FINITE = 1, 2


class SolveBatch:
    """The ctypes job table of dsm_window_solve_batch and its output arrays, built once: `run()` is the C call alone
    (tools/solve_timing.py times it), `results()` unpacks.  outputs: which of the optional outputs the jobs ask for."""

    def __init__(self, jobs, outputs=OPTIONAL):
        self.hes = HessianBatch(jobs, [k for k in outputs if k in HES_OPTIONAL])
        self.arr = (_lib.SolveJob * max(1, len(jobs)))()
        self.n = len(jobs)
        self.keep, self.outs = [], []
        for j, (S, job) in enumerate(zip(self.arr, jobs)):
            S.hes = self.hes.arr[j]
            for k in STITCHED:
                if k not in outputs:
                    setattr(S.hes, k, None)
            nf, n = S.hes.lin.n_frames, S.hes.lin.n_pts
            N = 4 + 8 * nf
            ins = {}
            for k, size in (("H_L", N * N), ("b_L", N), ("H_M", N * N), ("b_M", N), ("delta_x", N)):
                a = np.ascontiguousarray(job[k], np.float64).reshape(-1) if job.get(k) is not None else None
                if a is not None and len(a) != size:
                    raise ValueError(f"solve job: {k} has {len(a)} entries, not {size}")
                setattr(S, k, a.ctypes.data_as(c_double_p) if a is not None else None)
                ins[k] = a
            S.lambda_ = float(job.get("lambda", 0.0))
            basis, pinv = job.get("null_basis"), job.get("null_pinv")
            nn = int(job["n_null"]) if "n_null" in job else (0 if basis is None else np.asarray(basis).reshape(N, -1).shape[1])
            S.n_null = nn
            for k, a in (("null_basis", basis), ("null_pinv", pinv)):
                a = np.ascontiguousarray(a, np.float64).reshape(-1) if a is not None else None
                if a is not None and 0 <= nn <= 8 and len(a) != N * nn:
                    raise ValueError(f"solve job: {k} is not N x n_null")
                setattr(S, k, a.ctypes.data_as(c_double_p) if a is not None else None)
                ins[k] = a
            out = dict(x=np.full(N, FILL), step=np.full(max(1, n), FILL, np.float32), flags=np.full(1, 77, np.int32),
                       last_HS=np.full((N, N), FILL), last_bS=np.full(N, FILL))
            S.x, S.step, S.flags = out["x"].ctypes.data_as(c_double_p), out["step"].ctypes.data_as(c_float_p), out["flags"].ctypes.data_as(c_int_p)
            for k in LAST:
                setattr(S, k, out[k].ctypes.data_as(c_double_p) if k in outputs else None)
            self.keep.append(ins)
            self.outs.append((out, n))

    def run(self, ctx, params=None):
        """one dsm_window_solve_batch call"""
        p = params if params is not None else default_params()
        check(ctx.L.dsm_window_solve_batch(ctx.h, self.n, self.arr, C.byref(p)))

    def run_host(self, w, h, j, frames, params=None):
        """dsm_window_solve_host on job j; frames: the level-0 planes in frame_ids order"""
        p = params if params is not None else default_params()
        planes = [np.ascontiguousarray(f, np.float32) for f in frames]
        ptrs = (c_float_p * max(1, len(planes)))(*[a.ctypes.data_as(c_float_p) for a in planes])
        check(_lib.load().dsm_window_solve_host(int(w), int(h), C.byref(self.arr[j]), ptrs, C.byref(p)))

    def all_outputs(self):
        """per job every output array itself (the Hessian call's and the linearisation's among them)"""
        return [dict(ho, **so) for ho, (so, _) in zip(self.hes.all_outputs(), self.outs)]

    def results(self):
        """per job a dict: HessianBatch.results and, on top, x, step, flags (an int), last_HS, last_bS; what was not asked for, or not
        written, keeps the mirror's fill value"""
        res = self.hes.results()
        for d, (out, n) in zip(res, self.outs):
            for k, v in out.items():
                d[k] = v[:n].copy() if k == "step" else int(v[0]) if k == "flags" else v.copy()
        return res


def window_solve_batch(ctx, jobs, params=None, outputs=OPTIONAL):
    """dsm_window_solve_batch: per job the dict of SolveBatch.results"""
    b = SolveBatch(jobs, outputs)
    b.run(ctx, params)
    return b.results()


def window_solve_host(w, h, job, frames, params=None, outputs=OPTIONAL):
    """dsm_window_solve_host (no device): the same dict for one job"""
    b = SolveBatch([job], outputs)
    b.run_host(w, h, 0, frames, params)
    return b.results()[0]
