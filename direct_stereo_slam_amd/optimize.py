"""The accept / reject loop of FrontEnd::optimize (dso_helpers/FrontEndOptimize.cpp:362-371, :382-453) in one device call, every window
with its own lambda, factors, iteration count and break -- the ctypes mirror of dsm_window_optimize_batch and of the host form
dsm_window_optimize_host.  Semantics: DESIGN.md section 20.

A job is a step job (direct_stereo_slam_amd.step) at the window's current state WITHOUT frame_step, calib_step and idepth_step (the
loop forms them; stepfac and lambda are not read) and with max_iterations on top."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import c_double_p, c_float_p, c_int_p, check
from .linearize import default_params
from .step import OPTIONAL, StepBatch, default_step_params

MAX_ITERATIONS = 20
LOG = ("n_iterations", "n_passes", "pattern", "pass_energy", "pass_lambda", "iter_stepsize", "iter_can_break", "last_energy", "lambda_out",
       "frame_energy_th_out")
FILL_BYTE = 0xAB


def default_optimize_params(**kw):
    """dsm_optimize_params with the struct defaults (the loop of host/step_demo.cpp), then the given fields"""
    p = _lib.OptimizeParams()
    if _lib.load().dsm_optimize_params_default(C.byref(p)) != 0:
        raise _lib.DsmError("dsm_optimize_params_default failed")
    for k, v in kw.items():
        if not hasattr(p, k):
            raise ValueError(f"dsm_optimize_params has no field {k}")
        setattr(p, k, v)
    return p


class OptimizeBatch:
    """The ctypes job table of dsm_window_optimize_batch and its output arrays, built once: `run()` is the C call alone
    (tools/optimize_timing.py times it), `results()` unpacks.  outputs: as StepBatch's.  omit: names of LOG whose pointer stays NULL."""

    def __init__(self, jobs, outputs=OPTIONAL, omit=()):
        self.step = StepBatch([dict(job, stepfac=job.get("stepfac", (0.0,) * 5)) for job in jobs], outputs)
        self.arr = (_lib.OptimizeJob * max(1, len(jobs)))()
        self.n = len(jobs)
        self.logs = []
        for j, (G, job) in enumerate(zip(self.arr, jobs)):
            G.step = self.step.arr[j]
            its = int(job["max_iterations"])
            G.max_iterations = its
            m, p = max(1, min(its, MAX_ITERATIONS)), 1 + 2 * max(0, min(its, MAX_ITERATIONS))
            log = dict(n_iterations=np.full(1, 77, np.int32), n_passes=np.full(1, 77, np.int32), pattern=np.full(m, FILL_BYTE, np.uint8),
                       pass_energy=np.full((p, 2), np.nan), pass_lambda=np.full(p, np.nan), iter_stepsize=np.full(m, np.nan, np.float32),
                       iter_can_break=np.full(m, FILL_BYTE, np.uint8), last_energy=np.full(2, np.nan), lambda_out=np.full(1, np.nan),
                       frame_energy_th_out=np.full(1, np.nan, np.float32))
            ptr = dict(n_iterations=c_int_p, n_passes=c_int_p, pattern=C.POINTER(C.c_ubyte), pass_energy=c_double_p, pass_lambda=c_double_p,
                       iter_stepsize=c_float_p, iter_can_break=C.POINTER(C.c_ubyte), last_energy=c_double_p, lambda_out=c_double_p,
                       frame_energy_th_out=c_float_p)
            for k in LOG:
                setattr(G, k, None if k in omit else log[k].ctypes.data_as(ptr[k]))
            self.logs.append((log, its))

    def run(self, ctx, params=None, step_params=None, optimize_params=None):
        """one dsm_window_optimize_batch call"""
        p = params if params is not None else default_params()
        sp = step_params if step_params is not None else default_step_params()
        op = optimize_params if optimize_params is not None else default_optimize_params()
        check(ctx.L.dsm_window_optimize_batch(ctx.h, self.n, self.arr, C.byref(p), C.byref(sp), C.byref(op)))

    def run_host(self, w, h, j, frames, params=None, step_params=None, optimize_params=None):
        """dsm_window_optimize_host on job j; frames: the level-0 planes in frame_ids order"""
        p = params if params is not None else default_params()
        sp = step_params if step_params is not None else default_step_params()
        op = optimize_params if optimize_params is not None else default_optimize_params()
        planes = [np.ascontiguousarray(f, np.float32) for f in frames]
        ptrs = (c_float_p * max(1, len(planes)))(*[a.ctypes.data_as(c_float_p) for a in planes])
        check(_lib.load().dsm_window_optimize_host(int(w), int(h), C.byref(self.arr[j]), ptrs, C.byref(p), C.byref(sp), C.byref(op)))

    def all_outputs(self):
        """per job every output array itself (the step call's among them)"""
        return [dict(so, **log) for so, (log, _) in zip(self.step.all_outputs(), self.logs)]

    def results(self):
        """per job a dict: StepBatch.results (the job's last pass) and, on top, n_iterations, n_passes (ints), pattern (a str of the
        iterations run), pass_energy (n_passes x 2), pass_lambda (n_passes), iter_stepsize, iter_can_break (per iteration run),
        last_energy (2), lambda_out, frame_energy_th_out, and `raw`: the log arrays whole, as written"""
        res = self.step.results()
        for d, (log, its) in zip(res, self.logs):
            ni, npass = int(log["n_iterations"][0]), int(log["n_passes"][0])
            ok = 0 <= ni <= its and 0 <= npass <= 1 + 2 * its
            d.update(n_iterations=ni, n_passes=npass, last_energy=log["last_energy"].copy(), lambda_out=log["lambda_out"][0],
                     frame_energy_th_out=log["frame_energy_th_out"][0], raw={k: v.copy() for k, v in log.items()})
            if ok:
                d.update(pattern=bytes(log["pattern"][:ni]).decode("latin-1"), pass_energy=log["pass_energy"][:npass].copy(),
                         pass_lambda=log["pass_lambda"][:npass].copy(), iter_stepsize=log["iter_stepsize"][:ni].copy(),
                         iter_can_break=log["iter_can_break"][:ni].copy())
        return res


def window_optimize_batch(ctx, jobs, params=None, step_params=None, optimize_params=None, outputs=OPTIONAL):
    """dsm_window_optimize_batch: per job the dict of OptimizeBatch.results"""
    b = OptimizeBatch(jobs, outputs)
    b.run(ctx, params, step_params, optimize_params)
    return b.results()


def window_optimize_host(w, h, job, frames, params=None, step_params=None, optimize_params=None, outputs=OPTIONAL):
    """dsm_window_optimize_host (no device): the same dict for one job"""
    b = OptimizeBatch([job], outputs)
    b.run_host(w, h, 0, frames, params, step_params, optimize_params)
    return b.results()[0]
