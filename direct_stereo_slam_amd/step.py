"""One iteration of FrontEnd::optimize (dso_helpers/FrontEndOptimize.cpp:332-486) in one device call: doStepFromBackup (:182-262) with
setPrecalcValues (:300-323), the M energy and the priors, then the trial step of direct_stereo_slam_amd.solve at the new state -- the
ctypes mirror of dsm_window_step_batch and of the host form dsm_window_step_host.  Semantics: DESIGN.md section 19 (D1-D4, Q1-Q4, E1-E3,
V).

A job is a solve job (direct_stereo_slam_amd.solve) WITHOUT what the device forms (the six precalc tables, idepth_scaled,
idepth_zero_scaled, delta, delta_x; cam and cam_inv are not read) and with, on top: world_to_cam_eval (n x 7), state_zero,
state_backup, frame_step (n x 8), calib_zero, calib_backup, calib_step (4), idepth_backup, idepth_step (n_pts), exposure (n),
stepfac (C, T, R, A, D) and the optional state_prior, state_prior_zero (N: the C fields prior and prior_zero; "prior" is the points'
prior of the hessian job); N = 4 + 8 n_frames."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import c_double_p, c_float_p, c_int_p, check
from .linearize import PRE, KeyframeWindow, default_params  # noqa: F401  (the window type and the settings of this call)
from .solve import FILL
from .solve import OPTIONAL as SOLVE_OPTIONAL
from .solve import SolveBatch

FRAME_IN = (("world_to_cam_eval", 7), ("state_zero", 8), ("state_backup", 8), ("frame_step", 8))
CALIB_IN = ("calib_zero", "calib_backup", "calib_step")
PASS_THROUGH = ("cam",) + tuple(k for k, _ in PRE) + ("delta_x", "H_L_step", "b_L_step")
OPTIONAL = ("cam_to_world",) + PASS_THROUGH + SOLVE_OPTIONAL
FORMED = tuple(k for k, _ in PRE) + ("idepth_scaled", "idepth_zero_scaled", "delta", "delta_x")


def default_step_params(**kw):
    """dsm_step_params with the upstream defaults, then the given fields"""
    p = _lib.StepParams()
    if _lib.load().dsm_step_params_default(C.byref(p)) != 0:
        raise _lib.DsmError("dsm_step_params_default failed")
    for k, v in kw.items():
        if not hasattr(p, k):
            raise ValueError(f"dsm_step_params has no field {k}")
        setattr(p, k, v)
    return p


class StepBatch:
    """The ctypes job table of dsm_window_step_batch and its output arrays, built once: `run()` is the C call alone
    (tools/step_timing.py times it), `results()` unpacks.  outputs: which of the optional outputs the jobs ask for; the stitched H_L
    and b_L with the priors are "H_L_step" and "b_L_step" (a solve job's H_L and b_L are inputs)."""

    def __init__(self, jobs, outputs=OPTIONAL):
        n_of = [len(np.asarray(job["frame_ids"]).reshape(-1)) for job in jobs]
        np_of = [len(np.asarray(job["host"]).reshape(-1)) for job in jobs]
        # the solve mirror wants arrays of the right size where this call wants NULL; the pointers are cleared below unless the job
        # itself gives one (which the call refuses)
        filled = []
        for job, n, m in zip(jobs, n_of, np_of):
            d = dict(job, cam=(1.0, 1.0, 0.0, 0.0), cam_inv=(1.0, 1.0))
            for k, w in PRE:
                if d.get(k) is None:
                    d[k] = np.zeros((n, n, w), np.float32)
            for k in ("idepth_scaled", "idepth_zero_scaled"):
                if d.get(k) is None:
                    d[k] = np.zeros(m, np.float32)
            filled.append(d)
        self.sol = SolveBatch(filled, [k for k in outputs if k in SOLVE_OPTIONAL])
        self.arr = (_lib.StepJob * max(1, len(jobs)))()
        self.n = len(jobs)
        self.keep, self.outs = [], []
        for j, (S, job) in enumerate(zip(self.arr, jobs)):
            S.sol = self.sol.arr[j]
            L = S.sol.hes.lin
            for k, _ in PRE:
                if job.get(k) is None:
                    setattr(L, k, None)
            for k in ("idepth_scaled", "idepth_zero_scaled"):
                if job.get(k) is None:
                    setattr(L, k, None)
            n, m = n_of[j], np_of[j]
            N = 4 + 8 * n
            ins = {}

            def take(k, dtype, size, ptr, field=None):
                a = np.ascontiguousarray(job[k], dtype).reshape(-1) if job.get(k) is not None else None
                if a is not None and len(a) != size:
                    raise ValueError(f"step job: {k} has {len(a)} entries, not {size}")
                setattr(S, field or k, a.ctypes.data_as(ptr) if a is not None else None)
                ins[k] = a

            for k, w in FRAME_IN:
                take(k, np.float64, w * n, c_double_p)
            for k in CALIB_IN:
                take(k, np.float64, 4, c_double_p)
            take("idepth_backup", np.float32, m, c_float_p), take("idepth_step", np.float32, m, c_float_p), take("exposure", np.float32, n, c_float_p)
            take("state_prior", np.float64, N, c_double_p, "prior"), take("state_prior_zero", np.float64, N, c_double_p, "prior_zero")
            S.stepfac = (C.c_float * 5)(*[float(x) for x in job["stepfac"]])
            out = dict(state=np.full((n, 8), FILL), calib=np.full(4, FILL), idepth=np.full(max(1, m), FILL, np.float32),
                       world_to_cam=np.full((n, 7), FILL), cam_to_world=np.full((n, 7), FILL), can_break=np.full(1, 77, np.int32),
                       step_sums=np.full(6, FILL, np.float32), energy_m=np.full(1, FILL), cam=np.full(6, FILL, np.float32),
                       delta_x=np.full(N, FILL), H_L_step=np.full((N, N), FILL), b_L_step=np.full(N, FILL))
            out.update({k: np.full((n, n, w), FILL, np.float32) for k, w in PRE})
            S.state_out, S.calib_out, S.world_to_cam_out = (out[k].ctypes.data_as(c_double_p) for k in ("state", "calib", "world_to_cam"))
            S.idepth_out, S.step_sums = out["idepth"].ctypes.data_as(c_float_p), out["step_sums"].ctypes.data_as(c_float_p)
            S.can_break, S.energy_m = out["can_break"].ctypes.data_as(c_int_p), out["energy_m"].ctypes.data_as(c_double_p)
            S.cam_to_world_out = out["cam_to_world"].ctypes.data_as(c_double_p) if "cam_to_world" in outputs else None
            S.cam_out = out["cam"].ctypes.data_as(c_float_p) if "cam" in outputs else None
            for k, _ in PRE:
                setattr(S, k + "_out", out[k].ctypes.data_as(c_float_p) if k in outputs else None)
            S.delta_x_out = out["delta_x"].ctypes.data_as(c_double_p) if "delta_x" in outputs else None
            S.H_L_out = out["H_L_step"].ctypes.data_as(c_double_p) if "H_L_step" in outputs else None
            S.b_L_out = out["b_L_step"].ctypes.data_as(c_double_p) if "b_L_step" in outputs else None
            self.keep.append(ins)
            self.outs.append((out, m))

    def run(self, ctx, params=None, step_params=None):
        """one dsm_window_step_batch call"""
        p = params if params is not None else default_params()
        sp = step_params if step_params is not None else default_step_params()
        check(ctx.L.dsm_window_step_batch(ctx.h, self.n, self.arr, C.byref(p), C.byref(sp)))

    def run_host(self, w, h, j, frames, params=None, step_params=None):
        """dsm_window_step_host on job j; frames: the level-0 planes in frame_ids order"""
        p = params if params is not None else default_params()
        sp = step_params if step_params is not None else default_step_params()
        planes = [np.ascontiguousarray(f, np.float32) for f in frames]
        ptrs = (c_float_p * max(1, len(planes)))(*[a.ctypes.data_as(c_float_p) for a in planes])
        check(_lib.load().dsm_window_step_host(int(w), int(h), C.byref(self.arr[j]), ptrs, C.byref(p), C.byref(sp)))

    def all_outputs(self):
        """per job every output array itself (the solve call's among them)"""
        return [dict(so, **out) for so, (out, _) in zip(self.sol.all_outputs(), self.outs)]

    def results(self):
        """per job a dict: SolveBatch.results and, on top, state, calib, idepth, world_to_cam, cam_to_world, can_break (an int),
        step_sums, energy_m, cam, the six tables, delta_x, H_L_step, b_L_step; what was not asked for, or not written, keeps the
        mirror's fill value"""
        res = self.sol.results()
        for d, (out, m) in zip(res, self.outs):
            for k, v in out.items():
                d[k] = v[:m].copy() if k == "idepth" else int(v[0]) if k == "can_break" else v[0] if k == "energy_m" else v.copy()
        return res


def window_step_batch(ctx, jobs, params=None, step_params=None, outputs=OPTIONAL):
    """dsm_window_step_batch: per job the dict of StepBatch.results"""
    b = StepBatch(jobs, outputs)
    b.run(ctx, params, step_params)
    return b.results()


def window_step_host(w, h, job, frames, params=None, step_params=None, outputs=OPTIONAL):
    """dsm_window_step_host (no device): the same dict for one job"""
    b = StepBatch([job], outputs)
    b.run_host(w, h, 0, frames, params, step_params)
    return b.results()[0]
