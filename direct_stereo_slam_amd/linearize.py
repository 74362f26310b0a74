"""FrontEnd::linearizeAll (dso_helpers/FrontEndOptimize.cpp:121-179) on the device: PointFrameResidual::linearize for every active
residual of the windows of many sequences in one call -- the ctypes mirror of dsm_linearize_residuals_batch and of the host form
dsm_linearize_residuals_host.  Semantics: DESIGN.md section 16 (L1-L8, B1-B4).  The windows are immature.KeyframeWindow.

A job is a dict: window (a KeyframeWindow; not needed by the host form), cam (fxl, fyl, cxl, cyl), cam_inv (fxli, fyli), frame_ids,
the six precalc tables over [host][target] (pre_RTll_0 n x n x 9, pre_tTll_0 n x n x 3, pre_KRKiTll n x n x 9, pre_KtTll n x n x 3,
pre_aff_mode n x n x 2, pre_b0_mode n x n), frame_energy_th (n), the points (host, u, v, idepth_scaled, idepth_zero_scaled,
color n_pts x 8, weights n_pts x 8), the residuals (point, target, state_in, energy_in, is_new) and fix_linearization (default 0)."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import c_float_p, c_int_p, check
from .immature import RES_IN, RES_OOB, RES_OUTLIER, KeyframeWindow  # noqa: F401  (the window type and the states of this call)

J_FLOATS = 74  # DSM_LINEARIZE_J_FLOATS
c_ubyte_p = C.POINTER(C.c_ubyte)
PRE = (("pre_RTll_0", 9), ("pre_tTll_0", 3), ("pre_KRKiTll", 9), ("pre_KtTll", 3), ("pre_aff_mode", 2), ("pre_b0_mode", 1))
OPTIONAL = ("J", "center_projected_to", "projected_to", "keep", "rel_bs")


def default_params(**kw):
    """dsm_linearize_params with the upstream defaults, then the given fields"""
    p = _lib.LinearizeParams()
    if _lib.load().dsm_linearize_params_default(C.byref(p)) != 0:
        raise _lib.DsmError("dsm_linearize_params_default failed")
    for k, v in kw.items():
        if not hasattr(p, k):
            raise ValueError(f"dsm_linearize_params has no field {k}")
        setattr(p, k, v)
    return p


def _f(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1)


def _i(a):
    return np.ascontiguousarray(a, np.int32).reshape(-1)


def _b(a):
    return np.ascontiguousarray(a, np.uint8).reshape(-1)


class LinearizeBatch:
    """The ctypes job table of dsm_linearize_residuals_batch and its output arrays, built once: `run()` is the C call alone
    (tools/linearize_timing.py times it), `results()` unpacks.  outputs: which of the optional outputs the jobs ask for."""

    def __init__(self, jobs, outputs=OPTIONAL):
        self.arr = (_lib.LinearizeJob * max(1, len(jobs)))()
        self.n = len(jobs)
        self.keep, self.outs = [], []
        for J, job in zip(self.arr, jobs):
            ids = _i(job["frame_ids"])
            nf = len(ids)
            pre = [_f(job[k]) for k, _ in PRE]
            if [len(a) for a in pre] != [m * nf * nf for _, m in PRE]:
                raise ValueError("linearize job: a precalc table is not n_frames x n_frames x its width")
            eth = _f(job["frame_energy_th"])
            if len(eth) != nf:
                raise ValueError("linearize job: frame_energy_th is not n_frames long")
            host = _i(job["host"])
            n = len(host)
            per = [_f(job[k]) for k in ("u", "v", "idepth_scaled", "idepth_zero_scaled")]
            col, wts = _f(job["color"]), _f(job["weights"])
            if any(len(a) != n for a in per) or len(col) != 8 * n or len(wts) != 8 * n:
                raise ValueError("linearize job: per-point arrays of unequal length")
            point, target = _i(job["point"]), _i(job["target"])
            nr = len(point)
            state_in, energy_in, is_new = _b(job["state_in"]), _f(job["energy_in"]), _b(job["is_new"])
            if any(len(a) != nr for a in (target, state_in, energy_in, is_new)):
                raise ValueError("linearize job: per-residual arrays of unequal length")
            m = max(1, nr)
            out = dict(new_state=np.full(m, 77, np.uint8), new_energy=np.full(m, -7, np.float32),
                       new_energy_with_outlier=np.full(m, -7, np.float32), J=np.full((m, J_FLOATS), -7, np.float32),
                       center_projected_to=np.full((m, 3), -7, np.float32), projected_to=np.full((m, 16), -7, np.float32),
                       keep=np.full(m, 77, np.uint8), rel_bs=np.full(m, -7, np.float32), energy=np.full(1, -7, np.float64),
                       new_frame_energy_th=np.full(1, -7, np.float32))
            self.keep.append((ids, pre, eth, host, per, col, wts, point, target, state_in, energy_in, is_new, job.get("window")))
            self.outs.append((out, nr))
            J.window = job["window"].win if job.get("window") is not None else None
            J.cam = (C.c_float * 4)(*[float(x) for x in job["cam"]])
            J.cam_inv = (C.c_float * 2)(*[float(x) for x in job["cam_inv"]])
            J.n_frames, J.frame_ids = nf, ids.ctypes.data_as(c_int_p)
            for (k, _), a in zip(PRE, pre):
                setattr(J, k, a.ctypes.data_as(c_float_p))
            J.frame_energy_th = eth.ctypes.data_as(c_float_p)
            J.n_pts, J.host = n, host.ctypes.data_as(c_int_p)
            J.u, J.v, J.idepth_scaled, J.idepth_zero_scaled = (a.ctypes.data_as(c_float_p) for a in per)
            J.color, J.weights = col.ctypes.data_as(c_float_p), wts.ctypes.data_as(c_float_p)
            J.n_res, J.point, J.target = nr, point.ctypes.data_as(c_int_p), target.ctypes.data_as(c_int_p)
            J.state_in, J.energy_in, J.is_new = state_in.ctypes.data_as(c_ubyte_p), energy_in.ctypes.data_as(c_float_p), is_new.ctypes.data_as(c_ubyte_p)
            J.fix_linearization = int(job.get("fix_linearization", 0))
            J.new_state = out["new_state"].ctypes.data_as(c_ubyte_p)
            J.new_energy, J.new_energy_with_outlier = (out[k].ctypes.data_as(c_float_p) for k in ("new_energy", "new_energy_with_outlier"))
            J.J_out = out["J"].ctypes.data_as(c_float_p) if "J" in outputs else None
            J.center_projected_to = out["center_projected_to"].ctypes.data_as(c_float_p) if "center_projected_to" in outputs else None
            J.projected_to = out["projected_to"].ctypes.data_as(c_float_p) if "projected_to" in outputs else None
            J.keep = out["keep"].ctypes.data_as(c_ubyte_p) if "keep" in outputs else None
            J.rel_bs = out["rel_bs"].ctypes.data_as(c_float_p) if "rel_bs" in outputs else None
            J.energy_out = out["energy"].ctypes.data_as(_lib.c_double_p)
            J.new_frame_energy_th_out = out["new_frame_energy_th"].ctypes.data_as(c_float_p)

    def run(self, ctx, params=None):
        """one dsm_linearize_residuals_batch call"""
        p = params if params is not None else default_params()
        check(ctx.L.dsm_linearize_residuals_batch(ctx.h, self.n, self.arr, C.byref(p)))

    def run_host(self, w, h, j, frames, params=None):
        """dsm_linearize_residuals_host on job j; frames: the level-0 planes in frame_ids order"""
        p = params if params is not None else default_params()
        planes = [np.ascontiguousarray(f, np.float32) for f in frames]
        ptrs = (c_float_p * max(1, len(planes)))(*[a.ctypes.data_as(c_float_p) for a in planes])
        check(_lib.load().dsm_linearize_residuals_host(int(w), int(h), C.byref(self.arr[j]), ptrs, C.byref(p)))

    def results(self):
        """per job a dict: the arrays over its residuals (new_state, new_energy, new_energy_with_outlier, J, center_projected_to,
        projected_to, keep, rel_bs; what was not asked for, or not written, keeps the mirror's fill value), energy and
        new_frame_energy_th"""
        res = []
        for out, n in self.outs:
            d = {k: v[:n].copy() for k, v in out.items() if k not in ("energy", "new_frame_energy_th")}
            d["energy"], d["new_frame_energy_th"] = out["energy"][0], out["new_frame_energy_th"][0]
            res.append(d)
        return res


def linearize_residuals_batch(ctx, jobs, params=None, outputs=OPTIONAL):
    """dsm_linearize_residuals_batch: per job the dict of LinearizeBatch.results"""
    b = LinearizeBatch(jobs, outputs)
    b.run(ctx, params)
    return b.results()


def linearize_residuals_host(w, h, job, frames, params=None, outputs=OPTIONAL):
    """dsm_linearize_residuals_host (no device): the same dict for one job"""
    b = LinearizeBatch([job], outputs)
    b.run_host(w, h, 0, frames, params)
    return b.results()[0]
