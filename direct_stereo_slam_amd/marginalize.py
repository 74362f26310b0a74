"""What FrontEnd::makeKeyFrame does right after optimize (FrontEnd.cpp:816-839) on the device: the verdicts of flagPointsForRemoval,
marginalizePointsF and marginalizeFrame -- the ctypes mirror of dsm_window_marginalize_batch and of the host form
dsm_window_marginalize_host.  Semantics: DESIGN.md section 21 (C, M1, X1, A1', M2, G1-G7, Z, V).

A job is a hessian job (direct_stereo_slam_amd.hessian) that describes the whole window as optimize left it, with, on top: flagged
(n), n_good_residuals (n_pts), last_state (n_pts x 2), idepth_hessian (n_pts, an INPUT here), ad_ht_delta (n x n x 8 floats), c_delta
(4), the optional H_M (N x N doubles) and b_M (N), marg_frames (strictly ascending frame indices; default none) with frame_prior and
frame_delta_prior (8 doubles per marginalised frame); N = 4 + 8 n_frames.  The returned H_M_out / b_M_out are the H_M / b_M of the
next keyframe's solve job over the frames that stay."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import c_double_p, c_float_p, c_int_p, check
from .hessian import FILL, HessianBatch
from .hessian import OPTIONAL as HES_OPTIONAL
from .linearize import KeyframeWindow, default_params  # noqa: F401  (the window type and the linearisation's settings of this call)

c_ubyte_p = C.POINTER(C.c_ubyte)
KEEP, MARGINALIZE, DROP = 0, 1, 2
STITCHED = ("H_A", "b_A", "H_sc", "b_sc")
OWN_OPTIONAL = ("H_M_points", "b_M_points", "res_to_zero")
OPTIONAL = OWN_OPTIONAL + STITCHED + tuple(k for k in HES_OPTIONAL if k not in ("keep", "rel_bs"))  # lin.J_out, keep, rel_bs must be NULL


def default_marg_params(**kw):
    """dsm_marginalize_params with the defaults, then the given fields"""
    p = _lib.MarginalizeParams()
    if _lib.load().dsm_marginalize_params_default(C.byref(p)) != 0:
        raise _lib.DsmError("dsm_marginalize_params_default failed")
    for k, v in kw.items():
        if not hasattr(p, k):
            raise ValueError(f"dsm_marginalize_params has no field {k}")
        setattr(p, k, v)
    return p


class MarginalizeBatch:
    """The ctypes job table of dsm_window_marginalize_batch and its output arrays, built once: `run()` is the C call alone
    (tools/marginalize_timing.py times it), `results()` unpacks.  outputs: which of the optional outputs the jobs ask for."""

    def __init__(self, jobs, outputs=OPTIONAL):
        self.hes = HessianBatch(jobs, [k for k in outputs if k in HES_OPTIONAL])
        self.arr = (_lib.MarginalizeJob * max(1, len(jobs)))()
        self.n = len(jobs)
        self.keep, self.outs = [], []
        for j, (M, job) in enumerate(zip(self.arr, jobs)):
            M.hes = self.hes.arr[j]
            for k in STITCHED:
                if k not in outputs:
                    setattr(M.hes, k, None)
            nf, n, nr = M.hes.lin.n_frames, M.hes.lin.n_pts, M.hes.lin.n_res
            N = 4 + 8 * nf
            ins = {}

            def take(k, dtype, size, ptr):
                a = np.ascontiguousarray(job[k], dtype).reshape(-1) if job.get(k) is not None else None
                if a is not None and len(a) != size:
                    raise ValueError(f"marginalize job: {k} has {len(a)} entries, not {size}")
                setattr(M, k, a.ctypes.data_as(ptr) if a is not None else None)
                ins[k] = a

            marg = np.ascontiguousarray(job.get("marg_frames", ()), np.int32).reshape(-1)
            nm = len(marg)
            take("flagged", np.uint8, nf, c_ubyte_p), take("n_good_residuals", np.int32, n, c_int_p), take("last_state", np.uint8, 2 * n, c_ubyte_p)
            take("idepth_hessian", np.float32, n, c_float_p), take("ad_ht_delta", np.float32, nf * nf * 8, c_float_p)
            take("c_delta", np.float32, 4, c_float_p), take("H_M", np.float64, N * N, c_double_p), take("b_M", np.float64, N, c_double_p)
            take("frame_prior", np.float64, 8 * nm, c_double_p), take("frame_delta_prior", np.float64, 8 * nm, c_double_p)
            M.n_marg_frames = int(job.get("n_marg_frames", nm))
            M.marg_frames = marg.ctypes.data_as(c_int_p)
            ins["marg_frames"] = marg
            Nn = max(4, N - 8 * nm)
            out = dict(verdict=np.full(max(1, n), 77, np.uint8), H_M_out=np.full((Nn, Nn), FILL), b_M_out=np.full(Nn, FILL),
                       n_res_marg=np.full(1, -7, np.int32), H_M_points=np.full((N, N), FILL), b_M_points=np.full(N, FILL),
                       res_to_zero=np.full((max(1, nr), 8), FILL, np.float32))
            M.verdict = out["verdict"].ctypes.data_as(c_ubyte_p)
            M.H_M_out, M.b_M_out = out["H_M_out"].ctypes.data_as(c_double_p), out["b_M_out"].ctypes.data_as(c_double_p)
            M.n_res_marg = out["n_res_marg"].ctypes.data_as(c_int_p)
            for k in ("H_M_points", "b_M_points"):
                setattr(M, k, out[k].ctypes.data_as(c_double_p) if k in outputs else None)
            M.res_to_zero = out["res_to_zero"].ctypes.data_as(c_float_p) if "res_to_zero" in outputs else None
            self.keep.append(ins)
            self.outs.append((out, n, nr))

    def run(self, ctx, params=None, marg_params=None):
        """one dsm_window_marginalize_batch call"""
        p = params if params is not None else default_params()
        mp = marg_params if marg_params is not None else default_marg_params()
        check(ctx.L.dsm_window_marginalize_batch(ctx.h, self.n, self.arr, C.byref(p), C.byref(mp)))

    def run_host(self, w, h, j, frames, params=None, marg_params=None):
        """dsm_window_marginalize_host on job j; frames: the level-0 planes in frame_ids order"""
        p = params if params is not None else default_params()
        mp = marg_params if marg_params is not None else default_marg_params()
        planes = [np.ascontiguousarray(f, np.float32) for f in frames]
        ptrs = (c_float_p * max(1, len(planes)))(*[a.ctypes.data_as(c_float_p) for a in planes])
        check(_lib.load().dsm_window_marginalize_host(int(w), int(h), C.byref(self.arr[j]), ptrs, C.byref(p), C.byref(mp)))

    def all_outputs(self):
        """per job every output array itself (the Hessian call's and the linearisation's among them)"""
        return [dict(ho, **mo) for ho, (mo, _, _) in zip(self.hes.all_outputs(), self.outs)]

    def results(self):
        """per job a dict: HessianBatch.results (every per-residual and per-point array indexed as the window's, written for the
        sub-window only) and, on top, verdict, H_M_out, b_M_out, n_res_marg (an int), H_M_points, b_M_points, res_to_zero; what was
        not asked for, or not written, keeps the mirror's fill value"""
        res = self.hes.results()
        for d, (out, n, nr) in zip(res, self.outs):
            for k, v in out.items():
                d[k] = v[:n].copy() if k == "verdict" else v[:nr].copy() if k == "res_to_zero" else int(v[0]) if k == "n_res_marg" else v.copy()
        return res


def window_marginalize_batch(ctx, jobs, params=None, marg_params=None, outputs=OPTIONAL):
    """dsm_window_marginalize_batch: per job the dict of MarginalizeBatch.results"""
    b = MarginalizeBatch(jobs, outputs)
    b.run(ctx, params, marg_params)
    return b.results()


def window_marginalize_host(w, h, job, frames, params=None, marg_params=None, outputs=OPTIONAL):
    """dsm_window_marginalize_host (no device): the same dict for one job"""
    b = MarginalizeBatch([job], outputs)
    b.run_host(w, h, 0, frames, params, marg_params)
    return b.results()[0]
