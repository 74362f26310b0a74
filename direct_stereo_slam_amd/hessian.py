"""accumulateAF_MT / accumulateSCF_MT of FrontEnd::optimize (dso_helpers/FrontEndOptimize.cpp:332-486) on the device, after the
linearisation of the same pass -- the ctypes mirror of dsm_window_hessian_batch and of the host form dsm_window_hessian_host.
Semantics: DESIGN.md section 17 (A0-A3, P1, S1-S3, T1, V).

A job is a linearize job (direct_stereo_slam_amd.linearize) with, on top: ad_host, ad_target (n x n x 8 x 8 doubles, [host][target]),
the optional per-point inputs prior, delta, hdd_lin, bd_lin (n_pts) and hcd_lin (n_pts x 4), and shift_prior_to_zero (default 1)."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import c_double_p, c_float_p, check
from .linearize import OPTIONAL as LIN_OPTIONAL
from .linearize import KeyframeWindow, LinearizeBatch, default_params  # noqa: F401  (the window type and the settings of this call)

c_ubyte_p = C.POINTER(C.c_ubyte)
PER_POINT_IN = (("prior", 1), ("delta", 1), ("hdd_lin", 1), ("bd_lin", 1), ("hcd_lin", 4))
RAW = ("acc_top", "acc_D", "acc_E", "acc_EB", "acc_Hcc", "acc_bc")
PER_RESIDUAL = ("active", "JpJdF")
PER_POINT = ("hdd_acc", "bd_acc", "hcd_acc", "hdi", "bd_sum", "idepth_hessian")
OPTIONAL = RAW + PER_RESIDUAL + PER_POINT + tuple(k for k in LIN_OPTIONAL if k != "J")  # lin.J_out is normally NULL
FILL = -7.0


class HessianBatch:
    """The ctypes job table of dsm_window_hessian_batch and its output arrays, built once: `run()` is the C call alone
    (tools/hessian_timing.py times it), `results()` unpacks.  outputs: which of the optional outputs the jobs ask for ("J" and the
    other names of linearize.OPTIONAL among them)."""

    def __init__(self, jobs, outputs=OPTIONAL):
        self.lin = LinearizeBatch(jobs, [k for k in outputs if k in LIN_OPTIONAL])
        self.arr = (_lib.HessianJob * max(1, len(jobs)))()
        self.n = len(jobs)
        self.keep, self.outs = [], []
        for j, (H, job) in enumerate(zip(self.arr, jobs)):
            H.lin = self.lin.arr[j]
            nf, n, nr = H.lin.n_frames, H.lin.n_pts, H.lin.n_res
            N, mp, mr = 4 + 8 * nf, max(1, n), max(1, nr)
            ad = [np.ascontiguousarray(job[k], np.float64).reshape(-1) if job.get(k) is not None else None for k in ("ad_host", "ad_target")]
            if any(a is not None and len(a) != nf * nf * 64 for a in ad):
                raise ValueError("hessian job: ad_host / ad_target is not n_frames x n_frames x 8 x 8")
            H.ad_host, H.ad_target = (a.ctypes.data_as(c_double_p) if a is not None else None for a in ad)
            ins = []
            for k, m in PER_POINT_IN:
                a = np.ascontiguousarray(job[k], np.float32).reshape(-1) if job.get(k) is not None else None
                if a is not None and len(a) != m * n:
                    raise ValueError(f"hessian job: {k} is not n_pts x {m}")
                setattr(H, k, a.ctypes.data_as(c_float_p) if a is not None else None)
                ins.append(a)
            H.shift_prior_to_zero = int(job.get("shift_prior_to_zero", 1))
            out = dict(H_A=np.full((N, N), FILL), b_A=np.full(N, FILL), H_sc=np.full((N, N), FILL), b_sc=np.full(N, FILL),
                       acc_top=np.full((nf, nf, 13, 13), FILL), acc_D=np.full((nf, nf, nf, 8, 8), FILL), acc_E=np.full((nf, nf, 8, 4), FILL),
                       acc_EB=np.full((nf, nf, 8), FILL), acc_Hcc=np.full((4, 4), FILL), acc_bc=np.full(4, FILL),
                       active=np.full(mr, 77, np.uint8), JpJdF=np.full((mr, 8), FILL, np.float32),
                       hdd_acc=np.full(mp, FILL, np.float32), bd_acc=np.full(mp, FILL, np.float32), hcd_acc=np.full((mp, 4), FILL, np.float32),
                       hdi=np.full(mp, FILL, np.float32), bd_sum=np.full(mp, FILL, np.float32), idepth_hessian=np.full(mp, FILL, np.float32))
            for k in ("H_A", "b_A", "H_sc", "b_sc"):
                setattr(H, k, out[k].ctypes.data_as(c_double_p))
            for k in RAW:
                setattr(H, k, out[k].ctypes.data_as(c_double_p) if k in outputs else None)
            H.active = out["active"].ctypes.data_as(c_ubyte_p) if "active" in outputs else None
            for k in ("JpJdF",) + PER_POINT:
                setattr(H, k, out[k].ctypes.data_as(c_float_p) if k in outputs else None)
            self.keep.append((ad, ins))
            self.outs.append((out, n, nr))

    def run(self, ctx, params=None):
        """one dsm_window_hessian_batch call"""
        p = params if params is not None else default_params()
        check(ctx.L.dsm_window_hessian_batch(ctx.h, self.n, self.arr, C.byref(p)))

    def run_host(self, w, h, j, frames, params=None):
        """dsm_window_hessian_host on job j; frames: the level-0 planes in frame_ids order"""
        p = params if params is not None else default_params()
        planes = [np.ascontiguousarray(f, np.float32) for f in frames]
        ptrs = (c_float_p * max(1, len(planes)))(*[a.ctypes.data_as(c_float_p) for a in planes])
        check(_lib.load().dsm_window_hessian_host(int(w), int(h), C.byref(self.arr[j]), ptrs, C.byref(p)))

    def all_outputs(self):
        """per job every output array itself (the linearisation's among them), for callers that compare them before and after a call"""
        return [dict(lo, **ho) for (lo, _), (ho, _, _) in zip(self.lin.outs, self.outs)]

    def results(self):
        """per job a dict: the linearisation's results (linearize.LinearizeBatch.results) and, on top, H_A, b_A, H_sc, b_sc, the raw
        accumulators, active and JpJdF over the residuals and the per-point arrays; what was not asked for, or not written, keeps the
        mirror's fill value"""
        res = self.lin.results()
        for d, (out, n, nr) in zip(res, self.outs):
            for k, v in out.items():
                d[k] = v[:nr].copy() if k in PER_RESIDUAL else v[:n].copy() if k in PER_POINT else v.copy()
        return res


def window_hessian_batch(ctx, jobs, params=None, outputs=OPTIONAL):
    """dsm_window_hessian_batch: per job the dict of HessianBatch.results"""
    b = HessianBatch(jobs, outputs)
    b.run(ctx, params)
    return b.results()


def window_hessian_host(w, h, job, frames, params=None, outputs=OPTIONAL):
    """dsm_window_hessian_host (no device): the same dict for one job"""
    b = HessianBatch([job], outputs)
    b.run_host(w, h, 0, frames, params)
    return b.results()[0]
