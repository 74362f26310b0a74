"""What FrontEnd::makeKeyFrame does between removeOutliers and flagPointsForRemoval (FrontEnd.cpp:806): FrontEnd::optimizeScale behind
its scale search (FrontEnd.cpp:1010-1061) -- the ctypes mirror of dsm_window_rescale_batch and of the host form
dsm_window_rescale_host.  Semantics: DESIGN.md section 25 (S0-S6, V).

A job is a dict with the fields of dsm_rescale_job under their names: the scalars enabled, scale_error, new_scale, thres, trapped,
fails and aff_g2l (2), the points' idepth, idepth_scaled, idepth_zero_scaled and delta, the frames' world_to_cam_eval (n x 7), state,
state_zero (n x 8) and exposure, the newest frame's cam_to_tracking_ref, ref_cam_to_world and cam_to_world (7 each), calib_value and
calib_zero, ad_host and ad_target, and the given pre_* tables, cam, c_delta, delta_x, ad_ht_delta, world_to_cam and (optional)
cam_to_world_all.  A result dict names every output without its _out: its arrays are what dsm_marginalize_job, dsm_nullspace_job and the
next keyframe's dsm_step_job take."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import c_double_p, c_float_p, check

FILL = -7777.0
DISABLED, REJECTED, ACCEPTED = 0, 1, 2
PRE = (("pre_RTll_0", 9), ("pre_tTll_0", 3), ("pre_KRKiTll", 9), ("pre_KtTll", 3), ("pre_aff_mode", 2), ("pre_b0_mode", 1))
WORDS = ("decision", "scale_error_out", "trapped_out", "fails_out", "applied_scale")


def layout(n, n_pts):
    """(name, dtype, entries) of every array that has an input and an output"""
    n2, N = n * n, 4 + 8 * n
    f, d = np.float32, np.float64
    return ([(k, f, n_pts) for k in ("idepth", "idepth_scaled", "idepth_zero_scaled", "delta")]
            + [("world_to_cam_eval", d, 7 * n), ("state", d, 8 * n), ("state_zero", d, 8 * n), ("cam_to_tracking_ref", d, 7), ("cam_to_world", d, 7)]
            + [(k, f, m * n2) for k, m in PRE]
            + [("cam", f, 6), ("c_delta", f, 4), ("delta_x", d, N), ("ad_ht_delta", f, 8 * n2), ("world_to_cam", d, 7 * n), ("cam_to_world_all", d, 7 * n)])


def out_name(k):
    return "cam_to_world_out_all" if k == "cam_to_world_all" else k + "_out"


def geometry():
    """(workgroup size, the points' grid stride) of rsc_kernel"""
    b, s = C.c_int(0), C.c_int(0)
    check(_lib.load().dsm_rescale_geometry(C.byref(b), C.byref(s)))
    return b.value, s.value


class RescaleBatch:
    """The ctypes job table of dsm_window_rescale_batch and its output arrays, built once: `run()` is the C call alone
    (tools/rescale_timing.py times it), `results()` unpacks.  A job may carry n_frames and n_pts (otherwise the rows of state and the
    length of idepth), drop: the name of a required array (input, or output with its _out) to leave NULL (the tests of V), and
    all_poses=False to leave cam_to_world_out_all NULL."""

    def __init__(self, jobs):
        self.arr = (_lib.RescaleJob * max(1, len(jobs)))()
        self.n = len(jobs)
        self.keep, self.outs = [], []
        for S, job in zip(self.arr, jobs):
            n = np.asarray(job["state"]).reshape(-1, 8).shape[0] if job.get("state") is not None else 1
            n_pts = np.asarray(job["idepth"]).reshape(-1).shape[0] if job.get("idepth") is not None else 0
            drop = job.get("drop")
            ins, out = {}, {}

            def take(k, dtype, size):
                a = np.ascontiguousarray(job[k], dtype).reshape(-1) if job.get(k) is not None and k != drop else None
                if a is not None and len(a) != size:
                    raise ValueError(f"rescale job: {k} has {len(a)} entries, not {size}")
                setattr(S, k, a.ctypes.data_as(c_double_p if dtype == np.float64 else c_float_p) if a is not None else None)
                ins[k] = a

            for k, dtype, size in layout(n, n_pts):
                take(k, dtype, size)
                o = out_name(k)
                out[o] = np.full(size, FILL, dtype)
                given = o != drop and (k != "cam_to_world_all" or job.get("all_poses", True))
                setattr(S, o, out[o].ctypes.data_as(c_double_p if dtype == np.float64 else c_float_p) if given else None)
            n2 = n * n
            take("exposure", np.float32, n), take("ref_cam_to_world", np.float64, 7), take("calib_value", np.float64, 4)
            take("calib_zero", np.float64, 4), take("ad_host", np.float64, 64 * n2), take("ad_target", np.float64, 64 * n2)
            S.n_frames, S.n_pts = int(job.get("n_frames", n)), int(job.get("n_pts", n_pts))
            S.enabled, S.scale_error, S.new_scale, S.thres = int(job["enabled"]), float(job["scale_error"]), float(job["new_scale"]), float(job["thres"])
            S.trapped, S.fails = int(job["trapped"]), int(job["fails"])
            S.aff_g2l[0], S.aff_g2l[1] = float(job["aff_g2l"][0]), float(job["aff_g2l"][1])
            for k in WORDS:
                dtype = np.float32 if k in ("scale_error_out", "applied_scale") else np.int32
                out[k] = np.full(1, 77, dtype)
                ptr = c_float_p if dtype == np.float32 else _lib.c_int_p
                setattr(S, k, out[k].ctypes.data_as(ptr) if k != drop else None)
            self.keep.append(ins)
            self.outs.append(out)

    def run(self, ctx, lp=None, sp=None):
        """one dsm_window_rescale_batch call; a parameter set None: the C side's defaults (a NULL pointer)"""
        check(ctx.L.dsm_window_rescale_batch(ctx.h, self.n, self.arr, C.byref(lp) if lp is not None else None, C.byref(sp) if sp is not None else None))

    def run_host(self, lp=None, sp=None):
        """dsm_window_rescale_host on every job"""
        check(_lib.load().dsm_window_rescale_host(self.n, self.arr, C.byref(lp) if lp is not None else None, C.byref(sp) if sp is not None else None))

    def all_outputs(self):
        """per job every output array itself, under the C field's name"""
        return self.outs

    def results(self):
        """per job a dict: every array under its input's name, and decision, scale_error, trapped, fails, applied_scale"""
        res = []
        for out in self.outs:
            r = {}
            for o, v in out.items():
                if o in WORDS:
                    r[o[:-4] if o.endswith("_out") else o] = int(v[0]) if v.dtype == np.int32 else np.float32(v[0])
                else:
                    r["cam_to_world_all" if o == "cam_to_world_out_all" else o[:-4]] = v.copy()
            res.append(r)
        return res


def window_rescale_batch(ctx, jobs, lp=None, sp=None):
    """dsm_window_rescale_batch: per job the dict of RescaleBatch.results"""
    b = RescaleBatch(jobs)
    b.run(ctx, lp, sp)
    return b.results()


def window_rescale_host(jobs, lp=None, sp=None):
    """dsm_window_rescale_host (no device): the same dicts"""
    b = RescaleBatch(jobs)
    b.run_host(lp, sp)
    return b.results()
