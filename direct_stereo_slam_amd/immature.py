"""The second half of FrontEnd::activatePointsMT (FrontEnd.cpp:458-468) on the device: FrontEnd::optimizeImmaturePoint
(dso_helpers/FrontEndOptPoint.cpp:35-138) for the selected points of the windows of many sequences in one call -- the ctypes mirror
of dsm_window_* / dsm_optimize_immature_points_batch, and of the host form dsm_optimize_immature_points_host.  Semantics: DESIGN.md
section 13 (M1-M8, U1-U9).

A job is a dict: window (a KeyframeWindow; not needed by the host form), cam (fxl, fyl, cxl, cyl), cam_inv (fxli, fyli), frame_ids,
pre_R (n x n x 9, [host][target]), pre_t (n x n x 3), pre_aff (n x n x 2), host, u, v, idepth_min, idepth_max, energy_th,
color (n_pts x 8), weights (n_pts x 8), min_obs (default 1)."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import c_float_p, c_int_p, check

HUBER_TH, MIN_IDEPTH_H_ACT, GN_ITERATIONS = 9.0, 100.0, 3  # DSM_IMMATURE_*: the upstream defaults
RES_IN, RES_OOB, RES_OUTLIER, RES_HOST = 0, 1, 2, 255


class KeyframeWindow:
    """one dsm_window: the level-0 intensity planes of up to `capacity` keyframes on the device"""

    def __init__(self, ctx, w, h, capacity):
        self.ctx, self.L, self.w, self.h = ctx, ctx.L, int(w), int(h)
        win = C.c_void_p()
        check(self.L.dsm_window_create(ctx.h, self.w, self.h, int(capacity), C.byref(win)))
        self.win = win

    def close(self):
        if getattr(self, "win", None):
            self.L.dsm_window_destroy(self.win)
            self.win = None

    def __del__(self):
        self.close()

    def put_host(self, frame_id, image):
        a = np.ascontiguousarray(image, np.float32)
        if a.size != self.w * self.h:
            raise ValueError("KeyframeWindow.put_host: the image is not w * h")
        check(self.L.dsm_window_put_host(self.win, int(frame_id), a.ctypes.data_as(c_float_p)))

    def put_from_tracker(self, frame_id, tracker, slot):
        """level 0 of the frame resident in `slot` of a TrackerAndScaler, copied on the device"""
        check(self.L.dsm_window_put_from_tracker(self.win, int(frame_id), tracker.h, int(slot)))

    def drop(self, frame_id):
        check(self.L.dsm_window_drop(self.win, int(frame_id)))

    def get(self, frame_id):
        out = np.empty((self.h, self.w), np.float32)
        check(self.L.dsm_window_get(self.win, int(frame_id), out.ctypes.data_as(c_float_p)))
        return out


def _f(a, shape=-1):
    return np.ascontiguousarray(a, np.float32).reshape(shape)


def _i(a):
    return np.ascontiguousarray(a, np.int32).reshape(-1)


class ImmatureBatch:
    """The ctypes job table of dsm_optimize_immature_points_batch and its output arrays, built once: `run()` is the C call alone
    (tools/point_optimisation_timing.py times it), `results()` unpacks."""

    def __init__(self, jobs):
        self.arr = (_lib.ImmatureJob * max(1, len(jobs)))()
        self.n = len(jobs)
        self.keep, self.outs = [], []
        for J, job in zip(self.arr, jobs):
            ids = _i(job["frame_ids"])
            nf = len(ids)
            pre = [_f(job["pre_R"]), _f(job["pre_t"]), _f(job["pre_aff"])]
            if [len(a) for a in pre] != [9 * nf * nf, 3 * nf * nf, 2 * nf * nf]:
                raise ValueError("immature job: pre_R / pre_t / pre_aff are not n_frames x n_frames x 9 / 3 / 2")
            host = _i(job["host"])
            n = len(host)
            per = [_f(job[k]) for k in ("u", "v", "idepth_min", "idepth_max", "energy_th")]
            col, wts = _f(job["color"]), _f(job["weights"])
            if any(len(a) != n for a in per) or len(col) != 8 * n or len(wts) != 8 * n:
                raise ValueError("immature job: per-point arrays of unequal length")
            m = max(1, n)
            out = dict(status=np.full(m, 77, np.uint8), idepth=np.full(m, -1, np.float32), res_state=np.full((m, nf), 77, np.uint8),
                       hdd=np.full(m, -1, np.float32), bd=np.full(m, -1, np.float32), energy=np.full(m, -1, np.float32),
                       iterations=np.full(m, -1, np.int32))
            self.keep.append((ids, pre, host, per, col, wts, job.get("window")))
            self.outs.append((out, n))
            J.window = job["window"].win if job.get("window") is not None else None
            J.cam = (C.c_float * 4)(*[float(x) for x in job["cam"]])
            J.cam_inv = (C.c_float * 2)(*[float(x) for x in job["cam_inv"]])
            J.n_frames, J.frame_ids = nf, ids.ctypes.data_as(c_int_p)
            J.pre_R, J.pre_t, J.pre_aff = (a.ctypes.data_as(c_float_p) for a in pre)
            J.n_pts, J.host = n, host.ctypes.data_as(c_int_p)
            J.u, J.v, J.idepth_min, J.idepth_max, J.energy_th = (a.ctypes.data_as(c_float_p) for a in per)
            J.color, J.weights = col.ctypes.data_as(c_float_p), wts.ctypes.data_as(c_float_p)
            J.min_obs = int(job.get("min_obs", 1))
            J.status = out["status"].ctypes.data_as(C.POINTER(C.c_ubyte))
            J.idepth_out = out["idepth"].ctypes.data_as(c_float_p)
            J.res_state = out["res_state"].ctypes.data_as(C.POINTER(C.c_ubyte))
            J.hdd_out, J.bd_out, J.energy_out = (out[k].ctypes.data_as(c_float_p) for k in ("hdd", "bd", "energy"))
            J.iterations_out = out["iterations"].ctypes.data_as(c_int_p)

    def run(self, ctx, huber_th=HUBER_TH, min_idepth_h_act=MIN_IDEPTH_H_ACT, gn_iterations=GN_ITERATIONS):
        """one dsm_optimize_immature_points_batch call"""
        check(ctx.L.dsm_optimize_immature_points_batch(ctx.h, self.n, self.arr, huber_th, min_idepth_h_act, int(gn_iterations)))

    def run_host(self, w, h, j, frames, huber_th=HUBER_TH, min_idepth_h_act=MIN_IDEPTH_H_ACT, gn_iterations=GN_ITERATIONS):
        """dsm_optimize_immature_points_host on job j; frames: the level-0 planes in frame_ids order"""
        planes = [np.ascontiguousarray(f, np.float32) for f in frames]
        ptrs = (c_float_p * max(1, len(planes)))(*[p.ctypes.data_as(c_float_p) for p in planes])
        check(_lib.load().dsm_optimize_immature_points_host(int(w), int(h), C.byref(self.arr[j]), ptrs, huber_th, min_idepth_h_act,
                                                            int(gn_iterations)))

    def results(self):
        """per job a dict of arrays over its points: status, idepth, res_state (n_pts x n_frames), hdd, bd, energy, iterations"""
        return [{k: v[:n].copy() for k, v in out.items()} for out, n in self.outs]


def optimize_immature_points_batch(ctx, jobs, huber_th=HUBER_TH, min_idepth_h_act=MIN_IDEPTH_H_ACT, gn_iterations=GN_ITERATIONS):
    """dsm_optimize_immature_points_batch: per job a dict with status (0 not yet, 1 activated, 2 delete), idepth, res_state
    (RES_IN / RES_OOB / RES_OUTLIER per frame, RES_HOST in the host's column), hdd, bd, energy, iterations"""
    b = ImmatureBatch(jobs)
    b.run(ctx, huber_th, min_idepth_h_act, gn_iterations)
    return b.results()


def optimize_immature_points_host(w, h, job, frames, huber_th=HUBER_TH, min_idepth_h_act=MIN_IDEPTH_H_ACT, gn_iterations=GN_ITERATIONS):
    """dsm_optimize_immature_points_host (no device): the same dict for one job"""
    b = ImmatureBatch([job])
    b.run_host(w, h, 0, frames, huber_th, min_idepth_h_act, gn_iterations)
    return b.results()[0]
