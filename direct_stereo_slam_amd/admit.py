"""The head of FrontEnd::makeKeyFrame (FrontEnd.cpp:722-762): the new keyframe enters the window -- its pose and evaluation point,
flagFramesForMarginalization (dso_helpers/FrontEndMarginalize.cpp:62-146), insertFrame with setAdjointsF over all pairs,
setPrecalcValues on n + 1 frames and one forward residual per active point -- the ctypes mirror of dsm_window_admit_batch and of the
host form dsm_window_admit_host.  Semantics: DESIGN.md section 26 (A1-A6, V).

A job is a dict with the fields of dsm_admit_job under their names: the scalars new_keyframe_id, new_exposure, new_frame_energy_th and
aff_g2l (2), the old frames' world_to_cam_eval (n x 7), state, state_zero (n x 8), exposure, frame_energy_th, keyframe_id, n_points_in
and n_points_out, the new frame's ref_cam_to_world, cam_to_tracking_ref (7 each), new_frame_prior and new_frame_prior_zero (8 each),
calib_value and calib_zero, the optional H_M, b_M, H_L, b_L, prior and prior_zero, the points' host, last_res and last_state, and the
residuals' point, target, state_in, energy_in and is_new.  A result dict names every output without its _out (res_state for
res_state_out): its arrays are what dsm_step_job, dsm_finish_job, dsm_marginalize_job and dsm_nullspace_job take for n + 1 frames."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check

FILL = -7777.0
FILL_INT = 77
PRE = (("pre_RTll_0", 9), ("pre_tTll_0", 3), ("pre_KRKiTll", 9), ("pre_KtTll", 3), ("pre_aff_mode", 2), ("pre_b0_mode", 1))
WORDS = ("n_res_out", "n_flagged")
OPTIONAL = ("H_M", "b_M", "H_L", "b_L", "prior", "prior_zero")
f32, f64, i32, u8 = np.float32, np.float64, np.int32, np.uint8
_PTR = {f32: _lib.c_float_p, f64: _lib.c_double_p, i32: _lib.c_int_p, u8: _lib.c_ubyte_p}


def inputs(n, n_pts, n_res):
    """(name, dtype, entries) of every input array"""
    N = 4 + 8 * n
    return ([("world_to_cam_eval", f64, 7 * n), ("state", f64, 8 * n), ("state_zero", f64, 8 * n), ("exposure", f32, n), ("frame_energy_th", f32, n),
             ("keyframe_id", i32, n), ("n_points_in", i32, n), ("n_points_out", i32, n), ("ref_cam_to_world", f64, 7), ("cam_to_tracking_ref", f64, 7),
             ("new_frame_prior", f64, 8), ("new_frame_prior_zero", f64, 8), ("calib_value", f64, 4), ("calib_zero", f64, 4),
             ("H_M", f64, N * N), ("b_M", f64, N), ("H_L", f64, N * N), ("b_L", f64, N), ("prior", f64, N), ("prior_zero", f64, N),
             ("host", i32, n_pts), ("last_res", i32, 2 * n_pts), ("last_state", u8, 2 * n_pts),
             ("point", i32, n_res), ("target", i32, n_res), ("state_in", u8, n_res), ("energy_in", f32, n_res), ("is_new", u8, n_res)])


def outputs(n, n_pts, n_res):
    """(name, dtype, entries) of every output array, the two words apart"""
    m, M, no = n + 1, 12 + 8 * n, n_res + n_pts
    m2 = m * m
    return ([("world_to_cam_eval_out", f64, 7 * m), ("state_out", f64, 8 * m), ("state_zero_out", f64, 8 * m), ("exposure_out", f32, m),
             ("frame_energy_th_out", f32, m), ("keyframe_id_out", i32, m), ("world_to_cam_out", f64, 7 * m), ("flagged_out", u8, m),
             ("cam_to_world_out", f64, 7)]
            + [(k + "_out", f32, w * m2) for k, w in PRE]
            + [("distance_ll_out", f32, m2), ("cam_out", f32, 6), ("c_delta_out", f32, 4), ("delta_x_out", f64, M), ("ad_host_out", f64, 64 * m2),
               ("ad_target_out", f64, 64 * m2), ("ad_ht_delta_out", f32, 8 * m2), ("H_M_out", f64, M * M), ("b_M_out", f64, M), ("H_L_out", f64, M * M),
               ("b_L_out", f64, M), ("prior_out", f64, M), ("prior_zero_out", f64, M), ("frame_prior_out", f64, 8), ("frame_delta_prior_out", f64, 8),
               ("point_out", i32, no), ("target_out", i32, no), ("res_state_out", u8, no), ("energy_out", f32, no), ("is_new_out", u8, no),
               ("res_index_out", i32, n_res), ("new_res_index_out", i32, n_pts), ("last_res_out", i32, 2 * n_pts), ("last_state_out", u8, 2 * n_pts),
               ("dist_score_out", f64, n)])


def geometry():
    """(workgroup size, the lists' grid stride) of adm_kernel"""
    b, s = C.c_int(0), C.c_int(0)
    check(_lib.load().dsm_admit_geometry(C.byref(b), C.byref(s)))
    return b.value, s.value


def default_params(**kw):
    p = _lib.AdmitParams()
    _lib.load().dsm_admit_params_default(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise KeyError(k)
        setattr(p, k, v)
    return p


def _fill(dtype):
    return FILL if dtype in (f32, f64) else FILL_INT


class AdmitBatch:
    """The ctypes job table of dsm_window_admit_batch and its output arrays, built once: `run()` is the C call alone
    (tools/admit_timing.py times it), `results()` unpacks.  A job may carry n_frames, n_pts and n_res (otherwise the rows of state and the
    lengths of host and point), drop: the name of an array (input, or output with its _out) to leave NULL (the tests of V), and
    distances=False to leave distance_ll_out NULL.  The output arrays are allocated at exactly their size."""

    def __init__(self, jobs):
        self.arr = (_lib.AdmitJob * max(1, len(jobs)))()
        self.n = len(jobs)
        self.keep, self.outs, self.given = [], [], []
        for S, job in zip(self.arr, jobs):
            n = np.asarray(job["state"]).reshape(-1, 8).shape[0] if job.get("state") is not None else 1
            n_pts = np.asarray(job["host"]).reshape(-1).shape[0] if job.get("host") is not None else 0
            n_res = np.asarray(job["point"]).reshape(-1).shape[0] if job.get("point") is not None else 0
            drop = job.get("drop")
            ins, out, given = {}, {}, set()
            for k, dtype, size in inputs(n, n_pts, n_res):
                a = np.ascontiguousarray(job[k], dtype).reshape(-1) if job.get(k) is not None and k != drop else None
                if a is not None and len(a) != size:
                    raise ValueError(f"admit job: {k} has {len(a)} entries, not {size}")
                setattr(S, k, a.ctypes.data_as(_PTR[dtype]) if a is not None else None)
                ins[k] = a
            for o, dtype, size in outputs(n, n_pts, n_res):
                out[o] = np.full(size, _fill(dtype), dtype)
                src = o[:-4]
                absent = (src in OPTIONAL and ins.get(src) is None) or (o == "distance_ll_out" and not job.get("distances", True))
                if o != drop and not absent:
                    given.add(o)
                setattr(S, o, out[o].ctypes.data_as(_PTR[dtype]) if o in given else None)
            for k in WORDS:
                out[k] = np.full(1, FILL_INT, i32)
                setattr(S, k, out[k].ctypes.data_as(_lib.c_int_p) if k != drop else None)
                given.add(k)
            S.n_frames, S.n_pts, S.n_res = int(job.get("n_frames", n)), int(job.get("n_pts", n_pts)), int(job.get("n_res", n_res))
            S.new_keyframe_id, S.new_exposure, S.new_frame_energy_th = int(job["new_keyframe_id"]), float(job["new_exposure"]), float(job["new_frame_energy_th"])
            S.aff_g2l[0], S.aff_g2l[1] = float(job["aff_g2l"][0]), float(job["aff_g2l"][1])
            self.keep.append(ins)
            self.outs.append(out)
            self.given.append(given)

    @staticmethod
    def _refs(lp, sp, ap):
        return tuple(C.byref(p) if p is not None else None for p in (lp, sp, ap))

    def run(self, ctx, lp=None, sp=None, ap=None):
        """one dsm_window_admit_batch call; a parameter set None: the C side's defaults (a NULL pointer)"""
        check(ctx.L.dsm_window_admit_batch(ctx.h, self.n, self.arr, *self._refs(lp, sp, ap)))

    def run_host(self, lp=None, sp=None, ap=None):
        """dsm_window_admit_host on every job"""
        check(_lib.load().dsm_window_admit_host(self.n, self.arr, *self._refs(lp, sp, ap)))

    def all_outputs(self):
        """per job every output array itself, under the C field's name (also those left NULL, which keep their fill)"""
        return self.outs

    def results(self):
        """per job a dict: every array that was given under its name without _out, n_res and n_flagged as ints"""
        res = []
        for out, given in zip(self.outs, self.given):
            r = {}
            for o, v in out.items():
                if o not in given:
                    continue
                if o in WORDS:
                    r["n_res" if o == "n_res_out" else o] = int(v[0])
                else:
                    r[o[:-4]] = v.copy()
            res.append(r)
        return res


def window_admit_batch(ctx, jobs, lp=None, sp=None, ap=None):
    """dsm_window_admit_batch: per job the dict of AdmitBatch.results"""
    b = AdmitBatch(jobs)
    b.run(ctx, lp, sp, ap)
    return b.results()


def window_admit_host(jobs, lp=None, sp=None, ap=None):
    """dsm_window_admit_host (no device): the same dicts"""
    b = AdmitBatch(jobs)
    b.run_host(lp, sp, ap)
    return b.results()
