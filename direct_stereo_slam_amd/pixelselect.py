"""FrontEnd::makeNewTraces (FrontEnd.cpp:936-962) on the device: PixelSelector::makeMaps and the ImmaturePoint constructor for the new
keyframes of many sequences in one call -- the ctypes mirror of dsm_select_pixels_batch, and of the host form dsm_select_pixels_host.
Semantics: DESIGN.md section 15 (P1-P14).

A job is a dict: tracker (a TrackerAndScaler with >= 3 levels) and slot (not needed by the host form), density, potential
(currentPotential of the sequence, 3 at first use), max_pts, and optionally b_inv (256 floats) and want_map (default True).
A result is a dict: n_pts, num_total, counts (n2, n3, n4), passes, potential (to carry into the sequence's next call), map (h x w,
if wanted) and the arrays of the first min(n_pts, max_pts) points exactly as a trace job takes them: u, v, energy_th, grad_h (n x 4),
color (n x 8), weights (n x 8), status, idepth_min, idepth_max, quality, plus type."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import c_float_p, c_int_p, check

c_ubyte_p = C.POINTER(C.c_ubyte)
PARAMS = ("min_grad_hist_cut", "min_grad_hist_add", "grad_downweight_per_level", "select_direction_distribution", "th_factor", "recursions",
          "pattern_padding", "outlier_th", "outlier_th_sum_component", "overall_energy_th_weight")
POINT_FLOATS = (("u", 1), ("v", 1), ("energy_th", 1), ("grad_h", 4), ("color", 8), ("weights", 8), ("idepth_min", 1), ("idepth_max", 1),
                ("quality", 1), ("type", 1))


def params(**kw):
    """dsm_select_params: the upstream defaults (dsm_select_params_default), with the given fields replaced"""
    p = _lib.SelectParams()
    check(_lib.load().dsm_select_params_default(C.byref(p)))
    for k, v in kw.items():
        if k not in PARAMS:
            raise TypeError(f"dsm_select_params has no field {k}")
        setattr(p, k, v)
    return p


def random_pattern(w, h, seed=3141592):
    """w * h random bytes.  Upstream fills its pattern with srand(3141592), rand() & 0xFF, which depends on the libc; a caller that
    wants upstream's selection on its platform passes that pattern instead."""
    return np.random.default_rng(seed).integers(0, 256, w * h, dtype=np.uint8)


class PixelSelector:
    """dsm_pixel_selector: the device copy of the random pattern and all scratch for max_jobs jobs of one geometry"""

    def __init__(self, ctx, w, h, max_jobs, pattern=None):
        self.ctx, self.L, self.w, self.hgt, self.max_jobs = ctx, ctx.L, int(w), int(h), int(max_jobs)
        self.pattern = np.ascontiguousarray(random_pattern(w, h) if pattern is None else pattern, np.uint8).reshape(-1)
        if self.pattern.size != self.w * self.hgt:
            raise ValueError("PixelSelector: the random pattern is not w * h bytes")
        hnd = C.c_void_p()
        check(self.L.dsm_pixel_selector_create(ctx.h, self.w, self.hgt, self.max_jobs, self.pattern.ctypes.data_as(c_ubyte_p), C.byref(hnd)))
        self.h = hnd

    def close(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self.L.dsm_pixel_selector_destroy(self.h)
        self.h = None

    def __del__(self):
        self.close()


class SelectBatch:
    """The ctypes job table of dsm_select_pixels_batch and its output arrays, built once: `run()` is the C call alone
    (tools/select_timing.py times it), `reset()` restores the potentials the jobs came with, `results()` unpacks."""

    def __init__(self, jobs, w, h):
        self.arr = (_lib.SelectJob * max(1, len(jobs)))()
        self.n, self.w, self.h = len(jobs), int(w), int(h)
        self.keep, self.state = [], []
        for J, job in zip(self.arr, jobs):
            cap = int(job["max_pts"])
            st = {k: np.zeros(max(cap, 0) * n + 1, np.float32) for k, n in POINT_FLOATS}  # never an empty buffer
            st["status"] = np.zeros(max(cap, 0) + 1, np.uint8)
            st["ints"] = np.full(7, -1, np.int32)  # potential, n_pts, num_total, counts (3), passes
            st["ints"][0] = int(job.get("potential", 3))
            want_map = bool(job.get("want_map", True))
            st["map"] = np.full(self.w * self.h if want_map else 1, 255, np.uint8)
            b_inv = job.get("b_inv")
            if b_inv is not None:
                b_inv = np.ascontiguousarray(b_inv, np.float32).reshape(-1)
                if b_inv.size != 256:
                    raise ValueError("select job: b_inv is not 256 floats")
            trk = job.get("tracker")
            self.keep.append((b_inv, trk, int(st["ints"][0])))
            self.state.append((st, cap, want_map))
            J.tracker, J.slot = (trk.h if trk is not None else None), int(job.get("slot", 0))
            J.b_inv = b_inv.ctypes.data_as(c_float_p) if b_inv is not None else None
            J.density, J.max_pts = float(job["density"]), cap
            ints = st["ints"].ctypes.data
            J.potential_io, J.n_pts_out, J.num_total_out = (C.cast(ints + 4 * k, c_int_p) for k in range(3))
            J.counts_out, J.passes_out = C.cast(ints + 12, c_int_p), C.cast(ints + 24, c_int_p)
            for k, _ in POINT_FLOATS:
                setattr(J, k, st[k].ctypes.data_as(c_float_p))
            J.status = st["status"].ctypes.data_as(c_ubyte_p)
            J.map_out = st["map"].ctypes.data_as(c_ubyte_p) if want_map else None

    def reset(self):
        for (st, _, _), keep in zip(self.state, self.keep):
            st["ints"][0] = keep[2]

    def run(self, sel, p=None):
        """one dsm_select_pixels_batch call"""
        p = p if p is not None else params()
        check(sel.L.dsm_select_pixels_batch(sel.h, self.n, self.arr, C.byref(p)))

    def run_host(self, j, planes, pattern, p=None):
        """dsm_select_pixels_host on job j; planes: the intensity planes of levels 0, 1, 2"""
        p = p if p is not None else params()
        planes = [np.ascontiguousarray(a, np.float32) for a in planes]
        if [a.size for a in planes] != [(self.w >> l) * (self.h >> l) for l in range(3)]:
            raise ValueError("select job: the planes are not those of levels 0, 1, 2")
        pattern = np.ascontiguousarray(pattern, np.uint8).reshape(-1)
        if pattern.size != self.w * self.h:
            raise ValueError("select job: the random pattern is not w * h bytes")
        check(_lib.load().dsm_select_pixels_host(self.w, self.h, *(a.ctypes.data_as(c_float_p) for a in planes),
                                                 pattern.ctypes.data_as(c_ubyte_p), C.byref(self.arr[j]), C.byref(p)))

    def results(self):
        out = []
        for st, cap, want_map in self.state:
            ints = st["ints"]
            n = max(0, min(int(ints[1]), cap))
            r = dict(potential=int(ints[0]), n_pts=int(ints[1]), num_total=int(ints[2]), counts=ints[3:6].copy(), passes=int(ints[6]))
            for k, m in POINT_FLOATS:
                r[k] = st[k][: n * m].reshape((n, m) if m > 1 else (n,)).copy()
            r["status"] = st["status"][:n].copy()
            if want_map:
                r["map"] = st["map"].reshape(self.h, self.w).copy()
            out.append(r)
        return out


def select_pixels_batch(sel, jobs, **kw):
    """dsm_select_pixels_batch: a list of job dicts in, a list of result dicts out; keyword arguments are fields of dsm_select_params"""
    b = SelectBatch(jobs, sel.w, sel.hgt)
    b.run(sel, params(**kw))
    return b.results()


def select_pixels_host(w, h, planes, pattern, job, **kw):
    """dsm_select_pixels_host (no device): the same dict for one job on the intensity planes of levels 0, 1, 2"""
    b = SelectBatch([job], w, h)
    b.run_host(0, planes, pattern, params(**kw))
    return b.results()[0]
