"""The reference's `dso::CoarseDistanceMap` (src/scale_optimization/TrackerAndScaler.h:139-170) and the distance-map part of
FrontEnd::activatePointsMT (FrontEnd.cpp:371-451) on the device, for the windows of many sequences in one call: the ctypes mirror of
dsm_distmap_* / dsm_distmaps_make / dsm_activate_points_batch, and of the host form dsm_activate_points_host.  Semantics: DESIGN.md
section 12 (D1-D6).

A job is a dict: map (a DistanceMap; not needed by the host form), krki (n_hosts x 9, row-major K[1] R Ki[0]), kt (n_hosts x 3),
seed_host / seed_u / seed_v / seed_idepth, cand_host / cand_u / cand_v / cand_idepth / cand_type, min_act_dist."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import c_float_p, c_int_p, check


class DistanceMap:
    """one dsm_distmap: the (h >> 1) x (w >> 1) map of a window, 1000 everywhere when fresh"""

    def __init__(self, ctx, w, h):
        self.ctx, self.L = ctx, ctx.L
        self.w, self.h, self.w1, self.h1 = int(w), int(h), int(w) >> 1, int(h) >> 1
        m = C.c_void_p()
        check(self.L.dsm_distmap_create(ctx.h, self.w, self.h, C.byref(m)))
        self.m = m

    def close(self):
        if getattr(self, "m", None):
            self.L.dsm_distmap_destroy(self.m)
            self.m = None

    def __del__(self):
        self.close()

    def get(self):
        """fwdWarpedIDDistFinal: float32 (h1, w1), values 0 .. 39 and 1000"""
        out = np.empty((self.h1, self.w1), np.float32)
        check(self.L.dsm_distmap_get(self.m, out.ctypes.data_as(c_float_p)))
        return out

    def add(self, u, v):
        """addIntoDistFinal(u, v)"""
        check(self.L.dsm_distmap_add(self.m, int(u), int(v)))


def _f(a, shape=-1):
    return np.ascontiguousarray(a, np.float32).reshape(shape)


def _i(a):
    return np.ascontiguousarray(a, np.int32).reshape(-1)


class ActivationBatch:
    """The ctypes job table of dsm_distmaps_make / dsm_activate_points_batch and its output arrays, built once: `run()` and
    `make()` are the C call alone (tools/activation_timing.py times them), `results()` unpacks."""

    def __init__(self, jobs):
        self.arr = (_lib.ActivationJob * max(1, len(jobs)))()
        self.n = len(jobs)
        self.keep, self.outs = [], []
        for J, job in zip(self.arr, jobs):
            krki, kt = _f(job["krki"], (-1, 9)), _f(job["kt"], (-1, 3))
            s = [_i(job["seed_host"]), _f(job["seed_u"]), _f(job["seed_v"]), _f(job["seed_idepth"])]
            c = [_i(job["cand_host"]), _f(job["cand_u"]), _f(job["cand_v"]), _f(job["cand_idepth"]), _f(job["cand_type"])]
            if len(krki) != len(kt) or any(len(a) != len(s[0]) for a in s) or any(len(a) != len(c[0]) for a in c):
                raise ValueError("activation job: arrays of unequal length")
            dec, nact = np.zeros(max(1, len(c[0])), np.uint8), np.zeros(1, np.int32)
            self.keep.append((krki, kt, s, c, job.get("map")))
            self.outs.append((dec, nact, len(c[0])))
            J.map = job["map"].m if job.get("map") is not None else None
            J.n_hosts, J.krki, J.kt = len(krki), krki.ctypes.data_as(c_float_p), kt.ctypes.data_as(c_float_p)
            J.n_seeds, J.seed_host = len(s[0]), s[0].ctypes.data_as(c_int_p)
            J.seed_u, J.seed_v, J.seed_idepth = (a.ctypes.data_as(c_float_p) for a in s[1:])
            J.n_cand, J.cand_host = len(c[0]), c[0].ctypes.data_as(c_int_p)
            J.cand_u, J.cand_v, J.cand_idepth, J.cand_type = (a.ctypes.data_as(c_float_p) for a in c[1:])
            J.min_act_dist = float(job["min_act_dist"])
            J.decision_out, J.n_activated_out = dec.ctypes.data_as(C.POINTER(C.c_ubyte)), nact.ctypes.data_as(c_int_p)

    def run(self, ctx):
        """one dsm_activate_points_batch call (D1-D6)"""
        check(ctx.L.dsm_activate_points_batch(ctx.h, self.n, self.arr))

    def make(self, ctx):
        """one dsm_distmaps_make call (D1-D4 only)"""
        check(ctx.L.dsm_distmaps_make(ctx.h, self.n, self.arr))

    def run_host(self, w, h, j, map_out=None):
        """dsm_activate_points_host on job j"""
        check(_lib.load().dsm_activate_points_host(int(w), int(h), C.byref(self.arr[j]), None if map_out is None else map_out.ctypes.data_as(c_float_p)))

    def results(self):
        return [dict(decisions=dec[:n].copy(), n_activated=int(nact[0])) for dec, nact, n in self.outs]


def activate_points_batch(ctx, jobs):
    """dsm_activate_points_batch: per job a dict with decisions (uint8: 0 keep, 1 activate, 2 out of bounds) and n_activated; each
    job's DistanceMap then holds the map after its activations"""
    b = ActivationBatch(jobs)
    b.run(ctx)
    return b.results()


def make_distance_maps(ctx, jobs):
    """dsm_distmaps_make: makeDistanceMap for every job's map (the cand_* entries are not read)"""
    ActivationBatch(jobs).make(ctx)


def activate_points_host(w, h, job):
    """dsm_activate_points_host (no device): (map float32 (h1, w1), decisions, n_activated)"""
    b = ActivationBatch([job])
    m = np.empty((int(h) >> 1, int(w) >> 1), np.float32)
    b.run_host(w, h, 0, m)
    r = b.results()[0]
    return m, r["decisions"], r["n_activated"]
