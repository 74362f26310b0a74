"""The loop of FrontEnd::traceNewCoarse (FrontEnd.cpp:276-327) on the device: ImmaturePoint::traceOn for the immature points of many
sequences against each sequence's new frame in one call -- the ctypes mirror of dsm_trace_points_batch, and of the host form
dsm_trace_points_host.  Semantics: DESIGN.md section 14 (T1-T16).

A job is a dict: target (a KeyframeWindow of direct_stereo_slam_amd.immature with target_frame_id, or a TrackerAndScaler with
target_slot; not needed by the host form), krki (n_hosts x 9), kt (n_hosts x 3), aff (n_hosts x 2), host, u, v, energy_th,
grad_h (n_pts x 4), color (n_pts x 8), weights (n_pts x 8), and the state traceOn updates: status, idepth_min, idepth_max, quality,
trace_uv (n_pts x 2), trace_interval.  A result is a dict with that state after the call, steps and counts (per status)."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import c_float_p, c_int_p, check

GOOD, OOB, OUTLIER, SKIPPED, BADCONDITION, UNINITIALIZED = range(6)  # DSM_IPS_*
STATE = ("status", "idepth_min", "idepth_max", "quality", "trace_uv", "trace_interval")
PARAMS = ("max_pix_search", "slack_interval", "stepsize", "min_improvement", "min_test_radius", "gn_iterations", "gn_threshold",
          "extra_slack_on_th", "huber_th")


def params(**kw):
    """dsm_trace_params: the upstream defaults (dsm_trace_params_default), with the given fields replaced"""
    p = _lib.TraceParams()
    check(_lib.load().dsm_trace_params_default(C.byref(p)))
    for k, v in kw.items():
        if k not in PARAMS:
            raise TypeError(f"dsm_trace_params has no field {k}")
        setattr(p, k, v)
    return p


def _f(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1)


def _i(a):
    return np.ascontiguousarray(a, np.int32).reshape(-1)


class TraceBatch:
    """The ctypes job table of dsm_trace_points_batch and its in/out arrays, built once: `run()` is the C call alone
    (tools/trace_timing.py times it), `reset()` restores the state the jobs came with, `results()` unpacks."""

    def __init__(self, jobs):
        self.arr = (_lib.TraceJob * max(1, len(jobs)))()
        self.n = len(jobs)
        self.keep, self.state = [], []
        for J, job in zip(self.arr, jobs):
            hosts = [_f(job["krki"]), _f(job["kt"]), _f(job["aff"])]
            nh = len(hosts[0]) // 9
            if [len(a) for a in hosts] != [9 * nh, 3 * nh, 2 * nh]:
                raise ValueError("trace job: krki / kt / aff are not n_hosts x 9 / 3 / 2")
            host = _i(job["host"])
            n = len(host)
            per = [_f(job[k]) for k in ("u", "v", "energy_th", "grad_h", "color", "weights")]
            if [len(a) for a in per] != [n, n, n, 4 * n, 8 * n, 8 * n]:
                raise ValueError("trace job: per-point arrays of unequal length")
            first = dict(status=np.ascontiguousarray(job["status"], np.uint8).reshape(-1), idepth_min=_f(job["idepth_min"]),
                         idepth_max=_f(job["idepth_max"]), quality=_f(job["quality"]), trace_uv=_f(job["trace_uv"]),
                         trace_interval=_f(job["trace_interval"]))
            if [len(first[k]) for k in STATE] != [n, n, n, n, 2 * n, n]:
                raise ValueError("trace job: state arrays of unequal length")
            st = {k: np.concatenate([v, np.zeros(1, v.dtype)]) for k, v in first.items()}  # never an empty buffer
            st["steps"], st["counts"] = np.full(n + 1, -1, np.int32), np.full(6, -1, np.int32)
            target = job.get("target")
            self.keep.append((hosts, host, per, target, first))
            self.state.append((st, n))
            if target is None:
                J.target_tracker = J.target_window = None
            elif hasattr(target, "win"):
                J.target_tracker, J.target_window, J.target_frame_id = None, target.win, int(job["target_frame_id"])
            else:
                J.target_tracker, J.target_window, J.target_slot = target.h, None, int(job["target_slot"])
            J.n_hosts = nh
            J.krki, J.kt, J.aff = (a.ctypes.data_as(c_float_p) for a in hosts)
            J.n_pts, J.host = n, host.ctypes.data_as(c_int_p)
            J.u, J.v, J.energy_th, J.grad_h, J.color, J.weights = (a.ctypes.data_as(c_float_p) for a in per)
            J.status = st["status"].ctypes.data_as(C.POINTER(C.c_ubyte))
            J.idepth_min, J.idepth_max, J.quality, J.trace_uv, J.trace_interval = (st[k].ctypes.data_as(c_float_p) for k in STATE[1:])
            J.steps_out, J.counts_out = st["steps"].ctypes.data_as(c_int_p), st["counts"].ctypes.data_as(c_int_p)

    def reset(self):
        for (st, n), keep in zip(self.state, self.keep):
            for k in STATE:
                st[k][: len(keep[4][k])] = keep[4][k]

    def run(self, ctx, p=None):
        """one dsm_trace_points_batch call"""
        p = p if p is not None else params()
        check(ctx.L.dsm_trace_points_batch(ctx.h, self.n, self.arr, C.byref(p)))

    def run_host(self, w, h, j, target, p=None):
        """dsm_trace_points_host on job j; target: the new frame's level-0 plane"""
        p = p if p is not None else params()
        plane = np.ascontiguousarray(target, np.float32)
        if plane.size != int(w) * int(h):
            raise ValueError("trace job: the target plane is not w * h")
        check(_lib.load().dsm_trace_points_host(int(w), int(h), plane.ctypes.data_as(c_float_p), C.byref(self.arr[j]), C.byref(p)))

    def results(self):
        """per job a dict: status, idepth_min, idepth_max, quality, trace_uv (n_pts x 2), trace_interval, steps, counts (6)"""
        out = []
        for st, n in self.state:
            r = {k: st[k][:n].copy() for k in ("status", "idepth_min", "idepth_max", "quality", "trace_interval", "steps")}
            r["trace_uv"], r["counts"] = st["trace_uv"][: 2 * n].reshape(n, 2).copy(), st["counts"].copy()
            out.append(r)
        return out


def trace_points_batch(ctx, jobs, **kw):
    """dsm_trace_points_batch: a list of job dicts in, a list of result dicts out; keyword arguments are fields of dsm_trace_params"""
    b = TraceBatch(jobs)
    b.run(ctx, params(**kw))
    return b.results()


def trace_points_host(w, h, target, job, **kw):
    """dsm_trace_points_host (no device): the same dict for one job against the plane `target`"""
    b = TraceBatch([job])
    b.run_host(w, h, 0, target, params(**kw))
    return b.results()[0]
