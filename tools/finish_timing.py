#!/usr/bin/env python3
"""The loop of the window optimisation (six iterations, all accepted: force_accept = 1, min_iterations = max_iterations = 6, 7 passes)
WITH what optimize does behind it, on the device: ms per window for 1 / 11 / 64 windows of the workload of
tools/linearize_timing.py (KITTI-shaped, 1232 x 368, 8 keyframes, 2 000 points, 14 000 residuals), whole synchronous calls timed.  In
the same run, on the same inputs:
  (a) one_call  ONE dsm_window_finish_batch: the passes and the four launches of the finish back to back, one host wait
  (b) before    the route before: dsm_window_optimize_batch, then per window Z1-Z3 as the host form's loops on one core
                (dsm_diag_finish_prepare_host), ONE dsm_linearize_residuals_batch with the fix flag for all windows, then per window
                Z5-Z8 as the host form's loops (dsm_diag_finish_book_host)
After a warm-up the routes run in alternation; each figure is the median over the repetitions of a host clock.  The results of the two
routes are compared before anything is timed: the loop's outputs bit for bit, and every decision, integer and index map of the finish
equal (the two routes share the loop's kernels; (b)'s Z1-Z3 use the C library's sincos and exp, the device its own).  loop_alone is
dsm_window_optimize_batch by itself, so that the finish's own share of either route shows.  Prints one JSON line.

  python tools/finish_timing.py [--reps 9] [--batches 1,11,64] [--iterations 6] [--force-accept 0]   (0: the energy test decides)
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import hessian_timing as HT  # noqa: E402
import linearize_timing as LT  # noqa: E402
import solve_timing as ST  # noqa: E402
import step_timing as PT  # noqa: E402
from direct_stereo_slam_amd import _lib  # noqa: E402
from direct_stereo_slam_amd import finish as FN  # noqa: E402
from direct_stereo_slam_amd import linearize as L  # noqa: E402
from direct_stereo_slam_amd import optimize as OP  # noqa: E402
from direct_stereo_slam_amd import step as SP  # noqa: E402
from direct_stereo_slam_amd.tracker import Context  # noqa: E402

f32 = np.float32
DECISIONS = ("new_state", "keep", "n_good_residuals_out", "last_res_out", "last_state_out", "n_res_kept", "point_dropped", "res_index_out",
             "point_index_out", "n_res_out", "n_pts_out", "lost")


def finish_inputs(job):
    """slot 0 of every point names its first residual, slot 1 none; counters zero"""
    point = np.asarray(job["point"], np.int64)
    m = len(job["host"])
    last = np.full((m, 2), -1, np.int32)
    first = np.full(m, -1, np.int64)
    first[point[::-1]] = np.arange(len(point))[::-1]
    last[:, 0] = first
    return dict(job, n_good_residuals_in=np.zeros(m, np.int32), max_rel_baseline_in=np.zeros(m, f32), last_res=last,
                last_state_in=np.zeros((m, 2), np.uint8))


class Before:
    """route (b) on a FinishBatch of its own: its arrays receive the results"""

    def __init__(self, jobs):
        self.batch = FN.FinishBatch(jobs, (), finish_outputs=())
        n = self.batch.n
        self.lin = (_lib.LinearizeJob * n)()
        self.scratch = [np.zeros(len(job["frame_ids"]) + len(job["host"]) + 1, f32) for job in jobs]
        self.lib = _lib.load()

    def run(self, ctx, params, sp, op):
        b, lib = self.batch, self.lib
        _lib.check(ctx.L.dsm_window_optimize_batch(ctx.h, b.n, b.opt.arr, C.byref(params), C.byref(sp), C.byref(op)))
        for j in range(b.n):
            _lib.check(lib.dsm_diag_finish_prepare_host(C.byref(b.arr[j]), C.byref(params), C.byref(sp), self.scratch[j].ctypes.data_as(_lib.c_float_p),
                                                          C.byref(self.lin[j])))
        _lib.check(ctx.L.dsm_linearize_residuals_batch(ctx.h, b.n, self.lin, C.byref(params)))
        for j in range(b.n):
            _lib.check(lib.dsm_diag_finish_book_host(C.byref(b.arr[j])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batches", default="1,11,64")
    ap.add_argument("--iterations", type=int, default=6)
    ap.add_argument("--force-accept", type=int, default=1, help="0: the energy test decides (rejected steps, a second host wait in both routes)")
    args = ap.parse_args()
    batches = [int(b) for b in args.batches.split(",")]
    its = args.iterations
    ctx = Context(0)
    n = max(batches)
    tex = LT.base_texture()
    jobs, wins = [], []
    for j in range(n):
        job, fr = LT.window(900 + j, tex)
        win = L.KeyframeWindow(ctx, LT.W, LT.H, LT.N_FRAMES)
        for fid, img in zip(job["frame_ids"], fr):
            win.put_host(int(fid), img)
        extra = ST.solve_extras(7000 + j)
        extra.pop("delta_x")
        hes = HT.extras(5000 + j)
        hes.pop("delta", None)
        step = PT.step_job(job, 8000 + j)
        full = dict(step, window=win, fix_linearization=0, frame_step=None, calib_step=None, idepth_step=None, max_iterations=its, **hes, **extra)
        jobs.append(finish_inputs(full)), wins.append(win)
    params, sp = L.default_params(), SP.default_step_params()
    force = args.force_accept != 0
    op = OP.default_optimize_params(force_accept=int(force), min_iterations=its)

    # the two routes against each other before anything is timed
    a, b = FN.FinishBatch(jobs, (), finish_outputs=()), Before(jobs)
    a.run(ctx, params, sp, op)
    b.run(ctx, params, sp, op)
    decisions_equal, loop_equal, removed, dropped = True, True, 0, 0
    passes_run = []
    for (oa, ga), (ob, gb) in zip(a.results(), b.batch.results()):
        if force and (oa["n_passes"] != 1 + its or oa["pattern"] != "A" * its):
            raise SystemExit("the one call did not run 1 + iterations passes")
        passes_run.append(oa["n_passes"])
        loop_equal = loop_equal and all(np.asarray(oa[k]).tobytes() == np.asarray(ob[k]).tobytes() for k in ("state", "calib", "idepth", "new_state", "new_energy", "x"))
        decisions_equal = decisions_equal and all(np.array_equal(np.asarray(ga[k]), np.asarray(gb[k])) for k in DECISIONS)
        removed += int((ga["keep"] == 0).sum())
        dropped += int(ga["point_dropped"].sum())
    if not loop_equal:
        raise SystemExit("the one call and the route before disagree on the loop's outputs")
    if not decisions_equal:  # (b)'s tables are a C library's: a residual at a threshold may decide otherwise; reported, not hidden
        print("the finish's decisions differ between the routes", file=sys.stderr)
    del a, b

    one_call = {B: FN.FinishBatch(jobs[:B], (), finish_outputs=()) for B in batches}
    before = {B: Before(jobs[:B]) for B in batches}
    loop_only = {B: OP.OptimizeBatch(jobs[:B], ()) for B in batches}
    for _ in range(args.warmup):
        for B in batches:
            one_call[B].run(ctx, params, sp, op), before[B].run(ctx, params, sp, op), loop_only[B].run(ctx, params, sp, op)
    t = {(B, k): [] for B in batches for k in ("one_call", "before", "loop_only")}
    for _ in range(args.reps):
        for B in batches:
            t[(B, "one_call")].append(LT.timed(lambda: one_call[B].run(ctx, params, sp, op)))
            t[(B, "before")].append(LT.timed(lambda: before[B].run(ctx, params, sp, op)))
            t[(B, "loop_only")].append(LT.timed(lambda: loop_only[B].run(ctx, params, sp, op)))
    out = {"tool": "finish_timing", "reps": args.reps, "iterations": its, "force_accept": int(force),
           "passes": 1 + its if force else [min(passes_run), max(passes_run)], "geometry": [LT.W, LT.H], "frames": LT.N_FRAMES,
           "points_per_window": LT.N_PTS, "residuals_per_window": LT.N_PTS * (LT.N_FRAMES - 1), "decisions_equal": bool(decisions_equal),
           "loop_outputs_equal_bit_for_bit": bool(loop_equal), "residuals_removed": removed, "points_dropped": dropped, "per_batch": {}}
    for B in batches:
        x, y, z = (float(np.median(t[(B, k)])) for k in ("one_call", "before", "loop_only"))
        out["per_batch"][f"B={B}"] = {"one_call_ms": round(x, 3), "before_ms": round(y, 3), "loop_alone_ms": round(z, 3),
                                      "one_call_ms_per_window": round(x / B, 4), "before_ms_per_window": round(y / B, 4),
                                      "finish_in_the_call_ms_per_window": round((x - z) / B, 4), "finish_before_ms_per_window": round((y - z) / B, 4),
                                      "one_call_over_before": round(x / y, 3)}
    for w in wins:
        w.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
