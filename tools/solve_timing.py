#!/usr/bin/env python3
"""One trial step of the window optimisation on the device (dsm_window_solve_batch): ms per call and per window for 1 / 11 / 64
windows of the workload of tools/linearize_timing.py (KITTI-shaped, 1232 x 368, 8 keyframes, 2 000 points, 14 000 residuals), the
whole synchronous call timed.  In the same run, on the same inputs:
  (a) new_call     dsm_window_solve_batch with every optional output NULL: linearisation, accumulation, stitch, solve, steps
  (b) old_route    the route it replaces: dsm_window_hessian_batch (optional outputs NULL), plus F1-R3 on one host core -- timed as
                   dsm_window_solve_host minus dsm_window_hessian_host on the same window in the same repetition
  (c) host_form    a loop of dsm_window_solve_host, one core
After a warm-up the variants run in alternation; each figure is the median over the repetitions of a host clock.  Every device result
is compared with the host form's, bit for bit, before anything is timed.  Prints one JSON line.

  python tools/solve_timing.py [--reps 9] [--batches 1,11,64]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import hessian_timing as HT  # noqa: E402
import linearize_timing as LT  # noqa: E402
from direct_stereo_slam_amd import hessian as HS  # noqa: E402
from direct_stereo_slam_amd import linearize as L  # noqa: E402
from direct_stereo_slam_amd import solve as SV  # noqa: E402
from direct_stereo_slam_amd.tracker import Context  # noqa: E402


def solve_extras(seed):
    """H_L and the prior system of a window: positive semi-definite, of the size of the accumulated system's entries"""
    rng = np.random.default_rng(seed)
    N = 4 + 8 * LT.N_FRAMES
    sym = lambda M: np.tril(M) + np.tril(M, -1).T  # noqa: E731
    G, Gm = rng.normal(0, 30.0, (N, N)), rng.normal(0, 20.0, (N, 6))
    return {"H_L": sym(G @ G.T), "b_L": rng.normal(0, 300.0, N), "H_M": sym(Gm @ Gm.T + np.diag(rng.uniform(0, 5e3, N))),
            "b_M": rng.normal(0, 200.0, N), "delta_x": rng.normal(0, 0.05, N), "lambda": 1e-4}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batches", default="1,11,64")
    args = ap.parse_args()
    batches = [int(b) for b in args.batches.split(",")]
    ctx = Context(0)
    n = max(batches)
    tex = LT.base_texture()
    jobs, frames, wins = [], [], []
    for j in range(n):
        job, fr = LT.window(900 + j, tex)
        win = L.KeyframeWindow(ctx, LT.W, LT.H, LT.N_FRAMES)
        for fid, img in zip(job["frame_ids"], fr):
            win.put_host(int(fid), img)
        jobs.append(dict(job, window=win, **HT.extras(5000 + j), **solve_extras(7000 + j))), frames.append(fr), wins.append(win)
    params = L.default_params()
    new_call = {B: SV.SolveBatch(jobs[:B], ()) for B in batches}
    old_call = {B: HS.HessianBatch(jobs[:B], ()) for B in batches}
    host_solve, host_hes = SV.SolveBatch(jobs, ()), HS.HessianBatch(jobs, ())
    # the device form against the host form before anything is timed, every output asked for
    check_dev, check_host = SV.SolveBatch(jobs), SV.SolveBatch(jobs)
    check_dev.run(ctx, params)
    for j in range(n):
        check_host.run_host(LT.W, LT.H, j, frames[j], params)
    for j, (d, h) in enumerate(zip(check_dev.results(), check_host.results())):
        if d["flags"] or any(np.asarray(d[k]).tobytes() != np.asarray(h[k]).tobytes() for k in d):
            raise SystemExit(f"window {j}: the device form and the host form disagree")
    del check_dev, check_host
    for _ in range(args.warmup):
        for B in batches:
            new_call[B].run(ctx, params), old_call[B].run(ctx, params)
    keys = ("new_call", "old_device", "host_form", "host_hes", "host_solve")
    t = {(B, k): [] for B in batches for k in keys}
    for _ in range(args.reps):
        for B in batches:
            t[(B, "new_call")].append(LT.timed(lambda: new_call[B].run(ctx, params)))
            t[(B, "old_device")].append(LT.timed(lambda: old_call[B].run(ctx, params)))
            hf = LT.timed(lambda: [host_solve.run_host(LT.W, LT.H, j, frames[j], params) for j in range(B)])
            hh = LT.timed(lambda: [host_hes.run_host(LT.W, LT.H, j, frames[j], params) for j in range(B)])
            t[(B, "host_form")].append(hf), t[(B, "host_hes")].append(hh), t[(B, "host_solve")].append(hf - hh)
    out = {"tool": "solve_timing", "reps": args.reps, "geometry": [LT.W, LT.H], "frames": LT.N_FRAMES, "points_per_window": LT.N_PTS,
           "residuals_per_window": LT.N_PTS * (LT.N_FRAMES - 1), "per_batch": {}}
    for B in batches:
        m = {k: float(np.median(t[(B, k)])) for k in keys}
        route = m["old_device"] + m["host_solve"]
        out["per_batch"][f"B={B}"] = {
            "new_call_ms_per_window": round(m["new_call"] / B, 4), "old_route_ms_per_window": round(route / B, 4),
            "old_route_device_ms_per_window": round(m["old_device"] / B, 4), "old_route_host_solve_ms_per_window": round(m["host_solve"] / B, 4),
            "host_form_ms_per_window": round(m["host_form"] / B, 4), "new_call_over_old_route": round(m["new_call"] / route, 3)}
    for w in wins:
        w.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
