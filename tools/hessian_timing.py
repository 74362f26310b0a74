#!/usr/bin/env python3
"""Hessian and Schur accumulation of the window optimisation (dsm_window_hessian_batch): ms per call and per window for 1 / 11 / 64
windows of the workload of tools/linearize_timing.py (KITTI-shaped, 1232 x 368, 8 keyframes, 2 000 points, 14 000 residuals), the
whole synchronous call timed.  In the same run, on the same inputs:
  (a) new_call      dsm_window_hessian_batch with every optional output NULL: linearisation, accumulation, stitch
  (b) rows_route    the route before this call: dsm_linearize_residuals_batch with the rows, centres and projections read back, plus
                    the accumulation on one host core -- timed as dsm_window_hessian_host minus dsm_linearize_residuals_host on the
                    same window in the same repetition (the host form is the linearisation followed by the accumulation and the stitch)
  (c) host_form     a loop of dsm_window_hessian_host, one core
  stitch            T1 alone, timed as dsm_window_hessian_host on the same window without residuals: the stitch then runs on zero
                    accumulators, and its operation count does not depend on the values
After a warm-up the variants run in alternation; each figure is the median over the repetitions of a host clock.  Every device result
is compared with the host form's, bit for bit, before anything is timed.  Prints one JSON line.

  python tools/hessian_timing.py [--reps 9] [--batches 1,11,64]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import linearize_timing as LT  # noqa: E402
from direct_stereo_slam_amd import hessian as HS  # noqa: E402
from direct_stereo_slam_amd import linearize as L  # noqa: E402
from direct_stereo_slam_amd.tracker import Context  # noqa: E402

f32 = np.float32


def extras(seed):
    rng = np.random.default_rng(seed)
    nf, n = LT.N_FRAMES, LT.N_PTS
    return dict(ad_host=-np.eye(8) + rng.normal(0, 0.2, (nf, nf, 8, 8)), ad_target=np.eye(8) + rng.normal(0, 0.2, (nf, nf, 8, 8)),
                prior=np.where(rng.uniform(size=n) < 0.1, 2500.0, 0.0).astype(f32), delta=rng.normal(0, 0.01, n).astype(f32),
                hdd_lin=rng.uniform(0, 5e3, n).astype(f32), bd_lin=rng.normal(0, 50, n).astype(f32),
                hcd_lin=rng.normal(0, 50, (n, 4)).astype(f32), shift_prior_to_zero=1)


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
        jobs.append(dict(job, window=win, **extras(5000 + j))), frames.append(fr), wins.append(win)
    params = L.default_params()
    new_call = {B: HS.HessianBatch(jobs[:B], ()) for B in batches}
    rows_call = {B: L.LinearizeBatch(jobs[:B], LT.ROWS) for B in batches}
    host_form, host_lin = HS.HessianBatch(jobs, ()), L.LinearizeBatch(jobs, LT.ROWS)
    empty = HS.HessianBatch([dict(job, **{k: np.asarray(job[k])[:0] for k in ("point", "target", "state_in", "energy_in", "is_new")}) for job in jobs], ())
    # the device form against the host form before anything is timed, every output asked for
    check_dev, check_host = HS.HessianBatch(jobs), HS.HessianBatch(jobs)
    check_dev.run(ctx, params)
    for j in range(n):
        check_host.run_host(LT.W, LT.H, j, frames[j], params)
    active = []
    for j, (d, h) in enumerate(zip(check_dev.results(), check_host.results())):
        if any(np.asarray(d[k]).tobytes() != np.asarray(h[k]).tobytes() for k in d):
            raise SystemExit(f"window {j}: the device form and the host form disagree")
        active.append(d["active"].mean())
    del check_dev, check_host
    for _ in range(args.warmup):
        for B in batches:
            new_call[B].run(ctx, params), rows_call[B].run(ctx, params)
    keys = ("new_call", "rows_device", "host_form", "host_lin", "host_acc", "stitch")
    t = {(B, k): [] for B in batches for k in keys}
    for _ in range(args.reps):
        for B in batches:
            t[(B, "new_call")].append(LT.timed(lambda: new_call[B].run(ctx, params)))
            t[(B, "rows_device")].append(LT.timed(lambda: rows_call[B].run(ctx, params)))
            hf = LT.timed(lambda: [host_form.run_host(LT.W, LT.H, j, frames[j], params) for j in range(B)])
            hl = LT.timed(lambda: [host_lin.run_host(LT.W, LT.H, j, frames[j], params) for j in range(B)])
            t[(B, "host_form")].append(hf), t[(B, "host_lin")].append(hl), t[(B, "host_acc")].append(hf - hl)
            t[(B, "stitch")].append(LT.timed(lambda: [empty.run_host(LT.W, LT.H, j, frames[j], params) for j in range(B)]))
    out = {"tool": "hessian_timing", "reps": args.reps, "geometry": [LT.W, LT.H], "frames": LT.N_FRAMES, "points_per_window": LT.N_PTS,
           "residuals_per_window": LT.N_PTS * (LT.N_FRAMES - 1), "active_share": round(float(np.mean(active)), 4), "per_batch": {}}
    for B in batches:
        m = {k: float(np.median(t[(B, k)])) for k in keys}
        route = m["rows_device"] + m["host_acc"]
        out["per_batch"][f"B={B}"] = {
            "new_call_ms_per_window": round(m["new_call"] / B, 4), "rows_route_ms_per_window": round(route / B, 4),
            "rows_route_device_ms_per_window": round(m["rows_device"] / B, 4), "rows_route_host_accumulation_ms_per_window": round(m["host_acc"] / B, 4),
            "host_form_ms_per_window": round(m["host_form"] / B, 4), "stitch_ms_per_window": round(m["stitch"] / B, 4),
            "rows_route_over_new_call": round(route / m["new_call"], 2), "host_form_over_new_call": round(m["host_form"] / m["new_call"], 2),
            "stitch_share_of_new_call": round(m["stitch"] / m["new_call"], 3)}
    for w in wins:
        w.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
