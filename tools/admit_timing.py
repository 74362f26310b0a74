#!/usr/bin/env python3
"""Admitting the new keyframe for 1 / 11 / 64 windows of 7 old keyframes, 2 000 points and 12 000 residuals, with H_M, b_M, H_L, b_L and
the priors given: ms per window of
  (a) device  one dsm_window_admit_batch, whole synchronous call (staging, one launch, read-back)
  (b) host    one dsm_window_admit_host over the same windows: a loop on one core
in the same run, on the scenes of tests/_admit_ref.py (make_scene).  After a warm-up the two run in alternation; each figure is the
median over the repetitions of a host clock.  Before anything is timed every output of the device form is compared with the host
form's, bit for bit.  There is no pass mark.  Prints one JSON line.

  python tools/admit_timing.py [--reps 15] [--batches 1,11,64]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import _admit_ref as AR  # noqa: E402
from direct_stereo_slam_amd import admit as AD  # noqa: E402
from direct_stereo_slam_amd.tracker import Context  # noqa: E402

N_FRAMES, N_PTS, PER_POINT = 7, 2000, 6


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", default="1,11,64")
    args = ap.parse_args()
    batches = [int(b) for b in args.batches.split(",")]
    ctx = Context(0)
    jobs = [AR.call_job(AR.make_scene(seed=500 + j, n_frames=N_FRAMES, n_pts=N_PTS, counts=(PER_POINT,), ref=j % N_FRAMES)) for j in range(max(batches))]
    n_res = len(jobs[0]["point"])
    for j, (d, h) in enumerate(zip(AD.window_admit_batch(ctx, jobs), AD.window_admit_host(jobs))):
        for k in d:
            if np.asarray(d[k]).tobytes() != np.asarray(h[k]).tobytes():
                raise SystemExit(f"window {j}: the device form and the host form disagree on {k}")
    calls = {B: (AD.AdmitBatch(jobs[:B]), AD.AdmitBatch(jobs[:B])) for B in batches}
    for _ in range(args.warmup):
        for B in batches:
            calls[B][0].run(ctx), calls[B][1].run_host()
    t = {(B, k): [] for B in batches for k in ("device", "host")}
    for _ in range(args.reps):
        for B in batches:
            t[(B, "device")].append(timed(lambda: calls[B][0].run(ctx)))
            t[(B, "host")].append(timed(lambda: calls[B][1].run_host()))
    out = {"tool": "admit_timing", "reps": args.reps, "frames": N_FRAMES, "points": N_PTS, "residuals": n_res, "device_equals_host_bit_for_bit": True,
           "per_batch": {}}
    for B in batches:
        d, h = float(np.median(t[(B, "device")])), float(np.median(t[(B, "host")]))
        out["per_batch"][f"B={B}"] = {"device_ms_per_window": round(d / B, 4), "host_ms_per_window": round(h / B, 4), "device_over_host": round(d / h, 3)}
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
