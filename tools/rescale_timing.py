#!/usr/bin/env python3
"""Adopting the stereo scale into the window for 1 / 11 / 64 windows of 8 keyframes and 2 000 points, every scale accepted: ms per window of
  (a) device  one dsm_window_rescale_batch, whole synchronous call (staging, one launch, read-back)
  (b) host    one dsm_window_rescale_host over the same windows: a loop on one core
in the same run, on the scenes of tests/_rescale_ref.py (make_scene).  After a warm-up the two run in alternation; each figure is the
median over the repetitions of a host clock.  Before anything is timed every output of the device form is compared with the host
form's, bit for bit.  There is no pass mark.  Prints one JSON line.

  python tools/rescale_timing.py [--reps 15] [--batches 1,11,64]
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

import _rescale_ref as RR  # noqa: E402
from direct_stereo_slam_amd import rescale as RS  # noqa: E402
from direct_stereo_slam_amd.tracker import Context  # noqa: E402

N_FRAMES, N_PTS = 8, 2000


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
    jobs = [RR.call_job(RR.make_scene(seed=500 + j, n_frames=N_FRAMES, n_pts=N_PTS, new_scale=1.0 + 0.01 * (j + 1), ref=j % (N_FRAMES - 1)))
            for j in range(max(batches))]
    for j, (d, h) in enumerate(zip(RS.window_rescale_batch(ctx, jobs), RS.window_rescale_host(jobs))):
        if d["decision"] != RS.ACCEPTED:
            raise SystemExit(f"window {j}: not accepted")
        for k in d:
            if np.asarray(d[k]).tobytes() != np.asarray(h[k]).tobytes():
                raise SystemExit(f"window {j}: the device form and the host form disagree on {k}")
    calls = {B: (RS.RescaleBatch(jobs[:B]), RS.RescaleBatch(jobs[:B])) for B in batches}
    for _ in range(args.warmup):
        for B in batches:
            calls[B][0].run(ctx), calls[B][1].run_host()
    t = {(B, k): [] for B in batches for k in ("device", "host")}
    for _ in range(args.reps):
        for B in batches:
            t[(B, "device")].append(timed(lambda: calls[B][0].run(ctx)))
            t[(B, "host")].append(timed(lambda: calls[B][1].run_host()))
    out = {"tool": "rescale_timing", "reps": args.reps, "frames": N_FRAMES, "points": N_PTS, "device_equals_host_bit_for_bit": True, "per_batch": {}}
    for B in batches:
        d, h = float(np.median(t[(B, "device")])), float(np.median(t[(B, "host")]))
        out["per_batch"][f"B={B}"] = {"device_ms_per_window": round(d / B, 4), "host_ms_per_window": round(h / B, 4), "device_over_host": round(d / h, 3)}
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
