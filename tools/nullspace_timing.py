#!/usr/bin/env python3
"""The window's nullspaces and their pseudo-inverse for 1 / 11 / 64 windows of 8 keyframes (N = 68): ms per window of
  (a) device  one dsm_window_nullspace_batch (the optional outputs NULL), whole synchronous call
  (b) host    a loop of dsm_window_nullspace_host over the same windows on one core
in the same run, on the same poses (rotations up to 0.3 rad, translations of a few units).  After a warm-up the two run in alternation;
each figure is the median over the repetitions of a host clock.  Before anything is timed the device's result is compared with the host
form's behind the device's own blocks (bit for bit) and its blocks with the host form's.  There is no pass mark.  Prints one JSON line.

  python tools/nullspace_timing.py [--reps 15] [--batches 1,11,64]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from direct_stereo_slam_amd import nullspace as NS  # noqa: E402
from direct_stereo_slam_amd.tracker import Context  # noqa: E402

N_FRAMES = 8


def window(seed):
    rng = np.random.default_rng(seed)
    ev = np.zeros((N_FRAMES, 7))
    for f in range(N_FRAMES):
        axis = rng.normal(0, 1, 3)
        axis /= np.linalg.norm(axis)
        th = rng.uniform(0.0, 0.3)
        ev[f, :3], ev[f, 3] = np.sin(th / 2) * axis, np.cos(th / 2)
        ev[f, :4] /= np.linalg.norm(ev[f, :4])
        ev[f, 4:] = rng.normal(0, 2.0, 3)
    zero = np.zeros((N_FRAMES, 8))
    zero[:, 6] = rng.normal(0, 0.02, N_FRAMES)
    return dict(world_to_cam_eval=ev, state_zero=zero, exposure=rng.uniform(0.5, 2.0, N_FRAMES).astype(np.float32))


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
    jobs = [window(300 + j) for j in range(max(batches))]
    dev = NS.window_nullspace_batch(ctx, jobs)
    behind = NS.window_nullspace_host([dict(job, frame_null_in=d["frame_null"]) for job, d in zip(jobs, dev)])
    own = NS.window_nullspace_host(jobs)
    core = ("null_basis", "null_pinv", "sing", "rank", "flags")
    for j, (d, b, o) in enumerate(zip(dev, behind, own)):
        if d["flags"] or d["rank"] != 7 or any(np.asarray(d[k]).tobytes() != np.asarray(b[k]).tobytes() for k in core):
            raise SystemExit(f"window {j}: the device form and the host form behind its blocks disagree")
        if not np.allclose(d["frame_null"], o["frame_null"], rtol=0, atol=1e-9):
            raise SystemExit(f"window {j}: the device's blocks and the host form's disagree")
    blocks_equal = all(d["frame_null"].tobytes() == o["frame_null"].tobytes() for d, o in zip(dev, own))
    calls = {B: (NS.NullspaceBatch(jobs[:B], ()), NS.NullspaceBatch(jobs[:B], ())) for B in batches}
    for _ in range(args.warmup):
        for B in batches:
            calls[B][0].run(ctx), calls[B][1].run_host()
    t = {(B, k): [] for B in batches for k in ("device", "host")}
    for _ in range(args.reps):
        for B in batches:
            t[(B, "device")].append(timed(lambda: calls[B][0].run(ctx)))
            t[(B, "host")].append(timed(lambda: calls[B][1].run_host()))
    out = {"tool": "nullspace_timing", "reps": args.reps, "frames": N_FRAMES, "N": 4 + 8 * N_FRAMES,
           "device_blocks_equal_host_bit_for_bit": bool(blocks_equal), "per_batch": {}}
    for B in batches:
        d, h = float(np.median(t[(B, "device")])), float(np.median(t[(B, "host")]))
        out["per_batch"][f"B={B}"] = {"device_ms_per_window": round(d / B, 4), "host_ms_per_window": round(h / B, 4), "device_over_host": round(d / h, 3)}
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
