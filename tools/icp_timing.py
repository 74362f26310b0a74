#!/usr/bin/env python3
"""ICP fallback of loop closure on the device (dsm_icp_batch): ms per call and per match for batches of 1 / 11 / 64 matches of clouds of
2 000 / 10 000 / 20 000 points per side (two samplings of one street place, tests/_icp_ref.street, seen from poses 0.05 rad and 1.3 m
apart), the whole call timed: host staging, the launch sequence, the one read-back.  Pair evaluations of the brute-force scan are
counted from the results (every correspondence search and the fitness pass: n_src x n_tgt each) and given per second of the whole
call.  After a warm-up the batch sizes of one cloud size run in alternation; each figure is the median over the repetitions of a host
clock around the (synchronising) call.  The numpy checker of the contract (tests/_icp_ref.py) is timed on one match per size, once:
labelled as numpy, it is not PCL (which cannot be run here).  Prints one JSON line.

  python tools/icp_timing.py [--reps 9] [--sizes 2000,10000,20000] [--batches 1,11,64] [--numpy-sizes 2000,10000]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _icp_ref as R  # noqa: E402
from direct_stereo_slam_amd import icp as I  # noqa: E402
from direct_stereo_slam_amd.tracker import Context  # noqa: E402


def match(seed, n):
    """(pts_source, pts_target, guess): the matched keyframe's cloud, the current one's (another sampling of the place, moved), identity"""
    rng = np.random.default_rng(seed)
    T = R.rigid(R.rot((0.0, 0.05, 0.0)), [0.4, 0.0, 1.2])
    src = R.street(rng, n)
    tgt = R.street(rng, n) @ T[:3, :3].T + T[:3, 3] + rng.normal(0, 0.02, (n, 3))
    return src, tgt, np.eye(4)


def timed(f):
    t0 = time.perf_counter()
    f()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="2000,10000,20000")
    ap.add_argument("--batches", default="1,11,64")
    ap.add_argument("--numpy-sizes", default="2000,10000")
    args = ap.parse_args()
    sizes = [int(s) for s in args.sizes.split(",")]
    batches = [int(b) for b in args.batches.split(",")]
    ctx = Context(0)
    out = {"tool": "icp_timing", "reps": args.reps, "per_size": {}}
    for n in sizes:
        jobs = [match(1000 * n + j, n) for j in range(max(batches))]
        forms = {B: I.IcpBatch(ctx, jobs[:B]) for B in batches}
        for _ in range(args.warmup):
            for b in forms.values():
                b.run()
        t = {B: [] for B in batches}
        for _ in range(args.reps):
            for B, b in forms.items():
                t[B].append(timed(b.run))
        row = {}
        for B, b in forms.items():
            res = b.results()
            pairs = sum((len(r["corr_counts"]) + 1) * n * n for r in res)
            ms = float(np.median(t[B]))
            row[f"B={B}"] = {"ms_per_call": round(ms, 3), "ms_per_match": round(ms / B, 4), "pairs": pairs,
                             "pairs_per_s_whole_call": float(f"{pairs / (ms * 1e-3):.3g}"),
                             "iterations": sorted(set(r["iterations"] for r in res)), "ok": sum(r["ok"] for r in res)}
        out["per_size"][f"n={n}"] = row
    out["numpy_checker_ms_per_match"] = {}
    for n in [int(s) for s in args.numpy_sizes.split(",") if s]:
        src, tgt, guess = match(1000 * n, n)
        out["numpy_checker_ms_per_match"][f"n={n}"] = round(timed(lambda: R.icp(src, tgt, guess)), 1)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
