#!/usr/bin/env python3
"""Loop chain of S concurrent sequences, each with its own ring-key index (one LoopHandler each, LoopHandler.cpp:35-39): per keyframe
ms of
  (a) S calls of dsm_loop_detect_batch, one job each, each on its own index (the correct search without the _many form),
  (b) one dsm_loop_detect_batch_many call (one index per job),
  (c) one dsm_loop_detect_batch call over ONE shared index (the batched cost without the _many form; different semantics),
and of the search alone: S dsm_ringdb_query_then_enqueue calls against one dsm_ringdb_query_then_enqueue_many call.
Every index holds 2000 keys (about a KITTI-00 run's keyframes) and a full delay queue, so every call matures one key per index.  The
clouds are those of bench.py's loop_chain_leg: 8 keyframes, 16 000 points per job.  After a warm-up the forms run in alternation;
each figure is the median over the repetitions of a host clock around the (synchronising) calls.  Prints one JSON line.

  python tools/loop_chain_sequences.py [--reps 15] [--seqs 1,11,64]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KEYS_PER_INDEX = 2000
MARGIN = 100


def job(seed, n_pts=16000):
    """bench.py loop_chain_leg's keyframe: a street canyon seen from the current camera, 8 keyframes"""
    rng = np.random.default_rng(seed)
    n_kf = 8
    kf_ids = np.arange(100, 100 + n_kf)
    poses = np.hstack([rng.normal(0, 5, (n_kf, 3)), rng.normal(0, 0.08, (n_kf, 3))])
    cur_cw = np.hstack([np.eye(3), rng.normal(0, 1, (3, 1))])
    pt_kf = rng.choice(kf_ids, n_pts)
    g = np.stack([rng.uniform(-55, 55, n_pts), 1.6 + rng.normal(0, 0.05, n_pts), rng.uniform(-55, 55, n_pts)], 1)
    walls = rng.random(n_pts) < 0.35
    g[walls, 0] = np.where(rng.random(walls.sum()) < 0.5, 8.0, -9.0)
    g[walls, 1] = rng.uniform(-5, 1.6, walls.sum())
    return kf_ids, poses, cur_cw, pt_kf, g - cur_cw[:, 3]


def filled_index(ctx, seed):
    """an index as a running sequence holds it: KEYS_PER_INDEX entries and a full delay queue"""
    from direct_stereo_slam_amd.ringdb import RingKeyDB

    rng = np.random.default_rng(seed)
    p = rng.uniform(0.1, 0.9, 20)
    keys = (rng.binomial(60, p, size=(KEYS_PER_INDEX + MARGIN, 20)) / 60.0).astype(np.float32)
    db = RingKeyDB(ctx, margin=MARGIN, capacity=4096)
    db.add_points(keys[:KEYS_PER_INDEX])
    for k in keys[KEYS_PER_INDEX:]:
        db.enqueue(k)
    return db


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seqs", default="1,11,64")
    args = ap.parse_args()
    from direct_stereo_slam_amd.ringdb import LoopBatch, query_then_enqueue_many
    from direct_stereo_slam_amd.tracker import Context

    ctx = Context(0)
    counts = [int(s) for s in args.seqs.split(",")]
    jobs = [job(900 + s) for s in range(max(counts))]
    out = {"tool": "loop_chain_sequences", "keys_per_index": KEYS_PER_INDEX, "margin": MARGIN, "points_per_job": 16000,
           "reps": args.reps, "ms_per_keyframe": {}}
    for S in counts:
        own_a = [filled_index(ctx, 10 * s + 1) for s in range(S)]
        own_b = [filled_index(ctx, 10 * s + 1) for s in range(S)]
        shared = filled_index(ctx, 7)
        a = [LoopBatch(ctx, [jobs[s]], 40.0, db=own_a[s], selected_points=False) for s in range(S)]
        b = LoopBatch(ctx, jobs[:S], 40.0, dbs=own_b, selected_points=False)
        c = LoopBatch(ctx, jobs[:S], 40.0, db=shared, selected_points=False)
        b.run()
        keys = np.stack([o["ringkey"] for o, _ in b.outs])
        srch_a = [filled_index(ctx, 10 * s + 3) for s in range(S)]
        srch_b = [filled_index(ctx, 10 * s + 3) for s in range(S)]

        def run_a():
            for x in a:
                x.run()

        def search_a():
            for db, k in zip(srch_a, keys):
                db.search_ringkey(k)

        forms = {"a_per_sequence_calls": run_a, "b_many_call": b.run, "c_shared_index_call": c.run,
                 "search_per_sequence_calls": search_a, "search_many_call": lambda: query_then_enqueue_many(srch_b, keys)}
        for _ in range(args.warmup):
            for f in forms.values():
                f()
        t = {name: [] for name in forms}
        for _ in range(args.reps):
            for name, f in forms.items():
                t[name].append(timed(f))
        med = {name: round(float(np.median(v)) / S, 4) for name, v in t.items()}
        med["a_over_b"] = round(med["a_per_sequence_calls"] / med["b_many_call"], 2)
        med["b_over_c"] = round(med["b_many_call"] / med["c_shared_index_call"], 3)
        med["search_ratio"] = round(med["search_per_sequence_calls"] / med["search_many_call"], 2)
        out["ms_per_keyframe"][f"S={S}"] = med
        for db in own_a + own_b + srch_a + srch_b + [shared]:
            db.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
