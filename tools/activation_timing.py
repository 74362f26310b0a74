#!/usr/bin/env python3
"""Distance map and point activation (dsm_activate_points_batch): ms per call and per sequence for 1 / 11 / 64 sequences, each with a
KITTI-shape window (1232 x 368, 7 hosts x 2 000 seeds, 8 000 candidates, min_act_dist 2), the whole call timed: host validation and
staging, the launch sequence, the one read-back.  In the same run, on the same inputs: a loop of dsm_activate_points_host (the plain
sequential CPU form, one call per sequence) and dsm_distmaps_make alone (D1-D4, the share of the batched call that is map
construction).  The share of candidates left after the pre-filter -- in bounds and passing against the map before any activation,
the only ones the selection can ever accept -- is counted on the host from the constructed maps.  After a warm-up the batch sizes
run in alternation; each figure is the median over the repetitions of a host clock around the (synchronising) call.  Every device
result is compared with the host form's before anything is timed.  Prints one JSON line.

  python tools/activation_timing.py [--reps 9] [--batches 1,11,64]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from direct_stereo_slam_amd import distmap as D  # noqa: E402
from direct_stereo_slam_amd.tracker import Context  # noqa: E402

W, H, N_HOSTS, SEEDS_PER_HOST, N_CAND, MIN_ACT = 1232, 368, 7, 2000, 8000, 2.0
f32 = np.float32


def window(seed):
    """one sequence's window: hosts a small rotation and translation away from the newest frame, points anywhere in the image"""
    rng = np.random.default_rng(seed)
    fx, cx, cy = f32(0.58 * W), f32(0.5 * W - 0.5), f32(0.5 * H - 0.5)
    K1 = np.array([[fx * f32(0.5), 0, (cx + 0.5) / 2 - 0.5], [0, fx * f32(0.5), (cy + 0.5) / 2 - 0.5], [0, 0, 1]], f32)
    Ki0 = np.array([[1 / fx, 0, -cx / fx], [0, 1 / fx, -cy / fx], [0, 0, 1]], f32)
    krki, kt = np.zeros((N_HOSTS, 9), f32), np.zeros((N_HOSTS, 3), f32)
    for i in range(N_HOSTS):
        a = rng.normal(0, 0.01, 3)
        R = np.eye(3) + np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        krki[i] = (K1 @ R.astype(f32) @ Ki0).reshape(9)
        kt[i] = K1 @ rng.normal(0, 0.05, 3).astype(f32)

    def pts(n):
        return (rng.integers(0, N_HOSTS, n).astype(np.int32), rng.uniform(-4, W + 4, n).astype(f32), rng.uniform(-4, H + 4, n).astype(f32),
                rng.uniform(0.1, 2.0, n).astype(f32))

    sh, su, sv, sd = pts(N_HOSTS * SEEDS_PER_HOST)
    ch, cu, cv, cd = pts(N_CAND)
    return dict(krki=krki, kt=kt, seed_host=sh, seed_u=su, seed_v=sv, seed_idepth=sd, cand_host=ch, cand_u=cu, cand_v=cv, cand_idepth=cd,
                cand_type=rng.choice(np.array([1, 2, 4], f32), N_CAND).astype(f32), min_act_dist=MIN_ACT)


def pass_initial(job, m0):
    """candidates in bounds that pass against the constructed map m0 (float32 arithmetic as D2 / D6)"""
    M, T = job["krki"][job["cand_host"]], job["kt"][job["cand_host"]]
    u, v, d = job["cand_u"], job["cand_v"], job["cand_idepth"]
    p = [((M[:, 3 * r] * u + M[:, 3 * r + 1] * v) + M[:, 3 * r + 2]) + T[:, r] * d for r in range(3)]
    qu, qv = p[0] / p[2] + f32(0.5), p[1] / p[2] + f32(0.5)
    h1, w1 = m0.shape
    ok = (qu >= 1) & (qv >= 1) & (qu < f32(w1)) & (qv < f32(h1))
    cell = qu[ok].astype(np.int64) + w1 * qv[ok].astype(np.int64)
    dist = m0.reshape(-1)[cell] + (p[0][ok] - np.floor(p[0][ok]))
    return int(ok.sum()), int((dist >= f32(job["min_act_dist"]) * job["cand_type"][ok]).sum())


def timed(f):
    t0 = time.perf_counter()
    f()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batches", default="1,11,64")
    args = ap.parse_args()
    batches = [int(b) for b in args.batches.split(",")]
    ctx = Context(0)
    n = max(batches)
    maps = [D.DistanceMap(ctx, W, H) for _ in range(n)]
    jobs = [dict(window(500 + j), map=maps[j]) for j in range(n)]
    forms = {B: D.ActivationBatch(jobs[:B]) for B in batches}
    host = D.ActivationBatch(jobs)
    # the device form against the host form, and the pre-filter share, before anything is timed
    forms[n].make(ctx)
    in_bounds = passing = 0
    for j in range(n):
        a, b = pass_initial(jobs[j], maps[j].get())
        in_bounds, passing = in_bounds + a, passing + b
    forms[n].run(ctx)
    dev = forms[n].results()
    hm = np.empty((H >> 1, W >> 1), f32)
    for j in range(n):
        host.run_host(W, H, j, hm)
        r = host.results()[j]
        if not (np.array_equal(r["decisions"], dev[j]["decisions"]) and np.array_equal(hm, maps[j].get())):
            raise SystemExit(f"sequence {j}: the device form and the host form disagree")
    n_act = sum(r["n_activated"] for r in dev)
    for _ in range(args.warmup):
        for B, b in forms.items():
            b.run(ctx)
            b.make(ctx)
    t_run, t_make, t_host = {B: [] for B in batches}, {B: [] for B in batches}, {B: [] for B in batches}
    for _ in range(args.reps):
        for B, b in forms.items():
            t_run[B].append(timed(lambda: b.run(ctx)))
            t_make[B].append(timed(lambda: b.make(ctx)))
            t_host[B].append(timed(lambda: [host.run_host(W, H, j) for j in range(B)]))
    out = {"tool": "activation_timing", "reps": args.reps, "geometry": [W, H], "seeds": N_HOSTS * SEEDS_PER_HOST, "candidates": N_CAND,
           "min_act_dist": MIN_ACT, "activated_per_sequence": round(n_act / n, 1),
           "candidates_in_bounds_share": round(in_bounds / (n * N_CAND), 4), "candidates_after_prefilter_share": round(passing / (n * N_CAND), 4),
           "per_batch": {}}
    for B in batches:
        ms, mk, hs = (float(np.median(t[B])) for t in (t_run, t_make, t_host))
        out["per_batch"][f"B={B}"] = {"device_ms_per_call": round(ms, 3), "device_ms_per_sequence": round(ms / B, 4),
                                      "device_make_only_ms_per_call": round(mk, 3), "host_loop_ms": round(hs, 3),
                                      "host_ms_per_sequence": round(hs / B, 4), "host_over_device": round(hs / ms, 2)}
    for m in maps:
        m.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
