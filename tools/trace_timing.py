#!/usr/bin/env python3
"""Tracing of the immature points (dsm_trace_points_batch): ms per call and per sequence for 1 / 11 / 64 sequences, each KITTI-shaped
(1232 x 368) with 8 hosts x 2 000 immature points and a new frame of its own on the device (dsm_window) and on the host, the whole
call timed: host validation and staging, the one launch, the one read-back.  In the same run, on the same inputs: a loop of
dsm_trace_points_host (the plain sequential CPU form on one core, one call per sequence).

The state that is timed is the points' state after two earlier traces against two earlier frames, produced with the host form, so
that fresh, narrowed, skipped and out-of-bounds points are mixed: a fifth of the points is created (fresh) before each of the three
frames' traces, the rest before the first.  Both forms start every repetition from that state.  After a warm-up the batch sizes run
in alternation; each figure is the median over the repetitions of a host clock around the (synchronising) call.  The device results
are compared with the host form's, bit for bit, before anything is timed.  Prints one JSON line.

  python tools/trace_timing.py [--reps 9] [--batches 1,11,64]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from direct_stereo_slam_amd import immature as M  # noqa: E402
from direct_stereo_slam_amd import trace as T  # noqa: E402
from direct_stereo_slam_amd.tracker import Context  # noqa: E402

W, H, N_HOSTS, PTS_PER_HOST, PLANE_IDEPTH = 1232, 368, 8, 2000, 0.25
PATTERN = [(0, -2), (-1, -1), (1, -1), (-2, 0), (0, 0), (2, 0), (-1, 1), (0, 2)]
f32 = np.float32


def base_texture():
    rng = np.random.default_rng(11)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float32)
    v = np.full((H, W), 128.0, np.float32)
    for lam in np.linspace(9.0, 40.0, 6):
        th, ph = rng.uniform(0, np.pi), rng.uniform(0, 2 * np.pi)
        v += f32(13.0) * np.sin(f32(2 * np.pi / lam) * (xs * f32(np.cos(th)) + ys * f32(np.sin(th))) + f32(ph))
    return v


def sequence(seed, tex):
    """one sequence: host k's image is the texture moved sideways by k + 2 px, frame m (m = 0, 1, 2: two earlier frames and the new
    one) by -(3 m + 2) px, all looking at a plane of idepth 0.25 with R = I, so host k sees frame m at K t = ((k + 3 m + 4) / 0.25, 0, 0).
    Points sit anywhere their pattern fits; colour, weights and gradH come from the host's image.  Returns (job, [frame 0, 1, 2],
    [K t of frame 0, 1, 2], the index of the frame before which each point is created)."""
    rng = np.random.default_rng(seed)
    base = np.roll(tex, (int(rng.integers(0, H)), int(rng.integers(0, W))), axis=(0, 1))
    hosts = np.stack([np.roll(base, -(k + 2), axis=1) for k in range(N_HOSTS)])
    frames = [np.ascontiguousarray(np.roll(base, 3 * m + 2, axis=1)) for m in range(3)]
    kts = [np.array([[(k + 3 * m + 4) / PLANE_IDEPTH, 0.0, 0.0] for k in range(N_HOSTS)], f32) for m in range(3)]
    n = N_HOSTS * PTS_PER_HOST
    host = np.repeat(np.arange(N_HOSTS, dtype=np.int32), PTS_PER_HOST)  # grouped by host, as traceNewCoarse walks them
    u, v = rng.integers(3, W - 3, n), rng.integers(3, H - 3, n)
    gx = {d: f32(0.5) * (hosts[host, v + d[1], u + d[0] + 1] - hosts[host, v + d[1], u + d[0] - 1]) for d in PATTERN}
    gy = {d: f32(0.5) * (hosts[host, v + d[1] + 1, u + d[0]] - hosts[host, v + d[1] - 1, u + d[0]]) for d in PATTERN}
    color = np.stack([hosts[host, v + dy, u + dx] for dx, dy in PATTERN], axis=1).astype(f32)
    color += rng.normal(0, 1.0, color.shape).astype(f32)
    color[rng.random(n) < 0.05] += f32(90.0)  # one point in twenty sees another surface
    grad_h = sum(np.stack([gx[d] * gx[d], gx[d] * gy[d], gx[d] * gy[d], gy[d] * gy[d]], axis=1) for d in PATTERN).astype(f32)
    weights = np.stack([np.sqrt(f32(2500.0) / (f32(2500.0) + gx[d] * gx[d] + gy[d] * gy[d])) for d in PATTERN], axis=1).astype(f32)
    born = np.where(rng.random(n) < 0.6, 0, rng.integers(1, 3, n))  # 60 % before the first frame, 20 % before each later one
    job = dict(krki=np.tile(np.eye(3, dtype=f32).reshape(9), (N_HOSTS, 1)), kt=kts[0], aff=np.tile(np.array([1.0, 0.0], f32), (N_HOSTS, 1)),
               host=host, u=u.astype(f32), v=v.astype(f32), energy_th=np.full(n, 8 * 144.0, f32), grad_h=grad_h, color=color, weights=weights,
               status=np.full(n, T.UNINITIALIZED, np.uint8), idepth_min=np.zeros(n, f32), idepth_max=np.full(n, np.nan, f32),
               quality=np.full(n, 10000.0, f32), trace_uv=np.zeros((n, 2), f32), trace_interval=np.zeros(n, f32))
    return job, frames, kts, born


def earlier_traces(job, frames, kts, born):
    """the host form against the two earlier frames; a point takes part from the frame before which it is created"""
    for m in range(2):
        res = T.trace_points_host(W, H, frames[m], dict(job, kt=kts[m]))
        alive = born <= m
        for k in T.STATE:
            job[k] = np.where(alive.reshape((-1,) + (1,) * (np.asarray(job[k]).ndim - 1)), res[k], job[k])
    return dict(job, kt=kts[2])


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
    tex = base_texture()
    jobs, targets, wins = [], [], []
    for j in range(n):
        job, frames, kts, born = sequence(900 + j, tex)
        job = earlier_traces(job, frames, kts, born)
        win = M.KeyframeWindow(ctx, W, H, 1)
        win.put_host(0, frames[2])
        jobs.append(dict(job, target=win, target_frame_id=0)), targets.append(frames[2]), wins.append(win)
    entering = np.concatenate([j["status"] for j in jobs])
    forms = {B: T.TraceBatch(jobs[:B]) for B in batches}
    host = T.TraceBatch(jobs)
    p = T.params()
    # the device form against the host form before anything is timed
    forms[n].run(ctx, p)
    dev = forms[n].results()
    for j in range(n):
        host.run_host(W, H, j, targets[j], p)
    for j, (d, h) in enumerate(zip(dev, host.results())):
        for k in d:
            a, b = d[k], h[k]
            same = a.tobytes() == b.tobytes() if a.dtype != np.float32 else bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))
            if not same:
                raise SystemExit(f"sequence {j}: the device form and the host form disagree in {k}")
    status = np.concatenate([d["status"] for d in dev])
    steps = np.concatenate([d["steps"] for d in dev])

    def run_dev(b):
        b.reset()
        return timed(lambda: b.run(ctx, p))

    def run_host(B):
        host.reset()
        return timed(lambda: [host.run_host(W, H, j, targets[j], p) for j in range(B)])

    for _ in range(args.warmup):
        for b in forms.values():
            run_dev(b)
    t_run, t_host = {B: [] for B in batches}, {B: [] for B in batches}
    for _ in range(args.reps):
        for B, b in forms.items():
            t_run[B].append(run_dev(b))
            t_host[B].append(run_host(B))
    names = ("good", "oob", "outlier", "skipped", "badcondition", "uninitialized")
    out = {"tool": "trace_timing", "reps": args.reps, "geometry": [W, H], "hosts": N_HOSTS, "points_per_sequence": N_HOSTS * PTS_PER_HOST,
           "status_share_entering": {k: round(float((entering == i).mean()), 4) for i, k in enumerate(names)},
           "status_share_after": {k: round(float((status == i).mean()), 4) for i, k in enumerate(names)},
           "searched_share": round(float((steps > 0).mean()), 4), "mean_steps": round(float(steps.mean()), 3),
           "mean_steps_of_searched": round(float(steps[steps > 0].mean()), 3), "per_batch": {}}
    for B in batches:
        ms, hs = float(np.median(t_run[B])), float(np.median(t_host[B]))
        out["per_batch"][f"B={B}"] = {"device_ms_per_call": round(ms, 3), "device_ms_per_sequence": round(ms / B, 4), "host_loop_ms": round(hs, 3),
                                      "host_ms_per_sequence": round(hs / B, 4), "host_over_device": round(hs / ms, 2)}
    for w in wins:
        w.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
