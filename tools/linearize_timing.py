#!/usr/bin/env python3
"""Linearisation of the active residuals (dsm_linearize_residuals_batch): ms per call and per window for 1 / 11 / 64 windows, each
KITTI-shaped (1232 x 368, 8 keyframes, 2 000 points with a host among them and a residual against each of the 7 other frames, 8
pixels each), the whole call timed: host validation and staging, the one launch, the one read-back, the energy sum and the order
statistic.  In the same run, on the same inputs: a loop of dsm_linearize_residuals_host (the plain sequential CPU form on one core,
one call per window; not the reference's thread pool).  Both are timed twice: with the Jacobian rows, centres and projections read back
(296 + 12 + 64 bytes per residual) and with states and energies alone.  Every window has its own images (a texture seen at the
disparities of a plane) on the device (dsm_window) and on the host.  After a warm-up the variants run in alternation; each figure is
the median over the repetitions of a host clock around the (synchronising) call.  Every device result is compared with the host
form's, bit for bit, before anything is timed.  Prints one JSON line.

  python tools/linearize_timing.py [--reps 9] [--batches 1,11,64]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from direct_stereo_slam_amd import linearize as L  # noqa: E402
from direct_stereo_slam_amd.tracker import Context  # noqa: E402

W, H, N_FRAMES, N_PTS, PLANE_IDEPTH = 1232, 368, 8, 2000, 0.25
PATTERN = [(0, -2), (-1, -1), (1, -1), (-2, 0), (0, 0), (2, 0), (-1, 1), (0, 2)]
ROWS = ("J", "center_projected_to", "projected_to")
f32 = np.float32


def base_texture():
    rng = np.random.default_rng(11)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float32)
    v = np.full((H, W), 128.0, np.float32)
    for lam in np.linspace(6.0, 30.0, 6):
        th, ph = rng.uniform(0, np.pi), rng.uniform(0, 2 * np.pi)
        v += f32(13.0) * np.sin(f32(2 * np.pi / lam) * (xs * f32(np.cos(th)) + ys * f32(np.sin(th))) + f32(ph))
    return v


def window(seed, tex):
    """one sequence's window: frame k sees the texture moved by an integer disparity (camera k at t_x = shift / (fx idepth)), the
    last frame 30 brighter; points anywhere their pattern fits, hosted by any frame, idepth around the plane's, the linearisation
    point a little off the current state; a residual for every (point, other frame) pair, all entering IN"""
    rng = np.random.default_rng(seed)
    fx, cx, cy = f32(0.58 * W), f32(0.5 * W - 0.5), f32(0.5 * H - 0.5)
    K = np.array([[float(fx), 0, float(cx)], [0, float(fx), float(cy)], [0, 0, 1.0]])
    base = np.roll(tex, (int(rng.integers(0, H)), int(rng.integers(0, W))), axis=(0, 1))
    shifts = [0] + [(3 * (k + 1)) * (1 if k % 2 == 0 else -1) for k in range(N_FRAMES - 1)]
    frames = [np.ascontiguousarray(np.roll(base, s, axis=1)) for s in shifts]
    frames[-1] = frames[-1] + f32(30.0)
    cams = [np.array([s / (float(fx) * PLANE_IDEPTH), 0.0, 0.001 * k]) for k, s in enumerate(shifts)]
    t = np.array([[cams[b] - cams[a] for b in range(N_FRAMES)] for a in range(N_FRAMES)])
    eye = np.tile(np.eye(3, dtype=f32).reshape(9), (N_FRAMES, N_FRAMES, 1))
    host = rng.integers(0, N_FRAMES, N_PTS).astype(np.int32)
    u, v = rng.integers(3, W - 3, N_PTS), rng.integers(3, H - 3, N_PTS)
    stack = np.stack(frames)
    color = np.stack([stack[host, v + dy, u + dx] for dx, dy in PATTERN], axis=1).astype(f32)
    idepth = (PLANE_IDEPTH * (1.0 + rng.uniform(-0.2, 0.2, N_PTS))).astype(f32)
    point = np.repeat(np.arange(N_PTS, dtype=np.int32), N_FRAMES - 1)
    target = np.concatenate([[f for f in range(N_FRAMES) if f != h] for h in host]).astype(np.int32)
    n_res = len(point)
    job = dict(cam=(fx, fx, cx, cy), cam_inv=(f32(1.0) / fx, f32(1.0) / fx), frame_ids=np.arange(N_FRAMES, dtype=np.int32),
               pre_RTll_0=eye, pre_tTll_0=(t * 1.01).astype(f32), pre_KRKiTll=eye, pre_KtTll=(t @ K.T).astype(f32),
               pre_aff_mode=np.tile(np.array([1.0, 0.0], f32), (N_FRAMES, N_FRAMES, 1)), pre_b0_mode=np.zeros((N_FRAMES, N_FRAMES), f32),
               frame_energy_th=np.full(N_FRAMES, 8 * 144.0, f32), host=host, u=u.astype(f32), v=v.astype(f32), idepth_scaled=idepth,
               idepth_zero_scaled=(idepth * f32(1.01)).astype(f32), color=color,
               weights=np.sqrt(2500.0 / (2500.0 + rng.uniform(0, 400, (N_PTS, 8)))).astype(f32), point=point, target=target,
               state_in=np.zeros(n_res, np.uint8), energy_in=np.zeros(n_res, f32), is_new=np.zeros(n_res, np.uint8), fix_linearization=0)
    return job, frames


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
    jobs, frames, wins = [], [], []
    for j in range(n):
        job, fr = window(900 + j, tex)
        win = L.KeyframeWindow(ctx, W, H, N_FRAMES)
        for fid, img in zip(job["frame_ids"], fr):
            win.put_host(int(fid), img)
        jobs.append(dict(job, window=win)), frames.append(fr), wins.append(win)
    variants = {"with_rows": ROWS, "states_only": ()}
    forms = {(B, name): L.LinearizeBatch(jobs[:B], outs) for B in batches for name, outs in variants.items()}
    host = {name: L.LinearizeBatch(jobs, outs) for name, outs in variants.items()}
    params = L.default_params()
    # the device form against the host form before anything is timed
    states = []
    for name in variants:
        forms[(n, name)].run(ctx, params)
        dev = forms[(n, name)].results()
        for j in range(n):
            host[name].run_host(W, H, j, frames[j], params)
        for j, (d, h) in enumerate(zip(dev, host[name].results())):
            if any(np.asarray(d[k]).tobytes() != np.asarray(h[k]).tobytes() for k in d):
                raise SystemExit(f"window {j} ({name}): the device form and the host form disagree")
        states = np.concatenate([d["new_state"] for d in dev])
    for _ in range(args.warmup):
        for b in forms.values():
            b.run(ctx, params)
    t_run, t_host = {k: [] for k in forms}, {k: [] for k in forms}
    for _ in range(args.reps):
        for (B, name), b in forms.items():
            t_run[(B, name)].append(timed(lambda: b.run(ctx, params)))
            t_host[(B, name)].append(timed(lambda: [host[name].run_host(W, H, j, frames[j], params) for j in range(B)]))
    n_res = N_PTS * (N_FRAMES - 1)
    out = {"tool": "linearize_timing", "reps": args.reps, "geometry": [W, H], "frames": N_FRAMES, "points_per_window": N_PTS,
           "residuals_per_window": n_res, "state_share": [round(float((states == k).mean()), 4) for k in (0, 1, 2)], "per_batch": {}}
    for B in batches:
        row = {}
        for name in variants:
            ms, hs = float(np.median(t_run[(B, name)])), float(np.median(t_host[(B, name)]))
            row[name] = {"device_ms_per_call": round(ms, 3), "device_ms_per_window": round(ms / B, 4), "host_loop_ms": round(hs, 3),
                         "host_ms_per_window": round(hs / B, 4), "host_over_device": round(hs / ms, 2)}
        out["per_batch"][f"B={B}"] = row
    for w in wins:
        w.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
