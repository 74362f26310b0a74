#!/usr/bin/env python3
"""Pixel selection and creation of the immature points (dsm_select_pixels_batch): ms per call and per sequence for 1 / 11 / 64
sequences, each KITTI-shaped (1232 x 368) with a new keyframe of its own in a tracker slot on the device, the whole call timed: host
validation and staging, the fixed launch sequence, the one read-back.  In the same run, on the same frames: a loop of
dsm_select_pixels_host (the plain sequential CPU form on one core, one call per sequence).

Every sequence enters with the same potential and density (--potential, --density; 3 and 1500 are a sequence's first keyframe under
the reference's presets), so with --potential 1 every pass runs at the potential where the chain is longest.  Both forms start every
repetition from that potential.  After a warm-up the batch sizes run in alternation; each figure is the median over the repetitions of
a host clock around the (synchronising) call.  The device results are compared with the host form's, bit for bit, before anything is
timed.  Prints one JSON line.

  python tools/select_timing.py [--reps 9] [--batches 1,11,64] [--potential 3] [--density 1500] [--no-host]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from direct_stereo_slam_amd import pixelselect as P  # noqa: E402
from direct_stereo_slam_amd import synth  # noqa: E402
from direct_stereo_slam_amd.tracker import Context, TrackerAndScaler  # noqa: E402

W, H, MAX_PTS = 1232, 368, 4000
f32 = np.float32


def base_texture():
    """integer-valued, so that the 2 x 2 means of levels 1 and 2 are exact whoever forms them: sinusoids over a slow gradient, with
    a flat band (few hits) and fine noise (many)"""
    rng = np.random.default_rng(11)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    v = 110.0 + 0.05 * xs
    for lam in np.linspace(7.0, 60.0, 8):
        th, ph = rng.uniform(0, np.pi), rng.uniform(0, 2 * np.pi)
        v += 9.0 * np.sin(2 * np.pi / lam * (xs * np.cos(th) + ys * np.sin(th)) + ph)
    v += rng.normal(0, 2.5, v.shape) * (ys > H / 3)
    return v


def pyramid(I0):
    out = [np.ascontiguousarray(I0, f32)]
    for _ in range(2):
        a = out[-1]
        out.append((f32(0.25) * (((a[0::2, 0::2] + a[0::2, 1::2]) + a[1::2, 0::2]) + a[1::2, 1::2])).astype(f32))
    return out


def timed(f):
    t0 = time.perf_counter()
    f()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batches", default="1,11,64")
    ap.add_argument("--potential", type=int, default=3)
    ap.add_argument("--density", type=float, default=1500.0)
    ap.add_argument("--no-host", action="store_true", help="time the device form alone (a kernel trace of the run then holds nothing else)")
    args = ap.parse_args()
    batches = [int(b) for b in args.batches.split(",")]
    ctx = Context(0)
    n = max(batches)
    tex = base_texture()
    rng = np.random.default_rng(5)
    pattern = P.random_pattern(W, H)
    sel = P.PixelSelector(ctx, W, H, n, pattern)
    jobs, planes, trackers = [], [], []
    for j in range(n):
        I0 = np.clip(np.rint(np.roll(tex, (int(rng.integers(0, H)), int(rng.integers(0, W))), axis=(0, 1))), 0, 255).astype(f32)
        trk = TrackerAndScaler(ctx, W, H, 3, synth.KITTI_T_STEREO, (718.0, 718.0, W / 2.0, H / 2.0))
        trk.upload_image(0, I0)
        trackers.append(trk), planes.append(pyramid(I0))
        jobs.append(dict(tracker=trk, slot=0, density=args.density, potential=args.potential, max_pts=MAX_PTS, want_map=False))
    p = P.params()
    forms = {B: P.SelectBatch(jobs[:B], W, H) for B in batches}
    host = P.SelectBatch(jobs, W, H)
    # the device form against the host form before anything is timed
    forms[n].run(sel, p)
    dev = forms[n].results()
    if not args.no_host:
        for j in range(n):
            host.run_host(j, planes[j], pattern, p)
        for j, (d, h) in enumerate(zip(dev, host.results())):
            for k in d:
                a, b = np.asarray(d[k]), np.asarray(h[k])
                same = a.tobytes() == b.tobytes() if a.dtype != np.float32 else bool(np.all((a.view(np.uint32) == b.view(np.uint32))))
                if not same:
                    raise SystemExit(f"sequence {j}: the device form and the host form disagree in {k}")

    def run_dev(b):
        b.reset()
        return timed(lambda: b.run(sel, p))

    def run_host(B):
        host.reset()
        return timed(lambda: [host.run_host(j, planes[j], pattern, p) for j in range(B)])

    for _ in range(args.warmup):
        for b in forms.values():
            run_dev(b)
    t_run, t_host = {B: [] for B in batches}, {B: [] for B in batches}
    for _ in range(args.reps):
        for B, b in forms.items():
            t_run[B].append(run_dev(b))
            if not args.no_host:
                t_host[B].append(run_host(B))
    out = {"tool": "select_timing", "reps": args.reps, "geometry": [W, H], "potential": args.potential, "density": args.density,
           "compared_with_host_form": not args.no_host, "mean_points": round(float(np.mean([d["n_pts"] for d in dev])), 1),
           "mean_passes": round(float(np.mean([d["passes"] for d in dev])), 3),
           "potentials_after": sorted({d["potential"] for d in dev}), "per_batch": {}}
    for B in batches:
        ms = float(np.median(t_run[B]))
        r = {"device_ms_per_call": round(ms, 3), "device_ms_per_sequence": round(ms / B, 4)}
        if not args.no_host:
            hs = float(np.median(t_host[B]))
            r.update({"host_loop_ms": round(hs, 3), "host_ms_per_sequence": round(hs / B, 4), "host_over_device": round(hs / ms, 2)})
        out["per_batch"][f"B={B}"] = r
    sel.close()
    for t in trackers:
        t.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
