#!/usr/bin/env python3
"""Marginalising points and frames on the device (dsm_window_marginalize_batch): ms per call and per window for 1 / 11 / 64 windows of
the workload of tools/linearize_timing.py (KITTI-shaped, 1232 x 368, 8 keyframes, 2 000 points, 14 000 residuals) as optimize leaves
them: frame 0 is flagged and leaves, so the points it hosts (about 250, each with 7 residuals) are marginalised and every other
point is kept; the whole synchronous call timed, every optional output NULL.  In the same run, on the same inputs: a loop of
dsm_window_marginalize_host (one core, one call per window).  After a warm-up the two run in alternation; each figure is the median
over the repetitions of a host clock.  Every device result is compared with the host form's, bit for bit, before anything is timed.
Prints one JSON line.

  python tools/marginalize_timing.py [--reps 9] [--batches 1,11,64]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import hessian_timing as HT  # noqa: E402
import linearize_timing as LT  # noqa: E402
import solve_timing as ST  # noqa: E402
from direct_stereo_slam_amd import linearize as L  # noqa: E402
from direct_stereo_slam_amd import marginalize as MG  # noqa: E402
from direct_stereo_slam_amd.tracker import Context  # noqa: E402

f32 = np.float32


def marg_extras(seed):
    """what a marginalize job holds on top of the Hessian job: frame 0 flagged and leaving, every point good enough to be marginalised
    once its host is flagged, small deltas, the prior system of tools/solve_timing.py"""
    rng = np.random.default_rng(seed)
    nf, n = LT.N_FRAMES, LT.N_PTS
    flagged = np.zeros(nf, np.uint8)
    flagged[0] = 1
    sol = ST.solve_extras(seed)
    return dict(flagged=flagged, n_good_residuals=np.full(n, 9, np.int32), last_state=np.zeros((n, 2), np.uint8),
                idepth_hessian=np.full(n, 100.0, f32), ad_ht_delta=rng.normal(0, 0.01, (nf, nf, 8)).astype(f32),
                c_delta=rng.normal(0, 0.01, 4).astype(f32), H_M=sol["H_M"], b_M=sol["b_M"], marg_frames=np.array([0], np.int32),
                frame_prior=rng.uniform(0, 1e3, (1, 8)), frame_delta_prior=rng.normal(0, 0.01, (1, 8)))


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
        jobs.append(dict(job, window=win, **HT.extras(5000 + j), **marg_extras(7000 + j))), frames.append(fr), wins.append(win)
    params, mp = L.default_params(), MG.default_marg_params()
    # the device form against the host form before anything is timed, every output asked for
    check_dev, check_host = MG.MarginalizeBatch(jobs), MG.MarginalizeBatch(jobs)
    check_dev.run(ctx, params, mp)
    for j in range(n):
        check_host.run_host(LT.W, LT.H, j, frames[j], params, mp)
    n_marg, n_res = [], []
    for j, (d, h) in enumerate(zip(check_dev.results(), check_host.results())):
        if any(np.asarray(d[k]).tobytes() != np.asarray(h[k]).tobytes() for k in d):
            raise SystemExit(f"window {j}: the device form and the host form disagree")
        n_marg.append(int((d["verdict"] == MG.MARGINALIZE).sum())), n_res.append(d["n_res_marg"])
    del check_dev, check_host
    device = {B: MG.MarginalizeBatch(jobs[:B], ()) for B in batches}
    host = MG.MarginalizeBatch(jobs, ())
    for _ in range(args.warmup):
        for B in batches:
            device[B].run(ctx, params, mp)
    t = {(B, k): [] for B in batches for k in ("device", "host_form")}
    for _ in range(args.reps):
        for B in batches:
            t[(B, "device")].append(LT.timed(lambda: device[B].run(ctx, params, mp)))
            t[(B, "host_form")].append(LT.timed(lambda: [host.run_host(LT.W, LT.H, j, frames[j], params, mp) for j in range(B)]))
    out = {"tool": "marginalize_timing", "reps": args.reps, "geometry": [LT.W, LT.H], "frames": LT.N_FRAMES, "points_per_window": LT.N_PTS,
           "marginalised_points_per_window": round(float(np.mean(n_marg)), 1), "active_residuals_per_window": round(float(np.mean(n_res)), 1),
           "frames_leaving": 1, "per_batch": {}}
    for B in batches:
        m = {k: float(np.median(t[(B, k)])) for k in ("device", "host_form")}
        out["per_batch"][f"B={B}"] = {"device_ms_per_call": round(m["device"], 4), "device_ms_per_window": round(m["device"] / B, 4),
                                      "host_form_ms_per_window": round(m["host_form"] / B, 4), "device_over_host_form": round(m["device"] / m["host_form"], 3)}
    for w in wins:
        w.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
