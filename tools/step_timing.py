#!/usr/bin/env python3
"""Six iterations of the window optimisation's loop, all accepted, on the device: ms per iteration and per window for 1 / 11 / 64
windows of the workload of tools/linearize_timing.py (KITTI-shaped, 1232 x 368, 8 keyframes, 2 000 points, 14 000 residuals), whole
synchronous calls timed.  In the same run, on the same inputs:
  (a) new_route   one dsm_window_step_batch per iteration (every optional output NULL): the step applied, everything derived from it,
                  the linearisation at the new state and the next solve
  (b) old_route   what an iteration cost before: dsm_window_solve_batch at state k, the step applied on one host core, and
                  dsm_linearize_residuals_batch at state k + 1 for the energy of the accept test.  The host share is timed as
                  dsm_window_step_host minus dsm_window_solve_host on the same window WITHOUT its residuals in the same repetition
                  (D1-E3 do not read them; with them the difference of two host forms of 11 ms each is noise)
The windows' poses are those tools/linearize_timing.py builds its tables from (world_to_cam without rotation), the state a small way
off the evaluation point, the step small.  The six calls of a repetition run on the same inputs: the call is stateless and its cost
does not depend on the values.  After a warm-up the variants run in alternation; each figure is the median over the repetitions of
a host clock.  Every device result is compared with the host form's before anything is timed.  Prints one JSON line.

  python tools/step_timing.py [--reps 9] [--batches 1,11,64] [--iterations 6]
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
from direct_stereo_slam_amd import solve as SV  # noqa: E402
from direct_stereo_slam_amd import step as SP  # noqa: E402
from direct_stereo_slam_amd.tracker import Context  # noqa: E402

f32 = np.float32


def step_job(job, seed):
    """the step job of a window of linearize_timing: its tables replaced by the poses they were built from"""
    rng = np.random.default_rng(seed)
    n, N = LT.N_FRAMES, 4 + 8 * LT.N_FRAMES
    fx = float(job["cam"][0])
    shifts = [0] + [(3 * (k + 1)) * (1 if k % 2 == 0 else -1) for k in range(n - 1)]
    ev = np.zeros((n, 7))
    ev[:, 3] = 1.0
    ev[:, 4:] = [[s / (fx * LT.PLANE_IDEPTH), 0.0, 0.001 * k] for k, s in enumerate(shifts)]
    zero = np.zeros((n, 8))
    backup = zero.copy()
    backup[1:, :6] = rng.normal(0, 1e-4, (n - 1, 6))
    backup[:, 6:] = rng.normal(0, 1e-5, (n, 2))
    fstep = np.zeros((n, 8))
    fstep[1:, :3], fstep[1:, 3:6] = rng.normal(0, 1e-3, (n - 1, 3)), rng.normal(0, 1e-4, (n - 1, 3))
    fstep[:, 6], fstep[:, 7] = rng.normal(0, 1e-4, n), rng.normal(0, 1e-6, n)
    czero = np.array([float(x) for x in job["cam"]]) / 50.0
    idb = np.asarray(job["idepth_scaled"], f32)
    pr = np.zeros(N)
    pr[:4], pr[4:10], pr[10::8], pr[11::8] = 5e9, 1e12, 1e12, 1e8
    out = {k: v for k, v in job.items() if k not in SP.FORMED + ("cam", "cam_inv")}
    out.update(world_to_cam_eval=ev, state_zero=zero, state_backup=backup, frame_step=fstep, calib_zero=czero, calib_backup=czero.copy(),
               calib_step=rng.normal(0, 1e-7, 4), idepth_backup=idb, idepth_step=(idb * rng.uniform(-0.01, 0.01, len(idb))).astype(f32),
               exposure=np.ones(n, f32), stepfac=np.ones(5, f32), state_prior=pr, state_prior_zero=np.concatenate([czero, np.zeros(8 * n)]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batches", default="1,11,64")
    ap.add_argument("--iterations", type=int, default=6)
    args = ap.parse_args()
    batches = [int(b) for b in args.batches.split(",")]
    its = args.iterations
    ctx = Context(0)
    n = max(batches)
    tex = LT.base_texture()
    jobs, frames, wins = [], [], []
    for j in range(n):
        job, fr = LT.window(900 + j, tex)
        win = L.KeyframeWindow(ctx, LT.W, LT.H, LT.N_FRAMES)
        for fid, img in zip(job["frame_ids"], fr):
            win.put_host(int(fid), img)
        extra = ST.solve_extras(7000 + j)
        extra.pop("delta_x")
        hes = HT.extras(5000 + j)
        hes.pop("delta", None)
        jobs.append(dict(step_job(job, 8000 + j), window=win, **hes, **extra)), frames.append(fr), wins.append(win)
    params = L.default_params()
    # the device form against the host form before anything is timed, every output asked for; the completed jobs of the old route
    check_dev, check_host = SP.StepBatch(jobs), SP.StepBatch(jobs)
    check_dev.run(ctx, params)
    for j in range(n):
        check_host.run_host(LT.W, LT.H, j, frames[j], params)
    dev = check_dev.results()
    bit_equal, active = True, []
    for j, (d, h) in enumerate(zip(dev, check_host.results())):
        if d["flags"] or not np.array_equal(d["new_state"], h["new_state"]) or not np.allclose(d["x"], h["x"], rtol=1e-6, atol=1e-9):
            raise SystemExit(f"window {j}: the device form and the host form disagree")
        bit_equal = bit_equal and all(np.asarray(d[k]).tobytes() == np.asarray(h[k]).tobytes() for k in d)
        active.append(float(np.mean(d["active"])))
    completed = []
    for job, d in zip(jobs, dev):
        c = {k: v for k, v in job.items() if k not in ("world_to_cam_eval", "state_zero", "state_backup", "frame_step", "calib_zero", "calib_backup",
                                                        "calib_step", "idepth_backup", "idepth_step", "exposure", "stepfac", "state_prior", "state_prior_zero")}
        c.update({k: d[k] for k, _ in L.PRE})
        c.update(cam=d["cam"][:4], cam_inv=d["cam"][4:], idepth_scaled=d["idepth"], idepth_zero_scaled=d["idepth"], delta_x=d["delta_x"],
                 H_L=d["H_L_step"], b_L=d["b_L_step"])
        completed.append(c)
    del check_dev, check_host
    new_call = {B: SP.StepBatch(jobs[:B], ()) for B in batches}
    old_solve = {B: SV.SolveBatch(completed[:B], ()) for B in batches}
    old_lin = {B: L.LinearizeBatch(completed[:B], ()) for B in batches}
    res_keys = ("point", "target", "state_in", "energy_in", "is_new")
    bare = lambda job: dict(job, **{k: np.asarray(job[k])[:0] for k in res_keys})  # noqa: E731
    host_step, host_solve = SP.StepBatch([bare(j) for j in jobs], ()), SV.SolveBatch([bare(c) for c in completed], ())
    for _ in range(args.warmup):
        for B in batches:
            new_call[B].run(ctx, params), old_solve[B].run(ctx, params), old_lin[B].run(ctx, params)
    keys = ("new_route", "old_device", "host_apply")
    t = {(B, k): [] for B in batches for k in keys}
    for _ in range(args.reps):
        for B in batches:
            t[(B, "new_route")].append(LT.timed(lambda: [new_call[B].run(ctx, params) for _ in range(its)]))
            t[(B, "old_device")].append(LT.timed(lambda: [(old_solve[B].run(ctx, params), old_lin[B].run(ctx, params)) for _ in range(its)]))
            hs = LT.timed(lambda: [host_step.run_host(LT.W, LT.H, j, frames[j], params) for j in range(B)])
            hv = LT.timed(lambda: [host_solve.run_host(LT.W, LT.H, j, frames[j], params) for j in range(B)])
            t[(B, "host_apply")].append((hs - hv) * its)
    out = {"tool": "step_timing", "reps": args.reps, "iterations": its, "geometry": [LT.W, LT.H], "frames": LT.N_FRAMES,
           "points_per_window": LT.N_PTS, "residuals_per_window": LT.N_PTS * (LT.N_FRAMES - 1), "active_share": round(float(np.mean(active)), 4),
           "device_equals_host_bit_for_bit": bool(bit_equal), "per_batch": {}}
    for B in batches:
        m = {k: float(np.median(t[(B, k)])) for k in keys}
        route = m["old_device"] + m["host_apply"]
        out["per_batch"][f"B={B}"] = {
            "new_route_ms_per_window_and_iteration": round(m["new_route"] / B / its, 4),
            "old_route_ms_per_window_and_iteration": round(route / B / its, 4),
            "old_route_device_ms_per_window_and_iteration": round(m["old_device"] / B / its, 4),
            "old_route_host_apply_ms_per_window_and_iteration": round(m["host_apply"] / B / its, 4),
            "new_route_over_old_route": round(m["new_route"] / route, 3)}
    for w in wins:
        w.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
