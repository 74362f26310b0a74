#!/usr/bin/env python3
"""The whole loop of the window optimisation, six iterations, all accepted (force_accept = 1, min_iterations = max_iterations = 6: both
routes run exactly 7 passes), on the device: ms per window and pass for 1 / 11 / 64 windows of the workload of tools/linearize_timing.py
(KITTI-shaped, 1232 x 368, 8 keyframes, 2 000 points, 14 000 residuals), whole synchronous calls timed.  In the same run, on the same
inputs:
  (a) one_call    ONE dsm_window_optimize_batch: one staged copy, the passes back to back, the decision and the commits on the device
  (b) step_calls  the route before: 7 dsm_window_step_batch calls (every optional output NULL), after each the commit on the host --
                  the returned state, depths, residual states and x copied into the next call's inputs, in place, by numpy -- and the
                  accept test; B1 and B2 come with the call (linearize_job_summary on the host)
After a warm-up the routes run in alternation; each figure is the median over the repetitions of a host clock.  The results of the two
routes are compared bit for bit before anything is timed.  (c) prices a finished job: route (a) at the largest batch with ONE job of
max_iterations = 2 among the others of 6 (it is frozen for four passes: its kernels recompute the same bytes).  Prints one JSON line.

  python tools/optimize_timing.py [--reps 9] [--batches 1,11,64] [--iterations 6]
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
import step_timing as PT  # noqa: E402
from direct_stereo_slam_amd import linearize as L  # noqa: E402
from direct_stereo_slam_amd import optimize as OP  # noqa: E402
from direct_stereo_slam_amd import step as SP  # noqa: E402
from direct_stereo_slam_amd.tracker import Context  # noqa: E402

f32, f64 = np.float32, np.float64
LAMBDA, ACCEPT, FORCE_ACCEPT = 0.1, 0.25, True


class StepCalls:
    """route (b): one StepBatch whose input arrays are this object's, committed in place between the calls"""

    def __init__(self, jobs):
        self.first, self.own, self.jobs = [], [], []
        for job in jobs:
            n, m = len(job["frame_ids"]), len(job["host"])
            own = dict(state_backup=np.array(job["state_backup"], f64).reshape(-1), calib_backup=np.array(job["calib_backup"], f64).reshape(-1),
                       idepth_backup=np.array(job["idepth_backup"], f32).reshape(-1), frame_step=np.zeros(8 * n), calib_step=np.zeros(4),
                       idepth_step=np.zeros(m, f32), state_in=np.array(job["state_in"], np.uint8).reshape(-1),
                       energy_in=np.array(job["energy_in"], f32).reshape(-1), frame_energy_th=np.array(job["frame_energy_th"], f32).reshape(-1))
            self.own.append(own), self.first.append({k: v.copy() for k, v in own.items()})
            self.jobs.append(dict(job, stepfac=np.zeros(5, f32), **own))
        self.batch = SP.StepBatch(self.jobs, ())
        self.outs = self.batch.all_outputs()
        self.lam, self.accepted = LAMBDA, []

    def reset(self):
        for own, first in zip(self.own, self.first):
            for k, v in first.items():
                own[k][:] = v

    def one_pass(self, ctx, params, fac, lam):
        for j in range(self.batch.n):
            S = self.batch.arr[j]
            for k in range(5):
                S.stepfac[k] = fac
            S.sol.lambda_ = lam
        self.batch.run(ctx, params)
        total = []
        for own, out in zip(self.own, self.outs):  # WindowStep::accept(), and setNewFrameEnergyTH
            m = len(own["idepth_backup"])
            own["state_backup"][:] = out["state"].reshape(-1)
            own["calib_backup"][:] = out["calib"]
            own["idepth_backup"][:] = out["idepth"][:m]
            own["frame_step"][:] = -out["x"][4:]
            own["calib_step"][:] = -out["x"][:4]
            own["idepth_step"][:] = out["step"][:m]
            nr = len(own["state_in"])
            own["state_in"][:] = out["new_state"][:nr]
            own["energy_in"][:] = out["new_energy"][:nr]
            own["frame_energy_th"][-1] = out["new_frame_energy_th"][0]
            total.append(float(out["energy"][0]) + float(out["energy_m"][0]))
        return total

    def run(self, ctx, params, its):
        lam = LAMBDA
        last = self.one_pass(ctx, params, 0.0, lam)
        for _ in range(its):
            new = self.one_pass(ctx, params, 1.0, lam * ACCEPT)
            self.accepted = [FORCE_ACCEPT or a < b for a, b in zip(new, last)]  # :427-429, per window; every window commits here
            last, lam = new, lam * ACCEPT
        self.lam = lam


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
    jobs, wins = [], []
    for j in range(n):
        job, fr = LT.window(900 + j, tex)
        win = L.KeyframeWindow(ctx, LT.W, LT.H, LT.N_FRAMES)
        for fid, img in zip(job["frame_ids"], fr):
            win.put_host(int(fid), img)
        extra = ST.solve_extras(7000 + j)
        extra.pop("delta_x")
        hes = HT.extras(5000 + j)
        hes.pop("delta", None)
        step = PT.step_job(job, 8000 + j)
        jobs.append(dict(step, window=win, fix_linearization=0, **hes, **extra)), wins.append(win)
    params = L.default_params()
    op = OP.default_optimize_params(force_accept=1, min_iterations=its)
    as_optimize = lambda job, m: dict(job, frame_step=None, calib_step=None, idepth_step=None, max_iterations=m)  # noqa: E731

    # the two routes against each other before anything is timed
    check_a, check_b = OP.OptimizeBatch([as_optimize(job, its) for job in jobs], ()), StepCalls(jobs)
    check_a.run(ctx, params, optimize_params=op)
    check_b.run(ctx, params, its)
    equal = True
    for a, own, out in zip(check_a.results(), check_b.own, check_b.outs):
        if a["n_passes"] != 1 + its or a["pattern"] != "A" * its:
            raise SystemExit("the one call did not run 1 + iterations passes")
        m, nr = len(own["idepth_backup"]), len(own["state_in"])
        pairs = [(a["state"], out["state"]), (a["calib"], out["calib"]), (a["idepth"], out["idepth"][:m]), (a["x"], out["x"]), (a["step"], out["step"][:m]),
                 (a["new_state"], out["new_state"][:nr]), (a["new_energy"], out["new_energy"][:nr]), (a["pass_energy"][-1][0], out["energy"][0]),
                 (a["pass_energy"][-1][1], out["energy_m"][0]), (a["frame_energy_th_out"], out["new_frame_energy_th"][0]), (a["lambda_out"], f64(check_b.lam))]
        equal = equal and all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in pairs)
    if not equal:
        raise SystemExit("the one call and the loop of step calls disagree")
    del check_a, check_b

    one_call = {B: OP.OptimizeBatch([as_optimize(job, its) for job in jobs[:B]], ()) for B in batches}
    step_calls = {B: StepCalls(jobs[:B]) for B in batches}
    big = max(batches)
    mixed = OP.OptimizeBatch([as_optimize(job, min(2, its) if j == 0 else its) for j, job in enumerate(jobs[:big])], ())
    for _ in range(args.warmup):
        for B in batches:
            one_call[B].run(ctx, params, optimize_params=op)
            step_calls[B].reset(), step_calls[B].run(ctx, params, its)
        mixed.run(ctx, params, optimize_params=op)
    t = {(B, k): [] for B in batches for k in ("one_call", "step_calls")}
    t_mixed = []
    for _ in range(args.reps):
        for B in batches:
            t[(B, "one_call")].append(LT.timed(lambda: one_call[B].run(ctx, params, optimize_params=op)))
            step_calls[B].reset()
            t[(B, "step_calls")].append(LT.timed(lambda: step_calls[B].run(ctx, params, its)))
        t_mixed.append(LT.timed(lambda: mixed.run(ctx, params, optimize_params=op)))
    passes = 1 + its
    out = {"tool": "optimize_timing", "reps": args.reps, "iterations": its, "passes": passes, "geometry": [LT.W, LT.H], "frames": LT.N_FRAMES,
           "points_per_window": LT.N_PTS, "residuals_per_window": LT.N_PTS * (LT.N_FRAMES - 1), "routes_equal_bit_for_bit": bool(equal), "per_batch": {}}
    for B in batches:
        a, b = float(np.median(t[(B, "one_call")])), float(np.median(t[(B, "step_calls")]))
        out["per_batch"][f"B={B}"] = {"one_call_ms_per_window_and_pass": round(a / B / passes, 4), "step_calls_ms_per_window_and_pass": round(b / B / passes, 4),
                                      "one_call_ms": round(a, 3), "step_calls_ms": round(b, 3), "one_call_over_step_calls": round(a / b, 3)}
    full = float(np.median(t[(big, "one_call")]))
    out["one_job_finished_after_2_iterations"] = {"windows": big, "one_call_ms": round(float(np.median(t_mixed)), 3),
                                                  "over_all_unfinished": round(float(np.median(t_mixed)) / full, 3)}
    for w in wins:
        w.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
