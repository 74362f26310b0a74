"""The checker of the window optimisation's accept / reject loop: the loop of tests/test_step_demo.py's
optimize_ref layered on _step_ref.run (imported, not edited), with dsm_optimize_params' fields.  Doubles are Python floats, floats numpy
float32 scalars, the heuristic's sums loops in ascending index, `exp` the C library's."""
import math

import numpy as np

import _step_ref as T

f32, f64 = np.float32, np.float64
OP = dict(lambda_init=0.1, lambda_accept_fac=0.25, lambda_reject_fac=100.0, fixed_lambda=-1.0, min_iterations=1, force_accept=0, step_momentum=0)
LOG = ("n_iterations", "n_passes", "pattern", "pass_energy", "pass_lambda", "iter_stepsize", "iter_can_break", "last_energy", "lambda_out",
       "frame_energy_th_out")
SCENES = ("scene", "nine_frames", "two_frames", "three_frames", "sixteen_frames", "no_priors", "no_h_m", "one_frame", "three_frames_no_residuals",
          "no_points")


def window_job(job):
    """a step scene's job as the optimize call takes it: at its current state, without the three steps"""
    return dict(job, frame_step=None, calib_step=None, idepth_step=None, fix_linearization=0)


def heuristic(prev_x, stepsize, x):
    """O4 (:390-405): (the new step size, a float32; incDirChange)"""
    dot = pp = xx = 0.0
    with np.errstate(all="ignore"):
        for a, b in zip(prev_x, x):
            a, b = float(a), float(b)
            dot += a * b
            pp += a * a
            xx += b * b
        den = 1e-20 + math.sqrt(pp) * math.sqrt(xx) if not (math.isnan(pp) or math.isnan(xx)) else math.nan
        inc = (1e-20 + dot) / den if den != 0.0 else math.nan
        if math.isfinite(inc):
            fresh = f32(math.exp(inc * 1.4))
            if inc < 0 and stepsize > 1:
                stepsize = f32(1.0)
            stepsize = np.sqrt(np.sqrt(f32(f32(f32(fresh * stepsize) * stepsize) * stepsize)))
            stepsize = f32(min(max(stepsize, f32(0.25)), f32(2.0)))
    return f32(stepsize), inc


def run(job, frames, max_iterations, op=None, stepsizes=None, sp=None, params=None, pass_fn=None):
    """The loop.  pass_fn: what runs a pass in place of _step_ref.run (a step job as a dict -> its result dict), for a host-driven loop
    over another form of the step call.  stepsizes: an override list, one factor per iteration, in place of the heuristic's (a device
    comparison under step_momentum starts from the device's own values).  Returns the last pass's _step_ref.run result with the log on top (LOG; pattern a
    str, pass_energy (n_passes, 2), margins: |E + E_M - last| of every decision) and `committed`: state_backup, calib_backup,
    idepth_backup, state_in, energy_in, frame_energy_th as a following call would take them."""
    op = dict(OP, **(op or {}))
    n = len(job["frame_ids"])
    cur = dict(job, fix_linearization=0, frame_step=np.zeros((n, 8)), calib_step=np.zeros(4), idepth_step=np.zeros(len(job["host"]), f32),
               frame_energy_th=np.array(job["frame_energy_th"], f32, copy=True))
    log = dict(pass_energy=[], pass_lambda=[], iter_stepsize=[], iter_can_break=[], margins=[])
    fixed = float(op["fixed_lambda"])

    def call(fac, lam):
        # a pass is a pure function of its inputs: runs that share a prefix (other iteration counts, other breaks) share its passes
        used = fixed if fixed >= 0.0 else lam
        if pass_fn is not None:
            res = pass_fn(dict(cur, stepfac=np.array([fac] * 5, f32), **{"lambda": used}))
        else:
            key = (id(frames), id(job["point"]), fac, used, repr(sp), repr(params)) + tuple(
                np.asarray(cur[k]).tobytes() for k in ("state_backup", "calib_backup", "idepth_backup", "state_in", "energy_in", "frame_step",
                                                       "calib_step", "idepth_step", "frame_energy_th"))
            if key not in _passes:
                _passes[key] = T.run(dict(cur, stepfac=np.array([fac] * 5, f32), **{"lambda": used}), frames, sp=sp, params=params)
            res = _passes[key]
        cur["frame_energy_th"] = cur["frame_energy_th"].copy()
        cur["frame_energy_th"][-1] = res["new_frame_energy_th"]
        log["pass_energy"].append((float(res["energy"]), float(res["energy_m"])))
        log["pass_lambda"].append(lam)
        return res

    def commit(res):
        cur.update(state_backup=res["state"], calib_backup=res["calib"], idepth_backup=res["idepth"], state_in=res["new_state"],
                   energy_in=res["new_energy"], frame_step=-res["x"][4:].reshape(n, 8), calib_step=-res["x"][:4], idepth_step=res["step"])
        return (float(res["energy"]), float(res["energy_m"]))

    lam, pattern, stepsize = float(op["lambda_init"]), "", f32(1.0)
    prev_x = [math.nan] * (4 + 8 * n)
    final = call(0.0, lam)
    last = commit(final)
    for it in range(max_iterations):
        x = [float(v) for v in final["x"]]
        if op["step_momentum"]:
            stepsize, _ = heuristic(prev_x, stepsize, x)
        prev_x = x
        if stepsizes is not None:
            stepsize = f32(stepsizes[it])
        log["iter_stepsize"].append(stepsize)
        trial_lam = lam * float(op["lambda_accept_fac"])
        res = call(float(stepsize), trial_lam)
        e = float(res["energy"]) + float(res["energy_m"])
        log["margins"].append(abs(e - (last[0] + last[1])))
        log["iter_can_break"].append(int(res["can_break"]))
        if op["force_accept"] or e < last[0] + last[1]:
            final, lam, pattern = res, trial_lam, pattern + "A"
        else:
            lam *= float(op["lambda_reject_fac"])
            final, pattern = call(0.0, lam), pattern + "R"
        last = commit(final)
        if res["can_break"] and it >= op["min_iterations"]:
            break
    out = dict(final)
    out.update(n_iterations=len(pattern), n_passes=len(log["pass_lambda"]), pattern=pattern, pass_energy=np.array(log["pass_energy"], f64).reshape(-1, 2),
               pass_lambda=np.array(log["pass_lambda"], f64), iter_stepsize=np.array(log["iter_stepsize"], f32),
               iter_can_break=np.array(log["iter_can_break"], np.uint8), last_energy=np.array(last, f64), lambda_out=f64(lam),
               frame_energy_th_out=f32(final["new_frame_energy_th"]), margins=log["margins"],
               committed={k: cur[k] for k in ("state_backup", "calib_backup", "idepth_backup", "state_in", "energy_in", "frame_energy_th")})
    return out


_cache, _passes = {}, {}


def expected(name, max_iterations=6, **op):
    """(window job, frames, the checker's result) of a _step_ref scene, computed once"""
    key = (name, max_iterations, tuple(sorted(op.items())))
    if key not in _cache:
        job, frames = T.scene(name)
        _cache[key] = (window_job(job), frames, run(job, frames, max_iterations, op))
    return _cache[key]


def assert_log_equal(got, exp):
    """every log entry bit for bit"""
    assert got["n_iterations"] == exp["n_iterations"] and got["n_passes"] == exp["n_passes"], (got["n_iterations"], got["n_passes"], exp["pattern"])
    assert got["pattern"] == exp["pattern"], (got["pattern"], exp["pattern"])
    for k, dtype in (("pass_energy", f64), ("pass_lambda", f64), ("iter_stepsize", f32), ("last_energy", f64), ("lambda_out", f64),
                     ("frame_energy_th_out", f32)):
        a, b = np.asarray(got[k], dtype).reshape(-1), np.asarray(exp[k], dtype).reshape(-1)
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), (k, a, b)
    assert list(got["iter_can_break"]) == list(exp["iter_can_break"]), (got["iter_can_break"], exp["iter_can_break"])
