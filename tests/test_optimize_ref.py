"""CPU: the checker of the window optimisation's accept / reject loop (tests/_optimize_ref.py) covers the ground
the device tests rely on, asserted on its output alone; and the host form dsm_window_optimize_host equals it bit for bit on every
output and log entry (both use the same C library, the heuristic's exp included)."""
import numpy as np
import pytest

import _linearize_ref as R
import _optimize_ref as O
import _solve_ref as SR
import _step_ref as T
from direct_stereo_slam_amd import optimize as S
from direct_stereo_slam_amd._lib import DsmError

f32, f64 = np.float32, np.float64
HES_OUT = SR.HR.RAW + ("active", "JpJdF") + SR.HR.PER_POINT
# struct defaults, max_iterations = 6: the pattern, and the iterations run
PATTERNS = dict(scene="RAARAA", nine_frames="RARAAR", two_frames="AAARAR", three_frames="AAARAA", sixteen_frames="RAAAAA", no_priors="RAARAA",
                no_h_m="RARRA", one_frame="RR", three_frames_no_residuals="AARARR", no_points="ARARAA")
WITH_RESIDUALS = ("scene", "nine_frames", "two_frames", "three_frames", "sixteen_frames", "no_priors", "no_h_m")


def host(job, frames, max_iterations, **op):
    got = S.window_optimize_host(R.W, R.H, dict(job, max_iterations=max_iterations), frames, optimize_params=S.default_optimize_params(**op))
    return dict(got, H_L=got["H_L_step"], b_L=got["b_L_step"])


def assert_equal(got, exp, max_iterations):
    """every embedded output (the job's last pass) and every log entry, bit for bit; zeros behind the entries written"""
    T.assert_step_equal(got, exp)
    SR.assert_equal(got, exp, hes_outputs=HES_OUT)
    O.assert_log_equal(got, exp)
    raw, ni, npass = got["raw"], exp["n_iterations"], exp["n_passes"]
    assert not raw["pass_energy"][npass:].any() and not raw["pass_lambda"][npass:].any()
    if max_iterations:
        assert not raw["pattern"][ni:].any() and not raw["iter_stepsize"][ni:].any() and not raw["iter_can_break"][ni:].any()


# ---- the ground, on the checker's output alone --------------------------------------------------------------------------------------

def test_checker_patterns_breaks_and_margins():
    """With the struct defaults and six iterations every scene with residuals accepts and rejects; two scenes break early, at different
    iterations; and no decision of a scene with residuals is closer than 100 x n_res x 2^-22 x 20000 (tests/test_step_demo.py's bound on
    what the device's sincos and exp may move an energy by): a device run takes the same decisions."""
    early = {}
    for name, pattern in PATTERNS.items():
        job, _, exp = O.expected(name)
        assert exp["pattern"] == pattern, (name, exp["pattern"])
        assert exp["n_passes"] == 1 + len(pattern) + pattern.count("R")
        if len(pattern) < 6:
            assert exp["iter_can_break"][-1] == 1
            early[name] = len(pattern) - 1
        if name in WITH_RESIDUALS:
            n_res = len(job["point"])
            assert n_res > 0 and "A" in pattern and "R" in pattern
            bound = n_res * 2.0 ** -22 * 2500.0 * 8
            ratio = min(exp["margins"]) / bound
            print(f"{name}: {pattern}, smallest margin {min(exp['margins']):.4g}, {ratio:.0f} x the bound")
            assert ratio >= 100.0, (name, min(exp["margins"]), bound)
        else:
            assert len(job["point"]) == 0
    assert early == dict(no_h_m=4, one_frame=1)


def test_checker_force_accept_and_fixed_lambda():
    """force_accept gives all 'A'; fixed_lambda changes x but not the logged schedule of the same decisions"""
    for name in ("scene", "two_frames"):
        assert O.expected(name, force_accept=1)[2]["pattern"] == "AAAAAA"
    job, frames = T.scene("scene")
    free, fixed = O.run(job, frames, 0), O.run(job, frames, 0, dict(fixed_lambda=1e-5))
    assert free["x"].tobytes() != fixed["x"].tobytes() and free["pass_lambda"].tobytes() == fixed["pass_lambda"].tobytes()
    a, b = O.expected("scene", force_accept=1)[2], O.expected("scene", force_accept=1, fixed_lambda=1e-5)[2]
    assert a["pass_lambda"].tobytes() == b["pass_lambda"].tobytes() and a["x"].tobytes() != b["x"].tobytes()
    assert list(a["pass_lambda"]) == [0.1 * 0.25 ** k for k in range(7)]


def test_checker_step_momentum_moves_the_step_size():
    moved = []
    for name in ("scene", "two_frames", "nine_frames"):
        exp = O.expected(name, step_momentum=1)[2]
        assert exp["iter_stepsize"][0] == 1.0  # previousX starts as NaN
        moved.append(bool((exp["iter_stepsize"] != 1.0).any()))
    assert any(moved)


# ---- the host form -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", O.SCENES)
def test_host_form_equals_the_checker_bit_for_bit(built, name):
    job, frames = T.scene(name)
    wjob = O.window_job(job)
    for max_iterations in (0, 1, 6, 20):
        for min_iterations in (0, 3) if max_iterations == 6 else (1,):
            exp = O.run(job, frames, max_iterations, dict(min_iterations=min_iterations))
            assert_equal(host(wjob, frames, max_iterations, min_iterations=min_iterations), exp, max_iterations)
    exp = O.expected(name)[2]
    assert_equal(host(wjob, frames, 6), exp, 6)


@pytest.mark.parametrize("name", ["scene", "two_frames", "nine_frames", "one_frame", "no_points"])
def test_host_form_step_momentum_force_accept_and_fixed_lambda(built, name):
    job, frames = T.scene(name)
    wjob = O.window_job(job)
    for op in (dict(step_momentum=1), dict(force_accept=1, fixed_lambda=1e-5), dict(step_momentum=1, force_accept=1)):
        assert_equal(host(wjob, frames, 6, **op), O.expected(name, **op)[2], 6)


def test_host_form_leaves_the_inputs_alone_and_a_second_call_continues(built):
    """the call is stateless: the committed state it returns, passed as the next call's current state, continues the loop"""
    job, frames, exp = O.expected("three_frames")
    c = exp["committed"]
    nxt = dict(job, **c)
    got = host(nxt, frames, 2)
    ref = O.run(dict(T.scene("three_frames")[0], **c), frames, 2)
    assert_equal(got, ref, 2)
    assert got["state"].tobytes() != exp["state"].tobytes()


def invalid_cases(job):
    n, m = len(job["frame_ids"]), len(job["host"])
    bad = [("frame_step given", dict(job, frame_step=np.zeros((n, 8))), {}), ("calib_step given", dict(job, calib_step=np.zeros(4)), {}),
           ("idepth_step given", dict(job, idepth_step=np.zeros(m, f32)), {}),
           ("max_iterations -1", dict(job, max_iterations=-1), {}), ("max_iterations 21", dict(job, max_iterations=21), {}),
           ("no state_backup", dict(job, state_backup=None), {}), ("no H_L", dict(job, H_L=None), {}),
           ("pre_KtTll given", dict(job, pre_KtTll=np.zeros((n, n, 3), f32)), {}),
           ("state_backup NaN", dict(job, state_backup=np.full((n, 8), np.nan)), {})]
    bad += [(f"no {k}", job, dict(omit=(k,))) for k in S.LOG]
    return bad


INVALID_PARAMS = (dict(lambda_init=np.nan), dict(lambda_init=-1.0), dict(lambda_accept_fac=0.0), dict(lambda_reject_fac=-2.0),
                  dict(lambda_reject_fac=np.inf), dict(fixed_lambda=np.nan), dict(min_iterations=-1))


def test_host_form_refuses_all_or_nothing(built):
    job, frames = T.scene("three_frames")
    wjob = dict(O.window_job(job), max_iterations=3)
    cases = [(what, bad, kw, {}) for what, bad, kw in invalid_cases(wjob)] + [(str(p), wjob, {}, p) for p in INVALID_PARAMS]
    for what, bad, kw, op in cases:
        b = S.OptimizeBatch([bad], **kw)
        before = {k: v.copy() for k, v in b.all_outputs()[0].items()}
        with pytest.raises(DsmError):
            b.run_host(R.W, R.H, 0, frames, optimize_params=S.default_optimize_params(**op))
        for k, v in b.all_outputs()[0].items():
            assert v.tobytes() == before[k].tobytes(), (what, k)
