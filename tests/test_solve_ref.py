"""CPU: dsm_window_solve_host equals the checker tests/_solve_ref.py bit for bit on every output (DESIGN.md section 18, F1-F8, R1-R3,
V); and, independently of the stated order: the checker's LDLT is the oracle's orc_ldlt_solve on 8 x 8 systems; the residual of the
damped system, evaluated exactly, lies within the backward-error bound of the factorisation plus what section 17's own bound allows
for the stitched matrices; the projected x has no share of the null basis; and every point's step agrees with a float64 evaluation
of R1-R2.  Each bound is broken by the mutations named beside it."""
import math
from fractions import Fraction

import numpy as np
import pytest

import _hessian_ref as HR
import _linearize_ref as R
import _solve_ref as SR

U = 2.0 ** -53


def host_form(job, frames, **kw):
    from direct_stereo_slam_amd import solve

    return solve.window_solve_host(R.W, R.H, job, frames, **kw)


HES_OUT = HR.RAW + ("active", "JpJdF") + HR.PER_POINT


@pytest.mark.parametrize("name", SR.NAMES)
def test_host_form_equals_checker(name):
    job, frames, exp = SR.case(name)
    got = host_form(job, frames)
    SR.assert_equal(got, exp, hes_outputs=HES_OUT)
    assert got["flags"] == 0 and np.isfinite(got["x"]).all()
    if len(job["point"]) == 0:
        assert not got["step"].any()


VARIANTS = [dict(lam=lam) for lam in SR.LAMBDAS] + [dict(priors=False), dict(n_null=1), dict(n_null=7), dict(shift=0), dict(shift=1),
                                                    dict(lam=10.0, priors=False, n_null=7, shift=0)]


@pytest.mark.parametrize("name", ["scene", "two_frames"])
@pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: "-".join(f"{k}{x}" for k, x in v.items()))
def test_host_form_variants(name, variant):
    """every lambda, priors NULL and given, n_null 0 / 1 / 7, shift_prior_to_zero on and off"""
    job, frames, exp = SR.case(name, **variant)
    SR.assert_equal(host_form(job, frames), exp, hes_outputs=HES_OUT)


def test_points_with_no_one_and_every_possible_active_residual():
    """three frames: points with 0, 1 and n - 1 = 2 active residuals; the first have a zero step, the others do not"""
    job, frames, exp = SR.frames_case(3)
    per_point = np.bincount(np.asarray(job["point"])[exp["active"].astype(bool)], minlength=len(job["host"]))
    assert all((per_point == k).sum() >= 3 for k in (0, 1, 2)), np.bincount(per_point)
    got = host_form(job, frames)
    SR.assert_equal(got, exp, hes_outputs=HES_OUT)
    assert all(got["step"][per_point == k].any() == (k > 0) for k in (0, 1, 2))


def test_the_variants_differ():
    xs = [SR.case("scene", **v)[2]["x"].tobytes() for v in VARIANTS]
    assert len(set(xs)) == len(xs) - 1  # lam=1e-5 and shift=1 are both the default job (scene has the shift on)
    assert SR.case("scene")[2]["step"].any() and SR.case("scene", n_null=7)[2]["x0"].tobytes() != SR.case("scene", n_null=7)[2]["x"].tobytes()


def test_host_form_optional_outputs():
    """every optional output NULL: x, step and flags alone; then a few given"""
    job, frames, exp = SR.case("scene")
    got = host_form(job, frames, outputs=())
    SR.assert_equal(got, exp, outputs=("x", "step", "flags"))
    assert all((np.asarray(got[k]) == -7).all() for k in HR.STITCHED + ("last_HS", "last_bS") + HR.RAW)
    got = host_form(job, frames, outputs=("H_sc", "last_bS", "hdi"))
    SR.assert_equal(got, exp, outputs=("x", "step", "flags", "H_sc", "last_bS", "hdi"))
    assert (got["H_A"] == -7).all() and (got["last_HS"] == -7).all() and (got["bd_sum"] == -7).all()


# ---- 1. the checker's LDLT against the oracle's, on 8 x 8 systems ----------------------------------------------------------------

def test_checker_ldlt_equals_the_oracle_on_8x8_systems():
    import ctypes as C

    from oracle import oracle as O

    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    rng = np.random.default_rng(8)
    systems = []
    for i in range(40):
        G = rng.normal(0, 1, (8, 8))
        A = G @ G.T * 10.0 ** rng.integers(-3, 4)
        if i % 4 == 1:
            A[np.diag_indices(8)] = np.repeat(rng.uniform(1, 9, 4), 2)  # tied pairs
        if i % 4 == 2:
            A = A - 3.0 * np.eye(8)  # indefinite
        if i % 8 == 3:
            A[:, 3] = A[3, :] = 0.0  # a zero pivot
        systems.append((A, rng.normal(0, 1, 8)))
    systems.append((np.zeros((8, 8)), np.ones(8)))
    systems.append((np.eye(8), np.arange(8.0)))
    for A, b in systems:
        A = np.ascontiguousarray(A)
        x = np.zeros(8)
        O.lib().orc_ldlt_solve(8, dp(A), dp(b), dp(x))
        assert SR.ldlt_solve(A, b)[0].tobytes() == x.tobytes()


# ---- 5. solver edges, through H_L on jobs without residuals ------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["equal_diagonal", "tied_groups", "all_zero", "zero_pivot", "negative_diagonal", "twelve"])
def test_solver_edges(name):
    job, frames, exp = SR.edge_cases()[name]
    got = host_form(job, frames)
    SR.assert_equal(got, exp)
    N = 4 + 8 * len(job["frame_ids"])
    assert len(got["x"]) == N
    if name == "all_zero":
        assert not got["x"].any() and got["flags"] == 0
    if name == "negative_diagonal":
        assert np.isnan(got["x"]).any() and got["flags"] == 1
    if name == "zero_pivot":
        A, tr = exp["factor"]
        assert (np.diag(A) == 0).sum() == 1 and got["flags"] == 0 and np.isfinite(got["x"]).all()
    if name in ("equal_diagonal", "tied_groups"):
        d = np.abs(np.diag(exp["HS"]))
        assert len(set(d.tolist())) < N and got["flags"] == 0
    if name == "twelve":
        assert N == 12 and np.abs(job["H_L"] @ got["x"] - job["b_L"]).max() < 1e-9 * np.abs(job["b_L"]).max() * np.linalg.cond(job["H_L"])


def test_tied_groups_follow_the_swaps_not_a_stable_order():
    """the pivot order of the tied case is not the one a stable sort of |diagonal| gives: the literal selection loop is needed"""
    job, frames, exp = SR.edge_cases()["tied_groups"]
    A, tr = exp["factor"]
    order = list(range(len(tr)))
    for k, t in enumerate(tr):
        order[k], order[t] = order[t], order[k]
    d = np.abs(np.diag(exp["HS"]))
    assert order != list(np.argsort(-d, kind="stable"))


# ---- 6. validation -----------------------------------------------------------------------------------------------------------------

def test_invalid_jobs_are_refused_before_any_output_is_written():
    from direct_stereo_slam_amd import solve
    from direct_stereo_slam_amd._lib import DsmError

    job, frames, exp = SR.case("scene")
    calls = [(what, bad, {}) for what, bad in SR.invalid_jobs(job) + HR.invalid_jobs(job)] + list(R.invalid_jobs(job))
    assert len(calls) == 17 + 23
    for what, bad, kw in calls:
        b = solve.SolveBatch([bad])
        before = [{k: v.copy() for k, v in out.items()} for out in b.all_outputs()]
        with pytest.raises(DsmError):
            b.run_host(R.W, R.H, 0, frames, solve.default_params(**kw))
        for out, bef in zip(b.all_outputs(), before):
            assert all(np.array_equal(out[k], bef[k]) for k in out), what
    for k in ("x", "step", "flags"):  # a NULL required output
        b = solve.SolveBatch([job])
        setattr(b.arr[0], k, None)
        with pytest.raises(DsmError):
            b.run_host(R.W, R.H, 0, frames)
        assert (b.outs[0][0]["last_HS"] == -7).all() and (b.hes.lin.outs[0][0]["new_state"] == 77).all(), k
    SR.assert_equal(host_form(job, frames), exp)


# ---- 2. the residual of the damped system, evaluated exactly ----------------------------------------------------------------------
# With u = 2^-53, gamma_k = k u / (1 - k u), lam1 = 1 + lambda, s = 1 / lam1 (exact here), D_ij = lam1 on the diagonal and 1 elsewhere:
#   the solve works on H^ = fl(HF_damped) and b^ = fl(bF) formed from the STITCHED matrices, scales them, HS_ij = v_i H^_ij v_j (1 + d)^2,
#   r_i = v_i b^_i (1 + d), solves (P HS P' + dA) P y = P r with |dA| <= gamma_(3N+1) |L||D||L'| (Higham, Accuracy and Stability,
#   Theorem 10.4 with 10.3, for the factorisation and the two substitutions of an LDL' without further pivoting), and returns
#   x0_i = v_i y_i (1 + d).  Dividing row i by v_i:
#     |b^ - H^ x0|_i <= gamma_(3N+2) (W (|x0| / v))_i / v_i + u |b^_i| + gamma_3 (|H^| |x0|)_i,        W = P' |L||D||L'| P
#   H^ and b^ differ from the dense float64 construction (HF, bF from _hessian_ref.dense and the priors, damped exactly) by the
#   roundings of F1-F4 and by what section 17's bound allows for the stitched matrices (e_k = magnitude_k (n_k + 1) 2^-24):
#     |H^ - H|_ij <= gamma_4 (D_ij (|H_L| + |H_M| + |H_A|) + s |H_sc|)_ij + D_ij e_HA_ij + s e_Hsc_ij
#     |b^ - b|_i  <= gamma_4 (|b_L| + |b_M| + |b_A| + |b_sc|)_i + gamma_(N+4) (|H_M| |delta_x|)_i + e_bA_i + e_bsc_i
#   so |b - H x0|_i <= the first line + (|H^ - H| |x0|)_i + |b^ - b|_i.  Nothing here is fitted.
def gamma(k):
    return k * U / (1 - k * U)


def residual_check(job, exp, sol):
    """the rows where the exact residual of the dense damped system exceeds the derived bound (empty: the bound holds)"""
    from test_hessian_ref import roundings

    nf = len(job["frame_ids"])
    N = 4 + 8 * nf
    value, mag = HR.dense(job, exp, job)
    e = {k: mag[k] * (n + 1) * 2.0 ** -24 for k, n in roundings(nf).items()}
    get = lambda k, shape: np.asarray(job[k], np.float64).reshape(shape) if job.get(k) is not None else np.zeros(shape)  # noqa: E731
    HL, bL, HM, bM, dx = get("H_L", (N, N)), get("b_L", N), get("H_M", (N, N)), get("b_M", N), get("delta_x", N)
    lam1 = Fraction(1) + Fraction(float(job["lambda"]))
    s = 1 / lam1
    F = np.vectorize(Fraction, otypes=[object])
    Dg = np.where(np.eye(N, dtype=bool), lam1, Fraction(1))
    H = (F(HL) + F(HM) + F(value["H_A"])) * Dg - F(value["H_sc"]) * s  # exact
    b = F(bL) + F(bM) + F(HM).dot(F(dx)) + F(value["b_A"]) - F(value["b_sc"])
    x0 = sol["x0"]
    res = np.array([float(abs(v)) for v in b - H.dot(F(x0))])
    A, tr = sol["factor"]
    L, d = np.tril(A, -1) + np.eye(N), np.diag(A)
    order = list(range(N))
    for k, t in enumerate(tr):
        order[k], order[t] = order[t], order[k]
    Wp = np.abs(L) @ np.diag(np.abs(d)) @ np.abs(L).T
    W = np.zeros((N, N))
    W[np.ix_(order, order)] = Wp  # P' |L||D||L'| P
    v, ax = sol["v"], np.abs(x0)
    lam1f, sf = float(lam1), float(s)
    Df = np.where(np.eye(N, dtype=bool), lam1f, 1.0)
    Hhat, bhat = np.abs(sol["HF_damped"]), np.abs(sol["bF"])
    bound = gamma(3 * N + 2) * (W @ (ax / v)) / v + U * bhat + gamma(3) * (Hhat @ ax)
    dH = gamma(4) * (Df * (np.abs(HL) + np.abs(HM) + np.abs(exp["H_A"])) + sf * np.abs(exp["H_sc"])) + Df * e["H_A"] + sf * e["H_sc"]
    db = gamma(4) * (np.abs(bL) + np.abs(bM) + np.abs(exp["b_A"]) + np.abs(exp["b_sc"])) + gamma(N + 4) * (np.abs(HM) @ np.abs(dx)) + e["b_A"] + e["b_sc"]
    bound = (bound + dH @ ax + db) * (1 + 1e-9)  # (the bound itself is evaluated in floating point)
    return np.flatnonzero(~(res <= bound)), res, bound


@pytest.mark.parametrize("name", ["scene", "nine_frames"])
def test_residual_of_the_damped_system_within_the_derived_bound(name):
    job, frames, exp = SR.case(name, lam=0.1)
    bad, res, bound = residual_check(job, exp, exp)
    assert len(bad) == 0, (bad, res[bad], bound[bad])
    assert np.isfinite(bound).all() and (bound < 1e-3 * np.abs(exp["bF"]).max()).all()


def test_the_residual_bound_has_teeth():
    """damping dropped, H_sc not scaled by s, b_sc added instead of subtracted, H_M delta_x dropped: each breaks it"""
    for name in ("scene", "nine_frames"):
        job, frames, exp = SR.case(name, lam=0.1)
        for drop in ("damping", "s", "b_sc_sign", "HM_dx"):
            bad, _, _ = residual_check(job, exp, SR.solve(job, exp, drop=(drop,)))
            assert len(bad) > 0, (name, drop)


# ---- 3. the projected x has no share of the null basis ----------------------------------------------------------------------------
# t^ = fl(Q' x): |t^ - Q' x| <= gamma_N |Q'| |x|;  c = fl(Q t^): |c - Q t^| <= gamma_n |Q| |t^|;  x' = fl(x - c): |x' - (x - c)| <= u (|x| + |c|).
# Exactly, Q' x' = (Q' x - t^) + (I - Q' Q) t^ - Q' (c - Q t^) + Q' (x' - (x - c)), so
#   |Q' x'|_k <= gamma_N (|Q'| |x|)_k + (|I - Q' Q| |t^|)_k + (|Q'| (gamma_n |Q| |t^| + u (|x| + (1 + gamma_n) |Q| |t^|)))_k
@pytest.mark.parametrize("nn", [1, 7])
def test_projection_leaves_nothing_along_the_null_basis(nn):
    job, frames, exp = SR.case("scene", n_null=nn)
    N = len(exp["x"])
    Q = np.asarray(job["null_basis"]).reshape(N, nn)
    assert np.array_equal(np.asarray(job["null_pinv"]).reshape(nn, N), Q.T)
    F = np.vectorize(Fraction, otypes=[object])
    FQ = F(Q)

    def share(x):
        return np.array([float(abs(v)) for v in FQ.T.dot(F(x))])

    x0, aQ = exp["x0"], np.abs(Q)
    t = SR.dsum_rows(Q.T, x0)
    gram = np.array([[float(abs(v)) for v in row] for row in (F(np.eye(nn)) - FQ.T.dot(FQ))])
    at = np.abs(t)
    bound = gamma(N) * (aQ.T @ np.abs(x0)) + gram @ at + aQ.T @ (gamma(nn) * (aQ @ at) + U * (np.abs(x0) + (1 + gamma(nn)) * (aQ @ at)))
    assert (share(exp["x"]) <= bound * (1 + 1e-9)).all(), (share(exp["x"]), bound)
    assert (share(x0) > 1e6 * bound).all()  # before F7 x does have a share: the bound has teeth


# ---- 4. every point's step against a float64 evaluation of R1-R2 --------------------------------------------------------------------
# float32 roundings along the deepest term, a residual's share of b (m: the most active residuals a point can have, n_frames - 1):
#   x and ad to float (2), their product (1), the 8 sums of R1's fsum (8), the sum of the two halves (1), the product with JpJdF (1),
#   the 8 sums of R2's fsum (8), the subtractions of b (1 for the Hcd term and m for the residuals), the product with hdi (1): 23 + m.
#   The Hcd term is shallower: Hcd = hcd_acc + hcd_lin (1), x to float (1), product (1), 4 sums, m + 1 subtractions, hdi (1).
def step_check(job, exp, x, step, drop_residual=None, swap=False, no_lin=False):
    """the points where `step` is further than the bound from the float64 evaluation (optionally a mutated one)"""
    nf, n = len(job["frame_ids"]), len(job["host"])
    host, point, target = (np.asarray(job[k]) for k in ("host", "point", "target"))
    adh, adt = (np.asarray(job[k], np.float64).reshape(nf, nf, 8, 8) for k in ("ad_host", "ad_target"))
    if swap:
        adh, adt = adt, adh
    x = np.asarray(x, np.float64)
    xf = [x[4 + 8 * f:12 + 8 * f] for f in range(nf)]
    hcd = exp["hcd_acc"].astype(np.float64) + (0.0 if no_lin else np.asarray(job["hcd_lin"], np.float64).reshape(n, 4))
    ref, mag = np.zeros(n), np.zeros(n)
    for p in range(n):
        rs = [r for r in np.flatnonzero(point == p) if exp["active"][r] and r != drop_residual]
        if not [r for r in np.flatnonzero(point == p) if exp["active"][r]]:
            continue
        b, m = float(exp["bd_sum"][p]) - x[:4] @ hcd[p], abs(float(exp["bd_sum"][p])) + np.abs(x[:4]) @ np.abs(hcd[p])
        h = host[p]
        for r in rs:
            t, jp = target[r], exp["JpJdF"][r].astype(np.float64)
            b -= (xf[h] @ adh[h, t] + xf[t] @ adt[h, t]) @ jp
            m += (np.abs(xf[h]) @ np.abs(adh[h, t]) + np.abs(xf[t]) @ np.abs(adt[h, t])) @ np.abs(jp)
        ref[p], mag[p] = -b * float(exp["hdi"][p]), m * float(exp["hdi"][p])
    bound = mag * (23 + (nf - 1) + 1) * 2.0 ** -24
    return np.flatnonzero(~(np.abs(step.astype(np.float64) - ref) <= bound)), ref, bound


@pytest.mark.parametrize("name", ["scene", "nine_frames", "wide"])
def test_steps_against_a_float64_evaluation(name):
    job, frames, exp = SR.case(name)
    bad, ref, bound = step_check(job, exp, exp["x"], exp["step"])
    assert len(bad) == 0, (bad[:5], exp["step"][bad][:5], ref[bad][:5], bound[bad][:5])
    assert (np.abs(ref) > 100 * bound).sum() > 20  # the steps are far larger than the bound


def test_the_step_bound_has_teeth():
    """a dropped residual, host and target swapped in xAd, Hcd without hcd_lin: each breaks it"""
    job, frames, exp = SR.case("scene")
    r = int(np.flatnonzero(exp["active"])[5])
    assert job["point"][r] in step_check(job, exp, exp["x"], exp["step"], drop_residual=r)[0]
    assert len(step_check(job, exp, exp["x"], exp["step"], swap=True)[0]) > 20
    assert len(step_check(job, exp, exp["x"], exp["step"], no_lin=True)[0]) > 5
