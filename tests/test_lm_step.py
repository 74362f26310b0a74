"""The LM step -- wave_ldlt_solve8, propose_pose (extrapolation, SCALE_*, the non-finite guard, the last / residual-only decision,
se3_exp_wave, se3_mul, make_eval_rot, the helper hand-off) and propose_scale -- run in isolation on constructed systems
(dsm_diag_lm_propose) against the host references of tests/_lm_step_ref.py.

  A  finite systems: the raw increment, inc_norm, aff_cand, residual_only, cutoff bit for bit the oracle's step, every matrix class x
     lambda x affine mode x spec x helper (GPU)
  B  the case set really takes the slow (tie / NaN) pivot path and the fast one, and a swapped tie-break changes the oracle's bits (CPU)
  C  the oracle's solve against the exact rational solve (CPU): with A this pins the device's solve as well
  D  non-finite systems: the raw increment the oracle's in every affine mode, a NaN compared as a NaN, and the step's route (GPU)
  E  the SE3 update over the small-angle branch, the cancellation band and angles past pi and 2 pi (GPU; the oracle's own error
     against mpmath is measured on the CPU)
  F  the scale step against a float32 restatement (GPU)
  G  argument errors (CPU: what can be reached without a device; GPU: the rest)
"""
import ctypes as C
import functools
import math
from fractions import Fraction

import numpy as np
import pytest

import _lm_step_ref as R
from _scenes import SIZES
from direct_stereo_slam_amd import synth as S
from oracle import oracle as O

LVL = 1            # maxIterations[1] = 20
SIZE = "mini4"     # the smallest pyramid the library accepts; the step reads the tracker's parameters and K^-1 only
CUR = np.array([0.1825741858350554, -0.3651483716701107, 0.5477225575051661, 0.7302967433402214, 0.3, -0.2, 1.5])
AFF = (0.03, 2.0)
DELTA = 4 * R.EPS  # the sincos difference between the device's and the host's libm that the SE3 bounds are derived from


def ref_params(mode_name, fixed=0):
    p = O.default_params()
    p.affine_opt_mode_a, p.affine_opt_mode_b = R.MODES[mode_name]
    p.fixed_schedule = fixed
    return p


def level_K():
    return S.level_K(S.kitti_K_work(), SIZES[SIZE][2])


# ---------------------------------------------------------------------------------------------------------------------------------
# device side
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trackers(ctx):
    from direct_stereo_slam_amd.tracker import TrackerAndScaler, default_params

    made = {}

    def get(mode_name, fixed=0):
        if (mode_name, fixed) not in made:
            rp, p = ref_params(mode_name, fixed), default_params()
            for f in ("huber_th", "coarse_cutoff_th", "scale_xi_rot", "scale_xi_trans", "scale_a", "scale_b", "affine_opt_mode_a",
                      "affine_opt_mode_b", "lambda_extrapolation_limit", "fixed_schedule"):
                setattr(p, f, getattr(rp, f))
            for i in range(6):
                p.max_iterations[i] = rp.max_iterations[i]
            w, h, _, nl = SIZES[SIZE]
            trk = TrackerAndScaler(ctx, w, h, nl, S.KITTI_T_STEREO, level_K(), p)
            trk.makeK(*level_K())
            made[(mode_name, fixed)] = trk
        return made[(mode_name, fixed)]

    yield get
    for t in made.values():
        t.close()


def pack(problems):
    """[dict(H, b, lam, cur, aff_cur, iteration, ...)] -> LM_PROPOSE_IN records"""
    from direct_stereo_slam_amd.tracker import LM_PROPOSE_IN

    arr = np.zeros(len(problems), LM_PROPOSE_IN)
    for a, p in zip(arr, problems):
        a["H"] = np.asarray(p.get("H", np.zeros(64)), np.float64).reshape(64)
        a["b"] = p.get("b", np.zeros(8))
        a["cur"] = p.get("cur", CUR)
        a["aff_cur"] = p.get("aff_cur", AFF)
        a["lam"] = p["lam"]
        a["level_cutoff_repeat"] = p.get("level_cutoff_repeat", 1.0)
        a["iteration"] = p.get("iteration", 0)
        a["Hs"], a["bs"], a["scale_cur"] = p.get("Hs", 0.0), p.get("bs", 0.0), p.get("scale_cur", 0.0)
    return arr


def f64_bits(x):
    return R.bits64(np.float64(x))


# ---------------------------------------------------------------------------------------------------------------------------------
# A  finite systems
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def finite_case_set():
    max_it = O.default_params().max_iterations[LVL]
    return tuple(dict(cls=c, H=H, b=b, lam=lam, iteration=it, level_cutoff_repeat=(1.0, 2.0, 8.0)[n % 3])
                 for n, (c, H, b, lam, it) in enumerate(R.finite_problems(max_it)))


@functools.lru_cache(maxsize=None)
def finite_reference(mode_name, spec):
    p = ref_params(mode_name)
    return tuple(R.step_oracle(p, 0, LVL, q["H"], q["b"], q["lam"], CUR, AFF, q["iteration"], q["level_cutoff_repeat"], spec=spec)
                 for q in finite_case_set())


@pytest.mark.gpu
@pytest.mark.parametrize("helper", (0, 1))
@pytest.mark.parametrize("spec", (0, 1))
@pytest.mark.parametrize("mode_name", list(R.MODES))
def test_finite_systems_bit_for_bit(trackers, mode_name, spec, helper):
    """Given bitwise equal H, b and lambda the device's raw increment is the checker's, bit for bit (uint64 patterns; no entry of the
    oracle's increments on this set is a NaN, so no NaN sign or payload enters the comparison), and with it inc_norm, aff_cand,
    residual_only (on both sides of inc_norm = 1e-3 and of the iteration bound, which is iteration + 2 for a speculative proposal),
    cutoff and max_energy.  The strict upper triangle of every H handed over holds a sentinel (a large number or NaN): only the lower
    triangle is the system, under `stitch` as well."""
    cases, ref = finite_case_set(), finite_reference(mode_name, bool(spec))
    assert len(cases) <= 4096
    assert not any(np.isnan(r["inc"]).any() for r in ref)
    assert {r["residual_only"] for r, q in zip(ref, cases) if q["iteration"] == 0} == {0, 1}  # inc_norm on both sides of 1e-3
    out = trackers(mode_name).diagLmPropose(0, LVL, pack(cases), spec=spec, helper=helper)
    bad = []
    for n, (q, r, o) in enumerate(zip(cases, ref, out)):
        for name, got, want in (("inc", R.bits64(o["inc"]), R.bits64(r["inc"])), ("inc_norm", f64_bits(o["inc_norm"]), f64_bits(r["inc_norm"])),
                                ("aff_cand", R.bits64(o["aff_cand"]), R.bits64(r["aff_cand"])),
                                ("cutoff", R.bits32(o["cutoff"]), R.bits32(r["cutoff"])),
                                ("max_energy", R.bits32(o["max_energy"]), R.bits32(r["max_energy"])),
                                ("residual_only", np.int64(o["residual_only"]), np.int64(r["residual_only"]))):
            if not np.array_equal(got, want):
                bad.append((n, q["cls"], q["lam"], q["iteration"], name, o[name], r[name]))
    assert not bad, (len(bad), bad[:6])
    if spec:  # the speculative bound is iteration + 2: at max_it - 2 the two kinds of proposal decide differently
        plain = finite_reference(mode_name, False)
        assert any(a["residual_only"] != b["residual_only"] for a, b in zip(plain, ref))


# ---------------------------------------------------------------------------------------------------------------------------------
# B  the slow path is really taken, and a wrong tie-break would show
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode_name", list(R.MODES))
def test_case_set_takes_both_pivot_paths(built, mode_name):
    p, cases = ref_params(mode_name), finite_case_set()
    slow = sum(R.takes_slow_path(p, q["H"], q["lam"]) for q in cases)
    assert 3 * slow >= len(cases) and 3 * (len(cases) - slow) >= len(cases), (slow, len(cases))


@pytest.mark.parametrize("mode_name", list(R.MODES))
def test_swapped_tie_break_changes_the_bits(built, mode_name):
    """py_ldlt_solve is orc_ldlt_solve bit for bit on the whole set; with the pivot search taking the LAST of equal maxima instead of the
    first it is not, on tie cases -- so test A can see a wrong tie-break."""
    p, cases, ref = ref_params(mode_name), finite_case_set(), finite_reference(mode_name, False)
    changed = 0
    for q, r in zip(cases, ref):
        assert R.same_bits(R.raw_increment(p, q["H"], q["b"], q["lam"], R.py_solve), r["inc"]), q["cls"]
        if not R.same_bits(R.raw_increment(p, q["H"], q["b"], q["lam"], R.py_solve_larger_index), r["inc"]):
            assert R.takes_slow_path(p, q["H"], q["lam"]), q["cls"]  # (without a tie the tie-break cannot matter)
            changed += 1
    print(f"\n{mode_name}: larger-index tie-break changes the increment's bits on {changed} of {len(cases)} problems")
    assert changed >= 1


# ---------------------------------------------------------------------------------------------------------------------------------
# C  the oracle's solve against the exact one
# ---------------------------------------------------------------------------------------------------------------------------------
C_BOUND_DEFINITE, C_BOUND_INDEFINITE = 11.3, 67.5  # four times the measured worst: see the test's docstring


def test_oracle_solve_against_exact_rational_solve(built):
    """For the finite, full-rank systems of A with condition number <= 1e8 (the damped matrices H + lambda diag H as the solve sees
    them, 8-dim): max |x - x_exact| / max |x_exact| of orc_ldlt_solve against the Fraction solve, in units of cond_2 * 2^-53.
    Device = oracle bit for bit (test A), so the bounds hold for wave_ldlt_solve8 as well.  Three groups, because LDLT with diagonal
    pivoting is an algorithm for semi-definite matrices (Eigen documents it so):
      definite (all eigenvalues of one sign; 180 systems): measured worst 2.81 (equal_diag, lambda 1e-4, cond 1.0); bound 4 x = 11.3.
      indefinite with a nonzero diagonal (81 systems): no a-priori bound exists (the element growth of diagonal pivoting is
        unbounded there); measured worst on this set 16.81 (indefinite, lambda 1e-4, cond 2.9); bound 4 x = 67.5.
      zero diagonal (9 systems, all non-singular): the first pivot is zero and Eigen's rule returns the zero vector, which is not the
        solution (relative error 1: 8.7e14 in these units); asserted as what it is -- an exactly zero increment."""
    worst, count = {}, {}
    for q in finite_case_set():
        A = R.lower_symmetric(q["H"])
        lam1 = float(R.F32(1) + R.F32(q["lam"]))
        for i in range(8):
            A[i, i] = A[i, i] * lam1
        if not np.all(np.isfinite(A)) or np.linalg.matrix_rank(A) < 8:
            continue
        cond = np.linalg.cond(A)
        if not cond <= 1e8:
            continue
        x = R.orc_ldlt(A, -q["b"])
        if not np.diag(A).any():
            assert not x.any(), q["cls"]
            count["zero diagonal"] = count.get("zero diagonal", 0) + 1
            continue
        xe = R.solve_exact(A, -q["b"])
        scale = max(abs(v) for v in xe)
        assert scale > 0
        ev = np.linalg.eigvalsh(A)
        group = "definite" if (ev > 0).all() or (ev < 0).all() else "indefinite"
        err = float(max(abs(Fraction(float(a)) - e) for a, e in zip(x, xe)) / scale) / (cond * R.EPS)
        count[group] = count.get(group, 0) + 1
        if err > worst.get(group, (0.0,))[0]:
            worst[group] = (err, q["cls"], q["lam"], cond)
    print(f"\noracle LDLT vs exact, worst relative error / (cond 2^-53) and where: {worst}; systems: {count}")
    assert count["definite"] >= 150 and count["indefinite"] >= 50 and count["zero diagonal"] >= 5
    assert worst["definite"][0] <= C_BOUND_DEFINITE
    assert worst["indefinite"][0] <= C_BOUND_INDEFINITE


# ---------------------------------------------------------------------------------------------------------------------------------
# D  non-finite systems
# ---------------------------------------------------------------------------------------------------------------------------------
def active_unknowns(mode_name):
    return {"ab": range(8), "fix_ab": range(6), "fix_b": range(7), "fix_a": (0, 1, 2, 3, 4, 5, 7)}[mode_name]


@pytest.mark.gpu
@pytest.mark.parametrize("mode_name,fixed", [(m, 0) for m in R.MODES] + [("ab", 3)])
def test_nonfinite_systems(trackers, mode_name, fixed):
    """NaN / +-Inf on and off the diagonal and in b.  The raw increment is the oracle's in EVERY mode, a NaN compared as a NaN: the
    rows that pad a 6- or 7-dim sub-solve to eight are kept zero by selection, so the device performs the operations of the oracle's
    smaller system and nothing else reaches the active unknowns (a padding zero times a NaN would; with a NaN on the diagonal of the
    active block the oracle's increment is FINITE -- Eigen never divides by that pivot -- and so is the device's, bit for bit).  A bad
    entry outside the active block never enters.  Where the increment is not finite, both hold a non-finite active unknown and zeros
    for the inactive ones, the non-finite sum gives a zero step (cand = exp(0) * cur, aff_cand = aff_cur), inc_norm is NaN, and the
    evaluation is the level's last unless the schedule is fixed.  inc_norm, aff_cand and residual_only are the oracle's bit for bit
    throughout."""
    p = ref_params(mode_name, fixed)
    cases = [dict(H=H, b=b, lam=lam, iteration=n % 3) for n, (H, b, lam) in enumerate(R.nonfinite_problems())]
    out = trackers(mode_name, fixed).diagLmPropose(0, LVL, pack(cases), spec=False, helper=True)
    zero_step = R.orc_se3_mul(R.orc_se3_exp(np.zeros(6)), CUR)
    act = list(active_unknowns(mode_name))
    inact = [i for i in range(8) if i not in act]
    n_nonfinite, bad = 0, []
    for n, (q, o) in enumerate(zip(cases, out)):
        r = R.step_oracle(p, 0, LVL, q["H"], q["b"], q["lam"], CUR, AFF, q["iteration"])
        w = (mode_name, n, np.array(o["inc"]), r["inc"], o["inc_norm"], r["inc_norm"])
        ok = [R.same_bits(np.array(o["inc"]), r["inc"], nan_as_nan=True),
              R.same_bits(np.float64(o["inc_norm"]), np.float64(r["inc_norm"]), nan_as_nan=True),
              R.same_bits(np.array(o["aff_cand"]), r["aff_cand"]), o["residual_only"] == r["residual_only"]]
        if not np.all(np.isfinite(r["inc"])):
            n_nonfinite += 1
            ok += [not np.all(np.isfinite(o["inc"][act])) and not np.all(np.isfinite(r["inc"][act])),
                   not o["inc"][inact].any() and not r["inc"][inact].any(),
                   R.same_bits(np.array(o["cand"]), zero_step) and R.same_bits(r["cand"], zero_step),
                   R.same_bits(np.array(o["aff_cand"]), np.array(AFF)),
                   math.isnan(o["inc_norm"]) and math.isnan(r["inc_norm"]),
                   o["residual_only"] == (1 if not fixed else int(q["iteration"] + 1 >= fixed))]
        if not all(ok):
            bad.append((ok, w))
    print(f"\n{mode_name} fixed {fixed}: {n_nonfinite} of {len(cases)} increments not finite; {len(bad)} problems differ")
    assert not bad, (len(bad), bad[:4])
    assert n_nonfinite >= 25


# ---------------------------------------------------------------------------------------------------------------------------------
# E  the SE3 update
# ---------------------------------------------------------------------------------------------------------------------------------
def theta_of(xi):
    return math.sqrt(xi[3] * xi[3] + xi[4] * xi[4] + xi[5] * xi[5])  # (the code's own sum order)


@functools.lru_cache(maxsize=None)
def se3_reference():
    """per case: the system handed over and the oracle's step"""
    p = ref_params("ab")
    out = []
    for xi, cur in R.se3_cases():
        H, b = R.se3_system(p, xi)
        r = R.step_oracle(p, 0, LVL, H, b, 1.0, cur, AFF, 0)
        assert np.array_equal(r["inc_scaled"][:6], xi)  # the round trip through the solve is exact (up to the sign of a zero)
        out.append((dict(H=H, b=b, lam=1.0, cur=cur), r))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def se3_truth():
    """{case index: exp(xi) * cur in mpmath} for theta >= 1e-3"""
    return {n: R.se3_exp_mp(xi) * R.pose_to_mp(cur) for n, (xi, cur) in enumerate(R.se3_cases()) if theta_of(xi) >= 1e-3}


@functools.lru_cache(maxsize=None)
def oracle_mp_worst():
    """the oracle's own worst (rotation, translation) error against mpmath over the set, in R.mp_errors' units"""
    truth, cases = se3_truth(), R.se3_cases()
    errs = [R.mp_errors(se3_reference()[n][1]["cand"], T, theta_of(cases[n][0]), np.linalg.norm(cases[n][0][:3])) for n, T in truth.items()]
    return max(e[0] for e in errs), max(e[1] for e in errs)


def test_oracle_se3_against_mpmath(built):
    rot, tr = oracle_mp_worst()
    print(f"\noracle exp(xi) * cur vs mpmath over {len(se3_truth())} cases with theta >= 1e-3: worst rotation entry error {rot:.2f} x 2^-53, "
          f"worst translation error {tr:.2f} x 2^-53 ((1 + 1/theta) |upsilon| + |t|)")
    assert len(se3_truth()) >= 300
    # exp, one quaternion product, one rotation and the conversion to a matrix: tens of roundings at the most
    assert rot < 64 and tr < 64


@pytest.mark.gpu
@pytest.mark.parametrize("mode,spec,helper", [(0, 0, 1), (2, 0, 0), (0, 1, 1)])
def test_se3_update(trackers, mode, spec, helper):
    """H = I drives a chosen twist through the step.  theta < 1e-10: no sincos runs, the candidate is the oracle's bit for bit.
    Otherwise the device's and the host's sincos may differ by delta = 4 x 2^-53 and everything else is the same IEEE operations: the
    quaternion within 8 delta of the oracle's and of unit norm to 4 x 2^-53 (checked exactly, in rationals), the translation within
    8 delta (1 + 1/theta) |upsilon| + 8 x 2^-53 |t|; for theta >= 1e-3 also within four times the oracle's own worst error of mpmath's
    exp(xi) * cur.  M = float(R) K^-1 (mode 2: float(R)) and float(t), recomputed on the host from the DEVICE's candidate, bit for bit."""
    ref = se3_reference()
    cases = R.se3_cases()
    out = trackers("ab").diagLmPropose(mode, LVL, pack([q for q, _ in ref]), spec=spec, helper=helper)
    truth, (rot_worst, tr_worst) = se3_truth(), oracle_mp_worst()
    Ki = np.array(out[0]["Ki"])
    K = S.level_K(level_K(), LVL)  # makeK, TrackerAndScaler.cpp:117-133
    np.testing.assert_allclose(Ki.reshape(3, 3), np.linalg.inv(np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1.0]])), rtol=1e-6, atol=1e-9)
    mx = dict(q=0.0, t=0.0, norm=0.0, rot=0.0, tr=0.0)
    n_small = 0
    for n, ((xi, cur), (q, r), o) in enumerate(zip(cases, ref, out)):
        theta, ups = theta_of(xi), float(np.linalg.norm(xi[:3]))
        cand = np.array(o["cand"])
        w = (n, theta, ups, cand, r["cand"])
        assert R.same_bits(np.array(o["inc"]), r["inc"]), w
        if theta < 1e-10:
            n_small += 1
            assert R.same_bits(cand, r["cand"]), w
        else:
            dq = float(np.abs(cand[:4] - r["cand"][:4]).max())
            n2 = sum(Fraction(float(v)) ** 2 for v in cand[:4])
            lo, hi = (1 - Fraction(4 * R.EPS)) ** 2, (1 + Fraction(4 * R.EPS)) ** 2
            dt = float(np.abs(cand[4:] - r["cand"][4:]).max())
            t_bound = 8 * DELTA * (1 + 1 / theta) * ups + 8 * R.EPS * float(np.linalg.norm(r["cand"][4:]))
            mx["q"], mx["norm"] = max(mx["q"], dq / DELTA), max(mx["norm"], abs(math.sqrt(float(n2)) - 1) / R.EPS)
            if t_bound > 0:
                mx["t"] = max(mx["t"], dt / t_bound)
            assert dq <= 8 * DELTA, w
            assert lo <= n2 <= hi, w
            assert dt <= t_bound, (w, dt, t_bound)
        if n in truth:
            rot, tr = R.mp_errors(cand, truth[n], theta, ups)
            mx["rot"], mx["tr"] = max(mx["rot"], rot), max(mx["tr"], tr)
            assert rot <= 4 * rot_worst and tr <= 4 * tr_worst, (w, rot, tr, rot_worst, tr_worst)
        M, t = R.eval_rot(mode, cand, Ki)
        assert R.same_bits(np.array(o["M"]), M) and R.same_bits(np.array(o["t"]), t), (w, o["M"], M, o["t"], t)
        assert R.same_bits(np.array(o["aff_cand"]), np.array(AFF)), w
    assert n_small >= 100 and len(cases) - n_small >= 400
    print(f"\nmode {mode} spec {spec} helper {helper}: worst |dq| {mx['q']:.3f} delta (bound 8), | |q| - 1 | {mx['norm']:.2f} x 2^-53 (bound 4), "
          f"|dt| {mx['t']:.3f} of its bound; against mpmath: rotation {mx['rot']:.2f} x 2^-53 (oracle {rot_worst:.2f}), translation "
          f"{mx['tr']:.2f} units (oracle {tr_worst:.2f})")


# ---------------------------------------------------------------------------------------------------------------------------------
# F  the scale step
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("spec", (0, 1))
def test_scale_step(trackers, spec):
    """propose_scale against the float32 restatement: inc, scale_cand (a NaN compared as NaN), residual_only, cutoff, max_energy"""
    p = ref_params("ab")
    max_it = p.max_iterations[LVL]
    cases = [dict(Hs=Hs, bs=bs, scale_cur=sc, lam=lam, iteration=(0, max_it - 2, max_it - 1)[n % 3], level_cutoff_repeat=(1.0, 4.0)[n % 2])
             for n, (Hs, bs, sc, lam) in enumerate(R.scale_cases())]
    assert len(cases) <= 4096
    out = trackers("ab").diagLmPropose(1, LVL, pack(cases), spec=spec)
    seen = set()
    for n, (q, o) in enumerate(zip(cases, out)):
        inc, cand, last, cutoff, max_energy = R.scale_step_ref(p, LVL, q["Hs"], q["bs"], q["scale_cur"], q["lam"], q["iteration"],
                                                                q["level_cutoff_repeat"], spec=bool(spec))
        w = (n, q, o["inc_f"], o["scale_cand"], o["residual_only"], inc, cand, last)
        assert R.same_bits(np.float32(o["inc_f"]), inc), w
        assert R.same_bits(np.float32(o["scale_cand"]), cand, nan_as_nan=True), w
        assert o["residual_only"] == last, w
        assert R.same_bits(np.float32(o["cutoff"]), cutoff) and R.same_bits(np.float32(o["max_energy"]), max_energy), w
        seen.add((bool(inc != 0), last))
    assert seen == {(False, 1), (True, 0), (True, 1)}  # (a zero increment is never > 1e-3: it always ends the level)


# ---------------------------------------------------------------------------------------------------------------------------------
# G  argument errors
# ---------------------------------------------------------------------------------------------------------------------------------
def _call(L, handle, mode, lvl, n, arr_in, arr_out):
    from direct_stereo_slam_amd._lib import LmProposeIn, LmProposeOut

    return L.dsm_diag_lm_propose(handle, mode, lvl, n, None if arr_in is None else arr_in.ctypes.data_as(C.POINTER(LmProposeIn)), 0, 0,
                                 None if arr_out is None else arr_out.ctypes.data_as(C.POINTER(LmProposeOut)))


def test_null_tracker_is_invalid(built):
    from direct_stereo_slam_amd import _lib
    from direct_stereo_slam_amd.tracker import LM_PROPOSE_OUT

    L = _lib.load()
    out = np.zeros(2, LM_PROPOSE_OUT)
    out.view(np.uint8)[:] = 0xA5
    assert _call(L, None, 0, 0, 2, pack([dict(lam=0.01)] * 2), out) == -1  # DSM_ERR_INVALID
    assert b"dsm_diag_lm_propose" in L.dsm_last_error()
    assert np.all(out.view(np.uint8) == 0xA5)


@pytest.mark.gpu
def test_invalid_arguments(trackers, ctx):
    from direct_stereo_slam_amd.tracker import LM_PROPOSE_OUT, TrackerAndScaler

    trk = trackers("ab")
    L, nl = trk.L, SIZES[SIZE][3]
    arr = pack([dict(lam=0.01, H=np.eye(8))] * 2)
    out = np.zeros(2, LM_PROPOSE_OUT)
    out.view(np.uint8)[:] = 0xA5
    for args in ((trk.h, 0, LVL, 0, arr, out), (trk.h, 0, LVL, -3, arr, out), (trk.h, 0, LVL, 65537, arr, out), (trk.h, 3, LVL, 2, arr, out),
                 (trk.h, -1, LVL, 2, arr, out), (trk.h, 0, -1, 2, arr, out), (trk.h, 0, nl, 2, arr, out), (trk.h, 0, LVL, 2, None, out),
                 (None, 0, LVL, 2, arr, out)):
        assert _call(L, *args) == -1, args[1:4]
        assert np.all(out.view(np.uint8) == 0xA5), args[1:4]
    assert _call(L, trk.h, 0, LVL, 2, arr, None) == -1
    w, h, _, nl = SIZES[SIZE]
    fresh = TrackerAndScaler(ctx, w, h, nl, S.KITTI_T_STEREO, level_K())  # no makeK yet: no K^-1 to read
    assert _call(L, fresh.h, 0, LVL, 2, arr, out) == -1 and np.all(out.view(np.uint8) == 0xA5)
    fresh.close()
    assert _call(L, trk.h, 0, LVL, 2, arr, out) == 0 and not np.all(out.view(np.uint8) == 0xA5)  # and the same call with good arguments runs
