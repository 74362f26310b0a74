"""CPU: the checker of the window optimisation's step (tests/_step_ref.py), the scenes it is run on, the host form
dsm_window_step_host against it bit for bit, and four checks that do not depend on the restated formulas: the group structure of the
pair transforms in float64 4 x 4 matrices, the projection through the tables, the zero step, and W C = 1 with the error of exp and
se3_exp against mpmath at 50 digits."""
import math
from fractions import Fraction

import numpy as np
import pytest

import _linearize_ref as R
import _lm_step_ref as LS
import _solve_ref as SR
import _step_ref as T
from direct_stereo_slam_amd import step as S
from direct_stereo_slam_amd import synth
from direct_stereo_slam_amd._lib import DsmError

f32, f64 = np.float32, np.float64
U24, U53 = 2.0 ** -24, 2.0 ** -53
HOST_SCENES = ["scene", "nine_frames", "one_frame", "two_frames", "three_frames", "sixteen_frames", "no_points", "three_frames_no_residuals",
               "no_priors", "no_h_m", "zero_step", "lambda_10", "null_2"]


def host(job, frames, **kw):
    got = S.window_step_host(R.W, R.H, job, frames, **kw)
    return dict(got, H_L=got["H_L_step"], b_L=got["b_L_step"])


# ---- the scenes, on the checker's output alone -------------------------------------------------------------------------------------

def test_scenes_exercise_what_the_device_tests_rely_on():
    """Counted on the checker's output: after the step 102 residuals are active in the 5-frame scene and 122 in the 9-frame scene
    (at least 20 asked); between the zero step and the full step 19 residuals of the 5-frame scene change their new state (at least 3
    asked; IN -> OOB, IN -> OUTLIER, OOB -> IN, OUTLIER -> IN and OUTLIER -> OOB all occur); frame 0 takes se3_exp's series branch, every other frame the general one."""
    for name in ("scene", "nine_frames"):
        exp = T.expected(name)[2]
        assert int(exp["active"].sum()) >= 20, (name, int(exp["active"].sum()))
    full, zero = T.expected("scene")[2], T.expected("zero_step")[2]
    changed = full["new_state"] != zero["new_state"]
    assert int(changed.sum()) >= 3, int(changed.sum())
    pairs = set(zip(zero["new_state"][changed].tolist(), full["new_state"][changed].tolist()))
    assert pairs & {(R.IN, R.OUTLIER), (R.OUTLIER, R.IN), (R.IN, R.OOB), (R.OUTLIER, R.OOB)}, pairs
    taken = set()
    T.step(T.scene("scene")[0], taken=taken)
    assert taken == {"series", "general"}


def test_can_break_cases_are_decided_by_one_threshold_each():
    jobs = T.break_jobs()
    assert T.step(jobs["break"])["break_tests"] == [True] * 4 and T.step(jobs["break"])["can_break"] == 1
    for i, which in enumerate(("A", "B", "R", "T")):
        st = T.step(jobs[which])
        assert st["can_break"] == 0 and st["break_tests"] == [k != i for k in range(4)], (which, st["break_tests"])


def test_checker_se3_equals_the_oracle():
    rng = np.random.default_rng(11)
    for k in range(40):
        xi = rng.normal(0, 1, 6) * (1e-11 if k % 8 == 0 else 0.3)
        a = np.array(T.se3_exp(list(xi)))
        assert a.tobytes() == LS.orc_se3_exp(xi).tobytes()
        b = np.array(T.se3_exp(list(rng.normal(0, 0.5, 6))))
        assert np.array(T.se3_mul(list(a), list(b))).tobytes() == LS.orc_se3_mul(a, b).tobytes()
        assert np.array(T.quat_to_rot(list(a))).tobytes() == LS.orc_quat_to_rot(a).tobytes()


# ---- the host form -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", HOST_SCENES)
def test_host_form_equals_the_checker_bit_for_bit(built, name):
    """Every output of D1-E3 and of sections 16-18 at the trial state.  The checker's sin, cos and exp are the C library's, as the
    host form's: no relaxation is needed, and none is applied."""
    job, frames, exp = T.expected(name)
    got = host(job, frames)
    T.assert_step_equal(got, exp)
    SR.assert_equal(got, exp, hes_outputs=SR.HR.RAW + ("active", "JpJdF") + SR.HR.PER_POINT)


@pytest.mark.parametrize("which", ["break", "A", "B", "R", "T"])
def test_host_form_can_break(built, which):
    job = T.break_jobs()[which]
    frames = T.scene("two_frames")[1]
    got = host(job, frames)
    exp = T.step(job)
    assert got["can_break"] == exp["can_break"] == (1 if which == "break" else 0)
    T.assert_step_equal(got, exp, outputs=("step_sums", "state", "world_to_cam"))


def test_host_form_without_points_gives_the_reference_zero_by_zero(built):
    job, frames, exp = T.expected("no_points")
    got = host(job, frames)
    assert np.isnan(got["step_sums"][4]) and np.isnan(got["step_sums"][5]) and got["can_break"] == 0 == exp["can_break"]


def test_host_form_optional_outputs_null(built):
    job, frames, exp = T.expected("three_frames")
    got = S.window_step_host(R.W, R.H, job, frames, outputs=())
    T.assert_step_equal(got, exp, outputs=("state", "calib", "idepth", "world_to_cam", "can_break", "step_sums", "energy_m"))
    SR.assert_equal(got, exp, outputs=("x", "step", "flags"))
    for k in ("cam_to_world", "cam", "pre_KRKiTll", "delta_x", "H_L_step", "b_L_step"):
        assert (np.asarray(got[k]) == S.FILL).all(), k


def test_host_form_refuses_all_or_nothing(built):
    job, frames = T.scene("three_frames")
    for what, bad in T.invalid_jobs(job):
        b = S.StepBatch([bad])
        before = {k: v.copy() for k, v in b.all_outputs()[0].items()}
        with pytest.raises(DsmError):
            b.run_host(R.W, R.H, 0, frames)
        for k, v in b.all_outputs()[0].items():
            assert v.tobytes() == before[k].tobytes(), (what, k)
    for kw in (dict(scale_a=np.nan), dict(scale_b=0.0), dict(th_opt_iterations=np.inf)):
        with pytest.raises(DsmError):
            S.StepBatch([job]).run_host(R.W, R.H, 0, frames, step_params=S.default_step_params(**kw))


# ---- 1. group structure ------------------------------------------------------------------------------------------------------------

def _mat(pose):
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = synth.quat_to_rot(np.asarray(pose[:4], f64)), pose[4:7]
    return M


def _exp44(xi):
    """exp of [upsilon; omega] by Rodrigues' formula on matrices"""
    u, o = np.asarray(xi[:3], f64), np.asarray(xi[3:6], f64)
    th = float(np.linalg.norm(o))
    Om = np.array([[0, -o[2], o[1]], [o[2], 0, -o[0]], [-o[1], o[0], 0]])
    M = np.eye(4)
    if th < 1e-12:
        M[:3, :3], M[:3, 3] = np.eye(3) + Om, u
        return M
    M[:3, :3] = np.eye(3) + math.sin(th) / th * Om + (1 - math.cos(th)) / th ** 2 * Om @ Om
    M[:3, 3] = (np.eye(3) + (1 - math.cos(th)) / th ** 2 * Om + (th - math.sin(th)) / th ** 3 * Om @ Om) @ u
    return M


def _float_pair(L):
    return np.array([f32(x) for x in T.quat_to_rot(L)], f32).reshape(3, 3), np.array([f32(x) for x in L[4:7]], f32)


def _within(Rf, tf, M64):
    """The checker's float R, t against a float64 4 x 4.  Bound: the cast to float is one rounding, 2^-24 relative; before it, either
    side forms the entry from the inputs in fewer than 64 double operations on magnitudes of at most 1 + |t|, each rounding 2^-53."""
    tn = 1.0 + float(np.abs(M64[:3, 3]).max())
    return bool((np.abs(Rf.astype(f64) - M64[:3, :3]) <= U24 * np.abs(M64[:3, :3]) + 64 * U53 * tn).all()
                and (np.abs(tf.astype(f64) - M64[:3, 3]) <= U24 * np.abs(M64[:3, 3]) + 64 * U53 * tn).all())


def test_group_structure_of_the_pair_transforms():
    job, _ = T.scene("scene")
    n = 5
    a = 2
    zero = np.asarray(job["state_zero"], f64)
    backup = zero.copy()
    backup[:, :6] = 0.0
    fstep = np.zeros((n, 8))
    fstep[a, :6] = [0.03, -0.02, 0.01, 0.004, -0.003, 0.002]
    base = T.step(dict(job, state_backup=backup, frame_step=np.zeros((n, 8))))
    st = T.step(dict(job, state_backup=backup, frame_step=fstep))
    xi = np.array(st["scaled"][a][:6])
    E = [_mat(p) for p in np.asarray(job["world_to_cam_eval"], f64)]
    ev = [[float(x) for x in p] for p in np.asarray(job["world_to_cam_eval"], f64)]
    W, C = [[[float(x) for x in p] for p in st[k]] for k in ("world_to_cam", "cam_to_world")]
    ok_swapped = ok_right = 0
    for h in range(n):
        for t in range(n):
            if h == t:
                continue
            L0 = E[t] @ np.linalg.inv(E[h])
            want = _exp44(xi) @ L0 if t == a else L0 @ _exp44(-xi) if h == a else L0  # left factor on the target, right factor on the host
            Rf, tf = _float_pair(st["pairs"][h, t][0])
            assert _within(Rf, tf, want), (h, t)
            if a not in (h, t):
                for k in T.PRE:
                    assert st[k][h, t].tobytes() == base[k][h, t].tobytes(), (k, h, t)
            else:  # the mutations, on the checker's own code: host for target, and C_h W_t for W_t C_h
                ok_swapped += _within(*_float_pair(st["pairs"][t, h][0]), want)
                mut = T.pair_row(ev[t], T.se3_inverse(ev[h]), W[t], C[h], st["cam"], 1.0, 1.0, [0.0, 0.0], [0.0, 0.0], 0.0, 1.0, left=False)
                if 0 in (h, t):  # frame 0 has the identity pose and no step: its W and C are the identity, and the two orders are one
                    assert _within(*_float_pair(mut["L"]), want)
                else:
                    ok_right += _within(*_float_pair(mut["L"]), want)
                same = T.pair_row(ev[t], T.se3_inverse(ev[h]), W[t], C[h], st["cam"], 1.0, 1.0, [0.0, 0.0], [0.0, 0.0], 0.0, 1.0)
                assert same["L"] == st["pairs"][h, t][0]  # (the unmutated call is the checker's own row)
    assert ok_swapped == 0 and ok_right == 0, (ok_swapped, ok_right)


# ---- 2. projection -----------------------------------------------------------------------------------------------------------------

def test_projection_through_the_tables():
    """K R K^-1 (u, v, 1) + K t idepth, dehomogenised, against the float64 pinhole chain through cam, L and cam; and R0 (x, y, 1) +
    t0 idepth on normalised coordinates, the form L2 uses.  Bound: a table entry is formed from float casts of K, R and K^-1 (K^-1's
    third column one more product) by two nested three-term products: at most 12 roundings of 2^-24 on the absolute-value expression.
    An entry of K R is at most F = fx + cx + cy, the columns of K^-1 are (fxi, 0, 0), (0, fyi, 0) and (-cx fxi, -cy fyi, 1), so a
    component's absolute-value expression is at most S = F (fxi u + fyi v + cx fxi + cy fyi + 1) + |Kt| idepth; the quotient of two
    such components doubles the relative error.  pre_RTll_0 and pre_tTll_0 are float casts of the double entries and nothing more: ONE
    rounding of 2^-24 per entry, and the double entries within 64 x 2^-53 of the float64 chain's (the group-structure test's count); the
    test evaluates both sides in float64, so a component errs by at most (2^-24 + 64 x 2^-53) S0 with S0 = |x| + |y| + 1 + |t0| idepth
    (|R0_ij| <= 1), and the quotient doubles it."""
    job, _ = T.scene("scene")
    st = T.step(job)
    cam = st["cam"].astype(f64)
    K = np.array([[cam[0], 0, cam[2]], [0, cam[1], cam[3]], [0, 0, 1]])
    Ki = np.array([[cam[4], 0, -cam[2] * cam[4]], [0, cam[5], -cam[3] * cam[5]], [0, 0, 1]])
    F = cam[0] + cam[2] + cam[3]
    rng = np.random.default_rng(3)
    worst = worst0 = 0.0
    for _ in range(50):
        h, t = rng.choice(5, 2, replace=False)
        u, v, idp = rng.uniform(0, R.W), rng.uniform(0, R.H), rng.uniform(0.05, 0.5)
        L, L0, _a = st["pairs"][h, t]
        M64, M0 = _mat(L), _mat(L0)
        p = st["pre_KRKiTll"][h, t].astype(f64).reshape(3, 3) @ [u, v, 1.0] + st["pre_KtTll"][h, t].astype(f64) * idp
        x = Ki @ [u, v, 1.0]
        q = K @ (M64[:3, :3] @ x + M64[:3, 3] * idp)
        err = np.abs(p[:2] / p[2] - q[:2] / q[2]).max()
        S_abs = F * (cam[4] * u + cam[5] * v + cam[2] * cam[4] + cam[3] * cam[5] + 1) + np.abs(K @ M64[:3, 3]).max() * idp
        bound = 2 * 12 * U24 * S_abs / abs(q[2])
        assert err <= bound, (h, t, err, bound)
        worst = max(worst, err / bound)
        p0 = st["pre_RTll_0"][h, t].astype(f64).reshape(3, 3) @ x + st["pre_tTll_0"][h, t].astype(f64) * idp
        q0 = M0[:3, :3] @ x + M0[:3, 3] * idp
        S0 = np.abs(x).sum() + np.abs(M0[:3, 3]).max() * idp
        bound0 = 2 * (U24 + 64 * U53) * S0 / abs(q0[2])
        err0 = np.abs(p0[:2] / p0[2] - q0[:2] / q0[2]).max()
        assert err0 <= bound0, (h, t, err0, bound0)
        worst0 = max(worst0, err0 / bound0)
    print(f"\nprojection: worst error {worst:.4f} of its bound; through R0, t0 {worst0:.4f} of its bound")


# ---- 3. zero step ------------------------------------------------------------------------------------------------------------------

def test_zero_step_is_the_solve_at_the_backup_and_energy_m_is_exact():
    job, frames, exp = T.expected("zero_step")
    st = T.step(job)
    assert np.array_equal(st["state"], np.asarray(job["state_backup"], f64)) and np.array_equal(st["idepth"], np.asarray(job["idepth_backup"], f32))
    # the job a caller of dsm_window_solve_batch would hold at the backup state, assembled here from the checker's tables, through the
    # three checkers of sections 16-18 called directly
    cjob = {k: v for k, v in job.items() if k not in T.STEP_IN}
    cjob.update({k: st[k] for k in T.PRE})
    cjob.update(cam=tuple(st["cam"][:4]), cam_inv=tuple(st["cam"][4:]), idepth_scaled=np.asarray(job["idepth_backup"], f32),
                idepth_zero_scaled=np.asarray(job["idepth_backup"], f32), delta=np.zeros(len(job["host"]), f32), delta_x=st["delta_x"],
                H_L=st["H_L"], b_L=st["b_L"])
    lin = R.linearize(R.W, R.H, cjob, frames)
    hes = dict(lin, **SR.HR.hessian(cjob, lin, cjob))
    SR.assert_equal(exp, dict(hes, **SR.solve(cjob, hes)), hes_outputs=SR.HR.RAW + ("active", "JpJdF") + SR.HR.PER_POINT)
    N = len(st["delta_x"])
    dx = [Fraction(float(x)) for x in st["delta_x"]]
    HM, bM = np.asarray(job["H_M"], f64).reshape(N, N), np.asarray(job["b_M"], f64)
    exact = sum(dx[i] * (2 * Fraction(float(bM[i])) + sum(Fraction(float(HM[i, j])) * dx[j] for j in range(N))) for i in range(N))
    absval = sum(abs(dx[i]) * (2 * abs(Fraction(float(bM[i]))) + sum(abs(Fraction(float(HM[i, j]))) * abs(dx[j]) for j in range(N))) for i in range(N))
    gamma = (N + 2) * U53 / (1 - (N + 2) * U53)  # gamma_{N+2} of the absolute-value expression
    err = abs(Fraction(float(st["energy_m"])) - exact)
    print(f"\nenergy_m: error {float(err / (Fraction(gamma) * absval)):.3f} of gamma_(N+2) x the absolute-value expression")
    assert err <= Fraction(gamma) * absval


# ---- 4. W C = 1, and the checker's transcendental error --------------------------------------------------------------------------------

def test_world_to_cam_times_cam_to_world_is_the_identity_and_the_error_of_exp():
    """Against mpmath at 50 digits.  W C: both are unit quaternions to 4 x 2^-53 and C's translation is -(q' t) in 12 operations, so
    every entry of the 4 x 4 product is within 32 x 2^-53 (1 + |t|)^2 of the identity's.  Measured on the scenes: the checker's
    exp of Q4 errs by at most 0.97 units of 2^-53 relative (half an ulp), its se3_exp, where theta >= 1e-3, by 0.01 (rotation
    entries) and 0.38 (translation, in mp_errors' unit); printed below and recorded in DESIGN.md section 19."""
    mp = LS._mp()
    worst_exp = worst_rot = worst_tr = worst_wc = 0.0
    for name in ("scene", "nine_frames", "sixteen_frames"):
        job, _ = T.scene(name)
        st = T.step(job)
        for f, (Wp, Cp) in enumerate(zip(st["world_to_cam"], st["cam_to_world"])):
            D = LS.pose_to_mp(Wp) * LS.pose_to_mp(Cp) - mp.eye(4)
            tn = (1 + float(np.abs(Wp[4:]).max())) ** 2
            err = max(abs(D[i, j]) for i in range(4) for j in range(4))
            assert err <= 32 * U53 * tn, (name, f, float(err))
            worst_wc = max(worst_wc, float(err / (U53 * tn)))
            xi = st["scaled"][f][:6]
            theta = math.sqrt(sum(x * x for x in xi[3:]))
            if theta >= 1e-3:
                rot, tr = LS.mp_errors(np.array(T.se3_exp(xi)), LS.se3_exp_mp(xi), theta, math.sqrt(sum(x * x for x in xi[:3])))
                worst_rot, worst_tr = max(worst_rot, rot), max(worst_tr, tr)
        for (h, t), (_L, _L0, a) in st["pairs"].items():
            d = st["scaled"][t][6] - st["scaled"][h][6]
            truth = mp.exp(mp.mpf(d))
            worst_exp = max(worst_exp, float(abs(mp.mpf(math.exp(d)) - truth) / truth / mp.mpf(U53)))
    print(f"\nW C - 1: {worst_wc:.2f} x 2^-53 (1 + |t|)^2 (bound 32); exp of Q4: {worst_exp:.3f} x 2^-53; se3_exp: rotation {worst_rot:.2f}, "
          f"translation {worst_tr:.2f} x 2^-53")
    assert worst_exp <= 1.0 and worst_rot <= 8.0 and worst_tr <= 8.0
