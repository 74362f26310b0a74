"""CPU: the checker of the window's nullspaces and their pseudo-inverse (tests/_nullspace_ref.py), the host form
dsm_window_nullspace_host against it, and three checks that do not depend on the stated order: the analytic adjoint, numpy's pinv and
SVD, and the four Penrose conditions.

The constants C_POSE, C_SCALE, K_PINV and K_SING were measured on the checker over this file's scenes (`pytest -s` prints the figures
again); the bounds built from them are the issue's forms:
  a block entry against the adjoint:  c (1 + |t|) 2^-53 / 1e-3, c = C_* for the checker, 4 C_* for the host form and the device
                                      (4: the device's atan and tan may be a few ulp from the C library's, on two functions)
  null_pinv against numpy's:          K_PINV 2^-53 kappa_kept max|pinv|, K_PINV = 8 x the measured 14.2
  sing against numpy's SVD:           K_SING 2^-53 kappa_kept sigma_max, K_SING = 8 x the measured 5.5"""
import numpy as np
import pytest

import _nullspace_ref as NR
from direct_stereo_slam_amd import nullspace as NS
from direct_stereo_slam_amd._lib import DsmError

f64 = np.float64
U53 = 2.0 ** -53
C_POSE, C_SCALE = 1.5, 0.52  # measured on the checker: 1.454 and 0.517
K_PINV = 8 * 14.2            # measured on the checker: 14.16 (nine frames)
K_SING = 8 * 5.5             # measured on the checker: 5.50
DELTA = NR.NP["solver_mode_delta"]


def poses(job):
    return np.asarray(job["world_to_cam_eval"], f64).reshape(-1, 7)


def blocks_of_pre(pre, n):
    """the frames' 6 x 7 blocks back from null_x0_pre: x scale_xi_trans = 0.5 and x scale_xi_rot = 1 are exact"""
    pre = np.asarray(pre, f64).reshape(-1, 9)
    out = np.zeros((n, 6, 7))
    for f in range(n):
        rows = pre[4 + 8 * f:4 + 8 * f + 6][:, [0, 1, 2, 3, 4, 5, 8]]
        out[f] = rows * np.array([0.5, 0.5, 0.5, 1.0, 1.0, 1.0])[:, None]
    return out


def adjoint_worst(res, job):
    """(pose columns, scale column): the largest distance from the analytic adjoint, of frame_null and of null_x0_pre's blocks, in
    units of (1 + |t|) 2^-53 / 1e-3"""
    ev = poses(job)
    worst = [0.0, 0.0]
    for blocks in (np.asarray(res["frame_null"]).reshape(len(ev), 6, 7), blocks_of_pre(res["null_x0_pre"], len(ev))):
        for f in range(len(ev)):
            p, s = NR.adjoint_units(blocks[f], ev[f])
            worst = [max(worst[0], p), max(worst[1], s)]
    return worst


def kept_of(basis):
    sv = np.linalg.svd(basis, compute_uv=False)
    kept = sv[sv > DELTA * sv[0]]
    return sv, kept, float(kept[0] / kept[-1])


# ---- 1: the branch condition, and what follows from it --------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NR.POSE_SCENES)
def test_branches_and_libm_free_columns(name):
    """columns 0-2 and 6 take the two series branches, columns 3-5 atan / tan; so no libm function lies on the path of columns 0-2 and
    6, and the host form's equal the checker's bit for bit"""
    exp, job = NR.expected(name), NR.scene(name)
    for taken in exp["branches"]:
        for c, b in enumerate(taken):
            assert b == (("series", "series") if c % 6 < 3 or c >= 12 else ("atan", "tan")), (name, c, b)
    got = NS.window_nullspace_host([job])[0]
    a, b = got["frame_null"].reshape(-1, 6, 7), exp["frame_null"].reshape(-1, 6, 7)
    for col in (0, 1, 2, 6):
        assert NR.bits_equal(a[:, :, col], b[:, :, col]), (name, col)
    print(f"\n{name}: columns 3-5 {'equal' if NR.bits_equal(a, b) else 'differ from'} the checker's bit for bit (same C library)")


# ---- 2: bit equality with frame_null_in given ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [n for n in NR.GIVEN_SCENES if not any(n.endswith(f"_{k}") for k in (7, 9, 15))])
def test_host_form_equals_checker_bit_for_bit(name):
    """G4-G7 hold only + - x / sqrt (and G3's expf, the C library's in both): every output, for 1, 2, 3, 8 and 16 frames and the
    rank-deficient scenes, with the optional outputs given and NULL"""
    exp, job = NR.expected(name), NR.scene(name)
    NR.assert_equal(NS.window_nullspace_host([job])[0], exp)
    bare = NS.window_nullspace_host([job], outputs=())[0]
    NR.assert_equal(bare, exp, outputs=("null_basis", "null_pinv", "sing", "rank", "flags"))
    assert (bare["frame_null"] == NS.FILL).all() and (bare["null_x0_pre"] == NS.FILL).all()


def test_params_null_and_given_and_two_jobs():
    jobs = [NR.scene("given_frames_3"), NR.scene("given_frames_2")]
    both = NS.window_nullspace_host(jobs, params=NS.default_nullspace_params())
    for got, name in zip(both, ("given_frames_3", "given_frames_2")):
        NR.assert_equal(got, NR.expected(name))
    P = dict(scale_xi_trans=0.25, scale_xi_rot=2.0, scale_a=5.0, scale_b=100.0, solver_mode_delta=1e-3)
    NR.assert_equal(NS.window_nullspace_host(jobs[:1], params=NS.default_nullspace_params(**P))[0], NR.nullspace(jobs[0], P))


# ---- 3: the analytic adjoint --------------------------------------------------------------------------------------------------------

def test_adjoint_checker_and_host_form():
    """log(T exp(eps) T^-1) = Ad(T) eps exactly, so the central difference has no truncation error"""
    worst_c, worst_h = [0.0, 0.0], [0.0, 0.0]
    for name in NR.POSE_SCENES:
        job = NR.scene(name)
        c, h = adjoint_worst(NR.expected(name), job), adjoint_worst(NS.window_nullspace_host([job])[0], job)
        worst_c, worst_h = [max(a, b) for a, b in zip(worst_c, c)], [max(a, b) for a, b in zip(worst_h, h)]
    print(f"\nadjoint, in (1 + |t|) 2^-53 / 1e-3: checker pose {worst_c[0]:.3f} scale {worst_c[1]:.3f}; host form pose {worst_h[0]:.3f} scale {worst_h[1]:.3f}")
    assert worst_c[0] <= C_POSE and worst_c[1] <= C_SCALE, worst_c
    assert worst_h[0] <= 4 * C_POSE and worst_h[1] <= 4 * C_SCALE, worst_h


@pytest.mark.parametrize("mutation", [dict(conj_left=True), dict(no_inverse_scale=True), dict(divisor=1e-3)])
def test_adjoint_breaks_under_mutation(mutation):
    """T^-1 exp T instead, a missing 1 / scale, a divisor of 1e-3"""
    job = NR.scene("frames_3")
    p, s = adjoint_worst(NR.nullspace(job, **mutation), job)
    assert p > 100 * 4 * C_POSE, (mutation, p, s)


# ---- 4: numpy's pinv and SVD, Penrose -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["checker", "host"])
def test_pinv_and_singular_values_against_numpy(form):
    worst_p = worst_s = 0.0
    for name in NR.POSE_SCENES + ("equal_columns",):
        res = NR.expected(name) if form == "checker" else NS.window_nullspace_host([NR.scene(name)])[0]
        A, Ap = res["null_basis"], res["null_pinv"]
        N = A.shape[0]
        sv, kept, kappa = kept_of(A)
        ref = np.linalg.pinv(A, rcond=DELTA)
        unit_p, unit_s = U53 * kappa * float(np.abs(ref).max()), U53 * kappa * float(sv[0])
        dp = float(np.abs(Ap - ref).max())
        sing = np.sort(res["sing"])[::-1]
        ds = float(np.abs(sing[:len(kept)] - kept).max())
        worst_p, worst_s = max(worst_p, dp / unit_p), max(worst_s, ds / unit_s)
        assert res["rank"] == len(kept), (name, res["rank"], len(kept))
        assert dp <= K_PINV * unit_p and ds <= K_SING * unit_s, (name, dp / unit_p, ds / unit_s)
        assert (sing[len(kept):] <= DELTA * sing[0]).all(), name
        # Penrose, in float64: the products' own rounding is N 2^-53 of the factors' sizes; the dropped singular values enter the
        # first condition alone (the others hold exactly for the pseudo-inverse of the kept part)
        tol = N * K_PINV * U53 * kappa
        a, p = float(np.abs(A).max()), float(np.abs(Ap).max())
        dropped = float(sing[len(kept):].max()) if len(kept) < 7 else 0.0
        assert np.abs(A @ Ap @ A - A).max() <= tol * a * p * a + dropped, name
        assert np.abs(Ap @ A @ Ap - Ap).max() <= tol * p * a * p, name
        assert np.abs(A @ Ap - (A @ Ap).T).max() <= tol * a * p, name
        assert np.abs(Ap @ A - (Ap @ A).T).max() <= tol * a * p, name
    print(f"\n{form}: null_pinv within {worst_p:.2f} x 2^-53 kappa max|pinv| of numpy's (bound {K_PINV:.1f}), sing within {worst_s:.2f} x 2^-53 kappa sigma_max "
          f"(bound {K_SING:.1f})")


# ---- 5: rank and edge scenes ----------------------------------------------------------------------------------------------------------

def test_rank_and_edge_scenes():
    for name in NR.POSE_SCENES + NR.GIVEN_SCENES:
        exp = NR.expected(name)
        assert exp["flags"] & 2 == 0 and exp["sweeps"] < NR.SWEEP_CAP, (name, exp["flags"], exp["sweeps"])
        assert exp["flags"] & 1 == 0 and np.isfinite(exp["null_x0_pre"]).all(), name
    one = NR.expected("frames_1")
    assert np.abs(poses(NR.scene("frames_1"))[0, 4:]).max() > 0 and one["rank"] == 6 and one["flags"] == 0
    origin = NR.expected("origin_one")
    assert (origin["null_basis"][:, 6] == 0).all() and origin["flags"] == 4
    assert origin["rank"] == len(kept_of(origin["null_basis"])[1]) == 6
    assert NR.expected("origin_first")["rank"] == 7 and NR.expected("origin_first")["flags"] == 0
    eq = NR.expected("equal_columns")
    assert NR.bits_equal(eq["null_basis"][:, 1], eq["null_basis"][:, 4]) and eq["rank"] == len(kept_of(eq["null_basis"])[1]) == 6
    for name in ("frames_1", "origin_one", "origin_first", "equal_columns"):
        NR.assert_equal(NS.window_nullspace_host([NR.scene(name)])[0], NR.expected(name),
                        outputs=("rank", "flags") if "frame_null_in" not in NR.scene(name) else NR.OUT)


def test_full_rank_windows_have_orthonormal_pinv_rows_times_basis():
    """null_pinv null_basis = 1 on a full-rank window: what F7's projector needs"""
    for name in ("frames_2", "frames_8", "frames_16"):
        exp = NR.expected(name)
        kappa = kept_of(exp["null_basis"])[2]
        assert np.abs(exp["null_pinv"] @ exp["null_basis"] - np.eye(7)).max() <= exp["null_basis"].shape[0] * K_PINV * U53 * kappa


# ---- 6: validation ------------------------------------------------------------------------------------------------------------------

def test_refusals_touch_no_output():
    job = NR.scene("frames_2")
    cases = NR.invalid_jobs(job)
    assert any(what == "pose NaN" for what, _, _ in cases)
    for what, bad, params in cases:
        batch = NS.NullspaceBatch([NR.scene("frames_3"), bad])
        with pytest.raises(DsmError):
            batch.run_host(NS.default_nullspace_params(**params) if params else None)
        for out in batch.all_outputs():
            for k, v in out.items():
                assert (v == (77 if k in ("rank", "flags") else NS.FILL)).all(), (what, k)
    p = NS.default_nullspace_params()
    p.struct_size = 8
    with pytest.raises(DsmError):
        NS.NullspaceBatch([job]).run_host(p)
