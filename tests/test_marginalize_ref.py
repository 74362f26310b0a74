"""CPU: the checker of the marginalisation of points and frames (tests/_marginalize_ref.py) reaches every branch
of C on the shared scenes; dsm_window_marginalize_host equals it bit for bit on every output; and, independently of the stated
orders, res_toZeroF lies within a rounding bound of a float64 evaluation, the fold agrees with a dense float64 construction from the
rows, and a frame's marginalisation agrees with the Schur complement and the solution numpy.linalg.solve gives on the unscaled
system, within 16 times what the checker itself deviates from a numpy.longdouble evaluation of its own formulas."""
import ctypes as C

import numpy as np
import pytest

import _hessian_ref as HR
import _linearize_ref as R
import _marginalize_ref as MR

ld = np.longdouble


def host_form(job, frames, **kw):
    from direct_stereo_slam_amd import marginalize

    return marginalize.window_marginalize_host(R.W, R.H, job, frames, **kw)


def test_the_scenes_reach_every_branch():
    """asserted on the checker's output alone"""
    decided, sole, verdicts = set(), set(), set()
    for name in ("scene", "nine_frames", "sixteen_frames"):
        job, _, exp = MR.case(name)
        verdicts |= set(int(v) for v in exp["verdict"])
        for rule, cand in exp["why"]:
            decided.add(rule)
            if len(cand) == 1 and rule != "keep":
                sole.add(cand[0])
    assert verdicts == {MR.KEEP, MR.MARGINALIZE, MR.DROP}
    assert decided == {"c1_idepth", "c1_no_residuals", "keep", "c3_few_residuals", "c3_few_good", "c4_marginalize", "c4_drop"}, decided
    assert sole == {"oob1", "oob2", "oob3", "host_flagged"}, sole  # each clause of C2 decides a point alone
    job, _, exp = MR.case("scene")
    sub_active = exp["active"][exp["sub_residuals"]]
    assert (sub_active == 1).sum() >= 10 and (sub_active == 0).sum() >= 10
    before = np.asarray(job["state_in"])[exp["sub_residuals"]]
    assert (before == R.OOB).sum() >= 3 and (before == R.OUTLIER).sum() >= 3  # residuals that resetOOB brought back
    assert (exp["new_state"][exp["sub_residuals"]][before != R.IN] == R.IN).any()
    assert (np.asarray(job["prior"])[exp["sub_points"]] != 0).sum() >= 3 and (exp["sub"]["prior"] >= 2500.0 * 360000.0).sum() >= 3
    assert len(exp["sub_points"]) == (exp["verdict"] == MR.MARGINALIZE).sum() and exp["n_res_marg"] == (sub_active == 1).sum()


@pytest.mark.parametrize("name", list(MR.SCENES))
def test_host_form_equals_checker(name):
    """5, 9, 2, 1, 3, 4 and 16 frames; one frame leaving at the first, a middle and the last position, two frames, every frame, none;
    no points, no residuals"""
    job, frames, exp = MR.case(name)
    MR.assert_equal(host_form(job, frames), exp)
    N = 4 + 8 * len(job["frame_ids"])
    Nn = N - 8 * len(job["marg_frames"])
    assert exp["H_M_out"].shape == (Nn, Nn) and (exp["H_M_out"] == exp["H_M_out"].T).all()


@pytest.mark.parametrize("marg_frames", [(), (0,), (2,), (4,), (0, 4), (1, 2), (0, 1, 2, 3, 4)], ids=str)
def test_frames_leaving_at_every_position(marg_frames):
    job, frames, exp = MR.case("scene", marg_frames=marg_frames)
    MR.assert_equal(host_form(job, frames), exp)
    assert exp["H_M_out"].shape[0] == 44 - 8 * len(marg_frames)
    if not marg_frames:
        assert exp["H_M_out"].tobytes() == exp["H_M_points"].tobytes()


def test_options():
    """H_M / b_M NULL; every optional output NULL, then some given; the parameters are read"""
    job, frames, exp = MR.case("scene", priors=False)
    assert job.get("H_M") is None
    MR.assert_equal(host_form(job, frames), exp)
    job, frames, exp = MR.case("scene")
    optional = MR.OWN[4:] + HR.STITCHED + HR.RAW + HR.PER_POINT + ("center_projected_to", "projected_to", "JpJdF")
    got = host_form(job, frames, outputs=())
    MR.assert_equal(got, exp, outputs=("verdict", "H_M_out", "b_M_out", "n_res_marg", "new_state", "new_energy", "new_energy_with_outlier"))
    assert all((np.asarray(got[k]) == MR.FILL).all() for k in optional) and (got["active"] == 77).all()
    asked = ("res_to_zero", "H_sc", "b_M_points", "hdi", "acc_E", "active")
    got = host_form(job, frames, outputs=asked)
    MR.assert_equal(got, exp, outputs=MR.OWN[:4] + asked, fills=tuple(k for k in optional if k not in asked))
    loose = MR.case("scene", marg=MR.LOOSE)[2]
    assert (loose["verdict"] == MR.MARGINALIZE).sum() > (exp["verdict"] == MR.MARGINALIZE).sum()
    for marg in (MR.LOOSE, dict(min_idepth_h_marg=100.0), dict(marg_weight_fac=0.5), dict(idepth_fix_prior_marg_fac=1.0)):
        from direct_stereo_slam_amd import marginalize

        e = MR.case("scene", marg=marg)[2]
        assert e["H_M_out"].tobytes() != exp["H_M_out"].tobytes(), marg
        MR.assert_equal(host_form(job, frames, marg_params=marginalize.default_marg_params(**marg)), e)


def test_no_point_of_verdict_one_returns_the_prior():
    """Z: the fold adds w (0 - 0): the inputs as values"""
    job, frames, exp = MR.case("two_frames", marg_frames=())
    assert not (exp["verdict"] == MR.MARGINALIZE).any() and len(exp["verdict"]) > 0
    got = host_form(job, frames)
    MR.assert_equal(got, exp)
    assert (got["H_M_out"] == job["H_M"]).all() and (got["b_M_out"] == job["b_M"]).all()


@pytest.mark.parametrize("what", ["residuals", "points"])
def test_sub_window_sizes_at_the_block_edges(what):
    """sub-windows of 0, 1, 255, 256 and 257 residuals and of 63, 64 and 65 points, as the device tests run them"""
    sizes = dict(residuals=[("nine_frames", dict(n_residuals=m)) for m in (0, 1, 255, 256, 257)],
                 points=[("wide", dict(n_points=m)) for m in (63, 64, 65)])[what]
    from direct_stereo_slam_amd import marginalize

    for base, kw in sizes:
        job, frames, exp, marg = MR.forced_case(base, **kw)
        assert len(exp["sub_residuals"]) == kw.get("n_residuals", len(exp["sub_residuals"])), (kw, len(exp["sub_residuals"]))
        assert len(exp["sub_points"]) == kw.get("n_points", len(exp["sub_points"])), (kw, len(exp["sub_points"]))
        MR.assert_equal(host_form(job, frames, marg_params=marginalize.default_marg_params(**marg)), exp)


@pytest.mark.parametrize("nf", [3, 10, 11])
def test_further_frame_counts(nf):
    """three frames with residuals (LOOSE: no point of three frames has three residuals); N = 84 and 92, as the device tests run them"""
    from direct_stereo_slam_amd import marginalize

    job, frames, exp = MR.frames_case(nf, (nf // 3,), marg=MR.LOOSE)
    assert exp["n_res_marg"] > 0
    MR.assert_equal(host_form(job, frames, marg_params=marginalize.default_marg_params(**MR.LOOSE)), exp)


def test_geometry_101_by_53():
    from direct_stereo_slam_amd import marginalize

    job, frames, exp = MR.geometry_case()
    assert exp["n_res_marg"] > 20
    MR.assert_equal(marginalize.window_marginalize_host(*R.GEOMETRY, job, frames), exp)


def test_the_returned_prior_feeds_the_next_keyframe():
    """the second keyframe: dsm_window_solve_host on the shrunken window with the returned prior equals the checker's chain"""
    import _solve_ref as SR
    from direct_stereo_slam_amd import solve

    job, frames, exp = MR.case("scene")
    nxt, stay = MR.next_keyframe(job, host_form(job, frames))
    ref, _ = MR.next_keyframe(job, exp)
    assert len(stay) == 4 and len(nxt["host"]) == (exp["verdict"] == MR.KEEP).sum() and len(nxt["point"]) > 50
    lin = R.linearize(R.W, R.H, ref, [frames[f] for f in stay])
    hes = dict(lin, **HR.hessian(ref, lin, ref))
    want = dict(hes, **SR.solve(ref, hes))
    got = solve.window_solve_host(R.W, R.H, nxt, [frames[f] for f in stay])
    SR.assert_equal(got, want, hes_outputs=HR.RAW + ("active", "JpJdF") + HR.PER_POINT, lin_outputs=("center_projected_to", "projected_to"))
    assert np.isfinite(got["x"]).all() and np.abs(got["x"]).max() > 0


def test_invalid_jobs_are_refused_before_any_output_is_written():
    from direct_stereo_slam_amd import marginalize
    from direct_stereo_slam_amd._lib import DsmError

    job, frames, exp = MR.case("scene")

    def refused(b, what, lp=None, mp=None):
        before = [{k: v.copy() for k, v in out.items()} for out in b.all_outputs()]
        with pytest.raises(DsmError):
            b.run_host(R.W, R.H, 0, frames, lp, mp)
        for out, bef in zip(b.all_outputs(), before):
            assert all(np.array_equal(out[k], bef[k]) for k in out), what

    calls = [(what, bad, {}) for what, bad in MR.invalid_jobs(job) + HR.invalid_jobs(job)] + list(R.invalid_jobs(job))
    assert len(calls) == 24 + 10 + 13
    for what, bad, kw in calls:
        refused(marginalize.MarginalizeBatch([bad]), what, marginalize.default_params(**kw))
    for kw in MR.invalid_params():
        refused(marginalize.MarginalizeBatch([job]), kw, None, marginalize.default_marg_params(**kw))
    for k in ("verdict", "H_M_out", "b_M_out", "n_res_marg"):  # a NULL required output
        b = marginalize.MarginalizeBatch([job])
        setattr(b.arr[0], k, None)
        refused(b, k)
    room = np.zeros((len(job["point"]), 74), np.float32)
    for k, ptr in (("J_out", C.POINTER(C.c_float)), ("keep", C.POINTER(C.c_ubyte)), ("rel_bs", C.POINTER(C.c_float))):  # must be NULL
        b = marginalize.MarginalizeBatch([job])
        setattr(b.arr[0].hes.lin, k, room.ctypes.data_as(ptr))
        refused(b, k)
    assert not room.any()
    MR.assert_equal(host_form(job, frames), exp)


# ---- independent of the stated orders ----------------------------------------------------------------------------------------------

# float32 roundings along the deepest term of X1: the first product of jx's first sum is rounded once as a product and by each of the
# 5 later additions of the sum (6), by the sum of the two sums (7), by the addition of Jpdd delta (8), by the product with JIdx[0][i]
# (9) and by the four subtractions of rtz[i] (13)
RTZ_ROUNDINGS = 13


@pytest.mark.parametrize("name", ["scene", "nine_frames"])
def test_res_to_zero_against_a_float64_evaluation(name):
    job, frames, exp = MR.case(name)
    nf = len(job["frame_ids"])
    sub, lin = exp["sub"], exp["sub_lin"]
    dp = np.asarray(job["ad_ht_delta"]).reshape(nf, nf, 8)
    rows = np.flatnonzero(HR.active_of(sub, lin))
    assert len(rows) > 20
    moved = 0
    for i in rows:
        p = int(sub["point"][i])
        val, mag = MR.res_to_zero_f64(lin["J"][i], dp[int(sub["host"][p]), int(sub["target"][i])], job["c_delta"], sub["delta"][p])
        got = exp["res_to_zero"][exp["sub_residuals"][i]].astype(np.float64)
        assert (np.abs(got - val) <= (RTZ_ROUNDINGS + 1) * 2.0 ** -24 * mag).all(), i
        moved += int((np.abs(got - lin["J"][i][:8]) > 1e-3).any())
    assert moved > len(rows) // 2  # X1 does something on these scenes


def fold_check(job, exp, folded_H, folded_b):
    """the entries of the fold that miss w (dense - dense_sc) from the rtz rows, by section 17's bounds (its roundings per matrix)"""
    nf = len(job["frame_ids"])
    N = 4 + 8 * nf
    m = nf - 1
    sub = exp["sub"]
    value, mag = HR.dense(sub, dict(exp["sub_lin"], J=exp["sub_rows"]), sub)
    w = 0.25
    HM, bM = np.asarray(job["H_M"]).reshape(N, N), np.asarray(job["b_M"])
    bad = {}
    for key, got, prior, a, sc, na, nsc in (("H", folded_H, HM, "H_A", "H_sc", 5, 8 + m), ("b", folded_b, bM, "b_A", "b_sc", 11, 15 + m)):
        want = prior + w * (value[a] - value[sc])
        bound = w * ((na + 1) * mag[a] + (nsc + 1) * mag[sc]) * 2.0 ** -24 + 4 * 2.0 ** -53 * (np.abs(prior) + w * (mag[a] + mag[sc]))
        if not (np.abs(got - want) <= bound).all():
            bad[key] = float((np.abs(got - want) - bound).max())
    return bad


@pytest.mark.parametrize("name", ["scene", "nine_frames"])
def test_fold_against_a_dense_float64_construction(name):
    job, frames, exp = MR.case(name)
    assert not fold_check(job, exp, exp["H_M_points"], exp["b_M_points"])
    assert np.abs(exp["H_M_points"] - job["H_M"]).max() > 1


def lu_solve_ld(A, b):
    """A x = b in numpy.longdouble: Gaussian elimination with row partial pivoting"""
    A, b = np.array(A, ld), np.array(b, ld)
    n = len(b)
    for k in range(n):
        big = k + int(np.argmax(np.abs(A[k:, k])))
        A[[k, big]], b[[k, big]] = A[[big, k]], b[[big, k]]
        mult = A[k + 1:, k] / A[k, k]
        A[k + 1:, k:] -= mult[:, None] * A[k, k:][None, :]
        b[k + 1:] -= mult * b[k]
    x = np.zeros(n, ld)
    for i in range(n - 1, -1, -1):
        x[i] = (b[i] - A[i, i + 1:] @ x[i + 1:]) / A[i, i]
    return x


def unscaled(H, b, f, prior, delta_prior):
    """the system after G1 and G2, its Schur complement onto the frames that stay and the leading part of its solution, by
    numpy.linalg.solve on the unscaled system"""
    N = len(b)
    at, nd = 4 + 8 * f, N - 8
    order = list(range(at)) + list(range(at + 8, N)) + list(range(at, at + 8))
    Hp, bp = H[np.ix_(order, order)].copy(), b[order].copy()
    Hp[range(nd, N), range(nd, N)] += prior
    bp[nd:] += prior * delta_prior
    X = np.linalg.solve(Hp[nd:, nd:], np.column_stack([Hp[nd:, :nd], bp[nd:]]))
    return Hp[:nd, :nd] - Hp[:nd, nd:] @ X[:, :nd], bp[:nd] - Hp[:nd, nd:] @ X[:, nd], np.linalg.solve(Hp, bp)[:nd]


G_SCENES = ("scene", "nine_frames", "two_frames", "sixteen_frames", "no_points")
_steps = []


def frame_steps():
    """every (scene, frame) step of the G scenes: the system before, the frame, its priors, the checker's result in float64 and in
    numpy.longdouble, and the three relative deviations between the two (H', b', the solution of H' x' = b'), each over the largest
    magnitude of its longdouble side"""
    if not _steps:
        assert np.finfo(ld).eps < 2.0 ** -60, "numpy.longdouble is no wider than float64 here: the tolerance cannot be measured"
        for name in G_SCENES:
            job, _, exp = MR.case(name)
            H, b = exp["H_M_points"], exp["b_M_points"]
            for m, f in enumerate(job["marg_frames"]):
                args = (H, b, int(f) - m, job["frame_prior"][m], job["frame_delta_prior"][m])
                H64, b64 = MR.marginalize_frame(*args)
                Hld, bld = MR.marginalize_frame(*args, xp=ld)
                x64, xld = np.linalg.solve(H64, b64), lu_solve_ld(Hld, bld)
                dev = [float(np.abs(a - c).max() / np.abs(c).max()) for a, c in ((H64, Hld), (b64, bld), (x64, xld))]
                _steps.append(dict(name=name, args=args, H=H64, b=b64, x=x64, dev=dev))
                H, b = H64, b64
    return _steps


def tolerances():
    """16 x the largest deviation seen over the steps, for H', b' and x'"""
    return [16 * max(s["dev"][i] for s in frame_steps()) for i in range(3)]


def misses(H, b, step):
    """which of H', b', x' lie outside the tolerance of numpy's unscaled evaluation of the step"""
    Hn, bn, xn = unscaled(*step["args"])
    x = np.linalg.solve(H, b)
    err = [float(np.abs(a - c).max() / np.abs(c).max()) for a, c in ((H, Hn), (b, bn), (x, xn))]
    return {k for k, e, t in zip("Hbx", err, tolerances()) if not e <= t}, err


def test_frame_marginalisation_against_the_unscaled_schur_complement():
    steps = frame_steps()
    assert len(steps) == 6 and all(t > 0 for t in tolerances())
    for s in steps:
        bad, err = misses(s["H"], s["b"], s)
        print(s["name"], "deviation from longdouble", s["dev"], "from numpy", err, "tolerances", tolerances())
        assert not bad, (s["name"], bad, err, tolerances())
        assert np.linalg.eigvalsh(s["H"]).min() > 0  # the priors are symmetric positive definite, and stay so


def test_the_bounds_have_teeth():
    job, frames, exp = MR.case("scene")
    step = next(s for s in frame_steps() if s["name"] == "scene")  # frame 1 of 5: a middle frame
    for drop, what in ((("G2",), "bx"), (("bli_T",), "Hbx"), (("perm",), "Hbx")):
        H, b = MR.marginalize_frame(*step["args"], drop=drop)
        bad, err = misses(H, b, step)
        assert bad >= set(what), (drop, bad, err)
    i = int(np.flatnonzero(exp["sub_hes"]["active"])[5])  # one residual of the sub-window dropped from the accumulation
    mutant = MR.marginalize(R.W, R.H, job, frames, drop=(("residual", i),))
    assert set(fold_check(job, exp, mutant["H_M_points"], mutant["b_M_points"])) == {"H", "b"}
    bad, err = misses(mutant["H_M_out"], mutant["b_M_out"], step)
    assert bad == set("Hbx"), (bad, err)
