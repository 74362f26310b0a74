"""CPU: the checker of the Hessian and Schur accumulation (tests/_hessian_ref.py) reaches every branch on the
shared scenes; dsm_window_hessian_host equals it bit for bit on every output; and, independently of the stated order, every
accumulator entry lies within the bound of a sequential double sum of math.fsum of its float terms, and the stitched matrices agree
with a dense float64 construction from the rows within a bound formed from the same construction on absolute values."""
import math

import numpy as np
import pytest

import _hessian_ref as HR
import _linearize_ref as R

NAMES = list(HR.CASES) + ["clamp", "wide"]


def host_form(job, frames, **kw):
    from direct_stereo_slam_amd import hessian

    return hessian.window_hessian_host(R.W, R.H, job, frames, **kw)


def test_the_scenes_reach_every_branch():
    seen = dict(pair0=0, pair1=0, point0=0, straddle=0, lin=0, prior=0)
    for name in ("scene", "nine_frames"):
        job, _, exp = HR.case(name)
        nf = len(job["frame_ids"])
        on = exp["active"].astype(bool)
        pair = np.asarray(job["host"])[job["point"]] * nf + job["target"]
        counts = np.bincount(pair[on], minlength=nf * nf).reshape(nf, nf)
        off_diagonal = ~np.eye(nf, dtype=bool)
        seen["pair0"] += int((counts[off_diagonal] == 0).sum())
        seen["pair1"] += int((counts == 1).sum())
        for p in range(len(job["host"])):
            rs = np.flatnonzero(np.asarray(job["point"]) == p)
            a = on[rs]
            seen["point0"] += int(len(rs) > 0 and not a.any())
            inner = [i for i in range(1, len(rs) - 1) if not a[i] and exp["new_state"][rs[i]] in (R.OOB, R.OUTLIER) and a[:i].any() and a[i + 1:].any()]
            seen["straddle"] += int(bool(inner))
            if a.any():
                seen["lin"] += int(job["hdd_lin"][p] != 0 and job["bd_lin"][p] != 0)
                seen["prior"] += int(job["prior"][p] != 0 and job["delta"][p] != 0)
    assert all(v >= 3 for v in seen.values()), seen
    assert HR.case("scene")[0]["shift_prior_to_zero"] == 1 and HR.case("nine_frames")[0]["shift_prior_to_zero"] == 0
    job, _, exp = HR.case("clamp")  # the points of frame 0 see a zero translation: Jpdd = 0 and H falls under 1e-10
    on = exp["active"].astype(bool)
    rows = exp["J"][on & (np.asarray(job["host"])[job["point"]] == 0)]
    assert len(rows) >= 3 and (rows[:, HR.PDD:HR.PDD + 2] == 0).all()
    clamped = (exp["idepth_hessian"] == np.float32(1e-10)) & (exp["hdi"] == np.float32(1.0 / float(np.float32(1e-10))))
    assert clamped.sum() >= 3 and (exp["idepth_hessian"] > 1).sum() >= 3
    job, _, exp = HR.case("wide")  # what the chunk sizes of the device kernels ask for
    on = exp["active"].astype(bool)
    assert np.bincount(np.asarray(job["target"])[on]).max() > 32 and np.bincount(job["host"]).min() > 64 and len(job["host"]) > 128


@pytest.mark.parametrize("name", NAMES)
def test_host_form_equals_checker(name):
    job, frames, exp = HR.case(name)
    HR.assert_equal(host_form(job, frames), exp)
    N = 4 + 8 * len(job["frame_ids"])
    assert exp["H_A"].shape == (N, N) and (exp["H_A"] == exp["H_A"].T).all() and (exp["H_sc"] == exp["H_sc"].T).all()
    if len(job["point"]) == 0:
        assert all(not np.asarray(exp[k]).any() for k in HR.STITCHED + HR.RAW)
    else:  # acc_D[h][t1][t2] is the transpose of acc_D[h][t2][t1], bit for bit
        assert exp["acc_D"].tobytes() == np.ascontiguousarray(exp["acc_D"].transpose(0, 2, 1, 4, 3)).tobytes()


def test_host_form_options():
    """shift_prior_to_zero off and on, optional inputs NULL, optional outputs NULL, J_out given, fix_linearization off"""
    job, frames, exp = HR.case("scene")
    lin = {k: exp[k] for k in ("new_state", "J")}
    for variant in (dict(shift_prior_to_zero=0), dict(prior=None, delta=None), dict(hdd_lin=None, bd_lin=None, hcd_lin=None), dict(fix_linearization=0)):
        sub = dict(job, **variant)
        e = dict(R.assemble(sub, R.case("scene")[3], None), **HR.hessian(sub, lin, sub))
        HR.assert_equal(host_form(sub, frames), e)
    assert HR.hessian(dict(job, shift_prior_to_zero=0), lin, dict(job, shift_prior_to_zero=0))["b_sc"].tobytes() != exp["b_sc"].tobytes()
    got = host_form(job, frames, outputs=())
    HR.assert_equal(got, exp, outputs=(), lin_outputs=())
    assert all((np.asarray(got[k]) == (77 if k == "active" else -7)).all() for k in HR.RAW + ("active", "JpJdF") + HR.PER_POINT)
    got = host_form(job, frames, outputs=("J", "acc_D", "hdi"))
    HR.assert_equal(got, exp, outputs=("acc_D", "hdi"), lin_outputs=("J",))
    assert (got["J"][~exp["defined"]] == -7).all() and (got["acc_top"] == -7).all()


def fsum_entries(terms, shape):
    """(math.fsum, sum of magnitudes, count) of every entry over its list of float terms"""
    S = np.stack([t.astype(np.float64) for t in terms]).reshape(len(terms), -1)
    exact = np.array([math.fsum(S[:, i]) for i in range(S.shape[1])]).reshape(shape)
    return exact, np.abs(S).sum(axis=0).reshape(shape), len(terms)


@pytest.mark.parametrize("name", ["scene", "nine_frames"])
def test_accumulators_against_exact_sums(name):
    """a sequential double sum of K terms is within (K - 1) 2^-53 sum|term| of the exact sum, whatever the order"""
    job, frames, exp = HR.case(name, terms=True)
    checked = 0
    for key in HR.RAW:
        for at, terms in exp["terms"][key].items():
            got = exp[key][at]
            exact, mag, K = fsum_entries(terms, got.shape)
            assert (np.abs(got - exact) <= (K - 1) * 2.0 ** -53 * mag).all(), (key, at)
            checked += got.size
    assert checked > 5000


# float32 roundings along the deepest path of a term (m: the most active residuals a point can have, n_frames - 1):
#   H_A   5: ((x_a y_b) + (y_a x_b)) J01 is 3, the two sums of A3 make 5
#   b_A  11: JI_r is 8 products and 8 sums (9), x_a JI_r (10), the sum of A3 (11)
#   H_sc  8 + m: v0 (2), v0 Jpdd (3), its sum (4), the m sums of S1, hdd_lin, prior, the reciprocal (7 + m); JpJdF is 4, the product
#         of two 5, with hdi 8 + m
#   b_sc 15 + m: JI_r (9), JI_r Jpdd (10), its sum (11), the m sums of S1, bd_lin, prior delta (13 + m), hdi bd_sum (14 + m), JpJdF (...) 15 + m
# The double sums of P1, S3 and T1 add roundings of 2^-53, which the "+ 1" holds many times over.
def roundings(nf):
    m = nf - 1
    return dict(H_A=5, b_A=11, H_sc=8 + m, b_sc=15 + m)


def dense_check(job, exp, lin):
    value, mag = HR.dense(job, lin, job)
    nf = len(job["frame_ids"])
    bad = {}
    for k, n in roundings(nf).items():
        err, bound = np.abs(exp[k] - value[k]), mag[k] * (n + 1) * 2.0 ** -24
        if not (err <= bound).all():
            bad[k] = float((err - bound).max())
    return bad


@pytest.mark.parametrize("name", ["scene", "nine_frames", "clamp"])
def test_stitched_matrices_against_a_dense_float64_construction(name):
    job, frames, exp = HR.case(name)
    assert not dense_check(job, exp, exp)
    assert np.abs(exp["H_A"]).max() > 1 and np.abs(exp["H_sc"]).max() > 0


def test_the_bounds_have_teeth():
    job, frames, exp = HR.case("scene")
    nf = len(job["frame_ids"])
    ad = [np.asarray(job[k]).reshape(nf, nf, 8, 8) for k in ("ad_host", "ad_target")]
    r = int(np.flatnonzero(exp["active"])[5])
    dropped = HR.hessian(job, exp, job, drop=(r,))  # a dropped residual
    bad = dense_check(job, dropped, exp)
    assert "H_A" in bad and "b_A" in bad and "H_sc" in bad and "b_sc" in bad, bad
    acc = {k: exp[k] for k in HR.RAW}
    swapped = dict(acc, acc_top=np.ascontiguousarray(exp["acc_top"].transpose(1, 0, 2, 3)), acc_E=np.ascontiguousarray(exp["acc_E"].transpose(1, 0, 2, 3)),
                   acc_EB=np.ascontiguousarray(exp["acc_EB"].transpose(1, 0, 2)))  # host and target index swapped
    bad = dense_check(job, HR.stitch(nf, *ad, swapped), exp)
    assert "H_A" in bad and "b_A" in bad and "H_sc" in bad and "b_sc" in bad, bad
    h, t1, t2 = next((h, a, b) for h in range(nf) for a in range(nf) for b in range(nf) if a != b and exp["acc_D"][h, a, b].any())
    D = exp["acc_D"].copy()
    D[h, t1, t2] = D[h, t1, t2].T.copy()  # one block of acc_D transposed
    bad = dense_check(job, HR.stitch(nf, *ad, dict(acc, acc_D=D)), exp)
    assert "H_sc" in bad and "H_A" not in bad, bad


def test_invalid_jobs_are_refused_before_any_output_is_written():
    from direct_stereo_slam_amd import hessian
    from direct_stereo_slam_amd._lib import DsmError

    job, frames, exp = HR.case("scene")
    calls = [(what, bad, {}) for what, bad in HR.invalid_jobs(job)] + list(R.invalid_jobs(job))
    assert len(calls) == 23
    for what, bad, kw in calls:
        b = hessian.HessianBatch([bad])
        before = [{k: v.copy() for k, v in out.items()} for out in b.all_outputs()]
        with pytest.raises(DsmError):
            b.run_host(R.W, R.H, 0, frames, hessian.default_params(**kw))
        for out, bef in zip(b.all_outputs(), before):
            assert all(np.array_equal(out[k], bef[k]) for k in out), what
    for k in HR.STITCHED:  # a NULL required output
        b = hessian.HessianBatch([job])
        setattr(b.arr[0], k, None)
        with pytest.raises(DsmError):
            b.run_host(R.W, R.H, 0, frames)
        assert (b.outs[0][0]["acc_top"] == -7).all() and (b.lin.outs[0][0]["new_state"] == 77).all(), k
    HR.assert_equal(host_form(job, frames), exp)
