"""The first half of a Levenberg-Marquardt round on the device -- reduce_partials_groups / _groups2 / _final, build_rs, build_H_elem,
build_b_elem, lm_step_wave0, end_level, begin_level, finish_track: one production step per problem on constructed states and partials
(dsm_diag_lm_step) -- against the reference of tests/_lm_machine_ref.py, which tests/test_lm_machine_ref.py pins to the oracle.

  A  every row of the case table x {plain, coherent} x {helper off, on}: every output field bit for bit (a NaN compared as a NaN)
  B  the reduction alone at every chunk count, main and speculative partials
  C  one step that consumes a speculative candidate equals two plain steps, on the device
  D  a walk over the four levels of the mini4 pyramid, compared after every step
  E  argument errors
and the rows that stage an evaluation or give a verdict once more under a nonzero reference affine and unequal exposures.

Exact except: (1) the candidate pose of a step that proposes goes through the device's sincos: compared as test E of
tests/test_lm_step.py compares it (same bounds), and M, t of its staged evaluation are recomputed from the DEVICE's candidate, bit for
bit; (2) finish_track's logf decides a verdict only: the rows stand 1e-4 off the threshold.  last_residuals -- a sqrtf of a float -- is
compared bit for bit: the library is built without flags that relax it (csrc/Makefile: -O3 -ffp-contract=off, no fast-math)."""
import ctypes as C
import time

import numpy as np
import pytest

import _lm_machine_cases as Cs
import _lm_machine_ref as M
import _lm_step_ref as R
from _scenes import SIZES
from direct_stereo_slam_amd import synth as S

SIZE = "mini4"
DELTA = 4 * R.EPS  # as tests/test_lm_step.py
SCALARS_I = ("status", "lvl", "phase", "iteration", "have_repeated", "coarsest", "spec_valid", "ticks")
SCALARS_F = ("lam", "level_cutoff_repeat", "inc_f", "spec_inc_f", "scale_cur", "scale_cand", "spec_scale_cand", "Hs", "bs")
ARRAYS = ("H", "b", "cur", "aff_cur", "cand", "aff_cand", "spec_cand", "spec_aff_cand", "res_old", "min_res", "last_residuals", "last_inners", "flow",
          "evals", "evals_ro", "rounds")
SCALARS_D = ("inc_norm", "spec_inc_norm")
EV_FIELDS = ("M", "t", "aff0", "aff1", "cutoff", "max_energy", "residual_only", "scale")


def level_K():
    return S.level_K(S.kitti_K_work(), SIZES[SIZE][2])


@pytest.fixture(scope="module")
def trackers(ctx):
    from direct_stereo_slam_amd.tracker import TrackerAndScaler, default_params

    made = {}

    def get(pkey):
        if pkey not in made:
            rp, p = Cs.ref_params(pkey), default_params()
            for f in ("huber_th", "coarse_cutoff_th", "scale_xi_rot", "scale_xi_trans", "scale_a", "scale_b", "affine_opt_mode_a",
                      "affine_opt_mode_b", "lambda_extrapolation_limit", "fixed_schedule"):
                setattr(p, f, getattr(rp, f))
            for i in range(6):
                p.max_iterations[i] = rp.max_iterations[i]
            w, h, _, nl = SIZES[SIZE]
            assert nl == Cs.NLEVELS
            trk = TrackerAndScaler(ctx, w, h, nl, S.KITTI_T_STEREO, level_K(), p)
            trk.makeK(*level_K())
            made[pkey] = trk
        return made[pkey]

    yield get
    for t in made.values():
        t.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# records <-> reference states
# ---------------------------------------------------------------------------------------------------------------------------------
def pack(states, nchs):
    from direct_stereo_slam_amd.tracker import LM_STEP_STATE

    arr = np.zeros(len(states), LM_STEP_STATE)
    for a, st, nch in zip(arr, states, nchs):
        for k in SCALARS_I + SCALARS_F + SCALARS_D:
            a[k] = st[k]
        for k in ARRAYS:
            a[k] = np.asarray(st[k]).reshape(-1)
        a["nch"] = nch
        for blk in ("ev", "spec_ev"):
            for k in EV_FIELDS:
                a[blk][k] = st[blk][k]
    return arr


def unpack(rec):
    st = {k: int(rec[k]) for k in SCALARS_I}
    st.update({k: np.float32(rec[k]) for k in SCALARS_F})
    st.update({k: np.float64(rec[k]) for k in SCALARS_D})
    st.update({k: np.array(rec[k]) for k in ARRAYS})
    st["H"] = st["H"].reshape(8, 8)
    for blk in ("ev", "spec_ev"):
        e = rec[blk]
        st[blk] = dict(M=np.array(e["M"]), t=np.array(e["t"]), aff0=np.float32(e["aff0"]), aff1=np.float32(e["aff1"]), cutoff=np.float32(e["cutoff"]),
                       max_energy=np.float32(e["max_energy"]), residual_only=int(e["residual_only"]), scale=np.float32(e["scale"]))
    return st


def partial_block(cases, spec_block):
    """float32 [n, stride] and spec_off: every case's main partials, its speculative ones spec_off floats behind"""
    top = max(max(c["nch"] for c in cases), 1) * 64
    stride, spec_off = (2 * top, top) if spec_block else (top, 0)
    P = np.zeros((len(cases), stride), np.float32)
    P.view(np.uint32)[:] = 0x7FC00456  # what no chunk covers is never read: NaN patterns
    for row, c in zip(P, cases):
        row[:c["nch"] * 64] = c["part"].reshape(-1)
        if spec_block and c["spec_part"] is not None:
            row[spec_off:spec_off + c["nch"] * 64] = c["spec_part"].reshape(-1)
    return P, spec_off


def run_device(trk, mode, lvl, cases, spec_block, helper=False, coherent=False):
    P, spec_off = partial_block(cases, spec_block)
    return trk.diagLmStep(mode, lvl, pack([c["state"] for c in cases], [c["nch"] for c in cases]), P, spec=spec_block, spec_off=spec_off, helper=helper,
                          coherent=coherent)


_KI = {}


def level_Ki(trackers):
    """K^-1 of every level as the device holds it (float; the same for every parameter set): read off a step's staged evaluation,
    checked against makeK's K"""
    if not _KI:
        trk = trackers(("ab", 0, None))
        for lvl in range(Cs.NLEVELS):
            c = dict(state=M.new_state(lvl), nch=0, part=np.zeros((0, 64), np.float32), spec_part=None)
            rec = run_device(trk, 0, lvl, [c], False)[0]
            assert rec["lvl"] == lvl and rec["status"] == M.ST_RUNNING
            Ki = np.array(rec["ev"]["Ki"])
            K = S.level_K(level_K(), lvl)
            np.testing.assert_allclose(Ki.reshape(3, 3), np.linalg.inv(np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1.0]])), rtol=1e-6, atol=1e-9)
            _KI[lvl] = Ki
    return _KI


# ---------------------------------------------------------------------------------------------------------------------------------
# the comparison
# ---------------------------------------------------------------------------------------------------------------------------------
def bits_equal(a, b):
    a = np.asarray(a)
    b = np.asarray(b, a.dtype)
    if a.dtype.kind == "f":
        return R.same_bits(a, b, nan_as_nan=True)
    return bool(np.array_equal(a, b))


def check_candidate(mode, got, want, inc_scaled, Ki, ev, what):
    """the candidate pose of a proposal as tests/test_lm_step.py's test E bounds it, and M, t of its evaluation from the DEVICE's pose"""
    bad = []
    theta = float(np.sqrt(inc_scaled[3] * inc_scaled[3] + inc_scaled[4] * inc_scaled[4] + inc_scaled[5] * inc_scaled[5]))
    ups = float(np.linalg.norm(inc_scaled[:3]))
    if not np.all(np.isfinite(want)) or theta < 1e-10:
        if not R.same_bits(got, want, nan_as_nan=True):
            bad.append(what + " (exact)")
    else:
        dq, dt = float(np.abs(got[:4] - want[:4]).max()), float(np.abs(got[4:] - want[4:]).max())
        t_bound = 8 * DELTA * (1 + 1 / theta) * ups + 8 * R.EPS * float(np.linalg.norm(want[4:]))
        if not dq <= 8 * DELTA or not dt <= t_bound:
            bad.append(f"{what}: |dq| {dq:.3g} (bound {8 * DELTA:.3g}), |dt| {dt:.3g} (bound {t_bound:.3g})")
    if mode != 1 and np.all(np.isfinite(got)):
        Mx, t = R.eval_rot(mode, got, Ki)
        if not (R.same_bits(np.array(ev["M"]), Mx) and R.same_bits(np.array(ev["t"]), t)):
            bad.append(what + ": M, t of the staged evaluation")
    return bad


def compare(mode, inp, got, want, Ki):
    """got: the device's state (unpacked), want: the reference's.  Returns the names of the fields that differ."""
    bad = []
    proposed = want["status"] == M.ST_RUNNING and want["phase"] == M.PH_ITER
    twin = proposed and (not bits_equal(want["spec_inc_norm"], inp["spec_inc_norm"]) or not bits_equal(want["spec_inc_f"], inp["spec_inc_f"]) or
                         not bits_equal(want["spec_cand"], inp["spec_cand"]))
    handed = want["status"] == M.ST_RUNNING and want["phase"] == M.PH_INIT and bits_equal(want["iteration"], 0) and \
        (want["lvl"] != inp["lvl"] or want["have_repeated"] != inp["have_repeated"])
    inc = want.get("_inc_scaled", {})
    for k in SCALARS_I + SCALARS_F + SCALARS_D + ARRAYS:
        if mode != 1 and ((k == "cand" and proposed) or (k == "spec_cand" and twin)):
            continue
        if not bits_equal(got[k], want[k]):
            bad.append(k)
    for blk, pre, staged in (("ev", "", proposed), ("spec_ev", "spec_", twin)):
        for k in EV_FIELDS:
            if mode == 1 and k in ("M", "t", "aff0", "aff1"):
                continue  # (the scale problem's are the level's: R10 K^-1, tsl, (1, 0))
            if mode != 1 and k in ("M", "t") and (staged or (handed and blk == "ev")):
                continue  # (below, from the device's own pose)
            if not bits_equal(got[blk][k], want[blk][k]):
                bad.append(blk + "." + k)
        if mode != 1 and staged and pre in inc:
            bad += check_candidate(mode, got[pre + "cand"], want[pre + "cand"], inc[pre], Ki[want["lvl"]], got[blk], pre + "cand")
    if mode != 1 and handed:  # the level's first evaluation stands at the current pose: exact
        Mx, t = R.eval_rot(mode, got["cur"], Ki[want["lvl"]])
        if not (R.same_bits(got["ev"]["M"], Mx) and R.same_bits(got["ev"]["t"], t)):
            bad.append("ev.M, ev.t at the handed-down pose")
    return bad


def check_group(trk, Ki, mode, lvl, cases, spec_block, helper, coherent, info_kw=None):
    out = run_device(trk, mode, lvl, cases, spec_block, helper, coherent)
    bad = []
    for c, rec in zip(cases, out):
        want, _, _ = Cs.run_reference(c, Ki=Ki, info_kw=info_kw)
        got = unpack(rec)
        assert rec["nch"] == c["nch"]
        if want["status"] == M.ST_RUNNING:
            assert np.array_equal(np.array(rec["ev"]["Ki"]), Ki[want["lvl"]]) and np.array_equal(np.array(rec["spec_ev"]["Ki"]), Ki[want["lvl"]]), c["row"]
        diff = compare(mode, c["state"], got, want, Ki)
        if diff:
            k = diff[0]
            bad.append((c["row"], mode, diff, (got.get(k), want.get(k)) if k in want else None))
    return bad


def grouped(cases):
    groups = {}
    for c in cases:
        groups.setdefault((c["pkey"], c["mode"], c["lvl"], c["spec_block"]), []).append(c)
    return groups


# ---------------------------------------------------------------------------------------------------------------------------------
# A  the table
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("helper", (0, 1))
@pytest.mark.parametrize("coherent", (0, 1))
def test_every_row_bit_for_bit(trackers, coherent, helper):
    t0 = time.perf_counter()
    bad, n = [], 0
    for (pkey, mode, lvl, spec_block), cases in grouped(Cs.cases()).items():
        trk = trackers(pkey)
        bad += check_group(trk, level_Ki(trackers), mode, lvl, cases, spec_block, bool(helper), bool(coherent))
        n += len(cases)
    print(f"\ncoherent {coherent} helper {helper}: {n} cases, {len(bad)} differ, {time.perf_counter() - t0:.2f} s")
    assert n == len(Cs.cases()) and not bad, (len(bad), bad[:6])


@pytest.mark.gpu
def test_reference_affine_and_exposures(trackers, ctx):
    """The rows that stage an evaluation or give a verdict, on a tracker whose keyframe has a nonzero affine pair and whose frames have
    different exposure times: affLL = fromToVecExposure(...) of every staged evaluation and the relative affine of the verdict carry
    the exposure ratio and the reference's b.  Pose problems (the loop-closure estimator's reference is (0, 0) by construction)."""
    from direct_stereo_slam_amd.tracker import TrackerAndScaler

    photo = dict(ref_a=-0.3, ref_b=12.0, ref_exposure=0.8, exposure=1.3)
    Ki = level_Ki(trackers)
    w, h, _, nl = SIZES[SIZE]
    seen = set()
    for mode_name in ("ab", "prior", "fix_ab"):
        pkey = (mode_name, 0, None)
        trk = TrackerAndScaler(ctx, w, h, nl, S.KITTI_T_STEREO, level_K(), trackers(pkey).params)
        trk.makeK(*level_K())
        trk.setCoarseTrackingRef(0, (photo["ref_a"], photo["ref_b"]), photo["ref_exposure"], *[[np.zeros(0, np.float32)] * nl] * 4)  # (no template)
        trk.upload_intensity(0, [np.zeros((h >> l, w >> l), np.float32) for l in range(nl)], photo["exposure"])
        cases = [c for c in Cs.cases() if c["pkey"] == pkey and c["mode"] == 0 and c["row"].split("/")[0] in ("verdict", "end", "init", "spec")]
        assert cases
        for (_, mode, lvl, spec_block), group in grouped(cases).items():
            bad = check_group(trk, Ki, mode, lvl, group, spec_block, True, False, info_kw=photo)
            assert not bad, (mode_name, len(bad), bad[:4])
            for c in group:
                out = Cs.run_reference(c, Ki=Ki, info_kw=photo)[0]
                plain = Cs.run_reference(c, Ki=Ki)[0]
                seen.add(out["status"])
                if out["status"] == M.ST_RUNNING:  # the photometry does reach the staged evaluation
                    assert not bits_equal(out["ev"]["aff0"], plain["ev"]["aff0"]) or bits_equal(out["ev"]["aff0"], c["state"]["ev"]["aff0"]), c["row"]
        trk.close()
    assert {M.ST_RUNNING, M.ST_GOOD, M.ST_BAD_AFFINE, M.ST_ABORTED} <= seen


# ---------------------------------------------------------------------------------------------------------------------------------
# B  the reduction alone
# ---------------------------------------------------------------------------------------------------------------------------------
def reduction_case(params, mode, nch, seed, spec):
    """plain: PH_INIT without a repeat -- the step takes rs, H, b (Hs, bs) of the main partials.  spec: PH_ITER, the main evaluation
    rejected and the speculative one accepted -- the step takes them from the speculative partials (both go through the two-at-a-time
    reduction)."""
    rng = np.random.default_rng(9000 + seed)
    n_terms = int(rng.integers(nch, 4096 * nch + 1))
    ints = (n_terms, int(rng.integers(0, n_terms // 2 + 1)), int(rng.integers(0, 4096 * nch + 1)))
    part = Cs.gen_cancelling(7000 + seed, nch, ints)  # (the order of the additions shows in the float results)
    part[:, M.SLOT_E] += np.float32(1e4)  # (an energy the saturated terms' n_sat x max_energy does not swamp: a quarter of it is clearly less)
    st =Cs.base_state(params, mode, 1, M.PH_ITER if spec else M.PH_INIT, seed)
    c = dict(row=f"reduction nch {nch}", mode=mode, pkey=("ab", 0, None), lvl=1, state=st, nch=nch, part=part, spec_block=spec, spec_part=None)
    if spec:
        Cs.steer(st, Cs.evaluation(params, part, nch, st["ev"]["max_energy"])["rs"], "worse")
        sp = Cs.gen_cancelling(8000 + seed, nch, ints)
        sp[:, M.SLOT_E] = part[:, M.SLOT_E] * np.float32(0.25)
        c["spec_part"], st["spec_valid"] = sp, 1
    return c


@pytest.mark.gpu
@pytest.mark.parametrize("mode", (0, 1, 2))
def test_reduction_at_every_chunk_count(trackers, mode):
    pkey = ("ab", 0, None)
    params, trk = Cs.ref_params(pkey), trackers(pkey)
    Ki = level_Ki(trackers)
    for spec, counts in ((False, Cs.PLAIN_CHUNKS), (True, Cs.SPEC_CHUNKS), (True, Cs.PLAIN_CHUNKS[1:])):
        cases = [reduction_case(params, mode, nch, 10 * k + mode, spec) for k, nch in enumerate(counts)]
        if spec:  # the main partials through the two-at-a-time reduction as well: a PH_INIT step beside them
            cases += [dict(reduction_case(params, mode, nch, 500 + 10 * k + mode, False), spec_block=True) for k, nch in enumerate(counts)]
        for coherent in (False, True):
            out = run_device(trk, mode, 1, cases, spec, helper=True, coherent=coherent)
            for c, rec in zip(cases, out):
                src = c["spec_part"] if c["state"]["phase"] == M.PH_ITER else c["part"]
                e = Cs.evaluation(params, src, c["nch"], c["state"]["ev"]["max_energy"])
                w = (mode, spec, coherent, c["nch"], c["state"]["phase"])
                assert R.same_bits(np.array(rec["res_old"]), e["rs"], nan_as_nan=True), (w, rec["res_old"], e["rs"])
                if mode == 1:
                    assert R.same_bits(np.float32(rec["Hs"]), e["Hs"], nan_as_nan=True) and R.same_bits(np.float32(rec["bs"]), e["bs"], nan_as_nan=True), w
                else:
                    assert R.same_bits(np.array(rec["H"]).reshape(8, 8), e["H"], nan_as_nan=True), w
                    assert R.same_bits(np.array(rec["b"]), e["b"], nan_as_nan=True), w
                assert not compare(mode, c["state"], unpack(rec), Cs.run_reference(c, Ki=Ki)[0], Ki), w


# ---------------------------------------------------------------------------------------------------------------------------------
# C  speculation is scheduling only, on the device
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", (0, 1, 2))
def test_one_speculative_step_equals_two_plain_steps(trackers, mode):
    """Step 1, plain, on the case's state: the device rejects the main candidate and proposes the next one.  That proposal IS the
    speculative candidate a scheduler with a speculative block would have staged a step earlier: the case's state with it as the twin,
    stepped once with both evaluations, must equal step 1's output stepped plainly on the twin's evaluation -- every field but rounds
    and ticks (one more), the speculative block, and the candidate block where the level has ended (dead: _lm_machine_cases.dead_fields)."""
    n_pairs = 0
    for (pkey, m, lvl, _), cases in grouped([c for c in Cs.spec_cases() if c["mode"] == mode]).items():
        trk = trackers(pkey)
        plain = [dict(c, spec_block=False) for c in cases]
        out1 = [unpack(r) for r in run_device(trk, m, lvl, plain, False, helper=True)]
        twinned = []
        for c, o1 in zip(cases, out1):
            st = dict(c["state"])
            for k in ("cand", "aff_cand", "inc_norm", "scale_cand", "inc_f"):
                st["spec_" + k] = o1[k]
            st["spec_ev"] = o1["ev"]
            twinned.append(dict(c, state=st))
        one = [unpack(r) for r in run_device(trk, m, lvl, twinned, True, helper=True)]
        went_on = [o1["status"] == M.ST_RUNNING and o1["phase"] == M.PH_ITER and o1["lvl"] == lvl and o1["iteration"] == c["state"]["iteration"] + 1
                   and R.same_bits(o1["res_old"], c["state"]["res_old"]) for c, o1 in zip(cases, out1)]  # (rejected: res_old as it was)
        second = [dict(c, state=o1, part=c["spec_part"], spec_block=False) for c, o1, g in zip(cases, out1, went_on) if g]
        out2 = iter([unpack(r) for r in run_device(trk, m, lvl, second, False, helper=True)] if second else [])
        for c, o1, s, g in zip(cases, out1, one, went_on):
            two = next(out2) if g else o1
            consumed = s["evals"][lvl] - c["state"]["evals"][lvl] == 2
            assert consumed == g, c["row"]
            bad = Cs.state_diff(s, two, skip=Cs.SCHEDULING_ONLY + Cs.SPEC_BLOCK_FIELDS + Cs.dead_fields(s, lvl))
            assert not bad, (c["row"], mode, bad)
            assert two["rounds"][lvl] - s["rounds"][lvl] == int(g) and two["ticks"] - s["ticks"] == int(g), c["row"]
            n_pairs += int(g)
    assert n_pairs >= 4


# ---------------------------------------------------------------------------------------------------------------------------------
# D  a walk over four levels
# ---------------------------------------------------------------------------------------------------------------------------------
def walk_partials(st, mode, step, twin):
    """the next evaluation of the walk's script, steered through the partials: a level's first evaluation saturated once on the
    coarsest level (the cut-off repeat, later the level repeat); then a rejection, two accepted gentle steps and an accepted step whose
    system makes the NEXT proposal small, which ends the level.  A twin is accepted on even steps."""
    n_terms, n_warped = 400, 404
    old = float(st["res_old"][0] / st["res_old"][1]) if st["res_old"][1] > 0 else 10.0
    if st["phase"] == M.PH_INIT:
        if st["lvl"] == Cs.NLEVELS - 1 and float(st["level_cutoff_repeat"]) == 1 and not st["have_repeated"]:
            return Cs.gen_partials(100 + step, 2, (10, 9, 12))
        P = Cs.gen_partials(100 + step, 2, (n_terms, 0, n_warped), e_exact=np.float32(4000.0 + 100 * st["lvl"]))
        Cs.gentle_system(P)
        return P
    accept = (step % 2 == 0) if twin else st["iteration"] >= 1
    P = Cs.gen_partials(100 + step, 1 + step % 3, (n_terms, 0, n_warped), e_exact=np.float32(old * n_terms * (0.9 if accept else 1.1)))
    if st["iteration"] >= 3:
        Cs.dominant_diagonal(P)
    else:
        Cs.gentle_system(P)
        P[0, :45] *= np.float32(1.0 + 0.01 * step)
    return P


@pytest.mark.gpu
def test_walk_over_four_levels(trackers):
    pkey = ("ab", 0, None)
    params, trk = Cs.ref_params(pkey), trackers(pkey)
    Ki = level_Ki(trackers)
    t0 = time.perf_counter()
    for mode, spec_block in ((0, True), (1, True), (2, False)):
        st = M.new_state(Cs.NLEVELS - 1)
        st["cur"], st["aff_cur"], st["scale_cur"] = Cs.CUR.copy(), Cs.AFF.copy(), np.float32(1.3)
        M.begin_level(params, M.tracker_info(mode, Ki=Ki), st, Cs.NLEVELS - 1)
        seen = set()
        for step in range(80):
            if st["status"] != M.ST_RUNNING:
                break
            lvl = st["lvl"]
            part = walk_partials(st, mode, step, False)
            spec_part = walk_partials(st, mode, step, True) if spec_block and st["spec_valid"] else None
            c = dict(row=f"walk mode {mode} step {step}", mode=mode, pkey=pkey, lvl=lvl, state=st, nch=len(part), part=part, spec_block=spec_block,
                     spec_part=spec_part)
            want, _, _ = Cs.run_reference(c, Ki=Ki)
            got = unpack(run_device(trk, mode, lvl, [c], spec_block, helper=True)[0])
            diff = compare(mode, st, got, want, Ki)
            assert not diff, (c["row"], lvl, diff)
            d = got["evals"][lvl] - st["evals"][lvl]
            seen |= {"cut-off repeat"} if got["phase"] == M.PH_INIT and float(got["level_cutoff_repeat"]) > 1 else set()
            seen |= {"level repeat"} if got["have_repeated"] and not st["have_repeated"] else set()
            seen |= {"rejection"} if st["phase"] == M.PH_ITER and R.same_bits(got["res_old"], st["res_old"]) else set()
            seen |= {"twin consumed"} if d == 2 else set()
            seen |= {f"level {got['lvl']}"} if got["lvl"] != lvl else set()
            st = got  # the device's state feeds the next step (and the reference's next step)
        assert st["status"] == M.ST_GOOD, (mode, st["status"], step)
        assert {"cut-off repeat", "level repeat", "rejection", "level 2", "level 1", "level 0"} <= seen, (mode, seen)
        assert ("twin consumed" in seen) == spec_block, (mode, seen)
        assert 15 <= step <= 60, step
        assert not np.isnan(st["last_residuals"][:Cs.NLEVELS]).any() and st["rounds"].sum() == step
    print(f"\nwalk: {time.perf_counter() - t0:.2f} s")


# ---------------------------------------------------------------------------------------------------------------------------------
# E  argument errors
# ---------------------------------------------------------------------------------------------------------------------------------
def _call(L, handle, mode, lvl, n, arr_in, parts, stride, spec, spec_off, arr_out):
    from direct_stereo_slam_amd._lib import LmStepState, c_float_p

    return L.dsm_diag_lm_step(handle, mode, lvl, n, None if arr_in is None else arr_in.ctypes.data_as(C.POINTER(LmStepState)),
                              None if parts is None else parts.ctypes.data_as(c_float_p), stride, spec, spec_off, 0, 0,
                              None if arr_out is None else arr_out.ctypes.data_as(C.POINTER(LmStepState)))


def _error_case():
    from direct_stereo_slam_amd.tracker import LM_STEP_STATE

    st = M.new_state(1)
    arr = pack([st, st], [2, 2])
    parts = np.zeros((2, 256), np.float32)
    out = np.zeros(2, LM_STEP_STATE)
    out.view(np.uint8)[:] = 0xA5
    return arr, parts, out


def test_null_tracker_is_invalid(built):
    from direct_stereo_slam_amd import _lib

    L = _lib.load()
    arr, parts, out = _error_case()
    assert _call(L, None, 0, 1, 2, arr, parts, 256, 0, 0, out) == -1  # DSM_ERR_INVALID
    assert b"dsm_diag_lm_step" in L.dsm_last_error()
    assert np.all(out.view(np.uint8) == 0xA5)


@pytest.mark.gpu
def test_invalid_arguments(trackers, ctx):
    from direct_stereo_slam_amd.tracker import TrackerAndScaler

    trk = trackers(("ab", 0, None))
    L, nl = trk.L, SIZES[SIZE][3]
    arr, parts, out = _error_case()

    def edited(field, value):
        a = arr.copy()
        a[field][1] = value
        return a

    for args in ((trk.h, 0, 1, 0, arr, parts, 256, 0, 0), (trk.h, 0, 1, -3, arr, parts, 256, 0, 0), (trk.h, 0, 1, 65537, arr, parts, 256, 0, 0),
                 (trk.h, 3, 1, 2, arr, parts, 256, 0, 0), (trk.h, -1, 1, 2, arr, parts, 256, 0, 0), (trk.h, 0, -1, 2, arr, parts, 256, 0, 0),
                 (trk.h, 0, nl, 2, arr, parts, 256, 0, 0), (trk.h, 0, 1, 2, None, parts, 256, 0, 0), (trk.h, 0, 1, 2, arr, None, 256, 0, 0),
                 (None, 0, 1, 2, arr, parts, 256, 0, 0),
                 (trk.h, 0, 1, 2, arr, parts, 64, 0, 0),      # two chunks do not fit 64 floats
                 (trk.h, 0, 1, 2, arr, parts, 254, 0, 0),     # not a multiple of 4
                 (trk.h, 0, 1, 2, arr, parts, 0, 0, 0),
                 (trk.h, 0, 1, 2, arr, parts, 256, 1, 64),    # the main partials run into the speculative ones
                 (trk.h, 0, 1, 2, arr, parts, 256, 1, 192),   # the speculative ones run out of the block
                 (trk.h, 0, 1, 2, arr, parts, 256, 1, 126),   # not a multiple of 4
                 (trk.h, 0, 1, 2, arr, parts, 256, 1, -128),
                 (trk.h, 0, 1, 2, edited("nch", -1), parts, 256, 0, 0), (trk.h, 0, 1, 2, edited("nch", 4097), parts, 256, 0, 0),
                 (trk.h, 0, 1, 2, edited("phase", 2), parts, 256, 0, 0)):
        assert _call(L, *args, out) == -1, args[1:4] + args[6:]
        assert np.all(out.view(np.uint8) == 0xA5), args[1:4] + args[6:]
    assert _call(L, trk.h, 0, 1, 2, arr, parts, 256, 0, 0, None) == -1
    w, h, _, nl = SIZES[SIZE]
    fresh = TrackerAndScaler(ctx, w, h, nl, S.KITTI_T_STEREO, level_K())  # no makeK yet: no K^-1 to read
    assert _call(L, fresh.h, 0, 1, 2, arr, parts, 256, 0, 0, out) == -1 and np.all(out.view(np.uint8) == 0xA5)
    fresh.close()
    assert _call(L, trk.h, 0, 1, 2, arr, parts, 256, 1, 128, out) == 0 and not np.all(out.view(np.uint8) == 0xA5)  # and good arguments run
