"""CPU: the reference of the LM state machine (tests/_lm_machine_ref.py) and its case table (tests/_lm_machine_cases.py) stand on their
own, before the device is compared with them (tests/test_lm_machine.py).

  A  decide_ref, driven with the compiled oracle's own evaluations over whole runs, returns orc_track's / orc_optimize_scale's result
     bit for bit: pose, affine, flag, last residuals, flow indicators, per-level evaluation counts -- with and without a speculative
     block
  B  speculation is scheduling only: a step that consumes a speculative candidate equals two plain steps but for rounds / ticks
  C  the reduction order matters for the chosen data
  D  every row of the case table is reached by the reference alone, with the counters each row states
  E  a speculative evaluation that is not valid is never looked at
"""
import collections
import copy

import numpy as np
import pytest

import _lm_machine_cases as Cs
import _lm_machine_ref as M
import _lm_step_ref as R
from _scenes import make_scene, oracle_tracker
from direct_stereo_slam_amd import synth as S
from oracle import oracle as O


# ---------------------------------------------------------------------------------------------------------------------------------
# A  against the compiled oracle
# ---------------------------------------------------------------------------------------------------------------------------------
def drive(orc, params, mode, coarsest, pose=None, aff=None, scale=1.0, min_res=None, spec_block=False):
    """the loop of trackNewestCoarse / optimizeScale as decide_ref steps around the ORACLE's evaluations"""
    info = M.tracker_info(mode, 0.0, 0.0, 1.0, 1.0)
    st = M.new_state(coarsest)
    if mode == 0:
        st["cur"], st["aff_cur"] = np.array(pose, np.float64), np.array(aff, np.float64)
    st["scale_cur"] = np.float32(scale)
    if min_res is not None:
        st["min_res"] = np.array(min_res, np.float64)
    M.begin_level(params, info, st, coarsest)

    def evaluate(pre):
        lvl, ev = st["lvl"], st["spec_ev" if pre else "ev"]
        if mode == 1:
            s = float(st["scale_cur"] if st["phase"] == M.PH_INIT else st[pre + "scale_cand"])
            rs = orc.calc_res_scale(lvl, s, float(ev["cutoff"]))
            Hs, bs = orc.calc_gs_scale(lvl, s)
            return dict(rs=rs, Hs=Hs, bs=bs)
        p, a = (st["cur"], st["aff_cur"]) if st["phase"] == M.PH_INIT else (st[pre + "cand"], st[pre + "aff_cand"])
        rs = orc.calc_res_pose(lvl, p, a, float(ev["cutoff"]))
        H, b = orc.calc_gs_pose(lvl, p, a)
        return dict(rs=rs, H=H, b=b)

    steps = 0
    while st["status"] == M.ST_RUNNING:
        main = evaluate("")
        spec = evaluate("spec_") if spec_block and st["spec_valid"] else None
        st = M.decide_ref(params, info, st, main, spec, spec_block=spec_block)
        steps += 1
        assert steps < 2000
    return st


RUNS = [("tiny", 11, dict(), m, None) for m in R.MODES] + [("small", 3, dict(), m, None) for m in R.MODES] + [
    ("small", 10, dict(b=60.0), "ab", None),          # test_cutoff_repeat_and_level_repeat's scene
    ("small", 5, dict(), "ab", np.full(6, 1e-3)),     # test_track_abort_and_affine_checks': the abort ...
    ("small", 6, dict(b=240.0), "ab", None),          # ... and the implausible affine result
]


@pytest.mark.parametrize("spec_block", (False, True))
@pytest.mark.parametrize("size,seed,kw,mode_name,min_res", RUNS)
def test_decide_ref_is_the_oracles_loop(built, size, seed, kw, mode_name, min_res, spec_block):
    sc = make_scene(size, seed=seed, **kw)
    params = O.default_params()
    params.affine_opt_mode_a, params.affine_opt_mode_b = R.MODES[mode_name]
    orc = oracle_tracker(sc, params)
    # ---- trackNewestCoarse ----
    st = drive(orc, params, 0, sc.nl - 1, S.IDENTITY_POSE, [0.0, 0.0], min_res=min_res, spec_block=spec_block)
    good, pose, aff, last, flow = orc.track(S.IDENTITY_POSE, [0.0, 0.0], sc.nl - 1, min_res)
    assert (st["status"] == M.ST_GOOD) == good
    assert R.same_bits(st["last_residuals"], last, nan_as_nan=True), (st["last_residuals"], last)
    assert R.same_bits(st["flow"], flow)
    assert list(st["evals"])[:sc.nl] == orc.eval_counts()[0][:sc.nl]
    if st["status"] != M.ST_ABORTED:  # (an aborted call leaves the caller's pose alone: :598 returns before :612)
        assert R.same_bits(st["cur"], pose) and R.same_bits(st["aff_cur"], aff), (st["cur"], pose, st["aff_cur"], aff)
    else:
        assert min_res is not None and np.isnan(st["last_residuals"][0])
    if kw.get("b") == 60.0:
        assert st["have_repeated"] == 1  # the scene does reach the cut-off repeat and the level repeat
    if spec_block:  # fewer rounds than evaluations: candidates were consumed in pairs
        assert st["rounds"].sum() < st["evals"].sum()
    else:
        assert st["rounds"].sum() == st["evals"].sum()
    # ---- optimizeScale ----
    ss = drive(orc, params, 1, sc.nl - 1, scale=1.0, spec_block=spec_block)
    err, s = orc.optimize_scale(1.0, sc.nl - 1)
    assert ss["status"] == M.ST_GOOD
    assert R.same_bits(np.float32(ss["scale_cur"]), np.float32(s))
    assert R.same_bits(np.float32(ss["last_residuals"][0]), np.float32(err), nan_as_nan=True)
    assert list(ss["evals"])[:sc.nl] == orc.eval_counts()[0][:sc.nl]


# ---------------------------------------------------------------------------------------------------------------------------------
# B  speculation is scheduling only
# ---------------------------------------------------------------------------------------------------------------------------------
def with_consistent_twin(params, info, case):
    """the case's state with the speculative candidate the loop itself would propose after rejecting the main one (what a scheduler with
    a speculative block staged a step earlier), and the plain loop's state after that rejection"""
    st = copy.deepcopy(case["state"])
    twin = copy.deepcopy(st)
    twin["lam"] = M.lambda_after(params, st["lam"], False)
    twin["iteration"] = st["iteration"] + 1
    M.propose(params, info, twin, twin["lam"], False)
    for k in ("cand", "aff_cand", "inc_norm", "scale_cand", "inc_f"):
        st["spec_" + k] = copy.deepcopy(twin[k])
    st["spec_ev"] = copy.deepcopy(twin["ev"])
    return st


def test_speculation_is_scheduling_only(built):
    n_pairs = 0
    for c in Cs.spec_cases():
        params, info = Cs.ref_params(c["pkey"]), M.tracker_info(c["mode"])
        st = with_consistent_twin(params, info, c)
        main = Cs.evaluation(params, c["part"], c["nch"], st["ev"]["max_energy"])
        spec = Cs.evaluation(params, c["spec_part"], c["nch"], st["spec_ev"]["max_energy"])
        one = M.decide_ref(params, info, st, main, spec, spec_block=True)
        two = M.decide_ref(params, info, st, main, None, spec_block=False)
        consumed = one["evals"][c["lvl"]] - st["evals"][c["lvl"]] == 2
        if consumed:
            assert two["status"] == M.ST_RUNNING and two["phase"] == M.PH_ITER and two["lvl"] == c["lvl"], c["row"]
            assert not Cs.state_diff(two, st, skip=Cs.SCHEDULING_ONLY + ("lam", "iteration", "evals", "evals_ro", "cand", "aff_cand", "inc_norm", "scale_cand",
                                                                      "inc_f", "ev", "_inc_scaled", "spec_valid")), c["row"]  # the rejection changed nothing else
            assert not Cs.state_diff(dict(cand=two["cand"], aff_cand=two["aff_cand"], inc_norm=two["inc_norm"], scale_cand=two["scale_cand"], inc_f=two["inc_f"], ev=two["ev"]),
                                    dict(cand=st["spec_cand"], aff_cand=st["spec_aff_cand"], inc_norm=st["spec_inc_norm"], scale_cand=st["spec_scale_cand"],
                                         inc_f=st["spec_inc_f"], ev=st["spec_ev"])), c["row"]
            two = M.decide_ref(params, info, two, spec, None, spec_block=False)
            n_pairs += 1
        bad = Cs.state_diff(one, two, skip=Cs.SCHEDULING_ONLY + Cs.SPEC_BLOCK_FIELDS + Cs.dead_fields(one, c["lvl"]))
        assert not bad, (c["row"], c["mode"], bad)
        lvl = c["lvl"]
        assert two["rounds"][lvl] - one["rounds"][lvl] == (1 if consumed else 0) and two["ticks"] - one["ticks"] == (1 if consumed else 0), c["row"]
    assert n_pairs >= 12


# ---------------------------------------------------------------------------------------------------------------------------------
# C  the reduction order matters
# ---------------------------------------------------------------------------------------------------------------------------------
def reduction_sets():
    out = []
    for k, nch in enumerate(Cs.PLAIN_CHUNKS + Cs.SPEC_CHUNKS):
        rng = np.random.default_rng(77 + k)
        ints = tuple(int(rng.integers(0, 4096 * nch + 1)) for _ in range(3))
        out.append((nch, Cs.gen_cancelling(500 + k, nch, ints), ints))
    return out


def plain_order_sum(P, nch):
    s = np.zeros(M.SLOT_NTERMS)
    for c in range(nch):
        s = s + P[c, :M.SLOT_NTERMS].astype(np.float64)
    return s


def visible(params, sums, isums):
    """what a step can show of the 49 float sums: rs, H, b, Hs, bs -- every one a FLOAT of a sum before anything else happens to it"""
    e = M.system_ref(params, sums, isums, 0.0)
    return np.concatenate([e["rs"], e["H"].reshape(-1), e["b"], [np.float64(e["Hs"]), np.float64(e["bs"])]])


def test_reduction_order_matters_for_the_chosen_data(built):
    """Another order of the additions changes the bits of what the step RETURNS (not only of the float64 sums, whose last bits the
    cast to float drops): the plain chunk order beyond 19 chunks, two swapped groups, two swapped chunks inside a group."""
    params = O.default_params()
    for nch, P, ints in reduction_sets():
        sums, isums = M.reduce_ref(P, nch)
        assert tuple(int(v) for v in isums) == ints
        assert int(P.view(np.int32)[:, M.SLOT_NTERMS:M.NUM_SLOTS].max(initial=0)) <= 4096
        np.testing.assert_allclose(sums, plain_order_sum(P, nch), rtol=0, atol=1e-7)  # (the same sums up to the roundings at 1e-10)
        right = visible(params, sums, isums)
        if nch > M.GROUPS:  # (up to 19 chunks every group holds one chunk: the documented order IS the plain one)
            assert not R.same_bits(right, visible(params, plain_order_sum(P, nch), isums), nan_as_nan=True), nch
        else:
            assert R.same_bits(sums, plain_order_sum(P, nch)), nch
        if nch >= 18:
            order = list(range(M.GROUPS))
            order[0], order[7] = order[7], order[0]
            swapped, iswapped = M.reduce_ref(P, nch, group_order=order)
            assert not R.same_bits(right, visible(params, swapped, isums), nan_as_nan=True), nch
            assert np.array_equal(isums, iswapped)
            reverse = M.reduce_ref(P, nch, group_order=order[::-1])[0]
            assert not R.same_bits(right, visible(params, reverse, isums), nan_as_nan=True), nch
        if nch >= 3 * M.GROUPS:  # inside a group: chunks g + 19, g + 38, g instead of g, g + 19, g + 38 (two chunks commute)
            walk = list(range(M.GROUPS, 3 * M.GROUPS)) + list(range(M.GROUPS)) + list(range(3 * M.GROUPS, nch))
            assert not R.same_bits(right, visible(params, M.reduce_ref(P, nch, order=walk)[0], isums), nan_as_nan=True), nch
    # the partials span about 12 decades with mixed signs
    P = reduction_sets()[-1][1][:, :45]
    assert np.log10(np.abs(P).max() / np.abs(P).min()) > 11 and (P > 0).any() and (P < 0).any()


# ---------------------------------------------------------------------------------------------------------------------------------
# D  every row is reached
# ---------------------------------------------------------------------------------------------------------------------------------
ROWS = {  # row -> cases (the modes it applies to)
    "init/ratio 3/5 repeats": 3, "init/ratio 599/1000 takes the system": 3, "init/ratio 601/1000 repeats": 3,
    "init/repeat at 32 doubles to 64": 3, "init/no repeat at 64": 3, "init/fixed schedule never repeats": 3,
    "init/no iterations: the level ends at once": 3, "init/no terms: 0/0 ratio": 3, "init/n_warped mod 4": 12, "init/n_warped 0": 2,
    "iter/strictly better: accepted": 3, "iter/exactly equal: rejected": 3, "iter/worse: rejected": 3, "iter/NaN new ratio: rejected": 3,
    "iter/NaN old ratio: rejected": 3, "iter/fixed schedule: always accepted, never small": 3,
    "iter/lambda floor: 4 lambda below the limit": 3, "iter/lambda floor: 4 lambda at the limit": 3, "iter/lambda floor: 4 lambda above the limit": 3,
    "iter/iteration + 1 below the bound": 3, "iter/iteration + 1 at the bound": 3, "iter/iteration + 1 above the bound": 3,
    "iter/inc_norm at 1e-3": 2, "iter/inc_norm above": 2, "iter/inc_norm NaN": 2,
    "iter/scale inc_f negative and large: small (signed)": 1, "iter/scale inc_f at 1e-3f": 1, "iter/scale inc_f above": 1, "iter/scale inc_f well above": 1,
    "spec/main accepted: twin ignored, not counted": 3, "spec/main rejected, twin accepted": 3, "spec/main rejected, twin exactly equal: rejected": 3,
    "spec/both rejected: two lambda updates": 3,
    "spec/both rejected: each update floored": 3, "spec/twin small": 3, "spec/bound reached by the twin": 3,
    "spec/main small while spec_valid: twin not consumed": 3, "spec/spec_valid 0: NaN partials behind": 3,
    "spec/want_spec: iteration + 1 below the bound": 3, "spec/want_spec: iteration + 1 at the bound": 3, "spec/evals_ro from the main evaluation": 3,
    "spec/init stages a twin": 3, "spec/fixed schedule stages none": 3, "spec/spec_valid 0 after a small main proposal": 3,
    "spec/spec_valid 1 after a main proposal that is not small": 3,
    "end/E/n = 9, min_res 2: not aborted": 3, "end/E/n = 9, min_res just under 2: aborted (pose)": 3, "end/E/n = 9, min_res NaN: no limit": 3,
    "end/fixed schedule never aborts": 3, "end/level repeat taken once": 3, "end/level repeat not a second time": 3,
    "end/hand-down after an accepted step": 3, "end/hand-down from the coarsest level": 3, "end/scale from level 0: good": 1,
    "verdict/ab: |log rel_a| below 1.5": 2, "verdict/ab: |log rel_a| above 1.5": 2, "verdict/ab: |log rel_a| above 1.5, negative": 2,
    "verdict/ab: |rel_b| below 200": 2, "verdict/ab: |rel_b| above 200": 2, "verdict/prior: |a| below 1.2": 2, "verdict/prior: |a| above 1.2": 2,
    "verdict/prior: |b| below 200": 2, "verdict/prior: |b| above 200": 2, "verdict/fix_ab: negative modes zero the pair": 2,
    "verdict/fix_ab: negative modes: |a| above 1.2": 2, "verdict/fix_a: a zeroed, b kept": 2, "verdict/fix_b: b zeroed, a kept": 2,
}


def test_every_row_is_reached_by_the_reference(built):
    reached, missed = collections.Counter(), []
    for c in Cs.cases():
        out, _, _ = Cs.run_reference(c)
        i, lvl = c["state"], c["lvl"]
        ok = bool(c["expect"](i, out))
        ok &= out["evals"][lvl] - i["evals"][lvl] == c["d_evals"] and out["evals_ro"][lvl] - i["evals_ro"][lvl] == c["d_ro"]
        ok &= out["rounds"][lvl] - i["rounds"][lvl] == 1 and out["ticks"] - i["ticks"] == 1
        ok &= all(out[k][l] == i[k][l] for k in ("evals", "evals_ro", "rounds") for l in range(M.MAX_LEVELS) if l != lvl)
        if ok:
            reached[c["row"]] += 1
        else:
            missed.append((c["row"], c["mode"]))
    assert not missed, missed
    assert dict(reached) == ROWS, sorted(set(ROWS) ^ set(reached)) + [r for r in ROWS if reached.get(r) != ROWS[r]]
    assert {c["mode"] for c in Cs.cases()} == {0, 1, 2}


# ---------------------------------------------------------------------------------------------------------------------------------
# E  an invalid speculative evaluation is never looked at
# ---------------------------------------------------------------------------------------------------------------------------------
def test_invalid_speculative_evaluation_is_ignored(built):
    n = 0
    for c in Cs.cases():
        if not c["spec_block"] or c["state"]["spec_valid"]:
            continue
        assert np.isnan(c["spec_part"][:, :49]).all(), c["row"]  # NaN patterns behind the main partials
        params, info = Cs.ref_params(c["pkey"]), M.tracker_info(c["mode"])
        main = Cs.evaluation(params, c["part"], c["nch"], c["state"]["ev"]["max_energy"])
        with_nan = M.decide_ref(params, info, c["state"], main, Cs.evaluation(params, c["spec_part"], c["nch"], 0.0), spec_block=True)
        with_finite = M.decide_ref(params, info, c["state"], main, main, spec_block=True)
        assert not Cs.state_diff(with_nan, with_finite), c["row"]
        n += 1
    assert n >= 20
