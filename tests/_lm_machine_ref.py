"""Host reference of the first half of a Levenberg-Marquardt round -- the fixed-order reduction of an evaluation's chunk partials, their
conversion into rs, H and b, and the state machine that consumes them -- for tests/test_lm_machine_ref.py (CPU) and
tests/test_lm_machine.py (device).  CPU only; plain Python / numpy.

Written from the rules, not from the device code: DESIGN.md section 4 (the reduction order, the casts) and the reference's loops --
trackNewestCoarse (TrackerAndScaler.cpp:451-638), calcResPose's Vec6 (:843-851), calcGSSSEPose's scaling (:681-696), optimizeScale
(:854-964, calcGSSSEScale :1003-1004), PoseEstimator::estimate's verdict (PoseEstimator.cpp:459-477) -- cut at the point where a loop
waits for an evaluation: one call of decide_ref is what the loop does between receiving one evaluation's result and asking for the next.
test_lm_machine_ref.py pins it to the compiled oracle's whole runs bit for bit.

  reduce_ref   the 52 slot sums of an evaluation's chunk partials in the documented order
  system_ref   the sums as rs, H, b (Hs, bs) with the reference's float / double casts
  decide_ref   one step of the loop; the proposals it stages are _lm_step_ref.step_oracle / scale_step_ref
"""
import copy
import math

import numpy as np

import _lm_step_ref as R

F32 = np.float32
F64 = np.float64
MAX_LEVELS = 6
PH_INIT, PH_ITER = 0, 1
ST_RUNNING, ST_GOOD, ST_ABORTED, ST_BAD_AFFINE = 1, 2, 3, 4
GROUPS = 19  # group g adds chunks g, g + 19, g + 38, ... in ascending order; the groups are then added 0 .. 18
NUM_SLOTS, PARTIAL_STRIDE = 52, 64
SLOT_E, SLOT_FLOW_T, SLOT_FLOW_RT, SLOT_FLOW_NUM, SLOT_NTERMS, SLOT_NSAT, SLOT_NWARPED = 45, 46, 47, 48, 49, 50, 51


# ---------------------------------------------------------------------------------------------------------------------------------
# 1  the reduction
# ---------------------------------------------------------------------------------------------------------------------------------
def reduce_ref(partials, nch, order=None, group_order=None):
    """partials: float32 [>= nch, 64] (slots 49-51 hold integer bit patterns).  Returns (sums float64[49], isums int64[3]).
    order / group_order: test hooks -- another order of the chunks inside the groups' walk (None: the documented one) and of the
    final addition of the groups (None: 0 .. 18)."""
    P = np.ascontiguousarray(partials, np.float32).reshape(-1, PARTIAL_STRIDE)[:nch]
    Pd = P[:, :SLOT_NTERMS].astype(np.float64)
    Pi = P[:, SLOT_NTERMS:NUM_SLOTS].view(np.int32).astype(np.int64)
    chunks = list(range(nch)) if order is None else list(order)
    psum = np.zeros((GROUPS, SLOT_NTERMS))
    pisum = np.zeros((GROUPS, 3), np.int64)
    with np.errstate(all="ignore"):
        for pos, c in enumerate(chunks):  # (position pos of the walk belongs to group pos mod 19; ascending inside a group)
            g = pos % GROUPS
            psum[g] = psum[g] + Pd[c]
            pisum[g] = pisum[g] + Pi[c]
        gs = list(range(GROUPS)) if group_order is None else list(group_order)
        sums = psum[gs[0]].copy()
        for g in gs[1:]:
            sums = sums + psum[g]
    return sums, pisum.sum(axis=0)


def tri_idx(r, c):
    """(r, c), r <= c, in the row-major upper triangle of the 9 x 9 accumulator"""
    return r * 9 - (r * (r - 1)) // 2 + (c - r)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2  sums -> rs, H, b
# ---------------------------------------------------------------------------------------------------------------------------------
def _i32(v):
    return int(np.int64(v).astype(np.int32))


def system_ref(params, sums, isums, max_energy):
    """rs of calcResPose / calcResScale (:843-851; E, the flow sums and the ratio are floats there), H_out / b_out of calcGSSSEPose
    (:681-696: float accumulator entries widened, times the FLOAT 1.0f / n with n the warped count padded to a multiple of 4
    (:824-835), then the column's and the row's SCALE_*), H / b of calcGSSSEScale (:1003-1004: float times float).  The E slot holds
    the usable lanes' energy; every saturated residual adds the evaluation's max_energy (:800 / :809)."""
    with np.errstate(all="ignore"):
        E = F32(F64(sums[SLOT_E]) + F64(F32(max_energy)) * F64(int(isums[1])))
        sT, sRT, sN = F32(sums[SLOT_FLOW_T]), F32(sums[SLOT_FLOW_RT]), F32(sums[SLOT_FLOW_NUM])
        n_terms, n_sat, n_warped = _i32(isums[0]), _i32(isums[1]), _i32(isums[2])
        rs = np.zeros(6)
        rs[0] = F64(E)
        rs[1] = n_terms
        rs[2] = F64(sT) / (F64(sN) + 0.1)
        rs[3] = 0
        rs[4] = F64(sRT) / (F64(sN) + 0.1)
        rs[5] = F64(F32(n_sat) / F32(n_terms))
        n4 = (n_warped + 3) & ~3
        invn = F32(1.0) / F32(n4)
        sc = R.scales_of(params)
        H, b = np.zeros((8, 8)), np.zeros(8)
        for r in range(8):
            for c in range(8):
                hf = F32(sums[tri_idx(min(r, c), max(r, c))])
                H[r, c] = ((F64(hf) * F64(invn)) * sc[c]) * sc[r]
            b[r] = (F64(F32(sums[tri_idx(r, 8)])) * F64(invn)) * sc[r]
        Hs, bs = F32(sums[0]) * invn, F32(sums[1]) * invn
    return dict(rs=rs, H=H, b=b, Hs=F32(Hs), bs=F32(bs), n4=n4)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3  the state machine
# ---------------------------------------------------------------------------------------------------------------------------------
def new_eval():
    return dict(M=np.zeros(9, F32), t=np.zeros(3, F32), aff0=F32(0), aff1=F32(0), cutoff=F32(0), max_energy=F32(0), residual_only=0,
                scale=F32(1))


def new_state(lvl, coarsest=None):
    """a problem standing at the start of `lvl` with nothing evaluated yet (every field of dsm_lm_step_state the machine reads or writes)"""
    nan6 = np.full(MAX_LEVELS, np.nan)
    return dict(status=ST_RUNNING, lvl=lvl, phase=PH_INIT, iteration=0, have_repeated=0, coarsest=lvl if coarsest is None else coarsest,
                spec_valid=0, ticks=0, lam=F32(0.01), level_cutoff_repeat=F32(1),
                H=np.zeros((8, 8)), b=np.zeros(8), cur=np.array([0, 0, 0, 1.0, 0, 0, 0]), aff_cur=np.zeros(2), cand=np.zeros(7), aff_cand=np.zeros(2),
                spec_cand=np.zeros(7), spec_aff_cand=np.zeros(2), inc_norm=F64(0), spec_inc_norm=F64(0), res_old=np.zeros(6),
                min_res=nan6.copy(), last_residuals=nan6.copy(), last_inners=np.zeros(MAX_LEVELS), flow=np.full(3, 1000.0),
                evals=np.zeros(MAX_LEVELS, np.int64), evals_ro=np.zeros(MAX_LEVELS, np.int64), rounds=np.zeros(MAX_LEVELS, np.int64),
                inc_f=F32(0), spec_inc_f=F32(0), scale_cur=F32(1), scale_cand=F32(0), spec_scale_cand=F32(0), Hs=F32(0), bs=F32(0),
                ev=new_eval(), spec_ev=new_eval())


def tracker_info(mode, ref_a=0.0, ref_b=0.0, ref_exposure=0.0, exposure=0.0, Ki=None):
    """what the machine reads of the tracker: the problem kind, the reference affine and the two exposures (the loop-closure
    estimator's reference affine is (0, 0): PoseEstimator.cpp:317), and -- only to report M of a staged evaluation -- K^-1 per level"""
    return dict(mode=mode, ref_a=float(ref_a), ref_b=float(ref_b), ref_exposure=F32(ref_exposure), exposure=F32(exposure), Ki=Ki)


def aff_from_to(info, aff, for_eval):
    """AffLight::fromToVecExposure(lastRef->ab_exposure, new_frame_->ab_exposure, lastRef_aff_g2l, aff) (:647-649, :717-720): doubles"""
    exp_f, exp_t = float(info["ref_exposure"]), float(info["exposure"])
    if exp_f == 0 or exp_t == 0:
        exp_f = exp_t = 1.0
    ra, rb = (0.0, 0.0) if (for_eval and info["mode"] == 2) else (info["ref_a"], info["ref_b"])
    try:
        e = math.exp(float(aff[0]) - ra)  # (the C library's exp, as the oracle's)
    except OverflowError:
        e = math.inf
    with np.errstate(all="ignore"):
        a = F64(e) * exp_t / exp_f
        return a, F64(aff[1]) - a * rb


def _stage_pose(info, ev, pose, aff, lvl):
    """M, t, affLL of an evaluation at (pose, aff) (:715-720)"""
    if info["Ki"] is not None:
        ev["M"], ev["t"] = R.eval_rot(info["mode"], pose, info["Ki"][lvl])
    else:
        ev["t"] = np.asarray(pose[4:7], np.float64).astype(F32)
    a, b = aff_from_to(info, aff, True)
    with np.errstate(all="ignore"):
        ev["aff0"], ev["aff1"] = F32(a), F32(b)


def _stage_cutoff(params, ev, level_cutoff_repeat, residual_only):
    ev["cutoff"], ev["max_energy"] = R.cutoff_of(params, level_cutoff_repeat)  # :726-728 / :1030-1032
    ev["residual_only"] = int(residual_only)


def propose(params, info, st, lam, spec):
    """the first half of a loop iteration (:505-554 / :897-913) at lambda `lam`: the candidate and its evaluation, staged as the main
    or as the speculative one (the speculative one is consumed an iteration later: its bound is tested at iteration + 2)"""
    lvl, pre = st["lvl"], "spec_" if spec else ""
    ev = st["spec_ev" if spec else "ev"]
    if info["mode"] == 1:
        inc, cand, last, cutoff, max_energy = R.scale_step_ref(params, lvl, st["Hs"], st["bs"], st["scale_cur"], lam, st["iteration"],
                                                               st["level_cutoff_repeat"], spec=spec)
        st[pre + "inc_f"], st[pre + "scale_cand"] = inc, cand
        ev["scale"] = cand
        ev["cutoff"], ev["max_energy"], ev["residual_only"] = cutoff, max_energy, last
    else:
        r = R.step_oracle(params, info["mode"], lvl, st["H"], st["b"], lam, st["cur"], st["aff_cur"], st["iteration"],
                          st["level_cutoff_repeat"], spec=spec)
        st[pre + "cand"], st[pre + "aff_cand"], st[pre + "inc_norm"] = r["cand"], r["aff_cand"], F64(r["inc_norm"])
        _stage_pose(info, ev, r["cand"], r["aff_cand"], lvl)
        ev["cutoff"], ev["max_energy"], ev["residual_only"] = r["cutoff"], r["max_energy"], r["residual_only"]
        st.setdefault("_inc_scaled", {})[pre] = r["inc_scaled"]  # (for the tests' bound on the device's SE3 update; not state)
    if not spec:
        st["phase"] = PH_ITER


def _is_small(info, st, pre):
    """:588 |inc| after extrapolation; :937 the scale loop's test is SIGNED (a large negative increment ends the loop)"""
    return not (float(st[pre + "inc_f"]) > 1e-3) if info["mode"] == 1 else not (float(st[pre + "inc_norm"]) > 1e-3)


def lambda_after(params, lam, accept):
    lim = F32(params.lambda_extrapolation_limit)
    if accept:
        return F32(F32(lam) * F32(0.5))  # :581 / :930
    l4 = F32(F32(lam) * F32(4))  # :583-585 / :932-934
    return lim if l4 < lim else l4


def _consume(params, info, st, e, pre, fixed, max_it):
    """the second half of a loop iteration (:556-590 / :913-939) on the evaluation `e` of the candidate st[pre + ...]: accept or
    reject, lambda, the iteration count.  Returns (accepted, the loop ends)."""
    lvl = st["lvl"]
    ev = st["spec_ev" if pre else "ev"]
    with np.errstate(all="ignore"):
        accept = fixed or bool(F64(e["rs"][0]) / F64(e["rs"][1]) < F64(st["res_old"][0]) / F64(st["res_old"][1]))  # :559 / :915
    small = (not fixed) and _is_small(info, st, pre)
    st["evals"][lvl] += 1
    st["evals_ro"][lvl] += int(ev["residual_only"])
    if accept:
        st["res_old"] = np.array(e["rs"], np.float64)
        if info["mode"] == 1:
            st["Hs"], st["bs"], st["scale_cur"] = F32(e["Hs"]), F32(e["bs"]), F32(st[pre + "scale_cand"])
        else:
            st["H"], st["b"] = np.array(e["H"], np.float64).reshape(8, 8), np.array(e["b"], np.float64)
            st["cur"], st["aff_cur"] = np.array(st[pre + "cand"]), np.array(st[pre + "aff_cand"])
    st["lam"] = lambda_after(params, st["lam"], accept)
    st["iteration"] += 1
    return accept, small or st["iteration"] >= max_it


def _finish_track(params, info, st):
    """:612-637 / PoseEstimator.cpp:463-477: the affine plausibility verdict"""
    modeA, modeB = float(params.affine_opt_mode_a), float(params.affine_opt_mode_b)
    with np.errstate(all="ignore"):
        a, b = F32(st["aff_cur"][0]), F32(st["aff_cur"][1])
        good = not ((modeA != 0 and float(np.abs(a)) > 1.2) or (modeB != 0 and float(np.abs(b)) > 200))
        if good:
            ra, rb = aff_from_to(info, st["aff_cur"], False)
            rel0, rel1 = F32(ra), F32(rb)
            if (modeA == 0 and float(np.abs(np.log(rel0))) > 1.5) or (modeB == 0 and float(np.abs(rel1)) > 200):
                good = False
    if good:
        if modeA < 0:
            st["aff_cur"][0] = 0.0
        if modeB < 0:
            st["aff_cur"][1] = 0.0
    st["status"] = ST_GOOD if good else ST_BAD_AFFINE


def begin_level(params, info, st, lvl):
    st["lvl"], st["phase"], st["iteration"], st["level_cutoff_repeat"], st["spec_valid"] = lvl, PH_INIT, 0, F32(1), 0
    if info["mode"] == 1:
        st["ev"]["scale"] = F32(st["scale_cur"])
        st["spec_ev"]["scale"] = F32(1)  # (a level begins with the speculative block holding the level's constants alone)
    else:
        _stage_pose(info, st["ev"], st["cur"], st["aff_cur"], lvl)  # :475
    _stage_cutoff(params, st["ev"], st["level_cutoff_repeat"], False)


def _end_level(params, info, st, fixed):
    """:596-604 / :945-950, then the next level or the verdict"""
    lvl = st["lvl"]
    with np.errstate(all="ignore"):
        st["last_residuals"][lvl] = F64(np.sqrt(F32(F64(st["res_old"][0]) / F64(st["res_old"][1]))))
    st["last_inners"][lvl] = st["res_old"][1]  # PoseEstimator.cpp:463
    if info["mode"] == 0:
        st["flow"] = np.array([st["res_old"][2], st["res_old"][3], st["res_old"][4]])  # :597
        if not fixed and st["last_residuals"][lvl] > 1.5 * st["min_res"][lvl]:  # :598 (NaN: no limit)
            st["status"] = ST_ABORTED
            return
    nxt = lvl - 1
    if float(st["level_cutoff_repeat"]) > 1 and not st["have_repeated"]:  # :601-604: the level once more, once per call
        nxt, st["have_repeated"] = lvl, 1
    if nxt < 0:
        if info["mode"] == 1:
            st["status"] = ST_GOOD
        else:
            _finish_track(params, info, st)
        return
    begin_level(params, info, st, nxt)


def decide_ref(params, info, state, main, spec=None, spec_block=False):
    """One step: `main` = dict(rs, H, b, Hs, bs) of the pending (main) evaluation, `spec` the same of the speculative evaluation
    (looked at only where state['spec_valid'] and spec_block).  spec_block: the scheduler runs speculative evaluations -- a step that
    goes on also stages the proposal that would follow a rejection of its main one (lambda four times larger, :583-585), to be evaluated
    beside it.  Returns the next state (the argument is not changed)."""
    st = copy.deepcopy(state)
    st.pop("_inc_scaled", None)
    lvl, mode = st["lvl"], info["mode"]
    fixed = params.fixed_schedule > 0
    max_it = R.level_max_it(params, lvl)
    st["rounds"][lvl] += 1
    st["ticks"] += 1
    had_spec = bool(spec_block and st["spec_valid"])
    st["spec_valid"] = 0
    level_done = False
    if st["phase"] == PH_INIT:
        st["evals"][lvl] += 1
        if not fixed and main["rs"][5] > 0.6 and float(st["level_cutoff_repeat"]) < 50:  # :477-485 / :875-883
            st["level_cutoff_repeat"] = F32(F32(st["level_cutoff_repeat"]) * F32(2))
            _stage_cutoff(params, st["ev"], st["level_cutoff_repeat"], False)
            return st
        st["res_old"] = np.array(main["rs"], np.float64)
        if mode == 1:
            st["Hs"], st["bs"] = F32(main["Hs"]), F32(main["bs"])  # :885
        else:
            st["H"], st["b"] = np.array(main["H"], np.float64).reshape(8, 8), np.array(main["b"], np.float64)  # :487
        st["lam"], st["iteration"] = F32(0.01), 0  # :489
        level_done = max_it <= 0
    else:
        accept, level_done = _consume(params, info, st, main, "", fixed, max_it)
        if not level_done and not accept and had_spec:
            # the loop's next iteration proposes from the same H, b and pose at the lambda the rejection left: the speculative
            # candidate.  Its evaluation is already here: the iteration is taken now.
            _, level_done = _consume(params, info, st, spec, "spec_", fixed, max_it)
    if level_done:
        _end_level(params, info, st, fixed)
        return st
    propose(params, info, st, st["lam"], False)
    if spec_block and not fixed and st["iteration"] + 1 < max_it:
        propose(params, info, st, lambda_after(params, st["lam"], False), True)
        st["spec_valid"] = 0 if _is_small(info, st, "") else 1  # (a small main step ends the loop: nothing follows it)
    return st
