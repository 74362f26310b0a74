"""The case table of the LM state machine's tests: constructed states plus chunk partials, one list shared by the CPU tests of the
reference (tests/test_lm_machine_ref.py) and the device tests (tests/test_lm_machine.py).  CPU only.

A case is a dict: row (the table row it stands for), mode, pkey (parameter set: affine mode name, fixed_schedule, the level whose
iteration bound is 0 or None), lvl, state (a _lm_machine_ref state), nch, part (float32 [nch, 64]), spec_block, spec_part, expect (what
the reference's next state must show for the row to count as reached: a function of (state in, state out)), d_evals / d_ro (the
step's evaluation counts).  Every decision is steered through the STATE (res_old relative to the rs the partials reduce to, lambda,
iteration, the increments); the partials are generic: about 12 decades, mixed signs, integer slots up to 4096 per chunk, NaN patterns
in the twelve unused floats of every chunk."""
import functools

import numpy as np

import _lm_machine_ref as M
import _lm_step_ref as R
from oracle import oracle as O

F32 = np.float32
CUR = np.array([0.1825741858350554, -0.3651483716701107, 0.5477225575051661, 0.7302967433402214, 0.3, -0.2, 1.5])
AFF = np.array([0.03, 2.0])
MODES = dict(R.MODES, prior=(1.0, 1.0))  # affine_opt_mode_a, _b; "prior": nonzero and not negative (the |a|, |b| tests without zeroing)
NLEVELS = 4  # the mini4 pyramid
PLAIN_CHUNKS = (0, 1, 18, 19, 20, 38, 152, 153, 171, 305)
SPEC_CHUNKS = (1, 2, 19, 20, 32, 39)


def ref_params(pkey):
    mode_name, fixed, zero_it = pkey
    p = O.default_params()
    p.affine_opt_mode_a, p.affine_opt_mode_b = MODES[mode_name]
    p.fixed_schedule = fixed
    if zero_it is not None:
        p.max_iterations[zero_it] = 0
    return p


def split_ints(rng, total, nch, cap=4096):
    """`total` as nch non-negative integers of at most cap each"""
    out = np.zeros(nch, np.int64)
    left = int(total)
    assert left <= cap * max(nch, 0) and (nch > 0 or left == 0)
    for c in range(nch):
        room = cap * (nch - 1 - c)
        lo = max(0, left - room)
        out[c] = left if c == nch - 1 else int(rng.integers(lo, min(cap, left) + 1))
        left -= int(out[c])
    return out


def gen_partials(seed, nch, ints, e_exact=None):
    """float32 [nch, 64]; ints = (n_terms, n_sat, n_warped) totals; e_exact: the E slot sums to exactly this (chunk 0 holds it)"""
    rng = np.random.default_rng(seed)
    P = np.zeros((max(nch, 1), 64), np.float32)
    P[:, :49] = (rng.uniform(1, 10, (len(P), 49)) * 10.0 ** rng.uniform(-6, 6, (len(P), 49)) * rng.choice((-1.0, 1.0), (len(P), 49))).astype(np.float32)
    P[:, M.SLOT_E] = np.abs(P[:, M.SLOT_E])
    P[:, M.SLOT_FLOW_NUM] = np.abs(P[:, M.SLOT_FLOW_NUM])
    if e_exact is not None:
        P[:, M.SLOT_E] = 0
        P[0, M.SLOT_E] = e_exact
    iv = P.view(np.int32)
    for k, total in enumerate(ints):
        iv[:, M.SLOT_NTERMS + k] = split_ints(rng, total, nch) if nch else 0
    iv[:, 52:] = 0x7FC00000 + rng.integers(0, 1000, (len(P), 12))  # never read: NaN patterns
    return P[:nch].copy() if nch else np.zeros((0, 64), np.float32)


def gen_cancelling(seed, nch, ints):
    """gen_partials whose float slots make the ORDER of the float64 additions visible in the float32 results: in every slot a third of
    the chunks hold pairs +x, -x of 1e5 .. 1e6 that cancel exactly, the others values of 1e-6 .. 1e-5.  A running sum that holds a large
    and a small value at once needs more than 53 bits: it is rounded at about 1e-10, which of the roundings happen depends on the order,
    and after the large values have cancelled the difference stands at 1e-5 .. 1e-4 of the sum -- hundreds of float32 ulps.  (Values
    spread over 12 decades that do NOT cancel differ between two orders at 1e-16 of the sum: gone once the sum is cast to float.)"""
    P = gen_partials(seed, nch, ints)
    rng = np.random.default_rng(seed + 31)
    if nch < 4:
        return P
    for slot in range(M.SLOT_NTERMS):
        perm, npair = rng.permutation(nch), nch // 3
        small = rng.uniform(1, 10, nch) * 10.0 ** rng.uniform(-6, -5, nch) * (1.0 if slot in (M.SLOT_E, M.SLOT_FLOW_NUM) else rng.choice((-1.0, 1.0), nch))
        P[:, slot] = small.astype(np.float32)
        big = (rng.uniform(1, 10, npair) * 10.0 ** rng.uniform(5, 6, npair)).astype(np.float32)
        P[perm[:npair], slot] = big
        P[perm[npair:2 * npair], slot] = -big
    return P


def nan_partials(nch):
    P = np.zeros((nch, 64), np.float32)
    P.view(np.uint32)[:] = 0x7FC00123
    return P


def evaluation(params, part, nch, max_energy):
    sums, isums = M.reduce_ref(part, nch)
    return M.system_ref(params, sums, isums, max_energy)


def base_state(params, mode, lvl, phase, seed=1, lcr=1.0):
    rng = np.random.default_rng(1000 + seed)
    st = M.new_state(lvl, coarsest=NLEVELS - 1)
    st["phase"], st["level_cutoff_repeat"] = phase, F32(lcr)
    st["cur"], st["aff_cur"] = CUR.copy(), AFF.copy()
    st["cand"] = R.orc_se3_mul(R.orc_se3_exp(rng.normal(size=6) * 0.01), CUR)
    st["aff_cand"] = AFF + np.array([0.004, -0.7])
    st["spec_cand"] = R.orc_se3_mul(R.orc_se3_exp(rng.normal(size=6) * 0.004), CUR)
    st["spec_aff_cand"] = AFF + np.array([0.001, -0.2])
    st["H"], st["b"] = R._gn_like(rng), rng.normal(size=8) * 30
    st["Hs"], st["bs"] = F32(41.5), F32(-3.25)
    st["scale_cur"], st["scale_cand"], st["spec_scale_cand"] = F32(1.3), F32(1.25), F32(1.28)
    st["inc_norm"], st["spec_inc_norm"], st["inc_f"], st["spec_inc_f"] = np.float64(0.05), np.float64(0.02), F32(0.05), F32(0.02)
    st["res_old"] = np.array([5000.0, 400.0, 0.3, 0.0, 0.7, 0.1])
    st["lam"], st["iteration"] = F32(0.01), 2 if phase == M.PH_ITER else 0
    st["evals"][:NLEVELS] = (3, 5, 7, 9)
    st["evals_ro"][:NLEVELS] = (0, 1, 1, 2)
    st["rounds"][:NLEVELS] = (2, 4, 6, 8)
    st["ticks"] = 17
    st["last_residuals"][NLEVELS - 1], st["last_inners"][NLEVELS - 1] = 4.5, 77.0
    for ev, ro in ((st["ev"], 0), (st["spec_ev"], 0)):
        ev["cutoff"], ev["max_energy"] = R.cutoff_of(params, lcr)
        ev["residual_only"] = ro
        ev["M"], ev["t"] = rng.normal(size=9).astype(F32), rng.normal(size=3).astype(F32)
        ev["aff0"], ev["aff1"] = F32(1.01), F32(-0.5)
        if mode == 1:
            ev["scale"] = F32(1.25)
    return st


def steer(st, rs, how):
    """res_old so that the evaluation `rs` is strictly better / exactly equal / worse than it, or the old ratio a NaN"""
    r0 = F32(rs[0])
    st["res_old"] = np.array(rs, np.float64)
    if how == "better":
        st["res_old"][0] = np.float64(np.nextafter(r0, F32(np.inf)))
    elif how == "worse":
        st["res_old"][0] = np.float64(np.nextafter(r0, F32(-np.inf)))
    elif how == "nan_old":
        st["res_old"][:2] = 0.0
    else:
        assert how == "equal"
    st["res_old"][2:5] = (0.25, 0.0, 0.75)  # (what end_level reports unless the evaluation is accepted)


def gentle_system(P):
    """H = 4 I, b = -0.1 (before 1 / n and SCALE_*), Hs = 4, bs = -0.1 for a warped count of 404: a step of a few hundredths, not small"""
    P[:, :45] = 0
    for r in range(8):
        P[0, M.tri_idx(r, r)] = 4.0 * 404
        P[0, M.tri_idx(r, 8)] = -0.1 * 404
    P[0, 1] = -0.1 * 404


def dominant_diagonal(P):
    """H ~ 1e13 I (Hs likewise): |inc| ~ |b| / H, far below 1e-3"""
    for r in range(9):
        P[:, M.tri_idx(r, r)] = np.abs(P[:, M.tri_idx(r, r)]) + F32(1e13)


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    seed = [0]

    def add(row, mode, pkey=("ab", 0, None), lvl=1, phase=M.PH_ITER, nch=3, ints=(400, 40, 410), how=None, spec_block=False, spec=None,
            expect=None, d_evals=1, d_ro=0, mod=None, e_exact=None, lcr=1.0, part_mod=None):
        """spec: None, or (E factor of the speculative evaluation relative to the main one, spec_valid)"""
        seed[0] += 1
        params = ref_params(pkey)
        st = base_state(params, mode, lvl, phase, seed[0], lcr)
        part = gen_partials(seed[0], nch, ints, e_exact)
        if part_mod:
            part_mod(part)
        if how is not None:
            steer(st, evaluation(params, part, nch, st["ev"]["max_energy"])["rs"], how)
        spec_part = None
        if spec_block:
            spec_part = nan_partials(nch)
            if spec is not None:
                factor, valid = spec
                spec_part = part.copy()
                spec_part[:, M.SLOT_E] *= F32(factor)
                spec_part[:, :45] *= F32(-1.5)
                st["spec_valid"] = int(valid)
                if not valid:
                    spec_part.view(np.uint32)[:, :52] = 0x7FC00123
        if mod:
            mod(st)
        out.append(dict(row=row, mode=mode, pkey=pkey, lvl=lvl, state=st, nch=nch, part=part, spec_block=spec_block, spec_part=spec_part,
                        expect=expect, d_evals=d_evals, d_ro=d_ro))

    def setter(**kw):
        def f(st):
            for k, v in kw.items():
                if "." in k:
                    a, b = k.split(".")
                    st[a][b] = v
                else:
                    st[k] = v
        return f

    I, T = M.PH_INIT, M.PH_ITER
    repeated = lambda i, o: float(o["level_cutoff_repeat"]) == 2 * float(i["level_cutoff_repeat"]) and o["phase"] == I and o["lvl"] == i["lvl"]  # noqa: E731
    proposed = lambda i, o: o["phase"] == T and o["lvl"] == i["lvl"] and o["status"] == M.ST_RUNNING  # noqa: E731
    took_system = lambda i, o: proposed(i, o) and o["iteration"] == 0 and float(o["lam"]) == float(F32(0.01))  # noqa: E731
    ended = lambda i, o: (o["lvl"] != i["lvl"] or o["status"] != M.ST_RUNNING or (o["phase"] == I and o["iteration"] == 0))  # noqa: E731
    accepted = lambda i, o: float(o["lam"]) == float(F32(i["lam"]) * F32(0.5)) and o["iteration"] == i["iteration"] + 1  # noqa: E731
    rejected = lambda i, o: float(o["lam"]) >= float(i["lam"]) * 4 - 1e-12 and o["iteration"] == i["iteration"] + 1 and np.array_equal(o["cur"], i["cur"])  # noqa: E731

    staged_twin = lambda i, o: not np.array_equal(o["spec_cand"], i["spec_cand"]) or float(o["spec_scale_cand"]) != float(i["spec_scale_cand"])  # noqa: E731

    # ---- PH_INIT ----
    for mode in (0, 1, 2):
        add("init/ratio 3/5 repeats", mode, phase=I, ints=(5, 3, 8), expect=repeated)
        add("init/ratio 599/1000 takes the system", mode, phase=I, ints=(1000, 599, 1000), expect=took_system)
        add("init/ratio 601/1000 repeats", mode, phase=I, ints=(1000, 601, 1001), expect=repeated)
        add("init/repeat at 32 doubles to 64", mode, phase=I, ints=(10, 9, 10), lcr=32.0, expect=repeated)
        add("init/no repeat at 64", mode, phase=I, ints=(10, 9, 10), lcr=64.0, expect=took_system)
        add("init/fixed schedule never repeats", mode, pkey=("ab", 3, None), phase=I, ints=(10, 9, 10), expect=took_system)
        add("init/no iterations: the level ends at once", mode, pkey=("ab", 0, 1), phase=I, ints=(10, 1, 10),
            expect=lambda i, o: o["lvl"] == i["lvl"] - 1 and o["phase"] == I)
        add("init/no terms: 0/0 ratio", mode, phase=I, ints=(0, 0, 7), expect=took_system)
        for k in range(4):
            add("init/n_warped mod 4", mode, phase=I, ints=(300, 30, 404 + k), expect=took_system)
    add("init/n_warped 0", 0, phase=I, ints=(0, 0, 0), expect=took_system)
    add("init/n_warped 0", 1, phase=I, ints=(0, 0, 0), expect=took_system)
    # ---- PH_ITER ----
    for mode in (0, 1, 2):
        add("iter/strictly better: accepted", mode, how="better", expect=accepted)
        add("iter/exactly equal: rejected", mode, how="equal", expect=rejected)
        add("iter/worse: rejected", mode, how="worse", expect=rejected)
        add("iter/NaN new ratio: rejected", mode, ints=(0, 0, 12), e_exact=0.0, expect=rejected)
        add("iter/NaN old ratio: rejected", mode, how="nan_old", expect=rejected)
        add("iter/fixed schedule: always accepted, never small", mode, pkey=("ab", 5, None), how="worse",
            mod=setter(inc_norm=np.float64(0.0), inc_f=F32(-1.0)), expect=lambda i, o: accepted(i, o) and proposed(i, o))
        lim4 = F32(F32(0.001) / F32(4))
        for name, lam in (("below", np.nextafter(lim4, F32(0))), ("at", lim4), ("above", np.nextafter(lim4, F32(1)))):
            add("iter/lambda floor: 4 lambda " + name + " the limit", mode, how="worse", mod=setter(lam=F32(lam)),
                expect=lambda i, o, name=name: (float(o["lam"]) == float(F32(0.001))) == (name != "above"))
        for name, it in (("below", 17), ("at", 19), ("above", 25)):
            add("iter/iteration + 1 " + name + " the bound", mode, how="better", mod=setter(iteration=it),
                expect=lambda i, o, name=name: ended(i, o) == (name != "below"))
    for mode in (0, 2):
        for name, v in (("at 1e-3", np.float64(1e-3)), ("above", np.nextafter(np.float64(1e-3), 1.0)), ("NaN", np.float64(np.nan))):
            add("iter/inc_norm " + name, mode, how="better", mod=setter(inc_norm=v),
                expect=lambda i, o, name=name: ended(i, o) == (name != "above"))
    for name, v in (("negative and large: small (signed)", F32(-5.0)), ("at 1e-3f", F32(1e-3)), ("above", np.nextafter(F32(1e-3), F32(1))), ("well above", F32(2e-3))):
        add("iter/scale inc_f " + name, 1, how="better", mod=setter(inc_f=v),
            expect=lambda i, o, v=v: ended(i, o) == (not float(v) > 1e-3))
    # ---- a speculative block ----
    for mode in (0, 1, 2):
        add("spec/main accepted: twin ignored, not counted", mode, how="better", spec_block=True, spec=(0.5, 1), mod=setter(**{"spec_ev.residual_only": 1}),
            expect=lambda i, o: accepted(i, o))
        add("spec/main rejected, twin accepted", mode, how="equal", spec_block=True, spec=(0.5, 1), d_evals=2,
            expect=lambda i, o: o["iteration"] == i["iteration"] + 2 and float(o["lam"]) == float(F32(F32(i["lam"]) * F32(4)) * F32(0.5)))
        add("spec/main rejected, twin exactly equal: rejected", mode, how="equal", spec_block=True, spec=(1.0, 1), d_evals=2,
            expect=lambda i, o: o["iteration"] == i["iteration"] + 2 and float(o["lam"]) == float(i["lam"]) * 16 and np.array_equal(o["res_old"], i["res_old"]))
        add("spec/both rejected: two lambda updates", mode, how="worse", spec_block=True, spec=(2.0, 1), d_evals=2,
            expect=lambda i, o: o["iteration"] == i["iteration"] + 2 and float(o["lam"]) == float(i["lam"]) * 16)
        add("spec/both rejected: each update floored", mode, how="worse", spec_block=True, spec=(2.0, 1), d_evals=2, mod=setter(lam=F32(1e-5)),
            expect=lambda i, o: o["iteration"] == i["iteration"] + 2 and float(o["lam"]) == float(F32(F32(0.001) * F32(4))))
        add("spec/twin small", mode, how="worse", spec_block=True, spec=(0.5, 1), d_evals=2, mod=setter(spec_inc_norm=np.float64(5e-4), spec_inc_f=F32(5e-4)),
            expect=lambda i, o: ended(i, o) and o["evals"][i["lvl"]] == i["evals"][i["lvl"]] + 2)
        add("spec/bound reached by the twin", mode, how="worse", spec_block=True, spec=(0.5, 1), d_evals=2, d_ro=1,
            mod=setter(iteration=18, **{"spec_ev.residual_only": 1}), expect=lambda i, o: ended(i, o))
        add("spec/main small while spec_valid: twin not consumed", mode, how="worse", spec_block=True, spec=(0.5, 1),
            mod=setter(inc_norm=np.float64(1e-4), inc_f=F32(1e-4)), expect=lambda i, o: ended(i, o))
        add("spec/spec_valid 0: NaN partials behind", mode, how="worse", spec_block=True, spec=(0.5, 0), expect=rejected)
        add("spec/want_spec: iteration + 1 below the bound", mode, how="better", spec_block=True, mod=setter(iteration=17),
            expect=lambda i, o: proposed(i, o) and staged_twin(i, o))
        add("spec/want_spec: iteration + 1 at the bound", mode, how="better", spec_block=True, mod=setter(iteration=18),
            expect=lambda i, o: proposed(i, o) and not staged_twin(i, o) and o["spec_valid"] == 0)
        add("spec/evals_ro from the main evaluation", mode, how="better", spec_block=True, d_ro=1, mod=setter(**{"ev.residual_only": 1}), expect=accepted)
        add("spec/init stages a twin", mode, phase=I, ints=(300, 30, 404), spec_block=True, expect=lambda i, o: took_system(i, o) and staged_twin(i, o))
        add("spec/fixed schedule stages none", mode, pkey=("ab", 5, None), how="worse", spec_block=True, expect=lambda i, o: proposed(i, o) and not staged_twin(i, o) and o["spec_valid"] == 0)
    # returned spec_valid after a small main proposal: H = I, b tiny gives |inc| < 1e-3 (pose); Hs huge (scale)
    for mode in (0, 1, 2):
        add("spec/spec_valid 0 after a small main proposal", mode, phase=I, ints=(300, 30, 404), spec_block=True, part_mod=dominant_diagonal,
            expect=lambda i, o: took_system(i, o) and staged_twin(i, o) and o["spec_valid"] == 0)
        add("spec/spec_valid 1 after a main proposal that is not small", mode, phase=I, ints=(300, 30, 404), spec_block=True, part_mod=gentle_system,
            expect=lambda i, o: took_system(i, o) and staged_twin(i, o) and o["spec_valid"] == 1)
    # ---- end of level ----
    for mode in (0, 1, 2):
        for name, mr in (("min_res 2: not aborted", 2.0), ("min_res just under 2: aborted (pose)", np.nextafter(2.0, 0.0)), ("min_res NaN: no limit", np.nan)):
            def m(st, mr=mr):
                st["iteration"] = 19
                st["res_old"][:2] = (9.0 * 400, 400.0)
                st["min_res"][:] = mr
            add("end/E/n = 9, " + name, mode, how="worse", e_exact=1e6, mod=m,
                expect=lambda i, o, mode=mode, name=name: o["last_residuals"][i["lvl"]] == 3.0 and (o["status"] == M.ST_ABORTED) == (mode == 0 and "just under" in name))

        def m_fixed(st):
            st["iteration"] = 4
            st["min_res"][:] = 1e-3
        add("end/fixed schedule never aborts", mode, pkey=("ab", 5, None), how="worse", mod=m_fixed, expect=lambda i, o: o["lvl"] == i["lvl"] - 1 and o["status"] == M.ST_RUNNING)
        add("end/level repeat taken once", mode, how="worse", lcr=2.0, mod=setter(iteration=19),
            expect=lambda i, o: o["lvl"] == i["lvl"] and o["have_repeated"] == 1 and o["phase"] == I and float(o["level_cutoff_repeat"]) == 1)
        add("end/level repeat not a second time", mode, how="worse", lcr=2.0, mod=setter(iteration=19, have_repeated=1),
            expect=lambda i, o: o["lvl"] == i["lvl"] - 1 and o["have_repeated"] == 1)
        add("end/hand-down after an accepted step", mode, how="better", spec_block=True, spec=(0.5, 1), mod=setter(iteration=19),
            expect=lambda i, o, mode=mode: o["lvl"] == i["lvl"] - 1 and o["phase"] == I and o["iteration"] == 0 and o["spec_valid"] == 0
            and float(o["level_cutoff_repeat"]) == 1 and o["ev"]["residual_only"] == 0 and o["last_inners"][i["lvl"]] == o["res_old"][1]
            and o["last_residuals"][i["lvl"]] == np.float64(np.sqrt(F32(o["res_old"][0] / o["res_old"][1])))
            and np.array_equal(o["flow"], o["res_old"][2:5] if mode == 0 else i["flow"]))
        add("end/hand-down from the coarsest level", mode, lvl=3, how="worse", mod=setter(iteration=49), expect=lambda i, o: o["lvl"] == 2 and o["phase"] == I)
    add("end/scale from level 0: good", 1, lvl=0, how="worse", mod=setter(iteration=9), expect=lambda i, o: o["status"] == M.ST_GOOD)
    e15 = float(np.exp(1.5))
    for mode in (0, 2):
        for pk, rows in (("ab", (("|log rel_a| below 1.5", (np.log(e15 * (1 - 1e-4)), 2.0), True), ("|log rel_a| above 1.5", (np.log(e15 * (1 + 1e-4)), 2.0), False),
                                 ("|log rel_a| above 1.5, negative", (-np.log(e15 * (1 + 1e-4)), 2.0), False),
                                 ("|rel_b| below 200", (0.03, 199.99), True), ("|rel_b| above 200", (0.03, -200.01), False))),
                         ("prior", (("|a| below 1.2", (1.1999, 2.0), True), ("|a| above 1.2", (-1.2001, 2.0), False), ("|b| below 200", (0.03, -199.99), True),
                                    ("|b| above 200", (0.03, 200.01), False))),
                         ("fix_ab", (("negative modes zero the pair", (0.5, 20.0), True), ("negative modes: |a| above 1.2", (1.3, 20.0), False))),
                         ("fix_a", (("a zeroed, b kept", (0.5, 20.0), True),)), ("fix_b", (("b zeroed, a kept", (0.5, 20.0), True),))):
            for name, aff, good in rows:
                add("verdict/" + pk + ": " + name, mode, pkey=(pk, 0, None), lvl=0, how="worse", mod=setter(iteration=9, aff_cur=np.array(aff, np.float64)),
                    expect=lambda i, o, good=good, pk=pk: o["status"] == (M.ST_GOOD if good else M.ST_BAD_AFFINE)
                    and (o["aff_cur"][0] == 0) == (good and MODES[pk][0] < 0) and (o["aff_cur"][1] == 0) == (good and MODES[pk][1] < 0))
    return tuple(out)


def run_reference(case, Ki=None, info_kw=None, spec_block=None):
    """the reference's next state of a case (and the evaluations it was given)"""
    params = ref_params(case["pkey"])
    st = case["state"]
    info = M.tracker_info(case["mode"], Ki=Ki, **(info_kw or {}))
    main = evaluation(params, case["part"], case["nch"], st["ev"]["max_energy"])
    sb = case["spec_block"] if spec_block is None else spec_block
    spec = evaluation(params, case["spec_part"], case["nch"], st["spec_ev"]["max_energy"]) if sb and case["spec_part"] is not None else None
    return M.decide_ref(params, info, st, main, spec, spec_block=sb), main, spec


# ---- comparing states (the scheduling-only property, on the reference and on the device) ----
SCHEDULING_ONLY = ("rounds", "ticks")
SPEC_BLOCK_FIELDS = ("spec_valid", "spec_cand", "spec_aff_cand", "spec_inc_norm", "spec_scale_cand", "spec_inc_f", "spec_ev", "_inc_scaled")


def state_diff(a, b, skip=()):
    """the fields of two states that differ in a bit (a NaN equals a NaN)"""
    bad = []
    for k in a:
        if k in skip:
            continue
        x = np.asarray(a[k]) if not isinstance(a[k], dict) else None
        if x is None:
            bad += [k + "." + n for n in state_diff(a[k], b[k])]
        elif x.dtype.kind == "f":
            if not R.same_bits(x, np.asarray(b[k], x.dtype), nan_as_nan=True):
                bad.append(k)
        elif not np.array_equal(x, np.asarray(b[k])):
            bad.append(k)
    return bad


def dead_fields(out, lvl_in):
    """Once a step has ended the level, the candidate block is the last candidate CONSUMED and nothing reads it again (the next
    proposal overwrites it): the main one where a twin was consumed beside it, the twin where the loop ran plainly.  A problem that has
    its verdict keeps the last staged evaluation in the same way."""
    ended = out["status"] != M.ST_RUNNING or out["phase"] == M.PH_INIT
    return (("cand", "aff_cand", "inc_norm", "scale_cand", "inc_f") if ended else ()) + (("ev",) if out["status"] != M.ST_RUNNING else ())


def spec_cases():
    return [c for c in cases() if c["spec_block"] and c["state"]["spec_valid"] and c["state"]["phase"] == M.PH_ITER]
