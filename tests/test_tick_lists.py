"""The tick engine's device code below whole runs (csrc/form_tick.hpp: tick_reserve_kernel, TickReserve, tick_push, tick_after_step,
tick_try_admit / tick_admit_entry, tick_admit_kernel, tick_lm_kernel) through dsm_diag_tick_reserve / _stage / _step, against the rules
as tests/_tick_ref.py restates them (tests/test_tick_ref.py checks that restatement).  Every output is an integer or copied bits: every
comparison is exact.  The item allocation of a call is cap + chain_cap + a guard region, all prefilled with a sentinel: a write that
the list's bounds should have stopped shows as a changed word, never as a fault.

  A  reserve: the share of every segment and the ring index of every free slot, 64-bit heads
  B  stage: the lists of 300 mixed slots in one launch, the counters, chains on / off / bounded, every kind of reservation
  C  stage: a list that overflows by one word and by a block, a chain area one entry short
  D  stage: retirement into the result ring and the refill of the retired slots from the waiting ring, 64-bit counters
  E  step: the production tick_lm_kernel on the rows of tests/_lm_machine_cases.py -- the stored state is dsm_diag_lm_step's, the list is
     what the reference builds from it, an early reservation is never too short and a terminating step makes none
  F  admit: tick_admit_kernel behind tick_reserve_kernel's table
  G  argument errors"""
import ctypes as C
import time

import numpy as np
import pytest

import _lm_machine_cases as Cs
import _lm_machine_ref as M
import _tick_ref as T
from _gn_f64 import reduction_geometry
from _scenes import hip_tracker, make_scene
from test_lm_machine import grouped, pack, partial_block, trackers  # noqa: F401  (the mini4 trackers of the LM-machine table)

RING = 256
STEPPED_OFFSET = 28  # LMState::stepped: the eighth int of the state
TERMINATED = (T.ST_GOOD, T.ST_ABORTED, T.ST_BAD_AFFINE)


@pytest.fixture(scope="module")
def tiny(ctx):
    sc = make_scene("tiny")
    trk = hip_tracker(ctx, sc)
    yield trk, sc
    trk.close()


def slot_records(descs):
    from direct_stereo_slam_amd.tracker import TICK_SLOT

    arr = np.zeros(len(descs), TICK_SLOT)
    for i, (a, d) in enumerate(zip(arr, descs)):
        rng = np.random.default_rng(7000 + i)
        a["status"], a["lvl"], a["n"], a["ppt"] = d.get("status", T.ST_RUNNING), d.get("lvl", 0), d["n"], d["ppt"]
        a["spec_valid"], a["n0"], a["residual_only"] = int(d.get("twin", False)), d.get("n0", 100), d.get("ro", 0)
        a["ticks"], a["stepped"], a["ticket"] = 3 + i, 0, 1000 + i
        a["reserve"], a["res_base"], a["res_total"] = d.get("reserve", 0), d.get("res_base", 0), d.get("res_total", 0)
        for f, k in (("cur", 7), ("aff_cur", 2), ("last_residuals", 6), ("flow", 3)):
            a[f] = rng.standard_normal(k)
        a["last_residuals"][5] = np.nan  # (a level the problem never ran: copied as bits)
        a["scale_cur"] = rng.standard_normal()
        for f in ("evals", "evals_ro", "rounds"):
            a[f] = rng.integers(0, 2**40, 6)
    return arr


def nch_of(d):
    return T.chunks_of(d["n"], d["ppt"]) if d["ppt"] else 0


def expectation(descs, cfg):
    """what the slots' staging adds to the list, by the rules: (blocks, chains, abandoned words the count grew by, preplaced slots,
    per-level (evals, ro, items))"""
    blocks, chains, abandoned, preplaced = {}, [], 0, set()
    sched = np.zeros((3, 6), np.int64)
    for s, d in enumerate(descs):
        kind, nch, twin, n0 = d.get("reserve", 0), nch_of(d), d.get("twin", False), d.get("n0", 100)
        reserved = T.reservation(cfg["chain_cap"], cfg["chain_max_n0"], nch, kind == 2, n0) if kind in (1, 2) else d.get("res_total", 0) if kind == 3 else 0
        if d.get("status", T.ST_RUNNING) != T.ST_RUNNING:  # a terminated slot stages nothing: its reservation becomes no-ops
            abandoned += reserved if kind != 3 else 0
            continue
        to_chain, length, dropped = T.staged(cfg["chain_cap"], cfg["chain_max_n0"], nch, twin, n0, reserved)
        abandoned += dropped if kind != 3 else 0
        if to_chain:
            chains.append(s)
        elif length:
            blocks[s] = (nch, twin, length)
            if kind == 3 and reserved >= (2 if twin else 1) * T.npos(nch):  # (used: the block stands where the caller reserved)
                preplaced.add(s)
            lvl = d.get("lvl", 0)
            sched[0, lvl] += 1
            sched[1, lvl] += 1 if d.get("ro", 0) else 0
            sched[2, lvl] += (2 if twin else 1) * T.npos(nch)
    return blocks, chains, abandoned, preplaced, sched


def run_stage(trk, descs, cfg, ctl=None, pending=None, stepped=0, mode=0):
    ctl = ctl or dict(pending_head=0, pending_count=0, retired=0, ring=RING)
    return trk.diagTickStage(mode, slot_records(descs), cfg, ctl, pending, stepped)


def check_stage_lists(out, descs, cfg, overflowed=False):
    blocks, chains, abandoned, preplaced, sched = expectation(descs, cfg)
    seg, buf = out["seg"], cfg["buf"]
    T.check_list(out["items"], cfg["cap"], cfg["chain_cap"], cfg["count"], cfg["chain"], seg.count[buf], seg.chain[buf], blocks, chains, abandoned,
                 overflowed=overflowed, preplaced=preplaced)
    assert seg.overflow == int(overflowed)
    assert (seg.count[buf ^ 1], seg.chain[buf ^ 1]) == (7, 7) and not any(seg.pad)  # (tick_lm_kernel's slot 0 clears these; nothing here does)
    got = np.array([list(out["ctl"].sched_evals), list(out["ctl"].sched_ro), list(out["ctl"].sched_items)])
    assert np.array_equal(got, sched), (got, sched)
    return blocks, chains


# ---------------------------------------------------------------------------------------------------------------------------------
# A  reserve
# ---------------------------------------------------------------------------------------------------------------------------------
def free_patterns(ns):
    """running flags: no slot free, all, alternating, only the last, only slots 250 .. 262"""
    yield np.ones(ns, np.uint8)
    yield np.zeros(ns, np.uint8)
    yield (np.arange(ns) % 2).astype(np.uint8)
    r = np.ones(ns, np.uint8)
    r[-1] = 0
    yield r
    r = np.ones(ns, np.uint8)
    r[250:263] = 0
    yield r


def check_reserve(ctx, segs, running, head, count):
    idx, heads, intact = ctx.diagTickReserve(segs, running, head, count)
    want_idx, want_heads = T.reserve(segs, running, head, count)
    assert list(idx) == want_idx, (segs, head, count, [(j, int(a), b) for j, (a, b) in enumerate(zip(idx, want_idx)) if a != b][:6])
    assert heads == want_heads and intact, (segs, head, count, heads, want_heads, intact)
    assert all(idx[j] == -1 for j in np.nonzero(running)[0] if want_idx[j] != -2)  # running slots get nothing


@pytest.mark.gpu
def test_reserve_one_segment(ctx):
    t0, n = time.perf_counter(), 0
    for ns in (1, 63, 64, 65, 255, 256, 257, 600):
        for running in free_patterns(ns):
            F = int((running == 0).sum())
            for A in sorted({0, 1, max(F - 1, 0), F, F + 1}):
                for head in (0, RING - 3, 2**32 - 2, 2**32 + RING - 2)[:4 if ns in (65, 600) else 1]:
                    check_reserve(ctx, [(0, 0, ns)], running, [head, 11], [head + A, 11])  # (nothing waits on the other kind)
                    n += 1
    print(f"\nreserve, one segment: {n} calls, {time.perf_counter() - t0:.2f} s")


@pytest.mark.gpu
def test_reserve_many_segments(ctx):
    rng = np.random.default_rng(5)
    # pose groups, then scale companions, as build_segments lays them out
    tables = {
        "two": [(0, 0, 300), (1, 300, 100)],
        "three": [(0, 0, 257), (0, 257, 256), (1, 513, 64)],
        "twenty": [(0, 40 * k, 40) for k in range(13)] + [(0, 520, 0)] + [(1, 520 + 30 * k, 30) for k in range(6)],  # (one empty segment)
    }
    for name, segs in tables.items():
        nslots = max(i0 + ns for _, i0, ns in segs)
        for density in (0.0, 0.3, 0.9):
            running = (rng.random(nslots) < density).astype(np.uint8)
            m, i0, ns = segs[1]
            running[i0:i0 + ns] = 1  # a segment with no free slot
            for a0, a1 in ((0, 0), (1, 1), (7, 3), (100, 17), (257, 5000), (5000, 0)):
                for head in ([0, 0], [RING - 3, 2**32 - 2], [2**32 + RING - 2, RING - 3]):
                    check_reserve(ctx, segs, running, head, [head[0] + a0, head[1] + a1])
    # four pose groups of three free slots: 12 F = 12; A = 5 leaves a remainder of 1 behind the floors, A = 7 one of nseg - 1 = 3
    segs = [(0, 5 * k, 5) for k in range(4)] + [(1, 20, 5)]
    running = np.tile(np.array([1, 0, 0, 1, 0], np.uint8), 5)
    for A in (5, 7):
        assert A - sum(A * 3 // 12 for _ in range(4)) == (1 if A == 5 else 3)
        check_reserve(ctx, segs, running, [2**32 - 2, 0], [2**32 - 2 + A, 2])
    # pending_count < pending_head: nothing is handed out and the head stays
    idx, heads, intact = ctx.diagTickReserve(segs, running, [9, 2**32 + 5], [7, 2**32 + 4])
    assert heads == [9, 2**32 + 5] and intact and set(idx.tolist()) == {-1}
    # a slot no segment covers is not written
    idx, _, _ = ctx.diagTickReserve([(0, 2, 3)], np.zeros(8, np.uint8), [0, 0], [9, 9])
    assert idx.tolist() == [-2, -2, 0, 1, 2, -2, -2, -2]


# ---------------------------------------------------------------------------------------------------------------------------------
# B  stage: lists
# ---------------------------------------------------------------------------------------------------------------------------------
N0 = 5000
# real (n, ppt) pairs at the edges of the two chunk tables
TABLE_PAIRS = [(n, p) for n, p in ((256, 1), (257, 2), (512, 2), (513, 4), (2048, 8), (2049, 16), (4095, 1), (4096, 2), (16383, 2), (16384, 4), (65535, 4),
                                   (65536, 8))]


def mixed_slots(nslots=300, seed=1):
    """every chunk count x {no twin, twin} x every kind of reservation, n0 around the chain bound, three levels"""
    rng = np.random.default_rng(seed)
    shapes = [(nch * 256, 1) for nch in (0, 1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65)] + TABLE_PAIRS
    descs = []
    for s in range(nslots):
        n, ppt = shapes[s % len(shapes)]
        twin = (s // len(shapes)) % 2 == 1
        d = dict(n=n, ppt=ppt, twin=twin, n0=(N0 - 1, N0, N0 + 1)[s % 3], lvl=s % 3, ro=int(rng.integers(0, 2)))
        kind = int(rng.integers(0, 6))
        if kind == 1:
            d["reserve"] = 2 if twin else 1  # exact
        elif kind == 2:
            d["reserve"] = 2  # with the twin counted: padded where none is staged
        elif kind == 3:
            d["reserve"], d["explicit"] = 3, max((2 if twin else 1) * T.npos(nch_of(d)) - 1, 0)  # too short by one word
        elif kind == 4:
            d["reserve"], d["explicit"], d["status"] = 3, 5, TERMINATED[s % 3]  # a reservation on a slot that terminates
        elif kind == 5:
            d["reserve"] = 1  # made without the twin: too short where one is staged
        descs.append(d)
    base = 0
    for d in descs:  # the explicit reservations lie below the list's starting count
        if d.get("reserve") == 3:
            d["res_base"], d["res_total"] = base, d.pop("explicit")
            base += d["res_total"]
    return descs, base


@pytest.mark.gpu
@pytest.mark.parametrize("chains", ("off", "on", "bounded"))
def test_stage_lists_of_300_mixed_slots(tiny, chains):
    trk, _ = tiny
    descs, count0 = mixed_slots()
    cfg = dict(cap=count0 + 60000, chain_cap=0 if chains == "off" else len(descs), chain_max_n0=N0 if chains == "bounded" else 0, buf=1, count=count0, chain=0)
    t0 = time.perf_counter()
    out = run_stage(trk, descs, cfg)
    blocks, chain_slots = check_stage_lists(out, descs, cfg)
    print(f"\nchains {chains}: {len(blocks)} blocks, {len(chain_slots)} chain entries, count {out['seg'].count[1]}, {time.perf_counter() - t0:.2f} s")
    assert len(blocks) > 150 and (len(chain_slots) > 0) == (chains != "off")
    if chains == "bounded":  # n0 just below and at the bound chain, just above it does not
        assert {descs[s]["n0"] for s in chain_slots} == {N0 - 1, N0} and any(descs[s]["n0"] == N0 + 1 and nch_of(descs[s]) == 1 for s in blocks)
    # the running slots' states are not touched, no slot was given a tracker, a terminated one (nothing waits) keeps its state too
    rec = slot_records(descs)
    for f in ("status", "lvl", "n", "ppt", "spec_valid", "n0", "residual_only"):
        assert np.array_equal(out["slot_out"][f], rec[f]), f
    assert not out["slot_out"]["tracker_set"].any() and np.array_equal(out["slot_out"]["ticket"], rec["ticket"])


@pytest.mark.gpu
def test_stage_empty_level_books_nothing(tiny):
    trk, _ = tiny
    descs = [dict(n=0, ppt=1, twin=t, reserve=r) for t in (False, True) for r in (0, 1, 2)]
    cfg = dict(cap=64, chain_cap=8, chain_max_n0=0, buf=0, count=0, chain=0)
    out = run_stage(trk, descs, cfg)
    check_stage_lists(out, descs, cfg)
    assert out["seg"].count[0] == 0 and out["seg"].chain[0] == 0 and np.all(out["items"] == T.SENTINEL)
    assert not any(out["ctl"].sched_evals) and not any(out["ctl"].sched_items)


# ---------------------------------------------------------------------------------------------------------------------------------
# C  stage: overflow
# ---------------------------------------------------------------------------------------------------------------------------------
def overflow_slots(kind):
    """Every slot makes its reservation through TickReserve.  "mixed": a third of the slots then abandon it (made without the twin they
    stage, or the slot terminates), a third use it padded, a third exactly.  "abandoned": every slot terminates, so the list is
    reservations turned into no-ops from end to end and the one the list's end falls into is certainly among them.  Twelve further
    one-chunk slots are eligible for the chain area."""
    descs = []
    for s in range(96):
        nch = (2, 9, 17, 3)[s % 4]
        d = dict(n=nch * 256, ppt=1, twin=s % 3 == 0, reserve=1 if s % 3 == 0 else 2)
        if s % 3 == 1 or kind == "abandoned":
            d["status"] = TERMINATED[s % 2]
        descs.append(d)
    descs += [dict(n=200, ppt=1, reserve=1) for _ in range(12)]
    return descs


@pytest.mark.gpu
@pytest.mark.parametrize("short_by", ("room", "one word", "a block", "half"))
@pytest.mark.parametrize("kind", ("mixed", "abandoned"))
def test_stage_overflow_stays_inside_the_item_slots(tiny, kind, short_by):
    """Found by this test: the no-op fill of an abandoned reservation (tick_push's too-short branch and tick_after_step's terminated
    branch) wrote L.items[res_base + i] without the `< L.cap` check the item fill has -- into the chain entries and beyond.  Before the
    fix: mixed / half 470 and 528 no-ops at or behind cap in two runs (the other mixed cases passed by the luck of the order: the list's
    end was a fresh block), abandoned / one word, a block, half: 1, 48 and 895."""
    trk, _ = tiny
    descs = overflow_slots(kind)
    # one chain entry is taken at the start (its word stays as it was): the first word behind cap is nobody's to write
    roomy = dict(cap=1 << 14, chain_cap=13, chain_max_n0=0, buf=0, count=0, chain=1)
    blocks, chains, abandoned, _, _ = expectation(descs, roomy)
    need = sum(b[2] for b in blocks.values()) + abandoned
    assert len(chains) == 12 and need > 1000
    cfg = dict(roomy, cap=need - {"room": 0, "one word": 1, "a block": 48, "half": need // 2}[short_by], chain_cap=13 if short_by == "room" else 12)
    out = run_stage(trk, descs, cfg)
    seg, items, cap, ccap = out["seg"], out["items"], cfg["cap"], cfg["chain_cap"]
    changed = int(np.sum(items[cap + ccap:] != T.SENTINEL)) + int(np.sum((items[cap:cap + ccap] & T.NOOP) != 0))
    print(f"\n{kind}, {short_by}: cap {cap}, count {seg.count[0]}, chain {seg.chain[0]} of {ccap}, overflow {seg.overflow}; "
          f"no-ops at or behind cap: {changed}")
    assert seg.overflow == (0 if short_by == "room" else 1)
    assert seg.count[0] == need and seg.chain[0] == 13
    # no write of the item path at or behind cap: the chain area holds exactly chain_cap - 1 new, distinct, eligible slots behind the one
    # that was there, everything else is untouched
    entries = items[cap + 1:cap + ccap].tolist()
    assert items[cap] == T.SENTINEL, hex(int(items[cap]))
    assert len(set(entries)) == ccap - 1 and set(entries) <= set(chains), [hex(w) for w in entries]
    assert np.all(items[cap + ccap:] == T.SENTINEL), (changed, np.nonzero(items[cap + ccap:] != T.SENTINEL)[0][:8])
    T.check_list(items, cap, ccap, 0, 1, seg.count[0], seg.chain[0], blocks, chains, abandoned, overflowed=short_by != "room")
    if short_by == "room":
        check_stage_lists(out, descs, cfg)


# ---------------------------------------------------------------------------------------------------------------------------------
# D  stage: retire and refill
# ---------------------------------------------------------------------------------------------------------------------------------
def pending_records(n, coarsest, seed=3):
    from direct_stereo_slam_amd.tracker import TICK_PENDING

    rng = np.random.default_rng(seed)
    p = np.zeros(n, TICK_PENDING)
    for k, a in enumerate(p):
        q = rng.standard_normal(4)
        a["pose"] = np.concatenate([q / np.linalg.norm(q), rng.standard_normal(3)])
        a["aff"], a["min_res"] = rng.standard_normal(2), rng.uniform(1, 9, 6)
        a["scale"], a["coarsest"], a["ticket"] = 1.0 + k, coarsest, 5000 + k
    return p


RESULT_COPIED = ("cur", "aff_cur", "last_residuals", "flow", "scale_cur", "evals", "evals_ro", "rounds")


@pytest.mark.gpu
@pytest.mark.parametrize("base", (0, RING - 2, 2**32 - 1, 2**32 + RING - 1))
@pytest.mark.parametrize("R", (1, 64, 200))
def test_retire_and_refill(tiny, R, base):
    trk, sc = tiny
    coarsest = sc.nl - 1
    n_lvl = len(sc.tpl[0][coarsest])
    _, ppt, nch_start = reduction_geometry(n_lvl, 0)
    assert nch_start >= 1
    # R terminating slots among running ones
    descs = []
    for s in range(R + R // 2 + 1):
        descs.append(dict(n=512, ppt=1, lvl=1) if s % 3 == 2 or s >= R + R // 2 else dict(n=0, ppt=0, status=TERMINATED[s % 3]))
    retiring = [s for s, d in enumerate(descs) if "status" in d]
    assert len(retiring) == R
    rec = slot_records(descs)
    cfg = dict(cap=1 << 14, chain_cap=0, chain_max_n0=0, buf=0, count=0, chain=0)
    baseline = None
    for P in sorted({0, 1, R - 1, R, R + 5}):
        stepped = P % 2
        pend = pending_records(P, coarsest)
        ctl = dict(pending_head=base, pending_count=base + P, retired=base + 3, ring=RING)
        out = run_stage(trk, descs, cfg, ctl, pend, stepped)
        so, mc = out["slot_out"], out["ctl"]
        took = min(R, P)
        assert (mc.retired, mc.pending_head, mc.pending_count, mc.ring) == (base + 3 + R, base + took, base + P, RING), (R, P, base)
        # the result ring: every retiring slot's ticket once, at consecutive indices modulo the ring, every field the crafted state's bits
        res = out["results"]
        at = [(base + 3 + k) % RING for k in range(R)]
        assert sorted(res["ticket"][at].tolist()) == sorted(rec["ticket"][retiring].tolist())
        by_ticket = {int(t): i for i, t in zip(retiring, rec["ticket"][retiring])}
        for r in res[at]:
            src = rec[by_ticket[int(r["ticket"])]]
            assert r["status"] == src["status"] and r["ticks"] == src["ticks"]
            for f in RESULT_COPIED:
                assert np.asarray(r[f]).tobytes() == np.asarray(src[f]).tobytes(), f
        rest = np.delete(np.arange(RING), at)
        assert np.all(res[rest].view(np.uint8) == 0xA5)
        # the admitted slots: distinct entries covering exactly [head, head + min(R, P))
        admitted = [s for s in retiring if so["ticket"][s] >= 5000]
        assert sorted(int(so["ticket"][s]) - 5000 for s in admitted) == list(range(took)), (R, P, base)
        for s in admitted:
            k = int(so["ticket"][s]) - 5000
            assert so["tracker_set"][s] == 1 and so["status"][s] == T.ST_RUNNING and so["stepped"][s] == stepped and so["lvl"][s] == coarsest
            a, b = out["state_raw"][s].copy(), out["start_raw"][k].copy()
            assert b[STEPPED_OFFSET:STEPPED_OFFSET + 4].view(np.int32)[0] == 0
            a[STEPPED_OFFSET:STEPPED_OFFSET + 4] = 0
            assert a.tobytes() == b.tobytes(), (s, k, np.nonzero(a != b)[0][:8])  # LM_OP_START's state byte for byte, but for `stepped`
            assert (so["n"][s], so["ppt"][s], so["n0"][s]) == (n_lvl, ppt, len(sc.tpl[0][0]))
            assert np.array_equal(out["state_out"]["cur"][s], pend["pose"][k]) and out["state_out"]["scale_cur"][s] == pend["scale"][k]
        # slots that found nothing waiting keep their terminated state; running slots are not touched either
        if baseline is None:
            baseline = out["state_raw"].copy()
            assert not admitted and not so["tracker_set"].any()
            for f in ("cur", "aff_cur", "flow", "evals", "rounds"):
                assert np.asarray(out["state_out"][f]).tobytes() == np.asarray(rec[f]).tobytes(), f
            assert np.array_equal(so["status"], rec["status"])
        others = [s for s in range(len(descs)) if s not in admitted]
        assert np.array_equal(out["state_raw"][others], baseline[others])
        assert np.array_equal(so["ticket"][others], rec["ticket"][others]) and not so["tracker_set"][others].any()
        # the list: the running slots' evaluations and the first evaluation of every admitted problem, at the tracker's coarsest level
        blocks, chains, abandoned, pre, sched = expectation(descs, cfg)
        for s in admitted:
            blocks[s] = (nch_start, False, T.npos(nch_start))
            sched[0, coarsest] += 1
            sched[2, coarsest] += T.npos(nch_start)
        T.check_list(out["items"], cfg["cap"], 0, 0, 0, out["seg"].count[0], out["seg"].chain[0], blocks, chains, abandoned)
        assert out["seg"].overflow == 0
        assert np.array_equal(np.array([list(mc.sched_evals), list(mc.sched_ro), list(mc.sched_items)]), sched)


# ---------------------------------------------------------------------------------------------------------------------------------
# E  step: the production tick_lm_kernel on the LM machine's case table
# ---------------------------------------------------------------------------------------------------------------------------------
def step_slots(n, stepped=None, idle=None):
    from direct_stereo_slam_amd.tracker import TICK_SLOT

    a = np.zeros(n, TICK_SLOT)
    a["status"], a["ticket"] = T.ST_RUNNING, 1000 + np.arange(n)
    if stepped is not None:
        a["stepped"][stepped] = 1
    if idle is not None:
        a["status"][idle] = T.ST_IDLE
    return a


def same_states(a, b):
    """two arrays of LM_STEP_STATE records, byte for byte but for nch (the tick entries report the chunks of the evaluation now staged)"""
    a, b = a.copy(), b.copy()
    a["nch"], b["nch"] = 0, 0
    return [i for i in range(len(a)) if a[i].tobytes() != b[i].tobytes()]


@pytest.mark.gpu
@pytest.mark.parametrize("speculate", (0, 2))
@pytest.mark.parametrize("opts", (0, 1, 2, 3))
def test_tick_lm_kernel_on_the_lm_machine_table(trackers, opts, speculate):  # noqa: F811
    t0 = time.perf_counter()
    rows = padded = proposing = 0
    for (pkey, mode, lvl, _), cases in grouped([c for c in Cs.cases() if c["mode"] in (0, 1)]).items():
        trk, params = trackers(pkey), Cs.ref_params(pkey)
        P, spec_off = partial_block(cases, True)  # the speculative partials half a block behind, as tick_lm_kernel reads them
        states = pack([c["state"] for c in cases], [c["nch"] for c in cases])
        want = trk.diagLmStep(mode, lvl, states, P, spec=speculate == 2, spec_off=spec_off, helper=bool(opts & 1))
        n = len(cases)
        cfg = dict(cap=1 << 16, chain_cap=n if lvl % 2 else 0, chain_max_n0=0, buf=1, count=5, chain=0)
        ring = 1024  # (room for every row of a group to retire)
        ctl = dict(pending_head=0, pending_count=0, retired=2**32 - 1, ring=ring)
        assert n <= ring
        out = trk.diagTickStep(mode, lvl, states, step_slots(n), P, speculate, opts, cfg, ctl)
        diff = same_states(out["state_out"], want)
        assert not diff, (pkey, mode, lvl, [cases[i]["row"] for i in diff][:5])
        so = out["slot_out"]
        assert not so["stepped"].any() and np.array_equal(so["status"], want["status"]) and np.array_equal(so["lvl"], want["lvl"])
        # the list is what the rules build from the stored states; the early reservation as the step's hook is documented: made when the
        # step proposes (the state is left running, in the iteration phase), with the twin counted where one may be staged
        fixed = params.fixed_schedule > 0
        max_it = params.fixed_schedule if fixed else params.max_iterations[lvl]
        descs = []
        for i, c in enumerate(cases):
            running = want["status"][i] == M.ST_RUNNING
            proposes = running and want["phase"][i] == M.PH_ITER
            want_twin = proposes and speculate == 2 and not fixed and want["iteration"][i] + 1 < max_it
            d = dict(n=int(so["n"][i]), ppt=int(so["ppt"][i]), twin=bool(so["spec_valid"][i]), n0=int(so["n0"][i]), lvl=int(so["lvl"][i]),
                     ro=int(so["residual_only"][i]), status=int(want["status"][i]))
            if proposes:
                assert (d["n"], d["lvl"]) == (c["nch"] * 256, lvl), c["row"]  # the next evaluation is one of the level the step stood on
                if opts & 2:
                    d["reserve"] = 2 if want_twin else 1
                    nch = nch_of(d)
                    reserved = T.reservation(cfg["chain_cap"], 0, nch, want_twin, d["n0"])
                    used = 0 if T.chain_eligible(cfg["chain_cap"], 0, nch, d["twin"], d["n0"]) else (2 if d["twin"] else 1) * T.npos(nch)
                    # "a reservation is never too short": with none made (the chain area was to take the evaluation) nothing may be needed
                    assert reserved >= used or reserved == 0 and not d["twin"], (c["row"], reserved, used)
                    padded += int(reserved > used and used > 0)
                proposing += 1
            assert not d["twin"] or proposes, c["row"]  # a twin is staged by a proposal only
            descs.append(d)
        blocks, chains, abandoned, _, sched = expectation(descs, cfg)
        # "a step that proposes does not terminate": the count shows no reservation beyond the running rows' blocks and padding
        seg = out["seg"]
        T.check_list(out["items"], cfg["cap"], cfg["chain_cap"], 5, 0, seg.count[1], seg.chain[1], blocks, chains, abandoned)
        assert seg.overflow == 0 and (seg.count[0], seg.chain[0]) == (0, 0)  # slot 0 cleared the list the evaluation launch consumed
        mc = out["ctl"]
        assert np.array_equal(np.array([list(mc.sched_evals), list(mc.sched_ro), list(mc.sched_items)]), sched)
        # the terminated rows retired: results for each, none admitted (nothing waits)
        done = [i for i in range(n) if want["status"][i] != M.ST_RUNNING]
        assert mc.retired == 2**32 - 1 + len(done) and mc.pending_head == 0
        at = [(2**32 - 1 + k) % ring for k in range(len(done))]
        assert sorted(out["results"]["ticket"][at].tolist()) == [1000 + i for i in done]
        for r in out["results"][at]:
            i = int(r["ticket"]) - 1000
            assert r["status"] == want["status"][i] and r["ticks"] == want["ticks"][i]
            for f in RESULT_COPIED:
                assert np.asarray(r[f]).tobytes() == np.asarray(want[f][i]).tobytes(), (cases[i]["row"], f)
        rows += n
    print(f"\nopts {opts} speculate {speculate}: {rows} rows, {proposing} propose, {padded} with a padded twin, {time.perf_counter() - t0:.2f} s")
    assert rows == len([c for c in Cs.cases() if c["mode"] in (0, 1)]) and proposing >= 4
    assert padded == 0 or (opts & 2 and speculate == 2)


@pytest.mark.gpu
def test_tick_lm_kernel_leaves_stepped_and_free_slots_alone(trackers):  # noqa: F811
    pkey = ("ab", 0, None)
    trk = trackers(pkey)
    cases = [c for c in Cs.cases() if c["pkey"] == pkey and c["mode"] == 0 and c["lvl"] == 1][:12]
    assert len(cases) == 12
    P, _ = partial_block(cases, True)
    states = pack([c["state"] for c in cases], [c["nch"] for c in cases])
    cfg = dict(cap=1 << 14, chain_cap=0, chain_max_n0=0, buf=0, count=0, chain=0)
    ctl = dict(pending_head=0, pending_count=0, retired=0, ring=RING)
    filled = trk.diagTickStep(0, 1, states, step_slots(12, stepped=[2, 5], idle=[3, 7]), P, 2, 7, cfg, ctl)  # opts bit 2: no LM launch
    assert filled["slot_out"]["stepped"].tolist() == [int(i in (2, 5)) for i in range(12)] and filled["seg"].count[1] == 7
    out = trk.diagTickStep(0, 1, states, step_slots(12, stepped=[2, 5], idle=[3, 7]), P, 2, 3, cfg, ctl)
    plain = trk.diagTickStep(0, 1, states, step_slots(12), P, 2, 3, cfg, ctl)
    for i in range(12):
        a, b = out["state_raw"][i].copy(), filled["state_raw"][i]
        if i in (2, 5):  # stepped inside the evaluation launch: left alone but for the flag
            assert a[STEPPED_OFFSET:STEPPED_OFFSET + 4].view(np.int32)[0] == 0
            a[STEPPED_OFFSET:STEPPED_OFFSET + 4] = b[STEPPED_OFFSET:STEPPED_OFFSET + 4]
            assert a.tobytes() == b.tobytes()
        elif i in (3, 7):  # a free slot
            assert a.tobytes() == b.tobytes()
        else:
            assert a.tobytes() == plain["state_raw"][i].tobytes() and a.tobytes() != b.tobytes()
    live = [i for i in range(12) if i not in (2, 3, 5, 7)]
    descs = [dict(n=int(out["slot_out"]["n"][i]), ppt=int(out["slot_out"]["ppt"][i]), twin=bool(out["slot_out"]["spec_valid"][i]),
                  lvl=int(out["slot_out"]["lvl"][i]), status=int(out["slot_out"]["status"][i]) if i in live else T.ST_IDLE) for i in range(12)]
    blocks, chains, _, _, _ = expectation(descs, cfg)
    seg = out["seg"]
    padding = seg.count[0] - sum(b[2] for b in blocks.values())  # (twins reserved and not staged)
    assert padding >= 0 and set(blocks) <= set(live) and (seg.count[1], seg.chain[1]) == (0, 0)
    got_slots = {T.decode(int(w))[1] for w in out["items"][:seg.count[0]] if T.decode(int(w))[0] == "item"}
    assert got_slots == set(blocks)


# ---------------------------------------------------------------------------------------------------------------------------------
# F  admit
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("head", (0, 2**32 + RING - 2))
def test_admit_behind_the_reserve_table(tiny, ctx, head):
    trk, sc = tiny
    coarsest = sc.nl - 1
    n, P_wait = 70, 23
    running = (np.arange(n) % 3 == 0).astype(np.uint8)
    idx, heads, _ = ctx.diagTickReserve([(0, 0, n)], running, [head, 0], [head + P_wait, 0])
    assert heads[0] == head + P_wait and int((idx >= 0).sum()) == P_wait
    from direct_stereo_slam_amd.tracker import LM_STEP_STATE

    states = pack([M.new_state(coarsest)] * n, [1] * n)
    assert states.dtype == LM_STEP_STATE
    P = np.zeros((n, 2 * 64 * 8), np.float32)
    slots = step_slots(n, idle=np.nonzero(running == 0)[0])
    pend = pending_records(P_wait, coarsest)
    cfg = dict(cap=1 << 12, chain_cap=n, chain_max_n0=0, buf=0, count=0, chain=0)
    ctl = dict(pending_head=head, pending_count=head + P_wait, retired=0, ring=RING)
    before = trk.diagTickStep(0, coarsest, states, slots, P, 0, 4, cfg, ctl, pend, admit_idx=np.full(n, -1, np.int64))
    out = trk.diagTickStep(0, coarsest, states, slots, P, 0, 4, cfg, ctl, pend, admit_idx=idx)
    so = out["slot_out"]
    n_lvl = len(sc.tpl[0][coarsest])
    _, ppt, nch_start = reduction_geometry(n_lvl, 0)
    for s in range(n):
        if idx[s] < 0:  # untouched, byte for byte
            assert out["state_raw"][s].tobytes() == before["state_raw"][s].tobytes() and not so["tracker_set"][s] and so["ticket"][s] == 1000 + s
            continue
        k = int(idx[s]) - head
        assert so["ticket"][s] == 5000 + k and so["tracker_set"][s] == 1 and so["stepped"][s] == 0 and so["status"][s] == T.ST_RUNNING
        assert (so["lvl"][s], so["n"][s], so["ppt"][s]) == (coarsest, n_lvl, ppt)
        # the fields LM_OP_START writes are its bits; what it does not write keeps the slot's old bits (none is read)
        a, b, old = out["state_raw"][s], out["start_raw"][k], before["state_raw"][s]
        differs = a != b
        assert np.array_equal(a[differs], old[differs]), s
        assert np.array_equal(out["state_out"]["cur"][s], pend["pose"][k]) and np.array_equal(out["state_out"]["min_res"][s], pend["min_res"][k])
    admitted = [s for s in range(n) if idx[s] >= 0]
    blocks = {} if nch_start == 1 else {s: (nch_start, False, T.npos(nch_start)) for s in admitted}
    T.check_list(out["items"], cfg["cap"], n, 0, 0, out["seg"].count[0], out["seg"].chain[0], blocks, admitted if nch_start == 1 else [])
    mc = out["ctl"]
    assert (mc.pending_head, mc.retired) == (head, 0)  # (the reserve kernel moved the head; the admission does not)


# ---------------------------------------------------------------------------------------------------------------------------------
# G  argument errors
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_invalid_arguments_are_refused_by_name(tiny, ctx):
    from direct_stereo_slam_amd._lib import DsmError

    trk, sc = tiny
    good_cfg = dict(cap=64, chain_cap=4, chain_max_n0=0, buf=0, count=0, chain=0)
    good_ctl = dict(pending_head=0, pending_count=0, retired=0, ring=RING)
    one = [dict(n=256, ppt=1)]

    def refused(name, fn):
        with pytest.raises(DsmError) as e:
            fn()
        assert name in str(e.value), str(e.value)

    for bad in (dict(cap=-1), dict(chain_cap=-1), dict(count=-1), dict(chain=-1), dict(count=65), dict(chain=5), dict(buf=2)):
        refused("dsm_diag_tick_stage", lambda: run_stage(trk, one, dict(good_cfg, **bad)))
    for bad in (dict(ring=0), dict(ring=48), dict(ring=-64), dict(pending_head=-1), dict(retired=-1), dict(pending_count=1)):
        refused("dsm_diag_tick_stage", lambda: run_stage(trk, one, good_cfg, dict(good_ctl, **bad)))
    for bad in (dict(n=4096 * 256, ppt=1), dict(n=-1, ppt=1), dict(n=256, ppt=0), dict(n=256, ppt=1, lvl=6), dict(n=256, ppt=1, status=5),
                dict(n=256, ppt=1, reserve=4), dict(n=256, ppt=1, reserve=3, res_base=-1, res_total=2), dict(n=256, ppt=1, reserve=3, res_base=0, res_total=-2),
                dict(n=256, ppt=1, reserve=3, res_base=1 << 20, res_total=2)):
        refused("dsm_diag_tick_stage", lambda: run_stage(trk, [bad], good_cfg))
    refused("dsm_diag_tick_stage", lambda: run_stage(trk, one, good_cfg, mode=2))
    refused("dsm_diag_tick_stage", lambda: run_stage(trk, one, good_cfg, dict(good_ctl, ring=2), pending_records(3, 0)))  # more entries than the ring
    refused("dsm_diag_tick_stage", lambda: run_stage(trk, one, good_cfg, good_ctl, pending_records(1, sc.nl)))  # coarsest level out of range
    for segs, nslots in (([(2, 0, 4)], 8), ([(0, -1, 4)], 8), ([(0, 0, -4)], 8), ([(0, 6, 4)], 8), ([(0, 0, 1)] * 21, 8)):
        refused("dsm_diag_tick_reserve", lambda: ctx.diagTickReserve(segs, np.zeros(nslots, np.uint8), [0, 0], [1, 1]))
    states = pack([M.new_state(0)], [1])
    P = np.zeros((1, 128), np.float32)
    for kw in (dict(lvl=sc.nl), dict(speculate=3), dict(opts=8), dict(cfg=dict(good_cfg, cap=-1)), dict(ctl=dict(good_ctl, ring=3)),
               dict(P=np.zeros((1, 64), np.float32)), dict(admit=np.array([5], np.int64))):
        refused("dsm_diag_tick_step", lambda: trk.diagTickStep(0, kw.get("lvl", 0), states, step_slots(1), kw.get("P", P), kw.get("speculate", 0),
                                                               kw.get("opts", 0), kw.get("cfg", good_cfg), kw.get("ctl", good_ctl), None, kw.get("admit")))
    # and nothing was written by a refused call: the wrapper's first call asks for the length only; a direct call with outputs
    from direct_stereo_slam_amd import _lib

    items = np.full(16, 0x11111111, np.uint32)
    length, sb = C.c_int(16), C.c_int(-7)
    rec = slot_records(one)
    lc, mc = _lib.TickListCfg(**dict(good_cfg, cap=-1)), _lib.TickModeCtl(ring=RING)
    seg, mco = _lib.TickSegCtl(), _lib.TickModeCtl()
    raw = np.zeros(8192, np.uint8)
    rc = trk.L.dsm_diag_tick_stage(trk.h, 0, 1, rec.ctypes.data_as(C.POINTER(_lib.TickSlot)), C.byref(lc), C.byref(mc), 0, None, 0,
                                   items.ctypes.data_as(C.POINTER(C.c_uint)), C.byref(length), C.byref(seg), C.byref(mco), None, None, None,
                                   raw.ctypes.data_as(C.POINTER(C.c_ubyte)), C.byref(sb), None)
    assert rc == -1 and np.all(items == 0x11111111) and (length.value, sb.value) == (16, -7) and not raw.any()
