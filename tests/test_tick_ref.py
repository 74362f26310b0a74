"""CPU: the reference of the tick engine's list and ring rules (tests/_tick_ref.py) against the properties the rules exist for --
every chunk of an evaluation exactly once in its block, every waiting problem handed out exactly once, an item list that
tick_setup's sizing cannot overflow -- and the proof that each of these tests notices a reference that states a rule wrongly."""
import numpy as np
import pytest

import _tick_ref as T
from _gn_f64 import pts_per_thread

NFREE = (0, 1, 2, 3, 7, 64, 255, 256, 257, 600)
AVAIL = (0, 1, 2, 3, 5, 17, 255, 256, 257, 1000, 5000)


def check_banding():
    for nch in range(600):
        chunks = [T.position_chunk(nch, p) for p in range(T.npos(nch))]
        real = [c for c in chunks if c is not None]
        assert sorted(real) == list(range(nch)), nch  # every chunk once: a bijection of the positions onto a superset of [0, nch)
        assert len(chunks) == (nch if nch < 8 else 8 * ((nch + 7) // 8))
        if nch >= 8:  # XCD x (positions p = x mod 8) walks one band of consecutive chunks
            per = (nch + 7) // 8
            for x in range(8):
                band = [c for c in chunks[x::8] if c is not None]
                assert band == list(range(x * per, min((x + 1) * per, nch))), (nch, x)
    # nine chunks: bands of two; XCD 4 holds chunk 8 alone, XCDs 5-7 nothing
    N = None
    assert [T.position_chunk(9, p) for p in range(16)] == [0, 2, 4, 6, 8, N, N, N, 1, 3, 5, 7, N, N, N, N]


def check_shares(draws=3000):
    rng = np.random.default_rng(20)
    worst = 0.0
    for _ in range(draws):
        nseg = int(rng.integers(1, T.MAX_SEGS + 1))
        nfree = [int(rng.choice(NFREE)) for _ in range(nseg)]
        A = int(rng.choice(AVAIL))
        F = sum(nfree)
        take = T.shares(nfree, A)
        assert sum(take) == min(A, F), (nfree, A, take)
        assert all(0 <= t <= f for t, f in zip(take, nfree)), (nfree, A, take)
        if F:
            dev = max(abs(t - min(A, F) * f / F) for t, f in zip(take, nfree))
            worst = max(worst, dev)
            assert dev <= 1, (nfree, A, take)
    return worst


def check_handout(draws=300):
    """the indices the free slots get are distinct and contiguous from the head, per kind, in segment and slot order"""
    rng = np.random.default_rng(21)
    for _ in range(draws):
        nseg = int(rng.integers(1, 7))
        segs, i0 = [], 0
        for _ in range(nseg):
            ns = int(rng.choice((0, 1, 3, 64, 65, 257)))
            segs.append((int(rng.integers(0, 2)), i0, ns))
            i0 += ns
        running = (rng.random(max(i0, 1)) < rng.choice((0.0, 0.5, 0.9, 1.0))).astype(np.uint8)
        head = [int(rng.choice((0, 5, 2**32 - 2))), int(rng.choice((0, 61)))]
        count = [h + int(rng.choice((-1, 0, 1, 7, 300, 5000))) for h in head]
        idx, heads = T.reserve(segs, running, head, count)
        for mode in (0, 1):
            got = [idx[j] for m, a, ns in segs if m == mode for j in range(a, a + ns) if idx[j] >= 0]
            free = sum(1 for m, a, ns in segs if m == mode for j in range(a, a + ns) if not running[j])
            assert got == list(range(head[mode], head[mode] + min(free, max(count[mode] - head[mode], 0)))), (segs, head, count, got[:8])
            assert heads[mode] == head[mode] + len(got)
        assert all(idx[j] == -1 for j in range(i0) if running[j])


def check_block_layout():
    for nch in (1, 2, 7, 8, 9, 17, 64):
        for twin in (False, True):
            words = T.block(5, nch, twin, length=2 * T.npos(nch) + 3)
            n = T.npos(nch)
            main, second, pad = words[:n], words[n:2 * n] if twin else [], words[(2 if twin else 1) * n:]
            assert [T.decode(w)[2:] for w in main if w != T.NOOP] == [(T.position_chunk(nch, p), False) for p in range(n) if T.position_chunk(nch, p) is not None]
            assert all(w == T.NOOP for w in pad) and len(pad) == (3 if twin else n + 3)
            if twin:  # the twin's positions lie BEHIND the main ones, same chunks, the candidate bit set
                assert [w if w == T.NOOP else w | T.CAND for w in main] == second and any(w & T.CAND for w in second)
    # and a list built from blocks passes its own check; one with two slots' blocks swapped in content does not
    slots = [(0, 9, True, 100, 32), (1, 1, False, 100, 0), (2, 1, False, 9000, 0), (3, 17, False, 100, 48), (4, 2, True, 100, 2), (5, 0, False, 100, 0)]
    items, count, chain, blocks, chains, abandoned = T.build_list(400, 4, 5000, 3, slots)
    assert chains == [1] and blocks[2] == (1, False, 1) and blocks[3] == (17, False, 48) and blocks[4] == (2, True, 4) and abandoned == 2
    T.check_list(items, 400, 4, 3, 0, count, chain, blocks, chains, abandoned)
    bad = list(items)
    i = bad.index(T.item(0, 2, False))
    bad[i] = T.item(0, 1, False)
    with pytest.raises(AssertionError):
        T.check_list(bad, 400, 4, 3, 0, count, chain, blocks, chains, abandoned)


def test_banding_is_a_bijection():
    check_banding()


def test_share_rule():
    worst = check_shares()
    assert worst <= 1.0
    check_handout()


def test_block_layout():
    check_block_layout()


@pytest.mark.parametrize("w,h", ((64, 48), (640, 480), (1241, 376), (1920, 1080)))
def test_sizing_cannot_overflow(w, h):
    """tick_setup sizes a segment's list as ns * 2 * maxpos + 64, maxpos = max_chunks_upto(w h) rounded up to eight"""
    n = np.arange(0, w * h + 1, dtype=np.int64)
    prefix = None
    for g in (0, 1, 2):
        ppt = np.array([pts_per_thread(int(e), g) for e in (0, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4095, 4096, 4097, 16383, 16384, 65535, 65536,
                                                           262143, 262144)])  # (spot check of the vectorised table below against the scalar one)
        lat = np.where(n >= 256 * 1024, 16, np.where(n >= 64 * 1024, 8, np.where(n >= 16 * 1024, 4, np.where(n >= 4 * 1024, 2, 1))))
        thr = np.where(n > 2048, 16, np.where(n > 1024, 8, np.where(n > 512, 4, np.where(n > 256, 2, 1))))
        p = lat if g == 1 else thr if g == 0 else np.where(n > 4096, lat, thr)
        for e, want in zip((0, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4095, 4096, 4097, 16383, 16384, 65535, 65536, 262143, 262144), ppt):
            if e <= w * h:
                assert p[e] == want, (g, e)
        nch = (n + 256 * p - 1) // (256 * p)
        prefix = np.maximum.accumulate(nch) if prefix is None else np.maximum(prefix, np.maximum.accumulate(nch))
        maxpos = 8 * ((T.max_chunks_upto(w * h) + 7) // 8)
        npos = np.where(nch < 8, nch, 8 * ((nch + 7) // 8))
        assert int(npos.max()) <= maxpos  # one slot's worst block, 2 npos, never exceeds 2 maxpos: ns slots fit ns * 2 * maxpos (+ 64)
    caps = [c for c in (1, 255, 256, 257, 512, 513, 2048, 2049, 4095, 4096, 4097, 4352, 16383, 16384, 65535, 65536, 70000, 262143, 262144, 300000, w * h)
            if c <= w * h]
    for cap in caps:  # the restated rule against the brute-force maximum over every n <= cap and the three tables
        assert T.max_chunks_upto(cap) == int(prefix[cap]), cap


# ---- each deliberate break of the reference makes one of the tests above fail ----
def test_swapped_band_formula_is_noticed(monkeypatch):
    def swapped(nch, p):
        if nch < 8:
            return p
        per = -(-nch // 8)
        c = (p >> 3) * per + (p & 7)
        return c if c < nch else None

    monkeypatch.setattr(T, "position_chunk", swapped)
    with pytest.raises(AssertionError):
        check_banding()


def test_dropped_remainder_loop_is_noticed(monkeypatch):
    def floor_only(nfree, avail):
        total = sum(nfree)
        return list(nfree) if total <= avail else [avail * f // total for f in nfree]

    monkeypatch.setattr(T, "shares", floor_only)
    with pytest.raises(AssertionError):
        check_shares()


def test_rank_off_by_one_is_noticed(monkeypatch):
    monkeypatch.setattr(T, "rank_index", lambda base, rank: base + rank + 1)
    with pytest.raises(AssertionError):
        check_handout()


def test_twin_before_main_is_noticed(monkeypatch):
    plain = T.block

    def twin_first(slot, nch, twin, length=None):
        words = plain(slot, nch, twin, length)
        n = T.npos(nch)
        return words[n:2 * n] + words[:n] + words[2 * n:] if twin else words

    monkeypatch.setattr(T, "block", twin_first)
    with pytest.raises(AssertionError):
        check_block_layout()
