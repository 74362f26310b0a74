"""search_ringkey of many sequences in one call, each against its own index (dsm_ringdb_query_then_enqueue_many): bit for bit the
per-sequence dsm_ringdb_query_then_enqueue calls in call order -- candidates, counts, and every index's entries, size and delay queue
afterwards -- on twin indexes, and against the oracle's brute force."""
import ctypes as C

import numpy as np
import pytest

from direct_stereo_slam_amd import _lib
from direct_stereo_slam_amd.ringdb import LoopBatch, RingKeyDB, query_then_enqueue_many
from oracle import oracle as O

from test_oracle_ringkey import ring_keys

ERR_INVALID = -1  # DSM_ERR_INVALID


def test_invalid_calls_fail_before_any_device_work(built):
    """CPU: argument errors are reported without touching a device"""
    L = _lib.load()
    cand, nc = (C.c_int * 3)(), (C.c_int * 1)()
    key = (C.c_float * 20)()
    assert L.dsm_ringdb_query_then_enqueue_many(0, None, key, cand, nc) == ERR_INVALID
    assert L.dsm_ringdb_query_then_enqueue_many(1, None, key, cand, nc) == ERR_INVALID
    assert L.dsm_ringdb_query_then_enqueue_many(1, (C.c_void_p * 1)(None), key, cand, nc) == ERR_INVALID
    assert L.dsm_loop_detect_batch_many(None, 1, None, None, 40.0, 60, 20, cand, nc) == ERR_INVALID
    with pytest.raises(ValueError):
        LoopBatch(None, [], 40.0, db=object(), dbs=[])  # one index for all jobs, or one per job: not both


def _revisit(rng, content, dim):
    """a key near one already in the index (one element moved by a sector) or, one time in three, a new place"""
    if len(content) == 0 or rng.random() < 0.33:
        return (rng.integers(0, 61, dim) / 60.0).astype(np.float32)
    k = content[rng.integers(len(content))].copy()
    d = rng.integers(dim)
    k[d] = np.float32(k[d] - 1 / 60 if k[d] >= 1 else k[d] + 1 / 60)
    return k


class Seq:
    """one sequence: its index, a twin driven by the single-key call, and the keys it has seen"""

    def __init__(self, ctx, n_keys, margin, seed, dim=20, capacity=None, dummy=None):
        keys = ring_keys(n_keys, seed=seed)[:, :dim].copy() if n_keys else np.zeros((0, dim), np.float32)
        cap = capacity or max(1024, n_keys + 16)
        self.db, self.twin = (RingKeyDB(ctx, dim=dim, margin=margin, capacity=cap, dummy=dummy) for _ in range(2))
        if n_keys:
            self.db.add_points(keys)
            self.twin.add_points(keys)
        self.content, self.dim = list(keys), dim


def _drive(ctx, seqs, rng, calls, orc=None):
    """random traffic: each call leaves some sequences out and repeats some (up to twice); returns the number of candidates"""
    n_cand = 0
    for c in range(calls):
        picks = []
        for s, q in enumerate(seqs):
            r = rng.random()
            if r < 0.2:
                continue
            picks += [s] * (2 if r > 0.85 else 1)
        if not picks:
            picks = [0]
        rng.shuffle(picks)
        keys = [_revisit(rng, seqs[s].content, seqs[s].dim) for s in picks]
        got = query_then_enqueue_many([seqs[s].db for s in picks], keys)
        for s, key, g in zip(picks, keys, got):
            want = seqs[s].twin.search_ringkey(key)
            assert g == want, (c, s)
            if orc is not None and s == orc[0]:
                assert g == orc[1].query_then_enqueue(key)
            seqs[s].content.append(key)
            n_cand += len(g)
    return n_cand


def _same_indexes(seqs, rng):
    for q in seqs:
        assert q.db.size() == q.twin.size()
        probe = np.stack([_revisit(rng, q.content, q.dim) for _ in range(8)])
        assert np.array_equal(q.db.knn_packed_host(probe), q.twin.knn_packed_host(probe))


@pytest.mark.gpu
def test_many_indexes_equal_the_sequential_calls(ctx):
    """11 indexes from the dummy alone to 20000 keys; margins 3-5 so that keys mature inside calls; the 1020-entry index (capacity
    1024) grows inside a call, before its scan"""
    k = 3
    sizes = [0, k - 2, k - 1, k, 1022, 1023, 1024, 4096, 19999, 1019, 300]  # keys added; entries = keys + the dummy
    rng = np.random.default_rng(5)
    dummy = np.full(20, 0.5, np.float32)
    seqs = [Seq(ctx, n, margin=3 + i % 3, seed=100 + i, capacity=1024 if n == 1019 else None, dummy=dummy) for i, n in enumerate(sizes)]
    assert sorted(q.db.size() for q in seqs) == sorted([1, k - 1, k, k + 1, 1023, 1024, 1025, 4097, 20000, 1020, 301])
    orc = O.OracleRingDB(margin=3 + 6 % 3, dummy=dummy)  # sequence 6 (1025 entries) also against the oracle
    orc.add_points(ring_keys(sizes[6], seed=106))
    n_cand = _drive(ctx, seqs, rng, 60, orc=(6, orc))
    assert n_cand > 100
    assert seqs[9].db.size() > 1024  # grew past its capacity through keys that matured inside calls
    assert orc.size() == seqs[6].db.size()
    _same_indexes(seqs, rng)


@pytest.mark.gpu
def test_ties_and_duplicates_smaller_ordinal_first(ctx):
    """identical keys in one index, spread over several scan slices: equal distances list the smaller ordinal first"""
    keys = ring_keys(3000, seed=9)
    dup = keys[17].copy()
    for i in (17, 40, 1500, 2999):
        keys[i] = dup
    near = dup.copy()
    near[3] += np.float32(1 / 60)
    a, b = Seq(ctx, 0, margin=4, seed=0), Seq(ctx, 0, margin=4, seed=0)
    for q in (a, b):
        q.db.add_points(keys)
        q.twin.add_points(keys)
    got = query_then_enqueue_many([a.db, b.db, a.db], [dup, near, near])
    # keys[i] is ordinal i + 1 (the dummy is ordinal 0) and is reported as i: the three smallest ordinals of four ties, in three slices
    assert got[0] == [17, 40, 1500]
    assert got[1] == [17, 40, 1500] and got[2] == [17, 40, 1500]
    assert got == [a.twin.search_ringkey(dup), b.twin.search_ringkey(near), a.twin.search_ringkey(near)]


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [12, 7])
def test_other_dimensions(ctx, dim):
    rng = np.random.default_rng(dim)
    seqs = [Seq(ctx, n, margin=3, seed=200 + n, dim=dim) for n in (0, 5, 1500, 5000)]
    assert _drive(ctx, seqs, rng, 25) > 10
    _same_indexes(seqs, rng)


@pytest.mark.gpu
def test_each_sequence_sees_only_its_own_keyframes(ctx):
    """two sequences with identical key streams: with one index each, every query is handed exactly the lists its own sequence's
    calls give.  Contrast (today's batched search over one shared index): the same traffic returns keyframes of the other sequence
    and ordinals that do not index the caller's own loop_frames_"""
    rng = np.random.default_rng(3)
    margin = 3
    stream = []
    for i in range(40):
        stream.append(_revisit(rng, stream, 20) if i > 5 else (rng.integers(0, 61, 20) / 60.0).astype(np.float32))
    a, b = Seq(ctx, 0, margin, 0), Seq(ctx, 0, margin, 0)
    shared = RingKeyDB(ctx, margin=margin)
    own_lists, shared_lists = [], []
    for key in stream:
        got = query_then_enqueue_many([a.db, b.db], [key, key])
        assert got[0] == got[1] == a.twin.search_ringkey(key) == b.twin.search_ringkey(key)
        own_lists.append(got[0])
        shared_lists.append(shared.search_ringkey(key))  # sequence A's keyframe ...
        shared.search_ringkey(key)  # ... then sequence B's
    assert any(own_lists)
    assert own_lists != shared_lists
    # in the shared index ordinal 2i is A's i-th keyframe and 2i+1 B's: A's queries are handed B's keyframes
    assert any(c % 2 == 1 for lst in shared_lists for c in lst)


@pytest.mark.gpu
def test_errors_leave_every_index_unchanged(ctx):
    """every refusal of the contract: DSM_ERR_INVALID before any output, enqueue or index change"""
    from direct_stereo_slam_amd.tracker import Context

    rng = np.random.default_rng(11)
    seqs = [Seq(ctx, n, margin=3, seed=300 + n) for n in (10, 1100)]
    _drive(ctx, seqs, rng, 4)
    probe = np.stack([_revisit(rng, seqs[1].content, 20) for _ in range(6)])
    before = [(q.db.size(), q.db.knn_packed_host(probe)) for q in seqs]
    other_ctx = Context(0)
    foreign, sharded = RingKeyDB(other_ctx), RingKeyDB(ctx, shard_rank=0, shard_count=2)
    dim12, k2 = RingKeyDB(ctx, dim=12), RingKeyDB(ctx, k=2)
    A, B = seqs[0].db, seqs[1].db
    L = _lib.load()
    cand, nc = (C.c_int * 16)(), (C.c_int * 4)()
    keys = np.stack([_revisit(rng, seqs[0].content, 20) for _ in range(4)])
    kp = keys.ctypes.data_as(_lib.c_float_p)

    def call(dbs, n=None, k=kp, c=cand, m=nc):
        arr = (C.c_void_p * len(dbs))(*[d.h if d is not None else None for d in dbs])
        return L.dsm_ringdb_query_then_enqueue_many(len(dbs) if n is None else n, arr, k, c, m)

    cases = {
        "null keys": lambda: call([A, B], k=None),
        "null cand_out": lambda: call([A, B], c=None),
        "null ncand_out": lambda: call([A, B], m=None),
        "null index list": lambda: L.dsm_ringdb_query_then_enqueue_many(2, None, kp, cand, nc),
        "n < 1": lambda: call([A, B], n=0),
        "null index": lambda: call([A, None]),
        "mixed context": lambda: call([A, B, foreign]),
        "sharded": lambda: call([A, B, sharded]),
        "dim mismatch": lambda: call([A, B, dim12]),
        "k mismatch": lambda: call([A, B, k2]),
        "more than margin jobs on one index": lambda: call([A, A, A, A]),
    }
    for name, f in cases.items():
        assert f() == ERR_INVALID, name
        for q, (size, packed) in zip(seqs, before):
            assert q.db.size() == size and np.array_equal(q.db.knn_packed_host(probe), packed), name
    # the delay queues did not move either: the twins, which never saw these calls, still agree on every later call
    _drive(ctx, seqs, rng, 8)
    _same_indexes(seqs, rng)
    for d in (foreign, sharded, dim12, k2):
        d.close()
    other_ctx.close()
