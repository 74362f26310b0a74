"""The checker of the ring-key k-NN (csrc/ringkey_kernels.hip, csrc/ringdb_capi.hip): what every scan form must return, bit for bit.

Two routes to the same packed words  float_bits(d) << 32 | global index  (ascending as unsigned integers: nearest first, the
smaller index on ties; NO_CANDIDATE pads):
  * numpy: `l2_flann` restates flann::L2<float> in float32 -- subtract, square, sum each group of four as ((s0+s1)+s2)+s3, add the
    group to the running result, then the tail loop element by element -- and `topk_packed` sorts the packed words;
  * the C oracle (oracle/dsm_oracle.c: orc_ringdb_knn), one query at a time: for the cases too large for numpy.
tests/test_ringkey_ref.py holds the two against each other and against float64; tests/test_ringkey_forms.py holds the device
against them.  Nothing here has a tolerance.
"""
import numpy as np

NO_CANDIDATE = 0x7FFFFFFFFFFFFFFF
SECTOR = np.float32(1 / 60)  # a ring key's entries are counts of 60 sectors, divided by 60


def l2_flann(q, keys, chunk_pairs=1 << 21):
    """float32 squared distances (nq, n) in flann::L2's operation order, chunked over queries"""
    q, keys = np.ascontiguousarray(q, np.float32), np.ascontiguousarray(keys, np.float32)
    q = q.reshape(-1, keys.shape[1])
    nq, n, dim = q.shape[0], keys.shape[0], keys.shape[1]
    out = np.empty((nq, n), np.float32)
    kt = np.ascontiguousarray(keys.T)
    step = max(1, chunk_pairs // max(1, n))
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(0, nq, step):
            qc = q[a:a + step]
            res = np.zeros((qc.shape[0], n), np.float32)

            def sq(j):
                d = qc[:, j, None] - kt[j][None, :]
                return d * d

            j = 0
            while j + 3 < dim:
                res = res + (((sq(j) + sq(j + 1)) + sq(j + 2)) + sq(j + 3))
                j += 4
            while j < dim:
                res = res + sq(j)
                j += 1
            assert res.dtype == np.float32
            out[a:a + step] = res
    return out


def pack(dist, index):
    """float32 distances and global indices -> unsigned 64-bit candidates"""
    bits = np.ascontiguousarray(dist, np.float32).view(np.uint32).astype(np.uint64)
    return (bits << np.uint64(32)) | np.asarray(index).astype(np.uint64)


def _first_k(words, k):
    """the k smallest of each row as unsigned integers, ascending, padded with NO_CANDIDATE, as the int64 the C ABI hands out"""
    nq, n = words.shape
    if n < k:
        words = np.concatenate([words, np.full((nq, k - n), NO_CANDIDATE, np.uint64)], 1)
    elif n > 4 * k:
        words = np.partition(words, k - 1, axis=1)[:, :k]
    return np.sort(words, axis=1)[:, :k].view(np.int64)


def packed_matrix(q, keys, thres=np.inf, shard=(0, 1)):
    """every pair's packed candidate (nq, n_shard): NO_CANDIDATE where `not (d < thres)`; with a shard only the ordinals with
    ord % count == rank are kept, and the index stays global"""
    rank, count = shard
    keys = np.ascontiguousarray(keys, np.float32)
    ords = np.arange(rank, keys.shape[0], count)
    d = l2_flann(q, keys[ords])
    w = pack(d, ords[None, :])
    with np.errstate(invalid="ignore"):
        w[~(d < np.float32(thres))] = NO_CANDIDATE
    return w


def topk_packed(q, keys, k, thres=np.inf, shard=(0, 1)):
    """the checker: (nq, k) int64 packed candidates of the queries over `keys` (row i = global ordinal i, the dummy included)"""
    return _first_k(packed_matrix(q, keys, thres, shard), k)


def topk_packed_prefixes(q, keys, sizes, k=4):
    """{n: topk_packed(q, keys[:n], k, inf)} for every n of `sizes` from one distance matrix"""
    w = packed_matrix(q, keys[: max(sizes)])
    return {n: _first_k(w[:, :n], k) for n in sizes}


def narrow(ref, k, thres=np.inf):
    """from a reference at a larger k and thres = inf to (k, thres): a top-k is the prefix of a larger one, and the threshold cuts an
    ascending list's end (tests/test_ringkey_ref.py proves both against the direct computation)"""
    out = np.array(ref[:, :k], np.int64)
    dist = (out >> 32).astype(np.uint32).view(np.float32)
    with np.errstate(invalid="ignore"):
        out[(out != NO_CANDIDATE) & ~(dist < np.float32(thres))] = NO_CANDIDATE
    return out


def topk_packed_oracle(q, keys, k, thres=np.inf, shard=(0, 1)):
    """the same words through the C oracle's brute force, one query at a time (a shard: the oracle scans the shard's own keys, local
    slot i is global ordinal i * count + rank)"""
    from oracle import oracle as O

    rank, count = shard
    keys = np.ascontiguousarray(keys, np.float32)
    mine = np.ascontiguousarray(keys[rank::count])
    q = np.ascontiguousarray(q, np.float32).reshape(-1, keys.shape[1])
    out = np.full((q.shape[0], k), NO_CANDIDATE, np.int64)
    if mine.shape[0] == 0:
        return out
    orc = O.OracleRingDB(dim=keys.shape[1], k=k, thres=np.inf, dummy=mine[0])
    if mine.shape[0] > 1:
        orc.add_points(mine[1:])
    for i in range(q.shape[0]):
        idx, dist = orc.knn(q[i])
        idx, dist = np.array(idx, np.int64), np.array(dist, np.float32)
        with np.errstate(invalid="ignore"):
            ok = (idx >= 0) & (dist < np.float32(thres))
        n = int(ok.sum())
        assert ok[:n].all()  # ascending: the threshold cuts the end
        out[i, :n] = pack(dist[:n], idx[:n] * count + rank).view(np.int64)
    return out


def candidates(row):
    """search_ringkey's list from one packed row: the dummy (index 0) is dropped, index i is keyframe i - 1 (search_place.h:34-38)"""
    return [int(p & 0xFFFFFFFF) - 1 for p in np.asarray(row, np.int64) if p != NO_CANDIDATE and int(p & 0xFFFFFFFF) > 0]


# ---- cases -----------------------------------------------------------------------------------------------------------------------

def lattice_keys(n, dim=20, seed=0, revisit=0.3):
    """ring keys on the 1/60 lattice (entry = Binomial(60, p_ring) / 60); a share of the rows revisits an earlier row: the same key, or
    one or two entries moved by a sector.  Distances on the lattice are multiples of 1/3600 up to rounding: ties are common."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.1, 0.9, dim)
    keys = (rng.binomial(60, p, size=(n, dim)) / 60.0).astype(np.float32)
    for i in np.nonzero(rng.uniform(size=n) < revisit)[0]:
        if i == 0:
            continue
        keys[i] = keys[rng.integers(i)]
        for d in rng.integers(dim, size=rng.integers(0, 3)):
            keys[i, d] = np.float32(keys[i, d] + (SECTOR if keys[i, d] < 0.5 else -SECTOR))
    return keys


def lattice_queries(keys, nq, seed=0):
    """a third of the queries equals a key (distance 0, often several times), a third is a key with one entry moved by a sector, the
    rest are new places drawn like the keys"""
    rng = np.random.default_rng(seed + 7919)
    n, dim = keys.shape
    q = keys[rng.integers(n, size=nq)].copy()
    kind = rng.integers(3, size=nq)
    for i in np.nonzero(kind == 1)[0]:
        d = rng.integers(dim)
        q[i, d] = np.float32(q[i, d] + (SECTOR if q[i, d] < 0.5 else -SECTOR))
    fresh = np.nonzero(kind == 2)[0]
    q[fresh] = (rng.binomial(60, 0.5, size=(len(fresh), dim)) / 60.0).astype(np.float32)
    return q


def tiled_keys(n, base):
    """n keys from a few thousand: repetition r of the base has entry r % dim moved by 1 + (r // dim) % 7 sectors: nothing but the base is
    generated, neighbouring repetitions differ, and repetitions 7 * dim apart are equal again (ties between distant ordinals)"""
    m, dim = base.shape
    reps = (n + m - 1) // m
    keys = np.tile(base, (reps, 1))[:n]
    r = np.arange(n) // m
    keys[np.arange(n), r % dim] += ((1 + (r // dim) % 7) * np.float32(1 / 60)).astype(np.float32) * (r > 0)
    return keys


def tie_pair(keys, seed=0):
    """(tie key, closer key) far from every lattice key (from dim 5 on: dim / 14400 against the pair's 1 / 3600): the tie key's entries
    lie between lattice points, the closer key differs from it by one sector in entry 0.  A query at the tie key sees the ties at 0 and the closer key at 1/3600; a query at the closer key sees
    the closer key at 0 and every tie at the same 1/3600."""
    rng = np.random.default_rng(seed + 104729)
    dim = keys.shape[1]
    tie = ((rng.integers(0, 60, dim) + 0.5) / 60.0).astype(np.float32)
    closer = tie.copy()
    closer[0] = np.float32(closer[0] + SECTOR)
    return tie, closer
