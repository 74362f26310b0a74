"""CPU: the ring-key checker (tests/_ringkey_ref.py) against the C oracle, against float64, and against its own shortcuts.  The device
tests (test_ringkey_forms.py) trust the checker word for word, so it is checked here, where no GPU is needed."""
import numpy as np
import pytest

import _ringkey_ref as R

DIMS = [1, 3, 4, 7, 12, 20, 31, 32]


@pytest.fixture(scope="module")
def cases():
    """per dim: 700 lattice keys with revisits, 48 queries (exact hits, one-sector moves, new places)"""
    out = {}
    for dim in DIMS:
        keys = R.lattice_keys(700, dim, seed=dim)
        out[dim] = (keys, R.lattice_queries(keys, 48, seed=dim))
    return out


@pytest.mark.parametrize("dim", DIMS)
def test_numpy_route_equals_the_c_oracle(cases, dim):
    keys, q = cases[dim]
    n_ties = 0
    for k in (1, 2, 3, 4):
        for thres in (0.1, np.inf):
            a, b = R.topk_packed(q, keys, k, thres), R.topk_packed_oracle(q, keys, k, thres)
            np.testing.assert_array_equal(a, b)
            n_ties += int(((a[:, 1:] >> 32) == (a[:, :-1] >> 32))[a[:, 1:] != R.NO_CANDIDATE].sum()) if k > 1 else 0
    assert n_ties > 10  # the cases do hold equal distances, resolved by index
    # fewer entries than k, and shards (global index = local slot * count + rank)
    for n in (1, 2, 3, 5):
        np.testing.assert_array_equal(R.topk_packed(q, keys[:n], 4), R.topk_packed_oracle(q, keys[:n], 4))
        assert (R.topk_packed(q, keys[:n], 4)[:, n:] == R.NO_CANDIDATE).all()
    for shard in ((0, 2), (1, 2), (2, 3), (7, 8)):
        np.testing.assert_array_equal(R.topk_packed(q, keys, 4, 0.1, shard), R.topk_packed_oracle(q, keys, 4, 0.1, shard))


@pytest.mark.parametrize("dim", DIMS)
def test_float32_distance_against_float64(cases, dim):
    """|d32 - d64| <= (dim + 3) * 2^-24 * d64: every term takes one rounding in the subtraction (relative 2^-24 on the difference, twice
    that on its square), one in the square, and passes through at most dim - 1 additions of non-negative numbers"""
    keys, q = cases[dim]
    d32 = R.l2_flann(q, keys).astype(np.float64)
    d64 = ((q.astype(np.float64)[:, None, :] - keys.astype(np.float64)[None, :, :]) ** 2).sum(-1)
    bound = (dim + 3) * 2.0 ** -24 * d64
    err = np.abs(d32 - d64)
    print(f"dim {dim}: largest |d32 - d64| / (2^-24 d64) = {np.max(err[d64 > 0] / (2.0 ** -24 * d64[d64 > 0])):.2f} (bound {dim + 3})")
    assert (err <= bound).all()


@pytest.mark.parametrize("dim", DIMS)
def test_topk_agrees_with_the_float64_ranking(cases, dim):
    """wherever two float64 distances differ by more than the two pairs' error bounds, the float32 list orders them as float64 does:
    no entry of the list is beaten that clearly by its successor or by an entry left out"""
    keys, q = cases[dim]
    d64 = ((q.astype(np.float64)[:, None, :] - keys.astype(np.float64)[None, :, :]) ** 2).sum(-1)
    e = (dim + 3) * 2.0 ** -24
    top = R.topk_packed(q, keys, 4)
    idx = (top & 0xFFFFFFFF).astype(np.int64)
    rows = np.arange(len(q))[:, None]
    dl = d64[rows, idx]  # (nq, 4)
    assert (dl[:, 1:] >= dl[:, :-1] - e * (dl[:, 1:] + dl[:, :-1])).all()
    out = d64.copy()
    out[rows, idx] = np.inf
    best_out = out.min(1)
    assert (best_out >= dl[:, 3] - e * (best_out + dl[:, 3])).all()


@pytest.mark.parametrize("dim", [7, 20])
def test_one_reference_serves_every_k_and_threshold(cases, dim):
    """the top-4 at thres = inf, cut to k entries and filtered by the threshold, IS the top-k at that threshold; and the prefixes of
    an index share one distance matrix"""
    keys, q = cases[dim]
    ref4 = R.topk_packed(q, keys, 4)
    some_cut = False
    for k in (1, 2, 3, 4):
        np.testing.assert_array_equal(ref4[:, :k], R.topk_packed(q, keys, k))
        for thres in (0.1, 0.01, 1 / 3600, 0.0):
            want = R.topk_packed(q, keys, k, thres)
            np.testing.assert_array_equal(R.narrow(ref4, k, thres), want)
            some_cut |= bool((want == R.NO_CANDIDATE).any() and (want != R.NO_CANDIDATE).any())
    assert some_cut
    sizes = [1, 2, 3, 4, 5, 127, 128, 129, 700]
    pre = R.topk_packed_prefixes(q, keys, sizes)
    for n in sizes:
        np.testing.assert_array_equal(pre[n], R.topk_packed(q, keys[:n], 4))


@pytest.mark.parametrize("dim", [7, 20])
def test_non_finite_values_are_never_candidates(cases, dim):
    """a NaN anywhere in a pair makes its distance NaN, an inf makes it inf or NaN: `d < thres` and `d < the list's last` both fail, in
    the checker and in the C oracle alike"""
    keys, q = cases[dim]
    keys, q = keys.copy(), q[:6].copy()
    q[1, dim // 2] = np.nan
    q[4, 0] = np.inf
    bad = [3, 40, 41]
    keys[3] = q[0]
    keys[3, 2] = np.nan
    keys[40, dim - 1] = np.inf
    keys[41, 1] = -np.inf
    for thres in (0.1, np.inf):
        a, b = R.topk_packed(q, keys, 4, thres), R.topk_packed_oracle(q, keys, 4, thres)
        np.testing.assert_array_equal(a, b)
        assert (a[1] == R.NO_CANDIDATE).all() and (a[4] == R.NO_CANDIDATE).all()
        assert not np.isin(a[a != R.NO_CANDIDATE] & 0xFFFFFFFF, bad).any()
    assert (R.topk_packed(q, keys, 4)[[0, 2, 3, 5]] != R.NO_CANDIDATE).all()


def test_generators():
    base = R.lattice_keys(3000, 20, seed=1)
    big = R.tiled_keys(50001, base)
    assert big.shape == (50001, 20) and big.dtype == np.float32
    np.testing.assert_array_equal(big[:3000], base)
    assert len(np.unique(big[5::3000], axis=0)) == len(big[5::3000])  # the repetitions of one base key all differ
    tie, closer = R.tie_pair(base)
    d = R.l2_flann(np.stack([tie, closer]), np.vstack([base, tie[None], closer[None]]))
    assert d[0, -2] == 0 and d[1, -1] == 0 and d[0, -1] == d[1, -2] > 0
    assert d[:, :-2].min() > d[0, -1]  # every lattice key is farther from both than they are from each other
