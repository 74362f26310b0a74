"""Test infrastructure shared by tests/test_icp_stages.py (GPU: the device's stages through dsm_diag_icp_stages) and
tests/test_icp_stage_bars.py (CPU: numpy mutants of the contract must be rejected): the scenes, the assertion helpers that hold one
stage each ("Testing"), and a numpy model of every stage with its mutants.  The helpers take plain arrays, so
that the device's buffers and a mutant's are judged by the same code."""
import math

import numpy as np

import _icp_ref as R

NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
DBL_MAX = np.finfo(np.float64).max
TILE = 256  # kIcpTile = kIcpThreads
RUNNING = 0
# delta of the increment's bound |float(got) - x| <= ulp32(x) / 2 + DELTA: 16 x the largest difference, over step_scenes()' full-rank
# scenes, between exact_step and the device's step restated on the host (block_sum_order moments into the host build of icp_umeyama).
# Measured: at most 8.9e-16 on the scenes about the origin, 4.55e-13 on the scene shifted by 1000 m (four ulps of a double at 1000, in
# t = dst_mean - R src_mean); tests/test_icp_stage_bars.py::test_delta_is_sixteen_times_the_measured_difference re-measures it.
DELTA = 16 * 4.6e-13
SLICE_COUNTS = (1, 2, 3, 5, "tile")


# ---- the slice rule and the keys ---------------------------------------------------------------------------------------------------

def want_slices(n_tgt, want):
    """the want_slices argument of dsm_diag_icp_stages for an entry of SLICE_COUNTS ("tile": one slice per 256-target tile)"""
    return max(1, -(-n_tgt // TILE)) if want == "tile" else want


def slice_len(n_tgt, want):
    """`per` of the block table: the targets of one slice when a job of n_tgt targets is cut as `want` asks"""
    tiles = max(1, -(-n_tgt // TILE))
    slices = min(want_slices(n_tgt, want), tiles)
    return -(-n_tgt // slices)


def pack_keys(idx, dist):
    """(float bits of dist2 << 32) | index per source point; NO_KEY where the index is -1 (D5)"""
    idx = np.asarray(idx, np.int64)
    bits = np.ascontiguousarray(dist, np.float32).view(np.uint32).astype(np.uint64)
    keys = (bits << np.uint64(32)) | (idx & 0xFFFFFFFF).astype(np.uint64)
    return np.where(idx < 0, NO_KEY, keys)


def unpack_keys(keys):
    """(index int64, dist2 float32) of packed keys; NO_KEY gives (-1, NaN)"""
    keys = np.asarray(keys, np.uint64)
    idx = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    dist = (keys >> np.uint64(32)).astype(np.uint32).view(np.float32).copy()
    idx[keys == NO_KEY] = -1
    return idx, dist


def ulp32(x):
    """the spacing of float32 at the double x (of its binade, so that half of it bounds the rounding of x to float exactly)"""
    x = abs(float(x))
    if x < 2.0 ** -126:
        return 2.0 ** -149
    return math.ldexp(1.0, math.frexp(x)[1] - 1 - 23)


# ---- the assertion helpers: one stage each ------------------------------------------------------------------------------------------

def check_prep(src, tgt, guess, got):
    """P1: orig = work = the source through the guess in double, the target through the identity, rounded to float; w = 0; no keys;
    the state reset"""
    want_src, want_tgt = R.transform_double(src, guess), R.transform_double(tgt, np.eye(4))
    for name in ("orig", "work"):
        assert got[name][:, :3].tobytes() == want_src.tobytes(), name
        assert not got[name][:, 3].any(), name
    assert got["target"][:, :3].tobytes() == want_tgt.tobytes() and not got["target"][:, 3].any()
    assert np.all(got["keys"] == NO_KEY)
    S = got["state"]
    assert S["final_tf"].tobytes() == np.eye(4, dtype=np.float32).tobytes()
    assert S["prev_mse"] == DBL_MAX and S["fitness"] == np.inf
    assert S["state"] == (R.EMPTY if len(want_src) == 0 or len(want_tgt) == 0 else RUNNING)
    assert S["iterations"] == 0 and S["searches"] == 0 and S["pad"] == 0 and np.all(S["corr"] == -1)


def check_search(work, target, keys, planted=None):
    """P2 / D2 / D5: every source point's key -- index and distance bits -- is the checker's; `planted`: and the index is this one"""
    idx, d = R.nearest(np.ascontiguousarray(work[:, :3]), np.ascontiguousarray(target[:, :3]))
    want = pack_keys(idx, d)
    bad = np.flatnonzero(np.asarray(keys) != want)
    if len(bad):
        i = bad[0]
        gi, gd = unpack_keys(keys[i:i + 1])
        raise AssertionError(f"{len(bad)} of {len(want)} source points; first {i}: got target {gi[0]} at {gd[0]!r}, "
                             f"want {idx[i]} at {d[i]!r}")
    if planted is not None:
        np.testing.assert_array_equal(idx, planted)
    return idx, d


def expected_end_state(inc, mse, prev_mse, iterations, max_iterations, eps, swapped=False):
    """P6 in PCL's order on a float increment (swapped: a mutant that tests the transform before the iteration limit)"""
    inc = np.asarray(inc, np.float32)
    cos_angle = 0.5 * float(((inc[0, 0] + inc[1, 1]) + inc[2, 2]) - np.float32(1))
    tr2 = (inc[0, 3] * inc[0, 3] + inc[1, 3] * inc[1, 3]) + inc[2, 3] * inc[2, 3]
    if iterations >= max_iterations and not swapped:
        return R.ITERATIONS
    if cos_angle >= 1.0 - eps and float(tr2) <= eps:
        return R.TRANSFORM
    if iterations >= max_iterations:
        return R.ITERATIONS
    if abs(mse - prev_mse) < 1e-12:
        return R.ABS_MSE
    return RUNNING


def mse_bound(n_src, value):
    """D4 against the correctly rounded mean: a lane chain of ceil(n / 256) additions, the 8 levels of the tree, the division and the
    reference's own rounding, half an ulp of a double (2^-53 relative) each"""
    return (-(-n_src // 256) + 10) * 2.0 ** -53 * abs(value)


def check_increment(inc, Rx, tx, delta=DELTA):
    """P4: every entry of the float increment within half a float ulp (its rounding from double) + delta of the exact step's;
    returns the worst err / bound"""
    worst = 0.0
    for r in range(3):
        for c in range(4):
            x = float(Rx[r, c]) if c < 3 else float(tx[r])
            err, bound = abs(float(inc[r, c]) - x), ulp32(x) / 2 + delta
            assert err <= bound, f"increment[{r},{c}] = {inc[r, c]!r}, exact {x!r}: err {err:.3e} > {bound:.3e}"
            worst = max(worst, err / bound)
    return worst


def check_rank_deficient_increment(inc, work, target, idx, keep):
    """Planar, collinear or coincident pairs, where the exact step's rotation need not be unique: by properties.  The float R is a
    rotation to float rounding (4 ulps of 1 per entry of R R^T, 8 of the determinant); t is P4's dst_mean - R src_mean; and the fit is
    as good as the exact step's: the sum of squared residuals of the pairs under the rotation nearest to float R (its polar factor,
    which removes the rounding to float; t as above) equals the exact step's to 1e-9 relative -- plus, for pairs that fit exactly
    (coincident points, a planar reflection: the sum is 0 but for rounding), what evaluating a residual in double leaves: 16 half-ulps
    of the largest coordinate per point, squared."""
    Rf = np.asarray(inc, np.float64)[:3, :3]
    assert np.abs(Rf @ Rf.T - np.eye(3)).max() <= 4 * 2.0 ** -23 and abs(np.linalg.det(Rf) - 1) <= 8 * 2.0 ** -23
    s = np.asarray(work, np.float64)[keep]
    d = np.asarray(target, np.float64)[np.asarray(idx)[keep]]
    sm, dm = np.array([math.fsum(c) for c in s.T]) / len(s), np.array([math.fsum(c) for c in d.T]) / len(d)
    for r in range(3):  # t: the rounding of t itself + R's rounding to float (2^-24 relative per entry) carried through R src_mean
        x = dm[r] - Rf[r] @ sm
        assert abs(float(inc[r, 3]) - x) <= ulp32(x) / 2 + 2.0 ** -24 * float(np.abs(Rf[r]) @ np.abs(sm)) + DELTA, r
    U, _, Vt = np.linalg.svd(Rf)
    Rp = U @ Vt
    Rx, tx = R.exact_step(work, target, idx, keep)

    def residual(Rm, t):
        return math.fsum((((s @ Rm.T + t) - d) ** 2).ravel())

    got, want = residual(Rp, dm - Rp @ sm), residual(Rx, tx)
    floor = len(s) * (16 * 2.0 ** -53 * max(np.abs(s).max(), np.abs(d).max())) ** 2
    assert abs(got - want) <= 1e-9 * want + floor, (got, want, floor)
    return abs(got - want) / (1e-9 * want + floor) if want + floor else 0.0


def check_step(before, after, max_iterations, eps, max_corr_dist=2.0, full_rank=True, figures=None):
    """P3-P6 of ONE step, judged alone: `before` is what the device held after the search (work, target, keys, state), `after` what
    it holds after the step.  Exact: the pairs kept, the moved cloud, the keys, final, the counters and the end state; bounded: the
    increment against exact_step, the MSE against exact_mean.  figures: a dict that collects the worst err / bound."""
    work, target = np.ascontiguousarray(before["work"][:, :3]), np.ascontiguousarray(before["target"][:, :3])
    idx, d = unpack_keys(before["keys"])
    keep = d.astype(np.float64) <= max_corr_dist * max_corr_dist  # P2, in double; a NaN distance (no key) is not kept
    n = int(keep.sum())
    S0, S = before["state"], after["state"]
    k = int(S0["searches"])
    assert S0["state"] == RUNNING
    assert S["corr"][k] == n and np.array_equal(S["corr"][:k], S0["corr"][:k]) and np.all(S["corr"][k + 1:] == -1), (S["corr"][:k + 2], n)
    assert S["searches"] == k + 1
    assert after["orig"].tobytes() == before["orig"].tobytes() and after["target"].tobytes() == before["target"].tobytes()
    if n < 3:  # P3: the loop ends; nothing moves, final stays, the keys stay for the fitness prep to reset
        assert S["state"] == R.NO_CORRESPONDENCES and S["iterations"] == S0["iterations"]
        assert after["work"].tobytes() == before["work"].tobytes() and np.array_equal(after["keys"], before["keys"])
        assert S["final_tf"].tobytes() == S0["final_tf"].tobytes() and S["prev_mse"] == S0["prev_mse"]
        return None
    assert S["iterations"] == S0["iterations"] + 1
    assert S0["iterations"] == 0, "the increment is read from final: first steps only"
    inc = S["final_tf"].copy()  # final = inc * identity: the increment itself
    assert inc[3].tobytes() == np.array([0, 0, 0, 1], np.float32).tobytes()
    moved = R.transform_float(inc, work)  # P5, the last point included
    assert np.ascontiguousarray(after["work"][:, :3]).tobytes() == moved.tobytes() and not after["work"][:, 3].any()
    assert np.all(after["keys"] == NO_KEY)
    if full_rank:
        Rx, tx = R.exact_step(work, target, idx, keep)
        worst = check_increment(inc, Rx, tx)
    else:
        worst = check_rank_deficient_increment(inc, work, target, idx, keep)
    mse = R.exact_mean(d[keep])
    want_state = expected_end_state(inc, mse, float(S0["prev_mse"]), int(S["iterations"]), max_iterations, eps)
    assert S["state"] == want_state, (int(S["state"]), want_state)
    if want_state == RUNNING:  # only then is the MSE kept
        err, bound = abs(float(S["prev_mse"]) - mse), mse_bound(len(work), mse)
        assert err <= bound, f"prev_mse {S['prev_mse']!r}, exact {mse!r}: err {err:.3e} > {bound:.3e}"
        if figures is not None and bound:
            figures["mse"] = max(figures.get("mse", 0.0), err / bound)
    else:
        assert S["prev_mse"] == S0["prev_mse"]
    if figures is not None:
        key = "increment" if full_rank else "residual"
        figures[key] = max(figures.get(key, 0.0), worst)
    return inc


def check_fitness_prep(before, after):
    """P9, first half: the working cloud is the ORIGINAL (guess-moved) source moved by final, bit for bit; the keys are reset"""
    final = before["state"]["final_tf"]
    moved = R.transform_float(final, np.ascontiguousarray(before["orig"][:, :3]))
    assert np.ascontiguousarray(after["work"][:, :3]).tobytes() == moved.tobytes() and not after["work"][:, 3].any()
    assert np.all(after["keys"] == NO_KEY)
    assert after["orig"].tobytes() == before["orig"].tobytes() and after["state"].tobytes() == before["state"].tobytes()


def check_fitness(searched, after, figures=None):
    """P9 / D4: the fitness is the mean of the keys' distances, within the bound of the MSE of the correctly rounded mean"""
    _, d = unpack_keys(searched["keys"])
    want = R.exact_mean(d)
    got = float(after["state"]["fitness"])
    if math.isnan(want):
        assert math.isnan(got)
        return
    err, bound = abs(got - want), mse_bound(len(d), want)
    assert err <= bound, f"fitness {got!r}, exact {want!r}: err {err:.3e} > {bound:.3e}"
    if figures is not None and bound:
        figures["fitness"] = max(figures.get("fitness", 0.0), err / bound)


# ---- scenes -------------------------------------------------------------------------------------------------------------------------

SEAM_N_TGT = (1, 2, 255, 256, 257, 511, 512, 513, 1300)
SEAM_N_SRC = (1, 255, 256, 257, 600)


def seam_indices(n_tgt, per):
    """the target indices of {0, 255, 256, per - 1, per, 2 per - 1, 2 per, n_tgt - 1} that exist, ascending"""
    return sorted({p for p in (0, 255, 256, per - 1, per, 2 * per - 1, 2 * per, n_tgt - 1) if 0 <= p < n_tgt})


def seam_case(n_src, n_tgt, per, only=None):
    """(source, target, planted): every background target is 10 m or more from every source; source j's true neighbour is planted at
    the index cyc[j % len(cyc)], cyc = seam_indices(n_tgt, per) -- or, with `only`, at that one index for every source, so that every
    lane of every source block meets that seam -- at distance 0, a tiny distance or about 1 m in turn.  The planted targets stand
    20 m apart on the negative x axis, the sources within 1.1 m of theirs, the background on a 3 m lattice at x >= 100."""
    cyc = seam_indices(n_tgt, per)
    i = np.arange(n_tgt)
    tgt = np.stack([100.0 + 3.0 * (i % 23), 3.0 * ((i // 23) % 23) - 30.0, 3.0 * (i // 529)], 1)
    for k, p in enumerate(cyc):
        tgt[p] = (-20.0 * (k + 1), 0.25 * k, 0.5)
    j = np.arange(n_src)
    planted = np.array(cyc)[j % len(cyc)] if only is None else np.full(n_src, only)
    kind = (j // len(cyc)) % 3
    ang = 0.7 * j
    unit = np.stack([np.cos(ang), np.sin(ang) * np.cos(1.3 * j), np.sin(ang) * np.sin(1.3 * j)], 1)
    radius = np.where(kind == 0, 0.0, np.where(kind == 1, 1e-3 * (1 + j % 7), 0.9 + 0.01 * (j % 19)))
    src = tgt[planted] + radius[:, None] * unit
    return src, tgt, planted


def seam_jobs(n_tgt, want):
    """the jobs of one call of the seam sweep: SEAM_N_SRC's sizes with the seams in turn, then 600 sources on each single seam; the
    list is rotated by the slice count's position, so that the first workgroup of the call is not always the same job's"""
    per = slice_len(n_tgt, want)
    cases = [seam_case(n_src, n_tgt, per) for n_src in SEAM_N_SRC] + [seam_case(600, n_tgt, per, only=p) for p in seam_indices(n_tgt, per)]
    k = SLICE_COUNTS.index(want) % len(cases)
    return per, cases[k:] + cases[:k]


def tie_case(n_tgt, per):
    """(source, target, planted): groups of targets at EXACTLY the same float distance from their sources (lattice coordinates, as
    _icp_ref.ties); the smallest index of each group is planted.  Groups: indices (255, 256); (per - 1, per); (0, n_tgt - 1); two tiles
    of one slice (where a slice has two); a triple.  Each group has three sources, on the axis all its targets are equidistant from."""
    groups = [(255, 256), (0, n_tgt - 1), (7, 600, n_tgt - 10)]
    if per < n_tgt and (per - 1) not in (255, 256) and per not in (255, 256):
        groups.append((per - 1, per))
    if per > TILE + 2:  # a slice of more than one tile: slice 0's first and second tile
        groups.append((10, min(300, per - 2)))
    flat = [p for g in groups for p in g]
    assert len(set(flat)) == len(flat) and max(flat) < n_tgt
    i = np.arange(n_tgt)
    tgt = np.stack([200.0 + 4.0 * (i % 23), 4.0 * ((i // 23) % 23), 4.0 * (i // 529)], 1)
    offsets = np.array([[0.5, 0, 0], [-0.5, 0, 0], [0, 0.5, 0]])
    src, planted = [], []
    for k, g in enumerate(groups):
        centre = np.array([-16.0 * (k + 1), 8.0, 0.0])
        for m, p in enumerate(g):
            tgt[p] = centre + offsets[m]
        for z in (0.0, 1.0, 2.5):
            src.append(centre + np.array([0.0, 0.0, z]))
            planted.append(min(g))
    return np.array(src), tgt, np.array(planted)


def nonfinite_cases():
    """name -> (source, target): D5's rows"""
    rng = np.random.default_rng(31)
    src = rng.normal(0, 3, (300, 3))
    tgt = np.vstack([src + rng.normal(0, 0.05, src.shape), rng.normal(0, 3, (300, 3))])  # a fit exists: the step has something to find
    bad_t = tgt.copy()
    bad_t[[0, 255, 599]] = np.nan
    bad_t[[1, 256, 300]] = np.inf
    bad_t[[2, 511, 512]] = -np.inf
    bad_t[5, 1] = np.nan  # one coordinate is enough
    bad_s = src.copy()
    bad_s[[0, 77, 255, 299]] = np.nan
    bad_s[100, 2] = np.inf
    far = 1e20 * (1.0 + np.arange(300))[:, None] * np.ones(3)
    only = np.full((300, 3), np.nan)
    only[1::3], only[2::3] = np.inf, -np.inf
    return {"target_rows": (src, bad_t), "source_rows": (bad_s, bad_t), "overflow": (far[:260], -far), "target_all_nonfinite": (src, only)}


IDENTITY = np.eye(4)


def dense_case(shift):
    """(source, target): scene(61, 600, n_tgt = 1300) moved by `shift` metres along every axis.  The last 100 targets stand in pairs
    about 50 of the sources, 0.3 m to either side and k x 1e-5 m apart in distance: about the origin the float difference resolves
    which is nearer, 1000 m away (float spacing 6e-5) its rounding decides."""
    src, tgt, _ = R.scene(61, 600, n_tgt=1300)
    tgt = tgt.copy()
    k = np.arange(50)
    tgt[1200:1250] = src[7 * k] + np.stack([0.3 + 1e-5 * (k - 25), 0 * k, 0 * k], 1)
    tgt[1250:1300] = src[7 * k] - np.array([0.3, 0.0, 0.0])
    return src + shift, tgt + shift


def step_scenes():
    """name -> (source, target, guess, full_rank): the shapes of the step tests.  Full-rank scenes go against exact_step entry by
    entry (and are the scenes DELTA is measured on), the others by properties."""
    guess = R.rigid(R.rot((0.0, 0.01, 0.0)), [0.05, 0.0, 0.0])
    out = {}
    for n in (255, 256, 257, 2000):
        s, t, _ = R.scene(40 + n, n, n_tgt=n + 150)
        out[f"n{n}"] = (s, t, guess if n == 2000 else IDENTITY, True)
    s, t, _ = R.scene(43, 3, n_tgt=200)
    out["n3"] = (s, t, IDENTITY, False)  # three pairs span a plane at most
    s, t, _ = R.scene(47, 600, n_tgt=700)
    s = s.copy()
    s[::2, 1] -= 60.0  # every other source 60 m up: no target within 2 m, so the means run over half the points
    out["half_without_pairs"] = (s, t, IDENTITY, True)
    s, t, _ = R.scene(48, 600, n_tgt=700)
    out["shifted_1000m"] = (s + 1000.0, t + 1000.0, IDENTITY, True)  # Sigma must be centred: |mean|^2 is 1e6 times the spread
    rng = np.random.default_rng(49)
    x = 4.0 * np.arange(200)
    y = rng.uniform(0.1, 0.9, 200) * np.where(rng.random(200) < 0.5, -1, 1)
    out["reflected_planar"] = (np.stack([x, y, np.zeros(200)], 1), np.stack([x, -y, np.zeros(200)], 1), IDENTITY, False)
    T = R.rigid(R.rot((0.01, 0.02, 0.03)), [0.1, 0.05, -0.1])
    flat = np.stack([rng.uniform(-8, 8, 400), rng.uniform(-8, 8, 400), np.zeros(400)], 1)
    noise = np.stack([rng.normal(0, 0.05, 400), rng.normal(0, 0.05, 400), np.zeros(400)], 1)
    out["planar"] = (flat, (flat + noise) @ T[:3, :3].T + T[:3, 3], IDENTITY, False)
    u = np.array([1.0, 2.0, -0.5]) / np.linalg.norm([1.0, 2.0, -0.5])
    lam = np.linspace(-8, 8, 300)
    out["collinear"] = (np.outer(lam, u), np.outer(lam + rng.normal(0, 0.05, 300), u) @ T[:3, :3].T + T[:3, 3], IDENTITY, False)
    return out


def edge_jobs():
    """name -> (source, target): P2's threshold and P3's count.  The sources of a threshold job stand at the origin, so that
    source - target is exact and dist2 is exactly 4.0f or the next float above."""
    above = np.array([2.0, float(np.float32(0.00069)), 0.0])  # 4 + 0.00069^2 rounds to the float after 4.0f (0.00069^2 is 0.998 of its ulp)
    dy2 = np.float32(above[1]) * np.float32(above[1])
    assert np.float32(4.0) + dy2 == np.nextafter(np.float32(4.0), np.float32(5.0))
    origin3 = np.zeros((3, 3))
    far = np.array([[100.0, 0.0, 0.0]])
    return {
        "at_threshold": (origin3, np.array([[2.0, 0.0, 0.0], [0.0, 5.0, 0.0]])),              # 3 pairs at dist2 = 4.0f: kept, runs
        "above_threshold": (origin3, np.array([above, [0.0, 5.0, 0.0]])),         # the next float above: 0 kept
        "two_pairs": (np.vstack([origin3[:2], far]), np.array([[0.0, -2.0, 0.0]])),           # exactly 2 kept: state 5
        "three_pairs": (np.vstack([origin3, far, 2 * far]), np.array([[0.0, 0.0, 2.0]])),     # exactly 3 kept of 5: runs
        "three_kept_of_four": (np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.5], [50.0, 0.0, 0.0]]),
                                 np.array([[0.1, 0.0, 0.0], [1.0, 0.2, 0.0], [0.0, 1.0, 0.0], [2.0, 50.0, 0.0]])),
    }


# ---- a numpy model of the stages, with the mutants the bars must reject ---------------------------------------------------------------

def model_search(work, target, per, mutant=None):
    """icp_nn_kernel restated: per slice of `per` targets, tiles of 256 scanned in index order with a strict `<` (the first minimum
    of the slice), the slices merged by the minimum of the packed key.  Mutants: "skip_tile_last" (lane 77 skips the last target of
    every tile), "le" (`<=` in the scan: the last minimum), "merge_larger" (the merge keeps the larger index of equal distances)."""
    work, target = np.asarray(work, np.float32), np.asarray(target, np.float32)
    n, rows = len(work), np.arange(len(work))
    with np.errstate(over="ignore", invalid="ignore"):
        dx, dy, dz = (work[:, c:c + 1] - target[None, :, c] for c in range(3))
        D = (dx * dx + dy * dy) + dz * dz
    D = np.where(np.isfinite(D), D, np.float32(np.inf))
    keys = np.full(n, NO_KEY)
    for t0 in range(0, len(target), per):
        t1 = min(len(target), t0 + per)
        sub = D[:, t0:t1].copy()
        if mutant == "skip_tile_last":
            for a in range(t0, t1, TILE):
                sub[rows % 256 == 77, min(a + TILE, t1) - 1 - t0] = np.inf
        i = (t1 - t0 - 1) - np.argmin(sub[:, ::-1], axis=1) if mutant == "le" else np.argmin(sub, axis=1)
        best = sub[rows, i]
        part = pack_keys(np.where(np.isfinite(best), t0 + i, -1), best)
        if mutant == "merge_larger":
            same = (keys != NO_KEY) & (part != NO_KEY) & ((keys >> np.uint64(32)) == (part >> np.uint64(32)))
            keys = np.where(same, np.maximum(keys, part), np.minimum(keys, part))
        else:
            keys = np.minimum(keys, part)
    return keys


def _fit(sigma, sm, dm):
    U, _, Vt = np.linalg.svd(sigma)
    S = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2] = -1.0
    Rm = U @ np.diag(S) @ Vt
    return Rm, dm - Rm @ sm


def model_step(before, max_iterations, eps, max_corr_dist=2.0, mutant=None):
    """icp_step_kernel restated on the buffers `before` (as check_step reads them); returns the buffers after.  Mutants:
    "lt_threshold" (dist2 < max instead of <=), "means_over_all" (the means run over every point with a neighbour), "sigma_transposed",
    "sigma_float_uncentred" (Sigma = mean(dst src^T) - dst_mean src_mean^T in float), "p6_swapped" (the transform test before the
    iteration limit)."""
    after = {k: v.copy() for k, v in before.items()}
    S = after["state"]
    work, target = np.ascontiguousarray(before["work"][:, :3]), np.ascontiguousarray(before["target"][:, :3])
    idx, d = unpack_keys(before["keys"])
    max_d2 = max_corr_dist * max_corr_dist
    with np.errstate(invalid="ignore"):
        keep = d.astype(np.float64) < max_d2 if mutant == "lt_threshold" else d.astype(np.float64) <= max_d2
    n = int(keep.sum())
    S["corr"][S["searches"]] = n
    S["searches"] += 1
    if n < 3:
        S["state"] = R.NO_CORRESPONDENCES
        return after
    if mutant is None:
        Rm, t = R.exact_step(work, target, idx, keep)
    else:
        s, dd = work.astype(np.float64)[keep], target.astype(np.float64)[idx[keep]]
        sm, dm = s.mean(0), dd.mean(0)
        if mutant == "means_over_all":
            has = idx >= 0
            sm, dm = work.astype(np.float64)[has].mean(0), target.astype(np.float64)[idx[has]].mean(0)
        sigma = (dd - dm).T @ (s - sm) / n
        if mutant == "sigma_transposed":
            sigma = sigma.T
        if mutant == "sigma_float_uncentred":
            s32, d32 = work[keep], target[idx[keep]]
            sigma = ((d32.T @ s32) / np.float32(n) - np.outer(d32.mean(0), s32.mean(0))).astype(np.float64)
        Rm, t = _fit(sigma, sm, dm)
    inc = np.eye(4, dtype=np.float32)
    inc[:3, :3], inc[:3, 3] = Rm.astype(np.float32), t.astype(np.float32)
    F0, F = S["final_tf"].copy(), np.empty((4, 4), np.float32)
    for r in range(4):
        for c in range(4):
            F[r, c] = ((inc[r, 0] * F0[0, c] + inc[r, 1] * F0[1, c]) + inc[r, 2] * F0[2, c]) + inc[r, 3] * F0[3, c]
    S["final_tf"] = F
    S["iterations"] += 1
    mse = R.block_sum_order(np.where(keep, d.astype(np.float64), 0.0)) / n
    state = expected_end_state(inc, mse, float(S["prev_mse"]), int(S["iterations"]), max_iterations, eps, swapped=mutant == "p6_swapped")
    S["state"] = state
    if state == RUNNING:
        S["prev_mse"] = mse
    after["work"][:, :3] = R.transform_float(inc, work)
    after["keys"][:] = NO_KEY
    return after


def model_prep(src, tgt, guess):
    """icp_prep_kernel restated: the buffers after the prep stage"""
    from direct_stereo_slam_amd.icp import STATE_DTYPE

    o, t = R.transform_double(src, guess), R.transform_double(tgt, np.eye(4))
    S = np.zeros(1, STATE_DTYPE)[0]
    S["final_tf"], S["prev_mse"], S["fitness"], S["corr"] = np.eye(4, dtype=np.float32), DBL_MAX, np.inf, -1
    S["state"] = R.EMPTY if len(o) == 0 or len(t) == 0 else RUNNING

    def f4(p):
        return np.hstack([p, np.zeros((len(p), 1), np.float32)])

    return dict(orig=f4(o), work=f4(o), target=f4(t), keys=np.full(len(o), NO_KEY), state=S)


def model_searched(before, per=None, mutant=None):
    """the buffers after a search stage"""
    after = {k: v.copy() for k, v in before.items()}
    per = len(before["target"]) if per is None else per
    after["keys"] = model_search(before["work"][:, :3], before["target"][:, :3], per, mutant)
    return after


def model_fitness_prep(before, mutant=None):
    """icp_fitness_prep_kernel restated.  Mutant "iterated_cloud": the fitness is taken on the cloud the iterations left"""
    after = {k: v.copy() for k, v in before.items()}
    if mutant != "iterated_cloud":
        after["work"][:, :3] = R.transform_float(before["state"]["final_tf"], np.ascontiguousarray(before["orig"][:, :3]))
    after["keys"][:] = NO_KEY
    return after


def model_fitness(searched):
    """icp_fitness_kernel restated (D4's order)"""
    after = {k: v.copy() for k, v in searched.items()}
    _, d = unpack_keys(searched["keys"])
    after["state"]["fitness"] = R.block_sum_order(d.astype(np.float64)) / len(d)
    return after


def device_order_moments(work, target, idx, keep):
    """(Sigma, src_mean, dst_mean) as icp_step_kernel forms them: every sum in block_sum_order, times 1 / n"""
    a, b = np.asarray(work, np.float64), np.asarray(target, np.float64)[np.where(keep, idx, 0)]
    one_over_n = 1.0 / float(keep.sum())
    sm = np.array([R.block_sum_order(np.where(keep, a[:, c], 0.0)) * one_over_n for c in range(3)])
    tm = np.array([R.block_sum_order(np.where(keep, b[:, c], 0.0)) * one_over_n for c in range(3)])
    sc, dc = a - sm, b - tm
    sigma = np.array([[R.block_sum_order(np.where(keep, dc[:, r] * sc[:, c], 0.0)) * one_over_n for c in range(3)] for r in range(3)])
    return sigma, sm, tm
