"""Test infrastructure: a numpy restatement of the ICP fallback's contract (P1-P9, D1-D5), the checker the device
(dsm_icp_batch) is compared against.  Per-point arithmetic is float32 with the stated operation orders (a numpy float32 operation is one
IEEE operation, so distances, correspondences and counts can match the device bit for bit); the moments are float64 (D1) and the SVD is
numpy's (the device runs its own Jacobi SVD: the float increments agree to rounding).  Sums that the contract orders by source index
(the MSE of P6 and the fitness of P9) are summed in that order here; the device sums them in a fixed tree order (D4).
For the stage-by-stage tests (tests/test_icp_stages.py): exact_step and exact_mean are the correctly rounded sums the device's step and
fitness are bounded against, block_sum_order restates the device's own order of a sum."""
import math

import numpy as np

ITERATIONS, TRANSFORM, ABS_MSE, NO_CORRESPONDENCES, EMPTY = 1, 2, 3, 5, 6


def transform_double(pts, T):
    """P1: T [p; 1] per row in double, ((T_i0 x + T_i1 y) + T_i2 z) + T_i3, rounded to float"""
    p = np.asarray(pts, np.float64).reshape(-1, 3)
    T = np.asarray(T, np.float64)
    out = np.empty((len(p), 3), np.float32)
    for r in range(3):
        out[:, r] = (((T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1]) + T[r, 2] * p[:, 2]) + T[r, 3]).astype(np.float32)
    return out


def transform_float(T, p):
    """P5: a float 4x4 applied to float points, ((r0 x + r1 y) + r2 z) + t"""
    T = np.asarray(T, np.float32)
    out = np.empty_like(p)
    for r in range(3):
        out[:, r] = ((T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1]) + T[r, 2] * p[:, 2]) + T[r, 3]
    return out


def nearest(src, tgt, chunk=256):
    """P2 / P9: exact nearest target of every source point by ((dx dx) + dy dy) + dz dz in float32 (d = source - target); argmin keeps
    the first minimum, i.e. the smallest target index of a tie (D2).  D5: a distance that is not finite (NaN or +inf) is never a
    minimum; a source point without a finite distance has index -1 and distance NaN (no key).
    Returns (index int64, dist2 float32)."""
    idx = np.empty(len(src), np.int64)
    dist = np.empty(len(src), np.float32)
    tgt_finite = bool(np.isfinite(tgt).all())
    for a in range(0, len(src), chunk):
        s = src[a:a + chunk]
        with np.errstate(over="ignore", invalid="ignore"):
            dx = s[:, 0:1] - tgt[None, :, 0]
            dy = s[:, 1:2] - tgt[None, :, 1]
            dz = s[:, 2:3] - tgt[None, :, 2]
            d = (dx * dx + dy * dy) + dz * dz
        if not (tgt_finite and np.isfinite(s).all()):  # finite points give a finite or a +inf (overflowed) distance, never a NaN
            d = np.where(np.isnan(d), np.float32(np.inf), d)
        i = np.argmin(d, axis=1)
        di = d[np.arange(len(s)), i]
        none = ~np.isfinite(di)
        idx[a:a + chunk] = np.where(none, -1, i)
        dist[a:a + chunk] = np.where(none, np.float32(np.nan), di)
    return idx, dist


def umeyama(src, dst):
    """P4 / D1: Eigen::umeyama without scaling, in float64: (R, t) with dst ~ R src + t"""
    src = np.asarray(src, np.float64)
    dst = np.asarray(dst, np.float64)
    one_over_n = 1.0 / len(src)
    sm, dm = src.sum(0) * one_over_n, dst.sum(0) * one_over_n
    sigma = one_over_n * ((dst - dm).T @ (src - sm))
    U, _, Vt = np.linalg.svd(sigma)
    S = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2] = -1.0
    R = U @ np.diag(S) @ Vt
    return R, dm - R @ sm


def ordered_sum(x):
    """a float64 sum in index order (numpy's sum is pairwise)"""
    x = np.asarray(x, np.float64)
    return float(np.cumsum(x)[-1]) if len(x) else 0.0


def exact_step(work, target, idx, keep):
    """P4 without D1's order: the increment of the kept pairs (work[i], target[idx[i]]) from correctly rounded sums -- the means are
    math.fsum of the float coordinates as doubles over n, Sigma is math.fsum of the products of the coordinates centred on those means
    over n -- then numpy's SVD and the determinant fix.  Returns (R, t) in double."""
    s = np.asarray(work, np.float64)[keep]
    d = np.asarray(target, np.float64)[np.asarray(idx)[keep]]
    n = len(s)
    sm = np.array([math.fsum(s[:, c]) for c in range(3)]) / n
    dm = np.array([math.fsum(d[:, c]) for c in range(3)]) / n
    sc, dc = s - sm, d - dm
    sigma = np.array([[math.fsum(dc[:, r] * sc[:, c]) for c in range(3)] for r in range(3)]) / n
    U, _, Vt = np.linalg.svd(sigma)
    S = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2] = -1.0
    Rm = U @ np.diag(S) @ Vt
    return Rm, dm - Rm @ sm


def exact_mean(d):
    """P6 / P9 without D4's order: math.fsum of the float distances as doubles, over their number"""
    d = np.asarray(d, np.float64)
    return math.fsum(d) / len(d)


def block_sum_order(x, lanes=256):
    """D1 / D4: the sum of one double per source point in the device's order -- lane t of 256 adds x[t], x[t + 256], ... in turn from
    0.0 (a point that is not a kept pair is passed as 0.0: the lane skips it), then the halving tree red[t] += red[t + s] for
    s = 128, 64, .. 1.  Every operation is one IEEE double addition, as on the device."""
    x = np.asarray(x, np.float64).ravel()
    rows = -(-len(x) // lanes)
    padded = np.zeros(rows * lanes)
    padded[:len(x)] = x
    red = np.zeros(lanes)
    for row in padded.reshape(rows, lanes):
        red = red + row
    s = lanes // 2
    while s > 0:
        red[:s] = red[:s] + red[s:2 * s]
        s //= 2
    return float(red[0])


def icp(src, tgt, tfm, max_iterations=5, eps=0.01, max_corr_dist=2.0, score_thres=1.5, trace=None, search=None):
    """icp.h:44-71 with PCL's semantics as restated in P1-P9: returns dict(ok, tfm, score, iterations, state, corr_counts).
    trace: a list that receives dict(work, final, inc) after every increment (the iterated cloud and both float matrices);
    search: a stand-in for `nearest` (tests of the tests: what a wrong search does to the result)"""
    search = nearest if search is None else search
    guess = np.asarray(tfm, np.float64).reshape(4, 4)
    src = np.asarray(src, np.float64).reshape(-1, 3)
    tgt = np.asarray(tgt, np.float64).reshape(-1, 3)
    if len(src) == 0 or len(tgt) == 0:  # D3
        return dict(ok=False, tfm=guess.copy(), score=np.float32(np.inf), iterations=0, state=EMPTY, corr_counts=[])
    orig = transform_double(src, guess)
    target = transform_double(tgt, np.eye(4))
    work = orig.copy()
    final = np.eye(4, dtype=np.float32)
    prev_mse = np.finfo(np.float64).max
    it, state, counts = 0, 0, []
    max_d2 = max_corr_dist * max_corr_dist
    while state == 0:
        idx, d = search(work, target)
        keep = d.astype(np.float64) <= max_d2
        n = int(keep.sum())
        counts.append(n)
        if n < 3:  # P3
            state = NO_CORRESPONDENCES
            break
        R, t = umeyama(work[keep], target[idx[keep]])
        inc = np.eye(4, dtype=np.float32)
        inc[:3, :3], inc[:3, 3] = R.astype(np.float32), t.astype(np.float32)
        mse = ordered_sum(d[keep]) / n  # P6.3: this iteration's pairs, before the increment
        work = transform_float(inc, work)  # P5
        F = np.empty((4, 4), np.float32)
        for r in range(4):
            for c in range(4):
                F[r, c] = ((inc[r, 0] * final[0, c] + inc[r, 1] * final[1, c]) + inc[r, 2] * final[2, c]) + inc[r, 3] * final[3, c]
        final = F
        it += 1
        if trace is not None:
            trace.append(dict(work=work.copy(), final=final.copy(), inc=inc.copy()))
        cos_angle = 0.5 * float(((inc[0, 0] + inc[1, 1]) + inc[2, 2]) - np.float32(1))
        tr2 = (inc[0, 3] * inc[0, 3] + inc[1, 3] * inc[1, 3]) + inc[2, 3] * inc[2, 3]
        if it >= max_iterations:  # P6, in PCL's order
            state = ITERATIONS
        elif cos_angle >= 1.0 - eps and float(tr2) <= eps:
            state = TRANSFORM
        elif abs(mse - prev_mse) < 1e-12:
            state = ABS_MSE
        else:
            prev_mse = mse
    Fd = final.astype(np.float64)  # P8
    out = np.empty((4, 4))
    for r in range(4):
        for c in range(4):
            out[r, c] = ((Fd[r, 0] * guess[0, c] + Fd[r, 1] * guess[1, c]) + Fd[r, 2] * guess[2, c]) + Fd[r, 3] * guess[3, c]
    _, dfit = search(transform_float(final, orig), target)  # P9: the original source, no distance limit
    score = np.float32(ordered_sum(dfit) / len(dfit))
    return dict(ok=bool(float(score) < score_thres), tfm=out, score=score, iterations=it, state=state, corr_counts=counts)


def rot(rotvec):
    """rotation matrix of a rotation vector (Rodrigues)"""
    w = np.asarray(rotvec, np.float64)
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def rigid(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def canyon(rng, n, span=30.0):
    """a street canyon in a camera frame (y down, z forward): ground, two walls, clutter"""
    g = np.stack([rng.uniform(-span, span, n), 1.6 + rng.normal(0, 0.05, n), rng.uniform(-span, span, n)], 1)
    walls = rng.random(n) < 0.35
    g[walls, 0] = np.where(rng.random(walls.sum()) < 0.5, 8.0, -9.0) + rng.normal(0, 0.05, walls.sum())
    g[walls, 1] = rng.uniform(-5, 1.6, walls.sum())
    clutter = rng.random(n) < 0.15
    g[clutter] = rng.uniform([-8, -3, -span], [8, 1.6, span], (clutter.sum(), 3))
    return g


def scene(seed, n_src, n_tgt=None, rotvec=(0.0, 0.02, 0.0), trans=(0.1, 0.0, 0.05), noise=0.02, overlap=0.8):
    """(source, target, T_true): target = T_true * source + noise over a partial overlap -- source and target are two samplings of
    one canyon, `overlap` of the target's points drawn near the source's own"""
    rng = np.random.default_rng(seed)
    n_tgt = n_src if n_tgt is None else n_tgt
    world = canyon(rng, max(n_src, n_tgt) * 2)
    src = world[rng.choice(len(world), n_src, replace=False)]
    n_common = int(overlap * n_tgt)
    common = src[rng.choice(n_src, n_common, replace=n_common > n_src)]
    fresh = world[rng.choice(len(world), n_tgt - n_common, replace=False)]
    T = rigid(rot(rotvec), np.asarray(trans, np.float64))
    tgt = np.vstack([common, fresh]) @ T[:3, :3].T + T[:3, 3] + rng.normal(0, noise, (n_tgt, 3))
    return src, tgt, T


def blobs(seed, n, rotvec, trans, noise=0.02):
    """(source, target, T_true): twelve compact clusters, target = T_true * source + noise (a scene ICP walks through slowly)"""
    rng = np.random.default_rng(seed)
    centers = rng.uniform(-6, 6, (12, 3))
    src = centers[rng.integers(0, 12, n)] + rng.normal(0, 0.8, (n, 3))
    T = rigid(rot(rotvec), np.asarray(trans, np.float64))
    return src, src @ T[:3, :3].T + T[:3, 3] + rng.normal(0, noise, (n, 3)), T


def street(rng, n):
    """one place in world coordinates: a 17 m wide street (y down), its two facades and 24 poles along the kerbs -- structure in
    every direction, so that ICP can pin the along-street translation"""
    g = np.stack([rng.uniform(-9, 8, n), 1.6 + rng.normal(0, 0.05, n), rng.uniform(-35, 35, n)], 1)
    kind = rng.random(n)
    walls = kind < 0.35
    g[walls, 0] = np.where(rng.random(walls.sum()) < 0.5, 8.0, -9.0)
    g[walls, 1] = rng.uniform(-5, 1.6, walls.sum())
    poles = kind > 0.8
    k = rng.integers(0, 24, poles.sum())
    g[poles, 0] = np.where(k < 12, 5.5, -6.5) + rng.normal(0, 0.1, poles.sum())
    g[poles, 2] = np.linspace(-30, 30, 12)[k % 12] + rng.normal(0, 0.1, poles.sum())
    g[poles, 1] = rng.uniform(-4, 1.6, poles.sum())
    return g


def pose_error(T_est, T_true):
    """(rotation error in degrees, translation error in m) of T_est against T_true"""
    E = np.linalg.inv(T_true) @ T_est
    return float(np.degrees(np.arccos(np.clip((np.trace(E[:3, :3]) - 1) / 2, -1, 1)))), float(np.linalg.norm(E[:3, 3]))


def ties(seed, n=300, a=0.5):
    """(source, target, target_swapped): every source point has two distinct targets at EXACTLY the same float distance, s + a e and
    s - a e with e a coordinate axis (all coordinates are multiples of 0.5 on a 4 m lattice, exact in float; every other target is
    3.5 m away or more).  The + target has the smaller index in `target` and the larger in `target_swapped`, so the tie-break (D2)
    decides which of two different cross-covariances the first increment is fitted to.  The first half of the pairs sit at adjacent
    indices, the second half n/2 indices apart (another LDS tile or target slice of the device's search)."""
    rng = np.random.default_rng(seed)
    axis = np.arange(-20.0, 21.0, 4.0)
    lattice = np.stack(np.meshgrid(axis, axis, axis, indexing="ij"), -1).reshape(-1, 3)
    src = lattice[rng.choice(len(lattice), n, replace=False)]
    e = np.eye(3)[rng.integers(0, 3, n)]
    plus, minus = src + a * e, src - a * e
    h = n // 2

    def order(lo, hi):
        adjacent = np.stack([lo[:h], hi[:h]], 1).reshape(-1, 3)
        return np.vstack([adjacent, lo[h:], hi[h:]])

    return src, order(plus, minus), order(minus, plus)
