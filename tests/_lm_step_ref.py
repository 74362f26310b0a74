"""Host references of the LM step (the half of a Levenberg-Marquardt round that turns H, b and lambda into the next candidate) and the
seeded case generators that tests/test_lm_step.py runs on the CPU and on the device.  CPU only.

  step_oracle    the pose step exactly as orc_track writes it (oracle/dsm_oracle.c:705-760) around the oracle's own orc_ldlt_solve,
                 orc_se3_exp, orc_se3_mul and orc_quat_to_rot; the float32 pieces (1 + lambda, extrapFac, the cut-off, R K^-1) in numpy
                 float32 with the oracle's operation order
  scale_step_ref propose_scale (TrackerAndScaler.cpp:897-913) in numpy float32
  py_ldlt_solve  orc_ldlt_solve restated in Python floats, with the tie-break of the pivot search switchable
  solve_exact    the same linear system in fractions.Fraction
  se3_exp_mp     the matrix exponential in mpmath at 50 digits
"""
import ctypes as C
import functools
import math
from fractions import Fraction

import numpy as np

from oracle import oracle as O

F32 = np.float32
EPS = 2.0 ** -53
MODES = {"ab": (0.0, 0.0), "fix_ab": (-1.0, -1.0), "fix_b": (0.0, -1.0), "fix_a": (-1.0, 0.0)}  # affine_opt_mode_a, _b
LAMBDAS = (1e-4, 0.01, 40.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# bits
# ---------------------------------------------------------------------------------------------------------------------------------
def bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def bits32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b, nan_as_nan=False):
    """every value has the same bit pattern (signed zeros and infinities included); nan_as_nan: a NaN equals any NaN -- the sign and
    payload of a NaN an operation produces are the processor's choice, not IEEE's"""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape
    view = bits64 if a.dtype == np.float64 else bits32
    eq = view(a) == view(b)
    if nan_as_nan:
        eq = eq | (np.isnan(a) & np.isnan(b))
    return bool(np.all(eq))


# ---------------------------------------------------------------------------------------------------------------------------------
# the oracle's pieces
# ---------------------------------------------------------------------------------------------------------------------------------
def _dp(a):
    return a.ctypes.data_as(O.c_double_p)


def orc_ldlt(A, rhs):
    A = np.ascontiguousarray(A, np.float64)
    n = A.shape[0]
    rhs = np.ascontiguousarray(rhs, np.float64)
    x = np.zeros(n)
    O.lib().orc_ldlt_solve(n, _dp(A), _dp(rhs), _dp(x))
    return x


def orc_se3_exp(xi):
    out = np.zeros(7)
    O.lib().orc_se3_exp(_dp(np.ascontiguousarray(xi[:6], np.float64)), _dp(out))
    return out


def orc_se3_mul(a, b):
    out = np.zeros(7)
    O.lib().orc_se3_mul(_dp(np.ascontiguousarray(a, np.float64)), _dp(np.ascontiguousarray(b, np.float64)), _dp(out))
    return out


def orc_quat_to_rot(q):
    R = np.zeros(9)
    O.lib().orc_quat_to_rot(_dp(np.ascontiguousarray(q[:4], np.float64)), _dp(R))
    return R


def mat3f_mul(a, b):
    """the float ((a0 b0 + a1 b1) + a2 b2) product of two row-major 3x3 matrices"""
    a, b = np.asarray(a, F32).reshape(3, 3), np.asarray(b, F32).reshape(3, 3)
    o = np.zeros((3, 3), F32)
    for i in range(3):
        for j in range(3):
            o[i, j] = (a[i, 0] * b[0, j] + a[i, 1] * b[1, j]) + a[i, 2] * b[2, j]
    return o.reshape(9)


def eval_rot(mode, pose, Ki):
    """M, t of a candidate pose as the evaluation reads them: float(R) K^-1 (mode 2: float(R)), float(t)"""
    Rf = orc_quat_to_rot(pose).astype(F32)
    M = Rf if mode == 2 else mat3f_mul(Rf, Ki)
    return M, np.asarray(pose[4:7], np.float64).astype(F32)


def extrap_fac(params, lam):
    lim, lam = F32(params.lambda_extrapolation_limit), F32(lam)
    return np.sqrt(np.sqrt(lim / lam)) if lam < lim else F32(1)


def level_max_it(params, lvl):
    return params.fixed_schedule if params.fixed_schedule > 0 else params.max_iterations[lvl]


def cutoff_of(params, level_cutoff_repeat):
    h, cutoff = F32(params.huber_th), F32(params.coarse_cutoff_th) * F32(level_cutoff_repeat)
    return cutoff, F32(2) * h * cutoff - h * h


def scales_of(params):
    r, t = float(params.scale_xi_rot), float(params.scale_xi_trans)
    return np.array([r, r, r, t, t, t, float(params.scale_a), float(params.scale_b)])


def raw_increment(params, H, b, lam, solve=orc_ldlt):
    """inc of oracle/dsm_oracle.c:706-743: the full solve, replaced by the 6-, 7- or stitched 7-dim solve under the affine modes"""
    H = np.asarray(H, np.float64).reshape(8, 8)
    b = np.asarray(b, np.float64)
    lam1 = float(F32(1) + F32(lam))
    Hl = H.copy()
    for i in range(8):
        Hl[i, i] = Hl[i, i] * lam1
    nb = -b
    inc = solve(Hl, nb)
    fix_a, fix_b = params.affine_opt_mode_a < 0, params.affine_opt_mode_b < 0
    if fix_a and fix_b:
        inc = np.concatenate([solve(Hl[:6, :6], nb[:6]), [0.0, 0.0]])
    elif fix_b:
        inc = np.concatenate([solve(Hl[:7, :7], nb[:7]), [0.0]])
    elif fix_a:
        Hs, bs = Hl.copy(), b.copy()
        Hs[:, 6] = Hs[:, 7]
        Hs[6, :] = Hs[7, :]
        bs[6] = bs[7]
        x7 = solve(Hs[:7, :7], -bs[:7])
        inc = np.concatenate([x7[:6], [0.0, x7[6]]])
    return np.asarray(inc, np.float64)


def step_oracle(params, mode, lvl, H, b, lam, cur, aff_cur, iteration, level_cutoff_repeat=1.0, spec=False, solve=orc_ldlt, Ki=None):
    """one proposal of orc_track's loop.  Returns a dict: inc (raw), inc_scaled, inc_norm, cand, aff_cand, residual_only, cutoff,
    max_energy and, given the level's K^-1, M and t."""
    inc_raw = raw_increment(params, H, b, lam, solve)
    with np.errstate(all="ignore"):
        inc = inc_raw * float(extrap_fac(params, lam))
        inc_scaled = inc * scales_of(params)
        total = 0.0
        for v in inc_scaled:
            total += v
        if not math.isfinite(total):
            inc_scaled = np.zeros(8)
        ex = orc_se3_exp(inc_scaled)
        cand = orc_se3_mul(ex, cur)
        aff_cand = np.array([aff_cur[0] + inc_scaled[6], aff_cur[1] + inc_scaled[7]])
        nrm = 0.0
        for v in inc:
            nrm += v * v
        inc_norm = np.sqrt(np.float64(nrm))
    last = (params.fixed_schedule <= 0 and not inc_norm > 1e-3) or iteration + (2 if spec else 1) >= level_max_it(params, lvl)
    cutoff, max_energy = cutoff_of(params, level_cutoff_repeat)
    r = dict(inc=inc_raw, inc_scaled=inc_scaled, inc_norm=inc_norm, cand=cand, aff_cand=aff_cand, residual_only=int(last),
             cutoff=cutoff, max_energy=max_energy)
    if Ki is not None:
        r["M"], r["t"] = eval_rot(mode, cand, Ki)
    return r


def scale_step_ref(params, lvl, Hs, bs, scale_cur, lam, iteration, level_cutoff_repeat=1.0, spec=False):
    """propose_scale: TrackerAndScaler.cpp:897-913 in float32; returns (inc, scale_cand, residual_only, cutoff, max_energy)"""
    with np.errstate(all="ignore"):
        Hl = F32(Hs) * (F32(1) + F32(lam))
        inc = -F32(bs) / Hl
        inc = inc * extrap_fac(params, lam)
        if not np.isfinite(inc) or np.abs(inc) > F32(scale_cur):
            inc = F32(0)
        cand = F32(scale_cur) + inc
    last = (params.fixed_schedule <= 0 and not float(inc) > 1e-3) or iteration + (2 if spec else 1) >= level_max_it(params, lvl)
    return (F32(inc), F32(cand), int(last)) + cutoff_of(params, level_cutoff_repeat)


# ---------------------------------------------------------------------------------------------------------------------------------
# orc_ldlt_solve in Python floats (IEEE double, no contraction), operation for operation; larger_index_on_ties: the pivot search takes
# the LAST maximum of the remaining diagonal instead of the first
# ---------------------------------------------------------------------------------------------------------------------------------
def py_ldlt_solve(Ain, rhs, larger_index_on_ties=False):
    n = len(rhs)
    A = [[float(Ain[i][j]) for j in range(n)] for i in range(n)]
    tr = list(range(n))
    all_zero = False
    temp = [0.0] * n
    for k in range(n):
        big, bigv = k, abs(A[k][k])
        for i in range(k + 1, n):
            v = abs(A[i][i])
            if v > bigv or (larger_index_on_ties and v == bigv):
                bigv, big = v, i
        tr[k] = big
        if k != big:
            for j in range(k):
                A[k][j], A[big][j] = A[big][j], A[k][j]
            for i in range(big + 1, n):
                A[i][k], A[i][big] = A[i][big], A[i][k]
            A[k][k], A[big][big] = A[big][big], A[k][k]
            for i in range(k + 1, big):
                A[i][k], A[big][i] = A[big][i], A[i][k]
        rs = n - k - 1
        if k > 0:
            for j in range(k):
                temp[j] = A[j][j] * A[k][j]
            dot = 0.0
            for j in range(k):
                dot += A[k][j] * temp[j]
            A[k][k] -= dot
            for i in range(rs):
                s = 0.0
                for j in range(k):
                    s += A[k + 1 + i][j] * temp[j]
                A[k + 1 + i][k] -= s
        akk = A[k][k]
        valid = abs(akk) > 0.0
        if k == 0 and not valid:
            all_zero = True
            break
        if rs > 0 and valid:
            for i in range(rs):
                A[k + 1 + i][k] = _div(A[k + 1 + i][k], akk)
    y = [float(v) for v in rhs]
    if all_zero:
        return np.zeros(n)
    for k in range(n):
        y[k], y[tr[k]] = y[tr[k]], y[k]
    for i in range(n):
        for j in range(i):
            y[i] -= A[i][j] * y[j]
    tol = 1.0 / 1.7976931348623157e308
    for i in range(n):
        y[i] = _div(y[i], A[i][i]) if abs(A[i][i]) > tol else 0.0
    for i in range(n - 1, -1, -1):
        for j in range(i + 1, n):
            y[i] -= A[j][i] * y[j]
    for k in range(n - 1, -1, -1):
        y[k], y[tr[k]] = y[tr[k]], y[k]
    return np.array(y)


def _div(a, b):
    """IEEE division (Python raises on a zero divisor; the callers above never divide by zero, but infinities and NaNs pass through)"""
    return float(np.float64(a) / np.float64(b))


def py_solve_larger_index(A, rhs):
    return py_ldlt_solve(np.asarray(A), np.asarray(rhs), larger_index_on_ties=True)


def py_solve(A, rhs):
    return py_ldlt_solve(np.asarray(A), np.asarray(rhs))


def takes_slow_path(params, H, lam):
    """the device's wave-uniform `slow` predicate, from its definition: two ACTIVE diagonal entries of the damped system equal in
    magnitude, or one of them NaN (the pivot order is then Eigen's swaps', not the ranks')"""
    H = np.asarray(H, np.float64).reshape(8, 8)
    fix_a, fix_b = params.affine_opt_mode_a < 0, params.affine_opt_mode_b < 0
    rows = list(range(6)) if fix_a and fix_b else list(range(7)) if fix_b else [0, 1, 2, 3, 4, 5, 7] if fix_a else list(range(8))
    lam1 = float(F32(1) + F32(lam))
    with np.errstate(all="ignore"):
        d = [abs(H[i, i] * lam1) for i in rows]
    return any(math.isnan(v) for v in d) or len(set(d)) < len(d)


# ---------------------------------------------------------------------------------------------------------------------------------
# exact and high-precision references
# ---------------------------------------------------------------------------------------------------------------------------------
def solve_exact(A, rhs):
    """A x = rhs over the rationals (Gauss-Jordan with Fractions of the doubles' exact values); A must be non-singular"""
    n = len(rhs)
    M = [[Fraction(float(A[i][j])) for j in range(n)] + [Fraction(float(rhs[i]))] for i in range(n)]
    for c in range(n):
        p = next(r for r in range(c, n) if M[r][c] != 0)
        M[c], M[p] = M[p], M[c]
        inv = 1 / M[c][c]
        M[c] = [v * inv for v in M[c]]
        for r in range(n):
            if r != c and M[r][c] != 0:
                f = M[r][c]
                M[r] = [a - f * b for a, b in zip(M[r], M[c])]
    return [M[i][n] for i in range(n)]


def _mp():
    import mpmath

    mpmath.mp.dps = 50
    return mpmath


def se3_exp_mp(xi):
    """exp of the twist [upsilon ; omega] as a 4x4 mpmath matrix"""
    mp = _mp()
    u, o = [mp.mpf(float(v)) for v in xi[:3]], [mp.mpf(float(v)) for v in xi[3:6]]
    A = mp.matrix(4, 4)
    A[0, 1], A[0, 2], A[1, 0], A[1, 2], A[2, 0], A[2, 1] = -o[2], o[1], o[2], -o[0], -o[1], o[0]
    for i in range(3):
        A[i, 3] = u[i]
    return mp.expm(A)


def pose_to_mp(pose):
    """{qx,qy,qz,qw,t} -> 4x4 mpmath matrix (the quaternion normalised in mpmath)"""
    mp = _mp()
    x, y, z, w = [mp.mpf(float(v)) for v in pose[:4]]
    n = mp.sqrt(x * x + y * y + z * z + w * w)
    x, y, z, w = x / n, y / n, z / n, w / n
    T = mp.eye(4)
    R = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
         [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
         [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
    for i in range(3):
        for j in range(3):
            T[i, j] = R[i][j]
        T[i, 3] = mp.mpf(float(pose[4 + i]))
    return T


def mp_errors(cand, truth, theta, ups_norm):
    """(rotation error, translation error) of a double-precision pose against an mpmath 4x4: the largest rotation-matrix entry
    difference in units of 2^-53, and the largest translation difference in units of 2^-53 ((1 + 1/theta) |upsilon| + |t|) -- the
    scale of the rounding errors of V upsilon + R t_cur"""
    mp = _mp()
    D = pose_to_mp(cand) - truth
    rot = max(abs(D[i, j]) for i in range(3) for j in range(3))
    tn = mp.sqrt(sum(truth[i, 3] ** 2 for i in range(3)))
    tr = max(abs(D[i, 3]) for i in range(3))
    unit = mp.mpf(EPS) * ((1 + 1 / mp.mpf(theta)) * mp.mpf(ups_norm) + tn)
    return float(rot / mp.mpf(EPS)), float(tr / unit) if unit > 0 else (0.0 if tr == 0 else float("inf"))


# ---------------------------------------------------------------------------------------------------------------------------------
# case generators (seeded; shared by the CPU and the GPU tests)
# ---------------------------------------------------------------------------------------------------------------------------------
def _spd(rng, decades, scale=1.0):
    Q, _ = np.linalg.qr(rng.normal(size=(8, 8)))
    A = (Q * 10.0 ** rng.uniform(-decades / 2.0, decades / 2.0, 8)) @ Q.T
    return (A + A.T) * (0.5 * scale)


def _gn_like(rng, rows=40):
    """J^T J of a Jacobian whose columns have the magnitudes of the tracker's (rotation, translation, affine a, b)"""
    J = rng.normal(size=(rows, 8)) * np.array([30, 30, 30, 8, 8, 8, 900, 1000.0])
    return J.T @ J / rows


@functools.lru_cache(maxsize=None)
def finite_systems():
    """[(class name, H, b, has_ties)]: every matrix class of the finite-systems test.  Every entry is finite."""
    rng = np.random.default_rng(0x1D17)
    out = []

    def add(name, H, b=None):
        H = np.array(H, np.float64)
        out.append((name, H, rng.normal(size=8) * (np.abs(H).max() or 1.0) * 1e-2 if b is None else np.asarray(b, np.float64)))

    for k in range(13):  # SPD over 12 decades of scale, condition numbers 1e0 .. 1e8
        add("spd", _spd(rng, decades=(k % 5) * 2.0, scale=10.0 ** (k - 6)))
    for _ in range(8):
        add("gn", _gn_like(rng))
    for pair in ((0, 1), (2, 5), (6, 7), (3, 7), (5, 6), (0, 7)):  # ties of two
        H = _gn_like(rng)
        H[pair[1], pair[1]] = H[pair[0], pair[0]]
        add("tie2", H)
        H = _spd(rng, 2.0)
        H[pair[1], pair[1]] = H[pair[0], pair[0]]
        add("tie2", H)
    for quad in ((0, 1, 2, 3), (4, 5, 6, 7), (0, 2, 5, 7), (1, 3, 6, 7)):  # ties of four
        H = _gn_like(rng)
        for i in quad[1:]:
            H[i, i] = H[quad[0], quad[0]]
        add("tie4", H)
    for pair in ((0, 1), (4, 6), (6, 7), (2, 7), (5, 6)):  # ties of opposite sign
        H = _spd(rng, 2.0)
        H[pair[1], pair[1]] = -H[pair[0], pair[0]]
        add("tie_opposite", H)
        H = _gn_like(rng)
        H[pair[0], pair[0]] = -H[pair[1], pair[1]]
        add("tie_opposite", H)
    for s in (1.0, 3.7e-3, 2.5e6, -1.0):  # all-equal diagonal (the identity among them)
        H = _spd(rng, 1.0) * 0.1
        np.fill_diagonal(H, s)
        add("equal_diag", H)
        add("equal_diag", np.eye(8) * s)
    add("zero", np.zeros((8, 8)))
    add("zero", np.zeros((8, 8)), np.zeros(8))
    for _ in range(3):  # zero diagonal, off-diagonals present
        H = rng.normal(size=(8, 8))
        H = H + H.T
        np.fill_diagonal(H, 0.0)
        add("zero_diag", H)
    for _ in range(4):  # rank 5
        J = rng.normal(size=(5, 8))
        add("rank5", J.T @ J)
    for rows in ((3,), (7,), (6,), (0, 4), (6, 7), (2, 7)):  # one and two zero rows / columns
        H = _gn_like(rng)
        for r in rows:
            H[r, :] = 0
            H[:, r] = 0
        add("zero_rows", H)
    for _ in range(5):
        H = rng.normal(size=(8, 8))
        add("indefinite", H + H.T)
    for _ in range(3):
        add("negative_definite", -_spd(rng, 3.0))
    for i in (0, 5, 6, 7):
        H = _spd(rng, 2.0)
        H[i, i] = 1e12
        add("dominant", H)
    for s in (1e300, 1e-300):
        H = _spd(rng, 2.0)
        add("extreme_scale", H * s, rng.normal(size=8) * s)
        add("extreme_scale", H * s, rng.normal(size=8))
    for i, z in ((0, 0.0), (3, -0.0), (7, -0.0), (6, 0.0)):  # +-0 on the diagonal
        H = _spd(rng, 2.0)
        H[i, i] = z
        add("signed_zero_diag", H)
    H = np.zeros((8, 8))
    np.fill_diagonal(H, [0.0, -0.0] * 4)
    add("signed_zero_diag", H)
    for s in (0.5e-3, 0.999e-3, 1.001e-3, 2e-3):  # |inc| on both sides of 1e-3 (H = I: inc = -b / (1 + lambda), times extrapFac)
        for lam in LAMBDAS:
            v = rng.normal(size=8)
            scale = s * float(F32(1) + F32(lam)) / float(extrap_fac(O.default_params(), lam))
            add("inc_norm_edge", np.eye(8), v / np.linalg.norm(v) * scale)
    assert all(np.all(np.isfinite(H)) and np.all(np.isfinite(b)) for _, H, b in out)
    return tuple(out)


SENTINELS = (12345.678, float("nan"))  # written over the strict upper triangle: only the lower one is the system


def finite_problems(max_it):
    """[(class, H as handed over (upper triangle overwritten), b, lambda, iteration)]: every finite system at every lambda, the
    iteration cycling over values on both sides of the iteration bound for the plain and the speculative proposal"""
    its = (0, max_it - 3, max_it - 2, max_it - 1)
    out = []
    for n, (name, H, b) in enumerate(finite_systems()):
        for k, lam in enumerate(LAMBDAS):
            Hin = H.copy()
            Hin[np.triu_indices(8, 1)] = SENTINELS[(n + k) % 2]
            out.append((name, Hin, b, lam, its[(n + k) % 4]))
    return out


def lower_symmetric(H):
    """the system a lower-triangle reader sees"""
    L = np.tril(np.asarray(H, np.float64).reshape(8, 8))
    return L + np.tril(L, -1).T


@functools.lru_cache(maxsize=None)
def nonfinite_problems():
    """[(H, b, lambda)]: NaN, +Inf and -Inf at every diagonal position and at off-diagonal positions of every block the affine modes
    treat differently (inside the 6x6 block, rows 6 and 7, their crossing), and in b"""
    rng = np.random.default_rng(0xBAD)
    out = []
    for k, bad in enumerate((float("nan"), float("inf"), -float("inf"))):
        for i in range(8):
            H = _gn_like(rng)
            H[i, i] = bad
            out.append((H, rng.normal(size=8), LAMBDAS[(i + k) % 3]))
        for (i, j) in ((1, 0), (5, 2), (6, 3), (7, 4), (7, 6), (6, 0), (7, 0)):
            H = _gn_like(rng)
            H[i, j] = bad  # the lower triangle is the system
            H[j, i] = bad
            out.append((H, rng.normal(size=8), LAMBDAS[(i + j + k) % 3]))
        for i in (0, 5, 6, 7):
            b = rng.normal(size=8)
            b[i] = bad
            out.append((_gn_like(rng), b, 0.01))
    H = np.full((8, 8), float("nan"))
    out.append((H, np.full(8, float("nan")), 0.01))
    # a zero diagonal under non-finite off-diagonals: the first pivot is zero and Eigen's all_zero rule answers with the zero vector --
    # the one place where the rule shows (on finite input the zero pivots send every unknown through the 1 / highest() rule to the
    # same zeros)
    for bad in (float("nan"), float("inf")):
        for (i, j) in ((1, 0), (4, 2), (7, 5)):
            H = rng.normal(size=(8, 8))
            H = H + H.T
            np.fill_diagonal(H, 0.0)
            H[i, j] = H[j, i] = bad
            out.append((H, rng.normal(size=8), 0.01))
    return tuple(out)


THETAS = (0.0, 1e-300, 9.9e-11, 1.0e-10, 1.1e-10, 1e-8, 1e-6, 1e-4, 1e-3, 0.3, math.pi - 1e-9, math.pi, math.pi + 1e-9,
          2 * math.pi - 1e-9, 2 * math.pi + 1e-9, 7.0, 100.0)
UPSILONS = (0.0, 1e-3, 1.0, 1e3)


@functools.lru_cache(maxsize=None)
def se3_cases():
    """[(xi (the scaled twist the step should exponentiate), cur)]: every theta x axis x |upsilon| x current pose"""
    rng = np.random.default_rng(0x5E3)
    axes = [np.array(a, np.float64) for a in ((1, 0, 0), (0, 1, 0), (0, 0, 1))]
    for _ in range(2):
        v = rng.normal(size=3)
        axes.append(v / np.linalg.norm(v))
    far_q = rng.normal(size=4)
    far_q /= np.linalg.norm(far_q)
    far_t = rng.normal(size=3)
    far_t *= 1e3 / np.linalg.norm(far_t)
    curs = (np.array([0, 0, 0, 1, 0, 0, 0.0]), np.concatenate([far_q, far_t]))
    out = []
    for theta in THETAS:
        for a, axis in enumerate(axes):
            for un in UPSILONS:
                d = axes[(a + 1) % len(axes)] if a < 3 else rng.normal(size=3)
                ups = d / np.linalg.norm(d) * un
                for cur in curs:
                    out.append((np.concatenate([ups, axis * theta]), cur))
    return tuple(out)


def se3_system(params, xi, lam=1.0):
    """H = I and the b that makes the step exponentiate xi: inc = -b / (1 + lambda), xi = inc * SCALE (lambda = 1: 1 + lambda = 2 and
    extrapFac = 1, so with power-of-two scales the round trip is exact)"""
    sc = scales_of(params)
    b = np.zeros(8)
    b[:6] = -(xi / sc[:6]) * float(F32(1) + F32(lam))
    return np.eye(8), b


@functools.lru_cache(maxsize=None)
def scale_cases():
    """[(Hs, bs, scale_cur, lambda)] of the scale step"""
    nan = float("nan")
    out = []
    for lam in (1e-4, 0.5e-3, 0.001, 0.002, 0.01, 40.0):  # both sides of (and at) lambda_extrapolation_limit = 0.001
        for Hs in (0.0, -0.0, 1e-38, 1e-45, -2.5, 3.0, 1e30):
            for bs in (0.0, 0.7, -0.7, 1e-3, -1e30):
                for sc in (0.1, 1.0, 25.0):
                    out.append((Hs, bs, sc, lam))
        # |inc| on both sides of scale_cur: inc = -bs / (Hs (1 + lambda)) extrapFac
        for k in (0.999, 1.0, 1.001, -0.999, -1.001):
            out.append((2.0, -2.0 * k, 1.0, lam))
        # inc on both sides of 1e-3 (the signed break test)
        for k in (0.9e-3, 1.1e-3, -5e-3):
            out.append((1.0, -k, 1.0, lam))
        out += [(nan, 1.0, 1.0, lam), (1.0, nan, 1.0, lam), (1.0, 1.0, nan, lam), (float("inf"), 1.0, 1.0, lam), (1.0, float("inf"), 1.0, lam)]
    out.append((1.0, 1.0, 1.0, nan))
    return tuple(out)
