"""Independent checker of the stitch's use, damping, solve and back-substitution of the window optimisation: the
rules F1-F8 and R1-R3 as the project states them, on top of the results of the accumulation's checker (tests/_hessian_ref.py, whose
stitch is T1 and therefore T1d).  float32 scalars and arrays where the rules say float (every operation rounds once), float64 sums
as Python loops in the stated order.  The LDLT is a fresh N-dimensional restatement of the rules the project states for its 8 x 8
solve (the comment above wave_ldlt_solve8, orc_ldlt_solve): the unblocked, left-looking, lower-triangle algorithm with the literal
pivot selection loop and its swap bookkeeping.  Written from the statement, not from the C code.

solve(job, hes) returns x, step, flags, last_HS, last_bS and, for the tests that bound the result independently, what the solve saw:
HF_damped, bF, x0 (x before F7) and the factor."""
import numpy as np

import _hessian_ref as HR
import _linearize_ref as R

f32, f64 = np.float32, np.float64
SOLVE_KEYS = ("H_L", "b_L", "H_M", "b_M", "delta_x", "lambda", "null_basis", "null_pinv", "n_null")
OUT = ("x", "step", "flags", "last_HS", "last_bS")
LAMBDAS = (0.0, 1e-5, 0.1, 10.0)


def ldlt_solve(A_in, rhs):
    """x with A x = rhs by LDLT<Lower> with pivoting on the largest |diagonal|, operation for operation; also (L, d, transpositions)"""
    n = len(rhs)
    A = np.array(A_in, f64).reshape(n, n).copy()
    tr = list(range(n))
    all_zero = False
    for k in range(n):
        big, bigv = k, abs(A[k, k])
        for i in range(k + 1, n):
            if abs(A[i, i]) > bigv:  # false for a NaN on either side
                bigv, big = abs(A[i, i]), i
        tr[k] = big
        if k != big:  # the symmetric swap on the lower triangle
            A[k, :k], A[big, :k] = A[big, :k].copy(), A[k, :k].copy()
            A[big + 1:, k], A[big + 1:, big] = A[big + 1:, big].copy(), A[big + 1:, k].copy()
            A[k, k], A[big, big] = A[big, big], A[k, k]
            A[k + 1:big, k], A[big, k + 1:big] = A[big, k + 1:big].copy(), A[k + 1:big, k].copy()
        if k > 0:
            temp = np.diag(A)[:k] * A[k, :k]
            s = np.zeros(n - k)
            for j in range(k):  # every entry's own sum over ascending j, from 0.0
                s = s + A[k:, j] * temp[j]
            A[k:, k] = A[k:, k] - s
        akk = A[k, k]
        valid = abs(akk) > 0.0
        if k == 0 and not valid:
            all_zero = True
            break
        if valid and k + 1 < n:
            with np.errstate(all="ignore"):
                A[k + 1:, k] = A[k + 1:, k] / akk
    if all_zero:
        return np.zeros(n), (A, list(range(n)))
    y = np.array(rhs, f64).copy()
    with np.errstate(all="ignore"):
        for k in range(n):
            y[k], y[tr[k]] = y[tr[k]], y[k]
        for j in range(n):  # L^-1: y[i] -= L[i][j] y[j] over ascending j
            y[j + 1:] = y[j + 1:] - A[j + 1:, j] * y[j]
        tol = 1.0 / 1.7976931348623157e308
        for i in range(n):
            y[i] = y[i] / A[i, i] if abs(A[i, i]) > tol else 0.0
        for i in range(n - 1, -1, -1):  # L^-T: y[i] -= L[j][i] y[j] over ascending j
            for j in range(i + 1, n):
                y[i] = y[i] - A[j, i] * y[j]
        for k in range(n - 1, -1, -1):
            y[k], y[tr[k]] = y[tr[k]], y[k]
    return y, (A, tr)


def dsum_rows(M, x):
    """(M x)[i] as the double sum over ascending j from 0.0, for every row at once"""
    s = np.zeros(M.shape[0])
    for j in range(M.shape[1]):
        s = s + M[:, j] * x[j]
    return s


def system(job, hes, drop=()):
    """F1, F2: HF, bF (and H_sc); `drop`: mutations for the tests that show a bound has teeth"""
    nf = len(job["frame_ids"])
    N = 4 + 8 * nf
    get = lambda k, shape: np.asarray(job[k], f64).reshape(shape) if job.get(k) is not None else np.zeros(shape)  # noqa: E731
    HL, bL, HM, bM, dx = get("H_L", (N, N)), get("b_L", N), get("H_M", (N, N)), get("b_M", N), get("delta_x", N)
    top = bM + (0.0 if "HM_dx" in drop else dsum_rows(HM, dx))
    HF = (HL + HM) + hes["H_A"]
    bF = ((bL + top) + hes["b_A"]) + hes["b_sc"] if "b_sc_sign" in drop else ((bL + top) + hes["b_A"]) - hes["b_sc"]
    return HF, bF


def solve(job, hes, drop=()):
    """F1-F8, R1-R3 for a job whose accumulation result is `hes` (H_A, b_A, H_sc, b_sc, bd_sum, hcd_acc, hdi, JpJdF, active)"""
    nf, n = len(job["frame_ids"]), len(job["host"])
    N = 4 + 8 * nf
    HF, bF = system(job, hes, drop)
    Hsc = np.asarray(hes["H_sc"], f64)
    out = dict(last_HS=HF - Hsc, last_bS=bF.copy())
    lam1 = 1.0 + float(job.get("lambda", 0.0))
    s = 1.0 if "s" in drop else 1.0 / lam1
    HFd = HF.copy()
    HFd[np.diag_indices(N)] = np.diag(HF) * (1.0 if "damping" in drop else lam1)
    HFd = HFd - Hsc * s
    with np.errstate(all="ignore"):
        v = 1.0 / np.sqrt(np.diag(HFd) + 10.0)
        HS = (v[:, None] * HFd) * v[None, :]
        r = v * bF
        y, fac = ldlt_solve(HS, r)
        x = v * y
        x0 = x.copy()
        nn = int(job.get("n_null", 0 if job.get("null_basis") is None else np.asarray(job["null_basis"]).reshape(N, -1).shape[1]))
        if nn > 0:
            basis, pinv = np.asarray(job["null_basis"], f64).reshape(N, nn), np.asarray(job["null_pinv"], f64).reshape(nn, N)
            x = x - dsum_rows(basis, dsum_rows(pinv, x))
    flags = 0 if np.isfinite(x).all() else 1
    step = back_substitute(job, hes, x)
    if not np.isfinite(step).all():
        flags |= 2
    out.update(x=x, step=step, flags=flags, x0=x0, HF_damped=HFd, bF=bF, v=v, HS=HS, factor=fac)
    return out


def x_ad(job, x):
    """R1: nf x nf x 8 float32"""
    nf = len(job["frame_ids"])
    xF = np.asarray(x, f64).astype(f32)
    adh, adt = (np.asarray(job[k], f64).reshape(nf, nf, 8, 8).astype(f32) for k in ("ad_host", "ad_target"))
    out = np.zeros((nf, nf, 8), f32)
    with np.errstate(all="ignore"):
        for h in range(nf):
            for t in range(nf):
                if h == t:
                    continue
                a, b = np.zeros(8, f32), np.zeros(8, f32)
                for k in range(8):
                    a = a + xF[4 + 8 * h + k] * adh[h, t, k]
                    b = b + xF[4 + 8 * t + k] * adt[h, t, k]
                out[h, t] = a + b
    return out


def back_substitute(job, hes, x):
    """R1, R2: the step of every point"""
    host, point, target = (np.asarray(job[k]) for k in ("host", "point", "target"))
    n, nr = len(host), len(hes["active"])
    xF = np.asarray(x, f64).astype(f32)
    xad = x_ad(job, x)
    hcd_lin = np.asarray(job["hcd_lin"], f32).reshape(n, 4) if job.get("hcd_lin") is not None else np.zeros((n, 4), f32)
    step = np.zeros(n, f32)
    of_point = [[] for _ in range(n)]
    for r in range(nr):
        if hes["active"][r]:
            of_point[point[r]].append(r)
    with np.errstate(all="ignore"):
        for p in range(n):
            if not of_point[p]:
                continue
            Hcd = hes["hcd_acc"][p] + hcd_lin[p]
            acc = f32(0.0)
            for c in range(4):
                acc = f32(acc + f32(xF[c] * Hcd[c]))
            b = f32(hes["bd_sum"][p] - acc)
            for r in of_point[p]:
                acc = f32(0.0)
                for c in range(8):
                    acc = f32(acc + f32(xad[host[p], target[r], c] * hes["JpJdF"][r, c]))
                b = f32(b - acc)
            step[p] = -f32(b * hes["hdi"][p])
    return step


# ---- the shared scenes ------------------------------------------------------------------------------------------------------------

def make_solve_extra(job, seed, priors=True, n_null=0, lam=1e-5):
    """what a solve job holds on top of its hessian job: a positive semi-definite H_L of moderate size, optionally the prior system
    H_M, b_M with a stitched delta, and an orthonormal null basis (QR of a random matrix) with its transpose as pseudo-inverse"""
    rng = np.random.default_rng(2000 + seed)
    N = 4 + 8 * len(job["frame_ids"])
    sym = lambda M: np.tril(M) + np.tril(M, -1).T  # noqa: E731  (exactly symmetric)
    G = rng.normal(0, 3.0, (N, N))
    ex = {"H_L": sym(G @ G.T), "b_L": rng.normal(0, 30.0, N), "lambda": lam}
    if priors:
        G = rng.normal(0, 2.0, (N, 6))
        ex.update(H_M=sym(G @ G.T + np.diag(rng.uniform(0, 50, N))), b_M=rng.normal(0, 20.0, N), delta_x=rng.normal(0, 0.05, N))
    if n_null:
        Q, _ = np.linalg.qr(rng.normal(0, 1, (N, n_null)))
        ex.update(null_basis=np.ascontiguousarray(Q), null_pinv=np.ascontiguousarray(Q.T), n_null=n_null)
    return ex


NAMES = list(HR.CASES) + ["clamp", "wide", "sixteen_frames"]
_cache = {}


def case(name, priors=True, n_null=0, lam=1e-5, shift=None):
    """(job with the Hessian and the solve extras, frames, expected), computed once per variant"""
    key = (name, priors, n_null, lam, shift)
    if key not in _cache:
        job, frames, exp = HR.case(name)
        if shift is not None and int(job.get("shift_prior_to_zero", 1)) != shift:
            job = dict(job, shift_prior_to_zero=shift)
            exp = dict(exp, **HR.hessian(job, exp, job))
        job = dict(job, **make_solve_extra(job, NAMES.index(name) if name in NAMES else 50, priors, n_null, lam))
        _cache[key] = (job, frames, dict(exp, **solve(job, exp)))
    return _cache[key]


def frames_case(nf):
    """(job, frames, expected) of a window of nf frames and 40 points, for the frame counts the named scenes do not have"""
    key = ("frames", nf)
    if key not in _cache:
        job, frames = R.make_case(seed=20 + nf, n_frames=nf, n_pts=40, fix=1)
        lin = R.assemble(job, R.residuals_of(R.W, R.H, job, frames), None)
        job = dict(job, **HR.make_extra(job, seed=nf))
        exp = dict(lin, **HR.hessian(job, lin, job))
        job = dict(job, **make_solve_extra(job, 30 + nf))
        _cache[key] = (job, frames, dict(exp, **solve(job, exp)))
    return _cache[key]


def with_solve(job, exp, seed=60, **kw):
    """(job, expected) of a hessian job and its expected result (HR.case_prefix, HR.case_points) with solve extras on top"""
    job = dict(job, **make_solve_extra(job, seed, **kw))
    return job, dict(exp, **solve(job, exp))


def edge_cases():
    """name -> (job, frames, expected): arbitrary systems handed to the solver through H_L on jobs without residuals (three frames,
    N = 28, and one frame, N = 12), lambda = 0, no priors"""
    if "edges" in _cache:
        return _cache["edges"]
    out = {}
    rng = np.random.default_rng(77)

    def add(name, base, HL, bL=None, **kw):
        job, frames, exp = HR.case(base)
        N = 4 + 8 * len(job["frame_ids"])
        job = dict(job, H_L=np.asarray(HL, f64), b_L=rng.normal(0, 1, N) if bL is None else bL, **{"lambda": 0.0}, **kw)
        out[name] = (job, frames, dict(exp, **solve(job, exp)))

    N = 28
    off = rng.normal(0, 0.3, (N, N))
    off = np.tril(off, -1) + np.tril(off, -1).T
    add("equal_diagonal", "three_frames_no_residuals", off + 5.0 * np.eye(N))
    mixed = off + np.diag(np.tile([7.0, 3.0, 3.0, 7.0], 7))  # two interleaved groups of exact ties, where the swaps decide
    add("tied_groups", "three_frames_no_residuals", mixed)
    add("all_zero", "three_frames_no_residuals", np.zeros((N, N)))
    Z = np.diag(np.linspace(30.5, 3.5, N))
    Z[5:7, 5:7] = 4.0  # [[4, 4], [4, 4]] with equal scales on both rows: the second pivot of the pair is exactly zero
    add("zero_pivot", "three_frames_no_residuals", Z)
    Neg = off + 5.0 * np.eye(N)
    Neg[9, 9] = -20.0  # HF + 10 < 0: the square root gives a NaN that reaches x
    add("negative_diagonal", "three_frames_no_residuals", Neg)
    G = rng.normal(0, 1, (12, 12))
    add("twelve", "one_frame", G @ G.T + np.eye(12))
    _cache["edges"] = out
    return out


def assert_equal(got, exp, outputs=OUT + HR.STITCHED, hes_outputs=None, lin_outputs=None):
    """x, step, flags and the optional matrices bit for bit; then the accumulation's outputs as its own checker compares them.
    A NaN stands where the checker has a NaN, and that is all that is compared of it: IEEE 754 leaves the sign and the payload of the
    NaN an invalid operation returns to the implementation (sqrt of a negative number is 0xFFF8... on x86-64, 0x7FF8... on gfx950).
    Every other value, infinities and signed zeros included, is compared by its bytes."""
    for k in outputs:
        if k == "flags":
            assert int(got[k]) == int(exp[k]), (k, got[k], exp[k])
            continue
        a, b = np.asarray(got[k]), np.asarray(exp[k])
        assert a.dtype == b.dtype and a.shape == b.shape, (k, a.dtype, b.dtype, a.shape, b.shape)
        assert (np.isnan(a) == np.isnan(b)).all(), (k, np.argwhere(np.isnan(a) != np.isnan(b))[:6])
        a, b = np.where(np.isnan(a), a.dtype.type(0), a), np.where(np.isnan(b), b.dtype.type(0), b)
        ne = a.view(np.uint64 if a.dtype == f64 else np.uint32) != b.view(np.uint64 if a.dtype == f64 else np.uint32)
        assert a.tobytes() == b.tobytes(), (k, np.argwhere(ne)[:6], a[ne][:3], b[ne][:3])
    if hes_outputs is not None:
        HR.assert_equal(got, exp, outputs=hes_outputs, **({} if lin_outputs is None else dict(lin_outputs=lin_outputs)))


def invalid_jobs(job):
    """(what, job) of the calls the solve call refuses on top of the Hessian call's (a NULL H_A, ... is accepted here)"""
    def with_(key, at, value):
        a = np.array(job[key], f64, copy=True)
        a[at] = value
        return dict(job, **{key: a})

    N = 4 + 8 * len(job["frame_ids"])
    Q = np.linalg.qr(np.random.default_rng(3).normal(0, 1, (N, 2)))[0]
    nul = dict(null_basis=np.ascontiguousarray(Q), null_pinv=np.ascontiguousarray(Q.T), n_null=2)
    return [("no H_L", dict(job, H_L=None)), ("no b_L", dict(job, b_L=None)),
            ("lambda NaN", dict(job, **{"lambda": np.nan})), ("lambda inf", dict(job, **{"lambda": np.inf})),
            ("lambda -1", dict(job, **{"lambda": -1.0})), ("lambda -3", dict(job, **{"lambda": -3.0})),
            ("H_L NaN", with_("H_L", (3, 4), np.nan)), ("b_L inf", with_("b_L", 2, np.inf)), ("H_M inf", with_("H_M", (0, 0), -np.inf)),
            ("b_M NaN", with_("b_M", N - 1, np.nan)), ("delta_x NaN", with_("delta_x", 5, np.nan)),
            ("n_null -1", dict(job, n_null=-1)), ("n_null 9", dict(job, n_null=9)),
            ("n_null without a basis", dict(job, **dict(nul, null_basis=None))), ("n_null without a pseudo-inverse", dict(job, **dict(nul, null_pinv=None))),
            ("null_basis NaN", dict(job, **dict(nul, null_basis=np.where(np.arange(2 * N).reshape(N, 2) == 7, np.nan, nul["null_basis"])))),
            ("null_pinv inf", dict(job, **dict(nul, null_pinv=np.where(np.arange(2 * N).reshape(2, N) == 9, np.inf, nul["null_pinv"]))))]
