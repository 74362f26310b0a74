"""The checker of the window's nullspaces and their pseudo-inverse: Python floats (IEEE double) with
loops in the stated order, no numpy arithmetic on the path of a result.  FrontEnd::getNullspaces (dso_helpers/FrontEndOptimize.cpp:
525-574, called from solveSystem :488-494) is followed line for line; the frames' numeric nullspaces (FrameHessian::setStateZero), the
basis and its pseudo-inverse (EnergyFunctional::orthogonalize) are restated as G1, G2, G5 and G6 state them.

`nullspace(job)` records which branch of the logarithm every one of a frame's 14 logarithms took ("branches": n x 14 x 2 strings; 0-5 the
P of the pose columns, 6-11 their M, 12 and 13 the scale column's).  math.atan and math.tan are the C library's, expf is the C library's
through ctypes: G3 asks for that function, and no float32 exp of numpy is promised to be it."""
import ctypes
import ctypes.util
import math

import numpy as np

import _step_ref as T
import _window_files as W

f32, f64 = np.float32, np.float64
NP = dict(scale_xi_trans=0.5, scale_xi_rot=1.0, scale_a=10.0, scale_b=1000.0, solver_mode_delta=1e-5)
EPS_STEP = 1e-3          # G1: the central difference's step
SCALE_FAC = 1.00001      # G2
DIVISOR = 2e-3           # G1, G2
SWEEP_CAP = 30           # G6
TOL = 2.0 ** -50         # G6: rotate iff |c| > TOL sqrt(a b) and |c| > TOL (delta delta) amax
OUT = ("null_basis", "null_pinv", "sing", "rank", "flags", "frame_null", "null_x0_pre")

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.expf.restype, _libm.expf.argtypes = ctypes.c_float, [ctypes.c_float]


def expf(x):
    return f32(_libm.expf(ctypes.c_float(float(f32(x)))))


def unit_poses():
    """G1: the twelve constant poses exp(+eps e_i) (0-5) and exp(-eps e_i) (6-11)"""
    out = []
    for sign in (1.0, -1.0):
        for i in range(6):
            xi = [0.0] * 6
            xi[i] = sign * EPS_STEP
            out.append(T.se3_exp(xi))
    return out


def se3_log(pose, taken=None):
    """G1: Sophus SE3::log as section 23 restates it; the tangent [upsilon; omega]"""
    x, y, z, w = pose[:4]
    sn = (x * x + y * y) + z * z
    n = math.sqrt(sn)
    if sn < 1e-20:
        f = 2.0 / w - (2.0 * sn) / ((w * w) * w)
        b0 = "series"
    elif abs(w) < 1e-10:
        f = (math.pi if w > 0.0 else -math.pi) / n
        b0 = "pi"
    else:
        f = (2.0 * math.atan(n / w)) / n
        b0 = "atan"
    theta = f * n
    om = [f * x, f * y, f * z]
    Om = [0.0, -om[2], om[1], om[2], 0.0, -om[0], -om[1], om[0], 0.0]
    O2 = [(Om[i * 3 + 0] * Om[0 * 3 + j] + Om[i * 3 + 1] * Om[1 * 3 + j]) + Om[i * 3 + 2] * Om[2 * 3 + j] for i in range(3) for j in range(3)]
    if abs(theta) < 1e-10:
        k = 1.0 / 12.0
        b1 = "series"
    else:
        k = (1.0 - theta / (2.0 * math.tan(0.5 * theta))) / (theta * theta)
        b1 = "tan"
    if taken is not None:
        taken.append((b0, b1))
    Vi = [((1.0 if i % 4 == 0 else 0.0) - 0.5 * Om[i]) + k * O2[i] for i in range(9)]
    t = pose[4:7]
    return [(Vi[i * 3 + 0] * t[0] + Vi[i * 3 + 1] * t[1]) + Vi[i * 3 + 2] * t[2] for i in range(3)] + om


def frame_logs(Tf, units, taken=None, conj_left=False):
    """the 14 logarithms of one frame; conj_left: the mutation T^-1 exp T"""
    Ti = T.se3_inverse(Tf)
    logs = []
    for c in range(12):
        P = T.se3_mul(T.se3_mul(Ti, units[c]), Tf) if conj_left else T.se3_mul(T.se3_mul(Tf, units[c]), Ti)
        logs.append(se3_log(P, taken))
    up = list(Tf[:4]) + [Tf[4] * SCALE_FAC, Tf[5] * SCALE_FAC, Tf[6] * SCALE_FAC]
    dn = list(Tf[:4]) + [Tf[4] / SCALE_FAC, Tf[5] / SCALE_FAC, Tf[6] / SCALE_FAC]
    logs.append(se3_log(T.se3_mul(up, Ti), taken))
    logs.append(se3_log(T.se3_mul(dn, Ti), taken))
    return logs


def frame_null(Tf, units, taken=None, divisor=DIVISOR, conj_left=False):
    """G1, G2: the 6 x 7 block of one frame as 42 floats, row-major"""
    logs = frame_logs(Tf, units, taken, conj_left)
    blk = [0.0] * 42
    for i in range(7):
        P, M = (logs[i], logs[6 + i]) if i < 6 else (logs[12], logs[13])
        for r in range(6):
            blk[r * 7 + i] = (P[r] - M[r]) / divisor
    return blk


def dsum(terms):
    s = 0.0
    for t in terms:
        s += t
    return s


def round_pairs(r):
    """G6: the three disjoint pairs of round r"""
    return [tuple(sorted(((r + k) % 7, (r - k) % 7))) for k in (1, 2, 3)]


def jacobi(A, N, delta, tol=TOL):
    """G6 on the N x 7 list of rows A: (pinv 7 x N, sing, rank, capped, sweeps)"""
    W = [row[:] for row in A]
    V = [[1.0 if i == j else 0.0 for j in range(7)] for i in range(7)]
    amax = 0.0
    for k in range(7):
        s = dsum(W[i][k] * W[i][k] for i in range(N))
        if s > amax:
            amax = s
    capped, sweeps = True, 0
    for _ in range(SWEEP_CAP):
        sweeps += 1
        rotated = False
        for r in range(7):
            for p, q in round_pairs(r):
                a = dsum(W[i][p] * W[i][p] for i in range(N))
                b = dsum(W[i][q] * W[i][q] for i in range(N))
                c = dsum(W[i][p] * W[i][q] for i in range(N))
                if not (abs(c) > tol * math.sqrt(a * b) and abs(c) > (tol * (delta * delta)) * amax):
                    continue
                rotated = True
                zeta = (b - a) / (2.0 * c)
                t = (-1.0 if zeta < 0.0 else 1.0) / (abs(zeta) + math.sqrt(1.0 + zeta * zeta))
                cs = 1.0 / math.sqrt(1.0 + t * t)
                sn = cs * t
                for M, m in ((W, N), (V, 7)):
                    for i in range(m):
                        x, y = M[i][p], M[i][q]
                        M[i][p] = cs * x - sn * y
                        M[i][q] = sn * x + cs * y
        if not rotated:
            capped = False
            break
    sing = [math.sqrt(dsum(W[i][k] * W[i][k] for i in range(N))) for k in range(7)]
    smax = 0.0
    for s in sing:
        if s > smax:
            smax = s
    inv = [1.0 / s if s > delta * smax else 0.0 for s in sing]
    rank = sum(1 for s in sing if s > delta * smax)
    pinv = [[dsum((V[k][j] * inv[j]) * (W[i][j] * inv[j]) for j in range(7)) for i in range(N)] for k in range(7)]
    return pinv, sing, rank, capped, sweeps


def nullspace(job, params=None, divisor=DIVISOR, conj_left=False, no_inverse_scale=False):
    """G1-G7 for one job (a dict: world_to_cam_eval, state_zero, exposure, optional frame_null_in).  The keyword arguments are the
    mutations of the tests."""
    P = dict(NP, **(params or {}))
    ev = np.asarray(job["world_to_cam_eval"], f64).reshape(-1, 7)
    n = len(ev)
    N = 4 + 8 * n
    zero = np.asarray(job["state_zero"], f64).reshape(n, 8)
    expo = np.asarray(job["exposure"], f32).reshape(n)
    branches = []
    with np.errstate(all="ignore"):
        if job.get("frame_null_in") is not None:
            fn = [[float(x) for x in blk] for blk in np.asarray(job["frame_null_in"], f64).reshape(n, 42)]
        else:
            units = unit_poses()
            fn = []
            for f in range(n):
                taken = []
                fn.append(frame_null([float(x) for x in ev[f]], units, taken, divisor, conj_left))
                branches.append(taken)
        # G3
        aff_b = [f64(expf(f32(float(zero[f, 6]) * P["scale_a"])) * expo[f]) for f in range(n)]
        # G4: the nine N-vectors, columns pose 0-5, affA, affB, scale
        it, ir, ia, ib = 1.0 / P["scale_xi_trans"], 1.0 / P["scale_xi_rot"], 1.0 / P["scale_a"], 1.0 / P["scale_b"]
        if no_inverse_scale:
            it = ir = 1.0
        pre = [[0.0] * 9 for _ in range(N)]
        for f in range(n):
            for i in range(7):
                col = i if i < 6 else 8
                for r in range(6):
                    pre[4 + 8 * f + r][col] = fn[f][r * 7 + i] * (it if r < 3 else ir)
            pre[4 + 8 * f + 6][6] = 1.0 * ia
            pre[4 + 8 * f + 7][6] = 0.0 * ib
            pre[4 + 8 * f + 6][7] = 0.0 * ia
            pre[4 + 8 * f + 7][7] = float(aff_b[f]) * ib
        # G5
        A = [[pre[i][k if k < 6 else 8] for k in range(7)] for i in range(N)]
        flags = 0
        for k in range(7):
            s = dsum(A[i][k] * A[i][k] for i in range(N))
            if s > 0.0:
                d = math.sqrt(s)
                for i in range(N):
                    A[i][k] = A[i][k] / d
            else:
                flags |= 4
        pinv, sing, rank, capped, sweeps = jacobi(A, N, P["solver_mode_delta"])
    if capped:
        flags |= 2
    out = dict(null_basis=np.array(A, f64).reshape(N, 7), null_pinv=np.array(pinv, f64).reshape(7, N), sing=np.array(sing, f64), rank=rank,
               frame_null=np.array(fn, f64).reshape(n, 42), null_x0_pre=np.array(pre, f64).reshape(N, 9), sweeps=sweeps, branches=branches)
    if not (np.isfinite(out["null_basis"]).all() and np.isfinite(out["null_pinv"]).all() and np.isfinite(out["sing"]).all()):
        flags |= 1
    out["flags"] = flags
    return out


# ---- the analytic adjoint (independent of the stated order) ---------------------------------------------------------------------------

def adjoint_block(Tf):
    """the 6 x 7 block G1 and G2 approximate: columns 0-5 of Ad(T) = [[R, t^ R], [0, R]], then ((1.00001 - 1/1.00001) / 2e-3) [t; 0]"""
    R = np.array(T.quat_to_rot(list(Tf[:4])), f64).reshape(3, 3)
    t = np.asarray(Tf[4:7], f64)
    th = np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])
    blk = np.zeros((6, 7))
    blk[:3, :3], blk[:3, 3:6], blk[3:, 3:6] = R, th @ R, R
    blk[:3, 6] = ((SCALE_FAC - 1.0 / SCALE_FAC) / DIVISOR) * t
    return blk


def adjoint_units(blk, Tf):
    """max over the pose columns, and over the scale column, of |block - adjoint| in units of (1 + |t|) 2^-53 / 1e-3"""
    d = np.abs(np.asarray(blk, f64).reshape(6, 7) - adjoint_block(Tf))
    unit = (1.0 + float(np.linalg.norm(np.asarray(Tf[4:7], f64)))) * 2.0 ** -53 / 1e-3
    return float(d[:, :6].max() / unit), float(d[:, 6].max() / unit)


# ---- the shared scenes ----------------------------------------------------------------------------------------------------------------

def make_job(seed, n, rot=1.5, trans=100.0, origin_first=False):
    """n frames with rotations up to `rot` rad about random axes, translations up to about `trans`, a in state_zero, exposures"""
    rng = np.random.default_rng(9000 + seed)
    ev = np.zeros((n, 7))
    for f in range(n):
        axis = rng.normal(0, 1, 3)
        axis /= np.linalg.norm(axis)
        ev[f, :4] = T._rot_quat(axis * rng.uniform(0.0, rot))
        ev[f, 4:] = rng.normal(0, 1, 3) * rng.choice([0.01, 1.0, trans / 2.0])
    if origin_first:
        ev[0] = [0, 0, 0, 1, 0, 0, 0]
    zero = np.zeros((n, 8))
    zero[:, 6] = rng.normal(0, 0.02, n)
    zero[:, 7] = rng.normal(0, 0.002, n)
    return dict(world_to_cam_eval=ev, state_zero=zero, exposure=rng.uniform(0.5, 2.0, n).astype(f32))


FRAME_COUNTS = (1, 2, 3, 7, 8, 9, 15, 16)
_cache = {}


def scene(name):
    """the named job, computed once.  "frames_<n>": n frames; "origin_one": one frame at the origin (the scale column is zero);
    "origin_first": two frames, the first at the origin; "equal_columns": three frames with a frame_null_in whose columns 1 and 4 are
    equal in every frame; "given_<n>": frames_<n> with the checker's own frame_null as frame_null_in"""
    if name in _cache:
        return _cache[name]
    if name.startswith("frames_"):
        n = int(name[7:])
        job = make_job(n, n)
    elif name == "origin_one":
        job = make_job(40, 1, origin_first=True)
    elif name == "origin_first":
        job = make_job(41, 2, origin_first=True)
    elif name == "equal_columns":
        job = make_job(42, 3)
        fn = expected("frames_3")["frame_null"].reshape(3, 6, 7).copy()
        fn[:, :, 4] = fn[:, :, 1]
        job = dict(job, frame_null_in=fn.reshape(3, 42))
    elif name.startswith("given_"):
        base = name[6:]
        job = dict(scene(base), frame_null_in=expected(base)["frame_null"].copy())
    else:
        raise KeyError(name)
    _cache[name] = job
    return job


def expected(name):
    key = ("exp", name)
    if key not in _cache:
        _cache[key] = nullspace(scene(name))
    return _cache[key]


POSE_SCENES = tuple(f"frames_{n}" for n in FRAME_COUNTS) + ("origin_one", "origin_first")
GIVEN_SCENES = tuple(f"given_frames_{n}" for n in FRAME_COUNTS) + ("given_origin_one", "given_origin_first", "equal_columns")


# ---- for tools/nullspace_host_standalone.cpp ---------------------------------------------------------------------------------------

def write_case(path, job):
    """the stand-alone program's file (tests/_window_files.py)"""
    W.write_nullspace_job(path, job)


def hashes(exp):
    """what tools/nullspace_host_standalone.cpp prints, from a checker result"""
    out = {k: f"{W.fnv1a(np.ascontiguousarray(exp[k], np.float64).tobytes()):016x}" for k in ("null_basis", "null_pinv", "sing", "frame_null", "null_x0_pre")}
    out.update(rank=exp["rank"], flags=exp["flags"], forms_equal=1, refusal=1)
    return out


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_equal(got, exp, outputs=OUT):
    """every named output bit for bit (rank and flags as integers)"""
    for k in outputs:
        if k in ("rank", "flags"):
            assert int(got[k]) == int(exp[k]), (k, got[k], exp[k])
            continue
        a, b = np.asarray(got[k], f64), np.asarray(exp[k], f64).reshape(np.asarray(got[k]).shape)
        ne = a.view(np.uint64) != b.view(np.uint64)
        assert not ne.any(), (k, np.argwhere(ne)[:6], a[ne][:3], b[ne][:3])


def invalid_jobs(job):
    """(what, job, params) of the calls V refuses"""
    def with_(key, at, value, dtype=f64):
        a = np.array(job[key], dtype, copy=True)
        a[at] = value
        return dict(job, **{key: a})

    n = len(np.asarray(job["world_to_cam_eval"]).reshape(-1, 7))
    fn = np.zeros((n, 42))
    fn[0, 5] = np.nan
    out = [("no world_to_cam_eval", dict(job, world_to_cam_eval=None), None), ("no state_zero", dict(job, state_zero=None), None),
           ("no exposure", dict(job, exposure=None), None), ("no null_basis", dict(job, drop="null_basis"), None),
           ("no null_pinv", dict(job, drop="null_pinv"), None), ("no sing", dict(job, drop="sing"), None),
           ("no rank", dict(job, drop="rank"), None), ("no flags", dict(job, drop="flags"), None),
           ("n_frames 0", dict(job, n_frames=0), None), ("n_frames 17", dict(job, n_frames=17), None),
           ("quaternion not unit", with_("world_to_cam_eval", (0, 3), job["world_to_cam_eval"][0][3] + 1e-6), None),
           ("pose NaN", with_("world_to_cam_eval", (n - 1, 5), np.nan), None), ("pose inf", with_("world_to_cam_eval", (0, 4), np.inf), None),
           ("state_zero NaN", with_("state_zero", (0, 6), np.nan), None), ("exposure NaN", with_("exposure", n - 1, np.nan, f32), None),
           ("exposure 0", with_("exposure", 0, 0.0, f32), None), ("exposure negative", with_("exposure", 0, -1.0, f32), None),
           ("frame_null_in NaN", dict(job, frame_null_in=fn), None)]
    for k in NP:
        for what, v in (("0", 0.0), ("negative", -1.0), ("NaN", float("nan")), ("inf", float("inf"))):
            out.append((f"{k} {what}", job, {k: v}))
    return out
