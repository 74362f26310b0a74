"""Independent checker of the step of the window optimisation: the rules D1-D4, Q1-Q4 and E1-E3 as the project
states them, then the checkers of sections 16-18 (tests/_linearize_ref.py, _hessian_ref.py, _solve_ref.py; imported, not edited) on the
job completed with what the rules formed.  Doubles are Python floats (IEEE binary64, one rounding per operation, in the order
written), floats are numpy float32 scalars, sums are loops in the stated order.  sin, cos and exp are the C library's (math.*).

step(job, sp) returns every output of D1-E3; `W` and `aff_a` override D2's world_to_cam and the float of Q4's exponential factor, so
that a comparison against a device whose sincos and exp differ in the last places can start from the device's own values.
run(job, frames, ...) adds the outputs of sections 16-18 at the trial state."""
import math

import numpy as np

import _hessian_ref as HR
import _linearize_ref as R
import _solve_ref as SR
import _window_files as W

f32, f64 = np.float32, np.float64
SP = dict(scale_xi_trans=0.5, scale_xi_rot=1.0, scale_a=10.0, scale_b=1000.0, th_opt_iterations=1.2)
STEP_IN = ("world_to_cam_eval", "state_zero", "state_backup", "frame_step", "calib_zero", "calib_backup", "calib_step", "idepth_backup",
           "idepth_step", "exposure", "stepfac", "state_prior", "state_prior_zero")
PRE = tuple(k for k, _ in R.PRE)
STEP_OUT = ("state", "calib", "idepth", "world_to_cam", "cam_to_world", "can_break", "step_sums", "energy_m", "cam") + PRE + ("delta_x", "H_L", "b_L")
FORMED = PRE + ("idepth_scaled", "idepth_zero_scaled", "delta", "delta_x")


# ---- quaternions and SE3 on Python floats: {qx, qy, qz, qw, tx, ty, tz} -------------------------------------------------------------

def quat_normalize(q):
    n = math.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    return [q[0] / n, q[1] / n, q[2] / n, q[3] / n]


def quat_to_rot(q):
    x, y, z, w = q[:4]
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [1.0 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1.0 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1.0 - (txx + tyy)]


def quat_mul(a, b):
    ax, ay, az, aw = a[:4]
    bx, by, bz, bw = b[:4]
    return [aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx,
            aw * bw - ax * bx - ay * by - az * bz]


def quat_rotate(q, v):
    uv = [q[1] * v[2] - q[2] * v[1], q[2] * v[0] - q[0] * v[2], q[0] * v[1] - q[1] * v[0]]
    uv = [u + u for u in uv]
    c = [q[1] * uv[2] - q[2] * uv[1], q[2] * uv[0] - q[0] * uv[2], q[0] * uv[1] - q[1] * uv[0]]
    return [v[i] + q[3] * uv[i] + c[i] for i in range(3)]


def se3_mul(a, b):
    r = quat_rotate(a, b[4:7])
    q = quat_normalize(quat_mul(a, b))
    return q + [a[4] + r[0], a[5] + r[1], a[6] + r[2]]


def se3_inverse(a):
    qc = [-a[0], -a[1], -a[2], a[3]]
    r = quat_rotate(qc, a[4:7])
    return qc + [-r[0], -r[1], -r[2]]


def se3_exp(xi, taken=None):
    """Sophus SE3::exp of [upsilon; omega]; taken: a set that collects "series" / "general" """
    ups, om = xi[:3], xi[3:6]
    theta_sq = om[0] * om[0] + om[1] * om[1] + om[2] * om[2]
    theta = math.sqrt(theta_sq)
    half = 0.5 * theta
    small = theta < 1e-10
    if taken is not None:
        taken.add("series" if small else "general")
    if small:
        t2 = theta * theta
        t4 = t2 * t2
        imag = 0.5 - (1.0 / 48.0) * t2 + (1.0 / 3840.0) * t4
        real = 1.0 - 0.5 * t2 + (1.0 / 384.0) * t4
    else:
        imag = math.sin(half) / theta
        real = math.cos(half)
    q = quat_normalize([imag * om[0], imag * om[1], imag * om[2], real])
    if small:
        V = quat_to_rot(q)
    else:
        Om = [0.0, -om[2], om[1], om[2], 0.0, -om[0], -om[1], om[0], 0.0]
        O2 = [Om[i * 3 + 0] * Om[0 * 3 + j] + Om[i * 3 + 1] * Om[1 * 3 + j] + Om[i * 3 + 2] * Om[2 * 3 + j] for i in range(3) for j in range(3)]
        ca = (1.0 - math.cos(theta)) / theta_sq
        cb = (theta - math.sin(theta)) / (theta_sq * theta)
        V = [(1.0 if i % 4 == 0 else 0.0) + ca * Om[i] + cb * O2[i] for i in range(9)]
    return q + [V[i * 3 + 0] * ups[0] + V[i * 3 + 1] * ups[1] + V[i * 3 + 2] * ups[2] for i in range(3)]


def mat3f_mul(a, b):
    return [f32(f32(f32(a[i * 3 + 0] * b[0 * 3 + j]) + f32(a[i * 3 + 1] * b[1 * 3 + j])) + f32(a[i * 3 + 2] * b[2 * 3 + j])) for i in range(3) for j in range(3)]


def aff_exp(aff_h, aff_t):
    return math.exp(aff_t[0] - aff_h[0])


# ---- the rules ----------------------------------------------------------------------------------------------------------------------

def factor_of(stepfac, k):
    return float(stepfac[1] if k < 3 else stepfac[2] if k < 6 else stepfac[3])


def pair_row(eval_t, eval_inv_h, W_t, C_h, cam, exp_h, exp_t, aff_h, aff_t, zero_b_h, scale_b, aff_a=None, exp_fn=aff_exp, left=True):
    """Q1-Q4 of one pair.  left=False: a mutation for the group-structure test (C_h W_t instead of W_t C_h)"""
    L0 = se3_mul(eval_t, eval_inv_h)
    L = se3_mul(W_t, C_h) if left else se3_mul(C_h, W_t)
    o = dict(pre_RTll_0=[f32(x) for x in quat_to_rot(L0)], pre_tTll_0=[f32(x) for x in L0[4:7]])
    Rf, tf = [f32(x) for x in quat_to_rot(L)], [f32(x) for x in L[4:7]]
    fx, fy, cx, cy, fxi, fyi = cam
    z, one = f32(0.0), f32(1.0)
    K = [fx, z, cx, z, fy, cy, z, z, one]
    Ki = [fxi, z, f32(-cx * fxi), z, fyi, f32(-cy * fyi), z, z, one]
    o["pre_KRKiTll"] = mat3f_mul(mat3f_mul(K, Rf), Ki)
    o["pre_KtTll"] = [f32(f32(f32(K[i * 3] * tf[0]) + f32(K[i * 3 + 1] * tf[1])) + f32(K[i * 3 + 2] * tf[2])) for i in range(3)]
    eh, et = f32(exp_h), f32(exp_t)
    if eh == 0 or et == 0:
        eh = et = f32(1.0)
    a = exp_fn(aff_h, aff_t) * float(et) / float(eh)
    o["pre_aff_mode"] = [f32(a) if aff_a is None else f32(aff_a), f32(aff_t[1] - a * aff_h[1])]
    o["pre_b0_mode"] = [f32(zero_b_h * scale_b)]
    o["L"], o["L0"], o["a"] = L, L0, a
    return o


def step(job, sp=None, params=None, W=None, aff_a=None, taken=None, exp_fn=aff_exp):
    """D1-D4, Q1-Q4, E1-E3.  W (n x 7) and aff_a (n x n) replace D2's world_to_cam and the float of Q4's a; taken collects se3_exp's branches"""
    sp = dict(SP, **(sp or {}))
    P = dict(R.PARAMS, **(params or {}))
    n = len(job["frame_ids"])
    N = 4 + 8 * n
    d = lambda k, shape: np.asarray(job[k], f64).reshape(shape)  # noqa: E731
    ev, zero, backup, fstep = d("world_to_cam_eval", (n, 7)), d("state_zero", (n, 8)), d("state_backup", (n, 8)), d("frame_step", (n, 8))
    czero, cbackup, cstep = d("calib_zero", 4), d("calib_backup", 4), d("calib_step", 4)
    idb, ids = np.asarray(job["idepth_backup"], f32).reshape(-1), np.asarray(job["idepth_step"], f32).reshape(-1)
    expo, fac = np.asarray(job["exposure"], f32), np.asarray(job["stepfac"], f32)
    scale = [sp["scale_xi_trans"]] * 3 + [sp["scale_xi_rot"]] * 3 + [sp["scale_a"], sp["scale_b"]]
    out = {}
    with np.errstate(all="ignore"):
        # D1
        value = [float(cbackup[c]) + float(fac[0]) * float(cstep[c]) for c in range(4)]
        cam = [f32(float(f32(P["scale_f"] if c < 2 else P["scale_c"])) * value[c]) for c in range(4)]
        cam += [f32(f32(1.0) / cam[0]), f32(f32(1.0) / cam[1])]
        c_delta = [f32(value[c] - float(czero[c])) for c in range(4)]
        # D2
        state = [[float(backup[f, k]) + factor_of(fac, k) * float(fstep[f, k]) for k in range(8)] for f in range(n)]
        scaled = [[state[f][k] * scale[k] for k in range(8)] for f in range(n)]
        Wc = [se3_mul(se3_exp(scaled[f][:6], taken), [float(x) for x in ev[f]]) for f in range(n)]
        if W is not None:
            Wc = [[float(x) for x in row] for row in np.asarray(W, f64).reshape(n, 7)]
        Cw = [se3_inverse(w) for w in Wc]
        Ei = [se3_inverse([float(x) for x in ev[f]]) for f in range(n)]
        delta_f = [[state[f][k] - float(zero[f, k]) for k in range(8)] for f in range(n)]
        aff = [scaled[f][6:8] for f in range(n)]
        # D3
        idepth = (idb + fac[4] * ids).astype(f32)
        scaled_id = (f32(P["scale_idepth"]) * idepth).astype(f32)
        # D4
        sA = sB = sT = sR = f32(0.0)
        for f in range(n):
            s = [float(x) for x in fstep[f]]
            sA = f32(float(sA) + s[6] * s[6])
            sB = f32(float(sB) + s[7] * s[7])
            sT = f32(float(sT) + ((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]))
            sR = f32(float(sR) + ((s[3] * s[3] + s[4] * s[4]) + s[5] * s[5]))
        sID = sNID = num = f32(0.0)
        for p in range(len(idb)):
            sID = f32(sID + f32(ids[p] * ids[p]))
            sNID = f32(sNID + np.abs(idb[p]))
            num = f32(num + f32(1.0))
        nf_ = f32(n)
        sums = np.array([sA / nf_, sB / nf_, sR / nf_, sT / nf_, sID / num, sNID / num], f32)
        th = sp["th_opt_iterations"]
        tests = [float(np.sqrt(sums[0])) < 0.0005 * th, float(np.sqrt(sums[1])) < 0.00005 * th, float(np.sqrt(sums[2])) < 0.00005 * th,
                 float(f32(np.sqrt(sums[3]) * sums[5])) < 0.00005 * th]
        out.update(step_sums=sums, can_break=int(all(tests)), break_tests=tests)
        # Q1-Q4
        pre = {k: np.zeros((n, n, m), f32) for k, m in R.PRE}
        Ls = {}
        for h in range(n):
            for t in range(n):
                if h == t:
                    continue
                o = pair_row([float(x) for x in ev[t]], Ei[h], Wc[t], Cw[h], cam, expo[h], expo[t], aff[h], aff[t], float(zero[h, 7]), sp["scale_b"],
                             None if aff_a is None else np.asarray(aff_a, f32).reshape(n, n)[h, t], exp_fn)
                for k in PRE:
                    pre[k][h, t] = o[k]
                Ls[h, t] = (o["L"], o["L0"], o["a"])
        # E1-E3
        dx = [float(c) for c in c_delta] + [x for f in range(n) for x in delta_f[f]]
        HM = np.asarray(job["H_M"], f64).reshape(N, N) if job.get("H_M") is not None else None
        bM = np.asarray(job["b_M"], f64).reshape(N) if job.get("b_M") is not None else None
        em = 0.0
        for i in range(N):
            s = 0.0
            for j in range(N):
                s += (float(HM[i, j]) if HM is not None else 0.0) * dx[j]
            em += dx[i] * (2.0 * (float(bM[i]) if bM is not None else 0.0) + s)
        HL, bL = np.array(job["H_L"], f64).reshape(N, N).copy(), np.array(job["b_L"], f64).reshape(N).copy()
        if job.get("state_prior") is not None:
            pr, pz = np.asarray(job["state_prior"], f64), np.asarray(job["state_prior_zero"], f64)
            flat = [x for f in range(n) for x in state[f]]
            for i in range(N):
                dp = float(c_delta[i]) if i < 4 else flat[i - 4] - float(pz[i])
                HL[i, i] = float(HL[i, i]) + float(pr[i])
                bL[i] = float(bL[i]) + float(pr[i]) * dp
    out.update(state=np.array(state, f64).reshape(n, 8), calib=np.array(value, f64), idepth=idepth, idepth_scaled=scaled_id,
               world_to_cam=np.array(Wc, f64).reshape(n, 7), cam_to_world=np.array(Cw, f64).reshape(n, 7), energy_m=f64(em),
               cam=np.array(cam, f32), delta_x=np.array(dx, f64), H_L=HL, b_L=bL, c_delta=np.array(c_delta, f32), pairs=Ls, scaled=scaled, **pre)
    return out


def complete(job, st):
    """the solve job of sections 16-18 at the trial state: what a caller of dsm_window_solve_batch would pass"""
    c = {k: v for k, v in job.items() if k not in STEP_IN}
    c.update({k: st[k] for k in PRE})
    c.update(cam=tuple(st["cam"][:4]), cam_inv=tuple(st["cam"][4:]), idepth_scaled=st["idepth_scaled"], idepth_zero_scaled=st["idepth_scaled"],
             delta=None, delta_x=st["delta_x"], H_L=st["H_L"], b_L=st["b_L"])
    return c


def downstream(cjob, frames, w=R.W, h=R.H, params=None):
    """sections 16-18 on a completed job: the linearisation's, the accumulation's and the solve's results in one dict"""
    lin = R.linearize(w, h, cjob, frames, params)
    hes = dict(lin, **HR.hessian(cjob, lin, cjob))
    return dict(hes, **SR.solve(cjob, hes))


def run(job, frames, sp=None, params=None, W=None, aff_a=None):
    st = step(job, sp, params, W, aff_a)
    return dict(downstream(complete(job, st), frames, params=params), **{k: st[k] for k in STEP_OUT}, break_tests=st["break_tests"])


# ---- the shared scenes: everything from poses ----------------------------------------------------------------------------------------

def _rot_quat(v):
    v = np.asarray(v, f64)
    th = float(np.linalg.norm(v))
    if th == 0.0:
        return [0.0, 0.0, 0.0, 1.0]
    s = math.sin(th / 2) / th
    return quat_normalize([s * v[0], s * v[1], s * v[2], math.cos(th / 2)])


def make_scene(seed=1, n_frames=5, n_pts=110, fix=1, priors=True, h_m=True, stepfac=(1.0, 1.0, 1.0, 1.0, 1.0), frame_step_scale=1.0, lam=1e-5,
               n_null=0, residuals=True):
    """A step job on _linearize_ref.make_case's window (its plane, textures, NaN texels, constant patch, brightened frame, points and
    residuals), with the precalc tables replaced by what they derive from.  make_case puts frame k's camera at world_to_cam
    translation c_k = (+-0.08 k, 0, 0.002 k) without rotation; here world_to_cam_eval is that pose with a rotation of about 2e-3 and a
    translation error of about 2e-3, state_zero has no pose part and an affine part (b of frame 3 answers its brightening by 60),
    state_backup lies a small way off it, and the step has rotation about 1e-3, translation about 1e-2, a about 1e-3, b about 1e-5
    (unscaled) and depth +-5 %.  Frame 0 has no pose state and no pose step, so its se3_exp takes the series branch.  Frame 2 (or the
    last) has exposure 0.  Priors: 1e12 on frame 0's pose and on every a, 1e8 on every b, 5e9 on the calibration.
    Returns (job without "window", frames)."""
    base, frames = R.make_case(seed=seed, n_frames=n_frames, n_pts=n_pts, fix=fix)
    if not residuals:
        base = R.prefix(base, 0)
    rng = np.random.default_rng(5000 + seed)
    n, N = n_frames, 4 + 8 * n_frames
    cams = [np.zeros(3)] + [np.array([0.08 * k * (1 if (k - 1) % 2 == 0 else -1), 0.0, 0.002 * k]) for k in range(1, n)]
    job = {k: v for k, v in base.items() if k not in FORMED + ("cam", "cam_inv")}
    job.update(HR.make_extra(base, seed=seed))
    job["delta"] = None  # (the points' float "prior" of the hessian job stays; the N priors of E3 are "state_prior")
    ev = np.zeros((n, 7))
    for f in range(n):
        ev[f, :4] = _rot_quat(rng.normal(0, 0.002, 3) if f else np.zeros(3))
        ev[f, 4:] = cams[f] + (rng.normal(0, 1, 3) * (0.002, 0.002, 0.0002) if f else 0.0)
    zero = np.zeros((n, 8))
    zero[:, 6] = rng.normal(0, 0.002, n)
    zero[:, 7] = rng.normal(0, 0.002, n)
    if n > 3:
        zero[3, 7] = 0.06
    backup = zero.copy()
    backup[1:, :3] += rng.normal(0, 2e-3, (n - 1, 3))
    backup[1:, 3:6] += rng.normal(0, 1e-3, (n - 1, 3))
    backup[:, 6] += rng.normal(0, 1e-3, n)
    backup[:, 7] += rng.normal(0, 1e-5, n)
    fstep = np.zeros((n, 8))
    fstep[1:, :3] = rng.normal(0, 1e-2, (n - 1, 3))
    fstep[1:, 3:6] = rng.normal(0, 1e-3, (n - 1, 3))
    fstep[:, 6], fstep[:, 7] = rng.normal(0, 1e-3, n), rng.normal(0, 1e-5, n)
    fstep *= frame_step_scale
    cam = np.array([float(x) for x in base["cam"]])
    czero = cam / 50.0
    cbackup = czero + rng.normal(0, 1e-5, 4)
    cstep = rng.normal(0, 1e-5, 4)
    idb = np.asarray(base["idepth_scaled"], f32).copy()
    ids = (idb * rng.uniform(-0.05, 0.05, len(idb))).astype(f32)
    expo = rng.uniform(0.8, 1.25, n).astype(f32)
    expo[min(2, n - 1)] = 0.0
    job.update(world_to_cam_eval=ev, state_zero=zero, state_backup=backup, frame_step=fstep, calib_zero=czero, calib_backup=cbackup, calib_step=cstep,
               idepth_backup=idb, idepth_step=ids, exposure=expo, stepfac=np.array(stepfac, f32))
    ex = SR.make_solve_extra(base, 70 + seed, priors=h_m, n_null=n_null, lam=lam)
    ex.pop("delta_x", None)
    job.update(ex)
    if priors:
        pr = np.zeros(N)
        pr[:4] = 5e9
        pr[4:10] = 1e12
        pr[10::8], pr[11::8] = 1e12, 1e8
        pz = np.concatenate([czero, rng.normal(0, 1e-4, 8 * n)])
        job.update(state_prior=pr, state_prior_zero=pz)
    else:
        job.update(state_prior=None, state_prior_zero=None)
    return job, frames


SCENES = {
    "scene": dict(seed=1, n_frames=5, n_pts=110),
    "nine_frames": dict(seed=2, n_frames=9, n_pts=60),
    "one_frame": dict(seed=3, n_frames=1, n_pts=6),
    "two_frames": dict(seed=5, n_frames=2, n_pts=40),
    "three_frames": dict(seed=4, n_frames=3, n_pts=30),
    "three_frames_no_residuals": dict(seed=4, n_frames=3, n_pts=12, residuals=False),
    "no_points": dict(seed=6, n_frames=4, n_pts=0),
    "fifteen_frames": dict(seed=7, n_frames=15, n_pts=30),
    "sixteen_frames": dict(seed=8, n_frames=16, n_pts=30),
    "no_priors": dict(seed=1, n_frames=5, n_pts=40, priors=False),
    "no_h_m": dict(seed=1, n_frames=5, n_pts=40, h_m=False),
    "zero_step": dict(seed=1, n_frames=5, n_pts=110, stepfac=(0.0, 0.0, 0.0, 0.0, 0.0)),
    "lambda_10": dict(seed=9, n_frames=3, n_pts=30, lam=10.0),
    "null_2": dict(seed=9, n_frames=3, n_pts=30, n_null=2),
}
_cache = {}


def scene(name, **kw):
    """(job, frames), computed once; kw: make_scene arguments on top of the named scene's"""
    key = (name, tuple(sorted(kw.items())))
    if key not in _cache:
        _cache[key] = make_scene(**dict(SCENES[name], **kw))
    return _cache[key]


def expected(name, **kw):
    """(job, frames, the checker's result), computed once"""
    key = ("exp", name, tuple(sorted(kw.items())))
    if key not in _cache:
        job, frames = scene(name, **kw)
        _cache[key] = (job, frames, run(job, frames))
    return _cache[key]


def break_jobs():
    """name -> job (two frames, 40 points): can_break 1, and 0 because of each comparison alone.  The thresholds are 0.0005 th for
    sqrt(sumA) and 0.00005 th for the other three, th = 1.2; every step entry is a tenth of its threshold except the one that decides,
    which is twice it."""
    job, _ = scene("two_frames")
    out = {}
    idb = np.asarray(job["idepth_backup"], f32)
    for which in ("break", "A", "B", "R", "T"):
        s = np.zeros((2, 8))
        s[:, 6] = 0.0006 * (2.0 if which == "A" else 0.1)
        s[:, 7] = 0.00006 * (2.0 if which == "B" else 0.1)
        s[:, 3] = 0.00006 * (2.0 if which == "R" else 0.1)
        s[:, 0] = 0.00006 / float(np.mean(np.abs(idb))) * (2.0 if which == "T" else 0.1)
        out[which] = dict(job, frame_step=s)
    return out


def assert_step_equal(got, exp, outputs=STEP_OUT):
    """the outputs of D1-E3 bit for bit; a NaN is compared as a NaN (numID == 0 gives 0 / 0)"""
    for k in outputs:
        if k == "can_break":
            assert int(got[k]) == int(exp[k]), (k, got[k], exp[k])
            continue
        a, b = np.asarray(got[k]), np.asarray(exp[k])
        assert a.dtype == b.dtype, (k, a.dtype, b.dtype)
        a, b = a.reshape(-1), b.reshape(-1)
        assert a.shape == b.shape, (k, a.shape, b.shape)
        assert (np.isnan(a) == np.isnan(b)).all(), (k, "NaN pattern")
        a, b = np.where(np.isnan(a), a.dtype.type(0), a), np.where(np.isnan(b), b.dtype.type(0), b)
        view = np.uint64 if a.dtype == f64 else np.uint32
        ne = a.view(view) != b.view(view)
        assert not ne.any(), (k, np.argwhere(ne)[:6].ravel(), a[ne][:3], b[ne][:3])


def invalid_jobs(job):
    """(what, job) of the calls the step call refuses on top of the solve call's"""
    n = len(job["frame_ids"])

    def with_(key, at, value, dtype=f64):
        a = np.array(job[key], dtype, copy=True)
        a.reshape(-1)[at] = value
        return dict(job, **{key: a})

    q = np.array(job["world_to_cam_eval"], f64, copy=True)
    q[0, :4] *= 1.0 + 1e-6
    zeros = lambda k, m: np.zeros((n, n, m), f32)  # noqa: E731
    bad = [(f"{k} given", dict(job, **{k: zeros(k, m)})) for k, m in R.PRE]
    np_ = len(job["host"])
    bad += [("idepth_scaled given", dict(job, idepth_scaled=np.zeros(np_, f32))), ("idepth_zero_scaled given", dict(job, idepth_zero_scaled=np.zeros(np_, f32))),
            ("delta given", dict(job, delta=np.zeros(np_, f32))), ("delta_x given", dict(job, delta_x=np.zeros(4 + 8 * n)))]
    bad += [(f"no {k}", dict(job, **{k: None})) for k in STEP_IN[:10]]
    bad += [("state_prior without its zero", dict(job, state_prior_zero=None)), ("state_prior_zero without prior", dict(job, state_prior=None)),
            ("eval NaN", with_("world_to_cam_eval", 5, np.nan)), ("state_zero inf", with_("state_zero", 3, np.inf)),
            ("state_backup NaN", with_("state_backup", 8 * n - 1, np.nan)), ("frame_step NaN", with_("frame_step", 0, np.nan)),
            ("calib_zero NaN", with_("calib_zero", 1, np.nan)), ("calib_backup inf", with_("calib_backup", 2, np.inf)),
            ("calib_step NaN", with_("calib_step", 3, np.nan)), ("idepth_backup NaN", with_("idepth_backup", 0, np.nan, f32)),
            ("idepth_step inf", with_("idepth_step", np_ - 1, np.inf, f32)), ("exposure NaN", with_("exposure", 0, np.nan, f32)),
            ("stepfac NaN", with_("stepfac", 2, np.nan, f32)), ("stepfac inf", with_("stepfac", 4, np.inf, f32)),
            ("state_prior NaN", with_("state_prior", 4, np.nan)), ("state_prior_zero inf", with_("state_prior_zero", 0, np.inf)),
            ("quaternion not unit", dict(job, world_to_cam_eval=q)),
            ("no H_L", dict(job, H_L=None)), ("lambda NaN", dict(job, **{"lambda": np.nan})), ("H_M NaN", with_("H_M", 7, np.nan))]
    return bad


# ---- for tools/step_host_standalone.cpp ----------------------------------------------------------------------------------------------

def write_case(path, w, h, job, frames):
    """the step file (tests/_window_files.py)"""
    W.write_step(path, w, h, job, frames)


def hashes(exp):
    """what tools/step_host_standalone.cpp prints, from a checker result"""
    hx = lambda a: f"{W.fnv1a(np.ascontiguousarray(a).tobytes()):016x}"  # noqa: E731
    pre = 0
    for k in PRE:
        pre ^= W.fnv1a(np.ascontiguousarray(exp[k]).tobytes())
    out = {k: hx(exp[k]) for k in ("state", "calib", "idepth", "world_to_cam", "cam_to_world", "cam", "delta_x", "H_L", "b_L", "x", "step", "new_energy")}
    out.update(pre=f"{pre:016x}", energy_m=hx(np.array([exp["energy_m"]], f64)), can_break=int(exp["can_break"]), flags=int(exp["flags"]),
               n_res=len(exp["new_energy"]), lean_equal=1)
    return out
