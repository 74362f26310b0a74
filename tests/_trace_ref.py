"""Independent checker of the tracing of immature points: ImmaturePoint::traceOn as the rules T1-T16 state it,
one point at a time in numpy float32 (every operation rounds to float32; the eight pattern pixels, and the steps of the search, are
array elements, their sums are chains of float32 additions in pattern order).  Written from the rules, not from the C code.

trace(w, h, target, job, **params) returns the state after the call (status, idepth_min, idepth_max, quality, trace_uv,
trace_interval), steps, counts, `branches`: per branch name the number of points that took it, and `point_branches`: per point the
set of its branches.  make_scene / case build the seeded
160 x 64 scene the tests share, make_scene_at / geometry_case the same kinds of points at any geometry, with points on either side of
T2's bound next to all four sides; a case is computed once per process."""
import numpy as np

f32 = np.float32
GOOD, OOB, OUTLIER, SKIPPED, BADCONDITION, UNINITIALIZED = range(6)
PATTERN = [(0, -2), (-1, -1), (1, -1), (-2, 0), (0, 0), (2, 0), (-1, 1), (0, 2)]
DEFAULTS = dict(max_pix_search=0.027, slack_interval=1.5, stepsize=1.0, min_improvement=2.0, min_test_radius=2, gn_iterations=3,
                gn_threshold=0.1, extra_slack_on_th=1.2, huber_th=9.0)
BRANCHES = ("T1", "T2_oob", "T3_oob", "T3_skipped", "T4_taken", "T4_oob", "T5_oob", "T6_badcondition", "T6_clamp", "T7_dist_above_maxpix",
            "T7_cap", "T7_oob", "T8_guard_search", "T8_guard_gn", "nan_texel", "T10_steps_above_10", "T10_short_quality_lowered",
            "T10_short_quality_kept", "best_at_step_0", "best_at_last_step", "T11_reject", "T11_accept", "T11_clamp", "T11_break",
            "T12_outlier", "T12_outlier_to_oob", "T13_u_form", "T13_v_form", "T13_swap", "T14", "T15")
REQUIRED = tuple(b for b in BRANCHES if b != "T7_oob")  # what the scene must reach (T7's exit needs dist = 0 and a slack <= 0)
STATE = ("status", "idepth_min", "idepth_max", "quality", "trace_uv", "trace_interval")


def _inside(u, v, w, h):
    return bool(u > f32(4) and v > f32(4) and u < f32(w - 5) and v < f32(h - 5))


def _gfix(a):
    return np.where(np.isfinite(a), a, f32(0.0)).astype(f32)


def _sample(I, w, h, x, y, gradients):
    """U6 at the float32 arrays (x, y) under the guard T8: (guard passed, intensity, gx, gy); entries that fail the guard are unread"""
    ok = (x >= f32(1)) & (y >= f32(1)) & (x < f32(w - 2)) & (y < f32(h - 2))
    xs, ys = np.where(ok, x, f32(1)), np.where(ok, y, f32(1))
    ix, iy = xs.astype(np.int64), ys.astype(np.int64)
    dx, dy = (xs - ix.astype(f32)).astype(f32), (ys - iy.astype(f32)).astype(f32)
    dxdy = dx * dy
    w11, w01, w10 = dxdy, dy - dxdy, dx - dxdy
    w00 = ((f32(1.0) - dx) - dy) + dxdy

    def mix(t):  # t(ox, oy): the texel channel at (ix + ox, iy + oy)
        return ((w11 * t(1, 1) + w01 * t(0, 1)) + w10 * t(1, 0)) + w00 * t(0, 0)

    val = mix(lambda ox, oy: I[iy + oy, ix + ox])
    if not gradients:
        return ok, val, None, None
    gx = mix(lambda ox, oy: _gfix(f32(0.5) * (I[iy + oy, ix + ox + 1] - I[iy + oy, ix + ox - 1])))
    gy = mix(lambda ox, oy: _gfix(f32(0.5) * (I[iy + oy + 1, ix + ox] - I[iy + oy - 1, ix + ox])))
    return ok, val, gx, gy


def _huber(r, huber):
    ar = np.abs(r)
    with np.errstate(all="ignore"):
        return np.where(ar < huber, f32(1.0), huber / ar).astype(f32)


def trace_point(w, h, I, R, t, aff, pt, S):
    """one point; pt: dict of u, v, energy_th, grad_h (4), color (8), weights (8) and the state.  Returns (state, steps, branches)."""
    br = set()
    st = {k: pt[k] for k in ("status", "idepth_min", "idepth_max", "quality", "uv0", "uv1", "interval")}
    entered = st["status"]

    def oob_exit(name):
        br.add(name)
        st.update(uv0=f32(-1), uv1=f32(-1), interval=f32(0), status=OOB)
        return st, 0, br

    if entered == OOB:  # T1
        br.add("T1")
        return st, 0, br
    u, v, G = pt["u"], pt["v"], pt["grad_h"]
    stepsize = f32(S["stepsize"])
    maxPix = f32(f32(w + h) * f32(S["max_pix_search"]))  # T2
    pr = [f32(f32(f32(R[3 * i] * u) + f32(R[3 * i + 1] * v)) + R[3 * i + 2]) for i in range(3)]
    pmin = [f32(pr[i] + f32(t[i] * st["idepth_min"])) for i in range(3)]
    uMin, vMin = f32(pmin[0] / pmin[2]), f32(pmin[1] / pmin[2])
    if not _inside(uMin, vMin, w, h):
        return oob_exit("T2_oob")
    bounded = bool(np.isfinite(st["idepth_max"]))
    if bounded:  # T3
        pmax = [f32(pr[i] + f32(t[i] * st["idepth_max"])) for i in range(3)]
        uMax, vMax = f32(pmax[0] / pmax[2]), f32(pmax[1] / pmax[2])
        if not _inside(uMax, vMax, w, h):
            return oob_exit("T3_oob")
        du, dv = f32(uMin - uMax), f32(vMin - vMax)
        dist = f32(np.sqrt(f32(f32(du * du) + f32(dv * dv))))
        if dist < f32(S["slack_interval"]):
            br.add("T3_skipped")
            st.update(uv0=f32(f32(uMax + uMin) * f32(0.5)), uv1=f32(f32(vMax + vMin) * f32(0.5)), interval=dist, status=SKIPPED)
            return st, 0, br
    else:  # T4
        br.add("T4_taken")
        dist = maxPix
        pmax = [f32(pr[i] + f32(t[i] * f32(0.01))) for i in range(3)]
        uMax, vMax = f32(pmax[0] / pmax[2]), f32(pmax[1] / pmax[2])
        dx, dy = f32(uMax - uMin), f32(vMax - vMin)
        d = f32(f32(1.0) / f32(np.sqrt(f32(f32(dx * dx) + f32(dy * dy)))))
        uMax = f32(uMin + f32(f32(dist * dx) * d))
        vMax = f32(vMin + f32(f32(dist * dy) * d))
        if not _inside(uMax, vMax, w, h):
            return oob_exit("T4_oob")
    if not (st["idepth_min"] < 0 or (pmin[2] > f32(0.75) and pmin[2] < f32(1.5))):  # T5
        return oob_exit("T5_oob")
    dx, dy = f32(stepsize * f32(uMax - uMin)), f32(stepsize * f32(vMax - vMin))  # T6

    def form(p, q):
        return f32(f32(f32(f32(p * G[0]) + f32(q * G[2])) * p) + f32(f32(f32(p * G[1]) + f32(q * G[3])) * q))

    a, b = form(dx, dy), form(dy, f32(-dx))
    err = f32(f32(0.2) + f32(f32(f32(0.2) * f32(a + b)) / a))
    if f32(err * f32(S["min_improvement"])) > dist and bounded:
        br.add("T6_badcondition")
        st.update(uv0=f32(f32(uMax + uMin) * f32(0.5)), uv1=f32(f32(vMax + vMin) * f32(0.5)), interval=dist, status=BADCONDITION)
        return st, 0, br
    if err > f32(10):
        br.add("T6_clamp")
        err = f32(10)
    dx, dy = f32(dx / dist), f32(dy / dist)  # T7
    if dist > maxPix:
        br.add("T7_dist_above_maxpix")
        dist = maxPix
    fsteps = f32(f32(1.9999) + f32(dist / stepsize))
    numSteps = int(fsteps) if fsteps < f32(100) else 100  # (int): truncation; what no int holds is above the cap anyway
    k1000 = f32(uMin * f32(1000))
    randShift = f32(k1000 - np.floor(k1000))
    ptx, pty = f32(uMin - f32(randShift * dx)), f32(vMin - f32(randShift * dy))
    rpx = np.array([f32(f32(R[0] * f32(px)) + f32(R[1] * f32(py))) for px, py in PATTERN], f32)
    rpy = np.array([f32(f32(R[3] * f32(px)) + f32(R[4] * f32(py))) for px, py in PATTERN], f32)
    if not np.isfinite(dx) or not np.isfinite(dy):
        return oob_exit("T7_oob")
    if numSteps >= 100:
        br.add("T7_cap")
        numSteps = 99
    color, wt, huber = pt["color"], pt["weights"], f32(S["huber_th"])
    pred = (aff[0] * color + aff[1]).astype(f32)
    # T9: the positions are the chain of additions
    xs, ys = np.zeros(numSteps, f32), np.zeros(numSteps, f32)
    for i in range(numSteps):
        xs[i], ys[i] = ptx, pty
        ptx, pty = f32(ptx + dx), f32(pty + dy)
    ok, val, _, _ = _sample(I, w, h, xs[:, None] + rpx[None, :], ys[:, None] + rpy[None, :], False)
    fin = ok & np.isfinite(val)
    if (~ok).any():
        br.add("T8_guard_search")
    if (ok & ~np.isfinite(val)).any():
        br.add("nan_texel")
    r = (val - pred[None, :]).astype(f32)
    hw = _huber(r, huber)
    terms = np.where(fin, ((hw * r) * r) * (f32(2.0) - hw), f32(1e5)).astype(f32)
    errors = np.zeros(numSteps, f32)
    for k in range(8):
        errors = errors + terms[:, k]
    bestU, bestV, bestEnergy, bestIdx = f32(0), f32(0), f32(1e10), -1
    for i in range(numSteps):
        if errors[i] < bestEnergy:
            bestU, bestV, bestEnergy, bestIdx = xs[i], ys[i], errors[i], i
    if bestIdx == 0:
        br.add("best_at_step_0")
    if bestIdx == numSteps - 1:
        br.add("best_at_last_step")
    secondBest = f32(1e10)  # T10
    radius = int(S["min_test_radius"])
    for i in range(numSteps):
        if (i < bestIdx - radius or i > bestIdx + radius) and errors[i] < secondBest:
            secondBest = errors[i]
    q = f32(secondBest / bestEnergy)
    if numSteps > 10:
        br.add("T10_steps_above_10")
    else:
        br.add("T10_short_quality_lowered" if q < st["quality"] else "T10_short_quality_kept")
    if q < st["quality"] or numSteps > 10:
        st["quality"] = q
    uBak, vBak, stepBack = bestU, bestV, f32(0)  # T11
    if int(S["gn_iterations"]) > 0:
        bestEnergy = f32(1e5)
    for _ in range(int(S["gn_iterations"])):
        ok, val, gx, gy = _sample(I, w, h, (bestU + rpx).astype(f32), (bestV + rpy).astype(f32), True)
        fin = ok & np.isfinite(val)
        if (~ok).any():
            br.add("T8_guard_gn")
        if (ok & ~np.isfinite(val)).any():
            br.add("nan_texel")
        r = (val - pred).astype(f32)
        hw = _huber(r, huber)
        dRes = (dx * gx + dy * gy).astype(f32)
        tH, tb = ((hw * dRes) * dRes).astype(f32), ((hw * r) * dRes).astype(f32)
        tE = (((((wt * wt) * hw) * r) * r) * (f32(2.0) - hw)).astype(f32)
        Hs, bs, E = f32(1), f32(0), f32(0)
        for k in range(8):
            if fin[k]:
                Hs, bs, E = f32(Hs + tH[k]), f32(bs + tb[k]), f32(E + tE[k])
            else:
                E = f32(E + f32(1e5))
        if E > bestEnergy:
            br.add("T11_reject")
            stepBack = f32(stepBack * f32(0.5))
            bestU, bestV = f32(uBak + f32(stepBack * dx)), f32(vBak + f32(stepBack * dy))
        else:
            br.add("T11_accept")
            step = f32(f32(-bs) / Hs)
            if step < f32(-0.5):
                step = f32(-0.5)
                br.add("T11_clamp")
            elif step > f32(0.5):
                step = f32(0.5)
                br.add("T11_clamp")
            if not np.isfinite(step):
                step = f32(0)
            uBak, vBak, stepBack = bestU, bestV, step
            bestU, bestV = f32(bestU + f32(step * dx)), f32(bestV + f32(step * dy))
            bestEnergy = E
        if abs(stepBack) < f32(S["gn_threshold"]):
            br.add("T11_break")
            break
    if not bestEnergy < f32(pt["energy_th"] * f32(S["extra_slack_on_th"])):  # T12
        br.add("T12_outlier_to_oob" if entered == OUTLIER else "T12_outlier")
        st.update(uv0=f32(-1), uv1=f32(-1), interval=f32(0), status=OOB if entered == OUTLIER else OUTLIER)
        return st, numSteps, br
    if f32(dx * dx) > f32(dy * dy):  # T13
        br.add("T13_u_form")
        best, dd, p, tt = bestU, dx, pr[0], t[0]
    else:
        br.add("T13_v_form")
        best, dd, p, tt = bestV, dy, pr[1], t[1]
    xm, xp = f32(best - f32(err * dd)), f32(best + f32(err * dd))
    lo = f32(f32(f32(pr[2] * xm) - p) / f32(tt - f32(t[2] * xm)))
    hi = f32(f32(f32(pr[2] * xp) - p) / f32(tt - f32(t[2] * xp)))
    if lo > hi:
        br.add("T13_swap")
        lo, hi = hi, lo
    st["idepth_min"], st["idepth_max"] = lo, hi
    if not np.isfinite(lo) or not np.isfinite(hi) or hi < 0:  # T14
        br.add("T14")
        st.update(uv0=f32(-1), uv1=f32(-1), interval=f32(0), status=OUTLIER)
        return st, numSteps, br
    br.add("T15")
    st.update(interval=f32(f32(2) * err), uv0=bestU, uv1=bestV, status=GOOD)
    return st, numSteps, br


def trace(w, h, target, job, **params):
    """every point of a job (the dict of direct_stereo_slam_amd.trace) against the plane `target`"""
    S = dict(DEFAULTS, **params)
    I = np.asarray(target, f32).reshape(h, w)
    krki, kt, aff = (np.asarray(job[k], f32).reshape(-1, c) for k, c in (("krki", 9), ("kt", 3), ("aff", 2)))
    n = len(job["host"])
    uv = np.asarray(job["trace_uv"], f32).reshape(n, 2)
    out = dict(status=np.zeros(n, np.uint8), idepth_min=np.zeros(n, f32), idepth_max=np.zeros(n, f32), quality=np.zeros(n, f32),
               trace_uv=np.zeros((n, 2), f32), trace_interval=np.zeros(n, f32), steps=np.zeros(n, np.int32))
    branches, point_branches = dict.fromkeys(BRANCHES, 0), []
    with np.errstate(all="ignore"):
        for i in range(n):
            hst = int(job["host"][i])
            pt = dict(u=f32(job["u"][i]), v=f32(job["v"][i]), energy_th=f32(job["energy_th"][i]), grad_h=np.asarray(job["grad_h"], f32).reshape(n, 4)[i],
                      color=np.asarray(job["color"], f32).reshape(n, 8)[i], weights=np.asarray(job["weights"], f32).reshape(n, 8)[i],
                      status=int(job["status"][i]), idepth_min=f32(job["idepth_min"][i]), idepth_max=f32(job["idepth_max"][i]),
                      quality=f32(job["quality"][i]), uv0=uv[i, 0], uv1=uv[i, 1], interval=f32(job["trace_interval"][i]))
            st, steps, br = trace_point(w, h, I, krki[hst], kt[hst], aff[hst], pt, S)
            out["status"][i], out["idepth_min"][i], out["idepth_max"][i], out["quality"][i] = st["status"], st["idepth_min"], st["idepth_max"], st["quality"]
            out["trace_uv"][i], out["trace_interval"][i], out["steps"][i] = (st["uv0"], st["uv1"]), st["interval"], steps
            point_branches.append(br)
            for name in br:
                branches[name] += 1
    out["counts"] = np.bincount(out["status"], minlength=6).astype(np.int32)
    out["branches"], out["point_branches"] = branches, point_branches
    return out


def advance(job, res):
    """the job whose state is the outcome `res` of a trace: the input of the next frame's trace"""
    return dict(job, **{k: res[k].copy() for k in STATE})


# ---- the shared scene ----------------------------------------------------------------------------------------------------------------

W, H = 160, 64
FX, FY, CX, CY = 64.0, 64.0, 79.5, 31.5
PLANE_IDEPTH = 0.25
NAN_TEXELS = [(60, 20), (61, 20), (60, 41), (95, 30)]  # (x, y)


def texture(seed, x, y, plain=False):
    """six sinusoids, wavelengths 9 .. 30 px, about +-40 around 128; unless `plain`, columns 104 .. 127 hold stripes that depend on y
    alone and columns 128 .. 149 are flat"""
    rng = np.random.default_rng(2000 + seed)
    v = np.full(np.broadcast(x, y).shape, 128.0)
    for lam in np.linspace(9.0, 30.0, 6):
        th, ph = rng.uniform(0, np.pi), rng.uniform(0, 2 * np.pi)
        v = v + 13.0 * np.sin(2 * np.pi * (x * np.cos(th) + y * np.sin(th)) / lam + ph)
    if not plain:
        v = np.where((x >= 104) & (x < 128), 128.0 + 35.0 * np.sin(2 * np.pi * y / 9.0 + 1.0), v)
        v = np.where((x >= 128) & (x < 150), 128.0, v)
    return v


def _hosts():
    """K R K^-1 (row-major), K t and the affine pair of seven hosts: sideways, vertical, a small rotation, 35 degrees in the image plane,
    forward with the epipole at (80, 32), one whose depth changes enough for T5, and one whose matrix doubles the image about the
    principal point.  No rotation does that, but the call takes any matrix, and only a rotated pattern wider than the margin of the
    inside test (T2) reaches the sample guard (T8)."""
    K = np.array([[FX, 0, CX], [0, FY, CY], [0, 0, 1.0]])

    def rot(rx, ry, rz):
        cx_, sx = np.cos(rx), np.sin(rx)
        cy_, sy = np.cos(ry), np.sin(ry)
        cz, sz = np.cos(rz), np.sin(rz)
        return (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy_, 0, sy], [0, 1, 0], [-sy, 0, cy_]]) @
                np.array([[1, 0, 0], [0, cx_, -sx], [0, sx, cx_]]))

    Rs = [np.eye(3), np.eye(3), rot(0.01, -0.015, 0.02), rot(0, 0, np.deg2rad(35.0)), np.eye(3), np.eye(3), np.eye(3)]
    kts = [(16.0, 0, 0), (0, 12.0, 0), (-14.0, 5.0, 0.02), (10.0, -6.0, 0), (24.0, 9.6, 0.3), (8.0, 0, 0.6), (16.0, 0, 0)]
    affs = [(1.0, 0.0), (1.0, 0.0), (1.05, -3.0), (1.0, 0.0), (0.97, 2.0), (1.0, 0.0), (1.0, 0.0)]
    krki = np.stack([(K @ R @ np.linalg.inv(K)) for R in Rs])
    for i in (0, 1, 4, 5):
        krki[i] = np.eye(3)  # exactly
    krki[6] = np.array([[2.0, 0, -CX], [0, 2.0, -CY], [0, 0, 1.0]])
    return krki.reshape(-1, 9).astype(f32), np.array(kts, f32), np.array(affs, f32)


def project(krki, kt, x, y, idepth):
    """where the pixel (x, y) of a host lies in the new frame at inverse depth idepth (float64)"""
    M, t = krki.reshape(3, 3).astype(np.float64), kt.astype(np.float64)
    p = [M[i, 0] * x + M[i, 1] * y + M[i, 2] + t[i] * idepth for i in range(3)]
    return p[0] / p[2], p[1] / p[2]


def make_scene(seed=1, plain=False, n_random=150, noise=1.0, only=None):
    """(job without a target, target plane, true idepth).  The new frame is the texture with a few NaN texels; host k's image is
    what the plane at idepth 0.25 shows through its projection, under its affine pair.  Points sit at integer pixels; colour, weights
    and gradH come from the host image.  `plain`: the clean pair of the bracketing test (no stripes, no NaN, no noise, fresh points).
    `only`: these points alone, as tuples (host, u, v, status, idepth_min, idepth_max, quality, colour offset)."""
    rng = np.random.default_rng(seed)
    krki, kt, aff = _hosts()
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    target = texture(seed, xs, ys, plain).astype(f32)
    if not plain:
        for x, y in NAN_TEXELS:
            target[y, x] = np.nan
    host_img = []
    for k in range(len(kt)):
        px, py = project(krki[k], kt[k], xs, ys, PLANE_IDEPTH)
        host_img.append(((texture(seed, px, py, plain) - aff[k, 1]) / aff[k, 0]).astype(f32))
    pts = []  # (host, u, v, status, idepth_min, idepth_max, quality, colour offset)
    fresh = lambda hst, u, v, nan=False: pts.append((hst, u, v, UNINITIALIZED, 0.0, np.nan if nan else np.inf, 10000.0, 0.0))

    def narrowed(hst, u, v, lo, hi, status=GOOD, quality=None, off=0.0):
        pts.append((hst, u, v, status, lo, hi, rng.uniform(1.0, 3.0) if quality is None else quality, off))

    for i in range(0 if only is not None else n_random):  # fresh points anywhere, on every host
        fresh(i % 6, rng.integers(3, W - 3), rng.integers(3, H - 3), nan=bool(i & 1))
    if only is not None:
        pts.extend(only)
    elif not plain:
        for i in range(120):  # narrowed by earlier traces: intervals of every width around the truth
            r = rng.uniform(0.02, 1.5)
            c = PLANE_IDEPTH * rng.uniform(0.8, 1.25)
            narrowed(i % 6, rng.integers(3, W - 3), rng.integers(3, H - 3), c * (1 - r), c * (1 + r))
        for i in range(8):  # T1
            narrowed(i % 6, rng.integers(20, W - 20), rng.integers(10, H - 10), 0.2, 0.3, status=OOB)
        for i in range(16):  # T12: colours of another surface, half of them outliers already
            narrowed(i % 4, rng.integers(30, 90), rng.integers(12, H - 12), 0.05, 0.6, status=OUTLIER if i & 1 else GOOD, off=90.0)
        for i in range(48):  # the borders: T2, T3, T4 exits and the guard
            edge, hst = i % 4, (0, 1, 3, 0)[i % 4] if i < 24 else (2, 1, 0, 1)[i % 4]
            a, b = rng.integers(3, 10), rng.integers(8, 56)
            u, v = [(a, b), (rng.integers(8, 150), a), (W - 1 - a, b), (rng.integers(8, 150), H - 1 - a)][edge]
            if i % 3:
                fresh(hst, u, v)
            else:
                narrowed(hst, u, v, 0.05, rng.uniform(0.4, 1.2))
        for i in range(10):  # T5: the depth changes by more than a half
            lo = rng.uniform(0.9, 1.3)
            narrowed(5, rng.integers(60, 120), rng.integers(12, H - 12), lo, lo + rng.uniform(0.3, 0.6))
        for i in range(24):  # stripes along the epipolar line and flat ground: a = 0
            u = rng.integers(107, 120) if i % 2 else rng.integers(132, 142)
            if i % 4 < 2:
                fresh(0, u - 4, rng.integers(8, H - 8))
            else:
                narrowed(0, u - 4, rng.integers(8, H - 8), 0.1, 0.5)
        for i in range(24):  # next to the epipole of the forward host: the new interval straddles the pole
            du, dv = [(-2, 0), (-1, 0), (1, 0), (2, 0), (0, -2), (0, -1), (0, 1), (0, 2), (-1, -1), (1, 1), (-2, 1), (2, -1)][i % 12]
            fresh(4, 80 + du, 32 + dv)
        for i in range(16):  # the doubled host next to the upper and lower border: the rotated pattern reaches the guard
            if i % 2:
                fresh(6, rng.integers(50, 100), (18, 45)[(i // 2) % 2])
            else:
                narrowed(6, rng.integers(50, 100), (18, 45)[(i // 2) % 2], 0.05, 0.6)
        for i in range(28):  # the truth at the first step, and at the last
            hst = i % 2
            g = float(kt[hst, hst])  # pixels per unit of idepth
            u, v = rng.integers(20, 90), rng.integers(12, H - 20)
            if i % 4 < 2:
                narrowed(hst, u, v, PLANE_IDEPTH, PLANE_IDEPTH + rng.integers(3, 6) / g)
            else:
                narrowed(hst, u, v, 0.0, PLANE_IDEPTH - 0.5 / g)
        for i in range(24):  # lines across the NaN texels
            x, y = NAN_TEXELS[i % 4]
            fresh(0, x - 4 - rng.integers(0, 5), y + rng.integers(-2, 3))
        for i in range(10):  # room for 99 steps when max_pix_search allows them
            fresh(0, rng.integers(8, 40), rng.integers(8, H - 8))
    n = len(pts)
    host = np.array([p[0] for p in pts], np.int32)
    u, v = np.array([p[1] for p in pts], f32), np.array([p[2] for p in pts], f32)
    color, grad_h, weights = np.zeros((n, 8), f32), np.zeros((n, 4), f32), np.zeros((n, 8), f32)
    for i, p in enumerate(pts):
        img = host_img[p[0]]
        for k, (dx, dy) in enumerate(PATTERN):
            x, y = int(p[1]) + dx, int(p[2]) + dy
            gx, gy = f32(0.5) * (img[y, x + 1] - img[y, x - 1]), f32(0.5) * (img[y + 1, x] - img[y - 1, x])
            color[i, k] = img[y, x] + f32(p[7]) + f32(rng.normal(0, noise) if noise else 0.0)
            grad_h[i] += np.array([gx * gx, gx * gy, gx * gy, gy * gy], f32)
            weights[i, k] = np.sqrt(f32(2500.0) / (f32(2500.0) + (gx * gx + gy * gy)))
    job = dict(krki=krki, kt=kt, aff=aff, host=host, u=u, v=v, energy_th=np.full(n, 8 * 144.0, f32), grad_h=grad_h, color=color, weights=weights,
               status=np.array([p[3] for p in pts], np.uint8), idepth_min=np.array([p[4] for p in pts], f32),
               idepth_max=np.array([p[5] for p in pts], f32), quality=np.array([p[6] for p in pts], f32), trace_uv=np.zeros((n, 2), f32),
               trace_interval=np.zeros(n, f32))
    return job, target, PLANE_IDEPTH


# ---- a scene at any geometry: the 160 x 64 scene above is hard-wired to its size ------------------------------------------------------------
TX, TY = 8.0, 4.0  # pixels per unit of inverse depth of the sideways and of the vertical hosts: powers of two, so that a bound is met exactly
SIDES = ("left", "right", "top", "bottom")
SIDE_DELTAS = (0.25, 0.6, 1.2, 0.0, -0.25, -0.6, -1.2)  # how far inside the bound of T2 the projection at idepth_min lies; <= 0: outside


def side_bound(side, w, h):
    """(axis, bound, sign): T2 keeps a projection p when sign * (p[axis] - bound) > 0"""
    return {"left": (0, 4.0, 1), "right": (0, w - 5.0, -1), "top": (1, 4.0, 1), "bottom": (1, h - 5.0, -1)}[side]


def geometry_hosts(w, h):
    """five hosts: translations to the right, to the left, down and up (K R K^-1 the identity, exactly), and a small rotation"""
    K = np.array([[0.4 * w, 0, (w - 1) / 2.0], [0, 0.4 * w, (h - 1) / 2.0], [0, 0, 1.0]])
    a, b = 0.012, -0.01
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    krki = np.stack([np.eye(3)] * 4 + [K @ Rz @ Ry @ np.linalg.inv(K)])
    kts = [(TX, 0, 0), (-TX, 0, 0), (0, TY, 0), (0, -TY, 0), (-5.0, 3.0, 0.02)]
    affs = [(1.0, 0.0), (1.03, -2.0), (1.0, 0.0), (0.97, 2.0), (1.0, 1.0)]
    return krki.reshape(-1, 9).astype(f32), np.array(kts, f32), np.array(affs, f32)


def geometry_texture(seed, x, y, w):
    """the six sinusoids of `texture`; the columns [0.55 w, 0.8 w) hold stripes that depend on y alone (no gradient along a sideways
    epipolar line: T6)"""
    v = texture(seed, x, y, plain=True)
    return np.where((x >= int(0.55 * w)) & (x < int(0.8 * w)), 128.0 + 35.0 * np.sin(2 * np.pi * y / 9.0 + 1.0), v)


def make_scene_at(w, h, seed=1, n_random=60, noise=1.0):
    """(job, target plane, sides): the plane at idepth 0.25 seen by geometry_hosts; fresh and narrowed points on every host, skipped,
    ill-conditioned, outlier and out-of-bounds points, and next to each of the four sides points whose projection at idepth_min
    lies SIDE_DELTAS inside (or outside) the bound of T2.  sides: side -> the indices of its points, in SIDE_DELTAS' order."""
    rng = np.random.default_rng(seed)
    krki, kt, aff = geometry_hosts(w, h)
    nh = len(kt)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    target = geometry_texture(seed, xs, ys, w).astype(f32)
    host_img = []
    for k in range(nh):
        px, py = project(krki[k], kt[k], xs, ys, PLANE_IDEPTH)
        host_img.append(((geometry_texture(seed, px, py, w) - aff[k, 1]) / aff[k, 0]).astype(f32))
    pts, sides = [], {}
    ru, rv = (lambda: int(rng.integers(3, w - 3))), (lambda: int(rng.integers(3, h - 3)))
    fresh = lambda hst, u, v, nan=False: pts.append((hst, u, v, UNINITIALIZED, 0.0, np.nan if nan else np.inf, 10000.0, 0.0))
    narrowed = lambda hst, u, v, lo, hi, status=GOOD, off=0.0: pts.append((hst, u, v, status, lo, hi, rng.uniform(1.0, 3.0), off))
    for i in range(n_random):
        fresh(i % nh, ru(), rv(), nan=bool(i & 1))
    for i in range(n_random):  # intervals of every width around the truth
        r, c = rng.uniform(0.02, 1.5), PLANE_IDEPTH * rng.uniform(0.8, 1.25)
        narrowed(i % nh, ru(), rv(), c * (1 - r), c * (1 + r))
    for i in range(8):  # T3: less than slack_interval = 1.5 px between the ends
        narrowed(i % 4, ru(), rv(), PLANE_IDEPTH, PLANE_IDEPTH + rng.uniform(0.2, 1.2) / (TX, TX, TY, TY)[i % 4])
    for i in range(6):  # T1
        narrowed(i % nh, ru(), rv(), 0.2, 0.3, status=OOB)
    for i in range(12):  # T12: colours of another surface, half of them outliers already
        narrowed(i % 2, int(rng.integers(8, max(9, int(0.5 * w)))), rv(), 0.05, 0.6, status=OUTLIER if i & 1 else GOOD, off=90.0)
    for i in range(10):  # T6: stripes along the epipolar line of the sideways hosts
        narrowed(i % 2, int(rng.integers(int(0.55 * w) + 1, max(int(0.55 * w) + 2, int(0.8 * w) - 1))), rv(), 0.1, 0.5)
    for side in SIDES:
        axis, bound, sign = side_bound(side, w, h)
        hst = {"left": 1, "right": 0, "top": 3, "bottom": 2}[side]  # the host that moves the point towards the side
        g = (TX, TY)[axis]
        sides[side] = list(range(len(pts), len(pts) + len(SIDE_DELTAS)))
        for k, delta in enumerate(SIDE_DELTAS):
            at = 6 + k % 4  # the point's own distance from the side, in pixels: 6 .. 9
            lo = (at - 4 - delta) / g  # TX, TY and the bounds are exact in float32: delta = 0 meets the bound exactly
            along = int(rng.integers(8, (h, w)[axis] - 8))
            u, v = ((at, along), (w - 1 - at, along), (along, at), (along, h - 1 - at))[SIDES.index(side)]
            if k % 2:
                narrowed(hst, u, v, lo, lo + 0.3)
            else:
                pts.append((hst, u, v, GOOD, lo, np.inf, 2.0, 0.0))  # T4 behind a T2 that is passed or not
    n = len(pts)
    host = np.array([p[0] for p in pts], np.int32)
    u, v = np.array([p[1] for p in pts], f32), np.array([p[2] for p in pts], f32)
    color, grad_h, weights = np.zeros((n, 8), f32), np.zeros((n, 4), f32), np.zeros((n, 8), f32)
    for i, p in enumerate(pts):
        img = host_img[p[0]]
        for k, (dx, dy) in enumerate(PATTERN):
            x, y = int(p[1]) + dx, int(p[2]) + dy
            gx, gy = f32(0.5) * (img[y, x + 1] - img[y, x - 1]), f32(0.5) * (img[y + 1, x] - img[y - 1, x])
            color[i, k] = img[y, x] + f32(p[7]) + f32(rng.normal(0, noise) if noise else 0.0)
            grad_h[i] += np.array([gx * gx, gx * gy, gx * gy, gy * gy], f32)
            weights[i, k] = np.sqrt(f32(2500.0) / (f32(2500.0) + (gx * gx + gy * gy)))
    job = dict(krki=krki, kt=kt, aff=aff, host=host, u=u, v=v, energy_th=np.full(n, 8 * 144.0, f32), grad_h=grad_h, color=color, weights=weights,
               status=np.array([p[3] for p in pts], np.uint8), idepth_min=np.array([p[4] for p in pts], f32),
               idepth_max=np.array([p[5] for p in pts], f32), quality=np.array([p[6] for p in pts], f32), trace_uv=np.zeros((n, 2), f32),
               trace_interval=np.zeros(n, f32))
    return job, target, sides


GEOMETRIES = [(101, 53), (24, 20)]  # odd sizes, 184 points: partial waves at another stride; just above the 8 x 8 minimum
_geometry_cache = {}


def geometry_case(w, h):
    """(job, target, expected, sides) at a geometry, computed once"""
    if (w, h) not in _geometry_cache:
        job, target, sides = make_scene_at(w, h, seed=5)
        _geometry_cache[(w, h)] = (job, target, trace(w, h, target, job), sides)
    return _geometry_cache[(w, h)]


# name -> (make_scene arguments, dsm_trace_params fields); "defaults" and "wide" are the two cases whose branch coverage is asserted
CASES = {
    "defaults": (dict(seed=1), dict()),
    "wide": (dict(seed=1), dict(max_pix_search=0.5)),
    "huber_4": (dict(seed=2, n_random=60), dict(huber_th=4.0)),
    "no_gn": (dict(seed=2, n_random=60), dict(gn_iterations=0)),
    "gn_6": (dict(seed=2, n_random=60), dict(gn_iterations=6)),
    "radius_1": (dict(seed=2, n_random=60), dict(min_test_radius=1)),
    "half_steps": (dict(seed=2, n_random=60), dict(stepsize=0.5)),
}
_cache, _scenes = {}, {}


def scene(**kw):
    key = tuple(sorted(kw.items()))
    if key not in _scenes:
        _scenes[key] = make_scene(**kw)
    return _scenes[key]


def case(name):
    """(job, target, expected, params), computed once"""
    if name not in _cache:
        kw, params = CASES[name]
        job, target, _ = scene(**kw)
        _cache[name] = (job, target, trace(W, H, target, job, **params), params)
    return _cache[name]


_sequence = []


def sequence():
    """three frames in a row, the outputs of one trace being the inputs of the next: [(frame, job before, expected)]; every frame is
    the scene's new frame moved sideways by one more pixel"""
    if not _sequence:
        job, target, _, _ = case("defaults")
        for k in range(3):
            frame = np.ascontiguousarray(np.roll(target, k, axis=1))
            exp = trace(W, H, frame, job)
            _sequence.append((frame, job, exp))
            job = advance(job, exp)
    return _sequence


PER_POINT = ("host", "u", "v", "energy_th", "grad_h", "color", "weights") + STATE


def subset(job, idx, n_hosts=None):
    """the points `idx` of a job; n_hosts: only the first hosts (the points must not use the others)"""
    n = len(job["host"])
    out = dict(job, **{k: np.asarray(job[k]).reshape(n, -1)[idx].reshape((-1,) + np.asarray(job[k]).shape[1:]) for k in PER_POINT})
    if n_hosts is not None:
        out.update(krki=job["krki"][:n_hosts], kt=job["kt"][:n_hosts], aff=job["aff"][:n_hosts])
    return out


def subset_result(res, idx):
    out = {k: res[k][idx] for k in ("status", "idepth_min", "idepth_max", "quality", "trace_uv", "trace_interval", "steps")}
    out["counts"] = np.bincount(out["status"], minlength=6).astype(np.int32)
    return out


def same_bits(a, b):
    """float32 arrays: equal bit for bit, NaN payload aside"""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def assert_equal(got, exp):
    """status, steps and counts exactly; every float bit for bit, NaN payload aside"""
    for k in ("status", "steps", "counts"):
        assert np.array_equal(got[k], exp[k]), (k, np.flatnonzero(np.asarray(got[k]) != np.asarray(exp[k]))[:8])
    for k in ("idepth_min", "idepth_max", "quality", "trace_uv", "trace_interval"):
        g, e = np.asarray(got[k], f32), np.asarray(exp[k], f32)
        assert g.dtype == np.float32 and same_bits(g, e), (k, np.argwhere((g.view(np.uint32) != e.view(np.uint32)) & ~(np.isnan(g) & np.isnan(e)))[:8])


def invalid_calls(job):
    """(what, job, dsm_trace_params fields) of the calls that must be refused"""
    def changed(key, index, value):
        j = dict(job, **{key: np.array(job[key], copy=True)})
        j[key][index] = value
        return j

    nan, inf = float("nan"), float("inf")
    calls = [("host index past the end", changed("host", 3, len(job["kt"])), {}), ("host index below 0", changed("host", 0, -1), {}),
             ("status byte 6", changed("status", 2, 6), {}), ("17 hosts", dict(job, krki=np.zeros((17, 9), f32), kt=np.zeros((17, 3), f32),
                                                                            aff=np.zeros((17, 2), f32)), {}),
             ("gn_iterations 17", job, dict(gn_iterations=17)), ("gn_iterations -1", job, dict(gn_iterations=-1)),
             ("stepsize 0", job, dict(stepsize=0.0)), ("stepsize -1", job, dict(stepsize=-1.0)), ("stepsize inf", job, dict(stepsize=inf)),
             ("stepsize NaN", job, dict(stepsize=nan)), ("min_test_radius -1", job, dict(min_test_radius=-1))]
    for name in ("max_pix_search", "slack_interval", "min_improvement", "gn_threshold", "extra_slack_on_th", "huber_th"):
        calls.append((name + " NaN", job, {name: nan}))
    calls.append(("huber_th inf", job, dict(huber_th=inf)))
    return calls
