"""Independent checker of the Hessian and Schur accumulation of the window optimisation: the rules A0-A3, P1,
S1-S3 and T1 as the project states them, on top of the rows of the linearisation's checker (tests/_linearize_ref.py).  Every product
and every float sum rounds to float32 (numpy float32 scalars, or float32 arrays element by element, which round each operation the
same way); the accumulators and the stitch are float64 sums in the stated order.  Written from the statement, not from the C code.

hessian(job, lin, extra) returns the outputs of direct_stereo_slam_amd.hessian for a job whose linearisation result is `lin`;
with terms=True also the float terms of every accumulator entry, in the order they are added.  dense(...) is the float64
construction straight from T1's lift and g_p, with the same construction on absolute values beside it."""
import numpy as np

import _linearize_ref as R

f32, f64 = np.float32, np.float64
ZERO = f32(0.0)
# a row of L8
RESF, PDXI, PDC, PDD, IDX, ABF, IDX2, ABJIDX, AB2 = 0, 8, 20, 28, 30, 46, 62, 66, 70
EXTRA_KEYS = ("ad_host", "ad_target", "prior", "delta", "hdd_lin", "bd_lin", "hcd_lin", "shift_prior_to_zero")
RAW = ("acc_top", "acc_D", "acc_E", "acc_EB", "acc_Hcc", "acc_bc")
STITCHED = ("H_A", "b_A", "H_sc", "b_sc")
PER_POINT = ("hdd_acc", "bd_acc", "hcd_acc", "hdi", "bd_sum", "idepth_hessian")


def make_extra(job, seed, lin_inputs=True, shift=1):
    """what a hessian job holds on top of its linearize job: ad_host / ad_target near the identity, a prior on a third of the points,
    and (lin_inputs) non-zero sums of linearised residuals on a third"""
    rng = np.random.default_rng(1000 + seed)
    nf, n = len(job["frame_ids"]), len(job["host"])
    ex = dict(ad_host=-np.eye(8) + rng.normal(0, 0.2, (nf, nf, 8, 8)), ad_target=np.eye(8) + rng.normal(0, 0.2, (nf, nf, 8, 8)),
              shift_prior_to_zero=shift)
    ex["prior"] = np.where(rng.uniform(size=n) < 0.33, 2500.0, 0.0).astype(f32)
    ex["delta"] = rng.normal(0, 0.01, n).astype(f32)
    if lin_inputs:
        some = rng.uniform(size=n) < 0.33
        ex["hdd_lin"] = np.where(some, rng.uniform(0, 5e3, n), 0.0).astype(f32)
        ex["bd_lin"] = np.where(some, rng.normal(0, 50, n), 0.0).astype(f32)
        ex["hcd_lin"] = np.where(some[:, None], rng.normal(0, 50, (n, 4)), 0.0).astype(f32)
    return ex


def active_of(job, lin):
    """A0"""
    n = len(lin["new_state"])
    return (np.asarray(job["state_in"])[:n] != R.OOB) & (lin["new_state"] == R.IN)


def record(row):
    """A1, A2 and the operands of A3 of one active residual from its row"""
    row = np.asarray(row, f32)
    ji, jab, rr = [ZERO, ZERO], [ZERO, ZERO], ZERO
    for i in range(8):
        r = row[RESF + i]
        for k in range(2):
            ji[k] = f32(ji[k] + f32(r * row[IDX + 8 * k + i]))
            jab[k] = f32(jab[k] + f32(r * row[ABF + 8 * k + i]))
        rr = f32(rr + f32(r * r))
    x = np.concatenate([row[PDC:PDC + 4], row[PDXI:PDXI + 6]])
    y = np.concatenate([row[PDC + 4:PDC + 8], row[PDXI + 6:PDXI + 12]])
    d = row[PDD:PDD + 2]
    i2, k2 = row[IDX2:IDX2 + 4], row[ABJIDX:ABJIDX + 4]
    v0 = f32(f32(i2[0] * d[0]) + f32(i2[1] * d[1]))
    v1 = f32(f32(i2[2] * d[0]) + f32(i2[3] * d[1]))
    jp = [f32(f32(row[PDXI + i] * v0) + f32(row[PDXI + 6 + i] * v1)) for i in range(6)]
    jp += [f32(f32(k2[0] * d[0]) + f32(k2[1] * d[1])), f32(f32(k2[2] * d[0]) + f32(k2[3] * d[1]))]
    return dict(x=x, y=y, d=d, i2=i2, k2=k2, ab2=row[AB2:AB2 + 4], ji=ji, jab=jab, rr=rr, v=(v0, v1), jp=np.array(jp, f32))


def top_term(q):
    """A3: the 13 x 13 float term, full"""
    x, y = q["x"], q["y"]
    T = np.zeros((13, 13), f32)
    xx, xy, yx, yy = np.outer(x, x), np.outer(x, y), np.outer(y, x), np.outer(y, y)  # float32 products, one rounding each
    T[:10, :10] = (xx * q["i2"][0] + (xy + yx) * q["i2"][1]) + yy * q["i2"][3]
    T[:10, 10] = x * q["k2"][0] + y * q["k2"][1]
    T[:10, 11] = x * q["k2"][2] + y * q["k2"][3]
    T[:10, 12] = x * q["ji"][0] + y * q["ji"][1]
    T[10, 10], T[10, 11], T[10, 12] = q["ab2"][0], q["ab2"][1], q["jab"][0]
    T[11, 11], T[11, 12], T[12, 12] = q["ab2"][3], q["jab"][1], q["rr"]
    iu = np.triu_indices(13, 1)
    T[(iu[1], iu[0])] = T[iu]
    return T


def point_sums(recs):
    """S1 over the records of a point's active residuals, in ascending residual index"""
    bd, hdd, hcd = ZERO, ZERO, [ZERO] * 4
    for q in recs:
        d, (v0, v1) = q["d"], q["v"]
        bd = f32(bd + f32(f32(q["ji"][0] * d[0]) + f32(q["ji"][1] * d[1])))
        hdd = f32(hdd + f32(f32(v0 * d[0]) + f32(v1 * d[1])))
        hcd = [f32(hcd[c] + f32(f32(q["x"][c] * v0) + f32(q["y"][c] * v1))) for c in range(4)]
    return hdd, bd, hcd


def point_finish(hdd, bd, hcd, prior, delta, hdd_lin, bd_lin, hcd_lin, shift):
    """S2 for a point with an active residual: idepth_hessian, hdi, bd_sum, Hcd"""
    H = f32(f32(hdd + hdd_lin) + prior)
    if H < f32(1e-10):
        H = f32(1e-10)
    hdi = f32(1.0 / float(H))
    bd_sum = f32(bd + bd_lin)
    if shift:
        bd_sum = f32(bd_sum + f32(prior * delta))
    return H, hdi, bd_sum, np.array([f32(hcd[c] + hcd_lin[c]) for c in range(4)], f32)


def mm(A, B):
    """A B in float64: every entry the sum over ascending k, from 0.0"""
    C = np.zeros((A.shape[0], B.shape[1]))
    for k in range(A.shape[1]):
        C = C + A[:, k][:, None] * B[k, :][None, :]
    return C


def stitch(nf, ad_host, ad_target, acc):
    """T1 from the raw accumulators: H_A, b_A, H_sc, b_sc"""
    N = 4 + 8 * nf
    HA, bA, HS, bS = np.zeros((N, N)), np.zeros(N), np.zeros((N, N)), np.zeros(N)
    blk = lambda f: slice(4 + 8 * f, 12 + 8 * f)  # noqa: E731
    for h in range(nf):
        for t in range(nf):
            if t == h:
                continue
            A, Ah, At = acc["acc_top"][h, t], ad_host[h, t], ad_target[h, t]
            HA[:4, :4] += A[:4, :4]
            bA[:4] += A[:4, 12]
            HA[:4, blk(h)] += mm(A[:4, 4:12], Ah.T)
            HA[:4, blk(t)] += mm(A[:4, 4:12], At.T)
            Mh, Mt = mm(Ah, A[4:12, 4:12]), mm(At, A[4:12, 4:12])
            HA[blk(h), blk(h)] += mm(Mh, Ah.T)
            HA[blk(h), blk(t)] += mm(Mh, At.T)
            HA[blk(t), blk(h)] += mm(Mt, Ah.T)
            HA[blk(t), blk(t)] += mm(Mt, At.T)
            bA[blk(h)] += mm(Ah, A[4:12, 12:13])[:, 0]
            bA[blk(t)] += mm(At, A[4:12, 12:13])[:, 0]
    HS[:4, :4], bS[:4] = acc["acc_Hcc"], acc["acc_bc"]
    for h in range(nf):
        for t1 in range(nf):
            if t1 == h:
                continue
            Ah1, At1 = ad_host[h, t1], ad_target[h, t1]
            E, EB = acc["acc_E"][h, t1], acc["acc_EB"][h, t1]
            HS[:4, blk(h)] += mm(Ah1, E).T
            HS[:4, blk(t1)] += mm(At1, E).T
            bS[blk(h)] += mm(Ah1, EB[:, None])[:, 0]
            bS[blk(t1)] += mm(At1, EB[:, None])[:, 0]
            for t2 in range(nf):
                if t2 == h:
                    continue
                Ah2, At2, D = ad_host[h, t2], ad_target[h, t2], acc["acc_D"][h, t1, t2]
                Mh, Mt = mm(Ah1, D), mm(At1, D)
                HS[blk(h), blk(h)] += mm(Mh, Ah2.T)
                HS[blk(h), blk(t2)] += mm(Mh, At2.T)
                HS[blk(t1), blk(h)] += mm(Mt, Ah2.T)
                HS[blk(t1), blk(t2)] += mm(Mt, At2.T)
    for M in (HA, HS):  # the lower half mirrors the upper
        iu = np.triu_indices(N, 1)
        M[(iu[1], iu[0])] = M[iu]
    return dict(H_A=HA, b_A=bA, H_sc=HS, b_sc=bS)


def _point_inputs(ex, n):
    z1, z4 = np.zeros(n, f32), np.zeros((n, 4), f32)
    get = lambda k, z: np.asarray(ex[k], f32).reshape(z.shape) if ex.get(k) is not None else z  # noqa: E731
    return get("prior", z1), get("delta", z1), get("hdd_lin", z1), get("bd_lin", z1), get("hcd_lin", z4)


def hessian(job, lin, extra, terms=False, drop=()):
    """every output of a hessian job from the linearisation's result `lin` (its rows and states); `drop`: residuals left out on
    purpose (for the tests that show a bound has teeth)"""
    host, point, target = (np.asarray(job[k]) for k in ("host", "point", "target"))
    nf, n, nr = len(job["frame_ids"]), len(host), len(lin["new_state"])
    active = active_of(job, lin)
    for r in drop:
        active[r] = False
    recs = {r: record(lin["J"][r]) for r in range(nr) if active[r]}
    out = dict(active=active.astype(np.uint8), JpJdF=np.full((nr, 8), -7, f32))
    acc = dict(acc_top=np.zeros((nf, nf, 13, 13)), acc_D=np.zeros((nf, nf, nf, 8, 8)), acc_E=np.zeros((nf, nf, 8, 4)),
               acc_EB=np.zeros((nf, nf, 8)), acc_Hcc=np.zeros((4, 4)), acc_bc=np.zeros(4))
    T = {k: {} for k in RAW}

    def add(key, at, term):
        acc[key][at] = acc[key][at] + term.astype(f64)
        if terms:
            T[key].setdefault(at, []).append(term)

    for r in range(nr):  # P1: ascending residual index
        if active[r]:
            out["JpJdF"][r] = recs[r]["jp"]
            add("acc_top", (int(host[point[r]]), int(target[r])), top_term(recs[r]))
    prior, delta, hdd_lin, bd_lin, hcd_lin = _point_inputs(extra, n)
    shift = int(extra.get("shift_prior_to_zero", 1))
    per = {k: np.zeros((n, 4) if k == "hcd_acc" else n, f32) for k in PER_POINT}
    of_point = [[r for r in range(nr) if point[r] == p and active[r]] for p in range(n)]
    for p in range(n):  # S1, S2, then S3 in ascending point index
        hdd, bd, hcd = point_sums([recs[r] for r in of_point[p]])
        per["hdd_acc"][p], per["bd_acc"][p], per["hcd_acc"][p] = hdd, bd, hcd
        if not of_point[p]:
            continue
        H, hdi, bd_sum, Hcd = point_finish(hdd, bd, hcd, prior[p], delta[p], hdd_lin[p], bd_lin[p], hcd_lin[p], shift)
        per["idepth_hessian"][p], per["hdi"][p], per["bd_sum"][p] = H, hdi, bd_sum
        h = int(host[p])
        add("acc_Hcc", (), np.outer(Hcd, Hcd) * hdi)
        add("acc_bc", (), Hcd * f32(bd_sum * hdi))
        for r1 in of_point[p]:
            j1, t1 = recs[r1]["jp"], int(target[r1])
            add("acc_E", (h, t1), np.outer(j1, Hcd) * hdi)
            add("acc_EB", (h, t1), j1 * f32(hdi * bd_sum))
            for r2 in of_point[p]:
                add("acc_D", (h, t1, int(target[r2])), np.outer(j1, recs[r2]["jp"]) * hdi)
    out.update(acc)
    out.update(per)
    out.update(stitch(nf, np.asarray(extra["ad_host"], f64).reshape(nf, nf, 8, 8), np.asarray(extra["ad_target"], f64).reshape(nf, nf, 8, 8), acc))
    if terms:
        out["terms"] = T
    return out


def lift(nf, h, t, ad_host, ad_target):
    """L_ht of T1: N x 12"""
    L = np.zeros((4 + 8 * nf, 12))
    L[:4, :4] = np.eye(4)
    L[4 + 8 * h:12 + 8 * h, 4:] = ad_host[h, t]
    L[4 + 8 * t:12 + 8 * t, 4:] = ad_target[h, t]
    return L


def dense(job, lin, extra):
    """(value, magnitude) of H_A, b_A, H_sc, b_sc in float64 straight from the rows: A1-A3 / S1-S2 re-evaluated in float64, then T1's
    lift and g_p; `magnitude` is the same construction with every operand replaced by its absolute value."""
    host, point, target = (np.asarray(job[k]) for k in ("host", "point", "target"))
    nf, n, nr = len(job["frame_ids"]), len(host), len(lin["new_state"])
    N = 4 + 8 * nf
    adh, adt = (np.asarray(extra[k], f64).reshape(nf, nf, 8, 8) for k in ("ad_host", "ad_target"))
    active = active_of(job, lin)
    prior, delta, hdd_lin, bd_lin, hcd_lin = (a.astype(f64) for a in _point_inputs(extra, n))
    shift = int(extra.get("shift_prior_to_zero", 1))
    res = []
    for ab in (False, True):
        m = np.abs if ab else (lambda a: a)
        HA, bA, HS, bS = np.zeros((N, N)), np.zeros(N), np.zeros((N, N)), np.zeros(N)
        pts = [dict(hdd=0.0, bd=0.0, hcd=np.zeros(4), g=np.zeros(N - 4), hdd_true=0.0, k=0) for _ in range(n)]
        for r in range(nr):
            if not active[r]:
                continue
            row = lin["J"][r].astype(f64)
            true = dict(i2=row[IDX2:IDX2 + 4].reshape(2, 2), d=row[PDD:PDD + 2])
            row = m(row)
            h, t = int(host[point[r]]), int(target[r])
            L = m(lift(nf, h, t, adh, adt))
            JI, JAB, res8 = row[IDX:IDX + 16].reshape(2, 8), row[ABF:ABF + 16].reshape(2, 8), row[RESF:RESF + 8]
            XY = np.stack([np.concatenate([row[PDC:PDC + 4], row[PDXI:PDXI + 6]]), np.concatenate([row[PDC + 4:PDC + 8], row[PDXI + 6:PDXI + 12]])])
            I2, K2, d = row[IDX2:IDX2 + 4].reshape(2, 2), row[ABJIDX:ABJIDX + 4].reshape(2, 2), row[PDD:PDD + 2]
            T = np.zeros((13, 13))
            T[:10, :10] = XY.T @ I2 @ XY
            T[:10, 10:12] = XY.T @ K2.T
            T[:10, 12] = XY.T @ (JI @ res8)
            T[10:12, 10:12] = row[AB2:AB2 + 4].reshape(2, 2)
            T[10:12, 12] = JAB @ res8
            T[12, 12] = res8 @ res8
            T = np.triu(T) + np.triu(T, 1).T
            HA += L @ T[:12, :12] @ L.T
            bA += L @ T[:12, 12]
            v = I2 @ d
            jp = np.concatenate([XY[:, 4:].T @ v, K2 @ d])
            P = pts[int(point[r])]
            P["bd"] += (JI @ res8) @ d
            P["hdd"] += v @ d
            P["hdd_true"] += (true["i2"] @ true["d"]) @ true["d"]
            P["hcd"] += XY[:, :4].T @ v
            P["g"] += L[4:, 4:] @ jp
            P["k"] += 1
        for p, P in enumerate(pts):
            if not P["k"]:
                continue
            H_true = max(P["hdd_true"] + hdd_lin[p] + prior[p], float(f32(1e-10)))
            hdi = 1.0 / H_true
            if ab and H_true > float(f32(1e-10)):  # the reciprocal's share of H's magnitude over its value
                hdi *= (P["hdd"] + m(hdd_lin[p]) + m(prior[p])) / H_true
            bd_sum = P["bd"] + m(bd_lin[p]) + (m(prior[p]) * m(delta[p]) if shift else 0.0)
            g = np.concatenate([P["hcd"] + m(hcd_lin[p]), P["g"]])
            HS += hdi * np.outer(g, g)
            bS += hdi * bd_sum * g
        res.append(dict(H_A=HA, b_A=bA, H_sc=HS, b_sc=bS))
    return res[0], res[1]


# ---- the shared scenes ------------------------------------------------------------------------------------------------------------

# name -> (the linearize case it sits on, extras).  "clamp": two frames where PRE_tTll_0 of [0][1] is zero, so that Jpdd = 0 for the
# points of frame 0, without prior or linearised sums: H falls under 1e-10.  "wide": two frames and 140 points, so that a pair holds
# more than 48 residuals, a host more than 64 points and the job more than 128 points (the chunk sizes of the device kernels).
CASES = {
    "scene": ("scene", dict(seed=1)),
    "nine_frames": ("nine_frames", dict(seed=2, shift=0)),
    "one_frame": ("one_frame", dict(seed=3)),
    "three_frames_no_residuals": ("three_frames_no_residuals", dict(seed=4)),
    "two_frames": ("two_frames", dict(seed=5, lin_inputs=False)),
    "no_points": ("no_points", dict(seed=6)),
}
_cache = {}


def _lin_case(name):
    """(job, frames, linearisation result, per-residual results)"""
    if name in R.CASES:
        return R.case(name)
    if ("lin", name) not in _cache:
        if name == "clamp":
            job, frames = R.make_case(seed=5, n_frames=2, n_pts=40, fix=1)
            job["pre_tTll_0"] = job["pre_tTll_0"].copy()
            job["pre_tTll_0"][0, 1] = 0.0
        elif name == "wide":
            job, frames = R.make_case(seed=11, n_frames=2, n_pts=140, fix=1)
        elif name == "sixteen_frames":
            job, frames = R.make_case(seed=12, n_frames=16, n_pts=40, fix=1)
        per = R.residuals_of(R.W, R.H, job, frames)
        _cache[("lin", name)] = (job, frames, R.assemble(job, per, None), per)
    return _cache[("lin", name)]


def extra_of(name, job):
    if name in CASES:
        return make_extra(job, **CASES[name][1])
    if name == "clamp":
        ex = make_extra(job, seed=7, lin_inputs=False)
        ex["prior"] = np.zeros(len(job["host"]), f32)
        return ex
    return make_extra(job, seed=len(name))


def case(name, terms=False):
    """(job with its extras, frames, expected), computed once"""
    key = (name, terms)
    if key not in _cache:
        job, frames, lin, _ = _lin_case(name)
        job = dict(job, **extra_of(name, job))
        _cache[key] = (job, frames, dict(lin, **hessian(job, lin, job, terms=terms)))
    return _cache[key]


def case_prefix(name, n, fix=None):
    """(job, expected) of the first n residuals of a case"""
    job, frames, lin, per = _lin_case(name)
    sub = R.prefix(job, n)
    if fix is not None:
        sub["fix_linearization"] = fix
    sub = dict(sub, **extra_of(name, job))
    lin_sub = R.assemble(sub, per[:n], None)
    return sub, dict(lin_sub, **hessian(sub, lin_sub, sub))


def case_points(name, m):
    """(job, expected) of the first m points of a case and the residuals of those points"""
    job, frames, lin, per = _lin_case(name)
    idx = [r for r in range(len(job["point"])) if job["point"][r] < m]
    sub = R.subset(job, idx)
    ex = extra_of(name, job)
    for k in ("host", "u", "v", "idepth_scaled", "idepth_zero_scaled", "color", "weights"):
        sub[k] = np.asarray(job[k])[:m].copy()
    for k in ("prior", "delta", "hdd_lin", "bd_lin", "hcd_lin"):
        if ex.get(k) is not None:
            ex[k] = ex[k][:m].copy()
    sub = dict(sub, **ex)
    lin_sub = R.assemble(sub, [per[i] for i in idx], None)
    return sub, dict(lin_sub, **hessian(sub, lin_sub, sub))


def assert_equal(got, exp, outputs=RAW + ("active", "JpJdF") + PER_POINT, lin_outputs=("center_projected_to", "projected_to", "keep", "rel_bs")):
    """the linearisation as its checker has it; every float and double of the accumulation bit for bit (tobytes()); JpJdF on the
    active residuals only"""
    R.assert_equal(got, exp, outputs=lin_outputs)
    for k in STITCHED + tuple(outputs):
        a, b = np.asarray(got[k]), np.asarray(exp[k])
        if k == "JpJdF":
            on = exp["active"].astype(bool)
            assert (a[~on] == -7).all(), "JpJdF of a residual that is not active was written"
            a, b = a[on], b[on]
        assert a.dtype == b.dtype and a.shape == b.shape, (k, a.dtype, b.dtype, a.shape, b.shape)
        assert a.tobytes() == b.tobytes(), (k, np.argwhere(a != b)[:6], a[a != b][:3], b[a != b][:3])


def invalid_jobs(job):
    """(what, job) of the calls the Hessian call refuses on top of the linearisation's"""
    def with_(key, at, value):
        a = np.array(job[key], copy=True)
        a[at] = value
        return dict(job, **{key: a})

    dup = np.asarray(job["point"]).copy()
    r = next(r for r in range(1, len(dup)) if dup[r] == dup[r - 1])
    tgt = np.asarray(job["target"]).copy()
    tgt[r] = tgt[r - 1]
    out = [("no ad_host", dict(job, ad_host=None)), ("no ad_target", dict(job, ad_target=None)),
           ("ad_host NaN", with_("ad_host", (1, 0, 3, 3), np.nan)), ("ad_target inf", with_("ad_target", (0, 1, 7, 0), np.inf)),
           ("prior NaN", with_("prior", 3, np.nan)), ("delta inf", with_("delta", 0, np.inf)), ("hdd_lin NaN", with_("hdd_lin", 5, np.nan)),
           ("bd_lin -inf", with_("bd_lin", 2, -np.inf)), ("hcd_lin NaN", with_("hcd_lin", (4, 3), np.nan)),
           ("two residuals of a point against one target", dict(job, target=tgt))]
    return out
