"""Independent checker of the end of optimize behind its loop: the rules Z1-Z8 as numpy / Python loops, layered on
the checkers of sections 16, 19 and 20 (tests/_linearize_ref.py, _step_ref.py, _optimize_ref.py; imported, not edited).  Doubles are
Python floats (IEEE binary64, one rounding per operation, in the order written), floats are numpy float32 scalars, sums are loops in
the stated order; exp, sin and cos are the C library's (math.*).

finish(job, frames, loop) takes the loop's result (_optimize_ref.run) and returns every output of dsm_finish_job under its name.  The
pieces (new_eval_point, frames_at, adjoint_pair, tables, ad_ht_delta, bookkeeping) are callable on their own, so that a comparison
against a device whose sincos and exp differ in the last places can start from the device's own read-back."""
import math

import numpy as np

import _linearize_ref as R
import _optimize_ref as O
import _step_ref as T
import _window_files as W

f32, f64 = np.float32, np.float64
IN, OOB, OUTLIER = 0, 1, 2
FINISH_IN = ("n_good_residuals_in", "max_rel_baseline_in", "last_res", "last_state_in")
PRE_OUT = tuple(k + "_out" for k in T.PRE)
FRAME_OUT = ("world_to_cam_eval_out", "state_zero_out", "state_out", "ad_host_out", "ad_target_out", "ad_ht_delta_out", "c_delta_out", "delta_x_out",
             "cam_out") + PRE_OUT
LIN_OUT = ("new_state", "new_energy", "new_energy_with_outlier", "keep", "rel_bs", "energy", "frame_energy_th_out")
BOOK_OUT = ("n_good_residuals_out", "max_rel_baseline_out", "last_res_out", "last_state_out", "n_res_kept", "point_dropped", "res_index_out",
            "point_index_out", "n_res_out", "n_pts_out", "rmse", "lost")
ALL_OUT = FRAME_OUT + LIN_OUT + BOOK_OUT + ("cam_to_world_out",)
# the outputs that hold no result of an exp or a sincos of the form itself: decisions, integers and what derives from them
DECISIONS = ("new_state", "keep", "n_good_residuals_out", "last_res_out", "last_state_out", "n_res_kept", "point_dropped", "res_index_out",
             "point_index_out", "n_res_out", "n_pts_out", "lost")


def scales(sp):
    return [sp["scale_xi_trans"]] * 3 + [sp["scale_xi_rot"]] * 3 + [sp["scale_a"], sp["scale_b"]]


# ---- Z1 -----------------------------------------------------------------------------------------------------------------------------

def new_eval_point(job, loop, keep_old=False):
    """(eval', state', state_zero') as lists of lists of Python floats.  keep_old: the mutation "Z1 dropped" """
    n = len(job["frame_ids"])
    ev = [[float(x) for x in row] for row in np.asarray(job["world_to_cam_eval"], f64).reshape(n, 7)]
    zero = [[float(x) for x in row] for row in np.asarray(job["state_zero"], f64).reshape(n, 8)]
    state = [[float(x) for x in row] for row in np.asarray(loop["state"], f64).reshape(n, 8)]
    if not keep_old:
        f = n - 1
        ev[f] = [float(x) for x in np.asarray(loop["world_to_cam"], f64).reshape(n, 7)[f]]
        state[f] = [0.0] * 6 + [state[f][6], state[f][7]]
        zero[f] = list(state[f])
    return ev, state, zero


# ---- Z3's frames: D2 on given values ------------------------------------------------------------------------------------------------

def frames_at(ev, state, zero, sp):
    sc = scales(sp)
    n = len(ev)
    scaled = [[state[k][i] * sc[i] for i in range(8)] for k in range(n)]
    Wc = [T.se3_mul(T.se3_exp(scaled[k][:6]), ev[k]) for k in range(n)]
    return dict(W=Wc, C=[T.se3_inverse(w) for w in Wc], Ei=[T.se3_inverse(e) for e in ev],
                delta_f=[[state[k][i] - zero[k][i] for i in range(8)] for k in range(n)], aff=[scaled[k][6:8] for k in range(n)],
                aff0=[[zero[k][6] * sp["scale_a"], zero[k][7] * sp["scale_b"]] for k in range(n)])


# ---- Z2 -----------------------------------------------------------------------------------------------------------------------------

def adjoint(eval_t, eval_inv_h):
    """Adj(L0) as 6 rows of 6, L0 = eval_t eval_h^-1"""
    L0 = T.se3_mul(eval_t, eval_inv_h)
    Rm = T.quat_to_rot(L0)
    tx, ty, tz = L0[4:7]
    Tm = [0.0, -tz, ty, tz, 0.0, -tx, -ty, tx, 0.0]
    A = [[0.0] * 6 for _ in range(6)]
    for i in range(3):
        for j in range(3):
            tr = (Tm[i * 3 + 0] * Rm[0 * 3 + j] + Tm[i * 3 + 1] * Rm[1 * 3 + j]) + Tm[i * 3 + 2] * Rm[2 * 3 + j]
            A[i][j], A[i][3 + j], A[3 + i][j], A[3 + i][3 + j] = Rm[i * 3 + j], tr, 0.0, Rm[i * 3 + j]
    return A


def aff_a0(aff0_h, aff0_t, exp_h, exp_t):
    eh, et = f32(exp_h), f32(exp_t)
    if eh == 0 or et == 0:
        eh = et = f32(1.0)
    return float(f32(math.exp(aff0_t[0] - aff0_h[0]) * float(et) / float(eh)))


def adjoint_pair(Adj, a, sp):
    """(AH, AT): 8 rows of 8 Python floats"""
    sc = scales(sp)
    AH, AT = [[0.0] * 8 for _ in range(8)], [[0.0] * 8 for _ in range(8)]
    for k in range(8):
        for c in range(8):
            h = t = 1.0 if k == c else 0.0
            if k < 6 and c < 6:
                h = -Adj[c][k]
            if k == 6 and c == 6:
                h, t = a, -a
            if k == 7 and c == 7:
                h, t = a, -1.0
            AH[k][c], AT[k][c] = h * sc[k], t * sc[k]
    return AH, AT


def adjoints(job, ev, Ei, aff0, sp, a_of=None):
    """ad_host, ad_target (n, n, 8, 8): the job's, with the pairs of the newest frame replaced.  a_of[h, t]: Z2's a from elsewhere"""
    n = len(ev)
    f = n - 1
    AH, AT = np.array(job["ad_host"], f64).reshape(n, n, 8, 8).copy(), np.array(job["ad_target"], f64).reshape(n, n, 8, 8).copy()
    expo = np.asarray(job["exposure"], f32)
    for h in range(n):
        for t in range(n):
            if h != f and t != f:
                continue
            a = aff_a0(aff0[h], aff0[t], expo[h], expo[t]) if a_of is None else float(a_of[h, t])
            AH[h, t], AT[h, t] = adjoint_pair(adjoint(ev[t], Ei[h]), a, sp)
    return AH, AT


# ---- Z3 -----------------------------------------------------------------------------------------------------------------------------

def calibration(job, loop, params):
    value = [float(x) for x in np.asarray(loop["calib"], f64)]
    czero = np.asarray(job["calib_zero"], f64)
    cam = [f32(float(f32(params["scale_f"] if c < 2 else params["scale_c"])) * value[c]) for c in range(4)]
    cam += [f32(f32(1.0) / cam[0]), f32(f32(1.0) / cam[1])]
    return cam, [f32(value[c] - float(czero[c])) for c in range(4)]


def tables(job, ev, zero, F, cam, sp, aff_a=None):
    n = len(ev)
    expo = np.asarray(job["exposure"], f32)
    pre = {k: np.zeros((n, n, m), f32) for k, m in R.PRE}
    for h in range(n):
        for t in range(n):
            if h == t:
                continue
            o = T.pair_row(ev[t], F["Ei"][h], F["W"][t], F["C"][h], cam, expo[h], expo[t], F["aff"][h], F["aff"][t], zero[h][7], sp["scale_b"],
                           None if aff_a is None else np.asarray(aff_a, f32).reshape(n, n)[h, t])
            for k in T.PRE:
                pre[k][h, t] = o[k]
    return pre


def ad_ht_delta(AH, AT, delta_f):
    """section 21's setDeltaF: float products and sums over ascending k from 0, the host's part and the target's part added last"""
    n = len(delta_f)
    out = np.zeros((n, n, 8), f32)
    for h in range(n):
        for t in range(n):
            if h == t:
                continue
            for c in range(8):
                a = b = f32(0.0)
                for k in range(8):
                    a = f32(a + f32(f32(delta_f[h][k]) * f32(AH[h, t, k, c])))
                for k in range(8):
                    b = f32(b + f32(f32(delta_f[t][k]) * f32(AT[h, t, k, c])))
                out[h, t, c] = f32(a + b)
    return out


# ---- Z5 - Z8 ------------------------------------------------------------------------------------------------------------------------

def bookkeeping(job, lin, energy):
    """from the final linearisation's keep, new_state and rel_bs (and its energy): every output of Z5-Z8"""
    point, is_new = np.asarray(job["point"], int), np.asarray(job["is_new"])
    m, nr = len(job["host"]), len(point)
    keep, state, rel = np.asarray(lin["keep"]), np.asarray(lin["new_state"]), np.asarray(lin["rel_bs"], f32)
    n_good = np.array(job["n_good_residuals_in"], np.int32).reshape(m).copy()
    mrb = np.array(job["max_rel_baseline_in"], f32).reshape(m).copy()
    last_in = np.asarray(job["last_res"], np.int32).reshape(m, 2)
    last_res, last_state = last_in.copy(), np.array(job["last_state_in"], np.uint8).reshape(m, 2).copy()
    kept = np.zeros(m, np.int32)
    for r in range(nr):  # ascending index; a point's residuals in ascending index among them
        p = point[r]
        if keep[r]:
            kept[p] += 1
        if keep[r] and is_new[r]:
            n_good[p] += 1
            if rel[r] > mrb[p]:
                mrb[p] = rel[r]
    for p in range(m):
        l0, l1 = int(last_in[p, 0]), int(last_in[p, 1])
        if l0 >= 0:
            last_state[p, 0] = state[l0]
        if l1 >= 0 and l1 != l0:
            last_state[p, 1] = state[l1]
        if l0 >= 0 and not keep[l0]:
            last_res[p, 0] = -1
        if l1 >= 0 and l1 != l0 and not keep[l1]:
            last_res[p, 1] = -1
    dropped = (kept == 0).astype(np.uint8)
    res_index, point_index = np.full(nr, -1, np.int32), np.full(m, -1, np.int32)
    k = 0
    for r in range(nr):
        if keep[r]:
            res_index[r] = k
            k += 1
    q = 0
    for p in range(m):
        if not dropped[p]:
            point_index[p] = q
            q += 1
    with np.errstate(all="ignore"):
        rmse = np.sqrt(f32(f64(energy) / f64(8 * k)))
    return dict(n_good_residuals_out=n_good, max_rel_baseline_out=mrb, last_res_out=last_res, last_state_out=last_state, n_res_kept=kept,
                point_dropped=dropped, res_index_out=res_index, point_index_out=point_index, n_res_out=k, n_pts_out=q, rmse=f32(rmse),
                lost=int(not math.isfinite(float(energy))))


# ---- the whole ----------------------------------------------------------------------------------------------------------------------

def final_job(job, loop, pre, cam, params):
    """the linearize job of Z4: the window at the committed state on Z3's tables, with the fix flag"""
    c = {k: v for k, v in job.items() if k not in T.STEP_IN + FINISH_IN}
    eth = np.array(job["frame_energy_th"], f32, copy=True)
    eth[-1] = loop["new_frame_energy_th"]
    ids = (f32(params["scale_idepth"]) * np.asarray(loop["idepth"], f32)).astype(f32)
    c.update(pre)
    c.update(cam=tuple(cam[:4]), cam_inv=tuple(cam[4:]), idepth_scaled=ids, idepth_zero_scaled=ids, frame_energy_th=eth, state_in=loop["new_state"],
             energy_in=loop["new_energy"], fix_linearization=1)
    return c


def finish(job, frames, loop, sp=None, params=None, w=R.W, h=R.H, keep_old=False):
    """Z1-Z8 on the loop's result `loop` (_optimize_ref.run's): the outputs of dsm_finish_job by name"""
    sp = dict(T.SP, **(sp or {}))
    P = dict(R.PARAMS, **(params or {}))
    n = len(job["frame_ids"])
    with np.errstate(all="ignore"):
        ev, state, zero = new_eval_point(job, loop, keep_old)
        F = frames_at(ev, state, zero, sp)
        AH, AT = adjoints(job, ev, F["Ei"], F["aff0"], sp)
        cam, c_delta = calibration(job, loop, P)
        pre = tables(job, ev, zero, F, cam, sp)
        lin = R.linearize(w, h, final_job(job, loop, pre, cam, P), frames, params)
        out = bookkeeping(job, lin, lin["energy"])
    out.update(world_to_cam_eval_out=np.array(ev, f64).reshape(n, 7), state_zero_out=np.array(zero, f64).reshape(n, 8), state_out=np.array(state, f64).reshape(n, 8),
               ad_host_out=AH, ad_target_out=AT, ad_ht_delta_out=ad_ht_delta(AH, AT, F["delta_f"]), c_delta_out=np.array(c_delta, f32),
               delta_x_out=np.array([float(c) for c in c_delta] + [x for k in range(n) for x in F["delta_f"][k]], f64), cam_out=np.array(cam, f32),
               cam_to_world_out=np.array(F["C"], f64).reshape(n, 7), new_state=lin["new_state"], new_energy=lin["new_energy"],
               new_energy_with_outlier=lin["new_energy_with_outlier"], keep=lin["keep"], rel_bs=lin["rel_bs"], energy=f64(lin["energy"]),
               frame_energy_th_out=f32(lin["new_frame_energy_th"]), J_out=lin["J"], defined=lin["defined"], frames_at=F)
    out.update({k + "_out": pre[k] for k in T.PRE})
    return out


def run(job, frames, max_iterations, op=None, **kw):
    """(the loop's result, the finish's result)"""
    loop = O.run({k: v for k, v in job.items() if k not in FINISH_IN}, frames, max_iterations, op)
    return loop, finish(job, frames, loop, **kw)


# ---- the scenes: _step_ref's with seeded counters and last residuals ------------------------------------------------------------------

def seeded(job, seed=1):
    """the finish's inputs on a step scene's job.  Per point: n_good_residuals_in 0..5; max_rel_baseline_in 0 for two points in three (a
    kept new residual raises it) and 50 for the rest (none does); last_res: slot 0 one of the point's residuals or -1, slot 1 another
    one, the same one (the source's else-if) or -1; residuals in neither slot remain.  is_new is the scene's."""
    rng = np.random.default_rng(9000 + seed)
    point = np.asarray(job["point"], int)
    m = len(job["host"])
    of = [np.flatnonzero(point == p) for p in range(m)]
    last = np.full((m, 2), -1, np.int32)
    for p in range(m):
        if len(of[p]) == 0:
            continue
        if rng.random() < 0.8:
            last[p, 0] = rng.choice(of[p])
        u = rng.random()
        if u < 0.6:
            last[p, 1] = rng.choice(of[p])
        elif u < 0.7:
            last[p, 1] = last[p, 0]
    return dict(job, n_good_residuals_in=rng.integers(0, 6, m).astype(np.int32),
                max_rel_baseline_in=np.where(rng.random(m) < 2 / 3, 0.0, 50.0).astype(f32), last_res=last,
                last_state_in=rng.choice(np.array([IN, OOB, OUTLIER], np.uint8), (m, 2)))


_cache = {}


def scene(name, **kw):
    """(window job with the finish's inputs, frames), computed once"""
    key = (name, tuple(sorted(kw.items())))
    if key not in _cache:
        job, frames = T.scene(name, **kw)
        _cache[key] = (seeded(O.window_job(job), T.SCENES[name]["seed"]), frames)
    return _cache[key]


def expected(name, max_iterations=6, **op):
    """(job, frames, the loop's result, the finish's result), computed once"""
    key = ("exp", name, max_iterations, tuple(sorted(op.items())))
    if key not in _cache:
        job, frames = scene(name)
        _cache[key] = (job, frames) + run(job, frames, max_iterations, op)
    return _cache[key]


def assert_equal(got, exp, keys=ALL_OUT, what=""):
    """bit for bit; a NaN is compared as a NaN"""
    for k in keys:
        a, b = np.asarray(got[k]), np.asarray(exp[k])
        if a.dtype.kind in "iu" or b.dtype.kind in "iu":
            assert np.array_equal(a.reshape(-1).astype(np.int64), b.reshape(-1).astype(np.int64)), (what, k, a.reshape(-1)[:8], b.reshape(-1)[:8])
            continue
        assert a.dtype == b.dtype, (what, k, a.dtype, b.dtype)
        a, b = a.reshape(-1), b.reshape(-1)
        assert a.shape == b.shape, (what, k, a.shape, b.shape)
        view = np.uint64 if a.dtype == f64 else np.uint32
        nan = np.isnan(a) & np.isnan(b)
        ne = (a.view(view) != b.view(view)) & ~nan
        assert not ne.any(), (what, k, np.argwhere(ne)[:6].ravel(), a[ne][:3], b[ne][:3])


def assert_rows_equal(got, exp, what=""):
    """J_out: the rows of the residuals that do not end OOB (L8)"""
    d = np.asarray(exp["defined"], bool)
    assert np.asarray(got["J_out"])[d].tobytes() == np.asarray(exp["J_out"])[d].tobytes(), what


# ---- two keyframes: optimize + finish, marginalise, shrink, optimize + finish (the chain makeKeyFrame runs) ---------------------------

def marginalize_job(job, loop, fin, leaves):
    """The window as the finish left it, shrunk by Z7's maps, as dsm_marginalize_job takes it: the tables, cam, adHost, adTarget,
    adHTdeltaF, cDeltaF, the counters and the last states are the finish's; frame `leaves` is flagged and marginalised with prior
    100 (k + 1) and delta prior 0.001 (k + 1).  Returns (job, kept residuals, points that stay), indices into the window's lists."""
    nf = len(job["frame_ids"])
    rk, pk = np.flatnonzero(np.asarray(fin["keep"]) == 1), np.flatnonzero(np.asarray(fin["point_dropped"]) == 0)
    flagged = np.zeros(nf, np.uint8)
    flagged[leaves] = 1
    eth = np.array(job["frame_energy_th"], f32, copy=True)
    eth[-1] = fin["frame_energy_th_out"]
    idepth = (f32(R.PARAMS["scale_idepth"]) * np.asarray(loop["idepth"], f32)[pk]).astype(f32)
    m = {k: job[k] for k in ("frame_ids",)}
    m.update({k: np.asarray(job[k])[pk] for k in ("host", "u", "v", "color", "weights", "prior")})
    m.update({k: fin[k + "_out"] for k in T.PRE})
    m.update(point=np.asarray(fin["point_index_out"])[np.asarray(job["point"])[rk]].astype(np.int32), target=np.asarray(job["target"])[rk],
             is_new=np.asarray(job["is_new"])[rk], state_in=np.asarray(fin["new_state"])[rk], energy_in=np.asarray(fin["new_energy"], f32)[rk],
             cam=tuple(fin["cam_out"][:4]), cam_inv=tuple(fin["cam_out"][4:]), frame_energy_th=eth, idepth_scaled=idepth, idepth_zero_scaled=idepth,
             fix_linearization=0, delta=None, ad_host=fin["ad_host_out"], ad_target=fin["ad_target_out"], flagged=flagged,
             n_good_residuals=np.asarray(fin["n_good_residuals_out"])[pk], last_state=np.asarray(fin["last_state_out"])[pk],
             idepth_hessian=np.asarray(loop["idepth_hessian"], f32)[pk], ad_ht_delta=fin["ad_ht_delta_out"], c_delta=fin["c_delta_out"],
             H_M=job.get("H_M"), b_M=job.get("b_M"), marg_frames=np.array([leaves], np.int32),
             frame_prior=100.0 * np.arange(1, 9, dtype=f64).reshape(1, 8), frame_delta_prior=0.001 * np.arange(1, 9, dtype=f64).reshape(1, 8))
    return m, rk, pk


def second_job(job, frames, loop, fin, mjob, rk, pk, verdict, H_M_out, b_M_out, leaves):
    """the next keyframe's finish job: the frames that stay, the points of verdict 0 and their residuals against those frames, at the
    finish's evaluation point, on the returned prior; the counters, last residuals and last states carried over"""
    nf = len(job["frame_ids"])
    N = 4 + 8 * nf
    stay = [f for f in range(nf) if f != leaves]
    new_frame, new_point = -np.ones(nf, int), -np.ones(len(pk), int)
    new_frame[stay] = np.arange(len(stay))
    pts = np.flatnonzero(np.asarray(verdict) == 0)
    new_point[pts] = np.arange(len(pts))
    res = np.array([r for r in range(len(rk)) if new_point[mjob["point"][r]] >= 0 and new_frame[mjob["target"][r]] >= 0], int)
    new_res = -np.ones(len(job["point"]), int)
    new_res[rk[res]] = np.arange(len(res))
    idx = list(range(4)) + [4 + 8 * f + k for f in stay for k in range(8)]
    d = lambda k, shape: np.asarray(job[k], f64).reshape(shape)  # noqa: E731
    last = np.asarray(fin["last_res_out"])[pk][pts]
    two = dict(job)
    two.update(frame_ids=np.asarray(job["frame_ids"])[stay], frame_energy_th=np.asarray(mjob["frame_energy_th"], f32)[stay],
               host=new_frame[np.asarray(mjob["host"])[pts]].astype(np.int32), point=new_point[np.asarray(mjob["point"])[res]].astype(np.int32),
               target=new_frame[np.asarray(mjob["target"])[res]].astype(np.int32), state_in=np.asarray(mjob["state_in"])[res],
               energy_in=np.asarray(mjob["energy_in"], f32)[res], is_new=np.asarray(mjob["is_new"])[res])
    for k in ("u", "v", "color", "weights", "prior", "hdd_lin", "bd_lin", "hcd_lin"):
        two[k] = np.asarray(job[k])[pk][pts]
    two.update(ad_host=np.asarray(fin["ad_host_out"])[np.ix_(stay, stay)].copy(), ad_target=np.asarray(fin["ad_target_out"])[np.ix_(stay, stay)].copy(),
               H_L=d("H_L", (N, N))[np.ix_(idx, idx)].copy(), b_L=d("b_L", N)[idx], H_M=H_M_out, b_M=b_M_out, n_null=0, null_basis=None, null_pinv=None,
               world_to_cam_eval=np.asarray(fin["world_to_cam_eval_out"])[stay], state_zero=np.asarray(fin["state_zero_out"])[stay],
               state_backup=np.asarray(fin["state_out"])[stay], calib_backup=np.asarray(loop["calib"], f64), idepth_backup=np.asarray(loop["idepth"], f32)[pk][pts],
               exposure=np.asarray(job["exposure"], f32)[stay], n_good_residuals_in=np.asarray(fin["n_good_residuals_out"])[pk][pts],
               max_rel_baseline_in=np.asarray(fin["max_rel_baseline_out"], f32)[pk][pts], last_state_in=np.asarray(fin["last_state_out"])[pk][pts],
               last_res=np.where(last >= 0, new_res[np.maximum(last, 0)], -1).astype(np.int32))
    if job.get("state_prior") is not None:
        two.update(state_prior=d("state_prior", N)[idx], state_prior_zero=d("state_prior_zero", N)[idx])
    return two, [frames[f] for f in stay]


def keyframe_chain(job, frames, max_iterations, finish_fn, marg_fn, leaves=1):
    """finish_fn(job, frames, max_iterations) -> (loop's result, finish's result); marg_fn(marginalize job, frames) -> a dict with
    verdict, H_M_out, b_M_out, n_res_marg.  Returns the pieces of the chain by name."""
    loop, fin = finish_fn(job, frames, max_iterations)
    mjob, rk, pk = marginalize_job(job, loop, fin, leaves)
    marg = marg_fn(mjob, frames)
    two, frames2 = second_job(job, frames, loop, fin, mjob, rk, pk, marg["verdict"], marg["H_M_out"], marg["b_M_out"], leaves)
    loop2, fin2 = finish_fn(two, frames2, max_iterations)
    return dict(loop=loop, fin=fin, mjob=mjob, marg=marg, two=two, frames2=frames2, loop2=loop2, fin2=fin2)


def checker_chain(name="scene", max_iterations=6):
    """the chain through the checkers alone, computed once"""
    import _marginalize_ref as M

    key = ("chain", name, max_iterations)
    if key not in _cache:
        job, frames = scene(name)
        _cache[key] = keyframe_chain(job, frames, max_iterations, lambda j, f, its: run(j, f, its), lambda m, f: M.marginalize(R.W, R.H, m, f))
    return _cache[key]


# ---- for tools/finish_host_standalone.cpp ------------------------------------------------------------------------------------------

def write_case(path, w, h, job, frames):
    """the finish file (tests/_window_files.py)"""
    W.write_finish(path, w, h, job, frames)


def hashes(loop, fin):
    """what tools/finish_host_standalone.cpp prints, from the checker's results"""
    raw = lambda a: W.fnv1a(np.ascontiguousarray(a).tobytes())  # noqa: E731
    hx = lambda a: f"{raw(a):016x}"  # noqa: E731
    tables = 0
    for k in T.PRE:
        tables ^= raw(fin[k + "_out"])
    return dict(n_res=len(fin["keep"]), pattern=loop["pattern"], passes=loop["n_passes"], n_res_out=int(fin["n_res_out"]), n_pts_out=int(fin["n_pts_out"]),
                lost=int(fin["lost"]), x=hx(loop["x"]), eval=hx(fin["world_to_cam_eval_out"]), state=hx(fin["state_out"]), ad_host=hx(fin["ad_host_out"]),
                ad_target=hx(fin["ad_target_out"]), ad_ht_delta=hx(fin["ad_ht_delta_out"]), delta_x=hx(fin["delta_x_out"]), tables=f"{tables:016x}",
                new_state=hx(fin["new_state"]), new_energy=hx(fin["new_energy"]), keep=hx(fin["keep"]), rel_bs=hx(fin["rel_bs"]),
                energy=hx(np.array([fin["energy"]], f64)), n_good=hx(fin["n_good_residuals_out"]), max_rel_baseline=hx(fin["max_rel_baseline_out"]),
                last_res=hx(fin["last_res_out"]), last_state=hx(fin["last_state_out"]), res_index=hx(fin["res_index_out"]),
                point_index=hx(fin["point_index_out"]), cam_to_world=hx(fin["cam_to_world_out"]), lean_equal=1)
