"""Independent checker of adopting the stereo scale into the window: the rules S0-S6 as numpy / Python loops,
written from FrontEnd.cpp:1010-1061 and the text of S2-S4.  Doubles are Python floats (IEEE binary64, one rounding per operation, in
the order written), floats are numpy float32 scalars.  Q1-Q4 and the SE3 pieces are tests/_step_ref.py's, D2 on given values, the
calibration's D1 and setDeltaF are tests/_finish_ref.py's (imported, not edited).

rescale(job) returns every output of dsm_rescale_job under the names direct_stereo_slam_amd.rescale gives them.  The scenes are
synthetic windows (make_scene) and the finished windows of _finish_ref's scenes (finished_scene)."""
import math
import struct

import numpy as np

import _finish_ref as F
import _linearize_ref as R
import _step_ref as T
import _window_files as W

f32, f64 = np.float32, np.float64
DISABLED, REJECTED, ACCEPTED = 0, 1, 2
PRE = T.PRE
POINT = ("idepth", "idepth_scaled", "idepth_zero_scaled", "delta")
ARRAYS = POINT + ("world_to_cam_eval", "state", "state_zero", "cam_to_tracking_ref", "cam_to_world") + PRE + (
    "cam", "c_delta", "delta_x", "ad_ht_delta", "world_to_cam", "cam_to_world_all")
WORDS = ("decision", "scale_error", "trapped", "fails", "applied_scale")
ALL_OUT = ARRAYS + WORDS
SCALES = (0.1, 1.0, 1.4, 1.6, 50.0, -2.0)


# ---- S0, S1: FrontEnd.cpp:806, :1010-1023, :1057-1060 line by line ---------------------------------------------------------------------

def decide(enabled, scale_error, new_scale, thres, trapped, fails):
    """(decision, the returned error, trapped, fails)"""
    scale_error, new_scale, thres = f32(scale_error), f32(new_scale), f32(thres)
    if not enabled:                                                   # :806, :810
        return DISABLED, f32(-1.0), int(trapped), int(fails)
    scale_trapped, scale_opt_fails = bool(trapped), int(fails)
    scale_opt_succeed = bool(scale_error < thres)                     # :1010
    scale_jump = math.fabs(float(new_scale) - 1.0) > 0.5              # :1013
    if scale_trapped and scale_jump:                                  # :1014
        scale_opt_succeed = False
    scale_opt_fails = 0 if scale_opt_succeed else scale_opt_fails + 1  # :1019
    if scale_opt_fails > 5:                                           # :1020
        scale_trapped = False
        scale_error = f32(-1.0)
    if scale_opt_succeed and not scale_trapped:                       # :1057
        scale_trapped = True
    return (ACCEPTED if scale_opt_succeed else REJECTED), scale_error, int(scale_trapped), scale_opt_fails


# ---- S2-S4 -----------------------------------------------------------------------------------------------------------------------------

def rows(a, w):
    return [[float(x) for x in r] for r in np.asarray(a, f64).reshape(-1, w)]


def newest_frame(job, sp):
    """S3: (camToTrackingRef', camToWorld', eval'[f], state'[f])"""
    s = float(f32(job["new_scale"]))
    ctr = [float(x) for x in np.asarray(job["cam_to_tracking_ref"], f64)]
    ctr = ctr[:4] + [ctr[4] * s, ctr[5] * s, ctr[6] * s]                                  # :1045
    c2w = T.se3_mul([float(x) for x in np.asarray(job["ref_cam_to_world"], f64)], ctr)     # :1046
    ia, ib = float(f32(1.0) / f32(sp["scale_a"])), float(f32(1.0) / f32(sp["scale_b"]))    # SCALE_A_INVERSE, SCALE_B_INVERSE
    g = [float(x) for x in job["aff_g2l"]]
    return ctr, c2w, T.se3_inverse(c2w), [0.0] * 6 + [ia * g[0], ib * g[1]]                # :1048: setEvalPT_scaled


def rescale(job, sp=None, params=None):
    sp = dict(T.SP, **(sp or {}))
    P = dict(R.PARAMS, **(params or {}))
    dec, err, trapped, fails = decide(job["enabled"], job["scale_error"], job["new_scale"], job["thres"], job["trapped"], job["fails"])
    out = dict(decision=dec, scale_error=err, trapped=trapped, fails=fails, applied_scale=f32(job["new_scale"]) if dec == ACCEPTED else f32(1.0))
    n = np.asarray(job["state"]).reshape(-1, 8).shape[0]
    if dec != ACCEPTED:                                                                   # S6
        for k in ARRAYS:
            out[k] = None if job.get(k) is None else np.array(job[k], copy=True)
        return out
    scale = f32(job["new_scale"])
    with np.errstate(all="ignore"):
        idepth = (np.asarray(job["idepth"], f32).reshape(-1) / scale).astype(f32)           # :1038
        ids = (f32(P["scale_idepth"]) * idepth).astype(f32)
    out.update(idepth=idepth, idepth_scaled=ids, idepth_zero_scaled=ids.copy(), delta=np.zeros(len(idepth), f32))  # :1039
    ev, state, zero = rows(job["world_to_cam_eval"], 7), rows(job["state"], 8), rows(job["state_zero"], 8)
    f = n - 1
    ctr, c2w, ev[f], state[f] = newest_frame(job, sp)
    zero[f] = list(state[f])
    # S4: setPrecalcValues (:1055, :964-972)
    Fr = F.frames_at(ev, state, zero, sp)
    cam, c_delta = F.calibration(dict(calib_zero=job["calib_zero"]), dict(calib=job["calib_value"]), P)
    pre = F.tables(dict(exposure=job["exposure"]), ev, zero, Fr, cam, sp)
    AH, AT = np.asarray(job["ad_host"], f64).reshape(n, n, 8, 8), np.asarray(job["ad_target"], f64).reshape(n, n, 8, 8)
    out.update(world_to_cam_eval=np.array(ev, f64), state=np.array(state, f64), state_zero=np.array(zero, f64), cam_to_tracking_ref=np.array(ctr, f64),
               cam_to_world=np.array(c2w, f64), cam=np.array(cam, f32), c_delta=np.array(c_delta, f32),
               delta_x=np.array([float(c) for c in c_delta] + [x for k in range(n) for x in Fr["delta_f"][k]], f64),
               ad_ht_delta=F.ad_ht_delta(AH, AT, Fr["delta_f"]), world_to_cam=np.array(Fr["W"], f64), cam_to_world_all=np.array(Fr["C"], f64))
    out.update(pre)
    return out


# ---- the scenes ------------------------------------------------------------------------------------------------------------------------

def given_tables(ev, state, zero, exposure, calib_value, calib_zero, AH, AT, sp=None, params=None):
    """what setPrecalcValues left at the given values: the inputs that a job that is not accepted returns"""
    sp = dict(T.SP, **(sp or {}))
    P = dict(R.PARAMS, **(params or {}))
    n = len(ev)
    Fr = F.frames_at(ev, state, zero, sp)
    cam, c_delta = F.calibration(dict(calib_zero=calib_zero), dict(calib=calib_value), P)
    pre = F.tables(dict(exposure=exposure), ev, zero, Fr, cam, sp)
    g = dict(cam=np.array(cam, f32), c_delta=np.array(c_delta, f32),
             delta_x=np.array([float(c) for c in c_delta] + [x for k in range(n) for x in Fr["delta_f"][k]], f64),
             ad_ht_delta=F.ad_ht_delta(AH, AT, Fr["delta_f"]), world_to_cam=np.array(Fr["W"], f64), cam_to_world_all=np.array(Fr["C"], f64))
    g.update(pre)
    return g, Fr


def make_scene(seed=1, n_frames=3, n_pts=65, new_scale=1.4, ref=None, scale_error=0.5, thres=1.0, trapped=0, fails=0, enabled=1, consistent=True,
               perturb_eval=False):
    """A window of n_frames at distinct poses with rotations of about 0.1 and pose states of about 1e-3 (frame 0: none, so its se3_exp
    takes the series branch), points spread over the hosts (host[p] = p mod n_frames).  ref: the index of the tracking reference in the
    window, or None: a frame outside it.  consistent: the newest frame's given eval is (ref_cam_to_world cam_to_tracking_ref)^-1, the
    reference (if inside) has no pose state and eval[ref] = ref_cam_to_world^-1; perturb_eval then moves the given eval[f] off it.
    Returns the job with "host", "u", "v" on top (the points' hosts and pixels, which the call does not read)."""
    rng = np.random.default_rng(25000 + seed)
    n, f = n_frames, n_frames - 1
    ev = []
    for k in range(n):
        ev.append(T._rot_quat(rng.normal(0, 0.06, 3)) + [float(x) for x in rng.normal(0, 0.3, 3) + (0.4 * k, 0.0, 0.0)])
    zero = np.zeros((n, 8))
    zero[:, 6], zero[:, 7] = rng.normal(0, 0.002, n), rng.normal(0, 0.002, n)
    state = zero.copy()
    if n > 1:
        state[1:, :3] += rng.normal(0, 2e-3, (n - 1, 3))
        state[1:, 3:6] += rng.normal(0, 1e-3, (n - 1, 3))
    state[:, 6] += rng.normal(0, 1e-3, n)
    state[:, 7] += rng.normal(0, 1e-5, n)
    state[f, :6] = zero[f, :6] = 0.0
    state[f, 6:] = zero[f, 6:]  # as setEvalPT left the newest frame
    ctr = T._rot_quat(rng.normal(0, 0.05, 3)) + [float(x) for x in rng.normal(0, 0.2, 3) + (0.0, 0.0, 0.3)]
    if ref is not None and ref != f:
        state[ref, :6] = 0.0
        ref_c2w = T.se3_inverse(ev[ref])
    else:
        ref = None
        ref_c2w = T._rot_quat(rng.normal(0, 0.06, 3)) + [float(x) for x in rng.normal(0, 0.3, 3)]
    if consistent:
        ev[f] = T.se3_inverse(T.se3_mul(ref_c2w, ctr))
    c2w = T.se3_inverse(ev[f])
    if perturb_eval:
        ev[f] = T.se3_mul(T._rot_quat([0.01, -0.02, 0.015]) + [0.05, -0.03, 0.02], ev[f])
    expo = rng.uniform(0.8, 1.25, n).astype(f32)
    if n > 2:
        expo[1] = 0.0
    czero = np.array([277.34, 291.40, 312.23, 239.78]) / 50.0
    cval = czero + rng.normal(0, 1e-5, 4)
    AH, AT = rng.normal(0, 1, (n, n, 8, 8)), rng.normal(0, 1, (n, n, 8, 8))
    sp = T.SP
    given, _ = given_tables(ev, [list(map(float, r)) for r in state], [list(map(float, r)) for r in zero], expo, cval, czero, AH, AT)
    idepth = rng.uniform(0.05, 2.0, n_pts).astype(f32)
    ids = (f32(R.PARAMS["scale_idepth"]) * idepth).astype(f32)
    job = dict(enabled=enabled, scale_error=scale_error, new_scale=new_scale, thres=thres, trapped=trapped, fails=fails, idepth=idepth, idepth_scaled=ids,
               idepth_zero_scaled=(ids * f32(0.97)).astype(f32), delta=(ids - ids * f32(0.97)).astype(f32), world_to_cam_eval=np.array(ev, f64),
               state=state, state_zero=zero, exposure=expo, cam_to_tracking_ref=np.array(ctr, f64), ref_cam_to_world=np.array(ref_c2w, f64),
               cam_to_world=np.array(c2w, f64), aff_g2l=(float(state[f, 6]) * sp["scale_a"], float(state[f, 7]) * sp["scale_b"]), calib_value=cval,
               calib_zero=czero, ad_host=AH, ad_target=AT, host=np.arange(n_pts, dtype=np.int32) % n, ref=ref,
               u=rng.uniform(20, 600, n_pts).astype(f32), v=rng.uniform(20, 440, n_pts).astype(f32))
    job.update(given)
    return job


def finished_scene(name, new_scale=1.4, inside=True, max_iterations=2, **words):
    """The window dsm_window_finish_batch leaves on _finish_ref's scene `name`, shrunk by Z7's point map, as the rescale call takes it:
    the tracking reference is frame n - 2 (inside, n > 1) or a pose outside the window."""
    job, frames, loop, fin = F.expected(name, max_iterations)
    sp = T.SP
    n, f = len(job["frame_ids"]), len(job["frame_ids"]) - 1
    pk = np.flatnonzero(np.asarray(fin["point_dropped"]) == 0)
    idepth = np.asarray(loop["idepth"], f32)[pk]
    ids = (f32(R.PARAMS["scale_idepth"]) * idepth).astype(f32)
    Wc, Cw = fin["frames_at"]["W"], fin["frames_at"]["C"]
    if inside and n > 1:
        ref, ref_c2w, ctr = n - 2, Cw[n - 2], T.se3_mul(Wc[n - 2], Cw[f])
    else:
        ref, ref_c2w = None, T._rot_quat([0.01, 0.02, -0.01]) + [0.1, -0.05, 0.02]
        ctr = T.se3_mul(T.se3_inverse(ref_c2w), Cw[f])
    state = np.asarray(fin["state_out"], f64).reshape(n, 8)
    r = dict(dict(enabled=1, scale_error=0.5, thres=1.0, trapped=0, fails=0), **words)
    r.update(new_scale=new_scale, idepth=idepth, idepth_scaled=ids, idepth_zero_scaled=ids.copy(), delta=np.zeros(len(pk), f32),
             world_to_cam_eval=fin["world_to_cam_eval_out"], state=state, state_zero=fin["state_zero_out"], exposure=np.asarray(job["exposure"], f32),
             cam_to_tracking_ref=np.array(ctr, f64), ref_cam_to_world=np.array(ref_c2w, f64), cam_to_world=np.array(Cw[f], f64),
             aff_g2l=(float(state[f, 6]) * sp["scale_a"], float(state[f, 7]) * sp["scale_b"]), calib_value=np.asarray(loop["calib"], f64),
             calib_zero=np.asarray(job["calib_zero"], f64), ad_host=fin["ad_host_out"], ad_target=fin["ad_target_out"], cam=fin["cam_out"],
             c_delta=fin["c_delta_out"], delta_x=fin["delta_x_out"], ad_ht_delta=fin["ad_ht_delta_out"], world_to_cam=np.array(Wc, f64),
             cam_to_world_all=fin["cam_to_world_out"], host=np.asarray(job["host"])[pk], ref=ref, u=np.asarray(job["u"], f32)[pk],
             v=np.asarray(job["v"], f32)[pk])
    r.update({k: fin[k + "_out"] for k in PRE})
    return r


FINISHED = ("scene", "one_frame", "two_frames", "three_frames")
_cache = {}


def scenes():
    """name -> job: every window size and point count of the CPU tests at every scale, the words' cases, and the finished windows"""
    if "scenes" in _cache:
        return _cache["scenes"]
    s = {}
    for n in (1, 2, 3, 8):
        for m in (0, 1, 65):
            s[f"n{n}_p{m}"] = make_scene(seed=10 * n + (m % 7), n_frames=n, n_pts=m, ref=0 if n > 1 else None)
    for k, sc in enumerate(SCALES):
        s[f"scale_{sc}"] = make_scene(seed=40 + k, n_frames=3, n_pts=65, new_scale=sc, ref=1 if k % 2 else None)
    s["rejected"] = make_scene(seed=50, scale_error=2.0)
    s["rejected_nan"] = make_scene(seed=51, scale_error=float("nan"))
    s["rejected_jump"] = make_scene(seed=52, new_scale=1.6, trapped=1)
    s["disabled"] = make_scene(seed=53, enabled=0)
    s["quirk"] = make_scene(seed=54, scale_error=-1.0, new_scale=1.0)
    s["untrap"] = make_scene(seed=55, scale_error=2.0, trapped=1, fails=5)
    for name in FINISHED:
        s["finished_" + name] = finished_scene(name, inside=name != "three_frames")
    _cache["scenes"] = s
    return s


def call_job(job):
    """the job without what the call does not read"""
    return {k: v for k, v in job.items() if k not in ("host", "ref", "u", "v")}


def assert_equal(got, exp, keys=ALL_OUT, what=""):
    """bit for bit; a NaN is compared as a NaN"""
    for k in keys:
        if exp[k] is None:
            continue
        a, b = np.asarray(got[k]), np.asarray(exp[k])
        if a.dtype.kind in "iu" or b.dtype.kind in "iu":
            assert np.array_equal(a.reshape(-1).astype(np.int64), b.reshape(-1).astype(np.int64)), (what, k, a.reshape(-1)[:8], b.reshape(-1)[:8])
            continue
        a, b = a.reshape(-1), b.reshape(-1)
        assert a.dtype == b.dtype, (what, k, a.dtype, b.dtype)
        assert a.shape == b.shape, (what, k, a.shape, b.shape)
        view = np.uint64 if a.dtype == f64 else np.uint32
        nan = np.isnan(a) & np.isnan(b)
        ne = (a.view(view) != b.view(view)) & ~nan
        assert not ne.any(), (what, k, np.argwhere(ne)[:6].ravel(), a[ne][:3], b[ne][:3])


# ---- for tools/rescale_host_standalone.cpp and host/rescale_demo.cpp -------------------------------------------------------------------

def write_case(path, job):
    """The file tools/rescale_host_standalone.cpp reads, a rescale job, through tests/_window_files.py's section writers: int32 nf, n,
    enabled, trapped, fails; float32 scale_error, new_scale, thres; float64 aff_g2l[2]; float32 idepth[n], idepth_scaled[n],
    idepth_zero_scaled[n], delta[n]; float64 world_to_cam_eval[nf 7], state[nf 8], state_zero[nf 8]; float32 exposure[nf]; float64
    cam_to_tracking_ref[7], ref_cam_to_world[7], cam_to_world[7], calib_value[4], calib_zero[4], ad_host[nf nf 64], ad_target[nf nf 64];
    float32 the six tables one after the other, cam[6], c_delta[4]; float64 delta_x[N]; float32 ad_ht_delta[nf nf 8]; float64
    world_to_cam[nf 7], cam_to_world_all[nf 7]."""
    nf, n = np.asarray(job["state"]).reshape(-1, 8).shape[0], len(np.asarray(job["idepth"]).reshape(-1))
    W._write(path, struct.pack("iiiiifffdd", nf, n, int(job["enabled"]), int(job["trapped"]), int(job["fails"]), float(job["scale_error"]),
                               float(job["new_scale"]), float(job["thres"]), float(job["aff_g2l"][0]), float(job["aff_g2l"][1])),
             W._s(job, *POINT), W._d(job, "world_to_cam_eval", "state", "state_zero"), W._s(job, "exposure"),
             W._d(job, "cam_to_tracking_ref", "ref_cam_to_world", "cam_to_world", "calib_value", "calib_zero", "ad_host", "ad_target"),
             W._s(job, *(PRE + ("cam", "c_delta"))), W._d(job, "delta_x"), W._s(job, "ad_ht_delta"), W._d(job, "world_to_cam", "cam_to_world_all"))


def hashes(out):
    """what tools/rescale_host_standalone.cpp prints, from the checker's results"""
    hx = lambda a: f"{W.fnv1a(np.ascontiguousarray(a).tobytes()):016x}"  # noqa: E731
    tables = 0
    for k in PRE:
        tables ^= W.fnv1a(np.ascontiguousarray(out[k], f32).tobytes())
    return dict(decision=int(out["decision"]), trapped=int(out["trapped"]), fails=int(out["fails"]), scale_error=hx(np.array([out["scale_error"]], f32)),
                applied_scale=hx(np.array([out["applied_scale"]], f32)), idepth=hx(np.asarray(out["idepth"], f32)),
                idepth_scaled=hx(np.asarray(out["idepth_scaled"], f32)), idepth_zero_scaled=hx(np.asarray(out["idepth_zero_scaled"], f32)),
                delta=hx(np.asarray(out["delta"], f32)), eval=hx(np.asarray(out["world_to_cam_eval"], f64)), state=hx(np.asarray(out["state"], f64)),
                state_zero=hx(np.asarray(out["state_zero"], f64)), cam_to_tracking_ref=hx(np.asarray(out["cam_to_tracking_ref"], f64)),
                cam_to_world=hx(np.asarray(out["cam_to_world"], f64)), tables=f"{tables:016x}", cam=hx(np.asarray(out["cam"], f32)),
                c_delta=hx(np.asarray(out["c_delta"], f32)), delta_x=hx(np.asarray(out["delta_x"], f64)), ad_ht_delta=hx(np.asarray(out["ad_ht_delta"], f32)),
                world_to_cam=hx(np.asarray(out["world_to_cam"], f64)), cam_to_world_all=hx(np.asarray(out["cam_to_world_all"], f64)))
