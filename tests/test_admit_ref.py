"""CPU: the host form dsm_window_admit_host against the checker tests/_admit_ref.py, A4 against
FrontEndMarginalize.cpp:62-146 line by line on scripted windows whose flags are stated by name, and properties that restate nothing:
cutting the new frame back out returns the inputs, a point of the tracking reference lands in the new frame where the tracked motion
puts it, and the adjoints are -Adj(L0)^T."""
import math

import numpy as np
import pytest

import _admit_ref as AR
import _finish_ref as F
import _step_ref as T
from direct_stereo_slam_amd import admit as AD
from direct_stereo_slam_amd import linearize as LN
from direct_stereo_slam_amd import step as ST
from direct_stereo_slam_amd._lib import DsmError

f32, f64, i32, u8 = np.float32, np.float64, np.int32, np.uint8
U24, U53 = 2.0 ** -24, 2.0 ** -53


def host(job, **kw):
    return AD.window_admit_host([AR.call_job(job)], **kw)[0]


def n_of(job):
    return np.asarray(job["state"]).reshape(-1, 8).shape[0]


# ---- the host form against the checker --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(AR.scenes()))
def test_host_form_equals_checker(name):
    """1, 2, 3, 7 and 15 frames; 0, 1 and 65 points with 0, 1 and several residuals; the optional arrays given and NULL: every output
    bit for bit"""
    job = AR.scenes()[name]
    AR.assert_equal(host(job), AR.admit(job), what=name)


def test_scenes_cover_the_cases():
    s = AR.scenes()
    assert {n_of(j) for j in s.values()} >= {1, 2, 3, 7, 15}
    assert {len(j["host"]) for j in s.values()} >= {0, 1, 65}
    assert {j["H_M"] is None for j in s.values()} == {True, False}
    runs = np.bincount(s["n7_p65"]["point"], minlength=65)
    assert {0, 1, 3} <= set(runs)
    runs = np.bincount(s["n7_empty_first_last_middle"]["point"], minlength=7)
    assert runs[0] == 0 and runs[-1] == 0 and runs[3] == 0 and runs[4] == 0 and runs[2] == 5
    assert any(AR.admit(j)["n_flagged"] for j in s.values())
    assert {s[k]["H_M"] is None for k in PROPERTY_SCENES} == {True, False}


@pytest.mark.parametrize("name", AR.CHAINS)
def test_second_keyframe_windows_of_the_finish_chain(name):
    job = AR.chain_scene(name)
    assert (np.diff(job["point"]) >= 0).all()
    AR.assert_equal(host(job), AR.admit(job), what=name)


def test_other_parameters():
    job = AR.scenes()["n7_p65"]
    sp = dict(scale_xi_trans=0.25, scale_xi_rot=2.0, scale_a=5.0, scale_b=100.0)
    ap = dict(min_frames=2, max_frames=4, min_frame_age=2, min_points_remaining=0.6, max_log_aff_fac_in_window=0.01)
    got = host(job, lp=LN.default_params(scale_idepth=2.0, scale_f=40.0, scale_c=60.0), sp=ST.default_step_params(**sp), ap=AD.default_params(**ap))
    exp = AR.admit(job, sp=sp, params=dict(scale_idepth=2.0, scale_f=40.0, scale_c=60.0), ap=ap)
    AR.assert_equal(got, exp)
    plain = host(job)
    assert got["pre_KRKiTll"].tobytes() != plain["pre_KRKiTll"].tobytes() and got["flagged"].tobytes() != plain["flagged"].tobytes()


def test_defaults_are_the_recalled_settings():
    p = AD.default_params()
    assert (p.min_frames, p.max_frames, p.min_frame_age) == (5, 7, 1)
    assert f32(p.min_points_remaining) == f32(0.05) and f32(p.max_log_aff_fac_in_window) == f32(0.7)
    job = AR.scenes()["n7_p1"]
    AR.assert_equal(host(job, ap=p), host(job))


def test_in_a_batch_every_job_is_its_single_call():
    names = ["n15_p65", "n1_p0", "n3_p65_bare", "n7_empty_first_last_middle", "n2_p1"]
    jobs = [AR.call_job(AR.scenes()[k]) for k in names]
    for got, job, name in zip(AD.window_admit_host(jobs), jobs, names):
        AR.assert_equal(got, host(job), what=name)


# ---- A4 against the source, line by line ------------------------------------------------------------------------------------------------

class FH:
    """what flagFramesForMarginalization reads of a FrameHessian"""

    def __init__(self, frameID, n_in, n_out, ab_exposure, a, distanceLL):
        self.frameID, self.n_in, self.n_out, self.ab_exposure, self.a, self.distanceLL = frameID, n_in, n_out, ab_exposure, a, distanceLL
        self.flaggedForMarginalization = False


def source_lines(frame_hessians_, setting_minFrames, setting_maxFrames, setting_minFrameAge, setting_minPointsRemaining, setting_maxLogAffFacInWindow):
    """FrontEndMarginalize.cpp:62-146.  fh.distanceLL[t] stands for fh->targetPrecalc[t].distanceLL, fh.a for aff_g2l().a"""
    if setting_minFrameAge > setting_maxFrames:                                                  # :63
        for i in range(setting_maxFrames, len(frame_hessians_)):                                 # :64
            frame_hessians_[i - setting_maxFrames].flaggedForMarginalization = True              # :65-66
        return                                                                                   # :68
    flagged = 0                                                                                  # :71
    for i in range(len(frame_hessians_)):                                                        # :73
        fh = frame_hessians_[i]
        n_in, n_out = fh.n_in, fh.n_out                                                          # :75-77
        back = frame_hessians_[-1]
        eh, et = f32(back.ab_exposure), f32(fh.ab_exposure)                                      # :79-81, fromToVecExposure
        if eh == 0 or et == 0:
            eh = et = f32(1.0)
        refToFh0 = math.exp(fh.a - back.a) * float(et) / float(eh)
        with np.errstate(all="ignore"):
            log_a = abs(float(np.log(f32(refToFh0))))
        if ((f32(n_in) < f32(f32(setting_minPointsRemaining) * f32(n_in + n_out)) or log_a > float(f32(setting_maxLogAffFacInWindow)))  # :83-84
                and len(frame_hessians_) - flagged > setting_minFrames):                         # :85
            fh.flaggedForMarginalization = True                                                  # :95
            flagged += 1                                                                         # :96
    if len(frame_hessians_) - flagged >= setting_maxFrames:                                      # :110
        smallestScore = 1.0                                                                      # :111
        toMarginalize = None                                                                     # :112
        latest = frame_hessians_[-1]                                                             # :113
        for fh in frame_hessians_:                                                               # :115
            if fh.frameID > latest.frameID - setting_minFrameAge or fh.frameID == 0:             # :116-118
                continue
            distScore = 0.0                                                                      # :121
            for t, target in enumerate(frame_hessians_):                                         # :122
                if target.frameID > latest.frameID - setting_minFrameAge + 1 or target is fh:    # :123-125
                    continue
                distScore += 1 / (1e-5 + float(fh.distanceLL[t]))                                # :126
            distScore *= -float(np.sqrt(f32(fh.distanceLL[len(frame_hessians_) - 1])))           # :128
            if distScore < smallestScore:                                                        # :130
                smallestScore = distScore                                                        # :131
                toMarginalize = fh                                                               # :132
        if toMarginalize is not None:                                                            # stated: the source dereferences null here
            toMarginalize.flaggedForMarginalization = True                                       # :138


FLAGS = AR.flag_script()


@pytest.mark.parametrize("what,job,ap,expected", FLAGS, ids=[f[0] for f in FLAGS])
def test_flags_by_name_and_against_the_source(what, job, ap, expected):
    """the window's geometry is translations alone, so the source's inputs follow from the scene without any of the code under test:
    distanceLL = |c_h - c_t| rounded to float, a = 10 state[6]"""
    n = n_of(job)
    c = -np.asarray(job["world_to_cam_eval"], f64).reshape(n, 7)[:, 4:]
    dist = [[f32(math.sqrt((c[h][0] - c[t][0]) ** 2 + (c[h][1] - c[t][1]) ** 2 + (c[h][2] - c[t][2]) ** 2)) for t in range(n)] for h in range(n)]
    frames = [FH(int(job["keyframe_id"][i]), int(job["n_points_in"][i]), int(job["n_points_out"][i]), job["exposure"][i],
                 float(np.asarray(job["state"]).reshape(n, 8)[i, 6]) * T.SP["scale_a"], dist[i]) for i in range(n)]
    A = dict(AR.AP, **ap)
    source_lines(frames, A["min_frames"], A["max_frames"], A["min_frame_age"], A["min_points_remaining"], A["max_log_aff_fac_in_window"])
    assert [int(fh.flaggedForMarginalization) for fh in frames] == expected, what
    got = host(job, ap=AD.default_params(**ap))
    assert list(got["flagged"]) == expected + [0], what
    assert got["n_flagged"] == sum(expected)
    assert got["distance_ll"].reshape(n + 1, n + 1)[:n, :n].tobytes() == np.array(dist, f32).tobytes()
    AR.assert_equal(got, AR.admit(job, ap=ap), what=what)


def test_flag_scores():
    """dist_score: the candidates' scores where F2 ran, zeros elsewhere; the mirrored frames tie exactly"""
    by = {f[0]: f for f in FLAGS}
    tie = host(by["a tie goes to the first"][1])["dist_score"]
    assert tie[1] == tie[2] < min(tie[0], *tie[3:6]) and tie[6] == 0.0
    assert (host(by["fewer than max_frames frames: no F2"][1])["dist_score"] == 0.0).all()
    assert (host(by["no candidate: the newest is exempt, the rest are keyframe 0"][1])["dist_score"] == 0.0).all()
    exempt = host(by["keyframe_id 0 is exempt"][1])["dist_score"]
    assert exempt[0] == 0.0 and exempt[1] < 0.0


# ---- independent properties -------------------------------------------------------------------------------------------------------------

PROPERTY_SCENES = ("n2_p65", "n3_p65_full", "n7_p65", "n7_empty_first_last_middle", "n15_p1")


@pytest.mark.parametrize("name", PROPERTY_SCENES)
def test_cutting_the_new_frame_out_returns_the_inputs(name):
    """with the index sets _finish_ref.second_job uses for a frame that leaves; the old pairs' tables and adjoints are what
    _finish_ref.tables / adjoint_pair give on the n old frames alone"""
    job = AR.scenes()[name]
    got = host(job)
    n = n_of(job)
    m, N = n + 1, 4 + 8 * n
    stay = list(range(n))
    idx = list(range(4)) + [4 + 8 * f + k for f in stay for k in range(8)]
    for k, w, t in (("world_to_cam_eval", 7, f64), ("state", 8, f64), ("state_zero", 8, f64), ("exposure", 1, f32), ("frame_energy_th", 1, f32), ("keyframe_id", 1, i32)):
        assert got[k].reshape(m, w)[stay].tobytes() == np.ascontiguousarray(job[k], t).tobytes(), k
    if job["H_M"] is not None:
        for k in ("H_M", "H_L"):
            assert got[k].reshape(N + 8, N + 8)[np.ix_(idx, idx)].tobytes() == np.ascontiguousarray(job[k], f64).tobytes(), k
            rest = got[k].reshape(N + 8, N + 8).copy()
            rest[np.ix_(idx, idx)] = 0.0
            assert not rest.any(), k
        for k in ("b_M", "b_L", "prior", "prior_zero"):
            assert got[k][idx].tobytes() == np.ascontiguousarray(job[k], f64).tobytes(), k
        assert not got["b_M"][N:].any() and not got["b_L"][N:].any()
        assert got["prior"][N:].tobytes() == np.asarray(job["new_frame_prior"], f64).tobytes()
        assert got["prior_zero"][N:].tobytes() == np.asarray(job["new_frame_prior_zero"], f64).tobytes()
    else:
        assert not any(k in got for k in AR.GROWN)
    # the residual lists: what is not against the new frame, in the order given
    old = np.flatnonzero(got["target"] != n)
    assert len(old) == len(job["point"]) and got["n_res"] == len(job["point"]) + len(job["host"])
    for k, src in (("point", "point"), ("target", "target"), ("res_state", "state_in"), ("energy", "energy_in"), ("is_new", "is_new")):
        assert got[k][old].tobytes() == np.ascontiguousarray(job[src]).tobytes(), k
    assert np.array_equal(got["res_index"], old)
    new = np.flatnonzero(got["target"] == n)
    assert np.array_equal(got["point"][new], np.arange(len(job["host"]))) and np.array_equal(got["new_res_index"], new)
    assert (np.diff(got["point"]) >= 0).all()
    assert (got["res_state"][new] == AR.IN).all() and (got["energy"][new] == 0).all() and (got["is_new"][new] == 1).all()
    back = -np.ones(got["n_res"] + 1, i32)
    back[old] = np.arange(len(old))
    lr = got["last_res"].reshape(-1, 2)
    assert np.array_equal(lr[:, 0], new) and np.array_equal(back[lr[:, 1]], np.asarray(job["last_res"]).reshape(-1, 2)[:, 0])
    ls = got["last_state"].reshape(-1, 2)
    assert (ls[:, 0] == AR.IN).all() and np.array_equal(ls[:, 1], np.asarray(job["last_state"]).reshape(-1, 2)[:, 0])
    # the old pairs
    sp = T.SP
    ev, state, zero = AR.rows(job["world_to_cam_eval"], 7), AR.rows(job["state"], 8), AR.rows(job["state_zero"], 8)
    Fr = F.frames_at(ev, state, zero, sp)
    pre = F.tables(dict(exposure=job["exposure"]), ev, zero, Fr, [f32(x) for x in got["cam"]], sp)
    for k, w in AD.PRE:
        assert got[k].reshape(m, m, w)[:n, :n].tobytes() == pre[k].tobytes(), k
    AH, AT = got["ad_host"].reshape(m, m, 8, 8), got["ad_target"].reshape(m, m, 8, 8)
    for h in range(n):
        for t in range(n):
            eh, et = F.adjoint_pair(F.adjoint(ev[t], Fr["Ei"][h]), F.aff_a0(Fr["aff0"][h], Fr["aff0"][t], job["exposure"][h], job["exposure"][t]), sp)
            assert AH[h, t].tobytes() == np.array(eh, f64).tobytes() and AT[h, t].tobytes() == np.array(et, f64).tobytes(), (h, t)
    assert got["frame_prior"].tobytes() == np.asarray(job["new_frame_prior"], f64).tobytes()
    assert np.array_equal(got["frame_delta_prior"], got["state"].reshape(m, 8)[n] - np.asarray(job["new_frame_prior_zero"], f64))


def quat_rot(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def test_points_of_the_tracking_reference_land_where_the_tracked_motion_puts_them():
    """The tracking reference r is a window frame with no pose state and eval[r] = ref_cam_to_world^-1, so the motion from r into the
    new frame is cam_to_tracking_ref^-1.  The pixel from the float tables of pair (r, n), dehomogenised in float64, against the direct
    float64 projection K (R x + t d); the bound is test_rescale_ref.py's: 7 float roundings on an entry of K R K^-1, 4.5 on one of K t,
    against the same expressions in exact arithmetic, plus the double composition's error, which is 2^-29 of it"""
    n, r = 7, 3
    job = AR.make_scene(seed=80, n_frames=n, n_pts=64, ref=r)
    got = host(job)
    m = n + 1
    Mx = np.asarray(got["pre_KRKiTll"], f64).reshape(m, m, 3, 3)[r, n]
    Kt = np.asarray(got["pre_KtTll"], f64).reshape(m, m, 3)[r, n]
    cam = np.asarray(got["cam"], f64)
    K = np.array([[cam[0], 0, cam[2]], [0, cam[1], cam[3]], [0, 0, 1]])
    Ki = np.array([[cam[4], 0, -cam[2] * cam[4]], [0, cam[5], -cam[3] * cam[5]], [0, 0, 1]])
    ctr = np.asarray(job["cam_to_tracking_ref"], f64)
    Rm = quat_rot(ctr[:4]).T  # cam_to_tracking_ref^-1
    tm = -Rm @ ctr[4:]
    worst, pts = 0.0, np.flatnonzero(np.asarray(job["host"]) == r)
    assert len(pts) >= 9
    for p in pts:
        x, d = np.array([float(job["u"][p]), float(job["v"][p]), 1.0]), float(job["idepth"][p])
        num = Mx @ x + Kt * d
        ref = K @ (Rm @ (Ki @ x) + tm * d)
        err = 7 * U24 * (np.abs(K) @ np.ones((3, 3)) @ np.abs(Ki) @ np.abs(x)) + 4.5 * U24 * (np.abs(K) @ np.abs(tm)) * abs(d)
        err *= 1.0 + 2.0 ** -20
        assert abs(num[2]) > 100 * err[2]
        pix, pix_ref = num[:2] / num[2], ref[:2] / ref[2]
        bound = (err[:2] + np.abs(pix) * err[2]) / (abs(num[2]) - err[2])
        assert (np.abs(pix - pix_ref) <= bound).all(), (p, pix, pix_ref, bound)
        worst = max(worst, float(np.max(np.abs(pix - pix_ref) / bound)))
    print(f"reprojection into the new frame: worst pixel difference / bound {worst:.3f}")
    assert np.array_equal(got["pre_KRKiTll"].reshape(m, m, 9)[n, n], np.zeros(9, f32))


def test_adjoints_are_minus_adj_transposed():
    """ad_host[h][t]'s pose block is -Adj(L0)^T with row k scaled by the state's scale, L0 = eval_t eval_h^-1 recomputed in numpy
    float64 from the OUTPUT evaluation poses.  Bound: an entry of Adj is an entry of R (about 12 double roundings through the
    quaternion product, its normalisation and the rotation matrix, |entry| <= 1) or of t^ R (3 products and 2 sums of entries of
    size |t|, t itself from a rotation and a sum: 16 roundings of |t| in all): (12 + 16 |t|) 2^-53, on both sides"""
    job = AR.scenes()["n7_p65"]
    got = host(job)
    m = 8
    ev = got["world_to_cam_eval"].reshape(m, 7)
    sc = np.array(F.scales(T.SP)[:6])
    AH, AT = got["ad_host"].reshape(m, m, 8, 8), got["ad_target"].reshape(m, m, 8, 8)
    worst = 0.0
    for h in range(m):
        for t in range(m):
            Rh, Rt = quat_rot(ev[h, :4]), quat_rot(ev[t, :4])
            R0 = Rt @ Rh.T
            t0 = ev[t, 4:] - R0 @ ev[h, 4:]
            hat = np.array([[0, -t0[2], t0[1]], [t0[2], 0, -t0[0]], [-t0[1], t0[0], 0]])
            Adj = np.block([[R0, hat @ R0], [np.zeros((3, 3)), R0]])
            exp = -Adj.T * sc[:, None]
            bound = 2 * (12 + 16 * float(np.abs(t0).max() + np.abs(ev[h, 4:]).max())) * U53 * sc.max()
            diff = float(np.abs(AH[h, t][:6, :6] - exp).max())
            assert diff <= bound, (h, t, diff, bound)
            worst = max(worst, diff / bound)
            assert np.array_equal(AT[h, t][:6, :6], np.diag(sc)) and not AH[h, t][:6, 6:].any() and not AH[h, t][6:, :6].any()
    print(f"ad_host against -Adj(L0)^T in float64: worst difference / bound {worst:.3f}")


# ---- V --------------------------------------------------------------------------------------------------------------------------------

def refusals():
    job = AR.call_job(AR.make_scene(seed=90, n_frames=3, n_pts=5, counts=(2, 1, 0)))
    n, n_pts, n_res = 3, 5, len(job["point"])
    ins = [k for k, _, _ in AD.inputs(n, n_pts, n_res) if k not in AD.OPTIONAL]
    outs = [o for o, _, _ in AD.outputs(n, n_pts, n_res) if o != "distance_ll_out"] + list(AD.WORDS)
    for k in ins + outs:
        yield "NULL " + k, dict(job, drop=k), {}
    yield "prior without prior_zero", dict(job, drop="prior_zero"), {}
    yield "prior_zero without prior", dict(job, drop="prior"), {}
    for v in (0, 16, 17, -1):
        yield f"n_frames {v}", dict(job, n_frames=v), {}
    yield "n_pts -1", dict(job, n_pts=-1), {}
    yield "n_res -1", dict(job, n_res=-1), {}
    floats = [k for k, t, _ in AD.inputs(n, n_pts, n_res) if t in (f32, f64)]
    for k in floats:
        for bad in (float("nan"), float("inf")):
            a = np.array(job[k], copy=True).astype(f64 if np.asarray(job[k]).dtype == f64 else f32)
            a.reshape(-1)[-1] = bad
            yield f"{bad} in {k}", dict(job, **{k: a}), {}
    for k in ("new_exposure", "new_frame_energy_th"):
        yield "nan " + k, dict(job, **{k: float("nan")}), {}
    yield "nan aff_g2l", dict(job, aff_g2l=(0.0, float("nan"))), {}
    for k in ("world_to_cam_eval", "cam_to_tracking_ref", "ref_cam_to_world"):
        a = np.array(job[k], f64, copy=True).reshape(-1, 7)
        a[-1, :4] *= 1.0 + 1e-8
        yield "a quaternion off the sphere in " + k, dict(job, **{k: a}), {}

    def with_entry(k, i, v):
        a = np.array(job[k], copy=True)
        a.reshape(-1)[i] = v
        return dict(job, **{k: a})

    yield "host out of range", with_entry("host", 1, 3), {}
    yield "host negative", with_entry("host", 1, -1), {}
    yield "point out of range", with_entry("point", n_res - 1, 5), {}
    yield "target out of range", with_entry("target", 0, 3), {}
    yield "target equal to the host", with_entry("target", 0, int(job["host"][job["point"][0]])), {}
    yield "residuals not grouped", with_entry("point", 0, 1), {}
    yield "last_res out of range", with_entry("last_res", 0, n_res), {}
    yield "last_res below -1", with_entry("last_res", 0, -2), {}
    yield "last_res of another point", with_entry("last_res", 0, n_res - 1), {}
    yield "last_state that is no state", with_entry("last_state", 3, 3), {}
    yield "state_in that is no state", with_entry("state_in", 1, 255), {}
    yield "negative n_points_in", with_entry("n_points_in", 0, -1), {}
    yield "negative n_points_out", with_entry("n_points_out", 2, -1), {}
    yield "n_points_in + n_points_out overflows", dict(with_entry("n_points_in", 1, 2 ** 31 - 1), n_points_out=np.array([1, 1, 1], i32)), {}
    for k in ("scale_xi_trans", "scale_a"):
        for v in (float("nan"), 0.0):
            yield f"{k} {v}", job, dict(sp=ST.default_step_params(**{k: v}))
    for k in ("min_points_remaining", "max_log_aff_fac_in_window"):
        for v in (float("nan"), float("inf")):
            yield f"{k} {v}", job, dict(ap=AD.default_params(**{k: v}))
    yield "min_frames -1", job, dict(ap=AD.default_params(min_frames=-1))
    yield "max_frames -1", job, dict(ap=AD.default_params(max_frames=-1))


REFUSALS = list(refusals())


def untouched(b):
    for out in b.all_outputs():
        for k, v in out.items():
            fill = AD.FILL if v.dtype in (f32, f64) else AD.FILL_INT
            assert (v == v.dtype.type(fill)).all(), k


@pytest.mark.parametrize("what,job,kw", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_touch_nothing(what, job, kw):
    """alone, and as the second job of a call whose first job is valid: all or nothing"""
    good = AR.call_job(AR.make_scene(seed=91, n_frames=2, n_pts=4))
    for jobs in ([job], [good, job]):
        b = AD.AdmitBatch(jobs)
        with pytest.raises(DsmError):
            b.run_host(**kw)
        untouched(b)


def test_valid_edges():
    """no points, no residuals, a one-frame window, the optional arrays absent one by one, distance_ll_out NULL, 15 frames"""
    s = AR.scenes()
    assert host(s["n1_p0"])["n_res"] == 0
    assert host(s["n15_p65"])["state"].shape == (16 * 8,)
    job = AR.call_job(s["n3_p65_full"])
    full = host(job)
    for k in ("H_M", "b_M", "H_L", "b_L"):
        lean = host(dict(job, **{k: None}))
        assert k not in lean
        AR.assert_equal(lean, full, keys=[x for x in AR.ALL_OUT if x != k])
    lean = host(dict(job, distances=False))
    assert "distance_ll" not in lean
    AR.assert_equal(lean, full, keys=[x for x in AR.ALL_OUT if x != "distance_ll"])
