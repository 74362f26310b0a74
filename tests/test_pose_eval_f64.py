"""The loop-closure pose evaluation (MODE == 2 of the Gauss-Newton evaluation loop: PoseEstimator::calcRes + calcGSSSE,
PoseEstimator.cpp:84-296 -- what dsm_pose_estimator_estimate and dsm_pose_estimate_batch run at every LM step) against the exact sums of
tests/_gn_f64.py (pose2_ref on oracle/numpy_ref.NumpyPoseEstimator, pinned bit for bit to the C oracle), entry by entry, with the
assertions of tests/_gn_checks.py (the flow indicators compared column by column) and K_FORM2 = 19 as derived in _gn_f64's docstring.

dsm_diag_pose_estimator_eval loads the inputs with dsm_pose_estimator_estimate's own loading function and runs ONE evaluation through
the direct calls' preparation and reduction (LM_OP_SINGLE_PREP / _FINISH in mode 2) with the middle launch chosen:
  form 0  eval_kernel<2, LVL0, false, 0>: the kernel the estimator's LM run launches (levels >= 1: the one-point loop, at P = 16 over
          several chunks when the point set is large -- every level holds the same n_pts);
  form 1  the split pair eval_kernel<2, .., ROSEL 1> then <.., ROSEL 2>;
  form 3  the chains' one-chunk form (diag_chain_eval_kernel<2>: chain_kernel<2>'s two eval_chunk instantiations under its register
          budget; levels >= 1: the two-point loop) -- where n_pts is at most one chunk under the estimator's table.
Form 2 (the tick engine) has no mode-2 instantiation.  Each form full and residual-only, under the three chunk tables.

Bit equalities, by the reasoning of tests/test_eval_forms_f64.py's docstring (the forms share eval_chunk_impl's per-thread order of
stage_b calls, its reduction and LM_OP_SINGLE_FINISH; the two-point loop's masked extra point adds exact zeros; mode 2 changes stage_a
and the flow pass, not the order of anything): every form's full evaluation is bit for bit form 0's on every level; a residual-only
evaluation's rs is bit for bit the full one's, with the same warped count and H, b exactly zero.  With no usable point 1 / n is
infinite and H, b are not compared.

Figures of one MI355X run are in DESIGN.md section 4.4a."""
import ctypes as C

import numpy as np
import pytest

import _gn_checks as K
import _gn_f64 as G
import _pose_eval as PE
from _gn_checks import TABLES
from _scenes import regrad
from direct_stereo_slam_amd import synth as S
from oracle import numpy_ref as N

pytestmark = pytest.mark.gpu

FORMS = (0, 1, 3)
WORST = {}  # (form, residual_only, table, entry class) -> worst err / bound
CALLS = {}  # (form, residual_only, table) -> evaluations checked


@pytest.fixture(scope="module", autouse=True)
def report_worst():
    yield
    classes = ("diag", "offdiag", "b", "E", "flow")
    print("\nmode 2: worst err / bound per form, residual_only, chunk table and entry class (evaluations checked)")
    for f in FORMS:
        for ro in (0, 1):
            for t in TABLES:
                print(f"  form {f} ro {ro} table {t}: " + "  ".join(f"{c} {WORST.get((f, ro, t, c), float('nan')):.4f}" for c in classes) +
                      f"  ({CALLS.get((f, ro, t), 0)})")


@pytest.fixture(scope="module")
def estimators(ctx):
    """(w, h, nlevels) -> one PoseEstimator per chunk table"""
    from direct_stereo_slam_amd.tracker import PoseEstimator, default_params

    made = {}

    def get(w, h, nl):
        if (w, h, nl) not in made:
            pes = []
            for t in TABLES:
                p = default_params()
                p.chunk_geometry = t
                pes.append(PoseEstimator(ctx, w, h, nl, p))
            made[(w, h, nl)] = pes
        return made[(w, h, nl)]

    yield get
    for pes in made.values():
        for pe in pes:
            pe.close()


def _note(form, ro, table):
    CALLS[(form, ro, table)] = CALLS.get((form, ro, table), 0) + 1
    return lambda cls, err, bnd: K.note_worst(WORST, (form, ro, table, cls), err, bnd)


def _bits(out):
    """the outputs of an evaluation as bytes: equal exactly when every value has the same bits (NaNs and signed zeros included)"""
    return b"".join(np.ascontiguousarray(a).tobytes() for a in out)


def forms_of(n, table):
    """the forms that apply to n points under a chunk table: 3 where they are at most one chunk"""
    return FORMS if G.reduction_geometry(n, table)[2] <= 1 else FORMS[:2]


def check_forms(estimators, inp, npe, lvl, pose, aff, cutoff, where=""):
    """one evaluation of `inp` in every form, full and residual-only, under the three tables; returns the reference"""
    ref = G.pose2_ref(npe, lvl, PE.matrix(pose), aff, cutoff)
    n = ref["n_tpl"]
    for table, pe in zip(TABLES, estimators(inp.w, inp.h, inp.nl)):
        dev = pe.load_args(*inp.args())
        P = G.pts_per_thread(n, table)
        form0 = None
        for form in forms_of(n, table):
            w = (where, "form", form, "lvl", lvl, "table", table, "n", n, list(pose), list(aff), cutoff)
            full = pe.diagEval(dev, lvl, pose, aff, cutoff, form=form, residual_only=False)
            K.check_pose_outputs(full, ref, P, w + ("full",), _note(form, 0, table))
            if form == 0:
                form0 = full
            else:
                assert _bits(full) == _bits(form0), ("not bit-identical to form 0", w, full, form0)
            ro = pe.diagEval(dev, lvl, pose, aff, cutoff, form=form, residual_only=True)
            w = w + ("residual-only",)
            K.common_checks(ro[0], ro[3], ref, P, w, _note(form, 1, table))
            assert _bits(ro[:1]) == _bits(full[:1]), ("rs differs from the full evaluation's", w, ro[0], full[0])
            if ro[3] > 0:
                assert np.all(ro[1] == 0) and np.all(ro[2] == 0), ("normal equations of a residual-only evaluation", w, ro[1:3])
    return ref


# ---- chunk edges ------------------------------------------------------------------------------------------------------------
SWEEP = [1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 8193, 16383, 16384, 16385]


def test_chunk_edge_sweep_every_level(estimators):
    """308 x 92, three levels, the first n of 16 385 points for every n of SWEEP on EVERY level at the true pose: the same n on level 2
    is P = 16 in the one-point loop with a one-point last chunk (n = 4097, 8193), which mode 0 never produces"""
    whole = PE.scene_inputs("small", 84, SWEEP[-1])
    seen = {t: set() for t in TABLES}
    one_chunk = {t: 0 for t in TABLES}
    usable = 0
    for n in SWEEP:
        inp = whole.cut(n)
        npe = PE.numpy_estimator(inp)
        for t in TABLES:
            seen[t].add(G.pts_per_thread(n, t))
            one_chunk[t] += 3 in forms_of(n, t)
        for lvl in range(inp.nl):
            ref = check_forms(estimators, inp, npe, lvl, inp.sc.gt_pose, [0.0, 0.0], 20.0, where=f"n={n}")
            assert n < 63 or 4 * ref["n4"] >= n, ("a quarter of the points usable", n, lvl, ref["n4"])
            usable += ref["n4"]
    assert seen == {0: {1, 2, 4, 8, 16}, 1: {1, 2, 4}, 2: {1, 2, 4, 8, 16}}, seen  # every points-per-thread value these sizes reach
    assert one_chunk == {0: 19, 1: 7, 2: 19}, one_chunk  # form 3 ran: n <= 4096 (tables 0, 2), n <= 256 (the latency table)
    assert usable > 0


def test_chunk_edges_65536(estimators):
    """616 x 184: 65 536 -+ 1 points (the latency table's P = 8 edge) on level 0 and on the coarsest level (77 x 23 texels)"""
    whole = PE.scene_inputs("medium", 85, 65537)
    seen = set()
    for n in (65535, 65536, 65537):
        inp = whole.cut(n)
        npe = PE.numpy_estimator(inp)
        seen.add(G.pts_per_thread(n, 1))
        for lvl in (0, inp.nl - 1):
            ref = check_forms(estimators, inp, npe, lvl, inp.sc.gt_pose, [0.0, 0.0], 20.0, where=f"n={n}")
            assert 4 * ref["n4"] >= n, (n, lvl, ref["n4"])
    assert seen == {4, 8}, seen


# ---- every level, three poses --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,seed,photo", [("tiny", 81, None), ("small", 82, None), ("small", 83, (0.05, 4.0, 0.8, 1.3))])
def test_every_level_three_poses(estimators, size, seed, photo):
    """identity, the true pose and three times its motion at cut-offs 20 and 5 on every level; `photo` = (a, b, reference exposure, new
    exposure): a frame rendered with the brightness map AffLight::fromToVecExposure gives for that affine pair and those exposures
    (1.7 I + 4), evaluated at the pair"""
    a, b, ref_exp, new_exp = photo if photo else (0.0, 0.0, 1.0, 1.0)
    inp = PE.scene_inputs(size, seed, 1500, aff=(a, b), ref_exposure=ref_exp, new_exposure=new_exp)
    npe = PE.numpy_estimator(inp)
    affs = [[a, b]]
    oob = sat = 0
    for lvl in range(inp.nl):
        for pose in PE.three_poses(inp.sc):
            for aff in affs:
                for cutoff in (20.0, 5.0):
                    ref = check_forms(estimators, inp, npe, lvl, pose, aff, cutoff, where=size)
                    # the sweep tests something: on the reference alone
                    assert cutoff != 20.0 or 4 * ref["n4"] >= ref["n_tpl"], ("a quarter of the points usable", lvl, list(pose), aff, ref["n4"])
                    oob += ref["n_tpl"] - ref["n_terms"]
                    sat += ref["n_sat"]
    assert oob > 0 and sat > 0, (oob, sat)


def test_more_points_than_pixels(estimators):
    """154 x 46 with 4000 points: level 1 has 1771 texels, so several points land on one texel and n_pts exceeds the level's size"""
    inp = PE.scene_inputs("tiny", 86, 4000)
    assert len(inp.xyz) > (inp.w >> 1) * (inp.h >> 1)
    npe = PE.numpy_estimator(inp)
    for lvl in range(inp.nl):
        ref = check_forms(estimators, inp, npe, lvl, inp.sc.gt_pose, [0.0, 0.0], 20.0, where="4000 on tiny")
        assert 4 * ref["n4"] >= ref["n_tpl"]


# ---- operand-range edges of stage_a's shared-reciprocal quotients ---------------------------------------------------------------
def back_project(inp, pose, Ku, Kv, pt2):
    """the point (float64) that the pose warps to depth pt2 at level-0 pixel (Ku, Kv)"""
    fx, fy, cx, cy = (float(v) for v in inp.K)
    T = PE.matrix(pose)
    p = np.array([(Ku - cx) / fx * pt2, (Kv - cy) / fy * pt2, pt2], np.float64)
    return T[:3, :3].T @ (p - T[:3, 3])


def colours_from_target(inp, pose, where):
    """`inp` with the colours of the points `where` set, level by level, to the target's own intensity at their projection plus one
    grey level -- so that they are usable wherever they are inside the image"""
    npe = PE.numpy_estimator(inp)
    cols = [c.copy() for c in inp.cols]
    for lvl in range(inp.nl):
        npe.calc_res(lvl, PE.matrix(pose), [0.0, 0.0], 20.0)
        Ku, Kv = npe.warp["Ku"][where], npe.warp["Kv"][where]
        with np.errstate(invalid="ignore"):
            ok = (Ku > 2) & (Kv > 2) & (Ku < npe.w[lvl] - 3) & (Kv < npe.h[lvl] - 3)
        cols[lvl][where[ok]] = N.interp33(npe.new_dIp[lvl], Ku[ok], Kv[ok])[:, 0] + np.float32(1)
    return inp.with_points(inp.xyz, cols)


def depth_class(v):
    """which path of stage_a a warped depth takes: 0 behind the camera, 1 below 2^-33 (IEEE), 2 ordinary, 3 from 2^32 up (IEEE)"""
    return 0 if v <= 0 else 1 if v < 2.0 ** -33 else 2 if v < 2.0 ** 32 else 3


BELOW_2_32 = float(np.nextafter(np.float32(2.0 ** 32), np.float32(0)))
# (warped depth, poses it is placed under): the tiny depths need t = 0 -- with a translation the float32 narrowing of the point swamps 1e-11
DEPTHS = [(2.0 ** -34, "id rot"), (2.0 ** -33, "id rot"), (BELOW_2_32, "id rot gt"), (2.0 ** 32, "id rot gt"), (1e10, "id rot gt"), (-1.0, "id rot gt")]


@pytest.mark.parametrize("depth,poses", DEPTHS, ids=["2^-34", "2^-33", "below_2^32", "2^32", "1e10", "behind"])
def test_stage_a_operand_range(estimators, depth, poses):
    """a point of chosen warped depth (a) alone in a wave of ordinary points -- the whole wave then takes the IEEE divisions because of one
    lane -- and (b) as 64 consecutive indices, at the identity (where pt2 is the narrowed z exactly), under a pure rotation and, for the
    depths a translation does not swamp, at the true pose.  At the identity the float32 pt2 is exactly the chosen value; elsewhere the
    rotation rounds it, so the depth is moved a little into its class (x 1.5 or x 0.75) and the class is confirmed on the reference."""
    base = PE.scene_inputs("small", 87, 512)
    sc = base.sc
    rot = np.concatenate([sc.gt_pose[:4], np.zeros(3)])
    rng = np.random.default_rng(5)
    for name, pose in (("id", S.IDENTITY_POSE), ("rot", rot), ("gt", sc.gt_pose)):
        if name not in poses.split():
            continue
        d = depth
        if name != "id" and depth > 0:  # off the edge, inside the class
            d = depth * (0.75 if depth_class(depth * 0.75) == depth_class(depth) else 1.5)
            assert depth_class(d) == depth_class(depth)
        for placing, where in (("one lane", np.array([70])), ("a wave", np.arange(128, 192))):
            xyz = base.xyz.copy()
            for i in where:
                xyz[i] = back_project(base, pose, rng.uniform(20, sc.w - 20), rng.uniform(20, sc.h - 20), d)
            inp = colours_from_target(base.with_points(xyz), pose, where)
            npe = PE.numpy_estimator(inp)
            for lvl in range(inp.nl):
                ref = check_forms(estimators, inp, npe, lvl, pose, [0.0, 0.0], 20.0, where=f"pt2={depth} {name} {placing}")
                got = npe.warp["pt2"][where]
                if name == "id":
                    assert np.all(got == np.float32(depth)), (got, depth)
                assert all(depth_class(float(g)) == depth_class(depth) for g in got), (got, depth)
                if lvl == 0 and depth > 0:  # the placed points count: they are in the image with a small residual
                    assert np.all(np.isin(where, ref["idx"])), ("placed points usable", name, placing, np.setdiff1d(where, ref["idx"]))
                if depth <= 0:
                    assert not np.any(np.isin(where, ref["idx"]))


# ---- reference-side edges ---------------------------------------------------------------------------------------------------
def test_reference_side_edges(estimators):
    """z < 0, z = 0, a NaN coordinate and a double that narrows to inf -- away from the flow indices (finite flow indicators: within the
    bound) and at flow indices i % 32 == 0 (the SAME non-finite value on both sides); a pose with t2 = 1 exactly (1 - t2 = 0 in the flow
    pass); NaN / inf texels in the target with the gradients re-formed"""
    base = PE.scene_inputs("small", 88, 512)
    sc = base.sc
    gt = np.asarray(sc.gt_pose, np.float64)

    def edited(edits):
        xyz = base.xyz.copy()
        for i, f in edits:
            xyz[i] = f(xyz[i])
        return base.with_points(xyz)

    neg = lambda p: -p
    z0 = lambda p: np.array([p[0], p[1], 0.0])
    nan = lambda p: np.array([np.nan, p[1], p[2]])
    inf = lambda p: np.array([1e39, p[1], p[2]])
    cases = [("off the flow indices", edited([(10, neg), (33, z0), (40, nan), (41, inf), (300, lambda p: np.array([p[0], np.nan, p[2]]))]), True),
             ("z = 0 at a flow index", edited([(32, z0), (33, z0)]), False),
             ("z < 0 and origin at flow indices", edited([(64, neg), (96, lambda p: np.zeros(3))]), None),
             ("NaN at a flow index", edited([(128, nan)]), False),
             ("inf at a flow index", edited([(160, inf)]), False)]
    for name, inp, finite in cases:
        npe = PE.numpy_estimator(inp)
        for lvl in range(inp.nl):
            for pose in (S.IDENTITY_POSE, gt):
                ref = check_forms(estimators, inp, npe, lvl, pose, [0.0, 0.0], 20.0, where=name)
                if lvl == 0 and finite is not None:
                    assert bool(np.all(np.isfinite(ref["flow64"]))) == finite, (name, ref["flow64"])
                assert ref["n4"] > 100
    # t2 = 1 exactly: (x - t0) / (1 - t2) divides by zero at every flow point
    npe = PE.numpy_estimator(base)
    for pose in (np.concatenate([gt[:6], [1.0]]), np.concatenate([S.IDENTITY_POSE[:4], [0.0, 0.0, 1.0]])):
        ref = check_forms(estimators, base, npe, 0, pose, [0.0, 0.0], 20.0, where="t2 = 1")
        assert not np.isfinite(ref["flow64"][0]) and ref["n_terms"] > 0, (ref["flow64"], ref["n_terms"])
    # non-finite texels, as tests/_gn_checks.py edge_scene plants them
    dIp = [a.copy() for a in sc.new_p]
    dIp[0][40:44, 100:140, 0] = np.nan
    dIp[0][50, 60:70, 0] = np.inf
    dIp[0] = regrad(dIp[0])
    inp = PE.PoseInputs(sc, base.xyz, base.cols, dIp=dIp)
    npe = PE.numpy_estimator(inp)
    clean = G.residual2_ref(PE.numpy_estimator(base), 0, PE.matrix(gt), [0.0, 0.0], 20.0)
    for pose in (S.IDENTITY_POSE, gt):
        ref = check_forms(estimators, inp, npe, 0, pose, [0.0, 0.0], 20.0, where="NaN / inf texels")
    assert 0 < ref["n_terms"] < clean["n_terms"], "some points gather a non-finite intensity"


def test_empty_evaluation(estimators):
    """every point outside the image: rs[5] is NaN, E = 0 (common_checks), H and b are not compared"""
    inp = PE.scene_inputs("small", 88, 512)
    npe = PE.numpy_estimator(inp)
    far = S.pose_from_Rt(np.eye(3), [50.0, 0, 0])
    for lvl in range(inp.nl):
        ref = check_forms(estimators, inp, npe, lvl, far, [0.0, 0.0], 20.0, where="empty")
        assert ref["n_terms"] == 0 and ref["n4"] == 0


# ---- form 0 is what production runs ------------------------------------------------------------------------------------------
def test_form0_is_the_estimators_own_evaluation(ctx):
    """An estimator whose max_iterations are all zero ends its LM run at each level's first evaluation (the cut-off doubled while more
    than 0.6 of the terms saturate, PoseEstimator.cpp:337-345), so dsm_pose_estimator_estimate / dsm_pose_estimate_batch report
    pose_error = sqrtf(E / numTermsInE), inlier_percent = 100 numTermsInE / n and the ok flag of level 0's evaluation at the guess:
    the same figures from the diag entry's form 0, bit for bit.  Guesses whose quaternion is exact: the identity and a pure translation."""
    from direct_stereo_slam_amd.tracker import PoseBatch, PoseEstimator, default_params

    p = default_params()
    for l in range(len(p.max_iterations)):
        p.max_iterations[l] = 0
    for seed, new_exp in ((82, 1.0), (83, 1.3)):
        inp = PE.scene_inputs("small", seed, 1500, new_exposure=new_exp)
        pe, pb = PoseEstimator(ctx, inp.w, inp.h, inp.nl, p), PoseBatch(ctx, inp.w, inp.h, inp.nl, p)
        dev = pe.load_args(*inp.args())
        for t in (np.zeros(3), np.asarray(inp.sc.gt_pose[4:], np.float64), np.array([0.5, 0.0, 0.0])):
            guess = np.eye(4)
            guess[:3, 3] = t
            pose = np.concatenate([[0.0, 0.0, 0.0, 1.0], t])
            repeat = np.float32(1)
            rs = pe.diagEval(dev, 0, pose, [0.0, 0.0], float(np.float32(20.0) * repeat))[0]
            while rs[5] > 0.6 and repeat < 50:
                repeat = np.float32(repeat * 2)
                rs = pe.diagEval(dev, 0, pose, [0.0, 0.0], float(np.float32(20.0) * repeat))[0]
            err = np.sqrt(np.float32(rs[0] / rs[1]))
            inl = int(np.float32(100) * np.float32(int(rs[1])) / np.float32(len(inp.xyz)))
            ok = bool(err < 10.0 and inl > 90)  # (the affine pair stays (0, 0) and |log(new_exp)| < 1.5: aff_good)
            ok_s, T_s, err_s = pe.estimate(*inp.args(), 0, guess)
            (ok_b, T_b, err_b, inl_b), = pb.estimate_many([dict(pts_xyz=inp.xyz, ref_colors=inp.cols, ref_ab_exposure=inp.ref_exposure, new_dIp=inp.dIp,
                                                               new_ab_exposure=inp.new_exposure, new_cam=inp.K, ref_to_new=guess)], 0)
            assert np.float32(err_s).tobytes() == np.float32(err).tobytes() == np.float32(err_b).tobytes(), (seed, t, err_s, err_b, err, rs)
            assert inl_b == inl and ok_s == ok_b == ok, (seed, t, inl_b, inl, ok_s, ok_b, ok)
            np.testing.assert_array_equal(T_s, guess)
        pe.close()
        pb.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------
def test_bad_arguments_write_nothing(estimators):
    from direct_stereo_slam_amd._lib import c_double_p

    inp = PE.scene_inputs("small", 88, 512)
    pe = estimators(inp.w, inp.h, inp.nl)[1]  # the latency table: 512 points are two chunks
    assert G.reduction_geometry(512, 1)[2] == 2
    keep, dev = pe.load_args(*inp.args())
    pose, aff = np.ascontiguousarray(inp.sc.gt_pose, np.float64), np.zeros(2)
    dp = lambda a: None if a is None else a.ctypes.data_as(c_double_p)
    xyz = dev[1]
    bad = [dict(form=2), dict(form=4), dict(form=-1), dict(form=3), dict(lvl=-1), dict(lvl=inp.nl), dict(pose=None), dict(aff=None), dict(xyz=None)]
    for kw in bad:
        a = dict(form=0, lvl=0, pose=pose, aff=aff, xyz=xyz)
        a.update(kw)
        rs, H, b, n = np.full(6, 7.0), np.full(64, 7.0), np.full(8, 7.0), C.c_int(7)
        rc = pe.L.dsm_diag_pose_estimator_eval(pe.h, dev[0], a["xyz"], *dev[2:], a["lvl"], dp(a["pose"]), dp(a["aff"]), 20.0, a["form"], 0, dp(rs),
                                               dp(H), dp(b), C.byref(n))
        assert rc == -1, (kw, rc)  # DSM_ERR_INVALID
        assert np.all(rs == 7) and np.all(H == 7) and np.all(b == 7) and n.value == 7, kw
    # ... and the handle still evaluates
    ref = G.pose2_ref(PE.numpy_estimator(inp), 0, PE.matrix(pose), [0.0, 0.0], 20.0)
    K.check_pose_outputs(pe.diagEval((keep, dev), 0, pose, [0.0, 0.0], 20.0), ref, G.pts_per_thread(512, 1), "after bad arguments", lambda *a: None)
