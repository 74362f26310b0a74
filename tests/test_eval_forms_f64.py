"""Every FORM of the Gauss-Newton evaluation loop against the exact sums of tests/_gn_f64.py -- what tests/test_normal_equations_f64.py
asserts of the direct calls' kernel alone, asserted of each kernel the loop is compiled into, full and residual-only.

dsm_diag_single_eval runs ONE evaluation through dsm_tracker_calc_res_*'s own preparation and reduction with the middle launch chosen:
  form 0  eval_kernel<MODE, LVL0, false, 0>: the direct calls' kernel (arrival ticket; levels >= 1: the one-point loop, VC = 0);
  form 1  the split pair eval_kernel<.., ROSEL 1> then <.., ROSEL 2> (the residual-only kernel of seven waves per SIMD);
  form 2  tick_eval_kernel<MODE, false>'s item path (workgroup barrier; levels >= 1: the two-point loop, VC = 1);
  form 3  the chains' one-chunk form, the partial in LDS (diag_chain_eval_kernel: chain_kernel's eval_chunk instantiations under its
          register budget) -- levels of at most one chunk under the tracker's table only.
Each with residual_only 0 and 1, under the three chunk tables.

Full evaluations: the assertions of test_normal_equations_f64.py (tests/_gn_checks.py) for every form; form 0 is bit for bit
dsm_tracker_calc_res_pose / _scale, and every other form is bit for bit form 0 -- rs, H, b, h00, h01 -- at EVERY level:
  * the forms share the reduction at the end of eval_chunk_impl (tracker_kernels.hip: row16_sum of wave_ops.hpp, the 16 rows in order) and
    LM_OP_SINGLE_FINISH; the arrival ticket the waves take there hands the same additions in the same order to another wave;
  * on levels >= 1 forms 2 and 3 run eval_chunk_impl's two-point loop (DEEP) where form 0 runs its one-point loop.  Both call stage_b
    for the thread's points k = 0 .. P - 1 in that order, and stage_b is the only place the accumulators, E and the counts are added to.
    The two-point loop's extra call at odd P (P = 1: point k + 1 = P) is masked: `listed(.., false)` is an
    empty lane mask, so every term is an exact zero of either sign added to a sum that is never -0 (stage_b masks the Jacobian's
    inputs, the energy and the weight), which leaves the bits alone.  VC only chooses the register file of loop constants.
  So the per-thread addition order is the same and bit equality is asserted on levels >= 1 as well.

Residual-only evaluations: numTermsInE, the saturated share and the padded warped count equal the reference's -- stage_b counts
n_warped from the same `use` mask whether RO or not, so a residual-only evaluation reports the full evaluation's count; E and
the flow indicators within the bounds; rs bit for bit the full evaluation's of the same form, table and inputs (the intensity is
interpolated by the same four products in the same order from two 8-byte loads instead of four loads: taps_load / taps_interp with
GRAD = false); and every H / b entry, h00 and h01 exactly 0 (eval_chunk_impl's reduction writes a residual-only evaluation's partial
slots as zeros).  With no usable point (n_warped = 0) LM_OP_SINGLE_FINISH's
1 / n is infinite and H, b, h are not compared -- as for full evaluations, where the same holds."""
import ctypes as C

import numpy as np
import pytest

import _gn_checks as K
import _gn_f64 as G
from _gn_checks import TABLES, numpy_tracker, sweep_sizes, three_poses, trackers
from _scenes import _photometry, make_affine_scene, make_scene
from direct_stereo_slam_amd import synth as S
from oracle import numpy_ref as N

pytestmark = pytest.mark.gpu

FORMS = (0, 1, 2, 3)
WORST = {}  # (form, residual_only, table, entry class) -> worst err / bound
CALLS = {}  # (form, residual_only) -> evaluations checked


@pytest.fixture(scope="module", autouse=True)
def report_worst():
    yield
    classes = ("diag", "offdiag", "b", "E", "scale", "flow")
    print("\nworst err / bound per form, residual_only, chunk table and entry class (evaluations checked)")
    for f in FORMS:
        for ro in (0, 1):
            for t in TABLES:
                print(f"  form {f} ro {ro} table {t}: " + "  ".join(f"{c} {WORST.get((f, ro, t, c), float('nan')):.4f}" for c in classes) +
                      f"  ({CALLS.get((f, ro, t), 0)})")


def _note(form, ro, table):
    CALLS[(form, ro, table)] = CALLS.get((form, ro, table), 0) + 1
    return lambda cls, err, bnd: K.note_worst(WORST, (form, ro, table, cls), err, bnd)


def _bits(out):
    """the outputs of an evaluation as bytes: equal exactly when every value has the same bits (NaNs and signed zeros included)"""
    return b"".join(np.ascontiguousarray(a, np.float32 if isinstance(a, float) else None).tobytes() for a in out)


def forms_of(trk, lvl, n_tpl):
    """the forms that apply to a level of n_tpl points under trk's table: 3 where it is at most one chunk"""
    return FORMS if trk.reduction_geometry(lvl, n_tpl)[2] <= 1 else FORMS[:3]


def check_forms(kind, trk, table, ref, lvl, args, cutoff, where=""):
    """one evaluation in every form, full and residual-only; kind 'pose': args = (pose, aff), 'scale': args = (scale,)"""
    pose_kind = kind == "pose"
    direct = trk.calcResPose(lvl, *args, cutoff) if pose_kind else trk.calcResScale(lvl, *args, cutoff)
    run = trk.diagEvalPose if pose_kind else trk.diagEvalScale
    check = K.check_pose_outputs if pose_kind else K.check_scale_outputs
    P = G.pts_per_thread(ref["n_tpl"], table)
    forms = forms_of(trk, lvl, ref["n_tpl"])
    assert 3 in forms or G.reduction_geometry(ref["n_tpl"], table)[2] > 1
    form0 = None
    for form in forms:
        w = (where, kind, "form", form, "lvl", lvl, "table", table, "n", ref["n_tpl"], args, cutoff)
        full = run(lvl, *args, cutoff, form=form, residual_only=False)
        check(full, ref, P, w + ("full",), _note(form, 0, table))
        if form == 0:
            assert _bits(full) == _bits(direct), ("form 0 is not the direct call", w, full, direct)
            form0 = full
        else:
            assert _bits(full) == _bits(form0), ("not bit-identical to form 0", w, full, form0)
        ro = run(lvl, *args, cutoff, form=form, residual_only=True)
        w = w + ("residual-only",)
        K.common_checks(ro[0], ro[3], ref, P, w, _note(form, 1, table))
        assert _bits(ro[:1]) == _bits(full[:1]), ("rs differs from the full evaluation's", w, ro[0], full[0])
        if ro[3] > 0:
            assert np.all(np.asarray(ro[1]) == 0) and np.all(np.asarray(ro[2]) == 0), ("normal equations of a residual-only evaluation", w, ro[1:3])


def sweep_scene(ctx, sc, levels, poses, cutoffs=(20.0,), scales=(1.0,), where=""):
    npt, trks = numpy_tracker(sc), trackers(ctx, sc)
    for lvl in levels:
        for pose, aff in poses:
            for cutoff in cutoffs:
                ref = G.pose_ref(npt, lvl, N.pose_to_matrix(np.asarray(pose, np.float64)), aff, cutoff)
                for t, trk in zip(TABLES, trks):
                    check_forms("pose", trk, t, ref, lvl, (pose, aff), cutoff, where)
        for scale in scales:
            for cutoff in cutoffs:
                ref = G.scale_ref(npt, lvl, scale, cutoff)
                for t, trk in zip(TABLES, trks):
                    check_forms("scale", trk, t, ref, lvl, (scale,), cutoff, where)
    for trk in trks:
        trk.close()


@pytest.mark.parametrize("size,template", [("tiny", "dense"), ("odd", "dense"), ("mini4", "dense"), ("small", "sparse")])
def test_every_level(ctx, size, template):
    sc = make_scene(size, seed=11, template=template, n0=3000)
    sweep_scene(ctx, sc, range(sc.nl), three_poses(sc), cutoffs=(20.0, 5.0), scales=(1.0, 0.8), where=size)


def test_six_level_config_full_size(ctx):
    sc = make_scene("kitti6", seed=0x5EED0000, noise=2.0)
    sweep_scene(ctx, sc, (0, 3, 5), three_poses(sc), cutoffs=(20.0, 5.0), where="kitti6")


def test_affine_case(ctx):
    """a keyframe with its own affine brightness and another exposure time than the new frame's"""
    from test_parity_tracker import AFFINE_CASES

    sc = make_affine_scene("small", seed=31, **AFFINE_CASES["dark_keyframe_longer_exposure"])
    poses = [(p, a) for p in (S.IDENTITY_POSE, sc.gt_pose) for a in (list(sc.ref_aff), list(sc.gt_aff), [0.0, 0.0])]
    sweep_scene(ctx, sc, range(sc.nl), poses, where="dark_keyframe_longer_exposure")


def test_edge_inputs(ctx):
    """test_normal_equations_f64.test_edge_inputs' inputs: ragged sizes, an empty level, a single point, NaN / inf texels, NaN /
    negative / zero inverse depths; then every point outside the image and every residual saturated"""
    sc = K.edge_scene()
    sweep_scene(ctx, sc, range(sc.nl), [(sc.gt_pose, list(sc.gt_aff))], where="edge")
    far = S.pose_from_Rt(np.eye(3), [50.0, 0, 0])
    sweep_scene(ctx, sc, (0,), [(far, [0.0, 0.0]), (sc.gt_pose, [0.0, 200.0])], scales=(), where="edge")


def edge_sweep(ctx, lvl, expect_ppt):
    """level `lvl` of the dense KITTI template cut to every count of sweep_sizes() that it holds, and whole; both problem kinds, every
    form, under the three chunk tables.  expect_ppt[t]: the points-per-thread values table t must have been seen at."""
    sc = make_scene("kitti", seed=21)
    full = len(sc.tpl[0][lvl])
    ns = [n for n in sweep_sizes() if n < full] + [full]
    # the template's first rows leave the image under the true motion -- not one of the first 513 points of level 0 is usable -- so the small
    # counts (where a level is ONE chunk: form 3) are cut from the middle of the level as well
    npt, trks = numpy_tracker(sc), trackers(ctx, sc)
    pose_T = N.pose_to_matrix(np.asarray(sc.gt_pose, np.float64))
    both = np.intersect1d(G.pose_ref(npt, lvl, pose_T, list(sc.gt_aff), 20.0)["idx"], G.scale_ref(npt, lvl, 1.0, 20.0)["idx"])
    mid = int(both[np.searchsorted(both, full // 2)])  # the first point of the level's second half that both problem kinds can use
    cuts = [(0, n) for n in ns] + [(mid, n) for n in ns if n <= 4097]
    ref_aff, ref_exp, _ = _photometry(sc)
    seen = {t: set() for t in TABLES}
    one_chunk = {t: 0 for t in TABLES}
    usable_small = 0
    for start, n in cuts:
        tpl = [[a[l][start:start + n].copy() if l == lvl else a[l] for l in range(sc.nl)] for a in sc.tpl]
        npt.set_ref(ref_aff[0], ref_aff[1], ref_exp, *tpl)
        for t, trk in zip(TABLES, trks):
            trk.setCoarseTrackingRef(0, ref_aff, ref_exp, *tpl)
            assert trk.reduction_geometry(lvl, n) == G.reduction_geometry(n, t), (n, t)
            seen[t].add(G.pts_per_thread(n, t))
            one_chunk[t] += len(forms_of(trk, lvl, n)) == 4
        ref = G.pose_ref(npt, lvl, pose_T, list(sc.gt_aff), 20.0)
        sref = G.scale_ref(npt, lvl, 1.0, 20.0)
        usable_small += n <= 256 and ref["n4"] > 0 and sref["n4"] > 0
        for t, trk in zip(TABLES, trks):
            check_forms("pose", trk, t, ref, lvl, (sc.gt_pose, list(sc.gt_aff)), 20.0, where=f"n={n} from {start}")
            check_forms("scale", trk, t, sref, lvl, (1.0,), 20.0, where=f"n={n} from {start}")
    for trk in trks:
        trk.close()
    # every points-per-thread value of every table was visited (a changed table cannot skip one silently), and form 3 ran
    assert all(seen[t] == expect_ppt[t] for t in TABLES), seen
    assert all(one_chunk[t] >= 20 for t in TABLES), one_chunk  # (the latency table: n <= 256, ten counts from two places; the others: n <= 4096)
    assert usable_small >= 10, usable_small  # ... on points that count, for both problem kinds, under every table
    return full


def test_chunk_edge_sweep_level0(ctx):
    """test_normal_equations_f64.test_chunk_edge_sweep's inputs (446 992 points cut to every P edge +- 1, to one-point last chunks and
    to a few points) in every form"""
    full = edge_sweep(ctx, 0, {t: {1, 2, 4, 8, 16} for t in TABLES})
    assert full == 446992


def test_chunk_edge_sweep_level1(ctx):
    """the same counts on level 1, as far as it reaches (111 k points): where the tick engine's and the chains' two-point loop stands
    against the direct calls' one-point loop.  (The latency table takes 16 points per thread from 262 144 points up: not on this level.)"""
    full = edge_sweep(ctx, 1, {0: {1, 2, 4, 8, 16}, 1: {1, 2, 4, 8}, 2: {1, 2, 4, 8, 16}})
    assert full > 65537


def test_diagnostic_call_leaves_the_context_usable(ctx):
    """trackNewestCoarse and optimizeScale give the same bits after diagnostic evaluations in every form as before them"""
    sc = make_scene("small", seed=5)
    (trk,) = trackers(ctx, sc)[:1]
    before = trk.trackNewestCoarse(S.IDENTITY_POSE, [0.0, 0.0], sc.nl - 1)
    scale_before = trk.optimizeScale(1.0, sc.nl - 1)
    for lvl in range(sc.nl):
        for form in forms_of(trk, lvl, len(sc.tpl[0][lvl])):
            for ro in (False, True):
                trk.diagEvalPose(lvl, sc.gt_pose, list(sc.gt_aff), 20.0, form=form, residual_only=ro)
                trk.diagEvalScale(lvl, 1.0, 20.0, form=form, residual_only=ro)
        after = trk.trackNewestCoarse(S.IDENTITY_POSE, [0.0, 0.0], sc.nl - 1)
        assert after[0] == before[0] and _bits(after[1:]) == _bits(before[1:]), (lvl, after, before)
        assert _bits(trk.optimizeScale(1.0, sc.nl - 1)) == _bits(scale_before), lvl
    trk.close()


def test_bad_arguments_write_nothing(ctx):
    from direct_stereo_slam_amd._lib import c_double_p

    sc = make_scene("small", seed=5)
    trk = trackers(ctx, sc)[1]  # the latency table: level 0 is many chunks
    assert trk.reduction_geometry(0, len(sc.tpl[0][0]))[2] > 1
    pose, aff = np.ascontiguousarray(sc.gt_pose, np.float64), np.zeros(2)
    dp = lambda a: a.ctypes.data_as(c_double_p)
    for mode, lvl, form in [(2, 0, 0), (-1, 0, 0), (0, -1, 0), (0, sc.nl, 0), (1, sc.nl, 2), (0, 0, 4), (0, 0, -1), (1, 0, 4), (0, 0, 3), (1, 0, 3)]:
        rs, H, b = np.full(6, 7.0), np.full(64, 7.0), np.full(8, 7.0)
        hs, bs, n = C.c_float(7.0), C.c_float(7.0), C.c_int(7)
        rc = trk.L.dsm_diag_single_eval(trk.h, mode, lvl, dp(pose), dp(aff), 1.0, 20.0, form, 0, dp(rs), dp(H), dp(b), C.byref(hs), C.byref(bs),
                                        C.byref(n))
        assert rc == -1, (mode, lvl, form, rc)  # DSM_ERR_INVALID
        assert np.all(rs == 7) and np.all(H == 7) and np.all(b == 7) and hs.value == bs.value == 7 and n.value == 7, (mode, lvl, form)
    # ... and the tracker still evaluates
    K.check_pose_outputs(trk.calcResPose(0, sc.gt_pose, list(sc.gt_aff), 20.0),
                         G.pose_ref(numpy_tracker(sc), 0, N.pose_to_matrix(pose), list(sc.gt_aff), 20.0),
                         G.pts_per_thread(len(sc.tpl[0][0]), 1), "after bad arguments", lambda *a: None)
    trk.close()
