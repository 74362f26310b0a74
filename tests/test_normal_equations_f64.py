"""Every single evaluation's normal equations against their exact value (tests/_gn_f64.py): per entry, within the bound of the
device's summation tree and per-point formation, for each chunk table -- next to the whole-matrix bars of test_parity_tracker.py.

Integer outputs (numTermsInE, the saturated share, the padded warped count) equal the reference's; every H and b entry within
u ((P + 24) A + F); h00 and h01 alike; E within min(2e-6 E64, its bound); the flow indicators within theirs; an entry whose
absolute sum A is 0 exactly 0.  With no usable point only the integer outputs and E are compared, as in assert_eval_pose_equal.
(The assertions themselves live in tests/_gn_checks.py, shared with tests/test_eval_forms_f64.py.)"""
import numpy as np
import pytest

import _gn_checks as K
import _gn_f64 as G
from _gn_checks import TABLES, numpy_tracker, sweep_sizes, three_poses, trackers
from _scenes import _photometry, make_affine_scene, make_scene
from direct_stereo_slam_amd import synth as S
from oracle import numpy_ref as N

pytestmark = pytest.mark.gpu

WORST = {}  # (table, entry class) -> worst err / bound


@pytest.fixture(scope="module", autouse=True)
def report_worst():
    yield
    classes = ("diag", "offdiag", "b", "E", "scale", "flow")
    print("\nworst err / bound per chunk table and entry class")
    for t in TABLES:
        print(f"  table {t}: " + "  ".join(f"{c} {WORST.get((t, c), float('nan')):.4f}" for c in classes))


def _note(table):
    return lambda cls, err, bnd: K.note_worst(WORST, (table, cls), err, bnd)


def check_pose(trk, table, ref, lvl, pose, aff, cutoff, where=""):
    where = (where, "pose", lvl, table, tuple(np.round(pose, 4)), tuple(aff), cutoff)
    K.check_pose_outputs(trk.calcResPose(lvl, pose, aff, cutoff), ref, G.pts_per_thread(ref["n_tpl"], table), where, _note(table))


def check_scale(trk, table, ref, lvl, scale, cutoff, where=""):
    where = (where, "scale", lvl, table, scale, cutoff)
    K.check_scale_outputs(trk.calcResScale(lvl, scale, cutoff), ref, G.pts_per_thread(ref["n_tpl"], table), where, _note(table))


def sweep_scene(ctx, sc, levels, poses, cutoffs=(20.0, 5.0), scales=(1.0, 0.8), where=""):
    npt, trks = numpy_tracker(sc), trackers(ctx, sc)
    for lvl in levels:
        for pose, aff in poses:
            for cutoff in cutoffs:
                ref = G.pose_ref(npt, lvl, N.pose_to_matrix(np.asarray(pose, np.float64)), aff, cutoff)
                for t, trk in zip(TABLES, trks):
                    check_pose(trk, t, ref, lvl, pose, aff, cutoff, where)
        for scale in scales:
            for cutoff in cutoffs:
                ref = G.scale_ref(npt, lvl, scale, cutoff)
                for t, trk in zip(TABLES, trks):
                    check_scale(trk, t, ref, lvl, scale, cutoff, where)
    for trk in trks:
        trk.close()


@pytest.mark.parametrize("size,template", [("tiny", "dense"), ("small", "dense"), ("medium", "dense"), ("odd", "dense"), ("mini4", "dense"),
                                           ("small", "sparse")])
def test_every_level(ctx, size, template):
    sc = make_scene(size, seed=11, template=template, n0=3000)
    sweep_scene(ctx, sc, range(sc.nl), three_poses(sc), where=size)


@pytest.mark.parametrize("size,seed", [("kitti6", 0x5EED0000), ("hd6", 0x5EED0001)])
def test_six_level_configs_full_size(ctx, size, seed):
    sc = make_scene(size, seed=seed, noise=2.0)
    sweep_scene(ctx, sc, (0, 3, 5), three_poses(sc), scales=(1.0,), where=size)


@pytest.mark.parametrize("case", ["dark_keyframe_longer_exposure", "bright_keyframe_shorter_exposure", "zero_reference_exposure",
                                  "zero_new_exposure", "relief_family"])
def test_affine_cases(ctx, case):
    from test_parity_tracker import AFFINE_CASES

    sc = make_affine_scene("small", seed=31, **AFFINE_CASES[case])
    poses = [(p, a) for p in (S.IDENTITY_POSE, sc.gt_pose) for a in (list(sc.ref_aff), list(sc.gt_aff), [0.0, 0.0])]
    sweep_scene(ctx, sc, range(sc.nl), poses, cutoffs=(20.0,), scales=(1.0,), where=case)


def test_edge_inputs(ctx):
    """test_parity_tracker.test_edge_cases' inputs: ragged sizes, an empty level, a single point, NaN / inf texels, NaN / negative /
    zero inverse depths; then every point outside the image and every residual saturated"""
    sc = K.edge_scene()
    sweep_scene(ctx, sc, range(sc.nl), [(sc.gt_pose, list(sc.gt_aff))], cutoffs=(20.0,), scales=(1.0,), where="edge")
    far = S.pose_from_Rt(np.eye(3), [50.0, 0, 0])
    sweep_scene(ctx, sc, (0,), [(far, [0.0, 0.0]), (sc.gt_pose, [0.0, 200.0])], cutoffs=(20.0,), scales=(), where="edge")


def test_chunk_edge_sweep(ctx):
    """level 0 of a dense KITTI template (446 992 points) cut to every P edge +- 1, to one-point last chunks and to a few points;
    both problem kinds under the three chunk tables"""
    sc = make_scene("kitti", seed=21)
    full = [a[0] for a in sc.tpl]
    assert len(full[0]) == 446992
    ns = sweep_sizes() + [len(full[0])]
    npt, trks = numpy_tracker(sc), trackers(ctx, sc)
    ref_aff, ref_exp, _ = _photometry(sc)
    seen = {t: set() for t in TABLES}
    for n in ns:
        tpl = [[a[0][:n].copy()] + list(a[1:]) for a in sc.tpl]
        npt.set_ref(ref_aff[0], ref_aff[1], ref_exp, *tpl)
        for t, trk in zip(TABLES, trks):
            trk.setCoarseTrackingRef(0, ref_aff, ref_exp, *tpl)
            assert trk.reduction_geometry(0, n) == G.reduction_geometry(n, t), (n, t)
            seen[t].add(G.pts_per_thread(n, t))
        ref = G.pose_ref(npt, 0, N.pose_to_matrix(np.asarray(sc.gt_pose, np.float64)), list(sc.gt_aff), 20.0)
        sref = G.scale_ref(npt, 0, 1.0, 20.0)
        for t, trk in zip(TABLES, trks):
            check_pose(trk, t, ref, 0, sc.gt_pose, list(sc.gt_aff), 20.0, where=f"n={n}")
            check_scale(trk, t, sref, 0, 1.0, 20.0, where=f"n={n}")
    for trk in trks:
        trk.close()
    # every points-per-thread value of every table was visited (a changed table cannot skip one silently)
    assert all(seen[t] == {1, 2, 4, 8, 16} for t in TABLES), seen
