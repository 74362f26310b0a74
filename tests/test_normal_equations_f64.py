"""Every single evaluation's normal equations against their exact value (tests/_gn_f64.py): per entry, within the bound of the
device's summation tree and per-point formation, for each chunk table -- next to the whole-matrix bars of test_parity_tracker.py.

Integer outputs (numTermsInE, the saturated share, the padded warped count) equal the reference's; every H and b entry within
u ((P + 24) A + F); h00 and h01 alike; E within min(2e-6 E64, its bound); the flow indicators within theirs; an entry whose
absolute sum A is 0 exactly 0.  With no usable point only the integer outputs and E are compared, as in assert_eval_pose_equal."""
import numpy as np
import pytest

import _gn_f64 as G
from _scenes import SIZES, _photometry, hip_tracker, make_affine_scene, make_scene, regrad
from direct_stereo_slam_amd import synth as S
from oracle import numpy_ref as N

pytestmark = pytest.mark.gpu

TABLES = (0, 1, 2)
WORST = {}  # (table, entry class) -> worst err / bound


@pytest.fixture(scope="module", autouse=True)
def report_worst():
    yield
    classes = ("diag", "offdiag", "b", "E", "scale", "flow")
    print("\nworst err / bound per chunk table and entry class")
    for t in TABLES:
        print(f"  table {t}: " + "  ".join(f"{c} {WORST.get((t, c), float('nan')):.4f}" for c in classes))


def _note(table, cls, err, bnd):
    err, bnd = np.atleast_1d(err), np.atleast_1d(bnd)
    pos = bnd > 0
    if pos.any():
        WORST[(table, cls)] = max(WORST.get((table, cls), 0.0), float(np.max(err[pos] / bnd[pos])))


def numpy_tracker(sc):
    ref_aff, ref_exp, new_exp = _photometry(sc)
    t = N.NumpyTracker(sc.w, sc.h, sc.nl, sc.T, sc.K)
    t.make_k(*sc.K)
    t.set_ref(ref_aff[0], ref_aff[1], ref_exp, *sc.tpl)
    t.set_frame(0, sc.new_p, new_exp)
    t.set_frame(1, sc.right_p, 1.0)
    return t


def trackers(ctx, sc):
    from direct_stereo_slam_amd.tracker import default_params

    out = []
    for t in TABLES:
        p = default_params()
        p.chunk_geometry = t
        out.append(hip_tracker(ctx, sc, p))
    return out


def motion_3x(pose):
    """the pose with three times the rotation angle and the translation of `pose`"""
    from scipy.spatial.transform import Rotation

    q = Rotation.from_rotvec(3.0 * Rotation.from_quat(pose[:4]).as_rotvec()).as_quat()
    return np.concatenate([q if q[3] >= 0 else -q, 3.0 * np.asarray(pose[4:], np.float64)])


def _common_checks(rs, n, ref, P, table, where):
    assert int(rs[1]) == ref["n_terms"], ("numTermsInE", where)
    assert n == ref["n4"], ("warped count", where)
    if ref["n_terms"] > 0:
        assert np.float32(rs[5]) == ref["sat_ratio"], ("saturated share", where)
        E64 = ref["E64"]
        err, bnd = abs(rs[0] - E64), G.energy_bound(E64, P)
        assert err <= min(2e-6 * E64, bnd), ("E", where, err, bnd, 2e-6 * E64)
        _note(table, "E", err, bnd)
    else:
        assert np.isnan(rs[5]) and rs[0] == 0, ("empty evaluation", where)
    fl = np.array([rs[2], rs[4]])
    if np.all(np.isfinite(ref["flow64"])):
        err, bnd = np.abs(fl - ref["flow64"]), G.flow_bound(ref["flow64"])
        assert np.all(err <= bnd), ("flow", where, fl, ref["flow64"], bnd)
        _note(table, "flow", err, bnd)
    else:  # a flow point with a vanishing depth: the same non-finite value
        np.testing.assert_array_equal(fl, ref["flow64"])


def check_pose(trk, table, ref, lvl, pose, aff, cutoff, where=""):
    where = (where, "pose", lvl, table, tuple(np.round(pose, 4)), tuple(aff), cutoff)
    rs, H, b, n = trk.calcResPose(lvl, pose, aff, cutoff)
    P = G.pts_per_thread(ref["n_tpl"], table)
    _common_checks(rs, n, ref, P, table, where)
    if n == 0:
        return
    errH, bndH = np.abs(H - ref["H64"]), G.bound(ref["A"], ref["F"], P)
    errb, bndb = np.abs(b - ref["b64"]), G.bound(ref["Ab"], ref["Fb"], P)
    assert np.all(H[ref["A"] == 0] == 0) and np.all(b[ref["Ab"] == 0] == 0), ("entry of zero scale", where)
    bad = np.argwhere(errH > bndH)
    assert len(bad) == 0, ("H", where, [(int(i), int(j), errH[i, j] / bndH[i, j]) for i, j in bad[:8]])
    bad = np.flatnonzero(errb > bndb)
    assert len(bad) == 0, ("b", where, [(int(i), errb[i] / bndb[i]) for i in bad])
    d = np.eye(8, dtype=bool)
    _note(table, "diag", errH[d], bndH[d])
    _note(table, "offdiag", errH[~d], bndH[~d])
    _note(table, "b", errb, bndb)


def check_scale(trk, table, ref, lvl, scale, cutoff, where=""):
    where = (where, "scale", lvl, table, scale, cutoff)
    rs, h00, h01, n = trk.calcResScale(lvl, scale, cutoff)
    P = G.pts_per_thread(ref["n_tpl"], table)
    _common_checks(rs, n, ref, P, table, where)
    if n == 0:
        return
    h = np.array([h00, h01])
    err, bnd = np.abs(h - ref["h64"]), G.bound(ref["A"], ref["F"], P)
    assert np.all(h[ref["A"] == 0] == 0), ("entry of zero scale", where)
    assert np.all(err <= bnd), ("h00 / h01", where, err / np.where(bnd > 0, bnd, 1))
    _note(table, "scale", err, bnd)


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


def three_poses(sc):
    return [(S.IDENTITY_POSE, [0.0, 0.0]), (sc.gt_pose, list(sc.gt_aff)), (motion_3x(sc.gt_pose), list(sc.gt_aff))]


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
    sc = make_scene("small", seed=13)
    for lvl, n in [(0, 1001), (1, 0), (2, 1)]:
        for a in sc.tpl:
            a[lvl] = a[lvl][:n].copy()
    sc.new_p[0][40:44, 100:140, 0] = np.nan
    sc.new_p[0][50, 60:70, 0] = np.inf
    sc.new_p[0] = regrad(sc.new_p[0])
    sc.tpl[2][0][5] = np.nan
    sc.tpl[2][0][6] = -0.1
    sc.tpl[2][0][7] = 0.0
    sweep_scene(ctx, sc, range(sc.nl), [(sc.gt_pose, list(sc.gt_aff))], cutoffs=(20.0,), scales=(1.0,), where="edge")
    far = S.pose_from_Rt(np.eye(3), [50.0, 0, 0])
    sweep_scene(ctx, sc, (0,), [(far, [0.0, 0.0]), (sc.gt_pose, [0.0, 200.0])], cutoffs=(20.0,), scales=(), where="edge")


def sweep_sizes():
    """level-0 point counts of the chunk-edge sweep"""
    edges = [256, 512, 1024, 2048, 4096, 16384, 65536, 262144]  # P edges of the three tables (and the throughput table's one-chunk edge)
    ns = {e + d for e in edges for d in (-1, 0, 1)}
    # a one-point last chunk: 256 P k + 1 at P = 16 / 2 / 4 / 8 / 16 of the latency table's ranges and the throughput table's
    ns |= {4096 * 1 + 1, 4096 * 2 + 1, 512 * 9 + 1, 1024 * 20 + 1, 2048 * 40 + 1, 4096 * 70 + 1}
    ns |= {1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257}
    return sorted(ns)


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
