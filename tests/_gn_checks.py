"""What tests/test_normal_equations_f64.py and tests/test_eval_forms_f64.py share: the trackers of a scene (one per chunk table next to
the float64 reference's), the inputs of the sweeps, and the assertions of one evaluation's outputs against tests/_gn_f64.py's exact
sums -- as functions of the outputs, whichever entry point or form of the evaluation loop produced them.

`note(entry class, err, bound)` is the caller's book-keeping of the worst err / bound it has seen."""
import numpy as np

import _gn_f64 as G
from _scenes import _photometry, hip_tracker
from direct_stereo_slam_amd import synth as S
from oracle import numpy_ref as N

TABLES = (0, 1, 2)


def note_worst(worst, key, err, bnd):
    """worst[key] = the largest err / bound over the entries whose bound is positive"""
    err, bnd = np.atleast_1d(err), np.atleast_1d(bnd)
    pos = bnd > 0
    if pos.any():
        worst[key] = max(worst.get(key, 0.0), float(np.max(err[pos] / bnd[pos])))


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


def three_poses(sc):
    return [(S.IDENTITY_POSE, [0.0, 0.0]), (sc.gt_pose, list(sc.gt_aff)), (motion_3x(sc.gt_pose), list(sc.gt_aff))]


def edge_scene():
    """test_parity_tracker.test_edge_cases' inputs: ragged sizes, an empty level, a single point, NaN / inf texels, NaN / negative /
    zero inverse depths"""
    from _scenes import make_scene, regrad

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
    return sc


def sweep_sizes():
    """level-0 point counts of the chunk-edge sweep"""
    edges = [256, 512, 1024, 2048, 4096, 16384, 65536, 262144]  # P edges of the three tables (and the throughput table's one-chunk edge)
    ns = {e + d for e in edges for d in (-1, 0, 1)}
    # a one-point last chunk: 256 P k + 1 at P = 16 / 2 / 4 / 8 / 16 of the latency table's ranges and the throughput table's
    ns |= {4096 * 1 + 1, 4096 * 2 + 1, 512 * 9 + 1, 1024 * 20 + 1, 2048 * 40 + 1, 4096 * 70 + 1}
    ns |= {1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257}
    return sorted(ns)


def common_checks(rs, n, ref, P, where, note):
    assert int(rs[1]) == ref["n_terms"], ("numTermsInE", where)
    assert n == ref["n4"], ("warped count", where)
    if ref["n_terms"] > 0:
        assert np.float32(rs[5]) == ref["sat_ratio"], ("saturated share", where)
        E64 = ref["E64"]
        err, bnd = abs(rs[0] - E64), G.energy_bound(E64, P)
        assert err <= min(2e-6 * E64, bnd), ("E", where, err, bnd, 2e-6 * E64)
        note("E", err, bnd)
    else:
        assert np.isnan(rs[5]) and rs[0] == 0, ("empty evaluation", where)
    fl = np.array([rs[2], rs[4]])
    # column by column: a finite indicator within its bound, a non-finite one (a flow point with a vanishing depth; in mode 2 a pose with
    # t2 = 1, which makes the translation-only column infinite and leaves the other finite) the same non-finite value
    finite = np.isfinite(ref["flow64"])
    if finite.any():
        err, bnd = np.abs(fl[finite] - ref["flow64"][finite]), G.flow_bound(ref["flow64"][finite])
        assert np.all(err <= bnd), ("flow", where, fl, ref["flow64"], bnd)
        note("flow", err, bnd)
    if not finite.all():
        try:
            np.testing.assert_array_equal(fl[~finite], ref["flow64"][~finite])
        except AssertionError as e:
            raise AssertionError(("flow", where, fl, ref["flow64"])) from e


def check_pose_outputs(out, ref, P, where, note):
    """(rs, H, b, n) of one full pose evaluation against pose_ref's `ref` at P points per thread"""
    rs, H, b, n = out
    common_checks(rs, n, ref, P, where, note)
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
    note("diag", errH[d], bndH[d])
    note("offdiag", errH[~d], bndH[~d])
    note("b", errb, bndb)


def check_scale_outputs(out, ref, P, where, note):
    """(rs, h00, h01, n) of one full scale evaluation against scale_ref's `ref`"""
    rs, h00, h01, n = out
    common_checks(rs, n, ref, P, where, note)
    if n == 0:
        return
    h = np.array([h00, h01])
    err, bnd = np.abs(h - ref["h64"]), G.bound(ref["A"], ref["F"], P)
    assert np.all(h[ref["A"] == 0] == 0), ("entry of zero scale", where)
    assert np.all(err <= bnd), ("h00 / h01", where, err / np.where(bnd > 0, bnd, 1))
    note("scale", err, bnd)
