"""The float64 reference of tests/_gn_f64.py and its bound, on the CPU:
  (a) the device's documented summation tree (eval_chunk_impl in tracker_kernels.hip, row16_sum in wave_ops.hpp, reduce_partials_groups / _final in lm_step.hpp),
      restated in numpy float32 on the oracle's per-point values, lies well inside the reduction part of the bound for every
      chunk table -- so the bound is not tight against the order the device really uses;
  (b) the bound has teeth: a lost or doubled point and an entry off by 100 u A pass the whole-matrix bars of
      tests/test_parity_tracker.py and fail the per-entry bound;
  (c) the residual-only assertions of tests/test_eval_forms_f64.py have teeth: a lost point, a doubled point and a point whose
      intensity is gathered one column to the right, over the chunk-edge sweep's sizes."""
import numpy as np
import pytest

import _gn_f64 as G
from _gn_checks import sweep_sizes
from _scenes import make_scene
from direct_stereo_slam_amd import synth as S
from oracle import numpy_ref as N

FLOAT_RTOL = 2e-5  # tests/test_parity_tracker.py


def numpy_tracker(sc):
    t = N.NumpyTracker(sc.w, sc.h, sc.nl, sc.T, sc.K)
    t.make_k(*sc.K)
    t.set_ref(0.0, 0.0, 1.0, *sc.tpl)
    t.set_frame(0, sc.new_p, 1.0)
    t.set_frame(1, sc.right_p, 1.0)
    return t


def T_of(pose):
    return N.pose_to_matrix(np.asarray(pose, np.float64))


# ---- today's bars (assert_eval_pose_equal / assert_eval_scale_equal) as pure functions of (device, reference) -----------------
# (the teeth tests pass the exact sums as the reference: what the bars let through, apart from the oracle's own rounding)
def old_pose_ok(H_g, b_g, H_o, b_o):
    hb = FLOAT_RTOL * np.abs(H_o).max()
    bb = FLOAT_RTOL * max(np.abs(b_o).max(), 1e-3 * np.sqrt(np.abs(H_o).max()))
    return bool(np.all(np.abs(H_g - H_o) <= hb) and np.all(np.abs(b_g - b_o) <= bb))


def old_scale_ok(h_g, b_g, h_o, b_o):
    return abs(h_g - h_o) <= 5e-5 * abs(h_o) and abs(b_g - b_o) <= 5e-5 * max(abs(b_o), 1e-3 * abs(h_o))


def new_pose_ok(H_g, b_g, ref, P):
    return bool(np.all(np.abs(H_g - ref["H64"]) <= G.bound(ref["A"], ref["F"], P)) and
                np.all(np.abs(b_g - ref["b64"]) <= G.bound(ref["Ab"], ref["Fb"], P)))


def new_scale_ok(h, ref, P):
    return bool(np.all(np.abs(np.asarray(h) - ref["h64"]) <= G.bound(ref["A"], ref["F"], P)))


# ---- (a) the device's tree in float32 --------------------------------------------------------------------------------------
def f32(x):
    return np.asarray(x, np.float32)


def device_tree(values, idx, n_tpl, P, fma=None):
    """values (k, m) float32 per-point terms of the m usable points at template indices idx (fma = (a, b): terms a * b added with
    a fused multiply-add, as the accumulators are); returns the k sums as build_H_elem / build_rs read them (float of the double sum).
    Thread t of chunk c adds points c 256 P + j 256 + t, j = 0..P-1, in order; row16_sum adds the 16 lanes of a row pairwise; the 16
    rows are added in order into the chunk's float partial; group g of 19 adds chunks g, g + 19, ... in double, then the groups in order."""
    nch = (n_tpl + 256 * P - 1) // (256 * P)
    k = (fma[0] if fma is not None else values).shape[0]
    acc = np.zeros((k, nch, 256), np.float32)
    if fma is not None:
        a, b = (np.zeros((k, nch * 256 * P), np.float64) for _ in range(2))
        a[:, idx], b[:, idx] = fma[0], fma[1]
        a, b = a.reshape(k, nch, P, 256), b.reshape(k, nch, P, 256)
        for j in range(P):  # fmaf: the exact product plus the accumulator, rounded once
            acc = f32(acc.astype(np.float64) + a[:, :, j] * b[:, :, j])
    else:
        full = np.zeros((k, nch * 256 * P), np.float32)
        full[:, idx] = values
        full = full.reshape(k, nch, P, 256)
        for j in range(P):
            acc = f32(acc + full[:, :, j])
    v = acc.reshape(k, nch, 16, 16)  # [row][lane]: row = tid >> 4
    for _ in range(4):  # quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror, row_mirror: lane 0 ends with the balanced pairwise tree
        v = f32(v[..., 0::2] + v[..., 1::2])
    rows = v[..., 0]
    part = rows[:, :, 0].copy()
    for r in range(1, 16):
        part = f32(part + rows[:, :, r])
    groups = [np.zeros(k) for _ in range(19)]
    for c in range(nch):
        groups[c % 19] = groups[c % 19] + part[:, c].astype(np.float64)
    tot = groups[0].copy()
    for g in range(1, 19):
        tot = tot + groups[g]
    return f32(tot)


def tree_pose(ref, P, npt):
    """the device's H, b and E of one pose evaluation under the tree above, on the oracle's per-point values"""
    Jd, Wd = ref["products"]
    J32, W32 = f32(Jd), f32(Wd)
    m = len(ref["idx"])
    Jw = f32(J32 * W32)[:, :m]  # J_r w (stage_b), then fmaf(J_r w, J_c, acc)
    r_, c_ = np.triu_indices(9)
    sums = device_tree(None, ref["idx"], ref["n_tpl"], P, fma=(Jw[r_].astype(np.float64), J32[c_, :m].astype(np.float64)))
    T9 = np.zeros((9, 9))
    T9[r_, c_] = sums
    T9[c_, r_] = sums
    invn = float(np.float32(1.0) / np.float32(ref["n4"]))
    s = npt.scales
    H = (T9[:8, :8] * invn * s[None, :]) * s[:, None]
    b = T9[:8, 8] * invn * s
    E = float(np.float32(float(device_tree(ref["Eterms"][None, :], ref["idx"], ref["n_tpl"], P)[0]) + ref["n_sat"] * float(ref["max_energy"])))
    return H, b, E


def tree_scale(ref, P):
    j, wd = ref["products"]
    m = len(ref["idx"])
    J32, W32 = f32(j), f32(wd)
    J0w = f32(J32[0] * W32)[:m]
    sums = device_tree(None, ref["idx"], ref["n_tpl"], P, fma=(np.array([J0w, J0w], np.float64), J32[:, :m].astype(np.float64)))
    invn = np.float32(1.0) / np.float32(ref["n4"])
    return np.array([f32(sums[0] * invn), f32(sums[1] * invn)], np.float64)


@pytest.mark.parametrize("size,template", [("small", "dense"), ("medium", "sparse"), ("odd", "dense"), ("kitti", "dense")])
def test_device_tree_emulation_is_well_inside_the_bound(built, size, template):
    sc = make_scene(size, seed=11, template=template, n0=3000)
    npt = numpy_tracker(sc)
    worst = {}
    levels = (0, sc.nl - 1) if size == "kitti" else range(sc.nl)
    for lvl in levels:
        n_tpl = len(sc.tpl[0][lvl])
        for pose, aff in [(S.IDENTITY_POSE, [0.0, 0.0]), (sc.gt_pose, list(sc.gt_aff))]:
            ref = G.pose_ref(npt, lvl, T_of(pose), aff, 20.0)
            sref = G.scale_ref(npt, lvl, 1.0, 20.0)
            assert ref["n4"] > 0 and sref["n4"] > 0
            for geom in (0, 1, 2):
                P = G.pts_per_thread(n_tpl, geom)
                H, b, E = tree_pose(ref, P, npt)
                h = tree_scale(sref, P)
                red = lambda A: G.U * (P + G.K_TREE) * A  # the reduction part of the bound: the emulation uses the oracle's per-point values
                for name, err, bnd in (("H", np.abs(H - ref["H64"]), red(ref["A"])), ("b", np.abs(b - ref["b64"]), red(ref["Ab"])),
                                       ("E", abs(E - ref["E64"]), G.U * (P + G.K_TREE) * ref["E64"]),
                                       ("scale", np.abs(h - sref["h64"]), red(sref["A"]))):
                    ratio = np.max(np.where(bnd > 0, err / np.where(bnd > 0, bnd, 1), 0))
                    assert np.all(err[bnd == 0] == 0) if np.ndim(bnd) else True
                    worst[(geom, name)] = max(worst.get((geom, name), 0.0), float(ratio))
                    assert ratio <= 0.25, (lvl, geom, name, ratio)
    print(size, template, {k: round(v, 4) for k, v in sorted(worst.items())})


# ---- (b) teeth ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kitti_65537(built):
    """level 0 of the dense KITTI template cut to 65 537 points: one point in the last chunk of either table"""
    sc = make_scene("kitti", seed=21)
    n = 65537
    for a in sc.tpl:
        a[0] = a[0][:n].copy()
    assert [G.reduction_geometry(n, g)[1:] for g in (0, 1, 2)] == [(16, 17), (8, 33), (8, 33)]
    return sc, numpy_tracker(sc)


def _point_share(ref, k):
    """the contribution of usable point k (index into the buffer) to H and b"""
    Jd, Wd = ref["products"]
    n4 = ref["n4"]
    invn = float(np.float32(1.0) / np.float32(n4))
    p = np.outer(Jd[:, k] * Wd[k], Jd[:, k]) * invn
    return p


@pytest.mark.parametrize("case", ["drop_last", "double_middle"])
def test_bound_catches_one_point_the_old_bars_miss(kitti_65537, case):
    """the H sums (and h00) of an evaluation that lost its last point -- the lone point of the last chunk -- or counted a point twice.
    (Today's b bar, scaled to max |b|, does see such a point through b[7], where J7 = -1 meets SCALE_B = 1000: the per-entry bound is
    what holds the 36 entries of H to the same standard.)"""
    sc, npt = kitti_65537
    P = max(G.pts_per_thread(65537, g) for g in (0, 1, 2))  # the loosest table
    T, aff = T_of(sc.gt_pose), list(sc.gt_aff)
    ref = G.pose_ref(npt, 0, T, aff, 20.0)
    assert ref["idx"][-1] == 65536, "the lone point of the last chunk is usable"
    k = len(ref["idx"]) - 1 if case == "drop_last" else len(ref["idx"]) // 2
    sign = -1.0 if case == "drop_last" else 1.0
    p = _point_share(ref, k) * sign
    s = npt.scales
    H_pert = ref["H64"] + (p[:8, :8] * s[None, :]) * s[:, None]
    H_o, b_o = ref["H64"], ref["b64"]
    assert new_pose_ok(H_o, b_o, ref, P)
    assert old_pose_ok(H_pert, ref["b64"], H_o, b_o), "the whole-matrix bar lets the lost / doubled point through"
    assert not new_pose_ok(H_pert, ref["b64"], ref, P), "the per-entry bound catches it"


@pytest.mark.parametrize("pose", ["identity", "true"])
def test_bound_catches_one_entry_off_by_100_u_A(kitti_65537, pose):
    """one off-diagonal H entry (both of its places: the device builds H(r, c) and H(c, r) from one sum) and one b entry"""
    sc, npt = kitti_65537
    P = max(G.pts_per_thread(65537, g) for g in (0, 1, 2))
    T, aff = (T_of(S.IDENTITY_POSE), [0.0, 0.0]) if pose == "identity" else (T_of(sc.gt_pose), list(sc.gt_aff))
    ref = G.pose_ref(npt, 0, T, aff, 20.0)
    H_o, b_o = ref["H64"], ref["b64"]
    for (i, j), kb in (((0, 1), 2), ((3, 5), 0), ((6, 7), 2)):  # H: a gradient pair, a rotation pair, the affine pair; b: where the old bar exceeds 100 u A
        H_pert, b_pert = ref["H64"].copy(), ref["b64"].copy()
        H_pert[i, j] += 100 * G.U * ref["A"][i, j]
        H_pert[j, i] = H_pert[i, j]
        assert old_pose_ok(H_pert, ref["b64"], H_o, b_o) and not new_pose_ok(H_pert, ref["b64"], ref, P), (i, j)
        b_pert[kb] += 100 * G.U * ref["Ab"][kb]
        assert old_pose_ok(ref["H64"], b_pert, H_o, b_o) and not new_pose_ok(ref["H64"], b_pert, ref, P), kb
    # h00 and h01 of the scale problem alike
    sref = G.scale_ref(npt, 0, 1.0, 20.0)
    h_o, hb_o = sref["h64"]
    for e in (0, 1):
        h = sref["h64"].copy()
        h[e] += 100 * G.U * sref["A"][e]
        assert old_scale_ok(h[0], h[1], float(h_o), float(hb_o)) and not new_scale_ok(h, sref, P), e


# ---- (c) the residual-only assertions' teeth ------------------------------------------------------------------------------
def ro_device(ref, P, Eterms, idx, n_terms, n_sat):
    """what a residual-only evaluation returns -- (E, numTermsInE, saturated share, padded warped count) -- for usable points at template
    indices idx with energy terms Eterms, under the device's tree at P points per thread (build_rs: the float of E's double sum plus
    n_sat x max_energy)"""
    tree = float(device_tree(Eterms[None, :], idx, ref["n_tpl"], P)[0]) if len(idx) else 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.float32(tree + n_sat * float(ref["max_energy"]))), n_terms, np.float32(n_sat) / np.float32(n_terms), (len(idx) + 3) & ~3


def ro_caught(out, ref, P):
    """which of test_eval_forms_f64's residual-only assertions (tests/_gn_checks.py common_checks) fails on `out`: 'int', 'E' or None"""
    E, n_terms, sat_ratio, n4 = out
    if n_terms != ref["n_terms"] or n4 != ref["n4"] or (ref["n_terms"] > 0 and sat_ratio != ref["sat_ratio"]):
        return "int"
    if ref["n_terms"] > 0 and abs(E - ref["E64"]) > min(2e-6 * ref["E64"], G.energy_bound(ref["E64"], P)):
        return "E"
    return None


def shifted_terms(npt, ref, aff, cutoff):
    """every usable point's residual taken from the texel one column to the right (Ku + 1): (its energy term, whether the point stays
    usable -- finite and below the cut-off, so that the integer outputs do not move)"""
    B = ref["buf"]
    a, b = N.aff_from_to(npt.ref_exposure, npt.new_exposure, npt.ref_aff, aff)
    Ku, Kv = npt.fx[0] * B["u"] + npt.cx[0], npt.fy[0] * B["v"] + npt.cy[0]
    h = N.interp33(npt.new_dIp[0], Ku + np.float32(1), Kv)[:, 0]
    r = h - (np.float32(a) * B["refc"] + np.float32(b))
    ar = np.abs(r)
    with np.errstate(divide="ignore", invalid="ignore"):
        hw = np.where(ar < npt.huber, np.float32(1), npt.huber / ar).astype(np.float32)
        return (((hw * r) * r) * (np.float32(2) - hw)).astype(np.float32), np.isfinite(h) & (ar <= np.float32(cutoff))


SHIFT_LOW_DECILE_CAUGHT = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 4609, 8193,
                           16383, 16384, 16385, 20481, 65535, 65536, 65537, 81921]


def test_residual_only_assertions_catch_one_wrong_point(built):
    """The residual-only assertions (integer outputs equal, E within min(2e-6 E64, energy_bound)) against an emulated residual-only
    evaluation (the device's tree on the oracle's terms) of level 0 of the dense KITTI template, seed 21, at the true pose, cut to the
    chunk-edge sweep's sizes -- the first n points as the sweep cuts them; where those hold no usable point (n <= 513: the template's
    first rows leave the image), n points from the first usable point of the template's second half.  Loosest table of each size.
      * one usable point dropped, one counted twice: caught by the integer outputs at EVERY size;
      * one usable point's residual taken from the texel one column to the right (what a two-tap gather does when it goes wrong), the
        point staying usable so that the integer outputs cannot see it: E moves by the difference d of two energy terms, and the bar
        catches it while d exceeds about 2e-6 E64.  For the point of MEDIAN d among the usable ones that is every size of the sweep, the
        full 446 992 points included (d = 6.5e-6 E64 there, 3.2 times the bar).  For the point at the LOWEST DECILE of d it is the
        sizes of SHIFT_LOW_DECILE_CAUGHT: every size up to 81 921, none from 262 143 up.  Largest n caught: 81 921, where d is 0.999 of
        the bar and the tree's own rounding of E tips it over; 1.24 of the bar at 65 537, 0.35 at 262 143.  At 446 992 points 72 % of the
        usable points are individually visible to the E bar (asserted below as 0.70 .. 0.75), 91 % at 65 537, all of them up to 2049."""
    sc = make_scene("kitti", seed=21)
    npt = numpy_tracker(sc)
    T, aff, cutoff = T_of(sc.gt_pose), list(sc.gt_aff), 20.0
    whole = len(sc.tpl[0][0])
    assert whole == 446992
    idx_whole = G.residual_ref(npt, 0, T, aff, cutoff)["idx"]
    mid = int(idx_whole[np.searchsorted(idx_whole, whole // 2)])
    low_caught, rows = [], []
    for n in sweep_sizes() + [whole]:
        for start in (0, mid):
            npt.set_ref(0.0, 0.0, 1.0, *[[a[0][start:start + n].copy()] + list(a[1:]) for a in sc.tpl])
            ref = G.residual_ref(npt, 0, T, aff, cutoff)
            if len(ref["idx"]):
                break
        m = len(ref["idx"])
        assert m > 0 and ref["n_tpl"] == n, n
        P = max(G.pts_per_thread(n, g) for g in (0, 1, 2))
        args = (ref["Eterms"], ref["idx"], ref["n_terms"], ref["n_sat"])
        assert ro_caught(ro_device(ref, P, *args), ref, P) is None, n  # the unmutated evaluation passes
        k = m // 2
        keep = np.arange(m) != k
        assert ro_caught(ro_device(ref, P, ref["Eterms"][keep], ref["idx"][keep], ref["n_terms"] - 1, ref["n_sat"]), ref, P) == "int", ("dropped", n)
        twice = (np.append(ref["Eterms"], ref["Eterms"][k]), np.append(ref["idx"], n), ref["n_terms"] + 1, ref["n_sat"])  # (the copy in a slot past the list)
        ref_t = dict(ref, n_tpl=n + 1)
        assert ro_caught(ro_device(ref_t, P, *twice), ref, P) == "int", ("doubled", n)
        terms, stays = shifted_terms(npt, ref, aff, cutoff)
        d = np.abs(terms.astype(np.float64) - ref["Eterms"].astype(np.float64))
        cand = np.flatnonzero(stays)
        if len(cand) == 0:  # (n = 1 .. 5: the shifted point leaves the usable set -- the integer outputs see it)
            low_caught.append(n)
            continue
        order = cand[np.argsort(d[cand], kind="stable")]
        got = {}
        for name, k in (("median", order[len(order) // 2]), ("low decile", order[len(order) // 10])):
            Et = ref["Eterms"].copy()
            Et[k] = terms[k]
            got[name] = ro_caught(ro_device(ref, P, Et, *args[1:]), ref, P)
        bar = min(2e-6 * ref["E64"], G.energy_bound(ref["E64"], P))
        rows.append((n, m, got["median"], got["low decile"], float(d[order[len(order) // 2]] / bar), float(d[order[len(order) // 10]] / bar),
                     float(np.mean(d[cand] > bar))))
        assert got["median"] == "E", ("a typical point's shifted gather", n, rows[-1])
        if got["low decile"] == "E":
            low_caught.append(n)
    print("n, usable, median caught, low decile caught, d / bar (median, low decile), share of points with d > bar")
    for r in rows:
        print("  ", r)
    assert low_caught == SHIFT_LOW_DECILE_CAUGHT, low_caught
    assert 0.70 <= rows[-1][-1] <= 0.75, rows[-1]
