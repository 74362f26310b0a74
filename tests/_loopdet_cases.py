"""Named edge cases for the loop descriptors (csrc/loopdet_kernels.hip; host forms in csrc/host_capi.cpp; numpy oracle in
oracle/scancontext.py) and the one comparison all three go through ("edges").

A case is a job tuple (kf_ids, kf_pose_wc, cur_cw, pt_kf_id, pt_xyz) plus lidar_range, num_s, num_r.  Most cases use cur_cw =
identity and one kept keyframe: camera frame = world frame, and a voxel can be named by hand (1 x 0.5 x 1 m, cell
floor(p + range), floor((p + range) * 2), floor(p + range)).  Clouds whose ScanContext half is predicted by hand are dyadic
(multiples of 2^-10) and balanced -- closed under the four EVEN sign flips, (x, y, z) -> (x, -y, -z), (-x, y, -z), (-x, -y, z) --
so that the mean is exact, the covariance exactly diagonal, eig3_sym leaves at its first test and the aligned coordinates are
the inputs themselves (minus an exact mean).  Under the even flips a point with height +x keeps its bin to itself: its
partners of height -x lie in the mirrored sectors.

`reaches(h)` is asserted on the REFERENCE side (the host form's result): the case gets to the place it is named for."""
import collections

import numpy as np

KF = 5                                   # the one kept keyframe of the identity jobs
EYE_CW = np.hstack([np.eye(3), np.zeros((3, 1))])
# ... with a translation of -0.0: `+ cw[r][3] * 1.0` then keeps the sign of a zero coordinate (-0.0 + -0.0 = -0.0, +0.0 + -0.0 = +0.0); with +0.0
# every zero would leave to_camera positive
NEGZERO_CW = np.hstack([np.eye(3), -np.zeros((3, 1))])
FLOAT_KEYS = ("pts_spherical", "ringkey", "tfm_pca_rig")

Case = collections.namedtuple("Case", "name job lidar_range num_s num_r oracle_sc slow_oracle reaches")


# ---- the comparison ----------------------------------------------------------------------------------------------------------
def same_bits(a, b):
    """float arrays of one dtype: equal bit for bit, a NaN's payload and sign aside (tests/_trace_ref.same_bits, any width)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool(np.all((np.ascontiguousarray(a).view(u) == np.ascontiguousarray(b).view(u)) | (np.isnan(a) & np.isnan(b))))


def same_values(a, b):
    """-0.0 == +0.0, NaN == NaN, everything else exactly"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def assert_same(got, exp=None, oracle=None, oracle_sc=True):
    """got against exp (another form of the same code path: host form, a solo run): integers exactly, pts_spherical / ringkey /
    tfm_pca_rig bit for bit, sig_val by value (the sign of a zero in sig_val is no part of the contract: DESIGN.md 4.6).
    got against the numpy oracle: selection and ring key exact, sig_val rtol 1e-9 / atol 1e-12, tfm_pca_rig atol 1e-9 (the bars of
    tests/test_device_loopdet.py); oracle_sc = False leaves the oracle's ScanContext half out (named cases only)."""
    if exp is not None:
        assert set(got) == set(exp), (sorted(got), sorted(exp))
        for k in ("kf_keep", "sel_idx", "sig_idx"):
            if k in exp:
                assert np.array_equal(got[k], exp[k]), (k, got[k][:12], exp[k][:12])
        assert int(got["n_out"]) == int(exp["n_out"])
        for k in FLOAT_KEYS:
            if k in exp:
                assert same_bits(got[k], exp[k]), (k, got[k], exp[k])
        if "sig_val" in exp:
            assert same_values(got["sig_val"], exp["sig_val"]), ("sig_val", got["sig_val"], exp["sig_val"])
    if oracle is not None:
        assert np.array_equal(got["kf_keep"], oracle["kf_keep"]), ("kf_keep", got["kf_keep"], oracle["kf_keep"])
        assert np.array_equal(got["sel_idx"], oracle["sel_idx"]), ("sel_idx", got["sel_idx"][:12], oracle["sel_idx"][:12])
        assert same_bits(np.asarray(got["pts_spherical"], np.float64), np.asarray(oracle["pts_spherical"], np.float64)), "pts_spherical"
        if oracle_sc and "ringkey" in oracle:
            assert "ringkey" in got
            assert same_bits(got["ringkey"], oracle["ringkey"]), ("ringkey", got["ringkey"], oracle["ringkey"])
            assert np.array_equal(got["sig_idx"], oracle["sig_idx"]), ("sig_idx", got["sig_idx"][:12], oracle["sig_idx"][:12])
            np.testing.assert_allclose(got["sig_val"], oracle["sig_val"], rtol=1e-9, atol=1e-12, equal_nan=True)
            np.testing.assert_allclose(got["tfm_pca_rig"], oracle["tfm_pca_rig"], rtol=0, atol=1e-9)


# ---- the three forms, as one result dict each -----------------------------------------------------------------------------------
def run_host(case):
    from direct_stereo_slam_amd.ringdb import generate_spherical_points, scancontext_generate

    keep, sel, pts = generate_spherical_points(case.job[0], case.job[1], case.job[2], case.lidar_range, case.job[3], case.job[4])
    r = dict(kf_keep=keep, n_out=len(sel), sel_idx=sel, pts_spherical=pts)
    if len(sel):
        rk, si, sv, tfm = scancontext_generate(pts, case.lidar_range, case.num_s, case.num_r)
        r.update(ringkey=rk, sig_idx=si, sig_val=sv, tfm_pca_rig=tfm)
    return r


def run_oracle(case, filt=None, gen=None):
    """filt / gen: stand-ins for the oracle's two functions (tests/test_loopdet_edge_bars.py: the oracle with one line changed)"""
    from oracle import scancontext as SC

    filt = filt or (predict_filter if case.slow_oracle else SC.generate_spherical_points)
    keep, sel, pts = filt(case.job[0], case.job[1], case.job[2], case.lidar_range, case.job[3], case.job[4])
    r = dict(kf_keep=keep, n_out=len(sel), sel_idx=sel, pts_spherical=pts)
    if len(sel) and case.oracle_sc:
        with np.errstate(all="ignore"):  # 0 / 0 in sectors whose heights are all zero: NaN in every form, kept in
            rk, si, sv, tfm = (gen or SC.generate)(pts, case.lidar_range, case.num_s, case.num_r)
        r.update(ringkey=rk, sig_idx=si, sig_val=sv, tfm_pca_rig=tfm)
    return r


def run_device(ctx, case, **kw):
    from direct_stereo_slam_amd.ringdb import loop_descriptors_batch

    r = loop_descriptors_batch(ctx, [case.job], case.lidar_range, case.num_s, case.num_r, scancontext=not is_empty(case), **kw)[0]
    return strip_empty(r)


def strip_empty(r):
    """a device result as run_host shapes it: no ScanContext keys for an empty selection"""
    if int(r["n_out"]) == 0:
        r = {k: v for k, v in r.items() if k not in ("ringkey", "sig_idx", "sig_val", "tfm_pca_rig")}
    return r


_EMPTY = {}


def is_empty(case):
    """nothing survives the filter (predicted, not measured): the device call is made without descriptor outputs, which an empty
    selection refuses (tests/test_device_loopdet.py::test_point_filter_alone_and_degenerate_jobs)"""
    if case.name not in _EMPTY:
        _EMPTY[case.name] = len(predict_filter(case.job[0], case.job[1], case.job[2], case.lidar_range, case.job[3], case.job[4])[1]) == 0
    return _EMPTY[case.name]


# ---- a vectorised prediction of the filter (262 145 points take the oracle's Python loop 4.5 s) ---------------------------------------
def grid_dims(lidar_range):
    return int(np.floor(2 * lidar_range * 1.0)) + 1, int(np.floor(2 * lidar_range * 2.0)) + 1, int(np.floor(2 * lidar_range * 1.0)) + 1


def grid_cells(lidar_range):
    a, b, c = grid_dims(lidar_range)
    return a * b * c


def to_camera(cur_cw, xyz):
    cw = np.asarray(cur_cw, np.float64).reshape(3, 4)
    g = np.asarray(xyz, np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        return np.stack([((cw[r, 0] * g[:, 0] + cw[r, 1] * g[:, 1]) + cw[r, 2] * g[:, 2]) + cw[r, 3] for r in range(3)], 1)


def voxel_index(p, lidar_range):
    """cell of camera-frame points (n, 3) that lie inside the range"""
    vs0, vs1, _ = grid_dims(lidar_range)
    xi, yi, zi = np.floor((p[:, 0] + lidar_range) * 1.0), np.floor((p[:, 1] + lidar_range) * 2.0), np.floor((p[:, 2] + lidar_range) * 1.0)
    return (xi + yi * vs0 + zi * vs0 * vs1).astype(np.int64)


def predict_filter(kf_ids, kf_pose_wc, cur_cw, lidar_range, pt_kf_id, pt_xyz):
    """generate_spherical_points as array operations: the keyframe trim is the oracle's own, the winners of every voxel come from one
    lexicographic sort (voxel, y, index).  Equal to the oracle's loop on every case that runs both (test_loopdet_edges_ref.py)."""
    from oracle import scancontext as SC

    kf_keep = SC.generate_spherical_points(kf_ids, kf_pose_wc, cur_cw, lidar_range, [], np.zeros((0, 3)))[0]
    kept_ids = np.unique(np.asarray(kf_ids, np.int64)[kf_keep]) if len(kf_ids) else np.zeros(0, np.int64)
    p = to_camera(cur_cw, pt_xyz)
    with np.errstate(all="ignore"):
        inside = np.sqrt(p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1] + p[:, 2] * p[:, 2]) < lidar_range
    idx = np.flatnonzero(np.isin(np.asarray(pt_kf_id, np.int64), kept_ids) & inside)
    loc = voxel_index(p[idx], lidar_range)
    order = np.lexsort((idx, p[idx, 1] + 0.0, loc))  # (-0.0 + 0.0 = +0.0: the two zeros tie, as `<` has them)
    first = np.ones(len(order), bool)
    first[1:] = loc[order][1:] != loc[order][:-1]
    sel = idx[order][first]
    return kf_keep, sel.astype(np.int32), p[sel].reshape(-1, 3)


def aligned(h):
    """the PCA-aligned coordinates of a result's points, from its own tfm_pca_rig"""
    T = h["tfm_pca_rig"]
    return h["pts_spherical"] @ T[:3, :3].T + T[:3, 3]


def bins_of(h, case):
    """{(sector, ring): sig_val} of a result"""
    return {(int(i) // case.num_r, int(i) % case.num_r): float(v) for i, v in zip(h["sig_idx"], h["sig_val"])}


# ---- builders ------------------------------------------------------------------------------------------------------------------
def ident_job(xyz, pt_kf=None, kf_ids=(KF,), poses=None, cur_cw=EYE_CW):
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    kf_ids = np.asarray(kf_ids, np.int32)
    poses = np.zeros((len(kf_ids), 6)) if poses is None else np.asarray(poses, np.float64)
    pt_kf = np.full(len(xyz), KF, np.int32) if pt_kf is None else np.asarray(pt_kf, np.int32)
    return kf_ids, poses, np.asarray(cur_cw, np.float64), pt_kf, xyz


def case(name, job, lidar_range, reaches, num_s=60, num_r=20, oracle_sc=True, slow_oracle=False):
    return Case(name, job, float(lidar_range), num_s, num_r, oracle_sc, slow_oracle, reaches)


# six points in general position inside range 2, each in a voxel of its own and away from the voxels the cases below name: they keep the
# ScanContext half of a filter case generic (separated eigenvalues, a non-zero mean)
BALLAST = np.array([[1.3, 0.7, -0.4], [-0.6, 1.1, 0.9], [0.4, -1.2, -1.1], [-1.4, 0.3, -0.7], [0.8, 0.9, 1.2], [-0.3, -0.8, 1.4]])
BALLAST2 = np.array([[-1.1, -0.6, 0.3], [0.5, 1.4, -0.6], [1.2, -0.9, 0.6], [-0.7, -1.3, -0.2], [0.2, 0.4, -1.6], [1.5, -0.2, -0.9]])  # six more, same rule
NX = float(np.nextafter(2.0, 0.0))
TRIMMED = [0.0, 0.9, 0.0]                # a keyframe rotated by 0.9 rad against the identity: trimmed (> 0.5)


def with_ballast(pts):
    return np.vstack([np.asarray(pts, np.float64).reshape(-1, 3), BALLAST])


def even_orbit(points):
    """the points and their images under (+,-,-), (-,+,-), (-,-,+), without repeats, every zero positive"""
    out, seen = [], set()
    for p in np.asarray(points, np.float64).reshape(-1, 3):
        for s in ((1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1)):
            q = tuple(float(v) for v in (p * s + 0.0))
            if q not in seen:
                seen.add(q)
                out.append(q)
    return np.array(out)


# range 10: a frame that fixes the order of the variances, x < y < z, whatever few test points join it: eig3_sym returns the identity and
# aligned = input.  Its own bins: sectors 0, 15, 30, 45, heights 0.
FRAME = even_orbit([[0, 0, 9.5], [0, 0, 8.5], [0, 0, 7.5], [0, 7.25, 0], [0, 6.25, 0]])


def framed(points):
    return np.vstack([even_orbit(points), FRAME])


def _tfm_is(h, mean):
    T = np.eye(4)
    T[:3, 3] = -np.asarray(mean, np.float64)
    return same_values(h["tfm_pca_rig"], T)


# ---- the cases -----------------------------------------------------------------------------------------------------------------
def _voxel_cases():
    t = 2.0 ** -40
    out = []

    def faces(h):  # 4 voxels from 5 points, in ascending cell order; points 0 and 1 share cell 106, point 0 is the higher one (lower y)
        assert list(h["sel_idx"][np.isin(h["sel_idx"], range(5))]) == [4, 3, 2, 0]
        assert list(voxel_index(h["pts_spherical"][np.isin(h["sel_idx"], range(5))], 2.0)) == [61, 101, 105, 106]
    out.append(case("voxel_faces", ident_job(with_ballast([[-1, -0.5, 0], [-1, -0.5 + t, 0], [-1 - t, -0.5, 0], [-1, -0.5 - t, 0], [-1, -0.5, -t]])), 2, faces))

    def sphere(h):  # norm exactly 2: dropped; one ulp inside: kept, in row vs - 1 (p + range rounds up to 2 * range) and in row 0 for -y
        s = h["sel_idx"][h["sel_idx"] < 8]
        assert list(s) == [4, 3, 7, 6, 5]
        assert list(voxel_index(h["pts_spherical"][h["sel_idx"] < 8], 2.0)) == [92, 114, 115, 132, 202]
        assert NX + 2.0 == 4.0 and grid_dims(2.0) == (5, 9, 5) and grid_cells(2.0) == 225
    out.append(case("range_sphere_and_last_row", ident_job(with_ballast([[2, 0, 0], [0, -2, 0], [0, 0, 2], [NX, 0, 0], [0, -NX, 0], [0, 0, NX], [0, NX, 0],
                                                                        [-1.5, 0.6, 0.5]])), 2, sphere))

    def zeros(first):
        def reach(h):  # the lower index wins the tie of the two zeros, and the emitted point keeps its own signs
            assert 0 in h["sel_idx"] and 1 not in h["sel_idx"]
            p = h["pts_spherical"][list(h["sel_idx"]).index(0)]
            assert np.all(p == 0) and np.all(np.signbit(p) == np.signbit(first))
        return reach
    pz, nz = np.zeros(3), -np.zeros(3)
    out.append(case("zeros_positive_first", ident_job(with_ballast([pz, nz]), cur_cw=NEGZERO_CW), 2, zeros(pz)))
    out.append(case("zeros_negative_first", ident_job(with_ballast([nz, pz]), cur_cw=NEGZERO_CW), 2, zeros(nz)))

    # three exact duplicates at indices 300, 600 and 700, in thread blocks 1 and 2 of 256 points (the points between them belong to no keyframe
    # of the window): whichever block's atomic arrives last, index 300 wins; and a lower y at a higher index, which wins over the lower index
    n = 701
    xyz = np.tile([[0.1, 0.1, 0.1]], (n, 1))
    pk = np.full(n, 999, np.int32)
    for i in (300, 600, 700):
        xyz[i], pk[i] = [0.25, 0.375, 0.25], KF
    xyz[10], xyz[20], pk[10], pk[20] = [-0.75, 0.25, -0.25], [-0.5, 0.125, -0.5], KF, KF
    for k, b in enumerate(BALLAST):
        xyz[100 + 70 * k], pk[100 + 70 * k] = b, KF

    def dups(h):
        s = set(int(i) for i in h["sel_idx"])
        assert 300 in s and not s & {600, 700} and 20 in s and 10 not in s and len(s) == 2 + len(BALLAST)
    out.append(case("duplicates_across_blocks_and_lower_y_later", ident_job(xyz, pk), 2, dups))
    return out


def dense_cloud(lidar_range, seed=0, limit=None, margin=0.0, fill_block=None):
    """one point at the centre of every voxel whose centre lies inside (range - margin), shuffled, the first `limit` of them.
    fill_block: all 256 cells of that compaction block get a point on top (not cut by the limit) -- the centre, or, where the centre
    lies outside the sphere, the cell's point nearest to the origin, which must lie inside."""
    vs0, vs1, vs2 = grid_dims(lidar_range)
    zi, yi, xi = np.meshgrid(np.arange(vs2), np.arange(vs1), np.arange(vs0), indexing="ij")
    lo = np.stack([xi.ravel() - lidar_range, yi.ravel() / 2.0 - lidar_range, zi.ravel() - lidar_range], 1)
    centre = lo + [0.5, 0.25, 0.5]
    inside = np.sqrt((centre * centre).sum(1)) < lidar_range - margin
    rng = np.random.default_rng(seed)
    if fill_block is None:
        return centre[inside][rng.permutation(inside.sum())][:limit]
    block = np.arange(256 * fill_block, 256 * fill_block + 256)
    near = np.clip(0.0, lo[block], lo[block] + [1.0, 0.5, 1.0] - 2.0 ** -10)
    filled = np.where(inside[block, None], centre[block], near)
    assert np.all(np.sqrt((filled * filled).sum(1)) < lidar_range)
    inside[block] = False
    cloud = np.vstack([centre[inside][rng.permutation(inside.sum())][:limit], filled])
    return cloud[rng.permutation(len(cloud))]


def _occupancy(h, lidar_range):
    occ = np.zeros(-(-grid_cells(lidar_range) // 256) * 256, bool)
    occ[voxel_index(h["pts_spherical"], lidar_range)] = True
    return occ


def _compaction_cases():
    out = []

    def dense(lidar_range, nblocks, per, limit=None, fill_block=None):
        cloud = dense_cloud(lidar_range, seed=int(lidar_range * 2), limit=limit, fill_block=fill_block)

        def reach(h):
            cells = grid_cells(lidar_range)
            assert -(-cells // 256) == nblocks and -(-nblocks // 256) == per
            assert h["n_out"] == len(cloud) and np.array_equal(np.sort(h["sel_idx"]), np.arange(len(cloud)))
            occ = _occupancy(h, lidar_range)
            per_block = occ.reshape(-1, 256).sum(1)
            if lidar_range == 7.5:  # no partial block, empty blocks.  (Where 2 * range is an integer the last cell of every row, x index vs0 - 1, needs
                # p0 >= range and stays empty: no block and -- rows being shorter than 64 cells -- no wave can be full.  Range 40.25 below has both.)
                assert cells == 7936 == 31 * 256 and len(cloud) == 3558 and per_block.max() > 200 and per_block.min() == 0
            if fill_block is not None:  # a block with 256 of 256 cells occupied: ballots of all ones in all four waves
                assert per_block[fill_block] == 256 and h["n_out"] > 20000
            if lidar_range == 16.0:
                assert per_block.max() > 200 and per_block.min() == 0  # (per = 2: scan threads 0 .. 138 own the 277 blocks, the others nothing)
            if lidar_range == 3.0:
                assert cells == 637 and cells % 256 == 125 and occ[512:637].any()
            if lidar_range == 16.0:
                assert cells == 70785 and nblocks == 277 and per == 2
        return case("dense_range_%g" % lidar_range, ident_job(cloud), lidar_range, reach)
    out += [dense(3.0, 3, 1), dense(7.5, 31, 1), dense(16.0, 277, 2), dense(40.0, 4127, 17, limit=20000),
            dense(40.25, 4152, 17, limit=20000, fill_block=2076)]

    # lidar_range 0.7: 2 x 3 x 2 cells, small enough for cell 0 and the last cell to lie inside the sphere
    def one_cell(cell):
        def reach(h):
            assert grid_cells(0.7) == 12 and h["n_out"] == 1 and list(voxel_index(h["pts_spherical"], 0.7)) == [cell]
        return reach
    out.append(case("single_point_cell_0", ident_job([[-0.25, -0.3125, -0.25]]), 0.7, one_cell(0), oracle_sc=False))  # one point: tied (zero) eigenvalues
    out.append(case("single_point_last_cell", ident_job([[0.375, 0.375, 0.375]]), 0.7, one_cell(11), oracle_sc=False))
    return out


MANY_N = 262145  # one more point than 1024 blocks of 256 threads cover: the second trip of the grid-stride loop


def _many_case():
    i = np.arange(MANY_N)
    v = i % 18
    base = np.stack([(v % 3) * 4.0 - 4.0, (v // 3 % 3) * 3.0 - 3.0, (v // 9) * 5.0 - 2.0], 1)  # 18 voxels, all inside range 16
    off = np.stack([(i * 5 % 7) / 8.0, (i * 7 % 5) / 16.0 + 0.125, (i * 3 % 4) / 4.0], 1)     # dyadic; y offset in [0.125, 0.375]: exact ties throughout
    xyz = base + off
    xyz[MANY_N - 1, 1] = base[MANY_N - 1, 1] + 0.0625                                      # the last point is the one winner of its voxel

    def reach(h):
        assert h["n_out"] == 18 and MANY_N - 1 in h["sel_idx"] and (MANY_N - 1) // 256 == 1024
        y = xyz[:, 1]
        assert all(np.sum((v == k) & (y == y[v == k].min())) > 1000 for k in range(18) if k != (MANY_N - 1) % 18)  # ties: the lowest index wins
    return case("many_points_few_voxels", ident_job(xyz), 16, reach, slow_oracle=True)


def _keyframe_cases():
    out = []
    pts = np.vstack([BALLAST, BALLAST2])
    imin, imax = np.iinfo(np.int32).min, np.iinfo(np.int32).max

    def kf_case(name, kf_ids, trimmed, pt_kf, expect):
        poses = np.zeros((len(kf_ids), 6))
        for k in trimmed:
            poses[k, 3:] = TRIMMED

        def reach(h):
            assert list(h["kf_keep"]) == [k not in trimmed for k in range(len(kf_ids))]
            assert sorted(int(i) for i in h["sel_idx"]) == sorted(expect + [i + 6 for i in expect])
        return case(name, ident_job(pts, pt_kf + pt_kf, kf_ids, poses), 2, reach)
    out.append(kf_case("no_keyframes_with_points", [], [], [1, 2, 3, 4, 5, 6], []))
    out.append(kf_case("every_keyframe_trimmed", [1, 2], [0, 1], [1, 2, 1, 2, 1, 2], []))
    out.append(kf_case("ids_int32_min_and_max", [imax, imin, 7], [2], [imin, imax, 7, 0, imin, imax], [0, 1, 4, 5]))
    out.append(kf_case("unsorted_ids", [9, 3, 7, 1], [2], [1, 7, 9, 3, 2, 7], [0, 2, 3]))
    out.append(kf_case("id_twice_trimmed_and_kept", [4, 8, 4, 8, 6], [0, 3, 4], [4, 8, 6, 4, 8, 6], [0, 1, 3, 4]))  # (trimmed, kept) and (kept, trimmed)
    out.append(kf_case("id_twice_trimmed_both_times", [4, 4, 6], [0, 1], [4, 6, 4, 6, 4, 6], [1, 3, 5]))
    return out


def _nonfinite_cases():
    bad = []
    for v in (np.nan, np.inf, -np.inf):
        for a in range(3):
            p = np.array([0.3, 0.3, 0.3])
            p[a] = v
            bad.append(p)
    bad += [np.array([1e308, 1e308, 0.0]), np.array([-1e308, 0.0, 1e308])]
    n = len(bad) + len(BALLAST)
    finite_at = np.arange(1, n, 3)[: len(BALLAST)]  # the finite points stand between the others
    xyz = np.zeros((n, 3))
    mask = np.zeros(n, bool)
    mask[finite_at] = True
    xyz[mask], xyz[~mask] = BALLAST, np.array(bad)
    out = []
    c, s = np.cos(0.1), np.sin(0.1)
    rot = np.array([[c, 0.0, s, 0.05], [0.0, 1.0, 0.0, -0.02], [-s, 0.0, c, 0.03]])  # 0.1 rad about y (kept): c * inf stays inf, the zeros of the rows make NaN
    for name, cw in (("nonfinite_points", EYE_CW), ("nonfinite_points_rotated", rot)):
        def reach(h, cw=cw, name=name):
            c0 = case(name, ident_job(xyz[mask], cur_cw=cw), 2, None)
            ref = run_host(c0)  # the finite points alone: the same result, indices renumbered
            assert ref["n_out"] == len(BALLAST) == h["n_out"]
            assert np.array_equal(finite_at[ref["sel_idx"]], h["sel_idx"]) and same_bits(ref["pts_spherical"], h["pts_spherical"])
            for k in ("ringkey", "sig_val", "tfm_pca_rig"):
                assert same_bits(ref[k], h[k]), k
            p = to_camera(cw, xyz[~mask])
            assert np.isnan(p).any(1).sum() >= 9  # 0 * inf in to_camera: the inf points arrive as NaN as well
        out.append(case(name, ident_job(xyz, cur_cw=cw), 2, reach))
    return out


MOMENT_SIZES = (1, 2, 3, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 3073)


def _moment_cases():
    cloud = dense_cloud(7.5, seed=15, margin=0.3)
    jitter = np.random.default_rng(16).uniform(-1, 1, cloud.shape) * [0.2, 0.1, 0.2]  # inside the voxel, not dyadic: the summation order matters
    cloud = cloud + jitter
    assert len(cloud) >= max(MOMENT_SIZES)
    out = []
    for n in MOMENT_SIZES:
        def reach(h, n=n):
            assert h["n_out"] == n
        out.append(case("moments_n%d" % n, ident_job(cloud[:n]), 7.5, reach, oracle_sc=n > 3))  # n <= 3: rank < 3, tied zero eigenvalues
    return out


def _pca_cases():
    out = []

    def axes6(h):  # covariance 18 * I: V is exactly the identity
        assert h["n_out"] == 6 and _tfm_is(h, [0, 0, 0])
        assert set(bins_of(h, out[0])) == {(0, 0), (0, 6), (15, 6), (30, 6), (45, 6)}
    out.append(case("pca_six_axis_points", ident_job([[3, 0, 0], [-3, 0, 0], [0, 3, 0], [0, -3, 0], [0, 0, 3], [0, 0, -3]]), 10, axes6, oracle_sc=False))

    rng = np.random.default_rng(31)
    plane = np.round(rng.uniform(-6, 6, (40, 3)) * 8) / 8
    plane[:, 0] = 0.25

    def planar(h):  # an exactly zero eigenvalue, its vector exactly the x axis; every height a zero: 0 / 0 in every sector
        assert h["n_out"] > 20 and np.all(h["tfm_pca_rig"][0, :3] == [1, 0, 0]) and np.all(np.isnan(h["sig_val"]))
    out.append(case("pca_planar", ident_job(plane), 10, planar))

    line = np.zeros((9, 3))
    line[:, 2] = [-7.3, -5.1, -2.2, -0.4, 1.7, 3.3, 4.9, 6.1, 8.4]
    out.append(case("pca_collinear", ident_job(line), 10, lambda h: _assert(h["n_out"] == 9 and np.all(h["pts_spherical"][:, :2] == 0)), oracle_sc=False))
    out.append(case("pca_one_point", ident_job([[1.25, -0.5, 2.0]]), 10, lambda h: _assert(h["n_out"] == 1 and _tfm_is(h, [1.25, -0.5, 2.0])), oracle_sc=False))
    out.append(case("pca_two_points", ident_job([[1.25, -0.5, 2.0], [-3.5, 1.0, 0.25]]), 10, lambda h: _assert(h["n_out"] == 2), oracle_sc=False))

    # a balanced dyadic cloud with variances 12 < 82 < 240, turned by 45 degrees about x (and stretched by sqrt 2: still dyadic): the two
    # diagonal entries of the first rotation are equal, theta = 0, t = 1
    base = even_orbit([[1, 2, 5], [1, 4, 3], [1, 1.5, 6], [0, 0.5, 1], [0, 3.5, 2]])
    turned = np.stack([base[:, 0], base[:, 1] - base[:, 2], base[:, 1] + base[:, 2]], 1)

    def rot45(h):
        p = h["pts_spherical"]
        assert h["n_out"] == len(turned) and np.all(p.sum(0) == 0)
        cov = p.T @ p
        assert cov[1, 1] == cov[2, 2] and cov[1, 2] != 0 and cov[0, 1] == 0 == cov[0, 2]
        assert abs(abs(h["tfm_pca_rig"][1, 1]) - np.sqrt(0.5)) < 1e-15
    out.append(case("pca_turned_45_degrees", ident_job(turned), 10, rot45))

    e = 2.0 ** -24  # sum z^2 = 32 + 2^-47: one ulp above sum y^2 = 32

    def close(h):
        p = h["pts_spherical"]
        cov = p.T @ p
        assert h["n_out"] == 8 and cov[2, 2] == np.nextafter(32.0, 64.0) and cov[1, 1] == 32.0 and _tfm_is(h, [0, 0, 0])
    out.append(case("pca_eigenvalues_one_ulp_apart", ident_job([[1, 0, 0], [-1, 0, 0], [0, 4, 0], [0, -4, 0], [0, 0, 4], [0, 0, -4], [0, 0, e], [0, 0, -e]]), 10, close,
                    oracle_sc=False))

    far = np.array([0.0, 0.0, 9.0]) + rng.uniform(-1, 1, (200, 3)) * [1.5, 0.9, 0.8]

    def far_reach(h):
        assert h["n_out"] > 10 and np.linalg.norm(h["pts_spherical"].mean(0)) > 0.85 * 10
    out.append(case("pca_far_from_origin", ident_job(far), 10, far_reach))
    return out


def _assert(ok):
    assert ok


def _polar_cases():
    out = []

    def polar(name, points, reach, mean=(0, 0, 0), frame=True, **kw):
        pts = framed(points) if frame else np.asarray(points, np.float64)
        pts = pts + np.asarray(mean, np.float64)

        def full(h):
            assert h["n_out"] == len(pts), "every point in a voxel of its own"
            assert _tfm_is(h, mean), "exact mean, V = identity: aligned = input - mean"
            reach(h, bins_of(h, c))
        c = case(name, ident_job(pts), 10, full, **kw)
        out.append(c)

    def edges(h, b):  # theta = 0, pi/2, pi, 3 pi/2 exactly: sectors 0, 15, 30, 45 (3 * fl(pi/2) is a double, so 3 pi/2 / 2 pi = 0.75)
        for s in (0, 15, 30, 45):
            assert b[(s, 6)] > 0, (s, b)
    polar("polar_sector_edges", [[1, 3, 0], [2, 0, 3]], edges)

    tiny = 2.0 ** -50

    def wrap(h, b):  # (1, 4, -tiny): theta = -2^-52, theta + 2 pi rounds to 2 pi, the second loop makes it 0: sector 0, where its height 1 beats -1
        th = np.arctan2(-tiny, 4.0)
        assert th < 0 and th + 2 * np.pi == 2 * np.pi
        assert b[(0, 8)] > 0 and b[(30, 8)] > 0
    polar("polar_theta_rounds_to_two_pi", [[1, 4, -tiny]], wrap)

    def rings(h, b):  # rho = k * range / num_r for k = 1 .. 19 in sector 15: whatever ring rho / range * num_r truncates to, the same in every form
        rho = np.abs(aligned(h)[:, 2])
        assert all((rho == 0.5 * k).sum() == 4 for k in range(1, 20)) and len([r for (s, r) in b if s == 15]) >= 18
    polar("polar_ring_edges", np.vstack([even_orbit([[0.5 + k % 2, 0, 0.5 * k] for k in range(1, 20)]), even_orbit([[0, 7.25, 0], [0, 6.25, 0], [0, 5.25, 0]])]),
          rings, frame=False)

    def recentred(h, b):  # mean (0, 0, -2): the points (+-1, 0, 8) lie inside the range and at rho = 10 = range after recentring: dropped
        assert not any(s == 15 for (s, r) in b) and len(b) == 4 and np.abs(aligned(h)[:, 2]).max() == 10.0
    polar("polar_rho_at_range_after_recentring",
          [[1, 0, 10], [-1, 0, 10]] + [[sx, sy * y, -2.5] for y in (2, 3) for sx in (1, -1) for sy in (1, -1)], recentred, mean=(0, 0, -2), frame=False)

    def equal(h, b):  # two points of height 1 in bin (7, 16), from two voxels; their partners of height -1 alone in bins (52, 16) and (22, 16)
        assert b[(7, 16)] > 0 and b[(52, 16)] < 0 and b[(22, 16)] < 0 and b[(37, 16)] > 0 and len([k for k in b if k[1] == 16]) == 4
    polar("polar_equal_heights_in_one_bin", [[1, 5.75, 5.75], [1, 5.625, 6.125]], equal)
    polar("polar_bin_with_negative_heights_only", [[1.5, 2.5, 6.0]], lambda h, b: _assert(sum(v < 0 for v in b.values()) == 2 and sum(v > 0 for v in b.values()) == 2))

    ring = [[6, 7], [6, -7], [-6, 7], [-6, -7], [8, 0], [-8, 0], [0, 9], [0, -9], [0, 5], [0, -5], [4, 0], [-4, 0]]

    def at_threshold(h, b):  # height exactly -range in bin (0, 0): occupied
        assert aligned(h)[:, 0].min() == -10.0 and b[(0, 0)] < 0
    polar("polar_height_exactly_minus_range", [[-10, 0, 0]] + [[1, y, z] for y, z in ring[:10]], at_threshold, mean=(1, 0, 0), frame=False)

    def touched(h, b):  # height -10.5 in (-range - 1, -range): the bin is written and still counts as empty
        assert aligned(h)[:, 0].min() == -10.5 and (0, 0) not in b and len(b) == 12
    polar("polar_height_between_init_and_threshold", [[-10.5, 0, 0]] + [[0.875, y, z] for y, z in ring], touched, mean=(1, 0, 0), frame=False)

    def below(h, b):  # height -11.5 below the initial -range - 1: the bin keeps its initial value
        assert aligned(h)[:, 0].min() == -11.5 and (0, 0) not in b and len(b) == 8
    polar("polar_height_below_initial_value", [[-11.5, 0, 0]] + [[1.4375, y, z] for y, z in ring[:8]], below, mean=(2, 0, 0), frame=False)

    # reading 3 of the issue: a bin that holds only a -0.0 height, in a sector whose norm is not zero.  Host: -0.0 / norm = -0.0; device: the
    # zero was made positive before the atomic max.  Compared with the host form only (by value); the oracle's matrix product loses the sign.
    nz = np.vstack([framed([[1, 1.5, 2]]), [[-0.0, -3, -4], [0.0, 3, 4], [0.0, -3, 4], [0.0, 3, -4]]])

    def negzero(h):
        assert h["n_out"] == len(nz) and _tfm_is(h, [0, 0, 0])
        z = h["sig_val"][h["sig_val"] == 0]
        assert len(z) >= 1 and np.signbit(z).any(), "the host form keeps the sign of a -0.0 height"
    out.append(case("polar_negative_zero_height", ident_job(nz, cur_cw=NEGZERO_CW), 10, negzero, oracle_sc=False))
    return out


SHAPES = ((1, 1), (7, 3), (64, 64), (256, 1), (1, 256), (256, 256))


def generic_job(seed=41, n=500, lidar_range=10.0):
    """a cloud in general position under a pose that is not the identity, two keyframes, one of them trimmed"""
    rng = np.random.default_rng(seed)
    c, s = np.cos(0.2), np.sin(0.2)
    cw = np.array([[c, -s, 0.0, 0.3], [s, c, 0.0, -0.1], [0.0, 0.0, 1.0, 0.2]])
    xyz = rng.normal(0, 1, (n, 3)) * [0.45, 0.2, 0.5] * lidar_range
    poses = np.zeros((2, 6))
    poses[0, 3:], poses[1, 3:] = [0.0, 0.0, -0.15], [0.3, 0.8, 0.0]
    return np.array([11, 12], np.int32), poses, cw, rng.choice([11, 11, 11, 12], n).astype(np.int32), xyz


def _shape_cases():
    job = generic_job()
    return [case("shape_%dx%d" % (ns, nr), job, 10, lambda h: _assert(50 < h["n_out"] < 500), num_s=ns, num_r=nr) for ns, nr in SHAPES]


def all_cases():
    out = (_voxel_cases() + _compaction_cases() + [_many_case()] + _keyframe_cases() + _nonfinite_cases() + _moment_cases() + _pca_cases() + _polar_cases()
           + _shape_cases())
    assert len({c.name for c in out}) == len(out)
    return out


CASES = all_cases()
BY_NAME = {c.name: c for c in CASES}
