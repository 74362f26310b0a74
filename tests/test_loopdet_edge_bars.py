"""The edge cases of tests/_loopdet_cases.py bite: oracle/scancontext.py restated here with ONE line changed must be rejected by
assert_same on a named case (the same comparison, at the same bars, that holds the device form in tests/test_loopdet_edges.py).
The unchanged restatement passes every case.  No GPU."""
import math

import numpy as np
import pytest

import _loopdet_cases as LC
from oracle import scancontext as SC


def generate_spherical_points(kf_ids, kf_pose_wc, cur_cw, lidar_range, pt_kf_id, pt_xyz, v=""):
    """oracle/scancontext.py:generate_spherical_points; the keyframe trim is the oracle's own.  The per-point loop is written over arrays
    (the 262 145-point case), the winner rule stays the oracle's `loc not in best or p[1] < best[loc][1]`, taken voxel by voxel."""
    kf_keep = SC.generate_spherical_points(kf_ids, kf_pose_wc, cur_cw, lidar_range, [], np.zeros((0, 3)))[0]
    keep = {}
    for i, k in enumerate(kf_ids):
        if v == "the trimmed entry wins for a doubled id":
            keep[int(k)] = keep.get(int(k), True) and bool(kf_keep[i])
        else:
            keep[int(k)] = keep.get(int(k), False) or bool(kf_keep[i])
    steps = (1.0, 2.0, 1.0)
    plus = 0 if v == "vs without the + 1" else 1
    vs0 = int(np.floor(2 * lidar_range * steps[0])) + plus
    vs1 = int(np.floor(2 * lidar_range * steps[1])) + plus
    p = LC.to_camera(cur_cw, pt_xyz)
    with np.errstate(all="ignore"):
        norm = np.sqrt(p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1] + p[:, 2] * p[:, 2])
    inside = norm <= lidar_range if v == "> for >= at the range" else norm < lidar_range
    known = np.array([keep.get(int(k), False) for k in np.unique(pt_kf_id)], bool)
    idx = np.flatnonzero(known[np.searchsorted(np.unique(pt_kf_id), pt_kf_id)] & inside) if len(p) else np.zeros(0, np.int64)
    if v == "a point lost at index 262 144":
        idx = idx[idx != 262144]
    rnd = np.trunc if v == "truncation for floor" else np.floor
    xi, yi, zi = (rnd((p[idx, a] + lidar_range) * steps[a]).astype(np.int64) for a in range(3))
    loc = xi + yi * vs0 + zi * vs0 * vs1
    best = {}
    for i, l in zip(idx, loc):
        if l not in best:
            best[l] = i
        elif v == "the last index wins a tie":
            if p[i, 1] <= p[best[l], 1]:
                best[l] = i
        elif v == "-0.0 < +0.0 in the tie":
            if p[i, 1] < p[best[l], 1] or (p[i, 1] == 0 and p[best[l], 1] == 0 and np.signbit(p[i, 1]) and not np.signbit(p[best[l], 1])):
                best[l] = i
        elif p[i, 1] < p[best[l], 1]:
            best[l] = i
    sel = np.array([best[l] for l in sorted(best)], np.int32)
    return kf_keep, sel, p[sel].reshape(-1, 3)


def generate(pts, lidar_range, num_s=60, num_r=20, v=""):
    """oracle/scancontext.py:align_points_pca and generate"""
    pts = np.asarray(pts, np.float64)
    mean = pts.sum(0) / len(pts)
    mat = pts - mean
    if v == "a covariance that drops the last partial lane":
        full = len(mat) // 256 * 256
        cov = mat[:full].T @ mat[:full]
    else:
        cov = mat.T @ mat
    w, V = np.linalg.eigh(cov)
    for c in range(3):
        if V[np.argmax(np.abs(V[:, c])), c] < 0:
            V[:, c] = -V[:, c]
    aligned = mat @ V
    tfm = np.eye(4)
    tfm[:3, :3] = V.T
    tfm[:3, 3] = -V.T @ mean
    ringkey = np.zeros(num_r, np.float32)
    max_height = np.full(num_s * num_r + (1 if v == "ri > num_r for >=" else 0), -lidar_range - 1.0)  # (one cell of slack: the variant's last bin)
    for x, y, z in aligned:
        rho = math.sqrt(y * y + z * z)
        theta = math.atan2(z, y)
        while theta < 0:
            theta += 2.0 * math.pi
        while theta >= 2.0 * math.pi and v != "the missing second while on theta":
            theta -= 2.0 * math.pi
        si = int(theta / (2.0 * math.pi) * num_s)
        ri = int(rho / lidar_range * num_r)
        if (ri > num_r if v == "ri > num_r for >=" else ri >= num_r) or si >= num_s:
            continue
        max_height[si * num_r + ri] = max(max_height[si * num_r + ri], x)
    max_height = max_height[: num_s * num_r]
    idx = np.nonzero(max_height > -lidar_range if v == "> for >= at the -range threshold" else max_height >= -lidar_range)[0]
    for i in idx:
        ringkey[i % num_r] += np.float32(1.0)
    val = max_height[idx].copy()
    norm = np.zeros(num_s)
    for i, h in zip(idx, val):
        norm[i // num_r] += h * h
    ringkey = ringkey / np.float32(num_s)
    norm = np.sqrt(norm)
    val = val / norm[idx // num_r]
    return ringkey.astype(np.float32), idx.astype(np.int32), val, tfm


def restated(case, v=""):
    return LC.run_oracle(case, filt=lambda *a: generate_spherical_points(*a, v=v), gen=lambda *a: generate(*a, v=v))


@pytest.fixture(scope="module")
def host(built):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = LC.run_host(LC.BY_NAME[name])
        return cache[name]
    return get


@pytest.mark.parametrize("case", LC.CASES, ids=[c.name for c in LC.CASES])
def test_unchanged_restatement_is_the_oracle(host, case):
    r = restated(case)
    LC.assert_same(host(case.name), oracle=r, oracle_sc=case.oracle_sc)
    if not case.slow_oracle:
        o = LC.run_oracle(case)
        assert set(o) == set(r)
        for k in o:
            assert LC.same_bits(np.asarray(o[k], np.float64), np.asarray(r[k], np.float64)), k


# variant -> the case that rejects it
VARIANTS = {
    "the last index wins a tie": "duplicates_across_blocks_and_lower_y_later",
    "-0.0 < +0.0 in the tie": "zeros_positive_first",
    "> for >= at the range": "range_sphere_and_last_row",
    "vs without the + 1": "range_sphere_and_last_row",
    "a point lost at index 262 144": "many_points_few_voxels",
    "ri > num_r for >=": "polar_rho_at_range_after_recentring",
    "> for >= at the -range threshold": "polar_height_exactly_minus_range",
    "the missing second while on theta": "polar_theta_rounds_to_two_pi",
    "the trimmed entry wins for a doubled id": "id_twice_trimmed_and_kept",
    "a covariance that drops the last partial lane": "moments_n257",
}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_variant_is_rejected_by_its_named_case(host, variant):
    case = LC.BY_NAME[VARIANTS[variant]]
    assert case.oracle_sc
    with pytest.raises(AssertionError):
        LC.assert_same(host(case.name), oracle=restated(case, variant))


def test_truncation_for_floor_cannot_be_told_apart():
    """`truncation for floor` in the voxel index is the one variant no case can reject: a point that passes the range test has
    |p| < range in every coordinate, so p + range >= 0 and floor and truncation agree -- on the device as well, where the cast to a
    64-bit integer after floor truncates a value that floor already made integral.  Asserted here over every case, so that a case
    which one day tells them apart shows up."""
    for case in LC.CASES:
        if case.slow_oracle:
            continue
        p = LC.to_camera(case.job[2], case.job[4])
        with np.errstate(all="ignore"):
            inside = np.sqrt(p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1] + p[:, 2] * p[:, 2]) < case.lidar_range
        assert np.all(p[inside] + case.lidar_range >= 0)
        a, b = restated(case), restated(case, "truncation for floor")
        assert np.array_equal(a["sel_idx"], b["sel_idx"])
