"""The named edge cases of tests/_loopdet_cases.py on the HOST forms of the loop descriptors (dsm_generate_spherical_points,
dsm_scancontext_generate: csrc/host_capi.cpp) against the numpy oracle (oracle/scancontext.py), through the comparison the device
test uses (assert_same), and each case's assertion that it reaches the edge it is named for.  No GPU."""
import numpy as np
import pytest

import _loopdet_cases as LC
from oracle import scancontext as SC


@pytest.fixture(scope="module")
def host(built):
    cache = {}

    def get(case):
        if case.name not in cache:
            cache[case.name] = LC.run_host(case)
        return cache[case.name]
    return get


@pytest.mark.parametrize("case", LC.CASES, ids=[c.name for c in LC.CASES])
def test_case_reaches_its_edge_and_host_equals_oracle(host, case):
    h = host(case)
    case.reaches(h)
    LC.assert_same(h, oracle=LC.run_oracle(case), oracle_sc=case.oracle_sc)
    if not case.slow_oracle:  # the vectorised prediction the device test uses for the 262 145-point cloud: equal to the oracle's loop
        keep, sel, pts = LC.predict_filter(case.job[0], case.job[1], case.job[2], case.lidar_range, case.job[3], case.job[4])
        keep_o, sel_o, pts_o = SC.generate_spherical_points(case.job[0], case.job[1], case.job[2], case.lidar_range, case.job[3], case.job[4])
        assert np.array_equal(keep, keep_o) and np.array_equal(sel, sel_o) and LC.same_bits(pts, pts_o)


def test_the_oracle_is_left_out_by_name_only():
    """tied eigenvalues (LAPACK's vectors are arbitrary there) and the negative-zero height, nothing else"""
    left_out = {c.name for c in LC.CASES if not c.oracle_sc}
    assert left_out == {"single_point_cell_0", "single_point_last_cell", "moments_n1", "moments_n2", "moments_n3", "pca_six_axis_points", "pca_collinear",
                        "pca_one_point", "pca_two_points", "pca_eigenvalues_one_ulp_apart", "polar_negative_zero_height"}


def test_comparison_sees_what_it_should_and_no_more():
    a = dict(kf_keep=np.array([True]), n_out=1, sel_idx=np.array([0], np.int32), pts_spherical=np.array([[0.0, -0.0, np.nan]]),
             ringkey=np.array([0.5], np.float32), sig_idx=np.array([0, 1], np.int32), sig_val=np.array([0.0, np.nan]), tfm_pca_rig=np.eye(4))
    b = {k: np.copy(v) for k, v in a.items()}
    b["sig_val"][0] = -0.0                      # the sign of a zero in sig_val: no part of the contract
    LC.assert_same(a, b)
    b["pts_spherical"][0, 0] = -0.0             # ... in a selected point: seen
    with pytest.raises(AssertionError):
        LC.assert_same(a, b)
    b = {k: np.copy(v) for k, v in a.items()}
    b["tfm_pca_rig"][1, 2] = -0.0
    with pytest.raises(AssertionError):
        LC.assert_same(a, b)
    b = {k: np.copy(v) for k, v in a.items()}
    b["sig_val"][1] = 1.0
    with pytest.raises(AssertionError):
        LC.assert_same(a, b)
    o = {k: np.copy(v) for k, v in a.items()}
    o["tfm_pca_rig"][0, 3] = 2e-9
    with pytest.raises(AssertionError):
        LC.assert_same(a, oracle=o)
    o["tfm_pca_rig"][0, 3] = 5e-10
    LC.assert_same(a, oracle=o)
