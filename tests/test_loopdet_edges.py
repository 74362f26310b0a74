"""The twelve kernels of csrc/loopdet_kernels.hip at their edges: every named case of tests/_loopdet_cases.py through
dsm_loop_descriptors_batch -- alone, in batches, in mixed batches, from page-locked clouds -- against the host forms (bit for bit;
sig_val by value) and the numpy oracle (selection and ring key exact, sig_val 1e-9, tfm_pca_rig 1e-9).  That the cases reach their
edges and that the comparison rejects a form which gets one of them wrong is shown without a GPU (test_loopdet_edges_ref.py,
test_loopdet_edge_bars.py)."""
import numpy as np
import pytest

import _loopdet_cases as LC
from direct_stereo_slam_amd._lib import DsmError
from direct_stereo_slam_amd.ringdb import LoopBatch, RingKeyDB, loop_descriptors_batch

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def refs(built):
    """host form and oracle of every case, computed once"""
    cache = {}

    def get(case):
        if case.name not in cache:
            cache[case.name] = (LC.run_host(case), LC.run_oracle(case))
        return cache[case.name]
    return get


@pytest.fixture(scope="module")
def solo(ctx):
    """the device result of every case run alone, computed once"""
    cache = {}

    def get(case):
        if case.name not in cache:
            cache[case.name] = LC.run_device(ctx, case)
        return cache[case.name]
    return get


def worst(got, oracle, key):
    a, b = np.asarray(got[key], np.float64), np.asarray(oracle[key], np.float64)
    d = np.abs(a - b)[~(np.isnan(a) & np.isnan(b))]
    return float(d.max()) if d.size else 0.0


@pytest.mark.parametrize("case", LC.CASES, ids=[c.name for c in LC.CASES])
def test_case_alone_equals_host_form_and_oracle(solo, refs, case):
    host, oracle = refs(case)
    got = solo(case)
    if case.oracle_sc and "sig_val" in oracle and "sig_val" in got and len(got["sig_val"]) == len(oracle["sig_val"]):
        print("device-vs-oracle %s sig_val %.3e tfm_pca_rig %.3e" % (case.name, worst(got, oracle, "sig_val"), worst(got, oracle, "tfm_pca_rig")))
    LC.assert_same(got, host, oracle=oracle, oracle_sc=case.oracle_sc)


def _groups():
    """the small cases that share (lidar_range, num_s, num_r, empty or not): one batch each"""
    g = {}
    for c in LC.CASES:
        if len(c.job[4]) <= 4000:
            g.setdefault((c.lidar_range, c.num_s, c.num_r, LC.is_empty(c)), []).append(c)
    return [v for v in g.values() if len(v) > 1]


GROUPS = _groups()


@pytest.mark.parametrize("group", GROUPS, ids=["range_%g_%dx%d%s_%d_jobs" % (g[0].lidar_range, g[0].num_s, g[0].num_r, "_empty" if LC.is_empty(g[0]) else "", len(g)) for g in GROUPS])
def test_batch_equals_each_case_alone(ctx, solo, group):
    c0 = group[0]
    res = loop_descriptors_batch(ctx, [c.job for c in group], c0.lidar_range, c0.num_s, c0.num_r, scancontext=not LC.is_empty(c0))
    for c, r in zip(group, res):
        a, b = LC.strip_empty(r), solo(c)
        LC.assert_same(a, b)
        if "sig_val" in b:
            assert LC.same_bits(a["sig_val"], b["sig_val"]), c.name  # one form, two launches: the zero signs too


def test_groups_cover_the_small_cases():
    assert sum(len(g) for g in GROUPS) >= 40 and {g[0].lidar_range for g in GROUPS} >= {2.0, 7.5, 10.0}


def clear_descriptors(batch, j):
    """LoopBatch sets the descriptor outputs for all jobs or for none; the C ABI takes them job by job"""
    for k in ("ringkey", "sig_idx", "sig_val", "n_sig", "tfm_pca_rig"):
        setattr(batch.arr[j], k, None)


def test_zero_points_one_point_and_262145_points_in_one_batch(ctx, solo, refs):
    many = LC.BY_NAME["many_points_few_voxels"]
    one = LC.case("one_point_range_16", LC.ident_job([[1.25, -0.5, 2.0]]), 16, None)
    none = LC.ident_job(np.zeros((0, 3)))
    b = LoopBatch(ctx, [none, one.job, many.job], 16.0)
    clear_descriptors(b, 0)  # an empty cloud has no descriptor: the job asks for none (the C ABI's mixed batch)
    b.run()
    r = b.results()
    assert r[0]["n_out"] == 0 and len(r[0]["sel_idx"]) == 0 and not b.outs[0][0]["ringkey"].any() and b.outs[0][0]["n_sig"][0] == 0
    LC.assert_same(r[1], LC.run_host(one))
    LC.assert_same(r[2], solo(many))
    LC.assert_same(r[2], refs(many)[0], oracle=refs(many)[1])


def test_mixed_batch_skips_the_job_without_descriptor_outputs(ctx, solo):
    """dsm_loop_descriptors_batch accepts jobs with and without descriptor outputs in one batch (C ABI, host/LoopDetection.hpp; the
    Python wrapper sets them for all jobs or for none).  Every sc_* kernel skips the job without: nothing is stored through its null
    ring-key pointer, its own point filter is complete, and its neighbours equal their solo runs."""
    names = ["polar_sector_edges", "polar_equal_heights_in_one_bin", "pca_far_from_origin", "polar_height_exactly_minus_range"]
    cases = [LC.BY_NAME[n] for n in names]
    for cleared in (0, 2, 3):
        b = LoopBatch(ctx, [c.job for c in cases], 10.0)
        clear_descriptors(b, cleared)
        b.run()
        for j, (c, r) in enumerate(zip(cases, b.results())):
            s = solo(c)
            if j != cleared:
                LC.assert_same(r, s)
                continue
            assert r["n_out"] == s["n_out"] and np.array_equal(r["sel_idx"], s["sel_idx"]) and LC.same_bits(r["pts_spherical"], s["pts_spherical"])
            o = b.outs[j][0]  # the caller's descriptor arrays of the cleared job: never written
            assert not o["ringkey"].any() and not o["sig_idx"].any() and not o["sig_val"].any() and o["n_sig"][0] == 0 and not o["tfm"].any()
    # the fused chain searches every job's key: it refuses a job without one before anything runs, so the zeroed key slot is never searched
    db = RingKeyDB(ctx, capacity=64, margin=8)
    size = db.size()
    b = LoopBatch(ctx, [c.job for c in cases], 10.0, db=db)
    clear_descriptors(b, 1)
    with pytest.raises(DsmError):
        b.run()
    assert all(int(o["n_out"][0]) == 0 for o, _ in b.outs) and db.size() == size


def test_small_call_after_a_large_one_reads_nothing_of_the_arena(ctx, solo):
    big, small = LC.BY_NAME["dense_range_40"], LC.BY_NAME["single_point_cell_0"]
    a = LC.run_device(ctx, big)
    b = LC.run_device(ctx, small)
    c = LC.run_device(ctx, LC.BY_NAME["pca_one_point"])
    LC.assert_same(a, solo(big))
    LC.assert_same(b, LC.run_host(small))
    LC.assert_same(c, LC.run_host(LC.BY_NAME["pca_one_point"]))


@pytest.mark.parametrize("name", ["zeros_positive_first", "zeros_negative_first", "polar_negative_zero_height"])
def test_negative_zeros_from_page_locked_clouds(ctx, solo, name):
    case = LC.BY_NAME[name]
    assert np.signbit(case.job[4][case.job[4] == 0]).any()
    LC.assert_same(LC.run_device(ctx, case, pinned_clouds=True), solo(case))
    LC.assert_same(solo(case), LC.run_host(case))


@pytest.mark.parametrize("num_s,num_r", [(257, 20), (60, 257), (257, 257)])
def test_shape_257_is_refused_with_nothing_written(ctx, num_s, num_r):
    b = LoopBatch(ctx, [LC.generic_job()], 10.0, num_s, num_r)
    with pytest.raises(DsmError):
        b.run()
    for v in b.outs[0][0].values():
        assert not v.any()
