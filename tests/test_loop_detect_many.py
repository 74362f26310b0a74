"""dsm_loop_detect_batch_many: the fused loop chain with one index per job -- descriptors, candidates and index contents equal, per
job in order, dsm_loop_descriptors_batch of that job followed by search_ringkey on the job's own index."""
import numpy as np
import pytest

from direct_stereo_slam_amd.ringdb import RingKeyDB, loop_descriptors_batch

from test_device_loopdet import make_job

pytestmark = pytest.mark.gpu


def _sequential(ctx, jobs, twins):
    out = []
    for job, db in zip(jobs, twins):
        r = loop_descriptors_batch(ctx, [job], 40.0)[0]
        r["candidates"] = db.search_ringkey(r["ringkey"])
        out.append(r)
    return out


def _assert_same(seq, fus):
    for a, f in zip(seq, fus):
        assert a["candidates"] == f["candidates"]
        for key in ("ringkey", "sig_idx", "sig_val", "tfm_pca_rig", "kf_keep"):
            assert np.array_equal(a[key], f[key]), key
        assert a["n_out"] == f["n_out"]
        if "sel_idx" in f:
            assert np.array_equal(a["sel_idx"], f["sel_idx"]) and np.array_equal(a["pts_spherical"], f["pts_spherical"])


def _same_indexes(pairs, probe):
    for db, twin in pairs:
        assert db.size() == twin.size()
        assert np.array_equal(db.knn_packed_host(probe), twin.knn_packed_host(probe))


def test_sixty_four_sequences_each_with_its_own_index(ctx):
    places = [make_job(700 + s, n_kf=6, n_pts=2500) for s in range(16)]
    keys = np.stack([r["ringkey"] for r in loop_descriptors_batch(ctx, places, 40.0, selected_points=False)])
    rng = np.random.default_rng(2)
    # every sequence's index already knows a few of the places (as many keyframes as a short run), in its own order
    dbs, twins = [], []
    for s in range(64):
        known = keys[rng.permutation(16)[: 2 + s % 7]]
        filler = (rng.integers(0, 61, (50 + 40 * (s % 5), 20)) / 60.0).astype(np.float32)
        pair = [RingKeyDB(ctx, capacity=1024, margin=2) for _ in range(2)]
        for db in pair:
            db.add_points(np.concatenate([filler, known]))
            for _ in range(2):  # a full delay queue: every call matures one key per index
                db.enqueue(filler[0])
        dbs.append(pair[0])
        twins.append(pair[1])
    jobs = []
    for s in range(64):
        kf_ids, poses, cur_cw, pt_kf, xyz = places[(5 * s) % 16]
        jobs.append((kf_ids, poses, cur_cw, pt_kf, xyz + rng.normal(0, 0.002, xyz.shape)))
    for rep in range(2):
        fus = loop_descriptors_batch(ctx, jobs, 40.0, dbs=dbs, selected_points=(rep == 0))
        seq = _sequential(ctx, jobs, twins)
        _assert_same(seq, fus)
        assert sum(bool(r["candidates"]) for r in fus) > 8
    _same_indexes(zip(dbs, twins), keys[:8])


def test_repeated_indexes_and_short_margins(ctx):
    """four sequences; some advances marginalise two or three keyframes of one sequence, some none of another; margins 3 and 4 so
    that keys mature inside calls and the later jobs of an index see them"""
    rng = np.random.default_rng(7)
    places = [make_job(300 + s, n_pts=3000 + 200 * (s % 5)) for s in range(10)]
    margins = (3, 4, 3, 4)
    pairs = [[RingKeyDB(ctx, capacity=64, margin=m) for _ in range(2)] for m in margins]
    keys = np.stack([r["ringkey"] for r in loop_descriptors_batch(ctx, places, 40.0, selected_points=False)])
    for pair in pairs:  # each sequence has seen half of the places before, in its own order
        seen = keys[rng.permutation(len(places))[:5]]
        for db in pair:
            db.add_points(seen)
    owners = [[0, 1, 2, 3], [0, 0, 1], [2, 2, 2, 3, 1], [3, 0], [1, 1, 0, 0, 2, 3], [3, 3, 3], [0, 1, 2, 3, 0], [2, 1, 1, 0]]
    seq_all, fus_all = [], []
    for owner in owners:
        jobs = []
        for _ in owner:
            kf_ids, poses, cur_cw, pt_kf, xyz = places[rng.integers(len(places))]
            jobs.append((kf_ids, poses, cur_cw, pt_kf, xyz + rng.normal(0, 0.003, xyz.shape)))
        fus = loop_descriptors_batch(ctx, jobs, 40.0, dbs=[pairs[o][0] for o in owner])
        seq = _sequential(ctx, jobs, [pairs[o][1] for o in owner])
        _assert_same(seq, fus)
        seq_all += seq
        fus_all += fus
    assert sum(bool(r["candidates"]) for r in fus_all) > 5, "the scenario must produce loop candidates"
    probe = np.stack([r["ringkey"] for r in seq_all[:8]])
    _same_indexes(pairs, probe)


def test_empty_cloud_leaves_everything_untouched(ctx):
    jobs = [make_job(400 + s, n_kf=6, n_pts=2000) for s in range(3)]
    pairs = [[RingKeyDB(ctx, capacity=64, margin=2) for _ in range(2)] for _ in range(3)]
    warm = loop_descriptors_batch(ctx, jobs, 40.0, dbs=[p[0] for p in pairs])
    _sequential(ctx, jobs, [p[1] for p in pairs])
    probe = np.stack([r["ringkey"] for r in warm])
    before = [(p[0].size(), p[0].knn_packed_host(probe)) for p in pairs]
    kf_ids, poses, cur_cw, pt_kf, xyz = jobs[1]
    empty = (kf_ids, poses, cur_cw, pt_kf, xyz + 1000.0)  # every point beyond lidar_range: nothing survives the filter
    from direct_stereo_slam_amd._lib import DsmError

    with pytest.raises(DsmError):
        loop_descriptors_batch(ctx, [jobs[0], empty, jobs[2], jobs[0]], 40.0, dbs=[p[0] for p in pairs] + [pairs[0][0]])
    for p, (size, packed) in zip(pairs, before):
        assert p[0].size() == size and np.array_equal(p[0].knn_packed_host(probe), packed)
    # the delay queues did not move: the next calls still agree with the twins
    for _ in range(2):
        fus = loop_descriptors_batch(ctx, jobs, 40.0, dbs=[p[0] for p in pairs])
        _assert_same(_sequential(ctx, jobs, [p[1] for p in pairs]), fus)
    _same_indexes(pairs, probe)
