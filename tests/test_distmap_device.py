"""GPU: dsm_distmaps_make, dsm_distmap_add and dsm_activate_points_batch against the checker tests/_distmap_ref.py -- every map and
every decision as exact equality."""
import numpy as np
import pytest

import _distmap_ref as R

pytestmark = pytest.mark.gpu


def run(ctx, geom, jobs, make_only=False):
    """the jobs (checker dicts of one geometry) as ONE call on fresh maps: [(map, decisions, n_activated)]"""
    from direct_stereo_slam_amd import distmap

    maps = [distmap.DistanceMap(ctx, *geom) for _ in jobs]
    full = [dict(j, map=m) for j, m in zip(jobs, maps)]
    if make_only:
        distmap.make_distance_maps(ctx, full)
        out = [(m.get(), None, None) for m in maps]
    else:
        res = distmap.activate_points_batch(ctx, full)
        out = [(m.get(), r["decisions"], r["n_activated"]) for m, r in zip(maps, res)]
    for m in maps:
        m.close()
    return out


def check(got, exp_map, exp_dec):
    m, dec, n_act = got
    assert m.dtype == np.float32 and np.array_equal(m, exp_map)
    assert np.array_equal(dec, exp_dec) and n_act == int((exp_dec == 1).sum())


_big = {}


def big_case(name, w, h, **kw):
    if name not in _big:
        job = R.make_case(w=w, h=h, **kw)
        _big[name] = (job,) + R.activate(w, h, job)
    return _big[name]


def test_make_alone(ctx):
    for names in (["small", "no_seeds", "small_b"], ["medium"]):
        cs = [R.case(n) for n in names]
        got = run(ctx, cs[0][:2], [c[2] for c in cs], make_only=True)
        for c, g in zip(cs, got):
            assert np.array_equal(g[0], c[5]["initial_map"])


def test_fifty_adds_read_back_after_each(ctx):
    from direct_stereo_slam_amd import distmap

    w, h, job, _, _, info = R.case("small")
    w1, h1 = w >> 1, h >> 1
    dm = distmap.DistanceMap(ctx, w, h)
    assert (dm.get() == 1000).all()  # D1 / a fresh map
    distmap.make_distance_maps(ctx, [dict(job, map=dm)])
    ref = [int(v) for v in info["initial_map"].reshape(-1)]
    rng = np.random.default_rng(5)
    for i in range(50):
        u, v = int(rng.integers(0, w1)), int(rng.integers(0, h1))
        if i % 7 == 0:
            u = [0, w1 - 1][i % 2]  # border columns, and a corner
            v = 0 if i == 0 else v
        dm.add(u, v)
        R.add(ref, w1, h1, u + w1 * v)
        assert np.array_equal(dm.get(), R.as_float(ref, w1, h1)), i
    from direct_stereo_slam_amd._lib import DsmError

    for u, v in ((-1, 0), (w1, 0), (0, h1), (0, -1)):
        with pytest.raises(DsmError):
            dm.add(u, v)
    assert np.array_equal(dm.get(), R.as_float(ref, w1, h1))
    dm.close()


def test_batch_of_three_equals_each_alone_equals_checker(ctx):
    names = ["small", "no_seeds", "small_b"]
    cs = [R.case(n) for n in names]
    together = run(ctx, (64, 48), [c[2] for c in cs])
    for c, g in zip(cs, together):
        check(g, c[3], c[4])
        alone = run(ctx, (64, 48), [c[2]])[0]
        assert np.array_equal(alone[0], g[0]) and np.array_equal(alone[1], g[1]) and alone[2] == g[2]
    # the same job three times in one call: three equal results (a job does not depend on its neighbours)
    for g in run(ctx, (64, 48), [cs[0][2]] * 3):
        check(g, cs[0][3], cs[0][4])


def test_medium_alone_and_in_a_batch(ctx):
    w, h, job, exp_map, exp_dec, _ = R.case("medium")
    check(run(ctx, (w, h), [job])[0], exp_map, exp_dec)
    other = R.make_case(seed=9, w=w, h=h, n_hosts=2, n_seeds=50, n_cand=100, min_act_dist=0.5)
    got = run(ctx, (w, h), [other, job, other])
    check(got[1], exp_map, exp_dec)
    check(got[0], *R.activate(w, h, other)[:2])
    assert np.array_equal(got[0][0], got[2][0]) and np.array_equal(got[0][1], got[2][1])


def test_kitti_shape_map_held_in_lds(ctx):
    """1232 x 368: the 616 x 184 map is the shape the selection kernel keeps in LDS"""
    job, exp_map, exp_dec, _ = big_case("kitti", 1232, 368, seed=31, n_hosts=7, n_seeds=14000, n_cand=8000, min_act_dist=2.0)
    assert (exp_dec == 1).sum() > 500 and (exp_dec == 0).sum() > 500
    check(run(ctx, (1232, 368), [job])[0], exp_map, exp_dec)


def test_map_too_large_for_lds(ctx):
    """1024 x 768: the 512 x 384 map stays in global memory"""
    job, exp_map, exp_dec, _ = big_case("xga", 1024, 768, seed=32, n_hosts=4, n_seeds=3000, n_cand=1500, min_act_dist=2.0)
    assert (exp_dec == 1).sum() > 100 and (exp_dec == 0).sum() > 100
    check(run(ctx, (1024, 768), [job])[0], exp_map, exp_dec)


# ---- maps whose byte count is no multiple of 16 (odd w1): the padding of the 16-byte fill and of the copy through LDS ------------------
ODD_GEOMS = [(70, 50), (106, 54), (98, 46)]  # maps of 35 x 25 = 875, 53 x 27 = 1431, 49 x 23 = 1127 bytes


def points_on_the_last_column_and_row(job, w, h, rng, each=3):
    """(host, u, v, idepth) of points that the job's hosts project into the last column and into the last row of the map"""
    w1, h1 = w >> 1, h >> 1
    n, nh = 4000, len(job["krki"])
    hst, u, v = rng.integers(0, nh, n).astype(np.int32), rng.uniform(-4, w + 4, n).astype(np.float32), rng.uniform(-4, h + 4, n).astype(np.float32)
    d = rng.uniform(0.1, 2.0, n).astype(np.float32)
    c = R.project(job["krki"], job["kt"], hst, u, v, d, w1, h1)[0]
    col, row = np.flatnonzero((c >= 0) & (c % w1 == w1 - 1))[:each], np.flatnonzero((c >= 0) & (c // w1 == h1 - 1))[:each]
    pick = np.concatenate([col, row])
    return hst[pick], u[pick], v[pick], d[pick]


def odd_case(geom, k):
    """job k of three at an odd geometry, with seeds (k = 0, 2) and candidates put into the last column and row
    -> (job, expected map, expected decisions, info, seed cells, candidate cells, candidates activated in the last column or row)"""
    w, h = geom
    name = f"odd-{w}x{h}-{k}"
    if name not in _big:
        job = R.make_case(seed=600 + 10 * ODD_GEOMS.index(geom) + k, w=w, h=h, n_hosts=3, n_seeds=(40, 0, 15)[k], n_cand=300,
                          min_act_dist=(1.5, 2.0, 1.0)[k])
        rng = np.random.default_rng(700 + k)
        for kind in (("seed",) if k != 1 else ()) + ("cand",):
            extra = points_on_the_last_column_and_row(job, w, h, rng)
            for key, a in zip(("host", "u", "v", "idepth"), extra):
                job[f"{kind}_{key}"] = np.concatenate([job[f"{kind}_{key}"], a])
            if kind == "cand":  # type 1: the lowest threshold, so that some of them activate and are added at the edge
                job["cand_type"] = np.concatenate([job["cand_type"], np.ones(len(extra[0]), np.float32)])
        w1, h1 = w >> 1, h >> 1
        sc = R.project(job["krki"], job["kt"], job["seed_host"], job["seed_u"], job["seed_v"], job["seed_idepth"], w1, h1)[0]
        cc = R.project(job["krki"], job["kt"], job["cand_host"], job["cand_u"], job["cand_v"], job["cand_idepth"], w1, h1)[0]
        m, dec, info = R.activate(w, h, job)
        edge = (cc >= 0) & ((cc % w1 == w1 - 1) | (cc // w1 == h1 - 1))
        _big[name] = (job, m, dec, info, sc[sc >= 0], cc[cc >= 0], int((dec[edge] == 1).sum()))
    return _big[name]


@pytest.mark.parametrize("geom", ODD_GEOMS)
def test_odd_maps_made_alone(ctx, geom):
    w1, h1 = geom[0] >> 1, geom[1] >> 1
    assert (w1 * h1) % 16 and w1 % 2 == 1 and w1 * h1 in (875, 1431, 1127)
    cs = [odd_case(geom, k) for k in range(3)]
    for c in (cs[0], cs[2]):  # seeds in the last column and in the last row: 3 .. 5 each
        assert ((c[4] % w1) == w1 - 1).sum() >= 3 and ((c[4] // w1) == h1 - 1).sum() >= 3
    got = run(ctx, geom, [c[0] for c in cs], make_only=True)
    for c, g in zip(cs, got):
        assert g[0].shape == (h1, w1) and np.array_equal(g[0], c[3]["initial_map"])


@pytest.mark.parametrize("geom", ODD_GEOMS)
def test_odd_maps_fifty_adds_read_back_after_each(ctx, geom):
    from direct_stereo_slam_amd import distmap

    w, h = geom
    w1, h1 = w >> 1, h >> 1
    job, _, _, info = odd_case(geom, 0)[:4]
    dm = distmap.DistanceMap(ctx, w, h)
    assert dm.get().shape == (h1, w1) and (dm.get() == 1000).all()
    distmap.make_distance_maps(ctx, [dict(job, map=dm)])
    ref = [int(v) for v in info["initial_map"].reshape(-1)]
    rng = np.random.default_rng(6)
    for i in range(50):
        u, v = int(rng.integers(0, w1)), int(rng.integers(0, h1))
        if i % 5 == 0:
            u = w1 - 1 if i % 2 else u  # the last column, the last row and (i = 45 .. : both) the last cell of the map
            v = h1 - 1 if i % 2 == 0 or i >= 45 else v
        dm.add(u, v)
        R.add(ref, w1, h1, u + w1 * v)
        assert np.array_equal(dm.get(), R.as_float(ref, w1, h1)), i
    dm.close()


@pytest.mark.parametrize("geom", ODD_GEOMS)
def test_odd_maps_batch_of_three_equals_each_alone_equals_checker(ctx, geom):
    w1, h1 = geom[0] >> 1, geom[1] >> 1
    cs = [odd_case(geom, k) for k in range(3)]
    for c in cs:  # candidates in the last column and in the last row, and both decisions
        cc = c[5]
        assert ((cc % w1) == w1 - 1).sum() >= 3 and ((cc // w1) == h1 - 1).sum() >= 3 and c[6] >= 3  # 6 .. 13 of them activate: adds at the edge
        assert (c[2] == 1).sum() >= 10 and (c[2] == 0).sum() >= 10 and (c[2] == 2).sum() >= 10
    together = run(ctx, geom, [c[0] for c in cs])
    for c, g in zip(cs, together):
        check(g, c[1], c[2])
        alone = run(ctx, geom, [c[0]])[0]
        assert np.array_equal(alone[0], g[0]) and np.array_equal(alone[1], g[1]) and alone[2] == g[2]


# ---- the switch between the map in LDS and the map in global memory: bytes16 <= 138 240 ------------------------------------------------
def test_largest_map_held_in_lds(ctx):
    """960 x 576: the 480 x 288 map is 138 240 bytes, exactly what the selection kernel holds in LDS, no byte to spare.
    The checker takes 0.21 s on the CPU (that of test_kitti_shape_map_held_in_lds: 0.11 s)."""
    assert (960 >> 1) * (576 >> 1) == 138240 == 135 * 1024
    job, exp_map, exp_dec, _ = big_case("lds_limit", 960, 576, seed=33, n_hosts=4, n_seeds=3000, n_cand=1000, min_act_dist=2.0)
    assert (exp_dec == 1).sum() >= 100 and (exp_dec == 0).sum() >= 100, ((exp_dec == 1).sum(), (exp_dec == 0).sum())  # 344 and 523
    check(run(ctx, (960, 576), [job])[0], exp_map, exp_dec)


def test_smallest_map_left_in_global_memory(ctx):
    """1106 x 500: the 553 x 250 map is 138 250 bytes, 138 256 with its padding: the first size past the LDS limit.
    The checker takes 0.22 s on the CPU."""
    w1, h1 = 1106 >> 1, 500 >> 1
    assert w1 * h1 == 138250 and (w1 * h1 + 15) // 16 * 16 == 138256 > 135 * 1024
    job, exp_map, exp_dec, _ = big_case("global_limit", 1106, 500, seed=34, n_hosts=4, n_seeds=3000, n_cand=1000, min_act_dist=2.0)
    assert (exp_dec == 1).sum() >= 100 and (exp_dec == 0).sum() >= 100, ((exp_dec == 1).sum(), (exp_dec == 0).sum())  # 385 and 535
    check(run(ctx, (1106, 500), [job])[0], exp_map, exp_dec)


def edge_job(n_seeds, n_cand, min_act, seed=40, **over):
    job = R.make_case(seed=seed, w=96, h=64, n_hosts=2, n_seeds=n_seeds, n_cand=n_cand, min_act_dist=min_act)
    job.update(over)
    return job


def test_edge_cases(ctx):
    geom = (96, 64)
    jobs = {
        "nothing": edge_job(0, 0, 1.0),
        "no_candidates": edge_job(30, 0, 1.0),
        "min_act_0": edge_job(30, 150, 0.0),
        "threshold_16": edge_job(30, 150, 4.0, cand_type=np.full(150, 4.0, np.float32)),
    }
    oob = edge_job(30, 100, 1.0)
    oob["cand_u"] = oob["cand_u"] + np.float32(500.0)
    jobs["all_out_of_bounds"] = oob
    exp = {k: R.activate(*geom, j) for k, j in jobs.items()}
    assert (exp["nothing"][0] == 1000).all() and len(exp["nothing"][1]) == 0
    assert (exp["all_out_of_bounds"][1] == 2).all()
    d0 = exp["min_act_0"][1]
    assert (d0 != 0).all() and (d0 == 1).sum() > 50  # everything in bounds activates
    d16 = exp["threshold_16"][1]
    assert (d16 == 0).sum() > 50  # 16 exceeds most distances
    got = run(ctx, geom, list(jobs.values()))  # ... and all of them as one batch
    for k, g in zip(jobs, got):
        check(g, *exp[k][:2])
        check(run(ctx, geom, [jobs[k]])[0], *exp[k][:2])


@pytest.mark.parametrize("n", [64, 65, 129])
def test_only_the_last_candidate_passes(ctx, n):
    """just past the wave-sized look-ahead blocks: every candidate but the last is in bounds and fails, the last one passes"""
    geom = (96, 64)
    job = edge_job(30, n, 1.5, seed=50 + n)
    rng = np.random.default_rng(n)
    job["cand_u"], job["cand_v"] = rng.uniform(16, 80, n).astype(np.float32), rng.uniform(16, 48, n).astype(np.float32)
    job["cand_type"] = np.full(n, 1000.0, np.float32)  # threshold 1500 > 1000 + 1
    job["cand_type"][-1] = 0.0
    exp_map, exp_dec, _ = R.activate(*geom, job)
    assert exp_dec.tolist() == [0] * (n - 1) + [1]
    check(run(ctx, geom, [job])[0], exp_map, exp_dec)


def test_invalid_calls_leave_the_maps_untouched(ctx):
    from direct_stereo_slam_amd import distmap
    from direct_stereo_slam_amd._lib import DsmError

    w, h, job, _, _, info = R.case("small")
    a, b, c = distmap.DistanceMap(ctx, w, h), distmap.DistanceMap(ctx, w, h), distmap.DistanceMap(ctx, 96, 64)
    distmap.make_distance_maps(ctx, [dict(job, map=a), dict(R.case("small_b")[2], map=b)])
    before = [a.get(), b.get(), c.get()]
    assert np.array_equal(before[0], info["initial_map"]) and (before[2] == 1000).all()
    bad = dict(job, cand_host=job["cand_host"].copy())
    bad["cand_host"][-1] = 3  # n_hosts = 3
    bad_seed = dict(job, seed_host=job["seed_host"].copy())
    bad_seed["seed_host"][0] = -1
    for jobs in ([dict(job, map=a), dict(job, map=c)],      # mixed geometries
                 [dict(job, map=a), dict(bad, map=b)],      # a candidate's host index past the end
                 [dict(bad_seed, map=a)],                    # a seed's host index below 0
                 [dict(job, map=a), dict(job, map=a)]):      # one map in two jobs
        with pytest.raises(DsmError):
            distmap.activate_points_batch(ctx, jobs)
        for m, bef in zip((a, b, c), before):
            assert np.array_equal(m.get(), bef)
    with pytest.raises(DsmError):
        distmap.make_distance_maps(ctx, [dict(bad_seed, map=a)])
    assert np.array_equal(a.get(), before[0])
    for m in (a, b, c):
        m.close()
