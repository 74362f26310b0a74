"""CPU: the checker of the distance map (tests/_distmap_ref.py) against itself -- its list BFS and its independently written
whole-map dilation form agree, on inputs that two plausible but wrong forms fail -- and the host form dsm_activate_points_host
against the checker, map and decisions, as exact equality."""
import numpy as np
import pytest

import _distmap_ref as R


def random_map_cases(n=300):
    """maps 8..40 x 8..30, 0-5 seeds (columns 1 .. w1-1: u = w1-1 included, row / column 0 never: D2), 1-5 adds anywhere (borders and
    corners included)"""
    rng = np.random.default_rng(2024)
    for _ in range(n):
        w1, h1 = int(rng.integers(8, 41)), int(rng.integers(8, 31))
        seeds = [int(rng.integers(1, w1)) + w1 * int(rng.integers(1, h1)) for _ in range(int(rng.integers(0, 6)))]
        if seeds and rng.uniform() < 0.3:
            seeds[0] = (w1 - 1) + w1 * int(rng.integers(1, h1))
        adds = []
        for _ in range(int(rng.integers(1, 6))):
            x, y = int(rng.integers(0, w1)), int(rng.integers(0, h1))
            if rng.uniform() < 0.2:
                x = int(rng.choice([0, w1 - 1]))
            if rng.uniform() < 0.2:
                y = int(rng.choice([0, h1 - 1]))
            adds.append(x + w1 * y)
        yield w1, h1, seeds, adds


def test_list_bfs_equals_dilation_form_and_the_wrong_forms_do_not():
    n = differ_min = differ_once = 0
    for w1, h1, seeds, adds in random_map_cases():
        m = R.make_map(w1, h1, seeds)
        a = R.make_map_dilate(w1, h1, seeds)
        assert np.array_equal(np.asarray(m).reshape(h1, w1), a)
        for c in adds:
            R.add(m, w1, h1, c)
            R.add_dilate(a, c)
            assert np.array_equal(np.asarray(m).reshape(h1, w1), a), (w1, h1, seeds, adds)
        seq = np.asarray(m).reshape(h1, w1)
        differ_min += not np.array_equal(R.min_of_single_maps(w1, h1, seeds + adds), seq)
        differ_once += not np.array_equal(R.all_at_once(w1, h1, seeds + adds), seq)
        n += 1
    print(f"{n} cases: min-of-single-seed maps differs in {differ_min}, all-at-once in {differ_once}")
    assert n == 300
    assert differ_min >= n // 4  # the inputs discriminate: a quarter at least
    assert differ_once >= 1


def test_levels_alternate_8_and_4_neighbourhoods_and_borders_do_not_expand():
    """D3 / D4 on maps small enough to read: k = 1 is 8-connected, k = 2 4-connected; a border seed spreads nothing"""
    m = R.as_float(R.make_map(9, 9, [4 + 9 * 4]), 9, 9)
    assert m[3, 3] == 1 and m[3, 4] == 1 and m[2, 2] == 3 and m[2, 4] == 2 and m[2, 3] == 2  # diagonal step only at odd k
    assert m[0, 4] == 4 and m[0, 0] == 5  # (3,3) (2,3) (1,2) (1,1) (0,0): diagonal steps at k = 1, 3, 5
    b = R.as_float(R.make_map(9, 9, [8 + 9 * 4]), 9, 9)  # u = w1 - 1: a seed, but never expanded
    assert b[4, 8] == 0 and (b == 1000).sum() == 80
    e = [R.FAR] * 81
    R.add(e, 9, 9, 0)  # a corner add: the cell alone
    assert e[0] == 0 and sum(v == R.FAR for v in e) == 80


@pytest.mark.parametrize("name", list(R.CASES))
def test_host_form_equals_checker(built, name):
    from direct_stereo_slam_amd import distmap

    w, h, job, exp_map, exp_dec, info = R.case(name)
    m, dec, n_act = distmap.activate_points_host(w, h, job)
    assert np.array_equal(dec, exp_dec)
    assert m.dtype == np.float32 and np.array_equal(m, exp_map)
    assert n_act == int((exp_dec == 1).sum())
    assert set(np.unique(m)) <= set(range(40)) | {1000}


def test_first_case_covers_every_outcome():
    """activated, rejected, out of bounds, and rejected only because of an earlier activation: at least 40 each"""
    w, h, job, exp_map, dec, info = R.case("small")
    w1, h1 = w >> 1, h >> 1
    cc, p0 = R.project(job["krki"], job["kt"], job["cand_host"], job["cand_u"], job["cand_v"], job["cand_idepth"], w1, h1)
    frac = p0 - np.floor(p0)
    thr = np.float32(job["min_act_dist"]) * job["cand_type"]
    m0 = info["initial_map"].reshape(-1)
    late = sum(1 for i, c in enumerate(cc) if c >= 0 and dec[i] == 0 and m0[c] + frac[i] >= thr[i])
    counts = dict(activated=int((dec == 1).sum()), rejected=int((dec == 0).sum()), out_of_bounds=int((dec == 2).sum()), rejected_by_earlier_activation=late)
    print(counts)
    assert all(v >= 40 for v in counts.values()), counts
    assert len(set(job["cand_type"].tolist())) == 3


def test_non_finite_coordinates(built):
    """NaN and +-inf coordinates or depths: skipped as seeds, decision 2 as candidates -- checker and host form"""
    from direct_stereo_slam_amd import distmap

    w, h = 64, 48
    job = R.make_case(seed=7, w=w, h=h, n_hosts=2, n_seeds=12, n_cand=40, min_act_dist=1.0)
    bad = [np.nan, np.inf, -np.inf]
    clean = {k: job[k].copy() for k in ("seed_u", "seed_v", "seed_idepth")}
    for j, b in enumerate(bad):
        job["seed_u"][j], job["seed_v"][3 + j], job["seed_idepth"][6 + j] = b, b, b
        job["cand_u"][j], job["cand_v"][3 + j], job["cand_idepth"][6 + j] = b, b, b
    exp_map, exp_dec, _ = R.activate(w, h, job)
    assert (exp_dec[:9] == 2).all()
    # the same window with those nine seeds removed gives the same map: they were skipped
    keep = np.r_[9:12]
    sub = dict(job, seed_host=job["seed_host"][keep], seed_u=clean["seed_u"][keep], seed_v=clean["seed_v"][keep], seed_idepth=clean["seed_idepth"][keep])
    sub_map, sub_dec, _ = R.activate(w, h, sub)
    assert np.array_equal(sub_map, exp_map) and np.array_equal(sub_dec, exp_dec)
    m, dec, _ = distmap.activate_points_host(w, h, job)
    assert np.array_equal(m, exp_map) and np.array_equal(dec, exp_dec)


def test_host_form_rejects_a_bad_host_index(built):
    from direct_stereo_slam_amd import distmap
    from direct_stereo_slam_amd._lib import DsmError

    job = R.make_case(seed=8, w=64, h=48, n_hosts=2, n_seeds=5, n_cand=5, min_act_dist=1.0)
    job["cand_host"][3] = 2
    with pytest.raises(DsmError):
        distmap.activate_points_host(64, 48, job)
