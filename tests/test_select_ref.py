"""CPU: dsm_select_pixels_host against the checker tests/_select_ref.py -- the map, the counts, the passes, the new potential and every
point array exactly, floats bit for bit -- and the conditions the scene must meet so that the
comparison, here and in tests/test_select_device.py, covers every rule.  The conditions are asserted on the checker's output alone."""
import numpy as np
import pytest

import _select_ref as R


@pytest.mark.parametrize("name", list(R.CASES))
def test_host_form_equals_checker(built, name):
    from direct_stereo_slam_amd import pixelselect

    case = R.CASES[name]
    w, h = case["shape"]
    got = pixelselect.select_pixels_host(w, h, R.pyramid(R.image_of(case)), R.pattern(w, h), R.job_of(case), **case["params"])
    R.assert_equal(got, R.expected(name))


def test_outputs_are_optional_and_the_map_is_not_needed(built):
    from direct_stereo_slam_amd import pixelselect

    name = "104x72-adapt3-300"
    case = R.CASES[name]
    w, h = case["shape"]
    b = pixelselect.SelectBatch([R.job_of(case, want_map=False)], w, h)
    b.arr[0].counts_out = b.arr[0].passes_out = None
    b.run_host(0, R.pyramid(R.image_of(case)), R.pattern(w, h))
    got, exp = b.results()[0], R.expected(name)
    assert (got["n_pts"], got["num_total"], got["potential"]) == (exp["n_pts"], exp["num_total"], exp["potential"])
    assert np.array_equal(got["u"], exp["u"]) and np.array_equal(got["v"], exp["v"])
    assert got["counts"].tolist() == [-1, -1, -1] and got["passes"] == -1


# ---- what the scene must reach (the figures in the messages are what it reaches) ------------------------------------------------------
@pytest.mark.parametrize("shape", R.SHAPES)
def test_scene_is_integer_valued_so_every_level_is_exact(shape):
    I = R.pyramid(R.scene(*shape))
    assert I[0].min() >= 0 and I[0].max() <= 255 and np.array_equal(I[0], np.rint(I[0]))
    assert np.array_equal(I[1] * 4, np.rint(I[1] * 4)) and np.array_equal(I[2] * 16, np.rint(I[2] * 16))
    assert [a.shape for a in I] == [(shape[1] >> l, shape[0] >> l) for l in range(3)]


@pytest.mark.parametrize("shape", R.SHAPES)
@pytest.mark.parametrize("pot", R.POTENTIALS)
def test_masks_that_depend_on_the_direction(shape, pot):
    exp = R.expected(f"{shape[0]}x{shape[1]}-pot{pot}")
    masks = R.cell_masks(exp["info"]["frame"], pot)
    mixed = sum(1 for m in masks if m not in (0, 0xFFFF))
    assert mixed >= 20, mixed  # 31 .. 1456
    # the masks and the running count give the hits: the order-free form of P7 on the checker's own data
    n2 = 0
    for m in masks:
        n2 += (m >> (int(R.pattern(*shape)[n2]) & 15)) & 1
    assert n2 == exp["counts"][0]
    if pot <= 2:
        n2, n3, n4 = exp["counts"]
        assert n2 >= 100 and n3 >= 50, (n2, n3)  # 368 .. 758, 81 .. 288
        fast, slow = R.chain_groups(masks)
        assert fast >= 1 and slow >= 1, (fast, slow)  # 8 .. 54, 14 .. 63
    if pot == 1:
        assert exp["counts"][2] >= 20, exp["counts"]  # 35 and 40


@pytest.mark.parametrize("shape", R.SHAPES)
def test_adaptation_takes_each_way_and_thinning_runs_and_is_skipped(shape):
    e = {k: R.expected(f"{shape[0]}x{shape[1]}-adapt{k[0]}-{k[1]}") for k in [(3, 300), (3, 3000), (3, 30), (1, 150), (3, 60)]}
    ways = {k: (v["info"]["way"], [t["potential"] for t in v["info"]["trace"]], v["potential"]) for k, v in e.items()}
    assert ways[(3, 300)][0] == "neither" and ways[(3, 3000)][:2] == ("down", [3, 1]), ways
    assert ways[(3, 30)][0] == "up" and ways[(1, 150)][0] == "up" and ways[(3, 60)][0] == "up", ways
    assert ways[(3, 30)][1][1] >= 9 and ways[(1, 150)][1][1] >= 3, ways  # a jump to the ideal potential, not pot + 1
    thinned = [k for k, v in e.items() if v["info"]["thinned"]]
    assert len(thinned) >= 2 and len(thinned) < len(e), thinned
    for k in thinned:
        assert e[k]["num_total"] < e[k]["counts"].sum()
    assert R.expected("three_passes")["passes"] == 3
    down = R.expected("constant_image")
    assert (down["n_pts"], down["num_total"], down["potential"], down["passes"]) == (0, 0, 1, 2) and not down["map"].any()


def test_lost_row_clamp_and_cap():
    w, h = R.SHAPES[1]
    assert h % 4 == 0 and w % 32 == 8 and h % 32 == 8 and (w // 32, h // 32) == (3, 2)
    exp = R.expected(f"{w}x{h}-pot1")
    assert exp["info"]["lost_rows"] >= 1 and exp["map"][h - 4].any()  # P13: hits in row h - 4 make no point
    assert exp["n_pts"] < exp["num_total"]
    ys, xs = np.nonzero(exp["map"])
    assert ((xs >> 5) >= w // 32).any() and ((ys >> 5) >= h // 32).any()  # P3: hits whose threshold was read through the clamp
    F = exp["info"]["frame"]
    assert F.clamped[0] >= 1 and F.clamped[1] >= 1
    # P1: level 2 is read in its border row h_2 - 1 at yf = h - 4
    assert int((h - 4) * 0.25 + 0.125) == (h >> 2) - 1
    capped = R.expected("max_pts_below_yield")
    assert capped["n_pts"] > 37 and len(capped["u"]) == 37
    for name in ("b_inv", "no_direction_distribution"):
        assert not np.array_equal(R.expected(name)["map"], R.select_ref(R.scene(w, h), R.pattern(w, h), 2, 400.0, R.MAX_PTS)["map"]), name
    for name in R.CASES:
        assert R.expected(name)["n_pts"] <= R.MAX_PTS or name == "max_pts_below_yield"
