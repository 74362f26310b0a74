"""CPU: the numpy checker of the template builder (tests/_template_ref.py) against the C oracle and the host form
dsm_make_coarse_depth_l0, bit for bit on every case that tests/test_template_edges.py runs on the device; the coordinate contract on the
host form; and, from the checker alone, what each case is there for -- so that the device tests cannot pass vacuously."""
import numpy as np
import pytest

import _template_ref as R

F = np.float32
K = (100.0, 100.0, 32.0, 32.0)  # the builder does not read the camera


def _host(c, pu=None, pv=None):
    from direct_stereo_slam_amd.tracker import make_coarse_depth_l0

    return make_coarse_depth_l0(c.w, c.h, c.nl, c.pu if pu is None else pu, c.pv if pv is None else pv, c.pid, c.pw, R.dip(c.planes))


def _oracle(c):
    from direct_stereo_slam_amd import synth as S
    from oracle import oracle as O

    orc = O.OracleTracker(c.w, c.h, c.nl, S.KITTI_T_STEREO, K)
    return orc.make_coarse_depth_l0(c.pu, c.pv, c.pid, c.pw, R.dip(c.planes))


def _assert_lists_equal(got, ref, what):
    for l in range(len(ref.counts)):
        for k, name in enumerate(("u", "v", "idepth", "color")):
            assert len(got[k][l]) == ref.counts[l], (what, l, name, len(got[k][l]), ref.counts[l])
            np.testing.assert_array_equal(got[k][l], ref.lists[k][l], err_msg=f"{what}: level {l}, {name}")


def _entry(ref, l, x, y):
    """the emitted idepth of pixel (x, y) at level l, or None"""
    at = np.nonzero((ref.lists[0][l] == x) & (ref.lists[1][l] == y))[0]
    assert len(at) <= 1
    return ref.lists[2][l][at[0]] if len(at) else None


@pytest.mark.parametrize("name", R.CASES)
def test_numpy_reference_equals_oracle_and_host_form(built, name):
    c = R.case(name)
    assert R.accepted(c.pu, c.pv, c.w, c.h).all()
    _assert_lists_equal(_oracle(c), c.ref, "oracle")
    _assert_lists_equal(_host(c), c.ref, "host form")


def test_every_geometry_and_point_set_is_covered():
    geoms = {n.partition("-")[2] for n in R.CASES}
    assert geoms == set(R.GEOMETRIES)
    for kind in ("border", "dense", "checker", "lattice", "rows", "columns"):
        assert all(f"{kind}-{g}" in R.CASES for g in R.SMALL)
    # the structures the geometries are there for
    w, h, nl = R.GEOMETRIES["mini4"]
    assert ((w >> (nl - 1)) - 4) * ((h >> (nl - 1)) - 4) == 16 < R.WAVE
    w, h, nl = R.GEOMETRIES["g68"]
    assert [((w >> l) - 4) * ((h >> l) - 4) for l in range(nl)] == [4 * R.EMIT_BLOCK, 900, 169] and w - 4 == R.WAVE
    assert 169 < R.EMIT_THREADS < 900 < R.EMIT_BLOCK
    w, h, nl = R.GEOMETRIES["odd"]
    assert [(h >> l) for l in range(nl)] == [135, 67, 33]
    w, h, nl = R.GEOMETRIES["big"]
    assert (w - 4) * (h - 4) == 1056720 and R.emit_blocks(w, h) == 1032 > 1024


# ---- the coordinate contract -----------------------------------------------------------------------------------------------------------

def refused_coordinates(size):
    return [np.nan, np.inf, -np.inf, 1e20, -1.6, size - 0.5]


def accepted_coordinates(size):
    return [-0.4, -1.4, np.nextafter(F(size - 0.5), F(0))]


def test_coordinate_predicate():
    w, h, _ = R.GEOMETRIES["tiny"]
    for x in refused_coordinates(w):
        assert not R.accepted([x], [5.0], w, h)[0], x
    for y in refused_coordinates(h):
        assert not R.accepted([5.0], [y], w, h)[0], y
    for x, px in zip(accepted_coordinates(w), (0, 0, w - 1)):
        assert R.accepted([x], [5.0], w, h)[0] and R.pixels([x], [5.0])[0][0] == px, x
    for y, py in zip(accepted_coordinates(h), (0, 0, h - 1)):
        assert R.accepted([5.0], [y], w, h)[0] and R.pixels([5.0], [y])[1][0] == py, y
    with pytest.raises(ValueError):
        R.make_coarse_depth(w, h, 2, [np.nan], [5.0], [1.0], [1.0], R.case("single-tiny").planes)


@pytest.mark.parametrize("axis", ["u", "v"])
def test_host_form_coordinate_contract(built, axis):
    from direct_stereo_slam_amd._lib import DsmError

    c = R.case("border-tiny")
    size = c.w if axis == "u" else c.h
    k = len(c.pu) // 2
    for bad in refused_coordinates(size):
        pu, pv = c.pu.copy(), c.pv.copy()
        (pu if axis == "u" else pv)[k] = bad
        assert not R.accepted(pu, pv, c.w, c.h)[k]
        with pytest.raises(DsmError, match="dsm error -1"):  # DSM_ERR_INVALID
            _host(c, pu, pv)
    for good in accepted_coordinates(size):
        pu, pv = c.pu.copy(), c.pv.copy()
        (pu if axis == "u" else pv)[k] = good
        ref = R.make_coarse_depth(c.w, c.h, c.nl, pu, pv, c.pid, c.pw, c.planes)
        _assert_lists_equal(_host(c, pu, pv), ref, f"host form, {axis} = {good!r}")


# ---- what each case is there for ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("geom", R.SMALL + ("big",))
def test_border_points_reach_every_border_line(geom):
    c = R.case("twopass-big" if geom == "big" else f"border-{geom}")
    u, v = R.pixels(c.pu, c.pv)
    for col in (0, 1, c.w - 2, c.w - 1):
        assert (u == col).any(), col
    for row in (0, 1, c.h - 2, c.h - 1):
        assert (v == row).any(), row
    for a in (c.pu, c.pv):
        assert ((a > -1.5) & (a < -0.5)).any()
    assert c.ref.counts[0] > 0


@pytest.mark.parametrize("geom", R.SMALL)
def test_dense_fills_the_capacity(geom):
    c = R.case(f"dense-{geom}")
    u, v = R.pixels(c.pu, c.pv)
    assert len(np.unique(v * c.w + u)) == c.w * c.h == len(c.pu)
    for l in range(c.nl):
        wl, hl = c.w >> l, c.h >> l
        assert len(set(c.bad[l])) == 3 and c.bad[l][0] == (2, 2) and c.bad[l][2] == (wl - 3, hl - 3)
        assert all(not np.isfinite(c.planes[l][y, x]) for x, y in c.bad[l])
        assert c.ref.counts[l] == (wl - 4) * (hl - 4) - 3
        assert all(_entry(c.ref, l, x, y) is None for x, y in c.bad[l])


@pytest.mark.parametrize("geom", ["mini4", "g68", "tiny"])
def test_empty_single_and_dilation_only(geom):
    w, h, nl = R.GEOMETRIES[geom]
    assert R.case(f"empty-{geom}").ref.counts == [0] * nl
    c = R.case(f"single-{geom}")
    assert len(c.pu) == 1 and c.ref.counts[0] == 5  # its own pixel and the four diagonal fills
    u, v = R.pixels(c.pu, c.pv)
    assert _entry(c.ref, 0, u[0], v[0]) is not None
    # the only entry comes from the dilation: the point's own pixel (1, 1) is outside the interior, its fill (2, 2) inside
    c = R.case(f"dilated-{geom}")
    u, v = R.pixels(c.pu, c.pv)
    assert len(c.pu) == 1 and (u[0], v[0]) == (1, 1) and c.ref.counts == [1] + [0] * (nl - 1)
    assert _entry(c.ref, 0, 2, 2) == c.pid[0] * c.pw[0] / c.pw[0]
    # idepth < 0: the own pixel is left out and so is every fill, whose idepth / weight is the point's own
    c = R.case(f"negative-{geom}")
    assert len(c.pu) == 1 and c.pid[0] < 0 and c.ref.counts == [0] * nl
    assert (c.ref.dilated[0][1] > 0).sum() == 5


@pytest.mark.parametrize("geom", ["tiny", "g68"])
def test_collision_order_changes_the_bits(geom):
    c = R.case(f"collisions-{geom}")
    u, v = R.pixels(c.pu, c.pv)
    on = np.nonzero((u == c.pixel[0]) & (v == c.pixel[1]))[0]
    assert len(on) == R.N_COLLIDING == 300 and np.array_equal(on, c.colliding)
    assert np.log10(c.pw[on].max() / c.pw[on].min()) > 5.5  # six decades
    assert list(np.nonzero((u == c.pixel2[0]) & (v == c.pixel2[1]))[0]) == [0, len(c.pu) - 1]
    a = _entry(c.ref, 0, *c.pixel)
    assert a is not None and _entry(c.ref, 0, *c.pixel2) is not None
    pid, pw = c.pid.copy(), c.pw.copy()
    pid[on], pw[on] = c.pid[on[::-1]], c.pw[on[::-1]]
    b = _entry(R.make_coarse_depth(c.w, c.h, c.nl, c.pu, c.pv, pid, pw, c.planes), 0, *c.pixel)
    assert b is not None and a.view(np.uint32) != b.view(np.uint32), (a, b)


def test_values_case_holds_each_value():
    c = R.case("values-tiny")
    sid, sw = c.ref.sums[0]
    (zero, neg, wnan, winf, wninf, dnan, dinf, dninf, dzero, dneg, dnegzero) = c.specials
    # zero and negative weights (-inf and an exact cancellation among them): holes, dilated over and emitted
    for x, y in (zero, neg, wninf, (20, 40)):
        assert sw[y, x] <= 0 and c.ref.dilated[0][1][y, x] > 0 and _entry(c.ref, 0, x, y) is not None, (x, y)
    assert sw[neg[1], neg[0]] < 0 and sw[40, 20] == 0
    # a NaN weight is no hole and no entry; a weight of +inf gives idepth / weight = NaN
    assert np.isnan(sw[wnan[1], wnan[0]]) and np.isnan(c.ref.dilated[0][1][wnan[1], wnan[0]])
    assert sw[winf[1], winf[0]] == np.inf and sw[wninf[1], wninf[0]] == -np.inf
    for x, y in (wnan, winf, dnan, dninf, dzero, dneg, dnegzero, (60, 40)):
        assert _entry(c.ref, 0, x, y) is None, (x, y)
    assert np.isnan(sid[dnan[1], dnan[0]]) and sid[dzero[1], dzero[0]] == 0 and sid[dneg[1], dneg[0]] < 0
    assert sid[40, 60] < 0 < sw[40, 60]  # a negative weighted sum under a positive weight
    assert _entry(c.ref, 0, *dinf) == np.inf  # an infinite idepth is > 0: the reference keeps it
    # the non-finite sums reach level 1 too
    assert np.isnan(c.ref.sums[1][1]).any() and np.isinf(c.ref.sums[1][0]).any()


@pytest.mark.parametrize("geom", R.SMALL)
def test_dilation_patterns(geom):
    w, h, nl = R.GEOMETRIES[geom]
    c = R.case(f"checker-{geom}")
    # the diagonal dilation fills no hole of a checkerboard: level 0 emits the occupied interior pixels alone
    x, y = c.ref.lists[0][0].astype(int), c.ref.lists[1][0].astype(int)
    assert ((x + y) % 2 == 0).all() and c.ref.counts[0] == ((w - 4) * (h - 4) + 1) // 2
    c = R.case(f"lattice-{geom}")
    x, y = c.ref.lists[0][0].astype(int), c.ref.lists[1][0].astype(int)
    assert ((x % 2) == (y % 2)).all() and (x % 2 == 1).any() and (x % 2 == 0).any()
    c = R.case(f"rows-{geom}")
    y = c.ref.lists[1][0].astype(int)
    assert set(y) == {2, h - 3} and c.ref.counts[0] == 2 * (w - 4)  # row 1 dilates into row 2, row h-2 into row h-3
    assert (c.ref.dilated[0][1][0] == c.ref.sums[0][1][0]).all()  # row 0 is never a target
    c = R.case(f"columns-{geom}")
    x = c.ref.lists[0][0].astype(int)
    assert set(x) == {2, w - 3} and c.ref.counts[0] == 2 * (h - 4)


def test_block_patterns_occur():
    c = R.case("blocks-g68")
    block, pas, wave, lane, _ = R.emit_coordinates(c.ref.lists[0][0], c.ref.lists[1][0], c.w)
    assert R.emit_blocks(c.w, c.h) == 4
    assert set(block) == {0, 2, 3}  # block 1 emits nothing, between blocks that do
    assert set(pas[block == 2]) == {3}  # a block whose only entries are in its last pass
    assert set(pas[block == 0]) == {0, 1, 2, 3}
    key = (block * 4 + pas) * 4 + wave
    assert set(key[lane == 0]) & set(key[lane == 63])  # one wave with entries at its first and at its last lane
    assert set(block[lane == 0]) >= {0, 3} and set(block[lane == 63]) >= {0, 3}
    assert (lane == 0).any() and (lane == 63).any()


def test_two_scan_passes_are_needed_and_used():
    c = R.case("twopass-big")
    assert len(c.pu) == 20000
    _, _, _, _, item = R.emit_coordinates(c.ref.lists[0][0], c.ref.lists[1][0], c.w)
    assert (np.diff(item) > 0).all()  # row-major
    assert (item >= 1024 * R.EMIT_BLOCK).sum() > 100 and (item < 1024 * R.EMIT_BLOCK).sum() > 100
    assert item.max() // R.EMIT_BLOCK >= 1030  # entries in the last blocks of the second pass
