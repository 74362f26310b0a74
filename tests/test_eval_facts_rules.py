"""The rules behind the evaluation loop's settled checks (csrc/eval_facts.hpp), on the host: no GPU.

dsm_pose_fact_host and dsm_fact_rules_host are compiled from the inline functions the kernels run.  The pose rule claims: whenever it
says true for a pose row (M6, M7, M8, t2) and a box [xmin, xmax] x [ymin, ymax] x [0, idmax], the value the loop computes in float32,
pt2 = ((M6 x + M7 y) + M8) + t2 id, lies in [2^-21, 2^31) for every point of the box -- inside the range [2^-33, 2^32) in which the loop's
fast quotients are the IEEE quotients, and positive.  Checked here against float32 evaluation (numpy rounds every operation to float32,
as the kernel's contraction-free code does) at the box's corners and 10^4 interior samples per case, and against exact rational
arithmetic at the corners (pt2 is affine in (x, y, id): its extremes over a box are at corners).  The contrapositive -- a sample outside
the range means the rule said false -- is the same assertion read backwards; the adversarial cases make sure it is exercised, and the
ordinary cases make sure the rule is not vacuous."""
from fractions import Fraction

import numpy as np

from direct_stereo_slam_amd import _lib

F = np.float32
LO_CLAIM, HI_CLAIM = F(2.0 ** -21), F(2.0 ** 31)  # what eval_facts.hpp derives
LO_NEED, HI_NEED = F(2.0 ** -33), F(2.0 ** 32)    # what the loop's quotients need
N_INTERIOR = 10_000


def pose_fact(rows):
    rows = np.ascontiguousarray(rows, F).reshape(-1, 9)
    out = np.zeros(len(rows), np.int32)
    assert _lib.load().dsm_pose_fact_host(len(rows), rows.ctypes.data_as(_lib.c_float_p), out.ctypes.data_as(_lib.c_int_p)) == 0
    return out.astype(bool)


def rot(axis, deg):
    a = np.asarray(axis, float)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.deg2rad(deg)
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def camera_row(R, t2, fx=500.0, fy=480.0, cx=310.0, cy=230.0):
    """the third row of R K^-1 and t2, as make_eval_rot forms them (float32)"""
    Ki = np.array([[1 / fx, 0, -cx / fx], [0, 1 / fy, -cy / fy], [0, 0, 1]], F)
    M = (R.astype(F) @ Ki).astype(F)
    return [M[2, 0], M[2, 1], M[2, 2], F(t2)]


def cases():
    rng = np.random.default_rng(20240611)
    rows = []
    img_box = [4.0, 635.0, 4.0, 475.0]
    # ordinary: small motions of a camera over an image-sized box
    for _ in range(60):
        R = rot(rng.normal(size=3), rng.uniform(0, 8))
        rows.append(camera_row(R, rng.uniform(-0.1, 0.1)) + img_box + [rng.uniform(0.01, 2.0)])  # (pt2 >= 1 - 0.2 - 0.65 sin 8 deg - ...)
    # rotations up to 90 degrees about every kind of axis (pt2 reaches zero and below inside the box)
    for deg in np.linspace(10, 90, 33):
        for axis in ([1, 0, 0], [0, 1, 0], [1, 1, 0], [1, -1, 0.2], [0, 0, 1]):
            for s in (1, -1):
                rows.append(camera_row(rot(axis, s * deg), rng.normal(scale=0.3)) + img_box + [rng.uniform(0.01, 3.0)])
    # t2 * idmax near -M8: the translation eats the depth
    for eps in (0.0, 1e-7, 1e-6, 1e-5, 1e-3, 1e-2, 0.1, 0.5):
        for idmax in (0.5, 1.0, 7.0, 1e3):
            for sgn in (1, -1):
                rows.append([F(0), F(0), F(1), F(-(1 - sgn * eps) / idmax)] + img_box + [idmax])
    # bounds and coefficients at 2^+-30 and beyond
    for e in (-40, -31, -30, -29, -21, -20, -19, 0, 19, 20, 29, 30, 31, 40):
        s = 2.0 ** e
        rows.append([F(0), F(0), F(s), F(0)] + img_box + [1.0])              # M8 alone
        rows.append([F(s / 600), F(0), F(1), F(0)] + img_box + [1.0])        # slope in x
        rows.append([F(1e-3), F(1e-3), F(1), F(0)] + [-s, s, -s, s] + [1.0])  # box size, negative x and y
        rows.append([F(0), F(0), F(1), F(1)] + img_box + [s])                # idmax
        rows.append([F(0), F(0), F(1), F(-1)] + img_box + [s])
    # negative coordinates (a template in normalised coordinates), denormal inverse depths
    for _ in range(40):
        R = rot(rng.normal(size=3), rng.uniform(0, 60))
        x0, y0 = rng.uniform(-2, 0), rng.uniform(-2, 0)
        rows.append([F(R[2, 0]), F(R[2, 1]), F(R[2, 2]), F(rng.normal(scale=0.3))] + [x0, x0 + rng.uniform(0, 3), y0, y0 + rng.uniform(0, 3)]
                    + [rng.choice([1e-45, 1e-40, 2.0 ** -64, 1.0])])
    # random magnitudes over many octaves
    for _ in range(200):
        m = rng.normal(size=4) * 2.0 ** rng.integers(-34, 34, size=4)
        b = np.sort(rng.normal(size=2) * 2.0 ** rng.integers(-10, 34)), np.sort(rng.normal(size=2) * 2.0 ** rng.integers(-10, 34))
        rows.append([F(m[0]), F(m[1]), F(abs(m[2])), F(m[3])] + list(b[0]) + list(b[1]) + [abs(rng.normal()) * 2.0 ** rng.integers(-70, 34)])
    return np.array(rows, F)


def float_pt2(row, x, y, idv):
    M6, M7, M8, t2 = (F(v) for v in row[:4])
    return ((M6 * x + M7 * y) + M8) + t2 * idv  # float32 arrays: every operation rounds to float32


def samples(row, rng):
    xmin, xmax, ymin, ymax, idmax = (float(v) for v in row[4:])
    cx, cy, ci = np.meshgrid([xmin, xmax], [ymin, ymax], [0.0, idmax], indexing="ij")
    x = np.concatenate([cx.ravel(), rng.uniform(xmin, xmax, N_INTERIOR)]).astype(F)
    y = np.concatenate([cy.ravel(), rng.uniform(ymin, ymax, N_INTERIOR)]).astype(F)
    i = np.concatenate([ci.ravel(), rng.uniform(0.0, idmax, N_INTERIOR)]).astype(F)
    # rounding to float32 must not leave the box
    return np.clip(x, F(xmin), F(xmax)), np.clip(y, F(ymin), F(ymax)), np.clip(i, F(0), F(idmax))


ROWS = cases()
FACT = pose_fact(ROWS)


def test_rule_is_exercised_both_ways():
    assert FACT[:60].all(), "ordinary camera motions must pass the rule"
    assert 50 < FACT.sum() < len(ROWS) - 50


def test_true_means_every_float_pt2_is_ordinary_and_positive():
    rng = np.random.default_rng(7)
    with np.errstate(all="ignore"):
        for row, fact in zip(ROWS, FACT):
            x, y, i = samples(row, rng)
            pt2 = float_pt2(row, x, y, i)
            inside = bool(np.all((pt2 >= LO_NEED) & (pt2 < HI_NEED) & (pt2 > 0)))
            if fact:
                assert np.all((pt2 >= LO_CLAIM) & (pt2 < HI_CLAIM)), (row, float(pt2.min()), float(pt2.max()))
                assert inside
            if not inside:
                assert not fact, row


def test_true_means_exact_extremes_inside():
    for row in ROWS[FACT]:
        M6, M7, M8, t2, xmin, xmax, ymin, ymax, idmax = (Fraction(float(v)) for v in row)
        vals = [M6 * x + M7 * y + M8 + t2 * i for x in (xmin, xmax) for y in (ymin, ymax) for i in (0, idmax)]
        assert min(vals) >= Fraction(2) ** -21 and max(vals) < Fraction(2) ** 31, row


def test_adversarial_rows_say_false():
    box = [4.0, 635.0, 4.0, 475.0]
    nan, inf = float("nan"), float("inf")
    bad = [
        camera_row(rot([0, 1, 0], 90), 0.0) + box + [1.0],   # the optical axis lies in the image plane
        camera_row(rot([1, 0, 0], 180), 0.0) + box + [1.0],  # looking backwards
        [0, 0, 1, -1.0] + box + [1.0],                        # t2 * idmax = -M8
        [0, 0, 1, -0.999999] + box + [1.0],
        [0, 0, 2.0 ** 31, 0] + box + [1.0],                   # too large
        [0, 0, 2.0 ** -21, 0] + box + [1.0],                  # too small
        [1, 0, 1, 0] + [-2.0 ** 31, 2.0 ** 31, 0, 1] + [1.0],
        [0, 0, 1, 0] + box + [inf], [0, 0, 1, 0] + box + [nan], [nan, 0, 1, 0] + box + [1.0], [0, 0, nan, 0] + box + [1.0],
        [0, 0, 1, nan] + box + [1.0], [0, inf, 1, 0] + box + [1.0], [0, 0, 1, 0] + [0, inf, 0, 1] + [1.0],  # (a NaN bound cannot occur: the template fact wants finite x, y)
        [0, 0, 1, 0] + [inf, -inf, inf, -inf] + [-inf],       # the bounds of an empty list
    ]
    assert not pose_fact(np.array(bad, F)).any()
    assert pose_fact(np.array([[0, 0, 1, 0] + box + [1.0], [0, 0, 1, 0] + box + [1e-45]], F)).all()


def test_keys_and_value_rules():
    inf, nan = np.inf, np.nan
    v = np.array([-inf, -3e38, -1.0, -2.0 ** -64, -1e-45, -0.0, 0.0, 1e-45, 2.0 ** -70, 2.0 ** -64, 1.0, 255.0, 2.0 ** 100, 1e38, 3e38, inf, nan], F)
    out = np.zeros(4 * len(v), np.int32)
    assert _lib.load().dsm_fact_rules_host(len(v), v.ctypes.data_as(_lib.c_float_p), out.ctypes.data_as(_lib.c_int_p)) == 0
    key, bits, entry, pixel = out.reshape(-1, 4).T
    assert np.array_equal(bits, v.view(np.int32))                   # the key turns back into the same bits
    assert np.all(np.diff(key[:-1].astype(np.int64)) > 0)           # strictly increasing with the value (-0 below +0)
    id_ok = (entry & 1).astype(bool)
    assert list(v[id_ok]) == [F(2.0 ** -64), F(1.0), F(255.0), F(2.0 ** 100), F(1e38), F(3e38), F(inf)]  # not 0, 2^-70, negatives, NaN
    xy_ok = (entry & 2).astype(bool)
    assert np.array_equal(xy_ok, np.isfinite(v))
    assert np.array_equal(pixel.astype(bool), np.abs(v) <= F(2.0 ** 100))  # false for NaN, Inf, 1e38


def test_bad_arguments():
    L = _lib.load()
    assert L.dsm_pose_fact_host(-1, None, None) != 0 and L.dsm_pose_fact_host(1, None, None) != 0
    assert L.dsm_fact_rules_host(1, None, None) != 0 and L.dsm_pose_fact_host(0, None, None) == 0
