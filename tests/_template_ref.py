"""The checker of the template builder (csrc/template_kernels.hip, dsm_make_coarse_depth_l0): what makeCoarseDepthL0
(TrackerAndScaler.cpp:143-315) returns, restated on 2-D float32 arrays.  numpy only.

It is not the loop nest a fourth time.  The C forms (oracle/dsm_oracle.c, csrc/host_capi.cpp) walk flat indices, dilate in place and let a
neighbour offset run over a row's end into the next row (or, at i = wl, in front of the array); here every plane is [hl, wl], every
neighbour is a shifted view of a zero-padded plane, so a neighbour outside the image does not exist, and the emit is a boolean mask.
The two agree on every emitted entry because an emitted pixel has x in 2 .. wl-3 and y in 2 .. hl-3: its four neighbours lie inside the
image and inside their own rows, and what the dilation writes at x = 0 or x = wl-1 (the only targets that see a wrapped neighbour) is
read by nothing -- a dilated pixel is a hole, and holes are never read as neighbours; the 2 x 2 sums are taken before any dilation.

Operation order, all in float32:
  splat     u = trunc(pu + 0.5f), v = trunc(pv + 0.5f) (toward zero: C's float -> int);  idepth[v, u] += pidepth * pweight and
            weight[v, u] += pweight, one point after the other in list order (np.add.at: unbuffered and sequential), from zero planes;
  2x2 sums  level l from the UNDILATED level l-1 over the floor-halved crop: ((a + b) + c) + d with a = (2x, 2y), b = (2x+1, 2y),
            c = (2x, 2y+1), d = (2x+1, 2y+1);
  dilation  rows 1 .. hl-2, every pixel with bak <= 0 (bak = the undilated weights; NaN is not a hole): over the neighbours
            (dx, dy) = (+1,+1) (-1,-1) (-1,+1) (+1,-1) on levels 0-1, (+1,0) (-1,0) (0,+1) (0,-1) above, in that order,
            sum += idepth, num += bak, numn += 1 where bak[neighbour] > 0;  if numn > 0: idepth = sum / numn, weight = num / numn;
  emit      x in 2 .. wl-3, y in 2 .. hl-3, row-major: keep when weight > 0, the colour is finite and idepth / weight > 0;
            the entry is (float(x), float(y), idepth / weight, colour).
The coordinate contract (`accepted`): a point is taken exactly when pu + 0.5f and pv + 0.5f are finite and truncate into
[0, w) x [0, h); the reference itself would write out of bounds otherwise (:160), the library refuses the whole call.

tests/test_template_ref.py holds this against the C oracle and the host form and asserts what each case below is there for;
tests/test_template_edges.py holds the device against it.  Nothing here has a tolerance.
"""
import functools
from types import SimpleNamespace

import numpy as np

F = np.float32
HALF = F(0.5)
EMIT_BLOCK, EMIT_THREADS, WAVE = 1024, 256, 64  # the emit compaction's structure (template_kernels.hip: kEmitBlock, kEmitThreads)


def accepted(pu, pv, w, h):
    """the coordinate contract, per point"""
    with np.errstate(invalid="ignore", over="ignore"):
        su, sv = np.asarray(pu, F) + HALF, np.asarray(pv, F) + HALF
        tu, tv = np.trunc(su), np.trunc(sv)
        return np.isfinite(su) & np.isfinite(sv) & (tu >= 0) & (tu < w) & (tv >= 0) & (tv < h)


def pixels(pu, pv):
    """(u, v) of accepted points"""
    return np.trunc(np.asarray(pu, F) + HALF).astype(np.int64), np.trunc(np.asarray(pv, F) + HALF).astype(np.int64)


def _shift(plane, dx, dy):
    """plane[y + dy, x + dx], zero outside the image"""
    hl, wl = plane.shape
    p = np.zeros((hl + 2, wl + 2), F)
    p[1:-1, 1:-1] = plane
    return p[1 + dy:1 + dy + hl, 1 + dx:1 + dx + wl]


DIAGONAL = ((1, 1), (-1, -1), (-1, 1), (1, -1))
AXIS = ((1, 0), (-1, 0), (0, 1), (0, -1))


def make_coarse_depth(w, h, nlevels, pu, pv, pidepth, pweight, planes):
    """planes[l]: the keyframe's intensity at level l, [h >> l, w >> l].  Returns a namespace with
    lists = [pc_u, pc_v, pc_idepth, pc_color], each a list per level (the arguments of setCoarseTrackingRef);
    sums = [(idepth, weight)] per level before the dilation; dilated = [(idepth, weight)] per level after it."""
    pu, pv, pidepth, pweight = (np.ascontiguousarray(a, F) for a in (pu, pv, pidepth, pweight))
    ok = accepted(pu, pv, w, h)
    if not ok.all():
        raise ValueError("point %d is outside the level-0 image" % int(np.nonzero(~ok)[0][0]))
    with np.errstate(all="ignore"):
        u, v = pixels(pu, pv)
        idp, wgt = np.zeros((h, w), F), np.zeros((h, w), F)
        np.add.at(idp, (v, u), pidepth * pweight)
        np.add.at(wgt, (v, u), pweight)
        sums = [(idp, wgt)]
        for l in range(1, nlevels):
            wl, hl = w >> l, h >> l
            sums.append(tuple(((m[0:2 * hl:2, 0:2 * wl:2] + m[0:2 * hl:2, 1:2 * wl:2]) + m[1:2 * hl:2, 0:2 * wl:2]) + m[1:2 * hl:2, 1:2 * wl:2]
                              for m in sums[-1]))
        dilated, lists = [], [[], [], [], []]
        for l, (idp, bak) in enumerate(sums):
            hl, wl = bak.shape
            hole = bak <= 0
            hole[0], hole[hl - 1] = False, False
            s, num, numn = np.zeros((hl, wl), F), np.zeros((hl, wl), F), np.zeros((hl, wl), F)
            for dx, dy in (DIAGONAL if l < 2 else AXIS):
                nb, ni = _shift(bak, dx, dy), _shift(idp, dx, dy)
                m = nb > 0
                s, num, numn = np.where(m, s + ni, s), np.where(m, num + nb, num), np.where(m, numn + F(1), numn)
            fill = hole & (numn > 0)
            did, dws = np.where(fill, s / numn, idp), np.where(fill, num / numn, bak)
            assert did.dtype == F and dws.dtype == F
            dilated.append((did, dws))
            ci, cw, cc = did[2:hl - 2, 2:wl - 2], dws[2:hl - 2, 2:wl - 2], np.asarray(planes[l], F)[2:hl - 2, 2:wl - 2]
            q = ci / cw
            ys, xs = np.nonzero((cw > 0) & np.isfinite(cc) & (q > 0))
            for lst, a in zip(lists, ((xs + 2).astype(F), (ys + 2).astype(F), q[ys, xs], cc[ys, xs])):
                lst.append(np.ascontiguousarray(a, F))
    return SimpleNamespace(lists=lists, sums=sums, dilated=dilated, counts=[len(a) for a in lists[0]])


def emit_coordinates(x, y, wl):
    """(block, pass, wave, lane) of the emit compaction's item of pixel (x, y), and the item index itself"""
    item = (np.asarray(y, np.int64) - 2) * (wl - 4) + np.asarray(x, np.int64) - 2
    r = item % EMIT_BLOCK
    return item // EMIT_BLOCK, r // EMIT_THREADS, (r % EMIT_THREADS) // WAVE, r % WAVE, item


def emit_blocks(wl, hl):
    return ((wl - 4) * (hl - 4) + EMIT_BLOCK - 1) // EMIT_BLOCK if wl > 4 and hl > 4 else 0


# ---- cases -----------------------------------------------------------------------------------------------------------------------

# name: (w, h, levels).  mini4: the coarsest interior is 4 x 4 = 16 items, less than a wave.  g68: interiors 64 x 64 = 4096 (exactly four
# emit blocks, an interior row = a wave), 30 x 30 = 900 (one partial block), 13 x 13 = 169 (first pass only).  odd: floor halving drops the
# last row (135 -> 67 -> 33).  tiny: collisions and values.  big: 1036 x 1020 = 1 056 720 interior items = 1032 emit blocks, so the
# block-count scan's second pass covers 8 blocks.
GEOMETRIES = {"mini4": (64, 64, 4), "g68": (68, 68, 3), "odd": (240, 135, 3), "tiny": (154, 46, 2), "big": (1040, 1024, 2)}
SMALL = ("mini4", "g68", "odd", "tiny")
NONFINITE = (np.nan, np.inf, -np.inf)


def _planes(geom, seed, nonfinite=False):
    """intensity planes per level; nonfinite: NaN, +inf, -inf at the first, a middle and the last interior pixel of every level"""
    w, h, nl = GEOMETRIES[geom]
    rng = np.random.default_rng(seed)
    out, bad = [], []
    for l in range(nl):
        wl, hl = w >> l, h >> l
        p = rng.uniform(0, 255, (hl, wl)).astype(F)
        if nonfinite:
            at = ((2, 2), (wl // 2, hl // 2 - 1), (wl - 3, hl - 3))
            for (x, y), val in zip(at, NONFINITE):
                p[y, x] = val
            bad.append(at)
        out.append(p)
    return out, bad


def _values(rng, n):
    pid = rng.uniform(0.05, 2.0, n).astype(F)
    pw = np.sqrt(1e-3 / (rng.uniform(1e-3, 10, n) + 1e-12)).astype(F)  # the weights the reference forms (:158)
    return pid, pw


def _below(x):
    return np.nextafter(F(x), F(-np.inf))


def _on_pixels(rng, xs, ys):
    """one point on each pixel, a little off its centre, in shuffled list order"""
    xs, ys = np.asarray(xs).ravel(), np.asarray(ys).ravel()
    o = rng.permutation(len(xs))
    pu = (xs[o] + rng.uniform(-0.45, 0.45, len(xs))).astype(F)
    pv = (ys[o] + rng.uniform(-0.45, 0.45, len(xs))).astype(F)
    return (pu, pv) + _values(rng, len(xs))


def _border(rng, w, h, n):
    """coordinates over the whole accepted range; the first points are pinned to the eight border columns and rows and to (-1.5, -0.5)"""
    pu = np.minimum(rng.uniform(-0.5, w - 0.5, n).astype(F), _below(w - 0.5))  # (the conversion may round up to w - 0.5: refused)
    pv = np.minimum(rng.uniform(-0.5, h - 0.5, n).astype(F), _below(h - 0.5))
    k = 0
    for c in (0, 1, w - 2, w - 1):
        pu[k:k + 3] = c
        k += 3
    for r in (0, 1, h - 2, h - 1):
        pv[k:k + 3] = r
        k += 3
    pu[k:k + 4] = (-1.4, -0.6, _below(w - 0.5), 5.25)  # (-1.5, -0.5) truncates to pixel 0, as in the reference
    pv[k:k + 4] = (7.5, -1.2, -0.9, _below(h - 0.5))
    return (pu, pv) + _values(rng, n)


def _case(geom, pts, seed=1, nonfinite=False, **notes):
    w, h, nl = GEOMETRIES[geom]
    planes, bad = _planes(geom, seed, nonfinite)
    pu, pv, pid, pw = (np.ascontiguousarray(a, F) for a in pts)
    return SimpleNamespace(geom=geom, w=w, h=h, nl=nl, planes=planes, bad=bad, pu=pu, pv=pv, pid=pid, pw=pw, **notes)


COLLISION_SEED = 3  # chosen so that reversing the colliding points changes the emitted bits (asserted in tests/test_template_ref.py)
N_COLLIDING = 300


def _collisions(geom, seed=COLLISION_SEED):
    """300 points on one pixel with weights over six decades, scattered through the list among background points; a second pixel is hit by
    the first and the last point of the list"""
    w, h, _ = GEOMETRIES[geom]
    rng = np.random.default_rng(seed)
    nbg = 200
    px, py, qx, qy = w // 2 + 1, h // 2, w // 3, h // 2 + 3
    n = nbg + N_COLLIDING + 2
    pu = rng.uniform(3, w - 4, n).astype(F)
    pv = rng.uniform(3, h - 4, n).astype(F)
    pid, pw = _values(rng, n)
    where = np.sort(rng.choice(np.arange(1, n - 1), N_COLLIDING, replace=False))
    pu[where] = (px + rng.uniform(-0.4, 0.4, N_COLLIDING)).astype(F)
    pv[where] = (py + rng.uniform(-0.4, 0.4, N_COLLIDING)).astype(F)
    pw[where] = (10.0 ** rng.uniform(-3, 3, N_COLLIDING)).astype(F)
    pu[[0, n - 1]], pv[[0, n - 1]] = qx, qy
    # nothing else on the two pixels
    u, v = pixels(pu, pv)
    other = np.ones(n, bool)
    other[where], other[[0, n - 1]] = False, False
    clash = other & (((u == px) & (v == py)) | ((u == qx) & (v == qy)))
    pu[clash] += F(2)
    return _case(geom, (pu, pv, pid, pw), colliding=where, pixel=(px, py), pixel2=(qx, qy))


def _values_case(geom="tiny"):
    """zero and negative weights (holes that are dilated over), NaN and inf weights, NaN and inf idepths, an idepth of exactly 0 and a
    negative weighted sum, each alone on an interior pixel with ordinary points on its diagonal neighbours"""
    w, h, _ = GEOMETRIES[geom]
    rng = np.random.default_rng(11)
    special = [(0.7, 0.0), (0.7, -0.3), (0.7, np.nan), (0.7, np.inf), (0.7, -np.inf), (np.nan, 0.4), (np.inf, 0.4), (-np.inf, 0.4),
               (0.0, 0.4), (-0.6, 0.4), (-0.0, 0.4)]
    xs, ys, pid, pw = [], [], [], []
    for k, (d, wt) in enumerate(special):
        x, y = 8 + 12 * k, 10 + 7 * (k % 4)
        xs.append(x), ys.append(y), pid.append(d), pw.append(wt)
        for dx, dy in DIAGONAL[: 2 + k % 3]:
            xs.append(x + dx), ys.append(y + dy), pid.append(rng.uniform(0.1, 2)), pw.append(rng.uniform(0.01, 1))
    # a pixel whose weights cancel exactly (a hole) and one whose weighted sum is negative although its weight is positive
    for d, wt in ((1.0, 0.5), (1.5, -0.5)):
        xs.append(20), ys.append(40), pid.append(d), pw.append(wt)
    for x, y, d, wt in ((19, 39, 0.8, 0.3), (21, 41, 0.9, 0.2)):
        xs.append(x), ys.append(y), pid.append(d), pw.append(wt)
    for d, wt in ((1.0, 0.5), (-3.0, 0.25)):
        xs.append(60), ys.append(40), pid.append(d), pw.append(wt)
    nb = 150
    bu, bv = rng.uniform(3, w - 4, nb), rng.uniform(3, h - 4, nb)
    bid, bw = _values(rng, nb)
    near = (np.abs(np.rint(bu)[:, None] - np.array(xs)[None]) <= 2) & (np.abs(np.rint(bv)[:, None] - np.array(ys)[None]) <= 2)
    bu, bv, bid, bw = (a[~near.any(1)] for a in (bu, bv, bid, bw))  # the special pixels and their neighbours stay as placed
    pts = (np.concatenate([np.array(xs, F), bu.astype(F)]), np.concatenate([np.array(ys, F), bv.astype(F)]),
           np.concatenate([np.array(pid, F), bid]), np.concatenate([np.array(pw, F), bw]))
    o = rng.permutation(len(pts[0]))
    return _case(geom, tuple(a[o] for a in pts), specials=[(8 + 12 * k, 10 + 7 * (k % 4)) for k in range(len(special))])


def _blocks_case():
    """68 x 68, level 0: interior row r = image row r + 2 is one wave; a pass is 4 rows, an emit block 16.  Block 0 (image rows 2-17) gets
    entries, block 1 (rows 18-33) none -- the nearest points sit in row 16 and dilate into row 17 --, block 2 (rows 34-49) only in its
    last pass (rows 46-49: points in rows 47 and 48), block 3 entries at lane 0 (x = 2) and lane 63 (x = 65) of one wave."""
    rng = np.random.default_rng(21)
    xs = list(rng.integers(0, 68, 60)) + [2, 65, 30] + list(rng.integers(3, 65, 12)) + [2, 65, 2, 65]
    ys = list(rng.integers(0, 17, 60)) + [16, 16, 16] + list(rng.integers(47, 49, 12)) + [55, 55, 60, 61]
    return _case("g68", _on_pixels(rng, xs, ys))


def _two_pass_case():
    """1040 x 1024: 20 000 points over the whole accepted range, 600 of them in the last ten image rows, so that entries come from items
    below and above item 1 048 576 = 1024 emit blocks (interior row 1012.1: image rows from 1015 on lie wholly above it)"""
    w, h, _ = GEOMETRIES["big"]
    rng = np.random.default_rng(31)
    pu, pv, pid, pw = _border(rng, w, h, 20000)
    pv[1000:1600] = rng.uniform(1013.6, 1023.4, 600).astype(F)
    return _case("big", (pu, pv, pid, pw))


def _build(name):
    kind, _, geom = name.partition("-")
    w, h, nl = GEOMETRIES[geom]
    rng = np.random.default_rng(sum(map(ord, name)))
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "border":
        return _case(geom, _border(rng, w, h, max(64, w * h // 8)))
    if kind == "dense":
        return _case(geom, _on_pixels(rng, xx, yy), nonfinite=True)
    if kind == "empty":
        z = np.zeros(0, F)
        return _case(geom, (z, z, z, z))
    if kind == "single":
        return _case(geom, (np.array([w // 2 + 0.3], F), np.array([h // 2 - 0.2], F), np.array([0.8], F), np.array([0.1], F)))
    if kind == "dilated":  # one point on pixel (1, 1): outside the interior, so the only entry is its dilation into (2, 2)
        return _case(geom, (np.array([1.2], F), np.array([0.9], F), np.array([0.8], F), np.array([0.1], F)))
    if kind == "negative":  # one point with idepth < 0: its own pixel and every pixel dilated from it are left out
        return _case(geom, (np.array([w // 2], F), np.array([h // 2], F), np.array([-0.8], F), np.array([0.1], F)))
    if kind == "collisions":
        return _collisions(geom)
    if kind == "values":
        return _values_case(geom)
    if kind == "checker":  # a checkerboard: diagonal neighbours of a hole are holes (levels 0-1 fill nothing), axis neighbours are not
        m = (xx + yy) % 2 == 0
        return _case(geom, _on_pixels(rng, xx[m], yy[m]))
    if kind == "lattice":  # even x and even y: a hole at (odd, odd) has four diagonal neighbours, one at (odd, even) has none
        m = (xx % 2 == 0) & (yy % 2 == 0)
        return _case(geom, _on_pixels(rng, xx[m], yy[m]))
    if kind == "rows":  # rows 0, 1, h-2, h-1 only: row 1 dilates into row 2, row 0 is never a target
        m = np.isin(yy, (0, 1, h - 2, h - 1))
        return _case(geom, _on_pixels(rng, xx[m], yy[m]))
    if kind == "columns":
        m = np.isin(xx, (0, 1, w - 2, w - 1))
        return _case(geom, _on_pixels(rng, xx[m], yy[m]))
    if kind == "blocks":
        return _blocks_case()
    if kind == "twopass":
        return _two_pass_case()
    raise KeyError(name)


CASES = ([f"{k}-{g}" for k in ("border", "dense", "checker", "lattice", "rows", "columns") for g in SMALL]
         + [f"{k}-{g}" for k in ("empty", "single", "dilated", "negative") for g in ("mini4", "g68", "tiny")]
         + ["collisions-tiny", "collisions-g68", "values-tiny", "blocks-g68", "twopass-big"])


@functools.lru_cache(maxsize=None)
def case(name):
    """the case and its reference result (`.ref`), computed once per session and shared: treat both as read-only"""
    c = _build(name)
    c.name = name
    c.ref = make_coarse_depth(c.w, c.h, c.nl, c.pu, c.pv, c.pid, c.pw, c.planes)
    for a in (c.pu, c.pv, c.pid, c.pw, *c.planes, *[x for lst in c.ref.lists for x in lst]):
        a.setflags(write=False)
    return c


def dip(planes):
    """[h, w, 3] pyramid levels with the planes as channel 0 (the C forms read channel 0 alone)"""
    out = []
    for p in planes:
        d = np.zeros(p.shape + (3,), F)
        d[..., 0] = p
        out.append(d)
    return out
