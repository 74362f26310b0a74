"""The authority for the pixel selection: numpy float32, written from the rules with upstream's sequential
select() loop -- the running counter n2 behind every direction and the bestIdx = -2 flags.  It shares no code with the library.
Also the scene the selection tests run on, the cases (CASES at 96 x 64 and 104 x 72; EDGE_CASES at remainder and camera sizes), and what
the coverage assertions of tests/test_select_ref.py and tests/test_select_edges_ref.py count."""
import functools

import numpy as np

f32 = np.float32
DIRECTIONS = [(0, 1), (.3827, .9239), (.1951, .9808), (.9239, .3827), (.7071, .7071), (.3827, -.9239), (.8315, .5556), (.8315, -.5556),
              (.5556, -.8315), (.9808, .1951), (.9239, -.3827), (.7071, -.7071), (.5556, .8315), (.9808, -.1951), (1, 0), (.1951, -.9808)]
PATTERN = [(0, -2), (-1, -1), (1, -1), (-2, 0), (0, 0), (2, 0), (-1, 1), (0, 2)]
DEFAULTS = dict(min_grad_hist_cut=0.5, min_grad_hist_add=7.0, grad_downweight_per_level=0.75, select_direction_distribution=1, th_factor=1.0,
                recursions=1, pattern_padding=2, outlier_th=144.0, outlier_th_sum_component=2500.0, overall_energy_th_weight=1.0)
UNINITIALIZED = 5
SHAPES = [(96, 64), (104, 72)]
POTENTIALS = [1, 2, 3, 5, 7]


# ---- the scene -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene(w, h, seed=7):
    """integer-valued intensities in [0, 255]: texture (8 sinusoids + noise); the left quarter vertical bars of period 6 (gy = 0
    exactly); a ramp of slope 12 and a diagonal ramp of slope 4 (too flat for level 0, steep enough on level 1 and on level 2); a weak smooth wave"""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    v = np.full((h, w), 128.0)
    for lam in np.linspace(5.0, 31.0, 8):
        th, ph = rng.uniform(0, np.pi), rng.uniform(0, 2 * np.pi)
        v += 11.0 * np.sin(2 * np.pi / lam * (xs * np.cos(th) + ys * np.sin(th)) + ph)
    v += rng.normal(0, 3.0, v.shape)
    q = w // 4
    v[:, :q] = 128.0 + 60.0 * np.sin(2 * np.pi / 6.0 * xs[:, :q])  # bars
    tri = lambda t, s, period: s * np.abs((t % period) - period / 2.0)
    y0, y1 = 6, h // 2 + 8
    xa, xb = q + 4, q + 42
    v[y0:y1, xa:xb] = 30.0 + tri(xs[y0:y1, xa:xb], 12.0, 32.0)  # ramp, slope 12: level-1 hits it, level 0 does not
    v[y0:y1, xb:w - 4] = 60.0 + tri(xs[y0:y1, xb:w - 4] + ys[y0:y1, xb:w - 4], 4.0, 48.0)  # diagonal ramp, slope 4: only level 2 hits it
    yw = y1 + 3
    v[yw:h - 2, q + 4:q + 36] = 128.0 + 9.0 * np.sin(2 * np.pi / 17.0 * (xs[yw:h - 2, q + 4:q + 36] + 0.5 * ys[yw:h - 2, q + 4:q + 36]))  # weak wave
    return np.clip(np.rint(v), 0, 255).astype(f32)


def pattern(w, h, seed=3141592):
    return np.random.default_rng(seed).integers(0, 256, w * h, dtype=np.uint8)


def b_inv_table():
    """a smooth, strictly increasing inverse response"""
    x = np.arange(256, dtype=np.float64)
    return (255.0 * (x / 255.0) ** 1.3).astype(f32)


def pyramid(I0):
    """levels 0, 1, 2: 2 x 2 means, (a + b + c + d) * 0.25 in float32"""
    out = [np.ascontiguousarray(I0, f32)]
    for _ in range(2):
        a = out[-1]
        hl, wl = a.shape[0] // 2, a.shape[1] // 2
        a = a[:2 * hl, :2 * wl]
        out.append((f32(0.25) * (((a[0::2, 0::2] + a[0::2, 1::2]) + a[1::2, 0::2]) + a[1::2, 1::2])).astype(f32))
    return out


# ---- P1 --------------------------------------------------------------------------------------------------------------------------
def gradients(I):
    """central differences on the flat index for idx in [w, w (h - 1)): rows 0 and h - 1 stay zero; in columns 0 and w - 1 of the other
    rows the x difference wraps into the neighbouring row"""
    I = np.ascontiguousarray(I, f32)
    h, w = I.shape
    gx, gy = np.zeros_like(I), np.zeros_like(I)
    flat = I.reshape(-1)
    with np.errstate(invalid="ignore", over="ignore"):
        gx.reshape(-1)[w:w * (h - 1)] = f32(0.5) * (flat[w + 1:w * (h - 1) + 1] - flat[w - 1:w * (h - 1) - 1])
        gy[1:-1, :] = f32(0.5) * (I[2:, :] - I[:-2, :])
    gx[~np.isfinite(gx)] = 0
    gy[~np.isfinite(gy)] = 0
    return gx, gy


def abs_grad(I, b_inv=None):
    gx, gy = gradients(I)
    ag = gx * gx + gy * gy
    if b_inv is not None:
        c = np.clip((I + f32(0.5)).astype(np.int64), 5, 250)
        gw = np.asarray(b_inv, f32)[c + 1] - np.asarray(b_inv, f32)[c]
        ag = ag * (gw * gw)
        ag[0, :] = ag[-1, :] = 0
    return ag.astype(f32), gx, gy


# ---- P2, P3 ----------------------------------------------------------------------------------------------------------------------
def thresholds(ag0, S):
    h, w = ag0.shape
    w32, h32 = w // 32, h // 32
    ths = np.zeros((h32, w32), f32)
    for y in range(h32):
        for x in range(w32):
            hist = [0] * 50
            for j in range(32):
                for i in range(32):
                    it, jt = i + 32 * x, j + 32 * y
                    if it > w - 2 or jt > h - 2 or it < 1 or jt < 1:
                        continue
                    g = int(np.sqrt(ag0[jt, it]))
                    hist[min(g, 48) + 1] += 1
                    hist[0] += 1
            th = int(f32(hist[0]) * f32(S["min_grad_hist_cut"]) + f32(0.5))
            q = 90
            for i in range(90):
                th -= hist[i + 1] if i + 1 < 50 else 0
                if th < 0:
                    q = i
                    break
            ths[y, x] = f32(q) + f32(S["min_grad_hist_add"])
    sm = np.zeros_like(ths)
    for y in range(h32):
        for x in range(w32):
            num, s = 0, f32(0)
            for dx, dy in [(-1, -1), (-1, 1), (-1, 0), (1, -1), (1, 1), (1, 0), (0, -1), (0, 1), (0, 0)]:
                if 0 <= x + dx < w32 and 0 <= y + dy < h32:
                    num, s = num + 1, f32(s + ths[y + dy, x + dx])
            m = f32(s / f32(num))
            sm[y, x] = f32(m * m)
    return sm


class Frame:
    """everything select() reads of one frame, as Python lists for the sequential loop"""

    def __init__(self, I0, b_inv, S):
        self.h, self.w = I0.shape
        self.S = S
        self.I = pyramid(I0)
        ag0, gx, gy = abs_grad(self.I[0], b_inv)
        self.ag = [ag0.tolist(), abs_grad(self.I[1], b_inv)[0].tolist(), abs_grad(self.I[2], b_inv)[0].tolist()]
        self.ths_smoothed = thresholds(ag0, S)
        w32, h32 = self.w // 32, self.h // 32
        bx = np.minimum(np.arange(self.w) >> 5, w32 - 1)
        by = np.minimum(np.arange(self.h) >> 5, h32 - 1)
        t0 = self.ths_smoothed[by[:, None], bx[None, :]].astype(f32)
        dw, f = f32(S["grad_downweight_per_level"]), f32(S["th_factor"])
        t1 = t0 * dw
        t2 = t1 * f32(dw * dw)
        self.th = [(t0 * f).tolist(), (t1 * f).tolist(), (t2 * f).tolist()]
        self.clamped = int(((np.arange(self.w) >> 5) >= w32).sum()), int(((np.arange(self.h) >> 5) >= h32).sum())
        with np.errstate(invalid="ignore", over="ignore"):
            self.dirnorm = [np.abs(gx * f32(dx) + gy * f32(dy)).astype(f32).tolist() for dx, dy in DIRECTIONS]
        self.dd = bool(S["select_direction_distribution"])

    def rank(self, l, d, xf, yf, ag_l):
        return self.dirnorm[d][yf][xf] if self.dd else ag_l


def select(F, rp, pot):
    """PixelSelector::select as upstream's one loop.  Returns (map, [n2, n3, n4], the cells' n2 on entry in scan order)"""
    w, h = F.w, F.h
    out = np.zeros((h, w), np.uint8)
    n2 = n3 = n4 = 0
    entered = []
    for y4 in range(0, h, 4 * pot):
        for x4 in range(0, w, 4 * pot):
            my3, mx3 = min(4 * pot, h - y4), min(4 * pot, w - x4)
            best4, val4 = -1, 0.0
            dir4 = int(rp[n2]) & 15
            for y3 in range(0, my3, 2 * pot):
                for x3 in range(0, mx3, 2 * pot):
                    x34, y34 = x3 + x4, y3 + y4
                    my2, mx2 = min(2 * pot, h - y34), min(2 * pot, w - x34)
                    best3, val3 = -1, 0.0
                    dir3 = int(rp[n2]) & 15
                    for y2 in range(0, my2, pot):
                        for x2 in range(0, mx2, pot):
                            x234, y234 = x2 + x34, y2 + y34
                            my1, mx1 = min(pot, h - y234), min(pot, w - x234)
                            best2, val2 = -1, 0.0
                            dir2 = int(rp[n2]) & 15
                            entered.append((x234, y234, n2))
                            for y1 in range(my1):
                                for x1 in range(mx1):
                                    xf, yf = x1 + x234, y1 + y234
                                    idx = xf + w * yf
                                    if xf < 4 or xf >= w - 5 or yf < 4 or yf > h - 4:
                                        continue
                                    ag0 = F.ag[0][yf][xf]
                                    if ag0 > F.th[0][yf][xf]:
                                        dn = F.rank(0, dir2, xf, yf, ag0)
                                        if dn > val2:
                                            val2, best2, best3, best4 = dn, idx, -2, -2
                                    if best3 == -2:
                                        continue
                                    ag1 = F.ag[1][int(yf * 0.5 + 0.25)][int(xf * 0.5 + 0.25)]
                                    if ag1 > F.th[1][yf][xf]:
                                        dn = F.rank(1, dir3, xf, yf, ag1)
                                        if dn > val3:
                                            val3, best3, best4 = dn, idx, -2
                                    if best4 == -2:
                                        continue
                                    ag2 = F.ag[2][int(yf * 0.25 + 0.125)][int(xf * 0.25 + 0.125)]
                                    if ag2 > F.th[2][yf][xf]:
                                        dn = F.rank(2, dir4, xf, yf, ag2)
                                        if dn > val4:
                                            val4, best4 = dn, idx
                            if best2 > 0:
                                out[best2 // w, best2 % w] = 1
                                val3 = 1e10
                                n2 += 1
                    if best3 > 0:
                        out[best3 // w, best3 % w] = 2
                        val4 = 1e10
                        n3 += 1
            if best4 > 0:
                out[best4 // w, best4 % w] = 4
                n4 += 1
    return out, [n2, n3, n4], entered


# ---- P10 - P14 -------------------------------------------------------------------------------------------------------------------
def adapt(n, density, pot, left):
    """-> (quot, ideal, the next potential or 0)"""
    have, want = f32(n[0] + n[1] + n[2]), f32(density)
    with np.errstate(divide="ignore"):
        quot = f32(want / have)
    K = f32(f32(have * f32(pot + 1)) * f32(pot + 1))
    ideal = max(1, min(4096, int(f32(np.sqrt(f32(K / want))) - f32(1))))
    if left > 0 and quot > f32(1.25) and pot > 1:
        return quot, ideal, (pot - 1 if ideal >= pot else ideal)
    if left > 0 and quot < f32(0.25):
        return quot, ideal, (min(pot + 1, 4096) if ideal <= pot else ideal)
    return quot, ideal, 0


def select_ref(I0, rp, potential, density, max_pts, b_inv=None, **kw):
    """makeNewTraces on one frame: the result dict of direct_stereo_slam_amd.pixelselect, plus `trace`: per pass (potential, counts,
    the cells' entries) and `way`: how P10 went after the first pass, and whether P11 thinned"""
    S = dict(DEFAULTS, **kw)
    I0 = np.ascontiguousarray(I0, f32)
    h, w = I0.shape
    F = Frame(I0, b_inv, S)
    pot, left, passes, trace = int(potential), int(S["recursions"]), 0, []
    while True:
        m, n, entered = select(F, rp, pot)
        passes += 1
        quot, ideal, nxt = adapt(n, density, pot, left)
        trace.append(dict(potential=pot, counts=list(n), entered=entered, next=nxt))
        if not nxt:
            break
        pot, left = nxt, left - 1
    num_total, thinned = sum(n), False
    if quot < f32(0.95):
        thinned = True
        char_th = int(f32(255) * quot)
        flat = m.reshape(-1)
        rn = 0
        for i in np.flatnonzero(flat):
            if rp[rn] > char_th:
                flat[i] = 0
                num_total -= 1
            rn += 1
    pad = int(S["pattern_padding"])
    gx, gy = gradients(I0)
    C = f32(S["outlier_th_sum_component"])
    eth = f32(f32(f32(8) * f32(S["outlier_th"])) * f32(f32(S["overall_energy_th_weight"]) * f32(S["overall_energy_th_weight"])))
    pts, lost_rows = [], 0
    for y in range(h):
        for x in range(w):
            if not m[y, x]:
                continue
            if not (pad + 1 <= y < h - pad - 2 and pad + 1 <= x < w - pad - 2):
                lost_rows += y == h - 4
                continue
            G, color, wt, ok = [f32(0)] * 4, [], [], True
            for dx, dy in PATTERN:
                c = I0[y + dy, x + dx]
                if not np.isfinite(c):
                    ok = False
                    break
                a, b = gx[y + dy, x + dx], gy[y + dy, x + dx]
                G = [f32(G[0] + a * a), f32(G[1] + a * b), f32(G[2] + a * b), f32(G[3] + b * b)]
                color.append(c)
                wt.append(f32(np.sqrt(f32(C / f32(C + f32(a * a + b * b))))))
            if ok and np.isfinite(eth):
                pts.append((x, y, G, color, wt, m[y, x]))
    n_pts = len(pts)
    pts = pts[:max_pts]
    k = len(pts)
    res = dict(potential=ideal, n_pts=n_pts, num_total=num_total, counts=np.array(n, np.int32), passes=passes, map=m,
               u=np.array([p[0] for p in pts], f32), v=np.array([p[1] for p in pts], f32), energy_th=np.full(k, eth, f32),
               grad_h=np.array([p[2] for p in pts], f32).reshape(k, 4), color=np.array([p[3] for p in pts], f32).reshape(k, 8),
               weights=np.array([p[4] for p in pts], f32).reshape(k, 8), status=np.full(k, UNINITIALIZED, np.uint8),
               idepth_min=np.zeros(k, f32), idepth_max=np.full(k, np.nan, f32), quality=np.full(k, 10000.0, f32),
               type=np.array([p[5] for p in pts], f32))
    way = "neither" if len(trace) == 1 else ("down" if trace[1]["potential"] < trace[0]["potential"] else "up")
    res["info"] = dict(trace=trace, way=way, thinned=thinned, lost_rows=int(lost_rows), frame=F)
    return res


def cell_masks(F, pot):
    """per cell of the padded nested order (16 per 4 pot block; cells cut away are empty): the directions under which it is a hit"""
    w, h = F.w, F.h
    masks = []
    for y4 in range(0, h, 4 * pot):
        for x4 in range(0, w, 4 * pot):
            for l in range(16):
                x0, y0 = x4 + (((l >> 2) & 1) * 2 + (l & 1)) * pot, y4 + (((l >> 3) & 1) * 2 + ((l >> 1) & 1)) * pot
                m = 0
                for yf in range(y0, min(y0 + pot, h)):
                    for xf in range(x0, min(x0 + pot, w)):
                        if xf < 4 or xf >= w - 5 or yf < 4 or yf > h - 4 or not F.ag[0][yf][xf] > F.th[0][yf][xf]:
                            continue
                        for d in range(16):
                            if F.rank(0, d, xf, yf, F.ag[0][yf][xf]) > 0:
                                m |= 1 << d
                masks.append(m)
    return masks


def chain_groups(masks):
    """(groups of 64 cells whose masks are all 0 or 0xFFFF, the other groups)"""
    fast = slow = 0
    for g in range(0, len(masks), 64):
        if all(m in (0, 0xFFFF) for m in masks[g:g + 64]):
            fast += 1
        else:
            slow += 1
    return fast, slow


KEYS = ("u", "v", "energy_th", "grad_h", "color", "weights", "status", "idepth_min", "idepth_max", "quality", "type")


def assert_equal(got, exp, with_map=True):
    """integers equal, floats equal bit for bit (NaN patterns included)"""
    for k in ("potential", "n_pts", "num_total", "passes"):
        assert got[k] == exp[k], (k, got[k], exp[k])
    assert got["counts"].tolist() == exp["counts"].tolist(), (got["counts"], exp["counts"])
    if with_map:
        assert np.array_equal(got["map"], exp["map"]), f"{int((got['map'] != exp['map']).sum())} map entries differ"
    for k in KEYS:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(exp[k])
        assert a.shape == b.shape and a.dtype == b.dtype, (k, a.shape, b.shape, a.dtype, b.dtype)
        if a.dtype == np.float32:
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), k
        else:
            assert np.array_equal(a, b), k


# ---- the cases the host form (tests/test_select_ref.py) and the device form (tests/test_select_device.py) are compared on ------------
def _cases():
    c = {}
    for w, h in SHAPES:
        for pot in POTENTIALS:  # one pass at a fixed potential
            c[f"{w}x{h}-pot{pot}"] = dict(shape=(w, h), potential=pot, density=1500.0, params=dict(recursions=0))
        for pot, density in [(3, 300.0), (3, 3000.0), (3, 30.0), (1, 150.0), (3, 60.0)]:  # P10 and P11
            c[f"{w}x{h}-adapt{pot}-{int(density)}"] = dict(shape=(w, h), potential=pot, density=density, params={})
    w, h = SHAPES[1]
    c["b_inv"] = dict(shape=(w, h), potential=2, density=400.0, b_inv=True, params={})
    c["no_direction_distribution"] = dict(shape=(w, h), potential=2, density=400.0, params=dict(select_direction_distribution=0))
    c["max_pts_below_yield"] = dict(shape=(w, h), potential=2, density=400.0, max_pts=37, params={})
    c["constant_image"] = dict(shape=(w, h), potential=3, density=1500.0, constant=True, params={})
    c["three_passes"] = dict(shape=(w, h), potential=7, density=650.0, params=dict(recursions=2))  # 7 -> 2 -> 1
    c["padding3_thfactor2"] = dict(shape=(w, h), potential=1, density=2000.0, params=dict(pattern_padding=3, th_factor=2.0, min_grad_hist_add=5.0))
    return c


CASES = _cases()
MAX_PTS = 1500


def image_of(case):
    w, h = case["shape"]
    return np.full((h, w), 77.0, f32) if case.get("constant") else scene(w, h)


def job_of(case, **more):
    """the job dict of direct_stereo_slam_amd.pixelselect for a case (without its tracker)"""
    return dict(density=case["density"], potential=case["potential"], max_pts=case.get("max_pts", MAX_PTS),
                b_inv=b_inv_table() if case.get("b_inv") else None, **more)


@functools.lru_cache(maxsize=None)
def expected(name):
    """the checker's result for a case, computed once and shared: do not modify it"""
    case = CASES[name]
    w, h = case["shape"]
    return select_ref(image_of(case), pattern(w, h), case["potential"], case["density"], case.get("max_pts", MAX_PTS),
                      b_inv_table() if case.get("b_inv") else None, **case["params"])


# ---- remainder and camera sizes: a short case list of their own (SHAPES multiplies every case, these do not) ------------------------------
EDGE_SHAPES = [(105, 73), (106, 70), (107, 75), (33, 33), (63, 47)]  # w % 4 = 1, 2, 3 and odd h or h % 4 = 2; one 32-block; w32 = h32 = 1
CAMERA_SHAPES = [(1241, 376), (1226, 370)]  # tests/golden/cams
EDGE_MAX_PTS = 1500
CAMERA_MAX_PTS = 26000
UP_DENSITY = {(33, 33): 4.0, (63, 47): 12.0}  # what sends potential 3 up (quot < 0.25) where the frame has few cells


def _edge_cases():
    c = {}
    for w, h in EDGE_SHAPES:
        s = f"{w}x{h}"
        for pot in (1, 3, 7, 40):  # 4 * 40 exceeds both sides: a single padded block
            c[f"{s}-pot{pot}"] = dict(shape=(w, h), potential=pot, density=1500.0, params=dict(recursions=0))
        c[f"{s}-down"] = dict(shape=(w, h), potential=3, density=3000.0, params={})
        c[f"{s}-up"] = dict(shape=(w, h), potential=3, density=UP_DENSITY.get((w, h), 30.0), params={})
        c[f"{s}-pot4096"] = dict(shape=(w, h), potential=4096, density=1500.0, params=dict(recursions=0))
        c[f"{s}-pot4096-rec2"] = dict(shape=(w, h), potential=4096, density=1500.0, params=dict(recursions=2))
    for w, h in CAMERA_SHAPES:
        s = f"{w}x{h}"
        c[f"{s}-pot1"] = dict(shape=(w, h), potential=1, density=20000.0, max_pts=CAMERA_MAX_PTS, params={})  # quot 0.31: one pass
        c[f"{s}-pot3"] = dict(shape=(w, h), potential=3, density=2000.0, max_pts=CAMERA_MAX_PTS, params={})
        c[f"{s}-pot4096-rec2"] = dict(shape=(w, h), potential=4096, density=2000.0, max_pts=CAMERA_MAX_PTS, params=dict(recursions=2))
    w, h = CAMERA_SHAPES[1]
    c[f"{w}x{h}-pot5"] = dict(shape=(w, h), potential=5, density=3000.0, max_pts=CAMERA_MAX_PTS, params={})  # the fourth job of the batch
    w, h = EDGE_SHAPES[2]
    c["no_point_arrays"] = dict(shape=(w, h), potential=3, density=300.0, max_pts=0, params={})
    return c


EDGE_CASES = _edge_cases()
BATCH_OF_FOUR = [f"1226x370-{k}" for k in ("pot1", "pot3", "pot4096-rec2", "pot5")]  # run under one dsm_select_params: batch_expected


def edge_job_of(case, **more):
    return dict(density=case["density"], potential=case["potential"], max_pts=case.get("max_pts", EDGE_MAX_PTS), b_inv=None, **more)


@functools.lru_cache(maxsize=None)
def edge_expected(name):
    """the checker's result for an edge case, computed once and shared: do not modify it"""
    case = EDGE_CASES[name]
    w, h = case["shape"]
    return select_ref(scene(w, h), pattern(w, h), case["potential"], case["density"], case.get("max_pts", EDGE_MAX_PTS), None, **case["params"])


@functools.lru_cache(maxsize=None)
def batch_expected(name, recursions):
    """a batch has one dsm_select_params: the case's job under `recursions`.  Shared with edge_expected where the case's own is the same"""
    case = EDGE_CASES[name]
    if dict(DEFAULTS, **case["params"])["recursions"] == recursions:
        return edge_expected(name)
    w, h = case["shape"]
    return select_ref(scene(w, h), pattern(w, h), case["potential"], case["density"], case.get("max_pts", EDGE_MAX_PTS), None,
                      **dict(case["params"], recursions=recursions))


def null_point_arrays(batch, j):
    """job j of a pixelselect.SelectBatch without any point array (allowed with max_pts = 0)"""
    for k in ("u", "v", "energy_th", "grad_h", "color", "weights", "status", "idepth_min", "idepth_max", "quality", "type"):
        setattr(batch.arr[j], k, None)
    assert not batch.arr[j].u and not batch.arr[j].status


def level2_last_column_reads(F):
    """P1, P9: the scanned pixels that read level 2 in its last column w_2 - 1 -> (how many, how many of them have ag_2 > t2 under
    the flat-index rule, how many would under a rule that zeroes the border columns)"""
    w, h = F.w, F.h
    w2 = w >> 2
    reads = new = old = 0
    for yf in range(4, h - 3):
        for xf in range(4, w - 5):
            if int(xf * 0.25 + 0.125) != w2 - 1:
                continue
            reads += 1
            above = F.ag[2][int(yf * 0.25 + 0.125)][w2 - 1] > F.th[2][yf][xf]
            new += above
            old += 0.0 > F.th[2][yf][xf]
    return reads, new, old


# ---- for tools/select_host_standalone.cpp ------------------------------------------------------------------------------------------
def dump_scene(path, w, h):
    """the scene file the stand-alone program reads: int32 w, h, the planes of levels 0, 1, 2, the random pattern"""
    with open(path, "wb") as f:
        f.write(np.array([w, h], np.int32).tobytes())
        for a in pyramid(scene(w, h)):
            f.write(a.tobytes())
        f.write(pattern(w, h).tobytes())


def fingerprint(res):
    """what the stand-alone program prints for a result"""
    def fnv(hsh, data):
        for b in data:
            hsh = ((hsh ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
        return hsh

    hp = 1469598103934665603
    for k in ("u", "v", "energy_th", "grad_h", "color", "weights", "idepth_min", "idepth_max", "quality", "type"):
        a = np.ascontiguousarray(res[k], f32).reshape(-1).copy()
        a[np.isnan(a)] = np.nan
        hp = fnv(hp, a.tobytes())
    hp = fnv(hp, res["status"].tobytes())
    return dict(counts=[int(c) for c in res["counts"]], n_pts=res["n_pts"], num_total=res["num_total"], passes=res["passes"],
                potential=res["potential"], map_hash=f"{fnv(1469598103934665603, res['map'].tobytes()):016x}", points_hash=f"{hp:016x}")
