"""Checker of the distance map and the activation walk: pure numpy / Python, imports nothing from the
package.  The authority is the list BFS (`make_map`, `add`, `activate`), a restatement of CoarseDistanceMap::growDistBFS
(TrackerAndScaler.cpp:1235-1324) and of the walk of FrontEnd.cpp:431-449.  Beside it, independently written:
  - the whole-map dilation form (`make_map_dilate`, `add_dilate`): the frontier of level k is every non-border cell holding k - 1;
  - two forms that are WRONG (`min_of_single_maps`, `all_at_once`), kept only to prove that test inputs tell them apart.
A map is a flat Python list of ints (0 .. 39 or 1000) in the list forms and an (h1, w1) int array in the dilation form;
`as_float` gives the float32 map the C ABI returns."""
import numpy as np

FAR = 1000
OFF4 = ((1, 0), (-1, 0), (0, 1), (0, -1))
OFF8 = OFF4 + ((1, 1), (-1, 1), (-1, -1), (1, -1))
f32 = np.float32


def as_float(m, w1, h1):
    return np.asarray(m, np.float32).reshape(h1, w1)


# ---- the list BFS: the authority ----------------------------------------------------------------------------------------------

def grow_bfs(m, w1, h1, frontier):
    """D3 / D4: level-synchronous, k = 1 .. 39; odd k 8 neighbours, even k 4; strictly '> k'; a border cell is not expanded"""
    for k in range(1, 40):
        if not frontier:  # (the remaining levels would walk an empty list)
            break
        nxt = []
        for c in frontier:
            x, y = c % w1, c // w1
            if x == 0 or y == 0 or x == w1 - 1 or y == h1 - 1:
                continue
            for dx, dy in (OFF8 if k % 2 else OFF4):
                i = c + dx + dy * w1
                if m[i] > k:
                    m[i] = k
                    nxt.append(i)
        frontier = nxt


def make_map(w1, h1, seed_cells):
    """D1 + D3 / D4 from the accepted seeds (cell indices, in order, duplicates allowed as in the reference's list)"""
    m = [FAR] * (w1 * h1)
    for c in seed_cells:
        m[c] = 0
    grow_bfs(m, w1, h1, list(seed_cells))
    return m


def add(m, w1, h1, cell):
    """D5: the cell becomes 0 unconditionally, then the BFS from that single cell on the map as it stands"""
    m[cell] = 0
    grow_bfs(m, w1, h1, [cell])


def project(krki, kt, host, u, v, idepth, w1, h1):
    """D2: float32, ((m0 u + m1 v) + m2) + kt idepth per component; returns (cell or -1, ptp0) per point"""
    M = np.asarray(krki, f32).reshape(-1, 9)[np.asarray(host, np.int64)] if len(host) else np.zeros((0, 9), f32)
    T = np.asarray(kt, f32).reshape(-1, 3)[np.asarray(host, np.int64)] if len(host) else np.zeros((0, 3), f32)
    u, v, d = (np.asarray(a, f32) for a in (u, v, idepth))
    with np.errstate(all="ignore"):
        p = [((M[:, 3 * r] * u + M[:, 3 * r + 1] * v) + M[:, 3 * r + 2]) + T[:, r] * d for r in range(3)]
        assert all(a.dtype == f32 for a in p)
        qu, qv = p[0] / p[2] + f32(0.5), p[1] / p[2] + f32(0.5)
        ok = (qu >= f32(1)) & (qv >= f32(1)) & (qu < f32(w1)) & (qv < f32(h1))  # NaN and +-inf fail
        cell = np.full(len(u), -1, np.int64)
        cell[ok] = qu[ok].astype(np.int64) + w1 * qv[ok].astype(np.int64)
    return cell, p[0]


def activate(w, h, job):
    """D1-D6 for one window.  job: dict with krki, kt, seed_host/u/v/idepth, cand_host/u/v/idepth/type, min_act_dist.
    Returns (map float32 (h1, w1), decisions uint8, info) with info = dict(initial_map, pass_initial: candidates in bounds that
    pass against the map before any activation)."""
    w1, h1 = w >> 1, h >> 1
    sc, _ = project(job["krki"], job["kt"], job["seed_host"], job["seed_u"], job["seed_v"], job["seed_idepth"], w1, h1)
    m = make_map(w1, h1, [int(c) for c in sc if c >= 0])
    m0 = list(m)
    cc, p0 = project(job["krki"], job["kt"], job["cand_host"], job["cand_u"], job["cand_v"], job["cand_idepth"], w1, h1)
    with np.errstate(all="ignore"):
        frac = p0 - np.floor(p0)
        thr = f32(job["min_act_dist"]) * np.asarray(job["cand_type"], f32)
    assert frac.dtype == f32 and thr.dtype == f32
    dec = np.zeros(len(cc), np.uint8)
    pass_initial = 0
    for i, c in enumerate(cc):
        if c < 0:
            dec[i] = 2
            continue
        pass_initial += bool(f32(m0[c]) + frac[i] >= thr[i])
        if f32(m[c]) + frac[i] >= thr[i]:
            dec[i] = 1
            add(m, w1, h1, int(c))
    return as_float(m, w1, h1), dec, dict(initial_map=as_float(m0, w1, h1), pass_initial=pass_initial)


# ---- the whole-map dilation form (independent of the list form) ---------------------------------------------------------------

def _shift_or(src, offs):
    """cells with a neighbour (cell - offset) in src, i.e. src dilated by the offsets"""
    h1, w1 = src.shape
    out = np.zeros_like(src)
    for dx, dy in offs:
        ys, yd = (slice(0, h1 - dy), slice(dy, h1)) if dy >= 0 else (slice(-dy, h1), slice(0, h1 + dy))
        xs, xd = (slice(0, w1 - dx), slice(dx, w1)) if dx >= 0 else (slice(-dx, w1), slice(0, w1 + dx))
        out[yd, xd] |= src[ys, xs]
    return out


def grow_dilate(a):
    h1, w1 = a.shape
    inner = np.zeros((h1, w1), bool)
    inner[1:h1 - 1, 1:w1 - 1] = True
    for k in range(1, 40):
        src = (a == k - 1) & inner
        if not src.any():
            continue
        a[_shift_or(src, OFF8 if k % 2 else OFF4) & (a > k)] = k


def make_map_dilate(w1, h1, seed_cells):
    a = np.full((h1, w1), FAR, np.int64)
    for c in seed_cells:
        a[c // w1, c % w1] = 0
    grow_dilate(a)
    return a


def add_dilate(a, cell):
    h1, w1 = a.shape
    a[cell // w1, cell % w1] = 0
    grow_dilate(a)


# ---- two WRONG forms: only to show that inputs discriminate -------------------------------------------------------------------

def min_of_single_maps(w1, h1, cells):
    """cell-wise minimum over the maps of each seed / added cell alone"""
    out = np.full(w1 * h1, FAR, np.int64)
    for c in cells:
        out = np.minimum(out, np.asarray(make_map(w1, h1, [c]), np.int64))
    return out.reshape(h1, w1)


def all_at_once(w1, h1, cells):
    """every seed and every added cell as seeds of one construction"""
    return np.asarray(make_map(w1, h1, list(cells)), np.int64).reshape(h1, w1)


# ---- inputs -----------------------------------------------------------------------------------------------------------------------

def make_k(fx, fy, cx, cy):
    """K[0], K[1] and the closed-form inverse Ki[0] by the rule of CoarseDistanceMap::makeK (TrackerAndScaler.cpp:1343-1361), float32"""
    fx, fy, cx, cy = (f32(a) for a in (fx, fy, cx, cy))
    K0 = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], f32)
    K1 = np.array([[f32(fx * 0.5), 0, f32((np.float64(cx) + 0.5) / 2 - 0.5)], [0, f32(fy * 0.5), f32((np.float64(cy) + 0.5) / 2 - 0.5)], [0, 0, 1]], f32)
    Ki0 = np.array([[f32(1) / fx, 0, -cx / fx], [0, f32(1) / fy, -cy / fy], [0, 0, 1]], f32)
    return K0, K1, Ki0


def make_case(seed, w, h, n_hosts, n_seeds, n_cand, min_act_dist, types=(1.0, 2.0, 4.0)):
    """a window: hosts with small rotations and translations, raw coordinates from [-4, w + 4) x [-4, h + 4)"""
    rng = np.random.default_rng(seed)
    _, K1, Ki0 = make_k(0.8 * w, 0.8 * w, 0.5 * w - 0.5, 0.5 * h - 0.5)
    krki, kt = np.zeros((n_hosts, 9), f32), np.zeros((n_hosts, 3), f32)
    for i in range(n_hosts):
        r = rng.normal(0, 0.01, 3)
        th = np.linalg.norm(r)
        kx = np.array([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]]) / th
        R = np.eye(3) + np.sin(th) * kx + (1 - np.cos(th)) * kx @ kx
        krki[i] = (K1 @ R.astype(f32) @ Ki0).reshape(9)
        kt[i] = K1 @ rng.normal(0, 0.05, 3).astype(f32)

    def pts(n):
        return (rng.integers(0, max(n_hosts, 1), n).astype(np.int32), rng.uniform(-4, w + 4, n).astype(f32), rng.uniform(-4, h + 4, n).astype(f32),
                rng.uniform(0.1, 2.0, n).astype(f32))

    sh, su, sv, sd = pts(n_seeds)
    ch, cu, cv, cd = pts(n_cand)
    return dict(krki=krki, kt=kt, seed_host=sh, seed_u=su, seed_v=sv, seed_idepth=sd, cand_host=ch, cand_u=cu, cand_v=cv, cand_idepth=cd,
                cand_type=rng.choice(np.asarray(types, f32), n_cand).astype(f32), min_act_dist=float(min_act_dist))


# the cases the host form and the device form are both held to (geometry, then make_case's arguments); small_b is there so that
# three jobs of one geometry can share a batch
CASES = {
    "small": ((64, 48), dict(seed=101, n_hosts=3, n_seeds=20, n_cand=300, min_act_dist=1.5)),
    "no_seeds": ((64, 48), dict(seed=102, n_hosts=3, n_seeds=0, n_cand=200, min_act_dist=2.0)),
    "small_b": ((64, 48), dict(seed=104, n_hosts=2, n_seeds=8, n_cand=300, min_act_dist=1.0)),
    "medium": ((160, 96), dict(seed=103, n_hosts=5, n_seeds=200, n_cand=2000, min_act_dist=2.0)),
}
_cache = {}


def case(name):
    """(w, h, job, expected map, expected decisions, info), computed once per session and shared: treat as read-only"""
    if name not in _cache:
        (w, h), kw = CASES[name]
        job = make_case(w=w, h=h, **kw)
        _cache[name] = (w, h, job) + activate(w, h, job)
    return _cache[name]
