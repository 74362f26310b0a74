"""What tests/test_eval_trip_edges.py and tools/record_eval_trip_edges.py share: the point counts at which the evaluation loop's
per-wave trip bound and its peeled last trip can go wrong, the scenes they run on, templates of a chosen count, and the byte record
of one evaluation's outputs.

The counts (eval_chunk_impl, tracker_kernels.hip: a wave runs Pw = clamp(ceil((n - chunk_start - 64 wave) / 256), 1, P) trips, the last
one peeled in the two-point loop):
    1, 63, 64, 65, 255, 256, 257                       P = 1: trip bound 1, upper waves empty
    511, 512, 513, 1024, 1025, 2048, 2049              P = 2, 4, 8, 16 at their first and last point: one trip short of P, odd Pw
    4095, 4096, 4097, 4096 + {63, 64, 65, 255, 256, 257}   a last chunk of one point, one wave, one full trip, one trip and one point
    8191, 8193
Under the latency table (1) the same counts run at P = 1 up to 4095 and P = 2 from 4096: many chunks, the last one at every fill.

The scenes: 96 x 64 with two levels, the smallest image whose level 0 is several chunks.  A tracker holds at most width x height points
per level (dsm_tracker_set_ref), so level 0 of it takes the counts up to 6144 and level 1 those up to 1536; the others run on a
288 x 128 image (level 1: 144 x 64 = 9216 texels), same camera, same scene family.  A template of n points is the level's dense
template repeated cyclically: every evaluation form and the float64 reference take any list of points."""
import numpy as np

import _scenes
from _scenes import make_scene

COUNTS = (1, 63, 64, 65, 255, 256, 257,
          511, 512, 513, 1024, 1025, 2048, 2049,
          4095, 4096, 4097, 4096 + 63, 4096 + 64, 4096 + 65, 4096 + 255, 4096 + 256, 4096 + 257,
          8191, 8193)
CUTOFF = 20.0
SCALE = 1.0

# (width, height, level of the KITTI camera the default intrinsics are taken from, levels); the camera itself: centred, KITTI's baseline
_scenes.SIZES.setdefault("trip96", (96, 64, 3, 2))
_scenes.CAMERAS.setdefault("trip96", ((90.0, 90.0, 47.5, 31.5), -0.5372))
_scenes.SIZES.setdefault("trip288", (288, 128, 3, 2))
_scenes.CAMERAS.setdefault("trip288", ((180.0, 180.0, 143.5, 63.5), -0.5372))
SCENES = ("trip96", "trip288")


def scene(name):
    return make_scene(name, seed=41)


def capacity(sc, lvl):
    return (sc.w >> lvl) * (sc.h >> lvl)


def counts_of(name, lvl):
    """the counts that run on level lvl of scene `name`: on the small image whatever fits it, on the large one the rest"""
    small, large = (_scenes.SIZES[s] for s in SCENES)
    cap_small = (small[0] >> lvl) * (small[1] >> lvl)
    cap_large = (large[0] >> lvl) * (large[1] >> lvl)
    assert max(COUNTS) <= cap_large
    return [n for n in COUNTS if (n <= cap_small) == (name == SCENES[0])]


def template_of(sc, lvl, n):
    """sc's template with level lvl made n points long: its dense points repeated cyclically, from the middle of the level on, twenty
    points into a row (the first rows and columns leave the image under the true motion, and the small counts are to be met on points
    that count)"""
    full = len(sc.tpl[0][lvl])
    idx = (full // 2 + 20 + np.arange(n)) % full
    return [[np.ascontiguousarray(a[l][idx]) if l == lvl else a[l] for l in range(sc.nl)] for a in sc.tpl]


def bits(out):
    """the outputs of an evaluation as bytes (tests/test_eval_forms_f64.py's _bits): rs, H, b (or h00, h01) and the warped count"""
    return b"".join(np.ascontiguousarray(a, np.float32 if isinstance(a, float) else None).tobytes() for a in out)


def key(name, kind, lvl, table, n, ro):
    return f"{name}/{kind}/l{lvl}/t{table}/n{n}/{'ro' if ro else 'full'}"


def evaluate(trk, kind, lvl, sc, ro, form=0):
    if kind == "pose":
        return trk.diagEvalPose(lvl, sc.gt_pose, list(sc.gt_aff), CUTOFF, form=form, residual_only=ro)
    return trk.diagEvalScale(lvl, SCALE, CUTOFF, form=form, residual_only=ro)


def pack(records):
    """{key: bytes} -> the arrays of the fixture file: per kind the keys and one row of bytes per key"""
    out = {}
    for kind in ("pose", "scale"):
        keys = sorted(k for k in records if f"/{kind}/" in k)
        out[f"{kind}_keys"] = np.array(keys)
        out[f"{kind}_bits"] = np.stack([np.frombuffer(records[k], np.uint8) for k in keys])
    return out


def unpack(npz):
    return {str(k): npz[f"{kind}_bits"][i].tobytes() for kind in ("pose", "scale") for i, k in enumerate(npz[f"{kind}_keys"])}
