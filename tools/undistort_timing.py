"""Cost of the undistorted hand-over (dsm_upload_images_undistorted) against the plain u8 one (dsm_upload_images).

One process; the legs alternate within every repetition and each timed window is one batched synchronous hand-over of
512 stereo pairs (1024 images from page-locked buffers) between two device synchronisations.  Legs per camera:
  plain   -- DSM_PIXEL_U8 bytes already at the working size (what the replay leg hands over today)
  crop    -- raw camera bytes, undistorted crop (the shipped camera file)
  crop_pv -- the same with a response G and a vignette map (mode 0)
plus a host float32 numpy restatement of one image's undistortion (labelled CPU).  Prints one JSON line.

    python tools/undistort_timing.py [--pairs 512] [--reps 10]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from direct_stereo_slam_amd import synth as S  # noqa: E402
from direct_stereo_slam_amd._lib import c_float_p, c_int_p, check  # noqa: E402
from direct_stereo_slam_amd.tracker import Context, TrackerAndScaler, Undistorter, pinned_array, read_camera_file  # noqa: E402

CAMS = os.path.join(ROOT, "tests", "golden", "cams")
CAMERAS = {  # camera file, output size override (preset 2), pyramid levels
    "kitti": (os.path.join(CAMS, "kitti", "0_2", "camera0.txt"), None, 5),
    "robotcar_preset2": (os.path.join(CAMS, "robotcar", "camera0.txt"), (424, 320), 4),
}


def host_undistort(img, rx, ry, G, vig):
    """float32 numpy restatement of Undistort::undistort (photometric value, bilinear remap in upstream's order)"""
    h_in, w_in = img.shape
    p = (G[img] * vig).reshape(-1)
    out = rx < 0
    x, y = np.where(out, 0, rx), np.where(out, 0, ry)
    xi, yi = x.astype(np.int32), y.astype(np.int32)
    ax, ay = x - xi, y - yi
    axy = ax * ay
    b = xi + yi * w_in
    v = axy * p[b + 1 + w_in] + (ay - axy) * p[b + w_in] + (ax - axy) * p[b + 1] + (np.float32(1) - ax - ay + axy) * p[b]
    return np.where(out, np.float32(0), v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=512)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    ctx = Context(0)
    L = ctx.L
    rng = np.random.default_rng(0)
    n = 2 * a.pairs
    result = {"pairs": a.pairs, "images_per_handover": n, "reps": a.reps}
    for cam, (path, size_out, nl) in CAMERAS.items():
        cf = read_camera_file(path)
        (w_in, h_in), (w, h) = cf["size_in"], size_out or cf["size_out"]
        G = (255.0 * (np.arange(256) / 255.0) ** 0.8).astype(np.float32)
        X, Y = np.meshgrid(np.linspace(-1, 1, w_in), np.linspace(-1, 1, h_in))
        vig = (1.0 / (1.0 - 0.15 * (X * X + Y * Y))).astype(np.float32)
        und = {"crop": Undistorter.pinhole(ctx, path, size_out=(w, h)),
               "crop_pv": Undistorter.pinhole(ctx, path, size_out=(w, h), G=G, vignette_inv=vig)}
        K = und["crop"].K
        trks = [TrackerAndScaler(ctx, w, h, nl, S.KITTI_T_STEREO, K) for _ in range(a.pairs)]
        hs = (C.c_void_p * n)(*([t.h for t in trks] * 2))
        slots = np.array([0] * a.pairs + [1] * a.pairs, np.int32)
        ex = np.ones(n, np.float32)
        raw = [pinned_array((h_in, w_in), np.uint8) for _ in range(n)]
        work = [pinned_array((h, w), np.uint8) for _ in range(n)]
        for im in raw + work:
            im[...] = rng.integers(0, 256, im.shape, dtype=np.uint8)
        p_raw = (C.c_void_p * n)(*[im.ctypes.data for im in raw])
        p_work = (C.c_void_p * n)(*[im.ctypes.data for im in work])
        sl, exp = slots.ctypes.data_as(c_int_p), ex.ctypes.data_as(c_float_p)
        legs = {
            "plain": lambda: check(L.dsm_upload_images(ctx.h, n, hs, sl, p_work, exp, 1, 0)),
            "crop": lambda: check(L.dsm_upload_images_undistorted(ctx.h, und["crop"].h, n, hs, sl, p_raw, exp, 0, 0)),
            "crop_pv": lambda: check(L.dsm_upload_images_undistorted(ctx.h, und["crop_pv"].h, n, hs, sl, p_raw, exp, 0, 0)),
        }
        times = {k: [] for k in legs}
        for rep in range(a.warmup + a.reps):
            for k, fn in legs.items():
                ctx.sync()
                t0 = time.perf_counter()
                fn()
                ctx.sync()
                if rep >= a.warmup:
                    times[k].append((time.perf_counter() - t0) * 1e3)
        res = {"size_in": [w_in, h_in], "size_out": [w, h], "levels": nl}
        for k, v in times.items():
            res[f"{k}_ms"] = round(float(np.median(v)), 3)
            res[f"{k}_ms_min"] = round(float(np.min(v)), 3)
        res["crop_over_plain"] = round(res["crop_ms"] / res["plain_ms"], 3)
        res["crop_pv_over_plain"] = round(res["crop_pv_ms"] / res["plain_ms"], 3)
        # CPU: the host restatement of one image's photometric correction + remap
        from direct_stereo_slam_amd.tracker import pinhole_undistort_map

        _, _, rx, ry = pinhole_undistort_map(cf["calib"], cf["size_in"], "crop", (w, h))
        img = np.asarray(raw[0]).copy()
        host_undistort(img, rx, ry, G, vig)
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            host_undistort(img, rx, ry, G, vig)
            ts.append((time.perf_counter() - t0) * 1e3)
        res["cpu_numpy_ms_per_image"] = round(float(np.median(ts)), 3)
        result[cam] = res
        for u in und.values():
            u.close()
        for t in trks:
            t.close()
        del raw, work
    print(json.dumps(result))


if __name__ == "__main__":
    main()
