"""GPU: host/pose_batch_demo.cpp -- detect, search_sc, the batched direct alignment (dsm_host::PoseEstimatorBatch) and the ICP fallback
of the rejected matches, for several sequences at once through the C++ adaptors -- against the Python path on the same inputs."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from _pose_jobs import guess_matrix, make_job, scene_inputs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIDAR_RANGE = 40.0


def cloud(seed, n=1500):
    """a place as pts_spherical: points of a dozen wall segments around the camera, a layout of its own per seed"""
    rng = np.random.default_rng(seed)
    seg = rng.integers(0, 12, n)
    ang = rng.uniform(0, 2 * np.pi, 12)[seg] + rng.normal(0, 0.08, n)
    rad = rng.uniform(4, 36, 12)[seg] + rng.normal(0, 0.4, n)
    return np.stack([rad * np.cos(ang), rng.uniform(-2, 1, n), rad * np.sin(ang)], 1)


def f64(a):
    return np.ascontiguousarray(a, np.float64).tobytes()


def f32(a):
    return np.ascontiguousarray(a, np.float32).tobytes()


def test_cpp_pose_batch_demo_matches_the_python_path(ctx, tmp_path):
    from direct_stereo_slam_amd.tracker import PoseBatch

    # three sequences of the 308x92 geometry; in each the current keyframe revisits the place of earlier keyframe `true_match`;
    # sequence 1 starts direct alignment from the hopeless guess, so its match goes on to ICP
    plan = [(72, 1500, (0.01, 2.0), "identity", 2), (75, 1500, (0.02, -1.0), "far", 0), (77, 2500, (0.0, 3.0), "gt", 1)]
    seqs = []
    for s, (seed, n, (a, b), g, true_match) in enumerate(plan):
        sc, xyz, cols = scene_inputs("small", seed, n, a, b)
        place = cloud(1000 + s)
        hist = []
        for k in range(4):
            sph = place + np.random.default_rng(50 + s).normal(0, 0.02, place.shape) if k == true_match else cloud(2000 + 10 * s + k)
            # only the matched keyframe's points are ever aligned; the others carry a few points of their own
            hist.append((sph, xyz, cols) if k == true_match else (sph, xyz[:50] + 0.5, [c[:50] for c in cols]))
        seqs.append((sc, xyz, cols, g, true_match, hist, place))
    sc0 = seqs[0][0]
    path = tmp_path / "pose_batch.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("iiii", len(seqs), sc0.w, sc0.h, sc0.nl) + struct.pack("d", LIDAR_RANGE))
        for sc, xyz, cols, g, true_match, hist, place in seqs:
            f.write(f32(sc.K) + f64(guess_matrix(sc, g)) + struct.pack("i", len(hist)))
            for sph, kx, kc in hist:
                f.write(struct.pack("i", len(sph)) + f64(sph) + struct.pack("i", len(kx)) + f64(kx))
                for c in kc:
                    f.write(f32(c))
                f.write(struct.pack("f", 1.0))
            f.write(struct.pack("i", len(place)) + f64(place))
            for lvl in sc.new_p:
                f.write(f32(lvl))
            f.write(struct.pack("f", 1.0))
    exe = os.path.join(ROOT, "direct_stereo_slam_amd", "host", "_build", "pose_batch_demo")
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    res = [json.loads(line) for line in out.stdout.strip().splitlines() if line.startswith("{")]
    assert len(res) == len(seqs)
    # the Python path: the same matches in one PoseBatch call
    py = PoseBatch(ctx, sc0.w, sc0.h, sc0.nl).estimate_many([make_job(sc, xyz, cols, g) for sc, xyz, cols, g, *_ in seqs], sc0.nl - 1)
    for r, (sc, xyz, cols, g, true_match, hist, place), (ok, T, err, inl) in zip(res, seqs, py):
        assert true_match in r["candidates"] and r["matched"] == true_match, r
        assert bool(r["ok"]) == ok == (g != "far") and r["inlier_percent"] == inl
        assert np.array_equal(np.array(r["ref_to_new"]).view(np.uint64), T.reshape(16).view(np.uint64))
        assert np.float32(r["pose_error"]) == np.float32(err)
        assert ("icp_ok" in r) == (not ok)  # the ICP fallback ran for the rejected match alone
    icp = [r for r in res if "icp_ok" in r]
    assert len(icp) == 1 and np.isfinite(icp[0]["icp_score"]) and len(icp[0]["icp_tfm"]) == 16
