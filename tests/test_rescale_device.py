"""GPU: dsm_window_rescale_batch against the host form dsm_window_rescale_host: both evaluate one header without
contraction, so every output is compared bit for bit; the host form is held to the checker in tests/test_rescale_ref.py."""
import numpy as np
import pytest

import _finish_ref as F
import _linearize_ref as R
import _rescale_ref as RR

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64


def both(ctx, jobs):
    from direct_stereo_slam_amd import rescale

    jobs = [RR.call_job(j) for j in jobs]
    return rescale.window_rescale_batch(ctx, jobs), rescale.window_rescale_host(jobs)


def geometry():
    from direct_stereo_slam_amd import rescale

    return rescale.geometry()


def test_frame_counts_and_tracking_reference(ctx):
    """1, 2, 8 and DSM_WINDOW_MAX_FRAMES frames (256 pair lanes), the tracking reference inside and outside the window, every scale of
    the CPU tests; one call"""
    jobs = [RR.make_scene(seed=100 + n, n_frames=n, n_pts=33, ref=ref, new_scale=s)
            for n, s in ((1, 1.4), (2, 0.1), (8, 50.0), (16, -2.0)) for ref in ((None,) if n == 1 else (None, 0, n - 2))]
    jobs += [RR.scenes()[k] for k in sorted(RR.scenes()) if k.startswith(("scale_", "finished_"))]
    dev, host = both(ctx, jobs)
    for k, (d, h) in enumerate(zip(dev, host)):
        assert d["decision"] == RR.ACCEPTED
        RR.assert_equal(d, h, what=k)


def test_point_counts_at_the_kernels_edges(ctx):
    """0, 1, 63, 64, 65 points, the workgroup size - 1, itself and + 1, and one grid stride + 1: alone and in one call"""
    block, stride = geometry()
    assert block == 256 and stride % block == 0
    sizes = (0, 1, 63, 64, 65, block - 1, block, block + 1, stride + 1)
    jobs = [RR.make_scene(seed=200 + k, n_frames=2 + k % 3, n_pts=m, ref=0, new_scale=1.3) for k, m in enumerate(sizes)]
    dev, host = both(ctx, jobs)
    for m, job, d, h in zip(sizes, jobs, dev, host):
        assert len(d["idepth"]) == m
        RR.assert_equal(d, h, what=m)
        alone, _ = both(ctx, [job])
        RR.assert_equal(alone[0], d, what=("alone", m))


def test_mixed_batches_every_job_is_its_single_call(ctx):
    """batches of 1 and of 5: accepted, rejected and disabled jobs of different sizes; a call without an accepted job launches nothing"""
    s = RR.scenes()
    five = [RR.make_scene(seed=300, n_frames=8, n_pts=300, ref=3), s["rejected"], s["n1_p0"], s["disabled"],
            RR.make_scene(seed=301, n_frames=16, n_pts=65, new_scale=0.7)]
    dev, host = both(ctx, five)
    assert [d["decision"] for d in dev] == [2, 1, 2, 0, 2]
    for k, (job, d, h) in enumerate(zip(five, dev, host)):
        RR.assert_equal(d, h, what=k)
        one_dev, one_host = both(ctx, [job])
        RR.assert_equal(one_dev[0], d, what=("single", k))
        RR.assert_equal(one_host[0], d, what=("single host", k))
    dev, host = both(ctx, [s["rejected_nan"], s["disabled"]])
    for d, h, k in zip(dev, host, ("rejected_nan", "disabled")):
        RR.assert_equal(d, h, what=k)
        for a in RR.ARRAYS:
            assert d[a].tobytes() == np.ascontiguousarray(s[k][a], d[a].dtype).tobytes(), (k, a)


def test_optional_output_null_and_refusals(ctx):
    from direct_stereo_slam_amd import rescale
    from direct_stereo_slam_amd._lib import DsmError

    job = RR.call_job(RR.make_scene(seed=400, n_frames=3, n_pts=70, ref=1))
    b = rescale.RescaleBatch([dict(job, all_poses=False), job])
    b.run(ctx)
    lean, full = b.results()
    assert (lean["cam_to_world_all"] == rescale.FILL).all()
    RR.assert_equal(lean, full, keys=[k for k in RR.ALL_OUT if k != "cam_to_world_all"])
    for bad in (dict(job, new_scale=0.0), dict(job, n_frames=17), dict(job, fails=-1), dict(job, drop="ad_host"), dict(job, drop="decision")):
        b = rescale.RescaleBatch([job, bad])
        with pytest.raises(DsmError):
            b.run(ctx)
        for out in b.all_outputs():
            for k, v in out.items():
                assert (v == (77 if k in rescale.WORDS else rescale.FILL)).all(), k


def test_chain_marginalize_and_nullspace_from_device_and_host(ctx):
    """the finished 5-frame scene, the scale accepted, frame 1 leaving: dsm_window_marginalize_batch and dsm_window_nullspace_batch fed
    from the device's outputs equal the same calls fed from the host form's, bit for bit; and the prior differs from the one without
    the rescale"""
    from direct_stereo_slam_amd import marginalize, nullspace, step

    job, frames, loop, fin = F.expected("scene", 2)
    mjob, rk, pk = F.marginalize_job(job, loop, fin, 1)
    rjob = RR.finished_scene("scene")
    assert len(rjob["idepth"]) == len(pk)
    (dev,), (host,) = both(ctx, [rjob])
    RR.assert_equal(dev, host)
    win = step.KeyframeWindow(ctx, R.W, R.H, len(frames))
    for fid, img in zip(job["frame_ids"], frames):
        win.put_host(int(fid), img)

    expo = np.where(np.asarray(job["exposure"], f32) > 0, np.asarray(job["exposure"], f32), f32(1.0))  # the nullspace call wants them positive

    def chain(r):
        m = dict(mjob, window=win, cam=tuple(r["cam"][:4]), cam_inv=tuple(r["cam"][4:]), idepth_scaled=r["idepth_scaled"],
                 idepth_zero_scaled=r["idepth_zero_scaled"], delta=r["delta"], ad_ht_delta=r["ad_ht_delta"], c_delta=r["c_delta"],
                 **{k: r[k] for k in RR.PRE})
        marg = marginalize.window_marginalize_batch(ctx, [m])[0]
        null = nullspace.window_nullspace_batch(ctx, [dict(world_to_cam_eval=r["world_to_cam_eval"], state_zero=r["state_zero"], exposure=expo)])[0]
        return marg, null

    (md, nd), (mh, nh) = chain(dev), chain(host)
    plain = marginalize.window_marginalize_batch(ctx, [dict(mjob, window=win)])[0]
    win.close()
    for a, b in ((md, mh), (nd, nh)):
        for k in a:
            assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k
    assert np.isfinite(md["H_M_out"]).all() and md["H_M_out"].tobytes() != plain["H_M_out"].tobytes()
