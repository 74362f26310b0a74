"""GPU: dsm_window_admit_batch against the host form dsm_window_admit_host: both evaluate one header without
contraction, so every output is compared bit for bit; the host form is held to the checker in tests/test_admit_ref.py."""
import numpy as np
import pytest

import _admit_ref as AR
import _finish_ref as F
import _linearize_ref as R

pytestmark = pytest.mark.gpu

f32, f64, i32, u8 = np.float32, np.float64, np.int32, np.uint8


def both(ctx, jobs, ap=None):
    from direct_stereo_slam_amd import admit

    jobs = [AR.call_job(j) for j in jobs]
    ap = admit.default_params(**ap) if ap else None
    return admit.window_admit_batch(ctx, jobs, ap=ap), admit.window_admit_host(jobs, ap=ap)


def geometry():
    from direct_stereo_slam_amd import admit

    return admit.geometry()


def test_frame_counts(ctx):
    """1, 2, 7 and 15 old frames (16 frames = 256 pair lanes), the tracking reference inside and outside the window, the optional
    arrays given and NULL, the CPU tests' scenes and the second-keyframe windows of the finish chain; one call"""
    jobs = [AR.make_scene(seed=100 + n, n_frames=n, n_pts=33, ref=ref, optional=opt)
            for n, opt in ((1, True), (2, False), (7, True), (15, True), (15, False)) for ref in ((None,) if n == 1 else (None, 0, n - 1))]
    jobs += [AR.scenes()[k] for k in sorted(AR.scenes())] + [AR.chain_scene(k) for k in AR.CHAINS]
    dev, host = both(ctx, jobs)
    for k, (d, h) in enumerate(zip(dev, host)):
        AR.assert_equal(d, h, what=k)


def with_n_res(seed, n_frames, n_res):
    """a scene of exactly n_res residuals: points of n_frames - 1 residuals each and one with the remainder"""
    per = n_frames - 1
    counts = [per] * (n_res // per) + ([n_res % per] if n_res % per else [])
    job = AR.make_scene(seed=seed, n_frames=n_frames, n_pts=len(counts), counts=tuple(counts) or (0,), optional=False)
    assert len(job["point"]) == n_res
    return job


def test_point_and_residual_counts_at_the_kernels_edges(ctx):
    """0, 1, 63, 64, 65 points, the workgroup size - 1, itself and + 1, and one grid stride + 1, with one residual each and with none;
    the same residual counts over fewer points; empty runs first, last and in the middle: alone and in one call"""
    block, stride = geometry()
    assert block == 256 and stride % block == 0
    sizes = (0, 1, 63, 64, 65, block - 1, block, block + 1, stride + 1)
    jobs = [AR.make_scene(seed=200 + k, n_frames=2 + k % 3, n_pts=m, counts=(1,), optional=k % 2 == 0) for k, m in enumerate(sizes)]
    jobs += [AR.make_scene(seed=220 + k, n_frames=3, n_pts=m, counts=(0,), optional=False) for k, m in enumerate((65, stride + 1))]
    jobs += [with_n_res(240 + k, 7, m) for k, m in enumerate(sizes)]
    jobs += [AR.make_scene(seed=260, n_frames=7, n_pts=block + 3, counts=(0, 0, 2, 5, 0, 0, 6, 1, 0), optional=False), AR.scenes()["n7_empty_first_last_middle"]]
    for job, m in zip(jobs, sizes):
        assert len(job["host"]) == m and len(job["point"]) == m
    dev, host = both(ctx, jobs)
    for k, (job, d, h) in enumerate(zip(jobs, dev, host)):
        assert d["n_res"] == len(job["point"]) + len(job["host"])
        AR.assert_equal(d, h, what=k)
        alone, _ = both(ctx, [job])
        AR.assert_equal(alone[0], d, what=("alone", k))


def test_mixed_batches_every_job_is_its_single_call(ctx):
    """batches of 1 and of 5 mixing sizes"""
    s = AR.scenes()
    five = [AR.make_scene(seed=300, n_frames=7, n_pts=300, ref=3), s["n1_p0"], AR.make_scene(seed=301, n_frames=15, n_pts=65, optional=False), s["n2_p1"],
            with_n_res(302, 4, 2100)]
    dev, host = both(ctx, five)
    for k, (job, d, h) in enumerate(zip(five, dev, host)):
        AR.assert_equal(d, h, what=k)
        one_dev, one_host = both(ctx, [job])
        AR.assert_equal(one_dev[0], d, what=("single", k))
        AR.assert_equal(one_host[0], d, what=("single host", k))


def test_optional_arrays_null_and_refusals(ctx):
    from direct_stereo_slam_amd import admit
    from direct_stereo_slam_amd._lib import DsmError

    job = AR.call_job(AR.make_scene(seed=400, n_frames=3, n_pts=70, ref=1))
    lean_job = dict(job, distances=False, **{k: None for k in AR.GROWN})
    b = admit.AdmitBatch([lean_job, job])
    b.run(ctx)
    lean, full = b.results()
    assert not any(k in lean for k in AR.GROWN + ("distance_ll",))
    for out in (b.all_outputs()[0][k + "_out"] for k in AR.GROWN + ("distance_ll",)):
        assert (out == admit.FILL).all()
    AR.assert_equal(lean, full, keys=[k for k in AR.ALL_OUT if k not in AR.GROWN + ("distance_ll",)])
    ungrouped = dict(job, point=np.asarray(job["point"])[::-1].copy())
    for bad in (dict(job, n_frames=16), dict(AR.call_job(AR.make_scene(seed=401, n_frames=15, n_pts=3)), n_frames=16), dict(job, drop="host"),
                dict(job, drop="n_flagged"), dict(job, drop="prior_zero"), ungrouped, dict(job, new_exposure=float("inf"))):
        b = admit.AdmitBatch([job, bad])
        with pytest.raises(DsmError):
            b.run(ctx)
        for out in b.all_outputs():
            for k, v in out.items():
                assert (v == v.dtype.type(admit.FILL if v.dtype in (f32, f64) else admit.FILL_INT)).all(), k
    for ap in (dict(min_frames=-1), dict(max_frames=-1), dict(min_points_remaining=float("nan")), dict(max_log_aff_fac_in_window=float("inf"))):
        b = admit.AdmitBatch([job, lean_job])  # valid jobs: the parameters alone are refused
        with pytest.raises(DsmError):
            b.run(ctx, ap=admit.default_params(**ap))
        for out in b.all_outputs():
            for k, v in out.items():
                assert (v == v.dtype.type(admit.FILL if v.dtype in (f32, f64) else admit.FILL_INT)).all(), (ap, k)


def test_scripted_flags(ctx):
    """the scenes of tests/test_admit_ref.py whose flags are stated by name, through the device: the double exp and the float logf and
    sqrtf decide the same flags and give the same scores, bit for bit"""
    for what, job, ap, expected in AR.flag_script():
        (d,), (h,) = both(ctx, [job], ap=ap)
        assert list(d["flagged"]) == expected + [0] and d["n_flagged"] == sum(expected), what
        AR.assert_equal(d, h, what=what)


def test_chain_finish_on_the_admitted_window_from_device_and_host(ctx):
    """the shrunken second-keyframe window of the 5-frame scene, the new frame admitted and its plane put into the dsm_window:
    dsm_window_finish_batch fed from the device's outputs equals the same call fed from the host form's, bit for bit, and differs from
    the finish of the window without the new frame"""
    from direct_stereo_slam_amd import finish, step

    ch = F.checker_chain("scene", 2)
    two, frames2 = ch["two"], ch["frames2"]
    ajob = AR.chain_scene("scene")
    (dev,), (host,) = both(ctx, [ajob])
    AR.assert_equal(dev, host)
    n = len(two["frame_ids"])
    planes = list(frames2) + [frames2[-1]]  # the new frame lies a small motion off the newest one
    win = step.KeyframeWindow(ctx, R.W, R.H, n + 1)
    for fid, img in zip(dev["keyframe_id"], planes):
        win.put_host(int(fid), img)

    def admitted(r):
        return dict(two, window=win, max_iterations=2, frame_ids=r["keyframe_id"], frame_energy_th=r["frame_energy_th"], point=r["point"], target=r["target"],
                    state_in=r["res_state"], energy_in=r["energy"], is_new=r["is_new"], ad_host=r["ad_host"].reshape(n + 1, n + 1, 8, 8),
                    ad_target=r["ad_target"].reshape(n + 1, n + 1, 8, 8), H_L=r["H_L"].reshape(12 + 8 * n, -1), b_L=r["b_L"], H_M=r["H_M"].reshape(12 + 8 * n, -1),
                    b_M=r["b_M"], state_prior=r["prior"], state_prior_zero=r["prior_zero"], world_to_cam_eval=r["world_to_cam_eval"].reshape(n + 1, 7),
                    state_zero=r["state_zero"].reshape(n + 1, 8), state_backup=r["state"].reshape(n + 1, 8), exposure=r["exposure"],
                    last_res=r["last_res"].reshape(-1, 2), last_state_in=r["last_state"].reshape(-1, 2))

    (ld, fd), (lh, fh) = finish.window_finish_batch(ctx, [admitted(dev), admitted(host)])
    plain_l, plain_f = finish.window_finish_batch(ctx, [dict(two, window=win, max_iterations=2)])[0]
    win.close()

    def same(a, b, what):
        for k in a:
            if isinstance(a[k], dict):
                same(a[k], b[k], k)
            elif a[k] is None or isinstance(a[k], str):
                assert a[k] == b[k], (what, k)
            else:
                x, y = np.asarray(a[k]), np.asarray(b[k])
                assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), (what, k)

    same(ld, lh, "loop"), same(fd, fh, "finish")
    assert len(fd["new_state"]) == len(two["point"]) + len(two["host"])
    # the new frame's residuals entered the optimisation: some of them are IN after the final linearisation, they carry energy, and
    # the old frames' committed states moved with them
    forward = np.asarray(dev["target"]) == n
    assert forward.sum() == len(two["host"]) and (np.asarray(fd["new_state"])[forward] == AR.IN).sum() > 0
    assert float(np.asarray(fd["new_energy"], f32)[forward & (np.asarray(fd["new_state"]) == AR.IN)].sum()) > 0.0
    assert float(fd["energy"]) != float(plain_f["energy"]) and int(fd["n_res_out"]) > int(plain_f["n_res_out"])
    assert np.asarray(ld["state"]).reshape(-1, 8)[:n].tobytes() != np.asarray(plain_l["state"]).reshape(-1, 8).tobytes()
