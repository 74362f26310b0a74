"""Row N2, batched: dsm_pose_estimate_batch / tracker.PoseBatch -- PoseEstimator::estimate (PoseEstimator.cpp:298-506) of many
ScanContext matches in one call.  Expected values come from oracle.OraclePoseEstimator; the bits from the single call
dsm_pose_estimator_estimate, which every job of a batch must reproduce whatever the batch size, its place in the batch and the
scheduling form of the LM kernels."""
import ctypes as C

import numpy as np
import pytest

from _pose_jobs import GUESSES, geometry_jobs, guess_matrix, make_job, oracle_order_spread, oracle_result, scene_inputs, small_jobs

INVALID = -1  # DSM_ERR_INVALID


def params_with(**kw):
    from direct_stereo_slam_amd.tracker import default_params

    p = default_params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


_SINGLE = {}


def single_results(ctx, entries, params=None, key="default"):
    """dsm_pose_estimator_estimate of every entry on one handle of the entries' geometry: [(ok, T, err)]"""
    from direct_stereo_slam_amd.tracker import PoseEstimator

    out, pe = [], None
    for sc, xyz, cols, g, _ in entries:
        k = (key, id(sc), len(xyz), g)
        if k not in _SINGLE:
            if pe is None:
                pe = PoseEstimator(ctx, sc.w, sc.h, sc.nl, params)
            _SINGLE[k] = pe.estimate(xyz, cols, 1.0, sc.new_p, 1.0, sc.K, sc.nl - 1, guess_matrix(sc, g))
        out.append(_SINGLE[k])
    if pe is not None:
        pe.close()
    return out


def batch_results(ctx, entries, params=None):
    from direct_stereo_slam_amd.tracker import PoseBatch

    sc = entries[0][0]
    pb = PoseBatch(ctx, sc.w, sc.h, sc.nl, params)
    res = pb.estimate_many([e[4] for e in entries], sc.nl - 1)
    pb.close()
    return res


def assert_same_bits(batch, single, what):
    assert len(batch) == len(single)
    for i, ((ok_b, T_b, err_b, _), (ok_s, T_s, err_s)) in enumerate(zip(batch, single)):
        assert ok_b == ok_s, (what, i)
        assert np.array_equal(np.asarray(T_b).view(np.uint64), np.asarray(T_s).view(np.uint64)), (what, i, T_b - T_s)
        assert np.float32(err_b).view(np.uint32) == np.float32(err_s).view(np.uint32), (what, i, err_b, err_s)


def assert_matches_oracle(entries, res, tag):
    seen = {True: 0, False: 0}
    for i, ((sc, xyz, cols, g, _), (ok, T, err, inl)) in enumerate(zip(entries, res)):
        ok_o, T_o, err_o, inl_o = oracle_result(sc, xyz, cols, g, (tag, id(sc), len(xyz), g))
        print(f"{tag} job {i} guess {g}: ok {ok}/{ok_o} inliers {inl}/{inl_o} err {err:.6f}/{err_o:.6f} max |dT| {np.abs(T - T_o).max():.2e}")
        assert ok == bool(ok_o) and inl == inl_o
        np.testing.assert_allclose(T, T_o, atol=1e-4)
        assert abs(err - err_o) <= 1e-4 * err_o
        seen[ok] += 1
    return seen


# ---- CPU: the wrapper's own checks, before any library call ----
def test_wrapper_rejects_malformed_job_lists():
    from direct_stereo_slam_amd.tracker import PoseBatch

    w, h, nl, n = 64, 32, 2, 10
    pyr = [np.zeros((h >> l, w >> l, 3), np.float32) for l in range(nl)]
    planes = [np.zeros((h >> l, w >> l), np.float32) for l in range(nl)]

    def job(**kw):
        j = dict(pts_xyz=np.ones((n, 3)), ref_colors=[np.zeros(n, np.float32)] * nl, ref_ab_exposure=1.0, new_ab_exposure=1.0,
                 new_cam=(50.0, 50.0, 32.0, 16.0), ref_to_new=np.eye(4), new_dIp=pyr)
        j.update(kw)
        return j

    assert len(PoseBatch.check_jobs([job(), job(new_dIp=None, new_I=planes)], w, h, nl)) == 2
    bad = {
        "ragged colours": job(ref_colors=[np.zeros(n, np.float32), np.zeros(n - 1, np.float32)]),
        "a colour list short of levels": job(ref_colors=[np.zeros(n, np.float32)]),
        "both target forms": job(new_I=planes),
        "neither target form": job(new_dIp=None),
        "no points": job(pts_xyz=np.zeros((0, 3)), ref_colors=[np.zeros(0, np.float32)] * nl),
        "more points than pixels": job(pts_xyz=np.ones((w * h + 1, 3)), ref_colors=[np.zeros(w * h + 1, np.float32)] * nl),
        "a pyramid of another geometry": job(new_dIp=pyr[:1] + [np.zeros((3, 3, 3), np.float32)]),
        "a 3 x 4 guess": job(ref_to_new=np.eye(4)[:3]),
    }
    for what, j in bad.items():
        with pytest.raises(ValueError):
            PoseBatch.check_jobs([job(), j], w, h, nl)
        assert what
    with pytest.raises(ValueError):
        PoseBatch.check_jobs([], w, h, nl)
    missing = job()
    del missing["new_cam"]
    with pytest.raises(ValueError):
        PoseBatch.check_jobs([missing], w, h, nl)


OTHER_GEOMETRIES = [("medium", 73, 4000, 0.01, 2.0, GUESSES), ("tiny", 76, 4000, 0.02, 3.0, ("identity", "gt"))]


def test_chosen_jobs_are_well_conditioned_in_the_oracle():
    """The device is compared with the oracle at 1e-4; that only means something for jobs whose oracle result does not itself move by
    as much when its sums run in another order (tests/_pose_jobs.py: SMALL_AB).  Every job of the GPU tests: below 2e-5 (a fifth of the tolerance), and the same
    verdict and inlier percentage, across four point orders."""
    entries = small_jobs()
    for size, seed, n, a, b, guesses in OTHER_GEOMETRIES:
        entries += geometry_jobs(size, seed, n, a, b, guesses)
    for sc, xyz, cols, g, _ in entries:
        dT, de, verdicts = oracle_order_spread(sc, xyz, cols, g)
        print(f"{sc.w}x{sc.h} n {len(xyz)} guess {g}: spread |dT| {dT:.2e} rel. d err {de:.2e} {verdicts[0]}")
        assert len(set(verdicts)) == 1 and verdicts[0][0] == (g != "far"), (sc.w, len(xyz), g, verdicts)
        if sc.w == 616 and g == "far":
            # the one case that is not chosen here (it is the existing medium job, rejected from the hopeless guess): under each of the
            # four (a, b) its oracle result moves by 1.6e-3 .. 4.2e-2 across point orders (4.2e-2 / 5.5e-3 relative in the error with
            # this one); only its verdict and inlier percentage are stable
            continue
        assert dT < 2e-5 and de < 2e-5, (sc.w, len(xyz), g, dT, de)


# ---- GPU ----
@pytest.mark.gpu
def test_batch_of_21_matches_the_oracle(ctx):
    """the seven small jobs, each from the identity, the ground truth and the hopeless guess: accepted and rejected jobs in one call"""
    entries = small_jobs()
    assert len(entries) == 21
    res = batch_results(ctx, entries)
    seen = assert_matches_oracle(entries, res, "small")
    assert seen[True] == 14 and seen[False] == 7  # every job from identity / ground truth accepted, every far guess rejected
    for (_, _, _, g, _), (ok, _, err, inl) in zip(entries, res):
        assert ok == (g != "far")


@pytest.mark.gpu
@pytest.mark.parametrize("size,seed,n,a,b,guesses", OTHER_GEOMETRIES)
def test_other_geometries_match_the_oracle(ctx, size, seed, n, a, b, guesses):
    """616x184 with 4 levels, and 154x46 with more points than the coarse level has pixels: each a call of its own"""
    entries = geometry_jobs(size, seed, n, a, b, guesses)
    sc = entries[0][0]
    if size == "tiny":
        assert n > (sc.w >> 1) * (sc.h >> 1)
    res = batch_results(ctx, entries)
    seen = assert_matches_oracle(entries, res, size)
    if size == "medium":
        assert seen[True] == 2 and seen[False] == 1
    assert_same_bits(res, single_results(ctx, entries), size)


@pytest.mark.gpu
def test_every_job_equals_the_single_call_bit_for_bit(ctx):
    from direct_stereo_slam_amd.tracker import PoseBatch

    entries = small_jobs()
    single = single_results(ctx, entries)
    sc = entries[0][0]
    pb = PoseBatch(ctx, sc.w, sc.h, sc.nl)
    for i, e in enumerate(entries):  # batches of one, through one handle whose arenas are reused
        assert_same_bits(pb.estimate_many([e[4]], sc.nl - 1), [single[i]], f"batch of one, job {i}")
    assert_same_bits(pb.estimate_many([e[4] for e in entries], sc.nl - 1), single, "batch of 21")
    assert_same_bits(pb.estimate_many([e[4] for e in entries[::-1]], sc.nl - 1), single[::-1], "batch of 21, reversed")
    # 64 jobs: the list repeated with other guesses (the ground truth moved by k cm), so that the default work_queue rule (n >= 32)
    # takes the queue form
    many = list(entries)
    k = 1
    while len(many) < 64:
        scn, xyz, cols, _, _ = entries[(3 * k) % 21]
        many.append((scn, xyz, cols, ("near", k), make_job(scn, xyz, cols, ("near", k))))
        k += 1
    res = pb.estimate_many([e[4] for e in many], sc.nl - 1)
    assert ctx.stats().queue_blocks > 0  # the queue form ran
    assert_same_bits(res, single_results(ctx, many), "batch of 64")
    pb.close()


FORMS = {
    "launch per step": dict(work_queue=0),
    "work queue": dict(work_queue=2),
    "chain prefix": dict(work_queue=0, persistent_coarse=-1),
    "no speculation": dict(work_queue=0, speculate=0),
    "speculation on every level": dict(work_queue=0, speculate=2),
    "queue without speculation": dict(work_queue=2, speculate=0),
}


@pytest.mark.gpu
@pytest.mark.parametrize("geometry", [0, 1, 2])
def test_schedule_forms_give_identical_bits(ctx, geometry):
    """per chunk table (another table is another summation tree): every scheduling form of the 21-job batch returns the bits of the
    single call under that table"""
    entries = small_jobs()
    single = single_results(ctx, entries, params_with(chunk_geometry=geometry), key=("geometry", geometry))
    for name, kw in FORMS.items():
        res = batch_results(ctx, entries, params_with(chunk_geometry=geometry, **kw))
        st = ctx.stats()
        if kw.get("work_queue") == 2:
            assert st.queue_blocks > 0, name
        if kw.get("persistent_coarse", 0) < 0:  # (under the latency table the 40-point job alone is one chunk: still a chain launch)
            assert st.coarse_launches == 1, name
        assert_same_bits(res, single, f"table {geometry}, {name}")


@pytest.mark.gpu
def test_intensity_planes_give_the_bits_of_the_texel_pyramid(ctx):
    entries = small_jobs()
    res_dip = batch_results(ctx, entries)
    res_i = batch_results(ctx, small_jobs(planes=True))
    assert_same_bits(res_i, [r[:3] for r in res_dip], "new_I against new_dIp")
    assert [r[3] for r in res_i] == [r[3] for r in res_dip]
    # both forms in one call
    mixed = [e if i % 2 else p for i, (e, p) in enumerate(zip(entries, small_jobs(planes=True)))]
    assert_same_bits(batch_results(ctx, mixed), [r[:3] for r in res_dip], "mixed target forms")


@pytest.mark.gpu
def test_page_locked_job_arrays_give_the_same_bits(ctx):
    """points and colours in dsm_host_alloc memory are read in place by the pack kernel, the others are staged: same results, also mixed
    in one call"""
    from direct_stereo_slam_amd.tracker import pinned_array

    entries = small_jobs()
    pinned = []
    for i, (sc, xyz, cols, g, job) in enumerate(entries):
        if i % 3 == 1:  # every third job stays pageable
            pinned.append((sc, xyz, cols, g, job))
            continue
        px = pinned_array(xyz.shape, np.float64)
        px[:] = xyz
        pc = []
        for c in cols:
            a = pinned_array(c.shape, np.float32)
            a[:] = c
            pc.append(a)
        pinned.append((sc, xyz, cols, g, dict(job, pts_xyz=px, ref_colors=pc)))
    assert_same_bits(batch_results(ctx, pinned), single_results(ctx, entries), "page-locked points and colours")


def _raw_call(ctx, entries, mutate=None, coarsest=None, n_jobs=None, params=None):
    """the C call itself on sentinel-filled outputs: (rc, message, outputs untouched?)"""
    from direct_stereo_slam_amd import _lib
    from direct_stereo_slam_amd.tracker import PoseBatch

    sc = entries[0][0]
    pb = PoseBatch(ctx, sc.w, sc.h, sc.nl, params)
    arr, (T, err, inl, ok), keep = PoseBatch.build_jobs(PoseBatch.check_jobs([e[4] for e in entries], sc.w, sc.h, sc.nl))
    err[:], inl[:], ok[:] = -77.0, -77, -77
    extra = mutate(arr, T) if mutate else None
    T0 = T.copy()
    rc = ctx.L.dsm_pose_estimate_batch(pb.h_, len(arr) if n_jobs is None else n_jobs, arr, sc.nl - 1 if coarsest is None else coarsest)
    msg = _lib.load().dsm_last_error().decode()
    untouched = (np.array_equal(T.view(np.uint64), T0.view(np.uint64)) and (err == -77.0).all() and (inl == -77).all() and (ok == -77).all())
    pb.close()
    del keep, extra
    return rc, msg, untouched


@pytest.mark.gpu
def test_invalid_arguments_fail_the_whole_call_and_write_nothing(ctx):
    from direct_stereo_slam_amd import _lib

    entries = small_jobs(guesses=("identity",))[:4]
    sc = entries[0][0]
    rc, _, untouched = _raw_call(ctx, entries)
    assert rc == 0 and not untouched  # the unmutated call succeeds and writes
    null_f = C.POINTER(_lib.c_float_p)()

    def null_level(field):
        def m(arr, T):
            tab = (_lib.c_float_p * sc.nl)(*[getattr(arr[1], field)[l] for l in range(sc.nl)])
            tab[sc.nl - 1] = _lib.c_float_p()
            setattr(arr[1], field, tab)
            return tab
        return m

    def both(arr, T):
        arr[3].new_I = arr[3].new_dIp

    def nan_guess(arr, T):
        T[2, 7] = np.nan

    def inf_guess(arr, T):
        T[0, 0] = np.inf

    cases = {
        "NULL xyz": lambda arr, T: setattr(arr[2], "xyz", _lib.c_double_p()),
        "NULL ref_colors": lambda arr, T: setattr(arr[0], "ref_colors", null_f),
        "NULL ref_to_new_io": lambda arr, T: setattr(arr[3], "ref_to_new_io", _lib.c_double_p()),
        "NULL ok": lambda arr, T: setattr(arr[1], "ok", _lib.c_int_p()),
        "n_pts 0": lambda arr, T: setattr(arr[2], "n_pts", 0),
        "n_pts -5": lambda arr, T: setattr(arr[0], "n_pts", -5),
        "n_pts > w*h": lambda arr, T: setattr(arr[3], "n_pts", sc.w * sc.h + 1),
        "both targets": both,
        "neither target": lambda arr, T: setattr(arr[2], "new_dIp", null_f),
        "NULL colour level": null_level("ref_colors"),
        "NULL target level": null_level("new_dIp"),
        "NaN guess": nan_guess,
        "infinite guess": inf_guess,
    }
    for what, m in cases.items():
        rc, msg, untouched = _raw_call(ctx, entries, mutate=m)
        assert rc == INVALID and untouched, (what, rc, msg)
        assert "job" in msg, (what, msg)
    for what, kw in {"coarsest_lvl -1": dict(coarsest=-1), "coarsest_lvl = nlevels": dict(coarsest=sc.nl), "n_jobs 0": dict(n_jobs=0),
                     "n_jobs -1": dict(n_jobs=-1)}.items():
        rc, msg, untouched = _raw_call(ctx, entries, **kw)
        assert rc == INVALID and untouched, (what, rc, msg)
    from direct_stereo_slam_amd.tracker import PoseBatch
    pb = PoseBatch(ctx, sc.w, sc.h, sc.nl)
    assert ctx.L.dsm_pose_estimate_batch(pb.h_, 1, None, 0) == INVALID and ctx.L.dsm_pose_estimate_batch(None, 1, None, 0) == INVALID
    out = C.c_void_p()
    assert ctx.L.dsm_pose_batch_create(ctx.h, sc.w, sc.h, 0, None, C.byref(out)) == INVALID and not out.value
    assert ctx.L.dsm_pose_batch_create(ctx.h, sc.w, sc.h, sc.nl, None, None) == INVALID
    pb.close()
    # ... and the handle-free checks did not disturb the next valid call
    assert_same_bits(batch_results(ctx, entries), single_results(ctx, entries), "after the failed calls")


@pytest.mark.gpu
@pytest.mark.parametrize("k", [0, 2])
def test_a_corrupted_gradient_texel_fails_the_whole_call(ctx, k):
    """job k's pyramid carries one gradient value makeImages would not have produced: the call fails as dsm_tracker_upload_frame does,
    naming job, level and texel, and no job's outputs are written; with the check off the same call goes through"""
    base = small_jobs(guesses=("identity",))[:4]
    sc, xyz, cols, g, _ = base[k]
    lvl, x, y = 1, 17, 9
    broken = [p.copy() for p in sc.new_p]
    broken[lvl][y, x, 2] += 0.25
    job = make_job(sc, xyz, cols, g)
    job["new_dIp"] = broken
    entries = list(base)
    entries[k] = (sc, xyz, cols, g, job)
    rc, msg, untouched = _raw_call(ctx, entries)
    assert rc == INVALID and untouched, (rc, msg)
    assert f"job {k}:" in msg and f"level {lvl}:" in msg and f"(x = {x}, y = {y})" in msg and "1 texel(s)" in msg, msg
    rc, msg, untouched = _raw_call(ctx, entries, params=params_with(frame_check=0))
    assert rc == 0 and not untouched, msg
    # the device keeps channel 0 only: with the check off the corrupted gradient changes nothing
    assert_same_bits(batch_results(ctx, entries, params_with(frame_check=0)), single_results(ctx, base), "check off")


@pytest.mark.gpu
def test_device_memory_follows_the_points(ctx):
    """64 jobs of 2000 points at 1232x368x5, each with a target pyramid of its own: the batch handle and its call grow device memory by
    less than 64 single estimator handles would, and a second identical call by nothing.  Figures: DESIGN.md section 11."""
    import torch

    from direct_stereo_slam_amd.tracker import PoseBatch, PoseEstimator

    def free():
        ctx.sync()
        return torch.cuda.mem_get_info()[0]

    sc, xyz, cols = scene_inputs("kitti", 81, 2000, 0.01, 2.0)
    args = (xyz, cols, 1.0, sc.new_p, 1.0, sc.K, sc.nl - 1, np.eye(4))
    warm = PoseEstimator(ctx, sc.w, sc.h, sc.nl)  # grows the context's own staging and batch workspaces, which are not a handle's
    ok_s, T_s, err_s = warm.estimate(*args)
    warm.close()
    f0 = free()
    one = PoseEstimator(ctx, sc.w, sc.h, sc.nl)
    one.estimate(*args)
    single_bytes = f0 - free()
    one.close()
    jobs = []
    for i in range(64):
        j = make_job(sc, xyz, cols, "identity")
        j["new_dIp"] = [p.copy() for p in sc.new_p]  # a pyramid of its own: nothing shared between the jobs
        jobs.append(j)
    f1 = free()
    pb = PoseBatch(ctx, sc.w, sc.h, sc.nl)
    res = pb.estimate_many(jobs, sc.nl - 1)
    f2 = free()
    batch_bytes = f1 - f2
    print(f"device memory: one single handle {single_bytes / 2**20:.1f} MiB (x 64 = {64 * single_bytes / 2**20:.1f} MiB), "
          f"batch handle + 64 jobs {batch_bytes / 2**20:.1f} MiB")
    res2 = pb.estimate_many(jobs, sc.nl - 1)
    f3 = free()
    pb.close()
    assert single_bytes > 0 and batch_bytes > 0
    assert batch_bytes < 64 * single_bytes
    # templates scale with the points: 16 B x (2000 + slack) x 5 levels x 64 jobs is 15 MiB; with the planes (2.3 MiB per job), the
    # staging of 8 pyramids (6.9 MiB each), the staged inputs (6 MiB) and the LM workspaces (4 MiB) that is about 230 MiB, where ONE
    # single handle holds 35 MiB of templates alone: a quarter of 64 handles (at least 560 MiB) leaves a factor of two
    assert batch_bytes < 64 * single_bytes / 4
    assert f3 == f2, (f2, f3)
    assert_same_bits(res, [(ok_s, T_s, err_s)] * 64, "64 KITTI jobs")
    assert_same_bits(res2, [(ok_s, T_s, err_s)] * 64, "64 KITTI jobs, second call")
