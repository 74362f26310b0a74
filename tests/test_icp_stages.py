"""GPU: the ICP fallback stage by stage.  dsm_diag_icp_stages runs dsm_icp_batch's own launch sequence, stops after a stage and copies
out what the device holds; each stage is then held on its own (helpers and scenes: tests/_icp_stage_checks.py, which
tests/test_icp_stage_bars.py shows to reject the mistakes such kernels make):
  prep     bit for bit the checker's double evaluation (P1);
  search   every source point's target index and distance bits equal the checker's (P2, D2, D5), under forced target slices;
  step     from the device's own cloud and keys: counts, moved cloud, keys, final and end state exact, the increment within half a float
           ulp + DELTA of the exact step, the MSE within its rounding bound of the exact mean (P3-P6, D1, D4);
  fitness  the cloud is the original moved by final, the score the exact mean within the same bound (P9, D4);
and the whole sequence under the production slice rule equals what dsm_icp_batch returns, bit for bit."""
import numpy as np
import pytest

import _icp_ref as R
import _icp_stage_checks as K
from direct_stereo_slam_amd import icp as I
from direct_stereo_slam_amd._lib import DsmError

pytestmark = pytest.mark.gpu
FIGURES = {}  # worst err / bound per kind, printed by the tests that fill it (DESIGN.md section 10 quotes them)


def stages(ctx, jobs, stage, iteration=0, want=0, **params):
    with np.errstate(invalid="ignore"):
        return I.icp_stages(ctx, jobs, stage, iteration, want, **params)


def searched(ctx, src, tgt, want=0, guess=K.IDENTITY):
    return stages(ctx, [(src, tgt, guess)], I.STAGE_SEARCH, 0, want)[0]


def test_prep_equals_the_double_evaluation(ctx):
    rng = np.random.default_rng(5)
    guess = R.rigid(R.rot((0.3, -0.2, 0.5)), [1.25, -3.5, 0.75])
    src, tgt = rng.normal(0, 7, (257, 3)), rng.normal(0, 7, (300, 3))
    as_float = R.transform_float(guess.astype(np.float32), src.astype(np.float32))
    assert (as_float != R.transform_double(src, guess)).any()  # the test can tell a float evaluation from P1's
    jobs = [(src, tgt, guess), (src[:0], tgt, guess), (src[:5], tgt[:0], guess), (tgt, src, np.linalg.inv(guess))]
    got = stages(ctx, jobs, I.STAGE_PREP)
    for (s, t, g), out in zip(jobs, got):
        K.check_prep(s, t, g, out)
    assert [int(o["state"]["state"]) for o in got] == [0, R.EMPTY, R.EMPTY, 0]


@pytest.mark.parametrize("n_tgt", K.SEAM_N_TGT)
def test_search_seam_sweep(ctx, n_tgt):
    """every source's neighbour planted at a tile or slice seam, at distance 0, tiny and about 1 m; one call per slice count, its jobs
    the source sizes with the seams in turn and 600 sources on each single seam"""
    for want in K.SLICE_COUNTS:
        per, cases = K.seam_jobs(n_tgt, want)
        got = stages(ctx, [(s, t, K.IDENTITY) for s, t, _ in cases], I.STAGE_SEARCH, 0, K.want_slices(n_tgt, want))
        for (s, t, planted), out in zip(cases, got):
            assert out["work"][:, :3].tobytes() == s.astype(np.float32).tobytes()
            K.check_search(out["work"], out["target"], out["keys"], planted)


def test_search_exact_ties_go_to_the_smallest_index_under_every_slice_count(ctx):
    for want in K.SLICE_COUNTS:
        src, tgt, planted = K.tie_case(1300, K.slice_len(1300, want))
        out = searched(ctx, src, tgt, K.want_slices(1300, want))
        idx, d = K.check_search(out["work"], out["target"], out["keys"], planted)
        assert sorted(set(d.tolist())) == [0.25, 1.25, 6.5]  # exact in float: every target of a group at the same distance


@pytest.mark.parametrize("shift", [0.0, 1000.0])
def test_search_dense_scene(ctx, shift):
    """a street scene; shifted by 1000 m the float cancellation of source - target decides the neighbours, and the checker says how"""
    src, tgt = K.dense_case(shift)
    plain = R.nearest(*(p.astype(np.float32) for p in K.dense_case(0.0)))[0]
    for want in K.SLICE_COUNTS:
        out = searched(ctx, src, tgt, K.want_slices(1300, want))
        idx, _ = K.check_search(out["work"], out["target"], out["keys"])
        assert (idx != plain).any() == bool(shift)  # the shift does change neighbours: this case is not the plain one again


def test_search_nonfinite_rows_follow_d5(ctx):
    for name, (src, tgt) in K.nonfinite_cases().items():
        for want in (1, 2, "tile"):
            out = searched(ctx, src, tgt, K.want_slices(len(tgt), want))
            idx, _ = K.check_search(out["work"], out["target"], out["keys"])
            if name in ("overflow", "target_all_nonfinite"):
                assert np.all(out["keys"] == K.NO_KEY), name
            assert np.all(idx[~np.isfinite(out["work"][:, :3]).all(1)] == -1), name
            assert np.isfinite(out["target"][idx[idx >= 0], :3]).all(), name


def test_nonfinite_points_are_never_pairs_and_make_the_score_nan(ctx):
    src, tgt = K.nonfinite_cases()["source_rows"]
    jobs = [(src, tgt, K.IDENTITY)]
    before, after = stages(ctx, jobs, I.STAGE_SEARCH, max_iterations=2)[0], stages(ctx, jobs, I.STAGE_STEP, max_iterations=2)[0]
    K.check_step(before, after, 2, I.TRANSFORMATION_EPSILON)
    assert after["state"]["corr"][0] <= len(src) - 5
    got = I.icp(ctx, src, tgt, K.IDENTITY)
    with np.errstate(invalid="ignore"):
        want = R.icp(src, tgt, K.IDENTITY)
    assert np.isnan(got["score"]) and not got["ok"] and np.isnan(want["score"]) and not want["ok"]
    assert (got["state"], got["iterations"], got["corr_counts"]) == (want["state"], want["iterations"], want["corr_counts"])


def test_search_three_job_batch_with_an_empty_middle_job(ctx):
    a, b = R.scene(62, 300, n_tgt=700), R.scene(63, 520, n_tgt=513)
    jobs = [(a[0], a[1], K.IDENTITY), (a[0][:0], a[1][:9], K.IDENTITY), (b[0], b[1], K.IDENTITY)]
    for want in (0, 2, 3):
        got = stages(ctx, jobs, I.STAGE_SEARCH, 0, want)
        for j in (0, 2):
            K.check_search(got[j]["work"], got[j]["target"], got[j]["keys"])
        assert got[1]["state"]["state"] == R.EMPTY and len(got[1]["keys"]) == 0 and len(got[1]["target"]) == 9


def test_search_of_the_second_iteration_reads_the_moved_cloud(ctx):
    src, tgt, _ = R.blobs(3, 2000, (0, 0.1, 0), (1.5, 0.5, 0))
    out = stages(ctx, [(src, tgt, K.IDENTITY)], I.STAGE_SEARCH, 1, 3)[0]
    assert out["state"]["iterations"] == 1 and out["work"].tobytes() != out["orig"].tobytes()
    K.check_search(out["work"], out["target"], out["keys"])


def test_fitness_search_has_no_distance_limit(ctx):
    pts = np.random.default_rng(1).normal(0, 3, (500, 3))
    out = stages(ctx, [(pts, pts + np.array([50.0, 0.0, 0.0]), K.IDENTITY)], I.STAGE_FITNESS_SEARCH)[0]
    idx, d = K.check_search(out["work"], out["target"], out["keys"])
    assert out["state"]["state"] == R.NO_CORRESPONDENCES and np.all(idx >= 0) and d.min() > 30.0 ** 2


@pytest.mark.parametrize("name", list(K.step_scenes()))
def test_step_alone(ctx, name):
    """the step from the device's own cloud and keys; epsilon < 0 and two iterations, so that the state stays "running" and the MSE
    is kept where the test can read it"""
    src, tgt, guess, full_rank = K.step_scenes()[name]
    jobs, params = [(src, tgt, guess)], dict(max_iterations=2, transformation_epsilon=-1.0)
    before, after = stages(ctx, jobs, I.STAGE_SEARCH, **params)[0], stages(ctx, jobs, I.STAGE_STEP, **params)[0]
    fig = {}
    K.check_step(before, after, 2, -1.0, full_rank=full_rank, figures=fig)
    assert after["state"]["state"] == K.RUNNING and after["state"]["corr"][0] >= 3
    if name == "half_without_pairs":
        assert after["state"]["corr"][0] <= len(src) // 2
    print(name, "kept", int(after["state"]["corr"][0]), "worst err / bound:", fig)
    for k, v in fig.items():
        FIGURES[k] = max(FIGURES.get(k, 0.0), v)
    print("so far:", FIGURES)


def test_step_edges_threshold_and_pair_count(ctx):
    edges = K.edge_jobs()
    jobs, params = [(s, t, K.IDENTITY) for s, t in edges.values()], dict(max_iterations=2, transformation_epsilon=-1.0)
    before, after = stages(ctx, jobs, I.STAGE_SEARCH, **params), stages(ctx, jobs, I.STAGE_STEP, **params)
    kept = {"at_threshold": 3, "above_threshold": 0, "two_pairs": 2, "three_pairs": 3, "three_kept_of_four": 3}
    for name, b, a in zip(edges, before, after):
        K.check_step(b, a, 2, -1.0, full_rank=False)
        S = a["state"]
        assert S["corr"][0] == kept[name], name
        if kept[name] < 3:  # P3: nothing moved, final is the identity, one search and no iteration
            assert (S["state"], S["searches"], S["iterations"]) == (R.NO_CORRESPONDENCES, 1, 0), name
            assert S["final_tf"].tobytes() == np.eye(4, dtype=np.float32).tobytes() and a["work"].tobytes() == a["orig"].tobytes(), name
        else:
            assert (S["state"], S["searches"], S["iterations"]) == (K.RUNNING, 1, 1), name
    _, d = K.unpack_keys(before[0]["keys"])
    assert np.all(d == np.float32(4.0))
    _, d = K.unpack_keys(before[1]["keys"])
    assert np.all(d == np.nextafter(np.float32(4.0), np.float32(5.0)))


def test_p6_tests_the_iteration_limit_before_the_transform(ctx):
    src, tgt, _ = R.scene(1, 2000)
    jobs = [(src, tgt, K.IDENTITY)]
    for max_iterations, want in ((1, R.ITERATIONS), (2, R.TRANSFORM)):
        before = stages(ctx, jobs, I.STAGE_SEARCH, max_iterations=max_iterations)[0]
        after = stages(ctx, jobs, I.STAGE_STEP, max_iterations=max_iterations)[0]
        inc = K.check_step(before, after, max_iterations, I.TRANSFORMATION_EPSILON)
        assert K.expected_end_state(inc, 0.0, 1.0, 1, 2, I.TRANSFORMATION_EPSILON) == R.TRANSFORM  # the transform test holds
        assert after["state"]["state"] == want
    src, tgt, _ = R.blobs(3, 2000, (0, 0.1, 0), (1.5, 0.5, 0))
    jobs = [(src, tgt, K.IDENTITY)]
    before, after = stages(ctx, jobs, I.STAGE_SEARCH)[0], stages(ctx, jobs, I.STAGE_STEP)[0]
    K.check_step(before, after, I.MAX_ITERATIONS, I.TRANSFORMATION_EPSILON)
    assert after["state"]["state"] == K.RUNNING and after["state"]["prev_mse"] < 4.0  # the MSE itself: check_step bounds it


def test_fitness_is_taken_on_the_original_cloud_moved_by_final(ctx):
    src, tgt, _ = R.blobs(3, 2000, (0, 0.1, 0), (1.5, 0.5, 0))
    trace = []
    R.icp(src, tgt, K.IDENTITY, max_iterations=2, trace=trace)
    assert R.transform_float(trace[1]["final"], R.transform_double(src, K.IDENTITY)).tobytes() != trace[1]["work"].tobytes()
    jobs, params = [(src, tgt, K.IDENTITY)], dict(max_iterations=2)
    iterated = stages(ctx, jobs, I.STAGE_STEP, 1, **params)[0]
    prepared = stages(ctx, jobs, I.STAGE_FITNESS_PREP, **params)[0]
    assert iterated["state"]["state"] == R.ITERATIONS and iterated["state"]["iterations"] == 2
    K.check_fitness_prep(iterated, prepared)
    assert prepared["work"].tobytes() != iterated["work"].tobytes()
    fit_searched = stages(ctx, jobs, I.STAGE_FITNESS_SEARCH, **params)[0]
    assert fit_searched["work"].tobytes() == prepared["work"].tobytes()
    K.check_search(fit_searched["work"], fit_searched["target"], fit_searched["keys"])
    done = stages(ctx, jobs, I.STAGE_FITNESS, **params)[0]
    K.check_fitness(fit_searched, done, FIGURES)
    assert np.array_equal(done["keys"], fit_searched["keys"])
    print("worst err / bound:", FIGURES)
    got = I.icp(ctx, src, tgt, K.IDENTITY, max_iterations=2)
    assert got["score"].tobytes() == np.float32(done["state"]["fitness"]).tobytes()


@pytest.mark.parametrize("scene", ["small_motion_with_guess", "large_motion", "far_apart"])
def test_whole_sequence_under_the_production_rule_is_dsm_icp_batch(ctx, scene):
    guess = R.rigid(R.rot((0.0, 0.01, 0.0)), [0.05, 0.0, 0.0])
    pts = np.random.default_rng(1).normal(0, 3, (500, 3))
    src, tgt, guess = {"small_motion_with_guess": R.scene(1, 2000)[:2] + (guess,),
                       "large_motion": R.blobs(3, 2000, (0, 0.1, 0), (1.5, 0.5, 0))[:2] + (K.IDENTITY,),
                       "far_apart": (pts, pts + np.array([20.0, 0.0, 3.0]), guess)}[scene]
    S = stages(ctx, [(src, tgt, guess)], I.STAGE_FITNESS)[0]["state"]
    got = I.icp(ctx, src, tgt, guess)
    Fd, tfm = S["final_tf"].astype(np.float64), np.empty((4, 4))
    for r in range(4):  # P8
        for c in range(4):
            tfm[r, c] = ((Fd[r, 0] * guess[0, c] + Fd[r, 1] * guess[1, c]) + Fd[r, 2] * guess[2, c]) + Fd[r, 3] * guess[3, c]
    assert got["tfm"].tobytes() == tfm.tobytes() and got["score"].tobytes() == np.float32(S["fitness"]).tobytes()
    assert (got["state"], got["iterations"]) == (S["state"], S["iterations"])
    assert got["corr_counts"] == S["corr"][:S["searches"]].tolist() and np.all(S["corr"][S["searches"]:] == -1)
    K.check_fitness(stages(ctx, [(src, tgt, guess)], I.STAGE_FITNESS_SEARCH)[0], dict(state=S), FIGURES)


def test_diag_refuses_what_it_cannot_run(ctx):
    pts = np.random.default_rng(2).normal(0, 3, (30, 3))
    jobs = [(pts, pts + 0.1, K.IDENTITY)]
    bad_guess = np.eye(4)
    bad_guess[1, 3] = np.inf
    for kwargs in (dict(stage=6), dict(stage=-1), dict(stage=I.STAGE_SEARCH, iteration=5), dict(stage=I.STAGE_STEP, iteration=-1),
                   dict(stage=I.STAGE_PREP, want=-1), dict(stage=I.STAGE_PREP, max_iterations=65), dict(stage=I.STAGE_PREP, max_corr_dist=-1.0)):
        with pytest.raises(DsmError, match="dsm_diag_icp_stages"):
            stages(ctx, jobs, **kwargs)
    with pytest.raises(DsmError, match="non-finite guess"):
        stages(ctx, [(pts, pts, bad_guess)], I.STAGE_PREP)
    K.check_prep(*jobs[0], stages(ctx, jobs, I.STAGE_PREP)[0])  # and the context still serves
