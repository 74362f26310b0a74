"""The bench line the driver parses: flags, metric string, and (on a GPU) every key of the contract."""
import importlib.util
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_metric_is_baseline_jsons_and_defaults_are_the_contracts(monkeypatch):
    m = _bench()
    assert m.baseline_metric() == json.load(open(os.path.join(ROOT, "BASELINE.json")))["metric"]
    monkeypatch.setattr(sys, "argv", ["bench.py"])
    a = m.parse()
    assert a.gpus == 1 and a.steps >= 1 and a.warmup >= 1 and not a.with_upload
    # the default line runs what ships (dsm_params_default: no scheduling switch is overridden) on all-distinct frames
    assert a.queue is None and a.coarse is None and a.fuse is None and a.speculate is None and a.scenes is None and a.fixed_schedule == 0
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "7", "--warmup", "3"])
    a = m.parse()
    assert (a.gpus, a.steps, a.warmup) == (4, 7, 3)


def test_a_plain_run_is_the_headline_alone_and_full_restores_the_rest(monkeypatch):
    """without --full: no CPU baseline, no extra leg, no side file; --full runs them all (--quick keeps its meaning under it)"""
    m = _bench()
    legs = ("no_cpu", "no_fixed_leg", "no_second_leg", "no_plane_leg", "no_upload_leg", "no_replay_leg", "no_ringkey_leg")
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "5", "--warmup", "2"])
    a = m.parse()
    assert not a.full and all(getattr(a, k) for k in legs) and a.detail_out is None and a.dump_outputs is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full"])
    a = m.parse()
    assert a.full and not any(getattr(a, k) for k in legs) and a.detail_out == m.DETAIL_OUT
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--quick"])
    a = m.parse()
    assert a.full and all(getattr(a, k) for k in legs)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--dump-outputs", "out_dir"])
    assert m.parse().dump_outputs == "out_dir"


def test_dump_outputs_writes_float_arrays_within_the_size_bound(tmp_path):
    import numpy as np

    m = _bench()
    outs = {"track_pose": np.arange(70, dtype=np.float64).reshape(10, 7), "track_good": np.ones(10, bool), "scale": np.ones(2, np.float32)}
    m.dump_outputs(outs, str(tmp_path / "a"))
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert set(got) == set(outs) and all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert np.array_equal(got["track_pose"], outs["track_pose"]) and got["track_good"].dtype == np.float64 and got["scale"].dtype == np.float32
    # above the bound: the same seeded sample of rows every time, with the row numbers beside it
    big = {"track_pose": np.arange(7000, dtype=np.float64).reshape(1000, 7)}
    for d in ("b", "c"):
        m.dump_outputs(big, str(tmp_path / d), limit=8 * 7 * 100)
    rows = np.load(tmp_path / "b" / "track_pose_rows.npy").astype(int)
    sample = np.load(tmp_path / "b" / "track_pose.npy")
    assert sample.nbytes <= 8 * 7 * 100 and np.array_equal(sample, big["track_pose"][rows])
    assert np.array_equal(sample, np.load(tmp_path / "c" / "track_pose.npy"))
    # the bound holds for everything written, the row numbers and the .npy headers included
    assert sum(os.path.getsize(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b")) <= 8 * 7 * 100


def test_frames_rendered_on_threads_equal_the_forked_ones(monkeypatch):
    """build_frames forks its rendering processes only while no device is open in the process; once one is, it renders on
    threads and never forks -- the same images either way"""
    import multiprocessing

    import numpy as np

    m = _bench()
    from direct_stereo_slam_amd import synth as S

    w, h, K = 312, 96, (179.7, 179.7, 152.6, 47.3)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--batch", "24", "--u8"])
    a = m.parse()
    monkeypatch.setattr(m, "_device_open", lambda: False)
    tex_f, fr_f = m.build_frames(a, w, h, K, S.KITTI_T_STEREO)
    m._FRAMES.clear()

    def no_fork(*args, **kw):
        raise AssertionError("build_frames forked with a device open")

    monkeypatch.setattr(m, "_device_open", lambda: True)
    monkeypatch.setattr(multiprocessing, "get_context", no_fork)
    tex_t, fr_t = m.build_frames(a, w, h, K, S.KITTI_T_STEREO)
    m._FRAMES.clear()
    assert len(fr_t) == len(fr_f) == 24
    for (_, r1, q1), (_, r2, q2) in zip(tex_f, tex_t):
        assert np.array_equal(r1, r2) and np.array_equal(q1, q2)
    for f1, f2 in zip(fr_f, fr_t):
        assert f1[0] == f2[0] and all(np.array_equal(x, y) for x, y in zip(f1[1:], f2[1:]))


def test_gpus_flag_is_honoured_or_fails_loudly():
    """`--gpus N` without a launcher spawns N ranks itself; a mismatching launcher or too few devices is an error, never a
    silent 1-GPU run labelled otherwise"""
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4"], capture_output=True, text=True, env=env, cwd=ROOT)
    assert out.returncode == 2 and "WORLD_SIZE=2" in out.stderr
    import torch

    if torch.cuda.device_count() < 8:
        env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8"], capture_output=True, text=True, env=env, cwd=ROOT)
        assert out.returncode == 2 and "device(s) are visible" in out.stderr


def _line(out):
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1, "exactly one JSON line"
    return json.loads(lines[0])


CONTRACT_KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                 "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline")


def _check_compact(text, d):
    """the ONE stdout line: strict JSON, under 4 KB, every key the bench contract names"""
    assert len(text.encode()) < 4096, len(text.encode())
    assert "\n" not in text and json.loads(text) == d
    for k in CONTRACT_KEYS:
        assert k in d, k
    assert "workload" in d["config"] and "model" not in d["config"] and d["config"]["detail"]
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-4
    c = d["cpu_baseline"]
    if c is not None:
        for k in ("value", "unit", "cores", "kind", "sample"):
            assert k in c, k


def test_compact_line_of_the_largest_stored_result_fits_the_drivers_tail():
    """round 4's full object (20.7 KB: the driver's bounded stdout tail could not parse it) through compact_line, with an
    8-rank sharded ring-key leg added: < 4 KB, every contract key, and the figures the judge recomputes from"""
    m = _bench()
    full = json.load(open(os.path.join(ROOT, "profiles", "r04_bench_default.json")))
    leg = {"queries_per_s": 812345.678, "ms_per_step": 1.2605, "merge_us_per_call": 61.234, "collectives_per_call": 3,
           "us_per_collective_round": 20.4113, "matches_unsharded": True}
    full["config"]["ringkey_sharded"] = {"workload": "x" * 120, "shards": 8, "merge": "y" * 40, "allreduce_min": leg, "allgather": leg}
    text = m.compact_line(full, "gpurun_out/bench_detail.json")
    d = json.loads(text)
    _check_compact(text, d)
    assert abs(d["value"] - full["value"]) < 1e-4 * full["value"] and abs(d["ms_per_step"] - full["ms_per_step"]) < 1e-4 * full["ms_per_step"]
    assert d["roofline"]["evals_by_level"] == full["roofline"]["evals_by_level"]
    assert d["roofline"]["bytes_per_eval_by_level"] == full["roofline"]["bytes_per_eval_by_level"]
    assert d["config"]["legs"]["ringkey_sharded"]["allreduce_min"]["matches_unsharded"] is True
    assert d["cpu_baseline"]["ate_vs_cpu_ref"]["good_flags_equal"] is True
    # an error inside a leg stays an error in the line (never silently dropped)
    full["config"]["replay"] = {"error": "boom " * 100}
    full["config"]["ringkey"] = {"error": "bang"}
    d2 = json.loads(m.compact_line(full, "x.json"))
    assert "error" in d2["config"]["legs"]["ringkey"] and d2["config"]["legs"]["replay"]
    # the batch form (no config.stream) and a rank without the CPU leg
    full["config"].pop("stream")
    full["cpu_baseline"] = None
    d3 = json.loads(m.compact_line(full, "x.json"))
    assert d3["cpu_baseline"] is None and "batch" in d3["config"]["form"]


@pytest.mark.gpu
def test_bench_line_carries_every_key_of_the_contract(tmp_path):
    detail = str(tmp_path / "detail.json")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--batch", "8", "--scenes", "2", "--steps", "2",
                          "--warmup", "1", "--cpu-seconds", "0", "--second-leg-steps", "1", "--detail-out", detail], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    last = out.stdout.strip().splitlines()[-1]
    line = _line(out)
    _check_compact(last, line)  # the LAST stdout line is the one JSON line
    assert line["n_gpus"] == 1 and line["steps"] == 2 and line["warmup"] == 1 and line["higher_is_better"] is True
    assert line["scaling"] == "weak" and line["vs_baseline"] is None and line["dtype"] == "f32" and line["data"] == "synthetic"
    # the headline workload is the one the metric names: 6 levels
    assert "6-level" in line["metric"] and "6-level" in line["config"]["workload"] and "1248x384" in line["config"]["workload"]
    assert line["config"]["detail"] == detail
    assert line["value"] > 0 and abs(line["value"] - 8 * 2 / (line["ms_per_step"] * 2e-3)) < 1e-3 * line["value"]
    legs = line["config"]["legs"]
    assert legs["reference_five_level_S1"]["value"] > 0 and legs["fixed_schedule_1p3"]["cpu_value"] > 0
    assert all(k["bit_exact"] for k in legs["ringkey"]) and len(legs["ringkey"]) == 4
    # round 6: SURVEY.md 8d's literal scene family and the PCIe-inclusive figure in the line; RPE beside the ATE (ratios within 1 %)
    assert legs["plane"]["value"] > 0 and 0 < legs["plane"]["frac_whole_step"] < 1
    assert legs["with_upload"]["value"] > 0 and legs["with_upload"]["host_MB_per_step"] > 0
    assert 0.99 <= line["cpu_baseline"]["ate_vs_cpu_ref"]["ate_ratio_gpu_over_cpu"] <= 1.01
    rpe = line["cpu_baseline"]["rpe_vs_cpu_ref"]
    assert 0.99 <= rpe["rpe_trans_ratio_gpu_over_cpu"] <= 1.01 and 0.99 <= rpe["rpe_rot_ratio_gpu_over_cpu"] <= 1.01
    # the side file holds the FULL object: the same headline numbers and every leg's own object
    d = json.load(open(detail))
    for k in CONTRACT_KEYS:
        assert k in d, k
    assert abs(d["value"] - line["value"]) < 1e-4 * d["value"]
    five = d["config"]["reference_five_level"]
    assert "5-level" in five["workload"] and five["value"] > 0 and 0 < five["roofline"]["frac"] < 1
    r = d["roofline"]
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["form"] == "sse-restatement" and c["cores"] == 1 and c["value"] > 0
    ate = c["ate_vs_cpu_ref"]
    assert ate["frames"] >= 2 and ate["good_flags_equal"] and 0.99 <= ate["ate_ratio_gpu_over_cpu"] <= 1.01
    # the three roofline fractions (contract bytes, residual-only evaluations priced at what they read, bytes the pins moved)
    assert 0 < r["frac_full_evals"] <= r["frac"] and "frac_hbm_actual" in r and r["traffic_source"]
    assert d["config"]["distinct_frames"] == 2 and d["config"]["work_queue"] == 1 and d["config"]["fixed_schedule"] == 0
    # SURVEY.md 8d's fixed schedule as a second object: 1 + 3 evaluations per level on the GPU and on the CPU leg
    fx = d["config"]["fixed_schedule_leg"]
    assert all(abs(e - 4.0) < 1e-9 for e in fx["evals_per_frame_by_level"]) and fx["value"] > 0 and fx["cpu_baseline"]["value"] > 0
    assert "same fixed schedule" in fx["cpu_baseline"]["sample"]
    ac = c["all_cores"]
    assert ac["cores"] >= 2 and ac["value"] > 0 and ac["cpu_model"]


@pytest.mark.gpu
def test_plain_run_times_the_steps_asked_for_and_dumps_the_same_outputs_every_time(tmp_path):
    """a plain run: the contract keys, exactly --steps timed steps, and --dump-outputs: the last timed step's arrays, equal from run to run"""
    import ast

    import numpy as np

    dumps = []
    env = dict(os.environ, DSM_BENCH_TRACE_STEPS="1")  # the steps the run itself took, one host time each, on stderr
    for i, form in enumerate((["--stream", "1"], ["--stream", "1"], ["--stream", "0"])):
        d = str(tmp_path / f"out{i}")
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--batch", "8", "--scenes", "3", "--steps", "3", "--warmup", "1",
                              "--dump-outputs", d, *form], capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
        line = _line(out)
        # streamed: warm-up and timed steps (1 + 3) and no step after them; batch form: the timed steps alone
        trace = [l for l in out.stderr.splitlines() if l.startswith("per-step")]
        assert len(trace) == 1 and len(ast.literal_eval(trace[0].split(": ", 1)[1])) == (1 + 3 if form[1] == "1" else 3), trace
        assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1 and line["higher_is_better"] is True and line["dtype"] == "f32"
        assert line["value"] > 0 and abs(line["value"] - 8 * 3 / (line["ms_per_step"] * 3e-3)) < 1e-3 * line["value"]
        assert line["cpu_baseline"] is None and "legs" not in line["config"] and line["config"]["detail"] is None
        assert line["config"]["all_tracked"] is True and 0 < line["roofline"]["frac_whole_step"] < 1
        dumps.append({f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)})
    for got in dumps:
        assert all(a.dtype in (np.float32, np.float64) for a in got.values())
        assert got["track_pose"].shape == (8, 7) and got["scale"].shape == (2,) and (got["track_good"] == 1).all()
    assert set(dumps[0]) == set(dumps[1]) and all(np.array_equal(dumps[0][k], dumps[1][k], equal_nan=True) for k in dumps[0])
    # the batch form returns the same bits as the streamed form (dsm_stream_*: "bit-identical to the batch calls")
    for k in dumps[2]:
        assert np.array_equal(dumps[2][k], dumps[0][k], equal_nan=True), k


@pytest.mark.gpu
def test_bench_spawns_its_own_ranks():
    """two ranks on the one device of the test box (gloo plumbing; the RCCL ring-key leg needs one device per rank)"""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--device-override", "0", "--dist-backend", "gloo",
                          "--batch", "8", "--scenes", "2", "--steps", "2", "--warmup", "1", "--no-second-leg"],
                         capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    d = _line(out)
    assert len(out.stdout.strip().splitlines()[-1].encode()) < 4096
    assert d["n_gpus"] == 2 and d["config"]["replicas"] == 2 and d["cpu_baseline"] is None
    assert abs(d["value"] - 2 * 8 * 2 / (d["ms_per_step"] * 2e-3)) < 1e-3 * d["value"]


def test_frames_are_distinct_and_round_2s_workload_is_reproducible(monkeypatch):
    """bench.build_frames: every frame in flight has its own motion, noise and initial guess (textures repeat); with
    `--scenes 8 --textures converging` the frames are round 2's eight (same seeds, same draws)"""
    import numpy as np

    m = _bench()
    from direct_stereo_slam_amd import synth as S

    w, h, K = 312, 96, (179.7, 179.7, 152.6, 47.3)  # a quarter-size geometry keeps the rendering short
    monkeypatch.setattr(sys, "argv", ["bench.py", "--batch", "40"])
    a = m.parse()
    tex, frames = m.build_frames(a, w, h, K, S.KITTI_T_STEREO)
    assert len(tex) == 18 and len(frames) == 40 and m.frame_seeds(a) == tuple(range(18))
    gts = np.array([f[2] for f in frames])
    assert len({tuple(np.round(g, 12)) for g in gts}) == 40  # 40 distinct motions
    assert not np.array_equal(frames[0][1], frames[18][1])  # same texture, another motion and noise: another image
    assert all(np.array_equal(f[3], S.IDENTITY_POSE) for f in frames)  # identity guess
    m._FRAMES.clear()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--batch", "16", "--scenes", "8", "--textures", "converging", "--scene-family", "plane"])
    a = m.parse()
    tex8, frames8 = m.build_frames(a, w, h, K, S.KITTI_T_STEREO)
    assert len(frames8) == 8 and m.frame_seeds(a) == m.SCENE_SEEDS
    # round 2 drew, per scene: reference image, motion, new image, right image from ONE generator seeded by the scene
    seed = 0x5EED0000 + m.SCENE_SEEDS[3]
    scene, rng = S.PlaneScene(seed=seed), np.random.default_rng(seed)
    ref = scene.render(K, w, h, noise=2.0, rng=rng)
    R, t = S.random_motion(rng)
    new = scene.render(K, w, h, R, t, a=0.02, b=3.0, noise=2.0, rng=rng)
    np.testing.assert_array_equal(tex8[3][1], ref)
    np.testing.assert_array_equal(frames8[3][1], new)
    np.testing.assert_array_equal(frames8[3][2], S.pose_from_Rt(R, t))
    # the constant-motion guess is the true motion up to a bounded error
    m._FRAMES.clear()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--batch", "6", "--init", "constant-motion"])
    a = m.parse()
    _, fr = m.build_frames(a, w, h, K, S.KITTI_T_STEREO)
    assert all(0 < np.abs(f[3][4:] - f[2][4:]).max() < 0.3 for f in fr)
    m._FRAMES.clear()


def test_line_guard_prints_the_parked_line_only_when_rank0_dies():
    """bench.line_guard: the finished bench line is parked with a forked helper before the multi-rank RCCL leg; a rank 0 that
    dies inside a native library still yields exactly one JSON line, an orderly one prints its own"""
    import json
    import subprocess
    import sys

    prog = ("import os, sys, json; sys.path.insert(0, %r); import bench; "
            "g = bench.line_guard({'metric': 'm', 'value': 1.0, 'unit': 'u', 'n_gpus': 2, 'steps': 1, 'warmup': 1, 'ms_per_step': 1.0, "
            "'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None, 'dtype': 'f32', 'data': 'synthetic', 'config': {'workload': 'w'}, "
            "'roofline': {'bound': 'hbm', 'achieved': 1.0, 'peak': 8000.0, 'unit': 'GB/s', 'frac': 1.25e-4, 'traffic': None}, 'cpu_baseline': None}); "
            "%s")
    died = subprocess.run([sys.executable, "-c", prog % (ROOT, "os.kill(os.getpid(), 9)")], capture_output=True, text=True, timeout=120)
    lines = [l for l in died.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["value"] == 1.0 and "error" in d["config"]["legs"]["ringkey_sharded"]
    fine = subprocess.run([sys.executable, "-c", prog % (ROOT, "g(); print(json.dumps({'value': 2.0}))")], capture_output=True, text=True, timeout=120)
    lines = [l for l in fine.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1 and json.loads(lines[0])["value"] == 2.0
