"""GPU: hypothesis groups of the stream (dsm_stream_submit_hypotheses) -- FrontEnd::trackNewCoarse's whole list (FrontEnd.cpp:194-256) as
ONE submission.  A group is scheduling only: under both engines and any window its result equals tracker.track_hypotheses (try 0 alone,
then the rest as one batch) on the same tracker and frame bit for bit, and the plain problems sharing the stream with it come back as they
do without it."""
import ctypes as C
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from direct_stereo_slam_amd import synth as S

from _scenes import hip_tracker, make_scene
from test_hypotheses_resolve import CASES, hypothesis_scene
from test_track_hypotheses import reference_tries

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def groups(ctx):
    """per case: (tracker, tries, last_coarse_rmse0, track_hypotheses' result)"""
    from direct_stereo_slam_amd.tracker import track_hypotheses

    out = {}
    for case in CASES:
        sc, const_motion, last_rmse0 = hypothesis_scene(case)
        trk = hip_tracker(ctx, sc)
        tries = reference_tries(const_motion)
        out[case] = (trk, tries, last_rmse0, track_hypotheses(ctx, trk, tries, [0.0, 0.0], sc.nl - 1, last_rmse0), sc.nl)
    yield out
    for trk, *_ in out.values():
        trk.close()


@pytest.fixture(scope="module")
def others(ctx):
    """trackers of other sequences whose plain track / scale problems share the stream with the groups"""
    scs = [make_scene("small", seed=s) for s in (91, 92, 93)]
    trks = [hip_tracker(ctx, sc) for sc in scs]
    yield trks
    for t in trks:
        t.close()


def same_hypotheses(got, ref):
    assert got[0] == ref[0]
    for a, b in zip(got[1:5], ref[1:5]):
        assert np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True), (a, b)
    assert got[5] == ref[5]


def plain_fields(r):
    """every output of a plain result as one float64 vector (compared with np.array_equal, NaN equal to NaN)"""
    return np.concatenate([[r.kind, r.good, r.status], r.pose, r.aff, r.last_residuals, r.flow, [r.scale, r.err], np.array(r.evals, np.float64)])


def run_stream(ctx, engine, window, groups, others, with_groups):
    from direct_stereo_slam_amd.tracker import Stream

    st = Stream(ctx, 16, 4, engine=engine)
    st.set_hypothesis_window(window)
    plain, gtk = [], {}
    poses = np.tile(S.IDENTITY_POSE, (len(others), 1))
    plain += st.submit_track(others, poses, np.zeros((len(others), 2)), 2)
    plain += st.submit_scale(others, np.ones(len(others)), 2)
    if with_groups:
        for case, (trk, tries, last_rmse0, _, nl) in groups.items():
            gtk[st.submit_hypotheses(trk, tries, [0.0, 0.0], nl - 1, last_rmse0)] = case
        assert st.hypotheses_counts() == (len(groups), 0)
    plain += st.submit_track(others[::-1], poses, np.zeros((len(others), 2)), 2)
    st.advance()
    st.drain()
    assert st.counts() == (0, 0, len(plain))  # drain returned with every group resolved and nothing resident or waiting
    res = {r.ticket: r for r in st.results()}
    hyp = st.hypotheses_results()
    assert st.hypotheses_counts() == (0, 0)
    st.close()
    assert sorted(res) == sorted(plain)  # (a group try's result never appears among the plain results)
    return [plain_fields(res[t]) for t in plain], {gtk[t]: r for t, r in hyp}, [t for t, _ in hyp]


@pytest.mark.parametrize("engine", [0, 1])
@pytest.mark.parametrize("window", [1, 8, None])
def test_groups_equal_track_hypotheses_and_leave_plain_problems_alone(ctx, groups, others, engine, window):
    plain_ref, _, _ = run_stream(ctx, engine, window, groups, others, False)
    plain, hyp, order = run_stream(ctx, engine, window, groups, others, True)
    assert len(plain) == len(plain_ref)
    for got, ref in zip(plain, plain_ref):  # bit for bit, same order of submission
        assert np.array_equal(got, ref, equal_nan=True), (got, ref)
    assert sorted(hyp) == sorted(CASES) and len(order) == len(CASES)
    for case, got in hyp.items():
        ref = groups[case][3]
        same_hypotheses(got, ref)
        tries_used, tries_run = got[5], got[6]
        assert tries_used <= tries_run <= len(groups[case][1])
        if window == 1:  # one by one, as the reference runs them
            assert tries_run == tries_used, case
        elif window is None and tries_used > 1 and engine == 1:  # every try after try 0 handed to the device's waiting ring at once
            assert tries_run == len(groups[case][1]), case
    if window is None and engine == 0:  # 16 slots: the tries still waiting on the host when the loop was decided were dropped
        assert hyp["middle_takeover"][6] < len(groups["middle_takeover"][1])
        if case == "first_try_wins":
            assert tries_run == 1
    assert hyp["middle_takeover"][5] > 1 and hyp["needs_retries"][5] > 5 and not hyp["all_fail"][0]


def test_group_statistics(ctx, groups):
    from direct_stereo_slam_amd.tracker import Stream

    trk, tries, last_rmse0, ref, nl = groups["middle_takeover"]
    st = Stream(ctx, 8, 0, engine=1)
    tk = st.submit_hypotheses(trk, tries, [0.0, 0.0], nl - 1, last_rmse0)
    assert st.counts()[:2] == (0, 1)  # try 0 waits as a track problem
    st.drain()
    (r,) = st.hypotheses_results(raw=True)
    st.close()
    assert r.ticket == tk and r.tries_used == ref[5] and r.tries_run == len(tries)  # default window: every try after try 0 at once
    assert r.advances >= 2 and r.evals[0] >= r.tries_run  # every try run evaluates level 0 at least once


def test_argument_checks(ctx, groups):
    from direct_stereo_slam_amd import _lib
    from direct_stereo_slam_amd.tracker import Stream

    L = _lib.load()
    trk, tries, last_rmse0, _, nl = groups["first_try_wins"]
    tries = np.ascontiguousarray(tries, np.float64)
    aff = np.zeros(2)
    dp = lambda a: a.ctypes.data_as(_lib.c_double_p)  # noqa: E731
    tk = C.c_uint64()
    st = Stream(ctx, 4, 2)
    assert L.dsm_stream_submit_hypotheses(st.h, trk.h, 0, dp(tries), dp(aff), nl - 1, 1.0, 1.5, C.byref(tk)) == -1
    assert L.dsm_stream_submit_hypotheses(st.h, trk.h, 3, None, dp(aff), nl - 1, 1.0, 1.5, C.byref(tk)) == -1
    assert L.dsm_stream_submit_hypotheses(st.h, trk.h, 3, dp(tries), None, nl - 1, 1.0, 1.5, C.byref(tk)) == -1
    assert L.dsm_stream_submit_hypotheses(st.h, None, 3, dp(tries), dp(aff), nl - 1, 1.0, 1.5, C.byref(tk)) == -1
    assert L.dsm_stream_submit_hypotheses(st.h, trk.h, 3, dp(tries), dp(aff), nl - 1, 1.0, 1.5, None) == -1
    assert L.dsm_stream_submit_hypotheses(st.h, trk.h, 3, dp(tries), dp(aff), nl, 1.0, 1.5, C.byref(tk)) == -1  # coarsest level
    assert L.dsm_stream_set_hypothesis_window(st.h, -1) == -1
    # a tracker of another geometry than the stream's: the stream's geometry rule
    assert L.dsm_stream_submit_hypotheses(st.h, trk.h, 3, dp(tries), dp(aff), nl - 1, 1.0, 1.5, C.byref(tk)) == 0
    other = hip_tracker(ctx, make_scene("tiny", seed=5))
    assert L.dsm_stream_submit_hypotheses(st.h, other.h, 3, dp(tries), dp(aff), 1, 1.0, 1.5, C.byref(tk)) == -1
    assert st.hypotheses_counts() == (1, 0)  # the refused submissions left nothing behind
    st.drain()
    assert st.hypotheses_counts() == (0, 1)
    st.close()
    other.close()
    no_track = Stream(ctx, 0, 2)
    assert L.dsm_stream_submit_hypotheses(no_track.h, trk.h, 3, dp(tries), dp(aff), nl - 1, 1.0, 1.5, C.byref(tk)) == -1
    no_track.close()


def test_destroying_a_stream_with_groups_pending(ctx, groups):
    from direct_stereo_slam_amd.tracker import Stream, track_hypotheses

    trk, tries, last_rmse0, ref, nl = groups["needs_retries"]
    for engine in (0, 1):
        st = Stream(ctx, 8, 0, engine=engine)
        st.set_hypothesis_window(4)
        st.submit_hypotheses(trk, tries, [0.0, 0.0], nl - 1, last_rmse0)
        st.advance()
        st.advance()
        assert st.hypotheses_counts()[0] == 1
        st.close()
    same_hypotheses(track_hypotheses(ctx, trk, tries, [0.0, 0.0], nl - 1, last_rmse0), ref)  # the context and tracker are still fine


def test_cpp_stream_submit_hypotheses_matches_track_hypotheses(ctx, tmp_path, groups):
    """host/hypotheses_stream_demo.cpp: dsm_host::Stream::submitHypotheses under both engines and windows 0 (all) / 1 / 8 against
    dsm_host::trackHypotheses on the needs_retries scene, field for field"""
    from test_host_adaptor import run_host, write_fixture

    sc, const_motion, last_rmse0 = hypothesis_scene("needs_retries")
    tries = reference_tries(const_motion)
    write_fixture(sc, tmp_path / "fixture.bin")
    with open(tmp_path / "tries.bin", "wb") as f:
        f.write(struct.pack("i", len(tries)) + np.ascontiguousarray(tries, np.float64).tobytes())
    d = json.loads(run_host("hypotheses_stream_demo", tmp_path / "fixture.bin", str(tmp_path / "tries.bin"), repr(last_rmse0)))
    ref = groups["needs_retries"][3]
    assert d["have"] == int(ref[0]) and d["tries_used"] == ref[5] > 5 and d["n_tries"] == len(tries)
    assert np.array_equal(d["pose"], ref[1])  # the C++ and the Python adaptor: the same library calls
    assert len(d["groups"]) == 6
    for g in d["groups"]:
        assert g["equal"] == 1, g
        assert g["tries_run"] >= d["tries_used"]
        if g["window"] == 1:
            assert g["tries_run"] == d["tries_used"]


def test_replay_concurrent_leg_with_hypothesis_groups(ctx, tmp_path, monkeypatch):
    """tools/replay/replay_bench.cpp with DSM_REPLAY_HYPOTHESES=stream: every frame's list is one group; the tool's own check holds --
    every sequence's trajectory and scales equal the one-sequence run's"""
    from test_replay_bench import _run

    monkeypatch.setenv("DSM_REPLAY_HYPOTHESES", "stream")
    d, _ = _run(tmp_path, "gpu", extra=("6", "1"))
    c = d["concurrent"]
    assert c["hypothesis_lists_as_stream_groups"] is True
    assert c["sequences"] == 6 and c["frames"] == 6 * 44 and c["frames_lost"] == 0
    assert c["max_abs_trajectory_diff_vs_the_one_sequence_run_m"] == 0.0 and c["scales_equal_the_one_sequence_run"] is True
