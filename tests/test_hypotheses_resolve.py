"""CPU: dsm_hypotheses_resolve, the host replay behind the stream's hypothesis groups (dsm_stream_submit_hypotheses).  Every try of
FrontEnd::trackNewCoarse's list (FrontEnd.cpp:194-256) runs on the oracle tracker WITHOUT abort; the resolver, fed with their outputs in
try order, must give exactly what the reference's sequential loop -- with the real aborts of TrackerAndScaler.cpp:598 -- gives on the
same oracle, and must call the loop undecided for exactly the prefixes the sequential loop runs past."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from direct_stereo_slam_amd import synth as S

from _scenes import make_scene, oracle_tracker, regrad
from test_track_hypotheses import reference_tries, sequential_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["first_try_wins", "needs_retries", "all_fail", "middle_takeover"]


def hypothesis_scene(case):
    """(scene, constant-motion guess, last_coarse_rmse0): test_track_hypotheses' three scenes, plus one whose constant-motion try is poor
    (level-0 residual ~9.9) and whose 6th try takes over below the threshold: the loop stops in the middle of the list"""
    if case == "first_try_wins":
        sc = make_scene("small", seed=81)
        return sc, sc.gt_pose.copy(), 100.0
    if case == "needs_retries":
        return make_scene("small", seed=82, motion_scale=4.0), S.IDENTITY_POSE.copy(), 0.5
    if case == "all_fail":
        sc = make_scene("small", seed=83)
        sc.new_p = [regrad(np.full_like(p, np.nan)) for p in sc.new_p]
        return sc, S.IDENTITY_POSE.copy(), 1.0
    return make_scene("small", seed=86, motion_scale=5.0), S.IDENTITY_POSE.copy(), 2.0


@functools.lru_cache(maxsize=None)
def oracle_runs(case):
    """the sequential reference and every try run without abort, on the oracle"""
    sc, const_motion, last_rmse0 = hypothesis_scene(case)
    tries = reference_tries(const_motion)
    orc = oracle_tracker(sc)
    ref = sequential_reference(orc, tries, [0.0, 0.0], sc.nl - 1, last_rmse0)
    outs = [orc.track(t, [0.0, 0.0], sc.nl - 1) for t in tries]  # min_res None = all NaN: no abort
    per_try = tuple(np.array([o[j] for o in outs]) for j in range(5))  # good, pose, aff, last_residuals, flow
    return sc.nl, tries, last_rmse0, ref, per_try


def resolve(case, k):
    from direct_stereo_slam_amd.tracker import hypotheses_resolve

    nl, tries, last_rmse0, _, (good, pose, aff, last, flow) = oracle_runs(case)
    return hypotheses_resolve(tries, [0.0, 0.0], nl - 1, last_rmse0, good[:k], pose[:k], aff[:k], last[:k], flow[:k])


def assert_same_outcome(got, ref):
    assert got[0] == ref[0]
    assert np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2]) and np.array_equal(got[3], ref[3])
    assert np.array_equal(got[4], ref[4], equal_nan=True)
    assert got[5] == ref[5]


@pytest.mark.parametrize("case", CASES)
def test_resolver_reproduces_the_sequential_loop_exactly(built, case):
    _, tries, _, ref, _ = oracle_runs(case)
    decided, got = resolve(case, len(tries))
    assert decided
    assert_same_outcome(got, ref)
    assert got[6] == len(tries)  # tries_run: what it was fed
    used = ref[5]
    if case == "first_try_wins":
        assert used == 1 and ref[0]
    elif case == "needs_retries":
        assert used > 5 and ref[0]
    elif case == "all_fail":
        assert used == len(tries) and not ref[0] and np.array_equal(got[3], np.zeros(3))
    else:
        assert 1 < used < len(tries) // 2 and ref[0]


@pytest.mark.parametrize("case", CASES)
def test_prefix_is_undecided_exactly_while_the_loop_goes_on(built, case):
    _, tries, _, ref, _ = oracle_runs(case)
    used = ref[5]
    for k in range(len(tries) + 1):
        decided, got = resolve(case, k)
        assert decided == (k >= used), (k, used)
        if decided:
            assert_same_outcome(got, ref)
        else:
            assert got[5] == k


def test_resolver_argument_checks(built):
    from direct_stereo_slam_amd import _lib

    L = _lib.load()
    tries = np.tile(S.IDENTITY_POSE, (3, 1))
    aff = np.zeros(2)
    out, dec = _lib.StreamHypResult(), C.c_int()
    dp = lambda a: a.ctypes.data_as(_lib.c_double_p)  # noqa: E731
    assert L.dsm_hypotheses_resolve(3, dp(tries), dp(aff), 2, 1.0, 1.5, 0, None, None, None, None, None, C.byref(out), C.byref(dec)) == 0
    assert dec.value == 0 and out.tries_used == 0 and not out.have_one_good and np.array_equal(np.array(out.pose), S.IDENTITY_POSE)
    assert L.dsm_hypotheses_resolve(0, dp(tries), dp(aff), 2, 1.0, 1.5, 0, None, None, None, None, None, C.byref(out), C.byref(dec)) == -1
    assert L.dsm_hypotheses_resolve(3, dp(tries), dp(aff), 2, 1.0, 1.5, 4, None, None, None, None, None, C.byref(out), C.byref(dec)) == -1
    assert L.dsm_hypotheses_resolve(3, dp(tries), dp(aff), 2, 1.0, 1.5, 1, None, None, None, None, None, C.byref(out), C.byref(dec)) == -1
    assert L.dsm_hypotheses_resolve(3, None, dp(aff), 2, 1.0, 1.5, 0, None, None, None, None, None, C.byref(out), C.byref(dec)) == -1
    assert L.dsm_hypotheses_resolve(3, dp(tries), dp(aff), 6, 1.0, 1.5, 0, None, None, None, None, None, C.byref(out), C.byref(dec)) == -1


def test_hyp_result_layout_matches_the_header(built, tmp_path):
    """the ctypes mirror of dsm_stream_hyp_result: size and every field's offset as a C compiler lays the header's struct out"""
    from direct_stereo_slam_amd import _lib

    fields = [f for f, _ in _lib.StreamHypResult._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "dsm_hotpath.h"\nint main(void) {\n'
                   '  printf("size %zu\\n", sizeof(dsm_stream_hyp_result));\n'
                   + "".join(f'  printf("{f} %zu\\n", offsetof(dsm_stream_hyp_result, {f}));\n' for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(_lib.StreamHypResult)
    for f in fields:
        assert int(got[f]) == getattr(_lib.StreamHypResult, f).offset, f
