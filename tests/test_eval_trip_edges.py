"""The evaluation loop at the edges of its trip count (eval_chunk_impl, tracker_kernels.hip): a wave runs as many trips as it holds
points of the list -- not the chunk's P whatever it holds --, the two-point loop's last trip is peeled (no warp stage under an empty
lane mask, no template entries fetched behind it), and none of that may change a bit of any output.

Every count of tests/_trip_edges.py (see there: which edge each one exercises, and why two image sizes), level 0 (flow-indicator pass)
and level 1, pose and scale problems, under the three chunk tables, through dsm_diag_single_eval in every form that applies, full and
residual-only:
  * the assertions of tests/test_eval_forms_f64.py's check_forms: every output within the exact-sum bounds of tests/_gn_f64.py, form 0
    bit for bit the direct call, every other form bit for bit form 0, a residual-only evaluation's rs the full one's;
  * form 0's outputs, full and residual-only, bit for bit what the commit before the trip bound produced for the same inputs:
    tests/golden/eval_trip_edges.npz (tools/record_eval_trip_edges.py wrote it with that commit's library; every form being form 0 bit
    for bit, the file holds form 0 alone).

Then the tick engine on problems whose level sizes are such counts: poses, residuals, flags and per-level evaluation counts of an
eight-problem stream, chains off and on, bit for bit dsm_track_batch's and dsm_optimize_scale_batch's (tests/test_stream.py's checks)."""
import os

import numpy as np
import pytest

import _gn_f64 as G
import _trip_edges as E
from _gn_checks import TABLES, numpy_tracker, trackers
from _scenes import _photometry, hip_tracker, make_scene
from oracle import numpy_ref as N
from test_eval_forms_f64 import check_forms, forms_of

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_trip_edges.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return E.unpack(z)


@pytest.fixture(scope="module")
def scenes():
    return {name: E.scene(name) for name in E.SCENES}


@pytest.mark.parametrize("lvl", [0, 1])
@pytest.mark.parametrize("name", E.SCENES)
def test_trip_edges(ctx, scenes, golden, name, lvl):
    sc = scenes[name]
    counts = E.counts_of(name, lvl)
    assert counts and max(counts) <= E.capacity(sc, lvl)
    npt, trks = numpy_tracker(sc), trackers(ctx, sc)
    ref_aff, ref_exp, _ = _photometry(sc)
    pose_T = N.pose_to_matrix(np.asarray(sc.gt_pose, np.float64))
    usable = 0
    for n in counts:
        tpl = E.template_of(sc, lvl, n)
        npt.set_ref(ref_aff[0], ref_aff[1], ref_exp, *tpl)
        ref = G.pose_ref(npt, lvl, pose_T, list(sc.gt_aff), E.CUTOFF)
        sref = G.scale_ref(npt, lvl, E.SCALE, E.CUTOFF)
        usable += ref["n4"] > 0 and sref["n4"] > 0
        for t, trk in zip(TABLES, trks):
            trk.setCoarseTrackingRef(0, ref_aff, ref_exp, *tpl)
            assert trk.reduction_geometry(lvl, n) == G.reduction_geometry(n, t), (n, t)
            check_forms("pose", trk, t, ref, lvl, (sc.gt_pose, list(sc.gt_aff)), E.CUTOFF, where=f"{name} n={n}")
            check_forms("scale", trk, t, sref, lvl, (E.SCALE,), E.CUTOFF, where=f"{name} n={n}")
            assert 2 in forms_of(trk, lvl, n)  # the tick engine's form: the two-point loop on every level
            for kind in ("pose", "scale"):
                for ro in (False, True):
                    k = E.key(name, kind, lvl, t, n, ro)
                    got = E.bits(E.evaluate(trk, kind, lvl, sc, ro))
                    assert got == golden[k], ("not the bits of the commit before the trip bound", k)
    for trk in trks:
        trk.close()
    assert usable == len(counts), (usable, counts)  # every edge was met on points that count, for both problem kinds


def test_golden_file_covers_every_case(golden):
    """(no GPU work: the fixture's keys are exactly the cases above)"""
    want = {E.key(name, kind, lvl, t, n, ro) for name in E.SCENES for lvl in (0, 1) for n in E.counts_of(name, lvl) for t in TABLES
            for kind in ("pose", "scale") for ro in (False, True)}
    assert set(golden) == want
    assert {n for name in E.SCENES for n in E.counts_of(name, 0)} == set(E.COUNTS) == {n for name in E.SCENES for n in E.counts_of(name, 1)}
    # the points-per-thread values the counts reach: every one of the throughput table, the first two of the latency table
    assert {G.pts_per_thread(n, 0) for n in E.COUNTS} == {1, 2, 4, 8, 16} and {G.pts_per_thread(n, 1) for n in E.COUNTS} == {1, 2}


# level sizes (level 0, level 1) of the stream's eight problems: last chunks of one point, one wave and a point, one trip and a point,
# an odd trip bound, upper waves empty, and a whole template
STREAM_SIZES = ((4097, 257), (4096 + 65, 511), (4096 + 257, 513), (513, 1025), (2049, 65), (1025, None), (None, 63), (255, 1024))


@pytest.mark.parametrize("chain", [0, 4096])
def test_tick_engine_on_remainder_sizes(ctx, chain):
    from test_stream import _batch_reference, _check, _stream_run

    scs = []
    for i, sizes in enumerate(STREAM_SIZES):
        sc = make_scene(E.SCENES[0], seed=800 + i)
        full = [len(sc.tpl[0][l]) for l in range(sc.nl)]
        sc = _cut(sc, [full[l] if n is None else n for l, n in enumerate(sizes)])
        scs.append(sc)
    nl = scs[0].nl
    trks = [hip_tracker(ctx, sc) for sc in scs]
    scales = np.linspace(0.9, 1.2, len(trks)).astype(np.float32)
    ref = _batch_reference(ctx, trks, nl, scales)
    res, _, _ = _stream_run(ctx, trks, nl, scales.copy(), len(trks), len(trks), None, None, 1, engine=1, ticks=0, chain=chain)
    _check(res, ref, len(trks), nl)
    for trk in trks:
        trk.close()


def _cut(sc, sizes):
    """a copy of the scene's description whose template has sizes[l] points on level l (the first points of the dense template)"""
    import copy

    out = copy.copy(sc)
    assert all(n <= len(sc.tpl[0][l]) for l, n in enumerate(sizes)), sizes
    out.tpl = [[a[l][:n].copy() for l, n in enumerate(sizes)] for a in sc.tpl]
    return out
