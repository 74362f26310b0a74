"""The bars of tests/test_pose_eval_f64.py bite (no GPU): the loop-closure evaluation (mode 2) restated with ONE mistake at a time is
rejected by tests/_gn_checks.py's check_pose_outputs / common_checks against the unmutated exact sums.

The mistaken evaluation is oracle/numpy_ref.NumpyPoseEstimator's text with the one line changed, and what it hands to the assertions are
ITS OWN exact float64 sums -- no summation tree, no formation error: the most favourable case for the mistake, every difference is the
mistake's.  Inputs: 308 x 92, level 0 (the flow indicators exist there only), the true pose, cut-off 20, the first 257 / 4097 / 16 385
points, the loosest chunk table of each size.  EXPECT names the assertion of check_pose_outputs that fires first (they run in the order
numTermsInE, warped count, saturated share, E, flow, zero-scale entries, H, b):
  (a) the mode-0 warp R (x, y, 1) + t z on the mode-2 template: other pixels, other counts -- numTermsInE;
  (b) new_idepth = z / pt2 instead of 1 / pt2: the sign test and E are unchanged (z > 0), columns 0-2 of H scale with z -- H;
  (c) b0 = 3 instead of 0 in J6 = a (b0 - refColor): row 6 of H -- H;
  (d) flow shifts measured against (x, y) instead of (Ku0, Kv0) -- flow;
  (e) (x, y, z) instead of (x, y, 1) in the two translation-only flow points -- flow;
  (f) one usable point lost, one counted twice -- numTermsInE."""
import numpy as np
import pytest

import _gn_checks as K
import _gn_f64 as G
import _pose_eval as PE
from oracle import numpy_ref as N

f32 = np.float32
SIZES = (257, 4097, 16385)
EXPECT = {None: None, "warp0": "numTermsInE", "idepth_z": "H", "b0": "H", "flow_xy": "flow", "flow_xyz": "flow", "lost": "numTermsInE",
          "doubled": "numTermsInE"}


class Mistaken(N.NumpyPoseEstimator):
    """NumpyPoseEstimator.calc_res / jacobian with the line named by `mistake` changed (None: the same text, checked below)"""

    mistake = None

    def calc_res(self, lvl, T, aff, cutoff):
        m = self.mistake
        R, t = T[:3, :3].astype(np.float32), T[:3, 3].astype(np.float32)
        fx, fy, cx, cy = self.fx[lvl], self.fy[lvl], self.cx[lvl], self.cy[lvl]
        x, y, z = self.xyz[:, 0], self.xyz[:, 1], self.xyz[:, 2]
        one = f32(1)
        proj = lambda p: (fx * (p[0] / p[2]) + cx, fy * (p[1] / p[2]) + cy)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            Ku0, Kv0 = proj((x, y, z))
            if m == "warp0":
                pt = [((R[r, 0] * x + R[r, 1] * y) + R[r, 2]) + t[r] * z for r in range(3)]
            else:
                pt = [((R[r, 0] * x + R[r, 1] * y) + R[r, 2] * z) + t[r] for r in range(3)]
            u, v = pt[0] / pt[2], pt[1] / pt[2]
            Ku, Kv = fx * u + cx, fy * v + cy
            new_id = (z if m == "idepth_z" else one) / pt[2]
            flow = np.zeros(3, np.float32)
            flow_terms = (np.zeros(0, np.float32), np.zeros(0, np.float32))
            if lvl == 0:
                s = slice(0, None, 32)
                xs, ys, zs = x[s], y[s], (z[s] if m == "flow_xyz" else one)
                k0, l0 = (xs, ys) if m == "flow_xy" else (Ku0[s], Kv0[s])
                KuT, KvT = proj((xs + t[0], ys + t[1], zs + t[2]))
                KuT2, KvT2 = proj((xs - t[0], ys - t[1], zs - t[2]))
                Ku3, Kv3 = proj([((R[r, 0] * xs + R[r, 1] * ys) + R[r, 2]) - t[r] for r in range(3)])
                sq = lambda a, b: (a - k0) * (a - k0) + (b - l0) * (b - l0)
                flow_terms = (np.stack([sq(KuT, KvT), sq(KuT2, KvT2)], 1).ravel(), np.stack([sq(Ku[s], Kv[s]), sq(Ku3, Kv3)], 1).ravel())
                flow[0], flow[1] = N.seq_sum(flow_terms[0]), N.seq_sum(flow_terms[1])
                flow[2] = N.seq_sum(np.full(len(xs), 2, np.float32))
        rs, B = N._residuals(self.new_dIp[lvl], self.w[lvl], self.h[lvl], u, v, new_id, Ku, Kv, self.colors[lvl], self.huber, f32(cutoff),
                             self._aff(aff), flow, flow_terms)
        if m in ("lost", "doubled"):  # the usable point in the middle of the buffers
            k = len(B["hw"]) // 2
            sel = np.delete(np.arange(len(B["hw"])), k) if m == "lost" else np.insert(np.arange(len(B["hw"])), k, k)
            B = {key: (val if key == "flow_terms" else val[sel]) for key, val in B.items()}
            rs[1] += -1 if m == "lost" else 1
        self.buf = B
        return rs

    def jacobian(self, lvl, aff):
        b0 = f32(3.0) if self.mistake == "b0" else f32(self.ref_aff[1])
        return N._pose_vectors(self.buf, self.fx[lvl], self.fy[lvl], f32(self._aff(aff)[0]), b0)


def outputs_of(est, lvl, T, aff, cutoff):
    """(rs, H, b, n_warped) as an evaluation returns them, from the estimator's own exact sums"""
    r = G.pose2_ref(est, lvl, T, aff, cutoff)
    with np.errstate(invalid="ignore", divide="ignore"):
        sat = f32(r["n_sat"]) / f32(r["n_terms"])
    return (np.array([r["E64"], r["n_terms"], r["flow64"][0], 0.0, r["flow64"][1], sat]), r["H64"], r["b64"], r["n4"]), r


@pytest.fixture(scope="module")
def whole(built):
    return PE.scene_inputs("small", 84, SIZES[-1])


@pytest.mark.parametrize("n", SIZES)
def test_one_mistake_at_a_time_is_rejected(whole, n):
    inp = whole.cut(n)
    T, aff, cutoff = PE.matrix(inp.sc.gt_pose), [0.0, 0.0], 20.0
    ref = G.pose2_ref(PE.numpy_estimator(inp), 0, T, aff, cutoff)
    assert 4 * ref["n4"] >= n
    P = max(G.pts_per_thread(n, g) for g in K.TABLES)  # the loosest table
    est = Mistaken(inp.w, inp.h, inp.nl)
    est.load(*inp.args())
    caught = {}
    for mistake in EXPECT:
        est.mistake = mistake
        out, own = outputs_of(est, 0, T, aff, cutoff)
        try:
            K.check_pose_outputs(out, ref, P, mistake, lambda *a: None)
            caught[mistake] = None
        except AssertionError as e:
            caught[mistake] = e.args[0][0]
        if mistake is None:  # the copied text is the estimator's: the same bits
            np.testing.assert_array_equal(own["rs"], ref["rs"])
            np.testing.assert_array_equal(own["H64"], ref["H64"])
    print(n, caught)
    assert caught == EXPECT, (n, caught)


@pytest.mark.parametrize("n", SIZES)
def test_residual_only_checks_reject_the_mistakes_they_can_see(whole, n):
    """common_checks alone -- what a residual-only evaluation is held to: the mistakes in the warp, the flow pass and the point list are
    rejected, the two that touch only the Jacobian ((b), (c)) are invisible to it by construction"""
    inp = whole.cut(n)
    T, aff, cutoff = PE.matrix(inp.sc.gt_pose), [0.0, 0.0], 20.0
    ref = G.residual2_ref(PE.numpy_estimator(inp), 0, T, aff, cutoff)
    P = max(G.pts_per_thread(n, g) for g in K.TABLES)
    est = Mistaken(inp.w, inp.h, inp.nl)
    est.load(*inp.args())
    for mistake, expect in EXPECT.items():
        est.mistake = mistake
        out, _ = outputs_of(est, 0, T, aff, cutoff)
        try:
            K.common_checks(out[0], out[3], ref, P, mistake, lambda *a: None)
            got = None
        except AssertionError as e:
            got = e.args[0][0]
        assert got == (None if expect == "H" else expect), (n, mistake, got)
