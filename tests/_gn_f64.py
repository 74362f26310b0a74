"""float64 reference of one Gauss-Newton evaluation and the error bound the device's summation tree has to meet.

For one pose evaluation (calcResPose + calcGSSSEPose) `pose_ref` returns the EXACT sums of oracle/numpy_ref.py's float32
per-point values -- E64, H64 (8x8), b64 (8), the flow-indicator sums -- next to the same sums over absolute values (A, Ab,
the scale of every entry), the formation term F / Fb derived below, and the exact integer outputs.  `scale_ref` does the
same for calcResScale + calcGSSSEScale (h00, h01).  numpy_ref is pinned bit for bit to the C oracle
(tests/test_oracle_numpy_ref.py), so these are the values that both the device and the oracle approximate.  A product of
float32 values is exact in float64 up to 2^-53 and the float64 sums add at most n 2^-53 A_ij (below 2^-29 A_ij at the 2 M
points of the largest level): negligible next to 2^-24.  1 / n is float32 and the scales are applied in double as
TrackerAndScaler.cpp:682-692 does -- the device uses the same float 1 / n (build_H_elem), so it is a common factor.

The bound, u = 2^-24, P = points per thread of the level (dsm_kernels.hpp pts_per_thread), first order:

  |H_dev - H64|_ij <= u ((P + K_TREE) A_ij + F_ij)        (b, h00 / h01 alike; E: u (P + K_TREE + K_HUBER) E64)

* K_TREE = 24 roundings besides the thread's P sequential fmaf (eval_chunk_impl, tracker_kernels.hip): J_r w (1), the 16-lane DPP tree
  row16_sum (4), the 16 rows in order (15), the chunk partial stored as float and the chunks added in double
  (reduce_partials_groups / _final, lm_step.hpp: below 2^-40 for 4096 chunks), the float of the double sum (build_H_elem, build_rs: 1),
  and for the scale problem the float product with 1 / n (LM_OP_SINGLE_FINISH: 1) -- 22, plus the doubles of the scales.
* The per-point values are NOT all the oracle's bits: the integer outputs and the residual are (same float32 operations),
  but the Jacobian and the Huber weight are formed differently (tracker_kernels.hip taps_gradients, stage_a / stage_b):
  - the Huber weight is min(1, huber * rcp(|r|)): <= 2 u (rcp) + u (product) + u (the oracle's division): K_HUBER = 4 on
    every product (and on every term of E, whose derivative in the weight is below its own size);
  - the gradients are interpolated from the intensities' central differences with an fmaf chain (4 roundings) where the
    oracle interpolates the stored gradient channel (4), each then times the focal length (1 + 1): <= 10 u Dx with
    Dx = fx * (the interpolation of |dx|), the scale of the interpolated value;
  - new_idepth is id times a refined hardware reciprocal (<= 3 u) where the oracle divides (u): 4 u |new_idepth|;
  - J0..J5 are formed with fmaf (<= 3 roundings per term) where the oracle rounds every operation (<= 4).
  So |J_dev - J_orc|_i <= K_FORM u Jt_i with K_FORM = 10 + 4 + 7 = 21, where Jt_i is J_i's formula on absolute values with
  Dx, Dy in place of dx, dy (Jt = 0 for J6, J7 and the residual, formed by the same operations on both sides), and
      F_ij = sum over points of w (K_HUBER |J_i J_j| + K_FORM (Jt_i |J_j| + |J_i| Jt_j)).
  The scale problem's J0 differs by the gradients only (its other operations are the oracle's): the same F with
  Jt0 = Dx |deno xno| + Dy |deno yno|.
* The loop-closure evaluation (MODE == 2, PoseEstimator.cpp:84-296; `pose2_ref` on oracle/numpy_ref.NumpyPoseEstimator) goes through the
  same stage_b, the same tree and the same LM_OP_SINGLE_FINISH, so P, K_TREE and K_HUBER are unchanged and F has the same form with
  Jt built from |new_id|, |u|, |v| of the mode-2 buffers.  K_FORM is re-derived from eval_chunk_impl's MODE == 2 text:
  - the warp pt = ((R0 x + R1 y) + R2 z) + t is the oracle's operation sequence (no contraction); u and v are the IEEE quotients bit
    for bit on both paths of stage_a (they decide the integer outputs, which are asserted equal), so they add nothing;
  - the gradients and J0..J5 are stage_b's, as above: 10 + 7;
  - new_idepth is r1 ITSELF, r1 = fma(fma(-pt2, r0, 1), r0, r0) with r0 = rcp(pt2) (1 + e0), |e0| <= 2^-23: the inner fma returns
    -e0 up to 2^-47, so r1 = (1 - e0^2) / pt2 rounded once: <= u (+ 2^-46), against the oracle's correctly rounded 1 / pt2 (u): 2 u
    |new_idepth| where modes 0 / 1 have 4 u (no product with id).  A wave with a lane outside 2^-33 <= |pt2| < 2^32 takes the IEEE
    division: the oracle's bits.  No operand of this is subnormal inside the range (|r1| in (2^-32, 2^33]);
  - J6 = a (0 - refColor): b0 is forced to 0 on the device (make_eval_level) and is ref_aff_g2l_.b = 0 in the reference, 0 - refColor
    is exact and the one product is the same operation on both sides; J7 = -1 and the residual hit - (a refColor + b) likewise: Jt = 0.
  So K_FORM2 = 10 + 2 + 7 = 19 for mode 2: a smaller constant than 21 because the quotient loses its product, and the one used.
  The flow pass of mode 2 (shifts against (Ku0, Kv0), translation-only points (x, y, 1), divisions by z, 1 +- t2 and p3z) is the
  oracle's operation sequence term by term, so its bound is the tree's, as below; a term that is not finite on one side is the same
  non-finite value on the other.
* Flow indicators: one point per thread (two adds), the tree, the float of the double sum: u K_TREE sum / (N + 0.1), all
  terms >= 0.
"""
import numpy as np

from oracle import numpy_ref as N

U = 2.0 ** -24
K_TREE = 24
K_HUBER = 4
K_FORM = 21
K_FORM2 = 19
THREADS = 256


def pts_per_thread(n, geometry):
    """dsm_kernels.hpp pts_per_thread: 0 throughput, 1 latency, 2 chain (latency above 4096 points, throughput below)"""
    if geometry == 1 or (geometry == 2 and n > 4096):
        return 16 if n >= 256 * 1024 else 8 if n >= 64 * 1024 else 4 if n >= 16 * 1024 else 2 if n >= 4 * 1024 else 1
    return 16 if n > 2048 else 8 if n > 1024 else 4 if n > 512 else 2 if n > 256 else 1


def reduction_geometry(n, geometry):
    """(threads per chunk, points per thread, chunks) as dsm_reduction_geometry reports them"""
    p = pts_per_thread(n, geometry)
    return THREADS, p, (n + THREADS * p - 1) // (THREADS * p)


def _abs_interp(img, Ku, Kv):
    """getInterpolatedElement33 of |texel| (the bilinear weights are >= 0): the scale of each interpolated gradient, in float64"""
    return N.interp33(np.abs(img), Ku, Kv).astype(np.float64)


def _pad(a, n4):
    a = np.asarray(a, np.float64)
    return np.concatenate([a, np.zeros(n4 - len(a))])


def energy_terms(buf):
    """the usable points' float32 terms of E (:809), in the order of the buffer"""
    hw, r = buf["hw"], buf["residual"]
    return ((hw * r) * r) * (np.float32(2) - hw)


def _common(npt, buf, rs, cutoff):
    max_energy = N.f32(N.f32(N.f32(2) * npt.huber) * N.f32(cutoff)) - N.f32(npt.huber * npt.huber)
    n_terms = int(rs[1])
    n_sat = n_terms - len(buf["hw"])  # finite points minus the usable ones: the saturated (:797)
    fT, fRT = (t.astype(np.float64) for t in buf["flow_terms"])
    nflow = float(len(fT))  # two terms per flow point, each counting 2 / 2 (:784)
    return dict(rs=rs, n_terms=n_terms, n_sat=n_sat, sat_ratio=np.float32(rs[5]), max_energy=max_energy,
                E64=float(np.sum(energy_terms(buf).astype(np.float64))) + n_sat * float(max_energy),
                flow64=np.array([np.sum(fT) / (nflow + 0.1), np.sum(fRT) / (nflow + 0.1)]))


def residual_ref(npt, lvl, T, aff, cutoff):
    """the residual side of one pose evaluation alone -- what a residual-only evaluation returns: the integer outputs, E64 and the flow
    sums of pose_ref without the Jacobians (and the buffers of the usable points, `buf`)"""
    rs = npt.calc_res_pose(lvl, T, aff, cutoff)
    B = npt.pose_buf
    out = _common(npt, B, rs, cutoff)
    out.update(n4=(len(B["hw"]) + 3) & ~3, idx=B["idx"], n_tpl=len(npt.pc[lvl][0]), Eterms=energy_terms(B), buf=B)
    return out


def _pose_sums(out, B, J, w, fx, fy, cx, cy, img, scales, k_form):
    """the exact sums, their absolute scales and the formation terms of one pose-like evaluation (modes 0 and 2) from the float32
    per-point vectors J (9 x n4) and weights w of the buffers B; (fx, fy, cx, cy) and img: the level's camera and target"""
    n4 = len(w)
    Jd = np.array(J, np.float64)  # (9, n4)
    Wd = np.asarray(w, np.float64)
    Ja = np.abs(Jd)
    # Jt: J's formulas on absolute values, the interpolated gradients replaced by their scale (see the module docstring)
    Ku, Kv = fx * B["u"] + cx, fy * B["v"] + cy  # the same float32 operations as the restatement's warp
    G = _abs_interp(img, Ku, Kv)
    Dx, Dy = _pad(G[:, 1] * float(fx), n4), _pad(G[:, 2] * float(fy), n4)
    u, v, nid = (np.abs(_pad(B[k], n4)) for k in ("u", "v", "new_id"))
    Jt = np.zeros_like(Jd)
    Jt[0], Jt[1] = nid * Dx, nid * Dy
    Jt[2] = nid * (u * Dx + v * Dy)
    Jt[3] = (u * v) * Dx + Dy * (1 + v * v)
    Jt[4] = (u * v) * Dy + Dx * (1 + u * u)
    Jt[5] = u * Dy + v * Dx
    with np.errstate(invalid="ignore", over="ignore"):
        S9 = (Jd * Wd) @ Jd.T
        A9 = (Ja * Wd) @ Ja.T
        C9 = (Jt * Wd) @ Ja.T
    F9 = K_HUBER * A9 + k_form * (C9 + C9.T)
    invn = float(np.float32(1.0) / np.float32(n4)) if n4 else 0.0
    s = scales
    sc = lambda M: (M[:8, :8] * invn * s[None, :]) * s[:, None]
    scb = lambda M: M[:8, 8] * invn * s
    out.update(H64=sc(S9), b64=scb(S9), A=sc(A9), Ab=scb(A9), F=sc(F9), Fb=scb(F9), products=(Jd, Wd))
    return out


def pose_ref(npt, lvl, T, aff, cutoff):
    """one pose evaluation of NumpyTracker npt at the 4x4 pose T"""
    rs = npt.calc_res_pose(lvl, T, aff, cutoff)
    B = npt.pose_buf
    J, w = npt.pose_jacobian(lvl, aff)
    out = _common(npt, B, rs, cutoff)
    out.update(n4=len(w), idx=B["idx"], n_tpl=len(npt.pc[lvl][0]), Eterms=energy_terms(B))
    return _pose_sums(out, B, J, w, npt.fx[lvl], npt.fy[lvl], npt.cx[lvl], npt.cy[lvl], npt.new_dIp[lvl], npt.scales, K_FORM)


def residual2_ref(npe, lvl, T, aff, cutoff):
    """residual_ref for the loop-closure evaluation (mode 2) of NumpyPoseEstimator npe"""
    rs = npe.calc_res(lvl, T, aff, cutoff)
    B = npe.buf
    out = _common(npe, B, rs, cutoff)
    out.update(n4=(len(B["hw"]) + 3) & ~3, idx=B["idx"], n_tpl=len(npe.xyz), Eterms=energy_terms(B), buf=B)
    return out


def pose2_ref(npe, lvl, T, aff, cutoff):
    """pose_ref for the loop-closure evaluation (mode 2): PoseEstimator::calcRes + calcGSSSE of NumpyPoseEstimator npe"""
    rs = npe.calc_res(lvl, T, aff, cutoff)
    B = npe.buf
    J, w = npe.jacobian(lvl, aff)
    out = _common(npe, B, rs, cutoff)
    out.update(n4=len(w), idx=B["idx"], n_tpl=len(npe.xyz), Eterms=energy_terms(B), buf=B)
    return _pose_sums(out, B, J, w, npe.fx[lvl], npe.fy[lvl], npe.cx[lvl], npe.cy[lvl], npe.new_dIp[lvl], npe.scales, K_FORM2)


def scale_ref(npt, lvl, scale, cutoff):
    """one scale evaluation of NumpyTracker npt"""
    rs = npt.calc_res_scale(lvl, scale, cutoff)
    B = npt.scale_buf
    J0, J1, w = npt.scale_jacobian(lvl, scale)
    n4 = len(w)
    out = _common(npt, B, rs, cutoff)
    out.update(n4=n4, idx=B["idx"], n_tpl=len(npt.pc[lvl][0]), Eterms=energy_terms(B))
    fx, fy, cx, cy = npt.fx1[lvl], npt.fy1[lvl], npt.cx1[lvl], npt.cy1[lvl]
    Ku, Kv = fx * B["u"] + cx, fy * B["v"] + cy
    G = _abs_interp(npt.right_dIp[lvl], Ku, Kv)
    Dx, Dy = _pad(G[:, 1] * float(fx), n4), _pad(G[:, 2] * float(fy), n4)
    t = npt.T10[:3, 3].astype(np.float32)
    rx1, rx2, rx3 = (_pad(a, n4) for a in B["rx"])
    with np.errstate(divide="ignore", invalid="ignore"):
        deno = 1.0 / (float(np.float32(scale)) * rx3 + float(t[2])) ** 2
    xno, yno = rx1 * float(t[2]) - rx3 * float(t[0]), rx2 * float(t[2]) - rx3 * float(t[1])
    Jt0 = np.where(Dx + Dy > 0, Dx * np.abs(deno * xno) + Dy * np.abs(deno * yno), 0.0)
    j0, j1, wd = (np.asarray(a, np.float64) for a in (J0, J1, w))
    invn = float(np.float32(1.0) / np.float32(n4)) if n4 else 0.0
    h = np.array([np.sum(wd * j0 * j0), np.sum(wd * j0 * j1)]) * invn
    A = np.array([np.sum(wd * j0 * j0), np.sum(wd * np.abs(j0 * j1))]) * invn
    F = np.array([K_HUBER * np.sum(wd * j0 * j0) + 2 * K_FORM * np.sum(wd * Jt0 * np.abs(j0)),
                  K_HUBER * np.sum(wd * np.abs(j0 * j1)) + K_FORM * np.sum(wd * Jt0 * np.abs(j1))]) * invn
    out.update(h64=h, A=A, F=F, products=(np.array([j0, j1]), wd))
    return out


def bound(A, F, P):
    """the error bound of sums with absolute scale A and formation term F at P points per thread"""
    return U * ((P + K_TREE) * np.asarray(A) + np.asarray(F))


def energy_bound(E64, P):
    return U * (P + K_TREE + K_HUBER) * E64


def flow_bound(flow64):
    return U * K_TREE * np.abs(flow64)
