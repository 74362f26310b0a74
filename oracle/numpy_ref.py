"""A SECOND, independent restatement of the tracker's hot path in vectorised numpy float32.  TEST INFRASTRUCTURE ONLY.

Written from the text of the reference (src/scale_optimization/TrackerAndScaler.cpp, ScaleAccumulator.h), NOT from
oracle/dsm_oracle.c: its job is to remove single-author risk from the C oracle (tests/test_oracle_numpy_ref.py asserts
the two agree -- per evaluation bit for bit, per LM run in the accept / reject sequence, the integer counts and the
result).  It does not make parity "pinned": the reference itself still cannot be built or run here.

Structure differs from the C oracle on purpose: whole-array numpy arithmetic (IEEE float32 element-wise = the reference's
scalar float code without FMA contraction), np.cumsum for the sequential float sums (quirk Q1: E in point order),
block-wise cumsum for the SSE lane accumulators with their 1k / 1m shift-up (quirk Q4), poses as 4x4 double matrices with
the Lie-group exponential taken by scipy.linalg.expm instead of Sophus' closed form, numpy.linalg for nothing that
decides (the LDLT is written out, pivoting on the largest |diagonal| as Eigen's LDLT does).

UPSTREAM-DSO semantics restated from their published form (not present under /root/reference, hence recalled, not cited):
getInterpolatedElement33 (bilinear, weights dxdy, dy-dxdy, dx-dxdy, 1-dx-dy+dxdy on taps (+1,+1),(0,+1),(+1,0),(0,0)),
AffLight::fromToVecExposure, Accumulator9's lane / shift-up scheme (the same scheme ScaleAccumulator.h:60-105 spells out in
the reference tree), Eigen's Matrix3f::inverse() (cofactors * 1/det) and quaternion -> rotation matrix.
"""
import math

import numpy as np

f32 = np.float32


def _f(x):
    return np.asarray(x, dtype=np.float32)


def quat_to_rot(q):
    """Eigen QuaternionBase::toRotationMatrix (double)"""
    x, y, z, w = (float(v) for v in q)
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1.0 - (tyy + tzz), txy - twz, txz + twy],
                     [txy + twz, 1.0 - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, 1.0 - (txx + tyy)]])


def pose_to_matrix(pose):
    T = np.eye(4)
    T[:3, :3] = quat_to_rot(pose[:4])
    T[:3, 3] = pose[4:7]
    return T


def matrix_to_pose(T):
    """rotation matrix -> unit quaternion (x, y, z, w), w >= 0 ; translation"""
    from scipy.spatial.transform import Rotation

    q = Rotation.from_matrix(T[:3, :3]).as_quat()
    if q[3] < 0:
        q = -q
    return np.concatenate([q, T[:3, 3]])


def se3_exp(xi):
    """SE3::exp of the tangent (upsilon, omega) as a 4x4 matrix: the matrix exponential of the twist"""
    from scipy.linalg import expm

    ups, om = xi[:3], xi[3:6]
    A = np.zeros((4, 4))
    A[:3, :3] = [[0, -om[2], om[1]], [om[2], 0, -om[0]], [-om[1], om[0], 0]]
    A[:3, 3] = ups
    return expm(A)


def aff_from_to(expF, expT, g2F, g2T):
    """AffLight::fromToVecExposure (upstream DSO; call sites TrackerAndScaler.cpp:647-649,717-720)"""
    expF, expT = float(f32(expF)), float(f32(expT))
    if expF == 0 or expT == 0:
        expF = expT = 1.0
    a = math.exp(g2T[0] - g2F[0]) * expT / expF
    b = g2T[1] - a * g2F[1]
    return a, b


def mat3f_inverse(K):
    """Eigen Matrix3f::inverse(): every entry = cofactor * (1 / det), float32 (call site TrackerAndScaler.cpp:139)"""
    K = _f(K)

    def cof(i, j):
        a, b = [r for r in range(3) if r != i], [c for c in range(3) if c != j]
        m = f32(K[a[0], b[0]] * K[a[1], b[1]]) - f32(K[a[0], b[1]] * K[a[1], b[0]])
        return f32(m) if (i + j) % 2 == 0 else f32(-m)

    c0 = [cof(0, 0), cof(1, 0), cof(2, 0)]  # cofactors of column 0
    det = f32(f32(f32(c0[0] * K[0, 0]) + f32(c0[1] * K[1, 0])) + f32(c0[2] * K[2, 0]))
    invdet = f32(f32(1.0) / det)
    out = np.zeros((3, 3), np.float32)
    for i in range(3):
        for j in range(3):
            out[i, j] = f32(cof(j, i) * invdet)  # inverse = adjugate / det, adjugate(i,j) = cofactor(j,i)
    return out


def mat3f_mul(A, B):
    """3x3 float product as a coefficient-wise lazy product evaluates it: ((a0 b0 + a1 b1) + a2 b2)"""
    A, B = _f(A), _f(B)
    out = np.zeros((3, 3), np.float32)
    for i in range(3):
        for j in range(3):
            out[i, j] = f32(f32(f32(A[i, 0] * B[0, j]) + f32(A[i, 1] * B[1, j])) + f32(A[i, 2] * B[2, j]))
    return out


def interp33(img, x, y):
    """getInterpolatedElement33 on an (h, w, 3) float32 image for float32 coordinate arrays"""
    ix, iy = x.astype(np.int32), y.astype(np.int32)
    dx, dy = x - ix.astype(np.float32), y - iy.astype(np.float32)
    dxdy = dx * dy
    w11, w01, w10, w00 = dxdy, dy - dxdy, dx - dxdy, f32(1) - dx - dy + dxdy
    t00, t10, t01, t11 = img[iy, ix], img[iy, ix + 1], img[iy + 1, ix], img[iy + 1, ix + 1]
    return ((w11[:, None] * t11 + w01[:, None] * t01) + w10[:, None] * t10) + w00[:, None] * t00


def seq_sum(terms):
    """sequential float32 sum in array order (what `float E = 0; for (...) E += term;` computes)"""
    terms = _f(terms)
    return f32(0) if len(terms) == 0 else np.cumsum(terms, dtype=np.float32)[-1]


def lane_accumulate(prod):
    """prod: (n,) float32 per-entry products, n % 4 == 0, in buffer order.  The reference's accumulators keep 4 SSE lanes
    (entry i goes to lane i % 4), add pack after pack, and after every 1001st pack move the lane sums to the "1k" buffer --
    which, holding num_in_1k = 1001 > 1000 packs, is forwarded to the "1m" buffer at once (ScaleAccumulator.h:85-105, as
    written); finish() forces a last shift and adds the four lanes left to right (:43-57)."""
    lanes = _f(prod).reshape(-1, 4)
    d1m = np.zeros(4, np.float32)
    for b0 in range(0, len(lanes), 1001):
        blk = lanes[b0:b0 + 1001]
        d = np.cumsum(blk, axis=0, dtype=np.float32)[-1]  # SSEData: += pack after pack
        d1k = d + np.zeros(4, np.float32)                  # shiftUp: 1k = data + 1k (1k was zero)
        d1m = d1k + d1m                                    # ... and straight on: 1m = 1k + 1m
    return f32(f32(f32(d1m[0] + d1m[1]) + d1m[2]) + d1m[3])


def ldlt_solve(A, b):
    """Eigen LDLT<MatrixXd, Lower>::solve: LDL^T with symmetric pivoting on the largest |diagonal| (first one on ties),
    D^-1 with Eigen's tolerance, in double"""
    A = np.array(A, np.float64)
    n = len(A)
    A = np.tril(A) + np.tril(A, -1).T  # only the lower triangle is read
    perm = list(range(n))
    for k in range(n):
        p = k + int(np.argmax(np.abs(np.diag(A)[k:])))
        if p != k:
            A[[k, p], :] = A[[p, k], :]
            A[:, [k, p]] = A[:, [p, k]]
            perm[k], perm[p] = perm[p], perm[k]
        d = A[k, k]
        if k == 0 and abs(d) == 0.0 and not np.any(A):
            return np.zeros(n)
        if abs(d) > 0.0:
            l = A[k + 1:, k] / d
            A[k + 1:, k + 1:] -= np.outer(l, A[k + 1:, k])
            A[k + 1:, k] = l
    L = np.tril(A, -1) + np.eye(n)
    D = np.diag(A).copy()
    y = np.array(b, np.float64)[perm]
    for i in range(n):  # L y' = y
        y[i] -= L[i, :i] @ y[:i]
    tol = 1.0 / np.finfo(np.float64).max
    y = np.where(np.abs(D) > tol, y / np.where(D == 0, 1.0, D), 0.0)
    for i in range(n - 1, -1, -1):  # L^T x' = y'
        y[i] -= L[i + 1:, i] @ y[i + 1:]
    x = np.zeros(n)
    x[perm] = y
    return x


def _pad4(a):
    """zero entries up to a multiple of 4 (they count in n: quirk Q3)"""
    a = _f(a)
    return np.concatenate([a, np.zeros((-len(a)) % 4, np.float32)])


def _residuals(img, wl, hl, u, v, new_id, Ku, Kv, col, huber, cutoff, aff, flow, flow_terms):
    """the second half of a residual pass, the same text in calcResPose :786-851, calcResScale :1102-1172 and PoseEstimator::calcRes
    (PoseEstimator.cpp:233-295): the bounds test, the gather, the residual with its Huber weight, the energy in point order, the
    buffers of the usable points and the Vec6"""
    with np.errstate(invalid="ignore"):
        inb = (Ku > 2) & (Kv > 2) & (Ku < f32(wl - 3)) & (Kv < f32(hl - 3)) & (new_id > 0)  # :786 / :1102
    idx = np.nonzero(inb)[0]
    hit = interp33(img, Ku[idx], Kv[idx])  # :790 / :1106
    fin = np.isfinite(hit[:, 0])
    idx, hit = idx[fin], hit[fin]
    refc = col[idx]
    if aff is not None:
        residual = hit[:, 0] - (f32(aff[0]) * refc + f32(aff[1]))  # :793
    else:
        residual = hit[:, 0] - refc  # :1109
    ar = np.abs(residual)
    with np.errstate(divide="ignore"):
        hw = np.where(ar < huber, f32(1), huber / ar).astype(np.float32)  # :794-795
    sat = ar > cutoff  # :797
    max_energy = f32(f32(f32(2) * huber) * cutoff) - f32(huber * huber)  # :726-728
    terms = np.where(sat, max_energy, ((hw * residual) * residual) * (f32(2) - hw)).astype(np.float32)  # :800 / :809
    E = seq_sum(terms)
    n_terms, n_sat = len(idx), int(sat.sum())
    keep = ~sat
    with np.errstate(invalid="ignore", divide="ignore"):
        rs = np.array([E, n_terms, float(flow[0]) / (float(flow[2]) + 0.1), 0.0, float(flow[1]) / (float(flow[2]) + 0.1),
                       f32(n_sat) / f32(n_terms) if n_terms else np.nan])  # :843-851
    buf = dict(idx=idx[keep], u=u[idx][keep], v=v[idx][keep], new_id=new_id[idx][keep], dx=hit[keep, 1], dy=hit[keep, 2],
               residual=residual[keep], hw=hw[keep], refc=refc[keep], flow_terms=flow_terms)
    return rs, buf


def _pose_vectors(B, fxl, fyl, a, b0):
    """the per-point vectors handed to Accumulator9::updateSSE_eighted -- the same text in calcGSSSEPose :658-678 and
    PoseEstimator::calcGSSSE (PoseEstimator.cpp:101-120) -- on the buffers B of a residual pass, padded to a multiple of 4"""
    pad = _pad4
    dx, dy = pad(B["dx"]) * fxl, pad(B["dy"]) * fyl  # :658-659
    u, v, idp = pad(B["u"]), pad(B["v"]), pad(B["new_id"])
    zero, one = f32(0), f32(1)
    J = [idp * dx, idp * dy, zero - idp * (u * dx + v * dy), zero - ((u * v) * dx + dy * (one + v * v)),
         (u * v) * dy + dx * (one + u * u), u * dy - v * dx, a * (b0 - pad(B["refc"])), np.full(len(u), -1, np.float32),
         pad(B["residual"])]  # :664-678
    return J, pad(B["hw"])


def _normal_equations(J, wgt, scales):
    """acc.finish(), 1 / n and the SCALE_* factors (:681-696 / PoseEstimator.cpp:123-138) of the nine vectors J and the weights"""
    n = len(wgt)
    Hf = np.zeros((9, 9), np.float32)
    for r in range(9):
        Jw = J[r] * wgt
        for c in range(r, 9):
            Hf[r, c] = Hf[c, r] = lane_accumulate(Jw * J[c]) if n else f32(0)
    with np.errstate(divide="ignore", invalid="ignore"):
        invn = f32(1.0) / f32(n)
        H = Hf[:8, :8].astype(np.float64) * float(invn)  # :682-683
        b = Hf[:8, 8].astype(np.float64) * float(invn)
    H = (H * scales[None, :]) * scales[:, None]  # :685-692
    return H, b * scales, n


class NumpyTracker:
    """TrackerAndScaler (TrackerAndScaler.h:34-137) in numpy; parameter names follow dsm_params / orc_params"""

    def __init__(self, w, h, nlevels, T_f1_f0, K1, huber=9.0, cutoff=20.0, scale_xi_rot=1.0, scale_xi_trans=0.5, scale_a=10.0,
                 scale_b=1000.0, mode_a=0.0, mode_b=0.0, lambda_limit=0.001, max_iterations=(10, 20, 50, 50, 50, 50)):
        self.nl = nlevels
        self.w = [w >> l for l in range(nlevels)]
        self.h = [h >> l for l in range(nlevels)]
        self.huber, self.cutoff0 = f32(huber), f32(cutoff)
        self.scales = np.array([scale_xi_rot] * 3 + [scale_xi_trans] * 3 + [scale_a, scale_b], np.float64)  # :541-545 / :685-696
        self.mode_a, self.mode_b, self.lambda_limit = f32(mode_a), f32(mode_b), f32(lambda_limit)
        self.max_iterations = list(max_iterations)
        self.T10 = np.array(T_f1_f0, np.float64).reshape(4, 4)  # tfm_f1_f0_ (:82-86)
        # camera 1 pyramid (:89-98): float storage, double arithmetic in the expressions with 0.5
        self.fx1, self.fy1, self.cx1, self.cy1 = ([f32(v)] for v in K1)
        for l in range(1, nlevels):
            self.fx1.append(f32(float(self.fx1[l - 1]) * 0.5))
            self.fy1.append(f32(float(self.fy1[l - 1]) * 0.5))
            self.cx1.append(f32((float(self.cx1[0]) + 0.5) / (1 << l) - 0.5))
            self.cy1.append(f32((float(self.cy1[0]) + 0.5) / (1 << l) - 0.5))
        self.res_evals = [0] * nlevels
        self.trace = []

    def make_k(self, fx, fy, cx, cy):  # :117-141
        self.fx, self.fy, self.cx, self.cy = [f32(fx)], [f32(fy)], [f32(cx)], [f32(cy)]
        for l in range(1, self.nl):
            self.fx.append(f32(float(self.fx[l - 1]) * 0.5))
            self.fy.append(f32(float(self.fy[l - 1]) * 0.5))
            self.cx.append(f32((float(self.cx[0]) + 0.5) / (1 << l) - 0.5))
            self.cy.append(f32((float(self.cy[0]) + 0.5) / (1 << l) - 0.5))
        self.Ki = [mat3f_inverse([[self.fx[l], 0, self.cx[l]], [0, self.fy[l], self.cy[l]], [0, 0, 1]]) for l in range(self.nl)]

    def set_ref(self, ref_a, ref_b, ref_exposure, pc_u, pc_v, pc_idepth, pc_color):  # the result of setCoarseTrackingRef :317-327
        self.ref_aff, self.ref_exposure = (float(ref_a), float(ref_b)), ref_exposure
        self.pc = [tuple(_f(a[l]) for a in (pc_u, pc_v, pc_idepth, pc_color)) for l in range(self.nl)]

    def scale_depth(self, s):  # :329-336
        self.pc = [(u, v, (idp / f32(s)).astype(np.float32), c) for u, v, idp, c in self.pc]

    def set_frame(self, slot, dIp, exposure):
        if slot == 0:
            self.new_dIp, self.new_exposure = [_f(a) for a in dIp], exposure
        else:
            self.right_dIp, self.right_exposure = [_f(a) for a in dIp], exposure

    # ---- calcResPose :699-852 / calcResScale :1007-1172: shared warp-and-gather core ----------------------------------
    def _warp(self, lvl, M, t, img, fx, fy, cx, cy, cutoff, aff, flow_Ki=None, flow_M=None):
        u_, v_, id_, col = self.pc[lvl]
        x, y = u_, v_
        wl, hl = self.w[lvl], self.h[lvl]
        pt = [((M[r, 0] * x + M[r, 1] * y) + M[r, 2]) + t[r] * id_ for r in range(3)]  # :747 / :1061
        with np.errstate(divide="ignore", invalid="ignore"):
            u, v = pt[0] / pt[2], pt[1] / pt[2]
            new_id = id_ / pt[2]
        Ku, Kv = fx * u + cx, fy * v + cy
        flow = np.zeros(3, np.float32)
        flow_terms = (np.zeros(0, np.float32), np.zeros(0, np.float32))
        if lvl == 0 and flow_Ki is not None:  # :754-784 / :1070-1100: every 32nd template index
            s = slice(0, None, 32)
            xs, ys, ids = x[s], y[s], id_[s]
            kx = [(flow_Ki[r, 0] * xs + flow_Ki[r, 1] * ys) + flow_Ki[r, 2] for r in range(3)]
            rx = [(flow_M[r, 0] * xs + flow_M[r, 1] * ys) + flow_M[r, 2] for r in range(3)]
            tid = [t[r] * ids for r in range(3)]

            def proj(p):
                return fx * (p[0] / p[2]) + cx, fy * (p[1] / p[2]) + cy

            with np.errstate(divide="ignore", invalid="ignore"):
                KuT, KvT = proj([kx[r] + tid[r] for r in range(3)])
                KuT2, KvT2 = proj([kx[r] - tid[r] for r in range(3)])
                Ku3, Kv3 = proj([rx[r] - tid[r] for r in range(3)])
            sq = lambda a, b: (a - xs) * (a - xs) + (b - ys) * (b - ys)
            flow_terms = (np.stack([sq(KuT, KvT), sq(KuT2, KvT2)], 1).ravel(), np.stack([sq(Ku[s], Kv[s]), sq(Ku3, Kv3)], 1).ravel())
            flow[0] = seq_sum(flow_terms[0])
            flow[1] = seq_sum(flow_terms[1])
            flow[2] = seq_sum(np.full(len(xs), 2, np.float32))
        self.res_evals[lvl] += 1
        return _residuals(img, wl, hl, u, v, new_id, Ku, Kv, col, self.huber, cutoff, aff, flow, flow_terms)

    @staticmethod
    def _pad4(a):  # :824-834: zero entries up to a multiple of 4 (they count in n: quirk Q3)
        return _pad4(a)

    def calc_res_pose(self, lvl, T, aff, cutoff):
        R = T[:3, :3].astype(np.float32)
        RKi = mat3f_mul(R, self.Ki[lvl])  # :715
        t = T[:3, 3].astype(np.float32)   # :716
        a, b = aff_from_to(self.ref_exposure, self.new_exposure, self.ref_aff, aff)  # :717-720
        rs, buf = self._warp(lvl, RKi, t, self.new_dIp[lvl], self.fx[lvl], self.fy[lvl], self.cx[lvl], self.cy[lvl], f32(cutoff),
                             (a, b), self.Ki[lvl], RKi)
        self.pose_buf = buf
        return rs

    def pose_jacobian(self, lvl, aff):
        """calcGSSSEPose's per-point vectors (:658-678) on the buffers of the last calc_res_pose, padded with zero entries to a
        multiple of 4 (quirk Q3): J = the 8 tangent entries and the residual (9 float32 arrays), and the Huber weights"""
        a = f32(aff_from_to(self.ref_exposure, self.new_exposure, self.ref_aff, aff)[0])
        return _pose_vectors(self.pose_buf, self.fx[lvl], self.fy[lvl], a, f32(self.ref_aff[1]))

    def calc_gs_pose(self, lvl, aff):  # calcGSSSEPose :640-697
        return _normal_equations(*self.pose_jacobian(lvl, aff), self.scales)

    def calc_res_scale(self, lvl, scale, cutoff):
        R10 = self.T10[:3, :3].astype(np.float32)
        M = mat3f_mul(R10, self.Ki[lvl])  # :1022-1023
        t = self.T10[:3, 3].astype(np.float32)
        S = (f32(scale) * M).astype(np.float32)  # `scale * rot_f1_f0_K0_i` (:1061)
        rs, buf = self._warp(lvl, S, t, self.right_dIp[lvl], self.fx1[lvl], self.fy1[lvl], self.cx1[lvl], self.cy1[lvl], f32(cutoff),
                             None, (f32(scale) * self.Ki[lvl]).astype(np.float32), S)
        u_, v_, id_, _ = self.pc[lvl]
        i = buf["idx"]
        with np.errstate(divide="ignore", invalid="ignore"):
            buf["rx"] = [(((M[r, 0] * u_[i] + M[r, 1] * v_[i]) + M[r, 2]) / id_[i]).astype(np.float32) for r in range(3)]  # :1068
        self.scale_buf = buf
        return rs

    def scale_jacobian(self, lvl, scale):
        """calcGSSSEScale's per-point values (:983-999) on the buffers of the last calc_res_scale, padded with zero entries to a
        multiple of 4 (quirk Q3): J0 (d residual / d scale), J1 (the residual) and the Huber weights"""
        B = self.scale_buf
        pad = self._pad4
        t = self.T10[:3, 3].astype(np.float32)
        tx, ty, tz, s, one = t[0], t[1], t[2], f32(scale), f32(1)
        dxfx, dyfy = pad(B["dx"]) * self.fx1[lvl], pad(B["dy"]) * self.fy1[lvl]
        rx1, rx2, rx3 = (pad(a) for a in B["rx"])
        deno_sqrt = s * rx3 + tz
        with np.errstate(divide="ignore", invalid="ignore"):
            deno = one / (deno_sqrt * deno_sqrt)
            xno, yno = rx1 * tz - rx3 * tx, rx2 * tz - rx3 * ty
            J0 = dxfx * (deno * xno) + dyfy * (deno * yno)
        return J0, pad(B["residual"]), pad(B["hw"])

    def calc_gs_scale(self, lvl, scale):  # calcGSSSEScale :966-1005
        J0, J1, w = self.scale_jacobian(lvl, scale)
        n = len(J0)
        J0w = J0 * w
        h00, h01 = (lane_accumulate(J0w * J0), lane_accumulate(J0w * J1)) if n else (f32(0), f32(0))
        with np.errstate(divide="ignore", invalid="ignore"):
            invn = f32(1.0) / f32(n)
            return f32(h00 * invn), f32(h01 * invn), n  # :1003-1004

    # ---- trackNewestCoarse :451-638 -----------------------------------------------------------------------------------
    def track(self, pose, aff, coarsest, min_res=None):
        T = pose_to_matrix(np.asarray(pose, np.float64))
        aff = (float(aff[0]), float(aff[1]))
        min_res = [np.nan] * 6 if min_res is None else list(min_res)
        last = [np.nan] * 6  # :459
        flow = [1000.0] * 3  # :460
        have_repeated = False
        self.res_evals = [0] * self.nl
        self.trace = []
        lvl = coarsest
        while lvl >= 0:
            rep = f32(1)
            res_old = self.calc_res_pose(lvl, T, aff, self.cutoff0 * rep)  # :475
            while res_old[5] > 0.6 and rep < 50:  # :477-485
                rep = f32(rep * 2)
                res_old = self.calc_res_pose(lvl, T, aff, self.cutoff0 * rep)
            H, b, _ = self.calc_gs_pose(lvl, aff)  # :487
            lam = f32(0.01)
            for _ in range(self.max_iterations[lvl]):  # :505
                Hl = H.copy()
                Hl[np.diag_indices(8)] *= (1 + float(lam))  # :506-508
                inc = ldlt_solve(Hl, -b)  # :509
                if self.mode_a < 0 and self.mode_b < 0:  # :511-515
                    inc = np.concatenate([ldlt_solve(Hl[:6, :6], -b[:6]), [0, 0]])
                if not (self.mode_a < 0) and self.mode_b < 0:  # :516-520
                    inc = np.concatenate([ldlt_solve(Hl[:7, :7], -b[:7]), [0]])
                if self.mode_a < 0 and not (self.mode_b < 0):  # :521-534
                    Hs, bs = Hl.copy(), b.copy()
                    Hs[:, 6] = Hs[:, 7]
                    Hs[6, :] = Hs[7, :]
                    bs[6] = bs[7]
                    st = ldlt_solve(Hs[:7, :7], -bs[:7])
                    inc = np.concatenate([st[:6], [0, st[6]]])
                extrap = f32(1)
                if lam < self.lambda_limit:  # :536-539
                    extrap = f32(math.sqrt(math.sqrt(float(f32(self.lambda_limit / lam)))))
                inc = inc * float(extrap)
                inc_scaled = inc * self.scales  # :541-545
                if not np.isfinite(inc_scaled.sum()):
                    inc_scaled[:] = 0  # :547-548
                T_new = se3_exp(inc_scaled[:6]) @ T  # :550-551
                aff_new = (aff[0] + inc_scaled[6], aff[1] + inc_scaled[7])  # :552-554
                res_new = self.calc_res_pose(lvl, T_new, aff_new, self.cutoff0 * rep)  # :556
                accept = (res_new[0] / res_new[1]) < (res_old[0] / res_old[1])  # :559
                self.trace.append((lvl, bool(accept)))
                if accept:  # :576-581
                    H, b, _ = self.calc_gs_pose(lvl, aff_new)
                    res_old, aff, T = res_new, aff_new, T_new
                    lam = f32(lam * f32(0.5))
                else:  # :583-585
                    lam = f32(lam * f32(4))
                    if lam < self.lambda_limit:
                        lam = self.lambda_limit
                if not (np.linalg.norm(inc) > 1e-3):  # :588
                    break
            last[lvl] = float(np.sqrt(f32(res_old[0] / res_old[1])))  # :596
            flow = list(res_old[2:5])  # :597
            if last[lvl] > 1.5 * min_res[lvl]:  # :598
                return False, matrix_to_pose(T), aff, last, flow
            if rep > 1 and not have_repeated:  # :601-604
                lvl += 1
                have_repeated = True
            lvl -= 1
        good = True
        if (self.mode_a != 0 and abs(f32(aff[0])) > 1.2) or (self.mode_b != 0 and abs(f32(aff[1])) > 200):  # :615-617
            good = False
        rel = aff_from_to(self.ref_exposure, self.new_exposure, self.ref_aff, aff)  # :619-622
        if (self.mode_a == 0 and abs(math.log(float(f32(rel[0])))) > 1.5) or (self.mode_b == 0 and abs(f32(rel[1])) > 200):  # :624-626
            good = False
        return good, matrix_to_pose(T), aff, last, flow

    # ---- optimizeScale :854-964 ---------------------------------------------------------------------------------------
    def optimize_scale(self, scale, coarsest):
        cur = f32(scale)
        last = [np.nan] * 6
        have_repeated = False
        self.res_evals = [0] * self.nl
        self.trace = []
        lvl = coarsest
        while lvl >= 0:
            rep = f32(1)
            res_old = self.calc_res_scale(lvl, cur, self.cutoff0 * rep)  # :873
            while res_old[5] > 0.6 and rep < 50:  # :875-883
                rep = f32(rep * 2)
                res_old = self.calc_res_scale(lvl, cur, self.cutoff0 * rep)
            H, b, _ = self.calc_gs_scale(lvl, cur)  # :885
            lam = f32(0.01)
            for _ in range(self.max_iterations[lvl]):
                Hl = f32(H * f32(1 + lam))  # :897-898
                with np.errstate(divide="ignore", invalid="ignore"):
                    inc = f32(-b / Hl)  # :899
                extrap = f32(1)
                if lam < self.lambda_limit:  # :901-904
                    extrap = f32(math.sqrt(math.sqrt(float(f32(self.lambda_limit / lam)))))
                inc = f32(inc * extrap)
                if not np.isfinite(inc) or abs(inc) > cur:  # :906-907
                    inc = f32(0)
                new = f32(cur + inc)  # :909
                res_new = self.calc_res_scale(lvl, new, self.cutoff0 * rep)  # :911
                accept = (res_new[0] / res_new[1]) < (res_old[0] / res_old[1])  # :914
                self.trace.append((lvl, bool(accept)))
                if accept:  # :926-930
                    H, b, _ = self.calc_gs_scale(lvl, new)
                    res_old, cur = res_new, new
                    lam = f32(lam * f32(0.5))
                else:  # :931-935
                    lam = f32(lam * f32(4))
                    if lam < self.lambda_limit:
                        lam = self.lambda_limit
                if not (inc > 1e-3):  # :937 -- SIGNED (quirk Q7)
                    break
            last[lvl] = float(np.sqrt(f32(res_old[0] / res_old[1])))  # :945
            if rep > 1 and not have_repeated:  # :947-950
                lvl += 1
                have_repeated = True
            lvl -= 1
        return last[0], float(cur)  # :954, :963


class NumpyPoseEstimator:
    """PoseEstimator (src/loop_closure/pose_estimation/PoseEstimator.h:34-83) in numpy: one calcRes (PoseEstimator.cpp:141-296) and
    calcGSSSE (:84-139) on loaded inputs.  Written from that text; what it shares with TrackerAndScaler.cpp word for word (the bounds
    test onwards, the vectors of the accumulator) is shared with NumpyTracker above."""

    def __init__(self, w, h, nlevels, huber=9.0, scale_xi_rot=1.0, scale_xi_trans=0.5, scale_a=10.0, scale_b=1000.0):
        self.nl = nlevels
        self.w = [w >> l for l in range(nlevels)]
        self.h = [h >> l for l in range(nlevels)]
        self.huber = f32(huber)
        self.scales = np.array([scale_xi_rot] * 3 + [scale_xi_trans] * 3 + [scale_a, scale_b], np.float64)  # :127-138
        self.ref_aff = (0.0, 0.0)  # ref_aff_g2l_ = AffLight(0, 0), :317

    def load(self, xyz, colors, ref_ab_exposure, new_dIp, new_ab_exposure, new_cam):
        """the head of estimate: makeK(new_cam) :62-82 / :306, pts_ :183-185, the exposures and the new frame"""
        fx, fy, cx, cy = new_cam
        self.fx, self.fy, self.cx, self.cy = [f32(fx)], [f32(fy)], [f32(cx)], [f32(cy)]
        for l in range(1, self.nl):  # :72-77: float storage, double arithmetic in the expressions with 0.5
            self.fx.append(f32(float(self.fx[l - 1]) * 0.5))
            self.fy.append(f32(float(self.fy[l - 1]) * 0.5))
            self.cx.append(f32((float(self.cx[0]) + 0.5) / (1 << l) - 0.5))
            self.cy.append(f32((float(self.cy[0]) + 0.5) / (1 << l) - 0.5))
        with np.errstate(over="ignore"):
            self.xyz = np.asarray(xyz, np.float64).reshape(-1, 3).astype(np.float32)  # `float x = pts_[i].first(0)` :184-186
        self.colors = [_f(c) for c in colors]  # pts_[i].second[lvl]
        self.new_dIp = [_f(a) for a in new_dIp]
        self.ref_exposure, self.new_exposure = ref_ab_exposure, new_ab_exposure

    def _aff(self, aff):
        return aff_from_to(self.ref_exposure, self.new_exposure, self.ref_aff, aff)  # :158-161 / :91-92

    def calc_res(self, lvl, T, aff, cutoff):
        R = T[:3, :3].astype(np.float32)  # :156
        t = T[:3, 3].astype(np.float32)   # :157
        fx, fy, cx, cy = self.fx[lvl], self.fy[lvl], self.cx[lvl], self.cy[lvl]
        x, y, z = self.xyz[:, 0], self.xyz[:, 1], self.xyz[:, 2]
        one = f32(1)

        def proj(p):
            return fx * (p[0] / p[2]) + cx, fy * (p[1] / p[2]) + cy

        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            Ku0, Kv0 = proj((x, y, z))  # :187-190
            pt = [((R[r, 0] * x + R[r, 1] * y) + R[r, 2] * z) + t[r] for r in range(3)]  # :192
            u, v = pt[0] / pt[2], pt[1] / pt[2]
            Ku, Kv = fx * u + cx, fy * v + cy
            new_id = one / pt[2]  # :197
            flow = np.zeros(3, np.float32)
            flow_terms = (np.zeros(0, np.float32), np.zeros(0, np.float32))
            if lvl == 0:  # :199-231: every 32nd point
                s = slice(0, None, 32)
                xs, ys, k0, l0 = x[s], y[s], Ku0[s], Kv0[s]
                KuT, KvT = proj((xs + t[0], ys + t[1], one + t[2]))    # Vec3f(x, y, 1) + t
                KuT2, KvT2 = proj((xs - t[0], ys - t[1], one - t[2]))  # Vec3f(x, y, 1) - t
                Ku3, Kv3 = proj([((R[r, 0] * xs + R[r, 1] * ys) + R[r, 2]) - t[r] for r in range(3)])  # R * Vec3f(x, y, 1) - t
                sq = lambda a, b: (a - k0) * (a - k0) + (b - l0) * (b - l0)
                flow_terms = (np.stack([sq(KuT, KvT), sq(KuT2, KvT2)], 1).ravel(), np.stack([sq(Ku[s], Kv[s]), sq(Ku3, Kv3)], 1).ravel())
                flow[0] = seq_sum(flow_terms[0])
                flow[1] = seq_sum(flow_terms[1])
                flow[2] = seq_sum(np.full(len(xs), 2, np.float32))
        self.warp = dict(pt2=pt[2], Ku=Ku, Kv=Kv)  # (for tests that place points by their warped depth)
        rs, self.buf = _residuals(self.new_dIp[lvl], self.w[lvl], self.h[lvl], u, v, new_id, Ku, Kv, self.colors[lvl], self.huber,
                                  f32(cutoff), self._aff(aff), flow, flow_terms)
        return rs

    def jacobian(self, lvl, aff):
        """calcGSSSE's nine per-point vectors (:101-120) on the buffers of the last calc_res, padded to a multiple of 4, and the
        weights; b0 = ref_aff_g2l_.b = 0 (:90)"""
        return _pose_vectors(self.buf, self.fx[lvl], self.fy[lvl], f32(self._aff(aff)[0]), f32(self.ref_aff[1]))

    def calc_gs(self, lvl, aff):
        return _normal_equations(*self.jacobian(lvl, aff), self.scales)
