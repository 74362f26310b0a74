"""The binary case files of the window-optimisation family: what the demos under direct_stereo_slam_amd/host/ and the stand-alone CPU
programs under tools/ read.  This module writes them; direct_stereo_slam_amd/host/window_case.hpp reads them.  The two are the
definition of the format: one writer per section here, one reader per section there, in the same order.

All values are in native byte order, int32 / float32 / float64 as named.  With nf frames, n points, nr residuals, N = 4 + 8 nf:

  window prefix    int32 w, h; float32 cam[4], cam_inv[2]; int32 nf, fix_linearization; int32 frame_ids[nf]; nf planes of w h float32;
                   nf nf precalc rows of 27 float32 (pre_RTll_0[9], pre_tTll_0[3], pre_KRKiTll[9], pre_KtTll[3], pre_aff_mode[2],
                   pre_b0_mode), [host][target]; float32 frame_energy_th[nf]; int32 n; n point records of 21 words (int32 host, float32
                   u, v, idepth_scaled, idepth_zero_scaled, color[8], weights[8]); int32 nr; nr residual records of 5 words (int32
                   point, target, state_in, float32 energy_in, int32 is_new)
  hessian tail     float64 ad_host[nf nf 64], ad_target[nf nf 64]; per point `width` float32: (prior, delta) for width 2, (prior,
                   delta, hdd_lin, bd_lin, hcd_lin[4]) for width 8; for width 8 then int32 shift_prior_to_zero
  solve tail       float64 H_L[N N], b_L[N]; solve form: float64 H_M[N N], b_M[N], delta_x[N]; step form: int32 flag and, if set,
                   float64 H_M[N N], b_M[N] (no delta_x: the call forms it); then float64 lambda; int32 n_null; float64
                   null_basis[N n_null], null_pinv[n_null N]
  step tail        float64 world_to_cam_eval[nf 7], state_zero[nf 8], state_backup[nf 8], frame_step[nf 8], calib_zero[4],
                   calib_backup[4], calib_step[4]; float32 idepth_backup[n], idepth_step[n], exposure[nf], stepfac[5]; int32 flag and, if
                   set, float64 state_prior[N], state_prior_zero[N]
  finish tail      int32 n_good_residuals_in[n]; float32 max_rel_baseline_in[n]; int32 last_res[n 2]; uint8 last_state_in[n 2]
  marginalize tail uint8 flagged[nf]; int32 n_good_residuals[n]; uint8 last_state[n 2]; float32 idepth_hessian[n], ad_ht_delta[nf nf 8],
                   c_delta[4]; int32 flag and, if set, float64 H_M[N N], b_M[N]; int32 nm; int32 marg_frames[nm]; float64
                   frame_prior[nm 8], frame_delta_prior[nm 8]
  pose records     twice: float64 world_to_cam_eval[nf 7], state_zero[nf 8]; float32 exposure[nf]

  file kind     sections
  window        prefix
  hessian       prefix, hessian tail (8)
  solve         prefix, hessian tail (8), solve tail (solve form)
  nullspace     prefix, hessian tail (8), solve tail (solve form), pose records
  step          prefix, hessian tail (8), solve tail (step form), step tail; cam, cam_inv, the precalc rows and the points' two depths
                are zeros: the call forms them
  finish        the step file with frame_step, calib_step, idepth_step and stepfac as zeros, then the finish tail
  marginalize   prefix, hessian tail (2), marginalize tail

tools/nullspace_host_standalone.cpp reads a file of its own, a nullspace job: int32 nf, given; float64 world_to_cam_eval[nf 7],
state_zero[nf 8]; float32 exposure[nf]; if given, float64 frame_null_in[nf 42].
"""
import struct

import numpy as np

import _linearize_ref as R

f32, f64 = np.float32, np.float64


def fnv1a(b, h=1469598103934665603):
    for x in b:
        h = ((h ^ x) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def _d(job, *keys):
    return b"".join(np.ascontiguousarray(job[k], f64).tobytes() for k in keys)


def _s(job, *keys):
    return b"".join(np.ascontiguousarray(job[k], f32).tobytes() for k in keys)


def _flagged(job, *keys):
    """int32 flag, then the float64 arrays if the first of them is there"""
    there = job.get(keys[0]) is not None
    return struct.pack("i", int(there)) + (_d(job, *keys) if there else b"")


def window_prefix(w, h, job, frames):
    nf, n, nr = len(frames), len(job["host"]), len(job["point"])
    pre = np.concatenate([np.asarray(job[k], f32).reshape(nf * nf, m) for k, m in R.PRE], axis=1)
    prec = np.zeros((n, 21), f32)
    prec[:, 0] = np.asarray(job["host"], np.int32).view(f32)
    for k, name in enumerate(("u", "v", "idepth_scaled", "idepth_zero_scaled")):
        prec[:, 1 + k] = job[name]
    prec[:, 5:13], prec[:, 13:21] = job["color"], job["weights"]
    rrec = np.zeros((nr, 5), np.int32)
    rrec[:, 0], rrec[:, 1], rrec[:, 2], rrec[:, 4] = job["point"], job["target"], job["state_in"], job["is_new"]
    rrec[:, 3] = np.asarray(job["energy_in"], f32).view(np.int32)
    return (struct.pack("ii", w, h) + np.array(list(job["cam"]) + list(job["cam_inv"]), f32).tobytes()
            + struct.pack("ii", nf, int(job["fix_linearization"])) + np.asarray(job["frame_ids"], np.int32).tobytes()
            + b"".join(np.ascontiguousarray(fr, f32).tobytes() for fr in frames) + pre.tobytes() + _s(job, "frame_energy_th")
            + struct.pack("i", n) + prec.tobytes() + struct.pack("i", nr) + rrec.tobytes())


def hessian_tail(job, width):
    """width 8 or 2; a per-point array the job does not hold is written as zeros"""
    m = len(job["host"])
    columns = (("prior", 1), ("delta", 1), ("hdd_lin", 1), ("bd_lin", 1), ("hcd_lin", 4))[:5 if width == 8 else 2]
    pin = np.concatenate([np.asarray(job[k] if job.get(k) is not None else np.zeros(m * c), f32).reshape(m, c) for k, c in columns], axis=1)
    assert pin.shape == (m, width)
    return _d(job, "ad_host", "ad_target") + np.ascontiguousarray(pin, f32).tobytes() + (struct.pack("i", int(job["shift_prior_to_zero"])) if width == 8 else b"")


def solve_tail(job, step_form):
    nn = int(job.get("n_null", 0))
    prior = _flagged(job, "H_M", "b_M") if step_form else _d(job, "H_M", "b_M", "delta_x")
    return _d(job, "H_L", "b_L") + prior + struct.pack("d", float(job["lambda"])) + struct.pack("i", nn) + (_d(job, "null_basis", "null_pinv") if nn else b"")


def step_tail(job):
    if job.get("state_prior") is not None:
        assert len(job["state_prior"]) == 4 + 8 * len(job["frame_ids"])
    return (_d(job, "world_to_cam_eval", "state_zero", "state_backup", "frame_step", "calib_zero", "calib_backup", "calib_step")
            + _s(job, "idepth_backup", "idepth_step", "exposure", "stepfac") + _flagged(job, "state_prior", "state_prior_zero"))


def finish_tail(job):
    return (np.ascontiguousarray(job["n_good_residuals_in"], np.int32).tobytes() + _s(job, "max_rel_baseline_in")
            + np.ascontiguousarray(job["last_res"], np.int32).tobytes() + np.ascontiguousarray(job["last_state_in"], np.uint8).tobytes())


def marginalize_tail(job):
    marg = np.asarray(job.get("marg_frames", ()), np.int32).reshape(-1)
    return (np.ascontiguousarray(job["flagged"], np.uint8).tobytes() + np.ascontiguousarray(job["n_good_residuals"], np.int32).tobytes()
            + np.ascontiguousarray(job["last_state"], np.uint8).tobytes() + _s(job, "idepth_hessian", "ad_ht_delta", "c_delta")
            + _flagged(job, "H_M", "b_M") + struct.pack("i", len(marg)) + marg.tobytes() + _d(job, "frame_prior", "frame_delta_prior"))


def pose_records(poses):
    return b"".join(_d(p, "world_to_cam_eval", "state_zero") + _s(p, "exposure") for p in poses)


def _write(path, *sections):
    with open(path, "wb") as f:
        f.write(b"".join(sections))


def write_window(path, w, h, job, frames):
    _write(path, window_prefix(w, h, job, frames))


def write_hessian(path, w, h, job, frames):
    _write(path, window_prefix(w, h, job, frames), hessian_tail(job, 8))


def write_solve(path, w, h, job, frames):
    _write(path, window_prefix(w, h, job, frames), hessian_tail(job, 8), solve_tail(job, False))


def write_nullspace(path, w, h, job, frames, poses):
    _write(path, window_prefix(w, h, job, frames), hessian_tail(job, 8), solve_tail(job, False), pose_records(poses))


def write_step(path, w, h, job, frames, *tails):
    n, m = len(job["frame_ids"]), len(job["host"])
    formed = dict(job, cam=(0, 0, 0, 0), cam_inv=(0, 0), idepth_scaled=np.zeros(m, f32), idepth_zero_scaled=np.zeros(m, f32),
                  **{k: np.zeros((n, n, width), f32) for k, width in R.PRE})
    _write(path, window_prefix(w, h, formed, frames), hessian_tail(job, 8), solve_tail(job, True), step_tail(job), *tails)


def write_finish(path, w, h, job, frames):
    n, m = len(job["frame_ids"]), len(job["host"])
    step = dict(job, frame_step=np.zeros((n, 8)), calib_step=np.zeros(4), idepth_step=np.zeros(m, f32), stepfac=np.zeros(5, f32),
                **{"lambda": job.get("lambda", 1e-5)})
    write_step(path, w, h, step, frames, finish_tail(job))


def write_marginalize(path, w, h, job, frames):
    _write(path, window_prefix(w, h, job, frames), hessian_tail(job, 2), marginalize_tail(job))


def write_nullspace_job(path, job):
    ev = np.ascontiguousarray(job["world_to_cam_eval"], f64).reshape(-1, 7)
    fn = job.get("frame_null_in")
    _write(path, struct.pack("ii", len(ev), 0 if fn is None else 1), ev.tobytes(), _d(job, "state_zero"), _s(job, "exposure"),
           b"" if fn is None else _d(job, "frame_null_in"))
