"""Python host-side mirror of the reference's `dso::TrackerAndScaler` public surface
(src/scale_optimization/TrackerAndScaler.h:38-64) on top of the C ABI.  Used by tests/ and
bench.py; the C++ adaptor for the ROS node is direct_stereo_slam_amd/host/TrackerAndScaler.hpp.

Method names follow the reference: makeK, setCoarseTrackingRef (takes the template lists that
makeCoarseDepthL0 produced), scaleCoarseDepthL0, trackNewestCoarse, optimizeScale; the public
output fields refFrameID / lastFlowIndicators keep their names.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import (MAX_LEVELS, LmProposeIn, LmProposeOut, LmStepState, Params, Stats, TickListCfg, TickModeCtl, TickPending, TickResult, TickSeg,
                   TickSegCtl, TickSlot, TickSlotOut, c_double_p, c_float_p, c_int_p, check)

# numpy record layouts of dsm_lm_propose_in / dsm_lm_propose_out (the field names of _lib.LmProposeIn / LmProposeOut)
LM_PROPOSE_IN = np.dtype(LmProposeIn)
LM_PROPOSE_OUT = np.dtype(LmProposeOut)
LM_STEP_STATE = np.dtype(LmStepState)  # dsm_lm_step_state
# dsm_diag_tick_*: dsm_tick_slot / _slot_out / _pending / _result
TICK_SLOT, TICK_SLOT_OUT, TICK_PENDING, TICK_RESULT = np.dtype(TickSlot), np.dtype(TickSlotOut), np.dtype(TickPending), np.dtype(TickResult)


def _tick_call(fn, head_args, n, list_cfg, ctl, pending):
    """the common tail of dsm_diag_tick_stage / _step: asks for the length of the item allocation, runs, returns a dict of everything read back"""
    lc = TickListCfg(**list_cfg)
    mc = TickModeCtl(pending_head=ctl["pending_head"], pending_count=ctl["pending_count"], retired=ctl["retired"], ring=ctl["ring"])
    pending = np.ascontiguousarray(pending if pending is not None else np.zeros(0, TICK_PENDING), TICK_PENDING)
    npend, ring = len(pending), int(ctl["ring"])
    pend_p = pending.ctypes.data_as(C.POINTER(TickPending)) if npend else None
    length, sbytes = C.c_int(0), C.c_int(0)

    def call(*outs):
        check(fn(*head_args(C.byref(lc), C.byref(mc), npend, pend_p), *outs))

    call(None, C.byref(length), None, None, None, None, None, None, C.byref(sbytes), None)
    items = np.zeros(length.value, np.uint32)
    seg, mc_out = TickSegCtl(), TickModeCtl()
    results = np.zeros(max(ring, 0), TICK_RESULT)
    slot_out, state_out = np.zeros(n, TICK_SLOT_OUT), np.zeros(n, LM_STEP_STATE)
    raw, start_raw = np.zeros((n, sbytes.value), np.uint8), np.zeros((npend, sbytes.value), np.uint8)
    ub = C.POINTER(C.c_ubyte)
    call(items.ctypes.data_as(C.POINTER(C.c_uint)), C.byref(length), C.byref(seg), C.byref(mc_out), results.ctypes.data_as(C.POINTER(TickResult)),
         slot_out.ctypes.data_as(C.POINTER(TickSlotOut)), state_out.ctypes.data_as(C.POINTER(LmStepState)), raw.ctypes.data_as(ub), C.byref(sbytes),
         start_raw.ctypes.data_as(ub) if npend else None)
    return dict(items=items, seg=seg, ctl=mc_out, results=results, slot_out=slot_out, state_out=state_out, state_raw=raw, start_raw=start_raw)


def _fp(a):
    return a.ctypes.data_as(c_float_p)


def _dp(a):
    return a.ctypes.data_as(c_double_p)


def _ptr_array(arrs):
    arr = (c_float_p * len(arrs))()
    for i, a in enumerate(arrs):
        assert a.dtype == np.float32 and a.flags["C_CONTIGUOUS"]
        arr[i] = _fp(a)
    return arr


def pinned_array(shape, dtype=np.float32):
    """numpy array backed by pinned host memory (dsm_host_alloc): dsm_tracker_upload_image copies from it by DMA.
    The memory is released when the array is garbage collected."""
    L = _lib.load()
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    p = C.c_void_p()
    check(L.dsm_host_alloc(n, C.byref(p)))
    buf = (C.c_char * n).from_address(p.value)
    arr = np.frombuffer(buf, dtype=dtype).reshape(shape)

    class _Owner:
        def __init__(self, ptr):
            self.ptr = ptr

        def __del__(self):
            try:
                L.dsm_host_free(self.ptr)
            except Exception:
                pass

    owner = _Owner(p)
    out = arr.view()
    _PINNED_OWNERS[id(out)] = (owner, buf)
    import weakref

    weakref.finalize(out, _PINNED_OWNERS.pop, id(out), None)
    return out


_PINNED_OWNERS = {}


def default_params():
    p = Params()
    check(_lib.load().dsm_params_default_sized(C.byref(p), C.sizeof(Params)))  # (a layout drift of this mirror fails here)
    return p


class Context:
    """device + stream + batch workspaces (dsm_context)"""

    def __init__(self, device=0):
        self.L = _lib.load()
        h = C.c_void_p()
        check(self.L.dsm_context_create(device, C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.dsm_context_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def sync(self):
        check(self.L.dsm_context_sync(self.h))

    def diagTickReserve(self, segs, running, head, count):
        """tick_reserve_kernel alone (dsm_diag_tick_reserve).  segs: (mode, i0, ns) triples; running: per slot, nonzero = a running
        problem; head / count: the two kinds' pending_head / pending_count.  Returns (admit_idx [nslots] int64, heads [2], ctl_intact)"""
        sg = (TickSeg * max(len(segs), 1))(*[TickSeg(*s) for s in segs])
        running = np.ascontiguousarray(running, np.uint8)
        hd, cn = (C.c_longlong * 2)(*head), (C.c_longlong * 2)(*count)
        idx, hout, intact = np.zeros(len(running), np.int64), (C.c_longlong * 2)(), C.c_int()
        check(self.L.dsm_diag_tick_reserve(self.h, len(segs), sg, len(running), running.ctypes.data_as(C.POINTER(C.c_ubyte)), hd, cn,
                                           idx.ctypes.data_as(C.POINTER(C.c_longlong)), hout, C.byref(intact)))
        return idx, [int(hout[0]), int(hout[1])], bool(intact.value)

    def set_timing(self, on):
        check(self.L.dsm_context_set_timing(self.h, int(on)))

    def set_streams(self, n):
        check(self.L.dsm_context_set_streams(self.h, int(n)))

    def stream_queues(self):
        """(group streams in use, how many of them share a hardware queue with another group): dsm_context_stream_queues"""
        a, b = C.c_int(), C.c_int()
        check(self.L.dsm_context_stream_queues(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def stats(self):
        s = Stats()
        check(self.L.dsm_context_get_stats(self.h, C.byref(s)))
        return s

    def stats2(self):
        """statistics of the scale segment of the last track_and_scale_batch"""
        s = Stats()
        check(self.L.dsm_context_get_stats2(self.h, C.byref(s)))
        return s

    def read_bandwidth(self, nbytes=1 << 30, iters=10):
        """measurement aid: read-only streaming bandwidth in GB/s"""
        g = C.c_double()
        check(self.L.dsm_diag_read_bandwidth(self.h, nbytes, iters, C.byref(g)))
        return g.value

    def xwg_litmus(self, pairs=128, iters=80000):
        """(hand-offs, stale words) of the cross-workgroup hand-off litmus (dsm_diag_xwg_litmus)"""
        n, bad = C.c_longlong(), C.c_longlong()
        check(self.L.dsm_diag_xwg_litmus(self.h, pairs, iters, C.byref(n), C.byref(bad)))
        return n.value, bad.value

    def read_bandwidth_chunked(self, nbytes=1 << 30, chunk_bytes=112 * 1024, iters=10):
        """measurement aid: same, one contiguous chunk per workgroup (the eval kernels' access pattern)"""
        g = C.c_double()
        check(self.L.dsm_diag_read_bandwidth_chunked(self.h, nbytes, chunk_bytes, iters, C.byref(g)))
        return g.value

    # ---- batched forms -----------------------------------------------------------------
    def track_batch(self, trackers, poses, affs, coarsest, min_res=None):
        n = len(trackers)
        hs = (C.c_void_p * n)(*[t.h for t in trackers])
        poses = np.ascontiguousarray(poses, np.float64).reshape(n, 7).copy()
        affs = np.ascontiguousarray(affs, np.float64).reshape(n, 2).copy()
        mr = None
        if min_res is not None:
            mr = np.ascontiguousarray(min_res, np.float64).reshape(n, MAX_LEVELS)
        last = np.zeros((n, MAX_LEVELS))
        flow = np.zeros((n, 3))
        good = np.zeros(n, np.int32)
        check(self.L.dsm_track_batch(self.h, n, hs, _dp(poses), _dp(affs), coarsest, None if mr is None else _dp(mr),
                                     _dp(last), _dp(flow), good.ctypes.data_as(c_int_p)))
        return good.astype(bool), poses, affs, last, flow

    def upload_images(self, trackers, slots, images, exposures=None, asynchronous=False):
        """dsm_upload_images[_async]: hand over one level-0 image (float32 or uint8, all of one type) per (tracker, slot)
        in one call.  Images may be row-strided views (e.g. the calibration crop of a larger camera image), all with one
        pitch.  Slots 2 / 3 (DSM_SLOT_NEXT_LEFT / RIGHT) are the back buffers that advance_frames swaps in.
        asynchronous=True returns at once; the images must not be modified until upload_wait()."""
        n = len(trackers)
        if n == 0:
            return
        dt = np.dtype(images[0].dtype)
        if dt not in (np.dtype(np.float32), np.dtype(np.uint8)):
            raise TypeError("upload_images: float32 or uint8 images")
        keep, pitch = [], None
        for im, t in zip(images, trackers):
            if im.dtype != dt or im.shape != (t.hgt, t.w):
                raise ValueError("upload_images: image type / shape mismatch")
            if im.strides[1] != dt.itemsize or im.strides[0] < t.w * dt.itemsize:
                im = np.ascontiguousarray(im)
            if pitch is None:
                pitch = im.strides[0]
            elif im.strides[0] != pitch:
                raise ValueError("upload_images: images of one call share one row pitch")
            keep.append(im)
        hs = (C.c_void_p * n)(*[t.h for t in trackers])
        ps = (C.c_void_p * n)(*[im.ctypes.data for im in keep])
        sl = np.ascontiguousarray(slots, np.int32)
        ex = np.ones(n, np.float32) if exposures is None else np.ascontiguousarray(exposures, np.float32)
        fn = self.L.dsm_upload_images_async if asynchronous else self.L.dsm_upload_images
        check(fn(self.h, n, hs, sl.ctypes.data_as(c_int_p), ps, _fp(ex), 1 if dt == np.dtype(np.uint8) else 0, pitch))
        if asynchronous:
            self._pending_images = keep  # alive until upload_wait

    def upload_images_undistorted(self, und, trackers, slots, images, exposures=None, form="sync"):
        """dsm_upload_images_undistorted: hand over RAW uint8 camera images (und.original_size, all of one row pitch) per
        (tracker, slot); level 0 is their undistortion (Undistort::undistort, main.cpp:246-256).  form: "sync" (as
        upload_images), "async" (as upload_images(asynchronous=True): slots 2 / 3 + advance_frames, upload_wait) or
        "enqueue" (stream-ordered, front slots only; the images must stay untouched until upload_wait)."""
        forms = {"sync": 0, "async": 1, "enqueue": 2}
        if form not in forms:
            raise ValueError(f"upload_images_undistorted: form is one of {sorted(forms)}")
        n = len(trackers)
        if n == 0:
            return
        w_in, h_in = und.original_size
        keep, pitch = [], None
        for im in images:
            if im.dtype != np.uint8 or im.shape != (h_in, w_in):
                raise ValueError("upload_images_undistorted: uint8 images of the undistorter's input size")
            if im.strides[1] != 1 or im.strides[0] < w_in:
                im = np.ascontiguousarray(im)
            if pitch is None:
                pitch = im.strides[0]
            elif im.strides[0] != pitch:
                raise ValueError("upload_images_undistorted: images of one call share one row pitch")
            keep.append(im)
        hs = (C.c_void_p * n)(*[t.h for t in trackers])
        ps = (C.c_void_p * n)(*[im.ctypes.data for im in keep])
        sl = np.ascontiguousarray(slots, np.int32)
        ex = np.ones(n, np.float32) if exposures is None else np.ascontiguousarray(exposures, np.float32)
        check(self.L.dsm_upload_images_undistorted(self.h, und.h, n, hs, sl.ctypes.data_as(c_int_p), ps, _fp(ex), pitch, forms[form]))
        if form != "sync":
            self._pending_images = keep  # alive until upload_wait

    def upload_wait(self):
        check(self.L.dsm_upload_wait(self.h))
        self._pending_images = None

    def advance_frames(self, trackers, slots):
        """dsm_frames_advance: swap the back buffers of the given (tracker, slot in {0, 1}) pairs in"""
        n = len(trackers)
        if n == 0:
            return
        hs = (C.c_void_p * n)(*[t.h for t in trackers])
        sl = np.ascontiguousarray(slots, np.int32)
        check(self.L.dsm_frames_advance(self.h, n, hs, sl.ctypes.data_as(c_int_p)))

    def track_and_scale_batch(self, trackers, poses, affs, coarsest, scale_trackers, scales, min_res=None):
        """dsm_track_and_scale_batch: the frames' tracking and the keyframes' scale optimisation in one call (the scale
        problems run on their own stream under the tracking kernels); returns track_batch's tuple + (err, scales)"""
        n, n2 = len(trackers), len(scale_trackers)
        hs = (C.c_void_p * n)(*[t.h for t in trackers])
        hs2 = (C.c_void_p * max(1, n2))(*[t.h for t in scale_trackers])
        poses = np.ascontiguousarray(poses, np.float64).reshape(n, 7).copy()
        affs = np.ascontiguousarray(affs, np.float64).reshape(n, 2).copy()
        mr = None if min_res is None else np.ascontiguousarray(min_res, np.float64).reshape(n, MAX_LEVELS)
        last, flow, good = np.zeros((n, MAX_LEVELS)), np.zeros((n, 3)), np.zeros(n, np.int32)
        sc = np.ascontiguousarray(scales, np.float32).reshape(n2).copy()
        err = np.zeros(max(1, n2), np.float32)
        check(self.L.dsm_track_and_scale_batch(self.h, n, hs, _dp(poses), _dp(affs), coarsest, None if mr is None else _dp(mr), _dp(last),
                                               _dp(flow), good.ctypes.data_as(c_int_p), n2, hs2, _fp(sc) if n2 else None, _fp(err)))
        return good.astype(bool), poses, affs, last, flow, err[:n2], sc

    def optimize_scale_batch(self, trackers, scales, coarsest):
        n = len(trackers)
        hs = (C.c_void_p * n)(*[t.h for t in trackers])
        sc = np.ascontiguousarray(scales, np.float32).reshape(n).copy()
        err = np.zeros(n, np.float32)
        check(self.L.dsm_optimize_scale_batch(self.h, n, hs, _fp(sc), coarsest, _fp(err)))
        return err, sc


UNDISTORT_MODES = {"crop": 0, "none": 1, "explicit": 2}


def read_camera_file(path):
    """UPSTREAM-DSO's four-line camera file (cams/*/camera*.txt): `Pinhole fx fy cx cy 0` / `W H` / `crop | none |
    fx fy cx cy 0` / `W' H'`.  Returns dict(calib=(fx, fy, cx, cy), size_in=(W, H), mode="crop"|"none"|"explicit",
    out_calib=(4 floats) or None, size_out=(W', H')).  Other camera models are not built here (a caller's table covers
    them: Undistorter(..., remap=...))."""
    with open(path) as f:
        lines = [ln.strip() for ln in f.read().splitlines()]
    while lines and not lines[-1]:
        lines.pop()
    if len(lines) < 4:
        raise ValueError(f"{path}: a camera file has four lines")
    tok = lines[0].split()
    if len(tok) < 5 or tok[0] != "Pinhole":
        raise ValueError(f"{path}: line 1 is not `Pinhole fx fy cx cy 0`")
    calib = tuple(float(v) for v in tok[1:5])
    size_in = tuple(int(v) for v in lines[1].split()[:2])
    third = lines[2].split()
    if third == ["crop"]:
        mode, out_calib = "crop", None
    elif third == ["none"]:
        mode, out_calib = "none", None
    elif len(third) == 5:
        mode, out_calib = "explicit", tuple(float(np.float32(v)) for v in third[:4])  # (read with %f upstream)
    else:
        raise ValueError(f"{path}: line 3 is `crop`, `none` or five numbers (`full` is not supported)")
    size_out = tuple(int(v) for v in lines[3].split()[:2])
    return dict(calib=calib, size_in=size_in, mode=mode, out_calib=out_calib, size_out=size_out)


def pinhole_undistort_map(calib, size_in, mode="crop", size_out=None, out_calib=None):
    """dsm_pinhole_undistort_map (host code): (K_out (fx, fy, cx, cy) float32[4], passthrough, remap_x, remap_y) with the
    remap tables float32[h_out, w_out] (source coordinates, -1 = outside) or None for passthrough"""
    L = _lib.load()
    w_in, h_in = size_in
    w_out, h_out = size_in if size_out is None else size_out
    cal = np.ascontiguousarray(calib, np.float64)
    oc = None if out_calib is None else np.ascontiguousarray(out_calib, np.float32)
    K = np.zeros(4, np.float32)
    pt = C.c_int()
    rx = np.empty((h_out, w_out), np.float32)
    ry = np.empty((h_out, w_out), np.float32)
    check(L.dsm_pinhole_undistort_map(_dp(cal), w_in, h_in, UNDISTORT_MODES[mode], None if oc is None else _fp(oc), w_out, h_out,
                                      _fp(K), C.byref(pt), _fp(rx), _fp(ry)))
    if pt.value:
        return K, True, None, None
    return K, False, rx, ry


class Undistorter:
    """dsm_undistorter: one camera's undistortion on the device (UPSTREAM-DSO Undistort + PhotometricUndistorter) for
    Context.upload_images_undistorted.  remap_x / remap_y: float32[h_out, w_out] source coordinates (-1 = outside), None
    for passthrough; G: 256 floats (the rescaled response), vignette_inv: float32[h_in, w_in]; each optional."""

    def __init__(self, ctx, size_in, size_out, remap_x=None, remap_y=None, G=None, vignette_inv=None, K=None):
        self.L = _lib.load()
        self.ctx = ctx
        (w_in, h_in), (w_out, h_out) = size_in, size_out
        arrs = []
        for a, n in ((remap_x, w_out * h_out), (remap_y, w_out * h_out), (G, 256), (vignette_inv, w_in * h_in)):
            if a is None:
                arrs.append(None)
                continue
            a = np.ascontiguousarray(a, np.float32).reshape(-1)
            if a.size != n:
                raise ValueError("Undistorter: table of the wrong size")
            arrs.append(a)
        h = C.c_void_p()
        check(self.L.dsm_undistorter_create(ctx.h, w_in, h_in, w_out, h_out, *[None if a is None else _fp(a) for a in arrs], C.byref(h)))
        self.h = h
        self.original_size = (w_in, h_in)
        self.size = (w_out, h_out)
        self.K = None if K is None else np.asarray(K, np.float32)

    @classmethod
    def pinhole(cls, ctx, camera_file=None, calib=None, size_in=None, mode="crop", size_out=None, out_calib=None, G=None,
                vignette_inv=None):
        """From a camera file (size_out overrides its fourth line, as benchmarkSetting_width / height do: main.cpp:110-111)
        or from the values of one"""
        if camera_file is not None:
            cf = read_camera_file(camera_file)
            calib, size_in, mode, out_calib = cf["calib"], cf["size_in"], cf["mode"], cf["out_calib"]
            size_out = size_out or cf["size_out"]
        K, _, rx, ry = pinhole_undistort_map(calib, size_in, mode, size_out, out_calib)
        return cls(ctx, size_in, size_out or size_in, rx, ry, G, vignette_inv, K)

    def close(self):
        if getattr(self, "h", None):
            if getattr(self.ctx, "h", None):  # (destroy undistorters before their context)
                self.L.dsm_undistorter_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


class Stream:
    """Streaming form of Context.track_and_scale_batch (dsm_stream_*): a pool of resident problems advanced in passes; problems
    are admitted as slots free up and retire individually.  Results are bit-identical to the batch calls."""

    def __init__(self, ctx, track_slots, scale_slots=0, engine=None, ticks=0):
        self.ctx, self.L = ctx, ctx.L
        h = C.c_void_p()
        check(self.L.dsm_stream_create(ctx.h, int(track_slots), int(scale_slots), C.byref(h)))
        self.h = h
        if engine is not None:
            self.set_engine(engine, ticks)

    def set_engine(self, engine, ticks=0):
        """0: passes with carried stragglers; 1 (the library's default): ticks (one LM round per resident problem and tick, device-side admission).
        ticks = 0 keeps what is in force (initially: every advance sized by the stream from the retired problems' mean life)"""
        check(self.L.dsm_stream_set_engine(self.h, int(engine), int(ticks)))

    def set_chain(self, max_rounds):
        """tick engine: LM rounds a problem whose pending evaluation is ONE chunk may run inside one tick, in the workgroup that evaluates
        it (dsm_stream_set_chain); 0 = off, -1 = the library's default.  Scheduling only."""
        check(self.L.dsm_stream_set_chain(self.h, int(max_rounds)))

    def close(self):
        if getattr(self, "h", None):
            self.L.dsm_stream_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def submit_track(self, trackers, poses, affs, coarsest, min_res=None):
        n = len(trackers)
        hs = (C.c_void_p * n)(*[t.h for t in trackers])
        poses = np.ascontiguousarray(poses, np.float64).reshape(n, 7)
        affs = np.ascontiguousarray(affs, np.float64).reshape(n, 2)
        mr = None if min_res is None else np.ascontiguousarray(min_res, np.float64).reshape(n, MAX_LEVELS)
        tk = (C.c_uint64 * n)()
        check(self.L.dsm_stream_submit_track(self.h, n, hs, _dp(poses), _dp(affs), int(coarsest), None if mr is None else _dp(mr), tk))
        return list(tk)

    def submit_scale(self, trackers, scales, coarsest):
        n = len(trackers)
        hs = (C.c_void_p * n)(*[t.h for t in trackers])
        sc = np.ascontiguousarray(scales, np.float32).reshape(n)
        tk = (C.c_uint64 * n)()
        check(self.L.dsm_stream_submit_scale(self.h, n, hs, _fp(sc), int(coarsest), tk))
        return list(tk)

    def advance(self):
        check(self.L.dsm_stream_advance(self.h))

    def drain(self):
        check(self.L.dsm_stream_drain(self.h))

    def sync(self):
        """wait for everything in flight and read it back (the tick engine's advances are pipelined)"""
        check(self.L.dsm_stream_sync(self.h))

    def set_pipelined(self, on):
        check(self.L.dsm_stream_set_pipelined(self.h, int(bool(on))))

    def counts(self):
        """(resident, waiting, results ready)"""
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        check(self.L.dsm_stream_counts(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def results(self, max_results=None):
        """retired problems, oldest first: list of _lib.StreamResult"""
        if max_results is None:
            max_results = self.counts()[2]
        if max_results <= 0:
            return []
        buf = (_lib.StreamResult * max_results)()
        n = C.c_int()
        check(self.L.dsm_stream_results(self.h, max_results, buf, C.byref(n)))
        return [buf[i] for i in range(n.value)]

    def submit_hypotheses(self, trk, tries, aff_last_2_l, coarsestLvl, last_coarse_rmse0, reTrackThreshold=1.5):
        """the hypothesis loop of FrontEnd::trackNewCoarse (as track_hypotheses) as ONE group of the stream: the frame must be resident in
        trk's NEW_LEFT slot until the group's result is back.  Returns the group's ticket."""
        tries = np.ascontiguousarray(tries, np.float64).reshape(-1, 7)
        aff = np.ascontiguousarray(aff_last_2_l, np.float64).reshape(2)
        tk = C.c_uint64()
        check(self.L.dsm_stream_submit_hypotheses(self.h, trk.h, len(tries), _dp(tries), _dp(aff), int(coarsestLvl), float(last_coarse_rmse0),
                                                  float(reTrackThreshold), C.byref(tk)))
        return tk.value

    def hypotheses_results(self, raw=False):
        """resolved groups in resolution order: [(ticket, (haveOneGood, lastF_2_fh, aff_g2l, flowVecs, achievedRes, tries_used, tries_run))]
        -- track_hypotheses' tuple plus the tries the stream ran; raw=True: the _lib.StreamHypResult structures"""
        n_ready = self.hypotheses_counts()[1]
        if n_ready <= 0:
            return []
        buf = (_lib.StreamHypResult * n_ready)()
        n = C.c_int()
        check(self.L.dsm_stream_hypotheses_results(self.h, n_ready, buf, C.byref(n)))
        out = [buf[i] for i in range(n.value)]
        return out if raw else [(r.ticket, hyp_result_tuple(r)) for r in out]

    def hypotheses_counts(self):
        """(groups pending, group results ready)"""
        a, b = C.c_int(), C.c_int()
        check(self.L.dsm_stream_hypotheses_counts(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def set_hypothesis_window(self, w):
        """the most tries of one group waiting or resident at once after try 0; None / 0 = all of them.  Scheduling only."""
        check(self.L.dsm_stream_set_hypothesis_window(self.h, int(w or 0)))

    def set_quantile(self, q, lvl=-1):
        """q: one value (level lvl, or every level when lvl < 0) or a list from level 0"""
        if np.ndim(q) == 0:
            check(self.L.dsm_stream_set_quantile(self.h, int(lvl), float(q)))
        else:
            for l, v in enumerate(q):
                check(self.L.dsm_stream_set_quantile(self.h, l, float(v)))

    def set_rounds(self, mode, rounds):
        arr = None if rounds is None else (C.c_int * MAX_LEVELS)(*(list(rounds) + [0] * MAX_LEVELS)[:MAX_LEVELS])
        check(self.L.dsm_stream_set_rounds(self.h, int(mode), arr))

    def stats(self):
        a, b = Stats(), Stats()
        check(self.L.dsm_stream_get_stats(self.h, C.byref(a), C.byref(b)))
        return a, b

    def schedule(self, mode=0):
        r = (C.c_int * MAX_LEVELS)()
        p, q, c = C.c_longlong(), C.c_longlong(), C.c_longlong()
        check(self.L.dsm_stream_get_schedule(self.h, int(mode), r, C.byref(p), C.byref(q), C.byref(c)))
        return dict(rounds=list(r), passes=p.value, retired=q.value, carried_slot_passes=c.value)


class TrackerAndScaler:
    def __init__(self, ctx, w, h, nlevels, tfm_vec, K1, params=None):
        """tfm_vec: 16 doubles of T_stereo (cams/*/T_stereo.yaml); K1 = (fx,fy,cx,cy) of camera 1
        (reference ctor, TrackerAndScaler.cpp:47-109)."""
        self.ctx = ctx
        self.L = ctx.L
        self.w, self.hgt, self.nlevels = w, h, nlevels
        self.params = params if params is not None else default_params()
        T = np.ascontiguousarray(np.asarray(tfm_vec, np.float64).reshape(16))
        K1 = np.ascontiguousarray(np.asarray(K1, np.float32))
        hnd = C.c_void_p()
        check(self.L.dsm_tracker_create(ctx.h, w, h, nlevels, _dp(T), _fp(K1), C.byref(self.params), C.byref(hnd)))
        self.h = hnd
        self.lastFlowIndicators = np.full(3, 1000.0)
        self.firstCoarseRMSE = -1.0

    def close(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self.L.dsm_tracker_destroy(self.h)
        self.h = None

    def __del__(self):
        self.close()

    @property
    def refFrameID(self):
        return self.L.dsm_tracker_ref_frame_id(self.h)

    def makeK(self, fx, fy, cx, cy):
        check(self.L.dsm_tracker_make_k(self.h, fx, fy, cx, cy))

    def setCoarseTrackingRef(self, ref_frame_id, ref_aff, ref_exposure, pc_u, pc_v, pc_idepth, pc_color):
        n = (C.c_int * self.nlevels)(*[len(a) for a in pc_u])
        arrs = [[np.ascontiguousarray(a, np.float32) for a in lst] for lst in (pc_u, pc_v, pc_idepth, pc_color)]
        check(self.L.dsm_tracker_set_ref(self.h, ref_frame_id, float(ref_aff[0]), float(ref_aff[1]), ref_exposure, n,
                                         *[_ptr_array(a) for a in arrs]))
        self.firstCoarseRMSE = -1.0

    def setCoarseTrackingRefFromPoints(self, ref_frame_id, ref_aff, ref_exposure, pu, pv, pidepth, pweight,
                                       frame_owner=None, slot=0):
        """makeCoarseDepthL0 + setCoarseTrackingRef (TrackerAndScaler.cpp:143-327) on the device (row N3): the
        window's active points as flat arrays; the keyframe's pyramid is the one resident in `frame_owner`'s
        `slot` (default: this tracker's new-left slot).  Returns pc_n per level."""
        arrs = [np.ascontiguousarray(a, np.float32) for a in (pu, pv, pidepth, pweight)]
        npts = len(arrs[0])
        assert all(len(a) == npts for a in arrs)
        n = (C.c_int * self.nlevels)()
        owner = self if frame_owner is None else frame_owner
        check(self.L.dsm_tracker_set_ref_from_points(self.h, owner.h, slot, ref_frame_id, float(ref_aff[0]), float(ref_aff[1]),
                                                     ref_exposure, npts, *[_fp(a) for a in arrs], n))
        self.firstCoarseRMSE = -1.0
        return list(n)

    @staticmethod
    def setCoarseTrackingRefsFromPoints(ctx, jobs):
        """dsm_set_refs_from_points: the device templates of several trackers' new keyframes in ONE call (one host synchronisation).
        jobs: dicts with tracker, ref_frame_id, ref_aff, ref_exposure, pu, pv, pidepth, pweight and optionally frame_owner, slot.
        Returns pc_n per level for every job."""
        from ._lib import RefJob

        arr = (RefJob * len(jobs))()
        keep, outs = [], []
        for J, j in zip(arr, jobs):
            t = j["tracker"]
            a = [np.ascontiguousarray(j[k], np.float32) for k in ("pu", "pv", "pidepth", "pweight")]
            n = (C.c_int * t.nlevels)()
            keep.append(a)
            outs.append(n)
            J.t, J.frame_owner = t.h, j.get("frame_owner", t).h
            J.slot, J.ref_frame_id = j.get("slot", 0), j["ref_frame_id"]
            J.ref_aff_a, J.ref_aff_b, J.ref_exposure, J.npts = float(j["ref_aff"][0]), float(j["ref_aff"][1]), j["ref_exposure"], len(a[0])
            J.pu, J.pv, J.pidepth, J.pweight = [_fp(x) for x in a]
            J.n_out = C.cast(n, C.POINTER(C.c_int))
        check(ctx.L.dsm_set_refs_from_points(ctx.h, len(jobs), arr))
        for j in jobs:
            j["tracker"].firstCoarseRMSE = -1.0
        return [list(n) for n in outs]

    def scaleCoarseDepthL0(self, scale):
        check(self.L.dsm_tracker_scale_depth(self.h, scale))

    def get_template(self, lvl):
        n = C.c_int()
        check(self.L.dsm_tracker_get_template(self.h, lvl, C.byref(n), None, None, None, None))
        out = [np.zeros(n.value, np.float32) for _ in range(4)]
        check(self.L.dsm_tracker_get_template(self.h, lvl, C.byref(n), *[_fp(a) for a in out]))
        return out

    def upload_frame(self, slot, dIp, ab_exposure=1.0):
        dIp = [np.ascontiguousarray(a, np.float32) for a in dIp]
        check(self.L.dsm_tracker_upload_frame(self.h, slot, _ptr_array(dIp), ab_exposure))

    def upload_intensity(self, slot, planes, ab_exposure=1.0):
        """the intensity channel of every level alone (dsm_tracker_upload_intensity)"""
        planes = [np.ascontiguousarray(a, np.float32) for a in planes]
        check(self.L.dsm_tracker_upload_intensity(self.h, slot, _ptr_array(planes), ab_exposure))

    def upload_image(self, slot, image, ab_exposure=1.0):
        image = np.ascontiguousarray(image, np.float32)
        assert image.shape == (self.hgt, self.w)
        check(self.L.dsm_tracker_upload_image(self.h, slot, _fp(image), ab_exposure))

    def get_frame(self, slot, lvl):
        out = np.zeros((self.hgt >> lvl, self.w >> lvl, 3), np.float32)
        check(self.L.dsm_tracker_get_frame(self.h, slot, lvl, _fp(out)))
        return out

    def calcResPose(self, lvl, pose, aff, cutoff):
        """fused calcResPose + calcGSSSEPose: returns (rs[6], H[8,8], b[8], n_warped)"""
        pose = np.ascontiguousarray(pose, np.float64)
        aff = np.ascontiguousarray(aff, np.float64)
        rs, H, b, n = np.zeros(6), np.zeros(64), np.zeros(8), C.c_int()
        check(self.L.dsm_tracker_calc_res_pose(self.h, lvl, _dp(pose), _dp(aff), cutoff, _dp(rs), _dp(H), _dp(b), C.byref(n)))
        return rs, H.reshape(8, 8), b, n.value

    def calcResScale(self, lvl, scale, cutoff):
        rs, H, b, n = np.zeros(6), C.c_float(), C.c_float(), C.c_int()
        check(self.L.dsm_tracker_calc_res_scale(self.h, lvl, scale, cutoff, _dp(rs), C.byref(H), C.byref(b), C.byref(n)))
        return rs, H.value, b.value, n.value

    def diagEvalPose(self, lvl, pose, aff, cutoff, form=0, residual_only=False):
        """calcResPose with the evaluation launched in a chosen form of the loop (dsm_diag_single_eval): 0 the direct calls' kernel,
        1 the split pair, 2 the tick engine's items, 3 the chains' one-chunk form; returns (rs[6], H[8,8], b[8], n_warped)"""
        pose = np.ascontiguousarray(pose, np.float64)
        aff = np.ascontiguousarray(aff, np.float64)
        rs, H, b, n = np.zeros(6), np.zeros(64), np.zeros(8), C.c_int()
        check(self.L.dsm_diag_single_eval(self.h, 0, lvl, _dp(pose), _dp(aff), 1.0, cutoff, form, int(residual_only), _dp(rs), _dp(H), _dp(b),
                                          None, None, C.byref(n)))
        return rs, H.reshape(8, 8), b, n.value

    def diagEvalFacts(self, lvl, pose, with_bounds=False):
        """the facts that pick the instantiation of a pose evaluation of level lvl at pose (dsm_diag_eval_facts), derived on the
        device by the production code; returns (template fact, image fact, pose fact, fast) as 0 / 1 -- with_bounds: and the
        list's bounds (umin, umax, vmin, vmax, idepth max) as a float32 array"""
        pose = np.ascontiguousarray(pose, np.float64)
        out, bounds = np.zeros(4, np.int32), np.zeros(5, np.float32)
        check(self.L.dsm_diag_eval_facts(self.h, lvl, _dp(pose), out.ctypes.data_as(c_int_p), _fp(bounds)))
        facts = tuple(int(v) for v in out)
        return (facts, bounds) if with_bounds else facts

    def diagForceGeneral(self, on=True):
        """evaluations of this tracker take the general per-point code whatever the facts say (dsm_diag_tracker_force_general)"""
        check(self.L.dsm_diag_tracker_force_general(self.h, int(bool(on))))

    def diagEvalScale(self, lvl, scale, cutoff, form=0, residual_only=False):
        """calcResScale likewise; returns (rs[6], h00, h01, n_warped)"""
        rs, H, b, n = np.zeros(6), C.c_float(), C.c_float(), C.c_int()
        check(self.L.dsm_diag_single_eval(self.h, 1, lvl, None, None, scale, cutoff, form, int(residual_only), _dp(rs), None, None, C.byref(H),
                                          C.byref(b), C.byref(n)))
        return rs, H.value, b.value, n.value

    def diagLmPropose(self, mode, lvl, problems, spec=False, helper=False):
        """the proposing half of an LM step on caller-supplied systems (dsm_diag_lm_propose).  problems: a numpy array of
        LM_PROPOSE_IN records; returns an array of LM_PROPOSE_OUT records, one per problem"""
        problems = np.ascontiguousarray(problems, LM_PROPOSE_IN)
        out = np.zeros(len(problems), LM_PROPOSE_OUT)
        check(self.L.dsm_diag_lm_propose(self.h, mode, lvl, len(problems), problems.ctypes.data_as(C.POINTER(LmProposeIn)), int(spec), int(helper),
                                         out.ctypes.data_as(C.POINTER(LmProposeOut))))
        return out

    def diagLmStep(self, mode, lvl, states, partials, spec=False, spec_off=0, helper=False, coherent=False):
        """one production LM step per problem on caller-supplied states and partials (dsm_diag_lm_step).  states: a numpy array of
        LM_STEP_STATE records; partials: float32 [len(states), partial_stride] (view integer slots as float32), the speculative
        evaluation's spec_off floats behind the main ones.  Returns an array of LM_STEP_STATE records: the states after the step"""
        states = np.ascontiguousarray(states, LM_STEP_STATE)
        partials = np.ascontiguousarray(partials, np.float32)
        assert partials.ndim == 2 and len(partials) == len(states)
        out = np.zeros(len(states), LM_STEP_STATE)
        check(self.L.dsm_diag_lm_step(self.h, mode, lvl, len(states), states.ctypes.data_as(C.POINTER(LmStepState)), _fp(partials),
                                      partials.shape[1], int(spec), int(spec_off), int(helper), int(coherent),
                                      out.ctypes.data_as(C.POINTER(LmStepState))))
        return out

    def diagTickStage(self, mode, slots, list_cfg, ctl, pending=None, stepped=0):
        """tick_after_step behind each slot's reservation, one wave per slot in one launch (dsm_diag_tick_stage).  slots: TICK_SLOT
        records; list_cfg: dict(cap, chain_cap, chain_max_n0, buf, count, chain); ctl: dict(pending_head, pending_count, retired, ring);
        pending: TICK_PENDING records.  Returns a dict: items (the whole allocation), seg, ctl, results, slot_out, state_out, state_raw,
        start_raw"""
        slots = np.ascontiguousarray(slots, TICK_SLOT)
        sp = slots.ctypes.data_as(C.POINTER(TickSlot))
        return _tick_call(self.L.dsm_diag_tick_stage, lambda lc, mc, npend, pend: (self.h, mode, len(slots), sp, lc, mc, npend, pend, int(stepped)),
                          len(slots), list_cfg, ctl, pending)

    def diagTickStep(self, mode, lvl, states, slots, partials, speculate, opts, list_cfg, ctl, pending=None, admit_idx=None):
        """the production tick_admit_kernel (admit_idx given) and tick_lm_kernel on slots built as diagLmStep builds its problems
        (dsm_diag_tick_step; opts bit 2: the admission alone).  Returns diagTickStage's dict"""
        states = np.ascontiguousarray(states, LM_STEP_STATE)
        slots = np.ascontiguousarray(slots, TICK_SLOT)
        partials = np.ascontiguousarray(partials, np.float32)
        assert partials.ndim == 2 and len(partials) == len(states) == len(slots)
        adm = None if admit_idx is None else np.ascontiguousarray(admit_idx, np.int64)
        adm_p = None if adm is None else adm.ctypes.data_as(C.POINTER(C.c_longlong))
        st_p, sl_p = states.ctypes.data_as(C.POINTER(LmStepState)), slots.ctypes.data_as(C.POINTER(TickSlot))
        return _tick_call(self.L.dsm_diag_tick_step,
                          lambda lc, mc, npend, pend: (self.h, mode, lvl, len(states), st_p, sl_p, _fp(partials), partials.shape[1], int(speculate),
                                                       int(opts), lc, mc, npend, pend, adm_p),
                          len(states), list_cfg, ctl, pending)

    def trackNewestCoarse(self, lastToNew, aff_g2l, coarsestLvl, minResForAbort=None):
        """returns (good, lastToNew_out, aff_g2l_out, lastResiduals) and sets lastFlowIndicators"""
        pose = np.array(lastToNew, np.float64)
        aff = np.array(aff_g2l, np.float64)
        mr = None if minResForAbort is None else np.ascontiguousarray(minResForAbort, np.float64)
        last, flow, good = np.zeros(MAX_LEVELS), np.zeros(3), C.c_int()
        check(self.L.dsm_tracker_track(self.h, _dp(pose), _dp(aff), coarsestLvl, None if mr is None else _dp(mr), _dp(last),
                                       _dp(flow), C.byref(good)))
        self.lastFlowIndicators = flow
        return bool(good.value), pose, aff, last

    def optimizeScale(self, scale, coarsestLvl):
        """returns (error, scale_out) as the reference's `float optimizeScale(fh1, float &scale, lvl)`"""
        s, err = C.c_float(scale), C.c_float()
        check(self.L.dsm_tracker_optimize_scale(self.h, C.byref(s), coarsestLvl, C.byref(err)))
        return err.value, s.value

    def optimizeScaleGuesses(self, guesses, coarsestLvl):
        """the untrapped branch of FrontEnd::optimizeScale (FrontEnd.cpp:995-1003) as one batched call: returns
        (scale_error, new_scale, all_errors, all_scales)"""
        g = np.ascontiguousarray(guesses, np.float32)
        s, e = C.c_float(), C.c_float()
        sa, ea = np.zeros(len(g), np.float32), np.zeros(len(g), np.float32)
        check(self.L.dsm_tracker_optimize_scale_guesses(self.h, len(g), _fp(g), coarsestLvl, C.byref(s), C.byref(e), _fp(sa), _fp(ea)))
        return e.value, s.value, ea, sa

    def reduction_geometry(self, lvl, n):
        t, p, c = C.c_int(), C.c_int(), C.c_int()
        check(self.L.dsm_reduction_geometry(self.h, lvl, n, C.byref(t), C.byref(p), C.byref(c)))
        return t.value, p.value, c.value


def make_coarse_depth_l0(w, h, nlevels, pu, pv, pidepth, pweight, ref_dIp):
    """TrackerAndScaler::makeCoarseDepthL0 (TrackerAndScaler.cpp:143-315) from flat active-point arrays,
    through the C ABI (host code in this round).  Returns [pc_u, pc_v, pc_idepth, pc_color] lists per level,
    i.e. the arguments of setCoarseTrackingRef."""
    L = _lib.load()
    pu, pv, pidepth, pweight = [np.ascontiguousarray(a, np.float32) for a in (pu, pv, pidepth, pweight)]
    ref = [np.ascontiguousarray(a, np.float32) for a in ref_dIp]
    n_out = (C.c_int * nlevels)()
    outs = [[np.zeros((w >> l) * (h >> l), np.float32) for l in range(nlevels)] for _ in range(4)]
    check(L.dsm_make_coarse_depth_l0(w, h, nlevels, len(pu), _fp(pu), _fp(pv), _fp(pidepth), _fp(pweight), _ptr_array(ref),
                                     n_out, *[_ptr_array(o) for o in outs]))
    return [[o[l][: n_out[l]].copy() for l in range(nlevels)] for o in outs]


class PoseEstimator:
    """Python mirror of the reference's `dso::PoseEstimator` (PoseEstimator.h:34-83) on the C ABI."""

    def __init__(self, ctx, w, h, nlevels, params=None):
        self.ctx, self.L = ctx, ctx.L
        self.params = params if params is not None else default_params()
        hnd = C.c_void_p()
        check(self.L.dsm_pose_estimator_create(ctx.h, w, h, nlevels, C.byref(self.params), C.byref(hnd)))
        self.h = hnd

    def close(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self.L.dsm_pose_estimator_destroy(self.h)
        self.h = None

    def __del__(self):
        self.close()

    def estimate(self, pts_xyz, ref_colors, ref_ab_exposure, new_dIp, new_ab_exposure, new_cam, coarsest_lvl, ref_to_new):
        """returns (ok, ref_to_new 4x4, pose_error) like `bool estimate(pts, ref_ab_exposure, new_fh, new_cam,
        coarsest_lvl, Matrix4d& ref_to_new, float& pose_error)`"""
        xyz = np.ascontiguousarray(pts_xyz, np.float64).reshape(-1, 3)
        cols = [np.ascontiguousarray(c, np.float32) for c in ref_colors]
        dIp = [np.ascontiguousarray(a, np.float32) for a in new_dIp]
        cam = np.ascontiguousarray(new_cam, np.float32)
        T = np.ascontiguousarray(ref_to_new, np.float64).reshape(16).copy()
        err, ok = C.c_float(), C.c_int()
        check(self.L.dsm_pose_estimator_estimate(self.h, len(xyz), _dp(xyz), _ptr_array(cols), ref_ab_exposure, _ptr_array(dIp),
                                                 new_ab_exposure, _fp(cam), coarsest_lvl, _dp(T), C.byref(err), C.byref(ok)))
        return bool(ok.value), T.reshape(4, 4), err.value

    def load_args(self, pts_xyz, ref_colors, ref_ab_exposure, new_dIp, new_ab_exposure, new_cam):
        """the inputs of an evaluation as diagEval takes them, converted once (a sweep evaluates the same inputs many times).  Test aid."""
        xyz = np.ascontiguousarray(pts_xyz, np.float64).reshape(-1, 3)
        cols = [np.ascontiguousarray(c, np.float32) for c in ref_colors]
        dIp = [np.ascontiguousarray(a, np.float32) for a in new_dIp]
        cam = np.ascontiguousarray(new_cam, np.float32)
        return (xyz, cols, dIp, cam), (len(xyz), _dp(xyz), _ptr_array(cols), ref_ab_exposure, _ptr_array(dIp), new_ab_exposure, _fp(cam))

    def diagEval(self, inputs, lvl, pose, aff, cutoff, form=0, residual_only=False):
        """ONE evaluation of the loop-closure alignment in a chosen form of the loop (dsm_diag_pose_estimator_eval: 0 the direct
        kernel, 1 the split pair, 3 the chains' one-chunk form) on `inputs` = load_args(...): (rs, H[8,8], b, n_warped).  Test aid."""
        pose = np.ascontiguousarray(pose, np.float64)
        aff = np.ascontiguousarray(aff, np.float64)
        rs, H, b, n = np.zeros(6), np.zeros(64), np.zeros(8), C.c_int()
        check(self.L.dsm_diag_pose_estimator_eval(self.h, *inputs[1], lvl, _dp(pose), _dp(aff), cutoff, form, int(residual_only), _dp(rs),
                                                  _dp(H), _dp(b), C.byref(n)))
        return rs, H.reshape(8, 8), b, n.value


class PoseBatch:
    """`dso::PoseEstimator::estimate` of many matches in one call (dsm_pose_estimate_batch): one geometry, per job its own points,
    colours, intrinsics, exposures and guess.  A job is a dict with the keys pts_xyz, ref_colors, ref_ab_exposure, new_ab_exposure,
    new_cam, ref_to_new and exactly one of new_dIp (the AoS (I,dx,dy) pyramid) / new_I (its intensity planes)."""

    KEYS = ("pts_xyz", "ref_colors", "ref_ab_exposure", "new_ab_exposure", "new_cam", "ref_to_new")

    def __init__(self, ctx, w, h, nlevels, params=None):
        self.ctx, self.L = ctx, ctx.L
        self.w, self.h, self.nlevels = w, h, nlevels
        self.params = params if params is not None else default_params()
        hnd = C.c_void_p()
        check(self.L.dsm_pose_batch_create(ctx.h, w, h, nlevels, C.byref(self.params), C.byref(hnd)))
        self.h_ = hnd

    def close(self):
        if getattr(self, "h_", None) and getattr(self.ctx, "h", None):
            self.L.dsm_pose_batch_destroy(self.h_)
        self.h_ = None

    def __del__(self):
        self.close()

    @staticmethod
    def check_jobs(jobs, w, h, nlevels):
        """what is wrong with a job list, before any library call: ValueError.  Returns the jobs with their arrays in the ABI's types;
        the same array object passed by several jobs stays one array (the library shares the planes of a shared target pyramid)."""
        if len(jobs) < 1:
            raise ValueError("PoseBatch: an empty job list")
        conv = {}  # id(caller's array) -> converted array

        def as_f32(a):
            if id(a) not in conv:
                conv[id(a)] = (a, np.ascontiguousarray(a, np.float32))
            return conv[id(a)][1]

        out = []
        for j, job in enumerate(jobs):
            missing = [k for k in PoseBatch.KEYS if k not in job]
            if missing:
                raise ValueError(f"PoseBatch: job {j} lacks {missing}")
            has_dip, has_i = job.get("new_dIp") is not None, job.get("new_I") is not None
            if has_dip == has_i:
                raise ValueError(f"PoseBatch: job {j} needs exactly one of new_dIp and new_I")
            xyz = np.ascontiguousarray(job["pts_xyz"], np.float64)
            if xyz.ndim != 2 or xyz.shape[1] != 3 or not 1 <= len(xyz) <= w * h:
                raise ValueError(f"PoseBatch: job {j}: pts_xyz must be n x 3 with 1 <= n <= w*h")
            cols = [np.ascontiguousarray(c, np.float32).reshape(-1) for c in job["ref_colors"]]
            if len(cols) != nlevels or any(len(c) != len(xyz) for c in cols):
                raise ValueError(f"PoseBatch: job {j}: ref_colors must hold {nlevels} lists of {len(xyz)} colours (one per point and level)")
            tgt = [as_f32(a) for a in (job["new_dIp"] if has_dip else job["new_I"])]
            if len(tgt) != nlevels or any(a.size != (w >> l) * (h >> l) * (3 if has_dip else 1) for l, a in enumerate(tgt)):
                raise ValueError(f"PoseBatch: job {j}: the target pyramid must hold {nlevels} levels of this batch's geometry")
            cam = np.ascontiguousarray(job["new_cam"], np.float32).reshape(-1)
            T = np.array(job["ref_to_new"], np.float64).reshape(-1)
            if len(cam) != 4 or len(T) != 16:
                raise ValueError(f"PoseBatch: job {j}: new_cam is (fx, fy, cx, cy), ref_to_new a 4 x 4 matrix")
            out.append(dict(xyz=xyz, cols=cols, tgt=tgt, dip=has_dip, cam=cam, T=T.copy(), ref_exp=float(job["ref_ab_exposure"]),
                            new_exp=float(job["new_ab_exposure"])))
        return out

    @staticmethod
    def build_jobs(js):
        """the dsm_pose_job array of checked jobs (check_jobs), and what must outlive the call: (array, outputs, keep-alive list);
        outputs = (T n x 16 holding the guesses, pose_error, inlier_percent, ok)"""
        n = len(js)
        arr = (_lib.PoseJob * n)()
        T = np.stack([j["T"] for j in js])
        err, inl, ok = np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros(n, np.int32)
        keep = [js]
        tables = {}  # one pointer table per target pyramid: jobs that share a pyramid pass the same level pointers
        for i, j in enumerate(js):
            cols = _ptr_array(j["cols"])
            key = tuple(id(a) for a in j["tgt"])
            if key not in tables:
                tables[key] = _ptr_array(j["tgt"])
            keep.append(cols)
            a = arr[i]
            a.n_pts, a.xyz, a.ref_colors, a.ref_ab_exposure = len(j["xyz"]), _dp(j["xyz"]), cols, j["ref_exp"]
            if j["dip"]:
                a.new_dIp = tables[key]
            else:
                a.new_I = tables[key]
            a.new_ab_exposure = j["new_exp"]
            a.new_cam[:] = [float(v) for v in j["cam"]]
            a.ref_to_new_io = _dp(T[i:])
            a.pose_error = err[i:].ctypes.data_as(c_float_p)
            a.inlier_percent = inl[i:].ctypes.data_as(c_int_p)
            a.ok = ok[i:].ctypes.data_as(c_int_p)
        keep.append(tables)
        return arr, (T, err, inl, ok), keep

    def estimate_many(self, jobs, coarsest_lvl):
        """per job (ok, ref_to_new 4x4, pose_error, inlier_percent)"""
        arr, (T, err, inl, ok), keep = self.build_jobs(self.check_jobs(jobs, self.w, self.h, self.nlevels))
        check(self.L.dsm_pose_estimate_batch(self.h_, len(arr), arr, coarsest_lvl))
        del keep
        return [(bool(ok[i]), T[i].reshape(4, 4).copy(), float(err[i]), int(inl[i])) for i in range(len(arr))]


def track_hypotheses(ctx, trk, tries, aff_last_2_l, coarsestLvl, last_coarse_rmse0, reTrackThreshold=1.5):
    """The hypothesis loop of FrontEnd::trackNewCoarse (FrontEnd.cpp:194-247) with the same results as
    the reference's sequential loop, but evaluated as ONE batched launch sequence ("next" row N4).

    Reference semantics: try i is tracked with minResForAbort = achievedRes of the earlier tries and is
    aborted at the first level whose residual exceeds 1.5x that value (TrackerAndScaler.cpp:598); the
    loop ends at the first success below last_coarse_rmse*reTrackThreshold.  Here try 0 runs alone (the
    common case ends there); otherwise all remaining tries run as one batch WITHOUT abort, and the abort
    / take-over logic is replayed on the host from their per-level residuals -- a level's LM result does
    not depend on minResForAbort, so the replay is exact.
    Returns (haveOneGood, lastF_2_fh, aff_g2l, flowVecs, achievedRes, tries_used)."""
    tries = np.ascontiguousarray(tries, np.float64).reshape(-1, 7)
    n = len(tries)
    achieved = np.full(MAX_LEVELS, np.nan)
    have_good = False
    flow = np.array([100.0, 100.0, 100.0])
    best_pose, best_aff = IDENTITY_POSE7.copy(), np.zeros(2)

    def consume(good, pose, aff, cur_res, fl):
        nonlocal have_good, flow, best_pose, best_aff
        if good and np.isfinite(np.float32(cur_res[0])) and not (cur_res[0] >= achieved[0]):  # :225-233
            flow, best_aff, best_pose, have_good = fl.copy(), aff.copy(), pose.copy(), True
        if have_good:  # :236-243
            for l in range(5):
                if not np.isfinite(np.float32(achieved[l])) or achieved[l] > cur_res[l]:
                    achieved[l] = cur_res[l]
        return have_good and achieved[0] < last_coarse_rmse0 * reTrackThreshold  # :245-247

    # try 0 alone
    good, pose, aff, last = trk.trackNewestCoarse(tries[0], aff_last_2_l, coarsestLvl, achieved)
    used = 1
    if consume(good, pose, aff, last, trk.lastFlowIndicators) or n == 1:
        return have_good, (best_pose if have_good else tries[0]), (best_aff if have_good else np.asarray(aff_last_2_l, float)), \
            (flow if have_good else np.zeros(3)), achieved, used
    # the rest as one batch, no abort
    m = n - 1
    goods, poses, affs, lasts, flows = ctx.track_batch([trk] * m, tries[1:], np.tile(np.asarray(aff_last_2_l, np.float64), (m, 1)),
                                                       coarsestLvl, None)
    for i in range(m):
        used += 1
        cur = lasts[i].copy()
        good_i = bool(goods[i])
        # replay the abort test of TrackerAndScaler.cpp:598 level by level (coarse to fine)
        for l in range(coarsestLvl, -1, -1):
            if cur[l] > 1.5 * achieved[l]:
                cur[:l] = np.nan
                good_i = False
                break
        pose_i = poses[i] if good_i else tries[1 + i]  # an aborted try leaves lastToNew_out untouched
        if consume(good_i, pose_i, affs[i], cur, flows[i]):
            break
    if not have_good:  # :249-256
        return False, tries[0], np.asarray(aff_last_2_l, float), np.zeros(3), achieved, used
    return True, best_pose, best_aff, flow, achieved, used


IDENTITY_POSE7 = np.array([0, 0, 0, 1, 0, 0, 0], np.float64)


def hyp_result_tuple(r):
    """a dsm_stream_hyp_result in track_hypotheses' tuple shape, plus tries_run"""
    return (bool(r.have_one_good), np.array(r.pose), np.array(r.aff), np.array(r.flow), np.array(r.achieved_res), int(r.tries_used),
            int(r.tries_run))


def hypotheses_resolve(tries, aff_last_2_l, coarsestLvl, last_coarse_rmse0, goods, poses, affs, last_residuals, flows, reTrackThreshold=1.5):
    """dsm_hypotheses_resolve (host code): the loop of FrontEnd.cpp:194-256 replayed from the outputs of the first k = len(goods) tries run
    without abort.  Returns (decided, track_hypotheses' tuple plus tries_run)."""
    tries = np.ascontiguousarray(tries, np.float64).reshape(-1, 7)
    aff = np.ascontiguousarray(aff_last_2_l, np.float64).reshape(2)
    k = len(goods)
    g = np.ascontiguousarray(goods, np.int32).reshape(k)
    P = np.ascontiguousarray(poses, np.float64).reshape(k, 7)
    A = np.ascontiguousarray(affs, np.float64).reshape(k, 2)
    R = np.ascontiguousarray(last_residuals, np.float64).reshape(k, MAX_LEVELS)
    F = np.ascontiguousarray(flows, np.float64).reshape(k, 3)
    out, dec = _lib.StreamHypResult(), C.c_int()
    check(_lib.load().dsm_hypotheses_resolve(len(tries), _dp(tries), _dp(aff), int(coarsestLvl), float(last_coarse_rmse0), float(reTrackThreshold), k,
                                             g.ctypes.data_as(c_int_p), _dp(P), _dp(A), _dp(R), _dp(F), C.byref(out), C.byref(dec)))
    return bool(dec.value), hyp_result_tuple(out)
