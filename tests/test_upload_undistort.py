"""dsm_upload_images_undistorted: raw mono8 camera bytes in, pyramids out -- level 0 bit for bit the numpy restatement of
UPSTREAM-DSO's Undistort::undistort<unsigned char>(img, 1, 0, 1.0f) (main.cpp:246-256), every other level makeImages of it;
the geometry is that of the builder's output camera; bad tables and bad calls are refused."""
import os

import numpy as np
import pytest

import _undistort_ref as R
from direct_stereo_slam_amd import synth as S
from direct_stereo_slam_amd._lib import DsmError
from oracle import oracle as O

pytestmark = pytest.mark.gpu

CAMS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cams")
# camera file, output size (None: the file's), pyramid levels
CONFIGS = {
    "kitti": (os.path.join(CAMS, "kitti", "0_2", "camera0.txt"), None, 5),
    "malaga": (os.path.join(CAMS, "malaga", "camera0.txt"), None, 5),
    "robotcar_preset2": (os.path.join(CAMS, "robotcar", "camera0.txt"), (424, 320), 4),
}


def _photometric(kind, w_in, h_in):
    G = vig = None
    if kind in ("G", "G+vig"):
        G = (255.0 * (np.arange(256) / 255.0) ** 0.8).astype(np.float32)  # a rescaled response
    if kind in ("G+vig", "vig"):  # "vig": a vignette without a response table
        X, Y = np.meshgrid(np.linspace(-1, 1, w_in), np.linspace(-1, 1, h_in))
        vig = (1.0 / (1.0 - 0.3 * (X * X + Y * Y) / 2.0)).astype(np.float32)
    return G, vig


def _setup(ctx, conf, photo="none", n_trackers=1):
    from direct_stereo_slam_amd.tracker import TrackerAndScaler, Undistorter, pinhole_undistort_map, read_camera_file

    path, size_out, nl = CONFIGS[conf]
    cf = read_camera_file(path)
    size_out = size_out or cf["size_out"]
    G, vig = _photometric(photo, *cf["size_in"])
    und = Undistorter.pinhole(ctx, path, size_out=size_out, G=G, vignette_inv=vig)
    K, _, rx, ry = pinhole_undistort_map(cf["calib"], cf["size_in"], "crop", size_out)
    np.testing.assert_array_equal(und.K, K)
    assert und.size == size_out and und.original_size == cf["size_in"]
    trks = [TrackerAndScaler(ctx, size_out[0], size_out[1], nl, S.KITTI_T_STEREO, K) for _ in range(n_trackers)]
    return und, trks, (rx, ry, G, vig), nl


def _raw(rng, und, n):
    w_in, h_in = und.original_size
    return [rng.integers(0, 256, (h_in, w_in), dtype=np.uint8) for _ in range(n)]


def _check(trk, slot, img, tabs, nl):
    rx, ry, G, vig = tabs
    want = O.make_images(R.undistort(np.ascontiguousarray(img), rx, ry, G, vig), nl)
    for lvl in range(nl):
        np.testing.assert_array_equal(trk.get_frame(slot, lvl), want[lvl], err_msg=f"level {lvl}")


# every configuration under none, G and G+vig; the vignette without a response table on one remap and on the passthrough form
PYRAMID_CASES = [(conf, photo) for conf in sorted(CONFIGS) for photo in ("none", "G", "G+vig")] + [("robotcar_preset2", "vig"), ("passthrough", "vig")]


def _setup_passthrough(ctx, photo, nl=5):
    """mode "none" at the KITTI camera size 1241 x 376 (odd width: the quads of the last column have no right half)"""
    from direct_stereo_slam_amd.tracker import TrackerAndScaler, Undistorter

    calib, size_in = (718.8560, 718.8560, 607.1928, 185.2157), (1241, 376)
    G, vig = _photometric(photo, *size_in)
    und = Undistorter.pinhole(ctx, calib=calib, size_in=size_in, mode="none", G=G, vignette_inv=vig)
    assert und.size == size_in
    return und, [TrackerAndScaler(ctx, *size_in, nl, S.KITTI_T_STEREO, und.K)], (None, None, G, vig), nl


@pytest.mark.parametrize("conf,photo", PYRAMID_CASES, ids=[f"{c}-{p}" for c, p in PYRAMID_CASES])
def test_pyramids_equal_the_restatement(ctx, conf, photo):
    und, (trk,), tabs, nl = _setup_passthrough(ctx, photo) if conf == "passthrough" else _setup(ctx, conf, photo)
    assert (tabs[2] is None and tabs[3] is not None) == (photo == "vig")
    imgs = _raw(np.random.default_rng(1), und, 2)
    ctx.upload_images_undistorted(und, [trk, trk], [0, 1], imgs)
    for s in (0, 1):
        _check(trk, s, imgs[s], tabs, nl)
    und.close()


def test_odd_output_size_with_a_remap(ctx):
    """211 x 97 cropped from a 240 x 120 camera: the quads of the last column and of the last row are halves, the last quad a
    single pixel, in the remap form; levels 105 x 48, 52 x 24, 26 x 12 drop a column or a row each"""
    from direct_stereo_slam_amd.tracker import TrackerAndScaler, Undistorter, pinhole_undistort_map

    calib, size_in, size_out, nl = (190.0, 185.0, 121.3, 58.9), (240, 120), (211, 97), 4
    K, passthrough, rx, ry = pinhole_undistort_map(calib, size_in, "crop", size_out)
    assert not passthrough and rx.shape == (97, 211) and (rx[:, -1] >= 0).all() and (rx[-1] >= 0).all()  # the last column and row are inside
    assert (rx != np.floor(rx)).mean() > 0.9 and (ry != np.floor(ry)).mean() > 0.9  # a real interpolation nearly everywhere
    G, vig = _photometric("G+vig", *size_in)
    und = Undistorter(ctx, size_in, size_out, rx, ry, G, vig, K)
    trk = TrackerAndScaler(ctx, *size_out, nl, S.KITTI_T_STEREO, K)
    imgs = [np.random.default_rng(9).integers(0, 256, size_in[::-1], dtype=np.uint8) for _ in range(2)]
    ctx.upload_images_undistorted(und, [trk, trk], [0, 1], imgs)
    for s in (0, 1):
        _check(trk, s, imgs[s], (rx, ry, G, vig), nl)
    np.testing.assert_array_equal(trk.get_frame(0, 0)[..., 0], R.undistort(imgs[0], rx, ry, G, vig))
    und.close()


def test_more_quads_than_one_trip_of_the_grid(ctx):
    """1501 x 1399 from a 1536 x 1440 camera: 751 x 700 = 525 700 quads, more than the 2048 x 256 = 524 288 threads of the largest grid,
    so the quad loop takes a second trip (the last 1 412 quads); remap form, a vignette without a response table, two levels"""
    from direct_stereo_slam_amd.tracker import TrackerAndScaler, Undistorter, pinhole_undistort_map

    calib, size_in, size_out, nl = (1210.0, 1190.0, 770.2, 717.6), (1536, 1440), (1501, 1399), 2
    assert ((size_out[0] + 1) // 2) * ((size_out[1] + 1) // 2) > 2048 * 256 and size_out[0] * size_out[1] > 2097152
    K, passthrough, rx, ry = pinhole_undistort_map(calib, size_in, "crop", size_out)
    assert not passthrough and (rx >= 0).mean() > 0.99
    G, vig = _photometric("vig", *size_in)
    und = Undistorter(ctx, size_in, size_out, rx, ry, G, vig, K)
    trk = TrackerAndScaler(ctx, *size_out, nl, S.KITTI_T_STEREO, K)
    img = np.random.default_rng(10).integers(0, 256, size_in[::-1], dtype=np.uint8)
    ctx.upload_images_undistorted(und, [trk], [0], [img])
    want0 = R.undistort(img, rx, ry, G, vig)
    got0 = trk.get_frame(0, 0)[..., 0]
    second_trip = 2 * (524288 // 751)  # the row of the first quad of the second trip
    assert second_trip < size_out[1] - 2 and want0[second_trip:].any()
    np.testing.assert_array_equal(got0[second_trip:], want0[second_trip:], err_msg="the rows of the second trip")
    _check(trk, 0, img, (rx, ry, G, vig), nl)
    und.close()


def test_caller_table_with_holes(ctx):
    """a caller's table (here: the KITTI crop with punched holes, and a wider explicit output camera) -- outside = 0"""
    from direct_stereo_slam_amd.tracker import TrackerAndScaler, Undistorter, pinhole_undistort_map

    rng = np.random.default_rng(2)
    calib, size_in = (718.8560, 718.8560, 607.1928, 185.2157), (1241, 376)
    K, _, rx, ry = pinhole_undistort_map(calib, size_in, "crop", (1232, 368))
    hole = rng.random(rx.shape) < 0.05
    rx, ry = np.where(hole, -1, rx).astype(np.float32), np.where(hole, -1, ry).astype(np.float32)
    Ke, _, ex, ey = pinhole_undistort_map(calib, size_in, "explicit", (640, 192), (0.6, 1.9, 0.5, 0.48))
    assert (ex < 0).any()
    G, vig = _photometric("G+vig", *size_in)
    for (w, h), tx, ty, KK in (((1232, 368), rx, ry, K), ((640, 192), ex, ey, Ke)):
        und = Undistorter(ctx, size_in, (w, h), tx, ty, G, vig)
        trk = TrackerAndScaler(ctx, w, h, 4, S.KITTI_T_STEREO, KK)
        imgs = [rng.integers(0, 256, size_in[::-1], dtype=np.uint8) for _ in range(2)]
        ctx.upload_images_undistorted(und, [trk, trk], [0, 1], imgs)
        for s in (0, 1):
            _check(trk, s, imgs[s], (tx, ty, G, vig), 4)
            assert (trk.get_frame(s, 0)[..., 0][tx < 0] == 0).all()


@pytest.mark.parametrize("form", ["sync", "async", "enqueue"])
def test_forms_pitch_and_pinned_buffers(ctx, form):
    """tight and pitched rows (16-, 4- and 1-byte copy units when pinned), pinned and pageable; async through the back
    buffers + dsm_frames_advance; the caller's buffers are free once the call (sync) or upload_wait (others) returned"""
    from direct_stereo_slam_amd.tracker import pinned_array

    und, (trk,), tabs, nl = _setup(ctx, "robotcar_preset2", "G+vig")
    w_in, h_in = und.original_size
    rng = np.random.default_rng(3)
    for pinned in (False, True):
        for pad, y0 in ((0, 0), (4, 1), (7, 2)):
            shape = (h_in + y0 + 1, w_in + pad)
            cam = [pinned_array(shape, np.uint8) if pinned else np.empty(shape, np.uint8) for _ in range(2)]
            for c in cam:
                c[...] = rng.integers(0, 256, shape, dtype=np.uint8)
            views = [c[y0:y0 + h_in, pad:pad + w_in] for c in cam]
            want = [np.ascontiguousarray(v).copy() for v in views]
            if form == "async":
                ctx.upload_images_undistorted(und, [trk, trk], [2, 3], views, form="async")
                ctx.upload_wait()
                ctx.advance_frames([trk, trk], [0, 1])
            else:
                ctx.upload_images_undistorted(und, [trk, trk], [0, 1], views, form=form)
                if form == "enqueue":
                    ctx.upload_wait()
            for c in cam:
                c[...] = 0  # must not affect the pyramids
            for s in (0, 1):
                _check(trk, s, want[s], tabs, nl)


@pytest.mark.parametrize("pinned", [False, True])
def test_forty_images_in_one_call(ctx, pinned):
    """more than two copy groups; robotcar's 972 800 camera bytes grow the 542 720-byte staging buffers"""
    from direct_stereo_slam_amd.tracker import pinned_array

    und, trks, tabs, nl = _setup(ctx, "robotcar_preset2", "G", n_trackers=20)
    rng = np.random.default_rng(4 + pinned)
    imgs = _raw(rng, und, 40)
    if pinned:
        pin = [pinned_array(im.shape, np.uint8) for im in imgs]
        for p, im in zip(pin, imgs):
            p[...] = im
        src = pin
    else:
        src = imgs
    ctx.upload_images_undistorted(und, trks + trks, [0] * 20 + [1] * 20, src, np.linspace(0.5, 2.0, 40))
    for i in (0, 7, 19, 20, 33, 39):
        _check((trks + trks)[i], i // 20, imgs[i], tabs, nl)


def test_none_matches_the_plain_u8_hand_over(ctx):
    from direct_stereo_slam_amd.tracker import TrackerAndScaler, Undistorter

    calib, size_in = (718.8560, 718.8560, 607.1928, 185.2157), (1241, 376)
    und = Undistorter.pinhole(ctx, calib=calib, size_in=size_in, mode="none")
    np.testing.assert_array_equal(und.K, np.float32(calib))
    a, b = (TrackerAndScaler(ctx, 1241, 376, 5, S.KITTI_T_STEREO, und.K) for _ in range(2))
    imgs = _raw(np.random.default_rng(6), und, 2)
    ctx.upload_images_undistorted(und, [a, a], [0, 1], imgs)
    ctx.upload_images([b, b], [0, 1], imgs)
    for s in (0, 1):
        for lvl in range(5):
            np.testing.assert_array_equal(a.get_frame(s, lvl), b.get_frame(s, lvl))


def test_geometry_matches_a_frame_rendered_at_the_output_camera(ctx):
    """a plane rendered at the raw KITTI camera (1241 x 376), quantised to bytes and undistorted on the device, against the
    same plane rendered directly at the builder's K' (1232 x 368): interior intensities agree to interpolation error and
    tracking either frame gives the same result"""
    from direct_stereo_slam_amd.tracker import TrackerAndScaler, Undistorter

    calib, size_in, size_out, nl = (718.8560, 718.8560, 607.1928, 185.2157), (1241, 376), (1232, 368), 5
    und = Undistorter.pinhole(ctx, calib=calib, size_in=size_in, size_out=size_out)
    Kp = tuple(float(v) for v in und.K)
    (w, h), (w_in, h_in) = size_out, size_in
    q = lambda im: np.clip(np.rint(im), 0, 255).astype(np.uint8)  # noqa: E731
    scene = S.PlaneScene(seed=31, fx_ref=Kp[0], wavelength_px=(16.0, 128.0))
    rng = np.random.default_rng(31)
    ref = q(scene.render(Kp, w, h)).astype(np.float32)
    ref_p = O.make_images(ref, nl)
    tpl = S.dense_template(scene, Kp, w, h, nl, ref_p)
    R_, t_ = S.random_motion(rng)
    T = S.KITTI_T_STEREO
    raw = [q(scene.render(calib, w_in, h_in, R_, t_, a=0.02, b=3.0)), q(scene.render(calib, w_in, h_in, T[:3, :3], T[:3, 3]))]
    direct = [q(scene.render(Kp, w, h, R_, t_, a=0.02, b=3.0)), q(scene.render(Kp, w, h, T[:3, :3], T[:3, 3]))]
    a, b = (TrackerAndScaler(ctx, w, h, nl, T, Kp) for _ in range(2))
    for trk in (a, b):
        trk.makeK(*Kp)
        trk.setCoarseTrackingRef(0, (0.0, 0.0), 1.0, *tpl)
    ctx.upload_images_undistorted(und, [a, a], [0, 1], raw)
    ctx.upload_images([b, b], [0, 1], direct)
    m = 8
    diff = np.abs(a.get_frame(0, 0)[m:-m, m:-m, 0] - direct[0][m:-m, m:-m].astype(np.float32))
    mad = float(diff.mean())
    print(f"interior mean absolute difference: {mad:.4f} grey levels")
    assert mad < 1.0
    ra = a.trackNewestCoarse(S.IDENTITY_POSE, (0.0, 0.0), nl - 1)
    rb = b.trackNewestCoarse(S.IDENTITY_POSE, (0.0, 0.0), nl - 1)
    print("pose difference:", np.abs(ra[1] - rb[1]).max())
    assert ra[0] == rb[0]
    assert np.abs(ra[1] - rb[1]).max() < 1e-3


def test_errors_leave_the_previous_pyramid(ctx):
    from direct_stereo_slam_amd.tracker import TrackerAndScaler, Undistorter, pinhole_undistort_map

    calib, size_in = (983.044006, 983.044006, 643.646973, 493.378998), (1280, 760)
    K, _, rx, ry = pinhole_undistort_map(calib, size_in, "crop", (424, 320))
    # a table entry whose 2x2 footprint leaves the source is refused, and named
    for bad in ((1279.0, 5.0), (3.0, 759.0), (np.nan, 4.0), (2.0, -0.5)):
        bx, by = rx.copy(), ry.copy()
        bx[5, 7], by[5, 7] = bad
        with pytest.raises(DsmError, match=r"remap entry 2127 \(x = 7, y = 5\)"):
            Undistorter(ctx, size_in, (424, 320), bx, by)
    with pytest.raises(DsmError):  # passthrough needs the input size
        Undistorter(ctx, size_in, (424, 320))
    und = Undistorter(ctx, size_in, (424, 320), rx, ry)
    trk = TrackerAndScaler(ctx, 424, 320, 4, S.KITTI_T_STEREO, K)
    other = TrackerAndScaler(ctx, 416, 320, 4, S.KITTI_T_STEREO, K)
    rng = np.random.default_rng(7)
    imgs = _raw(rng, und, 3)
    ctx.upload_images_undistorted(und, [trk, trk], [0, 1], imgs[:2])
    before = [[trk.get_frame(s, l) for l in range(4)] for s in (0, 1)]
    with pytest.raises(DsmError, match="output size"):  # tracker geometry mismatch
        ctx.upload_images_undistorted(und, [other], [0], [imgs[2]])
    with pytest.raises(DsmError):
        ctx.upload_images_undistorted(und, [trk, other], [0, 0], [imgs[2], imgs[2]])
    with pytest.raises(DsmError, match="same slot twice"):
        ctx.upload_images_undistorted(und, [trk, trk], [0, 0], [imgs[2], imgs[2]])
    with pytest.raises(DsmError):  # the enqueue form takes front buffers only
        ctx.upload_images_undistorted(und, [trk], [2], [imgs[2]], form="enqueue")
    with pytest.raises(ValueError):  # not the undistorter's input size
        ctx.upload_images_undistorted(und, [trk], [0], [imgs[2][:, :-1]])
    for s in (0, 1):
        for lvl in range(4):
            np.testing.assert_array_equal(trk.get_frame(s, lvl), before[s][lvl])


def test_cpp_demo_gives_the_python_level_0(ctx, tmp_path):
    """host/undistort_demo (Undistort.hpp: camera file + G + vignette -> Undistort::uploadImage) produces the level-0 plane of
    the Python path"""
    import subprocess

    und, (trk,), tabs, nl = _setup(ctx, "robotcar_preset2", "G+vig")
    img = _raw(np.random.default_rng(8), und, 1)[0]
    ctx.upload_images_undistorted(und, [trk], [0], [img])
    _, G, vig = tabs[0], tabs[2], tabs[3]
    paths = {k: str(tmp_path / k) for k in ("raw.u8", "out.f32", "G.f32", "vig.f32")}
    img.tofile(paths["raw.u8"])
    G.tofile(paths["G.f32"])
    vig.tofile(paths["vig.f32"])
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "direct_stereo_slam_amd", "host", "_build", "undistort_demo")
    out = subprocess.run([exe, CONFIGS["robotcar_preset2"][0], paths["raw.u8"], paths["out.f32"], "424", "320", paths["G.f32"], paths["vig.f32"]],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    plane = np.fromfile(paths["out.f32"], np.float32).reshape(320, 424)
    np.testing.assert_array_equal(plane, trk.get_frame(0, 0)[..., 0])
