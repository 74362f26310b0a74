"""CPU: dsm_pinhole_undistort_map (UPSTREAM-DSO's Pinhole remap, host code) equals the numpy float32 restatement bit for
bit, and its tables have the properties a pinhole crop must have; the camera-file parser reads the shipped calibrations."""
import os

import numpy as np
import pytest

import _undistort_ref as R

CAMS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cams")
SHIPPED = {
    "kitti": os.path.join(CAMS, "kitti", "0_2", "camera0.txt"),
    "malaga": os.path.join(CAMS, "malaga", "camera0.txt"),
    "robotcar": os.path.join(CAMS, "robotcar", "camera0.txt"),
}
# (calib, size_in, mode, size_out, out_calib)
CASES = {
    "kitti": ((718.8560, 718.8560, 607.1928, 185.2157), (1241, 376), "crop", (1232, 368), None),
    "malaga": ((795.11588, 795.11588, 517.12973, 395.59665), (1024, 768), "crop", (1024, 768), None),
    "robotcar": ((983.044006, 983.044006, 643.646973, 493.378998), (1280, 760), "crop", (1280, 760), None),
    "robotcar_preset2": ((983.044006, 983.044006, 643.646973, 493.378998), (1280, 760), "crop", (424, 320), None),
    "relative": ((0.58, 1.9, 0.49, 0.51), (640, 480), "crop", (512, 384), None),
    "explicit": ((718.8560, 718.8560, 607.1928, 185.2157), (1241, 376), "explicit", (640, 192), (0.6, 1.9, 0.5, 0.48)),
    "none": ((718.8560, 718.8560, 607.1928, 185.2157), (1241, 376), "none", (1241, 376), None),
}


def _lib_map(case):
    from direct_stereo_slam_amd.tracker import pinhole_undistort_map

    calib, size_in, mode, size_out, out_calib = CASES[case]
    return pinhole_undistort_map(calib, size_in, mode, size_out, out_calib)


@pytest.mark.parametrize("case", sorted(CASES))
def test_builder_equals_numpy_restatement(built, case):
    K, pt, rx, ry = _lib_map(case)
    Kr, ptr, rxr, ryr = R.pinhole_map(*CASES[case])
    np.testing.assert_array_equal(K, Kr)
    assert pt == ptr
    if pt:
        assert rx is None and ry is None
    else:
        np.testing.assert_array_equal(rx, rxr)
        np.testing.assert_array_equal(ry, ryr)


def test_none_is_passthrough_with_the_input_camera(built):
    K, pt, rx, _ = _lib_map("none")
    assert pt and rx is None
    np.testing.assert_array_equal(K, np.float32([718.8560, 718.8560, 607.1928, 185.2157]))


@pytest.mark.parametrize("case", ["kitti", "malaga", "robotcar", "robotcar_preset2", "relative"])
def test_crop_tables_cover_the_image_inside_the_source(built, case):
    _, size_in, _, (w, h), _ = CASES[case]
    w_in, h_in = size_in
    K, pt, rx, ry = _lib_map(case)
    assert not pt and rx.shape == (h, w)
    assert (rx >= 0).all() and (ry >= 0).all(), "a pinhole crop has no holes"
    # every bilinear footprint inside the source
    assert (rx.astype(np.int32) + 1 <= w_in - 1).all() and (ry.astype(np.int32) + 1 <= h_in - 1).all()
    # the crop reaches (to within a pixel) the border of the source on every side
    assert rx[:, 0].min() < 1 and rx[:, -1].max() > w_in - 2
    assert ry[0, :].min() < 1 and ry[-1, :].max() > h_in - 2


@pytest.mark.parametrize("case", ["kitti", "robotcar_preset2", "relative", "explicit"])
def test_entries_are_the_pinhole_homography(built, case):
    calib, size_in, _, (w, h), _ = CASES[case]
    K, _, rx, ry = _lib_map(case)
    fx, fy, cx, cy = (float(v) for v in R.input_camera(calib, *size_in))
    X, Y = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    ex = fx * (X - K[2]) / K[0] + cx  # K_in K_out^-1 (x, y, 1)
    ey = fy * (Y - K[3]) / K[1] + cy
    inside = rx >= 0
    assert inside.mean() > 0.5
    tol = 1e-5 * max(size_in)
    assert np.abs(rx[inside] - ex[inside]).max() < tol
    assert np.abs(ry[inside] - ey[inside]).max() < tol
    # and the entries the builder left out are those whose footprint is not inside the source
    w_in, h_in = size_in
    outside = ~((ex > 0) & (ex < w_in - 1) & (ey > 0) & (ey < h_in - 1))
    assert (~inside == outside).mean() > 0.999


def test_explicit_output_line_is_relative_to_the_output_size(built):
    K, pt, rx, _ = _lib_map("explicit")
    assert not pt
    np.testing.assert_array_equal(K, np.float32([np.float32(0.6) * 640, np.float32(1.9) * 192,
                                                 np.float32(0.5) * 640 - 0.5, np.float32(0.48) * 192 - 0.5]))
    assert (rx < 0).any()  # a wider field than the camera sees: holes


def test_camera_file_parser_reads_the_shipped_calibrations():
    from direct_stereo_slam_amd.tracker import read_camera_file

    for name, path in SHIPPED.items():
        cf = read_camera_file(path)
        calib, size_in, mode, size_out, _ = CASES[name]
        assert cf["calib"] == calib and cf["size_in"] == size_in and cf["mode"] == mode == "crop"
        assert cf["size_out"] == size_out and cf["out_calib"] is None


def test_shipped_files_give_the_same_map_as_their_values(built):
    from direct_stereo_slam_amd.tracker import pinhole_undistort_map, read_camera_file

    cf = read_camera_file(SHIPPED["robotcar"])
    K, _, rx, ry = pinhole_undistort_map(cf["calib"], cf["size_in"], cf["mode"], (424, 320), cf["out_calib"])
    Kr, _, rxr, ryr = R.pinhole_map(*CASES["robotcar_preset2"])
    np.testing.assert_array_equal(K, Kr)
    np.testing.assert_array_equal(rx, rxr)
    np.testing.assert_array_equal(ry, ryr)


def test_builder_argument_errors(built):
    from direct_stereo_slam_amd._lib import DsmError
    from direct_stereo_slam_amd.tracker import pinhole_undistort_map

    with pytest.raises(DsmError):  # none needs the input size
        pinhole_undistort_map((718.0, 718.0, 607.0, 185.0), (1241, 376), "none", (1232, 368))
    with pytest.raises(DsmError):  # explicit needs its line
        pinhole_undistort_map((718.0, 718.0, 607.0, 185.0), (1241, 376), "explicit", (1232, 368))
