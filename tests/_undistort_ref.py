"""numpy float32 restatement of UPSTREAM-DSO's Pinhole undistortion (Undistort::readFromFile, makeOptimalK_crop,
UndistortPinhole::distortCoordinates, Undistort::undistort + PhotometricUndistorter::processFrame) as
dsm_pinhole_undistort_map and dsm_upload_images_undistorted restate it (deviation D1).
Every float operation is a float32 operation unless upstream rounds through double, which is spelt out."""
import numpy as np

f32 = np.float32


def _distort(cam, ofx, ofy, ocx, ocy, x, y):
    """distortCoordinates: ((x - ocx) / ofx) * fx + cx in float32"""
    fx, fy, cx, cy = cam
    ix = (x - ocx) / ofx
    iy = (y - ocy) / ofy
    return fx * ix + cx, fy * iy + cy


def input_camera(calib, w_in, h_in):
    """U1: relative calibration when cx < 1 and cy < 1, rescaled in double (parsOrg is a VecX), then read as float"""
    p = [float(v) for v in calib]
    if p[2] < 1 and p[3] < 1:
        p = [p[0] * w_in, p[1] * h_in, p[2] * w_in - 0.5, p[3] * h_in - 0.5]
    return tuple(f32(v) for v in p)


def optimal_k_crop(cam, w_in, h_in, w, h):
    one, zero = f32(1), f32(0)
    wm1, hm1 = f32(w_in - 1), f32(h_in - 1)
    t = (np.arange(100000).astype(f32) - f32(50000)) / f32(10000)
    ox, _ = _distort(cam, one, one, zero, zero, t, np.zeros_like(t))
    ok = np.nonzero((ox > 0) & (ox < wm1))[0]
    # U2: minX == 0 is "not found yet"; the first valid t is negative for every camera looking ahead
    minX = maxX = zero
    for i in ok:
        if minX == 0:
            minX = t[i]
        maxX = t[i]
    _, oy = _distort(cam, one, one, zero, zero, np.zeros_like(t), t)
    ok = np.nonzero((oy > 0) & (oy < hm1))[0]
    minY = maxY = zero
    for i in ok:
        if minY == 0:
            minY = t[i]
        maxY = t[i]
    # U3: float * double literal, rounded back to float
    minX, maxX, minY, maxY = (f32(float(v) * 1.01) for v in (minX, maxX, minY, maxY))
    ys = np.arange(h).astype(f32)
    xs = np.arange(w).astype(f32)
    for _ in range(501):
        yy = minY + (maxY - minY) * ys / (f32(h) - f32(1))
        lx, _ = _distort(cam, one, one, zero, zero, np.full(h, minX, f32), yy)
        rx, _ = _distort(cam, one, one, zero, zero, np.full(h, maxX, f32), yy)
        xx = minX + (maxX - minX) * xs / (f32(w) - f32(1))
        _, ty = _distort(cam, one, one, zero, zero, xx, np.full(w, minY, f32))
        _, by = _distort(cam, one, one, zero, zero, xx, np.full(w, maxY, f32))
        left = bool(np.any(~((lx > 0) & (lx < wm1))))
        right = bool(np.any(~((rx > 0) & (rx < wm1))))
        top = bool(np.any(~((ty > 0) & (ty < hm1))))
        bottom = bool(np.any(~((by > 0) & (by < hm1))))
        if not (left or right or top or bottom):
            break
        if (left or right) and (top or bottom):
            if (maxX - minX) > (maxY - minY):
                top = bottom = False
            else:
                left = right = False
        if left:
            minX = f32(float(minX) * 0.995)
        if right:
            maxX = f32(float(maxX) * 0.995)
        if top:
            minY = f32(float(minY) * 0.995)
        if bottom:
            maxY = f32(float(maxY) * 0.995)
    else:
        raise ValueError("makeOptimalK_crop did not converge")  # U4
    fx = (f32(w) - f32(1)) / (maxX - minX)
    fy = (f32(h) - f32(1)) / (maxY - minY)
    return np.array([fx, fy, -minX * fx, -minY * fy], f32)


def pinhole_map(calib, size_in, mode, size_out, out_calib=None):
    """(K_out float32[4], passthrough, remap_x, remap_y) as dsm_pinhole_undistort_map writes them"""
    w_in, h_in = size_in
    w, h = size_out
    cam = input_camera(calib, w_in, h_in)
    if mode == "none":
        assert (w, h) == (w_in, h_in)
        return np.array(cam, f32), True, None, None
    if mode == "crop":
        K = optimal_k_crop(cam, w_in, h_in, w, h)
    else:  # outputCalibration (float) relative to the output size
        a, b, c, d = (f32(v) for v in out_calib)
        K = np.array([a * f32(w), b * f32(h), c * f32(w) - f32(0.5), d * f32(h) - f32(0.5)], f32)
    X, Y = np.meshgrid(np.arange(w).astype(f32), np.arange(h).astype(f32))
    ix, iy = _distort(cam, K[0], K[1], K[2], K[3], X, Y)
    wm1, hm1 = f32(w_in - 1), f32(h_in - 1)
    # U5 (with upstream's slip: the iy == hOrg-1 branch writes ix)
    ix = np.where(ix == 0, f32(0.001), ix)
    iy = np.where(iy == 0, f32(0.001), iy)
    ix = np.where(ix == wm1, f32(w_in - 1.001), ix)
    ix = np.where(iy == hm1, f32(h_in - 1.001), ix)
    # U6 (iy against wOrg-1) + D1 (footprint inside: iy < hOrg-1)
    keep = (ix > 0) & (iy > 0) & (ix < wm1) & (iy < wm1) & (iy < hm1)
    return K, False, np.where(keep, ix, f32(-1)).astype(f32), np.where(keep, iy, f32(-1)).astype(f32)


def undistort(img_u8, remap_x, remap_y, G=None, vignette_inv=None):
    """level 0 of Undistort::undistort<unsigned char>(img, 1, 0, 1.0f): float32[h_out, w_out]"""
    img = np.asarray(img_u8)
    h_in, w_in = img.shape
    p = (np.asarray(G, f32)[img] if G is not None else img.astype(f32)).reshape(-1)
    if vignette_inv is not None:
        p = p * np.asarray(vignette_inv, f32).reshape(-1)
    if remap_x is None:
        return p.reshape(h_in, w_in).copy()
    x, y = np.asarray(remap_x, f32), np.asarray(remap_y, f32)
    out_side = x < 0
    xs, ys = np.where(out_side, f32(0), x), np.where(out_side, f32(0), y)
    xi, yi = xs.astype(np.int32), ys.astype(np.int32)
    ax = xs - xi.astype(f32)
    ay = ys - yi.astype(f32)
    axy = ax * ay
    b = xi + yi * w_in
    s00, s10, s01, s11 = p[b], p[b + 1], p[b + w_in], p[b + 1 + w_in]
    v = axy * s11 + (ay - axy) * s01 + (ax - axy) * s10 + (f32(1) - ax - ay + axy) * s00
    return np.where(out_side, f32(0), v).astype(f32)
