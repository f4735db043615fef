"""The pinhole camera of include/nerf_hip.h "pinhole camera" (csrc/camera.h) in numpy (a helper module, not a test): the one
reference of the camera for tests/_tsdf_ref.py, _raster_ref.py and _project_ref.py.  Every float step is a float32 array operation
in the header's order (numpy rounds each on its own; its division is correctly rounded), so the bits are the kernels'."""
import numpy as np

F32 = np.float32


def view_of(c2w, K):
    """float32 [16]: c2w [3, 4] row-major, then fx, fy, cx, cy, each cast once from the doubles (nerf_tsdf_view;
    engine.mesh.tsdf_views)."""
    v = np.empty(16, F32)
    v[:12] = np.asarray(c2w, np.float64)[:3, :4].reshape(12)
    K = np.asarray(K, np.float64)
    v[12:] = [K[0, 0], K[1, 1], K[0, 2], K[1, 2]]
    return v


def intrinsics(H, W, fov=0.9):
    f = 0.5 * W / np.tan(0.5 * fov)
    return np.array([[f, 0.0, 0.5 * W], [0.0, f, 0.5 * H], [0.0, 0.0, 1.0]])


def look_at(eye, target=(0.0, 0.0, 0.0), up=(0.0, 0.0, 1.0)):
    """c2w [3, 4] float64 of a camera at `eye` looking at `target` along its -z, x to the right, +y up in the image; a view along
    `up` (within 8 degrees) takes +y for it."""
    eye, target, up = (np.asarray(x, np.float64) for x in (eye, target, up))
    zax = eye - target
    zax /= np.linalg.norm(zax)
    if abs(np.dot(zax, up)) > 0.99:
        up = np.array([0.0, 1.0, 0.0])
    xax = np.cross(up, zax)
    xax /= np.linalg.norm(xax)
    yax = np.cross(zax, xax)
    return np.concatenate([np.stack([xax, yax, zax], 1), eye[:, None]], 1)


def point(p, view):
    """(xc, yc, zc) float32 of points p [n, 3] float32: camera_point."""
    p = np.asarray(p, F32).reshape(-1, 3)
    c = np.asarray(view, F32)
    with np.errstate(all="ignore"):
        q0, q1, q2 = p[:, 0] - c[3], p[:, 1] - c[7], p[:, 2] - c[11]
        xc = (c[0] * q0 + c[4] * q1) + c[8] * q2
        yc = (c[1] * q0 + c[5] * q1) + c[9] * q2
        zw = (c[2] * q0 + c[6] * q1) + c[10] * q2
        zc = F32(0.0) - zw
    return xc.astype(F32), yc.astype(F32), zc.astype(F32)


def project(p, view):
    """(u, v, zc) float32 of points p [n, 3] float32: camera_point, then camera_pixel (whatever zc is)."""
    c = np.asarray(view, F32)
    xc, yc, zc = point(p, view)
    with np.errstate(all="ignore"):
        u = c[12] * (xc / zc) + c[14]
        v = c[15] - c[13] * (yc / zc)
    return u.astype(F32), v.astype(F32), zc


def nearest(u, v, H, W):
    """(inside bool, pix int64) of the pixel of an H x W map nearest to (u, v): camera_nearest.  NaN and +-inf are outside; pix is 0
    there."""
    with np.errstate(all="ignore"):
        fu, fv = np.floor(u + F32(0.5)), np.floor(v + F32(0.5))
        inside = (fu >= 0) & (fu < F32(W)) & (fv >= 0) & (fv < F32(H))
    return inside, np.where(inside, fv, 0).astype(np.int64) * W + np.where(inside, fu, 0).astype(np.int64)
