"""numpy float32 restatement of csrc/multiview.hip in the kernel's operation order (no FMA contraction, IEEE division, rint
half to even), plus the synthetic rooms the multiview golden and the GPU tests use.

`frame_params` / `frame_pixels` give the mapping of every (frame, point); `fuse` applies project_multiview_features.py:170-200
to it.  Bit-exact against the device for any input; against the reference's own torch code only where no decision sits at a
float32 rounding boundary (the golden drops such points)."""
import numpy as np

f32 = np.float32
INTRINSICS = [[37.01983, 0, 20, 0], [0, 38.52470, 15.5, 0], [0, 0, 1, 0], [0, 0, 0, 1]]
DEFAULTS = dict(intrinsic=INTRINSICS, depth_min=0.1, depth_max=4.0, image_dims=(41, 32), accuracy=0.05)


def corner_points(intrinsic, depth_min, depth_max, image_dims):
    """projection.py:18-45: the image corners unprojected in double, stored as float32 -> (8, 3)"""
    W, H = image_dims
    fx, fy, cx, cy = intrinsic[0][0], intrinsic[1][1], intrinsic[0][2], intrinsic[1][2]
    out = []
    for k, (ux, uy) in enumerate([(0, 0), (W - 1, 0), (W - 1, H - 1), (0, H - 1)] * 2):
        d = depth_min if k < 4 else depth_max
        x, y = (ux - cx) / fx, (uy - cy) / fy
        out.append([d * x, d * y, d])
    return np.array(out, dtype=np.float64).astype(f32)


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def frame_params(c2w, cp):
    """c2w (F,4,4) float32, cp (8,3) -> corners (F,8,3), normals (F,6,3) (mv_params_kernel)"""
    M = np.asarray(c2w, f32)
    cc = np.empty((M.shape[0], 8, 3), f32)
    A, B, Cc = [3, 2, 3, 0, 1, 6], [0, 1, 2, 3, 0, 5], [1, 5, 6, 7, 4, 4]
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(8):
            for r in range(3):
                v = M[:, r, 0] * cp[k, 0] + M[:, r, 1] * cp[k, 1]
                v = v + M[:, r, 2] * cp[k, 2]
                cc[:, k, r] = v + M[:, r, 3]
        n = np.stack([_cross(cc[:, A[k]] - cc[:, B[k]], cc[:, Cc[k]] - cc[:, B[k]]) for k in range(6)], 1)
    return cc, n.astype(f32)


def frame_pixels(points, depth, w2c, corners, normals, intrinsic, depth_min, depth_max, image_dims, accuracy):
    """one frame: points (N,3) float32, depth (H,W), w2c (4,4), corners (8,3), normals (6,3) -> (N,) int64 pixel v*W+u or -1
    (mv_pixel)"""
    W, H = image_dims
    x, y, z = (np.asarray(points, f32)[:, i] for i in range(3))
    ok = np.ones(x.shape, bool)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for k in range(6):
            c = corners[2] if k < 3 else corners[4]
            n = normals[k]
            dot = (x - c[0]) * n[0] + (y - c[1]) * n[1]
            dot = dot + (z - c[2]) * n[2]
            ok &= dot * f32(100) < f32(-0.5)
        cam = []
        for r in range(3):
            v = w2c[r, 0] * x + w2c[r, 1] * y
            v = v + w2c[r, 2] * z
            cam.append(v + w2c[r, 3])
        u = np.rint((cam[0] * f32(intrinsic[0][0])) / cam[2] + f32(intrinsic[0][2]))
        v = np.rint((cam[1] * f32(intrinsic[1][1])) / cam[2] + f32(intrinsic[1][2]))
        ok &= (u >= 0) & (u < W) & (v >= 0) & (v < H)
        pix = np.where(ok, np.where(ok, v, 0).astype(np.int64) * W + np.where(ok, u, 0).astype(np.int64), 0)
        d = np.asarray(depth, f32).reshape(-1)[pix]
        ok &= (d >= f32(depth_min)) & (d <= f32(depth_max)) & (np.abs(d - cam[2]) <= f32(accuracy))
    return np.where(ok, pix, -1)


def scene_pixels(points, depths, c2w, w2c, intrinsic, depth_min, depth_max, image_dims, accuracy):
    """(F, N) int64 mapping of every frame"""
    cp = corner_points(intrinsic, depth_min, depth_max, image_dims)
    cc, nn = frame_params(c2w, cp)
    w2c = np.asarray(w2c, f32)
    return np.stack([frame_pixels(points, depths[f], w2c[f], cc[f], nn[f], intrinsic, depth_min, depth_max, image_dims, accuracy)
                     for f in range(len(depths))])


def index_lists(pix):
    """(F, N) mapping -> the reference's (F, N+1) indices_3d / indices_2d"""
    F, N = pix.shape
    i3, i2 = np.zeros((F, N + 1), np.int64), np.zeros((F, N + 1), np.int64)
    for f in range(F):
        sel = np.nonzero(pix[f] >= 0)[0]
        i3[f, 0] = i2[f, 0] = len(sel)
        i3[f, 1:1 + len(sel)] = sel
        i2[f, 1:1 + len(sel)] = pix[f, sel]
    return i3, i2


def _max(a, b):
    return np.where((a > b) | np.isnan(a), a, b)


def fuse(pix, features, maxpool):
    """pix (F, N), features (F, C, H, W) -> (N, C) float32 fused over the frames with a mapped point, in order.  Touches only the
    rows a frame can change: mapped points, and (maxpool=False) unmapped empty rows that hold a -0.0 the frame's zero row
    overwrites."""
    F, N = pix.shape
    Cn = features.shape[1]
    rows = np.zeros((N, Cn), f32)
    empty = np.ones(N, bool)
    negzero = np.zeros(N, bool)          # empty rows whose bits are not all +0.0
    for f in range(F):
        m = np.nonzero(pix[f] >= 0)[0]
        if len(m) == 0:
            continue
        P = np.asarray(features[f], f32).reshape(Cn, -1).T[pix[f, m]]
        full = (P != 0).any(1)
        e = empty[m]
        if maxpool:
            rows[m[e & full]] = P[e & full]
            pool = ~e & full
            rows[m[pool]] = _max(rows[m[pool]], P[pool])
            empty[m[full]] = ~(rows[m[full]] != 0).any(1)
        else:
            sel = m[e]
            rows[sel] = P[e]
            empty[sel] = ~full[e]
            negzero[sel] = ~full[e] & np.signbit(P[e]).any(1)
            mapped = np.zeros(N, bool)
            mapped[m] = True
            z = negzero & ~mapped
            rows[z] = 0
            negzero[z] = False
    return rows


# ------------------------------------------------------------------------------------------------ synthetic rooms
def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """camera_to_world (4,4) float32 of a camera at eye looking at target (camera +z forward, +y down, ScanNet's convention)"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    zc = target - eye
    zc /= np.linalg.norm(zc)
    xc = np.cross(zc, np.asarray(up, np.float64))
    xc /= np.linalg.norm(xc)
    yc = np.cross(zc, xc)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = xc, yc, zc, eye
    return m.astype(f32)


def room_points(rng, n, extent=(6.0, 5.0, 2.6), n_boxes=4):
    """points on the walls, floor and ceiling of a box room and on the faces of n_boxes objects -> (n, 3) float32"""
    ext = np.asarray(extent)
    boxes = [(np.zeros(3), ext)]
    for _ in range(n_boxes):
        size = rng.uniform(0.4, 1.2, 3) * np.array([1, 1, 1.2])
        lo = rng.uniform(0.3, 1, 3) * (ext - size - 0.3)
        lo[2] = 0.0
        boxes.append((lo, lo + size))
    area = np.array([2 * ((b[1] - b[0])[[0, 1, 0]] * (b[1] - b[0])[[1, 2, 2]]).sum() for b in boxes])
    which = rng.choice(len(boxes), size=n, p=area / area.sum())
    pts = np.empty((n, 3))
    for i, (lo, hi) in enumerate(boxes):
        sel = np.nonzero(which == i)[0]
        q = rng.uniform(lo, hi, (len(sel), 3))
        axis = rng.randint(0, 3, len(sel))
        side = rng.randint(0, 2, len(sel))
        q[np.arange(len(sel)), axis] = np.where(side == 1, hi[axis], lo[axis])
        pts[sel] = q
    return pts.astype(f32), ext


def room_poses(rng, F, ext, away=True, inf=True):
    """F - away - inf inward-looking poses from inside the room, then one looking out through a wall and one -inf pose"""
    poses = []
    for _ in range(F - int(away) - int(inf)):
        eye = rng.uniform(0.2, 0.8, 3) * ext
        eye[2] = rng.uniform(1.0, 2.0)
        tgt = rng.uniform(0.1, 0.9, 3) * ext
        tgt[2] = rng.uniform(0.2, 1.5)
        poses.append(look_at(eye, tgt))
    if away:
        eye = np.array([0.3, 0.3, 1.5])
        poses.append(look_at(eye, eye + np.array([-1.0, -1.0, 0.1])))
    if inf:
        poses.append(np.full((4, 4), -np.inf, f32))
    return np.stack(poses).astype(f32)


def zbuffer_depth(points, c2w, intrinsic, image_dims):
    """depth (H, W) float32: the nearest point per pixel, projected in float64 (0 where no point lands)"""
    W, H = image_dims
    if not np.isfinite(c2w).all():
        return np.zeros((H, W), f32)
    w2c = np.linalg.inv(np.asarray(c2w, np.float64))
    cam = np.asarray(points, np.float64) @ w2c[:3, :3].T + w2c[:3, 3]
    front = cam[:, 2] > 1e-3
    cam = cam[front]
    u = np.rint(cam[:, 0] * intrinsic[0][0] / cam[:, 2] + intrinsic[0][2]).astype(np.int64)
    v = np.rint(cam[:, 1] * intrinsic[1][1] / cam[:, 2] + intrinsic[1][2]).astype(np.int64)
    inside = (u >= 0) & (u < W) & (v >= 0) & (v < H)
    zb = np.full(H * W, np.inf)
    np.minimum.at(zb, v[inside] * W + u[inside], cam[inside, 2])
    zb[~np.isfinite(zb)] = 0.0
    return zb.reshape(H, W).astype(f32)


def enet_features(rng, F, image_dims, zero_rows=0.1, C=128):
    """ENet-like maps (F, C, H, W) float32: sparse (3 in 4 values zero), the rest from {-0.5, 0.25, 0.5, 1}, negatives
    included, plus a share of all-zero pixel rows"""
    W, H = image_dims
    vals = np.array([-0.5, 0.25, 0.5, 1.0], f32)[rng.randint(0, 4, size=(F, C, H * W))]
    feat = np.where(rng.rand(F, C, H * W) < 0.75, f32(0), vals).astype(f32)
    zero = rng.rand(F, H * W) < zero_rows
    feat[np.broadcast_to(zero[:, None, :], feat.shape)] = 0
    return feat.reshape(F, C, H, W)


def room_scene(seed, n, F, image_dims=(41, 32), intrinsic=INTRINSICS, depth_points=None):
    """points (n,3), depths (F,H,W), poses (F,4,4), features (F,128,H,W) of one synthetic room; the depth maps are z-buffered from
    depth_points (default: the scene's own points)"""
    rng = np.random.RandomState(seed)
    pts, ext = room_points(rng, n)
    poses = room_poses(rng, F, ext)
    src = pts if depth_points is None else depth_points
    depths = np.stack([zbuffer_depth(src, p, intrinsic, image_dims) for p in poses])
    return pts, depths, poses, enet_features(rng, F, image_dims)
