"""Multiview feature projection on the device: the per-scene preprocessing that builds the 128 `multiview` input channels
(`conf/path.yaml: multiview_features`, enet_feats_maxpool.hdf5) from per-frame ENet feature maps, depth maps and camera poses.

Reference: lib/utils/projection.py:ProjectionHelper (compute_projection :180-238, project :240-256) and the per-scene loop of
data/scannet/project_multiview_features.py:88-205, which runs ~10 torch launches and several host syncs per frame.  Here one
call (`project_multiview_features`) projects, depth-tests and fuses all frames of a scene in HIP (csrc/multiview.hip) with no
per-frame host loop.  The host computes only world_to_camera = torch.inverse(camera_to_world) on the CPU in float32, as the
reference does per frame.

Frame order is the caller's.  The reference lists a scene's frames with `sorted(os.listdir(...))`, lexicographic over file
names ("100.jpg" before "20.jpg"); `reference_frame_order` reproduces it.  The order matters for `maxpool=False` (the first
frame that fills a row wins) and, through the emptiness tests, for `maxpool=True`.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._call import _ptr, _stream

# project_multiview_features.py:22-23
INTRINSICS = [[37.01983, 0, 20, 0], [0, 38.52470, 15.5, 0], [0, 0, 1, 0], [0, 0, 0, 1]]
DEPTH_MIN, DEPTH_MAX, IMAGE_DIMS, ACCURACY = 0.1, 4.0, [41, 32], 0.05
NUM_FEATURES = 128


def reference_frame_order(names):
    """File names of a scene's frame directory (e.g. os.listdir of its `color/`) -> frame ids in the reference's order: sorted
    lexicographically over the file names, extension dropped at the first '.' (so ["20.jpg", "100.jpg"] -> ["100", "20"])."""
    return [n.split(".")[0] for n in sorted(names)]


def limits():
    """(max points, max frames, max pixels W*H) of csrc/multiview.hip"""
    a, b, c = C.c_int(), C.c_int(), C.c_int()
    _lib.lib().d3_multiview_limits(C.byref(a), C.byref(b), C.byref(c))
    return a.value, b.value, c.value


def _device(device, *xs):
    if device is not None:
        return torch.device(device)
    for x in xs:
        if torch.is_tensor(x) and x.is_cuda:
            return x.device
    return torch.device("cuda", torch.cuda.current_device())


def _f32(x, device):
    t = torch.as_tensor(np.asarray(x, dtype=np.float32)) if not torch.is_tensor(x) else x
    return t.to(device=device, dtype=torch.float32).contiguous()


def world_to_camera(poses):
    """torch.inverse of float32 camera_to_world poses on the CPU (the reference's arithmetic; a -inf pose gives NaN)"""
    p = poses if torch.is_tensor(poses) else torch.as_tensor(np.asarray(poses, dtype=np.float32))
    return torch.inverse(p.detach().to(device="cpu", dtype=torch.float32))


class ProjectionHelper:
    """Drop-in for the reference's ProjectionHelper (projection.py:5-256) on the device.  intrinsic: 4x4 nested list (fx = [0][0],
    fy = [1][1], cx = [0][2], cy = [1][2]); image_dims = [W, H]."""

    def __init__(self, intrinsic, depth_min, depth_max, image_dims, accuracy, device=None):
        self.intrinsic = intrinsic
        self.depth_min, self.depth_max, self.accuracy = float(depth_min), float(depth_max), float(accuracy)
        self.image_dims = [int(image_dims[0]), int(image_dims[1])]
        self.device = device
        self._intr = (C.c_double * 7)(float(intrinsic[0][0]), float(intrinsic[1][1]), float(intrinsic[0][2]), float(intrinsic[1][2]),
                                      self.depth_min, self.depth_max, self.accuracy)

    # ---------------------------------------------------------------------------------------------------- validation
    def _scene(self, points, depths, poses):
        W, H = self.image_dims
        pts, dep = points, depths
        if tuple(np.shape(pts))[1:] != (3,) or len(np.shape(pts)) != 2:
            raise ValueError("points must be (N, 3), got %s" % (tuple(np.shape(pts)),))
        if len(np.shape(dep)) != 3 or tuple(np.shape(dep))[1:] != (H, W):
            raise ValueError("depths must be (F, %d, %d), got %s" % (H, W, tuple(np.shape(dep))))
        F = np.shape(dep)[0]
        if tuple(np.shape(poses)) != (F, 4, 4):
            raise ValueError("poses must be (%d, 4, 4), got %s" % (F, tuple(np.shape(poses))))
        dev = _device(self.device, points, depths, poses)
        w2c = world_to_camera(poses)
        return dev, _f32(pts, dev), _f32(dep, dev), _f32(poses, dev), w2c.to(dev).contiguous()

    # ---------------------------------------------------------------------------------------------------- mapping
    def compute_projection_batch(self, points, depths, poses):
        """compute_projection for F frames at once -> (indices_3d, indices_2d), each (F, N+1) int64 on the device: row f =
        [count, point indices ascending, zeros] / [count, pixel v * W + u, zeros]; count 0 where the reference returns None."""
        dev, pts, dep, c2w, w2c = self._scene(points, depths, poses)
        N, F = pts.shape[0], dep.shape[0]
        W, H = self.image_dims
        i3d = torch.zeros((F, N + 1), dtype=torch.int64, device=dev)
        i2d = torch.zeros((F, N + 1), dtype=torch.int64, device=dev)
        if N == 0 or F == 0:
            return i3d, i2d
        L = _lib.lib()
        need = L.d3_multiview_project_ws_bytes(N, F)
        if need == 0:
            _lib.check(-2, "multiview_project (N=%d, F=%d)" % (N, F))
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.check(L.d3_multiview_project(_ptr(pts), N, _ptr(dep), _ptr(c2w), _ptr(w2c), F, self._intr, W, H, _ptr(i3d),
                                              _ptr(i2d), _ptr(ws), need, _stream()), "multiview_project")
        return i3d, i2d

    def compute_projection(self, points, depth, camera_to_world):
        """one frame: depth (H, W), camera_to_world (4, 4) -> None when no point maps, else (indices_3d, indices_2d) int64 (N+1)"""
        d = depth.reshape(1, *depth.shape) if torch.is_tensor(depth) else np.asarray(depth)[None]
        p = camera_to_world.reshape(1, 4, 4) if torch.is_tensor(camera_to_world) else np.asarray(camera_to_world)[None]
        i3d, i2d = self.compute_projection_batch(points, d, p)
        if int(i3d[0, 0]) == 0:
            return None
        return i3d[0], i2d[0]

    def project(self, label, lin_indices_3d, lin_indices_2d, num_points):
        """label (C, H, W) or (H, W) float32 -> (C, num_points): zeros, with label's pixel lin_indices_2d[1+j] at point
        lin_indices_3d[1+j] for j < lin_indices_3d[0]"""
        dev = _device(self.device, label, lin_indices_3d)
        lab = _f32(label, dev)
        Cn = 1 if lab.dim() == 2 else lab.shape[0]
        lab = lab.reshape(Cn, -1)
        i3 = torch.as_tensor(lin_indices_3d).to(device=dev, dtype=torch.int64).contiguous()
        i2 = torch.as_tensor(lin_indices_2d).to(device=dev, dtype=torch.int64).contiguous()
        n = int(num_points)
        if i3.dim() != 1 or i2.dim() != 1 or i3.numel() != n + 1 or i2.numel() != n + 1:
            raise ValueError("index lists must both be (num_points + 1,)")
        out = torch.empty((Cn, n), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().d3_multiview_project_frame(_ptr(lab), Cn, lab.shape[1], _ptr(i3), _ptr(i2), n, _ptr(out), _stream()),
                       "multiview_project_frame")
        return out

    # ---------------------------------------------------------------------------------------------------- fused scene
    def project_scene(self, points, depths, poses, features, maxpool=True, return_counts=False):
        """see project_multiview_features"""
        W, H = self.image_dims
        F = np.shape(depths)[0] if len(np.shape(depths)) else 0
        if len(np.shape(features)) != 4 or tuple(np.shape(features))[0] != F or tuple(np.shape(features))[2:] != (H, W):
            raise ValueError("features must be (%d, %d, %d, %d), got %s" % (F, NUM_FEATURES, H, W, tuple(np.shape(features))))
        dev, pts, dep, c2w, w2c = self._scene(points, depths, poses)
        N = pts.shape[0]
        Cf = int(np.shape(features)[1])
        feat = _f32(features, dev)
        out = torch.empty((N, Cf), dtype=torch.float32, device=dev)
        counts = torch.zeros(F, dtype=torch.int32, device=dev)
        L = _lib.lib()
        need = L.d3_multiview_fuse_ws_bytes(F, W, H) if F > 0 else 0
        ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.check(L.d3_multiview_fuse(_ptr(pts), N, _ptr(dep), _ptr(c2w), _ptr(w2c), F, self._intr, W, H, _ptr(feat), Cf,
                                           int(bool(maxpool)), _ptr(out), _ptr(counts) if F > 0 else None, _ptr(ws), need,
                                           _stream()), "multiview_fuse")
        return (out, counts) if return_counts else out


_DEFAULT = None


def default_helper():
    """the reference's projector (project_multiview_features.py:22-23)"""
    global _DEFAULT
    if _DEFAULT is None:
        _DEFAULT = ProjectionHelper(INTRINSICS, DEPTH_MIN, DEPTH_MAX, IMAGE_DIMS, ACCURACY)
    return _DEFAULT


def compute_projection_batch(points, depths, poses, helper=None):
    """(F, N+1) indices_3d, indices_2d of every frame (the reference's compute_projection, project_multiview_features.py:88-114)"""
    return (helper or default_helper()).compute_projection_batch(points, depths, poses)


def project_multiview_features(points, depths, poses, features, maxpool=True, helper=None, return_counts=False):
    """One scene's multiview features: points (N,3) float32 original mesh vertices, depths (F,32,41) metres, poses (F,4,4)
    camera_to_world, features (F,128,32,41) ENet maps, frames in the caller's order (see reference_frame_order) -> (N,128) float32
    on the device, row i = vertex i: what the reference stores per scene in enet_feats(_maxpool).hdf5.  Frames with no mapped
    point are dropped (a -inf pose maps nothing).  return_counts: also the (F,) int32 mapped-point count of each frame."""
    return (helper or default_helper()).project_scene(points, depths, poses, features, maxpool=maxpool, return_counts=return_counts)
