"""Box wireframes as PLY files: what a user looks at after an evaluation, as the reference's
`scripts/visualize_grounding.py` and `scripts/visualize_captioning.py` write it -- every predicted and ground-truth box a mesh of
twelve cylinders, 1320 vertices and 2400 triangles, ASCII PLY -- without the reference's Python loop per vertex (about 32 ms per
box on a CPU) and its per-vertex `str.format`.

csrc/visualize.hip computes the vertices AND their decimal text: `write_box_plys` runs one d3_box_wire_text launch and one
read-back per chunk of boxes, then the host writes, per file, a constant header, the box's bytes as they came back and a constant
face block.  The host does no arithmetic and no formatting of coordinates.  Every file is byte-equal to the reference's
(tests/golden/visualize_golden.npz holds files its own functions wrote).

Two places differ from the reference on purpose.  (1) A box with a zero extent, a non-finite coordinate or |coordinate| >= 1e5 is
refused (or dropped, on_degenerate="skip"); the reference prints 110 lines of `nan nan nan` per zero-length edge.  (2)
`write_aligned_mesh` writes the scene's mesh.ply itself; the reference writes it through plyfile, which is not a dependency here, so
that file is NOT claimed to be byte-equal (see its docstring).  No CPU fallback: the vertices and the text come from the GPU.
"""
import ctypes as C
import math
import os

import numpy as np
import torch

from . import _lib
from ._call import call, on, ptr, stream

EDGES, STACKS, SLICES, RADIUS = 12, 10, 10, 0.03
VERTS_PER_BOX = EDGES * (STACKS + 1) * SLICES           # 1320
FACES_PER_BOX = EDGES * STACKS * SLICES * 2             # 2400
MAX_COORDINATE = 1e5
PALETTE = {0: (0, 255, 0), 1: (0, 0, 255)}              # visualize_grounding.py:152-155: 0 = gt, 1 = pred
_TINY = np.float32(1.17549435e-38)
_STATUS_TEXT = {1: "a coordinate that is not finite or not below 1e5 in magnitude", 2: "an extent of zero", 4: "a mode other than 0 and 1"}
_cache = {}


def _ring():
    """0.03 cos / sin of the ten slice angles from the host's libm (create_cylinder_mesh, visualize_grounding.py:81-82)"""
    if "ring" not in _cache:
        theta = [i2 * 2.0 * math.pi / SLICES for i2 in range(SLICES)]
        _cache["ring"] = (C.c_double * 20)(*([RADIUS * math.cos(t) for t in theta] + [RADIUS * math.sin(t) for t in theta]))
    return _cache["ring"]


def wire_faces():
    """(2400, 3) int32, read-only: per edge k and (stack i, slice i2) the triangles ((i+1) S + i2, i S + i2, i S + n) and
    ((i+1) S + i2, i S + n, (i+1) S + n) with n = (i2 + 1) mod S, S = 10, plus the edge's vertex offset 110 k
    (visualize_grounding.py:84-88, :160-163).  The same for every box."""
    if "faces" not in _cache:
        i, i2 = np.meshgrid(np.arange(STACKS), np.arange(SLICES), indexing="ij")
        n = (i2 + 1) % SLICES
        a, b, c, d = (i + 1) * SLICES + i2, i * SLICES + i2, i * SLICES + n, (i + 1) * SLICES + n
        one = np.stack([np.stack([a, b, c], -1), np.stack([a, c, d], -1)], 2).reshape(-1, 3)
        f = (one[None] + (np.arange(EDGES) * (STACKS + 1) * SLICES)[:, None, None]).reshape(-1, 3).astype(np.int32)
        f.setflags(write=False)
        _cache["faces"] = f
    return _cache["faces"]


def _file_parts():
    """(header, face block) of every box file (write_ply, visualize_grounding.py:26-38, :41-42); mind 'ply ' with its space"""
    if "parts" not in _cache:
        header = ("ply \nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                  "property uchar red\nproperty uchar green\nproperty uchar blue\nelement face %d\n"
                  "property list uchar uint vertex_indices\nend_header\n" % (VERTS_PER_BOX, FACES_PER_BOX)).encode()
        _cache["parts"] = (header, "".join("3 %d %d %d\n" % tuple(f) for f in wire_faces().tolist()).encode())
    return _cache["parts"]


def _limits():
    if "limits" not in _cache:
        v, s, f = C.c_int(0), C.c_int(0), C.c_int(0)
        _lib.check(_lib.lib().d3_box_wire_limits(C.byref(v), C.byref(s), C.byref(f)), "box_wire_limits")
        if v.value != VERTS_PER_BOX:
            raise _lib.D3Error("libd3hip.so builds %d vertices per box, this module %d" % (v.value, VERTS_PER_BOX))
        _cache["limits"] = (s.value, f.value)
    return _cache["limits"]


def host_box_status(corners):
    """(M,) int status of host boxes by the library's limits, without the library: 1 a coordinate not finite or |c| >= 1e5, 2 an
    extent whose float32 square is not a normal positive number (a zero extent), 0 fine"""
    c = np.asarray(corners, np.float64).reshape(-1, 8, 3)
    with np.errstate(all="ignore"):
        bad_c = ~(np.abs(c) < MAX_COORDINATE).all(axis=(1, 2))
        d = (c.max(axis=1) - c.min(axis=1)).astype(np.float32)
        bad_e = ~((d * d) >= _TINY).all(axis=1)
    return np.where(bad_c, 1, np.where(bad_e, 2, 0))


def _boxes(corners, modes, name, on_degenerate):
    """-> (corners: cuda float64 (M,8,3) tensor or host float64 array, modes likewise int32, kept indices or None, is_device, the
    number of boxes given).  Host inputs are checked here, before the library is touched."""
    if on_degenerate not in ("raise", "skip"):
        raise ValueError("%s: on_degenerate is 'raise' or 'skip', got %r" % (name, on_degenerate))
    dev_in = torch.is_tensor(corners) and corners.is_cuda
    if dev_in:
        c = corners.detach()
        if c.dim() != 3 or tuple(c.shape[1:]) != (8, 3) or c.dtype not in (torch.float32, torch.float64):
            raise ValueError("%s: corners (M,8,3) float32 or float64 expected, got %s %s" % (name, tuple(c.shape), c.dtype))
        c = c.double().contiguous()
    else:
        c = corners.detach().numpy() if torch.is_tensor(corners) else np.asarray(corners)
        if c.ndim != 3 or c.shape[1:] != (8, 3) or c.dtype.kind not in "fiu":
            raise ValueError("%s: corners (M,8,3) of numbers expected, got %s %s" % (name, c.shape, c.dtype))
        c = np.ascontiguousarray(c, np.float64)
    M = c.shape[0]
    if torch.is_tensor(modes) and modes.is_cuda:
        if not dev_in:
            raise ValueError("%s: modes on the GPU need corners on the GPU" % name)
        m = modes.detach().to(torch.int32).contiguous()
    else:
        m = np.ascontiguousarray(modes.numpy() if torch.is_tensor(modes) else np.asarray(modes))
        if m.ndim == 0:
            m = np.full(M, m)
        if m.dtype.kind not in "iub" or not np.isin(m, (0, 1)).all():
            raise ValueError("%s: modes are 0 (ground truth) or 1 (prediction)" % name)
        m = m.astype(np.int32)
    if tuple(m.shape) != (M,):
        raise ValueError("%s: %d boxes but modes of shape %s" % (name, M, tuple(m.shape)))
    kept = None
    if not dev_in:
        st = host_box_status(c)
        if st.any():
            first = int(np.flatnonzero(st)[0])
            if on_degenerate == "raise":
                raise ValueError("%s: box %d has %s" % (name, first, _STATUS_TEXT[int(st[first])]))
            kept = np.flatnonzero(st == 0)
            c, m = c[kept], m[kept]
    return c, m, kept, dev_in, M


def _upload(c, m, device):
    device = torch.device(device)
    if torch.is_tensor(c):
        if device.index is not None and c.device != device:
            raise ValueError("the boxes are on %s, not on %s" % (c.device, device))
        return c, (m if torch.is_tensor(m) else torch.from_numpy(m).to(c.device))
    if device.type != "cuda":
        raise ValueError("the wireframes are computed on the GPU, there is no CPU fallback (device %s)" % device)
    both = torch.from_numpy(np.concatenate([c.reshape(-1), m.astype(np.float64)])).to(device)          # one upload
    return both[:c.size].view(-1, 8, 3), both[c.size:].to(torch.int32)


def _raise_status(name, status, offset=0):
    bits, first = int(status[0]), int(status[1])
    text = "; ".join(t for b, t in sorted(_STATUS_TEXT.items()) if bits & b)
    raise _lib.D3Error("%s: box %d is the first outside the limits (%s)" % (name, first + offset, text))


def box_wireframes(corners, modes, device="cuda"):
    """corners (M,8,3) float32 / float64 (numpy, nested lists or a tensor on either side), modes (M,) of 0 = ground truth, 1 =
    prediction -> (verts, faces, colors): verts (M,1320,3) float64 on the device, exactly the doubles the reference formats (one
    d3_box_wire_verts launch, nothing read back but the status word); faces the constant (2400,3) int32 host array of `wire_faces`;
    colors (M,3) uint8 host array, `0 255 0` or `0 0 255` per box.  Raises on a box outside the limits (module docstring)."""
    name = "box_wireframes"
    c, m, _, dev_in, M = _boxes(corners, modes, name, "raise")
    colors = np.array([PALETTE[0], PALETTE[1]], np.uint8)[(m.cpu().numpy() if torch.is_tensor(m) else m)]
    if M == 0:
        return torch.zeros((0, VERTS_PER_BOX, 3), dtype=torch.float64, device=device), wire_faces(), colors
    c, m = _upload(c, m, device)
    _limits()
    verts = torch.empty((M, VERTS_PER_BOX, 3), dtype=torch.float64, device=c.device)
    status = torch.tensor([0, 0x7fffffff], dtype=torch.int32, device=c.device)
    with on(c.device):
        call("box_wire_verts", ptr(c), M, _ring(), ptr(verts), ptr(status), stream())
    st = status.cpu().numpy()
    if st[0]:
        _raise_status(name, st)
    return verts, wire_faces(), colors


def format_f6(values, device="cuda"):
    """"{:f}".format(v) of every double, formatted on the device (d3_format_f6) -> list of str.  |v| >= 1e15 (finite) is refused."""
    if torch.is_tensor(values) and values.is_cuda:
        v = values.detach().double().contiguous().view(-1)
    else:
        v = torch.from_numpy(np.ascontiguousarray(values, np.float64).reshape(-1)).to(device)
    n = v.numel()
    if n == 0:
        return []
    slot = _limits()[1]
    buf = torch.empty(8 + 4 * n + slot * n, dtype=torch.uint8, device=v.device)
    buf[:8].zero_()
    with on(v.device):
        call("format_f6", ptr(v), n, ptr(buf[8 + 4 * n:]), ptr(buf[8:]), ptr(buf), stream())
    host = buf.cpu().numpy()
    lens = host[8:8 + 4 * n].view(np.int32)
    if host[:4].view(np.int32)[0]:
        raise _lib.D3Error("format_f6: value %d is finite with a magnitude of 1e15 or more" % int(np.flatnonzero(lens < 0)[0]))
    text = host[8 + 4 * n:].reshape(n, slot)
    return [text[i, :l].tobytes().decode("ascii") for i, l in enumerate(lens.tolist())]


def write_box_plys(corners, modes, paths, chunk=4096, device="cuda", on_degenerate="raise", timings=None):
    """One PLY file per box, byte-equal to the reference's `write_bbox(corners[i], modes[i], paths[i])`
    (scripts/visualize_grounding.py:45-168).  Per chunk of boxes one d3_box_wire_text launch and one read-back (status, byte counts
    and text in one buffer); the host writes header, the box's bytes and the face block.  -> the list of paths written.

    Limits (module docstring): host inputs (numpy, lists, host tensors) are checked before any launch and raise ValueError; inputs
    on the device are checked by the kernel and raise D3Error, naming the first bad box, with no file of this call left on disk.
    on_degenerate="skip" drops such boxes instead.  Directories must exist.  timings: a dict that receives the seconds spent in
    launch + read-back ("device_s") and in writing files ("files_s"), for tools/visualize_time.py."""
    import time
    name = "write_box_plys"
    paths = list(paths)
    c, m, kept, dev_in, given = _boxes(corners, modes, name, on_degenerate)
    if len(paths) != given:
        raise ValueError("%s: %d paths for %d boxes" % (name, len(paths), given))
    total = c.shape[0]
    if kept is not None:
        paths = [paths[i] for i in kept.tolist()]
    if chunk < 1:
        raise ValueError("%s: chunk >= 1" % name)
    if total == 0:
        return []
    c, m = _upload(c, m, device)
    stride = _limits()[0]
    header, face_block = _file_parts()
    n_max = min(int(chunk), total)
    buf = torch.empty(8 + 4 * n_max + stride * n_max, dtype=torch.uint8, device=c.device)
    init = torch.tensor([0, 0x7fffffff], dtype=torch.int32, device=c.device).view(torch.uint8)
    written = []
    for lo in range(0, total, n_max):
        n = min(n_max, total - lo)
        t0 = time.perf_counter()
        buf[:8].copy_(init)
        with on(c.device):
            call("box_wire_text", ptr(c[lo:]), ptr(m[lo:]), n, _ring(), ptr(buf[8 + 4 * n_max:]), ptr(buf[8:]), ptr(buf), stream())
        host = buf[:8 + 4 * n_max + stride * n].cpu().numpy()                       # the one read-back
        status, nbytes = host[:8].view(np.int32), host[8:8 + 4 * n].view(np.int32)
        t1 = time.perf_counter()
        if status[0] and on_degenerate == "raise":
            for path in written:
                os.remove(path)
            _raise_status(name, status, lo)
        text = memoryview(host)[8 + 4 * n_max:]
        for b in range(n):
            if nbytes[b] == 0:
                continue                                                            # a dropped box (on_degenerate="skip")
            with open(paths[lo + b], "wb") as f:
                f.write(header)
                f.write(text[b * stride:b * stride + int(nbytes[b])])
                f.write(face_block)
            written.append(paths[lo + b])
        if timings is not None:
            timings["device_s"] = timings.get("device_s", 0.0) + (t1 - t0)
            timings["files_s"] = timings.get("files_s", 0.0) + (time.perf_counter() - t1)
    return written


def _stacked(boxes):
    """a list of (8,3) boxes, all on the device or all on the host -> one (M,8,3) tensor / float64 array"""
    on_dev = [torch.is_tensor(b) and b.is_cuda for b in boxes]
    if any(on_dev):
        if not all(on_dev):
            raise ValueError("the boxes of one call live on one side: all on the GPU or all on the host")
        return torch.stack([b.detach().reshape(8, 3) for b in boxes])
    arrays = [np.asarray(b.detach().numpy() if torch.is_tensor(b) else b) for b in boxes]
    for a in arrays:
        if a.shape != (8, 3):
            raise ValueError("a box is (8,3) corners, got %s" % (a.shape,))
    # float32 and float64 boxes widen exactly; the reference subtracts in the box's own dtype, which rounds to the same float32
    return np.stack([a.astype(np.float64) for a in arrays]) if arrays else np.zeros((0, 8, 3))


def visualize_grounding(predictions, root, per_annotation_boxes=False, chunk=4096, device="cuda", on_degenerate="raise"):
    """scripts/visualize_grounding.py:267-295 (visualize): `predictions` is {scene: {object: {ann: {"pred_bbox", "gt_bbox", ...}}}}
    as `GroundingEvaluator.predictions()` returns it (numpy boxes) or as `GroundingEvaluator.device_predictions()` returns it (the
    same tree, the boxes rows of the evaluator's device records: nothing is read back and uploaded again).  Writes
    <root>/<scene>/gt-<object>.ply (the first annotation's gt_bbox, green) and <root>/<scene>/pred-<object>-<ann>.ply (blue).

    The reference writes the FIRST annotation's predicted box under every annotation's name (its line 291 reads `ann_ids[0]`); the
    default reproduces that, so that the files equal the reference's.  per_annotation_boxes=True writes each annotation's own box.
    -> the list of paths written."""
    os.makedirs(root, exist_ok=True)
    boxes, modes, paths = [], [], []
    for scene, objects in predictions.items():
        scene_root = os.path.join(root, scene)
        os.makedirs(scene_root, exist_ok=True)
        for obj, anns in objects.items():
            ids = list(anns.keys())
            boxes.append(anns[ids[0]]["gt_bbox"]); modes.append(0); paths.append(os.path.join(scene_root, "gt-{}.ply".format(obj)))
            for a in ids:
                boxes.append(anns[a if per_annotation_boxes else ids[0]]["pred_bbox"]); modes.append(1)
                paths.append(os.path.join(scene_root, "pred-{}-{}.ply".format(obj, a)))
    if not boxes:
        return []
    return write_box_plys(_stacked(boxes), np.array(modes, np.int32), paths, chunk=chunk, device=device, on_degenerate=on_degenerate)


def visualize_captioning(candidates, root, chunk=4096, device="cuda", on_degenerate="raise"):
    """scripts/visualize_captioning.py:268-293 (visualize) without its mesh.ply (see `write_aligned_mesh`): `candidates` maps
    "scene|object" (further `|` fields are ignored) to the dict of `caption_eval.assign_dense_caption` ("box", "gt_box") or to the
    reference's list, whose items 2 and 3 are the predicted and the ground-truth box.  Writes <root>/<scene>/pred-<object>.ply
    (blue) and <root>/<scene>/gt-<object>.ply (green).  -> the list of paths written."""
    os.makedirs(root, exist_ok=True)
    boxes, modes, paths = [], [], []
    for key, value in candidates.items():
        fields = key.split("|")
        if len(fields) < 2:
            raise ValueError("visualize_captioning: key %r is not 'scene|object'" % (key,))
        scene_root = os.path.join(root, fields[0])
        os.makedirs(scene_root, exist_ok=True)
        pred, gt = (value["box"], value["gt_box"]) if isinstance(value, dict) else (value[2], value[3])
        boxes += [pred, gt]; modes += [1, 0]
        paths += [os.path.join(scene_root, "pred-{}.ply".format(fields[1])), os.path.join(scene_root, "gt-{}.ply".format(fields[1]))]
    if not boxes:
        return []
    return write_box_plys(_stacked(boxes), np.array(modes, np.int32), paths, chunk=chunk, device=device, on_degenerate=on_degenerate)


MESH_PLY_VERTEX = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])


def write_aligned_mesh(export_or_scan_dir, path, faces=None):
    """The axis-aligned scene mesh that scripts/visualize_captioning.py:218-254 (align_mesh, visualize_aligned_mesh) puts beside the
    boxes as mesh.ply: vertices `float x, y, z`, `uchar red, green, blue`, faces `list uchar int vertex_indices`, binary little-endian.

    export_or_scan_dir: a raw scan directory (the mesh is read and aligned on the host exactly as align_mesh does: a float64 dot
    with the axisAlignment matrix, stored as float32) or a `scan_export.ScanExport`, whose aligned mesh is taken from the device;
    a ScanExport carries no faces, so `faces` -- an (F,3) integer array, a scan_export.FACE_DTYPE array or the scan directory -- is
    then required.

    The reference writes this file through plyfile, which is not installed where this library is built and tested: the header's
    wording (comments, property order of what plyfile emits) was not compared, and byte-equality with the reference's mesh.ply is
    NOT claimed.  The element layout above is the reference's and is what `scan_export.read_ply` reads back."""
    from . import scan_export as SE
    if isinstance(export_or_scan_dir, (str, os.PathLike)):
        p = SE.read_scan(os.fspath(export_or_scan_dir))
        if p.align is None:
            raise ValueError("write_aligned_mesh: %s has no axisAlignment line" % p.scene_id)
        pts = np.ones((len(p.vertex), 4))
        pts[:, 0], pts[:, 1], pts[:, 2] = p.vertex["x"], p.vertex["y"], p.vertex["z"]
        xyz = np.dot(pts, p.align.T)[:, :3].astype(np.float32)
        rgb = np.stack([p.vertex["red"], p.vertex["green"], p.vertex["blue"]], 1)
        face = p.face if faces is None else faces
    else:
        mesh = export_or_scan_dir.aligned_mesh.detach()[:, :6].cpu().numpy()
        xyz, rgb = mesh[:, :3].astype(np.float32), mesh[:, 3:6].astype(np.uint8)
        if faces is None:
            raise ValueError("write_aligned_mesh: a ScanExport carries no faces; pass faces= (an array or the scan directory)")
        face = faces
    if isinstance(face, (str, os.PathLike)):
        face = SE.read_scan(os.fspath(face)).face
    face = np.asarray(face)
    tri = face["vertex_indices"] if face.dtype.names else face
    if tri.ndim != 2 or tri.shape[1] != 3 or (tri.size and (tri.min() < 0 or tri.max() >= len(xyz))):
        raise ValueError("write_aligned_mesh: faces are (F,3) indices into the %d vertices" % len(xyz))
    v = np.empty(len(xyz), MESH_PLY_VERTEX)
    v["x"], v["y"], v["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    v["red"], v["green"], v["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    f = np.empty(len(tri), SE.FACE_DTYPE)
    f["count"], f["vertex_indices"] = 3, tri
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\nelement face %d\n"
              "property list uchar int vertex_indices\nend_header\n" % (len(v), len(f))).encode()
    with open(path, "wb") as fh:
        fh.write(header)
        fh.write(v.tobytes())
        fh.write(f.tobytes())
    return path
