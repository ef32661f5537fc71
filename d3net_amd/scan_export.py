"""ScanNet scan export on the device: a raw scan directory (`_vh_clean_2.ply`, `_vh_clean_2.labels.ply`, `.aggregation.json`,
`_vh_clean_2.0.010000.segs.json`, `<scene>.txt`) to the per-scan arrays that the reference's data/scannet/prepare_scannet.py
saves (export :138-178, process_one_scan :180-197) and to the instance GT codes of prepare_scannet_inst_gt.py:38-65.

The host reads the files (binary little-endian PLY through `np.frombuffer` on structured dtypes, no plyfile), parses the JSON and
meta files and builds the small object / segment tables.  Everything per vertex or per face runs in HIP (csrc/scan_export.hip):
face and vertex normals, the axis alignment, instance ids, labels, boxes of both meshes and the instance GT codes.  One
validation read per scan brings back the data-problem bits and the kept box-row count.

Deviations from the reference:
  * inputs on which it fails raise ValueError: a raw label >= 150 (IndexError), a segment listed by the aggregation that no
    vertex carries (KeyError), a segment file whose length differs from the mesh (assert), no object besides wall / floor /
    ceiling (max() of nothing), a face index >= N (IndexError), a face that is not a triangle;
  * inputs it accepts with a meaningless result also raise ValueError: a negative face index (numpy counts it from the end) and
    a negative objectId (its box row is written from the end of the array).  Negative segment ids are accepted, as in the
    reference, where they are only dictionary keys;
  * the test-split placeholder (no aggregation file) gives int64 -1 instance ids, as numpy 1.x did; under numpy 2 the reference's
    `uint32 * -1` raises.
"""
import collections
import concurrent.futures as cf
import ctypes as C
import json
import os
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from ._call import _ptr, _stream

# prepare_scannet.py:13, :23-25; prepare_scannet_inst_gt.py:15
DONOTCARE_CLASS_IDS = (1, 2, 22)
NYU40_IDS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39)
REMAPPER = np.full(150, -1.0)
REMAPPER[list(NYU40_IDS)] = np.arange(20)
IGNORED_GROUPS = ("wall", "floor", "ceiling")

MESH_SUFFIX, LABEL_SUFFIX = "_vh_clean_2.ply", "_vh_clean_2.labels.ply"
AGG_SUFFIX, SEG_SUFFIX, META_SUFFIX = ".aggregation.json", "_vh_clean_2.0.010000.segs.json", ".txt"

# flag bits of csrc/scan_export.hip
_FLAG_TEXT = {1: "a face is not a triangle", 2: "a face names a vertex outside the mesh", 4: "a raw label is 150 or more",
              8: "a segment id is outside the segment table", 16: "the aggregation lists a segment that no vertex carries",
              32: "an object table entry is outside its range or repeated"}

# ---------------------------------------------------------------------------------------------------------------- PLY
_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
              "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
              "double": "f8", "float64": "f8"}
MESH_VERTEX_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1"),
                              ("alpha", "u1")])
FACE_DTYPE = np.dtype([("count", "u1"), ("vertex_indices", "<i4", (3,))])


def _ply_header(buf):
    end = buf.find(b"end_header")
    if not buf.startswith(b"ply") or end < 0:
        raise ValueError("not a PLY file")
    nl = buf.find(b"\n", end)
    if nl < 0:
        raise ValueError("PLY header is not terminated")
    lines = [l.strip() for l in buf[:end].decode("ascii", "replace").splitlines()]
    fmt, elements = None, []
    for l in lines[1:]:
        t = l.split()
        if not t or t[0] in ("comment", "obj_info"):
            continue
        if t[0] == "format":
            fmt = t[1] if len(t) > 1 else None
        elif t[0] == "element" and len(t) == 3:
            elements.append([t[1], int(t[2]), []])
        elif t[0] == "property" and elements:
            if t[1] == "list" and len(t) == 5:
                if t[2] not in _PLY_TYPES or t[3] not in _PLY_TYPES:
                    raise ValueError("unknown PLY list type in %r" % l)
                elements[-1][2].append((t[4], ("list", _PLY_TYPES[t[2]], _PLY_TYPES[t[3]])))
            elif len(t) == 3 and t[1] in _PLY_TYPES:
                elements[-1][2].append((t[2], _PLY_TYPES[t[1]]))
            else:
                raise ValueError("unsupported PLY property %r" % l)
        else:
            raise ValueError("unsupported PLY header line %r" % l)
    if fmt != "binary_little_endian":
        raise ValueError("only binary_little_endian PLY is supported, got %r" % fmt)
    return elements, nl + 1


def _element_dtype(name, props):
    lists = [p for p in props if isinstance(p[1], tuple)]
    if not lists:
        return np.dtype([(n, "<" + t) for n, t in props])
    if len(props) != 1 or props[0][1][1] != "u1" or props[0][1][2] != "i4":
        raise ValueError("element %r: only one `list uchar int` property is supported" % name)
    return np.dtype([("count", "u1"), (props[0][0], "<i4", (3,))])


def read_ply(path_or_bytes):
    """binary little-endian PLY -> {element name: structured array (a view of the file's bytes)}.  Scalar-only elements and
    elements with one `list uchar int` property of triangles are supported; anything else raises ValueError."""
    if isinstance(path_or_bytes, (bytes, bytearray)):
        buf = path_or_bytes
    else:
        with open(path_or_bytes, "rb") as fh:      # a writable buffer: the arrays go to torch without a copy
            buf = bytearray(os.fstat(fh.fileno()).st_size)
            fh.readinto(buf)
    elements, off = _ply_header(buf)
    out = {}
    for name, count, props in elements:
        dt = _element_dtype(name, props)
        if off + count * dt.itemsize > len(buf):
            raise ValueError("PLY element %r is truncated" % name)
        a = np.frombuffer(buf, dtype=dt, count=count, offset=off)
        if "count" in dt.names and count and not (a["count"] == 3).all():
            raise ValueError("PLY element %r: only triangles are supported" % name)
        out[name] = a
        off += count * dt.itemsize
    return out


def read_mesh_ply(path_or_bytes):
    """_vh_clean_2.ply -> (vertex (N,) MESH_VERTEX_DTYPE, face (F,) FACE_DTYPE): the 7 vertex properties the reference's
    unpacking loop needs (scannet_utils.py:132) and `list uchar int vertex_indices` faces, nothing else"""
    el = read_ply(path_or_bytes)
    v, f = el.get("vertex"), el.get("face")
    if v is None or f is None:
        raise ValueError("mesh PLY needs vertex and face elements")
    if v.dtype != MESH_VERTEX_DTYPE:
        raise ValueError("mesh vertices must be float x, y, z, uchar red, green, blue, alpha; got %s" % (v.dtype,))
    if f.dtype != FACE_DTYPE:
        raise ValueError("mesh faces must be `list uchar int vertex_indices`; got %s" % (f.dtype,))
    return v, f


def read_label_ply(path_or_bytes):
    """_vh_clean_2.labels.ply -> (N,) uint16 nyu40 labels (the vertex property `label`, ushort)"""
    v = read_ply(path_or_bytes).get("vertex")
    if v is None or "label" not in v.dtype.names or v.dtype["label"] != np.dtype("<u2"):
        raise ValueError("label PLY needs a ushort vertex property `label`")
    return np.ascontiguousarray(v["label"])


# ---------------------------------------------------------------------------------------------------------------- other files
def read_axis_alignment(meta_path):
    """<scene>.txt -> (4, 4) float64 or None, parsed like read_axis_align_matrix (prepare_scannet.py:36-44): the last line that
    contains `axisAlignment`, with str.strip's character-set strip of 'axisAlignment = '"""
    m = None
    with open(meta_path) as fh:
        for line in fh.readlines():
            if "axisAlignment" in line:
                m = [float(x) for x in line.rstrip().strip("axisAlignment = ").split(" ")]
    if m:
        if len(m) != 16:
            raise ValueError("axisAlignment needs 16 numbers, got %d" % len(m))
        return np.array(m, dtype=np.float64).reshape(4, 4)
    return None


def read_segments(seg_path):
    """_vh_clean_2.0.010000.segs.json -> (N,) int64 segment id per vertex"""
    with open(seg_path) as fh:
        return np.asarray(json.load(fh)["segIndices"], dtype=np.int64)


def read_aggregation(agg_path):
    """.aggregation.json -> [(objectId, label, segments)] in file order"""
    with open(agg_path) as fh:
        data = json.load(fh)
    return [(int(g["objectId"]), g["label"], list(g["segments"])) for g in data["segGroups"]]


def object_tables(groups, scan_name):
    """read_agg_file + get_instance_ids (prepare_scannet.py:64-117) on the host's side: objects in dict order (wall / floor /
    ceiling dropped; the first object of each label also lists the later same-label objects' segments, as the reference's
    aliased lists do; for scene0217_00 the first half of the sorted ids), as (obj_id (K,), label_seg (K,), pair_seg (P,),
    pair_obj (P,)) int64.  label_seg[k] is the last segment of object k, or of the latest earlier object with segments (the
    reference's `verts` carries over an empty segment list)."""
    obj2segs, label2segs = {}, {}
    for oid, label, segs in groups:
        if label in IGNORED_GROUPS:
            continue
        segs = list(segs)
        obj2segs[oid] = segs
        # the reference keeps the first object's list itself in label2segs and extends it: that object then also lists the
        # segments of every later object with its label (prepare_scannet.py:78-82)
        if label in label2segs:
            label2segs[label].extend(segs)
        else:
            label2segs[label] = segs
    if scan_name == "scene0217_00":
        ids = sorted(obj2segs.keys())
        obj2segs = {o: obj2segs[o] for o in ids[:len(obj2segs) // 2]}
    if not obj2segs:
        raise ValueError("the aggregation names no object besides wall / floor / ceiling")
    obj_id, label_seg, pair_seg, pair_obj, last = [], [], [], [], None
    for k, (oid, segs) in enumerate(obj2segs.items()):
        if oid < 0:
            raise ValueError("negative objectId %d" % oid)
        pair_seg.extend(int(s) for s in segs)
        pair_obj.extend([k] * len(segs))
        if segs:
            last = int(segs[-1])
        if last is None:
            raise ValueError("object %d lists no segment" % oid)
        obj_id.append(oid)
        label_seg.append(last)
    return (np.asarray(obj_id, np.int64), np.asarray(label_seg, np.int64), np.asarray(pair_seg, np.int64).reshape(-1),
            np.asarray(pair_obj, np.int64).reshape(-1))


def limits():
    """(max vertices, max faces, max segment-id range, max objects, max box rows) of csrc/scan_export.hip"""
    v = [C.c_int() for _ in range(5)]
    _lib.lib().d3_scan_limits(*[C.byref(x) for x in v])
    return tuple(x.value for x in v)


# ---------------------------------------------------------------------------------------------------------------- host stage
@dataclass
class ParsedScan:
    """the host's part of one scan: file contents as arrays, ready for the device"""
    scene_id: str
    vertex: np.ndarray           # (N,) MESH_VERTEX_DTYPE
    face: np.ndarray             # (F,) FACE_DTYPE
    align: object                # (4, 4) float64 or None
    labels: object = None        # (N,) uint16, None without an aggregation file
    segments: object = None      # (N,) int64
    tables: object = None        # object_tables(...)


def scan_paths(scan_dir, scene_id):
    p = lambda s: os.path.join(scan_dir, scene_id + s)
    return dict(mesh=p(MESH_SUFFIX), labels=p(LABEL_SUFFIX), agg=p(AGG_SUFFIX), segs=p(SEG_SUFFIX), meta=p(META_SUFFIX))


def read_scan(scan_dir, scene_id=None):
    """read and parse one scan directory on the host (no device work)"""
    scan_dir = os.path.normpath(scan_dir)
    scan_name = os.path.basename(scan_dir)
    scene_id = scene_id or scan_name
    paths = scan_paths(scan_dir, scene_id)
    vertex, face = read_mesh_ply(paths["mesh"])
    p = ParsedScan(scene_id, vertex, face, read_axis_alignment(paths["meta"]))
    if os.path.isfile(paths["agg"]):
        p.labels = read_label_ply(paths["labels"])
        p.segments = read_segments(paths["segs"])
        n = len(vertex)
        if len(p.segments) != n:
            raise ValueError("%s: %d segment indices for %d vertices" % (scene_id, len(p.segments), n))
        if len(p.labels) != n:
            raise ValueError("%s: %d labels for %d vertices" % (scene_id, len(p.labels), n))
        # the reference's agg_file.split('/')[-2]: the scan directory's name decides the scene0217_00 rule
        p.tables = object_tables(read_aggregation(paths["agg"]), scan_name)
    return p


# ---------------------------------------------------------------------------------------------------------------- device stage
@dataclass
class ScanExport:
    """one exported scan as device tensors: the arrays process_one_scan saves plus the instance GT codes"""
    scene_id: str
    mesh: torch.Tensor                    # (N, 9) float32
    aligned_mesh: torch.Tensor            # (N, 9) float32
    sem_labels: torch.Tensor              # (N,) float64 in {-1, 0..19}
    instance_ids: torch.Tensor            # (N,) float64 (int64 for the placeholder)
    instance_bboxes: torch.Tensor         # (M, 8) float64
    aligned_instance_bboxes: torch.Tensor  # (M, 8) float64
    inst_gt: torch.Tensor                 # (N,) int32
    annotated: bool

    def to_reference_dict(self):
        """numpy arrays under the keys and dtypes that process_one_scan torch.saves (prepare_scannet.py:197)"""
        c = lambda t: t.detach().cpu().numpy()
        return {"mesh": c(self.mesh), "aligned_mesh": c(self.aligned_mesh), "sem_labels": c(self.sem_labels),
                "instance_ids": c(self.instance_ids), "instance_bboxes": c(self.instance_bboxes),
                "aligned_instance_bboxes": c(self.aligned_instance_bboxes)}


def _raise_flags(scene_id, bits):
    msgs = [t for b, t in sorted(_FLAG_TEXT.items()) if bits & b]
    raise ValueError("%s: %s" % (scene_id, "; ".join(msgs)))


def export_parsed(p, device=None):
    """the device stage of export_scan for a ParsedScan"""
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    L = _lib.lib()
    N, F = len(p.vertex), len(p.face)
    maxv, maxf, maxs, maxk, maxr = limits()
    if N < 1 or N > maxv or F > maxf:
        _lib.check(-2, "scan_export %s (N=%d, F=%d)" % (p.scene_id, N, F))
    with torch.cuda.device(device):
        st = _stream()
        vrec = torch.from_numpy(p.vertex.view(np.uint8)).to(device)
        frec = torch.from_numpy(p.face.view(np.uint8)).to(device) if F else None
        flags = torch.zeros(2, dtype=torch.int32, device=device)
        mesh = torch.empty((N, 9), dtype=torch.float32, device=device)
        aligned = torch.empty((N, 9), dtype=torch.float32, device=device)
        need = L.d3_scan_mesh_ws_bytes(N, F)
        ws = torch.empty(need, dtype=torch.uint8, device=device)
        al = None if p.align is None else (C.c_double * 16)(*np.ascontiguousarray(p.align, np.float64).reshape(-1).tolist())
        _lib.check(L.d3_scan_mesh(_ptr(vrec), N, _ptr(frec) if F else None, F, al, _ptr(mesh), _ptr(aligned), _ptr(flags), _ptr(ws),
                                  need, st), "d3_scan_mesh")
        if p.tables is None:
            f = flags.cpu().numpy()                                                       # the validation read
            if f[0]:
                _raise_flags(p.scene_id, int(f[0]))
            return ScanExport(p.scene_id, mesh, aligned, torch.full((N,), -1.0, dtype=torch.float64, device=device),
                              torch.full((N,), -1, dtype=torch.int64, device=device),
                              torch.zeros((1, 8), dtype=torch.float64, device=device),
                              torch.zeros((1, 8), dtype=torch.float64, device=device),
                              torch.zeros(N, dtype=torch.int32, device=device), False)
        obj_id, label_seg, pair_seg, pair_obj = p.tables
        seg = p.segments
        # segment ids are only keys to the reference (negative ones included): the device sees them shifted by the smallest id
        # of the segment file; listed segments outside that file's range cannot carry a vertex and become -1 (missing)
        base = int(seg.min())
        S, K, P, R = int(seg.max()) - base + 1, len(obj_id), len(pair_seg), int(obj_id.max()) + 1
        if S > maxs or K > maxk or R > maxr or P > (1 << 24):
            _lib.check(-2, "scan_export %s (segments=%d, objects=%d, rows=%d, pairs=%d)" % (p.scene_id, S, K, R, P))
        local = lambda a: np.where((a >= base) & (a < base + S), a - base, -1).astype(np.int32)
        # one upload of the int32 tables: segment ids, then the aggregation's pairs and objects
        tab = np.concatenate([(seg - base).astype(np.int32), local(pair_seg), pair_obj.astype(np.int32),
                              obj_id.astype(np.int32), local(label_seg)])
        tab_d = torch.from_numpy(tab).to(device)
        raw_d = torch.from_numpy(p.labels.view(np.int16)).to(device)      # the uint16 bits
        seg_d = tab_d[:N]
        o = N
        ps_d, po_d = tab_d[o:o + P], tab_d[o + P:o + 2 * P]
        o += 2 * P
        oid_d, ls_d = tab_d[o:o + K], tab_d[o + K:o + 2 * K]
        ids = torch.empty(N, dtype=torch.float64, device=device)
        sem = torch.empty(N, dtype=torch.float64, device=device)
        gt = torch.empty(N, dtype=torch.int32, device=device)
        boxes = torch.empty((R, 8), dtype=torch.float64, device=device)
        aboxes = torch.empty((R, 8), dtype=torch.float64, device=device)
        need = L.d3_scan_labels_ws_bytes(N, S, P, K, R)
        ws2 = torch.empty(need, dtype=torch.uint8, device=device)
        _lib.check(L.d3_scan_labels(_ptr(raw_d), _ptr(seg_d), N, S, _ptr(ps_d) if P else None, _ptr(po_d) if P else None, P,
                                    _ptr(oid_d), _ptr(ls_d), K, R, _ptr(mesh), _ptr(aligned), _ptr(ids), _ptr(sem), _ptr(gt),
                                    _ptr(boxes), _ptr(aboxes), _ptr(flags), _ptr(ws2), need, st), "d3_scan_labels")
        f = flags.cpu().numpy()                                                           # the validation read
        if f[0]:
            _raise_flags(p.scene_id, int(f[0]))
        kept = int(f[1])
        return ScanExport(p.scene_id, mesh, aligned, sem, ids, boxes[:kept], aboxes[:kept], gt, True)


def export_scan(scan_dir, scene_id=None, device=None):
    """One raw ScanNet scan directory -> ScanExport (device tensors): what export + process_one_scan compute
    (prepare_scannet.py:138-197) and the instance GT codes of prepare_scannet_inst_gt.py.  scene_id defaults to the directory
    name; the scene0217_00 rule follows the directory name, as in the reference."""
    return export_parsed(read_scan(scan_dir, scene_id), device)


def save_scan(export, path):
    """torch.save the reference dict (the reference's loader torch.loads it unchanged)"""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    torch.save(export.to_reference_dict(), path)


def inst_gt(export):
    """(N,) int32 instance GT codes of prepare_scannet_inst_gt.py:48-62 as a numpy array"""
    return export.inst_gt.detach().cpu().numpy()


def write_inst_gt(export, path):
    """the reference's split_gt/<split>/<scene>.txt (np.savetxt fmt='%d')"""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savetxt(path, inst_gt(export), fmt="%d")


def scene_from_export(export, multiview=None, use_color=True, use_normal=True):
    """the raw scene dict of scene_prep.prepare_scene ({"points", "feats", "sem_labels", "instance_ids"}) with the loader's
    features (lib/dataset/pipeline.py:774-802 on aligned_mesh): rgb if use_color, normals if use_normal, then multiview (N, 128)
    if given (e.g. multiview.project_multiview_features on export.mesh[:, :3])"""
    am = export.aligned_mesh
    cols = []
    if use_color:
        cols.append(am[:, 3:6])
    if use_normal:
        cols.append(am[:, 6:9])
    if multiview is not None:
        mv = multiview if torch.is_tensor(multiview) else torch.as_tensor(np.asarray(multiview))
        cols.append(mv.to(device=am.device, dtype=torch.float32))
    feats = torch.cat(cols, 1) if cols else am.new_zeros((am.shape[0], 0))
    return {"points": am[:, :3].contiguous(), "feats": feats.contiguous(), "sem_labels": export.sem_labels,
            "instance_ids": export.instance_ids}


def iter_parsed(scan_root, names, threads=16):
    """(name, ParsedScan) for every scan in `names`, in order, read on `threads` host threads (at most 16) with a bounded
    read-ahead: while the caller works on one scan, the next `threads` are being read.  Nothing is kept after it is yielded."""
    threads = max(1, min(16, int(threads)))
    names = list(names)
    with cf.ThreadPoolExecutor(max_workers=threads) as ex:
        ahead = collections.deque()
        nxt = 0
        while nxt < len(names) and len(ahead) < threads:
            ahead.append(ex.submit(read_scan, os.path.join(scan_root, names[nxt]), names[nxt]))
            nxt += 1
        for n in names:
            p = ahead.popleft().result()
            if nxt < len(names):
                ahead.append(ex.submit(read_scan, os.path.join(scan_root, names[nxt]), names[nxt]))
                nxt += 1
            yield n, p
            del p


def export_split(scan_root, names, out_root, split, threads=16, device=None, gt_root=None):
    """prepare_scannet.py's process_all_scans (+ prepare_scannet_inst_gt.py when gt_root is given): every scan in `names` to
    out_root/<split>/<scene>.pth (and gt_root/<split>/<scene>.txt).  Files are read on at most 16 host threads, up to
    `threads` scans ahead of the one being exported (iter_parsed), so host memory stays bounded for any split size.
    Returns the scene names in order."""
    names = sorted(names)
    out_dir = os.path.join(out_root, split)
    os.makedirs(out_dir, exist_ok=True)
    for n, p in iter_parsed(scan_root, names, threads):
        e = export_parsed(p, device)
        del p
        save_scan(e, os.path.join(out_dir, n + ".pth"))
        if gt_root is not None:
            write_inst_gt(e, os.path.join(gt_root, split, n + ".txt"))
        del e
    return names
