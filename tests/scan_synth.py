"""Synthetic ScanNet-format scans, deterministic per seed: `_vh_clean_2.ply`, `_vh_clean_2.labels.ply`, `.aggregation.json`,
`_vh_clean_2.0.010000.segs.json` and `<scene>.txt`, written in the layouts the ScanNet release uses.

Every scan covers: vertices named at the same corner by many faces, degenerate faces (zero normals), isolated vertices, segment
ids with gaps, segments shared by two objects, an object that loses all its vertices to later objects, objectId gaps,
wall / floor / ceiling groups and objects labelled 1, 2 and 22.  Options: no axisAlignment line, no aggregation file (the test
split), an object with an empty segment list."""
import json
import os

import numpy as np

VERTEX_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1"), ("alpha", "u1")])
LABEL_VERTEX_DTYPE = np.dtype(VERTEX_DTYPE.descr + [("label", "<u2")])
FACE_DTYPE = np.dtype([("count", "u1"), ("vertex_indices", "<i4", (3,))])
NAMES = ["chair", "table", "cabinet", "bed", "sofa", "door", "window", "bookshelf", "picture", "counter", "desk", "curtain",
         "toilet", "sink", "bathtub", "box", "lamp", "pillow"]


def make_scan(seed, n=2000, n_faces=None, n_objects=12, align=True, annotated=True, empty_object=False, extent=(6.0, 5.0, 2.6)):
    """-> dict of arrays and JSON-ready tables for one scan"""
    r = np.random.RandomState(seed)
    n_faces = 2 * n if n_faces is None else n_faces
    v = np.zeros(n, VERTEX_DTYPE)
    xyz = (r.rand(n, 3) * np.array(extent) - np.array([extent[0] / 2, extent[1] / 2, 0.0])).astype(np.float32)
    v["x"], v["y"], v["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    for c in ("red", "green", "blue"):
        v[c] = r.randint(0, 256, n)
    v["alpha"] = 255
    # faces: local triangles (a vertex and two of its index neighbours) over all but the isolated vertices
    isolated = r.choice(n, size=max(3, n // 200), replace=False)
    used = np.setdiff1d(np.arange(n), isolated)
    a = used[r.randint(0, len(used), n_faces)]
    pos = np.searchsorted(used, a)
    b = used[np.clip(pos + r.randint(1, 8, n_faces), 0, len(used) - 1)]
    c = used[np.clip(pos - r.randint(1, 8, n_faces), 0, len(used) - 1)]
    faces = np.stack([a, b, c], 1).astype(np.int32)
    nd = max(2, n_faces // 500)                      # degenerate faces: a repeated vertex, and three copies of one vertex
    faces[:nd, 1] = faces[:nd, 0]
    faces[nd:2 * nd, 1] = faces[nd:2 * nd, 0]
    faces[nd:2 * nd, 2] = faces[nd:2 * nd, 0]
    perm = r.permutation(n_faces)
    faces = faces[perm]
    # segments: contiguous runs of vertex indices, ids with gaps
    n_seg = max(8, n // 40)
    cuts = np.sort(r.choice(np.arange(1, n), n_seg - 1, replace=False))
    seg_of_run = np.sort(r.choice(np.arange(4 * n_seg), n_seg, replace=False))
    seg = np.repeat(seg_of_run, np.diff(np.concatenate([[0], cuts, [n]]))).astype(np.int64)
    # raw nyu40 labels per segment (0 unannotated .. 40)
    seg_label = {int(s): int(r.choice([0, 1, 2, 22, 3, 4, 5, 7, 39, 40, 14, 24])) for s in seg_of_run}
    labels = np.array([seg_label[int(s)] for s in seg], np.uint16)
    groups, k = [], 0
    segs = [int(s) for s in r.permutation(seg_of_run)]
    take = iter(segs)
    oid = 0
    for i in range(n_objects + 3):
        if i < 3:
            label = ["wall", "floor", "ceiling"][i]
        else:
            label = NAMES[r.randint(len(NAMES))]
        m = r.randint(1, 4)
        ss = [s for s, _ in zip(take, range(m))]
        if not ss:
            break
        groups.append({"id": len(groups), "objectId": oid, "segments": ss, "label": label})
        oid += 1 + (r.rand() < 0.25)                     # objectId gaps
    objs = [g for g in groups if g["label"] not in ("wall", "floor", "ceiling")]
    # a segment shared by two objects, and an object whose segments all go to later objects
    if len(objs) >= 4:
        objs[2]["segments"] = objs[2]["segments"] + [objs[0]["segments"][0]]
        objs[1]["segments"] = list(objs[1]["segments"])
        objs[3]["segments"] = objs[3]["segments"] + objs[1]["segments"]
    if empty_object and len(objs) >= 3:
        objs[-2]["segments"] = []
    g = {"sceneId": None, "appId": "synthetic", "segGroups": groups}
    ang = r.rand() * 2 * np.pi
    M = np.eye(4)
    M[:2, :2] = [[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]]
    M[:3, 3] = r.randn(3) * 3
    return dict(vertex=v, faces=faces, labels=labels, seg=seg, agg=g if annotated else None, align=M if align else None)


def _ply_bytes(vertex, faces, label=False):
    head = ["ply", "format binary_little_endian 1.0", "comment synthetic", "element vertex %d" % len(vertex),
            "property float x", "property float y", "property float z", "property uchar red", "property uchar green",
            "property uchar blue", "property uchar alpha"]
    if label:
        head.append("property ushort label")
    head += ["element face %d" % len(faces), "property list uchar int vertex_indices", "end_header"]
    f = np.zeros(len(faces), FACE_DTYPE)
    f["count"] = 3
    f["vertex_indices"] = faces
    return ("\n".join(head) + "\n").encode("ascii") + vertex.tobytes() + f.tobytes()


def scan_files(scene, scan):
    """-> {file name: bytes} of one scan"""
    out = {scene + "_vh_clean_2.ply": _ply_bytes(scan["vertex"], scan["faces"])}
    lv = np.zeros(len(scan["vertex"]), LABEL_VERTEX_DTYPE)
    for k in VERTEX_DTYPE.names:
        lv[k] = scan["vertex"][k]
    lv["label"] = scan["labels"]
    out[scene + "_vh_clean_2.labels.ply"] = _ply_bytes(lv, scan["faces"], label=True)
    out[scene + "_vh_clean_2.0.010000.segs.json"] = json.dumps(
        {"params": {"kThresh": "0.0001", "segMinVerts": "20"}, "sceneId": scene + "_vh_clean_2",
         "segIndices": [int(s) for s in scan["seg"]]}).encode()
    if scan["agg"] is not None:
        agg = dict(scan["agg"], sceneId="scannet." + scene, segmentsFile="scannet." + scene + "_vh_clean_2.0.010000.segs.json")
        out[scene + ".aggregation.json"] = json.dumps(agg, indent=1).encode()
    meta = ["colorHeight = 968", "colorWidth = 1296"]
    if scan["align"] is not None:
        meta.append("axisAlignment = " + " ".join(repr(float(x)) for x in scan["align"].reshape(-1)) + " ")
    meta += ["numColorFrames = 100", "sceneType = Bedroom"]
    out[scene + ".txt"] = ("\n".join(meta) + "\n").encode()
    return out


def write_files(scan_dir, files):
    os.makedirs(scan_dir, exist_ok=True)
    for name, data in files.items():
        with open(os.path.join(scan_dir, name), "wb") as fh:
            fh.write(data)
    return scan_dir


def write_scan(root, scene, scan):
    """writes root/<scene>/ and returns its path"""
    return write_files(os.path.join(root, scene), scan_files(scene, scan))
