"""numpy restatement of csrc/scan_export.hip in the device's operation order (float32 face / vertex normals, fp64 alignment in
the order ((x m0 + y m1) + z m2) + m3, last-face-per-corner accumulation, instance ids, labels, boxes, instance GT codes).
It follows the semantics of the reference's prepare_scannet.py / prepare_scannet_inst_gt.py, written afresh."""
import numpy as np

NYU40_IDS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39)
REMAP = np.full(150, -1.0)
REMAP[list(NYU40_IDS)] = np.arange(20)
EPS = np.float32(1e-8)


def _normalize(x, y, z):
    ln = np.sqrt((x * x + y * y) + z * z)
    d = ln + EPS
    return x / d, y / d, z / d


def face_normals(xyz, faces):
    p0, p1, p2 = xyz[faces[:, 0]], xyz[faces[:, 1]], xyz[faces[:, 2]]
    a, b = p1 - p0, p2 - p0
    n0 = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]
    n1 = a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]
    n2 = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
    return np.stack(_normalize(n0, n1, n2), 1).astype(np.float32)


def vertex_normals(xyz, faces):
    n, F = len(xyz), len(faces)
    fn = face_normals(xyz, faces) if F else np.zeros((0, 3), np.float32)
    acc = np.zeros((n, 3), np.float32)
    for c in range(3):
        last = np.full(n, -1, np.int64)
        if F:
            np.maximum.at(last, faces[:, c], np.arange(F))
        m = last >= 0
        acc[m] = acc[m] + fn[last[m]]
    return np.stack(_normalize(acc[:, 0], acc[:, 1], acc[:, 2]), 1).astype(np.float32)


def align_xyz(xyz, M):
    x, y, z = (xyz[:, j].astype(np.float64) for j in range(3))
    return np.stack([(((x * M[r, 0] + y * M[r, 1]) + z * M[r, 2]) + M[r, 3]) for r in range(3)], 1).astype(np.float32)


def mesh_arrays(vertex, faces, M):
    """-> (mesh, aligned_mesh) (N, 9) float32"""
    xyz = np.stack([vertex["x"], vertex["y"], vertex["z"]], 1).astype(np.float32)
    mesh = np.zeros((len(vertex), 9), np.float32)
    mesh[:, :3] = xyz
    mesh[:, 3], mesh[:, 4], mesh[:, 5] = vertex["red"], vertex["green"], vertex["blue"]
    mesh[:, 6:] = vertex_normals(xyz, np.asarray(faces, np.int64).reshape(-1, 3))
    aligned = mesh.copy()
    if M is not None:
        aligned[:, :3] = align_xyz(xyz, np.asarray(M, np.float64))
    return mesh, aligned


def objects(groups, scan_name):
    """[(objectId, segments)] in the reference's dict order, segment lists as the reference's aliasing leaves them"""
    d, first_of_label = {}, {}
    for g in groups:
        if g["label"] in ("wall", "floor", "ceiling"):
            continue
        segs = list(g["segments"])
        d[g["objectId"]] = segs
        if g["label"] in first_of_label:             # the first object of a label also lists the later ones' segments
            first_of_label[g["label"]].extend(segs)
        else:
            first_of_label[g["label"]] = segs
    if scan_name == "scene0217_00":
        keep = sorted(d)[:len(d) // 2]
        d = {o: d[o] for o in keep}
    return list(d.items())


def boxes(xyz, owner, obj_ids, labels):
    R = max(obj_ids) + 1
    out = np.zeros((R, 8))
    for k, o in enumerate(obj_ids):
        m = owner == k
        if not m.any():
            continue
        mn, mx = xyz[m].min(0), xyz[m].max(0)
        out[o, :3] = (mn + mx) / np.float32(2)
        out[o, 3:6] = mx - mn
        out[o, 6], out[o, 7] = labels[k], o
    return out


def export(vertex, faces, M, raw=None, seg=None, groups=None, scan_name=""):
    """-> the process_one_scan dict plus "inst_gt" (int32); groups None: the test-split placeholder"""
    mesh, aligned = mesh_arrays(vertex, faces, M)
    n = len(vertex)
    if groups is None:
        return dict(mesh=mesh, aligned_mesh=aligned, sem_labels=np.full(n, -1.0), instance_ids=np.full(n, -1, np.int64),
                    instance_bboxes=np.zeros((1, 8)), aligned_instance_bboxes=np.zeros((1, 8)), inst_gt=np.zeros(n, np.int32))
    raw = np.asarray(raw).astype(np.int64)
    seg = np.asarray(seg).astype(np.int64)
    useg, first = np.unique(seg, return_index=True)
    seg_first = dict(zip(useg.tolist(), first.tolist()))
    objs = objects(groups, scan_name)
    seg_owner = {}
    obj_ids, labels, last = [], [], None
    for k, (o, segs) in enumerate(objs):
        for s in segs:
            if s not in seg_first:
                raise ValueError("segment %d has no vertex" % s)
            seg_owner[s] = k
        if segs:
            last = segs[-1]
        obj_ids.append(o)
        labels.append(int(raw[seg_first[last]]))
    owner = np.array([seg_owner.get(s, -1) for s in seg.tolist()], np.int64)
    oid = np.asarray(obj_ids, np.int64)
    ids = np.where(owner >= 0, oid[np.maximum(owner, 0)], -1).astype(np.float64)
    sem = REMAP[raw]
    b = boxes(mesh[:, :3], owner, obj_ids, labels)
    ab = boxes(aligned[:, :3], owner, obj_ids, labels)
    if b.shape[0] > 1:
        keep = ~np.isin(b[:, 6], [1, 2, 22])
        b, ab = b[keep], ab[keep]
    gt = inst_gt(sem, ids)
    return dict(mesh=mesh, aligned_mesh=aligned, sem_labels=sem, instance_ids=ids, instance_bboxes=b, aligned_instance_bboxes=ab,
                inst_gt=gt)


def inst_gt(sem, ids):
    gt = (sem.astype(np.int32) + 1) * 1000
    for i in np.unique(ids):
        if i < 0:
            continue
        m = np.nonzero(ids == i)[0]
        s = int(sem[m[0]])
        gt[m] = (0 if s == -1 else NYU40_IDS[s]) * 1000 + int(i) + 1
    return gt.astype(np.int32)


def export_files(files, scene, scan_name=None):
    """restatement from the raw file bytes of scan_synth.scan_files (parsed here with plain numpy)"""
    import json
    from scan_synth import FACE_DTYPE, LABEL_VERTEX_DTYPE, VERTEX_DTYPE

    def ply(data, vdt):
        body = data[data.index(b"end_header\n") + len(b"end_header\n"):]
        head = data[:data.index(b"end_header")].decode().split("\n")
        nv = int([l for l in head if l.startswith("element vertex")][0].split()[2])
        nf = int([l for l in head if l.startswith("element face")][0].split()[2])
        v = np.frombuffer(body, vdt, nv)
        f = np.frombuffer(body, FACE_DTYPE, nf, offset=nv * vdt.itemsize)
        return v, f["vertex_indices"].astype(np.int64)

    v, f = ply(files[scene + "_vh_clean_2.ply"], VERTEX_DTYPE)
    M = None
    for line in files[scene + ".txt"].decode().splitlines():
        if line.startswith("axisAlignment"):
            M = np.array([float(x) for x in line.split("=")[1].split()]).reshape(4, 4)
    agg = files.get(scene + ".aggregation.json")
    if agg is None:
        return export(v, f, M)
    lv, _ = ply(files[scene + "_vh_clean_2.labels.ply"], LABEL_VERTEX_DTYPE)
    seg = json.loads(files[scene + "_vh_clean_2.0.010000.segs.json"])["segIndices"]
    return export(v, f, M, lv["label"], seg, json.loads(agg)["segGroups"], scan_name or scene)
