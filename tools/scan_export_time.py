#!/usr/bin/env python3
"""Per-scan cost of d3net_amd.scan_export on synthetic ScanNet-size scans (tests/scan_synth.py: 50 k - 300 k vertices, twice as
many faces, 60 objects), written to a temporary directory first.  Reports, per scan size:
  * host_ms: read_scan (PLY / JSON / meta parsing and the object tables) on one thread;
  * device_ms: export_parsed, HIP events on the current stream (uploads, both kernel stages, the validation read);
  * numpy_ms: a numpy path that follows the reference's algorithm (prepare_scannet.py export + process_one_scan: the per-vertex
    tuple loop, np.cross / fancy-index normals, the seg -> vertex dict, per-object loops) on the same parsed arrays;
and the end-to-end throughput of export_split (16 reader threads, .pth and instance-GT writes included).
Run under `timeout`; prints one JSON line."""
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from d3net_amd import scan_export as SX  # noqa: E402
import scan_synth as SS  # noqa: E402


def numpy_reference_path(p):
    """the reference's algorithm on a ParsedScan (its data structures and loops, restated in numpy)"""
    v = p.vertex
    mesh = np.zeros((len(v), 9), np.float32)
    for j, k in enumerate(("x", "y", "z", "red", "green", "blue")):
        mesh[:, j] = v[k]
    xyz = np.array([[x, y, z] for x, y, z, _, _, _, _ in v])
    face = np.array([f for f in p.face["vertex_indices"]])
    normals = np.zeros(xyz.shape, xyz.dtype)
    n = np.cross(xyz[face][:, 1] - xyz[face][:, 0], xyz[face][:, 2] - xyz[face][:, 0])
    ln = np.sqrt(n[:, 0] ** 2 + n[:, 1] ** 2 + n[:, 2] ** 2)
    n /= (ln + 1e-8)[:, None]
    for c in range(3):
        normals[face[:, c]] += n
    ln = np.sqrt(normals[:, 0] ** 2 + normals[:, 1] ** 2 + normals[:, 2] ** 2)
    normals /= (ln + 1e-8)[:, None]
    mesh[:, 6:] = normals
    aligned = mesh.copy()
    if p.align is not None:
        aligned[:, :3] = np.dot(np.concatenate([mesh[:, :3], np.ones((len(v), 1))], 1), p.align.T)[:, :3]
    seg2verts = {}
    for vert, s in enumerate(p.segments.tolist()):
        seg2verts.setdefault(s, []).append(vert)
    obj_id, _, pair_seg, pair_obj = p.tables
    ids = np.ones(len(v)) * -1
    labels = {}
    for k, o in enumerate(obj_id.tolist()):
        verts = None
        for s in pair_seg[pair_obj == k].tolist():
            verts = seg2verts[s]
            ids[verts] = o
        labels[o] = p.labels[verts][0] if verts is not None else 0
    out = []
    for m in (mesh, aligned):
        b = np.zeros((max(labels) + 1, 8))
        for o, lab in labels.items():
            pc = m[ids == o, 0:3]
            if len(pc) == 0:
                continue
            mn, mx = pc.min(0), pc.max(0)
            b[o] = np.concatenate([(mn + mx) / 2, mx - mn, [lab, o]])
        out.append(b)
    keep = ~np.isin(out[0][:, -2], [1, 2, 22])
    return mesh, aligned, ids, out[0][keep], out[1][keep]


def _ms(f, reps):
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ts))


def main(sizes=(50_000, 150_000, 300_000), reps=5, split_scans=8):
    dev = torch.device("cuda", 0)
    res = {"sizes": []}
    with tempfile.TemporaryDirectory() as tmp:
        for i, n in enumerate(sizes):
            scene = "scene%04d_00" % i
            d = SS.write_scan(tmp, scene, SS.make_scan(100 + i, n=n, n_faces=2 * n, n_objects=60))
            p = SX.read_scan(d)
            SX.export_parsed(p, dev)                     # warm-up
            torch.cuda.synchronize()
            host = _ms(lambda: SX.read_scan(d), reps)
            dt = []
            for _ in range(reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t = time.perf_counter()
                a.record()
                SX.export_parsed(p, dev)
                b.record()
                torch.cuda.synchronize()
                dt.append((a.elapsed_time(b), (time.perf_counter() - t) * 1e3))
            npy = _ms(lambda: numpy_reference_path(p), 2)
            row = {"vertices": n, "faces": 2 * n, "host_ms": round(host, 2),
                   "device_ms": round(float(np.median([x[0] for x in dt])), 3),
                   "device_wall_ms": round(float(np.median([x[1] for x in dt])), 3), "numpy_ms": round(npy, 1)}
            res["sizes"].append(row)
            print(json.dumps(row), flush=True)
        # end to end: export_split over split_scans scans of 150 k vertices
        names = []
        for j in range(split_scans):
            scene = "scene%04d_01" % j
            SS.write_scan(os.path.join(tmp, "split_in"), scene, SS.make_scan(200 + j, n=150_000, n_faces=300_000, n_objects=60))
            names.append(scene)
        t = time.perf_counter()
        SX.export_split(os.path.join(tmp, "split_in"), names, os.path.join(tmp, "out"), "train", threads=16, device=dev,
                        gt_root=os.path.join(tmp, "gt"))
        el = time.perf_counter() - t
        res["split"] = {"scans": split_scans, "vertices": 150_000, "s": round(el, 3), "scans_per_s": round(split_scans / el, 2)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
