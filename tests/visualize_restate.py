"""Plain numpy / Python restatement of the box-wireframe PLY files (csrc/visualize.hip, d3net_amd/visualize.py) and the cases of
tests/golden/visualize_golden.npz.  A test helper that shares no code with d3net_amd.visualize: tests/test_visualize.py pins it, with
`==` on bytes, against the files the reference's own write_bbox / write_ply / visualize wrote (tests/golden/gen_visualize_golden.py);
the GPU tests compare the kernels with it and with the golden.

The geometry is vectorised numpy, the text is Python's own "{:f}" -- neither is what the device does (a closed form per vertex,
integer arithmetic per digit)."""
import functools
import math
import os

import numpy as np

STACKS, SLICES, RADIUS = 10, 10, 0.03
EDGE_VERTS = (STACKS + 1) * SLICES
EDGES = ((0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7))
COLORS = {0: (0, 255, 0), 1: (0, 0, 255)}
# where the local (ring x, ring y, height) lands for an edge along axis a with sign s: rows of the signed permutation
_PERM = {(0, 1): ((2, 1), (1, 1), (0, -1)), (0, -1): ((2, -1), (1, 1), (0, 1)), (1, 1): ((0, 1), (2, 1), (1, -1)),
         (1, -1): ((0, 1), (2, -1), (1, 1)), (2, 1): ((0, 1), (1, 1), (2, 1))}


def ring():
    """the 20 doubles of the cylinder's cross-section, from the host's libm"""
    theta = [i2 * 2.0 * math.pi / SLICES for i2 in range(SLICES)]
    return np.array([RADIUS * math.cos(t) for t in theta] + [RADIUS * math.sin(t) for t in theta], np.float64)


def box_vertices(corners):
    """(8, 3) corners of any float dtype -> (1320, 3) float64, the reference's order"""
    c = np.asarray(corners)
    lo, hi = c.min(axis=0), c.max(axis=0)
    pick = lambda ix, iy, iz: np.array([(hi if ix else lo)[0], (hi if iy else lo)[1], (hi if iz else lo)[2]])
    corner = [pick(0, 0, 0), pick(1, 0, 0), pick(1, 1, 0), pick(0, 1, 0), pick(0, 0, 1), pick(1, 0, 1), pick(1, 1, 1), pick(0, 1, 1)]
    r = ring()
    i = np.repeat(np.arange(STACKS + 1), SLICES).astype(np.float64)
    i2 = np.tile(np.arange(SLICES), STACKS + 1)
    out = []
    for a, b in EDGES:
        p0, p1 = corner[a], corner[b]
        d = (p1 - p0).astype(np.float32)
        h = math.sqrt(np.float32(np.float32(d[0] * d[0]) + np.float32(d[1] * d[1])) + np.float32(d[2] * d[2]))
        axis = int(np.argmax(np.abs(d)))
        local = np.stack([r[i2], r[SLICES + i2], h * i / STACKS], 1)
        rows = _PERM[(axis, 1 if d[axis] > 0 else -1)]
        moved = np.stack([local[:, src] * sign for src, sign in rows], 1)
        out.append(((0.0 + p0.astype(np.float64))[None] + moved) + 0.0)
    return np.concatenate(out)


@functools.lru_cache(maxsize=None)
def faces():
    """(2400, 3) int64: the two triangles per stack and slice, with the edge's vertex offset"""
    out = []
    for k in range(len(EDGES)):
        for i in range(STACKS):
            for i2 in range(SLICES):
                n = (i2 + 1) % SLICES
                out.append(((i + 1) * SLICES + i2, i * SLICES + i2, i * SLICES + n))
                out.append(((i + 1) * SLICES + i2, i * SLICES + n, (i + 1) * SLICES + n))
        out[-2 * STACKS * SLICES:] = [tuple(v + k * EDGE_VERTS for v in f) for f in out[-2 * STACKS * SLICES:]]
    f = np.array(out, np.int64)
    f.setflags(write=False)
    return f


def header(nv, nf):
    return ("ply \nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\nproperty uchar red\n"
            "property uchar green\nproperty uchar blue\nelement face %d\nproperty list uchar uint vertex_indices\nend_header\n" % (nv, nf)).encode()


def vertex_text(corners, mode):
    tail = " %d %d %d\n" % COLORS[mode]
    return "".join("{:f} {:f} {:f}".format(*v) + tail for v in box_vertices(corners).tolist()).encode()


@functools.lru_cache(maxsize=None)
def face_text():
    return "".join("3 %d %d %d\n" % tuple(f) for f in faces().tolist()).encode()


def box_ply(corners, mode):
    f = faces()
    return header(len(EDGES) * EDGE_VERTS, len(f)) + vertex_text(corners, mode) + face_text()


# ------------------------------------------------------------------------------------------------------------------ cases
_SGN = np.array([[-1, -1, -1], [1, -1, -1], [1, 1, -1], [-1, 1, -1], [-1, -1, 1], [1, -1, 1], [1, 1, 1], [-1, 1, 1]], np.float64)


def _box(lo, hi, dtype):
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    return np.where(_SGN > 0, hi[None], lo[None]).astype(dtype)


def box_cases(seed=97):
    """-> [(name, (8, 3) corners, mode)]: float32 and float64, both modes, shuffled vertex order, negative coordinates, a min corner
    exactly at the origin (prints -0.000000), coordinates near +-9e4 with extents of 1e-3 (float64) or one float32 step (float32),
    extents that differ by 10^3 between the axes"""
    rng = np.random.default_rng(seed)
    cases = []
    for name, dt, mode in (("rand64_gt", np.float64, 0), ("rand64_pred", np.float64, 1), ("rand32_gt", np.float32, 0),
                           ("rand32_pred", np.float32, 1)):
        lo = rng.uniform(-4, 4, 3)
        cases.append((name, _box(lo, lo + rng.uniform(0.1, 3, 3), dt), mode))
    lo = rng.uniform(-4, 4, 3)
    shuffled = _box(lo, lo + rng.uniform(0.1, 3, 3), np.float32)[rng.permutation(8)]
    cases.append(("shuffled32", shuffled, 1))
    lo = rng.uniform(-900, -100, 3)
    cases.append(("negative64", _box(lo, lo + rng.uniform(1, 50, 3), np.float64)[rng.permutation(8)], 0))
    cases.append(("origin64", _box([0, 0, 0], rng.uniform(0.5, 2, 3), np.float64), 1))
    cases.append(("origin32", _box([0, 0, 0], rng.uniform(0.5, 2, 3), np.float32), 0))
    lo = np.array([9e4 + rng.uniform(0, 1), -9e4 + rng.uniform(0, 1), 89999.123456])
    cases.append(("far64", _box(lo, lo + 1e-3 * rng.uniform(0.9, 1.1, 3), np.float64), 1))
    lo32 = np.array([9e4 + 0.5, -9e4 - 0.25, 89999.125], np.float32)
    cases.append(("far32", _box(lo32, np.nextafter(lo32, np.float32(np.inf)), np.float32), 0))
    lo = rng.uniform(-2, 2, 3)
    cases.append(("aspect64", _box(lo, lo + np.array([0.0123, 12.3, 1.23]), np.float64), 0))
    cases.append(("aspect32", _box(lo, lo + np.array([45.6, 0.0456, 4.56]), np.float32), 1))
    return cases


def grounding_tree_case(seed=98):
    """-> predictions {scene: {object: {ann: {"pred_bbox", "gt_bbox", "iou"}}}} with float32 (8, 3) boxes, as
    GroundingEvaluator.predictions returns them.  Object "3" of the first scene has two annotations whose predicted boxes differ."""
    rng = np.random.default_rng(seed)

    def box():
        lo = rng.uniform(-3, 3, 3)
        return _box(lo, lo + rng.uniform(0.2, 2, 3), np.float32)

    def ann(gt):
        return {"pred_bbox": box(), "gt_bbox": gt, "iou": np.float32(rng.uniform())}

    gt3, gt7, gt0 = box(), box(), box()
    return {"scene0011_00": {"3": {"0": ann(gt3), "1": ann(gt3)}, "7": {"2": ann(gt7)}}, "scene0025_01": {"0": {"1": ann(gt0)}}}


def grounding_tree_files(predictions, per_annotation_boxes=False):
    """{relative path: bytes} of visualize_grounding: the reference writes the FIRST annotation's predicted box under every name"""
    out = {}
    for scene, objects in predictions.items():
        for obj, anns in objects.items():
            ids = list(anns.keys())
            out[os.path.join(scene, "gt-{}.ply".format(obj))] = box_ply(anns[ids[0]]["gt_bbox"], 0)
            for a in ids:
                out[os.path.join(scene, "pred-{}-{}.ply".format(obj, a))] = box_ply(anns[a if per_annotation_boxes else ids[0]]["pred_bbox"], 1)
    return out


def captioning_tree_case(seed=99):
    """-> (list form, dict form) of the candidates: "scene|object" -> [caption, iou, box, gt_box] with nested lists, as the
    reference's extra_caption.json holds them, and -> {"caption", "iou", "box", "gt_box"} as assign_dense_caption returns them"""
    rng = np.random.default_rng(seed)
    lists, dicts = {}, {}
    for key in ("scene0011_00|5", "scene0011_00|12", "scene0025_01|0"):
        lo = rng.uniform(-3, 3, 3)
        pred = _box(lo, lo + rng.uniform(0.2, 2, 3), np.float32)[rng.permutation(8)].tolist()
        gt = _box(lo + 0.1, lo + rng.uniform(0.3, 2, 3), np.float32).tolist()
        iou = float(rng.uniform())
        lists[key] = ["sos a chair eos", iou, pred, gt]
        dicts[key] = {"caption": "sos a chair eos", "iou": iou, "box": pred, "gt_box": gt}
    return lists, dicts


def captioning_tree_files(candidates):
    out = {}
    for key, value in candidates.items():
        scene, obj = key.split("|")[:2]
        pred, gt = (value["box"], value["gt_box"]) if isinstance(value, dict) else (value[2], value[3])
        out[os.path.join(scene, "pred-{}.ply".format(obj))] = box_ply(np.array(pred), 1)
        out[os.path.join(scene, "gt-{}.ply".format(obj))] = box_ply(np.array(gt), 0)
    return out


def load_golden():
    """tests/golden/visualize_golden.npz -> {"box/<case>" | "ground/<path>" | "cap/<path>": bytes}"""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "visualize_golden.npz"))
    return {str(n): z["file%03d" % i].tobytes() for i, n in enumerate(z["names"].tolist())}
