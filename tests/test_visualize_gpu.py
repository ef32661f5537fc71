"""The box-wireframe writers on the device (csrc/visualize.hip, d3net_amd.visualize): d3_format_f6 equals Python's "{:f}" on about
2 * 10^5 doubles; write_box_plys, visualize_grounding and visualize_captioning write files byte-equal to the ones the reference's own
functions wrote (tests/golden/visualize_golden.npz); box_wireframes' vertices equal the host restatement (tests/visualize_restate.py,
pinned to the golden on the CPU) with ==; a device-resident batch with a zero-extent and a NaN box raises, naming the first, and
leaves no file.
Tolerances: none but one.  Text is compared as bytes, vertices with ==: the geometry is IEEE subtraction, a float32 square, a
correctly rounded double square root, one multiplication, one division and one addition per coordinate, the same operations in
the same order on both sides, and the ring's 20 values come from the host.  The vertices against the numbers PARSED from the
golden text: 5e-7, half a unit of the sixth printed decimal, compared in exact rational arithmetic (a tie sits on the bound)."""
import os
import sys
import types
from fractions import Fraction

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import visualize_restate as VR  # noqa: E402
from test_visualize import _cfg  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return VR.load_golden()


@pytest.fixture(scope="module")
def cases():
    return VR.box_cases()


def _tree(root):
    out = {}
    for dp, _, fs in os.walk(root):
        for f in fs:
            p = os.path.join(dp, f)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


def _golden_tree(golden, prefix):
    return {k[len(prefix):]: v for k, v in golden.items() if k.startswith(prefix)}


def f6_values():
    rng = np.random.default_rng(7)
    ties = np.arange(1, 1024, 2) / 128.0                                       # the true six-decimal ties: odd k / 128
    return np.concatenate([rng.uniform(-1e5, 1e5, 100000), 10.0 ** rng.uniform(-20, 0, 50000) * rng.choice([-1.0, 1.0], 50000),
                           (np.arange(50000) + 0.5) / 1e6, ties, -ties,
                           [0.0, -0.0, 5e-324, -5e-324, 0.9999995, 99999.9999995, -99999.9999995, np.nan, np.inf, -np.inf, 1.0 / 128, 3.0 / 128]])


def test_format_f6_equals_python(dev):
    from d3net_amd import _lib, visualize as V
    v = f6_values()
    assert 2.0e5 <= len(v) <= 2.1e5
    got = V.format_f6(v, device=dev)
    want = ["{:f}".format(x) for x in v.tolist()]
    wrong = [(x, g, w) for x, g, w in zip(v.tolist(), got, want) if g != w]
    assert not wrong, (len(wrong), wrong[:5])
    assert got[-2:] == ["0.007812", "0.023438"] and got[-12:-5] == ["0.000000", "-0.000000", "0.000000", "-0.000000", "1.000000", "99999.999999",
                                                                 "-99999.999999"]
    assert got[-5:-2] == ["nan", "inf", "-inf"]
    # a tensor on the device is formatted where it is; beyond the range is refused, not misprinted
    assert V.format_f6(torch.tensor([1.5, -2.25], dtype=torch.float64, device=dev)) == ["1.500000", "-2.250000"]
    assert V.format_f6(np.array([999999999999999.9, -123456789012345.67]), device=dev) == ["999999999999999.875000", "-123456789012345.671875"]
    with pytest.raises(_lib.D3Error, match="value 1 is finite with a magnitude of 1e15"):
        V.format_f6(np.array([1.0, 1e15, 2.0]), device=dev)


def test_write_box_plys_equals_the_golden_files(dev, golden, cases, tmp_path):
    from d3net_amd import visualize as V
    name, corners, mode = cases[0]
    one = str(tmp_path / "one.ply")
    assert V.write_box_plys(corners[None], [mode], [one], device=dev) == [one]                       # M = 1
    assert open(one, "rb").read() == golden["box/" + name]
    stack = np.stack([c.astype(np.float64) for _, c, _ in cases])
    modes = [m for _, _, m in cases]
    paths = [str(tmp_path / ("all-%s.ply" % n)) for n, _, _ in cases]
    assert V.write_box_plys(stack, modes, paths, device=dev) == paths                                # all together
    for (n, _, _), p in zip(cases, paths):
        assert open(p, "rb").read() == golden["box/" + n], n
    # chunk = 2 over an odd number of boxes: chunk boundaries and a short last chunk; once all cases as float64 (13 boxes, the
    # first one twice), once the float32 cases as float32 (7 boxes)
    for dt in (np.float64, np.float32):
        sel = [i for i, (_, c, _) in enumerate(cases) if dt == np.float64 or c.dtype == np.float32]
        sel = sel + sel[:1]
        assert len(sel) % 2 == 1
        paths = [str(tmp_path / ("c2-%s-%d.ply" % (dt.__name__, j))) for j in range(len(sel))]
        c = np.stack([cases[i][1].astype(dt) for i in sel])
        assert V.write_box_plys(c, [cases[i][2] for i in sel], paths, chunk=2, device=dev) == paths
        for i, p in zip(sel, paths):
            assert open(p, "rb").read() == golden["box/" + cases[i][0]], (dt, cases[i][0])
    # the same boxes resident on the device, modes as a device tensor
    paths = [str(tmp_path / ("dev-%s.ply" % n)) for n, _, _ in cases]
    V.write_box_plys(torch.from_numpy(stack).to(dev), torch.tensor(modes, device=dev), paths, chunk=5)
    for (n, _, _), p in zip(cases, paths):
        assert open(p, "rb").read() == golden["box/" + n], n


def test_box_wireframes_equal_the_restatement(dev, golden, cases):
    from d3net_amd import visualize as V
    stack = np.stack([c.astype(np.float64) for _, c, _ in cases])
    modes = [m for _, _, m in cases]
    verts, faces, colors = V.box_wireframes(stack, modes, device=dev)
    assert verts.shape == (len(cases), 1320, 3) and verts.dtype == torch.float64 and verts.device.type == "cuda"
    assert faces is V.wire_faces() and colors.dtype == np.uint8 and colors.tolist() == [[0, 255, 0] if m == 0 else [0, 0, 255] for m in modes]
    got = verts.cpu().numpy()
    header, face_block = V._file_parts()
    for i, (n, c, m) in enumerate(cases):
        want = VR.box_vertices(c)
        assert np.array_equal(got[i], want), n                                                       # == on every coordinate
        assert not np.signbit(got[i][got[i] == 0]).any(), n                                          # a zero carries no sign, as the reference's
        text = golden["box/" + n][len(header):-len(face_block)].decode().split("\n")[:-1]
        # exactly, in rationals: at 9e4 a double's own spacing (1.5e-11) would blur a tie such as 89999.1328125 -> 89999.132812,
        # which lies at the bound itself
        parsed = [Fraction(t) for line in text for t in line.split()[:3]]
        assert len(parsed) == 3960 and max(abs(Fraction(v) - p) for v, p in zip(got[i].reshape(-1).tolist(), parsed)) <= Fraction(5, 10 ** 7), n
    # a float32 tensor on the device is widened there
    f32 = [i for i, (_, c, _) in enumerate(cases) if c.dtype == np.float32]
    v32, _, _ = V.box_wireframes(torch.from_numpy(np.stack([cases[i][1] for i in f32])).to(dev), [cases[i][2] for i in f32])
    assert torch.equal(v32, verts[f32])


def _evaluator_batches(pred, dev):
    """the case's tree as two tiny batches for GroundingEvaluator: one scene each, one row and one proposal slot per annotation, the
    row's score one-hot on its own slot -> (batches, chunked_data)"""
    batches, chunked = [], []
    for s, (scene, objects) in enumerate(pred.items()):
        rows = [(obj, a, rec) for obj, anns in objects.items() for a, rec in anns.items()]
        n = len(rows)
        chunked.append([{"scene_id": scene, "object_id": obj, "ann_id": a} for obj, a, _ in rows])
        t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
        batches.append({"cluster_ref": t(np.eye(n, dtype=np.float32)), "cluster_labels": t(np.eye(n, dtype=np.float32)),
                        "proposal_batch_mask": t(np.ones((1, n), np.float32)),
                        "proposal_bbox_batched": t(np.stack([r["pred_bbox"] for _, _, r in rows])[None]),
                        "ref_box_corner_label": t(np.stack([r["gt_bbox"] for _, _, r in rows])[None]),
                        "unique_multiple": t(np.zeros((1, n), np.int64)), "object_cat": t(np.zeros((1, n), np.int64)),
                        "id": t(np.array([s], np.int64)), "chunk_ids": t(np.arange(n, dtype=np.int64)[None])})
    return batches, chunked


def test_grounding_tree_equals_the_golden(dev, golden, tmp_path):
    from d3net_amd import grounding_eval as ge, visualize as V
    want = _golden_tree(golden, "ground/")
    pred = VR.grounding_tree_case()
    V.visualize_grounding(pred, str(tmp_path / "dict"), device=dev)
    assert _tree(str(tmp_path / "dict")) == want
    ev = ge.GroundingEvaluator(use_lang_classifier=False, keep_predictions=True, device=dev)
    batches, chunked = _evaluator_batches(pred, dev)
    for b in batches:
        ev.add_batch(b)
    kept = ev.device_predictions(chunked)
    leaf = kept["scene0011_00"]["3"]["1"]
    assert sorted(leaf) == ["gt_bbox", "pred_bbox"] and leaf["pred_bbox"].is_cuda and leaf["pred_bbox"].shape == (8, 3)
    torch.cuda.synchronize()
    written = V.visualize_grounding(kept, str(tmp_path / "ev"))
    assert _tree(str(tmp_path / "ev")) == want and len(written) == 7
    own = V.visualize_grounding(kept, str(tmp_path / "own"), per_annotation_boxes=True)
    got = _tree(str(tmp_path / "own"))
    assert len(own) == 7 and got == VR.grounding_tree_files(pred, per_annotation_boxes=True) and got != want


def test_captioning_tree_equals_the_golden(dev, golden, tmp_path):
    from d3net_amd import visualize as V
    want = _golden_tree(golden, "cap/")
    for form, cand in zip(("lists", "dicts"), VR.captioning_tree_case()):
        V.visualize_captioning(cand, str(tmp_path / form), device=dev)
        assert _tree(str(tmp_path / form)) == want, form


def test_degenerate_boxes_on_the_device(dev, golden, cases, tmp_path):
    from d3net_amd import _lib, visualize as V
    good = [cases[0], cases[3], cases[5]]
    c = np.stack([good[0][1].astype(np.float64), good[1][1].astype(np.float64), good[1][1].astype(np.float64), good[2][1].astype(np.float64),
                  good[2][1].astype(np.float64)])
    c[1, :, 2] = c[1, 0, 2]                                                                          # box 1: zero extent along z
    c[3, 4, 0] = np.nan                                                                              # box 3: a NaN corner
    modes = [good[0][2], 1, good[1][2], 0, good[2][2]]
    on_dev = torch.from_numpy(c).to(dev)
    for chunk in (4096, 1):                             # chunk = 1: box 0's file is written before box 1 is met, and is taken back
        out = tmp_path / ("raise%d" % chunk)
        out.mkdir()
        with pytest.raises(_lib.D3Error, match="box 1 is the first outside the limits .*extent of zero"):
            V.write_box_plys(on_dev, modes, [str(out / ("%d.ply" % i)) for i in range(5)], chunk=chunk)
        assert os.listdir(out) == []
    with pytest.raises(_lib.D3Error, match="box 1 is the first"):
        V.box_wireframes(on_dev, modes)
    out = tmp_path / "skip"
    out.mkdir()
    paths = [str(out / ("%d.ply" % i)) for i in range(5)]
    assert V.write_box_plys(on_dev, modes, paths, on_degenerate="skip", chunk=2) == [paths[0], paths[2], paths[4]]
    assert sorted(os.listdir(out)) == ["0.ply", "2.ply", "4.ply"]
    for i, (n, _, _) in zip((0, 2, 4), good):
        assert open(paths[i], "rb").read() == golden["box/" + n], n
    # the same batch from the host is refused before any launch; skipped, it writes the same three files
    with pytest.raises(ValueError, match="box 1 has an extent of zero"):
        V.write_box_plys(c, modes, paths, device=dev)
    hout = tmp_path / "hskip"
    hout.mkdir()
    hpaths = [str(hout / ("%d.ply" % i)) for i in range(5)]
    assert V.write_box_plys(c, modes, hpaths, on_degenerate="skip", device=dev) == [hpaths[0], hpaths[2], hpaths[4]]
    assert all(open(hpaths[i], "rb").read() == open(paths[i], "rb").read() for i in (0, 2, 4))


def test_pipeline_visualize_grounding_writes_the_evaluators_boxes(dev, tmp_path):
    """PipelineNet.visualize_grounding: the files are the restatement's of the boxes that an evaluation with keep_predictions keeps
    (an untrained listener may pick an empty slot, whose box has no extent: those are dropped)"""
    from d3net_amd import synthetic as S, grounding_eval as ge, visualize as V
    from d3net_amd.pipeline import PipelineNet
    vocab = 200
    ds = {"train": types.SimpleNamespace(vocabulary=S.make_vocabulary(vocab), glove=np.random.default_rng(0).standard_normal((vocab, 300)).astype(np.float32))}
    torch.manual_seed(2)
    net = PipelineNet(_cfg(no_captioning=True, no_grounding=False), ds).to(dev).train()
    net.detector.teacher = True
    batch = S.add_language(S.make_batch([S.small_scene(dims=(40, 32, 20), n_boxes=3, seed=3)], dev), dev, chunk=4, vocab=vocab)
    batch["unique_multiple"] = torch.zeros_like(batch["object_cat"])
    ids, chunks = batch["id"].cpu().tolist(), batch["chunk_ids"].cpu().tolist()
    net.dataset_chunk_data = [[{"scene_id": "scene%04d_00" % i, "object_id": str(c // 2), "ann_id": str(c)} for c in range(max(chunks[0]) + 1)]
                              for i in range(max(ids) + 1)]
    root = str(tmp_path / "vis")
    with pytest.raises(ValueError, match="keep_predictions=True"):
        net.visualize_grounding([batch], root, evaluator=ge.GroundingEvaluator(device=dev))
    assert not os.path.exists(root)
    ev = ge.GroundingEvaluator(use_lang_classifier=True, keep_predictions=True, device=dev)
    result, written = net.visualize_grounding([batch], root, evaluator=ev, seeds=[5], on_degenerate="skip")
    pred = ev.predictions(net.dataset_chunk_data)                              # the boxes that evaluation kept, read back
    assert net.training and result["stats"]["overall"]["overall"] == 4 and len(written) >= 1
    want = VR.grounding_tree_files(pred)
    got = _tree(root)
    assert len(got) == len(written) and set(got) <= set(want) and all(got[k] == want[k] for k in got)
    # a file is missing only where its box is outside the limits
    boxes = {}
    for s, objs in pred.items():
        for o, anns in objs.items():
            first = anns[list(anns)[0]]
            boxes[os.path.join(s, "gt-%s.ply" % o)] = first["gt_bbox"]
            for a in anns:
                boxes[os.path.join(s, "pred-%s-%s.ply" % (o, a))] = first["pred_bbox"]
    assert sorted(boxes) == sorted(want)
    assert all((V.host_box_status(b[None])[0] == 0) == (k in got) for k, b in boxes.items())
