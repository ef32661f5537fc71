"""The box-wireframe writers' specification, pinned on the CPU: the numpy / Python restatement (tests/visualize_restate.py) reproduces,
byte for byte, every file that the reference's own write_bbox / write_ply / visualize wrote (tests/golden/visualize_golden.npz, made
by gen_visualize_golden.py); the library's constant header and face block are the golden's; the path layout and the reference's
`ann_ids[0]` rule; host inputs outside the limits are refused before the library is touched; write_aligned_mesh; the mode refusal of
PipelineNet.visualize_grounding.  Every comparison is exact."""
import os
import types

import numpy as np
import pytest

import scan_synth
import visualize_restate as VR


@pytest.fixture(scope="module")
def golden():
    return VR.load_golden()


def test_restatement_reproduces_every_golden_file(golden):
    seen = set()
    for name, corners, mode in VR.box_cases():
        assert VR.box_ply(corners, mode) == golden["box/" + name], name
        seen.add("box/" + name)
    for rel, data in VR.grounding_tree_files(VR.grounding_tree_case()).items():
        assert data == golden["ground/" + rel], rel
        seen.add("ground/" + rel)
    lists, dicts = VR.captioning_tree_case()
    for cand in (lists, dicts):
        for rel, data in VR.captioning_tree_files(cand).items():
            assert data == golden["cap/" + rel], rel
            seen.add("cap/" + rel)
    assert seen == set(golden) and len(seen) == 25
    # what the cases are there for
    assert b"\n-0.000000 " in golden["box/origin64"] or b" -0.000000 " in golden["box/origin64"]
    assert b"nan" not in b"".join(golden.values())
    assert b" 0 255 0\n" in golden["box/rand64_gt"] and b" 0 0 255\n" in golden["box/rand64_pred"]


def test_the_first_annotation_rule_shows_in_the_golden(golden):
    """the reference writes ann_ids[0]'s predicted box under every annotation's name: pred-3-1.ply IS pred-3-0.ply, although the
    case's two predicted boxes differ"""
    case = VR.grounding_tree_case()["scene0011_00"]["3"]
    assert not np.array_equal(case["0"]["pred_bbox"], case["1"]["pred_bbox"])
    assert golden["ground/scene0011_00/pred-3-1.ply"] == golden["ground/scene0011_00/pred-3-0.ply"]
    own = VR.grounding_tree_files(VR.grounding_tree_case(), per_annotation_boxes=True)
    assert own["scene0011_00/pred-3-1.ply"] != golden["ground/scene0011_00/pred-3-1.ply"]
    assert own["scene0011_00/pred-3-0.ply"] == golden["ground/scene0011_00/pred-3-0.ply"]


def test_header_and_face_block_equal_the_goldens(golden):
    from d3net_amd import visualize as V
    header, face_block = V._file_parts()
    assert header.startswith(b"ply \nformat ascii 1.0\nelement vertex 1320\n") and header.endswith(b"end_header\n")
    assert header == VR.header(1320, 2400) and face_block == VR.face_text()
    f = V.wire_faces()
    assert f.shape == (2400, 3) and f.dtype == np.int32 and not f.flags.writeable and np.array_equal(f, VR.faces())
    assert f.min() == 0 and f.max() == 1319
    for name, data in golden.items():
        assert data.startswith(header) and data.endswith(face_block), name
        assert data[len(header):len(data) - len(face_block)].count(b"\n") == 1320, name
    assert V.VERTS_PER_BOX == 1320 and V.FACES_PER_BOX == 2400
    assert np.array_equal(np.frombuffer(V._ring(), np.float64), VR.ring())


def _captured(monkeypatch):
    from d3net_amd import visualize as V
    calls = []

    def fake(corners, modes, paths, **kw):
        calls.append((np.asarray(corners), np.asarray(modes), list(paths)))
        return list(paths)

    monkeypatch.setattr(V, "write_box_plys", fake)
    return V, calls


def test_grounding_paths_and_the_first_annotation_rule(tmp_path, monkeypatch):
    V, calls = _captured(monkeypatch)
    pred = VR.grounding_tree_case()
    root = str(tmp_path / "vis")
    written = V.visualize_grounding(pred, root)
    rel = [os.path.relpath(p, root) for p in written]
    assert rel == list(VR.grounding_tree_files(pred))                    # the reference's order: gt, then the annotations
    assert sorted(os.listdir(root)) == ["scene0011_00", "scene0025_01"]
    corners, modes, _ = calls[0]
    assert corners.shape == (7, 8, 3) and corners.dtype == np.float64 and modes.tolist() == [0, 1, 1, 0, 1, 0, 1]
    a = pred["scene0011_00"]["3"]
    assert np.array_equal(corners[0], a["0"]["gt_bbox"]) and np.array_equal(corners[1], a["0"]["pred_bbox"])
    assert np.array_equal(corners[2], a["0"]["pred_bbox"])               # ann "1" gets ann "0"'s box
    V.visualize_grounding(pred, root, per_annotation_boxes=True)
    assert np.array_equal(calls[1][0][2], a["1"]["pred_bbox"]) and calls[1][2] == calls[0][2]
    assert V.visualize_grounding({}, root) == [] and len(calls) == 2


def test_captioning_paths_from_both_candidate_forms(tmp_path, monkeypatch):
    V, calls = _captured(monkeypatch)
    lists, dicts = VR.captioning_tree_case()
    root = str(tmp_path / "vis")
    for cand in (lists, dicts):
        rel = [os.path.relpath(p, root) for p in V.visualize_captioning(cand, root)]
        assert rel == list(VR.captioning_tree_files(cand))
    assert np.array_equal(calls[0][0], calls[1][0]) and calls[0][1].tolist() == [1, 0] * 3
    assert np.array_equal(calls[0][0][0], np.array(lists["scene0011_00|5"][2])) and np.array_equal(calls[0][0][1], np.array(lists["scene0011_00|5"][3]))
    more = {"scene0011_00|5|chair|3": lists["scene0011_00|5"]}           # further fields are ignored
    assert [os.path.relpath(p, root) for p in V.visualize_captioning(more, root)] == ["scene0011_00/pred-5.ply", "scene0011_00/gt-5.ply"]
    with pytest.raises(ValueError, match="scene\\|object"):
        V.visualize_captioning({"scene0011_00": lists["scene0011_00|5"]}, root)


def test_boxes_outside_the_limits_are_refused_before_the_library_is_touched(tmp_path, monkeypatch):
    from d3net_amd import _lib, visualize as V

    def no_launch():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "lib", no_launch)
    good = np.stack([c.astype(np.float64) for _, c, _ in VR.box_cases()[:3]])
    paths = [str(tmp_path / ("%d.ply" % i)) for i in range(3)]

    def bad(change):
        c = good.copy()
        change(c)
        return c

    def flat(c):
        c[2, :, 1] = c[2, 0, 1]

    def far(c):
        c[1, 3, 0] = 1e5

    def nan(c):
        c[1, 0, 2] = np.nan

    def inf(c):
        c[0, 7, 0] = -np.inf

    for change, box, text in ((flat, 2, "extent of zero"), (far, 1, "not below 1e5"), (nan, 1, "not finite"), (inf, 0, "not finite")):
        for call in (lambda c: V.write_box_plys(c, [0, 1, 0], paths), lambda c: V.box_wireframes(c, [0, 1, 0]),
                     lambda c: V.write_box_plys(c.astype(np.float32), [0, 1, 0], paths)):
            with pytest.raises(ValueError, match="box %d has .*%s" % (box, text)):
                call(bad(change))
    assert V.host_box_status(bad(flat)).tolist() == [0, 0, 2] and V.host_box_status(bad(nan)).tolist() == [0, 1, 0]
    assert V.host_box_status(good).tolist() == [0, 0, 0]
    edge =good.copy(); edge[0, :, 0] = np.where(edge[0, :, 0] == edge[0, :, 0].max(), np.nextafter(1e5, 0), edge[0, :, 0])
    assert V.host_box_status(edge).tolist() == [0, 0, 0]
    for call, text in ((lambda: V.write_box_plys(good, [0, 1, 2], paths), "modes are 0"), (lambda: V.write_box_plys(good, [0, 1], paths), "modes of shape"),
                       (lambda: V.write_box_plys(good, [0, 1, 0], paths[:2]), "2 paths for 3 boxes"),
                       (lambda: V.write_box_plys(good.reshape(3, 24), [0, 1, 0], paths), "corners"),
                       (lambda: V.write_box_plys(good, [0, 1, 0], paths, on_degenerate="ignore"), "on_degenerate"),
                       (lambda: V.write_box_plys(good, [0, 1, 0], paths, device="cpu"), "no CPU fallback")):
        with pytest.raises(ValueError, match=text):
            call()
    # every box dropped: nothing to launch
    assert V.write_box_plys(bad(flat)[2:], [0], paths[:1], on_degenerate="skip") == []
    assert os.listdir(tmp_path) == []


def test_write_aligned_mesh_round_trips_and_matches_align_mesh(tmp_path):
    """mesh.ply read back with scan_export.read_ply (read_mesh_ply wants the scan's 7-property vertices, this file has the
    reference's 6) equals a numpy restatement of align_mesh: float64 dot with the axisAlignment matrix, stored as float32"""
    from d3net_amd import scan_export as SE, visualize as V
    scan = scan_synth.make_scan(5, n=500)
    d = scan_synth.write_scan(str(tmp_path), "scene0707_00", scan)
    out = V.write_aligned_mesh(d, str(tmp_path / "mesh.ply"))
    raw = open(out, "rb").read()
    assert raw.startswith(b"ply\nformat binary_little_endian 1.0\nelement vertex 500\nproperty float x\nproperty float y\nproperty float z\n"
                          b"property uchar red\nproperty uchar green\nproperty uchar blue\nelement face 1000\n"
                          b"property list uchar int vertex_indices\nend_header\n")
    el = SE.read_ply(out)
    v, f = el["vertex"], el["face"]
    assert v.dtype == V.MESH_PLY_VERTEX and f.dtype == SE.FACE_DTYPE and len(raw) == raw.index(b"end_header\n") + 11 + 500 * 15 + 1000 * 13
    src = scan["vertex"]
    pts = np.ones((500, 4))
    pts[:, :3] = np.stack([src["x"], src["y"], src["z"]], 1)
    M = SE.read_axis_alignment(os.path.join(d, "scene0707_00.txt"))
    want = np.dot(pts, M.T)[:, :3].astype(np.float32)
    assert np.array_equal(np.stack([v["x"], v["y"], v["z"]], 1), want)
    for c in ("red", "green", "blue"):
        assert np.array_equal(v[c], src[c])
    assert np.array_equal(f["vertex_indices"], scan["faces"]) and (f["count"] == 3).all()
    # a ScanExport-like object: the aligned mesh comes from it, the faces from the caller
    import torch
    mesh9 = np.concatenate([want, np.stack([src[c] for c in ("red", "green", "blue")], 1).astype(np.float32), np.zeros((500, 3), np.float32)], 1)
    export = types.SimpleNamespace(aligned_mesh=torch.from_numpy(mesh9))
    with pytest.raises(ValueError, match="carries no faces"):
        V.write_aligned_mesh(export, str(tmp_path / "m2.ply"))
    for faces in (scan["faces"], SE.read_scan(d).face, d):
        assert open(V.write_aligned_mesh(export, str(tmp_path / "m2.ply"), faces=faces), "rb").read() == raw
    with pytest.raises(ValueError, match="indices into the 500 vertices"):
        V.write_aligned_mesh(export, str(tmp_path / "m3.ply"), faces=scan["faces"] + 400)


def _cfg(**model):
    from d3net_amd.config import default_conf
    base = {"model": {"blocks": [1, 2, 3], "num_graph_steps": 2, "num_locals": 10, "use_relation": True, "use_orientation": True,
                      "match_type": "Transformer", "use_lang_classifier": True, "use_bidir": False, "num_bbox_class": 18,
                      "loss_type": "cross_entropy"},
            "data": {"num_des_per_scene": 4, "max_spk_len": 30, "max_lis_len": 126, "min_iou_threshold": 0.25, "num_ori_bins": 6},
            "train": {"use_rl": False, "sample_topn": 1}}
    base["model"].update(model)
    return default_conf(overrides=base)


def test_visualize_grounding_refuses_other_modes(tmp_path):
    from d3net_amd import synthetic as S
    from d3net_amd.pipeline import PipelineNet
    V = 50
    ds = {"train": types.SimpleNamespace(vocabulary=S.make_vocabulary(V), glove=np.zeros((V, 300), np.float32))}
    root = str(tmp_path / "vis")
    net0 = PipelineNet(_cfg(no_captioning=True, no_grounding=True), ds)
    with pytest.raises(NotImplementedError, match=r"modes 2 and 3\), this is mode 0"):
        net0.visualize_grounding([], root)
    net1 = PipelineNet(_cfg(no_captioning=False, no_grounding=True), ds)
    with pytest.raises(NotImplementedError, match=r"modes 2 and 3\), this is mode 1"):
        net1.visualize_grounding([], root)
    net2 = PipelineNet(_cfg(no_captioning=True, no_grounding=False), ds).train()
    with pytest.raises(ValueError, match="description store"):              # the right mode, but nothing names the annotations
        net2.visualize_grounding([], root)
    assert net2.training and not os.path.exists(root)                       # refused before any work


def test_binding_table_entries(built_lib):
    import ctypes as C
    from d3net_amd import _lib
    res, args = _lib.SIGNATURES["d3_box_wire_text"]
    assert res is C.c_int and len(args) == 8 and args[2] is C.c_int and args[3] is C.POINTER(C.c_double)
    res, args = _lib.SIGNATURES["d3_box_wire_verts"]
    assert res is C.c_int and len(args) == 6 and args[1] is C.c_int
    res, args = _lib.SIGNATURES["d3_format_f6"]
    assert res is C.c_int and len(args) == 6 and args[1] is C.c_longlong
    v, s, f = C.c_int(0), C.c_int(0), C.c_int(0)                             # a pure host entry point
    assert _lib.lib().d3_box_wire_limits(C.byref(v), C.byref(s), C.byref(f)) == 0
    assert (v.value, s.value, f.value) == (1320, 1320 * 56, 24)
