"""CPU side of d3net_amd.scan_export: the host PLY / meta / aggregation readers, the numpy restatement
(tests/scan_export_restate.py) against the reference's own outputs (tests/golden/scan_export_golden.npz), the test-split
placeholder, the input errors and the keys / dtypes of the saved dict."""
import json
import os

import numpy as np
import pytest

import scan_export_restate as R
import scan_synth as SS
from d3net_amd import scan_export as SX

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scan_export_golden.npz"))
CASES = [str(c) for c in G["cases"]]
KEYS = ("mesh", "aligned_mesh", "sem_labels", "instance_ids", "instance_bboxes", "aligned_instance_bboxes")


def golden_files(case):
    p = case + "/file/"
    return {k[len(p):]: G[k].tobytes() for k in G.files if k.startswith(p)}


def _same_bits(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    assert a.tobytes() == b.tobytes(), (what, int((a != b).sum()))


def ulp_diff(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7fffffff), ia)
    ib = np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return np.abs(ia - ib)


def test_ply_reader_matches_writer():
    scan = SS.make_scan(3, n=700)
    files = SS.scan_files("scene0005_00", scan)
    v, f = SX.read_mesh_ply(files["scene0005_00_vh_clean_2.ply"])
    assert v.dtype == SX.MESH_VERTEX_DTYPE and v.tobytes() == scan["vertex"].tobytes()
    np.testing.assert_array_equal(f["vertex_indices"], scan["faces"])
    assert (f["count"] == 3).all()
    lab = SX.read_label_ply(files["scene0005_00_vh_clean_2.labels.ply"])
    assert lab.dtype == np.uint16
    np.testing.assert_array_equal(lab, scan["labels"])


def test_ply_reader_rejects_other_layouts():
    scan = SS.make_scan(4, n=300)
    good = SS.scan_files("scene0006_00", scan)["scene0006_00_vh_clean_2.ply"]
    with pytest.raises(ValueError):
        SX.read_ply(good.replace(b"binary_little_endian", b"ascii", 1))
    with pytest.raises(ValueError):
        SX.read_ply(good.replace(b"binary_little_endian", b"binary_big_endian", 1))
    with pytest.raises(ValueError):                      # uint indices
        SX.read_ply(good.replace(b"list uchar int", b"list uchar uint", 1))
    with pytest.raises(ValueError):                      # an extra vertex property: not the reference's 7
        SX.read_mesh_ply(good.replace(b"property uchar alpha", b"property uchar alpha\nproperty float quality", 1))
    with pytest.raises(ValueError):                      # a quad
        i = good.index(b"end_header\n") + 11 + len(scan["vertex"]) * 16
        SX.read_ply(good[:i] + b"\x04" + good[i + 1:])
    with pytest.raises(ValueError):
        SX.read_ply(good[:-5])
    with pytest.raises(ValueError):                      # no label property
        SX.read_label_ply(good)


def test_axis_alignment_strip_quirk(tmp_path):
    M = np.arange(16, dtype=np.float64).reshape(4, 4) / 7
    vals = " ".join(repr(float(x)) for x in M.reshape(-1))
    p = tmp_path / "m.txt"
    # str.strip('axisAlignment = ') strips a character set: 'tangent ' goes too, and the last matching line wins
    p.write_text("axisAlignment = 1 0 0 0 0 1 0 0 0 0 1 0 0 0 0 1\ntangent axisAlignment =" + vals + "  \nsceneType = x\n")
    np.testing.assert_array_equal(SX.read_axis_alignment(str(p)), M)
    p.write_text("colorHeight = 968\n")
    assert SX.read_axis_alignment(str(p)) is None
    p.write_text("axisAlignment = 1 2 3\n")
    with pytest.raises(ValueError):
        SX.read_axis_alignment(str(p))


@pytest.mark.parametrize("case", CASES)
def test_restatement_equals_golden(case):
    r = R.export_files(golden_files(case), case)
    for k in KEYS + ("inst_gt",):
        g = G["%s/%s" % (case, k)]
        if k == "aligned_mesh":          # the reference's np.dot order is BLAS's: 1 ulp on aligned xyz, the rest exact
            _same_bits(r[k][:, 3:], g[:, 3:], k)
            d = ulp_diff(r[k][:, :3], g[:, :3])
            assert d.max() <= 1, (case, int(d.max()))
        else:
            _same_bits(r[k], g, "%s/%s" % (case, k))


def _prefilter_objects(case):
    """per object of the golden scan (SX.object_tables order): (objectId, owns a vertex, lists a segment, label of the first
    vertex of its label segment), from the files alone"""
    files = golden_files(case)
    groups = [(int(g["objectId"]), g["label"], list(g["segments"]))
              for g in json.loads(files[case + ".aggregation.json"])["segGroups"]]
    oid, ls, ps, po = SX.object_tables(groups, case)
    seg = np.asarray(json.loads(files[case + "_vh_clean_2.0.010000.segs.json"])["segIndices"])
    raw = SX.read_label_ply(files[case + "_vh_clean_2.labels.ply"])
    owner = {}
    for s_, k in zip(ps.tolist(), po.tolist()):
        owner[s_] = k                                       # the last listing object keeps a segment
    out = []
    for k, o in enumerate(oid.tolist()):
        mine = [s_ for s_, kk in zip(ps.tolist(), po.tolist()) if kk == k]
        owns = any(owner[s_] == k for s_ in mine)
        out.append((o, owns, bool(mine), int(raw[np.nonzero(seg == ls[k])[0][0]])))
    return out


def test_golden_covers_the_cases():
    """the fixture exercises what the issue lists, each asserted from the files: an object that loses every vertex to later
    objects, objectId gaps (zero rows that survive the filter), rows dropped for labels 1 / 2 / 22, wall / floor / ceiling
    groups, scene0217_00 and a scan without axisAlignment"""
    assert "scene0217_00" in CASES
    assert any(b"axisAlignment" not in golden_files(c)[c + ".txt"] for c in CASES)
    lost = dropped = zero_rows = 0
    for c in CASES:
        groups = json.loads(golden_files(c)[c + ".aggregation.json"])["segGroups"]
        assert {"wall", "floor", "ceiling"} <= {g["label"] for g in groups}
        objs = _prefilter_objects(c)
        boxes = G[c + "/instance_bboxes"]
        kept_ids = set(boxes[:, 7].astype(int).tolist())
        for o, owns, lists, label in objs:
            if lists and not owns:                          # listed segments, all claimed by later objects
                lost += 1
                assert o not in kept_ids
            if owns and label in (1, 2, 22):                # a real row, dropped by process_one_scan's filter
                dropped += 1
                assert o not in kept_ids
            if owns and label not in (1, 2, 22):
                assert o in kept_ids
        present = {o for o, owns, _, _ in objs if owns}
        gaps = set(range(max(o for o, _, _, _ in objs) + 1)) - present
        zero_rows += int((~boxes.any(1)).sum())
        assert int((~boxes.any(1)).sum()) == len(gaps)      # every id without vertices leaves a zero row, label 0: kept
    assert lost >= 1 and dropped >= 1 and zero_rows >= 1


def test_split_read_ahead_is_bounded(monkeypatch):
    """export_split's reader keeps at most `threads` scans in flight beyond the one being consumed, and keeps none it has
    handed out"""
    import gc
    import threading
    import weakref
    started, lock = [], threading.Lock()

    class Parsed:
        pass

    def fake_read(path, name):
        with lock:
            started.append(name)
        return Parsed()

    monkeypatch.setattr(SX, "read_scan", fake_read)
    names = ["scene%04d_00" % i for i in range(40)]
    refs = []
    for i, (n, p) in enumerate(SX.iter_parsed("/nonexistent", names, threads=4)):
        assert n == names[i]
        with lock:
            assert len(started) <= i + 1 + 4, (i, len(started))
        refs.append(weakref.ref(p))
        del p
        gc.collect()
        assert all(r() is None for r in refs[:-1]), i      # nothing handed out before is retained
    assert started == names


def test_object_tables_alias_and_0217():
    groups = [(0, "wall", [1]), (3, "chair", [5, 6]), (1, "table", [7]), (7, "chair", [8]), (2, "lamp", []), (5, "door", [9])]
    oid, ls, ps, po = SX.object_tables(groups, "scene0000_00")
    assert oid.tolist() == [3, 1, 7, 2, 5]
    # the first chair also lists the later chair's segment (the reference's aliased list); the empty lamp carries 8 over
    assert ps.tolist() == [5, 6, 8, 7, 8, 9] and po.tolist() == [0, 0, 0, 1, 2, 4]
    assert ls.tolist() == [8, 7, 8, 8, 9]
    oid, ls, ps, po = SX.object_tables(groups, "scene0217_00")
    assert oid.tolist() == [1, 2]                          # sorted ids [1, 2, 3, 5, 7], first half
    with pytest.raises(ValueError):
        SX.object_tables([(0, "wall", [1]), (1, "floor", [2])], "scene0000_00")
    with pytest.raises(ValueError):
        SX.object_tables([(0, "lamp", []), (1, "desk", [2])], "scene0000_00")


def test_placeholder_branch():
    scan = SS.make_scan(5, n=400, annotated=False)
    files = SS.scan_files("scene0707_00", scan)
    assert "scene0707_00.aggregation.json" not in files
    r = R.export_files(files, "scene0707_00")
    assert r["sem_labels"].dtype == np.float64 and (r["sem_labels"] == -1.0).all()
    assert r["instance_ids"].dtype == np.int64 and (r["instance_ids"] == -1).all()
    for k in ("instance_bboxes", "aligned_instance_bboxes"):
        assert r[k].shape == (1, 8) and r[k].dtype == np.float64 and not r[k].any()
    assert (r["inst_gt"] == 0).all()


def test_read_scan_errors(tmp_path):
    scan = SS.make_scan(6, n=500)
    files = SS.scan_files("scene0008_00", scan)
    d = SS.write_files(str(tmp_path / "scene0008_00"), files)
    p = SX.read_scan(d)
    assert p.scene_id == "scene0008_00" and len(p.vertex) == 500 and p.tables is not None
    segs = json.loads(files["scene0008_00_vh_clean_2.0.010000.segs.json"])
    segs["segIndices"] = segs["segIndices"][:-1]
    bad = dict(files, **{"scene0008_00_vh_clean_2.0.010000.segs.json": json.dumps(segs).encode()})
    SS.write_files(str(tmp_path / "short" / "scene0008_00"), bad)
    with pytest.raises(ValueError, match="segment indices"):
        SX.read_scan(str(tmp_path / "short" / "scene0008_00"))
    agg = json.loads(files["scene0008_00.aggregation.json"])
    agg["segGroups"] = [g for g in agg["segGroups"] if g["label"] in ("wall", "floor", "ceiling")]
    bad = dict(files, **{"scene0008_00.aggregation.json": json.dumps(agg).encode()})
    SS.write_files(str(tmp_path / "noobj" / "scene0008_00"), bad)
    with pytest.raises(ValueError):
        SX.read_scan(str(tmp_path / "noobj" / "scene0008_00"))


def test_reference_dict_keys_and_dtypes():
    import torch
    n = 5
    e = SX.ScanExport("scene0000_00", torch.zeros((n, 9)), torch.zeros((n, 9)), torch.zeros(n, dtype=torch.float64),
                      torch.zeros(n, dtype=torch.float64), torch.zeros((2, 8), dtype=torch.float64),
                      torch.zeros((2, 8), dtype=torch.float64), torch.zeros(n, dtype=torch.int32), True)
    d = e.to_reference_dict()
    assert tuple(d) == KEYS
    for k in KEYS:
        assert isinstance(d[k], np.ndarray) and d[k].dtype == G[CASES[0] + "/" + k].dtype, k
