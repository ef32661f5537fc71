"""d3net_amd.scan_export on the device (csrc/scan_export.hip) against the reference's own outputs (tests/golden/scan_export_golden.npz)
and the numpy restatement (tests/scan_export_restate.py) on ScanNet-size scans: mesh, normals, ids, labels, boxes and instance GT
bit for bit (aligned xyz within 1 ulp of the reference's BLAS order), determinism, the chain into multiview projection and
scene_prep.prepare_scene, the saved .pth, and the range / argument errors."""
import ctypes as C
import json
import os
import types

import numpy as np
import pytest
import torch

import scan_export_restate as R
import scan_synth as SS
from d3net_amd import _lib, multiview as MV, scan_export as SX, scene_prep as SP
from d3net_amd.pointgroup_ops import _stream
from test_scan_export import CASES, G, KEYS, golden_files, ulp_diff

pytestmark = pytest.mark.gpu

OUT_KEYS = KEYS + ("inst_gt",)


def _np(e, k):
    return getattr(e, k).cpu().numpy()


def _same_bits(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    if a.tobytes() != b.tobytes():
        raise AssertionError("%s: %d elements differ" % (what, int((a != b).sum())))


def _write(tmp_path, case, files):
    return SS.write_files(str(tmp_path / case), files)


@pytest.mark.parametrize("case", CASES)
def test_golden(dev, tmp_path, case):
    files = golden_files(case)
    e = SX.export_scan(_write(tmp_path, case, files), device=dev)
    g = lambda k: G["%s/%s" % (case, k)]
    for k in ("mesh", "sem_labels", "instance_ids", "instance_bboxes", "inst_gt"):
        _same_bits(_np(e, k), g(k), k)
    am = _np(e, "aligned_mesh")
    _same_bits(am[:, 3:], g("aligned_mesh")[:, 3:], "aligned rgb / normals")
    d = ulp_diff(am[:, :3], g("aligned_mesh")[:, :3])
    print("%s: aligned xyz elements off by 1 ulp: %d of %d" % (case, int((d > 0).sum()), d.size))
    assert d.max() <= 1 and (d > 0).sum() <= d.size // 100
    # the aligned boxes are exact against the restatement fed with the device's aligned xyz
    r = R.export_files(files, case)
    _same_bits(am, r["aligned_mesh"], "aligned mesh vs restatement")
    _same_bits(_np(e, "aligned_instance_bboxes"), r["aligned_instance_bboxes"], "aligned boxes")
    if d.max() == 0:
        _same_bits(_np(e, "aligned_instance_bboxes"), g("aligned_instance_bboxes"), "aligned boxes vs golden")


def _full_scan(seed, scene):
    return SS.make_scan(seed, n=250_000, n_faces=500_000, n_objects=60)


def test_fullsize_equals_restatement(dev, tmp_path):
    scene = "scene0100_00"
    files = SS.scan_files(scene, _full_scan(21, scene))
    e = SX.export_scan(_write(tmp_path, scene, files), device=dev)
    r = R.export_files(files, scene)
    assert r["instance_bboxes"].shape[0] > 40
    for k in OUT_KEYS:
        _same_bits(_np(e, k), r[k], k)
    # determinism: a second run is bitwise identical
    e2 = SX.export_scan(str(tmp_path / scene), device=dev)
    for k in OUT_KEYS:
        _same_bits(_np(e2, k), _np(e, k), "rerun " + k)


def test_placeholder_scan(dev, tmp_path):
    scene = "scene0707_00"
    files = SS.scan_files(scene, SS.make_scan(5, n=3000, annotated=False))
    e = SX.export_scan(_write(tmp_path, scene, files), device=dev)
    r = R.export_files(files, scene)
    assert not e.annotated
    for k in OUT_KEYS:
        _same_bits(_np(e, k), r[k], k)


def test_chain_into_prepare_scene(dev, tmp_path):
    """export -> multiview projection on the unaligned mesh xyz -> scene_from_export -> prepare_scene (host noise) equals
    prepare_scene fed the restatement's arrays"""
    case = CASES[0]
    files = golden_files(case)
    e = SX.export_scan(_write(tmp_path, case, files), device=dev)
    r = R.export_files(files, case)
    rs = np.random.RandomState(3)
    F = 6
    pts = r["mesh"][:, :3]
    poses = np.tile(np.eye(4, dtype=np.float32), (F, 1, 1))
    poses[:, :3, 3] = pts.mean(0) + rs.randn(F, 3).astype(np.float32) * 0.2
    poses[:, 2, 3] -= 2.0
    depths = (rs.rand(F, 32, 41) * 3 + 0.5).astype(np.float32)
    feats = rs.randn(F, 128, 32, 41).astype(np.float32)
    mv = MV.project_multiview_features(e.mesh[:, :3], depths, poses, feats)
    mv_ref = MV.project_multiview_features(pts, depths, poses, feats)
    assert torch.equal(mv, mv_ref)
    scene = SX.scene_from_export(e, multiview=mv)
    assert scene["feats"].shape == (len(pts), 134)
    ref_scene = {"points": r["aligned_mesh"][:, :3], "feats": np.concatenate([r["aligned_mesh"][:, 3:9], mv_ref.cpu().numpy()], 1),
                 "sem_labels": r["sem_labels"], "instance_ids": r["instance_ids"]}
    ns = types.SimpleNamespace
    cfg = ns(data=ns(scale=50, full_scale=[128, 512], max_num_point=250000, max_num_instance=128, requires_gt_mask=False,
                     requires_bbox=True, transform=ns(jitter=True, flip=True, rot=True)),
             model=ns(no_detection=False, no_captioning=True, no_grounding=True))
    msa = np.abs(np.random.RandomState(0).randn(18, 3)) + 0.5
    a = SP.prepare_scene(scene, cfg, msa, rng=np.random.RandomState(7), noise="host", device=dev)
    b = SP.prepare_scene(ref_scene, cfg, msa, rng=np.random.RandomState(7), noise="host", device=dev)
    assert set(a) == set(b)
    for k in a:
        if torch.is_tensor(a[k]):
            assert torch.equal(a[k], b[k]), k
        else:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


def test_saved_pth_round_trip(dev, tmp_path):
    case = CASES[1]
    e = SX.export_scan(_write(tmp_path, case, golden_files(case)), device=dev)
    path = str(tmp_path / "split" / "val" / (case + ".pth"))
    SX.save_scan(e, path)
    d = torch.load(path, weights_only=False)
    assert tuple(d) == KEYS
    for k in KEYS:
        _same_bits(d[k], e.to_reference_dict()[k], k)
    SX.write_inst_gt(e, str(tmp_path / "gt" / (case + ".txt")))
    np.testing.assert_array_equal(np.loadtxt(str(tmp_path / "gt" / (case + ".txt")), dtype=np.int64), G[case + "/inst_gt"])


def test_export_split(dev, tmp_path):
    names = []
    for i, seed in enumerate((31, 32, 33)):
        scene = "scene%04d_00" % (200 + i)
        SS.write_scan(str(tmp_path / "scans"), scene, SS.make_scan(seed, n=1500, annotated=i != 1))
        names.append(scene)
    out = SX.export_split(str(tmp_path / "scans"), names, str(tmp_path / "out"), "train", threads=3, device=dev,
                          gt_root=str(tmp_path / "gt"))
    assert out == names
    for scene in names:
        d = torch.load(str(tmp_path / "out" / "train" / (scene + ".pth")), weights_only=False)
        r = R.export_files(SS.scan_files(scene, SS.make_scan(31 + names.index(scene), n=1500, annotated=scene != names[1])), scene)
        for k in KEYS:
            _same_bits(d[k], r[k], scene + " " + k)
        assert os.path.exists(str(tmp_path / "gt" / "train" / (scene + ".txt")))


def test_data_errors(dev, tmp_path):
    scene = "scene0009_00"
    scan = SS.make_scan(8, n=800)
    files = SS.scan_files(scene, scan)
    bad = scan["labels"].copy()
    bad[17] = 150
    f2 = SS.scan_files(scene, dict(scan, labels=bad))
    with pytest.raises(ValueError, match="150"):
        SX.export_scan(_write(tmp_path / "lab", scene, f2), device=dev)
    faces = scan["faces"].copy()
    faces[3, 1] = 800
    f3 = SS.scan_files(scene, dict(scan, faces=faces))
    with pytest.raises(ValueError, match="outside the mesh"):
        SX.export_scan(_write(tmp_path / "face", scene, f3), device=dev)
    agg = dict(scan["agg"], segGroups=[dict(g) for g in scan["agg"]["segGroups"]])
    agg["segGroups"][4]["segments"] = agg["segGroups"][4]["segments"] + [int(scan["seg"].max()) + 1]
    f4 = SS.scan_files(scene, dict(scan, agg=agg))
    with pytest.raises(ValueError, match="no vertex carries"):
        SX.export_scan(_write(tmp_path / "seg", scene, f4), device=dev)
    SX.export_scan(_write(tmp_path / "ok", scene, files), device=dev)


def test_limits_and_arguments_before_launch(dev):
    L = _lib.lib()
    maxv, maxf, maxs, maxk, maxr = SX.limits()
    assert L.d3_scan_mesh_ws_bytes(maxv + 1, 10) == 0 and L.d3_scan_mesh_ws_bytes(10, maxf + 1) == 0
    assert L.d3_scan_labels_ws_bytes(10, maxs + 1, 1, 1, 1) == 0 and L.d3_scan_labels_ws_bytes(10, 10, 1, maxk + 1, 1) == 0
    assert L.d3_scan_labels_ws_bytes(10, 10, 1, 1, maxr + 1) == 0
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)
    flags = torch.zeros(2, dtype=torch.int32, device=dev)
    p = C.c_void_p(buf.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.d3_scan_mesh(p, maxv + 1, p, 1, None, p, p, p, p, 1 << 16, st) == -2
    assert L.d3_scan_mesh(p, 10, p, maxf + 1, None, p, p, p, p, 1 << 16, st) == -2
    assert L.d3_scan_mesh(None, 10, p, 1, None, p, p, p, p, 1 << 16, st) == -3
    assert L.d3_scan_mesh(C.c_void_p(buf.data_ptr() + 2), 10, p, 1, None, p, p, p, p, 1 << 16, st) == -3
    args = lambda N, S, P, K, R_, raw=p: (raw, p, N, S, p, p, P, p, p, K, R_, p, p, p, p, p, p, p, p, p, 1 << 16, st)
    assert L.d3_scan_labels(*args(10, maxs + 1, 1, 1, 1)) == -2
    assert L.d3_scan_labels(*args(10, 10, 1, maxk + 1, 1)) == -2
    assert L.d3_scan_labels(*args(10, 10, 1, 1, maxr + 1)) == -2
    assert L.d3_scan_labels(*args(0, 10, 1, 1, 1)) == -2
    assert L.d3_scan_labels(*args(10, 10, 1, 1, 1, raw=None)) == -3
    torch.cuda.synchronize()
    assert int(flags.sum()) == 0 and not buf.any()


def test_negative_segment_ids(dev, tmp_path):
    """segment ids are only keys to the reference: a scan whose ids are all shifted below zero exports like the restatement"""
    scene = "scene0011_00"
    scan = SS.make_scan(9, n=2000)
    shift = int(scan["seg"].max()) + 500
    agg = dict(scan["agg"], segGroups=[dict(g, segments=[s - shift for s in g["segments"]]) for g in scan["agg"]["segGroups"]])
    files = SS.scan_files(scene, dict(scan, seg=scan["seg"] - shift, agg=agg))
    e = SX.export_scan(_write(tmp_path, scene, files), device=dev)
    r = R.export_files(files, scene)
    assert (np.asarray(json.loads(files[scene + "_vh_clean_2.0.010000.segs.json"])["segIndices"]) < 0).all()
    for k in OUT_KEYS:
        _same_bits(_np(e, k), r[k], k)
    plain = R.export_files(SS.scan_files(scene, scan), scene)
    for k in OUT_KEYS:
        _same_bits(_np(e, k), plain[k], "unshifted " + k)


def test_object_table_guards(dev):
    """a direct caller's object tables outside the documented contract set flag 32 and are skipped, never used as an index:
    pair_obj = K, obj_id = R, a repeated obj_id.  The buffers are oversized so that even an unguarded index stays in them."""
    L = _lib.lib()
    N, S, K, R_ = 64, 8, 3, 4
    seg = torch.arange(N, dtype=torch.int32, device=dev) % S
    raw = torch.full((N,), 3, dtype=torch.int16, device=dev)
    mesh = torch.rand((N, 9), device=dev)
    pad = 1 << 20

    def run(pair_seg, pair_obj, obj_id, label_seg):
        t = lambda a: torch.tensor(a, dtype=torch.int32, device=dev)
        ps, po, oi, ls = t(pair_seg), t(pair_obj), t(obj_id + [0] * 64), t(label_seg + [0] * 64)
        ids = torch.empty(N, dtype=torch.float64, device=dev)
        sem = torch.empty(N, dtype=torch.float64, device=dev)
        gt = torch.empty(N, dtype=torch.int32, device=dev)
        bx = torch.zeros((R_ + 64) * 8, dtype=torch.float64, device=dev)
        abx = torch.zeros((R_ + 64) * 8, dtype=torch.float64, device=dev)
        flags = torch.zeros(2, dtype=torch.int32, device=dev)
        need = L.d3_scan_labels_ws_bytes(N, S, len(pair_seg), K, R_)
        ws = torch.empty(need + pad, dtype=torch.uint8, device=dev)
        p = lambda x: C.c_void_p(x.data_ptr())
        _lib.check(L.d3_scan_labels(p(raw), p(seg), N, S, p(ps), p(po), len(pair_seg), p(oi), p(ls), K, R_, p(mesh), p(mesh),
                                    p(ids), p(sem), p(gt), p(bx), p(abx), p(flags), p(ws), need, _stream()), "d3_scan_labels")
        torch.cuda.synchronize()
        return int(flags[0]), ids.cpu().numpy()

    ok, ids = run([0, 1, 2], [0, 1, 2], [0, 1, 3], [0, 1, 2])
    assert ok == 0 and set(np.unique(ids).tolist()) == {-1.0, 0.0, 1.0, 3.0}
    assert run([0, 1, 2], [0, 1, K], [0, 1, 3], [0, 1, 2])[0] == 32
    assert run([0, 1, 2], [0, 1, 2], [0, 1, R_], [0, 1, 2])[0] == 32
    assert run([0, 1, 2], [0, 1, 2], [0, 1, 1], [0, 1, 2])[0] == 32
