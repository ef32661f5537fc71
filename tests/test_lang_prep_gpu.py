"""d3net_amd.lang_prep on the device (csrc/lang_prep.hip): exact parity with the reference's collated batches
(tests/golden/lang_prep_golden.npz), the two entry points against the host restatement (tests/lang_prep_restate.py) at the sizes and
edge cases the golden cannot hold, their argument / range errors, and one PipelineNet grounding step on a prepared batch."""
import ctypes as C
import json
import os
import random
import types

import numpy as np
import pytest
import torch

import lang_prep_restate as LR
from d3net_amd import _lib, lang_prep as LP

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "lang_prep_golden.npz"))
ANN = json.loads(str(G["annotations_json"]))
TSV = os.path.join(HERE, "golden", "lang_prep_labels.tsv")
SEED, MAX_DES_LEN, CHUNK = int(G["seed"]), int(G["max_des_len"]), int(G["chunk"])
MSA = G["mean_size_arr"]

DESCRIPTION_KEYS = ("lang_feat", "lang_len", "lang_ids", "annotated", "chunk_ids", "object_id", "ann_id", "object_cat", "unique_multiple",
                    "ref_box_label", "ref_box_corner_label", "scene_object_ids", "scene_object_rotations", "scene_object_rotation_masks",
                    "id", "istrain")
BOX_KEYS = ("center_label", "sem_cls_label", "heading_class_label", "heading_residual_label", "size_class_label", "size_residual_label",
            "gt_bbox_object_id", "gt_bbox_label", "gt_bbox")


def _np(x):
    return x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def _cfg():
    ns = types.SimpleNamespace
    return ns(data=ns(scale=50, full_scale=[128, 512], max_num_point=250000, max_num_instance=128, requires_gt_mask=True,
                      requires_bbox=True, transform=ns(jitter=True, flip=True, rot=True)),
              model=ns(no_detection=False, no_captioning=False, no_grounding=True))


def _scenes():
    return {sid: {k: G["scene/%s/%s" % (sid, k)] for k in ("points", "feats", "sem_labels", "instance_ids")}
            for sid in sorted({d["scene_id"] for d in ANN["raw_data"]})}


def _index(dev):
    return LP.DescriptionIndex(ANN["raw_data"], ANN["vocabulary"], G["glove"], MAX_DES_LEN, CHUNK, LP.raw2label_from_tsv(TSV),
                               scan2cad_rotation=ANN["scan2cad_rotation"], device=dev)


def _ulp1(a, b, what):
    """scene_prep's bound on coordinates and boxes: one float32 ulp"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    tol = np.spacing(np.maximum(np.abs(a), np.abs(b)))
    bad = np.abs(a.astype(np.float64) - b.astype(np.float64)) > tol
    assert not bad.any(), (what, int(bad.sum()), a[bad][:5], b[bad][:5])


def _point_half(got, run):
    """scene_prep's bounds: exact integers, masks and truncated voxel coordinates, 1 float32 ulp on coordinates and boxes, 1e-6
    relative on instance means, exact instance min / max"""
    for k in ("instance_ids", "sem_labels", "instance_num_point", "feats", "batch_offsets", "instance_offsets", "gt_proposals_idx",
              "gt_proposals_offset", "locs_scaled"):
        w, g = G["%s/%s" % (run, k)], _np(got[k])
        assert w.dtype == g.dtype, (k, w.dtype, g.dtype)
        np.testing.assert_array_equal(g, w, err_msg=k)
    _ulp1(_np(got["locs"]), G[run + "/locs"], "locs")
    gi, wi = _np(got["instance_info"]), G[run + "/instance_info"]
    np.testing.assert_array_equal(gi[:, 6:12], wi[:, 6:12])
    _ulp1(gi[:, 3:6], wi[:, 3:6], "instance centre")
    np.testing.assert_allclose(gi[:, 0:3], wi[:, 0:3], rtol=1e-6, atol=0)
    for k in BOX_KEYS:
        w, g = G["%s/%s" % (run, k)], _np(got[k])
        assert w.dtype == g.dtype, (k, w.dtype, g.dtype)
        if w.dtype.kind == "f":
            _ulp1(g, w, k)
        else:
            np.testing.assert_array_equal(g, w, err_msg=k)


@pytest.mark.parametrize("run", ["aug", "plain"])
def test_golden_parity(dev, run):
    index = _index(dev)
    rng, pyrng = np.random.RandomState(SEED), random.Random(SEED)
    got = LP.prepare_pipeline_batch(index, range(len(index)), _scenes(), _cfg(), MSA, rng=rng, pyrng=pyrng, is_augment=run == "aug",
                                    noise="host", device=dev)
    torch.cuda.synchronize()
    assert got["scene_id"] == [str(s) for s in G[run + "/scene_id"]]
    for k in DESCRIPTION_KEYS:
        want = torch.from_numpy(G["%s/%s" % (run, k)])
        assert got[k].dtype == want.dtype and got[k].shape == want.shape, (k, got[k].dtype, want.dtype, got[k].shape, want.shape)
        assert torch.equal(got[k].cpu(), want), k
    assert (pyrng.random(), rng.rand()) == tuple(G[run + "/next_draws"][-1])          # the same draws were taken
    _point_half(got, run)
    # the corner label is the matched gt_bbox row of the same output, bit for bit, and zero where nothing matches
    ref, corner, box = _np(got["ref_box_label"]), _np(got["ref_box_corner_label"]), _np(got["gt_bbox"])
    matched = 0
    for b, j in np.ndindex(ref.shape[:2]):
        rows = np.nonzero(ref[b, j])[0]
        assert len(rows) <= 1
        if len(rows):
            assert corner[b, j].tobytes() == box[b, rows[-1]].tobytes()
            matched += 1
        else:
            assert not corner[b, j].any()
    assert 0 < matched < ref.shape[0] * ref.shape[1]
    assert int(_np(got["gt_bbox_label"])[2, -1]) == 1                                  # the first instance of the scene without id -1 sits in row -1


def test_descriptions_without_boxes(dev):
    index = _index(dev)
    got = LP.prepare_descriptions(index, [2, 0], device=dev)
    assert "ref_box_label" not in got and "scene_object_rotations" not in got
    for k in ("lang_feat", "lang_len", "lang_ids", "object_id", "unique_multiple"):
        assert torch.equal(got[k].cpu(), torch.from_numpy(G["plain/" + k][[2, 0]])), k
    assert got["id"].tolist() == [2, 0]


# ------------------------------------------------------------------------------------------------ the entry points
def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _hp(a):
    return a.ctypes.data_as(C.c_void_p)


def _tables(D, L, V=11, Nd=5, seed=0):
    r = np.random.RandomState(seed)
    lens = np.array([L, 2, 3, max(L // 2, 2), min(L, 5)], np.int32)[:Nd]
    tokens = np.zeros((Nd, L), np.int32)
    for i in range(Nd):
        tokens[i, :lens[i]] = r.randint(0, V, lens[i])
    tokens[0, L - 1] = V - 1                                                      # the table's last row, at the last position
    glove = r.randn(V, D).astype(np.float32)
    return tokens, lens, glove


def _slots(S, L):
    """slot 0: every position erased; then a -1 row, a slot with no erase, partial erases (also past the description's end)"""
    rows = np.array([0, -1, 1, 2, 0, 3, 4], np.int32)[:S]
    erase = [np.arange(L), [], [], [1], [0, L - 1], [L - 1], [2, 1]][:S]
    return rows, [np.asarray(e, np.int32) for e in erase]


def _run_features(dev, tokens, lens, glove, unk, rows, erase, L, D):
    S = len(rows)
    eptr = np.zeros(S + 1, np.int32)
    eptr[1:] = np.cumsum([len(e) for e in erase])
    epos = np.ascontiguousarray(np.concatenate(erase), np.int32)
    t, n, g = (torch.from_numpy(x).to(dev) for x in (tokens, lens, glove))
    feat = torch.full((S, L, D), 7.0, dtype=torch.float32, device=dev)
    ids = torch.full((S, L), 7, dtype=torch.int64, device=dev)
    ln = torch.full((S,), 7, dtype=torch.int64, device=dev)
    lib = _lib.lib()
    ws = torch.empty(max(int(lib.d3_lang_features_ws_bytes(S, len(epos))), 1), dtype=torch.uint8, device=dev)
    rc = lib.d3_lang_features(_ptr(t), _ptr(n), tokens.shape[0], _ptr(g), glove.shape[0], D, L, unk, _hp(rows), _hp(eptr), _hp(epos), S,
                              _ptr(feat), _ptr(ids), _ptr(ln), _ptr(ws), ws.numel(), None)
    torch.cuda.synchronize()
    return rc, feat.cpu().numpy(), ids.cpu().numpy(), ln.cpu().numpy()


@pytest.mark.parametrize("S", [1, 7])
@pytest.mark.parametrize("L", [8, 128])
@pytest.mark.parametrize("D", [300, 4])
def test_lang_features_against_restatement(dev, D, L, S):
    tokens, lens, glove = _tables(D, L)
    rows, erase = _slots(S, L)
    unk = 1
    rc, feat, ids, ln = _run_features(dev, tokens, lens, glove, unk, rows, erase, L, D)
    assert rc == 0
    wf, wi, wl = LR.lang_features(LR.description_store(tokens, lens, glove), lens, glove, unk, rows, erase, L)
    np.testing.assert_array_equal(feat, wf)
    np.testing.assert_array_equal(ids, wi)
    np.testing.assert_array_equal(ln, wl)
    assert (feat[0] == glove[unk]).all() and ids[0, L - 1] == glove.shape[0] - 1       # all erased; ids keep the tokens
    if S > 2:
        assert not feat[1].any() and ln[1] == 0 and not ids[1].any()                   # the -1 row
        assert not feat[2, 2:].any() and (feat[2, :2] == glove[tokens[1, :2]]).all()   # no erase: exact zeros after the tokens


@pytest.mark.parametrize("what,code", [("D", -3), ("erase_high", -3), ("erase_low", -3), ("row_high", -2), ("row_low", -2)])
def test_lang_features_errors_leave_outputs_untouched(dev, what, code):
    L, D = 8, 300
    tokens, lens, glove = _tables(D, L)
    rows, erase = _slots(7, L)
    if what == "D":
        D = 6
        glove = np.ascontiguousarray(glove[:, :6])
    elif what == "erase_high":
        erase[3] = np.array([L], np.int32)
    elif what == "erase_low":
        erase[3] = np.array([-1], np.int32)
    elif what == "row_high":
        rows[6] = tokens.shape[0]
    else:
        rows[6] = -2
    rc, feat, ids, ln = _run_features(dev, tokens, lens, glove, 1, rows, erase, L, D)
    assert rc == code
    assert (feat == 7).all() and (ids == 7).all() and (ln == 7).all()
    with pytest.raises(_lib.D3Error, match="D3_ERR_ARG" if code == -3 else "D3_ERR_RANGE"):
        _lib.check(rc, "d3_lang_features")


def _run_targets(dev, gid, glab, gbox, oid, tables, scene):
    B, R = gid.shape
    Cn = oid.shape[1]
    off, ids, mats = [0], [], []
    for t in tables:
        for k, m in t.items():
            ids.append(k)
            mats.append(m)
        off.append(len(ids))
    Ns = len(tables)
    d = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    g_id, g_lab, g_box, o_id = d(gid, np.int64), d(glab, np.int64), d(gbox, np.float32), d(oid, np.int64)
    r_off, r_ids, r_mats = d(off, np.int32), d(np.asarray(ids).reshape(-1), np.int32), d(np.asarray(mats).reshape(-1, 3, 3), np.float32)
    ref = torch.full((B, Cn, R), 7, dtype=torch.int64, device=dev)
    corner = torch.full((B, Cn, 8, 3), 7.0, dtype=torch.float32, device=dev)
    rots = torch.full((B, R, 3, 3), 7.0, dtype=torch.float32, device=dev)
    masks = torch.full((B, R), 7, dtype=torch.int64, device=dev)
    lib = _lib.lib()
    ws = torch.empty(int(lib.d3_ref_targets_ws_bytes(B)), dtype=torch.uint8, device=dev)
    sc = np.ascontiguousarray(scene, np.int32)
    rc = lib.d3_ref_targets(_ptr(g_id), _ptr(g_lab), _ptr(g_box), _ptr(o_id), B, Cn, R, _ptr(r_off) if Ns else None,
                            _ptr(r_ids) if Ns else None, _ptr(r_mats) if Ns else None, Ns, _hp(sc), _ptr(ref), _ptr(corner), _ptr(rots),
                            _ptr(masks), _ptr(ws), ws.numel(), None)
    torch.cuda.synchronize()
    return rc, [x.cpu().numpy() for x in (ref, corner, rots, masks)]


def _target_inputs(R, seed=0):
    r = np.random.RandomState(seed)
    B, Cn = 3, 5
    gid, glab = np.zeros((B, R), np.int64), np.zeros((B, R), np.int64)
    for b in range(B):
        k = (5, R - 1, R)[b]                                # a few boxes, all rows but one, every row
        gid[b, :k] = r.permutation(2 * R)[:k]
        glab[b, :k] = 1
    gid[0, -1], glab[0, -1] = 150, 1                          # the first instance in row -1
    gid[0, 7] = gid[0, 2]                                     # the same id in an unlabelled row: no match there
    gbox = r.randn(B, R, 8, 3).astype(np.float32)
    oid = np.array([[gid[0, 2], 150, -1, 999, gid[0, 0]], [gid[1, R - 2], 0, gid[1, 0], 999, -1],
                    [gid[2, R - 1], gid[2, 64 % R], gid[2, 0], 999, gid[2, 1]]], np.int64)
    t0 = {int(gid[0, 1]): r.randn(3, 3), 150: r.randn(3, 3), 100000: r.randn(3, 3)}
    t1 = {int(k): r.randn(3, 3) for k in gid[2, ::3]}         # more than one wave's worth of entries when R is 128
    return gid, glab, gbox, oid, [t0, {}, t1]


@pytest.mark.parametrize("R", [128, 70])
def test_ref_targets_against_restatement(dev, R):
    gid, glab, gbox, oid, tables = _target_inputs(R)
    for scene in ([0, -1, 2], [1, 0, -1]):
        rc, got = _run_targets(dev, gid, glab, gbox, oid, tables, scene)
        assert rc == 0
        want = LR.ref_targets(gid, glab, gbox, oid, [tables[s] if s >= 0 else None for s in scene])
        for g, w, k in zip(got, want, ("ref_box_label", "ref_box_corner_label", "rotations", "masks")):
            assert g.dtype == w.dtype, k
            np.testing.assert_array_equal(g, w, err_msg=k)
    assert got[0][0, 1, -1] == 1 and got[0][0, 0].sum() == 1 and not got[0][0, 2].any()
    rc, got = _run_targets(dev, gid, glab, gbox, oid, [], [-1, -1, -1])              # no Scan2CAD annotations at all
    assert rc == 0 and not got[2].any() and not got[3].any()


def test_ref_targets_scene_outside_table_is_a_range_error(dev):
    gid, glab, gbox, oid, tables = _target_inputs(70)
    for scene in ([0, 3, 1], [0, -2, 1]):
        rc, got = _run_targets(dev, gid, glab, gbox, oid, tables, scene)
        assert rc == -2 and all((g == 7).all() for g in got)


# ------------------------------------------------------------------------------------------------ one training step
def _training_inputs(dev, V=200):
    from d3net_amd import synthetic as S
    from d3net_amd.config import default_conf
    cfg = default_conf(overrides={
        "model": {"blocks": [1, 2, 3], "num_graph_steps": 2, "num_locals": 10, "use_relation": True, "use_orientation": True,
                  "match_type": "Transformer", "use_lang_classifier": True, "use_bidir": False, "num_bbox_class": 18,
                  "loss_type": "cross_entropy", "no_captioning": True, "no_grounding": False},
        "data": {"num_des_per_scene": 4, "max_spk_len": 30, "max_lis_len": 126, "min_iou_threshold": 0.25, "num_ori_bins": 6},
        "train": {"use_rl": False, "sample_topn": 1}})
    vocabulary = S.make_vocabulary(V)
    glove = np.random.default_rng(0).standard_normal((V, 300)).astype(np.float32)
    scenes, raw, r = {}, [], np.random.RandomState(2)
    lengths = iter([130, 12, 40, 126, 77, 10, 125])           # one over max_lis_len, one exactly at it
    for n, seed in enumerate((3, 4)):
        sc = S.small_scene(dims=(40, 32, 20), n_boxes=3, seed=seed)
        sid = "scene%04d_00" % n
        scenes[sid] = dict(points=sc["locs"], feats=sc["feats"], sem_labels=sc["sem_labels"], instance_ids=sc["instance_ids"])
        for j in range(4 - n):                               # the second scene's chunk is one short: its last slot repeats
            raw.append({"scene_id": sid, "object_id": str(j % 3), "object_name": "chair", "ann_id": str(j // 3),
                        "token": ["w%d" % w for w in r.randint(0, V - 4, next(lengths))]})
    index = LP.DescriptionIndex(raw, vocabulary, glove, cfg.data.max_lis_len, cfg.data.num_des_per_scene, {"chair": 2},
                                scan2cad_rotation={"scene0000_00": {"0": np.eye(3).tolist()}}, device=dev)
    return cfg, index, scenes, types.SimpleNamespace(vocabulary=vocabulary, glove=glove)


def test_prepared_batch_trains_grounding_step(dev):
    from d3net_amd.pipeline import PipelineNet
    cfg, index, scenes, train = _training_inputs(dev)
    batches = [LP.prepare_pipeline_batch(index, [0, 1], scenes, cfg, MSA, rng=np.random.RandomState(1), pyrng=random.Random(1),
                                         is_augment=True, noise="device", device=dev) for _ in range(2)]
    assert set(batches[0]) == set(batches[1])
    for k, v in batches[0].items():                          # the same seeds: bit-identical inputs
        assert torch.equal(v, batches[1][k]) if torch.is_tensor(v) else v == batches[1][k], k
    assert batches[0]["lang_feat"].shape == (2, 4, 128, 300) and int(batches[0]["lang_len"].max()) == 128
    torch.manual_seed(0)
    net = PipelineNet(cfg, {"train": train}).to(dev).train()
    assert net.mode == 2
    net.detector.teacher = True
    loss, d = net.training_step(batches[0])
    assert torch.isfinite(loss) and torch.isfinite(d["ref_loss"]) and torch.isfinite(d["lang_loss"])
    loss.backward()
    grads = [p.grad for p in net.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(g).all() for g in grads)
