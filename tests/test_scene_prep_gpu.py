"""d3net_amd.scene_prep on the device (csrc/scene_prep.hip) against the reference's own outputs (tests/golden/scene_prep_golden.npz,
host noise), a host restatement on ScanNet-size scenes (tests/scene_prep_restate.py), `collate.sparse_collate_fn`, its device
noise mode, one detector training step, and its range errors."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

import scene_prep_restate as HR
from d3net_amd import _lib, scene_prep as SP
from d3net_amd.collate import sparse_collate_fn

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scene_prep_golden.npz"))
CASES = [str(c) for c in G["cases"]]
MSA = G["mean_size_arr"]
BOX_KEYS = SP._BOX_KEYS


def _g(case, key):
    return G["%s/%s" % (case, key)]


def _cfg(max_num_point=250000, full_scale=512, gt_mask=False, captioning=False):
    ns = types.SimpleNamespace
    return ns(data=ns(scale=50, full_scale=[128, full_scale], max_num_point=max_num_point, max_num_instance=128,
                      requires_gt_mask=bool(gt_mask), requires_bbox=True, transform=ns(jitter=True, flip=True, rot=True)),
              model=ns(no_detection=False, no_captioning=not captioning, no_grounding=True))


def _np(x):
    return x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def _ulp1(a, b, what):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    tol = np.spacing(np.maximum(np.abs(a), np.abs(b)))
    bad = np.abs(a.astype(np.float64) - b.astype(np.float64)) > tol
    assert not bad.any(), (what, int(bad.sum()), a[bad][:5], b[bad][:5])


def compare_sample(dev, ref):
    """the bounds of the issue: exact integers / masks / truncated voxel coordinates, 1 float32 ulp on coordinates and boxes,
    1e-6 relative on instance means, exact instance min / max"""
    assert int(dev["num_instance"]) == int(ref["num_instance"])
    for k in ("instance_ids", "sem_labels", "instance_num_point", "feats"):
        np.testing.assert_array_equal(_np(dev[k]), np.asarray(ref[k]), err_msg=k)
    if "gt_proposals_idx" in ref:
        np.testing.assert_array_equal(_np(dev["gt_proposals_idx"]), ref["gt_proposals_idx"])
        np.testing.assert_array_equal(_np(dev["gt_proposals_offset"]), ref["gt_proposals_offset"])
    _ulp1(_np(dev["locs"]), ref["locs"], "locs")
    _ulp1(_np(dev["locs_scaled"]), ref["locs_scaled"], "locs_scaled")
    np.testing.assert_array_equal(_np(dev["locs_scaled"]).astype(np.int64), np.asarray(ref["locs_scaled"]).astype(np.int64))
    di, ri = _np(dev["instance_info"]), np.asarray(ref["instance_info"])
    np.testing.assert_array_equal(di[:, 6:12], ri[:, 6:12])
    _ulp1(di[:, 3:6], ri[:, 3:6], "instance centre")
    np.testing.assert_allclose(di[:, 0:3], ri[:, 0:3], rtol=1e-6, atol=0)
    for k in BOX_KEYS:
        d, r = _np(dev[k]), np.asarray(ref[k])
        if r.dtype.kind == "f":
            _ulp1(d, r, k)
        else:
            np.testing.assert_array_equal(d, r, err_msg=k)


def _golden_scene(case):
    return {k: _g(case, "in_" + k) for k in ("points", "feats", "sem_labels", "instance_ids")}


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_golden_parity_host_noise(dev, case):
    max_num_point, full_scale, gt_mask, captioning, aug = (int(v) for v in _g(case, "cfg"))
    cfg = _cfg(max_num_point, full_scale, gt_mask, captioning)
    rng = np.random.RandomState(int(_g(case, "seed")))
    out = SP.prepare_scene(_golden_scene(case), cfg, MSA, rng=rng, is_augment=bool(aug), noise="host", device=dev)
    torch.cuda.synchronize()
    ref = {k: _g(case, k) for k in ["locs", "locs_scaled", "feats", "sem_labels", "instance_ids", "num_instance", "instance_info",
                                    "instance_num_point"] + list(BOX_KEYS)}
    if gt_mask:
        ref["gt_proposals_idx"], ref["gt_proposals_offset"] = _g(case, "gt_proposals_idx"), _g(case, "gt_proposals_offset")
    compare_sample(out, ref)
    assert rng.rand() == float(_g(case, "next_draw"))          # the same draws were taken
    if case == "nolabel":                                       # slot -1: the first instance sits in the last row, cid -1
        assert int(out["gt_bbox_label"][-1]) == 1 and int(out["gt_bbox_object_id"][-1]) == int(np.unique(_g(case, "instance_ids"))[0])


def scannet_scene(seed, n, extent=(9.0, 7.0, 2.8), n_inst=40):
    r = np.random.RandomState(seed)
    pts = (r.rand(n, 3) * np.array(extent)).astype(np.float32)
    centers = r.rand(n_inst, 3) * np.array(extent)
    d = np.linalg.norm(pts[:, None, :] - centers[None], axis=2)
    ids = np.where(d.min(1) < 0.8, d.argmin(1), -1).astype(np.int64)
    sem = r.randint(-1, 20, size=n).astype(np.int64)
    feats = (r.rand(n, 3) * 2 - 1).astype(np.float32)
    return dict(points=pts, feats=feats, sem_labels=sem, instance_ids=ids)


BIG = [(21, 180_000), (22, 290_000)]       # the second is over max_num_point = 250000: the crop runs


@pytest.mark.gpu
def test_scannet_size_scenes_match_host_restatement(dev):
    cfg = _cfg(gt_mask=True)
    for seed, n in BIG:
        scene = scannet_scene(seed, n)
        ref = HR.prepare(scene, cfg, MSA, np.random.RandomState(seed))
        out = SP.prepare_scene(scene, cfg, MSA, rng=np.random.RandomState(seed), noise="host", device=dev)
        compare_sample(out, ref)
        if n > 250000:
            assert len(ref["locs"]) <= 250000 < n


@pytest.mark.gpu
def test_prepare_batch_equals_sparse_collate(dev):
    cfg = _cfg(gt_mask=True)
    scenes = [scannet_scene(seed, n // 4) for seed, n in BIG] + [_golden_scene("crop")]
    rng = np.random.RandomState(9)
    refs = [HR.prepare(s, cfg, MSA, rng) for s in scenes]
    for r in refs:
        r.pop("valid")
    want = sparse_collate_fn(refs, device=dev)
    got = SP.prepare_batch(scenes, cfg, MSA, rng=np.random.RandomState(9), noise="host", device=dev)
    assert set(got) == set(want), set(got) ^ set(want)
    for k in want:
        w, g = _np(want[k]), _np(got[k])
        assert w.dtype == g.dtype and w.shape == g.shape, (k, w.dtype, g.dtype, w.shape, g.shape)
        if w.dtype.kind == "f" and k != "instance_info":
            _ulp1(g, w, k)
        elif k == "instance_info":
            np.testing.assert_array_equal(g[:, 6:], w[:, 6:])
            np.testing.assert_allclose(g[:, :6], w[:, :6], rtol=1e-6, atol=0)
        else:
            np.testing.assert_array_equal(g, w, err_msg=k)


@pytest.mark.gpu
def test_device_noise_deterministic_and_scaled(dev):
    cfg = _cfg(gt_mask=True)
    scenes = [scannet_scene(31, 60_000), _golden_scene("crop")]
    a = SP.prepare_batch(scenes, cfg, MSA, rng=np.random.RandomState(4), noise="device", device=dev)
    b = SP.prepare_batch(scenes, cfg, MSA, rng=np.random.RandomState(4), noise="device", device=dev)
    for k in a:
        assert torch.equal(a[k], b[k]), k

    # the generator itself: N(0, 1) moments over 4 M values
    L = _lib.lib()
    g = torch.empty(4 << 20, dtype=torch.float32, device=dev)
    assert L.d3_scene_noise(C.c_void_p(g.data_ptr()), g.numel(), 12345, None) == 0
    torch.cuda.synchronize()
    assert abs(float(g.mean())) < 3e-3 and abs(float(g.std()) - 1) < 3e-3

    # displacement std on a large scene without a crop, over two seeds: host and device noise agree within 5 %.  (One
    # realisation of the coarse grid has only ~20 k nodes, so a single seed's std varies by several percent.)
    big = scannet_scene(32, 300_000, extent=(40.0, 40.0, 6.0))
    cfg = _cfg(max_num_point=10 ** 7)
    std = {"host": 0.0, "device": 0.0}
    for seed in (8, 9):
        M = SP.augment_matrix(np.random.RandomState(seed), cfg.data.transform)
        base = np.matmul(big["points"], M) * 50
        base -= base.min(0)
        for mode in std:
            out = SP.prepare_scene(big, cfg, MSA, rng=np.random.RandomState(seed), noise=mode, device=dev)
            disp = _np(out["locs_scaled"]).astype(np.float64) - base
            std[mode] += disp.std(0).mean()
    assert abs(std["device"] / std["host"] - 1) < 0.05, std


@pytest.mark.gpu
def test_batch_trains_detector_step(dev):
    from d3net_amd.config import default_conf
    from d3net_amd.pointgroup import PointGroup
    cfg = default_conf(overrides={"model": {"blocks": [1, 2, 3]}})
    cfg.data.max_num_point = 30000
    torch.manual_seed(0)
    model = PointGroup(cfg).to(dev).train()
    scenes = [scannet_scene(41, 40_000, extent=(5.0, 4.0, 2.5), n_inst=12), scannet_scene(42, 25_000, extent=(4.0, 4.0, 2.5), n_inst=8)]
    m = cfg.model
    width = m.use_color * 3 + m.use_normal * 3 + m.use_multiview * 128          # the per-point features the backbone expects
    for i, sc in enumerate(scenes):
        sc["feats"] = np.random.RandomState(i).rand(len(sc["points"]), width).astype(np.float32)
    batch = SP.prepare_batch(scenes, cfg, MSA, rng=np.random.RandomState(1), noise="device", device=dev)
    loss, _ = model.training_step(batch)
    loss.backward()
    torch.cuda.synchronize()
    assert torch.isfinite(loss)


@pytest.mark.gpu
def test_oversize_inputs_return_range_error(dev):
    L = _lib.lib()
    mp, mg, mi = C.c_int(), C.c_int(), C.c_int()
    assert L.d3_scene_limits(C.byref(mp), C.byref(mg), C.byref(mi)) == 0
    assert L.d3_scene_transform(None, mp.value + 1, None, 50.0, 1, None, None, None) == -2
    assert L.d3_scene_elastic(None, 10, None, None, 4096, 4096, 4096, 1.0, None, 0, None) == -2
    assert L.d3_scene_elastic_ws_bytes(4096, 3, 3) == 0
    assert L.d3_scene_ws_bytes(10, mi.value + 1) == 0
    cfg = _cfg()
    far = scannet_scene(51, 2000)
    far["points"][0] = [3.0e4, 0.0, 0.0]                  # a grid far beyond the limits
    with pytest.raises(_lib.D3Error, match="D3_ERR_RANGE"):
        SP.prepare_scene(far, cfg, MSA, rng=np.random.RandomState(0), noise="device", device=dev)
    big_id = scannet_scene(52, 2000)
    big_id["instance_ids"][5] = mi.value + 1
    with pytest.raises(_lib.D3Error, match="D3_ERR_RANGE"):
        SP.prepare_scene(big_id, cfg, MSA, rng=np.random.RandomState(0), is_augment=False, device=dev)
