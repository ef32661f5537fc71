"""scene_prep.prepare_batch_store (csrc/batch_prep.hip) against the per-scene path it replaces,
`collate_scenes_device([prepare_scene(store.scene(s), ...) for s in ids])`, which tests/test_scene_prep*.py and
tests/test_collate_device_gpu.py pin to the reference: every key equal bit for bit, over the shapes at which the kernels change
path (one point, around one 256-thread block, several tiles, 3 and 131 feature columns, aligned and unaligned feature rows), the
label edge cases of the box-slot rule, the float32 and the float64 coordinate path, and the host side (random draws, refusals,
the store left untouched, no host synchronisation)."""
import os

import numpy as np
import pytest
import torch

from d3net_amd import _lib
from d3net_amd import dataset as D
from d3net_amd import scene_prep as SP
from d3net_amd.config import default_conf

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MSA = np.load(os.path.join(HERE, "golden", "lang_prep_golden.npz"))["mean_size_arr"]


def _cfg(R=128, gt=True):
    # a language mode: is_augment then draws jitter / flip / rot and runs the float64 path without elastic distortion or crop
    return default_conf(overrides={"model": {"no_captioning": True, "no_grounding": False},
                                   "data": {"max_num_instance": R, "requires_gt_mask": gt, "batch_size": 4}})


def _scene(n, ids, width=3, seed=0):
    r = np.random.RandomState(seed)
    ids = np.asarray(ids, np.int32)
    assert ids.shape == (n,)
    return {"points": ((r.rand(n, 3) - 0.3) * np.array([4.0, 3.0, 2.0])).astype(np.float32), "feats": r.randn(n, width).astype(np.float32),
            "sem_labels": r.randint(-1, 20, n).astype(np.int32), "instance_ids": ids}


def _random_ids(n, k, seed):
    return np.random.RandomState(100 + seed).randint(-1, k, n)


def _assert_batches_equal(got, want):
    assert set(got) == set(want)
    for k, w in want.items():
        g = got[k]
        if torch.is_tensor(w):
            assert g.dtype == w.dtype and g.shape == w.shape, (k, g.dtype, w.dtype, g.shape, w.shape)
            assert torch.equal(g, w), k
        else:
            assert g == w, k


def _per_scene(store, ids, cfg, rng, is_augment, dev):
    samples = [SP.prepare_scene(store.scene(s), cfg, MSA, rng=rng, is_augment=is_augment, noise="device", device=dev) for s in ids]
    return SP.collate_scenes_device(samples, dev, cfg.data.mode)


def _check(store, ids, cfg, is_augment, dev, seed=11):
    r0, r1 = np.random.RandomState(seed), np.random.RandomState(seed)
    want = _per_scene(store, ids, cfg, r0, is_augment, dev)
    got = SP.prepare_batch_store(store, ids, cfg, MSA, rng=r1, is_augment=is_augment, device=dev, mode=cfg.data.mode)
    _assert_batches_equal(got, want)
    s0, s1 = r0.get_state(), r1.get_state()
    assert s0[0] == s1[0] and np.array_equal(s0[1], s1[1]) and s0[2:] == s1[2:]
    return got


SIZES = (1, 255, 256, 257, 2500)


@pytest.fixture(scope="module")
def stores(dev):
    return {w: D.SceneStore.from_scenes({"n%d" % n: _scene(n, _random_ids(n, 7, n), w, seed=n) for n in SIZES}, device=dev) for w in (3, 131)}


@pytest.mark.parametrize("is_augment", [False, True])
@pytest.mark.parametrize("gt", [True, False])
@pytest.mark.parametrize("width", [3, 131])
@pytest.mark.parametrize("ids", [("n2500",), ("n1", "n255", "n256"), ("n257", "n2500", "n1", "n255")])
def test_shapes_and_modes(dev, stores, ids, width, gt, is_augment):
    store = stores[width]
    before = {k: getattr(store, k).clone() for k in D._FIELDS}
    got = _check(store, list(ids), _cfg(gt=gt), is_augment, dev)
    assert ("gt_proposals_idx" in got) == gt and got["feats"].shape[1] == width and got["batch_offsets"].numel() == len(ids) + 1
    for k, v in before.items():                              # the store was read, not written
        assert torch.equal(getattr(store, k), v), k


def _edge_scenes():
    r = np.random.RandomState(5)
    many = np.concatenate([np.arange(130), r.randint(-1, 130, 2500 - 130)])
    sizes = np.concatenate([np.full(100, 0), np.full(64, 1), np.full(65, 3), np.full(1, 4), np.full(30, -1)])
    return {
        "allneg": _scene(300, np.full(300, -1), seed=1),
        "nounl_small": _scene(200, r.randint(0, 2, 200), seed=2),                 # K - 1 = 1 < R - 1: the k = -1 row stays
        "nounl_over": _scene(400, np.concatenate([np.arange(5), r.randint(0, 5, 395)]), seed=3),   # R = 4: an instance takes row R - 1
        "gaps": _scene(333, r.choice([-1, 0, 2, 5], 333), seed=4),
        "six": _scene(500, np.concatenate([np.arange(-1, 6), r.randint(-1, 6, 493)]), seed=5),
        "many": _scene(2500, r.permutation(many), seed=6),
        "many_nounl": _scene(2500, r.permutation(np.where(many < 0, 7, many)), seed=7),
        "sizes": _scene(260, r.permutation(sizes), seed=8),
        "odd": _scene(255, r.randint(-1, 3, 255), seed=9),
    }


@pytest.fixture(scope="module")
def edge_store(dev):
    return D.SceneStore.from_scenes(_edge_scenes(), device=dev)


EDGE_BATCHES = [
    (("allneg", "gaps", "six"), 4), (("gaps", "allneg", "six"), 4), (("gaps", "six", "allneg"), 4), (("allneg",), 4),
    (("nounl_small", "nounl_over"), 4), (("nounl_over", "nounl_small"), 128),
    (("six", "gaps"), 4),
    (("many", "many_nounl"), 128), (("many_nounl", "many"), 140),
    (("sizes",), 128),
    (("odd", "sizes", "odd", "gaps"), 128),                   # a scene after an odd point total: the unaligned word path
    (("gaps", "many", "gaps"), 128),                          # one scene in two slots
]


@pytest.mark.parametrize("is_augment", [False, True])
@pytest.mark.parametrize("ids,R", EDGE_BATCHES)
def test_label_edge_cases(dev, edge_store, ids, R, is_augment):
    got = _check(edge_store, list(ids), _cfg(R=R), is_augment, dev)
    assert got["center_label"].shape == (len(ids), R, 3)
    if ids == ("nounl_over", "nounl_small") or R == 4 and "nounl_over" in ids:
        row = ids.index("nounl_over")
        assert int(got["gt_bbox_label"][row].sum()) == min(R, 5)


def test_edge_scenes_are_what_they_claim():
    sc = _edge_scenes()
    count = lambda name, v: int((sc[name]["instance_ids"] == v).sum())
    assert count("sizes", 0) == 100 and count("sizes", 1) == 64
    assert len(np.unique(sc["many"]["instance_ids"])) == 131 and sc["many_nounl"]["instance_ids"].min() == 0
    assert sc["nounl_small"]["instance_ids"].min() == 0 and set(np.unique(sc["gaps"]["instance_ids"])) == {-1, 0, 2, 5}
    assert (255 * 3) % 4 != 0


def test_refusals(dev):
    L = _lib.lib()
    assert L.d3_batch_prepare_table_bytes(0) == 0 and L.d3_batch_prepare_table_bytes(513) == 0
    assert L.d3_batch_prepare_table_bytes(512) > 0
    bad = D.SceneStore.from_scenes({"fine": _scene(10, np.zeros(10)), "broken_scene": _scene(10, np.array([0] * 9 + [-2]))}, device=dev)
    with pytest.raises(_lib.D3Error, match="broken_scene"):
        bad.instance_index()
    pinned = D.SceneStore.from_scenes({"fine": _scene(10, np.zeros(10))}, device="cpu")
    with pytest.raises(ValueError):
        pinned.instance_index()
    assert pinned.index_bytes() == 0
    detector = default_conf(overrides={"model": {"no_captioning": True, "no_grounding": True}})
    ok = D.SceneStore.from_scenes({"fine": _scene(10, np.zeros(10))}, device=dev)
    with pytest.raises(ValueError):                          # elastic distortion and crop: prepare_scene's
        SP.prepare_batch_store(ok, ["fine"], detector, MSA, rng=np.random.RandomState(0), is_augment=True, device=dev)
    assert ok.index_bytes() == 0 and ok.instance_index() is ok.instance_index()
    assert ok.index_bytes() == 4 * 10 + 3 * 4 * 2 and ok.bytes() == 10 * (12 + 12 + 4 + 4)


def test_no_host_synchronisation(dev, stores):
    """one warmed batch of a fused detector-mode loader under torch's sync debug mode: nothing at the torch level may wait for
    the device (the voxelisation's count read-back is the library's own, as on every path)"""
    cfg = default_conf(overrides={"model": {"no_captioning": True, "no_grounding": True}, "data": {"batch_size": 4, "requires_gt_mask": True}})
    loader = D.PipelineLoader(cfg, stores[131], None, "val", "detector", seed=3, mean_size_arr=MSA, device=dev, fused=True)
    assert loader.fused_active()
    rng, pyrng = loader.generators(0)
    order = loader.order(0)[:4]
    for _ in range(2):                                      # warm: the index, the cached mean sizes, workspace and tables
        loader.build(order, rng, pyrng)
    torch.cuda.set_sync_debug_mode("error")
    try:
        assert torch.cuda.get_sync_debug_mode() == 2
        batch = loader.build(order, rng, pyrng)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert batch["locs"].shape[0] == sum(stores[131].num_points(loader.scene_ids[i]) for i in order)
