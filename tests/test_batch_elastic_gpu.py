"""scene_prep.prepare_batch_store_elastic (csrc/batch_elastic.hip) against the per-scene path it replaces in the augmented
detector-only mode, `collate_scenes_device([prepare_scene(store.scene(s), cfg, msa, rng, is_augment=True, noise="device") ...])`
(`_per_scene` of test_batch_prep_gpu.py): every key equal bit for bit (torch.equal, dtype, shape) -- without a crop, at the edge of
the noise-grid shape, with cropped slots in every position, with instances lost to the crop -- and the host side: the grid bound,
the refusals, the single read-back, the loader switch and `train --data --augment --fused-prep`."""
import json
import os

import numpy as np
import pytest
import torch

from d3net_amd import _lib
from d3net_amd import dataset as D
from d3net_amd import scene_prep as SP
from d3net_amd.config import default_conf

from test_batch_prep_gpu import MSA, SIZES, _assert_batches_equal, _edge_scenes, _per_scene, _random_ids, _scene
from test_batch_prep_loader_gpu import _raw_scenes, _write_dataset

pytestmark = pytest.mark.gpu
COL = {k: i for i, k in enumerate(SP.READBACK_COLUMNS)}


def _cfg(max_pt=250000, R=128, gt=True, transform=None, **data):
    data = dict({"max_num_instance": R, "requires_gt_mask": gt, "batch_size": 4, "max_num_point": max_pt}, **data)
    if transform is not None:
        data["transform"] = transform
    return default_conf(overrides={"model": {"no_captioning": True, "no_grounding": True}, "data": data})


class _CropFromSeed:
    """The yardstick's generator where a slot is cropped: `randn` / `randint` / `rand()` come from a RandomState as they would
    from a plain one; `rand(3)` -- the crop loop's draw -- comes from RandomState(v), v the value of the last `randint` call whose
    upper bound was 2**31 - 1 (the scene's noise seed), which is where prepare_batch_store_elastic takes its crop table from."""

    def __init__(self, seed):
        self.r, self.crop = np.random.RandomState(seed), None

    def randn(self, *a):
        return self.r.randn(*a)

    def randint(self, lo, hi=None, *a, **k):
        v = self.r.randint(lo, hi, *a, **k)
        if hi == 2 ** 31 - 1:
            self.crop = np.random.RandomState(int(v))
        return v

    def rand(self, *a):
        return self.crop.rand(3) if a == (3,) else self.r.rand(*a)


def _check(store, ids, cfg, dev, seed=11, cropped=False):
    """-> (batch, read-back rows); the bound guard holds for every batch that passes through here"""
    r0 = _CropFromSeed(seed) if cropped else np.random.RandomState(seed)
    r1 = np.random.RandomState(seed)
    want = _per_scene(store, ids, cfg, r0, True, dev)
    info = {}
    got = SP.prepare_batch_store_elastic(store, ids, cfg, MSA, rng=r1, device=dev, mode=cfg.data.mode, info=info)
    _assert_batches_equal(got, want)
    s0, s1 = (r0.r if cropped else r0).get_state(), r1.get_state()
    assert s0[0] == s1[0] and np.array_equal(s0[1], s1[1]) and s0[2:] == s1[2:]      # the stand-in's own stream never serves a crop
    rb, bounds = info["readback"], info["bounds"]
    assert rb.shape == (len(ids), len(COL)) and (rb[:, 3:9] <= bounds).all() and (rb[:, 3:9] >= 3).all()
    kept = np.diff(want["batch_offsets"].cpu().numpy())
    assert (kept > 0).all() and np.array_equal(kept, rb[:, COL["kept"]])               # every slot keeps a point (the zero-point slot is out of scope)
    assert np.array_equal(np.diff(want["instance_offsets"].cpu().numpy()), rb[:, COL["K"]])
    return got, rb


@pytest.fixture(scope="module")
def stores(dev):
    return {w: D.SceneStore.from_scenes({"n%d" % n: _scene(n, _random_ids(n, 7, n), w, seed=n) for n in SIZES}, device=dev) for w in (3, 131)}


@pytest.fixture(scope="module")
def edge_store(dev):
    return D.SceneStore.from_scenes(_edge_scenes(), device=dev)


def _long_scene(n=3000, seed=21):
    """12 m long in x (600 scaled units > 512), 3 m x 2 m across; instance 0 lives in the first 0.5 m, instance 1 in the last:
    no crop window narrower than 11 m holds both"""
    r = np.random.RandomState(seed)
    pts = (r.rand(n, 3) * np.array([12.0, 3.0, 2.0])).astype(np.float32)
    pts[0, 0], pts[1, 0] = 0.0, 12.0
    ids = r.randint(-1, 7, n)
    ids = np.where(ids <= 1, 2, ids)
    ids = np.where(pts[:, 0] < 0.5, 0, np.where(pts[:, 0] > 11.5, 1, ids))
    return {"points": pts, "feats": r.randn(n, 3).astype(np.float32), "sem_labels": r.randint(-1, 20, n).astype(np.int32),
            "instance_ids": ids.astype(np.int32)}


@pytest.fixture(scope="module")
def long_store(dev):
    scenes = {"long": _long_scene(), "n257": _scene(257, _random_ids(257, 7, 257), 3, seed=257), "gaps": _edge_scenes()["gaps"]}
    return D.SceneStore.from_scenes(scenes, device=dev)


# ---------------------------------------------------------------------------------------------------- no crop
@pytest.mark.parametrize("gt", [True, False])
@pytest.mark.parametrize("width", [3, 131])
@pytest.mark.parametrize("ids", [("n2500",), ("n1", "n255", "n256"), ("n257", "n2500", "n1", "n255")])
def test_uncropped_batches_equal_outright(dev, stores, ids, width, gt):
    store = stores[width]
    before = {k: getattr(store, k).clone() for k in D._FIELDS}
    got, rb = _check(store, list(ids), _cfg(gt=gt), dev)
    assert ("gt_proposals_idx" in got) == gt and got["feats"].shape[1] == width
    assert (rb[:, COL["crop_iters"]] == 0).all() and np.array_equal(rb[:, COL["kept"]], [store.num_points(s) for s in ids])
    for k, v in before.items():                              # the store was read, not written
        assert torch.equal(getattr(store, k), v), k


@pytest.mark.parametrize("ids,R", [(("allneg", "gaps", "six"), 4), (("gaps", "six", "allneg"), 128), (("nounl_over", "gaps"), 4),
                                   (("six", "nounl_over", "six"), 4)])
def test_relabel_and_box_rule_without_a_crop(dev, edge_store, ids, R):
    """`_croppedInstanceIds` runs whether or not a slot was cropped: ids with gaps move"""
    got, rb = _check(edge_store, list(ids), _cfg(R=R), dev)
    if "gaps" in ids:
        assert rb[ids.index("gaps"), COL["K"]] == 3           # ids {0, 2, 5} -> {0, 1, 2}
    if "nounl_over" in ids:
        assert int(got["gt_bbox_label"][ids.index("nounl_over")].sum()) == min(R, 5)


# ---------------------------------------------------------------------------------------------------- the grid-shape edge
@pytest.mark.parametrize("top", [59.99, 60.0, 60.01])
def test_grid_shape_edge(dev, top):
    """M = I; the largest |x| * scale sits just below, at and just above a multiple of the first elastic's granularity"""
    cfg = _cfg(transform={"jitter": False, "flip": False, "rot": False})
    scale = cfg.data.scale
    gran = SP.elastic_params(scale)[0][0]
    r = np.random.RandomState(3)
    pts = ((r.rand(300, 3) - 0.5) * np.array([2.0, 1.6, 0.8])).astype(np.float32)
    pts[0, 0] = -np.float32(top / scale) if top == 60.0 else np.float32(top / scale)
    sc = {"points": pts, "feats": r.randn(300, 3).astype(np.float32), "sem_labels": r.randint(-1, 20, 300).astype(np.int32),
          "instance_ids": _random_ids(300, 5, 1).astype(np.int32)}
    store = D.SceneStore.from_scenes({"edge": sc}, device=dev)
    _, rb = _check(store, ["edge"], cfg, dev)
    s = np.matmul(pts, np.eye(3)) * scale                    # sp_transform_kernel's float64 path with M = I is exact
    want = SP.grid_shape(np.abs(s).max(0), gran)
    assert np.array_equal(rb[0, 3:6], want)
    assert want[0] == int(np.float64(np.abs(pts[0, 0])) * scale) // gran + 3 and want[0] in (12, 13)


def test_grid_shape_edge_inputs_straddle_the_step():
    gran, scale = SP.elastic_params(50)[0][0], 50
    shapes = [int(np.float64(np.float32(t / scale)) * scale) // gran + 3 for t in (59.99, 60.0, 60.01)]
    assert shapes[0] == 12 and shapes[2] == 13 and shapes[1] in (12, 13)


# ---------------------------------------------------------------------------------------------------- crop
@pytest.mark.parametrize("max_pt", [2400, 1000])
@pytest.mark.parametrize("ids", [("n2500",), ("n2500", "n257", "n255"), ("n257", "n2500", "n255"), ("n1", "n256", "n2500"), ("n2500", "n2500")])
def test_cropped_slots_in_every_position(dev, stores, ids, max_pt):
    _, rb = _check(stores[3], list(ids), _cfg(max_pt=max_pt), dev, cropped=True)
    for i, s in enumerate(ids):
        if s == "n2500":
            assert 0 < rb[i, COL["kept"]] < 2500 and rb[i, COL["crop_iters"]] > 1
        else:
            assert rb[i, COL["crop_iters"]] == 0
    if ids == ("n2500", "n2500"):                           # one scene in two slots, two draws
        assert not np.array_equal(rb[0], rb[1])


def test_first_iteration_already_crops(dev, long_store):
    """600 scaled units along x against a first range of 512: one iteration drops points even though max_num_point is generous"""
    cfg = _cfg(max_pt=2999, transform={"jitter": False, "flip": True, "rot": False})
    _, rb = _check(long_store, ["long", "n257"], cfg, dev, cropped=True)
    assert rb[0, COL["crop_iters"]] >= 1 and 0 < rb[0, COL["kept"]] < 3000 and rb[1, COL["crop_iters"]] == 0


@pytest.mark.parametrize("ids", [("long",), ("gaps", "long", "n257"), ("long", "long")])
def test_instances_lost_to_the_crop(dev, long_store, ids):
    """the two end instances cannot both survive a crop to 500 points, so K falls below the scene's 7 instances and the ids move"""
    # no rotation: the cloud then fills its bounding box, so no crop window inside it is empty
    got, rb = _check(long_store, list(ids), _cfg(max_pt=500, transform={"jitter": True, "flip": True, "rot": False}), dev, cropped=True)
    scene_ids = _long_scene()["instance_ids"]
    assert len(np.unique(scene_ids[scene_ids >= 0])) == 7
    for i, s in enumerate(ids):
        if s == "long":
            assert 0 < rb[i, COL["K"]] < 7 and 0 < rb[i, COL["kept"]] <= 500 and rb[i, COL["crop_iters"]] > 1
    a, b = (int(v) for v in got["batch_offsets"][:2])
    first = got["instance_ids"][a:b]
    assert sorted(first[first >= 0].unique().tolist()) == list(range(int(rb[0, COL["K"]])))


# ---------------------------------------------------------------------------------------------------- guards
def test_refusals(dev, stores):
    L = _lib.lib()
    assert L.d3_batch_elastic_table_bytes(0, 17) == 0 and L.d3_batch_elastic_table_bytes(513, 17) == 0
    assert L.d3_batch_elastic_table_bytes(512, 17) > 0 and L.d3_batch_elastic_table_bytes(4, 0) == 0
    store, det = stores[3], _cfg()
    before = {k: getattr(store, k).clone() for k in D._FIELDS}
    rng = lambda: np.random.RandomState(0)
    listener = default_conf(overrides={"model": {"no_captioning": True, "no_grounding": False}})
    with pytest.raises(ValueError):                          # no elastic distortion there: prepare_batch_store's
        SP.prepare_batch_store_elastic(store, ["n255"], listener, MSA, rng=rng(), device=dev)
    pinned = D.SceneStore.from_scenes({"fine": _scene(10, np.zeros(10))}, device="cpu")
    with pytest.raises(ValueError):
        SP.prepare_batch_store_elastic(pinned, ["fine"], det, MSA, rng=rng(), device=dev)
    with pytest.raises(ValueError):
        SP.prepare_batch_store_elastic(store, [], det, MSA, rng=rng(), device=dev)
    with pytest.raises(_lib.D3Error):
        SP.prepare_batch_store_elastic(store, ["n1"] * 513, det, MSA, rng=rng(), device=dev)
    far = _scene(20, np.zeros(20))
    far["points"][3, 1] = 300.0                              # 15000 scaled units: a noise grid of 2500 cells along y
    huge = D.SceneStore.from_scenes({"far": far}, device=dev)
    with pytest.raises(_lib.D3Error):
        SP.prepare_batch_store_elastic(huge, ["far"], det, MSA, rng=rng(), device=dev)
    loader = D.PipelineLoader(det, store, None, "train", "detector", seed=3, mean_size_arr=MSA, device=dev, fused=True, fused_elastic=True,
                              is_augment=True, noise="host")
    assert not loader.fused_elastic_active() and not loader.fused_active()
    for k, v in before.items():
        assert torch.equal(getattr(store, k), v), k
    with pytest.raises(ValueError):                          # unchanged: the unaugmented entry still refuses this path
        SP.prepare_batch_store(store, ["n255"], det, MSA, rng=rng(), is_augment=True, device=dev)
    assert not SP.fused_applicable(det, True, store) and SP.elastic_applicable(det, True, store)


def test_queueing_half_never_waits(dev, stores):
    """everything up to the table read, once warmed, under torch's sync debug mode"""
    store, cfg = stores[131], _cfg(max_pt=2400)
    ids = ["n2500", "n257", "n1", "n255"]
    ms = torch.from_numpy(np.ascontiguousarray(MSA, dtype=np.float64)).to(dev)
    rng = np.random.RandomState(4)
    for _ in range(2):                                      # warm: the index, the |xyz| table, workspace and tables
        SP.prepare_batch_store_elastic(store, ids, cfg, ms, rng=rng, device=dev)
    torch.cuda.set_sync_debug_mode("error")
    try:
        pending = SP.elastic_batch_queue(store, ids, cfg, ms, rng=rng, device=dev)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    info = {}
    batch = SP.elastic_batch_finish(pending, cfg.data.mode, info)
    assert batch["locs"].shape[0] == int(info["readback"][:, COL["kept"]].sum()) < sum(store.num_points(s) for s in ids)


def test_two_batches_in_flight_keep_their_own_read_back(dev, stores):
    """Queue two batches, then finish them in order: each equals its solo run, key by key and in its read-back rows.  The first
    batch has a cropped slot and the second none, so their read-back tables differ.  With ONE host image of the read-back table
    per (device, thread, stream), as before the pinned ring, this test fails: the second batch's copy lands in the image the
    first batch reads, so the first is checked against the second's grid shapes (here a RuntimeError from the bound check) or
    cut to the second's `kept / K / Lp` (a wrong length, not an access out of bounds: the outputs are allocated at the scenes'
    full sizes)."""
    store, cfg = stores[3], _cfg(max_pt=1000)
    r = np.random.RandomState(8)
    jobs = [(list(ids), [(SP.augment_matrix(r, cfg.data.transform), int(r.randint(0, 2 ** 31 - 1))) for _ in ids])
            for ids in (("n2500", "n257"), ("n255", "n256"))]
    want, infos = [], []
    for ids, draws in jobs:
        infos.append({})
        want.append(SP.prepare_batch_store_elastic(store, ids, cfg, MSA, device=dev, mode=cfg.data.mode, draws=draws, info=infos[-1]))
    rb0, rb1 = infos[0]["readback"], infos[1]["readback"]
    assert rb0[0, COL["crop_iters"]] > 0 and 0 < rb0[0, COL["kept"]] < 2500 and (rb1[:, COL["crop_iters"]] == 0).all()
    assert not np.array_equal(rb0[:, :3], rb1[:, :3])        # the counts `elastic_batch_finish` cuts by differ
    pending = [SP.elastic_batch_queue(store, ids, cfg, MSA, device=dev, draws=draws) for ids, draws in jobs]
    torch.cuda.synchronize()                                 # both read-back copies have landed before the first batch is finished
    for p, w, solo in zip(pending, want, infos):
        info = {}
        _assert_batches_equal(SP.elastic_batch_finish(p, cfg.data.mode, info), w)
        assert np.array_equal(info["readback"], solo["readback"]) and np.array_equal(info["bounds"], solo["bounds"])


# ---------------------------------------------------------------------------------------------------- loader and command
@pytest.mark.parametrize("rank", [0, 1])
def test_loader_passes(dev, rank):
    store = D.SceneStore.from_scenes(_raw_scenes(5), device=dev)
    cfg = _cfg(batch_size=2)
    mk = lambda **kw: D.PipelineLoader(cfg, store, None, "train", "detector", rank=rank, world=2, seed=5, mean_size_arr=MSA, device=dev,
                                       is_augment=True, **kw)
    fused, plain = mk(fused=True, fused_elastic=True), mk()
    assert fused.fused_elastic_active() and not fused.fused_active() and not plain.fused_active() and not plain.fused_elastic_active()
    assert not mk(fused=True).fused_elastic_active() and not mk(fused_elastic=True).fused_elastic_active()
    n = 0
    for _ in range(2):
        got, want = list(fused), list(plain)
        assert len(got) == len(want) == len(plain)
        for g, w in zip(got, want):
            _assert_batches_equal(g, w)
            n += 1
    assert n == 4


def test_train_data_augment_fused_prep_end_to_end(dev, tmp_path, capsys):
    from d3net_amd import train
    data = _write_dataset(str(tmp_path))
    meta = os.path.join(data, "scannet", "meta_data")
    for split, seeds in (("train", (3, 4, 5)), ("val", (6, 7))):
        with open(os.path.join(meta, "scannetv2_%s.txt" % split), "w") as f:
            f.write("".join("scene%04d_00\n" % s for s in seeds))
    root = str(tmp_path / "run")
    over = {"DATA_PATH": data, "data": {"batch_size": 2}, "train": {"log_every_n_steps": 1},
            "model": {"use_multiview": False, "use_color": True, "pretrained_detector": None}}
    tr = train.main(["-c", "pointgroup.yaml", "--data", "--augment", "--fused-prep", "--teacher", "--epochs", "1", "--root", root], overrides=over)
    assert tr.global_step == 2
    assert "fused batch preparation: in use by 2 of 2 loaders (1 on the elastic / crop path)" in capsys.readouterr().out
    with open(os.path.join(root, "logs", "metrics.jsonl")) as f:
        records = [json.loads(line) for line in f]
    epochs = [r for r in records if r["kind"] == "epoch"]
    assert len(epochs) == 1 and epochs[0]["global_step"] == 2 and np.isfinite(epochs[0]["train/total_loss"])     # mode 0 logs train/<loss name>
