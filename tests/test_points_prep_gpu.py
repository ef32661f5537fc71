"""scene_prep.prepare_points_store and SceneStore.extents (csrc/batch_prep.hip: d3_points_batch, d3_store_extents) against the
per-scene labelled path with is_augment=False, `collate_scenes_device([prepare_scene(store.scene(s), ...)])` -- which
tests/test_scene_prep*.py and tests/test_collate_device_gpu.py pin to the reference -- and against the numpy restatement of the
reference's label-free branch (tests/points_prep_restate.py): the seven keys equal bit for bit, over the shapes at which the
kernels change path (one point, around one block, around one tile, several tiles, 3 and 131 feature columns, aligned and unaligned
feature rows), the coordinate edges, and the host side (the store left untouched, no host synchronisation, refusals)."""
import os

import numpy as np
import pytest
import torch

import points_prep_restate as PR
from d3net_amd import _lib
from d3net_amd import dataset as D
from d3net_amd import scene_prep as SP
from d3net_amd.config import default_conf

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MSA = np.load(os.path.join(HERE, "golden", "lang_prep_golden.npz"))["mean_size_arr"]
KEYS = ("locs", "locs_scaled", "feats", "batch_offsets", "voxel_locs", "p2v_map", "v2p_map")
SIZES = (1, 255, 256, 257, 1023, 1024, 1025, 2500)
BATCHES = [("n2500",), ("n1", "n255", "n256"), ("n257", "n2500", "n1", "n255"), ("n1025", "n255", "n1025", "n1023")]


def _cfg():
    return default_conf(overrides={"model": {"no_captioning": True, "no_grounding": False}, "data": {"batch_size": 4}})


def _scene(n, width=3, seed=0, points=None):
    r = np.random.RandomState(seed)
    pts = ((r.rand(n, 3) - 0.3) * np.array([4.0, 3.0, 2.0])).astype(np.float32) if points is None else np.asarray(points, np.float32)
    return {"points": pts, "feats": r.randn(n, width).astype(np.float32), "sem_labels": r.randint(-1, 20, n).astype(np.int32),
            "instance_ids": r.randint(-1, 7, n).astype(np.int32)}


def _scenes(width):
    return {"n%d" % n: _scene(n, width, seed=n) for n in SIZES}


@pytest.fixture(scope="module")
def stores(dev):
    """per feature width: the scenes, their labelled store and their labels=False store"""
    out = {}
    for w in (3, 131):
        sc = _scenes(w)
        bare = {k: {"points": v["points"], "feats": v["feats"]} for k, v in sc.items()}
        out[w] = (sc, D.SceneStore.from_scenes(sc, device=dev), D.SceneStore.from_scenes(bare, device=dev, labels=False))
    return out


@pytest.fixture(scope="module")
def labelled_batches(dev, stores):
    """the yardstick, computed once per (width, batch) and left unchanged"""
    cfg, out = _cfg(), {}
    for w, (_, store, _) in stores.items():
        for ids in BATCHES:
            samples = [SP.prepare_scene(store.scene(s), cfg, MSA, rng=np.random.RandomState(0), is_augment=False, device=dev) for s in ids]
            full = SP.collate_scenes_device(samples, dev, cfg.data.mode)
            out[(w, ids)] = {k: full[k] for k in KEYS}
    return out


def _assert_equal(got, want):
    assert set(got) == set(KEYS)
    for k in KEYS:
        g, w = got[k], want[k]
        assert g.dtype == w.dtype and g.shape == w.shape, (k, g.dtype, w.dtype, g.shape, w.shape)
        assert torch.equal(g, w), k


def _assert_equals_restatement(got, scenes, ids, scale):
    want = PR.batch(scenes, ids, scale)
    for k, w in want.items():
        g = got[k].cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), k


@pytest.mark.parametrize("width", [3, 131])
def test_extents_equal_the_scaled_minimum(dev, stores, width):
    """bit for bit per scene, one point up to several tiles; the table is cached per scale"""
    _, labelled, bare = stores[width]
    for store in (labelled, bare):
        for scale in (50, 7):
            ext = store.extents(scale)
            assert ext is store.extents(scale) and ext.shape == (len(store), 3) and ext.dtype == torch.int64 and ext.device == store.points.device
            got = SP._decode(ext.cpu().numpy().view(np.uint64))
            pts = store.points.cpu().numpy()
            for i, sid in enumerate(store.scene_ids):
                a, b = int(store.offsets[i]), int(store.offsets[i + 1])
                want = PR.extents(pts[a:b], scale)
                assert want.dtype == np.float32 and np.array_equal(got[i].astype(np.float32).view(np.uint32), want.view(np.uint32)), (sid, scale)
                assert np.array_equal(got[i], want.astype(np.float64)), (sid, scale)
    assert [store.num_points(s) for s in store.scene_ids] == list(SIZES)


@pytest.mark.parametrize("labels", [True, False])
@pytest.mark.parametrize("width", [3, 131])
@pytest.mark.parametrize("ids", BATCHES)
def test_batches_equal_the_labelled_path(dev, stores, labelled_batches, ids, width, labels):
    scenes, labelled, bare = stores[width]
    store = labelled if labels else bare
    before = {k: getattr(store, k).clone() for k in D._FIELDS}
    cfg = _cfg()
    got = SP.prepare_points_store(store, list(ids), cfg, device=dev, mode=cfg.data.mode)
    _assert_equal(got, labelled_batches[(width, ids)])
    _assert_equals_restatement(got, scenes, ids, cfg.data.scale)
    assert got["feats"].shape[1] == width and got["batch_offsets"].numel() == len(ids) + 1
    for k, v in before.items():                              # the store was read, not written
        assert torch.equal(getattr(store, k), v), k


def test_batches_are_what_they_claim():
    assert (131 * 255) % 4 != 0 and len(set(BATCHES[3])) < len(BATCHES[3])


def _edge_scenes():
    r = np.random.RandomState(4)
    zeros = np.zeros((40, 3), np.float32)
    zeros[::3, 0] = -0.0
    zeros[5, 1] = -0.0
    assert np.signbit(zeros).any() and not zeros.any()
    big = (1e4 + r.rand(300, 3) * 3).astype(np.float32)
    assert (big.astype(np.float64) * 50 != (big * np.float32(50)).astype(np.float64)).any()      # x * 50 rounds in float32
    return {"negative": _scene(300, seed=1, points=-(r.rand(300, 3) * 5 + 0.01)),
            "negzero": _scene(40, seed=2, points=zeros),
            "same": _scene(260, seed=3, points=np.tile(np.array([[1.37, -2.2, 0.123]], np.float32), (260, 1))),
            "big": _scene(300, seed=4, points=big)}


@pytest.mark.parametrize("ids", [("negative",), ("negzero",), ("same",), ("big",), ("same", "big", "negzero", "negative")])
def test_coordinate_edges(dev, ids):
    scenes = _edge_scenes()
    cfg = _cfg()
    store = D.SceneStore.from_scenes(scenes, device=dev)
    samples = [SP.prepare_scene(store.scene(s), cfg, MSA, rng=np.random.RandomState(0), is_augment=False, device=dev) for s in ids]
    want = SP.collate_scenes_device(samples, dev, cfg.data.mode)
    got = SP.prepare_points_store(store, list(ids), cfg, device=dev, mode=cfg.data.mode)
    _assert_equal(got, {k: want[k] for k in KEYS})
    _assert_equals_restatement(got, scenes, ids, cfg.data.scale)
    ls = got["locs_scaled"].cpu().numpy()
    assert (ls[:, 1:] >= 0).all() and (ls[:, 0] == np.repeat(np.arange(len(ids)), [len(scenes[s]["points"]) for s in ids])).all()
    if "same" in ids:
        rows = ls[ls[:, 0] == ids.index("same")]
        assert len(rows) == 260 and not rows[:, 1:].any()
    if ids == ("negzero",):
        assert not ls.any()


def test_no_host_synchronisation(dev, stores):
    """one warmed call under torch's sync debug mode: nothing at the torch level may wait for the device (the voxelisation's count
    read-back is the library's own, as on every path)"""
    cfg, (_, _, store) = _cfg(), stores[131]
    ids = ["n257", "n2500", "n1", "n255"]
    for _ in range(2):                                      # warm: the extents table, workspace and pinned tables
        SP.prepare_points_store(store, ids, cfg, device=dev, mode=cfg.data.mode)
    torch.cuda.set_sync_debug_mode("error")
    try:
        assert torch.cuda.get_sync_debug_mode() == 2
        batch = SP.prepare_points_store(store, ids, cfg, device=dev, mode=cfg.data.mode)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert batch["locs"].shape[0] == sum(store.num_points(s) for s in ids)


def test_refusals(dev):
    L = _lib.lib()
    assert L.d3_points_batch_table_bytes(0) == 0 and L.d3_points_batch_table_bytes(513) == 0 and L.d3_points_batch_table_bytes(512) > 0
    assert L.d3_points_batch_ws_bytes(0) == 0 and L.d3_points_batch_ws_bytes(513) == 0
    assert L.d3_points_batch_ws_bytes(512) >= L.d3_points_batch_table_bytes(512)
    assert L.d3_store_extents_table_bytes(0) == 0 and L.d3_store_extents_ws_bytes(0) == 0 and L.d3_store_extents_table_bytes(1) > 0
    cfg = _cfg()
    sc = {"fine": _scene(10)}
    ok = D.SceneStore.from_scenes(sc, device=dev, labels=False)
    with pytest.raises(ValueError):
        SP.prepare_points_store(ok, [], cfg, device=dev)
    with pytest.raises(_lib.D3Error):
        SP.prepare_points_store(ok, ["fine"] * 513, cfg, device=dev)
    with pytest.raises(ValueError, match="labels=False"):
        ok.instance_index()
    assert set(ok.scene("fine")) == {"points", "feats"}
    pinned = D.SceneStore.from_scenes(sc, device="cpu", labels=False)
    with pytest.raises(ValueError, match="pinned"):
        pinned.extents(cfg.data.scale)
    with pytest.raises(ValueError, match="pinned"):
        SP.prepare_points_store(pinned, ["fine"], cfg, device=dev)
    arrays = {k: np.ascontiguousarray(v.reshape(10, -1) if k in ("points", "feats") else v) for k, v in sc["fine"].items()}
    hollow = D.SceneStore(["fine", "hollow_scene"], [0, 10, 10], arrays, dev)                           # a labelled store may hold one
    with pytest.raises(ValueError, match="hollow_scene"):
        hollow.extents(cfg.data.scale)
    with pytest.raises(ValueError, match="hollow_scene"):
        SP.prepare_points_store(hollow, ["fine"], cfg, device=dev)
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match="not on"):
            SP.prepare_points_store(ok, ["fine"], cfg, device=torch.device("cuda", 1))
    # the entry point's own checks, before anything is queued: an empty slot, a slot outside the store, a misaligned output
    import ctypes as C
    ext = ok.extents(cfg.data.scale)
    locs, ls, feats, boff = (torch.empty(s, dtype=t, device=dev) for s, t in (((10, 3), torch.float32), ((11, 4), torch.int64),
                                                                              ((10, 3), torch.float32), ((2,), torch.int32)))
    table = torch.empty(int(L.d3_points_batch_table_bytes(1)), dtype=torch.uint8).pin_memory()
    ws = torch.empty(int(L.d3_points_batch_ws_bytes(1)), dtype=torch.uint8, device=dev)

    def status(n, row0=0, srow=0, ls_ptr=None, locs_ptr=None):
        a = lambda v, t: np.array([v], t).ctypes.data_as(C.c_void_p)
        keep = (a(row0, np.int64), a(srow, np.int32), a(n, np.int32))
        return L.d3_points_batch(SP._ptr(ok.points), SP._ptr(ok.feats), 10, SP._ptr(ext), 1, *keep, 1, 3, 50.0,
                                 SP._ptr(locs) if locs_ptr is None else locs_ptr, C.c_void_p(ls.data_ptr() if ls_ptr is None else ls_ptr),
                                 SP._ptr(feats), SP._ptr(boff), C.c_void_p(table.data_ptr()), SP._ptr(ws), ws.numel(), SP._stream())
    assert status(0) == -2 and status(-1) == -2
    assert status(11) == -3 and status(5, row0=6) == -3 and status(5, srow=1) == -3 and status(5, row0=-1) == -3
    assert status(10, ls_ptr=ls.data_ptr() + 8) == -3 and status(10, locs_ptr=C.c_void_p(0)) == -3
    torch.cuda.synchronize()
    assert status(10) == 0
    torch.cuda.synchronize()
    assert np.array_equal(locs.cpu().numpy(), sc["fine"]["points"]) and boff.tolist() == [0, 10]
