"""scene_prep.collate_scenes_device (csrc/collate.hip, ONE launch) against scene_prep.collate_scenes (the torch stacking it
replaces) on identical prepare_scene outputs: the same keys, dtypes, shapes and bits.  Scenes of 1 / 255 / 256 / 257 points put a
scene boundary on, before and after a block boundary and make every later scene's output offset odd (the word-wise path beside
the 16-byte one); a 2500-point scene gives every job kind more than one tile."""
import os
import types

import numpy as np
import pytest
import torch

from d3net_amd import scene_prep as SP

HERE = os.path.dirname(os.path.abspath(__file__))
MSA = np.load(os.path.join(HERE, "golden", "lang_prep_golden.npz"))["mean_size_arr"]


def _cfg(gt_mask, R=128):
    ns = types.SimpleNamespace
    return ns(data=ns(scale=50, full_scale=[128, 512], max_num_point=250000, max_num_instance=R, requires_gt_mask=gt_mask,
                      requires_bbox=True, transform=ns(jitter=True, flip=True, rot=True)),
              model=ns(no_detection=False, no_captioning=False, no_grounding=True))


def _scene(n, C, seed, instances=True):
    r = np.random.RandomState(seed)
    ids = (r.permutation(n) % min(3, n)) if instances else np.full(n, -1)
    if instances and n > 4:
        ids[r.randint(0, n, max(n // 10, 1))] = -1                                      # some unlabelled points too
    return {"points": (r.rand(n, 3) * 4).astype(np.float32), "feats": r.randn(n, C).astype(np.float32),
            "sem_labels": r.randint(-1, 20, n).astype(np.int64), "instance_ids": ids.astype(np.int64)}


def _samples(dev, spec, C, gt_mask, R=128, is_augment=False):
    cfg = _cfg(gt_mask, R)
    rng = np.random.RandomState(11)
    return [SP.prepare_scene(_scene(n, C, 100 + k, inst), cfg, MSA, rng=rng, is_augment=is_augment, noise="device", device=dev)
            for k, (n, inst) in enumerate(spec)]


def _assert_same(dev, samples):
    want = SP.collate_scenes(samples, dev)
    got = SP.collate_scenes_device(samples, dev)
    torch.cuda.synchronize()
    assert set(got) == set(want)
    for k, w in want.items():
        g = got[k]
        assert g.dtype == w.dtype and g.shape == w.shape and g.device == w.device, (k, g.dtype, w.dtype, g.shape, w.shape)
        assert torch.equal(g, w), k
    return got


BOUNDARY = [(1, True), (255, True), (256, True), (257, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("gt_mask", [True, False])
@pytest.mark.parametrize("C", [3, 131])
@pytest.mark.parametrize("spec", [[(257, True)], [(300, True), (2500, True), (7, True)], BOUNDARY], ids=["B1", "B3", "boundary"])
def test_matches_collate_scenes(dev, spec, C, gt_mask):
    got = _assert_same(dev, _samples(dev, spec, C, gt_mask))
    assert got["batch_offsets"].tolist() == np.cumsum([0] + [n for n, _ in spec]).tolist()
    assert ("gt_proposals_idx" in got) == gt_mask and got["locs_scaled"][:, 0].unique().numel() == len(spec)
    assert got["gt_bbox"].shape == (len(spec), 128, 8, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("gt_mask", [True, False])
@pytest.mark.parametrize("empty", [0, 1, 2], ids=["first", "middle", "last"])
def test_a_scene_without_instances(dev, empty, gt_mask):
    spec = [(130, k != empty) for k in range(3)]
    samples = _samples(dev, spec, 3, gt_mask)
    if gt_mask and empty == 1:
        # the torch stacking cannot do this one: the instance-less scene leaves an EMPTY offset list behind, whose last element the
        # next scene asks for (`gt_off[-1][-1]`, as the reference's sparse_collate_fn does).  The kernel shifts by the running
        # number of proposal entries instead; every other key still has its yardstick
        with pytest.raises(IndexError):
            SP.collate_scenes(samples, dev)
        plain = [{k: v for k, v in s.items() if not k.startswith("gt_proposals")} for s in samples]
        got, want = SP.collate_scenes_device(samples, dev), SP.collate_scenes(plain, dev)
        for k, w in want.items():
            assert got[k].dtype == w.dtype and torch.equal(got[k], w), k
        a, c = samples[0], samples[2]
        la = a["gt_proposals_idx"].shape[0]
        assert torch.equal(got["gt_proposals_offset"], torch.cat([a["gt_proposals_offset"], c["gt_proposals_offset"][1:] + la]))
        shift = torch.tensor([a["num_instance"], 260], dtype=torch.int32, device=dev)
        assert torch.equal(got["gt_proposals_idx"], torch.cat([a["gt_proposals_idx"], c["gt_proposals_idx"] + shift]))
    else:
        got = _assert_same(dev, samples)
    off = got["instance_offsets"].tolist()
    assert off[empty + 1] == off[empty] and off[-1] == got["instance_num_point"].numel() > 0
    assert (got["instance_ids"][130 * empty:130 * (empty + 1)] == -1).all()
    if gt_mask:
        assert got["gt_proposals_offset"].numel() == off[-1] + 1


@pytest.mark.gpu
def test_augmented_samples_and_a_configured_row_count(dev):
    """the detector's augmented path (elastic, crop, relabelling) and data.max_num_instance = 70 rows of box labels"""
    cfg = _cfg(True, 70)
    cfg.model.no_captioning = True
    rng = np.random.RandomState(3)
    samples = [SP.prepare_scene(_scene(n, 6, 50 + n), cfg, MSA, rng=rng, is_augment=True, noise="device", device=dev) for n in (900, 333)]
    got = _assert_same(dev, samples)
    assert got["center_label"].shape == (2, 70, 3) and got["sem_cls_label"].shape == (2, 70)


@pytest.mark.gpu
def test_refusals(dev):
    a, b = _samples(dev, [(9, True)], 3, True)[0], _samples(dev, [(9, True)], 3, False)[0]
    with pytest.raises(ValueError, match="some samples only"):
        SP.collate_scenes_device([a, b], dev)
    with pytest.raises(ValueError, match="no samples"):
        SP.collate_scenes_device([], dev)
    bad = dict(b, sem_labels=b["sem_labels"].long())
    with pytest.raises(ValueError, match="sem_labels"):
        SP.collate_scenes_device([bad], dev)


def test_table_size_is_bounded(built_lib):
    """a host entry point: 512 scenes at most, since the tile-prefix table of a launch lives in LDS"""
    from d3net_amd import _lib
    l = _lib.lib()
    assert l.d3_collate_table_bytes(0) == 0 and l.d3_collate_table_bytes(513) == 0
    assert 0 < l.d3_collate_table_bytes(1) < l.d3_collate_table_bytes(512) < (1 << 20)
