"""Host side of d3net_amd.scene_prep against tests/golden/scene_prep_golden.npz (the reference's own functions): the scalar
draws and their order, the crop loop and the relabel map.  No GPU."""
import os
import types

import numpy as np
import pytest

from d3net_amd import scene_prep as SP

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scene_prep_golden.npz"))
CASES = [str(c) for c in G["cases"]]


def _g(case, key):
    return G["%s/%s" % (case, key)]


def _tcfg():
    return types.SimpleNamespace(jitter=True, flip=True, rot=True)


@pytest.mark.parametrize("case", CASES)
def test_scalar_draw_sequence_matches_reference(case):
    """augment matrix, noise grids (host mode), crop draws, in the reference's order: the stream position after the scene and
    the crop mask agree with the golden"""
    max_num_point, full_scale, _, captioning, aug = (int(v) for v in _g(case, "cfg"))
    rng = np.random.RandomState(int(_g(case, "seed")))
    m = SP.augment_matrix(rng, _tcfg()) if aug else np.eye(3)
    np.testing.assert_array_equal(m, _g(case, "M"))
    bbs = _g(case, "bb")
    for bb in bbs:
        SP.host_noise(rng, bb)
    elastic = aug and not captioning
    assert len(bbs) == (2 if elastic else 0)
    valid = np.ones(len(_g(case, "precrop")), bool)
    if elastic:
        pc = _g(case, "precrop")
        kept = {}

        def count(offset, rng_):
            p = pc + offset
            v = (p.min(1) >= 0) * ((p < rng_).sum(1) == 3)
            kept["v"] = v
            return int(v.sum())
        off, n = SP.crop_loop(count, len(pc), pc.max(0) - pc.min(0), max_num_point, full_scale, rng)
        if off is not None:
            valid = kept["v"]
        assert n == int(valid.sum())
        assert (off is not None) == (int(_g(case, "crop_iters")) > 0)
    np.testing.assert_array_equal(valid, _g(case, "valid"))
    assert rng.rand() == float(_g(case, "next_draw"))


def test_device_noise_takes_one_draw():
    """noise="device" replaces the six grids by one randint draw: the draws before it are the reference's"""
    a, b = np.random.RandomState(5), np.random.RandomState(5)
    SP.augment_matrix(a, _tcfg())
    b.randn(3, 3); b.randint(0, 2); b.rand()
    assert a.randint(0, 2 ** 31 - 1) == b.randint(0, 2 ** 31 - 1)


@pytest.mark.parametrize("case", [c for c in CASES if int(_g(c, "crop_iters")) > 0])
def test_relabel_map_matches_reference(case):
    ids = _g(case, "in_instance_ids")[_g(case, "valid")]
    V = int(_g(case, "in_instance_ids").max()) + 1
    present = np.zeros(V, bool)
    present[ids[ids >= 0]] = True
    val_of = SP.relabel_table(present)
    out = np.where(ids >= 0, val_of[np.maximum(ids, 0)], ids)
    np.testing.assert_array_equal(out, _g(case, "instance_ids"))


def test_relabel_map_edge_cases():
    """the reference's loop: an absent j takes the CURRENT max id, repeatedly"""
    np.testing.assert_array_equal(SP.relabel_table([False, False, True, False, True]), [0, 1, 1, 3, 0])
    np.testing.assert_array_equal(SP.relabel_table([True, True, True]), [0, 1, 2])
    np.testing.assert_array_equal(SP.relabel_table([False] * 3), [0, 1, 2])


def test_grid_shape_and_axes():
    bb = SP.grid_shape([300.7, 12.0, 0.2], 6)
    np.testing.assert_array_equal(bb, [53, 5, 3])
    ax = SP.grid_axes(bb, 6)
    assert ax[1][0] == -24 and ax[1][-1] == 24 and len(ax[1]) == 5
