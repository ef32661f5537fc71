"""Host side of d3net_amd.multiview: the float32 restatement (tests/multiview_restate.py) against the reference's own outputs
(tests/golden/multiview_golden.npz), the reference's frame order, and argument validation.  No GPU."""
import os

import numpy as np
import pytest

import multiview_restate as R
from d3net_amd import multiview as MV

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "multiview_golden.npz"))
CASES = [str(c) for c in G["cases"]]


def _g(case, key):
    v = G["%s/%s" % (case, key)]
    return v.astype(np.float32) / 4 if key.endswith("_x4") else v


def _pix(case):
    poses = _g(case, "poses")
    w2c = MV.world_to_camera(poses).numpy()
    return R.scene_pixels(_g(case, "points"), _g(case, "depths"), poses, w2c, **R.DEFAULTS)


@pytest.mark.parametrize("case", CASES)
def test_restatement_indices_match_reference(case):
    i3, i2 = R.index_lists(_pix(case))
    np.testing.assert_array_equal(i3, _g(case, "indices_3d"))
    np.testing.assert_array_equal(i2, _g(case, "indices_2d"))


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("maxpool", [True, False])
def test_restatement_fusion_matches_reference(case, maxpool):
    got = R.fuse(_pix(case), _g(case, "features_x4"), maxpool)
    want = _g(case, "maxpool_x4" if maxpool else "first_x4")
    assert got.tobytes() == want.tobytes()


def test_golden_exercises_the_rules():
    """the fixture covers what the fusion rules branch on: negatives, all-zero pixel rows at mapped pixels, unmapped frames,
    points seen in several frames, and a maxpool result that differs from the first-frame rule"""
    for case in CASES:
        f = _g(case, "features_x4")
        i3, i2 = _g(case, "indices_3d"), _g(case, "indices_2d")
        assert (f < 0).any()
        F = len(f)
        zero_hit = sum(int((f[k].reshape(128, -1)[:, i2[k, 1:1 + i3[k, 0]]] == 0).all(0).sum()) for k in range(F))
        assert zero_hit > 0
        assert i3[-1, 0] == 0 and not np.isfinite(_g(case, "poses")[-1]).any()
        seen = np.zeros(i3.shape[1] - 1, int)
        for k in range(F):
            seen[i3[k, 1:1 + i3[k, 0]]] += 1
        assert (seen >= 2).sum() > 50
        assert not np.array_equal(_g(case, "maxpool_x4"), _g(case, "first_x4"))


def test_reference_frame_order():
    names = ["20.jpg", "100.jpg", "3.jpg", "0.jpg", "1000.jpg", "21.jpg"]
    assert MV.reference_frame_order(names) == ["0", "100", "1000", "20", "21", "3"]
    assert MV.reference_frame_order(["b.png", "a.png"]) == ["a", "b"]
    assert MV.reference_frame_order([]) == []


def test_world_to_camera_is_cpu_float32_inverse():
    poses = _g(CASES[0], "poses")
    w = MV.world_to_camera(poses)
    assert w.dtype.is_floating_point and str(w.device) == "cpu" and tuple(w.shape) == poses.shape
    assert np.isnan(w[-1].numpy()).all()                       # the -inf pose
    np.testing.assert_allclose(w[0].numpy() @ poses[0], np.eye(4), atol=1e-5)


@pytest.mark.parametrize("bad", ["points", "depths", "poses", "features"])
def test_argument_shapes_are_checked_before_the_device(bad):
    h = MV.ProjectionHelper(R.INTRINSICS, 0.1, 4.0, [41, 32], 0.05)
    pts, dep, poses = np.zeros((10, 3), np.float32), np.zeros((2, 32, 41), np.float32), np.tile(np.eye(4, dtype=np.float32), (2, 1, 1))
    feats = np.zeros((2, 128, 32, 41), np.float32)
    if bad == "points":
        pts = np.zeros((10, 4), np.float32)
    elif bad == "depths":
        dep = np.zeros((2, 41, 32), np.float32)
    elif bad == "poses":
        poses = poses[:1]
    else:
        feats = np.zeros((2, 128, 41, 32), np.float32)
    with pytest.raises(ValueError):
        if bad == "features":
            h.project_scene(pts, dep, poses, feats)
        else:
            h.compute_projection_batch(pts, dep, poses)


def test_corner_points_follow_the_reference_order():
    cp = R.corner_points(R.INTRINSICS, 0.1, 4.0, (41, 32))
    assert cp.dtype == np.float32 and cp.shape == (8, 3)
    np.testing.assert_array_equal(cp[:4, 2], np.float32(0.1))
    np.testing.assert_array_equal(cp[4:, 2], np.float32(4.0))
    assert cp[0, 0] < 0 and cp[1, 0] > 0 and cp[2, 1] > 0 and cp[0, 1] < 0     # (0,0), (W-1,0), (W-1,H-1), (0,H-1)
