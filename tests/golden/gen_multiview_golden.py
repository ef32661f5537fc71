#!/usr/bin/env python3
"""Generates tests/golden/multiview_golden.npz by RUNNING THE REFERENCE's own ProjectionHelper (lib/utils/projection.py:
compute_projection and project) on the CPU, frame by frame, on synthetic rooms (tests/multiview_restate.py: points on box walls
and objects, inward-looking poses plus one looking out through a wall and one -inf pose, depth z-buffered from the points in
float64, ENet-like features with negatives and all-zero pixel rows).  The reference calls .cuda() unconditionally, so
torch.Tensor.cuda is registered as the identity first.  The per-scene fusion of project_multiview_features.py:170-200 lives
in that script's __main__ and cannot be imported; it is restated here from its description, in both modes.

Points whose float64 decision margin is small in some frame -- a frustum plane's `dot * 100` within 1e-4 (relative to
100 |p - corner| |normal|) of the rounding half, a projected u or v within 2e-3 of a half pixel, a depth within 1e-5 of
depth_min / depth_max, or |depth - z| within 1e-4 of the accuracy -- are dropped before the reference runs, so any float32
operation order gives the same mapping and the fixture is exact.  Features are sparse multiples of 0.25 and stored x4 as int8, as are
the fused outputs (which only copy or max those values).  No output reads a pixel that no kept point maps to, so those pixel
rows are zeroed before the fusion runs: the fixture then compresses to a few hundred kB.  Run where the reference is available."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import multiview_restate as R  # noqa: E402

REF = "/root/reference"
CASES = {"room_a": dict(seed=1, n=2400, F=12), "room_b": dict(seed=2, n=2000, F=9)}


def _import_reference():
    torch.Tensor.cuda = lambda self, *a, **k: self
    sys.path.insert(0, REF)
    from lib.utils.projection import ProjectionHelper
    return ProjectionHelper


def robust_points(points, depths, poses, cfg):
    """mask of the points whose every decision in every frame is far from a float32 rounding boundary (float64 margins)"""
    intr, (W, H) = cfg["intrinsic"], cfg["image_dims"]
    cp = R.corner_points(intr, cfg["depth_min"], cfg["depth_max"], cfg["image_dims"]).astype(np.float64)
    p = points.astype(np.float64)
    keep = np.ones(len(p), bool)
    for f in range(len(poses)):
        M = poses[f].astype(np.float64)
        if not np.isfinite(M).all():
            continue
        cc = cp @ M[:3, :3].T + M[:3, 3]
        A, B, Cc = [3, 2, 3, 0, 1, 6], [0, 1, 2, 3, 0, 5], [1, 5, 6, 7, 4, 4]
        inside = np.ones(len(p), bool)
        for k in range(6):
            n = np.cross(cc[A[k]] - cc[B[k]], cc[Cc[k]] - cc[B[k]])
            d = p - (cc[2] if k < 3 else cc[4])
            x = d @ n * 100
            scale = 100 * np.linalg.norm(d, axis=1) * np.linalg.norm(n)
            keep &= ~(np.abs(x + 0.5) < 1e-4 * scale + 1e-5)
            inside &= x < -0.5
        w2c = np.linalg.inv(M)
        cam = p @ w2c[:3, :3].T + w2c[:3, 3]
        with np.errstate(divide="ignore", invalid="ignore"):
            u = cam[:, 0] * intr[0][0] / cam[:, 2] + intr[0][2]
            v = cam[:, 1] * intr[1][1] / cam[:, 2] + intr[1][2]
        near_half = (np.abs(u - np.floor(u) - 0.5) < 2e-3) | (np.abs(v - np.floor(v) - 0.5) < 2e-3)
        keep &= ~(inside & near_half)
        ur, vr = np.rint(u), np.rint(v)
        on = inside & (ur >= 0) & (ur < W) & (vr >= 0) & (vr < H)
        pix = np.where(on, vr * W + ur, 0).astype(np.int64)
        dd = depths[f].reshape(-1)[pix].astype(np.float64)
        marg = np.minimum(np.minimum(np.abs(dd - cfg["depth_min"]), np.abs(dd - cfg["depth_max"])) / 1e-5,
                          np.abs(np.abs(dd - cam[:, 2]) - cfg["accuracy"]) / 1e-4)
        keep &= ~(on & (marg < 1))
    return keep


def fuse_reference(helper, feats, i3s, i2s, N, maxpool):
    """project_multiview_features.py:164-200 restated: frames without mappings dropped, then each valid frame in order"""
    rows = torch.zeros(N, 128)
    valid = [f for f in range(len(i3s)) if i3s[f] is not None]
    for j, f in enumerate(valid):
        proj = helper.project(torch.from_numpy(feats[f]), i3s[f], i2s[f], N).transpose(1, 0)
        proj_full = (proj != 0).any(1)
        row_empty = ~(rows != 0).any(1)
        if maxpool:
            fill, pool = row_empty & proj_full, ~row_empty & proj_full
            rows[fill] = proj[fill]
            rows[pool] = torch.max(rows[pool], proj[pool])
        elif j == 0:
            rows = proj.clone()
        else:
            rows[row_empty] = proj[row_empty]
    return rows.numpy()


def _q(x):
    q = np.asarray(x, np.float64) * 4
    assert np.array_equal(q, np.rint(q)) and np.abs(q).max() <= 127
    return q.astype(np.int8)


def main():
    ProjectionHelper = _import_reference()
    cfg = R.DEFAULTS
    helper = ProjectionHelper(cfg["intrinsic"], cfg["depth_min"], cfg["depth_max"], list(cfg["image_dims"]), cfg["accuracy"])
    out = {"cases": np.array(list(CASES))}
    for name, c in CASES.items():
        pts, depths, poses, feats = R.room_scene(c["seed"], c["n"], c["F"])
        keep = robust_points(pts, depths, poses, cfg)
        pts = pts[keep]
        N, F = len(pts), len(poses)
        i3s, i2s = [], []
        I3, I2 = np.zeros((F, N + 1), np.int64), np.zeros((F, N + 1), np.int64)
        for f in range(F):
            r = helper.compute_projection(torch.from_numpy(pts), torch.from_numpy(depths[f]), torch.from_numpy(poses[f]))
            i3s.append(None if r is None else r[0])
            i2s.append(None if r is None else r[1])
            if r is not None:
                I3[f], I2[f] = r[0].numpy(), r[1].numpy()
        for f in range(F):                                                   # pixels no point reads carry no information
            unused = np.ones(feats.shape[2] * feats.shape[3], bool)
            unused[I2[f, 1:1 + I2[f, 0]]] = False
            feats[f].reshape(128, -1)[:, unused] = 0
        w2c = torch.inverse(torch.from_numpy(poses)).numpy()
        pix = R.scene_pixels(pts, depths, poses, w2c, **cfg)
        r3, r2 = R.index_lists(pix)
        assert np.array_equal(r3, I3) and np.array_equal(r2, I2), name       # the restatement agrees on the robust points
        assert I3[-1, 0] == 0                                                # the -inf pose maps nothing
        fused = {m: fuse_reference(helper, feats, i3s, i2s, N, m) for m in (True, False)}
        print("%s: %d of %d points kept, %d frames, mapped per frame %s" % (name, N, c["n"], F, I3[:, 0].tolist()))
        out.update({"%s/points" % name: pts, "%s/depths" % name: depths, "%s/poses" % name: poses,
                    "%s/features_x4" % name: _q(feats), "%s/indices_3d" % name: I3.astype(np.int32),
                    "%s/indices_2d" % name: I2.astype(np.int32), "%s/maxpool_x4" % name: _q(fused[True]),
                    "%s/first_x4" % name: _q(fused[False])})
    np.savez_compressed(os.path.join(HERE, "multiview_golden.npz"), **out)


if __name__ == "__main__":
    main()
