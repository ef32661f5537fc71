#!/usr/bin/env python3
"""Generates tests/golden/enet_golden.npz by RUNNING THE REFERENCE's own network (model/enet.py create_enet(41), imported by file
path) on the CPU in eval mode, with the deterministic name-seeded weights of tests/enet_restate.py:golden_weights (checked first
to cover exactly the state dict's keys and shapes for elements 0-25; element 26, the classifier, gets weights too but is never run).

Stored:
  * small/e3, small/e8, small/e25: outputs of elements 3, 8 and 25 for the 2 frames golden_input(1, 2, 64, 80);
  * full/e25: element 25 for the frame golden_input(2, 1, 256, 328) (the reference's frame size);
  * tables/<W0>x<H0>/rows, cols: the source row / column of each of the 256 x 328 output pixels of the reference's
    _resize_crop_image (compute_multiview_features.py:53-60) for 1296x968, 640x480 and 1920x1440 frames, read back from Pillow by
    resizing images whose pixels encode their own coordinates; tables/<W0>x<H0>/width, left: the resize width and crop offset.
Outputs are stored rounded to 16 explicit mantissa bits (relative error <= 2^-17 = 7.6e-6 of the value, 13x inside the tests'
1e-4 bound) so that the compressed fixture stays under 1 MB.  Inputs are regenerated from their seeds.
Run where the reference is available: `python tests/golden/gen_enet_golden.py`."""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import enet_restate as R  # noqa: E402

REF = "/root/reference"
SIZES = [(1296, 968), (640, 480), (1920, 1440)]


def _reference_enet():
    spec = importlib.util.spec_from_file_location("ref_enet", os.path.join(REF, "model", "enet.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.create_enet(41)


def round16(a):
    """round float32 to 16 explicit mantissa bits (nearest, ties away): the low 7 bits become zero"""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + (1 << 6)) >> 7) << 7
    return u.astype(np.uint32).view(np.float32)


def run(net, x, keep):
    out, y = {}, torch.from_numpy(x)
    with torch.no_grad():
        for i in range(26):
            y = net[i](y)
            if i in keep:
                out[i] = y.numpy().copy()
    return out


def main():
    torch.manual_seed(0)
    net = _reference_enet().eval()
    ref_sd = {k: v for k, v in net.state_dict().items() if not k.startswith("26.") and not k.endswith("num_batches_tracked")}
    shapes = R.state_shapes()
    assert set(ref_sd) == set(shapes), (sorted(set(ref_sd) ^ set(shapes))[:10])
    assert all(tuple(ref_sd[k].shape) == shapes[k] for k in shapes)
    w = R.golden_weights()
    full_sd = net.state_dict()
    full_sd.update(w)
    net.load_state_dict(full_sd)

    blobs = {}
    small = run(net, R.golden_input(1, 2, 64, 80), (3, 8, 25))
    for k, v in small.items():
        blobs["small/e%d" % k] = round16(v)
    blobs["full/e25"] = round16(run(net, R.golden_input(2, 1, 256, 328), (25,))[25])
    # the restatement is the reference, layer by layer
    chk = R.forward(w, R.golden_input(1, 2, 64, 80))
    for k in (3, 8, 25):
        e = R.rel_err(chk[k].numpy(), small[k]).max()
        assert e < 1e-6, (k, e)
    for W0, H0 in SIZES:
        rows, cols = R.pil_source_tables(H0, W0)
        wdt = int(np.floor(256 * float(W0) / float(H0)))
        key = "tables/%dx%d/" % (W0, H0)
        blobs[key + "rows"], blobs[key + "cols"] = rows.astype(np.int16), cols.astype(np.int16)
        blobs[key + "width"], blobs[key + "left"] = np.int32(wdt), np.int32(int(round((wdt - 328) / 2.0)))
    path = os.path.join(HERE, "enet_golden.npz")
    np.savez_compressed(path, **blobs)
    print(path, os.path.getsize(path), "bytes;", {k: v.shape for k, v in blobs.items()})


if __name__ == "__main__":
    main()
