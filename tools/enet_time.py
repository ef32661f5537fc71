#!/usr/bin/env python3
"""ENet frame-feature throughput on one GPU: frames per second at batch 256 from 1296x968 uint8 frames already on the device.

  (a) d3net_amd.enet (csrc/enet.hip): preprocessing + 67 convolution launches;
  (b) the same folded network through torch.nn.functional.conv2d (MIOpen, fp32 NCHW) + eager PReLU / max pool / add, fed the
      same preprocessed input: the in-tree baseline;
  (c) the host decode rate of enet.load_color_frames (Pillow JPEG decode into pinned memory, 16 threads) on synthetic 1296x968
      JPEGs written to a temporary directory.

(a) and (b) are timed with HIP events after a warm-up, median of the repeats.  Also printed: FLOPs and a lower bound on the bytes
moved per frame, from the layer shapes, for reading a kernel trace against the peak rates.  Weights are the deterministic test
weights (tests/enet_restate.py); the speed does not depend on them.
  python tools/enet_time.py [--frames 256] [--reps 10] [--warmup 3] [--jpegs 256]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch
import torch.nn.functional as Fn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from d3net_amd import enet as E  # noqa: E402
import enet_restate as R  # noqa: E402


def shape_costs(H=256, W=328):
    """(FLOPs, bytes) per frame: 2 MACs per multiply-add; bytes = every layer's input, side input and output read / written once"""
    t = E.layer_table().astype(np.int64).tolist()
    flops = 2 * (H // 2) * (W // 2) * 13 * 27 + 3 * H * W * 4            # initial conv + the input read of the pool
    byts = 4 * (3 * H * W + (H // 2) * (W // 2) * 16)
    h, w = H // 2, W // 2
    for l in range(1, 67, 3):
        ra, rb, rc = t[l], t[l + 1], t[l + 2]
        ho, wo = (h // 2, w // 2) if ra[4] == 2 else (h, w)
        for r in (ra, rb, rc):
            flops += 2 * ho * wo * r[1] * r[0] * r[2] * r[3]
        byts += 4 * (h * w * ra[0] + ho * wo * ra[1])                        # conv a
        byts += 4 * (2 * ho * wo * rb[0])                                     # conv b
        byts += 4 * (ho * wo * rc[0] + h * w * ra[0] + ho * wo * rc[1])       # conv c + side
        h, w = ho, wo
    return flops, byts


def torch_baseline(layers, dev):
    T = lambda a: torch.from_numpy(np.asarray(a, np.float32)).to(dev)  # noqa: E731
    W0, b0, ps, pt, sl = layers[0]
    init = (T(W0), T(b0), T(ps)[None, :, None, None], T(pt)[None, :, None, None], T(sl))
    convs = [(T(W), T(b), T(s)) for W, b, s in layers[1:]]

    def run(x):
        c = Fn.conv2d(x, init[0], init[1], stride=2, padding=1)
        y = Fn.prelu(torch.cat([c, Fn.max_pool2d(x, 2, 2) * init[2] + init[3]], 1), init[4])
        for i, (b, kind, cin, cout, inner, d, p) in enumerate(E.BLOCKS):
            (Wa, ba, sa), (Wb, bb, sb), (Wc, bc, sc) = convs[3 * i:3 * i + 3]
            t = Fn.prelu(Fn.conv2d(y, Wa, ba, stride=2 if kind == "down" else 1), sa)
            t = Fn.prelu(Fn.conv2d(t, Wb, bb, padding=2 if kind == "asym" else d, dilation=1 if kind == "asym" else d), sb)
            t = Fn.conv2d(t, Wc, bc)
            if kind == "down":
                s = Fn.max_pool2d(y, 2, 2)
                s = torch.cat([s, s.new_zeros((s.shape[0], cout - cin, s.shape[2], s.shape[3]))], 1)
            else:
                s = y
            y = Fn.prelu(t + s, sc)
        return y
    return run


def time_gpu(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), ts


def decode_rate(n, threads=16):
    from PIL import Image
    fr = R.synthetic_frames(0, 8, 968, 1296)
    with tempfile.TemporaryDirectory() as d:
        paths = []
        for i in range(n):
            p = os.path.join(d, "%d.jpg" % i)
            Image.fromarray(fr[i % 8]).save(p, quality=90)
            paths.append(p)
        E.load_color_frames(paths[:16], threads)
        t = time.perf_counter()
        out = E.load_color_frames(paths, threads)
        dt = time.perf_counter() - t
    assert out.shape == (n, 968, 1296, 3)
    return n / dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--jpegs", type=int, default=256)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    sd = R.golden_weights()
    net = E.ENetFeatures.from_checkpoint(sd, dev)
    frames = torch.from_numpy(R.synthetic_frames(1, a.frames, 968, 1296)).to(dev)
    ms_a, ts_a = time_gpu(lambda: net(frames), a.warmup, a.reps)
    x = E.preprocess_frames(frames, dev)
    base = torch_baseline(E.fold_state_dict(sd), dev)
    with torch.no_grad():
        ms_b, ts_b = time_gpu(lambda: base(x), a.warmup, a.reps)
        ref = base(x)
    got = net(frames)
    err = float((got - ref).abs().max() / ref.abs().max())
    fps_c = decode_rate(a.jpegs)
    flops, byts = shape_costs()
    res = {"frames": a.frames, "hip_ms": round(ms_a, 3), "hip_fps": round(a.frames / ms_a * 1e3, 1),
           "torch_conv2d_ms": round(ms_b, 3), "torch_conv2d_fps": round(a.frames / ms_b * 1e3, 1),
           "host_decode_fps_16_threads": round(fps_c, 1), "speedup_vs_conv2d": round(ms_b / ms_a, 2),
           "gflop_per_frame": round(flops / 1e9, 4), "mbytes_per_frame_lower_bound": round(byts / 1e6, 2),
           "hip_tflops": round(flops * a.frames / ms_a / 1e9, 2), "max_rel_diff_vs_conv2d": err,
           "hip_ms_all": [round(t, 3) for t in ts_a], "torch_ms_all": [round(t, 3) for t in ts_b]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
