"""Torch-CPU restatement of the reference's ENet feature path (model/enet.py create_enet(41), elements 0-25, eval mode, and
data/scannet/compute_multiview_features.py:53-73 preprocessing), for tests/golden/gen_enet_golden.py and the enet tests.

* `forward`: the UNFOLDED network, layer by layer as the reference's modules compute it (conv2d, batch_norm in eval, prelu,
  max_pool2d, appended zero channels, x(1 - p) of its Dropout2d), in any float dtype.
* `folded_forward`: the network from d3net_amd.enet.fold_state_dict's float64 fold (what the device runs), cast to a dtype.
* `state_shapes` / `golden_weights`: the key names and shapes of create_enet(41) elements 0-25 and deterministic name-seeded
  weights (the fixture stores no weights).
* `pil_source_tables` / `preprocess`: the source row / column of each output pixel read back from a live Pillow resize of an image
  whose pixels encode their own coordinates, and the reference's float32 normalisation in numpy.
"""
import math
import zlib

import numpy as np
import torch
import torch.nn.functional as Fn

from d3net_amd import enet as E

MEAN32 = np.array(E.MEAN, np.float32)
STD32 = np.array(E.STD, np.float32)


# ---------------------------------------------------------------------------------------------------------------- weights
def state_shapes():
    """key -> shape of every parameter / buffer of create_enet(41) elements 0-25 that the features read"""
    out = {"0.0.weight": (13, 3, 3, 3), "0.0.bias": (13,), "3.weight": (16,)}
    for k in ("weight", "bias", "running_mean", "running_var"):
        out["2." + k] = (16,)

    def bn(p, c):
        for k in ("weight", "bias", "running_mean", "running_var"):
            out[p + "." + k] = (c,)

    for b, kind, cin, cout, inner, d, p in E.BLOCKS:
        m = "%d.0.0." % b
        out[m + "0.weight"] = (inner, cin, 2, 2) if kind == "down" else (inner, cin, 1, 1)
        bn(m + "1", inner)
        out[m + "2.weight"] = (inner,)
        if kind == "asym":
            out[m + "3.weight"] = (inner, inner, 1, 5)
            out[m + "4.weight"], out[m + "4.bias"] = (inner, inner, 5, 1), (inner,)
            bn(m + "5", inner)
            out[m + "6.weight"] = (inner,)
            out[m + "7.weight"] = (cout, inner, 1, 1)
            bn(m + "8", cout)
        else:
            out[m + "3.weight"], out[m + "3.bias"] = (inner, inner, 3, 3), (inner,)
            bn(m + "4", inner)
            out[m + "5.weight"] = (inner,)
            out[m + "6.weight"] = (cout, inner, 1, 1)
            bn(m + "7", cout)
        out["%d.2.weight" % b] = (cout,)
    return out


def golden_weights(shapes=None):
    """deterministic float32 weights, N(0,1) seeded by crc32(name): convolutions N(0,1) * s / sqrt(fan_in) (s = 1.2 for the
    convolutions that feed a PReLU, 0.3 for conv c, whose output joins the residual sum), BN gamma 1 + 0.2 N, beta / running_mean
    0.2 N, running_var 0.4 + 0.6 |N|, PReLU slopes 0.25 + 0.15 N, convolution biases 0.1 N.  Activations stay O(1) through the
    22 blocks."""
    shapes = shapes or state_shapes()
    conv_c = {"%d.0.0.%d.weight" % (b, 7 if kind == "asym" else 6) for b, kind, *_ in E.BLOCKS}
    out = {}
    for name, shape in shapes.items():
        a = np.random.default_rng(zlib.crc32(name.encode())).standard_normal(shape)
        base, leaf = name.rsplit(".", 1)
        bn = base + ".running_var" in shapes
        if len(shape) == 4:
            a = a * ((0.3 if name in conv_c else 1.2) / math.sqrt(shape[1] * shape[2] * shape[3]))
        elif leaf == "running_var":
            a = 0.4 + 0.6 * np.abs(a)
        elif bn and leaf == "weight":
            a = 1.0 + 0.2 * a
        elif bn:                                         # BN bias, running_mean
            a = 0.2 * a
        elif leaf == "weight":                           # PReLU
            a = 0.25 + 0.15 * a
        else:                                            # convolution bias
            a = 0.1 * a
        out[name] = torch.from_numpy(np.asarray(a, np.float32).copy())
    return out


def golden_input(seed, F, H, W):
    """seeded stand-in for normalized frames: (F, 3, H, W) float32 N(0,1)"""
    return np.random.default_rng(seed).standard_normal((F, 3, H, W)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- network
def forward(sd, x, dtype=torch.float32, keep=(3, 8, 25)):
    """unfolded reference network on the CPU -> {element: output} for the elements in keep"""
    P = {k: v.to(dtype) for k, v in sd.items()}
    x = torch.as_tensor(x).to(dtype)

    def bn(t, p):
        return Fn.batch_norm(t, P[p + ".running_mean"], P[p + ".running_var"], P[p + ".weight"], P[p + ".bias"], False, 0.1, 1e-3)

    out = {}
    y = torch.cat([Fn.conv2d(x, P["0.0.weight"], P["0.0.bias"], stride=2, padding=1), Fn.max_pool2d(x, 2, 2)], 1)
    y = Fn.prelu(bn(y, "2"), P["3.weight"])
    if 3 in keep:
        out[3] = y
    for b, kind, cin, cout, inner, d, p in E.BLOCKS:
        m = "%d.0.0." % b
        if kind == "down":
            t = Fn.conv2d(y, P[m + "0.weight"], stride=2)
        else:
            t = Fn.conv2d(y, P[m + "0.weight"])
        t = Fn.prelu(bn(t, m + "1"), P[m + "2.weight"])
        if kind == "asym":
            t = Fn.conv2d(t, P[m + "3.weight"], padding=(0, 2))
            t = Fn.conv2d(t, P[m + "4.weight"], P[m + "4.bias"], padding=(2, 0))
            t = Fn.prelu(bn(t, m + "5"), P[m + "6.weight"])
            t = bn(Fn.conv2d(t, P[m + "7.weight"]), m + "8")
        else:
            t = Fn.conv2d(t, P[m + "3.weight"], P[m + "3.bias"], padding=d, dilation=d)
            t = Fn.prelu(bn(t, m + "4"), P[m + "5.weight"])
            t = bn(Fn.conv2d(t, P[m + "6.weight"]), m + "7")
        t = t * (1 - p)                                  # Dropout2d.forward: input * (1 - p), then eval identity
        if kind == "down":
            s = Fn.max_pool2d(y, 2, 2)
            s = torch.cat([s, s.new_zeros((s.shape[0], cout - cin, s.shape[2], s.shape[3]))], 1)
        else:
            s = y
        y = Fn.prelu(t + s, P["%d.2.weight" % b])
        if b in keep:
            out[b] = y
    return out


def folded_forward(layers, x, dtype=torch.float32):
    """the network from enet.fold_state_dict's layers (float64 arrays) cast to dtype -> element 25 output"""
    T = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)  # noqa: E731
    x = torch.as_tensor(x).to(dtype)
    W0, b0, ps, pt, sl = layers[0]
    c = Fn.conv2d(x, T(W0), T(b0), stride=2, padding=1)
    m = Fn.max_pool2d(x, 2, 2) * T(ps)[None, :, None, None] + T(pt)[None, :, None, None]
    y = Fn.prelu(torch.cat([c, m], 1), T(sl))
    l = 1
    for b, kind, cin, cout, inner, d, p in E.BLOCKS:
        Wa, ba, sa = layers[l]
        Wb, bb, sb = layers[l + 1]
        Wc, bc, sc = layers[l + 2]
        l += 3
        t = Fn.prelu(Fn.conv2d(y, T(Wa), T(ba), stride=2 if kind == "down" else 1), T(sa))
        pad = 2 if kind == "asym" else d
        t = Fn.prelu(Fn.conv2d(t, T(Wb), T(bb), padding=pad, dilation=1 if kind == "asym" else d), T(sb))
        t = Fn.conv2d(t, T(Wc), T(bc))
        if kind == "down":
            s = Fn.max_pool2d(y, 2, 2)
            s = torch.cat([s, s.new_zeros((s.shape[0], cout - cin, s.shape[2], s.shape[3]))], 1)
        else:
            s = y
        y = Fn.prelu(t + s, T(sc))
    return y


def rel_err(got, ref):
    """per frame: max |got - ref| / max |ref|"""
    g = np.asarray(got, np.float64).reshape(len(got), -1)
    r = np.asarray(ref, np.float64).reshape(len(ref), -1)
    return np.abs(g - r).max(1) / np.abs(r).max(1)


# ---------------------------------------------------------------------------------------------------------------- preprocessing
def pil_source_tables(H0, W0):
    """(rows, cols) of _resize_crop_image read back from live Pillow: resize images whose pixels hold their own coordinates with
    Image.NEAREST to (w, 256), then take the centre-crop box"""
    from PIL import Image
    W, H = E.IMAGE_DIMS
    w = int(math.floor(H * float(W0) / float(H0)))
    yy, xx = np.meshgrid(np.arange(H0), np.arange(W0), indexing="ij")
    enc = lambda a, b: np.stack([a & 255, a >> 8, b & 255], -1).astype(np.uint8)  # noqa: E731
    left, top = int(round((w - W) / 2.0)), int(round((H - H) / 2.0))
    box = (left, top, left + W, top + H)
    cx = np.asarray(Image.fromarray(enc(xx, yy)).resize((w, H), Image.NEAREST).crop(box)).astype(np.int64)
    cy = np.asarray(Image.fromarray(enc(yy, xx)).resize((w, H), Image.NEAREST).crop(box)).astype(np.int64)
    return (cy[:, 0, 0] + 256 * cy[:, 0, 1]).astype(np.int32), (cx[0, :, 0] + 256 * cx[0, :, 1]).astype(np.int32)


def preprocess(frames_u8, rows, cols):
    """the reference's float chain on the gathered pixels: astype(float32) / 255.0, then (x - mean) / std in float32 (NCHW)"""
    img = np.asarray(frames_u8)[:, rows][:, :, cols]                  # (F, H, W, 3)
    x = np.transpose(img, (0, 3, 1, 2)).astype(np.float32) / np.float32(255.0)
    return (x - MEAN32[None, :, None, None]) / STD32[None, :, None, None]


def synthetic_frames(seed, F, H0, W0):
    """uint8 (F, H0, W0, 3): smooth gradients plus noise, every value 0..255 present"""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.linspace(0, 1, H0), np.linspace(0, 1, W0), indexing="ij")
    out = np.empty((F, H0, W0, 3), np.uint8)
    for f in range(F):
        base = np.stack([xx, yy, 0.5 * (xx + yy)], -1) * 200 + rng.integers(0, 56, (H0, W0, 3))
        out[f] = np.clip(base + f, 0, 255).astype(np.uint8)
    return out
