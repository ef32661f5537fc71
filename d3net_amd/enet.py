"""ENet frame features on the device: RGB frames -> the (F,128,32,41) ENet maps that data/scannet/compute_multiview_features.py
computes per frame (EnetDataset._load_image :53-73, Sequential(enet_fixed, enet_trainable) of model/enet.py create_enet_for_3d
:697-715 in eval mode), and chained into multiview.project_multiview_features without leaving the device.  Inference only.

The host folds, once per checkpoint and in float64, every BatchNorm (eval) and the x(1 - p) of the reference's Dropout2d (its
forward scales by 1 - p even in eval mode) into the convolutions, folds the asymmetric 1x5 -> 5x1 pair into one 5x5, casts the
result to fp32 once and uploads it.  csrc/enet.hip then runs the preprocessing and 67 convolution launches per batch (DESIGN.md
3.2).  The preprocessing reproduces Pillow's NEAREST resize (ImagingScaleAffine: the source coordinate of output pixel x is the
integer part of a double accumulated by W0 / w per pixel from W0 / w / 2, not floor((x + 0.5) W0 / w)) and torchvision's
CenterCrop (left = int(round((w - 328) / 2.0)), round half to even) through per-size row / column tables.
"""
import concurrent.futures as cf
import ctypes as C
import math

import numpy as np
import torch

from . import _lib, multiview
from ._call import _ptr, _stream

IMAGE_DIMS = (328, 256)                      # (W, H): compute_multiview_features.py:30
MEAN = (0.496342, 0.466664, 0.440796)       # :70
STD = (0.277856, 0.28623, 0.291129)
NUM_FEATURES = 128
BN_EPS = 1e-3
BATCH = 256                                  # the reference's DataLoader batch_size (:93)

# blocks 4..25 of create_enet(41): (kind, cin, cout, inner, dropout p); kind: "down" (2x2/2 conv a, max pool + zero channels side),
# "reg" (3x3 dilated conv b: the int is the dilation) or "asym" (1x5 + 5x1 conv b)
_DIL = (1, 2, "asym", 4, 1, 8, "asym", 16, 1, 2, "asym", 4, 1, 8, "asym", 16)


def _blocks():
    out = [(4, "down", 16, 64, 16, 1, 0.01)] + [(b, "reg", 64, 64, 16, 1, 0.01) for b in range(5, 9)]
    out.append((9, "down", 64, 128, 32, 1, 0.1))
    for b in range(10, 26):
        d = _DIL[b - 10]
        out.append((b, "asym" if d == "asym" else "reg", 128, 128, 32, 1 if d == "asym" else d, 0.1))
    return out


BLOCKS = _blocks()


# ------------------------------------------------------------------------------------------------------------------------ tables
def pillow_nearest_table(n_in, n_out):
    """source index of each of n_out output pixels of PIL's Image.resize(..., NEAREST) along one axis of length n_in
    (Pillow's ImagingScaleAffine: a double stepped by n_in / n_out from n_in / n_out / 2, truncated)"""
    a = float(n_in) / float(n_out)
    v = a * 0.5
    out = np.empty(n_out, np.int32)
    for i in range(n_out):
        out[i] = -1 if v < 0.0 else int(v)
        v += a
    return out


def resize_width(W0, H0):
    """the reference's resize width: floor(256 * W0 / H0) in Python float (compute_multiview_features.py:56)"""
    return int(math.floor(IMAGE_DIMS[1] * float(W0) / float(H0)))


def crop_offset(w, out_w=IMAGE_DIMS[0]):
    """torchvision CenterCrop's left offset: int(round((w - out_w) / 2.0)), Python's round (half to even: 341 -> 6)"""
    return int(round((w - out_w) / 2.0))


def source_tables(H0, W0):
    """(rows (256,), cols (328,)) int32: the source row / column of every output pixel of _resize_crop_image for an (H0, W0)
    frame.  Frames whose resized width is below 328 are rejected (torchvision's CenterCrop pads them, version-dependently)."""
    W, H = IMAGE_DIMS
    if (W0, H0) == (W, H):
        return np.arange(H, dtype=np.int32), np.arange(W, dtype=np.int32)
    if H0 <= 0 or W0 <= 0:
        raise ValueError("frame size must be positive, got %dx%d" % (W0, H0))
    w = resize_width(W0, H0)
    if w < W:
        raise ValueError("a %dx%d frame resizes to width %d < %d: the reference's centre crop would pad it (unsupported)"
                         % (W0, H0, w, W))
    left, top = crop_offset(w), crop_offset(H, H)
    rows = pillow_nearest_table(H0, H)[top:top + H]
    cols = pillow_nearest_table(W0, w)[left:left + W]
    return np.ascontiguousarray(rows), np.ascontiguousarray(cols)


_TABLES = {}


def _device_tables(H0, W0, dev):
    key = (H0, W0, str(dev))
    if key not in _TABLES:
        r, c = source_tables(H0, W0)
        _TABLES[key] = (torch.from_numpy(r).to(dev), torch.from_numpy(c).to(dev))
    return _TABLES[key]


def preprocess_frames(frames_u8, device=None):
    """uint8 (F, H0, W0, 3) RGB frames (numpy or torch) -> (F, 3, 256, 328) float32 on the device: the reference's resize, crop and
    normalisation, bit for bit"""
    t = frames_u8 if torch.is_tensor(frames_u8) else torch.from_numpy(np.ascontiguousarray(frames_u8))
    if t.dtype != torch.uint8 or t.dim() != 4 or t.shape[3] != 3:
        raise ValueError("frames must be uint8 (F, H0, W0, 3), got %s %s" % (t.dtype, tuple(t.shape)))
    dev = torch.device(device) if device is not None else (t.device if t.is_cuda else torch.device("cuda", torch.cuda.current_device()))
    F, H0, W0 = int(t.shape[0]), int(t.shape[1]), int(t.shape[2])
    rows, cols = _device_tables(H0, W0, dev)
    t = t.to(dev, non_blocking=True).contiguous()
    W, H = IMAGE_DIMS
    out = torch.empty((F, 3, H, W), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().d3_enet_preprocess(_ptr(t), F, H0, W0, _ptr(rows), _ptr(cols), H, W, _ptr(out), _stream()),
                   "enet_preprocess")
    return out


# ------------------------------------------------------------------------------------------------------------------------ weights
def _keys_conv(p, bias):
    return [p + ".weight"] + ([p + ".bias"] if bias else [])


def _keys_bn(p):
    return [p + "." + k for k in ("weight", "bias", "running_mean", "running_var")]


def required_keys():
    """every state-dict key of create_enet(41) elements 0-25 that the features read (element 26, the classifier, is not one)"""
    keys = _keys_conv("0.0", True) + _keys_bn("2") + ["3.weight"]
    for b, kind, *_ in BLOCKS:
        m = "%d.0.0." % b
        keys += _keys_conv(m + "0", False) + _keys_bn(m + "1") + [m + "2.weight"]
        if kind == "asym":
            keys += _keys_conv(m + "3", False) + _keys_conv(m + "4", True) + _keys_bn(m + "5") + [m + "6.weight"]
            keys += _keys_conv(m + "7", False) + _keys_bn(m + "8")
        else:
            keys += _keys_conv(m + "3", True) + _keys_bn(m + "4") + [m + "5.weight"]
            keys += _keys_conv(m + "6", False) + _keys_bn(m + "7")
        keys.append("%d.2.weight" % b)
    return keys


def _bn_affine(sd, p):
    g, b, m, v = (sd[p + "." + k] for k in ("weight", "bias", "running_mean", "running_var"))
    scale = g / np.sqrt(v + BN_EPS)
    return scale, b - m * scale


def _fold(W, bias, scale, shift, mult=1.0):
    """BN(conv(x) + bias) * mult as one convolution (float64)"""
    Wf = W * scale[:, None, None, None] * mult
    b = (0.0 if bias is None else bias)
    return Wf, (b * scale + shift) * mult


def fold_state_dict(state_dict):
    """float64 fold of a create_enet(41) state dict -> list of 67 (W (cout, cin, kh, kw), bias, slope) float64 arrays in the order of
    d3_enet_layers; the initial block's entry is (W (13,3,3,3), bias 13, pool scale 3, pool shift 3, slope 16)."""
    missing = [k for k in required_keys() if k not in state_dict]
    if missing:
        raise KeyError("ENet checkpoint lacks %d key(s): %s" % (len(missing), ", ".join(missing[:8]) + (" ..." if len(missing) > 8 else "")))
    sd = {k: (v.detach().cpu().double().numpy() if torch.is_tensor(v) else np.asarray(v, np.float64)) for k, v in state_dict.items()
          if k in set(required_keys())}
    scale, shift = _bn_affine(sd, "2")
    W0, b0 = _fold(sd["0.0.weight"], sd["0.0.bias"], scale[:13], shift[:13])
    layers = [(W0, b0, scale[13:], shift[13:], sd["3.weight"])]
    for b, kind, *_rest in BLOCKS:
        p = _rest[-1]
        m = "%d.0.0." % b
        s, t = _bn_affine(sd, m + "1")
        layers.append(_fold(sd[m + "0.weight"], None, s, t) + (sd[m + "2.weight"],))
        if kind == "asym":
            W15, W51 = sd[m + "3.weight"], sd[m + "4.weight"]           # (32,32,1,5), (32,32,5,1)
            W55 = np.einsum("omy,mix->oiyx", W51[:, :, :, 0], W15[:, :, 0, :])
            s, t = _bn_affine(sd, m + "5")
            layers.append(_fold(W55, sd[m + "4.bias"], s, t) + (sd[m + "6.weight"],))
            cc, bc = m + "7", m + "8"
        else:
            s, t = _bn_affine(sd, m + "4")
            layers.append(_fold(sd[m + "3.weight"], sd[m + "3.bias"], s, t) + (sd[m + "5.weight"],))
            cc, bc = m + "6", m + "7"
        s, t = _bn_affine(sd, bc)
        layers.append(_fold(sd[cc + ".weight"], None, s, t, 1.0 - p) + (sd["%d.2.weight" % b],))
    return layers


def _pad4(a):
    a = np.asarray(a, np.float32).ravel()
    return np.concatenate([a, np.zeros((-len(a)) % 4, np.float32)])


def layer_table():
    """the library's (67, 7) layer table: cin, cout, kh, kw, stride, pad, dilation"""
    L = _lib.lib()
    n = L.d3_enet_layers(None, 0)
    t = (C.c_int * (7 * n))()
    if L.d3_enet_layers(t, 7 * n) != n:
        raise _lib.D3Error("d3_enet_layers failed")
    return np.array(t[:], np.int32).reshape(n, 7)


def pack_params(layers):
    """folded float64 layers -> the fp32 blob of d3_enet_layers' layout (one cast per value)"""
    segs = []
    W0, b0, ps, pt, sl = layers[0]
    segs += [_pad4(W0), _pad4(b0), _pad4(ps), _pad4(pt), _pad4(sl)]
    for W, b, sl in layers[1:]:
        segs += [_pad4(np.transpose(W, (2, 3, 0, 1))), _pad4(b), _pad4(sl)]
    return np.concatenate(segs)


class ENetFeatures:
    """The reference's Sequential(enet_fixed, enet_trainable).eval() on the device.  net(frames) -> (F,128,H/8,W/8) float32."""

    def __init__(self, params, device):
        self.device = torch.device(device)
        self.table = layer_table()
        want = int(_lib.lib().d3_enet_param_count())
        if params.size != want:
            raise ValueError("folded parameter blob has %d floats, the library expects %d" % (params.size, want))
        self.params = torch.from_numpy(np.ascontiguousarray(params, np.float32)).to(self.device)
        self._tab = (C.c_int * self.table.size)(*self.table.ravel().tolist())

    @classmethod
    def from_checkpoint(cls, path_or_state_dict, device="cuda"):
        """scannetv2_enet.pth (the state dict of create_enet(41); element 26 is ignored) or such a dict"""
        sd = path_or_state_dict
        if not isinstance(sd, dict):
            sd = torch.load(sd, map_location="cpu")
        layers = fold_state_dict(sd)
        table = layer_table()
        for l, (row, lay) in enumerate(zip(table, layers)):
            W = lay[0]
            shape = (13, 3, 3, 3) if l == 0 else (row[1], row[0], row[2], row[3])
            if tuple(W.shape) != shape:
                raise ValueError("ENet layer %d has weight shape %s, expected %s" % (l, tuple(W.shape), shape))
        return cls(pack_params(layers), device)

    def forward_preprocessed(self, x, upto=25):
        """x (F, 3, H, W) float32 on the device, H and W multiples of 8 -> (F, 128, H/8, W/8); upto < 25: the output of that element
        of create_enet(41) instead ((F, 16, H/2, W/2) for 3, (F, 64, H/4, W/4) for 4..8, (F, 128, H/8, W/8) for 9..24)"""
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError("input must be (F, 3, H, W), got %s" % (tuple(x.shape),))
        x = x.to(device=self.device, dtype=torch.float32).contiguous()
        F, H, W = int(x.shape[0]), int(x.shape[2]), int(x.shape[3])
        upto = int(upto)
        if upto == 25:
            out = torch.empty((F, NUM_FEATURES, H // 8, W // 8), dtype=torch.float32, device=self.device)
        else:
            d, c = (2, 16) if upto == 3 else ((4, 64) if upto <= 8 else (8, 128))
            out = torch.empty((F, H // d, W // d, c), dtype=torch.float32, device=self.device)
        if F == 0:
            return out if upto == 25 else out.permute(0, 3, 1, 2)
        L = _lib.lib()
        need = L.d3_enet_ws_bytes(F, H, W)
        ws = torch.empty(max(int(need), 1), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(L.d3_enet_forward(_ptr(x), F, H, W, _ptr(self.params), self.params.numel(), self._tab, self.table.size, upto,
                                         _ptr(out), _ptr(ws), need, _stream()), "enet_forward (F=%d, %dx%d)" % (F, H, W))
        return out if upto == 25 else out.permute(0, 3, 1, 2)

    def __call__(self, frames, batch=BATCH):
        """uint8 (F, H0, W0, 3) frames or preprocessed float32 (F, 3, H, W) -> (F, 128, H/8, W/8) float32 on the device, in chunks
        of `batch` frames"""
        u8 = frames.dtype == torch.uint8 if torch.is_tensor(frames) else np.asarray(frames).dtype == np.uint8
        if not torch.is_tensor(frames):
            frames = torch.from_numpy(np.ascontiguousarray(frames))
        if u8:
            W, H = IMAGE_DIMS
            if frames.dim() != 4 or frames.shape[3] != 3:
                raise ValueError("frames must be uint8 (F, H0, W0, 3), got %s" % (tuple(frames.shape),))
        else:
            H, W = int(frames.shape[2]), int(frames.shape[3])
        F = int(frames.shape[0])
        out = torch.empty((F, NUM_FEATURES, H // 8, W // 8), dtype=torch.float32, device=self.device)
        for s in range(0, F, batch):
            chunk = frames[s:s + batch]
            x = preprocess_frames(chunk, self.device) if u8 else chunk
            out[s:s + batch] = self.forward_preprocessed(x)
        return out


def scene_multiview_features(points, frames_u8, depths, poses, net, maxpool=True, helper=None, return_counts=False):
    """One scene's multiview rows straight from its RGB frames: project_multiview_features(points, depths, poses, net(frames_u8)).
    The ENet maps stay on the device."""
    feats = net(frames_u8)
    return multiview.project_multiview_features(points, depths, poses, feats, maxpool=maxpool, helper=helper,
                                                return_counts=return_counts)


def load_color_frames(paths, threads=16):
    """decode JPEG (or any Pillow-readable) colour frames on the host into one pinned uint8 (F, H0, W0, 3) tensor; all frames must
    share a size.  Pillow is what the reference's imageio.imread uses for JPEG."""
    from PIL import Image
    paths = list(paths)
    if not paths:
        raise ValueError("no frames")
    threads = max(1, min(16, int(threads)))
    with Image.open(paths[0]) as im:
        W0, H0 = im.size
    out = torch.empty((len(paths), H0, W0, 3), dtype=torch.uint8, pin_memory=torch.cuda.is_available())
    arr = out.numpy()

    def one(i):
        with Image.open(paths[i]) as im:
            a = np.asarray(im.convert("RGB"))
        if a.shape != (H0, W0, 3):
            raise ValueError("%s is %s, the first frame %s" % (paths[i], a.shape, (H0, W0, 3)))
        arr[i] = a

    with cf.ThreadPoolExecutor(max_workers=threads) as ex:
        list(ex.map(one, range(len(paths))))
    return out
