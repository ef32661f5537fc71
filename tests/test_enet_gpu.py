"""d3net_amd.enet on the device (csrc/enet.hip): preprocessing bit for bit against the reference's float chain, the network against
the reference's own outputs (tests/golden/enet_golden.npz) and the torch-CPU restatement (tests/enet_restate.py) within
max |dev - ref| <= 1e-4 max |ref| per frame, bitwise batch invariance and determinism, the chain into
multiview.project_multiview_features, and argument / range errors."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import enet_restate as R
import multiview_restate as MR
from d3net_amd import _lib, enet as E, multiview as MV

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "enet_golden.npz"))
TOL = 1e-4

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def net(dev):
    return E.ENetFeatures.from_checkpoint(R.golden_weights(), dev)


def _within(got, ref, what):
    e = R.rel_err(got.cpu().numpy() if torch.is_tensor(got) else got, ref)
    assert (e <= TOL).all(), (what, e.max())
    return e.max()


@pytest.mark.parametrize("W0,H0", [(1296, 968), (640, 480), (328, 256)])
def test_preprocess_bit_exact(dev, W0, H0):
    fr = R.synthetic_frames(W0, 3, H0, W0)
    got = E.preprocess_frames(fr, dev)
    assert got.shape == (3, 3, 256, 328) and got.device == dev
    rows, cols = E.source_tables(H0, W0)
    want = R.preprocess(fr, rows, cols)
    assert got.cpu().numpy().tobytes() == want.tobytes()


def test_golden_small(dev, net):
    x = torch.from_numpy(R.golden_input(1, 2, 64, 80)).to(dev)
    out = net(x)
    assert out.shape == (2, 128, 8, 10) and out.dtype == torch.float32
    _within(out, G["small/e25"], "element 25")


@pytest.mark.parametrize("elem", [3, 8])
def test_golden_intermediates(dev, net, elem):
    x = torch.from_numpy(R.golden_input(1, 2, 64, 80)).to(dev)
    out = net.forward_preprocessed(x, upto=elem)
    assert out.shape == G["small/e%d" % elem].shape
    _within(out, G["small/e%d" % elem], "element %d" % elem)


def test_golden_full_frame(dev, net):
    x = torch.from_numpy(R.golden_input(2, 1, 256, 328)).to(dev)
    out = net(x)
    assert out.shape == (1, 128, 32, 41)
    _within(out, G["full/e25"], "full frame")


def test_full_batch_against_restatement(dev, net):
    fr = R.synthetic_frames(11, 256, 968, 1296)
    frames = torch.from_numpy(fr).to(dev)
    out = net(frames)
    torch.cuda.synchronize()
    assert out.shape == (256, 128, 32, 41) and torch.isfinite(out).all()
    rows, cols = E.source_tables(968, 1296)
    pick = [0, 1, 37, 100, 128, 200, 254, 255]
    ref = R.forward(R.golden_weights(), R.preprocess(fr[pick], rows, cols), keep=(25,))[25].numpy()
    _within(out[pick], ref, "256-frame batch")


def test_batch_invariance_and_determinism(dev, net):
    fr = torch.from_numpy(R.synthetic_frames(5, 256, 480, 640)).to(dev)
    a = net(fr)
    b = net(fr)
    assert torch.equal(a, b), "two runs differ"
    one = net(fr[17:18])
    assert one[0].cpu().numpy().tobytes() == a[17].cpu().numpy().tobytes()
    part = net(fr[100:137])
    assert part.cpu().numpy().tobytes() == a[100:137].cpu().numpy().tobytes()
    c = net(fr, batch=37)
    assert c.cpu().numpy().tobytes() == a.cpu().numpy().tobytes()


def test_scene_multiview_features(dev, net):
    pts, dep, poses, _ = MR.room_scene(4, 3000, 10)
    fr = R.synthetic_frames(9, len(dep), 968, 1296)
    got = E.scene_multiview_features(pts, fr, dep, poses, net)
    feats = net(torch.from_numpy(fr).to(dev))
    want = MV.project_multiview_features(pts, dep, poses, feats)
    assert got.shape == (len(pts), 128)
    assert got.cpu().numpy().tobytes() == want.cpu().numpy().tobytes()
    # against restated features: the projection only gathers and max-pools, so the tolerance carries over per frame
    rows, cols = E.source_tables(968, 1296)
    rf = R.forward(R.golden_weights(), R.preprocess(fr, rows, cols), keep=(25,))[25]
    ref = MV.project_multiview_features(pts, dep, poses, rf.to(dev)).cpu().numpy()
    scale = np.abs(rf.numpy()).max()
    assert np.abs(got.cpu().numpy() - ref).max() <= TOL * scale
    assert (np.abs(ref).sum(1) > 0).mean() > 0.2


def test_errors(dev, net):
    with pytest.raises(_lib.D3Error, match="D3_ERR_ARG"):
        net(torch.zeros((1, 3, 60, 80), device=dev))
    with pytest.raises(ValueError):
        net(torch.zeros((1, 4, 64, 80), device=dev))
    t = net.table
    bad = (C.c_int * t.size)(*t.ravel().tolist())
    bad[7 * 67 - 6] = 64
    x = torch.zeros((1, 3, 64, 80), device=dev)
    out = torch.empty((1, 128, 8, 10), device=dev)
    L = _lib.lib()
    ws = torch.empty(L.d3_enet_ws_bytes(1, 64, 80), dtype=torch.uint8, device=dev)
    p = lambda a: C.c_void_p(a.data_ptr())  # noqa: E731
    rc = L.d3_enet_forward(p(x), 1, 64, 80, p(net.params), net.params.numel(), bad, t.size, 25, p(out), p(ws), ws.numel(), None)
    assert rc == -3
    rc = L.d3_enet_forward(p(x), 1, 32768, 16384, p(net.params), net.params.numel(), net._tab, t.size, 25, p(out), p(ws), ws.numel(), None)
    assert rc == -2
    with pytest.raises(ValueError, match="width"):
        E.preprocess_frames(np.zeros((1, 480, 400, 3), np.uint8), dev)
