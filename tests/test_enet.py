"""Host side of d3net_amd.enet: the torch-CPU restatement (tests/enet_restate.py) against the reference's own outputs
(tests/golden/enet_golden.npz), the preprocessing tables against Pillow, crop rounding, the checkpoint key mapping, the float64
fold, and argument errors of the C ABI that return before any launch.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import enet_restate as R
from d3net_amd import _lib, enet as E

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "enet_golden.npz"))
SIZES = [(1296, 968), (640, 480), (1920, 1440)]
TOL = 1e-4          # max |got - ref| <= TOL * max |ref| per frame


def test_restatement_matches_reference():
    out = R.forward(R.golden_weights(), R.golden_input(1, 2, 64, 80))
    for k in (3, 8, 25):
        assert R.rel_err(out[k].numpy(), G["small/e%d" % k]).max() < 2e-5, k
    full = R.forward(R.golden_weights(), R.golden_input(2, 1, 256, 328), keep=(25,))[25]
    assert R.rel_err(full.numpy(), G["full/e25"]).max() < 2e-5


def test_golden_activations_are_order_one():
    for k in ("small/e3", "small/e8", "small/e25", "full/e25"):
        a = G[k]
        assert 0.5 < np.abs(a).max() < 50 and (a < 0).mean() > 0.05, k


def test_state_shapes_cover_required_keys():
    assert set(R.state_shapes()) == set(E.required_keys())


@pytest.mark.parametrize("W0,H0", SIZES)
def test_host_tables_equal_pinned_pillow_tables(W0, H0):
    rows, cols = E.source_tables(H0, W0)
    key = "tables/%dx%d/" % (W0, H0)
    np.testing.assert_array_equal(rows, G[key + "rows"])
    np.testing.assert_array_equal(cols, G[key + "cols"])
    assert E.resize_width(W0, H0) == int(G[key + "width"])
    assert E.crop_offset(E.resize_width(W0, H0)) == int(G[key + "left"])
    assert rows.dtype == np.int32 and rows.shape == (256,) and cols.shape == (328,)


@pytest.mark.parametrize("W0,H0", SIZES + [(500, 300), (1000, 700), (333, 250), (328, 256)])
def test_host_tables_equal_live_pillow(W0, H0):
    pytest.importorskip("PIL")
    rows, cols = E.source_tables(H0, W0)
    r2, c2 = R.pil_source_tables(H0, W0)
    np.testing.assert_array_equal(rows, r2)
    np.testing.assert_array_equal(cols, c2)


def test_pillow_nearest_is_not_the_closed_form():
    t = E.pillow_nearest_table(1296, 342)
    closed = np.floor((np.arange(342) + 0.5) * 1296 / 342).astype(np.int32)
    assert (t != closed).sum() == 14
    t = E.pillow_nearest_table(640, 341)
    assert (t != np.floor((np.arange(341) + 0.5) * 640 / 341).astype(np.int32)).sum() == 1


def test_crop_rounding():
    assert E.resize_width(1296, 968) == 342 and E.crop_offset(342) == 7
    assert E.resize_width(640, 480) == 341 and E.crop_offset(341) == 6      # round(6.5) == 6: half to even
    assert E.crop_offset(343) == 8 and E.crop_offset(328) == 0
    rows, cols = E.source_tables(256, 328)
    assert (rows == np.arange(256)).all() and (cols == np.arange(328)).all()


def test_narrow_frames_rejected():
    with pytest.raises(ValueError, match="width"):
        E.source_tables(480, 400)        # 256 * 400 / 480 = 213 < 328


def test_preprocess_restatement_is_the_reference_chain():
    fr = R.synthetic_frames(3, 2, 968, 1296)
    rows, cols = E.source_tables(968, 1296)
    x = R.preprocess(fr, rows, cols)
    img = fr[0][rows][:, cols]
    want = (np.transpose(img, (2, 0, 1)).astype(np.float32) / 255.0 - R.MEAN32[:, None, None]) / R.STD32[:, None, None]
    assert x.dtype == np.float32 and x[0].tobytes() == want.astype(np.float32).tobytes()


def test_checkpoint_key_mapping():
    sd = R.golden_weights()
    sd["26.weight"] = torch.zeros(41, 16, 3, 3)       # the classifier: ignored
    sd["2.num_batches_tracked"] = torch.tensor(0)
    layers = E.fold_state_dict(sd)
    assert len(layers) == 67
    sd2 = dict(sd)
    del sd2["12.0.0.4.bias"], sd2["25.2.weight"]
    with pytest.raises(KeyError) as ei:
        E.fold_state_dict(sd2)
    assert "12.0.0.4.bias" in str(ei.value) and "25.2.weight" in str(ei.value)


def test_fold_matches_unfolded_layers():
    sd = R.golden_weights()
    layers = E.fold_state_dict(sd)
    x = R.golden_input(1, 2, 64, 80)
    ref64 = R.forward(sd, x, torch.float64, keep=(25,))[25].numpy()
    # the float64 fold is the unfolded network in exact arithmetic
    assert R.rel_err(R.folded_forward(layers, x, torch.float64).numpy(), ref64).max() < 1e-12
    # the fp32 cast of the fold stays 4x inside the device tolerance
    assert R.rel_err(R.folded_forward(layers, x).numpy(), ref64).max() < TOL / 4
    xf = R.golden_input(2, 1, 256, 328)
    ref64 = R.forward(sd, xf, torch.float64, keep=(25,))[25].numpy()
    assert R.rel_err(R.folded_forward(layers, xf).numpy(), ref64).max() < TOL / 4


def test_layer_table_and_blob(built_lib):
    t = E.layer_table()
    assert t.shape == (67, 7)
    assert tuple(t[0]) == (3, 16, 3, 3, 2, 1, 1)
    assert tuple(t[1]) == (16, 16, 2, 2, 2, 0, 1) and tuple(t[3]) == (16, 64, 1, 1, 1, 0, 1)
    assert tuple(t[1 + 3 * 8 + 1]) == (32, 32, 5, 5, 1, 2, 1)         # block 12: asymmetric, folded to 5x5
    assert tuple(t[1 + 3 * 21 + 1]) == (32, 32, 3, 3, 1, 16, 16)      # block 25: dilation 16
    blob = E.pack_params(E.fold_state_dict(R.golden_weights()))
    assert blob.dtype == np.float32 and blob.size == _lib.lib().d3_enet_param_count()


def test_argument_errors_before_launch(built_lib):
    L = _lib.lib()
    t = E.layer_table()
    n = int(L.d3_enet_param_count())
    tab = (C.c_int * t.size)(*t.ravel().tolist())
    dummy = C.c_void_p(16)
    ws = L.d3_enet_ws_bytes(2, 64, 80)
    assert ws > 0 and L.d3_enet_ws_bytes(2, 60, 80) == 0 and L.d3_enet_ws_bytes(2, 64, 84) == 0
    fwd = lambda F, H, W, n=n, tab=tab, nt=t.size, up=25: L.d3_enet_forward(dummy, F, H, W, dummy, n, tab, nt, up, dummy, dummy, 1 << 40, None)  # noqa: E731
    assert fwd(2, 60, 80) == -3 and fwd(2, 64, 84) == -3 and fwd(2, 0, 80) == -3
    assert fwd(2, 64, 80, n=n - 4) == -3
    bad = (C.c_int * t.size)(*t.ravel().tolist())
    bad[7 * 3 + 1] = 32                                               # block 4 conv c: 64 -> 32 output channels
    assert fwd(2, 64, 80, tab=bad) == -3
    assert fwd(2, 64, 80, nt=t.size - 7) == -3
    assert fwd(2, 32768, 16384) == -2                                 # H * W * 4 >= 2^31
    assert fwd(70000, 64, 80) == -2
    assert fwd(2, 64, 80, up=2) == -3 and fwd(2, 64, 80, up=26) == -3
    assert L.d3_enet_forward(dummy, 2, 64, 80, dummy, n, tab, t.size, 25, dummy, dummy, 16, None) == -1   # workspace too small
    pre = L.d3_enet_preprocess
    assert pre(dummy, 2, 968, 1296, dummy, dummy, 0, 328, dummy, None) == -3
    assert pre(dummy, 2, 46341, 15447, dummy, dummy, 256, 328, dummy, None) == -2
    assert pre(dummy, 70000, 968, 1296, dummy, dummy, 256, 328, dummy, None) == -2
    assert L.d3_enet_layers(tab, 10) == -3 and L.d3_enet_layers(None, 0) == 67


def test_python_argument_errors():
    with pytest.raises(ValueError):
        E.preprocess_frames(np.zeros((2, 968, 1296, 4), np.uint8))
    with pytest.raises(ValueError):
        E.preprocess_frames(np.zeros((2, 968, 1296, 3), np.float32))
    with pytest.raises(ValueError):
        E.ENetFeatures(np.zeros(10, np.float32), "cpu")
