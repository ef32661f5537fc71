"""GPU parity of the ScanRefer match module (d3net_amd.listener.ScanReferMatchModule over csrc/scanrefer_match.hip).

Against tests/golden/scanrefer_match_golden.npz -- the reference's own MatchModule / ListenerNet / loss_helper run in float64
(gen_scanrefer_match_golden.py) -- at module and at listener level, and against the same formulas written with plain torch
operators in float64 (`compose` below) on ragged shapes.  Bounds are the listener's (tests/test_listener_gpu.py): outputs and
running statistics rtol 1e-3, atol 1e-4; gradients rtol 5e-3, atol 1e-5 + 2e-3 max|ref|.  The reference in fp32 differs from
its own float64 run by at most 1e-5 (outputs, magnitude 10) and 5e-6 (gradients, magnitude 3) on the fixture: the bounds sit
10 x or more above fp32 rounding.

Gradients that are mathematically zero take max|ref| from the same layer's WEIGHT gradient instead of from the zero vector:
fuse.0.bias whenever fuse.1 normalises with batch statistics (a shift of its input cancels), match.5.bias and match.6.bias
under the softmax ranking loss (a shift of every confidence of a sample cancels)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

PARAMS = ("fuse.0.weight", "fuse.0.bias", "fuse.1.weight", "fuse.1.bias", "fuse.2.weight", "fuse.3.weight", "fuse.3.bias",
          "match.0.weight", "match.0.bias", "match.2.weight", "match.2.bias", "match.3.weight", "match.3.bias", "match.5.weight",
          "match.5.bias", "match.6.weight", "match.6.bias")
BNS = ("fuse.1", "match.2", "match.5")
ZERO_TRAIN_RANKING = ("fuse.0.bias", "match.5.bias", "match.6.bias")
ZERO_EVAL_RANKING = ("match.5.bias", "match.6.bias")
ZERO_TRAIN = ("fuse.0.bias",)


# ------------------------------------------------------------------------------------ torch composition
def compose(feats, lang, mask, div, sd, train, momentum=0.1, eps=1e-5):
    """MatchModule.forward (model/match_module.py:110-139; mask None: the RL branch :62-83) with plain torch operators in the
    dtype of its inputs.  sd: state dict (name -> tensor).  Returns (confidences (N, K), new running statistics)."""
    N, K = lang.shape[0], feats.shape[1]
    b = torch.arange(N, device=feats.device) // div
    x = torch.cat([feats[b], lang[:, None, :].expand(-1, K, -1)], dim=-1)
    if mask is not None:
        x = x * mask[b][:, :, None]
    new = {}

    def conv(x, name):
        return x @ sd[name + ".weight"].squeeze(-1).t() + sd[name + ".bias"]

    def bn(x, name):
        if train:
            mean, var = x.mean((0, 1)), x.var((0, 1), unbiased=False)
            n = x.shape[0] * x.shape[1]
            new[name + ".running_mean"] = (1 - momentum) * sd[name + ".running_mean"] + momentum * mean.detach()
            new[name + ".running_var"] = (1 - momentum) * sd[name + ".running_var"] + momentum * var.detach() * n / (n - 1)
        else:
            mean, var = sd[name + ".running_mean"], sd[name + ".running_var"]
        return (x - mean) / torch.sqrt(var + eps) * sd[name + ".weight"] + sd[name + ".bias"]

    h = bn(conv(x, "fuse.0"), "fuse.1")
    h = torch.where(h > 0, h, sd["fuse.2.weight"] * h)
    h = conv(h, "fuse.3")
    h = bn(torch.relu(conv(h, "match.0")), "match.2")
    h = bn(torch.relu(conv(h, "match.3")), "match.5")
    return conv(h, "match.6").squeeze(-1), new


# --------------------------------------------------------------------------------------------- helpers
def close_out(got, ref, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    err = float(np.abs(got - ref).max())
    print("%-58s max|ref| %.3e  max err %.3e" % (what, float(np.abs(ref).max()), err))
    assert np.allclose(got, ref, rtol=1e-3, atol=1e-4), (what, err)


def close_grad(got, ref, what, scale=None):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = float(np.abs(ref).max()) if scale is None else scale
    err = float(np.abs(got - ref).max())
    print("%-58s scale %.3e  max err %.3e" % (what, scale, err))
    assert np.allclose(got, ref, rtol=5e-3, atol=1e-5 + 2e-3 * scale), (what, err, scale)


def check_param_grads(mod, ref_of, zero, what, rows=None):
    """every parameter gradient of a ScanReferMatchModule against ref_of(name); `zero`: the mathematically zero ones"""
    grads = dict(mod.named_parameters())
    assert set(grads) == set(PARAMS)
    for n in PARAMS:
        assert grads[n].grad is not None, n
        got = grads[n].grad.detach().cpu().numpy()
        ref = np.asarray(ref_of(n), np.float64)
        if rows is not None and got.ndim >= 2:
            got = got[:rows]
        scale = None
        if n in zero:
            scale = float(np.abs(np.asarray(ref_of(n[:-len("bias")] + "weight"), np.float64)).max())
        close_grad(got, ref, "%s grad %s" % (what, n), scale)


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(HERE, "golden", "scanrefer_match_golden.npz"))
    return {k: g[k] for k in g.files}


def _listener(golden, dev, Cn=4):
    from gen_scanrefer_match_golden import scanrefer_cfg, scanrefer_weights
    from d3net_amd.listener import ListenerNet
    net = ListenerNet(scanrefer_cfg(Cn))
    net.load_state_dict(scanrefer_weights(net.state_dict(), int(golden["salt"])))
    for m in net.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    return net.to(dev)


def _check_stats(mod, golden, prefix, what, expect_nbt):
    for bn in BNS:
        for s in ("running_mean", "running_var"):
            close_out(getattr(mod.get_submodule(bn), s).cpu().numpy(), golden["%s/stat/match.%s.%s" % (prefix, bn, s)], "%s %s.%s" % (what, bn, s))
        assert int(mod.get_submodule(bn).num_batches_tracked) == expect_nbt == int(golden["%s/stat/match.%s.num_batches_tracked" % (prefix, bn)])


# ------------------------------------------------------------------------------------ golden, module level
@pytest.mark.parametrize("mode", ["eval", "train"])
def test_module_matches_reference_golden(dev, golden, mode):
    from gen_listener_golden import listener_inputs
    from d3net_amd.listener import get_grounding_loss
    net = _listener(golden, dev)
    mod = net.match.train(mode == "train")
    before = {k: v.clone() for k, v in mod.state_dict().items()}
    d = {k: torch.from_numpy(v).to(dev) for k, v in listener_inputs().items()}
    d["proposal_feats_batched"].requires_grad_(True)
    d["lang_emb"] = torch.from_numpy(golden[mode + "/lang_emb"].astype(np.float32)).to(dev).requires_grad_(True)
    feats, lang = d["proposal_feats_batched"], d["lang_emb"]
    d = mod(d)
    assert "random" not in d
    close_out(d["cluster_ref"].detach().cpu().numpy(), golden[mode + "/cluster_ref"], mode + " cluster_ref")
    _, d = get_grounding_loss(d)
    close_out(d["ref_loss"].item(), golden[mode + "/ref_loss"], mode + " ref_loss")
    d["ref_loss"].backward()
    check_param_grads(mod, lambda n: golden["%s/grad/match.%s" % (mode, n)], ZERO_TRAIN_RANKING if mode == "train" else ZERO_EVAL_RANKING,
                      mode, rows=32)
    close_grad(feats.grad.cpu().numpy(), golden[mode + "/grad/proposal_feats_batched"], mode + " grad proposal_feats_batched")
    close_grad(lang.grad.cpu().numpy(), golden[mode + "/grad_ref/lang_emb"], mode + " grad lang_emb")
    if mode == "train":
        _check_stats(mod, golden, "train", "train", 1)
    else:
        for k, v in mod.state_dict().items():
            assert torch.equal(v, before[k]), k


def test_module_rl_matches_reference_golden(dev, golden):
    from gen_scanrefer_match_golden import rl_inputs
    net = _listener(golden, dev, Cn=1)
    mod = net.match.train()
    inp = rl_inputs()
    feats = torch.from_numpy(inp["proposal_feats_batched"]).to(dev).requires_grad_(True)
    sampled = torch.from_numpy(inp["sampled"]).to(dev).requires_grad_(True)
    d = {"proposal_feats_batched": feats, "proposal_batch_mask": torch.from_numpy(inp["proposal_batch_mask"]).to(dev),
         "lang_emb": {"sampled": sampled, "baseline": torch.from_numpy(inp["baseline"]).to(dev)}, "sampled_topn": inp["sampled_topn"]}
    d = mod(d, use_rl=True)
    s, b = d["cluster_ref"]["sampled"], d["cluster_ref"]["baseline"]
    assert s.requires_grad and not b.requires_grad
    close_out(s.detach().cpu().numpy(), golden["rl/sampled"], "rl sampled")
    close_out(b.cpu().numpy(), golden["rl/baseline"], "rl baseline")
    (s ** 2).sum().backward()
    check_param_grads(mod, lambda n: golden["rl/grad/match." + n], ZERO_TRAIN, "rl", rows=32)
    close_grad(feats.grad.cpu().numpy(), golden["rl/grad/proposal_feats_batched"], "rl grad proposal_feats_batched")
    close_grad(sampled.grad.cpu().numpy(), golden["rl/grad/lang_emb"], "rl grad lang_emb")
    _check_stats(mod, golden, "rl", "rl", 2)


# ---------------------------------------------------------------------------------- golden, listener level
@pytest.mark.parametrize("mode", ["eval", "train"])
def test_listener_matches_reference_golden(dev, golden, mode):
    from gen_listener_golden import listener_inputs
    from gen_scanrefer_match_golden import METRICS
    from d3net_amd.listener import get_grounding_loss, get_lobjcls_loss
    net = _listener(golden, dev).train(mode == "train")
    d = {k: torch.from_numpy(v).to(dev) for k, v in listener_inputs().items()}
    d["proposal_feats_batched"].requires_grad_(True)
    feats = d["proposal_feats_batched"]
    d["istrain"] = torch.tensor([1 if mode == "train" else 0])
    d = net(d)
    _, d = get_grounding_loss(d)
    _, d = get_lobjcls_loss(d)
    for k in ("cluster_ref", "lang_emb", "cluster_labels", "ref_loss", "lang_loss") + METRICS:
        close_out(d[k].detach().cpu().numpy(), golden["%s/%s" % (mode, k)], "%s %s" % (mode, k))
    (d["ref_loss"] + d["lang_loss"]).backward()
    check_param_grads(net.match, lambda n: golden["%s/grad/match.%s" % (mode, n)], ZERO_TRAIN_RANKING if mode == "train" else ZERO_EVAL_RANKING,
                      mode + " listener", rows=32)
    close_grad(net.lang.gru.weight_hh_l0.grad.cpu().numpy()[:32], golden[mode + "/grad/lang.gru.weight_hh_l0"], mode + " grad gru.weight_hh_l0")
    close_grad(feats.grad.cpu().numpy(), golden[mode + "/grad/proposal_feats_batched"], mode + " listener grad proposal_feats_batched")
    if mode == "train":
        _check_stats(net.match, golden, "train", "train listener", 1)


# ------------------------------------------------------------------------- ragged shapes against `compose`
def _ragged_case(dev, B, Cn, K, m, seed):
    """module with random parameters and statistics, inputs with one scene without a valid proposal and one with all valid"""
    import types
    from d3net_amd.listener import ScanReferMatchModule
    ns = types.SimpleNamespace
    g = torch.Generator().manual_seed(seed)
    mod = ScanReferMatchModule(ns(model=ns(max_num_proposal=K, m=m), data=ns(num_des_per_scene=Cn)))
    with torch.no_grad():
        for n, p in mod.named_parameters():
            if p.dim() == 1 and n.endswith("weight"):
                p.copy_(1 + 0.2 * torch.randn(p.shape, generator=g))
            elif p.dim() == 1:
                p.copy_(0.2 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(torch.randn(p.shape, generator=g) / p.shape[1] ** 0.5)
        for n, b in mod.named_buffers():
            if n.endswith("running_mean"):
                b.copy_(0.2 * torch.randn(b.shape, generator=g))
            elif n.endswith("running_var"):
                b.copy_(0.5 + torch.rand(b.shape, generator=g))
    mask = torch.rand(B, K, generator=g) > 0.5
    mask[0] = False                 # no valid proposal (the only scene of a one-scene case keeps its random mask)
    if B > 1:
        mask[1] = True              # all valid
    else:
        mask[0] = torch.rand(K, generator=g) > 0.5
    feats = torch.randn(B, K, m, generator=g)
    lang = torch.randn(B * Cn, 256, generator=g)
    w = torch.randn(B * Cn, K, generator=g)
    return mod.to(dev), feats.to(dev), lang.to(dev), mask.to(dev), w.to(dev)


@pytest.mark.parametrize("mode", ["eval", "train"])
@pytest.mark.parametrize("shape", [(3, 2, 40, 8), (1, 1, 16, 16), (2, 4, 72, 4)], ids=lambda s: "x".join(map(str, s)))
def test_ragged_shapes_match_float64_composition(dev, shape, mode):
    B, Cn, K, m = shape
    train = mode == "train"
    mod, feats, lang, mask, w = _ragged_case(dev, B, Cn, K, m, seed=7)
    mod.train(train)
    sd64 = {k: v.detach().double().clone().requires_grad_(v.dtype.is_floating_point and "running" not in k) for k, v in mod.state_dict().items()}
    f64, l64 = feats.double().requires_grad_(True), lang.double().requires_grad_(True)
    ref, new = compose(f64, l64, mask.double(), Cn, sd64, train)
    (ref * w.double()).sum().backward()
    feats.requires_grad_(True)
    lang.requires_grad_(True)
    out = mod({"proposal_feats_batched": feats, "lang_emb": lang, "proposal_batch_mask": mask})["cluster_ref"]
    assert out.shape == (B * Cn, K)
    close_out(out.detach().cpu().numpy(), ref.detach().cpu().numpy(), "%s %s cluster_ref" % (shape, mode))
    (out * w).sum().backward()
    check_param_grads(mod, lambda n: sd64[n].grad.cpu().numpy(), ZERO_TRAIN if train else (), "%s %s" % (shape, mode))
    close_grad(feats.grad.cpu().numpy(), f64.grad.cpu().numpy(), "%s %s grad feats" % (shape, mode))
    close_grad(lang.grad.cpu().numpy(), l64.grad.cpu().numpy(), "%s %s grad lang" % (shape, mode))
    for bn in BNS:
        for s in ("running_mean", "running_var"):
            k = "%s.%s" % (bn, s)
            close_out(mod.state_dict()[k].cpu().numpy(), (new[k] if train else sd64[k]).detach().cpu().numpy(), "%s %s %s" % (shape, mode, k))
        assert int(mod.get_submodule(bn).num_batches_tracked) == int(train)


# ---------------------------------------------------------------------------------------- determinism
def test_two_training_runs_are_bit_identical(dev):
    res = []
    for _ in range(2):
        mod, feats, lang, mask, w = _ragged_case(dev, 3, 2, 40, 8, seed=3)
        mod.train()
        feats.requires_grad_(True)
        lang.requires_grad_(True)
        out = mod({"proposal_feats_batched": feats, "lang_emb": lang, "proposal_batch_mask": mask})["cluster_ref"]
        (out * w).sum().backward()
        torch.cuda.synchronize()
        res.append([out.detach(), feats.grad, lang.grad] + [p.grad for _, p in sorted(mod.named_parameters())] +
                   [b for _, b in sorted(mod.named_buffers())])
    assert len(res[0]) == 3 + 17 + 9
    for a, b in zip(*res):
        assert torch.equal(a, b)
