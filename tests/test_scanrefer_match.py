"""The ScanRefer matcher's host side (d3net_amd.listener.ScanReferMatchModule; reference model/match_module.py:11-141,
model/listener.py:25-32): construction, state-dict layout against the reference's (tests/golden/scanrefer_match_golden.npz),
and the checks that raise before anything is launched.  No GPU."""
import os
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(HERE, "golden", "scanrefer_match_golden.npz"))
    return {k: g[k] for k in g.files}


def test_listener_builds_the_scanrefer_matcher_with_the_reference_state_dict(golden):
    from gen_scanrefer_match_golden import scanrefer_cfg, scanrefer_weights
    from d3net_amd.listener import ListenerNet, ScanReferMatchModule
    net = ListenerNet(scanrefer_cfg())
    assert isinstance(net.match, ScanReferMatchModule)
    sd = net.state_dict()
    keys = [k for k in sd if k.startswith("match.")]
    assert keys == [str(k) for k in golden["match_keys"]]
    assert [",".join(str(s) for s in sd[k].shape) for k in keys] == [str(s) for s in golden["match_shapes"]]
    assert (net.match.num_proposals, net.match.lang_size, net.match.hidden_size, net.match.det_channel, net.match.chunk_size) == (128, 256, 128, 16, 4)
    res = net.load_state_dict(scanrefer_weights(sd, int(golden["salt"])), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert float(net.match.fuse[1].running_var.min()) >= 0.5


def test_unknown_match_type_still_raises():
    from gen_scanrefer_match_golden import scanrefer_cfg
    from d3net_amd.listener import ListenerNet
    cfg = scanrefer_cfg()
    cfg.model.match_type = "VoteNet"
    with pytest.raises(NotImplementedError):
        ListenerNet(cfg)


def test_rl_with_two_descriptions_per_scene_raises_on_the_host():
    """model/match_module.py:69 asserts features_exp.shape[0] == sampled_feat.shape[0]: true for one description per scene only"""
    from gen_scanrefer_match_golden import scanrefer_cfg
    from d3net_amd.listener import ScanReferMatchModule
    mod = ScanReferMatchModule(scanrefer_cfg(2))
    B, topn, K = 2, 3, 128
    d = {"proposal_feats_batched": torch.zeros(B, K, 16), "proposal_batch_mask": torch.ones(B, K), "sampled_topn": topn,
         "lang_emb": {"sampled": torch.zeros(B * topn * 2, 256), "baseline": torch.zeros(B * topn * 2, 256)}}
    with pytest.raises(ValueError, match="sampled_topn"):
        mod(d, use_rl=True)


def test_unsupported_inputs_raise_before_any_launch():
    from gen_scanrefer_match_golden import scanrefer_cfg
    from d3net_amd.listener import ScanReferMatchModule
    mod = ScanReferMatchModule(scanrefer_cfg(1))
    d = {"proposal_feats_batched": torch.zeros(2, 128, 16), "proposal_batch_mask": torch.ones(2, 128), "lang_emb": torch.zeros(2, 256)}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mod(dict(d))
    ns = types.SimpleNamespace
    with pytest.raises(NotImplementedError, match="hidden_size"):
        ScanReferMatchModule(scanrefer_cfg(1), hidden_size=64)(dict(d))
    odd = ScanReferMatchModule(ns(model=ns(max_num_proposal=128, m=6), data=ns(num_des_per_scene=1)))
    with pytest.raises((ValueError, RuntimeError)):
        odd({"proposal_feats_batched": torch.zeros(2, 128, 6), "proposal_batch_mask": torch.ones(2, 128), "lang_emb": torch.zeros(2, 256)})


def test_fixture_meets_the_argmax_condition(golden):
    """every sample's argmax on a valid proposal with top-1 - top-2 >= 0.01 in the float64 reference, both modes: the accuracy and
    IoU metrics of the fixture do not hang on how ties are broken"""
    assert float(golden["min_margin"]) >= 0.01
    valid = np.repeat(golden["valid_mask"], 4, axis=0) > 0
    for mode in ("eval", "train"):
        ref = golden[mode + "/cluster_ref"]
        assert valid[np.arange(ref.shape[0]), ref.argmax(1)].all()
        top = np.sort(ref, axis=1)
        assert float((top[:, -1] - top[:, -2]).min()) >= 0.01
        assert abs(float((top[:, -1] - top[:, -2]).min()) - float(golden[mode + "/min_margin"])) < 1e-12
