"""d3net_amd.trainer.Trainer on the device: a mode-0 PipelineNet on the scene of tests/test_config0_step_gpu.py (2 epochs of 2
steps, 2 validation batches, monitor val_loss/total_loss) -- the epoch means of metrics.jsonl equal the float64 means of the
per-step values with ==, both checkpoints load into a fresh model bit for bit -- and a shorter mode-2 run for the
([optimizer], [scheduler]) return and a val_score/... monitor."""
import json
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _capture(model):
    """wrap training_step / validation_step: after each call read `model.logged` back (the test's own read-back) -> the lists"""
    seen = {"train": [], "val": [], "state": []}
    t_step, v_step, v_end = model.training_step, model.validation_step, model.validation_epoch_end

    def read():
        return {k: float(v.double()) if torch.is_tensor(v) else float(v) for k, v in model.logged.items()}

    def training_step(batch, idx=0):
        out = t_step(batch, idx)
        seen["train"].append((model.current_epoch, read()))
        return out

    def validation_step(batch, idx=0, dataloader_idx=0):
        out = v_step(batch, idx, dataloader_idx)
        seen["val"].append((model.current_epoch, read()))
        return out

    def validation_epoch_end(outputs):
        seen["state"].append({k: v.detach().clone() for k, v in model.state_dict().items()})    # what this epoch's checkpoint holds
        return v_end(outputs)
    model.training_step, model.validation_step, model.validation_epoch_end = training_step, validation_step, validation_epoch_end
    return seen


def _mean64(values):
    """the record's arithmetic: one float64 addition per step in step order, then one division"""
    acc, w = np.float64(0.0), np.float64(0.0)
    for v in values:
        acc = acc + np.float64(1.0) * np.float64(v)
        w = w + np.float64(1.0)
    return float(acc / w)


def _epoch_records(root):
    with open(os.path.join(root, "logs", "metrics.jsonl")) as f:
        return [r for r in map(json.loads, f) if r["kind"] == "epoch"]


def _assert_loads_bit_equal(make_model, path, state):
    from d3net_amd.checkpoint import load_lightning_checkpoint
    fresh = make_model()
    load_lightning_checkpoint(fresh, path, strict=True)
    got = fresh.state_dict()
    assert set(got) == set(state)
    for k, v in state.items():
        assert torch.equal(got[k].cpu(), v.cpu()), k


def test_fit_mode0_epoch_means_and_checkpoints(dev, tmp_path):
    from d3net_amd import synthetic as S
    from d3net_amd.config import default_conf
    from d3net_amd.pipeline import PipelineNet
    from d3net_amd.trainer import Batches, Trainer
    root = str(tmp_path)
    cfg = default_conf(overrides={"general": {"root": root}, "train": {"epochs": 2, "num_sanity_val_steps": 1, "log_every_n_steps": 1}})
    assert cfg.general.monitor == "val_loss/total_loss" and cfg.general.monitor_mode == "min"

    def make_model():
        torch.manual_seed(cfg.general.manual_seed)
        net = PipelineNet(cfg).to(dev)
        net.detector.teacher = True
        return net
    model = make_model()
    assert model.mode == 0
    occ, sem, inst, _ = S.occupancy_grid((120, 90, 60), 6, (10, 34), (10, 28), 0)          # test_config0_step_gpu.py's scene
    batches = [S.make_batch([S.scene_from_grid(occ, sem, inst, feat_seed=2 + k)], dev) for k in range(2)]
    seen = _capture(model)
    tr = Trainer(cfg, model).fit(Batches(batches), Batches(batches))
    assert tr.global_step == 4 and tr.validated_epochs == [0, 1] and tr.sanity_steps_run == 1
    val = seen["val"][1:]                                  # (the first validation call was the sanity step)
    assert len(seen["train"]) == 4 and len(val) == 4
    ep = _epoch_records(root)
    assert [r["epoch"] for r in ep] == [0, 1]
    for e, r in enumerate(ep):
        steps = [d for ce, d in seen["train"] if ce == e]
        vsteps = [d for ce, d in val if ce == e][-2:]
        assert len(steps) == 2 and len(vsteps) == 2 and "train/total_loss" in steps[0] and "val_loss/total_loss" in vsteps[0]
        for k in steps[0]:
            assert r[k] == _mean64([d[k] for d in steps]), (e, k)
        for k in vsteps[0]:
            assert r[k] == _mean64([d[k] for d in vsteps]), (e, k)
        assert np.isfinite(r["train/total_loss"]) and "nonfinite" not in r
    scores = [r["val_loss/total_loss"] for r in ep]
    best = int(np.argmin(scores))
    assert tr.best_epoch == best and tr.best_score == scores[best]
    last = torch.load(os.path.join(root, "last.ckpt"), map_location="cpu")
    assert last["epoch"] == 1 and last["global_step"] == 4 and len(last["optimizer_states"]) == 1
    assert torch.load(os.path.join(root, "model.ckpt"), map_location="cpu")["epoch"] == best
    _assert_loads_bit_equal(make_model, os.path.join(root, "last.ckpt"), seen["state"][-1])
    _assert_loads_bit_equal(make_model, os.path.join(root, "model.ckpt"), seen["state"][1 + best])     # [0] is the sanity round's
    for k, v in model.state_dict().items():                # the last checkpoint is the model as fit() left it
        assert torch.equal(v.cpu(), last["state_dict"][k]), k


def test_fit_mode2_scheduler_and_score_monitor(dev, tmp_path):
    from d3net_amd import synthetic as S
    from d3net_amd.config import default_conf
    from d3net_amd.pipeline import PipelineNet
    from d3net_amd.trainer import Batches, Trainer
    root = str(tmp_path)
    V = 200
    cfg = default_conf(overrides={
        "general": {"root": root, "monitor": "val_score/ref_iou_rate_0.5", "monitor_mode": "max"},
        "model": {"blocks": [1, 2, 3], "num_graph_steps": 2, "num_locals": 10, "use_relation": True, "use_orientation": True,
                  "match_type": "Transformer", "use_lang_classifier": True, "use_bidir": False, "num_bbox_class": 18,
                  "loss_type": "cross_entropy", "no_captioning": True, "no_grounding": False},
        "data": {"num_des_per_scene": 4, "max_spk_len": 30, "max_lis_len": 126, "min_iou_threshold": 0.25, "num_ori_bins": 6},
        "train": {"use_rl": False, "sample_topn": 1, "epochs": 1, "num_sanity_val_steps": 0, "log_every_n_steps": 1}})
    ds = {"train": types.SimpleNamespace(vocabulary=S.make_vocabulary(V), glove=np.random.default_rng(0).standard_normal((V, 300)).astype(np.float32))}
    torch.manual_seed(cfg.general.manual_seed)
    model = PipelineNet(cfg, ds).to(dev)
    model.detector.teacher = True
    assert model.mode == 2
    scenes = [S.small_scene(dims=(40, 32, 20), n_boxes=3, seed=s) for s in (3, 4)]
    batch = S.add_language(S.make_batch(scenes, dev), dev, chunk=4, vocab=V)
    seen = _capture(model)
    tr = Trainer(cfg, model).fit(Batches([batch, batch]), Batches([batch]))
    assert len(tr.optimizers) == 1 and len(tr.schedulers) == 1 and tr.schedulers[0].last_epoch == 1 and tr.global_step == 2
    ep = _epoch_records(root)
    assert len(ep) == 1
    for k in seen["train"][0][1]:
        assert ep[0][k] == _mean64([d[k] for _e, d in seen["train"]]), k
    for k, v in seen["val"][0][1].items():
        assert ep[0][k] == v, k
    assert tr.best_epoch == 0 and tr.best_score == ep[0]["val_score/ref_iou_rate_0.5"] and 0.0 <= tr.best_score <= 1.0
    last = torch.load(os.path.join(root, "last.ckpt"), map_location="cpu")
    assert len(last["lr_schedulers"]) == 1 and last["lr_schedulers"][0]["last_epoch"] == 1
    assert os.path.exists(os.path.join(root, "model.ckpt"))
