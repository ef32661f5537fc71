"""d3net_amd.trainer.Trainer and d3net_amd.metric_log.MetricLog on the host: a small stub module with the hooks of PipelineNet on host
tensors (MetricLog's host arm: float64, one multiplication and one addition per call).  Validation cadence, sanity steps, the
monitored checkpoints, the scheduler's interval, resume, the log file, and the packed all-reduce over two gloo ranks."""
import json
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from d3net_amd.config import _wrap


class Stub(torch.nn.Module):
    """the hooks the trainer drives, on host tensors; `val_losses[e]` is what validation reports in its e-th validated epoch"""

    def __init__(self, val_losses=(), val_key="val_loss/total_loss", bare=False, sched_step=1):
        super().__init__()
        self.lin = torch.nn.Linear(3, 1)
        self.logged, self.current_epoch, self.global_step = {}, 0, 0
        self.val_losses, self.val_key, self.bare, self.sched_step = list(val_losses), val_key, bare, sched_step
        self.val_calls, self.val_epochs_seen, self.val_rounds, self.epoch_end_outputs = [], [], 0, []
        self.train_epochs_seen, self.train_values = [], []

    def log(self, name, value):
        self.logged[name] = value.detach() if torch.is_tensor(value) else value

    def configure_optimizers(self):
        opt = torch.optim.AdamW(self.parameters(), lr=0.5)
        if self.bare:
            return [opt]
        return [opt], [torch.optim.lr_scheduler.StepLR(opt, step_size=self.sched_step, gamma=0.5)]

    def training_step(self, batch, idx=0):
        self.logged = {}
        loss = self.lin(batch["x"]).pow(2).mean()
        self.log("train/total_loss", loss)
        self.log("train/idx", idx)                           # a Python number
        self.train_epochs_seen.append(self.current_epoch)
        self.train_values.append(float(loss.detach().double()))
        self.global_step += 1
        return loss, batch

    def validation_step(self, batch, idx=0, dataloader_idx=0):
        self.val_calls.append((self.val_rounds, idx))
        v = batch["v"] + (self.val_losses[min(self.val_rounds, len(self.val_losses) - 1)] if self.val_losses else 0.0)
        self.log(self.val_key, torch.tensor(v, dtype=torch.float32))
        return {"idx": idx}

    def validation_epoch_end(self, outputs):
        self.epoch_end_outputs.append(outputs)
        self.val_epochs_seen.append(self.current_epoch)
        self.val_rounds += 1
        self.log("val_score/at_end", 0.125 * self.val_rounds)
        return {}


def _cfg(root, **train):
    t = dict(epochs=4, check_val_every_n_epoch=1, num_sanity_val_steps=0, log_every_n_steps=1)
    t.update(train)
    return _wrap({"general": {"monitor": "val_loss/total_loss", "monitor_mode": "min", "root": str(root), "output_root": str(root),
                              "experiment": "stub"}, "train": t, "model": {"use_checkpoint": None}})


def _batches(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [{"x": torch.randn(4, 3, generator=g)} for _ in range(n)]


VAL = [{"v": 0.25}, {"v": 0.5}, {"v": 1.0}]      # dyadic: their float64 means are exact in any order


def _records(root, kind):
    with open(os.path.join(str(root), "logs", "metrics.jsonl")) as f:
        return [r for r in map(json.loads, f) if r["kind"] == kind]


def test_validation_cadence(tmp_path):
    from d3net_amd.trainer import Trainer
    m = Stub()
    tr = Trainer(_cfg(tmp_path, check_val_every_n_epoch=2), m).fit(_batches(2), VAL)
    assert tr.validated_epochs == [1, 3] and m.val_epochs_seen == [1, 3]
    assert m.train_epochs_seen == [0, 0, 1, 1, 2, 2, 3, 3]          # current_epoch is set before the epoch's first step
    assert [len(o) for o in m.epoch_end_outputs] == [3, 3] and m.epoch_end_outputs[0][2] == {"idx": 2}
    assert m.training                                                # validation leaves the module in training mode
    ep = _records(tmp_path, "epoch")
    assert ["val_loss/total_loss" in r for r in ep] == [False, True, False, True]


@pytest.mark.parametrize("n, want", [(0, 0), (2, 2), (-1, 3)])
def test_sanity_steps(tmp_path, n, want):
    from d3net_amd.trainer import Trainer
    m = Stub(val_losses=[100.0, 0.0])                # the sanity round reports values 100 higher than epoch 0's
    tr = Trainer(_cfg(tmp_path, epochs=1, num_sanity_val_steps=n), m).fit(_batches(2), VAL)
    assert tr.sanity_steps_run == want
    sanity_calls = [c for c in m.val_calls if c[0] == 0] if n else []
    assert len(sanity_calls) == want
    ep = _records(tmp_path, "epoch")
    assert len(ep) == 1
    base = 0.0 if n else 100.0                        # (without a sanity round, round 0 IS epoch 0)
    assert ep[0]["val_loss/total_loss"] == base + float(np.mean([0.25, 0.5, 1.0], dtype=np.float64))
    assert ep[0]["val_score/at_end"] == 0.125 * (2 if n else 1)


@pytest.mark.parametrize("mode, losses, best", [("min", [3.0, 1.0, 2.0, 1.0], 1), ("max", [1.0, 3.0, 2.0, 3.0], 1),
                                                ("min", [3.0, 2.0, 1.0, 0.5], 3)])
def test_monitor_selects_the_epoch(tmp_path, mode, losses, best):
    from d3net_amd.trainer import Trainer
    cfg = _cfg(tmp_path)
    cfg.general.monitor_mode = mode
    m = Stub(val_losses=losses)
    seen = []
    orig = Trainer._save

    def spy(self, state, name):
        seen.append((name, state["epoch"]))
        return orig(self, state, name)
    Trainer._save = spy
    try:
        tr = Trainer(cfg, m).fit(_batches(1), VAL[:1])
    finally:
        Trainer._save = orig
    assert tr.best_epoch == best and tr.best_score == losses[best] + 0.25
    model_ckpt = torch.load(os.path.join(str(tmp_path), "model.ckpt"))
    last_ckpt = torch.load(os.path.join(str(tmp_path), "last.ckpt"))
    assert model_ckpt["epoch"] == best and last_ckpt["epoch"] == 3
    assert [e for n, e in seen if n == "last.ckpt"] == [0, 1, 2, 3]          # rewritten after every validated epoch
    assert last_ckpt["callbacks"]["ModelCheckpoint"]["best_model_score"] == losses[best] + 0.25
    for k in ("epoch", "global_step", "state_dict", "optimizer_states", "lr_schedulers"):
        assert k in last_ckpt, k
    from d3net_amd.checkpoint import load_lightning_checkpoint
    fresh = Stub()
    load_lightning_checkpoint(fresh, os.path.join(str(tmp_path), "last.ckpt"), strict=True)
    for a, b in zip(fresh.parameters(), m.parameters()):
        assert torch.equal(a, b)


def test_missing_monitor_names_the_available_keys(tmp_path):
    from d3net_amd.trainer import Trainer
    cfg = _cfg(tmp_path, epochs=1)
    cfg.general.monitor = "val_score/ref_iou_rate_0.5"
    with pytest.raises(ValueError) as e:
        Trainer(cfg, Stub()).fit(_batches(1), VAL)
    assert "val_score/ref_iou_rate_0.5" in str(e.value) and "val_loss/total_loss" in str(e.value) and "val_score/at_end" in str(e.value)


def test_scheduler_steps_once_per_epoch_and_bare_optimizer_list(tmp_path):
    from d3net_amd.trainer import Trainer
    tr = Trainer(_cfg(tmp_path / "a", epochs=3), Stub()).fit(_batches(5), VAL)
    assert tr.schedulers[0].last_epoch == 3 and tr.optimizers[0].param_groups[0]["lr"] == 0.5 * 0.5 ** 3
    assert tr.global_step == 15
    tr = Trainer(_cfg(tmp_path / "b", epochs=2), Stub(bare=True)).fit(_batches(2), VAL)
    assert tr.schedulers == [] and tr.optimizers[0].param_groups[0]["lr"] == 0.5 and tr.global_step == 4


def test_resume_from_last_ckpt(tmp_path):
    from d3net_amd.trainer import Trainer
    m = Stub(val_losses=[2.0, 1.0])
    tr = Trainer(_cfg(tmp_path, epochs=2), m).fit(_batches(3), VAL)
    lr = tr.optimizers[0].param_groups[0]["lr"]
    steps = [float(s["step"]) for s in tr.optimizers[0].state_dict()["state"].values()]
    assert lr == 0.125 and steps == [6.0, 6.0]
    m2 = Stub(val_losses=[5.0])
    tr2 = Trainer(_cfg(tmp_path, epochs=2), m2)
    tr2._configure()
    tr2._logs()
    assert tr2._resume(os.path.join(str(tmp_path), "last.ckpt")) == 2           # the checkpoint's epoch + 1
    assert tr2.global_step == 6 and m2.global_step == 6 and tr2.best_score == 4.75 / 3 and tr2.best_epoch == 1
    assert tr2.optimizers[0].param_groups[0]["lr"] == lr and tr2.schedulers[0].last_epoch == 2
    assert [float(s["step"]) for s in tr2.optimizers[0].state_dict()["state"].values()] == steps
    for a, b in zip(m2.parameters(), m.parameters()):
        assert torch.equal(a, b)
    # through fit(): one more epoch continues at epoch 2 with step 7; a worse score leaves model.ckpt alone
    m3 = Stub(val_losses=[5.0])
    cfg = _cfg(tmp_path, epochs=3, num_sanity_val_steps=-1)
    tr3 = Trainer(cfg, m3).fit(_batches(3), VAL, ckpt_path=os.path.join(str(tmp_path), "last.ckpt"))
    assert m3.train_epochs_seen == [2, 2, 2] and tr3.global_step == 9 and tr3.sanity_steps_run == 0
    assert tr3.best_epoch == 1 and torch.load(os.path.join(str(tmp_path), "model.ckpt"))["epoch"] == 1
    assert torch.load(os.path.join(str(tmp_path), "last.ckpt"))["epoch"] == 2
    # model.use_checkpoint resolves to <output_root>/<use_checkpoint>/last.ckpt
    run = tmp_path / "RUN"
    run.mkdir()
    os.replace(os.path.join(str(tmp_path), "last.ckpt"), str(run / "last.ckpt"))
    cfg = _cfg(tmp_path, epochs=3)
    cfg.model.use_checkpoint = "RUN"
    tr4 = Trainer(cfg, Stub())
    tr4._configure()
    assert tr4._resume(None) == 3 and tr4.global_step == 9


def test_log_file(tmp_path):
    from d3net_amd.trainer import Trainer
    m = Stub()
    Trainer(_cfg(tmp_path, epochs=3, log_every_n_steps=2), m).fit(_batches(4), VAL)
    ep = _records(tmp_path, "epoch")
    assert [r["epoch"] for r in ep] == [0, 1, 2] and [r["global_step"] for r in ep] == [4, 8, 12]
    for e, r in enumerate(ep):
        assert {"train/total_loss", "train/idx", "val_loss/total_loss", "val_score/at_end"} <= set(r)
        vals = m.train_values[4 * e:4 * e + 4]
        acc = np.float64(0.0)
        for v in vals:                                   # the host arm's arithmetic: one float64 addition per step, in order
            acc = acc + np.float64(1.0) * np.float64(v)
        assert r["train/total_loss"] == float(acc / np.float64(4.0))
        assert r["train/idx"] == 1.5
    st = _records(tmp_path, "step")
    assert st and all("train/total_loss" in r and r["global_step"] % 2 == 0 for r in st)


def test_metric_log_host_arm():
    from d3net_amd.metric_log import MetricLog
    log = MetricLog()
    log.update({"a": 1.5, "b": torch.tensor(2, dtype=torch.int64)}, weight=2.0)
    log.update({"a": 0.5}, weight=0.5)
    log.update({"a": float("nan"), "c": torch.tensor(0.25)})
    assert log.counts() == {"a": 3, "b": 1, "c": 1} and log.nonfinite() == {"a": 1}
    got = log.compute()
    assert np.isnan(got["a"]) and got["b"] == 2.0 and got["c"] == 0.25
    assert log.last()["b"] == 2.0 and np.isnan(log.last()["a"])
    assert log.snapshot(tag=5) is None                                             # nothing earlier to hand out
    log.update({"b": 4.0})
    snap = log.snapshot(tag=7)
    assert snap["b"] == 2.0 and snap["c"] == 0.25 and log.snapshot_tag == 5        # the records as they were at tag 5
    log.reset()
    assert log.compute() == {} and log.snapshot() is None                          # pre-reset snapshots are not handed out
    assert log.snapshot() == {}
    log.update({"a": 3.0})
    assert log.compute() == {"a": 3.0} and list(log.counts()) == ["a", "b", "c"]


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def _values(rank):
    return [0.25 * (1 + rank) + 0.5 * k for k in range(3 + rank)]      # dyadic, a different count per rank


def _log_worker(rank, world, port, ret):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from d3net_amd.metric_log import MetricLog
    log = MetricLog()
    for k, v in enumerate(_values(rank)):
        log.update({"val_loss/total_loss": torch.tensor(v), "val_score/acc": float(v) * 2} if (k + rank) % 2 else
                   {"val_score/acc": float(v) * 2, "val_loss/total_loss": torch.tensor(v)})      # first-seen order differs per rank
    log.all_reduce()
    ret[rank] = log.compute()
    dist.barrier()
    dist.destroy_process_group()


def test_all_reduce_world2():
    """after all_reduce() both ranks' compute() equal the float64 mean over both ranks' values"""
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_log_worker, args=(2, _free_port(), ret), nprocs=2, join=True)
    both = np.array(_values(0) + _values(1), dtype=np.float64)
    for r in (0, 1):
        assert ret[r]["val_loss/total_loss"] == float(both.mean()) and ret[r]["val_score/acc"] == float((2 * both).mean())


def _fit_worker(rank, world, port, root, ret):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from d3net_amd.trainer import Trainer
    torch.manual_seed(rank)                                   # different replicas: fit() broadcasts rank 0's
    m = Stub()
    val = [{"v": 0.25 * (1 + rank)}, {"v": 0.5 * (1 + rank)}]
    tr = Trainer(_cfg(root, epochs=2), m).fit(_batches(2, seed=10 + rank), val)
    ret[rank] = dict(params=[p.detach().clone() for p in m.parameters()], train=m.train_values, best=tr.best_score)
    dist.barrier()
    dist.destroy_process_group()


def test_fit_world2(tmp_path):
    """two gloo ranks with different data: identical replicas after fit (broadcast + averaged gradients), the epoch means are the means
    over both ranks' values, and rank 0 alone writes the log and the checkpoints"""
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_fit_worker, args=(2, _free_port(), str(tmp_path), ret), nprocs=2, join=True)
    for a, b in zip(ret[0]["params"], ret[1]["params"]):
        assert torch.equal(a, b)
    assert ret[0]["train"] != ret[1]["train"]
    ep = _records(tmp_path, "epoch")
    assert [r["epoch"] for r in ep] == [0, 1]                   # one record per epoch: one writer
    for e, r in enumerate(ep):
        s0 = np.float64(ret[0]["train"][2 * e]) + np.float64(ret[0]["train"][2 * e + 1])
        s1 = np.float64(ret[1]["train"][2 * e]) + np.float64(ret[1]["train"][2 * e + 1])
        assert r["train/total_loss"] == float((s0 + s1) / np.float64(4.0))
        assert r["val_loss/total_loss"] == (0.25 + 0.5 + 0.5 + 1.0) / 4
    assert ret[0]["best"] == ret[1]["best"] == 0.5625
    assert torch.load(os.path.join(str(tmp_path), "last.ckpt"))["epoch"] == 1
