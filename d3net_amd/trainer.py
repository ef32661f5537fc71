"""`Trainer`: the fit loop Lightning's `pl.Trainer` runs for the reference (scripts/train.py:252-280,329-375), over the hooks
`PipelineNet` already has -- `configure_optimizers`, `training_step`, `validation_step`, `validation_epoch_end` -- with the
epoch means kept on the device (`d3net_amd.metric_log.MetricLog`) and `ModelCheckpoint(monitor, mode, dirpath=cfg.general.root,
filename="model", save_last=True)`'s two files.

    Trainer(cfg, model).fit(train_batches, val_batches=None, ckpt_path=None)

`train_batches` / `val_batches` are re-iterable sources of batches (lists, or objects whose `__iter__` starts a new pass); in
mode 3 a training batch is the pair `training_step` asserts and `val_batches` is a pair of sources (`dataloader_idx` 0 and 1).
A training source with a `set_epoch` method (`dataset.PipelineLoader`) gets `set_epoch(epoch)` before each pass.
Config keys read (all of them shipped by every conf/*.yaml): `train.epochs`, `train.check_val_every_n_epoch`,
`train.num_sanity_val_steps` (-1: all validation batches), `train.log_every_n_steps`, `general.monitor`,
`general.monitor_mode`, `model.use_checkpoint` (resume from `<general.output_root>/<use_checkpoint>/last.ckpt`,
scripts/train.py:332-334); the run directory is `general.root`, or `<general.output_root>/<EXPERIMENT>` as scripts/train.py:30.

Per training batch: `model.zero_grad`, `training_step`, `loss.backward()`, the gradient reducer of `d3net_amd.distributed` when a
process group with more than one rank is active, `optimizer.step()`, `MetricLog.update(model.logged)` -- one small launch and one
asynchronous copy, no host synchronisation beyond what `training_step` has.  Schedulers step once per training epoch (Lightning's
default `interval="epoch"`).  Every `log_every_n_steps` steps a `snapshot()` of the running epoch means goes to the log sink,
`<root>/logs/metrics.jsonl` (one JSON object per snapshot, `"kind": "step"`, and per epoch, `"kind": "epoch"`).

Validation runs every `check_val_every_n_epoch` epochs under `model.eval()` and `torch.no_grad()`; the epoch's metric dict is the
union of the means of what `validation_step` logged and what `validation_epoch_end` logged.  `last.ckpt` is written after every
validated epoch (after every epoch when there is no validation source), `model.ckpt` when the monitored value improves; both are dicts in Lightning's layout (`epoch`, `global_step`,
`state_dict`, `optimizer_states`, `lr_schedulers`, `callbacks["ModelCheckpoint"]` with the best score) that
`checkpoint.load_lightning_checkpoint` reads.  Resuming restores weights, optimizer and scheduler state, `epoch + 1`,
`global_step` and the best score.  With several ranks every rank runs the loop, the logs are all-reduced once per epoch (one packed
collective) and rank 0 writes the files."""
import json
import math
import os

import torch

from .metric_log import MetricLog


class Batches:
    """a re-iterable source over prepared batches: every pass hands out shallow copies (the hooks add keys to the dict they are
    given); a pair of dicts -- the joint mode's training batch -- is copied element-wise"""

    def __init__(self, batches):
        self.batches = list(batches)

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        for b in self.batches:
            yield dict(b) if isinstance(b, dict) else [dict(x) for x in b]


class Trainer:
    def __init__(self, cfg, model, root=None):
        self.cfg, self.model = cfg, model
        t, g = cfg.train, cfg.general
        self.epochs = int(t.epochs)
        self.check_val_every_n_epoch = max(1, int(t.get("check_val_every_n_epoch", 1) or 1))
        self.num_sanity_val_steps = int(t.get("num_sanity_val_steps", 0) or 0)
        self.log_every_n_steps = max(1, int(t.get("log_every_n_steps", 50) or 50))
        self.monitor = g.get("monitor") or None
        self.monitor_mode = g.get("monitor_mode") or "min"
        if self.monitor_mode not in ("min", "max"):
            raise ValueError("general.monitor_mode: %r is not min or max" % (self.monitor_mode,))
        self.root = root or g.get("root") or os.path.join(g.output_root, str(g.experiment).upper())
        self.global_step, self.current_epoch = 0, 0
        self.best_score, self.best_epoch, self.best_model_path = None, None, ""
        self.optimizers, self.schedulers = [], []
        self.train_log = self.val_log = None
        self.validated_epochs, self.sanity_steps_run = [], 0
        self.last_metrics = {}

    # ------------------------------------------------------------------------------------------------- pieces
    def _configure(self):
        """`configure_optimizers()` once: `([optimizers], [schedulers])`, a bare `[optimizer]` or one optimizer"""
        out = self.model.configure_optimizers()
        scheds = []
        if isinstance(out, tuple) and len(out) == 2 and isinstance(out[0], (list, tuple)):
            opts, scheds = list(out[0]), list(out[1])
        elif isinstance(out, (list, tuple)):
            opts = list(out)
        else:
            opts = [out]
        self.optimizers, self.schedulers = opts, scheds

    def _logs(self):
        """the training and the validation table: on a device model two halves of ONE record buffer"""
        p = next(self.model.parameters(), None)
        if p is not None and p.is_cuda:
            from .metric_log import CAPACITY
            buf = MetricLog.allocate(p.device, 2 * CAPACITY)
            self.train_log, self.val_log = MetricLog(records=buf, offset=0), MetricLog(records=buf, offset=CAPACITY)
        else:
            self.train_log, self.val_log = MetricLog(), MetricLog()

    def _reducer(self):
        """the gradient reducer, built as bench.py's multi-rank path builds it (None without a process group of several ranks)"""
        from . import distributed as D
        if not D._dist_active():
            return None
        model = self.model
        D.broadcast_module(model)       # identical replicas
        params = [p for p in model.parameters() if p.requires_grad]
        det = getattr(model, "detector", None)
        if det is None or not hasattr(det, "static_gradient_buckets"):
            return D.FlatGradAllReduce(params)
        det_ids = {id(p) for p in det.parameters()}
        sync = D.BucketGradAllReduce(params, det, early=[p for p in params if id(p) not in det_ids])
        model.grad_boundary = sync
        return sync

    @staticmethod
    def _rank():
        import torch.distributed as dist
        return dist.get_rank() if dist.is_available() and dist.is_initialized() else 0

    def _sink(self, record):
        if self._rank() != 0:
            return
        d = os.path.join(self.root, "logs")
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "metrics.jsonl"), "a") as f:
            f.write(json.dumps(record) + "\n")

    # ------------------------------------------------------------------------------------------------- validation
    def _val_sources(self, val_batches):
        return list(val_batches) if getattr(self.model, "mode", None) == 3 else [val_batches]

    def _validate(self, val_batches, limit=None):
        """`validation_step` per batch into the validation log, the outputs in the nesting `validation_epoch_end` expects (a list
        per dataloader in mode 3), then `validation_epoch_end` -> (the epoch's metric dict, validation steps run)"""
        model = self.model
        was_training = model.training
        model.eval()
        self.val_log.reset()
        steps, outputs = 0, []
        try:
            with torch.no_grad():
                for di, source in enumerate(self._val_sources(val_batches)):
                    outs = []
                    for i, batch in enumerate(source):
                        if limit is not None and i >= limit:
                            break
                        model.logged = {}
                        outs.append(model.validation_step(batch, i, di) if di else model.validation_step(batch, i))
                        self.val_log.update(model.logged)
                        steps += 1
                    outputs.append(outs)
                model.logged = {}
                model.validation_epoch_end(outputs if getattr(model, "mode", None) == 3 else outputs[0])
                at_end = dict(model.logged)
        finally:
            model.train(was_training)
        self.val_log.all_reduce()
        metrics = self.val_log.compute()
        metrics.update({k: float(v) for k, v in at_end.items()})
        return metrics, steps

    # ------------------------------------------------------------------------------------------------- checkpoints
    def _state(self, epoch, current):
        score = lambda x: None if x is None else float(x)
        return {"epoch": int(epoch), "global_step": int(self.global_step), "state_dict": self.model.state_dict(),
                "optimizer_states": [o.state_dict() for o in self.optimizers],
                "lr_schedulers": [s.state_dict() for s in self.schedulers],
                "callbacks": {"ModelCheckpoint": {"monitor": self.monitor, "mode": self.monitor_mode,
                                                  "best_model_score": score(self.best_score), "best_model_path": self.best_model_path,
                                                  "best_epoch": self.best_epoch, "current_score": score(current)}}}

    def _save(self, state, name):
        os.makedirs(self.root, exist_ok=True)
        path = os.path.join(self.root, name)
        torch.save(state, path + ".tmp")
        os.replace(path + ".tmp", path)
        return path

    def _checkpoint(self, epoch, metrics):
        """ModelCheckpoint(monitor, mode, filename="model", save_last=True) at the end of a validated epoch"""
        current = None
        if self.monitor is not None:
            if self.monitor not in metrics:
                raise ValueError("general.monitor: %r is not among the metrics of epoch %d; available keys: %s"
                               % (self.monitor, epoch, ", ".join(sorted(metrics)) or "(none)"))
            current = float(metrics[self.monitor])
            better = self.best_score is None and not math.isnan(current)
            if self.best_score is not None:
                better = current < self.best_score if self.monitor_mode == "min" else current > self.best_score
            if better:
                self.best_score, self.best_epoch = current, int(epoch)
                self.best_model_path = os.path.join(self.root, "model.ckpt")
        if self._rank() != 0:
            return
        state = self._state(epoch, current)
        if self.monitor is not None and self.best_epoch == epoch:
            self._save(state, "model.ckpt")
        self._save(state, "last.ckpt")

    def _resume(self, ckpt_path):
        if ckpt_path is None and self.cfg.model.get("use_checkpoint"):
            ckpt_path = os.path.join(self.cfg.general.output_root, self.cfg.model.use_checkpoint, "last.ckpt")
        if ckpt_path is None:
            return 0
        ckpt = torch.load(ckpt_path, map_location="cpu")
        self.model.load_state_dict(ckpt["state_dict"])
        for o, sd in zip(self.optimizers, ckpt.get("optimizer_states", [])):
            o.load_state_dict(sd)
        for s, sd in zip(self.schedulers, ckpt.get("lr_schedulers", [])):
            s.load_state_dict(sd)
        self.global_step = int(ckpt.get("global_step", 0))
        if hasattr(self.model, "global_step"):
            self.model.global_step = self.global_step
        mc = ckpt.get("callbacks", {}).get("ModelCheckpoint", {})
        self.best_score, self.best_epoch = mc.get("best_model_score"), mc.get("best_epoch")
        self.best_model_path = mc.get("best_model_path", "")
        return int(ckpt["epoch"]) + 1

    # ------------------------------------------------------------------------------------------------- the loop
    def training_batch(self, batch, idx, grad_sync=None):
        """one step of the training epoch: what `fit` runs per batch (tools/trainer_overhead.py times it against the bare loop)"""
        model = self.model
        model.zero_grad(set_to_none=True)
        out = model.training_step(batch, idx)
        loss = out[0] if isinstance(out, (tuple, list)) else out
        loss.backward()
        if grad_sync is not None:
            grad_sync()
        for o in self.optimizers:
            o.step()
        self.train_log.update(model.logged)
        self.global_step += 1
        if self.global_step % self.log_every_n_steps == 0:
            means = self.train_log.snapshot(tag=self.global_step)
            if means is not None:
                self._sink(dict(means, kind="step", epoch=self.current_epoch, global_step=self.train_log.snapshot_tag))
        return out

    def fit(self, train_batches, val_batches=None, ckpt_path=None):
        model = self.model
        self._configure()
        self._logs()
        start = self._resume(ckpt_path)
        grad_sync = self._reducer()
        if val_batches is not None and self.num_sanity_val_steps != 0 and start == 0:
            # the sanity check: that many validation batches (per dataloader) before epoch 0; results discarded, records cleared
            limit = None if self.num_sanity_val_steps < 0 else self.num_sanity_val_steps
            _m, self.sanity_steps_run = self._validate(val_batches, limit)
            self.val_log.reset()
        for epoch in range(start, self.epochs):
            self.current_epoch = model.current_epoch = epoch      # (the detector's prepare_epochs gate reads it)
            model.train()
            self.train_log.reset()
            if hasattr(train_batches, "set_epoch"):
                train_batches.set_epoch(epoch)            # (a loader's pass order follows the epoch: a resumed run continues the sequence)
            for i, batch in enumerate(train_batches):
                self.training_batch(batch, i, grad_sync)
            for s in self.schedulers:
                s.step()
            self.train_log.all_reduce()
            record = {"kind": "epoch", "epoch": epoch, "global_step": self.global_step}
            record.update(self.train_log.compute())
            bad = self.train_log.nonfinite()
            if bad:
                record["nonfinite"] = bad
            if val_batches is not None and (epoch + 1) % self.check_val_every_n_epoch == 0:
                metrics, _n = self._validate(val_batches)
                record.update(metrics)
                self.validated_epochs.append(epoch)
                self._checkpoint(epoch, metrics)
                self.last_metrics = metrics
            elif val_batches is None:
                if self._rank() == 0:
                    self._save(self._state(epoch, None), "last.ckpt")
            self._sink(record)
        return self
