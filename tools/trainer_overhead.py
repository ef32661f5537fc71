#!/usr/bin/env python3
"""Per-step cost of the fit loop: ms per step of `Trainer.training_batch` (zero_grad / training_step / backward / step +
MetricLog.update + the log_every_n_steps snapshot) against the bare zero_grad / training_step / backward / step loop bench.py times,
in ONE process on one model and one batch, the two arms alternated block by block as tools/ab.py does (clock drift and box noise hit
both alike).
usage: python tools/trainer_overhead.py [config] [--block 20] [--rounds 6]        (config: bench.py's names, default speaker)"""
import gc
import os
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from d3net_amd import synthetic as S  # noqa: E402
from d3net_amd.config import default_conf  # noqa: E402
from d3net_amd.trainer import Trainer  # noqa: E402


def opt_value(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


pos = [a for i, a in enumerate(sys.argv[1:], 1) if not a.startswith("--") and sys.argv[i - 1] not in ("--block", "--rounds")]
config = pos[0] if pos else "speaker"
block, rounds = opt_value("--block", 20), opt_value("--rounds", 6)
dev = torch.device("cuda", 0)
cfg = default_conf(bench.CONF[config], overrides={"general": {"root": tempfile.mkdtemp(prefix="trainer_overhead_")}})
torch.manual_seed(cfg.general.manual_seed)
scenes = bench.make_scenes(config, 0)
chunk = cfg.data.num_des_per_scene
from d3net_amd.pipeline import PipelineNet  # noqa: E402
model = PipelineNet(cfg, None if config == "detector" else bench.make_dataset(len(scenes), chunk, config == "joint")).to(dev).train()
model.detector.teacher = True
batch = S.make_batch(scenes, dev)
lis = None
if config != "detector":
    batch = S.add_language(batch, dev, chunk=chunk, vocab=bench.VOCAB)
    if config in ("speaker", "joint"):
        batch["lang_len"] = batch["spk_lang_len"]
    if config == "joint":
        lis = S.add_language(S.make_batch(scenes, dev), dev, chunk=chunk, vocab=bench.VOCAB, seed=9)

from d3net_amd.pointgroup import InputPrefetcher  # noqa: E402
feeder = InputPrefetcher(model.detector, (lambda: [dict(batch), dict(lis)]) if config == "joint" else (lambda: dict(batch)))

trainer = Trainer(cfg, model)
trainer._configure()           # the optimizer of configure_optimizers(): both arms step the same one
trainer._logs()
opt = trainer.optimizers[0]


def bare():
    model.zero_grad(set_to_none=True)
    loss, d = model.training_step(feeder.next())
    loss.backward()
    opt.step()


def fit_step():
    trainer.training_batch(feeder.next(), 0)


ARMS = (("bare loop", bare), ("fit loop", fit_step))
for _ in range(40):
    bare()
for _ in range(10):
    fit_step()
torch.cuda.synchronize()
gc.collect(); gc.freeze()
res = {name: [] for name, _f in ARMS}
for r in range(rounds):
    for name, f in (ARMS if r % 2 == 0 else ARMS[::-1]):
        for _ in range(4):
            f()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(block):
            f()
        torch.cuda.synchronize()
        res[name].append(1e3 * (time.perf_counter() - t0) / block)
means = trainer.train_log.compute()
assert means and all(v == v for v in means.values()), means
a, b = (statistics.median(res[name]) for name, _f in ARMS)
print("trainer_overhead (%s, log_every_n_steps %d): " % (config, trainer.log_every_n_steps) +
      "   ".join("%s -> %.3f ms (median %.3f, min %.3f)" % (name, statistics.mean(res[name]), statistics.median(res[name]), min(res[name]))
                 for name, _f in ARMS) + "   difference of the medians %+.3f ms (%+.2f %%), %d keys per step" % (b - a, 100.0 * (b - a) / a, len(means)),
      flush=True)
