"""`python -m d3net_amd.train -c <conf> (--synthetic N | --data) [--epochs E] [--root DIR]`, in place of scripts/train.py's
`__main__` (:329-391).

`--synthetic N`: `Trainer.fit` on synthetic scenes (d3net_amd/synthetic.py) -- a smoke path and a worked example of the fit loop,
not a dataset loader: N scenes in batches of `data.batch_size`, the first batch doubles as the validation split.

`--data`: `Trainer.fit` on the splits the configuration's paths name (conf/path.yaml): `dataset.build_loaders` loads each split into
a device-resident `SceneStore` and returns the mode's training and validation sources.  Under a launcher that sets WORLD_SIZE /
RANK / LOCAL_RANK (torch.distributed.run) every rank takes its shard of each pass.  Pretrained weights and freezes are applied as
`init_model` does (scripts/train.py:282-327); `--teacher` clusters on the labels, for a run that has no detector weights.
`--fused-prep` builds each batch's scene half straight from the store (`scene_prep.prepare_batch_store`: no read-back, the same
batches bit for bit) wherever that path applies; the start-up line says whether it is in use and what its index takes.
`--augment` augments the training split (the reference dataset's `is_augment`, which scripts/train.py leaves off); in the
detector-only mode that is PointGroup's own recipe -- elastic distortion and crop -- and with `--fused-prep` those batches come from
`scene_prep.prepare_batch_store_elastic` (one read-back per batch)."""
import argparse
import copy
import os
import types

import numpy as np
import torch

from . import synthetic as S
from .config import CONF_DIR, load_conf
from .pipeline import PipelineNet
from .trainer import Batches, Trainer

VOCAB = 3004      # the ScanRefer vocabulary's size


def synthetic_dataset(n_scenes, chunk):
    """the `dataset` object PipelineNet reads: vocabulary, a GloVe-shaped table, the annotation store of the reward and of validation"""
    ds = types.SimpleNamespace(vocabulary=S.make_vocabulary(VOCAB),
                               glove=np.random.default_rng(3).standard_normal((VOCAB, 300)).astype(np.float32))
    ds.chunked_data, ds.organized = S.make_language_corpus(n_scenes, chunk=chunk, vocab=VOCAB)
    ds.raw_data = S.corpus_raw_data(ds.organized)
    return {"train": ds, "val": ds}


def synthetic_batches(cfg, mode, n_scenes, dev):
    """-> (training source, validation source) in the shapes `Trainer.fit` takes for `mode`"""
    per, chunk = int(cfg.data.batch_size), int(cfg.data.num_des_per_scene)
    scenes = [S.small_scene(dims=(40, 32, 20), n_boxes=3, seed=3 + s) for s in range(n_scenes)]
    groups = [scenes[i:i + per] for i in range(0, n_scenes, per)]

    def language(group, seed, speaker):
        b = S.add_language(S.make_batch(group, dev), dev, chunk=chunk, vocab=VOCAB, seed=seed)
        if speaker:
            b["lang_len"] = b["spk_lang_len"]        # the speaker's lang_len is the caption length (+2)
        return b
    if mode == 0:
        train = [S.make_batch(g, dev) for g in groups]
        return Batches(train), Batches(train[:1])
    if mode in (1, 2):
        train = [language(g, 3, mode == 1) for g in groups]
        return Batches(train), Batches(train[:1])
    train = [[language(g, 3, True), language(g, 9, False)] for g in groups]        # the joint step's (speaker, listener) pair
    return Batches(train), (Batches([train[0][0]]), Batches([train[0][1]]))


def _ranks():
    """(world, rank, local rank) from the launcher's environment, as bench.py reads them; the process group of a multi-rank run"""
    import torch.distributed as dist
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1 and not dist.is_initialized():
        dist.init_process_group(os.environ.get("D3_DIST_BACKEND", "nccl"), rank=rank, world_size=world)
    return world, rank, local_rank


def _sources(x):
    """the PipelineLoaders inside a source, a PairedLoader or a tuple of them"""
    if isinstance(x, (tuple, list)):
        return [l for s in x for l in _sources(s)]
    return _sources(x.sources) if hasattr(x, "sources") else [x]


def fit_data(cfg, root, teacher=False, fused=False, augment=False):
    """--data: the configuration's splits through `dataset.build_loaders` into `Trainer.fit`"""
    from .checkpoint import apply_freeze, load_pretrained
    from .dataset import build_loaders
    world, rank, local_rank = _ranks()
    dev = torch.device("cuda", local_rank)
    torch.cuda.set_device(dev)
    torch.manual_seed(cfg.general.manual_seed)
    train, val, dataset, stores = build_loaders(cfg, dev, rank, world, fused=fused, augment=augment)
    model = PipelineNet(cfg, dataset).to(dev)             # init_model (scripts/train.py:282-327)
    loaded, frozen = load_pretrained(model, cfg), apply_freeze(model, cfg)
    print("=> pretrained: %s; frozen: %s" % (", ".join(loaded) or "none", ", ".join(frozen) or "none"))
    model.detector.teacher = bool(teacher)
    trainer = Trainer(cfg, model, root=root)
    nval = [len(v) for v in val] if isinstance(val, (tuple, list)) else len(val)
    print("=> train with MODE: %d, rank %d of %d; scene store: %s; %d training batches per epoch, %s validation batches, %d epochs -> %s"
          % (model.mode, rank, world, ", ".join("%s %d scenes %.1f MiB on %s" % (k, len(s), s.bytes() / 2 ** 20, s.device)
                                                for k, s in stores.items()), len(train), nval, trainer.epochs, trainer.root))
    if fused:
        loaders = _sources(train) + _sources(val)
        active = [l for l in loaders if l.fused_active(dev) or l.fused_elastic_active(dev)]
        elastic = [l for l in active if l.fused_elastic_active(dev)]
        for l in active:
            l.store.instance_index()                      # built here, once per store, not inside the first batch
            if l in elastic:
                l.store.absmax()
        print("=> fused batch preparation: in use by %d of %d loaders (%d on the elastic / crop path); instance index: %s"
              % (len(active), len(loaders), len(elastic), ", ".join("%s %.1f MiB" % (k, s.index_bytes() / 2 ** 20) for k, s in stores.items())))
    trainer.fit(train, val)
    return trainer


def main(argv=None, overrides=None):
    """overrides: a nested dict merged over the configuration files before `${...}` is resolved (e.g. {"DATA_PATH": ...})"""
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("-c", "--config", default="pointgroup.yaml", help="a task yaml: a path, or a file name under conf/")
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--synthetic", type=int, metavar="N", help="train on N synthetic scenes")
    src.add_argument("--data", action="store_true", help="train on the splits the configuration's paths name (dataset.build_loaders)")
    ap.add_argument("--teacher", action="store_true", help="with --data: cluster on the labels instead of the detector's predictions "
                    "(the switch --synthetic always sets; for a run without pretrained detector weights)")
    ap.add_argument("--fused-prep", action="store_true", help="with --data: build batches straight from the scene store "
                    "(scene_prep.prepare_batch_store) where that path applies")
    ap.add_argument("--augment", action="store_true", help="with --data: augment the training split as the reference dataset's "
                    "is_augment does (jitter / flip / rotation; elastic distortion and crop in the detector-only mode); with "
                    "--fused-prep the detector-only mode's batches come from scene_prep.prepare_batch_store_elastic")
    ap.add_argument("--epochs", type=int, default=None, help="override train.epochs")
    ap.add_argument("--root", default=None, help="run directory (default: <general.output_root>/<EXPERIMENT>)")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("d3net_amd.train needs a GPU: the product has no CPU path")
    conf = args.config if os.path.exists(args.config) else os.path.join(CONF_DIR, args.config)
    over = copy.deepcopy(overrides) if overrides else {}
    if args.epochs is not None:
        over.setdefault("train", {})["epochs"] = args.epochs
    cfg = load_conf(os.path.join(CONF_DIR, "path.yaml"), conf, overrides=over or None)
    if args.data:
        trainer = fit_data(cfg, args.root, args.teacher, args.fused_prep, args.augment)
        print("=> best %s: %s (epoch %s); metrics: %s" % (trainer.monitor, trainer.best_score, trainer.best_epoch,
                                                        os.path.join(trainer.root, "logs", "metrics.jsonl")))
        return trainer
    dev = torch.device("cuda", 0)
    torch.manual_seed(cfg.general.manual_seed)
    language = not (cfg.model.no_captioning and cfg.model.no_grounding)
    dataset = synthetic_dataset(min(args.synthetic, int(cfg.data.batch_size)), int(cfg.data.num_des_per_scene)) if language else None
    model = PipelineNet(cfg, dataset).to(dev)
    model.detector.teacher = True
    train, val = synthetic_batches(cfg, model.mode, args.synthetic, dev)
    trainer = Trainer(cfg, model, root=args.root)
    print("=> train with MODE: %d, %d scenes in %d batches, %d epochs -> %s" % (model.mode, args.synthetic, len(train), trainer.epochs, trainer.root))
    trainer.fit(train, val)
    print("=> best %s: %s (epoch %s); metrics: %s" % (trainer.monitor, trainer.best_score, trainer.best_epoch,
                                                    os.path.join(trainer.root, "logs", "metrics.jsonl")))
    return trainer


if __name__ == "__main__":
    main()
