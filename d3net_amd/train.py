"""`python -m d3net_amd.train -c <conf> --synthetic N [--epochs E] [--root DIR]`: `Trainer.fit` on synthetic scenes
(d3net_amd/synthetic.py), in place of scripts/train.py's `__main__` (:329-391).  A smoke path and a worked example of the fit
loop -- the batches are what `scene_prep.prepare_batch` / `lang_prep.prepare_pipeline_batch` produce from real scenes
 -- not a dataset loader: N scenes in batches of `data.batch_size`, the first batch doubles as the validation
split."""
import argparse
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


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("-c", "--config", default="pointgroup.yaml", help="a task yaml: a path, or a file name under conf/")
    ap.add_argument("--synthetic", type=int, required=True, metavar="N", help="train on N synthetic scenes")
    ap.add_argument("--epochs", type=int, default=None, help="override train.epochs")
    ap.add_argument("--root", default=None, help="run directory (default: <general.output_root>/<EXPERIMENT>)")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("d3net_amd.train needs a GPU: the product has no CPU path")
    conf = args.config if os.path.exists(args.config) else os.path.join(CONF_DIR, args.config)
    over = {"train": {"epochs": args.epochs}} if args.epochs is not None else None
    cfg = load_conf(os.path.join(CONF_DIR, "path.yaml"), conf, overrides=over)
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
