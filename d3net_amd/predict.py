"""`python -m d3net_amd.predict -c <conf> --task captioning|grounding|segmentation [--split test] [--root DIR] [--ckpt FILE]
[--out FILE]`, in place of the reference's `benchmark/benchmark_captioning.py` and `benchmark/benchmark_grounding.py`: from a
configuration and a checkpoint to the file one uploads to the Scan2Cap / ScanRefer benchmark server -- and, with --task
segmentation, in place of `PointGroup.test()` (model/pointgroup.py:543-625): the per-scene files of the ScanNet semantic-label and
instance benchmarks under `<root>/split_pred/<split>/`.

The split's scenes go into a label-free `SceneStore` (`dataset.build_test_loader`: nothing is read from the label arrays, which
are placeholders on the ScanNet test split), every batch is `scene_prep.prepare_points_store` plus the description keys, and
`PipelineNet.predict_captioning` / `predict_grounding` collect the records on the device (`submission.py`).  The scripts' own
overrides are applied: data.num_des_per_scene = 8 (captioning) / 1 (grounding), cluster.prepare_epochs = -1.  Weights come from
`<root>/model.ckpt` (or --ckpt), loaded non-strictly as the scripts do; the file is `<root>/benchmark_<split>.nms.json`
(captioning) or `<root>/pred.json` (grounding), or --out.  Single process: the scripts are, and a sampler's padding would repeat
scenes.

--task segmentation (default configuration pointgroup.yaml) needs no annotation file: the scenes are those of
SCANNETV2_PATH.<split>_list, one per sample in list order, in a label-free store and loader of its own (`segmentation_loader`);
`PipelineNet.predict_segmentation` writes the files through `seg_submission.SegmentationSubmission`, --out replaces <root> as the
directory that receives split_pred/.  Its only override is cluster.prepare_epochs = -1."""
import argparse
import copy
import os

import torch

from .config import CONF_DIR, load_conf

TASKS = {"captioning": {"num_des_per_scene": 8, "absent": "no_captioning", "head": "speaker", "config": "pointgroup_captioning.yaml"},
         "grounding": {"num_des_per_scene": 1, "absent": "no_grounding", "head": "listener", "config": "pointgroup_captioning.yaml"},
         "segmentation": {"num_des_per_scene": None, "absent": None, "head": None, "config": "pointgroup.yaml"}}


def default_output(root, task, split):
    """benchmark_captioning.py:192 / benchmark_grounding.py:182"""
    return os.path.join(root, "benchmark_%s.nms.json" % split if task == "captioning" else "pred.json")


def task_conf(config, task, overrides=None):
    """conf/path.yaml merged under `config` (a path, or a file name under conf/) and `overrides`, then the scripts' own
    (benchmark_captioning.py:40-45, benchmark_grounding.py:36-41): data.num_des_per_scene, cluster.prepare_epochs = -1"""
    conf = config if os.path.exists(config) else os.path.join(CONF_DIR, config)
    over = copy.deepcopy(overrides) if overrides else {}
    if TASKS[task]["num_des_per_scene"] is not None:
        over.setdefault("data", {})["num_des_per_scene"] = TASKS[task]["num_des_per_scene"]
    over.setdefault("cluster", {})["prepare_epochs"] = -1
    return load_conf(os.path.join(CONF_DIR, "path.yaml"), conf, overrides=over)


def main(argv=None, overrides=None):
    """overrides: a nested dict merged over the configuration files before `${...}` is resolved (e.g. {"DATA_PATH": ...}); the
    scripts' own overrides go on top of it.  -> the submission (its file is written)"""
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("-c", "--config", default=None,
                    help="a task yaml: a path, or a file name under conf/ (default: pointgroup_captioning.yaml; segmentation: pointgroup.yaml)")
    ap.add_argument("--task", required=True, choices=sorted(TASKS))
    ap.add_argument("--split", default="test", help="the split whose annotation file and scenes are read (default: test)")
    ap.add_argument("--root", default=None, help="run directory (default: general.root, or <general.output_root>/<EXPERIMENT>)")
    ap.add_argument("--ckpt", default=None, help="checkpoint (default: <root>/model.ckpt)")
    ap.add_argument("--out", default=None, help="prediction file (default: <root>/benchmark_<split>.nms.json or <root>/pred.json); "
                                                "segmentation: the directory that receives split_pred/ (default: <root>)")
    args = ap.parse_args(argv)
    task = TASKS[args.task]
    cfg = task_conf(args.config or task["config"], args.task, overrides)

    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("d3net_amd.predict is single-process (WORLD_SIZE is %s): the benchmark scripts are, and a sharded sampler's "
                         "padding would repeat scenes in the file" % os.environ["WORLD_SIZE"])
    if cfg.data.requires_gt_mask:
        raise SystemExit("d3net_amd.predict: data.requires_gt_mask is set, but a label-free batch has no GT proposals")
    if task["absent"] is None:
        if cfg.model.no_detection:
            raise SystemExit("d3net_amd.predict: --task segmentation needs the detector; this configuration has model.no_detection=True")
    elif cfg.model.no_detection or cfg.model[task["absent"]]:
        raise SystemExit("d3net_amd.predict: --task %s needs the detector and the %s; this configuration has model.no_detection=%s, model.%s=%s"
                         % (args.task, task["head"], cfg.model.no_detection, task["absent"], cfg.model[task["absent"]]))
    g = cfg.general
    root = args.root or g.get("root") or os.path.join(g.output_root, str(g.experiment).upper())
    ckpt = args.ckpt or os.path.join(root, "model.ckpt")
    if not os.path.exists(ckpt):
        raise SystemExit("d3net_amd.predict: no checkpoint at %s" % ckpt)
    if not torch.cuda.is_available():
        raise SystemExit("d3net_amd.predict needs a GPU: the product has no CPU path")

    if args.task == "segmentation":
        return _segmentation(cfg, args, root, ckpt)
    from .checkpoint import load_lightning_checkpoint
    from .dataset import build_test_loader
    from .pipeline import PipelineNet
    from .submission import CaptionSubmission, GroundingSubmission
    dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(dev)
    torch.manual_seed(g.manual_seed)
    loader, dataset, store = build_test_loader(cfg, dev, args.task, args.split)
    model = PipelineNet(cfg, dataset).to(dev)
    load_lightning_checkpoint(model, ckpt, strict=False)
    chunked = dataset[args.split].chunked_data
    print("=> predict %s on split %s: %d scenes (%.1f MiB on %s, no labels), %d samples in %d batches, weights %s"
          % (args.task, args.split, len(store), store.bytes() / 2 ** 20, store.device, loader.num_samples(), len(loader), ckpt))
    if args.task == "captioning":
        sub = CaptionSubmission(chunked, model.vocabulary, max_proposals=cfg.model.max_num_proposal, max_len=cfg.data.max_spk_len + 1, device=dev)
        model.predict_captioning(loader, sub)
    else:
        sub = GroundingSubmission(chunked, device=dev)
        model.predict_grounding(loader, sub)
    out = args.out or default_output(root, args.task, args.split)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    sub.write(out)
    print("=> wrote %s" % out)
    return sub


def segmentation_loader(cfg, device, split="test", store_device=None):
    """the scenes of SCANNETV2_PATH.<split>_list in a label-free `SceneStore` and a label-free `PipelineLoader` without descriptions,
    one scene per sample in list order, unshuffled -> (loader, store)"""
    from .dataset import PipelineLoader, SceneStore, read_scan_list
    scans = read_scan_list(cfg.SCANNETV2_PATH["%s_list" % split])
    store = SceneStore.load(cfg, split, scans, device if store_device is None else store_device, labels=False)
    loader = PipelineLoader(cfg, store, None, split, "detector", seed=int(cfg.general.manual_seed), device=device, label_free=True,
                            scene_ids=scans)
    return loader, store


def batch_scene_names(loader):
    """one list of scene names per batch of the pass `iter(loader)` has just begun: `loader.last_order` cut by data.batch_size"""
    order, size = loader.last_order, loader.batch_size
    return [[loader.sample_scene(i) for i in order[at:at + size]] for at in range(0, len(order), size)]


def _segmentation(cfg, args, root, ckpt):
    from .checkpoint import load_lightning_checkpoint
    from .pipeline import PipelineNet
    from .seg_submission import SegmentationSubmission
    dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(dev)
    torch.manual_seed(cfg.general.manual_seed)
    loader, store = segmentation_loader(cfg, dev, args.split)
    model = PipelineNet(cfg).to(dev)
    load_lightning_checkpoint(model, ckpt, strict=False)
    print("=> predict segmentation on split %s: %d scenes (%.1f MiB on %s, no labels) in %d batches, weights %s"
          % (args.split, len(store), store.bytes() / 2 ** 20, store.device, len(loader), ckpt))
    sub = SegmentationSubmission(args.out or root, split=args.split, device=dev)
    batches = iter(loader)
    model.predict_segmentation(batches, sub, scene_names=batch_scene_names(loader))
    print("=> wrote %d files of %d scenes under %s" % (len(sub.files()), loader.num_samples(), os.path.join(sub.root, "split_pred", args.split)))
    return sub


if __name__ == "__main__":
    main()
