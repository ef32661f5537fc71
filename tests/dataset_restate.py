"""Host restatement of the reference's list bookkeeping that d3net_amd.dataset replaces, written from the behaviour of
lib/dataset/pipeline.py:583-604 (_get_chunked_data / _chunks), :774-802 (_get_coord_and_feat_from_mesh) and scripts/train.py:41-245
(init_detector_data / init_speaker_data / init_listener_data), and of Lightning's max_size_cycle pairing of two training loaders.
Plain Python and numpy; the annotation entries themselves are carried, not their indices."""
import random
from copy import deepcopy

import numpy as np

FILL = "SYNTHETIC"


def fill_entry(scan):
    e = {"scene_id": scan}
    for key in ("object_id", "object_name", "ann_id", "description"):
        e[key] = FILL
    e["token"] = [FILL]
    return e


def chunked(raw_data, size):
    """the entries grouped per scene in first-appearance order, each group cut into pieces of at most `size`"""
    groups, order = {}, []
    for entry in raw_data:
        s = entry["scene_id"]
        if s not in groups:
            groups[s] = []
            order.append(s)
        groups[s].append(entry)
    pieces = []
    for s in order:
        lst, start = groups[s], 0
        while start < len(lst):
            pieces.append(lst[start:start + size])
            start += size
    return pieces


def scans_of(raw):
    seen = set()
    for entry in raw:
        seen.add(entry["scene_id"])
    return sorted(seen)


def detector(train_scans, val_scans):
    """-> {split: (entries, scan list)}"""
    return {"train": ([fill_entry(s) for s in train_scans], list(train_scans)),
            "val": ([fill_entry(s) for s in val_scans], list(val_scans))}


def speaker(raw_train, raw_val, all_train_scans, extra_ratio, seed):
    """-> {split: (entries, scan list)}; the fill's choices and the shuffle come from random.Random(seed)"""
    rnd = random.Random(seed)
    val_scans = scans_of(raw_val)
    val = []
    for s in val_scans:
        e = deepcopy(raw_val[0])
        e["scene_id"] = s
        val.append(e)
    train, train_scans = deepcopy(raw_train), scans_of(raw_train)
    if extra_ratio > 0:
        wanted = int(len(raw_train) * extra_ratio)
        unused = [s for s in all_train_scans if s not in train_scans]
        fill = []
        for i in range(wanted):
            fill.append(fill_entry(unused[i] if i < len(unused) else rnd.choice(unused)))
        train = train + fill
        train_scans = train_scans + scans_of(fill)
        rnd.shuffle(train)
    return {"train": (train, train_scans), "val": (val, val_scans)}


def listener(raw_train, raw_val):
    return {"train": (deepcopy(raw_train), scans_of(raw_train)), "val": (deepcopy(raw_val), scans_of(raw_val))}


def mesh_columns(mesh, use_color, use_normal, multiview):
    """-> (coords, feats): xyz, then rgb / normals / the 128 multiview columns as switched on; multiview None = not used"""
    data = mesh[:, :3]
    if use_color:
        data = np.concatenate([data, mesh[:, 3:6]], 1)
    if use_normal:
        assert mesh.shape[1] == 9
        data = np.concatenate([data, mesh[:, 6:9]], 1)
    if multiview is not None:
        data = np.concatenate([data, multiview], 1)
    return data[:, :3], data[:, 3:]


def max_size_cycle(lengths):
    """per step of the combined epoch, each loader's (pass number, batch number): the epoch is as long as the longest loader and an
    exhausted loader starts over"""
    steps = []
    for i in range(max(lengths)):
        steps.append([(i // n, i % n) for n in lengths])
    return steps
