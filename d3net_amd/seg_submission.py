"""ScanNet segmentation submission files written from the device: the four kinds of file that the
reference's `PointGroup.test()` leaves under `<root>/split_pred/<split>/` (model/pointgroup.py:543-625) -- the format of the ScanNet
semantic-label and instance benchmarks and of `seg_eval.evaluate_instance_files` / `evaluate_semantic_files` -- and the GT files of
lib/utils/eval.py:14-56, without `seg_eval.write_predictions`' copy of every array to the host and its `np.savetxt` per file.

`SegmentationSubmission.add_batch` takes `PointGroup.predict_instances`' dict: csrc/seg_submission.hip builds the cluster table
(scene, scene-local id, class per picked proposal), the per-point cluster ids and the decimal text of semantic/<scene>.txt and
instance/<scene>.cluster_ids.txt for the whole batch, read back ONCE into a reused pinned buffer; the mask files follow scene by
scene in chunks of whole proposals (two launches and one read-back per chunk).  The host writes slices of the pinned buffers and
formats only the lines of instance/<scene>.txt, so Python's `%.4f` stays the one rounding rule of a score.  Every file is
byte-equal to `seg_eval.write_predictions` / `write_gt`, which stay as they are.  No CPU fallback: tensors in host memory are refused.
"""
import ctypes as C
import os
import time

import numpy as np
import torch

from . import _lib
from . import seg_eval as SE
from ._call import call, on, ptr, stream, workspace
from .devstate import FLOATS, INTS, check_batch

TILE_LINES, MAX_WIDTH, MAX_SCENES, TABLE_COLS = 1024, 12, 4096, 5     # csrc/seg_submission.hip's; checked against the library
MAX_PICKS, MAX_PICKS_PER_SCENE = 1 << 20, 9999
INT32_MAX = 0x7fffffff
SEM_WIDTH = len(str(max(SE.SEM_CLASS_IDX))) + 1                        # "39\n"
GT_WIDTH = MAX_WIDTH                                                   # sem * 1000 + inst: any int32
_PRED_TABLE = {"pick": (INTS, (("n",),)), "scores": (FLOATS, (("n",),)), "proposals_idx": (INTS, (("L", 2),)),
               "proposals_offset": (INTS, (("P1",),)), "semantic_pred": (INTS, (("N",),)), "batch_offsets": (INTS, (("B1",),))}
_GT_TABLE = {"sem_labels": (INTS, (("N",),)), "instance_ids": (INTS, (("N",),)), "batch_offsets": (INTS, (("B1",),))}
_STATUS_TEXT = {1: "a value whose line does not fit the width planned for it", 2: "a semantic_pred outside [0, %d)" % len(SE.SEM_CLASS_IDX),
                4: "a pick outside the proposals, proposal offsets outside proposals_idx or a member outside the points"}
_cache = {}


# ------------------------------------------------------------------------------------------------ host planning
def cluster_id_width(n_picks):
    """bytes of the longest line of a cluster-id file, newline included, when no scene holds more than n_picks picks: "-1\\n" or
    the largest id n_picks - 1"""
    return max(3, len(str(max(int(n_picks) - 1, 0))) + 1)


def plan_tiles(batch_offsets, tile=TILE_LINES):
    """(B+1,) int64: the exclusive scan of ceil(points of scene b / tile); a block of the line kernels finds its scene in it"""
    n = np.diff(np.asarray(batch_offsets, np.int64))
    return np.concatenate([[0], np.cumsum((n + tile - 1) // tile)]).astype(np.int64)


def plan_chunks(count, npts, chunk_bytes):
    """[(first scene-local id, proposals)] : `count` mask files of 2 * npts bytes each in chunks of whole files of at most
    chunk_bytes; a chunk holds at least one file, even one larger than chunk_bytes"""
    per = 2 * int(npts)
    if count <= 0 or per <= 0:
        return []
    m_max = max(1, int(chunk_bytes) // per)
    return [(c, min(m_max, count - c)) for c in range(0, int(count), m_max)]


def record_layout(B, n, N, widths):
    """byte offsets inside the batch record that one read-back carries: status (2 int32), counts (B) int32, table (n,5) int32, per
    text lens (B) int64 -- up to `head`, zeroed before the launches -- then per text N * width bytes from a 16-byte boundary"""
    off, pos = {}, 0

    def take(name, nbytes, align):
        nonlocal pos
        pos = -(-pos // align) * align
        off[name] = pos
        pos += nbytes
    take("status", 8, 8); take("counts", 4 * B, 4); take("table", 4 * TABLE_COLS * n, 4)
    for k in range(len(widths)):
        take("lens%d" % k, 8 * B, 8)
    off["head"] = pos
    for k, w in enumerate(widths):
        take("text%d" % k, N * w, 16)
    off["total"] = -(-pos // 16) * 16
    return off


def instance_lines(name, table_rows):
    """instance/<scene>.txt (model/pointgroup.py:621-623) from the scene's rows of the read-back table, in pick order"""
    scores = np.ascontiguousarray(table_rows[:, 4]).view(np.float32)
    return "".join("predicted_masks/%s_%03d.txt %d %.4f\n" % (name, int(r[1]), int(r[2]), float(s)) for r, s in zip(table_rows, scores))


def _limits():
    if "limits" not in _cache:
        v = [C.c_int(0) for _ in range(4)]
        _lib.check(_lib.lib().d3_seg_submit_limits(*[C.byref(x) for x in v]), "seg_submit_limits")
        got = tuple(x.value for x in v)
        if got != (TILE_LINES, MAX_WIDTH, MAX_SCENES, TABLE_COLS):
            raise _lib.D3Error("libd3hip.so's segmentation writer has limits %s, this module %s" % (got, (TILE_LINES, MAX_WIDTH, MAX_SCENES, TABLE_COLS)))
        _cache["limits"] = got
    return _cache["limits"]


def _pinned(tag, nbytes):
    """a reused, growing pinned host buffer per use (the batch record, a mask chunk)"""
    buf = _cache.get(("pinned", tag))
    if buf is None or buf.numel() < nbytes:
        buf = _cache[("pinned", tag)] = torch.empty(int(nbytes * 1.25) + 4096, dtype=torch.uint8, pin_memory=True)
    return buf


def _read_back(tag, dev_bytes):
    """the device bytes -> a numpy view of the pinned buffer `tag`: one asynchronous copy, one wait for the stream"""
    host = _pinned(tag, dev_bytes.numel())[:dev_bytes.numel()]
    host.copy_(dev_bytes, non_blocking=True)
    torch.cuda.current_stream(dev_bytes.device).synchronize()
    return host.numpy()


def _lut(dev):
    key = ("lut", dev)
    if key not in _cache:
        _cache[key] = torch.tensor(SE.SEM_CLASS_IDX, dtype=torch.int32, device=dev)
    return _cache[key]


def _i32(t):
    return t.detach().to(torch.int32).contiguous()


def _at(t, offset):
    return C.c_void_p(t.data_ptr() + offset)


def _raise_status(name, status):
    raise _lib.D3Error("%s: the batch holds %s; no file of it was written" % (name, "; ".join(t for b, t in sorted(_STATUS_TEXT.items()) if status & b)))


class SegmentationSubmission:
    """model/pointgroup.py:603-625 on the device.  `add_batch(pred, data_dict, scene_names)`: pred is `predict_instances`' dict,
    data_dict needs only batch_offsets; the files go to <root>/split_pred/<split>/ with `seg_eval.write_predictions`' names,
    directories and overwrite rule (a file is replaced, an older mask file that is not written again stays).  A scene without picks
    gets an empty instance/<scene>.txt, no mask file and cluster ids of -1; a scene without points gets empty files.
    `add_gt(data_dict, scene_names)`: <root>/split_gt/<split>/<scene>.txt as `seg_eval.write_gt`.  `files()`: the paths written so
    far, relative to root, in order.  chunk_bytes bounds the mask bytes per read-back (whole proposals, at least one).  timings: a
    dict that receives the seconds spent in device work + read-back ("device_s") and in writing files ("files_s")."""

    def __init__(self, root, split="val", chunk_bytes=64 << 20, device="cuda", timings=None):
        if int(chunk_bytes) < 1:
            raise ValueError("SegmentationSubmission: chunk_bytes >= 1")
        self.root, self.split, self.chunk_bytes, self.device = os.fspath(root), split, int(chunk_bytes), torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("SegmentationSubmission: the text is made on the GPU, there is no CPU fallback (device %s)" % self.device)
        self.timings = timings
        self._files = []

    def files(self):
        return list(self._files)

    # ------------------------------------------------------------------------------------------- checks
    def _pred_geometry(self, names):
        def geometry(d):
            name = "SegmentationSubmission.add_batch"
            bo, pidx, poff = d["batch_offsets"], d["proposals_idx"], d["proposals_offset"]
            if bo.dim() != 1 or bo.numel() < 2:
                raise ValueError("%s: batch_offsets (B+1,) with B >= 1 expected, got %s" % (name, tuple(bo.shape)))
            B = bo.numel() - 1
            if len(names) != B:
                raise ValueError("%s: %d scene names for %d scenes" % (name, len(names), B))
            if B > MAX_SCENES:
                raise ValueError("%s: %d scenes in one batch, at most %d" % (name, B, MAX_SCENES))
            if pidx.dim() != 2 or pidx.shape[1] != 2:
                raise ValueError("%s: proposals_idx (L,2) expected, got %s" % (name, tuple(pidx.shape)))
            if poff.dim() != 1 or poff.numel() < 1:
                raise ValueError("%s: proposals_offset holds P + 1 entries in one dimension, got %s" % (name, tuple(poff.shape)))
            if d["pick"].dim() != 1 or d["semantic_pred"].dim() != 1:
                raise ValueError("%s: pick (n,) and semantic_pred (N,) expected, got %s and %s"
                                 % (name, tuple(d["pick"].shape), tuple(d["semantic_pred"].shape)))
            n, N, L = d["pick"].numel(), d["semantic_pred"].numel(), pidx.shape[0]
            if n > MAX_PICKS or L > INT32_MAX or N * max(SEM_WIDTH, cluster_id_width(n)) > INT32_MAX:
                raise ValueError("%s: totals outside int32 (N %d points, L %d members, n %d picks)" % (name, N, L, n))
            ints = all(d[k].dtype in INTS for k in ("pick", "proposals_idx", "proposals_offset", "batch_offsets"))
            if n > MAX_PICKS_PER_SCENE and ints and L > 0:                # (only then can a scene exceed the bound)
                most = int(_picks_per_scene(d["pick"], pidx, poff, bo).max())
                if most > MAX_PICKS_PER_SCENE:
                    raise ValueError("%s: %d picks in one scene, at most %d" % (name, most, MAX_PICKS_PER_SCENE))
            return dict(B=B, B1=B + 1, n=n, N=N, L=L, P1=poff.numel())
        return geometry

    @staticmethod
    def _gt_geometry(names):
        def geometry(d):
            name = "SegmentationSubmission.add_gt"
            bo = d["batch_offsets"]
            if bo.dim() != 1 or bo.numel() < 2:
                raise ValueError("%s: batch_offsets (B+1,) with B >= 1 expected, got %s" % (name, tuple(bo.shape)))
            B, N = bo.numel() - 1, d["sem_labels"].numel()
            if len(names) != B:
                raise ValueError("%s: %d scene names for %d scenes" % (name, len(names), B))
            if B > MAX_SCENES or N * GT_WIDTH > INT32_MAX:
                raise ValueError("%s: %d scenes (at most %d), totals outside int32 (N %d points)" % (name, B, MAX_SCENES, N))
            return dict(B=B, B1=B + 1, N=N)
        return geometry

    def _offsets(self, name, bo_dev, N):
        """batch_offsets on the host (the plan needs them: one read of B + 1 ints), checked"""
        bo = bo_dev.cpu().numpy().astype(np.int64)
        if bo[0] < 0 or bo[-1] > N or (np.diff(bo) < 0).any():
            raise ValueError("%s: batch_offsets must be nondecreasing within [0, %d]: %s" % (name, N, bo))
        return bo

    def _clock(self, t0, t1, t2):
        if self.timings is not None:
            self.timings["device_s"] = self.timings.get("device_s", 0.0) + (t1 - t0)
            self.timings["files_s"] = self.timings.get("files_s", 0.0) + (t2 - t1)

    def _write(self, path, *parts):
        with open(os.path.join(self.root, path), "wb") as f:
            for p in parts:
                f.write(p)
        self._files.append(path)

    def _lines(self, dev, texts, N, bo, bo_dev, rec, lay):
        """the three launches of d3_seg_int_lines for one or two (values, lut, width) texts into `rec` at `lay`"""
        B = len(bo) - 1
        prefix = plan_tiles(bo)
        tiles = int(prefix[-1])
        prefix_dev = torch.from_numpy(prefix.astype(np.int32)).to(dev)
        ws = workspace(max(int(_lib.lib().d3_seg_int_lines_ws_bytes(tiles, len(texts))), 256), dev, "seg_submission_lines")
        args = []
        for k in range(2):
            if k < len(texts):
                values, lut, width = texts[k]
                args += [ptr(values), ptr(lut), 0 if lut is None else lut.numel(), width, _at(rec, lay["text%d" % k]), _at(rec, lay["lens%d" % k])]
            else:
                args += [None, None, 0, 0, None, None]
        call("seg_int_lines", *args, N, ptr(bo_dev), ptr(prefix_dev), B, tiles, _at(rec, lay["status"]), ptr(ws), ws.numel(), stream())

    # ------------------------------------------------------------------------------------------- predictions
    def add_batch(self, pred, data_dict, scene_names):
        """table, ids and line launches, ONE read-back of the batch record (after the B + 1 batch offsets the plan needs); then per
        chunk of mask files two launches and one read-back.  `pred` and `data_dict` are left as they are."""
        name = "SegmentationSubmission.add_batch"
        names = list(scene_names)
        d = {k: pred[k] for k in ("pick", "scores", "proposals_idx", "proposals_offset", "semantic_pred") if k in pred}
        if "batch_offsets" in data_dict:
            d["batch_offsets"] = data_dict["batch_offsets"]
        dims = check_batch(name, d, _PRED_TABLE, self._pred_geometry(names), self.device)
        B, n, N, L, P = dims["B"], dims["n"], dims["N"], dims["L"], dims["P1"] - 1
        dev = d["pick"].device
        _limits()
        t0 = time.perf_counter()
        bo = self._offsets(name, d["batch_offsets"], N)
        pick, pidx, poff, sem, bo_dev = (_i32(d[k]) for k in ("pick", "proposals_idx", "proposals_offset", "semantic_pred", "batch_offsets"))
        scores = d["scores"].detach().contiguous()
        lut = _lut(dev)
        w_ids = cluster_id_width(n)
        lay = record_layout(B, n, N, (SEM_WIDTH, w_ids))
        rec = workspace(lay["total"], dev, "seg_submission_record")
        ids = workspace(4 * max(N, 1), dev, "seg_submission_ids")[:4 * max(N, 1)].view(torch.int32)
        with on(dev):
            rec[:lay["head"]].zero_()
            call("seg_cluster_table", ptr(pick), n, ptr(pidx), L, ptr(poff), P, ptr(sem), ptr(scores), N, ptr(bo_dev), B, ptr(lut), lut.numel(),
                 _at(rec, lay["table"]), _at(rec, lay["counts"]), _at(rec, lay["status"]), stream())
            call("seg_cluster_ids", _at(rec, lay["table"]), ptr(pick), n, ptr(pidx), L, ptr(poff), P, ptr(bo_dev), B, N, ptr(ids), stream())
            self._lines(dev, [(sem, lut, SEM_WIDTH), (ids, None, w_ids)], N, bo, bo_dev, rec, lay)
            host = _read_back("record", rec[:lay["total"]])                                   # the one read-back
        status = int(host[lay["status"]:lay["status"] + 4].view(np.int32)[0])
        if status:
            _raise_status(name, status)
        counts = host[lay["counts"]:lay["counts"] + 4 * B].view(np.int32)
        if n and int(counts.max()) > MAX_PICKS_PER_SCENE:
            raise ValueError("%s: %d picks in one scene, at most %d" % (name, int(counts.max()), MAX_PICKS_PER_SCENE))
        table = host[lay["table"]:lay["table"] + 4 * TABLE_COLS * n].view(np.int32).reshape(n, TABLE_COLS)
        lens = [host[lay["lens%d" % k]:lay["lens%d" % k] + 8 * B].view(np.int64) for k in range(2)]
        text = memoryview(host)
        t1 = time.perf_counter()
        self._clock(t0, t1, t1)

        base = os.path.join("split_pred", self.split)
        sem_dir, inst_dir = os.path.join(base, "semantic"), os.path.join(base, "instance")
        mask_dir = os.path.join(inst_dir, "predicted_masks")
        for sub in (sem_dir, mask_dir):
            os.makedirs(os.path.join(self.root, sub), exist_ok=True)
        # the largest chunk of any scene: its first one (the chunks of a scene are equal but for the last)
        mask_room = max([2 * int(bo[b + 1] - bo[b]) * m for b in range(B)
                         for _, m in plan_chunks(int(counts[b]), int(bo[b + 1] - bo[b]), self.chunk_bytes)[:1]] + [0])
        masks = workspace(mask_room + 16, dev, "seg_submission_masks") if mask_room else None
        for b, scene in enumerate(names):
            t1 = time.perf_counter()
            lo, npts = int(bo[b]), int(bo[b + 1] - bo[b])
            at = lay["text0"] + lo * SEM_WIDTH
            self._write(os.path.join(sem_dir, "%s.txt" % scene), text[at:at + int(lens[0][b])])
            rows = table[table[:, 0] == b]
            self._write(os.path.join(inst_dir, "%s.txt" % scene), instance_lines(scene, rows).encode())
            self._clock(t1, t1, time.perf_counter())
            for c_lo, m in plan_chunks(len(rows), npts, self.chunk_bytes):
                t0 = time.perf_counter()
                with on(dev):
                    call("seg_mask_lines", _at(rec, lay["table"]), ptr(pick), n, ptr(pidx), L, ptr(poff), P, b, lo, npts, c_lo, m, ptr(masks),
                         masks.numel() // 16 * 16, stream())
                    chunk = memoryview(_read_back("masks", masks[:2 * m * npts]))
                t1 = time.perf_counter()
                for c in range(m):
                    self._write(os.path.join(mask_dir, "%s_%03d.txt" % (scene, c_lo + c)), chunk[2 * npts * c:2 * npts * (c + 1)])
                self._clock(t0, t1, time.perf_counter())
            t1 = time.perf_counter()
            at = lay["text1"] + lo * w_ids
            self._write(os.path.join(inst_dir, "%s.cluster_ids.txt" % scene), text[at:at + int(lens[1][b])])
            self._clock(t1, t1, time.perf_counter())

    # ------------------------------------------------------------------------------------------- ground truth
    def add_gt(self, data_dict, scene_names):
        """<root>/split_gt/<split>/<scene>.txt: `seg_eval.gt_ids` on the device, sem * 1000 + inst, the line launches, one
        read-back of lengths and text"""
        name = "SegmentationSubmission.add_gt"
        names = list(scene_names)
        d = {k: data_dict[k] for k in _GT_TABLE if k in data_dict}
        dims = check_batch(name, d, _GT_TABLE, self._gt_geometry(names), self.device)
        B, N = dims["B"], dims["N"]
        dev = d["sem_labels"].device
        if "instance_offsets" in data_dict and not (torch.is_tensor(data_dict["instance_offsets"]) and data_dict["instance_offsets"].is_cuda):
            raise ValueError("%s: instance_offsets is in host memory; it must be on the GPU, there is no CPU fallback" % name)
        _limits()
        t0 = time.perf_counter()
        bo = self._offsets(name, d["batch_offsets"], N)
        gsem, ginst = SE.gt_ids(data_dict)
        enc = (gsem.to(torch.int32) * 1000 + ginst.to(torch.int32)).contiguous()
        bo_dev = _i32(d["batch_offsets"])
        lay = record_layout(B, 0, N, (GT_WIDTH,))
        rec = workspace(lay["total"], dev, "seg_submission_record")
        with on(dev):
            rec[:lay["head"]].zero_()
            self._lines(dev, [(enc, None, GT_WIDTH)], N, bo, bo_dev, rec, lay)
            host = _read_back("record", rec[:lay["total"]])
        status = int(host[lay["status"]:lay["status"] + 4].view(np.int32)[0])
        if status:
            _raise_status(name, status)
        lens = host[lay["lens0"]:lay["lens0"] + 8 * B].view(np.int64)
        text = memoryview(host)
        t1 = time.perf_counter()
        gt_dir = os.path.join("split_gt", self.split)
        os.makedirs(os.path.join(self.root, gt_dir), exist_ok=True)
        for b, scene in enumerate(names):
            at = lay["text0"] + int(bo[b]) * GT_WIDTH
            self._write(os.path.join(gt_dir, "%s.txt" % scene), text[at:at + int(lens[b])])
        self._clock(t0, t1, time.perf_counter())


def _picks_per_scene(pick, pidx, poff, bo):
    """(B,) picks per scene in torch, wherever the tensors live: the check of the 9 999 bound before anything is launched, needed
    only for a batch of more than 9 999 picks"""
    P, L, B = poff.numel() - 1, pidx.shape[0], bo.numel() - 1
    p = pick.long()
    ok = (p >= 0) & (p < P)
    p = p.clamp(0, max(P - 1, 0))
    s, e = poff.long()[p], poff.long()[(p + 1).clamp(max=P)]
    ok &= (e > s) & (s >= 0) & (s < L)
    first = pidx[s.clamp(0, L - 1), 1].long()
    bo = bo.long().to(first.device)
    ok &= (first >= bo[0]) & (first < bo[-1])
    scene = torch.bucketize(first, bo[1:].contiguous(), right=True).clamp(max=B - 1)
    return torch.bincount(scene[ok], minlength=B)
