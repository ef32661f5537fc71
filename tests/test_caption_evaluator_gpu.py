"""The captioning validation on the device (csrc/caption_eval.hip, caption_eval.CaptionEvaluator): d3_caption_stats through the
C ABI against the plain restatement (tests/caption_stats_restate.py, pinned to caption_metrics on the CPU), CaptionEvaluator
against eval_caption_step + eval_caption_epoch on the golden inputs and on a merged epoch, no read-back in add_batch,
PipelineNet.evaluate_captioning against the validation hooks, and what is refused.  BLEU and ROUGE compare with ==, CIDEr within
1e-12 relative (the bound tests/test_rl_gpu.py holds d3_cider_scores to)."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import caption_stats_restate as R  # noqa: E402

THRESHOLDS = (0.25, 0.5)


def _batch(inp, dev, scenes=None, names=None):
    """the six keys eval_caption_step reads, from caption_inputs()-shaped arrays"""
    sel = list(range(len(inp["scene_list"]))) if scenes is None else list(scenes)
    t = lambda k: torch.from_numpy(np.ascontiguousarray(inp[k][sel])).to(dev)
    return dict(lang_cap=t("pred_captions"), proposal_bbox_batched=t("pred_boxes"), gt_bbox=t("gt_boxes"), gt_bbox_object_id=t("gt_box_ids"),
                gt_bbox_label=t("gt_box_masks"), scene_id=list(names) if names is not None else [inp["scene_list"][i] for i in sel])


def _assert_epoch_equal(got, want, cider_rtol=1e-12):
    (gb, gc, gr, gm), (wb, wc, wr, wm) = got, want
    print("bleu", gb[0], wb[0], "rouge", gr[0], wr[0], "cider", gc[0], wc[0],
          "max cider rel", float(np.max(np.abs(gc[1] - wc[1]) / np.maximum(np.abs(wc[1]), 1e-300))) if len(wc[1]) else 0.0)
    assert gb[0] == wb[0] and gb[1] == wb[1]
    assert gr[0] == wr[0] and gr[1].tolist() == wr[1].tolist()
    assert abs(gc[0] - wc[0]) <= cider_rtol * abs(wc[0]) and np.allclose(gc[1], wc[1], rtol=cider_rtol, atol=0)
    assert gm[0] == 0.0 and gm[1].tolist() == wm[1].tolist()


@pytest.fixture(scope="module")
def golden(dev):
    from gen_caption_eval_golden import caption_inputs
    from d3net_amd import caption_eval as ce
    inp = caption_inputs()
    batch = _batch(inp, dev)
    host = ce.eval_caption_step(dict(batch), inp["vocab"])
    return inp, batch, host


def test_caption_stats_kernel_equals_the_restatement(dev):
    from d3net_amd import _lib
    rng = np.random.default_rng(31)
    E = 67
    alphabet = np.array([4, 5, 6, 7, 8, 65530, 65533, 65534])
    weights = np.array([.19, .19, .19, .19, .19, .02, .02, .01])
    lengths = [2, 3, 63, 64]

    def sentence(n):
        return [2] + rng.choice(alphabet, n - 2, p=weights).tolist() + [3]

    cands, refs = [], []
    for e in range(E):
        n = lengths[e % 8] if e % 8 < 4 else int(rng.integers(2, 65))
        cands.append(sentence(n))
        refs.append([sentence(lengths[(e + j) % 4] if (e + j) % 5 == 0 else int(rng.integers(2, 65))) for j in range(1 + e % 9)])
    cands[10] = list(refs[10][1])                                         # a candidate identical to one of its references
    cands[11], refs[11][0] = list(range(100, 164)), list(range(200, 264))    # a 64-token pair that shares nothing
    assert {len(c) for c in cands} >= {2, 3, 63, 64} and {len(r) for r in refs} == set(range(1, 10))
    # corpus rows in shuffled order: slot_row is not the identity
    flat = [(e, j) for e in range(E) for j in range(len(refs[e]))]
    place = rng.permutation(len(flat))
    tokens, lens = np.zeros((len(flat), 64), np.int32), np.zeros(len(flat), np.int32)
    slot_row, u_off = [], [0]
    for i, (e, j) in enumerate(flat):
        r = refs[e][j]
        tokens[place[i], :len(r)], lens[place[i]] = r, len(r)
        slot_row.append(int(place[i]))
        if j == len(refs[e]) - 1:
            u_off.append(len(slot_row))
    cand, clen = np.zeros((E, 64), np.int32), np.array([len(c) for c in cands], np.int32)
    for e, c in enumerate(cands):
        cand[e, :len(c)] = c
    want_stats = np.array([R.bleu_counts(cands[e], refs[e]) for e in range(E)])
    want_lcs = np.array([R.lcs_bits(cands[e], refs[e][j]) for e, j in flat])
    d = lambda a: torch.from_numpy(np.asarray(a, np.int32)).to(dev)
    t = dict(cand=d(cand), clen=d(clen), tokens=d(tokens), lens=d(lens), slot_row=d(slot_row), u_off=d(u_off))
    stats = torch.full((E, 6), -7, dtype=torch.int32, device=dev)
    lcs = torch.full((len(flat),), -7, dtype=torch.int32, device=dev)
    p = lambda x: C.c_void_p(x.data_ptr())
    with torch.cuda.device(dev):
        rc = _lib.lib().d3_caption_stats(p(t["cand"]), 64, p(t["clen"]), p(t["tokens"]), 64, p(t["lens"]), p(t["slot_row"]), p(t["u_off"]), E,
                                         p(stats), p(lcs), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    assert (stats.cpu().numpy() == want_stats).all() and (lcs.cpu().numpy() == want_lcs).all()
    assert want_lcs[flat.index((10, 1))] == len(cands[10]) and want_lcs[flat.index((11, 0))] == 0 and want_stats[11, :4].tolist() == [0] * 4
    assert _lib.lib().d3_caption_stats(p(t["cand"]), 64, p(t["clen"]), p(t["tokens"]), 64, p(t["lens"]), p(t["slot_row"]), p(t["u_off"]), 0,
                                       p(stats), p(lcs), None) == -3


def test_evaluator_on_the_golden_inputs(dev, golden):
    from d3net_amd import caption_eval as ce
    inp, batch, host = golden
    g = np.load(os.path.join(HERE, "golden", "caption_eval_golden.npz"))
    ev = ce.CaptionEvaluator(inp["raw"], inp["vocab"], max_len=30, device=dev)
    ev.add_batch(batch)
    got = ev.candidates()
    assert sorted(got) == sorted(host) == g["keys"].tolist()
    assert [got[k]["caption"] for k in sorted(got)] == [host[k]["caption"] for k in sorted(got)] == g["captions"].tolist()
    diff = max(abs(got[k]["iou"] - host[k]["iou"]) for k in got)
    print("max IoU difference", diff)
    assert diff <= 1e-6
    assert min(abs(v["iou"] - thr) for v in host.values() for thr in THRESHOLDS) >= 3.8e-4       # no candidate sits on a threshold
    for thr in THRESHOLDS:
        res = ev.compute(thr)
        _assert_epoch_equal(res, ce.eval_caption_epoch(host, inp["raw"], max_len=30, min_iou=thr))
        assert ev.keys == g["corpus_keys"].tolist()
        bleu, cider, rouge, _ = res
        assert abs(cider[0] - float(g["cider_%s" % thr])) <= 1e-9 * abs(float(g["cider_%s" % thr]))
        assert np.allclose(cider[1], g["cider_scores_%s" % thr], rtol=1e-9, atol=1e-12)
        assert np.allclose(bleu[0], g["bleu_%s" % thr], rtol=1e-12) and np.allclose(bleu[1], g["bleu_list_%s" % thr], rtol=1e-12)
        assert abs(rouge[0] - float(g["rouge_%s" % thr])) < 1e-12 and np.allclose(rouge[1], g["rouge_scores_%s" % thr], rtol=1e-12)
    ev.reset()
    assert ev.candidates() == {}


def test_merge_rule_over_an_epoch(dev, golden):
    """batches [s0, s1, s9], [s1', s2 without its last two objects], [s2'', s2''', an unknown scene]: the first batch wins, within a
    batch the last (b, g); s9 has descriptions and an all-zero GT mask (its keys leave the entries), one GT object of s0 has no
    description, one described object of s0 never appears (it scores as "sos eos")"""
    from d3net_amd import caption_eval as ce
    inp, _, _ = golden
    rng = np.random.default_rng(77)
    ids0 = inp["gt_box_ids"][0][inp["gt_box_masks"][0] == 1]
    orphan = int(ids0[0])
    raw = [d for d in inp["raw"] if not (d["scene_id"] == "scene0000_00" and d["object_id"] == str(orphan))]
    raw.insert(3, {"scene_id": "scene0000_00", "object_id": "45", "token": ["w1", "w2", "w3"]})        # permutation(40): never a GT id
    raw += [{"scene_id": "scene0009_00", "object_id": d["object_id"], "token": d["token"]} for d in inp["raw"] if d["scene_id"] == "scene0001_00"]

    def variant(seed):
        r = np.random.default_rng(seed)
        v = dict(inp)
        caps = r.integers(4, 60, inp["pred_captions"].shape).astype(np.int64)
        caps[r.random(caps.shape) < 0.08] = 3
        v["pred_captions"] = caps
        v["pred_boxes"] = (inp["pred_boxes"] + r.normal(0, 0.02, inp["pred_boxes"].shape)).astype(np.float32)
        return v

    def cat(parts, names):
        """parts: (inputs, scene) pairs -> one batch"""
        bs = [_batch(v, dev, [s]) for v, s in parts]
        out = {k: torch.cat([b[k] for b in bs]) for k in bs[0] if k != "scene_id"}
        out["scene_id"] = list(names)
        return out

    b1 = cat([(inp, 0), (inp, 1), (inp, 1)], ["scene0000_00", "scene0001_00", "scene0009_00"])
    b1["gt_bbox_label"][2] = 0
    b2 = cat([(variant(1), 1), (inp, 2)], ["scene0001_00", "scene0002_00"])
    n2 = int(inp["gt_box_masks"][2].sum())
    b2["gt_bbox_label"][1, n2 - 2:] = 0
    b3 = cat([(variant(2), 2), (variant(3), 2), (variant(4), 0)], ["scene0002_00", "scene0002_00", "somewhere_else"])
    batches = [b1, b2, b3]
    ev = ce.CaptionEvaluator(raw, inp["vocab"], max_len=30, device=dev)
    merged = {}
    for b in batches:
        ev.add_batch(b)
        for k, v in ce.eval_caption_step(dict(b), inp["vocab"]).items():
            merged.setdefault(k, v)
    got = ev.candidates()
    described = {"%s|%s" % (d["scene_id"], d["object_id"]) for d in raw}
    assert set(got) == set(merged) & described
    assert "scene0000_00|%d" % orphan in merged and "scene0000_00|45" not in got and not any(k.startswith("scene0009") for k in got)
    last_two = ["scene0002_00|%d" % i for i in inp["gt_box_ids"][2][n2 - 2:n2]]
    single = ce.eval_caption_step(dict(b3), inp["vocab"])
    for k in last_two:                                                    # they first appear in batch 3, twice: the second copy wins
        assert got[k]["caption"] == merged[k]["caption"] == single[k]["caption"]
    assert all(got[k]["caption"] == merged[k]["caption"] and abs(got[k]["iou"] - merged[k]["iou"]) <= 1e-6 for k in got)
    for thr in THRESHOLDS:
        res = ev.compute(thr)
        _assert_epoch_equal(res, ce.eval_caption_epoch(merged, raw, max_len=30, min_iou=thr))
        assert ev.keys == list(ce.prepare_corpus(raw, merged, 30)) and not any(k.startswith("scene0009") for k in ev.keys)
        e45 = ev.keys.index("scene0000_00|45")
        assert res[0][1][0][e45] == ce.eval_caption_epoch({"scene0000_00|45": {"caption": "sos eos", "iou": 1.0}}, raw[3:4], 30, thr)[0][1][0][0]


def test_add_batch_reads_nothing_back(dev, golden, monkeypatch):
    from d3net_amd import caption_eval as ce
    inp, batch, host = golden
    ev = ce.CaptionEvaluator(inp["raw"], inp["vocab"], max_len=30, device=dev)

    def refuse(*a, **k):
        raise AssertionError("add_batch read a tensor back")

    with monkeypatch.context() as m:
        for name in ("cpu", "item", "tolist", "numpy"):
            m.setattr(torch.Tensor, name, refuse)
        assert ev.add_batch(batch) is None
    got = ev.candidates()
    assert {k: v["caption"] for k, v in got.items()} == {k: v["caption"] for k, v in host.items()}


def test_evaluate_captioning_equals_the_validation_hooks(dev):
    from d3net_amd import synthetic as S
    from d3net_amd.pipeline import PipelineNet
    from test_pipeline_gpu import _cfg
    V = 200
    scenes = [S.small_scene(dims=(40, 32, 20), n_boxes=3, seed=s) for s in (3, 4)]
    chunked, organized = S.make_language_corpus(2, chunk=4, vocab=V, objects_per_scene=3)
    tr = types.SimpleNamespace(vocabulary=S.make_vocabulary(V), glove=np.random.default_rng(0).standard_normal((V, 300)).astype(np.float32),
                               chunked_data=chunked, organized=organized, raw_data=S.corpus_raw_data(organized))
    net = PipelineNet(_cfg(no_captioning=False, no_grounding=True), {"train": tr, "val": tr}).to(dev).eval()
    net.detector.teacher = True
    batch = S.add_language(S.make_batch(scenes, dev), dev, chunk=4, vocab=V)
    batch["lang_len"] = batch["spk_lang_len"]
    want = net.validation_epoch_end([net.validation_step(dict(batch), 0)])
    got = net.evaluate_captioning([dict(batch)])
    print(got, want)
    assert list(got) == list(want) and not net.training
    for k in want:
        if k == "cider":
            assert abs(got[k] - want[k]) <= 1e-12 * abs(want[k])
        else:
            assert got[k] == want[k]
    net0 = PipelineNet(_cfg(no_captioning=True, no_grounding=True), {"train": tr, "val": tr})
    with pytest.raises(NotImplementedError):
        net0.evaluate_captioning([])


def test_bad_input_is_refused(dev, golden):
    from d3net_amd import _lib, caption_eval as ce
    inp, batch, _ = golden
    ev = ce.CaptionEvaluator(inp["raw"], inp["vocab"], max_len=30, device=dev)
    launches = []
    orig = ce._assign_launch
    ce._assign_launch = lambda *a, **k: launches.append(1) or orig(*a, **k)
    try:
        for key in ("lang_cap", "gt_bbox", "gt_bbox_label"):
            bad = dict(batch); bad[key] = batch[key].cpu()
            with pytest.raises(ValueError, match=key):
                ev.add_batch(bad)
        bad = dict(batch); bad["lang_cap"] = torch.zeros((3, 128, 63), dtype=torch.int64, device=dev)
        with pytest.raises(ValueError, match="T = 63"):
            ev.add_batch(bad)
        B, G = 4097, 256                                                  # B * G = 2^20 + 256
        big = dict(lang_cap=torch.zeros((B, 1, 1), dtype=torch.int64, device=dev), proposal_bbox_batched=torch.zeros((B, 1, 8, 3), device=dev),
                   gt_bbox=torch.zeros((B, G, 8, 3), device=dev), gt_bbox_object_id=torch.zeros((B, G), dtype=torch.int64, device=dev),
                   gt_bbox_label=torch.zeros((B, G), device=dev), scene_id=["x"] * B)
        with pytest.raises(ValueError, match="1048832"):
            ev.add_batch(big)
        bad = dict(batch); bad["gt_bbox_object_id"] = batch["gt_bbox_object_id"].float()
        with pytest.raises(ValueError, match="dtype"):
            ev.add_batch(bad)
        assert not launches and ev.candidates() == {}
    finally:
        ce._assign_launch = orig
    p = lambda x: C.c_void_p(x.data_ptr())
    z = torch.zeros(64, dtype=torch.int64, device=dev)
    args = lambda B, G, T: (p(z), p(z), p(z), p(z), p(z), p(z), p(z), p(z), p(z), None, B, 1, G, T, 60, 1, 1, 1, 2, 3, 0, p(z), p(z), p(z), p(z),
                            p(z), p(z), None)
    assert _lib.lib().d3_caption_collect(*args(1, 1, 63)) == -2 and _lib.lib().d3_caption_collect(*args(4097, 256, 4)) == -2
    # a token outside the vocabulary in a winning record: the host raises KeyError in its decode, compute raises D3Error
    bad = dict(batch); bad["lang_cap"] = batch["lang_cap"].clone()
    bad["lang_cap"][:, :, 0] = 60
    ev.add_batch(bad)
    with pytest.raises(_lib.D3Error, match="vocabulary"):
        ev.compute()
    with pytest.raises(KeyError):
        ce.eval_caption_step(dict(bad), inp["vocab"])
    # ... and after the eos it is never decoded: no error
    ev.reset()
    ok = dict(batch); ok["lang_cap"] = batch["lang_cap"].clone()
    ok["lang_cap"][:, :, 5] = 3
    ok["lang_cap"][:, :, 6:] = -5
    ev.add_batch(ok)
    want = ce.eval_caption_step(dict(ok), inp["vocab"])
    _assert_epoch_equal(ev.compute(0.25), ce.eval_caption_epoch(want, inp["raw"], max_len=30, min_iou=0.25))
