"""The integer side of the device captioning evaluation, pinned on the CPU: the rules of csrc/caption_eval.hip as restated in
tests/caption_stats_restate.py, pushed through caption_metrics.bleu_from_counts / rouge_from_lcs, equal bleu_scores /
rouge_l_scores on the strings (==, corpus and per entry) and the reference's golden numbers; EvalCorpus is prepare_corpus as
token ids and refuses what the kernels cannot hold."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import caption_stats_restate as R  # noqa: E402


def _ids(sentences, table):
    return [[table.setdefault(w, len(table)) for w in s.split(" ")] for s in sentences]


def _restated_scores(refs, cands):
    """strings -> (bleu, rouge) from the restated integer rules and the floating-point halves"""
    from d3net_amd import caption_metrics as cm
    table = {}
    counts, entries = [], []
    for rs, c in zip(refs, cands):
        ri, ci = _ids(rs, table), _ids([c], table)[0]
        counts.append(R.bleu_counts(ci, ri))
        entries.append((len(ci), [len(r) for r in ri], [R.lcs_bits(ci, r) for r in ri]))
    return cm.bleu_from_counts(counts, 4), cm.rouge_from_lcs(entries)


def _assert_same(refs, cands):
    from d3net_amd import caption_metrics as cm
    bleu, rouge = _restated_scores(refs, cands)
    hb, hr = cm.bleu_scores(refs, cands, 4), cm.rouge_l_scores(refs, cands)
    assert bleu[0] == hb[0] and bleu[1] == hb[1]
    assert rouge[0] == hr[0] and rouge[1].tolist() == hr[1].tolist()
    return bleu, rouge


@pytest.fixture(scope="module")
def golden_candidates():
    from gen_caption_eval_golden import caption_inputs
    from d3net_amd import caption_eval as ce
    inp = caption_inputs()
    t = {k: torch.from_numpy(v) for k, v in inp.items() if isinstance(v, np.ndarray)}
    cands = ce.assign_dense_caption(t["pred_captions"], t["pred_boxes"], t["gt_boxes"], t["gt_box_ids"], t["gt_box_masks"],
                                    inp["scene_list"], inp["vocab"]["idx2word"], inp["vocab"]["special_tokens"])
    return inp, cands


@pytest.mark.parametrize("thr", [0.25, 0.5])
def test_restated_counts_give_the_host_scores_on_the_golden_candidates(golden_candidates, thr):
    from d3net_amd import caption_eval as ce
    inp, cands = golden_candidates
    g = np.load(os.path.join(HERE, "golden", "caption_eval_golden.npz"))
    corpus = ce.prepare_corpus(inp["raw"], cands, 30)
    kept = {k: v["caption"] for k, v in cands.items() if v["iou"] >= thr}
    keys = list(corpus)
    bleu, rouge = _assert_same([corpus[k] for k in keys], [kept.get(k, "sos eos") for k in keys])
    assert np.allclose(bleu[0], g["bleu_%s" % thr], rtol=1e-12) and np.allclose(bleu[1], g["bleu_list_%s" % thr], rtol=1e-12)
    assert abs(rouge[0] - float(g["rouge_%s" % thr])) < 1e-12 and np.allclose(rouge[1], g["rouge_scores_%s" % thr], rtol=1e-12)


def test_restated_counts_on_a_five_word_vocabulary():
    """200 random entries over 5 words: 2- to 4-grams repeat inside a sentence, so the clipping and the first-occurrence rule bite"""
    rng = np.random.default_rng(5)
    words = ["a", "b", "c", "d", "e"]
    sent = lambda n: "sos " + " ".join(words[i] for i in rng.integers(0, 5, n)) + " eos" if n else "sos eos"
    refs = [[sent(int(rng.integers(0, 63))) for _ in range(int(rng.integers(1, 10)))] for _ in range(200)]
    cands = [sent(int(rng.integers(0, 63))) for _ in range(200)]
    cands[3] = refs[3][0]
    cands[4], refs[4] = "sos " + " ".join(["a"] * 62) + " eos", ["sos " + " ".join(["a", "b"] * 31) + " eos"]
    _assert_same(refs, cands)
    table = {}
    clipped = 0
    for rs, c in zip(refs, cands):
        ci, ri = _ids([c], table)[0], _ids(rs, table)
        row = R.bleu_counts(ci, ri)
        unclipped = [sum(1 for p in range(len(ci) - k + 1) if any(ci[p:p + k] == r[q:q + k] for r in ri for q in range(len(r) - k + 1)))
                     for k in (1, 2, 3, 4)]
        clipped += sum(a < b for a, b in zip(row[:4], unclipped))
    assert clipped > 100          # the fixture does exercise the clipping


def test_bit_vector_lcs_equals_the_dynamic_programme():
    from d3net_amd.caption_metrics import _lcs
    rng = np.random.default_rng(9)
    for _ in range(2000):
        alpha = int(rng.integers(2, 61))
        a = rng.integers(0, alpha, int(rng.integers(0, 65))).tolist()
        b = rng.integers(0, alpha, int(rng.integers(0, 65))).tolist()
        assert R.lcs_bits(a, b) == _lcs(a, b)
    full = list(range(64))
    assert R.lcs_bits(full, full) == 64 and R.lcs_bits(full, [100 + i for i in range(64)]) == 0 and R.lcs_bits(full, full[::-1]) == 1


def test_closest_length_and_merge_priority():
    assert R.closest_length(10, [12, 8, 13]) == 8 and R.closest_length(10, [12, 9, 11]) == 9 and R.closest_length(2, [7]) == 7
    for testlen in range(1, 20):
        lens = [3, 17, 9, 9, 12]
        assert R.closest_length(testlen, lens) == min((abs(l - testlen), l) for l in lens)[1]
    # the host's merge: candidates[key] = ... inside a batch (the last (b, g) wins), setdefault across batches (the first wins)
    rng = np.random.default_rng(2)
    G = 7
    records, host = [], {}
    for seq in range(4):
        batch = {}
        for b in range(3):
            for g in range(G):
                key = "k%d" % rng.integers(0, 12)
                batch[key] = (seq, b, g)
                records.append((seq, b, g, G, key))
        for k, v in batch.items():
            host.setdefault(k, v)
    order = rng.permutation(len(records))
    assert R.merge_owner([records[i] for i in order]) == host
    assert R.priority(0, 0, 0, 1) == (1 << 20) - 1 and R.priority(1, 0, 0, 1) > R.priority(0, 0, 0, 1) > R.priority(0, 1, 3, 4)


def test_eval_corpus_is_prepare_corpus_as_token_ids():
    from gen_caption_eval_golden import caption_inputs
    from d3net_amd import caption_eval as ce
    inp = caption_inputs()
    raw = [dict(d) for d in inp["raw"]]
    raw[0]["token"] = raw[0]["token"] + ["zebra", "zebra", "quagga"]             # words outside the vocabulary
    raw[1]["token"] = ["w3"] * 40                                              # cut at max_len
    vocab = {"idx2word": dict(inp["vocab"]["idx2word"]), "special_tokens": inp["vocab"]["special_tokens"]}
    vocab["idx2word"]["60"] = "w5"                                             # a second id spelling w5
    c = ce.EvalCorpus(raw, vocab["idx2word"], vocab["special_tokens"], 30, "cpu")
    fake = {"%s|x" % s: None for s in inp["scene_list"]}
    corpus = ce.prepare_corpus(raw, fake, 30)
    assert c.keys == list(corpus)
    tok, lens = c.tokens.numpy(), c.lens.numpy()
    for s, k in enumerate(c.keys):
        assert [c.decode(tok[r, :lens[r]]) for r in range(c.row_off[s], c.row_off[s + 1])] == corpus[k]
    assert tok.max() == 62 and tok.dtype == np.int32 and lens.max() == 32 and c.V == 61
    lut = c.lut.numpy()
    assert lut[60] == lut[9] == 9 and (lut[:60] == np.arange(60)).all()
    slot_of = c.slot_of.numpy()
    assert slot_of.dtype == np.int32 and slot_of.shape[0] == 3 and (slot_of >= 0).sum() == len(c.keys)
    for s, k in enumerate(c.keys):
        scene, oid = k.split("|")
        assert slot_of[c.scene_index[scene], int(oid)] == s
    # one scene only: the other scenes' keys leave prepare_corpus, the slots stay numbered
    assert [k for k in c.keys if k.startswith("scene0001")] == list(ce.prepare_corpus(raw, {"scene0001_00|0": None}, 30))


@pytest.mark.parametrize("case,match", [("long", "66 tokens"), ("space", "whitespace"), ("empty", "whitespace"), ("object", "4096"),
                                        ("negative", "-1"), ("ngrams", "2160 n-gram"), ("ids", "65534")])
def test_eval_corpus_limits_raise(case, match):
    from d3net_amd import caption_eval as ce
    words = ["pad_", "unk", "sos", "eos", "a", "b"]
    idx2word = {str(i): w for i, w in enumerate(words)}
    special = {"bos_token": "sos", "eos_token": "eos", "unk_token": "unk", "pad_token": "pad_"}
    d = lambda tok, oid="3": {"scene_id": "s0", "object_id": oid, "token": tok}
    raw, max_len = [d(["a", "b"])], 30
    if case == "long":
        raw, max_len = [d(["a"] * 64)], 100
    elif case == "space":
        raw = [d(["a", "b c"])]
    elif case == "empty":
        raw = [d(["a", ""])]
    elif case == "object":
        raw = [d(["a"], "4096")]
    elif case == "negative":
        raw = [d(["a"], "-1")]
    elif case == "ngrams":
        raw = [d(["a"] * 28) for _ in range(18)]                                   # 18 rows of 30 tokens: 2160 positions
    elif case == "ids":
        idx2word = {str(i): "v%d" % i for i in range(65535)}
        idx2word["2"], idx2word["3"] = "sos", "eos"
    with pytest.raises(ValueError, match=match):
        ce.EvalCorpus(raw, idx2word, special, max_len, "cpu")
    if case == "ngrams":
        ce.EvalCorpus(raw[:17], idx2word, special, max_len, "cpu")                  # 2040 positions fit
    if case == "long":
        ce.EvalCorpus([d(["a"] * 62)], idx2word, special, 100, "cpu")               # 64 tokens fit
