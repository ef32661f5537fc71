"""Host side of d3net_amd.lang_prep against tests/golden/lang_prep_golden.npz (the reference's own _tranform_des, _get_chunked_data,
_get_unique_multiple_lookup, _get_raw2label and __getitem__): token rows and counts, chunk lists, unique_multiple, object_cat, raw2label
from the fixture TSV, the draw sequence, the erased features through the host restatement, and the ValueError cases.  No GPU."""
import json
import os
import random
import types

import numpy as np
import pytest

import lang_prep_restate as LR
from d3net_amd import lang_prep as LP, scene_prep as SP

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "lang_prep_golden.npz"))
ANN = json.loads(str(G["annotations_json"]))
TSV = os.path.join(HERE, "golden", "lang_prep_labels.tsv")
SEED, MAX_DES_LEN, CHUNK = int(G["seed"]), int(G["max_des_len"]), int(G["chunk"])


def make_index(**kw):
    args = dict(raw_data=ANN["raw_data"], vocabulary=ANN["vocabulary"], glove=G["glove"], max_des_len=MAX_DES_LEN,
                num_des_per_scene=CHUNK, raw2label=LP.raw2label_from_tsv(TSV), scan2cad_rotation=ANN["scan2cad_rotation"])
    args.update(kw)
    return LP.DescriptionIndex(**args)


@pytest.fixture(scope="module")
def index():
    return make_index()


def test_raw2label_from_fixture_tsv():
    r2l = LP.raw2label_from_tsv(TSV)
    assert sorted(r2l) == [str(n) for n in G["raw2label_names"]]
    np.testing.assert_array_equal([r2l[str(n)] for n in G["raw2label_names"]], G["raw2label_values"])
    assert r2l["office chair"] == 2 and r2l["trash can"] == 17


def test_token_rows_and_counts(index):
    np.testing.assert_array_equal(index.token_ids, G["token_rows"])
    assert index.token_ids.dtype == np.int32 and index.token_ids.shape == (index.Nd, MAX_DES_LEN + 2)
    real = [n for n, d in enumerate(ANN["raw_data"]) if d["object_id"] != "SYNTHETIC"]
    np.testing.assert_array_equal(index.row[real], np.arange(len(real)))
    want = [min(len(ANN["raw_data"][n]["token"]), MAX_DES_LEN) + 2 for n in real]
    np.testing.assert_array_equal(index.token_len, want)
    assert (index.row[[n for n in range(len(ANN["raw_data"])) if n not in real]] == -1).all()
    unk = ANN["vocabulary"]["word2idx"]["unk"]
    assert index.token_ids[0, 3] == unk and index.unk == unk                       # the out-of-vocabulary word
    assert index.token_len[1] == MAX_DES_LEN + 2 and index.token_ids[1, -1] == ANN["vocabulary"]["word2idx"]["eos"]   # trimmed


def test_chunk_lists(index):
    assert [len(c) for c in index.chunks] == G["chunk_sizes"].tolist()
    np.testing.assert_array_equal(np.concatenate(index.chunks), G["chunk_entries"])
    assert [index.scene_id(i) for i in range(len(index))] == [str(s) for s in G["aug/scene_id"]]


def test_unique_multiple_and_object_cat(index):
    np.testing.assert_array_equal(index.unique_multiple, G["unique_multiple"])
    for i, c in enumerate(index.chunks):
        real = [j for j, n in enumerate(c) if index.row[n] >= 0]
        np.testing.assert_array_equal(index.object_cat[[c[j] for j in real]], G["aug/object_cat"][i, real])


def _sample_rows(index, d):
    return dict(rows=d["rows"], erase=d["erase"])


@pytest.mark.parametrize("global_rng", [False, True])
@pytest.mark.parametrize("run", ["aug", "plain"])
def test_draw_sequence_and_host_features(index, run, global_rng):
    """per sample the description draws, then the scene's (the augment matrix; the captioning config has no elastic and no crop):
    the next draws of both generators equal the recorded ones, and the restated features equal the reference's"""
    aug = run == "aug"
    if global_rng:
        random.seed(SEED)
        np.random.seed(SEED)
        rng = pyrng = None
    else:
        rng, pyrng = np.random.RandomState(SEED), random.Random(SEED)
    tcfg = types.SimpleNamespace(jitter=True, flip=True, rot=True)
    glove32 = G["glove"].astype(np.float32)
    store = LR.description_store(index.token_ids, index.token_len, glove32)
    for i in range(len(index)):
        d = LP.draw_descriptions(index, i, rng, pyrng, is_augment=aug)
        if aug:
            SP.augment_matrix(np.random if rng is None else rng, tcfg)
        a, b = (random.getstate(), np.random.get_state()) if global_rng else (pyrng.getstate(), rng.get_state())
        nxt = (random.random(), np.random.rand()) if global_rng else (pyrng.random(), rng.rand())
        assert nxt == tuple(G[run + "/next_draws"][i]), (i, nxt)
        if global_rng:
            random.setstate(a), np.random.set_state(b)
        else:
            pyrng.setstate(a), rng.set_state(b)
        feat, ids, lens = LR.lang_features(store, index.token_len, glove32, index.unk, d["rows"], d["erase"], index.L)
        np.testing.assert_array_equal(feat, G[run + "/lang_feat"][i])
        np.testing.assert_array_equal(ids, G[run + "/lang_ids"][i])
        np.testing.assert_array_equal(lens, G[run + "/lang_len"][i])
        np.testing.assert_array_equal(d["lang_len"], G[run + "/lang_len"][i])
        for k in LP._META:
            np.testing.assert_array_equal(d[k], G["%s/%s" % (run, k)][i], err_msg=k)
    if not aug:
        assert all(len(e) == 0 for e in d["erase"])


def test_plain_run_takes_no_draws(index):
    rng, pyrng = np.random.RandomState(1), random.Random(1)
    for i in range(len(index)):
        LP.draw_descriptions(index, i, rng, pyrng, is_augment=False)
    assert rng.rand() == np.random.RandomState(1).rand() and pyrng.random() == random.Random(1).random()


def test_erase_off_still_draws_the_head(index):
    """the reference's `and` chain (:108) draws random.random() before it looks at apply_word_erase"""
    rng, pyrng, ref = np.random.RandomState(1), random.Random(1), random.Random(1)
    d = LP.draw_descriptions(index, 0, rng, pyrng, is_augment=True, apply_word_erase=False)
    for _ in range(4):
        ref.random()
    assert pyrng.random() == ref.random() and rng.rand() == np.random.RandomState(1).rand()
    assert all(len(e) == 0 for e in d["erase"])


def _short_index(n_tokens):
    raw = [dict(ANN["raw_data"][0], token=["w1"] * n_tokens)]
    return make_index(raw_data=raw, scan2cad_rotation=None)


def _head_seed():
    return next(s for s in range(100) if random.Random(s).random() < 0.5)


def test_too_short_description_raises_value_error():
    """fewer than two tokens after trimming leave no candidate position: the reference fails there (IndexError), this raises
    ValueError -- only when the description is picked for erasing"""
    s = _head_seed()
    for n in (0, 1):
        idx = _short_index(n)
        with pytest.raises(ValueError, match="fewer than two tokens"):
            LP.draw_descriptions(idx, 0, np.random.RandomState(0), random.Random(s), is_augment=True)
        LP.draw_descriptions(idx, 0, np.random.RandomState(0), random.Random(s), is_augment=False)
        LP.draw_descriptions(idx, 0, np.random.RandomState(0), random.Random(s), is_augment=True, apply_word_erase=False)
    d = LP.draw_descriptions(_short_index(2), 0, np.random.RandomState(0), random.Random(s), is_augment=True)
    assert len(d["erase"][0]) == 0
    with pytest.raises(ValueError, match="fewer than two tokens"):              # max_des_len 1 trims every description below two
        LP.draw_descriptions(make_index(max_des_len=1), 0, np.random.RandomState(0), random.Random(s), is_augment=True)


def test_index_build_errors():
    with pytest.raises(ValueError, match="GloVe table"):
        make_index(glove=G["glove"][:20])
    dup = ANN["raw_data"] + [dict(ANN["raw_data"][0], token=["w1", "w2"])]
    with pytest.raises(ValueError, match="share scene / object / annotation"):
        make_index(raw_data=dup)
    make_index(raw_data=ANN["raw_data"] + [dict(ANN["raw_data"][0])])           # an exact repeat is the reference's overwrite: harmless


def test_table_bytes(index):
    ours, theirs = index.table_bytes()
    assert ours == index.Nd * index.L * 4 + index.Nd * 4 + 40 * 300 * 4 and theirs == index.Nd * index.L * 301 * 8
