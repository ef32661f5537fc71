"""The C-ABI library builds for gfx950, loads, and exports every symbol include/d3hip.h declares."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    names = set()
    for h in os.listdir(os.path.join(ROOT, "include")):
        if h.endswith(".h"):
            txt = open(os.path.join(ROOT, "include", h)).read()
            txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
            names |= set(re.findall(r"\b(d3_[a-z0-9_]+)\s*\(", txt))
    return names


def test_every_declared_symbol_is_exported(built_lib):
    lib = ctypes.CDLL(built_lib)
    decl = _declared()
    assert len(decl) >= 20
    missing = [n for n in sorted(decl) if not hasattr(lib, n)]
    assert not missing, missing


def test_binding_table_matches_header(built_lib):
    from d3net_amd import _lib
    assert set(_lib.SIGNATURES) == _declared()
    # the clustering's entry points: the two size queries, the one-call form and its two halves -- no earlier generation beside them
    assert {n for n in _declared() if n.startswith("d3_bfs_cluster_")} == \
        {"d3_bfs_cluster_" + s for s in ("ws_bytes", "erec_bytes", "run", "begin", "end")}
    l = _lib.lib()
    assert l.d3_arch() == b"gfx950"
    assert l.d3_version() >= 100


def test_host_side_constants(built_lib):
    """Pure host entry points (no GPU): the padded ball query's slot size is the reference's 1000-neighbour cap
    (src/bfs_cluster/bfs_cluster.cu:38-44) and the AdamW chunk matches the block map d3net_amd.optim builds."""
    from d3net_amd import _lib
    l = _lib.lib()
    assert l.d3_ballquery_cap() == 1000
    assert l.d3_adamw_chunk() == 4096
    assert l.d3_bfs_cluster_erec_bytes(10) == 160
    assert l.d3_bfs_cluster_ws_bytes(1000) > 17 * 4 * 1000
    # the padded lists' range (round 5): n * cap slots inside start_len's int range -- the library's own bound, not 2 GiB of slots
    from d3net_amd import pointgroup_ops as P
    assert P.ballquery_padded_fits(1) and P.ballquery_padded_fits(852_000) and P.ballquery_padded_fits(2_147_483)
    assert not P.ballquery_padded_fits(2_147_484) and not P.ballquery_padded_fits(0)
    assert P.ballquery_padded_fits(536_870, max_bytes=2 << 30) and not P.ballquery_padded_fits(536_871, max_bytes=2 << 30)


def test_product_never_imports_oracle():
    """d3net_amd/ must not reference oracle/ (no CPU fallback through the checker)."""
    bad = []
    for dp, _, fs in os.walk(os.path.join(ROOT, "d3net_amd")):
        for f in fs:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                t = open(os.path.join(dp, f), errors="ignore").read()
                if re.search(r"^\s*(from|import)\s+oracle\b|libpgoracle|pg_oracle", t, flags=re.M):
                    bad.append(os.path.join(dp, f))
    assert not bad, bad


def test_convolutions_hand_nothing_over_through_globals():
    """the convolution dispatchers and the U-Net executor pass tables and partial-row counts as arguments (csrc/conv.h): no
    thread-local hint, no second copy of the BatchNorm argument struct"""
    csrc = os.path.join(ROOT, "d3net_amd", "csrc")
    banned = ("d3_spconv_next_", "d3_spconv_set_last_nparts", "g_c2_inst", "struct Conv3Bn", "struct Conv2Bn")
    bad = [(f, w) for f in sorted(os.listdir(csrc)) for w in banned if w in open(os.path.join(csrc, f), errors="ignore").read()]
    assert not bad, bad
    for f in ("spconv2.hip", "wgrad.hip"):
        assert "thread_local" not in open(os.path.join(csrc, f)).read(), f


def test_workspace_layouts_are_written_once():
    """a workspace's regions are listed by ONE layout function that the run carves with and the *_ws_bytes query measures
    (D3Carver, csrc/common.h): no `(char *)ws... +` / `(const char *)ws... +` arithmetic in an expression (the offset-struct
    layouts of topdown.hip, whose runs add checked offsets to a `char *` alias, are not what this looks for), and the hgemm.hip
    helpers are declared once"""
    csrc = os.path.join(ROOT, "d3net_amd", "csrc")
    hips = [f for f in sorted(os.listdir(csrc)) if f.endswith(".hip")]
    assert len(hips) >= 20
    arith = re.compile(r"\(\s*(?:const\s+)?char\s*\*\s*\)\s*ws\w*[^;\n]*\+")
    decl = re.compile(r"^\s*(?:static\s+|extern\s+)?(?:int|size_t)\s+(hg_launch|hg_colsum_ws_bytes|hg_colsum_multi)\s*\(", re.M)
    bad = []
    for f in hips:
        t = open(os.path.join(csrc, f), errors="ignore").read()
        bad += [(f, m.group(0)) for m in arith.finditer(t)]
        if f != "hgemm.hip":
            bad += [(f, m.group(1)) for m in decl.finditer(t)]
    assert not bad, bad
    assert len(decl.findall(open(os.path.join(csrc, "hgemm.hip")).read())) == 3
    assert len(decl.findall(open(os.path.join(csrc, "common.h")).read())) == 3


def test_clustering_host_side_is_written_once():
    """csrc/cluster.hip: ONE loop waits for the stream between count iterations and ONE place launches the generic level loop for the
    clusters beyond the record form's LDS bitmap -- the blocking path and `end` share both; the 64-bit pair sort, which lost its
    caller, is gone"""
    csrc = os.path.join(ROOT, "d3net_amd", "csrc")
    t = open(os.path.join(csrc, "cluster.hip")).read()
    assert len(re.findall(r"cl_bfs_kernel\s*<<<[^;]*B2_MAXSIZE\s*\)\s*;", t)) == 1
    assert t.count("cl_bfs_kernel<<<") == 1 and t.count("hipStreamSynchronize") == 1
    bad = [f for f in sorted(os.listdir(csrc)) if "d3_sort_pairs_u64" in open(os.path.join(csrc, f), errors="ignore").read()]
    assert not bad, bad


def test_workspace_sizes_are_pinned(built_lib):
    """the size queries without rocPRIM scratch are pure arithmetic: the values of the hand-written formulas that the layout
    functions replaced"""
    from d3net_amd import _lib
    l = _lib.lib()
    assert l.d3_topdown_step_ws_bytes(8, 16, 512, 300, 128) == 61696
    assert l.d3_gru_seq_bwd_ws_bytes(8, 30, 300, 256) == 1581312
    assert l.d3_edgeconv_ws_bytes(160, 128, 128) == 245760
    assert l.d3_edgeconv_bwd_ws_bytes(160, 128, 128) == 868352
    assert l.d3_enet_ws_bytes(2, 64, 80) == 409600
    assert l.d3_cider_ws_bytes(40, 8, 4096) == 543744
    assert l.d3_scan_labels_ws_bytes(1000, 50, 60, 10, 20) == 4352
    assert l.d3_scan_mesh_ws_bytes(1000, 2000) == 36096
    assert l.d3_multiview_fuse_ws_bytes(4, 41, 32) == 2688000
    assert l.d3_lang_features_ws_bytes(8, 5) == 768
    assert l.d3_ref_targets_ws_bytes(2) == 256


def test_switch_table_stays_small(built_lib):
    """the library's measurement / cross-check switches live in ONE table (csrc/tuning.hip): at most 12, every name unique"""
    from d3net_amd import _lib
    l = _lib.lib()
    n = l.d3_tuning_count()
    names = [l.d3_tuning_name(i) for i in range(n)]
    assert n <= 12 and len(set(names)) == n and all(x.startswith(b"D3_") for x in names), names
