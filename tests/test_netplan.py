"""The native U-Net executor's plan (csrc/unet.hip: d3_net_create decides, d3_net_plan lays out), read through d3_net_describe /
NativeUNet.describe() on the CPU -- the planner is pure host code -- for the programs the product builds:

  1. every decision that does not depend on row counts equals tests/golden/netplan_golden.json (recorded from the planner as it was
     before its decisions were gathered into one gradient-view table and per-op call descriptors: gen_netplan_golden.py);
  2. the weight-gradient partial buffer is sized from the very flag word the backward launches with;
  3. the two arenas' regions are aligned, disjoint, inside the arena, sized by their storage type, and only the second-level
     partial tables lie in the areas zeroed per call.

Grid-derived sizes read the device's compute-unit count (256 without a device); the conditions hold for any."""
import ctypes as C
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import gen_netplan_golden as G  # noqa: E402

ROWS = ((142920, 35127, 8282), (37, 9, 3, 1))
CASE_IDS = ["%s/%s" % c for c in G.CASES]
_cache = {}


def _case(built_lib, case):
    """(executor, describe() per row vector) of a case, built once"""
    if case not in _cache:
        program, var = case
        ex, _ = G.describe_case(program, var, ROWS[0])
        descs = []
        for first in ROWS:
            rows = G.level_rows(first, ex.nlevels)
            descs.append((rows, ex.describe(rows)))
        _cache[case] = (ex, descs)
    return _cache[case]


@pytest.fixture(scope="module")
def golden():
    return G.load_golden()


@pytest.mark.parametrize("case", G.CASES, ids=CASE_IDS)
def test_decisions_equal_the_recorded_ones(built_lib, golden, case):
    ex, descs = _case(built_lib, case)
    want = golden["%s/%s" % case]
    for rows, desc in descs:
        got = G.decisions(desc)
        assert got["header"] == want["header"]
        for key in ("ops", "tensors", "bufs"):
            assert len(got[key]) == len(want[key]), key
            for i, (g, w) in enumerate(zip(got[key], want[key])):
                assert g == w, (key, i, {k: (g[k], w[k]) for k in w if g.get(k) != w[k]})
    # the named record widths are the library's
    assert desc["header"]["nops"] == len(ex.b.ops) and desc["header"]["ntensors"] == len(ex.b.tensors) and desc["header"]["nbufs"] == len(ex.b.bufs)


@pytest.mark.parametrize("case", G.CASES, ids=CASE_IDS)
def test_weight_gradient_partials_are_sized_from_the_launch_word(built_lib, case):
    from d3net_amd import _lib
    from d3net_amd.netexec import OP_CONV
    ex, descs = _case(built_lib, case)
    L = _lib.lib()
    seen = 0
    for rows, desc in descs:
        for op, rec in zip(ex.b.ops, desc["ops"]):
            if op[0] != OP_CONV or not ex.b.grad_params[op[4]]:
                continue
            Min, Mout, K = rows[ex.b.tensors[op[1]][0]], rows[ex.b.tensors[op[2]][0]], op[7]
            args = (Min, Mout, K, rec["Cin"], rec["Cout"], rec["wgrad_flags"])
            assert rec["wsplits"] == L.d3_spconv_wgrad2_splits(*args), (op, rec)
            assert rec["wpart_bytes"] >= L.d3_spconv_wgrad2_ws_bytes(*args), (op, rec)
            assert rec["wpart_bytes"] >= rec["wsplits"] * K * rec["Cin"] * rec["Cout"] * 4      # what the batched reduction reads
            seen += 1
    assert seen >= 2 * 3


def _regions(desc):
    """-> (arena regions, gradient-arena regions, second-level tables of the arena, of the gradient arena) as (name, off, bytes)"""
    a, g, a2, g2 = [], [], [], []
    h = desc["header"]
    for i, b in enumerate(desc["bufs"]):
        a.append(("buf%d" % i, b["off"], b["bytes"]))
        g.append(("gbuf%d" % i, b["goff"], b["gbytes"]))
        g.append(("gshadow%d" % i, b["gshadow_off"], b["gshadow_bytes"]))
    for i, o in enumerate(desc["ops"]):
        for k in ("wp_fwd", "wp_bwd", "part", "state"):
            a.append(("op%d.%s" % (i, k), o[k + "_off"], o[k + "_bytes"]))
        for k in ("bpart", "wpart"):
            g.append(("op%d.%s" % (i, k), o[k + "_off"], o[k + "_bytes"]))
        a2.append(("op%d.part2" % i, o["part2_off"], o["part2_bytes"]))
        g2.append(("op%d.bpart2" % i, o["bpart2_off"], o["bpart2_bytes"]))
    g.append(("bnscr", h["bnscr_off"], h["bnscr_bytes"]))
    g.append(("wgws", h["wgws_off"], h["wgws_bytes"]))
    keep = lambda rs: [r for r in rs if r[2] > 0]      # noqa: E731  (a region of no bytes takes no place)
    return keep(a), keep(g), keep(a2), keep(g2)


def _check_arena(regions, second, total, zero_off, zero_bytes):
    for name, off, nbytes in regions + second:
        assert 0 <= off and off + nbytes <= total, (name, off, nbytes, total)
        assert off % 256 == 0, (name, off)
    order = sorted(regions + second, key=lambda r: r[1])
    for (n0, o0, b0), (n1, o1, b1) in zip(order, order[1:]):
        assert o0 + b0 <= o1, (n0, o0, b0, n1, o1)
    for name, off, nbytes in second:
        assert zero_off <= off and off + nbytes <= zero_off + zero_bytes, (name, off, nbytes, zero_off, zero_bytes)
    for name, off, nbytes in regions:
        assert off + nbytes <= zero_off or off >= zero_off + zero_bytes, (name, off, nbytes, zero_off, zero_bytes)
    assert 0 <= zero_off and zero_off + zero_bytes <= total


@pytest.mark.parametrize("case", G.CASES, ids=CASE_IDS)
def test_arena_layout_invariants(built_lib, case):
    from d3net_amd import _lib
    ex, descs = _case(built_lib, case)
    L = _lib.lib()
    al = lambda x: (x + 255) // 256 * 256      # noqa: E731
    for rows, desc in descs:
        h = desc["header"]
        assert h["planned"] == 1
        ex._plan_for(rows)      # (the offsets the library answers with are those of its current plan)
        a, g, a2, g2 = _regions(desc)
        assert a2 and (g2 or not any(o["fused_by"] >= 0 for o in desc["ops"]))
        _check_arena(a, a2, h["arena_bytes"], h["cnt_off0"], h["cnt_bytes"])
        _check_arena(g, g2, h["grad_bytes"], h["bcnt_off0"], h["bcnt_bytes"])
        for (level, width, dtype), b in zip(ex.b.bufs, desc["bufs"]):
            assert b["bytes"] == al(rows[level] * width * (2 if dtype == 1 else 4))
            if b["need_grad"]:
                assert b["gbytes"] == al(rows[level] * width * (2 if (b["gbf"] or b["gabf"]) else 4)), b
            else:
                assert b["gbytes"] == 0
            assert b["gshadow_bytes"] == (al(rows[level] * b["gshadow"] * 2) if b["gshadow"] else 0)
        for t, (level, Cc, width, coff, dtype, buf) in enumerate(ex.b.tensors):
            off = L.d3_net_tensor_offset(ex._net(), t)
            assert off == (-1 if buf < 0 else desc["bufs"][buf]["off"] + coff * (2 if dtype == 1 else 4))
            v = desc["tensors"][t]
            if v["kind"] == 2:      # a gradient-arena view: inside its root buffer's gradient region
                assert v["goff"] == desc["bufs"][v["root"]]["goff"] + v["coff"] * (2 if v["bf16"] else 4)
                assert v["ld"] == ex.b.bufs[v["root"]][1] and v["coff"] + Cc <= v["ld"]
            else:
                assert v["goff"] == -1 and v["root"] == (-1 if v["kind"] == 0 else -2)
        # planning the same rows again gives the same description
        ex._plan_key = None
        assert ex.describe(rows) == desc


def test_describe_reports_its_size_first(built_lib):
    from d3net_amd import _lib
    from d3net_amd.netexec import DESCRIBE_BUF, DESCRIBE_HEADER, DESCRIBE_OP, DESCRIBE_TENSOR
    ex, descs = _case(built_lib, ("scorenet", "default"))
    L = _lib.lib()
    nw = L.d3_net_describe(ex._net(), None, 0)
    b = ex.b
    assert nw == len(DESCRIBE_HEADER) + len(b.ops) * len(DESCRIBE_OP) + len(b.tensors) * len(DESCRIBE_TENSOR) + len(b.bufs) * len(DESCRIBE_BUF)
    short = (C.c_int64 * nw)(*([-7] * nw))
    assert L.d3_net_describe(ex._net(), short, nw - 1) == nw and all(v == -7 for v in short)      # too small: nothing written
