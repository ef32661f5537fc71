#!/usr/bin/env python3
"""Generates tests/golden/netplan_golden.json: the decisions of the native U-Net executor's planner (csrc/unet.hip, d3_net_create)
for the programs the product builds, as `NativeUNet.describe()` returns them -- every field that does not depend on row counts.

The file was recorded from the executor BEFORE its planner was restructured: d3_net_describe was first added on top of the unchanged
planner, evaluating the flag words with the launch sites' own expressions and the gradient views with the run-time lookup, and the
file written then pins those decisions.  Regenerate it only when a decision is changed on purpose; run on any machine with the
library built (pure host code, no GPU):  python tests/golden/gen_netplan_golden.py"""
import contextlib
import functools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(HERE, "netplan_golden.json")

# program -> (stem input channels or None, plane multipliers, block, exact); the backbone and the ScoreNet as d3net_amd/pointgroup.py
# builds them from conf/pointgroup.yaml (m 16, blocks 1..7, cluster_blocks [1, 2], block_reps 2), the ScoreNet also with VGG blocks,
# and the three-level stem program of tests/test_executor_ops_gpu.py
PROGRAMS = {
    "backbone": (134, [1, 2, 3, 4, 5, 6, 7], "ResidualBlock", False),
    "backbone_exact": (134, [1, 2, 3, 4, 5, 6, 7], "ResidualBlock", True),
    "scorenet": (None, [1, 2], "ResidualBlock", False),
    "scorenet_vgg": (None, [1, 2], "VGGBlock", False),
    "stem3": (134, [1, 2, 3], "ResidualBlock", False),
}
VARIANTS = ("default", "grad_f32", "conv_out_f32")      # D3_GRAD_BF16=0; netexec.SINGLE_READER_BF16 = False
CASES = [(p, "default") for p in PROGRAMS] + [(p, v) for v in VARIANTS[1:] for p in ("backbone", "scorenet", "stem3")]

# fields of describe() that depend on the level sizes (offsets, byte sizes, grid-derived counts): not pinned
ROW_DEPENDENT = {
    "header": {"planned", "arena_bytes", "grad_bytes", "cnt_off0", "cnt_bytes", "bcnt_off0", "bcnt_bytes", "bnscr_off", "bnscr_bytes",
               "wgws_off", "wgws_bytes"},
    "ops": {"wsplits", "nparts_max", "bparts_max", "wp_fwd_off", "wp_fwd_bytes", "wp_bwd_off", "wp_bwd_bytes", "part_off", "part_bytes",
            "part2_off", "part2_bytes", "state_off", "state_bytes", "bpart_off", "bpart_bytes", "bpart2_off", "bpart2_bytes", "wpart_off",
            "wpart_bytes"},
    "tensors": {"goff"},
    "bufs": {"off", "bytes", "goff", "gbytes", "gshadow_off", "gshadow_bytes"},
}


def level_rows(first, nlevels):
    """`first` for the leading levels, then a quarter of the level above, at least 1"""
    rows = list(first[:nlevels])
    while len(rows) < nlevels:
        rows.append(max(1, rows[-1] // 4))
    return rows


@contextlib.contextmanager
def variant(name):
    from d3net_amd import _lib, netexec
    if name == "grad_f32":
        with _lib.tuning(D3_GRAD_BF16=0):
            yield
    elif name == "conv_out_f32":
        old = netexec.SINGLE_READER_BF16
        netexec.SINGLE_READER_BF16 = False
        try:
            yield
        finally:
            netexec.SINGLE_READER_BF16 = old
    else:
        yield


def make_executor(program):
    """the NativeUNet of `program`, built on the CPU the way PointGroup builds it"""
    import torch.nn as nn
    from d3net_amd import common, minkowski as ME, netexec
    from d3net_amd.config import default_conf
    cfg = default_conf()
    stem_in, mult, block, exact = PROGRAMS[program]
    m = cfg.model.m
    sp_norm = functools.partial(ME.MinkowskiBatchNorm, eps=1e-4, momentum=0.1)
    ublock = common.UBlock([m * c for c in mult], sp_norm, cfg.model.block_reps, getattr(common, block))
    if stem_in is not None:
        net = nn.Sequential(ME.MinkowskiConvolution(stem_in, m, kernel_size=3, bias=False, dimension=3), ublock, sp_norm(m),
                            ME.MinkowskiReLU(inplace=True))
        ME.fuse_bn_relu(net)
        return netexec.NativeUNet(net[0], net[1], net[2], stem_in, False, exact=exact)
    net = nn.Sequential(ublock, sp_norm(m), ME.MinkowskiReLU(inplace=True))
    ME.fuse_bn_relu(net)
    return netexec.NativeUNet(None, net[0], net[1], m, True, exact=exact)


def decisions(desc):
    """the row-independent part of a describe() result"""
    out = {"header": {k: v for k, v in desc["header"].items() if k not in ROW_DEPENDENT["header"]}}
    for key in ("ops", "tensors", "bufs"):
        out[key] = [{k: v for k, v in rec.items() if k not in ROW_DEPENDENT[key]} for rec in desc[key]]
    return out


def describe_case(program, var, rows_first=(37, 9, 3, 1)):
    with variant(var):
        ex = make_executor(program)
        return ex, ex.describe(level_rows(rows_first, ex.nlevels))


def main():
    from d3net_amd import build
    build.build()
    golden = {}
    for program, var in CASES:
        _, desc = describe_case(program, var)
        golden["%s/%s" % (program, var)] = decisions(desc)
    # compact: one list of field names per record kind, the records as rows of numbers
    packed = {}
    for case, d in golden.items():
        packed[case] = {"header": d["header"]}
        for key in ("ops", "tensors", "bufs"):
            names = list(d[key][0].keys()) if d[key] else []
            packed[case][key] = {"fields": names, "rows": [[rec[k] for k in names] for rec in d[key]]}
    with open(GOLDEN, "w") as f:
        json.dump(packed, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")


def load_golden():
    with open(GOLDEN) as f:
        packed = json.load(f)
    out = {}
    for case, d in packed.items():
        out[case] = {"header": d["header"]}
        for key in ("ops", "tensors", "bufs"):
            out[case][key] = [dict(zip(d[key]["fields"], row)) for row in d[key]["rows"]]
    return out


if __name__ == "__main__":
    main()
