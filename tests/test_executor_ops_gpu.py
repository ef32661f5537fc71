"""Every op of the native U-Net executor (csrc/unet.hip), with its fused epilogues, pinned op by op at the canonical scene's
row counts -- "teacher forced": the oracle (oracle/sparse_oracle.py, bf16 mode = the kernels' arithmetic restated) is fed the
EXECUTOR'S OWN activations, so that each comparison is one op deep.

Why not end to end: two bf16 implementations that differ only in fp32 summation order decorrelate to the bf16 noise floor
within three layers (a 1e-7 difference flips a bf16 rounding with probability 2.5e-5; the flip is a 4e-3 perturbation of the
next layer's input; ...) and ~1 % of the ReLU masks then differ, which moves gradients by sqrt(1 %) = 10 % per layer --
tests/test_fullsize_step_gpu.py measures exactly that.  With the forward activations shared, every forward op is
deterministic up to summation order and the backward is a LINEAR function of the output gradient through fixed masks, so
tight bounds hold:
  forward : PADCAST bit-exact; every CONV output (incl. residual epilogue, strided concat halves) <= 1e-4 of its scale;
            every BN -> ReLU output within one bf16 ulp, differing from the re-rounded oracle value in < 0.1 % of elements;
  backward: the oracle back-propagates the same output gradient op by op through the executor's activations (fixed ReLU
            masks, fixed operands); EVERY parameter gradient (conv kernels: side-stream wgrad + batched split reduction; BN
            gamma / beta: the dgrad-epilogue reductions) and the input gradient must agree to <= 2e-2 relative L2.  Measured on
            MI355X: worst 8.5e-3, input gradient 4.4e-3 -- the bf16 noise floor: each data / weight gradient rounds its dy
            operand to bf16, a rounding step is discontinuous, so a relative difference d between two otherwise identical
            chains grows as sqrt(d * 2^-8) per layer towards the fixed point 2^-8 = 4e-3 (the same mechanism as in the forward,
            with the masks taken out).  A wrong index, epilogue or accumulation order produces O(1) errors.
The program covers every layer type of the backbone's levels 0-2: k3 16->16 / 32->32 / 48->48, k3 2C->C, k1 2C->C, stride-2
down 16->32 / 32->48, transposed up 48->32 / 32->16, stem 134->16 (zero-padded bf16 input), final BN; level 0 / 1 run the
persistent wave-per-tile kernel (142,920 / 35,127 rows), level 2 (8,282 rows) the split kernel.
Reference semantics: model/common.py:22-118, model/pointgroup.py:69-74."""
import ctypes as C
import functools
import struct

import numpy as np
import pytest
import torch

from oracle import sparse_oracle as so

pytestmark = pytest.mark.gpu


def l2err(a, b):
    a = a.detach().cpu().double(); b = b.detach().cpu().double()
    return float((a - b).norm() / (b.norm() + 1e-30))


def relerr(a, b):
    a = a.detach().cpu().double(); b = b.detach().cpu().double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def _bits_to_float(b):
    return struct.unpack("<f", struct.pack("<i", int(b)))[0]


@pytest.mark.parametrize("stem", [True, False])
def test_executor_ops_teacher_forced_at_canonical_rows(dev, stem):
    from d3net_amd import _lib, minkowski as ME, common, netexec, synthetic as S
    from d3net_amd.netexec import OP_CONV, OP_BNACT, OP_PADCAST, MAP_K1, MAP_K3, MAP_DOWN, MAP_UP
    planes, cin = [16, 32, 48], (134 if stem else 16)
    occ, _, _, _ = S.occupancy_grid()
    vox = np.argwhere(occ)
    coords = np.concatenate([np.zeros((len(vox), 1), np.int64), vox], 1)
    rng = np.random.default_rng(5 + stem)
    x = torch.from_numpy(rng.standard_normal((len(coords), cin)).astype(np.float32))
    torch.manual_seed(9)
    norm = functools.partial(ME.MinkowskiBatchNorm, eps=1e-4, momentum=0.1)
    net = torch.nn.Sequential(ME.MinkowskiConvolution(cin, planes[0], kernel_size=3, bias=False, dimension=3),
                              common.UBlock(planes, norm, 2, common.ResidualBlock), norm(planes[0]), ME.MinkowskiReLU(inplace=True))
    ME.fuse_bn_relu(net)
    with torch.no_grad():
        for n, p in net.named_parameters():
            if n.endswith("bn.weight"):
                p.uniform_(0.5, 1.5)
            if n.endswith("bn.bias"):
                p.uniform_(-0.2, 0.2)
    net = net.to(dev)
    ex = netexec.NativeUNet(net[0] if stem else None, net[1], net[2], cin, not stem)
    ex.debug_keep = True
    cm = ME.CoordinateManager(torch.from_numpy(coords).int().to(dev))
    xn = x.to(dev).requires_grad_(not stem)
    out = ex(xn, cm, True)
    g = torch.from_numpy(rng.standard_normal(tuple(out.shape)).astype(np.float32))
    out.backward(g.to(dev))
    torch.cuda.synchronize()
    arena, rows = ex.debug_last
    assert rows[:3] == [142920, 35127, 8282]
    arena = arena.cpu()
    L = _lib.lib()
    b = ex.b

    def tensor(i):
        """tensor i of the program as a CPU fp32 matrix (rows, C), read from the executor's arena"""
        level, Cc, width, coff, dtype, buf = b.tensors[i]
        if buf < 0:
            return x
        off = L.d3_net_tensor_offset(ex._net(), i)
        es = 2 if dtype == 1 else 4
        raw = arena[off:off + ((rows[level] - 1) * width + Cc) * es]
        t = raw.view(torch.bfloat16 if dtype == 1 else torch.float32)
        return torch.as_strided(t, (rows[level], Cc), (width, 1)).float()

    ocm = so.OracleCoords(coords)
    for l in range(len(planes) - 1):
        ocm.get_down(1 << l)
    params = [p.detach().cpu() for p in b.params]
    so.set_precision("bf16")
    try:
        def conv_fn(op):
            _, xi, oi, res, w, kind, mlevel, K, cin_w, _ = op[:10]
            ts = 1 << mlevel
            if kind == MAP_K3:
                return lambda xx, W: so.conv_k3(xx[:, :cin_w], W, ocm.get_k3(ts))
            if kind == MAP_DOWN:
                parent, kidx, Mo = ocm.get_down(ts)
                return lambda xx, W: so.conv_down(xx, W, parent, kidx, Mo)
            if kind == MAP_UP:
                parent, kidx, Mo = ocm.get_down(ts)
                return lambda xx, W: so.conv_up(xx, W, parent, kidx)
            return lambda xx, W: so.mm(xx, W)

        # ---------------- forward, op by op on the executor's activations
        n_conv = n_bn = n_conv_bf16 = 0
        worst_conv = 0.0
        for op in b.ops:
            if op[0] == OP_PADCAST:
                y = tensor(op[2])
                ref = torch.zeros_like(y); ref[:, :cin] = x.bfloat16().float()
                assert torch.equal(y, ref), "PADCAST is not the RNE bf16 cast of the zero-padded input"
            elif op[0] == OP_CONV:
                xi, oi, res, w = op[1], op[2], op[3], op[4]
                with torch.no_grad():
                    ref = conv_fn(op)(tensor(xi), params[w])
                    if res >= 0:
                        ref = ref + tensor(res)
                if b.tensors[oi][4] == 1:
                    # bf16 output (round 6: a convolution output with one reader, the BatchNorm behind it): the fp32 result rounded
                    # to nearest even -- one ulp, and almost always the same rounding as the oracle's
                    y, refq = tensor(oi), ref.bfloat16().float()
                    diff = (y - refq).abs()
                    assert float((diff > 0).double().mean()) < 1e-2, ("CONV rounding", float((diff > 0).double().mean()))
                    assert bool((diff <= refq.abs() * 2.0 ** -7 + 1e-6).all()), "bf16 CONV output differs by more than one bf16 ulp"
                    n_conv_bf16 += 1
                else:
                    e = relerr(tensor(oi), ref)
                    worst_conv = max(worst_conv, e)
                    assert e < 1e-4, ("CONV", op[:10], e)
                n_conv += 1
            elif op[0] == OP_BNACT:
                xi, oi = op[1], op[2]
                gamma, beta, relu, eps = params[op[4]], params[op[5]], op[8], _bits_to_float(op[9])
                with torch.no_grad():
                    xx = tensor(xi).double()
                    m, v = xx.mean(0), xx.var(0, unbiased=False)
                    ref = (xx - m) * torch.rsqrt(v + eps) * gamma.double() + beta.double()
                    if relu:
                        ref = torch.relu(ref)
                y = tensor(oi)
                if b.tensors[oi][4] == 1:      # bf16 output: one ulp, and almost always the same rounding
                    refq = ref.float().bfloat16().float()
                    diff = (y - refq).abs()
                    # (a bf16 INPUT: the executor's statistics come from the producer's unrounded accumulators, the oracle's from
                    # the stored values -- ~1e-5 relative apart instead of 1e-7)
                    lim = 2e-2 if b.tensors[xi][4] == 1 else 1e-3
                    assert float((diff > 0).double().mean()) < lim, ("BNACT rounding", float((diff > 0).double().mean()))
                    # (one bf16 ulp; next to the ReLU threshold the executor's 1e-7 different statistics may leave a value of
                    # rounding size where the oracle has 0)
                    slack = 2e-4 if b.tensors[xi][4] == 1 else 1e-5
                    assert bool((diff <= refq.abs() * 2.0 ** -7 + slack).all()), "BNACT differs by more than one bf16 ulp"
                else:
                    assert relerr(y, ref) < 1e-5
                n_bn += 1
        assert n_conv >= (25 if stem else 24) and n_bn >= 23 and n_conv_bf16 >= 10

        # ---------------- backward: the oracle back-propagates the same gradient through the executor's activations
        nb = len(b.bufs)
        Gbuf = {i: torch.zeros((rows[b.bufs[i][0]], b.bufs[i][1])) for i in range(nb)}
        Gext = torch.zeros_like(x)
        pgrad = {}

        def gview(i):
            level, Cc, width, coff, dtype, buf = b.tensors[i]
            return Gext if buf < 0 else Gbuf[buf][:, coff:coff + Cc]

        gview(ex.out_tensor).copy_(g)
        for op in reversed(b.ops):
            if op[0] == OP_CONV:
                xi, oi, res, w = op[1], op[2], op[3], op[4]
                dY = gview(oi).clone()
                xl = tensor(xi).requires_grad_(True)
                Wl = params[w].clone().requires_grad_(True)
                gx, gW = torch.autograd.grad(conv_fn(op)(xl, Wl), [xl, Wl], dY)
                if b.tensors[xi][5] >= 0 or ex.input_needs_grad:
                    gview(xi).add_(gx)
                pgrad[w] = pgrad.get(w, 0) + gW
                if res >= 0:
                    gview(res).add_(dY)
            elif op[0] == OP_BNACT:
                xi, oi = op[1], op[2]
                relu, eps = op[8], _bits_to_float(op[9])
                dY = gview(oi).clone()
                xl = tensor(xi).double().requires_grad_(True)
                ga = params[op[4]].double().clone().requires_grad_(True); be = params[op[5]].double().clone().requires_grad_(True)
                m, v = xl.mean(0), xl.var(0, unbiased=False)
                y = (xl - m) * torch.rsqrt(v + eps) * ga + be
                if relu:
                    y = torch.relu(y)
                gx, gg, gb = torch.autograd.grad(y, [xl, ga, be], dY.double())
                gview(xi).add_(gx.float())
                pgrad[op[4]] = gg.float(); pgrad[op[5]] = gb.float()
    finally:
        so.set_precision("fp32")
    errs = {}
    names = {id(p): n for n, p in net.named_parameters()}
    for i, ref in pgrad.items():
        p = b.params[i]
        if not b.grad_params[i]:
            continue
        errs[names[id(p)]] = l2err(p.grad, ref)
    worst = max(errs, key=errs.get)
    e_in = l2err(xn.grad, Gext) if not stem else 0.0
    print("executor ops teacher-forced (stem=%s): %d convs fwd worst %.1e; %d parameter gradients, worst rel-L2 %.2e (%s), input grad %.2e"
          % (stem, n_conv, worst_conv, len(errs), errs[worst], worst, e_in))
    assert len(errs) == sum(1 for p in net.parameters() if p.grad is not None) >= 70
    assert errs[worst] < 2e-2, (worst, errs[worst])
    assert e_in < 2e-2, e_in


def test_executor_ops_teacher_forced_with_fp32_gradient_storage(dev):
    """D3_GRAD_BF16=0 keeps every gradient buffer in fp32.  The plan then holds two launch arms no other test reaches: the one-launch
    BatchNorm backward with a bf16 BatchNorm input and a bf16 shadow as dy but an fp32 input gradient
    (un_bn_bwd_fused_small_kernel<false, true, true>), and the K = 27 weight gradients with an fp32 dy on the 16-bit kernel map
    (spconv_wgrad3_kernel<..., DYBF false, T16 true>).  Same program, same oracle, same bounds as above."""
    from d3net_amd import _lib, minkowski as ME, common, netexec
    from d3net_amd.netexec import OP_CONV, OP_BNACT
    DYBF16 = 64
    L = _lib.lib()
    with _lib.tuning(D3_GRAD_BF16=0):
        norm = functools.partial(ME.MinkowskiBatchNorm, eps=1e-4, momentum=0.1)
        net = torch.nn.Sequential(common.UBlock([16, 32, 48], norm, 2, common.ResidualBlock), norm(16), ME.MinkowskiReLU(inplace=True))
        ME.fuse_bn_relu(net)
        ex = netexec.NativeUNet(None, net[0], net[1], 16, True)
        d = ex.describe([142920, 35127, 8282])      # (the plan is host code)
        bn_arms = {(d["tensors"][raw[1]]["bf16"] if op["in_grad_mode"] else 0, d["tensors"][raw[2]]["bf16"], int(ex.b.tensors[raw[1]][4] == 1))
                   for op, raw in zip(d["ops"], ex.b.ops) if op["type"] == OP_BNACT and op["fused_by"] >= 0}
        assert (0, 1, 1) in bn_arms, bn_arms
        k27 = [op for op, raw in zip(d["ops"], ex.b.ops) if op["type"] == OP_CONV and raw[7] == 27]
        assert k27 and all(op["k3_tables"] == 1 and not (op["wgrad_flags"] & DYBF16) for op in k27), [(op["k3_tables"], op["wgrad_flags"]) for op in k27]
        n0 = L.d3_spconv_t16_launches()
        test_executor_ops_teacher_forced_at_canonical_rows(dev, False)
        n_big = sum(1 for op, raw in zip(d["ops"], ex.b.ops) if op["type"] == OP_CONV and raw[7] == 27 and ex.b.tensors[raw[1]][0] <= 1)
        assert n_big == 16 and L.d3_spconv_t16_launches() - n0 >= n_big      # one weight gradient on the 16-bit map per K = 27 layer of levels 0 and 1


def _detector_step(dev, scene, seed=0):
    """one bf16 detector step on `scene` -> (loss, flat backbone gradient, backbone output checksum)"""
    from d3net_amd import synthetic as S
    from d3net_amd.config import default_conf
    from d3net_amd.pointgroup import PointGroup
    cfg = default_conf("pointgroup.yaml")
    torch.manual_seed(seed)
    model = PointGroup(cfg).to(dev).train()
    model.teacher = True
    batch = S.make_batch([scene], dev)
    batch["cluster_rand"] = torch.rand(2, 3, generator=torch.Generator().manual_seed(1))
    batch["slot_perms"] = [torch.randperm(cfg.model.max_num_proposal, generator=torch.Generator().manual_seed(2))]
    loss, d = model.training_step(batch)
    loss.backward()
    torch.cuda.synchronize()
    ex = model._execs["backbone"]
    return float(loss), ex._flat_grad.clone(), d["semantic_scores"][0].detach().clone()


def test_int16_kernel_maps_are_bit_identical_to_the_dense_tables(dev):
    """Round 4: the K = 27 convolutions of the big levels read their kernel map as int16 deltas (csrc/coordmap.hip
    cm_pack16_kernel; the stem's forward: spconv_fwd2_c_kernel, weight gradients: spconv_wgrad3_kernel; the other forward / data-gradient
    launches of the big levels read the lane table, round 6 -- switched off here).
    Same neighbours, same order, same arithmetic: a whole detector step (loss, every backbone parameter gradient, the point
    logits) must be BIT-identical with D3_KMAP16 on and off -- and the 16-bit path must really have run."""
    from d3net_amd import _lib, synthetic as S
    L = _lib.lib()
    occ, sem, inst, _ = S.occupancy_grid()
    scene = S.scene_from_grid(occ, sem, inst)
    res = {}
    assert L.d3_tuning_set(b"D3_C3", 0) == 0      # (round 6: the lane-table kernel would take the big levels' forward / data gradients)
    try:
        for on in (1, 0):
            assert L.d3_tuning_set(b"D3_KMAP16", on) == 0
            n0 = L.d3_spconv_t16_launches()
            res[on] = _detector_step(dev, scene) + (L.d3_spconv_t16_launches() - n0,)
    finally:
        L.d3_tuning_set(b"D3_KMAP16", 1); L.d3_tuning_set(b"D3_C3", 1)
    assert res[1][3] >= 10, ("launches that read a 16-bit table", res[1][3])      # the stem's forward + the weight gradients of level 0
    assert res[0][3] == 0
    assert res[1][0] == res[0][0], (res[1][0], res[0][0])
    assert torch.equal(res[1][1], res[0][1]), "backbone parameter gradients"
    assert torch.equal(res[1][2], res[0][2]), "point logits"


def test_lane_table_kernel_equals_the_dense_table_kernels_to_fp32_rounding(dev):
    """Round 6: the K = 27 forward / data-gradient convolutions of the big levels run spconv_fwd3_kernel on the lane table
    (csrc/spconv3.hip): same bf16 operands and fp32 accumulation as spconv_fwd2_kernel, another summation order (per tile the live
    offsets first).  A whole detector step with D3_C3 on and off agrees like two bf16 runs (bounds below) -- and the lane-table path
    must really have run (level 0: >= 20 launches)."""
    from d3net_amd import _lib, netexec, synthetic as S
    L = _lib.lib()
    occ, sem, inst, _ = S.occupancy_grid()
    scene = S.scene_from_grid(occ, sem, inst)
    res = {}
    keep = netexec.SINGLE_READER_BF16
    netexec.SINGLE_READER_BF16 = False      # (fp32 between the two convolutions of a block: a bf16 store would turn a 1e-7 difference into an ulp flip)
    try:
        for on in (1, 0):
            assert L.d3_tuning_set(b"D3_C3", on) == 0
            n0 = L.d3_spconv_fwd3_launches()
            res[on] = _detector_step(dev, scene) + (L.d3_spconv_fwd3_launches() - n0,)
    finally:
        L.d3_tuning_set(b"D3_C3", 1)
        netexec.SINGLE_READER_BF16 = keep
    assert res[1][3] >= 20, ("lane-table launches", res[1][3])      # level 0: 11 convolutions forward + their data gradients (the deeper levels' flags may land after the forward)
    assert res[0][3] == 0
    # (every BatchNorm output is stored as bf16: a 1e-7 difference in front of a store is now and then a flipped ulp behind it, and 30
    # normalised layers carry it on -- the two programs agree like two bf16 runs do, tests/test_fullsize_step_gpu.py's bounds against
    # the fp32 oracle: loss 2e-2, logits 3e-2; the kernel-level parity is tests/test_conv3_gpu.py's 1e-4 against the oracle)
    assert abs(res[1][0] - res[0][0]) <= 5e-3 * abs(res[0][0]), (res[1][0], res[0][0])
    assert float((res[1][2] - res[0][2]).abs().max() / res[0][2].abs().max()) < 3e-2
    # gradients: ~70 BatchNorm / ReLU layers double a perturbation every other layer (measured op by op: 4e-8 behind the first
    # convolution, 2e-6 behind its bf16 store, 1e-3 at level 1, 1.5e-2 at level 6), so two bf16 programs agree in direction and size,
    # not entry by entry -- the bound of tests/test_fullsize_step_gpu.py for bf16 against fp32 operands: cosine of the flat gradient
    g1, g0 = res[1][1].double(), res[0][1].double()
    cosine = float((g1 * g0).sum() / (g1.norm() * g0.norm()))
    assert cosine > 0.7 and 0.8 < float(g1.norm() / g0.norm()) < 1.25, (cosine, float(g1.norm() / g0.norm()))


def test_int16_kernel_map_refuses_far_neighbours(dev):
    """a row order whose neighbours are more than 32767 rows apart does not fit int16 deltas: the validity flag of
    d3_kmap_k3_pack16 is 0 and the coordinate manager hands out no 16-bit table (the convolutions keep the dense one)"""
    from d3net_amd import minkowski as ME, synthetic as S
    occ, _, _, _ = S.occupancy_grid()
    vox = np.argwhere(occ)
    rng = np.random.default_rng(0)
    vox = vox[rng.permutation(len(vox))]                       # shuffled rows: neighbours anywhere in 0..M
    coords = torch.from_numpy(np.concatenate([np.zeros((len(vox), 1), np.int64), vox], 1)).int().to(dev)
    cm = ME.CoordinateManager(coords.contiguous())
    cm.k3_16(1)
    torch.cuda.synchronize()
    assert cm.k3_16(1) is None and cm._k3_16[1]["valid"] is False
    coords = torch.from_numpy(np.concatenate([np.zeros((len(vox), 1), np.int64), np.argwhere(occ)], 1)).int().to(dev)
    cm = ME.CoordinateManager(coords.contiguous())             # scan order: fits
    cm.k3_16(1)
    torch.cuda.synchronize()
    t16 = cm.k3_16(1)
    assert t16 is not None
    nbr = cm.k3(1).cpu().numpy()
    d = t16[:-2].view(-1, 27).cpu().numpy().astype(np.int64)
    rows = np.arange(nbr.shape[0])[:, None]
    assert np.array_equal(np.where(d == -32768, -1, rows + d), nbr)


def test_few_row_batchnorm_in_one_launch_matches_the_separate_kernels(dev):
    """Round 4: below D3_BN_FUSED_ROWS rows a BatchNorm is one launch per direction (un_bn_fused_small_kernel /
    un_bn_bwd_fused_small_kernel).  The statistics are reduced by another (fixed) tree than un_bn_finalize_kernel's, so the
    comparison with the separate kernels is to fp32 rounding, not bit for bit: loss 1e-6, gradients 1e-4 relative L2."""
    from d3net_amd import _lib, synthetic as S
    L = _lib.lib()
    scene = S.small_scene(dims=(64, 48, 32), n_boxes=4, seed=7)
    res = {}
    for rows in (16384, 0):
        assert L.d3_tuning_set(b"D3_BN_FUSED_ROWS", rows) == 0
        res[rows] = _detector_step(dev, scene)
    L.d3_tuning_set(b"D3_BN_FUSED_ROWS", 16384)
    assert abs(res[16384][0] - res[0][0]) <= 1e-5 * abs(res[0][0]), (res[16384][0], res[0][0])
    assert l2err(res[16384][2], res[0][2]) < 1e-3
    assert l2err(res[16384][1], res[0][1]) < 5e-2          # (bf16 chains decorrelate: see the module docstring; a wrong kernel gives O(1))


def test_second_level_batchnorm_partials_match_the_full_table_reduction(dev):
    """Round 5 (csrc/conv.h D3_P2_ROWS, csrc/unet.hip un_fs_reduce2, D3_BN_PART2): every producer workgroup also adds its
    BatchNorm partial row into a 16-row fp64 table (hardware fp64 atomics, row = workgroup % 16) and the BatchNorm launches
    reduce those 16 rows instead of the producer's whole per-workgroup table.  Both paths add the SAME fp32 partial values in fp64;
    such sums are exact (hence order-independent) unless one channel's addends span more than 2^29 in magnitude, so the two
    paths agree to the last bit almost everywhere and a bf16 step stays far inside its noise floor: loss 1e-6, logits 1e-4,
    parameter gradients 1e-3 relative L2 -- and two runs of the atomics path reproduce each other (loss identical, gradients 1e-6)."""
    from d3net_amd import _lib, synthetic as S
    L = _lib.lib()
    scene = S.small_scene(dims=(64, 48, 32), n_boxes=4, seed=7)
    res = {}
    try:
        for key, on in (("on", 1), ("off", 0), ("again", 1)):
            assert L.d3_tuning_set(b"D3_BN_PART2", on) == 0
            res[key] = _detector_step(dev, scene)
    finally:
        L.d3_tuning_set(b"D3_BN_PART2", 1)
    assert abs(res["on"][0] - res["off"][0]) <= 1e-6 * abs(res["off"][0]), (res["on"][0], res["off"][0])
    assert l2err(res["on"][2], res["off"][2]) < 1e-4
    assert l2err(res["on"][1], res["off"][1]) < 1e-3
    assert res["on"][0] == res["again"][0] and l2err(res["on"][1], res["again"][1]) < 1e-6
