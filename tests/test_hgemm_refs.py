"""tests/hgemm_refs.py against torch's own float64 CPU ops (torch.cat + torch.matmul, torch.nn.GRUCell's autograd), and the
properties of the guarded buffers that the GPU tests (tests/test_hgemm_edges_gpu.py) rely on."""
import pytest
import torch

import hgemm_refs as R

F64 = torch.float64


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def close(a, b):
    """1e-12 of the largest value: the reference adds segment by segment, torch.cat + matmul in one sum"""
    return a.shape == b.shape and float((a - b).abs().max()) <= 1e-12 * max(float(b.abs().max()), 1e-300)


def _inner(prob, ref):
    o = prob.out
    return ref[o.r0:o.r0 + o.rows, o.c0:o.c0 + o.cols]


@pytest.mark.parametrize("a_km,b_km", [(False, False), (False, True), (True, False), (True, True)])
def test_gemm_ref_layouts(a_km, b_km):
    g = _gen(1)
    M, N, K = 7, 5, 6
    A, B = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)
    bias, add = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    p = R.Prob([R.Seg(R.operand(A, a_km, 5, 1), R.operand(B, b_km, 4, 4), K, a_km, b_km)], M, N, R.output(M, N, 3, 2),
               bias=R.vector(bias), add=R.output(M, N, 2, 1, old=add), relu=True)
    ref = R.gemm_ref(p)
    want = torch.relu(torch.matmul(A.to(F64), B.to(F64).t()) + bias.to(F64) + add.to(F64))
    assert close(_inner(p, ref), want)
    assert ref.shape == p.out.buf.shape and bool(torch.isnan(ref[~p.out.inside()]).all())


def test_gemm_ref_three_segments_gather_permutation_accumulate():
    g = _gen(2)
    nb, s, N = 4, 3, 5
    M = nb * s
    Ks = (3, 1, 6)
    table = torch.randn(9, Ks[0], generator=g)
    idx = torch.randint(0, 9, (M,), generator=g)
    A1, A2 = torch.randn(M, Ks[1], generator=g), torch.randn(M, Ks[2], generator=g)
    W = torch.randn(N, sum(Ks), generator=g)
    old = torch.randn(M, N, generator=g)
    segs = [R.Seg(R.operand(table, extra_rows=2), R.operand(W[:, :3]), 3, ia=R.gather_index(idx, 9)),
            R.Seg(R.operand(A1, True), R.operand(W[:, 3:4], True), 1, True, True),
            R.Seg(R.operand(A2), R.operand(W[:, 4:], True), 6, False, True)]
    p = R.Prob(segs, M, N, R.output(M, N, 4, 1, old=old), accum=True, perm=(nb, s))
    x = torch.cat([table[idx], A1, A2], 1).to(F64)
    y = torch.matmul(x, W.to(F64).t())
    want = old.to(F64) + y.view(s, nb, N).transpose(0, 1).reshape(M, N)      # rows t * nb + b -> b * s + t
    assert close(_inner(p, R.gemm_ref(p)), want)
    # the same without accumulate: the interior is overwritten
    p.accum = False
    assert close(_inner(p, R.gemm_ref(p)), want - old.to(F64))
    # the magnitude form bounds the value
    p.accum = True
    assert bool((_inner(p, R.gemm_ref(p, magnitude=True)) >= _inner(p, R.gemm_ref(p)).abs()).all())


def test_gemm_ref_leaves_zero_row_and_gate_problems_untouched():
    p = R.Prob([R.Seg(R.operand(torch.zeros(0, 3)), R.operand(torch.ones(2, 3)), 3)], 0, 2, R.output(0, 2))
    assert bool(torch.isnan(R.gemm_ref(p)).all())


def test_gru_ref_is_grucell_autograd():
    g = _gen(3)
    M, I, H = 5, 4, 6
    cell = torch.nn.GRUCell(I, H).to(F64)
    x, hp = torch.randn(M, I, generator=g, dtype=F64), torch.randn(M, H, generator=g, dtype=F64)
    dh = torch.randn(M, H, generator=g, dtype=F64)
    gi = x @ cell.weight_ih.t() + cell.bias_ih
    gh = hp @ cell.weight_hh.t() + cell.bias_hh
    r = torch.sigmoid(gi[:, :H] + gh[:, :H]).detach()
    z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H]).detach()
    ghn = gh[:, 2 * H:].detach()
    n = torch.tanh(gi[:, 2 * H:] + r * ghn).detach()
    d0, d1 = 0.25 * dh, 0.5 * dh
    dgi, dgh, dhp = R.gru_ref(dh - d0 - d1, d0, d1, r, z, n, ghn, hp)
    for m in range(M):      # one row at a time: the bias gradients of the cell are then that row's dgi / dgh
        h = hp[m:m + 1].clone().requires_grad_(True)
        cell.zero_grad()
        cell(x[m:m + 1], h).backward(dh[m:m + 1])
        assert torch.allclose(dgi[m], cell.bias_ih.grad, rtol=1e-12, atol=1e-14)
        assert torch.allclose(dgh[m], cell.bias_hh.grad, rtol=1e-12, atol=1e-14)
        # d hp = dh' z (the direct path, g_dhp) + dgh W_hh (a GEMM of its own in the backward)
        assert torch.allclose(dhp[m] + dgh[m] @ cell.weight_hh.detach(), h.grad[0], rtol=1e-12, atol=1e-14)
    # absent d0 / d1
    a, b, c = R.gru_ref(dh, None, None, r, z, n, ghn, hp)
    assert torch.allclose(a, dgi, rtol=1e-12, atol=1e-14) and torch.allclose(c, dhp, rtol=1e-12, atol=1e-14)


def test_colsum_ref():
    x = torch.randn(17, 5, generator=_gen(4))
    old = torch.randn(5, generator=_gen(5))
    assert torch.equal(R.colsum_ref(x), x.to(F64).sum(0))
    assert torch.equal(R.colsum_ref(x, True, old), x.to(F64).sum(0) + old.to(F64))
    assert torch.equal(R.colsum_ref(torch.zeros(0, 5)), torch.zeros(5, dtype=F64))


@pytest.mark.parametrize("width", [1, 3, 4, 5, 16, 17, 33])
@pytest.mark.parametrize("kmajor", [False, True])
def test_builders_give_the_requested_alignment(width, kmajor):
    rows = 6
    vals = torch.arange(rows * width, dtype=torch.float32).view(rows, width)
    for mode in ("vec", "off1", "odd"):
        pad, off = R.pad_off(rows if kmajor else width, mode)
        g = R.operand(vals, kmajor, pad, off)
        assert g.buf.data_ptr() % 16 == 0
        vec = g.ld % 4 == 0 and g.ptr % 16 == 0          # the kernels' condition for 16-byte loads
        assert vec == (mode == "vec"), (mode, g.ld, g.ptr % 16)
        assert g.ptr == g.view.data_ptr() and g.ld == g.view.stride(0)
        assert torch.equal(R.logical(g, kmajor), vals)
        assert bool(torch.isnan(g.buf[~g.inside()]).all()) and int(g.inside().sum()) == rows * width
        assert g.r0 == 1 and g.buf.shape[0] == (width if kmajor else rows) + 2
        o = R.output(rows, width, *R.pad_off(width, mode))
        assert bool(torch.isnan(o.buf).all()) and o.buf.shape[0] == rows + 2
        assert (o.ld % 4 == 0 and o.ptr % 16 == 0) == (mode == "vec")


def test_gather_guards_point_at_a_nan_row():
    table = R.operand(torch.ones(9, 4), extra_rows=2)
    ia = R.gather_index(torch.tensor([0, 8, 3]), 9)
    assert ia.buf.dtype == torch.int32 and ia.buf[0].tolist() == [9, 0, 8, 3, 9, 9, 9]
    rows = table.buf[table.r0:]                       # what the kernel indexes: row 0 of the view onwards
    assert rows.shape[0] > 9 and bool(torch.isnan(rows[9]).all())
    assert ia.ptr == ia.buf.data_ptr() + 4


def test_guard_checks_and_whole_buffer_equality():
    o = R.output(3, 2, 3, 1)
    got = o.buf.clone()
    got[1:4, 1:3] = 1.0
    assert R.guard_intact(o, got) and R.interior_finite(o, got)
    ref = got.clone()
    assert R.same(got, ref) and R.first_difference(got, ref) is None
    bad = got.clone()
    bad[2, 3] = 0.0                                   # one element right of the view
    assert not R.guard_intact(o, bad) and not R.same(bad, ref)
    assert R.first_difference(bad, ref)[0] == (2, 3)
    bad = got.clone()
    bad[2, 2] = 2.0
    assert R.guard_intact(o, bad) and not R.same(bad, ref)
    bad[2, 2] = R.NAN
    assert not R.interior_finite(o, bad)


def test_exact_inputs_and_bound():
    g = _gen(6)
    A = R.ints(g, (40, 256), 4095, odd=True)
    assert float(A.abs().max()) <= 4095 and float((A % 2 != 0).float().mean()) > 0.8
    B = R.ints(g, (7, 256), 4)
    p = R.Prob([R.Seg(R.operand(A), R.operand(B), 256)], 40, 7, R.output(40, 7, old=R.ints(g, (40, 7), 100)),
               bias=R.vector(R.ints(g, (7,), 50)), accum=True)
    assert R.exact_bound(p) <= 256 * 4095 * 4 + 150 < R.EXACT_LIMIT
    R.assert_exact_inputs(p)
    ref = R.gemm_ref(p)
    assert torch.equal(ref.float().double()[p.out.inside()], ref[p.out.inside()])       # representable in fp32
    assert R.operand_hi(256) == 4095 and R.operand_hi(257) == 4
    p.segs[0].a.view[0, 0] = 0.5
    with pytest.raises(AssertionError):
        R.assert_exact_inputs(p)


def test_prob_to_keeps_aliases():
    o = R.output(4, 3, 0, 0)
    z = lambda *s: R.output(s[0], s[1], 0, 0, old=torch.zeros(s))
    gru = dict(H=3, d0=None, d1=None, r=z(4, 3), z=z(4, 3), n=z(4, 3), ghn=z(4, 3), hp=z(4, 3), dgi=R.output(4, 9, 2, 1),
               dgh=R.output(4, 9, 0, 0), dhp=o)
    p = R.Prob([R.Seg(R.operand(torch.ones(4, 2)), R.operand(torch.ones(3, 2)), 2)], 4, 3, o, gru=gru)
    q = p.to("cpu")
    assert q.gru["dhp"].buf is q.out.buf and q.gru["H"] == 3
    res = R.gru_prob_ref(p)
    assert set(res) == {"dgi", "dgh", "dhp"} and res["dgi"].shape == gru["dgi"].buf.shape
    assert bool(torch.isnan(R.gemm_ref(p)).all())      # C is not written with a gate epilogue
