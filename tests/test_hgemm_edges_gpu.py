"""d3_hgemm / d3_colsum (d3net_amd/csrc/hgemm.hip) element by element at the edges of every kernel class, against float64
(tests/hgemm_refs.py), called through the C entry points so that no wrapper decides the kernel: hg_gemm_kernel<RT=1> (M <= 32,
the decode step), hg_gemm_kernel<RT=2> (fewer than 2048 16 x 16 output tiles, K split over the waves of a workgroup),
hg_gemm_tiled_kernel (2048 tiles and more), the 4 / 8 / 16-wave forms (20 and 40 k blocks), the cut over workgroups at
K >= 8192, and nativelinear.linear / linear_multi on top of them.

Criterion.  v_mfma_f32_16x16x4_f32 and the epilogues are plain fp32: with integer inputs whose
    sum_seg K_seg max|A| max|B| + max|bias| + max|add| + max|old C|  <  2^24
(asserted on the CPU before every launch) every product, partial sum and epilogue term is an integer that fp32 holds, so
the result is the same in ANY summation order and equals the float64 reference rounded to fp32 -- which rounds nothing.
The comparison is equality over the whole output buffer; it needs no tolerance, and one wrong, missing or doubled term
fails it.  Up to K = 256, A holds mostly odd integers up to 4095 (12 significant bits) against B in [-4, 4]: an operand cut
to bf16 or tf32 on its way changes the result; deeper reductions draw both from [-4, 4].  The gate epilogue gets dyadic
gates (r, z in {0, 1/2, 1}, n and hp multiples of 1/2, |dh'| <= 2^12) for which the float32 evaluation of the reference
equals the float64 one bit for bit.  One randn case per kernel class (K <= 128) is held to the order-independent bound of a
K-term fp32 sum and three epilogue roundings, per element: 1.01 (K + 3) 2^-24 (|A||B|^T + |bias| + |add| + |old C|).

Guards.  Every operand, index vector, bias, add and output is a view inside a larger buffer (row 1, column `off`, ld =
width + pad; 16-byte aligned with ld % 4 == 0 for the kernels' vector loads, or one element off / an odd ld for the scalar
ones).  Operand guards are NaN, index guards point at a NaN row: a read past K, past row M - 1 or column N - 1 turns the
result into NaN.  Output guards are NaN and must still be NaN afterwards -- checked separately from the values --, and no
element inside may be NaN.  The d3_colsum workspace has exactly the queried size between two 256-byte bands of a fixed
pattern.

What the tests met first.  nativelinear.linear with a 0-row input: the forward handed d3_hgemm the null data pointers of
empty tensors (D3_ERR_ARG, "hgemm" raised), and the backward's dW = dy^T x is a K = 0 reduction, refused likewise; empty
batches now launch nothing and return an empty dx and zero dW / db.  The kernels themselves passed every case.

Kernel changes tried on a scratch copy, and what caught them.  `k0 + 3 <= K` in hg_load4 (a 16-byte load one element past
K): "NaN inside the output" in test_decode_class / test_ksplit_class [nn-vec, nk-vec] and test_wave_count_thresholds, first
at M = N = 1, K = 3.  `c > p.N` in hg_gemm_kernel's epilogue: "output guard overwritten" in every test_decode_class and
test_ksplit_class case that ran (the run stopped at eight failures); the same in the tiled kernel: every test_tiled_class_k_tails and
test_tiled_class_segments_gather_permutation case.  `kb -= K / HT_BK` (floor) in the tiled kernel's locate:
test_tiled_class_segments_gather_permutation[(33, 1, 64)], test_class_boundary_at_2048_tiles,
test_four_problems_of_one_class[2], test_two_ksplit_problems_whose_bounding_box_is_tiled and the randn case of the tiled
class.  `wave` in place of `(wave - gkb)` in the rotation of a segment's first k block changes no value and fails nothing:
with either start the waves own the residues of the segment's blocks modulo the wave count, each block exactly once -- the
rotation only balances the load between waves."""
import ctypes as C

import pytest
import torch

import hgemm_refs as R

pytestmark = pytest.mark.gpu

ERR_WORKSPACE, ERR_ARG = -1, -3
LAYOUTS = {"nn": (False, False), "nk": (False, True), "kk": (True, True)}      # y = x W^T, dx = dy W, dW = dy^T x
EPIS = [(), ("bias",), ("add",), ("relu",), ("accum",), ("perm",), ("bias", "add", "relu", "accum", "perm")]
ALL = EPIS[-1]


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _perm(M):
    """(perm_nb, perm_s) with perm_nb * perm_s == M: the smallest divisor above 1 (a prime M keeps its order)"""
    for nb in range(2, M):
        if M % nb == 0:
            return nb, M // nb
    return 1, max(M, 1)


def kernel_class(M, N):
    """the host's rule (hg_class): 0 decode step, 1 K split over the waves of a workgroup, 2 tiled"""
    if M <= 32:
        return 0
    return 1 if ((N + 15) // 16) * ((M + 15) // 16) < 2048 else 2


def blocks(Ks):
    return sum((k + 15) // 16 for k in Ks)


def make(g, M, N, Ks, layout="nn", align="vec", epi=(), gather=False, hi=None, rand=False):
    """one guarded problem with integer inputs (rand: randn).  align 'vec': every base 16-byte aligned and every ld a
    multiple of 4; 'mis': bases one element off and odd lds, alternating over operands and segments"""
    Ks = (Ks,) if isinstance(Ks, int) else tuple(Ks)
    hi = hi or R.operand_hi(sum(Ks))
    a_km, b_km = LAYOUTS[layout]
    big = (lambda sh: torch.randn(sh, generator=g)) if rand else (lambda sh: R.ints(g, sh, hi, odd=True))
    small = (lambda sh: torch.randn(sh, generator=g)) if rand else (lambda sh: R.ints(g, sh, 4))
    side = (lambda sh: torch.randn(sh, generator=g)) if rand else (lambda sh: R.ints(g, sh, 1000))
    segs = []
    for j, K in enumerate(Ks):
        am = "vec" if align == "vec" else ("off1", "odd")[j % 2]
        bm = "vec" if align == "vec" else ("odd", "off1")[j % 2]
        B = R.operand(small((N, K)), b_km, *R.pad_off(N if b_km else K, bm))
        if gather and j == 0 and not a_km:
            T = M + 3
            table = R.operand(big((T, K)), False, *R.pad_off(K, am), extra_rows=2)
            ia = R.gather_index(torch.randint(0, T, (M,), generator=g), T, lead=4 if align == "vec" else 1)
            segs.append(R.Seg(table, B, K, False, b_km, ia))
        else:
            A = R.operand(big((M, K)), a_km, *R.pad_off(M if a_km else K, am))
            segs.append(R.Seg(A, B, K, a_km, b_km))
    out = R.output(M, N, *R.pad_off(N, "vec" if align == "vec" else "off1"), old=side((M, N)) if "accum" in epi else None)
    bias = R.vector(side((N,)), lead=4 if align == "vec" else 1) if "bias" in epi else None
    add = R.output(M, N, *R.pad_off(N, "vec" if align == "vec" else "odd"), old=side((M, N))) if "add" in epi else None
    return R.Prob(segs, M, N, out, bias, add, "relu" in epi, "accum" in epi, _perm(M) if "perm" in epi else (0, 0))


def launch(dprobs):
    from d3net_amd import _lib
    from d3net_amd._lib import GemmProb
    arr = (GemmProb * len(dprobs))(*[p.struct() for p in dprobs])
    rc = _lib.lib().d3_hgemm(arr, len(dprobs), _stream())
    torch.cuda.synchronize()
    assert rc == 0, rc


def check_exact(p, d, tag):
    """p: the CPU problem, d: its device mirror after the call"""
    got = d.out.buf.cpu()
    ref = R.gemm_ref(p)
    ref32 = ref.float()
    inside = p.out.inside()
    assert R.same(ref32.double()[inside], ref[inside]), tag          # the reference rounds nothing
    assert R.guard_intact(p.out, got), (tag, "output guard overwritten", R.first_difference(got, ref32))
    if p.M > 0 and not p.gru:
        assert R.interior_finite(p.out, got), (tag, "NaN inside the output", R.first_difference(got, ref32))
    if not (p.gru and p.gru["dhp"] is p.out):       # (g_dhp aliasing C: the buffer is checked as dhp below)
        assert R.same(got, ref32), (tag, R.first_difference(got, ref32))
    if p.gru:
        r64, r32 = R.gru_prob_ref(p), R.gru_prob_ref(p, torch.float32)
        for k in R.GRU_OUT:
            assert R.same(r32[k].double(), r64[k]), (tag, k, "the gate inputs are not exact in fp32")
            gk = d.gru[k].buf.cpu()
            assert R.guard_intact(p.gru[k], gk), (tag, k, "guard overwritten")
            assert R.interior_finite(p.gru[k], gk), (tag, k)
            assert R.same(gk, r32[k]), (tag, k, R.first_difference(gk, r32[k]))


def run_exact(probs, dev, tag=""):
    """one launch of up to four CPU problems; every output buffer must equal its float64 image"""
    for p in probs:
        R.assert_exact_inputs(p)
    dprobs = [p.to(dev) for p in probs]
    launch(dprobs)
    for i, (p, d) in enumerate(zip(probs, dprobs)):
        check_exact(p, d, (tag, i, p.M, p.N, [s.K for s in p.segs]))
    return dprobs


def run_in_fours(probs, dev, tag):
    for i in range(0, len(probs), 4):
        run_exact(probs[i:i + 4], dev, (tag, i))


KS = (1, 3, 4, 5, 15, 16, 17, 33)


# ------------------------------------------------------------------------------------------------ decode and K-split classes
@pytest.mark.parametrize("align", ["vec", "mis"])
@pytest.mark.parametrize("layout", ["nn", "nk", "kk"])
def test_decode_class(dev, layout, align):
    """M <= 32: hg_gemm_kernel<1, true, 4>, one or two workgroups down the rows; four problems of different shapes per launch"""
    g = _gen(100 + len(layout + align))
    probs, i = [], 0
    for M in (1, 15, 16, 17, 31, 32):
        for N in (1, 15, 16, 17, 33):
            for K in KS:
                probs.append(make(g, M, N, K, layout, align, EPIS[i % 7]))
                i += 1
    run_in_fours(probs, dev, "decode")
    # every M alone with every epilogue option at once: the launch's bounding box is the problem's own
    for M in (1, 15, 16, 17, 31, 32):
        run_exact([make(g, M, 33, 17, layout, align, ALL, gather=True)], dev, "decode-alone")


@pytest.mark.parametrize("align", ["vec", "mis"])
@pytest.mark.parametrize("layout", ["nn", "nk", "kk"])
def test_ksplit_class(dev, layout, align):
    """M > 32 and fewer than 2048 tiles: hg_gemm_kernel<2, true, 4>, two row tiles per workgroup"""
    g = _gen(200 + len(layout + align))
    probs, i = [], 0
    for M in (33, 47, 48, 49, 64, 65):
        for N in (1, 16, 17, 77):
            for K in KS:
                probs.append(make(g, M, N, K, layout, align, EPIS[i % 7]))
                i += 1
    run_in_fours(probs, dev, "ksplit")
    for M in (33, 47, 48, 49, 64, 65):
        run_exact([make(g, M, 77, 17, layout, align, ALL, gather=True)], dev, "ksplit-alone")
    # 342 row groups (blockIdx.y), two column tiles
    run_exact([make(g, 10913, 17, 5, layout, align, ALL)], dev, "ksplit-tall")
    run_exact([make(g, 10913, 17, 33, layout, align, ("bias",), gather=True)], dev, "ksplit-tall")


@pytest.mark.parametrize("M", [17, 32, 33, 64])
def test_wave_count_thresholds(dev, M):
    """19 / 20 / 39 / 40 k blocks: 4, 8, 8, 16 waves (hg_launch_batch), as one segment and as three whose block counts are no
    multiple of the wave count (the per-segment rotation of the first block)"""
    g = _gen(300 + M)
    probs, i = [], 0
    for K, nb in ((304, 19), (305, 20), (624, 39), (625, 40)):
        # one segment; three with the same total K (one block more); three with the same number of blocks
        for Ks, want in (((K,), nb), ((5, 16, K - 21), None), ((5, 16, 16 * (nb - 3) + 1), nb), ((17, 33, 16 * (nb - 6) + 3), nb)):
            assert want is None or blocks(Ks) == want, (Ks, blocks(Ks))
            for layout in ("nn", "kk"):
                probs.append(make(g, M, 17, Ks, layout, ("vec", "mis")[i % 2], EPIS[i % 7]))
                i += 1
    for p in probs:           # one launch each: the wave count follows the batch's deepest problem
        run_exact([p], dev, "waves")


@pytest.mark.parametrize("M", [17, 40])
def test_shallow_with_deep_in_one_batch(dev, M):
    """K = 5 beside K = 640 in one launch: 16 waves, of which 15 own no block of the shallow problem"""
    g = _gen(400 + M)
    for layout in ("nn", "nk", "kk"):
        for align in ("vec", "mis"):
            run_exact([make(g, M, 33, 5, layout, align, ALL), make(g, M, 17, 640, layout, align, ("bias", "relu")),
                       make(g, M - 1, 16, (5, 1, 3), layout, align, ("accum",))], dev, "shallow+deep")


# ------------------------------------------------------------------------------------------------ tiled class
@pytest.mark.parametrize("align", ["vec", "mis"])
@pytest.mark.parametrize("layout", ["nn", "nk", "kk"])
def test_tiled_class_k_tails(dev, layout, align):
    """730 x 725: 46 x 46 tiles of 16 (the tiled kernel: 12 x 12 workgroups with tails in both granularities), every K tail
    of the 32-deep slab and the 4-wide load"""
    g = _gen(500 + len(layout + align))
    probs = [make(g, 730, 725, K, layout, align, EPIS[i % 7]) for i, K in enumerate((1, 3, 4, 31, 32, 33, 36, 67))]
    for i in range(0, len(probs), 2):
        run_exact(probs[i:i + 2], dev, "tiled")


@pytest.mark.parametrize("Ks", [(33, 1, 64), (32, 32, 5)])
def test_tiled_class_segments_gather_permutation(dev, Ks):
    """three segments whose boundaries fall inside and on slab edges, the first gathered through ia, all epilogue options"""
    g = _gen(600 + Ks[0])
    for layout in ("nn", "nk", "kk"):
        for align in ("vec", "mis"):
            run_exact([make(g, 730, 725, Ks, layout, align, ALL, gather=True)], dev, ("tiled-seg", layout, align))
    run_exact([make(g, 730, 725, Ks[:2], "nn", "mis", ("perm",), gather=True),
               make(g, 730, 725, Ks[1:], "nk", "vec", ("add", "relu"))], dev, "tiled-2seg")


def _without_last_column(p):
    """the same problem with N - 1 columns on the same operand values; the dropped column of C, bias and add joins the guard"""
    cut = lambda t, km: R.Guarded(t.buf, t.r0, t.rows - (0 if km else 1), t.c0, t.cols - (1 if km else 0))

    def narrow(t):
        if t is None:
            return None
        n = R.Guarded(t.buf.clone(), t.r0, t.rows, t.c0, t.cols - 1)
        n.buf[:, t.c0 + t.cols - 1] = R.NAN
        return n

    segs = [R.Seg(s.a, cut(s.b, s.b_km), s.K, s.a_km, s.b_km, s.ia) for s in p.segs]
    return R.Prob(segs, p.M, p.N - 1, narrow(p.out), narrow(p.bias), narrow(p.add), p.relu, p.accum, p.perm)


def test_class_boundary_at_2048_tiles(dev):
    """(33, 10913): 3 x 683 = 2049 tiles, the tiled kernel; (33, 10912): 2046, still K split over waves.  The same data on
    both sides: equal to the reference, hence to each other"""
    g = _gen(700)
    N = 10913
    assert kernel_class(33, N) == 2 and kernel_class(33, N - 1) == 1 and (N + 15) // 16 * 3 == 2049
    for layout, align, epi in (("nn", "vec", ALL), ("kk", "mis", ("bias", "accum")), ("nk", "mis", ("add", "relu"))):
        p = make(g, 33, N, (33, 4), layout, align, epi)
        q = _without_last_column(p)
        dp, dq = run_exact([p], dev, ("boundary", N))[0], run_exact([q], dev, ("boundary", N - 1))[0]
        inside = q.out.inside()
        assert torch.equal(dp.out.buf.cpu()[inside], dq.out.buf.cpu()[inside])


# ------------------------------------------------------------------------------------------------ batches
@pytest.mark.parametrize("cls", [0, 1, 2])
def test_four_problems_of_one_class(dev, cls):
    g = _gen(800 + cls)
    shapes = {0: [(1, 33, 17), (32, 1, 5), (17, 16, (3, 16)), (15, 77, 33)],
              1: [(33, 77, 1), (65, 1, 33), (48, 17, (5, 17, 4)), (200, 40, 15)],
              2: [(730, 725, 5), (1040, 520, (33, 3)), (520, 1040, 36), (32780, 3, 1)]}[cls]
    for align in ("vec", "mis"):
        probs = [make(g, M, N, K, ("nn", "nk", "kk", "nn")[i], align, EPIS[(i + 3) % 7 if i else 6], gather=i == 3)
                 for i, (M, N, K) in enumerate(shapes)]
        assert all(kernel_class(p.M, p.N) == cls for p in probs)
        run_exact(probs, dev, ("four", cls))


def test_mixed_classes_with_an_empty_problem(dev):
    """classes 0, 1 and 2 and an M = 0 problem in one call: three launches by class, the empty one's output untouched"""
    g = _gen(900)
    for align in ("vec", "mis"):
        probs = [make(g, 730, 725, 33, "nn", align, ALL), make(g, 0, 17, 5, "nn", align), make(g, 17, 33, (5, 16), "kk", align, ALL),
                 make(g, 65, 77, 36, "nk", align, ALL)]
        assert [kernel_class(p.M, p.N) for p in probs] == [2, 0, 0, 1]
        d = run_exact(probs, dev, "mixed")
        assert bool(torch.isnan(d[1].out.buf).all())


def test_two_ksplit_problems_whose_bounding_box_is_tiled(dev):
    """(2000, 16) and (48, 10000) have 125 and 1875 tiles; together 125 x 625: the batch runs on the tiled kernel"""
    g = _gen(1000)
    assert kernel_class(2000, 16) == 1 and kernel_class(48, 10000) == 1 and kernel_class(2000, 10000) == 2
    for la, lb, align in (("nn", "kk", "vec"), ("nk", "nn", "mis")):
        run_exact([make(g, 2000, 16, (33, 3), la, align, ALL, gather=True), make(g, 48, 10000, 36, lb, align, ("bias", "relu"))],
                  dev, "bbox")


def _gru_problem(g, M, H, K, d0, d1, accum, layout, align):
    half = lambda sh, lo, hi: torch.randint(lo, hi + 1, sh, generator=g).float() / 2
    plain = lambda t: R.output(t.shape[0], t.shape[1], 0, 0, old=t)
    p = make(g, M, H, K, layout, align, ("accum",) if accum else (), hi=4)
    if accum:                 # g_dhp aliases C: both are indexed with row stride H
        p.out = plain(R.ints(g, (M, H), 1000))
    wide = lambda t, pad, off: R.output(t.shape[0], t.shape[1], pad, off, old=t)
    gru = dict(H=H, d0=wide(R.ints(g, (M, H), 1000), 0, 0) if d0 else None,
               d1=wide(R.ints(g, (M, H), 1000), 7, 5) if d1 else None,                      # g_ld1 wider than its rows
               r=plain(half((M, H), 0, 2)), z=plain(half((M, H), 0, 2)), n=plain(half((M, H), -2, 2)),
               ghn=plain(R.ints(g, (M, H), 8)), hp=wide(half((M, H), -6, 6), 3, 2),
               dgi=R.output(M, 3 * H, 5, 3), dgh=R.output(M, 3 * H, 0, 0),                # g_lddgi wider than 3 H
               dhp=p.out if accum else R.output(M, H, 0, 0))
    p.gru = gru
    bound = R.exact_bound(p) + 2000
    assert bound <= 2 ** 12, bound        # |dh'| <= 2^12: every gate product stays within 24 significant bits
    return p


@pytest.mark.parametrize("H", [16, 48])
@pytest.mark.parametrize("M", [13, 32, 33, 64])
def test_gru_gate_epilogue_beside_a_plain_problem(dev, M, H):
    """the GRUCell gate backward on the finished element (include/d3hip.h), decode class (M <= 32) and K-split class: dgi, dgh
    and dhp bit-equal to the float64 gate arithmetic, C not written unless g_dhp aliases it"""
    g = _gen(1100 + M + H)
    i = 0
    for d0 in (False, True):
        for d1 in (False, True):
            for accum in (False, True):
                layout, align = ("nk", "nn", "kk")[i % 3], ("vec", "mis")[i % 2]
                p = _gru_problem(g, M, H, (5, 20, 33)[i % 3], d0, d1, accum, layout, align)
                plain = make(g, M, 33, 17, "nn", align, ALL)
                d = run_exact([plain, p] if i % 2 else [p, plain], dev, ("gru", d0, d1, accum))
                if not accum:
                    assert bool(torch.isnan(d[0 if not i % 2 else 1].out.buf).all())      # C is not written in this mode
                i += 1


# ------------------------------------------------------------------------------------------------ split over workgroups
@pytest.mark.parametrize("K", [8191, 8192, 8193, 8207])
@pytest.mark.parametrize("N", [1, 17])
def test_reduction_cut_over_workgroups(dev, N, K):
    """D3_HG_SPLITK at its default (K >= 8192: four slices and a reduce launch) and at 0: both exact, hence equal"""
    from d3net_amd import _lib
    g = _gen(1200 + K + N)
    cases = []
    for layout in ("nn", "kk"):
        for align in ("vec", "mis"):
            cases.append(make(g, 33, N, K, layout, align, ("bias", "add", "relu")))
            cases.append(make(g, 33, N, K, layout, align, ("accum",)))
            cases.append(make(g, 36, N, K, layout, align, ("perm",)))
    assert all(p.segs[0].a.view.abs().max() <= 4 for p in cases)
    got = {}
    for arm in ("default", "off"):
        if arm == "off":
            with _lib.tuning(D3_HG_SPLITK=0):
                ds = [run_exact([p], dev, ("splitk", arm, j))[0] for j, p in enumerate(cases)]
        else:
            ds = [run_exact([p], dev, ("splitk", arm, j))[0] for j, p in enumerate(cases)]
        got[arm] = [d.out.buf.cpu() for d in ds]
    for a, b in zip(got["default"], got["off"]):
        assert R.same(a, b)


# ------------------------------------------------------------------------------------------------ one randn case per class
@pytest.mark.parametrize("M,N,Ks", [(17, 33, (67, 5, 33)), (49, 77, (128,)), (730, 725, (67, 33))])
def test_fp32_rounding_bound(dev, M, N, Ks):
    """randn inputs: |got - ref| <= 1.01 (K + 3) 2^-24 (|A||B|^T + |bias| + |add| + |old C|) per element -- any order of K
    fp32 FMAs and three epilogue roundings stays inside; a 16-bit or tf32 operand does not"""
    K = sum(Ks)
    assert K <= 128
    g = _gen(1300 + M)
    for layout in ("nn", "nk", "kk"):
        for align in ("vec", "mis"):
            p = make(g, M, N, Ks, layout, align, ALL, gather=True, rand=True)
            d = p.to(dev)
            launch([d])
            got = d.out.buf.cpu()
            ref, mag = R.gemm_ref(p), R.gemm_ref(p, magnitude=True)
            inside = p.out.inside()
            assert R.guard_intact(p.out, got) and R.interior_finite(p.out, got)
            err = (got.double() - ref)[inside].abs()
            bound = 1.01 * (K + 3) * 2.0 ** -24 * mag[inside]
            print("M %d N %d K %d %s %s: max err / bound %.3f" % (M, N, K, layout, align, float((err / bound).max())))
            assert bool((err <= bound).all()), float((err / bound).max())


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_output_alone(dev):
    """argument checks that return D3_ERR_ARG before any launch"""
    g = _gen(1400)

    def refused(change, n=1, gru=False):
        p = _gru_problem(g, 17, 16, 5, True, True, False, "nn", "vec") if gru else make(g, 17, 16, 5)
        d = p.to(dev)
        from d3net_amd import _lib
        from d3net_amd._lib import GemmProb
        s = d.struct()
        change(s)
        arr = (GemmProb * 5)(*([s] * 5))
        rc = _lib.lib().d3_hgemm(arr, n, _stream())
        torch.cuda.synchronize()
        assert rc == ERR_ARG, rc
        bufs = [d.out] + ([d.gru[k] for k in R.GRU_OUT] if gru else [])
        assert all(bool(torch.isnan(t.buf).all()) for t in bufs)

    nothing = lambda s: None
    refused(nothing, n=0)
    refused(nothing, n=5)
    refused(lambda s: setattr(s, "nseg", 0))
    refused(lambda s: setattr(s, "nseg", 4))
    refused(lambda s: setattr(s, "N", 0))
    refused(lambda s: setattr(s, "C", None))
    refused(lambda s: setattr(s.seg[0], "K", 0))
    refused(lambda s: setattr(s, "relu", 1), gru=True)
    refused(lambda s: setattr(s, "gru_H", 32), gru=True)


# ------------------------------------------------------------------------------------------------ d3_colsum
@pytest.mark.parametrize("Cc", [1, 63, 64, 65, 130])
def test_colsum(dev, Cc):
    from d3net_amd import _lib
    L = _lib.lib()
    g = _gen(1500 + Cc)
    nbytes = L.d3_colsum_ws_bytes(Cc)
    assert nbytes > 0
    for R_ in (0, 1, 3, 15, 16, 17, 63, 65, 257):
        for wide in (False, True):
            for accum in (0, 1):
                vals = R.ints(g, (R_, Cc), 4095, odd=True)
                assert R_ * 4095 + 1000 < R.EXACT_LIMIT
                x = R.operand(vals, False, *((5, 2) if wide else (0, 0)))
                old = R.ints(g, (Cc,), 1000)
                out = R.vector(old if accum else torch.full((Cc,), R.NAN))
                wsb, guard = R.ws_guarded(nbytes)
                xd, od, wsd = x.to(dev), out.to(dev), wsb.to(dev)
                rc = L.d3_colsum(C.c_void_p(xd.ptr), x.ld, R_, Cc, C.c_void_p(od.ptr), accum, C.c_void_p(wsd.data_ptr() + guard), nbytes,
                                 _stream())
                torch.cuda.synchronize()
                assert rc == 0, rc
                got = od.buf.cpu()
                ref = out.buf.double().clone()
                ref[0, out.c0:out.c0 + Cc] = R.colsum_ref(vals, bool(accum), old)
                assert R.guard_intact(out, got) and R.interior_finite(out, got), (R_, Cc, wide, accum)
                assert R.same(got, ref.float()), (R_, Cc, wide, accum, R.first_difference(got, ref.float()))
                w = wsd.cpu()
                assert bool((w[:guard] == 0xA5).all()) and bool((w[guard + nbytes:] == 0xA5).all())
    # a workspace one byte short: refused, nothing written
    x, out = R.operand(R.ints(g, (17, Cc), 4)), R.vector(torch.full((Cc,), R.NAN))
    wsb, guard = R.ws_guarded(nbytes)
    xd, od, wsd = x.to(dev), out.to(dev), wsb.to(dev)
    rc = L.d3_colsum(C.c_void_p(xd.ptr), x.ld, 17, Cc, C.c_void_p(od.ptr), 0, C.c_void_p(wsd.data_ptr() + guard), nbytes - 1, _stream())
    torch.cuda.synchronize()
    assert rc == ERR_WORKSPACE, rc
    assert bool(torch.isnan(od.buf).all()) and bool((wsd == 0xA5).all())


# ------------------------------------------------------------------------------------------------ nativelinear
def _linear_case(dev, g, n, relu, rot):
    """n items through linear / linear_multi against float64 autograd of F.linear (+ ReLU); item 0 has a non-contiguous x, item
    1 stays out of the loss, item 2's x needs no gradient, odd items have no bias"""
    import torch.nn.functional as Fn
    from d3net_amd import nativelinear as NL
    Ms, Ds = (1, 13, 40), (5, 16, 33)
    leaves, items, items64, outs_w = [], [], [], []
    for i in range(n):
        M, K, N = Ms[(i + rot) % 3], Ds[(i + 2 * rot) % 3], Ds[(i + rot + 1) % 3]
        xv = R.ints(g, (M, 2 * K) if i == 0 else (M, K), 4095, odd=True)
        Wv, bv, wv = R.ints(g, (N, K), 4), (R.ints(g, (N,), 1000) if i % 2 == 0 else None), R.ints(g, (M, N), 4)
        assert K * 4095 * 4 + 1000 < R.EXACT_LIMIT and M * 4095 * 4 < R.EXACT_LIMIT and N * 16 < R.EXACT_LIMIT
        row = []
        for dtype, device in ((torch.float32, dev), (torch.float64, "cpu")):
            x = xv.to(device=device, dtype=dtype).requires_grad_(i != 2)
            W = Wv.to(device=device, dtype=dtype).requires_grad_(True)
            b = bv.to(device=device, dtype=dtype).requires_grad_(True) if bv is not None else None
            row.append((x, W, b, (x[:, ::2] if i == 0 else x), wv.to(device=device, dtype=dtype)))
        leaves.append(row)
    nat = [(r[0][3], r[0][1], r[0][2]) for r in leaves]
    assert not nat[0][0].is_contiguous()
    ys = [NL.linear(*nat[0], relu=relu)] if n == 1 else NL.linear_multi(nat, relu=relu)
    ys64 = []
    for r in leaves:
        y = Fn.linear(r[1][3], r[1][1], r[1][2])
        ys64.append(torch.relu(y) if relu else y)
    used = [i for i in range(n) if i != 1]
    sum((ys[i] * leaves[i][0][4]).sum() for i in used).backward()
    sum((ys64[i] * leaves[i][1][4]).sum() for i in used).backward()
    for i in range(n):
        assert torch.equal(ys[i].detach().cpu().double(), ys64[i].detach()), ("y", i)
        for j, name in ((0, "dx"), (1, "dW"), (2, "db")):
            a, b = leaves[i][0][j], leaves[i][1][j]
            if a is None or not a.requires_grad:
                assert a is None or a.grad is None, (name, i)
                continue
            want = b.grad if b.grad is not None else torch.zeros_like(b)       # (the item left out of the loss)
            gota = a.grad if a.grad is not None else torch.zeros_like(a)
            assert torch.equal(gota.cpu().double(), want), (name, i, n, relu, rot)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("n", [1, 3, 5])
def test_nativelinear_is_float64_autograd(dev, n, relu):
    """integer-valued x, W, b and output weights: y, dx, dW, db equal float64 autograd exactly; five items are ten backward
    problems in three launches"""
    g = _gen(1600 + n)
    for rot in range(3):
        _linear_case(dev, g, n, relu, rot)


@pytest.mark.parametrize("relu", [False, True])
def test_nativelinear_empty_batch(dev, relu):
    from d3net_amd import nativelinear as NL
    g = _gen(1700)
    W = R.ints(g, (16, 5), 4).to(dev).requires_grad_(True)
    b = R.ints(g, (16,), 4).to(dev).requires_grad_(True)
    x = torch.zeros(0, 5, device=dev, requires_grad=True)
    y = NL.linear(x, W, b, relu=relu)
    assert y.shape == (0, 16)
    y.sum().backward()
    assert x.grad.shape == (0, 5)
    assert W.grad.shape == (16, 5) and not bool(W.grad.any()) and b.grad.shape == (16,) and not bool(b.grad.any())
    # beside a non-empty item in one call
    x2 = R.ints(g, (13, 5), 4095, odd=True).to(dev).requires_grad_(True)
    x0 = torch.zeros(2, 0, 5, device=dev, requires_grad=True)
    W2 = W.detach().clone().requires_grad_(True)
    y0, y2 = NL.linear_multi([(x0, W, None), (x2, W2, b)], relu=relu)
    assert y0.shape == (2, 0, 16)
    (y0.sum() + y2.sum()).backward()
    ref = x2.detach().cpu().double().requires_grad_(True)
    W64 = W2.detach().cpu().double().requires_grad_(True)
    y64 = torch.nn.functional.linear(ref, W64, b.detach().cpu().double())
    (torch.relu(y64) if relu else y64).sum().backward()
    assert torch.equal(y2.detach().cpu().double(), (torch.relu(y64) if relu else y64).detach())
    assert torch.equal(x2.grad.cpu().double(), ref.grad) and torch.equal(W2.grad.cpu().double(), W64.grad)
    assert x0.grad.shape == (2, 0, 5)
