"""Float64 references and guarded buffers for d3net_amd/csrc/hgemm.hip (d3_hgemm, d3_colsum; contract: include/d3hip.h).
A test helper: tests/test_hgemm_refs.py pins the references against torch's float64 ops and autograd on the CPU, the GPU
tests (tests/test_hgemm_edges_gpu.py) compare the kernels with them.

Every operand and every output of a problem is a `Guarded`: a 2-d view inside a larger buffer whose other elements are the
guard -- NaN for floats, the index of a NaN table row for a gather vector.  A kernel that reads one element past K, past
row M - 1 or past column N - 1 adds NaN to its result; one that writes past its tile overwrites a NaN.  Guard values are
never out of range: a wrong kernel gives a wrong number, not a fault.

A `Prob` describes one d3_gemm_prob with CPU buffers; `Prob.to(device)` mirrors it, `struct()` fills the ctypes record,
`gemm_ref` returns the float64 image of the whole output buffer, guards included."""
import ctypes as C

import torch

NAN = float("nan")
EXACT_LIMIT = 2 ** 24
F32, F64 = torch.float32, torch.float64


# ------------------------------------------------------------------------------------------------ guarded buffers
class Guarded:
    """buf[r0:r0+rows, c0:c0+cols] of a 2-d contiguous buffer; the rest of buf is the guard"""

    def __init__(self, buf, r0, rows, c0, cols):
        assert buf.dim() == 2 and buf.is_contiguous()
        assert 0 <= r0 and r0 + rows <= buf.shape[0] and 0 <= c0 and c0 + cols <= buf.shape[1]
        self.buf, self.r0, self.rows, self.c0, self.cols = buf, r0, rows, c0, cols

    @property
    def view(self):
        return self.buf[self.r0:self.r0 + self.rows, self.c0:self.c0 + self.cols]

    @property
    def ld(self):
        return self.buf.shape[1]

    @property
    def ptr(self):
        return self.buf.data_ptr() + (self.r0 * self.ld + self.c0) * self.buf.element_size()

    def to(self, dev):
        return Guarded(self.buf.to(dev), self.r0, self.rows, self.c0, self.cols)

    def inside(self):
        m = torch.zeros(self.buf.shape, dtype=torch.bool)
        m[self.r0:self.r0 + self.rows, self.c0:self.c0 + self.cols] = True
        return m


def pad_off(width, mode):
    """(pad, off) of a view `width` elements wide: 'vec' -- ld % 4 == 0 and a 16-byte aligned base (the kernels' 16-byte
    loads); 'off1' -- ld % 4 == 0, base one element past alignment; 'odd' -- odd ld (scalar loads either way)"""
    if mode == "vec":
        return (-width) % 4 + 4, 4
    if mode == "off1":
        return (-width) % 4 + 4, 1
    assert mode == "odd"
    return (3 if width % 2 == 0 else 4), 2


def operand(vals, kmajor=False, pad=4, off=0, extra_rows=0):
    """vals (rows, K) float32 -> Guarded.  Row-major: a (rows + 2 + extra_rows, K + pad) buffer; k-major: (K + 2,
    rows + pad), holding vals^T.  The view starts at row 1, column off; everything else is NaN.  extra_rows: further NaN
    rows behind a gather table (the guard entries of its index vector point at the first of them)"""
    vals = vals.to(F32)
    rows, K = vals.shape
    assert 0 <= off <= pad
    if kmajor:
        buf = torch.full((K + 2, rows + pad), NAN, dtype=F32)
        g = Guarded(buf, 1, K, off, rows)
        g.view.copy_(vals.t())
    else:
        buf = torch.full((rows + 2 + extra_rows, K + pad), NAN, dtype=F32)
        g = Guarded(buf, 1, rows, off, K)
        g.view.copy_(vals)
    return g


def logical(g, kmajor):
    """the (rows, K) matrix an operand holds"""
    return g.view.t() if kmajor else g.view


def vector(vals, lead=1, trail=3, fill=NAN):
    """a 1-d array (bias, gather indices, column sums) as a one-row Guarded with `lead` / `trail` guard elements"""
    n = vals.numel()
    buf = torch.full((1, lead + n + trail), fill, dtype=vals.dtype)
    g = Guarded(buf, 0, 1, lead, n)
    g.view.copy_(vals.reshape(1, n))
    return g


def gather_index(idx, table_rows, lead=1, trail=3):
    """int32 row indices into a gather table of table_rows rows built with extra_rows >= 1: the guard entries hold
    table_rows, the first NaN row behind the table"""
    return vector(idx.to(torch.int32), lead, trail, fill=table_rows)


def output(M, N, pad=4, off=0, old=None):
    """(M + 2, N + pad) NaN buffer, the (M, N) view at row 1 / column off; old: its initial content (accumulate, add)"""
    assert 0 <= off <= pad
    buf = torch.full((M + 2, N + pad), NAN, dtype=F32)
    g = Guarded(buf, 1, M, off, N)
    if old is not None:
        g.view.copy_(old)
    return g


def guard_intact(g, got):
    """got: the buffer after the call (CPU).  True when every guard element still has its initial value"""
    out = ~g.inside()
    a, b = got[out], g.buf[out]
    if a.dtype.is_floating_point:
        return bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())
    return bool((a == b).all())


def interior_finite(g, got):
    return bool(torch.isfinite(got[g.inside()]).all())


def same(got, ref):
    """torch.equal over whole buffers, NaN guards included: the same elements are NaN and all others are equal"""
    if got.shape != ref.shape or got.dtype != ref.dtype:
        return False
    gn, rn = torch.isnan(got), torch.isnan(ref)
    return torch.equal(gn, rn) and torch.equal(got[~gn], ref[~rn])


def first_difference(got, ref):
    """(index, got, ref) of the first differing element, for a failure message"""
    bad = ~((got == ref) | (torch.isnan(got) & torch.isnan(ref)))
    idx = bad.nonzero()
    if idx.numel() == 0:
        return None
    i = tuple(int(v) for v in idx[0])
    return i, float(got[i]), float(ref[i]), int(bad.sum())


# ------------------------------------------------------------------------------------------------ problems
class Seg:
    def __init__(self, a, b, K, a_km=False, b_km=False, ia=None):
        self.a, self.b, self.K, self.a_km, self.b_km, self.ia = a, b, K, a_km, b_km, ia

    def A(self):
        """(M, K) float64 rows this segment contributes, gather applied"""
        A = logical(self.a, self.a_km).to(F64)
        return A[self.ia.view[0].long()] if self.ia is not None else A

    def B(self):
        return logical(self.b, self.b_km).to(F64)


GRU_OUT = ("dgi", "dgh", "dhp")


class Prob:
    """one d3_gemm_prob.  out: Guarded (M, N).  gru: None or a dict of Guarded -- d0, d1 (or None), r, z, n, ghn (M, H
    with ld == H), hp, dgi (M, 3H), dgh (M, 3H with ld == 3H), dhp (M, H with ld == H; `out` itself when it aliases C)"""

    def __init__(self, segs, M, N, out, bias=None, add=None, relu=False, accum=False, perm=(0, 0), gru=None):
        self.segs, self.M, self.N, self.out = list(segs), M, N, out
        self.bias, self.add, self.relu, self.accum, self.perm, self.gru = bias, add, relu, accum, perm, gru

    def to(self, dev):
        moved = {}

        def mv(g):          # one device copy per buffer, so that aliases stay aliases
            if g is None:
                return None
            if id(g.buf) not in moved:
                moved[id(g.buf)] = g.buf.to(dev)
            return Guarded(moved[id(g.buf)], g.r0, g.rows, g.c0, g.cols)

        segs = [Seg(mv(s.a), mv(s.b), s.K, s.a_km, s.b_km, mv(s.ia)) for s in self.segs]
        gru = {k: (mv(v) if isinstance(v, Guarded) else v) for k, v in self.gru.items()} if self.gru else None
        return Prob(segs, self.M, self.N, mv(self.out), mv(self.bias), mv(self.add), self.relu, self.accum, self.perm, gru)

    def total_k(self):
        return sum(s.K for s in self.segs)

    def struct(self):
        from d3net_amd._lib import GemmProb
        p = GemmProb()
        for i, s in enumerate(self.segs):
            q = p.seg[i]
            q.A, q.lda, q.a_kmajor = s.a.ptr, s.a.ld, int(s.a_km)
            q.B, q.ldb, q.b_kmajor = s.b.ptr, s.b.ld, int(s.b_km)
            q.ia = s.ia.ptr if s.ia is not None else None
            q.K = s.K
        p.nseg, p.M, p.N = len(self.segs), self.M, self.N
        p.C, p.ldc = self.out.ptr, self.out.ld
        p.bias = self.bias.ptr if self.bias is not None else None
        p.add = self.add.ptr if self.add is not None else None
        p.ldadd = self.add.ld if self.add is not None else 0
        p.relu, p.accum, p.perm_nb, p.perm_s = int(self.relu), int(self.accum), self.perm[0], self.perm[1]
        if self.gru:
            g = self.gru
            p.gru, p.gru_H = 1, g["H"]
            for k in ("d0", "d1"):
                if g[k] is not None:
                    setattr(p, "g_" + k, g[k].ptr)
                    setattr(p, "g_l" + k, g[k].ld)
            for k in ("r", "z", "n", "ghn"):
                assert g[k].ld == g["H"]
                setattr(p, "g_" + k, g[k].ptr)
            p.g_hp, p.g_ldh = g["hp"].ptr, g["hp"].ld
            assert g["dgh"].ld == 3 * g["H"] and g["dhp"].ld == g["H"]
            p.g_dgi, p.g_lddgi, p.g_dgh, p.g_dhp = g["dgi"].ptr, g["dgi"].ld, g["dgh"].ptr, g["dhp"].ptr
        return p


def _perm_rows(M, perm):
    r = torch.arange(M)
    return (r % perm[0]) * perm[1] + r // perm[0] if perm[0] > 0 else r


def _value(prob, magnitude=False):
    """(M, N) float64: the finished element before it is stored -- act(sum_seg A B^T + bias + add) (+ old C when
    accumulating, read at the permuted row).  magnitude: the same with every term replaced by its absolute value and no
    ReLU -- the scale of the rounding-error bound"""
    f = (lambda t: t.abs()) if magnitude else (lambda t: t)
    v = torch.zeros((prob.M, prob.N), dtype=F64)
    for s in prob.segs:
        v += f(s.A()) @ f(s.B()).t()
    if prob.bias is not None:
        v += f(prob.bias.view.to(F64))
    if prob.add is not None:
        v += f(prob.add.view.to(F64))
    if prob.relu and not magnitude:
        v = torch.clamp(v, min=0.0)
    if prob.accum:
        v = v + f(prob.out.view.to(F64)[_perm_rows(prob.M, prob.perm)])
    return v


def gemm_ref(prob, magnitude=False):
    """float64 image of prob.out.buf after the call: concat(A_seg[ia]) . concat(B_seg)^T + bias + add -> ReLU ->
    (+ old C when accum) -> row permutation, inside the untouched guard.  With a gate epilogue C is not written"""
    out = prob.out.buf.to(F64).clone()
    if prob.gru or prob.M == 0:
        return out
    v = _value(prob, magnitude)
    o = out[prob.out.r0:prob.out.r0 + prob.M, prob.out.c0:prob.out.c0 + prob.N]
    o[_perm_rows(prob.M, prob.perm)] = v
    return out


def gru_ref(v, d0, d1, r, z, n, ghn, hp, dtype=F64):
    """The gate epilogue of include/d3hip.h on the finished element v: dh' = d0 + d1 + v (None = absent);
    dn = dh'(1-z), dz = dh'(hp-n), dn_pre = dn(1-n^2); -> dgi = [dn_pre ghn r(1-r), dz z(1-z), dn_pre],
    dgh = [same, same, dn_pre r], dhp = dh' z.  Evaluated in `dtype`, left to right as written"""
    c = lambda t: t.to(dtype)
    dh = torch.zeros_like(c(v))
    if d0 is not None:
        dh = dh + c(d0)
    if d1 is not None:
        dh = dh + c(d1)
    dh = dh + c(v)
    r, z, n, ghn, hp = c(r), c(z), c(n), c(ghn), c(hp)
    dn, dz = dh * (1 - z), dh * (hp - n)
    dnp = dn * (1 - n * n)
    drp = dnp * ghn * r * (1 - r)
    dzp = dz * z * (1 - z)
    return torch.cat([drp, dzp, dnp], 1), torch.cat([drp, dzp, dnp * r], 1), dh * z


def gru_prob_ref(prob, dtype=F64):
    """{name: whole-buffer image} of the three gate outputs of a gru problem (dhp may alias prob.out)"""
    g = prob.gru
    v = _value(prob)
    opt = lambda k: g[k].view if g[k] is not None else None
    dgi, dgh, dhp = gru_ref(v, opt("d0"), opt("d1"), g["r"].view, g["z"].view, g["n"].view, g["ghn"].view, g["hp"].view, dtype)
    H, res = g["H"], {}
    for name, val in (("dgi", dgi), ("dgh", dgh), ("dhp", dhp)):
        t = g[name]
        buf = t.buf.to(dtype).clone()
        buf[t.r0:t.r0 + t.rows, t.c0:t.c0 + t.cols] = val
        res[name] = buf
    assert dgi.shape[1] == 3 * H
    return res


def exact_bound(prob):
    """sum_seg K_seg max|A| max|B| + max|bias| + max|add| + max|old C|: below 2^24 with integer inputs, every product,
    partial sum and epilogue term is an fp32 integer and the result does not depend on the summation order"""
    mx = lambda t: float(t.abs().max()) if t.numel() else 0.0
    b = sum(s.K * mx(s.a.view) * mx(s.b.view) for s in prob.segs)
    if prob.bias is not None:
        b += mx(prob.bias.view)
    if prob.add is not None:
        b += mx(prob.add.view)
    if prob.accum:
        b += mx(prob.out.view)
    return b


def assert_exact_inputs(prob):
    for s in prob.segs:
        for g in (s.a, s.b):
            assert bool((g.view == g.view.round()).all())
    for g in (prob.bias, prob.add, prob.out if prob.accum else None):
        if g is not None:
            assert bool((g.view == g.view.round()).all())
    assert exact_bound(prob) < EXACT_LIMIT, exact_bound(prob)


def colsum_ref(x, accum=False, old=None):
    """out[c] (+)= sum_r x[r, c] in float64; x (R, C), R may be 0"""
    s = x.to(F64).sum(0)
    return s + old.to(F64) if accum else s


# ------------------------------------------------------------------------------------------------ inputs
def ints(g, shape, hi, odd=False):
    """integer-valued float32 in [-hi, hi]; odd: mostly odd magnitudes (all mantissa bits down to the last one in use,
    so that an operand truncated to bf16 or tf32 changes the result)"""
    t = torch.randint(-hi, hi + 1, shape, generator=g)
    if odd:
        t = torch.where(torch.rand(shape, generator=g) < 0.9, t | 1, t)
        t = t.clamp(-hi, hi)
    return t.to(F32)


def operand_hi(total_k):
    """largest |A| of an exact case: 4095 up to K = 256 (with |B| <= 4: 256 * 4095 * 4 < 2^22), else 4"""
    return 4095 if total_k <= 256 else 4


def ws_guarded(nbytes, guard=256, pattern=0xA5):
    """a byte buffer of guard + nbytes + guard filled with `pattern`; the workspace is its middle"""
    return torch.full((guard + nbytes + guard,), pattern, dtype=torch.uint8), guard
