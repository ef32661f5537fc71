"""Float64 numpy references of the streaming reductions outside the convolutions: d3net_amd/csrc/bn.hip (d3_bn_stats,
d3_bn_relu_fwd, d3_bn_relu_bwd) and the reduction parts of d3net_amd/csrc/heads.hip (d3_cross_entropy, d3_tall_wgrad,
d3_offset_loss, d3_score_loss, d3_masked_xe).  One plain function per C entry point: it takes the arrays the entry point
takes, computes in float64 from the fp32 inputs and returns everything the entry point writes.  A test helper:
tests/test_reduction_refs.py pins every function against torch's float64 CPU ops and autograd, the GPU tests
(tests/test_reductions_f64_gpu.py) compare the kernels with it.  The second half builds the inputs both files use."""
import numpy as np

F = np.float32
D = np.float64


def _d(a):
    return np.asarray(a, dtype=D)


# ------------------------------------------------------------------------------------------------ references
def bn_stats(x, running_mean=None, running_var=None, momentum=0.1):
    """-> mean, biased var, new running_mean, new running_var (None without running statistics); the running variance
    takes the unbiased estimate var * M / (M - 1), factor 1 for M = 1 (the kernel's convention; torch refuses M = 1)"""
    x = _d(x)
    M = x.shape[0]
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    if running_mean is None:
        return mean, var, None, None
    mom = float(F(momentum))
    unbias = M / (M - 1.0) if M > 1 else 1.0
    return mean, var, (1.0 - mom) * _d(running_mean) + mom * mean, (1.0 - mom) * _d(running_var) + mom * var * unbias


def bn_relu_fwd(x, mean, var, gamma, beta, eps, relu):
    y = (_d(x) - _d(mean)) / np.sqrt(_d(var) + float(F(eps))) * _d(gamma) + _d(beta)
    return np.maximum(y, 0.0) if relu else y


def bn_relu_bwd(x, dy, mean, var, gamma, beta, eps, relu):
    """-> dx, dgamma, dbeta of y = relu(gamma * xhat + beta) with batch statistics; the ReLU passes nothing where y <= 0"""
    inv = 1.0 / np.sqrt(_d(var) + float(F(eps)))
    xh = (_d(x) - _d(mean)) * inv
    g = _d(dy).copy()
    if relu:
        g[xh * _d(gamma) + _d(beta) <= 0.0] = 0.0
    dbeta, dgamma = g.sum(0), (g * xh).sum(0)
    M = xh.shape[0]
    dx = _d(gamma) * inv * (g - dbeta / M - xh * (dgamma / M))
    return dx, dgamma, dbeta


def cross_entropy(z, label, ignore_index):
    """-> mean loss over the counted rows (0 when none), count, UNSCALED gradient softmax - onehot; a row counts unless its
    label is ignore_index or outside [0, C)"""
    z = _d(z)
    label = np.asarray(label, dtype=np.int64)
    N, C = z.shape
    counted = (label != ignore_index) & (label >= 0) & (label < C)
    m = z.max(1, keepdims=True)
    e = np.exp(z - m)
    se = e.sum(1, keepdims=True)
    grad = e / se
    rows = np.nonzero(counted)[0]
    grad[rows, label[rows]] -= 1.0
    grad[~counted] = 0.0
    losses = (m[:, 0] + np.log(se[:, 0]))[rows] - z[rows, label[rows]]
    count = int(counted.sum())
    return (float(losses.sum() / count) if count else 0.0), count, grad


def tall_wgrad(x, dy):
    """-> dW (O, I) = dy^T x, db (O) = column sums of dy"""
    return _d(dy).T @ _d(x), _d(dy).sum(0)


def offset_loss(pt, coords, info, ids, ignore):
    """-> out (3) = norm loss, direction loss, number of valid points; g1, g2 (N, 3) = the unscaled gradients of the two
    loss sums w.r.t. pt.  |pt| = 0: the norm's subgradient is taken as 0, i.e. g2 = -gt_ / 1e-8"""
    p = _d(pt)
    g = _d(info)[:, :3] - _d(coords)
    valid = (np.asarray(ids) != ignore).astype(D)
    d = p - g
    g1 = valid[:, None] * np.sign(d)
    gn, pn = np.sqrt((g * g).sum(1)), np.sqrt((p * p).sum(1))
    ig, ip = 1.0 / (gn + 1e-8), 1.0 / (pn + 1e-8)
    dot = (g * p).sum(1) * ig
    direction = -dot * ip
    q = np.where(pn > 0.0, dot * ip * ip / np.where(pn > 0.0, pn, 1.0), 0.0)
    g2 = -valid[:, None] * (g * (ig * ip)[:, None] - q[:, None] * p)
    c = valid.sum()
    out = np.array([(np.abs(d).sum(1) * valid).sum() / (c + 1e-6), (direction * valid).sum() / (c + 1e-6), c])
    return out, g1, g2


def score_loss(scores, ious, fg, bg):
    """-> loss, gt_iou (P), dscore (P), the per-proposal terms (P).  target = 1 above fg, 0 below bg (both strict), linear
    between; BCE with logits in the stable form"""
    x, fg, bg = _d(scores).reshape(-1), float(F(fg)), float(F(bg))
    gt_iou = _d(ious).max(1)
    z = np.where(gt_iou > fg, 1.0, np.where(gt_iou < bg, 0.0, gt_iou / (fg - bg) + bg / (bg - fg)))
    term = (1.0 - z) * x + np.maximum(-x, 0.0) + np.log1p(np.exp(-np.abs(x)))
    sig = np.where(x >= 0, 1.0 / (1.0 + np.exp(-np.abs(x))), np.exp(-np.abs(x)) / (1.0 + np.exp(-np.abs(x))))
    return float(term.mean()), gt_iou, (sig - z) / x.shape[0], term


def masked_xe(pred, target, good, S):
    """pred (N, S, V), target (N, ld >= S), good (N).  -> loss, accuracy, dpred, per-row loss terms (N*S), per-row hits
    (N*S), denom = max(number of non-zero targets of good rows, 1).  Target 0 = ignored; accuracy uses the FIRST arg-max"""
    pred = _d(pred)
    N, _, V = pred.shape
    tg = np.where(np.asarray(good).astype(bool)[:, None], np.asarray(target, dtype=np.int64)[:, :S], 0)
    denom = float(max(int((tg != 0).sum()), 1))
    x = pred.reshape(N * S, V)
    tg = tg.reshape(-1)
    valid = (tg > 0) & (tg < V)
    m = x.max(1, keepdims=True)
    e = np.exp(x - m)
    se = e.sum(1, keepdims=True)
    rows = np.nonzero(valid)[0]
    grad = e / se
    grad[rows, tg[rows]] -= 1.0
    grad *= (valid / denom)[:, None]
    term = np.zeros(N * S)
    term[rows] = (m[:, 0] + np.log(se[:, 0]))[rows] - x[rows, tg[rows]]
    hit = np.zeros(N * S)
    hit[rows] = x.argmax(1)[rows] == tg[rows]
    return float(term.sum() / denom), float(hit.sum() / denom), grad.reshape(pred.shape), term, hit, denom


# ------------------------------------------------------------------------ inputs shared by the CPU and the GPU tests
BN_FAMILIES = ("mean 0.5 std 2", "mean 0 std 1e-3", "mean 30 std 1", "mean -300 std 1", "mean 1000 std 0.1", "constant",
               "one 1e4 outlier", "outlier in row 0")
BN_EPS = 1e-4
BN_MASK_BAND = 1e-3


def bn_case(M, C, shift, seed):
    """One BatchNorm call: channel c draws from BN_FAMILIES[(c + shift) % 8]; the outlier sits in row M // 2, or in row 0,
    which the statistics kernel takes as its pivot.  dy is zero where
    the float64 |y| (before the ReLU) is below BN_MASK_BAND, so that no fp32 rounding of y decides the ReLU mask."""
    rng = np.random.default_rng(seed)
    fam = (np.arange(C) + shift) % len(BN_FAMILIES)
    zn = rng.standard_normal((M, C))
    x = np.empty((M, C), D)
    for c in range(C):
        f = fam[c]
        x[:, c] = (0.5 + 2 * zn[:, c], 1e-3 * zn[:, c], 30 + zn[:, c], -300 + zn[:, c], 1000 + 0.1 * zn[:, c],
                   np.full(M, rng.uniform(-5, 5)), 0.5 + 2 * zn[:, c], 0.5 + 2 * zn[:, c])[f]
        if f >= 6:
            x[M // 2 if f == 6 else 0, c] = 1e4
    x = x.astype(F)
    gamma = (rng.uniform(0.5, 1.5, C) * rng.choice([-1.0, 1.0], C)).astype(F)
    beta = (rng.uniform(0.05, 0.5, C) * rng.choice([-1.0, 1.0], C)).astype(F)
    rm, rv = rng.uniform(-1, 1, C).astype(F), rng.uniform(0.5, 2, C).astype(F)
    mean, var, _, _ = bn_stats(x)
    y = bn_relu_fwd(x, mean, var, gamma, beta, BN_EPS, 0)
    dy = rng.standard_normal((M, C)).astype(F)
    band = np.abs(y) < BN_MASK_BAND
    dy[band] = 0
    return dict(x=x, gamma=gamma, beta=beta, rm=rm, rv=rv, dy=dy, fam=fam, band=band)


def bn_rows(C):
    """the row counts at channel count C: 1, 2, one short of a pass of 256 // C rows, one past the 16 passes of one workgroup"""
    rpp = 256 // C
    return sorted({1, 2, max(rpp - 1, 1), 16 * rpp + 1})


def bn_cases():
    """(M, C, shift, relu) of every BatchNorm call of the GPU test; bn_case(M, C, shift, 1000 * C + M) is its input.  The
    narrow layers rotate the families over their calls, the others hold all of them at once."""
    for C in (1, 3, 16, 20, 48, 112, 256):
        for i, M in enumerate(bn_rows(C)):
            for relu in (0, 1):
                yield M, C, (i + 4 * relu if C < len(BN_FAMILIES) else i), relu
    for relu in (0, 1):
        yield 16421, 112, 0, relu           # 512 * 16 * 2 + 37 rows: the capped grid, two rows per pass
        yield 131072 + 37, 16, 0, relu      # the capped grid, 16 rows per pass


def ce_case(N, C, mode, ignore_index, seed):
    """logits 3 * randn with (N >= 3) a row of +-1e4, a row of equal values and a row that is -inf off its label; labels by
    mode: 'none' ignored, 'some' (~30 % ignore_index, a few outside [0, C), a few C - 1), 'all' ignored"""
    rng = np.random.default_rng(seed)
    z = (3 * rng.standard_normal((N, C))).astype(F)
    ok = np.array([c for c in range(C) if c != ignore_index], dtype=np.int64)
    outside = np.array([v for v in (C, C + 5, -7, -3) if v != ignore_index], dtype=np.int64)
    if mode == "all" or ok.size == 0:
        label = np.where(rng.random(N) < 0.7, ignore_index, rng.choice(outside, N)).astype(np.int64)
    else:
        label = rng.choice(ok, N).astype(np.int64)
        if mode == "some":
            u = rng.random(N)
            label[u < 0.3] = ignore_index
            label[(u >= 0.3) & (u < 0.4)] = rng.choice(outside, int(((u >= 0.3) & (u < 0.4)).sum()))
            if C - 1 != ignore_index:
                label[(u >= 0.4) & (u < 0.5)] = C - 1
    if N >= 3:
        z[0] = np.where(np.arange(C) % 2 == 0, 1e4, -1e4)
        z[1] = 1.75
        keep = label[2] if 0 <= label[2] < C else 0
        v = z[2, keep]
        z[2] = -np.inf
        z[2, keep] = v
    return z, label


def offset_case(N, ldi, shift, seed, all_ignored=False, ignore=-100):
    """coords and the instance centres on a 2^-10 grid below 8 (their fp32 difference is exact); row r by (r + shift) % 8:
    0 pt = gt, 1 pt = 0, 2 gt = 0, otherwise every |pt - gt| component >= 1e-3"""
    rng = np.random.default_rng(seed)
    coords = (rng.integers(0, 8192, (N, 3)) / 1024.0).astype(F)
    info = rng.standard_normal((N, ldi)).astype(F)
    info[:, :3] = (rng.integers(0, 8192, (N, 3)) / 1024.0).astype(F)
    kind = (np.arange(N) + shift) % 8
    info[kind == 2, :3] = coords[kind == 2]
    gt = info[:, :3] - coords
    pt = (0.5 * rng.standard_normal((N, 3))).astype(F)
    near = np.abs(pt - gt) < F(2e-3)
    pt[near] = (gt + F(0.01))[near]
    pt[kind == 0] = gt[kind == 0]
    pt[kind == 1] = 0
    ids = rng.integers(0, 20, N).astype(np.int64)
    ids[rng.random(N) < 0.3] = ignore
    if all_ignored:
        ids[:] = ignore
    return pt, coords, info, ids, kind


SCORE_FG, SCORE_BG = 0.75, 0.25


def score_case(P, nInst, seed):
    """IoUs on a 2^-10 grid (the linear target is exact in fp32); row p by p % 7: 0 max exactly fg, 1 max exactly bg, 2 all
    below bg; scores 3 * randn, from three proposals on with a +100 and a -100"""
    rng = np.random.default_rng(seed)
    ious = rng.integers(0, 1025, (P, nInst)) / 1024.0 * rng.choice([0.25, 0.5, 1.0], (P, 1))
    kind = (np.arange(P) + seed) % 7
    col = rng.integers(0, nInst, P)
    for k, cap in ((0, SCORE_FG), (1, SCORE_BG), (2, SCORE_BG - 1.0 / 1024)):
        r = np.nonzero(kind == k)[0]
        ious[r] = np.minimum(ious[r], cap)
        ious[r, col[r]] = cap
    scores = (3 * rng.standard_normal(P)).astype(F)
    if P >= 3:          # (alone, a saturated score leaves a loss below fp32's smallest normal number: nothing to compare)
        scores[0], scores[P // 2] = 100.0, -100.0
    return scores, ious.astype(F), kind


def xe_case(N, S, V, seed, good_none=False):
    """pred 2 * randn (N, S, V); target (N, S + 3) with ~20 % zeros (the three columns past S are never read); good ~70 %.
    With at least 3 rows: one counted row whose maximum is tied between the target and index 0 (a miss), one (V > 2) tied
    between the target and index V - 1 (a hit)"""
    rng = np.random.default_rng(seed)
    pred = (2 * rng.standard_normal((N, S, V))).astype(F)
    target = rng.integers(1, V, (N, S + 3)).astype(np.int64)
    target[rng.random((N, S + 3)) < 0.2] = 0
    good = (rng.random(N) < 0.7).astype(np.uint8)
    ties = []
    if N * S >= 3 and not good_none:
        n0, s0, n1, s1 = 0, 0, (N * S - 1) // S, (N * S - 1) % S
        good[n0] = good[n1] = 1
        target[n0, s0] = V - 1
        pred[n0, s0, V - 1] = pred[n0, s0, 0] = 50.0
        ties.append((n0 * S + s0, 0.0))
        if V > 2:
            target[n1, s1] = 1
            pred[n1, s1, 1] = pred[n1, s1, V - 1] = 50.0
            ties.append((n1 * S + s1, 1.0))
    if good_none:
        good[:] = 0
    return pred, target, good, ties
