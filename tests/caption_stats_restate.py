"""Plain python restatement of csrc/caption_eval.hip's rules over lists of token ids: the first-occurrence clipping of the BLEU
counts, the "closest" reference length, the bit-vector LCS and the merge priority of d3_caption_collect.  No GPU; the CPU tests
pin it to caption_metrics on strings, the GPU tests compare the kernels' integers with it."""

MASK64 = (1 << 64) - 1
PRIO_BITS = 20


def ngram_key(tok, p, n):
    """one 64-bit key per n-gram, 16 bits per token (id + 1): cider.hip's cd_key"""
    k = 0
    for q in range(n):
        k |= (tok[p + q] + 1) << (16 * q)
    return k


def bleu_counts(cand, refs, n=4):
    """-> [correct_1..n, testlen, reflen]: per order, the first occurrence of a candidate key carries min(its count in the
    candidate, the largest count in one reference); later occurrences carry nothing"""
    out = []
    for k in range(1, n + 1):
        keys = [ngram_key(cand, p, k) for p in range(len(cand) - k + 1)]
        total = 0
        for p, key in enumerate(keys):
            if key in keys[:p]:
                continue
            cnt = sum(1 for x in keys if x == key)
            refmax = 0
            for r in refs:
                refmax = max(refmax, sum(1 for q in range(len(r) - k + 1) if ngram_key(r, q, k) == key))
            total += min(cnt, refmax)
        out.append(total)
    return out + [len(cand), closest_length(len(cand), [len(r) for r in refs])]


def closest_length(testlen, reflens):
    """min((|l - testlen|, l)): the shorter on equal distance"""
    best_d, best_l = None, 0
    for l in reflens:
        d = abs(l - testlen)
        if best_d is None or d < best_d or (d == best_d and l < best_l):
            best_d, best_l = d, l
    return best_l


def lcs_bits(cand, ref):
    """bit i of V belongs to candidate token i (a wave64 lane); per reference token y: M = the lanes that hold y, U = V & M,
    V = (V + U) | (V - U) in 64-bit arithmetic from all ones; LCS = the zero bits among the low len(cand)"""
    assert len(cand) <= 64
    v = MASK64
    for y in ref:
        m = 0
        for i, x in enumerate(cand):
            if x == y:
                m |= 1 << i
        u = v & m
        v = ((v + u) | (v - u)) & MASK64
    return bin(~v & ((1 << len(cand)) - 1)).count("1")


def priority(batch_seq, b, g, G):
    """the smallest wins: the first batch, within a batch the last (b, g)"""
    assert 0 <= b * G + g < (1 << PRIO_BITS)
    return batch_seq * (1 << PRIO_BITS) + ((1 << PRIO_BITS) - 1 - (b * G + g))


def merge_owner(records):
    """records: (batch_seq, b, g, G, key) in any order -> {key: (batch_seq, b, g)} of the winners"""
    best = {}
    for seq, b, g, G, key in records:
        p = priority(seq, b, g, G)
        if key not in best or p < best[key][0]:
            best[key] = (p, (seq, b, g))
    return {k: v[1] for k, v in best.items()}
