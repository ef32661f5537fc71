// caption_eval.hip -- the captioning validation on the device (gfx950): the per-batch record of the matched captions and the
// integer statistics behind BLEU-1..4 and ROUGE-L.
//
// Replaces, per validation batch, the B x G python loop of lib/captioning/eval_helper.py:102-246 (assign_dense_caption after its
// Hungarian step: box3d_iou, decode of every matched caption, the candidates dict) and, at the end of the epoch, the counting half
// of lib/capeval/bleu/bleu_scorer.py (cook_refs / cook_test with the "closest" reference length) and lib/capeval/rouge/rouge.py
// (my_lcs), as d3net_amd/caption_eval.py and caption_metrics.py restate them on the host.  Sentences are int32 token ids as
// cider.hip defines them (string equality == id equality); the floating point of both metrics stays on the host.
//
//   d3_caption_collect   two launches per batch over the (b, g) GT slots with mask != 0.
//                        pass 1: one thread per slot marks its scene seen and, where the object has a corpus slot, takes
//                        atomicMin(owner[slot], prio) with prio = batch_seq * 2^20 + (2^20 - 1 - (b * G + g)): the first batch wins
//                        (`candidates.setdefault` in validation_epoch_end), within a batch the last (b, g) (`candidates[key] = ...`).
//                        pass 2: one wave per slot; the record whose prio == owner[slot] writes the IoU of the matched pair
//                        (lib/utils/bbox.py:273-305 in float32, torch's operation order, -ffp-contract=off) and the sentence
//                        [sos] + tokens through the lut up to and including the first eos (appended when absent): decode_caption.
//                        A prio is unique, so every output element has one writer; the atomics are integer min / or.
//   d3_caption_stats     one workgroup of 256 per entry (a candidate and its reference rows).  Thread i owns the candidate n-gram
//                        of order i / 64 + 1 at position i % 64 as one 64-bit key (cider.hip's packing); brute-force compares over
//                        LDS count it in the candidate and in each reference, the first occurrence of a key carries
//                        min(count, max over references); wave w sums order w + 1.  Then one wave per (candidate, reference) pair
//                        runs the bit-vector LCS recurrence: lane i holds candidate token i, per reference token y
//                        M = ballot(tok_i == y), U = V & M, V = (V + U) | (V - U) from all ones, LCS = popcount(~V & low len bits).
#include "common.h"

#define CE_MAXT 64              // tokens per sentence, sos and eos included
#define CE_PRIO_BITS 20         // (b * G + g) < 2^20 per batch
#define CE_THREADS 256

// torch.minimum / torch.maximum / min(dim) / max(dim): a NaN propagates
__device__ __forceinline__ float ce_min(float a, float b) { return a != a ? a : (b != b ? b : fminf(a, b)); }
__device__ __forceinline__ float ce_max(float a, float b) { return a != a ? a : (b != b ? b : fmaxf(a, b)); }
__device__ __forceinline__ float ce_clamp0(float x) { return x != x ? x : fmaxf(x, 0.f); }

__device__ __forceinline__ void ce_aabb(const float *__restrict__ c, float *lo, float *hi) {
#pragma unroll
    for (int a = 0; a < 3; a++) lo[a] = hi[a] = c[a];
#pragma unroll
    for (int k = 1; k < 8; k++)
#pragma unroll
        for (int a = 0; a < 3; a++) { lo[a] = ce_min(lo[a], c[k * 3 + a]); hi[a] = ce_max(hi[a], c[k * 3 + a]); }
}

// caption_eval.box3d_iou (bbox.py:273-305), float32
__device__ __forceinline__ float ce_iou(const float *__restrict__ c1, const float *__restrict__ c2) {
    float lo1[3], hi1[3], lo2[3], hi2[3], d[3];
    ce_aabb(c1, lo1, hi1);
    ce_aabb(c2, lo2, hi2);
#pragma unroll
    for (int a = 0; a < 3; a++) d[a] = ce_clamp0(ce_min(hi1[a], hi2[a]) - ce_max(lo1[a], lo2[a]));
    const float inter = (d[0] * d[1]) * d[2];
    const float v1 = ((hi1[0] - lo1[0]) * (hi1[1] - lo1[1])) * (hi1[2] - lo1[2]);
    const float v2 = ((hi2[0] - lo2[0]) * (hi2[1] - lo2[1])) * (hi2[2] - lo2[2]);
    return inter / (((v1 + v2) - inter) + 1e-8f);
}

// the corpus slot of GT slot e = b * G + g, or -1
__device__ __forceinline__ int ce_slot(const int *__restrict__ scene_idx, const long long *__restrict__ obj_ids,
                                       const int *__restrict__ slot_of, int n_scenes, int n_obj, int b, long long e) {
    const int sc = scene_idx[b];
    if (sc < 0 || sc >= n_scenes) return -1;
    const long long o = obj_ids[e];
    if (o < 0 || o >= n_obj) return -1;
    return slot_of[(size_t)sc * n_obj + o];
}

__global__ __launch_bounds__(CE_THREADS) void ce_claim_kernel(const int *__restrict__ mask, const long long *__restrict__ obj_ids,
                                                              const int *__restrict__ scene_idx, const int *__restrict__ slot_of,
                                                              const int *__restrict__ assign_status, int B, int G, int n_scenes, int n_obj,
                                                              int S, unsigned long long seq, unsigned long long *__restrict__ owner,
                                                              int *__restrict__ scene_seen, int *__restrict__ status) {
    const long long e = (long long)blockIdx.x * CE_THREADS + threadIdx.x;
    if (e < B && assign_status) {
        const int st = assign_status[e];
        if (st != 0) atomicOr(status, st == 1 ? 2 : 4);
    }
    if (e >= (long long)B * G || mask[e] == 0) return;
    const int b = (int)(e / G);
    const int sc = scene_idx[b];
    if (sc >= 0 && sc < n_scenes) scene_seen[sc] = 1;                  // (every writer stores the same value)
    const int slot = ce_slot(scene_idx, obj_ids, slot_of, n_scenes, n_obj, b, e);
    if (slot < 0 || slot >= S) return;
    atomicMin(&owner[slot], (seq << CE_PRIO_BITS) + (unsigned long long)((1 << CE_PRIO_BITS) - 1 - (int)e));
}

__global__ __launch_bounds__(CE_THREADS) void ce_write_kernel(const int *__restrict__ per_gt, const float *__restrict__ pred,
                                                              const float *__restrict__ gt, const int *__restrict__ mask,
                                                              const long long *__restrict__ obj_ids, const long long *__restrict__ caps,
                                                              const int *__restrict__ lut, const int *__restrict__ scene_idx,
                                                              const int *__restrict__ slot_of, int B, int K, int G, int T, int V,
                                                              int n_scenes, int n_obj, int S, int sos, int eos, unsigned long long seq,
                                                              const unsigned long long *__restrict__ owner, int *__restrict__ cap,
                                                              int *__restrict__ cap_len, float *__restrict__ iou, int *__restrict__ status) {
    const long long e = (long long)blockIdx.x * (CE_THREADS / 64) + (threadIdx.x >> 6);   // wave-uniform
    const int lane = threadIdx.x & 63;
    if (e >= (long long)B * G || mask[e] == 0) return;
    const int b = (int)(e / G);
    const int slot = ce_slot(scene_idx, obj_ids, slot_of, n_scenes, n_obj, b, e);
    if (slot < 0 || slot >= S) return;
    if (owner[slot] != (seq << CE_PRIO_BITS) + (unsigned long long)((1 << CE_PRIO_BITS) - 1 - (int)e)) return;
    const int k = min(max(per_gt[e], 0), K - 1);
    int id = -1;
    bool bad = false;
    if (lane < T) {
        const long long t = caps[((size_t)b * K + k) * T + lane];
        if (t >= 0 && t < V) id = lut[t];
        bad = id < 0;                                                  // outside [0, V) or an id the vocabulary does not hold
    }
    const unsigned long long eos_at = __ballot(id == eos), bad_at = __ballot(bad);
    const int first = eos_at ? __ffsll((long long)eos_at) - 1 : T;     // position of the first eos, T: none
    const int n = first < T ? first + 1 : T;                           // caption tokens kept
    if (bad_at & (n >= 64 ? ~0ull : (1ull << n) - 1ull)) {             // idx2word[...] would raise before the decode stops
        if (lane == 0) atomicOr(status, 1);
        id = max(id, 0);
    }
    int *row = cap + (size_t)slot * CE_MAXT;
    if (lane < n) row[1 + lane] = id;
    if (lane == 0) {
        row[0] = sos;
        if (first >= T) row[1 + T] = eos;
        cap_len[slot] = first < T ? n + 1 : T + 2;
        iou[slot] = ce_iou(pred + ((size_t)b * K + k) * 24, gt + (size_t)e * 24);
    }
}

// ------------------------------------------------------------------------------------------------- BLEU counts, LCS lengths
__device__ __forceinline__ unsigned long long ce_key(const int *tok, int p, int n) {      // cider.hip's cd_key
    unsigned long long k = 0;
    for (int q = 0; q < n; q++) k |= (unsigned long long)(unsigned)(tok[p + q] + 1) << (16 * q);
    return k;
}

__global__ __launch_bounds__(CE_THREADS) void ce_stats_kernel(const int *__restrict__ cand, int ldc, const int *__restrict__ clen,
                                                              const int *__restrict__ tokens, int ldt, const int *__restrict__ lens,
                                                              const int *__restrict__ slot_row, const int *__restrict__ u_off,
                                                              int *__restrict__ stats, int *__restrict__ lcs) {
    __shared__ int ctok[CE_MAXT], rtok[CE_MAXT];
    __shared__ unsigned long long ckey[4 * CE_MAXT];
    const int e = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int Lc = min(max(clen[e], 0), min(ldc, CE_MAXT));
    const int r0 = u_off[e], nref = max(u_off[e + 1] - r0, 0);
    if (t < CE_MAXT) ctok[t] = t < Lc ? cand[(size_t)e * ldc + t] : -1;
    __syncthreads();
    const int n = w + 1, p = lane;                                     // this thread's n-gram: order n at position p
    const bool valid = p + n <= Lc;
    const unsigned long long key = valid ? ce_key(ctok, p, n) : 0ull;  // (a real key is never 0: every field is id + 1)
    ckey[t] = key;
    __syncthreads();
    int cnt = 0;
    bool first = valid;
    if (valid)
        for (int q = 0; q + n <= Lc; q++)
            if (ckey[w * CE_MAXT + q] == key) { cnt++; if (q < p) first = false; }
    int refmax = 0, best_d = 0x7fffffff, best_l = 0;                   // "closest" reference length: min((|l - testlen|, l))
    for (int j = 0; j < nref; j++) {
        const int row = slot_row[r0 + j];
        const int Lr = min(max(lens[row], 0), min(ldt, CE_MAXT));
        __syncthreads();                                               // (the previous reference has been read)
        if (t < CE_MAXT) rtok[t] = t < Lr ? tokens[(size_t)row * ldt + t] : -1;
        __syncthreads();
        if (first) {
            int c = 0;
            for (int q = 0; q + n <= Lr; q++) c += ce_key(rtok, q, n) == key ? 1 : 0;
            refmax = max(refmax, c);
        }
        const int d = abs(Lr - Lc);
        if (d < best_d || (d == best_d && Lr < best_l)) { best_d = d; best_l = Lr; }
    }
    int v = first ? min(cnt, refmax) : 0;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    if (lane == 0) stats[(size_t)e * 6 + w] = v;
    if (t == 0) { stats[(size_t)e * 6 + 4] = Lc; stats[(size_t)e * 6 + 5] = best_l; }
    // LCS of the candidate with reference j, wave w takes j = w, w + 4, ...
    const int mine = ctok[lane];
    const unsigned long long low = Lc >= 64 ? ~0ull : (1ull << Lc) - 1ull;
    for (int j = w; j < nref; j += CE_THREADS / 64) {
        const int row = slot_row[r0 + j];
        const int Lr = min(max(lens[row], 0), min(ldt, CE_MAXT));
        unsigned long long Vv = ~0ull;
        for (int q = 0; q < Lr; q++) {
            const int y = tokens[(size_t)row * ldt + q];
            const unsigned long long M = __ballot(lane < Lc && mine == y);
            const unsigned long long U = Vv & M;
            Vv = (Vv + U) | (Vv - U);
        }
        if (lane == 0) lcs[r0 + j] = __popcll(~Vv & low);
    }
}

// ------------------------------------------------------------------------------------------------- host
extern "C" int d3_caption_collect(const int *per_gt, const float *pred_boxes, const float *gt_boxes, const int *gt_mask,
                                  const long long *gt_obj_ids, const long long *lang_cap, const int *lut, const int *scene_idx,
                                  const int *slot_of, const int *assign_status, int B, int K, int G, int T, int V, int n_scenes, int n_obj,
                                  int S, int sos, int eos, long long batch_seq, unsigned long long *owner, int *cap, int *cap_len,
                                  float *iou, int *scene_seen, int *status, void *stream) {
    D3_CLEAR();
    if (B < 1 || K < 1 || G < 1 || T < 0 || T > CE_MAXT - 2 || (long long)B * G > (1ll << CE_PRIO_BITS) || batch_seq < 0 ||
        batch_seq >= (1ll << (63 - CE_PRIO_BITS)))
        return D3_ERR_RANGE;
    if (V < 1 || n_scenes < 1 || n_obj < 1 || S < 1 || sos < 0 || eos < 0) return D3_ERR_ARG;
    if (!per_gt || !pred_boxes || !gt_boxes || !gt_mask || !gt_obj_ids || (T > 0 && !lang_cap) || !lut || !scene_idx || !slot_of || !owner ||
        !cap || !cap_len || !iou || !scene_seen || !status)
        return D3_ERR_ARG;
    hipStream_t s = d3_stream(stream);
    const int slots = B * G;
    ce_claim_kernel<<<(slots + CE_THREADS - 1) / CE_THREADS, CE_THREADS, 0, s>>>(gt_mask, gt_obj_ids, scene_idx, slot_of, assign_status, B, G,
                                                                                 n_scenes, n_obj, S, (unsigned long long)batch_seq, owner,
                                                                                 scene_seen, status);
    const int per_block = CE_THREADS / 64;
    ce_write_kernel<<<(slots + per_block - 1) / per_block, CE_THREADS, 0, s>>>(per_gt, pred_boxes, gt_boxes, gt_mask, gt_obj_ids, lang_cap, lut,
                                                                               scene_idx, slot_of, B, K, G, T, V, n_scenes, n_obj, S, sos, eos,
                                                                               (unsigned long long)batch_seq, owner, cap, cap_len, iou, status);
    D3_LAUNCH_CHECK();
    return 0;
}

extern "C" int d3_caption_stats(const int *cand, int ldc, const int *clen, const int *tokens, int ldt, const int *lens,
                                const int *slot_row, const int *u_off, int E, int *stats, int *lcs, void *stream) {
    D3_CLEAR();
    if (E < 1 || ldc < 1 || ldt < 1) return D3_ERR_ARG;
    if (!cand || !clen || !tokens || !lens || !slot_row || !u_off || !stats || !lcs) return D3_ERR_ARG;
    ce_stats_kernel<<<E, CE_THREADS, 0, d3_stream(stream)>>>(cand, ldc, clen, tokens, ldt, lens, slot_row, u_off, stats, lcs);
    D3_LAUNCH_CHECK();
    return 0;
}
