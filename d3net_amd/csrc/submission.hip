// submission.hip -- the two leaderboard prediction writers on the device (gfx950): per test batch the records of the Scan2Cap and
// of the ScanRefer submission file, kept in device state until the one read-back at the end.
//
// Replaces, per batch, the scene x proposal loop of benchmark/benchmark_captioning.py:151-188 (predict: three `.cpu()` copies and
// one decode_caption per kept proposal, `results[scene_id] = scene_outputs`) and the row loop of benchmark/benchmark_grounding.py:
// 122-180 (predict: the (N, K, 8, 3) repeated corners copied to the host, the `cached` list of "scene-object-ann" strings); the
// files themselves (:191-194, :182-184) are written on the host from the records kept here (d3net_amd/submission.py).
//
//   sb_caption_kernel    one workgroup of 256 per batch row b, after d3_nms3d_samecls has left pick (B, K), K <= 256.  The row's
//                        scene slot s = scene_of_id[id[b]].  All threads then walk the batch's ids: a later row of the same scene
//                        makes this one return (`results[scene_id] = ...`: the last write wins), an earlier one means the scene's
//                        file position is not this row's to claim; first_seen[s] = batch_seq * 2^20 + b is stored by the first
//                        such row and only while it is unset, so a scene keeps the place of its first appearance.  Exactly one
//                        workgroup per scene and batch writes, stream order serialises the batches: plain stores.
//                        Slot t's thread holds pick[b][t] == 1; the kept slots are compacted in slot order by a wave ballot, the
//                        popcount of the lower lanes and the four wave totals through LDS, which leaves the list of kept slots in
//                        LDS.  The n box rows are then copied as one run of n * 24 floats (consecutive lanes, consecutive
//                        destination addresses, 24-float source rows), thread r writes record r's class (sem - 2, negative -> 17,
//                        truncated: the reference's one-hot position) and score, and wave w takes the captions r = w, w + 4, ...:
//                        lane j reads token j, a ballot finds the first eos, the cut is that position + 1 or T (decode_caption,
//                        lib/captioning/eval_helper.py:62-73; the host adds "sos" and the missing "eos"), the tokens are stored as
//                        int32.  No confidence threshold: the reference applies none here.
//   sb_ground_kernel     one wave64 per description row n of the N = B * C rows (scene b = n / C), 4 rows per workgroup.  Lanes
//                        stride the K slots for ONE arg-max pass over the raw scores (torch_argmax.h; no validity mask: predict
//                        takes cluster_ref.argmax(-1) as it is, an invalid slot can win), 24 lanes copy the chosen box, one
//                        coordinate each.  key = key_of[id[b]][chunk_ids[n]] numbers the row's "scene-object-ann" string; the lanes
//                        stride the earlier rows of the batch and keep = 0 when one of them has the same key (`cached` is reset per
//                        batch).  Every row writes its record at row0 + n: no ordered append, no counter.
//   Both OR bits into *status (the only atomics); the host raises on them at the end.
#include "common.h"
#include "torch_argmax.h"

#define SB_THREADS 256
#define SB_WAVES (SB_THREADS / 64)
#define SB_MAX_K 256            // proposal slots per scene: nms.hip's limit
#define SB_MAX_T 62             // caption tokens, as caption_eval.hip (64 with sos and eos)
#define SB_MAX_GROUND_K 4096    // grounding_eval.hip's limit
#define SB_SEQ_BITS 20          // rows per batch < 2^20
#define SB_NUM_CLASS 18

__device__ __forceinline__ int sb_scene(const long long *__restrict__ ids, const int *__restrict__ scene_of_id, int D, int S, int b) {
    const long long id = ids[b];
    if (id < 0 || id >= D) return -1;
    const int s = scene_of_id[id];
    return s >= 0 && s < S ? s : -1;
}

__global__ __launch_bounds__(SB_THREADS) void sb_caption_kernel(
    const float *__restrict__ corners, const float *__restrict__ sem_cls, const float *__restrict__ scores, const float *__restrict__ pick,
    const long long *__restrict__ lang_cap, const long long *__restrict__ ids, const int *__restrict__ scene_of_id, int D, int B, int K,
    int T, int V, int eos, long long batch_seq, int S, int Kcap, int Tcap, float *__restrict__ rec_box, int *__restrict__ rec_cls,
    float *__restrict__ rec_score, int *__restrict__ rec_ntok, int *__restrict__ rec_tok, int *__restrict__ count,
    long long *__restrict__ first_seen, int *__restrict__ status) {
    __shared__ int src[SB_MAX_K];                   // the kept slots, in slot order
    __shared__ int wtot[SB_WAVES];
    __shared__ int same[2];                         // the scene is named by an earlier / a later row of this batch
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int s = sb_scene(ids, scene_of_id, D, S, b);           // workgroup-uniform
    if (s < 0) {
        if (t == 0) atomicOr(status, 4);
        return;
    }
    if (t < 2) same[t] = 0;
    __syncthreads();
    for (int o = t; o < B; o += SB_THREADS)
        if (o != b && sb_scene(ids, scene_of_id, D, S, o) == s) same[o < b ? 0 : 1] = 1;     // (every writer stores the same value)
    __syncthreads();
    if (!same[0] && t == 0 && first_seen[s] < 0) first_seen[s] = (batch_seq << SB_SEQ_BITS) + b;
    if (same[1]) return;                            // a later row of this batch replaces this one
    const bool kept = t < K && pick[(size_t)b * K + t] == 1.f;
    const unsigned long long m = __ballot(kept);
    if (lane == 0) wtot[w] = __popcll(m);
    __syncthreads();
    int base = 0, n = 0;
#pragma unroll
    for (int i = 0; i < SB_WAVES; i++) { if (i < w) base += wtot[i]; n += wtot[i]; }
    if (kept) src[base + __popcll(m & d3_lanemask_lt())] = t;
    __syncthreads();                                // n <= K <= Kcap records, src[0 .. n) ascending
    const size_t rec0 = (size_t)s * Kcap;
    {
        const float *from = corners + (size_t)b * K * 24;
        float *to = rec_box + rec0 * 24;
        for (int i = t; i < n * 24; i += SB_THREADS) {
            const int r = i / 24;
            to[i] = from[src[r] * 24 + (i - r * 24)];
        }
    }
    if (t < n) {
        float c = sem_cls[(size_t)b * K + src[t]] - 2.f;
        if (c < 0.f) c = 17.f;
        const bool ok = c >= 0.f && c < (float)SB_NUM_CLASS;     // (a NaN fails)
        if (!ok) atomicOr(status, 2);
        rec_cls[rec0 + t] = ok ? (int)c : 0;
        rec_score[rec0 + t] = scores[(size_t)b * K + src[t]];
    }
    for (int r = w; r < n; r += SB_WAVES) {
        long long tok = 0;
        if (lane < T) tok = lang_cap[((size_t)b * K + src[r]) * T + lane];
        const bool bad = lane < T && (tok < 0 || tok >= V);
        const unsigned long long eos_at = __ballot(lane < T && tok == eos), bad_at = __ballot(bad);
        const int cut = eos_at ? __ffsll((long long)eos_at) : T;            // tokens kept: the first eos included
        if (bad_at & ((1ull << cut) - 1ull)) {                             // idx2word[...] would raise before the decode stops (cut <= 62)
            if (lane == 0) atomicOr(status, 1);
        }
        if (lane < T) rec_tok[(rec0 + r) * Tcap + lane] = bad ? 0 : (int)tok;
        if (lane == 0) rec_ntok[rec0 + r] = cut;
    }
    if (t == 0) count[s] = n;
}

__device__ __forceinline__ int sb_key(const long long *__restrict__ ids, const long long *__restrict__ chunk_ids,
                                      const int *__restrict__ key_of, int D, int Cmax, int C, int n) {
    const long long id = ids[n / C], ch = chunk_ids[n];
    if (id < 0 || id >= D || ch < 0 || ch >= Cmax) return -1;
    return key_of[(size_t)id * Cmax + ch];
}

__global__ __launch_bounds__(SB_THREADS) void sb_ground_kernel(
    const float *__restrict__ cluster_ref, const float *__restrict__ boxes, const long long *__restrict__ unique_multiple,
    const long long *__restrict__ object_cat, const long long *__restrict__ ids, const long long *__restrict__ chunk_ids,
    const int *__restrict__ key_of, int D, int Cmax, int N, int C, int K, long long row0, float *__restrict__ rec_box,
    int *__restrict__ rec_pred_ref, long long *__restrict__ rec_um, int *__restrict__ rec_others, int *__restrict__ rec_key,
    int *__restrict__ rec_keep, long long *__restrict__ rec_ids, int *__restrict__ status) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * SB_WAVES + (threadIdx.x >> 6);   // wave-uniform
    if (n >= N) return;
    const int b = n / C;
    const float *sc = cluster_ref + (size_t)n * K;
    float v = 0.f;
    int i = GE_NONE;
    for (int k = lane; k < K; k += 64) {
        const float x = sc[k];
        if (ge_beats(x, k, v, i)) { v = x; i = k; }
    }
    const int pred = ge_wave_argmax(v, i);
    const int key = sb_key(ids, chunk_ids, key_of, D, Cmax, C, n);
    bool seen = false;
    if (key >= 0)
        for (int m = lane; m < n; m += 64) seen = seen || sb_key(ids, chunk_ids, key_of, D, Cmax, C, m) == key;
    const bool dup = __ballot(seen) != 0ull;
    const size_t r = (size_t)(row0 + n);
    if (lane < 24) rec_box[r * 24 + lane] = boxes[((size_t)b * K + pred) * 24 + lane];
    if (lane == 0) {
        if (key < 0) atomicOr(status, 1);
        rec_pred_ref[r] = pred;
        rec_um[r] = unique_multiple[n];
        rec_others[r] = object_cat[n] == 17 ? 1 : 0;
        rec_key[r] = key;
        rec_keep[r] = key >= 0 && !dup ? 1 : 0;
        rec_ids[r * 2] = ids[b];
        rec_ids[r * 2 + 1] = chunk_ids[n];
    }
}

// ------------------------------------------------------------------------------------------------- host
extern "C" int d3_caption_submit_batch(const float *corners, const float *sem_cls, const float *scores, const float *pick,
                                       const long long *lang_cap, const long long *ids, const int *scene_of_id, int D, int B, int K,
                                       int T, int V, int eos, long long batch_seq, int S, int Kcap, int Tcap, float *rec_box,
                                       int *rec_cls, float *rec_score, int *rec_ntok, int *rec_tok, int *count, long long *first_seen,
                                       int *status, void *stream) {
    D3_CLEAR();
    if (B < 1 || B > (1 << SB_SEQ_BITS) || K < 1 || K > SB_MAX_K || T < 1 || T > SB_MAX_T || Kcap < K || Tcap < T || batch_seq < 0 ||
        batch_seq >= (1ll << (63 - SB_SEQ_BITS)))
        return D3_ERR_RANGE;
    if (D < 1 || S < 1 || V < 1 || eos < 0) return D3_ERR_ARG;
    if (!corners || !sem_cls || !scores || !pick || !lang_cap || !ids || !scene_of_id || !rec_box || !rec_cls || !rec_score || !rec_ntok ||
        !rec_tok || !count || !first_seen || !status)
        return D3_ERR_ARG;
    sb_caption_kernel<<<B, SB_THREADS, 0, d3_stream(stream)>>>(corners, sem_cls, scores, pick, lang_cap, ids, scene_of_id, D, B, K, T, V, eos,
                                                              batch_seq, S, Kcap, Tcap, rec_box, rec_cls, rec_score, rec_ntok, rec_tok,
                                                              count, first_seen, status);
    D3_LAUNCH_CHECK();
    return 0;
}

extern "C" int d3_ground_submit_batch(const float *cluster_ref, const float *proposal_boxes, const long long *unique_multiple,
                                      const long long *object_cat, const long long *ids, const long long *chunk_ids, const int *key_of,
                                      int D, int Cmax, int B, int C, int K, long long row0, float *rec_box, int *rec_pred_ref,
                                      long long *rec_unique_multiple, int *rec_others, int *rec_key, int *rec_keep, long long *rec_ids,
                                      int *status, void *stream) {
    D3_CLEAR();
    if (B < 1 || C < 1 || K < 1 || K > SB_MAX_GROUND_K || (long long)B * C > 0x7fffffffll) return D3_ERR_RANGE;
    if (D < 1 || Cmax < 1 || row0 < 0) return D3_ERR_ARG;
    if (!cluster_ref || !proposal_boxes || !unique_multiple || !object_cat || !ids || !chunk_ids || !key_of || !rec_box || !rec_pred_ref ||
        !rec_unique_multiple || !rec_others || !rec_key || !rec_keep || !rec_ids || !status)
        return D3_ERR_ARG;
    const int N = B * C;
    sb_ground_kernel<<<(N + SB_WAVES - 1) / SB_WAVES, SB_THREADS, 0, d3_stream(stream)>>>(
        cluster_ref, proposal_boxes, unique_multiple, object_cat, ids, chunk_ids, key_of, D, Cmax, N, C, K, row0, rec_box, rec_pred_ref,
        rec_unique_multiple, rec_others, rec_key, rec_keep, rec_ids, status);
    D3_LAUNCH_CHECK();
    return 0;
}
