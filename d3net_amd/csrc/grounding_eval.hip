// grounding_eval.hip -- the grounding validation on the device (gfx950): per validation batch the referred-box choice of every
// description, its IoU with the GT box and the Acc@kIoU cell counters of the epoch.
//
// Replaces, per batch, lib/grounding/eval_helper.py:28-137 (get_eval: the arg-max one-hot, the per-description python loop with one
// .cpu().numpy() IoU each) and the per-batch list appends of scripts/eval.py:197-262 (eval_grounding); the table of
// scripts/eval.py:305-426 is formed on the host from the integers kept here (d3net_amd/grounding_eval.py).
//
//   ge_batch_kernel      one wave64 per description row n of the N = B * C rows (scene b = n / C), 4 rows per workgroup.
//                        Lanes stride the K proposal slots for three arg-max passes (scores, scores * valid, labels), a butterfly of
//                        __shfl_xor leaves the winners in every lane.  The rule is torch.argmax on the CPU: a NaN ranks above every
//                        number, +0 == -0, the lowest index wins among equals (within a lane the indices ascend and only a strictly
//                        better value replaces the held one; across lanes the lower index wins a draw).  The product with the 0/1
//                        validity is formed in float32 as the reference forms it: an invalid slot scores +-0 (a NaN or an infinity
//                        stays / becomes NaN), so a row whose valid scores are all negative picks its lowest invalid slot.
//                        The three boxes a row needs (proposal pred_ref, proposal gt_ref, the GT box) go through LDS, 24 lanes load
//                        one coordinate each; lane 0 takes the two IoUs in float32 in get_aabb3d_iou's operation order
//                        (lib/utils/bbox.py:221-244, numpy's NaN-propagating min / max; -ffp-contract=off).  No (N, K) IoU matrix, no
//                        repeated boxes.  Counters: every row adds to its cell [m][o][rows, ref_acc, iou >= 0.25, iou >= 0.5] of an
//                        int table in LDS, then at most 24 + 1 integer atomicAdd per workgroup reach the int64 table and the batch's
//                        language counter: order-free, bit-reproducible.  A NaN IoU compares false.
#include "common.h"
#include "torch_argmax.h"       // ge_beats, ge_wave_argmax, GE_NONE: the arg-max rule, shared with submission.hip

#define GE_THREADS 256
#define GE_WAVES (GE_THREADS / 64)
#define GE_MAX_K 4096
#define GE_MAX_LANG 64

// numpy's min / max / np.minimum / np.maximum: a NaN propagates
__device__ __forceinline__ float ge_min(float a, float b) { return a != a ? a : (b != b ? b : fminf(a, b)); }
__device__ __forceinline__ float ge_max(float a, float b) { return a != a ? a : (b != b ? b : fmaxf(a, b)); }

// get_aabb3d_iou (bbox.py:221-244) of two boxes of 8 corners each, float32
__device__ __forceinline__ float ge_iou(const float *c1, const float *c2) {
    float lo1[3], hi1[3], lo2[3], hi2[3], d[3];
#pragma unroll
    for (int a = 0; a < 3; a++) { lo1[a] = hi1[a] = c1[a]; lo2[a] = hi2[a] = c2[a]; }
#pragma unroll
    for (int k = 1; k < 8; k++)
#pragma unroll
        for (int a = 0; a < 3; a++) {
            lo1[a] = ge_min(lo1[a], c1[k * 3 + a]); hi1[a] = ge_max(hi1[a], c1[k * 3 + a]);
            lo2[a] = ge_min(lo2[a], c2[k * 3 + a]); hi2[a] = ge_max(hi2[a], c2[k * 3 + a]);
        }
#pragma unroll
    for (int a = 0; a < 3; a++) d[a] = ge_max(ge_min(hi1[a], hi2[a]) - ge_max(lo1[a], lo2[a]), 0.f);
    const float inter = (d[0] * d[1]) * d[2];
    const float v1 = ((hi1[0] - lo1[0]) * (hi1[1] - lo1[1])) * (hi1[2] - lo1[2]);
    const float v2 = ((hi2[0] - lo2[0]) * (hi2[1] - lo2[1])) * (hi2[2] - lo2[2]);
    return inter / (((v1 + v2) - inter) + 1e-8f);
}

__global__ __launch_bounds__(GE_THREADS) void ge_batch_kernel(
    const float *__restrict__ cluster_ref, const float *__restrict__ cluster_labels, const float *__restrict__ proposal_mask,
    const float *__restrict__ proposal_boxes, const float *__restrict__ ref_boxes, const long long *__restrict__ unique_multiple,
    const long long *__restrict__ object_cat, const float *__restrict__ lang_scores, int n_lang, const long long *__restrict__ scene_ids,
    const long long *__restrict__ chunk_ids, int N, int C, int K, long long row0, unsigned long long *__restrict__ table,
    unsigned long long *__restrict__ lang_correct, float *__restrict__ rec_iou, float *__restrict__ rec_best_iou,
    int *__restrict__ rec_pred_ref, int *__restrict__ rec_gt_ref, int *__restrict__ rec_ref_acc, float *__restrict__ rec_pred_box,
    float *__restrict__ rec_gt_box, long long *__restrict__ rec_ids, int *__restrict__ status) {
    __shared__ float box[GE_WAVES][3][24];          // per wave: proposal pred_ref, proposal gt_ref, the GT box
    __shared__ int cell[25];                        // table[3][2][4] of this workgroup, then its language count
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int n = blockIdx.x * GE_WAVES + w;        // wave-uniform
    const bool active = n < N;
    if (t < 25) cell[t] = 0;
    int top = 0, pred_ref = 0, gt_ref = 0, b = 0;
    if (active) {
        b = n / C;
        const float *sc = cluster_ref + (size_t)n * K, *lb = cluster_labels + (size_t)n * K, *mk = proposal_mask + (size_t)b * K;
        float v_top = 0.f, v_pred = 0.f, v_gt = 0.f;
        int i_top = GE_NONE, i_pred = GE_NONE, i_gt = GE_NONE;
        for (int k = lane; k < K; k += 64) {
            const float s = sc[k], l = lb[k], mv = mk[k];
            const float p = s * (mv >= 1.f && mv < 2.f ? 1.f : 0.f);       // `.long() == 1` (truncation), then the float32 product
            if (ge_beats(s, k, v_top, i_top)) { v_top = s; i_top = k; }
            if (ge_beats(p, k, v_pred, i_pred)) { v_pred = p; i_pred = k; }
            if (ge_beats(l, k, v_gt, i_gt)) { v_gt = l; i_gt = k; }
        }
        top = ge_wave_argmax(v_top, i_top);
        pred_ref = ge_wave_argmax(v_pred, i_pred);
        gt_ref = ge_wave_argmax(v_gt, i_gt);
        if (lane < 24) {
            const float *pb = proposal_boxes + (size_t)b * K * 24;
            box[w][0][lane] = pb[(size_t)pred_ref * 24 + lane];
            box[w][1][lane] = pb[(size_t)gt_ref * 24 + lane];
            box[w][2][lane] = ref_boxes[(size_t)n * 24 + lane];
        }
    }
    __syncthreads();                                // the boxes and the zeroed cells are in LDS
    if (active) {
        bool bad = false;
        if (lane < 24) {
            const float a0 = box[w][0][lane], a1 = box[w][1][lane], a2 = box[w][2][lane];
            bad = !(isfinite(a0) && isfinite(a1) && isfinite(a2));
            if (rec_pred_box) rec_pred_box[(size_t)(row0 + n) * 24 + lane] = a0;
            if (rec_gt_box) rec_gt_box[(size_t)(row0 + n) * 24 + lane] = a2;
        }
        const unsigned long long bad_at = __ballot(bad);
        int lang_ok = 0;
        if (lang_scores) {
            const bool has = lane < n_lang;
            const float v = has ? lang_scores[(size_t)n * n_lang + lane] : 0.f;
            lang_ok = (long long)ge_wave_argmax(v, has ? lane : GE_NONE) == object_cat[n] ? 1 : 0;
        }
        if (lane == 0) {
            const float iou = ge_iou(box[w][0], box[w][2]), best = ge_iou(box[w][1], box[w][2]);
            const int ref_acc = cluster_labels[(size_t)n * K + top] == 1.f ? 1 : 0;
            const long long um = unique_multiple[n];
            const int m = um == 0 ? 0 : (um == 1 ? 1 : 2), o = object_cat[n] == 17 ? 1 : 0;
            int *c = cell + (m * 2 + o) * 4;
            atomicAdd(c + 0, 1);
            if (ref_acc) atomicAdd(c + 1, 1);
            if (iou >= 0.25f) atomicAdd(c + 2, 1);
            if (iou >= 0.5f) atomicAdd(c + 3, 1);
            if (lang_ok) atomicAdd(cell + 24, 1);
            if (bad_at) atomicOr(status, 1);
            const size_t r = (size_t)(row0 + n);
            if (rec_iou) rec_iou[r] = iou;
            if (rec_best_iou) rec_best_iou[r] = best;
            if (rec_pred_ref) rec_pred_ref[r] = pred_ref;
            if (rec_gt_ref) rec_gt_ref[r] = gt_ref;
            if (rec_ref_acc) rec_ref_acc[r] = ref_acc;
            if (rec_ids) { rec_ids[r * 2] = scene_ids[b]; rec_ids[r * 2 + 1] = chunk_ids[n]; }
        }
    }
    __syncthreads();                                // the workgroup's counts are complete
    if (t < 24 && cell[t]) atomicAdd(table + t, (unsigned long long)cell[t]);
    if (t == 24 && lang_correct && cell[24]) atomicAdd(lang_correct, (unsigned long long)cell[24]);
}

extern "C" int d3_ground_eval_batch(const float *cluster_ref, const float *cluster_labels, const float *proposal_mask,
                                    const float *proposal_boxes, const float *ref_boxes, const long long *unique_multiple,
                                    const long long *object_cat, const float *lang_scores, int n_lang, const long long *scene_ids,
                                    const long long *chunk_ids, int B, int C, int K, long long row0, long long *table,
                                    long long *lang_correct, float *rec_iou, float *rec_best_iou, int *rec_pred_ref, int *rec_gt_ref,
                                    int *rec_ref_acc, float *rec_pred_box, float *rec_gt_box, long long *rec_ids, int *status,
                                    void *stream) {
    D3_CLEAR();
    if (B < 1 || C < 1 || K < 1 || K > GE_MAX_K || (long long)B * C > 0x7fffffffll) return D3_ERR_RANGE;
    if (lang_scores && (n_lang < 1 || n_lang > GE_MAX_LANG)) return D3_ERR_RANGE;
    if (!cluster_ref || !cluster_labels || !proposal_mask || !proposal_boxes || !ref_boxes || !unique_multiple || !object_cat || !table ||
        !status || row0 < 0)
        return D3_ERR_ARG;
    if ((lang_scores && !lang_correct) || (rec_ids && (!scene_ids || !chunk_ids))) return D3_ERR_ARG;
    const int N = B * C;
    ge_batch_kernel<<<(N + GE_WAVES - 1) / GE_WAVES, GE_THREADS, 0, d3_stream(stream)>>>(
        cluster_ref, cluster_labels, proposal_mask, proposal_boxes, ref_boxes, unique_multiple, object_cat, lang_scores, n_lang, scene_ids,
        chunk_ids, N, C, K, row0, (unsigned long long *)table, (unsigned long long *)lang_correct, rec_iou, rec_best_iou, rec_pred_ref,
        rec_gt_ref, rec_ref_acc, rec_pred_box, rec_gt_box, rec_ids, status);
    D3_LAUNCH_CHECK();
    return 0;
}
