// seg_eval.hip -- the per-point counting of the ScanNet segmentation evaluation on the device (gfx950).
//
// The reference scores PointGroup's output with two pure-Python evaluators that re-read per-scene text files:
//   * lib/evaluation/semantic_segmentation.py:18-25 build_confusion_for_scene: confusion[gt_id][pred_id] += 1 per point;
//   * lib/evaluation/instance_segmentation.py:219-274 assign_instances_for_scene (+ lib/utils/eval.py:142-158 get_instances):
//     per GT instance its vertex count and class (argmax of the bincount of its points' GT class ids, ties -> smallest id),
//     per prediction its vertex count, its void intersection (points whose GT class is outside the instance class set) and
//     one full-scene numpy pass per same-class GT instance for the intersection -- O(P * G * N) per scene.
// Here every count comes from two passes over the points, integer and order-free (bit-exact, deterministic):
//   se_points_kernel : workgroup = (chunk of SE_CHUNK points, scene).  LDS-private confusion (40 x 40) and per-instance class
//                      histogram (G x 40), flushed once per workgroup with one integer atomic per non-zero bin;
//   se_gt_kernel     : per (scene, instance) vertex count = row sum, class = first maximum of the row;
//   se_pred_kernel   : workgroup = one picked prediction, walking its contiguous member segment of proposals_idx into an LDS
//                      histogram over its scene's G instances; the row is written with plain stores (no global atomics).
// Same-address bursts (a clique of points of one instance, the common case) are folded per wave before the LDS atomic.
// The instance bound SE_MAX_INST is what keeps the point pass's LDS (G * 40 + 1600 ints) under 64 KiB.
#include "common.h"

#define SE_NCLS 40
#define SE_MAX_INST 368            // (368 * 40 + 40 * 40) * 4 B = 65,280 B of LDS in se_points_kernel
#define SE_CHUNK 4096
#define SE_T 256

// one LDS add per distinct key of the active lanes' leader: lanes sharing the first active lane's key add as one
__device__ __forceinline__ void se_lds_add(int *h, int key) {
    const int lead = __builtin_amdgcn_readfirstlane(key);
    const unsigned long long same = __ballot(key == lead);
    if (key == lead) {
        if ((__lane_id()) == __ffsll((long long)same) - 1) atomicAdd(&h[lead], __popcll(same));
    } else {
        atomicAdd(&h[key], 1);
    }
}

__global__ __launch_bounds__(SE_T) void se_points_kernel(const int *__restrict__ gt_sem, const int *__restrict__ gt_inst,
                                                         const int *__restrict__ pred_sem, const int *__restrict__ bo, int G,
                                                         int *__restrict__ confusion, int *__restrict__ inst_hist,
                                                         int *__restrict__ status) {
    extern __shared__ int sm[];                   // [0, 1600): confusion; [1600, 1600 + G * 40): instance x GT class
    const int b = blockIdx.y, t = threadIdx.x;
    const int lo = bo[b], hi = bo[b + 1];
    const int c0 = lo + blockIdx.x * SE_CHUNK;
    if (c0 >= hi) return;                         // uniform per workgroup
    const int c1 = min(hi, c0 + SE_CHUNK);
    const int nb = SE_NCLS * SE_NCLS + G * SE_NCLS;
    for (int i = t; i < nb; i += SE_T) sm[i] = 0;
    __syncthreads();
    int bad = 0;
    for (int p = c0 + t; p < c1; p += SE_T) {
        const int g = gt_sem[p], q = pred_sem[p], k = gt_inst[p];
        const bool ok = (unsigned)g < SE_NCLS && (unsigned)q < SE_NCLS && k >= 0 && k <= G;
        bad |= !ok;
        if (ok) {
            se_lds_add(sm, g * SE_NCLS + q);
            if (k > 0) se_lds_add(sm, SE_NCLS * SE_NCLS + (k - 1) * SE_NCLS + g);
        }
    }
    if (bad) atomicOr(status, 1);
    __syncthreads();
    int *ih = inst_hist + (long long)b * G * SE_NCLS;
    for (int i = t; i < nb; i += SE_T) {
        const int v = sm[i];
        if (v) atomicAdd(i < SE_NCLS * SE_NCLS ? &confusion[i] : &ih[i - SE_NCLS * SE_NCLS], v);
    }
}

// gt_stats (B, G, 2) = [vertex count, class (first maximum of the class histogram; 0 for an absent id)]
__global__ void se_gt_kernel(const int *__restrict__ inst_hist, int BG, int *__restrict__ gt_stats) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= BG) return;
    const int *h = inst_hist + (long long)e * SE_NCLS;
    int sum = 0, best = -1, arg = 0;
    for (int c = 0; c < SE_NCLS; c++) {
        const int v = h[c];
        sum += v;
        if (v > best) { best = v; arg = c; }
    }
    gt_stats[2 * e] = sum;
    gt_stats[2 * e + 1] = arg;
}

// pred_stats (n, 5) = [vertex count, void intersection, class of the first member, scene, flags]; inter (n, G)
// flags: 1 = members disagree on the predicted class; 2 = a member outside the scene of the first member, or a bad pick / segment
__global__ __launch_bounds__(SE_T) void se_pred_kernel(const int *__restrict__ pick, const int *__restrict__ pidx,
                                                       const int *__restrict__ poff, int P, long long S,
                                                       const int *__restrict__ gt_sem, const int *__restrict__ gt_inst,
                                                       const int *__restrict__ pred_sem, const int *__restrict__ bo, int B, int G,
                                                       unsigned long long inst_mask, int *__restrict__ inter,
                                                       int *__restrict__ pred_stats) {
    extern __shared__ int hist[];                 // G
    __shared__ int s_void, s_flags;
    const int j = blockIdx.x, t = threadIdx.x;
    for (int i = t; i < G; i += SE_T) hist[i] = 0;
    if (t == 0) { s_void = 0; s_flags = 0; }
    const int c = pick[j];
    long long beg = 0, end = 0;
    int flags = 0;
    if (c >= 0 && c < P) {
        beg = poff[c]; end = poff[c + 1];
        if (beg < 0 || end < beg || end > S) { beg = end = 0; flags = 2; }
    } else {
        flags = 2;
    }
    // the scene of the first member: bo[s] <= p0 < bo[s + 1]
    int scene = -1, cls0 = -1, lo = 0, hi = 0;
    if (end > beg) {
        const int p0 = pidx[2 * beg + 1];
        if (p0 >= bo[0] && p0 < bo[B]) {
            int a = 0, z = B;                     // invariant bo[a] <= p0 < bo[z]
            while (z - a > 1) {
                const int m = (a + z) >> 1;
                if (bo[m] <= p0) a = m; else z = m;
            }
            scene = a; lo = bo[a]; hi = bo[a + 1];
            cls0 = pred_sem[p0];
        } else {
            flags = 2;
        }
    }
    __syncthreads();
    int nvoid = 0;
    for (long long e = beg + t; e < end; e += SE_T) {
        const int p = pidx[2 * e + 1];
        if (p < lo || p >= hi) { flags |= 2; continue; }
        const int g = gt_sem[p], k = gt_inst[p];
        if (pred_sem[p] != cls0) flags |= 1;
        if (!((unsigned)g < SE_NCLS && ((inst_mask >> g) & 1ull))) nvoid++;
        if (k > 0 && k <= G) se_lds_add(hist, k - 1);
    }
    if (nvoid) atomicAdd(&s_void, nvoid);
    if (flags) atomicOr(&s_flags, flags);
    __syncthreads();
    int *row = inter + (long long)j * G;
    for (int i = t; i < G; i += SE_T) row[i] = hist[i];
    if (t == 0) {
        int *o = pred_stats + 5 * (long long)j;
        o[0] = (int)(end - beg); o[1] = s_void; o[2] = cls0; o[3] = scene; o[4] = s_flags;
    }
}

extern "C" int d3_seg_eval_max_inst(void) { return SE_MAX_INST; }

extern "C" size_t d3_seg_eval_ws_bytes(int B, int G) {
    return (size_t)(B > 0 ? B : 0) * (size_t)(G > 0 ? G : 0) * SE_NCLS * sizeof(int);
}

extern "C" int d3_seg_eval(const int *gt_sem, const int *gt_inst, const int *pred_sem, const int *batch_offsets, int B, int N,
                           int max_scene_points, int G, const int *pick, int n_pick, const int *proposals_idx,
                           const int *proposals_offset, int P, long long S, unsigned long long inst_class_mask, int *confusion,
                           int *gt_stats, int *pred_stats, int *inter, int *status, void *ws, size_t ws_bytes, void *stream) {
    D3_CLEAR();
    if (B < 1 || N < 0 || G < 0 || n_pick < 0 || P < 0 || S < 0 || max_scene_points < 0) return D3_ERR_ARG;
    if (G > SE_MAX_INST) return D3_ERR_RANGE;
    if (ws_bytes < d3_seg_eval_ws_bytes(B, G)) return D3_ERR_WORKSPACE;
    hipStream_t s = d3_stream(stream);
    D3_CHECK(hipMemsetAsync(confusion, 0, SE_NCLS * SE_NCLS * sizeof(int), s));
    D3_CHECK(hipMemsetAsync(status, 0, sizeof(int), s));
    if (G > 0) D3_CHECK(hipMemsetAsync(ws, 0, d3_seg_eval_ws_bytes(B, G), s));
    if (N > 0 && max_scene_points > 0) {
        const dim3 grid((max_scene_points + SE_CHUNK - 1) / SE_CHUNK, B);
        const size_t lds = (size_t)(SE_NCLS * SE_NCLS + G * SE_NCLS) * sizeof(int);
        se_points_kernel<<<grid, SE_T, lds, s>>>(gt_sem, gt_inst, pred_sem, batch_offsets, G, confusion, (int *)ws, status);
    }
    if (G > 0) se_gt_kernel<<<(B * G + 255) / 256, 256, 0, s>>>((const int *)ws, B * G, gt_stats);
    if (n_pick > 0)
        se_pred_kernel<<<n_pick, SE_T, (size_t)G * sizeof(int), s>>>(pick, proposals_idx, proposals_offset, P, S, gt_sem, gt_inst,
                                                                     pred_sem, batch_offsets, B, G, inst_class_mask, inter, pred_stats);
    D3_LAUNCH_CHECK();
    return 0;
}
