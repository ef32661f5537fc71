// lang_prep.hip -- the description half of the reference's PipelineDataset.__getitem__ on the device (driven by
// d3net_amd/lang_prep.py): language features as a gather from the device-resident token and GloVe tables
// (lib/dataset/pipeline.py:103-138, :504-565), and the grounding / rotation targets from the stacked box labels (:250-278).
// Plain loads and stores only: every output element has exactly one writer, so there are no atomics and no memsets.
#include "common.h"

#define LP_BLOCK 256
#define LP_MAX_L 4096                 // positions per description (the shipped configs use 32 and 128)
#define LP_MAX_SLOTS (1 << 20)        // S = B * C description slots, B scenes, R box rows: far above any batch

// ---------------------------------------------------------------------------------------------- d3_lang_features
// One thread per (slot, position, quad): the grid is flat over S * L * D/4, so a row of 75 float4 (D = 300) leaves no lane idle.
// The thread of quad 0 also writes lang_ids[slot, p]; the thread of (p 0, quad 0) writes lang_len[slot].
__global__ void __launch_bounds__(LP_BLOCK)
lp_features_kernel(const int *__restrict__ tokens, const int *__restrict__ lens, const float4 *__restrict__ glove, int Q, int L, int unk,
                   const int *__restrict__ rows, const int *__restrict__ erase_ptr, const int *__restrict__ erase_pos, int total,
                   float4 *__restrict__ lang_feat, long long *__restrict__ lang_ids, long long *__restrict__ lang_len) {
    int idx = (int)(blockIdx.x * LP_BLOCK + threadIdx.x);
    if (idx >= total) return;
    int row = idx / Q, q = idx - row * Q;                 // row = slot * L + p
    int slot = row / L, p = row - slot * L;
    int r = rows[slot];
    int n = 0, tok = 0, src = -1;                         // src: the GloVe row to copy, -1 = zeros
    if (r >= 0) {
        n = lens[r];
        if (p < n) src = tok = tokens[(size_t)r * L + p];
        for (int e = erase_ptr[slot], e1 = erase_ptr[slot + 1]; e < e1; ++e)
            if (erase_pos[e] == p) src = unk;             // pipeline.py:554-565: the features change, the ids do not
    }
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (src >= 0) v = glove[(size_t)src * Q + q];
    lang_feat[idx] = v;
    if (q == 0) {
        lang_ids[row] = tok;
        if (p == 0) lang_len[slot] = n;
    }
}

struct LpFeatWs { int *rows, *eptr, *epos; };
static void lp_features_layout(D3Carver &c, int S, int E, LpFeatWs &w) {
    w.rows = c.take<int>(S + 1); w.eptr = c.take<int>(S + 1); w.epos = c.take<int>(E > 0 ? E : 1);
}

size_t d3_lang_features_ws_bytes(int S, int E) {
    if (S < 0 || S > LP_MAX_SLOTS || E < 0 || (long long)E > (long long)LP_MAX_SLOTS * 64) return 0;
    D3Carver c(nullptr, 0);
    LpFeatWs w;
    lp_features_layout(c, S, E, w);
    return c.off;
}

int d3_lang_features(const int *tokens, const int *lens, int Nd, const float *glove, int V, int D, int L, int unk,
                     const int *rows_host, const int *erase_ptr_host, const int *erase_pos_host, int S, float *lang_feat,
                     long long *lang_ids, long long *lang_len, void *ws, size_t ws_bytes, void *stream) {
    if (D <= 0 || D % 4 != 0 || L < 1 || S < 0 || Nd < 0 || V < 1 || unk < 0 || unk >= V) return D3_ERR_ARG;
    if (S == 0) return 0;
    if (!rows_host || !erase_ptr_host) return D3_ERR_ARG;
    if (L > LP_MAX_L || S > LP_MAX_SLOTS) return D3_ERR_RANGE;
    int Q = D / 4;
    if ((long long)S * L * Q > 0x7fffffffll) return D3_ERR_RANGE;
    if (erase_ptr_host[0] != 0) return D3_ERR_ARG;
    for (int s = 0; s < S; ++s) {
        if (rows_host[s] < -1 || rows_host[s] >= Nd) return D3_ERR_RANGE;
        if (erase_ptr_host[s + 1] < erase_ptr_host[s] || erase_ptr_host[s + 1] - erase_ptr_host[s] > L) return D3_ERR_ARG;
    }
    int E = erase_ptr_host[S];
    if (E > 0 && !erase_pos_host) return D3_ERR_ARG;
    for (int e = 0; e < E; ++e)
        if (erase_pos_host[e] < 0 || erase_pos_host[e] >= L) return D3_ERR_ARG;
    if (!tokens || !lens || !glove || !lang_feat || !lang_ids || !lang_len) return D3_ERR_ARG;
    D3Carver cv(ws, ws_bytes);
    LpFeatWs w;
    lp_features_layout(cv, S, E, w);
    if (!cv.ok()) return D3_ERR_WORKSPACE;
    int *rows = w.rows, *eptr = w.eptr, *epos = w.epos;
    hipStream_t st = d3_stream(stream);
    D3_CLEAR();
    // pageable host memory is staged before hipMemcpyAsync returns; lang_prep.py keeps its arrays referenced all the same
    D3_CHECK(hipMemcpyAsync(rows, rows_host, (size_t)S * sizeof(int), hipMemcpyHostToDevice, st));
    D3_CHECK(hipMemcpyAsync(eptr, erase_ptr_host, (size_t)(S + 1) * sizeof(int), hipMemcpyHostToDevice, st));
    if (E > 0) D3_CHECK(hipMemcpyAsync(epos, erase_pos_host, (size_t)E * sizeof(int), hipMemcpyHostToDevice, st));
    int total = S * L * Q;
    hipLaunchKernelGGL(lp_features_kernel, dim3((total + LP_BLOCK - 1) / LP_BLOCK), dim3(LP_BLOCK), 0, st, tokens, lens,
                       (const float4 *)glove, Q, L, unk, (const int *)rows, (const int *)eptr, (const int *)epos, total,
                       (float4 *)lang_feat, lang_ids, lang_len);
    D3_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------------- d3_ref_targets
// One wave per (scene, slot): ref_box_label[b, c, :] and the corners of the highest matching row (pipeline.py:267-278: every
// match overwrites the slot's corners, so the last one stays).
__global__ void __launch_bounds__(D3_WAVE)
lp_ref_kernel(const long long *__restrict__ gt_ids, const long long *__restrict__ gt_label, const float *__restrict__ gt_bbox,
              const long long *__restrict__ object_id, int C, int R, long long *__restrict__ ref_label, float *__restrict__ ref_corner) {
    int slot = (int)blockIdx.x, b = slot / C, lane = d3_lane();
    long long oid = object_id[slot];
    int best = -1;
    for (int i = lane; i < R; i += D3_WAVE) {
        bool m = gt_label[(size_t)b * R + i] == 1 && gt_ids[(size_t)b * R + i] == oid;
        ref_label[(size_t)slot * R + i] = m ? 1 : 0;
        if (m) best = i;
    }
    for (int o = 32; o > 0; o >>= 1) best = max(best, __shfl_xor(best, o));
    if (lane < 24) ref_corner[(size_t)slot * 24 + lane] = best >= 0 ? gt_bbox[((size_t)b * R + best) * 24 + lane] : 0.f;
}

// One wave per (scene, row): the Scan2CAD rotation of a labelled box whose id is in the scene's table (pipeline.py:250-264).
__global__ void __launch_bounds__(D3_WAVE)
lp_rot_kernel(const long long *__restrict__ gt_ids, const long long *__restrict__ gt_label, int R, const int *__restrict__ rot_off,
              const int *__restrict__ rot_ids, const float *__restrict__ rot_mats, const int *__restrict__ scene,
              float *__restrict__ rots, long long *__restrict__ rot_masks) {
    int row = (int)blockIdx.x, b = row / R, lane = d3_lane();
    int sc = scene[b], best = -1;
    if (sc >= 0 && gt_label[row] == 1) {
        long long id = gt_ids[row];
        for (int t = rot_off[sc] + lane, t1 = rot_off[sc + 1]; t < t1; t += D3_WAVE)
            if ((long long)rot_ids[t] == id) best = t;
    }
    for (int o = 32; o > 0; o >>= 1) best = max(best, __shfl_xor(best, o));
    if (lane < 9) rots[(size_t)row * 9 + lane] = best >= 0 ? rot_mats[(size_t)best * 9 + lane] : 0.f;
    if (lane == 0) rot_masks[row] = best >= 0 ? 1 : 0;
}

static int *lp_ref_layout(D3Carver &c, int B) { return c.take<int>(B + 1); }      // the scene index of every batch row

size_t d3_ref_targets_ws_bytes(int B) {
    if (B < 0 || B > LP_MAX_SLOTS) return 0;
    D3Carver c(nullptr, 0);
    lp_ref_layout(c, B);
    return c.off;
}

int d3_ref_targets(const long long *gt_ids, const long long *gt_label, const float *gt_bbox, const long long *object_id, int B, int C,
                   int R, const int *rot_off, const int *rot_ids, const float *rot_mats, int Ns, const int *scene_host,
                   long long *ref_label, float *ref_corner, float *rots, long long *rot_masks, void *ws, size_t ws_bytes, void *stream) {
    if (B < 0 || C < 0 || R < 1 || Ns < 0) return D3_ERR_ARG;
    if (B == 0) return 0;
    if (B > LP_MAX_SLOTS || R > LP_MAX_SLOTS || (long long)B * C > LP_MAX_SLOTS || (long long)B * R > LP_MAX_SLOTS) return D3_ERR_RANGE;
    if (!scene_host || !gt_ids || !gt_label || !gt_bbox || !rots || !rot_masks) return D3_ERR_ARG;
    if (C > 0 && (!object_id || !ref_label || !ref_corner)) return D3_ERR_ARG;
    if (Ns > 0 && (!rot_off || !rot_ids || !rot_mats)) return D3_ERR_ARG;
    for (int b = 0; b < B; ++b)
        if (scene_host[b] < -1 || scene_host[b] >= Ns) return D3_ERR_RANGE;
    D3Carver cv(ws, ws_bytes);
    int *scene = lp_ref_layout(cv, B);
    if (!cv.ok()) return D3_ERR_WORKSPACE;
    hipStream_t st = d3_stream(stream);
    D3_CLEAR();
    D3_CHECK(hipMemcpyAsync(scene, scene_host, (size_t)B * sizeof(int), hipMemcpyHostToDevice, st));
    if (C > 0) {
        hipLaunchKernelGGL(lp_ref_kernel, dim3(B * C), dim3(D3_WAVE), 0, st, gt_ids, gt_label, gt_bbox, object_id, C, R, ref_label,
                           ref_corner);
        D3_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(lp_rot_kernel, dim3(B * R), dim3(D3_WAVE), 0, st, gt_ids, gt_label, R, rot_off, rot_ids, rot_mats,
                       (const int *)scene, rots, rot_masks);
    D3_LAUNCH_CHECK();
    return 0;
}
