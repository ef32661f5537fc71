// det_eval.hip -- detection mAP on the device (gfx950): the per-batch match of detections to GT boxes and the epoch-end
// precision / recall / VOC AP pass.
//
// Replaces, per validation batch, the list building of lib/det/ap_helper.py:80-150 (parse_predictions after its NMS) and :152-193
// (parse_groundtruths), and at the end of the epoch lib/det/eval_det.py:74-158 (eval_det_cls), :21-52 (voc_ap) and :165-204
// (eval_det), as d3net_amd/evaluator.py restates them on the host.
//
//   d3_det_match   one workgroup of 256 threads per scene, thread t owns proposal t (K <= 256), the GT boxes of the scene live
//                  in LDS (G <= 256).  A detection is kept when pick == 1 and score > float32(conf_thresh); for a kept detection
//                  the thread walks the valid GT boxes of its class in index order with eval_det_cls's strict `>` (the lowest j
//                  wins on equal IoU) in float64, operation for operation as evaluator.box3d_iou (-ffp-contract=off).
//                  The sequential "has this GT box been taken" loop of eval_det_cls is replaced by an order-free rule: detection
//                  d is a true positive at threshold tau iff ovmax_d > tau and no EARLIER detection d' of its scene and class has
//                  jmax_d' == jmax_d and ovmax_d' > tau (a GT box is taken by the first detection that clears tau on it, and only
//                  by such a detection).  Earlier = higher score, on exactly equal scores the lower proposal index.  K compares
//                  per thread over LDS, no serial walk.  Every output element is written once; the only atomic is an integer OR
//                  into the status word.
//   d3_det_ap      one workgroup per (class, threshold) over that class's records in descending score: the TP total forward, then
//                  256 records per pass from the END of the segment: the inclusive TP scan of the pass is placed by the carried
//                  total, precision's reverse running maximum is carried the same way, and the area terms
//                  (rec_k - rec_{k-1}) * envelope_k are summed where recall changes.  The (0,0) sentinel is rec_{-1} = 0 / npos;
//                  the (1,0) sentinel contributes (1 - rec) * 0.
#include "common.h"
#include <float.h>

#define DE_MAX 256        // proposals and GT slots per scene
#define DE_MAXT 4         // IoU thresholds per launch
#define DE_MAXC 256       // classes
#define DE_THREADS 256

struct DeThr { double t[DE_MAXT]; };
struct DeBox { double lo[3], hi[3], vol; };

__device__ __forceinline__ bool de_finite(float x) { return fabsf(x) <= 3.402823466e+38f; }

// np.maximum(x, 0): a NaN stays, -0.0 stays
__device__ __forceinline__ double de_max0(double x) { return (x >= 0.0 || x != x) ? x : 0.0; }

// AABB over the 8 corners (c1.min(0), c1.max(0)) and its volume (mx - mn).prod() = (x * y) * z; -> any coordinate non-finite
__device__ __forceinline__ bool de_box(const float *__restrict__ c, DeBox &q) {
    float lo[3] = {c[0], c[1], c[2]}, hi[3] = {c[0], c[1], c[2]};
    bool bad = !de_finite(c[0]) || !de_finite(c[1]) || !de_finite(c[2]);
#pragma unroll
    for (int k = 1; k < 8; k++)
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const float v = c[k * 3 + a];
            bad |= !de_finite(v);
            lo[a] = fminf(lo[a], v); hi[a] = fmaxf(hi[a], v);
        }
#pragma unroll
    for (int a = 0; a < 3; a++) { q.lo[a] = (double)lo[a]; q.hi[a] = (double)hi[a]; }
    q.vol = ((q.hi[0] - q.lo[0]) * (q.hi[1] - q.lo[1])) * (q.hi[2] - q.lo[2]);
    return bad;
}

// evaluator.box3d_iou (box_util.py:97-121) in float64
__device__ __forceinline__ double de_iou(const DeBox &a, const DeBox &b) {
    const double x = de_max0(fmin(a.hi[0], b.hi[0]) - fmax(a.lo[0], b.lo[0]));
    const double y = de_max0(fmin(a.hi[1], b.hi[1]) - fmax(a.lo[1], b.lo[1]));
    const double z = de_max0(fmin(a.hi[2], b.hi[2]) - fmax(a.lo[2], b.lo[2]));
    const double inter = (x * y) * z;
    return inter / (((a.vol + b.vol) - inter) + 1e-8);
}

__global__ __launch_bounds__(DE_THREADS) void de_match_kernel(
    const float *__restrict__ pred, const int *__restrict__ pred_cls, const float *__restrict__ scores, const float *__restrict__ pick,
    double conf, const float *__restrict__ gt, const float *__restrict__ gt_mask, const int *__restrict__ gt_cls, int K, int G, int NC,
    DeThr thr, int T, int *__restrict__ kept, int *__restrict__ cls_out, float *__restrict__ score_out, double *__restrict__ ovmax_out,
    int *__restrict__ jmax_out, int *__restrict__ tp_out, int *__restrict__ gt_count, int *__restrict__ status) {
    __shared__ DeBox gb[DE_MAX];
    __shared__ int gcl[DE_MAX];                          // class of a valid GT box, -1: masked
    __shared__ double pov[DE_MAX];
    __shared__ float psc[DE_MAX];
    __shared__ int pcl[DE_MAX], pjm[DE_MAX];             // class of a kept detection (-1: not kept), its jmax
    const int b = blockIdx.x, t = threadIdx.x;
    int bad = 0;
    if (t < G) {
        const size_t e = (size_t)b * G + t;
        int c = -1;
        if (gt_mask[e] == 1.f) {
            c = gt_cls[e];
            if (c < 0 || c >= NC) { bad |= 2; c = -1; }
            else if (de_box(gt + e * 24, gb[t])) bad |= 1;
        }
        gcl[t] = c;
    }
    DeBox me;
    int mycls = -1;
    float mysc = 0.f;
    if (t < K) {
        const size_t e = (size_t)b * K + t;
        const int c = pred_cls[e];
        mysc = scores[e] + 0.f;                          // -0.0 -> +0.0: one key for what compares equal
        if (pick[e] == 1.f && mysc > (float)conf && c >= 0 && c < NC) {   // float32, as numpy compares it with a Python float
            mycls = c;
            if (de_box(pred + e * 24, me)) bad |= 1;
        }
    }
    __syncthreads();
    for (int c = t; c < NC; c += DE_THREADS) {
        int n = 0;
        for (int j = 0; j < G; j++) n += gcl[j] == c ? 1 : 0;
        gt_count[(size_t)b * NC + c] = n;
    }
    double ov = -__builtin_inf();
    int jm = -1;
    if (t < K) {
        if (mycls >= 0)
            for (int j = 0; j < G; j++)
                if (gcl[j] == mycls) {
                    const double iou = de_iou(me, gb[j]);
                    if (iou > ov) { ov = iou; jm = j; }
                }
        pov[t] = ov; pjm[t] = jm; psc[t] = mysc; pcl[t] = mycls;
    }
    __syncthreads();
    if (t < K) {
        int bits = 0;
        if (mycls >= 0 && jm >= 0) {
            int taken = 0;
            for (int d = 0; d < K; d++)
                if (d != t && pcl[d] == mycls && pjm[d] == jm && (psc[d] > mysc || (psc[d] == mysc && d < t))) {
                    const double o = pov[d];
#pragma unroll
                    for (int q = 0; q < DE_MAXT; q++)
                        if (q < T && o > thr.t[q]) taken |= 1 << q;
                }
#pragma unroll
            for (int q = 0; q < DE_MAXT; q++)
                if (q < T && ov > thr.t[q] && !((taken >> q) & 1)) bits |= 1 << q;
        }
        const size_t e = (size_t)b * K + t;
        kept[e] = mycls >= 0 ? 1 : 0;
        cls_out[e] = mycls;
        score_out[e] = mysc;
        ovmax_out[e] = ov;
        jmax_out[e] = jm;
        tp_out[e] = bits;
    }
    if (bad) atomicOr(status, bad);
}

// ------------------------------------------------------------------------------------------------- AP
__device__ __forceinline__ int de_block_sum_i(int v, int *ws) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = v;
    __syncthreads();
    const int s = ((ws[0] + ws[1]) + ws[2]) + ws[3];
    __syncthreads();
    return s;
}

__device__ __forceinline__ double de_block_sum_d(double v, double *ws) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = v;
    __syncthreads();
    const double s = ((ws[0] + ws[1]) + ws[2]) + ws[3];
    __syncthreads();
    return s;
}

// inclusive scan over the 256 threads; total = the sum of all
__device__ __forceinline__ int de_block_scan_i(int v, int *ws, int &total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(v, d, 64);
        if (lane >= d) v += o;
    }
    if (lane == 63) ws[w] = v;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) { if (i < w) base += ws[i]; tot += ws[i]; }
    __syncthreads();
    total = tot;
    return v + base;
}

// max over the threads >= this one; all = the max of all
__device__ __forceinline__ double de_block_rmax_d(double v, double *ws, double &all) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double o = __shfl_down(v, d, 64);
        if (lane + d < 64) v = fmax(v, o);
    }
    if (lane == 0) ws[w] = v;
    __syncthreads();
    double a = ws[0];
#pragma unroll
    for (int i = 1; i < 4; i++) { if (i > w) v = fmax(v, ws[i]); a = fmax(a, ws[i]); }
    __syncthreads();
    all = a;
    return v;
}

// tp (N) int32: bit q = true positive at threshold q, records ordered by (class, descending score); off (NC + 1) segment bounds;
// gt_count (S, NC).  table (T, NC, 4) = AP, last recall, detections, present
__global__ __launch_bounds__(DE_THREADS) void de_ap_kernel(const int *__restrict__ tp, const int *__restrict__ off,
                                                           const int *__restrict__ gt_count, int S, int N, int NC,
                                                           double *__restrict__ table) {
    __shared__ int wi[4];
    __shared__ double wd[4];
    const int c = blockIdx.x, q = blockIdx.y, t = threadIdx.x;
    int part = 0;
    for (int s = t; s < S; s += DE_THREADS) part += gt_count[(size_t)s * NC + c];
    const int npos = de_block_sum_i(part, wi);
    const int lo = min(max(off[c], 0), N), hi = min(max(off[c + 1], lo), N);
    const int n = hi - lo;
    part = 0;
    for (int i = lo + t; i < hi; i += DE_THREADS) part += (tp[i] >> q) & 1;
    const int total = de_block_sum_i(part, wi);
    const double denom = (double)npos + 1e-8;            // eval_det.py:150 rec = tp / float(npos + 1e-8)
    int carry = total;                                   // TP count up to the end of the pass being worked on
    double env = 0.0, acc = 0.0;                         // mpre's trailing sentinel
    for (int ch = (n + DE_THREADS - 1) / DE_THREADS - 1; ch >= 0; ch--) {
        const int k = ch * DE_THREADS + t;               // position in the segment
        const bool in = k < n;
        const int bit = in ? (tp[lo + k] >> q) & 1 : 0;
        int chunk;
        const int incl = de_block_scan_i(bit, wi, chunk);
        const int start = carry - chunk;
        const int tpc = start + incl;
        // prec = tp / max(tp + fp, eps) with fp = (k + 1) - tp: the sum is the integer k + 1
        const double prec = in ? (double)tpc / fmax((double)(k + 1), DBL_EPSILON) : 0.0;
        double cmax;
        const double e = fmax(de_block_rmax_d(prec, wd, cmax), env);
        if (in) {
            const double rec = (double)tpc / denom, prev = (double)(tpc - bit) / denom;
            if (rec != prev) acc += (rec - prev) * e;
        }
        env = fmax(env, cmax);
        carry = start;
    }
    const double ap = de_block_sum_d(acc, wd);
    if (t == 0) {
        double *o = table + ((size_t)q * NC + c) * 4;
        o[0] = ap;
        o[1] = n > 0 ? (double)total / denom : 0.0;
        o[2] = (double)n;
        o[3] = (npos > 0 || n > 0) ? 1.0 : 0.0;
    }
}

// ------------------------------------------------------------------------------------------------- host
extern "C" int d3_det_match(const float *pred_corners, const int *pred_cls, const float *scores, const float *pick, double conf_thresh,
                            const float *gt_corners, const float *gt_mask, const int *gt_cls, int B, int K, int G, int num_class,
                            const double *thresholds, int T, int *kept, int *cls_out, float *score_out, double *ovmax, int *jmax,
                            int *tp_bits, int *gt_count, int *status, void *stream) {
    D3_CLEAR();
    if (K > DE_MAX || G > DE_MAX || T < 1 || T > DE_MAXT || B < 1 || num_class > DE_MAXC) return D3_ERR_RANGE;
    if (K < 0 || G < 0 || num_class < 1 || !thresholds || !gt_count || !status) return D3_ERR_ARG;
    if (K > 0 && (!pred_corners || !pred_cls || !scores || !pick || !kept || !cls_out || !score_out || !ovmax || !jmax || !tp_bits))
        return D3_ERR_ARG;
    if (G > 0 && (!gt_corners || !gt_mask || !gt_cls)) return D3_ERR_ARG;
    DeThr thr;
    for (int q = 0; q < DE_MAXT; q++) thr.t[q] = q < T ? thresholds[q] : 0.0;
    de_match_kernel<<<B, DE_THREADS, 0, d3_stream(stream)>>>(pred_corners, pred_cls, scores, pick, conf_thresh, gt_corners, gt_mask, gt_cls,
                                                             K, G, num_class, thr, T, kept, cls_out, score_out, ovmax, jmax, tp_bits,
                                                             gt_count, status);
    D3_LAUNCH_CHECK();
    return 0;
}

extern "C" int d3_det_ap(const int *tp_sorted, const int *seg_offsets, const int *gt_count, int S, long long N, int num_class, int T,
                         double *table, void *stream) {
    D3_CLEAR();
    if (T < 1 || T > DE_MAXT || num_class > DE_MAXC || N > 0x7fffff00LL) return D3_ERR_RANGE;   // (the last pass's positions stay below 2^31)
    if (S < 0 || N < 0 || num_class < 1 || !seg_offsets || !table) return D3_ERR_ARG;
    if ((N > 0 && !tp_sorted) || (S > 0 && !gt_count)) return D3_ERR_ARG;
    de_ap_kernel<<<dim3(num_class, T), DE_THREADS, 0, d3_stream(stream)>>>(tp_sorted, seg_offsets, gt_count, S, (int)N, num_class, table);
    D3_LAUNCH_CHECK();
    return 0;
}
