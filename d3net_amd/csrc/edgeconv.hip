// edgeconv.hip -- the relation graph of the speaker head as native gfx950 code: edge-list construction for all scenes in
// one launch, and EdgeConv (gather -> 2-layer message MLP -> segmented add in edge order) forward + backward.
//
// Reference: model/graph_module.py:21-114 (`EdgeConv`: message = MLP([x_i, x_j - x_i]), aggr "add"), :252-324
// (`GraphModule.forward`: per scene, edges = row-major non-zeros of the valid-node adjacency via scipy COO, two EdgeConv
// layers, an edge layer + orientation head).  PyG convention: x_j = x[edge_index[0]] (the adjacency row,
// "source"), x_i = x[edge_index[1]] (the neighbour column, "target"), messages are summed at edge_index[1].
// The reference walks the scenes in a python loop (scipy on the host, ~30 launches per scene and layer); here
//   * gm_edges_kernel: one workgroup per scene builds, on the device and with fixed-size outputs (no host round trip):
//     the edge list in the reference's order (global node ids + the compacted ids that `edge_index` reports), the
//     incoming-edge lists per node (for a deterministic aggregation in edge order), the outgoing ranges, n_source /
//     n_target, and the gather tables that place messages / orientation predictions into the (B,K,L,.) outputs;
//   * the edges of ALL scenes form one padded matrix (B*K*L rows): one gather launch, two GEMMs on the fp32 matrix
//     cores (hgemm.hip; exact fp32), one aggregation launch per EdgeConv -- 4 launches instead of ~30 x B;
//   * backward: message gradient = d_msg + d_node[target]; the MLP backward as k-major GEMMs; the node gradient is the
//     sum over a node's incoming and outgoing lists in edge order: deterministic, no atomics.
// HBM/latency bound: B*K*L = 5,120 rows x 256 floats = 5 MB per layer.
#include "common.h"
#include <string.h>

#define GM_MAXK 256

// adj (B,K,K) 0/1, mask (B,K) -> see d3_graph_edges in include/d3hip.h
__global__ __launch_bounds__(1024) void gm_edges_kernel(const float *__restrict__ adj, const float *__restrict__ mask, int K, int L,
                                                       int *__restrict__ src, int *__restrict__ dst, float *__restrict__ eidx,
                                                       int *__restrict__ cnt, int *__restrict__ in_ptr, int *__restrict__ in_list,
                                                       int *__restrict__ out_start, int *__restrict__ out_cnt,
                                                       long long *__restrict__ feat_src, long long *__restrict__ pred_src) {
    extern __shared__ int sm[];
    int *valid = sm, *cidx = valid + K, *rowcnt = cidx + K, *rowstart = rowcnt + K, *incnt = rowstart + K, *instart = incnt + K;
    int *dsts = instart + K + 1;   // K*L slots: target column | source row << 16 of this scene's edges
    unsigned *colmask = (unsigned *)(dsts + K * L);   // per target column: bitmask of the rows that own an edge to it (8 words, K <= 256)
    __shared__ int tot[3];
    const int b = blockIdx.x, t = threadIdx.x, KL = K * L;
    const long long Emax_total = (long long)gridDim.x * KL;
    for (int k = t; k < K; k += blockDim.x) valid[k] = mask[(long long)b * K + k] == 1.f ? 1 : 0;
    for (int k = t; k < K * 8; k += blockDim.x) colmask[k] = 0u;
    __syncthreads();
    // one wave per adjacency row, lanes along the columns (a thread walking its own 1 KB row read it uncoalesced, twice)
    const int lane = t & 63, wave = t >> 6, nwv = blockDim.x >> 6;
    for (int r = wave; r < K; r += nwv) {
        int c = 0;
        if (valid[r]) {
            const float *row = adj + ((long long)b * K + r) * K;
            for (int j0 = 0; j0 < K; j0 += 64) {
                const int j = j0 + lane;
                c += __popcll(__ballot(j < K && valid[j < K ? j : 0] && row[j < K ? j : 0] == 1.f));
            }
        }
        if (lane == 0) rowcnt[r] = c < L ? c : L;     // an adjacency row holds exactly L ones (top-L of _query_locals)
    }
    __syncthreads();
    // exclusive prefix sums over the K <= 256 rows by one wave, four rows per lane (a single thread walking them: 12 us each)
    if (wave == 0) {
        int v4[4], c4[4], sv = 0, sc = 0, sn = 0;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int k = lane * 4 + q;
            v4[q] = k < K ? valid[k] : 0; c4[q] = k < K ? rowcnt[k] : 0;
            sv += v4[q]; sc += c4[q]; sn += c4[q] > 0 ? 1 : 0;
        }
        int pv = sv, pc = sc;
        for (int o = 1; o < 64; o <<= 1) {
            const int av = __shfl_up(pv, o), ac = __shfl_up(pc, o);
            if (lane >= o) { pv += av; pc += ac; }
        }
        for (int o = 32; o > 0; o >>= 1) sn += __shfl_xor(sn, o);
        int ev = pv - sv, ec = pc - sc;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int k = lane * 4 + q;
            if (k < K) { cidx[k] = ev; rowstart[k] = ec; }
            ev += v4[q]; ec += c4[q];
        }
        if (lane == 63) { tot[0] = pc; tot[1] = sn; tot[2] = pv; }
    }
    __syncthreads();
    const int E = tot[0], nsrc = tot[1], ntar = nsrc > 0 ? E / nsrc : 0, n = nsrc * ntar;
    if (t == 0) { cnt[b * 4 + 0] = E; cnt[b * 4 + 1] = nsrc; cnt[b * 4 + 2] = ntar; cnt[b * 4 + 3] = tot[2]; }
    for (int e = t; e < KL; e += blockDim.x) {     // padding
        src[(long long)b * KL + e] = -1; dst[(long long)b * KL + e] = -1; dsts[e] = -1;
        eidx[((long long)b * 2 + 0) * KL + e] = 0.f; eidx[((long long)b * 2 + 1) * KL + e] = 0.f;
        // edge_feature[b, r, k] <- message of edge e' = r * ntar + k (reference: message[:n].view(n_src, n_tar, .))
        const int r = e / L, k = e - r * L;
        feat_src[(long long)b * KL + e] = (r < nsrc && k < ntar) ? (long long)b * KL + r * ntar + k : Emax_total;
        // edge_preds[b, :n] <- predictions of edges 0..n-1, only when every edge is covered (E == n; the reference's
        // assignment raises otherwise and the exception is swallowed: graph_module.py:291-308)
        pred_src[(long long)b * KL + e] = (E == n && e < n) ? (long long)b * KL + e : Emax_total;
    }
    __syncthreads();
    for (int r = t; r < K; r += blockDim.x) { out_start[(long long)b * K + r] = rowstart[r]; out_cnt[(long long)b * K + r] = rowcnt[r]; }
    for (int r = wave; r < K; r += nwv) {
        if (!valid[r] || rowcnt[r] == 0) continue;          // wave-uniform
        const float *row = adj + ((long long)b * K + r) * K;
        int e0 = rowstart[r], taken = 0;
        const int want = rowcnt[r];
        for (int j0 = 0; j0 < K && taken < want; j0 += 64) {
            const int j = j0 + lane;
            const bool hit = j < K && valid[j < K ? j : 0] && row[j < K ? j : 0] == 1.f;
            const unsigned long long bal = __ballot(hit);
            const int pos = taken + (int)__popcll(bal & ((1ull << lane) - 1ull));   // column order == the serial walk's order
            if (hit && pos < want) {
                const int e = e0 + pos;
                src[(long long)b * KL + e] = b * K + r; dst[(long long)b * KL + e] = b * K + j; dsts[e] = j | (r << 16);
                atomicOr(&colmask[j * 8 + (r >> 5)], 1u << (r & 31));
                if (e < n) { eidx[((long long)b * 2 + 0) * KL + e] = (float)cidx[r]; eidx[((long long)b * 2 + 1) * KL + e] = (float)cidx[j]; }
            }
            taken += (int)__popcll(bal);
        }
    }
    __syncthreads();
    // incoming lists in edge order: a row owns at most one edge to a target, edges are ordered by row, so the rank of edge
    // (r -> v) among v's incoming edges is the number of rows below r in v's row mask (each thread walking all E edges per
    // target, twice, was most of this kernel's 130 us)
    for (int v = t; v < K; v += blockDim.x) {
        int c = 0;
#pragma unroll
        for (int w = 0; w < 8; w++) c += __popc(colmask[v * 8 + w]);
        incnt[v] = c;
    }
    __syncthreads();
    if (wave == 0) {
        int c4[4], sc = 0;
#pragma unroll
        for (int q = 0; q < 4; q++) { const int k = lane * 4 + q; c4[q] = k < K ? incnt[k] : 0; sc += c4[q]; }
        int pc = sc;
        for (int o = 1; o < 64; o <<= 1) { const int ac = __shfl_up(pc, o); if (lane >= o) pc += ac; }
        int ec = pc - sc;
#pragma unroll
        for (int q = 0; q < 4; q++) { const int k = lane * 4 + q; if (k < K) instart[k] = ec; ec += c4[q]; }
        if (lane == 63) instart[K] = pc;
    }
    __syncthreads();
    for (int v = t; v <= K; v += blockDim.x) in_ptr[(long long)b * (K + 1) + v] = instart[v];
    for (int e = t; e < E; e += blockDim.x) {
        const int v = dsts[e] & 0xffff, r = dsts[e] >> 16;
        int rank = __popc(colmask[v * 8 + (r >> 5)] & ((1u << (r & 31)) - 1u));
        for (int w = 0; w < (r >> 5); w++) rank += __popc(colmask[v * 8 + w]);
        in_list[(long long)b * KL + instart[v] + rank] = e;
    }
}

extern "C" int d3_graph_edges(const float *adj, const float *mask, int B, int K, int L, int *src, int *dst, float *edge_index,
                              int *cnt, int *in_ptr, int *in_list, int *out_start, int *out_cnt, long long *feat_src,
                              long long *pred_src, void *stream) {
    D3_CLEAR();
    if (B < 1 || K < 1 || K > GM_MAXK || L < 1) return D3_ERR_ARG;
    const size_t lds = (size_t)(6 * K + 1 + K * L + 8 * K) * 4;
    gm_edges_kernel<<<B, 1024, lds, d3_stream(stream)>>>(adj, mask, K, L, src, dst, edge_index, cnt, in_ptr, in_list, out_start, out_cnt,
                                                        feat_src, pred_src);
    D3_LAUNCH_CHECK();
    return 0;
}

// Ein[e] = [x_i | x_j - x_i], x_i = x[dst[e]], x_j = x[src[e]]; padded rows are zero
__global__ void ec_gather_kernel(const float *__restrict__ x, const int *__restrict__ src, const int *__restrict__ dst,
                                 float *__restrict__ Ein, long long Emax, int C) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;   // one float4 of a row half
    const int c4 = C >> 2;
    if (i >= Emax * c4) return;
    const long long e = i / c4;
    const int c = (int)(i - e * c4) * 4;
    const int s = src[e], d = dst[e];
    float4 xi = make_float4(0.f, 0.f, 0.f, 0.f), df = xi;
    if (s >= 0) {
        xi = *(const float4 *)(x + (long long)d * C + c);
        const float4 xj = *(const float4 *)(x + (long long)s * C + c);
        df = make_float4(xj.x - xi.x, xj.y - xi.y, xj.z - xi.z, xj.w - xi.w);
    }
    *(float4 *)(Ein + e * 2 * C + c) = xi;
    *(float4 *)(Ein + e * 2 * C + C + c) = df;
}

// node[b*K + v] = sum over the incoming edges of v, in edge order; also clears the message rows of padded edges
__global__ void ec_aggregate_kernel(float *__restrict__ msg, const int *__restrict__ src, const int *__restrict__ in_ptr,
                                    const int *__restrict__ in_list, float *__restrict__ node, int K, int KL, int C) {
    const int bv = blockIdx.x, b = bv / K, v = bv - b * K, c = threadIdx.x;
    if (c < C) {
        const int p0 = in_ptr[(long long)b * (K + 1) + v], p1 = in_ptr[(long long)b * (K + 1) + v + 1];
        float s = 0.f;
        for (int p = p0; p < p1; p++) s += msg[((long long)b * KL + in_list[(long long)b * KL + p]) * C + c];
        node[(long long)bv * C + c] = s;
    }
    // (K*L >= K rows per scene: workgroup (b, v) also clears padded message rows v, v + K, ...)
    for (int e = v; e < KL; e += K)
        if (src[(long long)b * KL + e] < 0 && c < C) msg[((long long)b * KL + e) * C + c] = 0.f;
}

static d3_gemm_seg ec_seg(const float *A, long long lda, const float *B, long long ldb, int K, int akm, int bkm) {
    d3_gemm_seg s;
    s.A = A; s.ia = nullptr; s.lda = lda; s.a_kmajor = akm; s.B = B; s.ldb = ldb; s.b_kmajor = bkm; s.K = K;
    return s;
}
static d3_gemm_prob ec_prob(int M, int N, float *C, long long ldc) {
    d3_gemm_prob p;
    memset(&p, 0, sizeof(p));
    p.M = M; p.N = N; p.C = C; p.ldc = ldc; p.nseg = 1;
    return p;
}

#define EC_KSPLIT 4
// the forward's workspace, kept for the backward: gathered edge inputs and the hidden layer
struct EcFwdWs { float *Ein, *hid; };
static void ec_fwd_layout(D3Carver &c, long long Emax, int Cin, int Cout, EcFwdWs &w) {
    w.Ein = c.take<float>((size_t)Emax * 2 * Cin);
    w.hid = c.take<float>((size_t)Emax * Cout);
}
struct EcBwdWs { float *dm, *dh, *dE, *wpart; void *cs; size_t cs_bytes; };
static void ec_bwd_layout(D3Carver &c, long long Emax, int Cin, int Cout, EcBwdWs &w) {
    w.dm = c.take<float>((size_t)Emax * Cout);
    w.dh = c.take<float>((size_t)Emax * Cout);
    w.dE = c.take<float>((size_t)Emax * 2 * Cin);
    w.cs_bytes = hg_colsum_ws_bytes(2, Cout);
    w.cs = c.take<char>(w.cs_bytes);
    w.wpart = c.take<float>((size_t)EC_KSPLIT * Cout * 2 * Cin);
}
extern "C" size_t d3_edgeconv_ws_bytes(int Emax, int Cin, int Cout) {
    D3Carver c(nullptr, 0);
    EcFwdWs w;
    ec_fwd_layout(c, Emax, Cin, Cout, w);
    return c.off;
}
extern "C" size_t d3_edgeconv_bwd_ws_bytes(int Emax, int Cin, int Cout) {
    D3Carver c(nullptr, 0);
    EcBwdWs w;
    ec_bwd_layout(c, Emax, Cin, Cout, w);
    return c.off;
}
// out = part[0] + part[1] + part[2] + part[3] (fixed order)
__global__ void ec_sum_parts_kernel(const float *__restrict__ part, long long n, float *__restrict__ out) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    float v = part[e];
#pragma unroll
    for (int q = 1; q < EC_KSPLIT; q++) v += part[q * n + e];
    out[e] = v;
}
// dW (Mo, No) = A^T B over the Emax edge rows (both operands k-major): the reduction is 10 k deep and the output 128 x 128 ..
// 128 x 256, i.e. 32-64 workgroups walking 10 k rows each (32 us); four row ranges as four problems of ONE launch, then a
// fixed-order sum of the four partial products
static int ec_wgrad_split(const float *A, int Mo, const float *Bm, int No, long long Emax, float *dW, float *part, hipStream_t s) {
    d3_gemm_prob p[EC_KSPLIT];
    const long long per = ((Emax + EC_KSPLIT - 1) / EC_KSPLIT + 3) / 4 * 4;
    int np = 0;
    for (int q = 0; q < EC_KSPLIT; q++) {
        const long long k0 = q * per, k1 = k0 + per < Emax ? k0 + per : Emax;
        if (k0 >= k1) break;
        p[np] = ec_prob(Mo, No, part + (long long)np * Mo * No, No);
        p[np].seg[0] = ec_seg(A + k0 * Mo, Mo, Bm + k0 * No, No, (int)(k1 - k0), 1, 1);
        np++;
    }
    int rc = hg_launch(p, np, s);
    if (rc) return rc;
    if (np < EC_KSPLIT) hipMemsetAsync(part + (long long)np * Mo * No, 0, (size_t)(EC_KSPLIT - np) * Mo * No * sizeof(float), s);
    const long long n = (long long)Mo * No;
    ec_sum_parts_kernel<<<(int)((n + 255) / 256), 256, 0, s>>>(part, n, dW);
    return 0;
}

// x (B*K, Cin); W0 (Cout, 2 Cin), b0; W2 (Cout, Cout), b2 -> node (B*K, Cout), msg (B*K*L, Cout).  ws keeps [Ein | hid].
extern "C" int d3_edgeconv_fwd(const float *x, const float *W0, const float *b0, const float *W2, const float *b2, const int *src,
                               const int *dst, const int *in_ptr, const int *in_list, int B, int K, int L, int Cin, int Cout,
                               float *node, float *msg, void *ws, size_t ws_bytes, void *stream) {
    D3_CLEAR();
    if ((Cin & 3) || Cout > 1024 || B < 1) return D3_ERR_ARG;
    const long long Emax = (long long)B * K * L;
    D3Carver cv(ws, ws_bytes);
    EcFwdWs f;
    ec_fwd_layout(cv, Emax, Cin, Cout, f);
    if (!cv.ok()) return D3_ERR_WORKSPACE;
    hipStream_t s = d3_stream(stream);
    float *Ein = f.Ein, *hid = f.hid;
    const long long tot = Emax * (Cin / 4);
    ec_gather_kernel<<<(int)((tot + 255) / 256), 256, 0, s>>>(x, src, dst, Ein, Emax, Cin);
    int rc;
    d3_gemm_prob p = ec_prob((int)Emax, Cout, hid, Cout);
    p.seg[0] = ec_seg(Ein, 2 * Cin, W0, 2 * Cin, 2 * Cin, 0, 0); p.bias = b0; p.relu = 1;
    if ((rc = hg_launch(&p, 1, s))) return rc;
    d3_gemm_prob p2 = ec_prob((int)Emax, Cout, msg, Cout);
    p2.seg[0] = ec_seg(hid, Cout, W2, Cout, Cout, 0, 0); p2.bias = b2;
    if ((rc = hg_launch(&p2, 1, s))) return rc;
    ec_aggregate_kernel<<<B * K, ((Cout + 63) / 64) * 64, 0, s>>>(msg, src, in_ptr, in_list, node, K, K * L, Cout);
    D3_LAUNCH_CHECK();
    return 0;
}

// dm[e] = d_msg[e] + d_node[dst[e]] for real edges, 0 for padding
__global__ void ec_bwd_dm_kernel(const float *__restrict__ d_msg, const float *__restrict__ d_node, const int *__restrict__ dst,
                                 float *__restrict__ dm, long long Emax, int C) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Emax * C) return;
    const long long e = i / C;
    const int c = (int)(i - e * C), d = dst[e];
    dm[i] = d >= 0 ? (d_msg ? d_msg[i] : 0.f) + (d_node ? d_node[(long long)d * C + c] : 0.f) : 0.f;
}
__global__ void ec_relu_mask_kernel(float *__restrict__ d, const float *__restrict__ h, long long n) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n && h[e] <= 0.f) d[e] = 0.f;
}
// dx[b*K + v] = sum_{incoming e} (dE[e, :C] - dE[e, C:]) + sum_{outgoing e} dE[e, C:]   (edge order; no atomics)
__global__ void ec_bwd_dx_kernel(const float *__restrict__ dE, const int *__restrict__ in_ptr, const int *__restrict__ in_list,
                                 const int *__restrict__ out_start, const int *__restrict__ out_cnt, float *__restrict__ dx, int K,
                                 int KL, int C) {
    const int bv = blockIdx.x, b = bv / K, v = bv - b * K, c = threadIdx.x;
    if (c >= C) return;
    float s = 0.f;
    const int p0 = in_ptr[(long long)b * (K + 1) + v], p1 = in_ptr[(long long)b * (K + 1) + v + 1];
    for (int p = p0; p < p1; p++) {
        const float *row = dE + ((long long)b * KL + in_list[(long long)b * KL + p]) * 2 * C;
        s += row[c] - row[C + c];
    }
    const int o0 = out_start[bv], o1 = o0 + out_cnt[bv];
    for (int e = o0; e < o1; e++) s += dE[((long long)b * KL + e) * 2 * C + C + c];
    dx[(long long)bv * C + c] = s;
}

// d_node (B*K, Cout) / d_msg (B*K*L, Cout) (either may be NULL) -> dx (B*K, Cin), dW0, db0, dW2, db2 (written).
// ws: the forward's workspace ([Ein | hid]); ws2: d3_edgeconv_bwd_ws_bytes() of scratch.
extern "C" int d3_edgeconv_bwd(const float *W0, const float *W2, const int *src, const int *dst, const int *in_ptr, const int *in_list,
                               const int *out_start, const int *out_cnt, int B, int K, int L, int Cin, int Cout, const float *d_node,
                               const float *d_msg, const void *ws, float *dx, float *dW0, float *db0, float *dW2, float *db2,
                               void *ws2, size_t ws2_bytes, void *stream) {
    D3_CLEAR();
    if ((Cin & 3) || Cin > 1024 || B < 1) return D3_ERR_ARG;
    const long long Emax = (long long)B * K * L;
    D3Carver cv(ws2, ws2_bytes), cf(const_cast<void *>(ws), SIZE_MAX);      // (the forward checked its own size)
    EcBwdWs w;
    EcFwdWs f;
    ec_bwd_layout(cv, Emax, Cin, Cout, w);
    ec_fwd_layout(cf, Emax, Cin, Cout, f);
    if (!cv.ok() || !cf.ok()) return D3_ERR_WORKSPACE;
    hipStream_t s = d3_stream(stream);
    const float *Ein = f.Ein, *hid = f.hid;
    float *dm = w.dm, *dh = w.dh, *dE = w.dE, *wpart = w.wpart;
    (void)src;
    const long long tot = Emax * Cout;
    ec_bwd_dm_kernel<<<(int)((tot + 255) / 256), 256, 0, s>>>(d_msg, d_node, dst, dm, Emax, Cout);
    int rc;
    {   // dh = dm W2 (relu-masked); dW2 = dm^T hid; db2 = colsum(dm)
        d3_gemm_prob p[2];
        p[0] = ec_prob((int)Emax, Cout, dh, Cout); p[0].seg[0] = ec_seg(dm, Cout, W2, Cout, Cout, 0, 1);
        if ((rc = hg_launch(&p[0], 1, s))) return rc;
        if ((rc = ec_wgrad_split(dm, Cout, hid, Cout, Emax, dW2, wpart, s))) return rc;
        ec_relu_mask_kernel<<<(int)((tot + 255) / 256), 256, 0, s>>>(dh, hid, tot);
    }
    {   // dE = dh W0; dW0 = dh^T Ein; db0 = colsum(dh)
        d3_gemm_prob p[2];
        p[0] = ec_prob((int)Emax, 2 * Cin, dE, 2 * Cin); p[0].seg[0] = ec_seg(dh, Cout, W0, 2 * Cin, Cout, 0, 1);
        if ((rc = hg_launch(&p[0], 1, s))) return rc;
        if ((rc = ec_wgrad_split(dh, Cout, Ein, 2 * Cin, Emax, dW0, wpart, s))) return rc;
        // both bias gradients in one two-stage column sum (dm is not modified after the first block)
        const float *cx[2] = {dm, dh}; const long long cl[2] = {Cout, Cout}; const int cr[2] = {(int)Emax, (int)Emax}, cc[2] = {Cout, Cout};
        float *co[2] = {db2, db0};
        if ((rc = hg_colsum_multi(cx, cl, cr, cc, co, nullptr, 2, w.cs, w.cs_bytes, s))) return rc;
    }
    ec_bwd_dx_kernel<<<B * K, ((Cin + 63) / 64) * 64, 0, s>>>(dE, in_ptr, in_list, out_start, out_cnt, dx, K, K * L, Cin);
    D3_LAUNCH_CHECK();
    return 0;
}
