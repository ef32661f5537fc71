/*
 * d3hip.h -- C ABI of libd3hip.so, the MI355X (gfx950) implementation of D3Net's
 * PointGroup hot path.  Plain pointers and sizes only; no torch types.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless its name ends in `_host`;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); all work is
 *     stream-ordered on it;
 *   - return value: 0 = success, >0 = hipError_t, <0 = D3_ERR_* below;
 *   - no hidden allocation: ops that need scratch take `ws`/`ws_bytes` and have a
 *     `*_ws_bytes()` query (the one exception: the network object of d3_net_create owns two
 *     small grow-only job tables, allocated lazily inside d3_net_forward / d3_net_backward and
 *     freed by d3_net_destroy -- see there); data-dependent output sizes use a two-phase
 *     `*_count` (writes sizes to `*_host`, synchronises the stream) / `*_fill` pair so
 *     the caller allocates, exactly as the reference's python layer does
 *     (reference: lib/pointgroup_ops/functions/pointgroup_ops.py).
 *
 * Each entry point cites the reference interface it replaces.  Paths are relative to
 * the reference root; `PG_OP.x` is the pybind symbol of
 * lib/pointgroup_ops/src/pointgroup_ops_api.cpp:6-24.
 */
#ifndef D3HIP_H
#define D3HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define D3_ERR_WORKSPACE (-1) /* ws_bytes too small                          */
#define D3_ERR_RANGE     (-2) /* coordinate / batch index outside key range  */
#define D3_ERR_ARG       (-3) /* unsupported argument (mode, channel count)  */
#define D3_ERR_OVERFLOW  (-4) /* hash table / queue overflow                 */

int d3_version(void);
const char *d3_arch(void); /* "gfx950" */

/* ---- segment ops ------------------------------------------------------------------ */
/* PG_OP.sec_mean / sec_min / sec_max  (lib/pointgroup_ops/src/sec_mean/sec_mean.cu:12-86) */
int d3_sec_mean(const float *inp, const int *offsets, float *out, int nProposal, int C, void *stream);
int d3_sec_min(const float *inp, const int *offsets, float *out, int nProposal, int C, void *stream);
int d3_sec_max(const float *inp, const int *offsets, float *out, int nProposal, int C, void *stream);
/* Index plumbing around the two clusterings of PointGroup.forward (model/pointgroup.py:288-316; csrc/clusterprep.hip):
 *   select: the object points' batch ids, coordinates, shifted coordinates (coords + offsets) and semantic ids, compacted by
 *           object_idxs (n int64 scene point ids) -- four gathers, a cast and an add of the reference in one pass;
 *   merge : the (cluster, compact point) pairs of both clusterings mapped back to scene point ids, their batch ids, the second
 *           set's cluster ids / offsets shifted behind the first's, concatenated as the reference does (out_bid has S1+S2-1
 *           entries: the reference drops the first pair of the second set, :316). */
int d3_cluster_select(const float *locs, const float *pt_offsets, const int64_t *semantic_preds, const int *batch_idxs,
                      const int64_t *object_idxs, int n, int *batch_out, float *coords_out, float *shifted_out, int *semantic_out,
                      void *stream);
/* select + the batch offsets of the object points (model/pointgroup.py:110-122 get_batch_offsets, :296): batch_offsets_out[b] = object
 * points with a batch id below b, b = 0..batch_size, read off the boundaries of the (sorted) id column in the same pass; n >= 1 */
int d3_cluster_select2(const float *locs, const float *pt_offsets, const int64_t *semantic_preds, const int *batch_idxs,
                       const int64_t *object_idxs, int n, int batch_size, int *batch_out, float *coords_out, float *shifted_out,
                       int *semantic_out, int *batch_offsets_out, void *stream);
int d3_cluster_merge(const int *idx1, int S1, const int *off1, int P1, const int *idx2, int S2, const int *off2, int P2,
                     const int64_t *object_idxs, const int *batch_idxs, int *out_idx, int *out_off, int *out_bid, void *stream);
/* Per-proposal bookkeeping between the score head and the proposal selection (model/pointgroup.py:338-372): npoint (P) = points
 * per proposal, mask (P) bytes = sig > score_thr && npoint > npoint_thr, batch_id (P) = batch_id_all[min(offsets[p],
 * n_batch_id - 1)] (the reference's one-element-short batch-id vector), crop (P,9) = [center | size | 0 | semantic_preds of the
 * proposal's first point | sig].  sig = sigmoid of the proposal scores. */
int d3_proposal_prepare(const float *sig, const int *offsets, const int *batch_id_all, int n_batch_id, const int *proposals_idx,
                        const int64_t *semantic_preds, const float *center, const float *size, float score_thr, float npoint_thr,
                        int P, float *npoint, unsigned char *mask, int *batch_id, float *crop, void *stream);
/* The per-point passes of PointGroup.clusters_voxelization (model/pointgroup.py:125-178) over the S (cluster, point) pairs of
 * clusters_idx (S,2) without the gathered / shifted / scaled (S,3) temporaries of the library-op form:
 *   coords_stats: mean (P,3) = sec_mean of the clusters' point coordinates (same serial x/count chain, bit-exact), cmin / cmax
 *                 (P,3) = their per-cluster extrema (raw coordinates: min(x - m) == min(x) - m under monotone rounding);
 *   transform   : out (S,4) int64 = [cluster, trunc((coords[point] - mean[cluster]) * scale[cluster] + offset[cluster])],
 *                 each fp32 operation rounded separately (:141-166). */
int d3_cluster_coords_stats(const float *coords, const int *clusters_idx, const int *offsets, float *mean, float *cmin, float *cmax,
                            int nProposal, void *stream);
/* the same with S = number of (cluster, point) pairs and d3_cluster_coords_stats_ws_bytes(S) bytes of scratch: the addends of the
 * clusters' mean chains (coords / count, IEEE) are gathered by a chip-wide pass first and the serial chains stream them
 * (bit-identical results; 258 -> ~130 us for the 4-scene batch, whose 33 k-point floors set the launch time). */
size_t d3_cluster_coords_stats_ws_bytes(long long S);
int d3_cluster_coords_stats2(const float *coords, const int *clusters_idx, const int *offsets, long long S, float *mean, float *cmin,
                             float *cmax, int nProposal, void *ws, size_t ws_bytes, void *stream);
int d3_cluster_transform(const float *coords, const int *clusters_idx, const float *mean, const float *scale, const float *offset,
                         long long *out, long long S, void *stream);
/* The per-cluster arithmetic between the two (model/pointgroup.py:146-165): size = cmax - cmin, center = (cmax + cmin) / 2 + mean
 * (cmin / cmax relative to the mean), cscale = min(1 / max_k((cmax - cmin) / fullscale) - 0.01, scale_cap), and the placement
 * offset = -cmin * cscale + clamp(fullscale - range - 0.001, min 0) * r0 + clamp(fullscale - range + 0.001, max 0) * r1 with
 * range = (cmax - cmin) * cscale.  rand6 = HOST pointer to the six floats [r0 | r1] (the reference's two `torch.rand(3)` draws,
 * :161), passed as kernel arguments.  Bit-equal to the ~30 elementwise library launches it replaces. */
int d3_cluster_norm_params(const float *mean, const float *raw_min, const float *raw_max, int P, float fullscale, float scale_cap,
                           const float *rand6, float *size, float *center, float *cscale, float *offset, void *stream);
/* PG_OP.roipool_fp / roipool_bp  (src/roipool/roipool.cu:12-57) */
int d3_roipool_fp(const float *feats, const int *proposals_offset, float *output_feats, int *output_maxidx,
                  int nProposal, int C, void *stream);
int d3_roipool_bp(float *d_feats, const int *proposals_offset, const int *output_maxidx,
                  const float *d_output_feats, int nProposal, int C, void *stream);
/* PG_OP.get_iou  (src/get_iou/get_iou.cu:12-38) */
int d3_get_iou(const int *proposals_idx, const int *proposals_offset, const int64_t *instance_labels,
               const int *instance_pointnum, float *proposals_iou, int nInstance, int nProposal, void *stream);

/* ---- voxelize --------------------------------------------------------------------- */
/* PG_OP.voxelize_fp / voxelize_bp / point_recover_fp / point_recover_bp
 * (src/voxelize/voxelize.cu:10-53, src/voxelize/voxelize.cpp:155-202).  Outputs are
 * accumulated into (the caller zero-fills them, as functions/pointgroup_ops.py:57,70 do). */
int d3_voxelize_fp(const float *feats, float *output_feats, const int *output_map, int mode, int nActive,
                   int maxActive, int nPlane, void *stream);
/* voxelize_fp of the column concatenation [feats_a | feats_b] without materialising it; writes (does not accumulate into)
 * output_feats (M, Ca+Cb): PointGroup.feed's `voxelization(cat(feats, locs), v2p_map)` (model/pointgroup.py:468-471) */
int d3_voxelize_fp2(const float *feats_a, int Ca, const float *feats_b, int Cb, float *output_feats, const int *output_map, int mode,
                    int nActive, int maxActive, void *stream);
int d3_voxelize_bp(const float *d_output_feats, float *d_feats, const int *output_map, int mode, int nActive,
                   int maxActive, int nPlane, void *stream);
int d3_point_recover_fp(const float *feats, float *output_feats, const int *idx_map, int nActive,
                        int maxActive, int nPlane, void *stream);
int d3_point_recover_bp(const float *d_output_feats, float *d_feats, const int *idx_map, int nActive,
                        int maxActive, int nPlane, void *stream);

/* PG_OP.voxelize_idx  (src/voxelize/voxelize.cpp:10-152), on the device, two-phase.
 * coords (n, ncols) int64, ncols in {3,4} (column 0 = batch index when 4).
 * count: fills input_map (n) and writes M and maxActive to the host.
 * fill : writes output_coords (M, ncols) int64 and output_map (M, maxActive+1) int32
 *        (voxels in first-occurrence order, point ids ascending, zero padded).
 * Key range: batch in [0, 2^19), x/y/z in [-2^14, 2^14) after the reference's
 * int64->int32 truncation, else D3_ERR_RANGE. */
size_t d3_voxelize_idx_ws_bytes(int n);
int d3_voxelize_idx_count(const int64_t *coords, int n, int ncols, int mode, int *input_map, void *ws,
                          size_t ws_bytes, int *M_host, int *maxActive_host, void *stream);
int d3_voxelize_idx_fill(const int64_t *coords, int n, int ncols, int mode, const int *input_map, void *ws,
                         size_t ws_bytes, int64_t *output_coords, int *output_map, int M, int maxActive,
                         void *stream);

/* ---- ball query + clustering -------------------------------------------------------- */
/* PG_OP.ballquery_batch_p  (src/bfs_cluster/bfs_cluster.cu:15-90), two-phase, no retry loop.
 * count: per-point hit count (strict d2<r2, capped at 1000, same batch item only) ->
 *        start_len (n,2) with start = exclusive prefix sum of len in point order (the
 *        reference's starts come from atomicAdd and are scheduling dependent);
 *        *nActive_host = total.
 * fill : neighbour indices in ascending order; entries at positions >= idx_capacity are
 *        dropped exactly as the reference truncates at n*meanActive (bfs_cluster.cu:51-59). */
size_t d3_ballquery_ws_bytes(int n);
/* with a workspace of this size (adds n*1000 ints) the count phase also stashes the hits and the fill phase only
 * compacts them: one neighbour search instead of two */
size_t d3_ballquery_ws_bytes_single_pass(int n);
int d3_ballquery_count(const float *xyz, const int *batch_idxs, const int *batch_offsets, int n, float radius,
                       int *start_len, void *ws, size_t ws_bytes, int *nActive_host, void *stream);
int d3_ballquery_fill(const float *xyz, const int *batch_idxs, const int *batch_offsets, int n, float radius,
                      const int *start_len, const void *ws, size_t ws_bytes, int *idx, long long idx_capacity,
                      void *stream);
/* Padded, sync-free ball query: idx_padded holds n slots of d3_ballquery_cap() entries and start_len[q] = (s * cap, len)
 * with s = q, or -- when every point in the 27 search cells around q's cell lies within one ball (a collapsed instance:
 * all those queries have the same list) -- the smallest point index of q's cell, whose slot then holds the one shared copy.
 * Same neighbours in the same order as d3_ballquery_count/fill (uniform cell grid instead of the ordered scan:
 * csrc/ballquery.hip); no nActive, no host round trip.  Valid input of d3_bfs_cluster_* (they only index idx[start + e]).
 * ws: d3_ballquery_ws_bytes(n).  Replaces the same reference call as d3_ballquery_count (bfs_cluster.cu:13-63). */
int d3_ballquery_cap(void);
int d3_ballquery_padded(const float *xyz, const int *batch_idxs, const int *batch_offsets, int n, float radius,
                        int *start_len, void *ws, size_t ws_bytes, int *idx_padded, void *stream);

/* PG_OP.bfs_cluster  (src/bfs_cluster/bfs_cluster.cpp:28-112), on the device (csrc/cluster.hip).
 * count: connected components (same semantic label, directed ball-query lists, seeds in ascending index) with
 *        size >= threshold -> sumNPoint, nCluster.  Union-find over the mutual edges, then label pushes over all edges
 *        until nothing changes: one pair of sweeps unless capped lists form a chain.
 * fill : cluster_idxs (sumNPoint,2) = (cluster_id, point_idx) in the reference's FIFO-BFS visitation order,
 *        cluster_offsets (nCluster+1).  The level loop runs in "record form": a parallel pre-pass rewrites the lists of the
 *        kept clusters as (node, dense id, list start, list length) records and one workgroup per cluster replays the BFS
 *        with visited bits, frontier and first-discoverer arbitration in LDS -- one global round trip per batch of 3072
 *        edges.  A cluster that is its seed's own list is written without a level loop; one of more than 262,144 points
 *        (the LDS bitmap) by a level loop on the lists themselves.
 * ws  : d3_bfs_cluster_ws_bytes(n) bytes;  erec: d3_bfs_cluster_erec_bytes(nActive) bytes of scratch for the records,
 *       nActive = length of ball_query_idxs.
 * Outputs at their upper bounds: cluster_idxs cap_points x 2 ints, cap_points >= sumNPoint -- n always suffices;
 * cluster_offsets cap_clusters + 1 ints -- n / max(threshold, 1) + 1 suffices.  D3_ERR_WORKSPACE when ws, erec or a bound
 * is too small.
 * flags: D3_BFS_ASCENDING -- the caller guarantees that every neighbour list is in ascending index order
 *        (ballquery_batch_p's order, src/bfs_cluster/bfs_cluster.cu:27-47): the label push then skips, per node, the
 *        prefix of neighbours whose label cannot change (two 64-way probes).  Same results. */
#define D3_BFS_ASCENDING 1
size_t d3_bfs_cluster_ws_bytes(int n);
size_t d3_bfs_cluster_erec_bytes(long long nActive);
/* `begin` enqueues everything on `stream` -- the first pair of sweeps with the sizes behind them, the copy of the counts to
 * the host and an event, then the whole fill with its sizes read on the device (upper-bound grids: the speculative fill) --
 * and returns without waiting.  `end` waits for the event, not for the stream, returns the sizes, and finishes the rare
 * cases: more than 2048 kept clusters, a cluster beyond the LDS bitmap, more sweeps (the fill then runs again over the
 * speculative one).  One host thread keeps several clusterings in flight on different streams: begin, begin, end, end.
 * Without the speculative form (D3_CL_SPEC=0, cap_points < n) `begin` waits for the counts itself and `end` only hands the
 * sizes over.
 * Contract: `begin` returns 0 and a ticket, or a non-zero status and *ticket == NULL with nothing left allocated -- `end`
 * is then not called.  A ticket is consumed by exactly one `end`, whatever that returns; the buffers handed to `begin`
 * must stay alive until then. */
int d3_bfs_cluster_begin(const int *semantic_label, const int *ball_query_idxs, const int *start_len, int n, int threshold,
                         void *ws, size_t ws_bytes, void *erec, size_t erec_bytes, long long nActive, int flags,
                         int *cluster_idxs, long long cap_points, int *cluster_offsets, long long cap_clusters,
                         void **ticket, void *stream);
int d3_bfs_cluster_end(void *ticket, int *sumNPoint_host, int *nCluster_host);
/* `begin` + `end` as one call; both sizes are 0 when it fails.  Replaces the pair bfs_cluster.cpp:28-112 is called through
 * (functions/pointgroup_ops.py:203-231) without a return to the caller between the phases (a Python caller re-acquires
 * its interpreter lock there: idle device time). */
int d3_bfs_cluster_run(const int *semantic_label, const int *ball_query_idxs, const int *start_len, int n, int threshold,
                       void *ws, size_t ws_bytes, void *erec, size_t erec_bytes, long long nActive, int flags,
                       int *cluster_idxs, long long cap_points, int *cluster_offsets, long long cap_clusters,
                       int *sumNPoint_host, int *nCluster_host, void *stream);

/* ---- sparse 3-D convolution (MinkowskiEngine subset) ---------------------------------- */
/* Coordinates are (M,4) int32 rows [batch, x, y, z] (ME.SparseTensor(coordinates=...),
 * reference: model/pointgroup.py:176,268).  Key range as for voxelize_idx.
 * A kernel map is a dense table tbl (Mout, K) int32: tbl[u][k] = input row feeding output row u
 * through kernel offset k, or -1.  k = ox + Kd*oy + Kd*Kd*oz (x fastest).
 *
 * d3_kmap_k3      : K=27 neighbour table of a kernel-3 stride-1 conv at tensor stride ts
 *                   (MinkowskiConvolution(kernel_size=3): model/common.py:38,41,66; model/pointgroup.py:70).
 * d3_kmap_down_*  : kernel-2 stride-2 maps (MinkowskiConvolution(kernel_size=2, stride=2) and its
 *                   MinkowskiConvolutionTranspose: model/common.py:90,98): output coordinates
 *                   floor(c/(2ts))*2ts in first-occurrence order, parent/kidx per input row,
 *                   child (Mout,8) for the strided conv, up (M,8) for the transposed conv. */
size_t d3_coordmap_ws_bytes(int M);
int d3_kmap_k3(const int *coords, int M, int ts, void *ws, size_t ws_bytes, int *nbr, void *stream);
/* 16-bit form of a d3_kmap_k3 table: nbr16 (M*27 + 2 int16) = nbr - row, -32768 = absent; *ok16 (device int) = 1 when every
 * delta fits, else 0 (the consumers then read the dense table).  MinkowskiEngine keeps one int32 pair list per kernel map
 * (no counterpart); the executor hands both forms to the convolutions of a level (d3_net_set_k3_16). */
int d3_kmap_k3_pack16(const int *nbr, int M, void *nbr16, int *ok16, void *stream);
/* d3_kmap_k3 that writes the 16-bit form and its flag in the same pass (what the coordinate manager calls for big levels) */
int d3_kmap_k3_16(const int *coords, int M, int ts, void *ws, size_t ws_bytes, int *nbr, void *nbr16, int *ok16, void *stream);
/* LANE TABLE of a d3_kmap_k3 table (round 6; read by d3_spconv_fwd3*): per 16-row tile 64 lanes x 8 uint16 -- lane (r = lane & 15,
 * g = lane >> 4), slot q < 7 = nbr[tile*16 + r][4q + g] - tile*16 + 32768 (0xFFFF: absent; offset 27 and slot 7 are pads): the
 * order in which a wave of the convolution kernel consumes the map, one 16-byte load per lane and tile (round 6b: the tile's
 * LIVE offsets first, listed in a 32-byte record per tile behind the lane tables: csrc/spconv3.hip).  d3_kmap_k3_q16_bytes(M)
 * bytes; *okq (device int) = 1 when every entry fits, else 0 (the consumers then read the dense table). */
size_t d3_kmap_k3_q16_bytes(int M);
int d3_kmap_k3_packq(const int *nbr, int M, void *tq, int *okq, void *stream);
int d3_kmap_down_count(const int *coords, int M, int ts, void *ws, size_t ws_bytes, int *parent, int *kidx,
                       int *Mout_host, void *stream);
int d3_kmap_down_fill(const int *coords, int M, int ts, void *ws, size_t ws_bytes, const int *parent,
                      const int *kidx, int *out_coords, int *child, int *up, int Mout, void *stream);

/* All stride-2 levels with ONE host round trip (d3_kmap_down_count costs one per level): the coordinate pyramid is
 * built with device-side row counts, rows_host[l] returns them all, and the tables are then filled with exact sizes by
 * d3_kmap_k3 / d3_kmap_down_fill2 without further synchronisation.  coords_out: (nlevels-1, M0, 4); parent / kidx / flag:
 * (nlevels-1, M0) (level l at [l*M0], rows of level l); rows_dev: nlevels ints.  ws >= d3_coordmap_ws_bytes(M0). */
int d3_kmap_pyramid(const int *coords0, int M0, int nlevels, void *ws, size_t ws_bytes, int *coords_out, int *parent,
                    int *kidx, int *flag, int *rows_dev, int *rows_host, void *stream);
/* The same with the host round trip split in two: _begin enqueues the level kernels and the copy of the row counts and returns
 * a ticket; _end waits for that copy only (not for work enqueued on the stream in between -- the caller puts independent
 * device work there: PointGroup.feed the input voxelisation) and returns rows_host.  *ticket == NULL when M0 == 0. */
int d3_kmap_pyramid_begin(const int *coords0, int M0, int nlevels, void *ws, size_t ws_bytes, int *coords_out, int *parent,
                          int *kidx, int *flag, int *rows_dev, void **ticket, void *stream);
int d3_kmap_pyramid_end(void *ticket, int *rows_host, int nlevels);
int d3_kmap_down_fill2(int M, int Mout, const int *parent, const int *kidx, int *child, int *up, void *stream);

/* Gather-GEMM convolution  out[u,:] = sum_k x[tbl[u,k],:] @ Wk   (tbl == NULL: identity map, K = 1).
 * flags: D3_CONV_FLIPK  -> Wk = W[K-1-k]      (data gradient of a kernel-3 conv)
 *        D3_CONV_TRANSW -> W is laid out (K, Cout, Cin) and used transposed (data gradients)
 *        D3_CONV_EXACT  -> fp32 FMA kernel instead of the bf16-MFMA kernel (fp32 accumulate in both)
 * x (Min,Cin) f32 (Min = rows of x, used for bounds / traffic accounting), W (K,Cin,Cout) f32 [or (K,Cout,Cin) with TRANSW], out (Mout,Cout) f32.
 * MFMA path needs Cin % 2 == 0 and Cout <= 224, else D3_ERR_ARG. */
#define D3_CONV_FLIPK 1
#define D3_CONV_TRANSW 2
#define D3_CONV_EXACT 4
#define D3_CONV_XSTAT 8
#define D3_CONV_ACCUM 16
#define D3_CONV_XBF16 32   /* x is stored as bf16 (ushort), Cin % 8 == 0; not with D3_CONV_EXACT */
#define D3_CONV_DYBF16 64  /* dy is stored as bf16 (d3_spconv_wgrad2 only) */
#define D3_CONV_OUTBF16 512 /* d3_spconv_fwd2*: `out` is stored as bf16 (ushort, ldo in elements); not with D3_CONV_ACCUM, a residual or
                            * D3_CONV_F32.  BatchNorm partials are taken from the unrounded values. */
#define D3_CONV_BNXBF16 1024 /* d3_spconv_fwd2_bnbwd* / d3_spconv_fwd3_bnbwd: bnx (the BatchNorm input re-read by the epilogue) is stored as bf16 */
#define D3_CONV_F32 256    /* d3_spconv_pack / d3_spconv_fwd2* / d3_spconv_wgrad2: the REFERENCE'S PRECISION on the matrix cores -- fp32
                            * operands (x, dy fp32; weights packed as fp32 fragments: d3_spconv_pack_bytes_ex), exact fp32 products on
                            * v_mfma_f32_16x16x4_f32, fp32 accumulation.  Not with D3_CONV_XBF16 / D3_CONV_DYBF16. */
#define D3_CONV_NOREDUCE 128 /* d3_spconv_wgrad2: leave the row-split partials in ws (d3_spconv_wgrad2_splits() of them, or one
                              * when accumulating); the caller sums them (the executor does it for all layers in one launch) */
int d3_spconv_fwd(const float *x, const int *tbl, const float *W, float *out, int Min, int Mout, int K, int Cin,
                  int Cout, int flags, void *stream);
/* Weight gradient  dW[k] = sum_u x[tbl[u,k],:]^T dy[u,:]   (dW (K,Cin,Cout) f32; cleared here unless
 * D3_CONV_ACCUM is set, then accumulated into).
 * With D3_CONV_XSTAT, tbl is the TRANSPOSED map (one row per x row, entries = dy rows):
 * dW[k'] += sum_v x[v,:]^T dy[tbl[v,k],:], k' = K-1-k with D3_CONV_FLIPK else k -- same result, but the
 * wide operand (x) is read contiguously and the narrow one gathered. */
int d3_spconv_wgrad(const float *x, const int *tbl, const float *dy, float *dW, int Min, int Mout, int K, int Cin,
                    int Cout, int flags, void *stream);

/* Second-generation MFMA kernels (csrc/spconv2.hip; weight gradients: csrc/wgrad.hip): wave-autonomous register gather,
 * v_mfma_f32_16x16x32_bf16, weights pre-packed into bf16 MFMA fragment order.  Same contraction and flags as d3_spconv_fwd / d3_spconv_wgrad
 * (D3_CONV_FLIPK / D3_CONV_TRANSW are applied by the pack step); Cin % 8 == 0 (wgrad2: Cout % 8 == 0 too).
 *   pack   : W (K,Cin,Cout) f32 [(K,Cout,Cin) with TRANSW] -> Wp, d3_spconv_pack_bytes() bytes.
 *   fwd2   : out[u, 0:Cout] (row stride ldo) = sum_k x[tbl[u,k]] @ Wk (+ res[u] (row stride ldr)) (+ out with
 *            D3_CONV_ACCUM); x has row stride ldx (fp32, or bf16 with D3_CONV_XBF16).  part != NULL: per-workgroup
 *            per-channel sum / sum of squares of the stored values, [d3_spconv_fwd2_nparts()][2][ceil16(Cout)] f32
 *            -- the batch statistics of the following MinkowskiBatchNorm (consumed by d3_bn_finalize_parts).
 *   wgrad2 : dW (K,CinW,Cout) f32 (CinW <= Cin: x may carry zero-padded channels) written (accumulated into with D3_CONV_ACCUM); ws >= d3_spconv_wgrad2_ws_bytes()
 *            holds row-split partials that are summed in fixed order (deterministic, no atomics). */
size_t d3_spconv_pack_bytes(int K, int Cin, int Cout);
size_t d3_spconv_pack_bytes_ex(int K, int Cin, int Cout, int flags);   /* flags & D3_CONV_F32: fp32 fragments (2x) */
int d3_spconv_pack(const float *W, void *Wp, int K, int Cin, int Cout, int flags, void *stream);
int d3_spconv_fwd2_nparts(int Mout, int K, int Cin, int Cout);
int d3_spconv_fwd2_nparts_ex(int Mout, int K, int Cin, int Cout, int flags);   /* flags & D3_CONV_F32: that call's partial rows */
/* both are UPPER BOUNDS since round 6 (the kernel that serves a K = 27 shape depends on the tables the call is handed);
 * d3_spconv_last_nparts(): the partial rows the last d3_spconv_fwd2* / d3_spconv_fwd3* call of this thread through THIS interface
 * wrote (0 after a call with Mout <= 0 or one that failed before its launch); the U-Net executor's own convolutions do not touch it */
int d3_spconv_last_nparts(void);
/* which kernel fwd2 runs for a shape (tests assert the variant they mean to cover): out[6] = {split (1 = the few-row
 * spconv_fwd2_split_kernel, 0 = the persistent wave-per-tile spconv_fwd2_kernel), waves per workgroup, grid.x,
 * weights resident in LDS, column tiles per workgroup, grid.y} */
int d3_spconv_fwd2_plan(int Mout, int K, int Cin, int Cout, int *out6);
int d3_spconv_fwd2(const void *x, int ldx, const int *tbl, const void *Wp, float *out, int ldo, const float *res,
                   int ldr, float *part, int Min, int Mout, int K, int Cin, int Cout, int flags, void *stream);
/* fwd2 as the data gradient of a BatchNorm -> ReLU -> conv unit, with the BatchNorm-backward reductions in the epilogue:
 * out = (sum_k x[tbl[u,k]] @ Wk) * relu'(bn(bnx[u])), part = per-workgroup (sum out, sum out * xhat) per channel. */
int d3_spconv_fwd2_bnbwd(const void *x, int ldx, const int *tbl, const void *Wp, float *out, int ldo, float *part,
                         const float *bnx, int ldbx, const float *mean, const float *var, const float *gamma,
                         const float *beta, float eps, int relu, int Min, int Mout, int K, int Cin, int Cout, int flags,
                         void *stream);
/* Third-generation K = 27 forward / data-gradient kernel (round 6, csrc/spconv3.hip; replaces MinkowskiConvolution forward and
 * its data gradient at the stride-1 kernel-3 layers: model/common.py:38,41,66; model/pointgroup.py:70): x (Min, ldx) bf16,
 * tq = the level's lane table (d3_kmap_k3_packq), Wp = d3_spconv_pack fragments (K = 27), out (Mout, ldo) fp32 or bf16
 * (D3_CONV_OUTBF16), optional fp32 residual, optional BatchNorm partials part [d3_spconv_fwd3_nparts()][2][Cout] (+ part2
 * [16][2][Cout] fp64, zeroed by the caller).  Shapes with an instance: Cin/Cout in {16/16, 16/32, 32/16, 32/32, 32/64, 48/48,
 * 64/32}; others return D3_ERR_ARG (d3_spconv_fwd3_nparts() == 0).  _bnbwd: as d3_spconv_fwd2_bnbwd; bnx is fp32, or bf16 with
 * D3_CONV_BNXBF16 in flags.  d3_spconv_fwd3_launches(): launches so far (tests: the path really ran). */
int d3_spconv_fwd3_nparts(int Mout, int Cin, int Cout);
int d3_spconv_fwd3(const void *x, int ldx, const void *tq, const void *Wp, void *out, int ldo, const float *res, int ldr,
                   float *part, double *part2, int Min, int Mout, int Cin, int Cout, int flags, void *stream);
int d3_spconv_fwd3_bnbwd(const void *x, int ldx, const void *tq, const void *Wp, void *out, int ldo, float *part, double *part2,
                         const void *bnx, int ldbx, const float *mean, const float *var, const float *gamma, const float *beta,
                         float eps, int relu, int Min, int Mout, int Cin, int Cout, int flags, void *stream);
long long d3_spconv_fwd3_launches(void);
/* flags of the two queries: the D3_CONV_XSTAT / D3_CONV_XBF16 / D3_CONV_DYBF16 bits of the d3_spconv_wgrad2 call they size
 * (the kernel, and with it the number of row splits, depends on the operand types) */
size_t d3_spconv_wgrad2_ws_bytes(int Min, int Mout, int K, int Cin, int Cout, int flags);
int d3_spconv_wgrad2_splits(int Min, int Mout, int K, int Cin, int Cout, int flags);
int d3_spconv_wgrad2(const void *x, int ldx, const int *tbl, const void *dy, int ldy, float *dW, int Min, int Mout,
                     int K, int Cin, int Cout, int CinW, int flags, void *ws, size_t ws_bytes, void *stream);

/* Launch timing for bench.py: with profiling on, each MFMA convolution launch is bracketed by HIP events on
 * its stream.  family 0 = forward/data-gradient kernel (spconv_fwd2_kernel, or spconv_fwd_mfma_kernel for the first-
 * generation entry points), 1 = weight-gradient kernels, 2 = spconv_fwd2_split_kernel (few-row levels).
 * collect() synchronises. */
int d3_prof_enable(int on);
int d3_prof_collect(int family, long long *launches, double *total_ms, double *total_bytes, double *total_flops);
/* every sampled launch of a family as rows of 15 doubles {ms, bytes, flops, 12 tags}; families 3 = hg_gemm* (tags maxM, maxN,
 * K, problems, kernel 0 tiled / 1 split, row tiles, waves), 4 = td_gru4_fwd (1, N, H, I), 5 = cl_bfs2 (n, clusters), 6 = un_bn_*
 * (kernel, M, C); convolutions: Min, Mout, K, Cin, Cout + the template arguments of the instance (rocprofv3's kernel name).
 * *n = records of the family; at most `cap` rows are written.  No reference counterpart (measurement only). */
int d3_prof_dump(int family, double *rows, int cap, int *n);

/* Measurement / test switches.  The library reads its environment ONCE (csrc/tuning.hip: one
 * table, one parse at first use); these entry points let tests and the A/B tools flip a switch at run time instead of
 * mutating the environment.  name = the switch's environment name ("D3_WG3", "D3_BFS_NO_STAR", ...); unknown name ->
 * D3_ERR_ARG.  No reference counterpart: the reference's only switch on this path is CUDA_LAUNCH_BLOCKING
 * (scripts/train.py), read by the CUDA runtime. */
int d3_tuning_set(const char *name, int value);
int d3_tuning_get(const char *name, int *value);
int d3_tuning_count(void);
const char *d3_tuning_name(int i);

/* MinkowskiBatchNorm (+ MinkowskiReLU) over the rows of an (M,C) feature matrix
 * (reference: model/pointgroup.py:65,72-73; model/common.py:36-40).  Training-mode batch statistics.
 * stats : mean (C) and biased var (C) in fp32 (deterministic fp64 two-stage reduction); when running_mean /
 *         running_var are non-NULL they are updated like nn.BatchNorm1d in training mode
 *         (running = (1-momentum)*running + momentum*stat, unbiased variance).  ws >= d3_bn_ws_bytes(C).
 * fwd   : y = [relu]((x-mean)*rsqrt(var+eps)*gamma+beta)
 * bwd   : dx from dy (the relu mask is recomputed from x); dgamma / dbeta are WRITTEN. */
size_t d3_bn_ws_bytes(int C);
int d3_bn_stats(const float *x, int M, int C, float *mean, float *var, float *running_mean, float *running_var,
                float momentum, void *ws, size_t ws_bytes, void *stream);
int d3_bn_relu_fwd(const float *x, const float *mean, const float *var, const float *gamma, const float *beta,
                   float *y, int M, int C, float eps, int relu, void *stream);
/* same as d3_bn_relu_fwd with y stored as bf16 (RNE): for outputs consumed by a convolution (D3_CONV_XBF16) */
int d3_bn_relu_fwd_bf16(const float *x, const float *mean, const float *var, const float *gamma, const float *beta,
                        void *y_bf16, int M, int C, float eps, int relu, void *stream);
int d3_bn_relu_bwd(const float *x, const float *dy, const float *mean, const float *var, const float *gamma,
                   const float *beta, float *dx, float *dgamma, float *dbeta, int M, int C, float eps, int relu,
                   void *ws, size_t ws_bytes, void *stream);

/* ---- native sparse U-Net executor (csrc/unet.hip) ---------------------------------------------------
 * Runs the whole backbone / ScoreNet of the detector (model/pointgroup.py:69-74,88-92: stem conv, UBlock of
 * ResidualBlock / VGGBlock units (model/common.py:22-118), final BN + ReLU) from a layer program: one call for the
 * forward, one for the backward.  The program is three int64 tables built by d3net_amd/netexec.py:
 *   tensors (ntensors x 6): level, C, ld, coff, dtype (0 f32, 1 bf16), buffer id (-1 = the external input)
 *   bufs    (nbufs x 3)   : level, width, dtype
 *   prog    (nops x 16)   : [0] type 1 CONV {in, out, res|-1, weight param, map 0 k1 / 1 k3 / 2 down / 3 up, map level,
 *                           K, CinW (rows of the weight), stats 0/1}; 2 BNACT {in, out, -, gamma, beta, running_mean,
 *                           running_var, relu, eps bits, momentum bits}; 3 PADCAST {in, out} (fp32 -> zero-padded
 *                           bf16); 4 STATS {in} (batch statistics of the external input)
 * plan(rows per level) fixes the arena layout; forward writes activations / BN state / packed weights into the
 * caller's arena (kept for the backward); backward needs a gradient arena of grad_bytes.  params[i] / pgrads[i] are
 * device pointers of parameter i and of its gradient (NULL = frozen; paccum[i] != 0: accumulate).  k3 / child / up:
 * the kernel-map tables of d3_kmap_* per level.  Data gradients run on `stream`, weight gradients on an internal
 * side stream that `stream` joins before the call returns.
 * Memory owned by the network object (the exception to "no hidden allocation"): forward keeps a device copy of its
 * weight-packing job table (hipMalloc on first use / when the table grows; refreshing it synchronises `stream` once),
 * backward a pinned-host + device pair for the batched weight-gradient reduction jobs (hipHostMalloc + hipMalloc,
 * grow-only); a few KB each, released by d3_net_destroy. */
void *d3_net_create(const int64_t *prog, int nops, const int64_t *tensors, int ntensors, const int64_t *bufs, int nbufs,
                    int nlevels, int nparams, int input_needs_grad, int out_tensor);
void d3_net_destroy(void *net);
int d3_net_plan(void *net, const int *rows, size_t *arena_bytes, size_t *grad_bytes);
long long d3_net_tensor_offset(void *net, int tensor);
/* The executor's plan as numbers (pure host code, no GPU call): what d3_net_create decided per op, tensor and buffer, and, after a
 * d3_net_plan, where every region of the two arenas lies.  Returns the number of int64 words; fills `out` when cap suffices.
 * Layout: header[20] = version (1), nops, ntensors, nbufs, nlevels, planned, op_words, tensor_words, buf_words, f32, arena_bytes,
 * grad_bytes, cnt_off0, cnt_bytes, bcnt_off0, bcnt_bytes (the two zeroed-per-call areas), bnscr_off, bnscr_bytes, wgws_off,
 * wgws_bytes; then nops records of op_words, ntensors of tensor_words, nbufs of buf_words.
 * op record: type, in_grad_mode, res_mode, needs_dgrad_pack, bn_of_in, fused_by, wg_hazard, use_shadow, write_shadow, nsrcs,
 * 2 x (src op, c0, cn), fwd_flags, dgrad_flags (without D3_CONV_ACCUM: in_grad_mode == 2 adds it), wgrad_flags (without the per-call
 * D3_CONV_ACCUM), wgrad_map (0: the forward table, 1: the transposed one), wgrad_flip, k3_tables (may take the 16-bit / lane
 * table), Cin, Cout, dy_view (gradient view its backward reads dy from: a tensor, or ntensors + buffer = that buffer's bf16 shadow);
 * after a plan: wsplits, nparts_max, bparts_max, partw, then (offset, bytes) of wp_fwd, wp_bwd, part, part2, state (arena), bpart,
 * bpart2, wpart (gradient arena).
 * tensor record (its gradient view): kind (0: the caller's gin, 1: the caller's gout, 2: gradient arena), root buffer (-1 / -2 for
 * kinds 0 / 1), row stride, column offset, bf16, byte offset in the gradient arena (-1 before a plan and for kinds 0 / 1).
 * buffer record: galias, gbf, gabf, gshadow, need_grad; after a plan: off, bytes (arena), goff, gbytes, gshadow_off, gshadow_bytes
 * (gradient arena).  The field names live in d3net_amd/netexec.py (DESCRIBE_*), NativeUNet.describe() returns them named. */
long long d3_net_describe(void *net, int64_t *out, long long cap);
int d3_net_forward(void *net, const void *const *params, const int *const *k3, const int *const *child,
                   const int *const *up, const void *input, void *arena, int training, void *stream);
int d3_net_backward(void *net, const void *const *params, const int *const *k3, const int *const *child,
                    const int *const *up, const void *input, void *arena, void *grad_arena, const float *gout,
                    float *const *pgrads, const int *paccum, float *gin, void *stream);
/* Data-parallel overlap (the reference's DDP buckets: scripts/train.py:265-268 through Lightning).  The parameter gradients
 * of a backward complete in reverse program order, so a contiguous TAIL range of the flat gradient buffer is final long
 * before the call's last kernel.  d3_net_set_chunks: op_idx[k] (strictly descending) = the op after which chunk k is
 * complete; d3_net_backward then flushes the pending weight-gradient reductions there and records two events per chunk.
 * d3_net_chunk_wait makes `stream` wait for chunk k of the last backward -- the caller starts that chunk's all-reduce on
 * it while the rest of the backward is still running.  2 * (nchunks + 2) <= 32, i.e. nchunks <= 14 (else D3_ERR_ARG); 0 switches the feature off. */
int d3_net_set_chunks(void *net, const int *op_idx, int nchunks);
/* per level: the compact forms of the k3 table handed to the next d3_net_forward / d3_net_backward call -- k3_16[l]: the 16-bit
 * delta table (d3_kmap_k3_pack16; read by the weight-gradient kernels), k3_q[l]: the lane table (d3_kmap_k3_packq; read by
 * spconv_fwd3_kernel, the forward / data-gradient kernel of the big levels).  NULL entries, or NULL arrays, = dense tables only.
 * The caller passes only tables whose validity flag it has READ as 1.  The arrays are copied; the tables must stay alive like the
 * dense ones.  d3_spconv_t16_launches / d3_spconv_fwd3_launches: launches so far that read one (tests). */
int d3_net_set_k3_16(void *net, const void *const *k3_16, const int *const *k3_q);
/* Round 5 (input prefetch): the stem's zero-padded bf16 input prepared outside the forward.  d3_net_padded_channels: its width (0: this
 * executor has no such operand -- no stem, or the reference-precision program).  d3_net_padcast: (M, C_in) fp32 voxel features -> (M,
 * padded) bf16, the launch d3_net_forward would issue first.  d3_net_set_padded_input: hands the prepared buffer to the NEXT
 * d3_net_forward / d3_net_backward call (one call, then dropped), which reads the stem's operand from it.  No reference counterpart
 * (MinkowskiEngine convolves the fp32 features directly, model/pointgroup.py:70). */
int d3_net_padded_channels(void *net);
int d3_net_padcast(void *net, const void *input, void *out, long long M, void *stream);
int d3_net_set_padded_input(void *net, const void *xp);
long long d3_spconv_t16_launches(void);
int d3_net_chunk_wait(void *net, int k, void *stream);

/* ---- point-level heads (csrc/heads.hip) -------------------------------------------------------------
 * sem_seg / offset_net (model/pointgroup.py:77-85,274-279) and the semantic loss (:389-390) at N ~ 165k rows:
 *   tall_wgrad   : weight (and bias) gradient of y = x W^T + b for a tall-skinny x: dW (O,I) = dy^T x, db (O) = column
 *                  sums of dy (NULL to skip); I, O <= 32; deterministic two-stage reduction.
 *   cross_entropy: nn.functional.cross_entropy(z (N,C), label (N) int64, ignore_index), mean over counted rows:
 *                  out[0] = loss, out[1] = counted rows, grad (N,C) = softmax - onehot (0 on ignored rows). */
size_t d3_tall_wgrad_ws_bytes(int I, int O);
int d3_tall_wgrad(const float *x, const float *dy, float *dW, float *db, int N, int I, int O, void *ws, size_t ws_bytes,
                  void *stream);
/*   offset_loss  : the offset L1 and direction losses of PointGroup.loss (model/pointgroup.py:397-420) and their unscaled
 *                  gradients w.r.t. pt_offsets in one pass: out[0] = offset_norm_loss, out[1] = offset_dir_loss, out[2] =
 *                  sum(valid); d loss / d pt = (w_norm*g1 + w_dir*g2) / (out[2] + 1e-6). */
size_t d3_offset_loss_ws_bytes(void);
int d3_offset_loss(const float *pt, const float *coords, const float *info, int ldi, const int64_t *ids, long long ignore,
                   float *g1, float *g2, float *out, int N, void *ws, size_t ws_bytes, void *stream);
/* The two point-level heads of PointGroup (model/pointgroup.py:77-85, 277-283) on x (N, m = 16): scores (N,C) = x Ws^T + bs
 * (C <= 32), preds (N) int64 = first row arg-max, h (N,16) = x W0^T + b0, y (N,16) = ReLU(BatchNorm1d(h)) with batch statistics
 * (training != 0: running_mean / running_var / num_batches_tracked updated like nn.BatchNorm1d when given) or the running
 * statistics (training == 0), offsets (N,3) = y W3^T + b3.  stat (32) = [mean | 1/sqrt(var + eps)] (for the backward).
 * Three launches; x is read once.  ws: d3_point_heads_ws_bytes(). */
size_t d3_point_heads_ws_bytes(void);
int d3_point_heads_fwd(const float *x, long long N, int m, int C, const float *Ws, const float *bs, const float *W0, const float *b0,
                       const float *gamma, const float *beta, const float *W3, const float *b3, float eps, float momentum,
                       int training, float *running_mean, float *running_var, long long *num_batches_tracked, float *scores,
                       long long *preds, float *h, float *y, float *offsets, float *stat, void *ws, size_t ws_bytes, void *stream);
/* Backward pieces of the point heads: dy (N,16) = (g_off (N,3) W3 (3,16)) * (y > 0);  dx (N,16) = dh (N,16) W0 (16,16) +
 * g_scores (N,C) Ws (C,16) (either term may be NULL) -- the data gradients of the three tall Linear layers in one pass each
 * (the weight gradients: d3_tall_wgrad). */
int d3_point_heads_dy(const float *g_off, const float *W3, const float *y, long long N, float *dy, void *stream);
int d3_point_heads_dx(const float *dh, const float *W0, const float *g_scores, const float *Ws, long long N, int C, float *dx,
                      void *stream);
/* Proposal score loss of PointGroup.loss (reference model/pointgroup.py:436-452: ious.max(1), get_segmented_scores,
 * binary_cross_entropy_with_logits(...).mean()) in one launch.  ious: (P, nInst) row-major.  gt_iou: (P) row maxima;
 * dscore: (P) d loss / d score; out: 1 + P floats, out[0] = loss, out[1 + p] = proposal p's term (summed in proposal order). */
int d3_score_loss(const float *scores, const float *ious, int P, int nInst, float fg, float bg, float *gt_iou,
                  float *dscore, float *out, void *stream);
/* compute_cap_loss (lib/captioning/loss_helper.py:177-224) in two launches: pred (N,S,V) logits, target (N, S) int64 with row
 * pitch ld_target (a view of lang_ids[:, 1:S+1]), good (N) bool = descriptions whose target box passed the IoU threshold (the
 * others count as ignored, like target 0).  out2 = [sum of the word losses / count, word accuracy], count = max(#counted
 * words, 1); dpred (N,S,V) = d loss / d logits.  ws: d3_masked_xe_ws_bytes(N, S).  Deterministic. */
size_t d3_masked_xe_ws_bytes(int N, int S);
int d3_masked_xe(const float *pred, const long long *target, long long ld_target, const unsigned char *good, int N, int S, int V,
                 float *dpred, float *out2, void *ws, size_t ws_bytes, void *stream);
/* compute_node_orientation_loss (lib/captioning/loss_helper.py:244-307) in one launch.  preds: the num_bins orientation logits of
 * edge e of scene b at preds[b * ld_batch + e * ld_edge + 0..num_bins) (a view of the (B, E, num_bins + 1) edge predictions);
 * edge_index (B,2,E) float (compacted node ids; padded entries 0), num_src / num_tar (B) int64 (edges >= num_src * num_tar of a
 * scene get weight 0), assign (B,K) int64 = GT object of every proposal slot, rotations (B,G,3,3), rot_masks (B,G) fp32;
 * bounds_host = HOST pointer to the nbounds = num_bins - 1 bin boundaries (`radian_to_label`, :226-242), passed as kernel
 * arguments.  out2: 3 + 768 floats, out2[0..2] = [loss, accuracy, W = sum of the edge weights + 1e-8] (the rest: per-workgroup
 * partial sums); dpreds (B*E, num_bins) = W * d loss / d logits (the caller divides by W).  Deterministic (fixed-order reduction). */
int d3_orientation_loss(const float *preds, long long ld_batch, long long ld_edge, const float *edge_index,
                        const long long *num_src, const long long *num_tar, const long long *assign, const float *rotations,
                        const float *rot_masks, int B, int E, int K, int G, int num_bins, const float *bounds_host,
                        int nbounds, float *dpreds, float *out2, void *stream);
/* PointGroup.convert_stack_to_batch + get_object_assignments (reference model/pointgroup.py:216-263).  Kept proposals
 * (feats (P,m), crop (P,9): centre, size, -, semantic class, -; scores (P); bids (P) scene of each) are scattered to the
 * padded, per-scene shuffled (B,K,.) tensors, which the caller has zeroed: slot = b*K + inv_perm[b][rank of p in b]
 * for rank < K.  perm: (B,K) int64 permutations of 0..K-1.  slot: (P) out (-1: dropped).  assign (B,K) (optional):
 * index of the L1-nearest row of center_label (B,G,3) for every slot.  P <= 4096, B*K <= 8192. */
int d3_stack_to_batch(const float *feats, const float *crop, const float *scores, const int *bids, const long long *perm,
                      const float *center_label, int G, int P, int m, int B, int K, float *feats_b, float *bbox_b,
                      float *center_b, float *sem_b, float *scores_b, float *mask_b, long long *slot, long long *assign,
                      void *stream);
/* AdamW step (torch.optim.AdamW semantics: decoupled weight decay, bias-corrected moments, no amsgrad) over a list of
 * fp32 tensors in one launch.  ptrs: device table, 4 pointers per tensor (param, grad, exp_avg, exp_avg_sq); numel:
 * elements per tensor; blocks: (tensor, chunk) int pairs, one per workgroup, chunk = d3_adamw_chunk() elements.
 * The reference trains with torch.optim.Adam/AdamW through Lightning (model/pipeline.py:738-757). */
int d3_adamw_chunk(void);
int d3_adamw(const long long *ptrs, const int *numel, const void *blocks, int nblocks, double lr, double beta1, double beta2,
             double eps, double weight_decay, double bias_correction1, double bias_correction2_sqrt, void *stream);
/* Adam and SGD steps with the tables of d3_adamw (csrc/optim.hip), one launch per call: the other two optimizers that
 * `train.optim.classname` names (model/pipeline.py:738-757 for the pipeline, model/pointgroup.py:372-384 for the detector).
 * d3_adam: torch.optim.Adam with amsgrad = maximize = False; weight decay is L2, added to the gradient (g' = g + wd p)
 * before the moments; table columns (param, grad, exp_avg, exp_avg_sq).
 * d3_sgd: torch.optim.SGD with dampening = 0, nesterov = maximize = False; table columns (param, grad, momentum_buffer,
 * unused).  momentum == 0: no buffer is read or written.  first != 0: the launched range receives its first update,
 * buf = g' (the buffer is written, never read); first == 0: buf = momentum buf + g'.  first != 0 with momentum == 0:
 * D3_ERR_ARG. */
int d3_adam(const long long *ptrs, const int *numel, const void *blocks, int nblocks, double lr, double beta1, double beta2,
            double eps, double weight_decay, double bias_correction1, double bias_correction2_sqrt, void *stream);
int d3_sgd(const long long *ptrs, const int *numel, const void *blocks, int nblocks, double lr, double momentum,
           double weight_decay, int first, void *stream);
/* Global gradient-norm clipping and the non-finite skip for the three steps above, over their own tables: what
 * torch.nn.utils.clip_grad_norm_ does in front of a torch.optim step, and what Lightning's `gradient_clip_val` switches on
 * for the reference.  Two launches produce the control record; the _clipped steps read it and leave the gradients in
 * memory as they are.
 * The record (32 bytes of device memory, zero-filled by the caller before its first use):
 *   norm      the total 2-norm of the gradients before clipping (double accumulation, narrowed once)
 *   coef      torch.nn.utils.clip_grad_norm_'s coefficient in fp32: min(1.0f, max_norm / (norm + 1e-6f)); exactly 1 for
 *             max_norm = +inf and a finite norm (measure only); NaN when norm is NaN
 *   skip      1 when norm is not finite, else 0
 *   nskipped  incremented by every d3_grad_clip_finish whose skip is 1: cumulative
 *   enforce   written by the HOST alone: non-zero makes the _clipped steps return before their first store while skip
 *             is 1; zero makes them ignore skip (the non-finite coefficient then propagates, as it does through torch) */
typedef struct d3_clip_ctl {
    float norm;
    float coef;
    int skip;
    int nskipped;
    int enforce;
    int reserved[3];
} d3_clip_ctl;
/* d3_grad_sumsq: the first half of torch.nn.utils.clip_grad_norm_'s norm.  partials[b] = sum of grad^2 (table column 1)
 * over block b of the map, b in [0, nblocks), accumulated in double in a fixed order; no atomics.
 * d3_grad_clip_finish: sums partials[0..n) in double in a fixed order (n spans every group of the optimizer, one
 * contiguous segment per d3_grad_sumsq call; n == 0: norm 0), takes the square root and writes norm, coef, skip and
 * nskipped of the record as torch.nn.utils.clip_grad_norm_(max_norm) defines them.  max_norm > 0, +inf allowed.
 * The record is bit-identical from run to run for the same gradients. */
int d3_grad_sumsq(const long long *ptrs, const int *numel, const void *blocks, int nblocks, double *partials, void *stream);
int d3_grad_clip_finish(const double *partials, int n, double max_norm, void *ctl, void *stream);
/* d3_adamw / d3_adam / d3_sgd behind torch.nn.utils.clip_grad_norm_: each element uses g * ctl->coef (one fp32 multiply,
 * what clip_grad_norm_'s in-place mul_ would have left in memory; the gradient itself is NOT rewritten), and the launch
 * stores nothing while ctl->skip and ctl->enforce are set.  ctl: the device record d3_grad_clip_finish wrote on the
 * same stream. */
int d3_adamw_clipped(const long long *ptrs, const int *numel, const void *blocks, int nblocks, double lr, double beta1,
                     double beta2, double eps, double weight_decay, double bias_correction1, double bias_correction2_sqrt,
                     const void *ctl, void *stream);
int d3_adam_clipped(const long long *ptrs, const int *numel, const void *blocks, int nblocks, double lr, double beta1,
                    double beta2, double eps, double weight_decay, double bias_correction1, double bias_correction2_sqrt,
                    const void *ctl, void *stream);
int d3_sgd_clipped(const long long *ptrs, const int *numel, const void *blocks, int nblocks, double lr, double momentum,
                   double weight_decay, int first, const void *ctl, void *stream);
/* out[idx[s], :] += g[s, :] (out zero-filled by the caller): backward of the cluster feature gather
 * (model/pointgroup.py:130); deterministic when every output row receives at most two addends, as it does there */
int d3_scatter_add_rows(const float *g, const int64_t *idx, float *out, long long S, int C, void *stream);
/* out (S,C) = feats[idx]: the forward of the same gathers (C % 4 == 0) */
int d3_gather_rows(const float *feats, const int64_t *idx, float *out, long long S, int C, void *stream);
/* out[r] = idx[r] in [0, rows) ? feats[idx[r]] : 0 (scatter == 0; S rows of C floats), or its transpose for UNIQUE indices
 * (scatter != 0: out[idx[r]] = feats[r] for the in-range entries, out (rows, C) zero-filled by the caller): the padded
 * placement of the relation graph's edge messages / predictions (model/graph_module.py:291-308) without the zero-row copy. */
int d3_gather_rows_pad(const float *feats, long long rows, const int64_t *idx, float *out, long long S, int C, int scatter,
                       void *stream);
size_t d3_cross_entropy_ws_bytes(void);
int d3_cross_entropy(const float *z, const int64_t *label, float *grad, float *out, int N, int C, int ignore_index,
                     void *ws, size_t ws_bytes, void *stream);

/* ---- proposal-level attention (listener) ------------------------------------------------ */
/* Core of ScaledDotProductAttention.forward between the projections (model/transformer/attention.py:61-75):
 * softmax(q k^T / sqrt(dk) + bias, masked where mask == 0) v, per (batch item, head), fp32.
 * q (B,nq,h*dk), k (B,nk,h*dk), v (B,nk,h*dv), out (B,nq,h*dv) -- the layouts nn.Linear produces;
 * bias (B/bias_div, h, nq, nk) or NULL: additive attention weights, shared by bias_div consecutive batch items
 * (the reference replicates them per description chunk, model/match_module.py:324-326);
 * mask (B, nk) or NULL: 0 = masked key (the reference replicates it to (B,h,nq,nk), match_module.py:191-197);
 * P (B,h,nq,nk): softmax probabilities, kept for the backward.  nq,nk <= 128, dk,dv <= 32.
 * bwd: dS (B,h,nq,nk) scratch; dq, dk, dv written. */
int d3_attn_fwd(const float *q, const float *k, const float *v, const float *bias, const float *mask, float *out,
                float *P, int B, int h, int nq, int nk, int dk, int dv, int bias_div, void *stream);
int d3_attn_bwd(const float *q, const float *k, const float *v, const float *P, const float *dout, float *dS,
                float *dq, float *dk, float *dv, int B, int h, int nq, int nk, int dkdim, int dvdim, void *stream);

/* Fused residual add + LayerNorm (csrc/layernorm.hip): y = LayerNorm(a + b) * gamma + beta over the last dimension D of R
 * rows (b may be NULL), torch.nn.LayerNorm semantics (biased variance, eps inside the root).  Replaces
 * `self.layer_norm(queries + out)` of MultiHeadAttention (model/transformer/attention.py:170-176) and the LayerNorm of
 * `lang_fc` (model/match_module.py:170-173).  mean / rstd (R each) are kept for the backward; bwd: dx = d(a) = d(b),
 * dgamma / dbeta (D each, written); ws >= d3_layernorm_ws_bytes(R, D).  D <= 1024. */
int d3_layernorm_fwd(const float *a, const float *b, const float *gamma, const float *beta, float *y, float *mean,
                     float *rstd, int R, int D, float eps, void *stream);
size_t d3_layernorm_ws_bytes(int R, int D);
int d3_layernorm_bwd(const float *a, const float *b, const float *gamma, const float *mean, const float *rstd,
                     const float *dy, float *dx, float *dgamma, float *dbeta, int R, int D, void *ws, size_t ws_bytes,
                     void *stream);

/* ---- ScanRefer match module of the listener (csrc/scanrefer_match.hip) ---------------------------------
 * MatchModule.forward (model/match_module.py:24-39 the layers, :110-139 the supervised branch, :50-108 the RL branch):
 *     conf (N,K) = match(fuse(mask . cat[feats[n / div], lang[n]]))   with training- or eval-mode BatchNorm1d,
 * without the (N, K, m+L) concatenation or the per-description copies of the proposal rows: the first convolution is split into
 * P = feats W0[:, :m]^T and Q = lang W0[:, m:]^T, h1 = mask (P + Q) + b0 is recomputed where needed, and the chain is cut only
 * where a training-mode BatchNorm needs statistics over all N K positions (per-workgroup partial sums in double, added in
 * workgroup order by the consumer: deterministic, no atomics).  Hidden width 128 only; m % 4 == 0; N == B * div.
 *   feats (B,K,m), lang (N,L), mask (B,K) or NULL (RL branch: no mask, :76-83); W0 (128, m+L) = fuse.0, g1/be1/rm1/rv1 = fuse.1
 *   (running statistics and the nbt counters updated in place when train != 0: momentum, unbiased variance), alpha (128) = fuse.2, W3/b3 = fuse.3,
 *   W4/b4 = match.0, g2.. = match.2, W5/b5 = match.3, g3.. = match.5, w6 (128) / b6 (1) = match.6.
 *   Scratch the caller provides: PQ ((B K + N), 128); part (3, G, 2, 128) doubles with G = d3_scanrefer_match_groups(N, K);
 *   y2, y3 (N K, 128) (required when train != 0); x1, f, z2 (N K, 128) and bnstat (3, 2, 128: mean, rstd) are kept for the
 *   backward -- all of x1 / f / y2 / z2 / y3 / bnstat, or x1 == NULL for a forward without one.
 * fwd launches: 1-2 (hgemm P, Q) + 4 (train) or + 1 (eval).  bwd: 4 kernels + column sums + weight-gradient hgemm calls; dfeats
 * (B,K,m) / dlang (N,L) may be NULL; dW0 .. db6 are written (not accumulated); the rest of d3_srm_grads is scratch:
 * dpre3, dz2, dpre2, df, dbn1 (N K, 128), dP (B K, 128), dQ, db0part (N, 128), part (3, G, 3, 128) doubles,
 * ws >= d3_scanrefer_match_bwd_ws_bytes(). */
typedef struct {
    int B, K, N, div, m, L;
    const float *feats, *lang, *mask;
    const float *W0, *b0, *g1, *be1; float *rm1, *rv1; const float *alpha;
    const float *W3, *b3, *W4, *b4, *g2, *be2; float *rm2, *rv2;
    const float *W5, *b5, *g3, *be3; float *rm3, *rv3; const float *w6, *b6;
    float eps[3], momentum[3];
    long long *nbt[3];          /* num_batches_tracked of fuse.1, match.2, match.5 (or NULL): += 1 by the forward when train != 0 */
    float *PQ; double *part;
    float *x1, *f, *y2, *z2, *y3, *bnstat;
    float *conf;
} d3_srm_args;
typedef struct {
    const float *dconf;
    float *dW0, *db0, *dg1, *dbe1, *dalpha, *dW3, *db3, *dW4, *db4, *dg2, *dbe2, *dW5, *db5, *dg3, *dbe3, *dw6, *db6;
    float *dfeats, *dlang;
    float *dpre3, *dz2, *dpre2, *df, *dbn1, *dP, *dQ, *db0part; double *part;
    void *ws; size_t ws_bytes;
} d3_srm_grads;
int d3_scanrefer_match_groups(int N, int K);
int d3_scanrefer_match_fwd(const d3_srm_args *a, int train, void *stream);
size_t d3_scanrefer_match_bwd_ws_bytes(void);
int d3_scanrefer_match_bwd(const d3_srm_args *a, const d3_srm_grads *g, int train, void *stream);

/* ---- small-batch fp32 GEMMs of the proposal-level heads (csrc/hgemm.hip) ---------------------------
 * Every nn.Linear / nn.GRUCell product of the speaker and listener heads (model/caption_module.py:72-133,
 * model/graph_module.py:101-108, model/lang_module.py:51-55):
 *     C (M,N) [+]= act( sum_seg A_seg (M,K_seg) . B_seg (N,K_seg)^T + bias[N] + add (M,N) )
 * fp32 operands, exact fp32 products and accumulation on the matrix cores (v_mfma_f32_16x16x4_f32).  Up to three K
 * segments (torch.cat of inputs against one weight matrix is never materialised); A rows of a segment may be gathered
 * through `ia` (embedding lookup); an operand is row-major (element (r,k) at base[r*ld + k]) or k-major (base[k*ld + r]):
 * y = x W^T, dx = dy W (B k-major) and dW = dy^T x (both k-major) are the same kernel.  perm_nb > 0 stores row r at row
 * (r % perm_nb) * perm_s + r / perm_nb (time-major rows -> batch-major logits).  Up to 4 problems per call share a launch. */
typedef struct {
    const float *A; const int *ia; long long lda; int a_kmajor;
    const float *B; long long ldb; int b_kmajor;
    int K;
} d3_gemm_seg;
typedef struct {
    d3_gemm_seg seg[3]; int nseg;
    int M, N;
    float *C; long long ldc;
    const float *bias; const float *add; long long ldadd;
    int relu, accum, perm_nb, perm_s;
    /* Optional epilogue, gru != 0 (round 5; N == gru_H; the wave-per-tile / K-split kernels only: fewer than 2048 16 x 16 output tiles): the finished
     * element v (after bias / add / accumulate) is the last contribution to dh', the gradient of a GRUCell's NEW state, and the
     * cell's gate backward (torch.nn.GRUCell's autograd as model/caption_module.py:72-133 uses it) runs on it in place of a
     * launch of its own:   dh' = g_d0 + g_d1 + v  (NULL = absent);  dn = dh'(1-z), dz = dh'(hp-n), dn_pre = dn(1-n^2),
     *   g_dgi[row] = [dn_pre ghn r(1-r), dz z(1-z), dn_pre],  g_dgh[row] = [same, same, dn_pre r],  g_dhp = dh' z.
     * r / z / n / ghn: the cell's saved gates (M, gru_H); hp: its previous state (row stride g_ldh).  C is read (accumulate) but NOT
     * written in this mode: the carried gradient goes to g_dhp, which may alias C. */
    int gru, gru_H;
    const float *g_d0; long long g_ld0; const float *g_d1; long long g_ld1;
    const float *g_r, *g_z, *g_n, *g_ghn, *g_hp; long long g_ldh;
    float *g_dgi; long long g_lddgi; float *g_dgh; float *g_dhp;
} d3_gemm_prob;
int d3_hgemm(const d3_gemm_prob *probs, int nprobs, void *stream);
/* out[c] (+)= sum_r x[r*ld + c], r < R, c < C (bias gradients; two-stage, fixed summation order); ws >= d3_colsum_ws_bytes(C) */
size_t d3_colsum_ws_bytes(int C);
int d3_colsum(const float *x, long long ld, int R, int C, float *out, int accum, void *ws, size_t ws_bytes, void *stream);

/* ---- top-down captioner, native (csrc/topdown.hip) -------------------------------------------------------
 * TopDownSceneCaptionModule (model/caption_module.py:13-62 parameters, :72-133 step, :510-687 teacher-forced driver):
 * x1 = map_topdown([emb[word] | h2 | target]); h1 = GRUCell1(x1, h1); a = softmax_k(attend . tanh(map_feat(obj)[k] +
 * map_hidd(h1)), masked scores := 0); att = sum_k a[k] obj[k]; x2 = map_lang([att | h1]); h2 = GRUCell2(x2, h2);
 * logits = classifier(h2), for S steps with teacher forcing (step t reads word_ids[n, t]).  N samples, K proposals,
 * H hidden (512), E embedding (300), F feature (128), V vocabulary.  All matrices row-major fp32, nn.Linear layout
 * (out, in); GRU weights (3H, in) in torch's r, z, n gate order.  ws: d3_topdown_ws_bytes() bytes, filled by the forward
 * and read by the backward (saved activations).  H % 16 == 0, E % 4 == 0, F % 4 == 0, F <= 128. */
typedef struct {
    int N, K, S, V, H, E, F, Tw;          /* Tw: row stride of word_ids */
    const long long *word_ids;            /* (N, Tw) */
    const float *emb;                     /* (V, E) */
    const float *target;                  /* (N, F) */
    const float *obj;                     /* (N, K, F) */
    const float *mask;                    /* (N, K): 0 = masked proposal */
    const float *W_td, *b_td;             /* map_topdown (E, E+H+F), (E) */
    const float *Wih1, *Whh1, *bih1, *bhh1;   /* recurrent_cell_1 */
    const float *W_feat, *W_hidd, *w_att;     /* map_feat (H,F), map_hidd (H,H), attend (1,H) */
    const float *W_lang, *b_lang;         /* map_lang (E, F+H), (E) */
    const float *Wih2, *Whh2, *bih2, *bhh2;   /* recurrent_cell_2 */
    const float *Wc0, *bc0, *Wc2, *bc2;   /* classifier.0 (H,H), classifier.2 (V,H) */
    float *logits;                        /* out (N, S, V) */
    float *attn;                          /* out (N, K, S) = topdown_attn, or NULL */
    void *ws; size_t ws_bytes;
} d3_topdown_args;
typedef struct {
    const float *dlogits;                 /* (N, S, V) */
    float *dW_td, *db_td, *dWih1, *dWhh1, *dbih1, *dbhh1, *dW_feat, *dW_hidd, *dw_att, *dW_lang, *db_lang;
    float *dWih2, *dWhh2, *dbih2, *dbhh2, *dWc0, *dbc0, *dWc2, *dbc2;   /* written (same shapes as the parameters) */
    float *dobj, *dtarget;                /* (N,K,F), (N,F): written */
    void *ws; size_t ws_bytes;            /* d3_topdown_bwd_ws_bytes() of scratch */
} d3_topdown_grads;
size_t d3_topdown_ws_bytes(int N, int K, int S, int H, int E, int F);
size_t d3_topdown_bwd_ws_bytes(int N, int K, int S, int V, int H, int E, int F);
int d3_topdown_xe_forward(const d3_topdown_args *a, void *stream);
int d3_topdown_xe_backward(const d3_topdown_args *a, const d3_topdown_grads *g, void *stream);
/* the same with the parameter-gradient work (weight-gradient GEMMs batched over time, bias column sums: nothing the rest of the
 * backward waits for) on a second stream `side` (NULL: everything on `stream`).  The call forks `side` off `stream`; the caller joins:
 * `side` must be waited for before a parameter gradient is read, and every buffer of `a` / `g` must stay alive until then. */
int d3_topdown_xe_backward_ex(const d3_topdown_args *a, const d3_topdown_grads *g, void *stream, void *side);
/* One decode step for the greedy / evaluation decodes (model/caption_module.py:350-383, 689-770), inference only: uses N, K,
 * V, H, E, F, emb, target, obj, mask and the parameters of `a`.  word (N) int64 -> logits (N,V), attn (N,K); hidden states
 * h1_in / h2_in (N,H) -> h1_out / h2_out (distinct buffers).  fp = map_feat(obj) from d3_topdown_feat_proj (rows = number of
 * (K,F) object blocks * K).  obj_div: consecutive samples sharing one object block (1: one block per sample). */
size_t d3_topdown_step_ws_bytes(int N, int K, int H, int E, int F);
int d3_topdown_feat_proj(const float *obj, const float *W_feat, float *fp, int rows, int H, int F, void *stream);
int d3_topdown_step(const d3_topdown_args *a, const long long *word, const float *fp, int obj_div, const float *h1_in,
                    const float *h2_in, float *h1_out, float *h2_out, float *logits, float *attn, void *ws, size_t ws_bytes,
                    void *stream);

/* Selection step of the sampling loops around d3_topdown_step (beam search: model/caption_module.py:136-349; greedy: :350-383) in
 * one launch each: log_softmax, candidate scores sums + logp, the b best of live * V candidates best first (ties: lower flat
 * index), beam_ix / tok / chosen log-prob / running sums (snapshot and the -1000 penalised continuation, :300) / ended flags, the
 * token histories of the chosen beams (seq_out[n][r][:t] = seq_prev[n][beam_ix][:t], seq_out[n][r][t] = tok; rows of Tmax int64)
 * and the re-ordering of the two hidden states (h*_out row n*b + r = h*_in row n*b + beam_ix; h1_in NULL: skipped).
 * logits (N*b, V): row n*b + j = live beam j of sample n (live = 1 at t = 0); sums_in (N, live).  b <= 8.
 * d3_greedy_select: word[n] = first arg-max of logits[n], lp[n] = its log-softmax value. */
int d3_beam_select(const float *logits, const float *sums_in, int N, int live, int b, int V, int eos, int last, int t, int Tmax,
                   const long long *seq_prev, long long *seq_out, long long *tok_out, float *snap_out, unsigned char *ended_out,
                   float *sums_out, const float *h1_in, const float *h2_in, float *h1_out, float *h2_out, int H, void *stream);
int d3_greedy_select(const float *logits, int N, int V, long long *word, float *lp, void *stream);
/* The two decodes as single calls (same launches as the loops over d3_topdown_step + d3_*_select, issued inside the library).
 * d3_topdown_greedy (model/caption_module.py:350-383): h1_a / h2_a (N,H) = initial (zero) states, h1_b / h2_b scratch, logits (N,V)
 * and attn (N,K) scratch, first_word (N) = sos; words / lps (max_len, N) written.
 * d3_topdown_beam (:136-349): a->N = samples * b rows (row n*b + j = beam j of sample n, obj_div = b); h1 / h2: three (N,H) buffers
 * each, [0] = initial (zero) states; allseq (max_len, samples, b, max_len) zero-filled by the caller, snap_all / ended_all (max_len,
 * samples, b), sums0 (samples, b) zero-filled, sums1 (samples, b) and tok (a->N) scratch.  Every step's beams are kept (a beam that
 * ended at step t: ended_all[t] != 0, its score snap_all[t], its tokens allseq[t][..][:t+1]). */
int d3_topdown_greedy(const d3_topdown_args *a, const float *fp, int obj_div, float *h1_a, float *h2_a, float *h1_b, float *h2_b,
                      float *logits, float *attn, void *ws, size_t ws_bytes, const long long *first_word, int max_len,
                      long long *words, float *lps, void *stream);
int d3_topdown_beam(const d3_topdown_args *a, const float *fp, int b, float *const *h1, float *const *h2, float *logits, float *attn,
                    void *ws, size_t ws_bytes, const long long *first_word, int eos, int max_len, long long *allseq, float *snap_all,
                    unsigned char *ended_all, float *sums0, float *sums1, long long *tok, void *stream);
/* Both decodes of one self-critical step (model/caption_module.py:588-633) as one chain: a->N = samples * (b + 1) rows, row
 * n*(b+1) + j = beam j of sample n (j < b) / its greedy row (j = b), obj_div = b + 1; beam outputs as d3_topdown_beam, greedy
 * outputs g_words / g_lps (glen, samples), glen >= max_len.  tok (a->N) scratch.  Row for row the arithmetic of the separate calls. */
int d3_topdown_beam_greedy(const d3_topdown_args *a, const float *fp, int b, float *const *h1, float *const *h2, float *logits,
                           float *attn, void *ws, size_t ws_bytes, const long long *first_word, int eos, int max_len,
                           long long *allseq, float *snap_all, unsigned char *ended_all, float *sums0, float *sums1, long long *tok,
                           int glen, long long *g_words, float *g_lps, void *stream);

/* ---- packed-sequence GRU of the language encoder (csrc/topdown.hip) ---------------------------------------
 * nn.GRU(I -> H, batch_first=True) over pack_padded_sequence(x (N,T,I), lens (N)) as LangModule runs it
 * (model/lang_module.py:51-55, 146-150; torch gate order r, z, n): hiddens (N,T,H) zero beyond a sample's length, last (N,H)
 * the final state of every sample.  ws (d3_gru_seq_ws_bytes) keeps the input-side gates, states and gate values for the
 * backward.  backward: d_hiddens / d_last (either NULL) -> dWih (3H,I), dWhh (3H,H), dbih, dbhh (3H) written; dx (N,T,I)
 * written when non-NULL.  H % 16 == 0, I % 4 == 0. */
size_t d3_gru_seq_ws_bytes(int N, int T, int I, int H);
size_t d3_gru_seq_bwd_ws_bytes(int N, int T, int I, int H);
int d3_gru_seq_forward(const float *x, const int *lens, const float *Wih, const float *Whh, const float *bih, const float *bhh, int N,
                       int T, int I, int H, float *hiddens, float *last, void *ws, size_t ws_bytes, void *stream);
int d3_gru_seq_backward(const float *x, const int *lens, const float *Wih, const float *Whh, int N, int T, int I, int H,
                        const float *d_hiddens, const float *d_last, const void *ws, float *dWih, float *dWhh, float *dbih, float *dbhh,
                        float *dx, void *ws2, size_t ws2_bytes, void *stream);

/* ---- relation graph (csrc/edgeconv.hip) -----------------------------------------------------------------
 * GraphModule / EdgeConv (model/graph_module.py:21-114, 252-324) for all B scenes at once, fixed-size outputs, no host
 * round trip.  adj (B,K,K) 0/1 adjacency (rows = _query_locals of every proposal, L ones each), mask (B,K) valid proposals.
 * Edges = row-major non-zeros of adj restricted to valid x valid (the reference's scipy COO order), stored per scene in a
 * padded block of K*L slots:
 *   src / dst (B,K*L) int32   global node ids b*K + slot of the adjacency row (x_j) / column (x_i, aggregation target), -1 pad
 *   edge_index (B,2,K*L) f32  the reference's `edge_index` output: compacted (valid-only) node ids of the first n edges
 *   cnt (B,4) int32           E, n_source (rows with an edge), n_target = E / n_source, number of valid nodes
 *   in_ptr (B,K+1), in_list (B,K*L): incoming edges (scene-local edge ids) of every node in edge order
 *   out_start / out_cnt (B,K): the contiguous outgoing range of every node
 *   feat_src / pred_src (B,K*L) int64: row of the (B*K*L [+1 zero row], C) message / prediction matrix that lands in slot
 *       (r, k) of `edge_feature` (message r*n_target + k) resp. row j of `edge_orientations` (only when E == n); B*K*L = none
 * edgeconv_fwd: message = W2 relu(W0 [x_i | x_j - x_i] + b0) + b2 per edge (fp32 matrix cores), node = sum of incoming
 * messages in edge order.  ws (d3_edgeconv_ws_bytes) keeps [edge inputs | hidden] for the backward. */
int d3_graph_edges(const float *adj, const float *mask, int B, int K, int L, int *src, int *dst, float *edge_index, int *cnt,
                   int *in_ptr, int *in_list, int *out_start, int *out_cnt, long long *feat_src, long long *pred_src,
                   void *stream);
size_t d3_edgeconv_ws_bytes(int Emax, int Cin, int Cout);
size_t d3_edgeconv_bwd_ws_bytes(int Emax, int Cin, int Cout);
int d3_edgeconv_fwd(const float *x, const float *W0, const float *b0, const float *W2, const float *b2, const int *src,
                    const int *dst, const int *in_ptr, const int *in_list, int B, int K, int L, int Cin, int Cout, float *node,
                    float *msg, void *ws, size_t ws_bytes, void *stream);
int d3_edgeconv_bwd(const float *W0, const float *W2, const int *src, const int *dst, const int *in_ptr, const int *in_list,
                    const int *out_start, const int *out_cnt, int B, int K, int L, int Cin, int Cout, const float *d_node,
                    const float *d_msg, const void *ws, float *dx, float *dW0, float *db0, float *dW2, float *db2, void *ws2,
                    size_t ws2_bytes, void *stream);

/* ---- evaluation-path non-maximum suppressions (csrc/nms.hip) ------------------------------------------------
 * nms3d_samecls: class-aware greedy 3D box NMS of parse_predictions (lib/det/ap_helper.py:80-108, lib/det/nms.py:110-150),
 *   all scenes in one launch.  boxes (B,K,8) = [x1,y1,z1,x2,y2,z2,score,class], valid (B,K) != 0 -> pick (B,K) 0/1;
 *   float64 arithmetic like the numpy original; K <= 256.  visit: NULL (descending score, exact ties: later index first) or
 *   (B,K) int32 candidate indices in visiting order, -1 padded (numpy's argsort leaves the order of tied scores to its sort
 *   implementation; pass its order to reproduce it).
 * instance_cross_iou: point-mask IoU between all pairs of clusters (model/pointgroup.py:577-589) from the (cluster, point)
 *   lists instead of a dense (P,N) mask product; ious (P,P) f32; member: 2*N ints scratch; *overflow_dev = 1 when a point is
 *   in more than two clusters (then the result is invalid).
 * nms_matrix: get_nms_instances (lib/utils/eval.py:75-97) over a dense IoU matrix: candidates keep[i] != 0 in descending
 *   score; picked[0..*npicked) in pick order.  order_scratch / picked: n ints each.  n <= 12288. */
int d3_nms3d_samecls(const float *boxes, const float *valid, const int *visit, int B, int K, double iou_thr, int old_type, float *pick,
                     void *stream);
int d3_instance_cross_iou(const int *cluster_idxs, const int *offsets, long long S, int P, int N, float *ious, int *member,
                          int *overflow_dev, void *stream);
int d3_nms_matrix(const float *ious, const float *scores, const unsigned char *keep, int n, float thr, int *order_scratch, int *picked,
                  int *npicked, void *stream);

/* ---- segmentation evaluation counts (csrc/seg_eval.hip) ---------------------------------------------------------------------
 * The per-point counting of the ScanNet segmentation evaluators for a batch of B scenes (points [batch_offsets[b],
 * batch_offsets[b+1]) of N; batch_offsets nondecreasing, batch_offsets[B] <= N), all ids int32 raw class ids in [0, 40):
 *   gt_sem / gt_inst: the reference's GT files (lib/utils/eval.py:14-56, value = sem * 1000 + inst) split in two, gt_inst 1-based
 *     within its scene (0 = none, <= G = the largest id of any scene); pred_sem: NYU20_CLASS_IDX[1:][argmax] (model/pointgroup.py:561-566);
 *   predictions: pick[0..n_pick) proposal ids into proposals_offset (P+1) / proposals_idx (S,2) [cluster, point], in pick order.
 * Outputs (int32, bit-exact):
 *   confusion (40,40) [gt][pred] summed over the batch, GT row 0 included (lib/evaluation/semantic_segmentation.py:18-25);
 *   gt_stats (B,G,2) = [vertex count, class = first maximum of the instance's GT class bincount] (lib/utils/eval.py:142-158);
 *   pred_stats (n_pick,5) = [vertex count, void intersection (GT class not in inst_class_mask, bit per class id), class of the first
 *     member, scene of the first member, flags: 1 members disagree on the class (model/pointgroup.py:620 asserts they agree),
 *     2 a member outside that scene or a malformed pick / segment];
 *   inter (n_pick,G): points of prediction j with gt_inst == k + 1 in its scene (lib/evaluation/instance_segmentation.py:219-274);
 *   *status (device) = 1 when some point's ids are out of range (those points are skipped).
 * G > d3_seg_eval_max_inst() (the LDS bound of the point pass) returns D3_ERR_RANGE before any launch; ws: d3_seg_eval_ws_bytes(B, G). */
int d3_seg_eval_max_inst(void);
size_t d3_seg_eval_ws_bytes(int B, int G);
int d3_seg_eval(const int *gt_sem, const int *gt_inst, const int *pred_sem, const int *batch_offsets, int B, int N, int max_scene_points,
                int G, const int *pick, int n_pick, const int *proposals_idx, const int *proposals_offset, int P, long long S,
                unsigned long long inst_class_mask, int *confusion, int *gt_stats, int *pred_stats, int *inter, int *status, void *ws,
                size_t ws_bytes, void *stream);

/* ---- dense-caption assignment (csrc/assign.hip) ------------------------------------------------------------------------------
 * The Hungarian step of the captioning evaluation, one workgroup per scene, no host round trip.
 * d3_lsap_batched: scipy.optimize.linear_sum_assignment(cost[b, :, :ncols[b]]) for every scene b, as the loop of
 *   lib/captioning/eval_helper.py:120-182 (box_assignment) calls it.  cost (B,R,C) float32; ncols (B) int32, clamped to [0, C];
 *   per_col (B,C) int32: per_col[b, col] = row for the assigned pairs, every other element 0 (what `per_gt[b, cols] = rows`
 *   leaves on the host; the kernel writes all B * C elements); status (B) int32: 0 solved, 1 a non-finite cost in a valid
 *   column (scipy raises ValueError), 2 infeasible; per_col[b] is all 0 unless status[b] == 0.  float64 solver state, scipy's
 *   tie order.  R > 256 or C > 256: D3_ERR_RANGE before any launch.
 * d3_dense_caption_assign: the same solve with cost = -GIoU(proposal, GT) computed inside the kernel in float32, in the
 *   operation order of lib/utils/bbox.py generalized_box3d_iou (axis-aligned path, rotated_boxes=False) as
 *   d3net_amd.caption_eval restates it.  pred_boxes (B,K,8,3), gt_boxes (B,G,8,3) float32 corners; nactual (B) int32 valid GT
 *   boxes; per_gt (B,G) int32 and status (B) as above; cost_out: NULL, or (B,K,G) float32 that receives the cost (0 in the
 *   padded columns).  K > 256 or G > 256: D3_ERR_RANGE before any launch. */
int d3_lsap_batched(const float *cost, const int *ncols, int B, int R, int C, int *per_col, int *status, void *stream);
int d3_dense_caption_assign(const float *pred_boxes, const float *gt_boxes, const int *nactual, int B, int K, int G, int *per_gt,
                            int *status, float *cost_out, void *stream);

/* ---- detection mAP (csrc/det_eval.hip, driven by d3net_amd.evaluator.DetectionEvaluator) --------------------------------------
 * d3_det_match: per validation batch, one workgroup per scene, in place of the list building of lib/det/ap_helper.py:80-150
 *   (parse_predictions after its NMS), :152-193 (parse_groundtruths) and the IoU walk of lib/det/eval_det.py:113-136.
 *   pred_corners (B,K,8,3) float32; pred_cls (B,K) int32 already mapped (sem - 2, negative -> 17); scores (B,K) float32; pick (B,K)
 *   float32, the NMS mask; gt_corners (B,G,8,3) float32, gt_mask (B,G) float32 (== 1: valid), gt_cls (B,G) int32; thresholds:
 *   T doubles in HOST memory.  A detection is kept when pick == 1 && score > (float)conf_thresh && 0 <= class < num_class
 *   (float32, as numpy compares a float32 score with a Python float).  Per slot (B,K): kept 0/1, cls_out (-1 when not kept), score_out, ovmax float64 (box_util.py:97-121 box3d_iou in float64, -inf when no
 *   valid GT box of the class), jmax (lowest j on equal IoU, -1), tp_bits (bit q: true positive at thresholds[q]; see the order-free
 *   rule in det_eval.hip: exactly eval_det_cls's result with the detections of a class taken in descending score, exact ties
 *   by scene then proposal index).  gt_count (B,num_class) int32 valid GT boxes per class.  *status (device int32) is OR-ed with
 *   1 when a kept detection or a valid GT box holds a non-finite coordinate, 2 when a valid GT box's class is outside
 *   [0, num_class) (that box is skipped); the caller zeroes it.
 *   K > 256, G > 256, T outside [1, 4], B < 1 or num_class > 256: D3_ERR_RANGE before any launch.
 * d3_det_ap: the epoch-end pass of eval_det.py:148-156 and voc_ap :21-52 (use_07_metric=False), one workgroup per (class,
 *   threshold).  tp_sorted (N) int32: the tp_bits of the kept records ordered by class, then descending score, then record order;
 *   seg_offsets (num_class + 1) int32: class c owns [seg_offsets[c], seg_offsets[c+1]); gt_count (S,num_class) int32 of all S scenes.
 *   table (T,num_class,4) float64 = [AP, last recall (0 without detections), detections, present (any GT or any detection)].
 *   T outside [1, 4] or num_class > 256: D3_ERR_RANGE before any launch. */
int d3_det_match(const float *pred_corners, const int *pred_cls, const float *scores, const float *pick, double conf_thresh,
                 const float *gt_corners, const float *gt_mask, const int *gt_cls, int B, int K, int G, int num_class,
                 const double *thresholds, int T, int *kept, int *cls_out, float *score_out, double *ovmax, int *jmax, int *tp_bits,
                 int *gt_count, int *status, void *stream);
int d3_det_ap(const int *tp_sorted, const int *seg_offsets, const int *gt_count, int S, long long N, int num_class, int T,
              double *table, void *stream);

/* ---- captioning validation (csrc/caption_eval.hip, driven by d3net_amd.caption_eval.CaptionEvaluator) -----------------------
 * d3_caption_collect: per validation batch, in place of the B x G loop of lib/captioning/eval_helper.py:102-307
 *   (assign_dense_caption after its Hungarian step, and the `candidates.setdefault` merge of the epoch).  All pointers are device
 *   memory.  per_gt (B,G) int32 as d3_dense_caption_assign leaves it; pred_boxes (B,K,8,3), gt_boxes (B,G,8,3) float32; gt_mask
 *   (B,G) int32 (!= 0: a GT box); gt_obj_ids (B,G) int64; lang_cap (B,K,T) int64 token ids, T <= 62; lut (V) int32: the canonical
 *   id of a vocabulary id, -1 where the vocabulary has none; scene_idx (B) int32 scene of the corpus, -1: none; slot_of
 *   (n_scenes,n_obj) int32 corpus slot of (scene, object id), -1: none; assign_status: NULL or (B) int32, the assignment's status.
 *   State, sized by the corpus (S slots): owner (S) uint64, all ones = unowned; cap (S,64) int32; cap_len (S) int32; iou (S)
 *   float32; scene_seen (n_scenes) int32; *status int32.  A GT slot (b,g) with mask != 0 marks its scene seen and claims its
 *   corpus slot with prio = batch_seq * 2^20 + (2^20 - 1 - (b*G + g)) by integer atomicMin: the first batch wins, within a batch
 *   the last (b,g).  The winner writes iou = bbox.py:273-305 box3d_iou of (pred_boxes[b, per_gt[b,g]], gt_boxes[b,g]) in float32,
 *   torch's operation order, and cap = [sos] + lut[tokens] up to and including the first eos (eos appended when absent), as
 *   decode_caption builds it.  *status is OR-ed with 1 when a winner's caption holds a token outside the vocabulary before its
 *   eos, 2 / 4 when assign_status holds a 1 / 2.  Two launches, nothing read back.
 *   T > 62, B*G > 2^20 or batch_seq outside [0, 2^43): D3_ERR_RANGE before any launch.
 * d3_caption_stats: the counting halves of lib/capeval/bleu/bleu_scorer.py (cook_refs, cook_test, "closest" reference length)
 *   and lib/capeval/rouge/rouge.py (my_lcs), one workgroup per entry.  Entry e = candidate cand[e, :clen[e]] (E,ldc) int32
 *   against the corpus rows slot_row[u_off[e] .. u_off[e+1]) of tokens (R,ldt) / lens (R) (the layout d3_cider_scores reads
 *   with U = E); sentences are cut at 64 tokens, ids < 65535.  stats (E,6) int32 = clipped n-gram matches of order 1..4, the
 *   candidate length, the closest reference length (the shorter on equal distance); lcs (SR) int32 = LCS length of the entry's
 *   candidate with each of its rows, in slot_row order.  Integers only: the scores are formed on the host. */
int d3_caption_collect(const int *per_gt, const float *pred_boxes, const float *gt_boxes, const int *gt_mask,
                       const long long *gt_obj_ids, const long long *lang_cap, const int *lut, const int *scene_idx,
                       const int *slot_of, const int *assign_status, int B, int K, int G, int T, int V, int n_scenes, int n_obj,
                       int S, int sos, int eos, long long batch_seq, unsigned long long *owner, int *cap, int *cap_len,
                       float *iou, int *scene_seen, int *status, void *stream);
int d3_caption_stats(const int *cand, int ldc, const int *clen, const int *tokens, int ldt, const int *lens,
                     const int *slot_row, const int *u_off, int E, int *stats, int *lcs, void *stream);

/* ---- grounding validation (csrc/grounding_eval.hip, driven by d3net_amd.grounding_eval.GroundingEvaluator) ------------------
 * d3_ground_eval_batch: per validation batch, one launch, one wave per description row, in place of lib/grounding/eval_helper.py:28-137
 *   (get_eval) and the per-batch appends of scripts/eval.py:197-262 (eval_grounding).  All pointers are device memory.  N = B * C rows,
 *   scene of row n = n / C.  cluster_ref, cluster_labels (N,K) float32; proposal_mask (B,K) float32 (valid: truncates to 1, the
 *   reference's `.long() == 1`); proposal_boxes (B,K,8,3), ref_boxes (N,8,3) float32 corners; unique_multiple, object_cat (N) int64;
 *   lang_scores: NULL, or (N,n_lang) float32 with lang_correct non-NULL; scene_ids (B), chunk_ids (N) int64, read only when rec_ids
 *   is given.  Per row: top = argmax(cluster_ref[n]), pred_ref = argmax(cluster_ref[n] * valid[b]) with the product formed in
 *   float32, gt_ref = argmax(cluster_labels[n]), ref_acc = cluster_labels[n, top] == 1, iou / best_iou = lib/utils/bbox.py:221-244
 *   get_aabb3d_iou of proposal pred_ref / gt_ref of scene b with ref_boxes[n] in float32, the reference's operation order.
 *   Ties: the arg-max is torch.argmax on the CPU -- the lowest index wins among equal values, +0 == -0 (a row whose valid scores are
 *   all negative scores its lowest invalid slot, as the reference does), a NaN ranks above every number and the lowest NaN wins.
 *   table (3,2,4) int64 += per row, cell [m][o] with m = unique_multiple (0, 1, anything else -> 2), o = object_cat == 17:
 *   {rows, ref_acc, iou >= 0.25f, iou >= 0.5f}; a NaN IoU compares false.  *lang_correct (int64) += argmax(lang_scores[n]) ==
 *   object_cat[n].  Integer atomics only, at most 25 per workgroup: the sums do not depend on the order.  The caller zeroes table,
 *   lang_correct and status.  Records, each NULL or written at row row0 + n: rec_iou, rec_best_iou float32; rec_pred_ref, rec_gt_ref,
 *   rec_ref_acc int32; rec_pred_box, rec_gt_box (8,3) float32; rec_ids (2) int64 = scene_ids[b], chunk_ids[n].
 *   *status (device int32) is OR-ed with 1 when the box at pred_ref, the box at gt_ref or the GT box holds a non-finite coordinate.
 *   B < 1, C < 1, B * C >= 2^31, K outside [1, 4096] or, with lang_scores, n_lang outside [1, 64]: D3_ERR_RANGE before any launch.
 *   No workspace. */
int d3_ground_eval_batch(const float *cluster_ref, const float *cluster_labels, const float *proposal_mask,
                         const float *proposal_boxes, const float *ref_boxes, const long long *unique_multiple,
                         const long long *object_cat, const float *lang_scores, int n_lang, const long long *scene_ids,
                         const long long *chunk_ids, int B, int C, int K, long long row0, long long *table, long long *lang_correct,
                         float *rec_iou, float *rec_best_iou, int *rec_pred_ref, int *rec_gt_ref, int *rec_ref_acc,
                         float *rec_pred_box, float *rec_gt_box, long long *rec_ids, int *status, void *stream);

/* ---- leaderboard prediction writers (csrc/submission.hip, driven by d3net_amd.submission) -----------------------------------
 * All pointers are device memory; both are one launch, read nothing back and OR bits into *status (device int32, zeroed by the
 * caller), on which the host raises when it reads the records.
 * d3_caption_submit_batch: per test batch, after d3_nms3d_samecls, in place of the scene x proposal loop of
 *   benchmark/benchmark_captioning.py:151-188 (predict).  corners (B,K,8,3), sem_cls (B,K), scores (B,K), pick (B,K) float32 (pick
 *   == 1: kept by the NMS; no confidence threshold, as the reference); lang_cap (B,K,T) int64; ids (B) int64 dataset indices;
 *   scene_of_id (D) int32: the scene slot of chunked_data[id][0]["scene_id"], -1: none.  State of S scene slots with room for Kcap
 *   records of Tcap tokens each: rec_box (S,Kcap,8,3) float32, rec_cls (S,Kcap) int32 = the one-hot position of sem_prob (sem - 2,
 *   negative -> 17, truncated), rec_score (S,Kcap) float32, rec_ntok (S,Kcap) int32, rec_tok (S,Kcap,Tcap) int32, count (S) int32
 *   records of the scene, first_seen (S) int64 = batch_seq * 2^20 + row of the scene's first appearance, negative: never seen (the
 *   caller fills it with -1).  One workgroup per row compacts the kept slots in slot order; rec_ntok = position of the first eos
 *   + 1, or T without one (decode_caption's cut; "sos" and a missing "eos" are the host's).  Of several rows of one batch that
 *   name the same scene the LAST writes the records and the count (`results[scene_id] = ...`), first_seen is the first such row's
 *   and is written only while unset, the others return; stream order serialises the batches.
 *   *status |= 1: a token outside [0, V) before a kept caption's cut; 2: a kept slot's class outside [0, 18); 4: an id outside
 *   [0, D) or without a scene slot in [0, S) (that row writes nothing).
 *   B outside [1, 2^20], K outside [1, 256], T outside [1, 62], Kcap < K, Tcap < T or batch_seq outside [0, 2^43): D3_ERR_RANGE
 *   before any launch.
 * d3_ground_submit_batch: per test batch, one wave per description row, in place of benchmark/benchmark_grounding.py:122-180
 *   (predict).  N = B * C rows, scene of row n = n / C.  cluster_ref (N,K) float32; proposal_boxes (B,K,8,3) float32;
 *   unique_multiple, object_cat, chunk_ids (N) int64; ids (B) int64; key_of (D,Cmax) int32: the number of the annotation's
 *   "scene-object-ann" string (equal strings, equal numbers), -1: no such annotation.  pred_ref = argmax(cluster_ref[n]) over ALL
 *   slots, torch.argmax's CPU rule (d3_ground_eval_batch's `top`): the reference does not mask invalid slots here.  Record at row
 *   row0 + n: rec_box (8,3) float32 the box at pred_ref of scene n / C, rec_pred_ref int32, rec_unique_multiple int64, rec_others
 *   int32 = object_cat == 17, rec_key int32, rec_keep int32 = 0 when an earlier row of THIS batch has the same key (or the key is
 *   -1), rec_ids (2) int64 = ids[n / C], chunk_ids[n].  *status |= 1: an id / chunk id outside the table or a -1 entry.
 *   B < 1, C < 1, B * C >= 2^31 or K outside [1, 4096]: D3_ERR_RANGE before any launch.  No workspace. */
int d3_caption_submit_batch(const float *corners, const float *sem_cls, const float *scores, const float *pick,
                            const long long *lang_cap, const long long *ids, const int *scene_of_id, int D, int B, int K, int T,
                            int V, int eos, long long batch_seq, int S, int Kcap, int Tcap, float *rec_box, int *rec_cls,
                            float *rec_score, int *rec_ntok, int *rec_tok, int *count, long long *first_seen, int *status,
                            void *stream);
int d3_ground_submit_batch(const float *cluster_ref, const float *proposal_boxes, const long long *unique_multiple,
                           const long long *object_cat, const long long *ids, const long long *chunk_ids, const int *key_of, int D,
                           int Cmax, int B, int C, int K, long long row0, float *rec_box, int *rec_pred_ref,
                           long long *rec_unique_multiple, int *rec_others, int *rec_key, int *rec_keep, long long *rec_ids,
                           int *status, void *stream);

/* ---- PointGroup scene preparation (csrc/scene_prep.hip, driven by d3net_amd/scene_prep.py) ----------------------------------
 * One scene of n points: xyz (n,3) float32, ids / sem (n) int32 (ids -1 = none).  Coordinates are fp64 (numpy's float32 @ float64
 * promotion) unless fp32 != 0 (the validation path, float32 throughout like the reference's `points.copy() * scale`).
 * Sizes beyond d3_scene_limits (points, elements per noise grid, largest instance id) return D3_ERR_RANGE before any launch. */
int d3_scene_limits(int *max_points, int *max_grid, int *max_id);
/* lib/dataset/pipeline.py:145-146 + :679-697 (_augment): y = xyz @ m (m_host: 9 doubles, host memory), s = y * scale. */
int d3_scene_transform(const float *xyz, int n, const double *m_host, double scale, int fp32, double *y, double *s, void *stream);
/* stats (12 u64, device): order-preserving encodings of |s| max, min, max per axis (lib/utils/transform.py:elastic `bb`,
 * pipeline.py:155 offset, lib/utils/pc.py:38 pc_range) and ids min / max + 2^31 (ids may be NULL). */
int d3_scene_reduce(const double *s, const int *ids, int n, unsigned long long *stats, void *stream);
/* transform.py:elastic noise, device mode: count N(0,1) float32 values from Philox4x32-10 (key = seed) + Box-Muller. */
int d3_scene_noise(float *grid, long long count, unsigned long long seed, void *stream);
/* transform.py:elastic: grids = 3 noise grids (X,Y,Z) float32, contiguous, blurred in place by the six scipy.ndimage.convolve
 * passes; axes = the X + Y + Z np.linspace node values; then s += RegularGridInterpolator(...)(s) * mag (fill 0 outside).
 * ws: d3_scene_elastic_ws_bytes(X, Y, Z) (0: grid outside the limits). */
size_t d3_scene_elastic_ws_bytes(int X, int Y, int Z);
int d3_scene_elastic(double *s, int n, float *grids, const double *axes, int X, int Y, int Z, double mag, void *ws, size_t ws_bytes,
                     void *stream);
/* pipeline.py:155 `points -= points.min(0)` with the min of `stats` (d3_scene_reduce). */
int d3_scene_offset(double *s, int n, const unsigned long long *stats, int fp32, void *stream);
/* pc.py:crop :40-42 for one candidate: flags[i] = all(s + off >= 0) and all(s + off < range); *count (device) = sum(flags).
 * off_host / range_host: 3 doubles each, host memory.  The host runs the reference's while loop on the counts. */
int d3_scene_crop_count(const double *s, int n, const double *off_host, const double *range_host, int *flags, int *count,
                        void *stream);
/* workspace of d3_scene_emit / d3_scene_relabel / d3_scene_instances for n points and ids <= max_id (0: outside the limits) */
size_t d3_scene_ws_bytes(int n, int max_id);
/* pipeline.py:160-164 (+ :182-186 casts): stable order-preserving compaction of the points with flags[i] != 0 (flags NULL: all);
 * locs = (float)y, locs_scaled = (float)(s + off) (off_host NULL: 0), y_out = y, feats (n,C) rows, sem, ids. */
int d3_scene_emit(const double *y, const double *s, const float *feats, int C, const int *sem, const int *ids, int n,
                  const int *flags, const double *off_host, int fp32, double *y_out, float *locs, float *locs_scaled,
                  float *feats_out, int *sem_out, int *ids_out, void *ws, size_t ws_bytes, void *stream);
/* pipeline.py:699-709 (_croppedInstanceIds) in place, from the id-presence table of ids in [-1, max_id]. */
int d3_scene_relabel(int *ids, int n, int max_id, void *ws, size_t ws_bytes, void *stream);
/* pipeline.py:711-772 (_getInstanceInfo) and :804-833 (_generate_gt_clusters) over ids in np.unique order (ids in [-1, max_id]):
 *   info (n,12) float32 = mean, (min+max)/2, min, max of y per instance (zeros when unlabelled);
 *   num_point[r], gt_off[r] (r < K) and gt_off[K]; gt_idx (L,2) = [cid, point], ascending point index inside an instance;
 *   boxes (R,36) float64 rows = [center 3, size 3, class, id, label, size residual 3, 8 corners x 3] (zero-filled by the caller),
 *     with the reference's slot -1 / k >= 128 quirks; class = sem of the lowest-index point, c - 2 if c >= 2 else 17;
 *     residual = size - mean_size (18,3) float64 device;
 *   counts (4 int, device) = [K instances, L labelled points, has unlabelled points, 0].  Deterministic (no float atomics). */
int d3_scene_instances(const double *y, const int *ids, const int *sem, int n, int max_id, int fp32, int R, const double *mean_size,
                       float *info, int *num_point, int *gt_idx, int *gt_off, double *boxes, int *counts, void *ws,
                       size_t ws_bytes, void *stream);

/* ---- description batches (csrc/lang_prep.hip, driven by d3net_amd/lang_prep.py) ------------------------------------------------
 * The description half of PipelineDataset.__getitem__ (lib/dataset/pipeline.py:69-138, :250-318) from device-resident tables:
 * tokens (Nd,L) int32 = the sos / eos-wrapped, trimmed token ids of every description (_tranform_des, :504-552, ids only), zero
 * padded; lens (Nd) int32 = min(len(token) + 2, L) (:104-105); glove (V,D) float32.
 * d3_lang_features, over S = B * C slots (replaces the (L,300) float64 arrays of :531-549, the deepcopy of :103, the erase of
 * :554-565, the stores of :133-135, the casts of :301-303 and the stacking of scannet_collate_fn):
 *   rows_host (S): description of each slot, -1 = SYNTHETIC (all zeros, lang_len 0, :121-124); erase_ptr_host (S+1) /
 *   erase_pos_host: CSR list of each slot's erased positions; all three in HOST memory, copied into ws on the stream by the
 *   call (keep them valid until that copy has run; for pageable memory that is before the call returns).
 *   lang_feat (S,L,D): position p < lens[row] = glove[tokens[row,p]], an erased position = glove[unk], every other exactly 0;
 *   lang_ids (S,L) int64 (never erased), lang_len (S) int64.  One launch, 16-byte accesses, flat over (slot, position, quad).
 *   D % 4 != 0, unk outside [0,V) or an erase position outside [0,L): D3_ERR_ARG; a row outside [-1,Nd): D3_ERR_RANGE; all
 *   checked on the host before any copy or launch.  Token ids are the caller's to check against V (DescriptionIndex does).
 *   ws: d3_lang_features_ws_bytes(S, E), E = erase_ptr_host[S] (0: outside the limits). */
size_t d3_lang_features_ws_bytes(int S, int E);
int d3_lang_features(const int *tokens, const int *lens, int Nd, const float *glove, int V, int D, int L, int unk,
                     const int *rows_host, const int *erase_ptr_host, const int *erase_pos_host, int S, float *lang_feat,
                     long long *lang_ids, long long *lang_len, void *ws, size_t ws_bytes, void *stream);
/* d3_ref_targets (pipeline.py:250-278) from the stacked gt_bbox_object_id / gt_bbox_label (B,R) int64, gt_bbox (B,R,8,3) float32 and
 * object_id (B,C) int64:
 *   ref_label (B,C,R) int64: 1 where gt_label == 1 and the id equals the slot's object id; ref_corner (B,C,8,3): gt_bbox of the
 *   highest matching row (get_3d_box without heading == get_3d_box_batch with heading 0, bit for bit), zeros when none matches;
 *   rots (B,R,3,3) float32 / rot_masks (B,R) int64: the Scan2CAD matrix of a row with gt_label == 1 whose id is in its scene's
 *   table, else zeros.  Table: rot_off (Ns+1), rot_ids (T) int32, rot_mats (T,3,3) float32 on the device (NULL when Ns == 0);
 *   scene_host (B), HOST memory: each scene's table index, -1 = none; outside [-1,Ns): D3_ERR_RANGE before any launch.
 *   One wave per (scene, slot) and per (scene, row), plain stores.  ws: d3_ref_targets_ws_bytes(B). */
size_t d3_ref_targets_ws_bytes(int B);
int d3_ref_targets(const long long *gt_ids, const long long *gt_label, const float *gt_bbox, const long long *object_id, int B, int C,
                   int R, const int *rot_off, const int *rot_ids, const float *rot_mats, int Ns, const int *scene_host,
                   long long *ref_label, float *ref_corner, float *rots, long long *rot_masks, void *ws, size_t ws_bytes, void *stream);

/* ---- batch stacking (csrc/collate.hip, driven by d3net_amd/scene_prep.py:collate_scenes_device) -------------------------------
 * lib/dataset/pipeline.py:917- (sparse_collate_fn) over B per-scene samples that are already on the device, in ONE launch.
 *   ptrs_host (B,18), HOST memory: per scene the device pointers of locs (n,3) f32, locs_scaled (n,3) f32, feats (n,C) f32,
 *     sem_labels (n) i32, instance_ids (n) i32, instance_info (n,12) f32, instance_num_point (K) i32, gt_proposals_idx (Lp,2) i32,
 *     gt_proposals_offset (K+1) i32 (the last two read only when has_gt), then the nine box labels of R rows: center_label (R,3)
 *     f32, sem_cls_label (R) i64, heading_class_label (R) i64, heading_residual_label (R) f32, size_class_label (R) i64,
 *     size_residual_label (R,3) f32, gt_bbox_object_id (R) i64, gt_bbox_label (R) i64, gt_bbox (R,8,3) f32; all contiguous.
 *   counts_host (B,3), HOST memory: n points, K instances, Lp proposal entries per scene.
 *   out_host (20), HOST memory: the device pointers of the stacked outputs, N / I / L the sums of n / K / Lp: locs (N,3) f32,
 *     locs_scaled (N,4) i64 = [scene index, (int64) of each coordinate], feats (N,C) f32, sem_labels (N) i64, instance_ids (N) i64
 *     (ids other than -1 shifted by the instances of the scenes before), instance_info (N,12) f32, instance_num_point (I) i32,
 *     gt_proposals_idx (L,2) i32 (column 0 shifted by the instances, column 1 by the points before), gt_proposals_offset (I+1) i32
 *     (each scene's leading 0 dropped after the first, shifted by the entries before), batch_offsets (B+1) i32, instance_offsets
 *     (B+1) i32, then the nine box labels stacked to (B,R,...).  Outputs 7 and 8 may be NULL when has_gt == 0.
 *   table_host: d3_collate_table_bytes(B) bytes of (pinned) HOST memory the call fills with its job list, tile prefix and offset
 *     tables and copies to table_dev (as many device bytes) with ONE asynchronous copy on the stream: keep it unchanged until that
 *     copy has run.  One kernel: a block finds its job by binary search in the prefix table held in LDS; 16-byte accesses where
 *     source and destination are 16-byte aligned, lane-consecutive words otherwise; plain stores, one writer per element.
 *   B outside [1, 512] or sums outside int32: D3_ERR_RANGE (d3_collate_table_bytes: 0); a NULL pointer with a non-zero count, a
 *   negative count or a misaligned int64 output: D3_ERR_ARG; all checked on the host before any copy or launch. */
size_t d3_collate_table_bytes(int B);
int d3_collate_scenes(const void *const *ptrs_host, const int *counts_host, int B, int C, int R, int has_gt, void *const *out_host,
                      void *table_host, void *table_dev, size_t table_bytes, void *stream);

/* ---- a batch straight from the resident scene store (csrc/batch_prep.hip, driven by d3net_amd/scene_prep.py:prepare_batch_store)
 * What d3_scene_transform ... d3_scene_instances per scene and d3_collate_scenes per batch compute on the path WITHOUT elastic
 * distortion and crop (every scene keeps all its points), bit for bit, in ONE copy and THREE launches whatever B is, with no
 * read-back: everything that depends only on a scene's instance_ids / sem_labels comes from the store's instance index.
 *   xyz (S,3) f32, feats (S,C) f32, sem / ids (S) i32: the store's packed arrays of S rows (device), read only.
 *   ix_hist / ix_rank / ix_start (T) i32: per scene V + 1 entries from its table offset, V = max(largest id, 0) + 1: hist[0] the
 *     unlabelled points and hist[v + 1] those with id v; rank[v] / start[v] the exclusive scans of presence / count (np.unique
 *     order, first row in the proposal list).  ix_sorted (S) i32, per scene from its row offset: scene-local point indices
 *     grouped by instance in np.unique order, ascending inside each, unlabelled points last.  All read only.
 *   row0_host (B) i64, HOST: each slot's first store row.  slots_host (B,6) i32, HOST: n points, table offset, V, K instances,
 *     Lp labelled points, has-unlabelled flag.  One scene may fill several slots.  mats_host (B,9) f64, HOST: each slot's
 *     augmentation matrix; read when fp32 == 0 (fp32 != 0: the float32 validation path, y = xyz).
 *   mean_size (18,3) f64 device.  out_host (20), HOST: the device pointers of d3_collate_scenes' outputs, in its order and with
 *     its shapes and dtypes for N / I / L the sums of n / K / Lp (7 and 8 may be NULL when has_gt == 0, and so may an output without elements); none needs zeroing.
 *   table_host: d3_batch_prepare_table_bytes(B) bytes of (pinned) HOST memory the call fills -- per slot the offsets, counts,
 *     matrix and running point / instance / proposal-entry totals, the three stages' tile-prefix tables, and the start values of
 *     the per-slot minima -- and copies into ws with ONE asynchronous copy: keep it unchanged until that copy has run.
 *   ws: d3_batch_prepare_ws_bytes(B, sum of V) device bytes: the table's copy and 9 doubles per (slot, id value).
 * Stages, each a flat grid whose blocks find their (slot, tile) by binary search of the prefix table in LDS:
 *   1 transform + feature rows: s = (xyz @ M) * scale per point, the per-slot minimum by integer atomics on the order-preserving
 *     encoding; the feature rows copied once, store to batch, 16-byte accesses where both ends are 16-byte aligned;
 *   2 one wave per (slot, id value): count, exact min / max, the sum sequential over ascending point index (float when fp32,
 *     else double) -> instance_num_point, gt_proposals_offset, the instance's row of the nine box labels (the slot -1 / k >= 128 /
 *     k >= R rules of d3_scene_instances); rows no instance owns are written as zeros, and the two offset tables;
 *   3 per point locs, locs_scaled [slot, (int64) s - min], sem_labels, instance_ids (+ instances before unless -1),
 *     instance_info; per labelled point its gt_proposals_idx row with both shifts.
 * One writer per output element; no floating-point atomics.  y and s are recomputed where they are used, not stored.
 *   B outside [1, 512], a slot beyond d3_scene_limits, or a total outside int32: D3_ERR_RANGE (d3_batch_prepare_table_bytes: 0);
 *   a slot outside the store (store_rows) or the index tables (table_len), K > V, Lp > n, a NULL or misaligned pointer:
 *   D3_ERR_ARG; all checked on the host before anything is queued. */
size_t d3_batch_prepare_table_bytes(int B);
size_t d3_batch_prepare_ws_bytes(int B, long long v_total);
int d3_batch_prepare(const float *xyz, const float *feats, const int *sem, const int *ids, long long store_rows,
                     const int *ix_hist, const int *ix_rank, const int *ix_start, const int *ix_sorted, long long table_len,
                     const long long *row0_host, const int *slots_host, const double *mats_host, int B, int C, int R, int fp32,
                     int has_gt, double scale, const double *mean_size, void *const *out_host, void *table_host, void *ws,
                     size_t ws_bytes, void *stream);

/* ---- the label-free scene half of a test-split batch (csrc/batch_prep.hip, driven by d3net_amd/scene_prep.py:prepare_points_store
 * and d3net_amd/dataset.py:SceneStore.extents) ----
 * lib/dataset/pipeline.py:352-380 (the `else:` branch of __getitem__: points * scale, minus points.min(0), no label read) and
 * :937-976 (sparse_collate_fn's label-free half).  Nothing is drawn and no point is dropped there, so the per-scene minimum of
 * fl32(x * scale) is a constant of the (store, scale) pair and the batch is a row-wise map of the store's rows.
 *
 * d3_store_extents (lib/dataset/pipeline.py:352-380, `points -= points.min(0)`): ONE launch over all S scenes of a store.
 *   xyz (store_rows,3) f32 device, read only.  offsets_host (S+1) i64, HOST: the scenes' row offsets.
 *   extents (S,3) u64 device, 8-byte aligned: per scene and axis the ORDER-PRESERVING ENCODING (csrc/scene_prep.h:sp_enc; the host
 *     decodes it with scene_prep._decode) of min over the scene's points of (double)fl32(x * fl32(scale)); the call presets it
 *     to ~0 itself.  The table stays encoded: d3_points_batch decodes it where it reads it, as stage 3 of d3_batch_prepare does.
 *   table_host: d3_store_extents_table_bytes(S) bytes of (pinned) HOST memory the call fills (row offset, count, tile prefix) and
 *     copies into ws (d3_store_extents_ws_bytes(S) device bytes) with ONE asynchronous copy: keep it until that copy has run.
 *   A block finds its (scene, tile) by binary search of the tile-prefix table in LDS, reduces in the wave, then in the block, and
 *   combines blocks by the integer atomicMin on the encoding (deterministic).
 *   S outside [1, 8192], a scene without points or beyond d3_scene_limits, tiles outside int32: D3_ERR_RANGE (the size queries:
 *   0); a NULL or misaligned pointer, offsets outside [0, store_rows]: D3_ERR_ARG; all checked before anything is queued. */
size_t d3_store_extents_table_bytes(int S);
size_t d3_store_extents_ws_bytes(int S);
int d3_store_extents(const float *xyz, long long store_rows, const long long *offsets_host, int S, double scale,
                     unsigned long long *extents, void *table_host, void *ws, size_t ws_bytes, void *stream);
/* d3_points_batch (lib/dataset/pipeline.py:352-380 per sample, :937-976 stacked): ONE copy and ONE launch per batch.
 *   xyz (store_rows,3) f32, feats (store_rows,C) f32: the store's packed arrays (device), read only.  extents (S,3) u64: the
 *   table d3_store_extents wrote for the same store and scale.  row0_host (B) i64, srow_host (B) i32, n_host (B) i32, HOST: per
 *   slot its first store row, its scene's row of `extents` and its point count; one scene may fill several slots.
 *   Outputs (device), N the sum of n: locs (N,3) f32 = the store's xyz; locs_scaled (N,4) i64, 16-byte aligned = [slot, (int64)
 *   (float) of fl32(fl32(x * fl32(scale)) - min) per axis] -- d3_batch_prepare's fp32 expressions, so the same bits; out_feats
 *   (N,C) f32 (16-byte accesses where both ends are 16-byte aligned, lane-consecutive words otherwise); batch_offsets (B+1) i32,
 *   written inside the same launch by one designated thread per slot.  None needs zeroing; one writer per element, plain stores,
 *   no workspace reduction, no atomics, no read-back.
 *   table_host: d3_points_batch_table_bytes(B) bytes of (pinned) HOST memory the call fills (slots, tile prefix) and copies into
 *   ws (d3_points_batch_ws_bytes(B) device bytes) with ONE asynchronous copy: keep it unchanged until that copy has run.
 *   B outside [1, 512], C outside [0, 256], n outside [1, d3_scene_limits' points] (an empty slot: points.min(0) raises in the
 *   reference), a total outside int32: D3_ERR_RANGE (the size queries: 0); a NULL or misaligned pointer, a slot outside the store
 *   or the extents table: D3_ERR_ARG; all checked on the host before anything is queued. */
size_t d3_points_batch_table_bytes(int B);
size_t d3_points_batch_ws_bytes(int B);
int d3_points_batch(const float *xyz, const float *feats, long long store_rows, const unsigned long long *extents, int S,
                    const long long *row0_host, const int *srow_host, const int *n_host, int B, int C, double scale,
                    float *locs, long long *locs_scaled, float *out_feats, int *batch_offsets, void *table_host, void *ws,
                    size_t ws_bytes, void *stream);

/* ---- the augmented detector-only batch from the resident scene store (csrc/batch_elastic.hip, driven by
 * d3net_amd/scene_prep.py:prepare_batch_store_elastic) ----
 * lib/dataset/pipeline.py:145-164 (`_augment`, the two `elastic` calls of lib/utils/transform.py, `points -= points.min(0)`,
 * lib/utils/pc.py:crop, `_croppedInstanceIds` :699-709), then :711-772 / :804-833 and sparse_collate_fn's stacking: what
 * d3_scene_transform ... d3_scene_instances compute per scene WITH elastic distortion and crop and d3_collate_scenes then stacks,
 * bit for bit, in a number of copies and launches that depends neither on B, nor on the scenes' sizes, nor on the crop iterations
 * any slot runs, and with no read-back inside the call: `readback` is for the caller to fetch once, afterwards.
 *   xyz / feats / sem / ids, store_rows, row0_host, mats_host, mean_size, out_host: as for d3_batch_prepare, except that every
 *     output is allocated at its upper bound -- N = sum of n point rows, sum of V instances (+ 1 offsets), N proposal rows -- and
 *     the leading kept rows / K instances / Lp entries are written.
 *   slots_host (B,8) i32, HOST: n points (>= 1), V = max(largest id, 0) + 1, and the caller's UPPER BOUND of the two noise-grid
 *     shapes (3 + 3 ints, each in [3, 2048], at most 2^25 cells): the workspace regions are sized by it, the real shape
 *     `int32(|s| max) // gran + 3` is taken on the device from the reduction and clamped to it.
 *   seeds_host (B) u64, HOST: elastic e of a slot draws d3_scene_noise's stream with key (seed << 1) | e, counter = element index
 *     in the slot's real (3, X, Y, Z) layout.  crop_u_host (B,T,3) f64, HOST: the crop loop's draws, one row per iteration.
 *   T: the bound of pc.py:crop's loop, ceil(crop_scale / 32) + 1 (1 .. 80); gran0 / gran1, mag0 / mag1: the two elastic calls'
 *     granularity and magnitude; crop_scale: data.full_scale[1]; max_num_point: data.max_num_point.
 *   readback (B,10) i32 DEVICE: per slot kept points, K, Lp, the two real grid shapes as computed (a value above the bound means
 *     the bound was wrong and the batch is void) and the crop iterations run.
 *   table_host: d3_batch_elastic_table_bytes(B, T) bytes of (pinned) HOST memory the call fills and copies into ws with ONE
 *     asynchronous copy: keep it unchanged until that copy has run.  ws: d3_batch_elastic_ws_bytes(slots_host, B, C, T) bytes.
 * Stages: transform (y, s float64 kept; per-slot |s| max) -- twice: resolve the grid shape and axes, noise, six 3-tap passes,
 * interpolation (+ the next reduction) -- offset -- T crop launches (a finished slot's blocks exit) -- scan + emit (stable
 * compaction over all slots) + feature rows -- presence, relabel walk (one thread per slot), apply + hist -- rank / start / totals
 * (one block) -- keys, one stable sort over (slot, rank) -- one wave per (slot, id value) -- unowned box rows -- info / proposal rows.
 * Integer atomics only (encoded min / max, counts); per-instance sums sequential over ascending point index.
 *   B outside [1, 512], T outside [1, 80], a slot without points or beyond d3_scene_limits, a bound outside the grid limits, a
 *   total outside int32: D3_ERR_RANGE (the size queries: 0); a NULL or misaligned pointer, a slot outside the store: D3_ERR_ARG;
 *   all checked on the host before anything is queued. */
size_t d3_batch_elastic_table_bytes(int B, int T);
size_t d3_batch_elastic_ws_bytes(const int *slots_host, int B, int C, int T);
int d3_batch_elastic(const float *xyz, const float *feats, const int *sem, const int *ids, long long store_rows,
                     const long long *row0_host, const int *slots_host, const double *mats_host, const unsigned long long *seeds_host,
                     const double *crop_u_host, int B, int C, int R, int T, int has_gt, double scale, int gran0, int gran1,
                     double mag0, double mag1, double crop_scale, int max_num_point, const double *mean_size, void *const *out_host,
                     int *readback, void *table_host, void *ws, size_t ws_bytes, void *stream);

/* ---- multiview feature projection (csrc/multiview.hip, driven by d3net_amd/multiview.py) --------------------------------------
 * The reference's ProjectionHelper.compute_projection / project (lib/utils/projection.py:180-256) and the per-scene loop of
 * data/scannet/project_multiview_features.py:88-205.  One scene: points (N,3) float32 mesh vertices; F frames in the caller's order:
 * depths (F,H,W) float32 metres, c2w / w2c (F,4,4) float32 camera_to_world and its inverse (the caller's torch.inverse);
 * intr_host: 7 doubles, host memory = fx, fy, cx, cy, depth_min, depth_max, accuracy (the image corners are unprojected from them
 * in double and stored as float32, like projection.py:18-45).  Frustum, projection and depth test are float32 in a fixed order.
 * N, F, W * H beyond d3_multiview_limits return D3_ERR_RANGE before any launch. */
int d3_multiview_limits(int *max_points, int *max_frames, int *max_pixels);
/* compute_projection for F frames at once: idx3d / idx2d (F, N+1) int64, row f = [count, point ids ascending..., 0...] /
 * [count, pixel v * W + u..., 0...] (zero-filled here).  N * F must stay below 2^31 (else D3_ERR_RANGE);
 * ws: d3_multiview_project_ws_bytes(N, F) (0: outside the limits). */
size_t d3_multiview_project_ws_bytes(int N, int F);
int d3_multiview_project(const float *points, int N, const float *depths, const float *c2w, const float *w2c, int F,
                         const double *intr_host, int W, int H, long long *idx3d, long long *idx2d, void *ws, size_t ws_bytes,
                         void *stream);
/* ProjectionHelper.project for one frame: out (C, N) = 0, then out[:, idx3d[1+j]] = label[:, idx2d[1+j]] for j < idx3d[0] (read
 * on the device); label (C, HW) float32.  Indices outside [0, N) / [0, HW) are skipped. */
int d3_multiview_project_frame(const float *label, int C, int HW, const long long *idx3d, const long long *idx2d, int N, float *out,
                               void *stream);
/* The fused scene: feats (F, C, H, W) float32 ENet maps, C == 128 (the reference's emptiness test hard-codes 128; else
 * D3_ERR_ARG) -> out (N, 128) float32, fused over the frames with at least one mapped point, in order
 * (project_multiview_features.py:170-200): maxpool != 0: a non-empty projection fills an empty row and max-pools a filled one;
 * maxpool == 0: an empty row takes the frame's projection (zeros for an unmapped point).  "Empty" = all 128 values == 0.
 * frame_counts (F int32, device; may be NULL) = mapped points per frame.  Bitwise deterministic (no float atomics).
 * ws: d3_multiview_fuse_ws_bytes(F, W, H) (0: outside the limits). */
size_t d3_multiview_fuse_ws_bytes(int F, int W, int H);
int d3_multiview_fuse(const float *points, int N, const float *depths, const float *c2w, const float *w2c, int F,
                      const double *intr_host, int W, int H, const float *feats, int C, int maxpool, float *out, int *frame_counts,
                      void *ws, size_t ws_bytes, void *stream);

/* ---- ENet frame features (csrc/enet.hip, driven by d3net_amd/enet.py) ---------------------------------------------------------
 * Replaces data/scannet/compute_multiview_features.py:53-73 (EnetDataset._resize_crop_image / _load_image: PIL NEAREST resize to
 * height 256, CenterCrop to 256 x 328, x / 255, Normalize) and :77-96 (Sequential(enet_fixed, enet_trainable) of
 * model/enet.py:697-715 create_enet_for_3d, elements 0-25 of create_enet(41) at :130-695, in eval mode).  Inference only.
 * d3_enet_layers: the 67 convolution rows (initial block, then conv a / b / c of blocks 4-25), 7 ints each = cin, cout, kh, kw,
 * stride, pad, dilation (the asymmetric 1x5 + 5x1 pair is one folded 5x5 row); table == NULL: only the count, cap too small:
 * D3_ERR_ARG.  d3_enet_param_count: floats of the folded parameter blob, laid out per row in that order, every segment padded to
 * a multiple of 4 floats: the initial block = W (13,3,3,3), bias 13, pool scale 3, pool shift 3, PReLU 16; a convolution =
 * W (kh*kw, cout, cin), bias cout, PReLU cout (conv c: the block's output PReLU; its W and bias carry BN and the x(1 - p)). */
int d3_enet_layers(int *table, int cap);
long long d3_enet_param_count(void);
/* frames (F, H0, W0, 3) uint8 RGB -> out (F, 3, H, W) float32 = (src / 255 - mean) / std with src = frames[f, rows[y], cols[x]]
 * (rows (H), cols (W) int32 device tables, crop included; true float32 divisions).  Per-frame sizes of 2^31 elements or more or
 * F > 65535: D3_ERR_RANGE. */
int d3_enet_preprocess(const unsigned char *frames, int F, int H0, int W0, const int *rows, const int *cols, int H, int W, float *out,
                       void *stream);
/* x (F, 3, H, W) float32 -> out (F, 128, H/8, W/8) float32 (the reference's per-frame array).  params: the folded blob
 * (n_params == d3_enet_param_count()); table / n_table: the caller's copy of d3_enet_layers (any difference: D3_ERR_ARG).
 * upto = 25; 3..24 stops after that element of create_enet(41) and writes its output NHWC: (F, H/2, W/2, 16) for 3,
 * (F, H/4, W/4, 64) for 4..8, (F, H/8, W/8, 128) for 9..24 (a test hook; other values: D3_ERR_ARG).
 * H or W not a multiple of 8: D3_ERR_ARG; H * W * 4 >= 2^31 or F > 65535: D3_ERR_RANGE; all before any launch.  67 launches,
 * no host synchronisation; a frame's output is bitwise independent of F.  ws: d3_enet_ws_bytes(F, H, W) (0: invalid sizes). */
size_t d3_enet_ws_bytes(int F, int H, int W);
int d3_enet_forward(const float *x, int F, int H, int W, const float *params, long long n_params, const int *table, int n_table,
                    int upto, float *out, void *ws, size_t ws_bytes, void *stream);

/* ---- ScanNet scan export (csrc/scan_export.hip, driven by d3net_amd/scan_export.py) -----------------------------------------------
 * Replaces data/scannet/prepare_scannet.py:138-197 (export / process_one_scan) with the helpers it calls (:23-25, :29-135),
 * scannet_utils.py:21-48 / :117-136 (read_mesh_vertices_rgb_normal, compute_normal, normalize_v3) and the instance-GT body of
 * prepare_scannet_inst_gt.py:38-65.  The host parses the files and builds the object tables; everything per vertex or per face runs
 * here.  Integer atomics only: every output is bitwise reproducible.  Sizes outside d3_scan_limits return D3_ERR_RANGE and NULL or
 * misaligned pointers D3_ERR_ARG, both before any launch.  flags: device int[2], zeroed by the caller; flags[0] collects problem bits
 * of the data (1 face vertex count != 3, 2 face index outside [0, N), 4 raw label >= 150, 8 segment id outside [0, S), 16 a
 * listed segment that no vertex carries, 32 an object table entry outside its contract: pair_obj outside [0, K), obj_id outside
 * [0, R) or repeated; such entries are skipped, never used as an index), flags[1] = box rows kept by d3_scan_labels. */
int d3_scan_limits(int *max_vertices, int *max_faces, int *max_segments, int *max_objects, int *max_rows);
/* vertex_rec: N raw 16-byte PLY vertex records (float x, y, z; uchar red, green, blue, alpha), 4-byte aligned; face_rec: F raw
 * 13-byte face records (uchar count; int32 vertex_indices[3]).  mesh / aligned_mesh (N, 9) float32 = xyz, rgb, vertex normals
 * (numpy's buffered `normals[faces[:, c]] += n`: the last face per vertex and corner); aligned xyz = [x y z 1] . M^T in fp64,
 * ((x m0 + y m1) + z m2) + m3 rounded to float32 with M = align_host (host double[16], row-major), a copy when NULL.
 * ws: d3_scan_mesh_ws_bytes(N, F) (0: outside the limits). */
size_t d3_scan_mesh_ws_bytes(int N, int F);
int d3_scan_mesh(const void *vertex_rec, int N, const void *face_rec, int F, const double *align_host, float *mesh, float *aligned_mesh,
                 int *flags, void *ws, size_t ws_bytes, void *stream);
/* raw (N) uint16 nyu40 labels, seg (N) int32 segment ids in [0, S).  The aggregation as K objects in dict order (index k): P pairs
 * (pair_seg[p], pair_obj[p] = k), obj_id[k] = objectId, obj_label_seg[k] = the segment whose first vertex labels the object;
 * R = max objectId + 1.  Outputs: instance_ids / sem_labels (N) float64 (objectId of the last object listing the vertex's segment
 * or -1; remapper[raw]), inst_gt (N) int32 (the instance GT code), boxes / aligned_boxes (R, 8) float64 capacity: the first
 * flags[1] rows are get_instance_bboxes of mesh / aligned_mesh after process_one_scan's filter of labels 1, 2, 22.
 * ws: d3_scan_labels_ws_bytes(N, S, P, K, R) (0: outside the limits). */
size_t d3_scan_labels_ws_bytes(int N, int S, int P, int K, int R);
int d3_scan_labels(const unsigned short *raw, const int *seg, int N, int S, const int *pair_seg, const int *pair_obj, int P,
                   const int *obj_id, const int *obj_label_seg, int K, int R, const float *mesh, const float *aligned_mesh,
                   double *instance_ids, double *sem_labels, int *inst_gt, double *boxes, double *aligned_boxes, int *flags, void *ws,
                   size_t ws_bytes, void *stream);

/* ---- CIDEr-D reward of the self-critical speaker update (csrc/cider.hip) -----------------------------
 * Replaces lib/capeval/cider/cider_scorer.py:11-193 (precook / compute_doc_freq / counts2vec / sim) as called per RL step by
 * lib/captioning/loss_helper.py:15-96 (host python over word tuples, twice per step).  Sentences are int32 token ids (< 65535;
 * reference words outside the vocabulary get corpus-private ids): tokens (R, ldt) / lens (R) = the reference corpus.  One call
 * scores E entries: entry e = candidate cand[e, :clen[e]] ("eos" appended when absent, like the reference) against the reference
 * set ent_u[e] in [0, U); set u = corpus rows slot_row[u_off[u] .. u_off[u+1]) (SR rows in total), used by mult[u] entries (the
 * document frequency counts a set once per entry).  hash_slots: power of two >= 2 x the distinct n-grams of the used sets.
 * scores (E) float64 == Cider().compute_score per-entry scores (x10, sigma 6).  *overflow_dev != 0: a hash table overflowed or
 * nothing was written -- the caller falls back to its host scorer.  Sentences are cut at 160 tokens. */
size_t d3_cider_ws_bytes(int SR, int E, int hash_slots);
int d3_cider_scores(const int *tokens, int ldt, const int *lens, const int *slot_row, const int *u_off, const int *mult,
                    const int *ent_u, int U, int SR, const int *cand, int ldc, const int *clen, int E, int eos, double sigma,
                    int hash_slots, double *scores, int *overflow_dev, void *ws, size_t ws_bytes, void *stream);

/* ---- proposal geometry (speaker / graph heads) ------------------------------------------ */
/* Distance matrix of `_query_locals` (model/graph_module.py:184-227 == model/caption_module.py:800-842) for all
 * target proposals at once: corners (B,K,8,3), masks (B,K) -> dist (B,K,K), dist[b,t,j] as the reference's pc_dist
 * for target id t before its top-k (invalid / overlaid (IoU >= overlay_threshold) -> 1e30, self -> 0 or 1e30). */
int d3_query_locals_dist(const float *corners, const float *masks, float *dist, int B, int K, int include_self,
                         float overlay_threshold, int center_mode, void *stream);
/* mask (rows, K) = 1 at the L smallest entries of every row of dist (rows, K), ties by ascending index -- torch.topk(largest =
 * False) + scatter of ones (model/graph_module.py:218-227 / caption_module.py:833-842) in one launch. */
int d3_query_locals_mask(const float *dist, float *mask, int rows, int K, int L, void *stream);
/* The captioner's per-description inputs straight from the per-scene tensors (model/caption_module.py:416-508 `select_target`,
 * :530-560, :866-885 `_add_relation_feat`); description n belongs to scene n / per_scene.
 *   select_target: target_ids[n] = first arg-max over the scene's K proposals of the AABB IoU (lib/utils/bbox.py:247-271, fp32,
 *                  operation by operation as the library ops) between corners (B,K,8,3) and ref_corners (N,8,3); target_ious[n]
 *                  that IoU; labels[n] = first arg-max of ref_labels (N,G).
 *   inputs_fwd   : obj (N,K,F) = base[b] with edge[b][t][j] (edge: (B,K,L,F), NULL: none) added at the j-th one of the target's
 *                  adjacency row adj[b][t] (B,K,K); target_feats (N,F) = base[b][t]; valid (N,K) = locals[b][t] (NULL: skipped);
 *                  nbr (N,L) int32 = those slots (saved for the backward).
 *   inputs_bwd   : d_base (B,K,F), d_edge (B,K,L,F; zero-filled by the caller, NULL: none) from g_obj (N,K,F), g_target (N,F) or
 *                  NULL; a scene's descriptions are summed in ascending order (deterministic, no atomics). */
int d3_caption_select_target(const float *corners, const float *ref_corners, const float *ref_labels, int N, int per_scene, int K,
                             int G, long long *target_ids, float *target_ious, long long *labels, void *stream);
int d3_caption_inputs_fwd(const float *base, const float *edge, const float *adj, const float *locals, const long long *target_ids,
                          int N, int per_scene, int K, int L, int F, float *obj, float *target_feats, float *valid, int *nbr,
                          void *stream);
int d3_caption_inputs_bwd(const float *g_obj, const float *g_target, const long long *target_ids, const int *nbr, int N, int per_scene,
                          int K, int L, int F, float *d_base, float *d_edge, void *stream);

/* ---- box wireframes as PLY text (csrc/visualize.hip, driven by d3net_amd.visualize) ---------------------------------------
 * In place of write_bbox / write_ply of scripts/visualize_grounding.py:20-168 (scripts/visualize_captioning.py:20-168 is the same
 * code): per box the 12 x 11 x 10 = 1320 vertices of the twelve-cylinder wireframe, in the reference's order (edge, stack, slice),
 * and their text lines.  All pointers but ring20 are device memory; ring20 is HOST memory, 20 doubles: 0.03 * cos(i2 * 2 pi / 10)
 * for i2 = 0 .. 9, then the sines, from the host's libm (create_cylinder_mesh, :81-82), so that the bytes do not depend on the
 * device's trigonometry.  corners (M,8,3) float64 (a float32 box widened); min / max over the 8 corners is taken first, as :150-151.
 * Limits: every coordinate finite with |c| < 1e5, every extent's float32 square a normal positive number (the reference divides by
 * its root: a zero extent makes it print `nan nan nan`).  A box outside them is not written: status[0] |= 1 (coordinate) or 2
 * (extent) or 4 (mode outside {0, 1}), status[1] = min(status[1], box index); the caller sets status to {0, INT_MAX}.
 * d3_box_wire_limits: vertices per box (1320), the byte stride of a box's text (73920), the byte stride of a d3_format_f6 value (24).
 * d3_box_wire_verts : verts (M,1320,3) float64, one thread per vertex (create_cylinder_mesh, :75-106, for the 12 edges of :126-141).
 * d3_box_wire_text  : modes (M) int32, 0 = GT (colour `0 255 0`), 1 = prediction (`0 0 255`), :152-156.  text + b * stride receives
 *   box b's 1320 lines "{:f} {:f} {:f} r g b\n" (:39-40) back to back, nbytes[b] their length (0 for a refused box); the bytes of
 *   the slot behind nbytes[b], up to the next multiple of 4, are zeroed, the rest is left as it was.  One workgroup per box.
 * d3_format_f6      : the formatter alone: text + i * 24 receives "{:f}".format(values[i]) -- the exact binary value rounded
 *   half-to-even at six decimals, `-0.000000` for negatives that round to zero, nan / inf / -inf -- and lens[i] its length;
 *   a finite |value| >= 1e15 is refused: lens[i] = -1, *status |= 1 (status: one device int32).
 * M outside [1, 2^20], n outside [1, 2^30]: D3_ERR_RANGE before any launch.  No workspace. */
int d3_box_wire_limits(int *verts_per_box, int *text_stride, int *f6_stride);
int d3_box_wire_verts(const double *corners, int M, const double *ring20, double *verts, int *status, void *stream);
int d3_box_wire_text(const double *corners, const int *modes, int M, const double *ring20, char *text, int *nbytes, int *status,
                     void *stream);
int d3_format_f6(const double *values, long long n, char *text, int *lens, int *status, void *stream);

/* ---- ScanNet segmentation submission files (csrc/seg_submission.hip, driven by d3net_amd/seg_submission.py) ----------------------
 * In place of the file loop of PointGroup.test, model/pointgroup.py:603-625 (semantic/<scene>.txt, instance/<scene>.txt,
 * instance/predicted_masks/<scene>_<id:03d>.txt, instance/<scene>.cluster_ids.txt) and of the GT files of lib/utils/eval.py:14-56;
 * the bytes equal those of d3net_amd/seg_eval.py:write_predictions / write_gt.  All pointers are device memory, int32 unless said.
 * No kernel waits for another workgroup; plain vector stores and integer atomics only; no workspace but d3_seg_int_lines'.
 * d3_seg_submit_limits : lines per tile of d3_seg_int_lines (1024), its largest width (12), the most scenes per batch (4096), the
 *   ints per row of the cluster table (5).
 * d3_seg_cluster_table : model/pointgroup.py:608-623.  pick (n) proposal ids in pick order, proposals_idx (L,2), proposals_offset
 *   (P+1), semantic_pred (N), scores (n) float32, batch_offsets (B+1), lut (nlut) = the raw class id of a predicted class.  table
 *   (n,5) receives per pick [scene of its first member, scene-local id = earlier picks of that scene, lut[semantic_pred[first
 *   member]], flags, the score's bits]; a pick with an empty member list, or whose first member lies in no scene, is skipped: scene =
 *   id = -1, flags = 1.  counts (B): picks per scene.  *status |= 2 for a semantic_pred outside [0, nlut) (clamped), |= 4 for a pick
 *   outside [0, P), offsets outside [0, L] or a first member outside [0, N) (skipped).  One workgroup.
 * d3_seg_cluster_ids   : model/pointgroup.py:611-619.  cluster_ids (N) = the id of the LAST picked proposal of the point's scene
 *   that holds it, -1 for none: a fill launch, then atomicMax of the id per member entry; members outside the pick's scene are left.
 * d3_seg_int_lines     : np.savetxt(fmt="%d") (model/pointgroup.py:606, :625; lib/utils/eval.py:14-35) of one or two value arrays
 *   (values1 / lens1 NULL: one) cut by the same offsets (B+1) into B segments.  Per text: values (n_values), an optional lut
 *   applied first, width = the bytes of the longest line with its newline (2..12).  Segment b's text starts at byte offsets[b] *
 *   width of `text` (n_values * width bytes) and is dense from there; lens (B) int64 receives its length.  tile_prefix (B+1): the
 *   exclusive scan of ceil(segment length / 1024), tiles its last entry.  Three launches: per-tile byte totals, per-segment scan,
 *   the text.  *status |= 1 for a value whose line exceeds width (printed as 0), |= 2 for a value outside its lut (clamped), |= 4
 *   for tables that do not fit n_values (such a tile stores nothing).  ws: d3_seg_int_lines_ws_bytes(tiles, number of texts).
 * d3_seg_mask_lines    : model/pointgroup.py:614-624, the mask files c_lo .. c_lo + m - 1 of `scene`, whose points are [lo, lo +
 *   npts): text (16-byte aligned, text_bytes >= 2 m npts rounded up to 16) receives per file npts lines "0\n" / "1\n", file c at
 *   byte 2 npts (c - c_lo): a fill by 16-byte stores, then one byte store per member entry.  table / pick as above.
 * B outside [1, 4096], n above 2^20, L / N / n_values * width outside int32, a width outside [2, 12]: D3_ERR_RANGE before any launch. */
int d3_seg_submit_limits(int *tile_lines, int *max_width, int *max_scenes, int *table_cols);
int d3_seg_cluster_table(const int *pick, int n, const int *proposals_idx, long long L, const int *proposals_offset, int P,
                         const int *semantic_pred, const float *scores, long long N, const int *batch_offsets, int B, const int *lut,
                         int nlut, int *table, int *counts, int *status, void *stream);
int d3_seg_cluster_ids(const int *table, const int *pick, int n, const int *proposals_idx, long long L, const int *proposals_offset,
                       int P, const int *batch_offsets, int B, long long N, int *cluster_ids, void *stream);
size_t d3_seg_int_lines_ws_bytes(int tiles, int ntext);
int d3_seg_int_lines(const int *values0, const int *lut0, int nlut0, int width0, char *text0, long long *lens0, const int *values1,
                     const int *lut1, int nlut1, int width1, char *text1, long long *lens1, long long n_values, const int *offsets,
                     const int *tile_prefix, int B, int tiles, int *status, void *ws, size_t ws_bytes, void *stream);
int d3_seg_mask_lines(const int *table, const int *pick, int n, const int *proposals_idx, long long L, const int *proposals_offset, int P,
                      int scene, int lo, int npts, int c_lo, int m, char *text, size_t text_bytes, void *stream);

/* ---- running records of logged scalars (csrc/metric_log.hip, driven by d3net_amd.metric_log.MetricLog) --------------------
 * In place of Lightning's `self.log(..., on_epoch=True)` (model/pipeline.py:149,182,...): one launch per step folds every
 * scalar logged in that step into its slot's record; nothing is read back.
 * A table row names one slot's value of this step: the address of a 0-d device value (NULL: the key was not logged this
 * step, its record stays bit-unchanged), the value's type and a float64 weight.  A record is
 *   sum        sum of weight * value in float64: one multiplication and one addition per step, in step order, unfused
 *   wsum       sum of the weights
 *   last       the last value
 *   count      values folded in
 *   nonfinite  how many of them were inf or NaN (they propagate into sum as they do through a mean)
 * One thread per slot, one writer per record, no atomics: a record equals a sequential host sum bit for bit.
 * d3_metric_capacity  : slots one launch or one reset range covers (1024).
 * d3_metric_accumulate: table (nslots rows), records (nslots records), both device memory.  nslots outside
 *   [0, d3_metric_capacity()]: D3_ERR_RANGE before any launch -- never truncated.  A row whose dtype is none of the four codes is
 *   treated as not logged.
 * d3_metric_reset     : zeroes records[offset .. offset + count) (one asynchronous memset), so that several tables -- training
 *   and validation -- live in one buffer.  offset < 0 or count outside [0, d3_metric_capacity()]: D3_ERR_RANGE. */
#define D3_METRIC_F32 0
#define D3_METRIC_F64 1
#define D3_METRIC_I32 2
#define D3_METRIC_I64 3
typedef struct d3_metric_row {
    const void *value;
    long long dtype;
    double weight;
} d3_metric_row;
typedef struct d3_metric_rec {
    double sum;
    double wsum;
    double last;
    long long count;
    long long nonfinite;
} d3_metric_rec;
int d3_metric_capacity(void);
int d3_metric_accumulate(const void *table, int nslots, void *records, void *stream);
int d3_metric_reset(void *records, int offset, int count, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* D3HIP_H */
