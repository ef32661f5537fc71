// scene_prep.hip -- PointGroup scene preparation on the device: augmentation transform, elastic distortion, offset, crop,
// instance relabelling and per-instance statistics / box labels / GT proposal lists (reference: lib/dataset/pipeline.py:141-187,
// :679-772, :804-833; lib/utils/transform.py:elastic; lib/utils/pc.py:crop).  d3net_amd/scene_prep.py drives one scene at a
// time; the host keeps only the reference's data-dependent control flow (grid sizes, the crop loop, the instance count).
//
// Numerics follow numpy: the coordinate path is fp64 (float32 xyz @ float64 M stays float64 until the final cast), the blur
// rounds each pass to float32 after a double accumulation as scipy.ndimage.convolve does, the interpolation sums its eight
// corner terms in scipy's hypercube order.  The validation path (no augmentation) is float32 throughout, as in the reference.
// Every reduction that feeds an output is deterministic: min / max via integer atomics on an order-preserving encoding, sums
// in a fixed sequential order per instance, counts via integer atomics.
#include "scene_prep.h"

int d3_scene_limits(int *max_points, int *max_grid, int *max_id) {
    if (max_points) *max_points = SP_MAX_POINTS;
    if (max_grid) *max_grid = SP_MAX_GRID;
    if (max_id) *max_id = SP_MAX_ID;
    return 0;
}

static inline int sp_grid(long long n) {
    long long g = (n + SP_BLOCK - 1) / SP_BLOCK;
    return (int)(g < 1 ? 1 : (g > 65535 * 16 ? 65535 * 16 : g));
}

// ---- transform (pipeline.py:145-146, :679-697) ----------------------------------------------------------------------------------
struct SpMat { double m[9]; };

__global__ void sp_transform_kernel(const float *__restrict__ xyz, int n, SpMat M, double scale, float scale_f, int fp32,
                                    double *__restrict__ y, double *__restrict__ s) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        float x0 = xyz[3 * i], x1 = xyz[3 * i + 1], x2 = xyz[3 * i + 2];
        if (fp32) {                                   // points.copy() * scale: float32
            y[3 * i] = x0; y[3 * i + 1] = x1; y[3 * i + 2] = x2;
            s[3 * i] = (double)(x0 * scale_f); s[3 * i + 1] = (double)(x1 * scale_f); s[3 * i + 2] = (double)(x2 * scale_f);
        } else {                                      // np.matmul(xyz, m) in float64, then * scale
            for (int j = 0; j < 3; j++) {
                double v = (double)x0 * M.m[j] + (double)x1 * M.m[3 + j];
                v = v + (double)x2 * M.m[6 + j];
                y[3 * i + j] = v;
                s[3 * i + j] = v * scale;
            }
        }
    }
}

int d3_scene_transform(const float *xyz, int n, const double *m_host, double scale, int fp32, double *y, double *s, void *stream) {
    D3_CLEAR();
    if (n < 0 || n > SP_MAX_POINTS) return D3_ERR_RANGE;
    if (n == 0) return 0;
    if (!fp32 && !m_host) return D3_ERR_ARG;
    SpMat M;
    for (int k = 0; k < 9; k++) M.m[k] = fp32 ? 0.0 : m_host[k];
    hipLaunchKernelGGL(sp_transform_kernel, dim3(sp_grid(n)), dim3(SP_BLOCK), 0, d3_stream(stream), xyz, n, M, scale,
                       (float)scale, fp32, y, s);
    D3_LAUNCH_CHECK();
    return 0;
}

// ---- per-scene extents: |s| max (elastic grid sizes, transform.py:elastic), min / max (offset and crop), instance id range ----
// stats (12 u64): [0..2] enc |s| max, [3..5] enc min, [6..8] enc max, [9] id min + 2^31, [10] id max + 2^31
__global__ void sp_reduce_kernel(const double *__restrict__ s, const int *__restrict__ ids, int n, u64 *__restrict__ stats) {
    u64 amax[3] = {0, 0, 0}, mn[3] = {~0ull, ~0ull, ~0ull}, mx[3] = {0, 0, 0};
    u64 imn = ~0ull, imx = 0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        for (int d = 0; d < 3; d++) {
            double v = s[3 * i + d];
            u64 e = sp_enc(v), a = sp_enc(fabs(v));
            amax[d] = a > amax[d] ? a : amax[d];
            mn[d] = e < mn[d] ? e : mn[d];
            mx[d] = e > mx[d] ? e : mx[d];
        }
        if (ids) {
            u64 e = (u64)((long long)ids[i] + 2147483648ll);
            imn = e < imn ? e : imn;
            imx = e > imx ? e : imx;
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        for (int d = 0; d < 3; d++) {
            u64 a = __shfl_xor(amax[d], off), b = __shfl_xor(mn[d], off), c = __shfl_xor(mx[d], off);
            amax[d] = a > amax[d] ? a : amax[d];
            mn[d] = b < mn[d] ? b : mn[d];
            mx[d] = c > mx[d] ? c : mx[d];
        }
        u64 b = __shfl_xor(imn, off), c = __shfl_xor(imx, off);
        imn = b < imn ? b : imn;
        imx = c > imx ? c : imx;
    }
    if (d3_lane() == 0) {
        for (int d = 0; d < 3; d++) {
            atomicMax(&stats[d], amax[d]);
            atomicMin(&stats[3 + d], mn[d]);
            atomicMax(&stats[6 + d], mx[d]);
        }
        atomicMin(&stats[9], imn);
        atomicMax(&stats[10], imx);
    }
}

__global__ void sp_reduce_init(u64 *stats) {
    int t = threadIdx.x;
    if (t < 12) stats[t] = (t >= 3 && t < 6) || t == 9 ? ~0ull : 0ull;
}

int d3_scene_reduce(const double *s, const int *ids, int n, unsigned long long *stats, void *stream) {
    D3_CLEAR();
    if (n < 0 || n > SP_MAX_POINTS) return D3_ERR_RANGE;
    hipStream_t st = d3_stream(stream);
    hipLaunchKernelGGL(sp_reduce_init, dim3(1), dim3(64), 0, st, (u64 *)stats);
    D3_LAUNCH_CHECK();
    if (n == 0) return 0;
    int g = sp_grid(n);
    if (g > 1024) g = 1024;
    hipLaunchKernelGGL(sp_reduce_kernel, dim3(g), dim3(SP_BLOCK), 0, st, s, ids, n, (u64 *)stats);
    D3_LAUNCH_CHECK();
    return 0;
}

// ---- device noise: Philox4x32-10 + Box-Muller, counter = element index / 4, key = seed --------------------------------------
__global__ void sp_noise_kernel(float *__restrict__ g, long long count, u64 seed) {
    long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    for (; 4 * t < count; t += (long long)gridDim.x * blockDim.x) {
        float z[4];
        sp_noise_quad(t, seed, z);
        for (int j = 0; j < 4; j++)
            if (4 * t + j < count) g[4 * t + j] = z[j];
    }
}

int d3_scene_noise(float *grid, long long count, unsigned long long seed, void *stream) {
    D3_CLEAR();
    if (count < 0 || count > 3ll * SP_MAX_GRID) return D3_ERR_RANGE;
    if (count == 0) return 0;
    hipLaunchKernelGGL(sp_noise_kernel, dim3(sp_grid((count + 3) / 4)), dim3(SP_BLOCK), 0, d3_stream(stream), grid, count, (u64)seed);
    D3_LAUNCH_CHECK();
    return 0;
}

// ---- elastic (transform.py:elastic) ------------------------------------------------------------------------------------------
// One 3-tap box pass along `axis` over the scene's three grids in one launch: scipy.ndimage.convolve(mode='constant', cval=0)
// accumulates input * float32(1/3) in double over offsets -1, 0, +1 and rounds the sum to float32.  Six launches per elastic:
// a pass reads neighbours along one axis only, so fusing passes through LDS would need halo exchange across the whole tile
// for the z passes; the grids are at most a few MB (L2-resident) and the six launches cost microseconds.
__global__ void sp_blur_kernel(const float *__restrict__ in, float *__restrict__ out, int X, int Y, int Z, int axis) {
    long long per = (long long)X * Y * Z, total = 3 * per;
    long long stride = axis == 0 ? (long long)Y * Z : (axis == 1 ? Z : 1);
    int L = axis == 0 ? X : (axis == 1 ? Y : Z);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        long long e = i % per;
        int c = axis == 0 ? (int)(e / ((long long)Y * Z)) : (axis == 1 ? (int)((e / Z) % Y) : (int)(e % Z));
        float a = c > 0 ? in[i - stride] : 0.0f;
        float b = in[i];
        float d = c < L - 1 ? in[i + stride] : 0.0f;
        out[i] = sp_blur_tap(a, b, d);
    }
}

// RegularGridInterpolator(ax, noise, bounds_error=0, fill_value=0) at s, then s += g * mag
__global__ void sp_interp_kernel(double *__restrict__ s, int n, const float *__restrict__ g, const double *__restrict__ axes,
                                 int X, int Y, int Z, double mag) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        sp_interp_point(s + 3 * (size_t)i, g, axes, X, Y, Z, mag);
}

size_t d3_scene_elastic_ws_bytes(int X, int Y, int Z) {
    if (X < 3 || Y < 3 || Z < 3 || X > SP_MAX_GRID_DIM || Y > SP_MAX_GRID_DIM || Z > SP_MAX_GRID_DIM) return 0;
    long long per = (long long)X * Y * Z;
    if (per > SP_MAX_GRID) return 0;
    return d3_align((size_t)(3 * per) * sizeof(float));
}

int d3_scene_elastic(double *s, int n, float *grids, const double *axes, int X, int Y, int Z, double mag, void *ws,
                     size_t ws_bytes, void *stream) {
    D3_CLEAR();
    size_t need = d3_scene_elastic_ws_bytes(X, Y, Z);
    if (need == 0 || n < 0 || n > SP_MAX_POINTS) return D3_ERR_RANGE;
    if (need > ws_bytes || !ws) return D3_ERR_WORKSPACE;
    hipStream_t st = d3_stream(stream);
    long long total = 3ll * X * Y * Z;
    float *a = grids, *b = (float *)ws;
    for (int pass = 0; pass < 6; pass++) {            // x, y, z, x, y, z; an even count ends back in `grids`
        hipLaunchKernelGGL(sp_blur_kernel, dim3(sp_grid(total)), dim3(SP_BLOCK), 0, st, a, b, X, Y, Z, pass % 3);
        D3_LAUNCH_CHECK();
        float *t = a; a = b; b = t;
    }
    if (n == 0) return 0;
    hipLaunchKernelGGL(sp_interp_kernel, dim3(sp_grid(n)), dim3(SP_BLOCK), 0, st, s, n, (const float *)grids, axes, X, Y, Z, mag);
    D3_LAUNCH_CHECK();
    return 0;
}

// ---- offset: points -= points.min(0) (pipeline.py:155) -----------------------------------------------------------------------
__global__ void sp_offset_kernel(double *__restrict__ s, int n, const u64 *__restrict__ stats, int fp32) {
    double mn[3] = {sp_dec(stats[3]), sp_dec(stats[4]), sp_dec(stats[5])};
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        for (int d = 0; d < 3; d++)
            s[3 * i + d] = fp32 ? (double)((float)s[3 * i + d] - (float)mn[d]) : s[3 * i + d] - mn[d];
}

int d3_scene_offset(double *s, int n, const unsigned long long *stats, int fp32, void *stream) {
    D3_CLEAR();
    if (n < 0 || n > SP_MAX_POINTS) return D3_ERR_RANGE;
    if (n == 0) return 0;
    hipLaunchKernelGGL(sp_offset_kernel, dim3(sp_grid(n)), dim3(SP_BLOCK), 0, d3_stream(stream), s, n, (const u64 *)stats, fp32);
    D3_LAUNCH_CHECK();
    return 0;
}

// ---- crop candidate (pc.py:crop :40-42): flags[i] = all(s + off >= 0) and all(s + off < range); count = sum(flags) -------------
struct SpVec6 { double off[3], rng[3]; };

__global__ void sp_crop_kernel(const double *__restrict__ s, int n, SpVec6 p, int *__restrict__ flags, int *__restrict__ count) {
    int c = 0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        int f = sp_crop_keep(s + 3 * (size_t)i, p.off, p.rng);
        flags[i] = f;
        c += f;
    }
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
    if (d3_lane() == 0 && c) atomicAdd(count, c);
}

int d3_scene_crop_count(const double *s, int n, const double *off_host, const double *range_host, int *flags, int *count,
                        void *stream) {
    D3_CLEAR();
    if (n < 0 || n > SP_MAX_POINTS) return D3_ERR_RANGE;
    if (!off_host || !range_host) return D3_ERR_ARG;
    hipStream_t st = d3_stream(stream);
    D3_CHECK(hipMemsetAsync(count, 0, sizeof(int), st));
    if (n == 0) return 0;
    SpVec6 p;
    for (int d = 0; d < 3; d++) { p.off[d] = off_host[d]; p.rng[d] = range_host[d]; }
    int g = sp_grid(n);
    if (g > 2048) g = 2048;
    hipLaunchKernelGGL(sp_crop_kernel, dim3(g), dim3(SP_BLOCK), 0, st, s, n, p, flags, count);
    D3_LAUNCH_CHECK();
    return 0;
}

// ---- stable compaction of the kept points (pipeline.py:160-164) ----------------------------------------------------------------
__global__ void sp_emit_kernel(const double *__restrict__ y, const double *__restrict__ s, const float *__restrict__ feats, int C,
                               const int *__restrict__ sem, const int *__restrict__ ids, int n, const int *__restrict__ flags,
                               const int *__restrict__ pos, SpVec6 p, int fp32, double *__restrict__ y_out,
                               float *__restrict__ locs, float *__restrict__ locs_scaled, float *__restrict__ feats_out,
                               int *__restrict__ sem_out, int *__restrict__ ids_out) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        if (flags && !flags[i]) continue;
        int o = flags ? pos[i] : i;
        for (int d = 0; d < 3; d++) {
            double v = y[3 * i + d];
            y_out[3 * o + d] = v;
            locs[3 * o + d] = (float)v;
            locs_scaled[3 * o + d] = fp32 ? (float)s[3 * i + d] : (float)(s[3 * i + d] + p.off[d]);
        }
        for (int c = 0; c < C; c++) feats_out[(long long)o * C + c] = feats[(long long)i * C + c];
        sem_out[o] = sem[i];
        ids_out[o] = ids[i];
    }
}

// The three entry points share one workspace, one after the other: d3_scene_ws_bytes is the largest of their layouts.
struct SpEmitWs { int *pos; void *tmp; size_t tmp_bytes; };
static void sp_emit_layout(D3Carver &c, int n, SpEmitWs &w) {
    w.pos = c.take<int>(n);
    w.tmp_bytes = d3_scan_temp_bytes(n);
    w.tmp = c.take<char>(w.tmp_bytes);
}
struct SpRelabelWs { int *pres, *val_of, *orig_at; };
static void sp_relabel_layout(D3Carver &c, int V, SpRelabelWs &w) {
    w.pres = c.take<int>(V); w.val_of = c.take<int>(V); w.orig_at = c.take<int>(V);
}
struct SpInstWs {
    int *hist, *pres, *start, *rank, *keys, *vals, *keys2, *sorted;
    double *istats;
    void *scan_t, *sort_t; size_t scan_b, sort_b;
};
static void sp_inst_layout(D3Carver &c, int n, int V, SpInstWs &w) {
    w.hist = c.take<int>(V + 1); w.pres = c.take<int>(V + 1); w.start = c.take<int>(V + 1); w.rank = c.take<int>(V);
    w.keys = c.take<int>(n); w.vals = c.take<int>(n); w.keys2 = c.take<int>(n); w.sorted = c.take<int>(n);
    w.istats = c.take<double>(9 * (size_t)V);
    w.scan_b = d3_scan_temp_bytes(V + 1); w.sort_b = d3_sort_pairs_temp_bytes(n);
    w.scan_t = c.take<char>(w.scan_b); w.sort_t = c.take<char>(w.sort_b);
}

size_t d3_scene_ws_bytes(int n, int max_id) {
    if (n < 0 || n > SP_MAX_POINTS || max_id > SP_MAX_ID) return 0;
    const int V = (max_id < 0 ? 0 : max_id) + 1;
    D3Carver emit(nullptr, 0), relabel(nullptr, 0), inst(nullptr, 0);
    SpEmitWs we; SpRelabelWs wr; SpInstWs wi;
    sp_emit_layout(emit, n, we);
    sp_relabel_layout(relabel, V, wr);
    sp_inst_layout(inst, n, V, wi);
    const size_t m = emit.off > relabel.off ? emit.off : relabel.off;
    return m > inst.off ? m : inst.off;
}

int d3_scene_emit(const double *y, const double *s, const float *feats, int C, const int *sem, const int *ids, int n,
                  const int *flags, const double *off_host, int fp32, double *y_out, float *locs, float *locs_scaled,
                  float *feats_out, int *sem_out, int *ids_out, void *ws, size_t ws_bytes, void *stream) {
    D3_CLEAR();
    if (n < 0 || n > SP_MAX_POINTS || C < 0 || C > SP_MAX_FEAT) return D3_ERR_RANGE;
    if (n == 0) return 0;
    hipStream_t st = d3_stream(stream);
    SpVec6 p = {};
    if (off_host)
        for (int d = 0; d < 3; d++) p.off[d] = off_host[d];
    int *pos = nullptr;
    if (flags) {
        D3Carver cv(ws, ws_bytes);
        SpEmitWs w;
        sp_emit_layout(cv, n, w);
        if (!cv.ok()) return D3_ERR_WORKSPACE;
        pos = w.pos;
        int rc = d3_exclusive_scan_i32(flags, pos, n, w.tmp, w.tmp_bytes, st);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(sp_emit_kernel, dim3(sp_grid(n)), dim3(SP_BLOCK), 0, st, y, s, feats, C, sem, ids, n, flags, pos, p, fp32,
                       y_out, locs, locs_scaled, feats_out, sem_out, ids_out);
    D3_LAUNCH_CHECK();
    return 0;
}

// ---- _croppedInstanceIds (pipeline.py:699-709) -------------------------------------------------------------------------------
__global__ void sp_presence_kernel(const int *__restrict__ ids, int n, int V, int *__restrict__ pres) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        int v = ids[i];
        if (v >= 0 && v < V) pres[v] = 1;
    }
}

// The reference's loop, on the id-presence table: `while j < ids.max(): if j absent: ids[ids == ids.max()] = j; j += 1`.
// val_of[v] = the id the points that had id v end with; orig_at[u] = which original id holds value u now (-1: none).
__global__ void sp_relabel_map_kernel(const int *__restrict__ pres, int V, int *__restrict__ val_of, int *__restrict__ orig_at) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    sp_relabel_walk(pres, V, val_of, orig_at);
}

__global__ void sp_relabel_apply_kernel(int *__restrict__ ids, int n, int V, const int *__restrict__ val_of) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        int v = ids[i];
        if (v >= 0 && v < V) ids[i] = val_of[v];
    }
}

int d3_scene_relabel(int *ids, int n, int max_id, void *ws, size_t ws_bytes, void *stream) {
    D3_CLEAR();
    if (n < 0 || n > SP_MAX_POINTS || max_id > SP_MAX_ID) return D3_ERR_RANGE;
    if (n == 0 || max_id < 0) return 0;
    int V = max_id + 1;
    hipStream_t st = d3_stream(stream);
    D3Carver cv(ws, ws_bytes);
    SpRelabelWs w;
    sp_relabel_layout(cv, V, w);
    if (!cv.ok()) return D3_ERR_WORKSPACE;
    int *pres = w.pres, *val_of = w.val_of, *orig_at = w.orig_at;
    D3_CHECK(hipMemsetAsync(pres, 0, (size_t)V * 4, st));
    hipLaunchKernelGGL(sp_presence_kernel, dim3(sp_grid(n)), dim3(SP_BLOCK), 0, st, (const int *)ids, n, V, pres);
    D3_LAUNCH_CHECK();
    hipLaunchKernelGGL(sp_relabel_map_kernel, dim3(1), dim3(64), 0, st, (const int *)pres, V, val_of, orig_at);
    D3_LAUNCH_CHECK();
    hipLaunchKernelGGL(sp_relabel_apply_kernel, dim3(sp_grid(n)), dim3(SP_BLOCK), 0, st, ids, n, V, (const int *)val_of);
    D3_LAUNCH_CHECK();
    return 0;
}

// ---- _getInstanceInfo (pipeline.py:711-772) and _generate_gt_clusters (:804-833) ---------------------------------------------
// hist[v + 1] = points with id v (hist[0]: unlabelled); present ids in np.unique order get rank = exclusive scan of presence;
// start[v] = exclusive scan of the counts = the instance's first row in the GT proposal list.
__global__ void sp_hist_kernel(const int *__restrict__ ids, int n, int V, int *__restrict__ hist) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        int v = ids[i];
        if (v >= -1 && v < V) atomicAdd(&hist[v + 1], 1);
    }
}

__global__ void sp_presence_from_hist(const int *__restrict__ hist, int V, int *__restrict__ pres) {
    for (int v = blockIdx.x * blockDim.x + threadIdx.x; v < V; v += gridDim.x * blockDim.x) pres[v] = hist[v + 1] > 0;
}

// counts = {K instances, L labelled points, has unlabelled}
__global__ void sp_totals_kernel(const int *__restrict__ hist, const int *__restrict__ rank, const int *__restrict__ start,
                                 int V, int *__restrict__ counts) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    counts[0] = rank[V - 1] + (hist[V] > 0);
    counts[1] = start[V - 1] + hist[V];
    counts[2] = hist[0] > 0;
}

__global__ void sp_keys_kernel(const int *__restrict__ ids, int n, int V, const int *__restrict__ rank,
                               const int *__restrict__ counts, int *__restrict__ keys, int *__restrict__ vals) {
    int K = counts[0];
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        int v = ids[i];
        keys[i] = (v >= 0 && v < V) ? rank[v] : K;   // unlabelled points sort behind every instance
        vals[i] = i;
    }
}

// one wave per id value: count, exact min / max, and the sum in numpy's order (sequential over ascending point index) --
// float64 for the augmented path, float32 for the validation path.  Writes mean / min / max, instance_num_point, the GT
// proposal offsets and the instance's box slot.
template <typename T>
__global__ void __launch_bounds__(64) sp_instance_kernel(const double *__restrict__ y, const int *__restrict__ sem,
        const int *__restrict__ hist, const int *__restrict__ rank, const int *__restrict__ start, const int *__restrict__ sorted,
        const int *__restrict__ counts, int V, int R, const double *__restrict__ mean_size, double *__restrict__ istats,
        int *__restrict__ num_point, int *__restrict__ gt_off, double *__restrict__ boxes) {
    __shared__ T buf[64][3];
    int v = blockIdx.x, lane = threadIdx.x;
    if (v >= V) return;
    int cnt = hist[v + 1];
    if (cnt == 0) return;
    int st = start[v], r = rank[v];
    T mn[3], mx[3], sum[3];
    for (int d = 0; d < 3; d++) { mn[d] = (T)INFINITY; mx[d] = (T)-INFINITY; sum[d] = (T)0; }
    for (int base = 0; base < cnt; base += 64) {
        int m = cnt - base < 64 ? cnt - base : 64;
        if (lane < m) {
            int p = sorted[st + base + lane];
            for (int d = 0; d < 3; d++) {
                T val = (T)y[3 * (long long)p + d];
                buf[lane][d] = val;
                mn[d] = val < mn[d] ? val : mn[d];
                mx[d] = val > mx[d] ? val : mx[d];
            }
        }
        __syncthreads();
        if (lane < 3)
            for (int j = 0; j < m; j++) sum[lane] = sum[lane] + buf[j][lane];
        __syncthreads();
    }
    for (int off = 32; off > 0; off >>= 1)
        for (int d = 0; d < 3; d++) {
            T a = __shfl_xor(mn[d], off), b = __shfl_xor(mx[d], off);
            mn[d] = a < mn[d] ? a : mn[d];
            mx[d] = b > mx[d] ? b : mx[d];
        }
    if (lane < 3) {
        istats[9 * v + lane] = (double)(sum[lane] / (T)cnt);
        istats[9 * v + 3 + lane] = (double)mn[lane];
        istats[9 * v + 6 + lane] = (double)mx[lane];
    }
    if (lane != 0) return;
    num_point[r] = cnt;
    gt_off[r] = st;
    int K = counts[0], has_neg = counts[2];
    if (r == K - 1) gt_off[K] = st + cnt;
    // enumerate(np.unique(ids), -1): without unlabelled points the first instance gets k = -1 (the last row) -- unless a later
    // instance takes k = R - 1 and overwrites that row; k >= 128 is skipped (and so is k >= R, where the reference would index past
    // its arrays)
    int k = r - (has_neg ? 0 : 1);
    if (k >= 128 || k >= R) return;
    if (k < 0) {
        int kmax = K - 1 - (has_neg ? 0 : 1);
        if (R - 1 < 128 && kmax >= R - 1) return;
    }
    int slot = k < 0 ? R - 1 : k;
    int c = sem[sorted[st]];
    c = c >= 2 ? c - 2 : 17;
    double *b = boxes + 36 * (long long)slot;
    double ctr[3], size[3];
    for (int d = 0; d < 3; d++) {
        ctr[d] = (double)((mn[d] + mx[d]) / (T)2);
        size[d] = (double)(mx[d] - mn[d]);
        b[d] = ctr[d];
        b[3 + d] = size[d];
        b[9 + d] = size[d] - mean_size[3 * c + d];
    }
    b[6] = c; b[7] = v; b[8] = 1.0;
    // get_3d_box_batch with heading 0 (lib/utils/bbox.py:54-74): corners = center + (+-l/2, +-w/2, +-h/2)
    const int sx[8] = {1, 1, -1, -1, 1, 1, -1, -1}, sy[8] = {1, -1, -1, 1, 1, -1, -1, 1}, sz[8] = {1, 1, 1, 1, -1, -1, -1, -1};
    for (int q = 0; q < 8; q++) {
        b[12 + 3 * q] = sx[q] * (size[0] / 2) + ctr[0];
        b[13 + 3 * q] = sy[q] * (size[1] / 2) + ctr[1];
        b[14 + 3 * q] = sz[q] * (size[2] / 2) + ctr[2];
    }
}

// instance_info rows: mean, (min + max) / 2, min, max (zeros for unlabelled points)
template <typename T>
__global__ void sp_info_kernel(const int *__restrict__ ids, int n, int V, const double *__restrict__ istats, float *__restrict__ info) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        int v = ids[i];
        float *o = info + 12 * (long long)i;
        if (v < 0 || v >= V) {
            for (int c = 0; c < 12; c++) o[c] = 0.0f;
            continue;
        }
        const double *q = istats + 9 * v;
        for (int d = 0; d < 3; d++) {
            T mn = (T)q[3 + d], mx = (T)q[6 + d];
            o[d] = (float)q[d];
            o[3 + d] = (float)((mn + mx) / (T)2);
            o[6 + d] = (float)mn;
            o[9 + d] = (float)mx;
        }
    }
}

// gt_proposals_idx rows (cid, point), instances in unique order, ascending point index inside each (the stable sort)
__global__ void sp_gtidx_kernel(const int *__restrict__ ids, const int *__restrict__ sorted, const int *__restrict__ rank,
                                const int *__restrict__ counts, int *__restrict__ gt_idx) {
    int L = counts[1], shift = counts[2] ? 0 : 1;
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < L; p += gridDim.x * blockDim.x) {
        int i = sorted[p];
        gt_idx[2 * p] = rank[ids[i]] - shift;
        gt_idx[2 * p + 1] = i;
    }
}

int d3_scene_instances(const double *y, const int *ids, const int *sem, int n, int max_id, int fp32, int R, const double *mean_size,
                       float *info, int *num_point, int *gt_idx, int *gt_off, double *boxes, int *counts, void *ws,
                       size_t ws_bytes, void *stream) {
    D3_CLEAR();
    if (n < 0 || n > SP_MAX_POINTS || max_id > SP_MAX_ID || R < 1) return D3_ERR_RANGE;
    hipStream_t st = d3_stream(stream);
    int V = (max_id < 0 ? 0 : max_id) + 1;
    D3Carver cv(ws, ws_bytes);
    SpInstWs w;
    sp_inst_layout(cv, n, V, w);
    if (!cv.ok()) return D3_ERR_WORKSPACE;
    int *hist = w.hist, *pres = w.pres, *start = w.start, *rank = w.rank;
    int *keys = w.keys, *vals = w.vals, *keys2 = w.keys2, *sorted = w.sorted;
    double *istats = w.istats;
    int *cnt_dev = counts;
    const size_t scan_b = w.scan_b, sort_b = w.sort_b;
    void *scan_t = w.scan_t, *sort_t = w.sort_t;
    D3_CHECK(hipMemsetAsync(hist, 0, (size_t)(V + 1) * 4, st));
    D3_CHECK(hipMemsetAsync(counts, 0, 4 * sizeof(int), st));
    if (n > 0) {
        hipLaunchKernelGGL(sp_hist_kernel, dim3(sp_grid(n)), dim3(SP_BLOCK), 0, st, ids, n, V, hist);
        D3_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(sp_presence_from_hist, dim3(sp_grid(V)), dim3(SP_BLOCK), 0, st, (const int *)hist, V, pres);
    D3_LAUNCH_CHECK();
    int rc = d3_exclusive_scan_i32(pres, rank, V, scan_t, scan_b, st);
    if (rc) return rc;
    rc = d3_exclusive_scan_i32(hist + 1, start, V, scan_t, scan_b, st);
    if (rc) return rc;
    hipLaunchKernelGGL(sp_totals_kernel, dim3(1), dim3(64), 0, st, (const int *)hist, (const int *)rank, (const int *)start, V,
                       cnt_dev);
    D3_LAUNCH_CHECK();
    if (n == 0) return 0;
    hipLaunchKernelGGL(sp_keys_kernel, dim3(sp_grid(n)), dim3(SP_BLOCK), 0, st, ids, n, V, (const int *)rank,
                       (const int *)cnt_dev, keys, vals);
    D3_LAUNCH_CHECK();
    int bits = 1;
    while ((1 << bits) <= V) bits++;
    rc = d3_sort_pairs_i32(keys, keys2, vals, sorted, n, bits, sort_t, sort_b, st);
    if (rc) return rc;
    if (fp32)
        hipLaunchKernelGGL(sp_instance_kernel<float>, dim3(V), dim3(64), 0, st, y, sem, (const int *)hist, (const int *)rank,
                           (const int *)start, (const int *)sorted, (const int *)cnt_dev, V, R, mean_size, istats, num_point, gt_off, boxes);
    else
        hipLaunchKernelGGL(sp_instance_kernel<double>, dim3(V), dim3(64), 0, st, y, sem, (const int *)hist, (const int *)rank,
                           (const int *)start, (const int *)sorted, (const int *)cnt_dev, V, R, mean_size, istats, num_point, gt_off, boxes);
    D3_LAUNCH_CHECK();
    if (fp32)
        hipLaunchKernelGGL(sp_info_kernel<float>, dim3(sp_grid(n)), dim3(SP_BLOCK), 0, st, ids, n, V, (const double *)istats, info);
    else
        hipLaunchKernelGGL(sp_info_kernel<double>, dim3(sp_grid(n)), dim3(SP_BLOCK), 0, st, ids, n, V, (const double *)istats, info);
    D3_LAUNCH_CHECK();
    hipLaunchKernelGGL(sp_gtidx_kernel, dim3(sp_grid(n)), dim3(SP_BLOCK), 0, st, ids, (const int *)sorted, (const int *)rank,
                       (const int *)cnt_dev, gt_idx);
    D3_LAUNCH_CHECK();
    return 0;
}
