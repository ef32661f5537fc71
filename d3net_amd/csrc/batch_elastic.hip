// batch_elastic.hip -- the augmented detector-only batch (lib/dataset/pipeline.py:145-164: jitter / flip / rotation, two elastic
// distortions, crop to data.max_num_point, _croppedInstanceIds; then :711-772, :804-833 and sparse_collate_fn) straight from the
// resident scene store: what scene_prep.hip computes scene by scene and collate.hip then stacks, written once into the batch
// tensors, bit for bit.  Driven by d3net_amd/scene_prep.py:prepare_batch_store_elastic.
//
// Only the NUMBER of kept points is data-dependent here, so nothing but one small table (kept points, K, Lp, the two real noise-grid
// shapes and the crop iterations of every slot) goes back to the host, once per batch and after everything is queued:
//   * the noise grids are sized on the host by an upper bound; the real shape `int32(|s| max) // gran + 3` is resolved on the device
//     from the reduction, the kernels read it from device memory and blocks beyond a slot's real extent exit;
//   * the crop loop (pc.py:crop) has at most T iterations, so it is T launches; each reads the slot's earlier counts and exits at
//     once when the slot has finished (or never entered the loop).  The draws are a (T,3) table per slot;
//   * outputs are allocated at their static upper bounds; the running totals across slots are made on the device.
// The number of launches and copies depends neither on B nor on the scenes' sizes nor on the crop iterations any slot runs.
//
// The per-point and per-cell arithmetic is scene_prep.hip's (scene_prep.h), the box rows are batch_prep.hip's; -ffp-contract=off.
// Reductions are deterministic: min / max by integer atomics on the order-preserving encoding, counts by integer atomics, the
// per-instance sums sequential over ascending point index.  No floating-point atomics, no per-scene tensor.
#include "scene_prep.h"

#define BE_BLOCK 256
#define BE_PTILE 1024                 // points per block: 4 per thread
#define BE_GTILE 2048                 // noise-grid elements per block: 8 per thread (2 Philox quads per thread)
#define BE_MAX_B 512
#define BE_MAX_T 80                   // crop iterations: ceil(2048 / 32) + 1 and some
#define BE_RB 10                      // read-back ints per slot: kept, K, Lp, X1 Y1 Z1, X2 Y2 Z2, crop iterations
#define BE_KEY_BITS 17                // the in-slot sort key: a rank <= SP_MAX_ID + 1

struct BeSlot {
    long long row0;                   // first store row
    long long gbase;                  // first float of the slot's noise-grid region
    u64 seed;
    int n, P, V, vbase, abase, pad;   // points, points of the slots before (uncropped), id values, id values before, first axis entry
    int bnd[2][3];                    // the host's upper bound of the two grid shapes
    double m[9];
};

struct BeArgs {
    const float *xyz, *feats;
    const int *sem, *ids;
    const double *mean_size;
    // the table (one copy): slots, the start values of the reductions and counts, the crop draws, the tile prefixes
    const BeSlot *slots;
    u64 *stats;                       // (B,3,9): after the transform / elastic 1 / elastic 2: |s| max, min, max per axis, encoded
    int *cnt;                         // (B,T) kept points of every crop iteration that ran
    const double *u;                  // (B,T,3) crop draws
    const int *pprefix, *gprefix[2], *vprefix;
    // workspace
    double *y, *s, *y2, *istats, *axes;
    int *flags, *pos, *ids2, *slot_of, *keys, *vals, *sorted;
    long long *src;
    int *pres, *hist, *val_of, *orig_at, *rank, *start;
    int *dims, *real;                 // (B,2,3) the grid shapes the kernels use (clamped to the bound) / as computed
    int *sK, *sLp, *sUnl, *sI, *sQ;   // per slot: instances, labelled points, any unlabelled, instances / proposal entries before
    float *grid[2];
    int *readback;                    // (B, BE_RB)
    int B, C, R, T, has_gt, N, max_pt, gran[2];
    double scale, mag[2], crop_scale;
    BpOut o;
};

// wave-reduce one thread's encoded |s| max / min / max and combine across waves by integer atomics
__device__ __forceinline__ void be_reduce_stats(u64 *amax, u64 *mn, u64 *mx, u64 *__restrict__ stats) {
    for (int off = 32; off > 0; off >>= 1)
        for (int d = 0; d < 3; d++) {
            u64 a = __shfl_xor(amax[d], off), b = __shfl_xor(mn[d], off), c = __shfl_xor(mx[d], off);
            amax[d] = a > amax[d] ? a : amax[d];
            mn[d] = b < mn[d] ? b : mn[d];
            mx[d] = c > mx[d] ? c : mx[d];
        }
    if (d3_lane() == 0)
        for (int d = 0; d < 3; d++) {
            atomicMax(&stats[d], amax[d]);
            atomicMin(&stats[3 + d], mn[d]);
            atomicMax(&stats[6 + d], mx[d]);
        }
}

__device__ __forceinline__ void be_accumulate(const double *v, u64 *amax, u64 *mn, u64 *mx) {
    for (int d = 0; d < 3; d++) {
        u64 e = sp_enc(v[d]), a = sp_enc(fabs(v[d]));
        amax[d] = a > amax[d] ? a : amax[d];
        mn[d] = e < mn[d] ? e : mn[d];
        mx[d] = e > mx[d] ? e : mx[d];
    }
}

// ---- transform (pipeline.py:145-146): y, s kept as float64; flags start at 1; the |s| maxima of elastic 1 -----------------------------
__global__ void __launch_bounds__(BE_BLOCK) be_transform_kernel(BeArgs a) {
    extern __shared__ int s_prefix[];
    const int t = (int)threadIdx.x;
    const int slot = bp_find(s_prefix, a.pprefix, a.B), tile = (int)blockIdx.x - s_prefix[slot];
    const BeSlot *__restrict__ sl = a.slots + slot;
    const int n = sl->n;
    double m[9];
    for (int k = 0; k < 9; k++) m[k] = sl->m[k];
    const float *__restrict__ x = a.xyz + 3 * sl->row0;
    u64 amax[3] = {0, 0, 0}, mn[3] = {~0ull, ~0ull, ~0ull}, mx[3] = {0, 0, 0};
    for (int k = 0; k < BE_PTILE / BE_BLOCK; ++k) {
        int i = tile * BE_PTILE + t + k * BE_BLOCK;
        if (i >= n) continue;
        const size_t g = (size_t)sl->P + i;
        double y[3], s[3];
        bp_transform(x[3 * (size_t)i], x[3 * (size_t)i + 1], x[3 * (size_t)i + 2], m, 0, a.scale, 0.0f, y, s);
        for (int d = 0; d < 3; d++) { a.y[3 * g + d] = y[d]; a.s[3 * g + d] = s[d]; }
        a.flags[g] = 1;
        be_accumulate(s, amax, mn, mx);
    }
    be_reduce_stats(amax, mn, mx, a.stats + 27 * (size_t)slot);
}

// ---- elastic (transform.py:elastic) ---------------------------------------------------------------------------------------------------
// one thread per slot: bb = int32(|s| max) // gran + 3 from the reduction, clamped to the host's bound (the host raises after the
// read-back if the clamp ever bit), and the three axes -(b - 1) gran + 2 gran k, all exact integers (= np.linspace's values)
__global__ void be_resolve_kernel(BeArgs a, int e) {
    const int slot = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (slot >= a.B) return;
    const BeSlot *__restrict__ sl = a.slots + slot;
    const int gran = a.gran[e];
    double *ax = a.axes + sl->abase;
    for (int d = 0; d < 3; d++) {
        const double amax = sp_dec(a.stats[27 * (size_t)slot + 9 * e + d]);
        int bb = 3;
        if (amax >= 0.0 && amax < 2147483647.0) bb = (int)amax / gran + 3;
        else if (amax >= 2147483647.0) bb = 0x7fffffff;
        a.real[6 * slot + 3 * e + d] = bb;
        const int b = bb < 3 ? 3 : (bb > sl->bnd[e][d] ? sl->bnd[e][d] : bb);
        a.dims[6 * slot + 3 * e + d] = b;
        for (int k = 0; k < b; k++) ax[k] = (double)(-(b - 1) * gran + 2 * gran * k);
        ax += b;
    }
}

// sp_noise_kernel's stream: key (seed << 1) | e, counter = element index / 4 in the slot's real (3, X, Y, Z) layout
__global__ void __launch_bounds__(BE_BLOCK) be_noise_kernel(BeArgs a, int e) {
    extern __shared__ int s_prefix[];
    const int t = (int)threadIdx.x;
    const int slot = bp_find(s_prefix, a.gprefix[e], a.B), tile = (int)blockIdx.x - s_prefix[slot];
    const BeSlot *__restrict__ sl = a.slots + slot;
    const int *dm = a.dims + 6 * slot + 3 * e;
    const long long count = 3ll * dm[0] * dm[1] * dm[2];
    if ((long long)tile * BE_GTILE >= count) return;
    float *__restrict__ g = a.grid[0] + sl->gbase;
    const u64 seed = (sl->seed << 1) | (u64)e;
    for (int k = 0; k < BE_GTILE / (4 * BE_BLOCK); ++k) {
        const long long q = (long long)tile * (BE_GTILE / 4) + t + k * BE_BLOCK;
        if (4 * q >= count) continue;
        float z[4];
        sp_noise_quad(q, seed, z);
        for (int j = 0; j < 4; j++)
            if (4 * q + j < count) g[4 * q + j] = z[j];
    }
}

// sp_blur_kernel's pass along `axis` over every slot's three grids
__global__ void __launch_bounds__(BE_BLOCK) be_blur_kernel(BeArgs a, int e, int axis, int from) {
    extern __shared__ int s_prefix[];
    const int t = (int)threadIdx.x;
    const int slot = bp_find(s_prefix, a.gprefix[e], a.B), tile = (int)blockIdx.x - s_prefix[slot];
    const BeSlot *__restrict__ sl = a.slots + slot;
    const int *dm = a.dims + 6 * slot + 3 * e;
    const int X = dm[0], Y = dm[1], Z = dm[2];
    const long long per = (long long)X * Y * Z, total = 3 * per;
    if ((long long)tile * BE_GTILE >= total) return;
    const float *__restrict__ in = a.grid[from] + sl->gbase;
    float *__restrict__ out = a.grid[from ^ 1] + sl->gbase;
    const long long stride = axis == 0 ? (long long)Y * Z : (axis == 1 ? Z : 1);
    const int L = axis == 0 ? X : (axis == 1 ? Y : Z);
    for (int k = 0; k < BE_GTILE / BE_BLOCK; ++k) {
        const long long i = (long long)tile * BE_GTILE + t + k * BE_BLOCK;
        if (i >= total) continue;
        const long long el = i % per;
        const int c = axis == 0 ? (int)(el / ((long long)Y * Z)) : (axis == 1 ? (int)((el / Z) % Y) : (int)(el % Z));
        const float p = c > 0 ? in[i - stride] : 0.0f;
        const float q = in[i];
        const float r = c < L - 1 ? in[i + stride] : 0.0f;
        out[i] = sp_blur_tap(p, q, r);
    }
}

// sp_interp_kernel per point, and the reduction the next stage needs (elastic 2's |s| maxima / the extent)
__global__ void __launch_bounds__(BE_BLOCK) be_interp_kernel(BeArgs a, int e) {
    extern __shared__ int s_prefix[];
    const int t = (int)threadIdx.x;
    const int slot = bp_find(s_prefix, a.pprefix, a.B), tile = (int)blockIdx.x - s_prefix[slot];
    const BeSlot *__restrict__ sl = a.slots + slot;
    const int n = sl->n;
    const int *dm = a.dims + 6 * slot + 3 * e;
    const float *__restrict__ g = a.grid[0] + sl->gbase;                  // six passes end in the buffer they started from
    const double *__restrict__ ax = a.axes + sl->abase;
    u64 amax[3] = {0, 0, 0}, mn[3] = {~0ull, ~0ull, ~0ull}, mx[3] = {0, 0, 0};
    for (int k = 0; k < BE_PTILE / BE_BLOCK; ++k) {
        int i = tile * BE_PTILE + t + k * BE_BLOCK;
        if (i >= n) continue;
        double *s3 = a.s + 3 * ((size_t)sl->P + i);
        sp_interp_point(s3, g, ax, dm[0], dm[1], dm[2], a.mag[e]);
        be_accumulate(s3, amax, mn, mx);
    }
    be_reduce_stats(amax, mn, mx, a.stats + 27 * (size_t)slot + 9 * (e + 1));
}

// ---- offset (pipeline.py:155): the float64 arm of sp_offset_kernel -------------------------------------------------------------------
__global__ void __launch_bounds__(BE_BLOCK) be_offset_kernel(BeArgs a) {
    extern __shared__ int s_prefix[];
    const int t = (int)threadIdx.x;
    const int slot = bp_find(s_prefix, a.pprefix, a.B), tile = (int)blockIdx.x - s_prefix[slot];
    const BeSlot *__restrict__ sl = a.slots + slot;
    const u64 *st = a.stats + 27 * (size_t)slot + 18;
    const double mn[3] = {sp_dec(st[3]), sp_dec(st[4]), sp_dec(st[5])};
    for (int k = 0; k < BE_PTILE / BE_BLOCK; ++k) {
        int i = tile * BE_PTILE + t + k * BE_BLOCK;
        if (i >= sl->n) continue;
        double *s3 = a.s + 3 * ((size_t)sl->P + i);
        for (int d = 0; d < 3; d++) s3[d] = s3[d] - mn[d];
    }
}

// ---- crop (pc.py:crop) ------------------------------------------------------------------------------------------------------------------
// how many of the first `upto` iterations of `while valid > max_num_point` ran, and the count the last of them left
__device__ __forceinline__ int be_crop_ran(const int *__restrict__ cnt, int n, int max_pt, int upto, int *valid_out) {
    int valid = n, k = 0;
    while (k < upto && valid > max_pt) { valid = cnt[k]; k++; }
    *valid_out = valid;
    return k;
}

// iteration j's candidate: offset = min(max_pc_range - pc_range + 0.001, 0) * u_j with max_pc_range = [S - 32 j, S - 32 j, S]
__device__ __forceinline__ void be_crop_candidate(const u64 *__restrict__ st, const double *__restrict__ u, double S, int j,
                                                  double *off, double *rng) {
    double r = S;
    for (int k = 0; k < j; k++) r = r - 32.0;
    rng[0] = r; rng[1] = r; rng[2] = S;
    for (int d = 0; d < 3; d++) {
        const double pc = (sp_dec(st[6 + d]) - sp_dec(st[3 + d])) - 0.0;
        double v = (rng[d] - pc) + 0.001;
        v = v < 0.0 ? v : 0.0;
        off[d] = v * u[3 * j + d];
    }
}

__global__ void __launch_bounds__(BE_BLOCK) be_crop_kernel(BeArgs a, int j) {
    extern __shared__ int s_prefix[];
    const int t = (int)threadIdx.x;
    const int slot = bp_find(s_prefix, a.pprefix, a.B), tile = (int)blockIdx.x - s_prefix[slot];
    const BeSlot *__restrict__ sl = a.slots + slot;
    const int n = sl->n;
    int *cnt = a.cnt + (size_t)slot * a.T;
    int valid;
    if (be_crop_ran(cnt, n, a.max_pt, j, &valid) != j || valid <= a.max_pt) return;     // the slot has finished (or never began)
    double off[3], rng[3];
    be_crop_candidate(a.stats + 27 * (size_t)slot + 18, a.u + 3 * (size_t)slot * a.T, a.crop_scale, j, off, rng);
    int c = 0;
    for (int k = 0; k < BE_PTILE / BE_BLOCK; ++k) {
        int i = tile * BE_PTILE + t + k * BE_BLOCK;
        if (i >= n) continue;
        const size_t g = (size_t)sl->P + i;
        int f = sp_crop_keep(a.s + 3 * g, off, rng);
        a.flags[g] = f;
        c += f;
    }
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if (d3_lane() == 0 && c) atomicAdd(&cnt[j], c);
}

// ---- emit: stable compaction of the kept points of all slots (pipeline.py:160-164, sparse_collate_fn's point keys) --------------------
__global__ void __launch_bounds__(BE_BLOCK) be_emit_kernel(BeArgs a) {
    extern __shared__ int s_prefix[];
    const int t = (int)threadIdx.x;
    const int slot = bp_find(s_prefix, a.pprefix, a.B), tile = (int)blockIdx.x - s_prefix[slot];
    const BeSlot *__restrict__ sl = a.slots + slot;
    const int n = sl->n, P = sl->P;
    int valid;
    const int iters = be_crop_ran(a.cnt + (size_t)slot * a.T, n, a.max_pt, a.T, &valid);
    double off[3] = {0.0, 0.0, 0.0}, rng[3];
    if (iters > 0) be_crop_candidate(a.stats + 27 * (size_t)slot + 18, a.u + 3 * (size_t)slot * a.T, a.crop_scale, iters - 1, off, rng);
    if (tile == 0 && t == 0) {
        a.o.boff[slot] = a.pos[P];
        if (slot == a.B - 1) a.o.boff[a.B] = a.pos[a.N - 1] + a.flags[a.N - 1];
    }
    const long long row0 = sl->row0;
    for (int k = 0; k < BE_PTILE / BE_BLOCK; ++k) {
        int i = tile * BE_PTILE + t + k * BE_BLOCK;
        if (i >= n) continue;
        const size_t g = (size_t)P + i;
        if (!a.flags[g]) continue;
        const size_t o = (size_t)a.pos[g];
        float ls[3];
        for (int d = 0; d < 3; d++) {
            const double v = a.y[3 * g + d];
            a.y2[3 * o + d] = v;
            a.o.locs[3 * o + d] = (float)v;
            ls[d] = (float)(a.s[3 * g + d] + off[d]);
        }
        longlong2 *lo = (longlong2 *)(a.o.locs_scaled + 4 * o);           // 32-byte rows from a 16-byte aligned base
        lo[0] = make_longlong2((long long)slot, (long long)ls[0]);
        lo[1] = make_longlong2((long long)ls[1], (long long)ls[2]);
        a.o.sem[o] = (long long)a.sem[row0 + i];
        a.ids2[o] = a.ids[row0 + i];
        a.src[o] = row0 + i;
        a.slot_of[o] = slot;
    }
}

// the feature rows of the kept points, each word copied once
__global__ void __launch_bounds__(BE_BLOCK) be_feats_kernel(BeArgs a) {
    const long long total = (long long)a.o.boff[a.B] * a.C;
    for (int k = 0; k < 4; ++k) {
        const long long w = ((long long)blockIdx.x * 4 + k) * BE_BLOCK + threadIdx.x;
        if (w >= total) return;
        const long long o = w / a.C;
        a.o.feats[w] = a.feats[a.src[o] * a.C + (w - o * a.C)];
    }
}

// ---- _croppedInstanceIds per slot (pipeline.py:699-709) ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(BE_BLOCK) be_presence_kernel(BeArgs a) {
    const int o = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (o >= a.o.boff[a.B]) return;
    const BeSlot *__restrict__ sl = a.slots + a.slot_of[o];
    const int v = a.ids2[o];
    if (v >= 0 && v < sl->V) a.pres[sl->vbase + v] = 1;
}

__global__ void be_relabel_map_kernel(BeArgs a) {
    const int slot = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (slot >= a.B) return;
    const BeSlot *__restrict__ sl = a.slots + slot;
    sp_relabel_walk(a.pres + sl->vbase, sl->V, a.val_of + sl->vbase, a.orig_at + sl->vbase);
}

// sp_relabel_apply_kernel and sp_hist_kernel: hist has V + 1 entries per slot ([0]: the unlabelled points)
__global__ void __launch_bounds__(BE_BLOCK) be_apply_hist_kernel(BeArgs a) {
    const int o = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (o >= a.o.boff[a.B]) return;
    const int slot = a.slot_of[o];
    const BeSlot *__restrict__ sl = a.slots + slot;
    int v = a.ids2[o];
    if (v >= 0 && v < sl->V) {
        v = a.val_of[sl->vbase + v];
        a.ids2[o] = v;
    }
    if (v >= -1 && v < sl->V) atomicAdd(&a.hist[sl->vbase + slot + v + 1], 1);
}

// per slot rank / start (the exclusive scans of presence / count over the id values), K, Lp; then the totals across slots, the
// offset tables and the read-back table.  One block; B <= 512 threads do the per-slot walks, thread 0 the walk over slots.
__global__ void __launch_bounds__(BE_MAX_B) be_tables_kernel(BeArgs a) {
    const int slot = (int)threadIdx.x;
    if (slot < a.B) {
        const BeSlot *__restrict__ sl = a.slots + slot;
        const int V = sl->V;
        const int *hist = a.hist + sl->vbase + slot;
        int *rank = a.rank + sl->vbase, *start = a.start + sl->vbase;
        int r = 0, st = 0;
        for (int v = 0; v < V; v++) {
            rank[v] = r; start[v] = st;
            r += hist[v + 1] > 0; st += hist[v + 1];
        }
        a.sK[slot] = r; a.sLp[slot] = st; a.sUnl[slot] = hist[0] > 0;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    int I = 0, Q = 0;
    for (int s = 0; s < a.B; s++) {
        a.sI[s] = I; a.sQ[s] = Q;
        a.o.ioff[s] = I;
        int valid;
        int *rb = a.readback + BE_RB * s;
        rb[0] = a.o.boff[s + 1] - a.o.boff[s]; rb[1] = a.sK[s]; rb[2] = a.sLp[s];
        for (int k = 0; k < 6; k++) rb[3 + k] = a.real[6 * s + k];
        rb[9] = be_crop_ran(a.cnt + (size_t)s * a.T, a.slots[s].n, a.max_pt, a.T, &valid);
        I += a.sK[s]; Q += a.sLp[s];
    }
    a.o.ioff[a.B] = I;
    if (a.has_gt) a.o.gt_off[0] = 0;
}

// ---- instances (pipeline.py:711-772, :804-833) --------------------------------------------------------------------------------------------
// sp_keys_kernel over all slots: (slot, rank) -- unlabelled points behind every instance of their slot, unused rows behind every slot
__global__ void __launch_bounds__(BE_BLOCK) be_keys_kernel(BeArgs a) {
    const int o = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (o >= a.N) return;
    a.vals[o] = o;
    if (o >= a.o.boff[a.B]) { a.keys[o] = a.B << BE_KEY_BITS; return; }
    const int slot = a.slot_of[o];
    const BeSlot *__restrict__ sl = a.slots + slot;
    const int v = a.ids2[o];
    a.keys[o] = (slot << BE_KEY_BITS) | ((v >= 0 && v < sl->V) ? a.rank[sl->vbase + v] : a.sK[slot]);
}

// one wave per (slot, id value): sp_instance_kernel<double>'s count, exact min / max and sequential sum; batch_prep.hip's outputs
__global__ void __launch_bounds__(64) be_instance_kernel(BeArgs a) {
    extern __shared__ int s_prefix[];
    __shared__ double buf[64][3];
    const int lane = (int)threadIdx.x;
    const int slot = bp_find(s_prefix, a.vprefix, a.B), v = (int)blockIdx.x - s_prefix[slot];
    const BeSlot *__restrict__ sl = a.slots + slot;
    const int cnt = a.hist[sl->vbase + slot + v + 1];
    if (cnt == 0) return;
    const int st = a.start[sl->vbase + v], r = a.rank[sl->vbase + v];
    const int K = a.sK[slot], R = a.R, sh = a.sUnl[slot] ? 0 : 1, I = a.sI[slot];
    const int *__restrict__ sorted = a.sorted + a.o.boff[slot];
    double mn[3], mx[3], sum[3];
    for (int d = 0; d < 3; d++) { mn[d] = INFINITY; mx[d] = -INFINITY; sum[d] = 0.0; }
    for (int base = 0; base < cnt; base += 64) {
        int mm = cnt - base < 64 ? cnt - base : 64;
        if (lane < mm) {
            const size_t p = (size_t)sorted[st + base + lane];
            for (int d = 0; d < 3; d++) {
                double val = a.y2[3 * p + d];
                buf[lane][d] = val;
                mn[d] = val < mn[d] ? val : mn[d];
                mx[d] = val > mx[d] ? val : mx[d];
            }
        }
        __syncthreads();
        if (lane < 3)
            for (int q = 0; q < mm; q++) sum[lane] = sum[lane] + buf[q][lane];
        __syncthreads();
    }
    for (int off = 32; off > 0; off >>= 1)
        for (int d = 0; d < 3; d++) {
            double p = __shfl_xor(mn[d], off), q = __shfl_xor(mx[d], off);
            mn[d] = p < mn[d] ? p : mn[d];
            mx[d] = q > mx[d] ? q : mx[d];
        }
    double *__restrict__ is = a.istats + 9 * ((size_t)sl->vbase + v);
    if (lane < 3) {
        is[lane] = sum[lane] / (double)cnt;
        is[3 + lane] = mn[lane];
        is[6 + lane] = mx[lane];
    }
    if (lane != 0) return;
    a.o.num_point[I + r] = cnt;
    if (a.has_gt) a.o.gt_off[I + r + 1] = a.sQ[slot] + st + cnt;          // each instance writes its END: the next one's start
    // the box-slot rule of sp_instance_kernel / bp_stage2_kernel
    const int k = r - sh, kmax = K - 1 - sh;
    if (k >= 128 || k >= R) return;
    if (k < 0 && R - 1 < 128 && kmax >= R - 1) return;
    const long long row = (long long)slot * R + (k < 0 ? R - 1 : k);
    bp_box_row<double>(a.o, row, (int)a.o.sem[sorted[st]], v, mn, mx, a.mean_size);
}

__global__ void __launch_bounds__(64) be_boxrows_kernel(BeArgs a) {
    const int slot = (int)blockIdx.y;
    bp_unowned_rows(a.o, slot, a.R, a.sK[slot], a.sUnl[slot] ? 0 : 1, (int)blockIdx.x * 64 + (int)threadIdx.x);
}

// per kept point instance_ids (+ the instances before unless -1) and instance_info (sp_info_kernel<double>); per sorted position
// of a labelled point its gt_proposals_idx row (sp_gtidx_kernel with both shifts)
__global__ void __launch_bounds__(BE_BLOCK) be_info_kernel(BeArgs a) {
    const int o = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (o >= a.o.boff[a.B]) return;
    const int slot = a.slot_of[o];
    const BeSlot *__restrict__ sl = a.slots + slot;
    const int I = a.sI[slot];
    const int v = a.ids2[o];
    a.o.ids[o] = (long long)(v != -1 ? v + I : v);
    float f[12];
    if (v < 0 || v >= sl->V) {
        for (int c = 0; c < 12; c++) f[c] = 0.0f;
    } else {
        const double *q = a.istats + 9 * ((size_t)sl->vbase + v);
        for (int d = 0; d < 3; d++) {
            double mn = q[3 + d], mx = q[6 + d];
            f[d] = (float)q[d];
            f[3 + d] = (float)((mn + mx) / 2.0);
            f[6 + d] = (float)mn;
            f[9 + d] = (float)mx;
        }
    }
    float4 *io = (float4 *)(a.o.info + 12 * (size_t)o);                   // 48-byte rows from a 16-byte aligned base
    io[0] = make_float4(f[0], f[1], f[2], f[3]);
    io[1] = make_float4(f[4], f[5], f[6], f[7]);
    io[2] = make_float4(f[8], f[9], f[10], f[11]);
    if (!a.has_gt) return;
    const int p = o - a.o.boff[slot];                                     // the slot's sorted list starts at its first kept point
    if (p < a.sLp[slot]) {
        const int i = a.sorted[o];
        int2 *out = (int2 *)a.o.gt_idx + a.sQ[slot];
        out[p] = make_int2(a.rank[sl->vbase + a.ids2[i]] - (a.sUnl[slot] ? 0 : 1) + I, i);
    }
}

// ---- the table (host-built, one copy) and the workspace ------------------------------------------------------------------------------------
struct BeTable { BeSlot *slots; u64 *stats; int *cnt; double *u; int *pprefix, *gprefix[2], *vprefix; };
static void be_table_layout(D3Carver &c, int B, int T, BeTable &w) {
    w.slots = c.take<BeSlot>(B);
    w.stats = c.take<u64>(27 * (size_t)B);
    w.cnt = c.take<int>((size_t)B * T);
    w.u = c.take<double>(3 * (size_t)B * T);
    w.pprefix = c.take<int>((size_t)B + 1);
    w.gprefix[0] = c.take<int>((size_t)B + 1);
    w.gprefix[1] = c.take<int>((size_t)B + 1);
    w.vprefix = c.take<int>((size_t)B + 1);
}

struct BeWs {
    char *table;
    double *y, *s, *y2, *istats, *axes;
    int *flags, *pos, *ids2, *slot_of, *keys, *keys2, *vals, *sorted;
    long long *src;
    int *zeroed, *pres, *hist; size_t zeroed_bytes;
    int *val_of, *orig_at, *rank, *start, *dims, *real, *sK, *sLp, *sUnl, *sI, *sQ;
    float *grid[2];
    void *scan_t, *sort_t; size_t scan_b, sort_b;
};
static void be_ws_layout(D3Carver &c, size_t table_bytes, int B, long long N, long long Vt, long long axes, long long gfloats, BeWs &w) {
    const size_t n = (size_t)N, v = (size_t)Vt;
    w.table = c.take<char>(table_bytes);
    w.y = c.take<double>(3 * n); w.s = c.take<double>(3 * n); w.y2 = c.take<double>(3 * n);
    w.istats = c.take<double>(9 * v); w.axes = c.take<double>((size_t)axes);
    w.flags = c.take<int>(n); w.pos = c.take<int>(n); w.ids2 = c.take<int>(n); w.slot_of = c.take<int>(n);
    w.keys = c.take<int>(n); w.keys2 = c.take<int>(n); w.vals = c.take<int>(n); w.sorted = c.take<int>(n);
    w.src = c.take<long long>(n);
    const size_t z0 = c.off;
    w.pres = c.take<int>(v); w.hist = c.take<int>(v + (size_t)B);
    w.zeroed = w.pres; w.zeroed_bytes = c.off - z0;
    w.val_of = c.take<int>(v); w.orig_at = c.take<int>(v); w.rank = c.take<int>(v); w.start = c.take<int>(v);
    w.dims = c.take<int>(6 * (size_t)B); w.real = c.take<int>(6 * (size_t)B);
    w.sK = c.take<int>(B); w.sLp = c.take<int>(B); w.sUnl = c.take<int>(B); w.sI = c.take<int>(B); w.sQ = c.take<int>(B);
    w.grid[0] = c.take<float>((size_t)gfloats); w.grid[1] = c.take<float>((size_t)gfloats);
    w.scan_b = d3_scan_temp_bytes((int)N); w.sort_b = d3_sort_pairs_temp_bytes((int)N);
    w.scan_t = c.take<char>(w.scan_b); w.sort_t = c.take<char>(w.sort_b);
}

// the totals of a batch from slots_host (B,8) = n, V, the two bound shapes; false when something is out of range
struct BeTotals { long long N, Vt, axes, gfloats, tiles_p, tiles_g[2]; };
static bool be_totals(const int *slots_host, int B, int C, int T, BeTotals &t) {
    if (B < 1 || B > BE_MAX_B || T < 1 || T > BE_MAX_T || C < 0 || C > SP_MAX_FEAT || !slots_host) return false;
    const long long lim = 0x7fffffffll - 4096;
    t = BeTotals{0, 0, 0, 0, 0, {0, 0}};
    for (int i = 0; i < B; ++i) {
        const int *s = slots_host + 8 * i;
        const int n = s[0], V = s[1];
        if (n < 1 || n > SP_MAX_POINTS || V < 1 || V > SP_MAX_ID + 1) return false;     // a slot without points: points.min(0) raises
        long long cells = 0, ax = 0;
        for (int e = 0; e < 2; ++e) {
            const int *b = s + 2 + 3 * e;
            for (int d = 0; d < 3; ++d)
                if (b[d] < 3 || b[d] > SP_MAX_GRID_DIM) return false;
            const long long per = (long long)b[0] * b[1] * b[2];
            if (per > SP_MAX_GRID) return false;
            cells = per > cells ? per : cells;
            ax = (long long)b[0] + b[1] + b[2] > ax ? (long long)b[0] + b[1] + b[2] : ax;
            t.tiles_g[e] += (3 * per + BE_GTILE - 1) / BE_GTILE;
        }
        t.N += n; t.Vt += V; t.axes += ax; t.gfloats += 3 * cells;
        t.tiles_p += (n + BE_PTILE - 1) / BE_PTILE;
        if (t.N * (C > 12 ? C : 12) > lim || t.tiles_g[0] > lim || t.tiles_g[1] > lim) return false;
    }
    return true;
}

size_t d3_batch_elastic_table_bytes(int B, int T) {
    if (B < 1 || B > BE_MAX_B || T < 1 || T > BE_MAX_T) return 0;
    D3Carver c(nullptr, 0);
    BeTable w;
    be_table_layout(c, B, T, w);
    return c.off;
}

size_t d3_batch_elastic_ws_bytes(const int *slots_host, int B, int C, int T) {
    BeTotals t;
    if (!be_totals(slots_host, B, C, T, t)) return 0;
    D3Carver c(nullptr, 0);
    BeWs w;
    be_ws_layout(c, d3_batch_elastic_table_bytes(B, T), B, t.N, t.Vt, t.axes, t.gfloats, w);
    return c.off;
}

int d3_batch_elastic(const float *xyz, const float *feats, const int *sem, const int *ids, long long store_rows,
                     const long long *row0_host, const int *slots_host, const double *mats_host, const unsigned long long *seeds_host,
                     const double *crop_u_host, int B, int C, int R, int T, int has_gt, double scale, int gran0, int gran1,
                     double mag0, double mag1, double crop_scale, int max_num_point, const double *mean_size, void *const *out_host,
                     int *readback, void *table_host, void *ws, size_t ws_bytes, void *stream) {
    BeTotals tt;
    if (R < 1 || gran0 < 1 || gran1 < 1 || gran0 > 65536 || gran1 > 65536 || max_num_point < 0 || !be_totals(slots_host, B, C, T, tt)) return D3_ERR_RANGE;
    if ((long long)R * 24 > 0x7fffffffll - 4096 || (long long)((R + 63) / 64) > 65535) return D3_ERR_RANGE;
    if (!xyz || !sem || !ids || !row0_host || !mats_host || !seeds_host || !crop_u_host || !mean_size || !out_host || !readback ||
        !table_host || !ws || (C > 0 && !feats))
        return D3_ERR_ARG;
    for (int k = 0; k < 20; ++k)                              // every output is allocated at its upper bound
        if (!out_host[k] && !(k == 2 && C == 0) && !((k == 7 || k == 8) && !has_gt)) return D3_ERR_ARG;
    if (((size_t)out_host[3] | (size_t)out_host[4] | (size_t)out_host[12] | (size_t)out_host[13] | (size_t)out_host[15] |
         (size_t)out_host[17] | (size_t)out_host[18]) & 7)
        return D3_ERR_ARG;
    if (((size_t)out_host[1] | (size_t)out_host[5] | (size_t)out_host[19]) & 15) return D3_ERR_ARG;
    if (has_gt && ((size_t)out_host[7] & 7)) return D3_ERR_ARG;

    const size_t tb = d3_batch_elastic_table_bytes(B, T);
    D3Carver ch(table_host, tb);
    BeTable h;
    be_table_layout(ch, B, T, h);
    long long P = 0, Vt = 0, ax = 0, gf = 0, tp = 0, tg[2] = {0, 0}, tv = 0;
    for (int i = 0; i < B; ++i) {
        const int *s = slots_host + 8 * i;
        const long long row0 = row0_host[i];
        if (row0 < 0 || row0 + s[0] > store_rows) return D3_ERR_ARG;
        BeSlot &o = h.slots[i];
        o.row0 = row0; o.gbase = gf; o.seed = seeds_host[i];
        o.n = s[0]; o.P = (int)P; o.V = s[1]; o.vbase = (int)Vt; o.abase = (int)ax; o.pad = 0;
        long long cells = 0, a3 = 0;
        for (int e = 0; e < 2; ++e) {
            const int *b = s + 2 + 3 * e;
            for (int d = 0; d < 3; ++d) o.bnd[e][d] = b[d];
            const long long per = (long long)b[0] * b[1] * b[2];
            cells = per > cells ? per : cells;
            a3 = (long long)b[0] + b[1] + b[2] > a3 ? (long long)b[0] + b[1] + b[2] : a3;
            h.gprefix[e][i] = (int)tg[e];
            tg[e] += (3 * per + BE_GTILE - 1) / BE_GTILE;
        }
        for (int k = 0; k < 9; k++) o.m[k] = mats_host[9 * i + k];
        for (int st = 0; st < 3; ++st)
            for (int d = 0; d < 9; ++d) h.stats[27 * (size_t)i + 9 * st + d] = (d >= 3 && d < 6) ? ~0ull : 0ull;
        for (int k = 0; k < T; ++k) {
            h.cnt[(size_t)i * T + k] = 0;
            for (int d = 0; d < 3; ++d) h.u[3 * ((size_t)i * T + k) + d] = crop_u_host[3 * ((size_t)i * T + k) + d];
        }
        h.pprefix[i] = (int)tp; h.vprefix[i] = (int)tv;
        tp += (s[0] + BE_PTILE - 1) / BE_PTILE; tv += s[1];
        P += s[0]; Vt += s[1]; ax += a3; gf += 3 * cells;
    }
    h.pprefix[B] = (int)tp; h.vprefix[B] = (int)tv; h.gprefix[0][B] = (int)tg[0]; h.gprefix[1][B] = (int)tg[1];
    const int N = (int)P;

    D3Carver cw(ws, ws_bytes);
    BeWs w;
    be_ws_layout(cw, tb, B, tt.N, tt.Vt, tt.axes, tt.gfloats, w);
    if (!cw.ok()) return D3_ERR_WORKSPACE;
    D3Carver cd(w.table, tb);
    BeTable d;
    be_table_layout(cd, B, T, d);

    BeArgs a;
    a.xyz = xyz; a.feats = feats; a.sem = sem; a.ids = ids; a.mean_size = mean_size;
    a.slots = d.slots; a.stats = d.stats; a.cnt = d.cnt; a.u = d.u;
    a.pprefix = d.pprefix; a.gprefix[0] = d.gprefix[0]; a.gprefix[1] = d.gprefix[1]; a.vprefix = d.vprefix;
    a.y = w.y; a.s = w.s; a.y2 = w.y2; a.istats = w.istats; a.axes = w.axes;
    a.flags = w.flags; a.pos = w.pos; a.ids2 = w.ids2; a.slot_of = w.slot_of; a.keys = w.keys; a.vals = w.vals; a.sorted = w.sorted;
    a.src = w.src; a.pres = w.pres; a.hist = w.hist; a.val_of = w.val_of; a.orig_at = w.orig_at; a.rank = w.rank; a.start = w.start;
    a.dims = w.dims; a.real = w.real; a.sK = w.sK; a.sLp = w.sLp; a.sUnl = w.sUnl; a.sI = w.sI; a.sQ = w.sQ;
    a.grid[0] = w.grid[0]; a.grid[1] = w.grid[1]; a.readback = readback;
    a.B = B; a.C = C; a.R = R; a.T = T; a.has_gt = has_gt ? 1 : 0; a.N = N; a.max_pt = max_num_point;
    a.gran[0] = gran0; a.gran[1] = gran1; a.scale = scale; a.mag[0] = mag0; a.mag[1] = mag1; a.crop_scale = crop_scale;
    void *const *p = out_host;
    a.o = BpOut{(float *)p[0], (long long *)p[1], (float *)p[2], (long long *)p[3], (long long *)p[4], (float *)p[5], (int *)p[6],
                (int *)p[7], (int *)p[8], (int *)p[9], (int *)p[10], (float *)p[11], (long long *)p[12], (long long *)p[13],
                (float *)p[14], (long long *)p[15], (float *)p[16], (long long *)p[17], (long long *)p[18], (float *)p[19]};

    hipStream_t st = d3_stream(stream);
    const size_t lds = ((size_t)B + 1) * sizeof(int);
    const dim3 blk(BE_BLOCK), pgrid((unsigned)tp), flat((unsigned)((N + BE_BLOCK - 1) / BE_BLOCK)), perslot((unsigned)((B + 63) / 64));
    D3_CLEAR();
    // ONE copy: table_host is the caller's pinned buffer and must stay as it is until the copy has run
    D3_CHECK(hipMemcpyAsync(w.table, table_host, ch.off, hipMemcpyHostToDevice, st));
    D3_CHECK(hipMemsetAsync(w.zeroed, 0, w.zeroed_bytes, st));
    hipLaunchKernelGGL(be_transform_kernel, pgrid, blk, lds, st, a);
    D3_LAUNCH_CHECK();
    for (int e = 0; e < 2; ++e) {
        hipLaunchKernelGGL(be_resolve_kernel, perslot, dim3(64), 0, st, a, e);
        D3_LAUNCH_CHECK();
        hipLaunchKernelGGL(be_noise_kernel, dim3((unsigned)tg[e]), blk, lds, st, a, e);
        D3_LAUNCH_CHECK();
        for (int pass = 0; pass < 6; ++pass) {                // x, y, z, x, y, z; an even count ends back in grid[0]
            hipLaunchKernelGGL(be_blur_kernel, dim3((unsigned)tg[e]), blk, lds, st, a, e, pass % 3, pass & 1);
            D3_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(be_interp_kernel, pgrid, blk, lds, st, a, e);
        D3_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(be_offset_kernel, pgrid, blk, lds, st, a);
    D3_LAUNCH_CHECK();
    for (int j = 0; j < T; ++j) {
        hipLaunchKernelGGL(be_crop_kernel, pgrid, blk, lds, st, a, j);
        D3_LAUNCH_CHECK();
    }
    int rc = d3_exclusive_scan_i32(w.flags, w.pos, N, w.scan_t, w.scan_b, st);
    if (rc) return rc;
    hipLaunchKernelGGL(be_emit_kernel, pgrid, blk, lds, st, a);
    D3_LAUNCH_CHECK();
    if (C > 0) {
        const long long words = (long long)N * C;
        hipLaunchKernelGGL(be_feats_kernel, dim3((unsigned)((words + 4 * BE_BLOCK - 1) / (4 * BE_BLOCK))), blk, 0, st, a);
        D3_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(be_presence_kernel, flat, blk, 0, st, a);
    D3_LAUNCH_CHECK();
    hipLaunchKernelGGL(be_relabel_map_kernel, perslot, dim3(64), 0, st, a);
    D3_LAUNCH_CHECK();
    hipLaunchKernelGGL(be_apply_hist_kernel, flat, blk, 0, st, a);
    D3_LAUNCH_CHECK();
    hipLaunchKernelGGL(be_tables_kernel, dim3(1), dim3(BE_MAX_B), 0, st, a);
    D3_LAUNCH_CHECK();
    hipLaunchKernelGGL(be_keys_kernel, flat, blk, 0, st, a);
    D3_LAUNCH_CHECK();
    int bits = BE_KEY_BITS + 1;
    while ((1 << bits) <= (B << BE_KEY_BITS)) bits++;
    rc = d3_sort_pairs_i32(w.keys, w.keys2, w.vals, w.sorted, N, bits, w.sort_t, w.sort_b, st);
    if (rc) return rc;
    hipLaunchKernelGGL(be_instance_kernel, dim3((unsigned)tv), dim3(64), lds, st, a);
    D3_LAUNCH_CHECK();
    hipLaunchKernelGGL(be_boxrows_kernel, dim3((unsigned)((R + 63) / 64), (unsigned)B), dim3(64), 0, st, a);
    D3_LAUNCH_CHECK();
    hipLaunchKernelGGL(be_info_kernel, flat, blk, 0, st, a);
    D3_LAUNCH_CHECK();
    return 0;
}
