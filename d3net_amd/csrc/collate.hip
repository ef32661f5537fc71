// collate.hip -- the batch stacking of the reference's `sparse_collate_fn` (lib/dataset/pipeline.py:917-) over per-scene samples
// that already live on the device (driven by d3net_amd/scene_prep.py:collate_scenes_device): every concatenation, the scene-index
// column and float -> int64 truncation of locs_scaled, the int32 -> int64 label casts, the instance / point shifts of
// instance_ids, gt_proposals_idx and gt_proposals_offset, the two offset tables and the nine stacked box labels -- ONE launch.
//
// The host turns the batch into a list of copy jobs (one per scene and array with something to copy), each cut into tiles of
// CT_TILE output units; the grid is flat over all tiles.  A block finds its job by binary search in the tile-prefix table, which
// it first loads into LDS.  Every output element has exactly one writer: plain vector stores, no atomics, no memsets.
#include "common.h"

#define CT_BLOCK 256
#define CT_TILE 1024                  // output units per block: 4 per thread
#define CT_MAX_B 512                  // scenes per batch: the prefix table of (20 * B + 3) ints stays inside 64 KiB of LDS
#define CT_NPTR 18                    // per-scene input pointers
#define CT_NOUT 20                    // output pointers
#define CT_NBOX 9

enum { CT_WORDS = 0, CT_F2L = 1, CT_I2L = 2 };

// count units from src to dst.  CT_WORDS: 32-bit words, word w stored as src[w] + (w odd ? p1 : p0) in unsigned arithmetic (a
// float copy is the add of 0 to its bits); CT_F2L: rows of 3 float -> rows of 4 int64 [p0, trunc x, trunc y, trunc z];
// CT_I2L: int32 v -> int64 (v != -1 ? v + p0 : v), the add in int32 as torch's `ii + total_inst` before `.long()`.
struct CtJob { const void *src; void *dst; int count, kind, p0, p1; };

__device__ __forceinline__ long long ct_shift(int v, int add) { return (long long)(v != -1 ? v + add : v); }

__global__ void __launch_bounds__(CT_BLOCK)
ct_collate_kernel(const CtJob *__restrict__ jobs, const int *__restrict__ prefix, int J) {
    extern __shared__ int s_prefix[];                     // J + 1 entries, prefix[J] = gridDim.x
    const int t = (int)threadIdx.x;
    for (int i = t; i <= J; i += CT_BLOCK) s_prefix[i] = prefix[i];
    __syncthreads();
    const int b = (int)blockIdx.x;
    int lo = 0, hi = J;                                   // s_prefix[lo] <= b < s_prefix[hi]; every listed job has >= 1 tile
    while (hi - lo > 1) {
        int mid = (lo + hi) >> 1;
        if (s_prefix[mid] <= b) lo = mid; else hi = mid;
    }
    const CtJob jb = jobs[lo];
    const int base = (b - s_prefix[lo]) * CT_TILE, count = jb.count;
    const size_t align = (size_t)jb.src | (size_t)jb.dst;

    if (jb.kind == CT_WORDS) {
        const unsigned *__restrict__ src = (const unsigned *)jb.src;
        unsigned *__restrict__ dst = (unsigned *)jb.dst;
        const unsigned a0 = (unsigned)jb.p0, a1 = (unsigned)jb.p1;
        if ((align & 15) == 0) {                          // 16-byte accesses; base and 4 * t are even, so x / z take a0
            int w = base + 4 * t;
            if (w + 4 <= count) {
                uint4 v = *(const uint4 *)(src + w);
                v.x += a0; v.y += a1; v.z += a0; v.w += a1;
                *(uint4 *)(dst + w) = v;
            } else {
                for (; w < count; ++w) dst[w] = src[w] + ((w & 1) ? a1 : a0);
            }
        } else {                                          // lane-consecutive words
            for (int k = 0; k < CT_TILE / CT_BLOCK; ++k) {
                int w = base + t + k * CT_BLOCK;
                if (w < count) dst[w] = src[w] + ((w & 1) ? a1 : a0);
            }
        }
    } else if (jb.kind == CT_F2L) {                       // dst rows are 32 bytes from a 16-byte aligned base (checked by the host)
        const float *__restrict__ src = (const float *)jb.src;
        longlong2 *__restrict__ dst = (longlong2 *)jb.dst;
        for (int k = 0; k < CT_TILE / CT_BLOCK; ++k) {
            int r = base + t + k * CT_BLOCK;
            if (r < count) {
                float x = src[3 * (size_t)r], y = src[3 * (size_t)r + 1], z = src[3 * (size_t)r + 2];
                dst[2 * (size_t)r] = make_longlong2((long long)jb.p0, (long long)x);
                dst[2 * (size_t)r + 1] = make_longlong2((long long)y, (long long)z);
            }
        }
    } else {
        const int *__restrict__ src = (const int *)jb.src;
        long long *__restrict__ dst = (long long *)jb.dst;
        const int add = jb.p0;
        if (((size_t)jb.dst & 15) == 0 && ((size_t)jb.src & 7) == 0) {      // pairs: 8-byte loads, 16-byte stores
            for (int k = 0; k < CT_TILE / (2 * CT_BLOCK); ++k) {
                int e = base + 2 * (t + k * CT_BLOCK);
                if (e + 2 <= count) {
                    int2 v = *(const int2 *)(src + e);
                    *(longlong2 *)(dst + e) = make_longlong2(ct_shift(v.x, add), ct_shift(v.y, add));
                } else if (e < count) {
                    dst[e] = ct_shift(src[e], add);
                }
            }
        } else {
            for (int k = 0; k < CT_TILE / CT_BLOCK; ++k) {
                int e = base + t + k * CT_BLOCK;
                if (e < count) dst[e] = ct_shift(src[e], add);
            }
        }
    }
}

// the table the call builds in host memory and copies to the device as it stands
struct CtTable { CtJob *jobs; int *prefix, *boff, *ioff; };
static void ct_layout(D3Carver &c, int B, CtTable &w) {
    w.jobs = c.take<CtJob>((size_t)CT_NOUT * B + 2);
    w.prefix = c.take<int>((size_t)CT_NOUT * B + 3);
    w.boff = c.take<int>(B + 1);
    w.ioff = c.take<int>(B + 1);
}

size_t d3_collate_table_bytes(int B) {
    if (B < 1 || B > CT_MAX_B) return 0;
    D3Carver c(nullptr, 0);
    CtTable w;
    ct_layout(c, B, w);
    return c.off;
}

int d3_collate_scenes(const void *const *ptrs_host, const int *counts_host, int B, int C, int R, int has_gt, void *const *out_host,
                      void *table_host, void *table_dev, size_t table_bytes, void *stream) {
    // words per box-label row, in the order of scene_prep._BOX_KEYS (int64 keys count two words)
    static const int box_words[CT_NBOX] = {3, 2, 2, 1, 2, 3, 2, 2, 24};
    if (C < 0 || R < 0 || !ptrs_host || !counts_host || !out_host || !table_host || !table_dev) return D3_ERR_ARG;
    if (B < 1 || B > CT_MAX_B) return D3_ERR_RANGE;
    D3Carver ch(table_host, table_bytes), cd(table_dev, table_bytes);
    CtTable h, d;
    ct_layout(ch, B, h);
    ct_layout(cd, B, d);
    if (!ch.ok() || !cd.ok()) return D3_ERR_WORKSPACE;
    if (((size_t)out_host[1] | (size_t)out_host[3] | (size_t)out_host[4]) & 7) return D3_ERR_ARG;       // the int64 outputs
    if ((size_t)out_host[1] & 15) return D3_ERR_ARG;
    const long long lim = 0x7fffffffll - CT_TILE;
    long long P = 0, I = 0, Q = 0;                        // running points, instances, proposal entries
    for (int i = 0; i < B; ++i) {
        const int n = counts_host[3 * i], K = counts_host[3 * i + 1], Lp = counts_host[3 * i + 2];
        if (n < 0 || K < 0 || Lp < 0) return D3_ERR_ARG;
        if ((long long)n * (C > 12 ? C : 12) > lim || (long long)R * 24 > lim) return D3_ERR_RANGE;
        P += n; I += K; Q += Lp;
    }
    if (P > lim || I > lim || Q > lim) return D3_ERR_RANGE;

    int J = 0;
    long long tiles = 0;
    bool bad = false;
    auto job = [&](const void *src, void *dst, size_t dst_off_bytes, long long count, int kind, int p0, int p1) {
        if (count <= 0) return;
        if (!src || !dst) { bad = true; return; }
        h.prefix[J] = (int)tiles;
        h.jobs[J++] = CtJob{src, (void *)((size_t)dst + dst_off_bytes), (int)count, kind, p0, p1};
        tiles += (count + CT_TILE - 1) / CT_TILE;
    };
    P = I = Q = 0;
    for (int i = 0; i < B; ++i) {
        const void *const *p = ptrs_host + (size_t)CT_NPTR * i;
        const int n = counts_host[3 * i], K = counts_host[3 * i + 1], Lp = counts_host[3 * i + 2];
        h.boff[i] = (int)P; h.ioff[i] = (int)I;
        job(p[0], out_host[0], (size_t)P * 12, (long long)n * 3, CT_WORDS, 0, 0);                       // locs
        job(p[1], out_host[1], (size_t)P * 32, n, CT_F2L, i, 0);                                       // locs_scaled
        job(p[2], out_host[2], (size_t)P * C * 4, (long long)n * C, CT_WORDS, 0, 0);                   // feats
        job(p[3], out_host[3], (size_t)P * 8, n, CT_I2L, 0, 0);                                        // sem_labels
        job(p[4], out_host[4], (size_t)P * 8, n, CT_I2L, (int)I, 0);                                   // instance_ids
        job(p[5], out_host[5], (size_t)P * 48, (long long)n * 12, CT_WORDS, 0, 0);                     // instance_info
        job(p[6], out_host[6], (size_t)I * 4, K, CT_WORDS, 0, 0);                                      // instance_num_point
        if (has_gt) {
            job(p[7], out_host[7], (size_t)Q * 8, (long long)Lp * 2, CT_WORDS, (int)I, (int)P);        // gt_proposals_idx
            // gt_proposals_offset: K + 1 entries, the leading 0 dropped after the first scene, shifted by the entries so far
            if (!p[8]) bad = true;
            else if (i == 0) job(p[8], out_host[8], 0, (long long)K + 1, CT_WORDS, 0, 0);
            else job((const int *)p[8] + 1, out_host[8], (size_t)(I + 1) * 4, K, CT_WORDS, (int)Q, (int)Q);
        }
        for (int k = 0; k < CT_NBOX; ++k) {
            const long long words = (long long)R * box_words[k];
            job(p[9 + k], out_host[11 + k], (size_t)i * words * 4, words, CT_WORDS, 0, 0);
        }
        P += n; I += K; Q += Lp;
    }
    h.boff[B] = (int)P; h.ioff[B] = (int)I;
    job(d.boff, out_host[9], 0, B + 1, CT_WORDS, 0, 0);                                                // batch_offsets
    job(d.ioff, out_host[10], 0, B + 1, CT_WORDS, 0, 0);                                               // instance_offsets
    if (bad) return D3_ERR_ARG;
    if (tiles > 0x7fffffffll) return D3_ERR_RANGE;
    h.prefix[J] = (int)tiles;

    hipStream_t st = d3_stream(stream);
    D3_CLEAR();
    // ONE copy: table_host is the caller's pinned buffer and must stay as it is until the copy has run
    D3_CHECK(hipMemcpyAsync(table_dev, table_host, ch.off, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(ct_collate_kernel, dim3((unsigned)tiles), dim3(CT_BLOCK), (size_t)(J + 1) * sizeof(int), st,
                       (const CtJob *)d.jobs, (const int *)d.prefix, J);
    D3_LAUNCH_CHECK();
    return 0;
}
