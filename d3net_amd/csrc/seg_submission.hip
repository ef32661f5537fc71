// seg_submission.hip -- the ScanNet segmentation submission files as text on the device (gfx950): what PointGroup.test() leaves
// under <root>/split_pred/<split>/ (reference model/pointgroup.py:543-625) and the GT encoding of lib/utils/eval.py:14-56, without
// the host route's per-file np.savetxt (d3net_amd/seg_eval.py:write_predictions / write_gt, which stay the yardstick: every byte
// produced here equals theirs).  The host (d3net_amd/seg_submission.py) plans tiles and chunks, reads the buffers back and writes
// slices of them to files; it formats nothing but the few lines of instance/<scene>.txt.
//
//   ss_table_kernel   ONE workgroup.  Per picked proposal, in pick order: the scene of its first member (binary search of
//                     batch_offsets), its scene-local id c_id (the number of earlier picks of that scene), its class (the LUT at
//                     semantic_pred of the first member), its score's bits; an empty member list is skipped (`if len(m)`).  Picks
//                     go through LDS in rounds of 256: a thread counts the same-scene picks before it in the round and adds the
//                     scene's running count, held in LDS; the last pick of a scene in the round advances that count.
//   ss_fill_i32       cluster ids = -1.
//   ss_ids_kernel     blocks (pick, part): every member entry of a picked proposal does atomicMax(ids[point], c_id) -- c_id grows
//                     with pick order, so the maximum is the LAST pick that holds the point; integer atomics, the result does not
//                     depend on scheduling.  A member outside the first member's scene is skipped.
//   integer lines     np.savetxt(fmt="%d") over segments, for one or two texts that share the segments, in three launches on one
//                     stream.  A segment is cut into tiles of SS_TILE lines; the grids of launches 1 and 3 are flat over
//                     (text, tile) and a block finds its segment by binary search of the host's tile-prefix table.
//                       1 ss_tile_bytes_kernel  per tile the byte total of its lines
//                       2 ss_seg_scan_kernel    per (text, segment) the exclusive scan of its tiles' totals and the segment's length
//                       3 ss_lines_kernel       per tile the line lengths again, a block scan, the text dense in LDS, then out as
//                                               dwords.  Segment b's text starts at byte offsets[b] * width and is dense from there.
//                     A value whose text exceeds `width` bytes (newline included) sets status bit 1 and prints as 0; a value outside
//                     its LUT sets bit 2 and is clamped; an inconsistent table sets bit 4 and the tile stores nothing.
//   ss_mask_fill / ss_mask_ones   m mask files of one scene: "0\n" everywhere by 16-byte stores, then '1' at 2 (c n + i - lo) for
//                     every member i of chunk proposal c, byte stores; equal bytes where two members meet.
//
// No kernel waits for another workgroup: ordering is launch order on the stream.  Plain vector stores and integer atomics only.
#include "common.h"

#define SS_BLOCK 256
#define SS_WAVES (SS_BLOCK / 64)
#define SS_PER_THREAD 4
#define SS_TILE (SS_BLOCK * SS_PER_THREAD)      // 1024 lines per tile
#define SS_MAX_WIDTH 12                         // "-2147483648\n"
#define SS_MAX_B 4096                           // scenes per batch: the running counts of ss_table_kernel stay in 16 KiB of LDS
#define SS_MAX_PICKS (1 << 20)
#define SS_PARTS 8                              // blocks per picked proposal of ss_ids_kernel / ss_mask_ones_kernel
#define SS_COLS 5                               // table row: scene, c_id, class, flags, score bits

struct SsText { const int *values; const int *lut; int nlut, width; char *text; long long *lens; };
struct SsTexts { SsText t[2]; };

__device__ __forceinline__ int ss_ndigits(unsigned u) {
    return 1 + (u >= 10u) + (u >= 100u) + (u >= 1000u) + (u >= 10000u) + (u >= 100000u) + (u >= 1000000u) + (u >= 10000000u) +
           (u >= 100000000u) + (u >= 1000000000u);
}

// the last b in [0, B) with table[b] <= x, for a nondecreasing table with table[0] <= x < table[B]
__device__ __forceinline__ int ss_search(const int *__restrict__ table, int B, int x) {
    int lo = 0, hi = B;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (table[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

// ------------------------------------------------------------------------------------------------- cluster table
__global__ __launch_bounds__(SS_BLOCK) void ss_table_kernel(const int *__restrict__ pick, int n, const int *__restrict__ pidx, int L,
                                                            const int *__restrict__ poff, int P, const int *__restrict__ sem,
                                                            const float *__restrict__ scores, int N, const int *__restrict__ boff,
                                                            int B, const int *__restrict__ lut, int nlut, int *__restrict__ table,
                                                            int *__restrict__ counts, int *__restrict__ status) {
    __shared__ int s_count[SS_MAX_B];
    __shared__ int s_scene[SS_BLOCK];
    const int t = (int)threadIdx.x;
    for (int b = t; b < B; b += SS_BLOCK) s_count[b] = 0;
    for (int j0 = 0; j0 < n; j0 += SS_BLOCK) {
        const int j = j0 + t;
        int scene = -1, cls = 0, flags = 0, bad = 0;
        if (j < n) {
            const int p = pick[j];
            if (p < 0 || p >= P) { bad = 4; }
            else {
                const int s = poff[p], e = poff[p + 1];
                if (s < 0 || e > L || e < s) bad = 4;
                else if (e > s) {
                    const int first = pidx[2 * (size_t)s + 1];
                    if (first < 0 || first >= N) bad = 4;
                    else if (first >= boff[0] && first < boff[B]) {
                        scene = ss_search(boff, B, first);
                        int sp = sem[first];
                        if (sp < 0 || sp >= nlut) { bad = 2; sp = sp < 0 ? 0 : nlut - 1; }
                        cls = lut[sp];
                    }
                }
            }
            if (bad) atomicOr(status, bad);
            if (scene < 0) flags = 1;                       // skipped: empty, malformed or in no scene
        }
        __syncthreads();                                    // (the round before has read s_scene and written s_count)
        s_scene[t] = scene;
        __syncthreads();
        int before = 0, after = 0;
        if (scene >= 0) {
            for (int k = 0; k < SS_BLOCK; k++) {
                const int same = s_scene[k] == scene;
                before += same & (k < t);
                after += same & (k > t);
            }
        }
        const int c_id = scene >= 0 ? s_count[scene] + before : -1;
        __syncthreads();
        if (scene >= 0 && after == 0) s_count[scene] = c_id + 1;
        if (j < n) {
            int *row = table + (size_t)j * SS_COLS;
            row[0] = scene; row[1] = c_id; row[2] = cls; row[3] = flags; row[4] = __float_as_int(scores[j]);
        }
    }
    __syncthreads();
    for (int b = t; b < B; b += SS_BLOCK) counts[b] = s_count[b];
}

// ------------------------------------------------------------------------------------------------- per-point cluster id
__global__ __launch_bounds__(SS_BLOCK) void ss_fill_i32(int *__restrict__ dst, long long n, int value) {
    const long long i = (long long)blockIdx.x * SS_BLOCK + threadIdx.x;
    if (i < n) dst[i] = value;
}

__global__ __launch_bounds__(SS_BLOCK) void ss_ids_kernel(const int *__restrict__ table, const int *__restrict__ pick,
                                                          const int *__restrict__ pidx, int L, const int *__restrict__ poff, int P,
                                                          const int *__restrict__ boff, int B, int N, int *__restrict__ ids) {
    const int j = (int)(blockIdx.x / SS_PARTS), part = (int)(blockIdx.x % SS_PARTS);
    const int *row = table + (size_t)j * SS_COLS;
    const int scene = row[0], c_id = row[1];
    if (scene < 0 || scene >= B) return;                    // a skipped pick
    const int p = pick[j];
    if (p < 0 || p >= P) return;
    int s = poff[p], e = poff[p + 1];
    s = s < 0 ? 0 : s; e = e > L ? L : e;
    int lo = boff[scene], hi = boff[scene + 1];
    lo = lo < 0 ? 0 : lo; hi = hi > N ? N : hi;
    for (long long k = (long long)s + part * SS_BLOCK + threadIdx.x; k < e; k += SS_PARTS * SS_BLOCK) {
        const int i = pidx[2 * (size_t)k + 1];
        if (i >= lo && i < hi) atomicMax(ids + i, c_id);
    }
}

// ------------------------------------------------------------------------------------------------- integer lines
struct SsTile { int b, cnt; long long start; };

// tile g's segment, first line and line count; cnt = 0 and status bit 4 when the tables do not fit the values
__device__ __forceinline__ SsTile ss_locate(const int *__restrict__ offsets, const int *__restrict__ prefix, int B, int g, long long n_values,
                                            int *__restrict__ status) {
    SsTile r;
    r.b = ss_search(prefix, B, g);
    r.start = (long long)offsets[r.b] + (long long)(g - prefix[r.b]) * SS_TILE;
    const long long left = (long long)offsets[r.b + 1] - r.start;
    r.cnt = (int)(left < SS_TILE ? left : SS_TILE);
    if (r.start < 0 || r.cnt < 0 || r.start + r.cnt > n_values || g < prefix[r.b]) {
        r.cnt = 0;
        if (threadIdx.x == 0) atomicOr(status, 4);
    }
    return r;
}

// the thread's SS_PER_THREAD consecutive lines of the tile: the values as printed (LUT applied, clamped) and their lengths; -> the sum
__device__ __forceinline__ int ss_lines_of(const SsText &tx, const SsTile &tile, int t, int (&val)[SS_PER_THREAD], int (&len)[SS_PER_THREAD],
                                           int *__restrict__ status) {
    int sum = 0, bad = 0;
#pragma unroll
    for (int k = 0; k < SS_PER_THREAD; k++) {
        const int i = t * SS_PER_THREAD + k;
        int v = 0, l = 0;
        if (i < tile.cnt) {
            v = tx.values[tile.start + i];
            if (tx.lut) {
                if (v < 0 || v >= tx.nlut) { bad |= 2; v = v < 0 ? 0 : tx.nlut - 1; }
                v = tx.lut[v];
            }
            const unsigned u = v < 0 ? 0u - (unsigned)v : (unsigned)v;
            l = (v < 0) + ss_ndigits(u) + 1;
            if (l > tx.width) { bad |= 1; v = 0; l = 2; }
        }
        val[k] = v; len[k] = l;
        sum += l;
    }
    if (bad) atomicOr(status, bad);
    return sum;
}

// exclusive scan of `mine` over the block -> the thread's offset; total the block's sum
__device__ __forceinline__ int ss_block_scan(int mine, int *s_wave, int &total) {
    const int t = (int)threadIdx.x, lane = t & 63, w = t >> 6;
    int incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(incl, d);
        if (lane >= d) incl += up;
    }
    if (lane == 63) s_wave[w] = incl;
    __syncthreads();
    int base = incl - mine;
    total = 0;
#pragma unroll
    for (int i = 0; i < SS_WAVES; i++) { if (i < w) base += s_wave[i]; total += s_wave[i]; }
    __syncthreads();                                        // s_wave may be written again
    return base;
}

__global__ __launch_bounds__(SS_BLOCK) void ss_tile_bytes_kernel(SsTexts texts, long long n_values, const int *__restrict__ offsets,
                                                                 const int *__restrict__ prefix, int B, int tiles,
                                                                 int *__restrict__ tile_bytes, int *__restrict__ status) {
    __shared__ int s_wave[SS_WAVES];
    const int slot = (int)(blockIdx.x / tiles), g = (int)(blockIdx.x % tiles);
    const SsText tx = slot ? texts.t[1] : texts.t[0];       // (a select: no dynamic index into the argument)
    const SsTile tile = ss_locate(offsets, prefix, B, g, n_values, status);
    int val[SS_PER_THREAD], len[SS_PER_THREAD], total;
    const int mine = ss_lines_of(tx, tile, (int)threadIdx.x, val, len, status);
    ss_block_scan(mine, s_wave, total);
    if (threadIdx.x == 0) tile_bytes[(size_t)slot * tiles + g] = total;
}

// block (text, segment): tile_off = exclusive scan of the segment's tile totals, lens[b] = their sum (0 for a segment without tiles)
__global__ __launch_bounds__(SS_BLOCK) void ss_seg_scan_kernel(SsTexts texts, const int *__restrict__ prefix, int B, int tiles,
                                                               const int *__restrict__ tile_bytes, int *__restrict__ tile_off) {
    __shared__ int s_wave[SS_WAVES];
    const int slot = (int)(blockIdx.x / B), b = (int)(blockIdx.x % B);
    int g0 = prefix[b], g1 = prefix[b + 1];
    g0 = g0 < 0 ? 0 : g0; g1 = g1 > tiles ? tiles : g1;
    long long carry = 0;
    for (int c = g0; c < g1; c += SS_BLOCK) {
        const int g = c + (int)threadIdx.x;
        const int mine = g < g1 ? tile_bytes[(size_t)slot * tiles + g] : 0;
        int total;
        const int base = ss_block_scan(mine, s_wave, total);
        if (g < g1) tile_off[(size_t)slot * tiles + g] = (int)(carry + base);     // < n_values * width <= INT_MAX (checked by the host)
        carry += total;
    }
    if (threadIdx.x == 0) (slot ? texts.t[1].lens : texts.t[0].lens)[b] = carry;
}

__global__ __launch_bounds__(SS_BLOCK) void ss_lines_kernel(SsTexts texts, long long n_values, const int *__restrict__ offsets,
                                                            const int *__restrict__ prefix, int B, int tiles,
                                                            const int *__restrict__ tile_off, int *__restrict__ status) {
    __shared__ __attribute__((aligned(16))) char s_text[SS_TILE * SS_MAX_WIDTH];
    __shared__ int s_wave[SS_WAVES];
    const int slot = (int)(blockIdx.x / tiles), g = (int)(blockIdx.x % tiles), t = (int)threadIdx.x;
    const SsText tx = slot ? texts.t[1] : texts.t[0];       // (a select: no dynamic index into the argument)
    const SsTile tile = ss_locate(offsets, prefix, B, g, n_values, status);
    int val[SS_PER_THREAD], len[SS_PER_THREAD], total;
    const int mine = ss_lines_of(tx, tile, t, val, len, status);
    int at = ss_block_scan(mine, s_wave, total);
#pragma unroll
    for (int k = 0; k < SS_PER_THREAD; k++) {
        if (len[k]) {
            const int v = val[k];
            unsigned u = v < 0 ? 0u - (unsigned)v : (unsigned)v;
            int p = at + len[k] - 1;                        // < total <= SS_TILE * width <= sizeof s_text
            s_text[p] = '\n';
            do { s_text[--p] = (char)('0' + (int)(u % 10u)); u /= 10u; } while (u);
            if (v < 0) s_text[--p] = '-';
            at += len[k];
        }
    }
    __syncthreads();
    const long long base = (long long)offsets[tile.b] * tx.width + tile_off[(size_t)slot * tiles + g];
    if (total == 0) return;
    if (base < 0 || base + total > n_values * tx.width) {   // (cannot happen with the tables of launches 1 and 2)
        if (t == 0) atomicOr(status, 4);
        return;
    }
    char *dst = tx.text + base;
    int head = (int)((0 - (size_t)dst) & 3);                // bytes up to the first aligned dword
    head = head > total ? total : head;
    if (t < head) dst[t] = s_text[t];
    const int ndw = (total - head) >> 2;
    unsigned *dw = (unsigned *)(dst + head);
    for (int q = t; q < ndw; q += SS_BLOCK) {
        const char *s = s_text + head + 4 * q;
        dw[q] = (unsigned)(unsigned char)s[0] | ((unsigned)(unsigned char)s[1] << 8) | ((unsigned)(unsigned char)s[2] << 16) |
                ((unsigned)(unsigned char)s[3] << 24);
    }
    const int done = head + 4 * ndw;
    if (t < total - done) dst[done + t] = s_text[done + t];
}

// ------------------------------------------------------------------------------------------------- mask lines
__global__ __launch_bounds__(SS_BLOCK) void ss_mask_fill(uint4 *__restrict__ dst, long long n16) {
    const uint4 zero_lines = make_uint4(0x0a300a30u, 0x0a300a30u, 0x0a300a30u, 0x0a300a30u);     // "0\n" eight times
    for (long long i = (long long)blockIdx.x * SS_BLOCK + threadIdx.x; i < n16; i += (long long)gridDim.x * SS_BLOCK) dst[i] = zero_lines;
}

__global__ __launch_bounds__(SS_BLOCK) void ss_mask_ones_kernel(const int *__restrict__ table, const int *__restrict__ pick,
                                                                const int *__restrict__ pidx, int L, const int *__restrict__ poff, int P,
                                                                int scene, int lo, int npts, int c_lo, int m, char *__restrict__ text) {
    const int j = (int)(blockIdx.x / SS_PARTS), part = (int)(blockIdx.x % SS_PARTS);
    const int *row = table + (size_t)j * SS_COLS;
    const int c = row[1] - c_lo;
    if (row[0] != scene || c < 0 || c >= m) return;         // another scene's, another chunk's or a skipped pick
    const int p = pick[j];
    if (p < 0 || p >= P) return;
    int s = poff[p], e = poff[p + 1];
    s = s < 0 ? 0 : s; e = e > L ? L : e;
    char *file = text + 2 * (size_t)c * (size_t)npts;
    for (long long k = (long long)s + part * SS_BLOCK + threadIdx.x; k < e; k += SS_PARTS * SS_BLOCK) {
        const int i = pidx[2 * (size_t)k + 1] - lo;
        if (i >= 0 && i < npts) file[2 * (size_t)i] = '1';
    }
}

// ------------------------------------------------------------------------------------------------- host
extern "C" int d3_seg_submit_limits(int *tile_lines, int *max_width, int *max_scenes, int *table_cols) {
    if (tile_lines) *tile_lines = SS_TILE;
    if (max_width) *max_width = SS_MAX_WIDTH;
    if (max_scenes) *max_scenes = SS_MAX_B;
    if (table_cols) *table_cols = SS_COLS;
    return 0;
}

extern "C" int d3_seg_cluster_table(const int *pick, int n, const int *proposals_idx, long long L, const int *proposals_offset, int P,
                                    const int *semantic_pred, const float *scores, long long N, const int *batch_offsets, int B,
                                    const int *lut, int nlut, int *table, int *counts, int *status, void *stream) {
    if (B < 1 || B > SS_MAX_B || n < 0 || n > SS_MAX_PICKS || P < 0 || L < 0 || L > 0x7fffffffll || N < 0 || N > 0x7fffffffll || nlut < 1)
        return D3_ERR_RANGE;
    if (!proposals_offset || !batch_offsets || !lut || !counts || !status || (n && (!pick || !table || !scores)) || (L && !proposals_idx) ||
        (N && !semantic_pred))
        return D3_ERR_ARG;
    D3_CLEAR();
    ss_table_kernel<<<1, SS_BLOCK, 0, d3_stream(stream)>>>(pick, n, proposals_idx, (int)L, proposals_offset, P, semantic_pred, scores, (int)N,
                                                           batch_offsets, B, lut, nlut, table, counts, status);
    D3_LAUNCH_CHECK();
    return 0;
}

extern "C" int d3_seg_cluster_ids(const int *table, const int *pick, int n, const int *proposals_idx, long long L,
                                  const int *proposals_offset, int P, const int *batch_offsets, int B, long long N, int *cluster_ids,
                                  void *stream) {
    if (B < 1 || B > SS_MAX_B || n < 0 || n > SS_MAX_PICKS || P < 0 || L < 0 || L > 0x7fffffffll || N < 0 || N > 0x7fffffffll)
        return D3_ERR_RANGE;
    if (!proposals_offset || !batch_offsets || (N && !cluster_ids) || (n && (!pick || !table)) || (L && !proposals_idx)) return D3_ERR_ARG;
    hipStream_t st = d3_stream(stream);
    D3_CLEAR();
    if (N) {
        ss_fill_i32<<<(unsigned)((N + SS_BLOCK - 1) / SS_BLOCK), SS_BLOCK, 0, st>>>(cluster_ids, N, -1);
        D3_LAUNCH_CHECK();
    }
    if (n && N && L) {
        ss_ids_kernel<<<(unsigned)n * SS_PARTS, SS_BLOCK, 0, st>>>(table, pick, proposals_idx, (int)L, proposals_offset, P, batch_offsets, B,
                                                                    (int)N, cluster_ids);
        D3_LAUNCH_CHECK();
    }
    return 0;
}

struct SsWork { int *tile_bytes, *tile_off; };
static void ss_layout(D3Carver &c, int tiles, int ntext, SsWork &w) {
    w.tile_bytes = c.take<int>((size_t)tiles * ntext + 1);
    w.tile_off = c.take<int>((size_t)tiles * ntext + 1);
}

extern "C" size_t d3_seg_int_lines_ws_bytes(int tiles, int ntext) {
    if (tiles < 0 || ntext < 1 || ntext > 2) return 0;
    D3Carver c(nullptr, 0);
    SsWork w;
    ss_layout(c, tiles, ntext, w);
    return c.off;
}

extern "C" int d3_seg_int_lines(const int *values0, const int *lut0, int nlut0, int width0, char *text0, long long *lens0,
                                const int *values1, const int *lut1, int nlut1, int width1, char *text1, long long *lens1,
                                long long n_values, const int *offsets, const int *tile_prefix, int B, int tiles, int *status, void *ws,
                                size_t ws_bytes, void *stream) {
    const int ntext = lens1 ? 2 : 1;
    if (B < 1 || B > SS_MAX_B || tiles < 0 || n_values < 0 || n_values > 0x7fffffffll) return D3_ERR_RANGE;
    if ((long long)tiles > n_values / SS_TILE + B) return D3_ERR_RANGE;                   // more tiles than any cut of n_values lines into B segments has
    if (width0 < 2 || width0 > SS_MAX_WIDTH || (ntext == 2 && (width1 < 2 || width1 > SS_MAX_WIDTH))) return D3_ERR_RANGE;
    if (n_values * (long long)(ntext == 2 && width1 > width0 ? width1 : width0) > 0x7fffffffll) return D3_ERR_RANGE;
    if (!lens0 || !offsets || !tile_prefix || !status || (n_values && (!values0 || !text0)) || (lut0 && nlut0 < 1)) return D3_ERR_ARG;
    if (ntext == 2 && ((n_values && (!values1 || !text1)) || (lut1 && nlut1 < 1))) return D3_ERR_ARG;
    D3Carver c(ws, ws_bytes);
    SsWork w;
    ss_layout(c, tiles, ntext, w);
    if (!c.ok()) return D3_ERR_WORKSPACE;
    SsTexts texts;
    texts.t[0] = SsText{values0, lut0, nlut0, width0, text0, lens0};
    texts.t[1] = ntext == 2 ? SsText{values1, lut1, nlut1, width1, text1, lens1} : texts.t[0];
    hipStream_t st = d3_stream(stream);
    const unsigned grid = (unsigned)tiles * (unsigned)ntext;
    D3_CLEAR();
    if (tiles) {
        ss_tile_bytes_kernel<<<grid, SS_BLOCK, 0, st>>>(texts, n_values, offsets, tile_prefix, B, tiles, w.tile_bytes, status);
        D3_LAUNCH_CHECK();
    }
    ss_seg_scan_kernel<<<(unsigned)B * (unsigned)ntext, SS_BLOCK, 0, st>>>(texts, tile_prefix, B, tiles, w.tile_bytes, w.tile_off);
    D3_LAUNCH_CHECK();
    if (tiles) {
        ss_lines_kernel<<<grid, SS_BLOCK, 0, st>>>(texts, n_values, offsets, tile_prefix, B, tiles, w.tile_off, status);
        D3_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int d3_seg_mask_lines(const int *table, const int *pick, int n, const int *proposals_idx, long long L, const int *proposals_offset,
                                 int P, int scene, int lo, int npts, int c_lo, int m, char *text, size_t text_bytes, void *stream) {
    if (n < 1 || n > SS_MAX_PICKS || P < 0 || L < 0 || L > 0x7fffffffll || scene < 0 || lo < 0 || npts < 1 || c_lo < 0 || m < 1)
        return D3_ERR_RANGE;
    if (!table || !pick || !proposals_offset || !text || (L && !proposals_idx) || ((size_t)text & 15)) return D3_ERR_ARG;
    const size_t bytes = 2 * (size_t)m * (size_t)npts, n16 = (bytes + 15) / 16;
    if (text_bytes < n16 * 16) return D3_ERR_WORKSPACE;                                   // the fill runs to the next multiple of 16
    hipStream_t st = d3_stream(stream);
    const size_t blocks = (n16 + SS_BLOCK - 1) / SS_BLOCK;
    D3_CLEAR();
    ss_mask_fill<<<(unsigned)(blocks < (1u << 20) ? blocks : (1u << 20)), SS_BLOCK, 0, st>>>((uint4 *)text, (long long)n16);
    D3_LAUNCH_CHECK();
    if (L) {
        ss_mask_ones_kernel<<<(unsigned)n * SS_PARTS, SS_BLOCK, 0, st>>>(table, pick, proposals_idx, (int)L, proposals_offset, P, scene, lo, npts,
                                                                          c_lo, m, text);
        D3_LAUNCH_CHECK();
    }
    return 0;
}
