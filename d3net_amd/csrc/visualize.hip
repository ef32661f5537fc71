// visualize.hip -- box wireframes as PLY text on the device (gfx950): per box the 1320 vertex lines of the twelve-cylinder mesh that
// the reference's visualisers write, vertices and decimal text both.
//
// Replaces the Python vertex loop of scripts/visualize_grounding.py:45-168 (write_bbox: create_cylinder_mesh per edge, the 4 x 4
// transform per vertex) and the per-vertex "{:f} {:f} {:f} {:d} {:d} {:d}\n".format of write_ply (:39-40); scripts/
// visualize_captioning.py carries the same two functions.  The header, the constant face block and the files are the host's
// (d3net_amd/visualize.py), which does no arithmetic and no formatting of coordinates.
//
// Geometry (restated from the reference, not copied).  write_bbox takes min / max over the 8 corners, so all 12 edges are axis
// aligned: edges 0-3 walk the bottom face +x, +y, -x, -y from the min corner, 4-7 the top face, 8-11 go +z.  Per edge p0 -> p1:
//   d = float32(p1 - p0);  h = sqrt in double of the FLOAT32 square of d (compute_length_vec3 on a float32 vector);
//   local vertex (stack i of 0..10, slice i2 of 0..9) = (0.03 cos t, 0.03 sin t, (h * i) / 10), t = i2 * 2 pi / 10;
//   the reference's rotation() from +z onto the edge direction is, for an axis-aligned edge, a signed permutation with exact 0 / 1
//   entries: +x (lz, ly, -lx), -x (-lz, ly, lx), +y (lx, lz, -ly), -y (lx, -lz, ly), +z the identity;
//   vertex = p0 + that, ONE rounding per coordinate (the other products of the 4 x 4 row are exact zeros).  p0 enters as 0 + p0 and
//   the sum passes `+ [0, 0, 0]`, so a zero prints without a sign: both additions of 0.0 below are the reference's.
// The 20 values 0.03 cos t, 0.03 sin t come from the host's libm (VzRing), so the device does no trigonometry.
//
// Text: "{:f}" of a double is its exact binary value rounded half-to-even at six decimals.  vz_f6 splits |v| = m 2^e into the
// integer part and the fraction's mantissa f (< 2^53) over 2^s, forms f * 10^6 (< 2^73) in 128-bit integers, shifts by s, and rounds
// on the shifted-out bits; s >= 128 cannot reach half.  A carry into 10^6 goes to the integer part.  The sign is the sign bit, so
// -0.0 and every negative that rounds to zero print "-0.000000", as Python prints them.
//
//   vz_text_kernel    one workgroup of 256 per box.  Every thread reads the 8 corners (the same 24 doubles: one broadcast load each)
//                     and checks them; thread t formats the lines t, t + 256, ... into fixed 56-byte slots of LDS (a line is at
//                     most 53 bytes under the limits) and leaves their lengths; a block scan (6 lengths per thread, wave shuffles,
//                     four wave totals) gives the line offsets; then the text leaves as dwords in output order, the dword's first
//                     byte located by a binary search over the offsets: consecutive lanes, consecutive addresses.  No scratch.
//   vz_verts_kernel   one thread per vertex, the same vz_vertex.
//   vz_f6_kernel      one thread per value, 24-byte slots.
#include "common.h"
#include "dispatch.h"

#define VZ_THREADS 256
#define VZ_WAVES (VZ_THREADS / 64)
#define VZ_EDGE_VERTS 110                       // 11 stacks x 10 slices
#define VZ_VERTS (12 * VZ_EDGE_VERTS)           // 1320
#define VZ_LINE 56                              // LDS slot of a line; >= 14 + 1 + 14 + 1 + 14 + 9
#define VZ_BOX_BYTES (VZ_VERTS * VZ_LINE)       // 73920: the stride of a box's text in the output
#define VZ_PER_THREAD ((VZ_VERTS + VZ_THREADS - 1) / VZ_THREADS)     // 6
#define VZ_F6_SLOT 24                           // '-' + 16 digits + '.' + 6
#define VZ_LIMIT 1e5                            // |corner coordinate| below this
#define VZ_F6_LIMIT 1e15                        // |value| of d3_format_f6 below this

struct VzRing { double c[10], s[10]; };         // 0.03 cos(i2 2 pi / 10), 0.03 sin(...)
struct VzBox { double nx, ny, nz, xx, xy, xz; };

// "{:f}".format(v) -> dst, returns the length; -1 when |v| >= 1e15 (finite)
__host__ __device__ __forceinline__ int vz_f6(double v, char *dst) {
    unsigned long long bits;
    __builtin_memcpy(&bits, &v, 8);
    const bool neg = (bits >> 63) != 0;
    const int ex = (int)((bits >> 52) & 0x7ff);
    const unsigned long long man = bits & ((1ull << 52) - 1ull);
    int n = 0;
    if (ex == 0x7ff) {
        if (man) { dst[0] = 'n'; dst[1] = 'a'; dst[2] = 'n'; return 3; }
        if (neg) dst[n++] = '-';
        dst[n] = 'i'; dst[n + 1] = 'n'; dst[n + 2] = 'f';
        return n + 3;
    }
    if (!(fabs(v) < VZ_F6_LIMIT)) return -1;
    const unsigned long long m = ex ? (man | (1ull << 52)) : man;      // |v| = m 2^e2
    const int e2 = (ex ? ex : 1) - 1075;                               // < 0 below 2^53
    unsigned long long I;
    unsigned int q = 0;
    if (e2 >= 0) {
        I = m << e2;                                                   // (unreachable under the limit; an integer)
    } else {
        const int s = -e2;                                             // 1 .. 1074
        unsigned long long f;
        if (s >= 64) { I = 0; f = m; } else { I = m >> s; f = m & ((1ull << s) - 1ull); }
        if (s < 128) {
            const unsigned __int128 P = (unsigned __int128)f * 1000000u;
            const unsigned __int128 rem = P & ((((unsigned __int128)1) << s) - 1u), half = ((unsigned __int128)1) << (s - 1);
            q = (unsigned int)(unsigned long long)(P >> s);
            if (rem > half || (rem == half && (q & 1u))) q++;
            if (q == 1000000u) { q = 0; I++; }
        }
    }
    if (neg) dst[n++] = '-';
    int nd = 1;
    for (unsigned long long t = I; t >= 10ull; t /= 10ull) nd++;
    for (int k = nd - 1; k >= 0; k--) { dst[n + k] = (char)('0' + (int)(I % 10ull)); I /= 10ull; }
    n += nd;
    dst[n++] = '.';
#pragma unroll
    for (int k = 5; k >= 0; k--) { dst[n + k] = (char)('0' + (int)(q % 10u)); q /= 10u; }
    return n + 6;
}

// min / max corner of box b and its status bits: 1 a coordinate is not finite or |c| >= 1e5, 2 an extent whose float32 square is
// not a normal positive number (zero extent; the reference divides by its root)
__host__ __device__ __forceinline__ int vz_box(const double *__restrict__ corners, long long b, VzBox &o) {
    const double *c = corners + b * 24;
    int bad = 0;
    double lo[3], hi[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        lo[a] = hi[a] = c[a];
#pragma unroll
        for (int v = 0; v < 8; v++) {
            const double x = c[v * 3 + a];
            if (!(fabs(x) < VZ_LIMIT)) bad |= 1;            // (a NaN fails)
            lo[a] = x < lo[a] ? x : lo[a];
            hi[a] = x > hi[a] ? x : hi[a];
        }
        const float d = (float)(hi[a] - lo[a]);
        const float sq = d * d;
        if (!(sq >= 1.17549435e-38f)) bad |= 2;
    }
    o.nx = lo[0]; o.ny = lo[1]; o.nz = lo[2]; o.xx = hi[0]; o.xy = hi[1]; o.xz = hi[2];
    return bad & 1 ? 1 : bad;
}

// vertex L (0 .. 1319) of the box, in the reference's order: edge, stack, slice
__host__ __device__ __forceinline__ void vz_vertex(const VzBox &b, const VzRing &ring, int L, double &x, double &y, double &z) {
    const int k = L / VZ_EDGE_VERTS, r = L - k * VZ_EDGE_VERTS, i = r / 10, i2 = r - i * 10;
    const int dir = k >= 8 ? 4 : (k & 3);                   // 0 +x, 1 +y, 2 -x, 3 -y, 4 +z
    const int c0 = k >= 8 ? k - 8 : k, j = c0 & 3;          // the edge starts at corner c0 of get_bbox_verts
    const double px = ((j == 1 || j == 2) ? b.xx : b.nx) + 0.0, py = (j >= 2 ? b.xy : b.ny) + 0.0, pz = (c0 >= 4 ? b.xz : b.nz) + 0.0;
    const double ext = dir == 4 ? b.xz - b.nz : ((dir & 1) ? b.xy - b.ny : b.xx - b.nx);
    const float d = (float)ext;                             // |p1 - p0| along the edge; the two other components are exact zeros
    const float sq = d * d;
    const double h = sqrt((double)sq);
    const double lx = ring.c[i2], ly = ring.s[i2], lz = (h * (double)i) / 10.0;
    double ox, oy, oz;
    switch (dir) {
        case 0: ox = lz; oy = ly; oz = -lx; break;
        case 1: ox = lx; oy = lz; oz = -ly; break;
        case 2: ox = -lz; oy = ly; oz = lx; break;
        case 3: ox = lx; oy = -lz; oz = ly; break;
        default: ox = lx; oy = ly; oz = lz; break;
    }
    x = (px + ox) + 0.0; y = (py + oy) + 0.0; z = (pz + oz) + 0.0;
}

__device__ __forceinline__ void vz_flag(int *__restrict__ status, int bits, long long b) {
    atomicOr(status, bits);
    atomicMin(status + 1, (int)b);
}

__global__ __launch_bounds__(VZ_THREADS) void vz_text_kernel(const double *__restrict__ corners, const int *__restrict__ modes,
                                                             VzRing ring, char *__restrict__ text, int *__restrict__ nbytes,
                                                             int *__restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) char vz_lds[];
    int *off = (int *)vz_lds;                               // [VZ_VERTS + 1] line offsets, lengths before the scan
    int *wtot = off + VZ_VERTS + 4;                         // [VZ_WAVES]; all LDS is dynamic, so its base stays 16-byte aligned
    char *lines = vz_lds + (VZ_VERTS + 8) * sizeof(int);    // [VZ_VERTS][VZ_LINE]
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
    VzBox box;
    int bad = vz_box(corners, b, box);                      // workgroup-uniform
    const int mode = modes[b];
    if (mode != 0 && mode != 1) bad |= 4;
    if (bad) {
        if (t == 0) { vz_flag(status, bad, b); nbytes[b] = 0; }
        return;
    }
    for (int L = t; L < VZ_VERTS; L += VZ_THREADS) {
        double x, y, z;
        vz_vertex(box, ring, L, x, y, z);
        char *dst = lines + L * VZ_LINE;
        int n = vz_f6(x, dst);
        dst[n++] = ' ';
        n += vz_f6(y, dst + n);
        dst[n++] = ' ';
        n += vz_f6(z, dst + n);
        dst[n] = ' '; dst[n + 1] = '0'; dst[n + 2] = ' ';
        if (mode == 0) { dst[n + 3] = '2'; dst[n + 4] = '5'; dst[n + 5] = '5'; dst[n + 6] = ' '; dst[n + 7] = '0'; }
        else { dst[n + 3] = '0'; dst[n + 4] = ' '; dst[n + 5] = '2'; dst[n + 6] = '5'; dst[n + 7] = '5'; }
        dst[n + 8] = '\n';
        off[L + 1] = n + 9;
    }
    __syncthreads();
    // exclusive scan of the 1320 lengths: thread t owns lines [6 t, 6 t + 6)
    int len[VZ_PER_THREAD], mine = 0;
#pragma unroll
    for (int k = 0; k < VZ_PER_THREAD; k++) {
        const int L = t * VZ_PER_THREAD + k;
        len[k] = L < VZ_VERTS ? off[L + 1] : 0;
        mine += len[k];
    }
    int incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(incl, d);
        if (lane >= d) incl += up;
    }
    if (lane == 63) wtot[w] = incl;
    __syncthreads();                                        // (every length has been read into registers by now)
    int base = incl - mine, total = 0;
#pragma unroll
    for (int i = 0; i < VZ_WAVES; i++) { if (i < w) base += wtot[i]; total += wtot[i]; }
    if (t == 0) off[0] = 0;
#pragma unroll
    for (int k = 0; k < VZ_PER_THREAD; k++) {
        const int L = t * VZ_PER_THREAD + k;
        base += len[k];
        if (L < VZ_VERTS) off[L + 1] = base;
    }
    __syncthreads();
    unsigned int *out = (unsigned int *)(text + (size_t)b * VZ_BOX_BYTES);
    const int ndw = (total + 3) >> 2;                       // total <= 1320 * 53 < VZ_BOX_BYTES
    for (int j = t; j < ndw; j += VZ_THREADS) {
        const int p = j * 4;
        int lo = 0, hi = VZ_VERTS - 1;                      // the last line L with off[L] <= p
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (off[mid] <= p) lo = mid; else hi = mid - 1;
        }
        int L = lo, at = p - off[L], end = off[L + 1] - off[L];
        unsigned int word = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (p + k < total) {
                if (at >= end) { L++; at = 0; end = off[L + 1] - off[L]; }      // (a line is never empty)
                word |= (unsigned int)(unsigned char)lines[L * VZ_LINE + at] << (8 * k);
                at++;
            }
        }
        out[j] = word;
    }
    if (t == 0) nbytes[b] = total;
}

__global__ __launch_bounds__(VZ_THREADS) void vz_verts_kernel(const double *__restrict__ corners, VzRing ring, long long M,
                                                              double *__restrict__ verts, int *__restrict__ status) {
    const long long g = (long long)blockIdx.x * VZ_THREADS + threadIdx.x;
    if (g >= M * VZ_VERTS) return;
    const long long b = g / VZ_VERTS;
    const int L = (int)(g - b * VZ_VERTS);
    VzBox box;
    const int bad = vz_box(corners, b, box);
    if (bad) {
        if (L == 0) vz_flag(status, bad, b);
        return;
    }
    double x, y, z;
    vz_vertex(box, ring, L, x, y, z);
    verts[g * 3] = x; verts[g * 3 + 1] = y; verts[g * 3 + 2] = z;
}

__global__ __launch_bounds__(VZ_THREADS) void vz_f6_kernel(const double *__restrict__ values, long long n, char *__restrict__ text,
                                                           int *__restrict__ lens, int *__restrict__ status) {
    const long long g = (long long)blockIdx.x * VZ_THREADS + threadIdx.x;
    if (g >= n) return;
    const int len = vz_f6(values[g], text + g * VZ_F6_SLOT);
    lens[g] = len;
    if (len < 0) atomicOr(status, 1);
}

// ------------------------------------------------------------------------------------------------- host
static VzRing vz_ring(const double *ring20) {
    VzRing r;
    for (int i = 0; i < 10; i++) { r.c[i] = ring20[i]; r.s[i] = ring20[10 + i]; }
    return r;
}

extern "C" int d3_box_wire_limits(int *verts_per_box, int *text_stride, int *f6_stride) {
    if (verts_per_box) *verts_per_box = VZ_VERTS;
    if (text_stride) *text_stride = VZ_BOX_BYTES;
    if (f6_stride) *f6_stride = VZ_F6_SLOT;
    return 0;
}

extern "C" int d3_box_wire_verts(const double *corners, int M, const double *ring20, double *verts, int *status, void *stream) {
    D3_CLEAR();
    if (M < 1 || M > (1 << 20)) return D3_ERR_RANGE;
    if (!corners || !ring20 || !verts || !status) return D3_ERR_ARG;
    const long long n = (long long)M * VZ_VERTS;
    vz_verts_kernel<<<(unsigned int)((n + VZ_THREADS - 1) / VZ_THREADS), VZ_THREADS, 0, d3_stream(stream)>>>(corners, vz_ring(ring20), M, verts,
                                                                                                           status);
    D3_LAUNCH_CHECK();
    return 0;
}

extern "C" int d3_box_wire_text(const double *corners, const int *modes, int M, const double *ring20, char *text, int *nbytes,
                                int *status, void *stream) {
    D3_CLEAR();
    if (M < 1 || M > (1 << 20)) return D3_ERR_RANGE;
    if (!corners || !modes || !ring20 || !text || !nbytes || !status) return D3_ERR_ARG;
    const int lds = (VZ_VERTS + 8) * (int)sizeof(int) + VZ_BOX_BYTES;
    if (const int rc = d3_allow_lds<vz_text_kernel>(lds)) return rc;
    vz_text_kernel<<<M, VZ_THREADS, lds, d3_stream(stream)>>>(corners, modes, vz_ring(ring20), text, nbytes, status);
    D3_LAUNCH_CHECK();
    return 0;
}

extern "C" int d3_format_f6(const double *values, long long n, char *text, int *lens, int *status, void *stream) {
    D3_CLEAR();
    if (n < 1 || n > (1ll << 30)) return D3_ERR_RANGE;
    if (!values || !text || !lens || !status) return D3_ERR_ARG;
    vz_f6_kernel<<<(unsigned int)((n + VZ_THREADS - 1) / VZ_THREADS), VZ_THREADS, 0, d3_stream(stream)>>>(values, n, text, lens, status);
    D3_LAUNCH_CHECK();
    return 0;
}
