// tuning.hip -- the ONE place where libd3hip.so reads its environment.
//
// Every switch of the library lives in this table: the arms a test flips and compares against the default.  A
// measured-and-decided choice is not a switch: its winner is the code, its threshold a named constant at its use.  The environment is parsed
// exactly once, at the first d3_tune() of the process; launch paths read an array slot, never getenv().  Tests and the
// A/B tools flip a switch at run time through d3_tuning_set() (include/d3hip.h) instead of mutating the environment.
#include <atomic>
#include <mutex>
#include <stdlib.h>
#include <string.h>
#include "common.h"

namespace {
struct Entry { const char *name; int dflt; };
// order == enum D3Tune (common.h)
const Entry kTable[D3T_COUNT] = {
    {"D3_ATTN_SCALAR", 0},          // 1: round-1 scalar attention kernels (cross-check)
    {"D3_BFS_NO_STAR", 0},          // 1: force the BFS level loop for every cluster (tests)
    {"D3_WG3", 1},                  // 0: second-generation weight-gradient kernel
    {"D3_GRAD_BF16", 1},            // 0: every gradient buffer in fp32
    {"D3_BQ_GRID", 1},              // 0: padded ball query by the ordered chunk scan instead of the cell grid
    {"D3_BN_FUSED_ROWS", 16384},    // BatchNorm over at most this many rows: finalize + apply (forward) / final + apply (backward) in one launch (0: never)
    {"D3_KMAP16", 1},               // 0: the executor's K = 27 convolutions read the dense int32 kernel maps only
    {"D3_HG_SPLITK", 256},          // largest number of 16 x 16 output tiles of a deep (K >= 8192) heads GEMM whose reduction is cut over 4 workgroups; 0: never
    {"D3_BN_PART2", 1},             // 0: BatchNorm launches reduce the producer's whole per-workgroup partial table (rounds 1-4) instead of the 16-row fp64 second-level table
    {"D3_CL_SPEC", 1},              // 0: d3_bfs_cluster_run waits for the cluster counts before it enqueues the fill; 1: the fill is enqueued behind the count kernels with its sizes read on the device, the host waits for the counts while the fill already runs
    {"D3_TD_FUSE_GATES", 1},        // 0: the captioner's backward step keeps its two GRU gate kernels (rounds 2-4: 6 dependent launches per step) instead of running them as epilogues of the GEMMs that complete their input (4 launches)
    {"D3_C3", 1},                   // 0: the K = 27 convolutions of the big levels never run spconv_fwd3_kernel (lane table, round 6) -- A/B against spconv_fwd2_kernel
};
std::atomic<int> g_val[D3T_COUNT];
std::once_flag g_once;

void parse_once() {
    for (int i = 0; i < D3T_COUNT; i++) {
        const char *e = getenv(kTable[i].name);
        g_val[i].store((e && e[0]) ? atoi(e) : kTable[i].dflt, std::memory_order_relaxed);
    }
}
int find(const char *name) {
    for (int i = 0; name && i < D3T_COUNT; i++)
        if (!strcmp(name, kTable[i].name)) return i;
    return -1;
}
}  // namespace

int d3_tune(int key) {
    std::call_once(g_once, parse_once);
    return g_val[key].load(std::memory_order_relaxed);
}

extern "C" int d3_tuning_set(const char *name, int value) {
    std::call_once(g_once, parse_once);
    const int i = find(name);
    if (i < 0) return D3_ERR_ARG;
    g_val[i].store(value, std::memory_order_relaxed);
    return 0;
}

extern "C" int d3_tuning_get(const char *name, int *value) {
    std::call_once(g_once, parse_once);
    const int i = find(name);
    if (i < 0 || !value) return D3_ERR_ARG;
    *value = g_val[i].load(std::memory_order_relaxed);
    return 0;
}

extern "C" int d3_tuning_count(void) { return D3T_COUNT; }

extern "C" const char *d3_tuning_name(int i) { return (i >= 0 && i < D3T_COUNT) ? kTable[i].name : nullptr; }
