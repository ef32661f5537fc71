// metric_log.hip -- running per-key records of the scalars a training / validation step logs (gfx950), driven by
// d3net_amd.metric_log.MetricLog.  The reference hands every logged value to Lightning's `self.log(..., on_epoch=True)`
// (model/pipeline.py:149,182,...), which keeps a running mean per key; here ONE launch per step folds every value logged in
// that step into its slot's record and nothing is read back.
//
// One thread per slot, plain C++: a 24-byte table row in (address of the 0-d device value, dtype code, float64 weight), a
// 40-byte record out.  No atomics and no reduction across threads: a slot has exactly one writer and its sum receives one
// double multiplication and one double addition per step, in step order (the build runs with -ffp-contract=off, so the two
// are not fused) -- the record equals a sequential host sum bit for bit.  Slots beyond 256 go to further workgroups.
// A null address leaves the slot's record as it is.  Traffic: 24 + 40 + 40 bytes and one scalar load per logged key.
#include "common.h"

#define METRIC_CAP 1024   // = d3_metric_capacity(): slots per launch and per reset range

template <typename T>
__device__ __forceinline__ double metric_load(const void *p) {
    return (double)*(const T *)p;
}

__global__ __launch_bounds__(256) void metric_accumulate_kernel(const d3_metric_row *__restrict__ table, int nslots,
                                                               d3_metric_rec *__restrict__ records) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nslots) return;
    const d3_metric_row row = table[i];
    if (!row.value) return;                   // not logged this step: the record stays bit-unchanged
    double v;
    switch (row.dtype) {
    case D3_METRIC_F32: v = metric_load<float>(row.value); break;
    case D3_METRIC_F64: v = metric_load<double>(row.value); break;
    case D3_METRIC_I32: v = metric_load<int>(row.value); break;
    case D3_METRIC_I64: v = metric_load<long long>(row.value); break;
    default: return;                          // an unknown code is treated as "not logged" (MetricLog never writes one)
    }
    d3_metric_rec r = records[i];
    const double wv = row.weight * v;
    r.sum = r.sum + wv;
    r.wsum = r.wsum + row.weight;
    r.last = v;
    r.count += 1;
    r.nonfinite += isfinite(v) ? 0 : 1;
    records[i] = r;
}

extern "C" int d3_metric_capacity(void) { return METRIC_CAP; }

extern "C" int d3_metric_accumulate(const void *table, int nslots, void *records, void *stream) {
    D3_CLEAR();
    if (nslots < 0 || nslots > METRIC_CAP) return D3_ERR_RANGE;   // never truncated
    if (nslots == 0) return 0;
    if (!table || !records) return D3_ERR_ARG;
    metric_accumulate_kernel<<<(nslots + 255) / 256, 256, 0, d3_stream(stream)>>>((const d3_metric_row *)table, nslots,
                                                                               (d3_metric_rec *)records);
    D3_LAUNCH_CHECK();
    return 0;
}

extern "C" int d3_metric_reset(void *records, int offset, int count, void *stream) {
    D3_CLEAR();
    if (offset < 0 || count < 0 || count > METRIC_CAP) return D3_ERR_RANGE;
    if (count == 0) return 0;
    if (!records) return D3_ERR_ARG;
    D3_CHECK(hipMemsetAsync((d3_metric_rec *)records + offset, 0, (size_t)count * sizeof(d3_metric_rec), d3_stream(stream)));
    return 0;
}
