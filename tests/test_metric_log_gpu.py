"""csrc/metric_log.hip and d3net_amd.metric_log.MetricLog on the device.  d3_metric_accumulate through the C ABI against a sequential
float64 numpy restatement, compared with == (each sum receives one double multiplication and one double addition per step, in step
order: no tolerance is needed); absent keys, inf / NaN, freshly allocated tensors every step (the address refresh), the capacity
error, and no synchronisation in update() / snapshot()."""
import gc

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = (torch.float32, torch.float64, torch.int32, torch.int64)      # D3_METRIC_F32, F64, I32, I64
NP = {torch.float32: np.float32, torch.float64: np.float64, torch.int32: np.int32, torch.int64: np.int64}
WEIGHTS = (0.5, 1.25, 3.0, 0.1, 2.0)                                    # per step, none of them 1
STEPS = 5


def _values(n, step, seed=0):
    """host values of step `step` for n slots; slot i has dtype DTYPES[i % 4] in every step"""
    rng = np.random.default_rng(1000 * seed + step)
    out = []
    for i in range(n):
        dt = DTYPES[i % 4]
        if dt.is_floating_point:
            out.append(NP[dt](rng.standard_normal() * 10.0 ** rng.integers(-3, 4)))
        elif dt == torch.int64:
            out.append(np.int64(rng.integers(-2 ** 40, 2 ** 40)) if i % 8 == 3 else np.int64(2 ** 53 + 1 + 2 * i))   # (not a float64)
        else:
            out.append(np.int32(rng.integers(-2 ** 31, 2 ** 31)))
    return out


def _restate(rec, values, weight, present=None):
    """the record's definition, sequentially in float64; rec: dict of arrays (sum, wsum, last, count, nonfinite)"""
    for i, v in enumerate(values):
        if present is not None and not present[i]:
            continue
        x, w = np.float64(v), np.float64(weight)
        with np.errstate(all="ignore"):
            wv = w * x
            rec["sum"][i] = rec["sum"][i] + wv
        rec["wsum"][i] = rec["wsum"][i] + w
        rec["last"][i] = x
        rec["count"][i] += 1
        rec["nonfinite"][i] += 0 if np.isfinite(x) else 1


def _empty(n):
    return {"sum": np.zeros(n), "wsum": np.zeros(n), "last": np.zeros(n), "count": np.zeros(n, np.int64), "nonfinite": np.zeros(n, np.int64)}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _assert_records(got, want, where):
    """got: the (n, 5) float64 block read back; bit equality (NaN included)"""
    assert np.array_equal(_bits(got[:, 0]), _bits(want["sum"])), (where, "sum")
    assert np.array_equal(_bits(got[:, 1]), _bits(want["wsum"])), (where, "wsum")
    assert np.array_equal(_bits(got[:, 2]), _bits(want["last"])), (where, "last")
    assert np.array_equal(np.ascontiguousarray(got[:, 3]).view(np.int64), want["count"]), (where, "count")
    assert np.array_equal(np.ascontiguousarray(got[:, 4]).view(np.int64), want["nonfinite"]), (where, "nonfinite")


def _launch(L, table, n, records, offset=0):
    from d3net_amd._lib import check
    check(L.d3_metric_accumulate(table.data_ptr(), n, records.data_ptr() + 40 * offset, torch.cuda.current_stream().cuda_stream),
          "metric_accumulate")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257])
def test_accumulate_equals_sequential_float64(dev, n):
    """key counts at the wave edge, the last key of the first workgroup and the first of the second; dtypes change between
    slots, weights between steps"""
    from d3net_amd import _lib
    L = _lib.lib()
    guard = 3                                                     # records behind the last slot stay untouched
    records = torch.zeros((n + guard, 5), dtype=torch.float64, device=dev)
    records[n:] = 7.0
    want = _empty(n)
    for step in range(STEPS):
        vals = _values(n, step, seed=n)
        store = {dt: torch.tensor(np.array([v for i, v in enumerate(vals) if DTYPES[i % 4] == dt], dtype=NP[dt]), device=dev)
                 for dt in DTYPES}
        seen = {dt: 0 for dt in DTYPES}
        rows = np.zeros((n, 3), np.int64)
        for i in range(n):
            dt = DTYPES[i % 4]
            rows[i, 0] = store[dt].data_ptr() + store[dt].element_size() * seen[dt]
            rows[i, 1] = i % 4
            seen[dt] += 1
        rows[:, 2] = np.array([WEIGHTS[step]] * n, np.float64).view(np.int64)
        table = torch.from_numpy(rows).to(dev)
        _launch(L, table, n, records)
        torch.cuda.synchronize()
        _restate(want, vals, WEIGHTS[step])
        _assert_records(records[:n].cpu().numpy(), want, (n, step))
    assert bool((records[n:] == 7.0).all())
    # d3_metric_reset over a range: the slots in front of it and behind it keep their records
    if n >= 3:
        from d3net_amd._lib import check
        check(L.d3_metric_reset(records.data_ptr(), 1, n - 2, torch.cuda.current_stream().cuda_stream), "metric_reset")
        got = records.cpu().numpy()
        assert not got[1:n - 1].view(np.int64).any() and bool((records[n:] == 7.0).all())
        for k in (0, n - 1):
            assert got[k, 0] == want["sum"][k] and got[k, 1] == want["wsum"][k]


def _fresh(vals, dev):
    """every logged value a 0-d tensor of its own"""
    return [torch.tensor(v, dtype={np.float32: torch.float32, np.float64: torch.float64, np.int32: torch.int32,
                                   np.int64: torch.int64}[type(v)], device=dev) for v in vals]


def test_absent_key_nonfinite_and_fresh_allocations(dev):
    """through MetricLog.update: every logged tensor freshly allocated each step and the previous ones freed (the address column is
    refreshed every step); key 5 absent in steps 2 and 4; inf and NaN in key 8; means, counts and the other keys' records"""
    from d3net_amd.metric_log import MetricLog
    n = 70
    log = MetricLog(device=dev)
    names = ["k%03d" % i for i in range(n)]
    want = _empty(n)
    inject = {1: np.float64("inf"), 2: np.float64("nan"), 3: np.float64("-inf")}
    for step in range(STEPS):
        vals = _values(n, step, seed=77)
        if step in inject:
            vals[8] = np.float32(inject[step])                   # (slot 8 is a float32 slot)
        present = [not (i == 5 and step in (2, 4)) for i in range(n)]
        tensors = _fresh(vals, dev)
        logged = {k: t for k, t, p in zip(names, tensors, present) if p}
        del tensors
        log.update(logged, weight=WEIGHTS[step])
        del logged
        gc.collect()                                             # only the log still holds this step's tensors
        junk = [torch.full((), 12345.0, device=dev) for _ in range(n)]      # takes the blocks a premature free would hand out
        del junk
        _restate(want, vals, WEIGHTS[step], present)
    torch.cuda.synchronize()
    got = log._records[:n].cpu().numpy()
    _assert_records(got, want, "MetricLog")
    counts, means, bad = log.counts(), log.compute(), log.nonfinite()
    assert counts["k005"] == 3 and all(c == STEPS for k, c in counts.items() if k != "k005")
    with np.errstate(all="ignore"):
        for i, k in enumerate(names):
            m = want["sum"][i] / want["wsum"][i]
            assert means[k] == m or (np.isnan(means[k]) and np.isnan(m)), k
    assert not np.isfinite(means["k008"]) and bad == {"k008": 3}
    assert all(np.isfinite(v) for k, v in means.items() if k != "k008")
    assert log.last()["k005"] == float(np.float64(_values(n, 3, seed=77)[5]))           # its last value is step 3's
    log.reset()
    torch.cuda.synchronize()
    assert not log._records.cpu().numpy().view(np.int64).any() and log.compute() == {}


def test_shared_record_buffer_and_mixed_arms(dev):
    """two logs in one buffer (the trainer's training and validation tables): each writes and resets its own range only; a key that
    arrives as a Python number in one step and as a device scalar in the next is summed over both arms"""
    from d3net_amd.metric_log import CAPACITY, MetricLog
    buf = MetricLog.allocate(dev, 2 * CAPACITY)
    a, b = MetricLog(records=buf, offset=0), MetricLog(records=buf, offset=CAPACITY)
    a.update({"x": torch.tensor(1.5, device=dev), "y": 2})
    b.update({"x": torch.tensor(4.0, device=dev)})
    a.update({"x": 0.25, "y": torch.tensor(3, device=dev)})
    assert a.compute() == {"x": 0.875, "y": 2.5} and b.compute() == {"x": 4.0} and a.last() == {"x": 0.25, "y": 3.0}
    a.reset()
    assert a.compute() == {} and b.compute() == {"x": 4.0}


def test_capacity_is_an_error_not_a_truncation(dev):
    from d3net_amd import _lib
    from d3net_amd.metric_log import CAPACITY, MetricLog
    L = _lib.lib()
    cap = L.d3_metric_capacity()
    assert cap >= 256 and cap == CAPACITY
    records = torch.zeros((cap + 1, 5), dtype=torch.float64, device=dev)
    table = torch.zeros((cap + 1, 3), dtype=torch.int64, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    assert L.d3_metric_accumulate(table.data_ptr(), cap + 1, records.data_ptr(), st) == -2          # D3_ERR_RANGE
    assert L.d3_metric_accumulate(table.data_ptr(), cap, records.data_ptr(), st) == 0               # (all addresses null: no-op)
    assert L.d3_metric_reset(records.data_ptr(), 0, cap + 1, st) == -2 and L.d3_metric_reset(records.data_ptr(), -1, 1, st) == -2
    torch.cuda.synchronize()
    assert not records.cpu().numpy().view(np.int64).any()
    log = MetricLog(device=dev, capacity=4)
    with pytest.raises(_lib.D3Error, match="D3_ERR_RANGE"):
        log.update({"k%d" % i: torch.tensor(float(i), device=dev) for i in range(5)})


def test_update_and_snapshot_do_not_synchronise(dev):
    """the way tests/test_caption_evaluator_gpu.py checks add_batch: under sync-debug "error" a host synchronisation raises"""
    from d3net_amd.metric_log import MetricLog
    log = MetricLog(device=dev)
    steps = [{"a": torch.tensor(float(s), device=dev), "b": torch.tensor(s, device=dev), "c": 0.5 * s} for s in range(1, 9)]
    torch.cuda.synchronize()
    got = []
    torch.cuda.set_sync_debug_mode("error")
    try:
        for s, logged in enumerate(steps):
            log.update(logged, weight=2.0)
            if s % 2:
                got.append(log.snapshot(tag=s))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert got[0] is None                                  # the first call has nothing earlier to return
    torch.cuda.synchronize()
    last = log.snapshot()
    assert last is not None and log.snapshot_tag in (1, 3, 5, 7)
    k = log.snapshot_tag + 1                              # that snapshot saw steps 1 .. k
    assert last == {"a": (k + 1) / 2, "b": (k + 1) / 2, "c": 0.25 * (k + 1)}
    assert log.compute() == {"a": 4.5, "b": 4.5, "c": 2.25}
