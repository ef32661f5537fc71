"""d3net_amd.devstate on host tensors: the batch check's order, the record store, the read-back and the coercions.  No library
is loaded: `_lib.lib` is patched to fail."""
import numpy as np
import pytest
import torch

from d3net_amd import _lib, devstate as ds


@pytest.fixture(autouse=True)
def no_library(monkeypatch):
    def no_launch():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "lib", no_launch)


TABLE = {"boxes": (ds.FLOATS, None), "scores": (ds.FLOATS, (("B", "K"),)), "ids": (ds.INTS, (("B",), ("B", 1))), "names": None}


def _geometry(d):
    if d["boxes"].dim() != 4 or not 1 <= d["boxes"].shape[1] <= 4:
        raise ValueError("t: boxes (B,K,8,3) with 1 <= K <= 4 expected")
    return dict(B=d["boxes"].shape[0], K=d["boxes"].shape[1])


def _good():
    return dict(boxes=torch.zeros(2, 3, 8, 3), scores=torch.zeros(2, 3), ids=torch.zeros(2, dtype=torch.int64), names=["a", "b"])


def _refused(match, device=None, state=None, drop=(), **change):
    d = dict(_good(), **change)
    for k in drop:
        del d[k]
    with pytest.raises(ValueError, match=match):
        ds.check_batch("t", d, TABLE, _geometry, device, state)


def test_check_order_the_earlier_fault_is_reported():
    # each batch is wrong in two ways, one step apart in the documented order
    _refused("missing \\['ids', 'names'\\]", drop=("ids", "names"), scores=[0.0])            # missing before not-a-tensor
    _refused("scores must be a tensor", scores=[0.0], boxes=torch.zeros(2, 5, 8, 3))         # not-a-tensor before geometry
    _refused("1 <= K <= 4", boxes=torch.zeros(2, 5, 8, 3), scores=torch.zeros(2, 3))          # geometry before shapes
    _refused("scores has shape \\(2, 2\\), expected \\(2, 3\\)", scores=torch.zeros(2, 2), ids=torch.zeros(2))     # shapes before dtypes
    _refused("ids has shape \\(3,\\), expected \\(2,\\) or \\(2, 1\\)", ids=torch.zeros(3, dtype=torch.int64))
    _refused("ids has dtype torch.float32", ids=torch.zeros(2))                              # dtypes before device (all of it is in host memory)
    _refused("boxes is in host memory .*on the GPU.*no CPU fallback")                        # well-formed: refused for where it lives


def test_device_rule(monkeypatch):
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))            # host tensors posing as device ones
    good = _good()
    assert ds.check_batch("t", good, TABLE, _geometry) == dict(B=2, K=3)                   # no constructor device: the first key's
    assert ds.check_batch("t", good, TABLE, _geometry, torch.device("cuda")) == dict(B=2, K=3)      # no index: any one GPU
    _refused("boxes is on cpu; .*one GPU \\(cuda:1\\)", device=torch.device("cuda", 1))
    _refused("scores is on meta", scores=torch.zeros(2, 3, device="meta"))                 # not on the first key's device
    _refused("boxes is on cpu; .*\\(meta\\)", state=torch.zeros(1, device="meta"))         # not on the state's device


def test_record_store_grows_by_doubling():
    st = ds.RecordStore("cpu", box=((8, 3), torch.float32), ids=((2,), torch.int64), n=((), torch.int32))
    assert {k: tuple(t.shape) for k, t in st.t.items()} == {"box": (1024, 8, 3), "ids": (1024, 2), "n": (1024,)} and st.rows == 0
    g = torch.Generator().manual_seed(0)
    st["box"].copy_(torch.randn(1024, 8, 3, generator=g))
    st["ids"].copy_(torch.randint(-2 ** 62, 2 ** 62, (1024, 2), generator=g))
    st["n"].copy_(torch.randint(-2 ** 31, 2 ** 31 - 1, (1024,), generator=g, dtype=torch.int64).int())
    old = {k: t.clone() for k, t in st.t.items()}
    ptrs = {k: st[k].data_ptr() for k in old}
    st.reserve(1024)
    assert {k: st[k].data_ptr() for k in old} == ptrs and all(st[k].shape[0] == 1024 for k in old)
    st.reserve(1025)
    for k, t in old.items():
        assert st[k].shape[0] == 2048 and st[k].dtype == t.dtype and st[k].shape[1:] == t.shape[1:]
        assert torch.equal(st[k][:1024].view(torch.uint8), t.view(torch.uint8))           # the old rows, bit for bit
        assert not st[k][1024:].view(torch.uint8).any()                                    # the new rows are zero
    ptrs = {k: st[k].data_ptr() for k in old}
    st.reserve(2048)
    assert {k: st[k].data_ptr() for k in old} == ptrs                                      # within capacity: the same storage
    st.reserve(5000)
    assert all(st[k].shape[0] == 8192 for k in old)
    st.rows = 3
    assert {k: tuple(v.shape) for k, v in st.filled().items()} == {"box": (3, 8, 3), "ids": (3, 2), "n": (3,)}
    assert st.filled()["ids"].data_ptr() == st["ids"].data_ptr()                           # views, not copies
    small = ds.RecordStore("cpu", 2, t=((3, 2, 4), torch.int64))
    small.reserve(2)
    assert small["t"].shape == (2, 3, 2, 4)
    small.reserve(3)
    assert small["t"].shape == (4, 3, 2, 4)


def test_read_back_is_bit_exact_and_one_copy(monkeypatch):
    nan_payload = np.array([0x7fc12345, 0xffc00001, 0x80000000, 0x00000001], np.uint32).view(np.float32)      # NaNs, -0.0, a denormal
    nan64 = np.array([0x7ff8000000abcdef, 0x8000000000000000, 0xfff0000000000000], np.uint64).view(np.float64)
    tensors = [torch.tensor([[1, -2, 2 ** 31 - 1], [-2 ** 31, 0, 7]], dtype=torch.int32), torch.from_numpy(nan_payload.copy()),
               torch.tensor([2 ** 62, -2 ** 63, -1], dtype=torch.int64), torch.from_numpy(nan64.copy()),
               torch.arange(12, dtype=torch.float32).reshape(3, 4).t(),                   # not contiguous
               torch.zeros((0, 3), dtype=torch.float64), torch.tensor([5], dtype=torch.int32)]
    want = [t.numpy().copy() for t in tensors]
    calls, cpu = [], torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (calls.append(1), cpu(self, *a, **k))[1])
    got = ds.read_back(tensors)
    assert len(calls) == 1
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == np.ascontiguousarray(w).tobytes()
    st = ds.RecordStore("cpu", a=((2,), torch.int64), b=((), torch.float32))
    st["a"][:3] = torch.tensor([[1, 2], [3, 4], [5, 6]])
    st["b"][:3] = torch.from_numpy(nan_payload[:3].copy())
    st.rows = 3
    del calls[:]
    rec, (status,) = st.read_back(torch.tensor([9], dtype=torch.int32))
    assert len(calls) == 1 and list(rec) == ["a", "b"] and rec["a"].tolist() == [[1, 2], [3, 4], [5, 6]] and rec["a"].dtype == np.int64
    assert rec["b"].tobytes() == nan_payload[:3].tobytes() and status.dtype == np.int32 and status.tolist() == [9]


def test_coercions_alias_the_right_dtype():
    f = torch.arange(6, dtype=torch.float32).reshape(2, 3).requires_grad_()
    i = torch.arange(6, dtype=torch.int64)
    assert ds.as_f32(f).data_ptr() == f.data_ptr() and not ds.as_f32(f).requires_grad
    assert ds.as_i64(i).data_ptr() == i.data_ptr()
    ft = f.detach().t()                                                                    # right dtype, not contiguous: one copy
    assert ds.as_f32(ft).is_contiguous() and torch.equal(ds.as_f32(ft), ft) and ds.as_f32(ft).data_ptr() != f.data_ptr()
    for t, fn, dt in ((i, ds.as_f32, torch.float32), (torch.tensor([True, False]), ds.as_f32, torch.float32), (i.int(), ds.as_i64, torch.int64),
                      (f, ds.as_i64, torch.int64)):
        out = fn(t)
        assert out.dtype == dt and out.is_contiguous() and not out.requires_grad and torch.equal(out, t.detach().to(dt))


def test_evaluating_restores_the_mode():
    m = torch.nn.Linear(2, 2)
    for training in (True, False):
        m.train(training)
        with ds.evaluating(m):
            assert not m.training and not torch.is_grad_enabled()
        assert m.training is training and torch.is_grad_enabled()
    m.train()
    with pytest.raises(RuntimeError, match="boom"):
        with ds.evaluating(m):
            raise RuntimeError("boom")
    assert m.training and torch.is_grad_enabled()
