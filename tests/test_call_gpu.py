"""d3net_amd._call on the device: the stream read under the guard is the thread's current one, workspaces are per stream."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_stream_guard_workspace_and_ptr(dev):
    from d3net_amd import _call, pointgroup_ops
    assert _call.ptr(None) is None
    t = torch.zeros(4, device=dev)
    assert _call.ptr(t).value == t.data_ptr() and _call.ptr(t[1:]).value == t.data_ptr() + 4
    with _call.on(dev):
        assert (_call.stream().value or 0) == torch.cuda.current_stream(dev).cuda_stream
        a = _call.workspace(100, dev, "test_call")
        assert a.device == dev and a.dtype == torch.uint8 and a.numel() >= 100
        assert _call.workspace(64, dev, "test_call").data_ptr() == a.data_ptr()              # same thread, stream and tag: the cached buffer
        assert _call.workspace(64, dev, "test_call_other").data_ptr() != a.data_ptr()
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side), _call.on(dev):
        assert side.cuda_stream != 0 and _call.stream().value == side.cuda_stream == torch.cuda.current_stream(dev).cuda_stream
        b = _call.workspace(100, dev, "test_call")
    assert b.data_ptr() != a.data_ptr()                                                      # one thread, two streams: two buffers
    with _call.on(dev):
        assert (_call.stream().value or 0) == torch.cuda.current_stream(dev).cuda_stream    # and back
    assert (pointgroup_ops._stream, pointgroup_ops._ptr, pointgroup_ops._on, pointgroup_ops._workspace) == \
        (_call.stream, _call.ptr, _call.on, _call.workspace)
    grown = _call.workspace(10 * a.numel(), dev, "test_call")                                # a request beyond the buffer replaces it
    assert grown.numel() >= 10 * a.numel()
    for key in [k for k in _call._ws_cache if str(k[1]).startswith("test_call")]:
        del _call._ws_cache[key]
