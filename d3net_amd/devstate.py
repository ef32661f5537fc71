"""What a device-side epoch accumulator is made of: the batch check, the growable record store, the
one read-back and the dtype coercions that DetectionEvaluator, CaptionEvaluator, GroundingEvaluator and the two submissions share."""
import contextlib

import numpy as np
import torch

INTS = (torch.int32, torch.int64)
FLOATS = (torch.float32,)
FLAGS = (torch.float32, torch.bool, torch.uint8) + INTS       # what a mask may arrive as
GROUND_MAX_K = 4096                                           # proposal slots per scene of csrc/grounding_eval.hip and csrc/submission.hip


def check_batch(name, d, table, geometry, device=None, state=None):
    """Refuse a bad batch with ValueError before anything is launched.  table: key -> (allowed dtypes, allowed shapes) with a
    shape's entries ints or names of the dimensions `geometry(d)` returns as a dict; allowed shapes None leaves the key's shape
    to `geometry`, a table value None asks only for the key's presence (a key that is no tensor).  The order is fixed: missing
    keys, values that are no tensors, geometry(d) -- the class's own rule, it derives the dimensions and checks the limits --
    shapes, dtypes, device.  The device comes last: a well-formed batch in host memory is refused for where it lives, a malformed
    one for what is wrong with it.  Every tensor lives on a GPU, on `device` when that names an index, on the device of the
    first key and on the device of `state` (the accumulator's status word, None before the first batch).  -> the dimensions"""
    missing = [k for k in table if k not in d]
    if missing:
        raise ValueError("%s: missing %s" % (name, missing))
    keys = [k for k in table if table[k] is not None]
    for k in keys:
        if not torch.is_tensor(d[k]):
            raise ValueError("%s: %s must be a tensor" % (name, k))
    dims = geometry(d)
    for k in keys:
        shapes = [tuple(dims.get(n, n) for n in s) for s in table[k][1] or ()]
        if shapes and tuple(d[k].shape) not in shapes:
            raise ValueError("%s: %s has shape %s, expected %s" % (name, k, tuple(d[k].shape), " or ".join(map(str, shapes))))
    for k in keys:
        if d[k].dtype not in table[k][0]:
            raise ValueError("%s: %s has dtype %s, expected one of %s" % (name, k, d[k].dtype, table[k][0]))
    first = d[keys[0]].device
    home = state.device if state is not None else device if device is not None else first
    for k in keys:
        at = d[k].device
        if not d[k].is_cuda:
            raise ValueError("%s: %s is in host memory (%s); it must be on the GPU, there is no CPU fallback" % (name, k, at))
        if (device is not None and device.index is not None and at != device) or at != first or (state is not None and at != state.device):
            raise ValueError("%s: %s is on %s; the batches of one accumulation live on one GPU (%s)" % (name, k, at, home))
    return dims


@contextlib.contextmanager
def evaluating(module):
    """run the block with `module` in eval() mode under no_grad(); the module's mode is restored afterwards"""
    was_training = module.training
    module.eval()
    try:
        with torch.no_grad():
            yield module
    finally:
        module.train(was_training)


def as_f32(t):
    """contiguous float32 without autograd history; a float32 tensor is not converted (and not copied when contiguous)"""
    return t.detach().contiguous() if t.dtype == torch.float32 else t.detach().float().contiguous()


def as_i64(t):
    return t.detach().contiguous() if t.dtype == torch.int64 else t.detach().long().contiguous()


def read_back(tensors):
    """the one read-back: the tensors as one byte run, one `.cpu()` -> numpy arrays of their dtypes and shapes"""
    flat = torch.cat([t.contiguous().view(-1).view(torch.uint8) for t in tensors]).cpu().numpy()
    out, pos = [], 0
    for t in tensors:
        n = t.numel() * t.element_size()
        out.append(flat[pos:pos + n].view(np.dtype(str(t.dtype).replace("torch.", ""))).reshape(tuple(t.shape)))
        pos += n
    return out


class RecordStore:
    """Per-row device tensors that grow together: fields name -> (row shape, dtype), `rows` of them filled.  The kernels write rows
    through `store[name]` (the whole storage) after `reserve`; the count is the owner's to advance."""

    def __init__(self, device, capacity=1024, **fields):
        self.t = {k: torch.zeros((capacity,) + tuple(shape), dtype=dt, device=device) for k, (shape, dt) in fields.items()}
        self.rows = 0

    def __getitem__(self, name):
        return self.t[name]

    def reserve(self, rows):
        """room for `rows` rows: the capacity doubles, the old rows are copied on the device, the rest is zero"""
        for k, t in self.t.items():
            cap = t.shape[0]
            if cap < rows:
                while cap < rows:
                    cap *= 2
                self.t[k] = torch.zeros((cap,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
                self.t[k][:t.shape[0]].copy_(t)

    def filled(self):
        """views of the filled rows"""
        return {k: t[:self.rows] for k, t in self.t.items()}

    def read_back(self, *more):
        """the filled rows, and `more` tensors behind them, in one read-back -> ({name: array}, arrays of `more`)"""
        back = read_back(list(self.filled().values()) + list(more))
        return dict(zip(self.t, back)), back[len(self.t):]
