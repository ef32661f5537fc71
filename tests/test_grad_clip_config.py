"""`train.optim.max_grad_norm` / `train.optim.skip_nonfinite` (d3net_amd.optim.from_config) on host parameters, where the key means
`torch.nn.utils.clip_grad_norm_` in front of the torch.optim step -- what Lightning's `Trainer(gradient_clip_val=...)` is to the
reference -- and the host-side surface of the device options: constructor arguments, `param_groups`, `state_dict()`, the binding
table.  No GPU."""
import copy
import math
import pickle

import pytest
import torch

from d3net_amd.config import Cfg

KEYS = {"Adam": ("lr", "weight_decay"), "AdamW": ("lr", "weight_decay"), "SGD": ("lr", "momentum", "weight_decay")}
SHAPES = [(1,), (255,), (257,), (4095,), (4096,), (4097,), (2 * 4096 + 1,), (3, 3, 3, 16, 16)]
NEW = ("d3_grad_sumsq", "d3_grad_clip_finish", "d3_adamw_clipped", "d3_adam_clipped", "d3_sgd_clipped")


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-30))


def _cfg(name, **extra):
    return Cfg(dict(classname=name, lr=2e-3, momentum=0.9, weight_decay=0.05, **extra))


def _params(shapes):
    pa = [torch.nn.Parameter(torch.randn(s)) for s in shapes]
    return pa, [torch.nn.Parameter(p.detach().clone()) for p in pa]


def _no_drop():
    raise AssertionError("host parameters own no executor gradients")


@pytest.mark.parametrize("name", sorted(KEYS))
def test_host_parameters_clip_as_clip_grad_norm(name):
    """from_config with the key set == the plain optimizer fed hand-clipped gradients (coefficient max_norm / (norm + 1e-6),
    norm in float64 here): parameters after 3 steps within 1e-6, and the gradients ARE rewritten on the host, as torch does"""
    from d3net_amd.optim import from_config
    torch.manual_seed(1)
    pa, pb = _params([(40, 9), (4100,), (7,)])
    oa = from_config(_cfg(name, max_grad_norm=0.5), pa, KEYS, _no_drop)
    ob = from_config(_cfg(name), pb, KEYS, _no_drop)
    assert type(oa) is type(ob) is getattr(torch.optim, name)
    for _ in range(3):
        gs = [torch.randn_like(p) for p in pa]
        norm = math.sqrt(sum(float((g.double() ** 2).sum()) for g in gs))
        assert norm > 5.0
        for a, b, g in zip(pa, pb, gs):
            a.grad = g.clone()
            b.grad = g * (0.5 / (norm + 1e-6))
        oa.step(); ob.step()
        for a, b in zip(pa, pb):
            assert rel(a.grad, b.grad) < 1e-6
    for a, b in zip(pa, pb):
        assert rel(a.detach(), b.detach()) < 1e-6
    total = math.sqrt(sum(float((a.grad.double() ** 2).sum()) for a in pa))
    assert abs(total - 0.5) < 1e-5


@pytest.mark.parametrize("off", [{}, {"max_grad_norm": None}, {"max_grad_norm": 0}, {"max_grad_norm": 0.0}])
def test_key_absent_none_or_zero_is_the_plain_optimizer(off):
    from d3net_amd.optim import from_config
    torch.manual_seed(2)
    pa, pb = _params([(33,), (5, 4)])
    oa = from_config(_cfg("SGD", **off), pa, KEYS, _no_drop)
    ob = torch.optim.SGD(pb, lr=2e-3, momentum=0.9, weight_decay=0.05)
    assert type(oa) is torch.optim.SGD and not oa._optimizer_step_pre_hooks
    for _ in range(2):
        for a, b in zip(pa, pb):
            g = 100 * torch.randn_like(a); a.grad = g.clone(); b.grad = g.clone()
        oa.step(); ob.step()
    for a, b in zip(pa, pb):
        assert torch.equal(a.detach(), b.detach()) and torch.equal(a.grad, b.grad)


@pytest.mark.parametrize("name", sorted(KEYS))
def test_options_are_attributes_not_groups_or_checkpoint_entries(name):
    """the constructors take the two keywords (no device work before the first step); `param_groups` and `state_dict()` are what
    they are without them, so checkpoints keep interchanging with torch.optim; bad values are refused; pickling keeps them"""
    from d3net_amd import optim as O
    cls = O._FUSED[name]
    p = [torch.nn.Parameter(torch.randn(5))]
    plain, clipped = cls(p, lr=1e-3), cls(p, lr=1e-3, max_grad_norm=2.5, skip_nonfinite=False)
    assert (plain.max_grad_norm, plain.skip_nonfinite) == (None, True)
    assert (clipped.max_grad_norm, clipped.skip_nonfinite) == (2.5, False)
    assert cls(p, max_grad_norm=math.inf).max_grad_norm == math.inf
    assert plain.param_groups[0].keys() == clipped.param_groups[0].keys()
    assert not {"max_grad_norm", "skip_nonfinite"} & set(clipped.param_groups[0]) and not {"max_grad_norm", "skip_nonfinite"} & set(clipped.defaults)
    sa, sb = plain.state_dict(), clipped.state_dict()
    assert sa.keys() == sb.keys() == {"state", "param_groups"} and sa["param_groups"] == sb["param_groups"]
    getattr(torch.optim, name)(p, lr=1e-3).load_state_dict(copy.deepcopy(sb))     # still torch.optim's layout
    for bad in (0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            cls(p, max_grad_norm=bad)
    again = pickle.loads(pickle.dumps(clipped))
    assert (again.max_grad_norm, again.skip_nonfinite) == (2.5, False)
    assert clipped.nonfinite_steps() == 0                                      # no record, no read-back before the first step


def test_new_entries_are_bound():
    from d3net_amd import _lib
    for n in NEW:
        assert n in _lib.SIGNATURES, n
    vp = _lib.SIGNATURES["d3_adamw"][1][-1]
    for n in ("d3_adamw", "d3_adam", "d3_sgd"):       # the argument list of the unclipped entry, `ctl` before `stream`
        ret, args = _lib.SIGNATURES[n]
        assert _lib.SIGNATURES[n + "_clipped"] == (ret, args[:-1] + [vp, args[-1]]), n
    assert len(_lib.SIGNATURES["d3_grad_sumsq"][1]) == 6 and len(_lib.SIGNATURES["d3_grad_clip_finish"][1]) == 5


@pytest.mark.parametrize("weight_decay", [0, 0.05])
@pytest.mark.parametrize("name,extra", [("AdamW", {}), ("Adam", {}), ("SGD", {"momentum": 0}), ("SGD", {"momentum": 0.9})])
def test_float64_norm_coefficient_stays_within_the_bound_of_torchs_float32_route(name, extra, weight_decay):
    """the premise of tests/test_grad_clip_gpu.py's comparison against torch, checked where it costs nothing: the device path
    takes the norm in float64 and narrows it once, `clip_grad_norm_` accumulates in float32; the two coefficients differ in
    their last bits.  5 steps of torch.optim on the GPU test's shapes, one side clipped by `clip_grad_norm_`, the other by
    g * min(1.0f, max_norm / (float32(norm64) + 1e-6f)): parameters and state within rel < 1e-6 of each other."""
    torch.manual_seed(4)
    pa, pb = _params(SHAPES)
    kw = dict(lr=2e-3, weight_decay=weight_decay, **extra)
    oa, ob = (getattr(torch.optim, name)(ps, **kw) for ps in (pa, pb))
    for _ in range(5):
        gs = [torch.randn_like(p) for p in pa]
        norm = torch.sqrt(sum((g.double() ** 2).sum() for g in gs)).float()
        max_norm = torch.tensor(float(norm) / 10, dtype=torch.float32)
        coef = torch.clamp(max_norm / (norm + torch.tensor(1e-6, dtype=torch.float32)), max=1.0)
        assert coef.dtype == torch.float32
        for a, b, g in zip(pa, pb, gs):
            a.grad = g.clone()
            b.grad = g * coef
        torch.nn.utils.clip_grad_norm_(pa, float(max_norm))
        oa.step(); ob.step()
    for a, b in zip(pa, pb):
        assert rel(a.detach(), b.detach()) < 1e-6
        for k, v in ob.state[b].items():
            if torch.is_tensor(v) and v.dim():
                assert rel(oa.state[a][k], v) < 1e-6, k
