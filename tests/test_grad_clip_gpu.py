"""Global gradient-norm clipping and the non-finite skip inside the single-launch optimizers (csrc/optim.hip: grad_sumsq_kernel,
grad_clip_finish_kernel and the CTL instantiations of adamw_kernel / adam_kernel / sgd_kernel; d3net_amd.optim: `max_grad_norm`,
`skip_nonfinite`) against `torch.nn.utils.clip_grad_norm_` + torch.optim on cloned parameters -- what Lightning's
`Trainer(gradient_clip_val=...)` runs for the reference.
Tolerances.  The norm: float64 accumulation over < 1e8 terms errs by far less than a float32 ulp, which leaves one rounding
for the square root and the narrowing: the float32 nearest to the float64 reference or one of its two neighbours.  Parameters
and state against torch: the project's `rel(...) < 1e-6` (tests/test_optim_gpu.py); the two sides differ only in the last bits
of the coefficient (float64 accumulation here, float32 in the library), which tests/test_grad_clip_config.py shows to stay
inside that bound at these shapes."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-6
# the sizes of tests/test_optim_gpu.py: where a block map (256 threads, chunks of 4096) or a tail chunk can go wrong
SHAPES = [(1,), (255,), (257,), (4095,), (4096,), (4097,), (2 * 4096 + 1,), (3, 3, 3, 16, 16)]
CASES = [("AdamW", {}), ("Adam", {}), ("SGD", {"momentum": 0}), ("SGD", {"momentum": 0.9})]
STATE = {"AdamW": ("exp_avg", "exp_avg_sq"), "Adam": ("exp_avg", "exp_avg_sq")}
ENTRY = {"AdamW": "d3_adamw", "Adam": "d3_adam", "SGD": "d3_sgd"}


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-30))


def _fused(kind, params, **kw):
    from d3net_amd import optim as O
    return O._FUSED[kind](params, **kw)


def _torch(kind, params, **kw):
    return getattr(torch.optim, kind)(params, **kw)


def _params(shapes, dev):
    pa = [torch.nn.Parameter(torch.randn(s, device=dev)) for s in shapes]
    return pa, [torch.nn.Parameter(p.detach().clone()) for p in pa]


def _feed(pa, pb, skip=(), scale=1.0):
    for i, (a, b) in enumerate(zip(pa, pb)):
        if i in skip:
            a.grad = None; b.grad = None
        else:
            g = torch.randn_like(a) * scale; a.grad = g.clone(); b.grad = g.clone()


def _state_names(kind, kw):
    return STATE.get(kind) or (("momentum_buffer",) if kw.get("momentum") else ())


def _norm64(grads):
    """float64 reference of the total 2-norm, a 0-d float64 device tensor"""
    return torch.sqrt(sum((g.double() ** 2).sum() for g in grads))


def _assert_norm(got, grads, where=""):
    ref = _norm64(grads).float()
    assert got.dtype == torch.float32 and got.dim() == 0
    assert bool(torch.isfinite(got)), (where, float(got))
    near = [ref, torch.nextafter(ref, ref.new_tensor(math.inf)), torch.nextafter(ref, ref.new_tensor(-math.inf))]
    assert any(torch.equal(got, r) for r in near), (where, float(got), float(ref))


def _snapshot(kind, kw, opt, params):
    return [[p.detach().clone()] + [opt.state[p][k].clone() for k in _state_names(kind, kw) if k in opt.state.get(p, {})]
            for p in params]


def _assert_same(kind, kw, oa, ob, pa, pb, where=""):
    for i, (a, b) in enumerate(zip(pa, pb)):
        assert rel(a.detach(), b.detach()) < TOL, (where, i, rel(a.detach(), b.detach()))
        for k in _state_names(kind, kw):
            if b in ob.state and ob.state[b].get(k) is not None:
                assert rel(oa.state[a][k], ob.state[b][k]) < TOL, (where, i, k, rel(oa.state[a][k], ob.state[b][k]))


@pytest.mark.parametrize("scale", [1.0, 1e20, 1e-30])
@pytest.mark.parametrize("kind,extra", CASES)
def test_norm_value(dev, kind, extra, scale):
    """max_grad_norm = inf measures: the record's norm is the float64 reference narrowed to float32 (or a neighbour), also for
    gradients whose squares overflow (1e20) or underflow (1e-30) float32 -- the accumulation is in double"""
    torch.manual_seed(21)
    pa, pb = _params(SHAPES, dev)
    oa = _fused(kind, pa, lr=1e-6, max_grad_norm=math.inf, **extra)
    assert float(oa.last_grad_norm()) == 0.0
    for it in range(2):
        _feed(pa, pb, scale=scale)
        oa.step()
        _assert_norm(oa.last_grad_norm().clone(), [p.grad for p in pa], (scale, it))
    rec = oa._ctl.cpu()
    assert rec[1:2].view(torch.float32).item() == 1.0 and rec[2].item() == 0 and rec[3].item() == 0     # coef, skip, nskipped
    assert oa.last_grad_norm().data_ptr() == oa._ctl.data_ptr()                                         # aliases the record


@pytest.mark.parametrize("kind,extra", CASES)
def test_coefficient_of_one_is_exact(dev, kind, extra):
    """max_grad_norm above the norm: g * 1.0f is g; 5 steps are bit-equal to the unclipped entries on cloned inputs"""
    torch.manual_seed(22)
    pa, pb = _params(SHAPES, dev)
    kw = dict(lr=2e-3, weight_decay=0.05, **extra)
    oa, ob = _fused(kind, pa, max_grad_norm=1e6, **kw), _fused(kind, pb, **kw)
    for it in range(5):
        _feed(pa, pb)
        oa.step(); ob.step()
    assert 100.0 < float(oa.last_grad_norm()) < 1e6
    for x, y in zip(_snapshot(kind, kw, oa, pa), _snapshot(kind, kw, ob, pb)):
        assert len(x) == len(y) == 1 + len(_state_names(kind, kw))
        assert all(torch.equal(u, v) for u, v in zip(x, y))


@pytest.mark.parametrize("weight_decay", [0, 0.05])
@pytest.mark.parametrize("kind,extra", CASES)
def test_clipping_matches_torch_over_five_steps(dev, kind, extra, weight_decay):
    """max_grad_norm about a tenth of the norm (sqrt(27906) ~ 167 for these shapes) against clip_grad_norm_ + torch.optim;
    `p.grad` keeps its unclipped value on the device path (torch's is rewritten)"""
    torch.manual_seed(23)
    pa, pb = _params(SHAPES, dev)
    kw = dict(lr=2e-3, weight_decay=weight_decay, **extra)
    oa, ob = _fused(kind, pa, max_grad_norm=16.0, **kw), _torch(kind, pb, **kw)
    for it in range(5):
        _feed(pa, pb)
        gs = [a.grad.clone() for a in pa]
        oa.step()
        torch.nn.utils.clip_grad_norm_(pb, 16.0)
        ob.step()
        assert all(torch.equal(a.grad, g) for a, g in zip(pa, gs))
        assert rel(pb[7].grad, gs[7]) > 0.5                            # while the library's side was clipped, by about 10
    _assert_norm(oa.last_grad_norm().clone(), [p.grad for p in pa])
    _assert_same(kind, kw, oa, ob, pa, pb)


@pytest.mark.parametrize("kind,extra", CASES)
def test_two_param_groups_share_one_norm(dev, kind, extra):
    """the norm is global over the groups, as clip_grad_norm_(all parameters) and Lightning have it; each group keeps its lr"""
    torch.manual_seed(24)
    pa, pb = _params([(40, 9), (4100,), (7,), (5000, 3)], dev)
    groups = lambda ps: [{"params": ps[:2], "lr": 4e-3, "weight_decay": 0.03}, {"params": ps[2:], "lr": 1e-3, "weight_decay": 0.0}]
    oa, ob = _fused(kind, groups(pa), lr=1.0, max_grad_norm=12.0, **extra), _torch(kind, groups(pb), lr=1.0, **extra)
    for it in range(4):
        _feed(pa, pb)
        oa.step()
        _assert_norm(oa.last_grad_norm().clone(), [p.grad for p in pa], it)
        torch.nn.utils.clip_grad_norm_(pb, 12.0)
        ob.step()
    assert float(oa.last_grad_norm()) > 100.0
    _assert_same(kind, extra, oa, ob, pa, pb)


@pytest.mark.parametrize("kind,extra", CASES)
def test_tensors_without_a_gradient_stay_out_of_the_norm(dev, kind, extra):
    """tensors 1 and 3 get their first gradient at step 4: absent from the norm before, part of it after; Adam's late tensors
    start at t = 1 (state_dict steps [7, 4, 7, 4])"""
    torch.manual_seed(25)
    shapes, late = [(40, 9), (4100,), (7,), (3, 5)], {1, 3}
    pa, pb = _params(shapes, dev)
    p0 = [p.detach().clone() for p in pa]
    kw = dict(lr=3e-3, weight_decay=0.02, **extra)
    oa, ob = _fused(kind, pa, max_grad_norm=3.0, **kw), _torch(kind, pb, **kw)
    for it in range(1, 8):
        _feed(pa, pb, skip=late if it < 4 else ())
        oa.step()
        _assert_norm(oa.last_grad_norm().clone(), [p.grad for p in pa if p.grad is not None], it)
        torch.nn.utils.clip_grad_norm_(pb, 3.0)
        ob.step()
        if it == 3:
            assert float(oa.last_grad_norm()) < 25.0                   # sqrt(367) ~ 19; with the late tensors sqrt(4482) ~ 67
            for i in late:
                assert torch.equal(pa[i].detach(), p0[i]) and not oa.state.get(pa[i]), i
        if it == 4:
            assert float(oa.last_grad_norm()) > 50.0
            _assert_same(kind, kw, oa, ob, pa, pb, "step 4")
    _assert_same(kind, kw, oa, ob, pa, pb)
    if kind != "SGD":
        sd = oa.state_dict()["state"]
        assert [float(sd[i]["step"]) for i in range(4)] == [7.0, 4.0, 7.0, 4.0]


@pytest.mark.parametrize("bad", [math.inf, math.nan])
@pytest.mark.parametrize("kind,extra", CASES)
def test_non_finite_gradient_skips_the_step(dev, kind, extra, bad):
    """an inf / a NaN in the last element of the (4097,) tensor -- a one-element tail chunk: parameters and state bit-unchanged,
    one skipped step counted, the gradients untouched; the step counts still advance, so the following finite step is torch's
    with state[p]["step"] advanced by hand"""
    torch.manual_seed(26)
    pa, pb = _params(SHAPES, dev)
    kw = dict(lr=2e-3, weight_decay=0.05, **extra)
    oa, ob = _fused(kind, pa, max_grad_norm=16.0, **kw), _torch(kind, pb, **kw)

    def both():
        _feed(pa, pb)
        oa.step()
        torch.nn.utils.clip_grad_norm_(pb, 16.0)
        ob.step()

    both(); both()
    assert oa.nonfinite_steps() == 0
    before = _snapshot(kind, kw, oa, pa)
    _feed(pa, pb)
    pa[5].grad[-1] = bad
    gs = [a.grad.clone() for a in pa]
    oa.step()
    after = _snapshot(kind, kw, oa, pa)
    for x, y in zip(before, after):
        assert len(x) == len(y) and all(torch.equal(u, v) for u, v in zip(x, y))
    assert all(torch.equal(a.grad.view(torch.int32), g.view(torch.int32)) for a, g in zip(pa, gs))     # bitwise: a NaN != itself
    assert oa.nonfinite_steps() == 1 and not math.isfinite(float(oa.last_grad_norm()))
    for b in pb:                                                       # the library's optimizer sits this step out ...
        if "step" in ob.state.get(b, {}):
            ob.state[b]["step"] += 1                                   # ... but counts it, as the device path does
    both()
    assert oa.nonfinite_steps() == 1 and math.isfinite(float(oa.last_grad_norm()))
    _assert_same(kind, kw, oa, ob, pa, pb, "the step after the skipped one")
    if kind != "SGD":
        assert {float(st["step"]) for st in oa.state_dict()["state"].values()} == {4.0}


@pytest.mark.parametrize("bad", [math.inf, math.nan])
@pytest.mark.parametrize("kind,extra", CASES)
def test_skip_nonfinite_false_lets_it_propagate(dev, kind, extra, bad):
    """as through torch: inf * coef(= 0) and NaN coefficients reach the parameters; the step is still counted as non-finite"""
    torch.manual_seed(27)
    pa, pb = _params(SHAPES, dev)
    oa = _fused(kind, pa, lr=2e-3, max_grad_norm=16.0, skip_nonfinite=False, **extra)
    _feed(pa, pb)
    pa[5].grad[-1] = bad
    oa.step()
    assert not bool(torch.isfinite(pa[5].detach()).all())
    assert oa.nonfinite_steps() == 1


@pytest.mark.parametrize("kind,extra", CASES)
def test_records_and_parameters_are_deterministic(dev, kind, extra):
    """two optimizers fed the same gradients: bit-equal records and parameters (fixed-order reductions, no atomics)"""
    torch.manual_seed(28)
    pa, pb = _params(SHAPES, dev)
    kw = dict(lr=2e-3, weight_decay=0.05, max_grad_norm=16.0, **extra)
    oa, ob = _fused(kind, pa, **kw), _fused(kind, pb, **kw)
    for it in range(3):
        _feed(pa, pb)
        oa.step(); ob.step()
        assert torch.equal(oa._ctl, ob._ctl), it
    assert float(oa.last_grad_norm()) > 16.0
    for x, y in zip(_snapshot(kind, kw, oa, pa), _snapshot(kind, kw, ob, pb)):
        assert all(torch.equal(u, v) for u, v in zip(x, y))


@pytest.mark.parametrize("kind,extra", CASES)
def test_launch_count(dev, monkeypatch, kind, extra):
    """library calls of a one-group step in the steady state: clipping on -> one d3_grad_sumsq, one d3_grad_clip_finish, one
    _clipped update and no unclipped one; max_grad_norm=None -> the unclipped entry alone, none of the new entries"""
    from d3net_amd import _lib
    L = _lib.lib()
    calls = []
    names = ("d3_grad_sumsq", "d3_grad_clip_finish", ENTRY[kind], ENTRY[kind] + "_clipped")
    for n in names:
        monkeypatch.setattr(L, n, (lambda n, orig: lambda *a: (calls.append(n), orig(*a))[1])(n, getattr(L, n)))
    torch.manual_seed(29)
    pa, pb = _params([(40, 9), (4100,), (7,), (2 * 4096 + 1,)], dev)
    oa, ob = _fused(kind, pa, lr=1e-3, max_grad_norm=1.0, **extra), _fused(kind, pb, lr=1e-3, **extra)
    for it in range(3):
        _feed(pa, pb)
        del calls[:]
        oa.step()
        assert calls == ["d3_grad_sumsq", "d3_grad_clip_finish", ENTRY[kind] + "_clipped"], (it, calls)
        del calls[:]
        ob.step()
        assert calls == [ENTRY[kind]], (it, calls)


def test_detector_trains_with_clipping_end_to_end(dev):
    """PointGroup.configure_optimizers() with train.optim.max_grad_norm set small: two full steps train the backbone with a
    finite loss and a norm above the bound; on a step without proposals the ScoreNet parameters stay bit-unchanged and the
    logged norm is the float64 norm over the live gradients only (the executors' stale flat-buffer gradients are dropped by the
    pre-hook before the table -- and with it the norm -- is resolved)"""
    from d3net_amd import synthetic as S
    from d3net_amd.config import default_conf
    from d3net_amd.optim import FusedAdamW
    from d3net_amd.pointgroup import PointGroup
    max_norm = 1e-3
    cfg = default_conf(overrides={"model": {"blocks": [1, 2, 3]}, "train": {"optim": {"max_grad_norm": max_norm}}})
    torch.manual_seed(0)
    model = PointGroup(cfg).to(dev).train()
    model.teacher = True
    opt, = model.configure_optimizers()
    assert type(opt) is FusedAdamW and opt.max_grad_norm == max_norm and opt.skip_nonfinite is True
    assert "max_grad_norm" not in opt.param_groups[0]
    scene = S.small_scene(dims=(40, 32, 20), n_boxes=2, seed=3)
    kernel = model.backbone[1].blocks.block0.conv_branch[2].kernel
    bb = kernel.detach().clone()
    params = opt.param_groups[0]["params"]

    def step():
        model.zero_grad(set_to_none=True)
        loss, d = model.training_step(S.make_batch([scene], dev))
        loss.backward()
        opt.step()
        assert bool(torch.isfinite(loss))
        return d

    for _ in range(2):
        d = step()
        assert d["proposal_scores"][2].numel() - 1 > 0
        assert float(opt.last_grad_norm()) > max_norm
        _assert_norm(opt.last_grad_norm().clone(), [p.grad for p in params if p.grad is not None])
    assert not torch.equal(kernel.detach(), bb)
    assert opt.nonfinite_steps() == 0
    sn = {k: p.detach().clone() for k, p in model.score_net.named_parameters()}
    with_score_net = sum(1 for p in params if p.grad is not None)
    bb = kernel.detach().clone()
    model.cluster_npoint_thre = 10 ** 9                                    # no cluster survives: the _no_proposals path
    d = step()
    assert d["proposal_scores"][2].numel() - 1 == 0
    for k, p in model.score_net.named_parameters():
        assert torch.equal(p.detach(), sn[k]), k
        assert p.grad is None, k
    live = [p.grad for p in params if p.grad is not None]
    assert 0 < len(live) < with_score_net
    _assert_norm(opt.last_grad_norm().clone(), live, "no proposals")
    assert not torch.equal(kernel.detach(), bb)                            # the backbone still trains
