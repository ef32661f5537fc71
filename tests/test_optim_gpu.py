"""Single-launch Adam and SGD (csrc/optim.hip, d3net_amd.optim.FusedAdam / FusedSGD) against torch.optim.Adam / torch.optim.SGD on
cloned parameters on the same device, fed identical gradients -- what the reference itself runs (model/pipeline.py:738-757,
model/pointgroup.py:372-384).  Tolerance: the project's `rel(...) < 1e-6` (tests/test_heads_gpu.py) for parameters and every
state tensor: both sides do the same fp32 operations and differ only in fused-multiply-add contraction."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-6
# sizes at which the block map can go wrong (256 threads, chunks of 4096): one element, one short of / one past a row of threads,
# one short of / exactly / one past a chunk, two chunks and one, and a 5-d kernel of 6912 elements
SHAPES = [(1,), (255,), (257,), (4095,), (4096,), (4097,), (2 * 4096 + 1,), (3, 3, 3, 16, 16)]


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-30))


def _pair(kind, pa, pb, **kw):
    from d3net_amd.optim import FusedAdam, FusedSGD
    if kind == "Adam":
        return FusedAdam(pa, **kw), torch.optim.Adam(pb, **kw)
    return FusedSGD(pa, **kw), torch.optim.SGD(pb, **kw)


def _params(shapes, dev):
    pa = [torch.nn.Parameter(torch.randn(s, device=dev)) for s in shapes]
    return pa, [torch.nn.Parameter(p.detach().clone()) for p in pa]


def _feed(pa, pb, skip=()):
    for i, (a, b) in enumerate(zip(pa, pb)):
        if i in skip:
            a.grad = None; b.grad = None
        else:
            g = torch.randn_like(a); a.grad = g.clone(); b.grad = g.clone()


def _state_names(kind, kw):
    return ("exp_avg", "exp_avg_sq") if kind == "Adam" else (("momentum_buffer",) if kw.get("momentum") else ())


def _assert_same(kind, kw, oa, ob, pa, pb, where=""):
    for i, (a, b) in enumerate(zip(pa, pb)):
        assert rel(a.detach(), b.detach()) < TOL, (where, i, rel(a.detach(), b.detach()))
        for k in _state_names(kind, kw):
            if b in ob.state and ob.state[b].get(k) is not None:
                assert rel(oa.state[a][k], ob.state[b][k]) < TOL, (where, i, k, rel(oa.state[a][k], ob.state[b][k]))
        if not _state_names(kind, kw):
            assert not oa.state.get(a), (where, i)                            # SGD without momentum keeps no state


CASES = [("Adam", {}), ("SGD", {"momentum": 0}), ("SGD", {"momentum": 0.9})]


@pytest.mark.parametrize("weight_decay", [0, 0.05])
@pytest.mark.parametrize("kind,extra", CASES)
def test_matches_torch_over_five_steps(dev, kind, extra, weight_decay):
    """parameters and every state tensor after 5 steps; one tensor's gradient object is replaced mid-run (address refresh), the
    others are overwritten in place"""
    torch.manual_seed(11)
    pa, pb = _params(SHAPES, dev)
    kw = dict(lr=2e-3, weight_decay=weight_decay, **extra)
    oa, ob = _pair(kind, pa, pb, **kw)
    for it in range(5):
        for a, b in zip(pa, pb):
            g = torch.randn_like(a)
            if a.grad is None or (it == 3 and a.numel() == 257):
                a.grad = g.clone()
            else:
                a.grad.copy_(g)
            b.grad = g.clone()
        oa.step(); ob.step()
    _assert_same(kind, kw, oa, ob, pa, pb)
    for a in pa:
        assert set(oa.state.get(a, {})) - {"step"} == set(_state_names(kind, kw))


def test_adam_late_tensors_start_at_t_1(dev):
    """tensors 1 and 3 get their first gradient at step 4: bias correction at t = 1 (|delta| ~ lr, not ~ lr / 3), untouched and
    stateless before; state_dict steps [7, 4, 7, 4]"""
    from d3net_amd.optim import FusedAdam
    torch.manual_seed(3)
    shapes, late, lr = [(40, 9), (4100,), (7,), (3, 5)], {1, 3}, 3e-3
    pa, pb = _params(shapes, dev)
    p0 = [p.detach().clone() for p in pa]
    kw = dict(lr=lr, weight_decay=0.02)
    oa, ob = FusedAdam(pa, **kw), torch.optim.Adam(pb, **kw)
    for it in range(1, 8):
        _feed(pa, pb, skip=late if it < 4 else ())
        before = pa[1].detach().clone()
        oa.step(); ob.step()
        if it == 3:
            for i in late:
                assert torch.equal(pa[i].detach(), p0[i]) and not oa.state.get(pa[i]), i
            assert set(oa.state_dict()["state"]) == {0, 2}
        if it == 4:
            d = (pa[1].detach() - before).abs()
            assert 0.9 * lr < float(d.median()) < 1.1 * lr, float(d.median())
    _assert_same("Adam", kw, oa, ob, pa, pb)
    sd = oa.state_dict()["state"]
    assert [float(sd[i]["step"]) for i in range(4)] == [7.0, 4.0, 7.0, 4.0]
    assert all(sd[i]["step"].dtype == torch.float32 and sd[i]["step"].dim() == 0 for i in range(4))


@pytest.mark.parametrize("weight_decay", [0, 0.02])
def test_sgd_late_tensors_take_the_first_update_rule(dev, weight_decay):
    """tensors 1 and 3 get their first gradient at step 4: buf = g + wd * p_before (the library clones g' into the new buffer),
    while the tensors that own a buffer take buf = mu * buf + g' in the same step; untouched and stateless before"""
    from d3net_amd.optim import FusedSGD
    torch.manual_seed(5)
    shapes, late = [(40, 9), (4100,), (7,), (3, 5)], {1, 3}
    pa, pb = _params(shapes, dev)
    p0 = [p.detach().clone() for p in pa]
    kw = dict(lr=3e-3, momentum=0.9, weight_decay=weight_decay)
    oa, ob = FusedSGD(pa, **kw), torch.optim.SGD(pb, **kw)
    for it in range(1, 8):
        _feed(pa, pb, skip=late if it < 4 else ())
        before = [p.detach().clone() for p in pa]
        oa.step(); ob.step()
        if it == 3:
            for i in late:
                assert torch.equal(pa[i].detach(), p0[i]) and not oa.state.get(pa[i]), i
            assert set(oa.state_dict()["state"]) == {0, 2}
        if it == 4:
            for i in late:
                want = pa[i].grad.double() + weight_decay * before[i].double()
                assert rel(oa.state[pa[i]]["momentum_buffer"], want) < TOL, i
            _assert_same("SGD", kw, oa, ob, pa, pb, "step 4")
    _assert_same("SGD", kw, oa, ob, pa, pb)
    assert all(set(oa.state[p]) == {"momentum_buffer"} for p in pa)


@pytest.mark.parametrize("kind,extra", [("Adam", {}), ("SGD", {"momentum": 0.9})])
def test_checkpoints_interchange_with_torch(dev, kind, extra):
    """fused -> torch -> two more steps on both; torch -> fused -> one more step; (SGD) a torch checkpoint taken before any step"""
    torch.manual_seed(7)
    shapes = [(40, 9), (4100,), (7,), (3, 5)]
    pa, pb = _params(shapes, dev)
    kw = dict(lr=3e-3, weight_decay=0.02, **extra)
    oa, ob = _pair(kind, pa, pb, **kw)
    for it in range(1, 5):
        _feed(pa, pb, skip={1, 3} if it < 3 else ())
        oa.step(); ob.step()
    sd = oa.state_dict()
    pc = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    oc = _pair(kind, pa, pc, **kw)[1]
    oc.load_state_dict(copy.deepcopy(sd))
    for it in range(2):
        _feed(pa, pc)
        oa.step(); oc.step()
    _assert_same(kind, kw, oa, oc, pa, pc, "fused -> torch")
    od = _pair(kind, pa, pc, **kw)[0]
    od.load_state_dict(copy.deepcopy(oc.state_dict()))
    _feed(pa, pc)
    od.step(); oc.step()
    _assert_same(kind, kw, od, oc, pa, pc, "torch -> fused")
    if kind == "Adam":
        got = od.state_dict()["state"]
        assert [float(got[i]["step"]) for i in range(4)] == [7.0, 5.0, 7.0, 5.0]
    # a checkpoint of the library's optimizer taken before its first step: no state at all; the first update rule applies
    pe, pf = _params(shapes, dev)
    oe, of = _pair(kind, pe, pf, **kw)
    oe.load_state_dict(copy.deepcopy(of.state_dict()))
    for it in range(2):
        _feed(pe, pf)
        oe.step(); of.step()
    _assert_same(kind, kw, oe, of, pe, pf, "fresh torch checkpoint")


def test_sgd_loaded_none_buffer_means_first_update(dev):
    """older checkpoints of the library store `momentum_buffer: None` for a tensor that has not been updated"""
    from d3net_amd.optim import FusedSGD
    torch.manual_seed(9)
    pa, pb = _params([(300,), (17,)], dev)
    kw = dict(lr=1e-2, momentum=0.9, weight_decay=0.01)
    oa, ob = FusedSGD(pa, **kw), torch.optim.SGD(pb, **kw)
    _feed(pa, pb, skip={1})
    oa.step(); ob.step()
    sd = copy.deepcopy(ob.state_dict())
    sd["state"][1] = {"momentum_buffer": None}
    oa2 = FusedSGD(pa, **kw)
    oa2.load_state_dict(sd)
    for it in range(2):
        _feed(pa, pb)
        oa2.step(); ob.step()
    _assert_same("SGD", kw, oa2, ob, pa, pb)


@pytest.mark.parametrize("kind,extra", CASES)
def test_two_param_groups_follow_steplr(dev, kind, extra):
    """group["lr"] is read on every step (StepLR rewrites it); each group has its own lr and weight_decay"""
    torch.manual_seed(13)
    pa, pb = _params([(40, 9), (4100,), (7,), (5000, 3)], dev)
    groups = lambda ps: [{"params": ps[:2], "lr": 4e-3, "weight_decay": 0.03}, {"params": ps[2:], "lr": 1e-3, "weight_decay": 0.0}]
    oa, ob = _pair(kind, groups(pa), groups(pb), lr=1.0, **extra)
    sa, sb = (torch.optim.lr_scheduler.StepLR(o, step_size=1, gamma=0.5) for o in (oa, ob))
    for it in range(4):
        _feed(pa, pb)
        oa.step(); ob.step()
        sa.step(); sb.step()
    assert [g["lr"] for g in oa.param_groups] == [g["lr"] for g in ob.param_groups] == [4e-3 / 16, 1e-3 / 16]
    _assert_same(kind, extra, oa, ob, pa, pb)


@pytest.mark.parametrize("kind,extra,joining", [("Adam", {}, 2), ("SGD", {"momentum": 0.9}, 2), ("SGD", {"momentum": 0}, 1)])
def test_one_launch_per_step_in_the_steady_state(dev, monkeypatch, kind, extra, joining):
    """library calls per step: one in the steady state; on the step where late tensors join, one per distinct step count for Adam
    (which stays at two: the counts never meet), two for SGD with momentum (buffer owners + first update), then one again"""
    from d3net_amd import _lib
    L = _lib.lib()
    name = "d3_adam" if kind == "Adam" else "d3_sgd"
    orig, calls = getattr(L, name), []
    monkeypatch.setattr(L, name, lambda *a: (calls.append(a[3]), orig(*a))[1])
    torch.manual_seed(17)
    pa, pb = _params([(40, 9), (4100,), (7,), (2 * 4096 + 1,)], dev)
    kw = dict(lr=1e-3, **extra)
    oa, ob = _pair(kind, pa, pb, **kw)
    per_step = []
    for it in range(1, 7):
        _feed(pa, pb, skip={1, 3} if it < 4 else ())
        n0 = len(calls)
        oa.step(); ob.step()
        per_step.append(len(calls) - n0)
    after = 2 if kind == "Adam" else 1
    assert per_step == [1, 1, 1, joining, after, after], per_step
    assert sum(calls[-after:]) == 1 + 2 + 1 + 3                                # every (tensor, chunk) block is launched once a step
    _assert_same(kind, kw, oa, ob, pa, pb)


def test_detector_trains_with_sgd_end_to_end(dev):
    """PointGroup.configure_optimizers() with classname SGD: two full steps train the backbone with momentum buffers and no Adam
    moments; a step without proposals leaves the ScoreNet parameters and their buffers bit-unchanged (the executors' stale flat
    gradients are dropped by the pre-hook, as test_no_stale_executor_gradients... pins for AdamW)"""
    from d3net_amd import synthetic as S
    from d3net_amd.config import default_conf
    from d3net_amd.optim import FusedSGD
    from d3net_amd.pointgroup import PointGroup
    cfg = default_conf(overrides={"model": {"blocks": [1, 2, 3]}, "train": {"optim": {"classname": "SGD"}}})
    torch.manual_seed(0)
    model = PointGroup(cfg).to(dev).train()
    model.teacher = True
    opt, = model.configure_optimizers()
    assert type(opt) is FusedSGD
    g, = opt.param_groups
    assert (g["lr"], g["momentum"], g["weight_decay"]) == (cfg.train.optim.lr, cfg.train.optim.momentum, cfg.train.optim.weight_decay)
    scene = S.small_scene(dims=(40, 32, 20), n_boxes=2, seed=3)
    kernel = model.backbone[1].blocks.block0.conv_branch[2].kernel
    bb = kernel.detach().clone()

    def step():
        model.zero_grad(set_to_none=True)
        loss, d = model.training_step(S.make_batch([scene], dev))
        loss.backward()
        opt.step()
        return d

    for _ in range(2):
        d = step()
        assert d["proposal_scores"][2].numel() - 1 > 0
    assert not torch.equal(kernel.detach(), bb)
    assert "momentum_buffer" in opt.state[kernel] and "exp_avg" not in opt.state[kernel]
    assert all(set(st) == {"momentum_buffer"} for st in opt.state.values())
    sn = {k: p.detach().clone() for k, p in model.score_net.named_parameters()}
    m1 = {k: opt.state[p]["momentum_buffer"].clone() for k, p in model.score_net.named_parameters()}
    assert any(float(v.abs().sum()) > 0 for v in m1.values())            # the ScoreNet did train
    bb = kernel.detach().clone()
    model.cluster_npoint_thre = 10 ** 9                                    # no cluster survives: the _no_proposals path
    d = step()
    assert d["proposal_scores"][2].numel() - 1 == 0
    torch.cuda.synchronize()
    for k, p in model.score_net.named_parameters():
        assert torch.equal(p.detach(), sn[k]), k
        assert torch.equal(opt.state[p]["momentum_buffer"], m1[k]), k
        assert p.grad is None, k
    assert not torch.equal(kernel.detach(), bb)                            # the backbone still trains
