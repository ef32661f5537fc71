"""`train.optim.classname` is honoured by the model classes (reference: model/pipeline.py:738-757, model/pointgroup.py:372-384):
host-resident modules get the torch.optim class of that name with the config's lr / momentum / weight_decay; the single-launch
classes refuse the options their kernels do not implement before they touch the library; the two entry points are bound."""
import types

import numpy as np
import pytest
import torch

LR, MOM, WD = 0.0031, 0.85, 0.0007
NAMES = {"Adam": torch.optim.Adam, "AdamW": torch.optim.AdamW, "SGD": torch.optim.SGD, None: torch.optim.AdamW}


def _cfg(classname):
    from d3net_amd.config import default_conf
    optim = {"classname": classname, "lr": LR, "momentum": MOM, "weight_decay": WD}
    cfg = default_conf(overrides={
        "model": {"blocks": [1, 2, 3], "num_graph_steps": 2, "num_locals": 10, "use_relation": True, "use_orientation": True,
                  "match_type": "Transformer", "use_lang_classifier": True, "use_bidir": False, "num_bbox_class": 18,
                  "loss_type": "cross_entropy", "no_captioning": True, "no_grounding": True},
        "data": {"num_des_per_scene": 4, "max_spk_len": 30, "max_lis_len": 126, "min_iou_threshold": 0.25, "num_ori_bins": 6},
        "train": {"use_rl": False, "sample_topn": 1, "optim": optim}})
    if classname is None:
        del cfg.train.optim["classname"]
        assert "classname" not in cfg.train.optim
    return cfg


@pytest.fixture(scope="module")
def models():
    """one host-resident detector and pipeline; the tests swap `cfg` (configure_optimizers reads nothing else)"""
    from d3net_amd import synthetic as S
    from d3net_amd.pipeline import PipelineNet
    from d3net_amd.pointgroup import PointGroup
    V = 50
    ds = {"train": types.SimpleNamespace(vocabulary=S.make_vocabulary(V), glove=np.zeros((V, 300), np.float32))}
    cfg = _cfg("AdamW")
    return PointGroup(cfg), PipelineNet(cfg, ds)


def _check_group(opt, classname, detector):
    assert type(opt) is NAMES[classname]
    g, = opt.param_groups
    assert g["lr"] == LR
    if classname == "SGD":
        assert g["momentum"] == MOM and g["weight_decay"] == WD and g["dampening"] == 0 and not g["nesterov"]
    elif classname == "Adam" and detector:
        assert g["weight_decay"] == 0                    # model/pointgroup.py:378 passes lr alone
    else:
        assert g["weight_decay"] == WD


@pytest.mark.parametrize("classname", ["Adam", "AdamW", "SGD", None])
def test_pipeline_builds_the_named_optimizer_with_steplr(models, classname):
    _, net = models
    net.cfg = _cfg(classname)
    opts, scheds = net.configure_optimizers()
    assert len(opts) == 1 and len(scheds) == 1
    _check_group(opts[0], classname, detector=False)
    want = [p for p in net.parameters() if p.requires_grad]
    assert len(opts[0].param_groups[0]["params"]) == len(want) and all(a is b for a, b in zip(opts[0].param_groups[0]["params"], want))
    s = scheds[0]
    assert type(s) is torch.optim.lr_scheduler.StepLR and s.step_size == 10 and s.gamma == 0.8 and s.optimizer is opts[0]


@pytest.mark.parametrize("classname", ["Adam", "AdamW", "SGD", None])
def test_detector_builds_the_named_optimizer_without_a_scheduler(models, classname):
    det, _ = models
    det.cfg = _cfg(classname)
    out = det.configure_optimizers()
    assert isinstance(out, list) and len(out) == 1
    _check_group(out[0], classname, detector=True)
    want = [p for p in det.parameters() if p.requires_grad]
    assert len(out[0].param_groups[0]["params"]) == len(want)


def test_an_unknown_name_is_refused(models):
    det, net = models
    for m in (det, net):
        m.cfg = _cfg("RMSprop")
        with pytest.raises(ValueError, match="Adam, AdamW, SGD"):
            m.configure_optimizers()
    det.cfg = net.cfg = _cfg("AdamW")


def test_fused_classes_refuse_what_the_kernels_do_not_implement(monkeypatch):
    from d3net_amd import _lib
    from d3net_amd.optim import FusedAdam, FusedSGD

    def touched():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", touched)
    p = [torch.nn.Parameter(torch.zeros(3))]
    for cls, kw in ((FusedSGD, "nesterov"), (FusedSGD, "dampening"), (FusedSGD, "maximize"), (FusedSGD, "amsgrad"),
                    (FusedAdam, "amsgrad"), (FusedAdam, "maximize")):
        with pytest.raises(ValueError, match=kw):
            cls(p, lr=0.1, **{kw: True})
    FusedSGD(p, lr=0.1, momentum=0.9, weight_decay=1e-4)          # the accepted surface still constructs
    FusedAdam(p, lr=0.1, betas=(0.9, 0.99), eps=1e-6, weight_decay=1e-4)
    # a checkpoint of the library's class with such an option set is refused too, before any state is replaced
    ref = torch.optim.SGD([torch.nn.Parameter(torch.zeros(3))], lr=0.1, momentum=0.9, nesterov=True)
    with pytest.raises(ValueError, match="nesterov"):
        FusedSGD(p, lr=0.1, momentum=0.9).load_state_dict(ref.state_dict())
    ref = torch.optim.Adam([torch.nn.Parameter(torch.zeros(3))], lr=0.1, amsgrad=True)
    with pytest.raises(ValueError, match="amsgrad"):
        FusedAdam(p, lr=0.1).load_state_dict(ref.state_dict())


def test_state_layouts_are_the_librarys():
    """no GPU: state_dict() of hand-set states in torch.optim's layouts, loaded by the library's classes and back"""
    from d3net_amd.optim import FusedAdam, FusedSGD
    p = torch.nn.Parameter(torch.zeros(5))
    a = FusedAdam([p], lr=1e-3)
    a.state[p] = {"step": 3, "exp_avg": torch.ones(5), "exp_avg_sq": torch.full((5,), 2.0)}
    st = a.state_dict()["state"][0]
    assert torch.is_tensor(st["step"]) and st["step"].dtype == torch.float32 and float(st["step"]) == 3.0
    assert st is not a.state[p] and isinstance(a.state[p]["step"], int)
    ref = torch.optim.Adam([torch.nn.Parameter(torch.zeros(5))], lr=1e-3)
    ref.load_state_dict(a.state_dict())
    assert float(list(ref.state.values())[0]["step"]) == 3.0
    a2 = FusedAdam([torch.nn.Parameter(torch.zeros(5))], lr=1e-3)
    a2.load_state_dict(ref.state_dict())
    assert list(a2.state.values())[0]["step"] == 3
    s = FusedSGD([p], lr=1e-2, momentum=0.9)
    assert s.state_dict()["state"] == {}
    s.state[p] = {"momentum_buffer": torch.ones(5)}
    assert set(s.state_dict()["state"][0]) == {"momentum_buffer"}
    q = torch.nn.Parameter(torch.ones(5))
    ref = torch.optim.SGD([q], lr=1e-2, momentum=0.9)
    ref.load_state_dict(s.state_dict())
    q.grad = torch.ones(5)
    ref.step()                                                    # the loaded groups carry every key the library's step reads
    assert torch.equal(ref.state[q]["momentum_buffer"], torch.full((5,), 1.9))


def test_binding_table_has_the_two_entry_points(built_lib):
    from d3net_amd import _lib
    assert {"d3_adam", "d3_sgd"} <= set(_lib.SIGNATURES)
    l = _lib.lib()
    assert hasattr(l, "d3_adam") and hasattr(l, "d3_sgd")
