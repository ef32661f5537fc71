"""AdamW, Adam and SGD over every parameter tensor of a group in ONE launch (csrc/heads.hip: adamw_kernel; csrc/optim.hip:
adam_kernel, sgd_kernel).

Same updates as `torch.optim.AdamW` (decoupled weight decay, bias-corrected moments, no amsgrad / maximize), `torch.optim.Adam`
(the same moments, L2 weight decay added to the gradient) and `torch.optim.SGD` (momentum, L2 weight decay, no dampening /
nesterov / maximize), which the reference builds by `train.optim.classname` and configures through Lightning
(model/pipeline.py:738-757, model/pointgroup.py:372-384); `torch.optim.AdamW(fused=True)` issues one multi-tensor launch per ~30
tensors (8 launches, 0.27 ms for the detector's ~300 tensors), these issue one.
A device table of (param, grad, state, state) pointers is kept per group.  Per step the host only collects the
gradient addresses (the native U-Net executor keeps its flat gradient buffer, the few head gradients are re-allocated by
`zero_grad(set_to_none=True)`); when any of them moved, the address column is refreshed through a pinned staging buffer
(one asynchronous 10 KB copy, no synchronisation).

The step count is PER PARAMETER, as in `torch.optim.AdamW` (bias correction `1 - beta^t` with t = the number of updates this
tensor has received): ScoreNet / `score_linear` only start receiving gradients once proposals exist
(`epoch > prepare_epochs`, model/pointgroup.py:332) and must then start at t = 1, not at the backbone's t.  The tensors of a
table are ordered by their step count, so tensors with equal counts ("cohorts") own a contiguous range of the block map and
get one launch with their own bias corrections -- one launch in the steady state.  `state_dict()` carries
`state[p]["step"]`, so checkpoints move to and from `torch.optim.AdamW` / `torch.optim.Adam` in both directions.

SGD keeps no step count: its cohorts are "owns a momentum buffer" and "first update" (`buf = g'`, as the library clones the
gradient into the new buffer) -- two launches on the step where late tensors join, after which the two ranges are one cohort
again; without momentum there is no buffer, no state and one cohort.

Gradient clipping (`max_grad_norm=`; None: off, and the step calls exactly what it called before the option existed).  What
`torch.nn.utils.clip_grad_norm_` -- Lightning's `Trainer(gradient_clip_val=...)` for the reference -- does in front of the step
happens inside it: one `d3_grad_sumsq` launch per group over the group's table, one `d3_grad_clip_finish` launch that leaves
(norm, coef, skip, nskipped) in a 32-byte device record, and the `_clipped` update entries, which use `g * coef`.  The norm is
global over all groups, over the tensors that have a gradient this step (after the `drop_stale_grads` pre-hook), accumulated in
double in a fixed order; `math.inf` measures without clipping.  Differences from torch, both deliberate:
* `p.grad` is NOT rewritten: it keeps its unclipped value after `step()` (the write pass is what the native path saves);
* `skip_nonfinite=True` (default): when the norm is inf or NaN the update kernels store nothing -- parameters and every state
  tensor stay bit-unchanged -- and no value is read back to the host.  THE PER-PARAMETER STEP COUNTS STILL ADVANCE on such a
  step (they live on the host): the next finite step is `torch.optim`'s update with `state[p]["step"]` one higher, and an SGD
  tensor whose first update was skipped owns a zero momentum buffer, which gives the first-update rule anyway.
  `skip_nonfinite=False` lets the NaN propagate as it does through torch.
Neither option is a `param_groups` entry or part of `state_dict()`: checkpoints interchange with `torch.optim.*` as before.
With several ranks the gradients are identical after the all-reduce, so each rank's norm is the global one: no collective."""
import math
import operator

import numpy as np
import torch

from . import _lib
from ._call import call, on, stream


_DATA_PTR = operator.methodcaller("data_ptr")
_GRAD = operator.attrgetter("grad")


class _FusedTable(torch.optim.Optimizer):
    """The table machinery the three optimizers share: the pointer table and block map of a group (`_build`), its reuse and the
    refresh of moved gradient addresses through a ring of pinned buffers (`_table`), cohort ordering, `_flush_steps`.
    A subclass names its state tensors (`_slots`: table columns 2..), the cohort a tensor belongs to (`_key`) and launches.

    `max_grad_norm` (None: off; a positive float or math.inf) and `skip_nonfinite` are attributes, not `param_groups` entries
    and not in `state_dict()`.  With `max_grad_norm` set, `_measure` puts the global gradient norm, the clipping coefficient
    and the skip flag into a device record that the `_clipped` update entries read; `p.grad` keeps its unclipped value.
    A step skipped for a non-finite norm leaves parameters and state tensors bit-unchanged BUT STILL ADVANCES THE
    PER-PARAMETER STEP COUNTS: they live on the host and nothing is read back.  The next finite step is therefore
    `torch.optim`'s update with `state[p]["step"]` one higher."""

    RING = 4   # pinned staging slots per group: an address refresh never rewrites a buffer whose copy may still be queued

    def __init__(self, params, defaults, max_grad_norm=None, skip_nonfinite=True):
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError("%s: max_grad_norm is None (off), a positive float or math.inf" % type(self).__name__)
        super().__init__(params, defaults)
        self._tables = {}
        # attributes, not param_groups entries: state_dict() stays the torch.optim layout
        self.max_grad_norm = max_grad_norm
        self.skip_nonfinite = skip_nonfinite
        self._ctl = self._partials = None

    def __getstate__(self):
        return dict(super().__getstate__(), max_grad_norm=self.max_grad_norm, skip_nonfinite=self.skip_nonfinite)

    def _record(self):
        """the d3_clip_ctl record (include/d3hip.h) as 8 int32 words on the parameters' device; `enforce` follows `skip_nonfinite`"""
        enforce = int(bool(self.skip_nonfinite))
        if self._ctl is None:
            dev = self.param_groups[0]["params"][0].device
            self._ctl = torch.tensor([0, 0, 0, 0, enforce, 0, 0, 0], dtype=torch.int32, device=dev)
            self._enforce = enforce
        elif self._enforce != enforce:
            self._ctl[4] = enforce
            self._enforce = enforce
        return self._ctl

    def last_grad_norm(self):
        """0-d float32 device tensor ALIASING the record's `norm`: the total gradient 2-norm the last clipped step()
        measured, before clipping (0 before the first).  No synchronisation; every step() rewrites it in place."""
        return self._record()[0:1].view(torch.float32).reshape(())

    def nonfinite_steps(self):
        """number of steps whose gradient norm was not finite, over the optimizer's life (one small read-back)"""
        return 0 if self._ctl is None else int(self._ctl[3].item())

    def _resolve(self):
        """every group's table, after the step pre-hooks: [(group, table)] of the groups that have gradients"""
        tables = [(group, self._table(gi, group)) for gi, group in enumerate(self.param_groups)]
        return [(group, tb) for group, tb in tables if tb["nblocks"]]

    def _measure(self, tables):
        """torch.nn.utils.clip_grad_norm_ over every tensor of `tables`: one d3_grad_sumsq per group into one partials
        buffer, one d3_grad_clip_finish; -> the record's address for the _clipped entries (None: clipping is off)"""
        if self.max_grad_norm is None or not tables:
            return None
        ctl = self._record()
        dev = ctl.device
        total = sum(tb["nblocks"] for _g, tb in tables)
        if self._partials is None or self._partials.numel() < total:
            self._partials = torch.empty(total, dtype=torch.float64, device=dev)
        with on(dev):
            st = stream()
            o = 0
            for _g, tb in tables:
                if tb["device"] != dev:
                    raise RuntimeError("%s: max_grad_norm needs every group on one device" % type(self).__name__)
                call("grad_sumsq", tb["ptrs"].data_ptr(), tb["numel"].data_ptr(), tb["blocks"].data_ptr(), tb["nblocks"],
                     self._partials.data_ptr() + 8 * o, st)
                o += tb["nblocks"]
            call("grad_clip_finish", self._partials.data_ptr(), total, float(self.max_grad_norm), ctl.data_ptr(), st)
        return ctl.data_ptr()

    def _slots(self, group):
        """names of the per-parameter state tensors whose addresses fill table columns 2.."""
        raise NotImplementedError

    def _key(self, p, slots):
        """cohort of a tensor (an int; larger first): tensors with equal keys share a launch"""
        raise NotImplementedError

    def _flush_steps(self):
        """cohort step counters of the cached tables -> state[p]["step"] (python ints)"""

    def __setstate__(self, state):
        super().__setstate__(state)
        self._tables = {}
        self.__dict__.setdefault("max_grad_norm", None)
        self.__dict__.setdefault("skip_nonfinite", True)
        self._ctl = self._partials = None

    @classmethod
    def _validate(cls, p):
        g = p.grad
        if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and g.is_contiguous()
                and g.dtype == torch.float32 and not g.is_sparse and g.device == p.device):
            raise RuntimeError("%s: contiguous fp32 device parameters and gradients only" % cls.__name__)

    def _build(self, gi, group, plist):
        for p in plist:
            self._validate(p)
        slots = self._slots(group)
        key = {p: self._key(p, slots) for p in plist}
        # equal step counts adjacent (most-stepped first; stable): one contiguous block-map range, one launch per cohort
        plist.sort(key=lambda p: -key[p])
        dev = plist[0].device
        fresh = [p for p in plist if slots and self.state[p].get(slots[0]) is None]
        if fresh:   # moments of the tensors seen for the first time: one flat buffer
            flat = torch.zeros(len(slots) * sum(p.numel() for p in fresh), dtype=torch.float32, device=dev)
            o = 0
            for p in fresh:
                n = p.numel()
                for s in slots:
                    self.state[p][s] = flat[o:o + n].view_as(p)
                    o += n
        chunk = _lib.lib().d3_adamw_chunk()
        ring = [torch.empty((len(plist), 4), dtype=torch.int64).pin_memory() for _ in range(self.RING)]
        host = ring[0]
        hv = host.numpy()
        hv[:, 0] = [p.data_ptr() for p in plist]
        hv[:, 1] = [p.grad.data_ptr() for p in plist]
        hv[:, 2:] = 0
        for k, s in enumerate(slots):
            hv[:, 2 + k] = [self.state[p][s].data_ptr() for p in plist]
        numel = np.array([p.numel() for p in plist], dtype=np.int32)
        blocks = np.array([(t, c) for t, n in enumerate(numel) for c in range((int(n) + chunk - 1) // chunk)], dtype=np.int32)
        nblk = [(int(n) + chunk - 1) // chunk for n in numel]
        cohorts, lo, b0 = [], 0, 0      # [step count, first tensor, end tensor, first block, blocks]
        for i in range(1, len(plist) + 1):
            if i == len(plist) or key[plist[i]] != key[plist[lo]]:
                nb = sum(nblk[lo:i])
                cohorts.append([key[plist[lo]], lo, i, b0, nb])
                lo, b0 = i, b0 + nb
        tb = {"pptr": [p.data_ptr() for p in plist], "gptr": hv[:, 1].tolist(), "host": host, "ring": ring, "slot": 0, "cohorts": cohorts,
              "slots": slots, "nblocks": int(blocks.shape[0]), "ptrs": host.to(dev), "numel": torch.from_numpy(numel).to(dev),
              "blocks": torch.from_numpy(blocks.reshape(-1)).to(dev), "device": dev}
        self._tables[gi] = tb
        return tb

    def _table(self, gi, group):
        tb = self._tables.get(gi)
        params = group["params"]
        if tb is not None and len(tb["plist"]) <= len(params):
            plist = tb["plist"]
            try:
                gptr = list(map(_DATA_PTR, map(_GRAD, plist)))
            except AttributeError:          # a gradient went missing: rebuild over the tensors that have one
                gptr = None
            if gptr is not None and tb["ngrad"] == sum(1 for p in params if p.grad is not None) \
                    and tb["pptr"] == list(map(_DATA_PTR, plist)):
                if gptr != tb["gptr"]:   # some gradients were re-allocated: refresh their addresses (asynchronous, stream ordered)
                    for i, (a, b) in enumerate(zip(gptr, tb["gptr"])):
                        if a != b:
                            self._validate(plist[i])
                    # next pinned slot of the ring: the previous refresh's host->device copy may still be in flight
                    tb["slot"] = (tb["slot"] + 1) % self.RING
                    nxt = tb["ring"][tb["slot"]]
                    nxt.copy_(tb["host"]); tb["host"] = nxt
                    tb["host"].numpy()[:, 1] = gptr
                    tb["ptrs"].copy_(tb["host"], non_blocking=True)
                    tb["gptr"] = gptr
                return tb
        plist = [p for p in params if p.grad is not None]
        if not plist:
            return {"nblocks": 0, "plist": [], "ngrad": -1}
        self._flush_steps()            # the table being replaced owns the current counts
        self._tables.pop(gi, None)
        tb = self._build(gi, group, plist)
        tb["plist"] = plist
        tb["ngrad"] = len(plist)
        return tb


def _refuse(cls, unsupported):
    if unsupported:
        raise ValueError("%s: %s not supported (the single-launch kernels implement the library's defaults only)"
                         % (cls.__name__, ", ".join(sorted(unsupported))))


class _FusedMoments(_FusedTable):
    """Adam-family state: exp_avg, exp_avg_sq and a per-parameter step count; `_ENTRY` is the library call of the rule."""
    _ENTRY = None

    def _slots(self, group):
        return ("exp_avg", "exp_avg_sq")

    def _key(self, p, slots):
        return int(self.state[p].get("step", 0))

    def _flush_steps(self):
        for tb in self._tables.values():
            for t, lo, hi, _b0, _nb in tb.get("cohorts", ()):
                for p in tb["plist"][lo:hi]:
                    self.state[p]["step"] = t

    def state_dict(self):
        """torch.optim.AdamW's layout: per-parameter `step` (a float32 scalar tensor), `exp_avg`, `exp_avg_sq`.  The returned
        per-parameter dicts are COPIES: `Optimizer.state_dict()` hands out the live `self.state[p]` objects, and this class keeps
        python-int step counts there (converting in place also rewrote the dict already returned)."""
        self._flush_steps()
        sd = super().state_dict()
        sd["state"] = {k: (dict(st, step=torch.tensor(float(st["step"]))) if "step" in st and not torch.is_tensor(st["step"]) else dict(st))
                       for k, st in sd["state"].items()}
        return sd

    def load_state_dict(self, state_dict):
        """moments are replaced: the cached device tables (which hold their addresses) are dropped; the step counts come from
        the checkpoint: torch.optim.AdamW's per-parameter `state[p]["step"]`, or -- checkpoints written by the first
        version of this class -- one per-group `step` applied to every tensor that has moments"""
        super().load_state_dict(state_dict)
        self._tables = {}
        for group in self.param_groups:
            legacy = group.pop("step", None)
            for p in group["params"]:
                st = self.state.get(p)
                if st is None or "exp_avg" not in st:
                    continue
                if "step" in st:
                    st["step"] = int(st["step"])
                elif legacy is not None:
                    st["step"] = int(legacy)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        tables = self._resolve()
        ctl = self._measure(tables)
        name = self._ENTRY if ctl is None else self._ENTRY + "_clipped"
        tail = () if ctl is None else (ctl,)
        for group, tb in tables:
            b1, b2 = group["betas"]
            with on(tb["device"]):
                st = stream()
                for co in tb["cohorts"]:       # tensors with the same number of updates behind them: one launch
                    co[0] = t = co[0] + 1      # also on a step the record makes the kernels skip: nothing is read back
                    call(name, tb["ptrs"].data_ptr(), tb["numel"].data_ptr(), tb["blocks"].data_ptr() + 8 * co[3], co[4],
                         float(group["lr"]), float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]),
                         1.0 - b1 ** t, math.sqrt(1.0 - b2 ** t), *tail, st)
        return loss


class FusedAdamW(_FusedMoments):
    _ENTRY = "adamw"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=None, skip_nonfinite=True):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay), max_grad_norm, skip_nonfinite)


class FusedAdam(_FusedMoments):
    """torch.optim.Adam (amsgrad = maximize = False) in one launch: FusedAdamW's state and step counts, L2 weight decay
    (`g + weight_decay * p` enters both moments) instead of the decoupled one.  Checkpoints interchange with torch.optim.Adam."""
    _ENTRY = "adam"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, max_grad_norm=None, skip_nonfinite=True,
                 **unsupported):
        _refuse(type(self), unsupported)      # amsgrad, maximize, ...: refused whatever their value
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay), max_grad_norm, skip_nonfinite)

    def load_state_dict(self, state_dict):
        for g in state_dict["param_groups"]:
            _refuse(type(self), [k for k in ("amsgrad", "maximize", "decoupled_weight_decay") if g.get(k)])
        super().load_state_dict(state_dict)


class FusedSGD(_FusedTable):
    """torch.optim.SGD (dampening = 0, nesterov = maximize = False) in one launch.  State is `momentum_buffer` alone, as in the
    library (none at all with momentum 0); a tensor without a buffer -- new, or loaded as `momentum_buffer: None` -- receives
    the first-update rule `buf = g + weight_decay * p`.  Checkpoints interchange with torch.optim.SGD."""

    def __init__(self, params, lr=1e-3, momentum=0, weight_decay=0, max_grad_norm=None, skip_nonfinite=True, **unsupported):
        _refuse(type(self), unsupported)      # dampening, nesterov, maximize, amsgrad, ...: refused whatever their value
        if lr < 0.0 or momentum < 0.0 or weight_decay < 0.0:
            raise ValueError("FusedSGD: negative lr, momentum or weight_decay")
        # the three constants are what torch.optim.SGD expects to find in a checkpoint's param_groups
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=0, weight_decay=weight_decay, nesterov=False,
                                      maximize=False), max_grad_norm, skip_nonfinite)

    def _slots(self, group):
        return ("momentum_buffer",) if group["momentum"] != 0 else ()

    def _key(self, p, slots):
        return 0 if slots and self.state[p].get(slots[0]) is None else 1     # 0: first update still to come

    def load_state_dict(self, state_dict):
        """buffers are replaced: the cached device tables are dropped"""
        for g in state_dict["param_groups"]:
            _refuse(type(self), [k for k in ("dampening", "nesterov", "maximize") if g.get(k)])
        super().load_state_dict(state_dict)
        self._tables = {}

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for gi, group in enumerate(self.param_groups):
            tb = self._tables.get(gi)
            if tb is not None and tb["slots"] != self._slots(group):      # momentum switched on or off: other table columns
                del self._tables[gi]
        tables = self._resolve()
        ctl = self._measure(tables)
        name, tail = ("sgd", ()) if ctl is None else ("sgd_clipped", (ctl,))
        for group, tb in tables:
            with on(tb["device"]):
                st = stream()
                for co in tb["cohorts"]:       # buffer owners, then the tensors updated for the first time
                    call(name, tb["ptrs"].data_ptr(), tb["numel"].data_ptr(), tb["blocks"].data_ptr() + 8 * co[3], co[4],
                         float(group["lr"]), float(group["momentum"]), float(group["weight_decay"]), int(co[0] == 0), *tail, st)
            if len(tb["cohorts"]) > 1 or tb["cohorts"][0][0] == 0:      # every tensor owns a buffer now: one cohort, one launch
                tb["cohorts"] = [[1, 0, len(tb["plist"]), 0, tb["nblocks"]]]
        return loss


_FUSED = {"Adam": FusedAdam, "AdamW": FusedAdamW, "SGD": FusedSGD}


def from_config(optim_cfg, params, keys, drop_stale_grads):
    """The optimizer `train.optim.classname` names (AdamW when the key is absent), as the reference builds it by name
    (model/pipeline.py:741-748, model/pointgroup.py:375-382).  keys: {classname: the `train.optim` keys that class receives}.
    Device parameters get the single-launch class, with `drop_stale_grads` as a step pre-hook (the executors' flat gradient
    buffers outlive zero_grad()); host parameters get the torch.optim class of that name.
    `train.optim.max_grad_norm` (absent, None or 0: off) is what Lightning's `Trainer(gradient_clip_val=...)` is to the reference:
    the global 2-norm of all gradients is clipped to it -- inside the single-launch step on the device (with
    `train.optim.skip_nonfinite`, default true: a step whose norm is not finite is dropped), by a step pre-hook calling
    `torch.nn.utils.clip_grad_norm_` on the host."""
    name = optim_cfg.get("classname", "AdamW")
    if name not in keys:
        raise ValueError("train.optim.classname: %r is not one of %s" % (name, ", ".join(sorted(keys))))
    kw = {k: optim_cfg[k] for k in keys[name]}
    clip = optim_cfg.get("max_grad_norm") or None
    if params[0].is_cuda:   # one launch for all tensors (csrc/heads.hip, csrc/optim.hip); same update rule
        if clip is not None:
            kw.update(max_grad_norm=float(clip), skip_nonfinite=bool(optim_cfg.get("skip_nonfinite", True)))
        opt = _FUSED[name](params, **kw)
        opt.register_step_pre_hook(lambda *a: drop_stale_grads())
    else:
        opt = getattr(torch.optim, name)(params, **kw)
        if clip is not None:
            def clip_hook(*_a):     # a step pre-hook returns None (or new arguments), never the norm
                torch.nn.utils.clip_grad_norm_(params, float(clip))
            opt.register_step_pre_hook(clip_hook)
    return opt
