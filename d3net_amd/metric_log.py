"""`MetricLog`: running per-key records of the scalars the hooks log, kept on the device (csrc/metric_log.hip).

The reference hands every logged value to Lightning (`self.log(..., on_epoch=True, sync_dist=True)`, model/pipeline.py:149,182,
...), which keeps a running mean per key and all-reduces each key separately.  `PipelineNet.log` keeps the latest value of a key in
`model.logged`; a `MetricLog` consumes that dict after each hook:

* `update(logged, weight=1.0)`: ONE `d3_metric_accumulate` launch folds every device scalar of the step into its slot's record
  (`sum` = sum of w * v in float64, `wsum`, `last`, `count`, `nonfinite`); nothing is read back.  The logged tensors are new
  allocations every step, so the table's address column is rewritten every step through pinned staging buffers (one asynchronous
  copy of 24 bytes per key, no synchronisation; a staging buffer is reused only after its copy's event has completed, otherwise the
  ring grows -- the host may run any number of steps ahead of the device).  The tensors are held until the next `update`.
  Python numbers and host tensors are accumulated on the host in the same arithmetic: float64, one multiplication and one
  addition per call.  Device tensors of another type than float32 / float64 / int32 / int64 are widened to float64 first.
* `compute()` -> {name: sum / wsum} as Python floats after ONE read-back of the record block; `last()`, `counts()`,
  `nonfinite()` read the other fields; `reset()` clears the records (`d3_metric_reset`) and keeps the slots.
* `snapshot()`: enqueues an asynchronous copy of the records to a pinned buffer with an event (the pattern of
  `pipeline._HostScalars`) and returns the means of the newest earlier snapshot whose copy has completed, or None.  Never waits.
* `all_reduce()`: one packed collective over every key's (sum, wsum) -- the reference issues one per key, `reduce_logged` needs
  one host read per key -- after which `compute()` is the global mean.  Every rank must have logged the same keys.

Slots are keyed by name in first-seen order; `capacity` (default and maximum `d3_metric_capacity()` = 1024 keys) bounds them and
the library refuses a larger count (`D3Error`, D3_ERR_RANGE) instead of truncating.  Several logs can share one record buffer
(`records=`, `offset=`): the trainer keeps its training and validation tables in one."""
import numpy as np
import torch

from . import _lib
from ._call import call, on, stream
from ._lib import check

_CODES = {torch.float32: 0, torch.float64: 1, torch.int32: 2, torch.int64: 3}   # D3_METRIC_* (include/d3hip.h)
CAPACITY = 1024  # = d3_metric_capacity(): keys per log
_FIELDS = 5      # d3_metric_rec: sum, wsum, last (float64), count, nonfinite (int64)
_SUM, _WSUM, _LAST, _COUNT, _NONFINITE = range(_FIELDS)


def _as_host(rec):
    """(n, 5) float64 block whose columns 3 and 4 carry int64 bits -> (float64 (n, 3), int64 (n, 2))"""
    return rec[:, :3], rec[:, 3:].view(np.int64)


class MetricLog:
    SNAPSHOTS = 2     # pinned snapshot buffers: at most this many copies in flight, a further snapshot() call enqueues none

    def __init__(self, device=None, capacity=None, records=None, offset=0):
        """device: where the logged device scalars live (None: taken from the first one seen; a log that only ever sees host
        values needs neither a device nor the library).  records / offset: a float64 (N, 5) device buffer shared with other logs
        and this log's first slot in it (`MetricLog.allocate`)."""
        self.device = torch.device(device) if device is not None else (records.device if records is not None else None)
        if self.device is not None and self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.capacity = CAPACITY if capacity is None else int(capacity)
        if not 0 < self.capacity <= CAPACITY:
            raise ValueError("MetricLog: capacity is 1 .. %d keys" % CAPACITY)
        self._names, self._slot = [], {}
        self._records, self._offset = records, int(offset)
        self._host = np.zeros((0, _FIELDS), np.float64)          # the host arm's records, same layout
        self._host_newer = []                                    # per slot: the host arm saw the key after the device arm
        self._table = None
        self._ring, self._held = [], ()
        self._snaps, self._snap_free = [], None
        self._gen, self.snapshot_tag = 0, None       # snapshots taken before the last reset() are never handed out

    # ------------------------------------------------------------------------------------------------- storage
    @staticmethod
    def allocate(device, slots):
        """a zeroed record buffer for `slots` slots on `device` (40 bytes each)"""
        return torch.zeros((int(slots), _FIELDS), dtype=torch.float64, device=device)

    def _device_state(self, dev):
        if self.device is None:
            self.device = dev
        elif dev != self.device:
            raise ValueError("MetricLog: a logged tensor lives on %s, the log on %s" % (dev, self.device))
        if self._table is None:
            cap = self.capacity
            assert _lib.lib().d3_metric_capacity() == CAPACITY
            if self._records is None:
                self._records, self._offset = self.allocate(dev, cap), 0
            elif self._records.shape[0] < self._offset + cap or self._records.dtype != torch.float64 or self._records.device != dev:
                raise ValueError("MetricLog: the shared record buffer is a float64 (N, 5) tensor on %s with N >= offset + capacity" % dev)
            self._table = torch.zeros((cap, 3), dtype=torch.int64, device=dev)

    def _slot_of(self, name):
        i = self._slot.get(name)
        if i is None:
            i = self._slot[name] = len(self._names)
            self._names.append(name)
            self._host_newer.append(False)
            if i >= self._host.shape[0]:
                self._host = np.concatenate([self._host, np.zeros((max(16, i), _FIELDS), np.float64)])
        return i

    def _staging(self):
        """a pinned (capacity, 3) int64 buffer no queued copy still reads: the first of the ring whose event has completed, else a
        new one -- never a wait"""
        for slot in self._ring:
            if slot[1].query():
                return slot
        slot = [torch.zeros((self.capacity, 3), dtype=torch.int64).pin_memory(), torch.cuda.Event()]
        self._ring.append(slot)
        return slot

    # ------------------------------------------------------------------------------------------------- accumulation
    def update(self, logged, weight=1.0):
        """fold the values of `logged` ({name: 0-d tensor or number}, what `PipelineNet.log` fills) into their records with
        `weight`; keys absent from `logged` keep their records bit-unchanged"""
        w = float(weight)
        rows, held = [], []
        for name, v in logged.items():
            i = self._slot_of(name)
            if torch.is_tensor(v) and v.is_cuda:
                if v.numel() != 1:
                    raise ValueError("MetricLog: %r is not a scalar (shape %s)" % (name, tuple(v.shape)))
                v = v.detach()
                if v.dtype not in _CODES:
                    v = v.double()                      # (bool, half, ...: one small conversion launch, no read-back)
                rows.append((i, v.data_ptr(), _CODES[v.dtype]))
                held.append(v)
                self._host_newer[i] = False
            else:
                x = float(v)
                f, n = _as_host(self._host)
                f[i, _SUM] = f[i, _SUM] + w * x
                f[i, _WSUM] = f[i, _WSUM] + w
                f[i, _LAST] = x
                n[i, 0] += 1
                n[i, 1] += 0 if np.isfinite(x) else 1
                self._host_newer[i] = True
        n = len(self._names)
        if n > self.capacity:      # the library's answer to such a launch: refused, never truncated
            check(-2, "metric_accumulate (%d keys, capacity %d)" % (n, self.capacity))
        if not rows:
            self._held = ()
            return
        self._device_state(held[0].device)
        for v in held:
            if v.device != self.device:
                raise ValueError("MetricLog: a logged tensor lives on %s, the log on %s" % (v.device, self.device))
        pin, ev = self._staging()
        hv = pin.numpy()
        hv[:n, 0] = 0
        hv[:n, 2].view(np.float64)[:] = w
        for i, ptr, code in rows:
            hv[i, 0] = ptr
            hv[i, 1] = code
        with on(self.device):
            self._table[:n].copy_(pin[:n], non_blocking=True)
            ev.record()
            call("metric_accumulate", self._table.data_ptr(), n, self._rec_ptr(), stream())
        self._held = held        # alive until the launch that reads them is behind the next update's

    def _rec_ptr(self):
        return self._records.data_ptr() + 8 * _FIELDS * self._offset

    def reset(self):
        """clear every record; the slots (names and their order) stay"""
        self._host[:] = 0
        self._host_newer = [False] * len(self._names)
        self._gen += 1
        if self._table is not None:
            with on(self.device):
                call("metric_reset", self._records.data_ptr(), self._offset, self.capacity, stream())

    # ------------------------------------------------------------------------------------------------- reading
    @staticmethod
    def _merge(host, newer, dev_rec):
        """the records of both arms as (float64 (n, 3), int64 (n, 2)); host: the host arm's block, dev_rec: the device block
        read back (None: the log has no device arm), newer: per slot, whether the host arm saw the key last"""
        f, c = (a.copy() for a in _as_host(host))
        if dev_rec is not None and len(newer):
            df, dc = _as_host(dev_rec)
            f[:, :2] = df[:, :2] + f[:, :2]
            for i, host_last in enumerate(newer):
                if dc[i, 0] and not host_last:
                    f[i, _LAST] = df[i, _LAST]
            c = c + dc
        return f, c

    def _merged(self):
        n = len(self._names)
        dev_rec = None
        if self._table is not None and n:
            dev_rec = self._records[self._offset:self._offset + n].cpu().numpy()      # the one read-back
        return self._merge(self._host[:n], self._host_newer[:n], dev_rec)

    @staticmethod
    def _means(names, f, c):
        with np.errstate(all="ignore"):
            return {k: float(np.float64(f[i, _SUM]) / np.float64(f[i, _WSUM])) for i, k in enumerate(names) if c[i, 0]}

    def compute(self):
        """{name: sum / wsum} over the keys that received a value, as Python floats"""
        f, c = self._merged()
        return self._means(self._names, f, c)

    def last(self):
        f, c = self._merged()
        return {k: float(f[i, _LAST]) for i, k in enumerate(self._names) if c[i, 0]}

    def counts(self):
        _f, c = self._merged()
        return {k: int(c[i, 0]) for i, k in enumerate(self._names)}

    def nonfinite(self):
        """{name: how many of its values were inf or NaN} for the keys that had any"""
        _f, c = self._merged()
        return {k: int(c[i, 1]) for i, k in enumerate(self._names) if c[i, 1]}

    def snapshot(self, tag=None):
        """start copying the records to the host and return the means of the newest EARLIER snapshot that has arrived (None when
        there is none yet, or when a `reset()` came after it); `snapshot_tag` is then the `tag` that snapshot was taken with.
        Never waits: with every pinned buffer still in flight no new copy is enqueued."""
        done = None
        while self._snaps and (self._snaps[0][1] is None or self._snaps[0][1].query()):
            if done is not None and done[0] is not None:
                self._snap_free.append(done[0])
            done = self._snaps.pop(0)
        out = None
        if done is not None:
            pin, _ev, names, host, newer, gen, done_tag = done
            if gen == self._gen:
                f, c = self._merge(host, newer, None if pin is None else pin.numpy()[:len(names)])
                out, self.snapshot_tag = self._means(names, f, c), done_tag
            if pin is not None:
                self._snap_free.append(pin)
        n = len(self._names)
        state = (list(self._names), self._host[:n].copy(), list(self._host_newer), self._gen, tag)
        if self._table is None or not n:
            self._snaps.append((None, None) + state)
        else:
            if self._snap_free is None:
                self._snap_free = [torch.zeros((self.capacity, _FIELDS), dtype=torch.float64).pin_memory() for _ in range(self.SNAPSHOTS)]
            if self._snap_free:
                pin = self._snap_free.pop()
                with on(self.device):
                    pin[:n].copy_(self._records[self._offset:self._offset + n], non_blocking=True)
                    ev = torch.cuda.Event()
                    ev.record()
                self._snaps.append((pin, ev) + state)
        return out

    # ------------------------------------------------------------------------------------------------- ranks
    def all_reduce(self):
        """ONE packed all-reduce (sum) of every key's (sum, wsum), keys in name order; afterwards every rank's records hold the
        global sums and `compute()` is the global mean.  No process group, or a world of one: nothing to do."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
            return
        n = len(self._names)
        order = sorted(range(n), key=lambda i: self._names[i])
        f, _c = _as_host(self._host[:n])
        host = torch.from_numpy(np.concatenate([[float(n)], f[order, _SUM], f[order, _WSUM]]))
        if self._table is not None:
            idx = torch.tensor(order, dtype=torch.int64).to(self.device)
            rec = self._records[self._offset:self._offset + n]
            vec = host.to(self.device)
            vec[1:] += torch.cat([rec[idx, _SUM], rec[idx, _WSUM]])
        else:
            vec = host
        dist.all_reduce(vec)
        if self._table is not None:
            rec[idx, _SUM], rec[idx, _WSUM] = vec[1:1 + n], vec[1 + n:]
            f[:, _SUM] = 0; f[:, _WSUM] = 0
            keys = vec[0:1].cpu()
        else:
            out = vec.numpy()
            f[order, _SUM], f[order, _WSUM] = out[1:1 + n], out[1 + n:]
            keys = vec[0:1]
        if float(keys[0]) != float(n) * dist.get_world_size():
            raise RuntimeError("MetricLog.all_reduce: the ranks logged different numbers of keys (%d here)" % n)
