"""Streaming enhance: push audio as it arrives, get finished samples back
(longform.py has the definition and the host arithmetic,
csrc/ou_stream.hip the two kernels).

:class:`ModelStream` is what ``Universe.stream`` returns: the session on the
``(batch, window)`` plan ``enhance()`` would record, driving ou_stream_gather
and ou_stream_overlap_add through ctypes the way ``enhance_long`` drives its
kernels.  ``bundle.Bundle.stream`` returns the same interface on the C session
(ou_model_stream_*).  Both compute the same stream: ``enhance_long`` of
everything pushed, the noise a function of position in the native stream
(ou_randn) at ``(seed, offset + k 2^38)`` for draw ``k``.
"""
import ctypes

import torch

from . import _lib as L
from . import longform


def as_samples(x, dev):
    """A push's samples as a contiguous float32 vector on ``dev``."""
    x = torch.as_tensor(x)
    if x.ndim != 1 and x.numel() != x.shape[-1]:
        raise ValueError("a stream is one mono signal: push (n,), (1, n) or (1, 1, n)")
    return x.reshape(-1).to(device=dev, dtype=torch.float32).contiguous()


class ModelStream:
    """One stream through a model: ``push(x) -> Tensor`` (the samples that
    became final, on the device, possibly none), ``close() -> Tensor`` (the
    rest, up to the stream's length), ``bound(n)`` (how many ``push`` of ``n``
    samples would return: host arithmetic, no synchronisation).  A context
    manager; leaving it releases the ring and the carry.

    Device memory is the ring (``window + batch * hop`` floats), the carry
    (``overlap``) and the cached fade table, whatever the stream's length.

    The plan is fetched through the model's plan LRU for every group, so its
    eviction between two pushes is harmless.  Its status is checked after each
    group's replay, before that group's samples are crossfaded and returned.
    On a split-f16 range error the model widens the named layers' exponents
    (``_range_recover``) and reruns *that group only*: its input is still in
    the ring and its noise is a function of position.  Samples already
    returned stay as they were -- unlike ``enhance_long``, which reruns the
    whole clip, a stream cannot take back what it emitted."""

    def __init__(self, model, window, overlap, batch=1, n_steps=None, epsilon=None, keep_rms=False, seed=0,
                 offset=0):
        self.model = model
        self.n_steps = int(model.diff_kwargs.n_steps if n_steps is None else n_steps)
        self.epsilon = float(model.diff_kwargs.epsilon if epsilon is None else epsilon)
        self.keep_rms = bool(keep_rms)
        W = int(window)
        self.counts = longform.StreamCounts(W, overlap, batch, W + model.tot_ds - W % model.tot_ds)
        self.seed, self.offset = int(seed), int(offset)
        if not 0 <= self.seed < 2**64 or not 0 <= self.offset < 2**64:
            raise ValueError("seed and offset are unsigned 64-bit integers")
        eng = model._get_engine()
        self.dev = eng.device
        if self.dev.type != "cuda":
            raise L.OuHipError("Universe.stream needs the model on a HIP device")
        c = self.counts
        self.ring = torch.empty(c.cap, dtype=torch.float32, device=self.dev)
        self.carry = torch.empty(max(c.O, 1), dtype=torch.float32, device=self.dev)
        self.fade = model._fade_table(c.O, self.dev)
        self.fed = 0            # samples in the ring so far (the counts run ahead while a push lists its steps)
        self.failed = None
        self.lib = L.load()

    # ---- the plan enhance() would run for a (batch, window) input
    def _plan(self):
        c = self.counts
        key, make_plan = self.model._plan_spec(c.B, c.W, self.n_steps, self.epsilon, self.keep_rms)
        plan = self.model._arena_plan(key, 0, make_plan)
        if plan.n_noise != self.n_steps or plan.Tp != c.Tp:
            raise L.OuHipError(f"stream: the plan draws {plan.n_noise} x {plan.Tp}, expected {self.n_steps} x {c.Tp}")
        return plan

    def _feed(self, x):
        cap, at = self.counts.cap, self.fed % self.counts.cap
        head = min(x.numel(), cap - at)
        self.ring[at:at + head].copy_(x[:head])
        if head < x.numel():
            self.ring[:x.numel() - head].copy_(x[head:])
        self.fed += x.numel()

    def _group(self, first, count, closing, out):
        """Windows [first, first + count): gather, replay, status, overlap-add
        into ``out``; returns the number of samples written."""
        c, lib = self.counts, self.lib
        stream = torch.cuda.current_stream(self.dev).cuda_stream
        sp = ctypes.c_void_p(stream)
        closing, T = int(bool(closing)), self.fed if closing else 0
        w_ptr = 0

        def replay():
            plan = self._plan()
            L.check(lib.ou_stream_gather(self.ring.data_ptr(), c.cap, max(0, self.fed - c.cap), self.fed, c.W, c.O,
                                         first, count, c.B, closing, T, plan.n_noise, plan.Tp, self.seed,
                                         self.offset, plan.MIX.data_ptr(), c.W, plan.NZ.data_ptr(), c.B * plan.Tp,
                                         plan.Tp, sp), "stream_gather")
            plan._launch(stream, True)
            plan.check(pinned=True)
            return plan.OUT.data_ptr()

        if count > 0:
            try:
                w_ptr = replay()
            except L.OuRangeError as e:
                w_ptr = self.model._range_recover(e, replay)   # this group only: ring and noise are still there
        got = ctypes.c_int64(0)
        L.check(lib.ou_stream_overlap_add(w_ptr, c.W, c.W, c.O, first, count, closing, T,
                                          self.fade.data_ptr() if self.fade is not None else 0,
                                          self.carry.data_ptr() if c.O else 0, out.data_ptr() if out.numel() else 0,
                                          ctypes.byref(got), sp), "stream_overlap_add")
        return int(got.value)

    def _usable(self):
        if self.failed is not None:
            raise L.OuHipError(f"stream: the session failed earlier ({self.failed})")
        if self.ring is None:
            raise L.OuHipError("stream: the session was released")

    def _run(self, steps, x, n_out):
        out = torch.empty(n_out, dtype=torch.float32, device=self.dev)
        pos = at = 0
        try:
            with torch.no_grad(), torch.cuda.device(self.dev):
                for step in steps:
                    if step[0] == "feed":
                        self._feed(x[at:at + step[1]])
                        at += step[1]
                    else:
                        pos += self._group(step[1], step[2], step[3], out[pos:])
        except Exception as e:
            # the counts have run ahead of the device: nothing more is emitted
            self.failed = f"{type(e).__name__}: {e}"
            raise
        assert pos == n_out, (pos, n_out)
        return out

    def bound(self, n=0, closing=False):
        return self.counts.bound(int(n), closing)

    def push(self, x):
        self._usable()
        x = as_samples(x, self.dev)
        n_out = self.counts.bound(x.numel())
        return self._run(self.counts.push(x.numel()), x, n_out)

    def close(self):
        self._usable()
        n_out = self.counts.bound(0, closing=True)   # raises longform.StreamShort below one window
        return self._run(self.counts.close(), None, n_out)

    def release(self):
        self.ring = self.carry = self.fade = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.release()
        return False
