"""Multiplexed streams: many live streams share one batched plan (DESIGN.md
section 16; longform.py has the definition and the host arithmetic,
csrc/ou_mux.hip the two kernels).

:class:`ModelMux` is what ``Universe.stream_mux`` returns: ``channels``
section-15 streams, each with its own ring, carry and noise, whose ready
windows run together in the slots of the ``(batch, window)`` plan ``enhance()``
would record.  ``push`` only copies into a channel's ring; ``run`` pools
whatever windows are ready into groups of ``batch`` -- one ou_mux_gather, one
replay and one ou_mux_overlap_add per group -- and hands every channel the
samples that became final.  ``bundle.Bundle.stream_mux`` returns the same
interface on the C session (ou_model_mux_*).
"""
import ctypes

import torch

from . import _lib as L
from . import longform
from .stream import as_samples


def slot_table(group, state, cap):
    """The ou_mux_slot array of a group: ``state[c]`` is channel ``c``'s
    ``(fed, seed, offset)`` when the run began."""
    tab = (L.MuxSlot * len(group.slots))()
    for e, (c, _, start) in zip(tab, group.slots):
        fed, seed, offset = state[c]
        e.start, e.lo, e.fed, e.seed, e.offset, e.channel = start, max(0, fed - cap), fed, seed, offset, c
    return tab


def run_table(group):
    """The ou_mux_run array of a group."""
    tab = (L.MuxRun * len(group.runs))()
    for e, r in zip(tab, group.runs):
        e.first, e.T, e.out_off, e.count, e.closing, e.slot, e.channel = (r.first, r.T, r.out_off, r.count,
                                                                          r.closing, r.slot, r.channel)
    return tab


class ModelMux:
    """``channels`` streams through one model.  ``open(seed, offset) -> c``
    takes a free channel; ``push(c, x)`` feeds it (at most ``room(c)`` samples:
    a longer push is refused whole, call ``run()`` first); ``close(c)`` marks it
    closing -- it is free again once ``run()`` has emitted its last samples;
    ``run(full_only=False)`` returns one tensor per channel, the samples that
    became final (empty where none did), views of one buffer on the device;
    ``bound(full_only)`` gives their counts and offsets beforehand, host
    arithmetic alone.  A context manager; leaving it releases the buffers.

    Device memory is ``channels`` rings of ``window + batch * hop`` floats,
    ``channels`` carries of ``overlap`` and the cached fade table, whatever
    the streams' lengths.

    The plan comes through the model's plan LRU for every group, and its status
    is checked after each group's replay, before that group's samples are
    crossfaded.  On a split-f16 range error the named exponents widen and that
    group only reruns: rings and carries are untouched until the overlap-add.
    Any other failure fails the mux as a whole."""

    def __init__(self, model, window, overlap, channels, batch=8, n_steps=None, epsilon=None, keep_rms=False):
        self.model = model
        self.n_steps = int(model.diff_kwargs.n_steps if n_steps is None else n_steps)
        self.epsilon = float(model.diff_kwargs.epsilon if epsilon is None else epsilon)
        self.keep_rms = bool(keep_rms)
        W = int(window)
        self.counts = longform.MuxCounts(W, overlap, batch, channels, W + model.tot_ds - W % model.tot_ds)
        eng = model._get_engine()
        self.dev = eng.device
        if self.dev.type != "cuda":
            raise L.OuHipError("Universe.stream_mux needs the model on a HIP device")
        c = self.counts
        self.rings = torch.empty(c.C, c.cap, dtype=torch.float32, device=self.dev)
        self.carries = torch.empty(c.C, max(c.O, 1), dtype=torch.float32, device=self.dev)
        self.fade = model._fade_table(c.O, self.dev)
        self.failed = None
        self.lib = L.load()

    def _usable(self):
        if self.failed is not None:
            raise L.OuHipError(f"stream_mux: the session failed earlier ({self.failed})")
        if self.rings is None:
            raise L.OuHipError("stream_mux: the session was released")

    # ---- host arithmetic
    def open(self, seed=0, offset=0, channel=None):
        self._usable()
        return self.counts.open(seed, offset, channel)

    def room(self, c):
        return self.counts.room(c)

    def close(self, c):
        self._usable()
        self.counts.close(c)   # raises longform.StreamShort below one window; the channel stays open

    def bound(self, full_only=False):
        return self.counts.bound(full_only)

    # ---- a push only feeds the ring
    def push(self, c, x):
        self._usable()
        x = as_samples(x, self.dev)
        at = self.counts.push(c, x.numel()) % self.counts.cap
        ring = self.rings[int(c)]
        head = min(x.numel(), self.counts.cap - at)
        ring[at:at + head].copy_(x[:head])
        if head < x.numel():
            ring[:x.numel() - head].copy_(x[head:])

    # ---- the plan enhance() would run for a (batch, window) input
    def _plan(self):
        c = self.counts
        key, make_plan = self.model._plan_spec(c.B, c.W, self.n_steps, self.epsilon, self.keep_rms)
        plan = self.model._arena_plan(key, 0, make_plan)
        if plan.n_noise != self.n_steps or plan.Tp != c.Tp:
            raise L.OuHipError(f"stream_mux: the plan draws {plan.n_noise} x {plan.Tp}, expected {self.n_steps} x {c.Tp}")
        return plan

    def _group(self, group, state, out):
        c, lib = self.counts, self.lib
        stream = torch.cuda.current_stream(self.dev).cuda_stream
        sp = ctypes.c_void_p(stream)
        w_ptr = 0
        if group.slots:
            slots = slot_table(group, state, c.cap)

            def replay():
                plan = self._plan()
                L.check(lib.ou_mux_gather(self.rings.data_ptr(), c.cap, c.C, c.W, slots, len(slots), plan.n_noise,
                                          plan.Tp, plan.MIX.data_ptr(), c.W, plan.NZ.data_ptr(), c.B * plan.Tp,
                                          plan.Tp, sp), "mux_gather")
                plan._launch(stream, True)
                plan.check(pinned=True)
                return plan.OUT.data_ptr()

            try:
                w_ptr = replay()
            except L.OuRangeError as e:
                w_ptr = self.model._range_recover(e, replay)   # this group only: rings and noise are still there
        runs = run_table(group)
        L.check(lib.ou_mux_overlap_add(w_ptr, c.W, len(group.slots), c.W, c.O, runs, len(runs),
                                       self.fade.data_ptr() if self.fade is not None else 0,
                                       self.carries.data_ptr() if c.O else 0, self.carries.stride(0), c.C,
                                       out.data_ptr() if out.numel() else 0, out.numel(), None, sp),
                "mux_overlap_add")

    def run(self, full_only=False):
        self._usable()
        state = [(s.fed, s.seed, s.offset) for s in self.counts.ch]
        plan = self.counts.plan_run(full_only)
        out = torch.empty(sum(plan.counts), dtype=torch.float32, device=self.dev)
        try:
            with torch.no_grad(), torch.cuda.device(self.dev):
                for group in plan.groups:
                    self._group(group, state, out)
        except Exception as e:
            # the counts have run ahead of the device: nothing more is emitted
            self.failed = f"{type(e).__name__}: {e}"
            raise
        return [out[o:o + n] for o, n in zip(plan.offsets, plan.counts)]

    def release(self):
        self.rings = self.carries = self.fade = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.release()
        return False
