"""Windowed enhance of a long clip: the definition.

Pure Python and numpy; imports without a GPU.  ``Universe.enhance_long``, the
CLI, ``bundle.Bundle.enhance_long`` and the C host (csrc/ou_long.hip,
ou_model_enhance_long) all compute what this module states.

Symbols: ``W`` the window and ``O`` the overlap in samples at ``model.fs``,
``0 <= O <= W / 2``; ``H = W - O`` the hop; ``T`` the clip length.

Windows.  ``n = 1`` if ``T <= W`` else ``1 + ceil((T - W) / H)``;
``start_i = min(i H, T - W)`` -- the last window is shifted back to end at
``T``, nothing is zero-padded (per-item normalisation would see a quieter
window); ``e_i = start_i + W``.  An index ``i >= n`` means window ``n - 1``:
the unused batch slots of the last group repeat the last real window, whose
content is safe and whose outputs are dropped.

Seams.  Window ``i >= 1`` fades in over the global samples
``[e_{i-1} - O, e_{i-1})`` with weight ``f(u) = sin^2(pi (2 u + 1) / (4 O))``
at ``u = t - (e_{i-1} - O)``; window ``i - 1`` has ``1 - f(u)`` there.  Window
``i`` has weight 0 before its fade-in (the head of the shifted last window is
discarded), 0 outside its span and 1 elsewhere inside it; ``O = 0`` is a hard
switch at ``e_{i-1}``.  With ``O <= W / 2`` at most two windows are non-zero
at a sample, and the weights sum to 1 on ``[0, T)``.

Noise.  One global stream per sampler draw: draw ``k`` has the shape
``(1, 1, L)``, ``L = start_{n-1} + Tp`` with ``Tp`` the plan's padded window
length, drawn in the sampler's order (x0, then one z per intermediate step);
window ``i`` uses ``G[k, 0, start_i : start_i + Tp]``.  Two windows see the
same noise wherever they overlap, and the draws do not depend on how the
windows are grouped into batches.

Result.  ``y[t] = sum_i weight_i(t) out_i[t - start_i]`` with ``out_i`` what
``enhance()`` returns for window ``i`` inside its batch-``B`` group
(windows ``[g B, g B + B)``, ``B = min(batch, n)``) on its slice of the noise,
through the normal finish (crop, ``keep_rms`` against the window's own input
RMS, peak division).

Pooled windows (``Universe.enhance_long_many``, csrc/ou_pool.hip).  Clips
``c = 0 .. C - 1`` of lengths ``T_c > W`` have ``n_c`` windows each, with the
starts above.  The slot list is ``[(c, i) for c in order for i in
range(n_c)]``, ``N = sum n_c``; ``B = min(batch, N)`` and group ``g`` holds
the slots ``[g B, g B + B)``, a slot index ``>= N`` meaning slot ``N - 1`` (the
last window of the last clip, whose output is dropped).  The noise is per clip
and unchanged: clip ``c`` draws its ``n_noise`` tensors ``(1, 1, L_c)`` in
clip order -- the draws of consecutive ``enhance_long`` calls -- and window
``(c, i)`` uses ``G_c[k, 0, start_{c,i} : start_{c,i} + Tp]``.  The result is
``y_c[t] = sum_i weight_{c,i}(t) out_{c,i}[t - start_{c,i}]`` with the weights
above and ``out_{c,i}`` what ``enhance()`` returns for that window in its slot
of its group, evaluated per sample in float32 as ``(0 + w_{i-1} v_{i-1}) +
w_i v_i``, each product and sum rounded -- so ``y_c`` depends on the ``out``
values alone, not on where the group boundaries fall.  For one clip this is
``enhance_long`` itself: the same slots, the same replays, the same bits.

Streams (``Universe.stream``, ``bundle.Bundle.stream``, csrc/ou_stream.hip;
DESIGN.md section 15).  A stream is the windowed enhance of the concatenation
of everything pushed, ``B`` fixed.  With ``fed`` samples pushed, window ``i`` is
regular (``start_i = i H``) and ready once ``fed >= i H + W``; group ``g`` --
windows ``[g B, g B + B)`` -- runs when all of them are ready.  At close,
``T = fed``: the window list is the one above for ``T``, the windows that have
not run yet run as one last group (unused slots repeat window ``n - 1``), and
only window ``n - 1`` can be shifted, so every window that ran before close is
a regular window of the final list.  After windows ``[0, m)`` have run, the
samples ``[0, m H)`` are final and have been emitted; the last ``O`` samples of
window ``m - 1`` wait, raw, for their successor; close emits everything up to
``T``.  ``T < W`` at close is an error of its own (nothing has run).  The
noise is a function of position: sample ``t`` of draw ``k`` is element ``t`` of
the native stream (ou_randn) at ``(seed, offset + k 2^38)``, counters of four
samples, so a draw has ``2^40`` samples and a stream may not pass them; window
``i`` uses samples ``[start_i, start_i + Tp)`` of every draw, whatever ``T``,
the grouping or the cuts of the pushes are.  The input lives in a ring of
``W + B H`` samples, position ``p`` at ``p mod capacity``, which must retain
``[min(m H, fed - W), fed)``: the next window's samples, and the last ``W`` for
a shifted last window, which starts before ``m H``.  :class:`StreamCounts`
is that arithmetic.
"""
import collections

import numpy as np

DRAW_COUNTERS = 1 << 38         # Philox counters between two draws of a stream
STREAM_MAX_SAMPLES = 1 << 40    # samples of one draw


def check(T, W, O):
    """Validate (T, W, O); returns them as ints."""
    T, W, O = int(T), int(W), int(O)
    if W < 1:
        raise ValueError(f"window must be at least one sample, got {W}")
    if O < 0 or O > W // 2:
        raise ValueError(f"overlap must lie in [0, window / 2] = [0, {W // 2}], got {O}")
    if T < 1:
        raise ValueError(f"the clip has {T} samples")
    return T, W, O


def n_windows(T, W, O):
    T, W, O = check(T, W, O)
    if T <= W:
        return 1
    H = W - O
    return 1 + -(-(T - W) // H)


def start(i, T, W, O):
    """Start of window ``i``; ``i >= n`` clamps to the last window."""
    T, W, O = check(T, W, O)
    i = min(int(i), n_windows(T, W, O) - 1)
    return max(0, min(i * (W - O), T - W))


def starts(T, W, O):
    return [start(i, T, W, O) for i in range(n_windows(T, W, O))]


def noise_len(T, W, O, Tp):
    """``L``: the length of one global noise draw."""
    return start(n_windows(T, W, O) - 1, T, W, O) + int(Tp)


def groups(T, W, O, batch):
    """(B, [first window of each group]): ``B = min(batch, n)``."""
    n = n_windows(T, W, O)
    B = max(1, min(int(batch), n))
    return B, list(range(0, n, B))


def fade(O):
    """float64 ``f(u)``, ``u = 0 .. O - 1``."""
    u = np.arange(int(O), dtype=np.float64)
    return np.sin(np.pi * (2.0 * u + 1.0) / (4.0 * O)) ** 2 if O else u


def fade_table(O):
    """The table the kernels read: float32 (2, O), ``f`` then ``1 - f``, each
    rounded once from float64 (so their sum is within one float32 ulp of 1)."""
    f = fade(O)
    return np.stack([f, 1.0 - f]).astype(np.float32)


def weights(T, W, O, dtype=np.float64):
    """(n, T) weights: row ``i`` is window ``i``'s weight at every sample of
    the clip.  ``dtype=float32`` gives the weights the kernels use."""
    T, W, O = check(T, W, O)
    st = starts(T, W, O)
    n = len(st)
    tab = fade_table(O).astype(np.float64) if dtype == np.float32 else np.stack([fade(O), 1.0 - fade(O)])
    w = np.zeros((n, T), dtype=np.float64)
    for i, s in enumerate(st):
        lo = 0 if i == 0 else st[i - 1] + W - O          # where window i fades in
        hi = min(T, s + W) if i == n - 1 else s + W - O   # where window i + 1 fades in
        w[i, lo:hi] = 1.0
        if i:
            w[i, lo:lo + O] = tab[0]
            w[i - 1, lo:lo + O] = tab[1]
    return w.astype(dtype)


def overlap_add(outs, T, W, O, dtype=np.float64):
    """``y[t] = sum_i weight_i(t) outs[i][t - start_i]`` for outs (n, W)."""
    outs = np.asarray(outs)
    w = weights(T, W, O, dtype=np.float32 if dtype == np.float32 else np.float64)
    y = np.zeros(int(T), dtype=dtype)
    for i, s in enumerate(starts(T, W, O)):
        m = min(W, int(T) - s)
        y[s:s + m] += (w[i, s:s + m].astype(dtype) * outs[i, :m].astype(dtype)).astype(dtype)
    return y


def pool(Ts, W, O, batch):
    """(B, slots) of the pooled windows of clips of lengths ``Ts``, each longer
    than ``W``: ``slots = [(c, i) for c in order for i in range(n_c)]`` and
    ``B = min(batch, N)``; group ``g`` holds the slots ``[g B, g B + B)``."""
    slots = []
    for c, T in enumerate(Ts):
        T, W, O = check(T, W, O)
        if T <= W:
            raise ValueError(f"clip {c} has {T} samples: only clips longer than the window ({W}) take slots")
        slots.extend((c, i) for i in range(n_windows(T, W, O)))
    if not slots:
        raise ValueError("no clips")
    return max(1, min(int(batch), len(slots))), slots


def overlap_add_pooled(outs, Ts, W, O, batch):
    """The pooled result evaluated as ou_pool_overlap_add does, group by group
    in float32, for outs (N, W) in slot order: the list of ``y_c``.

    Sample ``t`` of a clip belongs to window ``own = min(t // H, n_c - 1)``.
    In the call for a group, the owner's slot stores the finished sample --
    ``0 + 1 v`` outside its fade-in, ``(0 + (1 - f) v_{i-1}) + f v_i`` inside
    it, the first term taken from slot ``b - 1`` when that is in the group and
    from ``y[t]`` (left by the group before) otherwise; a slot whose successor
    window is not in the group stores ``0 + (1 - f) v`` over the successor's
    fade-in; nothing else is written.  Every ``y_c`` starts as NaN, and no
    sample may be stored twice by one group."""
    B, slots = pool(Ts, W, O, batch)
    N, H, f32 = len(slots), int(W) - int(O), np.float32
    outs = np.asarray(outs, dtype=f32)
    tab = fade_table(O)
    ys = [np.full(int(T), np.nan, dtype=f32) for T in Ts]
    j = np.arange(int(W))
    for first in range(0, N, B):
        stop = min(first + B, N)
        stores = []   # applied after the group's reads: the threads of one call do not see each other's stores
        for b in range(first, stop):
            c, i = slots[b]
            n = n_windows(Ts[c], W, O)
            t = start(i, Ts[c], W, O) + j
            own = np.minimum(t // H, n - 1)
            v = outs[b]
            prev_in, next_in = i > 0 and b > first, i + 1 < n and b + 1 < stop
            u = t - i * H
            plain = (own == i) & ((i == 0) | (u >= O))
            stores.append((c, t[plain], f32(0) + f32(1) * v[plain]))
            fin = (own == i) & ~plain
            if fin.any():
                acc = f32(0) + tab[1][u[fin]] * outs[b - 1][u[fin] + H] if prev_in else ys[c][t[fin]]
                stores.append((c, t[fin], acc + tab[0][u[fin]] * v[fin]))
            out = own == i + 1
            if not next_in and out.any():
                stores.append((c, t[out], f32(0) + tab[1][t[out] - (i + 1) * H] * v[out]))
        seen = [np.zeros(int(T), dtype=bool) for T in Ts]
        for c, t, val in stores:
            assert not seen[c][t].any(), "one group stored a sample twice"
            seen[c][t] = True
            ys[c][t] = val.astype(f32)
    return ys


def stream_draw_offset(offset, k):
    """Counter offset of draw ``k`` of a stream opened at ``offset`` (64-bit)."""
    return (int(offset) + int(k) * DRAW_COUNTERS) & 0xFFFFFFFFFFFFFFFF


def stream_ring(W, O, B):
    """Capacity of a stream's input ring in samples."""
    return int(W) + int(B) * (int(W) - int(O))


class StreamShort(ValueError):
    """A stream was closed on fewer samples than one window."""


class StreamCounts:
    """The host arithmetic of one stream: ``fed`` samples pushed, ``run``
    windows run.  ``push(n)`` and ``close()`` list the steps a session takes --
    ``("feed", k)``: copy the next ``k`` samples into the ring at ``fed mod
    capacity``; ``("group", first, count, closing)``: run windows ``[first,
    first + count)`` (``count = 0``: emit the carry alone) -- and advance the
    counts as the list is built; ``bound`` is the number of samples those steps
    emit.  Nothing here depends on the device."""

    def __init__(self, W, O, B, Tp=None):
        _, self.W, self.O = check(1, W, O)
        if int(B) < 1:
            raise ValueError(f"batch must be at least 1, got {B}")
        self.B, self.H = int(B), self.W - self.O
        self.Tp = self.W if Tp is None else int(Tp)
        self.cap = stream_ring(self.W, self.O, self.B)
        self.fed = self.run = 0
        self.closed = False

    def ready(self, fed=None):
        """Regular windows whose samples are all there."""
        fed = self.fed if fed is None else fed
        return 0 if fed < self.W else (fed - self.W) // self.H + 1

    def retain(self):
        """The lowest position the ring must still hold."""
        return max(0, min(self.run * self.H, self.fed - self.W))

    def held(self):
        """The lowest position the ring does hold: it is never cleared."""
        return max(0, self.fed - self.cap)

    def bound(self, n=0, closing=False):
        """Samples ``push(n)`` would emit now, or ``close()`` with ``closing``."""
        if n < 0:
            raise ValueError(f"a push of {n} samples")
        if self.closed:
            return 0
        if closing:
            if self.fed < self.W:
                raise StreamShort(f"a stream of {self.fed} samples is shorter than one window of {self.W}")
            return self.fed - self.run * self.H
        return (self.ready(self.fed + n) - self.run) // self.B * self.B * self.H

    def push(self, n):
        n = int(n)
        if n < 0:
            raise ValueError(f"a push of {n} samples")
        if self.closed:
            raise ValueError("the stream is closed")
        if self.fed + n + self.Tp - self.W > STREAM_MAX_SAMPLES:
            raise ValueError("the stream would pass 2^40 samples")
        steps = []
        while True:
            while self.ready() - self.run >= self.B:
                steps.append(("group", self.run, self.B, False))
                self.run += self.B
            if n == 0:
                return steps
            room = self.cap - (self.fed - self.retain())
            assert room > 0, "the ring is full with no group ready"
            k = min(n, room)
            steps.append(("feed", k))
            self.fed += k
            n -= k

    def close(self):
        if self.closed:
            raise ValueError("the stream is closed")
        if self.fed < self.W:
            raise StreamShort(f"a stream of {self.fed} samples is shorter than one window of {self.W}")
        n = n_windows(self.fed, self.W, self.O)
        steps = [("group", self.run, n - self.run, True)]
        self.run, self.closed = n, True
        return steps

    @staticmethod
    def emitted(step, H, T=None):
        """Samples a ``group`` step emits (``T``: the length at close)."""
        _, first, count, closing = step
        return (T if closing else (first + count) * H) - first * H


# ---- multiplexed streams (csrc/ou_mux.hip, mux.py) -----
# C channels are streams as above, each with its own ring, carry, counts and
# (seed, offset); W, O, H and the batch B of the plan are shared.  A push only
# feeds a ring; run() pools the windows that are ready: the slot list is
# [(c, i) for c ascending for i in pending(c)], group g its slots [g B, g B + B),
# the unused slots of the last group repeating its last real slot.  A run is a
# maximal stretch of consecutive slots of one channel in a group; a closing
# channel with nothing left to run is a run without slots.  MuxCounts is that
# arithmetic; MuxOverlapAdd restates what ou_mux_overlap_add computes.

MuxRun = collections.namedtuple("MuxRun", "channel first count closing T slot out_off n")
MuxGroup = collections.namedtuple("MuxGroup", "slots real runs")   # slots: B of (channel, window, start)
MuxPlan = collections.namedtuple("MuxPlan", "slots groups counts offsets freed")

FREE, OPEN, CLOSING = "free", "open", "closing"


class MuxChannel:
    def __init__(self):
        self.state, self.fed, self.run, self.seed, self.offset = FREE, 0, 0, 0, 0


class MuxCounts:
    """The host arithmetic of ``C`` streams that share one batch-``B`` plan.
    ``open`` / ``push`` / ``close`` change one channel's counts; ``plan_run``
    lists what a ``run()`` does -- the slots, the groups with their runs, and
    per channel the count of emitted samples and its offset in the one output
    buffer (channel-major) -- and advances the counts; ``bound`` is the same
    list without advancing.  Nothing here depends on the device, and the
    grouping is a function of the sequence of calls alone."""

    def __init__(self, W, O, B, C, Tp=None):
        _, self.W, self.O = check(1, W, O)
        if int(B) < 1 or int(C) < 1:
            raise ValueError(f"batch {B} and channels {C} must be at least 1")
        self.B, self.C, self.H = int(B), int(C), self.W - self.O
        self.Tp = self.W if Tp is None else int(Tp)
        self.cap = stream_ring(self.W, self.O, self.B)
        self.ch = [MuxChannel() for _ in range(self.C)]

    def _busy(self, c, what):
        c = int(c)
        if not 0 <= c < self.C:
            raise ValueError(f"{what}: channel {c} of {self.C}")
        if self.ch[c].state == FREE:
            raise ValueError(f"{what}: channel {c} is free")
        return c, self.ch[c]

    def open(self, seed=0, offset=0, channel=None):
        if not 0 <= int(seed) < 2**64 or not 0 <= int(offset) < 2**64:
            raise ValueError("seed and offset are unsigned 64-bit integers")
        if channel is None:
            free = [c for c, s in enumerate(self.ch) if s.state == FREE]
            if not free:
                raise ValueError(f"open: all {self.C} channels are busy")
            channel = free[0]
        c = int(channel)
        if not 0 <= c < self.C:
            raise ValueError(f"open: channel {c} of {self.C}")
        s = self.ch[c]
        if s.state != FREE:
            raise ValueError(f"open: channel {c} is {s.state}")
        s.state, s.fed, s.run, s.seed, s.offset = OPEN, 0, 0, int(seed), int(offset)
        return c

    def ready(self, c):
        s = self.ch[c]
        return 0 if s.fed < self.W else (s.fed - self.W) // self.H + 1

    def retain(self, c):
        """The lowest position channel ``c``'s ring must still hold."""
        s = self.ch[c]
        return max(0, min(s.run * self.H, s.fed - self.W))

    def held(self, c):
        return max(0, self.ch[c].fed - self.cap)

    def room(self, c):
        c, s = self._busy(c, "room")
        return self.cap - (s.fed - self.retain(c)) if s.state == OPEN else 0

    def push(self, c, n):
        """Feed ``n`` samples to channel ``c``: returns the position they start
        at (they go to the ring at that position mod ``cap``).  More than
        ``room(c)`` is refused whole."""
        c, s = self._busy(c, "push")
        n = int(n)
        if n < 0:
            raise ValueError(f"a push of {n} samples")
        if s.state != OPEN:
            raise ValueError(f"push: channel {c} is closing")
        if n > self.room(c):
            raise ValueError(f"push: {n} samples, channel {c} has room for {self.room(c)}: run() first")
        if s.fed + n + self.Tp - self.W > STREAM_MAX_SAMPLES:
            raise ValueError("the stream would pass 2^40 samples")
        at = s.fed
        s.fed += n
        return at

    def close(self, c):
        c, s = self._busy(c, "close")
        if s.state != OPEN:
            raise ValueError(f"close: channel {c} is closing")
        if s.fed < self.W:
            raise StreamShort(f"channel {c}: a stream of {s.fed} samples is shorter than one window of {self.W}")
        s.state = CLOSING

    def pending(self, c):
        """The windows of channel ``c`` that can run now."""
        s = self.ch[c]
        if s.state == FREE:
            return range(0)
        return range(s.run, n_windows(s.fed, self.W, self.O) if s.state == CLOSING else self.ready(c))

    def _start(self, c, i):
        s = self.ch[c]
        return min(i * self.H, s.fed - self.W) if s.state == CLOSING else i * self.H

    def _plan(self, full_only):
        B, H = self.B, self.H
        S = [(c, i) for c in range(self.C) for i in self.pending(c)]
        if full_only:
            S = S[:len(S) // B * B]
        after = {c: s.run for c, s in enumerate(self.ch)}      # windows run, per channel, as the groups go by
        counts, freed, groups = [0] * self.C, [], []
        # closings with nothing left to run: the carry alone, ahead of every group
        alone = []
        for c, s in enumerate(self.ch):
            if s.state == CLOSING and not len(self.pending(c)):
                n = s.fed - s.run * H
                assert n == self.O, (n, self.O)
                alone.append([c, s.run, 0, 1, s.fed, 0, n])
                counts[c] = n
                freed.append(c)
        raw = []
        for g in range(0, len(S), B):
            real = S[g:g + B]
            runs = []
            for b, (c, i) in enumerate(real):
                if runs and runs[-1][0] == c:
                    runs[-1][2] += 1
                else:
                    runs.append([c, i, 1, 0, 0, b, 0])
            for r in runs:
                c, s = r[0], self.ch[r[0]]
                last = r[1] + r[2]
                if s.state == CLOSING and last == n_windows(s.fed, self.W, self.O):
                    r[3], r[4] = 1, s.fed
                    freed.append(c)
                r[6] = (s.fed if r[3] else last * H) - r[1] * H
                counts[c] += r[6]
                after[c] = last
            raw.append((real, runs))
        if alone:
            if raw:
                raw[0] = (raw[0][0], sorted(raw[0][1] + alone))
            else:
                raw.append(([], alone))
        offsets = [sum(counts[:c]) for c in range(self.C)]
        at = list(offsets)
        for real, runs in raw:
            slots = [(c, i, self._start(c, i)) for c, i in real]
            slots += [slots[-1]] * (B - len(slots)) if slots else []
            out = []
            for c, first, count, closing, T, slot, n in runs:
                out.append(MuxRun(c, first, count, closing, T, slot, at[c], n))
                at[c] += n
            groups.append(MuxGroup(slots, len(real), out))
        return MuxPlan(S, groups, counts, offsets, sorted(freed)), after

    def bound(self, full_only=False):
        """(counts, offsets) of what ``run(full_only)`` would emit now, per
        channel, in the one output buffer."""
        plan, _ = self._plan(full_only)
        return plan.counts, plan.offsets

    def plan_run(self, full_only=False):
        plan, after = self._plan(full_only)
        for c, s in enumerate(self.ch):
            s.run = after[c]
        for c in plan.freed:
            self.ch[c].__init__()
        return plan


class MuxOverlapAdd:
    """What ou_mux_overlap_add computes, group by group in float32, with the
    carries kept between the calls: ``run(plan, outs)`` takes the plan of one
    ``run()`` and, per group, the ``(B, W)`` outputs of its slots, and returns
    the per-channel samples.  Sample ``t`` of a run over windows ``[first,
    first + count)`` belongs to window ``own = min(t // H, first + count - 1)``:
    ``0 + 1 v`` outside the owner's fade-in, ``(0 + (1 - f) v_prev) + f v``
    inside it, ``v_prev`` from the slot before inside the run and from the
    channel's raw carry at the run's first window; a run that is not closing
    then leaves the raw last ``O`` samples of its last window in the carry.
    Here each product and sum is rounded (``overlap_add(dtype=float32)``); the
    kernel fuses each ``+ w v`` as ou_stream_overlap_add does.  Carries and
    outputs start as NaN, and padding slots are never read."""

    def __init__(self, W, O, C):
        self.W, self.O, self.H = int(W), int(O), int(W) - int(O)
        self.tab = fade_table(self.O)
        self.carry = np.full((int(C), self.O), np.nan, dtype=np.float32)

    def run(self, plan, outs):
        f32, W, O, H = np.float32, self.W, self.O, self.H
        ys = [np.full(n, np.nan, dtype=f32) for n in plan.counts]
        for grp, w in zip(plan.groups, outs):
            w = np.asarray(w, dtype=f32)
            for r in grp.runs:
                last = r.first + r.count - 1
                t_end = r.T if r.closing else (r.first + r.count) * H
                last_start = min(last * H, r.T - W) if r.closing else last * H
                y = ys[r.channel][r.out_off - plan.offsets[r.channel]:]
                carry = self.carry[r.channel].copy()
                for t in range(r.first * H, t_end):
                    m = t - r.first * H
                    own = min(t // H, last)
                    u = t - own * H
                    if own < r.first:
                        y[m] = f32(0) + f32(1) * carry[m]
                        continue
                    v = w[r.slot + own - r.first, t - (last_start if own == last else own * H)]
                    if own >= 1 and u < O:
                        vp = carry[u] if own == r.first else w[r.slot + own - 1 - r.first, u + H]
                        y[m] = (f32(0) + self.tab[1][u] * vp) + self.tab[0][u] * v
                    else:
                        y[m] = f32(0) + f32(1) * v
                if not r.closing:
                    self.carry[r.channel] = w[r.slot + r.count - 1, H:H + O]
        return ys
