"""The host arithmetic of multiplexed streams (longform.MuxCounts and
longform.MuxOverlapAdd) against brute force over random
sequences of open / push / close / run, and the refusals that need no device.
No GPU involved."""
import numpy as np
import pytest

from open_universe_amd import longform as LF


class Brute:
    """The definition, one channel at a time and one sample position at a
    time; nothing is shared with MuxCounts."""

    def __init__(self, W, O, B, C):
        self.W, self.O, self.B, self.C, self.H = W, O, B, C, W - O
        self.ch = {}          # c -> dict(fed, run, closing, ran, emitted)

    def pending(self, c):
        s = self.ch[c]
        out, i = [], s["run"]
        if s["closing"]:
            T = s["fed"]
            n = 1
            while (n - 1) * self.H + self.W < T:
                n += 1
            return [(i, min(i * self.H, T - self.W)) for i in range(s["run"], n)]
        while i * self.H + self.W <= s["fed"]:
            out.append((i, i * self.H))
            i += 1
        return out

    def run(self, full_only):
        S = [(c, i, st) for c in sorted(self.ch) for i, st in self.pending(c)]
        if full_only:
            S = S[:len(S) // self.B * self.B]
        groups = [S[g:g + self.B] for g in range(0, len(S), self.B)]
        emitted = {c: 0 for c in range(self.C)}
        for c, i, st in S:
            s = self.ch[c]
            assert i == s["run"]
            s["run"] += 1
            s["ran"].append(st)
        for c in sorted(self.ch):
            s = self.ch[c]
            final = s["run"] * self.H
            if s["closing"] and not self.pending(c):
                final = s["fed"]
            emitted[c] = final - s["emitted"]
            s["emitted"] = final
            if s["closing"] and final == s["fed"]:
                s["done"] = True
        done = {c: self.ch.pop(c) for c in [c for c in self.ch if self.ch[c].get("done")]}
        return S, groups, emitted, done


def _drive(seed, n_cases, check):
    rng = np.random.default_rng(seed)
    for _ in range(n_cases):
        W = int(rng.integers(1, 40))
        O = int(rng.integers(0, W // 2 + 1))
        B = int(rng.integers(1, 6))
        C = int(rng.integers(1, 5))
        m, br = LF.MuxCounts(W, O, B, C, Tp=W + 3), Brute(W, O, B, C)
        check.start(m, br)
        for _ in range(int(rng.integers(5, 60))):
            what = rng.choice(["open", "push", "push", "push", "close", "run", "run", "full"])
            busy = sorted(br.ch)
            if what == "open":
                if len(busy) == C:
                    with pytest.raises(ValueError):
                        m.open()
                    continue
                want = min(set(range(C)) - set(busy))
                c = m.open(seed=int(rng.integers(0, 100)))
                assert c == want
                br.ch[c] = dict(fed=0, run=0, closing=False, ran=[], emitted=0)
                check.opened(c)
            elif what == "push" and busy:
                c = int(rng.choice(busy))
                if br.ch[c]["closing"]:
                    with pytest.raises(ValueError):
                        m.push(c, 1)
                    continue
                room = m.room(c)
                n = int(min(room, rng.choice([0, 1, 2, W, W - O, room, int(rng.integers(0, 3 * W))])))
                fed = br.ch[c]["fed"]
                with pytest.raises(ValueError):
                    m.push(c, room + 1)            # refused whole: nothing consumed
                assert m.ch[c].fed == fed
                assert m.push(c, n) == fed
                br.ch[c]["fed"] += n
                check.pushed(c, fed, n)
            elif what == "close" and busy:
                c = int(rng.choice(busy))
                s = br.ch[c]
                if s["closing"]:
                    with pytest.raises(ValueError):
                        m.close(c)
                elif s["fed"] < W:
                    with pytest.raises(LF.StreamShort):
                        m.close(c)
                    assert m.ch[c].state == LF.OPEN      # that channel only, and it stays open
                else:
                    m.close(c)
                    s["closing"] = True
            elif what in ("run", "full"):
                full = what == "full"
                counts, offsets = m.bound(full)
                before = {c: dict(s) for c, s in br.ch.items()}
                S, groups, emitted, done = br.run(full)
                plan = m.plan_run(full)
                assert (plan.counts, plan.offsets) == (counts, offsets)
                assert plan.slots == [(c, i) for c, i, _ in S]
                assert counts == [emitted[c] for c in range(C)]
                assert offsets == [sum(counts[:c]) for c in range(C)]
                assert plan.freed == sorted(done)
                check.ran(plan, groups, before, done)
                for c, s in done.items():
                    assert s["emitted"] == s["fed"]          # the emitted counts sum to T_c
                    T = s["fed"]
                    assert s["ran"] == LF.starts(T, W, O)    # every window once, in order
                    assert m.ch[c].state == LF.FREE
            for c, s in br.ch.items():
                assert (m.ch[c].fed, m.ch[c].run) == (s["fed"], s["run"])


class _Nothing:
    def start(self, m, br): pass
    def opened(self, c): pass
    def pushed(self, c, at, n): pass
    def ran(self, plan, groups, before, done): pass


@pytest.mark.parametrize("seed", range(4))
def test_counts_slots_and_offsets_match_brute_force(seed):
    _drive(seed, 120, _Nothing())


class _Groups(_Nothing):
    """The groups and runs of a plan against the slot rule."""

    def start(self, m, br):
        self.m = m

    def ran(self, plan, groups, before, done):
        m = self.m
        B, H, W, O = m.B, m.H, m.W, m.O
        carry_only = [c for c, s in before.items() if s["closing"] and c in done and
                      not any(c == cc for cc, _, _ in sum(groups, []))]
        if not groups and carry_only:
            assert len(plan.groups) == 1 and plan.groups[0].slots == [] and plan.groups[0].real == 0
        else:
            assert len(plan.groups) == len(groups)
        at = list(plan.offsets)
        seen_alone = []
        for k, grp in enumerate(plan.groups):
            real = groups[k] if groups else []
            assert grp.real == len(real) and grp.slots[:grp.real] == real
            if real:
                assert len(grp.slots) == B and grp.slots[grp.real:] == [real[-1]] * (B - len(real))
            assert [r.channel for r in grp.runs] == sorted({r.channel for r in grp.runs})   # one run per channel
            covered = []
            for r in grp.runs:
                assert r.out_off == at[r.channel]
                at[r.channel] += r.n
                if r.count == 0:
                    assert k == 0 and r.closing and r.T == before[r.channel]["fed"] and r.n == O
                    assert r.T == (r.first - 1) * H + W
                    seen_alone.append(r.channel)
                    continue
                assert [(c, i) for c, i, _ in real[r.slot:r.slot + r.count]] == \
                    [(r.channel, r.first + j) for j in range(r.count)]
                covered.extend(range(r.slot, r.slot + r.count))
                # maximal: the neighbours are other channels
                assert r.slot == 0 or real[r.slot - 1][0] != r.channel
                assert r.slot + r.count == len(real) or real[r.slot + r.count][0] != r.channel
                if r.closing:
                    assert r.T == before[r.channel]["fed"] and r.first + r.count == LF.n_windows(r.T, W, O)
                    assert r.n == r.T - r.first * H
                else:
                    assert r.n == r.count * H
            assert covered == list(range(len(real)))     # padding slots belong to no run
        assert seen_alone == sorted(carry_only)
        assert at == [o + n for o, n in zip(plan.offsets, plan.counts)]


@pytest.mark.parametrize("seed", range(4))
def test_groups_and_runs_follow_the_slot_rule(seed):
    _drive(100 + seed, 120, _Groups())


class _Rings(_Nothing):
    """Simulate every ring position by position: at every run, every sample of
    every slot -- a shifted last window included -- is still in its ring."""

    def start(self, m, br):
        self.m = m
        self.rings = np.full((m.C, m.cap), -1, dtype=np.int64)

    def opened(self, c):
        self.rings[c] = -1

    def pushed(self, c, at, n):
        assert n <= self.m.cap
        p = np.arange(at, at + n)
        self.rings[c][p % self.m.cap] = p
        if at + n:
            q = np.arange(self.m.retain(c), at + n)
            assert (self.rings[c][q % self.m.cap] == q).all()
            assert self.m.held(c) <= self.m.retain(c)

    def ran(self, plan, groups, before, done):
        for grp in plan.groups:
            for c, i, st in grp.slots:
                p = np.arange(st, st + self.m.W)
                assert (self.rings[c][p % self.m.cap] == p).all(), (c, i, st)
                assert st >= max(0, before[c]["fed"] - self.m.cap)


@pytest.mark.parametrize("seed", range(4))
def test_no_ring_drops_a_sample_a_window_reads(seed):
    _drive(200 + seed, 120, _Rings())


@pytest.mark.parametrize("B", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("W,O", [(16, 0), (16, 1), (16, 5), (16, 8)])
def test_numpy_mux_overlap_add_equals_overlap_add_per_channel(W, O, B):
    """Three channels of different lengths pushed in uneven pieces, runs with
    and without ``full_only`` in between: per channel the concatenation of what
    MuxOverlapAdd emits equals ``overlap_add(dtype=float32)`` on that
    channel's windows, bit for bit, whatever slot each window ran in."""
    rng = np.random.default_rng(W * 100 + O * 10 + B)
    H = W - O
    Ts = [W, W + 1, 3 * H + W, 5 * H + W - 3][:3] if B % 2 else [5 * H + W - 3, W + 1, 3 * H + W]
    C = len(Ts)
    outs = [rng.standard_normal((LF.n_windows(T, W, O), W)).astype(np.float32) for T in Ts]
    m, oa = LF.MuxCounts(W, O, B, C), LF.MuxOverlapAdd(W, O, C)
    for T in Ts:
        m.open()
    fed, got = [0] * C, [[] for _ in Ts]

    def run(full):
        plan = m.plan_run(full)
        rows = [np.stack([outs[c][i] for c, i, _ in g.slots]) if g.slots else np.zeros((0, W), np.float32)
                for g in plan.groups]
        for g, r in zip(plan.groups, rows):      # padding rows are computed and must not be read
            r[g.real:] = np.nan
        for c, y in enumerate(oa.run(plan, rows)):
            got[c].append(y)

    step = 0
    while any(f < T for f, T in zip(fed, Ts)) or any(s.state != LF.FREE for s in m.ch):
        for c, T in enumerate(Ts):
            if m.ch[c].state != LF.OPEN:
                continue
            n = min(T - fed[c], m.room(c), int(rng.integers(0, 2 * W)))
            m.push(c, n)
            fed[c] += n
            if fed[c] == T:
                m.close(c)
        run(full=step % 3 == 1)
        step += 1
        assert step < 1000
    for c, T in enumerate(Ts):
        y = np.concatenate(got[c])
        want = LF.overlap_add(outs[c], T, W, O, dtype=np.float32)
        assert y.shape == want.shape and y.tobytes() == want.tobytes(), (c, T, np.flatnonzero(y != want)[:4])


def test_refusals_that_need_no_device():
    with pytest.raises(ValueError):
        LF.MuxCounts(8, 5, 2, 3)        # O > W / 2
    with pytest.raises(ValueError):
        LF.MuxCounts(8, 2, 0, 3)
    with pytest.raises(ValueError):
        LF.MuxCounts(8, 2, 2, 0)
    m = LF.MuxCounts(8, 2, 2, 2)
    for call in (lambda: m.push(0, 1), lambda: m.close(0), lambda: m.room(0), lambda: m.push(2, 1)):
        with pytest.raises(ValueError):
            call()                      # a free channel, a channel that is not there
    assert m.open(seed=2**64 - 1, offset=5, channel=1) == 1
    with pytest.raises(ValueError):
        m.open(channel=1)               # busy
    with pytest.raises(ValueError):
        m.open(seed=2**64)
    with pytest.raises(ValueError):
        m.open(channel=2)
    assert m.open() == 0
    with pytest.raises(ValueError):
        m.open()                        # none free
    assert m.room(1) == m.cap == 8 + 2 * 6
    with pytest.raises(ValueError):
        m.push(1, m.cap + 1)
    with pytest.raises(ValueError):
        m.push(1, -1)
    m.push(1, 7)
    with pytest.raises(LF.StreamShort):
        m.close(1)
    assert m.ch[1].state == LF.OPEN and m.bound() == ([0, 0], [0, 0])
    m.push(1, 1)
    m.close(1)
    with pytest.raises(ValueError):
        m.push(1, 1)                    # closing
    with pytest.raises(ValueError):
        m.open(channel=1)               # still busy until its last samples are out
    assert m.bound(full_only=True) == ([0, 0], [0, 0])
    plan = m.plan_run()
    assert plan.counts == [0, 8] and plan.freed == [1] and m.ch[1].state == LF.FREE
    big = LF.MuxCounts(8, 0, 1, 1, Tp=12)
    big.open()
    big.ch[0].fed = (1 << 40) - 8       # host arithmetic alone: no ring behind it
    big.ch[0].run = big.ch[0].fed // 8
    with pytest.raises(ValueError):
        big.push(0, 5)                  # 2^40 - 8 + 5 + (Tp - W) passes 2^40
    big.push(0, 4)
