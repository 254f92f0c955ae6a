"""Multiplexed streams on the GPU: the two kernels of
csrc/ou_mux.hip against ou_stream_gather / ou_stream_overlap_add called per
channel, ``Universe.stream_mux`` against the composition of the plan's runs on
groups assembled by hand from the slot rule, the bundle session
(ou_model_mux_*) in a fresh process, and the CLI with ``--channels``.

Everything here is bit for bit.  What is promised: per channel the kernels
give the bits of the section-15 kernels called for that channel alone, and a
mux session equals the plan's runs on the groups ``MuxCounts.plan_run`` lists,
crossfaded per channel by the float32 overlap-add of the device
(ou_overlap_add, whose ``+ w v`` are fused -- the bits section 15 defines).
Not promised: that a channel equals the same audio through a stand-alone
``Universe.stream``; that comparison, and the one with numpy's separately
rounded ``longform.overlap_add(dtype=float32)``, are printed."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import golden_state_dict, load_golden
from open_universe_amd import _lib as L
from open_universe_amd import bundle as Bd
from open_universe_amd import longform as LF
from open_universe_amd import mux as MX
from open_universe_amd.configs import get_config
from open_universe_amd.networks.universe import UniverseGAN
from open_universe_amd.utils.synthetic import synth_audio

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = torch.float32
W = 4000
POISON = 1e6
N_STEPS = 3
DRAW = 2**38


def _sp():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _fade(On):
    return torch.from_numpy(LF.fade_table(On)).to(DEV) if On else None


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------ ou_mux_gather
@pytest.mark.parametrize("On", [0, 500, 501, 2000])
@pytest.mark.parametrize("Tp,gap", [(4160, 0), (4163, 1)])
def test_mux_gather_rows_are_the_stream_gather_rows(On, Tp, gap):
    """Three channels with different ``fed``, two of them with a window that
    wraps its ring, one slot a shifted last window, the last slot a padding
    copy: every row equals ou_stream_gather for that channel with slots = 1."""
    lib = L.load()
    H, rows, C = W - On, 3, 3
    cap = W + 2 * H
    feds = [cap - 1, cap + W // 2 + 1, 2 * cap + W // 2 + 5]
    keys = [(7, 5), (2**40 + 1, 2**64 - 3), (3, 2**37)]
    rings = torch.full((C, cap), POISON, dtype=F32, device=DEV)
    for c, fed in enumerate(feds):
        x = torch.randn(fed, generator=torch.Generator().manual_seed(fed + On)).to(DEV)
        p = torch.arange(max(0, fed - cap), fed, device=DEV)
        rings[c, p % cap] = x[p]
    # (channel, window, shifted): regular windows, and the shifted last window of a stream that closes at fed
    last = [LF.n_windows(f, W, On) - 1 for f in feds]
    slots = [(0, 0, 0), (0, 1, 0), (1, (feds[1] - W) // H, 0), (1, last[1], 1), (2, (feds[2] - W) // H - 1, 0),
             (2, (feds[2] - W) // H, 0), (2, last[2], 1)]
    slots.append(slots[-1])   # padding
    n = len(slots)
    tab = (L.MuxSlot * n)()
    for e, (c, i, shifted) in zip(tab, slots):
        e.start = min(i * H, feds[c] - W) if shifted else i * H
        e.lo, e.fed, e.seed, e.offset, e.channel = max(0, feds[c] - cap), feds[c], keys[c][0], keys[c][1], c
    assert On != 501 or {e.start % 4 for e in tab} == {0, 1, 2, 3}   # the odd hop brings every residue
    mbs, nbs = W + gap, Tp + gap
    nrs = n * nbs + 5
    mix = torch.full((n * mbs + 3,), POISON, dtype=F32, device=DEV)
    nz = torch.full((rows * nrs + 3,), POISON, dtype=F32, device=DEV)
    want_mix, want_nz = mix.clone(), nz.clone()
    L.check(lib.ou_mux_gather(rings.data_ptr(), cap, C, W, tab, n, rows, Tp, mix.data_ptr(), mbs, nz.data_ptr(), nrs,
                              nbs, _sp()), "mux_gather")
    for b, (c, i, shifted) in enumerate(slots):
        L.check(lib.ou_stream_gather(rings[c].data_ptr(), cap, max(0, feds[c] - cap), feds[c], W, On, i, 1, 1, shifted,
                                     feds[c] if shifted else 0, rows, Tp, keys[c][0], keys[c][1],
                                     want_mix.data_ptr() + 4 * b * mbs, mbs, want_nz.data_ptr() + 4 * b * nbs, nrs, nbs,
                                     _sp()), "stream_gather")
    torch.cuda.synchronize()
    assert (want_mix != POISON).sum() == n * W
    assert torch.equal(mix, want_mix), (On, Tp, (mix != want_mix).nonzero()[:4].tolist())
    assert torch.equal(nz, want_nz), (On, Tp, (nz != want_nz).nonzero()[:4].tolist())


# ------------------------------------------------------------------ ou_mux_overlap_add
@pytest.mark.parametrize("On", [0, 500, 501, 2000])
@pytest.mark.parametrize("B", [1, 2, 3])
def test_mux_overlap_add_is_stream_overlap_add_per_channel(On, B):
    """Whole sessions on random OUT rows: after every group, the output
    buffer (misaligned, poison around it) and every carry equal what
    ou_stream_overlap_add leaves when called per run on that channel's own
    windows.  The lengths bring every way to close: T = W, T = W + 1, a
    regular last window closed late (the carry alone) and a shifted one."""
    lib = L.load()
    H, C = W - On, 4
    Ts = [W, W + 1, W + 3 * H, W + 2 * H + H // 2 + 1]
    late = [False, True, True, False]
    g = torch.Generator().manual_seed(100 * On + B)
    dw = [torch.randn(LF.n_windows(T, W, On), W + 8, generator=g).to(DEV)[:, :W] for T in Ts]
    tab = _fade(On)
    cs = max(On, 1) + 2
    carries = torch.full((C, cs), float("nan"), dtype=F32, device=DEV)
    ref_carries = carries.clone()
    m = LF.MuxCounts(W, On, B, C)
    for _ in Ts:
        m.open()
    fed, emitted, rnd = [0] * C, [0] * C, 0
    kinds, residues = set(), set()
    while any(s.state != LF.FREE for s in m.ch):
        rnd += 1
        assert rnd < 100
        for c, T in enumerate(Ts):
            if m.ch[c].state != LF.OPEN:
                continue
            if fed[c] == T:
                m.close(c)
                continue
            k = min(T - fed[c], m.room(c), [4100, 3999, 2 * H + 7, 10**6][c])
            m.push(c, k)
            fed[c] += k
            if fed[c] == T and not late[c]:
                m.close(c)
        plan = m.plan_run(full_only=rnd % 3 == 0)
        total, mis = sum(plan.counts), (rnd + B) % 4
        out = torch.full((total + 8,), POISON, dtype=F32, device=DEV)
        ref = out.clone()
        for grp in plan.groups:
            rows = torch.full((B, W + 8), float("nan"), dtype=F32, device=DEV)   # padding rows stay NaN
            for b, (c, i, _) in enumerate(grp.slots[:grp.real]):
                rows[b, :W] = dw[c][i]
            runs = MX.run_table(grp)
            L.check(lib.ou_mux_overlap_add(rows.data_ptr() if grp.slots else 0, W + 8, len(grp.slots), W, On, runs,
                                           len(runs), tab.data_ptr() if On else 0, carries.data_ptr() if On else 0, cs,
                                           C, out.data_ptr() + 4 * mis, total, None, _sp()), "mux_overlap_add")
            for r in grp.runs:
                got = ctypes.c_int64(-1)
                L.check(lib.ou_stream_overlap_add(dw[r.channel][r.first].data_ptr() if r.count else 0, W + 8, W, On,
                                                  r.first, r.count, r.closing, r.T, tab.data_ptr() if On else 0,
                                                  ref_carries[r.channel].data_ptr() if On else 0,
                                                  ref.data_ptr() + 4 * (mis + r.out_off), ctypes.byref(got), _sp()),
                        "stream_overlap_add")
                assert got.value == r.n
                residues.add((mis + r.out_off) % 4)
                kinds.add("alone" if r.count == 0 else "shifted" if r.closing and (r.first + r.count - 1) * H > r.T - W
                          else "closing" if r.closing else "two" if r.count > 1 else "one")
            if grp.slots and grp.real < B:
                kinds.add("padding")
            torch.cuda.synchronize()
            assert torch.equal(_bits(out), _bits(ref)), (On, B, rnd, (out != ref).nonzero()[:4].tolist())
            assert torch.equal(_bits(carries), _bits(ref_carries)), (On, B, rnd)
        assert (out[:mis] == POISON).all() and (out[mis + total:] == POISON).all()
        assert not torch.isnan(out).any()
        for c in range(C):
            emitted[c] += plan.counts[c]
    assert emitted == Ts
    assert {"shifted", "closing", "one"} <= kinds and (B == 1 or {"two", "padding"} <= kinds), kinds
    assert B == 3 or "alone" in kinds, kinds      # at B = 3 the late channel's last windows run with its close
    assert len(residues) >= 3, residues           # misaligned output offsets


# ------------------------------------------------------------------ the model
@pytest.fixture(scope="module")
def model():
    d = load_golden("pp16_c4")
    cfg = get_config("pp16", 4)
    m = UniverseGAN(**{k: v for k, v in cfg.items() if k != "_target_"})
    m.load_state_dict(golden_state_dict(d), strict=False)
    return m.to(DEV).eval()


def _clip(T, seed=0):
    return torch.from_numpy(synth_audio(T, 16000, seed)[0].astype(np.float32))


# A session as a list of calls, driven the same way on every kind of mux (Universe.stream_mux, Bundle.stream_mux,
# and -- for the composition -- a bare MuxCounts): ("open", channel, stream) takes the channel for the stream of that
# name, ("push", channel, n) feeds it the next n samples of its stream, ("close", channel), ("run", full_only).
# Returns {stream name: the concatenation of what its channel emitted}.  The source is shared with the child process.
_DRIVER = r'''
def drive(mux, script, streams, cat, between=None):
    """streams: {name: (samples, seed, offset)}."""
    on, at, got = {}, {}, {name: [] for name in streams}
    for op in script:
        if op[0] == "open":
            _, c, name = op
            assert mux.open(seed=streams[name][1], offset=streams[name][2], channel=c) == c
            on[c], at[name] = name, 0
        elif op[0] == "push":
            _, c, n = op
            name = on[c]
            assert n <= mux.room(c)
            mux.push(c, streams[name][0][at[name]:at[name] + n])
            at[name] += n
        elif op[0] == "close":
            mux.close(op[1])
        else:
            counts, offsets = mux.bound(op[1])
            ys = mux.run(op[1])
            assert [int(y.numel()) for y in ys] == list(counts)
            for c, y in enumerate(ys):
                if y.numel():
                    got[on[c]].append(y)
            if between is not None:
                between()
    return {name: cat(v) for name, v in got.items()}
'''
exec(_DRIVER)

LENS = {"a": 9000, "b": 10400, "c": 13600, "d": 4001}
KEYS = {"a": (21, 0), "b": (22, 1 << 33), "c": (2**64 - 1, 5), "d": (24, 0)}
# O = 800, B = 2: rings of 10400.  Uneven pushes; run 2 is full_only and leaves (b, 0) waiting; channel 0 closes,
# is freed by run 2 and reopened for stream d; run 3 has 7 slots (a padded last group, b across two groups, d's
# shifted last window); stream c's last window is regular, so run 4 closes it from the carry alone.
SCRIPT = [("open", 0, "a"), ("open", 1, "b"), ("open", 2, "c"),
          ("push", 0, 4100), ("push", 1, 1), ("push", 2, 7300), ("run", False),
          ("push", 0, 4900), ("close", 0), ("push", 1, 3999), ("push", 2, 17), ("run", True),
          ("open", 0, "d"), ("push", 0, 4001), ("close", 0), ("push", 1, 6400), ("close", 1), ("push", 2, 6283),
          ("run", False), ("close", 2), ("run", False), ("run", False)]


def _streams(dev=DEV):
    return {name: (_clip(T, 10 + k).to(dev), *KEYS[name]) for k, (name, T) in enumerate(LENS.items())}


class _Shadow:
    """A bare MuxCounts behind the driver's interface: records the plan of
    every run together with the channels' state when it began."""

    def __init__(self, On, B, C, Tp):
        self.m, self.plans = LF.MuxCounts(W, On, B, C, Tp), []
        self.open, self.room, self.close, self.bound = self.m.open, self.m.room, self.m.close, self.m.bound

    def push(self, c, x):
        self.m.push(c, x.numel())

    def run(self, full_only):
        state = [(s.fed, s.seed, s.offset) for s in self.m.ch]
        plan = self.m.plan_run(full_only)
        self.plans.append((plan, state))
        return [torch.empty(n) for n in plan.counts]


def _composition(model, plan_of, streams, On, B, keep_rms=False):
    """The definition: the groups MuxCounts.plan_run lists, assembled by hand
    -- MIX rows sliced from the streams, NZ rows from ou_randn at the slot's
    (seed, offset + k 2^38) -- through ``plan_of()``'s run_with_noise; then per
    stream ou_overlap_add over its windows' outputs."""
    lib = L.load()
    plan = plan_of()
    sh = _Shadow(On, B, 3, plan.Tp)
    drive(sh, SCRIPT, streams, lambda v: None)
    outs = {name: {} for name in streams}
    on = {}
    runs = iter(sh.plans)
    slots_seen = 0
    with torch.no_grad():
        for op in SCRIPT:
            if op[0] == "open":
                on[op[1]] = op[2]
            if op[0] != "run":
                continue
            p, state = next(runs)
            for grp in p.groups:
                if not grp.slots:
                    continue
                assert len(grp.slots) == B
                mix, nz = [], []
                for c, i, s in grp.slots:
                    x, seed, offset = streams[on[c]]
                    assert (seed, offset) == state[c][1:] and s + W <= state[c][0]
                    mix.append(x[s:s + W])
                    nz.append(torch.stack([Bd.randn(s + plan.Tp, seed, (offset + k * DRAW) % 2**64, device=DEV)[s:]
                                           for k in range(N_STEPS)]))
                out = plan_of().run_with_noise(torch.stack(mix)[:, None, :].contiguous(),
                                               torch.stack(nz, dim=1)[:, :, None, :].contiguous())
                for b, (c, i, _) in enumerate(grp.slots[:grp.real]):
                    assert i not in outs[on[c]]
                    outs[on[c]][i] = out[b, 0].clone() if out.ndim == 3 else out[b].clone()
                    slots_seen += 1
    tab = _fade(On)
    ys = {}
    for name, (x, _, _) in streams.items():
        T = x.numel()
        n = LF.n_windows(T, W, On)
        assert sorted(outs[name]) == list(range(n))
        w = torch.stack([outs[name][i] for i in range(n)]).contiguous()
        y = torch.full((T,), POISON, dtype=F32, device=DEV)
        L.check(lib.ou_overlap_add(w.data_ptr(), W, T, W, On, 0, n, tab.data_ptr() if On else 0, y.data_ptr(), _sp()),
                "overlap_add")
        torch.cuda.synchronize()
        ys[name] = y
        sep = LF.overlap_add(w.cpu().numpy(), T, W, On, dtype=np.float32)
        print(f"stream {name}: {int((sep != y.cpu().numpy()).sum())} of {T} samples differ from numpy's separately "
              f"rounded overlap_add(dtype=float32), max {np.abs(sep - y.cpu().numpy()).max():.3g}")
    assert slots_seen == sum(LF.n_windows(T, W, 800) for T in LENS.values())
    return ys


def _model_plan(model, B, keep_rms=False):
    def get():
        key, make = model._plan_spec(B, W, N_STEPS, model.diff_kwargs.epsilon, keep_rms)
        return model._arena_plan(key, 0, make)
    return get


@pytest.fixture(scope="module")
def session(model):
    """Universe.stream_mux on SCRIPT, and its composition."""
    streams = _streams()
    with model.stream_mux(W, 800, 3, batch=2, n_steps=N_STEPS) as mx:
        got = drive(mx, SCRIPT, streams, torch.cat)
    want = _composition(model, _model_plan(model, 2), streams, 800, 2)
    return streams, got, want


def test_universe_stream_mux_is_the_composition(model, session):
    streams, got, want = session
    for name, T in LENS.items():
        assert got[name].shape == (T,) and want[name].abs().max() > 1e-3
        assert torch.equal(got[name], want[name]), (name, float((got[name] - want[name]).abs().max()))
    # observed, not promised: the same audio through stand-alone streams on the same (2, W) plan
    for name, (x, seed, offset) in streams.items():
        with model.stream(W, 800, batch=2, n_steps=N_STEPS, seed=seed, offset=offset) as s:
            alone = torch.cat([s.push(x), s.close()])
        d = (alone - got[name]).abs()
        print(f"stream {name}: {int((d != 0).sum())} of {x.numel()} samples differ from a stand-alone "
              f"Universe.stream(batch=2), max {float(d.max()):.3g}")


def test_full_only_leaves_the_remainder_pending(model):
    x = _clip(W + 3200, 3).to(DEV)
    with model.stream_mux(W, 800, 2, batch=2, n_steps=N_STEPS) as mx:
        a, b = mx.open(seed=1), mx.open(seed=2)
        mx.push(a, x[:W])
        mx.push(b, x)
        assert mx.bound(True) == ([3200, 3200], [0, 3200]) and mx.bound(False) == ([3200, 6400], [0, 3200])
        ya, yb = mx.run(full_only=True)            # slots (a, 0), (b, 0); (b, 1) waits
        assert (ya.numel(), yb.numel()) == (3200, 3200)
        assert mx.bound(True) == ([0, 0], [0, 0])  # one slot is no full group
        assert [y.numel() for y in mx.run(full_only=True)] == [0, 0]
        ya, yb2 = mx.run()                         # the remainder, in a padded group
        assert (ya.numel(), yb2.numel()) == (0, 3200) and torch.isfinite(yb2).all()
        mx.close(a)
        mx.close(b)
        ya, yb3 = mx.run()                         # both last windows were regular: the carries alone
        assert (ya.numel(), yb3.numel()) == (800, 800)
        assert [y.numel() for y in mx.run()] == [0, 0]


def test_evicting_the_plan_between_runs_changes_nothing(model, session, monkeypatch):
    streams, got, _ = session
    monkeypatch.setenv("OUHIP_MAX_PLANS", "1")
    key, _ = model._plan_spec(2, W, N_STEPS, model.diff_kwargs.epsilon, False)
    evicted = []

    def between():
        with torch.no_grad():
            model.enhance(streams["a"][0][:3000], n_steps=N_STEPS)   # another length: the LRU of one entry drops the plan
        evicted.append(key not in model._plans)

    with model.stream_mux(W, 800, 3, batch=2, n_steps=N_STEPS) as mx:
        again = drive(mx, SCRIPT, streams, torch.cat, between)
    assert evicted and all(evicted)
    for name in LENS:
        assert torch.equal(again[name], got[name]), name


def test_stream_mux_refusals(model):
    for kw in ({"target": torch.zeros(1)}, {"use_aux_signal": True}, {"ensemble": 2}, {"warm_start": 1}):
        with pytest.raises(NotImplementedError):
            model.stream_mux(W, 800, 2, **kw)
    with pytest.raises(TypeError):
        model.stream_mux(W, 800, 2, windows=3)
    for bad in ((W, W // 2 + 1, 2, 1), (W, -1, 2, 1), (0, 0, 2, 1), (W, 800, 0, 1), (W, 800, 2, 0)):
        with pytest.raises(ValueError):
            model.stream_mux(bad[0], bad[1], bad[2], batch=bad[3])
    with model.stream_mux(W, 800, 2, batch=2, n_steps=N_STEPS) as mx:
        for call in (lambda: mx.push(0, _clip(5)), lambda: mx.close(0), lambda: mx.room(0)):
            with pytest.raises(ValueError):
                call()                               # a free channel
        c = mx.open(seed=3)
        assert c == 0 and mx.room(c) == W + 2 * 3200
        with pytest.raises(ValueError):
            mx.open(channel=0)                       # busy
        with pytest.raises(ValueError):
            mx.push(c, torch.zeros(mx.room(c) + 1))  # past room: refused whole
        assert mx.counts.ch[c].fed == 0
        mx.push(c, _clip(W - 1))
        with pytest.raises(LF.StreamShort):
            mx.close(c)
        assert [y.numel() for y in mx.run()] == [0, 0]
        mx.push(c, _clip(1))                         # the channel stayed open: one more sample makes a window
        mx.close(c)
        with pytest.raises(ValueError):
            mx.push(c, _clip(1))                     # closing
        ys = mx.run()
        assert ys[0].numel() == W and ys[1].numel() == 0 and mx.open() == 0   # free again
    cpu = UniverseGAN(**{k: v for k, v in get_config("pp16", 4).items() if k != "_target_"}).eval()
    with pytest.raises(L.OuHipError):
        cpu.stream_mux(W, 800, 2)
    # the C entry points refuse on the host, nothing is launched
    lib = L.load()
    x = torch.zeros(64, device=DEV)
    slot = (L.MuxSlot * 1)()
    slot[0].fed = 7
    assert lib.ou_mux_gather(x.data_ptr(), 20, 1, 8, slot, 1, 0, 0, x.data_ptr(), 8, 0, 0, 0, _sp()) != 0
    assert b"ring holds" in lib.ou_last_error()
    run = (L.MuxRun * 1)()
    assert lib.ou_mux_overlap_add(x.data_ptr(), 8, 1, 8, 2, run, 1, x.data_ptr(), x.data_ptr(), 2, 1, x.data_ptr(), 64,
                                  None, _sp()) != 0
    assert b"count" in lib.ou_last_error()


# ------------------------------------------------------------------ the bundle session
_CHILD = r'''
import sys
import numpy as np, torch
from open_universe_amd import _lib as L
from open_universe_amd.bundle import Bundle
from open_universe_amd.longform import StreamShort
assert "open_universe_amd.engine" not in sys.modules and "open_universe_amd.plan" not in sys.modules
path, xf, outf = sys.argv[1:4]
data = np.load(xf, allow_pickle=True)
script = [tuple(op) for op in data["script"].tolist()]
streams = {name: (torch.from_numpy(data["x_" + name]).cuda(), int(data["k_" + name][0]), int(data["k_" + name][1]))
           for name in data["names"].tolist()}
b = Bundle(path)
W, B = b.length, b.batch
x = streams["a"][0]
with b.stream_mux(800, 3) as mx:
    res = drive(mx, script, streams, torch.cat, between=lambda: b.status())
    assert b.status() == 0
    # refusals: a free channel, a busy one, a push past room, enhance* and a stream while the mux is open
    calls = [lambda: mx.push(1, x[:5]), lambda: mx.close(1), lambda: mx.room(1), lambda: b.stream(800),
             lambda: b.stream_mux(800, 2), lambda: b.enhance(torch.stack([x[:W]] * B)), lambda: b.enhance_long(x, 800)]
    c = mx.open(seed=3)
    assert c == 0 and mx.room(c) == W + B * (W - 800)
    calls += [lambda: mx.open(channel=0), lambda: mx.push(0, torch.zeros(mx.room(0) + 1)), lambda: mx.open(channel=3)]
    for k, call in enumerate(calls):
        try:
            call()
        except L.OuHipError as e:
            pass
        else:
            raise AssertionError(f"call {k} was accepted")
    mx.push(c, x[:W - 1])
    try:
        mx.close(c)
    except StreamShort as e:
        assert "shorter than one window" in str(e)
    else:
        raise AssertionError("a stream shorter than one window was closed")
    assert b.lib.ou_model_mux_close(mx.h, c) == L.STREAM_SHORT == 3
    mx.push(c, x[W - 1:W])                      # the channel stayed open
    mx.close(c)
    assert [y.numel() for y in mx.run()] == [W, 0, 0] and b.status() == 0
with b.stream(800) as s:                        # the mux is gone: a stream opens, and excludes a mux
    try:
        b.stream_mux(800, 2)
    except L.OuHipError as e:
        assert "session" in str(e)
    else:
        raise AssertionError("a mux was opened beside a stream")
assert torch.equal(b.enhance(torch.stack([x[:W]] * B), seed=1), b.enhance(torch.stack([x[:W]] * B), seed=1))
b.close()
np.savez(outf, **{k: v.cpu().numpy() for k, v in res.items()})
'''


def test_bundle_stream_mux_in_a_fresh_process(model, tmp_path, monkeypatch):
    """Bundle.stream_mux on the (2, 4000) bundle, driven by SCRIPT in a fresh
    process, equals Universe.stream_mux driven by SCRIPT here on the plan the
    bundle was written from -- the bundle's tiles and exponents."""
    streams = _streams("cpu")
    path = str(tmp_path / "b.oub")
    x = _clip(2 * W, 2)
    with torch.no_grad():
        ex = Bd.export_bundle(model, path, 2, W, n_steps=N_STEPS, calib=torch.stack([x[:W], x[W:]]), name="pp16_c4")
    xf, outf = str(tmp_path / "x.npz"), str(tmp_path / "out.npz")
    np.savez(xf, script=np.array(SCRIPT, dtype=object), names=np.array(list(streams)),
             **{"x_" + n: v[0].numpy() for n, v in streams.items()},
             **{"k_" + n: np.array(v[1:], dtype=np.uint64) for n, v in streams.items()})
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", _DRIVER + _CHILD, path, xf, outf], capture_output=True, text=True,
                       timeout=240, env=env, cwd=ROOT)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    res = np.load(outf)
    monkeypatch.setattr(model, "_arena_plan", lambda key, slot, make: ex.plan)
    with model.stream_mux(W, 800, 3, batch=2, n_steps=N_STEPS) as mx:
        want = drive(mx, SCRIPT, {n: (v[0].to(DEV), v[1], v[2]) for n, v in streams.items()}, torch.cat)
    for name, T in LENS.items():
        y = res[name]
        assert y.shape == (T,) and np.isfinite(y).all() and np.abs(y).max() > 1e-3
        assert np.array_equal(y, want[name].cpu().numpy()), (name, np.abs(y - want[name].cpu().numpy()).max())


# ------------------------------------------------------------------ the CLI
@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    from test_api_surface import _write_ckpt

    return _write_ckpt(str(tmp_path_factory.mktemp("mux_ckpt")), with_ema=False)[0]


def _cli(ckpt, data, *extra):
    # OUHIP_AUTOTUNE=0: the tuner picks tiles by timing them, so two processes may pick different ones and then
    # differ in the last bits; without it the tiles are a function of the shapes alone
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), OUHIP_AUTOTUNE="0")
    cmd = [sys.executable, "-m", "open_universe_amd.bin.enhance_stream", "--model", ckpt, "--n_steps", str(N_STEPS),
           "--window", "0.25", "--overlap", "0.05", "--seed", "11", "--device", DEV, "--chunk", "0.0817", *extra]
    r = subprocess.run(cmd, input=data, capture_output=True, timeout=240, env=env, cwd=ROOT)   # stdin is a pipe
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    return r


@pytest.fixture()
def untuned(monkeypatch):
    """As the CLI's process: a model loaded here records without the tuner;
    the engines of the other tests keep theirs."""
    monkeypatch.setenv("OUHIP_AUTOTUNE", "0")
    tuner = L.TUNER
    yield
    L.TUNER = tuner


@pytest.mark.parametrize("fmt", ["f32le", "s16le"])
def test_cli_with_two_channels_equals_stream_mux_in_lockstep(ckpt, fmt, untuned):
    from open_universe_amd import inference_utils
    from open_universe_amd.bin import enhance_stream as cli

    T, N, chunk = 9001, 2, 1307
    x = np.stack([_clip(T, 8).numpy() * 0.5, _clip(T, 9).numpy() * 0.4], axis=1)      # (T, 2) frames
    data = cli.encode(x.reshape(-1), fmt)
    r = _cli(ckpt, data + b"\x01", "--format", fmt, "--window-batch", "2", "--rate", "16000", "--channels", "2")
    frames = torch.from_numpy(cli.decode(data, fmt)).reshape(-1, N)                   # the torn last frame is dropped
    m = inference_utils.load_model(ckpt, device=DEV)
    outs = []
    with m.stream_mux(W, 800, N, batch=2, n_steps=N_STEPS) as mx, torch.no_grad():
        for c in range(N):
            mx.open(seed=11 + c)
        for at in range(0, T, chunk):
            for c in range(N):
                mx.push(c, frames[at:at + chunk, c])
            outs.append(torch.stack(mx.run(), dim=1))
        for c in range(N):
            mx.close(c)
        outs.append(torch.stack(mx.run(), dim=1))
    want = torch.cat(outs).cpu().numpy()
    assert want.shape == (T, N) and np.abs(want).max(axis=0).min() > 1e-3
    assert not np.array_equal(want[:, 0], want[:, 1])
    assert r.stdout == cli.encode(want.reshape(-1), fmt)


def test_cli_without_channels_is_the_single_stream(ckpt, untuned):
    from open_universe_amd import inference_utils
    from open_universe_amd.bin import enhance_stream as cli

    T = 9001
    data = cli.encode(_clip(T, 8).numpy() * 0.5, "f32le")
    r = _cli(ckpt, data, "--format", "f32le", "--window-batch", "2", "--rate", "16000")
    m = inference_utils.load_model(ckpt, device=DEV)
    with m.stream(W, 800, batch=2, n_steps=N_STEPS, seed=11) as s, torch.no_grad():
        want = torch.cat([s.push(torch.from_numpy(cli.decode(data, "f32le"))), s.close()]).cpu().numpy()
    assert want.shape == (T,) and r.stdout == cli.encode(want, "f32le")
