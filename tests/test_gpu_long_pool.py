"""Pooled windows on the GPU (csrc/ou_pool.hip, ``Universe.enhance_long_many``,
``--window-pool``): the two kernels on their own -- the gather bit for bit
against torch indexing, the overlap-add bit for bit against the existing
ou_overlap_add run clip by clip on the same windows, for every grouping --
``enhance_long_many`` end to end against the composition it is defined as (the
(3, 4000) plan run group by group on hand-assembled slots, crossfaded in
float64 with the weights written out in tests/test_gpu_long.py), its one-clip
and short-clip cases against ``enhance_long`` and ``enhance``, and the CLI at
world sizes 1 and 2.

Clips of 9000, 4001 and 10400 samples at W, O = 4000, 800 have 3 + 2 + 3
windows: at batch 3 the groups are {A0, A1, A2}, {B0, B1, C0}, {C1, C2, copy}.
Tolerances are those of tests/test_gpu_long.py (``_close``)."""
import contextlib
import ctypes
import os

import numpy as np
import pytest
import torch

from open_universe_amd import _lib as L
from test_gpu_long import DEV, F32, N_STEPS, O, POISON, W, _clip, _close, _crossfade, _sp, _starts
from test_gpu_long import model  # noqa: F401  (the pp16_c4 fixture)

pytestmark = pytest.mark.gpu
TS = [9000, 4001, 10400]


def _slots(Ts, Wn, On):
    return [(c, s) for c, T in enumerate(Ts) for s in _starts(T, Wn, On)]   # (clip, start of the window)


def _pool_clips(xs=None, noise=None, ys=None, Ts=TS, rstrides=None):
    """The ou_pool_clip array of device tensors (None: a null pointer)."""
    arr = (L.PoolClip * len(Ts))()
    for c, T in enumerate(Ts):
        arr[c] = L.PoolClip(xs[c].data_ptr() if xs else 0, noise[c].data_ptr() if noise else 0,
                            ys[c].data_ptr() if ys else 0, T, rstrides[c] if rstrides else 0)
    return arr


def _offset(n, mis, fill=None, gen=None):
    """n floats on the device starting ``mis`` floats past an allocation (256-byte aligned)."""
    buf = torch.empty(n + 8, dtype=F32, device=DEV)
    if gen is not None:
        buf.copy_(torch.randn(n + 8, generator=gen))
    else:
        buf.fill_(fill)
    return buf, buf[mis:mis + n]


# ------------------------------------------------------------------ ou_pool_gather
@pytest.mark.parametrize("win,gap,mis", [(4160, 0, 0), (4160, 36, 1), (4163, 1, 0), (4163, 0, 3)])
def test_pool_gather_is_bit_exact(win, gap, mis):
    """mix[b][j] = x_c[start + j] and nz[r][b][j] = noise_c[r][start + j] for
    slot first + b = (c, start): one clip's windows, a group that straddles two
    clips, one that runs past N (the clamp) and all slots at once; destination
    strides larger than a row with POISON between the rows; sources and rows at
    16-byte aligned and misaligned addresses."""
    lib = L.load()
    rows = 3
    slots = _slots(TS, W, O)
    N = len(slots)
    assert N == 8
    g = torch.Generator().manual_seed(win + mis)
    xs = [_offset(T, (mis + c) % 4, gen=g)[1] for c, T in enumerate(TS)]
    rs = [_starts(T, W, O)[-1] + win + 3 * (c % 2) for c, T in enumerate(TS)]   # the rows' bases differ mod 4
    noise = [_offset(rows * r, (mis + 2 * c) % 4, gen=g)[1] for c, r in enumerate(rs)]
    clips = _pool_clips(xs, noise, None, TS, rs)
    for first, count in ((0, 3), (3, 3), (6, 3), (0, N), (7, 1)):
        mbs, nbs = W + gap, win + gap
        nrs = count * nbs + 5
        mix = torch.full((count * mbs + 3,), POISON, dtype=F32, device=DEV)
        nz = torch.full((rows, nrs), POISON, dtype=F32, device=DEV)
        L.check(lib.ou_pool_gather(clips, len(TS), W, O, first, count, rows, win, mix.data_ptr(), mbs, nz.data_ptr(),
                                   nrs, nbs, _sp()), "pool_gather")
        want_mix, want_nz = torch.full_like(mix, POISON), torch.full_like(nz, POISON)
        for b in range(count):
            c, s = slots[min(first + b, N - 1)]
            want_mix[b * mbs:b * mbs + W] = xs[c][s:s + W]
            want_nz[:, b * nbs:b * nbs + win] = noise[c].view(rows, rs[c])[:, s:s + win]
        torch.cuda.synchronize()
        assert torch.equal(mix, want_mix) and torch.equal(nz, want_nz), (first, count)


# ------------------------------------------------------------------ ou_pool_overlap_add
def _fade(On):
    u = np.arange(On, dtype=np.float64)
    f = np.sin(np.pi * (2 * u + 1) / (4 * max(On, 1))) ** 2
    return torch.from_numpy(np.stack([f, 1 - f]).astype(np.float32)).to(DEV) if On else None   # [2][O], f then 1 - f


@pytest.mark.parametrize("On", [O, 0, 2000])
def test_pool_overlap_add_matches_overlap_add_clip_by_clip(On):
    """Every y starts as NaN inside POISON (clip 1's misaligned by 1).  For
    calls of 1, 2, 3, 5 and N slots each y_c equals, bit for bit, what
    ou_overlap_add stores for that clip alone from the same windows, and
    passes ``_close`` against the float64 crossfade."""
    lib = L.load()
    slots = _slots(TS, W, On)
    N = len(slots)
    g = torch.Generator().manual_seed(31 + On)
    wins = torch.randn(N, W + 8, generator=g)
    dw = wins.to(DEV)
    tab = _fade(On)
    tab_ptr = tab.data_ptr() if On else 0
    ref, s = [], 0
    for T in TS:   # the existing kernel, one call per clip
        n = len(_starts(T, W, On))
        y = torch.empty(T, dtype=F32, device=DEV)
        L.check(lib.ou_overlap_add(dw[s].data_ptr(), W + 8, T, W, On, 0, n, tab_ptr, y.data_ptr(), _sp()), "overlap_add")
        w = wins[s:s + n, :W].numpy()
        _close(f"overlap_add T{T} O{On}", y.cpu().numpy(), _crossfade(w, T, W, On, np.float64),
               _crossfade(w, T, W, On, np.float32))
        ref.append(y)
        s += n
    for count in (1, 2, 3, 5, N):
        bufs = [_offset(T, 1 if c == 1 else 0, fill=POISON) for c, T in enumerate(TS)]
        for _, y in bufs:
            y.fill_(float("nan"))
        clips = _pool_clips(None, None, [y for _, y in bufs], TS)
        for first in range(0, N, count):   # the last call's count runs past N
            L.check(lib.ou_pool_overlap_add(clips, len(TS), W, On, first, count, dw[first].data_ptr(), W + 8, tab_ptr,
                                            _sp()), "pool_overlap_add")
        torch.cuda.synchronize()
        for c, (buf, y) in enumerate(bufs):
            mis = 1 if c == 1 else 0
            assert (buf[:mis] == POISON).all() and (buf[mis + TS[c]:] == POISON).all(), (count, c)
            assert torch.equal(y, ref[c]), (count, c)


def test_pool_refusals_on_the_host():
    """Nothing is launched: every argument is checked first (tests/emu/pool_emu.cpp has the full list)."""
    lib = L.load()
    x = torch.zeros(9000, device=DEV)
    y = torch.zeros(9000, device=DEV)
    clips = _pool_clips([x], None, [y], [9000])
    assert lib.ou_pool_gather(clips, 1, W, O, 3, 2, 0, 0, y.data_ptr(), W, 0, 0, 0, _sp()) != 0
    assert b"first slot 3 of 3" in lib.ou_last_error()
    assert lib.ou_pool_overlap_add(clips, 1, W, W // 2 + 1, 0, 2, x.data_ptr(), W, x.data_ptr(), _sp()) != 0
    assert b"overlap" in lib.ou_last_error()
    two = _pool_clips([x, x], None, [y, y[4000:]], [9000, 5000])
    assert lib.ou_pool_overlap_add(two, 2, W, O, 0, 2, x.data_ptr(), W, x.data_ptr(), _sp()) != 0
    assert b"overlap" in lib.ou_last_error()
    torch.cuda.synchronize()
    assert not y.any()


# ------------------------------------------------------------------ enhance_long_many
def _draws(model, Ts, seed):
    """The draws of consecutive enhance_long calls: per clip N_STEPS x (1, 1, L_c) from one device generator."""
    Tp = W + model.tot_ds - W % model.tot_ds
    g = torch.Generator(device=DEV).manual_seed(seed)
    Gs = [torch.stack([torch.randn((1, 1, _starts(T, W, O)[-1] + Tp), generator=g, device=DEV) for _ in range(N_STEPS)])
          for T in Ts]
    return Gs, g, Tp


@pytest.mark.parametrize("keep_rms", [False, True])
def test_enhance_long_many_is_the_composition(model, keep_rms):
    seed = 4321
    xs = [_clip(T, c).to(DEV) for c, T in enumerate(TS)]
    with torch.no_grad():
        # the plan enhance() uses for a (3, W) batch, under its key in the plan LRU
        model.enhance(torch.stack([xs[0][:W], xs[0][W:2 * W], xs[2][:W]]), n_steps=N_STEPS, keep_rms=keep_rms,
                      rng=torch.Generator(device=DEV).manual_seed(1))
        key, _ = model._plan_spec(3, W, N_STEPS, model.diff_kwargs.epsilon, keep_rms)
        plan = model._plans[key]
        Gs, g_after, Tp = _draws(model, TS, seed)
        assert plan.Tp == Tp and plan.n_noise == N_STEPS
        slots = _slots(TS, W, O)
        slots.append(slots[-1])   # {A0, A1, A2}, {B0, B1, C0}, {C1, C2, copy}
        outs = []
        for first in range(0, 9, 3):
            grp = slots[first:first + 3]
            mix = torch.stack([xs[c][s:s + W] for c, s in grp])[:, None, :]
            nz = torch.stack([Gs[c][:, 0, 0, s:s + Tp] for c, s in grp], dim=1)[:, :, None, :]
            out = plan.run_with_noise(mix.contiguous(), nz.contiguous()).clone()
            outs.extend(out[b].cpu().numpy() for b in range(3))
        n_plans = len(model._plans)
        rng = torch.Generator(device=DEV).manual_seed(seed)
        ys = model.enhance_long_many(xs, W, O, batch=3, n_steps=N_STEPS, rng=rng, keep_rms=keep_rms)
        torch.cuda.synchronize()
    assert len(ys) == 3 and len(model._plans) == n_plans and model._plans[key] is plan   # nothing beyond the (3, W) plan
    assert torch.equal(rng.get_state(), g_after.get_state())
    s = 0
    for c, T in enumerate(TS):
        n = len(_starts(T, W, O))
        o = np.stack(outs[s:s + n])
        assert ys[c].shape == (T,) and np.abs(o).max() > 1e-3
        _close(f"enhance_long_many clip {c} keep_rms={keep_rms}", ys[c].cpu().numpy(), _crossfade(o, T, W, O, np.float64),
               _crossfade(o, T, W, O, np.float32))
        s += n
    # the generator ends where three enhance_long calls leave it
    with torch.no_grad():
        r3 = torch.Generator(device=DEV).manual_seed(seed)
        for x in xs:
            model.enhance_long(x, W, O, batch=3, n_steps=N_STEPS, rng=r3, keep_rms=keep_rms)
    assert torch.equal(rng.get_state(), r3.get_state())


def test_one_clip_is_enhance_long(model):
    with torch.no_grad():
        for T in (9000, 4001):
            x = _clip(T, 5).to(DEV)
            a = model.enhance_long(x, W, O, batch=2, n_steps=N_STEPS, rng=torch.Generator(device=DEV).manual_seed(8))
            r = torch.Generator(device=DEV).manual_seed(8)
            b = model.enhance_long_many([x], W, O, batch=2, n_steps=N_STEPS, rng=r)
            b2 = model.enhance_long_many([x[None, None, :]], W, O, batch=2, n_steps=N_STEPS,
                                         rng=torch.Generator(device=DEV).manual_seed(8))
            r2 = torch.Generator(device=DEV).manual_seed(8)
            model.skip_noise((T,), r2, n_steps=N_STEPS, window=W, overlap=O)
            assert len(b) == 1 and torch.equal(b[0], a) and torch.isfinite(a).all() and a.abs().max() > 0
            assert b2[0].shape == (1, 1, T) and torch.equal(b2[0][0, 0], a)   # the same call again: the same bits
            assert torch.equal(r.get_state(), r2.get_state())


def test_a_short_clip_in_the_list_is_enhance_itself(model):
    xa, xs, xc = _clip(9000, 1).to(DEV), _clip(3000, 2).to(DEV), _clip(10400, 3).to(DEV)
    calls = []
    with torch.no_grad():
        r = torch.Generator(device=DEV).manual_seed(21)
        ya, ys, yc = model.enhance_long_many([xa, xs, xc], W, O, batch=3, n_steps=N_STEPS, rng=r,
                                             pre_noise=calls.append)
        # the short clip: enhance() on the draws that follow clip A's
        r2 = torch.Generator(device=DEV).manual_seed(21)
        model.skip_noise((9000,), r2, n_steps=N_STEPS, window=W, overlap=O)
        want = model.enhance(xs, n_steps=N_STEPS, rng=r2)
        # the long clips without it, its draws skipped before clip C: unchanged
        r3 = torch.Generator(device=DEV).manual_seed(21)
        ya2, yc2 = model.enhance_long_many(
            [xa, xc], W, O, batch=3, n_steps=N_STEPS, rng=r3,
            pre_noise=lambda i: model.skip_noise((3000,), r3, n_steps=N_STEPS, window=W, overlap=O) if i == 1 else None)
    assert calls == [0, 1, 2] and ys.shape == (3000,) and torch.equal(ys, want)
    assert torch.equal(ya, ya2) and torch.equal(yc, yc2) and torch.equal(r.get_state(), r3.get_state())


def test_many_refusals(model):
    x = _clip(9000).to(DEV)
    for kw in ({"target": x}, {"use_aux_signal": True}, {"ensemble": 2}, {"warm_start": 1}):
        with pytest.raises(NotImplementedError):
            model.enhance_long_many([x], W, O, **kw)
    with pytest.raises(TypeError):
        model.enhance_long_many([x], W, O, windows=3)
    # refused before anything is drawn, recorded or launched -- also when only a later element is bad
    rng = torch.Generator(device=DEV).manual_seed(9)
    state, plans, calls = rng.get_state(), dict(model._plans), []
    for bad in (W // 2 + 1, -1):
        with pytest.raises(ValueError):
            model.enhance_long_many([x], W, bad, rng=rng, pre_noise=calls.append)
    with pytest.raises(ValueError):
        model.enhance_long_many([x, x[None, None, None, :]], W, O, rng=rng, pre_noise=calls.append)
    with pytest.raises(ValueError):
        model.enhance_long_many([x], W, O, batch=0, rng=rng, pre_noise=calls.append)
    assert torch.equal(rng.get_state(), state) and dict(model._plans) == plans and not calls
    assert model.enhance_long_many([], W, O) == []


# ------------------------------------------------------------------ CLI
LENS = {"a.wav": 9000, "b.wav": 10400, "c.wav": 4001, "d.wav": 3000}
CLI_ARGS = ["--n_steps", "3", "--seed", "11", "--device", "cuda:0", "--window", "0.25", "--overlap", "0.05",
            "--window-batch", "3", "--chunk", "4"]


@contextlib.contextmanager
def _world(rank=None):
    """RANK / LOCAL_RANK / WORLD_SIZE of rank ``rank`` of two (both on cuda:0), or none of them."""
    keys = ("RANK", "LOCAL_RANK", "WORLD_SIZE")
    old = {k: os.environ.pop(k, None) for k in keys}
    if rank is not None:
        os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE="2")
    try:
        yield
    finally:
        for k in keys:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


@pytest.fixture(scope="module")
def cli_run(tmp_path_factory):
    """The checkpoint, the four files and the one-rank run with --window-pool, shared by the CLI tests."""
    from scipy.io import wavfile

    from open_universe_amd.bin import enhance as cli
    from test_api_surface import _write_ckpt

    tmp = tmp_path_factory.mktemp("pool_cli")
    ckpt, _, _, _ = _write_ckpt(str(tmp), with_ema=False)
    src = tmp / "noisy"
    src.mkdir()
    rng = np.random.default_rng(5)
    for name, n in LENS.items():
        wavfile.write(src / name, 16000, (rng.standard_normal(n) * 0.1).astype(np.float32))

    def run(out, *extra, rank=None):
        with _world(rank):
            assert cli.main([str(src), str(tmp / out), "--model", ckpt] + CLI_ARGS + list(extra)) == 0
        return tmp / out

    run("pool1", "--window-pool")
    return tmp, src, ckpt, run


def test_cli_window_pool_is_enhance_long_many(cli_run):
    """One rank: every run of consecutive long files of the --chunk group is
    one enhance_long_many call on the loaded audio, bit for bit (a separately
    loaded model, the same seed); the short file goes the existing way."""
    from open_universe_amd import inference_utils
    from open_universe_amd.audio import load_audio
    from open_universe_amd.bin import enhance as cli

    tmp, src, ckpt, _ = cli_run
    files, _, _ = cli.find_files(src)
    assert sorted(p.name for p in files) == sorted(LENS)
    m = inference_utils.load_model(ckpt, device=DEV, strict=False)
    rng = torch.Generator(device=DEV).manual_seed(11)
    xs = [load_audio(p)[0].to(DEV) for p in files]
    want, j = [None] * len(xs), 0
    with torch.no_grad():
        while j < len(xs):
            k = j + 1
            long = xs[j].shape[-1] > W
            while k < len(xs) and (xs[k].shape[-1] > W) == long:
                k += 1
            if long:
                want[j:k] = m.enhance_long_many(xs[j:k], window=W, overlap=O, batch=3, n_steps=3, rng=rng)
            else:
                want[j:k] = m.enhance_many(xs[j:k], n_steps=3, rng=rng)
            j = k
    n_long = 0
    for p, y in zip(files, want):
        got, fs = load_audio(tmp / "pool1" / p.name)
        assert fs == 16000 and got.shape == (1, LENS[p.name]) and torch.isfinite(got).all() and got.abs().max() > 0
        assert torch.equal(got, y.cpu()), p.name
        n_long += LENS[p.name] > W
    assert n_long == 3


def test_cli_window_pool_across_world_sizes(cli_run, monkeypatch):
    """Two ranks against one.  With --window-pool the groups differ with the
    files a rank has, so the outputs agree to the project's end-to-end bar
    (rel-RMS <= 1e-3), every file on the same noise;
    without the flag nothing is pooled and they are bit-equal, as before."""
    from open_universe_amd.audio import load_audio
    from open_universe_amd.networks.universe import UniverseGAN

    tmp, _, _, run = cli_run
    for r in (0, 1):
        run("pool2", "--window-pool", rank=r)
    for name, n in LENS.items():
        a, _ = load_audio(tmp / "pool1" / name)
        b, _ = load_audio(tmp / "pool2" / name)
        assert b.shape == (1, n) and torch.isfinite(b).all()
        rel = float(((a - b).double().square().mean() / a.double().square().mean()).sqrt())
        print(f"window-pool world 2 against 1: {name} rel-RMS {rel:.3e}")
        assert rel <= 1e-3, (name, rel)

    def never(*a, **k):
        raise AssertionError("enhance_long_many was called without --window-pool")

    monkeypatch.setattr(UniverseGAN, "enhance_long_many", never)
    run("plain1")
    for r in (0, 1):
        run("plain2", rank=r)
    for name in LENS:
        a, _ = load_audio(tmp / "plain1" / name)
        b, _ = load_audio(tmp / "plain2" / name)
        assert torch.equal(a, b) and torch.isfinite(a).all() and a.abs().max() > 0, name
