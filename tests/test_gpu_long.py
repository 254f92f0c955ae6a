"""The windowed enhance on the GPU: the two kernels of csrc/ou_long.hip on
their own (the gather bit for bit against torch indexing, the overlap-add
against a float64 evaluation of the definition), ``Universe.enhance_long``
end to end against the composition it is defined as -- the (2, 4000) plan run
group by group on slices of the global noise, crossfaded in float64 with the
weights written out here from the formulas of DESIGN.md section 14 (nothing is
imported from longform.py) -- its bundle counterpart in a fresh process, and
the CLI at world sizes 1 and 2.

Tolerance of everything that goes through the overlap-add: ``_close`` of
tests/test_gpu_misc.py, 4 x the error of the same crossfade evaluated in
float32 on the CPU, with a floor of one float32 ulp of the largest output."""
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
from open_universe_amd.configs import get_config
from open_universe_amd.networks.universe import UniverseGAN
from open_universe_amd.utils.synthetic import synth_audio

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = torch.float32
W, O = 4000, 800
TS = [4001, 9000, 10400]   # 2 windows nearly coincident; 3 with a shifted last one; exactly 3
POISON = 1e6


# ------------------------------------------------------------------ the definition, written out
def _starts(T, Wn, On):
    H = Wn - On
    n = 1 if T <= Wn else 1 + -(-(T - Wn) // H)
    return [min(i * H, T - Wn) for i in range(n)]


def _weights(T, Wn, On):
    """float64 (n, T): window i fades in over [e_{i-1} - O, e_{i-1}) with
    sin^2(pi (2 u + 1) / (4 O)), window i - 1 has 1 - f there; 0 before the
    fade-in and outside the window's span, 1 elsewhere inside it."""
    st = _starts(T, Wn, On)
    w = np.zeros((len(st), T))
    for i, s in enumerate(st):
        w[i, s:s + Wn] = 1.0
    for i in range(1, len(st)):
        e_prev = st[i - 1] + Wn
        u = np.arange(On)
        f = np.sin(np.pi * (2 * u + 1) / (4 * On)) ** 2 if On else np.zeros(0)
        w[i, :e_prev - On] = 0.0
        w[i, e_prev - On:e_prev] = f
        w[i - 1, e_prev - On:e_prev] = 1.0 - f
        w[i - 1, e_prev:] = 0.0
    return st, w


def _crossfade(outs, T, Wn, On, dtype):
    """y[t] = sum_i weight_i(t) outs[i][t - start_i], evaluated in ``dtype``."""
    st, w = _weights(T, Wn, On)
    outs = np.asarray(outs)
    y = np.zeros(T, dtype=dtype)
    for i, s in enumerate(st):
        y[s:s + Wn] += w[i, s:s + Wn].astype(dtype) * outs[i].astype(dtype)
    return y


def _close(what, got, ref64, ref32, factor=4):
    """tests/test_gpu_misc.py's bound: max|got - ref64| <= factor x
    max(max|ref32 - ref64|, 2^-23 max|ref64|)."""
    got = np.asarray(got, dtype=np.float64)
    assert np.isfinite(got).all(), what
    err = np.abs(got - ref64).max()
    yard = max(np.abs(ref32.astype(np.float64) - ref64).max(), 2.0 ** -23 * np.abs(ref64).max())
    print(f"long-ratio {what} err {err:.3e} yardstick {yard:.3e} ratio {err / yard if yard else 0:.3f}")
    assert err <= factor * yard, f"{what}: err {err:.3e} > {factor} x {yard:.3e}"


def _sp():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------ ou_window_gather
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("rows,win,gap", [(1, W, 0), (1, W, 160), (7, 4160, 0), (7, 4160, 36), (7, 4163, 1)])
def test_window_gather_is_bit_exact(T, rows, win, gap):
    """y[r][b][j] = x[r][start(first + b) + j]: the clip (1 row, win = W) and
    the noise (7 rows, win = a padded length), first + b past n (the clamp),
    destination strides larger than win, 16-byte aligned and misaligned rows."""
    lib = L.load()
    st = _starts(T, W, O)
    n = len(st)
    row = st[-1] + win
    g = torch.Generator().manual_seed(T + rows)
    x = torch.randn(rows, row + 3, generator=g).to(DEV)   # row stride row + 3: the rows' bases differ mod 4
    for first, count in ((0, n + 2), (n - 1, 2), (1, 1)):
        if first >= n:
            continue
        ybs = win + gap
        y = torch.full((rows, count * ybs + 5), POISON, dtype=F32, device=DEV)
        L.check(lib.ou_window_gather(x.data_ptr(), row + 3, rows, T, W, O, first, count, win, y.data_ptr(),
                                     count * ybs + 5, ybs, _sp()), "window_gather")
        want = torch.full_like(y, POISON)
        for b in range(count):
            s = st[min(first + b, n - 1)]
            want[:, b * ybs:b * ybs + win] = x[:, s:s + win]
        torch.cuda.synchronize()
        assert torch.equal(y, want), (first, count)


# ------------------------------------------------------------------ ou_overlap_add
def _overlap_add(wins, T, On, calls, misalign=0):
    """Run ou_overlap_add over ``calls`` [(first, count)] on device windows
    (n, W + 8 stride); returns y on the CPU."""
    lib = L.load()
    u = np.arange(On, dtype=np.float64)
    f = np.sin(np.pi * (2 * u + 1) / (4 * max(On, 1))) ** 2
    tab = torch.from_numpy(np.stack([f, 1 - f]).astype(np.float32)).to(DEV) if On else None   # [2][O], f then 1 - f
    buf = torch.full((T + 8,), POISON, dtype=F32, device=DEV)
    y = buf[misalign:misalign + T]
    bs = wins.stride(0)
    for first, count in calls:
        L.check(lib.ou_overlap_add(wins[first].data_ptr(), bs, T, W, On, first, count,
                                   tab.data_ptr() if On else 0, y.data_ptr(), _sp()), "overlap_add")
    torch.cuda.synchronize()
    assert (buf[:misalign] == POISON).all() and (buf[misalign + T:] == POISON).all()
    return y.cpu()


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("On", [O, 0, 2000])
def test_overlap_add_matches_the_definition(T, On):
    n = len(_starts(T, W, On))
    g = torch.Generator().manual_seed(7 * T + On)
    wins = torch.randn(n, W + 8, generator=g)
    dw = wins.to(DEV)
    once = _overlap_add(dw[:, :W], T, On, [(0, n + 3)])
    ref64 = _crossfade(wins[:, :W].numpy(), T, W, On, np.float64)
    ref32 = _crossfade(wins[:, :W].numpy(), T, W, On, np.float32)
    _close(f"overlap_add T{T} O{On}", once.numpy(), ref64, ref32)
    # window by window, in groups of two, and at a misaligned y: the same bits
    assert torch.equal(_overlap_add(dw[:, :W], T, On, [(i, 1) for i in range(n)]), once)
    assert torch.equal(_overlap_add(dw[:, :W], T, On, [(i, 2) for i in range(0, n, 2)], misalign=1), once)
    # a constant 1.0 comes back within one ulp of 1
    ones = _overlap_add(torch.ones(n, W, device=DEV), T, On, [(0, n)], misalign=3)
    assert (ones - 1).abs().max().item() <= 2.0 ** -23


# ------------------------------------------------------------------ the model
N_STEPS = 3


@pytest.fixture(scope="module")
def model():
    d = load_golden("pp16_c4")
    cfg = get_config("pp16", 4)
    m = UniverseGAN(**{k: v for k, v in cfg.items() if k != "_target_"})
    m.load_state_dict(golden_state_dict(d), strict=False)
    return m.to(DEV).eval()


def _clip(T, seed=0):
    return torch.from_numpy(synth_audio(T, 16000, seed)[0].astype(np.float32))


def _global_noise(model, T, seed, n_noise=N_STEPS):
    """The draws enhance_long makes: n_noise x (1, 1, L) from a device generator."""
    Tp = W + model.tot_ds - W % model.tot_ds
    Ln = _starts(T, W, O)[-1] + Tp
    g = torch.Generator(device=DEV).manual_seed(seed)
    G = torch.stack([torch.randn((1, 1, Ln), generator=g, device=DEV) for _ in range(n_noise)])
    return G, g, Tp


def _compose(run_group, x, G, Tp, T, batch):
    """The definition: groups of ``batch`` windows (unused slots repeat the
    last window) through ``run_group(mix (B, 1, W), noise (n_noise, B, 1, Tp))
    -> (B, W)``; returns the windows' outputs (n, W) as float32 numpy."""
    st = _starts(T, W, O)
    n = len(st)
    B = min(batch, n)
    outs = []
    for first in range(0, n, B):
        ss = [st[min(first + b, n - 1)] for b in range(B)]
        mix = torch.stack([x[s:s + W] for s in ss])[:, None, :]
        nz = torch.stack([G[:, 0, 0, s:s + Tp] for s in ss], dim=1)[:, :, None, :]
        out = run_group(mix.contiguous(), nz.contiguous())
        outs.extend(out[b].cpu().numpy() for b in range(min(B, n - first)))
    return np.stack(outs)


@pytest.mark.parametrize("keep_rms", [False, True])
def test_enhance_long_is_the_composition(model, keep_rms):
    T, seed = 9000, 1234
    x = _clip(T).to(DEV)
    with torch.no_grad():
        # the plan enhance() uses for a (2, W) batch, under its key in the plan LRU
        model.enhance(torch.stack([x[:W], x[W:2 * W]]), n_steps=N_STEPS, keep_rms=keep_rms,
                      rng=torch.Generator(device=DEV).manual_seed(1))
        key, _ = model._plan_spec(2, W, N_STEPS, model.diff_kwargs.epsilon, keep_rms)
        plan = model._plans[key]
        G, g_after, Tp = _global_noise(model, T, seed)
        assert plan.Tp == Tp and plan.n_noise == N_STEPS
        outs = _compose(lambda mix, nz: plan.run_with_noise(mix, nz).clone(), x, G, Tp, T, 2)   # {0, 1}, {2, copy}
        n_plans = len(model._plans)
        rng = torch.Generator(device=DEV).manual_seed(seed)
        y = model.enhance_long(x, W, O, batch=2, n_steps=N_STEPS, rng=rng, keep_rms=keep_rms)
        torch.cuda.synchronize()
    assert y.shape == (T,) and len(model._plans) == n_plans and model._plans[key] is plan
    assert torch.equal(rng.get_state(), g_after.get_state())   # n_noise draws of (1, 1, L), nothing else
    _close(f"enhance_long keep_rms={keep_rms}", y.cpu().numpy(), _crossfade(outs, T, W, O, np.float64),
           _crossfade(outs, T, W, O, np.float32))
    assert np.abs(outs).max() > 1e-3
    # a mix on the CPU is moved to the engine's device, as enhance() does: the same result
    with torch.no_grad():
        yc = model.enhance_long(x.cpu(), W, O, batch=2, n_steps=N_STEPS, keep_rms=keep_rms,
                                rng=torch.Generator(device=DEV).manual_seed(seed))
    assert yc.device == y.device and torch.equal(yc, y)
    # (B, 1, T) in, (B, 1, T) out; the clips run one after another on consecutive draws
    with torch.no_grad():
        rng = torch.Generator(device=DEV).manual_seed(seed)
        y2 = model.enhance_long(torch.stack([x, x.flip(0)])[:, None, :], W, O, batch=2, n_steps=N_STEPS, rng=rng,
                                keep_rms=keep_rms)
    assert y2.shape == (2, 1, T) and torch.equal(y2[0, 0], y) and not torch.equal(y2[1, 0].flip(0), y)


def test_a_clip_that_fits_the_window_is_enhance_itself(model):
    x = _clip(3000, 3).to(DEV)
    with torch.no_grad():
        a = model.enhance(x, n_steps=N_STEPS, rng=torch.Generator(device=DEV).manual_seed(5))
        r = torch.Generator(device=DEV).manual_seed(5)
        b = model.enhance_long(x, W, O, batch=2, n_steps=N_STEPS, rng=r)
        r2 = torch.Generator(device=DEV).manual_seed(5)
        model.skip_noise((3000,), r2, n_steps=N_STEPS, window=W, overlap=O)
    assert torch.equal(a, b) and torch.equal(r.get_state(), r2.get_state())


def test_skip_noise_with_a_window_follows_enhance_long(model):
    x = _clip(9000, 4).to(DEV)
    with torch.no_grad():
        r = torch.Generator(device=DEV).manual_seed(6)
        model.enhance_long(x, W, O, batch=2, n_steps=N_STEPS, rng=r)
        r2 = torch.Generator(device=DEV).manual_seed(6)
        model.skip_noise((9000,), r2, n_steps=N_STEPS, window=W, overlap=O)
    assert torch.equal(r.get_state(), r2.get_state())


def test_refusals(model):
    x = _clip(9000).to(DEV)
    for kw in ({"target": x}, {"use_aux_signal": True}, {"ensemble": 2}, {"warm_start": 1}):
        with pytest.raises(NotImplementedError):
            model.enhance_long(x, W, O, **kw)
    with pytest.raises(TypeError):
        model.enhance_long(x, W, O, windows=3)
    # O > W / 2 is refused before anything is drawn, recorded or launched
    rng = torch.Generator(device=DEV).manual_seed(9)
    state, plans = rng.get_state(), dict(model._plans)
    for bad in (W // 2 + 1, -1):
        with pytest.raises(ValueError):
            model.enhance_long(x, W, bad, rng=rng)
    with pytest.raises(ValueError):
        model.enhance_long(x, 0, 0, rng=rng)
    assert torch.equal(rng.get_state(), state) and dict(model._plans) == plans
    # the C entry points refuse it too (host-side checks, nothing is launched)
    lib = L.load()
    assert lib.ou_window_gather(x.data_ptr(), 0, 1, 9000, W, W // 2 + 1, 0, 2, W, x.data_ptr(), 0, W, _sp()) != 0
    assert b"overlap" in lib.ou_last_error()
    assert lib.ou_overlap_add(x.data_ptr(), W, 9000, W, O, 3, 2, x.data_ptr(), x.data_ptr(), _sp()) != 0


# ------------------------------------------------------------------ bundle
_CHILD = r'''
import sys
import numpy as np, torch
from open_universe_amd.bundle import Bundle, randn
assert "open_universe_amd.engine" not in sys.modules and "open_universe_amd.plan" not in sys.modules
path, xf, noisef, outf, overlap = sys.argv[1:6]
overlap = int(overlap)
x = torch.from_numpy(np.load(xf)).cuda()
G = torch.from_numpy(np.load(noisef)).cuda()                     # (n_noise, L)
b = Bundle(path)
W, B, Tp, T = b.length, b.batch, b.padded_length, x.numel()
total, Ln = b.long_noise(T, overlap)
assert total == b.n_noise * Ln and G.shape == (b.n_noise, Ln)
res = {}
res["long"] = b.enhance_long_with_noise(x, overlap, G).cpu().numpy()
assert b.status() == 0
# the composition: enhance_with_noise per group of B windows (unused slots repeat the last window)
H = W - overlap
n = 1 + -(-(T - W) // H)
st = [min(i * H, T - W) for i in range(n)]
outs = []
for first in range(0, n, B):
    ss = [st[min(first + k, n - 1)] for k in range(B)]
    mix = torch.stack([x[s:s + W] for s in ss])
    nz = torch.stack([G[:, s:s + Tp] for s in ss], dim=1)
    o = b.enhance_with_noise(mix, nz.contiguous())
    assert b.status() == 0
    outs.extend(o[k].cpu().numpy() for k in range(min(B, n - first)))
res["outs"] = np.stack(outs)
# the native stream: draw k is ou_randn at (seed, counter k ceil(L / 4))
res["seed7"] = b.enhance_long(x, overlap, seed=7).cpu().numpy()
assert b.status() == 0
Gn = torch.stack([randn(Ln, 7, offset=k * ((Ln + 3) // 4)) for k in range(b.n_noise)])
res["seed7_noise"] = b.enhance_long_with_noise(x, overlap, Gn).cpu().numpy()
assert b.status() == 0
res["seed8"] = b.enhance_long(x, overlap, seed=8).cpu().numpy()
assert b.status() == 0
for bad in (x[:W], x[:W - 1]):                                   # n <= W is ou_model_enhance's case
    try:
        b.enhance_long(bad, overlap)
    except Exception as e:
        assert "use ou_model_enhance" in str(e), e
    else:
        raise AssertionError("n <= W was accepted")
b.close()
np.savez(outf, **res)
'''


def test_bundle_enhance_long_in_a_fresh_process(model, tmp_path):
    T = 9000
    x = _clip(T, 2)
    path = str(tmp_path / "b.oub")
    with torch.no_grad():
        ex = Bd.export_bundle(model, path, 2, W, n_steps=N_STEPS, calib=torch.stack([x[:W], x[W:2 * W]]),
                              name="pp16_c4")
    del ex
    G, _, Tp = _global_noise(model, T, 77)
    xf, noisef, outf = (str(tmp_path / n) for n in ("x.npy", "noise.npy", "out.npz"))
    np.save(xf, x.numpy())
    np.save(noisef, G[:, 0, 0].cpu().numpy())
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", _CHILD, path, xf, noisef, outf, str(O)], capture_output=True, text=True,
                       timeout=240, env=env, cwd=ROOT)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    res = np.load(outf)
    assert res["outs"].shape == (3, W) and res["long"].shape == (T,)
    _close("bundle enhance_long", res["long"], _crossfade(res["outs"], T, W, O, np.float64),
           _crossfade(res["outs"], T, W, O, np.float32))
    assert np.array_equal(res["seed7"], res["seed7_noise"])
    assert not np.array_equal(res["seed7"], res["seed8"]) and np.isfinite(res["seed8"]).all()


# ------------------------------------------------------------------ CLI
def test_cli_window_outputs_independent_of_world_size(tmp_path, monkeypatch):
    """Two files, one shorter than the window and one of 9000 samples that
    goes through enhance_long: rank 0 and rank 1 of WORLD_SIZE=2 (both on
    cuda:0 here) together write what the single-rank run writes, bit for bit
    (skip() draws the windowed run's global noise for the other rank's file)."""
    from scipy.io import wavfile

    from open_universe_amd.audio import load_audio
    from open_universe_amd.bin import enhance as cli
    from test_api_surface import _write_ckpt

    ckpt, _, _, _ = _write_ckpt(str(tmp_path), with_ema=False)
    src = tmp_path / "noisy"
    src.mkdir()
    rng = np.random.default_rng(5)
    lens = {"a_long.wav": 9000, "b_short.wav": 3000, "c_long.wav": 4001}
    for name, n in lens.items():
        wavfile.write(src / name, 16000, (rng.standard_normal(n) * 0.1).astype(np.float32))
    common = ["--model", ckpt, "--n_steps", "3", "--seed", "11", "--device", "cuda:0", "--chunk", "2",
              "--window", "0.25", "--overlap", "0.05", "--window-batch", "2"]
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        monkeypatch.delenv(k, raising=False)
    calls = []
    real = UniverseGAN.enhance_long
    monkeypatch.setattr(UniverseGAN, "enhance_long",
                        lambda self, mix, **kw: (calls.append((mix.shape[-1], kw["window"], kw["overlap"], kw["batch"])),
                                                 real(self, mix, **kw))[1])
    assert cli.main([str(src), str(tmp_path / "one")] + common) == 0
    assert sorted(calls) == [(4001, 4000, 800, 2), (9000, 4000, 800, 2)]   # the short file went the existing way
    for r in (0, 1):
        monkeypatch.setenv("RANK", str(r))
        monkeypatch.setenv("LOCAL_RANK", "0")
        monkeypatch.setenv("WORLD_SIZE", "2")
        assert cli.main([str(src), str(tmp_path / "two")] + common) == 0
    for name, n in lens.items():
        a, _ = load_audio(tmp_path / "one" / name)
        b, _ = load_audio(tmp_path / "two" / name)
        assert a.shape[-1] == n and torch.isfinite(a).all() and a.abs().max() > 0
        assert torch.equal(a, b), name
