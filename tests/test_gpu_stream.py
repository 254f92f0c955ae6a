"""The streaming enhance on the GPU: the two kernels of
csrc/ou_stream.hip on their own, the bundle session (ou_model_stream_*) in a
fresh process, ``Universe.stream``, the CLI on a pipe and the C++ example.

Everything here is bit for bit.  The invariant: for every length ``T >= W``
and every way of cutting the pushes, the concatenated output of a stream
equals the windowed enhance of the whole clip (ou_overlap_add over the
windows' outputs, the windows run in groups of ``B``) on noise rows
materialised by ou_randn -- draw ``k`` at ``(seed, offset + k 2^38)``.  The
starts and the window count are written out here from the formulas of section
14; nothing is imported from longform.py."""
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
HIPCC = "/opt/rocm/bin/hipcc"
F32 = torch.float32
W = 4000
POISON = 1e6
N_STEPS = 3
DRAW = 2**38


def _starts(T, Wn, On):
    H = Wn - On
    n = 1 if T <= Wn else 1 + -(-(T - Wn) // H)
    return [min(i * H, T - Wn) for i in range(n)]


def _sp():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _fade(On):
    u = np.arange(On, dtype=np.float64)
    f = np.sin(np.pi * (2 * u + 1) / (4 * max(On, 1))) ** 2
    return torch.from_numpy(np.stack([f, 1 - f]).astype(np.float32)).to(DEV) if On else None   # [2][O], f then 1 - f


# ------------------------------------------------------------------ ou_stream_gather
def _gather_case(On, Tp, fed, first, count, slots, closing, seed, offset, gap):
    """One call on a ring of W + 2 H samples that holds the last samples of a
    signal of ``fed``: MIX against the un-wrapped signal, NZ against ou_randn
    rows of start + Tp values sliced at start, poison around the rows."""
    lib = L.load()
    H, rows = W - On, 3
    cap = W + 2 * H
    x = torch.randn(fed, generator=torch.Generator().manual_seed(fed + On)).to(DEV)
    ring = torch.full((cap,), POISON, dtype=F32, device=DEV)
    p = torch.arange(max(0, fed - cap), fed, device=DEV)
    ring[p % cap] = x[p]
    mbs, nbs = W + gap, Tp + gap
    nrs = slots * nbs + 5
    mix = torch.full((slots * mbs + 3,), POISON, dtype=F32, device=DEV)
    nz = torch.full((rows * nrs + 3,), POISON, dtype=F32, device=DEV)
    L.check(lib.ou_stream_gather(ring.data_ptr(), cap, max(0, fed - cap), fed, W, On, first, count, slots, closing,
                                 fed if closing else 0, rows, Tp, seed, offset, mix.data_ptr(), mbs, nz.data_ptr(), nrs,
                                 nbs, _sp()), "stream_gather")
    want_mix, want_nz = torch.full_like(mix, POISON), torch.full_like(nz, POISON)
    residues = set()
    for b in range(slots):
        i = first + min(b, count - 1)
        s = min(i * H, fed - W) if closing and i == first + count - 1 else i * H
        residues.add(s % 4)
        want_mix[b * mbs:b * mbs + W] = x[s:s + W]
        for k in range(rows):
            row = Bd.randn(s + Tp, seed, (offset + k * DRAW) % 2**64, device=DEV)
            want_nz[k * nrs + b * nbs:k * nrs + b * nbs + Tp] = row[s:]
    torch.cuda.synchronize()
    assert torch.equal(mix, want_mix), (On, Tp, fed, first)
    assert torch.equal(nz, want_nz), (On, Tp, fed, first, (nz != want_nz).nonzero()[:4].tolist())
    return residues


@pytest.mark.parametrize("On", [800, 801, 0])
@pytest.mark.parametrize("Tp,gap", [(4160, 0), (4163, 0), (4160, 36), (4163, 1)])
def test_stream_gather_is_bit_exact(On, Tp, gap):
    """With O = 801 the hop is odd, so the regular starts have every residue
    mod 4; the shifted last window of a closing call brings the others for
    O = 800 and O = 0.  The ring wraps from the second group on."""
    H = W - On
    seen = set()
    for first in range(4):   # regular windows [first, first + 2)
        seen |= _gather_case(On, Tp, (first + 1) * H + W, first, 2, 2, 0, 7 + first, first * 1000, gap)
    for d in range(1, 5):    # closing: window 2 shifted back to T - W = 2 H - d; the third slot repeats it
        seen |= _gather_case(On, Tp, 2 * H + W - d, 1, 2, 3, 1, 2**40 + d, 2**64 - 3, gap)
    seen |= _gather_case(On, Tp, W, 0, 1, 2, 1, 3, 5, gap)   # T = W: the one window and its copy
    assert seen == {0, 1, 2, 3}


# ------------------------------------------------------------------ ou_stream_overlap_add
def _stream_overlap_add(dw, T, On, B, tab, misalign):
    """The calls a stream of T samples makes at group size B; returns the
    concatenation of what they emit (on the CPU) and the per-call counts."""
    lib = L.load()
    H, bs = W - On, dw.stride(0)
    n = len(_starts(T, W, On))
    ready = (T - W) // H + 1          # regular windows complete before close
    run = ready // B * B
    buf = torch.full((T + 8,), POISON, dtype=F32, device=DEV)
    y = buf[misalign:misalign + T]
    carry = torch.full((max(On, 1) + 2,), float("nan"), dtype=F32, device=DEV)
    got, counts = ctypes.c_int64(-1), []
    tp, cp = (tab.data_ptr(), carry.data_ptr()) if On else (0, 0)
    for first in range(0, run, B):
        L.check(lib.ou_stream_overlap_add(dw[first].data_ptr(), bs, W, On, first, B, 0, 0, tp, cp,
                                          y[first * H:].data_ptr(), ctypes.byref(got), _sp()), "stream_overlap_add")
        counts.append(got.value)
    L.check(lib.ou_stream_overlap_add(dw[run].data_ptr() if run < n else 0, bs, W, On, run, n - run, 1, T, tp, cp,
                                      y[run * H:].data_ptr() if run * H < T else 0, ctypes.byref(got), _sp()),
            "stream_overlap_add")
    counts.append(got.value)
    torch.cuda.synchronize()
    assert (buf[:misalign] == POISON).all() and (buf[misalign + T:] == POISON).all()
    assert torch.isnan(carry[max(On, 1):]).all()
    assert counts[:-1] == [B * H] * (run // B) and sum(counts) == T
    return y.cpu(), n - run


@pytest.mark.parametrize("On", [800, 801, 0, 2000])
def test_stream_overlap_add_emits_the_bits_of_overlap_add(On):
    lib = L.load()
    tab = _fade(On)
    closed_from_the_carry = set()
    for T in (4000, 4001, 9000, 9001, 10400, 13600):
        n = len(_starts(T, W, On))
        g = torch.Generator().manual_seed(7 * T + On)
        dw = torch.randn(n, W + 8, generator=g).to(DEV)[:, :W]
        ref = torch.full((T,), POISON, dtype=F32, device=DEV)
        L.check(lib.ou_overlap_add(dw.data_ptr(), dw.stride(0), T, W, On, 0, n, tab.data_ptr() if On else 0,
                                   ref.data_ptr(), _sp()), "overlap_add")
        ref = ref.cpu()
        for B in (1, 2, 3):
            y, left = _stream_overlap_add(dw, T, On, B, tab, (T + B) % 4)
            assert torch.equal(y, ref), (T, On, B, (y != ref).nonzero()[:4].tolist())
            if left == 0:
                closed_from_the_carry.add((T, B))
    if On == 800:   # 13600 = 3 H + W: four regular windows, so B = 2 (and 1) close from the carry alone
        assert (13600, 2) in closed_from_the_carry and (10400, 3) in closed_from_the_carry


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


@pytest.fixture(scope="module")
def exported(model, tmp_path_factory):
    """The (2, 4000) bundle of tests/test_gpu_long.py."""
    path = str(tmp_path_factory.mktemp("stream") / "b.oub")
    x = _clip(2 * W, 2)
    with torch.no_grad():
        ex = Bd.export_bundle(model, path, 2, W, n_steps=N_STEPS, calib=torch.stack([x[:W], x[W:]]), name="pp16_c4")
    del ex
    return path


# ------------------------------------------------------------------ the bundle session
_CHILD = r'''
import ctypes, sys
import numpy as np, torch
from open_universe_amd import _lib as L
from open_universe_amd.bundle import Bundle, randn
from open_universe_amd.longform import StreamShort
assert "open_universe_amd.engine" not in sys.modules and "open_universe_amd.plan" not in sys.modules
path, xf, outf, overlap = sys.argv[1:5]
O = int(overlap)
xs = torch.from_numpy(np.load(xf)).cuda()
b = Bundle(path)
W, B, Tp = b.length, b.batch, b.padded_length
H = W - O
SEED, OFF = 7, 11
ring = W + B * H

def stream(x, cuts, seed=SEED):
    """Push x in pieces of the given sizes (the last entry repeats), close; bound() checked on every call."""
    outs, at, k = [], 0, 0
    with b.stream(O, seed=seed, offset=OFF) as s:
        while at < x.numel():
            n = min(cuts[min(k, len(cuts) - 1)], x.numel() - at)
            want = s.bound(n)
            y = s.push(x[at:at + n] if k % 2 else x[at:at + n].cpu())   # device and CPU tensors go in
            assert y.is_cuda and y.numel() == want, (y.numel(), want)
            assert b.status() == 0
            outs.append(y)
            at, k = at + n, k + 1
        want = s.bound(closing=True)
        y = s.close()
        assert y.numel() == want and b.status() == 0
        assert s.bound(5) == 0
        outs.append(y)
    return torch.cat(outs)

res = {}
assert ring + 1000 + 5 < 13600
for T in (9001, 10400, 13600):
    x = xs[:T]
    n = 1 + -(-(T - W) // H)
    Ln = min((n - 1) * H, T - W) + Tp
    total, ln = b.long_noise(T, O)
    assert ln == Ln
    G = torch.stack([randn(Ln, SEED, OFF + k * 2**38) for k in range(b.n_noise)])
    ref = b.enhance_long_with_noise(x, O, G)
    assert b.status() == 0
    outs = {"all": stream(x, [T]), "one": stream(x, [1, T]), "1234": stream(x, [1234]),
            "big": stream(x, [5, ring + 1000, 777])}   # at 13600 samples: one push larger than the ring
    for name, y in outs.items():
        assert y.shape == ref.shape and torch.equal(y, ref), (T, name, float((y - ref).abs().max()))
    other = stream(x, [T], seed=8)
    assert torch.isfinite(other).all() and not torch.equal(other, ref)
    res[f"y{T}"] = ref.cpu().numpy()

# T = W: the one window in slot 0, the other slots its copies
x = xs[:W]
nz = torch.stack([randn(Tp, SEED, OFF + k * 2**38) for k in range(b.n_noise)])        # (n_noise, Tp)
one = b.enhance_with_noise(torch.stack([x] * B), nz[:, None, :].repeat(1, B, 1).contiguous())[0].clone()
assert b.status() == 0
assert torch.equal(stream(x, [W]), one) and torch.equal(stream(x, [999]), one)

# T = W - 1: close fails with its own code, the session stays valid and can be destroyed
s = b.stream(O, seed=SEED)
assert s.push(xs[:W - 1]).numel() == 0
try:
    s.close()
except StreamShort as e:
    assert "shorter than one window" in str(e)
else:
    raise AssertionError("a stream shorter than one window was closed")
got = ctypes.c_int64(0)
assert b.lib.ou_model_stream_close(s.h, 0, ctypes.byref(got), None) == L.STREAM_SHORT == 3
assert s.push(xs[W - 1:W]).numel() == 0 and s.close().numel() == W   # still valid: one more sample makes a window
assert b.status() == 0

# one session at a time; enhance* is refused while it is open
for call in (lambda: b.stream(O), lambda: b.enhance(torch.stack([x] * B)), lambda: b.enhance_long(xs[:9001], O)):
    try:
        call()
    except L.OuHipError as e:
        assert "session" in str(e), e
    else:
        raise AssertionError("accepted while a session is open")
s.release()
b.stream(O).release()                     # and again once it is gone
assert torch.equal(b.enhance(torch.stack([x] * B), seed=1), b.enhance(torch.stack([x] * B), seed=1))
for bad in (W // 2 + 1, -1):
    try:
        b.stream(bad)
    except L.OuHipError as e:
        assert "overlap" in str(e)
    else:
        raise AssertionError("overlap accepted")
b.close()
np.savez(outf, **res)
'''


def _run_child(argv, timeout=240):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(argv, capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return r


def test_bundle_stream_in_a_fresh_process(exported, tmp_path):
    """Every way of cutting the pushes gives ou_model_enhance_long_noise on the
    whole clip, on noise from ou_randn at (seed, offset + k 2^38)."""
    xf, outf = str(tmp_path / "x.npy"), str(tmp_path / "out.npz")
    np.save(xf, _clip(13600, 5).numpy())
    _run_child([sys.executable, "-c", _CHILD, exported, xf, outf, "800"])
    res = np.load(outf)
    for T in (9001, 10400, 13600):
        y = res[f"y{T}"]
        assert y.shape == (T,) and np.isfinite(y).all() and np.abs(y).max() > 1e-3


def test_cpp_stream_host_equals_the_python_session(exported, tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc is not installed here: the C++ host example cannot be built")
    exe = str(tmp_path / "stream_host")
    lib_dir = os.path.dirname(L.LIB_PATH)
    r = subprocess.run([HIPCC, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "stream_host.cpp"), "-o", exe, "-L", lib_dir, "-louhip",
                        "-Wl,-rpath," + lib_dir], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    T, O = 10401, 800
    x = _clip(T, 6)
    inf, outf = str(tmp_path / "in.f32"), str(tmp_path / "out.f32")
    x.numpy().astype("<f4").tofile(inf)
    _run_child([exe, exported, inf, outf, "1777", str(O), "--seed", "9"], timeout=120)
    out = torch.from_numpy(np.fromfile(outf, dtype="<f4"))
    b = Bd.Bundle(exported)
    with b.stream(O, seed=9) as s:
        want = torch.cat([s.push(x), s.close()]).cpu()
        assert b.status() == 0
    b.close()
    assert out.shape == want.shape == (T,) and torch.equal(out, want)
    # shorter than one window: a clear error and a non-zero exit
    x[:W - 1].numpy().astype("<f4").tofile(inf)
    env = dict(os.environ)
    r = subprocess.run([exe, exported, inf, outf, "1777", str(O)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 1 and "shorter than one window" in r.stderr


# ------------------------------------------------------------------ Universe.stream
def _reference(model, x, On, B, keep_rms, seed, offset):
    """The definition: the windows through plan.run_with_noise in groups of B
    (unused slots repeat the last window) on noise materialised by ou_randn,
    then ou_overlap_add.  Returns (y, the plan, its key)."""
    lib = L.load()
    T = x.numel()
    st = _starts(T, W, On)
    n = len(st)
    with torch.no_grad():
        model.enhance(torch.stack([x[:W]] * B), n_steps=N_STEPS, keep_rms=keep_rms,
                      rng=torch.Generator(device=DEV).manual_seed(1))
        key, _ = model._plan_spec(B, W, N_STEPS, model.diff_kwargs.epsilon, keep_rms)
        plan = model._plans[key]
        Tp = plan.Tp
        G = torch.stack([Bd.randn(st[-1] + Tp, seed, offset + k * DRAW, device=DEV) for k in range(N_STEPS)])
        outs = torch.empty(n, W, dtype=F32, device=DEV)
        for first in range(0, n, B):
            ss = [st[min(first + b, n - 1)] for b in range(B)]
            mix = torch.stack([x[s:s + W] for s in ss])[:, None, :].contiguous()
            nz = torch.stack([G[:, s:s + Tp] for s in ss], dim=1)[:, :, None, :].contiguous()
            out = plan.run_with_noise(mix, nz)
            outs[first:first + B] = out[:min(B, n - first)]
        y = torch.full((T,), POISON, dtype=F32, device=DEV)
        tab = _fade(On)
        L.check(lib.ou_overlap_add(outs.data_ptr(), W, T, W, On, 0, n, tab.data_ptr() if On else 0, y.data_ptr(),
                                   _sp()), "overlap_add")
        torch.cuda.synchronize()
    return y, plan, key


def _push_all(s, x, cuts):
    outs, at = [], 0
    for k, n in enumerate(cuts):
        piece = x[at:at + n]
        want = s.bound(n)
        y = s.push(piece.cpu() if k % 2 else piece)
        assert y.is_cuda and y.numel() == want
        outs.append(y)
        at += n
    assert at == x.numel()
    want = s.bound(closing=True)
    outs.append(s.close())
    assert outs[-1].numel() == want
    return torch.cat(outs)


@pytest.mark.parametrize("batch", [1, 2])
@pytest.mark.parametrize("keep_rms", [False, True])
def test_universe_stream_is_the_composition(model, batch, keep_rms):
    T, On, seed, offset = 9001, 800, 21, 1 << 33
    x = _clip(T, 4).to(DEV)
    ref, plan, key = _reference(model, x, On, batch, keep_rms, seed, offset)
    assert ref.abs().max() > 1e-3
    n_plans = len(model._plans)
    with model.stream(W, On, batch=batch, n_steps=N_STEPS, keep_rms=keep_rms, seed=seed, offset=offset) as s:
        y = _push_all(s, x, [1, 3999, 17, 3183, 1801])     # ragged: a window completes inside, at and after a push
    assert y.shape == (T,) and torch.equal(y, ref), float((y - ref).abs().max())
    assert len(model._plans) == n_plans and model._plans[key] is plan   # no plan beyond the (B, W) one
    with model.stream(W, On, batch=batch, n_steps=N_STEPS, keep_rms=keep_rms, seed=seed + 1, offset=offset) as s:
        assert not torch.equal(_push_all(s, x, [T]), ref)


def test_evicting_the_plan_between_pushes_changes_nothing(model, monkeypatch):
    T, On = 9001, 800
    x = _clip(T, 4).to(DEV)
    ref, _, key = _reference(model, x, On, 1, False, 5, 0)
    monkeypatch.setenv("OUHIP_MAX_PLANS", "1")
    with model.stream(W, On, batch=1, n_steps=N_STEPS, seed=5) as s, torch.no_grad():
        a = s.push(x[:5000])
        assert a.numel() == 3200
        model.enhance(x[:3000], n_steps=N_STEPS)      # records another length: the LRU of one entry drops the plan
        assert key not in model._plans
        b = s.push(x[5000:])
        c = s.close()
    assert torch.equal(torch.cat([a, b, c]), ref)


def test_universe_stream_refusals(model):
    for kw in ({"target": torch.zeros(1)}, {"use_aux_signal": True}, {"ensemble": 2}, {"warm_start": 1}):
        with pytest.raises(NotImplementedError):
            model.stream(W, 800, **kw)
    with pytest.raises(TypeError):
        model.stream(W, 800, windows=3)
    for bad in ((W, W // 2 + 1, 1), (W, -1, 1), (0, 0, 1), (W, 800, 0)):
        with pytest.raises(ValueError):
            model.stream(bad[0], bad[1], batch=bad[2])
    from open_universe_amd.longform import StreamShort

    with model.stream(W, 800, n_steps=N_STEPS) as s:
        assert s.push(_clip(W - 1)).numel() == 0
        with pytest.raises(StreamShort):
            s.close()
        # the session stayed valid: one more sample completes window 0 (batch 1), whose tail waits for close
        assert s.push(_clip(1)).numel() == W - 800 and s.close().numel() == 800


# ------------------------------------------------------------------ the CLI
@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    from test_api_surface import _write_ckpt

    return _write_ckpt(str(tmp_path_factory.mktemp("stream_ckpt")), with_ema=False)[0]


def _cli(ckpt, data, *extra, expect=0):
    # OUHIP_AUTOTUNE=0: the tuner picks tiles by timing them, so two processes may pick different ones and then
    # differ in the last bits; without it the tiles are a function of the shapes alone
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), OUHIP_AUTOTUNE="0")
    cmd = [sys.executable, "-m", "open_universe_amd.bin.enhance_stream", "--model", ckpt, "--n_steps", str(N_STEPS),
           "--window", "0.25", "--overlap", "0.05", "--seed", "11", "--device", DEV, "--chunk", "0.0817", *extra]
    r = subprocess.run(cmd, input=data, capture_output=True, timeout=240, env=env, cwd=ROOT)   # stdin is a pipe
    assert (r.returncode == 0) == (expect == 0), (r.returncode, r.stderr[-3000:])
    return r


@pytest.mark.parametrize("fmt,batch", [("s16le", 2), ("f32le", 1)])
def test_cli_on_a_pipe_equals_universe_stream(ckpt, fmt, batch, monkeypatch):
    from open_universe_amd import inference_utils
    from open_universe_amd.bin import enhance_stream as cli

    T = 9001
    x = (_clip(T, 8) * 0.5).numpy()
    data = cli.encode(x, fmt)
    r = _cli(ckpt, data, "--format", fmt, "--window-batch", str(batch), "--rate", "16000")   # 1307 samples per read
    monkeypatch.setenv("OUHIP_AUTOTUNE", "0")   # as the subprocess: this model's engine records without the tuner
    tuner = L.TUNER
    try:
        m = inference_utils.load_model(ckpt, device=DEV)
        with m.stream(W, 800, batch=batch, n_steps=N_STEPS, seed=11) as s, torch.no_grad():
            want = torch.cat([s.push(torch.from_numpy(cli.decode(data, fmt))), s.close()]).cpu().numpy()
    finally:
        L.TUNER = tuner   # the engines of the other tests keep theirs
    assert want.shape == (T,) and np.abs(want).max() > 1e-3
    assert r.stdout == cli.encode(want, fmt)


@pytest.mark.parametrize("what", ["rate", "short"])
def test_cli_refusals_exit_non_zero(ckpt, what):
    x = _clip(W - 1, 8).numpy().astype("<f4").tobytes()
    if what == "rate":
        r = _cli(ckpt, x, "--rate", "8000", expect=1)
        assert b"16000" in r.stderr and r.stdout == b""
    else:
        r = _cli(ckpt, x, expect=1)
        assert b"shorter than one window" in r.stderr and r.stdout == b""
