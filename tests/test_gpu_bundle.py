"""Exported enhance bundles on the GPU: the native noise stream (ou_randn)
against its numpy restatement, and a bundle replayed in a fresh process --
through the ctypes wrapper and through the C++ host example -- against the
recorded plan it was exported from, bit for bit (the same descriptors and
tiles through the same kernels: anything short of equality is a relocation or
initialisation bug)."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import golden_state_dict, load_golden, rel_rms, si_sdr
from open_universe_amd import _lib as L
from open_universe_amd import bundle as Bd
from open_universe_amd.configs import get_config
from open_universe_amd.networks.universe import Universe, UniverseGAN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
CONFIGS = {"pp16_c4": ("pp16", 4), "orig16_c4": ("orig16", 4), "pp24_c4": ("pp24", 4), "pp16": ("pp16", None)}


# ------------------------------------------------------------------ ou_randn
def _philox_np(q, seed):
    """Philox4x32-10 of the counters (q low, q high, 0, 0) under the key
    (seed low, seed high): uint32 (n, 4)."""
    M = np.uint64(0xFFFFFFFF)
    q = np.asarray(q, dtype=np.uint64)
    c = [q & M, q >> np.uint64(32), np.zeros_like(q), np.zeros_like(q)]
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M, (k1 + np.uint64(0xBB67AE85)) & M
    return np.stack(c, axis=1).astype(np.uint32)


def _randn_np(n, seed, offset=0):
    """The documented stream in float64: (z, r) per output."""
    nq = (n + 3) // 4
    x = _philox_np(np.arange(nq, dtype=np.uint64) + np.uint64(offset), seed).astype(np.float64)
    z, rr = np.empty((nq, 4)), np.empty((nq, 4))
    for a in (0, 2):
        u1 = (np.floor(x[:, a] / 256.0) + 1.0) * 2.0**-24
        u2 = np.floor(x[:, a + 1] / 256.0) * 2.0**-24
        r = np.sqrt(-2.0 * np.log(u1))
        z[:, a], z[:, a + 1] = r * np.cos(2 * np.pi * u2), r * np.sin(2 * np.pi * u2)
        rr[:, a] = rr[:, a + 1] = r
    return z.reshape(-1)[:n], rr.reshape(-1)[:n]


def _randn(out, seed, offset=0):
    L.check(L.load().ou_randn(out.data_ptr(), out.numel(), seed, offset,
                              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "randn")
    torch.cuda.synchronize()
    return out


N = 2**20 + 3   # the tail is not a multiple of 4
SEED = 0x1234_5678_9ABC_DEF1


@pytest.fixture(scope="module")
def draw():
    return _randn(torch.empty(N, dtype=torch.float32, device=DEV), SEED).cpu()


def test_randn_is_reproducible_and_offsets_are_slices(draw):
    again = Bd.randn(N, SEED, device=DEV).cpu()
    assert torch.equal(draw, again)
    k = 1237
    part = Bd.randn(N - 4 * k, SEED, offset=k, device=DEV).cpu()
    assert torch.equal(part, draw[4 * k:])
    # an output that is only float-aligned takes the scalar-store kernel: the same values
    buf = torch.empty(N + 1, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    assert torch.equal(_randn(buf[1:], SEED).cpu(), draw)
    assert not torch.equal(Bd.randn(N, SEED + 1, device=DEV).cpu(), draw)


def test_randn_matches_the_numpy_restatement(draw):
    z64, r = _randn_np(N, SEED)
    err = np.abs(draw.numpy().astype(np.float64) - z64)
    bound = 1e-5 * np.maximum(1.0, r)
    print(f"randn: max |z - z64| / bound = {float((err / bound).max()):.3e}")
    assert (err <= bound).all(), float((err / bound).max())


def test_randn_moments(draw):
    z = draw.numpy().astype(np.float64)
    assert np.isfinite(z).all()
    mean, var = z.mean(), z.var()
    print(f"randn: mean {mean:.3e} var - 1 {var - 1:.3e} max |z| {np.abs(z).max():.4f}")
    assert abs(mean) <= 5 / math.sqrt(N)
    assert abs(var - 1) <= 5 * math.sqrt(2 / N)
    assert np.abs(z).max() <= math.sqrt(2 * 24 * math.log(2)) + 1e-3


# ------------------------------------------------------------------ replay
_CHILD = r'''
import sys
import numpy as np, torch
from open_universe_amd.bundle import Bundle
assert "open_universe_amd.engine" not in sys.modules and "open_universe_amd.plan" not in sys.modules
path, mixf, noisef, outf = sys.argv[1:5]
mix = torch.from_numpy(np.load(mixf)).cuda()
noise = torch.from_numpy(np.load(noisef)).cuda()
outs = []
for capture in (True, False):
    b = Bundle(path, capture=capture)
    for _ in range(2):   # twice on one handle: a scratch region that needed zeroing again would show
        o = b.enhance_with_noise(mix, noise)
        assert b.status() == 0
        outs.append(o.cpu().numpy())
    b.close()
np.save(outf, np.stack(outs))
'''


def _child(cmd, timeout):
    """Run a child process under its own time limit; its exit status decides."""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return r


@pytest.fixture(scope="module")
def exported(tmp_path_factory):
    """tag -> the bundle exported from the live model, with the inputs and
    the plan's own result on them (CPU tensors); exported once per tag."""
    cache = {}

    def get(tag):
        if tag in cache:
            return cache[tag]
        name, nch = CONFIGS[tag]
        d = load_golden(tag)
        cfg = get_config(name, nch)
        cls = UniverseGAN if cfg["_target_"].endswith("UniverseGAN") else Universe
        m = cls(**{k: v for k, v in cfg.items() if k != "_target_"})
        m.load_state_dict(golden_state_dict(d), strict=False)
        m = m.to(DEV).eval()
        mix = torch.from_numpy(np.asarray(d["enh_mix"], dtype=np.float32))   # (B, 1, T)
        Bsz, _, T = mix.shape
        path = str(tmp_path_factory.mktemp(tag) / "b.oub")
        with torch.no_grad():
            ex = Bd.export_bundle(m, path, Bsz, T, calib=mix[:, 0], name=tag)
            plan = ex.plan
            # the reference's draws: a CPU generator, x0 first, then one z per step
            g = torch.Generator().manual_seed(1028282)
            noise = torch.stack([torch.randn((Bsz, 1, plan.Tp), generator=g) for _ in range(plan.n_noise)])
            ref = plan.run_with_noise(mix.to(DEV), noise.to(DEV)).clone().cpu()
        cache[tag] = {"path": path, "mix": mix, "noise": noise, "ref": ref, "d": d, "bytes": ex.file_bytes,
                      "dir": os.path.dirname(path)}
        del ex, plan, m
        torch.cuda.empty_cache()
        return cache[tag]

    return get


@pytest.mark.parametrize("tag", list(CONFIGS))
def test_replay_in_a_fresh_process_equals_the_plan(exported, tag):
    e = exported(tag)
    mixf, noisef, outf = (os.path.join(e["dir"], n) for n in ("mix.npy", "noise.npy", "out.npy"))
    np.save(mixf, e["mix"].numpy())
    np.save(noisef, e["noise"].numpy())
    _child([sys.executable, "-c", _CHILD, e["path"], mixf, noisef, outf], timeout=240)
    outs = torch.from_numpy(np.load(outf))   # captured x 2, eager x 2
    assert outs.shape == (4,) + tuple(e["ref"].shape)
    for k, what in enumerate(("captured, first", "captured, second", "eager, first", "eager, second")):
        assert torch.equal(outs[k], e["ref"]), (what, float((outs[k] - e["ref"]).abs().max()))
    want = e["d"]["enh_out"]
    assert math.isfinite(si_sdr(outs[0].numpy(), want))
    if tag == "pp16":   # the existing gate of enhance() against the reference, on the reference's noise
        assert rel_rms(outs[0].numpy(), want) < 1e-3


def test_native_noise_end_to_end(exported):
    e = exported("pp16_c4")
    b = Bd.Bundle(e["path"])
    mix = e["mix"].to(DEV)
    a1 = b.enhance(mix, seed=7).clone()
    assert b.status() == 0
    a2 = b.enhance(mix, seed=7).clone()
    assert b.status() == 0
    c = b.enhance(mix, seed=8).clone()
    assert b.status() == 0
    z = Bd.randn(b.n_noise * b.batch * b.padded_length, 7, device=DEV)
    w = b.enhance_with_noise(mix, z.view(b.n_noise, b.batch, 1, b.padded_length)).clone()
    assert b.status() == 0
    b.close()
    assert torch.equal(a1, a2) and torch.equal(a1, w) and not torch.equal(a1, c)
    assert torch.isfinite(a1).all() and math.isfinite(si_sdr(a1.cpu().numpy(), e["d"]["enh_out"]))
    assert b.info["batch"] == mix.shape[0] and b.info["config"] == "pp16_c4" and b.info["n_steps"] == 8


def test_cpp_host_equals_the_plan(exported):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc is not installed here: the C++ host example cannot be built")
    e = exported("pp16_c4")
    exe = os.path.join(e["dir"], "enhance_host")
    lib_dir = os.path.dirname(L.LIB_PATH)
    r = subprocess.run([HIPCC, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "enhance_host.cpp"), "-o", exe, "-L", lib_dir, "-louhip",
                        "-Wl,-rpath," + lib_dir], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    mixf, noisef, outf = (os.path.join(e["dir"], n) for n in ("mix.f32", "noise.f32", "out.f32"))
    e["mix"].numpy().astype("<f4").tofile(mixf)
    e["noise"].numpy().astype("<f4").tofile(noisef)
    _child([exe, e["path"], mixf, outf, noisef], timeout=120)
    out = torch.from_numpy(np.fromfile(outf, dtype="<f4").reshape(e["ref"].shape))
    assert torch.equal(out, e["ref"]), float((out - e["ref"]).abs().max())
