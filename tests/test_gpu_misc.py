"""The small kernels of csrc/ou_misc.hip on the GPU, each launched on its own
through the C ABI and compared with a plain float64 restatement:

  ou_embed, ou_head, ou_snake_aa (descriptors, L.run_now) and ou_normalize,
  ou_inv_rms, ou_rms, ou_power, ou_pad, ou_scale, ou_finish (ctypes entry
  points, as utils/stats.py calls its kernels).

The whole-network tests reach these ops only at a few aligned lengths and one
set of weights, at rel-RMS 1e-4 .. 1e-3.  Here every code path of each kernel
gets its own shape: the float4 / unrolled / scalar-tail loops of the
reductions at misaligned bases, the window of ou_finish inside a strided
buffer, both embeddings at ragged sizes, the head at channel counts off its
8-channel load group and at T == 1, Snake across its 256-sample tile seam.

Inputs are seeded generators only.  Tolerances come from ``_close`` (the
reference's own float32 error on the same inputs); ops whose arithmetic is
fully determined are compared bit for bit.  Descriptors the entry points must
refuse are checked on the CPU (tests/emu/misc_emu.cpp), never sent to a device.
"""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from open_universe_amd import _lib as L
from open_universe_amd import dsp
from oracle import ou_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
LENS = [1, 3, 4, 1023, 4099, 16391]   # < one float4; scalar tail only; one float4; < one pass of 1024 threads;
                                      # the single-float4 loop + 3-sample tail; the 4x-unrolled loop + tail
POISON = 1e6                          # fills whatever lies outside an item's window


def f32(v):
    """The float32 value a c_float field holds, as a Python float."""
    return float(np.float32(v))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _close(what, got, ref64, ref32, factor=4):
    """Assert max|got - ref64| <= factor * max(max|ref32 - ref64|, 2^-23 max|ref64|).

    The yardstick is the error of the same restatement evaluated in float32
    on the CPU, on the same inputs: what float32 arithmetic costs for this
    operation at this conditioning.  The factor 4 allows for a different but
    legitimate summation order and the device's sinf / expf.  The floor is
    one float32 ulp of the largest output, for the cases where the float32
    restatement happens to be exact.  Prints the measured ratio and returns
    the bound."""
    got = got.detach().cpu().to(F64)
    ref64 = ref64.to(F64).reshape(got.shape)
    ref32 = ref32.to(F64).reshape(got.shape)
    assert torch.isfinite(got).all(), what
    err = (got - ref64).abs().max().item()
    yard = max((ref32 - ref64).abs().max().item(), 2.0 ** -23 * ref64.abs().max().item())
    ratio = err / yard if yard > 0 else (0.0 if err == 0 else math.inf)
    print(f"misc-ratio {what} err {err:.3e} yardstick {yard:.3e} ratio {ratio:.3f}")
    assert err <= factor * yard, f"{what}: err {err:.3e} > {factor} x {yard:.3e} (ratio {ratio:.2f})"
    return factor * yard


def _strided(items, bstride, left=0):
    """items (B, n) placed at [left, left + n) of rows of ``bstride`` floats;
    every other float is POISON.  Returns the device buffer."""
    B, n = items.shape
    buf = torch.full((B, bstride), POISON, dtype=F32)
    buf[:, left:left + n] = items
    return buf.to(DEV)


# ------------------------------------------------------------------ reductions
def _normalize(x, level, eps):
    """utils/norm.py:47-87 (norm 2, zero mean): two-pass unbiased std; a
    single sample has variance 0 (the kernel's n > 1 ? n - 1 : 1)."""
    n = x.shape[-1]
    mean = x.mean(dim=-1, keepdim=True)
    ss = ((x - mean) ** 2).sum(dim=-1, keepdim=True)
    std = (ss / max(n - 1, 1)).sqrt()
    return (x - mean) * (level / std.clamp(min=eps))


def _run_normalize(x, level, eps):
    B, n = x.shape
    xd = x.to(DEV).contiguous()
    yd = torch.full((B, n), POISON, dtype=F32, device=DEV)
    L.check(L.load().ou_normalize(xd.data_ptr(), yd.data_ptr(), B, n, level, eps, _stream()), "normalize")
    torch.cuda.synchronize()
    return yd.cpu()


LEVEL, EPS = f32(10 ** (-26.0 / 20.0)), f32(1e-5)


@pytest.mark.parametrize("n", LENS)
def test_normalize_gaussian(n):
    """A plain Gaussian at every reduction path; the second item's base is
    misaligned whenever n is odd."""
    x = torch.randn(2, n, generator=_gen(100 + n)) * 0.3 + 0.05
    got = _run_normalize(x, LEVEL, EPS)
    ref64, ref32 = _normalize(x.double(), LEVEL, EPS), _normalize(x, LEVEL, EPS)
    if n > 1:   # the restatement is the oracle's normalize_batch (torch.std) where that is defined
        o64, _ = O.normalize_batch(x.double()[:, None, :], None, level_db=-26.0, eps=EPS)
        assert torch.allclose(o64[:, 0], ref64, rtol=1e-6, atol=0)
        _close(f"normalize[gauss n={n}]", got, ref64, ref32)
    else:
        assert torch.equal(got, torch.zeros(2, 1)), got


def test_normalize_large_mean():
    """Mean 10, standard deviation 0.01: a one-pass variance (E[x^2] - mean^2)
    loses every digit of it in float32."""
    n = 4099
    x = 10.0 + 0.01 * torch.randn(2, n, generator=_gen(7))
    got = _run_normalize(x, LEVEL, EPS)
    _close("normalize[mean 10 std 0.01]", got, _normalize(x.double(), LEVEL, EPS), _normalize(x, LEVEL, EPS))


def test_normalize_constant_takes_the_eps_clamp():
    """A constant 0.5 at n = 1024: the sum is exact, so the output is exactly
    0 -- and finite, through level / max(0, eps)."""
    got = _run_normalize(torch.full((2, 1024), 0.5), LEVEL, EPS)
    assert torch.equal(got, torch.zeros(2, 1024))


def _rms_ref(x, denom, eps, inverse):
    r = ((x * x).sum(dim=-1) / denom).sqrt()
    return 1.0 / r.clamp(min=eps) if inverse else r


def _run_rms(x, denom=None, eps=0.0):
    B, n = x.shape
    xd = x.to(DEV).contiguous()
    out = torch.full((B,), POISON, dtype=F32, device=DEV)
    lib = L.load()
    if denom is None:
        L.check(lib.ou_rms(xd.data_ptr(), out.data_ptr(), B, n, _stream()), "rms")
    else:
        L.check(lib.ou_inv_rms(xd.data_ptr(), out.data_ptr(), B, n, denom, eps, _stream()), "inv_rms")
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("n", LENS)
def test_rms(n):
    x = torch.randn(2, n, generator=_gen(200 + n)) * 0.7
    _close(f"rms[n={n}]", _run_rms(x), _rms_ref(x.double(), float(n), 0.0, False), _rms_ref(x, float(n), 0.0, False))


def test_rms_of_silence_is_zero():
    assert torch.equal(_run_rms(torch.zeros(2, 1023)), torch.zeros(2))


@pytest.mark.parametrize("n", LENS)
def test_inv_rms(n):
    """The mel path passes its own denominator (frames, not elements)."""
    x = torch.randn(2, n, generator=_gen(300 + n)) * 0.7
    denom = 7.0
    _close(f"inv_rms[n={n}]", _run_rms(x, denom, EPS), _rms_ref(x.double(), denom, EPS, True),
           _rms_ref(x, denom, EPS, True))


def test_inv_rms_of_silence_is_one_over_eps():
    z = torch.zeros(2, 4099)
    _close("inv_rms[zeros]", _run_rms(z, 7.0, EPS), _rms_ref(z.double(), 7.0, EPS, True), _rms_ref(z, 7.0, EPS, True))


# ------------------------------------------------------------------ finish
def _finish(xw, mix_rms):
    """universe.py:349-357 on the cropped window xw (B, len): keep_rms
    rescale by mix_rms / max(rms, 1e-5), then divide by the peak when it
    exceeds 1."""
    v = xw
    if mix_rms is not None:
        xr = (xw * xw).mean(dim=-1).sqrt().clamp(min=f32(1e-5))
        v = xw * (mix_rms / xr)[:, None]
    peak = v.abs().max(dim=-1, keepdim=True).values
    return torch.where(peak > 1.0, v / peak, v)


FINISH_REGIMES = ["copy", "peak", "rms_up", "rms_down"]


@pytest.mark.parametrize("n", LENS)
@pytest.mark.parametrize("left", [0, 1, 2, 3, 5])
@pytest.mark.parametrize("regime", FINISH_REGIMES)
def test_finish(regime, left, n):
    """The window [left, left + n) of rows of left + n + 7 floats; everything
    outside it is 1e6, so a read outside the window shows in the RMS or the
    peak.  The largest sample sits at the end of item 0's window (the scalar
    tail of the reductions) and at the start of item 1's.
      copy      no mix_rms, peak < 1: a bit-exact copy
      peak      no mix_rms, peak 2.5: divided by the peak
      rms_up    mix_rms 2: the rescaled peak (>= 2, the crest factor is >= 1) is divided out
      rms_down  mix_rms 0.1: the rescaled peak (0.1 x a crest factor below 2 for this input) is kept"""
    B = 2
    g = _gen(1000 * left + n)
    w = (torch.rand(B, n, generator=g) * 2 - 1) * 0.9
    top = 2.5 if regime == "peak" else 0.95
    w[0, n - 1], w[1, 0] = -top, top
    mix = {"rms_up": torch.tensor([2.0, 3.0]), "rms_down": torch.tensor([0.1, 0.15])}.get(regime)
    bs = left + n + 7
    xd = _strided(w, bs, left)
    yd = torch.full((B, n), POISON, dtype=F32, device=DEV)
    md = mix.to(DEV) if mix is not None else None
    L.check(L.load().ou_finish(xd.data_ptr(), bs, left, yd.data_ptr(), B, n, md.data_ptr() if md is not None else 0,
                               _stream()), "finish")
    torch.cuda.synchronize()
    got = yd.cpu()
    if regime == "copy":
        assert torch.equal(got, w)
        return
    ref64 = _finish(w.double(), mix.double() if mix is not None else None)
    ref32 = _finish(w, mix)
    bound = _close(f"finish[{regime} left={left} n={n}]", got, ref64, ref32)
    out_peak = got.abs().max(dim=-1).values.double()
    if regime in ("peak", "rms_up"):
        assert (ref64.abs().max(dim=-1).values == 1.0).all()   # the regime is the intended one
        assert ((out_peak - 1.0).abs() <= bound).all(), out_peak
    else:
        assert (out_peak < 1.0).all(), out_peak


# ------------------------------------------------------------------ elementwise
def test_power():
    """|STFT|^2 from [B][2][nf][frames]: real rows of magnitude ~1, imaginary
    rows ~10, so a swapped stride shows.  The device may contract the products
    into an FMA: tolerance, not equality."""
    B, nf, fr = 2, 5, 7
    g = _gen(5)
    x = torch.randn(B, 2, nf, fr, generator=g)
    x[:, 1] *= 10.0
    xd = x.to(DEV).contiguous()
    yd = torch.full((B, nf, fr), POISON, dtype=F32, device=DEV)
    L.check(L.load().ou_power(xd.data_ptr(), yd.data_ptr(), B, nf, fr, _stream()), "power")
    torch.cuda.synchronize()
    ref = lambda v: v[:, 0] ** 2 + v[:, 1] ** 2
    _close("power", yd, ref(x.double()), ref(x))


@pytest.mark.parametrize("n_in,n_out,left", [(5, 16, 0), (5, 16, 4), (5, 16, 11), (300, 513, 100)])
def test_pad(n_in, n_out, left):
    """Bit-exact, zeros included; the input rows are n_in + 3 apart."""
    B = 2
    x = torch.randn(B, n_in, generator=_gen(n_out + left))
    xd = _strided(x, n_in + 3)
    yd = torch.full((B, n_out), POISON, dtype=F32, device=DEV)
    L.check(L.load().ou_pad(xd.data_ptr(), n_in + 3, yd.data_ptr(), B, n_in, n_out, left, _stream()), "pad")
    torch.cuda.synchronize()
    ref = torch.zeros(B, n_out)
    ref[:, left:left + n_in] = x
    assert torch.equal(yd.cpu(), ref)


@pytest.mark.parametrize("with_add", [False, True])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_scale(n, with_add):
    """y = z * s (+ add), the sum of a separately rounded product: bit-exact
    against float32.  (The plans never alias y to add -- EnhancePlan writes X
    from NZ and SIG -- so that case is not part of the contract.)"""
    g = _gen(n)
    z, add = torch.randn(n, generator=g), torch.randn(n, generator=g)
    s = f32(0.3)
    zd, ad = z.to(DEV), add.to(DEV)
    yd = torch.full((n + 1,), POISON, dtype=F32, device=DEV)   # one float past the end: must stay
    L.check(L.load().ou_scale(zd.data_ptr(), yd.data_ptr(), n, s, ad.data_ptr() if with_add else 0, _stream()),
            "scale")
    torch.cuda.synchronize()
    ref = z * torch.tensor(s, dtype=F32)
    if with_add:
        ref = add + ref
    got = yd.cpu()
    assert torch.equal(got[:n], ref)
    assert got[n].item() == POISON


# ------------------------------------------------------------------ embedding
def _sigmas(n):
    return torch.tensor([1e-4, 1e-2, 1.0] if n == 3 else [0.03], dtype=F32)


def _run_embed(d, n, rows, dim):
    out = torch.full((n, rows), POISON, dtype=F32, device=DEV)
    gbuf = torch.full((n, dim), POISON, dtype=F32, device=DEV)
    d.out, d.gbuf = out.data_ptr(), gbuf.data_ptr()
    L.run_now(L.OP_EMBED, d, _stream())
    torch.cuda.synchronize()
    return out.cpu(), gbuf.cpu()


def _proj(rows, dim, g):
    return torch.randn(rows, dim, generator=g) / math.sqrt(dim), torch.randn(rows, generator=g)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("rows", [1, 6, 64])
@pytest.mark.parametrize("dim", [64, 96, 512])
def test_embed_simple_time_embedding(dim, rows, n):
    """kind 0 (sigma_block.py:73-78): [sin | cos](2 pi f k), f = sigmoid(w
    log10 sigma + b) / 2, then every FiLM projection.  rows off the 4 rows a
    workgroup projects, dim off the 64 lanes of a wave.

    The projection of the single-output case (rows = 1, n = 1) takes the
    factor 16: measured 8.8 at dim = 64 (err 2.9e-7 against a yardstick of
    3.3e-8), every other case of this test stays below 1.2.  g itself is at
    0.91 of its yardstick there (1.2e-6, from the float32 phase 2 pi f k at
    k up to 31), and 64 such errors weighted by |W| ~ 1/8 sum to about
    5e-7 -- the kernel's error is the expected one, while the float32
    restatement's cancel to 2 ulp by chance.  With one output there is no
    maximum over outputs to even that draw out; the g check keeps the
    factor 4."""
    g = _gen(dim * 100 + rows)
    sigma = _sigmas(n)
    W, bias = _proj(rows, dim, g)
    te_w, te_b = f32(0.7), f32(-0.4)

    def ref(dt):
        sd = {"e.weight": torch.tensor([te_w], dtype=dt), "e.bias": torch.tensor([te_b], dtype=dt)}
        gv = O.simple_time_embedding(sd, "e", torch.log10(sigma.to(dt)), dim)
        return gv, F.linear(gv, W.to(dt), bias.to(dt))

    keep = [sigma.to(DEV), W.to(DEV), bias.to(DEV)]
    d = L.EmbedDesc()
    d.sigma, d.n, d.kind, d.dim, d.rows = keep[0].data_ptr(), n, 0, dim, rows
    d.te_weight, d.te_bias = te_w, te_b
    d.w, d.bias = keep[1].data_ptr(), keep[2].data_ptr()
    out, gbuf = _run_embed(d, n, rows, dim)
    (g64, o64), (g32, o32) = ref(F64), ref(F32)
    _close(f"embed[simple dim={dim} rows={rows} n={n}] g", gbuf, g64, g32)
    _close(f"embed[simple dim={dim} rows={rows} n={n}] out", out, o64, o32, factor=16 if rows * n == 1 else 4)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("rows", [5, 64])
@pytest.mark.parametrize("n_rff,dim", [(4, 40), (32, 512), (128, 1024)])
def test_embed_sigma_block(n_rff, dim, rows, n):
    """kind 1 (sigma_block.py:24-57): random Fourier features -> three Linear +
    PReLU layers of widths 4 n_rff, 8 n_rff, dim, with three distinct slopes,
    then the projections.  (128, 1024) is the largest the kernel's LDS
    buffers hold."""
    g = _gen(n_rff * 10 + rows)
    sigma = _sigmas(n)
    W, bias = _proj(rows, dim, g)
    sd = {"s.freq": torch.randn(n_rff, generator=g) * 16.0}
    widths = [2 * n_rff, 4 * n_rff, 8 * n_rff, dim]
    slopes = [f32(0.25), f32(0.1), f32(0.4)]
    for i in range(3):
        sd[f"s.layer{i + 1}.lin.weight"] = torch.randn(widths[i + 1], widths[i], generator=g) / math.sqrt(widths[i])
        sd[f"s.layer{i + 1}.lin.bias"] = torch.randn(widths[i + 1], generator=g) * 0.1
        sd[f"s.layer{i + 1}.prelu.weight"] = torch.tensor([slopes[i]])

    def ref(dt):
        gv = O.sigma_block({k: v.to(dt) for k, v in sd.items()}, "s", torch.log10(sigma.to(dt)))
        return gv, F.linear(gv, W.to(dt), bias.to(dt))

    keep = {k: v.to(DEV).contiguous() for k, v in sd.items()}
    keep.update(sigma=sigma.to(DEV), W=W.to(DEV), bias=bias.to(DEV))
    d = L.EmbedDesc()
    d.sigma, d.n, d.kind, d.dim, d.rows = keep["sigma"].data_ptr(), n, 1, dim, rows
    d.rff_freq, d.n_rff = keep["s.freq"].data_ptr(), n_rff
    for i in range(3):
        d.mlp_w[i] = keep[f"s.layer{i + 1}.lin.weight"].data_ptr()
        d.mlp_b[i] = keep[f"s.layer{i + 1}.lin.bias"].data_ptr()
        d.mlp_slope[i] = slopes[i]
    d.w, d.bias = keep["W"].data_ptr(), keep["bias"].data_ptr()
    out, gbuf = _run_embed(d, n, rows, dim)
    (g64, o64), (g32, o32) = ref(F64), ref(F32)
    _close(f"embed[rff={n_rff} dim={dim} rows={rows} n={n}] g", gbuf, g64, g32)
    _close(f"embed[rff={n_rff} dim={dim} rows={rows} n={n}] out", out, o64, o32)


# ------------------------------------------------------------------ head
HEAD_COEF = dict(w_skip=f32(0.8), w_out=f32(0.6), s2=f32(0.49), c_score=f32(0.3), c_noise=f32(0.2), s_next=f32(0.5))
SLOPE1, SLOPE2 = f32(0.25), f32(0.1)


def _head(h, w, bias, x, z, mode, edm, c):
    """ouhip.h: net = conv3(prelu2(prelu1(h))) + bias (zero padding), then the
    EDM wrapper (universe.py:197-209) and the sampler update (:334-343)."""
    a = torch.where(h >= 0, h, h * SLOPE1)
    a = torch.where(a >= 0, a, a * SLOPE2)
    net = F.conv1d(a, w[None], padding=1)[:, 0] + bias
    if mode == 0:
        return net
    score = ((c["w_skip"] * x + c["w_out"] * net) - x) / c["s2"] if edm else net
    out = x + c["c_score"] * score
    if mode == 1:
        out = out + c["c_noise"] * (z * c["s_next"])
    return out


def _head_cases():
    combos = [(m, e) for m in (0, 1, 2) for e in (0, 1)]
    cases, i = [], 0
    for C in (1, 4, 8, 12, 33):
        for T in (1, 2, 256, 257, 515):
            every = (C, T) in ((33, 1), (12, 257))   # the clamped-neighbour case and the ragged one: all six
            for m, e in (combos if every else [combos[i % 6]]):
                cases.append((C, T, m, e))
            i += 1
    return cases


@pytest.mark.parametrize("C,T,mode,edm", _head_cases())
def test_head(C, T, mode, edm):
    """Rows C T + 5 apart (1e6 between them); the first and last sample of
    every channel are +-50, so a neighbour tap that is clamped to the edge
    instead of masked (both, at T == 1) is far outside the bound.  In the
    sampler modes the output overwrites x, as the plan records it."""
    B = 2
    g = _gen(C * 1000 + T)
    h = torch.randn(B, C, T, generator=g)
    sign = torch.tensor([1.0 if c % 2 == 0 else -1.0 for c in range(C)])
    h[:, :, 0] = 50.0 * sign
    h[:, :, T - 1] = -50.0 * sign
    w = torch.randn(C, 3, generator=g) / math.sqrt(3 * C)
    bias = f32(0.05)
    x, z = torch.randn(B, T, generator=g), torch.randn(B, T, generator=g)
    hd = _strided(h.reshape(B, C * T), C * T + 5)
    wd, zd = w.to(DEV).contiguous(), z.to(DEV)
    xd = x.to(DEV)
    od = xd if mode != 0 else torch.full((B, T), POISON, dtype=F32, device=DEV)
    d = L.HeadDesc()
    d.h, d.h_bstride = hd.data_ptr(), C * T + 5
    d.channels, d.length, d.batch, d.mode = C, T, B, mode
    d.slope1, d.slope2, d.w, d.bias, d.edm = SLOPE1, SLOPE2, wd.data_ptr(), bias, edm
    for k, v in HEAD_COEF.items():
        setattr(d, k, v)
    d.x, d.z, d.out = (xd.data_ptr() if mode else 0), (zd.data_ptr() if mode == 1 else 0), od.data_ptr()
    L.run_now(L.OP_HEAD, d, _stream())
    torch.cuda.synchronize()
    ref64 = _head(h.double(), w.double(), bias, x.double(), z.double(), mode, edm, HEAD_COEF)
    ref32 = _head(h, w, torch.tensor(bias, dtype=F32), x, z, mode, edm,
                  {k: torch.tensor(v, dtype=F32) for k, v in HEAD_COEF.items()})
    _close(f"head[C={C} T={T} mode={mode} edm={edm}]", od, ref64, ref32)


# ------------------------------------------------------------------ alias-free snake
SNAKE_T = [1, 2, 13, 255, 256, 257, 700]
SNAKE_ALPHA = torch.tensor([1e-3, 1.0, 8.0], dtype=F32)


def _snake(u, alpha):
    return u + (1.0 / (alpha + 1e-9)) * torch.sin(u * alpha) ** 2


def _run_snake(h, ku, wu, kd, wd):
    """h (B, C, T), ku (2, taps_up), kd (taps_down): the descriptor as
    Engine.rec_aux fills it (rows of one item T apart, items h_bstride apart)."""
    B, C, T = h.shape
    hd = _strided(h.reshape(B, C * T), C * T + 3)
    keep = [SNAKE_ALPHA.to(DEV), ku.reshape(-1).contiguous().to(DEV), kd.reshape(-1).contiguous().to(DEV)]
    out = torch.full((B, C, T), POISON, dtype=F32, device=DEV)
    d = L.SnakeDesc()
    d.h, d.h_bstride = hd.data_ptr(), C * T + 3
    d.channels, d.length, d.batch = C, T, B
    d.alpha, d.k_up, d.taps_up, d.width_up = keep[0].data_ptr(), keep[1].data_ptr(), ku.shape[1], wu
    d.k_down, d.taps_down, d.width_down, d.out = keep[2].data_ptr(), kd.shape[-1], wd, out.data_ptr()
    L.run_now(L.OP_SNAKE, d, _stream())
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("T", SNAKE_T)
def test_snake_aa(T):
    """The shipped filters (dsp.sinc_resample_kernel(1, 2) / (2, 1), as
    Engine._prep_sdl prepares them) against the oracle's torchaudio-style
    resample at float64: up x2, u + sin(a u)^2 / (a + 1e-9), down x2.  T
    shorter than the filters, and on either side of the 256-sample tile."""
    B, C = 2, 3
    h = torch.rand(B, C, T, generator=_gen(T)) * 4 - 2
    ku, wu = dsp.sinc_resample_kernel(1, 2)
    kd, wd = dsp.sinc_resample_kernel(2, 1)
    # the oracle's resample builds its own taps: they must be the engine's
    assert np.array_equal(O._sinc_resample_kernel(1, 2)[0].numpy().reshape(ku.shape), ku)
    assert np.array_equal(O._sinc_resample_kernel(2, 1)[0].numpy().reshape(kd.shape), kd)

    def ref(dt):
        u = O.resample(h.to(dt), 1, 2)
        return O.resample(_snake(u, SNAKE_ALPHA.to(dt)[None, :, None]), 2, 1)

    got = _run_snake(h, torch.from_numpy(ku), wu, torch.from_numpy(kd), wd)
    _close(f"snake_aa[T={T}]", got, ref(F64), ref(F32))


def _snake_direct(h, ku, wu, kd, wd, alpha):
    """The two formulas of the kernel's comment, zero outside the signals:
    u[2s + i] = sum_k ku[i][k] h[s + k - wu];  y[t] = sum_k kd[k] v[2t + k - wd]."""
    B, C, T = h.shape
    tu, td = ku.shape[1], kd.shape[0]
    x = F.pad(h.reshape(B * C, 1, T), (wu, tu))
    u = F.conv1d(x, ku[:, None, :])[:, :, :T]                  # [.][i][s]
    u = u.transpose(1, 2).reshape(B, C, 2 * T)
    v = _snake(u, alpha[None, :, None])
    v = F.pad(v.reshape(B * C, 1, 2 * T), (wd, td))
    return F.conv1d(v, kd[None, None, :], stride=2)[:, 0, :T].reshape(B, C, T)


@pytest.mark.parametrize("T", [13, 257, 700])
def test_snake_aa_at_the_tap_limits(T):
    """32 up / 64 down taps, the longest ou_snake_aa accepts (the shipped
    filters have 15 and 28): a full tile then stages the most input samples
    the kernel's LDS arrays hold.  Random taps; the restatement is written
    from the kernel's two formulas (and agrees with the oracle's resample on
    the shipped filters)."""
    B, C = 2, 3
    g = _gen(50 + T)
    h = torch.rand(B, C, T, generator=g) * 4 - 2
    ku = torch.randn(2, 32, generator=g) / math.sqrt(32.0)
    kd = torch.randn(64, generator=g) / math.sqrt(64.0)
    wu, wd = 15, 31
    sk, sw = dsp.sinc_resample_kernel(1, 2)
    dk, dw = dsp.sinc_resample_kernel(2, 1)
    a64 = SNAKE_ALPHA.double()
    shipped = _snake_direct(h.double(), torch.from_numpy(sk).double(), sw, torch.from_numpy(dk).double()[0], dw, a64)
    oracle = O.resample(_snake(O.resample(h.double(), 1, 2), a64[None, :, None]), 2, 1)
    assert torch.allclose(shipped, oracle, rtol=0, atol=1e-12)
    got = _run_snake(h, ku, wu, kd, wd)
    _close(f"snake_aa[limits T={T}]", got, _snake_direct(h.double(), ku.double(), wu, kd.double(), wd, a64),
           _snake_direct(h, ku, wu, kd, wd, SNAKE_ALPHA))
