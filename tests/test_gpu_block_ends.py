"""ou_block's two stages at the score network's ends, each against a float64
restatement written here and against the unfused launches on the same inputs:

  kEpiIn    the score input conv h = conv1d(in_scale[b] x, w_in) + b_in
            (1 -> C, k3) computed inside the first encoder block instead of
            read: alone, with FiLM, and with FiLM and the rate-change conv
            (y and e);
  kEpiHead  the score head on the block output, which is not stored: two
            PReLUs, output_conv C -> 1 k3, the EDM wrapper and the sampler
            update, alone and in the decoder form (input_cond + FiLM), every
            (mode, edm), out written over x in the sampler modes.

32 and 48 channels (48: padded MFMA rows), f32 / split-f16 / f16 operands,
batch 2.  Every variant runs at T in {1, 2, 3, Fo - 1, Fo, Fo + 1, 2 Fo + 1},
Fo the frames a workgroup of that variant owns (from ou_block_frames): the
clip's ends inside one workgroup, and a workgroup seam one frame before, at
and one frame after the clip's end.

Inputs are chosen so that a wrong padding rule, item or order is far past the
bound: per-item in_scale (0.5, 2) and NULL, b_in of order 1 (h = b_in outside
the clip would show), +-50 in the first and last sample, x rows further apart
than T with POISON between, distinct z per item, head slopes (0.25, 0.1) and
(-0.5, 0.1) -- with a negative first slope the order of the two PReLUs
matters.  Every output lies in a POISON-filled buffer with longer rows and a
spare item, which must stay POISON, as must the y buffer of a head launch.

Bounds: rel-RMS against float64 below 1e-5 (f32, split-f16) and 3e-3 (f16),
the figures of test_gpu_block.py for the same arithmetic.  The sampler modes'
out is affine in net with slope k = c_score w_out / s2 (EDM) or c_score: there
rms(out - ref) <= tol rms(k net_ref) + 2^-23 max|ref|, so the O(1) x term
hides nothing.  The unfused sequence (ou_conv input conv, three ou_conv
launches, ou_conv rate change, ou_head) must agree within the same figures.
Every measured ratio is printed ("ends-ratio ...").  Largest values measured
on an MI355X, against float64 / against the unfused launches:
  f32        y 1.6e-7 / 1.8e-7                      head 3.4e-7 / 4.7e-7
  split-f16  y 1.0e-7 / 1.3e-7   e 1.7e-7 / 1.9e-7  head 2.8e-7 / 2.7e-7
  f16        y 2.4e-4 / 3.2e-4   e 3.9e-4 / 5.3e-4  head 2.6e-4 / 2.5e-5

The descriptors ou_block must refuse are checked at the bottom: ou_block
returns before any launch."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from open_universe_amd import _lib as L
from open_universe_amd import engine as E
from test_gpu_block import _down_ref, _down_spec, _ref, _specs
from test_gpu_misc import HEAD_COEF, POISON, f32

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = torch.float32
B = 2
SCALES = (0.5, 2.0)
SLOPES = ((f32(0.25), f32(0.1)), (f32(-0.5), f32(0.1)))
HEAD_BIAS = f32(0.05)
EDGE = 50.0


def _tol(prec):
    return 1e-5 if prec in (0, 1) else 3e-3   # f32 and split-f16 operands: f32-class; f16: 11 bits


def _frames(C, kind, kt=0, r=2):
    """Frames a workgroup of the variant owns (block_f in ou_block.hip)."""
    Fw = L.load().ou_block_frames(C)
    if kind == "head":
        return Fw - 2
    if kind == "down":
        return (Fw - 2 * r * ((kt - 1) // 2)) // r * r
    return Fw


def _lengths(Fo):
    return [1, 2, 3, Fo - 1, Fo, Fo + 1, 2 * Fo + 1]


def _rms(a):
    return float(a.double().pow(2).mean().sqrt())


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


# ---------------------------------------------------------------- weights
@functools.lru_cache(maxsize=None)
def _weights(C, kt):
    """Logical weights of one variant family, the same at every precision and
    length: the block's three convs, the input conv, the rate-change conv
    (rate 2, kt frames; kt 0: none) and the head's output conv."""
    g = torch.Generator().manual_seed(9000 + C + kt)
    specs = _specs(C, g)
    w_in = torch.randn(C, 1, 3, generator=g) / np.sqrt(3.0)
    b_in = 1.0 + 0.5 * torch.randn(C, generator=g)
    rsp = _down_spec(C, 2, kt, g) if kt else None
    w_head = torch.randn(C, 3, generator=g) / np.sqrt(3.0 * C)
    return specs, w_in, b_in, rsp, w_head


class _Dev:
    """The weights of _weights(C, kt) packed for one precision."""

    def __init__(self, C, prec, kt=0):
        self.C, self.prec = C, prec
        self.specs, self.w_in, self.b_in, self.rsp, self.w_head = _weights(C, kt)
        self.status = torch.zeros(4, dtype=torch.int32, device=DEV)
        saved = E._PREP_STATUS
        E._PREP_STATUS = self.status.data_ptr() + 4
        try:
            cws = [E.make_conv(sp, DEV, prec=prec) for sp in self.specs]
            fused = E.prep_fused(self.specs, C, prec, DEV)
            in_spec = E.ConvSpec(self.w_in.numpy(), 1, 1, 1, 1, 1.0, self.b_in.numpy(), ref_macs=3.0 * C)
            self.c_in = E.make_conv(in_spec, DEV, prec=prec)
            rc = down = None
            if self.rsp is not None:
                rc = E.make_conv(self.rsp, DEV, prec=prec)
                down = E.prep_down_fused(self.rsp, C, prec, rc.bias, DEV)
                assert down is not None
        finally:
            E._PREP_STATUS = saved
        assert fused is not None
        self.bw = E.BlockW(C, "down" if kt else "none", 2 if kt else None, *cws, rc, fused, down)
        self.w_in_d = self.w_in.reshape(C, 3).contiguous().to(DEV)
        self.b_in_d = self.b_in.contiguous().to(DEV)
        self.w_head_d = self.w_head.contiguous().to(DEV)
        self.scales_d = torch.tensor(SCALES, dtype=F32, device=DEV)


# ---------------------------------------------------------------- float64 restatement
def _in_ref(x, scale, w_in, b_in):
    """h = conv1d(in_scale[b] x, w_in, padding=1) + b_in (score.py:244-246, 285), x (B, T)."""
    xs = x.double() if scale is None else x.double() * torch.tensor(scale, dtype=torch.float64)[:, None]
    return F.conv1d(xs[:, None], w_in.double(), padding=1) + b_in.double()[None, :, None]


def _head_net(y, w, bias, slopes, dtype=torch.float64):
    """net = conv3(prelu2(prelu1(y))) + bias, zero padding (test_gpu_misc._head with the slopes as arguments)."""
    y = y.to(dtype)
    a = torch.where(y >= 0, y, y * slopes[0])
    a = torch.where(a >= 0, a, a * slopes[1])
    return F.conv1d(a, w.to(dtype)[None], padding=1)[:, 0] + bias


def _head_out(net, x, z, mode, edm, c=HEAD_COEF):
    """The EDM wrapper (universe.py:197-209) and the sampler update (:334-343)."""
    if mode == 0:
        return net
    score = ((c["w_skip"] * x + c["w_out"] * net) - x) / c["s2"] if edm else net
    out = x + c["c_score"] * score
    if mode == 1:
        out = out + c["c_noise"] * (z * c["s_next"])
    return out


def _edges(t, g):
    """+-EDGE in the first and last sample of every row of t (..., T), the sign alternating from row to row."""
    shape = t.shape[:-1]
    sign = torch.ones(shape).reshape(-1)
    sign[1::2] = -1.0
    sign = sign.reshape(shape)
    t[..., 0] = EDGE * sign
    t[..., -1] = -EDGE * sign
    return t


@functools.lru_cache(maxsize=None)
def _in_problem(C, film, kt, T, scaled):
    """Inputs and the float64 y (and e) of an input-conv variant; shared by the precisions."""
    specs, w_in, b_in, rsp, _ = _weights(C, kt)
    g = torch.Generator().manual_seed(C * 100000 + T * 10 + film * 4 + kt + 2 * scaled)
    x = _edges(torch.randn(B, T, generator=g), g)
    fm = torch.randn(B, 2 * C, generator=g) * 0.5 + torch.cat([torch.ones(C), torch.zeros(C)]) if film else None
    h = _in_ref(x, SCALES if scaled else None, w_in, b_in)
    y, _ = _ref(specs, h, film=None if fm is None else fm.double())
    e = _down_ref(rsp, y) if kt else None
    return x, fm, y, e


@functools.lru_cache(maxsize=None)
def _head_problem(C, dec, T):
    """Inputs and the float64 block output of a head variant (dec: input_cond + FiLM)."""
    specs = _weights(C, 0)[0]
    g = torch.Generator().manual_seed(C * 100000 + T * 10 + 7 + dec)
    h = _edges(torch.randn(B, C, T, generator=g), g)
    sc = torch.randn(B, C, T, generator=g) if dec else None
    fm = (1.0 + 0.3 * torch.randn(B, 2 * C, generator=g)) if dec else None
    x, z = torch.randn(B, T, generator=g), torch.randn(B, T, generator=g)
    y, _ = _ref(specs, h.double(), None if sc is None else sc.double(), None if fm is None else fm.double())
    return h, sc, fm, x, z, y


# ---------------------------------------------------------------- buffers and launches
def _margin(Bn, C, T):
    """A POISON buffer of Bn + 1 items with rows 3 floats longer than T, and the Act of its (Bn, C, T) window."""
    buf = torch.full((Bn + 1, C, T + 3), POISON, dtype=F32, device=DEV)
    return buf, E.Act(buf[:Bn, :, :T])


def _margin_clean(buf, Bn, T):
    return bool((buf[:Bn, :, T:] == POISON).all()) and bool((buf[Bn] == POISON).all())


def _play(record, fill):
    """Record with the library's default tiles (a conv tuner left on by an
    earlier test would time convs on these very buffers while recording), then
    give the buffers their contents, then run."""
    prog = L.Program()
    saved, L.TUNER = L.TUNER, None
    try:
        record(prog)
    finally:
        L.TUNER = saved
    kinds = prog.op_kinds()
    fill()
    prog.run(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return kinds


def _unfused(bw):
    class _Off:
        def __enter__(self):
            self.keep = (bw.fused, bw.down)
            bw.fused = bw.down = None

        def __exit__(self, *a):
            bw.fused, bw.down = self.keep
    return _Off()


# ---------------------------------------------------------------- kEpiIn
def _run_in(dv, film, kt, T, scaled, report):
    C, prec = dv.C, dv.prec
    x, fm, y64, e64 = _in_problem(C, film, kt, T, scaled)
    U = -(-T // 2)
    scale_ptr = dv.scales_d.data_ptr() if scaled else 0
    xbuf = torch.full((B, 1, T + 5), POISON, dtype=F32, device=DEV)   # rows T + 5 apart
    xa = E.Act(xbuf[:, :, :T])
    fmd = fm.to(DEV) if film else None
    kw = {"film": fmd.data_ptr(), "film_bs": 2 * C} if film else {}

    def fill_x():
        xbuf.fill_(POISON)
        xbuf[:, 0, :T] = x.to(DEV)

    # fused: h is never read (POISON, and must stay so)
    hbuf = torch.full((B, C, T), POISON, dtype=F32, device=DEV)
    ha = E.Act(hbuf)
    ybuf, ya = _margin(B, C, T)
    ebuf, ea = _margin(B, 2 * C, U) if kt else (None, None)
    tA, tB = E.new_act(B, C, T, DEV), E.new_act(B, C, T, DEV)

    def rec_f(prog):
        d_in = E.conv_desc(dv.c_in, xa, ha, in_scale=scale_ptr)
        E.rec_block(prog, dv.bw, ha, ya, tA, tB, x_in=(xa, scale_ptr, dv.w_in_d, dv.b_in_d, d_in), e_out=ea, **kw)

    def fill_f():
        fill_x()
        hbuf.fill_(POISON), ybuf.fill_(POISON)
        if kt:
            ebuf.fill_(POISON)

    kinds = _play(rec_f, fill_f)
    assert kinds == [L.OP_BLOCK], kinds   # the input conv and the rate change ran inside the block
    assert bool((hbuf == POISON).all()), "h was written"
    assert _margin_clean(ybuf, B, T), "y stored outside its window"
    assert bool((xbuf[:, :, T:] == POISON).all())
    yf = ybuf[:B, :, :T].cpu()
    ef = ebuf[:B, :, :U].cpu() if kt else None
    if kt:
        assert _margin_clean(ebuf, B, U), "e stored outside its window"

    # unfused: ou_conv input conv, three ou_conv launches, ou_conv rate change
    hu, yu = E.new_act(B, C, T, DEV), E.new_act(B, C, T, DEV)
    eu = E.new_act(B, 2 * C, U, DEV) if kt else None

    def rec_u(prog):
        prog.add(L.OP_CONV, E.conv_desc(dv.c_in, xa, hu, in_scale=scale_ptr))
        with _unfused(dv.bw):
            E.rec_block(prog, dv.bw, hu, yu, tA, tB, e_out=eu, **kw)

    kinds_u = _play(rec_u, fill_x)
    assert L.OP_BLOCK not in kinds_u and kinds_u.count(L.OP_CONV) == (5 if kt else 4), kinds_u

    tol = _tol(prec)
    tag = f"in[C={C} prec={prec} film={int(film)} kt={kt} T={T} scaled={int(scaled)}]"
    checks = [("y", yf, y64, yu.t.cpu())] + ([("e", ef, e64, eu.t.cpu())] if kt else [])
    for what, got, ref, unf in checks:
        r64, ru = _rel(got, ref), _rel(got, unf)
        print(f"ends-ratio {tag} {what} vs f64 {r64:.3e} vs unfused {ru:.3e} (unfused vs f64 {_rel(unf, ref):.3e})")
        report.append((f"{tag} {what}", r64 < tol and ru < tol, r64, ru))


@pytest.mark.parametrize("prec", [0, 1, 2])
@pytest.mark.parametrize("C", [32, 48])
@pytest.mark.parametrize("film", [False, True])
def test_block_input_conv(C, film, prec):
    """kEpiIn and kEpiFilm|kEpiIn: y against float64 and the unfused launches."""
    dv = _Dev(C, prec)
    report = []
    for scaled in (True, False):
        for T in _lengths(_frames(C, "in")):
            _run_in(dv, film, 0, T, scaled, report)
    assert int(dv.status.abs().sum()) == 0
    assert all(ok for _, ok, _, _ in report), [r for r in report if not r[1]]


@pytest.mark.parametrize("prec", [1, 2])
@pytest.mark.parametrize("kt", [3, 1])
def test_block_input_conv_down(kt, prec):
    """kEpiFilm|kEpiIn|kEpiDown (32 channels, rate 2): y and e = rate_conv(y)."""
    C = 32
    dv = _Dev(C, prec, kt)
    report = []
    for scaled in (True, False):
        for T in _lengths(_frames(C, "down", kt)):
            _run_in(dv, True, kt, T, scaled, report)
    assert int(dv.status.abs().sum()) == 0
    assert all(ok for _, ok, _, _ in report), [r for r in report if not r[1]]


# ---------------------------------------------------------------- kEpiHead
def _head_desc(dv, T, mode, edm, slopes, x_ptr, z_ptr, out_ptr, h=None):
    d = L.HeadDesc()
    if h is not None:
        d.h, d.h_bstride = h.ptr, h.bs
    d.channels, d.length, d.batch, d.mode = dv.C, T, B, mode
    d.slope1, d.slope2, d.w, d.bias, d.edm = slopes[0], slopes[1], dv.w_head_d.data_ptr(), HEAD_BIAS, edm
    for k, v in HEAD_COEF.items():
        setattr(d, k, v)
    d.x, d.z, d.out = (x_ptr if mode else 0), (z_ptr if mode == 1 else 0), out_ptr
    d._flops = 2.0 * dv.C * 3 * T * B
    return d


def _run_head(dv, dec, T, mode, edm, slopes, report):
    C, prec = dv.C, dv.prec
    h, sc, fm, x, z, y64 = _head_problem(C, dec, T)
    ha = E.Act(h.to(DEV))
    zd = z.to(DEV)
    kw = {}
    if dec:
        fmd = fm.to(DEV)
        kw = {"sc": E.Act(sc.to(DEV)), "film": fmd.data_ptr(), "film_bs": 2 * C}
    tA, tB = E.new_act(B, C, T, DEV), E.new_act(B, C, T, DEV)

    def state():
        """The sampler state [B][T] with a spare POISON item; out is this buffer in modes 1 / 2, else all POISON."""
        xs = torch.full((B + 1, T), POISON, dtype=F32, device=DEV)
        return xs, (xs if mode else torch.full((B + 1, T), POISON, dtype=F32, device=DEV))

    def fill(xs, od):
        od.fill_(POISON)
        xs.fill_(POISON)
        if mode:
            xs[:B] = x.to(DEV)

    # fused: the y buffer handed to rec_block must stay untouched
    ybuf, ya = _margin(B, C, T)
    xs, od = state()
    hd = _head_desc(dv, T, mode, edm, slopes, xs.data_ptr(), zd.data_ptr(), od.data_ptr())
    kinds = _play(lambda prog: E.rec_block(prog, dv.bw, ha, ya, tA, tB, head=hd, **kw),
                  lambda: (fill(xs, od), ybuf.fill_(POISON)))
    assert kinds == [L.OP_BLOCK], kinds
    assert bool((ybuf == POISON).all()), "the block output was stored although the head consumes it"
    assert bool((od[B] == POISON).all()) and bool((xs[B] == POISON).all()), "out stored past the last item"
    if mode == 0:
        assert bool((xs == POISON).all())
    got = od[:B].cpu()

    # unfused: three ou_conv launches, then ou_head on the stored block output
    yu = E.new_act(B, C, T, DEV)
    xu, ou = state()
    hu = _head_desc(dv, T, mode, edm, slopes, xu.data_ptr(), zd.data_ptr(), ou.data_ptr(), h=yu)

    def rec_u(prog):
        with _unfused(dv.bw):
            E.rec_block(prog, dv.bw, ha, yu, tA, tB, **kw)
        prog.add(L.OP_HEAD, hu)

    kinds_u = _play(rec_u, lambda: fill(xu, ou))
    assert L.OP_BLOCK not in kinds_u and kinds_u.count(L.OP_HEAD) == 1, kinds_u
    unf = ou[:B].cpu()

    net = _head_net(y64, dv.w_head, HEAD_BIAS, slopes)
    ref = _head_out(net, x.double(), z.double(), mode, edm)
    k = 1.0 if mode == 0 else HEAD_COEF["c_score"] * (HEAD_COEF["w_out"] / HEAD_COEF["s2"] if edm else 1.0)
    tol = _tol(prec)
    scale = _rms(k * net)                                    # what an error of net is measured against
    floor = 2.0 ** -23 * float(ref.abs().max()) if mode else 0.0   # one f32 ulp of the largest output
    e64, eu = _rms(got.double() - ref), _rms(got.double() - unf.double())
    tag = (f"head[C={C} prec={prec} dec={int(dec)} T={T} mode={mode} edm={edm} slope1={slopes[0]:+.2f}]")
    print(f"ends-ratio {tag} vs f64 {e64 / scale:.3e} vs unfused {eu / scale:.3e} "
          f"(unfused vs f64 {_rms(unf.double() - ref) / scale:.3e}; floor/scale {floor / scale:.1e})")
    report.append((tag, e64 <= tol * scale + floor and eu <= tol * scale + floor, e64 / scale, eu / scale))


@pytest.mark.parametrize("prec", [0, 1, 2])
@pytest.mark.parametrize("C", [32, 48])
@pytest.mark.parametrize("dec", [False, True])
@pytest.mark.parametrize("mode,edm", [(m, e) for m in (0, 1, 2) for e in (0, 1)])
def test_block_head(C, dec, mode, edm, prec):
    """kEpiHead and kEpiFilm|kEpiSc|kEpiHead: head.out against float64 and the
    unfused launches, positive head slopes and a negative first slope."""
    dv = _Dev(C, prec)
    report = []
    for slopes in SLOPES:
        for T in _lengths(_frames(C, "head")):
            _run_head(dv, dec, T, mode, edm, slopes, report)
    assert int(dv.status.abs().sum()) == 0
    assert all(ok for _, ok, _, _ in report), [r for r in report if not r[1]]


# ---------------------------------------------------------------- refusals
def _refusal_desc(C, T=40, film=False, x=False, head=False, res2=False):
    """A launchable descriptor of every buffer the case names, outputs POISON."""
    dv = _Dev(C, 1)
    keep = {"dv": dv}
    ha = E.Act(torch.randn(B, C, T, generator=torch.Generator().manual_seed(3)).to(DEV))
    ybuf, ya = _margin(B, C, T)
    tA, tB = E.new_act(B, C, T, DEV), E.new_act(B, C, T, DEV)
    fmd = torch.ones(B, 2 * C, dtype=F32, device=DEV)
    r2 = E.Act(torch.zeros(B, C, T, dtype=F32, device=DEV)) if res2 else None
    d1 = E.conv_desc(dv.bw.conv1, ha, tA)
    d = E.block_desc(dv.bw, ha, ya, (d1,), film=fmd.data_ptr() if film else 0, film_bs=2 * C, res2=r2)
    xd = torch.zeros(B, 1, T, dtype=F32, device=DEV)
    if x:   # block_desc would assert on the channel count: the fields by hand
        d.x, d.x_bstride, d.in_scale = xd.data_ptr(), T, dv.scales_d.data_ptr()
        d.w_in, d.b_in = dv.w_in_d.data_ptr(), dv.b_in_d.data_ptr()
    od = torch.full((B, T), POISON, dtype=F32, device=DEV)
    if head:
        d.head = _head_desc(dv, T, 0, 1, SLOPES[0], 0, 0, od.data_ptr())
    keep.update(ha=ha, tA=tA, tB=tB, fmd=fmd, r2=r2, xd=xd)
    return d, (ybuf, od), keep


def _refused(d, outs, *words):
    rc = L.load().ou_block(ctypes.byref(d), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    msg = (L.load().ou_last_error() or b"").decode()
    torch.cuda.synchronize()
    assert rc == -1, (rc, msg)
    assert any(w in msg for w in words), msg
    for o in outs:
        assert bool((o == POISON).all()), "a refused descriptor was launched"


def _image(C, T):
    """A split image [C / 32][T][hi | lo][32] f16 per item, POISON-free zeros."""
    return torch.zeros(B, C // 32, T, 64, dtype=torch.float16, device=DEV)


def test_refuses_input_conv_at_64_channels():
    d, outs, keep = _refusal_desc(64, x=True)
    _refused(d, outs, "epilogue combination")


def test_refuses_head_with_res2():
    d, outs, keep = _refusal_desc(32, head=True, res2=True)
    _refused(d, outs, "epilogue combination")


def test_refuses_head_with_split_image_output():
    C, T = 32, 40
    d, outs, keep = _refusal_desc(C, T, head=True)
    img = _image(C, T)
    d.sy, d.sy_bstride, d.sy_rows, d.sy_shift, d.sy_slope = img.data_ptr(), img.stride(0) * 2, T, 6, 0.2
    _refused(d, outs, "no head", "epilogue combination")
    assert int(img.abs().sum()) == 0


def test_refuses_input_conv_with_split_image_input():
    C, T = 32, 40
    d, outs, keep = _refusal_desc(C, T, x=True)
    img = _image(C, T)
    d.xs, d.xs_bstride, d.xs_rows = img.data_ptr(), img.stride(0) * 2, T
    _refused(d, outs, "no input conv", "epilogue combination")


def test_refuses_input_conv_down_at_48_channels():
    """kEpiFilm|kEpiIn|kEpiDown exists at 32 channels only."""
    C, T, r, kt = 48, 40, 2, 3
    d, outs, keep = _refusal_desc(C, T, film=True, x=True)
    g = torch.Generator().manual_seed(4)
    w = (torch.randn(2 * C, C, kt * r, generator=g) / np.sqrt(C * kt * r)).numpy()
    packed, un = L.block_pack_np(np.ascontiguousarray(w))
    wd = torch.from_numpy(packed).to(DEV)
    bd = torch.zeros(2 * C, dtype=F32, device=DEV)
    U = -(-T // r)
    ebuf = torch.full((B, 2 * C, U), POISON, dtype=F32, device=DEV)
    d.w_down, d.w_down_unscale, d.b_down = wd.data_ptr(), un, bd.data_ptr()
    d.slope_down, d.rate, d.down_kt = 0.2, r, kt
    d.e, d.e_bstride, d.e_cstride = ebuf.data_ptr(), 2 * C * U, U
    _refused(d, outs + (ebuf,), "epilogue combination", "no fused rate-change conv")
