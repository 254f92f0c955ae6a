"""ou_block's fourth stage kEpiUp: the decoder's anti-aliased up-sampling conv
run inside the block that produces its input, against the unfused launches
(the block, then conv_fukernel) and a float64 restatement: the block, PReLU,
transposed conv, binomial FIR 'same' with zeros outside, bias, zero past
valid_len, (v + skip) / sqrt 2.  Several windows with a ragged last one,
exactly one window, a signal shorter than the halo; batch 2; split-f16 and
f16; with and without FiLM + input_cond; a cropped output; the y store
skipped; the range flag; and the whole model with the stage on and off."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from open_universe_amd import _lib as L
from open_universe_amd import dsp
from open_universe_amd import engine as E
from test_gpu_block import _ref, _rel, _specs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -12345.0


def _up_sd(C, r, g):
    """State-dict entries of an anti-aliased up-sampling PReLU_Conv(C -> C / 2, stride r)."""
    return {"u.conv.weight": torch.randn(C, C // 2, r, generator=g) / np.sqrt(C),
            "u.bias": 0.1 * torch.randn(C // 2, generator=g),
            "u.prelu.weight": torch.tensor([0.2])}


def _up_ref(sd, r, y, skip, out_len, valid_len):
    """float64: PReLU, transposed conv, FIR 'same' (zeros outside), bias, zero past valid_len, skip."""
    w = sd["u.conv.weight"].double()
    x = torch.where(y >= 0, y, float(sd["u.prelu.weight"][0]) * y)
    z = F.conv_transpose1d(x, w, stride=r)
    taps = torch.from_numpy(dsp.binomial_taps(2 * r + 1).astype(np.float64))
    co = z.shape[1]
    v = F.conv1d(z, taps.flip(0)[None, None].repeat(co, 1, 1), padding=r, groups=co)
    v = v + sd["u.bias"].double()[None, :, None]
    v[:, :, valid_len:] = 0.0
    return ((v[:, :, :out_len] + skip) * 0.5 ** 0.5)


def _prep(C, r, prec, g, status=None):
    specs = _specs(C, g)
    sd = _up_sd(C, r, g)
    usp = E.spec_up(sd, "u", r, True)
    saved = E._PREP_STATUS
    if status is not None:
        E._PREP_STATUS = status.data_ptr() + 4
    try:
        cws = [E.make_conv(sp, DEV, prec=prec) for sp in specs]
        rc = E.make_conv(usp, DEV, prec=prec)
        fused = E.prep_fused(specs, C, prec, DEV)
    finally:
        E._PREP_STATUS = saved
    up = E.prep_up_fused(usp, prec, rc.bias, DEV)
    assert fused is not None and up is not None and rc.fir is not None
    return specs, sd, E.BlockW(C, "none", None, *cws, None, fused), rc, up


def _run(bw, rc, up, h, skip, out_len, fused, y_fill=None, **kw):
    """The block on h and the up conv into a copy of ``skip`` (added in place)."""
    B, C, T = h.shape
    r = up.rate
    ha = E.Act(h.to(DEV))
    out = E.new_act(B, C, T, DEV)
    out.t.zero_()
    v = E.new_act(B, C // 2, out_len, DEV)
    v.t.zero_()
    tA, tB = E.new_act(B, C, T, DEV), E.new_act(B, C, T, DEV)
    d_up = E.conv_desc(rc, out, v, n_frames=T, out_len=out_len, valid_len=r * T, res1=v, s1=E.NF2)
    prog = L.Program()
    did = E.rec_block(prog, bw, ha, out, tA, tB, up=(up, d_up) if fused else None, store_out=not fused, **kw)
    assert bool(did) == fused
    if not fused:
        E.add_conv(prog, d_up)
    kinds = prog.op_kinds()
    # the buffers get their contents after recording: where an earlier test left a conv tuner
    # on, recording times the up conv on these very buffers, and it adds into v in place
    v.t.copy_(skip)
    if y_fill is not None:
        out.t.fill_(y_fill)
    prog.run(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return v.t.cpu(), out.t.cpu(), kinds


CASES = [(64, 2, 119), (64, 2, 58), (64, 2, 3), (128, 4, 53), (128, 4, 26), (128, 4, 3)]


@pytest.mark.parametrize("prec", [1, 2])
@pytest.mark.parametrize("C,r,T", CASES)
def test_block_fused_up(C, r, T, prec):
    g = torch.Generator().manual_seed(C + r + T)
    status = torch.zeros(4, dtype=torch.int32, device=DEV)
    specs, sd, bw, rc, up = _prep(C, r, prec, g, status)
    assert L.load().ou_block_frames(C) - 2 in (58, 26)
    B = 2
    h = torch.randn(B, C, T, generator=g)
    sc = torch.randn(B, C, T, generator=g)
    film = 1.0 + 0.3 * torch.randn(B, 2 * C, generator=g)
    filmd = film.to(DEV)
    tol = 1e-5 if prec == 1 else 3e-3
    # the full output, and once the crop level_lengths' ceil produces
    for out_len in ([r * T, r * T - 1] if (C, T) == (64, 119) or (C, T) == (128, 53) else [r * T]):
        skip = torch.randn(B, C // 2, out_len, generator=g)
        for cond in (False, True):
            kw = dict(sc=E.Act(sc.to(DEV)), film=filmd.data_ptr(), film_bs=2 * C) if cond else {}
            uf, yf, kf = _run(bw, rc, up, h, skip, out_len, True, y_fill=SENTINEL, **kw)
            uu, yu, ku = _run(bw, rc, up, h, skip, out_len, False, **kw)
            assert kf.count(L.OP_BLOCK) == 1 and kf.count(L.OP_CONV) == 0
            assert ku.count(L.OP_BLOCK) == 1 and ku.count(L.OP_CONV) == 1
            assert bool((yf == SENTINEL).all()), "the block output was stored although y is NULL"
            y_ref, _ = _ref(specs, h.double(), sc.double() if cond else None, film.double() if cond else None)
            u_ref = _up_ref(sd, r, y_ref, skip.double(), out_len, r * T)
            e_ref, e_unf = _rel(uf, u_ref), _rel(uf, uu)
            print(f"C {C} r {r} T {T} prec {prec} out_len {out_len} cond {cond}: vs f64 {e_ref:.2e}, "
                  f"vs unfused {e_unf:.2e}, unfused vs f64 {_rel(uu, u_ref):.2e}")
            assert e_ref < tol
            assert e_unf < tol
    assert int(status.abs().sum()) == 0


def test_block_fused_up_stores_y_when_asked():
    """With a y buffer the block output is stored too, as without the stage."""
    C, r, T = 64, 2, 119
    g = torch.Generator().manual_seed(5)
    specs, sd, bw, rc, up = _prep(C, r, 1, g)
    h = torch.randn(2, C, T, generator=g)
    skip = torch.randn(2, C // 2, r * T, generator=g)
    B = 2
    ha, out, v = E.Act(h.to(DEV)), E.new_act(B, C, T, DEV), E.Act(skip.to(DEV).clone())
    d_up = E.conv_desc(rc, out, v, n_frames=T, out_len=r * T, valid_len=r * T, res1=v, s1=E.NF2)
    prog = L.Program()
    assert E.rec_block(prog, bw, ha, out, out, E.new_act(B, C, T, DEV), up=(up, d_up), store_out=True)
    prog.run(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    y_ref, _ = _ref(specs, h.double())
    assert _rel(out.t, y_ref) < 1e-5
    assert _rel(v.t, _up_ref(sd, r, y_ref, skip.double(), r * T, r * T)) < 1e-5


def test_block_fused_up_range_flag():
    """A block output beyond the up conv's staging range sets range code 16."""
    C, r, T = 64, 2, 119
    g = torch.Generator().manual_seed(2)
    status = torch.zeros(4, dtype=torch.int32, device=DEV)
    specs, sd, bw, rc, up = _prep(C, r, 1, g, status)
    h = 0.01 * torch.randn(1, C, T, generator=g)
    # the residual path carries h to y = (h + c3) / sqrt 2: 4e6 / sqrt 2 * 2^-6 = 44194 >= 2^15 at the
    # up conv's staging (finite in f16); conv1's own staging trips its code 1 too
    h[0, 3, 50] = 4.0e6
    skip = torch.zeros(1, C // 2, r * T)
    _run(bw, rc, up, h, skip, r * T, True)
    assert int(status[1]) & 16


def test_decoder_up_fused_equal_unfused(monkeypatch):
    """The score decoder's two eligible up convs fused into the preceding
    blocks give the same enhance as separate launches, the score network
    still matches the reference's output, and the plan has at least two fewer
    ops per score pass."""
    from conftest import golden_state_dict, load_golden
    from open_universe_amd.configs import get_config
    from open_universe_amd.networks.universe import UniverseGAN

    d = load_golden("pp16")
    outs, nops, nblk = {}, {}, {}
    for fuse in ("1", "0"):
        monkeypatch.setenv("OUHIP_FUSE_UP", fuse)
        cfg = get_config("pp16", None)
        m = UniverseGAN(**{k: v for k, v in cfg.items() if k != "_target_"})
        m.load_state_dict(golden_state_dict(d), strict=False)
        m = m.to(DEV).eval()
        mix = torch.from_numpy(d["enh_mix"]).to(DEV)
        with torch.no_grad():
            outs[fuse] = m.enhance(mix[:, 0], rng=torch.Generator().manual_seed(1028282)).cpu()
            sc = m.get_score_model()(torch.from_numpy(d["score_x"]).to(DEV), torch.from_numpy(d["score_sigma"]).to(DEV),
                                     [torch.from_numpy(d[f"cond_out{i}"]).to(DEV) for i in range(5)]).cpu()
        plan = next(iter(m._plans.values()))
        nops[fuse] = len(plan.prog)
        nblk[fuse] = sum(1 for op, dd in zip(plan.prog.op_kinds(), plan.prog.descs) if op == L.OP_BLOCK and dd.w_up)
        steps = max(1, nblk["1"] // 2)
        assert _rel(sc, torch.from_numpy(d["score_out"])) < 1e-4
    print(f"ops fused {nops['1']} unfused {nops['0']}, blocks with the stage {nblk['1']}, "
          f"enhance fused vs unfused {_rel(outs['1'], outs['0']):.2e}")
    assert _rel(outs["1"], outs["0"]) < 1e-5
    assert nblk["0"] == 0 and nblk["1"] >= 2 and nblk["1"] % 2 == 0
    assert nops["1"] <= nops["0"] - 2 * steps
