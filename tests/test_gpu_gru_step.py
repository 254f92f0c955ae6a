"""The straight-line step loop of the k-split GRU kernel (the default for one
item per chain) against the earlier loop (ou_gru_desc.flags bit9), bit for
bit, and against torch.nn.GRU.

The T values straddle the LDS chunk size (CS = 128 at 4 units per wave, 64 at
8): the staged gi / residual chunk is reloaded at every chunk boundary, right
after the boundary step's granule store, and the first and last steps are
peeled, so T = CS - 1, CS, CS + 1 and 2 CS + 3 cover a boundary on the last
step, right before it, and two reloads plus a ragged tail.  Every case runs
with and without a residual (the loop is compiled once per combination).
Inputs and weights are synthetic."""
import pytest
import torch

from conftest import rel_rms
from open_universe_amd import _lib as L
from open_universe_amd import engine as E
from open_universe_amd.utils.synthetic import synth_tensor

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NEW, LEGACY, UW8 = 1, 1 | 512, 128   # flags: bit0 XCD-local chains (the default), bit9, bit7


def _state_dict(H):
    sd = {}
    for sfx in ("", "_reverse"):
        for kind, shape in (("weight_ih", (3 * H, 2 * H)), ("weight_hh", (3 * H, H)),
                            ("bias_ih", (3 * H,)), ("bias_hh", (3 * H,))):
            n = f"gru_step_h{H}.{kind}_l0{sfx}"
            sd[n] = synth_tensor(n, shape)
    return sd


_GW = {}


def _gw(H):
    if H not in _GW:
        sd = _state_dict(H)
        _GW[H] = (sd, E.prep_gru(sd, f"gru_step_h{H}", 1, DEV))
    return _GW[H]


def _inputs(H, B, T):
    x = torch.randn(B, 2 * H, T, generator=torch.Generator().manual_seed(100 + T)) * 0.5
    res = torch.randn(B, 2 * H, T, generator=torch.Generator().manual_seed(200 + T))
    return x, res


def _run(H, x, flags, res=None, pad=0, ws_zeroed=False, gran=None):
    """One launch; returns (y (B, 2H, T) on the CPU, the whole padded y buffer, workspace)."""
    gw = _gw(H)[1]
    B, _, T = x.shape
    status = torch.zeros(4, dtype=torch.int32, device=DEV)
    if gran is None:
        gran = torch.zeros(L.load().ou_gru_workspace_bytes(H, B) // 8, dtype=torch.int64, device=DEV)
    ybuf = torch.full((B, 2 * H, T + pad), -7.25, device=DEV)
    xa, gi, y = E.Act(x.to(DEV)), E.new_act(B, 6 * H, T, DEV), E.Act(ybuf[:, :, :T])
    saved = E.GRU_FLAGS, E._GRU_WS_ZEROED, L.TUNER
    E.GRU_FLAGS, E._GRU_WS_ZEROED, L.TUNER = flags, ws_zeroed, None   # the library's default tile: no tuning runs
    try:
        prog = L.Program()
        kw = {} if res is None else dict(res=E.Act(res.to(DEV)), res_scale=0.5)
        E.rec_gru(prog, gw, 0, xa, gi, y, gran, status, **kw)
        prog.run(torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    finally:
        E.GRU_FLAGS, E._GRU_WS_ZEROED, L.TUNER = saved
    assert int(status.abs().sum()) == 0
    return ybuf[:, :, :T].cpu(), ybuf.cpu(), gran


def _same(H, B, T, extra=0):
    x, res = _inputs(H, B, T)
    for r in (None, res):
        new = _run(H, x, NEW | extra, r)[0]
        old = _run(H, x, LEGACY | extra, r)[0]
        assert torch.isfinite(new).all() and float(new.abs().max()) > 1e-3
        assert torch.equal(new, old), (H, B, T, r is not None)


@pytest.mark.parametrize("T", [5, 127, 128, 129, 259])
@pytest.mark.parametrize("H", [64, 256, 512])
def test_new_loop_equals_legacy_loop(H, T):
    _same(H, 1, T)


def test_new_loop_equals_legacy_loop_several_chains():
    _same(256, 3, 129)


def test_several_items_per_chain():
    """A batch that launch_ks_uw gives two items per chain (NB = 2): more
    chains at one item each than fit the residency rule at 8 units per wave.
    Several items per chain keep the earlier loop, whatever bit9 says."""
    H = 256
    G8 = H // (8 * 4)                                       # workgroups per chain, 8 units per wave
    B = L.load().ou_gru_ks_max_workgroups() // (2 * G8) + 1   # 2 * B * G8 > the limit: nb = 2
    assert 2 * -(-B // 2) * G8 <= L.load().ou_gru_ks_max_workgroups()
    _same(H, B, 9)


@pytest.mark.parametrize("T", [63, 64, 65])
def test_new_loop_equals_legacy_loop_8_units_per_wave(T):
    _same(256, 1, T, extra=UW8)


def test_strided_output_keeps_the_padding():
    """y_cstride > T (a strided output view): the loop honours the stride and
    writes nothing past column T - 1."""
    H, T, pad = 256, 129, 31
    x, res = _inputs(H, 1, T)
    for r in (None, res):
        y, ybuf, _ = _run(H, x, NEW, r, pad=pad)
        assert torch.equal(ybuf[:, :, T:], torch.full((1, 2 * H, pad), -7.25))
        assert torch.equal(y, _run(H, x, LEGACY, r)[0])


_REF = {}


def _torch_gru(H, x):
    """torch.nn.GRU in float64 on the CPU, (B, 2H, T)."""
    sd = _gw(H)[0]
    m = torch.nn.GRU(2 * H, H, batch_first=True, bidirectional=True).double()
    m.load_state_dict({k.split(".", 1)[1]: v.double() for k, v in sd.items()})
    with torch.no_grad():
        return m(x.double().transpose(1, 2))[0].transpose(1, 2)


@pytest.mark.parametrize("T", [129, 801])
def test_new_loop_vs_torch_gru(T):
    """Tolerance: the GRU layer bound of test_gru_layers_vs_torch_gru
    (rel-RMS <= 1e-5)."""
    H = 256
    x, res = _inputs(H, 1, T)
    if T not in _REF:
        _REF[T] = _torch_gru(H, x)
    ref = _REF[T]
    assert rel_rms(_run(H, x, NEW)[0].double(), ref) < 1e-5
    assert rel_rms(_run(H, x, NEW, res)[0].double(), (ref + res.double()) * 0.5) < 1e-5


@pytest.mark.parametrize("Ts", [(5, 5, 5), (6, 6, 6), (5, 6, 5), (6, 5, 6)])
def test_ws_zeroed_back_to_back_leaves_the_workspace_as_the_legacy_loop(Ts):
    """Launches that skip the per-launch memset on one workspace zeroed once
    (as test_gru_ws_zeroed_short_launches_back_to_back): each equals the same
    layer run alone, and the workspace -- placement slots cleared, the tags
    T - 1 and T - 2 in the parity slots -- ends as the earlier loop leaves it."""
    H, B = 256, 2
    xs = [_inputs(H, B, T + 10 * i)[0][:, :, :T].contiguous() for i, T in enumerate(Ts)]

    def chain(flags):
        gran = torch.zeros(L.load().ou_gru_workspace_bytes(H, B) // 8, dtype=torch.int64, device=DEV)
        outs = [_run(H, x, flags, ws_zeroed=True, gran=gran)[0] for x in xs]
        return outs, gran.cpu()

    new, ws_new = chain(NEW)
    old, ws_old = chain(LEGACY)
    for x, yn, yo in zip(xs, new, old):
        assert torch.equal(yn, _run(H, x, NEW)[0])
        assert torch.equal(yn, yo)
    slots = ws_new[B * 4 * H:B * 4 * H + B * H // 4]
    assert int(slots.abs().sum()) == 0
    assert torch.equal(ws_new, ws_old)
