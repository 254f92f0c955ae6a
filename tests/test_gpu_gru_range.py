"""ou_gru launched alone (L.GruDesc by hand, L.run_now): step ranges
[t_begin, t_end), the carried state ``hstate``, every hidden size, and both
step loops of the k-split kernel plus the gather kernel against float64 per
element.  ``gi`` is written directly: no input projection runs.

Inputs come from seeded generators: w_hh uniform in +-2/sqrt(H), b_hh uniform
in +-1/sqrt(H), gi ~ N(0, 1), residual ~ N(0, 1) at res_scale 0.5.  With
these the recurrent state matters: zeroing w_hh moves the float64 output by
37 % (rel. norm), and continuing a range from a zero state is off by up to
0.7 in the columns after the seam.

The checks (``check_ranges``, ``check_vs_f64``) take a backend: ``Gpu`` is the
kernel, ``Sim`` a float32 restatement of ou_gru's range semantics on the CPU.
``test_checks_catch_mutants`` (no GPU needed) pushes wrong versions of ``Sim``
through the same checks and asserts that each is caught.

Per-element bound of ``check_vs_f64``, in the style of tests/test_gpu_misc.py:
max |kernel - float64| <= F x max(max |float32 restatement - float64|,
2^-23 max |float64|) of the same case, F = 4, the factor of that file.  No
case needs more.  Worst measured ratio err / yardstick per case on an MI355X
(over y and hstate, with and without the residual; T = 131, B = 2; the
yardsticks are 1.1e-7 .. 4.8e-7):

  straight-line loop, 4 units per wave   H = 64: 1.45   128: 1.43   256: 1.14
                                         H = 384: 0.85  512: 1.21
  straight-line loop, 8 units per wave   H = 256: 1.14
  earlier loop (bit 9)                   H = 256: 1.14
  gather kernel                          H = 32: 1.00   H = 256, bit 5 alone,
                                         bit 5 | 2 and bit 5 | 3: 0.83
  T == 1 (no placement handshake)        H = 256: 1.07

The CPU mutant tanh + 1e-6 lands at ratio 22 on the same check and at rel-RMS
below 1e-5, the bound of the older tests.
"""
import ctypes
import math

import pytest
import torch

from conftest import rel_rms
from open_universe_amd import _lib as L

gpu = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
DEFAULT, NEW, LEGACY, UW8, GATHER = -1, 1, 1 | 512, 128, 32   # ou_gru_desc.flags (bit0 is the default layout)
SENTINEL, HS_FILL, RES_SCALE = -7.25, 3.5, 0.5
FACTOR = 4   # check_vs_f64: see the module docstring


# ----------------------------------------------------------------------------
# inputs and the reference
# ----------------------------------------------------------------------------
class Case:
    _cache = {}

    def __init__(self, H, B, T):
        g = torch.Generator().manual_seed(7919 * H + 131 * B + T)
        self.H, self.B, self.T = H, B, T
        self.w_hh = (torch.rand(2, 3 * H, H, generator=g) * 2 - 1) * (2 / math.sqrt(H))
        self.b_hh = (torch.rand(2, 3 * H, generator=g) * 2 - 1) / math.sqrt(H)
        self.gi = torch.randn(B, 6 * H, T, generator=g)
        self.res = torch.randn(B, 2 * H, T, generator=g)
        self._ref, self._dev = {}, None

    @classmethod
    def get(cls, H, B, T):
        key = (H, B, T)
        if key not in cls._cache:
            cls._cache[key] = cls(H, B, T)
        return cls._cache[key]

    def ref(self, dtype):
        """(y, y with the residual, h_n) of the whole sequence in ``dtype``; computed once."""
        if dtype not in self._ref:
            y, h_n = ref_gru(self.gi, self.w_hh, self.b_hh, dtype)
            self._ref[dtype] = (y, (y + self.res.to(dtype)) * RES_SCALE, h_n)
        return self._ref[dtype]

    def dev(self):
        if self._dev is None:
            self._dev = {k: getattr(self, k).to(DEV).contiguous() for k in ("w_hh", "b_hh", "gi", "res")}
        return self._dev


def gru_step(h, gi_t, w, b, tanh=torch.tanh):
    """One step of ou_gru.hip's header comment (torch gate order r, z, n):
    h (B, H), gi_t (B, 3H), w (3H, H), b (3H,)."""
    H = h.shape[1]
    gh = h @ w.t() + b
    r = torch.sigmoid(gi_t[:, :H] + gh[:, :H])
    z = torch.sigmoid(gi_t[:, H:2 * H] + gh[:, H:2 * H])
    n = tanh(gi_t[:, 2 * H:] + r * gh[:, 2 * H:])
    return (1 - z) * n + z * h


def ref_gru(gi, w_hh, b_hh, dtype, tanh=torch.tanh):
    """The recurrence in ``dtype``: gi (B, 2*3H, T), w_hh (2, 3H, H), b_hh
    (2, 3H) -> y (B, 2H, T), h_n (B, 2, H).  The backward direction walks
    time T - 1 ... 0."""
    gi, w_hh, b_hh = gi.to(dtype), w_hh.to(dtype), b_hh.to(dtype)
    B, _, T = gi.shape
    H = w_hh.shape[2]
    y = torch.zeros(B, 2 * H, T, dtype=dtype)
    h_n = torch.zeros(B, 2, H, dtype=dtype)
    for dr in range(2):
        h = torch.zeros(B, H, dtype=dtype)
        for t in range(T):
            tm = t if dr == 0 else T - 1 - t
            h = gru_step(h, gi[:, dr * 3 * H:(dr + 1) * 3 * H, tm], w_hh[dr], b_hh[dr], tanh)
            y[:, dr * H:(dr + 1) * H, tm] = h
        h_n[:, dr] = h
    return y, h_n


# ----------------------------------------------------------------------------
# backends: launch(case, bufs, tb, te, ...) -> (whole y buffer, hstate) on the CPU
# ----------------------------------------------------------------------------
class Gpu:
    def bufs(self, case, pad=0, ws=None, hstate=True):
        H, B, T = case.H, case.B, case.T
        if ws is None:
            ws = torch.zeros(L.load().ou_gru_workspace_bytes(H, B) // 8, dtype=torch.int64, device=DEV)
        return dict(y=torch.full((B, 2 * H, T + pad), SENTINEL, device=DEV), ws=ws,
                    hstate=torch.full((B, 2, H), HS_FILL, device=DEV) if hstate else None,
                    status=torch.zeros(4, dtype=torch.int32, device=DEV))

    def desc(self, case, bufs, tb, te, flags=DEFAULT, use_res=False, ws_zeroed=0):
        H, B, T = case.H, case.B, case.T
        dv, y = case.dev(), bufs["y"]
        d = L.GruDesc()
        d.gi, d.gi_bstride = dv["gi"].data_ptr(), 6 * H * T
        d.w_hh, d.b_hh = dv["w_hh"].data_ptr(), dv["b_hh"].data_ptr()
        d.y, d.y_bstride, d.y_cstride = y.data_ptr(), y.stride(0), y.stride(1)
        if use_res:
            d.res, d.res_bstride, d.res_cstride, d.res_scale = dv["res"].data_ptr(), 2 * H * T, T, RES_SCALE
        d.hidden, d.steps, d.batch, d.flags = H, T, B, flags
        d.granules, d.status = bufs["ws"].data_ptr(), bufs["status"].data_ptr()
        d.t_begin, d.t_end = tb, te
        d.hstate = bufs["hstate"].data_ptr() if bufs["hstate"] is not None else None
        d.ws_zeroed = ws_zeroed
        return d

    def launch(self, case, bufs, tb, te, **kw):
        L.run_now(L.OP_GRU, self.desc(case, bufs, tb, te, **kw), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert int(bufs["status"].abs().sum()) == 0, "ou_gru set *status (hand-off timeout)"
        return bufs["y"].cpu(), bufs["hstate"].cpu() if bufs["hstate"] is not None else None


class Sim:
    """ou_gru's range semantics restated in float32 on the CPU.  ``mutant``
    selects one deliberate error (test_checks_catch_mutants)."""
    MUTANTS = ("zero_state", "other_dir_state", "bwd_cols", "hstate_early", "res_in_state", "tanh_eps")

    def __init__(self, mutant=None):
        assert mutant is None or mutant in self.MUTANTS
        self.mutant = mutant

    def bufs(self, case, pad=0, ws=None, hstate=True):
        H, B, T = case.H, case.B, case.T
        return dict(y=torch.full((B, 2 * H, T + pad), SENTINEL), ws=torch.zeros(1, dtype=torch.int64),
                    hstate=torch.full((B, 2, H), HS_FILL) if hstate else None)

    def launch(self, case, bufs, tb, te, flags=DEFAULT, use_res=False, ws_zeroed=0):
        H, B, T, m = case.H, case.B, case.T, self.mutant
        te = te or T
        split = tb != 0 or te != T
        tanh = (lambda v: torch.tanh(v) + 1e-6) if m == "tanh_eps" else torch.tanh
        y, hs = bufs["y"], bufs["hstate"]
        h_in = hs.clone() if hs is not None else None
        for dr in range(2):
            h = torch.zeros(B, H)
            if tb > 0 and m != "zero_state":
                h = h_in[:, 1 - dr if m == "other_dir_state" else dr].clone()
            before_last = h
            for t in range(tb, te):
                tm = t if dr == 0 else T - 1 - t
                before_last = h
                h = gru_step(h, case.gi[:, dr * 3 * H:(dr + 1) * 3 * H, tm], case.w_hh[dr], case.b_hh[dr], tanh)
                out = (h + case.res[:, dr * H:(dr + 1) * H, tm]) * RES_SCALE if use_res else h
                y[:, dr * H:(dr + 1) * H, t if (m == "bwd_cols" and split and dr == 1) else tm] = out
                if m == "res_in_state":
                    h = out
            if hs is not None:
                hs[:, dr] = before_last if m == "hstate_early" else h
        return y.clone(), hs.clone() if hs is not None else None


# ----------------------------------------------------------------------------
# the checks
# ----------------------------------------------------------------------------
def check_ranges(be, case, cuts, flags=DEFAULT, pad=0):
    """1a + 1b: launches [c_i, c_i+1) in order on one y / hstate / workspace
    (ws_zeroed = 0) against the single whole launch, with and without the
    residual.  Returns {use_res: (y, hstate)} of the whole launches."""
    H, B, T = case.H, case.B, case.T
    assert cuts[0] == 0 and cuts[-1] == T and all(b - a >= 2 for a, b in zip(cuts, cuts[1:]))
    whole, states = {}, {}
    for use_res in (False, True):
        yw, hw = be.launch(case, be.bufs(case, pad), 0, 0, flags=flags, use_res=use_res)
        assert torch.isfinite(yw[:, :, :T]).all() and float(yw[:, :, :T].abs().max()) > 1e-3
        assert torch.equal(yw[:, :, T:], torch.full((B, 2 * H, pad), SENTINEL))
        whole[use_res] = (yw, hw)
        bufs = be.bufs(case, pad)
        prev = torch.full((B, 2 * H, T + pad), SENTINEL)
        states[use_res] = []
        for tb, te in zip(cuts, cuts[1:]):
            y, hs = be.launch(case, bufs, tb, te, flags=flags, use_res=use_res)
            # nothing outside this launch's columns moved: forward rows
            # [tb, te), backward rows [T - te, T - tb)
            mine = torch.zeros(B, 2 * H, T + pad, dtype=torch.bool)
            mine[:, :H, tb:te] = True
            mine[:, H:, T - te:T - tb] = True
            assert torch.equal(y[~mine], prev[~mine]), (cuts, tb, te, use_res, "wrote outside its columns")
            assert not (y[mine] == SENTINEL).any(), (cuts, tb, te, use_res, "left a column unwritten")
            if not use_res:   # hstate is h of the range's last step
                assert torch.equal(hs[:, 0], y[:, :H, te - 1]), (cuts, tb, te, "forward hstate")
                assert torch.equal(hs[:, 1], y[:, H:, T - te]), (cuts, tb, te, "backward hstate")
            states[use_res].append(hs)
            prev = y
        assert torch.equal(prev, yw), (cuts, use_res, "ranges differ from the whole launch")
        assert torch.equal(states[use_res][-1], hw), (cuts, use_res, "hstate differs from the whole launch")
    # the whole launch too; and the residual never enters the carried state
    assert torch.equal(whole[False][1][:, 0], whole[False][0][:, :H, T - 1])
    assert torch.equal(whole[False][1][:, 1], whole[False][0][:, H:, 0])
    assert torch.equal(whole[True][1], whole[False][1]), "residual leaked into hstate (whole launch)"
    for i, (a, b) in enumerate(zip(states[True], states[False])):
        assert torch.equal(a, b), (cuts, i, "residual leaked into hstate")
    return whole


RATIOS = {}   # what -> measured err / yardstick (printed; the module docstring records the MI355X's)


def close(what, got, ref64, ref32, factor):
    """max|got - ref64| <= factor * max(max|ref32 - ref64|, 2^-23 max|ref64|)."""
    got = got.to(F64)
    assert torch.isfinite(got).all(), what
    err = (got - ref64).abs().max().item()
    yard = max((ref32.to(F64) - ref64).abs().max().item(), 2.0 ** -23 * ref64.abs().max().item())
    RATIOS[what] = err / yard
    print(f"gru-ratio {what} err {err:.3e} yardstick {yard:.3e} ratio {err / yard:.3f}")
    assert err <= factor * yard, f"{what}: err {err:.3e} > {factor} x {yard:.3e} (ratio {err / yard:.2f})"


def check_vs_f64(be, case, name, flags=DEFAULT, hstate=True):
    """1d: a whole launch against float64 per element, with and without the
    residual; hstate against h_n where the kernel writes it.  Returns y
    without the residual."""
    T, factor = case.T, FACTOR
    r64, r32 = case.ref(F64), case.ref(F32)
    out = None
    for use_res in (False, True):
        y, hs = be.launch(case, be.bufs(case, hstate=hstate), 0, 0, flags=flags, use_res=use_res)
        close(f"{name} res={int(use_res)} y", y[:, :, :T], r64[use_res], r32[use_res], factor)
        if hstate:
            close(f"{name} res={int(use_res)} hstate", hs, r64[2], r32[2], factor)
        out = y if out is None else out
    return out


# ----------------------------------------------------------------------------
# 1a / 1b: ranges equal the whole launch; hstate is the last state
# ----------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("cuts", [(0, 2, 129, 257, 386), (0, 5, 386)])
def test_ranges_4_units_per_wave_both_loops(cuts):
    """CS = 128: pieces of 2, CS - 1, CS, CS + 1 steps, the last ending at T;
    and one piece of 2 CS + 125 steps that starts off a chunk boundary (two
    chunk reloads relative to t_begin).  Both loops, same bits."""
    case = Case.get(256, 1, 386)
    new = check_ranges(Gpu(), case, cuts, NEW)
    old = check_ranges(Gpu(), case, cuts, LEGACY)
    for r in (False, True):
        assert torch.equal(new[r][0], old[r][0]) and torch.equal(new[r][1], old[r][1])


@gpu
def test_ranges_8_units_per_wave_both_loops():
    case, cuts = Case.get(256, 1, 194), (0, 2, 65, 129, 194)   # CS = 64
    new = check_ranges(Gpu(), case, cuts, NEW | UW8)
    old = check_ranges(Gpu(), case, cuts, LEGACY | UW8)
    for r in (False, True):
        assert torch.equal(new[r][0], old[r][0]) and torch.equal(new[r][1], old[r][1])


@gpu
@pytest.mark.parametrize("H", [64, 128, 256, 384, 512])
def test_ranges_every_hidden_size(H):
    check_ranges(Gpu(), Case.get(H, 1, 140), (0, 3, 131, 140), NEW)


@gpu
def test_ranges_several_chains():
    check_ranges(Gpu(), Case.get(256, 3, 140), (0, 3, 131, 140))


@gpu
def test_ranges_several_items_per_chain():
    """A batch that launch_ks_uw gives two items per chain (as
    test_gpu_gru_step.test_several_items_per_chain): the earlier loop, NB = 2."""
    H = 256
    G8 = H // (8 * 4)
    B = L.load().ou_gru_ks_max_workgroups() // (2 * G8) + 1
    assert 2 * -(-B // 2) * G8 <= L.load().ou_gru_ks_max_workgroups()
    check_ranges(Gpu(), Case.get(H, B, 11), (0, 2, 7, 11))


@gpu
def test_ranges_strided_output_keeps_the_padding():
    """y_cstride = T + 31: no range writes a padding column (check_ranges
    compares the whole buffer, padding included, after every launch)."""
    check_ranges(Gpu(), Case.get(256, 1, 140), (0, 3, 131, 140), NEW, pad=31)


# ----------------------------------------------------------------------------
# 1c: one workspace zeroed once, ws_zeroed = 1 throughout
# ----------------------------------------------------------------------------
@gpu
def test_ranges_and_whole_launches_share_a_zeroed_workspace():
    H, B = 256, 2
    be = Gpu()
    ws = torch.zeros(L.load().ou_gru_workspace_bytes(H, B) // 8, dtype=torch.int64, device=DEV)
    for T, cuts in ((9, (0, 9)), (140, (0, 3, 131, 140)), (6, (0, 6)), (7, (0, 2, 7))):
        case = Case.get(H, B, T)

        def seq(ws, ws_zeroed):
            bufs = be.bufs(case, ws=ws)
            for tb, te in zip(cuts, cuts[1:]):
                out = be.launch(case, bufs, tb, te if len(cuts) > 2 else 0, use_res=True, ws_zeroed=ws_zeroed)
            return out

        y, hs = seq(ws, 1)
        y1, hs1 = seq(None, 0)
        assert torch.equal(y, y1) and torch.equal(hs, hs1), (T, cuts)
        assert not (y == SENTINEL).any()
    slots = ws.cpu()[B * 4 * H:B * 4 * H + B * H // 4]
    assert int(slots.abs().sum()) == 0


# ----------------------------------------------------------------------------
# 1d: per element against float64
# ----------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("H", [64, 128, 256, 384, 512])
def test_new_loop_vs_float64_per_element(H):
    check_vs_f64(Gpu(), Case.get(H, 2, 131), f"new H={H}", NEW)


@gpu
def test_8_units_per_wave_and_the_earlier_loop_vs_float64_per_element():
    case = Case.get(256, 2, 131)
    check_vs_f64(Gpu(), case, "new uw8 H=256", NEW | UW8)
    check_vs_f64(Gpu(), case, "legacy H=256", LEGACY)


@gpu
@pytest.mark.parametrize("H,flags", [(32, DEFAULT), (256, GATHER), (256, GATHER | 4), (256, GATHER | 8)])
def test_gather_kernel_vs_float64_per_element(H, flags):
    """H = 32 has no other kernel; at H = 256 bit 5 selects the gather kernel
    at 32-, 64- (bit 2) and 128-unit (bit 3) workgroups.  It writes no hstate."""
    check_vs_f64(Gpu(), Case.get(H, 2, 131), f"gather H={H} flags={flags}", flags, hstate=False)


# ----------------------------------------------------------------------------
# 2: one-step launches
# ----------------------------------------------------------------------------
@gpu
def test_one_step_whole_launch():
    """T == 1 runs without the placement handshake (ou_gru sets flags bit 6):
    against float64, status 0 (Gpu.launch)."""
    H, B = 256, 2
    case, be = Case.get(H, B, 1), Gpu()
    y = check_vs_f64(be, case, "T=1 H=256", DEFAULT)
    bufs = be.bufs(case)
    y2, hs = be.launch(case, bufs, 0, 0)
    assert torch.equal(y2, y)
    assert torch.equal(hs[:, 0], y[:, :H, 0]) and torch.equal(hs[:, 1], y[:, H:, 0])


@gpu
def test_one_step_range_from_zero_then_the_rest():
    """A one-step range is allowed at t_begin == 0 (it reads no hstate)."""
    case, be = Case.get(256, 2, 9), Gpu()
    yw, hw = be.launch(case, be.bufs(case), 0, 0, use_res=True)
    bufs = be.bufs(case)
    y, hs = be.launch(case, bufs, 0, 1, use_res=True)
    assert torch.equal(y[:, :256, :1], yw[:, :256, :1]) and torch.equal(y[:, 256:, 8:], yw[:, 256:, 8:])
    assert (y[:, :256, 1:] == SENTINEL).all() and (y[:, 256:, :8] == SENTINEL).all()
    y, hs = be.launch(case, bufs, 1, 9, use_res=True)
    assert torch.equal(y, yw) and torch.equal(hs, hw)


# ----------------------------------------------------------------------------
# 1e: refusals (host checks: ou_gru returns before any HIP call)
# ----------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("what,H,tb,te,flags,hstate", [
    ("t_begin < 0", 256, -1, 4, DEFAULT, True),
    ("t_end <= t_begin", 256, 4, 4, DEFAULT, True),
    ("t_end < t_begin", 256, 4, 2, DEFAULT, True),
    ("t_end > steps", 256, 2, 10, DEFAULT, True),
    ("t_begin >= steps, t_end = 0", 256, 9, 0, DEFAULT, True),
    ("a range without hstate", 256, 2, 6, DEFAULT, False),
    ("a range at H = 32", 32, 2, 6, DEFAULT, True),
    ("a range on the gather kernel", 256, 2, 6, GATHER, True),
    ("a continuing range of one step", 256, 5, 6, DEFAULT, True),
    ("a continuing range of one step, t_end = 0", 256, 8, 0, DEFAULT, True),
])
def test_refusals(what, H, tb, te, flags, hstate):
    be, case = Gpu(), Case.get(H, 1, 9)
    bufs = be.bufs(case, hstate=hstate)
    lib = L.load()
    rc = lib.ou_gru(ctypes.byref(be.desc(case, bufs, tb, te, flags=flags)),
                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    msg = lib.ou_last_error()
    assert rc < 0 and msg and b"gru:" in msg, (what, rc, msg)
    torch.cuda.synchronize()
    assert (bufs["y"] == SENTINEL).all() and int(bufs["status"].abs().sum()) == 0, what


# ----------------------------------------------------------------------------
# 1f: the checks above catch a wrong kernel (CPU only)
# ----------------------------------------------------------------------------
def _fails(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


def test_checks_catch_mutants():
    """Sim passes check_ranges and check_vs_f64; each mutant of it fails the
    check that is there for it.  tanh + 1e-6 fails the per-element bound while
    it passes the rel-RMS 1e-5 of the older tests."""
    ra, rd = Case.get(64, 1, 140), Case.get(64, 2, 131)
    cuts = (0, 3, 131, 140)
    check_ranges(Sim(), ra, cuts)
    check_vs_f64(Sim(), rd, "sim")
    assert RATIOS["sim res=0 y"] <= 1.0 and RATIOS["sim res=0 hstate"] <= 1.0
    expect = {"zero_state": (True, False), "other_dir_state": (True, False), "bwd_cols": (True, False),
              "hstate_early": (True, True), "res_in_state": (True, True), "tanh_eps": (False, True)}
    for m in Sim.MUTANTS:
        got = (_fails(lambda: check_ranges(Sim(m), ra, cuts)), _fails(lambda: check_vs_f64(Sim(m), rd, m)))
        print(f"gru-mutant {m}: check_ranges {'fails' if got[0] else 'passes'}, "
              f"check_vs_f64 {'fails' if got[1] else 'passes'}")
        assert got == expect[m], (m, got)
    y = Sim("tanh_eps").launch(rd, Sim().bufs(rd), 0, 0)[0]
    assert rel_rms(y.double(), rd.ref(F64)[0]) < 1e-5
