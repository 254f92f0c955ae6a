"""hazards.footprint against what the kernels really read and write.

Each recorded plan is stepped op by op (tests/footprint_check.py): a word an
op changes outside its write boxes, or a poisoned word outside its read and
write boxes that changes its result, fails the plan's test and names the op,
the descriptor field and the bytes.  Everything is compared bit for bit.

Before it is stepped a plan is replayed on its fixed inputs (the reference
output) and on other inputs, and then every replay-written word but the
inputs is overwritten, so that no op finds the bits it is about to write
already in place and the closing check starts from a wrong output.

Engines are built with OUHIP_AUTOTUNE=0 (static tiles); the tile sweeps then
run every word the tuner would time on each distinct conv geometry of every
stepped pp16 plan, so the launches of an autotuned build under the same
switches are covered too.  A mutant test shows that the harness reports
footprints that are too small, at the first op concerned, also where that op
runs once per replay and nothing overwrites its output."""
import time

import numpy as np
import pytest
import torch

from conftest import golden_state_dict, load_golden
from footprint_check import KIND_NAMES, SYNC, Stepper, inputs
from open_universe_amd import _lib as L
from open_universe_amd import hazards as H
from open_universe_amd.configs import get_config
from open_universe_amd.engine import ConvTuner, Engine
from open_universe_amd.plan import EnhancePlan
from open_universe_amd.utils.synthetic import synth_audio

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, T, STEPS = 2, 4000, 3
_ENV = ("OUHIP_FIR", "OUHIP_SPLIT_IMAGES", "OUHIP_FUSE_BLOCKS", "OUHIP_FUSE_ENDS", "OUHIP_FUSE_DOWN",
        "OUHIP_FUSE_UP", "OUHIP_CONV_PREC", "OUHIP_OVERLAP", "OUHIP_GRU_FLAGS")

# case -> (fixture tag, environment, EnhancePlan options)
CASES = {
    "pp16": ("pp16", {}, {}),
    "pp16-fir1": ("pp16", {"OUHIP_FIR": "1"}, {}),
    "pp16-fir0": ("pp16", {"OUHIP_FIR": "0"}, {}),
    "pp16-no-split-images": ("pp16", {"OUHIP_SPLIT_IMAGES": "0"}, {}),
    "pp16-unfused": ("pp16", {"OUHIP_FUSE_BLOCKS": "0", "OUHIP_FUSE_ENDS": "0"}, {}),
    "pp16-f32": ("pp16", {"OUHIP_CONV_PREC": "f32"}, {}),
    "pp16-f16": ("pp16", {"OUHIP_CONV_PREC": "f16"}, {}),
    "pp16_c4": ("pp16_c4", {}, {}),
    "pp16-keep_rms": ("pp16", {}, {"keep_rms": True}),
    "pp16-aux": ("pp16", {}, {"use_aux_signal": True}),
    "pp16-ensemble": ("pp16", {}, {"ensemble": 2, "ensemble_mode": 1}),
    "pp16-warm": ("pp16", {}, {"warm_start": 1}),   # steps 1 and 2 of the 3
}
# the tile sweeps: (case, taps) over every stepped pp16 plan.  A sweep covers the conv geometries of its plan that
# no sweep listed before it has (the list decides, not the order the tests run in); the f32 geometries go in two
# halves by tap count.  pp16-fir1 records the default plan's geometries with autotuning off, so it adds none.
SWEEPS = (("pp16", None), ("pp16-fir1", None), ("pp16-fir0", None), ("pp16-no-split-images", None),
          ("pp16-unfused", None), ("pp16-f16", None), ("pp16-f32", (1,)), ("pp16-f32", (3, 4, 5)))


def _mix(tag, d):
    m = np.asarray(d["enh_mix"], dtype=np.float32)
    if m.shape[-1] >= T:
        return m[:, :, :T]
    return np.stack([synth_audio(T, 16000, i)[0] for i in range(B)])[:, None, :].astype(np.float32)


class _Cases:
    """Engines, golden fixtures, conv geometries and stepping reports, each made once per module."""

    def __init__(self):
        self.engines, self.reports, self.golden, self.geoms = {}, {}, {}, {}

    def record(self, case, mp):
        """(engine, freshly recorded plan, fixture) of a case.  One engine per (fixture, environment)."""
        tag, env, opts = CASES[case]
        if tag not in self.golden:
            self.golden[tag] = load_golden(tag)
        d = self.golden[tag]
        for k in _ENV:
            mp.delenv(k, raising=False)
        mp.setenv("OUHIP_AUTOTUNE", "0")
        for k, v in env.items():
            mp.setenv(k, v)
        key = (tag,) + tuple(sorted(env.items()))
        eng = self.engines.get(key)
        if eng is None:
            name, nch = ("pp16", 4) if tag == "pp16_c4" else ("pp16", None)
            eng = self.engines[key] = Engine(get_config(name, nch), golden_state_dict(d), DEV)
        return eng, EnhancePlan(eng, B * opts.get("ensemble", 1), T, STEPS, 1.3, **opts), d

    def plan(self, case, mp, prepare=None, limit=4):
        """(plan, reference output, Stepper ready to run) of a case.  The
        Stepper is made (its snapshot of the constants taken) before the plan
        first runs.  The plan is replayed on the fixed inputs for the reference
        output, then on other inputs; then the fixed inputs are put back
        without a launch and every other replay-written word is overwritten
        (Stepper.settle), so no op finds its own output already in place."""
        eng, plan, d = self.record(case, mp)
        if prepare is not None:
            prepare(plan)
        st = Stepper(eng, plan, limit=limit)
        mix, nz = inputs(plan, _mix(CASES[case][0], d))
        ref = plan.run_with_noise(mix, nz).clone()
        plan.MIX.copy_(-0.5 * mix.flip(-1))
        plan.NZ.copy_(inputs(plan, _mix(CASES[case][0], d), seed=77)[1])
        plan.prog.run(torch.cuda.current_stream(plan.dev).cuda_stream)
        plan.check()
        plan.MIX.copy_(mix)
        plan.NZ.copy_(nz)
        st.settle((plan.MIX, plan.NZ), strict=prepare is None)
        assert not torch.equal(self.out(plan), ref)   # the closing check starts from a wrong output
        return plan, ref, st

    @staticmethod
    def out(plan):
        return plan.OUT if plan.RED is None else plan.RED

    def geometries(self, case, mp):
        """The distinct conv geometries (ConvTuner.geometry, n_frames) of a case's plan."""
        if case not in self.geoms:
            with mp.context() as m:
                _, plan, _ = self.record(case, m)
            self.geoms[case] = {ConvTuner.geometry(d) + (d.n_frames,)
                                for op, d in zip(plan.prog.op_kinds(), plan.prog.descs) if op == L.OP_CONV}
        return self.geoms[case]

    def step(self, case, mp, variants=None, key=None):
        key = key or case
        if key not in self.reports:
            with mp.context() as m:
                t0 = time.time()
                plan, ref, st = self.plan(case, m)
                t1 = time.time()
                rep = st.run(variants=variants)
                rep.closing = bool(torch.equal(self.out(plan), ref)) and int(plan.eng.status.abs().sum()) == 0
                rep.seconds = (t1 - t0, time.time() - t1)
                ks = sum(1 for f, p, w in rep.tiles if w & L.TILE_RS and w & L.TILE_KS_MASK)
                print(f"footprints[{key}]: {rep.ops} ops, {rep.words} tile words stepped ({rep.refused} refused, "
                      f"{ks} register-streamed with K slices), {len(st.hot)} hot / {len(st.snap)} constant storages, "
                      f"build and replays {rep.seconds[0]:.1f} s, stepping {rep.seconds[1]:.1f} s, "
                      f"{len(rep.failures)} failures")
                self.reports[key] = rep
        return self.reports[key]


@pytest.fixture(scope="module")
def cases():
    c = _Cases()
    yield c
    c.engines.clear()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("case", list(CASES))
def test_kernels_stay_inside_their_footprints(cases, case, monkeypatch):
    rep = cases.step(case, monkeypatch)
    assert not rep.failures, str(rep)
    assert rep.closing, "stepping the ops one by one did not reproduce the replay's output"


def test_every_op_kind_was_stepped(cases, monkeypatch):
    seen = set()
    for case in CASES:
        seen |= cases.step(case, monkeypatch).kinds
    want = set(L.OP_STRUCT) - set(SYNC)
    assert seen == want, sorted(KIND_NAMES[k] for k in want - seen)


# ------------------------------------------------------------------ tile sweep
def _family(fir, prec, word):
    if word & L.TILE_FIR:
        return {1: "fir down", 2: "fir up", 3: "fir 3"}[fir]
    if word & L.TILE_SS:
        return "split-image"
    ks = bool(word & L.TILE_KS_MASK)
    if word & L.TILE_RS:
        return "register-streamed, K slices" if ks else "register-streamed"
    if word & L.TILE_WS:
        return "warp-specialised"
    if word & L.TILE_TPW_MASK:
        return "persistent"
    return "plain, K slices" if ks else "plain"


def _sweep(cases, case, taps, mp):
    """Stepping of ``case`` with every candidate word of the tuner on each
    conv geometry (of these tap counts) that no earlier entry of SWEEPS has."""
    key = f"sweep {case} taps {taps or 'all'}"
    if key in cases.reports:
        return cases.reports[key]
    earlier = set()
    for c, _ in SWEEPS[:[c for c, _ in SWEEPS].index(case)]:
        earlier |= cases.geometries(c, mp)
    done = set()

    def variants(i, d):
        g = ConvTuner.geometry(d) + (d.n_frames,)
        if g in earlier or g in done or (taps is not None and d.kt not in taps):
            return
        done.add(g)
        for word in ConvTuner.candidates(d):
            dv = L.ConvDesc.from_buffer_copy(d)
            dv.tile = word
            yield word, dv

    return cases.step(case, mp, variants=variants, key=key)


@pytest.mark.parametrize("case,taps", SWEEPS, ids=[c + ("" if t is None else "-taps" + "".join(map(str, t))) for c, t in SWEEPS])
def test_tile_sweep_stays_inside_the_footprints(cases, case, taps, monkeypatch):
    rep = _sweep(cases, case, taps, monkeypatch)
    assert not rep.failures, str(rep)
    assert rep.closing


def test_tile_sweep_covers_every_family(cases, monkeypatch):
    fams = {}
    for case, taps in SWEEPS:
        for t in _sweep(cases, case, taps, monkeypatch).tiles:
            f = _family(*t)
            fams[f] = fams.get(f, 0) + 1
    print("tile words stepped per family:", fams)
    print("register-streamed words that took K slices:", fams.get("register-streamed, K slices", 0))
    for f in ("plain", "plain, K slices", "register-streamed", "split-image", "fir down", "fir up", "fir 3",
              "persistent", "warp-specialised"):
        assert fams.get(f, 0) > 0, (f, fams)


# ------------------------------------------------------------------ the check bites
def _drop(boxes, ptr):
    return [b for b in boxes if b.base != (ptr or 0)]


def _shorten(boxes, ptr):
    return [H.Box(b.base, b.bs, b.cs, b.nb, b.nc, b.t0, b.t1 - 4) if b.base == (ptr or 0) else b for b in boxes]


# mutant -> (op kinds, label prefix of the ops it changes, (R, W, d) -> (R, W), the failing check, the field it
# names).  The "cond" ones change only ops of the conditioner, which run once per replay and whose outputs no later
# op overwrites.  A write mutant must be reported at the first op whose boxes it changes.
_CB = (L.OP_CONV, L.OP_BLOCK)
MUTANTS = {
    "conv res1 dropped from R": ((L.OP_CONV,), "", lambda R, W, d: (_drop(R, d.res1), W), "read culprit", "res1"),
    "conv x one word short": ((L.OP_CONV,), "", lambda R, W, d: (_shorten(R, d.x), W), "read culprit", "x"),
    "block y one word short": ((L.OP_BLOCK,), "", lambda R, W, d: (R, _shorten(W, d.y)), "write check", "y"),
    "sy dropped from W": (_CB, "", lambda R, W, d: (R, _drop(W, d.sy)), "write check", "sy"),
    "block sc dropped from R": ((L.OP_BLOCK,), "", lambda R, W, d: (_drop(R, d.sc), W), "read culprit", "sc"),
    "gru res dropped from R": ((L.OP_GRU,), "", lambda R, W, d: (_drop(R, d.res), W), "read culprit", "res"),
    "cond block y one word short": ((L.OP_BLOCK,), "cond", lambda R, W, d: (R, _shorten(W, d.y)), "write check", "y"),
    "cond block e one word short": ((L.OP_BLOCK,), "cond", lambda R, W, d: (R, _shorten(W, d.e)), "write check", "e"),
    "block u dropped from W": ((L.OP_BLOCK,), "", lambda R, W, d: (R, _drop(W, d.u)), "write check", "u"),
    "cond gru y one word short": ((L.OP_GRU,), "cond", lambda R, W, d: (R, _shorten(W, d.y)), "write check", "y"),
    "cond conv y one word short": ((L.OP_CONV,), "cond sc", lambda R, W, d: (R, _shorten(W, d.y)), "write check", "y"),
    "finish y one word short": ((L.OP_FINISH,), "", lambda R, W, d: (R, _shorten(W, d.y)), "write check", "y"),
}


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_a_footprint_too_small_is_reported(cases, mutant, monkeypatch):
    kinds, prefix, change, check, field = MUTANTS[mutant]
    real = H.footprint
    changed = []   # indices of the ops whose boxes the mutant changes, in program order

    with monkeypatch.context() as m:
        def prepare(plan):
            prog = plan.prog
            index = {id(d): i for i, d in enumerate(prog.descs)}
            mine = {id(d) for op, d, lab in zip(prog.op_kinds(), prog.descs, prog.labels)
                    if op in kinds and lab.startswith(prefix)}
            for op, d in zip(prog.op_kinds(), prog.descs):
                if id(d) in mine and change(*real(op, d), d) != real(op, d):
                    changed.append(index[id(d)])

            def footprint(op, d, lib=None):
                R, W = real(op, d, lib)
                return change(R, W, d) if id(d) in mine else (R, W)

            m.setattr(H, "footprint", footprint)

        _, _, st = cases.plan("pp16", m, prepare=prepare, limit=1)
        rep = st.run(kinds=kinds)
    assert changed, mutant
    hits = [f for f in rep.failures if f[2].startswith(check) and field in f[3].split("/")]
    assert hits and hits[0][0] in changed, (mutant, changed[:4], str(rep))
    if check == "write check":
        assert hits[0][0] == changed[0], (mutant, changed[:4], str(rep))
