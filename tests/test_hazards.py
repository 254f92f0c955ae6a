"""Race and lifetime checks of recorded programs (open_universe_amd/hazards.py),
on the CPU: every pair of ops on different lanes that touch the same bytes
(one writing) must be ordered by the lanes' events, and every byte a
descriptor points at must belong to a tensor the plan keeps alive."""
import gc

import pytest
import torch

from conftest import golden_state_dict, load_golden
from open_universe_amd import _lib as L
from open_universe_amd import hazards as H
from open_universe_amd.configs import get_config
from open_universe_amd.engine import Engine
from open_universe_amd.plan import CondPlan, EnhancePlan, ScorePlan


def test_box_overlap_is_exact():
    # rows 0..3 of 100-byte rows, bytes [0, 40) and [40, 80): interleaved, disjoint
    a = H.Box(1000, 0, 100, 1, 4, 0, 40)
    b = H.Box(1000, 0, 100, 1, 4, 40, 80)
    assert not H.overlap(a, b) and not H.overlap(b, a)
    assert H.overlap(a, H.Box(1000, 0, 100, 1, 4, 39, 41))
    # two batch items of 1000 bytes, the second item's first row
    c = H.Box(1000, 1000, 100, 2, 4, 0, 40)
    assert H.overlap(c, H.Box(2000, 0, 0, 1, 1, 0, 4))
    assert not H.overlap(c, H.Box(1400, 0, 0, 1, 1, 0, 600))   # between item 0's rows and item 1
    assert H.overlap(c, H.Box(1400, 0, 0, 1, 1, 0, 601))


def _memset(p, t):
    p.add(L.OP_MEMSET, L.MemsetArgs(ptr=t.data_ptr(), bytes=t.numel() * 4))


def _scale(p, src, dst):
    p.add(L.OP_SCALE, L.ScaleArgs(z=src.data_ptr(), y=dst.data_ptr(), n=src.numel(), scale=1.0, add=0))


@pytest.mark.parametrize("ordered", [False, True])
def test_unordered_lanes_are_reported(ordered):
    a, b = torch.zeros(256), torch.zeros(256)
    p = L.Program()
    ev0 = p.signal()
    p.lane(1)
    p.wait(ev0)
    _memset(p, a)              # lane 1 writes a
    ev1 = p.signal()
    p.lane(0)
    if ordered:
        p.wait(ev1)
    _scale(p, a, b)            # lane 0 reads a
    if not ordered:
        p.wait(ev1)
    hz = H.find_hazards(p)
    assert (hz == []) == ordered, hz
    if not ordered:
        assert hz[0][2] == "write-read"


def test_dangling_pointer_is_reported():
    keep = torch.zeros(64)
    p = L.Program()
    tmp = torch.zeros(64)
    _scale(p, keep, tmp)
    assert H.dangling(p, keep, tmp) == []
    del tmp
    gc.collect()
    assert [i for i, _, _ in H.dangling(p, keep)] == [0]


@pytest.fixture(scope="module")
def engines():
    out = {}
    for tag, name, nch in (("pp16_c4", "pp16", 4), ("orig16_c4", "orig16", 4), ("pp24_c4", "pp24", 4),
                           ("pp16", "pp16", None)):
        d = load_golden(tag)
        out[tag] = Engine(get_config(name, nch), golden_state_dict(d), "cpu", _record_only=True)
    return out


def _check(plan):
    gc.collect()
    assert H.find_hazards(plan.prog) == []
    assert H.dangling(plan.prog, plan) == []


@pytest.mark.parametrize("tag", ["pp16_c4", "orig16_c4", "pp24_c4", "pp16"])
@pytest.mark.parametrize("B", [1, 2, 3])
def test_enhance_plans_are_race_free(engines, tag, B):
    T = 16000 if tag == "pp16" else 4000
    _check(EnhancePlan(engines[tag], B, T, 8, 1.3))


@pytest.mark.parametrize("opts", [{"keep_rms": True}, {"use_aux_signal": True}, {"warm_start": 3},
                                  {"ensemble": 2, "ensemble_mode": 1}, {"st_lane": False}])
def test_enhance_plan_options_are_race_free(engines, opts):
    B = 2 * opts.get("ensemble", 1)
    _check(EnhancePlan(engines["pp16"], B, 16000, 8, 1.3, **opts))


@pytest.mark.parametrize("env", [{"OUHIP_OVERLAP": "0"}, {"OUHIP_SPLIT_IMAGES": "0"}, {"OUHIP_FIR": "1"},
                                 {"OUHIP_FIR": "0"}])
def test_enhance_plan_schedules_are_race_free(engines, env, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _check(EnhancePlan(engines["pp16_c4"], 2, 4000, 8, 1.3))


def test_network_plans_are_race_free(engines):
    _check(ScorePlan(engines["pp16"], 2, 1600))
    _check(CondPlan(engines["pp16"], 2, 1600))


# ------------------------------------------------------------------ overlap against brute force
def _bytes_of(b):
    return {b.base + i * b.bs + c * b.cs + t for i in range(b.nb) for c in range(b.nc) for t in range(b.t0, b.t1)}


def _random_box(rnd):
    t0 = rnd.randrange(0, 6)
    return H.Box(rnd.randrange(0, 48), rnd.choice((0, 0, 7, 16, 24, 40)), rnd.choice((0, 1, 3, 4, 8, 12)),
                 rnd.randrange(1, 4), rnd.randrange(1, 5), t0, t0 + rnd.randrange(1, 14))   # rows up to 13 bytes: wider
                                                                                           # than most row strides


def test_overlap_agrees_with_byte_sets():
    import random

    rnd = random.Random(20240611)
    hits = 0
    for _ in range(20000):
        a, b = _random_box(rnd), _random_box(rnd)
        want = bool(_bytes_of(a) & _bytes_of(b))
        hits += want
        assert H.overlap(a, b) == want and H.overlap(b, a) == want, (a, b, want)
        s0 = rnd.randrange(0, 160)
        s1 = s0 + rnd.randrange(1, 20)
        assert H._span_hits(s0, s1, a) == bool(_bytes_of(a) & set(range(s0, s1))), (s0, s1, a)
    assert 2000 < hits < 18000   # both answers are exercised


def test_overlap_of_very_many_rows_is_conservative():
    # more than 2^16 rows on both sides: not enumerated.  Interleaved rows share no byte, the answer is still
    # True (a race reported that is none, never one missed); disjoint address ranges stay False
    a = H.Box(0, 0, 8, 1, (1 << 16) + 1, 0, 4)
    b = H.Box(4, 0, 8, 1, (1 << 16) + 1, 0, 4)
    assert H.overlap(a, b) and H.overlap(b, a)
    far = H.Box(a.hi, 0, 8, 1, (1 << 16) + 1, 0, 4)
    assert not H.overlap(a, far) and not H.overlap(far, a)
    # one row fewer is enumerated, and exact
    c = H.Box(4, 0, 8, 1, 1 << 16, 0, 4)
    assert not H.overlap(a, c) and not H.overlap(c, a)


# ------------------------------------------------------------------ structural completeness
# (descriptor, field) pairs that may point into replay-written memory outside their op's boxes: a closed table,
# and each entry is one the GPU stepping (tests/test_gpu_footprints.py) covers without exemption
_UNDECLARED_OK = set()   # none is needed: a conv's K-slice workspace (ks_ws) is written, and then declared, only
#                          under a tile word with K slices, so without one it is no replay-written memory


def _undeclared_pointers(plan):
    """Pointer fields into replay-written memory that lie in no box of their own op."""
    import struct

    from open_universe_amd.bundle import pointer_fields

    prog = plan.prog
    ops = [(i, op, d) for i, (op, d) in enumerate(zip(prog.op_kinds(), prog.descs))
           if op not in (L.OP_LANE, L.OP_SIGNAL, L.OP_WAIT)]
    fps = {i: H.footprint(op, d) for i, op, d in ops}
    written = {b for _, W in fps.values() for b in W}
    for t in (getattr(plan, "MIX", None), getattr(plan, "NZ", None)):   # the host-written inputs
        if t is not None:
            written.add(H.Box(t.data_ptr(), 0, 0, 1, 1, 0, t.numel() * 4))
    in_p = {}
    bad = []
    for i, op, d in ops:
        blob = bytes(d)
        R, W = fps[i]
        for name, off in pointer_fields(type(d)):
            p = struct.unpack_from("<Q", blob, off)[0]
            if not p or (type(d).__name__, name) in _UNDECLARED_OK:
                continue
            if p not in in_p:
                in_p[p] = any(H._span_hits(p, p + 4, b) for b in written)
            if in_p[p] and not any(H._span_hits(p, p + 4, b) for b in R + W):
                bad.append((i, prog.labels[i], type(d).__name__, name, hex(p)))
    return bad


def _enhance(tag, B, T, **opts):
    return lambda engines: EnhancePlan(engines[tag], B, T, 8, 1.3, **opts)


_RECORDED = {f"{tag}-B{B}": _enhance(tag, B, 16000 if tag == "pp16" else 4000)
             for tag in ("pp16_c4", "orig16_c4", "pp24_c4", "pp16") for B in (1, 2, 3)}
_RECORDED.update({
    "pp16-keep_rms": _enhance("pp16", 2, 16000, keep_rms=True),
    "pp16-aux": _enhance("pp16", 2, 16000, use_aux_signal=True),
    "pp16-warm": _enhance("pp16", 2, 16000, warm_start=3),
    "pp16-ensemble": _enhance("pp16", 4, 16000, ensemble=2, ensemble_mode=1),
    "pp16-no-st-lane": _enhance("pp16", 2, 16000, st_lane=False),
    "pp16-score": lambda engines: ScorePlan(engines["pp16"], 2, 1600),
    "pp16-cond": lambda engines: CondPlan(engines["pp16"], 2, 1600),
})
_SCHEDULES = [{"OUHIP_OVERLAP": "0"}, {"OUHIP_SPLIT_IMAGES": "0"}, {"OUHIP_FIR": "1"}, {"OUHIP_FIR": "0"}]


@pytest.mark.parametrize("name", list(_RECORDED))
def test_pointer_fields_lie_inside_their_ops_boxes(engines, name):
    assert _undeclared_pointers(_RECORDED[name](engines)) == []


@pytest.mark.parametrize("env", _SCHEDULES)
@pytest.mark.parametrize("tag", ["pp16_c4", "pp16"])
def test_pointer_fields_lie_inside_their_ops_boxes_schedules(engines, tag, env, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    assert _undeclared_pointers(EnhancePlan(engines[tag], 2, 4000, 8, 1.3)) == []


def test_the_pointer_check_sees_a_missing_box(engines, monkeypatch):
    real = H.footprint

    def no_sc(op, d, lib=None):   # a block's input_cond left out of its reads
        R, W = real(op, d, lib)
        return ([b for b in R if op != L.OP_BLOCK or b.base != (d.sc or 0)], W)

    monkeypatch.setattr(H, "footprint", no_sc)
    bad = _undeclared_pointers(EnhancePlan(engines["pp16"], 2, 4000, 8, 1.3))
    assert bad and {b[3] for b in bad} == {"sc"}
