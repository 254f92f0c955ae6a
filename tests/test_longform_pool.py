"""Pooled windows (longform.py "Pooled windows") on the
CPU: the slot lists, the ownership rule of ou_pool_overlap_add evaluated in
numpy group by group against the existing float32 overlap-add -- the same bits
for every grouping, no sample left unwritten -- the layout of the clip struct,
and the CLI's refusal of ``--window-pool`` without ``--window``."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from open_universe_amd import _lib as L
from open_universe_amd import longform

TS = [9000, 4001, 10400]
W, O = 4000, 800


def test_pool_slot_lists():
    want = [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (2, 0), (2, 1), (2, 2)]
    for batch, B in ((2, 2), (3, 3), (8, 8), (64, 8)):
        assert longform.pool(TS, W, O, batch) == (B, want)
    # one clip: the slots and the group size of enhance_long
    for T in TS:
        B, slots = longform.pool([T], W, O, 2)
        assert (B, [i for _, i in slots][::B]) == longform.groups(T, W, O, 2)
    for bad in ([9000, 4000], [3000], []):   # a clip that fits the window takes no slot
        with pytest.raises(ValueError):
            longform.pool(bad, W, O, 2)
    with pytest.raises(ValueError):
        longform.pool(TS, W, W // 2 + 1, 2)


@pytest.mark.parametrize("Ts,Wn,On", [(TS, 4000, 800), (TS, 4000, 0), (TS, 4000, 2000), ([10397, 4001], 4000, 800),
                                      ([700, 38, 700, 101], 37, 18), ([700, 38, 700, 101], 37, 5)])
def test_grouping_does_not_change_bits(Ts, Wn, On):
    """overlap_add_pooled (every y starts as NaN; a sample stored twice by one
    group asserts) equals overlap_add(dtype=float32) per clip, bit for bit,
    for every group size from 1 to all slots."""
    _, slots = longform.pool(Ts, Wn, On, 1)
    rng = np.random.default_rng(len(slots) + On)
    outs = rng.standard_normal((len(slots), Wn)).astype(np.float32)
    want, s = [], 0
    for T in Ts:
        n = longform.n_windows(T, Wn, On)
        want.append(longform.overlap_add(outs[s:s + n], T, Wn, On, dtype=np.float32))
        s += n
    batches = range(1, len(slots) + 1) if len(slots) <= 8 else (1, 2, 3, 5, 22, 23, 33, len(slots))
    for batch in batches:
        got = longform.overlap_add_pooled(outs, Ts, Wn, On, batch)
        for c, (g, w) in enumerate(zip(got, want)):
            assert g.dtype == np.float32 and not np.isnan(g).any(), (batch, c)
            assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), (batch, c)


def test_pool_clip_layout_matches_c(tmp_path):
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ouhip.h")
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{header}"', "int main(void){",
             'printf("size %zu\\n", sizeof(ou_pool_clip));']
    lines += [f'printf("{f} %zu\\n", offsetof(ou_pool_clip, {f}));' for f, _ in L.PoolClip._fields_]
    lines.append("return 0;}")
    src, exe = str(tmp_path / "l.c"), str(tmp_path / "l")
    open(src, "w").write("\n".join(lines))
    subprocess.check_call(["gcc", "-std=c99", "-o", exe, src])
    got = dict(line.split() for line in subprocess.check_output([exe]).decode().splitlines())
    assert int(got["size"]) == ctypes.sizeof(L.PoolClip)
    for f, _ in L.PoolClip._fields_:
        assert int(got[f]) == getattr(L.PoolClip, f).offset, f


def test_pool_slots_agrees_with_longform():
    """ou_pool_slots (host arithmetic, no HIP call) against longform.pool."""
    lib = L.load()
    n = ctypes.c_int64(0)
    for Ts, Wn, On in ((TS, 4000, 800), (TS, 4000, 0), ([700, 38, 700, 101], 37, 18), ([2 ** 31 + 12345, 9000], 4000, 800)):
        arr = (ctypes.c_int64 * len(Ts))(*Ts)
        assert lib.ou_pool_slots(arr, len(Ts), Wn, On, ctypes.byref(n)) == 0
        assert n.value == sum(longform.n_windows(T, Wn, On) for T in Ts)
    arr = (ctypes.c_int64 * 2)(9000, 4000)
    assert lib.ou_pool_slots(arr, 2, 4000, 800, ctypes.byref(n)) != 0 and b"4000 samples" in lib.ou_last_error()


def test_cli_refuses_window_pool_without_window(tmp_path):
    from open_universe_amd.bin import enhance as cli

    with pytest.raises(SystemExit) as e:
        cli.main([str(tmp_path), str(tmp_path / "out"), "--model", str(tmp_path / "none.ckpt"), "--window-pool"])
    assert "--window-pool" in str(e.value) and "--window SECONDS" in str(e.value)
