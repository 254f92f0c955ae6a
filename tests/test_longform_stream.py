"""The host arithmetic of a streaming enhance (longform.StreamCounts; DESIGN.md
section 15) against brute-force simulation, and the refusals of the C entry
points that need no device.  No GPU involved."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from open_universe_amd import _lib as L
from open_universe_amd import longform as LF


def _cases(seed, n):
    rng = np.random.default_rng(seed)
    for _ in range(n):
        W = int(rng.integers(1, 60))
        O = int(rng.integers(0, W // 2 + 1))
        B = int(rng.integers(1, 5))
        T = int(rng.integers(0, 12 * W))
        cuts = []
        left = T
        while left:
            k = int(min(left, rng.choice([0, 1, 2, W, W - O, 3 * W + 1, int(rng.integers(1, 8 * W))])))
            cuts.append(k)
            left -= k
        yield W, O, B, T, cuts


def _brute_emitted(fed, W, O, B):
    """Samples final after ``fed`` samples: windows are found one sample position at a time."""
    H = W - O
    ready = 0
    while ready * H + W <= fed:
        ready += 1
    return ready // B * B * H, ready // B * B


@pytest.mark.parametrize("seed", range(4))
def test_emitted_counts_match_a_brute_force_simulation(seed):
    for W, O, B, T, cuts in _cases(seed, 150):
        c = LF.StreamCounts(W, O, B, Tp=W + 3)
        H, fed, emitted = W - O, 0, 0
        for k in cuts:
            want = _brute_emitted(fed + k, W, O, B)[0] - emitted
            assert c.bound(k) == want
            steps = c.push(k)
            assert sum(s[1] for s in steps if s[0] == "feed") == k
            got = sum(LF.StreamCounts.emitted(s, H) for s in steps if s[0] == "group")
            assert got == want
            fed, emitted = fed + k, emitted + got
            assert (c.fed, c.run) == (fed, _brute_emitted(fed, W, O, B)[1])
            assert emitted == c.run * H
        if T < W:
            with pytest.raises(LF.StreamShort):
                c.bound(closing=True)
            with pytest.raises(LF.StreamShort):
                c.close()
            assert not c.closed and c.push(0) == []   # still valid
            continue
        assert c.bound(closing=True) == T - emitted
        (step,) = c.close()
        assert LF.StreamCounts.emitted(step, H, T) == T - emitted
        assert c.closed and c.bound(5) == 0
        with pytest.raises(ValueError):
            c.push(1)


@pytest.mark.parametrize("seed", range(4))
def test_the_windows_run_are_the_final_window_list(seed):
    """Every window that ran before close is a regular window of the list
    ``longform`` gives for the final length; close runs the rest, once each,
    in order, in at most one group."""
    for W, O, B, T, cuts in _cases(10 + seed, 150):
        if T < W:
            continue
        c = LF.StreamCounts(W, O, B)
        H = W - O
        ran = []
        for k in cuts:
            for s in c.push(k):
                if s[0] == "group":
                    assert s[2] == B and not s[3]
                    ran.extend(range(s[1], s[1] + s[2]))
        starts = LF.starts(T, W, O)
        assert all(i * H == starts[i] for i in ran)
        (_, first, count, closing), = c.close()
        assert closing and 0 <= count <= B
        ran.extend(range(first, first + count))
        assert ran == list(range(LF.n_windows(T, W, O)))
        if count == 0:   # nothing left: the last window is regular and ended at T
            assert starts[-1] + W == T and starts[-1] == (len(starts) - 1) * H


@pytest.mark.parametrize("seed", range(4))
def test_the_ring_never_drops_a_sample_a_window_reads(seed):
    """Simulate the ring position by position: at every group, every sample of
    every window of it -- the shifted last one included -- is still there,
    and the ring's content is what ``held()`` says."""
    for W, O, B, T, cuts in _cases(20 + seed, 120):
        c = LF.StreamCounts(W, O, B)
        H = W - O
        assert c.cap == LF.stream_ring(W, O, B) == W + B * H
        ring = np.full(c.cap, -1, dtype=np.int64)
        fed = 0

        def run(steps, T_close=None):
            nonlocal fed
            for s in steps:
                if s[0] == "feed":
                    p = np.arange(fed, fed + s[1])
                    assert s[1] <= c.cap
                    ring[p % c.cap] = p
                    fed += s[1]
                    continue
                _, first, count, closing = s
                for i in range(first, first + count):
                    st = i * H if not closing else LF.start(i, T_close, W, O)
                    p = np.arange(st, st + W)
                    assert (ring[p % c.cap] == p).all(), (W, O, B, fed, i, st)
                    assert st >= max(0, fed - c.cap)

        for k in cuts:
            run(c.push(k))
            assert fed == c.fed and c.held() <= c.retain()
            if fed:
                p = np.arange(c.retain(), fed)
                assert (ring[p % c.cap] == p).all()   # the retain rule itself, for whatever close may ask
        if T >= W:
            run(c.close(), T)


def test_one_push_larger_than_the_ring_is_cut_into_pieces():
    c = LF.StreamCounts(4000, 800, 2)
    steps = c.push(50000)
    feeds = [s[1] for s in steps if s[0] == "feed"]
    assert sum(feeds) == 50000 and max(feeds) <= c.cap and len(feeds) > 4
    assert [s[1] for s in steps if s[0] == "group"] == list(range(0, c.run, 2))
    assert c.run == ((50000 - 4000) // 3200 + 1) // 2 * 2


def test_draw_offsets_and_limits():
    assert LF.stream_draw_offset(5, 0) == 5 and LF.stream_draw_offset(5, 3) == 5 + 3 * 2**38
    assert LF.stream_draw_offset(2**64 - 1, 1) == 2**38 - 1   # 64-bit counters wrap
    assert LF.DRAW_COUNTERS * 4 == LF.STREAM_MAX_SAMPLES
    c = LF.StreamCounts(4000, 800, 1, Tp=4160)
    c.fed = 2**40 - 160    # the last window's noise, Tp - W past its end, reaches sample 2^40 exactly
    c.run = c.ready()
    assert c.push(0) == []
    with pytest.raises(ValueError, match="2\\^40"):
        c.push(1)
    for bad in [(0, 0, 1), (8, 5, 1), (8, -1, 1), (8, 2, 0)]:
        with pytest.raises(ValueError):
            LF.StreamCounts(*bad)
    with pytest.raises(ValueError):
        LF.StreamCounts(8, 2, 1).push(-1)


# ---- the C entry points: what they refuse before any HIP call --------------
def _err(lib):
    return (lib.ou_last_error() or b"").decode()


def test_session_calls_refuse_nulls_without_a_device():
    lib = L.load()
    h = ctypes.c_void_p()
    n = ctypes.c_int64(7)
    assert lib.ou_model_stream_open(None, 800, 0, 0, ctypes.byref(h)) == -1 and "null" in _err(lib)
    assert lib.ou_model_stream_open(None, 800, 0, 0, None) == -1
    assert lib.ou_model_stream_push(None, 256, 10, 256, ctypes.byref(n), None) == -1
    assert lib.ou_model_stream_close(None, 256, ctypes.byref(n), None) == -1
    assert lib.ou_model_stream_bound(None, 10, 0) == -1
    assert lib.ou_model_stream_bound(None, -1, 0) == -1
    lib.ou_model_stream_destroy(None)   # a no-op
    assert L.STREAM_SHORT == 3 and L.STREAM_SHORT not in (1, 2)   # not one of ou_model_status' codes


def _gather(lib, **kw):
    a = dict(ring=256, cap=20, lo=0, fed=20, window=8, overlap=2, first=0, count=3, slots=3, closing=0, T=0,
             noise_rows=2, noise_win=9, seed=1, offset=0, mix=256, mix_bstride=8, nz=256, nz_rstride=27, nz_bstride=9)
    a.update(kw)
    return lib.ou_stream_gather(*a.values(), None)


def _oadd(lib, **kw):
    a = dict(w=256, w_bstride=8, window=8, overlap=2, first=0, count=3, closing=0, T=0, fade=256, carry=256, out=256,
             n_out=None)
    a.update(kw)
    return lib.ou_stream_overlap_add(*a.values(), None)


@pytest.mark.parametrize("kw", [dict(ring=None), dict(mix=None), dict(nz=None), dict(overlap=5), dict(overlap=-1),
                                dict(window=0), dict(count=0), dict(count=-1), dict(first=-1), dict(slots=2),
                                dict(cap=7), dict(fed=21), dict(lo=1), dict(closing=1, T=19),
                                dict(closing=1, T=20, count=2), dict(mix_bstride=7), dict(nz_bstride=8),
                                dict(nz_rstride=26), dict(noise_rows=-1), dict(noise_win=0), dict(ring=258)])
def test_stream_gather_refusals_need_no_device(kw):
    lib = L.load()
    assert _gather(lib, **kw) == -1 and "stream_gather" in _err(lib)


@pytest.mark.parametrize("kw", [dict(w=None), dict(out=None), dict(fade=None), dict(carry=None), dict(overlap=5),
                                dict(overlap=-1), dict(window=0), dict(count=0), dict(count=-1, closing=1, T=8),
                                dict(first=-1), dict(w_bstride=7), dict(closing=1, T=7, count=1),
                                dict(closing=1, T=20, count=2), dict(closing=1, T=19, first=3, count=0),
                                dict(out=258)])
def test_stream_overlap_add_refusals_need_no_device(kw):
    lib = L.load()
    assert _oadd(lib, **kw) == -1 and "stream_overlap_add" in _err(lib)


# ---- builds ------------------------------------------------------------------
HIPCC = "/opt/rocm/bin/hipcc"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not present")
def test_stream_host_example_compiles_and_links(tmp_path):
    """examples/stream_host.cpp against the built library (compiled and linked
    only: running it needs a GPU, tests/test_gpu_stream.py)."""
    exe = str(tmp_path / "stream_host")
    r = subprocess.run([HIPCC, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "stream_host.cpp"), "-o", exe,
                        "-L", os.path.dirname(L.LIB_PATH), "-louhip", "-Wl,-rpath," + os.path.dirname(L.LIB_PATH)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert os.path.exists(exe)


def test_cli_formats_round_trip():
    from open_universe_amd.bin import enhance_stream as cli

    x = np.array([0.0, 0.5, -0.5, 0.999, -1.0, 1.5, 1.0 / 32768], dtype=np.float32)
    s16 = cli.encode(x, "s16le")
    assert np.frombuffer(s16, "<i2").tolist() == [0, 16384, -16384, 32735, -32768, 32767, 1]
    assert cli.decode(s16, "s16le").tolist() == [0.0, 0.5, -0.5, 32735 / 32768, -1.0, 32767 / 32768, 1 / 32768]
    assert cli.decode(cli.encode(x, "f32le"), "f32le").tolist() == x.tolist()
    args = cli.build_parser().parse_args(["--bundle", "b.oub"])
    assert args.window_batch == 1 and args.format == "f32le" and args.rate is None
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args([])                        # --model or --bundle
    with pytest.raises(SystemExit):
        cli.check_rate(cli.build_parser().parse_args(["--bundle", "b.oub", "--rate", "8000"]), 16000)
