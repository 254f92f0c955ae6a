#!/usr/bin/env python
"""Measure multiplexed streams, not gated anywhere:
full-width PP16 synthetic weights (bench.py's model), windows of 1 s and 2 s
with an overlap of an eighth of the window, ``C = B`` in {2, 4, 8} live
streams of 16 s each, every one fed in hops of ``H = W - O`` -- so every round
of pushes after the first completes exactly one window per stream.

Per shape, in one process:
  * mux: ``Universe.stream_mux(channels=C, batch=C)``; a round is ``C`` pushes
    and one ``run()``, which replays the ``(C, W)`` plan once.  Device ms
    between two HIP events around ``run()`` alone and around the whole round
    (the pushes' copies included), median and max over the rounds that emitted.
  * baseline (the existing code): the same streams as ``C`` round-robin
    ``Universe.stream(batch=1)`` sessions; a round is ``C`` pushes, each of
    which replays the ``(1, W)`` plan.  Device ms around the round.
  * the kernels alone: one ou_mux_gather + one ou_mux_overlap_add for a group
    of ``C`` slots against the ``2 C`` ou_stream_gather / ou_stream_overlap_add
    launches they replace, on scratch buffers, device ms per group.
1 warm-up pass and 2 timed passes per shape.

    python tools/mux_bench.py --out profiles/stream_mux.json
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
SECONDS, WINDOWS_S, CHANNELS, WARMUP, PASSES, KERNEL_REPS = 16.0, (1.0, 2.0), (2, 4, 8), 1, 2, 50


def timed(fn):
    import torch

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), r


def mux_pass(model, xs, W, O, seed):
    """[(run ms, round ms)] of the rounds that emitted, and the samples emitted."""
    import torch

    H, C = W - O, len(xs)
    rows, n_out = [], 0
    with model.stream_mux(W, O, C, batch=C) as mx:
        for c in range(C):
            mx.open(seed=seed + c)
        for at in range(0, xs[0].numel(), H):
            box = {}

            def rnd():
                for c in range(C):
                    mx.push(c, xs[c][at:at + H])
                box["run"], ys = timed(mx.run)
                return ys

            ms, ys = timed(rnd)
            if ys[0].numel():
                rows.append((box["run"], ms))
            n_out += sum(y.numel() for y in ys)
        for c in range(C):
            mx.close(c)
        n_out += sum(y.numel() for y in mx.run())
        torch.cuda.synchronize()
    return rows, n_out


def round_robin_pass(model, xs, W, O, seed):
    """[round ms] of C stand-alone batch-1 streams served one after another."""
    H, C = W - O, len(xs)
    rows, n_out = [], 0
    ss = [model.stream(W, O, batch=1, seed=seed + c) for c in range(C)]
    try:
        for at in range(0, xs[0].numel(), H):
            ms, ys = timed(lambda: [s.push(x[at:at + H]) for s, x in zip(ss, xs)])
            if ys[0].numel():
                rows.append(ms)
            n_out += sum(y.numel() for y in ys)
        n_out += sum(s.close().numel() for s in ss)
    finally:
        for s in ss:
            s.release()
    return rows, n_out


def kernels_alone(W, O, C, rows, Tp, dev):
    """Device ms per group: the two mux launches, and the 2 C stream launches."""
    import torch

    from open_universe_amd import _lib as L
    from open_universe_amd import longform

    lib = L.load()
    H = W - O
    cap = W + C * H
    fed, first = 3 * H + W, 3                          # every channel's window 3, its carry from window 2
    rings = torch.randn(C, cap, device=dev)
    mix, nz = torch.empty(C, W, device=dev), torch.empty(rows, C, Tp, device=dev)
    w = torch.randn(C, W, device=dev)
    carries, out = torch.randn(C, max(O, 1), device=dev), torch.empty(C * H, device=dev)
    fade = torch.from_numpy(longform.fade_table(O)).to(dev)
    slots, runs = (L.MuxSlot * C)(), (L.MuxRun * C)()
    for c in range(C):
        s, r = slots[c], runs[c]
        s.start, s.lo, s.fed, s.seed, s.offset, s.channel = first * H, max(0, fed - cap), fed, c, 0, c
        r.first, r.T, r.out_off, r.count, r.closing, r.slot, r.channel = first, 0, c * H, 1, 0, c, c
    sp = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def mux():
        for _ in range(KERNEL_REPS):
            L.check(lib.ou_mux_gather(rings.data_ptr(), cap, C, W, slots, C, rows, Tp, mix.data_ptr(), W, nz.data_ptr(),
                                      C * Tp, Tp, sp), "mux_gather")
            L.check(lib.ou_mux_overlap_add(w.data_ptr(), W, C, W, O, runs, C, fade.data_ptr(), carries.data_ptr(),
                                           carries.stride(0), C, out.data_ptr(), out.numel(), None, sp),
                    "mux_overlap_add")

    def streams():
        for _ in range(KERNEL_REPS):
            for c in range(C):
                L.check(lib.ou_stream_gather(rings[c].data_ptr(), cap, max(0, fed - cap), fed, W, O, first, 1, 1, 0, 0,
                                             rows, Tp, c, 0, mix.data_ptr(), W, nz.data_ptr(), Tp, Tp, sp),
                        "stream_gather")
                L.check(lib.ou_stream_overlap_add(w[c].data_ptr(), W, W, O, first, 1, 0, 0, fade.data_ptr(),
                                                  carries[c].data_ptr(), out.data_ptr() + 4 * c * H, None, sp),
                        "stream_overlap_add")

    res = {}
    for name, fn in (("mux_two_launches_ms", mux), ("stream_2c_launches_ms", streams)):
        fn()
        res[name] = min(timed(fn)[0] for _ in range(3)) / KERNEL_REPS
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="write the JSON here as well")
    ap.add_argument("--seconds", type=float, default=SECONDS, help="length of every stream")
    a = ap.parse_args()
    import numpy as np
    import torch

    import bench
    from open_universe_amd.utils.synthetic import synth_audio

    dev = torch.device("cuda:0")
    cfg, model = bench.build_model(dev)
    fs = int(cfg["fs"])
    T = int(a.seconds * fs)
    n_steps = int(model.diff_kwargs.n_steps)
    clips = [torch.from_numpy(synth_audio(T, fs, c)[0].astype(np.float32)).to(dev) for c in range(max(CHANNELS))]
    out = {"shape": f"full-width PP16, synthetic weights, C = B live streams of {a.seconds:g} s at {fs} Hz, {n_steps} "
                    "steps, overlap = window / 8, every stream fed in hops of H",
           "warmup_passes": WARMUP, "timed_passes": PASSES, "kernel_reps": KERNEL_REPS, "shapes": []}
    med = statistics.median
    with torch.no_grad():
        for ws in WINDOWS_S:
            W = int(ws * fs)
            O = W // 8
            for C in CHANNELS:
                xs = clips[:C]
                for k in range(WARMUP):
                    mux_pass(model, xs, W, O, k)
                    round_robin_pass(model, xs, W, O, k)
                mux_rows, rr_rows = [], []
                for k in range(PASSES):
                    r, n_out = mux_pass(model, xs, W, O, 100 + k)
                    assert n_out == C * T, (n_out, C * T)
                    mux_rows += r
                    r, n_out = round_robin_pass(model, xs, W, O, 100 + k)
                    assert n_out == C * T, (n_out, C * T)
                    rr_rows += r
                Tp = W + model.tot_ds - W % model.tot_ds
                row = {"window_s": ws, "overlap_s": O / fs, "channels": C, "batch": C, "timed_rounds": len(mux_rows),
                       "mux_run_device_ms_median": med(r[0] for r in mux_rows),
                       "mux_run_device_ms_max": max(r[0] for r in mux_rows),
                       "mux_round_device_ms_median": med(r[1] for r in mux_rows),
                       "round_robin_b1_round_device_ms_median": med(rr_rows),
                       "round_robin_b1_round_device_ms_max": max(rr_rows)}
                row["round_robin_over_mux"] = row["round_robin_b1_round_device_ms_median"] / \
                    row["mux_round_device_ms_median"]
                row["streams_in_real_time_mux"] = C * ((W - O) / fs) / (1e-3 * row["mux_round_device_ms_median"])
                row["streams_in_real_time_round_robin"] = C * ((W - O) / fs) / \
                    (1e-3 * row["round_robin_b1_round_device_ms_median"])
                row.update(kernels_alone(W, O, C, n_steps, Tp, dev))
                out["shapes"].append(row)
                print(json.dumps(row), flush=True)
    out["range_fallbacks"], out["range_widenings"] = model.range_fallbacks, model.range_widenings
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
