#!/usr/bin/env python
"""Measure a streaming enhance, not gated anywhere:
full-width PP16 synthetic weights (bench.py's model), ``Universe.stream`` at
``batch`` 1 with windows of 1 s, 2 s and 8 s and an overlap of an eighth of
the window, one 64 s stream pushed in hops of ``H = W - O`` -- so every push
after the first completes exactly one window.

Per window length: 3 warm-up streams, then 3 timed ones.  For every push that
ran a window, the device time between two HIP events recorded around the push
on its stream (feed, gather, replay, status copy, overlap-add) and the host
time of the call, which ends in the status wait: median and max over all such
pushes.  Beside it ``enhance_long(batch=1)`` on the same clip in the same
process (3 warm-ups, 5 timed calls, a host clock around a call that ends in a
synchronise): the throughput of the same windows without the per-window
status wait and with one noise fill per clip.

    python tools/stream_bench.py --out profiles/stream_c2.json
"""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
SECONDS, WINDOWS_S, WARMUP, STREAMS, LONG_CALLS = 64.0, (1.0, 2.0, 8.0), 3, 3, 5


def one_stream(model, x, W, O, seed):
    """Push x in hops of H; returns [(device ms, host ms)] of the pushes that emitted, and the output length."""
    import torch

    H = W - O
    rows, n_out = [], 0
    with model.stream(W, O, batch=1, seed=seed) as s:
        for at in range(0, x.numel(), H):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t = time.perf_counter()
            e0.record()
            y = s.push(x[at:at + H])
            e1.record()
            e1.synchronize()
            host = 1e3 * (time.perf_counter() - t)
            if y.numel():
                rows.append((e0.elapsed_time(e1), host))
            n_out += y.numel()
        n_out += s.close().numel()
    return rows, n_out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="write the JSON here as well")
    a = ap.parse_args()
    import numpy as np
    import torch

    import bench
    from open_universe_amd import longform
    from open_universe_amd.utils.synthetic import synth_audio

    dev = torch.device("cuda:0")
    cfg, model = bench.build_model(dev)
    fs = int(cfg["fs"])
    T = int(SECONDS * fs)
    n_steps = int(model.diff_kwargs.n_steps)
    x = torch.from_numpy(synth_audio(T, fs, 0)[0].astype(np.float32)).to(dev)
    sync = lambda: torch.cuda.synchronize(dev)   # noqa: E731
    out = {"shape": f"full-width PP16, synthetic weights, one {SECONDS:g} s stream at {fs} Hz, {n_steps} steps, "
                    "batch 1, overlap = window / 8, pushed in hops of H",
           "warmup_streams": WARMUP, "timed_streams": STREAMS, "enhance_long_calls": LONG_CALLS, "windows": []}
    with torch.no_grad():
        for ws in WINDOWS_S:
            W = int(ws * fs)
            O = W // 8
            H = W - O
            for k in range(WARMUP):
                one_stream(model, x, W, O, k)
            sync()
            rows = []
            for k in range(STREAMS):
                r, n_out = one_stream(model, x, W, O, 100 + k)
                assert n_out == T, (n_out, T)
                rows += r
            dev_ms, host_ms = [r[0] for r in rows], [r[1] for r in rows]
            rng = torch.Generator(device=dev).manual_seed(1)
            for _ in range(WARMUP):
                model.enhance_long(x, W, O, batch=1, rng=rng)
            sync()
            long_ms = []
            for _ in range(LONG_CALLS):
                t = time.perf_counter()
                model.enhance_long(x, W, O, batch=1, rng=rng)
                sync()
                long_ms.append(1e3 * (time.perf_counter() - t))
            n = longform.n_windows(T, W, O)
            long_med = statistics.median(long_ms)
            out["windows"].append({
                "window_s": ws, "overlap_s": O / fs, "hop_s": H / fs, "windows": n, "timed_pushes": len(rows),
                "push_device_ms_median": statistics.median(dev_ms), "push_device_ms_max": max(dev_ms),
                "push_host_ms_median": statistics.median(host_ms), "push_host_ms_max": max(host_ms),
                "stream_realtime_factor": (H / fs) / (1e-3 * statistics.median(host_ms)),
                "enhance_long_b1_ms_median": long_med, "enhance_long_b1_ms_per_window": long_med / n,
                "enhance_long_b1_realtime_factor": SECONDS / (1e-3 * long_med)})
    out["range_fallbacks"], out["range_widenings"] = model.range_fallbacks, model.range_widenings
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
