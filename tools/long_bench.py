#!/usr/bin/env python
"""Measure the windowed enhance against the whole-clip one, not gated anywhere:
full-width PP16 synthetic weights (bench.py's model), one 64 s clip,

* ``enhance()`` on the whole clip;
* ``enhance_long`` at 8 s windows, 0.5 s overlap, ``batch`` 8 (nine windows: a
  full group and a second one holding the ninth window and seven copies of it),
  and beside it at ``batch`` 9, one group

3 warm-ups and 10 timed calls each, in one process on one device.  Written:
milliseconds per call, ``torch.cuda.max_memory_allocated`` of each mode (plans
and arenas dropped in between), the share of the two ou_long kernels (HIP
events around one call's gathers and overlap-adds, launched back to back on
the plan's buffers without the replays between them), and the SI-SDR between
the two outputs on the same seed.  With synthetic weights that SI-SDR says
nothing about perceived quality: it only shows how far the two definitions are
apart on this model.

    python tools/long_bench.py --out profiles/long_c64.json

``--pool`` measures the pooled leg instead: two such clips (18 windows) through
one ``enhance_long_many`` call, three replays of eight slots, against two
consecutive ``enhance_long`` calls, four replays -- the same warm-up and timed
call counts, one process, the same generator handed on from call to call.

    python tools/long_bench.py --pool --out profiles/long_pool.json
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
SECONDS, WINDOW_S, OVERLAP_S, BATCH, WARMUP, STEPS = 64.0, 8.0, 0.5, 8, 3, 10


def _timed(call, sync):
    for _ in range(WARMUP):
        call()
        sync()
    ms = []
    for _ in range(STEPS):
        t = time.perf_counter()
        call()
        sync()
        ms.append(1e3 * (time.perf_counter() - t))
    return {"median_ms": statistics.median(ms), "mean_ms": statistics.fmean(ms), "min_ms": min(ms), "max_ms": max(ms)}


def _si_sdr(est, ref):
    import numpy as np

    est, ref = np.asarray(est, np.float64).ravel(), np.asarray(ref, np.float64).ravel()
    a = np.dot(est, ref) / max(np.dot(ref, ref), 1e-30)
    e = est - a * ref
    return float(10 * np.log10(max(np.dot(a * ref, a * ref), 1e-30) / max(np.dot(e, e), 1e-30)))


def _kernel_ms(model, x, W, O, n_steps):
    """One call's ou_window_gather / ou_overlap_add launches between HIP
    events, on the recorded plan's own buffers (median of 10)."""
    import torch

    from open_universe_amd import _lib as L
    from open_universe_amd import longform

    lib, T = L.load(), x.numel()
    B, firsts = longform.groups(T, W, O, BATCH)
    key, _ = model._plan_spec(B, W, n_steps, model.diff_kwargs.epsilon)
    plan = model._plans[key]
    Ln = longform.noise_len(T, W, O, plan.Tp)
    G = torch.randn((plan.n_noise, Ln), device=x.device)
    y = torch.empty(T, device=x.device)
    fade = model._fade_table(O, x.device)
    sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    res = {"gather_ms": [], "overlap_add_ms": []}
    for _ in range(10):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        for first in firsts:
            L.check(lib.ou_window_gather(x.data_ptr(), 0, 1, T, W, O, first, B, W, plan.MIX.data_ptr(), 0, W, sp), "g")
            L.check(lib.ou_window_gather(G.data_ptr(), Ln, plan.n_noise, T, W, O, first, B, plan.Tp,
                                         plan.NZ.data_ptr(), B * plan.Tp, plan.Tp, sp), "g")
        ev[1].record()
        for first in firsts:
            L.check(lib.ou_overlap_add(plan.OUT.data_ptr(), W, T, W, O, first, B, fade.data_ptr(), y.data_ptr(), sp),
                    "o")
        ev[2].record()
        torch.cuda.synchronize()
        res["gather_ms"].append(ev[0].elapsed_time(ev[1]))
        res["overlap_add_ms"].append(ev[1].elapsed_time(ev[2]))
    return {k: statistics.median(v) for k, v in res.items()}, len(firsts)


def pooled():
    import numpy as np
    import torch

    import bench
    from open_universe_amd import longform
    from open_universe_amd.utils.synthetic import synth_audio

    dev = torch.device("cuda:0")
    cfg, model = bench.build_model(dev)
    fs = int(cfg["fs"])
    T, W, O = int(SECONDS * fs), int(WINDOW_S * fs), int(OVERLAP_S * fs)
    xs = [torch.from_numpy(synth_audio(T, fs, i)[0].astype(np.float32)).to(dev) for i in range(2)]
    sync = lambda: torch.cuda.synchronize(dev)   # noqa: E731
    B, slots = longform.pool([T, T], W, O, BATCH)
    out = {"shape": f"full-width PP16, synthetic weights, two {SECONDS:g} s clips at {fs} Hz, "
                    f"{int(model.diff_kwargs.n_steps)} steps",
           "window_s": WINDOW_S, "overlap_s": OVERLAP_S, "batch": BATCH, "warmup": WARMUP, "steps": STEPS,
           "windows": len(slots)}
    with torch.no_grad():
        rng = torch.Generator(device=dev).manual_seed(1)
        model.enhance(xs[0][:W], rng=rng)   # weights packed and tiles tuned outside both measurements
        sync()
        res = _timed(lambda: [model.enhance_long(x, W, O, batch=BATCH, rng=rng) for x in xs], sync)
        res["replays"] = 2 * len(longform.groups(T, W, O, BATCH)[1])
        out["enhance_long_twice"] = res
        res = _timed(lambda: model.enhance_long_many(xs, W, O, batch=BATCH, rng=rng), sync)
        res["replays"] = -(-len(slots) // B)
        out["enhance_long_many"] = res
        # the same seed: the same noise per clip, other neighbours in the groups
        r7 = torch.Generator(device=dev).manual_seed(7)
        seq = [model.enhance_long(x, W, O, batch=BATCH, rng=r7) for x in xs]
        many = model.enhance_long_many(xs, W, O, batch=BATCH, rng=torch.Generator(device=dev).manual_seed(7))
        out["rel_rms_many_vs_twice"] = [float(((a - b).double().square().mean() / b.double().square().mean()).sqrt())
                                        for a, b in zip(many, seq)]
    out["speedup"] = out["enhance_long_twice"]["median_ms"] / out["enhance_long_many"]["median_ms"]
    out["range_fallbacks"], out["range_widenings"] = model.range_fallbacks, model.range_widenings
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="write the JSON here as well")
    ap.add_argument("--pool", action="store_true", help="the pooled leg alone: enhance_long_many against two "
                                                        "enhance_long calls")
    a = ap.parse_args()
    if a.pool:
        text = json.dumps(pooled(), indent=1)
        print(text)
        if a.out:
            with open(a.out, "w") as f:
                f.write(text + "\n")
        return
    import numpy as np
    import torch

    import bench
    from open_universe_amd import longform
    from open_universe_amd.utils.synthetic import synth_audio

    dev = torch.device("cuda:0")
    cfg, model = bench.build_model(dev)
    fs = int(cfg["fs"])
    T, W, O = int(SECONDS * fs), int(WINDOW_S * fs), int(OVERLAP_S * fs)
    n_steps = int(model.diff_kwargs.n_steps)
    x = torch.from_numpy(synth_audio(T, fs, 0)[0].astype(np.float32)).to(dev)
    sync = lambda: torch.cuda.synchronize(dev)   # noqa: E731
    out = {"shape": f"full-width PP16, synthetic weights, one {SECONDS:g} s clip at {fs} Hz, {n_steps} steps",
           "window_s": WINDOW_S, "overlap_s": OVERLAP_S, "batch": BATCH, "warmup": WARMUP, "steps": STEPS}

    def drop_plans():
        model._plans.clear()
        getattr(model._get_engine(), "arenas", {}).clear()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(dev)

    with torch.no_grad():
        rng = torch.Generator(device=dev).manual_seed(1)
        model.enhance(x[:W], rng=rng)   # weights packed and tiles tuned outside both measurements
        sync()
        drop_plans()
        base = torch.cuda.memory_allocated(dev)
        res = _timed(lambda: model.enhance_long(x, W, O, batch=BATCH, rng=rng), sync)
        res["max_memory_allocated"] = torch.cuda.max_memory_allocated(dev)
        y_long = model.enhance_long(x, W, O, batch=BATCH, rng=torch.Generator(device=dev).manual_seed(7)).cpu()
        kern, n_groups = _kernel_ms(model, x, W, O, n_steps)
        res.update(kern, groups=n_groups,
                   long_kernels_share=(kern["gather_ms"] + kern["overlap_add_ms"]) / res["median_ms"])
        out["enhance_long"] = res
        # beside it: every window in one group (at batch 8 the ninth window runs as a second,
        # mostly padded group)
        n_win = longform.n_windows(T, W, O)
        drop_plans()
        res = _timed(lambda: model.enhance_long(x, W, O, batch=n_win, rng=rng), sync)
        res.update(batch=n_win, groups=1, max_memory_allocated=torch.cuda.max_memory_allocated(dev))
        out["enhance_long_one_group"] = res
        drop_plans()
        res = _timed(lambda: model.enhance(x, rng=rng), sync)
        res["max_memory_allocated"] = torch.cuda.max_memory_allocated(dev)
        y_whole = model.enhance(x, rng=torch.Generator(device=dev).manual_seed(7)).cpu()
        out["enhance_whole"] = res
    out["memory_allocated_before_plans"] = base
    out["speedup"] = out["enhance_whole"]["median_ms"] / out["enhance_long"]["median_ms"]
    out["si_sdr_long_vs_whole_db"] = _si_sdr(y_long.numpy(), y_whole.numpy())
    out["si_sdr_note"] = ("synthetic weights: this says nothing about perceived quality, only how far apart the two "
                          "definitions are on this model")
    out["range_fallbacks"], out["range_widenings"] = model.range_fallbacks, model.range_widenings
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
