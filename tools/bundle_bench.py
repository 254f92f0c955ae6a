#!/usr/bin/env python
"""Measure an exported bundle at the headline shape (bench.py's c2: full-width
PP16 synthetic weights, batch 1, 8 s, 8 steps), not gated anywhere:

* the bundle's file size and the export's wall time;
* in a fresh process: ``ou_bundle_load`` wall time, the first enhance, and
  steady-state ms per ``ou_model_enhance`` with native noise (20 calls after
  3 warm-ups, the stream synchronised after each);
* beside it, in another fresh process, the Python path from the same start
  line (device initialised, nothing built): model build, first ``enhance()``
  (weight folding and packing, tile tuning, recording) and its steady state.

    python tools/bundle_bench.py --out profiles/bundle_c2.json
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
SECONDS, WARMUP, STEPS = 8.0, 3, 20


def _clip(fs):
    import numpy as np
    import torch

    from open_universe_amd.utils.synthetic import synth_audio

    return torch.from_numpy(np.stack([synth_audio(int(SECONDS * fs), fs, 0)[0]]))


def _steady(call, sync):
    import statistics

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


def child_bundle(path):
    import torch

    torch.cuda.init()
    torch.zeros(1, device="cuda").item()   # the device is up before the clock starts
    from open_universe_amd.bundle import Bundle

    t0 = time.perf_counter()
    b = Bundle(path, capture=True)
    load_s = time.perf_counter() - t0
    mix = _clip(b.info["fs"]).cuda()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    b.enhance(mix, seed=1)
    b.status()
    first_s = time.perf_counter() - t1
    seeds = iter(range(2, 1000))
    res = _steady(lambda: b.enhance(mix, seed=next(seeds)), b.status)
    print(json.dumps({"load_s": load_s, "first_enhance_s": first_s, "start_to_first_output_s": load_s + first_s,
                      "enhance": res, "region_bytes": b.info["region_bytes"], "n_ops": b.info["n_ops"]}))


def child_python():
    import torch

    torch.cuda.init()
    torch.zeros(1, device="cuda").item()
    import bench

    t0 = time.perf_counter()
    cfg, model = bench.build_model(torch.device("cuda:0"))
    build_s = time.perf_counter() - t0
    mix = _clip(int(cfg["fs"])).cuda()
    rng = torch.Generator(device="cuda").manual_seed(1)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    with torch.no_grad():
        model.enhance(mix, rng=rng)
        torch.cuda.synchronize()
        first_s = time.perf_counter() - t1
        res = _steady(lambda: model.enhance(mix, rng=rng), torch.cuda.synchronize)
    print(json.dumps({"model_build_s": build_s, "first_enhance_s": first_s,
                      "start_to_first_output_s": build_s + first_s, "enhance": res}))


def _run(args):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True,
                       timeout=600, cwd=HERE)
    if r.returncode != 0:
        raise SystemExit(f"child {args} failed ({r.returncode}):\n{r.stderr[-3000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="write the JSON here as well")
    ap.add_argument("--child", choices=["bundle", "python"], default=None, help=argparse.SUPPRESS)
    ap.add_argument("--bundle", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child == "bundle":
        return child_bundle(a.bundle)
    if a.child == "python":
        return child_python()
    import torch

    import bench
    from open_universe_amd.bundle import export_bundle

    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "c2.oub")
        cfg, model = bench.build_model(torch.device("cuda:0"))
        t0 = time.perf_counter()
        with torch.no_grad():
            ex = export_bundle(model, path, 1, int(SECONDS * int(cfg["fs"])), name="pp16 synthetic")
        export_s = time.perf_counter() - t0
        out = {"shape": "c2: full-width PP16, synthetic weights, batch 1, 8 s at 16 kHz, 8 steps",
               "warmup": WARMUP, "steps": STEPS, "file_bytes": ex.file_bytes, "regions": len(ex.regions),
               "ops": len(ex.plan.prog), "relocations": len(ex.relocs), "export_s": export_s,
               "conv_prec": ex.engine.conv_prec}
        del ex, model
        torch.cuda.empty_cache()
        out["bundle"] = _run(["--child", "bundle", "--bundle", path])
        out["python"] = _run(["--child", "python"])
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
