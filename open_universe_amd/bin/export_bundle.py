"""Export a model's ``enhance()`` for one clip shape as a bundle file that
``ou_bundle_load`` replays from any host (open_universe_amd.bundle.Bundle, or
a C program: examples/enhance_host.cpp):

    python -m open_universe_amd.bin.export_bundle --model CKPT --seconds S \
        [--batch B --n-steps N --epsilon E --keep-rms] OUT.oub

The plan is recorded on the HIP device and run once on a synthetic clip, so
the file carries tuned tiles and settled split-f16 exponents.
"""
import argparse
import os
from pathlib import Path

import torch

from .. import inference_utils
from ..bundle import export_bundle


def main(argv=None):
    parser = argparse.ArgumentParser(description="Export enhance() for one (batch, length) as a bundle file")
    parser.add_argument("output", type=Path, help="Bundle file to write (.oub)")
    parser.add_argument("--model", type=str, required=True, help="Local checkpoint (.ckpt) of the model")
    parser.add_argument("--model-strict", action="store_true", help="Strict state-dict loading")
    parser.add_argument("--seconds", type=float, required=True, help="Clip length in seconds at the model's rate")
    parser.add_argument("--batch", type=int, default=1, help="Clips per call")
    parser.add_argument("--n-steps", type=int, default=None, help="Diffusion steps (default: the model's)")
    parser.add_argument("--epsilon", type=float, default=None, help="Sampler epsilon (default: the model's)")
    parser.add_argument("--keep-rms", action="store_true", help="Restore the input's RMS on the output")
    parser.add_argument("--device", type=str, default=None, help="cuda:X (default: cuda:LOCAL_RANK)")
    args = parser.parse_args(argv)
    device = args.device or f"cuda:{int(os.environ.get('LOCAL_RANK', '0'))}"
    if not device.startswith("cuda") or not torch.cuda.is_available():
        raise SystemExit("export_bundle records on a ROCm device (cuda:X)")
    torch.cuda.set_device(torch.device(device))
    model = inference_utils.load_model(args.model, device=device, strict=args.model_strict)
    length = int(round(args.seconds * model.fs))
    ex = export_bundle(model, str(args.output), args.batch, length, n_steps=args.n_steps, epsilon=args.epsilon,
                       keep_rms=args.keep_rms, name=Path(args.model).stem)
    print(f"wrote {ex.path}: batch {args.batch} x {length} samples, {len(ex.plan.prog)} ops, "
          f"{len(ex.regions)} regions, {ex.file_bytes / 2**20:.1f} MiB")


if __name__ == "__main__":
    main()
