"""Streaming enhance on a pipe: raw mono PCM at the model's rate on stdin, the
enhanced signal in the same format on stdout, written as soon as its samples
are final.

    arecord -t raw -f FLOAT_LE -r 16000 -c 1 | \
        python -m open_universe_amd.bin.enhance_stream --model exp/ckpt.ckpt --window 1 --overlap 0.125 | \
        aplay -t raw -f FLOAT_LE -r 16000 -c 1

``--model CKPT`` runs ``Universe.stream`` (the window, the overlap and the
group size are free); ``--bundle FILE`` runs ``Bundle.stream`` on an exported
bundle, whose window and group size are fixed in the file.  Sample ``t`` leaves
once window ``t // hop``'s group has run, which needs the input up to the end
of that group's last window; ``--window-batch 1`` is the low-latency case.
The output depends on ``--seed``, not on ``--chunk`` nor on how the pipe
delivered the bytes.  (Two processes agree bit for bit when they run the same
tiles: a bundle carries its own; with ``--model`` the tuner times its
candidates anew in every process, and ``OUHIP_AUTOTUNE=0`` takes the tiles
from the shapes alone.)  There is no resampling:
``--rate`` must be the model's.  A stream shorter than one window is an error.

``--channels N`` takes interleaved ``N``-channel PCM on stdin and writes it
interleaved on stdout.  Channel ``c`` is a stream of its own, with seed
``--seed + c`` and offset ``--offset``; all of them go through one mux
(``Universe.stream_mux`` / ``Bundle.stream_mux``), their
ready windows side by side in the slots of one plan of ``--window-batch``
windows, with a ``run()`` after every chunk.  The channels advance in lockstep,
so every run yields the same count for each.  A torn last frame is dropped.
Without ``--channels`` the program is the single stream above.
"""
import argparse
import sys

import numpy as np
import torch

FORMATS = {"f32le": ("<f4", 4), "s16le": ("<i2", 2)}


def build_parser():
    p = argparse.ArgumentParser(description="Enhance a raw mono PCM stream from stdin to stdout")
    src = p.add_mutually_exclusive_group(required=True)
    src.add_argument("--model", type=str, help="Local checkpoint (.ckpt) of the model")
    src.add_argument("--bundle", type=str, help="Exported enhance bundle (open_universe_amd.bin.export_bundle)")
    p.add_argument("--model-strict", action="store_true", help="Strict state-dict loading")
    p.add_argument("--format", choices=sorted(FORMATS), default="f32le", help="sample format of stdin and stdout")
    p.add_argument("--rate", type=int, default=None, help="sample rate of the stream; must be the model's")
    p.add_argument("--window", type=float, default=2.0, metavar="SECONDS", help="window length (with --model)")
    p.add_argument("--overlap", type=float, default=0.25, metavar="SECONDS",
                   help="crossfaded overlap of two windows, at most half the window")
    p.add_argument("--window-batch", type=int, default=1, metavar="N", help="windows per replay (with --model)")
    p.add_argument("--channels", type=int, default=None, metavar="N",
                   help="stdin and stdout are interleaved N-channel PCM: N streams through one mux, channel c with "
                        "seed --seed + c")
    p.add_argument("--chunk", type=float, default=0.1, metavar="SECONDS", help="samples read from stdin per push")
    p.add_argument("--seed", type=int, default=1028282, help="Seed of the sampler noise")
    p.add_argument("--offset", type=int, default=0, help="Philox counter offset of the sampler noise")
    p.add_argument("--device", type=str, default="cuda:0", help="cuda:X")
    p.add_argument("--n_steps", type=int, default=None, help="sampler steps (with --model; default: the model's)")
    p.add_argument("--epsilon", type=float, default=None, help="sampler epsilon (with --model; default: the model's)")
    p.add_argument("--keep_rms", action="store_true", help="restore each window's input RMS (with --model)")
    return p


def decode(raw, fmt):
    """Bytes of whole samples -> float32 numpy in [-1, 1)."""
    a = np.frombuffer(raw, dtype=FORMATS[fmt][0])
    return a.astype(np.float32) / np.float32(32768.0) if fmt == "s16le" else a.astype(np.float32)


def encode(x, fmt):
    """float32 numpy -> bytes (s16le: rounded to nearest, clipped)."""
    if fmt == "s16le":
        return np.clip(np.rint(x.astype(np.float64) * 32768.0), -32768, 32767).astype("<i2").tobytes()
    return x.astype("<f4").tobytes()


def read_exactly(f, n):
    """Up to ``n`` bytes: short only at the end of the stream (a pipe may
    deliver less per read)."""
    parts = []
    while n > 0:
        b = f.read(n)
        if not b:
            break
        parts.append(b)
        n -= len(b)
    return b"".join(parts)


def check_rate(args, fs):
    if args.rate is not None and args.rate != fs:
        raise SystemExit(f"--rate {args.rate}: the model runs at {fs} Hz and a stream is not resampled")


def open_session(args):
    """(session, fs, status) for --model or --bundle; ``status()`` raises when
    the latest replays did not run clean (a bundle checks on request)."""
    if args.bundle:
        from open_universe_amd.bundle import Bundle

        b = Bundle(args.bundle)
        fs = int(b.info["fs"])
        check_rate(args, fs)
        O = int(round(args.overlap * fs))
        if O < 0 or O > b.length // 2:
            raise SystemExit(f"--overlap {args.overlap}: between 0 and half the bundle's window of {b.length} samples")
        if args.channels is not None:
            return b.stream_mux(O, args.channels), fs, b.status
        return b.stream(O, seed=args.seed, offset=args.offset), fs, b.status
    from open_universe_amd import inference_utils

    model = inference_utils.load_model(args.model, device=args.device, strict=args.model_strict)
    fs = int(model.fs)
    check_rate(args, fs)
    W, O = int(round(args.window * fs)), int(round(args.overlap * fs))
    if W < 1 or O < 0 or O > W // 2 or args.window_batch < 1:
        raise SystemExit(f"--window {args.window} --overlap {args.overlap} --window-batch {args.window_batch}: the "
                         "window must be positive, the overlap between 0 and half the window, the batch at least 1")
    if args.channels is not None:
        return model.stream_mux(W, O, args.channels, batch=args.window_batch, n_steps=args.n_steps,
                                epsilon=args.epsilon, keep_rms=args.keep_rms), fs, lambda: 0
    s = model.stream(W, O, batch=args.window_batch, n_steps=args.n_steps, epsilon=args.epsilon,
                     keep_rms=args.keep_rms, seed=args.seed, offset=args.offset)
    return s, fs, lambda: 0   # Universe.stream checks every group before it returns its samples


def run_mux(args, mux, fs, status, stdin, stdout):
    """--channels N: de-interleave every chunk, push each channel what its
    ring has room for, run, re-interleave what became final."""
    from open_universe_amd.longform import StreamShort

    N = args.channels
    width = FORMATS[args.format][1] * N
    n_chunk = max(1, int(round(args.chunk * fs)))

    def emit(ys):
        status()
        assert len({y.numel() for y in ys}) == 1, [y.numel() for y in ys]   # lockstep
        if ys[0].numel():
            stdout.write(encode(torch.stack(ys, dim=1).reshape(-1).cpu().numpy(), args.format))
            stdout.flush()

    with mux, torch.no_grad():
        for c in range(N):
            assert mux.open(seed=(args.seed + c) % 2**64, offset=args.offset) == c
        while True:
            raw = read_exactly(stdin, n_chunk * width)
            whole = len(raw) - len(raw) % width   # a torn last frame is dropped
            x = torch.from_numpy(decode(raw[:whole], args.format)).reshape(-1, N)
            at = 0
            while at < x.shape[0]:
                n = min(x.shape[0] - at, mux.room(0))
                for c in range(N):
                    mux.push(c, x[at:at + n, c])
                emit(mux.run())
                at += n
            if len(raw) < n_chunk * width:
                break
        try:
            for c in range(N):
                mux.close(c)
        except StreamShort as e:
            print(f"enhance_stream: {e}", file=sys.stderr)
            return 1
        emit(mux.run())
    return 0


def main(argv=None, stdin=None, stdout=None):
    args = build_parser().parse_args(argv)
    if args.channels is not None and args.channels < 1:
        raise SystemExit(f"--channels {args.channels}: at least 1")
    stdin = sys.stdin.buffer if stdin is None else stdin
    stdout = sys.stdout.buffer if stdout is None else stdout
    if not args.device.startswith("cuda") or not torch.cuda.is_available():
        raise SystemExit("open_universe_amd runs on a ROCm device (cuda:X); the CPU path is the reference")
    torch.cuda.set_device(torch.device(args.device))
    session, fs, status = open_session(args)
    if args.channels is not None:
        return run_mux(args, session, fs, status, stdin, stdout)
    width = FORMATS[args.format][1]
    n_chunk = max(1, int(round(args.chunk * fs)))

    def emit(y):
        status()
        if y.numel():
            stdout.write(encode(y.cpu().numpy(), args.format))
            stdout.flush()

    from open_universe_amd.longform import StreamShort

    with session, torch.no_grad():
        while True:
            raw = read_exactly(stdin, n_chunk * width)
            whole = len(raw) - len(raw) % width   # a torn last sample is dropped
            if whole:
                emit(session.push(torch.from_numpy(decode(raw[:whole], args.format))))
            if len(raw) < n_chunk * width:
                break
        try:
            emit(session.close())
        except StreamShort as e:
            print(f"enhance_stream: {e}", file=sys.stderr)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
