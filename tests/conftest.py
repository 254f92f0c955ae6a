import glob
import io
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
GOLDEN = os.path.join(REPO, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs an MI355X (HIP device)")
    # under pytest-xdist, share the cores between workers (the oracle's torch
    # ops oversubscribe badly otherwise)
    n = int(os.environ.get("PYTEST_XDIST_WORKER_COUNT", "0") or 0)
    if n > 1:
        import torch

        torch.set_num_threads(max(1, (os.cpu_count() or 1) // n))


PART_BYTES = 1000 * 1024   # no fixture file reaches 1 MiB


def load_golden(tag):
    """The arrays of fixture ``tag``: ``<tag>.npz``, or, for a fixture that
    would pass PART_BYTES as one file, its parts ``<tag>.00.npz``,
    ``<tag>.01.npz``, ... (save_golden).  A part holds whole arrays under
    their names and, of an array too large for one part, flattened slices
    ``name@0``, ``name@1``, ... beside ``name@shape``; the arrays come back
    bit for bit, in the order they were saved."""
    paths = [os.path.join(GOLDEN, f"{tag}.npz")]
    if not os.path.exists(paths[0]):
        paths = sorted(glob.glob(os.path.join(GOLDEN, f"{tag}.[0-9][0-9].npz")))
        if not paths:
            raise FileNotFoundError(f"no golden fixture {tag!r} under {GOLDEN}")
    out, pieces = {}, {}
    for p in paths:
        with np.load(p, allow_pickle=False) as f:
            for k in f.files:
                if "@" in k:
                    name, i = k.split("@")
                    out.setdefault(name, None)   # keeps the array's place in the order
                    pieces.setdefault(name, {})[i] = f[k]
                else:
                    out[k] = f[k]
    for name, ps in pieces.items():
        shape = tuple(int(s) for s in ps.pop("shape"))
        out[name] = np.concatenate([ps[str(i)] for i in range(len(ps))]).reshape(shape)
    return out


def _npz_bytes(arrays):
    buf = io.BytesIO()
    np.savez_compressed(buf, **arrays)
    return buf.getbuffer().nbytes


def save_golden(tag, arrays):
    """Write fixture ``tag`` for load_golden: one ``<tag>.npz`` if it stays
    under PART_BYTES, else numbered parts that each do (tests/golden/make_golden.py)."""
    items = []   # (key, array, compressed bytes), in the arrays' order
    for name, a in arrays.items():
        a = np.asarray(a)
        c = _npz_bytes({name: a})
        if c <= PART_BYTES // 2:
            items.append((name, a, c))
            continue
        n = -(-c // (PART_BYTES // 2))   # slices of about half a part each
        flat = np.ascontiguousarray(a).reshape(-1)
        items.append((f"{name}@shape", np.asarray(a.shape, dtype=np.int64), 512))
        for i, s in enumerate(np.array_split(flat, n)):
            items.append((f"{name}@{i}", s, _npz_bytes({f"{name}@{i}": s})))
    parts, size = [{}], 0
    for k, a, c in items:
        if parts[-1] and size + c > PART_BYTES:
            parts.append({})
            size = 0
        parts[-1][k] = a
        size += c
    for old in [os.path.join(GOLDEN, f"{tag}.npz")] + glob.glob(os.path.join(GOLDEN, f"{tag}.[0-9][0-9].npz")):
        if os.path.exists(old):
            os.remove(old)
    for i, part in enumerate(parts):
        p = os.path.join(GOLDEN, f"{tag}.npz" if len(parts) == 1 else f"{tag}.{i:02d}.npz")
        np.savez_compressed(p, **part)
        assert os.path.getsize(p) <= PART_BYTES, (p, os.path.getsize(p))


def golden_state_dict(d, seed=0):
    """Synthetic weights for the golden manifest (same generator the fixture
    script applied to the reference model)."""
    from open_universe_amd.utils.synthetic import synth_state_dict

    spec = [(n, [int(s) for s in sh.split(",") if s != ""])
            for n, sh in zip(d["manifest_names"], d["manifest_shapes"])]
    rc_gain = float(d["synth_rc_gain"]) if "synth_rc_gain" in d else 1.0   # the damped family (pp24d)
    return synth_state_dict([(n, s) for n, s in spec if not n.startswith("loss_")], seed, rc_gain)


def rel_rms(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)) / max(np.sqrt(np.mean(b**2)), 1e-30))


def si_sdr(est, ref):
    """Scale-invariant SDR in dB (closed form, fast_bss_eval zero_mean=False,
    reference metrics/wrapper.py:197-213), over the flattened signals."""
    est = np.asarray(est, dtype=np.float64).ravel()
    ref = np.asarray(ref, dtype=np.float64).ravel()
    a = np.dot(est, ref) / max(np.dot(ref, ref), 1e-30)
    e = est - a * ref
    return float(10 * np.log10(max(np.dot(a * ref, a * ref), 1e-30) / max(np.dot(e, e), 1e-30)))


@pytest.fixture
def golden():
    return load_golden
