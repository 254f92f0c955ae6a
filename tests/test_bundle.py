"""Exported enhance bundles on the CPU (open_universe_amd/bundle.py,
csrc/ou_bundle.cpp): plans recorded without a GPU round-trip through the file
and the host layer of the loader byte for byte, relocate exactly, and a
damaged file is refused; the Philox block function answers Random123's
known-answer vectors."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

from conftest import golden_state_dict, load_golden
from open_universe_amd import _lib as L
from open_universe_amd import bundle as Bd
from open_universe_amd.configs import get_config
from open_universe_amd.engine import Engine
from open_universe_amd.networks.universe import Universe, UniverseGAN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
HIPCC = "/opt/rocm/bin/hipcc"
CONFIGS = {"pp16_c4": ("pp16", 4), "orig16_c4": ("orig16", 4), "pp24_c4": ("pp24", 4), "pp16": ("pp16", None)}
B, T = 2, 3000


def _model(tag):
    name, nch = CONFIGS[tag]
    cfg = get_config(name, nch)
    cls = UniverseGAN if cfg["_target_"].endswith("UniverseGAN") else Universe
    m = cls(**{k: v for k, v in cfg.items() if k != "_target_"})
    m.load_state_dict(golden_state_dict(load_golden(tag)), strict=False)
    return m.eval()


@pytest.fixture(scope="module")
def recorded():
    """tag -> (model, record-only engine), built once."""
    out = {}
    for tag in CONFIGS:
        m = _model(tag)
        out[tag] = (m, Engine(m._model_cfg(), m.state_dict(), "cpu", _record_only=True))
    return out


def _export(recorded, tag, opts, path):
    m, eng = recorded[tag]
    plan = Bd.record_plan(m, eng, B, T, int(opts.get("n_steps", m.diff_kwargs.n_steps)), float(m.diff_kwargs.epsilon),
                      bool(opts.get("keep_rms", False)))
    return Bd.write_plan(eng, plan, str(path), {"fs": m.fs, "config": tag})


class _Open:
    def __init__(self, path):
        self.lib = L.load()
        self.h = ctypes.c_void_p()
        rc = self.lib.ou_bundle_open(os.fsencode(str(path)), ctypes.byref(self.h))
        assert rc == 0, self.lib.ou_last_error()
        self.meta = L.BundleMeta()
        assert self.lib.ou_bundle_info(self.h, ctypes.byref(self.meta)) == 0

    def materialize(self, bases, i, nbytes):
        buf = ctypes.create_string_buffer(nbytes)
        arr = (ctypes.c_uint64 * len(bases))(*bases)
        assert self.lib.ou_bundle_materialize(self.h, arr, i, buf) == 0, self.lib.ou_last_error()
        return buf.raw

    def close(self):
        self.lib.ou_bundle_close(self.h)


def _nonnull_pointer_offsets(d):
    """Byte offsets of the non-null pointer-typed fields of a ctypes
    descriptor (its own walk of Structure._fields_)."""
    out = set()

    def walk(st, base):
        for name, typ in st._fields_:
            off = base + getattr(st, name).offset
            if typ is ctypes.c_void_p:
                out.add(off)
            elif issubclass(typ, ctypes.Array) and typ._type_ is ctypes.c_void_p:
                out.update(off + 8 * k for k in range(typ._length_))
            elif issubclass(typ, ctypes.Structure):
                walk(typ, off)

    walk(type(d), 0)
    blob = bytes(d)
    return {o for o in out if struct.unpack_from("<Q", blob, o)[0]}


@pytest.mark.parametrize("opts", [{}, {"n_steps": 3, "keep_rms": True}], ids=["default", "steps3_rms"])
@pytest.mark.parametrize("tag", list(CONFIGS))
def test_round_trip_and_relocation(recorded, tag, opts, tmp_path):
    ex = _export(recorded, tag, opts, tmp_path / "b.oub")
    plan, prog = ex.plan, ex.plan.prog
    assert os.path.getsize(ex.path) == ex.file_bytes
    o = _Open(ex.path)
    m = o.meta
    assert (m.mix.batch, m.mix.length) == (B, T) == (m.out.batch, m.out.length)
    assert (m.noise.count, m.noise.batch, m.noise.length) == (plan.n_noise, B, plan.Tp)
    assert m.n_ops == len(prog) and m.n_regions == len(ex.regions)
    assert m.status.count == 4 + len(ex.engine.range_owners)
    assert m.arch == b"gfx950" and b'"fs": %d' % recorded[tag][0].fs in m.json
    # region 0 is the arena; kinds and sizes as exported
    for i, (lo, hi, kind) in enumerate(ex.regions):
        k, n, data = ctypes.c_int32(), ctypes.c_int64(), ctypes.c_void_p()
        assert o.lib.ou_bundle_region(o.h, i, ctypes.byref(k), ctypes.byref(n), ctypes.byref(data)) == 0
        assert (k.value, n.value) == (kind, hi - lo) and (kind == Bd.KIND_ARENA) == (i == 0)
        assert bool(data.value) == (kind == Bd.KIND_SAVED)
        if kind == Bd.KIND_SAVED and n.value <= 4096:   # the saved bytes are the tensor's
            assert ctypes.string_at(data.value, n.value) == ctypes.string_at(lo, n.value)
    kinds = prog.op_kinds()
    base0 = [lo for lo, _, _ in ex.regions]
    # every base moved by its own multiple of 256
    delta = [256 * (3 + 7 * r) * (-1 if r % 3 == 1 else 1) for r in range(len(base0))]
    base1 = [b + dl + (1 << 40) for b, dl in zip(base0, delta)]
    by_op = {}
    for op, off, region, roff in ex.relocs:
        by_op.setdefault(op, {})[off] = (region, roff)
    for i, d in enumerate(prog.descs):
        want = bytes(d)
        k, n, label = ctypes.c_int32(), ctypes.c_int64(), ctypes.c_char_p()
        assert o.lib.ou_bundle_op(o.h, i, ctypes.byref(k), ctypes.byref(n), ctypes.byref(label)) == 0
        assert (k.value, n.value) == (kinds[i], len(want))
        assert label.value == prog.labels[i].encode()[:39]
        assert o.materialize(base0, i, len(want)) == want, (i, prog.labels[i])
        # completeness: exactly the non-null pointer fields are relocated
        rel = by_op.get(i, {})
        assert set(rel) == _nonnull_pointer_offsets(d), (i, prog.labels[i])
        moved = bytearray(want)
        for off, (region, roff) in rel.items():
            assert struct.unpack_from("<Q", want, off)[0] == base0[region] + roff
            struct.pack_into("<Q", moved, off, base1[region] + roff)
        assert o.materialize(base1, i, len(want)) == bytes(moved), (i, prog.labels[i])
    o.close()


def test_export_bundle_from_a_cpu_model(tmp_path):
    """The public entry point on a model that sits on the CPU: recorded
    without running, the JSON carries the options."""
    import json

    m = _model("pp16_c4")
    ex = Bd.export_bundle(m, str(tmp_path / "b.oub"), B, T, n_steps=4, epsilon=1.2, keep_rms=True, name="pp16_c4")
    o = _Open(ex.path)
    js = json.loads(o.meta.json.decode())
    assert js == {"fs": 16000, "n_steps": 4, "epsilon": 1.2, "keep_rms": True, "conv_prec": ex.engine.conv_prec,
                  "config": "pp16_c4"}
    assert o.meta.noise.count == 4 and o.meta.n_ops == len(ex.plan.prog)
    o.close()


def test_unresolved_pointer_aborts_the_export(recorded, tmp_path):
    m, eng = recorded["pp16_c4"]
    plan = Bd.record_plan(m, eng, B, T, 3, 1.3, False)
    i = next(k for k, op in enumerate(plan.prog.op_kinds()) if op == L.OP_FINISH)
    plan.prog.descs[i].y = 0x10   # an address inside no tensor
    with pytest.raises(L.OuHipError) as e:
        Bd.write_plan(eng, plan, str(tmp_path / "b.oub"), {})
    assert f"op {i} " in str(e.value) and repr(plan.prog.labels[i]) in str(e.value) and "FinishArgs.y" in str(e.value)
    assert not os.path.exists(tmp_path / "b.oub")


@pytest.mark.parametrize("opt", [{"ensemble": 2}, {"use_aux_signal": True}, {"warm_start": 2},
                                 {"target": torch.zeros(1)}, {"fake_score_snr": 5.0}])
def test_unsupported_options_are_refused(opt, tmp_path):
    with pytest.raises(NotImplementedError):
        Bd.export_bundle(None, str(tmp_path / "b.oub"), B, T, **opt)


def test_bundle_structs_match_c(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/ouhip.h"', "int main(void){"]
    for cname, py in (("ou_bundle_io", L.BundleIo), ("ou_bundle_meta", L.BundleMeta)):
        lines.append(f'printf("{cname} size %zu\\n", sizeof({cname}));')
        for fname, _ in py._fields_:
            lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append("return 0;}")
    (tmp_path / "l.c").write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-std=c99", "-o", str(tmp_path / "l"), str(tmp_path / "l.c")])
    got = dict(line.rsplit(" ", 1) for line in subprocess.check_output([str(tmp_path / "l")]).decode().split("\n") if line)
    for cname, py in (("ou_bundle_io", L.BundleIo), ("ou_bundle_meta", L.BundleMeta)):
        assert int(got[f"{cname} size"]) == ctypes.sizeof(py)
        for fname, _ in py._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(py, fname).offset, (cname, fname)


# ------------------------------------------------------------------ Philox
def _philox_np(ctr, key):
    """Philox4x32-10 on uint32 arrays ctr (n, 4), key (n, 2)."""
    c = [ctr[:, i].astype(np.uint64) for i in range(4)]
    k0, k1 = key[:, 0].astype(np.uint64), key[:, 1].astype(np.uint64)
    M = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M, (k1 + np.uint64(0xBB67AE85)) & M
    return np.stack(c, axis=1).astype(np.uint32)


def _philox_lib(ctr, key):
    lib = L.load()
    out = np.empty_like(ctr)
    u32 = ctypes.POINTER(ctypes.c_uint32)
    for i in range(len(ctr)):
        assert lib.ou_philox4x32(ctr[i].ctypes.data_as(u32), key[i].ctypes.data_as(u32), out[i].ctypes.data_as(u32)) == 0
    return out


KAT = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
       ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
       ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
        (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]


def test_philox_known_answers():
    ctr = np.array([c for c, _, _ in KAT], dtype=np.uint32)
    key = np.array([k for _, k, _ in KAT], dtype=np.uint32)
    want = np.array([w for _, _, w in KAT], dtype=np.uint32)
    np.testing.assert_array_equal(_philox_lib(ctr, key), want)
    np.testing.assert_array_equal(_philox_np(ctr, key), want)
    rng = np.random.default_rng(5)
    ctr = rng.integers(0, 1 << 32, (4096, 4), dtype=np.uint64).astype(np.uint32)
    key = rng.integers(0, 1 << 32, (4096, 2), dtype=np.uint64).astype(np.uint32)
    np.testing.assert_array_equal(_philox_lib(ctr, key), _philox_np(ctr, key))


# ------------------------------------------------------------------ builds
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not present")
def test_host_example_compiles_and_links(tmp_path):
    """examples/enhance_host.cpp against the built library (compiled and
    linked only: running it needs a GPU, tests/test_gpu_bundle.py)."""
    exe = str(tmp_path / "enhance_host")
    r = subprocess.run([HIPCC, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "enhance_host.cpp"), "-o", exe,
                        "-L", os.path.dirname(L.LIB_PATH), "-louhip", "-Wl,-rpath," + os.path.dirname(L.LIB_PATH)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert os.path.exists(exe)


@pytest.mark.skipif(not os.path.exists(CLANG), reason="ROCm clang++ not present")
def test_damaged_files_are_refused_under_asan(recorded, tmp_path):
    """tests/emu/bundle_parse.cpp: the host layer alone, built as a
    stand-alone program with AddressSanitizer, against truncations, byte
    corruptions of the header and tables, and targeted damage of a valid
    pp16_c4 bundle."""
    ex = _export(recorded, "pp16_c4", {"n_steps": 3}, tmp_path / "good.oub")
    exe = str(tmp_path / "bundle_parse")
    cmd = [CLANG, "-std=c++17", "-O1", "-g0", "-fsanitize=address", "-fno-omit-frame-pointer",
           "-DOU_BUNDLE_STANDALONE", os.path.join(ROOT, "tests", "emu", "bundle_parse.cpp"),
           os.path.join(ROOT, "open_universe_amd", "csrc", "ou_bundle.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe, ex.path, str(tmp_path / "scratch.oub")], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and "ok:" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    assert "AddressSanitizer" not in r.stderr
