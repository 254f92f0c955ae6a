"""conv_tile_words.npz: what the library answers to every ou_conv_desc.tile word.

    python tests/golden/make_conv_tile_words.py LIBOUHIP_SO OU_CONV_HIP

records, from a library and an ou_conv.hip built at one commit,
  ok        ou_conv_tile_ok(kt, tile) for kt in OK_KT and every tile in
            [0, NWORDS), bit-packed per kt; ok_extra the same for OK_EXTRA
  lds       the lds_request of ou_conv_lds_info(kt, t | v) for kt in LDS_KT,
            t < ou_conv_num_tiles() and v in LDS_VARIANTS (written before the
            device query, so no GPU is needed)
  codes     ou_conv()'s return code for every word tests/emu/conv_emu_words.cpp
            tries, per case: 0 accepted, 1 / 2 refused with -1 / -2
The committed table was recorded at the commit before the host-side tile-word
decoder; tests/test_conv_tile_words.py asks the same questions of the tree."""
import ctypes
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from open_universe_amd import _lib as L  # noqa: E402  (the tile constants only: the library is an argument)

EMU = os.path.join(os.path.dirname(HERE), "emu")
TABLE = os.path.join(HERE, "conv_tile_words.npz")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
ASAN = ("-O0", "-g0", "-fsanitize=address", "-fno-omit-frame-pointer")

OK_KT = (1, 2, 3, 4, 5)   # 2: no kernel has two taps
NWORDS = 2 * L.TILE_FIR   # one past the highest field
OK_EXTRA = (-1, NWORDS, 4 * NWORDS, 0x7FFFFFFF)
LDS_KT = (1, 3, 4, 5)
LDS_VARIANTS = (0, L.TILE_WS, L.TILE_SPLIT_QUERY)
CASES = 8


def tile_ok_tables(lib):
    ok = lib.ou_conv_tile_ok
    words = np.array([[bool(ok(kt, t)) for t in range(NWORDS)] for kt in OK_KT])
    extra = np.array([[bool(ok(kt, t)) for t in OK_EXTRA] for kt in OK_KT])
    return np.packbits(words, axis=1), extra


def lds_table(lib):
    req = ctypes.c_int(0)
    out = np.zeros((len(LDS_KT), lib.ou_conv_num_tiles(), len(LDS_VARIANTS)), np.int32)
    for i, kt in enumerate(LDS_KT):
        for t in range(out.shape[1]):
            for j, v in enumerate(LDS_VARIANTS):
                lib.ou_conv_lds_info(kt, t | v, ctypes.byref(req), None)
                out[i, t, j] = req.value
    return out


def conv_codes(workdir, conv_src=None):
    """uint8 [CASES, 32769]: the driver's answer per case, the cases run side by side."""
    exe = os.path.join(workdir, "conv_emu_words")
    cmd = [CLANG, "-std=c++17", "-Wno-psabi", *ASAN, "-I", EMU, "-x", "c++", os.path.join(EMU, "conv_emu_words.cpp"),
           "-o", exe]
    if conv_src:
        cmd.append(f'-DOU_EMU_CONV_SRC="{os.path.abspath(conv_src)}"')
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    procs = [subprocess.Popen([exe, str(c)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)
             for c in range(CASES)]
    rows = []
    for c, p in enumerate(procs):
        out, err = p.communicate(timeout=900)
        assert p.returncode == 0, (c, err[-3000:])
        line = out.strip()
        assert len(line) == 32769 and set(line) <= set("012"), (c, sorted(set(line)), err[-1000:])
        rows.append(np.frombuffer(line.encode(), np.uint8) - ord("0"))
    return np.stack(rows)


if __name__ == "__main__":
    import tempfile

    lib = ctypes.CDLL(os.path.abspath(sys.argv[1]))
    ok, ok_extra = tile_ok_tables(lib)
    with tempfile.TemporaryDirectory() as tmp:
        codes = conv_codes(tmp, sys.argv[2])
    np.savez_compressed(TABLE, ok=ok, ok_extra=ok_extra, lds=lds_table(lib), codes=codes)
    print(TABLE, os.path.getsize(TABLE), "bytes")
