"""CPU emulation of ou_block's fused up-sampling stage (kEpiUp): the kernel
source compiled for the host against the bounds-checking shim (tests/emu) as
a stand-alone program, in fiber mode under AddressSanitizer -- every kEpiUp
instantiation at ragged lengths, every access in bounds, and u (and y where
it is stored) against a double-precision evaluation.  No GPU involved."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"

pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason="ROCm clang++ not present")


def test_fused_up_stage_in_bounds_and_values(tmp_path):
    exe = str(tmp_path / "block_up_emu")
    cmd = [CLANG, "-std=c++17", "-Wno-psabi", "-O1", "-g0", "-fsanitize=address", "-fno-omit-frame-pointer",
           "-DOU_EMU_FIBERS", "-I", EMU, "-x", "c++", os.path.join(EMU, "block_up_emu.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    # one process per (precision, channel count) group, side by side
    procs = [subprocess.Popen([exe, str(g)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)
             for g in range(4)]
    for p in procs:
        out, err = p.communicate(timeout=1800)
        assert p.returncode == 0 and "ok:" in out, (out[-2000:], err[-4000:])
