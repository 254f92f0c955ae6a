"""CPU emulation of the pooled windows' kernels (csrc/ou_pool.hip): the HIP
source compiled for the host against the tests/emu shim and run, as a
stand-alone program under AddressSanitizer, over the shapes of
tests/test_gpu_long_pool.py with exact-size buffers.  The kernels have neither
barriers nor LDS, so the emulated values are real: tests/emu/pool_emu.cpp
checks the gather bit for bit, the overlap-add -- every result starting as
NaN -- bit for bit against its host restatement of the ownership rule for
every grouping, calls of more than 32 slots, every refusal of the three entry
points, and the slot arithmetic past 2^31 samples.  No GPU involved."""
import os

import pytest

from test_emu_kernels import ASAN, CLANG, _build, _must_fail, _mutant, _run

pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason="ROCm clang++ not present")


def test_pool_kernels_in_bounds_and_correct(tmp_path):
    exe = str(tmp_path / "pool_emu")
    _build("pool_emu.cpp", exe, *ASAN)
    out = _run([exe], env={"OUHIP_EMU_BLOCKS": "0"})   # every workgroup
    assert "ok:" in out and " 0 launches" not in out and " 0 calls refused" not in out


def test_emulator_catches_an_unguarded_last_vector(tmp_path):
    """A lane whose four values straddle the end of a noise row must take the
    guarded dword path: with the guard removed from the gather the 16-byte
    access runs past the row (noise_win = 4163), which the exact-size buffers
    report."""
    src = _mutant(tmp_path, "ou_pool.hip", "const bool whole = j + 4 <= win;", "const bool whole = true;")
    text = open(os.path.join(os.path.dirname(__file__), "emu", "pool_emu.cpp")).read()
    inc = '#include "../../open_universe_amd/csrc/ou_pool.hip"'
    assert inc in text
    prog = tmp_path / "pool_emu_rev.cpp"
    prog.write_text(text.replace(inc, f'#include "{src}"'))
    exe = str(tmp_path / "pool_emu_rev")
    _build(str(prog), exe, *ASAN)
    _must_fail([exe], env={"OUHIP_EMU_BLOCKS": "0"})
