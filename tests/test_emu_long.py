"""CPU emulation of the windowed enhance's kernels (csrc/ou_long.hip): the HIP
source compiled for the host against the tests/emu shim and run, as a
stand-alone program under AddressSanitizer, over the shapes of
tests/test_gpu_long.py with exact-size buffers.  The kernels have neither
barriers nor LDS, so the emulated values are real: tests/emu/long_emu.cpp also
checks them against its host restatement of the definition, the refusals of
both entry points, and one geometry past 2^31 samples through the arguments
alone.  No GPU involved."""
import os

import pytest

from test_emu_kernels import ASAN, CLANG, _build, _must_fail, _mutant, _run

pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason="ROCm clang++ not present")


def test_long_kernels_in_bounds_and_correct(tmp_path):
    exe = str(tmp_path / "long_emu")
    _build("long_emu.cpp", exe, *ASAN)
    out = _run([exe], env={"OUHIP_EMU_BLOCKS": "0"})   # every workgroup
    assert "ok:" in out and " 0 launches" not in out and " 0 calls refused" not in out


def test_emulator_catches_an_unguarded_last_vector(tmp_path):
    """A lane whose four values straddle the end of a window must take the
    guarded dword path: with the guard removed the 16-byte access runs past
    the window (win = 4003), which the exact-size buffers report."""
    src = _mutant(tmp_path, "ou_long.hip", "const bool whole = j + 4 <= win;", "const bool whole = true;")
    text = open(os.path.join(os.path.dirname(__file__), "emu", "long_emu.cpp")).read()
    inc = '#include "../../open_universe_amd/csrc/ou_long.hip"'
    assert inc in text
    prog = tmp_path / "long_emu_rev.cpp"
    prog.write_text(text.replace(inc, f'#include "{src}"'))
    exe = str(tmp_path / "long_emu_rev")
    _build(str(prog), exe, *ASAN)
    _must_fail([exe], env={"OUHIP_EMU_BLOCKS": "0"})
