"""CPU emulation of the streaming kernels (csrc/ou_stream.hip): the HIP source
compiled for the host against the tests/emu shim and run, as a stand-alone
program under AddressSanitizer, with exact-size buffers.  The kernels have
neither barriers nor LDS, so the emulated values are real:
tests/emu/stream_emu.cpp checks the gather over a wrapping ring -- window starts
of every residue mod 4, noise windows of 4160 and 4163 values, positions past
2^32 -- against the un-wrapped signal and a host loop over the same generator
function; the overlap-add, outputs and carry starting as NaN, bit for bit
against the per-sample rule of the whole stream for every grouping and every
way a stream closes (nothing left to run, a shifted last window, T = W,
T = W + 1); and every refusal of the two entry points.  No GPU involved."""
import os
import shutil

import pytest

from test_emu_kernels import ASAN, CLANG, ROOT, _build, _must_fail, _mutant, _run

pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason="ROCm clang++ not present")


def test_stream_kernels_in_bounds_and_correct(tmp_path):
    exe = str(tmp_path / "stream_emu")
    _build("stream_emu.cpp", exe, *ASAN)
    out = _run([exe], env={"OUHIP_EMU_BLOCKS": "0"})   # every workgroup
    assert "ok:" in out and " 0 launches" not in out and " 0 calls refused" not in out


def test_emulator_catches_an_unguarded_last_counter(tmp_path):
    """The lane that owns the last counter of a noise row holds fewer than
    four of its values when the row ends inside the counter: it must take the
    guarded dword path.  With that guard dropped the 16-byte store runs past
    the row (noise_win = 4163, a 16-byte aligned base), which the exact-size
    buffers report."""
    src = _mutant(tmp_path, "ou_stream.hip", "const bool tail = j0 + 4 > noise_win;", "const bool tail = false;")
    for h in ("ou_normal.h", "ou_philox.h"):   # the headers ou_stream.hip shares with ou_rand.hip
        shutil.copy(os.path.join(ROOT, "open_universe_amd", "csrc", h), os.path.dirname(src))
    text = open(os.path.join(os.path.dirname(__file__), "emu", "stream_emu.cpp")).read()
    inc = '#include "../../open_universe_amd/csrc/ou_stream.hip"'
    assert inc in text
    prog = tmp_path / "stream_emu_rev.cpp"
    prog.write_text(text.replace(inc, f'#include "{src}"'))
    exe = str(tmp_path / "stream_emu_rev")
    _build(str(prog), exe, *ASAN)
    _must_fail([exe], env={"OUHIP_EMU_BLOCKS": "0"})
