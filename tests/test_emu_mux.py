"""CPU emulation of the mux kernels (csrc/ou_mux.hip): the HIP source compiled
for the host against the tests/emu shim and run, as a stand-alone program under
AddressSanitizer, with exact-size buffers.  The kernels have neither barriers
nor LDS, so the emulated values are real: tests/emu/mux_emu.cpp checks the
gather over three rings that wrap at different places -- W = 64 with O in
{0, 1, 7, 32}, window starts of every residue mod 4, noise windows of 64 and 67
values, positions past 2^32, 33 slots in two launches, padding slots -- against
the un-wrapped signals and a host loop over the same generator function; the
overlap-add inside whole sessions, outputs and carries starting as NaN and
padding rows NaN, bit for bit per channel against the per-sample rule of that
channel's whole stream -- two windows of a channel in one group, a channel's
windows in different groups and different runs, every way to close, a call of
carry-only closings alone, 40 runs in two launches, output offsets of every
residue mod 4; and every refusal of the two entry points.  No GPU involved."""
import os
import shutil

import pytest

from test_emu_kernels import ASAN, CLANG, ROOT, _build, _must_fail, _mutant, _run

pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason="ROCm clang++ not present")


def test_mux_kernels_in_bounds_and_correct(tmp_path):
    exe = str(tmp_path / "mux_emu")
    _build("mux_emu.cpp", exe, *ASAN)
    out = _run([exe], env={"OUHIP_EMU_BLOCKS": "0"})   # every workgroup
    assert "ok:" in out and " 0 launches" not in out and " 0 calls refused" not in out


def test_emulator_catches_a_window_that_leaves_its_ring(tmp_path):
    """The rings are one buffer, so a window that wraps must wrap inside its
    own channel's ring.  With the wrap of the dword path dropped, a lane whose
    four samples straddle the end of a ring reads on into the next channel's --
    and, for the last channel, past the buffer, which the exact-size blocks
    report."""
    src = _mutant(tmp_path, "ou_mux.hip", "ring[p + k < cap ? p + k : p + k - cap]", "ring[p + k]")
    for h in ("ou_stream.hip", "ou_normal.h", "ou_philox.h"):   # what ou_mux.hip shares with ou_stream.hip
        shutil.copy(os.path.join(ROOT, "open_universe_amd", "csrc", h), os.path.dirname(src))
    exe = str(tmp_path / "mux_emu_rev")
    _build("mux_emu.cpp", exe, *ASAN, f'-DOU_EMU_MUX_SRC="{src}"')
    _must_fail([exe], env={"OUHIP_EMU_BLOCKS": "0"})
