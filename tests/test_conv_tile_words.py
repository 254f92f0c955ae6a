"""ou_conv_desc.tile is decoded in one place (ou_conv.hip decode_tile): every
word must get the answer it got from the scattered bit tests that function
replaced.  tests/golden/conv_tile_words.npz holds those answers, recorded by
tests/golden/make_conv_tile_words.py at the commit before the decoder; the same
module asks the questions here.  (No GPU: the queries are host code, and
ou_conv() runs against the CPU emulation shim of tests/emu.)"""
import importlib.util
import os

import numpy as np
import pytest

from open_universe_amd import _lib as L

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_conv_tile_words",
                                               os.path.join(HERE, "golden", "make_conv_tile_words.py"))
M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(M)


@pytest.fixture(scope="module")
def golden():
    return np.load(M.TABLE)


def test_tile_ok_answers_as_before(golden):
    """ou_conv_tile_ok(kt, tile) for five tap counts (2 has no kernel), every
    word below 1 << 18, and -1, 1 << 18, 1 << 20, 0x7fffffff."""
    ok, extra = M.tile_ok_tables(L.load())
    diff = np.flatnonzero(np.unpackbits(ok ^ golden["ok"], axis=1))
    assert diff.size == 0, [(M.OK_KT[i // M.NWORDS], hex(i % M.NWORDS)) for i in diff[:8]]
    np.testing.assert_array_equal(extra, golden["ok_extra"])
    assert golden["ok"].any(axis=1).tolist() == [kt != 2 for kt in M.OK_KT]   # the table is not empty


def test_lds_requests_as_before(golden):
    """ou_conv_lds_info's lds_request of every plain shape: f32, warp-specialised and split-f16 form."""
    lds = M.lds_table(L.load())
    assert lds.shape == golden["lds"].shape and lds.shape[1] == L.load().ou_conv_num_tiles()
    np.testing.assert_array_equal(lds, golden["lds"])
    assert (golden["lds"][:, :, 0] > 0).all()


@pytest.mark.skipif(not os.path.exists(M.CLANG), reason="ROCm clang++ not present")
def test_conv_refuses_and_accepts_as_before(golden, tmp_path):
    """ou_conv() on one tiny geometry per kernel family (tests/emu/
    conv_emu_words.cpp), every word of a shape id 0..31 and bits 8-17, and -1:
    the same words accepted, and the same one of -1 / -2 for each refusal --
    so the order of the dispatcher's checks is the recorded one."""
    codes = M.conv_codes(str(tmp_path))
    want = golden["codes"]
    assert codes.shape == want.shape
    bad = np.argwhere(codes != want)
    words = [(int(c), -1 if i == 32768 else hex((i & 31) | ((i >> 5) << L.TILE_TPW_SHIFT)), int(codes[c, i]),
              int(want[c, i])) for c, i in bad[:8]]
    assert not words, f"(case, word, code now, code before): {words}"
    assert (want == 0).any(axis=1).all()   # every case launches something
