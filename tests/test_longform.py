"""The windowed enhance's definition (open_universe_amd/longform.py) on the
CPU: window arithmetic and crossfade weights over a grid of (T, W, O), the
global noise shapes of ``noise_shapes(..., window=, overlap=)``, and the CLI's
window options.  No GPU."""
import math
from types import SimpleNamespace

import numpy as np
import pytest

from open_universe_amd import longform as LF
from open_universe_amd.configs import get_config
from open_universe_amd.networks.universe import UniverseGAN

# (T, W, O): T = W; T = W + 1; T = W + k H exactly (k = 1, 2, 3); O = 0; O = W / 2; a last window shifted back
# by less than O (T = W + 2 H - 3 = 10397: by 3) and by nearly a whole hop (T = W + H + 5 = 7205); T < W; tiny windows
GRID = [
    (4000, 4000, 800), (4001, 4000, 800), (7200, 4000, 800), (10400, 4000, 800), (13600, 4000, 800),
    (9000, 4000, 800), (9000, 4000, 0), (8000, 4000, 0), (8001, 4000, 0), (9000, 4000, 2000), (8000, 4000, 2000),
    (4001, 4000, 2000), (4001, 4000, 0), (10397, 4000, 800), (7205, 4000, 800), (3000, 4000, 800), (1, 4000, 0),
    (23, 7, 3), (22, 7, 3), (50, 7, 0), (51, 8, 4), (9, 2, 1), (5, 1, 0),
]


@pytest.mark.parametrize("T,W,O", GRID)
def test_window_arithmetic(T, W, O):
    n = LF.n_windows(T, W, O)
    H = W - O
    assert n == (1 if T <= W else 1 + math.ceil((T - W) / H))
    st = LF.starts(T, W, O)
    assert len(st) == n and st[0] == 0
    assert all(a < b for a, b in zip(st, st[1:])), st            # strictly monotone
    assert all(b <= a + H for a, b in zip(st, st[1:])), st       # no gap: consecutive windows overlap by >= O
    assert st[-1] + W == T if T >= W else st == [0]              # the last window ends with the clip
    covered = np.zeros(T, bool)
    for s in st:
        covered[s:s + W] = True
    assert covered.all()
    for i in (n, n + 1, n + 1000):                               # i >= n clamps to the last window
        assert LF.start(i, T, W, O) == st[-1]
    for i, s in enumerate(st):
        assert s == min(i * H, max(T - W, 0))


@pytest.mark.parametrize("T,W,O", GRID)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_weights(T, W, O, dtype):
    w = LF.weights(T, W, O, dtype=dtype)
    st = LF.starts(T, W, O)
    assert w.shape == (len(st), T) and w.dtype == dtype
    assert (w >= 0).all() and (w <= 1).all()
    assert ((w != 0).sum(axis=0) <= 2).all()                     # at most two windows at a sample
    assert ((w != 0).sum(axis=0) >= 1).all()
    total = w.astype(np.float64).sum(axis=0)
    assert np.abs(total - 1.0).max() <= 2.0 ** -23, np.abs(total - 1.0).max()   # one float32 ulp of 1
    for i, s in enumerate(st):
        outside = np.ones(T, bool)
        outside[s:s + W] = False
        assert not w[i, outside].any()                           # 0 outside its own span
        if i:
            lo = st[i - 1] + W - O                               # the fade-in of window i
            assert not w[i, :lo].any()                           # 0 before it (the shifted last window's head)
            u = np.arange(O)
            f = np.sin(np.pi * (2 * u + 1) / (4 * O)) ** 2 if O else u
            np.testing.assert_allclose(w[i, lo:lo + O], f, rtol=0, atol=2.0 ** -24)
            np.testing.assert_allclose(w[i - 1, lo:lo + O], 1 - f, rtol=0, atol=2.0 ** -24)
            assert not w[i - 1, lo + O:].any()


def test_fade_is_symmetric_and_never_zero():
    for O in (1, 2, 3, 800, 2000):
        f = LF.fade(O)
        np.testing.assert_allclose(f + f[::-1], 1.0, rtol=0, atol=1e-15)   # f(u) + f(O - 1 - u) = 1
        assert f.min() > 0 and f.max() < 1
        tab = LF.fade_table(O)
        assert tab.dtype == np.float32 and tab.shape == (2, O)
        assert np.abs(tab.astype(np.float64).sum(axis=0) - 1).max() <= 2.0 ** -23


def test_overlap_add_of_ones_is_one_and_groups():
    T, W, O = 9000, 4000, 800
    y = LF.overlap_add(np.ones((3, W)), T, W, O)
    np.testing.assert_allclose(y, 1.0, rtol=0, atol=1e-15)
    assert LF.groups(T, W, O, 2) == (2, [0, 2])
    assert LF.groups(T, W, O, 8) == (3, [0])
    assert LF.groups(4001, W, O, 8) == (2, [0])
    assert LF.noise_len(T, W, O, 4160) == 5000 + 4160


@pytest.mark.parametrize("T,W,O", [(9000, 4000, 2001), (9000, 4000, -1), (9000, 0, 0), (0, 4000, 0), (9, 3, 2)])
def test_bad_geometry_is_refused(T, W, O):
    with pytest.raises(ValueError):
        LF.check(T, W, O)


# ------------------------------------------------------------------ noise shapes
@pytest.fixture(scope="module")
def model():
    cfg = get_config("pp16", 4)
    return UniverseGAN(**{k: v for k, v in cfg.items() if k != "_target_"})


def _old_shapes(model, mix_shape, n_steps=None, target=None, use_aux_signal=False, ensemble=None, warm_start=None):
    """noise_shapes as it was before the window keywords."""
    n_steps = model.diff_kwargs.n_steps if n_steps is None else n_steps
    shape = tuple(mix_shape)
    shape = (1, 1) + shape if len(shape) == 1 else (shape[0], 1, shape[1]) if len(shape) == 2 else shape
    B, T = shape[0] * (ensemble or 1), shape[-1]
    Tp = T + model.tot_ds - T % model.tot_ds
    if target is not None:
        return [(B, 1, Tp)] * (2 * n_steps)
    if use_aux_signal:
        return []
    return [(B, 1, Tp)] * (1 + (n_steps - 1 - (warm_start or 0)))


CASES = [((4000,), {}), ((2, 4000), {}), ((3, 1, 4161), {"n_steps": 5}), ((2, 9000), {"ensemble": 3}),
         ((2, 9000), {"warm_start": 2}), ((9000,), {"use_aux_signal": True}), ((1, 9000), {"target": object()}),
         ((16000 * 3,), {"n_steps": 2})]


@pytest.mark.parametrize("shape,kw", CASES)
def test_noise_shapes_without_the_window_keywords_are_unchanged(model, shape, kw):
    assert model.noise_shapes(shape, **kw) == _old_shapes(model, shape, **kw)
    assert model.noise_shapes(shape, window=None, overlap=None, **kw) == _old_shapes(model, shape, **kw)


def test_noise_shapes_with_a_window(model):
    W, O = 4000, 800
    Tp = W + model.tot_ds - W % model.tot_ds
    n = model.diff_kwargs.n_steps
    assert model.noise_shapes((9000,), window=W, overlap=O) == [(1, 1, 5000 + Tp)] * n
    assert model.noise_shapes((9000,), n_steps=3, window=W, overlap=O) == [(1, 1, 5000 + Tp)] * 3
    assert model.noise_shapes((2, 10400), n_steps=3, window=W, overlap=O) == [(1, 1, 6400 + Tp)] * 6   # clip by clip
    assert model.noise_shapes((1, 1, 4001), n_steps=3, window=W, overlap=O) == [(1, 1, 1 + Tp)] * 3
    # a clip that fits the window is one plain enhance
    for T in (4000, 3000):
        assert model.noise_shapes((2, T), n_steps=3, window=W, overlap=O) == _old_shapes(model, (2, T), n_steps=3)
    for kw in ({"ensemble": 2}, {"warm_start": 1}, {"use_aux_signal": True}, {"target": object()}):
        with pytest.raises(NotImplementedError):
            model.noise_shapes((9000,), window=W, overlap=O, **kw)
        assert model.noise_shapes((3000,), window=W, overlap=O, **kw) == _old_shapes(model, (3000,), **kw)


# ------------------------------------------------------------------ CLI
def test_cli_window_options():
    from open_universe_amd.bin import enhance as cli

    base = ["in", "out", "--model", "m.ckpt"]
    a, rest = cli.build_parser().parse_known_args(base + ["--n_steps", "3"])
    assert a.window is None and a.window_batch == 8 and a.streams == 2 and a.chunk == 8 and a.seed == 1028282
    assert rest == ["--n_steps", "3"]
    assert cli.window_settings(a, 16000) is None
    a, _ = cli.build_parser().parse_known_args(base + ["--window", "0.25", "--overlap", "0.05", "--window-batch", "2"])
    assert (a.window, a.overlap, a.window_batch) == (0.25, 0.05, 2)
    assert cli.window_settings(a, 16000) == (4000, 800)
    a, _ = cli.build_parser().parse_known_args(base + ["--window", "8"])
    assert cli.window_settings(a, 16000) == (128000, 8000)       # the default overlap, 0.5 s
    for bad in (["--window", "1", "--overlap", "0.6"], ["--window", "0"], ["--window", "1", "--overlap", "-0.1"],
                ["--window", "1", "--window-batch", "0"]):
        a, _ = cli.build_parser().parse_known_args(base + bad)
        with pytest.raises(SystemExit):
            cli.window_settings(a, 16000)
    assert cli.window_settings(SimpleNamespace(window=None), 16000) is None
