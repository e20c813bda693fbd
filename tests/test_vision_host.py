"""CPU tests of the vision tower's host-side pieces (no GPU): the SAM window maps the engine builds once per
(images, grid) against the reference's pad / reshape / transpose window partition (oracle.vision.Sam.block)."""
import ctypes as C

import numpy as np
import pytest

from dsocr._lib import check, lib


def _window_maps(n, g, W):
    nw = -(-g // W)
    t2w = np.full(n * g * g, -7, np.int32)
    w2t = np.full(n * nw * nw * W * W, -7, np.int32)
    check(lib().dsocr_window_maps(n, g, W, t2w.ctypes.data_as(C.c_void_p), w2t.ctypes.data_as(C.c_void_p)))
    return t2w, w2t


@pytest.mark.parametrize("n,g,W", [(1, 16, 14), (2, 8, 14), (1, 28, 14), (3, 5, 2), (1, 64, 14)])
def test_window_maps_match_the_reference_partition(n, g, W):
    t2w, w2t = _window_maps(n, g, W)
    rows = n * g * g
    assert t2w.min() >= 0 and t2w.max() < w2t.size
    assert np.unique(t2w).size == rows, "tok2win is not injective"
    assert np.array_equal(w2t[t2w], np.arange(rows))
    rest = np.ones(w2t.size, bool)
    rest[t2w] = False
    assert np.all(w2t[rest] == -1) and int((w2t >= 0).sum()) == rows
    # Sam.block: pad bottom / right to a multiple of the window, cut into windows, rows of [windows][W][W]
    c = 3
    x = np.arange(1, rows * c + 1, dtype=np.float32).reshape(n, g, g, c)
    p = (W - g % W) % W
    hp = g + p
    padded = np.zeros((n, hp, hp, c), np.float32)
    padded[:, :g, :g] = x
    win = padded.reshape(n, hp // W, W, hp // W, W, c).transpose(0, 1, 3, 2, 4, 5).reshape(-1, c)
    assert win.shape[0] == w2t.size
    scattered = np.zeros_like(win)
    scattered[t2w] = x.reshape(rows, c)
    assert np.array_equal(scattered, win)
    # and back: the un-partition keeps rows win2tok names and drops the padding
    back = np.zeros((rows, c), np.float32)
    back[w2t[w2t >= 0]] = win[w2t >= 0]
    assert np.array_equal(back, x.reshape(rows, c))


def test_window_maps_bad_arguments():
    buf = np.zeros(16, np.int32)
    p = buf.ctypes.data_as(C.c_void_p)
    assert lib().dsocr_window_maps(0, 4, 2, p, p) != 0
    assert lib().dsocr_window_maps(1, 4, 0, p, p) != 0
    assert lib().dsocr_window_maps(1, 4, 2, None, p) != 0
