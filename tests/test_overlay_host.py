"""CPU: the burn-in overlay contract.  Known answers of the numpy restatement
(tests/_overlay_ref.py), dts_overlay_blend_host (the library's plain C++ restatement)
bit-exact against it for yuv420p and nv12, and the validation returns of the new calls."""
import ctypes

import numpy as np
import pytest

import dtsffi as D
import _overlay_ref as R
from _overlay_ref import IMAGES, RENDITIONS, SENTINEL, positions
from _util import random_frame


def padded_frame(w, h, fmt, rng, pad=5):
    """A random frame whose planes are views into sentinel-filled buffers with `pad` bytes of
    row padding: (planes, buffers)."""
    planes, bufs = [], []
    for s in D.plane_shapes(w, h, fmt):
        if s is None:
            planes.append(None)
            bufs.append(None)
            continue
        buf = np.full((s[0], s[1] + pad), SENTINEL, np.uint8)
        buf[:, :s[1]] = rng.integers(0, 256, s, dtype=np.uint8)
        planes.append(buf[:, :s[1]])
        bufs.append(buf)
    return planes, bufs


def test_div255_is_round_half_up():
    v = np.arange(0, 65026)
    assert np.array_equal(R.div255(v), (2 * v + 255) // 510)


def test_reference_known_answers():
    rng = np.random.default_rng(1)
    W, H = 64, 36
    for fmt in (D.FMT_YUV420P, D.FMT_NV12):
        base = random_frame(W, H, fmt, rng)
        img = R.random_image(17, 9, rng)
        # alpha 0 everywhere is the identity
        z = [img[0], img[1], img[2], np.zeros_like(img[3])]
        got = R.blend([None if p is None else p.copy() for p in base], fmt, z, 10, 6)
        assert all(p is None or np.array_equal(p, q) for p, q in zip(got, base))
        # alpha 255 replaces luma exactly
        o = [img[0], img[1], img[2], np.full_like(img[3], 255)]
        got = R.blend([None if p is None else p.copy() for p in base], fmt, o, 10, 6)
        assert np.array_equal(got[0][6:15, 10:27], img[0])
        # an odd x / y gives the same result as x - 1 / y - 1
        a = R.blend([None if p is None else p.copy() for p in base], fmt, img, 11, 7)
        b = R.blend([None if p is None else p.copy() for p in base], fmt, img, 10, 6)
        assert all(p is None or np.array_equal(p, q) for p, q in zip(a, b))
    # a constant picture under constant alpha a over a constant frame gives div255
    for a in (1, 77, 128, 254):
        fr = [np.full((36, 64), 200, np.uint8), np.full((18, 32), 90, np.uint8), np.full((18, 32), 30, np.uint8)]
        img = [np.full((8, 16), 50, np.uint8), np.full((4, 8), 60, np.uint8), np.full((4, 8), 70, np.uint8),
               np.full((8, 16), a, np.uint8)]
        R.blend(fr, D.FMT_YUV420P, img, 4, 4)
        assert (fr[0][4:12, 4:20] == R.div255(200 * (255 - a) + 50 * a)).all()
        assert (fr[1][2:6, 2:10] == R.div255(90 * (255 - a) + 60 * a)).all()
        assert (fr[2][2:6, 2:10] == R.div255(30 * (255 - a) + 70 * a)).all()
        assert fr[0][3, 4] == 200 and fr[0][12, 4] == 200 and fr[0][4, 3] == 200 and fr[0][4, 20] == 200


def test_chroma_alpha_edges():
    """The last chroma column and row take the pair form even when w / h are even."""
    A = np.array([[10, 20, 30, 41], [50, 60, 70, 81], [90, 100, 110, 121], [130, 140, 150, 161]], np.uint8)
    ca = R.chroma_alpha(A)
    assert ca[0, 0] == (10 + 50 + 20 + 60) >> 2
    assert ca[0, 1] == (((30 + 70) >> 1) + 30) >> 1           # last column: no horizontal pair
    assert ca[1, 0] == (90 + ((90 + 100) >> 1)) >> 1           # last row: no vertical pair
    assert ca[1, 1] == 110
    assert R.chroma_alpha(np.array([[7]], np.uint8))[0, 0] == 7


@pytest.mark.parametrize("fmt", [D.FMT_YUV420P, D.FMT_NV12])
@pytest.mark.parametrize("W,H", RENDITIONS)
def test_blend_host_vs_reference(W, H, fmt):
    rng = np.random.default_rng(W * 3 + H + fmt)
    sizes = IMAGES + ([(80, 40)] if (W, H) == (64, 36) else [])
    for (w, h) in sizes:
        img = R.random_image(w, h, rng)
        for (x, y) in positions(W, H, w, h):
            planes, bufs = padded_frame(W, H, fmt, rng)
            want = [None if b is None else b.copy() for b in bufs]
            wv = [None if b is None else b[:, :p.shape[1]] for b, p in zip(want, planes)]
            R.blend(wv, fmt, img, x, y)
            D.overlay_blend_host(img, x, y, W, H, fmt, planes)
            for pl, (g, wnt) in enumerate(zip(bufs, want)):
                if g is not None:
                    assert np.array_equal(g, wnt), (w, h, x, y, pl, int((g != wnt).sum()))


def test_blend_host_wholly_outside_changes_nothing():
    rng = np.random.default_rng(5)
    planes, bufs = padded_frame(64, 36, D.FMT_NV12, rng)
    before = [None if b is None else b.copy() for b in bufs]
    img = R.random_image(16, 8, rng)
    for (x, y) in [(64, 0), (0, 36), (-16, 0), (0, -8), (1000, 1000), (-1000, -1000)]:
        D.overlay_blend_host(img, x, y, 64, 36, D.FMT_NV12, planes)
    assert all(b is None or np.array_equal(b, q) for b, q in zip(bufs, before))


def test_validation_and_exports():
    L = D.lib()
    for n in ("dts_overlay_create", "dts_overlay_destroy", "dts_overlay_run_device", "dts_graph_set_overlay",
              "dts_graph_set_position", "dts_overlay_blend_host"):
        assert hasattr(L, n) and n in D.EXPORTS
    assert D.ABI_VERSION == 8 and L.dts_abi_version() == 8
    assert ctypes.sizeof(D.OverlayImage) == 72 and ctypes.sizeof(D.OverlayItem) == 32
    assert L.dts_abi_struct_size(8) == 72 and L.dts_abi_struct_size(9) == 32
    # NULL / bad arguments return, never crash
    assert L.dts_overlay_create(None, None, 0, None, 0, None) == D.E_INVAL
    assert L.dts_overlay_run_device(None, 64, 36, 0, None, 1, 0, None) == D.E_INVAL
    assert L.dts_graph_set_overlay(None, 0, None) == D.E_INVAL
    assert L.dts_graph_set_position(None, 0) == D.E_INVAL
    assert L.dts_overlay_blend_host(None, 0, 0, 64, 36, 0, None) == D.E_INVAL
    L.dts_overlay_destroy(None)
    rng = np.random.default_rng(2)
    img = R.random_image(4, 4, rng)
    fr = random_frame(64, 36, D.FMT_YUV420P, rng)
    with pytest.raises(D.DtsError) as e:
        D.overlay_blend_host(img, 0, 0, 64, 36, D.FMT_P010LE, fr)
    assert e.value.code == D.E_UNSUPPORTED
    with pytest.raises(D.DtsError) as e:
        D.overlay_blend_host(img, 0, 0, 0, 36, D.FMT_YUV420P, fr)
    assert e.value.code == D.E_INVAL
