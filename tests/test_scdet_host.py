"""CPU: dts_scdet_host (vf_scdet restated in plain C++) against the numpy restatement of the
contract (tests/_scdet_ref.py), every field with ==: integer sums, and IEEE-754 double
arithmetic in a fixed order with no multiply-add to fuse."""
import ctypes

import numpy as np
import pytest

import dtsffi as D
import _scdet_ref as R
from _util import random_frame

FMTS = [D.FMT_YUV420P, D.FMT_NV12, D.FMT_P010LE]
SIZES = [(37, 23), (64, 36), (130, 74)]


def scene_frames(w, h, fmt, n, rng, cuts=()):
    """n frames: a random base, small changes from frame to frame, a new base at every cut."""
    frames, base = [], None
    for f in range(n):
        if base is None or f in cuts:
            base = random_frame(w, h, fmt, rng)
        fr = [None if p is None else p.copy() for p in base]
        fr[0][...] = (fr[0].astype(np.int64) + rng.integers(-3, 4, fr[0].shape)).clip(0, 255).astype(np.uint8)
        frames.append(fr)
    return frames


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("w,h", SIZES)
def test_host_vs_reference(w, h, fmt):
    rng = np.random.default_rng(w * 7 + h + fmt)
    frames = scene_frames(w, h, fmt, 7, rng, cuts=(3, 5))
    for thr in (10.0, 0.0, 2.5):
        got = D.scdet_host(w, h, fmt, frames, thr)
        want = R.run(frames, w, h, fmt, thr)
        assert got == want, (thr, got, want)
    assert got[0] == {"sad": 0, "mafd": 0.0, "score": 0.0, "cut": 0, "has_prev": 0}
    assert any(s["cut"] for s in D.scdet_host(w, h, fmt, frames, 10.0)[1:])


def test_host_reads_the_padded_luma_only():
    """A pitch larger than the row and NULL chroma pointers: only w x h luma samples count."""
    w, h, fmt = 37, 23, D.FMT_YUV420P
    rng = np.random.default_rng(5)
    frames = []
    for _ in range(4):
        buf = rng.integers(0, 256, (h, w + 11), dtype=np.uint8)
        frames.append([buf[:, :w], None, None])
    assert D.scdet_host(w, h, fmt, frames) == R.run(frames, w, h, fmt)


def test_argument_refusals():
    L = D.lib()
    w, h = 16, 8
    fr = [D.alloc_frame(w, h, D.FMT_NV12) for _ in range(2)]
    arr = (D.Frame * 2)(*[D.frame_struct(f) for f in fr])
    out = (D.ScdStat * 2)()
    ok = lambda *a: L.dts_scdet_host(*a)
    assert ok(w, h, D.FMT_NV12, arr, 2, 10.0, out) == 0
    assert ok(w, h, D.FMT_NV12, None, 2, 10.0, out) == D.E_INVAL
    assert ok(w, h, D.FMT_NV12, arr, 2, 10.0, None) == D.E_INVAL
    assert ok(w, h, D.FMT_NV12, arr, 0, 10.0, out) == D.E_INVAL
    assert ok(0, h, D.FMT_NV12, arr, 2, 10.0, out) == D.E_INVAL
    assert ok(w, 0, D.FMT_NV12, arr, 2, 10.0, out) == D.E_INVAL
    assert ok(w, h, 7, arr, 2, 10.0, out) == D.E_INVAL
    assert ok(w, h, D.FMT_NV12, arr, 2, -0.5, out) == D.E_INVAL
    assert ok(w, h, D.FMT_NV12, arr, 2, 100.5, out) == D.E_INVAL
    assert ok(w, h, D.FMT_NV12, arr, 2, float("nan"), out) == D.E_INVAL
    assert ok(16385, h, D.FMT_NV12, arr, 2, 10.0, out) == D.E_RANGE
    assert ok(w, 16385, D.FMT_NV12, arr, 2, 10.0, out) == D.E_RANGE
    assert ok(w, h, D.FMT_NV12, arr, 2, 0.0, out) == 0 and ok(w, h, D.FMT_NV12, arr, 2, 100.0, out) == 0
    # the device-object calls refuse NULL without touching a device
    h_ = ctypes.c_void_p()
    assert L.dts_scdet_create(None, w, h, D.FMT_NV12, 10.0, 0, ctypes.byref(h_)) == D.E_INVAL
    assert L.dts_scdet_create(None, w, h, D.FMT_NV12, 10.0, 0, None) == D.E_INVAL
    assert L.dts_scdet_reset(None) == D.E_INVAL
    assert L.dts_scdet_run_device(None, None, 1, None) == D.E_INVAL
    assert L.dts_scdet_prime_host(None, arr, 1) == D.E_INVAL
    assert L.dts_scdet_fetch(None, out, 2) == D.E_INVAL
    assert L.dts_graph_set_scdet(None, None) == D.E_INVAL
    L.dts_scdet_destroy(None)


def test_struct_size_and_feature_probe():
    L = D.lib()
    assert ctypes.sizeof(D.ScdStat) == 32
    assert L.dts_abi_struct_size(D.STRUCT_SCD_STAT) == 32 > 0
    assert D.STRUCT_IDS[D.STRUCT_SCD_STAT] is D.ScdStat
    assert L.dts_abi_version() == 8           # new symbols and one struct id only: the ABI number stays


def test_exports_cover_the_new_calls():
    L = D.lib()
    for n in ("dts_scdet_create", "dts_scdet_destroy", "dts_scdet_reset", "dts_scdet_run_device",
              "dts_scdet_prime_host", "dts_scdet_fetch", "dts_graph_set_scdet", "dts_scdet_host"):
        assert n in D.EXPORTS and hasattr(L, n), n


def test_binding_accepts_a_library_from_before_the_feature():
    """An ABI-8 library without scene-change detection answers the probe with DTS_E_INVAL: the
    binding's layout check skips the struct it does not know, and refuses a wrong size."""
    L = D.lib()

    class Fake:
        def __init__(self, n):
            self.n = n

        def dts_abi_version(self):
            return D.ABI_VERSION

        def dts_abi_struct_size(self, which):
            return self.n if which == D.STRUCT_SCD_STAT else L.dts_abi_struct_size(which)
    D.abi_check(Fake(D.E_INVAL))
    D.abi_check(Fake(32))
    with pytest.raises(RuntimeError, match="ScdStat"):
        D.abi_check(Fake(40))
