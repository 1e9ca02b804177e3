"""GPU: scene-change detection (k_scdet, dts_scdet_*) against the numpy restatement of the
contract (tests/_scdet_ref.py), every field with ==.  Batches live in one buffer of random
bytes -- pitch padding included, different in every frame -- that is compared whole afterwards:
the detector writes no byte of it, and counting or mis-aligning the padding shows in the sums."""
import ctypes

import numpy as np
import pytest

import dtsffi as D
import _scdet_ref as R
from _util import first_diff, oracle_frame, planes_equal, random_frame

pytestmark = pytest.mark.gpu

BIC = D.SCALE_BICUBIC
FMTS = [D.FMT_YUV420P, D.FMT_NV12, D.FMT_P010LE]
# a workgroup owns 256 x 2 units of 16 bytes = 8 KiB of luma: 37x23 and 64x36 fit one workgroup
# (p010: 64x36 is 288 units too), 130x74, 384x216 and 200x83 (a row of 12.5 units; 1079 units: two
# whole bands and a 55-unit one that ends inside a unit) leave a partial last band
SIZES = [(37, 23), (64, 36), (130, 74), (384, 216), (200, 83)]


def bps(fmt):
    return 2 if fmt == D.FMT_P010LE else 1


class Batch:
    """n frames of (w, h, fmt) in one buffer of random bytes, host mirror `host` [n, fb].  The
    luma pitch is the row bytes + 1 rounded up to 16, plus `skew` bytes; the luma base and the
    frame stride are skewed by the same amount (0: the 16-byte path, 4: the 4-byte path, one
    sample: the sample-sized path).  luma_only: no chroma planes at all (NULL pointers)."""

    def __init__(self, w, h, fmt, n, rng, skew=0, luma_only=False):
        self.w, self.h, self.fmt, self.n, self.skew = w, h, fmt, n, skew
        self.shapes = D.plane_shapes(w, h, fmt)
        if luma_only:
            self.shapes = [self.shapes[0], None, None]
        self.pitch, self.off = [], []
        o = skew
        for s in self.shapes:
            if s is None:
                self.pitch.append(0)
                self.off.append(0)
                continue
            p = (s[1] + 1 + 15) // 16 * 16 + skew
            self.pitch.append(p)
            self.off.append(o)
            o += (p * s[0] + 15) // 16 * 16
        self.fb = (o + 15) // 16 * 16 + 16 + skew
        self.host = rng.integers(0, 256, (n, self.fb), dtype=np.uint8)
        self.t = None

    def planes(self, f):
        return [None if s is None else
                self.host[f, o:o + p * s[0]].reshape(s[0], p)[:, :s[1]]
                for s, p, o in zip(self.shapes, self.pitch, self.off)]

    def frames(self):
        return [self.planes(f) for f in range(self.n)]

    def fill(self, frames):
        for f, fr in enumerate(frames):
            for v, p in zip(self.planes(f), fr):
                if v is not None:
                    v[...] = p
        return self

    def upload(self):
        import torch
        self.t = torch.from_numpy(self.host).cuda()
        return self

    def dev(self, first=0):
        d = D.DevFrames()
        for p, s in enumerate(self.shapes):
            d.data[p] = None if s is None else self.t.data_ptr() + first * self.fb + self.off[p]
            d.pitch[p] = self.pitch[p]
        d.frame_stride = self.fb
        return d

    def untouched(self):
        return np.array_equal(self.t.cpu().numpy(), self.host)


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _sync():
    import torch
    torch.cuda.synchronize()


def scene_frames(w, h, fmt, n, rng, starts=(0,), noise=2):
    """n frames of `scenes`: an independent uniform-random base at every start, frames within a
    scene = base + noise in [-noise, noise] on the luma bytes."""
    out, base = [], None
    for f in range(n):
        if f in starts or base is None:
            base = random_frame(w, h, fmt, rng)
        fr = [None if p is None else p.copy() for p in base]
        fr[0][...] = (fr[0].astype(np.int64) + rng.integers(-noise, noise + 1, fr[0].shape)).clip(0, 255).astype(np.uint8)
        out.append(fr)
    return out


def run_split(ctx, b, splits, threshold=10.0, max_pending=0, fetch_each=False):
    sd = D.Scdet(ctx, b.w, b.h, b.fmt, threshold, max_pending)
    got, f0 = [], 0
    for m in splits:
        sd.run_device(b.dev(f0), m, _stream())
        f0 += m
        if fetch_each:
            got += sd.fetch()
    got += sd.fetch()
    sd.close()
    return got


@pytest.mark.parametrize("skew", [0, 4, "sample"])
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("w,h", SIZES)
def test_run_device_vs_reference(ctx, w, h, fmt, skew):
    """9 frames in three consecutive runs of 1 + 5 + 3 (the kept plane carries over twice), one
    fetch at the end."""
    skew = bps(fmt) if skew == "sample" else skew
    rng = np.random.default_rng(w * 11 + h + 5 * fmt + skew)
    b = Batch(w, h, fmt, 9, rng, skew)
    fr = scene_frames(w, h, fmt, 9, rng, starts=(0, 4, 7))
    b.fill(fr).upload()
    want = R.run(b.frames(), w, h, fmt)
    got = run_split(ctx, b, (1, 5, 3))
    assert got == want
    assert b.untouched(), "the detector wrote to the batch"
    assert [s["cut"] for s in want] == [0, 0, 0, 0, 1, 0, 0, 1, 0]


def test_long_batch(ctx):
    """70 frames of 64x36 in one run: longer than the kernel's 64-frame LDS window."""
    w, h, fmt = 64, 36, D.FMT_NV12
    rng = np.random.default_rng(70)
    b = Batch(w, h, fmt, 70, rng, luma_only=True)          # (chroma pointers NULL)
    b.fill(scene_frames(w, h, fmt, 70, rng, starts=(0, 13, 63, 64, 65))).upload()
    assert run_split(ctx, b, (70,)) == R.run(b.frames(), w, h, fmt)
    # and with a kept plane in front: frames 1.. start a window at slot 0 with a predecessor
    assert run_split(ctx, b, (3, 67)) == R.run(b.frames(), w, h, fmt)
    assert b.untouched()


def test_two_streams_without_sync(ctx):
    """Two runs on two torch streams, nothing between them: the detector hands its kept plane
    and records over itself; the result equals the one-stream run."""
    import torch
    w, h, fmt = 384, 216, D.FMT_YUV420P
    rng = np.random.default_rng(2)
    b = Batch(w, h, fmt, 8, rng)
    b.fill(scene_frames(w, h, fmt, 8, rng, starts=(0, 3, 5))).upload()
    _sync()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    sd = D.Scdet(ctx, w, h, fmt)
    sd.run_device(b.dev(0), 5, s1.cuda_stream)
    sd.run_device(b.dev(5), 3, s2.cuda_stream)
    got = sd.fetch()
    sd.close()
    assert got == run_split(ctx, b, (8,)) == R.run(b.frames(), w, h, fmt)


def test_reset(ctx):
    w, h, fmt = 64, 36, D.FMT_YUV420P
    rng = np.random.default_rng(3)
    b = Batch(w, h, fmt, 6, rng).upload()
    sd = D.Scdet(ctx, w, h, fmt)
    sd.run_device(b.dev(0), 4, _stream())
    first = sd.fetch()
    assert first == R.run(b.frames()[:4], w, h, fmt)
    sd.run_device(b.dev(4), 1, _stream())        # pending when the reset comes: dropped
    sd.reset()
    assert sd.fetch() == []
    sd.run_device(b.dev(2), 4, _stream())
    assert sd.fetch() == R.run(b.frames()[2:], w, h, fmt)     # a new stream: no prev, prev_mafd 0
    sd.close()


def test_busy_and_short_cap(ctx):
    w, h, fmt = 64, 36, D.FMT_NV12
    rng = np.random.default_rng(4)
    b = Batch(w, h, fmt, 6, rng).upload()
    want = R.run(b.frames()[:4], w, h, fmt)
    sd = D.Scdet(ctx, w, h, fmt, max_pending=4)
    sd.run_device(b.dev(0), 3, _stream())
    d = b.dev(3)
    assert D.lib().dts_scdet_run_device(sd.h, ctypes.byref(d), 2, ctypes.c_void_p(_stream())) == D.E_BUSY
    sd.run_device(b.dev(3), 1, _stream())        # nothing was enqueued by the refused call
    assert D.lib().dts_scdet_run_device(sd.h, ctypes.byref(d), 1, ctypes.c_void_p(_stream())) == D.E_BUSY
    out = (D.ScdStat * 4)()
    assert D.lib().dts_scdet_fetch(sd.h, out, 3) == D.E_INVAL      # cap < pending: nothing consumed
    assert sd.fetch(4) == want
    assert sd.fetch(4) == []
    # refusals of the device call itself
    assert D.lib().dts_scdet_run_device(sd.h, ctypes.byref(d), 0, None) == D.E_INVAL
    assert D.lib().dts_scdet_run_device(sd.h, None, 1, None) == D.E_INVAL
    bad = b.dev(0)
    bad.data[0] = None
    assert D.lib().dts_scdet_run_device(sd.h, ctypes.byref(bad), 1, None) == D.E_INVAL
    sd.close()
    for thr in (-1.0, 100.5, float("nan")):
        hh = ctypes.c_void_p()
        assert D.lib().dts_scdet_create(ctx.h, w, h, fmt, thr, 0, ctypes.byref(hh)) == D.E_INVAL
    hh = ctypes.c_void_p()
    assert D.lib().dts_scdet_create(ctx.h, 16385, h, fmt, 10.0, 0, ctypes.byref(hh)) == D.E_RANGE
    assert D.lib().dts_scdet_create(ctx.h, w, h, 5, 10.0, 0, ctypes.byref(hh)) == D.E_INVAL


@pytest.mark.parametrize("fmt", [D.FMT_YUV420P, D.FMT_P010LE])
@pytest.mark.parametrize("s", [3, 1])
def test_priming(ctx, s, fmt):
    """A segment that starts at stream frame s: primed with frames s - 2 and s - 1 (frame 0 alone
    at s = 1) its statistics equal rows s .. of one uninterrupted run."""
    w, h = 130, 74
    rng = np.random.default_rng(10 + s + fmt)
    n = s + 5
    b = Batch(w, h, fmt, n, rng)
    b.fill(scene_frames(w, h, fmt, n, rng, starts=(0, s - 1, s + 2) if s > 1 else (0, 1, 3))).upload()
    whole = R.run(b.frames(), w, h, fmt)
    sd = D.Scdet(ctx, w, h, fmt)
    sd.run_device(b.dev(0), 2, _stream())        # state and records the priming must discard
    sd.prime_host(b.frames()[max(0, s - 2):s])
    sd.run_device(b.dev(s), n - s, _stream())
    got = sd.fetch()
    sd.close()
    assert got == whole[s:]
    assert got != R.run(b.frames()[s:], w, h, fmt)      # (an unprimed segment differs)


@pytest.mark.parametrize("fmt", [D.FMT_NV12, D.FMT_P010LE])
def test_u64_carry(ctx, fmt):
    """One 7680x4320 pair made on the device, all 0 against all 255 (p010: 1023 << 6), chroma
    pointers NULL: the frame's sum passes 2^32."""
    import torch
    w, h = 7680, 4320
    rowb = w * bps(fmt)
    t = torch.zeros((2, h * rowb), dtype=torch.uint8, device="cuda")
    if fmt == D.FMT_P010LE:
        t[1].view(torch.int16).fill_(-64)        # 0xffc0 = 1023 << 6
    else:
        t[1].fill_(255)
    d = D.DevFrames()
    d.data[0], d.pitch[0], d.frame_stride = t.data_ptr(), rowb, h * rowb
    sd = D.Scdet(ctx, w, h, fmt)
    sd.run_device(d, 2, _stream())
    got = sd.fetch()
    sd.close()
    peak = 1023 if fmt == D.FMT_P010LE else 255
    assert got[1]["sad"] == w * h * peak > 2 ** 32
    assert got[1]["mafd"] == float(w * h * peak) * 100.0 / float(w * h) / float(1 << (10 if peak == 1023 else 8))
    assert got[0]["has_prev"] == 0 and got[1]["has_prev"] == 1 and got[1]["cut"] == 1


def test_cuts(ctx):
    """12 frames of three scenes, threshold 10: the reference's scores stay 1.0 or more away from
    the threshold (the >= at exact equality is not what this test is about) and its cuts are
    exactly the two scene starts; then the device result is compared."""
    w, h, fmt = 130, 74, D.FMT_YUV420P
    rng = np.random.default_rng(12)
    b = Batch(w, h, fmt, 12, rng)
    b.fill(scene_frames(w, h, fmt, 12, rng, starts=(0, 4, 9), noise=2)).upload()
    want = R.run(b.frames(), w, h, fmt, 10.0)
    assert all(abs(s["score"] - 10.0) >= 1.0 for s in want)
    assert [f for f, s in enumerate(want) if s["cut"]] == [4, 9]
    assert run_split(ctx, b, (12,), 10.0) == want


def _out_bufs(outs, n):
    import torch
    dsts, bufs = [], []
    for (ow, oh, _of, _m) in outs:
        size = ow * oh + 2 * ((ow + 1) // 2) * ((oh + 1) // 2)
        t = torch.zeros((n, (size + 63) // 64 * 64), dtype=torch.uint8, device="cuda")
        d = D.DevFrames()
        d.data[0], d.data[1], d.data[2] = t.data_ptr(), t.data_ptr() + ow * oh, 0
        d.pitch[0], d.pitch[1], d.pitch[2] = ow, 2 * ((ow + 1) // 2), 0
        d.frame_stride = t.stride(0)
        dsts.append(d)
        bufs.append(t)
    return dsts, bufs


def _at(d, f0):
    e = D.DevFrames()
    e.data[0], e.data[1], e.data[2] = d.data[0] + f0 * d.frame_stride, d.data[1] + f0 * d.frame_stride, 0
    e.pitch[0], e.pitch[1], e.pitch[2] = d.pitch[0], d.pitch[1], 0
    e.frame_stride = d.frame_stride
    return e


def test_attached_to_a_graph(ctx):
    """384x216 -> 192x108 + 96x54, max_batch 4, 11 frames: run_device (three calls) and run_host
    (three chunks over both slots and streams) also score the source frames; the renditions stay
    bit-exact against the oracle."""
    sw, sh, fmt, n = 384, 216, D.FMT_YUV420P, 11
    outs = [(192, 108, D.FMT_NV12, BIC), (96, 54, D.FMT_NV12, BIC)]
    rng = np.random.default_rng(21)
    b = Batch(sw, sh, fmt, n, rng)
    b.fill(scene_frames(sw, sh, fmt, n, rng, starts=(0, 4, 8))).upload()
    frames = b.frames()
    want = R.run(frames, sw, sh, fmt)
    wantr = [[oracle_frame(fr, sw, sh, fmt, o[0], o[1], o[2], o[3]) for o in outs] for fr in frames]
    g = D.Graph(ctx, D.make_spec(sw, sh, fmt, outs, max_batch=4))
    sd = D.Scdet(ctx, sw, sh, fmt)
    g.set_scdet(sd)
    # device path
    dsts, bufs = _out_bufs(outs, n)
    f0 = 0
    for m in (4, 6, 1):
        g.run_device(b.dev(f0), m, [_at(d, f0) for d in dsts], stream=_stream())
        f0 += m
    assert sd.fetch() == want
    _sync()
    assert b.untouched()
    for f in range(n):
        for k, (ow, oh, _of, _m) in enumerate(outs):
            raw = bufs[k][f].cpu().numpy()
            y = raw[:ow * oh].reshape(oh, ow)
            uv = raw[ow * oh: ow * oh + 2 * ((ow + 1) // 2) * ((oh + 1) // 2)].reshape((oh + 1) // 2, -1)
            assert planes_equal([y, uv, None], wantr[f][k]), first_diff([y, uv, None], wantr[f][k])
    # host path: a new stream
    sd.reset()
    got, _ = g.run_host(frames)
    assert sd.fetch() == want
    for f in range(n):
        for k in range(len(outs)):
            assert planes_equal(got[f][k], wantr[f][k]), first_diff(got[f][k], wantr[f][k])
    # a detached graph scores nothing; the detector outlives the graph's reference
    g.set_scdet(None)
    g.run_host(frames[:2])
    assert sd.fetch() == []
    g.set_scdet(sd)
    g.close()
    sd.run_device(b.dev(0), 2, _stream())
    assert len(sd.fetch()) == 2
    sd.close()


def test_graph_busy_enqueues_nothing(ctx):
    sw, sh, fmt = 64, 36, D.FMT_YUV420P
    outs = [(32, 18, D.FMT_NV12, BIC)]
    rng = np.random.default_rng(22)
    frames = scene_frames(sw, sh, fmt, 5, rng)
    g = D.Graph(ctx, D.make_spec(sw, sh, fmt, outs, max_batch=2))
    sd = D.Scdet(ctx, sw, sh, fmt, max_pending=4)
    g.set_scdet(sd)
    with pytest.raises(D.DtsError) as ei:
        g.run_host(frames)
    assert ei.value.code == D.E_BUSY
    assert sd.fetch() == []
    g.run_host(frames[:4])
    assert sd.fetch() == R.run(frames[:4], sw, sh, fmt)
    g.close()
    sd.close()


def test_hdr_graph_source_scored_at_10_bits(ctx):
    sw, sh, fmt = 384, 216, D.FMT_P010LE
    rng = np.random.default_rng(23)
    frames = scene_frames(sw, sh, fmt, 5, rng, starts=(0, 3))
    g = D.Graph(ctx, D.make_spec(sw, sh, fmt, [(192, 108, D.FMT_YUV420P, BIC)], max_batch=2,
                                 tonemap={"mode": D.TM_HABLE}))
    sd = D.Scdet(ctx, sw, sh, fmt)
    g.set_scdet(sd)
    g.run_host(frames)
    want = R.run(frames, sw, sh, fmt)
    assert sd.fetch() == want
    assert want[3]["cut"] == 1
    g.close()
    sd.close()


def test_graph_refusals(ctx):
    L = D.lib()
    outs = [(32, 18, D.FMT_NV12, BIC)]
    g = D.Graph(ctx, D.make_spec(64, 36, D.FMT_YUV420P, outs))
    gd = D.Graph(ctx, D.make_spec(64, 36, D.FMT_YUV420P, outs, deint=(0, 1)))
    sd = D.Scdet(ctx, 64, 36, D.FMT_YUV420P)
    assert L.dts_graph_set_scdet(gd.h, sd.h) == D.E_UNSUPPORTED
    for (w, h, fmt) in [(66, 36, D.FMT_YUV420P), (64, 38, D.FMT_YUV420P), (64, 36, D.FMT_NV12)]:
        other = D.Scdet(ctx, w, h, fmt)
        assert L.dts_graph_set_scdet(g.h, other.h) == D.E_INVAL
        other.close()
    assert L.dts_graph_set_scdet(g.h, sd.h) == 0
    assert L.dts_graph_set_scdet(g.h, None) == 0
    g.close()
    gd.close()
    sd.close()
