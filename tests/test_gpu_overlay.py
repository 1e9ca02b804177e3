"""GPU: burn-in overlays (k_overlay) bit-exact against the numpy restatement of the contract
(tests/_overlay_ref.py).  Device buffers are pre-filled with a sentinel and compared whole:
every byte outside the expected rectangles, pitch padding included, must keep its value."""
import numpy as np
import pytest

import dtsffi as D
import orc
import _overlay_ref as R
from _util import first_diff, planes_equal, random_frame
from _overlay_ref import IMAGES, RENDITIONS, SENTINEL, positions

pytestmark = pytest.mark.gpu

BIC = D.SCALE_BICUBIC


class Batch:
    """n frames of (w, h, fmt) in one sentinel-filled buffer, host mirror `host` [n, fb].
    Pitches are the row bytes + 1 rounded up to 16, plus `skew` (4: pitches that are no
    multiple of 8, the kernel's 4-byte path; 0: its 8-byte path), plus `extra[p]` for plane p
    alone (U and V planes of different pitches); planes 16-byte aligned."""

    def __init__(self, w, h, fmt, n, skew=0, extra=(0, 0, 0)):
        self.w, self.h, self.fmt, self.n = w, h, fmt, n
        self.shapes = D.plane_shapes(w, h, fmt)
        self.pitch, self.off = [], []
        o = 0
        for pl, s in enumerate(self.shapes):
            if s is None:
                self.pitch.append(0)
                self.off.append(0)
                continue
            p = (s[1] + 1 + 15) // 16 * 16 + skew + extra[pl]
            self.pitch.append(p)
            self.off.append(o)
            o += (p * s[0] + 15) // 16 * 16
        self.fb = o + 16
        self.host = np.full((n, self.fb), SENTINEL, np.uint8)
        self.t = None

    def planes(self, host, f):
        """Views of frame f's planes in a mirror array."""
        return [None if s is None else
                host[f, o:o + p * s[0]].reshape(s[0], p)[:, :s[1]]
                for s, p, o in zip(self.shapes, self.pitch, self.off)]

    def fill(self, frames):
        for f, fr in enumerate(frames):
            for v, p in zip(self.planes(self.host, f), fr):
                if v is not None:
                    v[...] = p
        return self

    def upload(self):
        import torch
        self.t = torch.from_numpy(self.host).cuda()
        return self

    def dev(self):
        d = D.DevFrames()
        for p, s in enumerate(self.shapes):
            d.data[p] = None if s is None else self.t.data_ptr() + self.off[p]
            d.pitch[p] = self.pitch[p]
        d.frame_stride = self.fb
        return d

    def download(self):
        return self.t.cpu().numpy()


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _sync():
    import torch
    torch.cuda.synchronize()


@pytest.mark.parametrize("skew", [0, 4])
@pytest.mark.parametrize("fmt", [D.FMT_YUV420P, D.FMT_NV12])
@pytest.mark.parametrize("W,H", RENDITIONS)
def test_run_device_vs_reference(ctx, W, H, fmt, skew):
    """dts_overlay_run_device: 5 frames from stream frame 7; one item for ever (every image
    size at every position), one over [8, 10), and two that overlap in space and time (list
    order must hold)."""
    rng = np.random.default_rng(W * 5 + H + fmt * 2 + skew)
    n, first = 5, 7
    frames = [random_frame(W, H, fmt, rng) for _ in range(n)]
    base = Batch(W, H, fmt, n, skew).fill(frames)
    sub = R.random_image(24, 6, rng)
    o1, o2 = R.random_image(10, 10, rng), R.random_image(9, 7, rng)
    sizes = IMAGES + ([(80, 40)] if (W, H) == (64, 36) else [])
    if (W, H) == (130, 74):
        sizes = sizes + [(121, 71)]          # more than one workgroup per frame
    for (w, h) in sizes:
        img = R.random_image(w, h, rng)
        images = [img, sub, o1, o2]
        for (x, y) in positions(W, H, w, h) + [(10, 6), (12, 2)]:
            items = [(0, x, y, 0, None), (1, 6, H - 10, 8, 10), (2, 20, 10, 7, 9), (3, 25, 13, 8, -1)]
            want = base.host.copy()
            for f in range(n):
                R.blend_items(base.planes(want, f), fmt, images, items, first + f)
            ov = D.Overlay(ctx, images, items)
            b = base.upload()
            ctx.overlay_device(ov, W, H, fmt, b.dev(), n, first, _stream())
            _sync()
            got = b.download()
            ov.close()
            assert np.array_equal(got, want), \
                f"image {w}x{h} at ({x},{y}): {int((got != want).sum())} bytes differ, first at " \
                f"{np.argwhere(got != want)[0]}"


@pytest.mark.parametrize("extra", [(0, 32, 0), (0, 0, 32), (0, 4, 16)])
@pytest.mark.parametrize("skew", [0, 4])
@pytest.mark.parametrize("W,H", [(130, 74), (37, 23)])
def test_run_device_u_and_v_pitches_differ(ctx, W, H, skew, extra):
    """yuv420p batches whose U and V planes have different pitches (the API takes each
    plane's own): every plane by its own pitch, on the 8-byte and the 4-byte path.  With
    the U pitch the larger, a V row addressed by it would land past the V plane."""
    fmt = D.FMT_YUV420P
    rng = np.random.default_rng(W + extra[1] + 3 * extra[2])
    n, first = 3, 0
    base = Batch(W, H, fmt, n, skew, extra).fill([random_frame(W, H, fmt, rng) for _ in range(n)])
    assert base.pitch[1] != base.pitch[2]
    images = [R.random_image(21, 11, rng), R.random_image(W, 6, rng)]
    items = [(0, W - 30, 4, 0, None), (1, 0, H - 8, 1, 2), (0, -6, H - 5, 0, None)]
    want = base.host.copy()
    for f in range(n):
        R.blend_items(base.planes(want, f), fmt, images, items, first + f)
    ov = D.Overlay(ctx, images, items)
    b = base.upload()
    ctx.overlay_device(ov, W, H, fmt, b.dev(), n, first, _stream())
    _sync()
    got = b.download()
    ov.close()
    assert np.array_equal(got, want), f"{int((got != want).sum())} bytes differ, first at {np.argwhere(got != want)[0]}"


def test_run_device_nothing_shown_and_validation(ctx):
    rng = np.random.default_rng(3)
    W, H = 64, 36
    img = R.random_image(16, 8, rng)
    b = Batch(W, H, D.FMT_NV12, 3).fill([random_frame(W, H, D.FMT_NV12, rng) for _ in range(3)]).upload()
    ov = D.Overlay(ctx, [img], [(0, 4, 4, 10, 12), (0, 200, 4, 0, None)])
    ctx.overlay_device(ov, W, H, D.FMT_NV12, b.dev(), 3, 0, _stream())        # before the range / outside
    ctx.overlay_device(ov, W, H, D.FMT_NV12, b.dev(), 3, 12, _stream())       # after the range
    _sync()
    assert np.array_equal(b.download(), b.host)
    with pytest.raises(D.DtsError) as e:
        ctx.overlay_device(ov, W, H, D.FMT_P010LE, b.dev(), 3, 0)
    assert e.value.code == D.E_UNSUPPORTED
    ov.close()
    for bad in ([(1, 0, 0, 0, None)], [(-1, 0, 0, 0, None)], [(0, 0, 0, -1, None)]):   # image index, first
        with pytest.raises(D.DtsError) as e:
            D.Overlay(ctx, [img], bad)
        assert e.value.code == D.E_INVAL
    with pytest.raises(D.DtsError) as e:
        D.Overlay(ctx, [img], [(0, 0, 0, 0, None)] * 257)
    assert e.value.code == D.E_INVAL
    with pytest.raises(D.DtsError) as e:
        D.Overlay(ctx, [img] * 65, [])
    assert e.value.code == D.E_INVAL


def _src_batch(frames, w, h, fmt):
    """Source frames on the device in bench.dev_batch's layout (16-byte aligned planes)."""
    import torch
    from bench import dev_batch, frame_bytes
    fb = frame_bytes(w, h, fmt)
    host = np.zeros((len(frames), fb), np.uint8)
    t = torch.zeros((len(frames), fb), dtype=torch.uint8, device="cuda")
    d, _ = dev_batch(t, w, h, fmt)
    for i, f in enumerate(frames):
        for p, pl in enumerate(f):
            if pl is None:
                continue
            off = d.data[p] - t.data_ptr()
            rows, cols = pl.shape
            host[i, off:off + rows * d.pitch[p]].reshape(rows, d.pitch[p])[:, :cols] = pl
    t.copy_(torch.from_numpy(host))
    return t, d


OUTS = [(192, 108, D.FMT_NV12, BIC), (128, 72, D.FMT_YUV420P, BIC)]


def test_graph_device_path_position_advances(ctx):
    """Two dts_graph_run_device calls of 3 frames, an item over [2, 5) on output 0 only: the
    stream position advances across the calls; output 1 is the plain oracle."""
    sw, sh = 384, 216
    rng = np.random.default_rng(11)
    frames = [random_frame(sw, sh, D.FMT_YUV420P, rng) for _ in range(6)]
    images = [R.random_image(40, 16, rng), R.random_image(21, 11, rng)]
    items = [(0, 140, 80, 2, 5), (1, 150, 84, 0, None)]
    g = D.Graph(ctx, D.make_spec(sw, sh, D.FMT_YUV420P, OUTS))
    ov = D.Overlay(ctx, images, items)
    g.set_overlay(0, ov)
    for call in range(2):
        st, sd = _src_batch(frames[3 * call:3 * call + 3], sw, sh, D.FMT_YUV420P)
        outs = [Batch(o[0], o[1], o[2], 3).upload() for o in OUTS]
        g.run_device(sd, 3, [b.dev() for b in outs], stream=_stream())
        _sync()
        for k, (w, h, fmt, m) in enumerate(OUTS):
            want = outs[k].host.copy()
            for f in range(3):
                fr = orc.scale_frame(frames[3 * call + f], sw, sh, D.FMT_YUV420P, w, h, fmt, m)
                if k == 0:
                    R.blend_items(fr, fmt, images, items, 3 * call + f)
                for v, p in zip(outs[k].planes(want, f), fr):
                    if v is not None:
                        v[...] = p
            got = outs[k].download()
            assert np.array_equal(got, want), f"call {call} output {k}: {int((got != want).sum())} bytes differ"
    g.close()
    ov.close()


def test_graph_host_path_chunks(ctx):
    """max_batch = 2, 5 frames through dts_graph_submit, an item over [1, 4): the chunk
    boundaries fall inside the range; then a second submit continues at position 5, and
    dts_graph_set_position rewinds."""
    sw, sh = 384, 216
    rng = np.random.default_rng(12)
    frames = [random_frame(sw, sh, D.FMT_YUV420P, rng) for _ in range(5)]
    images = [R.random_image(33, 15, rng)]
    items = [(0, 101, 51, 1, 4), (0, -10, -4, 6, 7)]
    g = D.Graph(ctx, D.make_spec(sw, sh, D.FMT_YUV420P, OUTS, max_batch=2))
    ov = D.Overlay(ctx, images, items)
    g.set_overlay(0, ov)
    plain = [[orc.scale_frame(fr, sw, sh, D.FMT_YUV420P, w, h, fmt, m) for (w, h, fmt, m) in OUTS] for fr in frames]

    def check(got, pos0, nfr):
        for f in range(nfr):
            want0 = R.blend_items([None if p is None else p.copy() for p in plain[f][0]], OUTS[0][2], images, items,
                                  pos0 + f)
            assert planes_equal(got[f][0], want0), (pos0, f, first_diff(got[f][0], want0))
            assert planes_equal(got[f][1], plain[f][1]), (pos0, f)

    got, _ = g.run_host(frames)
    check(got, 0, 5)
    got, _ = g.run_host(frames[:3])          # positions 5, 6, 7: the second item on frame 6
    check(got, 5, 3)
    g.set_position(1)
    got, _ = g.run_host(frames[:2])
    check(got, 1, 2)
    g.close()
    ov.close()


def test_graph_deinterlace(ctx):
    """Deinterlace graph, max_batch = 2, 5 frames, an item over [2, 4): the same graph's
    output without overlay, blended by the reference."""
    w, h = 64, 36
    rng = np.random.default_rng(13)
    seq = [random_frame(w, h, D.FMT_YUV420P, rng) for _ in range(7)]
    outs = [(64, 36, D.FMT_NV12, BIC), (32, 18, D.FMT_YUV420P, BIC)]
    images = [R.random_image(17, 9, rng)]
    items = [(0, 9, 5, 2, 4)]
    g = D.Graph(ctx, D.make_spec(w, h, D.FMT_YUV420P, outs, max_batch=2, deint=(0, 1)))
    plain, _ = g.run_host(seq)
    ov = D.Overlay(ctx, images, items)
    g.set_overlay(0, ov)
    g.set_overlay(1, ov)
    g.set_position(0)
    got, _ = g.run_host(seq)
    assert len(got) == 5
    for f in range(5):
        for k in range(2):
            want = R.blend_items([None if p is None else p.copy() for p in plain[f][k]], outs[k][2], images, items, f)
            assert planes_equal(got[f][k], want), (f, k, first_diff(got[f][k], want))
    g.close()
    ov.close()


def test_graph_hdr(ctx):
    """HDR10 -> SDR graph (the tests/golden/hdr_hable_64x36 geometry): the overlay output equals
    the no-overlay GPU output blended by the reference, exactly (the float stage's +-1 does
    not enter)."""
    rng = np.random.default_rng(14)
    frames = [D.synth_host(64, 36, D.FMT_P010LE, 0, 0x5EED, f) for f in range(3)]
    outs = [(64, 36, D.FMT_YUV420P, BIC)]
    images = [R.random_image(16, 8, rng), R.random_image(2, 2, rng)]
    items = [(0, 50, 30, 0, None), (1, 3, 3, 1, 2)]
    g = D.Graph(ctx, D.make_spec(64, 36, D.FMT_P010LE, outs, max_batch=2, tonemap={"mode": D.TM_HABLE, "desat": 0.0}))
    plain, _ = g.run_host(frames)
    ov = D.Overlay(ctx, images, items)
    g.set_overlay(0, ov)
    g.set_position(0)
    got, _ = g.run_host(frames)
    for f in range(3):
        want = R.blend_items([p.copy() for p in plain[f][0]], D.FMT_YUV420P, images, items, f)
        assert planes_equal(got[f][0], want), (f, first_diff(got[f][0], want))
    g.close()
    ov.close()


def test_refusals_and_detach(ctx):
    rng = np.random.default_rng(15)
    sw, sh = 384, 216
    img = R.random_image(16, 8, rng)
    ov = D.Overlay(ctx, [img], [(0, 8, 8, 0, None)])
    # p010 rendition
    g = D.Graph(ctx, D.make_spec(sw, sh, D.FMT_YUV420P, [(192, 108, D.FMT_P010LE, BIC), (128, 72, D.FMT_NV12, BIC)]))
    with pytest.raises(D.DtsError) as e:
        g.set_overlay(0, ov)
    assert e.value.code == D.E_UNSUPPORTED
    g.set_overlay(1, ov)                     # its 8-bit rendition takes one
    for bad in (-1, 2, 4):
        with pytest.raises(D.DtsError) as e:
            g.set_overlay(bad, ov)
        assert e.value.code == D.E_INVAL
    other = D.Context(0)                     # an overlay made on another ctx
    ov2 = D.Overlay(other, [img], [(0, 8, 8, 0, None)])
    with pytest.raises(D.DtsError) as e:
        g.set_overlay(1, ov2)
    assert e.value.code == D.E_INVAL
    ov2.close()
    other.close()
    g.close()
    # quality graphs, either kind
    g = D.Graph(ctx, D.make_spec(sw, sh, D.FMT_YUV420P, OUTS, quality=D.Q_BOTH, quality_out=0))
    with pytest.raises(D.DtsError) as e:
        g.set_overlay(1, ov)
    assert e.value.code == D.E_UNSUPPORTED
    g.close()
    g = D.Graph(ctx, D.make_spec(sw, sh, D.FMT_YUV420P,
                                 [(192, 108, D.FMT_NV12, BIC, None, (D.Q_PSNR, D.SCALE_LANCZOS)), OUTS[1]]))
    with pytest.raises(D.DtsError) as e:
        g.set_overlay(1, ov)
    assert e.value.code == D.E_UNSUPPORTED
    g.close()
    # detaching restores the plain output; the overlay may be closed while attached
    frames = [random_frame(sw, sh, D.FMT_YUV420P, rng)]
    g = D.Graph(ctx, D.make_spec(sw, sh, D.FMT_YUV420P, OUTS))
    plain = [orc.scale_frame(frames[0], sw, sh, D.FMT_YUV420P, w, h, fmt, m) for (w, h, fmt, m) in OUTS]
    g.set_overlay(0, ov)
    ov.close()
    got, _ = g.run_host(frames)
    want = R.blend([p if p is None else p.copy() for p in plain[0]], OUTS[0][2], img, 8, 8)
    assert planes_equal(got[0][0], want) and not planes_equal(got[0][0], plain[0])
    g.set_overlay(0, None)
    got, _ = g.run_host(frames)
    assert planes_equal(got[0][0], plain[0]) and planes_equal(got[0][1], plain[1])
    g.close()
