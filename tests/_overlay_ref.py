"""numpy restatement of the burn-in overlay contract: vf_overlay (FFmpeg 4.4) of a yuva420p
picture on a 4:2:0 8-bit rendition, format=yuv420, straight alpha.  Restated from
vf_overlay.c blend_plane from memory, unverified against an ffmpeg binary (none is at hand);
written from the contract, not from the library's C++.

Pictures are [Y, U, V, A] uint8 arrays (Y, A h x w; U, V ceil(h/2) x ceil(w/2)); frames are
dtsffi plane lists (yuv420p [Y, U, V], nv12 [Y, UV, None]) and are blended in place."""
import numpy as np

import dtsffi as D


# shared by the CPU and the GPU tests: buffer fill outside the planes, the renditions, the
# picture sizes (80x40 goes on the 64x36 rendition only: larger than the frame)
SENTINEL = 0xA5
RENDITIONS = [(64, 36), (130, 74), (37, 23)]
IMAGES = [(16, 8), (17, 9), (1, 1), (2, 2)]


def positions(W, H, w, h):
    """inside, odd, negative (partly off the left and top), overhanging the right and
    bottom, wholly outside"""
    return [(8, 6), (9, 7), (-w // 2 - 1, -h // 2 - 1), (W - w // 2 - 1, H - h // 2 - 1), (W + 2, 4), (4, -h - 2),
            (-6, H - 3)]


def div255(v):
    """round-half-up of v / 255 for 0 <= v <= 65025"""
    return ((np.asarray(v, np.int64) + 128) * 257) >> 16


def chroma_alpha(A):
    """The alpha of every chroma sample: the mean of its 2x2 luma alphas, except in the last
    chroma column and row, which average the horizontal and the vertical pair (each pair only
    when the neighbouring chroma sample exists)."""
    h, w = A.shape
    cw, ch = (w + 1) // 2, (h + 1) // 2
    P = np.zeros((2 * ch + 1, 2 * cw + 1), np.int64)
    P[:h, :w] = A
    a00, a01 = P[0:2 * ch:2, 0:2 * cw:2], P[0:2 * ch:2, 1:2 * cw + 1:2]
    a10, a11 = P[1:2 * ch + 1:2, 0:2 * cw:2], P[1:2 * ch + 1:2, 1:2 * cw + 1:2]
    kin = (np.arange(cw) + 1 < cw)[None, :]
    jin = (np.arange(ch) + 1 < ch)[:, None]
    quad = (a00 + a10 + a01 + a11) >> 2
    ah = np.where(kin, (a00 + a01) >> 1, a00)
    av = np.where(jin, (a00 + a10) >> 1, a00)
    return np.where(kin & jin, quad, (av + ah) >> 1)


def _blend_plane(dst, src, alpha, x, y):
    """dst[y + j, x + i] = div255(dst * (255 - alpha) + src * alpha) over the intersection"""
    H, W = dst.shape
    h, w = src.shape
    x0, y0, x1, y1 = max(x, 0), max(y, 0), min(x + w, W), min(y + h, H)
    if x0 >= x1 or y0 >= y1:
        return
    d = dst[y0:y1, x0:x1].astype(np.int64)
    s = src[y0 - y:y1 - y, x0 - x:x1 - x].astype(np.int64)
    a = np.asarray(alpha)[y0 - y:y1 - y, x0 - x:x1 - x].astype(np.int64)
    dst[y0:y1, x0:x1] = div255(d * (255 - a) + s * a).astype(np.uint8)


def blend(frame, fmt, image, x, y):
    """One picture into one frame, in place."""
    Y, U, V, A = image
    x &= ~1
    y &= ~1
    xp, yp = x >> 1, y >> 1
    _blend_plane(frame[0], Y, A, x, y)
    ca = chroma_alpha(A)
    if fmt == D.FMT_NV12:
        _blend_plane(frame[1][:, 0::2], U, ca, xp, yp)
        _blend_plane(frame[1][:, 1::2], V, ca, xp, yp)
    else:
        _blend_plane(frame[1], U, ca, xp, yp)
        _blend_plane(frame[2], V, ca, xp, yp)
    return frame


def shown(item, n):
    """item = (image, x, y, first, last); last None or < 0 = for ever"""
    last = item[4]
    return item[3] <= n and (last is None or last < 0 or n < last)


def blend_items(frame, fmt, images, items, n):
    """Every item shown on stream frame n, in list order."""
    for it in items:
        if shown(it, n):
            blend(frame, fmt, images[it[0]], it[1], it[2])
    return frame


def random_image(w, h, rng):
    """Random picture whose alpha has runs forced to 0 and to 255."""
    cw, ch = (w + 1) // 2, (h + 1) // 2
    Y = rng.integers(0, 256, (h, w), dtype=np.uint8)
    U = rng.integers(0, 256, (ch, cw), dtype=np.uint8)
    V = rng.integers(0, 256, (ch, cw), dtype=np.uint8)
    A = rng.integers(0, 256, (h, w), dtype=np.uint8)
    flat = A.reshape(-1)
    n = flat.size
    for val in (0, 255):
        for _ in range(3):
            a = int(rng.integers(0, n))
            flat[a:a + int(rng.integers(1, max(2, n // 4)))] = val
    return [Y, U, V, A]
