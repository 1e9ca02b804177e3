"""numpy restatement of the scene-change contract (vf_scdet of FFmpeg 4.4 on plane 0 of a YUV
input), written from the contract and not from the library's code: the reference of
tests/test_scdet_host.py, tests/test_gpu_scdet.py and tests/test_scene_node.py.

Per stream: prev (the previous frame's luma) and prev_mafd (0 at the start).  Per frame, with
no prev: everything 0 and has_prev 0.  Otherwise sad = sum |cur - prev| (exact, int64), mafd =
sad * 100 / count / 2^bitdepth in that order in doubles, diff = |mafd - prev_mafd|, score =
clip(float32(min(mafd, diff)), 0, 100) as a double, prev_mafd = mafd, cut = score >= threshold.
Samples: the luma bytes at 8 bits (yuv420p / nv12), the little-endian luma word >> 6 at 10 bits
(p010le)."""
import numpy as np

FMT_P010LE = 2


def luma(frame, w, h, fmt):
    """The w x h luma samples of a frame (plane list of uint8 arrays) as int64."""
    y = np.asarray(frame[0])
    if fmt == FMT_P010LE:
        y = y[:h, :2 * w].astype(np.int64)
        return (y[:, 0::2] | (y[:, 1::2] << 8)) >> 6
    return y[:h, :w].astype(np.int64)


class Detector:
    def __init__(self, w, h, fmt, threshold=10.0):
        self.w, self.h, self.fmt, self.threshold = w, h, fmt, float(threshold)
        self.bitdepth = 10 if fmt == FMT_P010LE else 8
        self.reset()

    def reset(self):
        self.prev = None
        self.prev_mafd = 0.0

    def push(self, frame):
        cur = luma(frame, self.w, self.h, self.fmt)
        if self.prev is None:
            self.prev = cur
            return {"sad": 0, "mafd": self.prev_mafd, "score": 0.0, "cut": 0, "has_prev": 0}
        sad = int(np.abs(cur - self.prev).sum(dtype=np.int64))
        count = self.w * self.h
        mafd = float(sad) * 100.0 / float(count) / float(1 << self.bitdepth)
        diff = abs(mafd - self.prev_mafd)
        c = np.float32(min(mafd, diff))
        c = np.float32(0.0) if c < 0 else (np.float32(100.0) if c > 100 else c)
        score = float(c)
        self.prev_mafd = mafd
        self.prev = cur
        return {"sad": sad, "mafd": mafd, "score": score, "cut": int(score >= self.threshold), "has_prev": 1}


def run(frames, w, h, fmt, threshold=10.0):
    d = Detector(w, h, fmt, threshold)
    return [d.push(f) for f in frames]
