"""bench.py --dump-outputs / --full: what a dump holds (host-side, on CPU tensors) and one
plain run of the benchmark on the GPU whose dump is checked against the oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dtsffi as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _batch(w, h, fmt, n, seed):
    """n random frames of (w, h, fmt) as planes, and the same frames as rows of a 2-D tensor
    laid out the way bench.dev_batch lays them (256-byte pitch, padding = 0xEE)."""
    import bench
    rng = np.random.default_rng(seed)
    t = torch.full((n, bench.frame_bytes(w, h, fmt)), 0xEE, dtype=torch.uint8)
    frames = []
    for f in range(n):
        planes, off = [], 0
        for s in D.plane_shapes(w, h, fmt):
            if s is None:
                continue
            p = rng.integers(0, 256, s, dtype=np.uint8)
            pitch = (s[1] + 255) // 256 * 256
            t[f, off:off + pitch * s[0]].view(s[0], pitch)[:, :s[1]] = torch.from_numpy(p)
            off += pitch * s[0]
            planes.append(p)
        frames.append(np.concatenate([p.ravel() for p in planes]))
    return np.concatenate(frames), t


OUTS = [(70, 38, D.FMT_NV12, 0), (33, 17, D.FMT_YUV420P, 0), (20, 10, D.FMT_P010LE, 0)]


def test_dump_whole_batch(tmp_path):
    """Renditions that fit the budget go out whole: every plane byte of every frame, in frame and
    plane order, the row padding left out; float32; quality records as float64."""
    import bench
    n = 3
    made = [_batch(w, h, fmt, n, 10 + k) for k, (w, h, fmt, _m) in enumerate(OUTS)]
    q = np.zeros((n, 6), np.float64)
    q.view(np.int64)[:, :3] = np.arange(3 * n).reshape(n, 3) * (1 << 33)
    q[:, 3:] = np.arange(3 * n).reshape(n, 3) + 0.25
    qt = torch.from_numpy(q.view(np.uint8).reshape(n, 48).copy())
    bench.dump_outputs(str(tmp_path), {"outs": OUTS}, [t for _, t in made], n, {"quality": qt})
    names = ["out0_70x38_nv12.npy", "out1_33x17_yuv420p.npy", "out2_20x10_p010le.npy"]
    assert sorted(os.listdir(tmp_path)) == sorted(names + ["quality_sse.npy", "quality_ssim_sum.npy"])
    for name, (want, _t) in zip(names, made):
        got = np.load(tmp_path / name)
        assert got.dtype == np.float32 and np.array_equal(got, want.astype(np.float32))
    sse, ssim = np.load(tmp_path / "quality_sse.npy"), np.load(tmp_path / "quality_ssim_sum.npy")
    assert sse.dtype == ssim.dtype == np.float64
    assert np.array_equal(sse, np.arange(3 * n).reshape(n, 3) * float(1 << 33))
    assert np.array_equal(ssim, q[:, 3:])


def test_dump_sample_is_fixed_and_bounded(tmp_path, monkeypatch):
    """Renditions beyond the budget: a sample within the budget, the same elements on every
    run, each one a real pixel (never row padding) of the batch."""
    import bench
    n = 4
    made = [_batch(w, h, fmt, n, 20 + k) for k, (w, h, fmt, _m) in enumerate(OUTS)]
    monkeypatch.setattr(bench, "DUMP_BYTES", 4 * 3 * 500)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"outs": OUTS}, [t for _, t in made], n)
    total = 0
    for k, name in enumerate(sorted(os.listdir(tmp_path / "a"))):
        a, b = np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)
        want = made[k][0]
        assert a.dtype == np.float32 and np.array_equal(a, b)
        sel = bench.sample_index(len(want), 500, bench.DUMP_SEED + k)
        assert len(sel) == len(a) == min(500, len(want)) and np.all(np.diff(sel) >= 0)
        assert np.array_equal(a, want[sel].astype(np.float32))
        total += a.nbytes
    assert total <= bench.DUMP_BYTES
    monkeypatch.undo()
    assert bench.DUMP_BYTES + (1 << 20) <= 64 * 10 ** 6   # the shipped budget + the quality records


@pytest.mark.gpu
def test_plain_bench_run_dumps_last_step(tmp_path):
    """A plain run (no --full) at a two-frame batch: the line has ms_per_step over exactly --steps
    steps and no oracle / CPU-baseline leg; the dump holds the last step's three renditions (the
    two smaller ones whole, the 1080p one as the fixed sample), equal to the oracle's for the
    source frames that step read."""
    import orc
    steps, warm, B, R = 2, 1, 2, 4
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warm),
           "--batch", str(B), "--ring", str(R), "--dump-outputs", str(tmp_path / "dump")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1
    line = lines[0]
    assert line["steps"] == steps and line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(steps * B / (line["ms_per_step"] * steps / 1e3), rel=0.02)
    assert line["unit"] == "frames/s" and line["higher_is_better"] is True and line["dtype"] == "u8"
    assert line["verified_vs_oracle"] is None and "cpu_baseline" not in line
    import bench
    sw, sh, sfmt = bench.WORKLOADS["cfg2"]["src"]
    first = ((warm + steps - 1) * B) % R                      # the last step's place in the ring
    srcs = [D.synth_host(sw, sh, sfmt, 0, 0x5EED, first + j) for j in range(B)]
    for k, (w, h, fmt, m) in enumerate(bench.LADDER):
        got = np.load(tmp_path / "dump" / f"out{k}_{w}x{h}_nv12.npy")
        assert got.dtype == np.float32
        want = np.concatenate([p.ravel() for s in srcs
                               for p in orc.scale_frame(s, sw, sh, sfmt, w, h, fmt, m) if p is not None])
        limit = bench.DUMP_BYTES // 4 // len(bench.LADDER)
        sel = bench.sample_index(len(want), limit, bench.DUMP_SEED + k)
        assert len(sel) == (len(want) if k else limit)        # 1080p is sampled, the others whole
        assert np.array_equal(got, want[sel].astype(np.float32))
