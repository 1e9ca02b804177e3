#!/usr/bin/env python3
"""overlay_rate.py -- what burn-in overlays add to the cfg2 step (4K yuv420p -> 1080p / 720p /
854x480 nv12, 512 frames per launch, a source ring far larger than the 256 MB cache).

Two graphs of the same spec run in one process over the same ring and output batches: one
plain, one with an overlay on every rung -- a logo a tenth of the rung's width on all frames
and a full-width subtitle strip a ninth of its height on half the frames (8 events of 32
frames per 512-frame step).  After warm-up the two alternate, each step timed with device
events.  Prints one JSON line: both step times, the overlay's algorithmic bytes (target
rectangles read + written, images read once), the added time, and that time against
overlay bytes / the byte rate the plain step achieved in the same run.

    python tools/overlay_rate.py [--steps 20] [--warmup 3] [--batch 512] [--ring 1024]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "distributed-transcoding-server_amd", "python"))
sys.path.insert(0, ROOT)
import dtsffi as D  # noqa: E402
from bench import LADDER, SRC_H, SRC_W, dev_batch, frame_bytes  # noqa: E402


def image(w, h, rng):
    cw, ch = (w + 1) // 2, (h + 1) // 2
    return [rng.integers(16, 236, (h, w), dtype=np.uint8), rng.integers(16, 241, (ch, cw), dtype=np.uint8),
            rng.integers(16, 241, (ch, cw), dtype=np.uint8), rng.integers(0, 256, (h, w), dtype=np.uint8)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--ring", type=int, default=1024)
    args = ap.parse_args()
    B = args.batch
    R = max(args.ring // B, 1) * B
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    sptr = stream.cuda_stream
    ctx = D.Context(0)
    spec = D.make_spec(SRC_W, SRC_H, D.FMT_YUV420P, LADDER, max_batch=B)
    plain, withov = D.Graph(ctx, spec), D.Graph(ctx, spec)
    rng = np.random.default_rng(1)
    ov_bytes, keep = 0, []
    for k, (w, h, _fmt, _m) in enumerate(LADDER):
        lw = (w // 10) & ~1
        lh = max(2, (lw * 2 // 5) & ~1)
        sh = (h // 9) & ~1
        images = [image(lw, lh, rng), image(w, sh, rng)]
        items = [(0, w - lw - 20, 20, 0, None)]
        shown = 0
        for e in range(0, B, 64):
            n = min(32, B - e)
            items.append((1, 0, h - sh - 8, e, e + n))
            shown += n
        ov = D.Overlay(ctx, images, items)
        withov.set_overlay(k, ov)
        keep.append(ov)
        # target rectangles read + written (luma + 4:2:0 chroma = 1.5 bytes per pixel, each way);
        # images (Y, A, U, V = 2.5 bytes per pixel) read once per step
        ov_bytes += 3 * lw * lh * B + 3 * w * sh * shown + (5 * lw * lh + 5 * w * sh) // 2

    src = torch.empty((R, frame_bytes(SRC_W, SRC_H, D.FMT_YUV420P)), dtype=torch.uint8, device=dev)
    sd, _ = dev_batch(src, SRC_W, SRC_H, D.FMT_YUV420P)
    ctx.synth_device(SRC_W, SRC_H, D.FMT_YUV420P, 0, 0x5EED, 0, sd, R, sptr)
    ods, outs = [], []
    for (w, h, fmt, _m) in LADDER:
        t = torch.empty((B, frame_bytes(w, h, fmt)), dtype=torch.uint8, device=dev)
        outs.append(t)
        ods.append(dev_batch(t, w, h, fmt)[0])

    def step(g, i):
        i0 = (i * B) % R
        d = D.DevFrames()
        for p in range(3):
            d.data[p] = sd.data[p] + i0 * sd.frame_stride
            d.pitch[p] = sd.pitch[p]
        d.frame_stride = sd.frame_stride
        g.set_position(0)
        g.run_device(d, B, ods, stream=sptr)

    for i in range(args.warmup):
        step(plain, 2 * i)
        step(withov, 2 * i + 1)
    torch.cuda.synchronize(dev)
    evs = {"plain": [], "overlay": []}
    with torch.cuda.stream(stream):
        for s in range(args.steps):
            for j, (name, g) in enumerate((("plain", plain), ("overlay", withov))):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                step(g, 2 * (args.warmup + s) + j)
                b.record(stream)
                evs[name].append((a, b))
    torch.cuda.synchronize(dev)
    ms = {n: sorted(a.elapsed_time(b) for a, b in v) for n, v in evs.items()}
    med = {n: v[len(v) // 2] for n, v in ms.items()}
    algo = plain.info.algo_bytes_per_frame * B
    rate = algo / (med["plain"] * 1e-3)
    added = med["overlay"] - med["plain"]
    at_rate = ov_bytes / rate * 1e3
    print(json.dumps({
        "tool": "overlay_rate", "workload": "cfg2 + logo (w/10, all frames) + subtitle strip (h/9, half the frames) "
                                            "on every rung",
        "batch": B, "ring": R, "steps": args.steps,
        "step_ms_plain": round(med["plain"], 4), "step_ms_overlay": round(med["overlay"], 4),
        "step_ms_plain_min_max": [round(ms["plain"][0], 4), round(ms["plain"][-1], 4)],
        "step_ms_overlay_min_max": [round(ms["overlay"][0], 4), round(ms["overlay"][-1], 4)],
        "fps_plain": round(B / med["plain"] * 1e3, 1), "fps_overlay": round(B / med["overlay"] * 1e3, 1),
        "ladder_algo_bytes": int(algo), "ladder_bytes_per_s": round(rate, 1),
        "overlay_algo_bytes": int(ov_bytes), "added_ms": round(added, 4),
        "overlay_ms_at_ladder_rate": round(at_rate, 4),
        "added_over_at_rate": round(added / at_rate, 3) if at_rate > 0 else None,
    }), flush=True)
    for g in (plain, withov):
        g.close()
    for ov in keep:
        ov.close()
    ctx.close()


if __name__ == "__main__":
    main()
