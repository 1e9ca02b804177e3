#!/usr/bin/env python3
"""scdet_rate.py -- what scene-change detection costs: k_scdet alone, and attached to the cfg2
step (4K yuv420p -> 1080p / 720p / 854x480 nv12, 512 frames per launch, a source ring far
larger than the 256 MB cache).

Three things alternate in one process over the same ring, each step timed with device events
after a warm-up: (a) dts_scdet_run_device on a 512-frame batch (the records' memset, one
k_scdet launch, the copy of the last frame's luma -- algorithmic bytes: the batch's luma once);
(b) the plain cfg2 graph; (c) the same graph with a detector attached.  Prints one JSON line
and writes it to --out: the medians with min / max, the standalone byte rate and its fraction
of the 8 TB/s roof, the time the detector adds to the step, and that time against luma bytes /
the byte rate the plain step achieved in the same run (added_over_at_rate, as overlay_rate.py).

    python tools/scdet_rate.py [--steps 20] [--warmup 3] [--batch 512] [--ring 1024] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "distributed-transcoding-server_amd", "python"))
sys.path.insert(0, ROOT)
import dtsffi as D  # noqa: E402
from bench import LADDER, SRC_H, SRC_W, dev_batch, frame_bytes  # noqa: E402

ROOF = 8e12      # bytes / s, the HBM figure README.md measures against


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--ring", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scdet_rate.json"))
    args = ap.parse_args()
    B = args.batch
    R = max(args.ring // B, 1) * B
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    sptr = stream.cuda_stream
    ctx = D.Context(0)
    spec = D.make_spec(SRC_W, SRC_H, D.FMT_YUV420P, LADDER, max_batch=B)
    plain, withsd = D.Graph(ctx, spec), D.Graph(ctx, spec)
    nrec = (args.steps + args.warmup + 1) * B          # every record of the run fits: no fetch between steps
    sd_graph = D.Scdet(ctx, SRC_W, SRC_H, D.FMT_YUV420P, 10.0, nrec)
    sd_alone = D.Scdet(ctx, SRC_W, SRC_H, D.FMT_YUV420P, 10.0, nrec)
    withsd.set_scdet(sd_graph)

    src = torch.empty((R, frame_bytes(SRC_W, SRC_H, D.FMT_YUV420P)), dtype=torch.uint8, device=dev)
    sd, _ = dev_batch(src, SRC_W, SRC_H, D.FMT_YUV420P)
    ctx.synth_device(SRC_W, SRC_H, D.FMT_YUV420P, 0, 0x5EED, 0, sd, R, sptr)
    ods, outs = [], []
    for (w, h, fmt, _m) in LADDER:
        t = torch.empty((B, frame_bytes(w, h, fmt)), dtype=torch.uint8, device=dev)
        outs.append(t)
        ods.append(dev_batch(t, w, h, fmt)[0])

    def batch(i):
        i0 = (i * B) % R
        d = D.DevFrames()
        for p in range(3):
            d.data[p] = sd.data[p] + i0 * sd.frame_stride
            d.pitch[p] = sd.pitch[p]
        d.frame_stride = sd.frame_stride
        return d

    runs = (("plain", lambda i: plain.run_device(batch(i), B, ods, stream=sptr)),
            ("scdet", lambda i: withsd.run_device(batch(i), B, ods, stream=sptr)),
            ("alone", lambda i: sd_alone.run_device(batch(i), B, sptr)))
    for i in range(args.warmup):
        for j, (_n, f) in enumerate(runs):
            f(3 * i + j)
    torch.cuda.synchronize(dev)
    evs = {n: [] for n, _f in runs}
    with torch.cuda.stream(stream):
        for s in range(args.steps):
            for j, (name, f) in enumerate(runs):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                f(3 * (args.warmup + s) + j)
                b.record(stream)
                evs[name].append((a, b))
    torch.cuda.synchronize(dev)
    nfetched = len(sd_graph.fetch()), len(sd_alone.fetch())
    ms = {n: sorted(a.elapsed_time(b) for a, b in v) for n, v in evs.items()}
    med = {n: v[len(v) // 2] for n, v in ms.items()}
    luma = SRC_W * SRC_H * B
    algo = plain.info.algo_bytes_per_frame * B
    rate = algo / (med["plain"] * 1e-3)
    alone_rate = luma / (med["alone"] * 1e-3)
    added = med["scdet"] - med["plain"]
    at_rate = luma / rate * 1e3
    mm = lambda n: [round(ms[n][0], 4), round(ms[n][-1], 4)]
    line = json.dumps({
        "tool": "scdet_rate", "workload": "k_scdet alone on 4K yuv420p luma; cfg2 with and without an attached detector",
        "batch": B, "ring": R, "steps": args.steps, "records_fetched": list(nfetched),
        "alone_ms": round(med["alone"], 4), "alone_ms_min_max": mm("alone"),
        "luma_bytes": int(luma), "alone_bytes_per_s": round(alone_rate, 1), "alone_roof_fraction": round(alone_rate / ROOF, 4),
        "step_ms_plain": round(med["plain"], 4), "step_ms_scdet": round(med["scdet"], 4),
        "step_ms_plain_min_max": mm("plain"), "step_ms_scdet_min_max": mm("scdet"),
        "fps_plain": round(B / med["plain"] * 1e3, 1), "fps_scdet": round(B / med["scdet"] * 1e3, 1),
        "ladder_algo_bytes": int(algo), "ladder_bytes_per_s": round(rate, 1),
        "added_ms": round(added, 4), "added_share_of_step": round(added / med["plain"], 4),
        "luma_share_of_ladder_bytes": round(luma / algo, 4),
        "scdet_ms_at_ladder_rate": round(at_rate, 4),
        "added_over_at_rate": round(added / at_rate, 3) if at_rate > 0 else None,
    })
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    for g in (plain, withsd):
        g.close()
    for d in (sd_graph, sd_alone):
        d.close()
    ctx.close()


if __name__ == "__main__":
    main()
