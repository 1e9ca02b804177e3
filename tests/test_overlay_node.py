"""The Node worker's burn-in overlays: codecSettings' "overlay" field (CPU: expression
evaluator, planLadders, the frame-rate refusal, the filtergraph.js message, the scheduler's
calls -- tests/node/test_overlay_settings.js) and, on the GPU, worker.js --dump bit-exact
against the oracle followed by the overlay restatement (tests/_overlay_ref.py)."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import dtsffi as D
import orc
import _overlay_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
pytestmark = pytest.mark.skipif(NODE is None, reason="node is not installed")
WORKER = os.path.join(ROOT, "distributed-transcoding-server_amd", "node", "worker.js")


def test_overlay_settings_cpu():
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "node", "test_overlay_settings.js")], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "overlay settings ok" in r.stdout


def test_addon_exports_overlay_calls_cpu():
    addon = os.path.join(ROOT, "distributed-transcoding-server_amd", "addon", "dts_napi.node")
    r = subprocess.run([NODE, "-e", f"const a=require({json.dumps(addon)});"
                                    "console.log(['createOverlay','graphSetOverlay','graphSetPosition']"
                                    ".every(function(n){return typeof a[n]==='function';}), a.version());"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert r.stdout.startswith("true ") and "abi 8" in r.stdout


def _packed(img):
    return b"".join(np.ascontiguousarray(p).tobytes() for p in img)


@pytest.mark.gpu
def test_worker_gpu_overlay_bitexact(tmp_path):
    """A 2-rung job over 2 segments of 3 frames: a logo for ever on one rung (with an
    expression position), and on the other an item whose range [2, 5) crosses the segment
    boundary, over a logo it overlaps."""
    sw, sh, seg = 384, 216, 3
    rng = np.random.default_rng(21)
    logo, sub = R.random_image(21, 9, rng), R.random_image(40, 10, rng)
    (tmp_path / "logo.yuva").write_bytes(_packed(logo))
    sub_dir = tmp_path / "subs"
    sub_dir.mkdir()
    (sub_dir / "ev1.yuva").write_bytes(_packed(sub))
    ov21 = [{"image": "logo.yuva", "w": 21, "h": 9, "x": "W-w-20", "y": 6, "from": 0, "to": None}]
    ov22 = [{"image": "logo.yuva", "w": 21, "h": 9, "x": 70, "y": "H-h-3"},
            {"image": "subs/ev1.yuva", "w": 40, "h": 10, "x": "(W-w)/2", "y": "H-h-4", "from": 2, "to": 5}]
    jobs = [{"id": 21, "sourceID": 5, "width": 192, "height": 108, "framerate": 60,
             "codecSettings": json.dumps({"overlay": ov21})},
            {"id": 22, "sourceID": 5, "width": 128, "height": 72, "framerate": 60,
             "codecSettings": json.dumps({"scale": "lanczos", "format": "yuv420p", "overlay": ov22})}]
    chunks = []
    for j in jobs:
        for off in range(2):
            chunks.append({"id": len(chunks) + 1, "mainJob": j["id"], "chunkOffset": off, "assignedTo": None,
                           "status": None, "result": None})
    cfg = {"workerId": 3, "segmentFrames": seg, "gpus": [0],
           "sources": {"5": {"w": sw, "h": sh, "fmt": 0, "fps": [60, 1]}}, "jobs": jobs, "chunks": chunks}
    (tmp_path / "job.json").write_text(json.dumps(cfg))
    dump = tmp_path / "out"
    dump.mkdir()
    r = subprocess.run([NODE, WORKER, str(tmp_path / "job.json"), "--dump", str(dump)], capture_output=True, text=True,
                       timeout=120, cwd=str(dump))       # images resolve against the job file's directory, not the cwd
    assert r.returncode == 0, r.stderr
    res = json.loads(r.stdout)
    outs = {21: (192, 108, D.FMT_NV12, D.SCALE_BICUBIC), 22: (128, 72, D.FMT_YUV420P, D.SCALE_LANCZOS)}
    items = {21: ([logo], [(0, 192 - 21 - 20, 6, 0, None)]),
             22: ([logo, sub], [(0, 70, 72 - 9 - 3, 0, None), (1, (128 - 40) // 2, 72 - 10 - 4, 2, 5)])}
    changed = 0
    for c in res["chunks"]:
        assert c["status"] == "done", c
        w, h, fmt, m = outs[c["mainJob"]]
        images, its = items[c["mainJob"]]
        for i in range(seg):
            n = c["chunkOffset"] * seg + i
            src = D.synth_host(sw, sh, D.FMT_YUV420P, 0, 0x5EED, n)
            plain = orc.scale_frame(src, sw, sh, D.FMT_YUV420P, w, h, fmt, m)
            want = R.blend_items([None if p is None else np.array(p) for p in plain], fmt, images, its, n)
            packed = b"".join(np.ascontiguousarray(p).tobytes() for p in want if p is not None)
            got = (dump / f"{c['mainJob']}_{c['chunkOffset']}_{i}.raw").read_bytes()
            assert got == packed, f"job {c['mainJob']} chunk {c['chunkOffset']} frame {i}"
            changed += packed != b"".join(np.ascontiguousarray(p).tobytes() for p in plain if p is not None)
    assert changed == 12          # every frame of both rungs carries a logo
