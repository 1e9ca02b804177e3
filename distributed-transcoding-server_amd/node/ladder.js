"use strict";
// ladder.js -- Jobs rows -> one libdts graph spec per source (SURVEY.md §8b/§8f).
//
// In the reference a rendition is one `job_list` row (database.js:61-94:
// width, height, framerate, bitrate, codec, codecSettings, chunks) that points
// at its source (`sourceID`, database.js:66-72).  A CPU worker would run one
// ffmpeg per row and segment; the GPU worker groups the rows that share a
// source into ONE graph with an output per row -- the `split=N` ladder -- so
// the source segment is read from HBM once for all renditions.
//
// Node 12 (this image): no `??` / `?.`.

const filtergraph = require("./filtergraph");

const FMT = { yuv420p: 0, nv12: 1, p010le: 2, p010: 2 };
// libswscale SWS_* flag values (swscale.h), as include/dts.h DTS_SCALE_*
const METHOD = { bilinear: 0x2, bicubic: 0x4, x: 0x8, point: 0x10, neighbor: 0x10, area: 0x20, gauss: 0x80,
                 sinc: 0x100, lanczos: 0x200 };
// vf_tonemap.c enum TonemapAlgorithm (include/dts.h DTS_TM_*)
const TONEMAP = { none: 0, linear: 1, gamma: 2, clip: 3, reinhard: 4, hable: 5, mobius: 6 };
const MAX_OUTPUTS = 4;

// Jobs.codecSettings is free text in the reference (database.js:78).  The GPU
// worker reads an optional JSON object from it with the filtergraph knobs a CPU
// worker would put on its ffmpeg command line:
//   {"scale": "bicubic", "format": "nv12", "param": [b, c], "tonemap": {"mode": "hable", ...},
//    "quality": "psnr" | "ssim" | "both", "qualityRef": "lanczos",
//    "deinterlace": "yadif" | {"mode": 0 | 2, "parity": "tff" | "bff"},
//    "inRange": "tv" | "pc", "outRange": "tv" | "pc",
//    "overlay": [{"image": file, "w", "h", "x", "y", "from", "to"}, ...],   (overlayOf below)
//    "sceneDetect": true | {"threshold": T}}                                (sceneOf below)
// inRange / outRange: `scale=in_range=R:out_range=R` (libswscale range conversion on
// the horizontally scaled lines; dts_graph_spec.range).
// deinterlace: `yadif=MODE:PARITY` ahead of the scale (frame-rate modes; vf_yadif.c),
// run on the GPU in the same graph (dts_graph_spec.deint).
// quality: `[rendition][reference]psnr` / `ssim` per segment against a reference
// rendition of the same size -- the source scaled with `qualityRef` (default
// lanczos) -- reported in JobChunks.result.quality.
// Or (round 6) the ffmpeg arguments / filtergraph a CPU worker would run with -- e.g.
//   -vf scale=1920:1080:flags=bicubic+accurate_rnd+bitexact,format=nv12 -preset fast
// -- read by filtergraph.js into the same object (its scale size and fps, when given, must agree
// with the row's width / height / framerate).
function parseSettings(text) {
    if (!text) return {};
    let o = null;
    try {
        o = JSON.parse(text);
    } catch (e) {
        const g = filtergraph.graphOfArgs(text);
        if (g === null) return {};        // plain encoder options: nothing for the filtergraph
        const r = filtergraph.parseFiltergraph(g);
        const st = r.settings;
        if (r.size) st._size = r.size;
        if (r.fps) st._fps = r.fps;
        return st;
    }
    return o && typeof o === "object" ? o : {};
}

function outputOf(job) {
    const s = parseSettings(job.codecSettings);
    const method = METHOD[String(s.scale || "bicubic").toLowerCase()];
    if (method === undefined) throw new Error("job " + job.id + ": unknown scale method " + s.scale);
    const fmt = FMT[String(s.format || "nv12").toLowerCase()];
    if (fmt === undefined) throw new Error("job " + job.id + ": unknown output format " + s.format);
    const o = { w: job.width | 0, h: job.height | 0, fmt: fmt, method: method };
    if (s._size && (s._size[0] !== o.w || s._size[1] !== o.h))
        throw new Error("job " + job.id + ": the graph scales to " + s._size.join("x") + ", the row asks " + o.w + "x" + o.h);
    if (s._fps && job.framerate && Math.abs(s._fps - job.framerate) > 1e-3 * job.framerate)
        throw new Error("job " + job.id + ": the graph's fps=" + s._fps + " is not the row's framerate " + job.framerate);
    if (Array.isArray(s.param)) o.param = s.param.slice(0, 2);
    return o;
}

// vf_overlay's x= / y= expressions, the subset a logo or subtitle position needs: integers,
// the variables W H w h main_w main_h overlay_w overlay_h, + - * / (unary too) and
// parentheses, evaluated in doubles and truncated toward zero as vf_overlay does.
// Anything else throws.
function overlayExpr(text, vars) {
    if (typeof text === "number") {
        if (!Number.isInteger(text)) throw new Error("overlay position " + text + " is not an integer");
        return text;
    }
    const src = String(text);
    const tok = src.match(/\s*([A-Za-z_][A-Za-z_0-9]*|\d+|[-+*/()])/gy);
    if (!tok || tok.join("").length !== src.replace(/\s+$/, "").length || !tok.length)
        throw new Error("overlay expression '" + src + "': unsupported syntax");
    const t = tok.map(function (s) { return s.trim(); });
    let pos = 0;
    function bad(what) { throw new Error("overlay expression '" + src + "': " + what); }
    function primary() {
        const s = t[pos++];
        if (s === undefined) bad("ends early");
        if (s === "(") {
            const v = sum();
            if (t[pos++] !== ")") bad("missing )");
            return v;
        }
        if (s === "-") return -primary();
        if (s === "+") return primary();
        if (/^\d+$/.test(s)) return Number(s);
        if (/^[A-Za-z_]/.test(s)) {
            if (!Object.prototype.hasOwnProperty.call(vars, s)) bad("unknown name " + s);
            return vars[s];
        }
        return bad("unexpected " + s);
    }
    function product() {
        let v = primary();
        while (t[pos] === "*" || t[pos] === "/") v = t[pos++] === "*" ? v * primary() : v / primary();
        return v;
    }
    function sum() {
        let v = product();
        while (t[pos] === "+" || t[pos] === "-") v = t[pos++] === "+" ? v + product() : v - product();
        return v;
    }
    const v = sum();
    if (pos !== t.length) bad("unexpected " + t[pos]);
    if (!isFinite(v) || Math.abs(v) > 0x3fffffff) bad("value " + v + " out of range");
    return Math.trunc(v);
}

// codecSettings.overlay: burn-in overlays of this rendition (vf_overlay of pre-rendered
// yuva420p bitmaps: a watermark, bitmap subtitle events), in list order:
//   [{"image": "logo1080.yuva", "w": 200, "h": 80, "x": "W-w-20", "y": 20, "from": 0, "to": null}, ...]
// image: a file of the packed Y, U, V, A planes (w*h, 2 x ceil(w/2)*ceil(h/2), w*h bytes),
// resolved against the job file's directory; x / y: integers or expressions (overlayExpr);
// shown on stream frames from <= n < to (to null = for ever).
// -> [{image, w, h, x, y, first, last}] or null
function overlayOf(job) {
    const s = parseSettings(job.codecSettings);
    if (s.overlay === undefined || s.overlay === null) return null;
    if (!Array.isArray(s.overlay)) throw new Error("job " + job.id + ": overlay must be a list of items");
    if (s.overlay.length > 256) throw new Error("job " + job.id + ": more than 256 overlay items");
    if (!s.overlay.length) return null;
    return s.overlay.map(function (it, i) {
        const what = "job " + job.id + " overlay item " + i + ": ";
        if (!it || typeof it !== "object") throw new Error(what + "not an object");
        if (typeof it.image !== "string" || !it.image) throw new Error(what + "image must name a file");
        const w = it.w, h = it.h;
        if (!Number.isInteger(w) || !Number.isInteger(h) || w < 1 || h < 1 || w > 16384 || h > 16384)
            throw new Error(what + "w / h must be integers in 1..16384");
        const vars = { W: job.width | 0, H: job.height | 0, w: w, h: h, main_w: job.width | 0, main_h: job.height | 0,
                       overlay_w: w, overlay_h: h };
        const first = it.from === undefined || it.from === null ? 0 : it.from;
        const last = it.to === undefined || it.to === null ? null : it.to;
        if (!Number.isInteger(first) || first < 0) throw new Error(what + "from must be a frame index >= 0");
        if (last !== null && (!Number.isInteger(last) || last < 0)) throw new Error(what + "to must be a frame index or null");
        try {
            return { image: it.image, w: w, h: h, x: overlayExpr(it.x === undefined ? 0 : it.x, vars),
                     y: overlayExpr(it.y === undefined ? 0 : it.y, vars), first: first, last: last };
        } catch (e) {
            throw new Error(what + e.message);
        }
    });
}

// codecSettings.sceneDetect: `scdet=threshold=T` ahead of the scale (vf_scdet.c; default 10): the
// scene-change scores of the SOURCE frames of every segment, reported in JobChunks.result.scenes.
// -> {threshold} or null
function sceneOf(job) {
    const s = parseSettings(job.codecSettings);
    if (!s.sceneDetect) return null;
    const t = s.sceneDetect === true ? 10 : (typeof s.sceneDetect === "object" && s.sceneDetect.threshold !== undefined ?
                                             s.sceneDetect.threshold : (typeof s.sceneDetect === "object" ? 10 : NaN));
    if (typeof t !== "number" || !(t >= 0 && t <= 100))
        throw new Error("job " + job.id + ": sceneDetect must be true or {\"threshold\": 0..100}");
    return { threshold: t };
}

const QUALITY = { psnr: 1, ssim: 2, both: 3, true: 3 };
const RANGE = { tv: 0, mpeg: 0, limited: 0, pc: 1, jpeg: 1, full: 1 };

// {src, dst}: DTS_RANGE_* of the source and of the renditions
function rangeOf(job) {
    const s = parseSettings(job.codecSettings);
    const r = function (v, what) {
        if (v === undefined) return 0;
        const x = RANGE[String(v).toLowerCase()];
        if (x === undefined) throw new Error("job " + job.id + ": unknown " + what + " " + v);
        return x;
    };
    return { src: r(s.inRange, "inRange"), dst: r(s.outRange, "outRange") };
}

// {mode, tff} or null
function deintOf(job) {
    const s = parseSettings(job.codecSettings);
    if (!s.deinterlace) return null;
    const d = typeof s.deinterlace === "object" ? s.deinterlace : {};
    if (typeof s.deinterlace === "string" && s.deinterlace.toLowerCase() !== "yadif")
        throw new Error("job " + job.id + ": unknown deinterlacer " + s.deinterlace);
    const mode = d.mode === undefined ? 0 : d.mode | 0;
    if (mode !== 0 && mode !== 2) throw new Error("job " + job.id + ": yadif mode " + mode + " (frame-rate modes 0 / 2 only)");
    const parity = String(d.parity || "tff").toLowerCase();
    if (parity !== "tff" && parity !== "bff") throw new Error("job " + job.id + ": yadif parity " + d.parity);
    return { mode: mode, tff: parity === "tff" ? 1 : 0 };
}

// {mode: DTS_Q_*, ref: DTS_SCALE_*} or null
function qualityOf(job) {
    const s = parseSettings(job.codecSettings);
    if (!s.quality) return null;
    const mode = QUALITY[String(s.quality).toLowerCase()];
    if (mode === undefined) throw new Error("job " + job.id + ": unknown quality " + s.quality);
    const ref = METHOD[String(s.qualityRef || "lanczos").toLowerCase()];
    if (ref === undefined) throw new Error("job " + job.id + ": unknown qualityRef " + s.qualityRef);
    return { mode: mode, ref: ref };
}

function tonemapOf(job) {
    const s = parseSettings(job.codecSettings);
    if (!s.tonemap) return null;
    const t = typeof s.tonemap === "string" ? { mode: s.tonemap } : s.tonemap;
    const mode = TONEMAP[String(t.mode || "hable").toLowerCase()];
    if (mode === undefined) throw new Error("job " + job.id + ": unknown tonemap " + t.mode);
    const r = { mode: mode };
    ["param", "desat", "peak", "npl"].forEach(function (k) { if (typeof t[k] === "number") r[k] = t[k]; });
    return r;
}

// Group rendition rows by source.  src: {w, h, fmt, fps: [num, den]} per sourceID.
// Returns [{sourceID, jobs: [row...], spec}] with at most MAX_OUTPUTS rows per graph
// (a larger ladder is split into several graphs over the same source).
function planLadders(jobs, sources) {
    const bySrc = new Map();                   // one ladder per (source, output frame rate)
    jobs.forEach(function (j) {
        const key = j.sourceID + "@" + (j.framerate || 0);
        if (!bySrc.has(key)) bySrc.set(key, []);
        bySrc.get(key).push(j);
    });
    const plans = [];
    bySrc.forEach(function (rows) {
        const sid = rows[0].sourceID;
        const src = sources[sid];
        if (!src) throw new Error("source " + sid + " has no stream info");
        rows.sort(function (a, b) { return b.width * b.height - a.width * a.height || a.id - b.id; });
        for (let i = 0; i < rows.length; i += MAX_OUTPUTS) {
            const part = rows.slice(i, i + MAX_OUTPUTS);
            const tm = tonemapOf(part[0]);
            part.forEach(function (r) {
                if (JSON.stringify(tonemapOf(r)) !== JSON.stringify(tm))
                    throw new Error("jobs " + part[0].id + "/" + r.id + ": one graph needs one tonemap setting");
            });
            const spec = { src: { w: src.w, h: src.h, fmt: src.fmt }, outputs: part.map(outputOf), quality: 0,
                           maxBatch: 32 };
            if (tm) spec.tonemap = tm;
            const di = deintOf(part[0]);
            part.forEach(function (r) {
                if (JSON.stringify(deintOf(r)) !== JSON.stringify(di))
                    throw new Error("jobs " + part[0].id + "/" + r.id + ": one graph needs one deinterlace setting");
            });
            if (di) spec.deint = di;
            const rg = rangeOf(part[0]);
            part.forEach(function (r) {
                if (JSON.stringify(rangeOf(r)) !== JSON.stringify(rg))
                    throw new Error("jobs " + part[0].id + "/" + r.id + ": one graph needs one range setting");
            });
            if (rg.src || rg.dst) { spec.srcRange = rg.src; spec.dstRange = rg.dst; }
            // per-rendition quality (codecSettings.quality): each requesting row against its
            // reference rendition, made and scored inside the same graph on the GPU
            // (dts_output_spec.quality / qref_method): no rendition crosses PCIe twice
            const q = part.map(qualityOf);
            const quality = q.some(function (x) { return x; }) ? { rows: q.map(function (x) { return x ? x.mode : 0; }) } : null;
            if (quality) spec.outputs.forEach(function (o, k) {
                if (q[k]) {
                    o.quality = q[k].mode;
                    o.qrefMethod = q[k].ref;
                }
            });
            if (quality && tm) throw new Error("job " + part[0].id + ": quality with tonemap is not supported");
            // burn-in overlays (codecSettings.overlay): the items ride on their output; the scheduler
            // makes a libdts overlay of them per GPU slot and attaches it to the graph's output
            part.forEach(function (r, k) {
                const ov = overlayOf(r);
                if (!ov) return;
                if (spec.outputs[k].fmt === FMT.p010le) throw new Error("job " + r.id + ": overlay on a p010 rendition is not supported");
                if (quality) throw new Error("job " + r.id + ": overlay in a ladder with quality is not supported");
                // frame ranges count output frames of the stream; a segment's position is only known
                // when the vf_fps map is the identity: a row that sets a framerate must be shown to
                // keep the source's (a source without a recorded rate cannot show it)
                const timed = ov.some(function (it) { return it.first > 0 || it.last !== null; });
                if (timed && r.framerate) {
                    const rt = rateOf(r.framerate);
                    if (!src.fps || rt[0] * src.fps[1] !== src.fps[0] * rt[1])
                        throw new Error("job " + r.id + ": an overlay item with a frame range (from / to) in a job that changes " +
                                        "the frame rate (" + (src.fps ? src.fps.join("/") : "unknown") + " -> " + r.framerate +
                                        ") is not supported; items shown for ever are");
                }
                spec.outputs[k].overlay = ov;
            });
            // scene detection (codecSettings.sceneDetect): one detector per graph scores its source
            // frames; the rows that ask must agree on the threshold
            const sc = part.map(sceneOf);
            let scene = null;
            part.forEach(function (r, k) {
                if (!sc[k]) return;
                if (!scene) scene = { threshold: sc[k].threshold, first: r.id, rows: part.map(function () { return false; }) };
                else if (sc[k].threshold !== scene.threshold)
                    throw new Error("jobs " + scene.first + "/" + r.id + ": one graph needs one sceneDetect threshold (" +
                                    scene.threshold + " / " + sc[k].threshold + ")");
                scene.rows[k] = true;
                // a cut's frame index counts source frames of the stream: the vf_fps map must be the identity
                if (r.framerate) {
                    const rt = rateOf(r.framerate);
                    if (!src.fps || rt[0] * src.fps[1] !== src.fps[0] * rt[1])
                        throw new Error("job " + r.id + ": sceneDetect in a job that changes the frame rate (" +
                                        (src.fps ? src.fps.join("/") : "unknown") + " -> " + r.framerate + ") is not supported");
                }
                if (di) throw new Error("job " + r.id + ": sceneDetect with deinterlace is not supported (scores after yadif are not built)");
            });
            if (scene) {
                delete scene.first;
                spec.scene = { threshold: scene.threshold };
            }
            plans.push({ sourceID: sid, framerate: part[0].framerate || 0, jobs: part, spec: spec, quality: quality,
                         scene: scene });
        }
    });
    return plans;
}

// Jobs.framerate (database.js:75) vs the source rate: the vf_fps (round=near)
// input frame of every output frame of a segment of `n` source frames.
function rateOf(fps) {
    return Number.isInteger(fps) ? [fps, 1] : [Math.round(fps * 1001), 1001];      // 29.97 -> 30000/1001
}

function fpsFrames(addon, n, srcFps, outFps) {
    if (!outFps || !srcFps) return null;
    const r = rateOf(outFps);
    if (r[0] * srcFps[1] === srcFps[0] * r[1]) return null;                       // same rate: identity
    return addon.fpsMap(n, srcFps[0], srcFps[1], r[0], r[1]);
}

// A segment's summed quality record from per-frame statistics (the addon's qstat
// objects): {frames, sse: [y, u, v], ssimSum: [y, u, v]} -- the running sums vf_psnr /
// vf_ssim keep (SSE exact; SSIM as the per-plane window sums), which add across segments.
// The per-plane window sums come back as ssim x windows (exact to the f64 rounding of the
// library's one division); a plane smaller than 8x8 has no SSIM window (vf_ssim scores none)
// and adds 0 (ADVICE r03: its NaN / negative count poisoned the job's sums).
function ssimWindows(pw, ph) {
    return Math.max(0, (pw >> 2) - 1) * Math.max(0, (ph >> 2) - 1);
}

function rawQuality(stats, w, h) {
    const pw = [w, (w + 1) >> 1, (w + 1) >> 1], ph = [h, (h + 1) >> 1, (h + 1) >> 1];
    const nw = [0, 1, 2].map(function (c) { return ssimWindows(pw[c], ph[c]); });
    const comp = ["y", "u", "v"], raw = { frames: stats.length, sse: [0, 0, 0], ssimSum: [0, 0, 0] };
    stats.forEach(function (q) {
        comp.forEach(function (c, i) {
            raw.sse[i] += q.sse[c];
            if (nw[i] > 0) raw.ssimSum[i] += q.ssim[c] * nw[i];
        });
    });
    return raw;
}

function addRaw(list) {
    const r = { frames: 0, sse: [0, 0, 0], ssimSum: [0, 0, 0] };
    list.forEach(function (x) {
        r.frames += x.frames;
        for (let i = 0; i < 3; ++i) {
            r.sse[i] += x.sse[i];
            r.ssimSum[i] += x.ssimSum[i];
        }
    });
    return r;
}

// vf_psnr / vf_ssim end-of-stream averages of a summed record: PSNR from the mean MSE
// (per plane and area-weighted overall), mean SSIM (as dts_qstat_stream)
function summarizeRaw(raw, w, h) {
    const pw = [w, (w + 1) >> 1, (w + 1) >> 1], ph = [h, (h + 1) >> 1, (h + 1) >> 1];
    const area = pw[0] * ph[0] + pw[1] * ph[1] + pw[2] * ph[2], n = raw.frames;
    const psnr = function (m) { return m === 0 ? "inf" : 10 * Math.log10(255 * 255 / m); };   // JSON has no Infinity
    const comp = ["y", "u", "v"], r = { frames: n, psnr: {}, ssim: {} };
    let mseAvg = 0, ssimAll = 0;
    let noWindows = false;
    comp.forEach(function (c, i) {
        const mse = raw.sse[i] / (n * pw[i] * ph[i]);
        const nw = ssimWindows(pw[i], ph[i]);
        r.psnr[c] = psnr(mse);
        r.ssim[c] = nw > 0 ? raw.ssimSum[i] / (n * nw) : null;      // no 8x8 window: no SSIM (not NaN)
        noWindows = noWindows || nw <= 0;
        mseAvg += mse * pw[i] * ph[i] / area;
        if (nw > 0) ssimAll += r.ssim[c] * pw[i] * ph[i] / area;
    });
    r.psnr.avg = psnr(mseAvg);
    r.ssim.all = noWindows ? null : ssimAll;
    return r;
}

// the same from the addon's qstatStream() object
function summaryOfStat(q, raw) {
    const f = function (x) { return x === Infinity ? "inf" : x; };
    const g = function (x) { return typeof x === "number" && isFinite(x) ? x : null; };   // 0/0 windows -> null
    return { frames: raw.frames, psnr: { y: f(q.psnr.y), u: f(q.psnr.u), v: f(q.psnr.v), avg: f(q.psnrAvg) },
             ssim: { y: g(q.ssim.y), u: g(q.ssim.u), v: g(q.ssim.v), all: g(q.ssimAll) } };
}

// Segment summary of per-frame statistics, as vf_psnr / vf_ssim print at the end of
// a stream: PSNR from the mean MSE (per plane and area-weighted overall), mean SSIM.
function summarizeQuality(stats, w, h) {
    const pw = [w, (w + 1) >> 1, (w + 1) >> 1], ph = [h, (h + 1) >> 1, (h + 1) >> 1];
    const area = pw[0] * ph[0] + pw[1] * ph[1] + pw[2] * ph[2];
    const comp = ["y", "u", "v"], n = stats.length;
    const mse = [0, 0, 0], ssim = [0, 0, 0];
    let ssimAll = 0;
    stats.forEach(function (q) {
        comp.forEach(function (c, i) {
            mse[i] += q.sse[c] / (pw[i] * ph[i]) / n;
            ssim[i] += q.ssim[c] / n;
        });
        ssimAll += q.ssimAll / n;
    });
    const psnr = function (m) { return m === 0 ? Infinity : 10 * Math.log10(255 * 255 / m); };
    const mseAvg = mse.reduce(function (a, m, i) { return a + m * pw[i] * ph[i] / area; }, 0);
    const r = { frames: n, psnr: {}, ssim: {} };
    comp.forEach(function (c, i) {
        r.psnr[c] = psnr(mse[i]);
        r.ssim[c] = ssim[i];
    });
    r.psnr.avg = psnr(mseAvg);
    r.ssim.all = ssimAll;
    return r;
}

module.exports = { FMT: FMT, METHOD: METHOD, TONEMAP: TONEMAP, MAX_OUTPUTS: MAX_OUTPUTS, parseSettings: parseSettings,
                   outputOf: outputOf, overlayOf: overlayOf, sceneOf: sceneOf, overlayExpr: overlayExpr, tonemapOf: tonemapOf, qualityOf: qualityOf, deintOf: deintOf, rangeOf: rangeOf,
                   planLadders: planLadders,
                   rateOf: rateOf, fpsFrames: fpsFrames, summarizeQuality: summarizeQuality, rawQuality: rawQuality,
                   addRaw: addRaw, summarizeRaw: summarizeRaw, summaryOfStat: summaryOfStat };
