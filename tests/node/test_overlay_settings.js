"use strict";
// CPU: the worker's overlay settings -- the x / y expression evaluator, overlayOf,
// planLadders carrying the items on each output, the frame-rate refusal, the scheduler
// attaching overlays and setting the stream position, and filtergraph.js pointing an
// `overlay` in a linear -vf chain at the JSON field.
const assert = require("assert");
const fs = require("fs");
const os = require("os");
const path = require("path");
const root = path.join(__dirname, "..", "..", "distributed-transcoding-server_amd", "node");
const ladder = require(path.join(root, "ladder.js"));
const fg = require(path.join(root, "filtergraph.js"));
const { GpuSegmentScheduler } = require(path.join(root, "scheduler.js"));

// ---- expressions -----------------------------------------------------------
const V = { W: 1920, H: 1080, w: 200, h: 80, main_w: 1920, main_h: 1080, overlay_w: 200, overlay_h: 80 };
const ev = function (t) { return ladder.overlayExpr(t, V); };
assert.strictEqual(ev("W-w-20"), 1700);
assert.strictEqual(ev(20), 20);
assert.strictEqual(ev(-7), -7);
assert.strictEqual(ev(" ( main_w - overlay_w ) / 2 "), 860);
assert.strictEqual(ev("(H-h)/2"), 500);
assert.strictEqual(ev("W/3"), 640);
assert.strictEqual(ev("H/7"), 154);              // 154.28 truncated
assert.strictEqual(ev("-H/7"), -154);            // toward zero, not floor
assert.strictEqual(ev("7/2*2"), 7);              // doubles, truncated once at the end
assert.strictEqual(ev("2+3*4"), 14);
assert.strictEqual(ev("-(w+h)*2"), -560);
assert.strictEqual(ev("10 - 2 - 3"), 5);
["W-", "W w", "t*2", "sin(1)", "1.5", "W^2", "", "(W", "W)", "1/0", "n", "W;1", "if(1,2,3)"].forEach(function (t) {
    assert.throws(function () { ev(t); }, /overlay expression/, "should refuse '" + t + "'");
});
assert.throws(function () { ev(1.5); }, /not an integer/);

// ---- overlayOf / planLadders -----------------------------------------------
const item = { image: "logo.yuva", w: 20, h: 8, x: "W-w-20", y: 20, from: 0, to: null };
const sub = { image: "sub.yuva", w: 64, h: 12, x: "(W-w)/2", y: "H-h-4", from: 2, to: 5 };
const job = function (id, w, h, settings, fr) {
    return { id: id, sourceID: 1, width: w, height: h, framerate: fr === undefined ? 60 : fr,
             codecSettings: settings ? JSON.stringify(settings) : undefined };
};
assert.strictEqual(ladder.overlayOf(job(1, 192, 108, null)), null);
assert.strictEqual(ladder.overlayOf(job(1, 192, 108, { overlay: [] })), null);
assert.deepStrictEqual(ladder.overlayOf(job(1, 192, 108, { overlay: [item, sub] })),
                       [{ image: "logo.yuva", w: 20, h: 8, x: 152, y: 20, first: 0, last: null },
                        { image: "sub.yuva", w: 64, h: 12, x: 64, y: 92, first: 2, last: 5 }]);
[{ overlay: {} }, { overlay: [{ w: 2, h: 2 }] }, { overlay: [{ image: "a", w: 0, h: 2 }] },
 { overlay: [{ image: "a", w: 2, h: 2.5 }] }, { overlay: [{ image: "a", w: 2, h: 2, x: "q" }] },
 { overlay: [{ image: "a", w: 2, h: 2, from: -1 }] }, { overlay: [{ image: "a", w: 2, h: 2, to: 1.5 }] },
 { overlay: [null] }].forEach(function (s) {
    assert.throws(function () { ladder.overlayOf(job(9, 64, 36, s)); }, /job 9/, JSON.stringify(s));
});

const sources = { 1: { w: 384, h: 216, fmt: 0, fps: [60, 1] } };
let plans = ladder.planLadders([job(1, 192, 108, { overlay: [item, sub] }), job(2, 128, 72, { format: "yuv420p" })], sources);
assert.strictEqual(plans.length, 1);
assert.strictEqual(plans[0].spec.outputs[0].overlay.length, 2);
assert.strictEqual(plans[0].spec.outputs[0].overlay[1].x, 64);
assert.strictEqual(plans[0].spec.outputs[1].overlay, undefined);
// per rendition: the same expression lands elsewhere on another rung
plans = ladder.planLadders([job(1, 192, 108, { overlay: [item] }), job(2, 128, 72, { overlay: [item] })], sources);
assert.strictEqual(plans[0].spec.outputs[0].overlay[0].x, 152);
assert.strictEqual(plans[0].spec.outputs[1].overlay[0].x, 88);
// a time-ranged item in a job that changes the frame rate is refused; all-time items are fine
assert.throws(function () { ladder.planLadders([job(1, 192, 108, { overlay: [sub] }, 30)], sources); },
              /frame range.*changes the frame rate/);
assert.throws(function () { ladder.planLadders([job(1, 192, 108, { overlay: [item, sub] }, 29.97)], sources); },
              /frame range.*changes the frame rate/);
// ... and so is one whose source has no recorded rate: the map cannot be shown to be the identity
assert.throws(function () { ladder.planLadders([job(1, 192, 108, { overlay: [sub] }, 60)], { 1: { w: 384, h: 216, fmt: 0 } }); },
              /frame range.*unknown -> 60/);
plans = ladder.planLadders([job(1, 192, 108, { overlay: [sub] }, 0)], { 1: { w: 384, h: 216, fmt: 0 } });   // no framerate: no map
assert.strictEqual(plans[0].spec.outputs[0].overlay.length, 1);
plans = ladder.planLadders([job(1, 192, 108, { overlay: [item] }, 30)], sources);
assert.strictEqual(plans[0].spec.outputs[0].overlay.length, 1);
plans = ladder.planLadders([job(1, 192, 108, { overlay: [sub] }, 60)], sources);      // the identity map
assert.strictEqual(plans[0].spec.outputs[0].overlay[0].first, 2);
// p010 renditions and quality ladders take none
assert.throws(function () { ladder.planLadders([job(1, 192, 108, { format: "p010le", overlay: [item] })], sources); }, /p010/);
assert.throws(function () {
    ladder.planLadders([job(1, 192, 108, { overlay: [item] }), job(2, 128, 72, { quality: "psnr" })], sources);
}, /quality/);

// ---- filtergraph.js ----------------------------------------------------------
assert.throws(function () { fg.parseFiltergraph("scale=1280:720,overlay=10:10"); }, /"overlay" field/);
assert.throws(function () { ladder.outputOf(job(3, 1280, 720, null)) && ladder.parseSettings("-vf overlay=W-w:0"); },
              /unsupported filter 'overlay'.*JSON/);
assert.throws(function () { fg.parseFiltergraph("scale=1280:720,unsharp"); }, /unsupported filter 'unsharp'/);

// ---- scheduler: one overlay per (slot, row), attached after createGraph, position per segment
(async function () {
    const dir = fs.mkdtempSync(path.join(os.tmpdir(), "dts-ov-"));
    fs.writeFileSync(path.join(dir, "logo.yuva"), Buffer.alloc(2 * 20 * 8 + 2 * 10 * 4, 7));
    fs.writeFileSync(path.join(dir, "sub.yuva"), Buffer.alloc(2 * 64 * 12 + 2 * 32 * 6, 9));
    const calls = [];
    const addon = {
        deviceCount: function () { return 1; },
        createContext: function (d) { return { dev: d }; },
        createGraph: function (ctx, spec) { calls.push(["graph"]); return { spec: spec, ov: {} }; },
        createOverlay: function (ctx, images, items) { calls.push(["overlay", images, items]); return { images: images, items: items }; },
        graphSetOverlay: function (g, k, ov) { calls.push(["attach", k]); g.ov[k] = ov; },
        graphSetPosition: function (g, n) { calls.push(["pos", n]); },
        synthFrame: function () {},
        fpsMap: function () { throw new Error("identity expected"); },
        run: function (g, src, dst) { calls.push(["run", src.length]); return Promise.resolve(null); },
    };
    const jobs = [job(1, 192, 108, { overlay: [item, sub, item] }), job(2, 128, 72, null)];
    const chunks = [];
    jobs.forEach(function (j) {
        for (let off = 0; off < 3; ++off) chunks.push({ id: chunks.length + 1, mainJob: j.id, chunkOffset: off, status: null });
    });
    const sched = new GpuSegmentScheduler({ addon: addon, gpus: [0], segmentFrames: 4, baseDir: dir, sink: function () {} });
    await sched.runJobs(jobs, chunks, sources);
    assert(chunks.every(function (c) { return c.status === "done"; }), JSON.stringify(chunks));
    const ov = calls.filter(function (c) { return c[0] === "overlay"; });
    assert.strictEqual(ov.length, 1);                                  // once for the slot's graph, not per segment
    assert.strictEqual(ov[0][1].length, 2);                            // logo.yuva read into one image, used twice
    assert.deepStrictEqual(ov[0][2].map(function (i) { return i.image; }), [0, 1, 0]);
    assert.deepStrictEqual(ov[0][2][1], { image: 1, x: 64, y: 92, first: 2, last: 5 });
    assert.strictEqual(ov[0][1][0].data.length, 2 * 20 * 8 + 2 * 10 * 4);
    assert.deepStrictEqual(calls.filter(function (c) { return c[0] === "attach"; }), [["attach", 0]]);
    assert.deepStrictEqual(calls.filter(function (c) { return c[0] === "pos"; }).map(function (c) { return c[1]; }), [0, 4, 8]);
    const order = calls.map(function (c) { return c[0]; });
    assert(order.indexOf("graph") < order.indexOf("overlay") && order.indexOf("attach") < order.indexOf("pos") &&
           order.indexOf("pos") < order.indexOf("run"));
    // a second run of the same scheduler reads the files again (nothing is cached across runs)
    fs.writeFileSync(path.join(dir, "logo.yuva"), Buffer.alloc(2 * 20 * 8 + 2 * 10 * 4, 8));
    chunks.forEach(function (c) { c.status = null; });
    await sched.runJobs(jobs, chunks, sources);
    const ov2 = calls.filter(function (c) { return c[0] === "overlay"; });
    assert.strictEqual(ov2.length, 2);
    assert.strictEqual(ov2[0][1][0].data[0], 7);
    assert.strictEqual(ov2[1][1][0].data[0], 8);
    // an image file shorter than its planes is refused
    fs.writeFileSync(path.join(dir, "logo.yuva"), Buffer.alloc(10));
    const chunks2 = [{ id: 1, mainJob: 1, chunkOffset: 0, status: null }];
    const s2 = new GpuSegmentScheduler({ addon: addon, gpus: [0], segmentFrames: 4, baseDir: dir, sink: function () {}, maxRetries: 0 });
    await s2.runJobs([jobs[0]], chunks2, sources);
    assert.strictEqual(chunks2[0].status, "failed");
    assert(/yuva420p needs/.test(chunks2[0].result), chunks2[0].result);
    // a ladder without overlays never touches the new addon calls
    const n0 = calls.length;
    const plain = { deviceCount: addon.deviceCount, createContext: addon.createContext, createGraph: addon.createGraph,
                    synthFrame: addon.synthFrame, run: addon.run };
    const chunks3 = [{ id: 1, mainJob: 2, chunkOffset: 0, status: null }];
    await new GpuSegmentScheduler({ addon: plain, gpus: [0], segmentFrames: 4, sink: function () {} }).runJobs([jobs[1]], chunks3, sources);
    assert.strictEqual(chunks3[0].status, "done");
    assert(calls.slice(n0).every(function (c) { return c[0] === "graph" || c[0] === "run"; }));
    fs.rmdirSync(dir, { recursive: true });
    console.log("overlay settings ok");
})().catch(function (e) {
    console.error(e && e.stack || e);
    process.exit(1);
});
