// overlay_walk.cpp -- k_overlay's grid walked on the CPU under AddressSanitizer / UBSan (no GPU):
// overlay.hip's per-thread body (ov_thread) and workgroup map (ov_map) are host-callable, so
// this program includes the kernel file and runs every thread of every workgroup of the grid
// the host would launch (ov_item_blocks) -- plus three workgroups past its end -- over random
// renditions, images, positions (inside, off every edge, outside), both formats, both access
// widths and U / V planes of different pitches, on heap buffers of the exact size, and
// compares every byte of the batch with a plain restatement of vf_overlay's blend_plane.
// Built and run by tools/overlay_walk.sh.  Exit status 0 = no difference and no report.
#include "../distributed-transcoding-server_amd/csrc/overlay.hip"
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>
using namespace dts;

static int div255(int v) { return ((v + 128) * 257) >> 16; }
static int64_t au(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

int main()
{
    std::mt19937 rng(7);
    auto rnd = [&](int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); };
    long cases = 0, bad = 0;
    for (int iter = 0; iter < 6000; ++iter) {
        const int W = rnd(1, 70), H = rnd(1, 40), w = rnd(1, 90), h = rnd(1, 50);
        const int nv12 = rnd(0, 1), wide = rnd(0, 1);
        int x = rnd(-w - 3, W + 3) & ~1, y = rnd(-h - 3, H + 3) & ~1;
        const int cw = (w + 1) / 2, ch = (h + 1) / 2, CW = (W + 1) / 2, CH = (H + 1) / 2;
        // image
        std::vector<uint8_t> iY(w * h), iA(w * h), iU(cw * ch), iV(cw * ch);
        for (auto &v : iY) v = rng();
        for (auto &v : iU) v = rng();
        for (auto &v : iV) v = rng();
        for (auto &v : iA) { int r = rnd(0, 5); v = r == 0 ? 0 : r == 1 ? 255 : rng(); }
        OvItem it{};
        it.x = x; it.y = y; it.w = w; it.h = h; it.first = 0; it.last = -1;
        const int pad = x & 7;
        it.py = (int)au(pad + w + 8, 16); it.pc = (int)au(pad / 2 + cw + 4, 16);
        size_t tot = 0;
        it.oy = tot; tot += (size_t)it.py * (h + 1);
        it.oa = tot; tot += (size_t)it.py * (h + 1);
        it.ou = tot; tot += (size_t)it.pc * ch;
        it.ov = tot; tot += (size_t)it.pc * ch;
        uint8_t *blob = (uint8_t *)calloc(tot, 1);
        for (int r = 0; r < h; ++r) {
            memcpy(blob + it.oy + (size_t)r * it.py + pad, &iY[r * w], w);
            memcpy(blob + it.oa + (size_t)r * it.py + pad, &iA[r * w], w);
        }
        for (int r = 0; r < ch; ++r) {
            memcpy(blob + it.ou + (size_t)r * it.pc + pad / 2, &iU[r * cw], cw);
            memcpy(blob + it.ov + (size_t)r * it.pc + pad / 2, &iV[r * cw], cw);
        }
        // frame: exact-size planes (ASan redzones right after the last row)
        const int al = wide ? 8 : 4;
        const int64_t p0 = au(W, al) + (wide ? 0 : (au(W, 4) % 8 ? 0 : 4));
        const int64_t cb = nv12 ? 2 * CW : CW;
        const int64_t p1 = au(cb, nv12 && wide ? 8 : 4);
        const int nfr = 2;
        const int64_t p2 = nv12 ? p1 : p1 + 4 * rnd(0, 2);      // planar: V with a pitch of its own
        const int64_t fs = au(p0 * H + (p1 + p2) * CH + 64, 8);
        uint8_t *buf = (uint8_t *)aligned_alloc(16, fs * nfr);
        for (int64_t i = 0; i < fs * nfr; ++i) buf[i] = rng();
        std::vector<uint8_t> ref(buf, buf + fs * nfr);
        OverlayParams p{};
        p.dst.data[0] = (uint64_t)buf;
        p.dst.data[1] = (uint64_t)(buf + au(p0 * H, 8));
        p.dst.data[2] = nv12 ? p.dst.data[1] : (uint64_t)(buf + au(p0 * H, 8) + au(p1 * CH, 4));
        p.dst.pitch[0] = p0; p.dst.pitch[1] = p1; p.dst.pitch[2] = p2;
        p.dst.fstride = fs;
        p.W = W; p.H = H; p.first_frame = 3; p.items = &it; p.blob = blob;
        // reference on `ref`
        for (int f = 0; f < nfr; ++f) {
            uint8_t *r0 = ref.data() + f * fs, *r1 = r0 + (p.dst.data[1] - p.dst.data[0]), *r2 = r0 + (p.dst.data[2] - p.dst.data[0]);
            for (int j = 0; j < h; ++j) for (int i = 0; i < w; ++i) {
                int tx = x + i, ty = y + j;
                if (tx < 0 || tx >= W || ty < 0 || ty >= H) continue;
                int a = iA[j * w + i];
                uint8_t *d = r0 + ty * p0 + tx;
                *d = div255(*d * (255 - a) + iY[j * w + i] * a);
            }
            for (int j = 0; j < ch; ++j) for (int k = 0; k < cw; ++k) {
                int tx = (x >> 1) + k, ty = (y >> 1) + j;
                if (tx < 0 || tx >= CW || ty < 0 || ty >= CH) continue;
                int a0 = iA[2 * j * w + 2 * k], alpha;
                if (j + 1 < ch && k + 1 < cw) alpha = (a0 + iA[(2 * j + 1) * w + 2 * k] + iA[2 * j * w + 2 * k + 1] + iA[(2 * j + 1) * w + 2 * k + 1]) >> 2;
                else {
                    int ah = k + 1 < cw ? (a0 + iA[2 * j * w + 2 * k + 1]) >> 1 : a0;
                    int av = j + 1 < ch ? (a0 + iA[(2 * j + 1) * w + 2 * k]) >> 1 : a0;
                    alpha = (av + ah) >> 1;
                }
                uint8_t *du = nv12 ? r1 + ty * p1 + 2 * tx : r1 + ty * p1 + tx;
                uint8_t *dv = nv12 ? du + 1 : r2 + ty * p2 + tx;
                *du = div255(*du * (255 - alpha) + iU[j * cw + k] * alpha);
                *dv = div255(*dv * (255 - alpha) + iV[j * cw + k] * alpha);
            }
        }
        // 1-D grid as overlay_launches sizes it (+ 3 workgroups past the end: ov_map must refuse them)
        const int span = wide ? 8 : 4;
        it.first = 4; it.last = rnd(0, 1) ? -1 : 5;          // batch = stream frames 3, 4: frame 0 never shown
        // the reference blended both frames: undo frame 0 (and frame 1 is shown: first 4 <= 4 < last)
        memcpy(ref.data(), buf, fs);
        OvItem two[2] = {it, it};
        two[0].first = 0; two[0].last = 3;                   // an item that shows on no frame of the batch
        p.items = two; p.nitems = 2; p.nframes = nfr;
        long blocks = 0;
        for (int i = 0; i < 2; ++i) { int nb, nf, f0; ov_item_blocks(two[i], W, H, span, p.first_frame, nfr, nb, nf, f0); blocks += (long)nb * nf; }
        for (unsigned bid = 0; bid < blocks + 3; ++bid) {
            int item, frame, bx;
            const bool ok = ov_map(p, span, bid, item, frame, bx);
            if (ok != (bid < blocks)) { printf("MAP bid %u\n", bid); ++bad; }
            if (!ok) continue;
            for (int t = 0; t < kOvThreads; ++t) {
                if (wide) { if (nv12) ov_thread<2, true>(p, bx, item, frame, t); else ov_thread<2, false>(p, bx, item, frame, t); }
                else { if (nv12) ov_thread<1, true>(p, bx, item, frame, t); else ov_thread<1, false>(p, bx, item, frame, t); }
            }
        }
        ++cases;
        if (memcmp(buf, ref.data(), fs * nfr)) {
            ++bad;
            if (bad < 5) printf("MISMATCH W%d H%d w%d h%d x%d y%d nv12 %d wide %d\n", W, H, w, h, x, y, nv12, wide);
        }
        free(buf);
        free(blob);
    }
    printf("overlay_walk: %ld cases, %ld bad\n", cases, bad);
    return bad != 0;
}
