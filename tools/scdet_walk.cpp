// scdet_walk.cpp -- k_scdet's grid walked on the CPU under AddressSanitizer / UBSan (no GPU):
// scdet.hip's per-thread body (scd_thread) and its workgroup count (scd_blocks) are
// host-callable, so this program includes the kernel file and runs every thread of every
// workgroup the host would launch -- plus three workgroups past the end -- over random sizes,
// both sample sizes, every load width with bases / pitches / frame strides aligned to exactly
// that width, with and without a kept plane, on heap buffers that end at the last row's last
// sample (a redzone follows), and compares each frame's sum with a plain loop.
// Built and run by tools/scdet_walk.sh.  Exit status 0 = no difference and no report.
#include "../distributed-transcoding-server_amd/csrc/scdet.hip"
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>
using namespace dts;

static int64_t au(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

template <int BPS, int LW>
static void walk(const ScdParams &p, unsigned blocks, std::vector<uint64_t> &sum)
{
    for (unsigned wg = 0; wg < blocks + 3; ++wg)
        for (int t = 0; t < kScdThreads; ++t)
            scd_thread<BPS, LW>(p, wg, t, [&](int f, uint32_t acc) { sum[(size_t)f] += acc; });
}

int main()
{
    std::mt19937 rng(11);
    auto rnd = [&](int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); };
    long cases = 0, bad = 0;
    for (int iter = 0; iter < 3000; ++iter) {
        const int bps = rnd(1, 2);
        // mostly small planes; some of several workgroups (> 16 KiB of luma)
        const int W = iter % 50 == 0 ? rnd(300, 700) : rnd(1, 90), H = iter % 50 == 0 ? rnd(30, 60) : rnd(1, 40);
        const int lws[3] = {16, 4, bps};
        const int lw = lws[rnd(0, 2)];
        const int n = rnd(1, 5), kept = rnd(0, 1);
        const int64_t rowb = (int64_t)W * bps;
        // pitch / frame stride / base: multiples of lw and (lw < 16) of nothing larger
        int64_t pitch = au(rowb, lw) + (int64_t)lw * rnd(0, 3);
        if (lw < 16 && pitch % (2 * lw) == 0) pitch += lw;
        const int64_t used = pitch * (H - 1) + rowb;             // a frame's last byte is its last sample
        int64_t fs = au(used, lw) + (int64_t)lw * rnd(0, 2);
        if (lw < 16 && fs % (2 * lw) == 0) fs += lw;
        const int64_t skew = lw < 16 ? lw : 0;
        const int64_t bytes = skew + fs * (n - 1) + used;
        // posix_memalign: a 16-byte aligned block of exactly `bytes`, the redzone right after it
        void *heap = nullptr;
        if (posix_memalign(&heap, 16, (size_t)bytes)) return 2;
        uint8_t *buf = (uint8_t *)heap;
        for (int64_t i = 0; i < bytes; ++i) buf[i] = (uint8_t)rng();
        const uint8_t *src = buf + skew;
        const int64_t kp = au(rowb, 16);
        uint8_t *kbuf = nullptr;
        if (kept) {
            kbuf = (uint8_t *)aligned_alloc(16, (size_t)(kp * H));
            for (int64_t i = 0; i < kp * H; ++i) kbuf[i] = (uint8_t)rng();
        }
        ScdParams p{};
        p.src = (uint64_t)src;
        p.pitch = pitch;
        p.fstride = fs;
        p.prev = (uint64_t)kbuf;
        p.prev_pitch = kp;
        p.rowb = (int32_t)rowb;
        p.H = H;
        p.upr = (int32_t)((rowb + 15) / 16);
        p.nframes = n;
        p.sad = nullptr;
        std::vector<uint64_t> got((size_t)n, 0), want((size_t)n, 0);
        auto sample = [&](const uint8_t *row, int x) {
            return bps == 2 ? (int)((row[2 * x] | row[2 * x + 1] << 8) >> 6) : (int)row[x];
        };
        for (int f = kept ? 0 : 1; f < n; ++f)
            for (int y = 0; y < H; ++y) {
                const uint8_t *a = src + f * fs + y * pitch;
                const uint8_t *b = f ? src + (f - 1) * fs + y * pitch : kbuf + y * kp;
                for (int x = 0; x < W; ++x) want[(size_t)f] += (uint64_t)abs(sample(a, x) - sample(b, x));
            }
        const unsigned blocks = scd_blocks((int)rowb, H);
        if ((int64_t)blocks * kScdThreads * kScdUnits < (int64_t)H * p.upr) { printf("GRID too small\n"); ++bad; }
        if (bps == 1) {
            if (lw == 16) walk<1, 16>(p, blocks, got);
            else if (lw == 4) walk<1, 4>(p, blocks, got);
            else walk<1, 1>(p, blocks, got);
        } else {
            if (lw == 16) walk<2, 16>(p, blocks, got);
            else if (lw == 4) walk<2, 4>(p, blocks, got);
            else walk<2, 2>(p, blocks, got);
        }
        ++cases;
        if (got != want) {
            ++bad;
            if (bad < 5) printf("MISMATCH W%d H%d bps %d lw %d n %d kept %d pitch %ld fs %ld\n", W, H, bps, lw, n, kept, (long)pitch, (long)fs);
        }
        free(heap);
        free(kbuf);
    }
    printf("scdet_walk: %ld cases, %ld bad\n", cases, bad);
    return bad != 0;
}
