// overlay.hip -- k_overlay: vf_overlay (FFmpeg 4.4, format=yuv420, straight alpha) of
// yuva420p pictures on a batch of 8-bit 4:2:0 renditions, in place.
//
// One launch covers every frame of the batch and every item of a layer: a 1-D grid of
// exactly the workgroups the items need on the frames that show them (ov_map finds a
// workgroup's item and frame; none is launched for a frame that does not show its item).
// A thread owns a span of 4 NW target luma columns by 2 rows -- whole 2x2 luma blocks with
// their U and V samples (item positions are even, so the blocks line up with chroma) -- and
// reads each block's four alphas once for all three planes, each image row's share of the
// span as one aligned load.  Spans sit on 4 NW-byte boundaries of the target row: a span
// wholly inside the item's clipped rectangle moves as one 4 NW-byte access per row and
// plane, the head / tail spans (and a last odd row) byte by byte, so no byte outside the
// rectangle is touched.
#include "dts_internal.h"

namespace dts {

namespace {

__host__ __device__ __forceinline__ uint32_t ov_div255(uint32_t v) { return ((v + 128u) * 257u) >> 16; }
__host__ __device__ __forceinline__ uint32_t ov_blend(uint32_t d, uint32_t s, uint32_t a)
{
    return ov_div255(d * (255u - a) + s * a);
}

template <int N> struct OvWord;
template <> struct OvWord<2> { typedef uint16_t T; };
template <> struct OvWord<4> { typedef uint32_t T; };
template <> struct OvWord<8> { typedef uint64_t T; };

// N bytes at an N-byte aligned address as one access
template <int N>
__host__ __device__ __forceinline__ void ov_load(const uint8_t *p, uint32_t (&o)[N])
{
    const typename OvWord<N>::T v = *reinterpret_cast<const typename OvWord<N>::T *>(p);
#pragma unroll
    for (int c = 0; c < N; ++c) o[c] = (uint32_t)(v >> (8 * c)) & 255u;
}

template <int N>
__host__ __device__ __forceinline__ void ov_store(uint8_t *p, const uint32_t (&o)[N])
{
    typename OvWord<N>::T v = 0;
#pragma unroll
    for (int c = 0; c < N; ++c) v |= (typename OvWord<N>::T)o[c] << (8 * c);
    *reinterpret_cast<typename OvWord<N>::T *>(p) = v;
}

// one thread's work: thread tx of block (bx, item, frame) -- host-callable: tools/overlay_walk.cpp
// includes this file and walks whole grids on the CPU under AddressSanitizer / UBSan
template <int NW, bool NV12>
__host__ __device__ __forceinline__ void ov_thread(const OverlayParams &p, int bx, int item, int frame, int tx)
{
    constexpr int SPAN = 4 * NW, NB = SPAN / 2;
    const OvItem it = p.items[item];
    const int64_t n = p.first_frame + (int64_t)frame;
    if (n < it.first || (it.last >= 0 && n >= it.last)) return;
    // the item's rectangle clipped to the frame (tx0, ty0 even)
    const int tx0 = max(it.x, 0), ty0 = max(it.y, 0);
    const int tx1 = (int)min((int64_t)it.x + it.w, (int64_t)p.W);
    const int ty1 = (int)min((int64_t)it.y + it.h, (int64_t)p.H);
    if (tx0 >= tx1 || ty0 >= ty1) return;
    const int X0 = tx0 & ~(SPAN - 1);
    const int nsp = (tx1 - X0 + SPAN - 1) / SPAN;
    const int nrp = (ty1 - ty0 + 1) >> 1;
    const int t = bx * kOvThreads + tx;
    if (t >= nsp * nrp) return;
    const int rp = t / nsp, sp = t - rp * nsp;
    const int X = X0 + sp * SPAN, Y = ty0 + 2 * rp;
    const int j = (Y - it.y) >> 1;                  // image chroma row; luma rows 2 j, 2 j + 1
    const int cw = (it.w + 1) >> 1, ch = (it.h + 1) >> 1;
    const bool full = X >= tx0 && X + SPAN <= tx1;
    const bool row1 = Y + 1 < ty1;
    const bool jin = j + 1 < ch;

    // the image: the item's copy is shifted right by x & 7 columns (x & 7 >> 1 in chroma), so the
    // span's columns sit at an aligned offset of its rows and come as one load per row and plane
    // (zero columns / a zero row around w x h); the block's chroma alpha by vf_overlay's rule
    const int cb = X - (it.x & ~7);                 // >= 0, a multiple of SPAN
    const uint8_t *ia = p.blob + it.oa + (int64_t)(2 * j) * it.py + cb;
    const uint8_t *iy = p.blob + it.oy + (int64_t)(2 * j) * it.py + cb;
    uint32_t al[2][SPAN], sy[2][SPAN], ac[NB], su[NB], sv[NB];
    ov_load<SPAN>(ia, al[0]);
    ov_load<SPAN>(ia + it.py, al[1]);
    ov_load<SPAN>(iy, sy[0]);
    ov_load<SPAN>(iy + it.py, sy[1]);
    ov_load<NB>(p.blob + it.ou + (int64_t)j * it.pc + (cb >> 1), su);
    ov_load<NB>(p.blob + it.ov + (int64_t)j * it.pc + (cb >> 1), sv);
    bool bv[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int xb = X + 2 * b;
        bv[b] = xb >= tx0 && xb < tx1;
        const int k = (xb - it.x) >> 1;             // (meaningful where bv[b])
        const uint32_t a00 = al[0][2 * b], a01 = al[0][2 * b + 1], a10 = al[1][2 * b], a11 = al[1][2 * b + 1];
        const bool kin = k + 1 < cw;
        const uint32_t ah = kin ? (a00 + a01) >> 1 : a00;
        const uint32_t av = jin ? (a00 + a10) >> 1 : a00;
        ac[b] = (kin && jin) ? (a00 + a10 + a01 + a11) >> 2 : (av + ah) >> 1;
    }

    const int64_t fo = (int64_t)frame * p.dst.fstride;
    // luma: rows Y and Y + 1
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        if (r == 1 && !row1) break;
        uint8_t *d = reinterpret_cast<uint8_t *>(p.dst.data[0]) + fo + (int64_t)(Y + r) * p.dst.pitch[0] + X;
        if (full) {
            uint32_t px[SPAN];
            ov_load<SPAN>(d, px);
#pragma unroll
            for (int c = 0; c < SPAN; ++c) px[c] = ov_blend(px[c], sy[r][c], al[r][c]);
            ov_store<SPAN>(d, px);
        } else {
#pragma unroll
            for (int c = 0; c < SPAN; ++c)
                if (X + c >= tx0 && X + c < tx1) d[c] = (uint8_t)ov_blend(d[c], sy[r][c], al[r][c]);
        }
    }
    // chroma row Y / 2: U and V of every block
    if (NV12) {
        uint8_t *d = reinterpret_cast<uint8_t *>(p.dst.data[1]) + fo + (int64_t)(Y >> 1) * p.dst.pitch[1] + X;
        if (full) {
            uint32_t px[SPAN];
            ov_load<SPAN>(d, px);
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                px[2 * b] = ov_blend(px[2 * b], su[b], ac[b]);
                px[2 * b + 1] = ov_blend(px[2 * b + 1], sv[b], ac[b]);
            }
            ov_store<SPAN>(d, px);
        } else {
#pragma unroll
            for (int b = 0; b < NB; ++b)
                if (bv[b]) {
                    d[2 * b] = (uint8_t)ov_blend(d[2 * b], su[b], ac[b]);
                    d[2 * b + 1] = (uint8_t)ov_blend(d[2 * b + 1], sv[b], ac[b]);
                }
        }
    } else {
        // (U and V may have different pitches: each plane by its own)
        uint8_t *du = reinterpret_cast<uint8_t *>(p.dst.data[1]) + fo + (int64_t)(Y >> 1) * p.dst.pitch[1] + (X >> 1);
        uint8_t *dv = reinterpret_cast<uint8_t *>(p.dst.data[2]) + fo + (int64_t)(Y >> 1) * p.dst.pitch[2] + (X >> 1);
        if (full) {
            uint32_t pu[NB], pv[NB];
            ov_load<NB>(du, pu);
            ov_load<NB>(dv, pv);
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                pu[b] = ov_blend(pu[b], su[b], ac[b]);
                pv[b] = ov_blend(pv[b], sv[b], ac[b]);
            }
            ov_store<NB>(du, pu);
            ov_store<NB>(dv, pv);
        } else {
#pragma unroll
            for (int b = 0; b < NB; ++b)
                if (bv[b]) {
                    du[b] = (uint8_t)ov_blend(du[b], su[b], ac[b]);
                    dv[b] = (uint8_t)ov_blend(dv[b], sv[b], ac[b]);
                }
        }
    }
}

// workgroup `bid` of the launch -> its item, batch frame and workgroup inside the item's frame:
// the items' (workgroups per frame x frames shown) laid end to end, frame-major inside an
// item.  A uniform scan over the layer's items (scalar loads); false past the end.
__host__ __device__ __forceinline__ bool ov_map(const OverlayParams &p, int span, unsigned bid, int &item, int &frame,
                                                int &bx)
{
    for (int i = 0; i < p.nitems; ++i) {
        int nb, nf, f0;
        ov_item_blocks(p.items[i], p.W, p.H, span, p.first_frame, p.nframes, nb, nf, f0);
        const unsigned cnt = (unsigned)nb * (unsigned)nf;
        if (bid < cnt) {
            item = i;
            frame = f0 + (int)(bid / (unsigned)nb);
            bx = (int)(bid % (unsigned)nb);
            return true;
        }
        bid -= cnt;
    }
    return false;
}

template <int NW, bool NV12>
__global__ void __launch_bounds__(kOvThreads) k_overlay(const OverlayParams p)
{
    int item, frame, bx;
    if (!ov_map(p, 4 * NW, blockIdx.x, item, frame, bx)) return;
    ov_thread<NW, NV12>(p, bx, item, frame, (int)threadIdx.x);
}

} // namespace

hipError_t launch_overlay(const OverlayParams &p, unsigned blocks, bool nv12, bool wide, hipStream_t s)
{
    const dim3 grid(blocks), block(kOvThreads);
    if (wide) {
        if (nv12) hipLaunchKernelGGL((k_overlay<2, true>), grid, block, 0, s, p);
        else hipLaunchKernelGGL((k_overlay<2, false>), grid, block, 0, s, p);
    } else {
        if (nv12) hipLaunchKernelGGL((k_overlay<1, true>), grid, block, 0, s, p);
        else hipLaunchKernelGGL((k_overlay<1, false>), grid, block, 0, s, p);
    }
    return hipGetLastError();
}

} // namespace dts
