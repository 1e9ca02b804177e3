// scdet.hip -- k_scdet: the luma SAD of vf_scdet (FFmpeg 4.4; `select`'s scene score is the same
// sum) between consecutive frames of a batch, one launch per batch, every luma byte read once.
//
// The plane is cut into 16-byte units, H x ceil(row bytes / 16) of them in row-major order.  A
// workgroup owns kScdThreads x kScdUnits consecutive units -- a band of rows, part rows at its
// ends -- and walks the batch's frames in time: a thread keeps its kScdUnits units of the previous
// frame in registers, loads the same units of the next frame and sums |cur - prev|, so frame f
// serves as `cur` and then as `prev` from one load.  The "previous" of frame 0 comes from the
// detector's kept plane (its own pitch); without one frame 0 only seeds the registers and the
// host marks it as having no predecessor.
//
// Sums are integers all the way (bitwise the same from run to run): a thread's u32 per frame,
// a wave's by shuffles, the workgroup's by one LDS add per wave into the frame's slot of a
// kScdChunk-frame window, and every kScdChunk frames one u64 atomic add per (workgroup, frame) into
// sad[f].  No u32 partial can overflow, whatever the plane's width (16384 and beyond): a
// workgroup's share of a frame is at most kScdThreads x kScdUnits x 16 bytes = 8 KiB, i.e.
// 8192 x 255 = 2.1e6 for 8-bit samples and 4096 x 1023 = 4.2e6 for 10-bit ones, far below 2^32;
// only the per-frame total (7680 x 4320 x 255 > 2^32) needs the u64.
//
// Units whose 16 bytes lie inside the row move as one 16-byte load when the batch's base, pitch
// and frame stride are multiples of 16 (4-byte or sample-sized loads otherwise).  A row's last,
// partial unit is read sample by sample up to the row's end and no further: pitch padding is
// neither counted nor -- in the last row, where nothing may follow it -- read.  The kernel reads
// plane 0 only and writes nothing but sad[].
#include "dts_internal.h"

namespace dts {

namespace {

// acc + sum of |a - b| over the samples of a dword: four bytes, or two p010 words >> 6
template <int BPS>
__host__ __device__ __forceinline__ uint32_t scd_sad(uint32_t a, uint32_t b, uint32_t acc)
{
    if (BPS == 2) {
        a = (a >> 6) & 0x03ff03ffu;
        b = (b >> 6) & 0x03ff03ffu;
    }
#if defined(__HIP_DEVICE_COMPILE__)
    return BPS == 1 ? __builtin_amdgcn_sad_u8(a, b, acc) : __builtin_amdgcn_sad_u16(a, b, acc);
#else
    constexpr int NB = 8 * BPS;
#pragma unroll
    for (int i = 0; i < 32; i += NB) {
        const uint32_t x = (a >> i) & ((1u << NB) - 1u), y = (b >> i) & ((1u << NB) - 1u);
        acc += x > y ? x - y : y - x;
    }
    return acc;
#endif
}

// one unit: nb valid bytes (16, a row's tail, or 0 past the plane) at p into four dwords, zeros
// beyond nb.  A whole unit moves in LW-byte accesses (p is a multiple of LW), a tail sample by sample
template <int BPS, int LW>
__host__ __device__ __forceinline__ void scd_load(const uint8_t *p, int nb, uint32_t (&v)[4])
{
    if (nb == 16) {
        if (LW == 16) {
            const uint4 q = *reinterpret_cast<const uint4 *>(p);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else if (LW == 4) {
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = reinterpret_cast<const uint32_t *>(p)[i];
        } else if (LW == 2) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                v[i] = (uint32_t)reinterpret_cast<const uint16_t *>(p)[2 * i] |
                       (uint32_t)reinterpret_cast<const uint16_t *>(p)[2 * i + 1] << 16;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                v[i] = (uint32_t)p[4 * i] | (uint32_t)p[4 * i + 1] << 8 | (uint32_t)p[4 * i + 2] << 16 |
                       (uint32_t)p[4 * i + 3] << 24;
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = 0;
#pragma unroll
    for (int s = 0; s < 16; s += BPS) {
        if (s >= nb) break;
        const uint32_t x = BPS == 2 ? (uint32_t)*reinterpret_cast<const uint16_t *>(p + s) : (uint32_t)p[s];
        v[s >> 2] |= x << (8 * (s & 3));
    }
}

// thread tx of workgroup wg: its units' SAD for every scored frame, handed to emit(f, sum) in
// frame order -- every thread of the workgroup calls emit for the same frames (threads past the
// plane with 0).  Host-callable: tools/scdet_walk.cpp includes this file and walks whole grids on
// the CPU under AddressSanitizer / UBSan
template <int BPS, int LW, class Emit>
__host__ __device__ __forceinline__ void scd_thread(const ScdParams &p, unsigned wg, int tx, Emit &&emit)
{
    const int64_t total = (int64_t)p.H * p.upr;
    int row[kScdUnits], col[kScdUnits], nb[kScdUnits];
#pragma unroll
    for (int j = 0; j < kScdUnits; ++j) {
        const int64_t u = ((int64_t)wg * kScdUnits + j) * kScdThreads + tx;
        row[j] = col[j] = nb[j] = 0;
        if (u < total) {
            row[j] = (int)(u / p.upr);
            col[j] = (int)(u - (int64_t)row[j] * p.upr) * 16;
            nb[j] = p.rowb - col[j] < 16 ? p.rowb - col[j] : 16;
        }
    }
    uint32_t prev[kScdUnits][4], cur[kScdUnits][4];
    const uint8_t *src = reinterpret_cast<const uint8_t *>(p.src);
    int f = 0;
    if (p.prev) {                                   // the kept plane: 16-byte aligned whatever the batch is
        const uint8_t *kp = reinterpret_cast<const uint8_t *>(p.prev);
#pragma unroll
        for (int j = 0; j < kScdUnits; ++j) scd_load<BPS, 16>(kp + (int64_t)row[j] * p.prev_pitch + col[j], nb[j], prev[j]);
    } else {
#pragma unroll
        for (int j = 0; j < kScdUnits; ++j) scd_load<BPS, LW>(src + (int64_t)row[j] * p.pitch + col[j], nb[j], prev[j]);
        f = 1;
    }
    for (; f < p.nframes; ++f) {
        const uint8_t *fr = src + (int64_t)f * p.fstride;
#pragma unroll
        for (int j = 0; j < kScdUnits; ++j) scd_load<BPS, LW>(fr + (int64_t)row[j] * p.pitch + col[j], nb[j], cur[j]);
        uint32_t acc = 0;
#pragma unroll
        for (int j = 0; j < kScdUnits; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                acc = scd_sad<BPS>(cur[j][i], prev[j][i], acc);
                prev[j][i] = cur[j][i];
            }
        emit(f, acc);
    }
}

template <int BPS, int LW>
__global__ void __launch_bounds__(kScdThreads) k_scdet(const ScdParams p)
{
    __shared__ uint32_t part[kScdChunk];           // the workgroup's sums of a window of frames
    const int tx = (int)threadIdx.x;
    if (tx < kScdChunk) part[tx] = 0;
    __syncthreads();
    scd_thread<BPS, LW>(p, blockIdx.x, tx, [&](int f, uint32_t acc) {
#pragma unroll
        for (int o = 32; o; o >>= 1) acc += __shfl_down(acc, o, 64);
        const int slot = f % kScdChunk;
        if ((tx & 63) == 0 && acc) atomicAdd(&part[slot], acc);
        if (slot == kScdChunk - 1 || f == p.nframes - 1) {      // (uniform: every thread sees the same f)
            __syncthreads();
            if (tx <= slot) {
                const uint32_t v = part[tx];
                if (v) atomicAdd(&p.sad[f - slot + tx], (unsigned long long)v);
                part[tx] = 0;
            }
            __syncthreads();
        }
    });
}

} // namespace

hipError_t launch_scdet(const ScdParams &p, int bps, int lw, hipStream_t s)
{
    const dim3 grid(scd_blocks(p.rowb, p.H)), block(kScdThreads);
    if (bps == 1) {
        if (lw == 16) hipLaunchKernelGGL((k_scdet<1, 16>), grid, block, 0, s, p);
        else if (lw == 4) hipLaunchKernelGGL((k_scdet<1, 4>), grid, block, 0, s, p);
        else hipLaunchKernelGGL((k_scdet<1, 1>), grid, block, 0, s, p);
    } else {
        if (lw == 16) hipLaunchKernelGGL((k_scdet<2, 16>), grid, block, 0, s, p);
        else if (lw == 4) hipLaunchKernelGGL((k_scdet<2, 4>), grid, block, 0, s, p);
        else hipLaunchKernelGGL((k_scdet<2, 2>), grid, block, 0, s, p);
    }
    return hipGetLastError();
}

} // namespace dts
