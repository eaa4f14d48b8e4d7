// qhuff_scan_dev.h -- the device side both scans share (qhuff_scan.hip: the
// literals; qhuff_hdrscan.hip: the header lines): a lane's window on the wire
// bytes and the workgroup's exclusive sums.  See qhuff_scan.hip.
#pragma once
#include "qhuff_kernels.h"
#include "qhuff_scan_impl.h"

// (QH_SCAN_BLOCKS is kept to reproduce the window-width comparison of
// profiles/scan/ab_read_path.txt: -DQH_SCAN_BLOCKS=4 or 8 through the
// Makefile's DEFS.  With 1 the window is two words and one compare.)
#ifndef QH_SCAN_BLOCKS
#define QH_SCAN_BLOCKS 1
#endif

namespace qhuff {

constexpr int kWinBlocks = QH_SCAN_BLOCKS;
static_assert(kWinBlocks >= 1 && (kWinBlocks & (kWinBlocks - 1)) == 0,
              "window blocks: a power of two");

struct WindowReader
{
    const uint8_t *buf;
    uintptr_t lo, hi;                    // the batch's blocks: [lo, hi] are
                                         // the first and the last one
    uintptr_t span;                      // address of the span held (1: none)
    uint64_t w[2 * kWinBlocks];

    // (A: ScanArgs or HdrScanArgs -- buf, sec_off, m)
    template <class A>
    __device__ __forceinline__ WindowReader(const A &a)
        : buf(a.buf), span(1)
    {
        lo = (uintptr_t) (a.buf + a.sec_off[0]) & ~(uintptr_t) 15;
        hi = ((uintptr_t) (a.buf + a.sec_off[a.m]) - 1) & ~(uintptr_t) 15;
    }

    __device__ __forceinline__ uint8_t get(uint32_t pos)
    {
        const uintptr_t a = (uintptr_t) (buf + pos);
        const uintptr_t b = a & ~(uintptr_t) (16 * kWinBlocks - 1);
        if (b != span)
        {
#pragma unroll
            for (int k = 0; k < kWinBlocks; ++k)
            {
                uintptr_t at = b + 16 * k;
                at = at < lo ? lo : at > hi ? hi : at;
                const u32x4 v = *(const QH_GLB u32x4 *) at;
                w[2 * k] = v.x | (uint64_t) v.y << 32;
                w[2 * k + 1] = v.z | (uint64_t) v.w << 32;
            }
            span = b;
        }
        const uint32_t k = (uint32_t) (a >> 3) & (2 * kWinBlocks - 1);
        uint64_t h = w[0];
#pragma unroll
        for (int j = 1; j < 2 * kWinBlocks; ++j)
            h = k == (uint32_t) j ? w[j] : h;
        return (uint8_t) (h >> ((a & 7) * 8));
    }
};

// exclusive sums of one value a thread over a workgroup of N threads
// (N a power of two); *total = the sum.  `s` holds N words.
template <uint32_t N>
__device__ __forceinline__ uint32_t
block_exclusive(uint32_t v, uint32_t *s, uint32_t tid, uint32_t *total)
{
    s[tid] = v;
    __syncthreads();
    for (uint32_t d = 1; d < N; d <<= 1)
    {
        const uint32_t x = tid >= d ? s[tid - d] : 0;
        __syncthreads();
        s[tid] += x;
        __syncthreads();
    }
    const uint32_t incl = s[tid];
    *total = s[N - 1];
    __syncthreads();                     // (s may be used again)
    return incl - v;
}

}  // namespace qhuff
