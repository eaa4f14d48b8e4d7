// qhuff_scan.hip -- field sections and encoder streams walked for their
// literals on the device (gfx950): the descriptors qhuff_decode_wire reads,
// made where the wire bytes already are.
//
// Reference path: the framing the reference walks one instruction at a time
// inside parse_header_data (lsqpack.c:3567-3915) and lsqpack_dec_enc_in
// (lsqpack.c:4574-4960); here, as in the host scanners (qhuff_frames.cpp),
// only the framing is walked and nothing is resolved.
//
// One chunk a lane, walked serially (qhuff_scan_impl.h): every byte's
// meaning depends on the bytes before it.  Three launches, none of which
// waits for another workgroup:
//   count   rc, consumed and the literal count of every chunk; a total per
//           workgroup
//   top     one workgroup turns the totals into exclusive sums
//   write   each workgroup scans its own counts from its sum, writes lit_off
//           and walks its OK chunks again, now writing descriptors.  The
//           second walk reads what the first left in L2 / MALL.
//
// Read path: a lane keeps a window of QH_SCAN_BLOCKS aligned 16-byte blocks
// (one aligned span) around the byte it is at in registers and refills it,
// by that many independent 16-byte loads, only when the walk leaves it: a
// payload is jumped over, not read.  One block is the default: wider windows
// and a copy of the workgroup's chunks in LDS were measured and are no
// faster.  A block of the span that lies outside the
// batch's own blocks is not loaded: its load is moved to a block of the
// batch (the walker never asks for a byte outside its chunk, so what such a
// slot holds is never looked at).
#include "qhuff_scan_dev.h"

namespace qhuff {

__global__ __launch_bounds__(kScanBlock) void
qhuff_scan_count_kernel(ScanArgs a)
{
    __shared__ uint32_t tot;
    const uint32_t tid = threadIdx.x;
    const uint64_t i = (uint64_t) blockIdx.x * kScanBlock + tid;
    if (tid == 0)
        tot = 0;
    __syncthreads();
    if (i < a.m)
    {
        WindowReader r(a);
        scan::CountSink s{0};
        uint32_t used;
        const int rc = scan::walk_chunk(r, s, a.mode, a.sec_off[i],
                                        a.sec_off[i + 1], &used);
        a.rc[i] = rc;
        if (a.consumed)
            a.consumed[i] = used;
        a.cnt[i] = s.n;
        if (s.n)
            atomicAdd(&tot, s.n);
    }
    __syncthreads();
    if (tid == 0)
        a.tot[blockIdx.x] = tot;
}

// tot[0 .. nb) -> their exclusive sums, in rounds of kScanTop
__global__ __launch_bounds__(kScanTop) void
qhuff_scan_top_kernel(uint32_t *tot, uint32_t nb)
{
    __shared__ uint32_t s[kScanTop];
    const uint32_t tid = threadIdx.x;
    uint32_t carry = 0;
    for (uint32_t b0 = 0; b0 < nb; b0 += kScanTop)
    {
        const uint32_t k = b0 + tid;         // (b0 < nb <= 2^24: no wrap)
        const uint32_t v = k < nb ? tot[k] : 0;
        uint32_t sum;
        const uint32_t ex = block_exclusive<kScanTop>(v, s, tid, &sum);
        if (k < nb)
            tot[k] = carry + ex;
        carry += sum;
    }
}

__global__ __launch_bounds__(kScanBlock) void
qhuff_scan_write_kernel(ScanArgs a)
{
    __shared__ uint32_t s[kScanBlock];
    const uint32_t tid = threadIdx.x;
    const uint64_t i = (uint64_t) blockIdx.x * kScanBlock + tid;
    const bool live = i < a.m;
    const uint32_t n = live ? a.cnt[i] : 0;
    uint32_t sum;
    const uint32_t first = a.tot[blockIdx.x]
                         + block_exclusive<kScanBlock>(n, s, tid, &sum);
    if (!live)
        return;
    if (i == 0)
        a.lit_off[0] = 0;
    a.lit_off[i + 1] = first + n;
    // (n != 0: the chunk's result was QHUFF_OK)
    const uint32_t last = first + n < a.max_lits ? first + n : a.max_lits;
    if (n == 0 || first >= last)
        return;
    WindowReader r(a);
    scan::WriteSink w{a.lits, first, last};
    uint32_t used;
    (void) scan::walk_chunk(r, w, a.mode, a.sec_off[i], a.sec_off[i + 1],
                            &used);
}

// launch `step` of the three (0 count, 1 top, 2 write) on st, m >= 1
hipError_t
launch_scan(const ScanArgs &a, unsigned step, hipStream_t st, hipEvent_t ev0,
            hipEvent_t ev1)
{
    const uint32_t nb = scan_blocks(a.m);
    if (step == 0)
        return launch_kernel(qhuff_scan_count_kernel, nb, kScanBlock, st, ev0,
                             ev1, a);
    if (step == 2)
        return launch_kernel(qhuff_scan_write_kernel, nb, kScanBlock, st, ev0,
                             ev1, a);
    if (ev0)
        hipExtLaunchKernelGGL(qhuff_scan_top_kernel, dim3(1), dim3(kScanTop),
                              0, st, ev0, ev1, 0, a.tot, nb);
    else
        hipLaunchKernelGGL(qhuff_scan_top_kernel, dim3(1), dim3(kScanTop), 0,
                           st, a.tot, nb);
    return hipGetLastError();
}

}  // namespace qhuff
