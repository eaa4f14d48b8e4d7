// qhuff_hdrscan.hip -- field sections walked for their header lines on the
// device (gfx950): the descriptors qhuff_decode_headers reads -- two a header,
// a literal where the line carries one, a static-table entry's name or value
// where it names one -- and each line's kind, static index and N bit.
//
// Reference path: what the reference's decoder does per line of a section
// that does not use the dynamic table (header_out_static_entry,
// header_out_begin_static_nameref, header_out_begin_literal,
// lsqpack.c:3013-3057, 3121-3159, 3211-3323, from the dispatch of
// parse_header_data, 3567-3915).
//
// The literal scan's shape (qhuff_scan.hip, whose window reader and block
// sums this file shares through qhuff_scan_dev.h): one section a lane, walked
// serially (qhuff_scan_impl.h walk_header_section); a count launch, the
// literal scan's own top launch over the workgroup totals, a write launch
// that walks the OK sections again.  Headers are counted, not literals.
#include "qhuff_scan_dev.h"

namespace qhuff {

__global__ __launch_bounds__(kScanBlock) void
qhuff_hdrscan_count_kernel(HdrScanArgs a)
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
        scan::HdrCountSink s{0};
        const int rc = scan::walk_header_section(r, s, a.sec_off[i],
                                                 a.sec_off[i + 1]);
        a.rc[i] = rc;
        a.cnt[i] = s.n;
        if (s.n)
            atomicAdd(&tot, s.n);
    }
    __syncthreads();
    if (tid == 0)
        a.tot[blockIdx.x] = tot;
}

__global__ __launch_bounds__(kScanBlock) void
qhuff_hdrscan_write_kernel(HdrScanArgs a)
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
        a.hdr_off[0] = 0;
    a.hdr_off[i + 1] = first + n;
    // (n != 0: the section's result was QHUFF_OK)
    const uint32_t last = first + n < a.max_hdrs ? first + n : a.max_hdrs;
    if (n == 0 || first >= last)
        return;
    WindowReader r(a);
    scan::HdrWriteSink w{a.strs, a.kind, a.static_id, a.hflags, first, last};
    (void) scan::walk_header_section(r, w, a.sec_off[i], a.sec_off[i + 1]);
}

hipError_t
launch_hdrscan(const HdrScanArgs &a, unsigned step, hipStream_t st,
               hipEvent_t ev0, hipEvent_t ev1)
{
    const uint32_t nb = scan_blocks(a.m);
    if (step == 0)
        return launch_kernel(qhuff_hdrscan_count_kernel, nb, kScanBlock, st,
                             ev0, ev1, a);
    return launch_kernel(qhuff_hdrscan_write_kernel, nb, kScanBlock, st, ev0,
                         ev1, a);
}

}  // namespace qhuff
