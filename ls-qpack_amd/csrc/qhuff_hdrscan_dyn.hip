// qhuff_hdrscan_dyn.hip -- field sections walked for their header lines on
// the device (gfx950) against the dynamic table's entries: qhuff_hdrscan.hip's
// two launches over the same walker with a table policy (qhuff_scan_impl.h
// DynWin), so that a line which names a dynamic entry becomes two DYN
// descriptors instead of ending its section with QHUFF_ENOTSUP.
//
// Reference path: what the reference's decoder does per dynamic line -- the
// entry resolved from Base and the line's index (qdec_get_table_entry_abs,
// lsqpack.c:2768-2775), name and value copied out (header_out_dynamic_entry,
// 3060-3117; header_out_begin_dynamic_nameref, from 3655-3662) -- and per
// section prefix (parse_header_prefix, 3955-4046).  The table is only read.
//
// One section a lane.  The count launch needs the section's window and
// MaxEntries only; the write launch reads the entry's three offsets,
// off[2k .. 2k + 2], per dynamic line: a dependent load in a serial walk,
// from an array that stays in L2.  A window is clamped into the table
// (DynWin::of), so no offset outside off[0 .. 2d] is read whatever sec_win
// holds.
#include "qhuff_scan_dev.h"

namespace qhuff {

__device__ __forceinline__ scan::DynWin
dyn_win(const HdrScanDynArgs &a, uint64_t i)
{
    return scan::DynWin::of(a.off, a.d, a.first, a.max_entries, a.sec_win, i);
}

__global__ __launch_bounds__(kScanBlock) void
qhuff_hdrscan_dyn_count_kernel(HdrScanDynArgs d)
{
    __shared__ uint32_t tot;
    const HdrScanArgs &a = d.h;
    const uint32_t tid = threadIdx.x;
    const uint64_t i = (uint64_t) blockIdx.x * kScanBlock + tid;
    if (tid == 0)
        tot = 0;
    __syncthreads();
    if (i < a.m)
    {
        WindowReader r(a);
        scan::HdrDynCountSink s{0};
        const int rc = scan::walk_header_section(r, s, a.sec_off[i],
                                                 a.sec_off[i + 1],
                                                 dyn_win(d, i));
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
qhuff_hdrscan_dyn_write_kernel(HdrScanDynArgs d)
{
    __shared__ uint32_t s[kScanBlock];
    const HdrScanArgs &a = d.h;
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
    scan::HdrDynWriteSink w{{a.strs, a.kind, a.static_id, a.hflags, first,
                             last}, d.dyn_id};
    (void) scan::walk_header_section(r, w, a.sec_off[i], a.sec_off[i + 1],
                                     dyn_win(d, i));
}

hipError_t
launch_hdrscan_dyn(const HdrScanDynArgs &a, unsigned step, hipStream_t st,
                   hipEvent_t ev0, hipEvent_t ev1)
{
    const uint32_t nb = scan_blocks(a.h.m);
    if (step == 0)
        return launch_kernel(qhuff_hdrscan_dyn_count_kernel, nb, kScanBlock,
                             st, ev0, ev1, a);
    return launch_kernel(qhuff_hdrscan_dyn_write_kernel, nb, kScanBlock, st,
                         ev0, ev1, a);
}

}  // namespace qhuff
