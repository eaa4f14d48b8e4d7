// qhuff_hdrscan_tabs.hip -- field sections of many connections walked for
// their header lines on the device (gfx950): qhuff_hdrscan_dyn.hip's count
// and write launches over the same walker, each section against its own
// table of a set (struct qhuff_dyn_tables, include/qhuff.h).
//
// Reference path: qhuff_hdrscan_dyn.hip's -- the reference's decoder per
// dynamic line and per section prefix (lsqpack.c:2768-2775, 3060-3117,
// 3955-4046) -- once per connection: a set of tables is that many decoders'
// tables held in one arena.  The tables are only read.
//
// One section a lane.  The only new thing a lane does is build its
// scan::DynWin from its section's table (qhuff_scan_impl.h dyn_win_tabs): one
// load of sec_tab[s], then ent[c], ent[c + 1], first[c] and max_entries[c],
// with `off` based at off + 2 * ent[c].  The walk, the sinks and the
// descriptors are the _dyn kernels': an entry's three offsets are already
// byte offsets in the shared bytes, which is what a DYN descriptor's instr
// is.  sec_tab[s] is clamped to T - 1, ent values to D = ent[T] (read here,
// one uniform load) and a window into its table, so no offset outside
// off[0 .. 2D] is read whatever sec_tab, ent and sec_win hold.
#include "qhuff_scan_dev.h"

namespace qhuff {

__device__ __forceinline__ scan::DynWin
tabs_win(const HdrScanTabsArgs &a, uint64_t i)
{
    const uint32_t D = a.T ? a.ent[a.T] : 0;
    return scan::dyn_win_tabs(a.off, a.ent, a.first, a.max_entries, a.T, D,
                              a.sec_tab, a.sec_win, i);
}

__global__ __launch_bounds__(kScanBlock) void
qhuff_hdrscan_tabs_count_kernel(HdrScanTabsArgs d)
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
                                                 tabs_win(d, i));
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
qhuff_hdrscan_tabs_write_kernel(HdrScanTabsArgs d)
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
                                     tabs_win(d, i));
}

hipError_t
launch_hdrscan_tabs(const HdrScanTabsArgs &a, unsigned step, hipStream_t st,
                    hipEvent_t ev0, hipEvent_t ev1)
{
    const uint32_t nb = scan_blocks(a.h.m);
    if (step == 0)
        return launch_kernel(qhuff_hdrscan_tabs_count_kernel, nb, kScanBlock,
                             st, ev0, ev1, a);
    return launch_kernel(qhuff_hdrscan_tabs_write_kernel, nb, kScanBlock, st,
                         ev0, ev1, a);
}

}  // namespace qhuff
