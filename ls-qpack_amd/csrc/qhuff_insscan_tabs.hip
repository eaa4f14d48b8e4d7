// qhuff_insscan_tabs.hip -- encoder-stream bytes of many connections walked
// for their inserts on the device (gfx950): qhuff_scan.hip's count and write
// launches over the insert walker (qhuff_scan_impl.h walk_insert_stream),
// chunk c against table c of a set (struct qhuff_dyn_tables).
//
// Reference path: lsqpack_dec_enc_in (lsqpack.c:4574-5030), the part of it
// that does not need a decoded string: the four instructions' framing, the
// static index (4620-4623), the capacity (5015) and a literal name's wire
// length (4798), once per connection.  The liveness of a reference and the
// lengths that depend on decoded names are the accounting's
// (qhuff_insapply_tabs.hip).
//
// One chunk a lane.  The lane tracks the capacity through its chunk -- it is
// cap[c] and the chunk's Set Capacity instructions alone -- and leaves per
// insert the two descriptors the decode launch reads, the capacities it is
// checked under and, for a reference to an insert of the same chunk, the
// root string (read back from what the lane wrote itself).  ent values are
// clamped to D = ent[T] (one uniform load), so no offset outside off[0 .. 2D]
// is read whatever ent holds; the wire bytes are read through the scan's
// window, which never leaves the blocks of buf[enc_off[0] .. enc_off[T]).
#include "qhuff_scan_dev.h"

namespace qhuff {

__global__ __launch_bounds__(kScanBlock) void
qhuff_insscan_tabs_count_kernel(InsScanArgs a)
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
        const uint32_t cap = a.cap[i], p = a.sec_off[i];
        scan::InsCountSink s{0, cap, cap};
        uint32_t stop = p;
        const int rc = scan::walk_insert_stream(r, s, p, a.sec_off[i + 1], cap,
                                                a.max_cap[i], &stop);
        const uint32_t n = rc ? 0u : s.n;
        a.rc[i] = rc ? QHUFF_EPROTO : QHUFF_OK;
        a.consumed[i] = rc ? 0u : stop - p;
        a.chunk_cap[2 * i] = rc ? cap : s.cmin;
        a.chunk_cap[2 * i + 1] = rc ? cap : s.cap;
        a.cnt[i] = n;
        if (n)
            atomicAdd(&tot, n);
    }
    __syncthreads();
    if (tid == 0)
        a.tot[blockIdx.x] = tot;
}

__global__ __launch_bounds__(kScanBlock) void
qhuff_insscan_tabs_write_kernel(InsScanArgs a)
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
        a.ins_off[0] = 0;
    a.ins_off[i + 1] = first + n;
    // (n != 0: the chunk's result was QHUFF_OK)
    const uint32_t last = first + n < a.max_ins ? first + n : a.max_ins;
    if (n == 0 || first >= last)
        return;
    WindowReader r(a);
    const uint32_t D = a.ent[a.m];
    const scan::TabView v = scan::ins_tab_view(a.ent, a.first, D,
                                               (uint32_t) i);
    scan::InsWriteSink w{a.strs, a.root, a.ins_cap, a.ins_ref, a.ins_kind,
                         a.off + 2ull * v.e0, v.d, v.first, first, first,
                         last};
    uint32_t stop;
    (void) scan::walk_insert_stream(r, w, a.sec_off[i], a.sec_off[i + 1],
                                    a.cap[i], a.max_cap[i], &stop);
}

hipError_t
launch_insscan_tabs(const InsScanArgs &a, unsigned step, hipStream_t st,
                    hipEvent_t ev0, hipEvent_t ev1)
{
    const uint32_t nb = scan_blocks(a.m);
    if (step == 0)
        return launch_kernel(qhuff_insscan_tabs_count_kernel, nb, kScanBlock,
                             st, ev0, ev1, a);
    return launch_kernel(qhuff_insscan_tabs_write_kernel, nb, kScanBlock, st,
                         ev0, ev1, a);
}

}  // namespace qhuff
