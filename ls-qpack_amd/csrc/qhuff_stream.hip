// qhuff_stream.hip -- batch resumable Huffman decode kernel (gfx950).
//
// Reference path: the second decoder, lsqpack_huff_decode_full
// (lsqpack.c:3443-3517, qdec_huff_dec4bits 5213-5231), which every call of
// lsqpack_huff_decode takes that is not `resume == 0 && final`
// (lsqpack.c:3520-3535): a literal that straddles two stream reads.
//
// The batch kernel's tile pipeline (qhuff_decode.hip) over another policy:
// string i's chunk i is decoded by one lane from the tree node its earlier
// chunks ended on (state[i].state, a node id: qhuff_tables.h) to the node it
// ends on.  The reference walks its tree a nibble at a time; here the node
// is turned back into its bit prefix, the one code it is in the middle of is
// resolved with the batch kernel's tables, and the rest of the chunk takes
// the batch kernel's window-table walk itself (window_walk,
// qhuff_decode_impl.h) under a stop policy that stops -- instead of
// rejecting -- where a code runs past the chunk's end
// (qhuff_stream_impl.h).  The tables' staging, the LDS layout, the staged
// source and the emitters are the batch kernel's too.  The lean structure:
// tiles past the 3 KB stages are coded out of line, each chunk by its lane.
#include "qhuff_stream_impl.h"

#ifndef QH_DEC_PER
#define QH_DEC_PER 2
#endif

namespace qhuff {

__global__ __launch_bounds__(64 * kWaves) void
qhuff_stream_kernel(StreamArgs s)
{
    __shared__ StreamSmem smem;
    QH_LDS StreamSmem *sm = (QH_LDS StreamSmem *) &smem;
    const DecArgs &a = s.d;
    const int tid = threadIdx.x;
    // (ticket claims, then the table loads -- the nodes among them --
    // stored once the first offsets loads are out)
    static_assert(kNodes <= 64 * kWaves, "one node per thread");
    const auto p = dec_prologue<QH_DEC_PER>(a, sm, tid, [&](int t) {
        return glb(s.nodes)[t < kNodes ? t : 0];
    });
    const Tickets &tk = p.tk;
    const DecTableLoads tl = p.tl;
    const uint32_t nd = p.own;
    StreamPolicy pol{{a.in, sm,
                      &sm->w[__builtin_amdgcn_readfirstlane(tid >> 6)], 0},
                     StreamIo{s.state, s.flags}, StreamEnd{0, 0, 0}};
    uint32_t t0, k1, k2;
    wave_tickets(a.c, tk, &sm->tk, &t0, &k1, &k2);
    auto tables = [&, tl]() {
        tl.store(sm, tid);
        if (tid < kNodes)
            sm->nodes[tid] = nd;
        __syncthreads();             // the tables
    };
    tile_pipeline(pol, a.c, tk, t0, k1, k2, a.in, a.in_off,
                  a.n, a.out, a.out_off, a.status, tables);
}

hipError_t
launch_stream(const StreamArgs &a, uint32_t grid, hipStream_t st,
              hipEvent_t ev0, hipEvent_t ev1)
{
    return launch_kernel(qhuff_stream_kernel, grid, 64 * kWaves, st, ev0, ev1,
                         a);
}

int
stream_waves_per_block()
{
    return kWaves;
}

}  // namespace qhuff
