// qhuff_hdrdec_dyn.hip -- header lists decoded from field sections against
// the static table and the dynamic table's entries (gfx950).
//
// Reference path: qhuff_hdrdec.hip's, and the header the reference's decoder
// hands out for a line that names a dynamic entry -- the entry's name and
// value (header_out_dynamic_entry, lsqpack.c:3060-3117), or its name and a
// literal value (header_out_begin_dynamic_nameref, from 3655-3662).  The
// table is read, never written.
//
// qhuff_hdrdec.hip's kernel over a policy with a third string source
// (qhuff_hdrdec_dyn_impl.h DynPolicy): a tile is 64 descriptors = 32 whole
// headers; a WIRE string is staged, walked or copied into its arena slot and
// compacted; a STATIC string comes from the table in the code object's
// constant data; a DYN string is `len` bytes of the caller's table at `instr`
// -- its lane sizes it from the descriptor it already holds, so the tile's
// size scan waits for no second load, and once the offsets are scanned copies
// it from global memory (the table is small and read by every tile: L2) into
// the out stage with aligned dword reads; an entry longer than 64 bytes is
// copied by the whole wave.  Tiles past the 3 KB stages -- the dynamic bytes
// count in the output -- are coded out of line, table to global memory.
#include "qhuff_hdrdec_dyn_impl.h"

#ifndef QH_DEC_PER
#define QH_DEC_PER 2
#endif

namespace qhuff {

__global__ __launch_bounds__(64 * kWaves) void
qhuff_hdrdec_dyn_kernel(HdrDynArgs h)
{
    __shared__ DecSmem smem;
    QH_LDS DecSmem *sm = (QH_LDS DecSmem *) &smem;
    const DecArgs &a = h.w.d;
    const int tid = threadIdx.x;
    // (ticket claims, then the table loads, stored once the first
    // descriptor loads are out)
    const auto p = dec_prologue<QH_DEC_PER>(a, sm, tid);
    const Tickets &tk = p.tk;
    const DecTableLoads tl = p.tl;
    DynPolicy pol{{a.in, sm,
                   &sm->w[__builtin_amdgcn_readfirstlane(tid >> 6)], 0},
                  h.w.max_len, DynBytes{h.dyn, h.dyn_len}, StaticStr{0, 0},
                  DynStr{0, 0}};
    uint32_t t0, k1, k2;
    wave_tickets(a.c, tk, &sm->tk, &t0, &k1, &k2);
    auto tables = [&, tl]() {
        tl.store(sm, tid);
        __syncthreads();             // the tables
    };
    tile_pipeline(pol, a.c, tk, t0, k1, k2, a.in, a.in_off,
                  a.n, a.out, a.out_off, a.status, tables);
}

hipError_t
launch_hdrdec_dyn(const HdrDynArgs &a, uint32_t grid, hipStream_t st,
                  hipEvent_t ev0, hipEvent_t ev1)
{
    return launch_kernel(qhuff_hdrdec_dyn_kernel, grid, 64 * kWaves, st, ev0,
                         ev1, a);
}

int
hdrdec_dyn_waves_per_block()
{
    return kWaves;
}

}  // namespace qhuff
