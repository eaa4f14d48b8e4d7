// qhuff_wire.hip -- QPACK string literals decoded in place from wire data
// (gfx950).
//
// Reference path: the literals the reference decodes one at a time from
// inside its instruction readers (parse_header_data, lsqpack.c:3567-3915;
// lsqpack_dec_enc_in, lsqpack.c:4574-4960), each Huffman one through
// lsqpack_huff_decode, each into a header buffer that never outgrows
// LSXPACK_MAX_STRLEN (header_out_grow_buf, lsqpack.c:3346-3351).
//
// The batch kernel's tile pipeline (qhuff_decode.hip) over a third policy:
// a tile is 64 descriptors (struct qhuff_literal, one 128-bit load a lane)
// of literals that lie in wire order in one buffer, a few instruction bytes
// between them, so the tile's input is one contiguous span of that buffer
// and is staged as the batch kernel stages a tile of packed strings.  A
// Huffman lane takes the batch kernel's walk (decode_string), a raw lane
// copies its bytes from the stage; arena, compaction, look-back and stores
// are the batch kernel's.  The length limit of field sections is one
// compare a lane, except for a VALUE literal within its name's upper bound
// of the limit (qhuff_wire_impl.h wire_limit).  The lean structure: tiles
// past the 3 KB stages -- a long literal, or short ones far apart -- are
// coded out of line, each literal by its lane.
#include "qhuff_wire_impl.h"

#ifndef QH_DEC_PER
#define QH_DEC_PER 2
#endif

namespace qhuff {

__global__ __launch_bounds__(64 * kWaves) void
qhuff_wire_kernel(WireArgs w)
{
    __shared__ DecSmem smem;
    QH_LDS DecSmem *sm = (QH_LDS DecSmem *) &smem;
    const DecArgs &a = w.d;
    const int tid = threadIdx.x;
    // (ticket claims, then the table loads, stored once the first
    // descriptor loads are out)
    const auto p = dec_prologue<QH_DEC_PER>(a, sm, tid);
    const Tickets &tk = p.tk;
    const DecTableLoads tl = p.tl;
    WirePolicy pol{{a.in, sm,
                    &sm->w[__builtin_amdgcn_readfirstlane(tid >> 6)], 0},
                   WireLimit{(const ::qhuff_literal *) a.in_off, w.max_len}};
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
launch_wire(const WireArgs &a, uint32_t grid, hipStream_t st, hipEvent_t ev0,
            hipEvent_t ev1)
{
    return launch_kernel(qhuff_wire_kernel, grid, 64 * kWaves, st, ev0, ev1,
                         a);
}

int
wire_waves_per_block()
{
    return kWaves;
}

}  // namespace qhuff
