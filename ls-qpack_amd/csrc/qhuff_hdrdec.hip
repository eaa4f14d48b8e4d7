// qhuff_hdrdec.hip -- header lists decoded from field sections against the
// static table (gfx950): the inverse of qhuff_encode_headers.
//
// Reference path: the header the reference's decoder hands out per line of a
// section that does not use the dynamic table -- a static entry's name and
// value (header_out_static_entry, lsqpack.c:3013-3057), a static name and a
// literal value (header_out_begin_static_nameref, 3121-3159), two literals
// (header_out_begin_literal / _write_name / _write_value, 3211-3323) -- each
// literal through lsqpack_huff_decode into a buffer that never outgrows
// LSXPACK_MAX_STRLEN (header_out_grow_buf, 3346-3351).
//
// The wire kernel's tile pipeline (qhuff_wire.hip) over a fourth policy of
// the decode family: a tile is 64 descriptors (struct qhuff_hstr, one
// 128-bit load a lane) = 32 whole headers, name on the even lane, value on
// the odd one, so a header never straddles a tile and the limit's name is
// always the lane before.  A WIRE string is a literal of the wire kernel:
// staged, walked or copied into its arena slot, compacted.  A STATIC string
// has no wire bytes: its lane sizes it from the static table's lengths and,
// once the tile's offsets are scanned, writes the entry's bytes from the
// table in this code object's constant data (the vector cache; four bytes a
// step) straight into the out stage.  A tile of 32 indexed lines stages an
// empty span and decodes nothing.  The lean structure: tiles past the 3 KB
// stages -- the static bytes count in the output -- are coded out of line.
#include "qhuff_hdrdec_impl.h"

#ifndef QH_DEC_PER
#define QH_DEC_PER 2
#endif

namespace qhuff {

__global__ __launch_bounds__(64 * kWaves) void
qhuff_hdrdec_kernel(WireArgs w)
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
    HdrPolicy pol{{a.in, sm,
                   &sm->w[__builtin_amdgcn_readfirstlane(tid >> 6)], 0},
                  w.max_len, StaticStr{0, 0}};
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
launch_hdrdec(const WireArgs &a, uint32_t grid, hipStream_t st, hipEvent_t ev0,
              hipEvent_t ev1)
{
    return launch_kernel(qhuff_hdrdec_kernel, grid, 64 * kWaves, st, ev0, ev1,
                         a);
}

int
hdrdec_waves_per_block()
{
    return kWaves;
}

}  // namespace qhuff
