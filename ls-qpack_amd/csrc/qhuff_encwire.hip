// qhuff_encwire.hip -- whole QPACK field lines and encoder-stream
// instructions encoded in one launch (gfx950).
//
// Reference path: every instruction the reference's encoder writes
// (lsqpack_enc_encode, lsqpack.c:1963-2124; the field-section prefix,
// lsqpack.c:1277, 1296) is an optional prefixed integer whose first byte
// carries the instruction bits (lsqpack_enc_int, lsqpack.c:787-814)
// followed by an optional string literal (lsqpack_enc_enc_str,
// lsqpack.c:839-876), or a name literal whose first byte carries them
// followed by a value literal.
//
// The batch kernel's tile pipeline (qhuff_encode.hip) over a third policy:
// a tile is 64 items (struct qhuff_item, one 64-bit load a lane beside the
// lane's offset pair), each an integer, a literal of string i, both or
// neither.  The dense pass runs over the staged span as it does for a batch
// of strings; sizing adds the integer's bytes to the literal's, framed with
// the lane's own prefix width; emit writes the integer, then the literal
// with str_first OR-ed into its first byte, into the zeroed output stage;
// look-back and stores are the batch kernel's.  The lean structure: a tile
// whose input span passes the 3 KB stage or whose output does not leave 64
// bytes of the output stage free is coded out of line, every item by its
// lane straight to global memory; a tile whose dense stream overflows is
// sized and packed item per lane from the stage (as the batch kernel's).
// No speed is promised for either.
#include "qhuff_encwire_impl.h"

#ifndef QH_ENC_PER
#define QH_ENC_PER 2
#endif

namespace qhuff {

__global__ __launch_bounds__(64 * kWaves) void
qhuff_encwire_kernel(EncWireArgs w)
{
    __shared__ EncSmem smem;
    QH_LDS EncSmem *sm = (QH_LDS EncSmem *) &smem;
    const EncArgs &a = w.e;
    const int tid = threadIdx.x;
    const Tickets tk = enc_prologue<QH_ENC_PER>(a.c, &sm->tk, [sm, &a, tid] {
        enc_tables_load(sm, a.enc, tid);
    });
    EncWirePolicyT<EncSmem> pol;
    pol.in = a.in;
    pol.sm = sm;
    pol.wv = &sm->w[__builtin_amdgcn_readfirstlane(tid >> 6)];
    pol.dense = false;
    uint32_t t0, k1, k2;
    wave_tickets(a.c, tk, &sm->tk, &t0, &k1, &k2);
    tile_pipeline(pol, a.c, tk, t0, k1, k2, a.in, a.in_off,
                  a.n, a.out, a.out_off, nullptr);
}

hipError_t
launch_encwire(const EncArgs &e, const ::qhuff_item *items, uint32_t grid,
               hipStream_t st, hipEvent_t ev0, hipEvent_t ev1)
{
    EncWireArgs a;
    a.items = items;
    a.e = e;
    return launch_kernel(qhuff_encwire_kernel, grid, 64 * kWaves, st, ev0,
                         ev1, a);
}

int
encwire_waves_per_block()
{
    return kWaves;
}

}  // namespace qhuff
