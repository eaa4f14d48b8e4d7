// qhuff_decode.hip -- batch Huffman decode kernel (gfx950).
//
// Reference path:
//   D1 lsqpack_huff_decode  lsqpack.c:3520-3535 (resume == 0 && final)
//   D2 huff_decode_fast     lsqpack.c:5234-5466 (16-bit window table, slow
//                           path to the nibble FSM for long codes)
//   D3 accept/reject rule: ERROR iff the EOS code occurs, or the bits after
//      the last complete symbol are >= 8 or not all ones
//      (lsqpack.c:5362-5426, 3482-3497)
//
// One string per lane, one 64-string tile per wave (qhuff_device.h).  The
// tile's Huffman input is staged in the wave's LDS region as big-endian
// dwords.  Each lane holds its bit stream as two dwords A:B and a bit
// position (decode_string): a step looks the next 13 bits up in a window
// table (up to two symbols of <= 13 bits), writes the entry's two symbol
// bytes to the string's arena slot and advances by the bits consumed.
// Codes of 14..30 bits stall their lane and are decoded together outside the
// step loop by a canonical length search.  Main steps run while the lane has
// >= 13 real bits; the last < 13 bits (at most two symbols) take a padded
// one-lookup epilogue that applies the D3 tail rule (fewer than 8 padding
// bits, all ones).
//
// After the wave scan of the output sizes the arena slots are compacted
// into the (now dead) input stage and copied out with 16-byte stores once
// the look-back has resolved the tile's output base.
#include "qhuff_decode_impl.h"

// tickets claimed per wave in the prologue, at most (see qhuff_encode.hip)
#ifndef QH_DEC_PER
#define QH_DEC_PER 2
#endif

namespace qhuff {

// Keep: the per-string entry points' kernel (DecPolicyT); a template
// parameter, so the batch kernel's code and registers are untouched
template <bool Keep, bool Full>
__global__ __launch_bounds__(64 * kWaves) void
qhuff_decode_kernel(DecArgs a)
{
    __shared__ DecSmem smem;
    QH_LDS DecSmem *sm = (QH_LDS DecSmem *) &smem;
    const int tid = threadIdx.x;
    prof_realtime(a.c, kProfIters - 1, 10);      // (profiling) wave entry
    const auto p = dec_prologue<QH_DEC_PER>(a, sm, tid);
    const Tickets &tk = p.tk;
    const DecTableLoads tl = p.tl;
    prof_realtime(a.c, kProfIters - 1, 11);      // (profiling) after it
    DecPolicyT<DecSmem, Keep, Full> pol{
        {a.in, sm, &sm->w[__builtin_amdgcn_readfirstlane(tid >> 6)], 0}};
#ifdef QHUFF_PROFILE
    pol.pc = &a.c;
#endif
    uint32_t t0, k1, k2;
    wave_tickets(a.c, tk, &sm->tk, &t0, &k1, &k2);
    // (tl by value: by reference the kernel's prologue is scheduled
    // differently)
    auto tables = [&, tl]() {
        tl.store(sm, tid);
        __syncthreads();             // the tables
    };
    tile_pipeline(pol, a.c, tk, t0, k1, k2, a.in, a.in_off,
                  a.n, a.out, a.out_off, a.status, tables);
}

hipError_t
launch_decode(const DecArgs &a, uint32_t grid, hipStream_t st, hipEvent_t ev0,
              hipEvent_t ev1, bool keep, bool full)
{
    // (the keep kernel is never timed)
    if (keep)
        return launch_kernel(qhuff_decode_kernel<true, false>, grid,
                             64 * kWaves, st, nullptr, nullptr, a);
    return launch_kernel(full ? qhuff_decode_kernel<false, true>
                              : qhuff_decode_kernel<false, false>,
                         grid, 64 * kWaves, st, ev0, ev1, a);
}

hipError_t
decode_occupancy(int *blocks_per_cu)
{
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(
        blocks_per_cu, reinterpret_cast<const void *>(qhuff_decode_kernel<false, true>),
        64 * kWaves, 0);
}

int
decode_waves_per_block()
{
    return kWaves;
}

uint32_t
decode_tile_strings()
{
    return kDecTS;
}

size_t
decode_lds_bytes()
{
    hipFuncAttributes fa;
    if (hipFuncGetAttributes(&fa, reinterpret_cast<const void *>(qhuff_decode_kernel<false, true>))
            != hipSuccess)
        return 0;
    return fa.sharedSizeBytes;
}

}  // namespace qhuff
