// qhuff_insapply_tabs.hip -- encoder-stream inserts applied to a set of tables
// on the device (gfx950): the accounting of every table, the sums over the
// tables and the copy that assembles the next arena
// (qhuff_apply_inserts_tabs; the source of the rules is
// qhuff_tabs_insert_impl.h, shared with qhuff_tabs_insert_cpu).
//
// Reference path: what lsqpack_dec_enc_in does once a literal is decoded --
// qdec_get_table_entry_rel (lsqpack.c:2756-2764), the length checks
// (4661-4667, 4878-4884), lsqpack_dec_push_entry (4534-4552) and
// qdec_remove_overflow_entries (4362-4377) -- once per connection, and the
// repacking of every connection's entries into one arena, which a host does
// with one memcpy per entry.
//
// Three launches, none of which waits for another workgroup:
//   account  a table a lane, serial over its chunk's inserts: every string's
//            final length through its root, the checks, the push and evict
//            rule; rc, ins_lo, the final state and the table's plan
//   sums     one workgroup: out_ent and each table's first output byte
//   copy     a table a wave: its retained old entries are one contiguous run
//            of the source arena, moved by 16-byte stores aligned to the
//            destination (the loads are unaligned by the residues'
//            difference); their offsets a lane each; a new entry's strings
//            from the decode launch's output through their roots, a string of
//            at most 64 bytes by its lane, a longer one by the wave.
// Everything read from the caller's arrays is clamped (qhuff_tabs_insert_
// impl.h); every store to out_bytes and out_off is cut to out_cap / ent_cap.
#include "qhuff_scan_dev.h"
#include "qhuff_tabs_insert_impl.h"

namespace qhuff {

constexpr uint32_t kInsBlock = 256;

__device__ __forceinline__ ins::Args
ins_args(const ins::Args &a)
{
    ins::Args b = a;
    b.D = a.ent[a.T];
    return b;
}

__global__ __launch_bounds__(kInsBlock) void
qhuff_insapply_account_kernel(ins::Args a0)
{
    const uint64_t c = (uint64_t) blockIdx.x * kInsBlock + threadIdx.x;
    if (c >= a0.T)
        return;
    const ins::Args a = ins_args(a0);
    ins::account(a, (uint32_t) c);
}

// plan[4c + 2], plan[4c + 3] -> sums[2c], sums[2c + 1], their exclusive sums
// in 64 bits, in rounds of a workgroup; out_ent[0 .. T] and the last offset
__global__ __launch_bounds__(kInsBlock) void
qhuff_insapply_sums_kernel(ins::Args a)
{
    __shared__ uint32_t s[kInsBlock];
    const uint32_t tid = threadIdx.x;
    uint64_t ce = 0, cb = 0;
    for (uint64_t c0 = 0; c0 < a.T; c0 += kInsBlock)
    {
        const uint64_t c = c0 + tid;
        const bool live = c < a.T;
        const uint32_t e = live ? a.plan[4 * c + 2] : 0u;
        const uint32_t b = live ? a.plan[4 * c + 3] : 0u;
        // (a round's 256 byte counts may pass 32 bits only in a set the host
        // form refuses; the halves are summed apart)
        uint32_t se, sl, sh;
        const uint32_t xe = block_exclusive<kInsBlock>(e, s, tid, &se);
        const uint32_t xl = block_exclusive<kInsBlock>(b & 0xffffu, s, tid,
                                                       &sl);
        const uint32_t xh = block_exclusive<kInsBlock>(b >> 16, s, tid, &sh);
        if (live)
        {
            a.sums[2 * c] = ce + xe;
            a.sums[2 * c + 1] = cb + xl + ((uint64_t) xh << 16);
            a.out_ent[c] = (uint32_t) (ce + xe);
        }
        ce += se;
        cb += sl + ((uint64_t) sh << 16);
    }
    if (tid == 0)
    {
        a.sums[2ull * a.T] = ce;
        a.sums[2ull * a.T + 1] = cb;
        a.out_ent[a.T] = (uint32_t) ce;
        ins::put_off(a, 2 * ce, cb);
    }
}

// n bytes from src to dst by the wave: the bytes up to dst's next 16-byte
// boundary and behind its last a lane each, the blocks between 16 bytes a
// lane, coalesced
__device__ __forceinline__ void
wave_copy(uint8_t *dst, const uint8_t *src, uint32_t n, uint32_t lane)
{
    uint32_t head = (uint32_t) (-(uintptr_t) dst & 15);
    head = head < n ? head : n;
    if (lane < head)
        dst[lane] = src[lane];
    const uint32_t body = (n - head) >> 4;
    for (uint32_t i = lane; i < body; i += 64)
    {
        const u32x4 v = ((const QH_GLB U4 *) (src + head + 16ull * i))->v;
        *(QH_GLB u32x4 *) (dst + head + 16ull * i) = v;
    }
    const uint32_t done = head + 16 * body;
    if (lane < n - done)
        dst[done + lane] = src[done + lane];
}

// at most 64 bytes by one lane: sixteen at a time, then single bytes
__device__ __forceinline__ void
lane_copy(uint8_t *dst, const uint8_t *src, uint32_t n)
{
    uint32_t k = 0;
    for (; k + 16 <= n; k += 16)
        ((QH_GLB U4 *) (dst + k))->v = ((const QH_GLB U4 *) (src + k))->v;
    for (; k < n; ++k)
        dst[k] = src[k];
}

__global__ __launch_bounds__(kInsBlock) void
qhuff_insapply_copy_kernel(ins::Args a0)
{
    const uint32_t lane = lane_id();
    const uint64_t c64 = (uint64_t) blockIdx.x * (kInsBlock / 64)
                       + threadIdx.x / 64;
    if (c64 >= a0.T)
        return;
    const uint32_t c = __builtin_amdgcn_readfirstlane((uint32_t) c64);
    const ins::Args a = ins_args(a0);
    const ins::Moves m = ins::moves(a, c);
    // the old run and its offsets
    wave_copy(a.out_bytes + m.base, a.bytes + m.sb,
              ins::out_room(a, m.base, m.nb), lane);
    for (uint64_t i = lane; i < 2ull * m.n_old; i += 64)
        ins::put_off(a, 2 * m.oe + i, m.base + ins::old_off(a, m, i));
    // the new strings
    const uint64_t nbase = m.base + m.nb;
    const uint32_t ns = 2 * m.n_new;
    for (uint32_t i0 = 0; i0 < ns; i0 += 64)
    {
        const uint32_t i = i0 + lane;
        const bool on = i < ns;
        const uint32_t s = m.s0 + (on ? i : 0u);
        const uint64_t at = nbase + (a.rel[s] - m.rel0);
        uint32_t n = 0, from = 0;
        if (on)
        {
            ins::put_off(a, 2 * (m.oe + m.n_old) + i, at);
            n = ins::out_room(a, at, ins::new_len(a, m, s));
            from = ins::new_src(a, m, s);
        }
        const bool wide = n > 64;
        if (!wide)
            lane_copy(a.out_bytes + at, a.dec + from, n);
        for (uint64_t w = __builtin_amdgcn_ballot_w64(wide); w; w &= w - 1)
        {
            const uint32_t j = (uint32_t) __builtin_ctzll(w);
            wave_copy(a.out_bytes + read_lane64(at, j),
                      a.dec + read_lane(from, j), read_lane(n, j), lane);
        }
    }
}

hipError_t
launch_insapply_tabs(const ins::Args &a, unsigned step, hipStream_t st,
                     hipEvent_t ev0, hipEvent_t ev1)
{
    if (step == 0)
        return launch_kernel(qhuff_insapply_account_kernel,
                             (uint32_t) (((uint64_t) a.T + kInsBlock - 1)
                                         / kInsBlock),
                             kInsBlock, st, ev0, ev1, a);
    if (step == 1)
        return launch_kernel(qhuff_insapply_sums_kernel, 1, kInsBlock, st, ev0,
                             ev1, a);
    return launch_kernel(qhuff_insapply_copy_kernel,
                         (uint32_t) (((uint64_t) a.T + kInsBlock / 64 - 1)
                                     / (kInsBlock / 64)),
                         kInsBlock, st, ev0, ev1, a);
}

}  // namespace qhuff
