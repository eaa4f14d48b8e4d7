// qhuff_lookup_dyn.hip -- batched lookup of headers in the static table and
// among the dynamic table's entries, and the items of their field lines
// (gfx950).
//
// Reference: lsqpack_enc_encode's lookups for a header that is not inserted
// (lsqpack.c:1671-1930 with index = 0): after the static probes of
// qhuff_lookup.hip, the walk of the two bucket lists over the dynamic
// entries (1738-1902), then the choice of the line (2033-2125) and, per
// section, the prefix (1267-1298).  The rule: include/qhuff.h; the source
// both this file and qhuff_dyn_lookup_cpu run: qhuff_lookup_dyn_impl.h.
//
// Three launches.
//
// 1. qhuff_dyn_index_kernel, one entry a lane: hashes the entry as a header
//    is hashed and claims a slot in each of the two indices with a 32-bit
//    compare-and-swap (the slots were cleared on the stream).
//
// 2. qhuff_lookup_dyn_kernel: qhuff_lookup_kernel's frame, copied -- one
//    header a lane, a 64-header tile per persistent wave, the tile's bytes
//    staged in the wave's LDS region with the next tile's in flight, a tile
//    past kHashCap read from global memory.  After the static probes a lane
//    walks the index's probe runs and compares its bytes with the entry's in
//    the table, read through the vector cache like the static table: a
//    typical table is 4-16 KB, its indices a few KB, next to 3.6 KB of static
//    table in a 32 KB L1.  (No copy in LDS: three workgroups of 8 x 6 KB
//    stages leave 12 KB a CU.)
//    Encode form (items != null): a lane finds its section before it looks
//    up, since the window and the Base are the section's; it writes its
//    line's two items with that Base.  A section's Required Insert Count is
//    1 + the largest index its lines named; the lines of one section may lie
//    in any tiles, so the wave reduces its lanes' indices by section
//    (one DPP maximum when the tile lies in one section, else a segmented
//    maximum over ds_bpermute) and one lane per (tile, section) does an
//    atomic maximum on the section's word.  Maximum does not depend on the
//    order: the result is deterministic.
//
// 3. qhuff_dyn_prefix_kernel, one section a lane: the two prefix items from
//    that word, the section's Base and max_entries, at 2 * sec_hdr[s] + 2s
//    over empty strings at the section's first header -- empty sections and
//    sections that start at n included.
//
// Then qhuff_encode_wire's launch and the gather of sec_out run on the
// arrays (qhuff_host.cpp).
#include "qhuff_kernels.h"
#include "qhuff_hash_impl.h"
#include "qhuff_lookup_dyn_impl.h"

namespace qhuff {

namespace {

__device__ const StaticTable kStaticDynDev = make_static_table();

// the table's bytes in global memory: HashGlb with a word as one unaligned
// dword load (four bytes of the string itself: nothing outside it is touched)
struct DynGlb
{
    const QH_GLB uint8_t *p;
    __device__ __forceinline__ uint32_t byte(uint32_t i) const { return p[i]; }
    __device__ __forceinline__ uint32_t word(uint32_t i) const
    {
        return ((const QH_GLB U1 *) (p + i))->v;
    }
    __device__ __forceinline__ void stripe(uint32_t i, uint32_t w[4]) const
    {
        w[0] = word(i);
        w[1] = word(i + 4);
        w[2] = word(i + 8);
        w[3] = word(i + 12);
    }
};

using GlbWords = const QH_GLB uint32_t *;
using DevTab = DynTab<DynGlb, GlbWords>;

// the table as device code reads it; t0 / t1 are loaded once (d != 0)
__device__ __forceinline__ DevTab
dev_tab(const DynLookupArgs &a)
{
    DevTab t;
    t.tb = DynGlb{glb(a.tab)};
    t.off = glb(a.tab_off);
    t.nv = glb(a.nv);
    t.nm = glb(a.nm);
    t.mask = a.mask;
    t.d = a.d;
    t.first = a.first;
    t.t0 = a.d ? t.off[0] : 0;
    t.t1 = a.d ? t.off[2ull * a.d] : 0;
    return t;
}

// section s's window and Base (encode form)
__device__ __forceinline__ void
section_view(const DynLookupArgs &a, uint64_t s, DynRange *w, uint32_t *base)
{
    if (a.sec_win)
        *w = dyn_window(glb(a.sec_win)[2 * s], glb(a.sec_win)[2 * s + 1],
                        a.first, a.d, a.max_entries);
    else
        *w = dyn_window(a.win_lo, a.win_hi, a.first, a.d, a.max_entries);
    *base = a.sec_base ? dyn_base(glb(a.sec_base)[s], a.first, a.d) : w->hi;
}

// how many s in [0, m) have sh[s] < x (sh non-decreasing); wave-uniform
__device__ __forceinline__ uint32_t
sections_before_dyn(const QH_GLB uint32_t *sh, uint32_t m, uint64_t x)
{
    if (x == 0)
        return 0;
    uint64_t lo = 0, hi = m;             // the answer lies in [lo, hi]
    while (hi > lo)
    {
        const uint64_t step = (hi - lo + 63) / 64;
        const uint64_t idx = lo + lane_id() * step;
        const bool p = idx < hi && sh[idx] < x;
        const uint32_t c = (uint32_t) __builtin_popcountll(
            __builtin_amdgcn_ballot_w64(p));
        if (c == 0)
            break;
        const uint64_t top = lo + c * step;
        lo += (c - 1) * step + 1;
        hi = top < hi ? top : hi;
    }
    return (uint32_t) lo;
}

// lane i's v from lane i - k (unspecified for i < k)
__device__ __forceinline__ uint32_t
lane_up(uint32_t v, uint32_t k)
{
    return (uint32_t) __builtin_amdgcn_ds_bpermute(
        (int) (4 * ((lane_id() - k) & 63)), (int) v);
}

}  // namespace

__global__ __launch_bounds__(256) void
qhuff_dyn_index_kernel(DynLookupArgs a)
{
    const GlbWords off = glb(a.tab_off);
    const DynGlb tb{glb(a.tab)};
    const uint32_t t0 = off[0], t1 = off[2ull * a.d];
    QH_GLB uint32_t *nv = glb(a.nv), *nm = glb(a.nm);
    auto cas = [](QH_GLB uint32_t *p, uint32_t v) {
        return atomicCAS((uint32_t *) p, 0u, v) == 0u;
    };
    const uint64_t stride = (uint64_t) gridDim.x * 256;
    for (uint64_t k = (uint64_t) blockIdx.x * 256 + threadIdx.x; k < a.d;
            k += stride)
        dyn_index_insert(tb, off, (uint32_t) k, t0, t1, nv, nm, a.mask, cas);
}

// ENC: the encode form (items, sections, no hashes out); else the lookup
// form.  The lookup form is held to qhuff_lookup_kernel's six waves a SIMD
// (three workgroups a CU, what the LDS allows), which it meets in 80 VGPRs
// with nothing spilled.  The encode form is not: held to six it spills 9
// VGPRs to scratch inside the tile loop, so it is left at 100 VGPRs, four
// waves a SIMD and no scratch.
template <bool ENC>
__global__ __launch_bounds__(64 * kHashWaves, ENC ? 4 : 6) void
qhuff_lookup_dyn_kernel(DynLookupArgs a)
{
    __shared__ HashWave sm[kHashWaves];
    const uint32_t lane = lane_id();
    const uint32_t wv = threadIdx.x >> 6;
    const uint64_t n = a.l.n;
    const uint64_t nt = (n + kWT - 1) / kWT;
    const uint64_t W = (uint64_t) gridDim.x * kHashWaves;
    uint64_t t = (uint64_t) blockIdx.x * kHashWaves + wv;
    if (t >= nt)
        return;
    const QH_GLB uint32_t *off = glb(a.l.off);
    auto clamp = [&](uint64_t x) { return x < nt ? x : nt - 1; };
    QH_LDS uint32_t *s = (QH_LDS uint32_t *) sm[wv].s;
    const DevTab tab = dev_tab(a);

    HashOffs o_cur, o_nxt, o_nn;
    o_cur.load(off, t, n, true);
    Span sp_cur = tile_span(a.l.in, o_cur.first(), o_cur.last(), kHashCap);
    Chunks<kHashNch> ch;
    ch.load(sp_cur);
    o_nxt.load(off, clamp(t + W), n, true);
    for (;;)
    {
        __builtin_amdgcn_s_waitcnt(0x0f70);           // vmcnt(0)
        if (sp_cur.staged)
            ch.store<false>((QH_LDS u32x4 *) s, sp_cur.n16);
        wave_sync();
        const Span sp_nxt = tile_span(a.l.in, o_nxt.first(), o_nxt.last(),
                                      kHashCap);
        if (t + W < nt)
            ch.load(sp_nxt);
        o_nn.load(off, clamp(t + 2 * W), n, true);

        // the two hashes first: the section's window, which only the lookup
        // needs, is not held across them
        uint32_t h1, h2;
        const uint32_t first = o_cur.first();
        // byte index of input offset x in the stage: x - first + skew
        const uint32_t skew = (uint32_t) ((uintptr_t) (a.l.in + first)
                                          - sp_cur.pa);
        if (sp_cur.staged)
        {
            const HashLds r{s};
            const uint32_t ra = o_cur.a - first + skew,
                           rm = o_cur.m - first + skew,
                           rb = o_cur.b - first + skew;
            h1 = xxh32(r, ra, rm - ra, kXxhSeed);
            h2 = xxh32(r, rm, rb - rm, h1);
        }
        else
        {
            const HashGlb r{glb(a.l.in)};
            h1 = xxh32(r, o_cur.a, o_cur.m - o_cur.a, kXxhSeed);
            h2 = xxh32(r, o_cur.m, o_cur.b - o_cur.m, h1);
        }

        const uint64_t s0 = t * kWT;
        const uint32_t cnt = o_cur.cnt;
        const uint32_t li = lane < cnt ? lane : cnt - 1;
        const uint64_t j = s0 + li;
        // the lane's section s1 - 1 (encode form), its window and its Base
        uint32_t s1 = 0;
        DynRange win;
        uint32_t base;
        if (ENC)
        {
            const QH_GLB uint32_t *sh = glb(a.l.sec_hdr);
            const uint32_t m = a.l.m;
            const uint32_t sa = sections_before_dyn(sh, m, s0);
            const uint64_t vi = (uint64_t) sa + lane;
            const uint32_t v = sh[vi < m ? vi : m];
            // s1 = sa + how many of v[0 .. 62] are <= j, then on in memory
            uint32_t c = 0;
#pragma unroll
            for (uint32_t step = 32; step; step >>= 1)
            {
                const uint32_t x = (uint32_t) __builtin_amdgcn_ds_bpermute(
                    (int) (4 * (c + step - 1)), (int) v);
                c += x <= j ? step : 0;
            }
            // (within [1, m] whatever sec_hdr holds: the items, the windows
            // and the words of the Required Insert Count stay inside their
            // arrays)
            const uint64_t sx = (uint64_t) sa + c;
            s1 = (uint32_t) (sx < 1 ? 1 : sx > m ? m : sx);
            if (c == 63)
                while (s1 < m && sh[s1] <= j)
                    ++s1;
            section_view(a, s1 - 1, &win, &base);
        }
        else
        {
            win = dyn_window(a.win_lo, a.win_hi, a.first, a.d, a.max_entries);
            base = win.hi;
        }

        DynHit hit;
        if (sp_cur.staged)
        {
            const HashLds r{s};
            hit = dyn_lookup(r, o_cur.a - first + skew, o_cur.m - first + skew,
                             o_cur.b - first + skew, h1, h2, kStaticDynDev,
                             tab, win.lo, win.hi);
        }
        else
        {
            const HashGlb r{glb(a.l.in)};
            hit = dyn_lookup(r, o_cur.a, o_cur.m, o_cur.b, h1, h2,
                             kStaticDynDev, tab, win.lo, win.hi);
        }
        if (lane < cnt)
        {
            if (!ENC && a.l.h1)
                glb(a.l.h1)[j] = h1;
            if (!ENC && a.l.h2)
                glb(a.l.h2)[j] = h2;
            if (a.l.kind)
                glb(a.l.kind)[j] = (uint8_t) hit.kind;
            if (a.l.id)
                glb(a.l.id)[j] = (uint8_t) hit.id;
            if (a.dyn_id)
                glb(a.dyn_id)[j] = hit.dyn;
        }
        if (ENC)
        {
            // abs + 1 of the lane's reference, 0: none (a lane past cnt
            // repeats lane cnt - 1's header: the same section, the same value)
            uint32_t ref = hit.dyn + 1;
            if (__builtin_amdgcn_ballot_w64(ref != 0))
            {
                const uint32_t sl = s1;
                bool tail;
                if (read_lane(sl, 0) == read_lane(sl, 63))
                {
                    ref = wave_max_dpp(ref);
                    tail = lane == 63;
                }
                else
                {
                    // segmented inclusive maximum: a section's lanes are
                    // consecutive
#pragma unroll
                    for (uint32_t k = 1; k < 64; k <<= 1)
                    {
                        const uint32_t ov = lane_up(ref, k);
                        const uint32_t os = lane_up(sl, k);
                        if (lane >= k && os == sl && ov > ref)
                            ref = ov;
                    }
                    const uint32_t ns = (uint32_t) __builtin_amdgcn_ds_bpermute(
                        (int) (4 * ((lane + 1) & 63)), (int) sl);
                    tail = lane == 63 || ns != sl;
                }
                if (tail && ref)
                    atomicMax(a.ric + (s1 - 1u), ref);
            }
            if (lane < cnt)
            {
                const uint32_t nbit = a.l.hflags
                    ? glb(a.l.hflags)[j] & QHUFF_HDR_NEVER_INDEX : 0;
                const ItemWords it = dyn_line_items(hit, base, nbit);
                const uint64_t p = 2 * j + 2ull * s1;
                *(QH_GLB u32x4 *) (a.l.items + p) =
                    (u32x4){it.w[0], it.w[1], it.w[2], it.w[3]};
                *(QH_GLB u32x2 *) (a.l.str_off + p) =
                    (u32x2){o_cur.a, o_cur.m};
                if (s0 + cnt == n && lane == cnt - 1)
                    glb(a.l.str_off)[2 * n + 2ull * a.l.m] = o_cur.b;
            }
        }
        wave_sync();
        t += W;
        if (t >= nt)
            break;
        o_cur = o_nxt;
        o_nxt = o_nn;
        sp_cur = sp_nxt;
    }
}

__global__ __launch_bounds__(256) void
qhuff_dyn_prefix_kernel(DynLookupArgs a)
{
    const uint64_t n = a.l.n;
    const uint64_t stride = (uint64_t) gridDim.x * 256;
    for (uint64_t s = (uint64_t) blockIdx.x * 256 + threadIdx.x; s < a.l.m;
            s += stride)
    {
        const uint32_t sh = glb(a.l.sec_hdr)[s];
        const uint64_t hdr = sh < n ? sh : n;
        const uint64_t p = 2 * hdr + 2 * s;
        DynRange win;
        uint32_t base;
        section_view(a, s, &win, &base);
        const ItemWords it = dyn_prefix_items(glb(a.ric)[s], base,
                                              a.max_entries);
        *(QH_GLB u32x4 *) (a.l.items + p) =
            (u32x4){it.w[0], it.w[1], it.w[2], it.w[3]};
        const uint32_t at = glb(a.l.off)[2 * hdr];
        *(QH_GLB u32x2 *) (a.l.str_off + p) = (u32x2){at, at};
    }
}

hipError_t
launch_dyn_index(const DynLookupArgs &a, hipStream_t st, hipEvent_t ev0,
                 hipEvent_t ev1)
{
    const uint64_t need = ((uint64_t) a.d + 255) / 256;
    const uint32_t grid = (uint32_t) (need < 1024 ? need : 1024);
    return launch_kernel(qhuff_dyn_index_kernel, grid, 256, st, ev0, ev1, a);
}

hipError_t
launch_lookup_dyn(const DynLookupArgs &a, uint32_t max_grid, hipStream_t st,
                  hipEvent_t ev0, hipEvent_t ev1)
{
    const uint64_t tiles = (a.l.n + kWT - 1) / kWT;
    const uint64_t need = (tiles + kHashWaves - 1) / kHashWaves;
    const uint32_t grid = (uint32_t) (need < max_grid ? need : max_grid);
    return a.l.items
        ? launch_kernel(qhuff_lookup_dyn_kernel<true>, grid, 64 * kHashWaves,
                        st, ev0, ev1, a)
        : launch_kernel(qhuff_lookup_dyn_kernel<false>, grid, 64 * kHashWaves,
                        st, ev0, ev1, a);
}

hipError_t
launch_dyn_prefix(const DynLookupArgs &a, hipStream_t st, hipEvent_t ev0,
                  hipEvent_t ev1)
{
    const uint64_t need = ((uint64_t) a.l.m + 255) / 256;
    const uint32_t grid = (uint32_t) (need < 1024 ? need : 1024);
    return launch_kernel(qhuff_dyn_prefix_kernel, grid, 256, st, ev0, ev1, a);
}

hipError_t
lookup_dyn_occupancy(bool enc, int *blocks_per_cu)
{
    return enc
        ? hipOccupancyMaxActiveBlocksPerMultiprocessor(
              blocks_per_cu, qhuff_lookup_dyn_kernel<true>, 64 * kHashWaves, 0)
        : hipOccupancyMaxActiveBlocksPerMultiprocessor(
              blocks_per_cu, qhuff_lookup_dyn_kernel<false>, 64 * kHashWaves,
              0);
}

}  // namespace qhuff
