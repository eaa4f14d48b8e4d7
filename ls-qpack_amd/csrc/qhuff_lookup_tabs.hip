// qhuff_lookup_tabs.hip -- batched lookup of the headers of many connections,
// each in the static table and among the entries of its own section's table
// of a set (struct qhuff_dyn_tables, include/qhuff.h), and the items of their
// field lines (gfx950).
//
// Reference: qhuff_lookup_dyn.hip's -- lsqpack_enc_encode's lookups for a
// header that is not inserted (lsqpack.c:1671-1930 with index = 0), the
// choice of the line (2033-2125) and the prefix (1267-1298) -- once per
// connection: a set of tables is that many encoders' tables held in one
// arena.  The rule: include/qhuff.h; the source both this file and
// qhuff_dyn_lookup_tabs_cpu run: qhuff_lookup_dyn_impl.h (the index and the
// probe) and qhuff_tabs_impl.h (a section's view of its table).
//
// Three launches, shaped like qhuff_lookup_dyn.hip's.
//
// 1. qhuff_tabs_index_kernel, one entry a lane: ONE pair of indices over all
//    D entries, a slot holding a global ordinal + 1.  The lane finds its
//    entry's table by a binary search of ent (tab_of_entry) rather than from
//    a per-entry table id written by a launch before it: ent is T + 1 words
//    that stay in the vector cache, at most 28 steps beside the entry's two
//    hashes, where the id array would cost D more words of scratch, a launch
//    and a dependent load of its own.  The table's mix is XOR-ed into the
//    entry's first slot, (hash ^ tab_mix(c)) & mask: connections hold the
//    same popular headers, and an entry that every one of T tables holds
//    would otherwise make one probe run of length T that every lookup of it
//    walks.
//
// 2. qhuff_lookup_tabs_kernel: qhuff_lookup_dyn_kernel's frame, copied, as
//    that is a copy of the static one.  Both forms find the lane's section
//    (the table is the section's).  The lane reads sec_tab and forms its
//    section's view (tab_section): the window as GLOBAL ordinals, so that the
//    probe's window filter rejects other tables' entries by ordinal alone and
//    the table the probe reads stays wave-uniform -- the shared offsets with
//    first = 0 and d = D.  Per lane there are the two window edges, the mix,
//    the Base and delta = first - ent[c], which turns a hit back into the
//    table's absolute index for dyn_id, the items and the Required Insert
//    Count word.  Lanes of one wave hold different tables: nothing of a
//    table is taken from another lane, and the segmented maximum and the
//    atomic maximum stay per section, because a section has one table.
//
// 3. qhuff_tabs_prefix_kernel, one section a lane: as qhuff_dyn_prefix_kernel,
//    with max_entries[sec_tab[s]].
//
// Then qhuff_encode_wire's launch and the gather of sec_out run on the
// arrays (qhuff_host.cpp).
#include "qhuff_kernels.h"
#include "qhuff_hash_impl.h"
#include "qhuff_tabs_impl.h"

namespace qhuff {

namespace {

__device__ const StaticTable kStaticTabsDev = make_static_table();

// the shared bytes in global memory (qhuff_lookup_dyn.hip's DynGlb)
struct TabsGlb
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
using DevTabs = DynTab<TabsGlb, GlbWords>;

// all D entries as one table of ordinals (first = 0); wave-uniform
__device__ __forceinline__ DevTabs
dev_tabs(const TabsLookupArgs &a)
{
    DevTabs t;
    t.tb = TabsGlb{glb(a.tab)};
    t.off = glb(a.tab_off);
    t.nv = glb(a.nv);
    t.nm = glb(a.nm);
    t.mask = a.mask;
    t.d = a.D;
    t.first = 0;
    t.t0 = a.D ? t.off[0] : 0;
    t.t1 = a.D ? t.off[2ull * a.D] : 0;
    return t;
}

// section s as the lookup sees it
__device__ __forceinline__ TabSection
section_view(const TabsLookupArgs &a, uint64_t s)
{
    return tab_section(glb(a.ent), glb(a.first), glb(a.max_entries), a.T, a.D,
                       glb(a.sec_tab), glb(a.sec_win), glb(a.sec_base), s);
}

// how many s in [0, m) have sh[s] < x (sh non-decreasing); wave-uniform
__device__ __forceinline__ uint32_t
sections_before_tabs(const QH_GLB uint32_t *sh, uint32_t m, uint64_t x)
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
qhuff_tabs_index_kernel(TabsLookupArgs a)
{
    const GlbWords off = glb(a.tab_off);
    const GlbWords ent = glb(a.ent);
    const TabsGlb tb{glb(a.tab)};
    const uint32_t t0 = off[0], t1 = off[2ull * a.D];
    QH_GLB uint32_t *nv = glb(a.nv), *nm = glb(a.nm);
    auto cas = [](QH_GLB uint32_t *p, uint32_t v) {
        return atomicCAS((uint32_t *) p, 0u, v) == 0u;
    };
    const uint64_t stride = (uint64_t) gridDim.x * 256;
    for (uint64_t k = (uint64_t) blockIdx.x * 256 + threadIdx.x; k < a.D;
            k += stride)
    {
        const uint32_t c = tab_of_entry(ent, a.T, a.D, (uint32_t) k);
        dyn_index_insert(tb, off, (uint32_t) k, t0, t1, nv, nm, a.mask, cas,
                         tab_mix(c));
    }
}

// ENC: the encode form (items, no hashes out); else the lookup form.  Both
// are held to four waves a SIMD, two workgroups a CU.  The encode form as
// qhuff_lookup_dyn_kernel's (101 VGPRs here, no scratch).  The lookup form,
// unlike that kernel's, finds sections and carries its section's view: held
// to six waves a SIMD it fits 80 VGPRs only by spilling two of them to
// scratch inside the tile loop, and five waves a SIMD are two workgroups of
// eight waves all the same, so it takes the lower bound too (DESIGN.md
// section 4 has the registers of both).
template <bool ENC>
__global__ __launch_bounds__(64 * kHashWaves, 4) void
qhuff_lookup_tabs_kernel(TabsLookupArgs a)
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
    const DevTabs tab = dev_tabs(a);

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

        // the two hashes first: the section's view, which only the lookup
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
        // the lane's section s1 - 1 and its view of its table
        uint32_t s1;
        {
            const QH_GLB uint32_t *sh = glb(a.l.sec_hdr);
            const uint32_t m = a.l.m;
            const uint32_t sa = sections_before_tabs(sh, m, s0);
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
            // (within [1, m] whatever sec_hdr holds: the items, sec_tab, the
            // windows and the words of the Required Insert Count stay inside
            // their arrays)
            const uint64_t sx = (uint64_t) sa + c;
            s1 = (uint32_t) (sx < 1 ? 1 : sx > m ? m : sx);
            if (c == 63)
                while (s1 < m && sh[s1] <= j)
                    ++s1;
        }
        const TabSection sec = section_view(a, s1 - 1);

        DynHit hit;
        if (sp_cur.staged)
        {
            const HashLds r{s};
            hit = dyn_lookup(r, o_cur.a - first + skew, o_cur.m - first + skew,
                             o_cur.b - first + skew, h1, h2, kStaticTabsDev,
                             tab, sec.glo, sec.ghi, sec.mix);
        }
        else
        {
            const HashGlb r{glb(a.l.in)};
            hit = dyn_lookup(r, o_cur.a, o_cur.m, o_cur.b, h1, h2,
                             kStaticTabsDev, tab, sec.glo, sec.ghi, sec.mix);
        }
        // (the ordinal back to the lane's table's absolute index)
        hit = tab_hit(hit, sec.delta);
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
                    // consecutive, and a section has one table
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
                const ItemWords it = dyn_line_items(hit, sec.base, nbit);
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
qhuff_tabs_prefix_kernel(TabsLookupArgs a)
{
    const uint64_t n = a.l.n;
    const uint64_t stride = (uint64_t) gridDim.x * 256;
    for (uint64_t s = (uint64_t) blockIdx.x * 256 + threadIdx.x; s < a.l.m;
            s += stride)
    {
        const uint32_t sh = glb(a.l.sec_hdr)[s];
        const uint64_t hdr = sh < n ? sh : n;
        const uint64_t p = 2 * hdr + 2 * s;
        const TabSection sec = section_view(a, s);
        const ItemWords it = dyn_prefix_items(glb(a.ric)[s], sec.base,
                                              sec.max_entries);
        *(QH_GLB u32x4 *) (a.l.items + p) =
            (u32x4){it.w[0], it.w[1], it.w[2], it.w[3]};
        const uint32_t at = glb(a.l.off)[2 * hdr];
        *(QH_GLB u32x2 *) (a.l.str_off + p) = (u32x2){at, at};
    }
}

hipError_t
launch_tabs_index(const TabsLookupArgs &a, hipStream_t st, hipEvent_t ev0,
                  hipEvent_t ev1)
{
    const uint64_t need = ((uint64_t) a.D + 255) / 256;
    const uint32_t grid = (uint32_t) (need < 1024 ? need : 1024);
    return launch_kernel(qhuff_tabs_index_kernel, grid, 256, st, ev0, ev1, a);
}

hipError_t
launch_lookup_tabs(const TabsLookupArgs &a, uint32_t max_grid, hipStream_t st,
                   hipEvent_t ev0, hipEvent_t ev1)
{
    const uint64_t tiles = (a.l.n + kWT - 1) / kWT;
    const uint64_t need = (tiles + kHashWaves - 1) / kHashWaves;
    const uint32_t grid = (uint32_t) (need < max_grid ? need : max_grid);
    return a.l.items
        ? launch_kernel(qhuff_lookup_tabs_kernel<true>, grid, 64 * kHashWaves,
                        st, ev0, ev1, a)
        : launch_kernel(qhuff_lookup_tabs_kernel<false>, grid,
                        64 * kHashWaves, st, ev0, ev1, a);
}

hipError_t
launch_tabs_prefix(const TabsLookupArgs &a, hipStream_t st, hipEvent_t ev0,
                   hipEvent_t ev1)
{
    const uint64_t need = ((uint64_t) a.l.m + 255) / 256;
    const uint32_t grid = (uint32_t) (need < 1024 ? need : 1024);
    return launch_kernel(qhuff_tabs_prefix_kernel, grid, 256, st, ev0, ev1, a);
}

hipError_t
lookup_tabs_occupancy(bool enc, int *blocks_per_cu)
{
    return enc
        ? hipOccupancyMaxActiveBlocksPerMultiprocessor(
              blocks_per_cu, qhuff_lookup_tabs_kernel<true>, 64 * kHashWaves,
              0)
        : hipOccupancyMaxActiveBlocksPerMultiprocessor(
              blocks_per_cu, qhuff_lookup_tabs_kernel<false>, 64 * kHashWaves,
              0);
}

}  // namespace qhuff
