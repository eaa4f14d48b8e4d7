// qhuff_lookup.hip -- batched static-table lookup of headers, and the items
// of their field lines (gfx950).
//
// Reference: the first step of lsqpack_enc_encode for every header
// (lsqpack.c:1671-1715, 1835-1866): XXH32 of the name, XXH32 of the value
// seeded with it, a probe of nameval2id_plus_one / name2id_plus_one
// (lsqpack.c:629-666, 721-764) and a compare of the bytes.  Without the
// dynamic table the answer is the whole encode program: EHA_INDEXED_STAT,
// EHA_LIT_WITH_NAME_STAT or EHA_LIT (lsqpack.c:2033-2039, 2110-2125,
// 2061-2076).
//
// The hash kernel's shape (qhuff_hash.hip; the frame, XXH32 and the readers
// are shared through qhuff_hash_impl.h): one header per lane, a 64-header
// tile per persistent wave, the tile's bytes staged in the wave's LDS region
// with the next tile's in flight, a tile past kHashCap read from global
// memory.  After its two hashes a lane probes and compares
// (qhuff_lookup_impl.h, the source qhuff_static_lookup_cpu runs), reading its
// own bytes from where it hashed them, and writes its outputs.
//
// The static table (2.2 KB of entry words, 0.4 KB of offsets and lengths)
// and the two probe tables (1 KB) are a constant of this code object, read
// through the vector cache: a lane reads one or two probe bytes and, on a
// hit, the candidate's lengths and at most its own bytes' worth of the
// entry, at addresses that differ from lane to lane.  All 3.6 KB stay
// resident in the CU's 32 KB L1 next to the streamed input, which passes
// through it once.  A copy in LDS would fit -- three workgroups of 8 x 6 KB
// stages fill 148 of the CU's 160 KB, three copies would leave 4.7 KB -- but
// it costs a copy loop and a workgroup barrier in a kernel that has neither,
// for reads that are a small part of a header's work and whose latency the
// CU's other waves cover.
//
// Encode form (items != null): lane j also writes the two items of its
// header's field line and their string offsets, behind the two prefix items
// of every section before it: header j of section s at 2j + 2(s + 1).  A
// section's prefix items, at 2 * sec_hdr[s] + 2s, are written by the tile
// that holds header sec_hdr[s] (the last tile for sections that start at n),
// one section a lane, so that empty sections get theirs.  (Sections without
// any header, n = 0, are their prefixes: a kernel of their own.)  A wave finds the
// first section that starts in its tile by a 64-ary search of sec_hdr, every
// lane one probe a step; a lane then finds its own section among the next
// 63 boundaries, which the wave holds one a lane, and walks on in memory
// only past those.
#include "qhuff_kernels.h"
#include "qhuff_hash_impl.h"
#include "qhuff_lookup_impl.h"

namespace qhuff {

__device__ const StaticTable kStaticDev = make_static_table();

// how many s in [0, m) have sh[s] < x (sh non-decreasing); wave-uniform
__device__ __forceinline__ uint32_t
sections_before(const QH_GLB uint32_t *sh, uint32_t m, uint64_t x)
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

// the two prefix items of section s: an 8-bit and a 7-bit integer, both 0
// (Required Insert Count, S + Delta Base: lsqpack.c:1277, 1296), over empty
// strings at the section's first header
__device__ __forceinline__ void
write_prefix(const LookupArgs &a, uint32_t s)
{
    const uint32_t sh = glb(a.sec_hdr)[s];
    const uint64_t hdr = sh < a.n ? sh : a.n;
    const uint64_t p = 2 * hdr + 2ull * s;
    *(QH_GLB u32x4 *) (a.items + p) = (u32x4){0, 8, 0, 7};
    const uint32_t at = glb(a.off)[2 * hdr];
    *(QH_GLB u32x2 *) (a.str_off + p) = (u32x2){at, at};
}

__global__ __launch_bounds__(64 * kHashWaves) void
qhuff_lookup_kernel(LookupArgs a)
{
    __shared__ HashWave sm[kHashWaves];
    const uint32_t lane = lane_id();
    const uint32_t wv = threadIdx.x >> 6;
    const uint64_t nt = (a.n + kWT - 1) / kWT;
    const uint64_t W = (uint64_t) gridDim.x * kHashWaves;
    uint64_t t = (uint64_t) blockIdx.x * kHashWaves + wv;
    if (t >= nt)
        return;
    const QH_GLB uint32_t *off = glb(a.off);
    auto clamp = [&](uint64_t x) { return x < nt ? x : nt - 1; };
    QH_LDS uint32_t *s = (QH_LDS uint32_t *) sm[wv].s;

    HashOffs o_cur, o_nxt, o_nn;
    o_cur.load(off, t, a.n, true);
    Span sp_cur = tile_span(a.in, o_cur.first(), o_cur.last(), kHashCap);
    Chunks<kHashNch> ch;
    ch.load(sp_cur);
    o_nxt.load(off, clamp(t + W), a.n, true);
    for (;;)
    {
        __builtin_amdgcn_s_waitcnt(0x0f70);           // vmcnt(0)
        if (sp_cur.staged)
            ch.store<false>((QH_LDS u32x4 *) s, sp_cur.n16);
        wave_sync();
        const Span sp_nxt = tile_span(a.in, o_nxt.first(), o_nxt.last(),
                                      kHashCap);
        if (t + W < nt)
            ch.load(sp_nxt);
        o_nn.load(off, clamp(t + 2 * W), a.n, true);

        uint32_t h1, h2;
        StaticHit hit;
        const uint32_t first = o_cur.first();
        if (sp_cur.staged)
        {
            // byte index of input offset x in the stage: x - first + skew
            const uint32_t skew = (uint32_t) ((uintptr_t) (a.in + first)
                                              - sp_cur.pa);
            const HashLds r{s};
            const uint32_t ra = o_cur.a - first + skew,
                           rm = o_cur.m - first + skew,
                           rb = o_cur.b - first + skew;
            h1 = xxh32(r, ra, rm - ra, kXxhSeed);
            h2 = xxh32(r, rm, rb - rm, h1);
            hit = static_lookup(r, ra, rm, rb, h1, h2, kStaticDev);
        }
        else
        {
            const HashGlb r{glb(a.in)};
            h1 = xxh32(r, o_cur.a, o_cur.m - o_cur.a, kXxhSeed);
            h2 = xxh32(r, o_cur.m, o_cur.b - o_cur.m, h1);
            hit = static_lookup(r, o_cur.a, o_cur.m, o_cur.b, h1, h2,
                                kStaticDev);
        }
        const uint64_t s0 = t * kWT;
        const uint32_t cnt = o_cur.cnt;
        const uint32_t li = lane < cnt ? lane : cnt - 1;
        const uint64_t j = s0 + li;
        if (lane < cnt)
        {
            if (a.h1)
                glb(a.h1)[j] = h1;
            if (a.h2)
                glb(a.h2)[j] = h2;
            if (a.kind)
                glb(a.kind)[j] = (uint8_t) hit.kind;
            if (a.id)
                glb(a.id)[j] = (uint8_t) hit.id;
        }
        if (a.items)
        {
            const QH_GLB uint32_t *sh = glb(a.sec_hdr);
            // sections [sa, sb) start in this tile
            const uint32_t sa = sections_before(sh, a.m, s0);
            const uint64_t vi = (uint64_t) sa + lane;
            const uint32_t v = sh[vi < a.m ? vi : a.m];
            // s1 - 1: lane's section, the last that starts at or before j
            // (s1 = sa + how many of v[0 .. 62] are <= j, then on in memory)
            uint32_t c = 0;
#pragma unroll
            for (uint32_t step = 32; step; step >>= 1)
            {
                const uint32_t x = (uint32_t) __builtin_amdgcn_ds_bpermute(
                    (int) (4 * (c + step - 1)), (int) v);
                c += x <= j ? step : 0;
            }
            // (within [1, m] whatever sec_hdr holds: the items stay inside
            // their arrays)
            uint64_t s1 = (uint64_t) sa + c;
            s1 = s1 < 1 ? 1 : s1 > a.m ? a.m : s1;
            if (c == 63)
                while (s1 < a.m && sh[s1] <= j)
                    ++s1;
            const bool last = s0 + cnt == a.n;
            const uint32_t sb = last ? a.m : read_lane((uint32_t) s1, cnt - 1);
            for (uint64_t k = (uint64_t) sa + lane; k < sb; k += 64)
                write_prefix(a, (uint32_t) k);
            if (lane < cnt)
            {
                const uint32_t nbit = a.hflags
                    ? glb(a.hflags)[j] & QHUFF_HDR_NEVER_INDEX : 0;
                // {ival, int_bits | int_first << 8 | str_bits << 16 |
                //  str_first << 24} of the line's two items
                u32x4 it;
                if (hit.kind == QHUFF_LINE_INDEXED)
                    it = (u32x4){hit.id, 6u | 0xC0u << 8, 0, 0};
                else if (hit.kind == QHUFF_LINE_NAMEREF)
                    it = (u32x4){hit.id, 4u | (0x50u | nbit << 5) << 8, 0,
                                 7u << 16};
                else
                    it = (u32x4){0, 3u << 16 | (0x20u | nbit << 4) << 24, 0,
                                 7u << 16};
                const uint64_t p = 2 * j + 2 * s1;
                *(QH_GLB u32x4 *) (a.items + p) = it;
                *(QH_GLB u32x2 *) (a.str_off + p) = (u32x2){o_cur.a, o_cur.m};
                if (last && lane == cnt - 1)
                    glb(a.str_off)[2 * a.n + 2ull * a.m] = o_cur.b;
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

hipError_t
launch_lookup(const LookupArgs &a, uint32_t max_grid, hipStream_t st,
              hipEvent_t ev0, hipEvent_t ev1)
{
    const uint64_t tiles = (a.n + kWT - 1) / kWT;
    const uint64_t need = (tiles + kHashWaves - 1) / kHashWaves;
    const uint32_t grid = (uint32_t) (need < max_grid ? need : max_grid);
    return launch_kernel(qhuff_lookup_kernel, grid, 64 * kHashWaves, st, ev0,
                         ev1, a);
}

// the sections' ends from the items' offsets: section s begins with item
// 2 * sec_hdr[s] + 2s
__global__ __launch_bounds__(256) void
qhuff_secout_kernel(const uint32_t *item_off, const uint32_t *sec_hdr,
                    uint32_t m, uint64_t n, uint32_t *sec_out)
{
    const uint64_t stride = (uint64_t) gridDim.x * blockDim.x;
    for (uint64_t s = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
            s <= m; s += stride)
    {
        const uint32_t sh = sec_hdr[s];
        const uint64_t hdr = sh < n ? sh : n;
        sec_out[s] = item_off[2 * hdr + 2 * s];
    }
}

// m sections without a header: m prefixes
__global__ __launch_bounds__(256) void
qhuff_empty_sections_kernel(uint32_t m, uint8_t *out, uint32_t *sec_out)
{
    const uint64_t stride = (uint64_t) gridDim.x * blockDim.x;
    for (uint64_t s = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
            s <= m; s += stride)
    {
        sec_out[s] = (uint32_t) (2 * s);
        if (s < m)
            out[2 * s] = out[2 * s + 1] = 0;
    }
}

hipError_t
launch_empty_sections(uint32_t m, uint8_t *out, uint32_t *sec_out,
                      hipStream_t st)
{
    const uint64_t need = ((uint64_t) m + 256) / 256;
    const uint32_t grid = (uint32_t) (need < 1024 ? need : 1024);
    hipLaunchKernelGGL(qhuff_empty_sections_kernel, dim3(grid), dim3(256), 0,
                       st, m, out, sec_out);
    return hipGetLastError();
}

hipError_t
launch_secout(const uint32_t *item_off, const uint32_t *sec_hdr, uint32_t m,
              uint64_t n, uint32_t *sec_out, hipStream_t st)
{
    const uint64_t need = ((uint64_t) m + 256) / 256;
    const uint32_t grid = (uint32_t) (need < 1024 ? need : 1024);
    hipLaunchKernelGGL(qhuff_secout_kernel, dim3(grid), dim3(256), 0, st,
                       item_off, sec_hdr, m, n, sec_out);
    return hipGetLastError();
}

}  // namespace qhuff
