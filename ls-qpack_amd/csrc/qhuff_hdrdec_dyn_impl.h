// qhuff_hdrdec_dyn_impl.h -- header lists decoded from their descriptors with
// the dynamic table's entries as a third string source
// (qhuff_decode_headers_dyn, include/qhuff.h).  See qhuff_hdrdec_dyn.hip.
// Here: the descriptor load with its two source bits, the table strings and
// the tile policy; the static strings and the length limit are
// qhuff_hdrdec_impl.h's, the rest qhuff_decode_impl.h's and
// qhuff_wire_impl.h's.
#pragma once

#include "qhuff_hdrdec_impl.h"

namespace qhuff {

// descriptor dword 2, the source byte masked to two bits: 1 STATIC, 2 DYN,
// 0 and 3 WIRE
__device__ __forceinline__ bool hd_static(uint32_t m) { return ((m >> 8) & 3) == 1; }
__device__ __forceinline__ bool hd_dyn(uint32_t m) { return ((m >> 8) & 3) == 2; }

// HdrOffs with the descriptor's fourth dword: a DYN string's offset in the
// table.  A STATIC or DYN string has no wire bytes whatever its len holds.
struct DynOffs
{
    uint32_t pos, len, meta, instr;

    __device__ __forceinline__ void load(const QH_GLB uint32_t *in_off,
                                         uint64_t s, uint32_t cnt)
    {
        const uint32_t lane = lane_id();
        const uint64_t i = s + (lane < cnt ? lane : cnt - 1);
        const u32x4 v = ((const QH_GLB W4 *) in_off)[i].v;
        pos = v.x;
        len = v.y;
        meta = v.z;
        instr = v.w;
    }
    __device__ __forceinline__ uint32_t wlen() const
    {
        return (hd_static(meta) || hd_dyn(meta)) ? 0u : len;
    }
    __device__ __forceinline__ uint32_t o0(bool valid) const
    {
        return valid ? pos : pos + wlen();
    }
    __device__ __forceinline__ uint32_t o1() const { return pos + wlen(); }
    __device__ __forceinline__ uint32_t first() const { return read_lane(pos, 0); }
    __device__ __forceinline__ uint32_t last() const
    {
        return read_lane(pos + wlen(), 63);
    }
};

// the table's bytes: [dyn, dyn + len), and the address of the last dword of
// the last 16-byte block that holds one of them (no read goes past it)
struct DynBytes
{
    const uint8_t *dyn;
    uint32_t len;

    __device__ __forceinline__ uintptr_t last_dword() const
    {
        return (((uintptr_t) dyn + (len ? len - 1 : 0)) & ~(uintptr_t) 15) + 12;
    }
    // the four bytes from table byte `at` on (at < len), from two aligned
    // dwords; past the last dword that one is read again, its bytes not used
    __device__ __forceinline__ uint32_t word(uint32_t at) const
    {
        const uintptr_t a = (uintptr_t) (dyn + at), a0 = a & ~(uintptr_t) 3;
        const uintptr_t last = last_dword();
        const uintptr_t a1 = a0 + 4 > last ? last : a0 + 4;
        return align_bytes(*(const QH_GLB uint32_t *) a1,
                           *(const QH_GLB uint32_t *) a0, (uint32_t) a & 3);
    }
};

// a lane's table string, clamped into the table: bytes [at, at + len) of it;
// len = 0: the lane has none
struct DynStr
{
    uint32_t at, len;
    static __device__ __forceinline__ DynStr of(const DynOffs &to,
                                                const DynBytes &t, bool on)
    {
        DynStr s;
        s.at = to.instr < t.len ? to.instr : t.len;
        const uint32_t room = t.len - s.at;
        s.len = !on ? 0u : to.len < room ? to.len : room;
        return s;
    }
};

__device__ __forceinline__ void
dyn_put4(QH_LDS uint8_t *dst, uint32_t w, uint32_t left)
{
    write_bytes(dst, w, left < 3 ? left : 3);
    if (left > 3)
        dst[3] = (uint8_t) (w >> 24);
}

// every lane's table string into the out stage at dst, n (its len, or 0 for a
// rejected one) bytes.  A string of at most 64 bytes by its lane, sixteen
// bytes a trip (five aligned dwords in flight); a longer one by the whole
// wave, a dword a lane, coalesced.
__device__ __forceinline__ void
dyn_to_stage(const DynBytes &t, const DynStr &s, QH_LDS uint8_t *dst,
             uint32_t n)
{
    const uint32_t lane = lane_id();
    const bool wide = n > 64;
    const uint32_t K = wave_max_dpp(wide ? 0u : (n + 15) >> 4);
    for (uint32_t k = 0; k < K; ++k)
        if (!wide && 16 * k < n)
        {
            const uint32_t at = s.at + 16 * k, left = n - 16 * k;
            const uintptr_t a = (uintptr_t) (t.dyn + at);
            const uintptr_t a0 = a & ~(uintptr_t) 3, last = t.last_dword();
            uint32_t w[5];
#pragma unroll
            for (int j = 0; j < 5; ++j)
            {
                const uintptr_t aj = a0 + 4 * j;
                w[j] = *(const QH_GLB uint32_t *) (aj > last ? last : aj);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (4u * j < left)
                    dyn_put4(dst + 16 * k + 4 * j,
                             align_bytes(w[j + 1], w[j], (uint32_t) a & 3),
                             left - 4 * j);
        }
    for (uint64_t m = __builtin_amdgcn_ballot_w64(wide); m; m &= m - 1)
    {
        const uint32_t j = (uint32_t) __builtin_ctzll(m);
        const uint32_t at = read_lane(s.at, j), nj = read_lane(n, j);
        QH_LDS uint8_t *d = (QH_LDS uint8_t *) (uintptr_t) read_lane(
            (uint32_t) (uintptr_t) dst, j);
        for (uint32_t i = 4 * lane; i < nj; i += 256)
            dyn_put4(d + i, t.word(at + i), nj - i);
    }
}

// the sizes and statuses of a tile past the stage, as hdr_tile_sizes: a DYN
// string from its descriptor (before the limit)
template <class SM>
__device__ __noinline__ SzSt
dyn_tile_sizes(const uint8_t *in, QH_LDS SM *sm, uint32_t cnt, DynOffs to,
               DynBytes t)
{
    const bool valid = lane_id() < cnt;
    SzSt o;
    o.sz = 0;
    o.st = QHUFF_DEC_OK;
    if (valid && hd_static(to.meta))
        o.sz = StaticStr::of(to.meta, true).len;
    else if (valid && hd_dyn(to.meta))
        o.sz = DynStr::of(to, t, true).len;
    else if (valid)
    {
        o.sz = to.len;
        if (wm_huff(to.meta))
        {
            CountEmit em{0};
            const int r = wire_walk_glb(in, sm, to.pos, to.len, em);
            o.sz = r >= 0 ? (uint32_t) r : 0u;
            o.st = r < 0 ? QHUFF_DEC_ERROR : QHUFF_DEC_OK;
        }
    }
    return o;
}

// A tile past the stages, as hdr_slow_tile(): a DYN string's sz bytes from
// the table to global memory, by its lane when short, by the whole wave when
// longer than 64 bytes.  Out of line (cold).
template <class SM, class BaseOf>
__device__ __noinline__ uint64_t
dyn_slow_tile(const uint8_t *in, QH_LDS SM *sm, QH_LDS DecWave *wv,
              uint32_t slot0, uint32_t cnt, DynOffs to, DynBytes t, Span sp,
              uint32_t sz, uint32_t st, uint8_t *out, uint32_t *t_off,
              uint8_t *t_status, BaseOf base_of)
{
    const uint32_t lane = lane_id();
    const SlowTile f = SlowTile::begin(sz, base_of);
    uint8_t *dst = out + f.base + f.excl;
    const bool on = lane < cnt && st == QHUFF_DEC_OK && sz;
    const bool stat = hd_static(to.meta), dynl = hd_dyn(to.meta);
    const bool wirel = on && !stat && !dynl;
    if (on && stat)
    {
        const StaticStr s = StaticStr::of(to.meta, true);
        for (uint32_t i = 0; i < sz; ++i)
            ((QH_GLB uint8_t *) dst)[i] = (uint8_t) s.word(i);
    }
    // (sz <= the clamped length: the bytes are the table's)
    const uint32_t dat = DynStr::of(to, t, true).at;
    if (on && dynl && sz <= 64)
    {
        const QH_GLB uint8_t *s = (const QH_GLB uint8_t *) (t.dyn + dat);
        for (uint32_t i = 0; i < sz; ++i)
            ((QH_GLB uint8_t *) dst)[i] = s[i];
    }
    if (sp.staged)
        arena_to_global(wv->arena + slot0, dst, wirel ? sz : 0u);
    const bool huff = wm_huff(to.meta);
    const bool glb = wirel && !sp.staged;
    if (glb && huff)
    {
        GlobalEmit em{dst, 0};
        wire_walk_glb(in, sm, to.pos, to.len, em);
    }
    else if (glb && sz <= 64)
    {
        const QH_GLB uint8_t *s = (const QH_GLB uint8_t *) (in + to.pos);
        for (uint32_t i = 0; i < sz; ++i)
            ((QH_GLB uint8_t *) dst)[i] = s[i];
    }
    // the long raw and table strings by the whole wave
    const bool wide = (sz > 64) & ((glb & !huff) | (on & dynl));
    for (uint64_t m = __builtin_amdgcn_ballot_w64(wide); m; m &= m - 1)
    {
        const uint32_t j = (uint32_t) __builtin_ctzll(m);
        const bool dj = read_lane((uint32_t) dynl, j);
        const QH_GLB uint8_t *s = (const QH_GLB uint8_t *)
            (dj ? t.dyn + read_lane(dat, j) : in + read_lane(to.pos, j));
        QH_GLB uint8_t *d =
            (QH_GLB uint8_t *) (out + f.base + read_lane(f.excl, j));
        const uint32_t nj = read_lane(sz, j);
        for (uint32_t i = lane; i < nj; i += 64)
            d[i] = s[i];
    }
    return f.end<true>(cnt, st, t_off, t_status);
}

// HdrPolicy with the third source.  A DYN string, as a STATIC one, has no
// wire bytes, takes no arena slot and walks no bit; its size is its
// descriptor's len (clamped into the table), known before any byte of the
// table is read, and emit() copies its bytes from the table -- gather reads
// of an L2-resident array -- into the out stage at the lane's exclusive
// offset after the arena's compaction.  The tile is fast iff total + 64 <=
// kOutCap with the static and the dynamic bytes in the total.
struct DynPolicy : DecStagePolicy<DecSmem>
{
    static constexpr bool kBig = false;
    static constexpr bool kCoop = false;
    static constexpr uint64_t coop = 0;
    using Offs = DynOffs;
    uint32_t max_len;                // 0: no limit
    DynBytes tab;
    StaticStr ss;                    // this lane's static string (current tile)
    DynStr ds;                       // this lane's table string

    __device__ __forceinline__ void trace_dyn(const Offs &to, uint32_t sz)
    {
#ifdef QH_PATH_TRACE
        tr.dyn = read_lane(wave_incl_scan(hd_dyn(to.meta) ? sz : 0u), 63);
#endif
    }
    // staged tile: this lane's WIRE string into its arena slot; a STATIC or
    // DYN one only sized
    __device__ __forceinline__ void codec(const Offs &to, uint32_t cnt,
                                          const Span &sp, uint32_t *sz,
                                          uint32_t *st)
    {
        const uint32_t lane = lane_id();
        const bool valid = lane < cnt;
        const bool stat = hd_static(to.meta), dynl = hd_dyn(to.meta);
        const uint32_t o0 = to.o0(valid), o1 = to.o1();
        const uint32_t hl = o1 - o0;
        place(lane, o0, o1, to.first(), valid, 2, kFixMaxLen);
        ss = StaticStr::of(to.meta, valid & stat);
        ds = DynStr::of(to, tab, valid & dynl);
        const uint32_t rs = (uint32_t) ((uintptr_t) (in + o0) - sp.pa);
        const uint32_t re = (uint32_t) ((uintptr_t) (in + o1) - sp.pa);
        const bool huff = !stat & !dynl & wm_huff(to.meta);
        int r = 0;
        if (valid)
        {
            // (a raw, static or table lane walks no bits)
            ArenaEmit em{wv->arena + slot0, wv->arena + slot0, 0};
            r = decode_string(DecLds{wv->in}, 8 * rs, huff ? 8 * re : 8 * rs,
                              sm->win, sm->long2, em);
        }
        const bool raw = valid & !huff;
        if (__builtin_amdgcn_ballot_w64(raw & (hl != 0)))
            wire_raw_copy(wv->in, raw, rs, hl, wv->arena + slot0);
        *sz = stat ? ss.len : dynl ? ds.len : raw ? hl
            : r >= 0 ? (uint32_t) r : 0u;
        *st = r < 0 ? QHUFF_DEC_ERROR : QHUFF_DEC_OK;
        if (max_len)
            hdr_limit(max_len, cnt, *sz, *st);
        trace_dyn(to, valid ? *sz : 0u);
    }
    // arena -> the (dead) input stage, compacted; then the static and the
    // table strings over whatever the compaction's whole-dword stores left
    // in their bytes
    __device__ __forceinline__ void emit(uint32_t excl, uint32_t sz, uint32_t)
    {
        QH_LDS uint8_t *stage = (QH_LDS uint8_t *) wv->in;
        const bool own = (ss.len | ds.len) != 0;
        compact_wave(wv->arena + slot0, stage + excl, own ? 0u : sz);
        wave_sync();
        if (__builtin_amdgcn_ballot_w64(ss.len != 0))
            static_to_stage(ss, stage + excl, ss.len ? sz : 0u);
        if (__builtin_amdgcn_ballot_w64(ds.len != 0))
            dyn_to_stage(tab, ds, stage + excl, ds.len ? sz : 0u);
    }
    __device__ __forceinline__ void slow_size(uint32_t cnt, Offs to, Span,
                                              uint32_t &sz, uint32_t &st)
    {
        const SzSt r = dyn_tile_sizes(in, sm, cnt, to, tab);
        sz = r.sz;
        st = r.st;
        if (max_len)
            hdr_limit(max_len, cnt, sz, st);
        trace_dyn(to, sz);
    }
    __device__ __forceinline__ void slow_tile(Coord c, uint32_t t, uint32_t cnt,
                                              Offs to, Span sp, uint32_t sz,
                                              uint32_t st, bool,
                                              uint8_t *out, uint32_t *out_off,
                                              uint8_t *status, uint64_t n,
                                              const LookBack &lb)
    {
        const uint64_t s0 = (uint64_t) t * kTS;
        const uint64_t end = dyn_slow_tile(in, sm, wv, slot0, cnt, to, tab, sp,
                                           sz, st, out, out_off + s0,
                                           status + s0, StartedBase{c, lb});
        last_tile_end(c, t, end, out_off, n);
    }
};

}  // namespace qhuff
