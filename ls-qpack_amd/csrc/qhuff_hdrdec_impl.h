// qhuff_hdrdec_impl.h -- header lists decoded from their descriptors
// (qhuff_decode_headers, include/qhuff.h).  See qhuff_hdrdec.hip.  Here: the
// descriptor load, the static strings, the length limit and the tile policy;
// the decoder, the raw copy, the arena and the stage policy are
// qhuff_decode_impl.h's and qhuff_wire_impl.h's.
#pragma once

#include "qhuff_wire_impl.h"
#include "qhuff_static.h"

namespace qhuff {

static_assert(sizeof(::qhuff_hstr) == 16, "one 128-bit load a descriptor");

// the static table (entry words, offsets, lengths) in this code object's
// constant data, read through the vector cache as qhuff_lookup.hip reads its
// copy
__device__ const StaticTable kHdrStatic = make_static_table();

constexpr uint32_t
static_longest(int what)             // 0 name, 1 value, 2 name + value
{
    uint32_t m = 0;
    for (uint32_t i = 0; i < kStaticNames; ++i)
    {
        const uint32_t nl = kStaticLens[i][0], vl = kStaticLens[i][1];
        const uint32_t v = what == 0 ? nl : what == 1 ? vl : nl + vl;
        m = v > m ? v : m;
    }
    return m;
}
static_assert(static_longest(0) == kStaticNameMax, "qhuff_names.h");
static_assert(static_longest(1) == 53, "the longest static value");
static_assert(static_longest(2) == 76,
              "qhuff_decode_headers_bound: 76 bytes of static text a header");

// descriptor dword 2: huffman, source, kind, static_id (a byte each), masked
// as the contract says: source and kind to a bit, static_id into the table
__device__ __forceinline__ bool hm_static(uint32_t m) { return (m >> 8) & 1; }
__device__ __forceinline__ bool hm_value(uint32_t m) { return (m >> 17) & 1; }
__device__ __forceinline__ uint32_t
hm_id(uint32_t m)
{
    const uint32_t id = m >> 24;
    return id < kStaticNames ? id : kStaticNames - 1;
}

// A tile's descriptors: lane i holds string s + i as loaded.  Lanes >= cnt
// hold the tile's last string; o0() gives them its end.  A STATIC string's
// len counts as 0 whatever it holds.  Every lane issues the load, and nothing
// is computed from it here (WireOffs).
struct HdrOffs
{
    uint32_t pos, len, meta;

    __device__ __forceinline__ void load(const QH_GLB uint32_t *in_off,
                                         uint64_t s, uint32_t cnt)
    {
        const uint32_t lane = lane_id();
        const uint64_t i = s + (lane < cnt ? lane : cnt - 1);
        const u32x4 v = ((const QH_GLB W4 *) in_off)[i].v;
        pos = v.x;
        len = v.y;
        meta = v.z;
    }
    __device__ __forceinline__ uint32_t wlen() const
    {
        return hm_static(meta) ? 0u : len;
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

// a lane's static string: its bytes are [at, at + len) of the table's entry
// words seen as bytes; len = 0: the lane has none (a WIRE string, a lane past
// the tile, an empty static value)
struct StaticStr
{
    uint32_t at, len;
    static __device__ __forceinline__ StaticStr of(uint32_t meta, bool on)
    {
        const uint32_t id = hm_id(meta);
        const bool val = hm_value(meta);
        const uint32_t nl = kHdrStatic.name_len[id], vl = kHdrStatic.val_len[id];
        StaticStr s;
        s.at = 4u * kHdrStatic.at[id] + (val ? nl : 0u);
        s.len = !on ? 0u : val ? vl : nl;
        return s;
    }
    // the four bytes from byte b on (the last word is read twice, not passed)
    __device__ __forceinline__ uint32_t word(uint32_t b) const
    {
        const uint32_t i = (at + b) >> 2;
        const uint32_t j = i + 1 < kStaticWords ? i + 1 : kStaticWords - 1;
        return align_bytes(kHdrStatic.words[j], kHdrStatic.words[i],
                           (at + b) & 3);
    }
};

// every lane's static string into the out stage at dst, n (its len, or 0 for
// a rejected one) bytes, four a step, the whole wave together
__device__ __forceinline__ void
static_to_stage(const StaticStr &s, QH_LDS uint8_t *dst, uint32_t n)
{
    const uint32_t K = wave_max_dpp((n + 3) >> 2);
    for (uint32_t k = 0; k < K; ++k)
        if (4 * k < n)
        {
            const uint32_t w = s.word(4 * k);
            const uint32_t left = n - 4 * k;
            write_bytes(dst + 4 * k, w, left < 3 ? left : 3);
            if (left > 3)
                dst[4 * k + 3] = (uint8_t) (w >> 24);
        }
}

// The limit over a tile's sizes and statuses (max_len != 0): a string longer
// than max_len is rejected; a value -- an odd lane: a tile begins with a
// name -- also when its length plus its name's, the lane before with status
// OK, passes it.  The name's check is its own size alone, so one DPP shift of
// the checked sizes gives every value its name.
__device__ __forceinline__ void
hdr_limit(uint32_t max_len, uint32_t cnt, uint32_t &sz, uint32_t &st)
{
    const uint32_t lane = lane_id();
    const bool valid = lane < cnt;
    const bool over = valid & (sz > max_len);
    st = over ? (uint32_t) QHUFF_DEC_ERROR : st;
    sz = over ? 0u : sz;
    // (a rejected name has sz = 0: it counts for nothing)
    const uint32_t name = all_lanes(wave_shr1(sz));
    const bool both = valid & ((lane & 1) != 0) & (st == QHUFF_DEC_OK)
                    & (name > max_len - sz);
    st = both ? (uint32_t) QHUFF_DEC_ERROR : st;
    sz = both ? 0u : sz;
}

// the sizes and statuses of a tile past the stage: a WIRE string counted in
// global memory, a STATIC one from the table (before the limit)
template <class SM>
__device__ __noinline__ SzSt
hdr_tile_sizes(const uint8_t *in, QH_LDS SM *sm, uint32_t cnt, HdrOffs to)
{
    const bool valid = lane_id() < cnt;
    const bool stat = hm_static(to.meta);
    SzSt o;
    o.sz = 0;
    o.st = QHUFF_DEC_OK;
    if (valid && stat)
        o.sz = StaticStr::of(to.meta, true).len;
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

// A tile past the stages, as wire_slow_tile(): the WIRE strings from the
// arena (staged) or walked / copied again in global memory (unstaged); a
// STATIC string's sz bytes from the table, by its lane, in both cases.  Out
// of line (cold).
template <class SM, class BaseOf>
__device__ __noinline__ uint64_t
hdr_slow_tile(const uint8_t *in, QH_LDS SM *sm, QH_LDS DecWave *wv,
              uint32_t slot0, uint32_t cnt, HdrOffs to, Span sp, uint32_t sz,
              uint32_t st, uint8_t *out, uint32_t *t_off, uint8_t *t_status,
              BaseOf base_of)
{
    const uint32_t lane = lane_id();
    const SlowTile f = SlowTile::begin(sz, base_of);
    uint8_t *dst = out + f.base + f.excl;
    const bool on = lane < cnt && st == QHUFF_DEC_OK && sz;
    const bool stat = hm_static(to.meta);
    if (on && stat)
    {
        const StaticStr s = StaticStr::of(to.meta, true);
        for (uint32_t i = 0; i < sz; ++i)
            ((QH_GLB uint8_t *) dst)[i] = (uint8_t) s.word(i);
    }
    if (sp.staged)
        arena_to_global(wv->arena + slot0, dst, on && !stat ? sz : 0u);
    else
    {
        const bool live = on && !stat;
        const bool huff = wm_huff(to.meta);
        const bool wide = live & !huff & (sz > 64);
        if (live && huff)
        {
            GlobalEmit em{dst, 0};
            wire_walk_glb(in, sm, to.pos, to.len, em);
        }
        else if (live && !wide)
        {
            const QH_GLB uint8_t *s = (const QH_GLB uint8_t *) (in + to.pos);
            for (uint32_t i = 0; i < sz; ++i)
                ((QH_GLB uint8_t *) dst)[i] = s[i];
        }
        for (uint64_t m = __builtin_amdgcn_ballot_w64(wide); m; m &= m - 1)
        {
            const uint32_t j = (uint32_t) __builtin_ctzll(m);
            const QH_GLB uint8_t *s =
                (const QH_GLB uint8_t *) (in + read_lane(to.pos, j));
            QH_GLB uint8_t *d =
                (QH_GLB uint8_t *) (out + f.base + read_lane(f.excl, j));
            const uint32_t nj = read_lane(sz, j);
            for (uint32_t i = lane; i < nj; i += 64)
                d[i] = s[i];
        }
    }
    return f.end<true>(cnt, st, t_off, t_status);
}

// Arena: WirePolicy's slots, unchanged -- fixed (stride kFixStride) iff no
// WIRE string of the tile has more than kFixMaxLen payload bytes, else placed
// by input offset.  A STATIC string takes no part in that comparison and
// uses no slot: it has no wire bytes (o1 == o0), its lane walks no bit and
// copies none, and emit() writes its bytes from the table straight into the
// out stage at the lane's exclusive offset, after the arena's compaction.
// What a static string does cost is out stage: the tile is fast iff total +
// 64 <= kOutCap with the static bytes in the total.
struct HdrPolicy : DecStagePolicy<DecSmem>
{
    static constexpr bool kBig = false;
    static constexpr bool kCoop = false;
    static constexpr uint64_t coop = 0;
    using Offs = HdrOffs;
    uint32_t max_len;                // 0: no limit
    StaticStr ss;                    // this lane's static string (current tile)

    // staged tile: this lane's WIRE string into its arena slot; a STATIC
    // one only sized
    __device__ __forceinline__ void codec(const Offs &to, uint32_t cnt,
                                          const Span &sp, uint32_t *sz,
                                          uint32_t *st)
    {
        const uint32_t lane = lane_id();
        const bool valid = lane < cnt;
        const bool stat = hm_static(to.meta);
        const uint32_t o0 = to.o0(valid), o1 = to.o1();
        const uint32_t hl = o1 - o0;
        place(lane, o0, o1, to.first(), valid, 2, kFixMaxLen);
        ss = StaticStr::of(to.meta, valid & stat);
        const uint32_t rs = (uint32_t) ((uintptr_t) (in + o0) - sp.pa);
        const uint32_t re = (uint32_t) ((uintptr_t) (in + o1) - sp.pa);
        const bool huff = !stat & wm_huff(to.meta);
        int r = 0;
        if (valid)
        {
            // (a raw or static lane walks no bits)
            ArenaEmit em{wv->arena + slot0, wv->arena + slot0, 0};
            r = decode_string(DecLds{wv->in}, 8 * rs, huff ? 8 * re : 8 * rs,
                              sm->win, sm->long2, em);
        }
        const bool raw = valid & !huff;
        if (__builtin_amdgcn_ballot_w64(raw & (hl != 0)))
            wire_raw_copy(wv->in, raw, rs, hl, wv->arena + slot0);
        *sz = stat ? ss.len : raw ? hl : r >= 0 ? (uint32_t) r : 0u;
        *st = r < 0 ? QHUFF_DEC_ERROR : QHUFF_DEC_OK;
        if (max_len)
            hdr_limit(max_len, cnt, *sz, *st);
    }
    // arena -> the (dead) input stage, compacted; then the static strings
    // over whatever the compaction's whole-dword stores left in their bytes
    __device__ __forceinline__ void emit(uint32_t excl, uint32_t sz, uint32_t)
    {
        QH_LDS uint8_t *stage = (QH_LDS uint8_t *) wv->in;
        compact_wave(wv->arena + slot0, stage + excl, ss.len ? 0u : sz);
        wave_sync();
        if (__builtin_amdgcn_ballot_w64(ss.len != 0))
            static_to_stage(ss, stage + excl, ss.len ? sz : 0u);
    }
    __device__ __forceinline__ void slow_size(uint32_t cnt, Offs to, Span,
                                              uint32_t &sz, uint32_t &st)
    {
        const SzSt r = hdr_tile_sizes(in, sm, cnt, to);
        sz = r.sz;
        st = r.st;
        if (max_len)
            hdr_limit(max_len, cnt, sz, st);
    }
    __device__ __forceinline__ void slow_tile(Coord c, uint32_t t, uint32_t cnt,
                                              Offs to, Span sp, uint32_t sz,
                                              uint32_t st, bool,
                                              uint8_t *out, uint32_t *out_off,
                                              uint8_t *status, uint64_t n,
                                              const LookBack &lb)
    {
        const uint64_t s0 = (uint64_t) t * kTS;
        const uint64_t end = hdr_slow_tile(in, sm, wv, slot0, cnt, to, sp, sz,
                                           st, out, out_off + s0, status + s0,
                                           StartedBase{c, lb});
        last_tile_end(c, t, end, out_off, n);
    }
};

}  // namespace qhuff
