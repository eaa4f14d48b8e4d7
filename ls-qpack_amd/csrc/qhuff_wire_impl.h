// qhuff_wire_impl.h -- literals decoded where they lie in QPACK wire data
// (qhuff_decode_wire, include/qhuff.h).  See qhuff_wire.hip.  Here: the
// descriptor loads, the raw copy, the length limit and the tile policy; the
// decoder, the sources, the emitters, the arena and the stage policy are
// qhuff_decode_impl.h's.
#pragma once

#include "qhuff_decode_impl.h"
#include "qhuff_names.h"

namespace qhuff {

static_assert(sizeof(::qhuff_literal) == 16, "one 128-bit load a descriptor");

// descriptor dword 2: huffman, prefix_bits, kind, hdr_len (a byte each)
__device__ __forceinline__ bool wm_huff(uint32_t m) { return (m & 0xff) != 0; }
__device__ __forceinline__ uint32_t wm_kind(uint32_t m) { return (m >> 16) & 0xff; }
__device__ __forceinline__ uint32_t wm_hdr(uint32_t m) { return m >> 24; }

// dword-aligned views of a descriptor (the array needs its type's alignment
// only: 4 bytes)
struct __attribute__((packed, aligned(4))) W4 { u32x4 v; };
typedef uint32_t u32x3 __attribute__((ext_vector_type(3)));
struct __attribute__((packed, aligned(4))) W3 { u32x3 v; };

// A tile's descriptors: lane i holds literal s + i as loaded -- pos, len,
// the four bytes, instr -- and len, bytes and instr of the literal before
// it (the batch's first literal: its own; only a VALUE literal looks at
// them, for a NAME, and it is no NAME).  Lanes >= cnt hold the tile's last
// literal; o0() gives them its end, as TileOffs gives in_off[s + cnt].
// Every lane issues both loads, and nothing is computed from them here:
// load() is called a codec before the values are used (qhuff_pipeline.h).
// s0: the tile's first literal (wave-uniform).
struct WireOffs
{
    uint32_t pos, len, meta, instr;
    uint32_t p_len, p_meta, p_instr;
    uint32_t s0;

    __device__ __forceinline__ void load(const QH_GLB uint32_t *in_off,
                                         uint64_t s, uint32_t cnt)
    {
        const uint32_t lane = lane_id();
        const uint64_t i = s + (lane < cnt ? lane : cnt - 1);
        const u32x4 v = ((const QH_GLB W4 *) in_off)[i].v;
        const u32x3 p =
            ((const QH_GLB W3 *) (in_off + 4 * (i ? i - 1 : 0) + 1))->v;
        pos = v.x;
        len = v.y;
        meta = v.z;
        instr = v.w;
        p_len = p.x;
        p_meta = p.y;
        p_instr = p.z;
        s0 = (uint32_t) s;
    }
    __device__ __forceinline__ uint32_t o0(bool valid) const
    {
        return valid ? pos : pos + len;
    }
    __device__ __forceinline__ uint32_t o1() const { return pos + len; }
    __device__ __forceinline__ uint32_t first() const { return read_lane(pos, 0); }
    __device__ __forceinline__ uint32_t last() const
    {
        return read_lane(pos + len, 63);
    }
};

// One Huffman literal walked in global memory by its lane (decode_string
// over DecGlb: no dword past its last byte is read).  Returns as
// decode_string.
template <class SM, class Emit>
__device__ __forceinline__ int
wire_walk_glb(const uint8_t *in, QH_LDS SM *sm, uint32_t pos, uint32_t len,
              Emit &em)
{
    const uintptr_t a = (uintptr_t) (in + pos);
    const uintptr_t pa = a & ~(uintptr_t) 15;
    const uint32_t rs = (uint32_t) (a - pa);
    const DecGlb src{(const QH_GLB uint32_t *) pa, 8 * (rs + len)};
    return decode_string(src, 8 * rs, 8 * (rs + len), sm->win, sm->long2, em);
}

// the static table's name lengths (qhuff_names.h) in the code object's
// constant data
struct WireNames
{
    uint8_t v[(kStaticNames + 3) & ~3u];
};
constexpr WireNames
wire_names()
{
    WireNames t{};
    for (uint32_t i = 0; i < kStaticNames; ++i)
        t.v[i] = kStaticNameLen[i];
    return t;
}
__device__ const WireNames kWireNames = wire_names();

// field_ref_name_len (qhuff_frames.cpp) on the device: the static-table
// name's length of a VALUE literal whose instruction is 01NT with T = 1 and
// a 4-bit-prefix index (lsqpack_dec_int24's rules: qhuff_frames.cpp
// dec_int / dec_int24), or 0.  Reads the instruction bytes
// [instr, pos - hdr_len).
__device__ __forceinline__ uint32_t
wire_ref_name_len(const uint8_t *in, uint32_t pos, uint32_t meta,
                  uint32_t instr)
{
    const uint32_t hdr = wm_hdr(meta);
    if (wm_kind(meta) != QHUFF_LIT_VALUE || hdr > pos
            || (uint64_t) instr + 1 > pos - hdr)
        return 0;
    const QH_GLB uint8_t *p = (const QH_GLB uint8_t *) (in + instr);
    const QH_GLB uint8_t *const end = (const QH_GLB uint8_t *) (in + (pos - hdr));
    const uint32_t b0 = *p++;
    if ((b0 & 0xd0) != 0x50)
        return 0;
    uint64_t v = b0 & 15;
    if (v == 15)
    {
        uint32_t M = 0, B;
        do
        {
            if (p >= end)
                return 0;
            B = *p++;
            v += (uint64_t) (B & 0x7f) << M;
            M += 7;
        } while ((B & 0x80) && M < 64);
        if (!(M <= 63 || (M == 70 && B <= 1 && (v & (1ull << 63)))))
            return 0;
    }
    return v < kStaticNames ? (uint32_t) kWireNames.v[v] : 0u;
}

struct WireLimit
{
    const ::qhuff_literal *lits;     // the descriptors (the rare path reloads)
    uint32_t max_len;                // 0: none
};

// The limit's rare path (out of line): some VALUE literal of the tile is
// within its name's upper bound of max_len, so the name's exact length
// decides.  As qhuff_decode_literals_ex counts it: the decoded length of the
// literal directly before, when that is a NAME of the same instruction with
// status OK -- lane - 1's size, or, for lane 0, a counting walk of the
// previous tile's last literal in global memory -- else the static-table
// name the instruction refers to, else nothing.  sz / st: every lane's size
// and status with its own `sz > max_len` check applied (a NAME's whole
// check).  Returns this lane's status.
template <class SM>
__device__ __noinline__ uint32_t
wire_limit_rare(const uint8_t *in, QH_LDS SM *sm, WireLimit lim, WireOffs to,
                uint32_t cnt, uint32_t sz, uint32_t st)
{
    const uint32_t lane = lane_id();
    // (every lane: cross-lane reads)
    uint32_t n_sz = all_lanes(wave_shr1(sz));
    uint32_t n_st = all_lanes(wave_shr1(st));
    if (lane >= cnt || wm_kind(to.meta) != QHUFF_LIT_VALUE
            || st != QHUFF_DEC_OK)
        return st;
    uint32_t used = 0;
    bool named = false;
    // (the batch's first literal holds itself as the one before: no NAME)
    if (wm_kind(to.p_meta) == QHUFF_LIT_NAME && to.p_instr == to.instr)
    {
        if (lane == 0)
        {
            // the previous tile's last literal
            const uint32_t p_pos =
                ((const QH_GLB uint32_t *) lim.lits)[4 * ((uint64_t) to.s0 - 1)];
            n_st = QHUFF_DEC_OK;
            n_sz = to.p_len;
            if (wm_huff(to.p_meta))
            {
                CountEmit em{0};
                const int r = wire_walk_glb(in, sm, p_pos, to.p_len, em);
                n_st = r < 0 ? QHUFF_DEC_ERROR : QHUFF_DEC_OK;
                n_sz = r < 0 ? 0u : (uint32_t) r;
            }
            if (n_sz > lim.max_len)
                n_st = QHUFF_DEC_ERROR;
        }
        named = n_st == QHUFF_DEC_OK;
        used = n_sz;
    }
    if (!named)
        used = wire_ref_name_len(in, to.pos, to.meta, to.instr);
    return (uint64_t) used + sz > lim.max_len ? (uint32_t) QHUFF_DEC_ERROR : st;
}

// The limit over a tile's sizes and statuses (max_len != 0).  A lane needs
// another literal's result only when its own size plus an upper bound of its
// name passes max_len -- the bound: what the literal before can emit if that
// is a NAME (floor(8 * len / 5), or len if raw), and the longest static name
// in any case (a NAME that turns out invalid leaves the static reference) --
// which takes a string within a few bytes of 64 KB: out of line.  Every
// other lane's check is sz > max_len.
template <class SM>
__device__ __forceinline__ void
wire_limit(const uint8_t *in, QH_LDS SM *sm, const WireLimit &lim,
           const WireOffs &to, uint32_t cnt, uint32_t &sz, uint32_t &st)
{
    const bool valid = lane_id() < cnt;
    const bool over = valid & (sz > lim.max_len);
    st = over ? (uint32_t) QHUFF_DEC_ERROR : st;
    sz = over ? 0u : sz;
    // (32-bit: a length whose bound does not fit counts as the largest; a
    // valid lane with status OK has sz <= max_len here)
    const uint32_t nb = wm_kind(to.p_meta) != QHUFF_LIT_NAME ? 0u
                      : !wm_huff(to.p_meta) ? to.p_len
                      : to.p_len > (1u << 28) ? 0xffffffffu : to.p_len * 8 / 5;
    const uint32_t ub = nb > kStaticNameMax ? nb : kStaticNameMax;
    const bool near = valid & (wm_kind(to.meta) == QHUFF_LIT_VALUE)
                    & (st == QHUFF_DEC_OK) & (ub > lim.max_len - sz);
    if (__builtin_expect(__builtin_amdgcn_ballot_w64(near) != 0, 0))
    {
        st = wire_limit_rare(in, sm, lim, to, cnt, sz, st);
        sz = st == QHUFF_DEC_OK ? sz : 0u;
    }
}

// a raw literal's bytes from the staged source -- byte-swapped dwords
// (Chunks::store<true>), read as the walk reads them (DecLds) -- into its
// arena slot: bytes [rs, rs + len) of the stage, four a trip
__device__ __forceinline__ void
wire_raw_copy(const QH_LDS uint32_t *stage, bool raw, uint32_t rs, uint32_t len,
              QH_LDS uint8_t *dst)
{
    const DecLds src{stage};
    const uint32_t n = raw ? len : 0u;
    const uint32_t K = wave_max_dpp((n + 3) >> 2);
    const uint32_t i0 = rs >> 2, sk = 8 * (rs & 3);
    for (uint32_t k = 0; k < K; ++k)
        if (4 * k < n)
        {
            const uint32_t a = src.dw(i0 + k), b = src.dw(i0 + k + 1);
            const uint32_t w =
                bswap32(sk ? __builtin_amdgcn_alignbit(a, b, 32 - sk) : a);
            const uint32_t left = n - 4 * k;
            write_bytes(dst + 4 * k, w, left < 3 ? left : 3);
            if (left > 3)
                dst[4 * k + 3] = (uint8_t) (w >> 24);
        }
}

// the sizes and statuses of a tile past the stage, counted in global memory
// (before the limit)
template <class SM>
__device__ __noinline__ SzSt
wire_tile_sizes(const uint8_t *in, QH_LDS SM *sm, uint32_t cnt, WireOffs to)
{
    const bool valid = lane_id() < cnt;
    SzSt o;
    o.sz = 0;
    o.st = QHUFF_DEC_OK;
    if (valid)
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

// A tile past the stages, as dec_slow_tile(): staged input -> the arena
// already holds the bytes; otherwise the sizes and statuses were counted in
// global memory (wire_tile_sizes, then the limit) and each valid literal is
// written to global by its lane -- a Huffman one walked again, a raw one
// copied, the long raw ones by the whole wave.  Out of line (cold).
template <class SM, class BaseOf>
__device__ __noinline__ uint64_t
wire_slow_tile(const uint8_t *in, QH_LDS SM *sm, QH_LDS DecWave *wv,
               uint32_t slot0, uint32_t cnt, WireOffs to, Span sp, uint32_t sz,
               uint32_t st, uint8_t *out, uint32_t *t_off, uint8_t *t_status,
               BaseOf base_of)
{
    const uint32_t lane = lane_id();
    const SlowTile f = SlowTile::begin(sz, base_of);
    uint8_t *dst = out + f.base + f.excl;
    if (sp.staged)
        arena_to_global(wv->arena + slot0, dst, sz);
    else
    {
        const bool live = lane < cnt && st == QHUFF_DEC_OK && sz;
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

// Arena slots: DecPolicyT's (qhuff_decode_impl.h), unchanged.  A slot is
// sized from its literal's payload bytes for the most a Huffman string can
// emit, floor(8 * len / 5) + 1; a raw literal emits len <= floor(8 * len / 5)
// bytes and writes none past them.  Slots placed by input offset start at
// 2 * lane + floor(8 * (o0 - A) / 5): instruction bytes and gaps between two
// literals move the next slot up, never down (o0 of lane i + 1 is at least
// o1 of lane i: the order rule), and the last slot ends below
// 2 * 64 + floor(8 * (span) / 5), the span at most kDecInCap as before.
static_assert(kFixMaxLen <= 8 * kFixMaxLen / 5, "a raw literal fits its slot");

// the in-place side of the wave pipeline (qhuff_pipeline.h): a lean policy
// -- tiles past the stages out of line, every literal by its lane
struct WirePolicy : DecStagePolicy<DecSmem>
{
    static constexpr bool kBig = false;
    static constexpr bool kCoop = false;
    static constexpr uint64_t coop = 0;
    using Offs = WireOffs;
    WireLimit lim;

    // staged tile: this lane's literal into its arena slot
    __device__ __forceinline__ void codec(const Offs &to, uint32_t cnt,
                                          const Span &sp, uint32_t *sz,
                                          uint32_t *st)
    {
        const uint32_t lane = lane_id();
        const bool valid = lane < cnt;
        const uint32_t o0 = to.o0(valid), o1 = to.o1();
        const uint32_t hl = o1 - o0;
        place(lane, o0, o1, to.first(), valid, 2, kFixMaxLen);
        const uint32_t rs = (uint32_t) ((uintptr_t) (in + o0) - sp.pa);
        const uint32_t re = (uint32_t) ((uintptr_t) (in + o1) - sp.pa);
        const bool huff = wm_huff(to.meta);
        int r = 0;
        if (valid)
        {
            // (a raw lane walks no bits)
            ArenaEmit em{wv->arena + slot0, wv->arena + slot0, 0};
            r = decode_string(DecLds{wv->in}, 8 * rs, huff ? 8 * re : 8 * rs,
                              sm->win, sm->long2, em);
        }
        const bool raw = valid & !huff;
        if (__builtin_amdgcn_ballot_w64(raw))
            wire_raw_copy(wv->in, raw, rs, hl, wv->arena + slot0);
        *sz = raw ? hl : r >= 0 ? (uint32_t) r : 0u;
        *st = r < 0 ? QHUFF_DEC_ERROR : QHUFF_DEC_OK;
        if (lim.max_len)
            wire_limit(in, sm, lim, to, cnt, *sz, *st);
    }
    __device__ __forceinline__ void slow_size(uint32_t cnt, Offs to, Span,
                                              uint32_t &sz, uint32_t &st)
    {
        const SzSt r = wire_tile_sizes(in, sm, cnt, to);
        sz = r.sz;
        st = r.st;
        if (lim.max_len)
            wire_limit(in, sm, lim, to, cnt, sz, st);
    }
    __device__ __forceinline__ void slow_tile(Coord c, uint32_t t, uint32_t cnt,
                                              Offs to, Span sp, uint32_t sz,
                                              uint32_t st, bool,
                                              uint8_t *out, uint32_t *out_off,
                                              uint8_t *status, uint64_t n,
                                              const LookBack &lb)
    {
        const uint64_t s0 = (uint64_t) t * kTS;
        const uint64_t end = wire_slow_tile(in, sm, wv, slot0, cnt, to, sp, sz,
                                            st, out, out_off + s0, status + s0,
                                            StartedBase{c, lb});
        last_tile_end(c, t, end, out_off, n);
    }
};

}  // namespace qhuff
