// qhuff_encwire_impl.h -- whole QPACK field lines and instructions encoded
// in one launch (qhuff_encode_wire, include/qhuff.h).  See
// qhuff_encwire.hip.  Here: the item loads, the prefixed integer, the
// out-of-line tile and the tile policy; the dense pass, sizing, the bit
// packers and the literal framing are qhuff_encode_impl.h's, unchanged.
#pragma once

#include <stddef.h>

#include "qhuff_encode_impl.h"

// pending tiles: with the item in flight across the dense pass a third
// tile's output in registers spills 18 VGPRs (2 at depth 2)
#ifndef QH_ENCW_DEPTH
#define QH_ENCW_DEPTH 2
#endif

namespace qhuff {

static_assert(sizeof(::qhuff_item) == 8 && alignof(::qhuff_item) == 4
              && offsetof(::qhuff_item, int_bits) == 4
              && offsetof(::qhuff_item, str_first) == 7,
              "one 64-bit load an item: ival, then the four bytes");

// The kernel's arguments: the items first, at offset 0 of the kernel
// argument segment (kernel_items() reads them there: the tile pipeline
// hands a policy's loads the offsets pointer only).
struct EncWireArgs
{
    const ::qhuff_item *items;
    EncArgs e;                       // (e.mode unused: every item has its own)
};
static_assert(offsetof(EncWireArgs, items) == 0, "kernel_items()");

// A descriptor as the kernel uses it, one dword: whatever bytes the caller
// left are masked into the item rule's ranges here, so that no item passes
// 6 + 6 bytes of framing and none writes outside its own bytes.
//   [3:0] int_bits 0..8   [6:4] str_bits 0..7   [10:8] the integer's bytes
//   [23:16] int_first, its prefix bits clear
//   [31:24] str_first, its H bit and prefix bits clear
__device__ __forceinline__ uint32_t im_ib(uint32_t m) { return m & 15; }
__device__ __forceinline__ uint32_t im_sb(uint32_t m) { return (m >> 4) & 7; }
__device__ __forceinline__ uint32_t im_ilen(uint32_t m) { return (m >> 8) & 7; }
__device__ __forceinline__ uint32_t im_ifirst(uint32_t m) { return (m >> 16) & 0xff; }
__device__ __forceinline__ uint32_t im_sfirst(uint32_t m) { return m >> 24; }

// raw: the item's second dword (int_bits, int_first, str_bits, str_first)
__device__ __forceinline__ uint32_t
item_meta(uint32_t raw, uint32_t ival)
{
    const uint32_t ib = min(raw & 0xff, 8u);
    const uint32_t sb = (raw >> 16) & 7;
    const uint32_t ifirst = ib ? (raw >> 8) & 0xff & ~((1u << ib) - 1) : 0u;
    const uint32_t sfirst = sb ? (raw >> 24) & ~((2u << sb) - 1) : 0u;
    const uint32_t ilen = ib ? int_len(ival, ib) : 0u;       // <= 6
    return ib | (sb << 4) | (ilen << 8) | (ifirst << 16) | (sfirst << 24);
}

// dword-aligned view of an item (the array needs its type's alignment only)
struct __attribute__((packed, aligned(4))) I2 { u32x2 v; };

// this launch's items: the kernel's first argument (EncWireArgs)
__device__ __forceinline__ const QH_GLB I2 *
kernel_items()
{
    typedef const __attribute__((address_space(4))) uint64_t KArg;
    return (const QH_GLB I2 *) (uintptr_t)
        *(KArg *) __builtin_amdgcn_kernarg_segment_ptr();
}

// item s0 + lane of a tile of cnt items (lanes >= cnt: the tile's last)
__device__ __forceinline__ u32x2
item_load(uint32_t s0, uint32_t cnt)
{
    const uint32_t lane = lane_id();
    return kernel_items()[(uint64_t) s0 + (lane < cnt ? lane : cnt - 1)].v;
}

// A tile's offsets: TileOffs, and where its items are -- the tile's first
// item and its count, wave-uniform.  The items themselves are loaded when
// the tile is staged (EncWirePolicyT::stage_in), a dense pass before their
// use: held here they would wait in registers for two tiles, as the offsets
// do, and the tile loop has none to spare.
struct ItemOffs
{
    uint32_t o0, o1;
    uint32_t s0, cnt;

    __device__ __forceinline__ void load(const QH_GLB uint32_t *in_off,
                                         uint64_t s, uint32_t n)
    {
        const uint32_t lane = lane_id();
        o0 = in_off[s + (lane < n ? lane : n)];
        o1 = in_off[s + (lane + 1 < n ? lane + 1 : n)];
        s0 = (uint32_t) s;
        cnt = n;
    }
    __device__ __forceinline__ uint32_t first() const { return read_lane(o0, 0); }
    __device__ __forceinline__ uint32_t last() const { return read_lane(o1, 63); }
};

// the item's size: its integer, and its literal as size_from_bits /
// size_string frame it with the lane's own prefix width (none: nothing)
__device__ __forceinline__ EncSize
item_size_bits(uint32_t m, uint32_t bits, uint32_t len)
{
    EncSize z = (EncSize){0, 0, true};
    if (im_sb(m))
        z = size_from_bits(im_sb(m), bits, len);
    return z;
}

template <class Src>
__device__ __forceinline__ EncSize
item_size_string(uint32_t m, const Src &src, uint32_t rs, uint32_t re,
                 const QH_LDS uint8_t *s_len)
{
    EncSize z = (EncSize){0, 0, true};
    if (im_sb(m))
        z = size_string(im_sb(m), src, rs, re, s_len);
    return z;
}

// lsqpack_enc_int (lsqpack.c:787-814) into the zeroed LDS stage at byte
// `start`: the value on a prefix of im_ib(m) bits of a first byte preset to
// int_first
__device__ __forceinline__ void
emit_int(QH_LDS uint32_t *st, uint32_t start, uint32_t m, uint32_t v)
{
    const uint32_t mask = (1u << im_ib(m)) - 1;
    uint32_t pos = 8 * start;
    if (v < mask)
    {
        or_bits(st, pos, im_ifirst(m) | v, 8);
        return;
    }
    or_bits(st, pos, im_ifirst(m) | mask, 8);
    pos += 8;
    v -= mask;
    while (v >= 128)
    {
        or_bits(st, pos, 0x80 | (v & 0x7f), 8);
        pos += 8;
        v >>= 7;
    }
    or_bits(st, pos, v, 8);
}

// an item straight to global memory (the out-of-line tile): the integer,
// then the literal as emit_string frames it with str_first on its first byte
template <class Src, class Sink>
__device__ __forceinline__ void
emit_item(const Src &src, uint32_t rs, uint32_t re, uint32_t m, uint32_t ival,
          const EncSize &z, const QH_LDS u32x2 *s_enc, Packer<Sink> &pk)
{
    if (im_ib(m))
    {
        const uint32_t mask = (1u << im_ib(m)) - 1;
        uint32_t v = ival;
        if (v < mask)
            pk.put(im_ifirst(m) | v, 8);
        else
        {
            pk.put(im_ifirst(m) | mask, 8);
            v -= mask;
            while (v >= 128)
            {
                pk.put(0x80 | (v & 0x7f), 8);
                v >>= 7;
            }
            pk.put(v, 8);
        }
    }
    if (const uint32_t sb = im_sb(m))
    {
        const uint32_t mask = (1u << sb) - 1;
        const uint32_t first = im_sfirst(m) | (z.huff ? 1u << sb : 0u);
        if (z.plen < mask)
            pk.put(first | z.plen, 8);
        else
        {
            pk.put(first | mask, 8);
            uint32_t v = z.plen - mask;
            while (v >= 128)
            {
                pk.put(0x80 | (v & 0x7f), 8);
                v >>= 7;
            }
            pk.put(v, 8);
        }
        pack_string(src, rs, re, !z.huff, s_enc, pk);
    }
    pk.finish();
}

// the sizes of a tile past the stage, from global memory
template <class SM>
__device__ __noinline__ EncSize
encwire_tile_sizes(const uint8_t *in, QH_LDS SM *sm, uint32_t cnt, ItemOffs to,
                   uint32_t m, Span sp)
{
    EncSize z = (EncSize){0, 0, true};
    if (lane_id() < cnt)
    {
        const EncGlb gsrc{(const QH_GLB uint32_t *) sp.pa};
        const uint32_t rs = (uint32_t) ((uintptr_t) (in + to.o0) - sp.pa);
        const uint32_t re = (uint32_t) ((uintptr_t) (in + to.o1) - sp.pa);
        z = item_size_string(m, gsrc, rs, re, sm->len);
    }
    return z;
}

// A tile whose input or output does not fit the stages, as enc_slow_tile():
// sized already (sz, z: from the stage, or encwire_tile_sizes), every item
// packed straight to global memory by its lane -- from the stage when the
// input is there, else from global memory.  Out of line (cold).
template <class SM, class BaseOf>
__device__ __noinline__ uint64_t
encwire_slow_tile(const uint8_t *in, QH_LDS SM *sm, QH_LDS EncWave *wv,
                  EncSize z, uint32_t m, uint32_t ival, uint32_t cnt,
                  ItemOffs to, Span sp,
                  uint32_t sz, uint8_t *out, uint32_t *t_off, BaseOf base_of)
{
    const bool valid = lane_id() < cnt;
    const uint32_t rs = valid ? (uint32_t) ((uintptr_t) (in + to.o0) - sp.pa) : 0;
    const uint32_t re = valid ? (uint32_t) ((uintptr_t) (in + to.o1) - sp.pa) : 0;
    const SlowTile f = SlowTile::begin(sz, base_of);
    if (valid && sz)
    {
        const uint32_t adj = (uint32_t) ((uintptr_t) out & 3);
        Packer<PackGlb> pk;
        pk.sink.out = out - adj;
        const uint32_t p0 = adj + (uint32_t) f.base + f.excl;
        pk.init(p0, p0 + sz);
        if (sp.staged)
            emit_item(EncLds{wv->in}, rs, re, m, ival, z, sm->enc, pk);
        else
            emit_item(EncGlb{(const QH_GLB uint32_t *) sp.pa}, rs, re, m,
                      ival, z, sm->enc, pk);
    }
    return f.end<false>(cnt, 0, t_off, nullptr);
}

// the item side of the wave pipeline (qhuff_pipeline.h): a lean policy over
// the encode stages -- EncPolicyT<SM, false> with the framing per lane
template <class SM>
struct EncWirePolicyT
{
    static constexpr bool kStatus = false;
    static constexpr bool kBig = false;
    static constexpr bool kCoop = false;
    static constexpr uint64_t coop = 0;
    static constexpr int kInCap = kEncInCap;
    static constexpr int kDepth = QH_ENCW_DEPTH;
    static constexpr int kOutCap = kEncOutCap;
    static constexpr int kNch = kChunks;
    static constexpr uint32_t kTS = kWT;          // items per tile
    using Offs = ItemOffs;
    const uint8_t *in;
    QH_LDS SM *sm;
    QH_LDS EncWave *wv;
    uint32_t rse;                    // this lane's string in the stage:
                                     // start | end << 16 (<= 3 KB)
    uint32_t dsb;                    // its range of the dense stream:
                                     // start | bits << 16 (< 2^15 each)
    uint32_t m, ival;                // its item (item_meta; the item's
                                     // second dword until codec())
    EncSize z;                       // its literal
    uint32_t dense;                  // wave-uniform: tile from the dense stream
#ifdef QH_PATH_TRACE
    PathTrace tr;                    // (diagnostic) the current tile's paths
#endif

    // staged tile: chunks into the LDS stage; the tile's items on their way
    __device__ __forceinline__ void stage_in(const Chunks<kChunks> &ch,
                                             const Span &sp, const Offs &to)
    {
        ch.store<false>((QH_LDS u32x4 *) wv->in, sp.n16);
        const u32x2 v = item_load(to.s0, to.cnt);
        ival = v.x;
        m = v.y;
    }
    // the byte-parallel pass over the staged span, as the batch kernel's
    __device__ __forceinline__ void prepare(const Span &sp)
    {
        if constexpr (SM::kMtRep)
            dense_pass<true>(sp.n16, sm->mtr, wv);
        else
            dense_pass<false>(sp.n16, sm->mt, wv);
        dense = true;
    }
    __device__ __forceinline__ const QH_LDS uint32_t *out_stage() const
    {
        return wv->out;
    }
    // staged tile: size this lane's item
    __device__ __forceinline__ void codec(const Offs &to, uint32_t cnt,
                                          const Span &sp, uint32_t *sz,
                                          uint32_t *st)
    {
        const uint32_t lane = lane_id();
        const bool valid = lane < cnt;
        const uint32_t rs = valid ? (uint32_t) ((uintptr_t) (in + to.o0) - sp.pa) : 0;
        const uint32_t re = valid ? (uint32_t) ((uintptr_t) (in + to.o1) - sp.pa) : 0;
        rse = rs | (re << 16);
        m = valid ? item_meta(m, ival) : 0u;
        z = (EncSize){0, 0, true};
        uint32_t bits = 0;
        if (dense)
        {
            // string i spans the dense bits between the offsets of its ends
            // (an item without a literal too: its bytes shift the others')
            const uint32_t se = dense_at(wv, re);
            const uint32_t ra = (uint32_t) ((uintptr_t) (in + to.first()) - sp.pa);
            const uint32_t s_first = dense_at(wv, ra);
            uint32_t prev = wave_shr1(se);
            // (every lane shifts: not moved into the select's branch)
            asm volatile("" : "+v"(prev));
            const uint32_t ds = lane != 0 ? prev : s_first;
            bits = se - ds;
            dense = read_lane(se, cnt - 1) + 64 <= kDenseBits;
            dsb = ds | (bits << 16);
        }
#ifdef QH_PATH_TRACE
        tr.units += 1;
        tr.dense += dense ? 1u : 0u;
#endif
        if (valid)
            z = dense ? item_size_bits(m, bits, re - rs)
                      : item_size_string(m, EncLds{wv->in}, rs, re, sm->len);
        *sz = im_ilen(m) + z.size;
        *st = 0;
    }
    // the integer, then the literal with str_first on its first byte, into
    // the zeroed output stage
    __device__ __forceinline__ void emit(uint32_t excl, uint32_t sz,
                                         uint32_t total)
    {
        QH_LDS u32x4 *o4 = (QH_LDS u32x4 *) wv->out;
        const uint32_t n16 = (total + 15) / 16 + 1;
        for (uint32_t i = lane_id(); i < n16; i += 64)
            o4[i] = (u32x4){0, 0, 0, 0};
        wave_sync();
        (void) sz;
        if (im_ib(m))
            emit_int(wv->out, excl, m, ival);
        const uint32_t sb = im_sb(m);
        if (!sb)
            return;
        const uint32_t start = excl + im_ilen(m);
        const uint32_t rs = rse & 0xffff, re = rse >> 16;
        // (emit_prefix ORs the H bit and the length beside it)
        or_bits(wv->out, 8 * start, im_sfirst(m), 8);
        if (dense)
            emit_dense(wv->in, rs, re, sb, z, wv->dense, dsb & 0xffff,
                       dsb >> 16, sm->enc, wv->out, start);
        else
            emit_bits(wv->in, rs, re, sb, z.huff, z.plen, sm->enc, wv->out,
                      start);
    }
    // the sizes of a tile past the stage (no codec ran)
    __device__ __forceinline__ void slow_size(uint32_t cnt, Offs to, Span sp,
                                              uint32_t &sz, uint32_t &st)
    {
        const u32x2 v = item_load(to.s0, cnt);
        ival = v.x;
        m = lane_id() < cnt ? item_meta(v.y, v.x) : 0u;
        z = encwire_tile_sizes(in, sm, cnt, to, m, sp);
        sz = im_ilen(m) + z.size;
        st = 0;
    }
    // ... its output once the look-back lb (aggregate published) resolves
    __device__ __forceinline__ void slow_tile(Coord c, uint32_t t, uint32_t cnt,
                                              Offs to, Span sp, uint32_t sz,
                                              uint32_t, bool, uint8_t *out,
                                              uint32_t *out_off, uint8_t *,
                                              uint64_t n, const LookBack &lb)
    {
        const uint64_t end = encwire_slow_tile(in, sm, wv, z, m, ival, cnt, to, sp,
                                               sz, out,
                                               out_off + (uint64_t) t * kTS,
                                               StartedBase{c, lb});
        last_tile_end(c, t, end, out_off, n);
    }
};

}  // namespace qhuff
