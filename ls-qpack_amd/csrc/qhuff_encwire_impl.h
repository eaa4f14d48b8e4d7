// qhuff_encwire_impl.h -- whole QPACK field lines and instructions encoded
// in one launch (qhuff_encode_wire, include/qhuff.h).  See
// qhuff_encwire.hip.  Here: the item loads, an item's frame (ItemFrame) and
// the tile policy.  Everything else is qhuff_encode_impl.h's: the stage
// policy (EncStagePolicy), the dense pass, sizing, the bit packers, the one
// writer of prefixed integers (put_int, into the LDS stage or a Packer) and
// the out-of-line tile (enc_tile_sizes, enc_slow_tile, over the frame).
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

// An item's frame (qhuff_encode_impl.h, StrFrame): the integer on its own
// first byte, then the literal on a prefix of str_bits bits with str_first
// on its first byte; without str_bits no literal, whatever the string.
struct ItemFrame
{
    uint32_t m, ival;                // item_meta, the integer's value
    __device__ __forceinline__ EncSize size(uint32_t bits, uint32_t len) const
    {
        EncSize z = (EncSize){0, 0, true};
        if (im_sb(m))
            z = size_from_bits(im_sb(m), bits, len);
        return z;
    }
    __device__ __forceinline__ uint32_t front() const { return im_ilen(m); }
    __device__ __forceinline__ bool payload() const { return im_sb(m) != 0; }
    template <class Bytes>
    __device__ __forceinline__ void head(Bytes s, const EncSize &z) const
    {
        if (im_ib(m))
            s = put_int(s, im_ifirst(m), im_ib(m), ival);
        if (const uint32_t sb = im_sb(m))
            put_int(s, im_sfirst(m) | (z.huff ? 1u << sb : 0u), sb, z.plen);
    }
};

// the item side of the wave pipeline (qhuff_pipeline.h): a lean policy over
// the encode stages (EncStagePolicy) with the framing per lane
template <class SM>
struct EncWirePolicyT : EncStagePolicy<SM>
{
    using Base = EncStagePolicy<SM>;
    using Base::in;
    using Base::sm;
    using Base::wv;
    using Base::dense;
    using Base::kTS;
#ifdef QH_PATH_TRACE
    using Base::tr;
#endif
    static constexpr bool kBig = false;
    static constexpr int kDepth = QH_ENCW_DEPTH;
    using Offs = ItemOffs;
    uint32_t rse;                    // this lane's string in the stage:
                                     // start | end << 16 (<= 3 KB)
    uint32_t dsb;                    // its range of the dense stream:
                                     // start | bits << 16 (< 2^15 each)
    uint32_t m, ival;                // its item (item_meta; the item's
                                     // second dword until codec())
    EncSize z;                       // its literal

    // staged tile: chunks into the LDS stage; the tile's items on their way
    __device__ __forceinline__ void stage_in(const Chunks<Base::kNch> &ch,
                                             const Span &sp, const Offs &to)
    {
        Base::stage_in(ch, sp, to);
        const u32x2 v = item_load(to.s0, to.cnt);
        ival = v.x;
        m = v.y;
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
        uint32_t ds = 0, bits = 0;
        this->dense_range(to, sp, re, 0, cnt, ds, bits);
        dsb = ds | (bits << 16);
        if (valid)
            z = dense ? ItemFrame{m, ival}.size(bits, re - rs)
                      : size_string(ItemFrame{m, ival}, EncLds{wv->in}, rs, re,
                                    sm->len);
        *sz = im_ilen(m) + z.size;
        *st = 0;
    }
    // the integer, then the literal with str_first on its first byte, into
    // the zeroed output stage
    __device__ __forceinline__ void emit(uint32_t excl, uint32_t sz,
                                         uint32_t total)
    {
        this->zero_out(total);
        (void) sz;
        if (im_ib(m))
            put_int(StageBytes{wv->out, 8 * excl}, im_ifirst(m), im_ib(m), ival);
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
        z = enc_tile_sizes(in, ItemFrame{m, ival}, sm, cnt, to, sp);
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
        // (sized: by codec() or slow_size())
        const uint64_t end = enc_slow_tile(in, ItemFrame{m, ival}, sm, wv, z,
                                           cnt, to, sp, sz, true, out,
                                           out_off + (uint64_t) t * kTS,
                                           StartedBase{c, lb});
        last_tile_end(c, t, end, out_off, n);
    }
};

}  // namespace qhuff
