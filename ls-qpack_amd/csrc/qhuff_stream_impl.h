// qhuff_stream_impl.h -- the resumable decoder: a chunk of a string, from
// the tree node the string's earlier chunks ended on to the node this one
// ends on (qhuff_decode_stream, include/qhuff.h).  See qhuff_stream.hip.
// Here: the nodes, the pending-code start, the stop policy and the tile
// policy; the step loop, the tail lookup, both sources (the stage, and
// DecGlb for chunks past it) and the stage policy are qhuff_decode_impl.h's.
#pragma once

#include "qhuff_decode_impl.h"

namespace qhuff {

// A node is a key (qhuff_tables.h): its bit prefix left-aligned, then a
// marker one; depth = 31 - ctz(key).  The table holds key ^ kNodeRoot in
// ascending order, the root first.
__device__ __forceinline__ uint32_t
node_depth(uint32_t key)
{
    return 31u - (uint32_t) __builtin_ctz(key);
}

// the first d (<= 29) bits of w as a key
__device__ __forceinline__ uint32_t
node_key(uint32_t w, uint32_t d)
{
    return (w & ~(0xffffffffu >> (d & 31))) | (1u << ((31u - d) & 31));
}

// accepts: the root, or an all-ones path of at most 7 bits (D3: what may be
// left after a string's last symbol)
__device__ __forceinline__ bool
node_accepts(uint32_t key)
{
    const uint32_t d = node_depth(key);
    return d <= 7 && key == ~(0x7fffffffu >> d);
}

// key -> id: the last entry <= the key (8 probes, no lane branches)
__device__ __forceinline__ uint32_t
node_find(const QH_LDS uint32_t *s_nodes, uint32_t key)
{
    const uint32_t t = key ^ kNodeRoot;
    uint32_t lo = 0;
#pragma unroll
    for (uint32_t step = kNodes / 2; step; step >>= 1)
        lo += s_nodes[lo + step] <= t ? step : 0u;
    return lo;
}

// Stop policy of window_walk(): a long code running past the chunk's end
// stops its lane there.  The chunk's bits complete no code (the table would
// have found it, whatever lies behind them): the rem <= 29 left are the
// node reached.  held: `key` is set, the rest of the chunk is skipped.
struct StopAtNode
{
    uint32_t key, held;
    __device__ __forceinline__ bool past_end(bool past, uint32_t W,
                                             uint32_t rem)
    {
        key = past ? node_key(W, rem) : key;
        held |= past ? 1u : 0u;
        return past;
    }
};

struct StreamEnd
{
    uint32_t status;                 // QHUFF_DEC_OK / _ERROR / _MORE
    uint32_t node;                   // the node reached (not after an ERROR)
    uint32_t eos;                    // it accepts
};

// Decode the chunk whose bits are [bit0, bitend) of the big-endian dword
// stream `src`, from node `node_in`; emitted bytes go through `emit`
// (emit.n: their count).  With the semantics of lsqpack_huff_decode_full
// (lsqpack.c:3443-3517) given a dst that cannot run out:
//   start  a node of depth d > 0 is d bits into a code: the window of those
//          bits and the chunk's first 32 - d resolves that one code with the
//          window table or the canonical search, it is emitted and the walk
//          starts behind it; a chunk that ends before the code does descends
//          the node by all its bits and emits nothing;
//   walk   window_walk(), the batch decoder's step loop
//          (qhuff_decode_impl.h), under the StopAtNode policy: a long code
//          running past the chunk's end stops the lane there (in
//          decode_string it rejects the string); the EOS code rejects
//          as before;
//   end    the bits behind the last complete symbol (<= 29: no code is
//          complete) are the node reached; a final chunk is accepted iff
//          that node accepts -- the D3 tail rule over the carried bits too.
template <class Src, class Emit>
__device__ __forceinline__ StreamEnd
stream_decode(const Src &src, uint32_t bit0, uint32_t bitend, uint32_t node_in,
              bool fin, const QH_LDS uint32_t *s_win,
              const QH_LDS uint16_t *s_sorted, const QH_LDS uint16_t *s_long2,
              const QH_LDS uint32_t *s_nodes, Emit &emit)
{
    uint32_t rem = bitend - bit0;            // real bits not yet consumed
    uint32_t bad = 0;                        // (a u32: no lane-mask phis)
    StopAtNode stop{kNodeRoot, 0};           // the node reached
    const uint32_t kin = s_nodes[node_in & (kNodes - 1)] ^ kNodeRoot;
    const uint32_t d = node_depth(kin);
    if (__builtin_amdgcn_ballot_w64(d != 0))
    {
        // the code the string was in the middle of
        const uint32_t i0 = bit0 >> 5, sk = bit0 & 31;
        const uint32_t a = src.dw(i0), b = src.dw(i0 + 1);
        uint32_t cw = sk ? __builtin_amdgcn_alignbit(a, b, 32 - sk) : a;
        cw |= rem < 32 ? 0xffffffffu >> rem : 0u;    // ones past the chunk
        const uint32_t W = (kin & ~(1u << ((31u - d) & 31))) | (cw >> d);
        const uint32_t e = s_win[W >> (32 - kWinBits)];
        uint32_t L = ent_l0(e), sym = e & 0xff;
        const bool lng = e < (1u << 24);
        if (__builtin_amdgcn_ballot_w64((d != 0) & lng))
        {
            uint32_t L2;
            const uint32_t s2 = long_code(W, s_sorted, &L2);
            L = lng ? L2 : L;
            sym = lng ? s2 : sym;
        }
        const bool pend = d != 0;
        const uint32_t need = L - d;         // (a node's codes are longer)
        const bool done = pend & (L > d) & (need <= rem);
        const bool eosc = done & (sym == 256);
        const bool stay = pend & !done;      // then d + rem <= 29
        emit(sym, (done & !eosc) ? 1u : 0u);
        bad |= eosc ? 1u : 0u;
        stop.key = stay ? node_key(W, d + rem) : stop.key;
        stop.held |= (stay | eosc) ? 1u : 0u;
        const uint32_t c = done ? need : 0u;
        bit0 += c;
        rem = (stay | eosc) ? 0u : rem - c;
    }

    const Walked k = window_walk<true>(src, bit0, rem, s_win, s_long2, emit,
                                       stop);
    bad |= k.bad;
    // the r2 (<= 12) bits behind the last symbols complete no code
    const Tail tl = tail_lookup(k.W, k.rem, !(bad || k.rem == 0), s_win, emit);
    const uint32_t key = stop.held ? stop.key
                                   : node_key(tl.w << (tl.c & 31), tl.r2);
    emit.finish();
    StreamEnd r;
    r.eos = node_accepts(key) ? 1u : 0u;
    bad |= (fin && !r.eos) ? 1u : 0u;
    r.node = node_find(s_nodes, key);
    r.status = bad ? QHUFF_DEC_ERROR : fin ? QHUFF_DEC_OK : QHUFF_DEC_MORE;
    return r;
}

// Arena slots of the stream policy: a chunk of len bytes emits at most
// floor(8 * len / 5) + 1 bytes (the pending symbol needs one bit, the other
// 8 * len - 1 hold floor((8 * len - 1) / 5) codes at most) and the emitter
// writes two past its end: one byte a string more than DecPolicyT's slots.
// Fixed stride: floor(8 * len / 5) + 3 <= kFixStride; by input offset:
// 3 * lane + floor(8 * (o0 - A) / 5).
constexpr uint32_t kStreamFixMaxLen = (5 * (kFixStride - 3)) / 8;
static_assert(8 * kStreamFixMaxLen / 5 + 3 <= kFixStride, "fixed slot");
static_assert(3 * kDecTS + 8 * kDecInCap / 5 + QH_ARENA_SLACK <= kArenaBytes,
              "slots by input offset");

struct StreamSmem : DecSmem
{
    uint32_t nodes[kNodes];          // sorted node keys (qhuff_tables.h)
};

// a tile's offsets and its first string's index (the state and flags of
// string s0 + lane)
struct StreamOffs : TileOffs
{
    uint32_t s0;
    __device__ __forceinline__ void load(const QH_GLB uint32_t *in_off,
                                         uint64_t s, uint32_t cnt)
    {
        TileOffs::load(in_off, s, cnt);
        s0 = (uint32_t) s;
    }
};

struct StreamIo
{
    ::qhuff_decode_status *state;
    const uint8_t *flags;
    // this lane's node and FINAL bit (every lane loads: index clamped)
    __device__ __forceinline__ void load(uint32_t s0, uint32_t cnt,
                                         uint32_t *node, bool *fin) const
    {
        const uint32_t lane = lane_id();
        const uint64_t i = (uint64_t) s0 + (lane < cnt ? lane : cnt - 1);
        *node = ((const QH_GLB uint8_t *) state)[2 * i];
        *fin = flags ? (((const QH_GLB uint8_t *) flags)[i]
                        & QHUFF_STREAM_FINAL) != 0 : false;
    }
    __device__ __forceinline__ void store(uint32_t s0, const StreamEnd &e) const
    {
        const uint64_t i = (uint64_t) s0 + lane_id();
        ((QH_GLB uint8_t *) state)[2 * i] = (uint8_t) e.node;
        ((QH_GLB uint8_t *) state)[2 * i + 1] = (uint8_t) e.eos;
    }
};

// A tile past the stages (qhuff_pipeline.h), as dec_slow_tile(): staged
// input -> the arena already holds the bytes and the states are written;
// otherwise the sizes, statuses and end nodes were counted from global
// memory (stream_tile_sizes) and the chunks are decoded again to global,
// each by its lane, before its state is replaced.  Out of line (cold).
template <class BaseOf>
__device__ __noinline__ uint64_t
stream_slow_tile(const uint8_t *in, QH_LDS StreamSmem *sm, QH_LDS DecWave *wv,
                 StreamIo io, uint32_t slot0, uint32_t cnt, StreamOffs to,
                 Span sp, uint32_t sz, uint32_t st, StreamEnd end,
                 uint8_t *out, uint32_t *t_off, uint8_t *t_status,
                 BaseOf base_of)
{
    const bool valid = lane_id() < cnt;
    const SlowTile f = SlowTile::begin(sz, base_of);
    uint8_t *dst = out + f.base + f.excl;
    if (sp.staged)
        arena_to_global(wv->arena + slot0, dst, sz);
    else
    {
        uint32_t node;
        bool fin;
        io.load(to.s0, cnt, &node, &fin);
        if (valid && sz)
        {
            const uint32_t rs = (uint32_t) ((uintptr_t) (in + to.o0) - sp.pa);
            const uint32_t re = (uint32_t) ((uintptr_t) (in + to.o1) - sp.pa);
            const DecGlb src{(const QH_GLB uint32_t *) sp.pa, 8 * re};
            GlobalEmit em{dst, 0};
            stream_decode(src, 8 * rs, 8 * re, node, fin, sm->win, sm->sorted,
                          sm->long2, sm->nodes, em);
        }
        if (valid)
            io.store(to.s0, end);
    }
    return f.end<true>(cnt, st, t_off, t_status);
}

// the sizes, statuses and end nodes of a tile past the stage, counted in
// global memory
struct StreamSized
{
    uint32_t sz, st;
    StreamEnd end;
};
__device__ __noinline__ StreamSized
stream_tile_sizes(const uint8_t *in, QH_LDS StreamSmem *sm, StreamIo io,
                  uint32_t cnt, StreamOffs to, Span sp)
{
    const bool valid = lane_id() < cnt;
    uint32_t node;
    bool fin;
    io.load(to.s0, cnt, &node, &fin);
    StreamSized o;
    o.sz = 0;
    o.st = 0;
    o.end = StreamEnd{0, 0, 0};
    if (valid)
    {
        const uint32_t rs = (uint32_t) ((uintptr_t) (in + to.o0) - sp.pa);
        const uint32_t re = (uint32_t) ((uintptr_t) (in + to.o1) - sp.pa);
        const DecGlb src{(const QH_GLB uint32_t *) sp.pa, 8 * re};
        CountEmit em{0};
        o.end = stream_decode(src, 8 * rs, 8 * re, node, fin, sm->win,
                              sm->sorted, sm->long2, sm->nodes, em);
        o.st = o.end.status;
        o.sz = o.st == QHUFF_DEC_ERROR ? 0u : em.n;
    }
    return o;
}

// the stream side of the wave pipeline (qhuff_pipeline.h): a lean policy --
// tiles past the stages out of line, every chunk by its lane
struct StreamPolicy : DecStagePolicy<StreamSmem>
{
    static constexpr bool kBig = false;
    static constexpr bool kCoop = false;
    static constexpr uint64_t coop = 0;
    using Offs = StreamOffs;
    StreamIo io;
    StreamEnd slow_end;              // (slow_size -> slow_tile)

    // staged tile: this lane's chunk into its arena slot, its state replaced
    __device__ __forceinline__ void codec(const Offs &to, uint32_t cnt,
                                          const Span &sp, uint32_t *sz,
                                          uint32_t *st)
    {
        const uint32_t lane = lane_id();
        const bool valid = lane < cnt;
        uint32_t node;
        bool fin;
        io.load(to.s0, cnt, &node, &fin);
        place(lane, to.o0, to.o1, read_lane(to.o0, 0), valid, 3,
              kStreamFixMaxLen);
        const uint32_t rs = (uint32_t) ((uintptr_t) (in + to.o0) - sp.pa);
        const uint32_t re = (uint32_t) ((uintptr_t) (in + to.o1) - sp.pa);
        *sz = 0;
        *st = 0;
        if (valid)
        {
            ArenaEmit em{wv->arena + slot0, wv->arena + slot0, 0};
            const StreamEnd e = stream_decode(DecLds{wv->in}, 8 * rs, 8 * re,
                                              node, fin, sm->win, sm->sorted,
                                              sm->long2, sm->nodes, em);
            *st = e.status;
            *sz = e.status == QHUFF_DEC_ERROR ? 0u : em.n;
            io.store(to.s0, e);
        }
    }
    __device__ __forceinline__ void slow_size(uint32_t cnt, Offs to, Span sp,
                                              uint32_t &sz, uint32_t &st)
    {
        const StreamSized r = stream_tile_sizes(in, sm, io, cnt, to, sp);
        sz = r.sz;
        st = r.st;
        slow_end = r.end;
    }
    __device__ __forceinline__ void slow_tile(Coord c, uint32_t t, uint32_t cnt,
                                              Offs to, Span sp, uint32_t sz,
                                              uint32_t st, bool,
                                              uint8_t *out, uint32_t *out_off,
                                              uint8_t *status, uint64_t n,
                                              const LookBack &lb)
    {
        const uint64_t s0 = (uint64_t) t * kTS;
        const uint64_t end = stream_slow_tile(in, sm, wv, io, slot0, cnt, to,
                                              sp, sz, st, slow_end, out,
                                              out_off + s0, status + s0,
                                              StartedBase{c, lb});
        last_tile_end(c, t, end, out_off, n);
    }
};

}  // namespace qhuff
