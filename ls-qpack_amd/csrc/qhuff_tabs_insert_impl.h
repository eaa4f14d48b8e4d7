// qhuff_tabs_insert_impl.h -- encoder-stream inserts applied to a set of
// tables (qhuff_apply_inserts_tabs, include/qhuff.h): the accounting of one
// table and the plan of its part of the next arena.
//
// The same source runs as device code (qhuff_insapply_tabs.hip: a table a
// lane for the accounting, a table a wave for the copy) and as plain C++ on
// the host (qhuff_tabs_insert_cpu, qhuff_frames.cpp; tests/c/ builds it with
// g++ under the sanitizers).  The rules are the reference's push and evict
// (lsqpack_dec_push_entry, lsqpack.c:4534-4552; qdec_remove_overflow_entries,
// 4362-4377), its entry lookup (qdec_get_table_entry_rel, 2756-2764) and its
// length checks (4661-4667, 4878-4884), stated in include/qhuff.h.
//
// Everything read from arrays whose form the caller owes is clamped: ent
// values to D, offsets into [off[0], off[2D]], live_lo and keep into their
// table, ordinals to n_ins, a root to an earlier string of its own chunk.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/qhuff.h"
#include "qhuff_scan_impl.h"
#include "qhuff_tabs_impl.h"

namespace qhuff {
namespace ins {

// the arguments of the accounting, the sums and the copy
struct Args
{
    // the input set and its state
    const uint8_t *bytes;
    const uint32_t *off, *ent, *first;
    const uint32_t *cap, *live_lo, *keep;        // keep may be null
    uint32_t T, D;
    uint32_t arena;                      // the bytes `bytes` holds
    // what the scan left
    int32_t *rc;
    uint32_t *consumed;
    const uint32_t *ins_off, *chunk_cap;
    const ::qhuff_hstr *strs;
    const uint32_t *root, *ins_cap, *ins_ref;
    const uint8_t *ins_kind;
    uint32_t n_ins;
    // what the decode launch left: string s is dec[dec_off[s] .. dec_off[s+1])
    const uint8_t *dec;
    const uint32_t *dec_off;
    const uint8_t *status;
    // scratch: fin[2 n_ins] final lengths, rel[2 n_ins] a string's offset
    // among its chunk's new strings, plan[4T], sums[2 (T + 1)] (entries and
    // bytes before each table, 64 bits)
    uint32_t *fin, *rel, *plan;
    uint64_t *sums;
    // outputs
    uint32_t *ins_lo;
    uint8_t *out_bytes;
    uint32_t *out_off, *out_ent, *out_first, *cap_out, *live_lo_out;
    uint64_t out_cap;
    uint32_t ent_cap;
};

// a table's part of the next arena: plan[4c ..]
struct Plan
{
    uint32_t keep;       // absolute index of its first entry (out_first)
    uint32_t napp;       // inserts applied
    uint32_t cnt;        // entries it holds
    uint32_t bytes;      // their bytes
};

// What 2n descriptors of n inserts can decode to (the scratch of the apply and,
// behind the old arena, qhuff_tabs_insert_bound): qhuff_decode_headers_dyn_
// bound's formula, the one place both take it from
inline uint64_t
decode_bound(uint64_t wire_bytes, uint32_t n, uint32_t dyn_longest)
{
    return wire_bytes * 8 / 5 + (dyn_longest > 76 ? dyn_longest : 76ull) * n
         + 16;
}

QH_HD inline uint32_t
clampu(uint64_t v, uint64_t lo, uint64_t hi)
{
    return (uint32_t) (v < lo ? lo : v > hi ? hi : v);
}

// table c of the set and its chunk's ordinals, clamped
struct View
{
    uint32_t e0, d, first, k0, k1;
    uint32_t o_lo, o_hi;                 // off[0], off[2D]: the arena's span
    uint64_t ins0;
};

QH_HD inline View
view(const Args &a, uint32_t c)
{
    const scan::TabView t = scan::ins_tab_view(a.ent, a.first, a.D, c);
    View v;
    v.e0 = t.e0;
    v.d = t.d;
    v.first = t.first;
    v.ins0 = (uint64_t) t.first + t.d;
    v.k0 = a.ins_off[c] < a.n_ins ? a.ins_off[c] : a.n_ins;
    v.k1 = clampu(a.ins_off[c + 1], v.k0, a.n_ins);
    v.o_hi = a.D ? a.off[2ull * a.D] : 0;
    v.o_hi = v.o_hi < a.arena ? v.o_hi : a.arena;
    v.o_lo = a.D ? a.off[0] : 0;
    v.o_lo = v.o_lo < v.o_hi ? v.o_lo : v.o_hi;
    return v;
}

// offset i of the table's own (i in [0, 2d]), inside the arena's span
QH_HD inline uint32_t
tab_off(const Args &a, const View &v, uint64_t i)
{
    // (no entries at all: off may be null)
    return a.D ? clampu(a.off[2ull * v.e0 + i], v.o_lo, v.o_hi) : 0u;
}

// the string whose decoded bytes string s of chunk [2 k0, ..) takes: its
// root when that is an earlier string of the same chunk, else itself
QH_HD inline uint32_t
src_of(const Args &a, uint32_t k0, uint32_t s)
{
    const uint32_t r = a.root[s];
    return r != QHUFF_DYN_NONE && r >= 2 * k0 && r < s ? r : s;
}

QH_HD inline uint32_t
dec_len(const Args &a, uint32_t s)
{
    const uint32_t o0 = a.dec_off[s], o1 = a.dec_off[s + 1];
    return o1 > o0 ? o1 - o0 : 0u;
}

// The accounting of table c: rc, consumed, ins_lo, fin, rel, the final state
// and the plan.  Serial over the chunk's inserts.
QH_HD inline void
account(const Args &a, uint32_t c)
{
    const View v = view(a, c);
    const uint32_t lo0 = clampu(a.live_lo[c], v.first, v.ins0);
    // an entry's size, old (from the set) or new (from fin)
    auto size = [&](uint64_t abs) -> uint64_t {
        if (abs < v.ins0)
        {
            const uint64_t e = 2 * (abs - v.first);
            const uint32_t o0 = tab_off(a, v, e), o2 = tab_off(a, v, e + 2);
            return (o2 > o0 ? o2 - o0 : 0u) + 32ull;
        }
        const uint64_t s = 2 * (v.k0 + (abs - v.ins0));
        return (uint64_t) a.fin[s] + a.fin[s + 1] + 32;
    };
    uint64_t used = 0;
    for (uint64_t e = lo0; e < v.ins0; ++e)
        used += size(e);
    uint64_t lo = lo0, ins = v.ins0;
    uint32_t cap = a.cap[c], run = 0;
    bool ok = a.rc[c] == QHUFF_OK;
    for (uint32_t k = v.k0; ok && k < v.k1; ++k)
    {
        const uint32_t cmin = a.ins_cap[2ull * k];
        for (; used > cmin && lo < ins; ++lo)
            used -= size(lo);
        cap = a.ins_cap[2ull * k + 1];
        const uint32_t kind = a.ins_kind[k] & 3;
        const uint32_t sn = src_of(a, v.k0, 2 * k);
        const uint32_t sv = src_of(a, v.k0, 2 * k + 1);
        const uint32_t N = dec_len(a, sn), V = dec_len(a, sv);
        if (kind >= QHUFF_INS_DYN)
        {
            const uint64_t r = a.ins_ref[k];
            ok = r >= lo && r < ins;
        }
        if (kind != QHUFF_INS_DUP)
        {
            const ::qhuff_hstr &val = a.strs[2ull * k + 1];
            ok = ok && N <= cap
                 && val.len <= ((uint64_t) (cap - N) << 2 * (val.huffman & 1));
        }
        ok = ok && !(a.status[sn] | a.status[sv]);
        if (!ok)
            break;
        a.fin[2ull * k] = N;
        a.fin[2ull * k + 1] = V;
        a.rel[2ull * k] = run;
        a.rel[2ull * k + 1] = run + N;
        run += N + V;
        ++ins;
        used += (uint64_t) N + V + 32;
        for (; used > cap && lo < ins; ++lo)
            used -= size(lo);
        a.ins_lo[k] = (uint32_t) lo;
    }
    if (ok && a.rc[c] == QHUFF_OK)
    {
        const uint32_t cmin = a.chunk_cap[2ull * c];
        for (; used > cmin && lo < ins; ++lo)
            used -= size(lo);
        cap = a.chunk_cap[2ull * c + 1];
    }
    else
    {
        if (a.rc[c] == QHUFF_OK)
        {
            a.rc[c] = QHUFF_EPROTO;
            a.consumed[c] = 0;
        }
        for (uint32_t k = v.k0; k < v.k1; ++k)
            a.ins_lo[k] = lo0;
        lo = lo0;
        ins = v.ins0;
        cap = a.cap[c];
    }
    a.cap_out[c] = cap;
    a.live_lo_out[c] = (uint32_t) lo;
    // the plan: [keep, ins0) of the old entries, then the new ones from keep
    Plan p;
    // (in 64 bits: a set whose insert count passes 2^32 - 1 is the host
    // forms' QHUFF_ERANGE, and here only wrong numbers)
    uint64_t keep = a.keep ? a.keep[c] : lo;
    keep = keep < v.first ? v.first : keep > lo ? lo : keep;
    p.keep = (uint32_t) keep;
    p.napp = (uint32_t) (ins - v.ins0);
    p.cnt = (uint32_t) (ins - keep);
    uint64_t bytes = 0;
    if (keep < v.ins0)
    {
        // (a decreasing pair: the run counts as empty, as in moves())
        const uint32_t sb = tab_off(a, v, 2ull * (keep - v.first));
        const uint32_t se = tab_off(a, v, 2ull * v.d);
        bytes = se > sb ? se - sb : 0u;
    }
    const uint64_t j0 = keep > v.ins0 ? keep - v.ins0 : 0;
    if (j0 < p.napp)
        bytes += run - a.rel[2 * (v.k0 + j0)];
    p.bytes = (uint32_t) bytes;
    a.out_first[c] = p.keep;
    a.plan[4ull * c] = p.keep;
    a.plan[4ull * c + 1] = p.napp;
    a.plan[4ull * c + 2] = p.cnt;
    a.plan[4ull * c + 3] = p.bytes;
}

// what the copy of table c moves: its old run [sb, sb + nb) of the arena, its
// entries' offsets and its new strings
struct Moves
{
    uint64_t oe, base;           // its first output entry and byte
    uint32_t n_old, n_new;       // old entries kept, new entries kept
    uint32_t sb, nb;             // the old run: source offset and bytes
    uint64_t oi;                 // index into off of the old run's first
    uint32_t s0, rel0;           // first new string kept and its rel
    uint32_t k0;
};

QH_HD inline Moves
moves(const Args &a, uint32_t c)
{
    const View v = view(a, c);
    Moves m;
    const uint32_t keep = a.plan[4ull * c], napp = a.plan[4ull * c + 1];
    m.oe = a.sums[2ull * c];
    m.base = a.sums[2ull * c + 1];
    m.k0 = v.k0;
    m.n_old = keep < v.ins0 ? (uint32_t) (v.ins0 - keep) : 0u;
    m.n_old = m.n_old > v.d ? v.d : m.n_old;
    const uint64_t i0 = 2ull * (v.d - m.n_old);
    m.oi = 2ull * v.e0 + i0;
    m.sb = tab_off(a, v, i0);
    const uint32_t se = tab_off(a, v, 2ull * v.d);
    m.nb = m.n_old && se > m.sb ? se - m.sb : 0u;
    const uint64_t j0 = keep > v.ins0 ? keep - v.ins0 : 0;
    uint32_t room = v.k1 - v.k0;
    room = napp < room ? napp : room;
    m.n_new = j0 < room ? (uint32_t) (room - j0) : 0u;
    m.s0 = 2 * (v.k0 + (uint32_t) (j0 < room ? j0 : 0));
    m.rel0 = m.n_new ? a.rel[m.s0] : 0u;
    return m;
}

// out_off of old-run offset i (i in [0, 2 n_old)) and of new string i
QH_HD inline void
put_off(const Args &a, uint64_t at, uint64_t v)
{
    if (at <= 2ull * a.ent_cap)
        a.out_off[at] = (uint32_t) v;
}

QH_HD inline uint32_t
old_off(const Args &a, const Moves &m, uint64_t i)
{
    const uint32_t o = a.off[m.oi + i];
    const uint32_t hi = m.sb + m.nb;
    return (o < m.sb ? m.sb : o > hi ? hi : o) - m.sb;
}

// bytes [at, at + n) of out_bytes that may be written: n cut to the room
QH_HD inline uint32_t
out_room(const Args &a, uint64_t at, uint32_t n)
{
    if (at >= a.out_cap)
        return 0;
    return a.out_cap - at < n ? (uint32_t) (a.out_cap - at) : n;
}

// a new string's source bytes: their offset in dec, and their count -- the
// final length the accounting left, at most the source string's own
QH_HD inline uint32_t
new_src(const Args &a, const Moves &m, uint32_t s)
{
    return a.dec_off[src_of(a, m.k0, s)];
}

QH_HD inline uint32_t
new_len(const Args &a, const Moves &m, uint32_t s)
{
    const uint32_t l = dec_len(a, src_of(a, m.k0, s));
    return a.fin[s] < l ? a.fin[s] : l;
}

// the sums over the tables (host form; the device's is a workgroup's scan)
inline void
sums_host(const Args &a)
{
    uint64_t e = 0, b = 0;
    for (uint32_t c = 0; c < a.T; ++c)
    {
        a.sums[2ull * c] = e;
        a.sums[2ull * c + 1] = b;
        a.out_ent[c] = (uint32_t) e;
        e += a.plan[4ull * c + 2];
        b += a.plan[4ull * c + 3];
    }
    a.sums[2ull * a.T] = e;
    a.sums[2ull * a.T + 1] = b;
    a.out_ent[a.T] = (uint32_t) e;
    put_off(a, 2 * e, b);
}

// the copy of table c (host form): a memcpy for the old run, one a new string
inline void
copy_host(const Args &a, uint32_t c)
{
    const Moves m = moves(a, c);
    const uint32_t nb = out_room(a, m.base, m.nb);
    if (nb)
        memcpy(a.out_bytes + m.base, a.bytes + m.sb, nb);
    for (uint64_t i = 0; i < 2ull * m.n_old; ++i)
        put_off(a, 2 * m.oe + i, m.base + old_off(a, m, i));
    const uint64_t nbase = m.base + m.nb;
    for (uint32_t i = 0; i < 2 * m.n_new; ++i)
    {
        const uint32_t s = m.s0 + i;
        const uint64_t at = nbase + (a.rel[s] - m.rel0);
        put_off(a, 2 * (m.oe + m.n_old) + i, at);
        const uint32_t n = out_room(a, at, new_len(a, m, s));
        const uint32_t from = new_src(a, m, s);
        if (n)
            memcpy(a.out_bytes + at, a.dec + from, n);
    }
}

// The host and _cpu forms' check of their arguments: QHUFF_OK, QHUFF_EINVAL or
// QHUFF_ERANGE as include/qhuff.h lists them.  *D = ent[T]; *longest = the
// longest name + value of all entries.
inline int
check(const ::qhuff_dyn_tables *t, const ::qhuff_ins_state *st,
      const uint8_t *buf, const uint32_t *enc_off, const ::qhuff_ins_scan *sc,
      const ::qhuff_ins_out *o, uint32_t *D, uint32_t *longest)
{
    *D = 0;
    *longest = 0;
    if (!t || !st || !sc || !o || !sc->ins_off || !o->out_ent || !o->out_off)
        return QHUFF_EINVAL;
    const uint32_t T = t->T;
    if (T && (!st->cap || !st->max_cap || !st->live_lo || !enc_off || !sc->rc
              || !sc->consumed || !o->out_first || !o->cap_out
              || !o->live_lo_out))
        return QHUFF_EINVAL;
    if (sc->max_ins && (!sc->ins_ref || !sc->ins_kind || !o->ins_lo))
        return QHUFF_EINVAL;
    if (sc->max_ins > 0x7fffffffu)
        return QHUFF_ERANGE;
    if (const int r = tabs_check(t, nullptr, nullptr, nullptr, 0, false, D,
                                 longest))
        return r;
    for (uint32_t c = 0; c < T; ++c)
    {
        if (enc_off[c + 1] < enc_off[c])
            return QHUFF_EINVAL;
        const uint32_t e0 = t->ent[c], d = t->ent[c + 1] - e0;
        const uint64_t first = t->first[c], lo = st->live_lo[c];
        if (lo < first || lo > first + d)
            return QHUFF_EINVAL;
        uint64_t used = 0;
        for (uint64_t e = e0 + (lo - first); e < (uint64_t) e0 + d; ++e)
            used += t->off[2 * e + 2] - t->off[2 * e] + 32ull;
        if (used > st->cap[c] || st->cap[c] > st->max_cap[c]
                || st->max_cap[c] > (1u << 28)
                || t->max_entries[c] != st->max_cap[c] / 32)
            return QHUFF_EINVAL;
    }
    if (T && enc_off[T] > enc_off[0] && !buf)
        return QHUFF_EINVAL;
    if (*D + (uint64_t) sc->max_ins && !o->out_bytes && o->out_cap)
        return QHUFF_EINVAL;
    return QHUFF_OK;
}

// QHUFF_ERANGE when a table's insert count would pass 2^32 - 1
inline int
check_counts(const ::qhuff_dyn_tables *t, const uint32_t *ins_off)
{
    for (uint32_t c = 0; c < t->T; ++c)
        if ((uint64_t) t->first[c] + (t->ent[c + 1] - t->ent[c])
                + (ins_off[c + 1] - ins_off[c]) > 0xffffffffull)
            return QHUFF_ERANGE;
    return QHUFF_OK;
}

}  // namespace ins
}  // namespace qhuff
