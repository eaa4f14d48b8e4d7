// qhuff_lookup_dyn_impl.h -- one header against the static table and the
// dynamic table's entries: lsqpack_enc_encode's lookups with index = 0
// (lsqpack.c:1671-1930) when the table is given and nothing is inserted.
//
// The same source runs as device code (qhuff_lookup_dyn.hip: the index build
// one entry a lane, the lookup one header a lane) and as plain C++ on the
// host (qhuff_dyn_lookup_cpu, qhuff_frames.cpp).  The static half is
// qhuff_lookup_impl.h's static_lookup, called unchanged.
//
// The index.  The reference keeps two bucket arrays over its entries, by
// name+value hash and by name hash (lsqpack.c:1738-1902).  Here both are
// open-addressing arrays of `slots` 32-bit words, rebuilt from the d entries
// on every call: a slot holds an entry's ordinal + 1 (0: empty), entry k
// claims the first empty slot from hash & (slots - 1) on, linearly, wrapping
// at the array's end.  slots = dyn_index_slots(d): the smallest power of two
// >= 2d, at least kDynIndexFloor -- a load of at most 1/2, so a probe run
// ends.  Which slot of a run an entry gets depends on the order of the
// claims (on the device: which lane's compare-and-swap wins).  The lookup's
// result does not: it walks the whole run to the first empty slot and
// applies its rule to every entry of it that is in the window and whose
// bytes are the header's -- the highest absolute index for a full match
// (lsqpack.c:1801-1824), the lowest for a name match (1877-1901).
#pragma once
#include <stdint.h>

#include "../../include/qhuff.h"
#include "qhuff_hash_impl.h"
#include "qhuff_lookup_impl.h"

namespace qhuff {

constexpr uint32_t kDynIndexFloor = 64;       // slots of the smallest index
constexpr uint32_t kDynMaxD = 1u << 28;       // entries an index is built for

QH_HDI constexpr uint32_t
dyn_index_slots(uint32_t d)
{
    uint32_t c = kDynIndexFloor;
    while (c < 2ull * d && c < (1u << 31))
        c <<= 1;
    return c;
}

// The table as the lookup reads it.  TB: a reader of its bytes (HashMem,
// HashGlb); P: a pointer to const uint32_t (plain, or in the global address
// space).  t0 / t1 = off[0] / off[2d] (0 when d = 0): an entry's offsets are
// clamped into them, and a decreasing pair is an empty string, so whatever
// `off` holds only bytes [t0, t1) are read.
template <class TB, class P>
struct DynTab
{
    TB tb;
    P off;                               // 2d + 1
    P nv, nm;                            // the two indices, mask + 1 slots each
    uint32_t mask;
    uint32_t d, first;
    uint32_t t0, t1;
};

struct DynEntry
{
    uint32_t a, m, b;                    // name [a, m), value [m, b)
};

template <class P>
QH_HDI DynEntry
dyn_entry(P off, uint32_t k, uint32_t t0, uint32_t t1)
{
    DynEntry e;
    e.a = off[2ull * k];
    e.m = off[2ull * k + 1];
    e.b = off[2ull * k + 2];
    e.a = e.a < t0 ? t0 : e.a > t1 ? t1 : e.a;
    e.m = e.m < e.a ? e.a : e.m > t1 ? t1 : e.m;
    e.b = e.b < e.m ? e.m : e.b > t1 ? t1 : e.b;
    return e;
}

// Entry k into both indices.  cas(p, v): *p == 0 ? (*p = v, true) : false,
// atomically where lanes run this side by side.  x is XOR-ed into both
// hashes for the first slot (0; over a set of tables: the mix of the entry's
// table, qhuff_tabs_impl.h).
template <class TB, class P, class W, class CAS>
QH_HDI void
dyn_index_insert(const TB &tb, P off, uint32_t k, uint32_t t0, uint32_t t1,
                 W nv, W nm, uint32_t mask, const CAS &cas, uint32_t x = 0)
{
    const DynEntry e = dyn_entry(off, k, t0, t1);
    const uint32_t h1 = xxh32(tb, e.a, e.m - e.a, QHUFF_XXH_SEED);
    const uint32_t h2 = xxh32(tb, e.m, e.b - e.m, h1);
    // (at most mask + 1 steps: it ends whatever the slots hold)
    uint32_t i = (h2 ^ x) & mask;
    for (uint32_t steps = 0; steps <= mask; ++steps, i = (i + 1) & mask)
        if (cas(nv + i, k + 1))
            break;
    i = (h1 ^ x) & mask;
    for (uint32_t steps = 0; steps <= mask; ++steps, i = (i + 1) & mask)
        if (cas(nm + i, k + 1))
            break;
}

// bytes [a, a + len) of r against bytes [ta, ta + len) of the table
template <class R, class TB>
QH_HDI bool
dyn_same(const R &r, uint32_t a, const TB &tb, uint32_t ta, uint32_t len)
{
    uint32_t i = 0;
    for (; len - i >= 4; i += 4)
        if (r.word(a + i) != tb.word(ta + i))
            return false;
    for (; i < len; ++i)
        if (r.byte(a + i) != tb.byte(ta + i))
            return false;
    return true;
}

struct DynHit
{
    uint32_t kind;                       // QHUFF_LINE_* (| QHUFF_LINE_DYN)
    uint32_t id;                         // static index, or QHUFF_STATIC_NONE
    uint32_t dyn;                        // absolute index, or QHUFF_DYN_NONE
};

// The best entry of one index's probe run from hash h on: FULL, name and
// value equal, the highest absolute index; else the name equal, the lowest.
// Entries outside the window [lo, hi) do not count.  -> found
template <bool FULL, class R, class TB, class P>
QH_HDI bool
dyn_probe(const R &r, uint32_t a, uint32_t nl, uint32_t vl, uint32_t h,
          const DynTab<TB, P> &t, uint32_t lo, uint32_t hi, uint32_t *best)
{
    const P slot = FULL ? t.nv : t.nm;
    bool found = false;
    uint32_t i = h & t.mask;
    for (uint32_t steps = 0; steps <= t.mask; ++steps, i = (i + 1) & t.mask)
    {
        uint32_t k = slot[i];
        if (!k)
            break;
        --k;
        // (a slot the build did not write cannot lead outside `off`)
        if (k >= t.d)
            continue;
        const uint32_t abs = t.first + k;
        if (abs < lo || abs >= hi)
            continue;
        if (found && (FULL ? abs < *best : abs > *best))
            continue;
        const DynEntry e = dyn_entry(t.off, k, t.t0, t.t1);
        if (e.m - e.a != nl || (FULL && e.b - e.m != vl))
            continue;
        // (a name is directly followed by its value on both sides)
        if (!dyn_same(r, a, t.tb, e.a, FULL ? nl + vl : nl))
            continue;
        *best = abs;
        found = true;
    }
    return found;
}

// The header with name r[a, m) and value r[m, b), hashed to h1 and h2,
// against the static table and the entries in [lo, hi), in the reference's
// order: static full, dynamic full, static name, dynamic name, literal.
// x: what the index build XOR-ed into its entries' first slots.
template <class R, class TB, class P>
QH_HDI DynHit
dyn_lookup(const R &r, uint32_t a, uint32_t m, uint32_t b, uint32_t h1,
           uint32_t h2, const StaticTable &st, const DynTab<TB, P> &t,
           uint32_t lo, uint32_t hi, uint32_t x = 0)
{
    const StaticHit s = static_lookup(r, a, m, b, h1, h2, st);
    if (s.kind == QHUFF_LINE_INDEXED || hi <= lo)
        return DynHit{s.kind, s.id, QHUFF_DYN_NONE};
    const uint32_t nl = m - a, vl = b - m;
    uint32_t best = 0;
    if (dyn_probe<true>(r, a, nl, vl, h2 ^ x, t, lo, hi, &best))
        return DynHit{QHUFF_LINE_INDEXED | QHUFF_LINE_DYN, QHUFF_STATIC_NONE,
                      best};
    if (s.kind == QHUFF_LINE_NAMEREF)
        return DynHit{s.kind, s.id, QHUFF_DYN_NONE};
    if (dyn_probe<false>(r, a, nl, vl, h1 ^ x, t, lo, hi, &best))
        return DynHit{QHUFF_LINE_NAMEREF | QHUFF_LINE_DYN, QHUFF_STATIC_NONE,
                      best};
    return DynHit{QHUFF_LINE_LITERAL, QHUFF_STATIC_NONE, QHUFF_DYN_NONE};
}

// A window [lo, hi) clamped into the table [first, first + d] (64-bit: the
// device form does not know that first + d fits 32 bits); max_entries = 0:
// empty
struct DynRange
{
    uint32_t lo, hi;
};

QH_HDI DynRange
dyn_window(uint64_t lo, uint64_t hi, uint32_t first, uint32_t d,
           uint32_t max_entries)
{
    const uint64_t t0 = first;
    uint64_t t1 = (uint64_t) first + d;
    t1 = t1 > 0xffffffffull ? 0xffffffffull : t1;
    lo = lo < t0 ? t0 : lo > t1 ? t1 : lo;
    hi = hi < lo ? lo : hi > t1 ? t1 : hi;
    if (!max_entries)
        hi = lo;
    return DynRange{(uint32_t) lo, (uint32_t) hi};
}

// a section's Base: at most first + d (below `first` is legal: every entry
// is then named post-base)
QH_HDI uint32_t
dyn_base(uint64_t base, uint32_t first, uint32_t d)
{
    uint64_t t1 = (uint64_t) first + d;
    t1 = t1 > 0xffffffffull ? 0xffffffffull : t1;
    return (uint32_t) (base > t1 ? t1 : base);
}

// The host and _cpu forms' check of a table, of m windows (sec_win null:
// the whole table, once) and of m Bases (or null): QHUFF_OK, QHUFF_EINVAL (a
// null pointer with d != 0, decreasing offsets, a window or a Base outside
// the rule of include/qhuff.h) or QHUFF_ERANGE (first + d passes 2^32 - 1, d
// passes 2^28).
inline int
dyn_enc_check(const ::qhuff_dyn_table *t, const uint32_t *sec_win,
              const uint32_t *sec_base, uint32_t m)
{
    if (!t || (t->d && (!t->off || !t->bytes)))
        return QHUFF_EINVAL;
    if ((uint64_t) t->first + t->d > 0xffffffffull || t->d > kDynMaxD)
        return QHUFF_ERANGE;
    for (uint64_t i = 0; i < 2ull * t->d; ++i)
        if (t->off[i + 1] < t->off[i])
            return QHUFF_EINVAL;
    const uint64_t t0 = t->first, t1 = t0 + t->d;
    if (!sec_win && m && t->max_entries && t->d > t->max_entries)
        return QHUFF_EINVAL;
    for (uint64_t s = 0; s < m; ++s)
    {
        if (sec_win)
        {
            const uint64_t lo = sec_win[2 * s], hi = sec_win[2 * s + 1];
            if (lo < t0 || hi < lo || hi > t1
                    || (t->max_entries && hi - lo > t->max_entries))
                return QHUFF_EINVAL;
        }
        if (sec_base && sec_base[s] > t1)
            return QHUFF_EINVAL;
    }
    return QHUFF_OK;
}

// ---- items ------------------------------------------------------------------
// {ival, int_bits | int_first << 8 | str_bits << 16 | str_first << 24} of a
// line's two items (struct qhuff_item twice), as four words

struct ItemWords
{
    uint32_t w[4];
};

// the line of a hit, in a section of Base `base`; nbit: the header's N
QH_HDI ItemWords
dyn_line_items(const DynHit &hit, uint32_t base, uint32_t nbit)
{
    const bool post = hit.dyn != QHUFF_DYN_NONE && hit.dyn >= base;
    const uint32_t rel = post ? hit.dyn - base : base - 1 - hit.dyn;
    switch (hit.kind)
    {
    case QHUFF_LINE_INDEXED:
        return ItemWords{{hit.id, 6u | 0xC0u << 8, 0, 0}};
    case QHUFF_LINE_INDEXED | QHUFF_LINE_DYN:
        // 10 + 6 bits (EHA_INDEXED_DYN, lsqpack.c:2051-2060), or 0001 + 4
        // bits post-base (2042-2050); no N bit
        return post ? ItemWords{{rel, 4u | 0x10u << 8, 0, 0}}
                    : ItemWords{{rel, 6u | 0x80u << 8, 0, 0}};
    case QHUFF_LINE_NAMEREF:
        return ItemWords{{hit.id, 4u | (0x50u | nbit << 5) << 8, 0,
                          7u << 16}};
    case QHUFF_LINE_NAMEREF | QHUFF_LINE_DYN:
        // 01N0 + 4 bits (EHA_LIT_WITH_NAME_DYN, 2093-2109), or 0000N + 3
        // bits post-base (2079-2092)
        return post ? ItemWords{{rel, 3u | (nbit << 3) << 8, 0, 7u << 16}}
                    : ItemWords{{rel, 4u | (0x40u | nbit << 5) << 8, 0,
                                 7u << 16}};
    default:
        return ItemWords{{0, 3u << 16 | (0x20u | nbit << 4) << 24, 0,
                          7u << 16}};
    }
}

// a section's two prefix items (lsqpack.c:1267-1298): ric = the Required
// Insert Count (1 + the largest absolute index named, 0: none)
QH_HDI ItemWords
dyn_prefix_items(uint32_t ric, uint32_t base, uint32_t max_entries)
{
    if (!ric || !max_entries)
        return ItemWords{{0, 8, 0, 7}};
    const uint32_t enc = (uint32_t) (ric % (2ull * max_entries)) + 1;
    if (base >= ric)
        return ItemWords{{enc, 8, base - ric, 7}};
    return ItemWords{{enc, 8, ric - base - 1, 7u | 0x80u << 8}};
}

}  // namespace qhuff
