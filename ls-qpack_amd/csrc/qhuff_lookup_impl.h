// qhuff_lookup_impl.h -- one header against the static table: the first step
// of lsqpack_enc_encode (lsqpack.c:1671-1715, 1835-1866) when the dynamic
// table is not used.
//
// The same source runs as device code, one header a lane (qhuff_lookup.hip,
// over the reader the lane hashed its bytes with), and as plain C++ on the
// host (qhuff_static_lookup_cpu, qhuff_frames.cpp).  Hashes: qhuff_hash_impl.h;
// the table and its probe tables: qhuff_static.h.
#pragma once
#include <stdint.h>

#include "../../include/qhuff.h"
#include "qhuff_hash_impl.h"
#include "qhuff_static.h"

namespace qhuff {

struct StaticHit
{
    uint32_t kind;                       // QHUFF_LINE_*
    uint32_t id;                         // static index, or QHUFF_STATIC_NONE
};

// bytes [a, a + len) of r against the first len bytes of the entry whose
// words begin at `at`: four at a time, then the tail (the reader is asked
// for bytes of the header only)
template <class R>
QH_HDI bool
static_same(const R &r, uint32_t a, const StaticTable &t, uint32_t at,
            uint32_t len)
{
    uint32_t i = 0;
    for (; i + 4 <= len; i += 4)
        if (r.word(a + i) != t.words[at + i / 4])
            return false;
    for (; i < len; ++i)
        if (r.byte(a + i) != t.byte(at, i))
            return false;
    return true;
}

// The header with name r[a, m) and value r[m, b), hashed to h1 (name) and h2
// (value seeded with h1): find_in_static_full (lsqpack.c:721-740), else
// lsqpack_find_in_static_headers (lsqpack.c:747-764) -- probe, compare the
// lengths, then the bytes.
template <class R>
QH_HDI StaticHit
static_lookup(const R &r, uint32_t a, uint32_t m, uint32_t b, uint32_t h1,
              uint32_t h2, const StaticTable &t)
{
    const uint32_t nl = m - a, vl = b - m;
    uint32_t id = t.nameval2id[h2 % kStaticSlots];
    if (id)
    {
        --id;
        // (a name is directly followed by its value on both sides)
        if (t.name_len[id] == nl && t.val_len[id] == vl
                && static_same(r, a, t, t.at[id], nl + vl))
            return StaticHit{QHUFF_LINE_INDEXED, id};
    }
    id = t.name2id[h1 % kStaticSlots];
    if (id)
    {
        --id;
        if (t.name_len[id] == nl && static_same(r, a, t, t.at[id], nl))
            return StaticHit{QHUFF_LINE_NAMEREF, id};
    }
    return StaticHit{QHUFF_LINE_LITERAL, QHUFF_STATIC_NONE};
}

}  // namespace qhuff
