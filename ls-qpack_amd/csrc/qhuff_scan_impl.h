// qhuff_scan_impl.h -- the framing walker of qhuff_scan_sections: one chunk
// of QPACK wire data (a field section, or encoder-stream bytes) walked
// serially, its literals reported to a sink.
//
// The same source runs in two places: as device code, one chunk a lane
// (qhuff_scan.hip), and as plain C++ on the host (qhuff_scan_sections_cpu,
// qhuff_frames.cpp, which also builds with g++ alone).  It restates the
// rules of the host scanners (qhuff_scan_field_section and
// qhuff_scan_encoder_stream, qhuff_frames.cpp, which stay the independent
// implementation the tests compare with), i.e. the reference's
// lsqpack_dec_int / _int24 (lsqpack.c:2372-2460), parse_header_prefix /
// parse_header_data (lsqpack.c:3955-4046, 3567-3915) and lsqpack_dec_enc_in
// (lsqpack.c:4574-4960).
//
// A walker sees its bytes only through a reader, `uint8_t R::get(uint32_t
// pos)`, pos an offset into the wire buffer, and asks only for pos inside
// its own chunk: bytes outside a chunk cannot affect its result.
#pragma once
#include <stdint.h>

#include "../../include/qhuff.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define QH_HD __host__ __device__
#else
#define QH_HD
#endif

namespace qhuff {
namespace scan {

// a literal as the walker found it; offsets into the wire buffer
struct Lit
{
    uint32_t pos, len;
    uint8_t h, bits, kind, hdr;
};

QH_HD inline ::qhuff_literal
descriptor(const Lit &l, uint32_t instr)
{
    ::qhuff_literal d;
    d.pos = l.pos;
    d.len = l.len;
    d.huffman = l.h;
    d.prefix_bits = l.bits;
    d.kind = l.kind;
    d.hdr_len = l.hdr;
    d.instr = instr;
    return d;
}

// sinks: put(l, instr) takes the next literal, n counts them; a walker may
// set n back (an encoder-stream instruction that turns out partial)
struct CountSink
{
    uint32_t n;
    QH_HD void put(const Lit &, uint32_t) { ++n; }
};

// descriptors with indices in [n0, limit) are written.  The limit is both
// max_lits and the end of the chunk's own range: the literal of a partial
// instruction, counted and then taken back, lies at or past it -- in the
// next chunk's range, which another lane writes.
struct WriteSink
{
    ::qhuff_literal *lits;
    uint32_t n, limit;
    QH_HD void put(const Lit &l, uint32_t instr)
    {
        if (n < limit)
            lits[n] = descriptor(l, instr);
        ++n;
    }
};

// lsqpack_dec_int on a complete buffer [.., end): 0 ok, -1 the buffer ends
// inside the integer, -2 the value does not fit 64 bits
template <class R>
QH_HD inline int
dec_int(R &r, uint32_t *pp, uint32_t end, unsigned prefix_bits, uint64_t *v_out)
{
    uint32_t p = *pp;
    if (p >= end)
        return -1;
    const unsigned pmax = (1u << prefix_bits) - 1;
    uint64_t v = r.get(p++) & pmax;
    if (v < pmax)
    {
        *pp = p;
        *v_out = v;
        return 0;
    }
    unsigned M = 0;
    uint8_t B;
    do
    {
        if (p >= end)
            return -1;
        B = r.get(p++);
        v += (uint64_t) (B & 0x7f) << M;
        M += 7;
    } while ((B & 0x80) && M < 64);
    if (M <= 63 || (M == 70 && B <= 1 && (v & (1ull << 63))))
    {
        *pp = p;
        *v_out = v;
        return 0;
    }
    return -2;
}

// lsqpack_dec_int24: values >= 2^24 are errors
template <class R>
QH_HD inline int
dec_int24(R &r, uint32_t *pp, uint32_t end, unsigned prefix_bits,
          uint32_t *v_out)
{
    uint64_t v;
    const int rc = dec_int(r, pp, end, prefix_bits, &v);
    if (rc)
        return rc;
    if (v >= (1u << 24))
        return -2;
    *v_out = (uint32_t) v;
    return 0;
}

// a string literal whose H bit sits just above its N-bit length prefix;
// max_len > 0: a declared length above it is an error before the payload is
// looked for (the field-section rule)
template <class R, class S>
QH_HD inline int
literal(R &r, S &s, uint32_t *pp, uint32_t end, unsigned prefix_bits,
        unsigned kind, uint32_t instr, uint32_t max_len)
{
    uint32_t p = *pp;
    if (p >= end)
        return -1;
    const uint32_t start = p;
    Lit l;
    l.h = (uint8_t) ((r.get(p) >> prefix_bits) & 1);
    const int rc = dec_int24(r, &p, end, prefix_bits, &l.len);
    if (rc)
        return rc;
    if (max_len && l.len > max_len)
        return -2;
    if (end - p < l.len)
        return -1;
    l.pos = p;
    l.bits = (uint8_t) prefix_bits;
    l.kind = (uint8_t) kind;
    l.hdr = (uint8_t) (p - start);
    s.put(l, instr);
    *pp = p + l.len;
    return 0;
}

// one complete field section in [p, end): 0, -1 (ends inside a line) or -2
template <class R, class S>
QH_HD inline int
walk_field_section(R &r, S &s, uint32_t p, uint32_t end)
{
    const uint32_t max_str = QHUFF_MAX_STRLEN;
    uint64_t v;
    int rc;
    // section prefix: Required Insert Count (8-bit prefix), S + Delta Base
    // (7-bit prefix)
    if ((rc = dec_int(r, &p, end, 8, &v)) || (rc = dec_int(r, &p, end, 7, &v)))
        return rc;
    while (p < end)
    {
        const uint8_t b = r.get(p);
        const uint32_t at = p;
        uint32_t idx;
        if (b & 0x80)                          // 1Txxxxxx indexed field line
            rc = dec_int24(r, &p, end, 6, &idx);
        else if (b & 0x40)                     // 01NTxxxx literal, name ref
        {
            rc = dec_int24(r, &p, end, 4, &idx);
            if (!rc)
                rc = literal(r, s, &p, end, 7, QHUFF_LIT_VALUE, at, max_str);
        }
        else if (b & 0x20)                     // 001NHxxx literal name
        {
            rc = literal(r, s, &p, end, 3, QHUFF_LIT_NAME, at, max_str);
            if (!rc)
                rc = literal(r, s, &p, end, 7, QHUFF_LIT_VALUE, at, max_str);
        }
        else if (b & 0x10)                     // 0001xxxx indexed post-base
            rc = dec_int24(r, &p, end, 4, &idx);
        else                                   // 0000Nxxx post-base name ref
        {
            rc = dec_int24(r, &p, end, 3, &idx);
            if (!rc)
                rc = literal(r, s, &p, end, 7, QHUFF_LIT_VALUE, at, max_str);
        }
        if (rc)
            return rc;
    }
    return 0;
}

// encoder-stream bytes in [p, end): 0 with *stop the end of the last
// complete instruction (a partial one is left, its literals taken back), or
// -2
template <class R, class S>
QH_HD inline int
walk_encoder_stream(R &r, S &s, uint32_t p, uint32_t end, uint32_t *stop)
{
    while (p < end)
    {
        uint32_t q = p;
        const uint8_t b = r.get(q);
        const uint32_t n0 = s.n;
        uint32_t v;
        int rc;
        if (b & 0x80)                // 1Txxxxxx insert with name reference
        {
            rc = dec_int24(r, &q, end, 6, &v);
            if (!rc)
                rc = literal(r, s, &q, end, 7, QHUFF_LIT_VALUE, p, 0);
        }
        else if (b & 0x40)           // 01Hxxxxx insert with literal name
        {
            rc = literal(r, s, &q, end, 5, QHUFF_LIT_NAME, p, 0);
            if (!rc)
                rc = literal(r, s, &q, end, 7, QHUFF_LIT_VALUE, p, 0);
        }
        else                         // 001xxxxx capacity / 000xxxxx dup
        {
            uint64_t w;
            rc = dec_int(r, &q, end, 5, &w);
            if (!rc && !(b & 0x20) && w >= (1u << 24))
                rc = -2;
        }
        if (rc == -1)
        {
            s.n = n0;
            break;
        }
        if (rc)
            return rc;
        p = q;
    }
    *stop = p;
    return 0;
}

// One chunk [a, b) in `mode`: its QHUFF_* result and its consumed bytes;
// the sink's n has advanced by the chunk's literals, or is back where it
// was when the result is not QHUFF_OK.
template <class R, class S>
QH_HD inline int
walk_chunk(R &r, S &s, unsigned mode, uint32_t a, uint32_t b,
           uint32_t *consumed)
{
    const uint32_t n0 = s.n;
    uint32_t stop = b;
    const int rc = mode == QHUFF_SCAN_FIELD_SECTION
                       ? walk_field_section(r, s, a, b)
                       : walk_encoder_stream(r, s, a, b, &stop);
    if (rc)
    {
        s.n = n0;
        *consumed = 0;
        return rc == -1 ? QHUFF_ETRUNC : QHUFF_EPROTO;
    }
    *consumed = stop - a;
    return QHUFF_OK;
}

// ---- header lines (qhuff_scan_headers) --------------------------------------
//
// The same sections walked for their header lines: what the reference's
// decoder does per line when the dynamic table is not used
// (header_out_static_entry, header_out_begin_static_nameref,
// header_out_begin_literal: lsqpack.c:3013-3057, 3121-3159, 3211-3323).

// a literal() sink that keeps the literal for the line it belongs to
struct LitCatch
{
    Lit l;
    QH_HD void put(const Lit &x, uint32_t) { l = x; }
};

QH_HD inline ::qhuff_hstr
hstr_wire(const Lit &l, uint32_t kind, uint32_t at)
{
    ::qhuff_hstr d;
    d.pos = l.pos;
    d.len = l.len;
    d.huffman = l.h;
    d.source = QHUFF_HSTR_WIRE;
    d.kind = (uint8_t) kind;
    d.static_id = QHUFF_STATIC_NONE;
    d.instr = at;
    return d;
}

QH_HD inline ::qhuff_hstr
hstr_static(uint32_t id, uint32_t kind, uint32_t at)
{
    ::qhuff_hstr d;
    d.pos = at;
    d.len = 0;
    d.huffman = 0;
    d.source = QHUFF_HSTR_STATIC;
    d.kind = (uint8_t) kind;
    d.static_id = (uint8_t) id;
    d.instr = at;
    return d;
}

// header sinks: line(kind, id, nbit, at, name, value) takes the next header
// line -- kind QHUFF_LINE_*, id its static index (any for LITERAL), at its
// first byte, name / value its literals where the kind has them
struct HdrCountSink
{
    uint32_t n;
    QH_HD void line(uint32_t, uint32_t, uint32_t, uint32_t, const Lit &,
                    const Lit &)
    {
        ++n;
    }
};

// headers with indices in [n0, limit) are written: two descriptors and a
// byte of each array that is there
struct HdrWriteSink
{
    ::qhuff_hstr *strs;
    uint8_t *kind, *static_id, *hflags;
    uint32_t n, limit;
    QH_HD void line(uint32_t k, uint32_t id, uint32_t nbit, uint32_t at,
                    const Lit &name, const Lit &value)
    {
        if (n < limit)
        {
            const uint64_t i = 2 * (uint64_t) n;
            strs[i] = k == QHUFF_LINE_LITERAL
                          ? hstr_wire(name, QHUFF_LIT_NAME, at)
                          : hstr_static(id, QHUFF_LIT_NAME, at);
            strs[i + 1] = k == QHUFF_LINE_INDEXED
                              ? hstr_static(id, QHUFF_LIT_VALUE, at)
                              : hstr_wire(value, QHUFF_LIT_VALUE, at);
            if (kind)
                kind[n] = (uint8_t) k;
            if (static_id)
                static_id[n] = (uint8_t) (k == QHUFF_LINE_LITERAL
                                              ? QHUFF_STATIC_NONE : id);
            if (hflags)
                hflags[n] = (uint8_t) (nbit ? QHUFF_HDR_NEVER_INDEX : 0);
        }
        ++n;
    }
};

constexpr uint32_t kHdrStaticEntries = 99;    // lsqpack.c:3021, 3130

// ---- the dynamic table as a section's walk sees it (qhuff_scan_headers_dyn) --
//
// walk_header_lines / walk_header_section take a table policy.  NoDyn: there
// is no table, a section that needs one is QHUFF_ENOTSUP (qhuff_scan_headers;
// nothing of what follows is compiled into that walk).  DynWin: the table's
// offsets and the section's window, for the read the reference's decoder does
// per dynamic line (qdec_get_table_entry_abs, lsqpack.c:2768-2775;
// header_out_dynamic_entry, 3060-3117; header_out_begin_dynamic_nameref).
struct NoDyn
{
    static constexpr bool kOn = false;
};

struct DynWin
{
    static constexpr bool kOn = true;
    const uint32_t *off;                 // the table's 2d + 1 offsets
    uint32_t first, max_entries;
    uint64_t lo, ins;                    // the window, inside [first, first + d]

    // section s's window from sec_win (or the whole table), clamped into the
    // table: whatever sec_win holds, an index inside [lo, ins) has its three
    // offsets inside `off`
    QH_HD static DynWin of(const uint32_t *off, uint32_t d, uint32_t first,
                           uint32_t max_entries, const uint32_t *sec_win,
                           uint64_t s)
    {
        DynWin w;
        w.off = off;
        w.first = first;
        w.max_entries = max_entries;
        const uint64_t t0 = first, t1 = (uint64_t) first + d;
        w.lo = sec_win ? sec_win[2 * s] : t0;
        w.ins = sec_win ? sec_win[2 * s + 1] : t1;
        w.lo = w.lo < t0 ? t0 : w.lo;
        w.ins = w.ins > t1 ? t1 : w.ins;
        return w;
    }
};

// ---- a set of tables and a table per section (struct qhuff_dyn_tables) ------
//
// Table c of a set as one table: its entries are the ordinals [e0, e0 + d)
// of the shared arrays.
struct TabView
{
    uint32_t c, e0, d, first, max_entries;
};

// The table of section s.  P: a pointer to const uint32_t (plain, or in the
// global address space).  Whatever the arrays hold: sec_tab[s] is clamped to
// T - 1 and ent values to D, a decreasing pair is an empty table, so e0 + d
// <= D.  T = 0 (or no sec_tab): a table with d = 0 and max_entries = 0.
template <class P>
QH_HD inline TabView
tab_view(P ent, P first, P max_entries, uint32_t T, uint32_t D, P sec_tab,
         uint64_t s)
{
    if (!T || !sec_tab)
        return TabView{0, 0, 0, 0, 0};
    uint32_t c = sec_tab[s];
    c = c < T ? c : T - 1;
    uint32_t e0 = ent[c], e1 = ent[c + 1];
    e0 = e0 < D ? e0 : D;
    e1 = e1 < D ? e1 : D;
    return TabView{c, e0, e1 > e0 ? e1 - e0 : 0u, first[c], max_entries[c]};
}

// DynWin::of for section s of a batch over a set of tables: one load of
// sec_tab[s], then the table's four words; the offsets based at the table's
// first entry, the window clamped into the table
QH_HD inline DynWin
dyn_win_tabs(const uint32_t *off, const uint32_t *ent, const uint32_t *first,
             const uint32_t *max_entries, uint32_t T, uint32_t D,
             const uint32_t *sec_tab, const uint32_t *sec_win, uint64_t s)
{
    const TabView v = tab_view(ent, first, max_entries, T, D, sec_tab, s);
    return DynWin::of(off + 2ull * v.e0, v.d, v.first, v.max_entries, sec_win,
                      s);
}

// the host forms' check of a table and of m windows: QHUFF_OK, QHUFF_EINVAL
// (a null pointer with d != 0, decreasing offsets, a window outside the
// rule) or QHUFF_ERANGE (first + d passes 2^32 - 1); *longest = the longest
// name + value
inline int
dyn_check(const ::qhuff_dyn_table *t, const uint32_t *sec_win, uint32_t m,
          uint32_t *longest)
{
    *longest = 0;
    if (!t || (t->d && (!t->off || !t->bytes)))
        return QHUFF_EINVAL;
    if ((uint64_t) t->first + t->d > 0xffffffffull)
        return QHUFF_ERANGE;
    for (uint64_t i = 0; i < 2ull * t->d; ++i)
        if (t->off[i + 1] < t->off[i])
            return QHUFF_EINVAL;
    for (uint64_t k = 0; k < t->d; ++k)
    {
        const uint32_t l = t->off[2 * k + 2] - t->off[2 * k];
        *longest = l > *longest ? l : *longest;
    }
    for (uint64_t s = 0; sec_win && s < m; ++s)
        if (sec_win[2 * s] < t->first || sec_win[2 * s + 1] < sec_win[2 * s]
                || sec_win[2 * s + 1] > t->first + t->d)
            return QHUFF_EINVAL;
    return QHUFF_OK;
}

QH_HD inline ::qhuff_hstr
hstr_dyn(uint32_t toff, uint32_t len, uint32_t kind, uint32_t at)
{
    ::qhuff_hstr d;
    d.pos = at;
    d.len = len;
    d.huffman = 0;
    d.source = QHUFF_HSTR_DYN;
    d.kind = (uint8_t) kind;
    d.static_id = QHUFF_STATIC_NONE;
    d.instr = toff;
    return d;
}

// HdrCountSink for a walk with a table: dyn_line(kind, abs, nbit, at, value,
// table) takes a line that names the dynamic entry `abs`
struct HdrDynCountSink
{
    uint32_t n;
    QH_HD void line(uint32_t, uint32_t, uint32_t, uint32_t, const Lit &,
                    const Lit &)
    {
        ++n;
    }
    QH_HD void dyn_line(uint32_t, uint64_t, uint32_t, uint32_t, const Lit &,
                        const DynWin &)
    {
        ++n;
    }
};

// HdrWriteSink for a walk with a table: the entry's name and value come from
// its three offsets (a decreasing pair counts as an empty string)
struct HdrDynWriteSink
{
    HdrWriteSink w;
    uint32_t *dyn_id;
    QH_HD void line(uint32_t k, uint32_t id, uint32_t nbit, uint32_t at,
                    const Lit &name, const Lit &value)
    {
        if (w.n < w.limit && dyn_id)
            dyn_id[w.n] = QHUFF_DYN_NONE;
        w.line(k, id, nbit, at, name, value);
    }
    QH_HD void dyn_line(uint32_t k, uint64_t abs, uint32_t nbit, uint32_t at,
                        const Lit &value, const DynWin &t)
    {
        if (w.n < w.limit)
        {
            const uint64_t e = 2 * (abs - t.first);
            const uint32_t o0 = t.off[e], o1 = t.off[e + 1], o2 = t.off[e + 2];
            const uint64_t i = 2 * (uint64_t) w.n;
            w.strs[i] = hstr_dyn(o0, o1 > o0 ? o1 - o0 : 0u, QHUFF_LIT_NAME, at);
            w.strs[i + 1] = k == QHUFF_LINE_INDEXED
                ? hstr_dyn(o1, o2 > o1 ? o2 - o1 : 0u, QHUFF_LIT_VALUE, at)
                : hstr_wire(value, QHUFF_LIT_VALUE, at);
            if (w.kind)
                w.kind[w.n] = (uint8_t) (k | QHUFF_LINE_DYN);
            if (w.static_id)
                w.static_id[w.n] = QHUFF_STATIC_NONE;
            if (w.hflags)
                w.hflags[w.n] = (uint8_t) (nbit ? QHUFF_HDR_NEVER_INDEX : 0);
            if (dyn_id)
                dyn_id[w.n] = (uint32_t) abs;
        }
        ++w.n;
    }
};

// the sink's count, whichever sink
QH_HD inline uint32_t &sink_n(HdrCountSink &s) { return s.n; }
QH_HD inline uint32_t &sink_n(HdrWriteSink &s) { return s.n; }
QH_HD inline uint32_t &sink_n(HdrDynCountSink &s) { return s.n; }
QH_HD inline uint32_t &sink_n(HdrDynWriteSink &s) { return s.w.n; }

// One complete field section in [p, end) walked for its header lines: the
// framing result of walk_field_section (0, -1 or -2) -- the walk goes on to
// the section's end whatever the lines mean, so that a framing error wins --
// and in *flags
//   bit 0  the section needs the dynamic table and there is none (NoDyn:
//          Required Insert Count != 0 or a dynamic form);
//   bit 1  a static index >= 99; with a table also: a dynamic line with a
//          Required Insert Count of 0 or an index outside the window, or no
//          line that names Required Insert Count - 1;
//   bit 2  (table) the encoded Required Insert Count is above 2 * MaxEntries,
//          or the count it stands for is not positive;
//   bit 3  (table) the Required Insert Count is above the section's inserts.
// Lines are reported until the first flag is raised.
template <class R, class S, class D>
QH_HD inline int
walk_header_lines(R &r, S &s, uint32_t p, uint32_t end, uint32_t *flags,
                  const D &dy)
{
    const uint32_t max_str = QHUFF_MAX_STRLEN;
    uint64_t ric, v;
    int rc;
    uint32_t f = 0;
    *flags = 0;
    // (no table: the Delta Base and its sign are read and ignored)
    if ((rc = dec_int(r, &p, end, 8, &ric)))
        return rc;
    [[maybe_unused]] bool sign = false;
    if constexpr (D::kOn)
        sign = p < end && (r.get(p) & 0x80);
    if ((rc = dec_int(r, &p, end, 7, &v)))
        return rc;
    [[maybe_unused]] uint64_t base = 0;
    [[maybe_unused]] bool named = false;     // a line named ric - 1
    if constexpr (D::kOn)
    {
        // the Required Insert Count the encoded one stands for (RFC 9204
        // 4.5.1.1; the reference's modular ids, lsqpack.c:2749-2753,
        // 3914-3923, 3973-3981): the value == ric - 1 (mod 2 * MaxEntries)
        // in [ins - MaxEntries + 1, ins + MaxEntries]
        const int64_t me = dy.max_entries, full = 2 * me;
        if (ric > (uint64_t) full)
            f |= 4;
        else if (ric)
        {
            const int64_t lo = (int64_t) dy.ins - me + 1;
            int64_t m = ((int64_t) ric - 1 - lo) % full;
            m += m < 0 ? full : 0;
            const int64_t req = lo + m;
            if (req <= 0)
                f |= 4;
            else if ((uint64_t) req > dy.ins)
                f |= 8;
            ric = (uint64_t) req;
        }
        // (lsqpack.c:4015-4022; two's complement, 64 bits)
        base = sign ? ric - v - 1 : ric + v;
    }
    else if (ric)
        f |= 1;
    while (p < end)
    {
        const uint8_t b = r.get(p);
        const uint32_t at = p;
        uint32_t idx = 0, k = QHUFF_LINE_LITERAL, nbit = 0;
        bool dyn = false;
        [[maybe_unused]] bool post = false;
        LitCatch name, value;
        name.l = Lit();
        value.l = Lit();
        if (b & 0x80)                          // 1Txxxxxx indexed field line
        {
            rc = dec_int24(r, &p, end, 6, &idx);
            k = QHUFF_LINE_INDEXED;
            dyn = !(b & 0x40);
        }
        else if (b & 0x40)                     // 01NTxxxx literal, name ref
        {
            rc = dec_int24(r, &p, end, 4, &idx);
            if (!rc)
                rc = literal(r, value, &p, end, 7, QHUFF_LIT_VALUE, at,
                             max_str);
            k = QHUFF_LINE_NAMEREF;
            nbit = b & 0x20;
            dyn = !(b & 0x10);
        }
        else if (b & 0x20)                     // 001NHxxx literal name
        {
            rc = literal(r, name, &p, end, 3, QHUFF_LIT_NAME, at, max_str);
            if (!rc)
                rc = literal(r, value, &p, end, 7, QHUFF_LIT_VALUE, at,
                             max_str);
            nbit = b & 0x10;
        }
        else if (b & 0x10)                     // 0001xxxx indexed post-base
        {
            rc = dec_int24(r, &p, end, 4, &idx);
            dyn = true;
            if constexpr (D::kOn)
            {
                k = QHUFF_LINE_INDEXED;
                post = true;
            }
        }
        else                                   // 0000Nxxx post-base name ref
        {
            rc = dec_int24(r, &p, end, 3, &idx);
            if (!rc)
                rc = literal(r, value, &p, end, 7, QHUFF_LIT_VALUE, at,
                             max_str);
            dyn = true;
            if constexpr (D::kOn)
            {
                k = QHUFF_LINE_NAMEREF;
                nbit = b & 0x08;
                post = true;
            }
        }
        if (rc)
            return rc;
        if constexpr (D::kOn)
        {
            if (dyn)
            {
                // (an index below 0 is a large one here: outside any window)
                const uint64_t abs = post ? base + idx : base - 1 - idx;
                if (!ric || abs < dy.lo || abs >= dy.ins)
                    f |= 2;
                else
                {
                    named |= abs == ric - 1;
                    if (!f)
                        s.dyn_line(k, abs, nbit, at, value.l, dy);
                }
                continue;
            }
        }
        if (dyn)
            f |= 1;
        else if (k != QHUFF_LINE_LITERAL && idx >= kHdrStaticEntries)
            f |= 2;
        if (!f)
            s.line(k, idx, nbit, at, name.l, value.l);
    }
    if constexpr (D::kOn)
        if (ric && !named)
            f |= 2;
    *flags = f;
    return 0;
}

// One section [a, b): its QHUFF_* result in the order of qhuff_scan_headers
// (NoDyn) or of qhuff_scan_headers_dyn; the sink's n has advanced by the
// section's headers, or is back where it was when the result is not QHUFF_OK.
template <class R, class S, class D>
QH_HD inline int
walk_header_section(R &r, S &s, uint32_t a, uint32_t b, const D &dy)
{
    const uint32_t n0 = sink_n(s);
    uint32_t flags;
    const int rc = walk_header_lines(r, s, a, b, &flags, dy);
    if (!rc && !flags)
        return QHUFF_OK;
    sink_n(s) = n0;
    if constexpr (D::kOn)
        if (!rc && (flags & 12))
            return (flags & 4) ? QHUFF_EPROTO : QHUFF_EBLOCKED;
    return rc == -1 ? QHUFF_ETRUNC
         : rc ? QHUFF_EPROTO
         : (flags & 1) ? QHUFF_ENOTSUP : QHUFF_EPROTO;
}

template <class R, class S>
QH_HD inline int
walk_header_section(R &r, S &s, uint32_t a, uint32_t b)
{
    return walk_header_section(r, s, a, b, NoDyn());
}

// ---- encoder-stream inserts (qhuff_scan_inserts_tabs) ------------------------
//
// walk_encoder_stream's four instructions walked for what they mean
// (lsqpack_dec_enc_in, lsqpack.c:4574-5030): every insert goes to a sink with
// the capacity it is checked and pushed under.  The capacity of a chunk is a
// function of cap[c] and the chunk's Set Capacity instructions alone, so the
// walk tracks it; what depends on decoded sizes -- the liveness of a
// reference, N > cap, the value's length, the push -- is the accounting's
// (qhuff_tabs_insert_impl.h).  A verdict is given on complete instructions.
//
// Sinks: insert(kind, idx, at, name, value, cmin, cap) takes the next insert
// -- kind QHUFF_INS_*, idx its static or relative index, at its first byte,
// cmin the lowest capacity since the previous insert (cap included), cap the
// one in force; tail(cmin, cap): the same behind the last insert.
struct InsCountSink
{
    uint32_t n, cmin, cap;
    QH_HD void insert(uint32_t, uint32_t, uint32_t, const Lit &, const Lit &,
                      uint32_t, uint32_t)
    {
        ++n;
    }
    QH_HD void tail(uint32_t m, uint32_t c)
    {
        cmin = m;
        cap = c;
    }
};

// Inserts with ordinals in [n0, limit) are written: two descriptors, two
// roots, the two capacities, the reference and the kind.  off: the set's
// offsets based at the table's first entry (d entries from the absolute index
// first).  A reference to an insert of the same chunk is a DYN descriptor of
// length 0 whose root is that insert's string, or that string's own root: the
// lane reads back what it wrote itself, earlier in program order.
struct InsWriteSink
{
    ::qhuff_hstr *strs;
    uint32_t *root, *ins_cap, *ins_ref;
    uint8_t *ins_kind;
    const uint32_t *off;
    uint32_t d, first;
    uint32_t n0, n, limit;

    QH_HD uint32_t root_of(uint64_t s) const
    {
        const uint32_t r = root[s];
        return r == QHUFF_DYN_NONE ? (uint32_t) s : r;
    }
    QH_HD void insert(uint32_t kind, uint32_t idx, uint32_t at,
                      const Lit &name, const Lit &value, uint32_t cmin,
                      uint32_t cap)
    {
        if (n < limit)
        {
            const uint64_t i = 2 * (uint64_t) n;
            const uint64_t ins0 = (uint64_t) first + d, ins = ins0 + (n - n0);
            uint32_t ref = QHUFF_DYN_NONE, rn = QHUFF_DYN_NONE,
                     rv = QHUFF_DYN_NONE;
            ::qhuff_hstr sn, sv = hstr_wire(value, QHUFF_LIT_VALUE, at);
            if (kind == QHUFF_INS_LITERAL)
                sn = hstr_wire(name, QHUFF_LIT_NAME, at);
            else if (kind == QHUFF_INS_STATIC)
                sn = hstr_static(idx, QHUFF_LIT_NAME, at);
            else
            {
                const bool dup = kind == QHUFF_INS_DUP;
                sn = hstr_dyn(0, 0, QHUFF_LIT_NAME, at);
                if (dup)
                    sv = hstr_dyn(0, 0, QHUFF_LIT_VALUE, at);
                if (idx < ins)
                {
                    const uint64_t a = ins - 1 - idx;
                    ref = (uint32_t) a;
                    if (a >= ins0)
                    {
                        // (a - ins0 < n - n0: an ordinal this lane wrote)
                        const uint64_t k = 2 * (n0 + (a - ins0));
                        rn = root_of(k);
                        if (dup)
                            rv = root_of(k + 1);
                    }
                    else if (a >= first)
                    {
                        const uint64_t e = 2 * (a - first);
                        const uint32_t o0 = off[e], o1 = off[e + 1],
                                       o2 = off[e + 2];
                        sn = hstr_dyn(o0, o1 > o0 ? o1 - o0 : 0u,
                                      QHUFF_LIT_NAME, at);
                        if (dup)
                            sv = hstr_dyn(o1, o2 > o1 ? o2 - o1 : 0u,
                                          QHUFF_LIT_VALUE, at);
                    }
                }
            }
            strs[i] = sn;
            strs[i + 1] = sv;
            root[i] = rn;
            root[i + 1] = rv;
            ins_cap[i] = cmin;
            ins_cap[i + 1] = cap;
            ins_ref[n] = ref;
            ins_kind[n] = (uint8_t) kind;
        }
        ++n;
    }
    QH_HD void tail(uint32_t, uint32_t) {}
};

// encoder-stream bytes in [p, end) of a table with capacity cap and maximum
// max_cap: 0 with *stop the end of the last complete instruction, or -2
template <class R, class S>
QH_HD inline int
walk_insert_stream(R &r, S &s, uint32_t p, uint32_t end, uint32_t cap,
                   uint32_t max_cap, uint32_t *stop)
{
    uint32_t cmin = cap;
    while (p < end)
    {
        uint32_t q = p;
        const uint8_t b = r.get(q);
        uint32_t idx = 0, kind;
        LitCatch name, value;
        name.l = Lit();
        value.l = Lit();
        int rc;
        if (b & 0x80)                // 1Txxxxxx insert with name reference
        {
            kind = (b & 0x40) ? QHUFF_INS_STATIC : QHUFF_INS_DYN;
            rc = dec_int24(r, &q, end, 6, &idx);
            if (!rc)
                rc = literal(r, value, &q, end, 7, QHUFF_LIT_VALUE, p, 0);
            if (!rc && kind == QHUFF_INS_STATIC && idx >= kHdrStaticEntries)
                rc = -2;                             // lsqpack.c:4620-4623
        }
        else if (b & 0x40)           // 01Hxxxxx insert with literal name
        {
            kind = QHUFF_INS_LITERAL;
            rc = literal(r, name, &q, end, 5, QHUFF_LIT_NAME, p, 0);
            if (!rc)
                rc = literal(r, value, &q, end, 7, QHUFF_LIT_VALUE, p, 0);
            if (!rc && name.l.len > ((uint64_t) cap << 2 * name.l.h))
                rc = -2;                             // lsqpack.c:4798
        }
        else if (b & 0x20)           // 001xxxxx set dynamic table capacity
        {
            uint64_t w;
            rc = dec_int(r, &q, end, 5, &w);
            if (rc == -1)
                break;
            if (rc || w > max_cap)                   // lsqpack.c:5015
                return -2;
            cap = (uint32_t) w;
            cmin = cap < cmin ? cap : cmin;
            p = q;
            continue;
        }
        else                         // 000xxxxx duplicate
        {
            kind = QHUFF_INS_DUP;
            rc = dec_int24(r, &q, end, 5, &idx);
        }
        if (rc == -1)
            break;
        if (rc)
            return rc;
        s.insert(kind, idx, p, name.l, value.l, cmin, cap);
        cmin = cap;
        p = q;
    }
    *stop = p;
    s.tail(cmin, cap);
    return 0;
}

// the scan's view of table c of a set for its chunk: the entries' offsets
// based at the table's first entry, d, first (tab_view's clamps)
template <class P>
QH_HD inline TabView
ins_tab_view(P ent, P first, uint32_t D, uint32_t c)
{
    uint32_t e0 = ent[c], e1 = ent[c + 1];
    e0 = e0 < D ? e0 : D;
    e1 = e1 < D ? e1 : D;
    return TabView{c, e0, e1 > e0 ? e1 - e0 : 0u, first[c], 0};
}

}  // namespace scan
}  // namespace qhuff
