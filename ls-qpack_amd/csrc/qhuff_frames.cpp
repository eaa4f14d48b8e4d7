// qhuff_frames.cpp -- literal-span pre-parse of QPACK wire data and the
// batched literal decode built on it.
//
// The reference decodes string literals one at a time from inside its
// resumable instruction readers:
//   encoder stream   lsqpack_dec_enc_in       lsqpack.c:4574-4960
//   field section    parse_header_data et al. lsqpack.c:3567-3915
// and every Huffman literal goes through lsqpack_huff_decode
// (lsqpack.c:3718, 3795, 4714, 4824, 4908).  Here a cheap host pass walks
// the instruction framing only (prefixed integers, RFC 9204 sections 4.3 and
// 4.5 / lsqpack_dec_int(24), lsqpack.c:2372-2460) and records each literal's
// span; the Huffman spans of any number of blocks are then gathered into one
// pinned batch and decoded by the GPU kernel in a single launch.  Dynamic
// table references, blocked streams and the decoder's state machine stay
// with the reference: the scan resolves no index and allocates nothing.
// Plain C++ (no HIP): tests/c/ also builds it with ASan/UBSan on the CPU.
#include <stdint.h>
#include <string.h>

#include <new>

#include "../../include/qhuff.h"
#include "qhuff_lookup_impl.h"
#include "qhuff_lookup_dyn_impl.h"
#include "qhuff_names.h"
#include "qhuff_scan_impl.h"
#include "qhuff_tables.h"
#include "qhuff_tabs_impl.h"
#include "qhuff_tabs_insert_impl.h"

namespace {

// lsqpack_dec_int (lsqpack.c:2372-2437) on a complete buffer: 0 ok, -1 the
// buffer ends inside the integer, -2 the value does not fit 64 bits.  The
// reference's other -2 (out of input after >= LSQPACK_UINT64_ENC_SZ = 11
// bytes, lsqpack.c:2413-2423) counts bytes across resumed calls; in one call
// the loop reads at most the prefix byte and 10 continuation bytes and
// checks for input before the 10th, so out of input is always -1 here.
int
dec_int(const uint8_t **pp, const uint8_t *end, unsigned prefix_bits,
        uint64_t *v_out)
{
    const uint8_t *p = *pp;
    if (p >= end)
        return -1;
    const unsigned pmax = (1u << prefix_bits) - 1;
    uint64_t v = *p++ & pmax;
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
        B = *p++;
        v += (uint64_t) (B & 0x7f) << M;
        M += 7;
    } while ((B & 0x80) && M < 64);
    if (M <= 63 || (M == 70 && p[-1] <= 1 && (v & (1ull << 63))))
    {
        *pp = p;
        *v_out = v;
        return 0;
    }
    return -2;
}

// lsqpack_dec_int24 (lsqpack.c:2443-2460): values >= 2^24 are errors
int
dec_int24(const uint8_t **pp, const uint8_t *end, unsigned prefix_bits,
          uint32_t *v_out)
{
    uint64_t v;
    const int r = dec_int(pp, end, prefix_bits, &v);
    if (r)
        return r;
    if (v >= (1u << 24))
        return -2;
    *v_out = (uint32_t) v;
    return 0;
}

struct Sink
{
    const uint8_t *base;
    uint32_t pos_base;
    qhuff_literal *lits;
    uint32_t cap, n;
    bool overflow;
};

// a string literal whose H bit sits just above its N-bit length prefix
// (the layouts lsqpack_enc_enc_str writes for N = 3, 5, 7, lsqpack.c:839).
// max_len > 0: a declared length above it is an error as soon as the length
// is decoded, before the payload is looked for -- the field-section rule
// (LSXPACK_MAX_STRLEN, lsqpack.c:3682-3685 values, 3769-3772 names; pinned
// by test/test_header_alloc_clamp.c:108-135).
int
literal(Sink &s, const uint8_t **pp, const uint8_t *end, unsigned prefix_bits,
        unsigned kind, uint32_t instr, uint32_t max_len)
{
    const uint8_t *p = *pp;
    if (p >= end)
        return -1;
    const uint8_t *const start = p;
    const unsigned h = (*p >> prefix_bits) & 1;
    uint32_t len;
    const int r = dec_int24(&p, end, prefix_bits, &len);
    if (r)
        return r;
    if (max_len && len > max_len)
        return -2;
    if ((uint64_t) (end - p) < len)
        return -1;
    if (s.n < s.cap)
    {
        qhuff_literal &l = s.lits[s.n];
        l.pos = s.pos_base + (uint32_t) (p - s.base);
        l.len = len;
        l.huffman = (uint8_t) h;
        l.prefix_bits = (uint8_t) prefix_bits;
        l.kind = (uint8_t) kind;
        l.hdr_len = (uint8_t) (p - start);
        l.instr = s.pos_base + instr;
    }
    else
        s.overflow = true;
    ++s.n;
    *pp = p + len;
    return 0;
}

int
rc_of(int r)
{
    return r == -1 ? QHUFF_ETRUNC : QHUFF_EPROTO;
}

}  // namespace

// (the static table's name lengths: qhuff_names.h, shared with the device)
namespace qhuff {

// The length of the name a field-section VALUE literal's instruction refers
// to, when the framing alone knows it: a static name reference (01NT with
// T = 1, 4-bit index; lsqpack.c:3620-3642 header_out_begin_static_nameref
// copies static_table[idx].name into the header buffer) -> its length;
// a dynamic or post-base reference (the dynamic table stays with the
// reference) or anything else -> 0.  buf: the buffer lits' offsets are
// relative to (the instruction lies in [l.instr, l.pos - l.hdr_len)).
uint32_t
field_ref_name_len(const uint8_t *buf, const struct qhuff_literal &l)
{
    if (l.kind != QHUFF_LIT_VALUE || l.hdr_len > l.pos
            || (uint64_t) l.instr + 1 > l.pos - l.hdr_len)
        return 0;
    const uint8_t *p = buf + l.instr, *const end = buf + (l.pos - l.hdr_len);
    if ((*p & 0xd0) != 0x50)                 // 01NT, T = 1
        return 0;
    uint32_t idx;
    if (dec_int24(&p, end, 4, &idx) || idx >= kStaticNames)
        return 0;
    return kStaticNameLen[idx];
}

}  // namespace qhuff

// (ABI 7) the scanners' integer decoder on its own: lsqpack_dec_int
// (lsqpack.c:2372-2437) on a complete buffer -- pinned to the reference's
// own vectors (test/test_int.c:19-183, tests/golden/kat_int.json)
extern "C" int
qhuff_dec_int(const uint8_t *buf, size_t len, unsigned prefix_bits,
              uint64_t *value, size_t *consumed)
{
    if ((!buf && len) || !value || !consumed || prefix_bits < 1
            || prefix_bits > 8)
        return QHUFF_EINVAL;
    const uint8_t *p = buf;
    uint64_t v = 0;
    const int r = dec_int(&p, buf + len, prefix_bits, &v);
    if (r)
        return rc_of(r);
    *value = v;
    *consumed = (size_t) (p - buf);
    return QHUFF_OK;
}

extern "C" int
qhuff_scan_field_section(const uint8_t *buf, size_t len, uint32_t pos_base,
                         struct qhuff_literal *lits, uint32_t max_lits,
                         uint32_t *n_lits)
{
    if ((!buf && len) || (!lits && max_lits) || !n_lits
            || (uint64_t) pos_base + len > 0xffffffffu)
        return QHUFF_EINVAL;
    *n_lits = 0;
    Sink s{buf, pos_base, lits, max_lits, 0, false};
    const uint8_t *p = buf, *const end = buf + len;
    const uint32_t max_str = QHUFF_MAX_STRLEN;
    uint64_t v;
    int r;
    // section prefix: Required Insert Count (8-bit prefix), S + Delta Base
    // (7-bit prefix) -- RFC 9204 4.5.1, parse_header_prefix, lsqpack.c:3955-4046
    if ((r = dec_int(&p, end, 8, &v)) || (r = dec_int(&p, end, 7, &v)))
        return rc_of(r);
    while (p < end)
    {
        const uint8_t b = *p;
        const uint32_t at = (uint32_t) (p - buf);
        uint32_t idx;
        if (b & 0x80)                          // 1Txxxxxx indexed field line
            r = dec_int24(&p, end, 6, &idx);
        else if (b & 0x40)                     // 01NTxxxx literal, name ref
        {
            r = dec_int24(&p, end, 4, &idx);
            if (!r)
                r = literal(s, &p, end, 7, QHUFF_LIT_VALUE, at, max_str);
        }
        else if (b & 0x20)                     // 001NHxxx literal name
        {
            r = literal(s, &p, end, 3, QHUFF_LIT_NAME, at, max_str);
            if (!r)
                r = literal(s, &p, end, 7, QHUFF_LIT_VALUE, at, max_str);
        }
        else if (b & 0x10)                     // 0001xxxx indexed post-base
            r = dec_int24(&p, end, 4, &idx);
        else                                   // 0000Nxxx post-base name ref
        {
            r = dec_int24(&p, end, 3, &idx);
            if (!r)
                r = literal(s, &p, end, 7, QHUFF_LIT_VALUE, at, max_str);
        }
        if (r)
            return rc_of(r);
    }
    *n_lits = s.n;
    return s.overflow ? QHUFF_ERANGE : QHUFF_OK;
}

extern "C" int
qhuff_scan_encoder_stream(const uint8_t *buf, size_t len, uint32_t pos_base,
                          struct qhuff_literal *lits, uint32_t max_lits,
                          uint32_t *n_lits, size_t *consumed)
{
    if ((!buf && len) || (!lits && max_lits) || !n_lits || !consumed
            || (uint64_t) pos_base + len > 0xffffffffu)
        return QHUFF_EINVAL;
    *n_lits = 0;
    *consumed = 0;
    Sink s{buf, pos_base, lits, max_lits, 0, false};
    const uint8_t *p = buf, *const end = buf + len;
    while (p < end)
    {
        const uint8_t *q = p;
        const uint8_t b = *q;
        const uint32_t at = (uint32_t) (p - buf);
        const uint32_t n0 = s.n;
        uint32_t v;
        int r;
        if (b & 0x80)                // 1Txxxxxx insert with name reference
        {
            r = dec_int24(&q, end, 6, &v);
            if (!r)
                r = literal(s, &q, end, 7, QHUFF_LIT_VALUE, at, 0);
        }
        else if (b & 0x40)           // 01Hxxxxx insert with literal name
        {
            r = literal(s, &q, end, 5, QHUFF_LIT_NAME, at, 0);
            if (!r)
                r = literal(s, &q, end, 7, QHUFF_LIT_VALUE, at, 0);
        }
        else                         // 001xxxxx capacity / 000xxxxx dup
        {
            uint64_t w;
            r = dec_int(&q, end, 5, &w);
            if (!r && !(b & 0x20) && w >= (1u << 24))
                r = -2;
        }
        if (r == -1)
        {
            // a partial instruction: stop before it (the reference resumes
            // there when more stream data arrives, lsqpack.c:4574)
            s.n = n0;
            break;
        }
        if (r)
            return QHUFF_EPROTO;
        p = q;
    }
    if (s.n > s.cap)
    {
        *n_lits = s.n;
        return QHUFF_ERANGE;
    }
    *n_lits = s.n;
    *consumed = (size_t) (p - buf);
    return QHUFF_OK;
}

// ---- the device scan's walker on the host (qhuff_scan_impl.h) --------------
//
// qhuff_scan_sections' two passes in plain C++, chunk by chunk: the kernels'
// walker source over a reader that is the buffer itself.  The scanners above
// share no code with it.

namespace {

struct HostReader
{
    const uint8_t *buf;
    uint8_t get(uint32_t pos) const { return buf[pos]; }
};

}  // namespace

extern "C" int
qhuff_scan_sections_cpu(const uint8_t *buf, const uint32_t *sec_off,
                        uint32_t m, unsigned mode, struct qhuff_literal *lits,
                        uint32_t max_lits, uint32_t *lit_off, int32_t *rc,
                        uint32_t *consumed)
{
    if (!lit_off || (mode != QHUFF_SCAN_FIELD_SECTION
                     && mode != QHUFF_SCAN_ENCODER_STREAM)
            || (m && (!buf || !sec_off || !rc
                      || (!consumed && mode == QHUFF_SCAN_ENCODER_STREAM)))
            || (max_lits && !lits))
        return QHUFF_EINVAL;
    for (uint32_t i = 0; i < m; ++i)
        if (sec_off[i + 1] < sec_off[i])
            return QHUFF_EINVAL;
    HostReader r{buf};
    // the count pass
    lit_off[0] = 0;
    for (uint32_t i = 0; i < m; ++i)
    {
        qhuff::scan::CountSink s{0};
        uint32_t used;
        rc[i] = qhuff::scan::walk_chunk(r, s, mode, sec_off[i], sec_off[i + 1],
                                        &used);
        if (consumed)
            consumed[i] = used;
        lit_off[i + 1] = lit_off[i] + s.n;
    }
    // the write pass
    for (uint32_t i = 0; i < m; ++i)
    {
        const uint32_t first = lit_off[i];
        const uint32_t last = lit_off[i + 1] < max_lits ? lit_off[i + 1]
                                                        : max_lits;
        if (lit_off[i + 1] == first || first >= last)
            continue;
        qhuff::scan::WriteSink w{lits, first, last};
        uint32_t used;
        (void) qhuff::scan::walk_chunk(r, w, mode, sec_off[i], sec_off[i + 1],
                                       &used);
    }
    return lit_off[m] > max_lits ? QHUFF_ERANGE : QHUFF_OK;
}

// qhuff_scan_headers' two passes in plain C++, section by section: the
// kernels' header-line walker over the same reader.
extern "C" int
qhuff_scan_headers_cpu(const uint8_t *buf, const uint32_t *sec_off, uint32_t m,
                       struct qhuff_hstr *strs, uint32_t max_hdrs,
                       uint32_t *hdr_off, int32_t *rc, uint8_t *kind,
                       uint8_t *static_id, uint8_t *hflags)
{
    if (!hdr_off || (m && (!buf || !sec_off || !rc)) || (max_hdrs && !strs))
        return QHUFF_EINVAL;
    for (uint32_t i = 0; i < m; ++i)
        if (sec_off[i + 1] < sec_off[i])
            return QHUFF_EINVAL;
    HostReader r{buf};
    // the count pass
    hdr_off[0] = 0;
    for (uint32_t i = 0; i < m; ++i)
    {
        qhuff::scan::HdrCountSink s{0};
        rc[i] = qhuff::scan::walk_header_section(r, s, sec_off[i],
                                                 sec_off[i + 1]);
        hdr_off[i + 1] = hdr_off[i] + s.n;
    }
    // the write pass
    for (uint32_t i = 0; i < m; ++i)
    {
        const uint32_t first = hdr_off[i];
        const uint32_t last = hdr_off[i + 1] < max_hdrs ? hdr_off[i + 1]
                                                        : max_hdrs;
        if (hdr_off[i + 1] == first || first >= last)
            continue;
        qhuff::scan::HdrWriteSink w{strs, kind, static_id, hflags, first, last};
        (void) qhuff::scan::walk_header_section(r, w, sec_off[i],
                                                sec_off[i + 1]);
    }
    return hdr_off[m] > max_hdrs ? QHUFF_ERANGE : QHUFF_OK;
}

// qhuff_scan_headers_dyn's two passes in plain C++: the same walker with the
// table and each section's window.
extern "C" int
qhuff_scan_headers_dyn_cpu(const uint8_t *buf, const uint32_t *sec_off,
                           uint32_t m, const struct qhuff_dyn_table *tab,
                           const uint32_t *sec_win, struct qhuff_hstr *strs,
                           uint32_t max_hdrs, uint32_t *hdr_off, int32_t *rc,
                           uint8_t *kind, uint8_t *static_id, uint8_t *hflags,
                           uint32_t *dyn_id)
{
    namespace qs = qhuff::scan;
    if (!hdr_off || !tab || (m && (!buf || !sec_off || !rc))
            || (max_hdrs && !strs))
        return QHUFF_EINVAL;
    for (uint32_t i = 0; i < m; ++i)
        if (sec_off[i + 1] < sec_off[i])
            return QHUFF_EINVAL;
    uint32_t longest;
    if (const int r = qs::dyn_check(tab, sec_win, m, &longest))
        return r;
    HostReader r{buf};
    auto win = [&](uint32_t i) {
        return qs::DynWin::of(tab->off, tab->d, tab->first, tab->max_entries,
                              sec_win, i);
    };
    // the count pass
    hdr_off[0] = 0;
    for (uint32_t i = 0; i < m; ++i)
    {
        qs::HdrDynCountSink s{0};
        rc[i] = qs::walk_header_section(r, s, sec_off[i], sec_off[i + 1],
                                        win(i));
        hdr_off[i + 1] = hdr_off[i] + s.n;
    }
    // the write pass
    for (uint32_t i = 0; i < m; ++i)
    {
        const uint32_t first = hdr_off[i];
        const uint32_t last = hdr_off[i + 1] < max_hdrs ? hdr_off[i + 1]
                                                        : max_hdrs;
        if (hdr_off[i + 1] == first || first >= last)
            continue;
        qs::HdrDynWriteSink w{{strs, kind, static_id, hflags, first, last},
                              dyn_id};
        (void) qs::walk_header_section(r, w, sec_off[i], sec_off[i + 1],
                                       win(i));
    }
    return hdr_off[m] > max_hdrs ? QHUFF_ERANGE : QHUFF_OK;
}

// ---- the lookup kernel's source on the host (qhuff_lookup_impl.h) -----------
//
// qhuff_static_lookup in plain C++, header by header: the kernels' XXH32 and
// lookup source over a reader that is the buffer itself, against this
// translation unit's copy of the static table and its probe tables.

namespace {

constexpr qhuff::StaticTable kStaticHost = qhuff::make_static_table();

}  // namespace

extern "C" int
qhuff_static_lookup_cpu(const uint8_t *in, const uint32_t *off, uint32_t n,
                        uint32_t *name_hash, uint32_t *nameval_hash,
                        uint8_t *kind, uint8_t *static_id)
{
    if (!off || (n && (!in || !kind || !static_id)))
        return QHUFF_EINVAL;
    if (n > 0x7fffffffu)
        return QHUFF_ERANGE;
    for (uint64_t i = 0; i < 2ull * n; ++i)
        if (off[i + 1] < off[i])
            return QHUFF_EINVAL;
    const qhuff::HashMem r{in};
    for (uint32_t i = 0; i < n; ++i)
    {
        const uint32_t a = off[2ull * i], m = off[2ull * i + 1],
                       b = off[2ull * i + 2];
        const uint32_t h1 = qhuff::xxh32(r, a, m - a, QHUFF_XXH_SEED);
        const uint32_t h2 = qhuff::xxh32(r, m, b - m, h1);
        const qhuff::StaticHit hit = qhuff::static_lookup(r, a, m, b, h1, h2,
                                                          kStaticHost);
        if (name_hash)
            name_hash[i] = h1;
        if (nameval_hash)
            nameval_hash[i] = h2;
        kind[i] = (uint8_t) hit.kind;
        static_id[i] = (uint8_t) hit.id;
    }
    return QHUFF_OK;
}

// ---- ... and the dynamic lookup's (qhuff_lookup_dyn_impl.h) -------------------

extern "C" uint32_t
qhuff_dyn_index_slots(uint32_t d)
{
    return qhuff::dyn_index_slots(d);
}

// the index built entry by entry in ordinal order, then the kernel's lookup
// source header by header, the window clamped as the kernel clamps it
static int
dyn_lookup_cpu_run(const uint8_t *in, const uint32_t *off, uint32_t n,
                   const struct qhuff_dyn_table *tab, uint32_t win_lo,
                   uint32_t win_hi, uint32_t *name_hash,
                   uint32_t *nameval_hash, uint8_t *kind, uint8_t *static_id,
                   uint32_t *dyn_id)
{
    const uint32_t d = tab->d;
    const uint32_t slots = d ? qhuff::dyn_index_slots(d) : 0;
    uint32_t *idx = slots ? new (std::nothrow) uint32_t[2ull * slots]() : nullptr;
    if (slots && !idx)
        return QHUFF_ENOMEM;
    qhuff::DynTab<qhuff::HashMem, const uint32_t *> t;
    t.tb = qhuff::HashMem{tab->bytes};
    t.off = tab->off;
    t.nv = idx;
    t.nm = idx + slots;
    t.mask = slots ? slots - 1 : 0;
    t.d = d;
    t.first = tab->first;
    t.t0 = d ? tab->off[0] : 0;
    t.t1 = d ? tab->off[2ull * d] : 0;
    auto claim = [](uint32_t *p, uint32_t v) {
        if (*p)
            return false;
        *p = v;
        return true;
    };
    for (uint32_t k = 0; k < d; ++k)
        qhuff::dyn_index_insert(t.tb, t.off, k, t.t0, t.t1, idx, idx + slots,
                                t.mask, claim);
    const qhuff::DynRange w = qhuff::dyn_window(win_lo, win_hi, tab->first, d,
                                                tab->max_entries);
    const qhuff::HashMem r{in};
    for (uint32_t i = 0; i < n; ++i)
    {
        const uint32_t a = off[2ull * i], m = off[2ull * i + 1],
                       b = off[2ull * i + 2];
        const uint32_t h1 = qhuff::xxh32(r, a, m - a, QHUFF_XXH_SEED);
        const uint32_t h2 = qhuff::xxh32(r, m, b - m, h1);
        const qhuff::DynHit hit = qhuff::dyn_lookup(r, a, m, b, h1, h2,
                                                    kStaticHost, t, w.lo,
                                                    w.hi);
        if (name_hash)
            name_hash[i] = h1;
        if (nameval_hash)
            nameval_hash[i] = h2;
        kind[i] = (uint8_t) hit.kind;
        static_id[i] = (uint8_t) hit.id;
        if (dyn_id)
            dyn_id[i] = hit.dyn;
    }
    delete[] idx;
    return QHUFF_OK;
}

// qhuff_dyn_lookup in plain C++, after the host form's checks
extern "C" int
qhuff_dyn_lookup_cpu(const uint8_t *in, const uint32_t *off, uint32_t n,
                     const struct qhuff_dyn_table *tab, uint32_t win_lo,
                     uint32_t win_hi, uint32_t *name_hash,
                     uint32_t *nameval_hash, uint8_t *kind,
                     uint8_t *static_id, uint32_t *dyn_id)
{
    if (!off || (n && (!in || !kind || !static_id)))
        return QHUFF_EINVAL;
    const uint32_t win[2] = {win_lo, win_hi};
    if (const int rc = qhuff::dyn_enc_check(tab, win, nullptr, 1))
        return rc;
    if (n > 0x7fffffffu)
        return QHUFF_ERANGE;
    for (uint64_t i = 0; i < 2ull * n; ++i)
        if (off[i + 1] < off[i])
            return QHUFF_EINVAL;
    return dyn_lookup_cpu_run(in, off, n, tab, win_lo, win_hi, name_hash,
                              nameval_hash, kind, static_id, dyn_id);
}

// ---- ... over a set of tables, a table per section (qhuff_tabs_impl.h) -------

// qhuff_scan_headers_tabs' two passes in plain C++: qhuff_scan_headers_dyn_cpu
// with each section's window formed from its own table.
extern "C" int
qhuff_scan_headers_tabs_cpu(const uint8_t *buf, const uint32_t *sec_off,
                            uint32_t m, const struct qhuff_dyn_tables *tabs,
                            const uint32_t *sec_tab, const uint32_t *sec_win,
                            struct qhuff_hstr *strs, uint32_t max_hdrs,
                            uint32_t *hdr_off, int32_t *rc, uint8_t *kind,
                            uint8_t *static_id, uint8_t *hflags,
                            uint32_t *dyn_id)
{
    namespace qs = qhuff::scan;
    if (!hdr_off || (m && (!buf || !sec_off || !rc)) || (max_hdrs && !strs))
        return QHUFF_EINVAL;
    for (uint32_t i = 0; i < m; ++i)
        if (sec_off[i + 1] < sec_off[i])
            return QHUFF_EINVAL;
    uint32_t D, longest;
    if (const int r = qhuff::tabs_check(tabs, sec_tab, sec_win, nullptr, m,
                                        false, &D, &longest))
        return r;
    HostReader r{buf};
    auto win = [&](uint32_t i) {
        return qs::dyn_win_tabs(tabs->off, tabs->ent, tabs->first,
                                tabs->max_entries, tabs->T, D, sec_tab,
                                sec_win, i);
    };
    // the count pass
    hdr_off[0] = 0;
    for (uint32_t i = 0; i < m; ++i)
    {
        qs::HdrDynCountSink s{0};
        rc[i] = qs::walk_header_section(r, s, sec_off[i], sec_off[i + 1],
                                        win(i));
        hdr_off[i + 1] = hdr_off[i] + s.n;
    }
    // the write pass
    for (uint32_t i = 0; i < m; ++i)
    {
        const uint32_t first = hdr_off[i];
        const uint32_t last = hdr_off[i + 1] < max_hdrs ? hdr_off[i + 1]
                                                        : max_hdrs;
        if (hdr_off[i + 1] == first || first >= last)
            continue;
        qs::HdrDynWriteSink w{{strs, kind, static_id, hflags, first, last},
                              dyn_id};
        (void) qs::walk_header_section(r, w, sec_off[i], sec_off[i + 1],
                                       win(i));
    }
    return hdr_off[m] > max_hdrs ? QHUFF_ERANGE : QHUFF_OK;
}

extern "C" uint32_t
qhuff_dyn_tables_index_slots(uint32_t D)
{
    return qhuff::dyn_index_slots(D);
}

// qhuff_dyn_lookup_tabs in plain C++, after the host form's checks: the one
// pair of indices built entry by entry in ordinal order, each entry's first
// slot mixed with its table, then the kernel's lookup source section by
// section, header by header
extern "C" int
qhuff_dyn_lookup_tabs_cpu(const uint8_t *in, const uint32_t *off, uint32_t n,
                          const uint32_t *sec_hdr, uint32_t m,
                          const struct qhuff_dyn_tables *tabs,
                          const uint32_t *sec_tab, const uint32_t *sec_win,
                          uint32_t *name_hash, uint32_t *nameval_hash,
                          uint8_t *kind, uint8_t *static_id, uint32_t *dyn_id)
{
    if (!off || !sec_hdr || (n && (!in || !kind || !static_id)))
        return QHUFF_EINVAL;
    if (n > 0x7fffffffu)
        return QHUFF_ERANGE;
    if (sec_hdr[0] != 0 || sec_hdr[m] != n)
        return QHUFF_EINVAL;
    for (uint32_t s = 0; s < m; ++s)
        if (sec_hdr[s + 1] < sec_hdr[s])
            return QHUFF_EINVAL;
    for (uint64_t i = 0; i < 2ull * n; ++i)
        if (off[i + 1] < off[i])
            return QHUFF_EINVAL;
    uint32_t D, longest;
    if (const int rc = qhuff::tabs_check(tabs, sec_tab, sec_win, nullptr, m,
                                         true, &D, &longest))
        return rc;
    const uint32_t slots = D ? qhuff::dyn_index_slots(D) : 0;
    uint32_t *idx = slots ? new (std::nothrow) uint32_t[2ull * slots]() : nullptr;
    if (slots && !idx)
        return QHUFF_ENOMEM;
    // all D entries as one table of ordinals
    qhuff::DynTab<qhuff::HashMem, const uint32_t *> t;
    t.tb = qhuff::HashMem{tabs->bytes};
    t.off = tabs->off;
    t.nv = idx;
    t.nm = idx + slots;
    t.mask = slots ? slots - 1 : 0;
    t.d = D;
    t.first = 0;
    t.t0 = D ? tabs->off[0] : 0;
    t.t1 = D ? tabs->off[2ull * D] : 0;
    auto claim = [](uint32_t *p, uint32_t v) {
        if (*p)
            return false;
        *p = v;
        return true;
    };
    for (uint32_t k = 0; k < D; ++k)
        qhuff::dyn_index_insert(
            t.tb, t.off, k, t.t0, t.t1, idx, idx + slots, t.mask, claim,
            qhuff::tab_mix(qhuff::tab_of_entry(tabs->ent, tabs->T, D, k)));
    const qhuff::HashMem r{in};
    for (uint32_t s = 0; s < m; ++s)
    {
        const qhuff::TabSection sec = qhuff::tab_section(
            tabs->ent, tabs->first, tabs->max_entries, tabs->T, D, sec_tab,
            sec_win, (const uint32_t *) nullptr, s);
        for (uint32_t i = sec_hdr[s]; i < sec_hdr[s + 1]; ++i)
        {
            const uint32_t a = off[2ull * i], mid = off[2ull * i + 1],
                           b = off[2ull * i + 2];
            const uint32_t h1 = qhuff::xxh32(r, a, mid - a, QHUFF_XXH_SEED);
            const uint32_t h2 = qhuff::xxh32(r, mid, b - mid, h1);
            const qhuff::DynHit hit = qhuff::tab_hit(
                qhuff::dyn_lookup(r, a, mid, b, h1, h2, kStaticHost, t,
                                  sec.glo, sec.ghi, sec.mix), sec.delta);
            if (name_hash)
                name_hash[i] = h1;
            if (nameval_hash)
                nameval_hash[i] = h2;
            kind[i] = (uint8_t) hit.kind;
            static_id[i] = (uint8_t) hit.id;
            if (dyn_id)
                dyn_id[i] = hit.dyn;
        }
    }
    delete[] idx;
    return QHUFF_OK;
}

extern "C" int
qhuff_static_probe_tables(uint8_t name2id_plus_one[512],
                          uint8_t nameval2id_plus_one[512])
{
    if (!name2id_plus_one || !nameval2id_plus_one)
        return QHUFF_EINVAL;
    static_assert(qhuff::kStaticSlots == 512, "the public table size");
    memcpy(name2id_plus_one, kStaticHost.name2id, 512);
    memcpy(nameval2id_plus_one, kStaticHost.nameval2id, 512);
    return QHUFF_OK;
}

// ---- encoder-stream inserts applied to a set of tables, on the host ---------
//
// qhuff_tabs_insert_host's path in plain C++: the kernels' walker
// (qhuff_scan_impl.h walk_insert_stream), the descriptors decoded by a host
// decoder -- a bit-by-bit canonical Huffman walk over the code lengths of
// qhuff_tables.h --, then the kernels' accounting, sums and copy
// (qhuff_tabs_insert_impl.h).

namespace {

namespace qi = qhuff::ins;

// RFC 7541 Appendix B as a canonical code: per length the first code, the
// count and the rank of its first symbol; the symbols in canonical order
struct HostHuff
{
    uint32_t first[31], count[31], base[31];
    uint16_t sorted[257];
    HostHuff()
    {
        memset(count, 0, sizeof(count));
        for (int s = 0; s < 257; ++s)
            count[qhuff::kLen[s]]++;
        uint32_t next = 0, rank = 0;
        first[0] = base[0] = 0;
        for (int L = 1; L <= 30; ++L)
        {
            next <<= 1;
            first[L] = next;
            base[L] = rank;
            next += count[L];
            rank += count[L];
        }
        uint32_t at[31];
        memcpy(at, base, sizeof(at));
        for (int s = 0; s < 257; ++s)
            sorted[at[qhuff::kLen[s]]++] = (uint16_t) s;
    }
};

// src[0 .. n) decoded into dst (room for 8 n / 5): its length, or -1 (the EOS
// code in the data, padding of more than 7 bits or not all ones:
// QHUFF_DEC_ERROR)
int64_t
huff_decode_host(const uint8_t *src, uint32_t n, uint8_t *dst)
{
    static const HostHuff h;
    uint32_t code = 0, len = 0;
    int64_t m = 0;
    for (uint64_t b = 0; b < 8ull * n; ++b)
    {
        code = code << 1 | ((src[b >> 3] >> (7 - (b & 7))) & 1);
        ++len;
        if (h.count[len] && code - h.first[len] < h.count[len])
        {
            const uint32_t sym = h.sorted[h.base[len] + code - h.first[len]];
            if (sym == 256)
                return -1;
            dst[m++] = (uint8_t) sym;
            code = len = 0;
        }
        else if (len == 30)
            return -1;
    }
    if (len > 7 || code != (1u << len) - 1)
        return -1;
    return m;
}

// qhuff_decode_headers_dyn's result for 2n descriptors with max_len = 0
void
decode_strs_host(const uint8_t *buf, const struct qhuff_hstr *strs, uint64_t n2,
                 const uint8_t *dyn, uint32_t dyn_len, uint8_t *out,
                 uint32_t *off, uint8_t *status)
{
    uint32_t at = 0;
    off[0] = 0;
    for (uint64_t s = 0; s < n2; ++s)
    {
        const struct qhuff_hstr &d = strs[s];
        status[s] = QHUFF_DEC_OK;
        if (d.source == QHUFF_HSTR_STATIC)
        {
            const uint32_t id = d.static_id < qhuff::kStaticNames
                                    ? d.static_id : qhuff::kStaticNames - 1;
            const bool val = d.kind == QHUFF_LIT_VALUE;
            const uint32_t nl = kStaticHost.name_len[id];
            const uint32_t l = val ? kStaticHost.val_len[id] : nl;
            for (uint32_t k = 0; k < l; ++k)
                out[at + k] = (uint8_t) kStaticHost.byte(kStaticHost.at[id],
                                                         (val ? nl : 0) + k);
            at += l;
        }
        else if (d.source == QHUFF_HSTR_DYN)
        {
            const uint32_t from = d.instr < dyn_len ? d.instr : dyn_len;
            const uint32_t l = d.len < dyn_len - from ? d.len : dyn_len - from;
            if (l)
                memcpy(out + at, dyn + from, l);
            at += l;
        }
        else if (d.huffman)
        {
            const int64_t l = huff_decode_host(buf + d.pos, d.len, out + at);
            if (l < 0)
                status[s] = QHUFF_DEC_ERROR;
            else
                at += (uint32_t) l;
        }
        else
        {
            if (d.len)
                memcpy(out + at, buf + d.pos, d.len);
            at += d.len;
        }
        off[s + 1] = at;
    }
}

}  // namespace

extern "C" uint64_t
qhuff_tabs_insert_bound(uint64_t arena_bytes, uint64_t wire_bytes,
                        uint32_t max_ins, uint32_t dyn_longest)
{
    return arena_bytes + qi::decode_bound(wire_bytes, max_ins, dyn_longest);
}

extern "C" int
qhuff_tabs_insert_cpu(const struct qhuff_dyn_tables *tabs,
                      const struct qhuff_ins_state *st, const uint8_t *buf,
                      const uint32_t *enc_off, const uint32_t *keep,
                      const struct qhuff_ins_scan *sc,
                      const struct qhuff_ins_out *o)
{
    namespace qs = qhuff::scan;
    uint32_t D, longest;
    if (const int r = qi::check(tabs, st, buf, enc_off, sc, o, &D, &longest))
        return r;
    const uint32_t T = tabs->T;
    const uint64_t wire = T ? (uint64_t) enc_off[T] - enc_off[0] : 0;
    const uint64_t arena = D ? tabs->off[2ull * D] : 0;
    if (qhuff_tabs_insert_bound(arena, wire, sc->max_ins, longest)
            > 0xffffffffull)
        return QHUFF_ERANGE;
    HostReader r{buf};
    // the scan: the count pass, then the write pass
    uint32_t *ccap = sc->chunk_cap ? sc->chunk_cap
                                   : new uint32_t[2ull * T + 1];
    sc->ins_off[0] = 0;
    for (uint32_t c = 0; c < T; ++c)
    {
        qs::InsCountSink s{0, st->cap[c], st->cap[c]};
        uint32_t stop = enc_off[c];
        const int rc = qs::walk_insert_stream(r, s, enc_off[c], enc_off[c + 1],
                                              st->cap[c], st->max_cap[c],
                                              &stop);
        sc->rc[c] = rc ? QHUFF_EPROTO : QHUFF_OK;
        sc->consumed[c] = rc ? 0 : stop - enc_off[c];
        ccap[2ull * c] = rc ? st->cap[c] : s.cmin;
        ccap[2ull * c + 1] = rc ? st->cap[c] : s.cap;
        sc->ins_off[c + 1] = sc->ins_off[c] + (rc ? 0 : s.n);
    }
    const uint32_t total = sc->ins_off[T];
    int ret = total > sc->max_ins ? QHUFF_ERANGE
                                  : qi::check_counts(tabs, sc->ins_off);
    // (QHUFF_ERANGE: the first max_ins inserts' scan results, nothing applied)
    const uint64_t n = total < sc->max_ins ? total : sc->max_ins;
    struct qhuff_hstr *strs = sc->strs ? sc->strs
                                       : new struct qhuff_hstr[2 * n + 1];
    uint32_t *root = sc->root ? sc->root : new uint32_t[2 * n + 1];
    uint32_t *icap = sc->ins_cap ? sc->ins_cap : new uint32_t[2 * n + 1];
    uint32_t *dec_off = new uint32_t[2 * n + 1];
    uint32_t *fin = new uint32_t[4 * n + 1], *rel = fin + 2 * n;
    uint32_t *plan = new uint32_t[4ull * T + 1];
    uint64_t *sums = new uint64_t[2ull * T + 2];
    uint8_t *status = new uint8_t[2 * n + 1];
    uint8_t *dec = nullptr;
    for (uint32_t c = 0; c < T; ++c)
    {
        const uint32_t k0 = sc->ins_off[c];
        const uint32_t k1 = sc->ins_off[c + 1] < n ? sc->ins_off[c + 1]
                                                   : (uint32_t) n;
        if (k0 >= k1)
            continue;
        const qs::TabView v = qs::ins_tab_view(tabs->ent, tabs->first, D, c);
        qs::InsWriteSink w{strs, root, icap, sc->ins_ref, sc->ins_kind,
                           tabs->off + 2ull * v.e0, v.d, v.first, k0, k0, k1};
        uint32_t stop;
        (void) qs::walk_insert_stream(r, w, enc_off[c], enc_off[c + 1],
                                      st->cap[c], st->max_cap[c], &stop);
    }
    if (!ret)
    {
        dec = new uint8_t[qi::decode_bound(wire, (uint32_t) n, longest)];
        decode_strs_host(buf, strs, 2 * n, tabs->bytes, (uint32_t) arena, dec,
                         dec_off, status);
        qi::Args a;
        a.bytes = tabs->bytes;
        a.off = tabs->off;
        a.ent = tabs->ent;
        a.first = tabs->first;
        a.cap = st->cap;
        a.live_lo = st->live_lo;
        a.keep = keep;
        a.T = T;
        a.D = D;
        a.arena = (uint32_t) arena;
        a.rc = sc->rc;
        a.consumed = sc->consumed;
        a.ins_off = sc->ins_off;
        a.chunk_cap = ccap;
        a.strs = strs;
        a.root = root;
        a.ins_cap = icap;
        a.ins_ref = sc->ins_ref;
        a.ins_kind = sc->ins_kind;
        a.n_ins = (uint32_t) n;
        a.dec = dec;
        a.dec_off = dec_off;
        a.status = status;
        a.fin = fin;
        a.rel = rel;
        a.plan = plan;
        a.sums = sums;
        a.ins_lo = o->ins_lo;
        a.out_bytes = o->out_bytes;
        a.out_off = o->out_off;
        a.out_ent = o->out_ent;
        a.out_first = o->out_first;
        a.cap_out = o->cap_out;
        a.live_lo_out = o->live_lo_out;
        a.out_cap = o->out_cap;
        a.ent_cap = o->ent_cap;
        for (uint32_t c = 0; c < T; ++c)
            qi::account(a, c);
        qi::sums_host(a);
        for (uint32_t c = 0; c < T; ++c)
            qi::copy_host(a, c);
    }
    delete[] dec;
    delete[] status;
    delete[] sums;
    delete[] plan;
    delete[] fin;
    delete[] dec_off;
    if (icap != sc->ins_cap)
        delete[] icap;
    if (root != sc->root)
        delete[] root;
    if (strs != sc->strs)
        delete[] strs;
    if (ccap != sc->chunk_cap)
        delete[] ccap;
    return ret;
}

// ---- literal framing from a precomputed payload ---
//
// lsqpack_enc_enc_str (lsqpack.c:839-876) with its Huffman step already done
// by a PAYLOAD-mode batch: the strict size test (lsqpack.c:848), the H bit
// and the prefixed length (lsqpack_val2len / lsqpack_enc_int_nocheck,
// lsqpack.c:767-836), the payload or the raw string, -1 when dst_len is
// short.  dst[0] bits above the H bit are kept, as in the reference.

namespace {

unsigned
val2len(uint64_t v, unsigned prefix_bits)
{
    const uint64_t mask = (1ull << prefix_bits) - 1;
    unsigned n = 1;
    if (v >= mask)
        for (v -= mask, ++n; v >= 128; v >>= 7)
            ++n;
    return n;
}

void
put_int(uint8_t *dst, uint64_t v, unsigned prefix_bits)
{
    const uint64_t mask = (1ull << prefix_bits) - 1;
    if (v < mask)
    {
        *dst |= (uint8_t) v;
        return;
    }
    *dst++ |= (uint8_t) mask;
    for (v -= mask; v >= 128; v >>= 7)
        *dst++ = (uint8_t) (0x80 | v);
    *dst = (uint8_t) v;
}

}  // namespace

extern "C" int
qhuff_frame_literal(unsigned prefix_bits, unsigned char *dst, size_t dst_len,
                    const unsigned char *str, unsigned str_len,
                    const unsigned char *huff, unsigned huff_len)
{
    if (!dst || (!str && str_len) || (!huff && huff_len)
            || (prefix_bits != 3 && prefix_bits != 5 && prefix_bits != 7))
        return -1;
    const bool h = huff_len < str_len;
    const unsigned n = h ? huff_len : str_len;
    const unsigned len_size = val2len(n, prefix_bits);
    if ((uint64_t) len_size + n > dst_len)
        return -1;
    dst[0] &= (uint8_t) ~((1u << (prefix_bits + 1)) - 1);
    if (h)
        dst[0] |= (uint8_t) (1u << prefix_bits);
    put_int(dst, n, prefix_bits);
    memcpy(dst + len_size, h ? huff : str, n);
    return (int) (len_size + n);
}

// The order rule of the in-place literal decode (qhuff_decode_wire,
// qhuff_wire.hip): descriptors in wire order and disjoint, each with its
// header and its instruction in front of it, every end within 32 bits.
// Both scanners above emit descriptors of this form.
extern "C" int
qhuff_literals_check(const struct qhuff_literal *lits, uint32_t n,
                     uint32_t *bad)
{
    if (!lits && n)
        return QHUFF_EINVAL;
    for (uint32_t i = 0; i < n; ++i)
    {
        const qhuff_literal &l = lits[i];
        const uint64_t end = (uint64_t) l.pos + l.len;
        const bool ok = l.hdr_len <= l.pos && l.instr <= l.pos - l.hdr_len
                     && end <= 0xffffffffull
                     && (i + 1 == n || end <= lits[i + 1].pos);
        if (!ok)
        {
            // (a pair out of order is reported at its second literal)
            const bool self = l.hdr_len > l.pos || l.instr > l.pos - l.hdr_len
                           || end > 0xffffffffull;
            if (bad)
                *bad = self ? i : i + 1;
            return QHUFF_EINVAL;
        }
    }
    return QHUFF_OK;
}
