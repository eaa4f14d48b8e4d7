// tabs_san.cpp -- the source the calls over a set of dynamic tables run on
// the CPU (csrc/qhuff_tabs_impl.h and qhuff_scan_impl.h's dyn_win_tabs: a
// section's view of its table, the window as ordinals, the entry-to-table
// search, the mixed first slot) under ASan/UBSan.  Stand-alone: built by
// tests/test_headers_tabs.py with qhuff_frames.cpp and nothing else.
//
// Every array is a heap buffer of exactly its size: a read that leaves one is
// an ASan report.  Part 1 runs qhuff_scan_headers_tabs_cpu and
// qhuff_dyn_lookup_tabs_cpu on inputs inside the rule and checks a few
// answers and the checks' verdicts.  Part 2 drives the source itself, as the
// device forms run it where nothing can be checked: sec_tab out of range,
// ent that decreases or passes D, windows and Bases outside their table, off
// that decreases or points past the bytes.  The results must stay inside the
// section's table and window, and the walk inside `off`.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/qhuff.h"
#include "../../ls-qpack_amd/csrc/qhuff_tabs_impl.h"

namespace {

struct Packed
{
    uint8_t *bytes;
    uint32_t *off;
    uint32_t n;
};

Packed
pack(const std::vector<std::pair<std::string, std::string>> &hs, uint32_t pad)
{
    std::string all(pad, '#');
    std::vector<uint32_t> off(1, pad);
    for (const auto &h : hs)
    {
        all += h.first;
        off.push_back((uint32_t) all.size());
        all += h.second;
        off.push_back((uint32_t) all.size());
    }
    Packed p;
    p.n = (uint32_t) hs.size();
    p.bytes = (uint8_t *) malloc(all.size() ? all.size() : 1);
    memcpy(p.bytes, all.data(), all.size());
    p.off = (uint32_t *) malloc(4 * off.size());
    memcpy(p.off, off.data(), 4 * off.size());
    return p;
}

uint32_t *
words(const std::vector<uint32_t> &v)
{
    uint32_t *p = (uint32_t *) malloc(4 * (v.size() ? v.size() : 1));
    memcpy(p, v.data(), 4 * v.size());
    return p;
}

#define CHECK(x)                                                             \
    do {                                                                     \
        if (!(x))                                                            \
        {                                                                    \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x);          \
            return 1;                                                        \
        }                                                                    \
    } while (0)

uint64_t rng_state = 0x9E3779B97F4A7C15ull;

uint32_t
rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t) (rng_state >> 16);
}

const qhuff::StaticTable kStatic = qhuff::make_static_table();

struct Reader
{
    const uint8_t *buf;
    uint8_t get(uint32_t pos) const { return buf[pos]; }
};

}  // namespace

int
main()
{
    using namespace qhuff;
    // four tables of 5, 0, 7 and 3 entries; the same names in each
    const uint32_t T = 4, dn[4] = {5, 0, 7, 3};
    const uint32_t firsts[4] = {7, 100, 0, 0xfffffff0u}, mes[4] = {8, 8, 0, 4};
    std::vector<std::pair<std::string, std::string>> ents, hs;
    std::vector<uint32_t> ent_v(1, 0);
    for (uint32_t c = 0; c < T; ++c)
    {
        for (uint32_t k = 0; k < dn[c]; ++k)
            ents.push_back({"x-e" + std::to_string(k % 4),
                            "v" + std::to_string(k)});
        ent_v.push_back((uint32_t) ents.size());
    }
    const uint32_t D = (uint32_t) ents.size();
    for (uint32_t k = 0; k < 8; ++k)
    {
        hs.push_back({"x-e" + std::to_string(k % 4), "v" + std::to_string(k)});
        hs.push_back({"x-e" + std::to_string(k % 4), "other"});
    }
    hs.push_back({":method", "GET"});
    hs.push_back({"x-none", ""});
    const Packed TB = pack(ents, 3), H = pack(hs, 5);
    const uint32_t hn = H.n;

    // ---- part 1: inside the rule ------------------------------------------
    {
        uint32_t *ent = words(ent_v);
        uint32_t *first = words({firsts[0], firsts[1], firsts[2], firsts[3]});
        uint32_t *me = words({mes[0], mes[1], mes[2], mes[3]});
        struct qhuff_dyn_tables tabs = {TB.bytes, TB.off, ent, first, me, T};
        // a section a table, all of them looking up the same headers
        std::vector<std::pair<std::string, std::string>> all;
        for (uint32_t c = 0; c < T; ++c)
            all.insert(all.end(), hs.begin(), hs.end());
        const Packed A = pack(all, 1);
        uint32_t *sec_hdr = words({0, hn, 2 * hn, 3 * hn, 4 * hn});
        uint32_t *sec_tab = words({0, 1, 2, 3});
        // (table 3 holds 3 entries under max_entries 4: the whole table)
        uint32_t *h1 = (uint32_t *) malloc(4 * A.n);
        uint32_t *h2 = (uint32_t *) malloc(4 * A.n);
        uint32_t *did = (uint32_t *) malloc(4 * A.n);
        uint8_t *kind = (uint8_t *) malloc(A.n), *sid = (uint8_t *) malloc(A.n);
        CHECK(qhuff_dyn_lookup_tabs_cpu(A.bytes, A.off, A.n, sec_hdr, T, &tabs,
                                        sec_tab, NULL, h1, h2, kind, sid, did)
              == QHUFF_OK);
        // table 0: (x-e0, v4) is its entry 4, the name x-e0 first at 0
        CHECK(kind[8] == (QHUFF_LINE_INDEXED | QHUFF_LINE_DYN));
        CHECK(did[8] == firsts[0] + 4);
        CHECK(kind[9] == (QHUFF_LINE_NAMEREF | QHUFF_LINE_DYN));
        CHECK(did[9] == firsts[0] + 0);
        // (x-e1, v5) is table 2's entry: here only its name is held
        CHECK(kind[10] == (QHUFF_LINE_NAMEREF | QHUFF_LINE_DYN));
        CHECK(did[10] == firsts[0] + 1 && did[11] == firsts[0] + 1);
        // table 1 is empty, table 2 disabled: no dynamic line
        for (uint32_t i = hn; i < 3 * hn; ++i)
            CHECK(did[i] == QHUFF_DYN_NONE && !(kind[i] & QHUFF_LINE_DYN));
        // table 3: near the top of the index space
        CHECK(did[3 * hn + 4] == firsts[3] + 2 && did[3 * hn + 6] == QHUFF_DYN_NONE);
        CHECK(kind[4 * hn - 2] == QHUFF_LINE_INDEXED && sid[4 * hn - 2] == 17);
        // the checks
        uint32_t *bad_tab = words({0, 1, 2, 4});
        CHECK(qhuff_dyn_lookup_tabs_cpu(A.bytes, A.off, A.n, sec_hdr, T, &tabs,
                                        bad_tab, NULL, h1, h2, kind, sid, did)
              == QHUFF_EINVAL);
        uint32_t *bad_win = words({7, 12, 100, 100, 0, 7, 0xfffffff0u,
                                   0xfffffff4u});
        CHECK(qhuff_dyn_lookup_tabs_cpu(A.bytes, A.off, A.n, sec_hdr, T, &tabs,
                                        sec_tab, bad_win, h1, h2, kind, sid,
                                        did) == QHUFF_EINVAL);
        struct qhuff_dyn_tables none = {NULL, NULL, NULL, NULL, NULL, 0};
        CHECK(qhuff_dyn_lookup_tabs_cpu(A.bytes, A.off, A.n, sec_hdr, T, &none,
                                        NULL, NULL, h1, h2, kind, sid, did)
              == QHUFF_OK);
        CHECK(did[8] == QHUFF_DYN_NONE);
        CHECK(qhuff_dyn_tables_index_slots(0) == 64
              && qhuff_dyn_tables_index_slots(33) == 128);
        // the scan: a section a table that names its entry first + 1, Base =
        // Required Insert Count = first + 2 (encoded (first + 2) % 2me + 1)
        std::vector<uint8_t> wire;
        std::vector<uint32_t> so(1, 0);
        for (uint32_t c = 0; c < T; ++c)
        {
            const uint32_t ric = firsts[c] + 2;
            wire.push_back(mes[c] ? (uint8_t) (ric % (2 * mes[c]) + 1) : 0);
            wire.push_back(0);
            wire.push_back(0x80);                  // indexed, Base - 1 - 0
            so.push_back((uint32_t) wire.size());
        }
        uint8_t *w = (uint8_t *) malloc(wire.size());
        memcpy(w, wire.data(), wire.size());
        uint32_t *sec_off = words(so), hdr_off[5], dyn_id[4];
        int32_t rc[4];
        struct qhuff_hstr *strs = (struct qhuff_hstr *) malloc(8 * 16);
        uint8_t k4[4], s4[4], f4[4];
        CHECK(qhuff_scan_headers_tabs_cpu(w, sec_off, T, &tabs, sec_tab, NULL,
                                          strs, 4, hdr_off, rc, k4, s4, f4,
                                          dyn_id) == QHUFF_OK);
        CHECK(rc[0] == QHUFF_OK && rc[3] == QHUFF_OK && hdr_off[4] == 2);
        // (an empty table: the count is above its inserts; a disabled one:
        // a dynamic line with no Required Insert Count)
        CHECK(rc[1] == QHUFF_EBLOCKED && rc[2] == QHUFF_EPROTO);
        CHECK(dyn_id[0] == firsts[0] + 1 && dyn_id[1] == firsts[3] + 1);
        CHECK(strs[0].source == QHUFF_HSTR_DYN && strs[0].instr == TB.off[2]);
        CHECK(strs[2].instr == TB.off[2 * (ent_v[3] + 1)]);
        CHECK(qhuff_scan_headers_tabs_cpu(w, sec_off, T, &tabs, bad_tab, NULL,
                                          strs, 4, hdr_off, rc, k4, s4, f4,
                                          dyn_id) == QHUFF_EINVAL);
        free(ent); free(first); free(me); free(sec_hdr); free(sec_tab);
        free(h1); free(h2); free(did); free(kind); free(sid); free(bad_tab);
        free(bad_win); free(w); free(sec_off); free(strs);
        free(A.bytes); free(A.off);
    }

    // ---- part 2: outside the rule: the clamps -------------------------------
    const uint32_t slots = dyn_index_slots(D);
    unsigned dyn_hits = 0, walked = 0;
    for (int round = 0; round < 400; ++round)
    {
        // the shared offsets: some replaced by garbage
        uint32_t *off = (uint32_t *) malloc(4 * (2 * D + 1));
        memcpy(off, TB.off, 4 * (2 * D + 1));
        const uint32_t t0 = off[0], t1 = off[2 * D];
        for (int k = 0; k < round % 5; ++k)
        {
            const uint32_t i = 1 + rnd() % (2 * D - 1);   // not the two ends
            const uint32_t kinds[4] = {0u, 0xffffffffu, off[i - 1] - 1,
                                       t1 + 1 + rnd() % 100};
            off[i] = kinds[rnd() % 4];
        }
        // ent: decreasing pairs, values past D
        std::vector<uint32_t> ev = ent_v;
        if (round % 3 == 1)
            ev[1 + rnd() % T] = rnd() % 2 ? D + 1 + rnd() % 50 : 0xffffffffu;
        if (round % 3 == 2)
        {
            const uint32_t i = 1 + rnd() % (T - 1);
            const uint32_t x = ev[i];
            ev[i] = ev[i + 1];
            ev[i + 1] = x;
        }
        uint32_t *ent = words(ev);
        uint32_t *first = words({firsts[0], firsts[1], firsts[2], firsts[3]});
        uint32_t *me = words({mes[0], mes[1], round % 7 ? 0u : 16u, mes[3]});
        // the index, each entry's first slot mixed with the table the search
        // gives it (inside [0, T - 1] whatever ent holds)
        uint32_t *idx = (uint32_t *) calloc(2 * slots, 4);
        auto claim = [](uint32_t *p, uint32_t v) {
            if (*p)
                return false;
            *p = v;
            return true;
        };
        const HashMem tb{TB.bytes};
        for (uint32_t k = 0; k < D; ++k)
        {
            const uint32_t c = tab_of_entry((const uint32_t *) ent, T, D, k);
            CHECK(c < T);
            dyn_index_insert(tb, (const uint32_t *) off, k, t0, t1, idx,
                             idx + slots, slots - 1, claim, tab_mix(c));
        }
        if (round % 4 == 1)                   // ordinals the build never wrote
            for (int k = 0; k < 4; ++k)
                idx[rnd() % (2 * slots)] = D + 1 + rnd() % 1000;
        DynTab<HashMem, const uint32_t *> t;
        t.tb = tb;
        t.off = off;
        t.nv = idx;
        t.nm = idx + slots;
        t.mask = slots - 1;
        t.d = D;
        t.first = 0;
        t.t0 = t0;
        t.t1 = t1;
        // sections: tables in and out of range, windows and Bases of any value
        const uint32_t m = 6;
        uint32_t *sec_tab = (uint32_t *) malloc(4 * m);
        uint32_t *sec_win = (uint32_t *) malloc(8 * m);
        uint32_t *sec_base = (uint32_t *) malloc(4 * m);
        for (uint32_t s = 0; s < m; ++s)
        {
            const uint32_t tabv[4] = {s % T, T, T + rnd() % 100, 0xffffffffu};
            sec_tab[s] = tabv[rnd() % 4];
            const uint32_t f = firsts[s % T];
            const uint32_t edge[6] = {0, f - 1, f + 2, f + dn[s % T],
                                      f + dn[s % T] + 1, 0xffffffffu};
            sec_win[2 * s] = edge[rnd() % 6];
            sec_win[2 * s + 1] = edge[rnd() % 6];
            sec_base[s] = edge[rnd() % 6];
        }
        const HashMem r{H.bytes};
        for (uint32_t s = 0; s < m; ++s)
        {
            const bool whole = (round + s) % 5 == 0;
            const scan::TabView v = scan::tab_view(
                (const uint32_t *) ent, (const uint32_t *) first,
                (const uint32_t *) me, T, D, (const uint32_t *) sec_tab, s);
            CHECK(v.c < T && v.e0 <= D && v.d <= D - v.e0);
            const TabSection sec = tab_section(
                (const uint32_t *) ent, (const uint32_t *) first,
                (const uint32_t *) me, T, D, (const uint32_t *) sec_tab,
                whole ? (const uint32_t *) nullptr : (const uint32_t *) sec_win,
                (const uint32_t *) sec_base, s);
            // the window as ordinals lies inside the table's
            CHECK(v.e0 <= sec.glo && sec.glo <= sec.ghi
                  && sec.ghi <= v.e0 + v.d);
            CHECK(sec.max_entries || sec.glo == sec.ghi);
            CHECK((uint64_t) sec.base <= (uint64_t) v.first + v.d);
            uint32_t ric = 0;
            for (uint32_t i = 0; i < hn; ++i)
            {
                const uint32_t a = H.off[2 * i], mid = H.off[2 * i + 1],
                               b = H.off[2 * i + 2];
                const uint32_t h1 = xxh32(r, a, mid - a, QHUFF_XXH_SEED);
                const uint32_t h2 = xxh32(r, mid, b - mid, h1);
                const DynHit raw = dyn_lookup(r, a, mid, b, h1, h2, kStatic, t,
                                              sec.glo, sec.ghi, sec.mix);
                const bool dyn = (raw.kind & QHUFF_LINE_DYN) != 0;
                CHECK(dyn == (raw.dyn != QHUFF_DYN_NONE));
                // an ordinal of the section's own table and window
                CHECK(!dyn || (sec.glo <= raw.dyn && raw.dyn < sec.ghi));
                const DynHit hit = tab_hit(raw, sec.delta);
                if (dyn)
                {
                    ++dyn_hits;
                    CHECK(hit.dyn - v.first == raw.dyn - v.e0);
                    ric = hit.dyn + 1 > ric ? hit.dyn + 1 : ric;
                }
                (void) dyn_line_items(hit, sec.base, i & 1);
            }
            const ItemWords pre = dyn_prefix_items(ric, sec.base,
                                                   sec.max_entries);
            CHECK(pre.w[0] <= 2 * sec.max_entries);
            CHECK((pre.w[1] & 0xff) == 8 && (pre.w[3] & 0xff) == 7);
            // the walk's view of the same section: every index of the window
            // has its three offsets inside `off`
            const scan::DynWin w = scan::dyn_win_tabs(
                off, ent, first, me, T, D, sec_tab, whole ? nullptr : sec_win,
                s);
            CHECK(w.off >= off && w.off + 2 * v.d <= off + 2 * D);
            CHECK(w.lo >= w.first && w.ins <= (uint64_t) w.first + v.d);
            // a section that names every index from lo - 1 to ins: Required
            // Insert Count and Base = ins; rule 4 cuts what is outside
            uint8_t wire[3] = {0, 0, 0};
            if (w.max_entries && w.ins > w.lo)
            {
                wire[0] = (uint8_t) (w.ins % (2ull * w.max_entries) + 1);
                wire[2] = (uint8_t) (0x80 | (rnd() % 2 ? 0 : rnd() % 8));
                uint8_t *heap = (uint8_t *) malloc(3);
                memcpy(heap, wire, 3);
                Reader rd{heap};
                struct qhuff_hstr strs[2];
                uint8_t k1, s1, f1;
                uint32_t d1 = QHUFF_DYN_NONE;
                scan::HdrDynWriteSink sink{{strs, &k1, &s1, &f1, 0, 1}, &d1};
                const int rc = scan::walk_header_section(rd, sink, 0, 3, w);
                CHECK(rc == QHUFF_OK || rc == QHUFF_EPROTO
                      || rc == QHUFF_EBLOCKED);
                if (rc == QHUFF_OK)
                {
                    ++walked;
                    CHECK(w.lo <= d1 && d1 < w.ins);
                }
                free(heap);
            }
        }
        free(off); free(ent); free(first); free(me); free(idx);
        free(sec_tab); free(sec_win); free(sec_base);
    }
    CHECK(dyn_hits > 1000);
    CHECK(walked > 50);
    free(TB.bytes);
    free(TB.off);
    free(H.bytes);
    free(H.off);
    printf("ok: %u dynamic hits and %u walked sections under the clamps\n",
           dyn_hits, walked);
    return 0;
}
