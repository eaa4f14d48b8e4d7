// lookup_dyn_san.cpp -- the dynamic lookup's source on the CPU
// (csrc/qhuff_lookup_dyn_impl.h: the index build, the lookup, the clamps of
// windows, Bases and table offsets, the items) under ASan/UBSan.
// Stand-alone: built by tests/test_encode_headers_dyn.py with
// qhuff_frames.cpp and nothing else.
//
// Every array is a heap buffer of exactly its size: a read that leaves one
// is an ASan report.  Part 1 runs qhuff_dyn_lookup_cpu on inputs inside the
// rule and checks a few answers.  Part 2 drives the source itself, as the
// device form runs it where nothing can be checked, over table offsets that
// decrease or point past the table's bytes, index slots that hold ordinals
// past d, and windows and Bases outside [first, first + d]: the results must
// stay inside the table and the window.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/qhuff.h"
#include "../../ls-qpack_amd/csrc/qhuff_lookup_dyn_impl.h"

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

}  // namespace

int
main()
{
    using namespace qhuff;
    std::vector<std::pair<std::string, std::string>> ents, hs;
    for (int k = 0; k < 40; ++k)
        ents.push_back({"x-e" + std::to_string(k % 30),
                        "v" + std::to_string(k)});
    ents.push_back({"", ""});
    ents.push_back({"x-long", std::string(5000, 'q')});
    const uint32_t d = (uint32_t) ents.size(), first = 7;
    for (const auto &e : ents)
    {
        hs.push_back(e);
        hs.push_back({e.first, e.second + "x"});
        hs.push_back({e.first + "y", e.second});
    }
    hs.push_back({":method", "GET"});
    hs.push_back({":path", "/nowhere"});
    const Packed T = pack(ents, 3), H = pack(hs, 5);

    // ---- part 1: inside the rule ------------------------------------------
    {
        struct qhuff_dyn_table tab = {T.bytes, T.off, d, first, 64};
        uint32_t *h1 = (uint32_t *) malloc(4 * H.n);
        uint32_t *h2 = (uint32_t *) malloc(4 * H.n);
        uint32_t *did = (uint32_t *) malloc(4 * H.n);
        uint8_t *kind = (uint8_t *) malloc(H.n), *sid = (uint8_t *) malloc(H.n);
        CHECK(qhuff_dyn_lookup_cpu(H.bytes, H.off, H.n, &tab, first, first + d,
                                   h1, h2, kind, sid, did) == QHUFF_OK);
        // entry 35 = (x-e5, v35): the only equal entry; its name first at 5
        CHECK(kind[3 * 35] == (QHUFF_LINE_INDEXED | QHUFF_LINE_DYN));
        CHECK(did[3 * 35] == first + 35);
        CHECK(kind[3 * 35 + 1] == (QHUFF_LINE_NAMEREF | QHUFF_LINE_DYN));
        CHECK(did[3 * 35 + 1] == first + 5);
        CHECK(kind[3 * 35 + 2] == QHUFF_LINE_LITERAL);
        CHECK(did[3 * 35 + 2] == QHUFF_DYN_NONE);
        CHECK(kind[3 * 41] == (QHUFF_LINE_INDEXED | QHUFF_LINE_DYN));
        CHECK(kind[H.n - 2] == QHUFF_LINE_INDEXED && sid[H.n - 2] == 17);
        CHECK(kind[H.n - 1] == QHUFF_LINE_NAMEREF && sid[H.n - 1] == 1);
        // a narrower window, null hashes and dyn_id, d = 0, the checks
        CHECK(qhuff_dyn_lookup_cpu(H.bytes, H.off, H.n, &tab, first + 10,
                                   first + 36, NULL, NULL, kind, sid, NULL)
              == QHUFF_OK);
        CHECK(kind[3 * 5 + 1] == (QHUFF_LINE_NAMEREF | QHUFF_LINE_DYN));
        struct qhuff_dyn_table none = {NULL, NULL, 0, first, 64};
        CHECK(qhuff_dyn_lookup_cpu(H.bytes, H.off, H.n, &none, first, first,
                                   h1, h2, kind, sid, did) == QHUFF_OK);
        CHECK(did[3 * 35] == QHUFF_DYN_NONE);
        CHECK(qhuff_dyn_lookup_cpu(H.bytes, H.off, H.n, &tab, first - 1,
                                   first + 2, h1, h2, kind, sid, did)
              == QHUFF_EINVAL);
        CHECK(qhuff_dyn_lookup_cpu(H.bytes, H.off, H.n, &tab, first,
                                   first + d + 1, h1, h2, kind, sid, did)
              == QHUFF_EINVAL);
        CHECK(qhuff_dyn_lookup_cpu(H.bytes, H.off, H.n, NULL, 0, 0, h1, h2,
                                   kind, sid, did) == QHUFF_EINVAL);
        CHECK(qhuff_dyn_index_slots(0) == 64 && qhuff_dyn_index_slots(32) == 64
              && qhuff_dyn_index_slots(33) == 128);
        free(h1);
        free(h2);
        free(did);
        free(kind);
        free(sid);
    }

    // ---- part 2: outside the rule: the clamps -------------------------------
    const uint32_t slots = dyn_index_slots(d);
    unsigned dyn_hits = 0;
    for (int round = 0; round < 300; ++round)
    {
        // the table's offsets: some entries' replaced by garbage
        uint32_t *off = (uint32_t *) malloc(4 * (2 * d + 1));
        memcpy(off, T.off, 4 * (2 * d + 1));
        const uint32_t t0 = off[0], t1 = off[2 * d];
        for (int k = 0; k < round % 7; ++k)
        {
            const uint32_t i = 1 + rnd() % (2 * d - 1);   // not the two ends
            const uint32_t kinds[4] = {0u, 0xffffffffu, off[i - 1] - 1,
                                       t1 + 1 + rnd() % 100};
            off[i] = kinds[rnd() % 4];
        }
        uint32_t *idx = (uint32_t *) calloc(2 * slots, 4);
        auto claim = [](uint32_t *p, uint32_t v) {
            if (*p)
                return false;
            *p = v;
            return true;
        };
        const HashMem tb{T.bytes};
        for (uint32_t k = 0; k < d; ++k)
            dyn_index_insert(tb, (const uint32_t *) off, k, t0, t1, idx,
                             idx + slots, slots - 1, claim);
        // slots that hold ordinals the build never wrote
        if (round % 3 == 1)
            for (int k = 0; k < 6; ++k)
                idx[rnd() % (2 * slots)] = d + 1 + rnd() % 1000;
        if (round % 11 == 5)                  // a full index: the probe ends
            for (uint32_t i = 0; i < 2 * slots; ++i)
                idx[i] = idx[i] ? idx[i] : 0x80000000u + i;
        DynTab<HashMem, const uint32_t *> t;
        t.tb = tb;
        t.off = off;
        t.nv = idx;
        t.nm = idx + slots;
        t.mask = slots - 1;
        t.d = d;
        t.first = first;
        t.t0 = t0;
        t.t1 = t1;
        // windows and Bases of any value
        const uint64_t edge[6] = {0, first - 1, first + d / 2, first + d,
                                  (uint64_t) first + d + 1, ~0ull};
        const uint64_t wl = edge[rnd() % 6], wh = edge[rnd() % 6];
        const uint32_t me = round % 5 ? 64 : 0;
        const DynRange w = dyn_window(wl, wh, first, d, me);
        CHECK(first <= w.lo && w.lo <= w.hi && w.hi <= first + d);
        CHECK(me || w.lo == w.hi);
        const uint32_t base = dyn_base(edge[rnd() % 6], first, d);
        CHECK(base <= first + d);
        const HashMem r{H.bytes};
        uint32_t ric = 0;
        for (uint32_t i = 0; i < H.n; ++i)
        {
            const uint32_t a = H.off[2 * i], m = H.off[2 * i + 1],
                           b = H.off[2 * i + 2];
            const uint32_t h1 = xxh32(r, a, m - a, QHUFF_XXH_SEED);
            const uint32_t h2 = xxh32(r, m, b - m, h1);
            const DynHit hit = dyn_lookup(r, a, m, b, h1, h2, kStatic, t, w.lo,
                                          w.hi);
            const bool dyn = (hit.kind & QHUFF_LINE_DYN) != 0;
            CHECK(dyn == (hit.dyn != QHUFF_DYN_NONE));
            CHECK(!dyn || (w.lo <= hit.dyn && hit.dyn < w.hi));
            const ItemWords it = dyn_line_items(hit, base, i & 1);
            if (dyn)
            {
                ++dyn_hits;
                CHECK(it.w[0] < first + d);   // a relative index in the table
                ric = hit.dyn + 1 > ric ? hit.dyn + 1 : ric;
            }
        }
        const ItemWords pre = dyn_prefix_items(ric, base, me);
        CHECK(pre.w[0] <= 2 * me && pre.w[2] <= first + d);
        CHECK((pre.w[1] & 0xff) == 8 && (pre.w[3] & 0xff) == 7);
        free(idx);
        free(off);
    }
    CHECK(dyn_hits > 1000);
    free(T.bytes);
    free(T.off);
    free(H.bytes);
    free(H.off);
    printf("ok: %u dynamic hits under the clamps\n", dyn_hits);
    return 0;
}
