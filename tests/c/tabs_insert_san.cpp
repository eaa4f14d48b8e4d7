// tabs_insert_san.cpp -- the source that applies encoder-stream inserts to a
// set of tables (csrc/qhuff_scan_impl.h walk_insert_stream and its sinks,
// csrc/qhuff_tabs_insert_impl.h account / sums_host / copy_host) on the CPU
// under ASan/UBSan.  Stand-alone: built by tests/test_tabs_insert.py with
// qhuff_frames.cpp and nothing else.
//
// Every array is a heap buffer of exactly its size: an access that leaves one
// is an ASan report.  Part 1 runs qhuff_tabs_insert_cpu on the RFC 9204
// Appendix B encoder stream, whole and cut at every position, and checks the
// answers.  Part 2 drives the shared source itself, as the device forms run it
// where nothing can be checked: ent that decreases or passes D, off that
// decreases or points past the bytes, live_lo and keep outside their table,
// ins_off outside the inserts, roots that point anywhere, kinds, references
// and capacities of any value.  The results are not looked at: the accounting
// and the copy must stay inside the arrays, out_bytes inside out_cap and
// out_off inside ent_cap.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/qhuff.h"
#include "../../ls-qpack_amd/csrc/qhuff_tabs_insert_impl.h"

namespace {

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

// a heap array of exactly n elements (at least one byte)
template <class T>
struct Heap
{
    T *p;
    size_t n;
    explicit Heap(size_t n_) : n(n_)
    {
        p = (T *) malloc(n ? n * sizeof(T) : 1);
        memset(p, 0, n * sizeof(T));
    }
    Heap(const std::vector<T> &v) : Heap(v.size())
    {
        if (v.size())
            memcpy(p, v.data(), v.size() * sizeof(T));
    }
    ~Heap() { free(p); }
    Heap(const Heap &) = delete;
    T &operator[](size_t i) { return p[i]; }
};

const uint8_t kRfc[74] = {
    0x3f, 0xbd, 0x01, 0xc0, 0x0f, 0x77, 0x77, 0x77, 0x2e, 0x65, 0x78, 0x61,
    0x6d, 0x70, 0x6c, 0x65, 0x2e, 0x63, 0x6f, 0x6d, 0xc1, 0x0c, 0x2f, 0x73,
    0x61, 0x6d, 0x70, 0x6c, 0x65, 0x2f, 0x70, 0x61, 0x74, 0x68, 0x4a, 0x63,
    0x75, 0x73, 0x74, 0x6f, 0x6d, 0x2d, 0x6b, 0x65, 0x79, 0x0c, 0x63, 0x75,
    0x73, 0x74, 0x6f, 0x6d, 0x2d, 0x76, 0x61, 0x6c, 0x75, 0x65, 0x02, 0x81,
    0x0d, 0x63, 0x75, 0x73, 0x74, 0x6f, 0x6d, 0x2d, 0x76, 0x61, 0x6c, 0x75,
    0x65, 0x32};

// the RFC stream cut at `cut`, applied to T copies of an empty table
int
rfc_case(uint32_t cut, uint32_t T)
{
    const uint32_t max_ins = 5 * T;
    Heap<uint8_t> buf(cut * T);
    Heap<uint32_t> enc_off(T + 1), ent(T + 1), first(T), me(T), cap(T),
        max_cap(T), lo(T);
    for (uint32_t c = 0; c < T; ++c)
    {
        memcpy(buf.p + cut * c, kRfc, cut);
        enc_off[c + 1] = cut * (c + 1);
        me[c] = 220 / 32;
        max_cap[c] = 220;
    }
    struct qhuff_dyn_tables tabs = {nullptr, nullptr, ent.p, first.p, me.p, T};
    struct qhuff_ins_state st = {cap.p, max_cap.p, lo.p, 0, 0};
    Heap<int32_t> rc(T);
    Heap<uint32_t> consumed(T), ins_off(T + 1), ins_ref(max_ins),
        ins_lo(max_ins), out_ent(T + 1), out_first(T), cap_out(T), lo_out(T),
        out_off(2 * max_ins + 1);
    Heap<uint8_t> kind(max_ins);
    const uint64_t bound = qhuff_tabs_insert_bound(0, cut * T, max_ins, 0);
    Heap<uint8_t> out(bound);
    struct qhuff_ins_scan sc = {rc.p, consumed.p, ins_off.p, nullptr, nullptr,
                                nullptr, nullptr, ins_ref.p, kind.p, max_ins};
    struct qhuff_ins_out o = {ins_lo.p, out.p, out_off.p, out_ent.p,
                              out_first.p, cap_out.p, lo_out.p, bound,
                              max_ins};
    CHECK(qhuff_tabs_insert_cpu(&tabs, &st, buf.p, enc_off.p, nullptr, &sc, &o)
          == QHUFF_OK);
    static const uint32_t ends[] = {3, 20, 34, 58, 59, 74};
    uint32_t want = 0, n = 0;
    for (uint32_t k = 0; k < 6; ++k)
        if (ends[k] <= cut)
        {
            want = ends[k];
            n = k;
        }
    for (uint32_t c = 0; c < T; ++c)
    {
        CHECK(rc[c] == QHUFF_OK && consumed[c] == want);
        CHECK(ins_off[c + 1] - ins_off[c] == n);
        CHECK(cap_out[c] == (cut >= 3 ? 220u : 0u));
        CHECK(lo_out[c] == (n == 5 ? 1u : 0u));
        CHECK(out_ent[c + 1] - out_ent[c] == (n == 5 ? 4u : n));
    }
    if (cut == 74)
    {
        CHECK(out_off[2 * out_ent[1]] == 215 - 4 * 32);
        CHECK(!memcmp(out.p, ":path/sample/pathcustom-key", 27));
        CHECK(kind[4] == QHUFF_INS_DYN && ins_ref[4] == 2 && ins_lo[4] == 1);
    }
    return 0;
}

// a set of T tables with entries of random sizes, a chunk a table built from
// the four instructions, scanned by the shared walker; then everything the
// caller owes is overwritten with noise (mode bits) and the accounting, the
// sums and the copy run on it
int
noise_case(uint32_t T, uint32_t mode)
{
    namespace qs = qhuff::scan;
    namespace qi = qhuff::ins;
    std::vector<uint32_t> ent(1, 0), off(1, 3), first, cap, max_cap, lo,
        enc_off(1, 0);
    std::vector<uint8_t> bytes(3, '#'), wire;
    for (uint32_t c = 0; c < T; ++c)
    {
        const uint32_t d = rnd() % 5;
        for (uint32_t k = 0; k < 2 * d; ++k)
        {
            const uint32_t l = rnd() % 9;
            bytes.insert(bytes.end(), l, (uint8_t) ('a' + k));
            off.push_back((uint32_t) bytes.size());
        }
        ent.push_back(ent.back() + d);
        first.push_back(rnd() % 50);
        lo.push_back(first.back() + (d ? rnd() % (d + 1) : 0));
        max_cap.push_back(64 + rnd() % 300);
        cap.push_back(max_cap.back());
        const uint32_t k_ins = rnd() % 6;
        for (uint32_t k = 0; k < k_ins; ++k)
            switch (rnd() % 5)
            {
            case 0:                                  // duplicate
                wire.push_back((uint8_t) (rnd() % 4));
                break;
            case 1:                                  // set capacity
                wire.push_back((uint8_t) (0x20 | rnd() % 31));
                break;
            case 2:                                  // static name, raw value
                wire.push_back((uint8_t) (0xc0 | rnd() % 60));
                wire.push_back(2);
                wire.push_back('v');
                wire.push_back('w');
                break;
            case 3:                                  // dynamic name
                wire.push_back((uint8_t) (0x80 | rnd() % 5));
                wire.push_back(1);
                wire.push_back('x');
                break;
            default:                                 // literal name
                wire.push_back(0x42);
                wire.push_back('n');
                wire.push_back('m');
                wire.push_back(0x81);                // Huffman: "a" (00011|111)
                wire.push_back(0x1f);
            }
        enc_off.push_back((uint32_t) wire.size());
    }
    const uint32_t D = ent.back();
    Heap<uint8_t> h_bytes(bytes), h_wire(wire);
    Heap<uint32_t> h_off(off), h_ent(ent), h_first(first), h_cap(cap),
        h_max(max_cap), h_lo(lo), h_enc(enc_off);
    struct HostReader
    {
        const uint8_t *buf;
        uint8_t get(uint32_t pos) const { return buf[pos]; }
    } r{h_wire.p};
    // the scan, as qhuff_tabs_insert_cpu runs it
    Heap<int32_t> rc(T);
    Heap<uint32_t> consumed(T), ins_off(T + 1), chunk_cap(2 * T);
    for (uint32_t c = 0; c < T; ++c)
    {
        qs::InsCountSink s{0, cap[c], cap[c]};
        uint32_t stop = enc_off[c];
        const int e = qs::walk_insert_stream(r, s, enc_off[c], enc_off[c + 1],
                                             cap[c], max_cap[c], &stop);
        rc[c] = e ? QHUFF_EPROTO : QHUFF_OK;
        consumed[c] = e ? 0 : stop - enc_off[c];
        chunk_cap[2 * c] = e ? cap[c] : s.cmin;
        chunk_cap[2 * c + 1] = e ? cap[c] : s.cap;
        ins_off[c + 1] = ins_off[c] + (e ? 0 : s.n);
    }
    const uint32_t n = ins_off[T];
    Heap<struct qhuff_hstr> strs(2 * n);
    Heap<uint32_t> root(2 * n), ins_cap(2 * n), ins_ref(n);
    Heap<uint8_t> kind(n);
    for (uint32_t c = 0; c < T; ++c)
    {
        if (ins_off[c + 1] == ins_off[c])
            continue;
        const qs::TabView v = qs::ins_tab_view(h_ent.p, h_first.p, D, c);
        qs::InsWriteSink w{strs.p, root.p, ins_cap.p, ins_ref.p, kind.p,
                           h_off.p + 2ull * v.e0, v.d, v.first, ins_off[c],
                           ins_off[c], ins_off[c + 1]};
        uint32_t stop;
        (void) qs::walk_insert_stream(r, w, enc_off[c], enc_off[c + 1], cap[c],
                                      max_cap[c], &stop);
    }
    // a decode result of random lengths (the decode launch's own output is
    // the library's, not the caller's: its form holds)
    Heap<uint32_t> dec_off(2 * n + 1);
    Heap<uint8_t> status(2 * n);
    for (uint32_t s = 0; s < 2 * n; ++s)
    {
        dec_off[s + 1] = dec_off[s] + rnd() % 12;
        status[s] = rnd() % 16 == 0;
    }
    Heap<uint8_t> dec(dec_off[2 * n]);
    // the caller's arrays turned to noise
    Heap<uint32_t> keep(T);
    auto wild = [&](uint32_t range) {
        const uint32_t x = rnd();
        return x % 4 == 0 ? 0xffffffffu - x % 3 : x % (range + 2);
    };
    for (uint32_t c = 0; c < T; ++c)
        keep[c] = mode & 1 ? wild(60) : lo[c];
    if (mode & 2)
        for (uint32_t c = 0; c <= T; ++c)
            h_ent[c] = wild(D + 3);
    if (mode & 4)
        for (size_t i = 0; i < off.size(); ++i)
            h_off[i] = wild((uint32_t) bytes.size() + 40);
    if (mode & 8)
        for (uint32_t c = 0; c < T; ++c)
        {
            h_lo[c] = wild(70);
            h_first[c] = mode & 1 ? wild(70) : h_first[c];
        }
    if (mode & 16)
        for (uint32_t c = 0; c <= T; ++c)
            ins_off[c] = wild(n + 3);
    if (mode & 32)
        for (uint32_t s = 0; s < 2 * n; ++s)
        {
            root[s] = wild(2 * n + 3);
            ins_cap[s] = wild(400);
            ins_ref[s / 2] = wild(80);
            kind[s / 2] = (uint8_t) rnd();
            strs[s].len = wild(500);
            strs[s].huffman = (uint8_t) rnd();
        }
    const uint32_t ent_cap = D + n;
    const uint64_t out_cap = mode & 64 ? rnd() % 40
                                       : bytes.size() + dec_off[2 * n] + 16;
    Heap<uint8_t> out(out_cap);
    Heap<uint32_t> fin(2 * n), rel(2 * n), plan(4 * T), ins_lo(n),
        out_off(2 * ent_cap + 1), out_ent(T + 1), out_first(T), cap_out(T),
        lo_out(T);
    Heap<uint64_t> sums(2 * (T + 1));
    qi::Args a;
    a.bytes = h_bytes.p;
    a.off = h_off.p;
    a.ent = h_ent.p;
    a.first = h_first.p;
    a.cap = h_cap.p;
    a.live_lo = h_lo.p;
    a.keep = mode & 128 ? nullptr : keep.p;
    a.T = T;
    a.D = h_ent[T] < D ? h_ent[T] : D;    // (the kernels read ent[T]; off holds
                                          // 2D + 1 entries: ent[T] is owed)
    a.arena = (uint32_t) bytes.size();
    a.rc = rc.p;
    a.consumed = consumed.p;
    a.ins_off = ins_off.p;
    a.chunk_cap = chunk_cap.p;
    a.strs = strs.p;
    a.root = root.p;
    a.ins_cap = ins_cap.p;
    a.ins_ref = ins_ref.p;
    a.ins_kind = kind.p;
    a.n_ins = n;
    a.dec = dec.p;
    a.dec_off = dec_off.p;
    a.status = status.p;
    a.fin = fin.p;
    a.rel = rel.p;
    a.plan = plan.p;
    a.sums = sums.p;
    a.ins_lo = ins_lo.p;
    a.out_bytes = out.p;
    a.out_off = out_off.p;
    a.out_ent = out_ent.p;
    a.out_first = out_first.p;
    a.cap_out = cap_out.p;
    a.live_lo_out = lo_out.p;
    a.out_cap = out_cap;
    a.ent_cap = ent_cap;
    for (uint32_t c = 0; c < T; ++c)
        qi::account(a, c);
    qi::sums_host(a);
    for (uint32_t c = 0; c < T; ++c)
        qi::copy_host(a, c);
    if (!mode)
    {
        // inside the rule: the next set is a set
        CHECK(out_ent[0] == 0);
        for (uint32_t c = 0; c < T; ++c)
        {
            CHECK(out_ent[c + 1] >= out_ent[c]);
            CHECK(lo_out[c] >= out_first[c]);
        }
        for (uint32_t i = 0; i < 2 * out_ent[T]; ++i)
            CHECK(out_off[i + 1] >= out_off[i]);
        CHECK(out_off[2 * out_ent[T]] <= out_cap);
    }
    return 0;
}

}  // namespace

int
main()
{
    for (uint32_t cut = 0; cut <= 74; ++cut)
        if (rfc_case(cut, 1 + cut % 3))
            return 1;
    for (uint32_t round = 0; round < 40; ++round)
        for (uint32_t mode = 0; mode < 256; mode += 1 + (round & 1) * 6)
            if (noise_case(1 + rnd() % 9, mode))
                return 1;
    if (noise_case(300, 0) || noise_case(300, 255))
        return 1;
    printf("ok\n");
    return 0;
}
