// hdrscan_dyn_san.cpp -- the header scan's walker with the dynamic table's
// entries on the CPU (qhuff_scan_headers_dyn_cpu, the kernels' source in
// csrc/qhuff_scan_impl.h) under ASan/UBSan, against the model's results
// (tests/headers_dyn_model.py).  Stand-alone: built by
// tests/test_scan_headers_dyn.py with qhuff_frames.cpp and nothing else.
//
// usage: hdrscan_dyn_san TABLE [FILE EXPECT]...
// TABLE: u32 d, first, max_entries, then off[2d + 1] (off[0] = 0) and the
// off[2d] bytes.  FILE: u32 has_win, then records of u32 LE length + payload,
// one section each, each followed by its window (2 x u32) when has_win.
// EXPECT: u32 m, u32 n, rc[m] (i32), hdr_off[m + 1], the 2n descriptors,
// kind[n], static_id[n], hflags[n], dyn_id[n] (u32).  Wire bytes, table
// bytes, off and sec_win lie in heap buffers of exactly their size, the
// outputs too, at max_hdrs = the total, the total - 1 and 0, with and without
// the optional arrays.
//
// Then the walker's clamps, which the _cpu form's argument check keeps callers
// from reaching: every section is walked again through the walker itself
// with windows and offsets outside the rule (windows past the table, reversed,
// huge; offsets decreasing and random).  There is no expectation but that no
// access leaves the arrays.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/qhuff.h"
#include "../../ls-qpack_amd/csrc/qhuff_scan_impl.h"

static int
die(const char *file, const char *what, size_t i)
{
    fprintf(stderr, "%s: %s at %zu\n", file, what, i);
    return 1;
}

static bool
slurp(const char *path, std::vector<uint8_t> *raw)
{
    FILE *f = fopen(path, "rb");
    if (!f)
    {
        perror(path);
        return false;
    }
    uint8_t tmp[65536];
    size_t n;
    while ((n = fread(tmp, 1, sizeof(tmp), f)) > 0)
        raw->insert(raw->end(), tmp, tmp + n);
    fclose(f);
    return true;
}

struct Table
{
    qhuff_dyn_table t;
    uint8_t *bytes;
    uint32_t *off;
};

static bool
load_table(const std::vector<uint8_t> &raw, Table *o)
{
    if (raw.size() < 12)
        return false;
    uint32_t h[3];
    memcpy(h, raw.data(), 12);
    const size_t no = 2 * (size_t) h[0] + 1;
    if (raw.size() < 12 + 4 * no)
        return false;
    o->off = (uint32_t *) malloc(4 * no);
    memcpy(o->off, &raw[12], 4 * no);
    const size_t nb = o->off[no - 1];
    if (raw.size() != 12 + 4 * no + nb)
        return false;
    o->bytes = (uint8_t *) malloc(nb ? nb : 1);
    memcpy(o->bytes, &raw[12 + 4 * no], nb);
    o->t.bytes = h[0] ? o->bytes : nullptr;
    o->t.off = h[0] ? o->off : nullptr;
    o->t.d = h[0];
    o->t.first = h[1];
    o->t.max_entries = h[2];
    return true;
}

namespace {
struct Reader
{
    const uint8_t *buf;
    uint8_t get(uint32_t pos) const { return buf[pos]; }
};
}  // namespace

// the walker over windows and offsets outside the rule
static void
clamps(const uint8_t *buf, const uint32_t *sec_off, uint32_t m, const Table &tb,
       uint32_t total)
{
    namespace qs = qhuff::scan;
    const uint32_t d = tb.t.d, first = tb.t.first;
    const size_t no = 2 * (size_t) d + 1;
    uint32_t *off = (uint32_t *) malloc(4 * no);
    uint32_t *win = (uint32_t *) malloc(m ? 8 * (size_t) m : 1);
    uint32_t x = 2463534242u;
    auto rnd = [&]() {
        x ^= x << 13;
        x ^= x >> 17;
        x ^= x << 5;
        return x;
    };
    for (int round = 0; round < 4; ++round)
    {
        for (size_t i = 0; i < no; ++i)
            off[i] = round == 0 ? tb.off[i]
                   : round == 1 ? tb.off[no - 1 - i]       // decreasing
                   : rnd();
        for (uint32_t s = 0; s < m; ++s)
        {
            const uint32_t k = rnd() % 6;
            win[2 * s] = k == 0 ? 0 : k == 1 ? 0xffffffffu
                       : k == 2 ? first + d : k == 3 ? first - 1 : rnd();
            win[2 * s + 1] = k == 0 ? 0xffffffffu : k == 1 ? 0
                           : k == 2 ? first + d + 1 + rnd() % 9
                           : k == 3 ? first + d / 2 : rnd();
        }
        const size_t cap = (size_t) total + 64;
        qhuff_hstr *strs = (qhuff_hstr *) malloc(32 * cap);
        uint32_t *did = (uint32_t *) malloc(4 * cap);
        uint8_t *kind = (uint8_t *) malloc(cap);
        Reader r{buf};
        for (uint32_t s = 0; s < m; ++s)
        {
            const qs::DynWin w = qs::DynWin::of(off, d, first,
                                                tb.t.max_entries, win, s);
            qs::HdrDynCountSink c{0};
            (void) qs::walk_header_section(r, c, sec_off[s], sec_off[s + 1], w);
            // (a section's headers are at most its bytes)
            qs::HdrDynWriteSink ws{{strs, kind, nullptr, nullptr, 0,
                                    c.n < cap ? c.n : (uint32_t) cap}, did};
            (void) qs::walk_header_section(r, ws, sec_off[s], sec_off[s + 1],
                                           w);
        }
        free(strs);
        free(did);
        free(kind);
    }
    free(off);
    free(win);
}

static int
run(const char *file, const Table &tb, const std::vector<uint8_t> &raw,
    const std::vector<uint8_t> &exp)
{
    if (raw.size() < 4)
        return die(file, "short file", 0);
    uint32_t has_win;
    memcpy(&has_win, &raw[0], 4);
    std::vector<uint32_t> off(1, 0), wins;
    size_t at = 4, bytes = 0;
    std::vector<const uint8_t *> src;
    while (at + 4 <= raw.size())
    {
        uint32_t n;
        memcpy(&n, &raw[at], 4);
        at += 4;
        if (n > raw.size() - at)
            return die(file, "bad record", at);
        src.push_back(raw.data() + at);
        at += n;
        bytes += n;
        off.push_back((uint32_t) bytes);
        if (has_win)
        {
            if (raw.size() - at < 8)
                return die(file, "bad window", at);
            uint32_t w[2];
            memcpy(w, &raw[at], 8);
            at += 8;
            wins.push_back(w[0]);
            wins.push_back(w[1]);
        }
    }
    const uint32_t m = (uint32_t) src.size();
    uint32_t em, total;
    if (exp.size() < 8)
        return die(file, "short expectation", 0);
    memcpy(&em, &exp[0], 4);
    memcpy(&total, &exp[4], 4);
    const size_t need = 8 + 4 * (size_t) m + 4 * ((size_t) m + 1)
                      + 39 * (size_t) total;
    if (em != m || exp.size() != need)
        return die(file, "expectation size", exp.size());
    const uint8_t *w_rc = &exp[8];
    const uint8_t *w_off = w_rc + 4 * (size_t) m;
    const uint8_t *w_strs = w_off + 4 * ((size_t) m + 1);
    const uint8_t *w_kind = w_strs + 32 * (size_t) total;
    const uint8_t *w_id = w_kind + total, *w_hf = w_id + total;
    const uint8_t *w_did = w_hf + total;

    uint8_t *buf = (uint8_t *) malloc(bytes ? bytes : 1);
    for (uint32_t i = 0; i < m; ++i)
        memcpy(buf + off[i], src[i], off[i + 1] - off[i]);
    uint32_t *sec_off = (uint32_t *) malloc(4 * ((size_t) m + 1));
    memcpy(sec_off, off.data(), 4 * ((size_t) m + 1));
    uint32_t *sec_win = nullptr;
    if (has_win)
    {
        sec_win = (uint32_t *) malloc(m ? 8 * (size_t) m : 1);
        memcpy(sec_win, wins.data(), 8 * (size_t) m);
    }

    const uint32_t caps[3] = {total, total ? total - 1 : 0, 0};
    for (int opt = 0; opt < 2; ++opt)
        for (uint32_t cap : caps)
        {
            qhuff_hstr *strs = (qhuff_hstr *) malloc(cap ? 32 * (size_t) cap : 1);
            uint32_t *hdr_off = (uint32_t *) malloc(4 * ((size_t) m + 1));
            int32_t *rc = (int32_t *) malloc(m ? 4 * (size_t) m : 1);
            uint8_t *kind = opt ? (uint8_t *) malloc(cap ? cap : 1) : nullptr;
            uint8_t *id = opt ? (uint8_t *) malloc(cap ? cap : 1) : nullptr;
            uint8_t *hf = opt ? (uint8_t *) malloc(cap ? cap : 1) : nullptr;
            uint32_t *did = opt ? (uint32_t *) malloc(cap ? 4 * (size_t) cap : 1)
                                : nullptr;
            const int r = qhuff_scan_headers_dyn_cpu(buf, sec_off, m, &tb.t,
                                                     sec_win, strs, cap,
                                                     hdr_off, rc, kind, id,
                                                     hf, did);
            if (r != (total > cap ? QHUFF_ERANGE : QHUFF_OK))
                return die(file, "return value", cap);
            if (memcmp(hdr_off, w_off, 4 * ((size_t) m + 1)))
                return die(file, "hdr_off", cap);
            if (m && memcmp(rc, w_rc, 4 * (size_t) m))
                return die(file, "rc", cap);
            if (cap && memcmp(strs, w_strs, 32 * (size_t) cap))
                return die(file, "descriptors", cap);
            if (opt && cap && (memcmp(kind, w_kind, cap) || memcmp(id, w_id, cap)
                               || memcmp(hf, w_hf, cap)
                               || memcmp(did, w_did, 4 * (size_t) cap)))
                return die(file, "kind / static_id / hflags / dyn_id", cap);
            free(strs);
            free(hdr_off);
            free(rc);
            free(kind);
            free(id);
            free(hf);
            free(did);
        }
    clamps(buf, sec_off, m, tb, total);
    free(buf);
    free(sec_off);
    free(sec_win);
    printf("%s: %u sections, %u headers\n", file, m, total);
    return 0;
}

int
main(int argc, char **argv)
{
    if (argc < 4 || (argc & 1))
    {
        fprintf(stderr,
                "usage: hdrscan_dyn_san TABLE FILE EXPECT [FILE EXPECT]...\n");
        return 2;
    }
    std::vector<uint8_t> traw;
    Table tb;
    if (!slurp(argv[1], &traw) || !load_table(traw, &tb))
        return 2;
    for (int k = 2; k + 1 < argc; k += 2)
    {
        std::vector<uint8_t> raw, exp;
        if (!slurp(argv[k], &raw) || !slurp(argv[k + 1], &exp))
            return 2;
        if (run(argv[k], tb, raw, exp))
            return 1;
    }
    free(tb.bytes);
    free(tb.off);
    return 0;
}
