// hdrscan_san.cpp -- the header scan's walker on the CPU (qhuff_scan_headers_cpu,
// the kernels' source in csrc/qhuff_scan_impl.h) under ASan/UBSan, against
// the model's results (tests/headers_decode_model.py).  Stand-alone: built by
// tests/test_decode_headers.py with qhuff_frames.cpp and nothing else.
//
// usage: hdrscan_san FILE EXPECT [FILE EXPECT]...
// FILE: records of u32 LE length + payload, one section each.  EXPECT: u32 m,
// u32 n, rc[m] (i32), hdr_off[m + 1], the 2n descriptors, kind[n],
// static_id[n], hflags[n].  The payloads are packed back to back with no
// padding into a heap buffer of exactly their size (a read past a section's
// end that leaves the buffer is an ASan report; one that stays inside shows
// as a wrong result), the outputs in exactly-sized heap buffers, at max_hdrs =
// the total, the total - 1 and 0, with and without the optional arrays.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/qhuff.h"

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

static int
run(const char *file, const std::vector<uint8_t> &raw,
    const std::vector<uint8_t> &exp)
{
    std::vector<uint32_t> off(1, 0);
    size_t at = 0, bytes = 0;
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
    }
    const uint32_t m = (uint32_t) src.size();
    uint32_t em, total;
    if (exp.size() < 8)
        return die(file, "short expectation", 0);
    memcpy(&em, &exp[0], 4);
    memcpy(&total, &exp[4], 4);
    const size_t need = 8 + 4 * (size_t) m + 4 * ((size_t) m + 1)
                      + 35 * (size_t) total;
    if (em != m || exp.size() != need)
        return die(file, "expectation size", exp.size());
    const uint8_t *w_rc = &exp[8];
    const uint8_t *w_off = w_rc + 4 * (size_t) m;
    const uint8_t *w_strs = w_off + 4 * ((size_t) m + 1);
    const uint8_t *w_kind = w_strs + 32 * (size_t) total;
    const uint8_t *w_id = w_kind + total, *w_hf = w_id + total;

    uint8_t *buf = (uint8_t *) malloc(bytes ? bytes : 1);
    for (uint32_t i = 0; i < m; ++i)
        memcpy(buf + off[i], src[i], off[i + 1] - off[i]);
    uint32_t *sec_off = (uint32_t *) malloc(4 * ((size_t) m + 1));
    memcpy(sec_off, off.data(), 4 * ((size_t) m + 1));

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
            const int r = qhuff_scan_headers_cpu(buf, sec_off, m, strs, cap,
                                                 hdr_off, rc, kind, id, hf);
            if (r != (total > cap ? QHUFF_ERANGE : QHUFF_OK))
                return die(file, "return value", cap);
            if (memcmp(hdr_off, w_off, 4 * ((size_t) m + 1)))
                return die(file, "hdr_off", cap);
            if (m && memcmp(rc, w_rc, 4 * (size_t) m))
                return die(file, "rc", cap);
            if (cap && memcmp(strs, w_strs, 32 * (size_t) cap))
                return die(file, "descriptors", cap);
            if (opt && cap && (memcmp(kind, w_kind, cap) || memcmp(id, w_id, cap)
                               || memcmp(hf, w_hf, cap)))
                return die(file, "kind / static_id / hflags", cap);
            free(strs);
            free(hdr_off);
            free(rc);
            free(kind);
            free(id);
            free(hf);
        }
    free(buf);
    free(sec_off);
    printf("%s: %u sections, %u headers\n", file, m, total);
    return 0;
}

int
main(int argc, char **argv)
{
    if (argc < 3 || !(argc & 1))
    {
        fprintf(stderr, "usage: hdrscan_san FILE EXPECT [FILE EXPECT]...\n");
        return 2;
    }
    for (int k = 1; k + 1 < argc; k += 2)
    {
        std::vector<uint8_t> raw, exp;
        if (!slurp(argv[k], &raw) || !slurp(argv[k + 1], &exp))
            return 2;
        if (run(argv[k], raw, exp))
            return 1;
    }
    return 0;
}
