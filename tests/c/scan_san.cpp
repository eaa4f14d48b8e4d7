// scan_san.cpp -- the device scan's walker on the CPU (qhuff_scan_sections_cpu,
// the kernels' source in csrc/qhuff_scan_impl.h) under ASan/UBSan, against
// the host scanners chunk by chunk.  Stand-alone: built by
// tests/test_scan_device.py with qhuff_frames.cpp and nothing else.
//
// usage: scan_san FILE...
// FILE: records of u32 LE length + payload.  Every file is run in both modes:
// its payloads packed back to back with no padding into a heap buffer of
// exactly their size (a read past a chunk's end that leaves the buffer is an
// ASan report; one that stays inside shows as a wrong result), the outputs in
// exactly-sized heap buffers, at max_lits = the total, the total - 1 and 0.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/qhuff.h"

static int
die(const char *file, unsigned mode, const char *what, size_t i)
{
    fprintf(stderr, "%s mode %u: %s at %zu\n", file, mode, what, i);
    return 1;
}

static int
run(const char *file, const std::vector<uint8_t> &raw, unsigned mode)
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
            return die(file, mode, "bad record", at);
        src.push_back(raw.data() + at);
        at += n;
        bytes += n;
        off.push_back((uint32_t) bytes);
    }
    const uint32_t m = (uint32_t) src.size();
    uint8_t *buf = (uint8_t *) malloc(bytes ? bytes : 1);
    for (uint32_t i = 0; i < m; ++i)
        memcpy(buf + off[i], src[i], off[i + 1] - off[i]);
    uint32_t *sec_off = (uint32_t *) malloc(4 * (m + 1));
    memcpy(sec_off, off.data(), 4 * (m + 1));

    // the host scanners, chunk by chunk, each on a copy of its own
    std::vector<qhuff_literal> want;
    std::vector<uint32_t> w_off(1, 0), w_used(m, 0);
    std::vector<int32_t> w_rc(m, 0);
    for (uint32_t i = 0; i < m; ++i)
    {
        const size_t len = off[i + 1] - off[i];
        uint8_t *c = (uint8_t *) malloc(len ? len : 1);
        memcpy(c, buf + off[i], len);
        std::vector<qhuff_literal> l(len + 1);
        uint32_t n = 0;
        size_t used = 0;
        int rc;
        if (mode == QHUFF_SCAN_FIELD_SECTION)
        {
            rc = qhuff_scan_field_section(c, len, off[i], l.data(),
                                          (uint32_t) l.size(), &n);
            used = rc == QHUFF_OK ? len : 0;
        }
        else
            rc = qhuff_scan_encoder_stream(c, len, off[i], l.data(),
                                           (uint32_t) l.size(), &n, &used);
        free(c);
        if (rc != QHUFF_OK)
            n = 0, used = 0;
        w_rc[i] = rc;
        w_used[i] = (uint32_t) used;
        want.insert(want.end(), l.begin(), l.begin() + n);
        w_off.push_back((uint32_t) want.size());
    }
    const uint32_t total = (uint32_t) want.size();

    const uint32_t caps[3] = {total, total ? total - 1 : 0, 0};
    for (uint32_t cap : caps)
    {
        qhuff_literal *lits = (qhuff_literal *) malloc(cap ? 16 * (size_t) cap : 1);
        uint32_t *lit_off = (uint32_t *) malloc(4 * (m + 1));
        int32_t *rc = (int32_t *) malloc(m ? 4 * m : 1);
        uint32_t *used = (uint32_t *) malloc(m ? 4 * m : 1);
        const int r = qhuff_scan_sections_cpu(buf, sec_off, m, mode, lits, cap,
                                              lit_off, rc, used);
        if (r != (total > cap ? QHUFF_ERANGE : QHUFF_OK))
            return die(file, mode, "return value", cap);
        if (memcmp(lit_off, w_off.data(), 4 * (m + 1)))
            return die(file, mode, "lit_off", cap);
        for (uint32_t i = 0; i < m; ++i)
            if (rc[i] != w_rc[i] || used[i] != w_used[i])
                return die(file, mode, "rc / consumed", i);
        if (cap && memcmp(lits, want.data(), 16 * (size_t) cap))
            return die(file, mode, "descriptors", cap);
        free(lits);
        free(lit_off);
        free(rc);
        free(used);
    }
    free(buf);
    free(sec_off);
    printf("%s mode %u: %u chunks, %u literals\n", file, mode, m, total);
    return 0;
}

int
main(int argc, char **argv)
{
    if (argc < 2)
    {
        fprintf(stderr, "usage: scan_san FILE...\n");
        return 2;
    }
    for (int k = 1; k < argc; ++k)
    {
        FILE *f = fopen(argv[k], "rb");
        if (!f)
        {
            perror(argv[k]);
            return 2;
        }
        std::vector<uint8_t> raw;
        uint8_t tmp[65536];
        size_t n;
        while ((n = fread(tmp, 1, sizeof(tmp), f)) > 0)
            raw.insert(raw.end(), tmp, tmp + n);
        fclose(f);
        if (run(argv[k], raw, QHUFF_SCAN_FIELD_SECTION)
                || run(argv[k], raw, QHUFF_SCAN_ENCODER_STREAM))
            return 1;
    }
    return 0;
}
