// lookup_san.cpp -- the lookup kernel's source on the CPU
// (qhuff_static_lookup_cpu: csrc/qhuff_hash_impl.h, qhuff_lookup_impl.h,
// qhuff_static.h) under ASan/UBSan.  Stand-alone: built by
// tests/test_static_lookup.py with qhuff_frames.cpp and nothing else.
//
// usage: lookup_san FILE
// FILE: u32 LE n, then n records of u32 name_len, u32 value_len, u8 kind,
// u8 static_id, u32 name_hash, u32 nameval_hash, name, value.  The names and
// values are packed back to back with no padding into a heap buffer of
// exactly their size (a read past a header's end that leaves the buffer is
// an ASan report; one that stays inside shows as a wrong result), the
// outputs in exactly-sized heap buffers; then once more without the hashes.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/qhuff.h"

static uint32_t
u32(const uint8_t *p)
{
    uint32_t v;
    memcpy(&v, p, 4);
    return v;
}

int
main(int argc, char **argv)
{
    if (argc != 2)
    {
        fprintf(stderr, "usage: lookup_san FILE\n");
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f)
    {
        perror(argv[1]);
        return 2;
    }
    std::vector<uint8_t> raw;
    uint8_t tmp[65536];
    size_t got;
    while ((got = fread(tmp, 1, sizeof(tmp), f)) > 0)
        raw.insert(raw.end(), tmp, tmp + got);
    fclose(f);
    if (raw.size() < 4)
        return 2;
    const uint32_t n = u32(raw.data());
    std::vector<uint32_t> offs(1, 0), w_h1, w_h2;
    std::vector<uint8_t> bytes, w_kind, w_id;
    size_t at = 4;
    for (uint32_t i = 0; i < n; ++i)
    {
        if (at + 18 > raw.size())
            return 2;
        const uint32_t nl = u32(&raw[at]), vl = u32(&raw[at + 4]);
        w_kind.push_back(raw[at + 8]);
        w_id.push_back(raw[at + 9]);
        w_h1.push_back(u32(&raw[at + 10]));
        w_h2.push_back(u32(&raw[at + 14]));
        at += 18;
        if ((size_t) nl + vl > raw.size() - at)
            return 2;
        bytes.insert(bytes.end(), raw.begin() + at, raw.begin() + at + nl + vl);
        at += (size_t) nl + vl;
        offs.push_back(offs.back() + nl);
        offs.push_back(offs.back() + vl);
    }
    uint8_t *in = (uint8_t *) malloc(bytes.size() ? bytes.size() : 1);
    memcpy(in, bytes.data(), bytes.size());
    uint32_t *off = (uint32_t *) malloc(4 * offs.size());
    memcpy(off, offs.data(), 4 * offs.size());
    for (int with_hashes = 1; with_hashes >= 0; --with_hashes)
    {
        uint32_t *h1 = (uint32_t *) malloc(n ? 4 * (size_t) n : 1);
        uint32_t *h2 = (uint32_t *) malloc(n ? 4 * (size_t) n : 1);
        uint8_t *kind = (uint8_t *) malloc(n ? n : 1);
        uint8_t *id = (uint8_t *) malloc(n ? n : 1);
        const int rc = qhuff_static_lookup_cpu(in, off, n,
                                               with_hashes ? h1 : NULL,
                                               with_hashes ? h2 : NULL, kind,
                                               id);
        if (rc != QHUFF_OK)
        {
            fprintf(stderr, "return value %d\n", rc);
            return 1;
        }
        for (uint32_t i = 0; i < n; ++i)
            if (kind[i] != w_kind[i] || id[i] != w_id[i]
                    || (with_hashes && (h1[i] != w_h1[i] || h2[i] != w_h2[i])))
            {
                fprintf(stderr, "header %u: kind %u id %u, expected %u %u\n",
                        i, kind[i], id[i], w_kind[i], w_id[i]);
                return 1;
            }
        free(h1);
        free(h2);
        free(kind);
        free(id);
    }
    uint8_t a[512], b[512];
    if (qhuff_static_probe_tables(a, b) != QHUFF_OK
            || qhuff_static_probe_tables(NULL, b) != QHUFF_EINVAL)
        return 1;
    free(in);
    free(off);
    printf("%u headers\n", n);
    return 0;
}
