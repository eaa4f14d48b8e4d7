// qhuff_static.h -- the QPACK static table (RFC 9204 Appendix A; the
// reference's static_table[], lsqpack.c:104-209 -- the list in
// tests/golden/qpack_static_table.json) and the two probe tables of the
// reference's static lookup (find_in_static_full and
// lsqpack_find_in_static_headers, lsqpack.c:721-764).
//
// Plain C++, all of it made at compile time: the entries' bytes as
// little-endian words, every entry from a word of its own (a name directly
// followed by its value, so that a full match is one run of bytes, compared
// four at a time), their lengths, and the probe tables, which the library
// builds from these entries with its own XXH32 (qhuff_hash_impl.h) -- slot
// hash & 511 holds id + 1, entries inserted in ascending id, the first to
// claim a slot keeps it -- instead of copying the reference's arrays
// (lsqpack.c:629-666; tests/test_static_lookup.py compares).  The lookup
// kernel's code object holds a copy (qhuff_lookup.hip kStaticDev), the host
// another (qhuff_frames.cpp).
#pragma once

#include <stdint.h>

#include "qhuff_hash_impl.h"
#include "qhuff_names.h"

// X(name, value), id 0 .. 98
#define QHUFF_STATIC_TABLE(X) \
    X(":authority", "") \
    X(":path", "/") \
    X("age", "0") \
    X("content-disposition", "") \
    X("content-length", "0") \
    X("cookie", "") \
    X("date", "") \
    X("etag", "") \
    X("if-modified-since", "") \
    X("if-none-match", "") \
    X("last-modified", "") \
    X("link", "") \
    X("location", "") \
    X("referer", "") \
    X("set-cookie", "") \
    X(":method", "CONNECT") \
    X(":method", "DELETE") \
    X(":method", "GET") \
    X(":method", "HEAD") \
    X(":method", "OPTIONS") \
    X(":method", "POST") \
    X(":method", "PUT") \
    X(":scheme", "http") \
    X(":scheme", "https") \
    X(":status", "103") \
    X(":status", "200") \
    X(":status", "304") \
    X(":status", "404") \
    X(":status", "503") \
    X("accept", "*/*") \
    X("accept", "application/dns-message") \
    X("accept-encoding", "gzip, deflate, br") \
    X("accept-ranges", "bytes") \
    X("access-control-allow-headers", "cache-control") \
    X("access-control-allow-headers", "content-type") \
    X("access-control-allow-origin", "*") \
    X("cache-control", "max-age=0") \
    X("cache-control", "max-age=2592000") \
    X("cache-control", "max-age=604800") \
    X("cache-control", "no-cache") \
    X("cache-control", "no-store") \
    X("cache-control", "public, max-age=31536000") \
    X("content-encoding", "br") \
    X("content-encoding", "gzip") \
    X("content-type", "application/dns-message") \
    X("content-type", "application/javascript") \
    X("content-type", "application/json") \
    X("content-type", "application/x-www-form-urlencoded") \
    X("content-type", "image/gif") \
    X("content-type", "image/jpeg") \
    X("content-type", "image/png") \
    X("content-type", "text/css") \
    X("content-type", "text/html; charset=utf-8") \
    X("content-type", "text/plain") \
    X("content-type", "text/plain;charset=utf-8") \
    X("range", "bytes=0-") \
    X("strict-transport-security", "max-age=31536000") \
    X("strict-transport-security", "max-age=31536000; includesubdomains") \
    X("strict-transport-security", "max-age=31536000; includesubdomains; preload") \
    X("vary", "accept-encoding") \
    X("vary", "origin") \
    X("x-content-type-options", "nosniff") \
    X("x-xss-protection", "1; mode=block") \
    X(":status", "100") \
    X(":status", "204") \
    X(":status", "206") \
    X(":status", "302") \
    X(":status", "400") \
    X(":status", "403") \
    X(":status", "421") \
    X(":status", "425") \
    X(":status", "500") \
    X("accept-language", "") \
    X("access-control-allow-credentials", "FALSE") \
    X("access-control-allow-credentials", "TRUE") \
    X("access-control-allow-headers", "*") \
    X("access-control-allow-methods", "get") \
    X("access-control-allow-methods", "get, post, options") \
    X("access-control-allow-methods", "options") \
    X("access-control-expose-headers", "content-length") \
    X("access-control-request-headers", "content-type") \
    X("access-control-request-method", "get") \
    X("access-control-request-method", "post") \
    X("alt-svc", "clear") \
    X("authorization", "") \
    X("content-security-policy", "script-src 'none'; object-src 'none'; base-uri 'none'") \
    X("early-data", "1") \
    X("expect-ct", "") \
    X("forwarded", "") \
    X("if-range", "") \
    X("origin", "") \
    X("purpose", "prefetch") \
    X("server", "") \
    X("timing-allow-origin", "*") \
    X("upgrade-insecure-requests", "1") \
    X("user-agent", "") \
    X("x-forwarded-for", "") \
    X("x-frame-options", "deny") \
    X("x-frame-options", "sameorigin")

namespace qhuff {

constexpr uint32_t kStaticSlots = 512;       // XXH_NAME_WIDTH = XXH_NAMEVAL_WIDTH = 9
constexpr uint32_t kXxhSeed = 39378473u;     // LSQPACK_XXH_SEED, lsqpack.c:623

#define QH_STATIC_BYTES(n, v) n v
#define QH_STATIC_LENS(n, v) {sizeof(n) - 1, sizeof(v) - 1},
constexpr char kStaticText[] = QHUFF_STATIC_TABLE(QH_STATIC_BYTES);
constexpr uint8_t kStaticLens[][2] = {QHUFF_STATIC_TABLE(QH_STATIC_LENS)};
#undef QH_STATIC_BYTES
#undef QH_STATIC_LENS
constexpr uint32_t kStaticBytes = sizeof(kStaticText) - 1;
static_assert(sizeof(kStaticLens) / 2 == kStaticNames, "99 entries");

constexpr uint32_t
static_words()
{
    uint32_t w = 0;
    for (uint32_t i = 0; i < kStaticNames; ++i)
        w += (kStaticLens[i][0] + kStaticLens[i][1] + 3u) / 4;
    return w;
}
constexpr uint32_t kStaticWords = static_words();

struct StaticTable
{
    uint32_t words[kStaticWords];            // entry i: name from word at[i],
    uint16_t at[kStaticNames];               // then its value
    constexpr uint32_t byte(uint32_t w, uint32_t i) const
    {
        return words[w + i / 4] >> 8 * (i % 4) & 0xff;
    }
    uint8_t name_len[kStaticNames], val_len[kStaticNames];
    uint8_t name2id[kStaticSlots];           // id + 1, or 0
    uint8_t nameval2id[kStaticSlots];
};

constexpr StaticTable
make_static_table()
{
    StaticTable t{};
    uint8_t bytes[kStaticBytes] = {};
    for (uint32_t i = 0; i < kStaticBytes; ++i)
        bytes[i] = (uint8_t) kStaticText[i];
    const HashMem r{bytes};
    uint32_t at = 0, w = 0;
    for (uint32_t i = 0; i < kStaticNames; ++i)
    {
        const uint32_t nl = kStaticLens[i][0], vl = kStaticLens[i][1];
        t.at[i] = (uint16_t) w;
        t.name_len[i] = (uint8_t) nl;
        t.val_len[i] = (uint8_t) vl;
        for (uint32_t k = 0; k < nl + vl; ++k)
            t.words[w + k / 4] |= (uint32_t) bytes[at + k] << 8 * (k % 4);
        const uint32_t h1 = xxh32(r, at, nl, kXxhSeed);
        const uint32_t h2 = xxh32(r, at + nl, vl, h1);
        at += nl + vl;
        w += (nl + vl + 3) / 4;
        if (!t.name2id[h1 % kStaticSlots])
            t.name2id[h1 % kStaticSlots] = (uint8_t) (i + 1);
        if (!t.nameval2id[h2 % kStaticSlots])
            t.nameval2id[h2 % kStaticSlots] = (uint8_t) (i + 1);
    }
    return t;
}

constexpr bool
static_names_agree()
{
    uint32_t total = 0;
    for (uint32_t i = 0; i < kStaticNames; ++i)
    {
        if (kStaticLens[i][0] != kStaticNameLen[i])
            return false;
        total += kStaticLens[i][0] + kStaticLens[i][1];
    }
    return total == kStaticBytes;
}
static_assert(static_names_agree(), "qhuff_names.h holds this table's name lengths");

}  // namespace qhuff
