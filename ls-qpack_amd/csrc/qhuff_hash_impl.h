// qhuff_hash_impl.h -- XXH32 over a byte reader, and the readers.
//
// The same source runs in three places: as device code in the hash and the
// lookup kernels (qhuff_hash.hip, qhuff_lookup.hip) over a wave's LDS stage
// (HashLds) or global memory (HashGlb), as plain C++ on the host over the
// buffer itself (HashMem: qhuff_static_lookup_cpu, qhuff_frames.cpp, which
// also builds with g++ alone), and at compile time, where the static table's
// probe tables are made (qhuff_static.h).  qhuff_scan_impl.h is the precedent.
//
// A reader R sees bytes by index: byte(i), word(i) (4 bytes, little endian)
// and stripe(i, w) (16 bytes as 4 words).  The LDS and global-address-space
// readers exist where qhuff_device.h came first (it defines QH_LDS).
#pragma once
#include <stdint.h>

#ifndef QH_HD
#if defined(__HIPCC__) || defined(__HIP__)
#define QH_HD __host__ __device__
#else
#define QH_HD
#endif
#endif
#ifndef QH_HDI
#if defined(__HIPCC__) || defined(__HIP__)
#define QH_HDI __host__ __device__ inline __attribute__((always_inline))
#else
#define QH_HDI inline
#endif
#endif

namespace qhuff {

constexpr uint32_t kP1 = 2654435761u, kP2 = 2246822519u, kP3 = 3266489917u,
                   kP4 = 668265263u, kP5 = 374761393u;

QH_HDI constexpr uint32_t
rotl32(uint32_t x, uint32_t r)
{
#if defined(__HIP_DEVICE_COMPILE__)
    if (!__builtin_is_constant_evaluated())
        return __builtin_amdgcn_alignbit(x, x, 32 - r);
#endif
    return (x << r) | (x >> (32 - r));
}

QH_HDI constexpr uint32_t
xxh_round(uint32_t acc, uint32_t w)
{
    return rotl32(acc + w * kP2, 13) * kP1;
}

// bytes behind a byte pointer of type P (plain, or in the global address
// space): byte loads only, so nothing outside the string is touched
template <class P>
struct HashBytes
{
    P p;
    QH_HDI constexpr uint32_t byte(uint32_t i) const { return p[i]; }
    QH_HDI constexpr uint32_t word(uint32_t i) const
    {
        return p[i] | (p[i + 1] << 8) | (p[i + 2] << 16)
             | ((uint32_t) p[i + 3] << 24);
    }
    QH_HDI constexpr void stripe(uint32_t i, uint32_t w[4]) const
    {
        w[0] = word(i);
        w[1] = word(i + 4);
        w[2] = word(i + 8);
        w[3] = word(i + 12);
    }
};

// host memory (and constant evaluation)
using HashMem = HashBytes<const uint8_t *>;

#ifdef QH_LDS
// bytes staged in LDS; byte index i = global address - 16-aligned span base
struct HashLds
{
    const QH_LDS uint32_t *s;
    __device__ __forceinline__ uint32_t word(uint32_t i) const
    {
        const uint32_t q = i >> 2;
        return align_bytes(s[q + 1], s[q], i & 3);
    }
    __device__ __forceinline__ void stripe(uint32_t i, uint32_t w[4]) const
    {
        const uint32_t q = i >> 2, sh = i & 3;
        const uint32_t d0 = s[q], d1 = s[q + 1], d2 = s[q + 2], d3 = s[q + 3],
                       d4 = s[q + 4];
        w[0] = align_bytes(d1, d0, sh);
        w[1] = align_bytes(d2, d1, sh);
        w[2] = align_bytes(d3, d2, sh);
        w[3] = align_bytes(d4, d3, sh);
    }
    __device__ __forceinline__ uint32_t byte(uint32_t i) const
    {
        return ((const QH_LDS uint8_t *) s)[i];
    }
};

// bytes read straight from global (tiles too large for the stage)
using HashGlb = HashBytes<const QH_GLB uint8_t *>;
#endif

// XXH32 of bytes [a, a + len) (xxhash.c XXH32 / XXH32_endian_align):
// 16-byte stripes into four lanes, merge, + len, 4-byte then 1-byte tail,
// avalanche
template <class R>
QH_HDI constexpr uint32_t
xxh32(const R &r, uint32_t a, uint32_t len, uint32_t seed)
{
    uint32_t p = a;
    const uint32_t end = a + len;
    uint32_t h = 0;
    if (len >= 16)
    {
        uint32_t v1 = seed + kP1 + kP2, v2 = seed + kP2, v3 = seed,
                 v4 = seed - kP1;
        const uint32_t limit = end - 16;
        do
        {
            uint32_t w[4] = {0, 0, 0, 0};
            r.stripe(p, w);
            v1 = xxh_round(v1, w[0]);
            v2 = xxh_round(v2, w[1]);
            v3 = xxh_round(v3, w[2]);
            v4 = xxh_round(v4, w[3]);
            p += 16;
        } while (p <= limit);
        h = rotl32(v1, 1) + rotl32(v2, 7) + rotl32(v3, 12) + rotl32(v4, 18);
    }
    else
        h = seed + kP5;
    h += len;
    // (end - p, not p + 4: in global memory p is the input offset itself,
    // and p + 4 wraps for a string that ends within 4 bytes of 2^32)
    while (end - p >= 4)
    {
        h += r.word(p) * kP3;
        h = rotl32(h, 17) * kP4;
        p += 4;
    }
    while (p < end)
    {
        h += r.byte(p) * kP5;
        h = rotl32(h, 11) * kP1;
        ++p;
    }
    h ^= h >> 15;
    h *= kP2;
    h ^= h >> 13;
    h *= kP3;
    h ^= h >> 16;
    return h;
}

#ifdef QH_LDS
// ---- the tile frame of the hash and the lookup kernel ----------------------

constexpr int kHashWaves = 8;                      // waves per workgroup
constexpr int kHashNch = 6;                        // 16-byte chunks per lane
constexpr uint32_t kHashCap = 64 * kHashNch * 16;  // staged bytes per wave

struct HashWave
{
    alignas(16) uint32_t s[kHashCap / 4 + 8];      // + slack for stripe reads
};

// a tile's offsets: lane l holds header/string l's start, name end (pairs)
// and end; every lane loads (clamped index), so the count is fixed
struct HashOffs
{
    uint32_t a, m, b, cnt;

    __device__ __forceinline__ void load(const QH_GLB uint32_t *off,
                                         uint64_t t, uint64_t n, bool pairs)
    {
        const uint64_t s0 = t * kWT;
        cnt = (uint32_t) min((uint64_t) kWT, n - s0);
        const uint32_t k = pairs ? 2 : 1;
        const uint32_t li = lane_id() < cnt ? lane_id() : cnt - 1;
        const QH_GLB uint32_t *o = off + s0 * k + k * li;
        a = o[0];
        m = o[1];
        b = pairs ? o[2] : m;
    }
    __device__ __forceinline__ uint32_t first() const { return read_lane(a, 0); }
    __device__ __forceinline__ uint32_t last() const
    {
        return read_lane(b, cnt - 1);
    }
};
#endif

}  // namespace qhuff
