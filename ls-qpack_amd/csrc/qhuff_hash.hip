// qhuff_hash.hip -- batched XXH32 of header names and values (gfx950).
//
// Reference: every header the encoder takes
// and every header the decoder emits is hashed twice with XXH32
// (deps/xxhash/xxhash.c, 32-bit variant):
//
//   name_hash    = XXH32(name,  name_len,  LSQPACK_XXH_SEED)  lsqpack.c:1681,
//                                                             3268-3269
//   nameval_hash = XXH32(value, value_len, name_hash)         lsqpack.c:1685,
//                                                             3308-3309
//
// (LSQPACK_XXH_SEED = 39378473, lsqpack.c:623).  The hashes index the static
// table (name2id_plus_one / nameval2id_plus_one, lsqpack.c:629-753) and the
// dynamic table.  Like the Huffman kernels this is per-string byte work:
// one header per lane, one 64-header tile per wave, the tile's contiguous
// name/value bytes staged into the wave's LDS region with coalesced 16-byte
// loads, then each lane walks its own bytes out of LDS (four 32-bit
// accumulators over 16-byte stripes, then 4-byte and 1-byte tails).  The
// outputs are fixed-size (two u32 per header), so no scan or look-back is
// needed; waves are persistent (grid = what is resident) and prefetch the
// next tile's bytes while hashing the current one.  HBM-bound: a header
// costs its name + value bytes + 8 B of offsets + 8 B of hashes.
// XXH32 itself and the byte readers (HashLds, HashGlb) are in
// qhuff_hash_impl.h, shared with qhuff_lookup.hip and the host.
#include "qhuff_kernels.h"
#include "qhuff_hash_impl.h"

namespace qhuff {

template <class R>
__device__ __forceinline__ void
hash_lane(const R &r, bool pairs, uint32_t a, uint32_t m, uint32_t b,
          uint32_t seed, uint32_t *h1, uint32_t *h2)
{
    if (pairs)
    {
        *h1 = xxh32(r, a, m - a, seed);
        *h2 = xxh32(r, m, b - m, *h1);
    }
    else
        *h1 = xxh32(r, a, b - a, seed);
}

// Persistent waves, software-pipelined like the codec kernels: while tile t
// is hashed out of LDS, the bytes of tile t + W and the offsets of tile
// t + 2W are already in flight (W = waves in the grid).
__global__ __launch_bounds__(64 * kHashWaves) void
qhuff_hash_kernel(HashArgs a)
{
    __shared__ HashWave sm[kHashWaves];
    const uint32_t lane = lane_id();
    const uint32_t wv = threadIdx.x >> 6;
    const uint64_t nt = (a.n + kWT - 1) / kWT;
    const uint64_t W = (uint64_t) gridDim.x * kHashWaves;
    uint64_t t = (uint64_t) blockIdx.x * kHashWaves + wv;
    if (t >= nt)
        return;
    const bool pairs = a.pairs != 0;
    const QH_GLB uint32_t *off = glb(a.off);
    auto clamp = [&](uint64_t x) { return x < nt ? x : nt - 1; };
    QH_LDS uint32_t *s = (QH_LDS uint32_t *) sm[wv].s;

    HashOffs o_cur, o_nxt, o_nn;
    o_cur.load(off, t, a.n, pairs);
    Span sp_cur = tile_span(a.in, o_cur.first(), o_cur.last(), kHashCap);
    Chunks<kHashNch> ch;
    ch.load(sp_cur);
    o_nxt.load(off, clamp(t + W), a.n, pairs);
    for (;;)
    {
        __builtin_amdgcn_s_waitcnt(0x0f70);           // vmcnt(0)
        if (sp_cur.staged)
            ch.store<false>((QH_LDS u32x4 *) s, sp_cur.n16);
        wave_sync();
        const Span sp_nxt = tile_span(a.in, o_nxt.first(), o_nxt.last(),
                                      kHashCap);
        if (t + W < nt)
            ch.load(sp_nxt);
        o_nn.load(off, clamp(t + 2 * W), a.n, pairs);

        uint32_t h1 = 0, h2 = 0;
        const uint32_t first = o_cur.first();
        if (sp_cur.staged)
        {
            // byte index of input offset x in the stage: x - first + skew
            const uint32_t skew = (uint32_t) ((uintptr_t) (a.in + first)
                                              - sp_cur.pa);
            const HashLds r{s};
            hash_lane(r, pairs, o_cur.a - first + skew, o_cur.m - first + skew,
                      o_cur.b - first + skew, a.seed, &h1, &h2);
        }
        else
        {
            const HashGlb r{glb(a.in)};
            hash_lane(r, pairs, o_cur.a, o_cur.m, o_cur.b, a.seed, &h1, &h2);
        }
        const uint64_t s0 = t * kWT;
        if (lane < o_cur.cnt)
        {
            glb(a.h1)[s0 + lane] = h1;
            if (pairs)
                glb(a.h2)[s0 + lane] = h2;
        }
        wave_sync();
        t += W;
        if (t >= nt)
            break;
        o_cur = o_nxt;
        o_nxt = o_nn;
        sp_cur = sp_nxt;
    }
}

hipError_t
launch_hash(const HashArgs &a, uint32_t max_grid, hipStream_t st,
            hipEvent_t ev0, hipEvent_t ev1)
{
    const uint64_t tiles = (a.n + kWT - 1) / kWT;
    const uint64_t need = (tiles + kHashWaves - 1) / kHashWaves;
    const uint32_t grid = (uint32_t) (need < max_grid ? need : max_grid);
    return launch_kernel(qhuff_hash_kernel, grid, 64 * kHashWaves, st, ev0,
                         ev1, a);
}

// Shard stitching (qhuff_*_batch_multi): off[i] += add for i in [0, n],
// four offsets per lane with 16-byte accesses where the array allows
// (a grid-stride loop: every wave exits when its range is done).
__global__ __launch_bounds__(256) void
qhuff_rebase_kernel(uint32_t *off, uint64_t n, uint32_t add)
{
    const uint64_t stride = (uint64_t) gridDim.x * blockDim.x;
    const uint64_t head = (4 - (((uintptr_t) off >> 2) & 3)) & 3;   // to 16 B
    const uint64_t h = head < n ? head : n;
    const uint64_t t = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (t < h)
        off[t] += add;
    U4 *v = (U4 *) (off + h);
    const uint64_t nv = (n - h) / 4;
    for (uint64_t i = t; i < nv; i += stride)
    {
        u32x4 x = v[i].v;
        x.x += add;
        x.y += add;
        x.z += add;
        x.w += add;
        v[i].v = x;
    }
    for (uint64_t i = h + 4 * nv + t; i < n; i += stride)
        off[i] += add;
}

hipError_t
launch_rebase(uint32_t *off, uint64_t n, uint32_t add, hipStream_t st)
{
    if (n == 0 || add == 0)
        return hipSuccess;
    const uint64_t need = (n / 4 + 255) / 256 + 1;
    const uint32_t grid = (uint32_t) (need < 2048 ? need : 2048);
    hipLaunchKernelGGL(qhuff_rebase_kernel, dim3(grid), dim3(256), 0, st, off,
                       n, add);
    return hipGetLastError();
}

int
hash_waves_per_block()
{
    return kHashWaves;
}

hipError_t
hash_occupancy(int *blocks_per_cu)
{
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(
        blocks_per_cu, reinterpret_cast<const void *>(qhuff_hash_kernel),
        64 * kHashWaves, 0);
}

}  // namespace qhuff
