// qhuff_multi.cpp -- the *_multi calls of the C-ABI and qhuff_shard_cuts.
#include "qhuff_ctx.h"

// ---- one batch over several contexts ---------------
//
// The path shards trivially -- a string's output depends on its own bytes
// and the static table only (lsqpack.c:5085-5195, 5234-5466) -- so a batch
// is cut by input bytes (qhuff_shard_cuts) into one contiguous shard per
// context, every shard runs on its own host thread (the caller's thread
// takes shard 0), and the outputs are stitched by adding each shard's base
// (the exclusive scan of the shard totals) to its offsets.  No collective:
// the only cross-shard dependency is that base.

// contexts distinct and non-null
static bool
ctxs_ok(qhuff_ctx *const *ctxs, uint32_t g)
{
    if (!ctxs || g == 0 || g > 1024)
        return false;
    for (uint32_t k = 0; k < g; ++k)
    {
        if (!ctxs[k])
            return false;
        for (uint32_t j = 0; j < k; ++j)
            if (ctxs[j] == ctxs[k])
                return false;
    }
    return true;
}

// run f(k) for k in [0, g): threads for k >= 1, the caller for k = 0;
// the first failing return code (in shard order), or QHUFF_OK
// (A shard whose thread cannot be created runs on the caller's thread after
// shard 0, in shard order: a shard only ever waits for earlier ones.)
template <class F>
static int
run_shards(uint32_t g, F f)
{
    std::vector<int> rc(g, QHUFF_OK);
    std::vector<std::thread> th;
    std::vector<uint32_t> inline_k;
    th.reserve(g ? g - 1 : 0);
    for (uint32_t k = 1; k < g; ++k)
    {
        try
        {
            th.emplace_back([&rc, &f, k] { rc[k] = f(k); });
        }
        catch (...)
        {
            inline_k.push_back(k);
        }
    }
    rc[0] = f(0);
    for (uint32_t k : inline_k)
        rc[k] = f(k);
    for (auto &t : th)
        t.join();
    for (uint32_t k = 0; k < g; ++k)
        if (rc[k])
            return rc[k];
    return QHUFF_OK;
}

static int
host_multi(qhuff_ctx *const *ctxs, uint32_t g, bool enc, const uint8_t *in,
           const uint32_t *in_off, uint32_t n, unsigned mode, uint8_t *out,
           uint32_t *out_off, uint8_t *status)
{
    if (!ctxs_ok(ctxs, g) || !in_off || !out_off || (n && (!in || !out))
            || (!enc && n && !status))
        return QHUFF_EINVAL;
    if (enc && !mode_ok(mode))
        return QHUFF_EINVAL;
    const uint64_t bytes = (uint64_t) in_off[n] - in_off[0];
    if (bound_of(enc, bytes, n, mode) > 0xffffffffull)
        return QHUFF_ERANGE;
    std::vector<uint32_t> cuts(g + 1);
    int rc = qhuff_shard_cuts(in_off, n, g, cuts.data());
    if (rc)
        return rc;
    ShardSync sync(g);
    // direct DMA into `out` only if the whole call's bound is registered:
    // shard k's bytes land at out + base[k], anywhere inside it
    const bool out_reg = host_registered(out, bound_of(enc, bytes, n, mode));
    return run_shards(g, [&](uint32_t k) -> int {
        const uint32_t s0 = cuts[k], m = cuts[k + 1] - s0;
        const int r = host_batch(ctxs[k], enc, in, in_off + s0, m, mode, out,
                                 out_off + s0, status ? status + s0 : nullptr,
                                 &sync, k, k + 1 == g, out_reg);
        if (r)
            sync.fail();
        return r;
    });
}

extern "C" int
qhuff_encode_batch_host_multi(qhuff_ctx *const *ctxs, uint32_t g,
                              const uint8_t *in, const uint32_t *in_off,
                              uint32_t n, unsigned mode, uint8_t *out,
                              uint32_t *out_off)
{
    return host_multi(ctxs, g, true, in, in_off, n, mode, out, out_off,
                      nullptr);
}

extern "C" int
qhuff_decode_batch_host_multi(qhuff_ctx *const *ctxs, uint32_t g,
                              const uint8_t *in, const uint32_t *in_off,
                              uint32_t n, uint8_t *out, uint32_t *out_off,
                              uint8_t *status)
{
    return host_multi(ctxs, g, false, in, in_off, n, 0, out, out_off, status);
}

// Device-resident shards: shard k is already on ctxs[k]'s device.  Each
// thread launches its shard and reads its total; the bases are the
// exclusive scan; with rebase, a small kernel adds shard k's base to its
// out_off on its own device (out_off then holds offsets into the
// concatenation of the shards' outputs).  Synchronous.
static int
dev_multi(qhuff_ctx *const *ctxs, uint32_t g, bool enc,
          const struct qhuff_shard *sh, unsigned mode, uint64_t *base,
          int rebase)
{
    if (!ctxs_ok(ctxs, g) || !sh || !base)
        return QHUFF_EINVAL;
    ShardSync sync(g);
    std::vector<uint64_t> bases(g + 1, 0);
    const int rc = run_shards(g, [&](uint32_t k) -> int {
        qhuff_ctx *c = ctxs[k];
        const qhuff_shard &s = sh[k];
        hipStream_t st = (hipStream_t) s.stream;
        int r = enc ? qhuff_encode_batch(c, s.in, s.in_off, s.n, mode, s.out,
                                         s.out_off, s.stream)
                    : qhuff_decode_batch(c, s.in, s.in_off, s.n, s.out,
                                         s.out_off, s.status, s.stream);
        uint32_t t = 0;
        if (!r)
        {
            hipError_t e = hipMemcpyAsync(&t, s.out_off + s.n, 4,
                                          hipMemcpyDeviceToHost, st);
            if (e == hipSuccess)
                e = hipStreamSynchronize(st);
            if (e != hipSuccess)
                r = fail(c, e, "shard total");
        }
        if (!r && c->err_host[0])
            r = mirror_error(c);
        if (r)
        {
            sync.fail();
            return r;
        }
        sync.publish(k, t);
        const uint64_t b = sync.base_of(k);
        if (b == ~0ull)
            return QHUFF_EDEVICE;
        bases[k] = b;
        if (b + t > 0xffffffffull)
            return QHUFF_ERANGE;
        if (rebase && b)
        {
            HIPCHK(c, hipSetDevice(c->device));
            HIPCHK(c, launch_rebase(s.out_off, (uint64_t) s.n + 1,
                                    (uint32_t) b, st));
            HIPCHK(c, hipStreamSynchronize(st));
        }
        if (k + 1 == g)
            bases[g] = b + t;
        return QHUFF_OK;
    });
    if (rc)
        return rc;
    memcpy(base, bases.data(), 8ull * (g + 1));
    return QHUFF_OK;
}

extern "C" int
qhuff_encode_batch_multi(qhuff_ctx *const *ctxs, uint32_t g,
                         const struct qhuff_shard *shards, unsigned mode,
                         uint64_t *base, int rebase)
{
    if (!mode_ok(mode))
        return QHUFF_EINVAL;
    return dev_multi(ctxs, g, true, shards, mode, base, rebase);
}

extern "C" int
qhuff_decode_batch_multi(qhuff_ctx *const *ctxs, uint32_t g,
                         const struct qhuff_shard *shards, uint64_t *base,
                         int rebase)
{
    return dev_multi(ctxs, g, false, shards, 0, base, rebase);
}

extern "C" int
qhuff_shard_cuts(const uint32_t *in_off, uint32_t n, uint32_t g,
                 uint32_t *cuts)
{
    if (!in_off || !cuts || g == 0)
        return QHUFF_EINVAL;
    const uint64_t a = in_off[0], tot = (uint64_t) in_off[n] - a;
    cuts[0] = 0;
    uint32_t i = 0;
    for (uint32_t k = 1; k < g; ++k)
    {
        uint64_t target = a + tot * k / g;
        // first string index whose start offset reaches the target
        uint32_t lo = i, hi = n;
        while (lo < hi)
        {
            uint32_t mid = lo + (hi - lo) / 2;
            if (in_off[mid] < target)
                lo = mid + 1;
            else
                hi = mid;
        }
        i = lo;
        cuts[k] = i;
    }
    cuts[g] = n;
    return QHUFF_OK;
}
