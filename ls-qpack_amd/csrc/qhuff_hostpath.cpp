// qhuff_hostpath.cpp -- the pinned host-memory path of the C-ABI, buffer
// registration and the per-string mirrors of the reference entry points.
#include "qhuff_ctx.h"
#include "qhuff_tabs_insert_impl.h"
#include "qhuff_scan_impl.h"
#include "qhuff_lookup_dyn_impl.h"
#include "qhuff_tabs_impl.h"

namespace qhuff {
// qhuff_frames.cpp: a VALUE literal's static-table name length, or 0
uint32_t field_ref_name_len(const uint8_t *buf, const struct qhuff_literal &l);
}

// Host copy workers for the PCIe-inclusive path: a staging memcpy of tens
// of MB runs at one core's copy rate, so the pinned staging copies (and the
// out_off rebasing) are split into slices run by a few persistent threads.
struct CopyPool
{
    std::vector<std::thread> th;
    std::mutex mu;
    std::condition_variable go, done;
    std::function<void(unsigned)> job;
    unsigned slices = 0;
    std::atomic<unsigned> next{0};
    unsigned finished = 0;
    unsigned active = 0;                 // workers inside a claim loop
    uint64_t gen = 0;
    bool stop = false;

    explicit CopyPool(unsigned n)
    {
        for (unsigned i = 0; i < n; ++i)
            th.emplace_back([this] { worker(); });
    }
    ~CopyPool()
    {
        {
            std::lock_guard<std::mutex> g(mu);
            stop = true;
        }
        go.notify_all();
        for (auto &t : th)
            t.join();
    }
    void worker()
    {
        uint64_t seen = 0;
        for (;;)
        {
            std::unique_lock<std::mutex> lk(mu);
            go.wait(lk, [&] { return stop || gen != seen; });
            if (stop)
                return;
            seen = gen;
            ++active;
            const unsigned ns = slices;
            lk.unlock();
            unsigned k;
            while ((k = next.fetch_add(1)) < ns)
            {
                job(k);
                std::lock_guard<std::mutex> g(mu);
                ++finished;
            }
            std::lock_guard<std::mutex> g(mu);
            --active;
            done.notify_all();
        }
    }
    // run fn(0 .. n-1) on the workers and the calling thread; returns when
    // every slice is done
    void run(unsigned n, std::function<void(unsigned)> fn)
    {
        if (n == 0)
            return;
        if (th.empty() || n == 1)
        {
            for (unsigned k = 0; k < n; ++k)
                fn(k);
            return;
        }
        {
            std::lock_guard<std::mutex> g(mu);
            job = std::move(fn);
            slices = n;
            finished = 0;
            next.store(0);
            ++gen;
        }
        go.notify_all();
        unsigned k;
        while ((k = next.fetch_add(1)) < n)
        {
            job(k);
            std::lock_guard<std::mutex> g(mu);
            ++finished;
        }
        // every slice done AND no worker still inside its claim loop: a
        // straggler's late fetch_add can then not race the next run()'s
        // reset of job / slices / next (it reads `ns`, its own copy)
        std::unique_lock<std::mutex> lk(mu);
        done.wait(lk, [&] { return finished == n && active == 0; });
    }
    // memcpy split into ~1 MB slices
    void copy(void *dst, const void *src, size_t n)
    {
        const size_t sl = 1u << 20;
        const unsigned k = (unsigned) ((n + sl - 1) / sl);
        run(k, [=](unsigned i) {
            const size_t a = (size_t) i * sl, b = a + sl < n ? a + sl : n;
            memcpy((uint8_t *) dst + a, (const uint8_t *) src + a, b - a);
        });
    }
};

// ---- host-memory path ------------------------------------------------------

static int
ensure_stage(qhuff_ctx *c, size_t bytes)
{
    if (bytes > c->h_stage_cap)
    {
        if (c->h_stage)
            (void) hipHostFree(c->h_stage);
        c->h_stage = nullptr;
        c->h_stage_cap = 0;
        HIPCHK(c, hipHostMalloc((void **) &c->h_stage, bytes));
        c->h_stage_cap = bytes;
    }
    if (bytes > c->d_stage_cap)
    {
        if (c->d_stage)
            (void) hipFree(c->d_stage);
        c->d_stage = nullptr;
        c->d_stage_cap = 0;
        HIPCHK(c, hipMalloc((void **) &c->d_stage, bytes));
        c->d_stage_cap = bytes;
    }
    return QHUFF_OK;
}

static inline size_t
up16(size_t x)
{
    return (x + 15) & ~(size_t) 15;
}

static int
pipe_setup(qhuff_ctx *c)
{
    if (c->pipe_ready)
        return QHUFF_OK;
    HIPCHK(c, hipStreamCreateWithFlags(&c->h2d_stream, hipStreamNonBlocking));
    HIPCHK(c, hipStreamCreateWithFlags(&c->d2h_stream, hipStreamNonBlocking));
    for (unsigned i = 0; i < kMaxChunks; ++i)
    {
        HIPCHK(c, hipEventCreateWithFlags(&c->ev_in[i], hipEventDisableTiming));
        HIPCHK(c, hipEventCreateWithFlags(&c->ev_k[i], hipEventDisableTiming));
        HIPCHK(c, hipEventCreateWithFlags(&c->ev_out[i], hipEventDisableTiming));
    }
    unsigned t = 8;
    if (const char *e = getenv("QHUFF_HOST_THREADS"))
        t = (unsigned) strtoul(e, nullptr, 0);
    if (t > 64)
        t = 64;
    c->pool = new CopyPool(t > 1 ? t - 1 : 0);   // + the calling thread
    c->pipe_ready = true;
    return QHUFF_OK;
}

// what pipe_setup made (qhuff_close)
void
qhuff::pipe_teardown(qhuff_ctx *c)
{
    if (c->pipe_ready)
    {
        (void) hipStreamDestroy(c->h2d_stream);
        (void) hipStreamDestroy(c->d2h_stream);
        for (unsigned i = 0; i < kMaxChunks; ++i)
        {
            (void) hipEventDestroy(c->ev_in[i]);
            (void) hipEventDestroy(c->ev_k[i]);
            (void) hipEventDestroy(c->ev_out[i]);
        }
    }
    delete c->pool;
}

// The variant the kernels' own rules call for on a batch whose offsets the
// host holds (the host-memory paths): the full kernel when a string is
// longer than kHintLen bytes (decode: the cooperative threshold, kCoopMin
// Huffman bytes; encode: a payload the full emit copies with the whole
// wave, at ~8 bits a byte) or a 64-string tile spans more than the 3 KB
// stage can take (a big tile).  One pass over the offsets on the copy
// workers.  VERDICT r04 item 2: the device-pointer calls can only go by
// history; these need not.
constexpr uint32_t kHintLen = 128;
constexpr uint32_t kHintSpan = 3072 - 32;
// strings [a, b) of one tile
static inline bool
tile_rare(const uint32_t *off, uint32_t a, uint32_t b)
{
    bool r = off[b] - off[a] > kHintSpan;
    for (uint32_t i = a; i < b; ++i)
        r |= off[i + 1] - off[i] > kHintLen;
    return r;
}

static bool
host_rare(qhuff_ctx *c, const uint32_t *off, uint32_t n)
{
    std::atomic<bool> rare{false};
    const uint32_t tiles = (n + 63) / 64, per = 1024;   // tiles per slice
    c->pool->run((tiles + per - 1) / per, [&](unsigned k) {
        const uint32_t t0 = k * per, t1 = t0 + per < tiles ? t0 + per : tiles;
        bool r = false;
        for (uint32_t t = t0; t < t1 && !r; ++t)
        {
            const uint32_t a = 64 * t, b = a + 64 < n ? a + 64 : n;
            r = tile_rare(off, a, b);
        }
        if (r)
            rare.store(true, std::memory_order_relaxed);
    });
    return rare.load();
}

static void
host_hint(qhuff_ctx *c, bool enc, const uint32_t *off, uint32_t n)
{
    if (c->kernels == 0)
        c->hint[enc ? 0 : 1] = host_rare(c, off, n) ? 1 : 0;
}

extern "C" int
qhuff_batch_needs_full(const uint32_t *off, uint32_t n)
{
    if (!off)
        return QHUFF_EINVAL;
    for (uint32_t a = 0; a < n; a += 64)
    {
        if (tile_rare(off, a, a + 64 < n ? a + 64 : n))
            return 1;
    }
    return 0;
}

// ---- caller buffers registered for direct DMA (qhuff_host_register) -------
//
// The host path stages the caller's input into pinned memory and its output
// back out of it: ~67 MB of host memcpy for a 1M-string encode + decode,
// which bounds it near the copy workers' rate (~22 GB/s of payload each way,
// DESIGN.md section 5).  Buffers the caller registered once (hipHostRegister,
// portable: every device's DMA engines reach them) are read and written by
// the transfers directly: no staging copy, and the path is bound by PCIe.
struct HostReg
{
    std::mutex mu;
    std::vector<std::pair<uintptr_t, uintptr_t>> r;      // [begin, end)
};
static HostReg g_reg;

bool
qhuff::host_registered(const void *p, uint64_t bytes)
{
    if (!bytes)
        return true;
    const uintptr_t a = (uintptr_t) p, b = a + bytes;
    std::lock_guard<std::mutex> g(g_reg.mu);
    for (const auto &x : g_reg.r)
        if (x.first <= a && b <= x.second)
            return true;
    return false;
}

extern "C" int
qhuff_host_register(void *ptr, size_t bytes)
{
    if (!ptr || !bytes)
        return QHUFF_EINVAL;
    std::lock_guard<std::mutex> g(g_reg.mu);
    for (const auto &x : g_reg.r)
        if (x.first == (uintptr_t) ptr)
            return QHUFF_EINVAL;         // (already registered)
    const hipError_t e = hipHostRegister(ptr, bytes, hipHostRegisterPortable);
    if (e != hipSuccess)
    {
        (void) hipGetLastError();
        snprintf(t_open_err, sizeof(t_open_err), "hipHostRegister: %s",
                 hipGetErrorString(e));
        return e == hipErrorOutOfMemory ? QHUFF_ENOMEM : QHUFF_EDEVICE;
    }
    g_reg.r.emplace_back((uintptr_t) ptr, (uintptr_t) ptr + bytes);
    return QHUFF_OK;
}

extern "C" int
qhuff_host_unregister(void *ptr)
{
    std::lock_guard<std::mutex> g(g_reg.mu);
    for (size_t i = 0; i < g_reg.r.size(); ++i)
        if (g_reg.r[i].first == (uintptr_t) ptr)
        {
            const hipError_t e = hipHostUnregister(ptr);
            g_reg.r.erase(g_reg.r.begin() + (ptrdiff_t) i);
            if (e != hipSuccess)
            {
                (void) hipGetLastError();
                return QHUFF_EDEVICE;
            }
            return QHUFF_OK;
        }
    return QHUFF_EINVAL;
}

// ---- the chunk plan of the host path -----------------------------------------
//
// Chunks of >= 2^shift bytes of input (QHUFF_HOST_CHUNK_SHIFT, 16..30;
// default 8 MB: measured on MI355X, 1M strings, 8 copy threads -- 2 MB
// chunks 2.9 / 2.7 ms enc / dec, 4 MB 2.2 / 2.0, 8 MB 1.8 / 1.7, 16 MB
// 1.9 / 2.3; tools/host_path_probe.py), at most kMaxChunks and at most one
// a string.  Chunk i is the strings [cut[i], cut[i + 1]); its output region
// in the stage starts at ob[i] and holds its own bound, rounded up to 16.
struct ChunkPlan
{
    unsigned K;
    uint32_t cut[kMaxChunks + 1];
    uint64_t ob[kMaxChunks + 1];                 // out region starts
    // a small batch brings its whole output bound back right behind the
    // kernel: one synchronisation instead of two (latency, not bandwidth)
    bool small;
};

static inline unsigned
chunk_shift_of(unsigned v)
{
    return v >= 16 && v <= 30 ? v : 23u;
}

// the process's own shift, read once
static unsigned
env_chunk_shift()
{
    static const unsigned shift = [] {
        const char *e = getenv("QHUFF_HOST_CHUNK_SHIFT");
        return chunk_shift_of(e ? (unsigned) strtoul(e, nullptr, 0) : 23u);
    }();
    return shift;
}

static void
chunk_plan(bool enc, unsigned mode, const uint32_t *in_off, uint32_t n,
           unsigned shift, ChunkPlan &p)
{
    const uint64_t in_bytes = (uint64_t) in_off[n] - in_off[0];
    unsigned K = (unsigned) (in_bytes >> shift);
    K = K < 1 ? 1 : (K > kMaxChunks ? kMaxChunks : K);
    if (K > n)
        K = n ? n : 1;
    p.K = K;
    p.ob[0] = 0;
    for (unsigned i = 0; i <= K; ++i)
        p.cut[i] = (uint32_t) ((uint64_t) n * i / K);
    for (unsigned i = 0; i < K; ++i)
    {
        const uint32_t s0 = p.cut[i], s1 = p.cut[i + 1];
        const uint64_t b = (uint64_t) in_off[s1] - in_off[s0];
        p.ob[i + 1] = p.ob[i] + up16(bound_of(enc, b, s1 - s0, mode));
    }
    p.small = K == 1 && p.ob[1] <= (4u << 20);
}

extern "C" int
qhuff_host_chunks(int enc, unsigned mode, const uint32_t *in_off, uint32_t n,
                  unsigned chunk_shift, uint32_t *cut, uint32_t *small)
{
    if (!in_off || !cut || (enc && !mode_ok(mode)) || in_off[n] < in_off[0])
        return QHUFF_EINVAL;
    ChunkPlan p;
    chunk_plan(enc != 0, mode, in_off, n,
               chunk_shift ? chunk_shift_of(chunk_shift) : env_chunk_shift(), p);
    if (p.ob[p.K] > 0xffffffffull)
        return QHUFF_ERANGE;
    memcpy(cut, p.cut, 4ull * (p.K + 1));
    if (small)
        *small = p.small;
    return (int) p.K;
}

// The PCIe-inclusive path as a chunked pipeline.  The batch is cut into K
// string ranges; per chunk: pinned staging copy (copy workers) -> H2D on the
// upload stream -> kernel on the context stream (its out_off / status come
// back on the same stream) -> once the chunk's size is known, D2H of exactly
// its output bytes on the download stream -> copy out + rebase out_off on
// the host.  Chunk i's host copies overlap chunk i-1's kernel and transfers.
// Kernels stay serialised on one stream (one look-back workspace).
//
// Stage layout (pinned and device alike): [in bytes | in_off (n + 1) |
// out: per-chunk bound regions | out_off: n_i + 1 per chunk | status n].
// The kernels read the original offsets: `in` is passed rebased by -in_off[0].
//
// Shard k of a multi-context call (qhuff_*_batch_host_multi, `sync`): the
// shard's output goes to `out` at a base only known once every earlier shard
// has sized its output, so its copies out of the pinned stage wait until
// all its chunks are fetched and the base is published -- its uploads,
// kernels and downloads never wait for another shard.
int
qhuff::host_batch(qhuff_ctx *c, bool enc, const uint8_t *in, const uint32_t *in_off,
           uint32_t n, unsigned mode, uint8_t *out, uint32_t *out_off,
           uint8_t *status, ShardSync *sync, unsigned shard, bool last_shard,
           bool out_reg)
{
    if (!c || !in_off || !out_off || (n && (!in || !out)) || (!enc && n && !status))
        return QHUFF_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = pipe_setup(c);
    if (rc)
        return rc;
    const uint64_t a0 = in_off[0], in_bytes = (uint64_t) in_off[n] - a0;
    // (the plan qhuff_host_chunks reports)
    ChunkPlan plan;
    chunk_plan(enc, mode, in_off, n, env_chunk_shift(), plan);
    const unsigned K = plan.K;
    const uint32_t *cut = plan.cut;
    const uint64_t *ob = plan.ob;
    if (ob[K] > 0xffffffffull)
        return QHUFF_ERANGE;
    const size_t o_in = 0, o_off = up16(in_bytes);
    const size_t o_out = o_off + up16(4ull * (n + 1));
    const size_t o_oo = o_out + ob[K];
    const size_t o_st = o_oo + up16(4ull * (n + K));
    const size_t total = o_st + up16(n ? n : 1);
    rc = ensure_stage(c, total);
    if (rc)
        return rc;
    uint8_t *H = c->h_stage, *D = c->d_stage;
    hipStream_t sk = c->own_stream;
    uint64_t base = 0;                           // output bytes so far
    uint32_t tot[kMaxChunks];
    uint64_t obase[kMaxChunks];                  // chunk i's output start
    uint64_t fbase = 0;                          // (relative to the call's)
    const bool small = plan.small;
    // caller buffers registered for DMA (qhuff_host_register): transferred
    // directly, no staging copy
    const bool din = host_registered(in + a0, in_bytes)
                  && host_registered(in_off, 4ull * (n + 1));
    // (a shard of a multi-context call writes at out + its base, beyond its
    // own bound from `out`: out_reg is host_multi's verdict over the whole
    // call's bound, the range the shards can write)
    const bool dout = !small
        && (sync ? out_reg
                 : host_registered(out, bound_of(enc, in_bytes, n, mode)))
        && host_registered(out_off, 4ull * (n + 1))
        && (enc || host_registered(status, n));

    auto stage_in = [&](unsigned i) -> int {
        const uint32_t s0 = cut[i], s1 = cut[i + 1];
        const uint64_t b0 = in_off[s0] - a0, b1 = in_off[s1] - a0;
        const uint8_t *src_in = in + a0;
        const uint8_t *src_off = (const uint8_t *) in_off;
        if (!din)
        {
            c->pool->copy(H + o_in + b0, in + a0 + b0, b1 - b0);
            memcpy(H + o_off + 4ull * s0, in_off + s0, 4ull * (s1 - s0 + 1));
            src_in = H + o_in;
            src_off = H + o_off;
        }
        HIPCHK(c, hipMemcpyAsync(D + o_in + b0, src_in + b0, b1 - b0,
                                 hipMemcpyHostToDevice, c->h2d_stream));
        HIPCHK(c, hipMemcpyAsync(D + o_off + 4ull * s0, src_off + 4ull * s0,
                                 4ull * (s1 - s0 + 1), hipMemcpyHostToDevice,
                                 c->h2d_stream));
        HIPCHK(c, hipEventRecord(c->ev_in[i], c->h2d_stream));
        HIPCHK(c, hipStreamWaitEvent(sk, c->ev_in[i], 0));
        const uint8_t *din = D + o_in - a0;      // kernels see original offsets
        const uint32_t *doff = (const uint32_t *) (D + o_off) + s0;
        uint32_t *doo = (uint32_t *) (D + o_oo) + s0 + i;
        host_hint(c, enc, in_off + s0, s1 - s0);
        int r = enc ? qhuff_encode_batch(c, din, doff, s1 - s0, mode,
                                         D + o_out + ob[i], doo, sk)
                    : qhuff_decode_batch(c, din, doff, s1 - s0,
                                         D + o_out + ob[i], doo, D + o_st + s0,
                                         sk);
        if (r)
            return r;
        if (dout)
        {
            // the chunk-local offsets straight into out_off (rebased in
            // place by unstage), the chunk's total into the stage
            HIPCHK(c, hipMemcpyAsync(out_off + s0, doo, 4ull * (s1 - s0),
                                     hipMemcpyDeviceToHost, sk));
            HIPCHK(c, hipMemcpyAsync(H + o_oo + 4ull * (s1 + i), doo + (s1 - s0),
                                     4, hipMemcpyDeviceToHost, sk));
            if (!enc)
                HIPCHK(c, hipMemcpyAsync(status + s0, D + o_st + s0, s1 - s0,
                                         hipMemcpyDeviceToHost, sk));
        }
        else
        {
            HIPCHK(c, hipMemcpyAsync(H + o_oo + 4ull * (s0 + i), doo,
                                     4ull * (s1 - s0 + 1), hipMemcpyDeviceToHost,
                                     sk));
            if (!enc)
                HIPCHK(c, hipMemcpyAsync(H + o_st + s0, D + o_st + s0, s1 - s0,
                                         hipMemcpyDeviceToHost, sk));
        }
        if (small)
            HIPCHK(c, hipMemcpyAsync(H + o_out, D + o_out, ob[1],
                                     hipMemcpyDeviceToHost, sk));
        HIPCHK(c, hipEventRecord(c->ev_k[i], sk));
        return QHUFF_OK;
    };
    // chunk i's output bytes back: to the stage, or (dout) straight to
    // out + dst (once its base is known)
    auto issue_out = [&](unsigned i, uint64_t dst) -> int {
        HIPCHK(c, hipStreamWaitEvent(c->d2h_stream, c->ev_k[i], 0));
        if (tot[i])
            HIPCHK(c, hipMemcpyAsync(dout ? out + dst : H + o_out + ob[i],
                                     D + o_out + ob[i], tot[i],
                                     hipMemcpyDeviceToHost, c->d2h_stream));
        HIPCHK(c, hipEventRecord(c->ev_out[i], c->d2h_stream));
        return QHUFF_OK;
    };
    auto fetch = [&](unsigned i) -> int {
        HIPCHK(c, hipEventSynchronize(c->ev_k[i]));
        const uint32_t s1 = cut[i + 1];
        tot[i] = ((const uint32_t *) (H + o_oo))[s1 + i];
        obase[i] = fbase;
        fbase += tot[i];
        if (small)
            return QHUFF_OK;                     // already here
        // (a shard of a multi-context call learns its base only later: its
        // direct copies out wait for it)
        if (dout && sync)
            return QHUFF_OK;
        return issue_out(i, obase[i]);
    };
    auto unstage = [&](unsigned i) -> int {
        if (!small)
            HIPCHK(c, hipEventSynchronize(c->ev_out[i]));
        const uint32_t s0 = cut[i], s1 = cut[i + 1];
        if (dout)
        {
            // bytes and statuses are in place; the offsets get the base
            const uint32_t bs = (uint32_t) base;
            const uint32_t m = s1 - s0, sl = 1u << 16;
            if (bs)
                c->pool->run((m + sl - 1) / sl, [=](unsigned k) {
                    const uint32_t a = k * sl, b = a + sl < m ? a + sl : m;
                    for (uint32_t j = a; j < b; ++j)
                        out_off[s0 + j] += bs;
                });
            base += tot[i];
            return QHUFF_OK;
        }
        c->pool->copy(out + base, H + o_out + ob[i], tot[i]);
        const uint32_t *ho = (const uint32_t *) (H + o_oo) + s0 + i;
        const uint32_t bs = (uint32_t) base;
        const uint32_t m = s1 - s0, sl = 1u << 16;
        c->pool->run((m + sl - 1) / sl, [=](unsigned k) {
            const uint32_t a = k * sl, b = a + sl < m ? a + sl : m;
            for (uint32_t j = a; j < b; ++j)
                out_off[s0 + j] = bs + ho[j];
        });
        if (!enc)
            memcpy(status + s0, H + o_st + s0, m);
        base += tot[i];
        return QHUFF_OK;
    };

    if (n == 0)
    {
        if (sync)
        {
            sync->publish(shard, 0);
            base = sync->base_of(shard);
            if (base == ~0ull)
                return QHUFF_EDEVICE;
        }
        if (last_shard)
            out_off[0] = (uint32_t) base;
        return QHUFF_OK;
    }
    if (sync)
    {
        // every chunk in flight first, then the copies out at the base
        for (unsigned i = 0; i < K; ++i)
        {
            if ((rc = stage_in(i)))
                return rc;
            if (i >= 1 && (rc = fetch(i - 1)))
                return rc;
        }
        if ((rc = fetch(K - 1)))
            return rc;
        uint64_t t = 0;
        for (unsigned i = 0; i < K; ++i)
            t += tot[i];
        sync->publish(shard, t);
        base = sync->base_of(shard);
        if (base == ~0ull)
            return QHUFF_EDEVICE;
        if (dout && !small)
            for (unsigned i = 0; i < K; ++i)
                if ((rc = issue_out(i, base + obase[i])))
                    return rc;
        for (unsigned i = 0; i < K; ++i)
            if ((rc = unstage(i)))
                return rc;
    }
    else
    {
        for (unsigned i = 0; i < K; ++i)
        {
            if ((rc = stage_in(i)))
                return rc;
            if (i >= 1 && (rc = fetch(i - 1)))
                return rc;
            if (i >= 2 && (rc = unstage(i - 2)))
                return rc;
        }
        if ((rc = fetch(K - 1)))
            return rc;
        for (unsigned i = K >= 2 ? K - 2 : 0; i < K; ++i)
            if ((rc = unstage(i)))
                return rc;
    }
    // (a shard's closing offset is the next shard's first one: written by
    // the last shard only)
    if (last_shard)
        out_off[n] = (uint32_t) base;
    if ((rc = mirror_error(c)))
        return rc;
    return QHUFF_OK;
}

extern "C" int
qhuff_encode_batch_host(qhuff_ctx *c, const uint8_t *in,
                        const uint32_t *in_off, uint32_t n, unsigned mode,
                        uint8_t *out, uint32_t *out_off)
{
    if (!mode_ok(mode))
        return QHUFF_EINVAL;
    // with a service attached the context may be shared between threads
    // (qhuff_lsqpack_set_context): every call goes through svc_call, which
    // serialises the ones too large for a slot on the context's host path
    // (host_batch shares the context's staging buffers, streams and events)
    if (c && c->svc)
        return svc_call(c->svc, true, in, in_off, n, mode, out, out_off, nullptr);
    return host_batch(c, true, in, in_off, n, mode, out, out_off, nullptr);
}

extern "C" int
qhuff_decode_batch_host(qhuff_ctx *c, const uint8_t *in,
                        const uint32_t *in_off, uint32_t n, uint8_t *out,
                        uint32_t *out_off, uint8_t *status)
{
    if (c && c->svc)                      // (see qhuff_encode_batch_host)
        return svc_call(c->svc, false, in, in_off, n, 0, out, out_off, status);
    return host_batch(c, false, in, in_off, n, 0, out, out_off, status);
}

// ---- one staged round trip ---------------------------------------------------
//
// qhuff_decode_stream_host, qhuff_decode_wire_host, qhuff_encode_wire_host
// (and, the first half, qhuff_xxh32_headers_host): the caller lays its
// regions out in the stage and makes its device-pointer call on the
// context's stream between stage_up() and stage_down().  Two
// synchronisations, the second for output bytes only.
struct StageIn
{
    const void *src;
    size_t bytes, at;                    // `at`: its offset in the stage
};

// a stage of `bytes`, the regions copied in, [0, up_end) sent in one copy
static int
stage_up(qhuff_ctx *c, size_t bytes, std::initializer_list<StageIn> in,
         size_t up_end)
{
    if (const int rc = ensure_stage(c, bytes))
        return rc;
    for (const StageIn &r : in)
        if (r.bytes)
            memcpy(c->h_stage + r.at, r.src, r.bytes);
    HIPCHK(c, hipMemcpyAsync(c->d_stage, c->h_stage, up_end,
                             hipMemcpyHostToDevice, c->own_stream));
    return QHUFF_OK;
}

// the small results [lo, o_out) back (out_off, n + 1 at o_oo, among them),
// the kernels' error word, then exactly out_off[n] bytes of out
static int
stage_down(qhuff_ctx *c, size_t lo, size_t o_oo, size_t o_out, uint32_t n,
           uint8_t *out, uint32_t *out_off)
{
    uint8_t *H = c->h_stage, *D = c->d_stage;
    hipStream_t sk = c->own_stream;
    HIPCHK(c, hipMemcpyAsync(H + lo, D + lo, o_out - lo, hipMemcpyDeviceToHost,
                             sk));
    HIPCHK(c, hipStreamSynchronize(sk));
    if (const int rc = mirror_error(c))
        return rc;
    const uint32_t total = ((const uint32_t *) (H + o_oo))[n];
    if (total)
    {
        HIPCHK(c, hipMemcpyAsync(H + o_out, D + o_out, total,
                                 hipMemcpyDeviceToHost, sk));
        HIPCHK(c, hipStreamSynchronize(sk));
        memcpy(out, H + o_out, total);
    }
    memcpy(out_off, H + o_oo, 4ull * (n + 1));
    return QHUFF_OK;
}

// Host pointers: one staged round trip on the context's stream.  Stage
// layout: [in | in_off | flags | state | out_off | status | out].
extern "C" int
qhuff_decode_stream_host(qhuff_ctx *c, const uint8_t *in,
                         const uint32_t *in_off, uint32_t n,
                         struct qhuff_decode_status *state,
                         const uint8_t *flags, uint8_t *out,
                         uint32_t *out_off, uint8_t *status)
{
    if (!c || !in_off || !out_off || (n && (!in || !out || !status || !state)))
        return QHUFF_EINVAL;
    if (n == 0)
    {
        out_off[0] = 0;
        return QHUFF_OK;
    }
    if (in_off[n] < in_off[0])
        return QHUFF_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t a0 = in_off[0], in_bytes = (uint64_t) in_off[n] - a0;
    const uint64_t bound = qhuff_decode_stream_bound(in_bytes, n);
    if (bound > 0xffffffffull)
        return QHUFF_ERANGE;
    const size_t o_off = up16(in_bytes) + 16;
    const size_t o_fl = o_off + up16(4ull * (n + 1));
    const size_t o_state = o_fl + up16(n);
    const size_t o_oo = o_state + up16(2ull * n);
    const size_t o_st = o_oo + up16(4ull * (n + 1));
    const size_t o_out = o_st + up16(n);
    int rc = stage_up(c, o_out + up16(bound),
                      {{in + a0, in_bytes, 0}, {in_off, 4ull * (n + 1), o_off},
                       {flags, flags ? n : 0, o_fl},
                       {state, 2ull * n, o_state}}, o_oo);
    if (rc)
        return rc;
    uint8_t *D = c->d_stage;
    // (the kernel reads the caller's offsets: `in` rebased by -in_off[0])
    rc = qhuff_decode_stream(c, D - a0, (const uint32_t *) (D + o_off), n,
                             (struct qhuff_decode_status *) (D + o_state),
                             flags ? D + o_fl : nullptr, D + o_out,
                             (uint32_t *) (D + o_oo), D + o_st, c->own_stream);
    if (rc)
        return rc;
    if ((rc = stage_down(c, o_state, o_oo, o_out, n, out, out_off)))
        return rc;
    memcpy(state, c->h_stage + o_state, 2ull * n);
    memcpy(status, c->h_stage + o_st, n);
    return QHUFF_OK;
}

// ---- batched literal decode (pre-parsed spans, qhuff_frames.cpp) -----------

extern "C" uint64_t
qhuff_literals_bound(const struct qhuff_literal *lits, uint32_t n)
{
    uint64_t b = 16;
    for (uint32_t i = 0; lits && i < n; ++i)
        b += lits[i].huffman ? (uint64_t) lits[i].len * 8 / 5 : lits[i].len;
    return b;
}

// Huffman payloads gathered straight into the pinned stage (one copy), one
// decode launch for all of them, raw literals copied on the host meanwhile.
// Stage layout: [huff bytes | in_off | out bytes | out_off | status].
extern "C" int
qhuff_decode_literals_host(qhuff_ctx *c, const uint8_t *buf,
                           const struct qhuff_literal *lits, uint32_t n,
                           uint8_t *out, uint32_t *out_off, uint8_t *status)
{
    return qhuff_decode_literals_ex(c, buf, lits, n, 0, out, out_off, status);
}

// max_len > 0: the field-section limit -- a string that decodes (or is
// declared, raw) longer than LSXPACK_MAX_STRLEN is an error in the
// reference (header_out_grow_buf, lsqpack.c:3350-3351; 3682-3685,
// 3769-3772), whatever the kernel's status.
extern "C" int
qhuff_decode_literals_ex(qhuff_ctx *c, const uint8_t *buf,
                         const struct qhuff_literal *lits, uint32_t n,
                         uint32_t max_len, uint8_t *out, uint32_t *out_off,
                         uint8_t *status)
{
    if (!c || !out_off || (n && (!buf || !lits || !out || !status)))
        return QHUFF_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    uint64_t hb = 0;
    uint32_t nh = 0;
    for (uint32_t i = 0; i < n; ++i)
        if (lits[i].huffman)
        {
            hb += lits[i].len;
            ++nh;
        }
    const uint64_t ob = qhuff_decode_bound(hb, nh);
    if (ob > 0xffffffffull || hb > 0xffffffffull)
        return QHUFF_ERANGE;
    const size_t o_off = up16(hb), o_out = o_off + up16(4ull * (nh + 1));
    const size_t o_oo = o_out + up16(ob), o_st = o_oo + up16(4ull * (nh + 1));
    const size_t total = o_st + up16(nh ? nh : 1);
    int rc = ensure_stage(c, total);
    if (rc)
        return rc;
    hipStream_t st = c->own_stream;
    uint32_t *hoff = (uint32_t *) (c->h_stage + o_off);
    {
        uint32_t k = 0, a = 0;
        for (uint32_t i = 0; i < n; ++i)
            if (lits[i].huffman)
            {
                memcpy(c->h_stage + a, buf + lits[i].pos, lits[i].len);
                hoff[k++] = a;
                a += lits[i].len;
            }
        hoff[k] = a;
    }
    if (nh)
    {
        // the variant from this batch (auto mode only: a pinned variant
        // needs neither the copy workers nor the scan)
        if (c->kernels == 0)
        {
            if (!c->pipe_ready && (rc = pipe_setup(c)))
                return rc;
            host_hint(c, false, hoff, nh);
        }
        HIPCHK(c, hipMemcpyAsync(c->d_stage, c->h_stage, o_out,
                                 hipMemcpyHostToDevice, st));
        rc = qhuff_decode_batch(c, c->d_stage, (const uint32_t *) (c->d_stage
                                + o_off), nh, c->d_stage + o_out,
                                (uint32_t *) (c->d_stage + o_oo),
                                c->d_stage + o_st, st);
        if (rc)
            return rc;
        if (o_st + nh - o_out <= (4u << 20))
        {
            // small: the decoded bytes' bound, sizes and status in one copy
            HIPCHK(c, hipMemcpyAsync(c->h_stage + o_out, c->d_stage + o_out,
                                     o_st + nh - o_out, hipMemcpyDeviceToHost,
                                     st));
            HIPCHK(c, hipStreamSynchronize(st));
        }
        else
        {
            // sizes and status first, then exactly the decoded bytes
            HIPCHK(c, hipMemcpyAsync(c->h_stage + o_oo, c->d_stage + o_oo,
                                     4ull * (nh + 1), hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipMemcpyAsync(c->h_stage + o_st, c->d_stage + o_st, nh,
                                     hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipStreamSynchronize(st));
            const uint32_t dec_total = ((const uint32_t *) (c->h_stage + o_oo))[nh];
            HIPCHK(c, hipMemcpyAsync(c->h_stage + o_out, c->d_stage + o_out,
                                     dec_total, hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipStreamSynchronize(st));
        }
        if ((rc = mirror_error(c)))
            return rc;
    }
    const uint32_t *doo = (const uint32_t *) (c->h_stage + o_oo);
    const uint8_t *dst = c->h_stage + o_st;
    uint64_t o = 0;
    uint32_t k = 0;
    // max_len (field sections): the reference decodes a field line's name
    // and value into ONE header buffer, which never grows past
    // LSXPACK_MAX_STRLEN (header_out_grow_buf, lsqpack.c:3346-3351; its
    // size is a uint16 lsxpack_strlen_t): a name decoded here (NAME literal
    // of the same instruction) or a static-table name (field_ref_name_len)
    // counts against its value.  A dynamic-table name is not known to the
    // framing: that value is checked alone.
    uint32_t name_len = 0, name_instr = 0;
    bool have_name = false;
    for (uint32_t i = 0; i < n; ++i)
    {
        out_off[i] = (uint32_t) o;
        uint32_t len = lits[i].len;
        uint8_t stv = QHUFF_DEC_OK;
        const uint8_t *src = buf + lits[i].pos;
        if (lits[i].huffman)
        {
            const uint32_t a = doo[k], b = doo[k + 1];
            stv = dst[k];
            ++k;
            len = b - a;
            src = c->h_stage + o_out + a;
        }
        uint32_t lim_used = 0;
        if (max_len && lits[i].kind == QHUFF_LIT_VALUE)
            lim_used = have_name && name_instr == lits[i].instr
                     ? name_len : field_ref_name_len(buf, lits[i]);
        have_name = false;
        if (max_len && (uint64_t) lim_used + len > max_len)
            stv = QHUFF_DEC_ERROR;
        status[i] = stv;
        if (stv != QHUFF_DEC_OK)
            continue;
        if (lits[i].kind == QHUFF_LIT_NAME)
        {
            have_name = true;
            name_len = len;
            name_instr = lits[i].instr;
        }
        memcpy(out + o, src, len);
        o += len;
    }
    out_off[n] = (uint32_t) o;
    return QHUFF_OK;
}

// The literals decoded where they lie (qhuff_decode_wire): the wire bytes
// from the first literal's instruction to the last literal's end go up as
// they are, with the descriptors; one launch; exactly the decoded bytes
// come back.  No payload is gathered and no result interleaved on the host.
// Stage layout: [16 | wire bytes | 16 | lits | out_off | status | out]; the
// kernel sees the caller's positions: `buf` rebased by -lo.
extern "C" int
qhuff_decode_wire_host(qhuff_ctx *c, const uint8_t *buf,
                       const struct qhuff_literal *lits, uint32_t n,
                       uint32_t max_len, uint8_t *out, uint32_t *out_off,
                       uint8_t *status)
{
    if (!c || !out_off || (n && (!buf || !lits || !out || !status)))
        return QHUFF_EINVAL;
    if (n == 0)
    {
        out_off[0] = 0;
        return QHUFF_OK;
    }
    if (qhuff_literals_check(lits, n, nullptr))
        return QHUFF_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    // the order rule puts every payload behind the first literal's
    // instruction; an instruction the limit may read (a VALUE literal's) is
    // the one thing it lets lie before that
    uint64_t lo = lits[0].instr < lits[0].pos ? lits[0].instr : lits[0].pos;
    if (max_len)
        for (uint32_t i = 1; i < n; ++i)
            if (lits[i].instr < lo)
                lo = lits[i].instr;
    const uint64_t hi = (uint64_t) lits[n - 1].pos + lits[n - 1].len;
    const uint64_t span = hi - lo, bound = qhuff_literals_bound(lits, n);
    if (bound > 0xffffffffull || span > 0xffffffffull)
        return QHUFF_ERANGE;
    const size_t o_buf = 16, o_lits = up16(o_buf + span) + 16;
    const size_t o_oo = o_lits + 16ull * n;
    const size_t o_st = o_oo + up16(4ull * (n + 1));
    const size_t o_out = o_st + up16(n);
    int rc = stage_up(c, o_out + up16(bound),
                      {{buf + lo, span, o_buf}, {lits, 16ull * n, o_lits}},
                      o_oo);
    if (rc)
        return rc;
    uint8_t *D = c->d_stage;
    rc = qhuff_decode_wire(c, D + o_buf - lo,
                           (const struct qhuff_literal *) (D + o_lits), n,
                           max_len, D + o_out, (uint32_t *) (D + o_oo),
                           D + o_st, c->own_stream);
    if (rc)
        return rc;
    if ((rc = stage_down(c, o_oo, o_oo, o_out, n, out, out_off)))
        return rc;
    memcpy(status, c->h_stage + o_st, n);
    return QHUFF_OK;
}

// ---- chunks scanned on the device (qhuff_scan_sections) --------------------

// The wire bytes and their offsets up, the scan on the context's stream, the
// small results (lit_off, rc, consumed) back: the first half of both host
// forms.  Stage layout: [16 | wire bytes | 16 | sec_off | lit_off | rc | consumed |
// lits]; the kernels read the caller's offsets unchanged: `buf` rebased by
// -sec_off[0].  *o_lits: where the descriptors are in the stage, *o_end: the
// end of the (max_lits) descriptors; `extra` more bytes are kept behind them.
static int
scan_staged(qhuff_ctx *c, const uint8_t *buf, const uint32_t *sec_off,
            uint32_t m, unsigned mode, uint32_t max_lits, uint32_t *lit_off,
            int32_t *rc, uint32_t *consumed, uint64_t extra, size_t *o_lits,
            size_t *o_end)
{
    const uint64_t a0 = sec_off[0], bytes = (uint64_t) sec_off[m] - a0;
    const size_t o_so = up16(16 + bytes) + 16;
    const size_t o_lo = o_so + up16(4ull * (m + 1));
    const size_t o_rc = o_lo + up16(4ull * (m + 1));
    const size_t o_co = o_rc + up16(4ull * m);
    *o_lits = o_co + up16(4ull * m);
    *o_end = *o_lits + 16ull * max_lits;
    int r = stage_up(c, *o_end + extra,
                     {{buf + a0, bytes, 16}, {sec_off, 4ull * (m + 1), o_so}},
                     o_lo);
    if (r)
        return r;
    uint8_t *H = c->h_stage, *D = c->d_stage;
    r = qhuff_scan_sections(c, D + 16 - a0, (const uint32_t *) (D + o_so), m, mode,
                            (struct qhuff_literal *) (D + *o_lits), max_lits,
                            (uint32_t *) (D + o_lo), (int32_t *) (D + o_rc),
                            (uint32_t *) (D + o_co), c->own_stream);
    if (r)
        return r;
    HIPCHK(c, hipMemcpyAsync(H + o_lo, D + o_lo, *o_lits - o_lo,
                             hipMemcpyDeviceToHost, c->own_stream));
    HIPCHK(c, hipStreamSynchronize(c->own_stream));
    memcpy(lit_off, H + o_lo, 4ull * (m + 1));
    memcpy(rc, H + o_rc, 4ull * m);
    if (consumed)
        memcpy(consumed, H + o_co, 4ull * m);
    return QHUFF_OK;
}

static bool
scan_args_ok(qhuff_ctx *c, const uint8_t *buf, const uint32_t *sec_off,
             uint32_t m, unsigned mode, struct qhuff_literal *lits,
             uint32_t max_lits, uint32_t *lit_off, int32_t *rc,
             uint32_t *consumed)
{
    if (!c || !lit_off || (mode != QHUFF_SCAN_FIELD_SECTION
                           && mode != QHUFF_SCAN_ENCODER_STREAM)
            || (m && (!buf || !sec_off || !rc
                      || (!consumed && mode == QHUFF_SCAN_ENCODER_STREAM)))
            || (max_lits && !lits))
        return false;
    for (uint32_t i = 0; i < m; ++i)
        if (sec_off[i + 1] < sec_off[i])
            return false;
    return true;
}

extern "C" int
qhuff_scan_sections_host(qhuff_ctx *c, const uint8_t *buf,
                         const uint32_t *sec_off, uint32_t m, unsigned mode,
                         struct qhuff_literal *lits, uint32_t max_lits,
                         uint32_t *lit_off, int32_t *rc, uint32_t *consumed)
{
    if (!scan_args_ok(c, buf, sec_off, m, mode, lits, max_lits, lit_off, rc,
                      consumed))
        return QHUFF_EINVAL;
    if (m == 0)
    {
        lit_off[0] = 0;
        return QHUFF_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    size_t o_lits, o_end;
    int r = scan_staged(c, buf, sec_off, m, mode, max_lits, lit_off, rc,
                        consumed, 0, &o_lits, &o_end);
    if (r)
        return r;
    const uint32_t n = lit_off[m] < max_lits ? lit_off[m] : max_lits;
    if (n)
    {
        HIPCHK(c, hipMemcpyAsync(c->h_stage + o_lits, c->d_stage + o_lits,
                                 16ull * n, hipMemcpyDeviceToHost,
                                 c->own_stream));
        HIPCHK(c, hipStreamSynchronize(c->own_stream));
        memcpy(lits, c->h_stage + o_lits, 16ull * n);
    }
    return lit_off[m] > max_lits ? QHUFF_ERANGE : QHUFF_OK;
}

// The whole decode path: scan_staged, then qhuff_decode_wire on the
// descriptors where the scan left them, then the descriptors, out_off and
// status in one copy and exactly out_off[n] bytes in another.  Behind the n
// descriptors the stage holds [out_off | status | out].
extern "C" int
qhuff_decode_sections_host(qhuff_ctx *c, const uint8_t *buf,
                           const uint32_t *sec_off, uint32_t m, unsigned mode,
                           uint32_t max_len, struct qhuff_literal *lits,
                           uint32_t max_lits, uint32_t *lit_off, int32_t *rc,
                           uint32_t *consumed, uint8_t *out, uint32_t *out_off,
                           uint8_t *status)
{
    if (!out_off || !scan_args_ok(c, buf, sec_off, m, mode, lits, max_lits,
                                  lit_off, rc, consumed)
            || (max_lits && (!out || !status)))
        return QHUFF_EINVAL;
    if (m == 0)
    {
        lit_off[0] = 0;
        out_off[0] = 0;
        return QHUFF_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t bytes = (uint64_t) sec_off[m] - sec_off[0];
    const uint64_t bound = qhuff_decode_bound(bytes, 0);
    if (bound > 0xffffffffull)
        return QHUFF_ERANGE;
    // (room for max_lits literals; laid out for the n there are, so that
    // what comes back is theirs alone)
    size_t o_lits, o_end;
    int r = scan_staged(c, buf, sec_off, m, mode, max_lits, lit_off, rc,
                        consumed, up16(4ull * ((uint64_t) max_lits + 1))
                                      + up16(max_lits) + up16(bound),
                        &o_lits, &o_end);
    if (r)
        return r;
    const uint32_t n = lit_off[m];
    if (n > max_lits)
    {
        // as qhuff_scan_sections_host: the first max_lits descriptors
        if (max_lits)
        {
            HIPCHK(c, hipMemcpyAsync(c->h_stage + o_lits, c->d_stage + o_lits,
                                     16ull * max_lits, hipMemcpyDeviceToHost,
                                     c->own_stream));
            HIPCHK(c, hipStreamSynchronize(c->own_stream));
            memcpy(lits, c->h_stage + o_lits, 16ull * max_lits);
        }
        return QHUFF_ERANGE;
    }
    const size_t o_oo = o_lits + 16ull * n;
    const size_t o_st = o_oo + up16(4ull * ((uint64_t) n + 1));
    const size_t o_out = o_st + up16(n);
    uint8_t *D = c->d_stage;
    r = qhuff_decode_wire(c, D + 16 - sec_off[0],
                          (const struct qhuff_literal *) (D + o_lits), n,
                          max_len, D + o_out, (uint32_t *) (D + o_oo),
                          D + o_st, c->own_stream);
    if (r)
        return r;
    if ((r = stage_down(c, o_lits, o_oo, o_out, n, out, out_off)))
        return r;
    if (n)
    {
        memcpy(lits, c->h_stage + o_lits, 16ull * n);
        memcpy(status, c->h_stage + o_st, n);
    }
    return QHUFF_OK;
}

// ---- header lists from field sections (qhuff_scan_headers) ------------------

// The first half of both host forms, as scan_staged: the wire bytes and their
// offsets up, the header scan on the context's stream, hdr_off and rc back.
// Stage layout: [16 | wire bytes | 16 | sec_off | hdr_off | rc | strs | kind |
// static_id | hflags], the last four sized for max_hdrs; `extra` more bytes
// are kept behind them, from o->end.
struct HdrStage
{
    size_t strs, kind, id, hf, end;
};

static int
hdr_staged(qhuff_ctx *c, const uint8_t *buf, const uint32_t *sec_off,
           uint32_t m, uint32_t max_hdrs, uint32_t *hdr_off, int32_t *rc,
           uint64_t extra, HdrStage *o)
{
    const uint64_t a0 = sec_off[0], bytes = (uint64_t) sec_off[m] - a0;
    const size_t o_so = up16(16 + bytes) + 16;
    const size_t o_ho = o_so + up16(4ull * (m + 1));
    const size_t o_rc = o_ho + up16(4ull * (m + 1));
    o->strs = o_rc + up16(4ull * m);
    o->kind = o->strs + 32ull * max_hdrs;
    o->id = o->kind + up16(max_hdrs);
    o->hf = o->id + up16(max_hdrs);
    o->end = o->hf + up16(max_hdrs);
    int r = stage_up(c, o->end + extra,
                     {{buf + a0, bytes, 16}, {sec_off, 4ull * (m + 1), o_so}},
                     o_ho);
    if (r)
        return r;
    uint8_t *H = c->h_stage, *D = c->d_stage;
    r = qhuff_scan_headers(c, D + 16 - a0, (const uint32_t *) (D + o_so), m,
                           (struct qhuff_hstr *) (D + o->strs), max_hdrs,
                           (uint32_t *) (D + o_ho), (int32_t *) (D + o_rc),
                           D + o->kind, D + o->id, D + o->hf, c->own_stream);
    if (r)
        return r;
    HIPCHK(c, hipMemcpyAsync(H + o_ho, D + o_ho, o->strs - o_ho,
                             hipMemcpyDeviceToHost, c->own_stream));
    HIPCHK(c, hipStreamSynchronize(c->own_stream));
    memcpy(hdr_off, H + o_ho, 4ull * (m + 1));
    memcpy(rc, H + o_rc, 4ull * m);
    return QHUFF_OK;
}

static bool
hdr_args_ok(qhuff_ctx *c, const uint8_t *buf, const uint32_t *sec_off,
            uint32_t m, uint32_t *hdr_off, int32_t *rc)
{
    if (!c || !hdr_off || (m && (!buf || !sec_off || !rc)))
        return false;
    for (uint32_t i = 0; i < m; ++i)
        if (sec_off[i + 1] < sec_off[i])
            return false;
    return true;
}

// the first n headers' byte arrays from the stage, those the caller asked for
static void
hdr_bytes_out(const qhuff_ctx *c, const HdrStage &o, uint32_t n, uint8_t *kind,
              uint8_t *static_id, uint8_t *hflags)
{
    if (kind)
        memcpy(kind, c->h_stage + o.kind, n);
    if (static_id)
        memcpy(static_id, c->h_stage + o.id, n);
    if (hflags)
        memcpy(hflags, c->h_stage + o.hf, n);
}

extern "C" int
qhuff_scan_headers_host(qhuff_ctx *c, const uint8_t *buf,
                        const uint32_t *sec_off, uint32_t m,
                        struct qhuff_hstr *strs, uint32_t max_hdrs,
                        uint32_t *hdr_off, int32_t *rc, uint8_t *kind,
                        uint8_t *static_id, uint8_t *hflags)
{
    if (!hdr_args_ok(c, buf, sec_off, m, hdr_off, rc) || (max_hdrs && !strs))
        return QHUFF_EINVAL;
    if (m == 0)
    {
        hdr_off[0] = 0;
        return QHUFF_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    HdrStage o;
    int r = hdr_staged(c, buf, sec_off, m, max_hdrs, hdr_off, rc, 0, &o);
    if (r)
        return r;
    const uint32_t n = hdr_off[m] < max_hdrs ? hdr_off[m] : max_hdrs;
    if (n)
    {
        uint8_t *H = c->h_stage, *D = c->d_stage;
        HIPCHK(c, hipMemcpyAsync(H + o.strs, D + o.strs, 32ull * n,
                                 hipMemcpyDeviceToHost, c->own_stream));
        HIPCHK(c, hipMemcpyAsync(H + o.kind, D + o.kind, o.hf + n - o.kind,
                                 hipMemcpyDeviceToHost, c->own_stream));
        HIPCHK(c, hipStreamSynchronize(c->own_stream));
        memcpy(strs, H + o.strs, 32ull * n);
        hdr_bytes_out(c, o, n, kind, static_id, hflags);
    }
    return hdr_off[m] > max_hdrs ? QHUFF_ERANGE : QHUFF_OK;
}

// The whole path: hdr_staged, then qhuff_decode_headers on the descriptors
// where the scan left them and, if asked for, qhuff_xxh32_headers over its
// output where that lies; then the byte arrays, off, status and hashes in one
// copy and exactly off[2n] bytes in another.  Behind the scan's regions the
// stage holds [off | status | name_hash | nameval_hash | out], laid out for
// the n headers there are.
extern "C" int
qhuff_decode_headers_host(qhuff_ctx *c, const uint8_t *buf,
                          const uint32_t *sec_off, uint32_t m,
                          uint32_t max_len, uint32_t max_hdrs,
                          uint32_t *hdr_off, int32_t *rc, uint8_t *kind,
                          uint8_t *static_id, uint8_t *hflags, uint8_t *out,
                          uint32_t *off, uint8_t *status, uint32_t *name_hash,
                          uint32_t *nameval_hash)
{
    if (!off || !hdr_args_ok(c, buf, sec_off, m, hdr_off, rc)
            || (max_hdrs && (!out || !status)))
        return QHUFF_EINVAL;
    if (max_hdrs > 0x7fffffffu)
        return QHUFF_ERANGE;
    if (m == 0)
    {
        hdr_off[0] = 0;
        off[0] = 0;
        return QHUFF_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t bytes = (uint64_t) sec_off[m] - sec_off[0];
    if (qhuff_decode_headers_bound(bytes, max_hdrs) > 0xffffffffull)
        return QHUFF_ERANGE;
    const uint64_t mh = max_hdrs;
    HdrStage o;
    int r = hdr_staged(c, buf, sec_off, m, max_hdrs, hdr_off, rc,
                       up16(4 * (2 * mh + 1)) + up16(2 * mh)
                           + 2 * up16(4 * mh)
                           + up16(qhuff_decode_headers_bound(bytes, max_hdrs)),
                       &o);
    if (r)
        return r;
    const uint32_t n = hdr_off[m];
    if (n > max_hdrs)
        return QHUFF_ERANGE;
    const size_t o_off = o.end;
    const size_t o_st = o_off + up16(4 * (2ull * n + 1));
    const size_t o_h1 = o_st + up16(2ull * n);
    const size_t o_h2 = o_h1 + up16(4ull * n);
    const size_t o_out = o_h2 + up16(4ull * n);
    uint8_t *H = c->h_stage, *D = c->d_stage;
    r = qhuff_decode_headers(c, D + 16 - sec_off[0],
                             (const struct qhuff_hstr *) (D + o.strs), n,
                             max_len, D + o_out, (uint32_t *) (D + o_off),
                             D + o_st, c->own_stream);
    if (r)
        return r;
    if (n && (name_hash || nameval_hash))
    {
        r = qhuff_xxh32_headers(c, D + o_out, (const uint32_t *) (D + o_off),
                                n, QHUFF_XXH_SEED, (uint32_t *) (D + o_h1),
                                (uint32_t *) (D + o_h2), c->own_stream);
        if (r)
            return r;
    }
    if ((r = stage_down(c, o.kind, o_off, o_out, 2 * n, out, off)))
        return r;
    if (n)
    {
        hdr_bytes_out(c, o, n, kind, static_id, hflags);
        memcpy(status, H + o_st, 2ull * n);
        if (name_hash)
            memcpy(name_hash, H + o_h1, 4ull * n);
        if (nameval_hash)
            memcpy(nameval_hash, H + o_h2, 4ull * n);
    }
    return QHUFF_OK;
}

// ---- ... against the dynamic table's entries (qhuff_scan_headers_dyn) --------

// hdr_staged with the table: its bytes, its offsets and the windows go up
// with the wire bytes.  Stage layout: [16 | wire bytes | 16 | sec_off | table
// bytes | table off | sec_win | hdr_off | rc | strs | kind | static_id |
// hflags | dyn_id], the last five sized for max_hdrs; `extra` more bytes are
// kept behind them, from o->h.end.
struct DynStage
{
    HdrStage h;
    size_t tab, did;                     // the table's bytes; dyn_id
};

static int
dyn_staged(qhuff_ctx *c, const uint8_t *buf, const uint32_t *sec_off,
           uint32_t m, const struct qhuff_dyn_table *tab,
           const uint32_t *sec_win, uint32_t max_hdrs, uint32_t *hdr_off,
           int32_t *rc, uint64_t extra, DynStage *o)
{
    const uint64_t a0 = sec_off[0], bytes = (uint64_t) sec_off[m] - a0;
    const uint64_t d = tab->d;
    const uint64_t t0 = d ? tab->off[0] : 0, tb = d ? tab->off[2 * d] - t0 : 0;
    const size_t o_so = up16(16 + bytes) + 16;
    o->tab = o_so + up16(4ull * (m + 1));
    const size_t o_to = o->tab + up16(tb);
    const size_t o_sw = o_to + up16(4 * (2 * d + 1));
    const size_t o_ho = o_sw + up16(sec_win ? 8ull * m : 0);
    const size_t o_rc = o_ho + up16(4ull * (m + 1));
    o->h.strs = o_rc + up16(4ull * m);
    o->h.kind = o->h.strs + 32ull * max_hdrs;
    o->h.id = o->h.kind + up16(max_hdrs);
    o->h.hf = o->h.id + up16(max_hdrs);
    o->did = o->h.hf + up16(max_hdrs);
    o->h.end = o->did + up16(4ull * max_hdrs);
    int r = stage_up(c, o->h.end + extra,
                     {{buf + a0, bytes, 16}, {sec_off, 4ull * (m + 1), o_so},
                      {d ? tab->bytes + t0 : nullptr, tb, o->tab},
                      {tab->off, d ? 4 * (2 * d + 1) : 0, o_to},
                      {sec_win, sec_win ? 8ull * m : 0, o_sw}},
                     o_ho);
    if (r)
        return r;
    uint8_t *H = c->h_stage, *D = c->d_stage;
    // (the kernels read the caller's offsets unchanged: the table's bytes are
    // passed rebased by -off[0])
    struct qhuff_dyn_table dev = *tab;
    dev.bytes = D + o->tab - t0;
    dev.off = d ? (const uint32_t *) (D + o_to) : nullptr;
    r = qhuff_scan_headers_dyn(c, D + 16 - a0, (const uint32_t *) (D + o_so),
                               m, &dev,
                               sec_win ? (const uint32_t *) (D + o_sw)
                                       : nullptr,
                               (struct qhuff_hstr *) (D + o->h.strs), max_hdrs,
                               (uint32_t *) (D + o_ho), (int32_t *) (D + o_rc),
                               D + o->h.kind, D + o->h.id, D + o->h.hf,
                               (uint32_t *) (D + o->did), c->own_stream);
    if (r)
        return r;
    HIPCHK(c, hipMemcpyAsync(H + o_ho, D + o_ho, o->h.strs - o_ho,
                             hipMemcpyDeviceToHost, c->own_stream));
    HIPCHK(c, hipStreamSynchronize(c->own_stream));
    memcpy(hdr_off, H + o_ho, 4ull * (m + 1));
    memcpy(rc, H + o_rc, 4ull * m);
    return QHUFF_OK;
}

extern "C" int
qhuff_scan_headers_dyn_host(qhuff_ctx *c, const uint8_t *buf,
                            const uint32_t *sec_off, uint32_t m,
                            const struct qhuff_dyn_table *tab,
                            const uint32_t *sec_win, struct qhuff_hstr *strs,
                            uint32_t max_hdrs, uint32_t *hdr_off, int32_t *rc,
                            uint8_t *kind, uint8_t *static_id,
                            uint8_t *hflags, uint32_t *dyn_id)
{
    if (!hdr_args_ok(c, buf, sec_off, m, hdr_off, rc) || (max_hdrs && !strs))
        return QHUFF_EINVAL;
    uint32_t longest;
    if (const int r = scan::dyn_check(tab, sec_win, m, &longest))
        return r;
    if (m == 0)
    {
        hdr_off[0] = 0;
        return QHUFF_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    DynStage o;
    int r = dyn_staged(c, buf, sec_off, m, tab, sec_win, max_hdrs, hdr_off,
                       rc, 0, &o);
    if (r)
        return r;
    const uint32_t n = hdr_off[m] < max_hdrs ? hdr_off[m] : max_hdrs;
    if (n)
    {
        uint8_t *H = c->h_stage, *D = c->d_stage;
        HIPCHK(c, hipMemcpyAsync(H + o.h.strs, D + o.h.strs, 32ull * n,
                                 hipMemcpyDeviceToHost, c->own_stream));
        HIPCHK(c, hipMemcpyAsync(H + o.h.kind, D + o.h.kind,
                                 o.did + 4ull * n - o.h.kind,
                                 hipMemcpyDeviceToHost, c->own_stream));
        HIPCHK(c, hipStreamSynchronize(c->own_stream));
        memcpy(strs, H + o.h.strs, 32ull * n);
        hdr_bytes_out(c, o.h, n, kind, static_id, hflags);
        if (dyn_id)
            memcpy(dyn_id, H + o.did, 4ull * n);
    }
    return hdr_off[m] > max_hdrs ? QHUFF_ERANGE : QHUFF_OK;
}

// The whole path, as qhuff_decode_headers_host: dyn_staged, then
// qhuff_decode_headers_dyn on the descriptors and on the table's bytes where
// they lie.
extern "C" int
qhuff_decode_headers_dyn_host(qhuff_ctx *c, const uint8_t *buf,
                              const uint32_t *sec_off, uint32_t m,
                              const struct qhuff_dyn_table *tab,
                              const uint32_t *sec_win, uint32_t max_len,
                              uint32_t max_hdrs, uint32_t *hdr_off,
                              int32_t *rc, uint8_t *kind, uint8_t *static_id,
                              uint8_t *hflags, uint32_t *dyn_id, uint8_t *out,
                              uint32_t *off, uint8_t *status,
                              uint32_t *name_hash, uint32_t *nameval_hash)
{
    if (!off || !hdr_args_ok(c, buf, sec_off, m, hdr_off, rc)
            || (max_hdrs && (!out || !status)))
        return QHUFF_EINVAL;
    if (max_hdrs > 0x7fffffffu)
        return QHUFF_ERANGE;
    uint32_t longest;
    if (const int r = scan::dyn_check(tab, sec_win, m, &longest))
        return r;
    if (m == 0)
    {
        hdr_off[0] = 0;
        off[0] = 0;
        return QHUFF_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t bytes = (uint64_t) sec_off[m] - sec_off[0];
    const uint64_t bound = qhuff_decode_headers_dyn_bound(bytes, max_hdrs,
                                                          longest);
    if (bound > 0xffffffffull)
        return QHUFF_ERANGE;
    const uint64_t mh = max_hdrs;
    DynStage o;
    int r = dyn_staged(c, buf, sec_off, m, tab, sec_win, max_hdrs, hdr_off,
                       rc,
                       up16(4 * (2 * mh + 1)) + up16(2 * mh)
                           + 2 * up16(4 * mh) + up16(bound),
                       &o);
    if (r)
        return r;
    const uint32_t n = hdr_off[m];
    if (n > max_hdrs)
        return QHUFF_ERANGE;
    const size_t o_off = o.h.end;
    const size_t o_st = o_off + up16(4 * (2ull * n + 1));
    const size_t o_h1 = o_st + up16(2ull * n);
    const size_t o_h2 = o_h1 + up16(4ull * n);
    const size_t o_out = o_h2 + up16(4ull * n);
    uint8_t *H = c->h_stage, *D = c->d_stage;
    const uint32_t t0 = tab->d ? tab->off[0] : 0;
    const uint32_t t1 = tab->d ? tab->off[2ull * tab->d] : 0;
    // (dyn_bytes rebased as the scan's table: instr is an offset from
    // tab->bytes; the kernel's blocks are those of [t0, t1) of it)
    r = qhuff_decode_headers_dyn(c, D + 16 - sec_off[0],
                                 (const struct qhuff_hstr *) (D + o.h.strs), n,
                                 max_len, t1 ? D + o.tab - t0 : nullptr, t1,
                                 D + o_out, (uint32_t *) (D + o_off),
                                 D + o_st, c->own_stream);
    if (r)
        return r;
    if (n && (name_hash || nameval_hash))
    {
        r = qhuff_xxh32_headers(c, D + o_out, (const uint32_t *) (D + o_off),
                                n, QHUFF_XXH_SEED, (uint32_t *) (D + o_h1),
                                (uint32_t *) (D + o_h2), c->own_stream);
        if (r)
            return r;
    }
    if ((r = stage_down(c, o.h.kind, o_off, o_out, 2 * n, out, off)))
        return r;
    if (n)
    {
        hdr_bytes_out(c, o.h, n, kind, static_id, hflags);
        if (dyn_id)
            memcpy(dyn_id, H + o.did, 4ull * n);
        memcpy(status, H + o_st, 2ull * n);
        if (name_hash)
            memcpy(name_hash, H + o_h1, 4ull * n);
        if (nameval_hash)
            memcpy(nameval_hash, H + o_h2, 4ull * n);
    }
    return QHUFF_OK;
}

// Items encoded in one launch (qhuff_encode_wire): the strings, their
// offsets and the items go up in one copy; one launch; the offsets come
// back, then exactly the out_off[n] bytes written.  Nothing is framed or
// spliced on the host: its only loop over the items is the rule's check.
// Stage layout: [strings | in_off | items | out_off | out]; the kernel reads
// the caller's offsets unchanged: `in` is passed rebased by -in_off[0].
extern "C" int
qhuff_encode_wire_host(qhuff_ctx *c, const uint8_t *in, const uint32_t *in_off,
                       const struct qhuff_item *items, uint32_t n,
                       uint8_t *out, uint32_t *out_off)
{
    if (!c || !out_off || (n && (!in || !in_off || !items || !out)))
        return QHUFF_EINVAL;
    if (qhuff_items_check(items, n, nullptr))
        return QHUFF_EINVAL;
    if (n == 0)
    {
        out_off[0] = 0;
        return QHUFF_OK;
    }
    if (in_off[n] < in_off[0])
        return QHUFF_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t a0 = in_off[0], bytes = (uint64_t) in_off[n] - a0;
    const uint64_t bound = qhuff_encode_wire_bound(bytes, n);
    if (bound > 0xffffffffull)
        return QHUFF_ERANGE;
    const size_t o_io = up16(bytes) + 16;
    const size_t o_it = o_io + up16(4ull * (n + 1));
    const size_t o_oo = o_it + up16(8ull * n);
    const size_t o_out = o_oo + up16(4ull * (n + 1));
    int rc = stage_up(c, o_out + up16(bound),
                      {{in + a0, bytes, 0}, {in_off, 4ull * (n + 1), o_io},
                       {items, 8ull * n, o_it}}, o_oo);
    if (rc)
        return rc;
    uint8_t *D = c->d_stage;
    rc = qhuff_encode_wire(c, D - a0, (const uint32_t *) (D + o_io),
                           (const struct qhuff_item *) (D + o_it), n,
                           D + o_out, (uint32_t *) (D + o_oo),
                           c->own_stream);
    if (rc)
        return rc;
    return stage_down(c, o_oo, o_oo, o_out, n, out, out_off);
}

// ---- header hashing, host buffers ----------------------------------------------

// Stage layout: [name/value bytes | offsets (2n + 1) | name_hash | nameval_hash].
// The kernel reads the caller's offsets unchanged: `in` is passed rebased by
// -off[0].
extern "C" int
qhuff_xxh32_headers_host(qhuff_ctx *c, const uint8_t *in, const uint32_t *off,
                         uint32_t n, uint32_t seed, uint32_t *name_hash,
                         uint32_t *nameval_hash)
{
    if (!c || !off || (n && (!in || !name_hash || !nameval_hash)))
        return QHUFF_EINVAL;
    if (n > 0x7fffffffu)
        return QHUFF_ERANGE;
    if (n == 0)
        return QHUFF_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t a0 = off[0], bytes = (uint64_t) off[2ull * n] - a0;
    const size_t o_off = up16(bytes), o_h1 = o_off + up16(4ull * (2ull * n + 1));
    const size_t o_h2 = o_h1 + up16(4ull * n), total = o_h2 + up16(4ull * n);
    int rc = stage_up(c, total, {{in + a0, bytes, 0},
                                 {off, 4ull * (2ull * n + 1), o_off}}, o_h1);
    if (rc)
        return rc;
    uint8_t *H = c->h_stage, *D = c->d_stage;
    hipStream_t st = c->own_stream;
    rc = qhuff_xxh32_headers(c, D - a0, (const uint32_t *) (D + o_off), n,
                             seed, (uint32_t *) (D + o_h1),
                             (uint32_t *) (D + o_h2), st);
    if (rc)
        return rc;
    HIPCHK(c, hipMemcpyAsync(H + o_h1, D + o_h1, total - o_h1,
                             hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    memcpy(name_hash, H + o_h1, 4ull * n);
    memcpy(nameval_hash, H + o_h2, 4ull * n);
    return QHUFF_OK;
}

// ---- headers against the static table, host buffers ----------------------------

// (the checks the host forms make of a header list: n within the pairs
// layout's range, offsets that do not decrease)
static int
headers_ok(const uint32_t *off, uint32_t n)
{
    if (n > 0x7fffffffu)
        return QHUFF_ERANGE;
    for (uint64_t i = 0; i < 2ull * n; ++i)
        if (off[i + 1] < off[i])
            return QHUFF_EINVAL;
    return QHUFF_OK;
}

// Stage layout: [name/value bytes | offsets (2n + 1) | name_hash |
// nameval_hash | kind | static_id]; `in` is passed rebased by -off[0].
extern "C" int
qhuff_static_lookup_host(qhuff_ctx *c, const uint8_t *in, const uint32_t *off,
                         uint32_t n, uint32_t *name_hash,
                         uint32_t *nameval_hash, uint8_t *kind,
                         uint8_t *static_id)
{
    if (!c || !off || (n && (!in || !kind || !static_id)))
        return QHUFF_EINVAL;
    if (const int rc = headers_ok(off, n))
        return rc;
    if (n == 0)
        return QHUFF_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t a0 = off[0], bytes = (uint64_t) off[2ull * n] - a0;
    const size_t o_off = up16(bytes) + 16;
    const size_t o_h1 = o_off + up16(4ull * (2ull * n + 1));
    const size_t o_h2 = o_h1 + up16(4ull * n), o_k = o_h2 + up16(4ull * n);
    const size_t o_id = o_k + up16(n), total = o_id + up16(n);
    int rc = stage_up(c, total, {{in + a0, bytes, 0},
                                 {off, 4ull * (2ull * n + 1), o_off}}, o_h1);
    if (rc)
        return rc;
    uint8_t *H = c->h_stage, *D = c->d_stage;
    hipStream_t st = c->own_stream;
    rc = qhuff_static_lookup(c, D - a0, (const uint32_t *) (D + o_off), n,
                             (uint32_t *) (D + o_h1), (uint32_t *) (D + o_h2),
                             D + o_k, D + o_id, st);
    if (rc)
        return rc;
    HIPCHK(c, hipMemcpyAsync(H + o_h1, D + o_h1, total - o_h1,
                             hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (name_hash)
        memcpy(name_hash, H + o_h1, 4ull * n);
    if (nameval_hash)
        memcpy(nameval_hash, H + o_h2, 4ull * n);
    memcpy(kind, H + o_k, n);
    memcpy(static_id, H + o_id, n);
    return QHUFF_OK;
}

// Header lists to field sections (qhuff_encode_headers): the bytes, their
// offsets, the flags and the sections' bounds go up in one copy; the
// launches; sec_out, kind and static_id come back, then exactly the
// sec_out[m] bytes written.  The host loops over the offsets and the
// sections' bounds only to check them.  Stage layout: [bytes | off | hflags |
// sec_hdr | sec_out | kind | static_id | out]; `in` is passed rebased by
// -off[0].
extern "C" int
qhuff_encode_headers_host(qhuff_ctx *c, const uint8_t *in, const uint32_t *off,
                          uint32_t n, const uint8_t *hflags,
                          const uint32_t *sec_hdr, uint32_t m, uint8_t *out,
                          uint32_t *sec_out, uint8_t *kind, uint8_t *static_id)
{
    if (!c || !off || !sec_hdr || !sec_out || (n && !in) || ((n || m) && !out))
        return QHUFF_EINVAL;
    if (2ull * n + 2ull * m > 0xffffffffull)
        return QHUFF_ERANGE;
    if (sec_hdr[0] != 0 || sec_hdr[m] != n)
        return QHUFF_EINVAL;
    for (uint32_t s = 0; s < m; ++s)
        if (sec_hdr[s + 1] < sec_hdr[s])
            return QHUFF_EINVAL;
    if (const int rc = headers_ok(off, n))
        return rc;
    if (m == 0)
    {
        sec_out[0] = 0;
        return QHUFF_OK;
    }
    const uint64_t a0 = off[0], bytes = (uint64_t) off[2ull * n] - a0;
    const uint64_t bound = qhuff_encode_headers_bound(bytes, n, m);
    if (bound > 0xffffffffull)
        return QHUFF_ERANGE;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t o_off = up16(bytes) + 16;
    const size_t o_fl = o_off + up16(4ull * (2ull * n + 1));
    const size_t o_sh = o_fl + up16(n);
    const size_t o_so = o_sh + up16(4ull * (m + 1ull));
    const size_t o_k = o_so + up16(4ull * (m + 1ull));
    const size_t o_id = o_k + up16(n), o_out = o_id + up16(n);
    int rc = stage_up(c, o_out + up16(bound),
                      {{bytes ? in + a0 : nullptr, bytes, 0},
                       {off, 4ull * (2ull * n + 1), o_off},
                       {hflags, hflags ? (size_t) n : 0, o_fl},
                       {sec_hdr, 4ull * (m + 1ull), o_sh}}, o_so);
    if (rc)
        return rc;
    uint8_t *D = c->d_stage;
    rc = qhuff_encode_headers(c, D - a0, (const uint32_t *) (D + o_off), n,
                              hflags ? D + o_fl : nullptr,
                              (const uint32_t *) (D + o_sh), m, D + o_out,
                              (uint32_t *) (D + o_so), D + o_k, D + o_id,
                              c->own_stream);
    if (rc)
        return rc;
    if ((rc = stage_down(c, o_so, o_so, o_out, m, out, sec_out)))
        return rc;
    if (kind && n)
        memcpy(kind, c->h_stage + o_k, n);
    if (static_id && n)
        memcpy(static_id, c->h_stage + o_id, n);
    return QHUFF_OK;
}

// ---- ... and among the dynamic table's entries, host buffers -------------------

// the table's part of a stage: its bytes (rebased by -off[0]) and its offsets
struct DynUp
{
    uint64_t t0, tb;                     // off[0], the bytes held
    size_t bytes, off;                   // where they lie in the stage
};

static DynUp
dyn_up(const struct qhuff_dyn_table *tab, size_t at)
{
    DynUp u;
    const uint64_t d = tab->d;
    u.t0 = d ? tab->off[0] : 0;
    u.tb = d ? tab->off[2 * d] - u.t0 : 0;
    u.bytes = at;
    u.off = at + up16(u.tb) + 16;
    return u;
}

static size_t
dyn_up_end(const struct qhuff_dyn_table *tab, const DynUp &u)
{
    return u.off + up16(tab->d ? 4 * (2ull * tab->d + 1) : 0);
}

// Stage layout: [name/value bytes | offsets (2n + 1) | table bytes | table
// off | name_hash | nameval_hash | dyn_id | kind | static_id]; `in` and the
// table's bytes are passed rebased by -off[0].
extern "C" int
qhuff_dyn_lookup_host(qhuff_ctx *c, const uint8_t *in, const uint32_t *off,
                      uint32_t n, const struct qhuff_dyn_table *tab,
                      uint32_t win_lo, uint32_t win_hi, uint32_t *name_hash,
                      uint32_t *nameval_hash, uint8_t *kind,
                      uint8_t *static_id, uint32_t *dyn_id)
{
    if (!c || !off || (n && (!in || !kind || !static_id)))
        return QHUFF_EINVAL;
    const uint32_t win[2] = {win_lo, win_hi};
    if (const int rc = dyn_enc_check(tab, win, nullptr, 1))
        return rc;
    if (const int rc = headers_ok(off, n))
        return rc;
    if (n == 0)
        return QHUFF_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t a0 = off[0], bytes = (uint64_t) off[2ull * n] - a0;
    const size_t o_off = up16(bytes) + 16;
    const DynUp u = dyn_up(tab, o_off + up16(4ull * (2ull * n + 1)));
    const size_t o_h1 = dyn_up_end(tab, u);
    const size_t o_h2 = o_h1 + up16(4ull * n), o_did = o_h2 + up16(4ull * n);
    const size_t o_k = o_did + up16(4ull * n);
    const size_t o_id = o_k + up16(n), total = o_id + up16(n);
    int rc = stage_up(c, total,
                      {{bytes ? in + a0 : nullptr, bytes, 0},
                       {off, 4ull * (2ull * n + 1), o_off},
                       {u.tb ? tab->bytes + u.t0 : nullptr, u.tb, u.bytes},
                       {tab->off, tab->d ? 4 * (2ull * tab->d + 1) : 0, u.off}},
                      o_h1);
    if (rc)
        return rc;
    uint8_t *H = c->h_stage, *D = c->d_stage;
    hipStream_t st = c->own_stream;
    struct qhuff_dyn_table dev = *tab;
    dev.bytes = D + u.bytes - u.t0;
    dev.off = tab->d ? (const uint32_t *) (D + u.off) : nullptr;
    rc = qhuff_dyn_lookup(c, D - a0, (const uint32_t *) (D + o_off), n, &dev,
                          win_lo, win_hi, (uint32_t *) (D + o_h1),
                          (uint32_t *) (D + o_h2), D + o_k, D + o_id,
                          (uint32_t *) (D + o_did), st);
    if (rc)
        return rc;
    HIPCHK(c, hipMemcpyAsync(H + o_h1, D + o_h1, total - o_h1,
                             hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (name_hash)
        memcpy(name_hash, H + o_h1, 4ull * n);
    if (nameval_hash)
        memcpy(nameval_hash, H + o_h2, 4ull * n);
    if (dyn_id)
        memcpy(dyn_id, H + o_did, 4ull * n);
    memcpy(kind, H + o_k, n);
    memcpy(static_id, H + o_id, n);
    return QHUFF_OK;
}

// Header lists to field sections against the table
// (qhuff_encode_headers_dyn), as qhuff_encode_headers_host: one upload of the
// headers and the table, the launches, then sec_out, the optional arrays and
// exactly sec_out[m] bytes come back.  The host loops over the offsets, the
// sections' bounds, the windows and the Bases only to check them.  Stage
// layout: [bytes | off | hflags | sec_hdr | table bytes | table off | sec_win
// | sec_base | sec_out | dyn_id | kind | static_id | out].
extern "C" int
qhuff_encode_headers_dyn_host(qhuff_ctx *c, const uint8_t *in,
                              const uint32_t *off, uint32_t n,
                              const uint8_t *hflags, const uint32_t *sec_hdr,
                              uint32_t m, const struct qhuff_dyn_table *tab,
                              const uint32_t *sec_win,
                              const uint32_t *sec_base, uint8_t *out,
                              uint32_t *sec_out, uint8_t *kind,
                              uint8_t *static_id, uint32_t *dyn_id)
{
    if (!c || !off || !sec_hdr || !sec_out || (n && !in) || ((n || m) && !out))
        return QHUFF_EINVAL;
    if (2ull * n + 2ull * m > 0xffffffffull)
        return QHUFF_ERANGE;
    if (sec_hdr[0] != 0 || sec_hdr[m] != n)
        return QHUFF_EINVAL;
    for (uint32_t s = 0; s < m; ++s)
        if (sec_hdr[s + 1] < sec_hdr[s])
            return QHUFF_EINVAL;
    if (const int rc = headers_ok(off, n))
        return rc;
    if (const int rc = dyn_enc_check(tab, sec_win, sec_base, m))
        return rc;
    if (m == 0)
    {
        sec_out[0] = 0;
        return QHUFF_OK;
    }
    const uint64_t a0 = off[0], bytes = (uint64_t) off[2ull * n] - a0;
    const uint64_t bound = qhuff_encode_headers_dyn_bound(bytes, n, m);
    if (bound > 0xffffffffull)
        return QHUFF_ERANGE;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t o_off = up16(bytes) + 16;
    const size_t o_fl = o_off + up16(4ull * (2ull * n + 1));
    const size_t o_sh = o_fl + up16(n);
    const DynUp u = dyn_up(tab, o_sh + up16(4ull * (m + 1ull)));
    const size_t o_sw = dyn_up_end(tab, u);
    const size_t o_sb = o_sw + up16(sec_win ? 8ull * m : 0);
    const size_t o_so = o_sb + up16(sec_base ? 4ull * m : 0);
    const size_t o_did = o_so + up16(4ull * (m + 1ull));
    const size_t o_k = o_did + up16(4ull * n);
    const size_t o_id = o_k + up16(n), o_out = o_id + up16(n);
    int rc = stage_up(c, o_out + up16(bound),
                      {{bytes ? in + a0 : nullptr, bytes, 0},
                       {off, 4ull * (2ull * n + 1), o_off},
                       {hflags, hflags ? (size_t) n : 0, o_fl},
                       {sec_hdr, 4ull * (m + 1ull), o_sh},
                       {u.tb ? tab->bytes + u.t0 : nullptr, u.tb, u.bytes},
                       {tab->off, tab->d ? 4 * (2ull * tab->d + 1) : 0, u.off},
                       {sec_win, sec_win ? 8ull * m : 0, o_sw},
                       {sec_base, sec_base ? 4ull * m : 0, o_sb}}, o_so);
    if (rc)
        return rc;
    uint8_t *D = c->d_stage;
    struct qhuff_dyn_table dev = *tab;
    dev.bytes = D + u.bytes - u.t0;
    dev.off = tab->d ? (const uint32_t *) (D + u.off) : nullptr;
    rc = qhuff_encode_headers_dyn(c, D - a0, (const uint32_t *) (D + o_off), n,
                                  hflags ? D + o_fl : nullptr,
                                  (const uint32_t *) (D + o_sh), m, &dev,
                                  sec_win ? (const uint32_t *) (D + o_sw)
                                          : nullptr,
                                  sec_base ? (const uint32_t *) (D + o_sb)
                                           : nullptr,
                                  D + o_out, (uint32_t *) (D + o_so), D + o_k,
                                  D + o_id, (uint32_t *) (D + o_did),
                                  c->own_stream);
    if (rc)
        return rc;
    if ((rc = stage_down(c, o_so, o_so, o_out, m, out, sec_out)))
        return rc;
    if (kind && n)
        memcpy(kind, c->h_stage + o_k, n);
    if (static_id && n)
        memcpy(static_id, c->h_stage + o_id, n);
    if (dyn_id && n)
        memcpy(dyn_id, c->h_stage + o_did, 4ull * n);
    return QHUFF_OK;
}

// ---- ... over a set of tables, a table per section, host buffers ---------------

// a set's part of a stage: the shared bytes (rebased by -off[0]), the
// offsets, then the small arrays ent, first and max_entries
struct TabsUp
{
    uint64_t t0, tb;                     // off[0], the bytes held
    size_t bytes, off, ent, first, me, end;
    uint32_t D;
};

static TabsUp
tabs_up(const struct qhuff_dyn_tables *t, uint32_t D, size_t at)
{
    TabsUp u;
    const uint64_t T = t->T;
    u.D = D;
    u.t0 = D ? t->off[0] : 0;
    u.tb = D ? t->off[2ull * D] - u.t0 : 0;
    u.bytes = at;
    u.off = at + up16(u.tb) + 16;
    u.ent = u.off + up16(D ? 4 * (2ull * D + 1) : 0);
    u.first = u.ent + up16(T ? 4 * (T + 1) : 0);
    u.me = u.first + up16(4 * T);
    u.end = u.me + up16(4 * T);
    return u;
}

// the set as the device-pointer calls read it from the stage at D
static struct qhuff_dyn_tables
tabs_dev(const struct qhuff_dyn_tables *t, const TabsUp &u, uint8_t *D)
{
    struct qhuff_dyn_tables dev = *t;
    dev.bytes = D + u.bytes - u.t0;
    dev.off = t->T ? (const uint32_t *) (D + u.off) : nullptr;
    dev.ent = t->T ? (const uint32_t *) (D + u.ent) : nullptr;
    dev.first = t->T ? (const uint32_t *) (D + u.first) : nullptr;
    dev.max_entries = t->T ? (const uint32_t *) (D + u.me) : nullptr;
    return dev;
}

#define TABS_STAGE_IN(t, u)                                                  \
    {(u).tb ? (t)->bytes + (u).t0 : nullptr, (size_t) (u).tb, (u).bytes},    \
    {(t)->off, (u).D ? (size_t) (4 * (2ull * (u).D + 1)) : 0, (u).off},      \
    {(t)->ent, (t)->T ? (size_t) (4 * ((t)->T + 1ull)) : 0, (u).ent},        \
    {(t)->first, (size_t) (4ull * (t)->T), (u).first},                       \
    {(t)->max_entries, (size_t) (4ull * (t)->T), (u).me}

// dyn_staged with a set of tables: the set, the sections' tables and the
// windows go up with the wire bytes.  Stage layout: [16 | wire bytes | 16 |
// sec_off | the set (TabsUp) | sec_tab | sec_win | hdr_off | rc | strs | kind
// | static_id | hflags | dyn_id], the last five sized for max_hdrs; `extra`
// more bytes are kept behind them, from o->h.end.
static int
tabs_staged(qhuff_ctx *c, const uint8_t *buf, const uint32_t *sec_off,
            uint32_t m, const struct qhuff_dyn_tables *tabs, uint32_t D_all,
            const uint32_t *sec_tab, const uint32_t *sec_win,
            uint32_t max_hdrs, uint32_t *hdr_off, int32_t *rc, uint64_t extra,
            DynStage *o)
{
    const uint64_t a0 = sec_off[0], bytes = (uint64_t) sec_off[m] - a0;
    const size_t o_so = up16(16 + bytes) + 16;
    const TabsUp u = tabs_up(tabs, D_all, o_so + up16(4ull * (m + 1)));
    const bool st = tabs->T != 0;
    o->tab = u.bytes;
    const size_t o_st = u.end;
    const size_t o_sw = o_st + up16(st ? 4ull * m : 0);
    const size_t o_ho = o_sw + up16(sec_win ? 8ull * m : 0);
    const size_t o_rc = o_ho + up16(4ull * (m + 1));
    o->h.strs = o_rc + up16(4ull * m);
    o->h.kind = o->h.strs + 32ull * max_hdrs;
    o->h.id = o->h.kind + up16(max_hdrs);
    o->h.hf = o->h.id + up16(max_hdrs);
    o->did = o->h.hf + up16(max_hdrs);
    o->h.end = o->did + up16(4ull * max_hdrs);
    int r = stage_up(c, o->h.end + extra,
                     {{buf + a0, bytes, 16}, {sec_off, 4ull * (m + 1), o_so},
                      TABS_STAGE_IN(tabs, u),
                      {sec_tab, st ? 4ull * m : 0, o_st},
                      {sec_win, sec_win ? 8ull * m : 0, o_sw}},
                     o_ho);
    if (r)
        return r;
    uint8_t *H = c->h_stage, *D = c->d_stage;
    const struct qhuff_dyn_tables dev = tabs_dev(tabs, u, D);
    r = qhuff_scan_headers_tabs(c, D + 16 - a0, (const uint32_t *) (D + o_so),
                                m, &dev,
                                st ? (const uint32_t *) (D + o_st) : nullptr,
                                sec_win ? (const uint32_t *) (D + o_sw)
                                        : nullptr,
                                (struct qhuff_hstr *) (D + o->h.strs),
                                max_hdrs, (uint32_t *) (D + o_ho),
                                (int32_t *) (D + o_rc), D + o->h.kind,
                                D + o->h.id, D + o->h.hf,
                                (uint32_t *) (D + o->did), c->own_stream);
    if (r)
        return r;
    HIPCHK(c, hipMemcpyAsync(H + o_ho, D + o_ho, o->h.strs - o_ho,
                             hipMemcpyDeviceToHost, c->own_stream));
    HIPCHK(c, hipStreamSynchronize(c->own_stream));
    memcpy(hdr_off, H + o_ho, 4ull * (m + 1));
    memcpy(rc, H + o_rc, 4ull * m);
    return QHUFF_OK;
}

extern "C" int
qhuff_scan_headers_tabs_host(qhuff_ctx *c, const uint8_t *buf,
                             const uint32_t *sec_off, uint32_t m,
                             const struct qhuff_dyn_tables *tabs,
                             const uint32_t *sec_tab, const uint32_t *sec_win,
                             struct qhuff_hstr *strs, uint32_t max_hdrs,
                             uint32_t *hdr_off, int32_t *rc, uint8_t *kind,
                             uint8_t *static_id, uint8_t *hflags,
                             uint32_t *dyn_id)
{
    if (!hdr_args_ok(c, buf, sec_off, m, hdr_off, rc) || (max_hdrs && !strs))
        return QHUFF_EINVAL;
    uint32_t D_all, longest;
    if (const int r = tabs_check(tabs, sec_tab, sec_win, nullptr, m, false,
                                 &D_all, &longest))
        return r;
    if (m == 0)
    {
        hdr_off[0] = 0;
        return QHUFF_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    DynStage o;
    int r = tabs_staged(c, buf, sec_off, m, tabs, D_all, sec_tab, sec_win,
                        max_hdrs, hdr_off, rc, 0, &o);
    if (r)
        return r;
    const uint32_t n = hdr_off[m] < max_hdrs ? hdr_off[m] : max_hdrs;
    if (n)
    {
        uint8_t *H = c->h_stage, *D = c->d_stage;
        HIPCHK(c, hipMemcpyAsync(H + o.h.strs, D + o.h.strs, 32ull * n,
                                 hipMemcpyDeviceToHost, c->own_stream));
        HIPCHK(c, hipMemcpyAsync(H + o.h.kind, D + o.h.kind,
                                 o.did + 4ull * n - o.h.kind,
                                 hipMemcpyDeviceToHost, c->own_stream));
        HIPCHK(c, hipStreamSynchronize(c->own_stream));
        memcpy(strs, H + o.h.strs, 32ull * n);
        hdr_bytes_out(c, o.h, n, kind, static_id, hflags);
        if (dyn_id)
            memcpy(dyn_id, H + o.did, 4ull * n);
    }
    return hdr_off[m] > max_hdrs ? QHUFF_ERANGE : QHUFF_OK;
}

// The whole path, as qhuff_decode_headers_dyn_host: tabs_staged, then
// qhuff_decode_headers_dyn unchanged on the descriptors and on the shared
// bytes where they lie.
extern "C" int
qhuff_decode_headers_tabs_host(qhuff_ctx *c, const uint8_t *buf,
                               const uint32_t *sec_off, uint32_t m,
                               const struct qhuff_dyn_tables *tabs,
                               const uint32_t *sec_tab,
                               const uint32_t *sec_win, uint32_t max_len,
                               uint32_t max_hdrs, uint32_t *hdr_off,
                               int32_t *rc, uint8_t *kind, uint8_t *static_id,
                               uint8_t *hflags, uint32_t *dyn_id, uint8_t *out,
                               uint32_t *off, uint8_t *status,
                               uint32_t *name_hash, uint32_t *nameval_hash)
{
    if (!off || !hdr_args_ok(c, buf, sec_off, m, hdr_off, rc)
            || (max_hdrs && (!out || !status)))
        return QHUFF_EINVAL;
    if (max_hdrs > 0x7fffffffu)
        return QHUFF_ERANGE;
    uint32_t D_all, longest;
    if (const int r = tabs_check(tabs, sec_tab, sec_win, nullptr, m, false,
                                 &D_all, &longest))
        return r;
    if (m == 0)
    {
        hdr_off[0] = 0;
        off[0] = 0;
        return QHUFF_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t bytes = (uint64_t) sec_off[m] - sec_off[0];
    const uint64_t bound = qhuff_decode_headers_dyn_bound(bytes, max_hdrs,
                                                          longest);
    if (bound > 0xffffffffull)
        return QHUFF_ERANGE;
    const uint64_t mh = max_hdrs;
    DynStage o;
    int r = tabs_staged(c, buf, sec_off, m, tabs, D_all, sec_tab, sec_win,
                        max_hdrs, hdr_off, rc,
                        up16(4 * (2 * mh + 1)) + up16(2 * mh)
                            + 2 * up16(4 * mh) + up16(bound),
                        &o);
    if (r)
        return r;
    const uint32_t n = hdr_off[m];
    if (n > max_hdrs)
        return QHUFF_ERANGE;
    const size_t o_off = o.h.end;
    const size_t o_st = o_off + up16(4 * (2ull * n + 1));
    const size_t o_h1 = o_st + up16(2ull * n);
    const size_t o_h2 = o_h1 + up16(4ull * n);
    const size_t o_out = o_h2 + up16(4ull * n);
    uint8_t *H = c->h_stage, *D = c->d_stage;
    const uint32_t t0 = D_all ? tabs->off[0] : 0;
    const uint32_t t1 = D_all ? tabs->off[2ull * D_all] : 0;
    // (dyn_bytes rebased as the scan's: instr is an offset from tabs->bytes)
    r = qhuff_decode_headers_dyn(c, D + 16 - sec_off[0],
                                 (const struct qhuff_hstr *) (D + o.h.strs), n,
                                 max_len, t1 ? D + o.tab - t0 : nullptr, t1,
                                 D + o_out, (uint32_t *) (D + o_off),
                                 D + o_st, c->own_stream);
    if (r)
        return r;
    if (n && (name_hash || nameval_hash))
    {
        r = qhuff_xxh32_headers(c, D + o_out, (const uint32_t *) (D + o_off),
                                n, QHUFF_XXH_SEED, (uint32_t *) (D + o_h1),
                                (uint32_t *) (D + o_h2), c->own_stream);
        if (r)
            return r;
    }
    if ((r = stage_down(c, o.h.kind, o_off, o_out, 2 * n, out, off)))
        return r;
    if (n)
    {
        hdr_bytes_out(c, o.h, n, kind, static_id, hflags);
        if (dyn_id)
            memcpy(dyn_id, H + o.did, 4ull * n);
        memcpy(status, H + o_st, 2ull * n);
        if (name_hash)
            memcpy(name_hash, H + o_h1, 4ull * n);
        if (nameval_hash)
            memcpy(nameval_hash, H + o_h2, 4ull * n);
    }
    return QHUFF_OK;
}

// ---- encoder-stream inserts applied to a set of tables, host buffers ---------

// The whole path: the wire bytes, the set and its state go up once; the scan
// runs and its small results come back (n = ins_off[T]); the apply runs on
// the descriptors where they are; the per-insert arrays, the next set's small
// arrays and offsets come back, then exactly its bytes.  Stage layout: [16 |
// wire bytes | 16 | enc_off | the set (TabsUp) | cap | max_cap | live_lo | keep
// | rc | consumed | ins_off | chunk_cap | ins_ref | ins_kind | strs | root |
// ins_cap | ins_lo | out_ent | out_first | cap_out | live_lo_out | out_off |
// out_bytes], the per-insert parts sized for max_ins.
extern "C" int
qhuff_tabs_insert_host(qhuff_ctx *c, const struct qhuff_dyn_tables *tabs,
                       const struct qhuff_ins_state *s, const uint8_t *buf,
                       const uint32_t *enc_off, const uint32_t *keep,
                       const struct qhuff_ins_scan *sc,
                       const struct qhuff_ins_out *o)
{
    if (!c)
        return QHUFF_EINVAL;
    uint32_t D_all, longest;
    if (const int r = ins::check(tabs, s, buf, enc_off, sc, o, &D_all,
                                 &longest))
        return r;
    const uint64_t T = tabs->T, mi = sc->max_ins;
    if (T == 0)
    {
        sc->ins_off[0] = 0;
        o->out_ent[0] = 0;
        o->out_off[0] = 0;
        return QHUFF_OK;
    }
    const uint64_t a0 = enc_off[0], wire = (uint64_t) enc_off[T] - a0;
    const uint64_t arena = D_all ? tabs->off[2ull * D_all] : 0;
    const uint64_t bound = qhuff_tabs_insert_bound(arena, wire, sc->max_ins,
                                                   longest);
    if (bound > 0xffffffffull || D_all + mi > 0x7fffffffull)
        return QHUFF_ERANGE;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t o_eo = up16(16 + wire) + 16;
    const TabsUp u = tabs_up(tabs, D_all, o_eo + up16(4 * (T + 1)));
    const size_t o_cap = u.end;
    const size_t o_mc = o_cap + up16(4 * T);
    const size_t o_ll = o_mc + up16(4 * T);
    const size_t o_keep = o_ll + up16(4 * T);
    const size_t o_rc = o_keep + up16(keep ? 4 * T : 0);
    const size_t o_cons = o_rc + up16(4 * T);
    const size_t o_io = o_cons + up16(4 * T);
    const size_t o_cc = o_io + up16(4 * (T + 1));
    const size_t o_ref = o_cc + up16(8 * T);
    const size_t o_kind = o_ref + up16(4 * mi);
    const size_t o_strs = o_kind + up16(mi);
    const size_t o_root = o_strs + 32 * mi;
    const size_t o_icap = o_root + up16(8 * mi);
    const size_t o_lo = o_icap + up16(8 * mi);
    const size_t o_oe = o_lo + up16(4 * mi);
    const size_t o_of = o_oe + up16(4 * (T + 1));
    const size_t o_co = o_of + up16(4 * T);
    const size_t o_lo2 = o_co + up16(4 * T);
    const size_t o_oo = o_lo2 + up16(4 * T);
    const size_t o_ob = o_oo + up16(4 * (2 * (D_all + mi) + 1));
    int r = stage_up(c, o_ob + up16(bound),
                     {{buf + a0, (size_t) wire, 16},
                      {enc_off, (size_t) (4 * (T + 1)), o_eo},
                      TABS_STAGE_IN(tabs, u),
                      {s->cap, (size_t) (4 * T), o_cap},
                      {s->max_cap, (size_t) (4 * T), o_mc},
                      {s->live_lo, (size_t) (4 * T), o_ll},
                      {keep, keep ? (size_t) (4 * T) : 0, o_keep}},
                     o_rc);
    if (r)
        return r;
    uint8_t *H = c->h_stage, *Dv = c->d_stage;
    hipStream_t sk = c->own_stream;
    const struct qhuff_dyn_tables dev = tabs_dev(tabs, u, Dv);
    struct qhuff_ins_state ds;
    ds.cap = (const uint32_t *) (Dv + o_cap);
    ds.max_cap = (const uint32_t *) (Dv + o_mc);
    ds.live_lo = (const uint32_t *) (Dv + o_ll);
    ds.arena_bytes = (uint32_t) arena;
    ds.dyn_longest = longest;
    struct qhuff_ins_scan dsc;
    dsc.rc = (int32_t *) (Dv + o_rc);
    dsc.consumed = (uint32_t *) (Dv + o_cons);
    dsc.ins_off = (uint32_t *) (Dv + o_io);
    dsc.chunk_cap = (uint32_t *) (Dv + o_cc);
    dsc.strs = (struct qhuff_hstr *) (Dv + o_strs);
    dsc.root = (uint32_t *) (Dv + o_root);
    dsc.ins_cap = (uint32_t *) (Dv + o_icap);
    dsc.ins_ref = (uint32_t *) (Dv + o_ref);
    dsc.ins_kind = Dv + o_kind;
    dsc.max_ins = sc->max_ins;
    r = qhuff_scan_inserts_tabs(c, &dev, &ds, Dv + 16 - a0,
                                (const uint32_t *) (Dv + o_eo), &dsc, sk);
    if (r)
        return r;
    HIPCHK(c, hipMemcpyAsync(H + o_rc, Dv + o_rc, o_ref - o_rc,
                             hipMemcpyDeviceToHost, sk));
    HIPCHK(c, hipStreamSynchronize(sk));
    memcpy(sc->rc, H + o_rc, 4 * T);
    memcpy(sc->consumed, H + o_cons, 4 * T);
    memcpy(sc->ins_off, H + o_io, 4 * (T + 1));
    if (sc->chunk_cap)
        memcpy(sc->chunk_cap, H + o_cc, 8 * T);
    const uint64_t total = sc->ins_off[T], n = total < mi ? total : mi;
    auto scan_out = [&]() {
        if (!n)
            return;
        memcpy(sc->ins_ref, H + o_ref, 4 * n);
        memcpy(sc->ins_kind, H + o_kind, n);
        if (sc->strs)
            memcpy(sc->strs, H + o_strs, 32 * n);
        if (sc->root)
            memcpy(sc->root, H + o_root, 8 * n);
        if (sc->ins_cap)
            memcpy(sc->ins_cap, H + o_icap, 8 * n);
    };
    r = total > mi ? QHUFF_ERANGE : ins::check_counts(tabs, sc->ins_off);
    if (r)
    {
        // (the scan's convention: the first max_ins inserts' scan results)
        if (n)
        {
            HIPCHK(c, hipMemcpyAsync(H + o_ref, Dv + o_ref, o_lo - o_ref,
                                     hipMemcpyDeviceToHost, sk));
            HIPCHK(c, hipStreamSynchronize(sk));
        }
        scan_out();
        return r;
    }
    struct qhuff_ins_out dout;
    dout.ins_lo = (uint32_t *) (Dv + o_lo);
    dout.out_bytes = Dv + o_ob;
    dout.out_off = (uint32_t *) (Dv + o_oo);
    dout.out_ent = (uint32_t *) (Dv + o_oe);
    dout.out_first = (uint32_t *) (Dv + o_of);
    dout.cap_out = (uint32_t *) (Dv + o_co);
    dout.live_lo_out = (uint32_t *) (Dv + o_lo2);
    dout.out_cap = bound;
    dout.ent_cap = (uint32_t) (D_all + mi);
    r = qhuff_apply_inserts_tabs(c, &dev, &ds, Dv + 16 - a0, (uint32_t) wire,
                                 keep ? (const uint32_t *) (Dv + o_keep)
                                      : nullptr,
                                 &dsc, (uint32_t) n, &dout, sk);
    if (r)
        return r;
    HIPCHK(c, hipMemcpyAsync(H + o_rc, Dv + o_rc, o_ob - o_rc,
                             hipMemcpyDeviceToHost, sk));
    HIPCHK(c, hipStreamSynchronize(sk));
    if (const int e = mirror_error(c))
        return e;
    memcpy(sc->rc, H + o_rc, 4 * T);
    memcpy(sc->consumed, H + o_cons, 4 * T);
    scan_out();
    if (n)
        memcpy(o->ins_lo, H + o_lo, 4 * n);
    memcpy(o->out_ent, H + o_oe, 4 * (T + 1));
    memcpy(o->out_first, H + o_of, 4 * T);
    memcpy(o->cap_out, H + o_co, 4 * T);
    memcpy(o->live_lo_out, H + o_lo2, 4 * T);
    const uint64_t De = o->out_ent[T];
    if (De > o->ent_cap || De > D_all + mi)
        return QHUFF_EINVAL;             // (out_off too small for the set)
    memcpy(o->out_off, H + o_oo, 4 * (2 * De + 1));
    const uint64_t bytes = o->out_off[2 * De];
    if (bytes > o->out_cap)
        return QHUFF_EINVAL;
    if (bytes)
    {
        HIPCHK(c, hipMemcpyAsync(H + o_ob, Dv + o_ob, bytes,
                                 hipMemcpyDeviceToHost, sk));
        HIPCHK(c, hipStreamSynchronize(sk));
        memcpy(o->out_bytes, H + o_ob, bytes);
    }
    return QHUFF_OK;
}

// the checks the section-wise host forms make of sec_hdr
static int
sections_ok(const uint32_t *sec_hdr, uint32_t m, uint32_t n)
{
    if (sec_hdr[0] != 0 || sec_hdr[m] != n)
        return QHUFF_EINVAL;
    for (uint32_t s = 0; s < m; ++s)
        if (sec_hdr[s + 1] < sec_hdr[s])
            return QHUFF_EINVAL;
    return QHUFF_OK;
}

// Stage layout: [name/value bytes | offsets (2n + 1) | sec_hdr | the set |
// sec_tab | sec_win | name_hash | nameval_hash | dyn_id | kind | static_id].
extern "C" int
qhuff_dyn_lookup_tabs_host(qhuff_ctx *c, const uint8_t *in,
                           const uint32_t *off, uint32_t n,
                           const uint32_t *sec_hdr, uint32_t m,
                           const struct qhuff_dyn_tables *tabs,
                           const uint32_t *sec_tab, const uint32_t *sec_win,
                           uint32_t *name_hash, uint32_t *nameval_hash,
                           uint8_t *kind, uint8_t *static_id, uint32_t *dyn_id)
{
    if (!c || !off || !sec_hdr || (n && (!in || !kind || !static_id)))
        return QHUFF_EINVAL;
    if (n > 0x7fffffffu)
        return QHUFF_ERANGE;
    if (const int rc = sections_ok(sec_hdr, m, n))
        return rc;
    if (const int rc = headers_ok(off, n))
        return rc;
    uint32_t D_all, longest;
    if (const int rc = tabs_check(tabs, sec_tab, sec_win, nullptr, m, true,
                                  &D_all, &longest))
        return rc;
    if (n == 0)
        return QHUFF_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const bool stb = tabs->T != 0;
    const uint64_t a0 = off[0], bytes = (uint64_t) off[2ull * n] - a0;
    const size_t o_off = up16(bytes) + 16;
    const size_t o_sh = o_off + up16(4ull * (2ull * n + 1));
    const TabsUp u = tabs_up(tabs, D_all, o_sh + up16(4ull * (m + 1ull)));
    const size_t o_st = u.end;
    const size_t o_sw = o_st + up16(stb ? 4ull * m : 0);
    const size_t o_h1 = o_sw + up16(sec_win ? 8ull * m : 0);
    const size_t o_h2 = o_h1 + up16(4ull * n), o_did = o_h2 + up16(4ull * n);
    const size_t o_k = o_did + up16(4ull * n);
    const size_t o_id = o_k + up16(n), total = o_id + up16(n);
    int rc = stage_up(c, total,
                      {{bytes ? in + a0 : nullptr, bytes, 0},
                       {off, 4ull * (2ull * n + 1), o_off},
                       {sec_hdr, 4ull * (m + 1ull), o_sh},
                       TABS_STAGE_IN(tabs, u),
                       {sec_tab, stb ? 4ull * m : 0, o_st},
                       {sec_win, sec_win ? 8ull * m : 0, o_sw}},
                      o_h1);
    if (rc)
        return rc;
    uint8_t *H = c->h_stage, *D = c->d_stage;
    hipStream_t st = c->own_stream;
    const struct qhuff_dyn_tables dev = tabs_dev(tabs, u, D);
    rc = tabs_lookup_dev(c, D - a0, (const uint32_t *) (D + o_off), n,
                         (const uint32_t *) (D + o_sh), m, &dev, D_all,
                         stb ? (const uint32_t *) (D + o_st) : nullptr,
                         sec_win ? (const uint32_t *) (D + o_sw) : nullptr,
                         (uint32_t *) (D + o_h1), (uint32_t *) (D + o_h2),
                         D + o_k, D + o_id, (uint32_t *) (D + o_did), st);
    if (rc)
        return rc;
    HIPCHK(c, hipMemcpyAsync(H + o_h1, D + o_h1, total - o_h1,
                             hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (name_hash)
        memcpy(name_hash, H + o_h1, 4ull * n);
    if (nameval_hash)
        memcpy(nameval_hash, H + o_h2, 4ull * n);
    if (dyn_id)
        memcpy(dyn_id, H + o_did, 4ull * n);
    memcpy(kind, H + o_k, n);
    memcpy(static_id, H + o_id, n);
    return QHUFF_OK;
}

// Header lists to field sections against a set of tables
// (qhuff_encode_headers_tabs), as qhuff_encode_headers_dyn_host.  Stage
// layout: [bytes | off | hflags | sec_hdr | the set | sec_tab | sec_win |
// sec_base | sec_out | dyn_id | kind | static_id | out].
extern "C" int
qhuff_encode_headers_tabs_host(qhuff_ctx *c, const uint8_t *in,
                               const uint32_t *off, uint32_t n,
                               const uint8_t *hflags, const uint32_t *sec_hdr,
                               uint32_t m, const struct qhuff_dyn_tables *tabs,
                               const uint32_t *sec_tab,
                               const uint32_t *sec_win,
                               const uint32_t *sec_base, uint8_t *out,
                               uint32_t *sec_out, uint8_t *kind,
                               uint8_t *static_id, uint32_t *dyn_id)
{
    if (!c || !off || !sec_hdr || !sec_out || (n && !in) || ((n || m) && !out))
        return QHUFF_EINVAL;
    if (2ull * n + 2ull * m > 0xffffffffull)
        return QHUFF_ERANGE;
    if (const int rc = sections_ok(sec_hdr, m, n))
        return rc;
    if (const int rc = headers_ok(off, n))
        return rc;
    uint32_t D_all, longest;
    if (const int rc = tabs_check(tabs, sec_tab, sec_win, sec_base, m, true,
                                  &D_all, &longest))
        return rc;
    if (m == 0)
    {
        sec_out[0] = 0;
        return QHUFF_OK;
    }
    const uint64_t a0 = off[0], bytes = (uint64_t) off[2ull * n] - a0;
    const uint64_t bound = qhuff_encode_headers_bound(bytes, n, m);
    if (bound > 0xffffffffull)
        return QHUFF_ERANGE;
    HIPCHK(c, hipSetDevice(c->device));
    const bool stb = tabs->T != 0;
    const size_t o_off = up16(bytes) + 16;
    const size_t o_fl = o_off + up16(4ull * (2ull * n + 1));
    const size_t o_sh = o_fl + up16(n);
    const TabsUp u = tabs_up(tabs, D_all, o_sh + up16(4ull * (m + 1ull)));
    const size_t o_st = u.end;
    const size_t o_sw = o_st + up16(stb ? 4ull * m : 0);
    const size_t o_sb = o_sw + up16(sec_win ? 8ull * m : 0);
    const size_t o_so = o_sb + up16(sec_base ? 4ull * m : 0);
    const size_t o_did = o_so + up16(4ull * (m + 1ull));
    const size_t o_k = o_did + up16(4ull * n);
    const size_t o_id = o_k + up16(n), o_out = o_id + up16(n);
    int rc = stage_up(c, o_out + up16(bound),
                      {{bytes ? in + a0 : nullptr, bytes, 0},
                       {off, 4ull * (2ull * n + 1), o_off},
                       {hflags, hflags ? (size_t) n : 0, o_fl},
                       {sec_hdr, 4ull * (m + 1ull), o_sh},
                       TABS_STAGE_IN(tabs, u),
                       {sec_tab, stb ? 4ull * m : 0, o_st},
                       {sec_win, sec_win ? 8ull * m : 0, o_sw},
                       {sec_base, sec_base ? 4ull * m : 0, o_sb}}, o_so);
    if (rc)
        return rc;
    uint8_t *D = c->d_stage;
    hipStream_t st = c->own_stream;
    const struct qhuff_dyn_tables dev = tabs_dev(tabs, u, D);
    if (n == 0)
        rc = qhuff_encode_headers_tabs(
            c, D - a0, (const uint32_t *) (D + o_off), n, nullptr,
            (const uint32_t *) (D + o_sh), m, &dev,
            stb ? (const uint32_t *) (D + o_st) : nullptr, nullptr, nullptr,
            D + o_out, (uint32_t *) (D + o_so), D + o_k, D + o_id,
            (uint32_t *) (D + o_did), st);
    else
        rc = tabs_encode_dev(c, D - a0, (const uint32_t *) (D + o_off), n,
                             hflags ? D + o_fl : nullptr,
                             (const uint32_t *) (D + o_sh), m, &dev, D_all,
                             stb ? (const uint32_t *) (D + o_st) : nullptr,
                             sec_win ? (const uint32_t *) (D + o_sw) : nullptr,
                             sec_base ? (const uint32_t *) (D + o_sb)
                                      : nullptr,
                             D + o_out, (uint32_t *) (D + o_so), D + o_k,
                             D + o_id, (uint32_t *) (D + o_did), st);
    if (rc)
        return rc;
    if ((rc = stage_down(c, o_so, o_so, o_out, m, out, sec_out)))
        return rc;
    if (kind && n)
        memcpy(kind, c->h_stage + o_k, n);
    if (static_id && n)
        memcpy(static_id, c->h_stage + o_id, n);
    if (dyn_id && n)
        memcpy(dyn_id, c->h_stage + o_did, 4ull * n);
    return QHUFF_OK;
}

// ---- per-string mirrors -----------------------------------------------------

extern "C" int
qhuff_enc_enc_str(qhuff_ctx *c, unsigned prefix_bits, unsigned char *dst,
                  size_t dst_len, const unsigned char *str, unsigned str_len)
{
    if (!c || !dst || (!str && str_len) || (prefix_bits != 3
            && prefix_bits != 5 && prefix_bits != 7))
        return -1;
    uint32_t off[2] = {0, str_len};
    uint64_t bound = qhuff_encode_bound(str_len, 1, prefix_bits);
    unsigned char *tmp = (unsigned char *) malloc(bound);
    unsigned char dummy = 0;
    uint32_t oo[2];
    if (!tmp)
        return -1;
    int rc = qhuff_encode_batch_host(c, str_len ? str : &dummy, off, 1,
                                     prefix_bits, tmp, oo);
    int r = -1;
    if (rc == QHUFF_OK && oo[1] <= dst_len)
    {
        // keep dst[0] bits above the H bit (lsqpack.c:852, 863)
        unsigned char keep = dst[0] & (unsigned char) ~((1u << (prefix_bits + 1)) - 1);
        memcpy(dst, tmp, oo[1]);
        dst[0] |= keep;
        r = (int) oo[1];
    }
    free(tmp);
    return r;
}

extern "C" unsigned
qhuff_enc_str_size(qhuff_ctx *c, const unsigned char *str, unsigned str_len)
{
    if (!c || (!str && str_len))
        return 0;
    uint32_t off[2] = {0, str_len};
    uint64_t bound = qhuff_encode_bound(str_len, 1, 0);
    unsigned char *tmp = (unsigned char *) malloc(bound);
    unsigned char dummy = 0;
    uint32_t oo[2] = {0, 0};
    if (!tmp)
        return 0;
    int rc = qhuff_encode_batch_host(c, str_len ? str : &dummy, off, 1, 0, tmp,
                                     oo);
    free(tmp);
    return rc == QHUFF_OK ? oo[1] : 0;
}

// qhuff_huff_decode_ex (lsqpack_huff_decode with its full signature): see
// qhuff_shim.cpp
