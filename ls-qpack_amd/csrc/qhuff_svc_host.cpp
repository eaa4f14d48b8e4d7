// qhuff_svc_host.cpp -- host half of the resident service: qhuff_svc_*.
#include "qhuff_ctx.h"

// ---- low-latency service (qhuff_service.hip) -----------------------------------
//
// The resident kernel's request slots live in pinned, device-mapped host
// memory (fine-grained: the device's loads and stores of a slot go over PCIe
// and are coherent with the host's).  A call takes a free slot, writes the
// rebased offsets, the bytes and the header, then the request sequence
// number (release); it spins on the slot's done word (acquire), copies the
// results out and frees the slot.  The kernel is (re)started on demand: at
// the first call, and by a waiting call that finds the service stream idle
// (the waves leave after idle_us without requests).

struct qhuff_svc
{
    qhuff_ctx *ctx;
    hipStream_t stream;              // the resident kernel's own stream
    uint8_t *slots_h, *slots_d;      // pinned slots, host / device views
    uint32_t *ctl_h, *ctl_d;         // pinned control word: [0] stop
    uint8_t *scratch;                // device: kSvcScratchBytes per slot
    uint64_t *active;                // device: last serve time (100 MHz)
    uint32_t n_slots, grid;
    uint64_t idle_ticks, life_ticks;
    std::atomic<uint32_t> *busy;     // per slot: 0 free, 1 taken
    uint32_t *seq;                   // per slot: last posted sequence
    std::atomic<uint32_t> next_slot{0};
    std::mutex launch_mu;            // (re)launch of the kernel
    std::mutex fallback_mu;          // large requests: the context's host path
    std::atomic<uint64_t> served{0}, launches{0}, fallbacks{0};
    // steady-clock ns of the last answered request: within idle_us / 2 of
    // it the kernel cannot have left for idle, and a call skips the stream
    // query (a lock in the HIP runtime every caller would queue on)
    std::atomic<int64_t> last_done_ns{0};
    int64_t fresh_ns;
};

static inline int64_t
steady_ns()
{
    return std::chrono::duration_cast<std::chrono::nanoseconds>(
               std::chrono::steady_clock::now().time_since_epoch())
        .count();
}

static inline SvcHdr *
svc_hdr(qhuff_svc *v, uint32_t k)
{
    return (SvcHdr *) (v->slots_h + (size_t) k * kSvcSlotBytes);
}

static bool
svc_fits(const uint32_t *in_off, uint32_t n)
{
    return n <= kSvcMaxStrings && (uint64_t) in_off[n] - in_off[0] <= kSvcInCap
           && in_off[n] >= in_off[0];
}

// start the kernel if its stream is idle (a previous instance has left)
static int
svc_ensure_running(qhuff_svc *v)
{
    std::lock_guard<std::mutex> g(v->launch_mu);
    qhuff_ctx *c = v->ctx;
    const hipError_t q = hipStreamQuery(v->stream);
    if (q == hipErrorNotReady)
        return QHUFF_OK;
    if (q != hipSuccess)
        return fail(c, q, "hipStreamQuery(service)");
    HIPCHK(c, hipSetDevice(c->device));
    __atomic_store_n(&v->ctl_h[0], 0u, __ATOMIC_RELEASE);
    HIPCHK(c, hipMemsetAsync(v->active, 0, sizeof(uint64_t), v->stream));
    SvcArgs a;
    a.slots = v->slots_d;
    a.scratch = v->scratch;
    a.ctl = v->ctl_d;
    a.active = v->active;
    a.win = c->tab->win;
    a.sorted = c->tab->sorted;
    a.long2 = c->tab->long2;
    a.enc = c->tab->enc;
    a.idle_ticks = v->idle_ticks;
    a.life_ticks = v->life_ticks;
    HIPCHK(c, launch_service(a, v->grid, v->stream));
    v->launches.fetch_add(1, std::memory_order_relaxed);
    return QHUFF_OK;
}

extern "C" int
qhuff_svc_open(qhuff_ctx *c, unsigned slots, unsigned idle_us, qhuff_svc **out)
{
    if (!c || !out)
        return QHUFF_EINVAL;
    *out = nullptr;
    if (c->svc)
        return QHUFF_EINVAL;                     // one service per context
    HIPCHK(c, hipSetDevice(c->device));
    const uint32_t wpb = (uint32_t) service_waves_per_block();
    uint32_t grid = slots ? (slots + wpb - 1) / wpb : 1;
    if (grid > (uint32_t) c->n_cu / 4)
        grid = (uint32_t) c->n_cu / 4;           // at most a quarter of the CUs
    if (grid < 1)
        grid = 1;
    qhuff_svc *v = new (std::nothrow) qhuff_svc();
    if (!v)
        return QHUFF_ENOMEM;
    v->ctx = c;
    v->grid = grid;
    v->n_slots = grid * wpb;
    v->idle_ticks = 100ull * (idle_us ? idle_us : 20000u);   // 100 MHz clock
    v->fresh_ns = 500ll * (idle_us ? idle_us : 20000u);      // idle_us / 2
    v->life_ticks = 100ull * 1000000ull * 10;                // 10 s
    v->busy = new std::atomic<uint32_t>[v->n_slots];
    v->seq = new uint32_t[v->n_slots];
    for (uint32_t k = 0; k < v->n_slots; ++k)
    {
        v->busy[k].store(0);
        v->seq[k] = 0;
    }
    const size_t sb = (size_t) v->n_slots * kSvcSlotBytes;
    hipError_t e = hipHostMalloc((void **) &v->slots_h, sb,
                                 hipHostMallocMapped | hipHostMallocCoherent);
    if (e == hipSuccess)
    {
        memset(v->slots_h, 0, sb);
        e = hipHostGetDevicePointer((void **) &v->slots_d, v->slots_h, 0);
    }
    if (e == hipSuccess)
        e = hipHostMalloc((void **) &v->ctl_h, 64,
                          hipHostMallocMapped | hipHostMallocCoherent);
    if (e == hipSuccess)
    {
        memset(v->ctl_h, 0, 64);
        e = hipHostGetDevicePointer((void **) &v->ctl_d, v->ctl_h, 0);
    }
    if (e == hipSuccess)
        e = hipMalloc((void **) &v->scratch, (size_t) v->n_slots * kSvcScratchBytes);
    if (e == hipSuccess)
        e = hipMalloc((void **) &v->active, 64);
    if (e == hipSuccess)
        e = hipStreamCreateWithFlags(&v->stream, hipStreamNonBlocking);
    if (e != hipSuccess)
    {
        const int rc = fail(c, e, "service setup");
        c->svc = v;
        qhuff_svc_close(v);
        return rc;
    }
    c->svc = v;
    const int rc = svc_ensure_running(v);
    if (rc)
    {
        qhuff_svc_close(v);
        return rc;
    }
    *out = v;
    return QHUFF_OK;
}

extern "C" void
qhuff_svc_close(qhuff_svc *v)
{
    if (!v)
        return;
    qhuff_ctx *c = v->ctx;
    (void) hipSetDevice(c->device);
    if (v->ctl_h)
        __atomic_store_n(&v->ctl_h[0], 1u, __ATOMIC_RELEASE);
    if (v->stream)
    {
        (void) hipStreamSynchronize(v->stream);
        (void) hipStreamDestroy(v->stream);
    }
    if (v->scratch)
        (void) hipFree(v->scratch);
    if (v->active)
        (void) hipFree(v->active);
    if (v->slots_h)
        (void) hipHostFree(v->slots_h);
    if (v->ctl_h)
        (void) hipHostFree(v->ctl_h);
    delete[] v->busy;
    delete[] v->seq;
    if (c->svc == v)
        c->svc = nullptr;
    delete v;
}

// (qhuff_shim.cpp) whether ctx has the low-latency service attached
bool
qhuff::ctx_has_service(const qhuff_ctx *c)
{
    return c && c->svc;
}

// (qhuff_shim.cpp) one host-memory decode call whose rejected strings keep,
// as their output, the bytes decoded before the error (the DecPolicyT Keep
// kernel): the per-string entry points replay from them where the
// reference's decoder stops on an invalid string.  Through the context's
// host path, under the service's fallback lock when one is attached (the
// context may then be shared between threads).
int
qhuff::decode_keep_rejected(qhuff_ctx *c, const uint8_t *in,
                            const uint32_t *in_off, uint32_t n, uint8_t *out,
                            uint32_t *out_off, uint8_t *status)
{
    if (!c)
        return QHUFF_EINVAL;
    std::unique_lock<std::mutex> lk;
    if (c->svc)
        lk = std::unique_lock<std::mutex>(c->svc->fallback_mu);
    c->keep_rejected = true;
    const int rc = host_batch(c, false, in, in_off, n, 0, out, out_off, status);
    c->keep_rejected = false;
    return rc;
}

extern "C" int
qhuff_svc_stats(qhuff_svc *v, uint64_t *served, uint64_t *launches,
                uint64_t *fallbacks)
{
    if (!v)
        return QHUFF_EINVAL;
    if (served)
        *served = v->served.load();
    if (launches)
        *launches = v->launches.load();
    if (fallbacks)
        *fallbacks = v->fallbacks.load();
    return QHUFF_OK;
}

// Slot states (qhuff_svc::busy): free, taken by a call, or orphaned -- its
// request was posted but the call gave up on it (an error while waiting);
// an orphaned slot is free again once its done word shows that request.
constexpr uint32_t kSlotFree = 0, kSlotTaken = 1, kSlotOrphan = 2;

// take a free slot (spinning / yielding while none is); try_only: return
// n_slots at once if none is free.  A blocking take gives up after 10 s
// (every slot held by calls that never finish, e.g. a service that cannot
// run): it returns n_slots then too, and the caller reports QHUFF_EDEVICE.
static uint32_t
svc_take(qhuff_svc *v, bool try_only)
{
    uint32_t k = v->next_slot.fetch_add(1, std::memory_order_relaxed) % v->n_slots;
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t tries = 0;; ++tries)
    {
        uint32_t z = kSlotFree;
        if (v->busy[k].compare_exchange_strong(z, kSlotTaken,
                                               std::memory_order_acquire))
            return k;
        if (z == kSlotOrphan
            && __atomic_load_n(&svc_hdr(v, k)->done, __ATOMIC_ACQUIRE) == v->seq[k]
            && v->busy[k].compare_exchange_strong(z, kSlotTaken,
                                                  std::memory_order_acquire))
            return k;                            // its abandoned request is done
        k = (k + 1) % v->n_slots;
        if (tries % v->n_slots == v->n_slots - 1)
        {
            if (try_only)
                return v->n_slots;
            if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(10))
                return v->n_slots;
            std::this_thread::yield();
        }
    }
}

// a call that stops waiting for slot k's request sq: free the slot if the
// request is done, else leave it orphaned (svc_take frees it once it is)
static void
svc_abandon(qhuff_svc *v, uint32_t k, uint32_t sq)
{
    const bool done = __atomic_load_n(&svc_hdr(v, k)->done, __ATOMIC_ACQUIRE) == sq;
    v->busy[k].store(done ? kSlotFree : kSlotOrphan, std::memory_order_release);
}

// write strings [s0, s1) of the call into slot k and post it; returns the
// request's sequence number
static uint32_t
svc_post(qhuff_svc *v, uint32_t k, bool enc, const uint8_t *in,
         const uint32_t *in_off, uint32_t s0, uint32_t s1, unsigned mode)
{
    uint8_t *sb = v->slots_h + (size_t) k * kSvcSlotBytes;
    SvcHdr *h = svc_hdr(v, k);
    const uint32_t n = s1 - s0, a0 = in_off[s0], nb = in_off[s1] - a0;
    uint32_t *so = (uint32_t *) (sb + kSvcInOffAt);
    for (uint32_t i = 0; i <= n; ++i)
        so[i] = in_off[s0 + i] - a0;
    if (nb)
        memcpy(sb + kSvcInAt, in + a0, nb);
    h->n = n;
    h->in_bytes = nb;
    h->opmode = (enc ? kSvcOpEncode : kSvcOpDecode) | (mode << 8);
    const uint32_t sq = v->seq[k] + 1 ? v->seq[k] + 1 : 1;
    v->seq[k] = sq;
    __atomic_store_n(&h->req, sq, __ATOMIC_RELEASE);
    return sq;
}

// Wait for slot k's request sq: spin on the done word; every ~50 us check
// that the kernel still runs (its waves leave after idle_us with no request
// served, and one may have left just as this request was posted); give up
// after 10 s (the slot then stays taken).
static int
svc_wait(qhuff_svc *v, uint32_t k, uint32_t sq)
{
    SvcHdr *h = svc_hdr(v, k);
    const auto t0 = std::chrono::steady_clock::now();
    auto t_chk = t0;
    for (uint32_t it = 0;; ++it)
    {
        if (__atomic_load_n(&h->done, __ATOMIC_ACQUIRE) == sq)
            return QHUFF_OK;
        if ((it & 255) == 255)
        {
            const auto now = std::chrono::steady_clock::now();
            if (now - t_chk > std::chrono::microseconds(50))
            {
                t_chk = now;
                int rc = svc_ensure_running(v);
                if (rc)
                    return rc;
                if (now - t0 > std::chrono::seconds(10))
                {
                    snprintf(v->ctx->err_msg, sizeof(v->ctx->err_msg),
                             "service request timed out");
                    return QHUFF_EDEVICE;
                }
            }
        }
        __builtin_ia32_pause();
    }
}

// slot k's result for n strings -> out + base, out_off / status (the
// piece's first string); returns its output bytes
static uint32_t
svc_collect(qhuff_svc *v, uint32_t k, bool enc, uint32_t n, uint32_t base,
            uint8_t *out, uint32_t *out_off, uint8_t *status)
{
    const uint8_t *sb = v->slots_h + (size_t) k * kSvcSlotBytes;
    const uint32_t *oo = (const uint32_t *) (sb + kSvcOutOffAt);
    const uint32_t total = oo[n];
    for (uint32_t i = 0; i < n; ++i)
        out_off[i] = base + oo[i];
    if (total)
        memcpy(out + base, sb + kSvcOutAt, total);
    if (!enc)
        memcpy(status, sb + kSvcStatusAt, n);
    return total;
}

// A call is cut into pieces of at most one staged tile each (64 strings,
// kSvcTileBytes input bytes; a longer string alone), one slot per piece: the
// service codes a one-tile piece straight from its slot, and the pieces of
// a call run on as many waves at once as there are free slots.

// the end of the piece that starts at string s0 (s0 < n)
static uint32_t
svc_piece_end(const uint32_t *in_off, uint32_t s0, uint32_t n)
{
    uint32_t s1 = s0 + 1;
    while (s1 < n && s1 - s0 < (uint32_t) kWT
           && in_off[s1 + 1] - in_off[s0] <= kSvcTileBytes)
        ++s1;
    return s1;
}

// (diagnostic, host arithmetic only) the cuts svc_call makes
extern "C" int
qhuff_svc_pieces(const uint32_t *in_off, uint32_t n, uint32_t *cuts,
                 uint32_t max_pieces, uint32_t *n_pieces)
{
    if (!in_off || !cuts || !n_pieces)
        return QHUFF_EINVAL;
    for (uint32_t i = 0; i < n; ++i)
        if (in_off[i + 1] < in_off[i])
            return QHUFF_EINVAL;
    *n_pieces = 0;
    cuts[0] = 0;
    if (!svc_fits(in_off, n))                    // the context's host path
        return QHUFF_OK;
    uint32_t np = 0;
    for (uint32_t s0 = 0; s0 < n; ++np)
    {
        s0 = svc_piece_end(in_off, s0, n);
        if (np < max_pieces)
            cuts[np + 1] = s0;
    }
    *n_pieces = np;
    return np > max_pieces ? QHUFF_ERANGE : QHUFF_OK;
}

int
qhuff::svc_call(qhuff_svc *v, bool enc, const uint8_t *in, const uint32_t *in_off,
         uint32_t n, unsigned mode, uint8_t *out, uint32_t *out_off,
         uint8_t *status)
{
    qhuff_ctx *c = v->ctx;
    if (!in_off || !out_off || (n && (!in || !out)) || (!enc && n && !status))
        return QHUFF_EINVAL;
    if (enc && !mode_ok(mode))
        return QHUFF_EINVAL;
    if (n == 0)
    {
        out_off[0] = 0;
        return QHUFF_OK;
    }
    for (uint32_t i = 0; i < n; ++i)             // the kernel trusts the slot
        if (in_off[i + 1] < in_off[i])
            return QHUFF_EINVAL;
    if (!svc_fits(in_off, n))
    {
        // too large for a slot: the context's host path (one caller at a time)
        std::lock_guard<std::mutex> g(v->fallback_mu);
        v->fallbacks.fetch_add(1, std::memory_order_relaxed);
        return host_batch(c, enc, in, in_off, n, mode, out, out_off, status);
    }
    constexpr uint32_t kMaxRound = 64;           // pieces in flight per call
    uint32_t base = 0;
    uint32_t s0 = 0;
    while (s0 < n)
    {
        // this round's pieces, each in its own slot (the first slot waited
        // for, further ones only while free)
        uint32_t slot[kMaxRound], p0[kMaxRound + 1], sq[kMaxRound];
        uint32_t np = 0;
        p0[0] = s0;
        while (s0 < n && np < kMaxRound)
        {
            const uint32_t s1 = svc_piece_end(in_off, s0, n);
            const uint32_t k = svc_take(v, np > 0);
            if (k == v->n_slots)
            {
                if (np > 0)
                    break;                       // a partial round: go on
                snprintf(c->err_msg, sizeof(c->err_msg),
                         "service: no request slot freed within 10 s");
                return QHUFF_EDEVICE;
            }
            slot[np] = k;
            sq[np] = svc_post(v, k, enc, in, in_off, s0, s1, mode);
            p0[++np] = s1;
            s0 = s1;
        }
        int rc = QHUFF_OK;
        if (steady_ns() - v->last_done_ns.load(std::memory_order_relaxed)
                > v->fresh_ns)
            rc = svc_ensure_running(v);
        for (uint32_t j = 0; j < np; ++j)
        {
            if (!rc)
                rc = svc_wait(v, slot[j], sq[j]);
            if (rc)
            {
                // this piece and the rest of the round are abandoned: their
                // slots come back once their requests are done
                svc_abandon(v, slot[j], sq[j]);
                continue;
            }
            const uint32_t a = p0[j], m = p0[j + 1] - a;
            base += svc_collect(v, slot[j], enc, m, base, out, out_off + a,
                                enc ? nullptr : status + a);
            v->busy[slot[j]].store(kSlotFree, std::memory_order_release);
        }
        if (rc)
            return rc;
    }
    out_off[n] = base;
    v->served.fetch_add(1, std::memory_order_relaxed);
    v->last_done_ns.store(steady_ns(), std::memory_order_relaxed);
    return QHUFF_OK;
}

extern "C" int
qhuff_svc_encode(qhuff_svc *v, const uint8_t *in, const uint32_t *in_off,
                 uint32_t n, unsigned mode, uint8_t *out, uint32_t *out_off)
{
    if (!v)
        return QHUFF_EINVAL;
    return svc_call(v, true, in, in_off, n, mode, out, out_off, nullptr);
}

extern "C" int
qhuff_svc_decode(qhuff_svc *v, const uint8_t *in, const uint32_t *in_off,
                 uint32_t n, uint8_t *out, uint32_t *out_off, uint8_t *status)
{
    if (!v)
        return QHUFF_EINVAL;
    return svc_call(v, false, in, in_off, n, 0, out, out_off, status);
}
