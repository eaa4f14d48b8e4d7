// qhuff_host.cpp -- host side of the C-ABI in include/qhuff.h: context
// (tables uploaded once, look-back workspace, error word, grid sizing),
// device-pointer batch calls and host-only helpers (the rest: qhuff_ctx.h).
#include "qhuff_ctx.h"
#include "qhuff_lookup_dyn_impl.h"
#include "qhuff_tabs_insert_impl.h"

// ---------------------------------------------------------------------------
// host side: context, C-ABI

// device words: [0] sticky error word (rest reserved)
constexpr size_t kErrWords = 64;

// the calling thread's last qhuff_open failure (qhuff_last_error(NULL))
thread_local char qhuff::t_open_err[160] = "no context";

int
qhuff::fail(qhuff_ctx *c, hipError_t e, const char *what)
{
    if (c)
    {
        snprintf(c->err_msg, sizeof(c->err_msg), "%s: %s", what, hipGetErrorString(e));
        snprintf(t_open_err, sizeof(t_open_err), "%s", c->err_msg);
    }
    return e == hipErrorOutOfMemory ? QHUFF_ENOMEM : QHUFF_EDEVICE;
}

// ---- big-tile output slots ---------------------------------------------------
//
// A launch in auto or full-only mode may code big tiles through kBigSlots
// global slots per wave of its grid (qhuff_pipeline.h tile_loop): 48 KB a
// wave, 151 MB for the resident grid of 256 CUs.  A launch of at most
// kSmallGrid workgroups (the per-string entry points, small batches) uses a
// region of its own context, allocated at its first such launch (4.7 MB);
// larger ones use one of the device's pool banks (up to kPoolBanks, each
// allocated at its first use, all freed with the last context that used
// the pool).  So a context's own device memory stays small (tables,
// look-back flags, its staging), however many contexts a process opens.
//
// A bank belongs to the context of its last launch.  A context launches on
// its own bank without any ordering (its own launches are ordered by
// prepare_launch); a launch on a bank another context used last first
// records the bank's event on that context's last stream and waits for it.
// A context takes a bank from another only when it has none, or when no new
// bank can be had: a context whose bank was taken from it (two contexts
// alternating -- an encode stream and a decode stream) gets a bank of its
// own, so concurrent contexts are not serialised; one context after another
// (a second context opened later) reuses the first's bank.  Nothing is
// recorded while a context keeps its bank -- an event record after every
// launch cost the bench line 4 % (683-689 against 713-720 GB/s,
// profiles/r06_c) -- and no device synchronisation is needed (it would also
// wait for other libraries' streams and a resident service kernel, ADVICE
// r05; only if recording on the last launch's stream fails, e.g. the caller
// destroyed it, is the device synchronised).  A bank outgrown by a larger
// grid is retired, not freed, until the pool's last user closes.
// (QHUFF_SLOT_BANKS=1..4 caps the banks, read at qhuff_open; 1: every
// context on one bank, the round-6 first design.)
constexpr uint32_t kSmallGrid = 8;
constexpr uint64_t kWaveSlotBytes = (uint64_t) kBigSlots * kBigSlotBytes;
constexpr int kMaxDevices = 64;
constexpr uint32_t kPoolBanks = 4;

struct SlotBank
{
    uint8_t *p = nullptr;
    uint64_t waves = 0;                  // slots for this many waves
    hipEvent_t ev = nullptr;             // (recorded when it changes hands)
    const qhuff_ctx *last_ctx = nullptr; // the last launch on it: its context
    hipStream_t last_st = nullptr;       // and stream
};

struct SlotPool
{
    std::mutex mu;
    SlotBank bank[kPoolBanks];
    int refs = 0;                        // contexts that used it
    std::vector<uint8_t *> retired;      // outgrown banks (freed with it)
};
static SlotPool g_pool[kMaxDevices];

static void
pool_release(int device, const qhuff_ctx *c)
{
    if (device < 0 || device >= kMaxDevices)
        return;
    SlotPool &sp = g_pool[device];
    std::lock_guard<std::mutex> g(sp.mu);
    for (SlotBank &b : sp.bank)
        if (b.last_ctx == c)             // (its launches have completed)
            b.last_ctx = nullptr;
    if (--sp.refs > 0)
        return;
    for (SlotBank &b : sp.bank)
    {
        if (b.p)
            (void) hipFree(b.p);
        if (b.ev)
            (void) hipEventDestroy(b.ev);
        b = SlotBank();
    }
    for (uint8_t *q : sp.retired)
        (void) hipFree(q);
    sp.retired.clear();
}

static uint64_t
max_grid_waves(const qhuff_ctx *c)
{
    const uint64_t e = (uint64_t) c->enc_grid * encode_waves_per_block();
    const uint64_t d = (uint64_t) c->dec_grid * decode_waves_per_block();
    return e > d ? e : d;
}

// the bank context c launches on (sp.mu held): its own; else a free one
// (never used, or its context closed); else, if c's bank was taken from it,
// a new one (up to c->max_banks); else the one c had, or bank 0
static uint32_t
pool_pick(SlotPool &sp, const qhuff_ctx *c)
{
    const uint32_t own = c->pool_bank;
    if (own && (sp.bank[own - 1].last_ctx == c || !sp.bank[own - 1].last_ctx))
        return own - 1;
    for (uint32_t i = 0; i < c->max_banks; ++i)
        if (sp.bank[i].p && !sp.bank[i].last_ctx)
            return i;
    if (own || !sp.bank[0].p)
        for (uint32_t i = 0; i < c->max_banks; ++i)
            if (!sp.bank[i].p)
                return i;
    return own ? own - 1 : 0;
}

// Runs launch(slots) for a launch of `grid` workgroups of `wpb` waves: the
// big-tile slots a full kernel needs (*full), null for the lean one.  When
// they cannot be allocated the launch runs the lean kernel (*full is
// cleared): big tiles out of line, the same output.
template <class F>
static int
with_slots(qhuff_ctx *c, uint32_t grid, uint64_t wpb, bool *full,
           hipStream_t st, F launch)
{
    if (!*full)
        return launch((uint8_t *) nullptr);
    if (grid <= kSmallGrid)
    {
        if (!c->big_small)
        {
            const uint64_t w = (uint64_t) kSmallGrid
                * (uint64_t) (encode_waves_per_block() > decode_waves_per_block()
                              ? encode_waves_per_block() : decode_waves_per_block());
            if (hipMalloc((void **) &c->big_small, w * kWaveSlotBytes) != hipSuccess)
            {
                c->big_small = nullptr;
                (void) hipGetLastError();
                *full = false;
                return launch((uint8_t *) nullptr);
            }
        }
        return launch(c->big_small);
    }
    if (c->device < 0 || c->device >= kMaxDevices)
    {
        *full = false;
        return launch((uint8_t *) nullptr);
    }
    SlotPool &sp = g_pool[c->device];
    std::lock_guard<std::mutex> g(sp.mu);
    if (!c->pool_ref)
    {
        ++sp.refs;
        c->pool_ref = true;
    }
    const uint64_t need = (uint64_t) grid * wpb;
    uint32_t bi = pool_pick(sp, c);
    if (!sp.bank[bi].p && bi != 0 && sp.bank[0].p)
    {
        // a new bank for a context whose bank was taken: if it cannot be
        // had, share (the ordering below), never the lean kernel
        const uint64_t mw = max_grid_waves(c);
        const uint64_t w = mw > need ? mw : need;
        if (hipMalloc((void **) &sp.bank[bi].p, w * kWaveSlotBytes) == hipSuccess)
            sp.bank[bi].waves = w;
        else
        {
            sp.bank[bi].p = nullptr;
            (void) hipGetLastError();
            bi = c->pool_bank ? c->pool_bank - 1 : 0;
        }
    }
    SlotBank &b = sp.bank[bi];
    if (b.waves < need)
    {
        if (b.p)
        {
            // (a grid larger than any seen: launches still running on the
            // old bank keep it until the pool's last user closes)
            sp.retired.push_back(b.p);
            b.p = nullptr;
            b.waves = 0;
        }
        const uint64_t mw = max_grid_waves(c);
        const uint64_t w = mw > need ? mw : need;
        if (hipMalloc((void **) &b.p, w * kWaveSlotBytes) != hipSuccess)
        {
            b.p = nullptr;
            (void) hipGetLastError();
            *full = false;
            return launch((uint8_t *) nullptr);
        }
        b.waves = w;
    }
    if (b.last_ctx && b.last_ctx != c)
    {
        // after the bank's last launch, another context's: everything on
        // its stream so far
        if (!b.ev)
            HIPCHK(c, hipEventCreateWithFlags(&b.ev, hipEventDisableTiming));
        hipError_t e = hipEventRecord(b.ev, b.last_st);
        if (e == hipSuccess)
            e = hipStreamWaitEvent(st, b.ev, 0);
        if (e != hipSuccess)
        {
            (void) hipGetLastError();
            HIPCHK(c, hipDeviceSynchronize());
        }
    }
    const int rc = launch(b.p);
    if (rc == QHUFF_OK)
    {
        b.last_ctx = c;
        b.last_st = st;
        c->pool_bank = bi + 1;
    }
    return rc;
}

extern "C" int
qhuff_open(int device, qhuff_ctx **ctx_out)
{
    if (!ctx_out)
        return QHUFF_EINVAL;
    *ctx_out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
        return QHUFF_ENODEV;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess)
        return QHUFF_ENODEV;
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return QHUFF_ENODEV;              // code objects are gfx950 only
    qhuff_ctx *c = new (std::nothrow) qhuff_ctx();
    if (!c)
        return QHUFF_ENOMEM;
    c->device = device;
    HIPCHK(c, hipSetDevice(device));
    c->n_cu = prop.multiProcessorCount;
    HostTables *ht = new HostTables;
    build_tables(ht);
    DevTables dt;
    for (int i = 0; i < 257; ++i)
        dt.enc[i] = make_uint2(ht->code[i], ht->bits[i]);
    memcpy(dt.win, ht->win, sizeof(dt.win));
    memcpy(dt.sorted, ht->sorted, sizeof(dt.sorted));
    memcpy(dt.long2, ht->long2, sizeof(dt.long2));
    memcpy(dt.nodes, ht->nodes, sizeof(dt.nodes));
    memset(&c->lp, 0, sizeof(c->lp));
    c->lp.n = ht->n_long;
    memcpy(c->lp.l, ht->longc, sizeof(LongLen) * ht->n_long);
    delete ht;
    int rc, occ_e = 0, occ_d = 0, occ_h = 0;
    hipError_t e = encode_occupancy(&occ_e);
    if (e == hipSuccess)
        e = decode_occupancy(&occ_d);
    if (e == hipSuccess)
        e = hash_occupancy(&occ_h);
    if (e != hipSuccess || occ_e < 1 || occ_d < 1 || occ_h < 1)
    {
        char what[96];
        snprintf(what, sizeof(what), "occupancy query (enc %d dec %d hash %d)",
                 occ_e, occ_d, occ_h);
        rc = fail(c, e, what);
        delete c;
        return rc ? rc : QHUFF_EDEVICE;
    }
    // One launch's grid: the workgroups that fit at once (tiles come from
    // in-order tickets, so a grid that is not co-resident -- another
    // context or process on the GPU -- is slower, not wrong).
    c->enc_grid = (uint32_t) (occ_e * c->n_cu);
    c->dec_grid = (uint32_t) (occ_d * c->n_cu);
    c->hash_grid = (uint32_t) (occ_h * c->n_cu);
    e = hipMalloc((void **) &c->tab, sizeof(DevTables));
    if (e != hipSuccess)
    {
        rc = fail(c, e, "hipMalloc tables");
        delete c;
        return rc;
    }
    e = hipMemcpy(c->tab, &dt, sizeof(dt), hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = hipMalloc((void **) &c->err, kErrWords * sizeof(uint32_t));
    if (e == hipSuccess)
        e = hipMemset(c->err, 0, kErrWords * sizeof(uint32_t));
    if (e == hipSuccess)
    {
        const char *kv = getenv("QHUFF_KERNELS");
        c->kernels = !kv ? 0 : !strcmp(kv, "lean") ? 1 : !strcmp(kv, "full") ? 2 : 0;
        // test / A-B knob: the super-flag replica every wave polls; unset,
        // -1 or out of range: by workgroup (qhuff_device.h kLbReplicas)
        const char *rv = getenv("QHUFF_LB_REPLICA");
        const long r = rv ? strtol(rv, nullptr, 0) : -1;
        c->lb_replica = r >= 0 && r < (long) kLbReplicas ? (int) r : -1;
    }
    if (e == hipSuccess)
        e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking);
    if (e == hipSuccess)
        e = hipEventCreateWithFlags(&c->ev_last, hipEventDisableTiming);
    if (e == hipSuccess)
        e = hipHostMalloc((void **) &c->err_host, 4 * sizeof(uint32_t),
                          hipHostMallocMapped | hipHostMallocCoherent);
    if (e == hipSuccess)
    {
        memset(c->err_host, 0, 4 * sizeof(uint32_t));
        e = hipHostGetDevicePointer((void **) &c->err_host_dev, c->err_host, 0);
    }
    if (e != hipSuccess)
    {
        rc = fail(c, e, "context setup");
        qhuff_close(c);
        return rc;
    }
    c->epoch = 0;
    // test knob: the epoch the context starts behind, so that a test can
    // open one a few launches before the 22-bit wrap (prepare_launch)
    if (const char *e0 = getenv("QHUFF_EPOCH0"))
        c->epoch = (uint32_t) strtoul(e0, nullptr, 0) & kEpochMask;
    c->hint[0] = c->hint[1] = -1;
    c->max_banks = kPoolBanks;
    if (const char *sb = getenv("QHUFF_SLOT_BANKS"))
    {
        const uint32_t k = (uint32_t) strtoul(sb, nullptr, 0);
        if (k >= 1 && k <= kPoolBanks)
            c->max_banks = k;
    }
    {
        // tuning override: fewer workgroups per CU than fit
        const char *g = getenv("QHUFF_GRID_WG_PER_CU");
        if (g)
        {
            uint32_t k = (uint32_t) strtoul(g, nullptr, 0);
            if (k >= 1 && k <= (uint32_t) occ_e)
                c->enc_grid = k * c->n_cu;
            if (k >= 1 && k <= (uint32_t) occ_d)
                c->dec_grid = k * c->n_cu;
            if (k >= 1 && k <= (uint32_t) occ_h)
                c->hash_grid = k * c->n_cu;
        }
        // experiment: a percentage of the resident grid (half the CUs' worth
        // of workgroups at 50: per-CU vs chip-wide limits)
        const char *pc = getenv("QHUFF_GRID_PCT");
        if (pc)
        {
            const uint32_t q = (uint32_t) strtoul(pc, nullptr, 0);
            if (q >= 1 && q <= 100)
            {
                c->enc_grid = c->enc_grid * q / 100 ? c->enc_grid * q / 100 : 1;
                c->dec_grid = c->dec_grid * q / 100 ? c->dec_grid * q / 100 : 1;
                c->hash_grid = c->hash_grid * q / 100 ? c->hash_grid * q / 100 : 1;
            }
        }
    }
    *ctx_out = c;
    return QHUFF_OK;
}

extern "C" void
qhuff_close(qhuff_ctx *c)
{
    if (!c)
        return;
    (void) hipSetDevice(c->device);
    if (c->svc)
        qhuff_svc_close(c->svc);
    if (c->own_stream)
        (void) hipStreamSynchronize(c->own_stream);
    (void) hipDeviceSynchronize();
    if (c->tab)
        (void) hipFree(c->tab);
    if (c->flags)
        (void) hipFree(c->flags);
    if (c->big_small)
        (void) hipFree(c->big_small);
    if (c->pool_ref)
        pool_release(c->device, c);
    if (c->err)
        (void) hipFree(c->err);
    if (c->d_stage)
        (void) hipFree(c->d_stage);
    if (c->h_stage)
        (void) hipHostFree(c->h_stage);
    if (c->prof)
        (void) hipFree(c->prof);
    if (c->scan_ws)
        (void) hipFree(c->scan_ws);
    if (c->scan_ev)
        (void) hipEventDestroy(c->scan_ev);
    if (c->hdr_ws)
        (void) hipFree(c->hdr_ws);
    if (c->hdr_ev)
        (void) hipEventDestroy(c->hdr_ev);
    if (c->dyn_ws)
        (void) hipFree(c->dyn_ws);
    if (c->ins_ws)
        (void) hipFree(c->ins_ws);
    if (c->tev)
    {
        for (unsigned i = 0; i < 2 * QHUFF_TIMING_SLOTS; ++i)
            (void) hipEventDestroy(c->tev[i]);
        delete[] c->tev;
    }
    if (c->own_stream)
        (void) hipStreamDestroy(c->own_stream);
    if (c->ev_last)
        (void) hipEventDestroy(c->ev_last);
    if (c->err_host)
        (void) hipHostFree(c->err_host);
    pipe_teardown(c);
    delete c;
}

extern "C" const char *
qhuff_last_error(qhuff_ctx *c)
{
    return c ? c->err_msg : t_open_err;
}

extern "C" int
qhuff_device_error(qhuff_ctx *c)
{
    if (!c)
        return QHUFF_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    uint32_t v = 0;
    HIPCHK(c, hipMemcpy(&v, c->err, 4, hipMemcpyDeviceToHost));
    if (v)
        HIPCHK(c, hipMemset(c->err, 0, 4));
    v |= c->err_host[0];
    c->err_host[0] = 0;
    return (int) v;
}

// Profile builds: copy the stamp buffer of the last launch (synchronous).
// Path-trace builds (QH_PATH_TRACE): the last tile launch's records,
// kTraceWords u64 per tile (qhuff_device.h PathTrace).
// Returns the number of u64 words available (0 in normal builds).
extern "C" uint64_t
qhuff_profile_read(qhuff_ctx *c, uint64_t *dst, uint64_t max_words)
{
    if (!c || !c->prof)
        return 0;
    (void) hipDeviceSynchronize();
    const uint64_t w = c->prof_words < max_words ? c->prof_words : max_words;
    if (dst && w)
        (void) hipMemcpy(dst, c->prof, w * 8, hipMemcpyDeviceToHost);
    return c->prof_words;
}

extern "C" uint64_t
qhuff_encode_bound(uint64_t in_bytes, uint32_t n, unsigned mode)
{
    // 30-bit longest code: ceil(30 * len / 8) per string; framing adds at
    // most 6 bytes of prefixed length (32-bit value) per literal
    uint64_t b = (in_bytes * 30 + 7) / 8 + n;
    if (mode)
        b += 6ull * n;
    return b + 16;
}

extern "C" uint64_t
qhuff_decode_bound(uint64_t in_bytes, uint32_t n)
{
    (void) n;
    return in_bytes * 8 / 5 + 16;
}

// look-back workspace: the tile tickets [2][kTickGroups] (u32, kTickStride
// apart), tile flags [cap_tiles], super flags [kLbReplicas][cap_super] (each
// replica from a 256-byte boundary), super accumulators [2][cap_super]
// (u64, kAccStride apart)
constexpr size_t kTickBytes = 4 * 2 * kTickGroups * kTickStride;
static_assert(kTickBytes % 256 == 0, "the flags start on a 256-byte boundary");
static uint64_t
round_256b(uint64_t words)               // u64 words, up to whole 256 bytes
{
    return (words + 31) & ~(uint64_t) 31;
}
static size_t
lb_bytes(uint64_t cap_tiles, uint64_t cap_super)
{
    return kTickBytes + 8 * (round_256b(cap_tiles * kFlagStride)
                             + (uint64_t) kLbReplicas * sflag_stride((uint32_t) cap_super)
                             + 2 * cap_super * kAccStride);
}

// make room for the look-back workspace of `tiles` tiles and advance the
// epoch (flags are epoch-tagged; the claim counters and super accumulators
// of a launch are cleared by the launch before it).  Orders the launch
// after the context's previous one when that ran on another stream, and
// reports (then clears) a device error a previous launch left behind.
static int
prepare_launch(qhuff_ctx *c, uint64_t tiles, hipStream_t st)
{
    if (c->err_host[0])
    {
        snprintf(c->err_msg, sizeof(c->err_msg),
                 "device error %u in an earlier launch (outputs invalid)",
                 c->err_host[0]);
        c->err_host[0] = 0;
        (void) hipStreamSynchronize(c->last_stream);
        (void) hipMemset(c->err, 0, 4);
        return QHUFF_EDEVICE;
    }
    if (c->have_last && st != c->last_stream)
    {
        // everything queued on the previous stream so far, our last launch
        // included, before this one
        HIPCHK(c, hipEventRecord(c->ev_last, c->last_stream));
        HIPCHK(c, hipStreamWaitEvent(st, c->ev_last, 0));
    }
    if (tiles > c->cap_tiles)
    {
        if (c->flags)
        {
            HIPCHK(c, hipStreamSynchronize(st));
            HIPCHK(c, hipFree(c->flags));
            c->flags = nullptr;
        }
        uint64_t cap = tiles < 4096 ? 4096 : tiles;
        uint64_t caps = (cap + kSuper - 1) / kSuper;
        HIPCHK(c, hipMalloc((void **) &c->flags, lb_bytes(cap, caps)));
        HIPCHK(c, hipMemsetAsync(c->flags, 0, lb_bytes(cap, caps), st));
        c->cap_tiles = cap;
        c->cap_super = caps;
    }
    c->epoch = (c->epoch + 1) & kEpochMask;
    if (c->epoch == 0)
    {
        // wrapped: stale flags could alias the new epoch, and the
        // accumulators of epoch 1 were last used, not cleared
        HIPCHK(c, hipMemsetAsync(c->flags, 0, lb_bytes(c->cap_tiles, c->cap_super),
                                 st));
        c->epoch = 1;
    }
    return QHUFF_OK;
}

static Coord
coord(qhuff_ctx *c, uint64_t tiles, hipStream_t st)
{
    Coord k;
    k.prof = nullptr;
#ifdef QH_PATH_TRACE
    {
        // one record per tile of this launch, zeroed ahead of it on its
        // stream (qhuff_device.h PathTrace; a failed allocation leaves no
        // words to read)
        const size_t words = (size_t) tiles * kTraceWords;
        if (words > c->prof_cap)
        {
            if (c->prof)
            {
                (void) hipDeviceSynchronize();
                (void) hipFree(c->prof);
            }
            c->prof = nullptr;
            c->prof_cap = 0;
            const size_t cap = words < 4096 * kTraceWords ? 4096 * kTraceWords
                                                          : words;
            if (hipMalloc((void **) &c->prof, cap * 8) == hipSuccess)
                c->prof_cap = cap;
            else
                c->prof = nullptr;
        }
        c->prof_words = 0;
        if (c->prof
            && hipMemsetAsync(c->prof, 0, words * 8, st) == hipSuccess)
        {
            c->prof_words = words;
            k.prof = c->prof;
        }
    }
#else
    (void) st;
#endif
#ifdef QHUFF_PROFILE
    {
        const size_t words = (size_t) c->n_cu * 32 * kProfIters * kProfSlots;
        if (!c->prof && hipMalloc((void **) &c->prof, words * 8) == hipSuccess)
            c->prof_words = words;
        if (c->prof)
            (void) hipMemset(c->prof, 0, c->prof_words * 8);
        k.prof = c->prof;
    }
#endif
    k.tick = (uint32_t *) c->flags;
    k.flags = c->flags + kTickBytes / 8;
    k.sflags = k.flags + round_256b(c->cap_tiles * kFlagStride);
    k.sacc = k.sflags + (uint64_t) kLbReplicas * sflag_stride((uint32_t) c->cap_super);
    k.cap_super = (uint32_t) c->cap_super;   // (below 2^20: n is 32 bits)
    k.pin = (uint32_t) (c->lb_replica + 1);
    k.err = c->err;
    k.err_host = c->err_host_dev;
    k.epoch = c->epoch;
    k.n_tiles = (uint32_t) tiles;
    k.spread = 0;
    k.big = nullptr;                     // (with_slots)
    return k;
}

// the event pair of the next launch (kind QHUFF_KIND_*) with timing on, and
// its ring slot; *e0 = *e1 = null and kNoTiming otherwise.  The slot is
// taken by timing_commit once the launch has gone out: a launch that fails
// leaves no slot with unrecorded events behind.
constexpr uint32_t kNoTiming = 0xffffffffu;
static uint32_t
timing_slot(qhuff_ctx *c, uint32_t kind, hipEvent_t *e0, hipEvent_t *e1)
{
    *e0 = *e1 = nullptr;
    if (!c->t_on)
        return kNoTiming;
    // sampled: each timed launch costs the step ~4.6 us of queue time
    // (tools/timing_cost.py: 114.8 vs 105.6 us per encode + decode step)
    if (c->t_seen[kind]++ % c->t_every != 0)
        return kNoTiming;
    const uint32_t k = (uint32_t) (c->t_next % QHUFF_TIMING_SLOTS);
    *e0 = c->tev[2 * k];
    *e1 = c->tev[2 * k + 1];
    return k;
}

static void
timing_commit(qhuff_ctx *c, uint32_t k, uint32_t kind)
{
    if (k == kNoTiming)
        return;
    c->t_kind[k] = (uint8_t) kind;
    ++c->t_next;
}

// One launch of `kind` inside its timing bracket: launch(e0, e1) sends it
// with the slot's event pair (null: not timed) and returns the HIP error; the
// slot is committed only once the launch has gone out.  `what` names the
// launch in the context's error message.
template <class F>
static int
timed(qhuff_ctx *c, uint32_t kind, const char *what, F launch)
{
    hipEvent_t e0, e1;
    const uint32_t ts = timing_slot(c, kind, &e0, &e1);
    const hipError_t e = launch(e0, e1);
    if (e != hipSuccess)
        return fail(c, e, what);
    timing_commit(c, ts, kind);
    return QHUFF_OK;
}

extern "C" int
qhuff_timing_enable(qhuff_ctx *c, int on)
{
    if (!c)
        return QHUFF_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    if (on && !c->tev)
    {
        hipEvent_t *ev = new (std::nothrow) hipEvent_t[2 * QHUFF_TIMING_SLOTS]();
        if (!ev)
            return QHUFF_ENOMEM;
        for (unsigned i = 0; i < 2 * QHUFF_TIMING_SLOTS; ++i)
        {
            const hipError_t e = hipEventCreate(&ev[i]);
            if (e != hipSuccess)
            {
                for (unsigned j = 0; j < i; ++j)
                    (void) hipEventDestroy(ev[j]);
                delete[] ev;
                return fail(c, e, "hipEventCreate (timing)");
            }
        }
        c->tev = ev;
    }
    c->t_on = on > 0;
    c->t_every = on > 1 ? (uint32_t) on : 1u;
    c->t_seen[0] = c->t_seen[1] = c->t_seen[2] = c->t_seen[3] = 0;
    c->t_first = c->t_next;
    return QHUFF_OK;
}

extern "C" int
qhuff_timing_read(qhuff_ctx *c, uint32_t *kind, double *us, uint32_t max)
{
    if (!c || (max && (!kind || !us)))
        return QHUFF_EINVAL;
    if (!c->tev)
        return 0;
    HIPCHK(c, hipSetDevice(c->device));
    uint64_t a = c->t_first;
    const uint64_t b = c->t_next;
    if (b - a > QHUFF_TIMING_SLOTS)
        a = b - QHUFF_TIMING_SLOTS;
    if (b - a > max)
        a = b - max;
    uint32_t n = 0;
    for (uint64_t i = a; i < b; ++i, ++n)
    {
        const uint32_t k = (uint32_t) (i % QHUFF_TIMING_SLOTS);
        HIPCHK(c, hipEventSynchronize(c->tev[2 * k + 1]));
        float ms = 0.f;
        HIPCHK(c, hipEventElapsedTime(&ms, c->tev[2 * k], c->tev[2 * k + 1]));
        kind[n] = c->t_kind[k];
        us[n] = 1e3 * (double) ms;
    }
    c->t_first = b;
    return (int) n;
}

// Workgroups for a launch of `tiles` tiles, at most `cap` (the co-resident
// count: more would only queue); tiles are claimed from tickets, so any grid
// size is correct.  A batch of at most one tile per wave of the full grid
// is spread: one workgroup per tile up to `cap`, the first *spread waves
// of each taking one tile each (Coord::spread; fewer waves per CU code
// their tile faster, and the whole batch is handed out by one returning
// add per workgroup on one counter, in order).  Larger batches: every wave,
// ticket groups.
static uint32_t
grid_for(uint64_t tiles, uint64_t waves_per_block, uint32_t cap,
         uint32_t *spread)
{
    *spread = 0;
    if (tiles <= (uint64_t) cap * waves_per_block)
    {
        const uint32_t g = (uint32_t) (tiles < cap ? tiles : cap);
        *spread = (uint32_t) ((tiles + g - 1) / g);
        return g;
    }
    const uint64_t need = (tiles + waves_per_block - 1) / waves_per_block;
    return (uint32_t) (need < cap ? need : cap);
}

// The kernel variant of the next launch of `kind` (0 encode, 1 decode).
// The full kernel codes every batch at its best; the lean one (no big-tile
// slots, no cooperative long-string decode: those tiles out of line, one
// lane per string, up to 30x slower on the QIF corpus) is 0.7 % (encode) /
// 1.3 % (decode) faster on batches that never need them (profiles/r06_i,
// same-box pairs).  So: the full kernel, unless the caller's batch is known
// to have no string over 128 bytes and no tile over the 3 KB stage -- the
// host-memory calls read their offsets (host_hint), a device-pointer caller
// may say so with qhuff_batch_hint -- or QHUFF_KERNELS pins one.  (Until
// round 5 decode went by a history of earlier launches, lean until one
// reported such tiles: the first launch of a long-string batch after token
// batches then took 4.3x its warmed time.  Round 6 took the full decode
// kernel's cost on the token batch from +3.3 % to +1.3 %: the lane id
// opaque to the optimiser, uniform flags as u32, the cooperative phase on
// the big-tile path)
static bool
pick_full(qhuff_ctx *c, int kind)
{
    // a hint applies to the next launch of its kind only, whatever decides
    // this one
    const int hint = c->hint[kind];
    c->hint[kind] = -1;
    if (c->kernels)
        return c->last_full[kind] = c->kernels == 2;
    if (hint >= 0)
        return c->last_full[kind] = hint > 0;
    return c->last_full[kind] = true;
}

extern "C" int
qhuff_kernel_variant(qhuff_ctx *c, int kind)
{
    if (!c || (kind != QHUFF_KIND_ENCODE && kind != QHUFF_KIND_DECODE))
        return QHUFF_EINVAL;
    return c->last_full[kind] ? 1 : 0;
}

extern "C" int
qhuff_grid_waves(qhuff_ctx *c, int kind)
{
    if (!c)
        return QHUFF_EINVAL;
    switch (kind)
    {
    case QHUFF_KIND_ENCODE:
        return (int) (c->enc_grid * (uint32_t) encode_waves_per_block());
    case QHUFF_KIND_DECODE:
        return (int) (c->dec_grid * (uint32_t) decode_waves_per_block());
    case QHUFF_KIND_HASH:
        return (int) (c->hash_grid * (uint32_t) hash_waves_per_block());
    default:
        return QHUFF_EINVAL;
    }
}

extern "C" int
qhuff_batch_hint(qhuff_ctx *c, int kind, int hint)
{
    if (!c || (kind != QHUFF_KIND_ENCODE && kind != QHUFF_KIND_DECODE)
            || hint < -1 || hint > 1)
        return QHUFF_EINVAL;
    c->hint[kind] = hint;
    return QHUFF_OK;
}

// ---- the tile calls' launch frame ------------------------------------------
//
// qhuff_encode_batch, qhuff_decode_batch, qhuff_decode_stream,
// qhuff_decode_wire, qhuff_encode_wire and qhuff_decode_headers check their
// own arguments and then go through tile_launch; what differs between them
// is the body.

static EncArgs
enc_args(const qhuff_ctx *c, const uint8_t *in, const uint32_t *in_off,
         uint8_t *out, uint32_t *out_off, uint32_t n, unsigned mode,
         const Coord &k)
{
    EncArgs a;
    a.in = in;
    a.in_off = in_off;
    a.out = out;
    a.out_off = out_off;
    a.enc = c->tab->enc;
    a.n = n;
    a.mode = mode;
    a.c = k;
    return a;
}

static DecArgs
dec_args(const qhuff_ctx *c, const uint8_t *in, const uint32_t *in_off,
         uint8_t *out, uint32_t *out_off, uint8_t *status, uint32_t n,
         const Coord &k)
{
    DecArgs a;
    a.in = in;
    a.in_off = in_off;
    a.out = out;
    a.out_off = out_off;
    a.status = status;
    a.win = c->tab->win;
    a.sorted = c->tab->sorted;
    a.long2 = c->tab->long2;
    a.n = n;
    a.c = k;
    a.lp = c->lp;
    return a;
}

// One launch over n strings in tiles of `tile_strings`, by a kernel of `wpb`
// waves a workgroup on at most `cap` workgroups (its family's resident grid:
// the tiles are claimed from tickets, so any grid is correct).  n == 0
// writes out_off[0] and launches nothing.  Otherwise the look-back workspace
// is prepared, body(k, grid) fills its argument block around the launch's
// Coord k (spread set, big null) and launches on st; the context remembers
// the stream of a launch that went out (the ordering event is recorded only
// when a later launch comes on another stream, see prepare_launch).
template <class F>
static int
tile_launch(qhuff_ctx *c, uint32_t n, uint64_t tile_strings, uint64_t wpb,
            uint32_t cap, uint32_t *out_off, hipStream_t st, F body)
{
    HIPCHK(c, hipSetDevice(c->device));
    if (n == 0)
    {
#ifdef QH_PATH_TRACE
        c->prof_words = 0;               // (no tile, no record)
#endif
        HIPCHK(c, hipMemsetAsync(out_off, 0, 4, st));
        return QHUFF_OK;
    }
    const uint64_t tiles = (n + tile_strings - 1) / tile_strings;
    int rc = prepare_launch(c, tiles, st);
    if (rc)
        return rc;
    Coord k = coord(c, tiles, st);
    const uint32_t grid = grid_for(tiles, wpb, cap, &k.spread);
    rc = body(k, grid);
    if (rc)
        return rc;
    c->last_stream = st;
    c->have_last = true;
    return QHUFF_OK;
}

extern "C" int
qhuff_encode_batch(qhuff_ctx *c, const uint8_t *in, const uint32_t *in_off,
                   uint32_t n, unsigned mode, uint8_t *out, uint32_t *out_off,
                   void *stream)
{
    if (!c || !in_off || !out_off || (n && (!in || !out)))
        return QHUFF_EINVAL;
    if (!mode_ok(mode))
        return QHUFF_EINVAL;
    hipStream_t st = (hipStream_t) stream;
    const uint64_t wpb = (uint64_t) encode_waves_per_block();
    return tile_launch(c, n, kWT, wpb, c->enc_grid, out_off, st,
                       [&](const Coord &k, uint32_t grid) -> int {
        EncArgs a = enc_args(c, in, in_off, out, out_off, n, mode, k);
        bool full = pick_full(c, 0);
        const int rc = with_slots(c, grid, wpb, &full, st,
                                  [&](uint8_t *slots) -> int {
            a.c.big = slots;
            return timed(c, QHUFF_KIND_ENCODE, "launch_encode",
                         [&](hipEvent_t e0, hipEvent_t e1) {
                return launch_encode(a, grid, st, e0, e1, full);
            });
        });
        if (rc == QHUFF_OK)
            c->last_full[0] = full;
        return rc;
    });
}

extern "C" int
qhuff_decode_batch(qhuff_ctx *c, const uint8_t *in, const uint32_t *in_off,
                   uint32_t n, uint8_t *out, uint32_t *out_off,
                   uint8_t *status, void *stream)
{
    if (!c || !in_off || !out_off || (n && (!in || !out || !status)))
        return QHUFF_EINVAL;
    hipStream_t st = (hipStream_t) stream;
    const uint64_t wpb = (uint64_t) decode_waves_per_block();
    return tile_launch(c, n, decode_tile_strings(), wpb, c->dec_grid, out_off,
                       st, [&](const Coord &k, uint32_t grid) -> int {
        DecArgs a = dec_args(c, in, in_off, out, out_off, status, n, k);
        // (keep: the per-string replay -- the lean keep kernel, never timed,
        // and outside the variant choice of the batch kernel: ADVICE r04)
        const bool keep = c->keep_rejected;
        bool full = false;
        if (!keep)
            full = pick_full(c, 1);
        else
            c->hint[1] = -1;             // (consumed by this launch too)
        const int rc = with_slots(c, grid, wpb, &full, st,
                                  [&](uint8_t *slots) -> int {
            a.c.big = slots;
            if (keep)
            {
                HIPCHK(c, launch_decode(a, grid, st, nullptr, nullptr, true,
                                        full));
                return QHUFF_OK;
            }
            return timed(c, QHUFF_KIND_DECODE, "launch_decode",
                         [&](hipEvent_t e0, hipEvent_t e1) {
                return launch_decode(a, grid, st, e0, e1, false, full);
            });
        });
        if (rc == QHUFF_OK && !keep)
            c->last_full[1] = full;
        return rc;
    });
}

// ---- header hashing ---------------------------------------------------------

static int
hash_call(qhuff_ctx *c, const uint8_t *in, const uint32_t *off, uint32_t n,
          uint32_t seed, uint32_t *h1, uint32_t *h2, bool pairs, void *stream)
{
    if (!c || !off || (n && (!in || !h1 || (pairs && !h2))))
        return QHUFF_EINVAL;
    if (pairs && n > 0x7fffffffu)
        return QHUFF_ERANGE;
    HIPCHK(c, hipSetDevice(c->device));
    if (n == 0)
        return QHUFF_OK;
    HashArgs a;
    a.in = in;
    a.off = off;
    a.h1 = h1;
    a.h2 = h2;
    a.n = n;
    a.seed = seed;
    a.pairs = pairs ? 1u : 0u;
    return timed(c, QHUFF_KIND_HASH, "launch_hash",
                 [&](hipEvent_t e0, hipEvent_t e1) {
        return launch_hash(a, c->hash_grid, (hipStream_t) stream, e0, e1);
    });
}

extern "C" int
qhuff_xxh32_headers(qhuff_ctx *c, const uint8_t *in, const uint32_t *off,
                    uint32_t n, uint32_t seed, uint32_t *name_hash,
                    uint32_t *nameval_hash, void *stream)
{
    return hash_call(c, in, off, n, seed, name_hash, nameval_hash, true,
                     stream);
}

extern "C" int
qhuff_xxh32_batch(qhuff_ctx *c, const uint8_t *in, const uint32_t *in_off,
                  uint32_t n, uint32_t seed, uint32_t *hash, void *stream)
{
    return hash_call(c, in, in_off, n, seed, hash, nullptr, false, stream);
}

// The kernels' sticky error word, read from its pinned host mirror (the
// kernels set both; call once the launch's stream has been synchronised):
// no device round trip on the synchronous paths.
int
qhuff::mirror_error(qhuff_ctx *c)
{
    const uint32_t v = __atomic_exchange_n(&c->err_host[0], 0u, __ATOMIC_ACQ_REL);
    if (!v)
        return QHUFF_OK;
    (void) hipMemset(c->err, 0, 4);
    snprintf(c->err_msg, sizeof(c->err_msg), "device error %u", v);
    return QHUFF_EDEVICE;
}

// ---- resumable decode (qhuff_stream.hip) -----------------------------------

extern "C" uint64_t
qhuff_decode_stream_bound(uint64_t in_bytes, uint32_t n)
{
    // per chunk floor(8 * len / 5) + 1: the pending symbol on one bit, then
    // 5-bit codes
    return in_bytes * 8 / 5 + n + 16;
}

extern "C" int
qhuff_decode_stream(qhuff_ctx *c, const uint8_t *in, const uint32_t *in_off,
                    uint32_t n, struct qhuff_decode_status *state,
                    const uint8_t *flags, uint8_t *out, uint32_t *out_off,
                    uint8_t *status, void *stream)
{
    if (!c || !in_off || !out_off || (n && (!in || !out || !status || !state)))
        return QHUFF_EINVAL;
    hipStream_t st = (hipStream_t) stream;
    // (the lean structure, here and in the two calls below: no slots, no
    // hint consumed, the batch kernel's last variant left as it is)
    return tile_launch(c, n, decode_tile_strings(), stream_waves_per_block(),
                       c->dec_grid, out_off, st,
                       [&](const Coord &k, uint32_t grid) -> int {
        StreamArgs a;
        a.d = dec_args(c, in, in_off, out, out_off, status, n, k);
        a.nodes = c->tab->nodes;
        a.state = state;
        a.flags = flags;
        return timed(c, QHUFF_KIND_DECODE, "launch_stream",
                     [&](hipEvent_t e0, hipEvent_t e1) {
            return launch_stream(a, grid, st, e0, e1);
        });
    });
}

// ---- literals in place (qhuff_wire.hip) ------------------------------------

extern "C" int
qhuff_decode_wire(qhuff_ctx *c, const uint8_t *buf,
                  const struct qhuff_literal *lits, uint32_t n,
                  uint32_t max_len, uint8_t *out, uint32_t *out_off,
                  uint8_t *status, void *stream)
{
    if (!c || !out_off || (n && (!buf || !lits || !out || !status)))
        return QHUFF_EINVAL;
    hipStream_t st = (hipStream_t) stream;
    return tile_launch(c, n, decode_tile_strings(), wire_waves_per_block(),
                       c->dec_grid, out_off, st,
                       [&](const Coord &k, uint32_t grid) -> int {
        WireArgs a;
        // (the tile pipeline's offsets pointer: the policy reads descriptors)
        a.d = dec_args(c, buf, (const uint32_t *) lits, out, out_off, status,
                       n, k);
        a.max_len = max_len;
        return timed(c, QHUFF_KIND_DECODE, "launch_wire",
                     [&](hipEvent_t e0, hipEvent_t e1) {
            return launch_wire(a, grid, st, e0, e1);
        });
    });
}

// ---- field sections and encoder streams scanned (qhuff_scan.hip) -----------

// the scan's scratch for m chunks, and its launches on st ordered behind the
// scan launches that went out on another stream (one scratch per context)
static int
scan_prepare(qhuff_ctx *c, uint32_t m, hipStream_t st)
{
    if (!c->scan_ev)
        HIPCHK(c, hipEventCreateWithFlags(&c->scan_ev, hipEventDisableTiming));
    if (c->scan_have && st != c->scan_stream)
    {
        HIPCHK(c, hipEventRecord(c->scan_ev, c->scan_stream));
        HIPCHK(c, hipStreamWaitEvent(st, c->scan_ev, 0));
    }
    if (m > c->scan_cap)
    {
        if (c->scan_ws)
        {
            // (earlier scans may still read it)
            if (c->scan_have)
                HIPCHK(c, hipStreamSynchronize(c->scan_stream));
            HIPCHK(c, hipFree(c->scan_ws));
            c->scan_ws = nullptr;
            c->scan_cap = 0;
        }
        const uint64_t cap = m < 4096 ? 4096 : m;
        HIPCHK(c, hipMalloc((void **) &c->scan_ws,
                            4 * (cap + (cap + kScanBlock - 1) / kScanBlock)));
        c->scan_cap = cap;
    }
    return QHUFF_OK;
}

extern "C" int
qhuff_scan_sections(qhuff_ctx *c, const uint8_t *buf, const uint32_t *sec_off,
                    uint32_t m, unsigned mode, struct qhuff_literal *lits,
                    uint32_t max_lits, uint32_t *lit_off, int32_t *rc,
                    uint32_t *consumed, void *stream)
{
    if (!c || !lit_off || (mode != QHUFF_SCAN_FIELD_SECTION
                           && mode != QHUFF_SCAN_ENCODER_STREAM)
            || (m && (!buf || !sec_off || !rc
                      || (!consumed && mode == QHUFF_SCAN_ENCODER_STREAM)))
            || (max_lits && !lits))
        return QHUFF_EINVAL;
    hipStream_t st = (hipStream_t) stream;
    HIPCHK(c, hipSetDevice(c->device));
    if (m == 0)
    {
        HIPCHK(c, hipMemsetAsync(lit_off, 0, 4, st));
        return QHUFF_OK;
    }
    if (const int r = scan_prepare(c, m, st))
        return r;
    ScanArgs a;
    a.buf = buf;
    a.sec_off = sec_off;
    a.lits = lits;
    a.lit_off = lit_off;
    a.rc = rc;
    a.consumed = consumed;
    a.cnt = c->scan_ws;
    a.tot = c->scan_ws + c->scan_cap;
    a.m = m;
    a.max_lits = max_lits;
    a.mode = mode;
    for (unsigned step = 0; step < 3; ++step)
    {
        const int r = timed(c, QHUFF_KIND_SCAN, "launch_scan",
                            [&](hipEvent_t e0, hipEvent_t e1) {
            return launch_scan(a, step, st, e0, e1);
        });
        // (a launch went out: later scans on another stream wait for it)
        if (step || !r)
        {
            c->scan_stream = st;
            c->scan_have = true;
        }
        if (r)
            return r;
    }
    return QHUFF_OK;
}

// ---- header lists from field sections (qhuff_hdrscan.hip, qhuff_hdrdec.hip) -

// The literal scan's frame over the header walker: its scratch, its stream
// ordering, its top launch.
extern "C" int
qhuff_scan_headers(qhuff_ctx *c, const uint8_t *buf, const uint32_t *sec_off,
                   uint32_t m, struct qhuff_hstr *strs, uint32_t max_hdrs,
                   uint32_t *hdr_off, int32_t *rc, uint8_t *kind,
                   uint8_t *static_id, uint8_t *hflags, void *stream)
{
    if (!c || !hdr_off || (m && (!buf || !sec_off || !rc))
            || (max_hdrs && !strs))
        return QHUFF_EINVAL;
    hipStream_t st = (hipStream_t) stream;
    HIPCHK(c, hipSetDevice(c->device));
    if (m == 0)
    {
        HIPCHK(c, hipMemsetAsync(hdr_off, 0, 4, st));
        return QHUFF_OK;
    }
    if (const int r = scan_prepare(c, m, st))
        return r;
    HdrScanArgs a;
    a.buf = buf;
    a.sec_off = sec_off;
    a.strs = strs;
    a.hdr_off = hdr_off;
    a.rc = rc;
    a.kind = kind;
    a.static_id = static_id;
    a.hflags = hflags;
    a.cnt = c->scan_ws;
    a.tot = c->scan_ws + c->scan_cap;
    a.m = m;
    a.max_hdrs = max_hdrs;
    ScanArgs top = {};                   // (the top launch reads tot and m)
    top.tot = a.tot;
    top.m = m;
    for (unsigned step = 0; step < 3; ++step)
    {
        const int r = timed(c, QHUFF_KIND_SCAN, "launch_hdrscan",
                            [&](hipEvent_t e0, hipEvent_t e1) {
            return step == 1 ? launch_scan(top, 1, st, e0, e1)
                             : launch_hdrscan(a, step, st, e0, e1);
        });
        if (step || !r)
        {
            c->scan_stream = st;
            c->scan_have = true;
        }
        if (r)
            return r;
    }
    return QHUFF_OK;
}

extern "C" uint64_t
qhuff_decode_headers_bound(uint64_t wire_bytes, uint32_t n)
{
    // the literals as qhuff_decode_bound; per header the longest static name
    // + value (qhuff_hdrdec_impl.h asserts the 76)
    return wire_bytes * 8 / 5 + 76ull * n + 16;
}

extern "C" int
qhuff_decode_headers(qhuff_ctx *c, const uint8_t *buf,
                     const struct qhuff_hstr *strs, uint32_t n,
                     uint32_t max_len, uint8_t *out, uint32_t *off,
                     uint8_t *status, void *stream)
{
    if (!c || !off || (n && (!buf || !strs || !out || !status)))
        return QHUFF_EINVAL;
    if (n > 0x7fffffffu)
        return QHUFF_ERANGE;
    hipStream_t st = (hipStream_t) stream;
    // (one string a lane: 2n strings, a tile 32 whole headers)
    return tile_launch(c, 2 * n, decode_tile_strings(),
                       hdrdec_waves_per_block(), c->dec_grid, off, st,
                       [&](const Coord &k, uint32_t grid) -> int {
        WireArgs a;
        a.d = dec_args(c, buf, (const uint32_t *) strs, out, off, status,
                       2 * n, k);
        a.max_len = max_len;
        return timed(c, QHUFF_KIND_DECODE, "launch_hdrdec",
                     [&](hipEvent_t e0, hipEvent_t e1) {
            return launch_hdrdec(a, grid, st, e0, e1);
        });
    });
}

// ---- ... against the dynamic table's entries (qhuff_hdrscan_dyn.hip,
// qhuff_hdrdec_dyn.hip) --------------------------------------------------------

// qhuff_scan_headers' frame over the walker with a table: the same scratch,
// the same order, the same top launch.
extern "C" int
qhuff_scan_headers_dyn(qhuff_ctx *c, const uint8_t *buf,
                       const uint32_t *sec_off, uint32_t m,
                       const struct qhuff_dyn_table *tab,
                       const uint32_t *sec_win, struct qhuff_hstr *strs,
                       uint32_t max_hdrs, uint32_t *hdr_off, int32_t *rc,
                       uint8_t *kind, uint8_t *static_id, uint8_t *hflags,
                       uint32_t *dyn_id, void *stream)
{
    if (!c || !hdr_off || !tab || (tab->d && !tab->off)
            || (m && (!buf || !sec_off || !rc)) || (max_hdrs && !strs))
        return QHUFF_EINVAL;
    hipStream_t st = (hipStream_t) stream;
    HIPCHK(c, hipSetDevice(c->device));
    if (m == 0)
    {
        HIPCHK(c, hipMemsetAsync(hdr_off, 0, 4, st));
        return QHUFF_OK;
    }
    if (const int r = scan_prepare(c, m, st))
        return r;
    HdrScanDynArgs a;
    a.h.buf = buf;
    a.h.sec_off = sec_off;
    a.h.strs = strs;
    a.h.hdr_off = hdr_off;
    a.h.rc = rc;
    a.h.kind = kind;
    a.h.static_id = static_id;
    a.h.hflags = hflags;
    a.h.cnt = c->scan_ws;
    a.h.tot = c->scan_ws + c->scan_cap;
    a.h.m = m;
    a.h.max_hdrs = max_hdrs;
    a.off = tab->off;
    a.sec_win = sec_win;
    a.dyn_id = dyn_id;
    a.d = tab->d;
    a.first = tab->first;
    a.max_entries = tab->max_entries;
    ScanArgs top = {};                   // (the top launch reads tot and m)
    top.tot = a.h.tot;
    top.m = m;
    for (unsigned step = 0; step < 3; ++step)
    {
        const int r = timed(c, QHUFF_KIND_SCAN, "launch_hdrscan_dyn",
                            [&](hipEvent_t e0, hipEvent_t e1) {
            return step == 1 ? launch_scan(top, 1, st, e0, e1)
                             : launch_hdrscan_dyn(a, step, st, e0, e1);
        });
        if (step || !r)
        {
            c->scan_stream = st;
            c->scan_have = true;
        }
        if (r)
            return r;
    }
    return QHUFF_OK;
}

extern "C" uint64_t
qhuff_decode_headers_dyn_bound(uint64_t wire_bytes, uint32_t n,
                               uint32_t dyn_longest)
{
    // qhuff_decode_headers_bound, a header's fixed text the longer of the
    // longest static and the longest dynamic entry
    return wire_bytes * 8 / 5 + (dyn_longest > 76 ? dyn_longest : 76ull) * n
         + 16;
}

extern "C" int
qhuff_decode_headers_dyn(qhuff_ctx *c, const uint8_t *buf,
                         const struct qhuff_hstr *strs, uint32_t n,
                         uint32_t max_len, const uint8_t *dyn_bytes,
                         uint32_t dyn_len, uint8_t *out, uint32_t *off,
                         uint8_t *status, void *stream)
{
    if (!c || !off || (n && (!buf || !strs || !out || !status))
            || (dyn_len && !dyn_bytes))
        return QHUFF_EINVAL;
    if (n > 0x7fffffffu)
        return QHUFF_ERANGE;
    hipStream_t st = (hipStream_t) stream;
    return tile_launch(c, 2 * n, decode_tile_strings(),
                       hdrdec_dyn_waves_per_block(), c->dec_grid, off, st,
                       [&](const Coord &k, uint32_t grid) -> int {
        HdrDynArgs a;
        a.w.d = dec_args(c, buf, (const uint32_t *) strs, out, off, status,
                         2 * n, k);
        a.w.max_len = max_len;
        a.dyn = dyn_bytes;
        a.dyn_len = dyn_len;
        return timed(c, QHUFF_KIND_DECODE, "launch_hdrdec_dyn",
                     [&](hipEvent_t e0, hipEvent_t e1) {
            return launch_hdrdec_dyn(a, grid, st, e0, e1);
        });
    });
}

// ---- items encoded in one launch (qhuff_encwire.hip) -----------------------

extern "C" uint64_t
qhuff_encode_wire_bound(uint64_t in_bytes, uint32_t n)
{
    // per item: 1 byte of rounding, 6 of prefixed length, 6 of integer
    return (in_bytes * 30 + 7) / 8 + 13ull * n + 16;
}

extern "C" int
qhuff_items_check(const struct qhuff_item *items, uint32_t n, uint32_t *bad)
{
    if (n && !items)
        return QHUFF_EINVAL;
    for (uint32_t i = 0; i < n; ++i)
    {
        const struct qhuff_item &t = items[i];
        const unsigned ib = t.int_bits, sb = t.str_bits;
        // (an unused part's *_first: every bit counts)
        const bool ok = ib <= 8
                     && !(t.int_first & (ib ? (1u << ib) - 1 : 0xffu))
                     && (sb == 0 || sb == 3 || sb == 5 || sb == 7)
                     && !(t.str_first & (sb ? (2u << sb) - 1 : 0xffu));
        if (!ok)
        {
            if (bad)
                *bad = i;
            return QHUFF_EINVAL;
        }
    }
    return QHUFF_OK;
}

extern "C" int
qhuff_encode_wire(qhuff_ctx *c, const uint8_t *in, const uint32_t *in_off,
                  const struct qhuff_item *items, uint32_t n, uint8_t *out,
                  uint32_t *out_off, void *stream)
{
    if (!c || !out_off || (n && (!in || !in_off || !items || !out)))
        return QHUFF_EINVAL;
    hipStream_t st = (hipStream_t) stream;
    return tile_launch(c, n, kWT, encwire_waves_per_block(), c->enc_grid,
                       out_off, st, [&](const Coord &k, uint32_t grid) -> int {
        // (mode unused: every item has its own framing)
        const EncArgs a = enc_args(c, in, in_off, out, out_off, n, 0, k);
        return timed(c, QHUFF_KIND_ENCODE, "launch_encwire",
                     [&](hipEvent_t e0, hipEvent_t e1) {
            return launch_encwire(a, items, grid, st, e0, e1);
        });
    });
}

// ---- headers against the static table (qhuff_lookup.hip) -------------------

static LookupArgs
lookup_args(const uint8_t *in, const uint32_t *off, uint32_t n,
            uint32_t *h1, uint32_t *h2, uint8_t *kind, uint8_t *id)
{
    LookupArgs a = {};
    a.in = in;
    a.off = off;
    a.h1 = h1;
    a.h2 = h2;
    a.kind = kind;
    a.id = id;
    a.n = n;
    return a;
}

// (the grid is the hash kernel's resident one, from hash_occupancy: the
// lookup kernel has the hash kernel's LDS frame and, today, its occupancy --
// 79 VGPRs, three workgroups a CU.  Should it grow past that, it needs an
// occupancy query of its own to stay resident; any grid is correct.)
static int
lookup_launch(qhuff_ctx *c, const LookupArgs &a, hipStream_t st)
{
    return timed(c, QHUFF_KIND_HASH, "launch_lookup",
                 [&](hipEvent_t e0, hipEvent_t e1) {
        return launch_lookup(a, c->hash_grid, st, e0, e1);
    });
}

extern "C" int
qhuff_static_lookup(qhuff_ctx *c, const uint8_t *in, const uint32_t *off,
                    uint32_t n, uint32_t *name_hash, uint32_t *nameval_hash,
                    uint8_t *kind, uint8_t *static_id, void *stream)
{
    if (!c || !off || (n && (!in || !kind || !static_id)))
        return QHUFF_EINVAL;
    if (n > 0x7fffffffu)
        return QHUFF_ERANGE;
    HIPCHK(c, hipSetDevice(c->device));
    if (n == 0)
        return QHUFF_OK;
    return lookup_launch(c, lookup_args(in, off, n, name_hash, nameval_hash,
                                        kind, static_id),
                         (hipStream_t) stream);
}

extern "C" uint64_t
qhuff_encode_headers_bound(uint64_t in_bytes, uint32_t n, uint32_t m)
{
    // two items a header and two a section prefix; above 32 bits (which the
    // calls reject) the count saturates, and so does the bound
    const uint64_t items = 2ull * n + 2ull * m;
    if (items > 0xffffffffull)
        return ~0ull;
    return qhuff_encode_wire_bound(in_bytes, (uint32_t) items);
}

static inline size_t
hdr_up16(size_t x)
{
    return (x + 15) & ~(size_t) 15;
}

// the scratch for `items` items, and this call's launches on st ordered
// behind those that went out on another stream (one scratch per context)
static int
hdr_prepare(qhuff_ctx *c, uint64_t items, hipStream_t st)
{
    if (!c->hdr_ev)
        HIPCHK(c, hipEventCreateWithFlags(&c->hdr_ev, hipEventDisableTiming));
    if (c->hdr_have && st != c->hdr_stream)
    {
        HIPCHK(c, hipEventRecord(c->hdr_ev, c->hdr_stream));
        HIPCHK(c, hipStreamWaitEvent(st, c->hdr_ev, 0));
    }
    if (items > c->hdr_cap)
    {
        if (c->hdr_ws)
        {
            // (earlier calls may still use it)
            if (c->hdr_have)
                HIPCHK(c, hipStreamSynchronize(c->hdr_stream));
            HIPCHK(c, hipFree(c->hdr_ws));
            c->hdr_ws = nullptr;
            c->hdr_cap = 0;
        }
        const uint64_t cap = items < 4096 ? 4096 : items;
        HIPCHK(c, hipMalloc((void **) &c->hdr_ws,
                            8 * cap + 2 * hdr_up16(4 * (cap + 1))));
        c->hdr_cap = cap;
    }
    return QHUFF_OK;
}

extern "C" int
qhuff_encode_headers(qhuff_ctx *c, const uint8_t *in, const uint32_t *off,
                     uint32_t n, const uint8_t *hflags,
                     const uint32_t *sec_hdr, uint32_t m, uint8_t *out,
                     uint32_t *sec_out, uint8_t *kind, uint8_t *static_id,
                     void *stream)
{
    if (!c || !off || !sec_hdr || !sec_out || (n && !in) || ((n || m) && !out))
        return QHUFF_EINVAL;
    const uint64_t items = 2ull * n + 2ull * m;
    if (items > 0xffffffffull)
        return QHUFF_ERANGE;
    hipStream_t st = (hipStream_t) stream;
    HIPCHK(c, hipSetDevice(c->device));
    if (items == 0)
    {
        HIPCHK(c, hipMemsetAsync(sec_out, 0, 4, st));
        return QHUFF_OK;
    }
    // (headers without a section: sec_hdr[0] = 0 != n, the caller's breach)
    if (m == 0)
        return QHUFF_EINVAL;
    if (n == 0)
    {
        // (no header: the sections are their prefixes, the strings unread)
        HIPCHK(c, launch_empty_sections(m, out, sec_out, st));
        return QHUFF_OK;
    }
    if (const int r = hdr_prepare(c, items, st))
        return r;
    LookupArgs a = lookup_args(in, off, n, nullptr, nullptr, kind, static_id);
    a.hflags = hflags;
    a.sec_hdr = sec_hdr;
    a.m = m;
    a.items = (struct qhuff_item *) c->hdr_ws;
    a.str_off = (uint32_t *) (c->hdr_ws + 8 * c->hdr_cap);
    uint32_t *item_off = (uint32_t *) (c->hdr_ws + 8 * c->hdr_cap
                                       + hdr_up16(4 * (c->hdr_cap + 1)));
    int r = lookup_launch(c, a, st);
    if (r)
        return r;
    // (a launch went out: later calls on another stream wait for it)
    c->hdr_stream = st;
    c->hdr_have = true;
    r = qhuff_encode_wire(c, in, a.str_off, a.items, (uint32_t) items, out,
                          item_off, st);
    if (r)
        return r;
    HIPCHK(c, launch_secout(item_off, sec_hdr, m, n, sec_out, st));
    return QHUFF_OK;
}

// ---- ... and among the dynamic table's entries (qhuff_lookup_dyn.hip) --------

extern "C" uint64_t
qhuff_encode_headers_dyn_bound(uint64_t in_bytes, uint32_t n, uint32_t m)
{
    // (the same items; a prefix's two integers fit an item's 13 bytes)
    return qhuff_encode_headers_bound(in_bytes, n, m);
}

// what the device forms can check of a table: a host struct
static int
dyn_tab_ok(const struct qhuff_dyn_table *tab)
{
    if (!tab || (tab->d && (!tab->off || !tab->bytes)))
        return QHUFF_EINVAL;
    if ((uint64_t) tab->first + tab->d > 0xffffffffull || tab->d > kDynMaxD)
        return QHUFF_ERANGE;
    return QHUFF_OK;
}

// dyn_ws grown to `words` words and that many cleared on st
static int
dyn_scratch(qhuff_ctx *c, uint64_t words, hipStream_t st)
{
    if (words > c->dyn_cap)
    {
        if (c->dyn_ws)
        {
            // (earlier calls may still use it)
            if (c->hdr_have)
                HIPCHK(c, hipStreamSynchronize(c->hdr_stream));
            HIPCHK(c, hipFree(c->dyn_ws));
            c->dyn_ws = nullptr;
            c->dyn_cap = 0;
        }
        const uint64_t cap = words < 4096 ? 4096 : words;
        HIPCHK(c, hipMalloc((void **) &c->dyn_ws, 4 * cap));
        c->dyn_cap = cap;
    }
    if (words)
        HIPCHK(c, hipMemsetAsync(c->dyn_ws, 0, 4 * words, st));
    return QHUFF_OK;
}

// The dynamic lookup's scratch for m sections and a table of d entries --
// [ric: m words | the two indices: qhuff_dyn_index_slots(d) words each, none
// when d = 0], cleared on st -- and the table's part of the arguments.
// After hdr_prepare: the scratch is ordered across streams with hdr_ws, by
// the same event.
static int
dyn_prepare(qhuff_ctx *c, const struct qhuff_dyn_table *tab, uint32_t m,
            hipStream_t st, DynLookupArgs *a)
{
    const uint64_t slots = tab->d ? dyn_index_slots(tab->d) : 0;
    if (const int r = dyn_scratch(c, (uint64_t) m + 2 * slots, st))
        return r;
    a->tab = tab->d ? tab->bytes : nullptr;
    a->tab_off = tab->d ? tab->off : nullptr;
    a->ric = c->dyn_ws;
    a->nv = slots ? c->dyn_ws + m : nullptr;
    a->nm = slots ? c->dyn_ws + m + slots : nullptr;
    a->mask = slots ? (uint32_t) slots - 1 : 0;
    a->d = tab->d;
    a->first = tab->first;
    a->max_entries = tab->max_entries;
    a->win_lo = tab->first;
    a->win_hi = tab->first + tab->d;
    return QHUFF_OK;
}

// the index build (d != 0) and the lookup, on st
static int
dyn_launches(qhuff_ctx *c, const DynLookupArgs &a, hipStream_t st)
{
    if (a.d)
    {
        const int r = timed(c, QHUFF_KIND_HASH, "launch_dyn_index",
                            [&](hipEvent_t e0, hipEvent_t e1) {
            return launch_dyn_index(a, st, e0, e1);
        });
        // (a launch went out: later calls on another stream wait for it)
        c->hdr_stream = st;
        c->hdr_have = true;
        if (r)
            return r;
    }
    const bool enc = a.l.items != nullptr;
    if (!c->dyn_grid[enc])
    {
        // (the workgroups of this kernel that fit at once, as hash_grid is
        // the hash kernel's; any grid is correct)
        int occ = 0;
        HIPCHK(c, lookup_dyn_occupancy(enc, &occ));
        c->dyn_grid[enc] = (uint32_t) (occ > 0 ? occ : 1) * (uint32_t) c->n_cu;
    }
    const int r = timed(c, QHUFF_KIND_HASH, "launch_lookup_dyn",
                        [&](hipEvent_t e0, hipEvent_t e1) {
        return launch_lookup_dyn(a, c->dyn_grid[enc], st, e0, e1);
    });
    if (!r)
    {
        c->hdr_stream = st;
        c->hdr_have = true;
    }
    return r;
}

extern "C" int
qhuff_dyn_lookup(qhuff_ctx *c, const uint8_t *in, const uint32_t *off,
                 uint32_t n, const struct qhuff_dyn_table *tab,
                 uint32_t win_lo, uint32_t win_hi, uint32_t *name_hash,
                 uint32_t *nameval_hash, uint8_t *kind, uint8_t *static_id,
                 uint32_t *dyn_id, void *stream)
{
    if (!c || !off || (n && (!in || !kind || !static_id)))
        return QHUFF_EINVAL;
    if (const int r = dyn_tab_ok(tab))
        return r;
    if (n > 0x7fffffffu)
        return QHUFF_ERANGE;
    hipStream_t st = (hipStream_t) stream;
    HIPCHK(c, hipSetDevice(c->device));
    if (n == 0)
        return QHUFF_OK;
    if (const int r = hdr_prepare(c, 0, st))
        return r;
    DynLookupArgs a = {};
    a.l = lookup_args(in, off, n, name_hash, nameval_hash, kind, static_id);
    a.dyn_id = dyn_id;
    if (const int r = dyn_prepare(c, tab, 0, st, &a))
        return r;
    a.win_lo = win_lo;
    a.win_hi = win_hi;
    return dyn_launches(c, a, st);
}

extern "C" int
qhuff_encode_headers_dyn(qhuff_ctx *c, const uint8_t *in, const uint32_t *off,
                         uint32_t n, const uint8_t *hflags,
                         const uint32_t *sec_hdr, uint32_t m,
                         const struct qhuff_dyn_table *tab,
                         const uint32_t *sec_win, const uint32_t *sec_base,
                         uint8_t *out, uint32_t *sec_out, uint8_t *kind,
                         uint8_t *static_id, uint32_t *dyn_id, void *stream)
{
    if (!c || !off || !sec_hdr || !sec_out || (n && !in) || ((n || m) && !out))
        return QHUFF_EINVAL;
    if (const int r = dyn_tab_ok(tab))
        return r;
    const uint64_t items = 2ull * n + 2ull * m;
    if (items > 0xffffffffull)
        return QHUFF_ERANGE;
    hipStream_t st = (hipStream_t) stream;
    HIPCHK(c, hipSetDevice(c->device));
    if (items == 0)
    {
        HIPCHK(c, hipMemsetAsync(sec_out, 0, 4, st));
        return QHUFF_OK;
    }
    // (headers without a section: sec_hdr[0] = 0 != n, the caller's breach)
    if (m == 0)
        return QHUFF_EINVAL;
    if (n == 0)
    {
        // (no header, no reference: every section is 00 00)
        HIPCHK(c, launch_empty_sections(m, out, sec_out, st));
        return QHUFF_OK;
    }
    if (const int r = hdr_prepare(c, items, st))
        return r;
    DynLookupArgs a = {};
    a.l = lookup_args(in, off, n, nullptr, nullptr, kind, static_id);
    a.l.hflags = hflags;
    a.l.sec_hdr = sec_hdr;
    a.l.m = m;
    a.l.items = (struct qhuff_item *) c->hdr_ws;
    a.l.str_off = (uint32_t *) (c->hdr_ws + 8 * c->hdr_cap);
    uint32_t *item_off = (uint32_t *) (c->hdr_ws + 8 * c->hdr_cap
                                       + hdr_up16(4 * (c->hdr_cap + 1)));
    a.sec_win = sec_win;
    a.sec_base = sec_base;
    a.dyn_id = dyn_id;
    if (const int r = dyn_prepare(c, tab, m, st, &a))
        return r;
    int r = dyn_launches(c, a, st);
    if (r)
        return r;
    r = timed(c, QHUFF_KIND_HASH, "launch_dyn_prefix",
              [&](hipEvent_t e0, hipEvent_t e1) {
        return launch_dyn_prefix(a, st, e0, e1);
    });
    if (r)
        return r;
    r = qhuff_encode_wire(c, in, a.l.str_off, a.l.items, (uint32_t) items, out,
                          item_off, st);
    if (r)
        return r;
    HIPCHK(c, launch_secout(item_off, sec_hdr, m, n, sec_out, st));
    return QHUFF_OK;
}

// ---- ... over a set of tables, a table per section ---------------------------
// (qhuff_hdrscan_tabs.hip, qhuff_lookup_tabs.hip)

// what the device forms can check of a set: a host struct
static int
tabs_ok(const struct qhuff_dyn_tables *t, const uint32_t *sec_tab, uint32_t m)
{
    if (!t || (t->T && (!t->ent || !t->first || !t->max_entries
                        || (m && !sec_tab))))
        return QHUFF_EINVAL;
    return QHUFF_OK;
}

// qhuff_scan_headers_dyn's frame over the walker with a table per section.
// (D is not known here: the kernels read ent[T]; off may be null only when
// T = 0.)
extern "C" int
qhuff_scan_headers_tabs(qhuff_ctx *c, const uint8_t *buf,
                        const uint32_t *sec_off, uint32_t m,
                        const struct qhuff_dyn_tables *tabs,
                        const uint32_t *sec_tab, const uint32_t *sec_win,
                        struct qhuff_hstr *strs, uint32_t max_hdrs,
                        uint32_t *hdr_off, int32_t *rc, uint8_t *kind,
                        uint8_t *static_id, uint8_t *hflags, uint32_t *dyn_id,
                        void *stream)
{
    if (!c || !hdr_off || (m && (!buf || !sec_off || !rc))
            || (max_hdrs && !strs))
        return QHUFF_EINVAL;
    if (const int r = tabs_ok(tabs, sec_tab, m))
        return r;
    if (tabs->T && !tabs->off)
        return QHUFF_EINVAL;
    hipStream_t st = (hipStream_t) stream;
    HIPCHK(c, hipSetDevice(c->device));
    if (m == 0)
    {
        HIPCHK(c, hipMemsetAsync(hdr_off, 0, 4, st));
        return QHUFF_OK;
    }
    if (const int r = scan_prepare(c, m, st))
        return r;
    HdrScanTabsArgs a;
    a.h.buf = buf;
    a.h.sec_off = sec_off;
    a.h.strs = strs;
    a.h.hdr_off = hdr_off;
    a.h.rc = rc;
    a.h.kind = kind;
    a.h.static_id = static_id;
    a.h.hflags = hflags;
    a.h.cnt = c->scan_ws;
    a.h.tot = c->scan_ws + c->scan_cap;
    a.h.m = m;
    a.h.max_hdrs = max_hdrs;
    a.off = tabs->off;
    a.ent = tabs->ent;
    a.first = tabs->first;
    a.max_entries = tabs->max_entries;
    a.sec_tab = tabs->T ? sec_tab : nullptr;
    a.sec_win = sec_win;
    a.dyn_id = dyn_id;
    a.T = tabs->T;
    ScanArgs top = {};                   // (the top launch reads tot and m)
    top.tot = a.h.tot;
    top.m = m;
    for (unsigned step = 0; step < 3; ++step)
    {
        const int r = timed(c, QHUFF_KIND_SCAN, "launch_hdrscan_tabs",
                            [&](hipEvent_t e0, hipEvent_t e1) {
            return step == 1 ? launch_scan(top, 1, st, e0, e1)
                             : launch_hdrscan_tabs(a, step, st, e0, e1);
        });
        if (step || !r)
        {
            c->scan_stream = st;
            c->scan_have = true;
        }
        if (r)
            return r;
    }
    return QHUFF_OK;
}

// D = ent[T] of a set in device memory: one 4-byte copy on st, waited for
static int
tabs_read_entries(qhuff_ctx *c, const struct qhuff_dyn_tables *t,
                  hipStream_t st, uint32_t *D)
{
    *D = 0;
    if (!t->T)
        return QHUFF_OK;
    HIPCHK(c, hipMemcpyAsync(D, t->ent + t->T, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    return QHUFF_OK;
}

// The tabs lookup's scratch -- dyn_prepare's layout with one pair of indices
// over all D entries -- and the set's part of the arguments.  After
// hdr_prepare.
static int
tabs_prepare(qhuff_ctx *c, const struct qhuff_dyn_tables *t, uint32_t D,
             const uint32_t *sec_tab, uint32_t ric_words, hipStream_t st,
             TabsLookupArgs *a)
{
    if (D > kDynMaxD)
        return QHUFF_ERANGE;
    if (D && (!t->off || !t->bytes))
        return QHUFF_EINVAL;
    const uint64_t slots = D ? dyn_index_slots(D) : 0;
    if (const int r = dyn_scratch(c, (uint64_t) ric_words + 2 * slots, st))
        return r;
    a->tab = D ? t->bytes : nullptr;
    a->tab_off = D ? t->off : nullptr;
    a->ent = t->ent;
    a->first = t->first;
    a->max_entries = t->max_entries;
    a->sec_tab = t->T ? sec_tab : nullptr;
    a->ric = c->dyn_ws;
    a->nv = slots ? c->dyn_ws + ric_words : nullptr;
    a->nm = slots ? c->dyn_ws + ric_words + slots : nullptr;
    a->mask = slots ? (uint32_t) slots - 1 : 0;
    a->T = t->T;
    a->D = D;
    return QHUFF_OK;
}

// the index build (D != 0) and the lookup, on st
static int
tabs_launches(qhuff_ctx *c, const TabsLookupArgs &a, hipStream_t st)
{
    if (a.D)
    {
        const int r = timed(c, QHUFF_KIND_HASH, "launch_tabs_index",
                            [&](hipEvent_t e0, hipEvent_t e1) {
            return launch_tabs_index(a, st, e0, e1);
        });
        // (a launch went out: later calls on another stream wait for it)
        c->hdr_stream = st;
        c->hdr_have = true;
        if (r)
            return r;
    }
    const bool enc = a.l.items != nullptr;
    if (!c->tabs_grid[enc])
    {
        // (the workgroups of this kernel that fit at once; any grid is
        // correct)
        int occ = 0;
        HIPCHK(c, lookup_tabs_occupancy(enc, &occ));
        c->tabs_grid[enc] = (uint32_t) (occ > 0 ? occ : 1) * (uint32_t) c->n_cu;
    }
    const int r = timed(c, QHUFF_KIND_HASH, "launch_lookup_tabs",
                        [&](hipEvent_t e0, hipEvent_t e1) {
        return launch_lookup_tabs(a, c->tabs_grid[enc], st, e0, e1);
    });
    if (!r)
    {
        c->hdr_stream = st;
        c->hdr_have = true;
    }
    return r;
}

// qhuff_dyn_lookup_tabs after its checks, D known (the host form knows it)
int
qhuff::tabs_lookup_dev(qhuff_ctx *c, const uint8_t *in, const uint32_t *off,
                       uint32_t n, const uint32_t *sec_hdr, uint32_t m,
                       const struct qhuff_dyn_tables *tabs, uint32_t D,
                       const uint32_t *sec_tab, const uint32_t *sec_win,
                       uint32_t *name_hash, uint32_t *nameval_hash,
                       uint8_t *kind, uint8_t *static_id, uint32_t *dyn_id,
                       hipStream_t st)
{
    if (const int r = hdr_prepare(c, 0, st))
        return r;
    TabsLookupArgs a = {};
    a.l = lookup_args(in, off, n, name_hash, nameval_hash, kind, static_id);
    a.l.sec_hdr = sec_hdr;
    a.l.m = m;
    a.sec_win = sec_win;
    a.dyn_id = dyn_id;
    if (const int r = tabs_prepare(c, tabs, D, sec_tab, 0, st, &a))
        return r;
    return tabs_launches(c, a, st);
}

extern "C" int
qhuff_dyn_lookup_tabs(qhuff_ctx *c, const uint8_t *in, const uint32_t *off,
                      uint32_t n, const uint32_t *sec_hdr, uint32_t m,
                      const struct qhuff_dyn_tables *tabs,
                      const uint32_t *sec_tab, const uint32_t *sec_win,
                      uint32_t *name_hash, uint32_t *nameval_hash,
                      uint8_t *kind, uint8_t *static_id, uint32_t *dyn_id,
                      void *stream)
{
    if (!c || !off || !sec_hdr || (n && (!in || !kind || !static_id)))
        return QHUFF_EINVAL;
    if (const int r = tabs_ok(tabs, sec_tab, m))
        return r;
    if (n > 0x7fffffffu)
        return QHUFF_ERANGE;
    hipStream_t st = (hipStream_t) stream;
    HIPCHK(c, hipSetDevice(c->device));
    if (n == 0)
        return QHUFF_OK;
    // (headers without a section: sec_hdr[0] = 0 != n, the caller's breach)
    if (m == 0)
        return QHUFF_EINVAL;
    uint32_t D;
    if (const int r = tabs_read_entries(c, tabs, st, &D))
        return r;
    return tabs_lookup_dev(c, in, off, n, sec_hdr, m, tabs, D, sec_tab,
                           sec_win, name_hash, nameval_hash, kind, static_id,
                           dyn_id, st);
}

// qhuff_encode_headers_tabs after its checks, D known; n and m not 0
int
qhuff::tabs_encode_dev(qhuff_ctx *c, const uint8_t *in, const uint32_t *off,
                       uint32_t n, const uint8_t *hflags,
                       const uint32_t *sec_hdr, uint32_t m,
                       const struct qhuff_dyn_tables *tabs, uint32_t D,
                       const uint32_t *sec_tab, const uint32_t *sec_win,
                       const uint32_t *sec_base, uint8_t *out,
                       uint32_t *sec_out, uint8_t *kind, uint8_t *static_id,
                       uint32_t *dyn_id, hipStream_t st)
{
    const uint64_t items = 2ull * n + 2ull * m;
    if (const int r = hdr_prepare(c, items, st))
        return r;
    TabsLookupArgs a = {};
    a.l = lookup_args(in, off, n, nullptr, nullptr, kind, static_id);
    a.l.hflags = hflags;
    a.l.sec_hdr = sec_hdr;
    a.l.m = m;
    a.l.items = (struct qhuff_item *) c->hdr_ws;
    a.l.str_off = (uint32_t *) (c->hdr_ws + 8 * c->hdr_cap);
    uint32_t *item_off = (uint32_t *) (c->hdr_ws + 8 * c->hdr_cap
                                       + hdr_up16(4 * (c->hdr_cap + 1)));
    a.sec_win = sec_win;
    a.sec_base = sec_base;
    a.dyn_id = dyn_id;
    if (const int r = tabs_prepare(c, tabs, D, sec_tab, m, st, &a))
        return r;
    int r = tabs_launches(c, a, st);
    if (r)
        return r;
    r = timed(c, QHUFF_KIND_HASH, "launch_tabs_prefix",
              [&](hipEvent_t e0, hipEvent_t e1) {
        return launch_tabs_prefix(a, st, e0, e1);
    });
    if (r)
        return r;
    r = qhuff_encode_wire(c, in, a.l.str_off, a.l.items, (uint32_t) items, out,
                          item_off, st);
    if (r)
        return r;
    HIPCHK(c, launch_secout(item_off, sec_hdr, m, n, sec_out, st));
    return QHUFF_OK;
}

extern "C" int
qhuff_encode_headers_tabs(qhuff_ctx *c, const uint8_t *in, const uint32_t *off,
                          uint32_t n, const uint8_t *hflags,
                          const uint32_t *sec_hdr, uint32_t m,
                          const struct qhuff_dyn_tables *tabs,
                          const uint32_t *sec_tab, const uint32_t *sec_win,
                          const uint32_t *sec_base, uint8_t *out,
                          uint32_t *sec_out, uint8_t *kind, uint8_t *static_id,
                          uint32_t *dyn_id, void *stream)
{
    if (!c || !off || !sec_hdr || !sec_out || (n && !in) || ((n || m) && !out))
        return QHUFF_EINVAL;
    if (const int r = tabs_ok(tabs, sec_tab, m))
        return r;
    const uint64_t items = 2ull * n + 2ull * m;
    if (items > 0xffffffffull)
        return QHUFF_ERANGE;
    hipStream_t st = (hipStream_t) stream;
    HIPCHK(c, hipSetDevice(c->device));
    if (items == 0)
    {
        HIPCHK(c, hipMemsetAsync(sec_out, 0, 4, st));
        return QHUFF_OK;
    }
    // (headers without a section: sec_hdr[0] = 0 != n, the caller's breach)
    if (m == 0)
        return QHUFF_EINVAL;
    if (n == 0)
    {
        // (no header, no reference: every section is 00 00)
        HIPCHK(c, launch_empty_sections(m, out, sec_out, st));
        return QHUFF_OK;
    }
    uint32_t D;
    if (const int r = tabs_read_entries(c, tabs, st, &D))
        return r;
    return tabs_encode_dev(c, in, off, n, hflags, sec_hdr, m, tabs, D, sec_tab,
                           sec_win, sec_base, out, sec_out, kind, static_id,
                           dyn_id, st);
}

// ---- encoder-stream inserts applied to a set of tables -----------------------
// (qhuff_insscan_tabs.hip, qhuff_insapply_tabs.hip)

static inline size_t
ins_up16(size_t x)
{
    return (x + 15) & ~(size_t) 15;
}

// the scan's frame over the insert walker: its scratch, its stream ordering,
// its top launch
extern "C" int
qhuff_scan_inserts_tabs(qhuff_ctx *c, const struct qhuff_dyn_tables *tabs,
                        const struct qhuff_ins_state *s, const uint8_t *buf,
                        const uint32_t *enc_off,
                        const struct qhuff_ins_scan *sc, void *stream)
{
    if (!c || !tabs || !s || !sc || !sc->ins_off)
        return QHUFF_EINVAL;
    const uint32_t T = tabs->T;
    if (T && (!tabs->ent || !tabs->first || !tabs->off || !s->cap
              || !s->max_cap || !buf || !enc_off || !sc->rc || !sc->consumed
              || !sc->chunk_cap))
        return QHUFF_EINVAL;
    if (sc->max_ins && (!sc->strs || !sc->root || !sc->ins_cap || !sc->ins_ref
                        || !sc->ins_kind))
        return QHUFF_EINVAL;
    if (sc->max_ins > 0x7fffffffu)
        return QHUFF_ERANGE;
    hipStream_t st = (hipStream_t) stream;
    HIPCHK(c, hipSetDevice(c->device));
    if (T == 0)
    {
        HIPCHK(c, hipMemsetAsync(sc->ins_off, 0, 4, st));
        return QHUFF_OK;
    }
    if (const int r = scan_prepare(c, T, st))
        return r;
    InsScanArgs a;
    a.buf = buf;
    a.sec_off = enc_off;
    a.off = tabs->off;
    a.ent = tabs->ent;
    a.first = tabs->first;
    a.cap = s->cap;
    a.max_cap = s->max_cap;
    a.rc = sc->rc;
    a.consumed = sc->consumed;
    a.ins_off = sc->ins_off;
    a.chunk_cap = sc->chunk_cap;
    a.strs = sc->strs;
    a.root = sc->root;
    a.ins_cap = sc->ins_cap;
    a.ins_ref = sc->ins_ref;
    a.ins_kind = sc->ins_kind;
    a.cnt = c->scan_ws;
    a.tot = c->scan_ws + c->scan_cap;
    a.m = T;
    a.max_ins = sc->max_ins;
    ScanArgs top = {};                   // (the top launch reads tot and m)
    top.tot = a.tot;
    top.m = T;
    for (unsigned step = 0; step < 3; ++step)
    {
        const int r = timed(c, QHUFF_KIND_SCAN, "launch_insscan_tabs",
                            [&](hipEvent_t e0, hipEvent_t e1) {
            return step == 1 ? launch_scan(top, 1, st, e0, e1)
                             : launch_insscan_tabs(a, step, st, e0, e1);
        });
        if (step || !r)
        {
            c->scan_stream = st;
            c->scan_have = true;
        }
        if (r)
            return r;
    }
    return QHUFF_OK;
}

// The decode launch on the scan's descriptors, then the accounting, the sums
// and the copy, each timed as QHUFF_KIND_SCAN.  Scratch layout: [dec_off | fin
// | rel | plan | sums | status | dec].
extern "C" int
qhuff_apply_inserts_tabs(qhuff_ctx *c, const struct qhuff_dyn_tables *tabs,
                         const struct qhuff_ins_state *s, const uint8_t *buf,
                         uint32_t wire_bytes, const uint32_t *keep,
                         const struct qhuff_ins_scan *sc, uint32_t n_ins,
                         const struct qhuff_ins_out *o, void *stream)
{
    if (!c || !tabs || !s || !sc || !o || !o->out_ent || !o->out_off
            || !sc->ins_off)
        return QHUFF_EINVAL;
    const uint32_t T = tabs->T;
    if (T && (!tabs->ent || !tabs->first || !tabs->off || !s->cap
              || !s->live_lo || !sc->rc || !sc->consumed || !sc->chunk_cap
              || !o->out_first || !o->cap_out || !o->live_lo_out
              || (o->out_cap && !o->out_bytes)))
        return QHUFF_EINVAL;
    if (n_ins > sc->max_ins
            || (n_ins && (!buf || !sc->strs || !sc->root || !sc->ins_cap
                          || !sc->ins_ref || !sc->ins_kind || !o->ins_lo)))
        return QHUFF_EINVAL;
    const uint64_t bound = ins::decode_bound(wire_bytes, n_ins,
                                             s->dyn_longest);
    if (n_ins > 0x7fffffffu || bound > 0xffffffffull)
        return QHUFF_ERANGE;
    hipStream_t st = (hipStream_t) stream;
    HIPCHK(c, hipSetDevice(c->device));
    if (T == 0)
    {
        HIPCHK(c, hipMemsetAsync(o->out_ent, 0, 4, st));
        HIPCHK(c, hipMemsetAsync(o->out_off, 0, 4, st));
        return QHUFF_OK;
    }
    if (const int r = scan_prepare(c, T, st))
        return r;
    const uint64_t n2 = 2ull * n_ins;
    const size_t o_fin = ins_up16(4 * (n2 + 1));
    const size_t o_rel = o_fin + ins_up16(4 * n2);
    const size_t o_plan = o_rel + ins_up16(4 * n2);
    const size_t o_sums = o_plan + 16ull * T;
    const size_t o_st = o_sums + 16ull * (T + 1ull);
    const size_t o_dec = o_st + ins_up16(n2);
    const size_t need = o_dec + ins_up16(bound);
    if (need > c->ins_ws_cap)
    {
        if (c->ins_ws)
        {
            // (earlier calls may still use it)
            if (c->scan_have)
                HIPCHK(c, hipStreamSynchronize(c->scan_stream));
            HIPCHK(c, hipFree(c->ins_ws));
            c->ins_ws = nullptr;
            c->ins_ws_cap = 0;
        }
        const size_t cap = need < (1u << 20) ? (1u << 20) : need;
        HIPCHK(c, hipMalloc((void **) &c->ins_ws, cap));
        c->ins_ws_cap = cap;
    }
    uint8_t *W = c->ins_ws;
    c->scan_stream = st;
    c->scan_have = true;
    if (n_ins)
    {
        const int r = qhuff_decode_headers_dyn(c, buf, sc->strs, n_ins, 0,
                                               tabs->bytes, s->arena_bytes,
                                               W + o_dec, (uint32_t *) W,
                                               W + o_st, st);
        if (r)
            return r;
    }
    ins::Args a;
    a.bytes = tabs->bytes;
    a.off = tabs->off;
    a.ent = tabs->ent;
    a.first = tabs->first;
    a.cap = s->cap;
    a.live_lo = s->live_lo;
    a.keep = keep;
    a.T = T;
    a.D = 0;                             // (the kernels read ent[T])
    a.arena = s->arena_bytes;
    a.rc = sc->rc;
    a.consumed = sc->consumed;
    a.ins_off = sc->ins_off;
    a.chunk_cap = sc->chunk_cap;
    a.strs = sc->strs;
    a.root = sc->root;
    a.ins_cap = sc->ins_cap;
    a.ins_ref = sc->ins_ref;
    a.ins_kind = sc->ins_kind;
    a.n_ins = n_ins;
    a.dec = W + o_dec;
    a.dec_off = (const uint32_t *) W;
    a.status = W + o_st;
    a.fin = (uint32_t *) (W + o_fin);
    a.rel = (uint32_t *) (W + o_rel);
    a.plan = (uint32_t *) (W + o_plan);
    a.sums = (uint64_t *) (W + o_sums);
    a.ins_lo = o->ins_lo;
    a.out_bytes = o->out_bytes;
    a.out_off = o->out_off;
    a.out_ent = o->out_ent;
    a.out_first = o->out_first;
    a.cap_out = o->cap_out;
    a.live_lo_out = o->live_lo_out;
    a.out_cap = o->out_cap;
    a.ent_cap = o->ent_cap;
    for (unsigned step = 0; step < 3; ++step)
    {
        const int r = timed(c, QHUFF_KIND_SCAN, "launch_insapply_tabs",
                            [&](hipEvent_t e0, hipEvent_t e1) {
            return launch_insapply_tabs(a, step, st, e0, e1);
        });
        if (r)
            return r;
    }
    return QHUFF_OK;
}

// ---- host helpers --------------------------------------------------------------

extern "C" uint64_t
qhuff_synth_batch(uint64_t seed, uint32_t n, uint32_t min_len,
                  uint32_t max_len, const uint8_t *alphabet,
                  uint32_t alphabet_len, uint8_t *data, uint32_t *in_off)
{
    uint64_t x = seed ? seed : 0x9E3779B97F4A7C15ull;
    uint64_t pos = 0;
    const uint32_t span = max_len - min_len + 1;
    for (uint32_t i = 0; i < n; ++i)
    {
        in_off[i] = (uint32_t) pos;
        x ^= x << 13; x ^= x >> 7; x ^= x << 17;
        uint32_t len = min_len + (uint32_t) (x % span);
        for (uint32_t k = 0; k < len; ++k)
        {
            x ^= x << 13; x ^= x >> 7; x ^= x << 17;
            data[pos++] = alphabet[x % alphabet_len];
        }
    }
    in_off[n] = (uint32_t) pos;
    return pos;
}
