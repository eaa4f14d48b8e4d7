// qhuff_ctx.h -- host-internal: the context, and what the host files of the
// C-ABI share (qhuff_host.cpp context and device-pointer calls, _hostpath
// pinned host-memory calls, _multi several contexts, _svc_host the service).
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

#include "qhuff_kernels.h"

using namespace qhuff;

struct CopyPool;                         // (qhuff_hostpath.cpp)

struct DevTables
{
    uint32_t win[kWinSize];              // 16-byte aligned (copied as uint4)
    uint2 enc[257];                      // {code, bits}
    uint16_t sorted[257];
    uint16_t long2[kLong2Size];
    uint32_t nodes[kNodes];              // (qhuff_decode_stream)
};

constexpr unsigned kMaxChunks = 16;          // host-path pipeline depth

struct qhuff_ctx
{
    int device;
    int n_cu;
    uint32_t enc_grid, dec_grid;         // workgroups per launch
    uint32_t hash_grid;                  // resident hash workgroups
    hipStream_t own_stream;
    DevTables *tab;                      // device
    LongParams lp;
    unsigned long long *flags;           // device look-back workspace:
                                         // tile flags [cap_tiles], super
                                         // flags [kLbReplicas][cap_super],
                                         // super accumulators [2][cap_super]
    uint32_t *err;                       // device: [0] error word, [1..3]
                                         // census, then claim counters
    uint64_t cap_tiles, cap_super;
    uint8_t *big_small;                  // device: big-tile output slots
                                         // (Coord::big) of launches of at
                                         // most kSmallGrid workgroups, lazily;
                                         // larger launches use the device's
                                         // pool (slot_pool)
    bool pool_ref;                       // holds a reference on that pool
    uint32_t max_banks;                  // pool banks it may open (1..4)
    uint32_t pool_bank;                  // 1 + the pool bank its last full
                                         // launch used (0: none yet)
    // kernel variant per kind (0 encode, 1 decode; pick_full): the full
    // kernel unless the batch is known (a hint) to need only the lean one
    bool last_full[2];                   // variant of the last launch
    int hint[2];                         // the next launch's variant from
                                         // its batch, known on the host
                                         // (host_hint), or -1: full
    int kernels;                         // QHUFF_KERNELS: 0 auto, 1 lean,
                                         // 2 full
    int lb_replica;                      // QHUFF_LB_REPLICA: the super-flag
                                         // replica every wave polls, or -1
    unsigned long long *prof;            // QHUFF_PROFILE builds: stamp buffer;
                                         // QH_PATH_TRACE builds: tile records
    size_t prof_words;                   // words of the last launch
    size_t prof_cap;                     // words allocated (path trace)
    uint32_t epoch;
    // host-path staging
    uint8_t *h_stage;                    // pinned
    size_t h_stage_cap;
    uint8_t *d_stage;
    size_t d_stage_cap;
    // host-path pipeline: copy streams, per-chunk events, copy workers
    hipStream_t h2d_stream, d2h_stream;
    hipEvent_t ev_in[kMaxChunks], ev_k[kMaxChunks], ev_out[kMaxChunks];
    bool pipe_ready;
    CopyPool *pool;
    // launch ordering: every look-back launch records ev_last on its stream;
    // a launch on another stream waits for it first (one workspace per
    // context, whichever streams the caller and the host path use)
    hipEvent_t ev_last;
    hipStream_t last_stream;
    bool have_last;
    // pinned, device-mapped mirror of the device error word: a kernel that
    // sets an error bit also writes it here, so a batch call reports an
    // error an earlier (completed) launch left without synchronising
    uint32_t *err_host;
    uint32_t *err_host_dev;
    // the low-latency service attached by qhuff_svc_open (small host-path
    // calls on this context go through it)
    qhuff_svc *svc;
    // decode launches keep a rejected string's bytes decoded before its error
    // (qhuff::decode_keep_rejected, for qhuff_shim.cpp)
    bool keep_rejected;
    // launch timing (qhuff_timing_enable): a start / stop event pair per
    // launch, a ring of the last QHUFF_TIMING_SLOTS launches
    hipEvent_t *tev;                     // [2 * QHUFF_TIMING_SLOTS], or null
    bool t_on;
    uint32_t t_every;                    // time every t_every-th launch of
    uint64_t t_seen[4];                  // each kind (launches seen)
    uint64_t t_next, t_first;            // launches timed / first unread
    uint8_t t_kind[QHUFF_TIMING_SLOTS];
    // qhuff_scan_sections' scratch (counts [cap chunks], then a total per
    // workgroup of the count launch), allocated at the first scan call; its
    // launches are ordered across streams as the look-back launches are
    uint32_t *scan_ws;
    uint64_t scan_cap;                   // chunks it holds
    hipEvent_t scan_ev;
    hipStream_t scan_stream;
    bool scan_have;
    // qhuff_encode_headers' scratch for hdr_cap items (2n + 2m of a call):
    // the items [8 * cap], their string offsets [cap + 1] and their output
    // offsets [cap + 1], each part 16-byte aligned; allocated at the first
    // call, ordered across streams as scan_ws is
    uint8_t *hdr_ws;
    uint64_t hdr_cap;                    // items it holds
    hipEvent_t hdr_ev;
    hipStream_t hdr_stream;
    bool hdr_have;
    // the dynamic lookup's scratch (qhuff_dyn_lookup,
    // qhuff_encode_headers_dyn): dyn_cap words -- a word a section, then the
    // table's two indices -- rebuilt on every call; ordered across streams
    // with hdr_ws, by hdr_ev
    uint32_t *dyn_ws;
    uint64_t dyn_cap;
    uint32_t dyn_grid[2];                // resident workgroups of its lookup
                                         // kernel ([1]: the encode form's),
                                         // found at the first call
    uint32_t tabs_grid[2];               // the same of the lookup over a set
                                         // of tables (qhuff_lookup_tabs.hip)
    // qhuff_apply_inserts_tabs' scratch (the decode launch's outputs, the
    // final lengths, the plans and the sums), grown on demand; ordered across
    // streams with scan_ws, by scan_ev
    uint8_t *ins_ws;
    uint64_t ins_ws_cap;                 // bytes it holds
    char err_msg[256];
};

// (the shards of a multi-context call: host_batch, qhuff_hostpath.cpp)
struct ShardSync
{
    std::mutex mu;
    std::condition_variable cv;
    std::vector<uint64_t> total;         // output bytes of each shard
    std::vector<char> known;
    bool failed = false;
    explicit ShardSync(unsigned g) : total(g, 0), known(g, 0) {}
    void publish(unsigned k, uint64_t t)
    {
        std::lock_guard<std::mutex> l(mu);
        total[k] = t;
        known[k] = 1;
        cv.notify_all();
    }
    void fail()
    {
        std::lock_guard<std::mutex> l(mu);
        failed = true;
        cv.notify_all();
    }
    // the output bytes of shards [0, k), or ~0 if one of them failed
    uint64_t base_of(unsigned k)
    {
        std::unique_lock<std::mutex> l(mu);
        uint64_t b = 0;
        for (unsigned j = 0; j < k; ++j)
        {
            cv.wait(l, [&] { return known[j] || failed; });
            if (failed)
                return ~0ull;
            b += total[j];
        }
        return b;
    }
};

#pragma GCC visibility push(hidden)
namespace qhuff {
// qhuff_host.cpp
extern thread_local char t_open_err[160];
int fail(qhuff_ctx *c, hipError_t e, const char *what);
int mirror_error(qhuff_ctx *c);
// (qhuff_dyn_lookup_tabs / qhuff_encode_headers_tabs after their checks, with
// D = ent[T] known to the caller; n and m not 0)
int tabs_lookup_dev(qhuff_ctx *c, const uint8_t *in, const uint32_t *off,
                    uint32_t n, const uint32_t *sec_hdr, uint32_t m,
                    const struct qhuff_dyn_tables *tabs, uint32_t D,
                    const uint32_t *sec_tab, const uint32_t *sec_win,
                    uint32_t *name_hash, uint32_t *nameval_hash,
                    uint8_t *kind, uint8_t *static_id, uint32_t *dyn_id,
                    hipStream_t st);
int tabs_encode_dev(qhuff_ctx *c, const uint8_t *in, const uint32_t *off,
                    uint32_t n, const uint8_t *hflags, const uint32_t *sec_hdr,
                    uint32_t m, const struct qhuff_dyn_tables *tabs,
                    uint32_t D, const uint32_t *sec_tab,
                    const uint32_t *sec_win, const uint32_t *sec_base,
                    uint8_t *out, uint32_t *sec_out, uint8_t *kind,
                    uint8_t *static_id, uint32_t *dyn_id, hipStream_t st);
// qhuff_hostpath.cpp
void pipe_teardown(qhuff_ctx *c);
bool host_registered(const void *p, uint64_t bytes);
int host_batch(qhuff_ctx *c, bool enc, const uint8_t *in,
               const uint32_t *in_off, uint32_t n, unsigned mode, uint8_t *out,
               uint32_t *out_off, uint8_t *status, ShardSync *sync = nullptr,
               unsigned shard = 0, bool last_shard = true,
               bool out_reg = false);
// qhuff_svc_host.cpp
int svc_call(qhuff_svc *v, bool enc, const uint8_t *in, const uint32_t *in_off,
             uint32_t n, unsigned mode, uint8_t *out, uint32_t *out_off,
             uint8_t *status);
}
#pragma GCC visibility pop

#define HIPCHK(c, call)                                                      \
    do {                                                                     \
        hipError_t e_ = (call);                                              \
        if (e_ != hipSuccess)                                                \
            return fail((c), e_, #call);                                     \
    } while (0)

// the encode modes: 0 payload, 3 / 5 / 7 literal prefix bits
static inline bool
mode_ok(unsigned mode)
{
    return mode == 0 || mode == 3 || mode == 5 || mode == 7;
}

static inline uint64_t
bound_of(bool enc, uint64_t bytes, uint32_t n, unsigned mode)
{
    return enc ? qhuff_encode_bound(bytes, n, mode) : qhuff_decode_bound(bytes, n);
}
