// qhuff_kernels.h -- argument blocks and launch entry points shared by the
// kernel translation units and the host C-ABI files (qhuff_ctx.h).
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>

#include "../../include/qhuff.h"
#include "qhuff_device.h"
#include "qhuff_tables.h"

namespace qhuff {

struct LongParams
{
    LongLen l[kMaxLong];
    uint32_t n;
};

struct EncArgs
{
    const uint8_t *in;
    const uint32_t *in_off;
    uint8_t *out;
    uint32_t *out_off;
    const uint2 *enc;            // 257 x {code, bits}
    uint64_t n;
    uint32_t mode;               // 0 payload, 3/5/7 literal prefix bits
    Coord c;
};

struct DecArgs
{
    const uint8_t *in;
    const uint32_t *in_off;
    uint8_t *out;
    uint32_t *out_off;
    uint8_t *status;
    const uint32_t *win;         // kWinSize window entries
    const uint16_t *sorted;      // 257 symbols in canonical order
    const uint16_t *long2;       // kLong2Size long codes by leading ones
    uint64_t n;
    Coord c;
    LongParams lp;
};

// resumable decode (qhuff_stream.hip): the decode arguments, the node table
// and the per-string state carried across calls
struct StreamArgs
{
    DecArgs d;
    const uint32_t *nodes;       // kNodes sorted node keys (qhuff_tables.h)
    ::qhuff_decode_status *state;    // n, read and written
    const uint8_t *flags;        // n, or null: no chunk is final
};

// literals decoded in place from wire data (qhuff_wire.hip): the decode
// arguments -- d.in the wire buffer, d.in_off the n 16-byte descriptors
// (struct qhuff_literal) reinterpreted -- and the length limit.  (The static
// table's name lengths, qhuff_names.h, are a constant of the kernel's code
// object, kWireNames in qhuff_wire_impl.h: no pointer to carry and nothing
// to upload.)
struct WireArgs
{
    DecArgs d;
    uint32_t max_len;            // 0: no limit
};

// field sections / encoder streams walked on the device (qhuff_scan.hip):
// m chunks of buf between sec_off[0 .. m]; cnt (m words) and tot (one word a
// workgroup of the count launch) are the context's scratch
constexpr uint32_t kScanBlock = 256;     // chunks (lanes) per workgroup
constexpr uint32_t kScanTop = 1024;      // totals per round of the top launch
static inline uint32_t
scan_blocks(uint32_t m)
{
    return (uint32_t) (((uint64_t) m + kScanBlock - 1) / kScanBlock);
}

struct ScanArgs
{
    const uint8_t *buf;
    const uint32_t *sec_off;
    ::qhuff_literal *lits;
    uint32_t *lit_off;
    int32_t *rc;
    uint32_t *consumed;          // or null
    uint32_t *cnt, *tot;
    uint32_t m, max_lits, mode;
};

// field sections walked for their header lines (qhuff_hdrscan.hip): the
// scan's sections and scratch; strs holds 2 * max_hdrs descriptors; kind,
// static_id and hflags may each be null
struct HdrScanArgs
{
    const uint8_t *buf;
    const uint32_t *sec_off;
    ::qhuff_hstr *strs;
    uint32_t *hdr_off;
    int32_t *rc;
    uint8_t *kind, *static_id, *hflags;
    uint32_t *cnt, *tot;
    uint32_t m, max_hdrs;
};

// the header scan against the dynamic table's entries
// (qhuff_hdrscan_dyn.hip): the table's offsets and each section's window;
// sec_win and dyn_id may be null
struct HdrScanDynArgs
{
    HdrScanArgs h;
    const uint32_t *off;         // 2d + 1, or null when d = 0
    const uint32_t *sec_win;     // 2m, or null
    uint32_t *dyn_id;            // max_hdrs, or null
    uint32_t d, first, max_entries;
};

// header lists decoded with a third string source (qhuff_hdrdec_dyn.hip):
// the table's bytes
struct HdrDynArgs
{
    WireArgs w;
    const uint8_t *dyn;          // dyn_len bytes, or null with 0
    uint32_t dyn_len;
};

struct HashArgs
{
    const uint8_t *in;
    const uint32_t *off;         // pairs: 2n + 1 offsets, else n + 1
    uint32_t *h1;                // name hash (pairs) / string hash
    uint32_t *h2;                // name+value hash (pairs only)
    uint64_t n;
    uint32_t seed;
    uint32_t pairs;
};

// headers looked up in the static table, and their field lines' items
// (qhuff_lookup.hip): the hash kernel's pairs layout.  Every output may be
// null.  Encode form (items != null): m sections between sec_hdr[0 .. m];
// items and str_off hold 2n + 2m items / 2n + 2m + 1 offsets (the context's
// scratch, items 16-byte and str_off 8-byte aligned).
struct LookupArgs
{
    const uint8_t *in;
    const uint32_t *off;         // 2n + 1 offsets
    uint32_t *h1, *h2;           // name hash, name+value hash
    uint8_t *kind, *id;          // QHUFF_LINE_*, static index
    const uint8_t *hflags;       // or null: all 0
    const uint32_t *sec_hdr;
    ::qhuff_item *items;
    uint32_t *str_off;
    uint64_t n;
    uint32_t m;
};

// headers looked up in the static table and among the dynamic table's
// entries (qhuff_lookup_dyn.hip): the lookup's arguments, the table, its two
// indices (mask + 1 slots each, the context's scratch, cleared on the stream
// before the index launch; null when d = 0) and the window.  Lookup form
// (l.items = null): every header sees [win_lo, win_hi).  Encode form:
// section s sees sec_win[2s .. 2s + 1] (null: [win_lo, win_hi)) with the Base
// sec_base[s] (null: its window's end); ric holds a word a section, cleared
// on the stream before the lookup launch.
struct DynLookupArgs
{
    LookupArgs l;
    const uint8_t *tab;          // the table's bytes, or null when d = 0
    const uint32_t *tab_off;     // 2d + 1, or null when d = 0
    uint32_t *nv, *nm;           // by name+value hash, by name hash
    const uint32_t *sec_win;     // 2m, or null
    const uint32_t *sec_base;    // m, or null
    uint32_t *dyn_id;            // n, or null
    uint32_t *ric;               // m: 1 + the largest index a section named
    uint32_t d, first, max_entries, mask;
    uint32_t win_lo, win_hi;
};

// the header scan over a set of tables, a table per section
// (qhuff_hdrscan_tabs.hip; struct qhuff_dyn_tables): the shared offsets, the
// tables' bounds and each section's table and window.  The kernels read D =
// ent[T] themselves.  T = 0: every pointer of the set may be null.
struct HdrScanTabsArgs
{
    HdrScanArgs h;
    const uint32_t *off;         // 2D + 1, or null when D = 0
    const uint32_t *ent;         // T + 1
    const uint32_t *first;       // T
    const uint32_t *max_entries; // T
    const uint32_t *sec_tab;     // m
    const uint32_t *sec_win;     // 2m, or null
    uint32_t *dyn_id;            // max_hdrs, or null
    uint32_t T;
};

// headers looked up in the static table and in their section's table of a
// set (qhuff_lookup_tabs.hip): DynLookupArgs with one pair of indices over
// all D entries (slots hold global ordinals + 1) and a table per section.
// Both forms go by sections (l.sec_hdr, l.m); lookup form: l.items = null,
// no sec_base, no ric.
struct TabsLookupArgs
{
    LookupArgs l;
    const uint8_t *tab;          // the shared bytes, or null when D = 0
    const uint32_t *tab_off;     // 2D + 1, or null when D = 0
    const uint32_t *ent;         // T + 1
    const uint32_t *first;       // T
    const uint32_t *max_entries; // T
    uint32_t *nv, *nm;           // by name+value hash, by name hash
    const uint32_t *sec_tab;     // m (null when T = 0)
    const uint32_t *sec_win;     // 2m, or null
    const uint32_t *sec_base;    // m, or null
    uint32_t *dyn_id;            // n, or null
    uint32_t *ric;               // m: 1 + the largest index a section named
    uint32_t T, D, mask;
};

// encoder-stream inserts of T connections walked on the device
// (qhuff_insscan_tabs.hip): chunk c of buf between sec_off[c .. c + 1] against
// table c of the set; the scan's scratch.  The kernels read D = ent[T].
struct InsScanArgs
{
    const uint8_t *buf;
    const uint32_t *sec_off;     // enc_off, T + 1
    const uint32_t *off, *ent, *first;
    const uint32_t *cap, *max_cap;
    int32_t *rc;
    uint32_t *consumed, *ins_off, *chunk_cap;
    ::qhuff_hstr *strs;          // 2 * max_ins
    uint32_t *root, *ins_cap;    // 2 * max_ins each
    uint32_t *ins_ref;           // max_ins
    uint8_t *ins_kind;           // max_ins
    uint32_t *cnt, *tot;
    uint32_t m, max_ins;         // m = T
};

// ---- low-latency service (qhuff_service.hip, qhuff_svc_host.cpp) ----------
//
// One request slot per service wave, in pinned host memory mapped into the
// device (fine-grained): the host writes a request and then its sequence
// number; the wave polls that word, codes the request and writes the result
// back into the slot, then the done word.  Slot layout (bytes):
//   header      kSvcHdrBytes   (SvcHdr)
//   in_off      (n + 1) u32, rebased to 0
//   in          the request's bytes
//   out_off     (n + 1) u32
//   status      n u8 (decode)
//   out         the output bytes
constexpr uint32_t kSvcMaxStrings = 1024;     // strings per request
constexpr uint32_t kSvcInCap = 65536;         // input bytes per request
constexpr uint32_t kSvcHdrBytes = 256;
constexpr uint32_t kSvcOffBytes = 4352;       // (kSvcMaxStrings + 1) u32, 256-aligned
constexpr uint32_t kSvcInOffAt = kSvcHdrBytes;
constexpr uint32_t kSvcInAt = kSvcInOffAt + kSvcOffBytes;
constexpr uint32_t kSvcOutOffAt = kSvcInAt + kSvcInCap + 256;
constexpr uint32_t kSvcStatusAt = kSvcOutOffAt + kSvcOffBytes;
constexpr uint32_t kSvcOutAt = kSvcStatusAt + kSvcMaxStrings + 256;
// the encode bound of a full request (qhuff_encode_bound: 30-bit codes, 7
// bytes of framing per literal, 16 slack), rounded up
constexpr uint32_t kSvcOutCap =
    ((kSvcInCap * 30 + 7) / 8 + 7 * kSvcMaxStrings + 16 + 4095) & ~4095u;
constexpr uint32_t kSvcSlotBytes = (kSvcOutAt + kSvcOutCap + 4095) & ~4095u;
// device scratch per slot (a request of more than one tile): the slot's
// layout; in_off and in are copied in, the tile loop reads them and writes
// out_off, status and out at device-memory latency, and those are copied
// back into the slot at the end
constexpr uint32_t kSvcScratchBytes = kSvcSlotBytes;
static_assert(kSvcInOffAt % 256 == 0 && kSvcInAt % 256 == 0
              && kSvcOutOffAt % 256 == 0 && kSvcStatusAt % 256 == 0
              && kSvcOutAt % 256 == 0, "slot regions 256-aligned");

// a piece coded straight from its slot: one staged tile (64 strings, the
// stage's bytes; qhuff_service.hip checks it against kStageCap)
constexpr uint32_t kSvcTileBytes = 3072;

constexpr uint32_t kSvcOpDecode = 0;
constexpr uint32_t kSvcOpEncode = 1;

struct SvcHdr
{
    // the request's first 16 bytes are read by one 16-byte load per poll:
    // the host writes n, in_bytes and opmode, then req (release), all in one
    // cache line, so a load that sees the new req sees the fields too
    uint32_t req;                // host: sequence of the posted request (last)
    uint32_t n;                  // strings
    uint32_t in_bytes;
    uint32_t opmode;             // kSvcOp* | encode mode << 8
    uint32_t pad0[28];           // (the device's words on their own line)
    uint32_t done;               // device: sequence of the last served request
    uint32_t total;              // device: its output bytes
    uint32_t pad1[30];
};
static_assert(sizeof(SvcHdr) <= kSvcHdrBytes, "slot header");

struct SvcArgs
{
    uint8_t *slots;              // device view of the pinned slots
    uint8_t *scratch;            // device memory, kSvcScratchBytes per slot
    const uint32_t *ctl;         // device view of the pinned control word
                                 // [0]: stop
    uint64_t *active;            // device: last time any wave served (100 MHz)
    const uint32_t *win;
    const uint16_t *sorted;
    const uint16_t *long2;
    const uint2 *enc;
    uint64_t idle_ticks;         // a wave leaves after this long with no
                                 // request served by any wave (100 MHz ticks)
    uint64_t life_ticks;         // and after this long in any case
};

template <class T>
__device__ __forceinline__ const QH_GLB T *
glb(const T *p)
{
    return (const QH_GLB T *) p;
}

template <class T>
__device__ __forceinline__ QH_GLB T *
glb(T *p)
{
    return (QH_GLB T *) p;
}

// One launch of `kernel` over `grid` workgroups of `block` threads (the
// kernel files' launch_* functions).  ev0 / ev1 non-null: the launch records
// its own start / stop time in them (the dispatch's timestamps, no extra
// queue packets).
template <class K, class A>
static inline hipError_t
launch_kernel(K kernel, uint32_t grid, uint32_t block, hipStream_t st,
              hipEvent_t ev0, hipEvent_t ev1, const A &args)
{
    if (ev0)
        hipExtLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, st, ev0,
                              ev1, 0, args);
    else
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, st, args);
    return hipGetLastError();
}

// full: the kernel variant with big-tile slots and cooperative long strings
// (qhuff_pipeline.h); the lean one is the default (qhuff_host.cpp)
hipError_t launch_encode(const EncArgs &a, uint32_t grid, hipStream_t st,
                         hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr,
                         bool full = false);
// keep: the kernel that keeps a rejected string's bytes decoded before its
// error (qhuff_shim.cpp)
hipError_t launch_decode(const DecArgs &a, uint32_t grid, hipStream_t st,
                         hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr,
                         bool keep = false, bool full = false);
hipError_t launch_stream(const StreamArgs &a, uint32_t grid, hipStream_t st,
                         hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);
int stream_waves_per_block();
hipError_t launch_wire(const WireArgs &a, uint32_t grid, hipStream_t st,
                       hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);
int wire_waves_per_block();
// launch `step` of a scan's three (0 count, 1 top, 2 write), m >= 1
hipError_t launch_scan(const ScanArgs &a, unsigned step, hipStream_t st,
                       hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);
// the count (step 0) and write (step 2) launches of a header scan, m >= 1;
// its sums are launch_scan's step 1 over the same tot
hipError_t launch_hdrscan(const HdrScanArgs &a, unsigned step, hipStream_t st,
                          hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);
// header lists decoded from their descriptors (qhuff_hdrdec.hip): the wire
// call's arguments, d.in_off the 2n descriptors (struct qhuff_hstr), d.n = 2n
hipError_t launch_hdrdec(const WireArgs &a, uint32_t grid, hipStream_t st,
                         hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);
int hdrdec_waves_per_block();
// the same two pairs with the dynamic table's entries
// (qhuff_hdrscan_dyn.hip, qhuff_hdrdec_dyn.hip)
hipError_t launch_hdrscan_dyn(const HdrScanDynArgs &a, unsigned step,
                              hipStream_t st, hipEvent_t ev0 = nullptr,
                              hipEvent_t ev1 = nullptr);
hipError_t launch_hdrdec_dyn(const HdrDynArgs &a, uint32_t grid,
                             hipStream_t st, hipEvent_t ev0 = nullptr,
                             hipEvent_t ev1 = nullptr);
int hdrdec_dyn_waves_per_block();
// items encoded in one launch (qhuff_encwire.hip): the encode arguments
// (mode unused: every item has its own framing) and the n items
hipError_t launch_encwire(const EncArgs &a, const ::qhuff_item *items,
                          uint32_t grid, hipStream_t st,
                          hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);
int encwire_waves_per_block();
hipError_t launch_hash(const HashArgs &a, uint32_t max_grid, hipStream_t st,
                       hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);
hipError_t hash_occupancy(int *blocks_per_cu);
// (a.n != 0)
hipError_t launch_lookup(const LookupArgs &a, uint32_t max_grid,
                         hipStream_t st, hipEvent_t ev0 = nullptr,
                         hipEvent_t ev1 = nullptr);
// the three launches of a lookup against the dynamic table
// (qhuff_lookup_dyn.hip): the index build (a.d != 0), the lookup (a.l.n != 0)
// and, in the encode form, the sections' prefix items (a.l.m != 0)
hipError_t launch_dyn_index(const DynLookupArgs &a, hipStream_t st,
                            hipEvent_t ev0 = nullptr,
                            hipEvent_t ev1 = nullptr);
hipError_t launch_lookup_dyn(const DynLookupArgs &a, uint32_t max_grid,
                             hipStream_t st, hipEvent_t ev0 = nullptr,
                             hipEvent_t ev1 = nullptr);
hipError_t launch_dyn_prefix(const DynLookupArgs &a, hipStream_t st,
                             hipEvent_t ev0 = nullptr,
                             hipEvent_t ev1 = nullptr);
// (enc: of the encode form's kernel, else of the lookup form's)
hipError_t lookup_dyn_occupancy(bool enc, int *blocks_per_cu);
// the same launches over a set of tables (qhuff_hdrscan_tabs.hip,
// qhuff_lookup_tabs.hip): the index build (a.D != 0), the lookup (a.l.n != 0,
// a.l.m != 0), the prefix items (encode form)
hipError_t launch_hdrscan_tabs(const HdrScanTabsArgs &a, unsigned step,
                               hipStream_t st, hipEvent_t ev0 = nullptr,
                               hipEvent_t ev1 = nullptr);
hipError_t launch_tabs_index(const TabsLookupArgs &a, hipStream_t st,
                             hipEvent_t ev0 = nullptr,
                             hipEvent_t ev1 = nullptr);
hipError_t launch_lookup_tabs(const TabsLookupArgs &a, uint32_t max_grid,
                              hipStream_t st, hipEvent_t ev0 = nullptr,
                              hipEvent_t ev1 = nullptr);
hipError_t launch_tabs_prefix(const TabsLookupArgs &a, hipStream_t st,
                              hipEvent_t ev0 = nullptr,
                              hipEvent_t ev1 = nullptr);
hipError_t lookup_tabs_occupancy(bool enc, int *blocks_per_cu);
// the inserts' scan (step 0 count, 2 write; its sums are launch_scan's step 1
// over the same tot), m >= 1, and their apply (qhuff_insapply_tabs.hip;
// ins::Args of qhuff_tabs_insert_impl.h, T >= 1): step 0 the accounting, 1
// the sums, 2 the copy
hipError_t launch_insscan_tabs(const InsScanArgs &a, unsigned step,
                               hipStream_t st, hipEvent_t ev0 = nullptr,
                               hipEvent_t ev1 = nullptr);
namespace ins { struct Args; }
hipError_t launch_insapply_tabs(const ins::Args &a, unsigned step,
                                hipStream_t st, hipEvent_t ev0 = nullptr,
                                hipEvent_t ev1 = nullptr);
// m sections of no headers: out = m x "00 00", sec_out[s] = 2s, s in [0, m]
hipError_t launch_empty_sections(uint32_t m, uint8_t *out, uint32_t *sec_out,
                                 hipStream_t st);
// sec_out[s] = item_off[2 * sec_hdr[s] + 2 * s], s in [0, m]
hipError_t launch_secout(const uint32_t *item_off, const uint32_t *sec_hdr,
                         uint32_t m, uint64_t n, uint32_t *sec_out,
                         hipStream_t st);
// off[0 .. n) += add (shard stitching, qhuff_*_batch_multi)
hipError_t launch_rebase(uint32_t *off, uint64_t n, uint32_t add,
                         hipStream_t st);
int hash_waves_per_block();
hipError_t encode_occupancy(int *blocks_per_cu);
hipError_t decode_occupancy(int *blocks_per_cu);
size_t encode_lds_bytes();
size_t decode_lds_bytes();
int encode_waves_per_block();
int decode_waves_per_block();
uint32_t decode_tile_strings();            // strings per decode tile
hipError_t launch_service(const SvcArgs &a, uint32_t grid, hipStream_t st);
bool ctx_has_service(const qhuff_ctx *c);   // (qhuff_svc_host.cpp)
int decode_keep_rejected(qhuff_ctx *c, const uint8_t *in,
                         const uint32_t *in_off, uint32_t n, uint8_t *out,
                         uint32_t *out_off, uint8_t *status);
int service_waves_per_block();
size_t service_lds_bytes();

}  // namespace qhuff
