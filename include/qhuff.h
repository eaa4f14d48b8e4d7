/*
 * qhuff.h -- C-ABI of the MI355X-native QPACK Huffman string-literal codec.
 *
 * Drop-in boundary for the string-literal step of ls-qpack (v2.6.5).  The
 * reference codes one string per synchronous call:
 *
 *   lsqpack_enc_enc_str()      lsqpack.c:839-876   (test/lsqpack-test.h:17-19)
 *   qenc_enc_str_size()        lsqpack.c:5198-5210 (static; ratio guard 1946)
 *   qenc_huffman_enc()         lsqpack.c:5085-5195 (static)
 *   lsqpack_huff_decode()      lsqpack.c:3520-3535 (LSQPACK_DEVEL_MODE export)
 *   lsqpack_huff_decode_full() lsqpack.c:3443-3517 (exported)
 *
 * This library codes a BATCH of independent strings per call on one GPU.
 * Every entry point is plain C: pointers, sizes, status codes.  No HIP or
 * torch types cross this header; `stream` is an opaque hipStream_t (NULL =
 * the device's default stream).
 *
 * Batch layout (device memory unless a function says host):
 *   in      strings packed back to back.
 *   in_off  n + 1 uint32 exclusive offsets: string i is
 *           in[in_off[i] .. in_off[i+1]).  in_off[0] need not be 0.
 *   out     packed outputs; out_off (n + 1 entries) is written by the call:
 *           output i is out[out_off[i] .. out_off[i+1]), out_off[0] = 0.
 *
 * Buffer contract (every batch call, device or host memory; enforced by
 * tests/test_buffer_contract.py).  The pointers need no alignment beyond
 * their types' (uint32 arrays 4 bytes, byte buffers none).
 *   Writes: out[0 .. out_off[n]), out_off[0 .. n], status[0 .. n) (decode)
 *           and n words of each hash output -- nothing else.  Bytes of `out`
 *           past out_off[n] are not written, on any path: the bound sizes
 *           the buffer, the call does not scribble in its slack.  For
 *           n = 0 only out_off[0] (= 0) is written.
 *   Reads:  in[in_off[0] .. in_off[n]) and in_off[0 .. n].  The kernels
 *           load the 16-byte-aligned blocks that contain those input bytes,
 *           so up to 15 bytes before in + in_off[0] and after in + in_off[n]
 *           are read as well; those bytes never affect a result.  Nothing
 *           the call reads is written.
 *
 * Results are bit-exact with the reference functions named on each call.
 * Failure is loud: a call returns a negative QHUFF_E* code, and the library
 * has no CPU fallback -- without a usable gfx950 device qhuff_open fails.
 */
#ifndef QHUFF_H
#define QHUFF_H 1

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI versions:
 *   1  batch encode / decode, host path, per-string mirrors.  (An early
 *      header of this version declared qhuff_huff_decode with 7 arguments,
 *      state and final included; the symbol takes 5 -- a caller built
 *      against that header links but its state / final are ignored: use
 *      qhuff_huff_decode_ex and check qhuff_abi_version() >= 2.)
 *   2  qhuff_huff_decode_ex (the reference's full argument list) beside the
 *      5-argument qhuff_huff_decode, which is unchanged
 *   3  the low-latency service (qhuff_svc_*) and, in qhuff_lsqpack.h,
 *      qhuff_lsqpack_set_context
 *   4  launch timing (qhuff_timing_enable / qhuff_timing_read)
 *   5  qhuff_kernel_variant (which kernel variant the last launch ran);
 *      qhuff_timing_enable(ctx, k > 1) samples every k-th launch
 *   6  QHUFF_MAX_STRLEN: qhuff_scan_field_section rejects (QHUFF_EPROTO) a
 *      literal whose declared length exceeds it; qhuff_decode_literals_ex
 *      rejects a literal whose decoded length does; qhuff_batch_hint /
 *      qhuff_batch_needs_full (the kernel variant from the batch)
 *   7  qhuff_dec_int (the pre-parse's integer decoder); qhuff_decode_
 *      literals_ex applies max_len to a field line's name + value;
 *      qhuff_encode_batch_host_multi / qhuff_decode_batch_host_multi and
 *      qhuff_*_batch_multi (one batch over several contexts / GPUs); an
 *      unhinted launch runs the full kernel (decode's launch history is
 *      gone); qhuff_host_register / qhuff_host_unregister (direct DMA for
 *      the host-memory calls) */
#define QHUFF_ABI_VERSION 7

/* QHUFF_ABI_VERSION of the loaded library (compare with the header's) */
int qhuff_abi_version(void);

/* return codes */
#define QHUFF_OK          0
#define QHUFF_EINVAL    (-22)   /* bad argument (NULL pointer, bad mode)   */
#define QHUFF_ENOMEM    (-12)   /* device allocation failed                */
#define QHUFF_ENODEV    (-19)   /* no usable device                        */
#define QHUFF_ERANGE    (-34)   /* batch too large for 32-bit offsets      */
#define QHUFF_EDEVICE   (-5)    /* a HIP call failed (see qhuff_last_error) */

/* encode modes (qhuff_encode_batch `mode`) */
#define QHUFF_ENC_PAYLOAD   0   /* qenc_huffman_enc output only (forced
                                   Huffman, no framing), lsqpack.c:5085   */
#define QHUFF_ENC_LITERAL3  3   /* lsqpack_enc_enc_str(3, ...) framing     */
#define QHUFF_ENC_LITERAL5  5   /* lsqpack_enc_enc_str(5, ...)             */
#define QHUFF_ENC_LITERAL7  7   /* lsqpack_enc_enc_str(7, ...)             */

/* per-string decode status (qhuff_decode_batch `status`) */
#define QHUFF_DEC_OK     0      /* HUFF_DEC_OK, lsqpack.c:3424             */
#define QHUFF_DEC_ERROR  1      /* HUFF_DEC_ERROR, lsqpack.c:3427: EOS in
                                   the data, padding > 7 bits, or padding
                                   that is not the EOS prefix              */

typedef struct qhuff_ctx qhuff_ctx;

/* Open a codec context on HIP device `device` (one context per host thread
 * per GPU).  Uploads the static Huffman tables once.  A context is not
 * thread-safe; its launches may use any streams (a launch on another stream
 * than the context's previous one is ordered after it).  Several contexts
 * may run on one GPU at once (tiles are claimed in order, so a grid need not
 * be co-resident).  Returns QHUFF_OK or QHUFF_E*. */
int qhuff_open(int device, qhuff_ctx **ctx_out);
void qhuff_close(qhuff_ctx *ctx);

/* Worst-case output bytes for an encode batch of n strings totalling
 * in_bytes: ceil(30 * in_bytes / 8) + n (30-bit longest code, each string
 * rounded up to a byte), + 6 * n in the LITERAL modes (the longest prefixed
 * length), + 16.  The 16 bytes are slack of the bound, not space the call
 * uses (see the buffer contract above). */
uint64_t qhuff_encode_bound(uint64_t in_bytes, uint32_t n, unsigned mode);

/* Worst-case output bytes for a decode batch (5-bit shortest code,
 * lsqpack.c:5072): floor(8 * in_bytes / 5) + 16 (slack, as above; n is not
 * used). */
uint64_t qhuff_decode_bound(uint64_t in_bytes, uint32_t n);

/* Encode n strings (device pointers).
 *   mode PAYLOAD: output i = qenc_huffman_enc(string i) (lsqpack.c:5085),
 *                 exactly qenc_enc_str_size(string i) bytes (lsqpack.c:5198).
 *   mode LITERAL3/5/7: output i = the bytes lsqpack_enc_enc_str(mode, dst,
 *                 bound, string i) writes with dst[0] = 0 beforehand
 *                 (lsqpack.c:839): H bit + prefixed length + Huffman, or
 *                 H=0 + length + raw copy when Huffman is not shorter.
 *                 Bits of byte 0 above the H bit are 0; the caller ORs its
 *                 instruction bits in (as the reference's callers do).
 * `out` must hold qhuff_encode_bound(...) bytes.  Asynchronous on `stream`. */
int qhuff_encode_batch(qhuff_ctx *ctx, const uint8_t *in,
                       const uint32_t *in_off, uint32_t n, unsigned mode,
                       uint8_t *out, uint32_t *out_off, void *stream);

/* Decode n complete Huffman strings (device pointers), with the semantics of
 * lsqpack_huff_decode(src, len, dst, dst_len, &{resume 0}, final = 1)
 * (lsqpack.c:3524-3529 -> huff_decode_fast, 5243) given a dst_len that
 * cannot run out.  status[i] = QHUFF_DEC_OK or QHUFF_DEC_ERROR; an ERROR
 * string contributes 0 output bytes.  `out` must hold
 * qhuff_decode_bound(...) bytes.  Asynchronous on `stream`. */
int qhuff_decode_batch(qhuff_ctx *ctx, const uint8_t *in,
                       const uint32_t *in_off, uint32_t n, uint8_t *out,
                       uint32_t *out_off, uint8_t *status, void *stream);

/* Host-memory variants (PCIe-inclusive path: host -> pinned staging ->
 * device -> kernel -> device -> pinned -> host).  Synchronous.  in_off and
 * the returned out_off are host arrays of n + 1 entries; out must hold the
 * corresponding bound; out_off[n] is the output total. */
int qhuff_encode_batch_host(qhuff_ctx *ctx, const uint8_t *in,
                            const uint32_t *in_off, uint32_t n, unsigned mode,
                            uint8_t *out, uint32_t *out_off);
int qhuff_decode_batch_host(qhuff_ctx *ctx, const uint8_t *in,
                            const uint32_t *in_off, uint32_t n, uint8_t *out,
                            uint32_t *out_off, uint8_t *status);

/* (ABI 7) Register caller buffers for direct DMA by the host-memory calls
 * (hipHostRegister, portable to every device; process-wide).  When a host
 * call's input bytes and offsets each lie within one registered range they
 * are transferred to the device directly, without the pinned staging copy;
 * when its output buffer (the bound), offsets and statuses do, the results
 * are transferred straight into them (batches past one 4 MB staging chunk).  Register long-lived buffers once (it pins
 * their pages: milliseconds for tens of MB); the results are the same either
 * way.  qhuff_host_register: QHUFF_OK, QHUFF_EINVAL (null, 0 bytes, or ptr
 * already registered), QHUFF_ENOMEM / QHUFF_EDEVICE (the reason in
 * qhuff_last_error(NULL)).  qhuff_host_unregister: ptr as registered; no call
 * may be using it. */
int qhuff_host_register(void *ptr, size_t bytes);
int qhuff_host_unregister(void *ptr);

/* Diagnostic, host-only: the string ranges qhuff_*_batch_host cuts this
 * batch into (in_off: n + 1 host offsets; enc 0: decode, else encode with
 * `mode`).  One chunk per 2^chunk_shift bytes of input, at most 16 and at
 * most one a string; chunk i is the strings [cut[i], cut[i + 1]), with
 * cut[i] = n * i / K.
 * chunk_shift 0: the process's own (QHUFF_HOST_CHUNK_SHIFT, default 23); a
 * value outside 16..30 counts as 23, as in the environment.
 * cut: K + 1 entries (room for 17).  *small (may be null): 1 when the call
 * takes the one-synchronisation path (one chunk whose output bound, rounded
 * up to 16, is at most 4 MB; registered outputs are then staged).  Returns K
 * (>= 1), QHUFF_EINVAL (a null pointer, a bad mode, in_off[n] < in_off[0])
 * or QHUFF_ERANGE (the chunks' bounds together pass 2^32 - 1).  A shard of a
 * *_host_multi call is cut the same way from its own offsets.  Host
 * arithmetic only: no context, no device call.  QHUFF_FEATURE_HOST_CHUNKS
 * and the symbol announce it (the ABI version is unchanged). */
#define QHUFF_FEATURE_HOST_CHUNKS 1
int qhuff_host_chunks(int enc, unsigned mode, const uint32_t *in_off,
                      uint32_t n, unsigned chunk_shift, uint32_t *cut,
                      uint32_t *small);

/* ---- low-latency service ----------------------------------------------
 * The reference codes one literal per call, a few dozen per header block
 * (lsqpack.c:3718, 3795, 4714, 4824, 4908 decode; 1983-2119 encode).  A
 * batch call pays a kernel launch, copies and a stream synchronisation; the
 * service instead keeps a kernel resident on the context's GPU (its own
 * stream; one workgroup = one CU per 12 request slots) that polls request
 * slots in pinned host memory: a call writes its strings into a free slot,
 * the kernel codes them and writes the result back into the slot.
 *
 * qhuff_svc_open: attach a service to ctx (one per context) with at least
 * `slots` request slots (0: 12; at most a quarter of the CUs' worth); its
 * kernel leaves after idle_us microseconds without a request (0: 20000) and
 * the next call starts it again.  Once attached, the context's host-path
 * calls (qhuff_*_batch_host and the per-string entry points below) that fit
 * a slot go through the service too.
 *
 * qhuff_svc_encode / qhuff_svc_decode: the arguments, outputs and return
 * codes of qhuff_encode_batch_host / qhuff_decode_batch_host; callable from
 * any number of threads at once (each call takes a free slot, waiting if
 * none is free).  A call of more than QHUFF_SVC_MAX_STRINGS strings or
 * QHUFF_SVC_MAX_BYTES input bytes runs the context's host path instead (one
 * such call at a time).  Offsets must not decrease (QHUFF_EINVAL).
 *
 * qhuff_svc_close: stop the kernel and free the service (no call may be in
 * flight); qhuff_close closes an attached service.  qhuff_svc_stats: calls
 * served by the kernel, kernel launches, calls sent to the host path. */
#define QHUFF_SVC_MAX_STRINGS 1024
#define QHUFF_SVC_MAX_BYTES   65536

typedef struct qhuff_svc qhuff_svc;

int qhuff_svc_open(qhuff_ctx *ctx, unsigned slots, unsigned idle_us,
                   qhuff_svc **svc_out);
void qhuff_svc_close(qhuff_svc *svc);
int qhuff_svc_encode(qhuff_svc *svc, const uint8_t *in, const uint32_t *in_off,
                     uint32_t n, unsigned mode, uint8_t *out,
                     uint32_t *out_off);
int qhuff_svc_decode(qhuff_svc *svc, const uint8_t *in, const uint32_t *in_off,
                     uint32_t n, uint8_t *out, uint32_t *out_off,
                     uint8_t *status);
int qhuff_svc_stats(qhuff_svc *svc, uint64_t *served, uint64_t *launches,
                    uint64_t *fallbacks);

/* Diagnostic: the pieces a service call of these n strings (in_off: n + 1
 * host offsets) is cut into, one request slot each: at most 64 strings and
 * 3072 input bytes a piece, a longer string alone.  Piece p is the strings
 * [cuts[p], cuts[p + 1]): cuts[0] = 0 ... cuts[*n_pieces] = n, in an array
 * of max_pieces + 1 entries.  QHUFF_OK; QHUFF_EINVAL for a null pointer or
 * decreasing offsets; QHUFF_ERANGE when the call needs more than max_pieces
 * pieces (*n_pieces is then the count needed, cuts holds the first
 * max_pieces).  A call that would run the context's host path (more than
 * QHUFF_SVC_MAX_STRINGS strings or QHUFF_SVC_MAX_BYTES bytes) reports
 * *n_pieces = 0 with QHUFF_OK.  Host arithmetic only: no context, no device
 * call.  QHUFF_FEATURE_SVC_PIECES and the symbol announce it (the ABI
 * version is unchanged). */
#define QHUFF_FEATURE_SVC_PIECES 1
int qhuff_svc_pieces(const uint32_t *in_off, uint32_t n, uint32_t *cuts,
                     uint32_t max_pieces, uint32_t *n_pieces);

/* ---- per-string mirrors of the reference entry points -----------------
 * Same argument meaning, return values and error behaviour as the reference
 * functions; each call runs a one-string batch on the context's GPU (no CPU
 * fallback).  Host pointers.  Synchronous. */

/* lsqpack_enc_enc_str (lsqpack.c:839): returns bytes written or -1 when
 * dst_len is too small.  Bits of dst[0] above prefix_bits+1 are kept. */
int qhuff_enc_enc_str(qhuff_ctx *ctx, unsigned prefix_bits,
                      unsigned char *dst, size_t dst_len,
                      const unsigned char *str, unsigned str_len);

/* qenc_enc_str_size (lsqpack.c:5198): Huffman size in bytes. */
unsigned qhuff_enc_str_size(qhuff_ctx *ctx, const unsigned char *str,
                            unsigned str_len);

/* struct huff_decode_retval (lsqpack.c:3420-3431) */
enum qhuff_huff_dec_status
{
    QHUFF_HUFF_DEC_OK,
    QHUFF_HUFF_DEC_END_SRC,
    QHUFF_HUFF_DEC_END_DST,
    QHUFF_HUFF_DEC_ERROR
};

struct qhuff_decode_retval
{
    enum qhuff_huff_dec_status  status;
    unsigned                    n_dst;
    unsigned                    n_src;
};

/* struct lsqpack_decode_status / lsqpack_huff_decode_state (lsqpack.h:
 * 747-757), same layout */
struct qhuff_decode_status
{
    uint8_t state;
    uint8_t eos;
};

struct qhuff_huff_decode_state
{
    int                         resume;
    struct qhuff_decode_status  status;
};

/* lsqpack_huff_decode(src, src_len, dst, dst_len, state, final)
 * (lsqpack.c:3524) on context ctx: complete strings (resume == 0 && final)
 * on the GPU -- OK, ERROR with n_dst = n_src = 0, or END_DST with the
 * reference's byte-boundary back-off (lsqpack.c:5438-5450) when dst_len is
 * too small; streaming input through the decoder registered with
 * qhuff_lsqpack_set_decode_full (qhuff_lsqpack.h, which documents the exact
 * semantics). */
struct qhuff_decode_retval
qhuff_huff_decode_ex(qhuff_ctx *ctx, const unsigned char *src, int src_len,
                     unsigned char *dst, int dst_len,
                     struct qhuff_huff_decode_state *state, int final);

/* (ABI 1) a complete string: qhuff_huff_decode_ex with a zeroed state and
 * final = 1 -- OK, ERROR with n_dst = n_src = 0, or END_DST with the
 * reference's partial progress when dst_len is too small */
struct qhuff_decode_retval
qhuff_huff_decode(qhuff_ctx *ctx, const unsigned char *src, int src_len,
                  unsigned char *dst, int dst_len);

/* ---- batched resumable decode: strings continued across chunks --------
 * The reference decodes a literal that straddles two stream reads with its
 * second, resumable decoder: every lsqpack_huff_decode call that is not
 * `resume == 0 && final` goes to lsqpack_huff_decode_full (lsqpack.c:
 * 3520-3535, 3443-3517; callers 3718, 3795, 4714, 4824, 4908).  A server
 * that batches literals over many connections holds many such partial
 * literals; qhuff_decode_stream decodes one chunk of each of n strings per
 * call.  QHUFF_FEATURE_STREAM and the symbols announce it (the ABI version
 * is unchanged).
 *
 * Chunk i is in[in_off[i] .. in_off[i+1]), the next bytes of string i, and
 * behaves like lsqpack_huff_decode_full(src, len, dst, dst_len, &st, final)
 * given a dst_len that cannot run out (qdec_huff_dec4bits, lsqpack.c:
 * 5213-5231):
 *   state[i]   carries string i from call to call.  Zeroed: a fresh string
 *              (the reference's resume == 0, lsqpack.c:3463-3464).  On input
 *              only .state is read: the id of the internal node of the code
 *              tree the string has reached -- 0 is the root, the other ids
 *              are THIS LIBRARY'S numbering (the tree's 256 internal nodes
 *              in the order of their bit prefixes; the reference's own
 *              numbering lives in its huff-tables.h) and opaque to the
 *              caller: a string begun by this call is continued by this call,
 *              not by the reference's decoder, and the other way round.  On
 *              output .eos = 1 iff that node accepts (the root, or an
 *              all-ones path of at most 7 bits).
 *   flags[i]   bit 0 (QHUFF_STREAM_FINAL): the chunk is the string's last.
 *              flags == NULL: no chunk is.
 *   out        every symbol whose last bit lies in the chunk, the one the
 *              incoming state was in the middle of included.
 *   status[i]  QHUFF_DEC_MORE  not final; state[i] updated.
 *              QHUFF_DEC_OK    final, and the end state accepts.
 *              QHUFF_DEC_ERROR the EOS code completed in this chunk (final
 *                              or not), or the chunk is final and the end
 *                              state does not accept.  The chunk contributes
 *                              0 output bytes; state[i] as written is
 *                              unspecified and must not be resumed.
 *   An empty chunk: not final -- MORE, state unchanged; final -- OK or ERROR
 *   by the incoming state.
 * `out` must hold qhuff_decode_stream_bound(in_bytes, n) bytes: a chunk of
 * len bytes emits at most floor(8 * len / 5) + 1 (the pending symbol may
 * need one bit only, and the other 8 * len - 1 bits hold at most
 * floor((8 * len - 1) / 5) codes), so floor(8 * in_bytes / 5) + n + 16
 * (slack, as qhuff_decode_bound's).
 *
 * The buffer contract above applies: the call writes out[0 .. out_off[n]),
 * out_off[0 .. n], status[0 .. n) and state[0 .. n), nothing else; for
 * n = 0 only out_off[0].  Read slack, 32-bit offsets (QHUFF_ERANGE, the
 * sticky device error word) and launch timing (QHUFF_KIND_DECODE) as
 * qhuff_decode_batch.  Asynchronous on `stream`; qhuff_decode_stream_host:
 * host pointers, synchronous.  Every chunk is decoded by one lane: there
 * is no cooperative walk for long chunks, and 64-chunk tiles over 3 KB take
 * the lean kernels' out-of-line path. */
#define QHUFF_FEATURE_STREAM 1
#define QHUFF_DEC_MORE     2    /* HUFF_DEC_END_SRC, lsqpack.c:3425        */
#define QHUFF_STREAM_FINAL 1    /* flags[i] bit 0                          */

uint64_t qhuff_decode_stream_bound(uint64_t in_bytes, uint32_t n);

int qhuff_decode_stream(qhuff_ctx *ctx, const uint8_t *in,
                        const uint32_t *in_off, uint32_t n,
                        struct qhuff_decode_status *state,
                        const uint8_t *flags, uint8_t *out, uint32_t *out_off,
                        uint8_t *status, void *stream);

int qhuff_decode_stream_host(qhuff_ctx *ctx, const uint8_t *in,
                             const uint32_t *in_off, uint32_t n,
                             struct qhuff_decode_status *state,
                             const uint8_t *flags, uint8_t *out,
                             uint32_t *out_off, uint8_t *status);

/* ---- literal-span pre-parse + batched literal decode (SURVEY.md 8(f)
 * rank 3).  A host pass walks only the instruction framing of QPACK wire
 * data -- field sections (RFC 9204 4.5; the reference's parse_header_prefix /
 * parse_header_data, lsqpack.c:3955-4046, 3567-3915) and encoder-stream
 * instructions (RFC 9204 4.3; lsqpack_dec_enc_in, lsqpack.c:4574-4960) --
 * with the reference's integer rules (lsqpack_dec_int / _int24,
 * lsqpack.c:2372-2460), and records every string literal.  Indices are not
 * resolved: the dynamic table stays with the reference.  The literals of
 * any number of blocks are then decoded in one GPU launch. */
#define QHUFF_EPROTO    (-71)   /* malformed instruction (bad integer)     */
#define QHUFF_ETRUNC    (-61)   /* input ends inside an instruction        */

#define QHUFF_LIT_NAME   1
#define QHUFF_LIT_VALUE  2

/* LSXPACK_MAX_STRLEN (lsxpack_header.h:12-13): the longest name or value a
 * field section may carry.  The reference rejects a field-section literal
 * whose declared length exceeds it right after the length integer
 * (lsqpack.c:3682-3685 values, 3769-3772 names) and a decoded one that
 * outgrows it (header_out_grow_buf, lsqpack.c:3350-3351). */
#define QHUFF_MAX_STRLEN 65535u

struct qhuff_literal
{
    uint32_t pos;               /* payload offset: pos_base + offset in buf */
    uint32_t len;               /* payload bytes                            */
    uint8_t  huffman;           /* H bit                                    */
    uint8_t  prefix_bits;       /* 3, 5 or 7: its length prefix             */
    uint8_t  kind;              /* QHUFF_LIT_NAME / QHUFF_LIT_VALUE         */
    uint8_t  hdr_len;           /* bytes of H bit + prefixed length: the
                                   literal's wire bytes are
                                   [pos - hdr_len, pos + len)                */
    uint32_t instr;             /* pos_base + offset of its instruction     */
};

/* One complete encoded field section (prefix + field lines).  Writes up to
 * max_lits literals in wire order and the count to *n_lits.  QHUFF_OK,
 * QHUFF_ETRUNC (ends inside a line), QHUFF_EPROTO (an integer the reference
 * rejects, or (ABI 6) a literal length above QHUFF_MAX_STRLEN, reported as
 * soon as the length is decoded, whether or not its bytes follow),
 * QHUFF_ERANGE (*n_lits is the count needed). */
int qhuff_scan_field_section(const uint8_t *buf, size_t len, uint32_t pos_base,
                             struct qhuff_literal *lits, uint32_t max_lits,
                             uint32_t *n_lits);

/* Encoder-stream bytes (may end inside an instruction: *consumed is the
 * length of the complete instructions, whose literals are reported; the
 * caller keeps the rest for the next chunk, as the reference resumes). */
int qhuff_scan_encoder_stream(const uint8_t *buf, size_t len,
                              uint32_t pos_base, struct qhuff_literal *lits,
                              uint32_t max_lits, uint32_t *n_lits,
                              size_t *consumed);

/* (ABI 7) The scanners' prefixed-integer decoder (RFC 7541 5.1) with the
 * reference's rules: lsqpack_dec_int (lsqpack.c:2372-2437) given the whole
 * integer in one buffer.  prefix_bits 1..8; the bits of buf[0] above the
 * prefix are ignored.  QHUFF_OK with *value and *consumed (the integer's
 * bytes), QHUFF_ETRUNC when buf ends inside the integer (the reference's -1),
 * QHUFF_EPROTO when the value does not fit 64 bits or the integer runs past
 * 10 continuation bytes (its -2). */
int qhuff_dec_int(const uint8_t *buf, size_t len, unsigned prefix_bits,
                  uint64_t *value, size_t *consumed);

/* Output bytes qhuff_decode_literals_host may write for these literals:
 * floor(8 * len / 5) per Huffman literal, len per raw one, + 16 (slack). */
uint64_t qhuff_literals_bound(const struct qhuff_literal *lits, uint32_t n);

/* Decode n literals whose payloads lie in host buffer `buf` (lits[i].pos is
 * relative to buf): Huffman ones (H = 1) on the GPU in one batch, with the
 * lsqpack_huff_decode semantics of qhuff_decode_batch; raw ones copied.
 * Host out_off[n + 1], status[n] (QHUFF_DEC_OK / QHUFF_DEC_ERROR, an ERROR
 * literal contributes 0 bytes).  `out` holds qhuff_literals_bound bytes.
 * Synchronous. */
int qhuff_decode_literals_host(qhuff_ctx *ctx, const uint8_t *buf,
                               const struct qhuff_literal *lits, uint32_t n,
                               uint8_t *out, uint32_t *out_off,
                               uint8_t *status);

/* (ABI 6) qhuff_decode_literals_host with a length limit: a literal whose
 * decoded (Huffman) or raw length exceeds max_len gets QHUFF_DEC_ERROR and
 * 0 bytes.  Field-section literals take max_len = QHUFF_MAX_STRLEN (the
 * reference's header_out_grow_buf rule, lsqpack.c:3350-3351: a string
 * never outgrows LSXPACK_MAX_STRLEN); 0 = no limit (encoder-stream literals,
 * whose bound is the dynamic table's capacity, lsqpack.c:4661-4667). */
int qhuff_decode_literals_ex(qhuff_ctx *ctx, const uint8_t *buf,
                             const struct qhuff_literal *lits, uint32_t n,
                             uint32_t max_len, uint8_t *out, uint32_t *out_off,
                             uint8_t *status);

/* ---- literals decoded in place from wire data ----------------------------
 * qhuff_decode_literals_ex gathers every Huffman payload on the host, decodes
 * the packed batch and interleaves the results with the raw literals on the
 * host again; it has no device-pointer form.  qhuff_decode_wire takes the
 * scanners' descriptors as they are: one descriptor a lane, the payloads read
 * where they lie in the wire buffer, one launch.  The output of
 * qhuff_encode_batch(..., QHUFF_ENC_LITERAL7, ...) is such a buffer too.
 * QHUFF_FEATURE_WIRE and the symbols announce it (the ABI version is
 * unchanged).
 *
 * For descriptors that satisfy the order rule, out, out_off[0 .. n] and
 * status[0 .. n) are byte for byte those of qhuff_decode_literals_ex(ctx, buf,
 * lits, n, max_len, ...): a Huffman literal decodes as in qhuff_decode_batch,
 * a raw one is copied; with max_len != 0 a literal longer than max_len once
 * decoded (or copied) gets QHUFF_DEC_ERROR and 0 bytes, a VALUE literal's
 * length counted together with the decoded length of the NAME literal
 * directly before it (same instr, status OK) or else with the static-table
 * name its instruction refers to (01NT, T = 1); max_len = 0: no limit.
 * `out` must hold qhuff_literals_bound(lits, n) bytes.
 *
 * Order rule -- THE CALLER'S DUTY for qhuff_decode_wire, whose descriptors
 * are in device memory where the call cannot check them: the descriptors are
 * in wire order and disjoint, pos[i] + len[i] <= pos[i + 1] (and within 32
 * bits), with hdr_len <= pos and instr <= pos - hdr_len.  Both scanners emit
 * descriptors of this form.  qhuff_literals_check (host only) tests it:
 * QHUFF_OK, or QHUFF_EINVAL with *bad (may be NULL) = the first offending
 * index -- of a pair out of order or overlapping, the second literal.
 * qhuff_decode_wire_host runs the check itself (QHUFF_EINVAL).
 *
 * The buffer contract above applies.  Writes: out[0 .. out_off[n]),
 * out_off[0 .. n], status[0 .. n), nothing else; for n = 0 only out_off[0].
 * Reads: lits[0 .. n) and the 16-byte-aligned blocks that contain the wire
 * bytes from lits[0].pos to lits[n-1].pos + lits[n-1].len, the bytes between
 * the literals included; with max_len != 0 also the instruction bytes
 * [instr, pos - hdr_len) of VALUE literals.  32-bit output offsets (the
 * sticky QHUFF_DEVERR_RANGE) and launch timing (QHUFF_KIND_DECODE) as
 * qhuff_decode_batch.  qhuff_decode_wire: device pointers (buf, lits, out,
 * out_off, status), asynchronous on `stream`.  qhuff_decode_wire_host: host
 * pointers, synchronous; QHUFF_ERANGE when the bound or the wire span passes
 * 32 bits.  Every literal is decoded by one lane: there is no cooperative
 * walk for long literals, and a 64-literal tile whose wire span passes 3 KB
 * -- a long literal, or short ones far apart -- takes the lean kernels'
 * out-of-line path; no speed is promised for those. */
#define QHUFF_FEATURE_WIRE 1

int qhuff_literals_check(const struct qhuff_literal *lits, uint32_t n,
                         uint32_t *bad);

int qhuff_decode_wire(qhuff_ctx *ctx, const uint8_t *buf,
                      const struct qhuff_literal *lits, uint32_t n,
                      uint32_t max_len, uint8_t *out, uint32_t *out_off,
                      uint8_t *status, void *stream);

int qhuff_decode_wire_host(qhuff_ctx *ctx, const uint8_t *buf,
                           const struct qhuff_literal *lits, uint32_t n,
                           uint32_t max_len, uint8_t *out, uint32_t *out_off,
                           uint8_t *status);

/* ---- field sections and encoder streams scanned on the device -------------
 * qhuff_scan_field_section and qhuff_scan_encoder_stream walk one chunk a
 * call on the host, and their descriptors go up beside the wire bytes (16
 * bytes a literal).  qhuff_scan_sections walks m chunks of one wire buffer
 * where it lies in device memory and leaves the descriptors there, in the
 * form and order qhuff_decode_wire reads.  QHUFF_FEATURE_SCAN_DEVICE and the
 * symbols announce it (the ABI version is unchanged).
 *
 * Input: buf, the wire bytes; sec_off[0 .. m], non-decreasing: chunk i is
 * buf[sec_off[i] .. sec_off[i + 1]); mode --
 *   QHUFF_SCAN_FIELD_SECTION   each chunk one complete field section, by the
 *                              rules (and their order) of
 *                              qhuff_scan_field_section;
 *   QHUFF_SCAN_ENCODER_STREAM  each chunk encoder-stream bytes of one
 *                              connection, by those of
 *                              qhuff_scan_encoder_stream: a partial last
 *                              instruction is left unconsumed, no length
 *                              limit.
 * Output:
 *   rc[m]          QHUFF_OK, QHUFF_ETRUNC or QHUFF_EPROTO: what the host
 *                  scanner returns for that chunk alone;
 *   consumed[m]    (may be NULL in field-section mode) encoder stream: the
 *                  bytes of the complete instructions, 0 with QHUFF_EPROTO;
 *                  field section: the chunk's length when OK, else 0;
 *   lit_off[m + 1] lit_off[0] = 0; chunk i's descriptors are lits[lit_off[i]
 *                  .. lit_off[i + 1]); a chunk that is not OK has none;
 *                  lit_off[m] is the full count whatever max_lits is (as the
 *                  host scanners' *n_lits under QHUFF_ERANGE);
 *   lits           the descriptors, packed, in wire order; only those with an
 *                  index below max_lits are written.  pos and instr are
 *                  offsets into buf (the host scanners' pos_base =
 *                  sec_off[i]); all 16 bytes are what the host scanner
 *                  writes.  They satisfy qhuff_decode_wire's order rule.
 *
 * The buffer contract above applies.  Reads: sec_off[0 .. m] and the
 * 16-byte-aligned blocks that contain buf[sec_off[0] .. sec_off[m]); bytes
 * outside a chunk, the next chunk's and the read slack among them, never
 * affect that chunk's result.  Writes: the outputs named above and nothing
 * else; for m = 0 only lit_off[0].  Three launches on `stream` (count, sum,
 * write), none of which waits for another workgroup; timed as
 * QHUFF_KIND_SCAN, one entry a launch.  Scratch, 4 bytes a chunk and 4 a
 * group of 256 chunks, belongs to the context: allocated at the first scan
 * call, grown on demand.  One chunk is walked by one lane: a very long chunk
 * is walked no faster than a short one.
 *
 * qhuff_scan_sections: device pointers, asynchronous on `stream`;
 * QHUFF_EINVAL for a null pointer (consumed too in encoder-stream mode) or a
 * bad mode.  The caller reads lit_off[m] and compares it with max_lits.
 * qhuff_scan_sections_host: host pointers, synchronous, one staged round
 * trip; QHUFF_EINVAL also for decreasing offsets; QHUFF_ERANGE when lit_off[m]
 * > max_lits -- lit_off, rc and consumed are valid and the first max_lits
 * descriptors are returned.
 * qhuff_decode_sections_host: the whole decode path -- the wire bytes and
 * offsets go up once, the scan runs, the small results come back (n =
 * lit_off[m]), qhuff_decode_wire(max_len) runs on the descriptors where they
 * are, and descriptors, offsets, statuses and exactly out_off[n] bytes come
 * back.  `out` holds qhuff_decode_bound(wire bytes, 0), out_off n + 1 and
 * status n entries (max_lits + 1 and max_lits are enough).  The results are
 * those of the host scanner per chunk followed by qhuff_decode_wire_host on
 * the concatenated descriptors.  QHUFF_ERANGE when n > max_lits: nothing is
 * decoded and out, out_off and status are not written; lit_off, rc and
 * consumed are valid and the first max_lits descriptors are returned, as
 * by qhuff_scan_sections_host.  The context's staging buffers (pinned host
 * and device) grow to the call's size, about the wire bytes + 21 bytes per
 * descriptor of max_lits + the bound of `out`, and stay with the context:
 * pass a max_lits near the count, not a loose bound.
 * qhuff_scan_sections_cpu: the same walker source as the kernels', run on
 * the host over host pointers: no context and no device call.  A diagnostic
 * (as qhuff_host_chunks); returns as qhuff_scan_sections_host. */
#define QHUFF_FEATURE_SCAN_DEVICE 1
#define QHUFF_SCAN_FIELD_SECTION  0
#define QHUFF_SCAN_ENCODER_STREAM 1

int qhuff_scan_sections(qhuff_ctx *ctx, const uint8_t *buf,
                        const uint32_t *sec_off, uint32_t m, unsigned mode,
                        struct qhuff_literal *lits, uint32_t max_lits,
                        uint32_t *lit_off, int32_t *rc, uint32_t *consumed,
                        void *stream);

int qhuff_scan_sections_host(qhuff_ctx *ctx, const uint8_t *buf,
                             const uint32_t *sec_off, uint32_t m,
                             unsigned mode, struct qhuff_literal *lits,
                             uint32_t max_lits, uint32_t *lit_off, int32_t *rc,
                             uint32_t *consumed);

int qhuff_decode_sections_host(qhuff_ctx *ctx, const uint8_t *buf,
                               const uint32_t *sec_off, uint32_t m,
                               unsigned mode, uint32_t max_len,
                               struct qhuff_literal *lits, uint32_t max_lits,
                               uint32_t *lit_off, int32_t *rc,
                               uint32_t *consumed, uint8_t *out,
                               uint32_t *out_off, uint8_t *status);

int qhuff_scan_sections_cpu(const uint8_t *buf, const uint32_t *sec_off,
                            uint32_t m, unsigned mode,
                            struct qhuff_literal *lits, uint32_t max_lits,
                            uint32_t *lit_off, int32_t *rc,
                            uint32_t *consumed);

/* ---- field lines and instructions encoded in one launch ------------------
 * qhuff_encode_batch frames every literal of a launch with one prefix width
 * and leaves the instruction bits and the prefixed integers between the
 * literals -- static, dynamic and post-base indices, the field-section
 * prefix -- to the host.  qhuff_encode_wire takes one descriptor per item and
 * writes the wire bytes themselves: every instruction the reference's encoder
 * writes (lsqpack_enc_encode, lsqpack.c:1963-2124) is an optional prefixed
 * integer whose first byte carries the instruction bits, followed by an
 * optional string literal, or a name literal whose first byte carries them,
 * followed by a value literal; the field-section prefix (lsqpack.c:1277,
 * 1296) is two integers.  qhuff_scan_field_section + qhuff_decode_wire read
 * the output straight back.  QHUFF_FEATURE_ENCODE_WIRE and the symbols
 * announce it (the ABI version is unchanged).
 *
 * Output of item i: out[out_off[i] .. out_off[i + 1]), two parts in this
 * order --
 *   1. int_bits != 0: ival as lsqpack_enc_int (lsqpack.c:787-814) writes it
 *      with an int_bits-bit prefix into a first byte preset to int_first;
 *   2. str_bits != 0: the bytes lsqpack_enc_enc_str(str_bits, ...) writes for
 *      string i (in[in_off[i] .. in_off[i + 1])) with dst[0] = str_first
 *      beforehand: the strict-< choice between Huffman and raw of
 *      QHUFF_ENC_LITERAL3/5/7.
 * With str_bits == 0 string i's bytes are ignored, whatever their length; an
 * item with neither part emits nothing.  The outputs are concatenated in item
 * order: a field section is a run of items, its length the difference of
 * out_off at its ends.
 *
 * Item rule -- THE CALLER'S DUTY for qhuff_encode_wire, whose items are in
 * device memory where the call cannot check them: int_bits <= 8 and
 * int_first & ((1 << int_bits) - 1) == 0; str_bits one of 0, 3, 5, 7 and
 * str_first & ((2 << str_bits) - 1) == 0; an unused part's *_first is 0.
 * qhuff_items_check (host only) tests it: QHUFF_OK, or QHUFF_EINVAL with *bad
 * (may be NULL) = the first offending index.  qhuff_encode_wire_host runs the
 * check itself (QHUFF_EINVAL, nothing written).  The kernel masks what it
 * reads: for items outside the rule their own bytes are unspecified, their
 * size is at most 12 + the literal's payload, and all other items are
 * unaffected -- the bound and the buffer contract hold for any descriptor
 * bytes whatever.
 *
 * `out` must hold qhuff_encode_wire_bound(in_bytes, n) = ceil(30 * in_bytes /
 * 8) + 13 * n + 16 bytes: per item 1 for byte rounding, 6 for the longest
 * prefixed length and 6 for the longest 32-bit integer (a 1-bit prefix); the
 * 16 are slack of the bound.
 *
 * The buffer contract above applies.  Writes: out[0 .. out_off[n]) and
 * out_off[0 .. n], nothing else; for n = 0 only out_off[0].  Reads:
 * items[0 .. n) (4-byte alignment is enough), in_off[0 .. n] and the
 * 16-byte-aligned blocks that contain in[in_off[0] .. in_off[n]).  32-bit
 * output offsets (the sticky QHUFF_DEVERR_RANGE) as qhuff_encode_batch;
 * launches are timed as QHUFF_KIND_ENCODE.  The call does not consume
 * qhuff_batch_hint and does not change what qhuff_kernel_variant reports.
 * qhuff_encode_wire: device pointers (in, in_off, items, out, out_off),
 * asynchronous on `stream`.  qhuff_encode_wire_host: host pointers,
 * synchronous -- one upload, one launch, then the offsets and exactly
 * out_off[n] bytes come back, with no loop over the items on the host but
 * the check; QHUFF_ERANGE when the bound passes 32 bits.  Every item is coded by one lane, and a 64-item tile
 * whose input span passes 3 KB, whose output passes 3008 bytes or whose
 * Huffman codes together pass 24,576 bits leaves the byte-parallel path (the
 * first two for the lean kernels' out-of-line path); no speed is promised
 * for those. */
#define QHUFF_FEATURE_ENCODE_WIRE 1

struct qhuff_item {          /* 8 bytes, 4-byte aligned */
    uint32_t ival;           /* the integer's value (int_bits != 0)            */
    uint8_t  int_bits;       /* 0: no integer; 1..8: its prefix width          */
    uint8_t  int_first;      /* OR-ed into the integer's first byte            */
    uint8_t  str_bits;       /* 0: no literal; 3, 5 or 7: its length prefix    */
    uint8_t  str_first;      /* OR-ed into the literal's first byte            */
};

uint64_t qhuff_encode_wire_bound(uint64_t in_bytes, uint32_t n);

int qhuff_items_check(const struct qhuff_item *items, uint32_t n,
                      uint32_t *bad);

int qhuff_encode_wire(qhuff_ctx *ctx, const uint8_t *in,
                      const uint32_t *in_off, const struct qhuff_item *items,
                      uint32_t n, uint8_t *out, uint32_t *out_off,
                      void *stream);

int qhuff_encode_wire_host(qhuff_ctx *ctx, const uint8_t *in,
                           const uint32_t *in_off,
                           const struct qhuff_item *items, uint32_t n,
                           uint8_t *out, uint32_t *out_off);

/* ---- header lists encoded to field sections against the static table ------
 * qhuff_encode_wire writes field lines once somebody has decided, per header,
 * which form the line takes.  That decision is the first thing
 * lsqpack_enc_encode does for every header (lsqpack.c:1671-1715, 1835-1866,
 * 1904-1930): hash the name, hash the value seeded with the name's hash, probe
 * nameval2id_plus_one / name2id_plus_one (lsqpack.c:629-666, 721-764), compare
 * the bytes.  Whenever the dynamic table is not used -- LQEF_NO_DYN, an
 * encoder of capacity 0, a LSXPACK_NEVER_INDEX header that is not in the
 * dynamic table -- it is per header and stateless, and the line is one of
 *   QHUFF_LINE_INDEXED  EHA_INDEXED_STAT (lsqpack.c:2033-2039): name and value
 *                       are a static entry; 0xC0 | id on a 6-bit prefix
 *   QHUFF_LINE_NAMEREF  EHA_LIT_WITH_NAME_STAT (2110-2125): only the name is;
 *                       0x50 | N << 5, id on a 4-bit prefix, then
 *                       lsqpack_enc_enc_str(7, value)
 *   QHUFF_LINE_LITERAL  EHA_LIT (2061-2076): neither; 0x20 | N << 4 +
 *                       lsqpack_enc_enc_str(3, name), then
 *                       lsqpack_enc_enc_str(7, value)
 * (N: the header is never to be indexed), behind the field-section prefix
 * 00 00 (lsqpack.c:1277, 1296).  QHUFF_FEATURE_ENCODE_HEADERS and the symbols
 * announce it (the ABI version is unchanged).
 *
 * Headers are laid out as for qhuff_xxh32_headers: off[2n + 1], header i is
 * name in[off[2i] .. off[2i+1]) and value in[off[2i+1] .. off[2i+2]).
 *
 * qhuff_static_lookup -- per header the two hashes (those of
 * qhuff_xxh32_headers with seed QHUFF_XXH_SEED; name_hash / nameval_hash may
 * each be NULL), kind[i] = QHUFF_LINE_* and static_id[i] = the static index the
 * reference finds (find_in_static_full, else lsqpack_find_in_static_headers;
 * of several entries with one name the lowest), QHUFF_STATIC_NONE for
 * LITERAL.  One launch, timed as QHUFF_KIND_HASH.  Device pointers,
 * asynchronous on `stream`.  A stateful caller copies the results into its
 * lsxpack_header (name_hash, nameval_hash, qpack_index and the flags
 * LSXPACK_NAME_HASH | LSXPACK_NAMEVAL_HASH | LSXPACK_QPACK_IDX (|
 * LSXPACK_VAL_MATCHED)) and lsqpack_enc_encode skips its own hashing and,
 * by the line, its static probes (lsqpack.c:1672-1694, 1836-1840): both for
 * an INDEXED header, lsqpack_find_in_static_headers but not
 * find_in_static_full for a NAMEREF one, none for a LITERAL one
 * (INTEGRATION.md).
 * qhuff_static_lookup_host: host pointers, synchronous, one staged round trip.
 * qhuff_static_lookup_cpu: the kernel's lookup source run on the host over
 * host pointers: no context and no device call (a diagnostic, as
 * qhuff_scan_sections_cpu).  QHUFF_EINVAL for a null pointer, QHUFF_ERANGE
 * for n above 2^31 - 1.
 * qhuff_static_probe_tables (diagnostic, host only): the library's two probe
 * tables, 512 bytes each, id + 1 or 0, as it builds them from the static
 * table with its own XXH32.
 *
 * qhuff_encode_headers -- m field sections; section s holds the headers
 * [sec_hdr[s], sec_hdr[s+1]), sec_hdr[0] = 0, sec_hdr[m] = n, non-decreasing.
 * hflags[i] bit 0 (QHUFF_HDR_NEVER_INDEX) is the N bit of header i; hflags
 * may be NULL (all 0).  Output: the sections back to back, each its two
 * prefix bytes and its lines -- the bytes lsqpack_enc_start_header /
 * lsqpack_enc_encode(..., flags | LQEF_NO_DYN) / lsqpack_enc_end_header write
 * for it; an empty section is its two prefix bytes -- section s in
 * out[sec_out[s] .. sec_out[s+1]), sec_out[0] = 0; kind[n] and static_id[n] as
 * qhuff_static_lookup's, each may be NULL.  LSXPACK_QPACK_IDX on input is out
 * of scope.  `out` must hold qhuff_encode_headers_bound(in_bytes, n, m) =
 * qhuff_encode_wire_bound(in_bytes, 2n + 2m) bytes.
 *
 * Launches on `stream`: the lookup (QHUFF_KIND_HASH), which also writes
 * 2n + 2m items and their string offsets into scratch of the context -- two
 * per section prefix, two per header -- then qhuff_encode_wire's launch
 * unchanged on those arrays (QHUFF_KIND_ENCODE), then a gather of sec_out from
 * the items' offsets.  The names of INDEXED and NAMEREF lines still pass
 * through the encode kernel's stage although no literal is made of them; that
 * is accepted.  Scratch, 16 bytes an item, belongs to the context: allocated at
 * the first call, grown on demand, ordered across streams as the scan's.
 *
 * The buffer contract above applies.  Writes: out[0 .. sec_out[m]),
 * sec_out[0 .. m], kind and static_id (n bytes each), nothing else; for
 * n = m = 0 only sec_out[0].  Reads: off[0 .. 2n], sec_hdr[0 .. m], hflags and
 * the 16-byte-aligned blocks that contain in[off[0] .. off[2n]).
 * qhuff_encode_headers: device pointers, asynchronous; sec_hdr is in device
 * memory where the call cannot check it: its form is THE CALLER'S DUTY.
 * QHUFF_EINVAL for a null pointer.  qhuff_encode_headers_host: host pointers,
 * synchronous -- one upload, the launches, then sec_out, the optional byte
 * arrays and exactly sec_out[m] bytes come back; no loop over the headers on
 * the host but the offsets' check.  QHUFF_EINVAL for a null pointer, decreasing
 * off or sec_hdr, sec_hdr[0] != 0 or sec_hdr[m] != n; QHUFF_ERANGE when
 * 2n + 2m or the bound passes 32 bits. */
#define QHUFF_FEATURE_ENCODE_HEADERS 1
#define QHUFF_HDR_NEVER_INDEX 1     /* hflags[i] bit 0: LQEF_NEVER_INDEX /
                                       LSXPACK_NEVER_INDEX                  */
#define QHUFF_LINE_INDEXED 0        /* EHA_INDEXED_STAT                     */
#define QHUFF_LINE_NAMEREF 1        /* EHA_LIT_WITH_NAME_STAT               */
#define QHUFF_LINE_LITERAL 2        /* EHA_LIT                              */
#define QHUFF_STATIC_NONE  0xFF

int qhuff_static_lookup(qhuff_ctx *ctx, const uint8_t *in, const uint32_t *off,
                        uint32_t n, uint32_t *name_hash,
                        uint32_t *nameval_hash, uint8_t *kind,
                        uint8_t *static_id, void *stream);

int qhuff_static_lookup_host(qhuff_ctx *ctx, const uint8_t *in,
                             const uint32_t *off, uint32_t n,
                             uint32_t *name_hash, uint32_t *nameval_hash,
                             uint8_t *kind, uint8_t *static_id);

int qhuff_static_lookup_cpu(const uint8_t *in, const uint32_t *off, uint32_t n,
                            uint32_t *name_hash, uint32_t *nameval_hash,
                            uint8_t *kind, uint8_t *static_id);

int qhuff_static_probe_tables(uint8_t name2id_plus_one[512],
                              uint8_t nameval2id_plus_one[512]);

uint64_t qhuff_encode_headers_bound(uint64_t in_bytes, uint32_t n, uint32_t m);

int qhuff_encode_headers(qhuff_ctx *ctx, const uint8_t *in,
                         const uint32_t *off, uint32_t n,
                         const uint8_t *hflags, const uint32_t *sec_hdr,
                         uint32_t m, uint8_t *out, uint32_t *sec_out,
                         uint8_t *kind, uint8_t *static_id, void *stream);

int qhuff_encode_headers_host(qhuff_ctx *ctx, const uint8_t *in,
                              const uint32_t *off, uint32_t n,
                              const uint8_t *hflags, const uint32_t *sec_hdr,
                              uint32_t m, uint8_t *out, uint32_t *sec_out,
                              uint8_t *kind, uint8_t *static_id);

/* ---- field sections decoded to header lists against the static table ------
 * qhuff_scan_sections and qhuff_decode_wire give a section's literals and
 * nothing else: an indexed line has none, a name-reference line only its
 * value, and which static entry a line named, or its N bit, is not reported.
 * These calls are the inverse of qhuff_encode_headers: for a field section
 * that does not use the dynamic table the reference's decoder is stateless
 * per line (header_out_static_entry, lsqpack.c:3013-3057;
 * header_out_begin_static_nameref, 3121-3159; header_out_begin_literal /
 * _write_name / _write_value, 3211-3323; the dispatch of parse_header_data,
 * 3567-3915), and the result is a header list in the layout
 * qhuff_encode_headers and qhuff_xxh32_headers take: off[2n + 1], name then
 * value, packed.  QHUFF_FEATURE_DECODE_HEADERS and the symbols announce it
 * (the ABI version is unchanged).
 *
 * Descriptors: one struct qhuff_hstr per string, two per header -- strings 2i
 * and 2i + 1 are the name and the value of header i.  A WIRE string is a
 * literal as in struct qhuff_literal; a STATIC string is the name or the
 * value of static entry static_id and occupies no wire bytes.  The
 * descriptors follow qhuff_decode_wire's order rule: pos does not decrease
 * and pos[i] + len[i] <= pos[i + 1].
 *
 * qhuff_scan_headers walks m field sections (buf, sec_off as
 * qhuff_scan_sections) and gives
 *   rc[m]           per section, decided in this order:
 *                   1. what qhuff_scan_field_section returns for the section
 *                      alone when that is not OK (QHUFF_ETRUNC / QHUFF_EPROTO,
 *                      QHUFF_MAX_STRLEN included);
 *                   2. QHUFF_ENOTSUP: the Required Insert Count is not 0, or a
 *                      line is a dynamic form -- indexed with T = 0, name
 *                      reference with T = 0, indexed post-base, post-base name
 *                      reference: the section needs the dynamic table; give
 *                      it to the reference's decoder;
 *                   3. QHUFF_EPROTO: a static index >= 99 (lsqpack.c:3021,
 *                      3130);
 *                   4. QHUFF_OK.
 *                   With a Required Insert Count of 0 the Delta Base and its
 *                   sign are read and ignored (lsqpack.c:4024-4028).  A
 *                   section of just its two prefix bytes is OK, no headers.
 *   hdr_off[m + 1]  hdr_off[0] = 0; section s holds the headers
 *                   [hdr_off[s], hdr_off[s + 1]); a section that is not OK
 *                   has none; hdr_off[m] is the full count whatever max_hdrs
 *                   is;
 *   and, for the headers with an index below max_hdrs,
 *   strs            their two descriptors (strs holds 2 * max_hdrs);
 *   kind[n]         QHUFF_LINE_INDEXED / _NAMEREF / _LITERAL;
 *   static_id[n]    the entry the line named, QHUFF_STATIC_NONE for LITERAL;
 *   hflags[n]       bit 0 (QHUFF_HDR_NEVER_INDEX) = the line's N bit, 0 for
 *                   indexed lines
 *   -- the arrays of the same names in qhuff_encode_headers; each of the three
 *   may be NULL.
 * qhuff_scan_headers: device pointers, asynchronous on `stream`, three
 * launches none of which waits for another workgroup, timed as
 * QHUFF_KIND_SCAN, on the scan's scratch; QHUFF_EINVAL for a null pointer;
 * the caller reads hdr_off[m].  qhuff_scan_headers_host: host pointers, one
 * staged round trip; QHUFF_EINVAL also for decreasing offsets; QHUFF_ERANGE
 * when hdr_off[m] > max_hdrs, hdr_off and rc valid and the first max_hdrs
 * headers returned.  qhuff_scan_headers_cpu: the kernels' walker source on the
 * host over host pointers, no context and no device call; returns as the
 * host form.  Reads and writes as qhuff_scan_sections: the outputs named
 * above and nothing else, for m = 0 only hdr_off[0].
 *
 * qhuff_decode_headers: n headers = 2n descriptors (device pointers,
 * asynchronous, one launch timed as QHUFF_KIND_DECODE).  Writes
 * out[0 .. off[2n]), off[0 .. 2n] and status[0 .. 2n), nothing else; for
 * n = 0 only off[0].  A WIRE string decodes exactly as in qhuff_decode_wire
 * (Huffman as qhuff_decode_batch, raw copied); a STATIC string is the entry's
 * name or value from RFC 9204 Appendix A.  A rejected string has
 * QHUFF_DEC_ERROR and 0 bytes; its header's other string keeps its bytes: a
 * header is good iff both statuses are 0.  max_len != 0: a string longer
 * than max_len is rejected, and a value whose length plus its name's -- the
 * name is string 2i, whatever its source, when its status is OK -- passes
 * max_len (header_out_grow_buf, lsqpack.c:3346-3351, as the wire call).
 * `out` must hold qhuff_decode_headers_bound(wire_bytes, n) = 8 * wire_bytes
 * / 5 + 76 * n + 16 bytes (76: the longest static name + value).  The form
 * of the descriptors is THE CALLER'S DUTY, as for qhuff_decode_wire; the
 * kernel masks what it reads -- static_id clamped into the table, source and
 * kind to a bit, a STATIC string's len taken as 0 -- so descriptors outside
 * the rule give unspecified bytes, at most 53 for a STATIC string, for their
 * own string only and no access outside the blocks of the wire span.
 * QHUFF_EINVAL for a null pointer, QHUFF_ERANGE for n above 2^31 - 1.  One
 * string a lane, 32 headers a tile; a tile whose wire span passes 3 KB or
 * whose output, static bytes included, passes 3008 bytes takes the lean
 * kernels' out-of-line path.
 *
 * qhuff_decode_headers_host: the whole path, as qhuff_decode_sections_host is
 * for literals -- the wire bytes go up once, the scan runs, the small results
 * come back (n = hdr_off[m]), the decode launch runs on the descriptors where
 * they are, and off[0 .. 2n], status[0 .. 2n), the optional byte arrays and
 * exactly off[2n] bytes come back; name_hash / nameval_hash (each may be
 * NULL): qhuff_xxh32_headers with QHUFF_XXH_SEED runs over (out, off) on the
 * device, by definition what qhuff_xxh32_headers gives on the returned
 * arrays (LSQPACK_DEC_OPT_HASH_NAME / _NAMEVAL).  `out` holds
 * qhuff_decode_headers_bound(wire bytes, max_hdrs), off 2 * max_hdrs + 1,
 * status 2 * max_hdrs, the per-header arrays max_hdrs entries.  QHUFF_ERANGE
 * when n > max_hdrs: nothing is decoded, out / off / status and the hashes
 * are not written, hdr_off and rc are valid.  No loop over headers or
 * strings on the host. */
#define QHUFF_FEATURE_DECODE_HEADERS 1
#define QHUFF_ENOTSUP   (-95)   /* the section needs the dynamic table     */
#define QHUFF_HSTR_WIRE   0
#define QHUFF_HSTR_STATIC 1

struct qhuff_hstr {          /* 16 bytes, 4-byte aligned */
    uint32_t pos;        /* WIRE: payload offset in buf.  STATIC: offset of
                            its line's first byte                           */
    uint32_t len;        /* WIRE: payload bytes.          STATIC: 0         */
    uint8_t  huffman;    /* WIRE: H bit.                  STATIC: 0         */
    uint8_t  source;     /* QHUFF_HSTR_WIRE / QHUFF_HSTR_STATIC             */
    uint8_t  kind;       /* QHUFF_LIT_NAME / QHUFF_LIT_VALUE                */
    uint8_t  static_id;  /* STATIC: the entry whose name or value this is;
                            WIRE: QHUFF_STATIC_NONE                         */
    uint32_t instr;      /* offset of its line's first byte                 */
};

int qhuff_scan_headers(qhuff_ctx *ctx, const uint8_t *buf,
                       const uint32_t *sec_off, uint32_t m,
                       struct qhuff_hstr *strs, uint32_t max_hdrs,
                       uint32_t *hdr_off, int32_t *rc, uint8_t *kind,
                       uint8_t *static_id, uint8_t *hflags, void *stream);

int qhuff_scan_headers_host(qhuff_ctx *ctx, const uint8_t *buf,
                            const uint32_t *sec_off, uint32_t m,
                            struct qhuff_hstr *strs, uint32_t max_hdrs,
                            uint32_t *hdr_off, int32_t *rc, uint8_t *kind,
                            uint8_t *static_id, uint8_t *hflags);

int qhuff_scan_headers_cpu(const uint8_t *buf, const uint32_t *sec_off,
                           uint32_t m, struct qhuff_hstr *strs,
                           uint32_t max_hdrs, uint32_t *hdr_off, int32_t *rc,
                           uint8_t *kind, uint8_t *static_id,
                           uint8_t *hflags);

uint64_t qhuff_decode_headers_bound(uint64_t wire_bytes, uint32_t n);

int qhuff_decode_headers(qhuff_ctx *ctx, const uint8_t *buf,
                         const struct qhuff_hstr *strs, uint32_t n,
                         uint32_t max_len, uint8_t *out, uint32_t *off,
                         uint8_t *status, void *stream);

int qhuff_decode_headers_host(qhuff_ctx *ctx, const uint8_t *buf,
                              const uint32_t *sec_off, uint32_t m,
                              uint32_t max_len, uint32_t max_hdrs,
                              uint32_t *hdr_off, int32_t *rc, uint8_t *kind,
                              uint8_t *static_id, uint8_t *hflags,
                              uint8_t *out, uint32_t *off, uint8_t *status,
                              uint32_t *name_hash, uint32_t *nameval_hash);

/* ---- header lists from field sections that use the dynamic table -----------
 * The calls above, for sections that name dynamic entries, the table's
 * entries given by the caller as plain arrays.  Decoding a section against
 * the dynamic table is a read of that table: the reference's decoder resolves
 * each dynamic line to an entry (qdec_get_table_entry_abs, lsqpack.c:
 * 2768-2775) and copies name and value out (header_out_dynamic_entry,
 * 3060-3117; header_out_begin_dynamic_nameref, from 3655-3662); inserts come
 * only from the encoder stream (4544 ff.), which these calls leave to the
 * caller (qhuff_tabs_insert_host below applies it to a set of tables).  With
 * the entries at hand a dynamic line is per line and stateless, as a static
 * one is.  QHUFF_FEATURE_DECODE_HEADERS_DYN and the symbols announce it (the
 * ABI version is unchanged); the calls above behave as before.
 *
 * struct qhuff_dyn_table is a read-only view: the entries held decoded (plain
 * bytes), oldest first, packed as a header list -- bytes, off[2d + 1] as
 * qhuff_xxh32_headers' off -- entry k with the absolute index (0-based insert
 * ordinal) first + k.  d = 0 with null pointers is legal.  max_entries is
 * MaxEntries = max table capacity / 32 (lsqpack.c:2789).
 *
 * qhuff_scan_headers_dyn / _host / _cpu: the arguments of the
 * qhuff_scan_headers family and
 *   tab       the table;
 *   sec_win   2m entries, or NULL: sec_win[2s] = the oldest absolute index
 *             still live when section s is decoded, sec_win[2s + 1] = the
 *             insert count it sees; the rule: first <= sec_win[2s] <=
 *             sec_win[2s + 1] <= first + d.  NULL: every section sees
 *             [first, first + d).  One batch may so hold sections decoded at
 *             different moments against one history of entries;
 *   dyn_id    n entries, or NULL: the absolute index a line named, or
 *             QHUFF_DYN_NONE.
 * rc[s] is decided in this order (ins = the section's insert count):
 *   1. what qhuff_scan_field_section returns for the section alone when that
 *      is not OK;
 *   2. QHUFF_EPROTO: the encoded Required Insert Count is above 2 *
 *      max_entries (lsqpack.c:3973) -- any non-zero one when max_entries = 0;
 *   3. the Required Insert Count (RFC 9204 4.5.1.1; the reference's modular
 *      ids, ID_MINUS, qdec_in_future, 2749-2753, 3914-3923): 0 when encoded
 *      as 0, else the one value RIC == enc - 1 (mod 2 * max_entries) in
 *      [ins - max_entries + 1, ins + max_entries]; RIC <= 0: QHUFF_EPROTO;
 *      RIC > ins: QHUFF_EBLOCKED (3980-3981: the section waits for inserts;
 *      submit it again after more of them);
 *   4. Base = RIC + DeltaBase, or RIC - DeltaBase - 1 when the sign bit is set
 *      (4015-4022), in 64-bit two's complement; a line names Base - 1 - idx
 *      (indexed and name reference, T = 0) or Base + idx (the post-base
 *      forms).  QHUFF_EPROTO when that index is outside the section's window
 *      (the entry is not there: 3070-3072, 3656-3658), when RIC = 0 and the
 *      section has a dynamic line (3895), when RIC != 0 and no line names
 *      RIC - 1 (3891-3894), or when a static index is >= 99.  A line's index
 *      is not compared with RIC (the reference does not either);
 *   5. QHUFF_OK.
 * Never QHUFF_ENOTSUP.  The result equals the reference's whenever its
 * modular ids are unambiguous, i.e. for references within MaxEntries of the
 * insert count; where the reference's ids alias, the rule above (absolute
 * indices) is the definition.
 *
 * A DYN descriptor: pos = the offset of its line's first byte (as STATIC; it
 * occupies no wire bytes for the order rule), len = the string's bytes in the
 * table, instr = its byte offset in tab->bytes, source = QHUFF_HSTR_DYN,
 * static_id = QHUFF_STATIC_NONE.  kind[] of a line that names a dynamic entry
 * has QHUFF_LINE_DYN OR-ed in (INDEXED|DYN = 4, NAMEREF|DYN = 5), its
 * static_id[] is QHUFF_STATIC_NONE; an indexed dynamic line has N = 0, a
 * dynamic name reference its line's N bit.
 * Device form: device pointers, asynchronous, three launches on the scan's
 * scratch timed as QHUFF_KIND_SCAN; tab is a host struct of device pointers
 * (tab->bytes is not read).  The form of sec_win and off is THE CALLER'S
 * DUTY: the walker clamps a window into [first, first + d] and takes a
 * decreasing pair of offsets as an empty string, so nothing outside the
 * arrays is read.  Host and _cpu forms: QHUFF_EINVAL also for a decreasing
 * off, off[2d] < off[0] or a window outside the rule, QHUFF_ERANGE when
 * first + d passes 2^32 - 1.
 *
 * qhuff_decode_headers_dyn: qhuff_decode_headers and the table's bytes
 * (dyn_bytes, dyn_len of them; NULL with 0).  WIRE and STATIC strings as
 * there; a DYN string is len bytes from dyn_bytes + instr; the max_len rule
 * is unchanged (the name is string 2i whatever its source).  The kernel masks
 * what it reads: source to two bits (3 behaves as WIRE), instr clamped to
 * dyn_len, len to dyn_len - instr; it reads inside the 16-byte blocks that
 * hold dyn_bytes[0 .. dyn_len) only.  `out` must hold
 * qhuff_decode_headers_dyn_bound(wire_bytes, n, dyn_longest) = 8 * wire_bytes
 * / 5 + max(76, dyn_longest) * n + 16 bytes, dyn_longest the table's longest
 * name + value.  A tile is fast iff its output, dynamic bytes included, is at
 * most 3008 bytes.
 *
 * qhuff_decode_headers_dyn_host: the whole path in one call, as
 * qhuff_decode_headers_host: the wire bytes and the table go up once, the
 * scan runs, the small results come back, the decode launch runs on the
 * descriptors where they are; `out` holds qhuff_decode_headers_dyn_bound(wire
 * bytes, max_hdrs, the table's longest entry).  The host's only loop is over
 * the table's d entries. */
#define QHUFF_FEATURE_DECODE_HEADERS_DYN 1
#define QHUFF_EBLOCKED  (-11)  /* Required Insert Count above the inserts the
                                  section may see                           */
#define QHUFF_HSTR_DYN  2      /* qhuff_hstr.source: a dynamic entry's name
                                  or value                                  */
#define QHUFF_LINE_DYN  4      /* OR-ed into kind[]: the line names a dynamic
                                  entry                                     */
#define QHUFF_DYN_NONE  0xFFFFFFFFu

struct qhuff_dyn_table {
    const uint8_t  *bytes;     /* entries packed: name then value           */
    const uint32_t *off;       /* off[2d + 1]                               */
    uint32_t d;                /* entries held                              */
    uint32_t first;            /* absolute index of entry 0                 */
    uint32_t max_entries;      /* MaxEntries                                */
};

int qhuff_scan_headers_dyn(qhuff_ctx *ctx, const uint8_t *buf,
                           const uint32_t *sec_off, uint32_t m,
                           const struct qhuff_dyn_table *tab,
                           const uint32_t *sec_win,
                           struct qhuff_hstr *strs, uint32_t max_hdrs,
                           uint32_t *hdr_off, int32_t *rc, uint8_t *kind,
                           uint8_t *static_id, uint8_t *hflags,
                           uint32_t *dyn_id, void *stream);

int qhuff_scan_headers_dyn_host(qhuff_ctx *ctx, const uint8_t *buf,
                                const uint32_t *sec_off, uint32_t m,
                                const struct qhuff_dyn_table *tab,
                                const uint32_t *sec_win,
                                struct qhuff_hstr *strs, uint32_t max_hdrs,
                                uint32_t *hdr_off, int32_t *rc, uint8_t *kind,
                                uint8_t *static_id, uint8_t *hflags,
                                uint32_t *dyn_id);

int qhuff_scan_headers_dyn_cpu(const uint8_t *buf, const uint32_t *sec_off,
                               uint32_t m, const struct qhuff_dyn_table *tab,
                               const uint32_t *sec_win,
                               struct qhuff_hstr *strs, uint32_t max_hdrs,
                               uint32_t *hdr_off, int32_t *rc, uint8_t *kind,
                               uint8_t *static_id, uint8_t *hflags,
                               uint32_t *dyn_id);

uint64_t qhuff_decode_headers_dyn_bound(uint64_t wire_bytes, uint32_t n,
                                        uint32_t dyn_longest);

int qhuff_decode_headers_dyn(qhuff_ctx *ctx, const uint8_t *buf,
                             const struct qhuff_hstr *strs, uint32_t n,
                             uint32_t max_len, const uint8_t *dyn_bytes,
                             uint32_t dyn_len, uint8_t *out, uint32_t *off,
                             uint8_t *status, void *stream);

int qhuff_decode_headers_dyn_host(qhuff_ctx *ctx, const uint8_t *buf,
                                  const uint32_t *sec_off, uint32_t m,
                                  const struct qhuff_dyn_table *tab,
                                  const uint32_t *sec_win, uint32_t max_len,
                                  uint32_t max_hdrs, uint32_t *hdr_off,
                                  int32_t *rc, uint8_t *kind,
                                  uint8_t *static_id, uint8_t *hflags,
                                  uint32_t *dyn_id, uint8_t *out,
                                  uint32_t *off, uint8_t *status,
                                  uint32_t *name_hash,
                                  uint32_t *nameval_hash);

/* ---- header lists encoded to field sections against the dynamic table ------
 * qhuff_encode_headers writes what lsqpack_enc_encode(..., LQEF_NO_DYN)
 * writes.  These calls write what it writes with the table in use and
 * LQEF_NO_INDEX: nothing is inserted, the header is looked up in the static
 * table and among the dynamic entries, and a line is written
 * (lsqpack.c:1671-1930 with index = 0).  Encoding against a given table is a
 * read of that table, as decoding is: with the entries at hand the decision
 * is per header and stateless; only a section's prefix depends on all of its
 * lines.  Inserting, the encoder stream, the history, risked-stream
 * accounting and duplication stay with the host.
 * QHUFF_FEATURE_ENCODE_HEADERS_DYN and the symbols announce it (the ABI
 * version is unchanged); the calls above behave as before.
 *
 * Inputs: those of qhuff_encode_headers, and
 *   tab       the table, as in the _dyn decode calls (in the device form a
 *             host struct of device pointers; here tab->bytes is read);
 *             d = 0 with null pointers is legal;
 *   sec_win   2m entries, or NULL: section s may name the entries with an
 *             absolute index in [sec_win[2s], sec_win[2s + 1]).  The low
 *             edge is the caller's "not draining" bound
 *             (qenc_entry_is_draining, lsqpack.c:1528), the high edge the
 *             insert count it may reference: qpe_max_acked_id when it may
 *             not risk, else the insert count (1790-1791, 1879-1881).  The
 *             rule: first <= lo <= hi <= first + d and, when max_entries is
 *             not 0, hi - lo <= max_entries (else the encoded Required
 *             Insert Count is ambiguous).  NULL: every section sees [first,
 *             first + d);
 *   sec_base  m entries, or NULL: the section's Base, the reference's
 *             qpe_cur_header.base_idx -- the insert count at
 *             lsqpack_enc_start_header (lsqpack.c:1106).  Any value <= first
 *             + d (below `first`: every entry is named post-base).  NULL:
 *             sec_win[2s + 1].  An entry with abs >= Base is named by the
 *             post-base forms, as the reference's EHA_INDEXED_NEW /
 *             EHA_LIT_WITH_NAME_NEW name an entry inserted during the
 *             section (2040-2050, 2077-2092).
 * Per header the line is chosen in the reference's order:
 *   1. name and value are a static entry (find_in_static_full, 1687-1715):
 *      QHUFF_LINE_INDEXED, as qhuff_encode_headers;
 *   2. name and value, bytes compared, are an entry of the window (the walk
 *      of 1743-1834): QHUFF_LINE_INDEXED | QHUFF_LINE_DYN.  Of several equal
 *      entries the HIGHEST absolute index: the reference takes the newer of
 *      its two candidates (1801-1824); its tables never hold more than two,
 *      for more this rule is the definition.  0x80 | (Base - 1 - abs) on 6
 *      bits (EHA_INDEXED_DYN, 2051-2060), or post-base 0x10 | (abs - Base) on
 *      4 bits (2042-2050); no N bit;
 *   3. the name is a static entry's (lsqpack_find_in_static_headers,
 *      1835-1866): QHUFF_LINE_NAMEREF, as qhuff_encode_headers;
 *   4. the name is that of an entry of the window: QHUFF_LINE_NAMEREF |
 *      QHUFF_LINE_DYN.  The LOWEST absolute index in the window: the
 *      reference's bucket lists are appended at the tail and it takes the
 *      first hit (1877-1901).  0x40 | N << 5 with the index on 4 bits
 *      (EHA_LIT_WITH_NAME_DYN, 2093-2109), or post-base 0x00 | N << 3 on 3
 *      bits (2079-2092); then lsqpack_enc_enc_str(7, value);
 *   5. QHUFF_LINE_LITERAL, as qhuff_encode_headers.
 * The section's prefix (lsqpack_enc_end_header, lsqpack.c:1267-1298): the
 * Required Insert Count RIC = 1 + the largest absolute index any of its lines
 * named, 0 if none; encoded RIC % (2 * max_entries) + 1 (0 for 0) on 8 bits;
 * then S = 0 and Base - RIC on 7 bits when Base >= RIC, else S = 1 and RIC -
 * Base - 1.  RIC = 0 gives 00 00 whatever Base is.  max_entries = 0 or an
 * empty window: no dynamic lines.
 *
 * Outputs: those of qhuff_encode_headers and dyn_id[n] (the absolute index
 * the line named, or QHUFF_DYN_NONE; may be NULL).  kind and static_id follow
 * the _dyn scan's conventions (static_id = QHUFF_STATIC_NONE on a dynamic
 * line), so qhuff_decode_headers_dyn_host on the output with the same table
 * and windows returns the same three arrays and the header lists.  `out`
 * must hold qhuff_encode_headers_dyn_bound(in_bytes, n, m) =
 * qhuff_encode_headers_bound(in_bytes, n, m).  The buffer contract above
 * applies: out[0 .. sec_out[m]), sec_out[0 .. m] and the optional arrays are
 * written, nothing else.
 *
 * Launches on `stream`, after one clear of the scratch: the index build
 * (two open-addressing indices over the d entries, by name+value hash and by
 * name hash, qhuff_dyn_index_slots(d) 32-bit slots each: the smallest power
 * of two >= 2d, at least 64; rebuilt on every call), the lookup, which writes
 * every header's two items with its section's Base and reduces each
 * section's largest reference into a word of scratch, a small launch that
 * writes every section's two prefix items from that word (all three timed as
 * QHUFF_KIND_HASH), then qhuff_encode_wire's launch and the gather of
 * sec_out unchanged.  For n = 0 every section is 00 00.  Scratch belongs to
 * the context, grown on demand and ordered across streams as
 * qhuff_encode_headers'.
 *
 * qhuff_encode_headers_dyn: device pointers, asynchronous.  QHUFF_EINVAL for
 * a null pointer, QHUFF_ERANGE when 2n + 2m passes 32 bits, first + d passes
 * 2^32 - 1 or d passes 2^28.  The form of sec_hdr, sec_win, sec_base and
 * tab->off is THE CALLER'S DUTY: the kernel clamps a window into [first,
 * first + d] and a Base to at most first + d, clamps an entry's offsets into
 * [off[0], off[2d]] and takes a decreasing pair as an empty string, so
 * nothing outside the arrays and the table's bytes is read, and items stay
 * inside their arrays.
 * qhuff_encode_headers_dyn_host: host pointers, synchronous -- one upload of
 * the headers and the table, the launches, then sec_out, the optional arrays
 * and exactly sec_out[m] bytes come back; the host's only loops are the
 * checks of the offsets, the windows and the Bases.  QHUFF_EINVAL for a null
 * pointer, for the sec_hdr / off faults of qhuff_encode_headers_host, for a
 * window or a Base outside the rule, for a decreasing tab->off; QHUFF_ERANGE
 * as there and as above; nothing is written then.
 *
 * qhuff_dyn_lookup / _host / _cpu: the lookup alone, as qhuff_static_lookup
 * is -- the two hashes (each may be NULL), kind, static_id and dyn_id (may be
 * NULL) per header, one window [win_lo, win_hi) for the whole call, under
 * the same rule.  A stateful encoder copies the results into its
 * lsxpack_header and skips its bucket walks.
 * The index build and the lookup launch, timed as QHUFF_KIND_HASH.  _cpu:
 * the kernel's lookup source on the host over host pointers, no context and
 * no device call; it returns what the host form returns.
 * qhuff_dyn_index_slots(d) (diagnostic, host only): the slots of each index
 * for a table of d entries; an entry's first slot is hash & (slots - 1), the
 * name+value hash in one index, the name hash in the other. */
#define QHUFF_FEATURE_ENCODE_HEADERS_DYN 1

int qhuff_dyn_lookup(qhuff_ctx *ctx, const uint8_t *in, const uint32_t *off,
                     uint32_t n, const struct qhuff_dyn_table *tab,
                     uint32_t win_lo, uint32_t win_hi, uint32_t *name_hash,
                     uint32_t *nameval_hash, uint8_t *kind,
                     uint8_t *static_id, uint32_t *dyn_id, void *stream);

int qhuff_dyn_lookup_host(qhuff_ctx *ctx, const uint8_t *in,
                          const uint32_t *off, uint32_t n,
                          const struct qhuff_dyn_table *tab, uint32_t win_lo,
                          uint32_t win_hi, uint32_t *name_hash,
                          uint32_t *nameval_hash, uint8_t *kind,
                          uint8_t *static_id, uint32_t *dyn_id);

int qhuff_dyn_lookup_cpu(const uint8_t *in, const uint32_t *off, uint32_t n,
                         const struct qhuff_dyn_table *tab, uint32_t win_lo,
                         uint32_t win_hi, uint32_t *name_hash,
                         uint32_t *nameval_hash, uint8_t *kind,
                         uint8_t *static_id, uint32_t *dyn_id);

uint32_t qhuff_dyn_index_slots(uint32_t d);

uint64_t qhuff_encode_headers_dyn_bound(uint64_t in_bytes, uint32_t n,
                                        uint32_t m);

int qhuff_encode_headers_dyn(qhuff_ctx *ctx, const uint8_t *in,
                             const uint32_t *off, uint32_t n,
                             const uint8_t *hflags, const uint32_t *sec_hdr,
                             uint32_t m, const struct qhuff_dyn_table *tab,
                             const uint32_t *sec_win,
                             const uint32_t *sec_base, uint8_t *out,
                             uint32_t *sec_out, uint8_t *kind,
                             uint8_t *static_id, uint32_t *dyn_id,
                             void *stream);

int qhuff_encode_headers_dyn_host(qhuff_ctx *ctx, const uint8_t *in,
                                  const uint32_t *off, uint32_t n,
                                  const uint8_t *hflags,
                                  const uint32_t *sec_hdr, uint32_t m,
                                  const struct qhuff_dyn_table *tab,
                                  const uint32_t *sec_win,
                                  const uint32_t *sec_base, uint8_t *out,
                                  uint32_t *sec_out, uint8_t *kind,
                                  uint8_t *static_id, uint32_t *dyn_id);

/* ---- the _dyn calls over many connections: a dynamic table per section -----
 * One struct qhuff_dyn_table is one QPACK connection; sec_win only lets the
 * sections of a batch see different moments of that one history.  These calls
 * take a set of T tables and, per section, the table it belongs to, so that
 * one batch holds sections of many connections.
 * QHUFF_FEATURE_HEADERS_TABS and the symbols announce it (the ABI version is
 * unchanged); the calls above behave as before, and a batch with T = 1 and
 * sec_tab all 0 gives through these calls exactly what it gives through them.
 *
 * struct qhuff_dyn_tables is a read-only view of T tables that share one
 * arena: `bytes` and `off` as in struct qhuff_dyn_table over all D = ent[T]
 * entries, table c's entries being the ordinals [ent[c], ent[c + 1]), oldest
 * first, entry ent[c] + k with the absolute index first[c] + k of that table;
 * max_entries[c] is its MaxEntries.  A table may be empty.  T = 0 with null
 * pointers is legal: every section then behaves as one of a table with d = 0
 * and max_entries = 0, and sec_tab may be NULL.
 *
 * Every call takes `tabs, sec_tab` where its _dyn counterpart takes `tab`:
 * sec_tab[s] (m entries) is the table of section s.  Everything else means
 * what it means there, read against table sec_tab[s]: sec_win[2s .. 2s + 1],
 * sec_base[s] and dyn_id[] are absolute indices of that table (a NULL sec_win:
 * the whole of that table); a DYN descriptor's instr is a byte offset in the
 * shared `bytes`.  The rules per section -- rc[s] (qhuff_scan_headers_dyn,
 * 1.-5.), the choice of the line and the prefix (qhuff_encode_headers_dyn,
 * 1.-5. and "The section's prefix") -- are those stated above, applied to
 * (tabs, sec_tab[s]); they are not restated here.
 *
 * qhuff_scan_headers_tabs / _host / _cpu: qhuff_scan_headers_dyn's three.
 * qhuff_decode_headers_tabs_host: the whole decode path in one call -- this
 * scan, then qhuff_decode_headers_dyn's launch unchanged on the shared bytes
 * (the descriptors already address them); `out` holds
 * qhuff_decode_headers_dyn_bound(wire bytes, max_hdrs, the longest entry of
 * all tables).
 * qhuff_dyn_lookup_tabs / _host / _cpu: the lookup alone, by sections: header
 * j of section s (sec_hdr[s] <= j < sec_hdr[s + 1]; sec_hdr as in
 * qhuff_encode_headers) is looked up in table sec_tab[s] within sec_win[2s ..
 * 2s + 1], under the encode calls' window rule.  _cpu: the kernel's lookup
 * source on the host.
 * qhuff_encode_headers_tabs / _host: qhuff_encode_headers_dyn's two; the
 * bound is qhuff_encode_headers_bound.  Launches: the index build -- ONE pair
 * of open-addressing indices over all D entries,
 * qhuff_dyn_tables_index_slots(D) slots each (the smallest power of two >= 2D,
 * at least 64), a slot holding a global ordinal + 1, an entry's first slot
 * (hash ^ mix(c)) & (slots - 1) with c its table: connections hold the same
 * popular headers, and without the table in the slot an entry held by every
 * one of T tables would make one probe run of length T --, the lookup, the
 * prefix launch with max_entries[sec_tab[s]], then qhuff_encode_wire's launch
 * and the gather of sec_out unchanged.
 *
 * Host and _cpu forms: QHUFF_EINVAL for a null pointer, ent[0] != 0 or a
 * decreasing ent, sec_tab[s] >= T, a decreasing off, a window or a Base
 * outside its table's rule (and for what the _dyn forms return it for);
 * QHUFF_ERANGE when first[c] + d_c passes 2^32 - 1, when D passes 2^28, and
 * for the _dyn forms' 32-bit bounds; nothing is written then.  The host's
 * only loops are these checks.
 * Device forms: tabs is a host struct of device pointers; the form of the
 * arrays is THE CALLER'S DUTY.  The kernels clamp sec_tab[s] to T - 1, ent
 * values to D (a decreasing pair is an empty table), windows and Bases into
 * their table and an entry's offsets as the _dyn kernels do, so nothing
 * outside the arrays is read or written.  The scan's kernels read D = ent[T]
 * on the device (so tabs->off may be NULL there only when T = 0:
 * QHUFF_EINVAL otherwise).  The lookup and encode forms size their indices
 * by D on the host: they read ent[T] back with one 4-byte copy on `stream` and wait for
 * it (the host forms, which know D, do not), then are asynchronous;
 * QHUFF_ERANGE when that D passes 2^28. */
#define QHUFF_FEATURE_HEADERS_TABS 1

struct qhuff_dyn_tables {          /* read-only view of T tables          */
    const uint8_t  *bytes;         /* every table's entries, packed        */
    const uint32_t *off;           /* off[2D + 1], D = ent[T]              */
    const uint32_t *ent;           /* ent[T + 1], ent[0] = 0: table c holds
                                      entry ordinals [ent[c], ent[c + 1]),
                                      oldest first                         */
    const uint32_t *first;         /* first[T]: absolute index of table c's
                                      entry ent[c]                         */
    const uint32_t *max_entries;   /* max_entries[T]                       */
    uint32_t T;
};

int qhuff_scan_headers_tabs(qhuff_ctx *ctx, const uint8_t *buf,
                            const uint32_t *sec_off, uint32_t m,
                            const struct qhuff_dyn_tables *tabs,
                            const uint32_t *sec_tab, const uint32_t *sec_win,
                            struct qhuff_hstr *strs, uint32_t max_hdrs,
                            uint32_t *hdr_off, int32_t *rc, uint8_t *kind,
                            uint8_t *static_id, uint8_t *hflags,
                            uint32_t *dyn_id, void *stream);

int qhuff_scan_headers_tabs_host(qhuff_ctx *ctx, const uint8_t *buf,
                                 const uint32_t *sec_off, uint32_t m,
                                 const struct qhuff_dyn_tables *tabs,
                                 const uint32_t *sec_tab,
                                 const uint32_t *sec_win,
                                 struct qhuff_hstr *strs, uint32_t max_hdrs,
                                 uint32_t *hdr_off, int32_t *rc, uint8_t *kind,
                                 uint8_t *static_id, uint8_t *hflags,
                                 uint32_t *dyn_id);

int qhuff_scan_headers_tabs_cpu(const uint8_t *buf, const uint32_t *sec_off,
                                uint32_t m,
                                const struct qhuff_dyn_tables *tabs,
                                const uint32_t *sec_tab,
                                const uint32_t *sec_win,
                                struct qhuff_hstr *strs, uint32_t max_hdrs,
                                uint32_t *hdr_off, int32_t *rc, uint8_t *kind,
                                uint8_t *static_id, uint8_t *hflags,
                                uint32_t *dyn_id);

int qhuff_decode_headers_tabs_host(qhuff_ctx *ctx, const uint8_t *buf,
                                   const uint32_t *sec_off, uint32_t m,
                                   const struct qhuff_dyn_tables *tabs,
                                   const uint32_t *sec_tab,
                                   const uint32_t *sec_win, uint32_t max_len,
                                   uint32_t max_hdrs, uint32_t *hdr_off,
                                   int32_t *rc, uint8_t *kind,
                                   uint8_t *static_id, uint8_t *hflags,
                                   uint32_t *dyn_id, uint8_t *out,
                                   uint32_t *off, uint8_t *status,
                                   uint32_t *name_hash,
                                   uint32_t *nameval_hash);

int qhuff_dyn_lookup_tabs(qhuff_ctx *ctx, const uint8_t *in,
                          const uint32_t *off, uint32_t n,
                          const uint32_t *sec_hdr, uint32_t m,
                          const struct qhuff_dyn_tables *tabs,
                          const uint32_t *sec_tab, const uint32_t *sec_win,
                          uint32_t *name_hash, uint32_t *nameval_hash,
                          uint8_t *kind, uint8_t *static_id, uint32_t *dyn_id,
                          void *stream);

int qhuff_dyn_lookup_tabs_host(qhuff_ctx *ctx, const uint8_t *in,
                               const uint32_t *off, uint32_t n,
                               const uint32_t *sec_hdr, uint32_t m,
                               const struct qhuff_dyn_tables *tabs,
                               const uint32_t *sec_tab,
                               const uint32_t *sec_win, uint32_t *name_hash,
                               uint32_t *nameval_hash, uint8_t *kind,
                               uint8_t *static_id, uint32_t *dyn_id);

int qhuff_dyn_lookup_tabs_cpu(const uint8_t *in, const uint32_t *off,
                              uint32_t n, const uint32_t *sec_hdr, uint32_t m,
                              const struct qhuff_dyn_tables *tabs,
                              const uint32_t *sec_tab,
                              const uint32_t *sec_win, uint32_t *name_hash,
                              uint32_t *nameval_hash, uint8_t *kind,
                              uint8_t *static_id, uint32_t *dyn_id);

uint32_t qhuff_dyn_tables_index_slots(uint32_t D);

int qhuff_encode_headers_tabs(qhuff_ctx *ctx, const uint8_t *in,
                              const uint32_t *off, uint32_t n,
                              const uint8_t *hflags, const uint32_t *sec_hdr,
                              uint32_t m, const struct qhuff_dyn_tables *tabs,
                              const uint32_t *sec_tab,
                              const uint32_t *sec_win,
                              const uint32_t *sec_base, uint8_t *out,
                              uint32_t *sec_out, uint8_t *kind,
                              uint8_t *static_id, uint32_t *dyn_id,
                              void *stream);

int qhuff_encode_headers_tabs_host(qhuff_ctx *ctx, const uint8_t *in,
                                   const uint32_t *off, uint32_t n,
                                   const uint8_t *hflags,
                                   const uint32_t *sec_hdr, uint32_t m,
                                   const struct qhuff_dyn_tables *tabs,
                                   const uint32_t *sec_tab,
                                   const uint32_t *sec_win,
                                   const uint32_t *sec_base, uint8_t *out,
                                   uint32_t *sec_out, uint8_t *kind,
                                   uint8_t *static_id, uint32_t *dyn_id);

/* ---- encoder-stream inserts applied to the connections' tables --------------
 * The _tabs calls read a set of tables; these calls make the next one.  Chunk
 * c, buf[enc_off[c] .. enc_off[c + 1]), is encoder-stream bytes of connection
 * c (one chunk a table, T chunks); its complete instructions are applied to
 * table c in order, as lsqpack_dec_enc_in does (lsqpack.c:4574-5030), and the
 * T tables that result are written as a new arena, directly a struct
 * qhuff_dyn_tables for the calls above.  A partial last instruction is left
 * unconsumed, as by qhuff_scan_encoder_stream.  QHUFF_FEATURE_TABS_INSERT and
 * the symbols announce it (the ABI version is unchanged); no call above
 * changes.  The decoder stream, which blocked sections to submit again and
 * everything the encoder decides stay with the host.
 *
 * State of table c: (cap, lo, ins, used) -- cap the capacity in bytes now in
 * force (qpd_cur_max_capacity), lo the oldest live absolute index, ins the
 * insert count (first[c] + d_c on entry), used the sum of name + value + 32
 * over [lo, ins) (DTE_SIZE, qpd_cur_capacity).  struct qhuff_ins_state gives
 * cap[T], max_cap[T] (qpd_max_capacity) and live_lo[T]; entries of the set
 * below live_lo[c] are history kept for sections decoded earlier.
 *
 * Rules, the reference's, on complete instructions only (the reference can
 * reject a partial one early by its declared length or index; here the
 * verdict waits for the whole instruction -- a stated difference):
 *   Set Dynamic Table Capacity v   v > max_cap[c] fails (lsqpack.c:5015);
 *       else cap = v and entries are evicted from lo while used > cap
 *       (qdec_update_max_capacity, 4362-4377).
 *   Insert With Name Reference, static   index >= 99 fails (4620-4623).
 *   Insert With Name Reference, dynamic, and Duplicate   a = ins - 1 - idx in
 *       64 bits; fails unless lo <= a < ins at that moment
 *       (qdec_get_table_entry_rel, 2756-2764; 4627-4630, 4987-4989): after
 *       the evictions of the chunk's earlier instructions, before this
 *       insert's own.  a may be an entry inserted earlier in the same chunk.
 *   Lengths, on wire lengths, in 64 bits   a literal name of wire length Ln
 *       with H bit Hn fails when Ln > cap << 2 * Hn (4798); with N the decoded
 *       name's length, whatever its source, N > cap fails (4661, 4878), and
 *       the value's wire length Lv fails when Lv > (cap - N) << 2 * Hv (4666,
 *       4883).  A Duplicate has no such check.
 *   A literal the Huffman decoder rejects fails.
 *   Push (lsqpack_dec_push_entry, 4534-4552)   ins += 1, used += size, then
 *       entries are evicted from lo while used > cap.  An entry that passed
 *       the checks above but is larger than cap evicts everything, itself
 *       included (lo = ins, used = 0), and is not an error.  RFC 9204 3.2.2
 *       calls that an error; the reference is the definition here.
 *   rc[c] = QHUFF_OK or QHUFF_EPROTO (the reference's -1).  A chunk that fails
 *       changes nothing: its table comes out as it went in, no entry of it is
 *       inserted and consumed[c] = 0; other chunks are unaffected.
 * References are absolute indices where the reference's modular ids would
 * alias, as in the calls above.
 *
 * Per chunk:   rc[T], consumed[T], ins_off[T + 1] -- the inserts of chunk c
 *   are the ordinals [ins_off[c], ins_off[c + 1]); ins_off[T] is the full
 *   count whatever max_ins is.  The ordinals are given out by the scan, before
 *   anything is decoded: a chunk the scan rejects (an integer, a static index,
 *   a capacity, Ln) has none; one rejected later (liveness, N, Lv, Huffman)
 *   keeps its ordinals, with ins_lo[k] = live_lo[c] for each.
 * Per insert k: ins_kind[k] = QHUFF_INS_*; ins_ref[k] = the absolute index
 *   named, or QHUFF_DYN_NONE (also for an idx past the first insert);
 *   ins_lo[k] = the oldest live absolute index right after insert k and its
 *   evictions: a section decoded between inserts k and k + 1 has sec_win =
 *   (ins_lo[k], first[c] + d_c + (k - ins_off[c]) + 1).
 * The next set:  out_bytes, out_off[2D' + 1], out_ent[T + 1], out_first[T],
 *   cap_out[T], live_lo_out[T]; cap_out and live_lo_out include the chunk's
 *   trailing Set Capacity instructions.  Entry out_ent[c] + k has the
 *   absolute index out_first[c] + k.  keep[T] (or NULL) is the lowest
 *   absolute index to retain, clamped into [first[c], live_lo_out[c]]; NULL
 *   retains exactly the live entries.  An empty table holds no bytes.
 *   out_bytes must hold qhuff_tabs_insert_bound(arena_bytes, wire_bytes,
 *   max_ins, dyn_longest) = arena_bytes + qhuff_decode_headers_dyn_bound(
 *   wire_bytes, max_ins, dyn_longest) bytes -- the old arena plus everything
 *   the inserts can decode to --, out_off 2 * (D + max_ins) + 1 entries.
 *
 * struct qhuff_ins_scan is what the scan leaves for the apply: the per-chunk
 * and per-insert arrays above, chunk_cap[2T] (the minimum and the last
 * capacity behind a chunk's last insert), two struct qhuff_hstr per insert
 * (name, value) under the order rule -- WIRE for a literal, STATIC for a
 * static name, DYN for a name or a duplicate taken from an entry of the input
 * set -- root[2 * max_ins] and ins_cap[2 * max_ins] (the minimum capacity
 * since the previous insert and the capacity in force).  A reference to an
 * insert of the same chunk cannot be sized before decoding: it is a DYN
 * descriptor of length 0 and root[] names the string of the same chunk whose
 * bytes it takes (chains collapsed; QHUFF_DYN_NONE: the string's own).
 *
 * qhuff_scan_inserts_tabs: device pointers, asynchronous: the scan's three
 *   launches on the scan's scratch (QHUFF_KIND_SCAN).  The caller reads
 *   ins_off[T].
 * qhuff_apply_inserts_tabs: device pointers, asynchronous; n_ins = ins_off[T]
 *   (<= max_ins), wire_bytes = enc_off[T] - enc_off[0]: qhuff_decode_headers_
 *   dyn's launch unchanged on the descriptors (max_len 0), the accounting (a
 *   table a lane), the sums, the copy (a table a wave), the last three timed
 *   as QHUFF_KIND_SCAN.  Scratch belongs to the context.  st->arena_bytes = the bytes of tabs->bytes (>= off[2D]),
 *   st->dyn_longest >= the longest entry, o->out_cap / o->ent_cap = what
 *   out_bytes / out_off hold: nothing is written past them.  The form of the
 *   arrays is THE CALLER'S DUTY; what the kernels read of ent, off, enc_off,
 *   live_lo, keep, root and the scan's arrays is clamped, so wrong arrays give
 *   wrong bytes and no access outside the arrays -- with one value trusted,
 *   as by the _tabs kernels above: D = ent[T], which the kernels read on the
 *   device and clamp everything else to; off must hold 2 * ent[T] + 1
 *   entries.
 * qhuff_tabs_insert_host: host pointers, synchronous, the whole path: wire
 *   bytes and tables go up once.  sc->strs, root, ins_cap, chunk_cap may be
 *   NULL.  QHUFF_EINVAL unless first[c] <= live_lo[c] <= first[c] + d_c, used
 *   <= cap[c] <= max_cap[c] <= 2^28 and max_entries[c] == max_cap[c] / 32 (and
 *   for what tabs_check rejects, a decreasing enc_off, a null pointer);
 *   QHUFF_ERANGE when ins_off[T] > max_ins (rc, consumed and ins_off valid,
 *   nothing applied, the tables not written), when first + d + inserts
 *   passes 2^32 - 1 or an arena passes 32 bits.
 * qhuff_tabs_insert_cpu: the same shared source on the host, no context; its
 *   literals are decoded by a host Huffman decoder of this library. */
#define QHUFF_FEATURE_TABS_INSERT 1
#define QHUFF_INS_LITERAL 0     /* insert with literal name                 */
#define QHUFF_INS_STATIC  1     /* insert with static name reference        */
#define QHUFF_INS_DYN     2     /* insert with dynamic name reference       */
#define QHUFF_INS_DUP     3     /* duplicate                                */

struct qhuff_ins_state {
    const uint32_t *cap;        /* cap[T]                                   */
    const uint32_t *max_cap;    /* max_cap[T]                               */
    const uint32_t *live_lo;    /* live_lo[T]                               */
    uint32_t arena_bytes;       /* device forms: bytes of tabs->bytes       */
    uint32_t dyn_longest;       /* device forms: >= the longest entry       */
};

struct qhuff_ins_scan {
    int32_t  *rc;               /* T                                        */
    uint32_t *consumed;         /* T                                        */
    uint32_t *ins_off;          /* T + 1                                    */
    uint32_t *chunk_cap;        /* 2T                                       */
    struct qhuff_hstr *strs;    /* 2 * max_ins                              */
    uint32_t *root;             /* 2 * max_ins                              */
    uint32_t *ins_cap;          /* 2 * max_ins                              */
    uint32_t *ins_ref;          /* max_ins                                  */
    uint8_t  *ins_kind;         /* max_ins                                  */
    uint32_t max_ins;
};

struct qhuff_ins_out {
    uint32_t *ins_lo;           /* max_ins                                  */
    uint8_t  *out_bytes;
    uint32_t *out_off;          /* 2 * ent_cap + 1                          */
    uint32_t *out_ent;          /* T + 1                                    */
    uint32_t *out_first;        /* T                                        */
    uint32_t *cap_out;          /* T                                        */
    uint32_t *live_lo_out;      /* T                                        */
    uint64_t out_cap;           /* bytes out_bytes holds                    */
    uint32_t ent_cap;           /* entries out_off holds (D + max_ins)      */
};

uint64_t qhuff_tabs_insert_bound(uint64_t arena_bytes, uint64_t wire_bytes,
                                 uint32_t max_ins, uint32_t dyn_longest);

int qhuff_scan_inserts_tabs(qhuff_ctx *ctx,
                            const struct qhuff_dyn_tables *tabs,
                            const struct qhuff_ins_state *st,
                            const uint8_t *buf, const uint32_t *enc_off,
                            const struct qhuff_ins_scan *sc, void *stream);

int qhuff_apply_inserts_tabs(qhuff_ctx *ctx,
                             const struct qhuff_dyn_tables *tabs,
                             const struct qhuff_ins_state *st,
                             const uint8_t *buf, uint32_t wire_bytes,
                             const uint32_t *keep,
                             const struct qhuff_ins_scan *sc, uint32_t n_ins,
                             const struct qhuff_ins_out *o, void *stream);

int qhuff_tabs_insert_host(qhuff_ctx *ctx,
                           const struct qhuff_dyn_tables *tabs,
                           const struct qhuff_ins_state *st,
                           const uint8_t *buf, const uint32_t *enc_off,
                           const uint32_t *keep,
                           const struct qhuff_ins_scan *sc,
                           const struct qhuff_ins_out *o);

int qhuff_tabs_insert_cpu(const struct qhuff_dyn_tables *tabs,
                          const struct qhuff_ins_state *st,
                          const uint8_t *buf, const uint32_t *enc_off,
                          const uint32_t *keep,
                          const struct qhuff_ins_scan *sc,
                          const struct qhuff_ins_out *o);

/* ---- encoder-side hook ---------------------------
 * lsqpack_enc_enc_str (lsqpack.c:839-876) for a string whose Huffman
 * payload was precomputed by a QHUFF_ENC_PAYLOAD batch (huff, huff_len =
 * that batch's output i; huff_len is also qenc_enc_str_size, the figure the
 * ratio guard at lsqpack.c:1946-1957 reads).  Same bytes, return value and
 * -1 on short dst_len as the reference; bits of dst[0] above the H bit are
 * kept.  Host-only, no device call: a patched lsqpack.c calls it per literal
 * after batch-encoding every name and value of a header list up front
 * (INTEGRATION.md). */
int qhuff_frame_literal(unsigned prefix_bits, unsigned char *dst,
                        size_t dst_len, const unsigned char *str,
                        unsigned str_len, const unsigned char *huff,
                        unsigned huff_len);

/* ---- header hashing ---------------------
 * XXH32 (deps/xxhash/xxhash.c) of header names and values, as the reference
 * computes it for every header it encodes (lsqpack.c:1681-1685) or decodes
 * (lsqpack.c:3268-3269, 3308-3309), seeded with LSQPACK_XXH_SEED
 * (lsqpack.c:623) to index its static and dynamic tables. */
#define QHUFF_XXH_SEED 39378473u

/* n headers (device pointers); header i is name in[off[2i] .. off[2i+1])
 * followed by value in[off[2i+1] .. off[2i+2]) (2n + 1 offsets, the name /
 * value layout of an lsxpack_header buffer).  Writes
 *   name_hash[i]    = XXH32(name,  name_len,  seed)
 *   nameval_hash[i] = XXH32(value, value_len, name_hash[i]).
 * Asynchronous on `stream`. */
int qhuff_xxh32_headers(qhuff_ctx *ctx, const uint8_t *in,
                        const uint32_t *off, uint32_t n, uint32_t seed,
                        uint32_t *name_hash, uint32_t *nameval_hash,
                        void *stream);

/* n independent strings (device pointers, n + 1 offsets as in the codec
 * batches): hash[i] = XXH32(string i, seed).  Asynchronous on `stream`. */
int qhuff_xxh32_batch(qhuff_ctx *ctx, const uint8_t *in,
                      const uint32_t *in_off, uint32_t n, uint32_t seed,
                      uint32_t *hash, void *stream);

/* Host-memory variant of qhuff_xxh32_headers (pinned staging, H2D, kernel,
 * D2H; synchronous): off is a host array of 2n + 1 offsets into in. */
int qhuff_xxh32_headers_host(qhuff_ctx *ctx, const uint8_t *in,
                             const uint32_t *off, uint32_t n, uint32_t seed,
                             uint32_t *name_hash, uint32_t *nameval_hash);

/* Last HIP error string for this context (diagnostics); with ctx == NULL,
 * the reason of the calling thread's last failed qhuff_open. */
const char *qhuff_last_error(qhuff_ctx *ctx);

/* Synchronise the device and return (then clear) the context's sticky device
 * error word: 0 = no error; QHUFF_DEVERR_SPIN = a look-back wait gave up;
 * QHUFF_DEVERR_RANGE = an output offset passed 2^32 (outputs of that launch
 * are invalid).  Negative QHUFF_E* on HIP failure.  The asynchronous batch
 * calls also report such an error: the next qhuff_encode_batch /
 * qhuff_decode_batch on the context returns QHUFF_EDEVICE (and clears it)
 * once the launch that hit it has completed. */
#define QHUFF_DEVERR_SPIN 1
#define QHUFF_DEVERR_RANGE 2
int qhuff_device_error(qhuff_ctx *ctx);

/* Diagnostic: in a QHUFF_PROFILE build (libqhuff_prof.so) copy up to
 * max_words per-wave phase stamps of the last launch into dst and return
 * the number available; 0 in normal builds.  In a QH_PATH_TRACE build
 * (libqhuff_trace.so) the words are the last tile launch's path records,
 * 8 per tile in tile order.  Synchronous. */
uint64_t qhuff_profile_read(qhuff_ctx *ctx, uint64_t *dst, uint64_t max_words);

/* Launch timing.  With timing on, every encode / decode / hash / scan launch of
 * the context is dispatched with a pair of HIP events that carry the
 * dispatch's own start and end timestamps (hipExtLaunchKernel: the kernel's
 * device time, what rocprofv3's kernel trace reports, with no timing
 * packets queued around the launch), kept in a ring of the last
 * QHUFF_TIMING_SLOTS launches.  qhuff_timing_read waits for them and
 * returns, oldest first, the launches timed since timing was enabled or
 * last read (at most `max`, the most recent ones): kind[i] (QHUFF_KIND_*)
 * and us[i], microseconds.  qhuff_timing_enable(ctx, 0) turns it off;
 * `on` = k > 1 (ABI 5) times only every k-th launch of each kind, counted
 * from the call (a timed launch costs a few microseconds of queue time).
 * Return QHUFF_OK / the count, or QHUFF_E*. */
#define QHUFF_TIMING_SLOTS 256
#define QHUFF_KIND_ENCODE 0
#define QHUFF_KIND_DECODE 1
#define QHUFF_KIND_HASH   2
#define QHUFF_KIND_SCAN   3     /* each of qhuff_scan_sections' three launches */
int qhuff_timing_enable(qhuff_ctx *ctx, int on);
int qhuff_timing_read(qhuff_ctx *ctx, uint32_t *kind, double *us, uint32_t max);

/* Kernel variants.  Encode and decode each have a lean kernel and a full
 * one that also carries the big-tile slots and the cooperative long-string
 * decode.  By default (QHUFF_KERNELS=auto) a launch runs the full kernel,
 * unless its batch is known to need only the lean one: the host-memory calls
 * read their offsets, a device-pointer caller may pass a hint (below);
 * QHUFF_KERNELS=lean|full pins one.  (Until ABI 6 decode chose by a history
 * of earlier launches.)  Returns 1 if the context's last launch of `kind`
 * (QHUFF_KIND_ENCODE / QHUFF_KIND_DECODE) ran the full kernel, 0 if the
 * lean one or none yet, QHUFF_EINVAL otherwise.  Diagnostic: the output
 * bytes are the same either way.
 * QHUFF_LB_REPLICA, read at qhuff_open like QHUFF_KERNELS, is a test and A/B
 * knob of the tile kernels' look-back: the super-tile flags are kept in
 * several replicas, and by default (unset, -1 or out of range) a wave polls
 * the replica of its workgroup; r pins every wave's polls to replica r.
 * The output bytes are the same either way. */
int qhuff_kernel_variant(qhuff_ctx *ctx, int kind);

/* Diagnostic: the most waves one launch of `kind` (QHUFF_KIND_ENCODE /
 * _DECODE / _HASH) puts on the device -- workgroups per launch x waves per
 * workgroup, after QHUFF_GRID_WG_PER_CU / QHUFF_GRID_PCT.  QHUFF_EINVAL for
 * a null context or another kind.  Host arithmetic only.
 * QHUFF_FEATURE_GRID_WAVES and the symbol announce it (the ABI version is
 * unchanged). */
#define QHUFF_FEATURE_GRID_WAVES 1
int qhuff_grid_waves(qhuff_ctx *ctx, int kind);

/* (ABI 6) The variant of the next launch of `kind` from what the caller
 * knows of its batch: hint 1 = the batch has
 * a string longer than 128 bytes or a 64-string tile spanning more than the
 * kernels' 3 KB stage (the full kernel), 0 = it has none (the lean one),
 * -1 = no hint.  Applies to the next launch of that kind only.  The host-
 * memory calls (qhuff_*_batch_host, qhuff_decode_literals_*) set it
 * themselves from the offsets they hold; a caller of the device-pointer
 * calls that keeps a host copy of its offsets (e.g. from
 * qhuff_scan_field_section) can compute it with qhuff_batch_needs_full. */
int qhuff_batch_hint(qhuff_ctx *ctx, int kind, int hint);

/* 1 if host offsets in_off[n + 1] describe a batch the full kernel is for
 * (the rule above), 0 if not, QHUFF_EINVAL for a null pointer.  Host only. */
int qhuff_batch_needs_full(const uint32_t *in_off, uint32_t n);

/* ---- multi-GPU sharding helpers (host arithmetic only) ----------------
 * Byte-balanced contiguous partition of a batch into g shards: writes
 * g + 1 string indices to cuts (cuts[0] = 0, cuts[g] = n) so shard k holds
 * strings [cuts[k], cuts[k+1]) with roughly equal input bytes
 * (SURVEY.md section 8(e)). */
int qhuff_shard_cuts(const uint32_t *in_off, uint32_t n, uint32_t g,
                     uint32_t *cuts);

/* (ABI 7) One batch over g contexts -- one per GPU, or several on one GPU
 * (distinct contexts; none in use by another thread during the call).  The
 * path shards trivially (a string's output depends only on its own bytes,
 * lsqpack.c:5085-5195, 5234-5466): the batch is cut by qhuff_shard_cuts
 * into g contiguous shards, shard k runs on ctxs[k] on a host thread of its
 * own (the calling thread takes shard 0), and the outputs are stitched by
 * each shard's base, the exclusive scan of the shard totals.  No
 * collective.
 *
 * Host memory: the arguments, outputs and return codes of
 * qhuff_encode_batch_host / qhuff_decode_batch_host on one context, and the
 * same bytes (out_off is global).  Each shard's uploads, kernels and
 * downloads run unsynchronised; only its copies into `out` wait for the
 * earlier shards' totals.  (Registered buffers, qhuff_host_register: the
 * shards write `out` directly only when the whole call's bound lies in one
 * registered range.)  Synchronous. */
int qhuff_encode_batch_host_multi(qhuff_ctx *const *ctxs, uint32_t g,
                                  const uint8_t *in, const uint32_t *in_off,
                                  uint32_t n, unsigned mode, uint8_t *out,
                                  uint32_t *out_off);
int qhuff_decode_batch_host_multi(qhuff_ctx *const *ctxs, uint32_t g,
                                  const uint8_t *in, const uint32_t *in_off,
                                  uint32_t n, uint8_t *out, uint32_t *out_off,
                                  uint8_t *status);

/* Device-resident shards (shard k in ctxs[k]'s device memory, laid out as
 * for qhuff_encode_batch / qhuff_decode_batch; status unused by encode;
 * stream: an opaque hipStream_t of that device, NULL = its default stream).
 * Launches every shard, waits for them, and writes base[0 .. g]: base[k] =
 * the output bytes of shards [0, k), base[g] the total.  rebase != 0: shard
 * k's out_off (n_k + 1 entries) is also rebased by base[k] on its device, so
 * that it indexes the concatenation of the shards' outputs (the stitched
 * batch; the total must fit 32 bits, else QHUFF_ERANGE).  Synchronous. */
struct qhuff_shard
{
    const uint8_t  *in;
    const uint32_t *in_off;
    uint32_t        n;
    uint8_t        *out;
    uint32_t       *out_off;
    uint8_t        *status;
    void           *stream;
};
int qhuff_encode_batch_multi(qhuff_ctx *const *ctxs, uint32_t g,
                             const struct qhuff_shard *shards, unsigned mode,
                             uint64_t *base, int rebase);
int qhuff_decode_batch_multi(qhuff_ctx *const *ctxs, uint32_t g,
                             const struct qhuff_shard *shards, uint64_t *base,
                             int rebase);

/* Synthetic header-string batch: xorshift64
 * seeded with `seed` (0 -> 0x9E3779B97F4A7C15); len = min_len +
 * r % (max_len - min_len + 1); bytes alphabet[r % alphabet_len].  Host
 * buffers: in_off gets n + 1 entries; data must hold n * max_len bytes.
 * Returns the total bytes written. */
uint64_t qhuff_synth_batch(uint64_t seed, uint32_t n, uint32_t min_len,
                           uint32_t max_len, const uint8_t *alphabet,
                           uint32_t alphabet_len, uint8_t *data,
                           uint32_t *in_off);

#ifdef __cplusplus
}
#endif

#endif
