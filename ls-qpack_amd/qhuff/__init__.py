"""Python plumbing over libqhuff.so (include/qhuff.h).

The product is the C-ABI library (HIP kernels for gfx950 + host C); this
module only binds it with ctypes so tests and bench.py can drive it with
torch device tensors.  There is no CPU fallback: if libqhuff.so is missing or
no gfx950 device is usable, Codec() raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
PKG_ROOT = os.path.dirname(_HERE)                 # .../ls-qpack_amd
LIB_PATH = os.environ.get("QHUFF_LIB") or os.path.join(PKG_ROOT, "libqhuff.so")
HEADER = os.path.join(os.path.dirname(PKG_ROOT), "include", "qhuff.h")
HEADERS = (HEADER, os.path.join(os.path.dirname(PKG_ROOT), "include",
                                "qhuff_lsqpack.h"))

OK = 0
EINVAL, ENOMEM, ENODEV, ERANGE, EDEVICE = -22, -12, -19, -34, -5
ENC_PAYLOAD, ENC_LITERAL3, ENC_LITERAL5, ENC_LITERAL7 = 0, 3, 5, 7
DEC_OK, DEC_ERROR = 0, 1
DEC_MORE = 2                              # QHUFF_DEC_MORE (qhuff_decode_stream)
STREAM_FINAL = 1                          # QHUFF_STREAM_FINAL, flags bit 0
HUFF_DEC_OK, HUFF_DEC_END_SRC, HUFF_DEC_END_DST, HUFF_DEC_ERROR = 0, 1, 2, 3

# every function include/qhuff.h declares (checked by tests/test_abi.py)
EXPORTS = (
    "qhuff_open", "qhuff_close", "qhuff_encode_bound", "qhuff_decode_bound",
    "qhuff_encode_batch", "qhuff_decode_batch", "qhuff_encode_batch_host",
    "qhuff_decode_batch_host", "qhuff_enc_enc_str", "qhuff_enc_str_size",
    "qhuff_huff_decode", "qhuff_huff_decode_ex", "qhuff_abi_version",
    "qhuff_last_error", "qhuff_shard_cuts",
    "qhuff_synth_batch", "qhuff_device_error", "qhuff_profile_read",
    "qhuff_xxh32_headers", "qhuff_xxh32_batch",
    "qhuff_scan_field_section", "qhuff_scan_encoder_stream",
    "qhuff_literals_bound", "qhuff_decode_literals_host",
    "qhuff_decode_literals_ex", "qhuff_batch_hint", "qhuff_batch_needs_full",
    "qhuff_frame_literal", "qhuff_xxh32_headers_host",
    "qhuff_svc_open", "qhuff_svc_close", "qhuff_svc_encode",
    "qhuff_svc_decode", "qhuff_svc_stats", "qhuff_svc_pieces",
    "qhuff_timing_enable", "qhuff_timing_read", "qhuff_kernel_variant",
    "qhuff_dec_int", "qhuff_encode_batch_host_multi",
    "qhuff_decode_batch_host_multi", "qhuff_encode_batch_multi",
    "qhuff_decode_batch_multi", "qhuff_host_register", "qhuff_host_unregister",
    "qhuff_host_chunks",
    "qhuff_decode_stream_bound", "qhuff_decode_stream",
    "qhuff_decode_stream_host",
    "qhuff_literals_check", "qhuff_decode_wire", "qhuff_decode_wire_host",
    "qhuff_grid_waves",
    "qhuff_encode_wire_bound", "qhuff_items_check", "qhuff_encode_wire",
    "qhuff_encode_wire_host",
    "qhuff_scan_sections", "qhuff_scan_sections_host",
    "qhuff_decode_sections_host", "qhuff_scan_sections_cpu",
    "qhuff_static_lookup", "qhuff_static_lookup_host",
    "qhuff_static_lookup_cpu", "qhuff_static_probe_tables",
    "qhuff_encode_headers_bound", "qhuff_encode_headers",
    "qhuff_encode_headers_host",
    "qhuff_scan_headers", "qhuff_scan_headers_host", "qhuff_scan_headers_cpu",
    "qhuff_decode_headers_bound", "qhuff_decode_headers",
    "qhuff_decode_headers_host",
    "qhuff_scan_headers_dyn", "qhuff_scan_headers_dyn_host",
    "qhuff_scan_headers_dyn_cpu", "qhuff_decode_headers_dyn_bound",
    "qhuff_decode_headers_dyn", "qhuff_decode_headers_dyn_host",
    "qhuff_dyn_lookup", "qhuff_dyn_lookup_host", "qhuff_dyn_lookup_cpu",
    "qhuff_dyn_index_slots", "qhuff_encode_headers_dyn_bound",
    "qhuff_encode_headers_dyn", "qhuff_encode_headers_dyn_host",
    "qhuff_scan_headers_tabs", "qhuff_scan_headers_tabs_host",
    "qhuff_scan_headers_tabs_cpu", "qhuff_decode_headers_tabs_host",
    "qhuff_dyn_lookup_tabs", "qhuff_dyn_lookup_tabs_host",
    "qhuff_dyn_lookup_tabs_cpu", "qhuff_dyn_tables_index_slots",
    "qhuff_encode_headers_tabs", "qhuff_encode_headers_tabs_host",
    "qhuff_tabs_insert_bound", "qhuff_scan_inserts_tabs",
    "qhuff_apply_inserts_tabs", "qhuff_tabs_insert_host",
    "qhuff_tabs_insert_cpu",
    # include/qhuff_lsqpack.h
    "qhuff_lsqpack_enc_enc_str", "qhuff_lsqpack_huff_decode",
    "qhuff_lsqpack_set_decode_full", "qhuff_lsqpack_set_device",
    "qhuff_lsqpack_set_context",
)
EPROTO, ETRUNC = -71, -61
ENOTSUP = -95                             # QHUFF_ENOTSUP (qhuff_scan_headers)
EBLOCKED = -11                            # QHUFF_EBLOCKED (qhuff_scan_headers_dyn)
HSTR_WIRE, HSTR_STATIC, HSTR_DYN = 0, 1, 2    # QHUFF_HSTR_*
LINE_DYN = 4                              # QHUFF_LINE_DYN
DYN_NONE = 0xFFFFFFFF                     # QHUFF_DYN_NONE
INS_LITERAL, INS_STATIC, INS_DYN, INS_DUP = 0, 1, 2, 3    # QHUFF_INS_*
HSTR_WIRE, HSTR_STATIC = 0, 1             # QHUFF_HSTR_*
TIMING_SLOTS = 256                        # QHUFF_TIMING_SLOTS
KIND_ENCODE, KIND_DECODE, KIND_HASH = 0, 1, 2
KIND_SCAN = 3                             # qhuff_scan_sections' three launches
SCAN_FIELD_SECTION, SCAN_ENCODER_STREAM = 0, 1    # QHUFF_SCAN_*
LIT_NAME, LIT_VALUE = 1, 2
MAX_STRLEN = 65535                        # QHUFF_MAX_STRLEN (LSXPACK_MAX_STRLEN)

XXH_SEED = 39378473                       # LSQPACK_XXH_SEED, lsqpack.c:623
HDR_NEVER_INDEX = 1                       # QHUFF_HDR_NEVER_INDEX, hflags bit 0
LINE_INDEXED, LINE_NAMEREF, LINE_LITERAL = 0, 1, 2    # QHUFF_LINE_*
STATIC_NONE = 0xFF                        # QHUFF_STATIC_NONE


class QhuffError(RuntimeError):
    pass


class Literal(C.Structure):
    """struct qhuff_literal (include/qhuff.h)"""
    _fields_ = [("pos", C.c_uint32), ("len", C.c_uint32),
                ("huffman", C.c_uint8), ("prefix_bits", C.c_uint8),
                ("kind", C.c_uint8), ("hdr_len", C.c_uint8),
                ("instr", C.c_uint32)]


class Hstr(C.Structure):
    """struct qhuff_hstr (include/qhuff.h): one string of a header"""
    _fields_ = [("pos", C.c_uint32), ("len", C.c_uint32),
                ("huffman", C.c_uint8), ("source", C.c_uint8),
                ("kind", C.c_uint8), ("static_id", C.c_uint8),
                ("instr", C.c_uint32)]


class Item(C.Structure):
    """struct qhuff_item (include/qhuff.h): one item of encode_wire -- an
    optional prefixed integer, then an optional literal of string i"""
    _fields_ = [("ival", C.c_uint32), ("int_bits", C.c_uint8),
                ("int_first", C.c_uint8), ("str_bits", C.c_uint8),
                ("str_first", C.c_uint8)]


class Shard(C.Structure):
    """struct qhuff_shard (include/qhuff.h): one device-resident shard"""
    _fields_ = [("in_", C.c_void_p), ("in_off", C.c_void_p),
                ("n", C.c_uint32), ("out", C.c_void_p),
                ("out_off", C.c_void_p), ("status", C.c_void_p),
                ("stream", C.c_void_p)]


class DecodeRetval(C.Structure):
    """struct qhuff_decode_retval (= struct huff_decode_retval,
    lsqpack.c:3420-3431)"""
    _fields_ = [("status", C.c_int), ("n_dst", C.c_uint), ("n_src", C.c_uint)]


class DecodeState(C.Structure):
    """struct qhuff_huff_decode_state (= struct lsqpack_huff_decode_state,
    lsqpack.h:747-757)"""
    _fields_ = [("resume", C.c_int), ("state", C.c_uint8), ("eos", C.c_uint8)]


DECODE_FULL_FN = C.CFUNCTYPE(DecodeRetval, C.c_void_p, C.c_int, C.c_void_p,
                             C.c_int, C.POINTER(DecodeState), C.c_int)


_lib = None


def lib():
    """Load libqhuff.so (built by `make -C ls-qpack_amd`)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise QhuffError("libqhuff.so not built: run make -C %s" % PKG_ROOT)
        # One HIP runtime per process: PyTorch ships its own libamdhip64
        # (NEEDED as "libamdhip64.so", soname libamdhip64.so.7).  Loaded
        # first, it satisfies libqhuff's libamdhip64.so.7 dependency; loaded
        # after libqhuff it would be a second runtime (the GPU appears twice,
        # occupancy queries and torch.cuda break).
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        vp, u32p = C.c_void_p, C.c_void_p
        L.qhuff_open.restype = C.c_int
        L.qhuff_open.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        L.qhuff_close.restype = None
        L.qhuff_close.argtypes = [vp]
        L.qhuff_encode_bound.restype = C.c_uint64
        L.qhuff_encode_bound.argtypes = [C.c_uint64, C.c_uint32, C.c_uint]
        L.qhuff_decode_bound.restype = C.c_uint64
        L.qhuff_decode_bound.argtypes = [C.c_uint64, C.c_uint32]
        L.qhuff_encode_batch.restype = C.c_int
        L.qhuff_encode_batch.argtypes = [vp, vp, u32p, C.c_uint32, C.c_uint,
                                         vp, u32p, vp]
        L.qhuff_decode_batch.restype = C.c_int
        L.qhuff_decode_batch.argtypes = [vp, vp, u32p, C.c_uint32, vp, u32p,
                                         vp, vp]
        L.qhuff_encode_batch_host.restype = C.c_int
        L.qhuff_encode_batch_host.argtypes = [vp, vp, u32p, C.c_uint32,
                                              C.c_uint, vp, u32p]
        L.qhuff_decode_batch_host.restype = C.c_int
        L.qhuff_decode_batch_host.argtypes = [vp, vp, u32p, C.c_uint32, vp,
                                              u32p, vp]
        L.qhuff_enc_enc_str.restype = C.c_int
        L.qhuff_enc_enc_str.argtypes = [vp, C.c_uint, vp, C.c_size_t,
                                        C.c_char_p, C.c_uint]
        L.qhuff_profile_read.restype = C.c_uint64
        L.qhuff_profile_read.argtypes = [vp, vp, C.c_uint64]
        L.qhuff_enc_str_size.restype = C.c_uint
        L.qhuff_enc_str_size.argtypes = [vp, C.c_char_p, C.c_uint]
        L.qhuff_huff_decode_ex.restype = DecodeRetval
        L.qhuff_huff_decode_ex.argtypes = [vp, vp, C.c_int, vp, C.c_int,
                                           C.POINTER(DecodeState), C.c_int]
        L.qhuff_huff_decode.restype = DecodeRetval
        L.qhuff_huff_decode.argtypes = [vp, vp, C.c_int, vp, C.c_int]
        L.qhuff_abi_version.restype = C.c_int
        L.qhuff_abi_version.argtypes = []
        L.qhuff_lsqpack_enc_enc_str.restype = C.c_int
        L.qhuff_lsqpack_enc_enc_str.argtypes = [C.c_uint, vp, C.c_size_t,
                                                C.c_char_p, C.c_uint]
        L.qhuff_lsqpack_huff_decode.restype = DecodeRetval
        L.qhuff_lsqpack_huff_decode.argtypes = [vp, C.c_int, vp, C.c_int,
                                                C.POINTER(DecodeState),
                                                C.c_int]
        L.qhuff_lsqpack_set_decode_full.restype = None
        L.qhuff_lsqpack_set_decode_full.argtypes = [C.c_void_p]
        L.qhuff_lsqpack_set_context.restype = C.c_int
        L.qhuff_lsqpack_set_context.argtypes = [C.c_void_p]
        L.qhuff_lsqpack_set_device.restype = C.c_int
        L.qhuff_lsqpack_set_device.argtypes = [C.c_int]
        L.qhuff_last_error.restype = C.c_char_p
        L.qhuff_last_error.argtypes = [vp]
        L.qhuff_shard_cuts.restype = C.c_int
        L.qhuff_shard_cuts.argtypes = [u32p, C.c_uint32, C.c_uint32, u32p]
        L.qhuff_device_error.restype = C.c_int
        L.qhuff_device_error.argtypes = [vp]
        L.qhuff_synth_batch.restype = C.c_uint64
        L.qhuff_synth_batch.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32,
                                        C.c_uint32, C.c_char_p, C.c_uint32,
                                        vp, u32p]
        L.qhuff_xxh32_headers.restype = C.c_int
        L.qhuff_xxh32_headers.argtypes = [vp, vp, u32p, C.c_uint32,
                                          C.c_uint32, u32p, u32p, vp]
        L.qhuff_xxh32_batch.restype = C.c_int
        L.qhuff_xxh32_batch.argtypes = [vp, vp, u32p, C.c_uint32, C.c_uint32,
                                        u32p, vp]
        L.qhuff_scan_field_section.restype = C.c_int
        L.qhuff_scan_field_section.argtypes = [C.c_char_p, C.c_size_t,
                                               C.c_uint32, vp, C.c_uint32,
                                               C.POINTER(C.c_uint32)]
        L.qhuff_scan_encoder_stream.restype = C.c_int
        L.qhuff_scan_encoder_stream.argtypes = [
            C.c_char_p, C.c_size_t, C.c_uint32, vp, C.c_uint32,
            C.POINTER(C.c_uint32), C.POINTER(C.c_size_t)]
        L.qhuff_literals_bound.restype = C.c_uint64
        L.qhuff_literals_bound.argtypes = [vp, C.c_uint32]
        L.qhuff_decode_literals_host.restype = C.c_int
        L.qhuff_decode_literals_host.argtypes = [vp, vp, vp, C.c_uint32, vp,
                                                 u32p, vp]
        L.qhuff_decode_literals_ex.restype = C.c_int
        L.qhuff_decode_literals_ex.argtypes = [vp, vp, vp, C.c_uint32,
                                               C.c_uint32, vp, u32p, vp]
        L.qhuff_xxh32_headers_host.restype = C.c_int
        L.qhuff_xxh32_headers_host.argtypes = [vp, vp, u32p, C.c_uint32,
                                               C.c_uint32, u32p, u32p]
        L.qhuff_svc_open.restype = C.c_int
        L.qhuff_svc_open.argtypes = [vp, C.c_uint, C.c_uint,
                                     C.POINTER(C.c_void_p)]
        L.qhuff_svc_close.restype = None
        L.qhuff_svc_close.argtypes = [vp]
        L.qhuff_svc_encode.restype = C.c_int
        L.qhuff_svc_encode.argtypes = [vp, vp, u32p, C.c_uint32, C.c_uint, vp,
                                       u32p]
        L.qhuff_svc_decode.restype = C.c_int
        L.qhuff_svc_decode.argtypes = [vp, vp, u32p, C.c_uint32, vp, u32p, vp]
        L.qhuff_svc_stats.restype = C.c_int
        L.qhuff_svc_stats.argtypes = [vp, C.POINTER(C.c_uint64),
                                      C.POINTER(C.c_uint64),
                                      C.POINTER(C.c_uint64)]
        L.qhuff_svc_pieces.restype = C.c_int
        L.qhuff_svc_pieces.argtypes = [u32p, C.c_uint32, u32p, C.c_uint32,
                                       C.POINTER(C.c_uint32)]
        L.qhuff_timing_enable.restype = C.c_int
        L.qhuff_timing_enable.argtypes = [vp, C.c_int]
        L.qhuff_kernel_variant.restype = C.c_int
        L.qhuff_kernel_variant.argtypes = [vp, C.c_int]
        L.qhuff_grid_waves.restype = C.c_int
        L.qhuff_grid_waves.argtypes = [vp, C.c_int]
        L.qhuff_batch_hint.restype = C.c_int
        L.qhuff_batch_hint.argtypes = [vp, C.c_int, C.c_int]
        L.qhuff_batch_needs_full.restype = C.c_int
        L.qhuff_batch_needs_full.argtypes = [u32p, C.c_uint32]
        L.qhuff_timing_read.restype = C.c_int
        L.qhuff_timing_read.argtypes = [vp, u32p, C.POINTER(C.c_double),
                                        C.c_uint32]
        L.qhuff_frame_literal.restype = C.c_int
        L.qhuff_frame_literal.argtypes = [C.c_uint, vp, C.c_size_t,
                                          C.c_char_p, C.c_uint, C.c_char_p,
                                          C.c_uint]
        L.qhuff_dec_int.restype = C.c_int
        L.qhuff_dec_int.argtypes = [C.c_char_p, C.c_size_t, C.c_uint,
                                    C.POINTER(C.c_uint64),
                                    C.POINTER(C.c_size_t)]
        L.qhuff_encode_batch_host_multi.restype = C.c_int
        L.qhuff_encode_batch_host_multi.argtypes = [vp, C.c_uint32, vp, u32p,
                                                    C.c_uint32, C.c_uint, vp,
                                                    u32p]
        L.qhuff_decode_batch_host_multi.restype = C.c_int
        L.qhuff_decode_batch_host_multi.argtypes = [vp, C.c_uint32, vp, u32p,
                                                    C.c_uint32, vp, u32p, vp]
        L.qhuff_encode_batch_multi.restype = C.c_int
        L.qhuff_encode_batch_multi.argtypes = [vp, C.c_uint32, vp, C.c_uint,
                                               vp, C.c_int]
        L.qhuff_decode_batch_multi.restype = C.c_int
        L.qhuff_decode_batch_multi.argtypes = [vp, C.c_uint32, vp, vp,
                                               C.c_int]
        L.qhuff_host_register.restype = C.c_int
        L.qhuff_host_register.argtypes = [vp, C.c_size_t]
        L.qhuff_host_unregister.restype = C.c_int
        L.qhuff_host_unregister.argtypes = [vp]
        L.qhuff_host_chunks.restype = C.c_int
        L.qhuff_host_chunks.argtypes = [C.c_int, C.c_uint, u32p, C.c_uint32,
                                        C.c_uint, u32p, C.POINTER(C.c_uint32)]
        L.qhuff_decode_stream_bound.restype = C.c_uint64
        L.qhuff_decode_stream_bound.argtypes = [C.c_uint64, C.c_uint32]
        L.qhuff_decode_stream.restype = C.c_int
        L.qhuff_decode_stream.argtypes = [vp, vp, u32p, C.c_uint32, vp, vp,
                                          vp, u32p, vp, vp]
        L.qhuff_decode_stream_host.restype = C.c_int
        L.qhuff_decode_stream_host.argtypes = [vp, vp, u32p, C.c_uint32, vp,
                                               vp, vp, u32p, vp]
        L.qhuff_literals_check.restype = C.c_int
        L.qhuff_literals_check.argtypes = [vp, C.c_uint32,
                                           C.POINTER(C.c_uint32)]
        L.qhuff_decode_wire.restype = C.c_int
        L.qhuff_decode_wire.argtypes = [vp, vp, vp, C.c_uint32, C.c_uint32,
                                        vp, u32p, vp, vp]
        L.qhuff_decode_wire_host.restype = C.c_int
        L.qhuff_decode_wire_host.argtypes = [vp, vp, vp, C.c_uint32,
                                             C.c_uint32, vp, u32p, vp]
        L.qhuff_encode_wire_bound.restype = C.c_uint64
        L.qhuff_encode_wire_bound.argtypes = [C.c_uint64, C.c_uint32]
        L.qhuff_items_check.restype = C.c_int
        L.qhuff_items_check.argtypes = [vp, C.c_uint32, C.POINTER(C.c_uint32)]
        L.qhuff_encode_wire.restype = C.c_int
        L.qhuff_encode_wire.argtypes = [vp, vp, u32p, vp, C.c_uint32, vp,
                                        u32p, vp]
        L.qhuff_encode_wire_host.restype = C.c_int
        L.qhuff_encode_wire_host.argtypes = [vp, vp, u32p, vp, C.c_uint32, vp,
                                             u32p]
        i32p = C.c_void_p
        L.qhuff_scan_sections.restype = C.c_int
        L.qhuff_scan_sections.argtypes = [vp, vp, vp, C.c_uint32, C.c_uint,
                                          vp, C.c_uint32, vp, vp, vp, vp]
        L.qhuff_scan_sections_host.restype = C.c_int
        L.qhuff_scan_sections_host.argtypes = [vp, vp, u32p, C.c_uint32,
                                               C.c_uint, vp, C.c_uint32, u32p,
                                               i32p, u32p]
        L.qhuff_decode_sections_host.restype = C.c_int
        L.qhuff_decode_sections_host.argtypes = [vp, vp, u32p, C.c_uint32,
                                                 C.c_uint, C.c_uint32, vp,
                                                 C.c_uint32, u32p, i32p, u32p,
                                                 vp, u32p, vp]
        L.qhuff_scan_sections_cpu.restype = C.c_int
        L.qhuff_scan_sections_cpu.argtypes = [vp, u32p, C.c_uint32, C.c_uint,
                                              vp, C.c_uint32, u32p, i32p, u32p]
        L.qhuff_static_lookup.restype = C.c_int
        L.qhuff_static_lookup.argtypes = [vp, vp, u32p, C.c_uint32, u32p, u32p,
                                          vp, vp, vp]
        L.qhuff_static_lookup_host.restype = C.c_int
        L.qhuff_static_lookup_host.argtypes = [vp, vp, u32p, C.c_uint32, u32p,
                                               u32p, vp, vp]
        L.qhuff_static_lookup_cpu.restype = C.c_int
        L.qhuff_static_lookup_cpu.argtypes = [vp, u32p, C.c_uint32, u32p, u32p,
                                              vp, vp]
        L.qhuff_static_probe_tables.restype = C.c_int
        L.qhuff_static_probe_tables.argtypes = [vp, vp]
        L.qhuff_encode_headers_bound.restype = C.c_uint64
        L.qhuff_encode_headers_bound.argtypes = [C.c_uint64, C.c_uint32,
                                                 C.c_uint32]
        L.qhuff_encode_headers.restype = C.c_int
        L.qhuff_encode_headers.argtypes = [vp, vp, u32p, C.c_uint32, vp, u32p,
                                           C.c_uint32, vp, u32p, vp, vp, vp]
        L.qhuff_encode_headers_host.restype = C.c_int
        L.qhuff_encode_headers_host.argtypes = [vp, vp, u32p, C.c_uint32, vp,
                                                u32p, C.c_uint32, vp, u32p, vp,
                                                vp]
        L.qhuff_scan_headers.restype = C.c_int
        L.qhuff_scan_headers.argtypes = [vp, vp, vp, C.c_uint32, vp,
                                         C.c_uint32, vp, vp, vp, vp, vp, vp]
        L.qhuff_scan_headers_host.restype = C.c_int
        L.qhuff_scan_headers_host.argtypes = [vp, vp, u32p, C.c_uint32, vp,
                                              C.c_uint32, u32p, i32p, vp, vp,
                                              vp]
        L.qhuff_scan_headers_cpu.restype = C.c_int
        L.qhuff_scan_headers_cpu.argtypes = [vp, u32p, C.c_uint32, vp,
                                             C.c_uint32, u32p, i32p, vp, vp,
                                             vp]
        L.qhuff_decode_headers_bound.restype = C.c_uint64
        L.qhuff_decode_headers_bound.argtypes = [C.c_uint64, C.c_uint32]
        L.qhuff_decode_headers.restype = C.c_int
        L.qhuff_decode_headers.argtypes = [vp, vp, vp, C.c_uint32, C.c_uint32,
                                           vp, u32p, vp, vp]
        dtp = C.POINTER(DynTable)
        L.qhuff_scan_headers_dyn.restype = C.c_int
        L.qhuff_scan_headers_dyn.argtypes = [vp, vp, vp, C.c_uint32, dtp, vp,
                                             vp, C.c_uint32, vp, vp, vp, vp,
                                             vp, vp, vp]
        L.qhuff_scan_headers_dyn_host.restype = C.c_int
        L.qhuff_scan_headers_dyn_host.argtypes = [vp, vp, u32p, C.c_uint32,
                                                  dtp, vp, vp, C.c_uint32, vp,
                                                  vp, vp, vp, vp, vp]
        L.qhuff_scan_headers_dyn_cpu.restype = C.c_int
        L.qhuff_scan_headers_dyn_cpu.argtypes = [vp, u32p, C.c_uint32, dtp,
                                                 vp, vp, C.c_uint32, vp, vp,
                                                 vp, vp, vp, vp]
        L.qhuff_decode_headers_dyn_bound.restype = C.c_uint64
        L.qhuff_decode_headers_dyn_bound.argtypes = [C.c_uint64, C.c_uint32,
                                                     C.c_uint32]
        L.qhuff_decode_headers_dyn.restype = C.c_int
        L.qhuff_decode_headers_dyn.argtypes = [vp, vp, vp, C.c_uint32,
                                               C.c_uint32, vp, C.c_uint32,
                                               vp, vp, vp, vp]
        L.qhuff_decode_headers_dyn_host.restype = C.c_int
        L.qhuff_decode_headers_dyn_host.argtypes = [vp, vp, u32p, C.c_uint32,
                                                    dtp, vp, C.c_uint32,
                                                    C.c_uint32, vp, vp, vp,
                                                    vp, vp, vp, vp, vp, vp,
                                                    vp, vp]
        L.qhuff_dyn_lookup.restype = C.c_int
        L.qhuff_dyn_lookup.argtypes = [vp, vp, vp, C.c_uint32, dtp, C.c_uint32,
                                       C.c_uint32, vp, vp, vp, vp, vp, vp]
        L.qhuff_dyn_lookup_host.restype = C.c_int
        L.qhuff_dyn_lookup_host.argtypes = [vp, vp, vp, C.c_uint32, dtp,
                                            C.c_uint32, C.c_uint32, vp, vp,
                                            vp, vp, vp]
        L.qhuff_dyn_lookup_cpu.restype = C.c_int
        L.qhuff_dyn_lookup_cpu.argtypes = [vp, vp, C.c_uint32, dtp,
                                           C.c_uint32, C.c_uint32, vp, vp, vp,
                                           vp, vp]
        L.qhuff_dyn_index_slots.restype = C.c_uint32
        L.qhuff_dyn_index_slots.argtypes = [C.c_uint32]
        L.qhuff_encode_headers_dyn_bound.restype = C.c_uint64
        L.qhuff_encode_headers_dyn_bound.argtypes = [C.c_uint64, C.c_uint32,
                                                     C.c_uint32]
        L.qhuff_encode_headers_dyn.restype = C.c_int
        L.qhuff_encode_headers_dyn.argtypes = [vp, vp, vp, C.c_uint32, vp, vp,
                                               C.c_uint32, dtp, vp, vp, vp,
                                               vp, vp, vp, vp, vp]
        L.qhuff_encode_headers_dyn_host.restype = C.c_int
        L.qhuff_encode_headers_dyn_host.argtypes = [vp, vp, vp, C.c_uint32,
                                                    vp, vp, C.c_uint32, dtp,
                                                    vp, vp, vp, vp, vp, vp,
                                                    vp]
        # (the _dyn calls' lists with `tabs, sec_tab` where `tab` stands)
        tsp = C.POINTER(DynTables)
        u32 = C.c_uint32
        L.qhuff_scan_headers_tabs.restype = C.c_int
        L.qhuff_scan_headers_tabs.argtypes = [vp, vp, vp, u32, tsp, vp, vp,
                                              vp, u32] + [vp] * 7
        L.qhuff_scan_headers_tabs_host.restype = C.c_int
        L.qhuff_scan_headers_tabs_host.argtypes = [vp, vp, u32p, u32, tsp, vp,
                                                   vp, vp, u32] + [vp] * 6
        L.qhuff_scan_headers_tabs_cpu.restype = C.c_int
        L.qhuff_scan_headers_tabs_cpu.argtypes = [vp, u32p, u32, tsp, vp, vp,
                                                  vp, u32] + [vp] * 6
        L.qhuff_decode_headers_tabs_host.restype = C.c_int
        L.qhuff_decode_headers_tabs_host.argtypes = [vp, vp, u32p, u32, tsp,
                                                     vp, vp, u32, u32] \
            + [vp] * 11
        L.qhuff_dyn_lookup_tabs.restype = C.c_int
        L.qhuff_dyn_lookup_tabs.argtypes = [vp, vp, vp, u32, vp, u32, tsp] \
            + [vp] * 8
        L.qhuff_dyn_lookup_tabs_host.restype = C.c_int
        L.qhuff_dyn_lookup_tabs_host.argtypes = [vp, vp, vp, u32, vp, u32,
                                                 tsp] + [vp] * 7
        L.qhuff_dyn_lookup_tabs_cpu.restype = C.c_int
        L.qhuff_dyn_lookup_tabs_cpu.argtypes = [vp, vp, u32, vp, u32, tsp] \
            + [vp] * 7
        L.qhuff_dyn_tables_index_slots.restype = C.c_uint32
        L.qhuff_dyn_tables_index_slots.argtypes = [u32]
        L.qhuff_encode_headers_tabs.restype = C.c_int
        L.qhuff_encode_headers_tabs.argtypes = [vp, vp, vp, u32, vp, vp, u32,
                                                tsp] + [vp] * 9
        L.qhuff_encode_headers_tabs_host.restype = C.c_int
        L.qhuff_encode_headers_tabs_host.argtypes = [vp, vp, vp, u32, vp, vp,
                                                     u32, tsp] + [vp] * 8
        # (encoder-stream inserts applied to a set of tables)
        isp, icp, iop = (C.POINTER(InsState), C.POINTER(InsScan),
                         C.POINTER(InsOut))
        L.qhuff_tabs_insert_bound.restype = C.c_uint64
        L.qhuff_tabs_insert_bound.argtypes = [C.c_uint64, C.c_uint64, u32, u32]
        L.qhuff_scan_inserts_tabs.restype = C.c_int
        L.qhuff_scan_inserts_tabs.argtypes = [vp, tsp, isp, vp, vp, icp, vp]
        L.qhuff_apply_inserts_tabs.restype = C.c_int
        L.qhuff_apply_inserts_tabs.argtypes = [vp, tsp, isp, vp, u32, vp, icp,
                                               u32, iop, vp]
        L.qhuff_tabs_insert_host.restype = C.c_int
        L.qhuff_tabs_insert_host.argtypes = [vp, tsp, isp, vp, vp, vp, icp,
                                             iop]
        L.qhuff_tabs_insert_cpu.restype = C.c_int
        L.qhuff_tabs_insert_cpu.argtypes = [tsp, isp, vp, vp, vp, icp, iop]
        L.qhuff_decode_headers_host.restype = C.c_int
        L.qhuff_decode_headers_host.argtypes = [vp, vp, u32p, C.c_uint32,
                                                C.c_uint32, C.c_uint32, u32p,
                                                i32p, vp, vp, vp, vp, u32p, vp,
                                                u32p, u32p]
        _lib = L
    return _lib


# ---- host-only helpers (no device needed) ---------------------------------

def encode_bound(in_bytes, n, mode=ENC_PAYLOAD):
    return int(lib().qhuff_encode_bound(in_bytes, n, mode))


def decode_bound(in_bytes, n):
    return int(lib().qhuff_decode_bound(in_bytes, n))


def decode_stream_bound(in_bytes, n):
    return int(lib().qhuff_decode_stream_bound(in_bytes, n))


def _np_ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def shard_cuts(in_off, g):
    """Byte-balanced contiguous partition into g shards -> g+1 string
    indices (include/qhuff.h qhuff_shard_cuts)."""
    import numpy as np
    in_off = np.ascontiguousarray(in_off, dtype=np.uint32)
    cuts = np.zeros(g + 1, dtype=np.uint32)
    rc = lib().qhuff_shard_cuts(_np_ptr(in_off), len(in_off) - 1, g,
                                _np_ptr(cuts))
    if rc:
        raise QhuffError("qhuff_shard_cuts: %d" % rc)
    return cuts


def svc_pieces(in_off, max_pieces=None):
    """qhuff_svc_pieces: the string indices at which a service call of these
    offsets is cut into pieces, [0, ..., n] -- [0] for a call that would run
    the context's host path (or has no strings)."""
    import numpy as np
    in_off = np.ascontiguousarray(in_off, dtype=np.uint32)
    n = len(in_off) - 1
    if max_pieces is None:
        max_pieces = max(n, 1)
    cuts = np.zeros(max_pieces + 1, dtype=np.uint32)
    k = C.c_uint32()
    rc = lib().qhuff_svc_pieces(_np_ptr(in_off), n, _np_ptr(cuts), max_pieces,
                                C.byref(k))
    if rc:
        raise QhuffError("qhuff_svc_pieces: %d (%d pieces)" % (rc, k.value))
    return [int(x) for x in cuts[:k.value + 1]]


def host_chunks(in_off, enc=True, mode=ENC_PAYLOAD, chunk_shift=0):
    """qhuff_host_chunks: (cut, small) -- the K + 1 string indices at which
    the host-memory calls cut a batch of these offsets into chunks, and
    whether the call takes the one-synchronisation path.  chunk_shift 0: the
    process's own (QHUFF_HOST_CHUNK_SHIFT)."""
    import numpy as np
    in_off = np.ascontiguousarray(in_off, dtype=np.uint32)
    cut = np.zeros(17, dtype=np.uint32)
    small = C.c_uint32()
    k = lib().qhuff_host_chunks(int(bool(enc)), mode if enc else 0,
                                _np_ptr(in_off), len(in_off) - 1, chunk_shift,
                                _np_ptr(cut), C.byref(small))
    if k < 1:
        raise QhuffError("qhuff_host_chunks: %d" % k)
    return [int(x) for x in cut[:k + 1]], bool(small.value)


def batch_needs_full(in_off):
    """qhuff_batch_needs_full: 1 if host offsets describe a batch the full
    kernel is for (a string > 128 bytes or a tile past the 3 KB stage)."""
    import numpy as np
    in_off = np.ascontiguousarray(in_off, dtype=np.uint32)
    return int(lib().qhuff_batch_needs_full(_np_ptr(in_off), len(in_off) - 1))


def _scan(fn, buf, pos_base, *extra):
    cap = 64
    while True:
        lits = (Literal * cap)()
        n = C.c_uint32()
        rc = fn(buf, len(buf), pos_base, lits, cap, C.byref(n), *extra)
        if rc == ERANGE:
            cap = max(2 * cap, n.value)
            continue
        return rc, list(lits[:n.value])


def scan_field_section(buf, pos_base=0):
    """Literals of one encoded field section -> (rc, [Literal])."""
    return _scan(lib().qhuff_scan_field_section, bytes(buf), pos_base)


def scan_encoder_stream(buf, pos_base=0):
    """Literals of the complete encoder-stream instructions in buf ->
    (rc, [Literal], consumed bytes)."""
    consumed = C.c_size_t()
    rc, lits = _scan(lib().qhuff_scan_encoder_stream, bytes(buf), pos_base,
                     C.byref(consumed))
    return rc, lits, consumed.value


def _sections_host_args(buf, sec_off, max_lits):
    """the host forms' arrays: (buf, sec_off, m, max_lits, lits, lit_off, rc,
    consumed)"""
    import numpy as np
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    sec_off = np.ascontiguousarray(sec_off, dtype=np.uint32)
    m = len(sec_off) - 1
    return (buf, sec_off, m, max_lits,
            np.zeros(16 * max(max_lits, 1), dtype=np.uint8),
            np.zeros(m + 1, dtype=np.uint32), np.zeros(max(m, 1), dtype=np.int32),
            np.zeros(max(m, 1), dtype=np.uint32))


def scan_sections_cpu(buf, sec_off, mode=SCAN_FIELD_SECTION, max_lits=None):
    """qhuff_scan_sections_cpu: the device scan's walker run on the host over
    chunks buf[sec_off[i] : sec_off[i + 1]] -> (ret, lits, lit_off, rc,
    consumed): ret OK or ERANGE (lit_off[-1] > max_lits), lits the uint8
    array of the min(lit_off[-1], max_lits) descriptors written.  max_lits
    None: a first call with room for none counts them."""
    if max_lits is None:
        max_lits = int(scan_sections_cpu(buf, sec_off, mode, 0)[2][-1])
    buf, sec_off, m, max_lits, lits, lit_off, rc, consumed = \
        _sections_host_args(buf, sec_off, max_lits)
    ret = lib().qhuff_scan_sections_cpu(
        _np_ptr(buf) if len(buf) else None, _np_ptr(sec_off), m, mode,
        _np_ptr(lits), max_lits, _np_ptr(lit_off), _np_ptr(rc),
        _np_ptr(consumed))
    if ret not in (OK, ERANGE):
        raise QhuffError("qhuff_scan_sections_cpu failed: %d" % ret)
    n = min(int(lit_off[-1]), max_lits)
    return ret, lits[:16 * n], lit_off, rc[:m], consumed[:m]


def decode_headers_bound(wire_bytes, n):
    return int(lib().qhuff_decode_headers_bound(wire_bytes, n))


def _headers_host_args(buf, sec_off, max_hdrs):
    """the header scans' host arrays: (buf, sec_off, m, strs, hdr_off, rc,
    kind, static_id, hflags)"""
    import numpy as np
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    sec_off = np.ascontiguousarray(sec_off, dtype=np.uint32)
    m = len(sec_off) - 1
    k = max(max_hdrs, 1)
    return (buf, sec_off, m, np.zeros(32 * k, dtype=np.uint8),
            np.zeros(m + 1, dtype=np.uint32), np.zeros(max(m, 1), dtype=np.int32),
            np.zeros(k, dtype=np.uint8), np.zeros(k, dtype=np.uint8),
            np.zeros(k, dtype=np.uint8))


def scan_headers_cpu(buf, sec_off, max_hdrs=None):
    """qhuff_scan_headers_cpu: the header scan's walker run on the host over
    sections buf[sec_off[i] : sec_off[i + 1]] -> (ret, strs, hdr_off, rc,
    kind, static_id, hflags): ret OK or ERANGE (hdr_off[-1] > max_hdrs), strs
    the uint8 array of the 2 * min(hdr_off[-1], max_hdrs) descriptors written
    (16 bytes each).  max_hdrs None: a first call with room for none counts
    them."""
    if max_hdrs is None:
        max_hdrs = int(scan_headers_cpu(buf, sec_off, 0)[2][-1])
    buf, sec_off, m, strs, hdr_off, rc, kind, sid, hf = \
        _headers_host_args(buf, sec_off, max_hdrs)
    ret = lib().qhuff_scan_headers_cpu(
        _np_ptr(buf) if len(buf) else None, _np_ptr(sec_off), m,
        _np_ptr(strs), max_hdrs, _np_ptr(hdr_off), _np_ptr(rc), _np_ptr(kind),
        _np_ptr(sid), _np_ptr(hf))
    if ret not in (OK, ERANGE):
        raise QhuffError("qhuff_scan_headers_cpu failed: %d" % ret)
    n = min(int(hdr_off[-1]), max_hdrs)
    return ret, strs[:32 * n], hdr_off, rc[:m], kind[:n], sid[:n], hf[:n]


class DynTable(C.Structure):
    """struct qhuff_dyn_table"""
    _fields_ = [("bytes", C.c_void_p), ("off", C.c_void_p), ("d", C.c_uint32),
                ("first", C.c_uint32), ("max_entries", C.c_uint32)]


def decode_headers_dyn_bound(wire_bytes, n, dyn_longest):
    return int(lib().qhuff_decode_headers_dyn_bound(wire_bytes, n,
                                                    dyn_longest))


def dyn_table_host(data, off, first=0, max_entries=0):
    """The dynamic table's entries as host arrays -> (DynTable, the arrays it
    points to): data the packed names and values, off uint32 [2d + 1] (None
    or one entry: d = 0), entry k the absolute index first + k."""
    import numpy as np
    off = np.zeros(1, np.uint32) if off is None else \
        np.ascontiguousarray(off, dtype=np.uint32)
    d = (len(off) - 1) // 2
    data = np.ascontiguousarray(data if data is not None else [],
                                dtype=np.uint8)
    if not len(data):
        data = np.zeros(1, dtype=np.uint8)   # (d entries, all empty)
    t = DynTable(_np_ptr(data) if d else None,
                 _np_ptr(off) if d else None, d, first, max_entries)
    return t, (data, off)


def _sec_win_host(sec_win):
    import numpy as np
    return None if sec_win is None else \
        np.ascontiguousarray(sec_win, dtype=np.uint32).reshape(-1)


def scan_headers_dyn_cpu(buf, sec_off, table, sec_win=None, max_hdrs=None):
    """qhuff_scan_headers_dyn_cpu: scan_headers_cpu against the dynamic
    table's entries.  table: (data, off, first, max_entries) host arrays as
    dyn_table_host takes them; sec_win: uint32 [2m] or None -> (ret, strs,
    hdr_off, rc, kind, static_id, hflags, dyn_id); ret OK, ERANGE, or EINVAL /
    ERANGE of the argument checks (the arrays then as they were made)."""
    import numpy as np
    if max_hdrs is None:
        max_hdrs = int(scan_headers_dyn_cpu(buf, sec_off, table, sec_win,
                                            0)[2][-1])
    buf, sec_off, m, strs, hdr_off, rc, kind, sid, hf = \
        _headers_host_args(buf, sec_off, max_hdrs)
    did = np.zeros(max(max_hdrs, 1), dtype=np.uint32)
    t, keep = dyn_table_host(*table)
    win = _sec_win_host(sec_win)
    ret = lib().qhuff_scan_headers_dyn_cpu(
        _np_ptr(buf) if len(buf) else None, _np_ptr(sec_off), m, C.byref(t),
        _np_ptr(win) if win is not None else None, _np_ptr(strs), max_hdrs,
        _np_ptr(hdr_off), _np_ptr(rc), _np_ptr(kind), _np_ptr(sid),
        _np_ptr(hf), _np_ptr(did))
    del keep
    n = min(int(hdr_off[-1]), max_hdrs)
    return (ret, strs[:32 * n], hdr_off, rc[:m], kind[:n], sid[:n], hf[:n],
            did[:n])


class DynTables(C.Structure):
    """struct qhuff_dyn_tables"""
    _fields_ = [("bytes", C.c_void_p), ("off", C.c_void_p),
                ("ent", C.c_void_p), ("first", C.c_void_p),
                ("max_entries", C.c_void_p), ("T", C.c_uint32)]


def dyn_tables_host(data=None, off=None, ent=None, first=None,
                    max_entries=None):
    """A set of T dynamic tables as host arrays -> (DynTables, the arrays it
    points to): data / off the packed entries of all tables (off uint32 [2D +
    1]), ent uint32 [T + 1] the tables' bounds in entry ordinals, first and
    max_entries uint32 [T].  ent None: T = 0, every pointer null.  The arrays
    are passed as they are (the checks are the library's)."""
    import numpy as np
    if ent is None:
        return DynTables(None, None, None, None, None, 0), ()
    u32 = lambda a: np.ascontiguousarray(a, dtype=np.uint32)  # noqa: E731
    ent, first, max_entries = u32(ent), u32(first), u32(max_entries)
    off = np.zeros(1, np.uint32) if off is None else u32(off)
    data = np.ascontiguousarray(data if data is not None else [],
                                dtype=np.uint8)
    if not len(data):
        data = np.zeros(1, dtype=np.uint8)
    t = DynTables(_np_ptr(data), _np_ptr(off), _np_ptr(ent), _np_ptr(first),
                  _np_ptr(max_entries), len(first))
    return t, (data, off, ent, first, max_entries)


def _tabs_longest(tables):
    """the longest name + value of a set's entries"""
    off = tables[1] if len(tables) > 1 else None
    if off is None or len(off) < 3:
        return 0
    import numpy as np
    off = np.asarray(off, dtype=np.int64)
    return max(int((off[2::2] - off[:-2:2]).max()), 0)


def _opt_u32(a):
    import numpy as np
    return None if a is None else \
        np.ascontiguousarray(a, dtype=np.uint32).reshape(-1)


def _opt_ptr(a):
    return _np_ptr(a) if a is not None and len(a) else None


def dyn_tables_index_slots(D):
    """qhuff_dyn_tables_index_slots: the slots of each of the two indices a
    lookup over a set of tables builds over its D entries."""
    return int(lib().qhuff_dyn_tables_index_slots(D))


def scan_headers_tabs_cpu(buf, sec_off, tables, sec_tab, sec_win=None,
                          max_hdrs=None):
    """qhuff_scan_headers_tabs_cpu: scan_headers_dyn_cpu with a table per
    section.  tables: (data, off, ent, first, max_entries) as dyn_tables_host
    takes them (() or None: T = 0); sec_tab uint32 [m] -> as
    scan_headers_dyn_cpu."""
    import numpy as np
    if max_hdrs is None:
        max_hdrs = int(scan_headers_tabs_cpu(buf, sec_off, tables, sec_tab,
                                             sec_win, 0)[2][-1])
    buf, sec_off, m, strs, hdr_off, rc, kind, sid, hf = \
        _headers_host_args(buf, sec_off, max_hdrs)
    did = np.zeros(max(max_hdrs, 1), dtype=np.uint32)
    t, keep = dyn_tables_host(*(tables or ()))
    tab, win = _opt_u32(sec_tab), _sec_win_host(sec_win)
    ret = lib().qhuff_scan_headers_tabs_cpu(
        _np_ptr(buf) if len(buf) else None, _np_ptr(sec_off), m, C.byref(t),
        _opt_ptr(tab), _np_ptr(win) if win is not None else None,
        _np_ptr(strs), max_hdrs, _np_ptr(hdr_off), _np_ptr(rc), _np_ptr(kind),
        _np_ptr(sid), _np_ptr(hf), _np_ptr(did))
    del keep
    n = min(int(hdr_off[-1]), max_hdrs)
    return (ret, strs[:32 * n], hdr_off, rc[:m], kind[:n], sid[:n], hf[:n],
            did[:n])


def dyn_lookup_tabs_cpu(data, off, sec_hdr, tables, sec_tab, sec_win=None):
    """qhuff_dyn_lookup_tabs_cpu: the lookup kernel's source run on the host,
    header j of section s (sec_hdr uint32 [m + 1]) in table sec_tab[s] within
    sec_win[2s .. 2s + 1] (None: the whole of that table) -> (ret, name_hash,
    nameval_hash uint32 [n], kind, static_id uint8 [n], dyn_id uint32 [n])."""
    import numpy as np
    data = np.ascontiguousarray(data, dtype=np.uint8)
    off = np.ascontiguousarray(off, dtype=np.uint32)
    sec_hdr = np.ascontiguousarray(sec_hdr, dtype=np.uint32)
    n, m = (len(off) - 1) // 2, len(sec_hdr) - 1
    h1, h2, did = (np.zeros(max(n, 1), dtype=np.uint32) for _ in range(3))
    kind, sid = (np.zeros(max(n, 1), dtype=np.uint8) for _ in range(2))
    t, keep = dyn_tables_host(*(tables or ()))
    tab, win = _opt_u32(sec_tab), _sec_win_host(sec_win)
    ret = lib().qhuff_dyn_lookup_tabs_cpu(
        _np_ptr(data) if len(data) else _np_ptr(np.zeros(1, np.uint8)),
        _np_ptr(off), n, _np_ptr(sec_hdr), m, C.byref(t), _opt_ptr(tab),
        _opt_ptr(win), _np_ptr(h1), _np_ptr(h2), _np_ptr(kind), _np_ptr(sid),
        _np_ptr(did))
    del keep
    return ret, h1[:n], h2[:n], kind[:n], sid[:n], did[:n]


# ---- encoder-stream inserts applied to a set of tables -----------------------

class InsState(C.Structure):
    """struct qhuff_ins_state"""
    _fields_ = [("cap", C.c_void_p), ("max_cap", C.c_void_p),
                ("live_lo", C.c_void_p), ("arena_bytes", C.c_uint32),
                ("dyn_longest", C.c_uint32)]


class InsScan(C.Structure):
    """struct qhuff_ins_scan"""
    _fields_ = [("rc", C.c_void_p), ("consumed", C.c_void_p),
                ("ins_off", C.c_void_p), ("chunk_cap", C.c_void_p),
                ("strs", C.c_void_p), ("root", C.c_void_p),
                ("ins_cap", C.c_void_p), ("ins_ref", C.c_void_p),
                ("ins_kind", C.c_void_p), ("max_ins", C.c_uint32)]


class InsOut(C.Structure):
    """struct qhuff_ins_out"""
    _fields_ = [("ins_lo", C.c_void_p), ("out_bytes", C.c_void_p),
                ("out_off", C.c_void_p), ("out_ent", C.c_void_p),
                ("out_first", C.c_void_p), ("cap_out", C.c_void_p),
                ("live_lo_out", C.c_void_p), ("out_cap", C.c_uint64),
                ("ent_cap", C.c_uint32)]


def tabs_insert_bound(arena_bytes, wire_bytes, max_ins, dyn_longest):
    return int(lib().qhuff_tabs_insert_bound(arena_bytes, wire_bytes, max_ins,
                                             dyn_longest))


class Inserted:
    """What an insert call gives: ret; per chunk rc, consumed, ins_off,
    chunk_cap; per insert ins_kind, ins_ref, ins_lo, strs (the descriptors'
    bytes), root, ins_cap; the next set as `tables` = (data, off, ent, first,
    max_entries), the tuple the _tabs calls take, with cap and live_lo.  On
    QHUFF_EINVAL nothing but ret is set; on QHUFF_ERANGE the next set is
    None."""
    tables = cap = live_lo = None


def _tabs_insert(fn, ctx, what, tables, cap, max_cap, live_lo, buf, enc_off,
                 keep, max_ins):
    import numpy as np
    u32 = lambda a: np.ascontiguousarray(a, dtype=np.uint32).reshape(-1)  # noqa: E731
    cap, max_cap, live_lo = u32(cap), u32(max_cap), u32(live_lo)
    enc_off = u32(enc_off)
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    t, keep_t = dyn_tables_host(*(tables or ()))
    T = t.T
    D = int(keep_t[2][-1]) if T else 0
    if max_ins is None:
        max_ins = int(_tabs_insert(fn, ctx, what, tables, cap, max_cap,
                                   live_lo, buf, enc_off, keep,
                                   0).ins_off[-1])
    k = max(max_ins, 1)
    r = Inserted()
    r.rc = np.zeros(max(T, 1), dtype=np.int32)
    r.consumed, r.out_first, r.cap, r.live_lo = (
        np.zeros(max(T, 1), dtype=np.uint32) for _ in range(4))
    r.ins_off, out_ent = (np.zeros(T + 1, dtype=np.uint32) for _ in range(2))
    r.chunk_cap = np.zeros(max(2 * T, 1), dtype=np.uint32)
    r.strs = np.zeros(32 * k, dtype=np.uint8)
    r.root, r.ins_cap = (np.zeros(2 * k, dtype=np.uint32) for _ in range(2))
    r.ins_ref, r.ins_lo = (np.zeros(k, dtype=np.uint32) for _ in range(2))
    r.ins_kind = np.zeros(k, dtype=np.uint8)
    wire = max(int(enc_off[-1]) - int(enc_off[0]), 0) if T else 0
    arena = int(keep_t[1][2 * D]) if D else 0
    bound = tabs_insert_bound(arena, wire, max_ins,
                              _tabs_longest(tables or ()))
    out = np.full(min(bound, 1 << 32), 0xA5, dtype=np.uint8)
    out_off = np.zeros(2 * (D + max_ins) + 1, dtype=np.uint32)
    kp = _opt_u32(keep)
    st = InsState(_np_ptr(cap), _np_ptr(max_cap), _np_ptr(live_lo), 0, 0)
    sc = InsScan(_np_ptr(r.rc), _np_ptr(r.consumed), _np_ptr(r.ins_off),
                 _np_ptr(r.chunk_cap), _np_ptr(r.strs), _np_ptr(r.root),
                 _np_ptr(r.ins_cap), _np_ptr(r.ins_ref), _np_ptr(r.ins_kind),
                 max_ins)
    o = InsOut(_np_ptr(r.ins_lo), _np_ptr(out), _np_ptr(out_off),
               _np_ptr(out_ent), _np_ptr(r.out_first), _np_ptr(r.cap),
               _np_ptr(r.live_lo), len(out), D + max_ins)
    r.ret = fn(*ctx, C.byref(t), C.byref(st),
               _np_ptr(buf) if len(buf) else None, _np_ptr(enc_off),
               _opt_ptr(kp), C.byref(sc), C.byref(o))
    r.out_raw = out
    if r.ret == EINVAL:
        return r
    n = min(int(r.ins_off[-1]), max_ins)
    r.rc, r.consumed = r.rc[:T], r.consumed[:T]
    r.chunk_cap = r.chunk_cap[:2 * T]
    r.strs, r.root, r.ins_cap = r.strs[:32 * n], r.root[:2 * n], \
        r.ins_cap[:2 * n]
    r.ins_ref, r.ins_kind, r.ins_lo = r.ins_ref[:n], r.ins_kind[:n], \
        r.ins_lo[:n]
    if r.ret == ERANGE:
        r.ins_lo = r.cap = r.live_lo = None
        return r
    if r.ret != OK:
        raise QhuffError("%s failed: %d" % (what, r.ret))
    r.cap, r.live_lo, r.out_first = r.cap[:T], r.live_lo[:T], r.out_first[:T]
    De = int(out_ent[-1])
    off = out_off[:2 * De + 1]
    r.tables = ((out[:off[-1]], off, out_ent, r.out_first,
                 u32(tables[4])) if T else ())
    return r


def tabs_insert_cpu(tables, cap, max_cap, live_lo, buf, enc_off, keep=None,
                    max_ins=None):
    """qhuff_tabs_insert_cpu: chunk c of buf (enc_off uint32 [T + 1]) applied
    to table c of `tables` = (data, off, ent, first, max_entries) in the state
    cap / max_cap / live_lo uint32 [T]; keep uint32 [T] or None -> Inserted.
    max_ins None: the call is made twice, first with max_ins = 0 for the count
    (the host form then uploads twice: pass max_ins where that matters).
    r.out_raw is the whole out_bytes buffer, preset to 0xA5."""
    return _tabs_insert(lib().qhuff_tabs_insert_cpu, (), "qhuff_tabs_insert_cpu",
                        tables, cap, max_cap, live_lo, buf, enc_off, keep,
                        max_ins)


def hstrs_array(strs):
    """[Hstr] -> the descriptors as qhuff_decode_headers reads them: a numpy
    uint8 array of 16 bytes each (two a header)."""
    import numpy as np
    n = len(strs)
    arr = (Hstr * max(n, 1))(*strs)
    return np.frombuffer(bytes(arr), dtype=np.uint8)[:16 * n].copy()


def literals_array(lits):
    """[Literal] -> the descriptors as qhuff_decode_wire reads them: a numpy
    uint8 array of 16 * n bytes (torch.from_numpy(...).cuda() for the device
    call)."""
    import numpy as np
    n = len(lits)
    arr = (Literal * max(n, 1))(*lits)
    return np.frombuffer(bytes(arr), dtype=np.uint8)[:16 * n].copy()


def literals_check(lits):
    """qhuff_literals_check: the order rule of decode_wire over [Literal] (or
    their uint8 array) -> (rc, first offending index or None)."""
    import numpy as np
    a = lits if isinstance(lits, np.ndarray) else literals_array(lits)
    a = np.ascontiguousarray(a, dtype=np.uint8)
    bad = C.c_uint32(0xffffffff)
    rc = lib().qhuff_literals_check(_np_ptr(a) if len(a) else None,
                                    len(a) // 16, C.byref(bad))
    return rc, (bad.value if rc != OK else None)


def literals_bound(lits):
    """qhuff_literals_bound over [Literal] or their uint8 array"""
    import numpy as np
    a = lits if isinstance(lits, np.ndarray) else literals_array(lits)
    a = np.ascontiguousarray(a, dtype=np.uint8)
    return int(lib().qhuff_literals_bound(_np_ptr(a) if len(a) else None,
                                          len(a) // 16))


def encode_wire_bound(in_bytes, n):
    return int(lib().qhuff_encode_wire_bound(in_bytes, n))


def items_array(items):
    """[Item] -> the items as qhuff_encode_wire reads them: a numpy uint8
    array of 8 * n bytes (torch.from_numpy(...).cuda() for the device
    call)."""
    import numpy as np
    n = len(items)
    arr = (Item * max(n, 1))(*items)
    return np.frombuffer(bytes(arr), dtype=np.uint8)[:8 * n].copy()


def items_check(items):
    """qhuff_items_check: the item rule of encode_wire over [Item] (or their
    uint8 array) -> (rc, first offending index or None)."""
    import numpy as np
    a = items if isinstance(items, np.ndarray) else items_array(items)
    a = np.ascontiguousarray(a, dtype=np.uint8)
    bad = C.c_uint32(0xffffffff)
    rc = lib().qhuff_items_check(_np_ptr(a) if len(a) else None,
                                 len(a) // 8, C.byref(bad))
    return rc, (bad.value if rc != OK else None)


def encode_headers_bound(in_bytes, n, m):
    return int(lib().qhuff_encode_headers_bound(in_bytes, n, m))


def static_probe_tables():
    """qhuff_static_probe_tables -> (name2id_plus_one, nameval2id_plus_one),
    uint8 [512] each: the probe tables the library builds from the static
    table with its own XXH32."""
    import numpy as np
    a, b = np.zeros(512, dtype=np.uint8), np.zeros(512, dtype=np.uint8)
    rc = lib().qhuff_static_probe_tables(_np_ptr(a), _np_ptr(b))
    if rc != OK:
        raise QhuffError("qhuff_static_probe_tables failed: %d" % rc)
    return a, b


def static_lookup_cpu(data, off):
    """qhuff_static_lookup_cpu: the lookup kernel's source run on the host
    over headers data[off[2i] : off[2i+1]] / data[off[2i+1] : off[2i+2]] ->
    (name_hash, nameval_hash uint32 [n], kind, static_id uint8 [n])."""
    import numpy as np
    data = np.ascontiguousarray(data, dtype=np.uint8)
    off = np.ascontiguousarray(off, dtype=np.uint32)
    n = (len(off) - 1) // 2
    h1, h2 = (np.zeros(max(n, 1), dtype=np.uint32) for _ in range(2))
    kind, sid = (np.zeros(max(n, 1), dtype=np.uint8) for _ in range(2))
    rc = lib().qhuff_static_lookup_cpu(
        _np_ptr(data) if len(data) else _np_ptr(np.zeros(1, np.uint8)),
        _np_ptr(off), n, _np_ptr(h1), _np_ptr(h2), _np_ptr(kind), _np_ptr(sid))
    if rc != OK:
        raise QhuffError("qhuff_static_lookup_cpu failed: %d" % rc)
    return h1[:n], h2[:n], kind[:n], sid[:n]


def encode_headers_dyn_bound(in_bytes, n, m):
    return int(lib().qhuff_encode_headers_dyn_bound(in_bytes, n, m))


def dyn_index_slots(d):
    """qhuff_dyn_index_slots: the slots of each of the dynamic lookup's two
    indices for a table of d entries"""
    return int(lib().qhuff_dyn_index_slots(d))


def _window(table, win):
    """(lo, hi) of a window, None: the whole table (data, off, first, ...)"""
    if win is not None:
        return int(win[0]), int(win[1])
    off, first = table[1], (table[2] if len(table) > 2 else 0)
    d = 0 if off is None else (len(off) - 1) // 2
    return first, first + d


def dyn_lookup_cpu(data, off, table, win=None):
    """qhuff_dyn_lookup_cpu: the dynamic lookup kernel's source run on the
    host.  table: (data, off, first, max_entries) host arrays as
    dyn_table_host takes them; win: (lo, hi) or None, the whole table ->
    (ret, name_hash, nameval_hash uint32 [n], kind, static_id uint8 [n],
    dyn_id uint32 [n])."""
    import numpy as np
    data = np.ascontiguousarray(data, dtype=np.uint8)
    off = np.ascontiguousarray(off, dtype=np.uint32)
    n = (len(off) - 1) // 2
    h1, h2, did = (np.zeros(max(n, 1), dtype=np.uint32) for _ in range(3))
    kind, sid = (np.zeros(max(n, 1), dtype=np.uint8) for _ in range(2))
    t, keep = dyn_table_host(*table)
    lo, hi = _window(table, win)
    ret = lib().qhuff_dyn_lookup_cpu(
        _np_ptr(data) if len(data) else _np_ptr(np.zeros(1, np.uint8)),
        _np_ptr(off), n, C.byref(t), lo, hi, _np_ptr(h1), _np_ptr(h2),
        _np_ptr(kind), _np_ptr(sid), _np_ptr(did))
    del keep
    return ret, h1[:n], h2[:n], kind[:n], sid[:n], did[:n]


def dec_int(buf, prefix_bits):
    """qhuff_dec_int (the scanners' lsqpack_dec_int, complete buffer) ->
    (rc, value, consumed)."""
    v, used = C.c_uint64(), C.c_size_t()
    rc = lib().qhuff_dec_int(bytes(buf), len(buf), prefix_bits, C.byref(v),
                             C.byref(used))
    return rc, (v.value if rc == OK else None), (used.value if rc == OK else 0)


def frame_literal(prefix_bits, s, huff, first_byte=0, dst_len=1 << 16):
    """lsqpack_enc_enc_str framing of s given its precomputed Huffman
    payload (include/qhuff.h qhuff_frame_literal) -> bytes or -1."""
    buf = C.create_string_buffer(max(dst_len, 1))
    buf[0] = first_byte
    r = lib().qhuff_frame_literal(prefix_bits, buf, dst_len, s, len(s), huff,
                                  len(huff))
    return r if r < 0 else buf.raw[:r]


TOKEN_ALPHABET = b"abcdefghijklmnopqrstuvwxyz0123456789-_./:;=, "
BASE64_ALPHABET = (b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz"
                   b"0123456789+/")


def synth_batch(n, seed=0, min_len=8, max_len=64, alphabet=TOKEN_ALPHABET):
    """Synthetic header strings: returns (data uint8,
    in_off uint32[n+1]) numpy arrays."""
    import numpy as np
    data = np.zeros(max(n * max_len, 1), dtype=np.uint8)
    off = np.zeros(n + 1, dtype=np.uint32)
    tot = lib().qhuff_synth_batch(seed, n, min_len, max_len, alphabet,
                                  len(alphabet), _np_ptr(data), _np_ptr(off))
    return data[:tot].copy(), off


# ---- exact-signature shims (include/qhuff_lsqpack.h) -------------------------

def lsqpack_enc_enc_str(prefix_bits, s, first_byte=0, dst_len=1 << 16):
    """qhuff_lsqpack_enc_enc_str -> bytes or -1 (thread's default context)."""
    buf = C.create_string_buffer(max(dst_len, 1))
    buf[0] = first_byte
    r = lib().qhuff_lsqpack_enc_enc_str(prefix_bits, buf, dst_len, s, len(s))
    return r if r < 0 else buf.raw[:r]


def lsqpack_huff_decode(src, dst_len, state=None, final=1):
    """qhuff_lsqpack_huff_decode -> (status, dst[:n_dst], n_dst, n_src,
    state)."""
    s = C.create_string_buffer(bytes(src), len(src) + 1)
    d = C.create_string_buffer(max(dst_len, 1))
    st = state if state is not None else DecodeState(0, 0, 0)
    rv = lib().qhuff_lsqpack_huff_decode(s, len(src), d, dst_len, C.byref(st),
                                         final)
    return rv.status, d.raw[:rv.n_dst], rv.n_dst, rv.n_src, st


def lsqpack_set_decode_full(fn):
    """Register the streaming decoder (a DECODE_FULL_FN or None); returns
    the ctypes callback object, which the caller must keep alive."""
    cb = fn if fn is None or isinstance(fn, DECODE_FULL_FN) else DECODE_FULL_FN(fn)
    lib().qhuff_lsqpack_set_decode_full(
        C.cast(cb, C.c_void_p) if cb is not None else None)
    return cb


# ---- one batch over several contexts (qhuff_*_batch_*multi) ---------------

def _ctx_array(codecs):
    arr = (C.c_void_p * len(codecs))(*[c._ctx.value for c in codecs])
    return arr


def host_register(arr):
    """qhuff_host_register over a contiguous numpy array: the host-memory
    calls then move it by DMA directly (no staging copy) -> rc."""
    assert arr.flags["C_CONTIGUOUS"]
    return int(lib().qhuff_host_register(_np_ptr(arr), arr.nbytes))


def host_unregister(arr):
    return int(lib().qhuff_host_unregister(_np_ptr(arr)))


class registered:
    """with registered(a, b, ...): the arrays are registered for direct DMA
    inside the block (raises QhuffError if a registration fails)."""

    def __init__(self, *arrays):
        self.arrays = arrays
        self.done = []

    def __enter__(self):
        for a in self.arrays:
            rc = host_register(a)
            if rc:
                self.__exit__()
                raise QhuffError("qhuff_host_register: %d %s"
                                 % (rc, lib().qhuff_last_error(None).decode()))
            self.done.append(a)
        return self

    def __exit__(self, *exc):
        while self.done:
            host_unregister(self.done.pop())
        return False


def encode_host_multi(codecs, data, in_off, mode=ENC_PAYLOAD):
    """qhuff_encode_batch_host_multi: host batch sharded over the contexts
    -> (out bytes, global out_off)."""
    import numpy as np
    data = np.ascontiguousarray(data, dtype=np.uint8)
    in_off = np.ascontiguousarray(in_off, dtype=np.uint32)
    n = len(in_off) - 1
    out = np.zeros(encode_bound(int(in_off[-1] - in_off[0]), n, mode),
                   dtype=np.uint8)
    out_off = np.zeros(n + 1, dtype=np.uint32)
    rc = lib().qhuff_encode_batch_host_multi(
        _ctx_array(codecs), len(codecs), _np_ptr(data), _np_ptr(in_off), n,
        mode, _np_ptr(out), _np_ptr(out_off))
    if rc:
        raise QhuffError("qhuff_encode_batch_host_multi: %d" % rc)
    return out[:out_off[-1]], out_off


def decode_host_multi(codecs, data, in_off):
    """qhuff_decode_batch_host_multi -> (out bytes, out_off, status)."""
    import numpy as np
    data = np.ascontiguousarray(data, dtype=np.uint8)
    in_off = np.ascontiguousarray(in_off, dtype=np.uint32)
    n = len(in_off) - 1
    out = np.zeros(decode_bound(int(in_off[-1] - in_off[0]), n),
                   dtype=np.uint8)
    out_off = np.zeros(n + 1, dtype=np.uint32)
    status = np.zeros(max(n, 1), dtype=np.uint8)
    rc = lib().qhuff_decode_batch_host_multi(
        _ctx_array(codecs), len(codecs), _np_ptr(data), _np_ptr(in_off), n,
        _np_ptr(out), _np_ptr(out_off), _np_ptr(status))
    if rc:
        raise QhuffError("qhuff_decode_batch_host_multi: %d" % rc)
    return out[:out_off[-1]], out_off, status[:n]


def batch_multi(codecs, shards, encode, mode=ENC_PAYLOAD, rebase=True):
    """qhuff_encode_batch_multi / qhuff_decode_batch_multi over
    device-resident shards: shards[k] = dict(in_, in_off, n, out, out_off,
    status, stream) of torch tensors / ints (stream: a torch stream or
    None) -> base list (g + 1 entries)."""
    g = len(codecs)
    arr = (Shard * g)()
    for k, s in enumerate(shards):
        st = s.get("stream")
        arr[k] = Shard(s["in_"].data_ptr(), s["in_off"].data_ptr(), s["n"],
                       s["out"].data_ptr(), s["out_off"].data_ptr(),
                       s["status"].data_ptr() if s.get("status") is not None
                       else None,
                       st.cuda_stream if st is not None else None)
    base = (C.c_uint64 * (g + 1))()
    if encode:
        rc = lib().qhuff_encode_batch_multi(_ctx_array(codecs), g, arr, mode,
                                            base, int(rebase))
    else:
        rc = lib().qhuff_decode_batch_multi(_ctx_array(codecs), g, arr, base,
                                            int(rebase))
    if rc:
        raise QhuffError("qhuff_%s_batch_multi: %d"
                         % ("encode" if encode else "decode", rc))
    return list(base)


# ---- device codec ----------------------------------------------------------

class Codec:
    """One qhuff_ctx on one GPU.  Tensor arguments are torch CUDA(HIP)
    tensors; offsets are int32 tensors reinterpreted as uint32."""

    def __init__(self, device=0):
        self._ctx = C.c_void_p()
        rc = lib().qhuff_open(device, C.byref(self._ctx))
        if rc != OK:
            raise QhuffError("qhuff_open(device=%d) failed: %d (%s)" % (
                device, rc, lib().qhuff_last_error(None).decode()))
        self.device = device

    def close(self):
        if self._ctx:
            svc = getattr(self, "_service", None)
            if svc is not None:
                svc._svc = C.c_void_p()      # qhuff_close frees it
            lib().qhuff_close(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def profile_read(self):
        """Phase stamps of the last launch (QHUFF_PROFILE build) or the path
        records of the last tile launch, 8 words a tile (QH_PATH_TRACE
        build, libqhuff_trace.so), as a numpy uint64 array; None in a
        normal build."""
        import numpy as np
        n = lib().qhuff_profile_read(self._ctx, None, 0)
        if not n:
            return None
        a = np.zeros(n, dtype=np.uint64)
        lib().qhuff_profile_read(self._ctx, a.ctypes.data, n)
        return a

    def device_error(self):
        """Synchronise and return (then clear) the sticky device error word
        (0 = none, 1 = a look-back wait gave up)."""
        return int(lib().qhuff_device_error(self._ctx))

    def timing(self, on=True, every=1):
        """qhuff_timing_enable: time every later launch of this context (or
        every `every`-th of each kind) by its dispatch's own start / stop
        timestamps."""
        self._check(lib().qhuff_timing_enable(
            self._ctx, max(1, int(every)) if on else 0), "qhuff_timing_enable")

    def kernel_variant(self, kind):
        """qhuff_kernel_variant: 1 if the last launch of kind (KIND_ENCODE /
        KIND_DECODE) ran the full kernel, 0 for the lean one."""
        r = lib().qhuff_kernel_variant(self._ctx, kind)
        if r < 0:
            self._check(r, "qhuff_kernel_variant")
        return r

    def grid_waves(self, kind):
        """qhuff_grid_waves: the most waves one launch of kind (KIND_ENCODE /
        KIND_DECODE / KIND_HASH) puts on the device."""
        r = lib().qhuff_grid_waves(self._ctx, kind)
        if r < 0:
            self._check(r, "qhuff_grid_waves")
        return r

    def batch_hint(self, kind, hint):
        """qhuff_batch_hint: the next launch of kind runs the full (1) or
        lean (0) kernel, or no hint (-1: the full kernel)."""
        self._check(lib().qhuff_batch_hint(self._ctx, kind, hint),
                    "qhuff_batch_hint")

    def timing_read(self, max_launches=TIMING_SLOTS):
        """qhuff_timing_read -> list of (kind, microseconds) of the launches
        timed since timing() or the last read, oldest first (KIND_*)."""
        kinds = (C.c_uint32 * max_launches)()
        us = (C.c_double * max_launches)()
        n = lib().qhuff_timing_read(self._ctx, kinds, us, max_launches)
        if n < 0:
            self._check(n, "qhuff_timing_read")
        return [(int(kinds[i]), float(us[i])) for i in range(n)]

    def _check(self, rc, what):
        if rc != OK:
            err = lib().qhuff_last_error(self._ctx)
            raise QhuffError("%s failed: %d (%s)" % (what, rc,
                             err.decode() if err else ""))

    @staticmethod
    def _stream(stream):
        if stream is None:
            import torch
            stream = torch.cuda.current_stream()
        return C.c_void_p(stream.cuda_stream)

    # device-resident batch calls ------------------------------------------
    def encode_into(self, data, in_off, n, mode, out, out_off, stream=None):
        rc = lib().qhuff_encode_batch(self._ctx, data.data_ptr(),
                                      in_off.data_ptr(), n, mode,
                                      out.data_ptr(), out_off.data_ptr(),
                                      self._stream(stream))
        self._check(rc, "qhuff_encode_batch")

    def decode_into(self, data, in_off, n, out, out_off, status, stream=None):
        rc = lib().qhuff_decode_batch(self._ctx, data.data_ptr(),
                                      in_off.data_ptr(), n, out.data_ptr(),
                                      out_off.data_ptr(), status.data_ptr(),
                                      self._stream(stream))
        self._check(rc, "qhuff_decode_batch")

    def encode(self, data, in_off, mode=ENC_PAYLOAD, stream=None):
        """data: uint8 cuda tensor, in_off: int32 cuda tensor [n+1].
        Returns (out uint8 [bound], out_off int32 [n+1])."""
        import torch
        n = in_off.numel() - 1
        in_bytes = int(data.numel())
        out = torch.empty(encode_bound(in_bytes, n, mode), dtype=torch.uint8,
                          device=data.device)
        out_off = torch.empty(n + 1, dtype=torch.int32, device=data.device)
        self.encode_into(data, in_off, n, mode, out, out_off, stream)
        return out, out_off

    def decode(self, data, in_off, stream=None):
        import torch
        n = in_off.numel() - 1
        out = torch.empty(decode_bound(int(data.numel()), n),
                          dtype=torch.uint8, device=data.device)
        out_off = torch.empty(n + 1, dtype=torch.int32, device=data.device)
        status = torch.empty(max(n, 1), dtype=torch.uint8, device=data.device)
        self.decode_into(data, in_off, n, out, out_off, status, stream)
        return out, out_off, status[:n]

    # resumable decode: one chunk of each string per call ---------------------
    def decode_stream_into(self, data, in_off, n, state, flags, out, out_off,
                           status, stream=None):
        """qhuff_decode_stream: state is a uint8 tensor [n, 2] ({state, eos}
        per string, read and written), flags a uint8 tensor [n] or None."""
        rc = lib().qhuff_decode_stream(
            self._ctx, data.data_ptr(), in_off.data_ptr(), n,
            state.data_ptr(), flags.data_ptr() if flags is not None else None,
            out.data_ptr(), out_off.data_ptr(), status.data_ptr(),
            self._stream(stream))
        self._check(rc, "qhuff_decode_stream")

    def decode_stream(self, data, in_off, state=None, flags=None, stream=None):
        """One chunk of each of n strings (device tensors).  state None: fresh
        strings.  Returns (out, out_off, status, state): state is updated in
        place and passed to the call that continues the strings."""
        import torch
        n = in_off.numel() - 1
        if state is None:
            state = torch.zeros((max(n, 1), 2), dtype=torch.uint8,
                                device=data.device)
        out = torch.empty(decode_stream_bound(int(data.numel()), n),
                          dtype=torch.uint8, device=data.device)
        out_off = torch.empty(n + 1, dtype=torch.int32, device=data.device)
        status = torch.empty(max(n, 1), dtype=torch.uint8, device=data.device)
        self.decode_stream_into(data, in_off, n, state, flags, out, out_off,
                                status, stream)
        return out, out_off, status[:n], state

    def decode_stream_host(self, data, in_off, state=None, flags=None):
        """qhuff_decode_stream_host over numpy arrays -> (out, out_off,
        status, state); state: uint8 [n, 2], a copy updated by the call."""
        import numpy as np
        data = np.ascontiguousarray(data, dtype=np.uint8)
        in_off = np.ascontiguousarray(in_off, dtype=np.uint32)
        n = len(in_off) - 1
        state = (np.zeros((max(n, 1), 2), dtype=np.uint8) if state is None
                 else np.array(state, dtype=np.uint8).reshape(-1, 2))
        if flags is not None:
            flags = np.ascontiguousarray(flags, dtype=np.uint8)
        out = np.zeros(decode_stream_bound(int(in_off[-1] - in_off[0]), n),
                       dtype=np.uint8)
        out_off = np.zeros(n + 1, dtype=np.uint32)
        status = np.zeros(max(n, 1), dtype=np.uint8)
        rc = lib().qhuff_decode_stream_host(
            self._ctx, _np_ptr(data), _np_ptr(in_off), n, _np_ptr(state),
            _np_ptr(flags) if flags is not None else None, _np_ptr(out),
            _np_ptr(out_off), _np_ptr(status))
        self._check(rc, "qhuff_decode_stream_host")
        return out[:out_off[-1]], out_off, status[:n], state[:n]

    # header hashing (XXH32, lsqpack.c:1681-1685) ---------------------------
    def xxh32_headers_into(self, data, off, n, seed, name_hash, nameval_hash,
                           stream=None):
        rc = lib().qhuff_xxh32_headers(self._ctx, data.data_ptr(),
                                       off.data_ptr(), n, seed,
                                       name_hash.data_ptr(),
                                       nameval_hash.data_ptr(),
                                       self._stream(stream))
        self._check(rc, "qhuff_xxh32_headers")

    def xxh32_headers(self, data, off, seed=XXH_SEED, stream=None):
        """off: int32 cuda tensor [2n+1] (name, value, name, value ...).
        Returns (name_hash, nameval_hash) int32 tensors [n] (uint32 bits)."""
        import torch
        n = (off.numel() - 1) // 2
        h1 = torch.empty(max(n, 1), dtype=torch.int32, device=data.device)
        h2 = torch.empty(max(n, 1), dtype=torch.int32, device=data.device)
        self.xxh32_headers_into(data, off, n, seed & 0xffffffff, h1, h2,
                                stream)
        return h1[:n], h2[:n]

    def xxh32_headers_host(self, data, off, seed=XXH_SEED):
        """Host numpy buffers -> (name_hash, nameval_hash) uint32[n]."""
        import numpy as np
        data = np.ascontiguousarray(data, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint32)
        n = (len(off) - 1) // 2
        h1 = np.zeros(max(n, 1), dtype=np.uint32)
        h2 = np.zeros(max(n, 1), dtype=np.uint32)
        rc = lib().qhuff_xxh32_headers_host(self._ctx, _np_ptr(data),
                                            _np_ptr(off), n, seed & 0xffffffff,
                                            _np_ptr(h1), _np_ptr(h2))
        self._check(rc, "qhuff_xxh32_headers_host")
        return h1[:n], h2[:n]

    def xxh32(self, data, in_off, seed=XXH_SEED, stream=None):
        """hash[i] = XXH32(string i, seed); int32 tensor [n]."""
        import torch
        n = in_off.numel() - 1
        h = torch.empty(max(n, 1), dtype=torch.int32, device=data.device)
        rc = lib().qhuff_xxh32_batch(self._ctx, data.data_ptr(),
                                     in_off.data_ptr(), n, seed & 0xffffffff,
                                     h.data_ptr(), self._stream(stream))
        self._check(rc, "qhuff_xxh32_batch")
        return h[:n]

    # headers against the static table, header lists to field sections -------
    def static_lookup_into(self, data, off, n, name_hash, nameval_hash, kind,
                           static_id, stream=None):
        """qhuff_static_lookup on device tensors; name_hash / nameval_hash
        may be None"""
        rc = lib().qhuff_static_lookup(
            self._ctx, data.data_ptr(), off.data_ptr(), n,
            name_hash.data_ptr() if name_hash is not None else None,
            nameval_hash.data_ptr() if nameval_hash is not None else None,
            kind.data_ptr(), static_id.data_ptr(), self._stream(stream))
        self._check(rc, "qhuff_static_lookup")

    def static_lookup(self, data, off, stream=None):
        """off: int32 cuda tensor [2n+1] (name, value, name, value ...).
        Returns (name_hash, nameval_hash int32 [n] (uint32 bits), kind,
        static_id uint8 [n])."""
        import torch
        n = (off.numel() - 1) // 2
        h1, h2 = (torch.empty(max(n, 1), dtype=torch.int32, device=data.device)
                  for _ in range(2))
        kind, sid = (torch.empty(max(n, 1), dtype=torch.uint8,
                                 device=data.device) for _ in range(2))
        self.static_lookup_into(data, off, n, h1, h2, kind, sid, stream)
        return h1[:n], h2[:n], kind[:n], sid[:n]

    def static_lookup_host(self, data, off):
        """Host numpy buffers -> (name_hash, nameval_hash uint32 [n], kind,
        static_id uint8 [n])."""
        import numpy as np
        data = np.ascontiguousarray(data, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint32)
        n = (len(off) - 1) // 2
        h1, h2 = (np.zeros(max(n, 1), dtype=np.uint32) for _ in range(2))
        kind, sid = (np.zeros(max(n, 1), dtype=np.uint8) for _ in range(2))
        rc = lib().qhuff_static_lookup_host(
            self._ctx, _np_ptr(data), _np_ptr(off), n, _np_ptr(h1),
            _np_ptr(h2), _np_ptr(kind), _np_ptr(sid))
        self._check(rc, "qhuff_static_lookup_host")
        return h1[:n], h2[:n], kind[:n], sid[:n]

    def encode_headers_into(self, data, off, n, hflags, sec_hdr, m, out,
                            sec_out, kind=None, static_id=None, stream=None):
        """qhuff_encode_headers on device tensors; hflags, kind and static_id
        may be None.  sec_hdr must be a valid section list (the caller's
        duty)."""
        opt = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        rc = lib().qhuff_encode_headers(
            self._ctx, data.data_ptr(), off.data_ptr(), n, opt(hflags),
            sec_hdr.data_ptr(), m, out.data_ptr(), sec_out.data_ptr(),
            opt(kind), opt(static_id), self._stream(stream))
        self._check(rc, "qhuff_encode_headers")

    def encode_headers(self, data, off, sec_hdr, hflags=None, stream=None):
        """data: uint8 cuda tensor; off: int32 cuda tensor [2n+1]; sec_hdr:
        int32 cuda tensor [m+1]; hflags: uint8 cuda tensor [n] or None.
        Returns (out uint8 [bound], sec_out int32 [m+1], kind, static_id
        uint8 [n])."""
        import torch
        n, m = (off.numel() - 1) // 2, sec_hdr.numel() - 1
        out = torch.empty(encode_headers_bound(int(data.numel()), n, m),
                          dtype=torch.uint8, device=data.device)
        sec_out = torch.empty(m + 1, dtype=torch.int32, device=data.device)
        kind, sid = (torch.empty(max(n, 1), dtype=torch.uint8,
                                 device=data.device) for _ in range(2))
        self.encode_headers_into(data, off, n, hflags, sec_hdr, m, out,
                                 sec_out, kind, sid, stream)
        return out, sec_out, kind[:n], sid[:n]

    def encode_headers_host(self, data, off, sec_hdr, hflags=None):
        """qhuff_encode_headers_host over host buffers -> (out uint8 ndarray
        [sec_out[m]], sec_out uint32 [m+1], kind, static_id uint8 [n])."""
        import numpy as np
        data = np.ascontiguousarray(data, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint32)
        sec_hdr = np.ascontiguousarray(sec_hdr, dtype=np.uint32)
        if hflags is not None:
            hflags = np.ascontiguousarray(hflags, dtype=np.uint8)
        n, m = (len(off) - 1) // 2, len(sec_hdr) - 1
        out = np.zeros(encode_headers_bound(int(off[-1]) - int(off[0]), n, m),
                       dtype=np.uint8)
        sec_out = np.zeros(m + 1, dtype=np.uint32)
        kind, sid = (np.zeros(max(n, 1), dtype=np.uint8) for _ in range(2))
        rc = lib().qhuff_encode_headers_host(
            self._ctx, _np_ptr(data) if len(data) else None, _np_ptr(off), n,
            _np_ptr(hflags) if hflags is not None and n else None,
            _np_ptr(sec_hdr), m, _np_ptr(out), _np_ptr(sec_out),
            _np_ptr(kind), _np_ptr(sid))
        self._check(rc, "qhuff_encode_headers_host")
        return out[:sec_out[-1]], sec_out, kind[:n], sid[:n]

    # ... and among the dynamic table's entries ----------------------------------
    def dyn_lookup(self, data, off, tab_data, tab_off, first, max_entries,
                   win=None, stream=None):
        """qhuff_dyn_lookup on device tensors: data / off as static_lookup,
        tab_data uint8 / tab_off int32 [2d+1] cuda tensors (None, None: d =
        0); win (lo, hi) or None, the whole table -> (name_hash, nameval_hash
        int32 [n] (uint32 bits), kind, static_id uint8 [n], dyn_id int32 [n]
        (uint32 bits))."""
        import torch
        n = (off.numel() - 1) // 2
        d = (tab_off.numel() - 1) // 2 if tab_off is not None else 0
        h1, h2, did = (torch.empty(max(n, 1), dtype=torch.int32,
                                   device=data.device) for _ in range(3))
        kind, sid = (torch.empty(max(n, 1), dtype=torch.uint8,
                                 device=data.device) for _ in range(2))
        t = DynTable(tab_data.data_ptr() if d else None,
                     tab_off.data_ptr() if d else None, d, first, max_entries)
        lo, hi = win if win is not None else (first, first + d)
        rc = lib().qhuff_dyn_lookup(
            self._ctx, data.data_ptr(), off.data_ptr(), n, C.byref(t), lo, hi,
            h1.data_ptr(), h2.data_ptr(), kind.data_ptr(), sid.data_ptr(),
            did.data_ptr(), self._stream(stream))
        self._check(rc, "qhuff_dyn_lookup")
        return h1[:n], h2[:n], kind[:n], sid[:n], did[:n]

    def dyn_lookup_host(self, data, off, table, win=None):
        """qhuff_dyn_lookup_host over host buffers; table as dyn_table_host
        takes it -> (ret, name_hash, nameval_hash, kind, static_id, dyn_id);
        ret OK, or EINVAL / ERANGE of the argument checks."""
        import numpy as np
        data = np.ascontiguousarray(data, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint32)
        n = (len(off) - 1) // 2
        h1, h2, did = (np.zeros(max(n, 1), dtype=np.uint32) for _ in range(3))
        kind, sid = (np.zeros(max(n, 1), dtype=np.uint8) for _ in range(2))
        t, keep = dyn_table_host(*table)
        lo, hi = _window(table, win)
        ret = lib().qhuff_dyn_lookup_host(
            self._ctx, _np_ptr(data) if len(data) else None, _np_ptr(off), n,
            C.byref(t), lo, hi, _np_ptr(h1), _np_ptr(h2), _np_ptr(kind),
            _np_ptr(sid), _np_ptr(did))
        del keep
        if ret not in (EINVAL, ERANGE):
            self._check(ret, "qhuff_dyn_lookup_host")
        return ret, h1[:n], h2[:n], kind[:n], sid[:n], did[:n]

    def encode_headers_dyn_into(self, data, off, n, hflags, sec_hdr, m, tab,
                                sec_win, sec_base, out, sec_out, kind=None,
                                static_id=None, dyn_id=None, stream=None):
        """qhuff_encode_headers_dyn on device tensors; tab: a DynTable of
        device pointers; hflags, sec_win, sec_base, kind, static_id and
        dyn_id may be None.  The form of the arrays is the caller's duty."""
        opt = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        rc = lib().qhuff_encode_headers_dyn(
            self._ctx, data.data_ptr(), off.data_ptr(), n, opt(hflags),
            sec_hdr.data_ptr(), m, C.byref(tab), opt(sec_win), opt(sec_base),
            out.data_ptr(), sec_out.data_ptr(), opt(kind), opt(static_id),
            opt(dyn_id), self._stream(stream))
        self._check(rc, "qhuff_encode_headers_dyn")

    def encode_headers_dyn(self, data, off, sec_hdr, tab_data, tab_off, first,
                           max_entries, sec_win=None, sec_base=None,
                           hflags=None, stream=None):
        """Device tensors as encode_headers, the table as dyn_lookup, sec_win
        int32 [2m] / sec_base int32 [m] cuda tensors or None -> (out uint8
        [bound], sec_out int32 [m+1], kind, static_id uint8 [n], dyn_id int32
        [n])."""
        import torch
        n, m = (off.numel() - 1) // 2, sec_hdr.numel() - 1
        d = (tab_off.numel() - 1) // 2 if tab_off is not None else 0
        out = torch.empty(encode_headers_dyn_bound(int(data.numel()), n, m),
                          dtype=torch.uint8, device=data.device)
        sec_out = torch.empty(m + 1, dtype=torch.int32, device=data.device)
        kind, sid = (torch.empty(max(n, 1), dtype=torch.uint8,
                                 device=data.device) for _ in range(2))
        did = torch.empty(max(n, 1), dtype=torch.int32, device=data.device)
        t = DynTable(tab_data.data_ptr() if d else None,
                     tab_off.data_ptr() if d else None, d, first, max_entries)
        self.encode_headers_dyn_into(data, off, n, hflags, sec_hdr, m, t,
                                     sec_win, sec_base, out, sec_out, kind,
                                     sid, did, stream)
        return out, sec_out, kind[:n], sid[:n], did[:n]

    def encode_headers_dyn_host(self, data, off, sec_hdr, table, sec_win=None,
                                sec_base=None, hflags=None):
        """qhuff_encode_headers_dyn_host over host buffers; table as
        dyn_table_host takes it, sec_win uint32 [2m] / sec_base uint32 [m] or
        None -> (ret, out uint8 [sec_out[m]], sec_out uint32 [m+1], kind,
        static_id uint8 [n], dyn_id uint32 [n]); ret OK, or EINVAL / ERANGE
        of the argument checks (the arrays then as they were made)."""
        import numpy as np
        data = np.ascontiguousarray(data, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint32)
        sec_hdr = np.ascontiguousarray(sec_hdr, dtype=np.uint32)
        if hflags is not None:
            hflags = np.ascontiguousarray(hflags, dtype=np.uint8)
        n, m = (len(off) - 1) // 2, len(sec_hdr) - 1
        span = max(int(off[-1]) - int(off[0]), 0)
        out = np.zeros(encode_headers_dyn_bound(span, n, m), dtype=np.uint8)
        sec_out = np.zeros(m + 1, dtype=np.uint32)
        kind, sid = (np.zeros(max(n, 1), dtype=np.uint8) for _ in range(2))
        did = np.zeros(max(n, 1), dtype=np.uint32)
        t, keep = dyn_table_host(*table)
        win = _sec_win_host(sec_win)
        base = None if sec_base is None else \
            np.ascontiguousarray(sec_base, dtype=np.uint32)
        ret = lib().qhuff_encode_headers_dyn_host(
            self._ctx, _np_ptr(data) if len(data) else None, _np_ptr(off), n,
            _np_ptr(hflags) if hflags is not None and n else None,
            _np_ptr(sec_hdr), m, C.byref(t),
            _np_ptr(win) if win is not None and m else None,
            _np_ptr(base) if base is not None and m else None, _np_ptr(out),
            _np_ptr(sec_out), _np_ptr(kind), _np_ptr(sid), _np_ptr(did))
        del keep
        if ret in (EINVAL, ERANGE):
            return ret, out[:0], sec_out, kind[:n], sid[:n], did[:n]
        self._check(ret, "qhuff_encode_headers_dyn_host")
        return ret, out[:sec_out[-1]], sec_out, kind[:n], sid[:n], did[:n]

    # field sections decoded to header lists --------------------------------
    def scan_headers_into(self, buf, sec_off, m, strs, max_hdrs, hdr_off, rc,
                          kind=None, static_id=None, hflags=None, stream=None):
        """qhuff_scan_headers: all device tensors; strs holds 32 * max_hdrs
        bytes; kind, static_id and hflags may be None."""
        opt = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        r = lib().qhuff_scan_headers(
            self._ctx, buf.data_ptr(), sec_off.data_ptr(), m, opt(strs),
            max_hdrs, hdr_off.data_ptr(), rc.data_ptr(), opt(kind),
            opt(static_id), opt(hflags), self._stream(stream))
        self._check(r, "qhuff_scan_headers")

    def scan_headers(self, buf, sec_off, max_hdrs, stream=None):
        """buf: uint8 cuda tensor of wire bytes; sec_off: int32 cuda tensor
        [m+1].  Returns device tensors (strs uint8 [32 * max_hdrs], hdr_off
        int32 [m+1], rc int32 [m], kind, static_id, hflags uint8 [max_hdrs]);
        hdr_off[m] is the full count, to be compared with max_hdrs."""
        import torch
        m = sec_off.numel() - 1
        dev = buf.device
        k = max(max_hdrs, 1)
        strs = torch.empty(32 * k, dtype=torch.uint8, device=dev)
        hdr_off = torch.empty(m + 1, dtype=torch.int32, device=dev)
        rc = torch.empty(max(m, 1), dtype=torch.int32, device=dev)
        kind, sid, hf = (torch.empty(k, dtype=torch.uint8, device=dev)
                         for _ in range(3))
        self.scan_headers_into(buf, sec_off, m, strs, max_hdrs, hdr_off, rc,
                               kind, sid, hf, stream)
        return strs, hdr_off, rc[:m], kind, sid, hf

    def scan_headers_host(self, buf, sec_off, max_hdrs=None):
        """qhuff_scan_headers_host over host arrays -> as scan_headers_cpu
        (max_hdrs None: a first call with room for none counts them)."""
        if max_hdrs is None:
            max_hdrs = int(self.scan_headers_host(buf, sec_off, 0)[2][-1])
        buf, sec_off, m, strs, hdr_off, rc, kind, sid, hf = \
            _headers_host_args(buf, sec_off, max_hdrs)
        ret = lib().qhuff_scan_headers_host(
            self._ctx, _np_ptr(buf) if len(buf) else None, _np_ptr(sec_off),
            m, _np_ptr(strs), max_hdrs, _np_ptr(hdr_off), _np_ptr(rc),
            _np_ptr(kind), _np_ptr(sid), _np_ptr(hf))
        if ret != ERANGE:
            self._check(ret, "qhuff_scan_headers_host")
        n = min(int(hdr_off[-1]), max_hdrs)
        return ret, strs[:32 * n], hdr_off, rc[:m], kind[:n], sid[:n], hf[:n]

    def decode_headers_into(self, buf, strs, n, max_len, out, off, status,
                            stream=None):
        """qhuff_decode_headers: buf the wire bytes, strs the 2n descriptors
        (16 bytes each), all device tensors; the descriptors' form is the
        caller's duty."""
        rc = lib().qhuff_decode_headers(
            self._ctx, buf.data_ptr(), strs.data_ptr(), n, max_len or 0,
            out.data_ptr(), off.data_ptr(), status.data_ptr(),
            self._stream(stream))
        self._check(rc, "qhuff_decode_headers")

    def decode_headers(self, buf, strs, n, max_len=None, stream=None,
                       wire_bytes=None):
        """buf: uint8 cuda tensor of wire bytes; strs: uint8 cuda tensor of
        the 2n descriptors.  Returns (out uint8 [bound], off int32 [2n+1],
        status uint8 [2n]).  wire_bytes: the sections' bytes when they are
        fewer than buf's (the bound)."""
        import torch
        if wire_bytes is None:
            wire_bytes = int(buf.numel())
        out = torch.empty(decode_headers_bound(wire_bytes, n),
                          dtype=torch.uint8, device=buf.device)
        off = torch.empty(2 * n + 1, dtype=torch.int32, device=buf.device)
        status = torch.empty(max(2 * n, 1), dtype=torch.uint8,
                             device=buf.device)
        self.decode_headers_into(buf, strs, n, max_len, out, off, status,
                                 stream)
        return out, off, status[:2 * n]

    def decode_headers_host(self, buf, sec_off, max_len=None, max_hdrs=None,
                            hashes=False):
        """qhuff_decode_headers_host: scan and decode in one call -> (ret,
        hdr_off, rc, kind, static_id, hflags, out, off, status[, name_hash,
        nameval_hash]); ret OK, or ERANGE (hdr_off[-1] > max_hdrs: nothing
        decoded, the arrays after rc None).  max_hdrs None:
        scan_headers_host counts the headers first."""
        import numpy as np
        if max_hdrs is None:
            max_hdrs = int(self.scan_headers_host(buf, sec_off, 0)[2][-1])
        buf, sec_off, m, _, hdr_off, rc, kind, sid, hf = \
            _headers_host_args(buf, sec_off, max_hdrs)
        wire = max(int(sec_off[-1]) - int(sec_off[0]), 0)
        out = np.zeros(decode_headers_bound(wire, max_hdrs), dtype=np.uint8)
        off = np.zeros(2 * max_hdrs + 1, dtype=np.uint32)
        status = np.zeros(max(2 * max_hdrs, 1), dtype=np.uint8)
        h1, h2 = (np.zeros(max(max_hdrs, 1), dtype=np.uint32)
                  for _ in range(2))
        ret = lib().qhuff_decode_headers_host(
            self._ctx, _np_ptr(buf) if len(buf) else None, _np_ptr(sec_off),
            m, max_len or 0, max_hdrs, _np_ptr(hdr_off), _np_ptr(rc),
            _np_ptr(kind), _np_ptr(sid), _np_ptr(hf), _np_ptr(out),
            _np_ptr(off), _np_ptr(status), _np_ptr(h1) if hashes else None,
            _np_ptr(h2) if hashes else None)
        tail = (None,) * (8 if hashes else 6)
        if ret == ERANGE:
            return (ret, hdr_off, rc[:m]) + tail
        self._check(ret, "qhuff_decode_headers_host")
        n = int(hdr_off[-1])
        res = (ret, hdr_off, rc[:m], kind[:n], sid[:n], hf[:n],
               out[:off[2 * n]], off[:2 * n + 1], status[:2 * n])
        return res + ((h1[:n], h2[:n]) if hashes else ())

    # ... against the dynamic table's entries --------------------------------
    def scan_headers_dyn_into(self, buf, sec_off, m, tab_off, d, first,
                              max_entries, sec_win, strs, max_hdrs, hdr_off,
                              rc, kind=None, static_id=None, hflags=None,
                              dyn_id=None, stream=None):
        """qhuff_scan_headers_dyn: all device tensors; tab_off the table's
        int32 [2d + 1] offsets (None with d = 0), sec_win int32 [2m] or
        None; kind, static_id, hflags and dyn_id may be None."""
        opt = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        t = DynTable(None, opt(tab_off) if d else None, d, first, max_entries)
        r = lib().qhuff_scan_headers_dyn(
            self._ctx, buf.data_ptr(), sec_off.data_ptr(), m, C.byref(t),
            opt(sec_win), opt(strs), max_hdrs, hdr_off.data_ptr(),
            rc.data_ptr(), opt(kind), opt(static_id), opt(hflags),
            opt(dyn_id), self._stream(stream))
        self._check(r, "qhuff_scan_headers_dyn")

    def scan_headers_dyn(self, buf, sec_off, tab_off, first, max_entries,
                         sec_win, max_hdrs, stream=None):
        """scan_headers against the table -> (strs, hdr_off, rc, kind,
        static_id, hflags, dyn_id int32 [max_hdrs]) device tensors."""
        import torch
        m = sec_off.numel() - 1
        dev = buf.device
        k = max(max_hdrs, 1)
        strs = torch.empty(32 * k, dtype=torch.uint8, device=dev)
        hdr_off = torch.empty(m + 1, dtype=torch.int32, device=dev)
        rc = torch.empty(max(m, 1), dtype=torch.int32, device=dev)
        kind, sid, hf = (torch.empty(k, dtype=torch.uint8, device=dev)
                         for _ in range(3))
        did = torch.empty(k, dtype=torch.int32, device=dev)
        d = (tab_off.numel() - 1) // 2 if tab_off is not None else 0
        self.scan_headers_dyn_into(buf, sec_off, m, tab_off, d, first,
                                   max_entries, sec_win, strs, max_hdrs,
                                   hdr_off, rc, kind, sid, hf, did, stream)
        return strs, hdr_off, rc[:m], kind, sid, hf, did

    def scan_headers_dyn_host(self, buf, sec_off, table, sec_win=None,
                              max_hdrs=None):
        """qhuff_scan_headers_dyn_host over host arrays -> as
        scan_headers_dyn_cpu."""
        import numpy as np
        if max_hdrs is None:
            max_hdrs = int(self.scan_headers_dyn_host(buf, sec_off, table,
                                                      sec_win, 0)[2][-1])
        buf, sec_off, m, strs, hdr_off, rc, kind, sid, hf = \
            _headers_host_args(buf, sec_off, max_hdrs)
        did = np.zeros(max(max_hdrs, 1), dtype=np.uint32)
        t, keep = dyn_table_host(*table)
        win = _sec_win_host(sec_win)
        ret = lib().qhuff_scan_headers_dyn_host(
            self._ctx, _np_ptr(buf) if len(buf) else None, _np_ptr(sec_off),
            m, C.byref(t), _np_ptr(win) if win is not None else None,
            _np_ptr(strs), max_hdrs, _np_ptr(hdr_off), _np_ptr(rc),
            _np_ptr(kind), _np_ptr(sid), _np_ptr(hf), _np_ptr(did))
        del keep
        if ret not in (ERANGE, EINVAL):
            self._check(ret, "qhuff_scan_headers_dyn_host")
        n = min(int(hdr_off[-1]), max_hdrs)
        return (ret, strs[:32 * n], hdr_off, rc[:m], kind[:n], sid[:n],
                hf[:n], did[:n])

    def decode_headers_dyn_into(self, buf, strs, n, max_len, dyn, dyn_len,
                                out, off, status, stream=None):
        """qhuff_decode_headers_dyn: decode_headers_into and the table's
        bytes (a uint8 device tensor, or None with dyn_len 0)."""
        rc = lib().qhuff_decode_headers_dyn(
            self._ctx, buf.data_ptr(), strs.data_ptr(), n, max_len or 0,
            dyn.data_ptr() if dyn is not None and dyn_len else None, dyn_len,
            out.data_ptr(), off.data_ptr(), status.data_ptr(),
            self._stream(stream))
        self._check(rc, "qhuff_decode_headers_dyn")

    def decode_headers_dyn(self, buf, strs, n, dyn, dyn_longest, max_len=None,
                           stream=None, wire_bytes=None):
        """decode_headers with the table's bytes `dyn` (uint8 cuda tensor or
        None); dyn_longest: its longest name + value (the bound)."""
        import torch
        if wire_bytes is None:
            wire_bytes = int(buf.numel())
        out = torch.empty(decode_headers_dyn_bound(wire_bytes, n, dyn_longest),
                          dtype=torch.uint8, device=buf.device)
        off = torch.empty(2 * n + 1, dtype=torch.int32, device=buf.device)
        status = torch.empty(max(2 * n, 1), dtype=torch.uint8,
                             device=buf.device)
        self.decode_headers_dyn_into(buf, strs, n, max_len, dyn,
                                     int(dyn.numel()) if dyn is not None
                                     else 0, out, off, status, stream)
        return out, off, status[:2 * n]

    def decode_headers_dyn_host(self, buf, sec_off, table, sec_win=None,
                                max_len=None, max_hdrs=None, hashes=False):
        """qhuff_decode_headers_dyn_host: scan and decode against the table
        in one call -> (ret, hdr_off, rc, kind, static_id, hflags, dyn_id,
        out, off, status[, name_hash, nameval_hash]); ret OK, or ERANGE
        (hdr_off[-1] > max_hdrs: nothing decoded, the arrays after rc
        None)."""
        import numpy as np
        if max_hdrs is None:
            max_hdrs = int(self.scan_headers_dyn_host(buf, sec_off, table,
                                                      sec_win, 0)[2][-1])
        buf, sec_off, m, _, hdr_off, rc, kind, sid, hf = \
            _headers_host_args(buf, sec_off, max_hdrs)
        did = np.zeros(max(max_hdrs, 1), dtype=np.uint32)
        t, keep = dyn_table_host(*table)
        toff = keep[1]
        longest = int((toff[2::2] - toff[:-2:2]).max()) if t.d else 0
        win = _sec_win_host(sec_win)
        wire = max(int(sec_off[-1]) - int(sec_off[0]), 0)
        out = np.zeros(decode_headers_dyn_bound(wire, max_hdrs, longest),
                       dtype=np.uint8)
        off = np.zeros(2 * max_hdrs + 1, dtype=np.uint32)
        status = np.zeros(max(2 * max_hdrs, 1), dtype=np.uint8)
        h1, h2 = (np.zeros(max(max_hdrs, 1), dtype=np.uint32)
                  for _ in range(2))
        ret = lib().qhuff_decode_headers_dyn_host(
            self._ctx, _np_ptr(buf) if len(buf) else None, _np_ptr(sec_off),
            m, C.byref(t), _np_ptr(win) if win is not None else None,
            max_len or 0, max_hdrs, _np_ptr(hdr_off), _np_ptr(rc),
            _np_ptr(kind), _np_ptr(sid), _np_ptr(hf), _np_ptr(did),
            _np_ptr(out), _np_ptr(off), _np_ptr(status),
            _np_ptr(h1) if hashes else None, _np_ptr(h2) if hashes else None)
        del keep
        tail = (None,) * (9 if hashes else 7)
        if ret == ERANGE:
            return (ret, hdr_off, rc[:m]) + tail
        self._check(ret, "qhuff_decode_headers_dyn_host")
        n = int(hdr_off[-1])
        res = (ret, hdr_off, rc[:m], kind[:n], sid[:n], hf[:n], did[:n],
               out[:off[2 * n]], off[:2 * n + 1], status[:2 * n])
        return res + ((h1[:n], h2[:n]) if hashes else ())

    # ... over a set of tables, a table per section ---------------------------
    @staticmethod
    def dyn_tables_dev(tab_data, tab_off, ent, first, max_entries):
        """struct qhuff_dyn_tables of device tensors: tab_data uint8, tab_off
        int32 [2D + 1], ent int32 [T + 1], first / max_entries int32 [T]
        (uint32 bits); ent None: T = 0."""
        if ent is None:
            return DynTables(None, None, None, None, None, 0)
        opt = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        return DynTables(opt(tab_data), opt(tab_off), ent.data_ptr(),
                         first.data_ptr(), max_entries.data_ptr(),
                         first.numel())

    def scan_headers_tabs(self, buf, sec_off, tabs, sec_tab, sec_win,
                          max_hdrs, stream=None):
        """qhuff_scan_headers_tabs on device tensors; tabs: a DynTables of
        device pointers, sec_tab int32 [m] (None with T = 0), sec_win int32
        [2m] or None -> as scan_headers_dyn."""
        import torch
        m = sec_off.numel() - 1
        dev = buf.device
        k = max(max_hdrs, 1)
        strs = torch.empty(32 * k, dtype=torch.uint8, device=dev)
        hdr_off = torch.empty(m + 1, dtype=torch.int32, device=dev)
        rc = torch.empty(max(m, 1), dtype=torch.int32, device=dev)
        kind, sid, hf = (torch.empty(k, dtype=torch.uint8, device=dev)
                         for _ in range(3))
        did = torch.empty(k, dtype=torch.int32, device=dev)
        self.scan_headers_tabs_into(buf, sec_off, m, tabs, sec_tab, sec_win,
                                    strs, max_hdrs, hdr_off, rc, kind, sid,
                                    hf, did, stream)
        return strs, hdr_off, rc[:m], kind, sid, hf, did

    def scan_headers_tabs_into(self, buf, sec_off, m, tabs, sec_tab, sec_win,
                               strs, max_hdrs, hdr_off, rc, kind=None,
                               static_id=None, hflags=None, dyn_id=None,
                               stream=None):
        opt = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        r = lib().qhuff_scan_headers_tabs(
            self._ctx, buf.data_ptr(), sec_off.data_ptr(), m, C.byref(tabs),
            opt(sec_tab), opt(sec_win), opt(strs), max_hdrs,
            hdr_off.data_ptr(), rc.data_ptr(), opt(kind), opt(static_id),
            opt(hflags), opt(dyn_id), self._stream(stream))
        self._check(r, "qhuff_scan_headers_tabs")

    def scan_headers_tabs_host(self, buf, sec_off, tables, sec_tab,
                               sec_win=None, max_hdrs=None):
        """qhuff_scan_headers_tabs_host over host arrays -> as
        scan_headers_tabs_cpu."""
        import numpy as np
        if max_hdrs is None:
            max_hdrs = int(self.scan_headers_tabs_host(
                buf, sec_off, tables, sec_tab, sec_win, 0)[2][-1])
        buf, sec_off, m, strs, hdr_off, rc, kind, sid, hf = \
            _headers_host_args(buf, sec_off, max_hdrs)
        did = np.zeros(max(max_hdrs, 1), dtype=np.uint32)
        t, keep = dyn_tables_host(*(tables or ()))
        tab, win = _opt_u32(sec_tab), _sec_win_host(sec_win)
        ret = lib().qhuff_scan_headers_tabs_host(
            self._ctx, _np_ptr(buf) if len(buf) else None, _np_ptr(sec_off),
            m, C.byref(t), _opt_ptr(tab),
            _np_ptr(win) if win is not None else None, _np_ptr(strs),
            max_hdrs, _np_ptr(hdr_off), _np_ptr(rc), _np_ptr(kind),
            _np_ptr(sid), _np_ptr(hf), _np_ptr(did))
        del keep
        if ret not in (ERANGE, EINVAL):
            self._check(ret, "qhuff_scan_headers_tabs_host")
        n = min(int(hdr_off[-1]), max_hdrs)
        return (ret, strs[:32 * n], hdr_off, rc[:m], kind[:n], sid[:n],
                hf[:n], did[:n])

    def decode_headers_tabs_host(self, buf, sec_off, tables, sec_tab,
                                 sec_win=None, max_len=None, max_hdrs=None,
                                 hashes=False):
        """qhuff_decode_headers_tabs_host: scan and decode against a table
        per section in one call -> as decode_headers_dyn_host (EINVAL / ERANGE
        of the argument checks: the arrays after rc None)."""
        import numpy as np
        if max_hdrs is None:
            max_hdrs = int(self.scan_headers_tabs_host(
                buf, sec_off, tables, sec_tab, sec_win, 0)[2][-1])
        buf, sec_off, m, _, hdr_off, rc, kind, sid, hf = \
            _headers_host_args(buf, sec_off, max_hdrs)
        did = np.zeros(max(max_hdrs, 1), dtype=np.uint32)
        t, keep = dyn_tables_host(*(tables or ()))
        tab, win = _opt_u32(sec_tab), _sec_win_host(sec_win)
        wire = max(int(sec_off[-1]) - int(sec_off[0]), 0)
        out = np.zeros(decode_headers_dyn_bound(
            wire, max_hdrs, _tabs_longest(tables or ())), dtype=np.uint8)
        off = np.zeros(2 * max_hdrs + 1, dtype=np.uint32)
        status = np.zeros(max(2 * max_hdrs, 1), dtype=np.uint8)
        h1, h2 = (np.zeros(max(max_hdrs, 1), dtype=np.uint32)
                  for _ in range(2))
        ret = lib().qhuff_decode_headers_tabs_host(
            self._ctx, _np_ptr(buf) if len(buf) else None, _np_ptr(sec_off),
            m, C.byref(t), _opt_ptr(tab),
            _np_ptr(win) if win is not None else None, max_len or 0, max_hdrs,
            _np_ptr(hdr_off), _np_ptr(rc), _np_ptr(kind), _np_ptr(sid),
            _np_ptr(hf), _np_ptr(did), _np_ptr(out), _np_ptr(off),
            _np_ptr(status), _np_ptr(h1) if hashes else None,
            _np_ptr(h2) if hashes else None)
        del keep
        tail = (None,) * (9 if hashes else 7)
        if ret in (ERANGE, EINVAL):
            return (ret, hdr_off, rc[:m]) + tail
        self._check(ret, "qhuff_decode_headers_tabs_host")
        n = int(hdr_off[-1])
        res = (ret, hdr_off, rc[:m], kind[:n], sid[:n], hf[:n], did[:n],
               out[:off[2 * n]], off[:2 * n + 1], status[:2 * n])
        return res + ((h1[:n], h2[:n]) if hashes else ())

    def tabs_insert_host(self, tables, cap, max_cap, live_lo, buf, enc_off,
                         keep=None, max_ins=None):
        """qhuff_tabs_insert_host over host arrays -> as tabs_insert_cpu."""
        return _tabs_insert(lib().qhuff_tabs_insert_host, (self._ctx,),
                            "qhuff_tabs_insert_host", tables, cap, max_cap,
                            live_lo, buf, enc_off, keep, max_ins)

    def scan_inserts_tabs(self, tabs, state, buf, enc_off, scan, stream=None):
        """qhuff_scan_inserts_tabs: tabs a DynTables, state an InsState, scan
        an InsScan, all of device pointers; buf, enc_off device tensors."""
        r = lib().qhuff_scan_inserts_tabs(
            self._ctx, C.byref(tabs), C.byref(state), buf.data_ptr(),
            enc_off.data_ptr(), C.byref(scan), self._stream(stream))
        self._check(r, "qhuff_scan_inserts_tabs")

    def apply_inserts_tabs(self, tabs, state, buf, wire_bytes, keep, scan,
                           n_ins, out, stream=None):
        """qhuff_apply_inserts_tabs: as scan_inserts_tabs, keep a device
        tensor or None, out an InsOut of device pointers."""
        r = lib().qhuff_apply_inserts_tabs(
            self._ctx, C.byref(tabs), C.byref(state), buf.data_ptr(),
            wire_bytes, keep.data_ptr() if keep is not None else None,
            C.byref(scan), n_ins, C.byref(out), self._stream(stream))
        self._check(r, "qhuff_apply_inserts_tabs")

    def dyn_lookup_tabs_into(self, data, off, n, sec_hdr, m, tabs, sec_tab,
                             sec_win, name_hash, nameval_hash, kind,
                             static_id, dyn_id=None, stream=None):
        """qhuff_dyn_lookup_tabs on device tensors; tabs: a DynTables of
        device pointers.  The form of the arrays is the caller's duty."""
        opt = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        rc = lib().qhuff_dyn_lookup_tabs(
            self._ctx, data.data_ptr(), off.data_ptr(), n, sec_hdr.data_ptr(),
            m, C.byref(tabs), opt(sec_tab), opt(sec_win), opt(name_hash),
            opt(nameval_hash), kind.data_ptr(), static_id.data_ptr(),
            opt(dyn_id), self._stream(stream))
        self._check(rc, "qhuff_dyn_lookup_tabs")

    def dyn_lookup_tabs(self, data, off, sec_hdr, tabs, sec_tab, sec_win=None,
                        stream=None):
        """-> (name_hash, nameval_hash int32 [n] (uint32 bits), kind,
        static_id uint8 [n], dyn_id int32 [n] (uint32 bits))."""
        import torch
        n, m = (off.numel() - 1) // 2, sec_hdr.numel() - 1
        h1, h2, did = (torch.empty(max(n, 1), dtype=torch.int32,
                                   device=data.device) for _ in range(3))
        kind, sid = (torch.empty(max(n, 1), dtype=torch.uint8,
                                 device=data.device) for _ in range(2))
        self.dyn_lookup_tabs_into(data, off, n, sec_hdr, m, tabs, sec_tab,
                                  sec_win, h1, h2, kind, sid, did, stream)
        return h1[:n], h2[:n], kind[:n], sid[:n], did[:n]

    def dyn_lookup_tabs_host(self, data, off, sec_hdr, tables, sec_tab,
                             sec_win=None):
        """qhuff_dyn_lookup_tabs_host over host buffers -> as
        dyn_lookup_tabs_cpu."""
        import numpy as np
        data = np.ascontiguousarray(data, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint32)
        sec_hdr = np.ascontiguousarray(sec_hdr, dtype=np.uint32)
        n, m = (len(off) - 1) // 2, len(sec_hdr) - 1
        h1, h2, did = (np.zeros(max(n, 1), dtype=np.uint32) for _ in range(3))
        kind, sid = (np.zeros(max(n, 1), dtype=np.uint8) for _ in range(2))
        t, keep = dyn_tables_host(*(tables or ()))
        tab, win = _opt_u32(sec_tab), _sec_win_host(sec_win)
        ret = lib().qhuff_dyn_lookup_tabs_host(
            self._ctx, _np_ptr(data) if len(data) else None, _np_ptr(off), n,
            _np_ptr(sec_hdr), m, C.byref(t), _opt_ptr(tab), _opt_ptr(win),
            _np_ptr(h1), _np_ptr(h2), _np_ptr(kind), _np_ptr(sid),
            _np_ptr(did))
        del keep
        if ret not in (EINVAL, ERANGE):
            self._check(ret, "qhuff_dyn_lookup_tabs_host")
        return ret, h1[:n], h2[:n], kind[:n], sid[:n], did[:n]

    def encode_headers_tabs_into(self, data, off, n, hflags, sec_hdr, m, tabs,
                                 sec_tab, sec_win, sec_base, out, sec_out,
                                 kind=None, static_id=None, dyn_id=None,
                                 stream=None):
        """qhuff_encode_headers_tabs on device tensors; tabs: a DynTables of
        device pointers.  The form of the arrays is the caller's duty."""
        opt = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        rc = lib().qhuff_encode_headers_tabs(
            self._ctx, data.data_ptr(), off.data_ptr(), n, opt(hflags),
            sec_hdr.data_ptr(), m, C.byref(tabs), opt(sec_tab), opt(sec_win),
            opt(sec_base), out.data_ptr(), sec_out.data_ptr(), opt(kind),
            opt(static_id), opt(dyn_id), self._stream(stream))
        self._check(rc, "qhuff_encode_headers_tabs")

    def encode_headers_tabs(self, data, off, sec_hdr, tabs, sec_tab,
                            sec_win=None, sec_base=None, hflags=None,
                            stream=None):
        """-> (out uint8 [bound], sec_out int32 [m+1], kind, static_id uint8
        [n], dyn_id int32 [n])."""
        import torch
        n, m = (off.numel() - 1) // 2, sec_hdr.numel() - 1
        out = torch.empty(encode_headers_bound(int(data.numel()), n, m),
                          dtype=torch.uint8, device=data.device)
        sec_out = torch.empty(m + 1, dtype=torch.int32, device=data.device)
        kind, sid = (torch.empty(max(n, 1), dtype=torch.uint8,
                                 device=data.device) for _ in range(2))
        did = torch.empty(max(n, 1), dtype=torch.int32, device=data.device)
        self.encode_headers_tabs_into(data, off, n, hflags, sec_hdr, m, tabs,
                                      sec_tab, sec_win, sec_base, out,
                                      sec_out, kind, sid, did, stream)
        return out, sec_out, kind[:n], sid[:n], did[:n]

    def encode_headers_tabs_host(self, data, off, sec_hdr, tables, sec_tab,
                                 sec_win=None, sec_base=None, hflags=None):
        """qhuff_encode_headers_tabs_host over host buffers -> as
        encode_headers_dyn_host."""
        import numpy as np
        data = np.ascontiguousarray(data, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint32)
        sec_hdr = np.ascontiguousarray(sec_hdr, dtype=np.uint32)
        if hflags is not None:
            hflags = np.ascontiguousarray(hflags, dtype=np.uint8)
        n, m = (len(off) - 1) // 2, len(sec_hdr) - 1
        span = max(int(off[-1]) - int(off[0]), 0)
        out = np.zeros(encode_headers_bound(span, n, m), dtype=np.uint8)
        sec_out = np.zeros(m + 1, dtype=np.uint32)
        kind, sid = (np.zeros(max(n, 1), dtype=np.uint8) for _ in range(2))
        did = np.zeros(max(n, 1), dtype=np.uint32)
        t, keep = dyn_tables_host(*(tables or ()))
        tab, win = _opt_u32(sec_tab), _sec_win_host(sec_win)
        base = _opt_u32(sec_base)
        ret = lib().qhuff_encode_headers_tabs_host(
            self._ctx, _np_ptr(data) if len(data) else None, _np_ptr(off), n,
            _np_ptr(hflags) if hflags is not None and n else None,
            _np_ptr(sec_hdr), m, C.byref(t), _opt_ptr(tab), _opt_ptr(win),
            _opt_ptr(base), _np_ptr(out), _np_ptr(sec_out), _np_ptr(kind),
            _np_ptr(sid), _np_ptr(did))
        del keep
        if ret in (EINVAL, ERANGE):
            return ret, out[:0], sec_out, kind[:n], sid[:n], did[:n]
        self._check(ret, "qhuff_encode_headers_tabs_host")
        return ret, out[:sec_out[-1]], sec_out, kind[:n], sid[:n], did[:n]

    # host-memory batch calls (numpy) ----------------------------------------
    def encode_host(self, data, in_off, mode=ENC_PAYLOAD, out=None,
                    out_off=None):
        """Host buffers in and out (PCIe-inclusive path).  out / out_off may
        be given (reused, already faulted-in buffers of the bound size)."""
        import numpy as np
        data = np.ascontiguousarray(data, dtype=np.uint8)
        in_off = np.ascontiguousarray(in_off, dtype=np.uint32)
        n = len(in_off) - 1
        if out is None:
            out = np.zeros(encode_bound(int(in_off[-1] - in_off[0]), n, mode),
                           dtype=np.uint8)
        if out_off is None:
            out_off = np.zeros(n + 1, dtype=np.uint32)
        rc = lib().qhuff_encode_batch_host(self._ctx, _np_ptr(data),
                                           _np_ptr(in_off), n, mode,
                                           _np_ptr(out), _np_ptr(out_off))
        self._check(rc, "qhuff_encode_batch_host")
        return out[:out_off[-1]], out_off

    def decode_host(self, data, in_off, out=None, out_off=None, status=None):
        import numpy as np
        data = np.ascontiguousarray(data, dtype=np.uint8)
        in_off = np.ascontiguousarray(in_off, dtype=np.uint32)
        n = len(in_off) - 1
        if out is None:
            out = np.zeros(decode_bound(int(in_off[-1] - in_off[0]), n),
                           dtype=np.uint8)
        if out_off is None:
            out_off = np.zeros(n + 1, dtype=np.uint32)
        if status is None:
            status = np.zeros(max(n, 1), dtype=np.uint8)
        rc = lib().qhuff_decode_batch_host(self._ctx, _np_ptr(data),
                                           _np_ptr(in_off), n, _np_ptr(out),
                                           _np_ptr(out_off), _np_ptr(status))
        self._check(rc, "qhuff_decode_batch_host")
        return out[:out_off[-1]], out_off, status[:n]

    def decode_literals_host(self, buf, lits, max_len=None):
        """Decode pre-parsed literals of host buffer buf in one GPU batch ->
        (list of bytes, status uint8 ndarray).  max_len (e.g. MAX_STRLEN for
        field-section literals) calls qhuff_decode_literals_ex: a literal
        longer than it once decoded is an ERROR."""
        import numpy as np
        n = len(lits)
        arr = (Literal * max(n, 1))(*lits)
        src = np.frombuffer(bytes(buf) + b"\0", dtype=np.uint8)
        cap = int(lib().qhuff_literals_bound(arr, n))
        out = np.zeros(cap, dtype=np.uint8)
        out_off = np.zeros(n + 1, dtype=np.uint32)
        status = np.zeros(max(n, 1), dtype=np.uint8)
        if max_len is None:
            rc = lib().qhuff_decode_literals_host(
                self._ctx, _np_ptr(src), arr, n, _np_ptr(out), _np_ptr(out_off),
                _np_ptr(status))
        else:
            rc = lib().qhuff_decode_literals_ex(
                self._ctx, _np_ptr(src), arr, n, max_len, _np_ptr(out),
                _np_ptr(out_off), _np_ptr(status))
        self._check(rc, "qhuff_decode_literals_host")
        return ([out[out_off[i]:out_off[i + 1]].tobytes() for i in range(n)],
                status[:n])

    # literals decoded in place from wire data ------------------------------
    def decode_wire_into(self, buf, lits, n, max_len, out, out_off, status,
                         stream=None):
        """qhuff_decode_wire: buf the wire bytes, lits the n descriptors (16
        bytes each), all device tensors; the descriptors must satisfy the
        order rule (literals_check)."""
        rc = lib().qhuff_decode_wire(
            self._ctx, buf.data_ptr(), lits.data_ptr(), n, max_len or 0,
            out.data_ptr(), out_off.data_ptr(), status.data_ptr(),
            self._stream(stream))
        self._check(rc, "qhuff_decode_wire")

    def decode_wire(self, buf, lits, max_len=None, stream=None, bound=None):
        """buf: uint8 cuda tensor of wire bytes; lits: uint8 cuda tensor of
        16 * n bytes (literals_array of the scanners' Literals).  Returns
        (out uint8 [bound], out_off int32 [n+1], status uint8 [n]).  bound:
        qhuff_literals_bound of the descriptors when the caller has it (it
        is computed from a host copy of lits otherwise)."""
        import torch
        n = lits.numel() // 16
        if bound is None:
            bound = literals_bound(lits.cpu().numpy())
        out = torch.empty(bound, dtype=torch.uint8, device=buf.device)
        out_off = torch.empty(n + 1, dtype=torch.int32, device=buf.device)
        status = torch.empty(max(n, 1), dtype=torch.uint8, device=buf.device)
        self.decode_wire_into(buf, lits, n, max_len, out, out_off, status,
                              stream)
        return out, out_off, status[:n]

    def decode_wire_host(self, buf, lits, max_len=None):
        """qhuff_decode_wire_host over host buffer buf and [Literal] ->
        (list of bytes, status uint8 ndarray), as decode_literals_host."""
        import numpy as np
        n = len(lits)
        arr = (Literal * max(n, 1))(*lits)
        src = np.frombuffer(bytes(buf) + b"\0", dtype=np.uint8)
        cap = int(lib().qhuff_literals_bound(arr, n))
        out = np.zeros(cap, dtype=np.uint8)
        out_off = np.zeros(n + 1, dtype=np.uint32)
        status = np.zeros(max(n, 1), dtype=np.uint8)
        rc = lib().qhuff_decode_wire_host(
            self._ctx, _np_ptr(src), arr, n, max_len or 0, _np_ptr(out),
            _np_ptr(out_off), _np_ptr(status))
        self._check(rc, "qhuff_decode_wire_host")
        return ([out[out_off[i]:out_off[i + 1]].tobytes() for i in range(n)],
                status[:n])

    # field sections and encoder streams scanned on the device ---------------
    def scan_sections_into(self, buf, sec_off, m, mode, lits, max_lits,
                           lit_off, rc, consumed, stream=None):
        """qhuff_scan_sections: all device tensors (consumed may be None in
        field-section mode); lits holds 16 * max_lits bytes."""
        r = lib().qhuff_scan_sections(
            self._ctx, buf.data_ptr(), sec_off.data_ptr(), m, mode,
            lits.data_ptr() if lits is not None else None, max_lits,
            lit_off.data_ptr(), rc.data_ptr(),
            consumed.data_ptr() if consumed is not None else None,
            self._stream(stream))
        self._check(r, "qhuff_scan_sections")

    def scan_sections(self, buf, sec_off, mode=SCAN_FIELD_SECTION,
                      max_lits=None, stream=None):
        """buf: uint8 cuda tensor of wire bytes; sec_off: int32 cuda tensor
        [m+1].  Returns device tensors (lits uint8 [16 * max_lits], lit_off
        int32 [m+1], rc int32 [m], consumed int32 [m]); lit_off[m] is the
        full count, to be compared with max_lits.  max_lits None: a first
        scan with room for no descriptor counts them (it waits for that
        count: two scans and a synchronisation; a caller that knows a bound
        passes it)."""
        import torch
        m = sec_off.numel() - 1
        dev = buf.device
        if max_lits is None:
            lit_off = torch.empty(m + 1, dtype=torch.int32, device=dev)
            rc = torch.empty(max(m, 1), dtype=torch.int32, device=dev)
            consumed = torch.empty(max(m, 1), dtype=torch.int32, device=dev)
            self.scan_sections_into(buf, sec_off, m, mode, None, 0, lit_off,
                                    rc, consumed, stream)
            (stream or torch.cuda.current_stream()).synchronize()
            max_lits = int(lit_off[m].item()) & 0xFFFFFFFF
        lits = torch.empty(16 * max(max_lits, 1), dtype=torch.uint8, device=dev)
        lit_off = torch.empty(m + 1, dtype=torch.int32, device=dev)
        rc = torch.empty(max(m, 1), dtype=torch.int32, device=dev)
        consumed = torch.empty(max(m, 1), dtype=torch.int32, device=dev)
        self.scan_sections_into(buf, sec_off, m, mode, lits, max_lits,
                                lit_off, rc, consumed, stream)
        return lits, lit_off, rc[:m], consumed[:m]

    def scan_sections_host(self, buf, sec_off, mode=SCAN_FIELD_SECTION,
                           max_lits=None):
        """qhuff_scan_sections_host over host arrays -> (ret, lits, lit_off,
        rc, consumed) as scan_sections_cpu (max_lits None: a first call
        with room for none counts them)."""
        if max_lits is None:
            max_lits = int(self.scan_sections_host(buf, sec_off, mode,
                                                   0)[2][-1])
        buf, sec_off, m, max_lits, lits, lit_off, rc, consumed = \
            _sections_host_args(buf, sec_off, max_lits)
        ret = lib().qhuff_scan_sections_host(
            self._ctx, _np_ptr(buf) if len(buf) else None, _np_ptr(sec_off),
            m, mode, _np_ptr(lits), max_lits, _np_ptr(lit_off),
            _np_ptr(rc), _np_ptr(consumed))
        if ret != ERANGE:
            self._check(ret, "qhuff_scan_sections_host")
        n = min(int(lit_off[-1]), max_lits)
        return ret, lits[:16 * n], lit_off, rc[:m], consumed[:m]

    def decode_sections_host(self, buf, sec_off, mode=SCAN_FIELD_SECTION,
                             max_len=None, max_lits=None):
        """qhuff_decode_sections_host: scan and decode in one call -> (ret,
        lits, lit_off, rc, consumed, out, out_off, status); ret OK, or ERANGE
        (lit_off[-1] > max_lits: nothing decoded, the first max_lits
        descriptors, out / out_off / status None).  max_lits None:
        scan_sections_host counts the literals first (one more round trip;
        the context's stage grows with max_lits, so a caller passes the
        count or a bound near it, not a loose one)."""
        import numpy as np
        if max_lits is None:
            max_lits = int(self.scan_sections_host(buf, sec_off, mode,
                                                   0)[2][-1])
        buf, sec_off, m, max_lits, lits, lit_off, rc, consumed = \
            _sections_host_args(buf, sec_off, max_lits)
        wire = max(int(sec_off[-1]) - int(sec_off[0]), 0)
        out = np.zeros(decode_bound(wire, 0), dtype=np.uint8)
        out_off = np.zeros(max_lits + 1, dtype=np.uint32)
        status = np.zeros(max(max_lits, 1), dtype=np.uint8)
        ret = lib().qhuff_decode_sections_host(
            self._ctx, _np_ptr(buf) if len(buf) else None, _np_ptr(sec_off),
            m, mode, max_len or 0, _np_ptr(lits), max_lits, _np_ptr(lit_off),
            _np_ptr(rc), _np_ptr(consumed),
            _np_ptr(out), _np_ptr(out_off), _np_ptr(status))
        if ret == ERANGE:
            return (ret, lits[:16 * max_lits], lit_off, rc[:m], consumed[:m],
                    None, None, None)
        self._check(ret, "qhuff_decode_sections_host")
        n = int(lit_off[-1])
        return (ret, lits[:16 * n], lit_off, rc[:m], consumed[:m],
                out[:out_off[n]], out_off[:n + 1], status[:n])

    # field lines and instructions encoded in one launch ---------------------
    def encode_wire_into(self, data, in_off, items, n, out, out_off,
                         stream=None):
        """qhuff_encode_wire: data the strings, in_off their n + 1 offsets,
        items the n items (8 bytes each), all device tensors; the items must
        satisfy the item rule (items_check)."""
        rc = lib().qhuff_encode_wire(
            self._ctx, data.data_ptr(), in_off.data_ptr(), items.data_ptr(),
            n, out.data_ptr(), out_off.data_ptr(), self._stream(stream))
        self._check(rc, "qhuff_encode_wire")

    def encode_wire(self, data, in_off, items, stream=None):
        """data: uint8 cuda tensor; in_off: int32 cuda tensor [n+1]; items:
        uint8 cuda tensor of 8 * n bytes (items_array of [Item]).  Returns
        (out uint8 [bound], out_off int32 [n+1])."""
        import torch
        n = in_off.numel() - 1
        out = torch.empty(encode_wire_bound(int(data.numel()), n),
                          dtype=torch.uint8, device=data.device)
        out_off = torch.empty(n + 1, dtype=torch.int32, device=data.device)
        self.encode_wire_into(data, in_off, items, n, out, out_off, stream)
        return out, out_off

    def encode_wire_host(self, data, in_off, items):
        """qhuff_encode_wire_host over host buffers and [Item] (or their
        uint8 array) -> (out uint8 ndarray [out_off[n]], out_off uint32
        [n+1])."""
        import numpy as np
        data = np.ascontiguousarray(data, dtype=np.uint8)
        in_off = np.ascontiguousarray(in_off, dtype=np.uint32)
        a = items if isinstance(items, np.ndarray) else items_array(items)
        a = np.ascontiguousarray(a, dtype=np.uint8)
        n = len(in_off) - 1
        out = np.zeros(encode_wire_bound(int(in_off[-1] - in_off[0]), n),
                       dtype=np.uint8)
        out_off = np.zeros(n + 1, dtype=np.uint32)
        rc = lib().qhuff_encode_wire_host(
            self._ctx, _np_ptr(data), _np_ptr(in_off),
            _np_ptr(a) if len(a) else None, n, _np_ptr(out), _np_ptr(out_off))
        self._check(rc, "qhuff_encode_wire_host")
        return out[:out_off[-1]], out_off

    def service(self, slots=0, idle_us=0):
        """Attach the low-latency service (qhuff_svc_open) -> Service."""
        self._service = Service(self, slots, idle_us)
        return self._service

    # per-string mirrors of the reference entry points ----------------------
    def enc_enc_str(self, prefix_bits, s, first_byte=0, dst_len=1 << 20):
        buf = C.create_string_buffer(max(dst_len, 1))
        buf[0] = first_byte
        r = lib().qhuff_enc_enc_str(self._ctx, prefix_bits, buf, dst_len, s,
                                    len(s))
        return r if r < 0 else buf.raw[:r]

    def enc_str_size(self, s):
        return int(lib().qhuff_enc_str_size(self._ctx, s, len(s)))

    def huff_decode(self, src, dst_len=None, state=None, final=1):
        """qhuff_huff_decode_ex (lsqpack_huff_decode's arguments on this
        context) -> (status, dst bytes [:n_dst], n_src)."""
        if dst_len is None:
            dst_len = len(src) * 8 // 5 + 1
        s = C.create_string_buffer(bytes(src), len(src) + 1)
        d = C.create_string_buffer(max(dst_len, 1))
        st = state if state is not None else DecodeState(0, 0, 0)
        rv = lib().qhuff_huff_decode_ex(self._ctx, s, len(src), d, dst_len,
                                        C.byref(st), final)
        return rv.status, d.raw[:rv.n_dst], rv.n_src


class Service:
    """The resident low-latency service on a Codec's context (qhuff_svc_*):
    small host-memory batches without a kernel launch per call.  While it is
    open, the context's own host-path calls that fit a slot use it too."""

    def __init__(self, codec, slots=0, idle_us=0):
        self.codec = codec                   # keeps the context alive
        self._svc = C.c_void_p()
        rc = lib().qhuff_svc_open(codec._ctx, slots, idle_us,
                                  C.byref(self._svc))
        if rc != OK:
            err = lib().qhuff_last_error(codec._ctx)
            raise QhuffError("qhuff_svc_open failed: %d (%s)" % (
                rc, err.decode() if err else ""))

    def close(self):
        if self._svc:
            lib().qhuff_svc_close(self._svc)
            self._svc = C.c_void_p()
        if getattr(self.codec, "_service", None) is self:
            self.codec._service = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc, what):
        if rc != OK:
            err = lib().qhuff_last_error(self.codec._ctx)
            raise QhuffError("%s failed: %d (%s)" % (what, rc,
                             err.decode() if err else ""))

    def stats(self):
        """(calls served by the kernel, kernel launches, calls sent to the
        host path)"""
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(lib().qhuff_svc_stats(self._svc, C.byref(a), C.byref(b),
                                          C.byref(c)), "qhuff_svc_stats")
        return a.value, b.value, c.value

    def encode(self, data, in_off, mode=ENC_PAYLOAD, out=None, out_off=None):
        import numpy as np
        data = np.ascontiguousarray(data, dtype=np.uint8)
        in_off = np.ascontiguousarray(in_off, dtype=np.uint32)
        n = len(in_off) - 1
        if out is None:
            out = np.zeros(encode_bound(int(in_off[-1] - in_off[0]), n, mode),
                           dtype=np.uint8)
        if out_off is None:
            out_off = np.zeros(n + 1, dtype=np.uint32)
        self._check(lib().qhuff_svc_encode(self._svc, _np_ptr(data),
                                           _np_ptr(in_off), n, mode,
                                           _np_ptr(out), _np_ptr(out_off)),
                    "qhuff_svc_encode")
        return out[:out_off[-1]], out_off

    def decode(self, data, in_off, out=None, out_off=None, status=None):
        import numpy as np
        data = np.ascontiguousarray(data, dtype=np.uint8)
        in_off = np.ascontiguousarray(in_off, dtype=np.uint32)
        n = len(in_off) - 1
        if out is None:
            out = np.zeros(decode_bound(int(in_off[-1] - in_off[0]), n),
                           dtype=np.uint8)
        if out_off is None:
            out_off = np.zeros(n + 1, dtype=np.uint32)
        if status is None:
            status = np.zeros(max(n, 1), dtype=np.uint8)
        self._check(lib().qhuff_svc_decode(self._svc, _np_ptr(data),
                                           _np_ptr(in_off), n, _np_ptr(out),
                                           _np_ptr(out_off), _np_ptr(status)),
                    "qhuff_svc_decode")
        return out[:out_off[-1]], out_off, status[:n]
