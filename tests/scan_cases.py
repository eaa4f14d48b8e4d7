"""Cases and expected values of the device scan (qhuff_scan_sections and its
host, composite and CPU forms), shared by tests/test_scan_device.py's CPU and
GPU halves.

A case is (mode, [chunk bytes]).  The expected outputs come from the Python
restatement of the reference's framing rules (qpack_frames.ref_scan_*), per
chunk, with positions moved to where the chunk lies in the batch; the host
scanners (qhuff_scan_field_section / qhuff_scan_encoder_stream) are checked
against the same model on every distinct chunk.  Nothing here runs the code
under test."""
import functools
import glob
import json
import os
import random

import numpy as np

import _paths  # noqa: F401
import qhuff
import qpack_frames as Q

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIELD, STREAM = qhuff.SCAN_FIELD_SECTION, qhuff.SCAN_ENCODER_STREAM
RC = {"ok": qhuff.OK, "trunc": qhuff.ETRUNC, "proto": qhuff.EPROTO}
STREAMS = ("netbsd", "fb-req", "fb-resp")

# struct qhuff_literal
LIT = np.dtype([("pos", "<u4"), ("len", "<u4"), ("huffman", "u1"),
                ("prefix_bits", "u1"), ("kind", "u1"), ("hdr_len", "u1"),
                ("instr", "<u4")])
assert LIT.itemsize == 16

# qhuff_kernels.h kScanBlock (chunks a workgroup of the count and write
# launches) and kScanTop (workgroup totals a round of the top launch)
SCAN_BLOCK = 256
SCAN_TOP = 1024


def _read(rel):
    with open(os.path.join(G, rel), "rb") as f:
        return f.read()


# ---- the model -------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def model(mode, chunk):
    """-> (rc, consumed, LIT array with positions relative to the chunk);
    the host scanner of that mode agrees (checked here, once a chunk)."""
    if mode == FIELD:
        st, spans = Q.ref_scan_field_section(chunk)
        used = len(chunk) if st == "ok" else 0
        rc, hl = qhuff.scan_field_section(chunk, 7)
        hused = used
    else:
        st, spans, used = Q.ref_scan_encoder_stream(chunk)
        rc, hl, hused = qhuff.scan_encoder_stream(chunk, 7)
    a = np.zeros(len(spans), dtype=LIT)
    for k, (pos, ln, h, pb, hdr, kind, instr) in enumerate(spans):
        a[k] = (pos, ln, h, pb, kind, hdr, instr)
    assert rc == RC[st] and (rc != qhuff.OK or hused == used)
    assert [(l.pos - 7, l.len, l.huffman, l.prefix_bits, l.hdr_len, l.kind,
             l.instr - 7) for l in (hl if rc == qhuff.OK else [])] == spans
    return RC[st], used, a


class Expect:
    """the five outputs for chunks packed back to back from offset a0"""

    def __init__(self, mode, chunks, a0=0):
        m = len(chunks)
        self.mode, self.m, self.a0 = mode, m, a0
        self.sec_off = np.zeros(m + 1, dtype=np.uint32)
        self.sec_off[0] = a0
        if m:
            np.cumsum([len(c) for c in chunks], out=self.sec_off[1:])
            self.sec_off[1:] += np.uint32(a0)
        self.rc = np.zeros(m, dtype=np.int32)
        self.consumed = np.zeros(m, dtype=np.uint32)
        self.lit_off = np.zeros(m + 1, dtype=np.uint32)
        parts = []
        for i, c in enumerate(chunks):
            rc, used, a = model(mode, c)
            self.rc[i], self.consumed[i] = rc, used
            self.lit_off[i + 1] = self.lit_off[i] + len(a)
            if len(a):
                a = a.copy()
                a["pos"] += self.sec_off[i]
                a["instr"] += self.sec_off[i]
                parts.append(a)
        self.lits = (np.concatenate(parts) if parts
                     else np.zeros(0, dtype=LIT))
        self.total = int(self.lit_off[-1])
        assert self.total == len(self.lits)
        self.wire = b"".join(chunks)

    def lit_bytes(self, max_lits=None):
        n = self.total if max_lits is None else min(self.total, max_lits)
        return self.lits[:n].view(np.uint8).reshape(-1)


# ---- 1. reference data -----------------------------------------------------

@functools.lru_cache(maxsize=None)
def interop_frames():
    out = []
    for name in STREAMS:
        out += list(Q.read_interop(_read("data/%s.out.256.100.1" % name)))
    return out


def interop_sections():
    return FIELD, [p for sid, p in interop_frames() if sid != 0]


def interop_encoder():
    return STREAM, [p for sid, p in interop_frames() if sid == 0]


@functools.lru_cache(maxsize=None)
def fuzz_payloads():
    out = []
    for f in sorted(glob.glob(os.path.join(G, "data", "fuzz", "*", "*"))):
        out += [p for _, p in Q.fuzz_records(_read(f), strict=False)]
    return out


def fuzz_as_sections():
    return FIELD, fuzz_payloads()


def fuzz_as_encoder():
    return STREAM, fuzz_payloads()


def kat_blocks():
    hb = json.loads(_read("kat_header_blocks.json"))["header_blocks"]
    return FIELD, [bytes.fromhex(k["prefix"] + k["header"]) for k in hb]


def kat_encoder():
    hb = json.loads(_read("kat_header_blocks.json"))["header_blocks"]
    es = json.loads(_read("kat_enc_stream.json"))["enc_stream"]
    return STREAM, ([bytes.fromhex(k["enc"]) for k in hb]
                    + [bytes.fromhex(k["enc_stream"]) for k in es])


# ---- 2. every prefix -------------------------------------------------------

def lit(first, prefix_bits, payload, huffman=0):
    """a string literal as it is framed: H above an N-bit length"""
    return Q.enc_int(first | (huffman << prefix_bits), len(payload),
                     prefix_bits) + bytes(payload)


def all_forms_section():
    """one section with the five field-line forms, each with one-byte and
    multi-byte integers; a multi-byte Required Insert Count, a one-byte
    Delta Base"""
    s = Q.enc_int(0, 300, 8) + Q.enc_int(0x80, 5, 7)
    s += Q.enc_int(0xC0, 1, 6) + Q.enc_int(0x80, 1000, 6)            # indexed
    s += Q.enc_int(0x50, 3, 4) + lit(0, 7, b"abc")                   # name ref
    s += Q.enc_int(0x60, 300, 4) + lit(0, 7, bytes(range(130)), 1)
    s += lit(0x20, 3, b"xy", 1) + lit(0, 7, b"value")                # lit name
    s += lit(0x30, 3, b"long-name") + lit(0, 7, bytes(200), 1)
    s += Q.enc_int(0x10, 1, 4) + Q.enc_int(0x10, 20, 4)              # post-base
    s += Q.enc_int(0x00, 2, 3) + lit(0, 7, b"v")                     # pb name ref
    s += Q.enc_int(0x08, 40, 3) + lit(0, 7, b"")
    assert Q.ref_scan_field_section(s)[0] == "ok"
    assert len(Q.ref_scan_field_section(s)[1]) == 8
    return s


def all_forms_stream():
    s = Q.enc_int(0xC0, 1, 6) + lit(0, 7, b"abc")              # name ref
    s += Q.enc_int(0x80, 700, 6) + lit(0, 7, bytes(140), 1)
    s += lit(0x40, 5, b"nm", 1) + lit(0, 7, b"value")          # literal name
    s += lit(0x40, 5, bytes(40)) + lit(0, 7, bytes(129))
    s += Q.enc_int(0x20, 4, 5) + Q.enc_int(0x20, 4096, 5)      # capacity
    s += Q.enc_int(0x00, 2, 5) + Q.enc_int(0x00, 31, 5)        # duplicate
    st, lits, used = Q.ref_scan_encoder_stream(s)
    assert (st, len(lits), used) == ("ok", 6, len(s))
    return s


def prefixes(s):
    return [s[:k] for k in range(len(s) + 1)]


def every_prefix_sections():
    return FIELD, prefixes(all_forms_section())


def every_prefix_stream():
    return STREAM, prefixes(all_forms_stream())


# ---- 3. integer edges ------------------------------------------------------

def _kat_conts():
    """the continuation bytes of the kat_int vectors whose prefix saturates
    (a vector with a small value has none: it is its prefix alone)"""
    k = json.loads(_read("kat_int.json"))
    vec = list(k["dec_int"]) + [k["overlong_full_buffer"]]
    out = []
    for v in vec:
        e, pmax = bytes.fromhex(v["encoded"]), (1 << v["prefix_bits"]) - 1
        out.append(e[1:] if e[0] & pmax == pmax else None)
    assert any(c is not None and len(c) == 10 for c in out)    # M == 70
    return out


def kat_int_sections():
    """every vector as Required Insert Count and as Delta Base, and every
    strict prefix of each placement"""
    ch = []
    for c in _kat_conts():
        if c is None:
            ch += [bytes([5, 3]), bytes([5, 3, 0xC1])]
            continue
        ch += prefixes(bytes([0xFF]) + c + bytes([0x00, 0xC1]))
        ch += prefixes(bytes([0x00, 0xFF]) + c + bytes([0xC1]))
    return FIELD, ch


def kat_int_stream():
    ch = []
    for c in _kat_conts():
        if c is None:
            ch.append(bytes([0x25]))
            continue
        ch += prefixes(bytes([0x3F]) + c + bytes([0x02]))
    return STREAM, ch


V_OK, V_BAD = (1 << 24) - 1, 1 << 24


def int24_sections():
    """indices on prefix widths 6, 4, 4, 3 and lengths on 7 and 3, at
    2^24 - 1 and 2^24 (lengths without their bytes: the clamp, then 2^24)"""
    ch = []
    for v in (V_OK, V_BAD):
        ch.append(b"\0\0" + Q.enc_int(0x80, v, 6))
        ch.append(b"\0\0" + Q.enc_int(0x40, v, 4) + lit(0, 7, b"a"))
        ch.append(b"\0\0" + Q.enc_int(0x10, v, 4))
        ch.append(b"\0\0" + Q.enc_int(0x00, v, 3) + lit(0, 7, b"a"))
        ch.append(b"\0\0" + Q.enc_int(0x50, 1, 4) + Q.enc_int(0, v, 7))
        ch.append(b"\0\0" + Q.enc_int(0x20, v, 3))
    want = [qhuff.OK] * 4 + [qhuff.EPROTO] * 8
    assert [model(FIELD, c)[0] for c in ch] == want
    return FIELD, ch


def int24_stream():
    """indices on 6 and 5, lengths on 5 and 7; a 2^24 - 1 length once with
    its bytes (OK) and once without (a partial instruction)"""
    ch = []
    for v in (V_OK, V_BAD):
        ch.append(Q.enc_int(0x80, v, 6) + lit(0, 7, b"a"))
        ch.append(Q.enc_int(0x00, v, 5))
        ch.append(b"\x22" + Q.enc_int(0x40, v, 5))
        ch.append(b"\x22" + Q.enc_int(0xC0, 1, 6) + Q.enc_int(0, v, 7))
    body = bytes(V_OK)
    ch.append(b"\x22" + Q.enc_int(0x40, V_OK, 5) + body + lit(0, 7, b"v")
              + b"\x03")
    ch.append(b"\x22" + Q.enc_int(0xC0, 1, 6) + Q.enc_int(0x80, V_OK, 7)
              + body + b"\x03")
    want = [(qhuff.OK, len(ch[0])), (qhuff.OK, len(ch[1])), (qhuff.OK, 1),
            (qhuff.OK, 1)] + [(qhuff.EPROTO, 0)] * 4
    assert [model(STREAM, c)[:2] for c in ch[:8]] == want
    assert all(model(STREAM, c)[:2] == (qhuff.OK, len(c)) for c in ch[8:])
    return STREAM, ch


def _padded_len(first, prefix_bits, n, pad):
    """length n >= 2^N - 1 with `pad` continuation bytes of 0x80 put before
    its last byte (a non-minimal integer the reference accepts)"""
    e = bytearray(Q.enc_int(first, n, prefix_bits))
    assert len(e) >= 2
    e[-1] |= 0x80
    return bytes(e) + b"\x80" * (pad - 1) + b"\x00"


def nonminimal_sections():
    ch = []
    for pad in (1, 2, 5, 8):
        ch.append(b"\0\0\x51" + _padded_len(0, 7, 130, pad) + bytes(130))
        ch.append(b"\0\0" + _padded_len(0x20, 3, 9, pad) + bytes(9)
                  + lit(0, 7, b"v"))
        ch.append(b"\0\0" + Q.enc_int(0x80, 63, 6)[:1]
                  + b"\x80" * pad + b"\x00")
    assert all(model(FIELD, c)[0] == qhuff.OK for c in ch)
    return FIELD, ch


def nonminimal_stream():
    ch = []
    for pad in (1, 2, 5, 8):
        ch.append(b"\xC1" + _padded_len(0, 7, 130, pad) + bytes(130))
        ch.append(_padded_len(0x40, 5, 40, pad) + bytes(40) + lit(0, 7, b"v"))
    assert all(model(STREAM, c)[:2] == (qhuff.OK, len(c)) for c in ch)
    return STREAM, ch


def _declared(mode):
    ch = []
    for n in (65535, 65536):
        for have in (n, n - 1, 0):
            if mode == FIELD:
                ch.append(b"\0\0\x51" + Q.enc_int(0, n, 7) + bytes(have))
                ch.append(b"\0\0" + Q.enc_int(0x20, n, 3) + bytes(have)
                          + (lit(0, 7, b"v") if have == n else b""))
            else:
                ch.append(b"\x22\xC1" + Q.enc_int(0, n, 7) + bytes(have))
                ch.append(b"\x22" + Q.enc_int(0x40, n, 5) + bytes(have)
                          + (lit(0, 7, b"v") if have == n else b""))
    return ch


def declared_sections():
    ch = _declared(FIELD)
    # the clamp goes before the look for the payload
    assert [model(FIELD, c)[0] for c in ch] == \
        [qhuff.OK] * 2 + [qhuff.ETRUNC] * 4 + [qhuff.EPROTO] * 6
    return FIELD, ch


def declared_stream():
    ch = _declared(STREAM)
    assert [model(STREAM, c)[1] for c in ch] == \
        [len(ch[0]), len(ch[1]), 1, 1, 1, 1, len(ch[6]), len(ch[7]), 1, 1, 1, 1]
    return STREAM, ch


def alloc_clamp():
    k = json.loads(_read("kat_header_alloc_clamp.json"))
    ch = [bytes.fromhex(c["block"]) for c in k["cases"]]
    assert [model(FIELD, c)[0] for c in ch] == [qhuff.EPROTO] * len(ch)
    return FIELD, ch


# ---- 5. counts -------------------------------------------------------------

SHORT = (b"\0\0", b"\0\0\xC1", b"\0\0\x51\x01a", b"\0\0\x20\x00", b"",
         b"\0\0\x51\x05abc", b"\0\0\xFF", b"\0\0\x23ab\x81\xFF", b"\0")


def counted(m, seed=3):
    """m short sections in a seeded order: OK ones with 0, 1 and 2 literals,
    truncated ones, an empty chunk"""
    rng = random.Random(seed * 1000003 + m)
    return FIELD, [SHORT[rng.randrange(len(SHORT))] for _ in range(m)]


COUNTS = (0, 1, 63, 64, 65, SCAN_BLOCK - 1, SCAN_BLOCK, SCAN_BLOCK + 1,
          2 * SCAN_BLOCK + 1, SCAN_BLOCK * SCAN_TOP - 1,
          SCAN_BLOCK * SCAN_TOP, SCAN_BLOCK * SCAN_TOP + 1,
          SCAN_BLOCK * (SCAN_TOP + 1) + 1)


def five_byte_sections():
    five = (b"\0\0\x51\x01a", b"\0\0\x20\x00\x00", b"\0\0\xFF\x01\xC2",
            b"\0\0\x51\x02a", b"\x01\x80\x23ab")
    rng = random.Random(11)
    ch = [five[rng.randrange(len(five))] for _ in range(70000)]
    assert sum(map(len, ch)) == 350000
    return FIELD, ch


def skewed():
    """one chunk of 40 KB of `20 00` pairs (a literal name and a value, both
    empty: 40,960 literals from one lane) between empty and index-only
    chunks"""
    big = b"\0\0" + b"\x20\x00" * 20480
    assert len(model(FIELD, big)[2]) == 40960
    ch = [b"", b"\0\0\xC1", b"\0\0"] * 20
    ch[31:31] = [big]
    return FIELD, ch + [b"\0\0\x51\x01a"]


# ---- 7. long chunks --------------------------------------------------------

def long_stream():
    rng = random.Random(23)
    parts, size = [], 0
    while size < 200 * 1024:
        k = rng.randrange(4)
        if k == 0:
            s = Q.enc_int(0xC0, rng.randrange(99), 6) \
                + lit(0, 7, bytes(rng.randrange(300)), rng.randrange(2))
        elif k == 1:
            s = lit(0x40, 5, bytes(rng.randrange(60)), rng.randrange(2)) \
                + lit(0, 7, bytes(rng.randrange(2000)), rng.randrange(2))
        elif k == 2:
            s = Q.enc_int(0x20, rng.randrange(1 << 20), 5)
        else:
            s = Q.enc_int(0x00, rng.randrange(5000), 5)
        parts.append(s)
        size += len(s)
    _, short = counted(63, 29)
    return STREAM, short[:30] + [b"".join(parts)] + short[30:]


def long_value():
    sec = b"\0\0\x51" + Q.enc_int(0, 65535, 7) + bytes(65535) \
        + lit(0x20, 3, b"n") + lit(0, 7, b"after")
    assert len(model(FIELD, sec)[2]) == 3
    _, short = counted(63, 31)
    return FIELD, short[:17] + [sec] + short[17:]


# ---- havoc (the stand-alone program's and the CPU tests' extra input) ------

def havoc(chunks, n, seed):
    rng = random.Random(seed)
    base = [c for c in chunks if c]
    out = []
    for _ in range(n):
        b = bytearray(base[rng.randrange(len(base))])
        for _ in range(rng.randrange(1, 4)):
            if not b:
                break
            op, j = rng.randrange(4), rng.randrange(len(b))
            if op == 0:
                b[j] ^= 1 << rng.randrange(8)
            elif op == 1:
                b[j] = rng.choice((0x00, 0x7F, 0x80, 0xFF, rng.randrange(256)))
            elif op == 2:
                del b[j:]
            else:
                b[j:j] = bytes(rng.randrange(256)
                               for _ in range(rng.randrange(1, 12)))
        out.append(bytes(b))
    return out


def havoc_sections():
    return FIELD, havoc(interop_sections()[1] + fuzz_payloads(), 1500, 41)


def havoc_stream():
    return STREAM, havoc(interop_encoder()[1] + fuzz_payloads(), 1500, 43)


# every case both halves run, by name
CASES = {
    "interop_sections": interop_sections, "interop_encoder": interop_encoder,
    "fuzz_as_sections": fuzz_as_sections, "fuzz_as_encoder": fuzz_as_encoder,
    "kat_blocks": kat_blocks, "kat_encoder": kat_encoder,
    "every_prefix_sections": every_prefix_sections,
    "every_prefix_stream": every_prefix_stream,
    "kat_int_sections": kat_int_sections, "kat_int_stream": kat_int_stream,
    "int24_sections": int24_sections, "int24_stream": int24_stream,
    "nonminimal_sections": nonminimal_sections,
    "nonminimal_stream": nonminimal_stream,
    "declared_sections": declared_sections, "declared_stream": declared_stream,
    "alloc_clamp": alloc_clamp,
    "five_byte_sections": five_byte_sections, "skewed": skewed,
    "long_stream": long_stream, "long_value": long_value,
    "havoc_sections": havoc_sections, "havoc_stream": havoc_stream,
}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> Expect of CASES[name] / of "count<m>", packed from offset 0"""
    if name.startswith("count"):
        mode, chunks = counted(int(name[5:]))
    else:
        mode, chunks = CASES[name]()
    return Expect(mode, chunks)
