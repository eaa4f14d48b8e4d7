"""The model of qhuff_scan_headers / qhuff_decode_headers: the header list a
field section decodes to when it does not use the dynamic table.

Nothing here comes from the library.  A section's framing verdict is
qpack_frames.ref_scan_field_section's (the reference's integer and length
rules); its lines are then dispatched as parse_header_data does
(lsqpack.c:3567-3915): an indexed line names a static entry
(header_out_static_entry, 3013-3057), a name reference a static name
(header_out_begin_static_nameref, 3121-3159), a literal line two literals
(3211-3323).  The static table is tests/golden/qpack_static_table.json, the
payloads go through the CPU oracle's Huffman decoder (oracle_lib), and the
length limit is header_out_grow_buf's (3346-3351).

The result code of a section, in this order:
  1. the framing verdict when it is not ok (ETRUNC / EPROTO);
  2. ENOTSUP: Required Insert Count != 0, or any line a dynamic form
     (indexed with T = 0, name reference with T = 0, indexed post-base,
     post-base name reference);
  3. EPROTO: a static index >= 99 (lsqpack.c:3021, 3130);
  4. OK.
A section that is not OK has no headers."""
import functools
import json
import os

import numpy as np

import _paths  # noqa: F401
import oracle_lib as O
import qpack_frames as Q

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

OK, ETRUNC, EPROTO, ENOTSUP = 0, -61, -71, -95
INDEXED, NAMEREF, LITERAL = 0, 1, 2      # QHUFF_LINE_*
NONE = 0xFF                              # QHUFF_STATIC_NONE
WIRE, STATIC_SRC = 0, 1                  # QHUFF_HSTR_*
NAME, VALUE = 1, 2                       # QHUFF_LIT_*
DEC_OK, DEC_ERROR = 0, 1
MAX_STRLEN = 65535

with open(os.path.join(G, "qpack_static_table.json")) as f:
    STATIC = [(n.encode("latin-1"), v.encode("latin-1"))
              for n, v in json.load(f)["static_table"]]
assert len(STATIC) == 99
assert max(len(n) + len(v) for n, v in STATIC) == 76    # the bound's 76
assert max(len(n) for n, _ in STATIC) == 32
assert max(len(v) for _, v in STATIC) == 53

# struct qhuff_hstr
HSTR = np.dtype([("pos", "<u4"), ("len", "<u4"), ("huffman", "u1"),
                 ("source", "u1"), ("kind", "u1"), ("static_id", "u1"),
                 ("instr", "<u4")])
assert HSTR.itemsize == 16


def bound(wire_bytes, n):
    """qhuff_decode_headers_bound (include/qhuff.h)"""
    return 8 * wire_bytes // 5 + 76 * n + 16


class Line:
    """one header line: kind, static id (NONE for LITERAL), N bit, the offset
    of its first byte, and its literals (pos, len, huffman) or None"""
    __slots__ = ("kind", "id", "never", "at", "name", "value")

    def __init__(self, kind, sid, never, at, name, value):
        self.kind, self.id, self.never, self.at = kind, sid, never, at
        self.name, self.value = name, value


def section(buf):
    """-> (rc, [Line]) of one field section; positions relative to buf"""
    return _section(bytes(buf))


@functools.lru_cache(maxsize=None)
def _section(buf):
    st, _ = Q.ref_scan_field_section(buf)
    if st != "ok":
        return (ETRUNC if st == "trunc" else EPROTO), []
    ric, pos = Q.dec_int(buf, 0, 8)
    _, pos = Q.dec_int(buf, pos, 7)          # Delta Base: read and ignored
    notsup, bad_id, lines = ric != 0, False, []

    def span(l):
        return (l[0], l[1], l[2])

    while pos < len(buf):
        b, at = buf[pos], pos
        if b & 0x80:                         # 1T indexed
            idx, pos = Q.dec_int24(buf, pos, 6)
            if not b & 0x40:
                notsup = True
            elif idx >= 99:
                bad_id = True
            else:
                lines.append(Line(INDEXED, idx, 0, at, None, None))
        elif b & 0x40:                       # 01NT name reference
            idx, pos = Q.dec_int24(buf, pos, 4)
            v, pos = Q._lit(buf, pos, 7, VALUE, at, MAX_STRLEN)
            if not b & 0x10:
                notsup = True
            elif idx >= 99:
                bad_id = True
            else:
                lines.append(Line(NAMEREF, idx, b >> 5 & 1, at, None, span(v)))
        elif b & 0x20:                       # 001N literal name
            n, pos = Q._lit(buf, pos, 3, NAME, at, MAX_STRLEN)
            v, pos = Q._lit(buf, pos, 7, VALUE, at, MAX_STRLEN)
            lines.append(Line(LITERAL, NONE, b >> 4 & 1, at, span(n), span(v)))
        elif b & 0x10:                       # 0001 indexed post-base
            _, pos = Q.dec_int24(buf, pos, 4)
            notsup = True
        else:                                # 0000N post-base name reference
            _, pos = Q.dec_int24(buf, pos, 3)
            _, pos = Q._lit(buf, pos, 7, VALUE, at, MAX_STRLEN)
            notsup = True
    if notsup:
        return ENOTSUP, []
    if bad_id:
        return EPROTO, []
    return OK, lines


def _payloads(wire, lits):
    """the decoded bytes and statuses of literals [(pos, len, huffman)]: the
    Huffman ones through the oracle in one batch"""
    hs = [wire[p:p + n] for p, n, h in lits if h]
    off = np.zeros(len(hs) + 1, dtype=np.uint32)
    np.cumsum([len(x) for x in hs], out=off[1:])
    data = np.frombuffer(b"".join(hs) + bytes(16), dtype=np.uint8)
    out, oo, st = O.decode_batch(data, off) if hs else (None, None, None)
    res, k = [], 0
    for p, n, h in lits:
        if not h:
            res.append((wire[p:p + n], DEC_OK))
            continue
        bad = bool(st[k])
        res.append((b"" if bad else out[oo[k]:oo[k + 1]].tobytes(),
                    DEC_ERROR if bad else DEC_OK))
        k += 1
    return res


class Decoded:
    """sections (each bytes) packed back to back from offset a0 -> every
    output of the scan and of the decode (max_len 0: no limit)"""

    def __init__(self, sections, max_len=MAX_STRLEN, a0=0):
        sections = [bytes(s) for s in sections]
        m = len(sections)
        self.m, self.a0 = m, a0
        self.wire = b"".join(sections)
        self.sec_off = np.zeros(m + 1, dtype=np.uint32)
        self.sec_off[0] = a0
        if m:
            np.cumsum([len(s) for s in sections], out=self.sec_off[1:])
            self.sec_off[1:] += np.uint32(a0)
        self.rc = np.zeros(m, dtype=np.int32)
        self.hdr_off = np.zeros(m + 1, dtype=np.uint32)
        lines = []
        for i, s in enumerate(sections):
            rc, ls = section(s)
            self.rc[i] = rc
            self.hdr_off[i + 1] = self.hdr_off[i] + len(ls)
            base = int(self.sec_off[i])
            for l in ls:
                mv = lambda x: None if x is None else (x[0] + base, x[1], x[2])  # noqa: E731
                lines.append(Line(l.kind, l.id, l.never, l.at + base,
                                  mv(l.name), mv(l.value)))
        self.lines = lines
        n = self.n = len(lines)
        self.kind = np.array([l.kind for l in lines], dtype=np.uint8)
        self.static_id = np.array([l.id for l in lines], dtype=np.uint8)
        self.hflags = np.array([l.never for l in lines], dtype=np.uint8)
        # descriptors
        self.strs = np.zeros(2 * n, dtype=HSTR)
        for i, l in enumerate(lines):
            self.strs[2 * i] = (
                (l.at, 0, 0, STATIC_SRC, NAME, l.id, l.at) if l.name is None
                else (l.name[0], l.name[1], l.name[2], WIRE, NAME, NONE, l.at))
            self.strs[2 * i + 1] = (
                (l.at, 0, 0, STATIC_SRC, VALUE, l.id, l.at) if l.value is None
                else (l.value[0], l.value[1], l.value[2], WIRE, VALUE, NONE,
                      l.at))
        self.max_len = max_len

    @functools.cached_property
    def _decoded(self):
        return self.decode(self.max_len)

    @property
    def strings(self):
        return self._decoded[0]

    @property
    def status(self):
        return self._decoded[1]

    @functools.cached_property
    def off(self):
        off = np.zeros(2 * self.n + 1, dtype=np.uint32)
        np.cumsum([len(s) for s in self.strings], out=off[1:])
        return off

    @functools.cached_property
    def data(self):
        return b"".join(self.strings)

    def decode(self, max_len):
        """-> ([bytes] * 2n, status uint8 [2n]) under the limit"""
        full = bytes(self.a0) + self.wire
        lits = [x for l in self.lines for x in (l.name, l.value)
                if x is not None]
        got = iter(_payloads(full, lits))
        strings, status = [], []
        for l in self.lines:
            nm, ns = (STATIC[l.id][0], DEC_OK) if l.name is None else next(got)
            v, vs = (STATIC[l.id][1], DEC_OK) if l.value is None else next(got)
            if max_len and len(nm) > max_len:
                nm, ns = b"", DEC_ERROR
            if max_len and vs == DEC_OK and \
                    len(v) + (len(nm) if ns == DEC_OK else 0) > max_len:
                v, vs = b"", DEC_ERROR
            strings += [nm, v]
            status += [ns, vs]
        return strings, np.array(status, dtype=np.uint8)

    @property
    def headers(self):
        s = self.strings
        return [(s[2 * i], s[2 * i + 1]) for i in range(self.n)]

    def str_bytes(self, max_hdrs=None):
        n = self.n if max_hdrs is None else min(self.n, max_hdrs)
        return self.strs[:2 * n].view(np.uint8).reshape(-1)

    @property
    def bound(self):
        return bound(len(self.wire), self.n)


# ---- the path each tile of qhuff_decode_headers takes (qhuff_hdrdec_impl.h) -----

TILE = 64                     # strings a tile: 32 whole headers
STAGE = 3072                  # kDecInCap = kOutCap
OUT_FAST = 3008               # total + 64 <= kOutCap
FIX_MAX = 66                  # kFixMaxLen: the fixed arena's longest wire string


def layout(d, residue=0):
    """per tile of d's descriptors, the buffer's first byte at `residue` mod
    16: {"staged": the 16-byte-aligned wire span fits the stage, "fast": and
    the output, static bytes included, fits the out stage, "fixed": no wire
    string of the tile is longer than FIX_MAX, "wire": its wire span's
    bytes, "out": its output bytes}"""
    sizes = [len(s) for s in d.strings]
    out = []
    for t0 in range(0, 2 * d.n, TILE):
        s = d.strs[t0:t0 + TILE]
        a = residue + int(s["pos"][0])
        b = residue + int(s["pos"][-1]) + int(s["len"][-1])
        span = (b + 15) // 16 * 16 - a // 16 * 16
        total = sum(sizes[t0:t0 + TILE])
        staged = span <= STAGE
        out.append({"staged": staged, "fast": staged and total <= OUT_FAST,
                    "fixed": int(s["len"].max()) <= FIX_MAX,
                    "wire": b - a, "out": total})
    return out
