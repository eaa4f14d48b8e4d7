"""The model of qhuff_scan_headers_dyn / qhuff_decode_headers_dyn: the header
list a field section decodes to against the dynamic table, the table's
entries given as plain arrays.

Nothing here comes from the library.  Framing is qpack_frames' restatement of
the reference's integer rules, the static table and the Huffman payloads are
headers_decode_model's (the golden table, the CPU oracle).  What is new:

  replay()   an interop file replayed: the encoder stream's instructions
             (qpack_frames.encoder_stream_instructions) applied to a table of
             the file's capacity -- the history of entries, oldest first --
             and every field section with the window [oldest live, insert
             count) it is decoded in;
  section()  one section's result code and lines under the rules of
             include/qhuff.h (qhuff_scan_headers_dyn), in their order:
               1. the framing verdict when it is not ok;
               2. EPROTO: encoded Required Insert Count > 2 * MaxEntries;
               3. RIC = the one value == enc - 1 (mod 2 * MaxEntries) in
                  [ins - MaxEntries + 1, ins + MaxEntries] (enc = 0: 0);
                  RIC <= 0 (enc != 0): EPROTO; RIC > ins: EBLOCKED;
               4. Base = RIC + DeltaBase, or RIC - DeltaBase - 1 (64-bit two's
                  complement); a dynamic line names Base - 1 - idx or, post
                  base, Base + idx; EPROTO when that is outside the window,
                  when RIC = 0 and a line is dynamic, when RIC != 0 and no
                  line names RIC - 1, when a static index is >= 99;
               5. OK;
  builders   of sections with dynamic lines, and the tile layout model with
             the dynamic bytes in a tile's output."""
import os

import numpy as np

import _paths  # noqa: F401
import headers_decode_model as H
import qpack_frames as Q

OK, ETRUNC, EPROTO, EBLOCKED = 0, -61, -71, -11
EINVAL, ERANGE = -22, -34
INDEXED, NAMEREF, LITERAL, LINE_DYN = 0, 1, 2, 4
NONE = 0xFF
DYN_NONE = 0xFFFFFFFF
WIRE, STATIC_SRC, DYN_SRC = 0, 1, 2
NAME, VALUE = 1, 2
DEC_OK, DEC_ERROR = 0, 1
MAX_STRLEN = H.MAX_STRLEN
HSTR = H.HSTR
STATIC = H.STATIC
M64 = (1 << 64) - 1

DATA = os.path.join(H.G, "data")
INTEROP = {"netbsd": (18, 18, 15), "fb-req": (9, 10, 8), "fb-resp": (7, 11, 6)}
INTEROP_CAPACITY = 256                   # the files' ".256." : MaxEntries 8


def bound(wire_bytes, n, dyn_longest):
    """qhuff_decode_headers_dyn_bound"""
    return 8 * wire_bytes // 5 + max(76, dyn_longest) * n + 16


class Table:
    """struct qhuff_dyn_table: entries [(name, value)] oldest first, entry k
    the absolute index first + k; `pad` bytes before the first entry"""

    def __init__(self, entries=(), first=0, max_entries=8, pad=0):
        self.entries = [(bytes(n), bytes(v)) for n, v in entries]
        self.first, self.max_entries, self.d = first, max_entries, len(entries)
        flat = [x for e in self.entries for x in e]
        self.off = np.zeros(2 * self.d + 1, dtype=np.uint32)
        self.off[0] = pad
        if flat:
            np.cumsum([len(x) for x in flat], out=self.off[1:])
            self.off[1:] += np.uint32(pad)
        self.bytes = bytes(pad) + b"".join(flat)
        self.longest = max([len(n) + len(v) for n, v in self.entries] or [0])

    @property
    def data(self):
        return np.frombuffer(self.bytes, dtype=np.uint8)

    def entry(self, abs_id):
        return self.entries[abs_id - self.first]


# ---- an interop file replayed -----------------------------------------------

def _lit_bytes(lit):
    if not lit["huffman"]:
        return lit["payload"]
    p = lit["payload"]
    (s, st), = H._payloads(p, [(0, len(p), 1)])
    assert st == DEC_OK
    return s


class Replay:
    """entries: every insert of the file in order; sections: [bytes] in file
    order with their stream ids; win: per section (oldest live, insert
    count) at its place in the file"""

    def __init__(self, name, capacity=INTEROP_CAPACITY):
        with open(os.path.join(DATA, name + ".out.256.100.1"), "rb") as f:
            data = f.read()
        self.max_entries = capacity // 32
        self.entries, self.sections, self.sids, self.win = [], [], [], []
        cap, oldest = capacity, 0

        def insert(n, v):
            nonlocal oldest
            size = lambda e: len(e[0]) + len(e[1]) + 32       # noqa: E731
            used = sum(size(e) for e in self.entries[oldest:])
            assert size((n, v)) <= cap
            while used + size((n, v)) > cap:
                used -= size(self.entries[oldest])
                oldest += 1
            self.entries.append((n, v))

        for sid, fr in Q.read_interop(data):
            if sid:
                self.sections.append(bytes(fr))
                self.sids.append(sid)
                self.win.append((oldest, len(self.entries)))
                continue
            for kind, info in Q.encoder_stream_instructions(fr):
                ins = len(self.entries)
                if kind == "capacity":
                    cap = info["capacity"]
                    assert cap <= capacity
                elif kind == "dup":
                    a = ins - 1 - info["index"]
                    assert oldest <= a
                    insert(*self.entries[a])
                elif kind == "insert_literal":
                    insert(_lit_bytes(info["name"]), _lit_bytes(info["value"]))
                else:
                    if info["static"]:
                        nm = STATIC[info["index"]][0]
                    else:
                        a = ins - 1 - info["index"]
                        assert oldest <= a
                        nm = self.entries[a][0]
                    insert(nm, _lit_bytes(info["value"]))
        self.oldest = oldest
        self.table = Table(self.entries, 0, self.max_entries)
        self.sec_win = np.array(self.win, dtype=np.uint32).reshape(-1)

    def qif_lists(self, name):
        with open(os.path.join(DATA, name + ".qif"), "rb") as f:
            lists = Q.qif_header_lists(f.read())
        return [lists[sid - 1] for sid in self.sids]


# ---- the rules ----------------------------------------------------------------

def enc_ric(ric, max_entries):
    """RFC 9204 4.5.1.1: the encoded Required Insert Count"""
    return 0 if ric == 0 else ric % (2 * max_entries) + 1


def ric_of(enc, ins, max_entries):
    """-> (rc, RIC): rules 2 and 3"""
    if enc > 2 * max_entries:
        return EPROTO, None
    if enc == 0:
        return OK, 0
    full = 2 * max_entries
    lo = ins - max_entries + 1
    ric = lo + (enc - 1 - lo) % full
    assert lo <= ric <= ins + max_entries and (ric - enc + 1) % full == 0
    if ric <= 0:
        return EPROTO, ric
    if ric > ins:
        return EBLOCKED, ric
    return OK, ric


def _s64(x):
    x &= M64
    return x - (1 << 64) if x >> 63 else x


class Line:
    """as headers_decode_model.Line, and dyn: the absolute index the line
    named, or None"""
    __slots__ = ("kind", "id", "never", "at", "name", "value", "dyn")

    def __init__(self, kind, sid, never, at, name, value, dyn=None):
        self.kind, self.id, self.never, self.at = kind, sid, never, at
        self.name, self.value, self.dyn = name, value, dyn


def section(buf, lo, ins, max_entries):
    """-> (rc, [Line]) of one field section decoded in the window [lo, ins)"""
    buf = bytes(buf)
    st, _ = Q.ref_scan_field_section(buf)
    if st != "ok":
        return (ETRUNC if st == "trunc" else EPROTO), []
    enc, pos = Q.dec_int(buf, 0, 8)
    sign = buf[pos] >> 7
    delta, pos = Q.dec_int(buf, pos, 7)
    rc, ric = ric_of(enc, ins, max_entries)
    if rc != OK:
        return rc, []
    base = _s64(ric - delta - 1 if sign else ric + delta)
    bad, used_ric, lines = False, False, []

    def dyn(a):
        nonlocal bad, used_ric
        a = _s64(a)
        if ric == 0 or not lo <= a < ins:
            bad = True
            return None
        if a == ric - 1:
            used_ric = True
        return a

    def span(l):
        return (l[0], l[1], l[2])

    while pos < len(buf):
        b, at = buf[pos], pos
        if b & 0x80:                         # 1T indexed
            idx, pos = Q.dec_int24(buf, pos, 6)
            if b & 0x40:
                if idx >= 99:
                    bad = True
                else:
                    lines.append(Line(INDEXED, idx, 0, at, None, None))
            else:
                lines.append(Line(INDEXED | LINE_DYN, NONE, 0, at, None, None,
                                  dyn(base - 1 - idx)))
        elif b & 0x40:                       # 01NT name reference
            idx, pos = Q.dec_int24(buf, pos, 4)
            v, pos = Q._lit(buf, pos, 7, VALUE, at, MAX_STRLEN)
            if b & 0x10:
                if idx >= 99:
                    bad = True
                else:
                    lines.append(Line(NAMEREF, idx, b >> 5 & 1, at, None,
                                      span(v)))
            else:
                lines.append(Line(NAMEREF | LINE_DYN, NONE, b >> 5 & 1, at,
                                  None, span(v), dyn(base - 1 - idx)))
        elif b & 0x20:                       # 001N literal name
            n, pos = Q._lit(buf, pos, 3, NAME, at, MAX_STRLEN)
            v, pos = Q._lit(buf, pos, 7, VALUE, at, MAX_STRLEN)
            lines.append(Line(LITERAL, NONE, b >> 4 & 1, at, span(n), span(v)))
        elif b & 0x10:                       # 0001 indexed post-base
            idx, pos = Q.dec_int24(buf, pos, 4)
            lines.append(Line(INDEXED | LINE_DYN, NONE, 0, at, None, None,
                              dyn(base + idx)))
        else:                                # 0000N post-base name reference
            idx, pos = Q.dec_int24(buf, pos, 3)
            v, pos = Q._lit(buf, pos, 7, VALUE, at, MAX_STRLEN)
            lines.append(Line(NAMEREF | LINE_DYN, NONE, b >> 3 & 1, at, None,
                              span(v), dyn(base + idx)))
    if bad or (ric != 0 and not used_ric):
        return EPROTO, []
    return OK, lines


# ---- builders -------------------------------------------------------------------

def prefix(enc, sign=0, delta=0):
    """a section's two prefix integers"""
    return Q.enc_int(0, enc, 8) + Q.enc_int(sign << 7, delta, 7)


def prefix_for(ric, base, max_entries):
    """the prefix that gives Required Insert Count ric and Base base"""
    if base >= ric:
        return prefix(enc_ric(ric, max_entries), 0, base - ric)
    return prefix(enc_ric(ric, max_entries), 1, ric - base - 1)


def indexed_dyn(idx):
    return Q.enc_int(0x80, idx, 6)


def indexed_post(idx):
    return Q.enc_int(0x10, idx, 4)


def _value(value, huffman):
    import oracle_lib as O
    p = O.huffman_enc(value) if huffman else bytes(value)
    return Q.enc_int(0x80 if huffman else 0, len(p), 7) + p


def nameref_dyn(idx, value, never=0, huffman=0):
    return Q.enc_int(0x40 | never << 5, idx, 4) + _value(value, huffman)


def nameref_post(idx, value, never=0, huffman=0):
    return Q.enc_int(never << 3, idx, 3) + _value(value, huffman)


def indexed_static(idx):
    return Q.enc_int(0xc0, idx, 6)


def nameref_static(idx, value, never=0, huffman=0):
    return Q.enc_int(0x50 | never << 5, idx, 4) + _value(value, huffman)


def literal(name, value, never=0, huffman=0):
    import oracle_lib as O
    p = O.huffman_enc(name) if huffman else bytes(name)
    return (Q.enc_int(0x20 | never << 4 | (8 if huffman else 0), len(p), 3)
            + p + _value(value, huffman))


# ---- every output of the scan and of the decode -----------------------------------

class Decoded:
    """sections packed back to back from offset a0, decoded against `table`,
    section s in the window win[s] = (lo, ins) (None: the whole table)"""

    def __init__(self, sections, table, win=None, max_len=MAX_STRLEN, a0=0):
        sections = [bytes(s) for s in sections]
        m = len(sections)
        self.m, self.a0, self.table = m, a0, table
        if win is None:
            win = [(table.first, table.first + table.d)] * m
            self.sec_win = None
        else:
            self.sec_win = np.array(win, dtype=np.uint32).reshape(-1)
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
            rc, ls = section(s, win[i][0], win[i][1], table.max_entries)
            self.rc[i] = rc
            self.hdr_off[i + 1] = self.hdr_off[i] + len(ls)
            base = int(self.sec_off[i])
            for l in ls:
                mv = lambda x: None if x is None else (x[0] + base, x[1], x[2])  # noqa: E731
                lines.append(Line(l.kind, l.id, l.never, l.at + base,
                                  mv(l.name), mv(l.value), l.dyn))
        self.lines = lines
        n = self.n = len(lines)
        self.kind = np.array([l.kind for l in lines], dtype=np.uint8)
        self.static_id = np.array([l.id for l in lines], dtype=np.uint8)
        self.hflags = np.array([l.never for l in lines], dtype=np.uint8)
        self.dyn_id = np.array([DYN_NONE if l.dyn is None else l.dyn
                                for l in lines], dtype=np.uint32)
        self.strs = np.zeros(2 * n, dtype=HSTR)
        for i, l in enumerate(lines):
            k = None if l.dyn is None else l.dyn - table.first
            for j, (lit, kd) in enumerate(((l.name, NAME), (l.value, VALUE))):
                if lit is not None:
                    d = (lit[0], lit[1], lit[2], WIRE, kd, NONE, l.at)
                elif k is None:
                    d = (l.at, 0, 0, STATIC_SRC, kd, l.id, l.at)
                else:
                    a, b = table.off[2 * k + j], table.off[2 * k + j + 1]
                    d = (l.at, int(b - a), 0, DYN_SRC, kd, NONE, int(a))
                self.strs[2 * i + j] = d
        self.max_len = max_len
        self._dec = None

    def decode(self, max_len):
        """-> ([bytes] * 2n, status uint8 [2n]) under the limit"""
        full = bytes(self.a0) + self.wire
        lits = [x for l in self.lines for x in (l.name, l.value)
                if x is not None]
        got = iter(H._payloads(full, lits))
        strings, status = [], []
        for l in self.lines:
            fixed = (None if l.kind == LITERAL
                     else self.table.entry(l.dyn) if l.dyn is not None
                     else STATIC[l.id])
            nm, ns = (fixed[0], DEC_OK) if l.name is None else next(got)
            v, vs = (fixed[1], DEC_OK) if l.value is None else next(got)
            if max_len and len(nm) > max_len:
                nm, ns = b"", DEC_ERROR
            if max_len and vs == DEC_OK and \
                    len(v) + (len(nm) if ns == DEC_OK else 0) > max_len:
                v, vs = b"", DEC_ERROR
            strings += [nm, v]
            status += [ns, vs]
        return strings, np.array(status, dtype=np.uint8)

    @property
    def strings(self):
        if self._dec is None:
            self._dec = self.decode(self.max_len)
        return self._dec[0]

    @property
    def status(self):
        self.strings
        return self._dec[1]

    @property
    def off(self):
        off = np.zeros(2 * self.n + 1, dtype=np.uint32)
        np.cumsum([len(s) for s in self.strings], out=off[1:])
        return off

    @property
    def data(self):
        return b"".join(self.strings)

    @property
    def headers(self):
        s = self.strings
        return [(s[2 * i], s[2 * i + 1]) for i in range(self.n)]

    def header_lists(self):
        h = self.headers
        return [h[self.hdr_off[i]:self.hdr_off[i + 1]] for i in range(self.m)]

    def str_bytes(self, max_hdrs=None):
        n = self.n if max_hdrs is None else min(self.n, max_hdrs)
        return self.strs[:2 * n].view(np.uint8).reshape(-1)

    @property
    def bound(self):
        return bound(len(self.wire), self.n, self.table.longest)


# ---- the path each tile of qhuff_decode_headers_dyn takes ---------------------------

TILE, STAGE, OUT_FAST, FIX_MAX = H.TILE, H.STAGE, H.OUT_FAST, H.FIX_MAX


def layout(d, residue=0):
    """as headers_decode_model.layout -- a DYN string has no wire bytes, its
    bytes count in the tile's output -- and "dyn": the tile's dynamic bytes"""
    sizes = [len(s) for s in d.strings]
    out = []
    for t0 in range(0, 2 * d.n, TILE):
        s = d.strs[t0:t0 + TILE]
        wl = np.where(s["source"] == WIRE, s["len"], 0)
        a = residue + int(s["pos"][0])
        b = residue + int(s["pos"][-1]) + int(wl[-1])
        span = (b + 15) // 16 * 16 - a // 16 * 16
        total = sum(sizes[t0:t0 + TILE])
        dyn = sum(z for z, src in zip(sizes[t0:t0 + TILE], s["source"])
                  if src == DYN_SRC)
        staged = span <= STAGE
        out.append({"staged": staged, "fast": staged and total <= OUT_FAST,
                    "fixed": int(wl.max()) <= FIX_MAX, "wire": b - a,
                    "out": total, "dyn": dyn})
    return out
