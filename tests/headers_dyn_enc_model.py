"""The model of qhuff_dyn_lookup / qhuff_encode_headers_dyn: which field line
the reference's encoder writes for a header when the dynamic table is given
and nothing is inserted, and the section's bytes.

Nothing here comes from the library.  The rule is include/qhuff.h's, restated
as a scan of the window's entries (no hashes, no index): static full match
(headers_model.lookup), else the HIGHEST equal entry of the window, else the
static name match, else the LOWEST entry of the window with the name, else a
literal.  Static and literal lines are headers_model.line's bytes; dynamic
lines and the prefix are built with headers_dyn_model's builders
(indexed_dyn / indexed_post / nameref_dyn / nameref_post / prefix_for), the
value's Huffman choice being lsqpack_enc_enc_str's (oracle_lib.enc_enc_str).
RIC = 1 + the largest index named; max_entries = 0 or an empty window: no
dynamic lines."""
import functools

import numpy as np

import _paths  # noqa: F401
import headers_dyn_model as D
import headers_model as HM
import oracle_lib as O

INDEXED, NAMEREF, LITERAL, LINE_DYN = D.INDEXED, D.NAMEREF, D.LITERAL, D.LINE_DYN
NONE, DYN_NONE = D.NONE, D.DYN_NONE


def choose(name, value, table, lo, hi):
    """-> (kind, static id, absolute index or None)"""
    _, _, kind, sid = HM.lookup(name, value)
    lo, hi = max(lo, table.first), min(hi, table.first + table.d)
    if kind == INDEXED or hi <= lo or table.max_entries == 0:
        return kind, sid, None
    full = [a for a in range(lo, hi) if table.entry(a) == (name, value)]
    if full:
        return INDEXED | LINE_DYN, NONE, max(full)
    if kind == NAMEREF:
        return kind, sid, None
    named = [a for a in range(lo, hi) if table.entry(a)[0] == name]
    if named:
        return NAMEREF | LINE_DYN, NONE, min(named)
    return LITERAL, NONE, None


def _huffman(value):
    """lsqpack_enc_enc_str's choice for a 7-bit literal"""
    return O.enc_enc_str(7, value)[0] >> 7


def line(name, value, never, table, lo, hi, base):
    """the field line's bytes -> (bytes, kind, static id, abs or None)"""
    kind, sid, a = choose(name, value, table, lo, hi)
    n = 1 if never & HM.NEVER else 0
    if a is None:
        b, k2, s2 = HM.line(name, value, never)
        assert (k2, s2) == (kind, sid)
        return b, kind, sid, None
    post = a >= base
    rel = a - base if post else base - 1 - a
    if kind == INDEXED | LINE_DYN:
        b = D.indexed_post(rel) if post else D.indexed_dyn(rel)
    else:
        f = D.nameref_post if post else D.nameref_dyn
        b = f(rel, value, n, _huffman(value))
        assert b.endswith(O.enc_enc_str(7, value))
    return b, kind, sid, a


def section(headers, table, lo, hi, base):
    """one section -> (bytes, [(kind, static id, abs or None)])"""
    ls = [line(h[0], h[1], h[2] if len(h) > 2 else 0, table, lo, hi, base)
          for h in headers]
    ric = max([x[3] + 1 for x in ls if x[3] is not None] or [0])
    pre = D.prefix_for(ric, base, table.max_entries) if ric else b"\0\0"
    return pre + b"".join(x[0] for x in ls), [x[1:] for x in ls]


class Encoded:
    """header lists, one section each, against `table` -> the call's arrays
    and what it must give back.  win: [(lo, hi)] per section or None (the
    whole table); base: [Base] per section or None (the window's end)"""

    def __init__(self, sections, table, win=None, base=None, flags=True):
        self.h = HM.Headers(sections, flags)
        self.table, self.n, self.m = table, self.h.n, self.h.m
        self.win, self.base = win, base
        self.sec_win = None if win is None else \
            np.array(win, dtype=np.uint32).reshape(-1)
        self.sec_base = None if base is None else \
            np.array(base, dtype=np.uint32)
        whole = (table.first, table.first + table.d)
        self.wins = [whole] * self.m if win is None else list(win)
        self.bases = [w[1] for w in self.wins] if base is None else list(base)
        self.data, self.off = self.h.data, self.h.off
        self.sec_hdr, self.hflags = self.h.sec_hdr, self.h.hflags

    @property
    def tab(self):
        """the table as qhuff.dyn_table_host takes it"""
        t = self.table
        return (t.data, t.off, t.first, t.max_entries)

    @functools.cached_property
    def _enc(self):
        return [section(s, self.table, w[0], w[1], b) for s, w, b in
                zip(self.h.sections, self.wins, self.bases)]

    @property
    def want_sections(self):
        return [e[0] for e in self._enc]

    @property
    def want(self):
        return b"".join(self.want_sections)

    @functools.cached_property
    def want_sec_out(self):
        o = np.zeros(self.m + 1, dtype=np.uint32)
        np.cumsum([len(s) for s in self.want_sections], out=o[1:])
        return o

    def _col(self, i, dtype, none):
        return np.array([none if x[i] is None else x[i]
                         for e in self._enc for x in e[1]], dtype=dtype)

    @functools.cached_property
    def want_kind(self):
        return self._col(0, np.uint8, 0)

    @functools.cached_property
    def want_id(self):
        return self._col(1, np.uint8, 0)

    @functools.cached_property
    def want_dyn(self):
        return self._col(2, np.uint32, DYN_NONE)

    @property
    def bound(self):
        return self.h.bound

    def decode_win(self):
        """the windows qhuff_decode_headers_dyn takes for the output: what
        the encoder could name the decoder must hold"""
        return self.wins


def lookup(pairs, table, lo, hi):
    """qhuff_dyn_lookup's arrays for [(name, value)] in one window ->
    (name_hash, nameval_hash, kind, static_id, dyn_id)"""
    hs = [HM.hashes(n, v) for n, v in pairs]
    ch = [choose(n, v, table, lo, hi) for n, v in pairs]
    return (np.array([h[0] for h in hs], dtype=np.uint32),
            np.array([h[1] for h in hs], dtype=np.uint32),
            np.array([c[0] for c in ch], dtype=np.uint8),
            np.array([c[1] for c in ch], dtype=np.uint8),
            np.array([DYN_NONE if c[2] is None else c[2] for c in ch],
                     dtype=np.uint32))
