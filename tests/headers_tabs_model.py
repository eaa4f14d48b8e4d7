"""The model of the calls over a set of dynamic tables (struct
qhuff_dyn_tables: qhuff_scan_headers_tabs, qhuff_dyn_lookup_tabs,
qhuff_encode_headers_tabs): a batch whose sections belong to different
connections, each with its own table.

There is no rule here.  A multi-table batch is a loop that hands each section
its own headers_dyn_model.Table: the scan's result of a section is
headers_dyn_model.Decoded of that section alone against its table, the encode's
headers_dyn_enc_model.section, the lookup's headers_dyn_enc_model.lookup.  What
this file adds is the packing: the tables' entries in one arena (Tables) and
the per-section results laid side by side as the calls return them, a DYN
descriptor's instr moved from its table's own bytes to the shared ones."""
import functools

import numpy as np

import _paths  # noqa: F401
import headers_dyn_enc_model as E
import headers_dyn_model as D
import headers_model as HM


class Tables:
    """struct qhuff_dyn_tables over [headers_dyn_model.Table]: the entries
    packed in table order behind `pad` bytes.  The tables' own first,
    max_entries and entries are kept; their own pad is not used."""

    def __init__(self, tables, pad=0):
        self.tables = list(tables)
        self.T = len(self.tables)
        flat = [x for t in self.tables for e in t.entries for x in e]
        self.D = len(flat) // 2
        self.off = np.zeros(2 * self.D + 1, dtype=np.uint32)
        self.off[0] = pad
        if flat:
            np.cumsum([len(x) for x in flat], out=self.off[1:])
            self.off[1:] += np.uint32(pad)
        self.bytes = bytes(pad) + b"".join(flat)
        self.ent = np.zeros(self.T + 1, dtype=np.uint32)
        if self.T:
            np.cumsum([t.d for t in self.tables], out=self.ent[1:])
        self.first = np.array([t.first for t in self.tables], dtype=np.uint32)
        self.max_entries = np.array([t.max_entries for t in self.tables],
                                    dtype=np.uint32)
        self.longest = max([t.longest for t in self.tables] or [0])

    @property
    def data(self):
        return np.frombuffer(self.bytes, dtype=np.uint8)

    @property
    def args(self):
        """the set as qhuff.dyn_tables_host takes it"""
        if not self.T:
            return ()
        return (self.data, self.off, self.ent, self.first, self.max_entries)

    def table(self, c):
        return self.tables[c] if self.T else D.Table([], 0, 0)

    def whole(self, c):
        t = self.table(c)
        return (t.first, t.first + t.d)

    def byte_base(self, c):
        """where table c's first entry lies in the shared bytes"""
        return int(self.off[2 * int(self.ent[c])]) if self.T else 0


def _sec_tab(tabs, sec_tab, m):
    if not tabs.T:
        return [0] * m, None
    st = [int(c) for c in sec_tab]
    assert len(st) == m
    return st, np.array(st, dtype=np.uint32)


class Decoded:
    """sections packed back to back from offset a0, section s decoded against
    table sec_tab[s] of `tabs` in the window win[s] = (lo, ins) (win None: the
    whole of its table) -> the arrays of qhuff_scan_headers_tabs and the
    decoded strings, as headers_dyn_model.Decoded gives them for one table"""

    def __init__(self, sections, tabs, sec_tab, win=None,
                 max_len=D.MAX_STRLEN, a0=0):
        sections = [bytes(s) for s in sections]
        m = self.m = len(sections)
        self.tabs, self.a0 = tabs, a0
        self.tab_of, self.sec_tab = _sec_tab(tabs, sec_tab, m)
        self.sec_win = None if win is None else \
            np.array(win, dtype=np.uint32).reshape(-1)
        self.wins = [tabs.whole(c) for c in self.tab_of] if win is None \
            else [tuple(w) for w in win]
        self.wire = b"".join(sections)
        self.sec_off = np.zeros(m + 1, dtype=np.uint32)
        self.sec_off[0] = a0
        if m:
            np.cumsum([len(s) for s in sections], out=self.sec_off[1:])
            self.sec_off[1:] += np.uint32(a0)
        # the loop: each section alone, against its own table
        self.parts = [D.Decoded([s], tabs.table(c), [w], max_len,
                                int(self.sec_off[i]))
                      for i, (s, c, w) in
                      enumerate(zip(sections, self.tab_of, self.wins))]
        self.rc = np.array([int(p.rc[0]) for p in self.parts], dtype=np.int32)
        self.hdr_off = np.zeros(m + 1, dtype=np.uint32)
        if m:
            np.cumsum([p.n for p in self.parts], out=self.hdr_off[1:])
        self.n = int(self.hdr_off[-1])
        cat = lambda f, dt: np.concatenate(  # noqa: E731
            [f(p) for p in self.parts] + [np.zeros(0, dt)]).astype(dt)
        self.kind = cat(lambda p: p.kind, np.uint8)
        self.static_id = cat(lambda p: p.static_id, np.uint8)
        self.hflags = cat(lambda p: p.hflags, np.uint8)
        self.dyn_id = cat(lambda p: p.dyn_id, np.uint32)
        strs = []
        for p, c in zip(self.parts, self.tab_of):
            s = p.strs.copy()
            # (a table's own offsets start at 0: instr moves to the arena)
            t = tabs.table(c)
            s["instr"] = np.where(s["source"] == D.DYN_SRC,
                                  s["instr"] - np.uint32(t.off[0])
                                  + np.uint32(tabs.byte_base(c)), s["instr"])
            strs.append(s)
        self.strs = np.concatenate(strs + [np.zeros(0, D.HSTR)])

    @functools.cached_property
    def strings(self):
        return [x for p in self.parts for x in p.strings]

    @functools.cached_property
    def status(self):
        return np.concatenate([p.status for p in self.parts]
                              + [np.zeros(0, np.uint8)])

    @property
    def off(self):
        off = np.zeros(2 * self.n + 1, dtype=np.uint32)
        np.cumsum([len(s) for s in self.strings], out=off[1:])
        return off

    @property
    def data(self):
        return b"".join(self.strings)

    def header_lists(self):
        s = self.strings
        h = [(s[2 * i], s[2 * i + 1]) for i in range(self.n)]
        return [h[self.hdr_off[i]:self.hdr_off[i + 1]] for i in range(self.m)]

    def str_bytes(self, max_hdrs=None):
        n = self.n if max_hdrs is None else min(self.n, max_hdrs)
        return self.strs[:2 * n].view(np.uint8).reshape(-1)

    @property
    def buf(self):
        return np.frombuffer(bytes(self.a0) + self.wire, dtype=np.uint8)


class Encoded:
    """header lists, one section each, section s against table sec_tab[s] of
    `tabs` -> the call's arrays and what it must give back, as
    headers_dyn_enc_model.Encoded for one table.  win: [(lo, hi)] per section
    or None (the whole of its table); base: [Base] or None (the window's
    end)"""

    def __init__(self, sections, tabs, sec_tab, win=None, base=None,
                 flags=True):
        self.h = HM.Headers(sections, flags)
        self.tabs, self.n, self.m = tabs, self.h.n, self.h.m
        self.tab_of, self.sec_tab = _sec_tab(tabs, sec_tab, self.m)
        self.sec_win = None if win is None else \
            np.array(win, dtype=np.uint32).reshape(-1)
        self.sec_base = None if base is None else \
            np.array(base, dtype=np.uint32)
        self.wins = [tabs.whole(c) for c in self.tab_of] if win is None \
            else [tuple(w) for w in win]
        self.bases = [w[1] for w in self.wins] if base is None else list(base)
        self.data, self.off = self.h.data, self.h.off
        self.sec_hdr, self.hflags = self.h.sec_hdr, self.h.hflags

    @functools.cached_property
    def _enc(self):
        # the loop: each section alone, against its own table
        return [E.section(s, self.tabs.table(c), w[0], w[1], b)
                for s, c, w, b in zip(self.h.sections, self.tab_of, self.wins,
                                      self.bases)]

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
        return self._col(2, np.uint32, D.DYN_NONE)

    @functools.cached_property
    def want_lookup(self):
        """qhuff_dyn_lookup_tabs' five arrays"""
        parts = [E.lookup([h[:2] for h in s], self.tabs.table(c), w[0], w[1])
                 for s, c, w in zip(self.h.sections, self.tab_of, self.wins)
                 if s]
        dts = (np.uint32, np.uint32, np.uint8, np.uint8, np.uint32)
        return tuple(np.concatenate([p[i] for p in parts] + [np.zeros(0, dt)])
                     .astype(dt) for i, dt in enumerate(dts))

    @property
    def bound(self):
        return self.h.bound
