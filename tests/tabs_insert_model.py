"""The model of qhuff_tabs_insert_host / _cpu (include/qhuff.h): encoder-stream
chunks applied to the tables of T connections, and the next set of tables.

Nothing here comes from the library.  The instructions are qpack_frames'
(encoder_stream_instructions; the framing verdict and the consumed bytes
ref_scan_encoder_stream's), the literals' bytes headers_dyn_model._lit_bytes'
Huffman oracle.  The rules are those of include/qhuff.h, the reference's:

  state of a table  (cap, lo, ins, used), used = sum of name + value + 32 over
                    [lo, ins);
  Set Capacity v    v > max_cap fails; else cap = v, evict from lo while
                    used > cap;
  static name ref   index >= 99 fails;
  dynamic name ref, duplicate
                    a = ins - 1 - idx, fails unless lo <= a < ins then;
  lengths           literal name: Ln > cap << 2 Hn fails; N > cap fails;
                    Lv > (cap - N) << 2 Hv fails (not for a duplicate);
  a literal the Huffman decoder rejects fails;
  push              ins += 1, used += size, evict from lo while used > cap (an
                    entry larger than cap evicts everything, itself included);
  a chunk that fails changes nothing and consumes nothing.

Ordinals are given out before anything is decoded: a chunk that fails on its
framing, a static index, a capacity or Ln has none; a chunk that fails later
keeps its ordinals (kind and ref as written on the wire, ins_lo = live_lo)."""
import numpy as np

import _paths  # noqa: F401
import headers_decode_model as H
import headers_dyn_model as D
import headers_tabs_model as TM
import qpack_frames as Q

OK, EPROTO, EINVAL, ERANGE = 0, -71, -22, -34
LITERAL, STATIC_REF, DYN_REF, DUP = 0, 1, 2, 3
NONE = 0xFFFFFFFF
STATIC = D.STATIC


def lit(l):
    """-> (bytes, ok) of a literal of qpack_frames.read_literal"""
    if not l["huffman"]:
        return l["payload"], True
    p = l["payload"]
    (s, st), = H._payloads(p, [(0, len(p), 1)])
    return s, st == D.DEC_OK


def size(e):
    return len(e[0]) + len(e[1]) + 32


class Chunk:
    """One chunk applied to one table: entries (all of them from absolute
    index `first`), the state (lo, cap, max_cap) -> rc, consumed, inserts
    [(kind, ref, ins_lo)], and the table after: entries, lo, cap."""

    def __init__(self, entries, first, lo, cap, max_cap, chunk):
        chunk = bytes(chunk)
        self.entries, self.lo, self.cap = list(entries), lo, cap
        self.inserts, self.rc, self.consumed = [], OK, 0
        st, _, consumed = Q.ref_scan_encoder_stream(chunk)
        instr = list(Q.encoder_stream_instructions(chunk[:consumed])) \
            if st == "ok" else []
        # what is known before anything is decoded
        c = cap
        bad = st != "ok"
        for kind, info in instr:
            if kind == "capacity":
                if info["capacity"] > max_cap:
                    bad = True
                    break
                c = info["capacity"]
            elif kind == "insert_nameref" and info["static"] \
                    and info["index"] >= 99:
                bad = True
            elif kind == "insert_literal":
                n = info["name"]
                if len(n["payload"]) > c << 2 * n["huffman"]:
                    bad = True
            if bad:
                break
        if bad:
            self.rc = EPROTO
            return
        ins0 = first + len(entries)
        ent = list(entries)
        used = sum(size(e) for e in ent[lo - first:])
        ok = True

        def evict(limit):
            nonlocal used, lo
            while used > limit:
                used -= size(ent[lo - first])
                lo += 1

        wire = []
        for kind, info in instr:
            # (the insert count as the wire gives it: while the chunk is good,
            # first + len(ent))
            ins = ins0 + len(wire)
            if kind == "capacity":
                cap = info["capacity"]
                evict(cap)
                continue
            if kind == "insert_literal":
                wire.append((LITERAL, NONE))
            elif kind == "insert_nameref" and info["static"]:
                wire.append((STATIC_REF, NONE))
            else:
                a = ins - 1 - info["index"]
                wire.append((DUP if kind == "dup" else DYN_REF,
                             a if a >= 0 else NONE))
            if not ok:
                continue
            k, a = wire[-1]
            if k in (DYN_REF, DUP) and not (a != NONE and lo <= a < ins):
                ok = False
                continue
            if k == DUP:
                e = ent[a - first]
            else:
                if k == LITERAL:
                    name, good = lit(info["name"])
                else:
                    name, good = (STATIC[info["index"]][0] if k == STATIC_REF
                                  else ent[a - first][0]), True
                v = info["value"]
                if len(name) > cap or \
                        len(v["payload"]) > (cap - len(name)) << 2 * v["huffman"]:
                    ok = False
                    continue
                value, vgood = lit(v)
                if not (good and vgood):
                    ok = False
                    continue
                e = (name, value)
            ent.append(e)
            used += size(e)
            evict(cap)
            self.inserts.append((k, a, lo))
        if not ok:
            self.rc = EPROTO
            self.inserts = [(k, a, self.lo) for k, a in wire]
            return
        self.consumed = consumed
        self.entries, self.lo, self.cap = ent, lo, cap


class Inserted:
    """T chunks applied to the T tables of `tabs` (headers_tabs_model.Tables)
    in the state cap / max_cap / live_lo: every array of the call."""

    def __init__(self, tabs, cap, max_cap, live_lo, chunks, keep=None, a0=0):
        T = tabs.T
        assert len(chunks) == T
        self.wire = bytes(a0) + b"".join(bytes(c) for c in chunks)
        self.enc_off = np.zeros(T + 1, dtype=np.uint32)
        self.enc_off[0] = a0
        if T:
            np.cumsum([len(c) for c in chunks], out=self.enc_off[1:])
            self.enc_off[1:] += np.uint32(a0)
        self.chunks = [Chunk(tabs.tables[c].entries, tabs.tables[c].first,
                             int(live_lo[c]), int(cap[c]), int(max_cap[c]),
                             chunks[c]) for c in range(T)]
        ch = self.chunks
        self.rc = np.array([x.rc for x in ch], dtype=np.int32)
        self.consumed = np.array([x.consumed for x in ch], dtype=np.uint32)
        self.ins_off = np.zeros(T + 1, dtype=np.uint32)
        if T:
            np.cumsum([len(x.inserts) for x in ch], out=self.ins_off[1:])
        flat = [i for x in ch for i in x.inserts]
        self.n = len(flat)
        self.ins_kind = np.array([i[0] for i in flat], dtype=np.uint8)
        self.ins_ref = np.array([i[1] for i in flat], dtype=np.uint32)
        self.ins_lo = np.array([i[2] for i in flat], dtype=np.uint32)
        self.cap_out = np.array([x.cap for x in ch], dtype=np.uint32)
        self.live_lo_out = np.array([x.lo for x in ch], dtype=np.uint32)
        out = []
        for c, x in enumerate(ch):
            f = tabs.tables[c].first
            k = x.lo if keep is None else min(max(int(keep[c]), f), x.lo)
            out.append(D.Table(x.entries[k - f:], k,
                               tabs.tables[c].max_entries))
        self.tabs = TM.Tables(out)
        self.out_first = self.tabs.first

    def check(self, r):
        """r: qhuff.Inserted of the same call"""
        assert r.ret == OK
        for name in ("rc", "consumed", "ins_off", "ins_kind", "ins_ref",
                     "ins_lo"):
            assert np.array_equal(getattr(r, name), getattr(self, name)), name
        assert np.array_equal(r.cap, self.cap_out)
        assert np.array_equal(r.live_lo, self.live_lo_out)
        if not self.tabs.T:
            assert r.tables == ()
            return
        data, off, ent, first, me = r.tables
        assert np.array_equal(ent, self.tabs.ent)
        assert np.array_equal(first, self.tabs.first)
        assert np.array_equal(off, self.tabs.off)
        assert bytes(data) == self.tabs.bytes
        assert np.array_equal(me, self.tabs.max_entries)
