"""qhuff_encode_wire / qhuff_encode_wire_host: whole QPACK field lines and
encoder-stream instructions encoded in one launch (include/qhuff.h), and
qhuff_items_check, the item rule the device call relies on.

Expectations never come from the library: an item's bytes are
qpack_frames.enc_int(int_first, ival, int_bits) followed by
oracle_lib.enc_enc_str(str_bits, string, str_first) -- both pinned to the
reference's vectors -- or the reference's own files; the large batch's are
oracle_lib.encode_batch per prefix class plus numpy integer coding, checked
here against the per-item form.  The shape builders recompute from the sizes
which path each 64-item tile takes (input stage, output stage, dense
stream), so that each shape is known to reach the path it is named for at
the residues it runs at."""
import ctypes as C
import functools
import json
import os
import random

import numpy as np
import pytest

import _paths  # noqa: F401
import limits
import oracle_lib as O
import qhuff
import qpack_frames as Q
from test_buffer_contract import FILLS, Arena
from test_frames import STREAMS, data_file, frames

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TILE = limits.TS
STAGE = limits.STAGE
OUT_FAST = limits.OUT_FAST
DENSE_MAX = limits.DENSE_MAX
HIGH = 0xF0000000
TOKEN = limits.TOKEN
B8 = bytes(limits.BY_LEN[8])          # Huffman as long as raw: sent raw
B30 = limits.B30                      # the long-code alphabet


def allowed_first(p):
    """every bit of a literal's first byte above its H bit"""
    return ~((2 << p) - 1) & 0xFF


# ---- items and their expectation ------------------------------------------------

def item(ival=0, int_bits=0, int_first=0, str_bits=0, str_first=0):
    return qhuff.Item(ival, int_bits, int_first, str_bits, str_first)


def item_bytes(it, s):
    out = b""
    if it.int_bits:
        out += Q.enc_int(it.int_first, it.ival, it.int_bits)
    if it.str_bits:
        out += O.enc_enc_str(it.str_bits, s, it.str_first)
    return out


class Batch:
    """n strings and n items; want(): the n outputs"""

    def __init__(self, strings, items):
        assert len(strings) == len(items)
        self.strings, self.items = list(strings), list(items)
        self.n = len(items)
        self.data, self.off = limits.pack(self.strings)
        assert qhuff.items_check(self.items) == (qhuff.OK, None)

    @functools.cached_property
    def want(self):
        return [item_bytes(it, s) for it, s in zip(self.items, self.strings)]

    @functools.cached_property
    def want_off(self):
        off = np.zeros(self.n + 1, dtype=np.uint32)
        np.cumsum([len(w) for w in self.want], out=off[1:])
        return off

    @property
    def total(self):
        return int(self.want_off[-1])

    @property
    def bound(self):
        return qhuff.encode_wire_bound(len(self.data), self.n)

    def paths(self, r):
        """the path of every tile with the data pointer at r mod 16:
        "in" (input span past the stage: out of line), "out" (output past
        the output stage: out of line), "dense", "lane" (dense stream
        overflown: item per lane from the stage)"""
        raw, off, out = self.data.tobytes(), [int(x) for x in self.off], []
        for t0 in range(0, self.n, TILE):
            cnt = min(TILE, self.n - t0)
            a, b = off[t0], off[t0 + cnt]
            if limits._span(r, a, b) > STAGE:
                out.append("in")
            elif int(self.want_off[t0 + cnt] - self.want_off[t0]) > OUT_FAST:
                out.append("out")
            else:
                # the dense pass codes the span from its 16-byte boundary:
                # up to 15 bytes in front of the tile, of any code length
                lead = (r + a) % 16
                lo = limits.code_bits(raw[max(a - lead, 0):b])
                hi = lo + 30 * max(lead - a, 0)
                assert hi <= DENSE_MAX or lo > DENSE_MAX, "on the dense edge"
                out.append("dense" if hi <= DENSE_MAX else "lane")
        return out


# ---- the frame walker -------------------------------------------------------------

def _string(lit):
    if not lit["huffman"]:
        return lit["payload"]
    st, s = O.huff_decode(lit["payload"])
    assert st == O.OK
    return s


def _int_item(buf, pos, bits, lit_bits=0):
    """the prefixed integer at pos (its first byte's bits above the prefix
    are the instruction's) and, with lit_bits, the literal behind it ->
    (item, string, end)"""
    first = buf[pos] & ~((1 << bits) - 1) & 0xFF
    v, pos = Q.read_int(buf, pos, bits)
    if not lit_bits:
        return item(v, bits, first), b"", pos
    lit = Q.read_literal(buf, pos, lit_bits)
    sfirst = lit["first_byte"] & allowed_first(lit_bits)
    return item(v, bits, first, lit_bits, sfirst), _string(lit), lit["end"]


def _lit_item(buf, pos, bits):
    lit = Q.read_literal(buf, pos, bits)
    return (item(str_bits=bits, str_first=lit["first_byte"] & allowed_first(bits)),
            _string(lit), lit["end"])


def walk_field_section(buf):
    """a field section, prefix included -> [(item, string)] (RFC 9204 4.5)"""
    out, pos = [], 0
    for bits in (8, 7):                # Required Insert Count, S + Delta Base
        it, s, pos = _int_item(buf, pos, bits)
        out.append((it, s))
    while pos < len(buf):
        b = buf[pos]
        if b & 0x80:                   # indexed
            it, s, pos = _int_item(buf, pos, 6)
        elif b & 0x40:                 # literal with name reference
            it, s, pos = _int_item(buf, pos, 4, 7)
        elif b & 0x20:                 # literal with literal name
            it, s, pos = _lit_item(buf, pos, 3)
            out.append((it, s))
            it, s, pos = _lit_item(buf, pos, 7)
        elif b & 0x10:                 # indexed post-base
            it, s, pos = _int_item(buf, pos, 4)
        else:                          # literal with post-base name reference
            it, s, pos = _int_item(buf, pos, 3, 7)
        out.append((it, s))
    assert pos == len(buf)
    return out


def walk_encoder_stream(buf):
    """complete encoder-stream instructions -> [(item, string)] (RFC 9204
    4.3)"""
    out, pos = [], 0
    while pos < len(buf):
        b = buf[pos]
        if b & 0x80:                   # insert with name reference
            it, s, pos = _int_item(buf, pos, 6, 7)
        elif b & 0x40:                 # insert with literal name
            it, s, pos = _lit_item(buf, pos, 5)
            out.append((it, s))
            it, s, pos = _lit_item(buf, pos, 7)
        else:                          # set capacity / duplicate
            it, s, pos = _int_item(buf, pos, 5)
        out.append((it, s))
    assert pos == len(buf)
    return out


def _walk(enc_stream, body):
    return (walk_encoder_stream if enc_stream else walk_field_section)(body)


def _plain(pairs):
    return [(bytes(it), s) for it, s in pairs]


class Frames:
    """frames walked into one batch: ends[k] is the item count after frame
    k, bodies the frames' bytes.  other: the frames that are not what the
    reference's encoder writes for their own content -- a decoder test's
    hand-written input whose literal is raw where Huffman is shorter; the
    helpers' bytes for those say the same in the encoder's form, and that is
    what the frame is expected to come out as."""

    def __init__(self, frames_):
        pairs, self.ends, self.bodies, self.other = [], [], [], []
        for k, (enc_stream, body) in enumerate(frames_):
            w = _walk(enc_stream, body)
            mine = b"".join(item_bytes(it, s) for it, s in w)
            if mine != body:
                assert len(mine) < len(body)
                assert _plain(_walk(enc_stream, mine)) == _plain(w)
                self.other.append(k)
                body = mine
            pairs += w
            self.ends.append(len(pairs))
            self.bodies.append(body)
        self.batch = Batch([s for _, s in pairs], [it for it, _ in pairs])

    def check(self, out, out_off):
        assert out == b"".join(self.bodies)
        at = np.array([0] + self.ends)
        assert [int(x) for x in np.diff(out_off[at].astype(np.int64))] \
            == [len(b) for b in self.bodies]


@functools.lru_cache(maxsize=None)
def interop():
    fr = Frames([(sid == 0, body) for name in STREAMS
                 for sid, body in frames(name)])
    assert not fr.other
    return fr


@functools.lru_cache(maxsize=None)
def kats():
    with open(os.path.join(G, "kat_header_blocks.json")) as f:
        hb = json.load(f)["header_blocks"]
    with open(os.path.join(G, "kat_enc_stream.json")) as f:
        es = json.load(f)["enc_stream"]
    fr = []
    for k in hb:
        fr.append((False, bytes.fromhex(k["prefix"] + k["header"])))
        fr.append((True, bytes.fromhex(k["enc"])))
    fr += [(True, bytes.fromhex(k["enc_stream"])) for k in es]
    assert len(hb) > 3 and len(es) > 3
    fr = Frames(fr)
    # test_read_enc_stream.c:83 and :129, inputs written for the decoder: a
    # raw "Respect my authorata!" and a raw "aaa"
    assert [k - 2 * len(hb) for k in fr.other] \
        == [i for i, k in enumerate(es)
            if k["source"].rsplit(":", 1)[1] in ("83", "129")]
    assert len(fr.other) == 2
    return fr


# ---- shapes ----------------------------------------------------------------------------

def tokens(rng, n):
    return bytes(rng.choice(TOKEN) for _ in range(n))


def mixed_item(rng, i):
    """the item patterns of a field section, and the two without a literal
    over a string that is there all the same"""
    k = i % 7
    if k == 0:
        return item(rng.randrange(99), 4, 0x50, 7, 0)       # name reference
    if k == 1:
        return item(str_bits=3, str_first=0x20 | 0x10 * (i & 1))
    if k == 2:
        return item(str_bits=7)
    if k == 3:
        return item(rng.randrange(1 << rng.randrange(1, 32)), 6, 0x80)
    if k == 4:
        return item(str_bits=5, str_first=0x40)
    if k == 5:
        return item()                                        # nothing
    return item(rng.randrange(70000), 3, 0x08, 7, 0)         # post-base


@functools.lru_cache(maxsize=None)
def counts(n):
    rng = random.Random(2000 + n)
    strs = [tokens(rng, rng.randrange(0, 41)) if i % 3 else
            bytes(rng.randrange(256) for _ in range(rng.randrange(0, 20)))
            for i in range(n)]
    return Batch(strs, [mixed_item(rng, i) for i in range(n)])


@functools.lru_cache(maxsize=None)
def ints_only():
    rng = random.Random(31)
    its = [item(rng.randrange(1 << rng.randrange(1, 33)), 1 + i % 8,
                (0xFF << (1 + i % 8)) & 0xFF if i & 8 else 0)
           for i in range(TILE)]
    return Batch([b""] * TILE, its)


@functools.lru_cache(maxsize=None)
def ignored():
    """no literal anywhere: the strings' bytes are there and are ignored"""
    rng = random.Random(32)
    strs = [tokens(rng, rng.randrange(1, 40)) for _ in range(TILE)]
    its = [item(rng.randrange(5000), 5, 0x20) if i % 3 else item()
           for i in range(TILE)]
    b = Batch(strs, its)
    assert len(b.data) > 500 and b.total < 2 * TILE
    return b


@functools.lru_cache(maxsize=None)
def out_edge(total):
    """a dense tile whose output, integers included, is `total` bytes: 64
    raw literals (8-bit codes: Huffman is as long, so raw) each behind an
    integer of 1..6 bytes"""
    rng = random.Random(33)
    lens = [rng.randrange(38, 47) for _ in range(TILE)]
    strs = [bytes(rng.choice(B8) for _ in range(n)) for n in lens]
    ilen = [1] * TILE
    left = total - sum(1 + n for n in lens) - TILE
    assert 0 <= left <= 5 * TILE
    while left:
        i = rng.randrange(TILE)
        if ilen[i] < 6:
            ilen[i] += 1
            left -= 1
    # the smallest value of k bytes on a 4-bit prefix: 15 + 128^(k - 2)
    its = [item(3 if k == 1 else 15 + (1 << 7 * (k - 2)), 4, 0x50, 7, 0)
           for k in ilen]
    b = Batch(strs, its)
    assert b.total == total
    assert all(len(Q.enc_int(0x50, it.ival, 4)) == k for it, k in zip(its, ilen))
    return b


@functools.lru_cache(maxsize=None)
def span_edge(nbytes):
    """64 token strings of nbytes in all: 3072 is the stage exactly when the
    data is 16-byte aligned"""
    rng = random.Random(34)
    lens = [nbytes // TILE] * TILE
    for i in range(nbytes - sum(lens)):
        lens[i] += 1
    rng.shuffle(lens)
    strs = [tokens(rng, n) for n in lens]
    return Batch(strs, [mixed_item(rng, i) if i % 7 != 5 else item(str_bits=7)
                        for i in range(TILE)])


@functools.lru_cache(maxsize=None)
def dense_overflow():
    rng = random.Random(35)
    strs = [bytes(rng.choice(B30) for _ in range(40)) for _ in range(TILE)]
    its = [item(i, 6, 0xC0, 7, 0) if i % 2 else item(str_bits=5, str_first=0x80)
           for i in range(TILE)]
    return Batch(strs, its)


@functools.lru_cache(maxsize=None)
def long_value():
    rng = random.Random(36)
    strs = [tokens(rng, rng.randrange(0, 30)) for _ in range(TILE)]
    strs[29] = tokens(rng, 65535)
    its = [mixed_item(rng, i) for i in range(TILE)]
    its[29] = item(17, 4, 0x50, 7, 0)
    return Batch(strs, its)


@functools.lru_cache(maxsize=None)
def strings200():
    rng = random.Random(37)
    strs = [tokens(rng, 200) if i % 4 else
            bytes(rng.choice(B8) for _ in range(200)) for i in range(TILE)]
    its = [item(str_bits=(3, 5, 7)[i % 3], str_first=(0x30, 0xC0, 0)[i % 3])
           if i % 5 else item(1 << 20, 6, 0x40, 7, 0) for i in range(TILE)]
    return Batch(strs, its)


# name -> (builder, {residue: the paths its tiles must take})
SHAPES = {
    "n0": (lambda: counts(0), {0: [], 5: []}),
    "n1": (lambda: counts(1), {0: ["dense"], 5: ["dense"]}),
    "n63": (lambda: counts(63), {0: ["dense"], 5: ["dense"]}),
    "n64": (lambda: counts(64), {0: ["dense"], 5: ["dense"]}),
    "n65": (lambda: counts(65), {0: ["dense"] * 2, 5: ["dense"] * 2}),
    "n129": (lambda: counts(129), {0: ["dense"] * 3, 5: ["dense"] * 3}),
    "ints_only": (ints_only, {0: ["dense"], 5: ["dense"]}),
    "ignored": (ignored, {0: ["dense"], 5: ["dense"]}),
    "out3008": (lambda: out_edge(3008), {0: ["dense"], 5: ["dense"]}),
    "out3009": (lambda: out_edge(3009), {0: ["out"], 5: ["out"]}),
    "span3072": (lambda: span_edge(3072), {0: ["dense"], 5: ["in"]}),
    "span3073": (lambda: span_edge(3073), {0: ["in"], 5: ["in"]}),
    "dense_overflow": (dense_overflow, {0: ["lane"], 5: ["lane"]}),
    "long_value": (long_value, {0: ["in"], 5: ["in"]}),
    "strings200": (strings200, {0: ["in"], 5: ["in"]}),
}
RESIDUES = (0, 5)


# ---- the large batch, vectorised ----------------------------------------------------

def np_int_code(ival, ib, ifirst):
    """lsqpack_enc_int over arrays -> (bytes [n, 6], lengths [n])"""
    n = len(ival)
    v, mask = ival.astype(np.int64), (1 << ib.astype(np.int64)) - 1
    has, small = ib > 0, ival.astype(np.int64) < (1 << ib.astype(np.int64)) - 1
    B = np.zeros((n, 6), dtype=np.uint8)
    B[:, 0] = np.where(has, ifirst | np.where(small, v, mask), 0)
    L = has.astype(np.int64)
    r, cont = v - mask, has & ~small
    for j in range(1, 6):
        more = cont & (r >= 128)
        B[:, j] = np.where(cont, np.where(more, 0x80 | (r & 0x7F), r), 0)
        L += cont
        r = np.where(more, r >> 7, r)
        cont = more
    assert not cont.any()
    return B, L


def _spread(starts, lens):
    """indices starts[i] .. starts[i] + lens[i], concatenated"""
    tot = int(lens.sum())
    base = np.cumsum(lens) - lens
    return np.repeat(starts - base, lens) + np.arange(tot, dtype=np.int64)


def np_expect(data, off, ival, ib, ifirst, sb, sfirst):
    """the wire bytes of a batch of items given as arrays -> (out, out_off)"""
    off = off.astype(np.int64)
    n = len(ival)
    B, L = np_int_code(ival, ib, ifirst)
    slen = np.zeros(n, dtype=np.int64)
    lit = {}
    for p in (3, 5, 7):
        idx = np.flatnonzero(sb == p)
        if not len(idx):
            continue
        lens = off[idx + 1] - off[idx]
        soff = np.zeros(len(idx) + 1, dtype=np.uint32)
        np.cumsum(lens, out=soff[1:])
        sub = data[_spread(off[idx], lens)] if lens.sum() else \
            np.zeros(0, dtype=np.uint8)
        enc, eoff = O.encode_batch(np.concatenate([sub, np.zeros(16, np.uint8)]),
                                   soff, p)
        lit[p] = (idx, enc, eoff.astype(np.int64))
        slen[idx] = np.diff(eoff.astype(np.int64))
    ooff = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(L + slen, out=ooff[1:])
    out = np.zeros(int(ooff[-1]), dtype=np.uint8)
    for j in range(6):
        m = L > j
        out[ooff[:-1][m] + j] = B[m, j]
    for p, (idx, enc, eoff) in lit.items():
        at = ooff[idx] + L[idx]
        out[_spread(at, np.diff(eoff))] = enc[:eoff[-1]]
        out[at] |= sfirst[idx]
    return out, ooff.astype(np.uint32)


def arrays_of(items):
    a = qhuff.items_array(items).reshape(-1, 8)
    return (a[:, :4].copy().view(np.uint32).reshape(-1), a[:, 4], a[:, 5],
            a[:, 6], a[:, 7])


def big_batch(n, seed=5):
    """n items in a mixed pattern over strings of 0..8 bytes, as arrays ->
    (data, off, items uint8 [8n], fields)"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 9, n)
    off = np.zeros(n + 1, dtype=np.uint32)
    np.cumsum(lens, out=off[1:])
    alpha = np.frombuffer(TOKEN, dtype=np.uint8)
    data = alpha[rng.integers(0, len(alpha), int(off[-1]))]
    # one byte in 16 from the whole range: literals on both sides of raw
    wild = rng.integers(0, 16, len(data)) == 0
    data = np.where(wild, rng.integers(0, 256, len(data)), data).astype(np.uint8)
    kind = rng.integers(0, 6, n)
    ib = np.choose(kind, [4, 0, 0, 6, 0, 3]).astype(np.uint8)
    ifirst = np.choose(kind, [0x50, 0, 0, 0x80, 0, 0x08]).astype(np.uint8)
    sb = np.choose(kind, [7, 3, 7, 0, 0, 7]).astype(np.uint8)
    sfirst = np.choose(kind, [0, 0x30, 0, 0, 0, 0]).astype(np.uint8)
    ival = np.where(ib > 0, rng.integers(0, 1 << 32, n, dtype=np.uint64)
                    >> rng.integers(0, 32, n).astype(np.uint64), 0)
    ival = ival.astype(np.uint32)
    items = np.zeros((n, 8), dtype=np.uint8)
    items[:, :4] = ival.view(np.uint8).reshape(-1, 4)
    items[:, 4], items[:, 5], items[:, 6], items[:, 7] = ib, ifirst, sb, sfirst
    return data, off, items.reshape(-1), (ival, ib, ifirst, sb, sfirst)


# ---- CPU -------------------------------------------------------------------------------

def test_symbols_and_header():
    L = qhuff.lib()
    for name in ("qhuff_encode_wire_bound", "qhuff_items_check",
                 "qhuff_encode_wire", "qhuff_encode_wire_host"):
        assert hasattr(L, name) and name in qhuff.EXPORTS
    hdr = open(qhuff.HEADER).read()
    assert "#define QHUFF_FEATURE_ENCODE_WIRE 1" in hdr
    assert "#define QHUFF_ABI_VERSION 7" in hdr
    assert "struct qhuff_item {" in hdr
    assert C.sizeof(qhuff.Item) == 8 and C.alignment(qhuff.Item) == 4
    assert qhuff.Item.ival.offset == 0 and qhuff.Item.str_first.offset == 7
    off = np.zeros(2, dtype=np.uint32)
    p = off.ctypes.data_as(C.c_void_p)
    assert L.qhuff_encode_wire(None, None, None, None, 0, None, p,
                               None) == qhuff.EINVAL
    assert L.qhuff_encode_wire_host(None, None, None, None, 0, None,
                                    p) == qhuff.EINVAL


@pytest.mark.parametrize("in_bytes,n", [(0, 0), (1, 1), (7, 3), (4096, 64),
                                        (1 << 33, 1 << 20)])
def test_bound_formula(in_bytes, n):
    assert qhuff.encode_wire_bound(in_bytes, n) \
        == (30 * in_bytes + 7) // 8 + 13 * n + 16


def test_bound_covers_the_worst_item():
    # a 32-bit integer on a 1-bit prefix, and a raw literal of long codes
    s = bytes(B30[:1]) * 135
    w = item_bytes(item(0xFFFFFFFF, 1, 0xFE, 3, 0xF0), s)
    assert len(w) == 6 + 3 + 135
    assert len(w) <= 12 + len(s) <= qhuff.encode_wire_bound(len(s), 1)


def test_items_check_accepts_the_walker():
    for fr, least in ((interop(), 600), (kats(), 50)):
        b = fr.batch
        assert b.n > least
        assert qhuff.items_check(b.items) == (qhuff.OK, None)
        # the walker and the two helpers give the frames back
        fr.check(b"".join(b.want), b.want_off)
    used = {(it.int_bits, it.str_bits) for it in interop().batch.items}
    assert {(8, 0), (7, 0), (6, 0), (4, 7), (0, 3), (0, 7), (6, 7),
            (0, 5)} <= used
    assert qhuff.items_check([]) == (qhuff.OK, None)
    a = qhuff.items_array([item(5, 8), item(str_bits=7)])
    assert qhuff.lib().qhuff_items_check(a.ctypes.data_as(C.c_void_p), 2,
                                         None) == qhuff.OK
    for name, (make, _) in SHAPES.items():
        make()                          # (Batch checks its items)


@pytest.mark.parametrize("bad", [
    item(1, 9), item(1, 255), item(1, 4, 0x08), item(1, 4, 0x51),
    item(1, 8, 0x80), item(0, 0, 0x80), item(0, 0, 0x01),
    item(str_bits=1), item(str_bits=2), item(str_bits=4), item(str_bits=6),
    item(str_bits=8), item(str_bits=3, str_first=0x08),
    item(str_bits=3, str_first=0x01), item(str_bits=5, str_first=0x20),
    item(str_bits=7, str_first=0x80), item(str_first=0x80),
    item(str_first=0x01)], ids=lambda it: "%d_%d_%02x_%d_%02x" % (
        it.ival, it.int_bits, it.int_first, it.str_bits, it.str_first))
def test_items_check_rejects(bad):
    ok = [item(3, 4, 0x50, 7, 0), item(str_bits=3, str_first=0xF0),
          item(9, 8), item(1, 1, 0xFE), item(str_bits=5, str_first=0xC0),
          item()]
    assert qhuff.items_check(ok) == (qhuff.OK, None)
    for at in (0, 3, len(ok)):
        its = ok[:at] + [bad] + ok[at:]
        assert qhuff.items_check(its) == (qhuff.EINVAL, at)
    # the first offender is reported; a NULL `bad` is allowed
    its = ok + [bad, bad]
    assert qhuff.items_check(its) == (qhuff.EINVAL, len(ok))
    a = qhuff.items_array(its)
    assert qhuff.lib().qhuff_items_check(a.ctypes.data_as(C.c_void_p),
                                         len(its), None) == qhuff.EINVAL


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shapes_reach_their_paths(name):
    make, want = SHAPES[name]
    b = make()
    for r in RESIDUES:
        assert b.paths(r) == want[r], r
    if name == "ints_only":
        assert len(b.data) == 0 and b.total > TILE
    if name in ("out3008", "out3009"):
        assert b.total + 64 - STAGE == (0 if name == "out3008" else 1)
    if name == "span3072":
        assert limits._span(0, 0, len(b.data)) == STAGE
    if name == "long_value":
        assert len(b.strings[29]) == 65535 and len(b.want[29]) > 40000


def test_vectorised_expectation_matches_the_helpers():
    data, off, items, f = big_batch(700)
    out, ooff = np_expect(data, off, *f)
    raw = data.tobytes()
    its = [qhuff.Item.from_buffer_copy(items[8 * i:8 * i + 8].tobytes())
           for i in range(700)]
    b = Batch([raw[off[i]:off[i + 1]] for i in range(700)], its)
    assert np.array_equal(ooff, b.want_off)
    assert out.tobytes() == b"".join(b.want)
    assert len({(it.int_bits, it.str_bits) for it in its}) == 6
    # and over the shapes' items (every integer length, literals past 127)
    for name in ("n129", "strings200", "ints_only", "out3009"):
        b = SHAPES[name][0]()
        out, ooff = np_expect(b.data, b.off, *arrays_of(b.items))
        assert np.array_equal(ooff, b.want_off)
        assert out.tobytes() == b"".join(b.want)


# ---- GPU -------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def codec():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("gpu test without a GPU")
    c = qhuff.Codec(0)
    yield c
    c.close()


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if len(a) else np.zeros(1, a.dtype)).cuda()


def padded(data):
    return np.concatenate([data, np.zeros(16, dtype=np.uint8)])


def run_device(codec, b, stream=None):
    """-> (out bytes, out_off uint32 [n + 1])"""
    import torch
    out, oo = codec.encode_wire(dev(padded(b.data)), dev(b.off.view(np.int32)),
                                dev(qhuff.items_array(b.items)), stream=stream)
    assert out.numel() == qhuff.encode_wire_bound(len(b.data) + 16, b.n)
    if stream is not None:
        return out, oo
    torch.cuda.synchronize()
    assert codec.device_error() == 0
    return fetch(out, oo)


def fetch(out, oo):
    oo = oo.cpu().numpy().view(np.uint32)
    return out[:int(oo[-1])].cpu().numpy().tobytes(), oo


def check_both(codec, b):
    """the device form and the host form against the expectation"""
    want = b"".join(b.want)
    out, oo = run_device(codec, b)
    assert np.array_equal(oo, b.want_off)
    assert out == want
    hout, hoo = codec.encode_wire_host(b.data, b.off, b.items)
    assert np.array_equal(hoo, b.want_off)
    assert hout.tobytes() == want == out
    return out, oo


@pytest.mark.gpu
def test_rebuild_interop_streams_in_one_launch(codec):
    """every frame of the three reference streams, encoder stream and field
    sections alike, from one launch"""
    fr = interop()
    assert len(fr.bodies) > 30 and fr.batch.n > 600
    out, oo = check_both(codec, fr.batch)
    fr.check(out, oo)
    whole = b"".join(body for name in STREAMS
                     for _, body in Q.read_interop(
                         data_file(name + ".out.256.100.1")))
    assert out == whole


@pytest.mark.gpu
def test_rebuild_reference_kats(codec):
    fr = kats()
    out, oo = check_both(codec, fr.batch)
    fr.check(out, oo)


def int_cases():
    with open(os.path.join(G, "kat_int.json")) as f:
        kat = [k for k in json.load(f)["dec_int"]
               if k["retval"] == 0 and int(k["decoded"]) < 1 << 32]
    assert len(kat) >= 3
    cases = []
    for k in kat:
        enc, p = bytes.fromhex(k["encoded"]), k["prefix_bits"]
        cases.append((int(k["decoded"]), p, enc[0] & ~((1 << p) - 1) & 0xFF))
    for p in range(1, 9):
        mask = (1 << p) - 1
        vals = {mask - 1, mask, mask + 1, mask + 127, mask + 128, 0xFFFFFFFF}
        for e in (14, 21, 28):          # the continuation edges
            vals |= {mask + (1 << e) - 1, mask + (1 << e)}
        for v in sorted(vals):
            cases.append((v, p, 0))
            if p < 8:
                cases.append((v, p, (0xFF << p) & 0xFF))
                cases.append((v, p, 0x80))
    return cases


@pytest.mark.gpu
def test_integers_alone(codec):
    cases = int_cases()
    assert Q.enc_int(0xFE, 0xFFFFFFFF, 1) == b"\xff\xfe\xff\xff\xff\x0f"
    assert (0xFFFFFFFF, 1, 0xFE) in cases
    b = Batch([b""] * len(cases), [item(v, p, f) for v, p, f in cases])
    assert len(b.want[:3]) == 3 and b.paths(0) == ["dense"] * len(b.paths(0))
    out, oo = check_both(codec, b)
    sizes = set()
    for i, (v, p, f) in enumerate(cases):
        w = out[oo[i]:oo[i + 1]]
        assert w == Q.enc_int(f, v, p), (v, p, f)
        assert qhuff.dec_int(w, p) == (qhuff.OK, v, len(w))
        assert w[0] & ~((1 << p) - 1) & 0xFF == f
        sizes.add(len(w))
    assert sizes == {1, 2, 3, 4, 5, 6}
    with open(os.path.join(G, "kat_int.json")) as f:
        for k in json.load(f)["dec_int"][:3]:
            # the reference's own vectors are the minimal coding
            p, enc = k["prefix_bits"], bytes.fromhex(k["encoded"])
            i = cases.index((int(k["decoded"]), p, enc[0] & ~((1 << p) - 1) & 0xFF))
            assert out[oo[i]:oo[i + 1]] == enc


def literal_cases(p):
    """(kind, string) for payload lengths on both sides of the prefix and of
    its second continuation byte: Huffman a byte shorter than raw, as long
    (raw), longer (raw)"""
    rng = random.Random(50 + p)
    mask = (1 << p) - 1
    out = []
    for L in (mask - 1, mask, mask + 127, mask + 128):
        shorter = limits.with_bits(L + 1, 8 * L, rng)
        assert O.enc_str_size(shorter) == L
        equal = limits.with_bits(L, 8 * L, rng)
        assert O.enc_str_size(equal) == L
        longer = bytes(rng.choice(B30) for _ in range(L))
        out += [("shorter", shorter, L, 1), ("equal", equal, L, 0),
                ("longer", longer, L, 0)]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("p", [3, 5, 7])
def test_literals_with_instruction_bits(codec, p):
    cases = literal_cases(p)
    first = allowed_first(p)
    assert first == {3: 0xF0, 5: 0xC0, 7: 0}[p]
    # all of them in one tile (p = 7: the long codes overflow the dense
    # stream, every item by its lane), then each kind alone
    groups = [cases] + [[c for c in cases if c[0] == kind]
                        for kind in ("shorter", "equal", "longer")]
    seen = set()
    for grp in groups:
        b = Batch([c[1] for c in grp], [item(str_bits=p, str_first=first)] * len(grp))
        seen.add(b.paths(0)[0])
        out, oo = check_both(codec, b)
        for i, (kind, s, L, huff) in enumerate(grp):
            w = out[oo[i]:oo[i + 1]]
            hdr = Q.enc_int(first | (huff << p), L, p)
            assert w[:len(hdr)] == hdr and len(w) == len(hdr) + L, (kind, L)
            assert w == O.enc_enc_str(p, s, first)
            lit = Q.read_literal(w, 0, p)
            assert lit["huffman"] == huff and lit["end"] == len(w)
            assert (O.huff_decode(lit["payload"])[1] if huff
                    else lit["payload"]) == s
    assert "dense" in seen and (p != 7 or "lane" in seen)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 129])
def test_counts(codec, n):
    b = counts(n)
    out, oo = check_both(codec, b)
    assert len(oo) == n + 1 and oo[0] == 0
    if n >= 63:
        assert sum(1 for w in b.want if not w) >= n // 7
        assert {len(Q.enc_int(0, it.ival, it.int_bits)) for it in b.items
                if it.int_bits} >= {1, 2, 3, 4, 5}


@pytest.mark.gpu
def test_every_wave_three_tiles(codec):
    import torch
    waves = codec.grid_waves(qhuff.KIND_ENCODE)
    n = 3 * TILE * waves + 37
    data, off, items, f = big_batch(n)
    want, want_off = np_expect(data, off, *f)
    assert qhuff.items_check(items) == (qhuff.OK, None)
    out, oo = codec.encode_wire(dev(padded(data)), dev(off.view(np.int32)),
                                dev(items))
    torch.cuda.synchronize()
    assert codec.device_error() == 0
    out, oo = fetch(out, oo)
    assert np.array_equal(oo, want_off)
    assert np.array_equal(np.frombuffer(out, dtype=np.uint8), want)


@pytest.mark.gpu
@pytest.mark.parametrize("p", [3, 5, 7])
def test_uniform_literals_equal_encode_batch(codec, p):
    """no integers, str_first = 0, one prefix width: qhuff_encode_batch(p)"""
    import torch
    rng = random.Random(60 + p)
    strs = [tokens(rng, rng.randrange(0, 64)) if i % 4 else
            bytes(rng.randrange(256) for _ in range(rng.randrange(0, 40)))
            for i in range(5 * TILE + 11)]
    strs[100] = tokens(rng, 4000)
    b = Batch(strs, [item(str_bits=p)] * len(strs))
    d, o = dev(padded(b.data)), dev(b.off.view(np.int32))
    ref, roo = codec.encode(d, o, p)
    torch.cuda.synchronize()
    ref, roo = fetch(ref, roo)
    out, oo = check_both(codec, b)
    assert np.array_equal(oo, roo) and out == ref


def field_sections():
    """the golden streams' field sections as one batch -> (Frames, strings
    of the literal items, in order)"""
    fr = Frames([(False, body) for name in STREAMS
                 for sid, body in frames(name) if sid != 0])
    assert not fr.other
    lits = [s for it, s in zip(fr.batch.items, fr.batch.strings)
            if it.str_bits]
    return fr, lits


@pytest.mark.gpu
def test_device_round_trip(codec):
    """encode_wire -> scan_field_section (a host copy of the bytes) ->
    decode_wire on the device buffer: the strings again"""
    import torch
    fr, strings = field_sections()
    b = fr.batch
    out, oo = codec.encode_wire(dev(padded(b.data)), dev(b.off.view(np.int32)),
                                dev(qhuff.items_array(b.items)))
    torch.cuda.synchronize()
    host, hoo = fetch(out, oo)
    lits = []
    for k, end in enumerate(fr.ends):
        a = int(hoo[fr.ends[k - 1] if k else 0])
        rc, ls = qhuff.scan_field_section(host[a:int(hoo[end])], a)
        assert rc == qhuff.OK
        lits += ls
    assert len(lits) == len(strings) > 200
    assert qhuff.literals_check(lits) == (qhuff.OK, None)
    dec, doo, st = codec.decode_wire(out, dev(qhuff.literals_array(lits)),
                                     qhuff.MAX_STRLEN,
                                     bound=qhuff.literals_bound(lits))
    torch.cuda.synchronize()
    assert codec.device_error() == 0
    assert not st.cpu().numpy().any()
    doo = doo.cpu().numpy().view(np.uint32)
    dec = dec.cpu().numpy()
    assert [dec[doo[i]:doo[i + 1]].tobytes() for i in range(len(lits))] \
        == strings


def wire_specs(b, k, r_in, out_bytes):
    return [("in", len(b.data), r_in),
            ("in_off", 4 * (b.n + 1), 4 * (k % 4)),
            ("items", 8 * b.n, 4 + 8 * (k % 2)),          # 4 mod 8
            ("out", out_bytes, (7 * k + 3) % 16),
            ("out_off", 4 * (b.n + 1), 4 * ((k + 1 + k // 4) % 4))]


def contract_call(codec, b, host, k, r_in, fill, back=0, items=None,
                  out_bytes=None):
    """one call with every buffer at its contractual size in a dirty guarded
    arena -> (arena, image after)"""
    import torch
    ar = Arena(wire_specs(b, k, r_in,
                          b.total if out_bytes is None else out_bytes),
               seed=9000 + 16 * k + r_in)
    ar.put("in", b.data)
    ar.put("in_off", (b.off.astype(np.uint64) + back).astype(np.uint32))
    ar.put("items", qhuff.items_array(b.items) if items is None else items)
    ar.neighbours("in", fill)
    ar.commit(not host)
    assert ar.addr("items") % 8 == 4
    if host:
        rc = qhuff.lib().qhuff_encode_wire_host(
            codec._ctx, ar.addr("in", back), ar.addr("in_off"),
            ar.addr("items"), b.n, ar.addr("out"), ar.addr("out_off"))
        assert rc == qhuff.OK
    else:
        codec.encode_wire_into(ar.ptr("in", back), ar.ptr("in_off"),
                               ar.ptr("items"), b.n, ar.ptr("out"),
                               ar.ptr("out_off"))
        torch.cuda.synchronize()
        assert codec.device_error() == 0
    return ar, ar.after()


@pytest.mark.gpu
@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
@pytest.mark.parametrize("r_in", RESIDUES)
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_tile_paths_and_buffer_contract(codec, name, r_in, host):
    """each shape at each residue of the input pointer, `out` exactly
    out_off[n] bytes, the items at 4 mod 8, plain and with every offset's
    top bits set (`in` 0xF0000000 below the bytes): the expected bytes and
    offsets, and nothing else written; the device form then over random
    descriptor bytes, `out` at the bound"""
    make, want = SHAPES[name]
    b = make()
    assert b.paths(r_in) == want[r_in]
    assert int(b.off[-1]) + HIGH < 1 << 32
    for k, fill in enumerate(FILLS):
        k += 3 * host
        back = HIGH if k % 2 else 0
        ar, img = contract_call(codec, b, host, k, r_in, fill, back)
        assert np.array_equal(ar.get(img, "out_off", np.uint32), b.want_off)
        assert ar.get(img, "out").tobytes() == b"".join(b.want)
        ar.check(img, {"out": b.total, "out_off": 4 * (b.n + 1)})
    if host:
        return
    rnd = np.random.default_rng(77 + r_in).integers(0, 256, 8 * b.n,
                                                    dtype=np.uint8)
    ar, img = contract_call(codec, b, False, 1, r_in, "random", items=rnd,
                            out_bytes=b.bound)
    oo = ar.get(img, "out_off", np.uint32).astype(np.int64)
    assert oo[0] == 0 and (np.diff(oo) >= 0).all() and oo[-1] <= b.bound
    # an item's size: at most 12 + its literal's payload
    lens = np.diff(b.off.astype(np.int64))
    assert (np.diff(oo) <= 12 + lens).all()
    ar.check(img, {"out": int(oo[-1]), "out_off": 4 * (b.n + 1)})


@pytest.mark.gpu
def test_out_of_rule_items_leave_the_others_alone(codec):
    """every other item out of rule (random bytes): the items between them
    come out as they must"""
    import torch
    b = counts(129)
    raw = qhuff.items_array(b.items).reshape(-1, 8).copy()
    rnd = np.random.default_rng(3).integers(0, 256, raw.shape, dtype=np.uint8)
    raw[1::2] = rnd[1::2]
    out, oo = codec.encode_wire(dev(padded(b.data)), dev(b.off.view(np.int32)),
                                dev(raw.reshape(-1)))
    torch.cuda.synchronize()
    assert codec.device_error() == 0
    out, oo = fetch(out, oo)
    assert (np.diff(oo.astype(np.int64)) >= 0).all()
    for i in range(0, b.n, 2):
        assert out[oo[i]:oo[i + 1]] == b.want[i], i


@pytest.mark.gpu
def test_host_entry_checks_the_item_rule(codec):
    b = counts(65)
    its = list(b.items)
    its[40] = item(1, 4, 0x01)
    assert qhuff.items_check(its) == (qhuff.EINVAL, 40)
    with pytest.raises(qhuff.QhuffError):
        codec.encode_wire_host(b.data, b.off, its)
    # nothing is written
    out = np.full(b.bound, 0xA5, dtype=np.uint8)
    oo = np.full(b.n + 1, 0xA5A5A5A5, dtype=np.uint32)
    a = qhuff.items_array(its)
    rc = qhuff.lib().qhuff_encode_wire_host(
        codec._ctx, b.data.ctypes.data, b.off.ctypes.data, a.ctypes.data, b.n,
        out.ctypes.data, oo.ctypes.data)
    assert rc == qhuff.EINVAL
    assert (out == 0xA5).all() and (oo == 0xA5A5A5A5).all()
    # and the context is as good as before
    check_both(codec, b)


@pytest.mark.gpu
def test_ordering_timing_and_variant(codec):
    """two calls back to back on two streams of one context; one between two
    encode_batch launches; timed as an encode; the batch kernel's variant
    and hint untouched"""
    import torch
    a, b = interop().batch, counts(129)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        ra = run_device(codec, a, stream=s1)
    with torch.cuda.stream(s2):
        rb = run_device(codec, b, stream=s2)
    torch.cuda.synchronize()
    assert codec.device_error() == 0
    for r, x in ((ra, a), (rb, b)):
        out, oo = fetch(*r)
        assert np.array_equal(oo, x.want_off) and out == b"".join(x.want)

    data, off = qhuff.synth_batch(5000, seed=3)
    want, want_off = O.encode_batch(data, off, 0)
    d, o = dev(padded(data)), dev(off.view(np.int32))
    cur = torch.cuda.current_stream()
    for variant in (0, 1):
        codec.batch_hint(qhuff.KIND_ENCODE, variant)
        codec.encode(d, o)
        assert codec.kernel_variant(qhuff.KIND_ENCODE) == variant
        codec.timing(True)
        try:
            codec.timing_read()
            e1 = codec.encode(d, o)
            v = codec.kernel_variant(qhuff.KIND_ENCODE)
            # a hint for the next encode_batch launch: not this call's
            codec.batch_hint(qhuff.KIND_ENCODE, variant)
            rw = run_device(codec, a, stream=cur)
            assert codec.kernel_variant(qhuff.KIND_ENCODE) == v
            e2 = codec.encode(d, o)
            assert codec.kernel_variant(qhuff.KIND_ENCODE) == variant
            torch.cuda.synchronize()
            assert codec.device_error() == 0
            t = codec.timing_read()
        finally:
            codec.timing(False)
        assert [k for k, _ in t] == [qhuff.KIND_ENCODE] * 3
        assert all(us > 0 for _, us in t)
        out, oo = fetch(*rw)
        assert np.array_equal(oo, a.want_off) and out == b"".join(a.want)
        for out, oo in (e1, e2):
            out, oo = fetch(out, oo)
            assert np.array_equal(oo, want_off)
            assert np.array_equal(np.frombuffer(out, dtype=np.uint8), want)
