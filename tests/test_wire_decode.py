"""qhuff_decode_wire / qhuff_decode_wire_host: QPACK literals decoded where
they lie in wire data (include/qhuff.h), and qhuff_literals_check, the order
rule the device call relies on.

Expectations: Codec.decode_literals_host(buf, lits, max_len) -- the gather /
decode / interleave path that was there before -- and, where named, the
oracle's decode of a Huffman payload.  Every GPU test checks
qhuff.literals_check before it hands descriptors to the device call, and the
shape builders recompute from the descriptors which 64-literal tiles fit the
kernels' 3 KB stage, so that each shape is known to reach the path it is
named for (at every alignment of the buffer)."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import _paths  # noqa: F401
import limits
import oracle_lib as O
import qhuff
import qpack_frames as Q
from test_buffer_contract import FILLS, Arena, Ptr
from test_frames import all_literals, field_line, static_name_len

STAGE = 3072                # qhuff_pipeline.h kStageCap
TILE = 64
HIGH = 0xF0000000
TOKEN = qhuff.TOKEN_ALPHABET


# ---- shapes ---------------------------------------------------------------------

def tile_staged(lits, r):
    """per 64-literal tile: does its 16-byte-aligned wire span, first
    literal's pos to last literal's end, fit the stage when the buffer's
    address is r mod 16?"""
    out = []
    for a in range(0, len(lits), TILE):
        t = lits[a:a + TILE]
        lo = (r + t[0].pos) & ~15
        hi = (r + t[-1].pos + t[-1].len + 15) & ~15
        out.append(hi - lo <= STAGE)
    return out


def paths(lits):
    """(some tile staged, some tile not) -- the same at every residue"""
    per = [tile_staged(lits, r) for r in range(16)]
    assert all(p == per[0] for p in per), "a tile on the stage's edge"
    return any(per[0]), not all(per[0])


def lit(pos, payload, huffman, kind=qhuff.LIT_VALUE):
    return qhuff.Literal(pos, len(payload), int(huffman), 7, kind, 0, 0)


class Shape:
    def __init__(self, buf, lits, staged=None, unstaged=None, residue=None):
        self.buf, self.lits = bytes(buf), list(lits)
        assert qhuff.literals_check(self.lits) == (qhuff.OK, None)
        if residue is not None:
            # a tile on the stage's edge: staged at this residue of the
            # buffer's address and at no other
            assert len(self.lits) == TILE
            assert [r for r in range(16) if tile_staged(self.lits, r)[0]] \
                == [residue]
        elif self.lits:
            s, u = paths(self.lits)
            assert staged is None or s == staged
            assert unstaged is None or u == unstaged
        self._want = {}

    def want(self, codec, max_len=None):
        """the expectation, once per limit"""
        if max_len not in self._want:
            outs, st = codec.decode_literals_host(self.buf, self.lits, max_len)
            self._want[max_len] = (outs, [int(s) for s in st])
        return self._want[max_len]


def mixed(rng, i):
    """test_gpu_decode_literals_with_errors' literals: 0-40 bytes, one in
    three raw, one in five of the rest a raw payload flagged Huffman"""
    s = bytes(rng.randrange(256) for _ in range(rng.randrange(0, 41)))
    if i % 3:
        s = O.huffman_enc(s[:30]) if i % 5 else s
    return s, i % 3 != 0


@functools.lru_cache(maxsize=None)
def counts(n):
    rng = random.Random(1000 + n)
    buf, lits = b"", []
    for i in range(n):
        if i:
            buf += bytes(rng.randrange(256) for _ in range(rng.randrange(4)))
        s, h = mixed(rng, i)
        lits.append(lit(len(buf), s, h))
        buf += s
    return Shape(buf, lits, staged=n > 0 or None, unstaged=False if n else None)


@functools.lru_cache(maxsize=None)
def all_raw():
    rng = random.Random(7)
    buf, lits = b"", []
    for i in range(TILE):
        buf += bytes(rng.randrange(256) for _ in range(rng.randrange(4))) \
            if i else b""
        s = bytes(rng.randrange(256) for _ in range(rng.randrange(0, 41)))
        lits.append(lit(len(buf), s, False))
        buf += s
    return Shape(buf, lits, staged=True, unstaged=False)


@functools.lru_cache(maxsize=None)
def all_empty():
    rng = random.Random(8)
    buf, lits = b"", []
    for i in range(TILE):
        buf += bytes(rng.randrange(256) for _ in range(rng.randrange(4))) \
            if i else b""
        lits.append(lit(len(buf), b"", i % 2 == 0))
    buf += b"\x00"              # (the buffer is not empty)
    return Shape(buf, lits, staged=True, unstaged=False)


@functools.lru_cache(maxsize=None)
def far_apart():
    """64 ten-byte literals 100 bytes apart: past the stage by gaps alone"""
    rng = random.Random(9)
    buf, lits = bytearray(), []
    for i in range(TILE):
        s = bytes(rng.choice(TOKEN) for _ in range(16))
        s = O.huffman_enc(s)[:10] if i % 2 else s[:10]
        s = s + b"\xff" * (10 - len(s))
        buf += bytes(rng.randrange(256) for _ in range(100 * i - len(buf)))
        lits.append(lit(len(buf), s, i % 2 == 1))
        buf += s
    assert lits[1].pos - lits[0].pos == 100 and all(l.len == 10 for l in lits)
    return Shape(buf, lits, staged=False, unstaged=True)


@functools.lru_cache(maxsize=None)
def big_output():
    """a staged tile whose output passes the 3 KB output stage: the arena is
    copied out of line"""
    rng = random.Random(12)
    buf, lits, total = b"", [], 0
    for i in range(TILE):
        s = bytes(rng.choice(TOKEN) for _ in range(60))
        total += 47 if i % 4 == 0 else 60
        s = s[:47] if i % 4 == 0 else O.huffman_enc(s)
        lits.append(lit(len(buf), s, i % 4 != 0))
        buf += s
    assert total + 64 > STAGE
    return Shape(buf, lits, staged=True, unstaged=False)


@functools.lru_cache(maxsize=None)
def long_text():
    rng = random.Random(10)
    return bytes(rng.choice(TOKEN) for _ in range(65535))


@functools.lru_cache(maxsize=None)
def long_one(huffman, alone):
    """one literal of 65,535 decoded bytes, alone or in the middle of a
    tile of short ones"""
    rng = random.Random(11 + 2 * huffman + alone)
    big = O.huffman_enc(long_text()) if huffman else long_text()
    if huffman:
        assert O.huff_decode(big) == (O.OK, long_text())
    buf, lits = b"", []
    for i in range(1 if alone else TILE):
        if i == (0 if alone else 29):
            s, h = big, huffman
        else:
            s, h = mixed(rng, i)
        lits.append(lit(len(buf), s, h))
        buf += s + (b"" if alone else bytes(rng.randrange(4)))
    return Shape(buf, lits, staged=False, unstaged=True)


@functools.lru_cache(maxsize=None)
def stage_edge(longest):
    """64 adjacent literals (no byte between them) that span exactly 3072
    bytes: staged when the buffer is 16-byte aligned, in units at any other
    residue.  Three in four are Huffman strings of 5-bit codes (they decode
    to 8/5 of their length and fill their arena slots), the rest raw.
    longest 66: twenty 66-byte literals, the fixed-stride arena's limit;
    67: one of them a byte longer, and the variable arena packed to 3072
    bytes of input."""
    rng = random.Random(longest)
    lens = [66] * 20 + [40] * 36 + [39] * 8
    if longest == 67:
        lens[0], lens[20] = 67, 39
    assert sum(lens) == STAGE and max(lens) == longest
    rng.shuffle(lens)
    buf, lits = b"", []
    for i, n in enumerate(lens):
        raw = i % 4 == 3 and n < 66
        s = bytes(rng.randrange(256) for _ in range(n)) if raw \
            else limits.maxexp(n, rng)
        lits.append(lit(len(buf), s, not raw))
        buf += s
    assert len(buf) == STAGE
    return Shape(buf, lits, residue=0)


SHAPES = {"edge3072_fix66": lambda: stage_edge(66),
          "edge3072_var67": lambda: stage_edge(67),
          "n0": lambda: counts(0), "n1": lambda: counts(1),
          "n63": lambda: counts(63), "n64": lambda: counts(64),
          "n65": lambda: counts(65), "n129": lambda: counts(129),
          "all_raw": all_raw, "all_empty": all_empty, "far_apart": far_apart,
          "big_output": big_output,
          "raw64k": lambda: long_one(False, True),
          "huff64k": lambda: long_one(True, True),
          "raw64k_mid": lambda: long_one(False, False),
          "huff64k_mid": lambda: long_one(True, False)}


@functools.lru_cache(maxsize=None)
def golden():
    buf, lits, _ = all_literals()
    return Shape(buf, lits, staged=True, unstaged=True)


@functools.lru_cache(maxsize=None)
def a_payload(n):
    return O.huffman_enc(b"a" * n)


@functools.lru_cache(maxsize=None)
def clamp(front):
    """test_gpu_decode_clamp's seventeen cases in one buffer.  front: None,
    or the number of a 64-literal tile's lanes in front of each case --
    filler literals bring every case's first literal to that lane, so that
    with 63 a case's NAME is a tile's lane 63 and its VALUE the next tile's
    lane 0, and a lone VALUE a lane 63.  -> (Shape, expected statuses)"""
    nm_h = O.huffman_enc(b"nm")
    cases = [(field_line(0x20, 3, b"nm"), 65533, [0, 0]),
             (field_line(0x20, 3, b"nm"), 65534, [0, 1]),
             (field_line(0x20, 3, b"nm"), 65535, [0, 1]),
             (field_line(0x20, 3, b"nm"), 65536, [0, 1]),
             (field_line(0x20, 3, nm_h, huffman=True), 65533, [0, 0]),
             (field_line(0x20, 3, nm_h, huffman=True), 65534, [0, 1]),
             (field_line(0x20, 3, b"nm"), 10, [0, 0]),
             (field_line(0x20, 3, b"nm"), 0, [0, 0]),
             (b"\x50", 65535 - static_name_len(0), [0]),
             (b"\x50", 65536 - static_name_len(0), [1]),
             (b"\x52", 65535 - static_name_len(2), [0]),
             (b"\x52", 65536 - static_name_len(2), [1]),
             (Q.enc_int(0x50, 31, 4), 65535 - static_name_len(31), [0]),
             (Q.enc_int(0x50, 31, 4), 65536 - static_name_len(31), [1]),
             (b"\x45", 65535, [0]),
             (b"\x45", 65536, [1]),
             (b"\x02", 65535, [0])]
    assert len(cases) == 17
    buf, lits, status, where = b"", [], [], []

    def add(blk, st):
        nonlocal buf, lits, status
        rc, ls = qhuff.scan_field_section(blk, len(buf))
        assert rc == qhuff.OK and len(ls) == len(st)
        buf += blk
        lits += ls
        status += st

    k = 0
    for head, n, st in cases:
        while front is not None and len(lits) % TILE != front:
            # one short VALUE literal behind a dynamic name reference
            add(b"\x00\x00\x45" + field_line(0, 7, b"v%d" % k), [0])
            k += 1
        where.append(len(lits) % TILE)
        add(b"\x00\x00" + head
            + field_line(0, 7, a_payload(n), huffman=True), st)
    if front is not None:
        assert where == [front] * 17
    return Shape(buf, lits), status


def rebased(lits, base):
    return [qhuff.Literal(l.pos + base, l.len, l.huffman, l.prefix_bits,
                          l.kind, l.hdr_len, l.instr + base) for l in lits]


# ---- CPU -------------------------------------------------------------------------

def test_symbols_and_header():
    L = qhuff.lib()
    for name in ("qhuff_literals_check", "qhuff_decode_wire",
                 "qhuff_decode_wire_host"):
        assert hasattr(L, name) and name in qhuff.EXPORTS
    hdr = open(qhuff.HEADER).read()
    assert "#define QHUFF_FEATURE_WIRE 1" in hdr
    assert "#define QHUFF_ABI_VERSION 7" in hdr
    off = np.zeros(2, dtype=np.uint32)
    p = off.ctypes.data_as(C.c_void_p)
    assert L.qhuff_decode_wire(None, None, None, 0, 0, None, p, None,
                               None) == qhuff.EINVAL
    assert L.qhuff_decode_wire_host(None, None, None, 0, 0, None, p,
                                    None) == qhuff.EINVAL


def test_literals_check_accepts_the_scanners():
    buf, lits, _ = all_literals()
    assert len(lits) == 341
    assert qhuff.literals_check(lits) == (qhuff.OK, None)
    assert qhuff.literals_check(rebased(lits, HIGH)) == (qhuff.OK, None)
    assert qhuff.literals_check([]) == (qhuff.OK, None)
    # adjacent literals: no byte between them
    adj = [lit(0, b"abc", False), lit(3, b"", True), lit(3, b"de", True)]
    assert qhuff.literals_check(adj) == (qhuff.OK, None)
    # a NULL `bad` is allowed
    a = qhuff.literals_array(adj)
    assert qhuff.lib().qhuff_literals_check(
        a.ctypes.data_as(C.c_void_p), 3, None) == qhuff.OK
    a = qhuff.literals_array(adj[::-1])
    assert qhuff.lib().qhuff_literals_check(
        a.ctypes.data_as(C.c_void_p), 3, None) == qhuff.EINVAL


def test_literals_check_rejects():
    _, lits, _ = all_literals()
    lits = lits[:40]
    sw = list(lits)
    sw[10], sw[11] = sw[11], sw[10]
    assert qhuff.literals_check(sw) == (qhuff.EINVAL, 11)
    ov = list(lits)
    l = ov[20]
    assert l.len > 0
    ov[21] = qhuff.Literal(l.pos + l.len - 1, 5, 1, 7, 2, 0, 0)
    assert qhuff.literals_check(ov) == (qhuff.EINVAL, 21)
    hd = list(lits)
    hd[0] = qhuff.Literal(1, 2, 0, 7, 2, 2, 0)           # hdr_len > pos
    assert qhuff.literals_check(hd) == (qhuff.EINVAL, 0)
    ins = list(lits)
    l = ins[30]
    ins[30] = qhuff.Literal(l.pos, l.len, l.huffman, l.prefix_bits, l.kind,
                            l.hdr_len, l.pos - l.hdr_len + 1)
    assert qhuff.literals_check(ins) == (qhuff.EINVAL, 30)
    ok = list(lits)
    ok[30] = qhuff.Literal(l.pos, l.len, l.huffman, l.prefix_bits, l.kind,
                           l.hdr_len, l.pos - l.hdr_len)
    assert qhuff.literals_check(ok) == (qhuff.OK, None)
    # an end past 32 bits
    assert qhuff.literals_check([qhuff.Literal(0xfffffff0, 16, 0, 7, 2, 0, 0)]) \
        == (qhuff.EINVAL, 0)
    assert qhuff.literals_check([qhuff.Literal(0xfffffff0, 15, 0, 7, 2, 0, 0)]) \
        == (qhuff.OK, None)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shapes_reach_their_paths(name):
    """(CPU) the builders' own assertions; the golden streams hold a staged
    and an unstaged tile, the clamp layouts put the cases where they say"""
    s = SHAPES[name]()
    assert s.lits or name == "n0"
    if name == "n0":
        g = golden()
        assert len(g.lits) == 341 and paths(g.lits) == (True, True)
        assert tile_staged(g.lits, 0).count(False) == 1
        for front in (None, 63, 62):
            sh, st = clamp(front)
            assert len(sh.lits) == len(st)
            # every case's tiles are past the stage
            assert paths(sh.lits)[1]


# ---- GPU ---------------------------------------------------------------------------

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
    a = np.array(a)
    return torch.from_numpy(a if len(a) else np.zeros(1, a.dtype)).cuda()


def split(out, out_off, status, n):
    oo = out_off.cpu().numpy().view(np.uint32)
    o = out.cpu().numpy()
    assert oo[0] == 0 and (np.diff(oo.astype(np.int64)) >= 0).all()
    return ([o[oo[i]:oo[i + 1]].tobytes() for i in range(n)],
            [int(s) for s in status.cpu().numpy()[:n]])


def run_device(codec, shape, max_len=None, stream=None):
    import torch
    assert qhuff.literals_check(shape.lits)[0] == qhuff.OK
    n = len(shape.lits)
    buf = dev(np.frombuffer(shape.buf, dtype=np.uint8))
    lits = dev(qhuff.literals_array(shape.lits))
    out, oo, st = codec.decode_wire(buf, lits, max_len, stream=stream,
                                    bound=qhuff.literals_bound(shape.lits))
    if stream is None:
        torch.cuda.synchronize()
        assert codec.device_error() == 0
    return out, oo, st, n


def check_both(codec, shape, max_len=None):
    """device call and host call against the expectation -> (outs, status)"""
    want = shape.want(codec, max_len)
    got = split(*run_device(codec, shape, max_len))
    assert got[1] == want[1]
    assert got[0] == want[0]
    outs, st = codec.decode_wire_host(shape.buf, shape.lits, max_len)
    assert [int(s) for s in st] == want[1]
    assert outs == want[0]
    for o, s in zip(*want):
        assert s in (0, 1) and (s == 0 or o == b"")
    return want


@pytest.mark.gpu
def test_golden_streams(codec):
    """all 341 literals of the three interop streams in one call"""
    g = golden()
    outs, status = check_both(codec, g)
    assert not any(status)
    n_huff = 0
    for l, o in zip(g.lits, outs):
        payload = g.buf[l.pos:l.pos + l.len]
        if l.huffman:
            st, w = O.huff_decode(payload)
            assert st == O.OK and o == w
            n_huff += 1
        else:
            assert o == payload
    assert n_huff > 100
    # field-section use: nothing is near the limit
    assert not any(check_both(codec, g, qhuff.MAX_STRLEN)[1])


@pytest.mark.gpu
@pytest.mark.parametrize("max_len", [12, 30])
def test_golden_streams_small_limit(codec, max_len):
    """a limit among the strings' own lengths: the staged tiles' limit code,
    its out-of-line path (a value within its name's bound of the limit)
    included, against the host loop's"""
    g = golden()
    status = check_both(codec, g, max_len)[1]
    assert 0 < sum(status) < len(status)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["n0", "n1", "n63", "n64", "n65", "n129",
                                  "all_raw", "all_empty"])
def test_counts(codec, name):
    s = SHAPES[name]()
    outs, status = check_both(codec, s)
    for l, o, st in zip(s.lits, outs, status):
        payload = s.buf[l.pos:l.pos + l.len]
        if l.huffman:
            ost, w = O.huff_decode(payload)
            assert st == (0 if ost == O.OK else 1)
            assert o == (w if ost == O.OK else b"")
        else:
            assert st == 0 and o == payload
    if name == "n129":
        # (the 17 literals with i % 5 == 0 and i % 3 != 0, the valid ones of
        # them aside)
        assert 0 < sum(status) <= 17
    if name == "all_empty":
        assert outs == [b""] * 64 and not any(status)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["far_apart", "big_output", "raw64k",
                                  "huff64k", "raw64k_mid", "huff64k_mid"])
def test_past_the_stage(codec, name):
    """past the input stage by gaps alone or by one long literal; past the
    output stage (staged input) by the decoded sizes"""
    s = SHAPES[name]()
    outs, status = check_both(codec, s)
    if name == "big_output":
        assert not any(status) and sum(len(o) for o in outs) + 64 > STAGE
    elif name == "far_apart":
        assert [len(o) for o, l in zip(outs, s.lits) if not l.huffman] \
            == [10] * 32
    else:
        i = 0 if len(s.lits) == 1 else 29
        assert status[i] == 0 and outs[i] == long_text()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["edge3072_fix66", "edge3072_var67"])
def test_stage_edge(codec, name):
    """a tile of exactly 3072 bytes of adjacent literals at residue 0, its
    Huffman literals at the 8/5 expansion (66 bytes: the fixed arena's
    limit; 67: the variable arena, full): every literal against the oracle"""
    s = SHAPES[name]()
    assert tile_staged(s.lits, 0) == [True] and tile_staged(s.lits, 1) == [False]
    outs, status = check_both(codec, s)
    assert not any(status)
    for l, o in zip(s.lits, outs):
        payload = s.buf[l.pos:l.pos + l.len]
        if l.huffman:
            assert (O.OK, o) == O.huff_decode(payload)
            assert len(o) == 8 * l.len // 5
        else:
            assert o == payload
    assert sum(len(o) for o in outs) + 64 > STAGE


@pytest.mark.gpu
@pytest.mark.parametrize("front", [None, 63, 62], ids=["plain", "across",
                                                        "within"])
def test_limit(codec, front):
    """test_gpu_decode_clamp's cases and statuses; then each case's NAME on a
    tile's lane 63 and its VALUE on the next tile's lane 0; then both in
    one tile"""
    s, status = clamp(front)
    outs, got = check_both(codec, s, qhuff.MAX_STRLEN)
    assert got == status
    for o, st in zip(outs, got):
        if st:
            assert o == b""
        else:
            assert o == b"nm" or o[:1] == b"v" or o == b"a" * len(o)
    assert not any(check_both(codec, s, None)[1])


@pytest.mark.gpu
def test_limit_raw_literal(codec):
    s = Shape(b"z" * 70000, [qhuff.Literal(0, 70000, 0, 7, 2, 0, 0)])
    assert check_both(codec, s, qhuff.MAX_STRLEN) == ([b""], [1])
    assert check_both(codec, s, None) == ([b"z" * 70000], [0])


def wire_specs(shape, k):
    n = len(shape.lits)
    return [("buf", len(shape.buf), (5 * k + 1) % 16),
            ("lits", 16 * n, 4 * (k % 4)),
            ("out", qhuff.literals_bound(shape.lits), (7 * k + 3) % 16),
            ("out_off", 4 * (n + 1), 4 * ((k + 1 + k // 4) % 4)),
            ("status", n, (2 * k + 1) % 16)]


@pytest.mark.gpu
@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_buffer_contract(codec, name, host):
    """every buffer at its contractual size in a dirty guarded arena, buf
    and out at odd residues, lits and out_off at every word residue: nothing
    but out[0 .. out_off[n]), out_off and status changes, and the result does
    not depend on the bytes around the wire data"""
    import torch
    s = SHAPES[name]()
    n = len(s.lits)
    assert qhuff.literals_check(s.lits)[0] == qhuff.OK
    if n:
        assert s.lits[0].pos == 0
    outs, status = s.want(codec)
    want_off = np.zeros(n + 1, dtype=np.uint32)
    np.cumsum([len(o) for o in outs], out=want_off[1:])
    total = int(want_off[-1])
    L = qhuff.lib()
    for k, fill in enumerate(FILLS):
        k += 3 * host
        ar = Arena(wire_specs(s, k), seed=7000 + k)
        ar.put("buf", np.frombuffer(s.buf, dtype=np.uint8))
        ar.put("lits", qhuff.literals_array(s.lits))
        ar.neighbours("buf", fill)
        ar.commit(not host)
        if host:
            rc = L.qhuff_decode_wire_host(
                codec._ctx, ar.addr("buf"), ar.addr("lits"), n, 0,
                ar.addr("out"), ar.addr("out_off"), ar.addr("status"))
            assert rc == qhuff.OK
        else:
            codec.decode_wire_into(ar.ptr("buf"), ar.ptr("lits"), n, None,
                                   ar.ptr("out"), ar.ptr("out_off"),
                                   ar.ptr("status"))
            torch.cuda.synchronize()
            assert codec.device_error() == 0
        img = ar.after()
        assert np.array_equal(ar.get(img, "out_off", np.uint32), want_off)
        assert ar.get(img, "out", count=total).tobytes() == b"".join(outs)
        assert list(ar.get(img, "status")) == status
        ar.check(img, {"out": total, "out_off": 4 * (n + 1), "status": n})


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["golden", "n129", "far_apart", "across"])
def test_high_offsets(codec, name):
    """every pos and instr with its top bit set: `buf` points 0xF0000000
    below a small allocation, which no 4 GB buffer backs"""
    import torch
    s = (golden() if name == "golden" else clamp(63)[0] if name == "across"
         else SHAPES[name]())
    max_len = None if name in ("n129", "far_apart") else qhuff.MAX_STRLEN
    want = s.want(codec, max_len)
    hi = rebased(s.lits, HIGH)
    assert qhuff.literals_check(hi)[0] == qhuff.OK
    assert all(l.pos >> 31 for l in hi)
    n = len(hi)
    buf = dev(np.frombuffer(s.buf, dtype=np.uint8))
    lits = dev(qhuff.literals_array(hi))
    out = torch.empty(qhuff.literals_bound(hi), dtype=torch.uint8, device="cuda")
    oo = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    st = torch.empty(n, dtype=torch.uint8, device="cuda")
    codec.decode_wire_into(Ptr(buf.data_ptr() - HIGH), lits, n, max_len, out,
                           oo, st)
    torch.cuda.synchronize()
    assert codec.device_error() == 0
    assert split(out, oo, st, n) == want
    # the host entry
    src = np.frombuffer(s.buf + b"\0" * 16, dtype=np.uint8)
    arr = qhuff.literals_array(hi)
    ho = np.zeros(qhuff.literals_bound(hi), dtype=np.uint8)
    hoo = np.zeros(n + 1, dtype=np.uint32)
    hst = np.zeros(n, dtype=np.uint8)
    rc = qhuff.lib().qhuff_decode_wire_host(
        codec._ctx, src.ctypes.data - HIGH, arr.ctypes.data, n, max_len or 0,
        ho.ctypes.data, hoo.ctypes.data, hst.ctypes.data)
    assert rc == qhuff.OK
    assert ([ho[hoo[i]:hoo[i + 1]].tobytes() for i in range(n)],
            [int(x) for x in hst]) == want


@pytest.mark.gpu
def test_host_entry_checks_the_order_rule(codec):
    s = counts(65)
    sw = list(s.lits)
    sw[3], sw[4] = sw[4], sw[3]
    assert qhuff.literals_check(sw)[0] == qhuff.EINVAL
    with pytest.raises(qhuff.QhuffError):
        codec.decode_wire_host(s.buf, sw)
    # and the context is as good as before
    check_both(codec, s)


@pytest.mark.gpu
def test_ordering_and_timing(codec):
    """two calls back to back on two streams of one context; one between two
    decode launches; the launch is timed as a decode"""
    import torch
    a, b = golden(), counts(129)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        ra = run_device(codec, a, qhuff.MAX_STRLEN, stream=s1)
    with torch.cuda.stream(s2):
        rb = run_device(codec, b, None, stream=s2)
    torch.cuda.synchronize()
    assert codec.device_error() == 0
    assert split(*ra) == a.want(codec, qhuff.MAX_STRLEN)
    assert split(*rb) == b.want(codec)

    data, off = qhuff.synth_batch(5000, seed=3)
    h, ho = O.encode_batch(data, off, 0)
    hd, hod = dev(h), dev(ho.view(np.int32))
    codec.timing(True)
    try:
        codec.timing_read()
        d1 = codec.decode(hd, hod)
        rw = run_device(codec, a, None, stream=torch.cuda.current_stream())
        d2 = codec.decode(hd, hod)
        torch.cuda.synchronize()
        assert codec.device_error() == 0
        t = codec.timing_read()
    finally:
        codec.timing(False)
    assert [k for k, _ in t] == [qhuff.KIND_DECODE] * 3
    assert all(us > 0 for _, us in t)
    assert split(*rw) == a.want(codec)
    for out, oo, st in (d1, d2):
        assert not st.cpu().numpy().any()
        assert np.array_equal(oo.cpu().numpy().view(np.uint32), off)
        assert np.array_equal(out.cpu().numpy()[:int(off[-1])], data)
