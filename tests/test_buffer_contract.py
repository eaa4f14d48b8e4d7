"""The batch calls' buffer contract (include/qhuff.h, "Buffer contract"): a
call writes exactly its outputs and nothing else, for any legal pointers.

Every other GPU test hands the library fresh, allocator-aligned outputs and
inputs followed by zero bytes.  Here each buffer of a call is carved out of a
larger arena: exactly its contractual size, at a chosen residue mod 16, with
at least 256 guard bytes either side, the whole arena (guards and the
buffer's own bytes) filled from a seeded RNG.  After the call

  (a) bytes, offsets, statuses and hashes equal the oracle's;
  (b) every guard byte is unchanged;
  (c) the inputs are unchanged;
  (d) the bytes of `out` past out_off[n], up to the bound, are unchanged,

with the bytes next to the input all 0x00, all 0xFF and random.  Device
arenas are torch tensors, host arenas numpy arrays; the comparison itself
(`violations`) is plain numpy and has CPU tests of its own.  Also: the
device multi-context rebase at every alignment of out_off, input offsets
with bit 31 set, and a multi-context host call whose `out` is registered
for direct DMA over the first shard's share only."""
import ctypes as C
import functools
import os
import random

import numpy as np
import pytest

import _paths  # noqa: F401
import limits
import oracle_lib as O
import qhuff
import qpack_frames as Q
from qhuff import workload
from test_gpu_parity import ALPHAS, pack, rand_strings

HERE = os.path.dirname(os.path.abspath(__file__))
GUARD = 256
NEIGH = 64                  # bytes set either side of `in` by neighbours()
FILLS = ("zero", "ff", "random")
BIG_SLOT = 12 * 1024        # qhuff_pipeline.h kBigSlotBytes


# ---- the harness: arenas, carved buffers, the comparison ---------------------

class Ptr:
    """an address with the data_ptr() of a tensor (Codec.*_into take those)"""

    def __init__(self, addr):
        self.addr = addr

    def data_ptr(self):
        return self.addr


def carve(specs, guard=GUARD):
    """specs: (name, bytes, residue mod 16) in order -> ({name: (start,
    bytes)}, arena size); `guard` bytes before and after every buffer (the
    arena's base is 16-byte aligned)"""
    reg, pos = {}, 0
    for name, nbytes, res in specs:
        pos += guard
        pos += (res - pos) % 16
        reg[name] = (pos, int(nbytes))
        pos += int(nbytes) + guard
    return reg, pos + 16


def violations(before, after, reg, written, guard=GUARD):
    """Every byte that differs between the arena images outside the bytes
    the call may write -- written[name] leading bytes of buffer `name`
    (absent: none) -- as (name, "before" | "after" | "inside" | "far",
    distance): in the guard before / after a buffer, inside it past its
    written bytes (distance from its start), or elsewhere in the arena."""
    may = np.zeros(len(before), dtype=bool)
    for name, w in written.items():
        s, nb = reg[name]
        assert 0 <= w <= nb, (name, w, nb)
        may[s:s + w] = True
    out = []
    for i in np.flatnonzero((before != after) & ~may):
        i = int(i)
        hit = (None, "far", i)
        for name, (s, nb) in reg.items():
            if s <= i < s + nb:
                hit = (name, "inside", i - s)
                break
            if s - guard <= i < s:
                hit = (name, "before", s - i)
            elif s + nb <= i < s + nb + guard and hit[1] == "far":
                hit = (name, "after", i - (s + nb) + 1)
        out.append(hit)
    return out


class Arena:
    """One call's buffers in one dirty arena.  put() the inputs, commit() to
    the device (torch) or the host (numpy), call with ptr()s, then check()
    the image read back by after()."""

    def __init__(self, specs, seed, guard=GUARD):
        self.guard = guard
        self.reg, self.size = carve(specs, guard)
        self.before = np.random.default_rng(seed).integers(
            0, 256, self.size, dtype=np.uint8)
        self.dev = self.host = None

    def put(self, name, a):
        s, nb = self.reg[name]
        b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        assert len(b) == nb, (name, len(b), nb)
        self.before[s:s + nb] = b

    def neighbours(self, name, fill):
        """the bytes just before and just after buffer `name`"""
        s, nb = self.reg[name]
        assert NEIGH <= self.guard
        if fill != "random":
            v = 0 if fill == "zero" else 0xFF
            self.before[s - NEIGH:s] = v
            self.before[s + nb:s + nb + NEIGH] = v

    def commit(self, device):
        if device:
            import torch
            self.dev = torch.from_numpy(self.before).cuda()
            self.base = self.dev.data_ptr()
        else:
            mem = np.empty(self.size + 16, dtype=np.uint8)
            sh = (-mem.ctypes.data) % 16
            self.host = mem[sh:sh + self.size]
            self.host[:] = self.before
            self.base = self.host.ctypes.data
        assert self.base % 16 == 0
        return self

    def addr(self, name, back=0):
        return self.base + self.reg[name][0] - back

    def ptr(self, name, back=0):
        return Ptr(self.addr(name, back))

    def view(self, name):
        """(host arenas) the live buffer"""
        s, nb = self.reg[name]
        return self.host[s:s + nb]

    def after(self):
        if self.dev is not None:
            return self.dev.cpu().numpy()
        return self.host.copy()

    def get(self, img, name, dtype=np.uint8, count=None):
        s, nb = self.reg[name]
        a = img[s:s + nb].view(dtype)
        return a if count is None else a[:count]

    def check(self, img, written):
        bad = violations(self.before, img, self.reg, written, self.guard)
        assert not bad, "stray writes (buffer, where, distance): %r" % bad[:8]


# ---- CPU: the harness reports what it must -----------------------------------

def _fake_call(where):
    """a numpy 'encode' of 40 bytes into a 100-byte `out`, with one stray
    byte (or none)"""
    ar = Arena([("in", 33, 5), ("out", 100, 13), ("out_off", 4 * 4, 4),
                ("status", 3, 1)], seed=1).commit(False)
    ar.view("out")[:40] ^= 0x5A
    ar.view("out_off")[:] ^= 0xA5
    ar.view("status")[:] ^= 0xFF
    s, nb = ar.reg["out"]
    if where == "before":
        ar.host[s - 1] ^= 0xFF
    elif where == "after":
        ar.host[s + nb] ^= 0xFF
    elif where == "past_total":
        ar.host[s + 40] ^= 0xFF
    elif where == "input":
        ar.view("in")[32] ^= 1
    elif where == "status_guard":
        ar.host[ar.reg["status"][0] + 3] ^= 1
    return violations(ar.before, ar.after(), ar.reg,
                      {"out": 40, "out_off": 16, "status": 3})


def test_harness_exact_write_is_clean():
    assert _fake_call(None) == []


@pytest.mark.parametrize("where,want", [
    ("before", ("out", "before", 1)),
    ("after", ("out", "after", 1)),
    ("past_total", ("out", "inside", 40)),
    ("input", ("in", "inside", 32)),
    ("status_guard", ("status", "after", 1)),
])
def test_harness_reports_stray_byte(where, want):
    assert _fake_call(where) == [want]


def test_harness_layout():
    """sizes exact, residues as asked, >= GUARD bytes around every buffer,
    the fill not a repeating pattern"""
    specs = [("a", 0, 1), ("b", 77, 8), ("c", 4 * 9, 12), ("d", 5, 15)]
    ar = Arena(specs, seed=2)
    prev_end = 0
    for name, nb, res in specs:
        s, got = ar.reg[name]
        assert got == nb and s % 16 == res and s - prev_end >= GUARD
        prev_end = s + nb
    assert ar.size - prev_end >= GUARD
    f = ar.before
    assert len(np.unique(f)) > 200 and not np.array_equal(f[:64], f[64:128])
    assert np.array_equal(f, Arena(specs, seed=2).before)
    ar.neighbours("b", "ff")
    s, nb = ar.reg["b"]
    assert (ar.before[s - NEIGH:s] == 0xFF).all()
    assert (ar.before[s + nb:s + nb + NEIGH] == 0xFF).all()


# ---- batches, each asserted to reach the path it is for ----------------------

def tile_stats(off):
    """per 64-string tile: its 16-byte aligned span at residue 0, its
    longest string, its bytes"""
    off = np.asarray(off).astype(np.int64)
    n = len(off) - 1
    t0 = np.arange(0, n, workload.TILE, dtype=np.int64)
    t1 = np.minimum(t0 + workload.TILE, n)
    span = ((off[t1] + 15) & ~15) - (off[t0] & ~15)
    mx = np.maximum.reduceat(np.diff(off), t0) if n else np.zeros(0, np.int64)
    return span, mx, off[t1] - off[t0]


class Batch:
    """raw: strings to encode (data, off); huff: strings to decode"""

    def __init__(self, raw=None, huff=None):
        self.raw, self.huff = raw, huff
        self._want = {}

    def ops(self):
        return ([0, 3, 5, 7] if self.raw is not None else []) \
            + (["dec"] if self.huff is not None else [])

    def inputs(self, op):
        return self.huff if op == "dec" else self.raw

    def want(self, op):
        """the oracle's (out, out_off, status or None), computed once"""
        if op not in self._want:
            d, o = self.inputs(op)
            if op == "dec":
                self._want[op] = O.decode_batch(d, o)
            else:
                self._want[op] = O.encode_batch(d, o, op) + (None,)
        return self._want[op]


def _valid(raw):
    b = Batch(raw=raw)
    b.huff = b.want(0)[:2]
    return b


def _token(n, seed):
    b = _valid(qhuff.synth_batch(n, seed=seed))
    d, o = b.raw
    sh = workload.tile_shares(d, o, b.huff[1])
    assert len(o) - 1 == n and sh["tiles"] == -(-n // 64)
    assert sh["decode_slow_tile_share"] == 0 == sh["encode_slow_tile_share"]
    assert np.diff(o).min() >= 8 and np.diff(o).max() <= 64
    return b


def _big():
    """test_big_tile_slots' three tile kinds, two tiles each, ordinary tiles
    between: tiles 0, 2, .. 10 are the big ones"""
    rng = random.Random(77)
    strs = []
    for t in range(6):
        k = t % 3
        if k == 0:
            tile = (rand_strings(rng, 63, ALPHAS["token"], 0, 20)
                    + rand_strings(rng, 1, ALPHAS["token"], 3200, 5000))
        elif k == 1:
            tile = rand_strings(rng, 8, ALPHAS["all"], 600, 1100) \
                + rand_strings(rng, 56, ALPHAS["token"], 0, 30)
        else:
            tile = rand_strings(rng, 64, ALPHAS["token"], 40, 70)
        rng.shuffle(tile)
        strs += tile + rand_strings(rng, 64, ALPHAS["token"], 8, 40)
    b = _valid(pack(strs))
    big = np.arange(0, 12, 2)
    espan, emax, _ = tile_stats(b.raw[1])
    dspan, dmax, etot = tile_stats(b.huff[1])
    S = workload.STAGE
    assert (espan[big] > S).all() and (espan[big + 1] <= S).all()
    assert (emax[[0, 6]] > S).all()                  # a string past the stage
    assert (emax[[2, 4, 8, 10]] <= S).all()          # several staged units
    assert (espan[[4, 10]] < S + 1024).all()         # just over the stage
    assert ((etot[big] > S) & (etot[big] <= BIG_SLOT)).any()    # a slot
    # decode: input past the stage (kinds 0, 1) or output past it (kind 2)
    _, _, rtot = tile_stats(b.raw[1])
    assert (dspan[[0, 2, 6, 8]] > S).all() and (dmax[[0, 6]] > S).all()
    assert (dspan[[4, 10]] <= S).all() and (rtot[[4, 10]] + 64 > S).all()
    assert (rtot[big] <= BIG_SLOT).any()
    return b


def _slow():
    rng = random.Random(5)
    huge = bytes(rng.choice(ALPHAS["all"]) for _ in range(70000))
    b = _valid(pack(rand_strings(rng, 300, ALPHAS["token"], 0, 40) + [huge]
                    + rand_strings(rng, 300, ALPHAS["token"], 0, 40)))
    for off in (b.raw[1], b.huff[1]):                # no slot holds it
        assert tile_stats(off)[1].max() > BIG_SLOT
    return b


def _corrupt(rng, i, h):
    """test_decode_cooperative_invalid's corruptions"""
    k = i % 5
    if k == 0:                                       # EOS at a byte boundary
        at = rng.randrange(len(h) // 4, len(h) // 2)
        h[at:at] = b"\xff\xff\xff\xfc"
    elif k == 1:
        h[rng.randrange(len(h))] ^= 1 << rng.randrange(8)
    elif k == 2:
        h[-1] &= 0xfe                                # non-ones padding
    elif k == 3:
        h += b"\xff"                                 # padding of >= 8 bits
    else:
        h = h[:-3]                                   # cut
    return h


def _coop():
    """one string of 150..2400 raw bytes among 63 short ones per tile; the
    decode input has every third long string corrupted"""
    rng = random.Random(4242)
    lens = [150, 161, 200, 256, 300, 480, 700, 1000, 1461, 1900, 2400,
            170, 1200, 2000, 640]
    raw, huff, longs = [], [], []
    for t, ln in enumerate(lens):
        short = rand_strings(rng, 63, ALPHAS["token"], 0, 24)
        s = bytes(rng.choice(ALPHAS["token"]) for _ in range(ln))
        pos = rng.randrange(64)
        tile = short[:pos] + [s] + short[pos:]
        raw += tile
        hs = [O.huffman_enc(x) for x in tile]
        if t % 3 == 0:
            hs[pos] = bytes(_corrupt(rng, t // 3, bytearray(hs[pos])))
        huff += hs
        longs.append(64 * t + pos)
    b = Batch(raw=pack(raw), huff=pack(huff))
    dspan, dmax, _ = tile_stats(b.huff[1])
    coop = (dspan <= workload.STAGE) & (dmax > workload.COOP_MIN)
    assert coop.sum() >= 12, (dspan, dmax)
    st = b.want("dec")[2][longs]
    assert st.sum() >= 3 and (st == 0).sum() >= 9     # ERROR and OK long ones
    oo = b.want("dec")[1]
    assert all(oo[i + 1] == oo[i] for i in np.array(longs)[st == 1])
    sh = workload.tile_shares(b.raw[0], b.raw[1], b.want(0)[1])
    assert sh["encode_coop_tile_share"] > 0
    return b


def _garbage():
    rng = random.Random(11)
    b = Batch(huff=pack([bytes(rng.randrange(256)
                               for _ in range(rng.randint(0, 40)))
                         for _ in range(2000)]))
    st = b.want("dec")[2]
    assert st.sum() > 100 and (st == 0).sum() > 100
    return b


def _alpha(name):
    rng = random.Random(len(name))
    b = _valid(pack(rand_strings(rng, 1000, ALPHAS[name], 0, 80)))
    # the raw-copy literal path: H = 0 literals in every framed mode
    for mode in (3, 5, 7):
        out, oo, _ = b.want(mode)
        first = out[oo[:-1][np.diff(oo) > 1]]
        assert ((first >> mode) & 1 == 0).sum() > 100
    return b


def _none():
    b = Batch(raw=(np.zeros(0, np.uint8), np.zeros(1, np.uint32)),
              huff=(np.zeros(0, np.uint8), np.zeros(1, np.uint32)))
    return b


def _empties():
    b = _valid(pack([b""] * 130))
    assert b.raw[1][-1] == 0 and all(b.want(op)[1][-1] == 0 for op in (0, "dec"))
    assert b.want(7)[1][-1] == 130                   # one framing byte each
    return b


BUILDERS = {
    "token357": lambda: _token(64 * 5 + 37, 7),
    "token1": lambda: _token(1, 1),
    "token2": lambda: _token(2, 2),
    "token63": lambda: _token(63, 63),
    "token64": lambda: _token(64, 64),
    "token65": lambda: _token(65, 65),
    "none": _none,
    "empties": _empties,
    "big": _big,
    "slow": _slow,
    "coop": _coop,
    "garbage": _garbage,
    "long": lambda: _alpha("long"),
    "high": lambda: _alpha("high"),
}


@functools.lru_cache(maxsize=None)
def batch(name):
    return BUILDERS[name]()


@pytest.mark.parametrize("name", sorted(BUILDERS))
def test_batches_reach_their_paths(name):
    """(CPU) the builders' own assertions: each batch holds the tiles it is
    meant to reach, for the committed seeds"""
    b = batch(name)
    assert b.ops()


CODEC_CASES = [(name, op) for name in BUILDERS
               for op in ([0, 3, 5, 7, "dec"] if name != "garbage" else ["dec"])]


def bound_of(op, in_bytes, n):
    return (qhuff.decode_bound(in_bytes, n) if op == "dec"
            else qhuff.encode_bound(in_bytes, n, op))


def codec_specs(op, in_bytes, n, r_in, r_out, k):
    """the buffers of one codec call at their contractual sizes; the word
    arrays at residues 0/4/8/12, the statuses at an odd address"""
    specs = [("in", in_bytes, r_in), ("in_off", 4 * (n + 1), 4 * (k % 4)),
             ("out", bound_of(op, in_bytes, n), r_out),
             ("out_off", 4 * (n + 1), 4 * ((k + 1 + k // 4) % 4))]
    if op == "dec":
        specs.append(("status", n, (2 * k + 1) % 16))
    return specs


def load_codec(ar, data, off, back):
    """put the batch's bytes and offsets; the call's `in` is the buffer's
    address - back and its offsets start at `back` (in_off[0] != 0)"""
    a0 = int(off[0])
    ar.put("in", data[a0:int(off[-1])])
    ar.put("in_off", (off.astype(np.int64) - a0 + back).astype(np.uint32))


def check_codec(ar, img, op, want, n, slack=0):
    out, oo, st = want
    total = int(oo[-1])
    assert np.array_equal(ar.get(img, "out_off", np.uint32), oo)
    assert np.array_equal(ar.get(img, "out", count=total), out)
    written = {"out": total + slack, "out_off": 4 * (n + 1)}
    if op == "dec":
        assert np.array_equal(ar.get(img, "status"), st)
        written["status"] = n
    ar.check(img, written)          # guards, inputs, out past its total


# ---- GPU: device-pointer codec calls ------------------------------------------

@pytest.fixture(scope="module")
def codecs():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("gpu test without a GPU")
    cs = [qhuff.Codec(0) for _ in range(3)]
    yield cs
    for c in cs:
        c.close()


@pytest.fixture(scope="module")
def codec(codecs):
    return codecs[0]


def device_codec_call(codec, op, variant, ar, n, back):
    import torch
    kind = qhuff.KIND_DECODE if op == "dec" else qhuff.KIND_ENCODE
    codec.batch_hint(kind, variant)
    if op == "dec":
        codec.decode_into(ar.ptr("in", back), ar.ptr("in_off"), n,
                          ar.ptr("out"), ar.ptr("out_off"), ar.ptr("status"))
    else:
        codec.encode_into(ar.ptr("in", back), ar.ptr("in_off"), n, op,
                          ar.ptr("out"), ar.ptr("out_off"))
    torch.cuda.synchronize()
    assert codec.device_error() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name,op", CODEC_CASES,
                         ids=["%s-%s" % c for c in CODEC_CASES])
def test_device_codec_contract(codec, name, op):
    """qhuff_encode_batch / qhuff_decode_batch, lean and full kernels: all
    16 residues of `in` and `out` on the token batch, three mixed ones on
    the others, each with the input's neighbours 0x00, 0xFF and random"""
    b = batch(name)
    data, off = b.inputs(op)
    n = len(off) - 1
    in_bytes = int(off[-1] - off[0])
    if name == "token357":
        residues = [(r, (7 * r + 3) % 16) for r in range(16)]
    else:
        residues = [(1, 8), (8, 13), (13, 1)]
    k = 0
    for variant in (0, 1):
        for r_in, r_out in residues:
            for fill in FILLS:
                back = (0, 3, 200)[k % 3]
                ar = Arena(codec_specs(op, in_bytes, n, r_in, r_out, k),
                           seed=1000 + k)
                load_codec(ar, data, off, back)
                ar.neighbours("in", fill)
                ar.commit(True)
                device_codec_call(codec, op, variant, ar, n, back)
                check_codec(ar, ar.after(), op, b.want(op), n)
                k += 1


# ---- GPU: hashing ----------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def hash_shape(kind):
    """test_xxh32.py's shapes, at most 2,000 headers: (data, off[2n + 1])"""
    rng = random.Random(len(kind) * 131)
    if kind == "ragged":
        lens = [rng.choice([0, 1, 3, 4, 15, 16, 17, 31, 32, 33, 200])
                for _ in range(2 * 1000)]
    elif kind == "long":                        # tiles larger than the stage
        # (64 strings of 0..699 bytes never fit the hash kernel's 6144-byte
        # stage: 128 headers of short ones follow, so that tiles on either
        # side of it, and one that holds both kinds, are in the batch)
        lens = [rng.randrange(0, 700) for _ in range(2 * 700)] \
            + [rng.randrange(0, 40) for _ in range(2 * 128)]
    else:
        lens = [0] * (2 * 130)
    blob = bytes(rng.randrange(256) for _ in range(sum(lens)))
    off = np.zeros(len(lens) + 1, dtype=np.uint32)
    np.cumsum(lens, out=off[1:])
    data = np.frombuffer(blob, dtype=np.uint8).copy()
    if kind == "long":
        assert (tile_stats(off[::2])[0] > workload.STAGE).any()
        # the hash kernel's own stage, in both calls' layouts and at the
        # residues test_device_hash_contract puts the batch on
        for pairs in (True, False):
            for res in (0, 1, 8, 13):
                span = np.array([t["span"] for t in
                                 limits.classify_hash(off, res, pairs)])
                assert (span > limits.HASH_STAGE).any()
                assert (span <= limits.HASH_STAGE).any()
    return data, off


def test_hash_long_shape_reaches_both_sides():
    """(CPU) hash_shape's own assertions"""
    data, off = hash_shape("long")
    assert len(off) % 2 == 1 and off[-1] == len(data)


def hash_want(data, off, pairs):
    if pairs:
        return O.xxh32_headers(data, off)
    return (np.array([O.xxh32(data[off[i]:off[i + 1]].tobytes())
                      for i in range(len(off) - 1)], dtype=np.uint32),)


def device_hash_call(codec, pairs, n, in_ptr, off_ptr, h1, h2):
    import torch
    L = qhuff.lib()
    st = codec._stream(None)
    if pairs:
        rc = L.qhuff_xxh32_headers(codec._ctx, in_ptr, off_ptr, n,
                                   qhuff.XXH_SEED, h1, h2, st)
    else:
        rc = L.qhuff_xxh32_batch(codec._ctx, in_ptr, off_ptr, n,
                                 qhuff.XXH_SEED, h1, st)
    assert rc == qhuff.OK
    torch.cuda.synchronize()
    assert codec.device_error() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("pairs", [True, False], ids=["headers", "batch"])
@pytest.mark.parametrize("kind", ["ragged", "long", "empty"])
def test_device_hash_contract(codec, kind, pairs):
    """qhuff_xxh32_headers / qhuff_xxh32_batch: n words per hash output at
    residues 0/4/8/12, guards, inputs and neighbours as for the codec"""
    data, off = hash_shape(kind)
    n = (len(off) - 1) // 2 if pairs else len(off) - 1
    want = hash_want(data, off, pairs)
    k = 0
    for r_in in (1, 8, 13, 0):
        for fill in FILLS:
            back = (0, 3, 200)[k % 3]
            specs = [("in", len(data), r_in), ("in_off", 4 * len(off), 4 * (k % 4)),
                     ("h1", 4 * n, 4 * ((k + 1) % 4)),
                     ("h2", 4 * n if pairs else 0, 4 * ((k + 2 + k // 4) % 4))]
            ar = Arena(specs, seed=2000 + k)
            load_codec(ar, data, off, back)
            ar.neighbours("in", fill)
            ar.commit(True)
            device_hash_call(codec, pairs, n, ar.addr("in", back),
                             ar.addr("in_off"), ar.addr("h1"), ar.addr("h2"))
            img = ar.after()
            assert np.array_equal(ar.get(img, "h1", np.uint32), want[0])
            if pairs:
                assert np.array_equal(ar.get(img, "h2", np.uint32), want[1])
            ar.check(img, {"h1": 4 * n, "h2": 4 * n if pairs else 0})
            k += 1


# ---- GPU: device multi-context rebase at every alignment ------------------------

REBASE_SIZES = [0, 1, 2, 3, 4, 6, 7, 8]          # n_k + 1 in {1..5, 7, 8, 9}


@functools.lru_cache(maxsize=None)
def _multi_source():
    return _token(2100, 31)


@pytest.mark.gpu
@pytest.mark.parametrize("encode", [True, False], ids=["encode", "decode"])
@pytest.mark.parametrize("g", [2, 3])
def test_device_multi_rebase_every_alignment(codecs, g, encode):
    """qhuff_*_batch_multi with rebase: every shard's out_off (n_k + 1
    entries, at residues 0/4/8/12, guarded) holds the stitched offsets in
    ALL its entries -- shard k's last one is base[k + 1] -- for shard sizes
    that leave qhuff_rebase_kernel only a head, a head and a tail, or head,
    vector body and tail"""
    import torch
    b = _multi_source()
    op = 0 if encode else "dec"
    data, off = b.inputs(op)
    out, oo, st = b.want(op)
    runs = 0
    for res in (0, 4, 8, 12):
        sizes = REBASE_SIZES + [1000 + res // 4]
        for j, m in enumerate(sizes):
            # shard 0 gives the later ones a base; the last shard (g = 3)
            # takes another size of the list
            ns = [5, m] if g == 2 else [5, m, sizes[(j + 3) % len(sizes)]]
            cuts = np.concatenate([[0], np.cumsum(ns)])
            assert cuts[-1] <= len(off) - 1
            arenas, shards = [], []
            for k in range(g):
                a, e = int(cuts[k]), int(cuts[k + 1])
                so = off[a:e + 1]
                nb = int(so[-1] - so[0])
                specs = codec_specs(op, nb, e - a, (3 * k + 1) % 16,
                                    (5 * k + 2) % 16, 0)
                specs[3] = ("out_off", 4 * (e - a + 1), (res + 4 * k) % 16)
                ar = Arena(specs, seed=3000 + runs * 4 + k)
                load_codec(ar, data, so, 0)
                ar.commit(True)
                arenas.append(ar)
                shards.append(dict(
                    in_=ar.ptr("in"), in_off=ar.ptr("in_off"), n=e - a,
                    out=ar.ptr("out"), out_off=ar.ptr("out_off"),
                    status=None if encode else ar.ptr("status")))
            base = qhuff.batch_multi(codecs[:g], shards, encode, 0, rebase=True)
            torch.cuda.synchronize()
            assert base == [int(oo[c]) for c in cuts]
            for k, ar in enumerate(arenas):
                a, e = int(cuts[k]), int(cuts[k + 1])
                img = ar.after()
                got = ar.get(img, "out_off", np.uint32)
                assert np.array_equal(got, oo[a:e + 1]), (res, ns, k)
                assert got[-1] == base[k + 1]
                tot = base[k + 1] - base[k]
                assert np.array_equal(ar.get(img, "out", count=tot),
                                      out[base[k]:base[k + 1]])
                written = {"out": tot, "out_off": 4 * (e - a + 1)}
                if not encode:
                    assert np.array_equal(ar.get(img, "status"), st[a:e])
                    written["status"] = e - a
                ar.check(img, written)
            runs += 1
    for c in codecs[:g]:
        assert c.device_error() == 0


# ---- GPU: input offsets with the top bit set ---------------------------------------

@functools.lru_cache(maxsize=None)
def _top_bit_batch():
    """~60 KB: token tiles, a tile with one cooperative string, a tile just
    over the stage (last, so the batch ends in the global-memory walks)"""
    rng = random.Random(2 ** 31)
    strs = rand_strings(rng, 64 * 20, ALPHAS["token"], 8, 64)
    tile = rand_strings(rng, 63, ALPHAS["token"], 0, 24)
    tile.insert(17, bytes(rng.choice(ALPHAS["token"]) for _ in range(1500)))
    strs += tile
    strs += rand_strings(rng, 64, ALPHAS["token"], 80, 110)
    b = _valid(pack(strs))
    for o in (b.raw[1], b.huff[1]):
        span, mx, _ = tile_stats(o)
        assert span[-1] > workload.STAGE and (span[:-1] <= workload.STAGE).all()
        assert mx[-2] > workload.COOP_MIN
    assert 45_000 < b.raw[1][-1] < 70_000
    return b


TOP_R = (0, 1, 5, 12)       # the last string ends at 2^32 - 1 - r


@functools.lru_cache(maxsize=None)
def _top_bit_hash_batch(tail):
    """~20 KB for the hash calls alone: token tiles, then 128 strings of
    100 bytes or more, so that the last tile passes the hash kernel's stage
    as 64 strings and as 64 headers and the batch ends in the reader of
    global memory; the last string of 20 + tail bytes (tail 1..3: a stripe,
    a word, then tail bytes whose p + 4 wraps where the string ends within
    4 bytes of 2^32) -> (data, off, {pairs: hashes})"""
    rng = random.Random(2 ** 32 + tail)
    strs = rand_strings(rng, 128 * 2, ALPHAS["token"], 8, 40) \
        + rand_strings(rng, 127, ALPHAS["all"], 100, 120) \
        + rand_strings(rng, 1, ALPHAS["all"], 20 + tail, 20 + tail)
    data, off = pack(strs)
    assert len(off) - 1 == 3 * 128 and 1 <= tail <= 3
    assert int(off[-1] - off[-2]) % 4 == tail and off[-1] - off[-2] >= 20
    return data, off, {p: hash_want(data, off, p) for p in (True, False)}


def test_top_bit_hash_batch_ends_unstaged():
    """(CPU) at every place test_input_offsets_with_top_bit_set puts it,
    the hash-only batch's last tile is past the hash kernel's stage in both
    layouts (limits.classify_hash on the offsets the kernel gets: the
    buffer is 16-byte aligned) and the tiles before it are staged"""
    for tail in (1, 2, 3):
        data, off, _ = _top_bit_hash_batch(tail)
        for at in [(1 << 32) - 1 - r - len(data) for r in TOP_R] \
                + [(1 << 31) - 5000]:
            goff = off.astype(np.int64) + at
            assert goff[-1] <= (1 << 32) - 1
            for pairs in (True, False):
                info = limits.classify_hash(goff, 0, pairs)
                assert not info[-1]["staged"] and info[-1]["cnt"] == 64
                assert info[0]["staged"] and info[1]["staged"]


@pytest.mark.gpu
def test_input_offsets_with_top_bit_set(codec):
    """in_off up to 2^32 - 1 and straddling 2^31 (uint32 offsets carried in
    int32 tensors): encode (modes 0, 7), decode and both hash calls,
    bit-exact with the oracle run on the same strings at offset 0.  The
    buffer is 2^32 bytes plus one page that no offset reaches, so the whole
    16-byte block around the last string lies inside the allocation.  The
    hash calls also run a batch of their own (_top_bit_hash_batch) whose
    last tile is read from global memory and whose last string leaves 1, 2
    and 3 tail bytes at 2^32 - 1 - r."""
    import torch
    b = _top_bit_batch()
    size = 1 << 32
    buf = torch.empty(size + 4096, dtype=torch.uint8, device="cuda")
    try:
        assert buf.data_ptr() % 16 == 0
        starts = {op: [size - 1 - r - int(b.inputs(op)[1][-1])
                       for r in TOP_R] + [(1 << 31) - 5000]
                  for op in (0, "dec")}
        k = 0
        for i in range(5):
            for op in (0, 7, "dec", "hash", "headers"):
                src = "dec" if op == "dec" else 0
                data, off = b.inputs(src)
                n = len(off) - 1
                at = starts[src][i]
                end = at + len(data)
                assert end <= size - 1 and end > 1 << 31
                assert (i < 4) == (at > 1 << 31)
                dd = torch.from_numpy(data).cuda()
                buf[at:end] = dd
                goff = (off.astype(np.uint64) + np.uint64(at)).astype(np.uint32)
                assert goff[-1] >> 31 == 1
                off_t = torch.from_numpy(goff.view(np.int32)).cuda()
                if op in ("hash", "headers"):
                    pairs = op == "headers"
                    m = n // 2 if pairs else n
                    ar = Arena([("h1", 4 * m, 4), ("h2", 4 * m if pairs else 0,
                                                   12)], seed=4000 + k)
                    ar.commit(True)
                    device_hash_call(codec, pairs, m, buf.data_ptr(),
                                     off_t.data_ptr(), ar.addr("h1"),
                                     ar.addr("h2"))
                    img = ar.after()
                    want = hash_want(data, off[:2 * m + 1] if pairs else off,
                                     pairs)
                    assert np.array_equal(ar.get(img, "h1", np.uint32), want[0])
                    if pairs:
                        assert np.array_equal(ar.get(img, "h2", np.uint32),
                                              want[1])
                    ar.check(img, {"h1": 4 * m, "h2": 4 * m if pairs else 0})
                else:
                    for variant in (0, 1):
                        specs = codec_specs(op, len(data), n, 0, (5 + k) % 16,
                                            k)[2:]
                        ar = Arena(specs, seed=4000 + k).commit(True)
                        kind = (qhuff.KIND_DECODE if op == "dec"
                                else qhuff.KIND_ENCODE)
                        codec.batch_hint(kind, variant)
                        if op == "dec":
                            codec.decode_into(buf, off_t, n, ar.ptr("out"),
                                              ar.ptr("out_off"),
                                              ar.ptr("status"))
                        else:
                            codec.encode_into(buf, off_t, n, op, ar.ptr("out"),
                                              ar.ptr("out_off"))
                        torch.cuda.synchronize()
                        assert codec.device_error() == 0
                        check_codec(ar, ar.after(), op, b.want(op), n)
                        k += 1
                # the inputs are as they were
                assert torch.equal(buf[at:end], dd)
                assert np.array_equal(off_t.cpu().numpy().view(np.uint32), goff)
                k += 1
                if op not in ("hash", "headers"):
                    continue
                # the hash-only batch in the same buffer
                for tail in (1, 2, 3):
                    hd, hoff, hwant = _top_bit_hash_batch(tail)
                    at = (size - 1 - TOP_R[i] - len(hd) if i < 4
                          else (1 << 31) - 5000)
                    end = at + len(hd)
                    assert end <= size - 1 and end > 1 << 31
                    if i < 4:
                        assert end == size - 1 - TOP_R[i]
                    dd = torch.from_numpy(hd).cuda()
                    buf[at:end] = dd
                    goff = (hoff.astype(np.uint64)
                            + np.uint64(at)).astype(np.uint32)
                    info = limits.classify_hash(goff, 0, pairs)
                    assert not info[-1]["staged"]
                    off_t = torch.from_numpy(goff.view(np.int32)).cuda()
                    m = (len(hoff) - 1) // (2 if pairs else 1)
                    ar = Arena([("h1", 4 * m, 4), ("h2", 4 * m if pairs else 0,
                                                   12)], seed=4500 + k)
                    ar.commit(True)
                    device_hash_call(codec, pairs, m, buf.data_ptr(),
                                     off_t.data_ptr(), ar.addr("h1"),
                                     ar.addr("h2"))
                    img = ar.after()
                    want = hwant[pairs]
                    assert np.array_equal(ar.get(img, "h1", np.uint32), want[0])
                    if pairs:
                        assert np.array_equal(ar.get(img, "h2", np.uint32),
                                              want[1])
                    ar.check(img, {"h1": 4 * m, "h2": 4 * m if pairs else 0})
                    assert torch.equal(buf[at:end], dd)
                    k += 1
    finally:
        del buf
        torch.cuda.empty_cache()


# ---- GPU: host-memory entry points ----------------------------------------------------

def host_codec_call(L, fn_ctx, op, ar, n, back, multi=None, svc=False):
    """the host-memory codec call over the arena's buffers -> rc"""
    a = ar.addr
    if multi is not None:
        ctxs = (C.c_void_p * len(multi))(*[c._ctx.value for c in multi])
        if op == "dec":
            return L.qhuff_decode_batch_host_multi(
                ctxs, len(multi), a("in", back), a("in_off"), n, a("out"),
                a("out_off"), a("status"))
        return L.qhuff_encode_batch_host_multi(
            ctxs, len(multi), a("in", back), a("in_off"), n, op, a("out"),
            a("out_off"))
    if op == "dec":
        fn = L.qhuff_svc_decode if svc else L.qhuff_decode_batch_host
        return fn(fn_ctx, a("in", back), a("in_off"), n, a("out"),
                  a("out_off"), a("status"))
    fn = L.qhuff_svc_encode if svc else L.qhuff_encode_batch_host
    return fn(fn_ctx, a("in", back), a("in_off"), n, op, a("out"),
              a("out_off"))


def register_all(ar, names):
    """qhuff_host_register over exactly the named buffers (the arena's
    guard keeps two buffers off one page)"""
    assert ar.guard >= 8192
    done = []
    for nm in names:
        nb = ar.reg[nm][1]
        if nb:
            rc = qhuff.lib().qhuff_host_register(ar.addr(nm), nb)
            assert rc == qhuff.OK, (nm, rc)
            done.append(nm)
    return done


def unregister_all(ar, names):
    for nm in names:
        assert qhuff.lib().qhuff_host_unregister(ar.addr(nm)) == qhuff.OK


@functools.lru_cache(maxsize=None)
def _past_small():
    """a batch whose bounds pass the host path's 4 MB 'small' threshold in
    both directions (and, halved, in each of two shards)"""
    b = _token(250_000, 41)
    assert qhuff.decode_bound(int(b.huff[1][-1]) // 2 - 64, 1) > 4 << 20
    return b


HOST_CASES = ["small", "coop", "past_small", "registered", "registered_small",
              "multi2", "multi3", "svc"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", HOST_CASES)
def test_host_codec_contract(codecs, case):
    """qhuff_*_batch_host (small and past the 4 MB threshold, staged and
    with exactly the buffers registered), qhuff_*_batch_host_multi and
    qhuff_svc_*: numpy arenas, the same guards and exact sizes"""
    L = qhuff.lib()
    name = {"coop": "coop", "past_small": None, "registered": None}.get(
        case, "token357")
    b = batch(name) if name else _past_small()
    reg = case.startswith("registered")
    multi = codecs[:int(case[-1])] if case.startswith("multi") else None
    c, svc = codecs[0], None
    if case == "svc":
        c = qhuff.Codec(0)
        svc = c.service()
    try:
        k = 0
        big = name is None
        for op in ((0, "dec") if big else (0, 7, "dec")):
            data, off = b.inputs(op)
            n = len(off) - 1
            in_bytes = int(off[-1] - off[0])
            for r_in, r_out in ([(5, 11)] if big else [(1, 8), (8, 13), (13, 1)]):
                fill = FILLS[k % 3]
                back = (0, 3, 200)[k % 3]
                ar = Arena(codec_specs(op, in_bytes, n, r_in, r_out, k),
                           seed=5000 + k, guard=8192 if reg else GUARD)
                load_codec(ar, data, off, back)
                ar.neighbours("in", fill)
                ar.commit(False)
                names = [s[0] for s in codec_specs(op, 0, 0, 0, 0, 0)]
                done = register_all(ar, names) if reg else []
                try:
                    rc = host_codec_call(L, svc._svc if svc else c._ctx, op,
                                         ar, n, back, multi, svc is not None)
                finally:
                    unregister_all(ar, done)
                assert rc == qhuff.OK
                check_codec(ar, ar.after(), op, b.want(op), n)
                k += 1
        if svc:
            assert svc.stats()[0] == k               # served by the kernel
        for x in (multi or [c]):
            assert x.device_error() == 0
    finally:
        if svc:
            svc.close()
            c.close()


@pytest.mark.gpu
def test_host_literals_contract(codec):
    """qhuff_decode_literals_host on the literals of one interop stream
    (fb-resp: Huffman and raw ones): `out` of qhuff_literals_bound bytes,
    buf exactly the stream's bytes"""
    raw = open(os.path.join(HERE, "golden", "data", "fb-resp.out.256.100.1"),
               "rb").read()
    buf, lits = b"", []
    for sid, payload in Q.read_interop(raw):
        if sid == 0:
            rc, ls, _ = qhuff.scan_encoder_stream(payload, len(buf))
        else:
            rc, ls = qhuff.scan_field_section(payload, len(buf))
            if rc == qhuff.ETRUNC:
                continue
        assert rc == qhuff.OK
        buf += payload
        lits += ls
    n = len(lits)
    assert n > 100 and any(l.huffman for l in lits) \
        and any(not l.huffman for l in lits)
    want = b""
    woff = [0]
    for l in lits:
        p = buf[l.pos:l.pos + l.len]
        if l.huffman:
            st, p = O.huff_decode(p)
            assert st == O.OK
        want += p
        woff.append(len(want))
    arr = (qhuff.Literal * n)(*lits)
    bound = int(qhuff.lib().qhuff_literals_bound(arr, n))
    for k, (r_in, r_out) in enumerate([(1, 8), (8, 13), (13, 1)]):
        ar = Arena([("in", len(buf), r_in), ("out", bound, r_out),
                    ("out_off", 4 * (n + 1), 4 * k), ("status", n, 2 * k + 1)],
                   seed=6000 + k)
        ar.put("in", np.frombuffer(buf, dtype=np.uint8))
        ar.neighbours("in", FILLS[k])
        ar.commit(False)
        rc = qhuff.lib().qhuff_decode_literals_host(
            codec._ctx, ar.addr("in"), arr, n, ar.addr("out"),
            ar.addr("out_off"), ar.addr("status"))
        assert rc == qhuff.OK
        check_codec(ar, ar.after(), "dec",
                    (np.frombuffer(want, dtype=np.uint8),
                     np.array(woff, dtype=np.uint32), np.zeros(n, np.uint8)), n)
    assert codec.device_error() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["ragged", "long", "empty"])
def test_host_hash_contract(codec, kind):
    """qhuff_xxh32_headers_host: n words per output, guarded"""
    data, off = hash_shape(kind)
    n = (len(off) - 1) // 2
    want = O.xxh32_headers(data, off)
    for k, r_in in enumerate((1, 8, 13)):
        back = (0, 3, 200)[k]
        ar = Arena([("in", len(data), r_in), ("in_off", 4 * len(off), 4 * k),
                    ("h1", 4 * n, 4 * (k + 1)), ("h2", 4 * n, (4 * k + 12) % 16)],
                   seed=7000 + k)
        load_codec(ar, data, off, back)
        ar.neighbours("in", FILLS[k])
        ar.commit(False)
        rc = qhuff.lib().qhuff_xxh32_headers_host(
            codec._ctx, ar.addr("in", back), ar.addr("in_off"), n,
            qhuff.XXH_SEED, ar.addr("h1"), ar.addr("h2"))
        assert rc == qhuff.OK
        img = ar.after()
        assert np.array_equal(ar.get(img, "h1", np.uint32), want[0])
        assert np.array_equal(ar.get(img, "h2", np.uint32), want[1])
        ar.check(img, {"h1": 4 * n, "h2": 4 * n})
    assert codec.device_error() == 0


# ---- GPU: registration is checked over the range a shard writes ---------------------

@pytest.mark.gpu
@pytest.mark.parametrize("encode", [True, False], ids=["encode", "decode"])
def test_multi_registered_first_share_only(codecs, encode):
    """A two-context host call, each shard past the 4 MB threshold, whose
    `out` is registered over the first shard's share only (out_off and
    status fully): shard 1 writes at out + base[1], outside that range, so
    the call must not take `out` for registered on the strength of
    [out, out + bound(shard)).  QHUFF_OK, the single-context call's bytes,
    offsets and statuses, guards intact."""
    L = qhuff.lib()
    b = _past_small()
    op = 0 if encode else "dec"
    data, off = b.inputs(op)
    n = len(off) - 1
    in_bytes = int(off[-1])
    cuts = qhuff.shard_cuts(off, 2)
    share = [bound_of(op, int(off[cuts[k + 1]] - off[cuts[k]]),
                      int(cuts[k + 1] - cuts[k])) for k in range(2)]
    assert min(share) > 4 << 20 and max(share) < bound_of(op, in_bytes, n)
    # the single-context call, into a plain buffer
    one = [np.zeros(bound_of(op, in_bytes, n), np.uint8),
           np.zeros(n + 1, np.uint32), np.zeros(n, np.uint8)]
    c = codecs[0]
    if encode:
        c.encode_host(data, off, 0, out=one[0], out_off=one[1])
    else:
        c.decode_host(data, off, out=one[0], out_off=one[1], status=one[2])
    want = b.want(op)
    assert np.array_equal(one[1], want[1])
    assert np.array_equal(one[0][:one[1][-1]], want[0])
    ar = Arena(codec_specs(op, in_bytes, n, 0, 0, 0), seed=8000, guard=8192)
    load_codec(ar, data, off, 0)
    ar.commit(False)
    ptrs = [(ar.addr("out"), max(share)), (ar.addr("out_off"), 4 * (n + 1))]
    if not encode:
        ptrs.append((ar.addr("status"), n))
    done = []
    try:
        for p, nb in ptrs:
            assert L.qhuff_host_register(p, nb) == qhuff.OK
            done.append(p)
        rc = host_codec_call(L, None, op, ar, n, 0, multi=codecs[:2])
    finally:
        for p in done:
            assert L.qhuff_host_unregister(p) == qhuff.OK
    assert rc == qhuff.OK
    img = ar.after()
    check_codec(ar, img, op, want, n)
    assert np.array_equal(ar.get(img, "out_off", np.uint32), one[1])
    if not encode:
        assert np.array_equal(ar.get(img, "status"), one[2])
    for x in codecs[:2]:
        assert x.device_error() == 0
