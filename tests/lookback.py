"""Batches and arithmetic for the shared coordination layer of the five tile
calls: the two-level look-back (LookBack, qhuff_device.h), the ticket claims
and the pending ring of tile_pipeline (qhuff_pipeline.h), and the host's
workspace, epoch and parity bookkeeping (prepare_launch, qhuff_host.cpp).
No device here: tests/test_lookback.py runs the kernels on these batches.

The batches go up to ~800k strings, so they are built with numpy and every
expectation is one call of the oracle over the whole batch
(oracle_lib.encode_batch / decode_batch), never the library's own result.
The super-tile arithmetic of the kernels is restated in Python (supers,
in_super, windows, cap_after) so that a test can say which window and lane
a tile of a named case sits in."""
import functools

import numpy as np

import _paths  # noqa: F401
import limits as L
import oracle_lib as O
import qhuff

TS = 64                       # kWT: strings per tile
SUPER = 64                    # kSuper: tiles per super tile
WINDOW = 64                   # lanes of a poll window
CAP_FLOOR = 4096              # prepare_launch: the smallest workspace, tiles
EPOCH_BITS = 22               # kEpochMask
EPOCH_LAST = (1 << EPOCH_BITS) - 1
PUBLISHED = 4                 # kDepth + 1: tiles a wave publishes before it
                              # waits for its oldest one's look-back
SLOW_LEN = 24576              # with_slow "slow": bytes of the long string
SLOT_LEN = 100                # with_slow "slot": bytes of each string

_ALPHA = np.frombuffer(qhuff.TOKEN_ALPHABET, dtype=np.uint8)
_CODE_LEN = np.array(L.CODE_LEN, dtype=np.int64)


# ---- the arithmetic ----------------------------------------------------------------

def supers(T):
    """super tiles of a launch of T tiles"""
    return (T + SUPER - 1) // SUPER


def in_super(T, s):
    """tiles of super tile s (LookBack::super_agg / finish: in_super)"""
    assert 0 <= s < supers(T)
    return min(SUPER, T - s * SUPER)


def publisher(T, s):
    """the tile that publishes super tile s's inclusive flag"""
    return s * SUPER + in_super(T, s) - 1


def windows(tile):
    """what the look-back of `tile` polls: (tile window, [super window at
    back 0, 1, 2]).  The tile window is the earlier tiles of its super tile,
    nearest first (empty for the first tile of a super tile: nq == 0); a
    super window has one entry a lane, the super tile s - 1 - lane - 64 back
    or None where that is below 0 (super_val: inclusive 0)."""
    s = tile // SUPER
    nq = tile - s * SUPER
    tw = [tile - 1 - q for q in range(nq)]
    sw = []
    for back in range(3):
        j = [s - 1 - lane - WINDOW * back for lane in range(WINDOW)]
        sw.append([x if x >= 0 else None for x in j])
    return tw, sw


def cap_after(history):
    """(cap_tiles, cap_super) of a context after each launch of `history`
    (tile counts), and whether that launch reallocated (prepare_launch)"""
    cap, out = 0, []
    for T in history:
        grew = T > cap
        if grew:
            cap = max(CAP_FLOOR, T)
        out.append((cap, (cap + SUPER - 1) // SUPER, grew))
    return out


def epochs(epoch0, launches):
    """the epoch of each of `launches` launches on a context opened at
    epoch0, and whether prepare_launch wrapped (memset, restart at 1)"""
    e, out = epoch0 & EPOCH_LAST, []
    for _ in range(launches):
        e = (e + 1) & EPOCH_LAST
        wrapped = e == 0
        if wrapped:
            e = 1
        out.append((e, wrapped))
    return out


# ---- the batches -------------------------------------------------------------------

def enc_sizes(data, off, mode):
    """bytes of each string's encode output, from the code lengths alone:
    mode 0 the Huffman payload, mode 7 one length byte and the shorter of
    payload and raw string (strings below 127 bytes)"""
    bits = np.zeros(len(data) + 1, dtype=np.int64)
    np.cumsum(_CODE_LEN[data], out=bits[1:])
    o = off.astype(np.int64)
    huff = (bits[o[1:]] - bits[o[:-1]] + 7) // 8
    if mode == 0:
        return huff
    assert mode == 7
    raw = np.diff(o)
    assert raw.max(initial=0) < 127
    return 1 + np.where(huff < raw, huff, raw)


def prefix(sizes):
    """want_off: the uint64 cumulative sum in front of each string"""
    w = np.zeros(len(sizes) + 1, dtype=np.uint64)
    np.cumsum(sizes, out=w[1:], dtype=np.uint64)
    return w


class Batch:
    """raw strings (data, off), their Huffman batch (huff, huff_off) and the
    oracle's results over the whole batch"""

    def __init__(self, data, off, name):
        self.data = np.ascontiguousarray(data, dtype=np.uint8)
        self.off = np.ascontiguousarray(off, dtype=np.uint32)
        self.n = len(off) - 1
        self.T = (self.n + TS - 1) // TS
        self.name = name
        self.huff, self.huff_off = O.encode_batch(self.data, self.off, 0)

    def __repr__(self):
        return self.name

    @functools.lru_cache(maxsize=None)
    def enc(self, mode):
        """(bytes, want_off) of an encode in `mode`"""
        out, o_off = (self.huff, self.huff_off) if mode == 0 else \
            O.encode_batch(self.data, self.off, mode)
        want = prefix(enc_sizes(self.data, self.off, mode))
        assert int(want[-1]) < 1 << 32
        assert np.array_equal(want, o_off.astype(np.uint64))
        return out, want

    @functools.cached_property
    def dec(self):
        """(bytes, want_off, status) of a decode of the Huffman batch"""
        out, o_off, st = O.decode_batch(self.huff, self.huff_off)
        want = prefix(np.diff(self.off.astype(np.int64)))
        assert np.array_equal(want, o_off.astype(np.uint64))
        assert np.array_equal(out, self.data) and not st.any()
        return out, want, st

    @functools.lru_cache(maxsize=None)
    def expect(self, call, mode=0):
        """(bytes, out_off as uint32) a call has to return: "encode" in
        `mode`, "encwire" (every item a 7-bit literal: mode 7) or one of the
        decodes"""
        if call == "encode":
            out, want = self.enc(mode)
        elif call == "encwire":
            out, want = self.enc(7)
        else:
            out, want, _ = self.dec
        return np.ascontiguousarray(out), want.astype(np.uint32)

    def tile(self, t):
        """strings [a, b) of tile t"""
        return t * TS, min(self.n, (t + 1) * TS)


def _pack(lens, rng):
    off = np.zeros(len(lens) + 1, dtype=np.uint32)
    np.cumsum(lens, out=off[1:])
    data = _ALPHA[rng.integers(0, len(_ALPHA), int(off[-1]))]
    return data, off


def _count(T, last):
    assert T >= 1 and 1 <= last <= TS
    return TS * (T - 1) + last


@functools.lru_cache(maxsize=None)
def tiny(T, last, seed=0):
    """T tiles, `last` strings in the last one, of 0-3 token bytes; tile 2
    all empty, and with more than 128 tiles all of super tile 1 (tiles
    64..127): a tile's and a super tile's aggregate of 0"""
    n = _count(T, last)
    rng = np.random.default_rng([T, last, seed])
    lens = rng.integers(0, 4, n)
    lens[2 * TS:3 * TS] = 0
    if T > 2 * SUPER:
        lens[SUPER * TS:2 * SUPER * TS] = 0
    data, off = _pack(lens, rng)
    return Batch(data, off, "tiny(%d,%d)" % (T, last))


@functools.lru_cache(maxsize=None)
def twin(T, last, k):
    """the same shape, every string exactly k token bytes: two launches of
    equal tile count differ in every prefix"""
    n = _count(T, last)
    rng = np.random.default_rng([T, last, k, 1])
    data, off = _pack(np.full(n, k, dtype=np.int64), rng)
    return Batch(data, off, "twin(%d,%d,%d)" % (T, last, k))


def with_slow(batch, tile, kind, slow_len=SLOW_LEN):
    """`batch` with the strings of one tile replaced so that the tile is
    slow: "slow" its string 0 of slow_len token bytes (encode output and
    decode payload past every slot: slow_tile), "slot" each of its strings of
    100 (unstaged, the output fits a big slot: pending with a slot on the
    full kernels, out of line on the lean ones)"""
    a, b = batch.tile(tile)
    lens = np.diff(batch.off.astype(np.int64))
    rng = np.random.default_rng([batch.T, batch.n, tile, int(kind == "slow")])
    if kind == "slow":
        new = lens[a:b].copy()
        new[0] = slow_len
    else:
        assert kind == "slot"
        new = np.full(b - a, SLOT_LEN, dtype=np.int64)
    tile_data, _ = _pack(new, rng)
    # (string 0 apart, a "slow" tile keeps its bytes)
    if kind == "slow":
        keep = batch.data[int(batch.off[a]) + int(lens[a]):int(batch.off[b])]
        tile_data[slow_len:] = keep
    data = np.concatenate([batch.data[:int(batch.off[a])], tile_data,
                           batch.data[int(batch.off[b]):]])
    lens = np.concatenate([lens[:a], new, lens[b:]])
    off = np.zeros(batch.n + 1, dtype=np.uint32)
    np.cumsum(lens, out=off[1:])
    return Batch(data, off, "%s+%s@%d" % (batch.name, kind, tile))


@functools.lru_cache(maxsize=None)
def slow_case(T, last, tile, kind):
    return with_slow(tiny(T, last), tile, kind)


def tile_paths(batch, t):
    """(decode path, encode path) of tile t by the layout model
    (limits.classify / classify_enc), run on that tile alone in front of the
    bytes up to its 16-byte boundary: what the kernels see of a batch whose
    buffers are 16-byte aligned"""
    a, b = batch.tile(t)
    out = []
    for data, off, sizes in (
            (batch.huff, batch.huff_off,
             np.diff(batch.off.astype(np.int64))[a:b]),
            (batch.data, batch.off, enc_sizes(batch.data, batch.off, 0)[a:b])):
        base = int(off[a]) & ~15
        o = off[a:b + 1].astype(np.int64) - base
        if data is batch.huff:
            info = L.classify(o, 0, sizes)
        else:
            info = L.classify_enc(data[base:int(off[b])].tobytes(), o, 0, 0,
                                  sizes)
        assert len(info) == 1
        out.append(info[0]["path"])
    return tuple(out)


# ---- the lean calls over a tiny batch ----------------------------------------------

ITEM_DTYPE = np.dtype([("ival", "<u4"), ("int_bits", "u1"),
                       ("int_first", "u1"), ("str_bits", "u1"),
                       ("str_first", "u1")])
LITERAL_DTYPE = np.dtype([("pos", "<u4"), ("len", "<u4"), ("huffman", "u1"),
                          ("prefix_bits", "u1"), ("kind", "u1"),
                          ("hdr_len", "u1"), ("instr", "<u4")])


class Wire:
    """encode_wire, decode_wire and decode_stream over a batch of strings
    below 127 bytes: every item a 7-bit-prefix literal, so that the
    encode_wire output is the oracle's mode-7 batch; every literal behind
    its one length byte in that output; every stream string fresh and
    final"""

    def __init__(self, batch):
        self.batch = batch
        n = batch.n
        items = np.zeros(n, dtype=ITEM_DTYPE)
        items["str_bits"] = 7
        self.items = items.view(np.uint8).copy()
        self.wire, self.wire_off = batch.enc(7)
        at = self.wire_off[:-1].astype(np.int64)
        head = self.wire[at]
        lits = np.zeros(n, dtype=LITERAL_DTYPE)
        lits["pos"] = at + 1
        lits["len"] = head & 0x7f
        lits["huffman"] = head >> 7
        lits["prefix_bits"] = 7
        lits["kind"] = qhuff.LIT_VALUE
        assert np.array_equal(at + 1 + lits["len"],
                              self.wire_off[1:].astype(np.int64))
        self.lits = lits.view(np.uint8).copy()
        self.lit_fields = lits
