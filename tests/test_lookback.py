"""The layer all five tile calls share, at its own edges: the two-level
look-back (LookBack, qhuff_device.h), the ticket claims and the drain of
tile_pipeline (qhuff_pipeline.h), and the workspace, epoch and parity
bookkeeping of prepare_launch / coord (qhuff_host.cpp).  DESIGN section 4,
"The look-back's edges", names the comparison each case sits on.

CPU part: the builders of lookback.py give the paths, sums and window lanes
the cases are named for.  GPU part: every launch is compared whole with the
oracle -- out_off[0..n], the statuses, every output byte -- in
sentinel-filled buffers, and leaves no device error.  Nothing here aims at
the spin limit: every launch is one the code is meant to complete."""
import functools
import os

import numpy as np
import pytest

import _paths  # noqa: F401
import lookback as B
import oracle_lib as O
import qhuff
from test_encode_wire import item, item_bytes
from test_launch_frame import SENTINEL, dev
from test_stream_decode import fresh, oracle_chunk
from test_wire_decode import lit

E, D = qhuff.KIND_ENCODE, qhuff.KIND_DECODE
W_256CU = 3072                # grid_waves of either kind on 256 CUs

EDGE_TILES = (1, 63, 64, 65, 128, 129, 4095, 4096, 4097, 8192, 8193, 8257)
SLOW_TILES = (130, 321)       # a spread launch on the default grid; 5 super
                              # tiles + 1
SLOW_LAST = {130: 64, 321: 40}
CAP_HISTORY = (3, 4096, 4097, 4096, 70, 8193, 4097, 1)
CAP_KINDS = (E, D, D, E, E, D, D, E)


def deep_tiles(W):
    """every wave of a grid of W publishes kDepth + 1 tiles, and 65 more"""
    return B.PUBLISHED * W + 65


def slow_positions(T):
    return (0, 63, 64, T - 1)


# ---- CPU: what the cases rely on -----------------------------------------------------

def test_super_arithmetic():
    assert [B.supers(T) for T in (1, 64, 65, 4096, 4097, 8193)] == \
        [1, 1, 2, 64, 65, 129]
    # a partial last super tile, down to one tile: old >> 48 == 0 in
    # super_agg, and that tile is first (nq == 0) and publisher at once
    for T in (65, 129, 4097, 8193, 321):
        s = B.supers(T) - 1
        assert B.in_super(T, s) == 1 and B.publisher(T, s) == T - 1
        assert B.windows(T - 1)[0] == []
    assert B.in_super(8193, 128) == 1               # alone in super 128
    assert B.in_super(8257, 129) == 1 and B.in_super(8257, 128) == 64
    assert B.in_super(63, 0) == 63 and B.publisher(63, 0) == 62
    assert B.in_super(4095, 63) == 63 and B.in_super(4096, 63) == 64
    # the tile window: nearest first, never past the super tile's start
    assert B.windows(64)[0] == [] and B.windows(127)[0][-1] == 64
    assert B.windows(63)[0] == list(range(62, -1, -1))
    # the j < 0 clamp in the first, second and third window
    first = lambda sw: [x is None for x in sw].index(True)
    assert first(B.windows(64)[1][0]) == 1          # super 1: lane 0 alone
    assert None not in B.windows(4096)[1][0]       # super 64: none yet
    tw, sw = B.windows(4097 - 1)                    # super 64
    assert sw[0] == list(range(63, -1, -1)) and sw[1] == [None] * 64
    tw, sw = B.windows(8193 - 1)                    # super 128
    assert None not in sw[0] and None not in sw[1] and sw[2] == [None] * 64
    tw, sw = B.windows(8257 - 1)                    # super 129
    assert sw[1][-1] == 1 and sw[2][:2] == [0, None]
    # the deep case on 256 CUs: tiles of the super tiles 129..192 read real
    # flags and clamped lanes in their third window; (kDepth + 1) W tiles
    # = 192 super tiles are all that can be published in front of an
    # unresolved tile, so a fourth window is never polled
    T = deep_tiles(W_256CU)
    assert T == 12353 and B.supers(T) == 194 and B.in_super(T, 193) == 1
    assert B.PUBLISHED * W_256CU == 192 * B.SUPER
    for s in (129, 150, 192):
        sw = B.windows(s * B.SUPER + 5)[1]
        assert None not in sw[0] and None not in sw[1]
        assert sw[2][0] == s - 129 and sw[2][s - 129] == 0
        assert sw[2][s - 128:] == [None] * (64 - (s - 128))


def test_capacity_and_epoch_arithmetic():
    caps = B.cap_after(CAP_HISTORY)
    assert caps == [(4096, 64, True), (4096, 64, False), (4097, 65, True),
                    (4097, 65, False), (4097, 65, False), (8193, 129, True),
                    (8193, 129, False), (8193, 129, False)]
    # each kind on both parities
    par = {(k, e & 1) for k, (e, _) in zip(CAP_KINDS, B.epochs(0, 8))}
    assert par == {(E, 0), (E, 1), (D, 0), (D, 1)}
    # the wrap: the launch after epoch 2^22 - 1 restarts at 1, the same
    # parity as the launch before it
    ep = B.epochs(B.EPOCH_LAST - 5, 14)
    assert [w for _, w in ep].index(True) == 5 and ep[4] == (B.EPOCH_LAST, False)
    assert ep[5] == (1, True) and ep[4][0] & 1 == ep[5][0] & 1
    assert sum(w for _, w in ep) == 1
    assert [w for _, w in B.epochs(B.EPOCH_LAST - 2, 14)].index(True) == 2
    assert B.epochs(B.EPOCH_LAST, 2) == [(1, True), (2, False)]


def test_zero_aggregates():
    b = B.tiny(129, 1)
    for sizes in (np.diff(b.dec[1]), np.diff(b.enc(0)[1])):
        per_tile = np.add.reduceat(sizes.astype(np.int64),
                                   np.arange(0, b.n, B.TS))
        assert per_tile[2] == 0
        assert per_tile[64:128].sum() == 0          # super tile 1
        assert per_tile[:64].sum() > 0 and per_tile[128] >= 0
        assert (per_tile[3:64] > 0).all()
    assert np.diff(B.tiny(128, 64).dec[1])[64 * 64:].sum() > 0


def test_twins_differ_in_every_prefix():
    a, b = B.twin(70, 64, 1), B.twin(70, 64, 3)
    assert a.n == b.n == 70 * 64
    assert (a.dec[1][1:] != b.dec[1][1:]).all()
    assert (a.enc(0)[1][1:] != b.enc(0)[1][1:]).all()
    assert (a.enc(0)[1][1:] != b.dec[1][1:]).all()


@pytest.mark.parametrize("T", SLOW_TILES)
@pytest.mark.parametrize("kind", ["slow", "slot"])
def test_slow_tiles_reach_their_paths(T, kind):
    """the replaced tile is classified `kind` for decode and for encode, at
    the residue it has in the batch; the tiny tiles around it are fast"""
    for pos in slow_positions(T):
        b = B.slow_case(T, SLOW_LAST[T], pos, kind)
        assert b.T == T and b.n == B.tiny(T, SLOW_LAST[T]).n
        assert B.tile_paths(b, pos) == (kind, kind), (b, pos)
        for t in {0, 1, 2, 62, 63, 64, 65, 127, 128, T - 2, T - 1} - {pos}:
            assert B.tile_paths(b, t) == ("fast", "fast"), (b, t)
        b.dec, b.enc(0)                              # (the oracle agrees)
    if kind == "slow":
        b = B.slow_case(T, SLOW_LAST[T], 0, kind)
        assert int(b.huff_off[1]) >= 15360 > 12288  # kBigSlotBytes
        assert int(b.huff_off[1]) > 7679


def test_deep_case_slow_tile():
    b = B.with_slow(B.tiny(300, 64), 0, "slow")
    assert B.tile_paths(b, 0) == ("slow", "slow")
    assert B.tile_paths(b, 1) == ("fast", "fast")


def test_epoch_knob_is_in_the_library():
    """the name test_epoch_wrap sets is one the built library reads"""
    with open(qhuff.LIB_PATH, "rb") as f:
        assert b"QHUFF_EPOCH0\0" in f.read()


@functools.lru_cache(maxsize=None)
def wire_of(T, last):
    return B.Wire(B.tiny(T, last))


def test_wire_identities():
    """the vectorised expectations of the three lean calls, on a sample of
    1,000 strings against the per-item references: item_bytes for the
    encode_wire output, the oracle's complete-string decode for a literal,
    its resumable decoder for a fresh final chunk"""
    w = wire_of(4097, 1)
    b = w.batch
    assert qhuff.items_check(w.items) == (qhuff.OK, None)
    assert qhuff.literals_check(w.lits) == (qhuff.OK, None)
    rng = np.random.default_rng(5)
    sample = sorted({0, 1, b.n - 1, 2 * 64, 2 * 64 + 1}
                    | set(int(i) for i in rng.integers(0, b.n, 1000)))
    raw, wire, huff = b.data.tobytes(), w.wire.tobytes(), b.huff.tobytes()
    it = item(str_bits=7, str_first=0)
    huffman = 0
    for i in sample:
        s = raw[b.off[i]:b.off[i + 1]]
        assert len(s) <= 3
        assert wire[int(w.wire_off[i]):int(w.wire_off[i + 1])] == \
            item_bytes(it, s)
        assert w.items[8 * i:8 * i + 8].tobytes() == \
            qhuff.items_array([it]).tobytes()
        f = w.lit_fields[i]
        payload = wire[int(f["pos"]):int(f["pos"]) + int(f["len"])]
        assert w.lits[16 * i:16 * i + 16].tobytes() == qhuff.literals_array(
            [lit(int(w.wire_off[i]) + 1, payload, int(f["huffman"]))]).tobytes()
        if f["huffman"]:
            huffman += 1
            assert O.huff_decode(payload) == (O.OK, s)
        else:
            assert payload == s
        chunk = huff[b.huff_off[i]:b.huff_off[i + 1]]
        assert oracle_chunk(fresh(), chunk, True) == (qhuff.DEC_OK, s, 1)
    assert 0 < huffman < len(sample)


# ---- GPU ---------------------------------------------------------------------------

def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("gpu test without a GPU")
    return torch


def open_codec(env):
    """a codec opened with `env` set around the constructor alone"""
    _torch()
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return qhuff.Codec(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def codec():
    c = open_codec({})
    yield c
    c.close()


@pytest.fixture(scope="module")
def lean_codec():
    c = open_codec({"QHUFF_KERNELS": "lean"})
    yield c
    c.close()


@pytest.fixture(scope="module", params=["full", "lean"])
def small_grid_codec(request):
    """a grid of a few workgroups (test_limits.small_grid_codec): every
    batch here is claimed by tickets, each wave holding pending tiles"""
    c = open_codec({"QHUFF_GRID_PCT": "1", "QHUFF_KERNELS": request.param})
    yield c
    c.close()


@pytest.fixture(scope="module",
                params=["default", "lean", "small-full", "small-lean"])
def any_codec(request):
    env = {"default": {}, "lean": {"QHUFF_KERNELS": "lean"},
           "small-full": {"QHUFF_GRID_PCT": "1", "QHUFF_KERNELS": "full"},
           "small-lean": {"QHUFF_GRID_PCT": "1", "QHUFF_KERNELS": "lean"}}
    c = open_codec(env[request.param])
    yield c
    c.close()


class Inputs:
    """a batch's inputs on the device"""

    def __init__(self, b, wire=None):
        self.b = b
        self.data, self.off = dev(b.data, 16), dev(b.off)
        self.huff, self.huff_off = dev(b.huff, 16), dev(b.huff_off)
        if wire is not None:
            self.wire = dev(wire.wire, 16)
            self.items, self.lits = dev(wire.items), dev(wire.lits)
            self.flags = dev(np.full(b.n, qhuff.STREAM_FINAL, np.uint8))


@functools.lru_cache(maxsize=4)
def inputs(b):
    return Inputs(b)


class Launch:
    """one call into sentinel-filled buffers of its bound, and its check
    against the oracle"""

    def __init__(self, inp, call, mode=0, wire=None):
        torch = _torch()
        b = inp.b
        n = b.n
        self.inp, self.call, self.b, self.mode = inp, call, b, mode
        bound = {
            "encode": lambda: qhuff.encode_bound(len(b.data), n, mode),
            "decode": lambda: qhuff.decode_bound(len(b.huff), n),
            "stream": lambda: qhuff.decode_stream_bound(len(b.huff), n),
            "wire": lambda: qhuff.literals_bound(wire.lits),
            "encwire": lambda: qhuff.encode_wire_bound(len(b.data), n),
        }[call]()
        self.out = torch.full((max(bound, 1),), SENTINEL, dtype=torch.uint8,
                              device="cuda")
        self.out_off = torch.full((n + 1,), -1, dtype=torch.int32,
                                  device="cuda")
        self.status = torch.full((n,), SENTINEL, dtype=torch.uint8,
                                 device="cuda")
        self.state = torch.zeros((n, 2), dtype=torch.uint8, device="cuda")

    def go(self, codec, stream=None):
        """(the buffers' fill is ordered before it by the caller when
        `stream` is not the one they were filled on)"""
        inp, call, n, mode = self.inp, self.call, self.b.n, self.mode
        if call == "encode":
            codec.encode_into(inp.data, inp.off, n, mode, self.out,
                              self.out_off, stream)
        elif call == "decode":
            codec.decode_into(inp.huff, inp.huff_off, n, self.out,
                              self.out_off, self.status, stream)
        elif call == "stream":
            codec.decode_stream_into(inp.huff, inp.huff_off, n, self.state,
                                     inp.flags, self.out, self.out_off,
                                     self.status, stream)
        elif call == "wire":
            codec.decode_wire_into(inp.wire, inp.lits, n, None, self.out,
                                   self.out_off, self.status, stream)
        else:
            codec.encode_wire_into(inp.data, inp.off, inp.items, n, self.out,
                                   self.out_off, stream)
        return self

    def check(self):
        """(after a synchronisation) compared on the device: what comes back
        to the host is a verdict, and the first difference when there is one"""
        torch = _torch()
        b, tag = self.b, (self.call, self.b)
        want, want_off = b.expect(self.call, self.mode)
        eq = self.out_off == dev(want_off)
        if not bool(eq.all()):
            i = int(torch.nonzero(~eq)[0])
            assert False, (tag, "out_off differs first at string", i, "tile",
                           i // B.TS, int(self.out_off[i]) & 0xffffffff,
                           int(want_off[i]))
        total = int(want_off[-1])
        assert total == len(want), tag
        if total:
            assert torch.equal(self.out[:total], dev(want)), tag
        assert bool((self.out[total:] == SENTINEL).all()), tag
        if self.call in ("decode", "stream", "wire"):
            assert bool((self.status == qhuff.DEC_OK).all()), tag
        if self.call == "stream":
            assert bool((self.state[:, 1] == 1).all()), tag


def run_checked(codec, b, calls=("encode", "decode"), mode=0):
    torch = _torch()
    inp = inputs(b)
    res = [Launch(inp, call, mode).go(codec) for call in calls]
    torch.cuda.synchronize()
    assert codec.device_error() == 0, b
    for r in res:
        r.check()


# a. tile-count edges

@pytest.mark.gpu
@pytest.mark.parametrize("last", [1, 64])
@pytest.mark.parametrize("T", EDGE_TILES)
def test_tile_count_edges(codec, T, last):
    run_checked(codec, B.tiny(T, last))


@pytest.mark.gpu
def test_tile_count_edge_mode7(codec):
    run_checked(codec, B.tiny(4097, 1), ("encode",), 7)


@pytest.mark.gpu
@pytest.mark.parametrize("T", [65, 129, 4097])
def test_tile_count_edges_small_grid(small_grid_codec, T):
    for last in (1, 64):
        run_checked(small_grid_codec, B.tiny(T, last))


# b. a slow tile at each position the look-back treats differently

@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["slow", "slot"])
@pytest.mark.parametrize("T", SLOW_TILES)
def test_slow_tile_positions(any_codec, T, kind):
    """tile 0 (every later tile's prefix hangs on it), 63 (publishes super
    0's inclusive flag), 64 (first of a super tile: no tile window) and
    T - 1 (resolved in the drain; alone in its super tile at T = 321)"""
    for pos in slow_positions(T):
        run_checked(any_codec, B.slow_case(T, SLOW_LAST[T], pos, kind))


# c. the deep look-back

def _timed(codec, b, call):
    torch = _torch()
    inp = inputs(b)
    codec.timing(True)
    try:
        codec.timing_read()
        r = Launch(inp, call).go(codec)
        torch.cuda.synchronize()
        t = codec.timing_read()
    finally:
        codec.timing(False)
    assert codec.device_error() == 0, b
    r.check()
    assert len(t) == 1 and t[0][0] == (E if call == "encode" else D)
    return t[0][1]


@pytest.mark.gpu
@pytest.mark.parametrize("call", ["decode", "encode"])
@pytest.mark.parametrize("variant", ["full", "lean"])
def test_deep_lookback(codec, lean_codec, variant, call):
    """T = 4 W + 65 tiles of tiny strings behind a slow tile 0 (W the
    grid's waves: 12,353 tiles, 790k strings on 256 CUs): every wave
    publishes kDepth + 1 tiles and waits behind tile 0, so tiles of the
    super tiles from 129 on meet no inclusive super flag in the two windows
    polled with the tile window, poll a third (poll_super(c, 2)) and use its
    j < 0 clamp.  Its twin without the slow tile runs too.  No time is
    asserted; the device times of both launches are printed.  Measured on
    MI355X (256 CUs), slow / twin in us: full decode 10,040 / 33.0, full
    encode 3,917 / 37.2, lean decode 6,910 / 33.2, lean encode 3,076 / 37.9
    (80 to 300 times the twin).  A profile build counted the waves whose
    drain polled a third window: 235 to 571 in three of these four slow
    launches, none in the lean decode, and 69 to 401 in each twin -- the
    shape reaches it on most launches, the slow tile does not force it
    (DESIGN section 4)."""
    c = codec if variant == "full" else lean_codec
    W = c.grid_waves(E if call == "encode" else D)
    base = B.tiny(deep_tiles(W), 64)
    slow = B.with_slow(base, 0, "slow")
    us_twin = _timed(c, base, call)
    us_slow = _timed(c, slow, call)
    print("deep look-back %s %s: W %d, T %d, slow %.1f us, twin %.1f us, "
          "ratio %.1f" % (variant, call, W, base.T, us_slow, us_twin,
                          us_slow / us_twin))


# d. workspace capacity and parities

def _twin_plan(history, kinds):
    """(kind, batch) of each launch: the k = 1 and k = 3 twins alternately
    at equal tile counts"""
    seen, plan = {}, []
    for T, kind in zip(history, kinds):
        k = (1, 3)[seen.get(T, 0) % 2]
        seen[T] = seen.get(T, 0) + 1
        plan.append((kind, B.twin(T, 64, k)))
    return plan


# A partial last super tile that a later launch on the same parity fills and
# reads, with one smaller launch between and no growth: 8129 tiles leave one
# tile's count and bytes in accumulator 127; the 1-tile launch has to clear
# it (clear_next_launch over cap_super, not over its own tile count), or the
# second 12289-tile launch publishes super tile 127's aggregate at its 63rd
# add, with the stale bytes in it, and the tiles of super tiles 128-191 sum
# that.  (An accumulator left with a whole super tile's count, 64, only
# keeps the aggregate flag from being published: the look-backs then resolve
# through the inclusive flags, slowly and exactly.  So the pairs of equal
# tile counts below pin the tickets, not the accumulators.)
STALE_BIG, STALE_PART = 192 * B.SUPER + 1, 127 * B.SUPER + 1
CAP_TAIL = (STALE_BIG, STALE_PART, 1, STALE_BIG)
CAP_PLAN = (CAP_HISTORY + CAP_TAIL + (4097,) * 6,
            CAP_KINDS + (E, D, E, D) + (E, E, E, D, D, D))


def _run_plan(c, plan, sync, streams):
    """the launches of `plan` in order on one fresh context, each into
    buffers of its own; checked at the end"""
    torch = _torch()
    ins = {b: Inputs(b) for _, b in plan}
    res = [Launch(ins[b], "encode" if kind == E else "decode")
           for kind, b in plan]
    torch.cuda.synchronize()             # the inputs and the sentinels
    for i, r in enumerate(res):
        r.go(c, streams[i % len(streams)] if streams else None)
        if sync:
            torch.cuda.synchronize()
    torch.cuda.synchronize()
    assert c.device_error() == 0
    for r in res:
        r.check()


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["synchronised", "one-stream", "two-streams"])
def test_capacity_and_parities(order):
    """3, 4096, 4097, 4096, 70, 8193, 4097, 1 tiles on a fresh context: the
    4096-tile floor, growth by one tile (cap_super 64 -> 65) and to 8193,
    smaller launches after larger ones (clear_next_launch clears all
    cap_super accumulators of the other parity), encode and decode on both
    parities of the one workspace; then A, B, A at 4097 tiles of each kind:
    launch e + 2 on the accumulators and tickets launch e used and launch
    e + 1 cleared.  Between the two: growth to 12289 tiles, then 8129, 1 and
    12289 again (CAP_TAIL: the one pair here in which an accumulator that was
    not cleared gives a wrong offset)"""
    torch = _torch()
    plan = _twin_plan(*CAP_PLAN)
    assert [b.T for _, b in plan[12:]] == [4097] * 6
    assert plan[12][1] is plan[14][1] is not plan[13][1]
    # the pair: one parity, the partial super tile filled by the later one,
    # other bytes in it, no reallocation between
    ep = [e for e, _ in B.epochs(0, len(plan))]
    assert ep[9] & 1 == ep[11] & 1 and plan[9][1] is not plan[11][1]
    assert B.in_super(STALE_PART, 127) == 1 and B.in_super(STALE_BIG, 127) == 64
    assert [g for _, _, g in B.cap_after([b.T for _, b in plan])[9:]] == \
        [False] * 9
    c = open_codec({})
    try:
        streams = {"synchronised": None,
                   "one-stream": [torch.cuda.Stream()],
                   "two-streams": [torch.cuda.Stream(), torch.cuda.Stream()]}
        _run_plan(c, plan, order == "synchronised", streams[order])
    finally:
        c.close()


# e. the epoch wrap

WRAP_KINDS = (E, D) * 6
WRAP_K = (1, 3, 3, 1)          # launches one and two apart differ in prefix


def _wrap_plan(tail=True):
    plan = [(WRAP_KINDS[i], B.twin(4097, 64, WRAP_K[i % 4]))
            for i in range(12)]
    if tail:
        plan += [(D, B.twin(8193, 64, 1)), (E, B.twin(65, 64, 3))]
    return plan


@pytest.mark.gpu
@pytest.mark.parametrize("epoch0,streams", [(B.EPOCH_LAST - 5, 1),
                                            (B.EPOCH_LAST - 2, 2),
                                            (B.EPOCH_LAST, 1)])
def test_epoch_wrap(epoch0, streams):
    """a context opened QHUFF_EPOCH0 launches into its life runs across the
    22-bit wrap: the launch after epoch 2^22 - 1 memsets the workspace and
    takes epoch 1, the parity of the launch before it, whose tickets and
    accumulators only that memset makes zero.  Twelve alternating launches
    at 4097 tiles, then growth to 8193 after the wrap, then 65; once more
    from 2^22 - 3 on two alternating streams (the memset ordered behind a
    launch on the other stream); and from 2^22 - 1, where the first launch
    allocates, clears and wraps in one call.  (Nothing reads a context's
    epoch back: that these launches cross the wrap rests on B.epochs and on
    qhuff_open reading QHUFF_EPOCH0, which test_epoch_knob_is_in_the_library
    pins by name only.  With the knob ignored the same launches pass without
    a wrap.  In these plans a missing wrap memset shows through the ticket
    counters; test_epoch_wrap_accumulators is the case for the accumulators.)"""
    torch = _torch()
    plan = _wrap_plan()
    wraps = [w for _, w in B.epochs(epoch0, len(plan))]
    assert sum(wraps) == 1 and wraps.index(True) < 12
    c = open_codec({"QHUFF_EPOCH0": str(epoch0)})
    try:
        _run_plan(c, plan, False,
                  [torch.cuda.Stream() for _ in range(streams)])
    finally:
        c.close()


@pytest.mark.gpu
def test_epoch_wrap_accumulators():
    """12289 tiles (the workspace's size), 8129 at epoch 2^22 - 1, 12289 at
    the wrap, on the same parity with no launch between: accumulator 127
    holds one tile's count and bytes that only the wrap's memset clears
    (CAP_TAIL has the mechanism)"""
    torch = _torch()
    plan = [(E, B.twin(STALE_BIG, 64, 1)), (D, B.twin(STALE_PART, 64, 1)),
            (D, B.twin(STALE_BIG, 64, 3))]
    ep = B.epochs(B.EPOCH_LAST - 2, 3)
    assert ep == [(B.EPOCH_LAST - 1, False), (B.EPOCH_LAST, False), (1, True)]
    c = open_codec({"QHUFF_EPOCH0": str(B.EPOCH_LAST - 2)})
    try:
        _run_plan(c, plan, False, [torch.cuda.Stream()])
    finally:
        c.close()


# f. the three lean calls

@pytest.mark.gpu
@pytest.mark.parametrize("T,last", [(64, 64), (65, 1), (4097, 1)])
def test_lean_calls(codec, T, last):
    torch = _torch()
    w = wire_of(T, last)
    inp = Inputs(w.batch, w)
    res = [Launch(inp, call, wire=w).go(codec)
           for call in ("stream", "wire", "encwire")]
    torch.cuda.synchronize()
    assert codec.device_error() == 0
    for r in res:
        r.check()
