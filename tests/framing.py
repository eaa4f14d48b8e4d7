"""Literals whose payload length sits on each boundary of the prefixed length
integer, on each path that frames them (no GPU).

A QPACK literal is H bit + length (an HPACK integer on a 3-, 5- or 7-bit
prefix) + payload.  The kernels size that header in one place (int_len,
size_from_bits) and write it, and encode_wire's integers, in one other:
put_int, through one of two byte sinks.  StageBytes ORs the byte into the
out stage (emit_prefix for emit_bits and emit_dense, the encode_wire
policy's integer); PackBytes hands it to the global bit packer (emit_string:
pack_lds from the stage, enc_slow_tile from the stage or from global memory,
with the batch's frame or the item's).  What differs from path to path is
the sink and the first byte and prefix width its caller passes; a slip there
at one boundary still moves every later byte of its tile.

cases(): for each prefix, payloads of mask - 1, mask, mask + 127, mask + 128,
mask + 16383 and mask + 16384 bytes (headers of 1, 2, 2, 3, 3 and 4 bytes),
each as a string whose Huffman form is one byte shorter than itself (sent
Huffman), exactly as long (the tie: sent raw) and longer (raw); and, on the
5-bit prefix, mask + 2^21 - 1 and mask + 2^21 (4 and 5 bytes).

batches(): one batch per path and prefix -- two ordinary tiles, the fixture
tiles, two ordinary tiles (limits.place) -- built so that limits.classify_enc
puts every fixture tile on the path the batch is named for.  Every fixture
tile comes four times, with 0..3 empty strings (one byte of output each) in
front, and every tile's output is a multiple of four bytes (a raw string of
1..4 bytes, the tuner, sees to it), so each case starts on each byte residue
of an output dword.  tests/test_literal_framing.py checks all of this on the
CPU and runs the batches through every entry point on the GPU.
"""
import collections
import functools
import random

import numpy as np

import _paths  # noqa: F401
import limits as L
import oracle_lib as O
import qpack_frames as Q

PREFIXES = (3, 5, 7)
KINDS = ("shorter", "equal", "longer")
B8 = bytes(L.BY_LEN[8])               # Huffman as long as raw: the tie
SMALL = 4                             # the lengths a staged tile can hold
PADS = (0, 3, 5)                      # bytes in front of the input, added

Case = collections.namedtuple("Case", "p L kind s huff hdr")


def lengths(p):
    """payload lengths on both sides of the prefix and of the length's
    second, third and fourth byte -> [(L, header bytes)]"""
    mask = (1 << p) - 1
    return list(zip((mask - 1, mask, mask + 127, mask + 128, mask + 16383,
                     mask + 16384), (1, 2, 2, 3, 3, 4)))


def big_lengths():
    """the fifth byte, on the 5-bit prefix only: strings of about 2 MB"""
    return [(31 + (1 << 21) - 1, 4), (31 + (1 << 21), 5)]


def _case(p, n, hdr, kind, rng):
    if kind == "shorter":
        return Case(p, n, kind, L.with_bits(n + 1, 8 * n, rng), 1, hdr)
    if kind == "equal":
        return Case(p, n, kind, L.with_bits(n, 8 * n, rng), 0, hdr)
    return Case(p, n, kind, bytes(rng.choice(L.B30) for _ in range(n)), 0, hdr)


@functools.lru_cache(maxsize=None)
def cases():
    """the 54 cases of the first group, in the order (p, L, kind)"""
    rng = random.Random(7541)
    return [_case(p, n, hdr, kind, rng) for p in PREFIXES
            for n, hdr in lengths(p) for kind in KINDS]


def with_bits_np(n, bits, seed):
    """limits.with_bits for a string of megabytes: the same census of code
    lengths (as few 30-bit symbols as it takes, the rest of 5..8 bits, evenly),
    in random order, drawn with numpy"""
    for n30 in range(n + 1):
        m, r = n - n30, bits - 30 * n30
        if 5 * m <= r <= 8 * m:
            break
    else:
        raise ValueError("no %d symbols of %d bits" % (n, bits))
    q, x = divmod(r - 5 * m, m) if m else (0, 0)
    lens = np.concatenate([np.full(x, 6 + q), np.full(m - x, 5 + q),
                           np.full(n30, 30)])
    g = np.random.default_rng(seed)
    g.shuffle(lens)
    out = np.zeros(n, dtype=np.uint8)
    for ln in np.unique(lens):
        at = lens == ln
        out[at] = g.choice(np.array(L.BY_LEN[int(ln)], dtype=np.uint8),
                           int(at.sum()))
    s = out.tobytes()
    assert len(s) == n
    assert int(np.array(L.CODE_LEN, dtype=np.int64)[out].sum()) == bits
    return s


@functools.lru_cache(maxsize=None)
def big_cases():
    """the four 2 MB strings: shorter and equal, as _case() has them"""
    return [Case(5, n, kind, with_bits_np(n + (kind == "shorter"), 8 * n,
                                          n + len(kind)),
                 int(kind == "shorter"), hdr)
            for n, hdr in big_lengths() for kind in ("shorter", "equal")]


def group(p, kind, big):
    """the cases of one prefix and kind: the four lengths a staged tile can
    hold, or the two that pass the stage on their own"""
    cs = [c for c in cases() if c.p == p and c.kind == kind]
    return cs[SMALL:] if big else cs[:SMALL]


def lit_size(p, s):
    """the bytes of s as a literal on a p-bit prefix: Huffman only if
    strictly shorter (lsqpack.c:848)"""
    hb = (L.code_bits(s) + 7) // 8
    n = hb if hb < len(s) else len(s)
    return len(Q.enc_int(0, n, p)) + n


# ---- the paths ----------------------------------------------------------------------
#
# name -> (what frames the literal there, the lengths it can hold, why not the
# others).  classify_enc's fields are in expect() below.

STAGED_ONLY = ("a tile is staged only while its input fits the 3072-byte "
               "stage: payloads of mask + 16383 bytes and more cannot be in "
               "one")
PAST_STAGE = ("a string is a unit of its own only when its input alone "
              "passes the stage: 3073 bytes and more")
PATHS = collections.OrderedDict([
    ("a", ("full kernel, staged, fast, dense: emit_dense (and the wave's "
           "payload copy)", "small", STAGED_ONLY)),
    ("b", ("full kernel, staged, fast, dense stream overflown: emit_bits",
           "small", STAGED_ONLY)),
    ("c", ("full kernel, staged, output 3009..12288: pack_lds, "
           "emit_string<EncLds>", "small", STAGED_ONLY)),
    ("d", ("full kernel, past the stage, in a slot: the cases' unit through "
           "the out stage, the unit behind it packed by lanes", "small",
           "the cases sit in a staged unit: " + STAGED_ONLY)),
    ("e", ("lean kernel, fast: the tiles of a and b", "small", STAGED_ONLY)),
    ("f", ("lean kernel, staged, output above 3008: enc_slow_tile over "
           "EncLds: the tiles of c", "small", STAGED_ONLY)),
    ("g", ("full and lean kernel, the string past the stage and the slot: "
           "a lone unit, enc_slow_tile, emit_string<EncGlb>", "big",
           PAST_STAGE)),
])
# the batches behind each path, and whether the lean model classifies them
BEHIND = {"a": (("a",), False), "b": (("b",), False), "c": (("c",), False),
          "d": (("d",), False), "e": (("a", "b"), True), "f": (("c",), True),
          "g": (("g",), False)}
# the 2 MB strings run on path g at one start residue each: four residues
# would be sixteen strings of 2 MB, for a header the two 16 KB lengths of
# every prefix already take to four bytes at every residue
BIG_NOTE = "g, one start residue each"


def holds(path, p):
    """the payload lengths the path can hold on prefix p"""
    ls = [n for n, _ in lengths(p)]
    return ls[:SMALL] if PATHS[path][1] == "small" else ls[SMALL:]


# ---- tiles -----------------------------------------------------------------------------

def _tokens(rng, n):
    return bytes(rng.choice(L.TOKEN) for _ in range(n))


def _raw(rng, n):
    return bytes(rng.choice(B8) for _ in range(n))


def tile_of(p, lead, body, tail=()):
    """`lead` empty strings, body, the tuner, tail, empty strings up to 64:
    the tuner is a raw string of 1..4 bytes that makes the tile's output a
    multiple of four.  -> 64 strings"""
    rest = L.TS - lead - len(body) - 1 - len(tail)
    assert rest >= 0
    total = lead + rest + sum(lit_size(p, s) for s in list(body) + list(tail))
    t = (-(total + 1)) % 4 or 4
    tile = [b""] * lead + list(body) + [B8[:1] * t] + list(tail) + [b""] * rest
    assert len(tile) == L.TS and sum(lit_size(p, s) for s in tile) % 4 == 0
    return tile


def fixture_tile(path, p, kind, lead, rng):
    """one tile of `path` with the cases of (p, kind) behind `lead` empty
    strings -> (strings, lead, [(lane, case)])"""
    cs = group(p, kind, path == "g")
    body, tail = [c.s for c in cs], []
    at = list(range(lead, lead + len(cs)))
    bits = sum(L.code_bits(s) for s in body)
    nin = sum(len(s) for s in body)
    if path == "a":
        pass
    elif path == "b":
        # 30-bit codes until the span's code bits pass kDenseBits - 64,
        # whatever the 15 bytes in front of the tile add
        tail = [bytes(rng.choice(L.B30)
                      for _ in range(-(-(L.DENSE_MAX + 300 - bits) // 30)))]
    elif path == "c":
        # 3000 bytes of input that go raw (or tie): with a byte of header
        # or more for each of 45 strings the output passes 3008
        each = (3000 - nin) // 40
        body += [_raw(rng, each) for _ in range(40)]
    elif path == "d":
        # the cases' unit ends where a raw string of 2900 bytes does not fit
        # behind it; that string's unit emits more than 3008 bytes
        body += [_tokens(rng, 20) for _ in range(4)]
        tail = [_raw(rng, 2900)] + [_raw(rng, 40) for _ in range(3)]
    else:
        # (the same token strings behind each number of empty ones)
        rng = random.Random(10 * p + KINDS.index(kind))
        body, at = [], []
        for c in cs:
            body += [_tokens(rng, rng.randint(8, 40)) for _ in range(3)]
            at.append(lead + len(body))
            body.append(c.s)
        body += [_tokens(rng, rng.randint(8, 40)) for _ in range(3)]
    tile = tile_of(p, lead, body, tail)
    for lane, c in zip(at, cs):
        assert tile[lane] is c.s
    return tile, lead, list(zip(at, cs))


class Batch:
    """One batch: `strings`, `pad` bytes in front of them in an aligned
    buffer (limits.place, residue 0), `tiles` = [(tile index, lead, [(lane,
    case)])] the fixture tiles; data, off = limits.pack(strings)."""

    def __init__(self, name, path, p, strings, pad, tiles):
        self.name, self.path, self.p = name, path, p
        self.strings, self.pad, self.tiles = strings, pad, tiles
        self.data, self.off = L.pack(strings)

    def __repr__(self):
        return self.name

    @functools.lru_cache(maxsize=None)
    def want(self, mode):
        """the oracle's (bytes, offsets) in `mode`"""
        return O.encode_batch(self.data, self.off, mode)

    def model(self, pad, lean=False, mode=None):
        """classify_enc with `pad` more bytes in front"""
        mode = self.p if mode is None else mode
        pad += self.pad
        sizes = np.diff(self.want(mode)[1].astype(np.int64))
        return L.classify_enc(bytes(pad) + self.data.tobytes(),
                              self.off.astype(np.int64) + pad, 0, mode, sizes,
                              lean=lean)

    def fixture_tiles(self):
        return [ti for ti, _, _ in self.tiles]

    def reached(self):
        """(p, L, kind, the byte residue of the literal's first byte)"""
        oo = self.want(self.p)[1]
        return [(c.p, c.L, c.kind, int(oo[ti * L.TS + lane]) % 4)
                for ti, _, lanes in self.tiles for lane, c in lanes]

    def tile_call(self, ti):
        """one fixture tile as a call of its own -> (data, off)"""
        return L.pack(self.strings[ti * L.TS:(ti + 1) * L.TS])


def _placed(name, path, p, tiles, rng):
    """limits.place around the fixture tiles; the last ordinary string in
    front becomes a raw one of 1..4 bytes that makes the output in front a
    multiple of four: every fixture tile then starts on a dword of the
    output, and a case behind k empty strings k bytes further than without"""
    flat = [s for t, _, _ in tiles for s in t]
    strs, pad, ti = L.place(rng, flat, 0, around=L.token_raw)
    n0 = ti * L.TS
    front = sum(lit_size(p, s) for s in strs[:n0 - 1])
    strs[n0 - 1] = B8[1:2] * ((-(front + 1)) % 4 or 4)
    pad = -sum(len(s) for s in strs[:n0]) % 16
    where = [(ti + j, lead, lanes) for j, (_, lead, lanes) in enumerate(tiles)]
    return Batch(name, path, p, strs, pad, where)


@functools.lru_cache(maxsize=None)
def batches():
    """name -> Batch, one per path that has tiles of its own and prefix"""
    out = collections.OrderedDict()
    for path in ("a", "b", "c", "d", "g"):
        for p in PREFIXES:
            rng = random.Random(100 * ord(path) + p)
            tiles = [fixture_tile(path, p, kind, lead, rng)
                     for kind in KINDS for lead in range(4)]
            name = "%s_p%d" % (path, p)
            out[name] = _placed(name, path, p, tiles, rng)
    return out


@functools.lru_cache(maxsize=None)
def big_batch():
    """the four 2 MB strings in one tile of token strings, mode 5"""
    rng = random.Random(2 << 21)
    body, at = [], []
    for c in big_cases():
        body += [_tokens(rng, rng.randint(8, 40)) for _ in range(3)]
        at.append(len(body))
        body.append(c.s)
    tile = tile_of(5, 0, body)
    return _placed("big_p5", "g", 5, [(tile, 0, list(zip(at, big_cases())))],
                   rng)


def expect(path, info, lanes, lean):
    """what classify_enc must say of a fixture tile of `path` (info: its
    entry; lanes: [(lane, case)]): None, or the words of what is wrong"""
    at = [lane for lane, _ in lanes]
    if lean:
        want = {"a": (True, "fast"), "b": (True, "fast"), "c": (True, "slow"),
                "d": (False, "slow"), "g": (False, "slow")}[path]
        if (info["staged"], info["path"]) != want:
            return "lean: %r, not %r" % ((info["staged"], info["path"]), want)
        return None
    want = {"a": (True, "fast"), "b": (True, "fast"), "c": (True, "slot"),
            "d": (False, "slot"), "g": (False, "slow")}[path]
    if (info["staged"], info["path"]) != want:
        return "%r, not %r" % ((info["staged"], info["path"]), want)
    if path == "a":
        coop = [lane for lane, c in lanes
                if c.kind == "shorter" and 8 * c.L > L.ENC_COOP_BITS]
        if not info["dense"] or info["coop"] != coop:
            return "dense %r, coop %r, not %r" % (info["dense"], info["coop"],
                                                  coop)
    if path == "b" and (info["dense"] or info["coop"]):
        return "dense"
    if path == "d":
        u = info["units"]
        if len(u) < 2 or any(x["lone"] for x in u):
            return "units %r" % (u,)
        if not (u[0]["lo"] == 0 and u[0]["hi"] > max(at) and u[0]["run"] == 0
                and u[0]["out"] + L.OUT_FREE <= L.OUT_CAP):
            return "the cases' unit is not emitted from the out stage"
        if not any(x["out"] + L.OUT_FREE > L.OUT_CAP for x in u[1:]):
            return "no unit packed by lanes"
    if path == "g":
        lone = [x["lo"] for x in info["units"] if x["lone"]]
        if lone != at:
            return "lone units %r, not %r" % (lone, at)
    return None
