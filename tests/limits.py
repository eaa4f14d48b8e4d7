"""Inputs that sit exactly on the limits of the kernels' LDS layouts, and a
plain-Python restatement of the path each 64-string tile takes (no GPU).

Every kernel places per-string data in LDS by worst-case arithmetic -- a
Huffman string of len bytes decodes to at most floor(8 * len / 5) bytes,
reached only by strings made of 5-bit codes -- and chooses its path by exact
comparisons.  The builders here make strings that reach those worst cases
(each asserts its own claim with the oracle); classify() / classify_enc()
say which side of every comparison a tile is on, from the constants of the
headers written out as numbers; DECODE and ENCODE name one tile per edge
and side.
tests/test_limits.py checks the fixtures against the model (CPU) and the
kernels against the oracle on them (GPU); tests/test_path_trace.py checks
the model itself against the kernels' own record of the path each tile took
(trace_expect / trace_expect_enc, coop_expect); the wire, stream and shim tests
take some of the same strings through their entry points.  The resident
service has a cutter and a tile loop of its own: svc_pieces(),
classify_svc() / classify_svc_enc(), SVC_DECODE and SVC_ENCODE, with
tests/test_service_limits.py, which also sends every DECODE and ENCODE tile
through the service.  The header-hash kernel has a stage of its own:
classify_hash() and HASH, at the end, with tests/test_hash_limits.py.
"""
import random

import numpy as np

import _paths  # noqa: F401
import oracle_lib as O
from test_coop_model import coop_model, coop_walks, seg_bits  # noqa: F401

# ---- the headers' constants, as numbers --------------------------------------

TS = 64                       # kWT / kDecTS (qhuff_device.h): strings per tile
STAGE = 3072                  # kStageCap = kDecInCap = kEncInCap (qhuff_pipeline.h)
OUT_CAP = 3072                # kDecStageCap / kEncOutCap: P::kOutCap
OUT_FREE = 64                 # `total + 64 <= kOutCap` (tile_pipeline)
OUT_FAST = 3008               # the largest fast output: kOutCap - 64
BIG_SLOT = 12288              # kBigSlotBytes (qhuff_device.h)
FIX_STRIDE = 108              # kFixStride (qhuff_decode_impl.h)
FIX_MAX = 66                  # kFixMaxLen = 5 * (kFixStride - 1) / 8
STREAM_FIX_MAX = 65           # kStreamFixMaxLen = 5 * (kFixStride - 3) / 8
COOP_MIN = 128                # kCoopMin (qhuff_decode_impl.h)
COOP_MAX_STRINGS = 48         # `popcount(coop) > 48` (codec_range)
VAR_ARENA = 2 * TS + 8 * STAGE // 5 + 16      # kVarArenaBytes = 5059
COPY_MIN = 64                 # `ls > 64` (dec_big_sizes put): copy_out
# (kDenseWords = kStageCap / 4 + 4 = 772, two of them spare: the largest
# dense tile has 24576 code bits, all of a 3072-byte stage at 8 bits a byte)
DENSE_BITS = 32 * (STAGE // 4 + 4 - 2)        # kDenseBits = 24640
DENSE_FREE = 64               # `se + 64 <= kDenseBits` (EncPolicyT::codec_range)
DENSE_MAX = 24576             # the largest dense tile: kDenseBits - 64
ENC_COOP_BITS = 1024          # kEncCoopBits (qhuff_encode_impl.h)

assert FIX_MAX == 5 * (FIX_STRIDE - 1) // 8
assert STREAM_FIX_MAX == 5 * (FIX_STRIDE - 3) // 8
assert OUT_FAST == OUT_CAP - OUT_FREE and DENSE_MAX == DENSE_BITS - DENSE_FREE

# ---- builders --------------------------------------------------------------------

CODE_LEN = [O.code_of(s)[1] for s in range(256)]
F5 = bytes(s for s in range(256) if CODE_LEN[s] == 5)
assert F5 == b"012aceiost"
B30 = bytes(s for s in range(256) if CODE_LEN[s] == 30)
assert B30 == bytes([10, 13, 22])
BY_LEN = {}
for _s in range(256):
    BY_LEN.setdefault(CODE_LEN[_s], []).append(_s)

TOKEN = b"abcdefghijklmnopqrstuvwxyz0123456789-_./:;=, "


def code_bits(s):
    return sum(CODE_LEN[c] for c in s)


def _checked(s, L):
    h = O.huffman_enc(s)
    assert len(h) == L, (len(h), L)
    st, out = O.huff_decode(h)
    assert st == O.OK and out == s
    return h


def maxexp(L, rng):
    """A Huffman string of exactly L bytes that decodes to floor(8 * L / 5)
    bytes, the most any string of L bytes can: random 5-bit symbols.  (5 *
    floor(8L / 5) > 8L - 5, so the padding is at most 4 bits: every L.)"""
    return _checked(bytes(rng.choice(F5) for _ in range(8 * L // 5)), L)


def periodic(L, unit):
    """maxexp(L) with `unit` (5-bit symbols) repeated: every segment of the
    cooperative decode looks alike, so a guessed walk that starts off a
    code boundary never meets the true one."""
    assert unit and all(c in F5 for c in unit)
    n = 8 * L // 5
    return _checked((unit * (n // len(unit) + 1))[:n], L)


def symbols(k, rng):
    """k random 5-bit symbols: ceil(5k / 8) input bytes, k output bytes."""
    return _checked(bytes(rng.choice(F5) for _ in range(k)), (5 * k + 7) // 8)


def invalid_twin(h):
    """h (valid) with its last padding bit cleared -- or, where it has no
    padding, one 0x00 byte appended (five bits of '0' and three zero padding
    bits): rejected by the oracle only after every symbol of h has been
    decoded."""
    st, out = O.huff_decode(h)
    assert st == O.OK
    pad = 8 * len(h) - code_bits(out)
    assert 0 <= pad < 8
    t = h[:-1] + bytes([h[-1] & 0xfe]) if pad else h + b"\x00"
    assert O.huff_decode(t)[0] == O.ERROR
    pre, eos = O.decoded_prefix(t)
    assert not eos and pre == (out if pad else out + b"0")
    return t


def with_bits(n, bits, rng):
    """n bytes whose codes total exactly `bits` bits: as few 30-bit symbols
    as it takes, the rest of 5..8 bits, in random order (the encoder's
    edges are counted in code bits)."""
    for n30 in range(n + 1):
        m, r = n - n30, bits - 30 * n30
        if 5 * m <= r <= 8 * m:
            break
    else:
        raise ValueError("no %d symbols of %d bits" % (n, bits))
    lens = [5] * m
    for i in range(r - 5 * m):
        lens[i % m] += 1
    lens += [30] * n30
    rng.shuffle(lens)
    s = bytes(rng.choice(BY_LEN[x]) for x in lens)
    assert len(s) == n and code_bits(s) == bits
    return s


def token_tiles(rng, tiles=2):
    """ordinary tiles (Huffman strings of 8..40 token characters)"""
    return [O.huffman_enc(bytes(rng.choice(TOKEN)
                                for _ in range(rng.randint(8, 40))))
            for _ in range(TS * tiles)]


def token_raw(rng, tiles=2):
    return [bytes(rng.choice(TOKEN) for _ in range(rng.randint(8, 40)))
            for _ in range(TS * tiles)]


def place(rng, tile, residue, around=token_tiles):
    """two ordinary tiles, `tile`, two ordinary tiles, and the bytes of
    padding in front that put the tile's first byte on `residue` (mod 16)
    of a 16-byte-aligned buffer: (strings, pad_front, index of the tile)"""
    pre, post = around(rng), around(rng)
    pad = (residue - sum(len(s) for s in pre)) % 16
    return pre + list(tile) + post, pad, len(pre) // TS


def pack(strings):
    off = np.zeros(len(strings) + 1, dtype=np.uint32)
    np.cumsum([len(s) for s in strings], out=off[1:])
    return np.frombuffer(b"".join(strings), dtype=np.uint8).copy(), off


# ---- the layout model --------------------------------------------------------------

def _span(res, a, b):
    """16-byte-aligned span of the bytes [a, b) of a buffer at `res` mod 16
    (tile_span, unit_len)"""
    return ((res + b + 15) & ~15) - ((res + a) & ~15)


def _unit(off, sizes, lo, hi, t0):
    """codec_range over the lanes [lo, hi) of the tile at string t0: the
    arena, the cooperative set and the last slot's end"""
    hl = [int(off[t0 + i + 1]) - int(off[t0 + i]) for i in range(lo, hi)]
    fixed = all(x <= FIX_MAX for x in hl)
    A = int(off[t0 + lo])
    coop = [] if fixed else [lo + i for i, x in enumerate(hl) if x > COOP_MIN]
    if len(coop) > COOP_MAX_STRINGS:         # (unreachable: see classify)
        coop = []
    u = {"lo": lo, "hi": hi, "lone": False,
         "arena": "fixed" if fixed else "var", "coop": coop,
         "out": sum(sizes[t0 + lo:t0 + hi])}
    if coop:
        S = seg_bits([hl[i - lo] for i in coop])
        u["S"] = S
        u["segs"] = [max(1, 8 * hl[i - lo] // S) for i in coop]
        assert sum(u["segs"]) <= 64
    # the bytes the last lane may write: its bound and the emitter's two
    last = hi - 1
    if fixed:
        u["slot_end"] = FIX_STRIDE * last + 8 * hl[-1] // 5 + 2
        u["arena_cap"] = FIX_STRIDE * TS
    else:
        u["slot_end"] = (2 * last + 8 * (int(off[t0 + last]) - A) // 5
                         + 8 * hl[-1] // 5 + 2)
        u["arena_cap"] = VAR_ARENA
    return u


def classify(off, base_residue, oracle_sizes, lean=False):
    """The path of every 64-string tile of a decode batch through the full
    kernel (tile_pipeline, DecPolicyT::codec_range, dec_big_sizes): off the
    n + 1 offsets as the kernel gets them, base_residue the data pointer
    mod 16, oracle_sizes the n output sizes (0 for a rejected string).  Per
    tile a dict:

      staged   the 16-byte-aligned span of its input is <= 3072
      units    one entry for a staged tile; for an unstaged one the greedy
               runs of lanes whose aligned span is <= 3072, and a string
               past that alone ("lone": walked in global memory by the
               staged strings' decode_string over the guarded source
               DecGlb, with its bound 8 * len / 5 + 1 and the output
               before it, "run"); each
               with its arena ("fixed": every string <= 66 bytes, "var"),
               its cooperative lanes (> 128 bytes), their segment size S and
               segments, its output bytes and the end of its last slot
               against the arena
      total    output bytes
      path     "fast" (staged, no cooperative string, total <= 3008),
               "slot" (all of it fits the 12288-byte slot as it is
               produced), "slow"
      copy_out the lanes whose bytes leave the arena through copy_out
               (more than 64 of them) rather than the byte loop, in a tile
               that goes to a slot

    A unit holds at most floor(3072 / 129) = 23 strings above kCoopMin, so
    the `popcount(coop) > 48` branch of codec_range cannot be reached while
    kDecInCap is 3072; no fixture is built for it.

    lean: the lean kernel instead (DecPolicyT<..., Full = false>, kBig and
    kCoop off): see _lean()."""
    off = [int(x) for x in off]
    sizes = [int(x) for x in oracle_sizes]
    n = len(off) - 1
    res = base_residue
    tiles = []
    for t0 in range(0, n, TS):
        cnt = min(TS, n - t0)
        o = off[t0:t0 + cnt + 1]
        total = sum(sizes[t0:t0 + cnt])
        info = {"staged": _span(res, o[0], o[cnt]) <= STAGE, "total": total,
                "copy_out": []}
        if info["staged"]:
            u = _unit(off, sizes, 0, cnt, t0)
            info["units"] = [u]
            if not u["coop"] and total <= OUT_FAST:
                info["path"] = "fast"
            else:
                info["path"] = "slot" if total <= BIG_SLOT else "slow"
        else:
            units, run, fits, i0 = [], 0, True, 0
            while i0 < cnt:
                k = sum(1 for i in range(i0, cnt)
                        if _span(res, o[i0], o[i + 1]) <= STAGE)
                if k == 0:
                    bound = 8 * (o[i0 + 1] - o[i0]) // 5 + 1
                    fits = fits and run + bound <= BIG_SLOT
                    units.append({"lo": i0, "hi": i0 + 1, "lone": True,
                                  "bound": bound, "run": run, "coop": [],
                                  "into_slot": fits, "out": sizes[t0 + i0]})
                    run += sizes[t0 + i0]
                    i0 += 1
                    continue
                u = _unit(off, sizes, i0, i0 + k, t0)
                u["run"] = run
                fits = fits and run + u["out"] <= BIG_SLOT
                run += u["out"]
                units.append(u)
                i0 += k
            info["units"] = units
            info["path"] = "slot" if fits else "slow"
        if info["path"] == "slot":
            info["copy_out"] = [i for u in info["units"] if not u["lone"]
                                for i in range(u["lo"], u["hi"])
                                if sizes[t0 + i] > COPY_MIN]
        tiles.append(_lean(info) if lean else info)
    return tiles


def _lean(info):
    """A tile of the full kernels' model as the lean kernels code it
    (tile_pipeline with P::kBig and P::kCoop false): "fast" iff the tile is
    staged and its output <= 3008, otherwise "slow" (P::slow_tile, out of
    line); no slots, no strings for the whole wave.  A staged tile's one
    unit is the codec's call -- its arena, or its dense bit, as in the full
    kernel; an unstaged tile is sized and coded in global memory (decode:
    the same decode_string over DecGlb, tests/test_global_walk.py), no
    unit."""
    t = dict(info)
    t["units"] = []
    if t["staged"]:
        u = {k: v for k, v in info["units"][0].items()
             if k not in ("S", "segs")}
        u["coop"] = []
        t["units"] = [u]
    t["path"] = "fast" if t["staged"] and t["total"] <= OUT_FAST else "slow"
    if "copy_out" in t:
        t["copy_out"] = []
    if "coop" in t:
        t["coop"] = []
    return t


def _enc_unit(raw, off, sizes, res, mode, lo, hi, t0):
    """EncPolicyT::codec_range / emit over the lanes [lo, hi) of the tile at
    string t0 of the buffer raw (at `res` mod 16): se, dense, the output and
    the lanes whose payload the whole wave copies"""
    a, b = off[t0 + lo], off[t0 + hi]
    lead = (res + a) % 16
    se = code_bits(raw[a - lead:b]) if a >= lead else None
    bits = [code_bits(raw[off[t0 + i]:off[t0 + i + 1]])
            for i in range(lo, hi)]
    ln = [off[t0 + i + 1] - off[t0 + i] for i in range(lo, hi)]
    huff = [mode == 0 or (x + 7) // 8 < l for x, l in zip(bits, ln)]
    out = sum(sizes[t0 + lo:t0 + hi])
    dense = se is not None and se <= DENSE_MAX
    emitted = dense and out <= OUT_FAST
    return {"lo": lo, "hi": hi, "lone": False, "se": se, "dense": dense,
            "out": out,
            "coop": [lo + i for i in range(hi - lo)
                     if emitted and huff[i] and sizes[t0 + lo + i]
                     and bits[i] > ENC_COOP_BITS]}


def classify_enc(data, off, base_residue, mode, oracle_sizes, lean=False):
    """The same for an encode batch (EncPolicyT::codec_range / emit,
    enc_big_sizes): data the whole input buffer, off the n + 1 offsets into
    it.  Per tile: staged; se, the code bits of the span's bytes up to the
    tile's end (the dense pass codes the span from its 16-byte boundary, so
    the bytes in front of the tile count), and dense = se <= 24576, whatever
    a string then emits -- a literal that falls back to raw counts its code
    bits all the same; total; path as classify; coop, the lanes whose
    Huffman payload is copied by the whole wave (more than 1024 bits, in a
    dense tile or unit that is emitted from the out stage).  lean: the lean
    kernel instead, see _lean()."""
    off = [int(x) for x in off]
    sizes = [int(x) for x in oracle_sizes]
    raw = bytes(data)
    n = len(off) - 1
    res = base_residue
    tiles = []

    def unit(lo, hi, t0):
        return _enc_unit(raw, off, sizes, res, mode, lo, hi, t0)

    for t0 in range(0, n, TS):
        cnt = min(TS, n - t0)
        o = off[t0:t0 + cnt + 1]
        total = sum(sizes[t0:t0 + cnt])
        info = {"staged": _span(res, o[0], o[cnt]) <= STAGE, "total": total}
        if info["staged"]:
            u = unit(0, cnt, t0)
            info["units"] = [u]
            info["se"], info["dense"] = u["se"], u["dense"]
            if total <= OUT_FAST:
                info["path"] = "fast"
            else:
                info["path"] = "slot" if total <= BIG_SLOT else "slow"
                u["coop"] = []               # (packed by each lane)
            info["coop"] = u["coop"]
        else:
            units, run, fits, i0 = [], 0, True, 0
            while i0 < cnt:
                k = sum(1 for i in range(i0, cnt)
                        if _span(res, o[i0], o[i + 1]) <= STAGE)
                if k == 0:
                    fits = fits and run + sizes[t0 + i0] <= BIG_SLOT
                    units.append({"lo": i0, "hi": i0 + 1, "lone": True,
                                  "run": run, "out": sizes[t0 + i0],
                                  "coop": []})
                    run += sizes[t0 + i0]
                    i0 += 1
                    continue
                u = unit(i0, i0 + k, t0)
                u["run"] = run
                fits = fits and run + u["out"] <= BIG_SLOT
                if not fits:
                    u["coop"] = []           # (sized only: nothing emitted)
                run += u["out"]
                units.append(u)
                i0 += k
            info["units"] = units
            info["path"] = "slot" if fits else "slow"
            info["coop"] = [i for u in units for i in u["coop"]]
        tiles.append(_lean(info) if lean else info)
    return tiles


# ---- the model as a path-trace record ------------------------------------------
#
# A QH_PATH_TRACE build of the library (qhuff_device.h PathTrace) writes, per
# tile, which side of each comparison the kernel took; these give the same
# fields from classify() / classify_enc(), for tests/test_path_trace.py.

TRACE_WORDS = 8               # kTraceWords: u64 words per tile record
TRACE_EXIT = {1: "fast", 2: "slot", 3: "slow"}


def trace_records(words):
    """Codec.profile_read()'s words of a path-trace build as one dict per
    tile (the record's layout: qhuff_device.h PathTrace)"""
    w = np.asarray(words, dtype=np.uint64).reshape(-1, TRACE_WORDS)
    out = []
    for r in w:
        r = [int(x) for x in r]
        out.append({"written": r[0] & 1, "staged": bool(r[0] & 2),
                    "path": TRACE_EXIT.get((r[0] >> 2) & 3),
                    "units": r[1] & 0xffff, "lone": (r[1] >> 16) & 0xffff,
                    "var": (r[1] >> 32) & 0xffff, "dense": r[1] >> 48,
                    "coop": r[2], "fail": r[3],
                    "S": r[4] & 0xffffffff if r[4] >> 63 else None,
                    "rounds": (r[4] >> 32) & 0xffff if r[4] >> 63 else None,
                    "enc_coop": r[5]})
    return out


def _mask(lanes):
    m = 0
    for i in lanes:
        m |= 1 << i
    return m


def coop_expect(strings, info):
    """What the cooperative decode of one decode tile does, by the model:
    strings the tile's Huffman strings, info its classify() entry.  Per unit
    with cooperative lanes coop_walks(h, S) for each of them -> (fail, S,
    rounds): fail the mask of the lanes the model hands back to their own
    lane (None), OR-ed over the units; S and rounds those of the first such
    unit, as the record keeps them (None, None without one).  rounds is the
    largest of the unit's strings' rounds, the rejected ones included: B is
    one loop for the wave, over before W rejects anything."""
    fail, S, rounds = 0, None, None
    for u in info["units"]:
        if not u["coop"]:
            continue
        rs = [coop_walks(strings[i], u["S"]) for i in u["coop"]]
        fail |= _mask(i for i, r in zip(u["coop"], rs) if r[0] is None)
        if S is None:
            S, rounds = u["S"], max(r[1] for r in rs)
    return fail, S, rounds


def trace_expect(strings, info):
    """The record of a decode tile by the model (full or lean entry)"""
    units = [u for u in info["units"] if not u["lone"]]
    fail, S, rounds = coop_expect(strings, info)
    return {"written": 1, "staged": info["staged"], "path": info["path"],
            "units": len(units), "lone": len(info["units"]) - len(units),
            "var": sum(1 for u in units if u["arena"] == "var"),
            "coop": _mask(c for u in units for c in u["coop"]),
            "fail": fail, "S": S, "rounds": rounds}


def trace_expect_enc(info):
    """The record of an encode tile by the model (full or lean entry)"""
    units = [u for u in info["units"] if not u["lone"]]
    return {"written": 1, "staged": info["staged"], "path": info["path"],
            "units": len(units), "lone": len(info["units"]) - len(units),
            "dense": sum(1 for u in units if u["dense"]),
            "enc_coop": _mask(info["coop"])}


# ---- the fixtures ------------------------------------------------------------------

class Fixture:
    """One special tile: `tile` its 64 strings (Huffman strings for decode,
    raw ones for encode), `residues` the alignments (mod 16) of its first
    byte it is run at, `key` the property of its classify() entry it is
    named for and `want` that property's value per residue; `twin` the
    fixture on the other side of the edge; `special` the lanes of the
    strings the fixture is about."""

    def __init__(self, name, tile, key, want, edge, residues=(0, 5),
                 twin=None, special=(), mode=None):
        assert len(tile) == TS
        self.name, self.tile, self.key, self.edge = name, tile, key, edge
        self.want = want if isinstance(want, dict) else {
            r: want for r in residues}
        self.residues, self.twin, self.special = residues, twin, special
        self.mode = mode

    def __repr__(self):
        return self.name


def k_arena(i):
    return i["units"][0]["arena"]


def k_path(i):
    return i["path"]


def k_staged_path(i):
    return (i["staged"], i["path"])


def k_coop(i):
    return tuple(c for u in i["units"] for c in u["coop"])


def k_copy(i):
    return tuple(i["copy_out"])


def k_segs(i):
    return tuple((u.get("S"), tuple(u.get("segs", ()))) for u in i["units"]
                 if u["coop"])


def k_dense(i):
    return i["dense"]


def k_enc_coop(i):
    return tuple(i["coop"])


def _decode_fixtures():
    rng = random.Random(20240)
    fx = []

    def add(*a, **k):
        fx.append(Fixture(*a, **k))

    # hl > kFixMaxLen
    t66 = [maxexp(66, rng) for _ in range(20)] + [maxexp(10, rng)
                                                  for _ in range(44)]
    rng.shuffle(t66)
    sp66 = tuple(i for i, h in enumerate(t66) if len(h) == 66)
    t67 = list(t66)
    t67[sp66[7]] = maxexp(67, rng)
    add("fix66", t66, k_arena, "fixed", "hl > kFixMaxLen, at it: 20 strings "
        "of 66 bytes fill 105 + 2 bytes of their 108-byte stride",
        twin="var67", special=sp66)
    add("var67", t67, k_arena, "var", "hl > kFixMaxLen, past it: one string "
        "of 67 bytes puts the tile in the variable arena", twin="fix66",
        special=sp66)
    # total + 64 <= kOutCap
    t3008 = [symbols(47, rng) for _ in range(64)]
    t3009 = list(t3008)
    t3009[41] = symbols(48, rng)
    add("out3008", t3008, k_path, "fast", "total + 64 <= kOutCap, at it: "
        "output 3008", twin="out3009")
    add("out3009", t3009, k_path, "slot", "total + 64 <= kOutCap, past it: "
        "output 3009 leaves the arena for a big slot", twin="out3008")
    # the variable arena packed to its top
    full = [maxexp(48, rng) for _ in range(62)] + [maxexp(67, rng),
                                                   maxexp(29, rng)]
    add("arena_full", full, k_staged_path,
        {0: (True, "slot"), 5: (False, "slot")},
        "span <= kDecInCap, exactly 3072 at residue 0: the variable arena "
        "packed to its top; at residue 5 the span is 3088 and the tile "
        "splits into units", special=tuple(range(0, 64, 1)))
    # ls > 64
    t64 = [symbols(64 + (i & 1), rng) for i in range(64)]
    add("copy64_65", t64, k_copy, tuple(range(1, 64, 2)),
        "ls > 64 in put: the 64-byte outputs by the byte loop, the 65-byte "
        "ones by copy_out, alternating")
    # hl > kCoopMin
    sh = [maxexp(rng.randint(1, 40), rng) for _ in range(61)]
    c128 = sh[:30] + [maxexp(128, rng), maxexp(127, rng), maxexp(70, rng)] \
        + sh[30:]
    c129 = sh[:30] + [maxexp(128, rng), maxexp(129, rng), maxexp(200, rng)] \
        + sh[30:]
    add("coop128", c128, k_coop, (), "hl > kCoopMin, at it: a string of 128 "
        "bytes is decoded by its lane", twin="coop129", special=(30, 31, 32))
    add("coop129", c129, k_coop, (31, 32), "hl > kCoopMin, past it: 129 and "
        "200 bytes go to the whole wave (200: N == 8 * len / 5 exactly, "
        "bitmap inside a full slot), 128 beside them does not",
        twin="coop128", special=(31, 32, 30))
    # 23 cooperative strings, one segment each
    c23 = [maxexp(129, rng) for _ in range(23)] \
        + [maxexp(3, rng) for _ in range(23)] \
        + [maxexp(2, rng) for _ in range(18)]
    rng.shuffle(c23)
    sp23 = tuple(i for i, h in enumerate(c23) if len(h) == 129)
    add("coop23", c23, k_segs, {0: ((608, (1,) * 23),)},
        "the most cooperative strings a 3072-byte stage holds: 23, S = 608, "
        "one segment each", residues=(0,), special=sp23)
    # 63 segments, >= 60 rounds of B
    for L in (504, 3024):
        for tag, mk in (("ssi", lambda L=L: periodic(L, b"ssi")),
                        ("0", lambda L=L: periodic(L, b"0")),
                        ("rand", lambda L=L: maxexp(L, rng))):
            for lane in (0, 29, 63):
                room = 3072 - 16 - L         # (any residue: one chunk spare)
                sh = [b""] * 63
                for i in rng.sample(range(63), 12):
                    sh[i] = maxexp(min(room // 12, rng.randint(1, 30)), rng)
                tile = sh[:lane] + [mk()] + sh[lane:]
                add("coop63_%d_%s_lane%d" % (L, tag, lane), tile, k_segs,
                    ((8 * L // 63, (63,)),),
                    "one string in 63 segments (8L = 63 S): %s" %
                    ("a periodic one, >= 60 rounds of B" if tag != "rand"
                     else "a random one, <= 4 rounds"),
                    residues=(0, 11), special=(lane,))
    # several round chains in one wave
    for k in (2, 3, 8):
        tile = [b""] * 64
        lanes = sorted(rng.sample(range(64), k))
        for i in lanes:
            tile[i] = periodic(3000 // k, b"ssc")
        rest = [i for i in range(64) if i not in lanes]
        for i in rng.sample(rest, 14):
            tile[i] = maxexp(rng.randint(1, 4), rng)
        add("coop_k%d" % k, tile, k_coop, tuple(lanes),
            "%d equal periodic strings of %d bytes: several round chains in "
            "one wave" % (k, 3000 // k), residues=(0, 3),
            special=tuple(lanes))
    # run + ut <= kBigSlotBytes
    s88 = [symbols(192, rng) for _ in range(64)]
    s89 = list(s88)
    s89[50] = symbols(193, rng)
    add("slot12288", s88, k_staged_path, (False, "slot"),
        "run + ut <= kBigSlotBytes, at it: units whose output totals 12288",
        twin="slot12289", special=tuple(range(64)))
    add("slot12289", s89, k_staged_path, (False, "slow"),
        "run + ut <= kBigSlotBytes, past it: 12289, a slow tile",
        twin="slot12288")
    # run + bound <= kBigSlotBytes, a string walked in global memory
    one = symbols(1, rng)
    g79, g80 = maxexp(7679, rng), maxexp(7680, rng)
    add("glob7679_lane0", [g79, one, one] + [b""] * 61, k_path, "slot",
        "run + bound <= kBigSlotBytes, below it: bound 12287 at run 0, and "
        "the two bytes after it fill the slot", twin="glob7680_lane0",
        special=(0,))
    add("glob7680_lane0", [g80, one, one] + [b""] * 61, k_path, "slow",
        "run + bound <= kBigSlotBytes, past it: bound 12289, counted then "
        "slow", twin="glob7679_lane0", special=(0,))
    add("glob7679_lane63_run1", [b""] * 30 + [one] + [b""] * 32 + [g79],
        k_path, "slot", "run + bound <= kBigSlotBytes, at it: run 1 + "
        "bound 12287", twin="glob7679_lane63_run2", special=(63,))
    add("glob7679_lane63_run2", [one] + [b""] * 29 + [one] + [b""] * 32
        + [g79], k_path, "slow", "run + bound <= kBigSlotBytes, past it: "
        "run 2 + bound 12287", twin="glob7679_lane63_run1", special=(63,))
    byname = {f.name: f for f in fx}
    # a rejected string that decoded all its symbols first
    for name in ("fix66", "arena_full", "coop129", "coop63_504_ssi_lane29",
                 "coop63_3024_0_lane63", "slot12288"):
        f = byname[name]
        tile = list(f.tile)
        for i in f.special[::3]:
            tile[i] = invalid_twin(tile[i])
        add(name + "_invalid", tile, None, None, "every third special "
            "string of %s replaced by its invalid twin: status 1, size 0, "
            "neighbours untouched" % name, residues=f.residues[:1],
            special=f.special[::3])
    return fx


def _encode_fixtures():
    rng = random.Random(20241)
    fx = []

    def add(*a, **k):
        fx.append(Fixture(*a, **k))

    def b30(n):
        return bytes(rng.choice(B30) for _ in range(n))
    t8 = [b30(12 + (i & 1)) for i in range(64)]
    t9 = list(t8)
    t9[20] = t9[20] + bytes([rng.choice(F5)])
    add("enc_out3008", t8, k_path, "fast", "total + 64 <= kOutCap, at it: "
        "30-bit codes, 3.75x expansion to 3008 bytes", twin="enc_out3009",
        residues=(0,), mode=0)
    add("enc_out3009", t9, k_path, "slot", "total + 64 <= kOutCap, past it: "
        "3009 bytes", twin="enc_out3008", residues=(0,), mode=0)
    # se + 64 <= kDenseBits.  40-byte strings of 384 code bits: 48 bytes of
    # Huffman each, so mode 0 emits 3072 bytes (a big slot) and mode 7 falls
    # back to raw for every string (41 bytes each, a fast tile) -- and codec()
    # takes se from the dense offsets before it knows what a string emits,
    # so the raw strings' codes count: the edge sits inside a fast tile.
    d76 = [with_bits(40, 384, rng) for _ in range(64)]
    d77 = d76[:63] + [with_bits(40, 385, rng)]
    d12 = d76[:63] + [with_bits(40, 384 - 64, rng)]
    d13 = d76[:63] + [with_bits(40, 385 - 64, rng)]
    for mode, path in ((0, "slot"), (7, "fast")):
        add("enc_dense24576_mode%d" % mode, d76, k_dense, True,
            "se + 64 <= kDenseBits, at it: 24576 code bits (%s tile)" % path,
            twin="enc_dense24577_mode%d" % mode, residues=(0,), mode=mode)
        add("enc_dense24577_mode%d" % mode, d77, k_dense, False,
            "se + 64 <= kDenseBits, past it: 24577 code bits, sized and "
            "emitted per string", twin="enc_dense24576_mode%d" % mode,
            residues=(0,), mode=mode)
        # 24512 + 64 is the stage in bits, 64 below the dense stream's limit
        add("enc_dense24512_mode%d" % mode, d12, k_dense, True,
            "24512 code bits: dense", residues=(0,), mode=mode)
        add("enc_dense24513_mode%d" % mode, d13, k_dense, True,
            "24513 code bits: dense", residues=(0,), mode=mode)
    # bits > kEncCoopBits
    short = [bytes(rng.choice(TOKEN) for _ in range(rng.randint(0, 30)))
             for _ in range(62)]
    p1024 = with_bits(204, 1024, rng)
    assert sorted(CODE_LEN[c] for c in p1024) == [5] * 200 + [6] * 4
    p1025 = bytes(rng.choice(F5) for _ in range(205))
    add("enc_coop1024_1025", short[:17] + [p1024] + short[17:40] + [p1025]
        + short[40:], k_enc_coop, (41,), "bits > kEncCoopBits: the payload "
        "of 1024 bits by its lane, the one of 1025 by the wave",
        residues=(0, 5), mode=0, special=(17, 41))
    # big slot against slow tile
    s88 = [with_bits(60, 1536, rng) for _ in range(64)]
    s89 = s88[:33] + [with_bits(60, 1537, rng)] + s88[34:]
    add("enc_slot12288", s88, k_staged_path, (False, "slot"),
        "run + ut <= kBigSlotBytes, at it: units packing 12288 bytes",
        twin="enc_slot12289", residues=(0, 5), mode=0)
    add("enc_slot12289", s89, k_staged_path, (False, "slow"),
        "run + ut <= kBigSlotBytes, past it: 12289", twin="enc_slot12288",
        residues=(0, 5), mode=0)
    return fx


DECODE = _decode_fixtures()
ENCODE = _encode_fixtures()
DECODE_BY_NAME = {f.name: f for f in DECODE}
ENCODE_BY_NAME = {f.name: f for f in ENCODE}


def decode_batch_of(f, residue):
    """(data, off, pad_front, tile index) of fixture f between ordinary
    tiles: with pad_front bytes in front of data in a 16-byte-aligned
    buffer (and added to off) the tile's first byte is at `residue`"""
    rng = random.Random(len(f.name) * 131 + residue)
    strs, pad, ti = place(rng, f.tile, residue)
    data, off = pack(strs)
    assert (int(off[ti * TS]) + pad) % 16 == residue
    return data, off, pad, ti


def encode_batch_of(f, residue):
    rng = random.Random(len(f.name) * 137 + residue)
    strs, pad, ti = place(rng, f.tile, residue, around=token_raw)
    data, off = pack(strs)
    assert (int(off[ti * TS]) + pad) % 16 == residue
    return data, off, pad, ti


def combined(fixtures, raw=False, repeat=1):
    """Every fixture at every one of its residues in one batch, two ordinary
    tiles in front of each (the last ordinary string lengthened to put the
    fixture's first byte on its residue) and two at the end: a batch of a
    few hundred tiles, for a grid of fewer waves than that -- every wave
    then codes several tiles and a fixture's tile is coded between pending
    ones (repeat: the whole list that many times over).  -> (data, off,
    [(fixture, residue, tile index)]); the buffer is 16-byte aligned and
    off[0] is 0."""
    rng = random.Random(len(fixtures))
    around = token_raw if raw else token_tiles
    strs, where, pos = [], [], 0
    for f in list(fixtures) * repeat:
        if raw and f.mode != 0:
            continue
        for r in f.residues:
            pre = around(rng)
            pos += sum(len(s) for s in pre)
            p = (r - pos) % 16
            n = len(pre[-1]) + p
            pre[-1] = bytes(rng.choice(TOKEN) for _ in range(n)) if raw \
                else maxexp(n, rng)
            pos += p
            assert pos % 16 == r and len(strs) % TS == 0
            where.append((f, r, (len(strs) + len(pre)) // TS))
            strs += pre + list(f.tile)
            pos += sum(len(s) for s in f.tile)
    strs += around(rng)
    data, off = pack(strs)
    return data, off, where


# ---- the resident service (qhuff_service.hip, qhuff_svc_host.cpp) ------------------
#
# The service runs the same policies behind a host cutter (svc_call) and in a
# tile loop of its own (serve_tiles): svc_pieces() is the cutter,
# classify_svc() / classify_svc_enc() the path of every piece, SVC_DECODE and
# SVC_ENCODE whole calls that sit on the cutter's, the kernel's and copy2's
# comparisons (tests/test_service_limits.py).

SVC_MAX_STRINGS = 1024        # QHUFF_SVC_MAX_STRINGS = kSvcMaxStrings
SVC_MAX_BYTES = 65536         # QHUFF_SVC_MAX_BYTES = kSvcInCap
SVC_SLOTS = 12                # slots of a default service: one workgroup's waves
COPY_PASS = 512               # copy2: 64 lanes x 8 chunks of 16 bytes a pass
assert STAGE == 3072          # kSvcTileBytes == kStageCap (static_assert)


def svc_pieces(off):
    """svc_call's cutter (qhuff_svc_host.cpp, svc_piece_end), transcribed:
    the string indices [0, ..., n] at which a call of these n + 1 offsets is
    cut -- a piece takes strings while it has fewer than 64 and the next one
    keeps it within 3072 bytes, its first string whatever its length; None
    for a call that takes the context's host path (svc_fits)."""
    off = [int(x) for x in off]
    n = len(off) - 1
    if n > SVC_MAX_STRINGS or off[n] - off[0] > SVC_MAX_BYTES:
        return None
    cuts, s0 = [0], 0
    while s0 < n:
        s1 = s0 + 1
        while s1 < n and s1 - s0 < TS and off[s1 + 1] - off[s0] <= STAGE:
            s1 += 1
        cuts.append(s1)
        s0 = s1
    return cuts


def _svc_piece(n, nb, total):
    """what the two models share: the route (the kernel's `one`) and, for a
    scratch piece, copy2's chunks and passes"""
    p = {"n": n, "bytes": nb, "total": total,
         "route": "direct" if n <= TS and nb <= STAGE else "scratch"}
    if p["route"] == "scratch":
        assert n == 1                        # the cutter leaves it alone
        p["staged"], p["path"] = False, "slow"
        p["copy_in"] = (4 * (n + 1) + 15) // 16 + (nb + 15) // 16
        p["copy_out"] = (total + 15) // 16
        p["passes_in"] = -(-p["copy_in"] // COPY_PASS)
        p["passes_out"] = -(-p["copy_out"] // COPY_PASS)
    else:
        p["staged"] = True
        p["path"] = "fast" if total <= OUT_FAST else "slow"
    return p


def classify_svc(off, oracle_sizes):
    """The path of every piece of a decode call through the service
    (svc_call, qhuff_service_kernel, serve_tiles): one dict per piece, or
    None for a call that takes the host path.  What differs from classify():

      * the residue is always 0: a piece's offsets are rebased to 0 and the
        slot's regions are 256-aligned, so the span is the piece's bytes;
      * a piece of at most 64 strings and 3072 bytes ("route": "direct") is
        one tile coded straight from its slot, and always staged;
      * there is no big slot, and the cooperative phase runs in the tile
        loop itself: "path" is "fast" iff total <= 3008, cooperative
        strings or not (DecPolicyT::emit copies them out of the arena with
        the whole wave), else "slow": dec_slow_tile from the staged arena
        into the slot;
      * any other piece ("scratch") is one string of more than 3072 bytes,
        copied to device scratch, sized and decoded there by its lane from
        global memory, and copied back: copy2 moves 1 + ceil(bytes / 16)
        chunks in (copy_in) and, after the chunk of offsets and the one of
        the status, ceil(total / 16) chunks out (copy_out), 512 chunks a
        pass (passes_in, passes_out).

    Per piece: n, bytes, total, route, staged, path; a direct piece also has
    _unit's arena, coop lanes, S, segs, slot_end and arena_cap."""
    cuts = svc_pieces(off)
    if cuts is None:
        return None
    sizes = [int(x) for x in oracle_sizes]
    pieces = []
    for s0, s1 in zip(cuts, cuts[1:]):
        o = [int(off[i]) - int(off[s0]) for i in range(s0, s1 + 1)]
        p = _svc_piece(s1 - s0, o[-1], sum(sizes[s0:s1]))
        p.update(arena=None, coop=(), S=None, segs=())
        if p["route"] == "direct":
            u = _unit(o, sizes[s0:s1], 0, s1 - s0, 0)
            p.update(arena=u["arena"], coop=tuple(u["coop"]), S=u.get("S"),
                     segs=tuple(u.get("segs", ())), slot_end=u["slot_end"],
                     arena_cap=u["arena_cap"])
        pieces.append(p)
    return pieces


def classify_svc_enc(data, off, mode, oracle_sizes):
    """The same for an encode call; what differs from classify_enc():

      * residue 0, so se is the code bits of the piece's own bytes;
      * a direct piece is always staged and dense-passed; "path" is "fast"
        iff total <= 3008, else "slow": enc_slow_tile packs each lane's
        string from the stage into the slot (no big slot);
      * the wave copies a payload ("coop") only in a dense tile that is
        emitted fast;
      * a scratch piece is one string, sized and packed by its lane in
        device memory (se None, not dense), with copy2's chunks as in
        classify_svc.

    Per piece: n, bytes, total, route, staged, path, se, dense, coop."""
    cuts = svc_pieces(off)
    if cuts is None:
        return None
    sizes = [int(x) for x in oracle_sizes]
    raw = bytes(data)
    pieces = []
    for s0, s1 in zip(cuts, cuts[1:]):
        a = int(off[s0])
        o = [int(off[i]) - a for i in range(s0, s1 + 1)]
        p = _svc_piece(s1 - s0, o[-1], sum(sizes[s0:s1]))
        p.update(se=None, dense=False, coop=())
        if p["route"] == "direct":
            u = _enc_unit(raw[a:a + o[-1]], o, sizes[s0:s1], 0, mode, 0,
                          s1 - s0, 0)
            p.update(se=u["se"], dense=u["dense"], coop=tuple(u["coop"]))
        pieces.append(p)
    return pieces


def token_huff(L, rng):
    """the Huffman string, of exactly L bytes with 1..7 bits of padding, of
    random token text (codes of 5..8 bits: a sum that grows by at most 8
    cannot jump the 8 values that give L bytes)"""
    s, bits = [], 0
    while True:
        while bits <= 8 * L - 8:
            s.append(rng.choice(TOKEN))
            bits += CODE_LEN[s[-1]]
        if bits < 8 * L:
            return _checked(bytes(s), L)
        bits -= CODE_LEN[s.pop()]


def padded5(L, rng, unit=None):
    """L bytes of 5-bit codes with 1..5 bits of padding: maxexp(L) -- or
    periodic(L, unit) -- with one symbol fewer where 8 L is a multiple of 5,
    so that its invalid twin has L bytes too"""
    n = (8 * L - 1) // 5
    s = (unit * (n // len(unit) + 1))[:n] if unit else \
        bytes(rng.choice(F5) for _ in range(n))
    return _checked(s, L)


def invalid_same_len(h):
    """invalid_twin(h) for a string with padding, without that function's
    bit-by-bit walk (strings of 64 KB): the last padding bit cleared, so
    the string is rejected only at its very end"""
    st, out = O.huff_decode(h)
    assert st == O.OK and 1 <= 8 * len(h) - code_bits(out) < 8
    t = h[:-1] + bytes([h[-1] & 0xfe])
    assert O.huff_decode(t)[0] == O.ERROR and t[:-1] == h[:-1]
    return t


class SvcFixture:
    """One service call: `strings` (Huffman strings for decode, raw ones for
    encode in `mode`), `want` one dict per piece of the items its
    classify_svc() / classify_svc_enc() entry must have, `bad` the strings
    the oracle rejects, `edge` the comparison it sits on and `twin` the
    fixture on the other side."""

    def __init__(self, name, strings, want, edge, twin=None, mode=None,
                 bad=0):
        self.name, self.strings, self.want, self.edge = name, strings, want, edge
        self.twin, self.mode, self.bad = twin, mode, bad
        assert len(strings) <= SVC_MAX_STRINGS
        assert sum(len(s) for s in strings) <= SVC_MAX_BYTES

    def __repr__(self):
        return self.name


# input sizes of one string on the scratch route, in pairs across an edge:
# the kernel's nb <= kStageCap (3072 | 3073), a whole last chunk or one byte
# in the next (3088 | 3089), copy2's pass of 512 chunks counting the chunk of
# offsets (511 chunks of input | 512, and 1023 | 1024), the slot's last byte
SCRATCH_SIZES = (3073, 3088, 3089, 8176, 8177, 16368, 16369, 65535, 65536)
SCRATCH_PASSES_IN = {3073: 1, 3088: 1, 3089: 1, 8176: 1, 8177: 2, 16368: 2,
                     16369: 3, 65535: 9, 65536: 9}
SCRATCH_TWIN = {3073: 3072, 3088: 3089, 3089: 3088, 8176: 8177, 8177: 8176,
                16368: 16369, 16369: 16368, 65535: 65536, 65536: 65535}


def _svc_name(size, tag):
    return ("svc_one%d_%s" if size in (3072, 3073) else "svc_scr%d_%s") % (
        size, tag)


def _svc_decode_fixtures():
    rng = random.Random(20243)
    fx = []

    def add(*a, **k):
        fx.append(SvcFixture(*a, **k))

    # total + 64 <= kOutCap with a cooperative string in the tile
    ks = [45] * 28 + [44] * 35
    rng.shuffle(ks)
    t8 = [symbols(k, rng) for k in ks]
    t8.insert(17, symbols(208, rng))
    t9 = list(t8)
    t9[40] = symbols(ks[39] + 1, rng)
    assert len(t8[17]) == 130 and sum(len(s) for s in t9) < 2048
    add("svc_coop_out3008", t8, [{"n": 64, "route": "direct", "path": "fast",
                                  "total": 3008, "coop": (17,)}],
        "total + 64 <= kOutCap in serve_tiles, at it, with a string of 130 "
        "bytes: emitted fast, the cooperative string copied out of the "
        "arena by DecPolicyT::emit", twin="svc_coop_out3009")
    add("svc_coop_out3009", t9, [{"n": 64, "route": "direct", "path": "slow",
                                  "total": 3009, "coop": (17,)}],
        "the same, past it: 3009 bytes from the staged arena by "
        "dec_slow_tile", twin="svc_coop_out3008")
    # in_off[s1 + 1] - in_off[s0] <= kSvcTileBytes: strings of 64 bytes that
    # decode to 60 (two 30-bit codes each), so the first piece is a fast one
    s64 = [_checked(with_bits(60, 512, rng), 64) for _ in range(48)]
    s65 = _checked(with_bits(61, 520, rng), 65)
    tail = symbols(16, rng)
    add("svc_cut3072", s64 + [tail],
        [{"n": 48, "bytes": 3072, "route": "direct", "path": "fast"},
         {"n": 1, "bytes": 10}],
        "<= kSvcTileBytes, at it: 48 strings reach 3072 bytes, the next one "
        "opens a piece", twin="svc_cut3073")
    add("svc_cut3073", s64[:47] + [s65, tail],
        [{"n": 47, "bytes": 3008}, {"n": 2, "bytes": 75}],
        "<= kSvcTileBytes, past it: the 48th string would make 3073 bytes "
        "and opens the second piece", twin="svc_cut3072")
    # s1 - s0 < kWT
    short = [symbols(rng.randint(8, 40), rng) for _ in range(65)]
    add("svc_count65", short, [{"n": 64, "path": "fast"}, {"n": 1}],
        "s1 - s0 < kWT: 65 short strings are cut (64, 1)")
    add("svc_empty64_one", [b""] * 64 + [short[0]],
        [{"n": 64, "bytes": 0, "total": 0, "path": "fast"}, {"n": 1}],
        "s1 - s0 < kWT with no bytes at all: 64 empty strings are a piece "
        "of zero bytes")
    add("svc_3072_empties", [padded5(3072, rng)] + [b""] * 70,
        [{"n": 64, "bytes": 3072, "route": "direct", "path": "slow",
          "coop": (0,)}, {"n": 7, "bytes": 0, "total": 0}],
        "both cuts: empty strings join a full 3072-byte piece until it has "
        "64 strings, the other 7 are a piece of zero bytes")
    add("svc_all_empty", [b""] * 70,
        [{"n": 64, "bytes": 0}, {"n": 6, "bytes": 0}],
        "a call of empty strings only: two pieces of zero bytes")
    # nb <= kStageCap, and the scratch route's sizes
    makers = (("maxexp", lambda L: padded5(L, rng)),
              ("ssi", lambda L: padded5(L, rng, b"ssi")),
              ("token", lambda L: token_huff(L, rng)))
    for size in (3072,) + SCRATCH_SIZES:
        for tag, mk in makers:
            h = mk(size)
            if size == 3072:
                want = {"n": 1, "bytes": 3072, "route": "direct",
                        "path": "slow", "coop": (0,)}
                edge = "nb <= kStageCap, at it: one string of 3072 bytes, " \
                       "staged and decoded by the whole wave"
                twin = 3073
            else:
                want = {"n": 1, "bytes": size, "route": "scratch",
                        "path": "slow", "copy_in": 1 + (size + 15) // 16,
                        "passes_in": SCRATCH_PASSES_IN[size]}
                edge = "one string of %d bytes through the scratch: %d " \
                       "chunks in, %d pass(es) of copy2" % (
                           size, want["copy_in"], want["passes_in"])
                twin = SCRATCH_TWIN[size]
            add(_svc_name(size, tag), [h], [want], edge,
                twin=_svc_name(twin, tag))
            # (3072: the whole wave finds the error, the lane decodes the
            # string again and the tile, of no bytes, is emitted fast)
            bad = dict(want, total=0)
            if size == 3072:
                bad.update(path="fast")
            else:
                bad.update(copy_out=0, passes_out=0)
            add(_svc_name(size, tag) + "_invalid", [invalid_same_len(h)],
                [bad], "the same string rejected at its very end: status 1, "
                "no output" + ("" if size == 3072 else ", nothing copied "
                               "back"), bad=1)
    # copy2's pass on the way back
    for k, twin in ((8192, 8193), (8193, 8192)):
        add("svc_back%d" % k, [symbols(k, rng)],
            [{"n": 1, "route": "scratch", "total": k,
              "copy_out": (k + 15) // 16, "passes_out": 1 + (k > 8192)}],
            "copy2's pass of 512 chunks on the way back: %d bytes out, "
            "%d chunks" % (k, (k + 15) // 16), twin="svc_back%d" % twin)
    return fx


def _svc_encode_fixtures():
    rng = random.Random(20244)
    fx = []

    def add(*a, **k):
        k.setdefault("mode", 0)
        fx.append(SvcFixture(*a, **k))

    def tok(n):
        return bytes(rng.choice(TOKEN) for _ in range(n))

    s64 = [tok(64) for _ in range(48)]
    add("svc_enc_cut3072", s64 + [tok(10)],
        [{"n": 48, "bytes": 3072, "route": "direct", "path": "fast",
          "dense": True}, {"n": 1, "bytes": 10}],
        "<= kSvcTileBytes, at it: 48 strings reach 3072 bytes",
        twin="svc_enc_cut3073")
    add("svc_enc_cut3073", s64[:47] + [tok(65), tok(10)],
        [{"n": 47, "bytes": 3008}, {"n": 2, "bytes": 75}],
        "<= kSvcTileBytes, past it: the 48th string opens the second piece",
        twin="svc_enc_cut3072")
    short = [tok(rng.randint(8, 40)) for _ in range(65)]
    add("svc_enc_count65", short, [{"n": 64, "path": "fast"}, {"n": 1}],
        "s1 - s0 < kWT: 65 short strings are cut (64, 1)")
    add("svc_enc_empty64_one", [b""] * 64 + [short[0]],
        [{"n": 64, "bytes": 0, "se": 0, "path": "fast"}, {"n": 1}],
        "64 empty strings are a piece of zero bytes")
    add("svc_enc_3072_empties", [tok(3072)] + [b""] * 70,
        [{"n": 64, "bytes": 3072, "route": "direct", "path": "fast",
          "dense": True, "coop": (0,)}, {"n": 7, "bytes": 0}],
        "both cuts: empty strings join a full piece until it has 64 strings, "
        "the other 7 are a piece of zero bytes")
    add("svc_enc_all_empty", [b""] * 70,
        [{"n": 64, "bytes": 0}, {"n": 6, "bytes": 0}],
        "a call of empty strings only")
    makers = (("token", tok),
              ("f5", lambda n: bytes(rng.choice(F5) for _ in range(n))),
              ("b30", lambda n: bytes(rng.choice(B30) for _ in range(n))))
    for size in (3072,) + SCRATCH_SIZES:
        for tag, mk in makers:
            if size == 3072:
                # 3072 bytes of 30-bit codes are 92160 code bits: not dense,
                # 11520 bytes packed by the lane from the stage
                want = {"n": 1, "bytes": 3072, "route": "direct",
                        "dense": tag != "b30",
                        "path": "slow" if tag == "b30" else "fast",
                        "coop": () if tag == "b30" else (0,)}
                edge = "nb <= kStageCap, at it: one string of 3072 bytes, " \
                       "staged"
                twin = 3073
            else:
                want = {"n": 1, "bytes": size, "route": "scratch",
                        "path": "slow", "dense": False,
                        "copy_in": 1 + (size + 15) // 16,
                        "passes_in": SCRATCH_PASSES_IN[size]}
                edge = "one string of %d bytes through the scratch: %d " \
                       "chunks in, %d pass(es) of copy2" % (
                           size, want["copy_in"], want["passes_in"])
                twin = SCRATCH_TWIN[size]
            if tag == "b30":
                want["total"] = (30 * size + 7) // 8
            add(_svc_name(size, "enc_" + tag), [mk(size)], [want], edge,
                twin=_svc_name(twin, "enc_" + tag))
    for k, n, twin in ((8192, 13107, 8193), (8193, 13108, 8192)):
        add("svc_enc_back%d" % k, [bytes(rng.choice(F5) for _ in range(n))],
            [{"n": 1, "route": "scratch", "total": k,
              "copy_out": (k + 15) // 16, "passes_out": 1 + (k > 8192)}],
            "copy2's pass of 512 chunks on the way back: %d 5-bit codes, %d "
            "bytes out" % (n, k), twin="svc_enc_back%d" % twin)
    return fx


SVC_DECODE = _svc_decode_fixtures()
SVC_ENCODE = _svc_encode_fixtures()
SVC_DECODE_BY_NAME = {f.name: f for f in SVC_DECODE}
SVC_ENCODE_BY_NAME = {f.name: f for f in SVC_ENCODE}
assert len(SVC_DECODE_BY_NAME) == len(SVC_DECODE)
assert len(SVC_ENCODE_BY_NAME) == len(SVC_ENCODE)


# ---- the header-hash kernel (qhuff_hash.hip) ---------------------------------------
#
# The hash kernel has a stage of its own (kHashCap) and one comparison: a
# tile whose 16-byte-aligned span fits the stage is copied to LDS and hashed
# there (HashLds: dword reads that depend on the address mod 4, the last
# stripe and word of a full stage reaching into the slack words), any other
# is hashed from global memory by byte loads (HashGlb).  A tile is 64 strings
# (qhuff_xxh32_batch) or 64 headers, 128 strings (qhuff_xxh32_headers).

HASH_STAGE = 6144             # kHashCap = 64 * kHashNch * 16 (qhuff_hash.hip)
HASH_NCH = 6                  # kHashNch: 16-byte chunks per lane
HASH_SLACK_WORDS = 8          # HashWave::s: words past the stage

assert HASH_STAGE == TS * HASH_NCH * 16


def classify_hash(off, base_residue, pairs):
    """Per tile of a hash batch -- 64 headers (pairs: off has 2n + 1
    entries) or 64 strings (n + 1) -- as the kernel gets them, base_residue
    the data pointer mod 16: span (tile_span's 16-byte-aligned bytes), n16
    (its 16-byte chunks), staged (span <= 6144) and cnt (headers or strings
    in the tile)."""
    off = [int(x) for x in off]
    k = 2 if pairs else 1
    assert (len(off) - 1) % k == 0
    n = (len(off) - 1) // k
    tiles = []
    for t0 in range(0, n, TS):
        cnt = min(TS, n - t0)
        span = _span(base_residue, off[k * t0], off[k * (t0 + cnt)])
        tiles.append({"span": span, "n16": span // 16,
                      "staged": span <= HASH_STAGE, "cnt": cnt})
    return tiles


LAYOUTS = ("pairs", "single")
# the last-string lengths of hash_stage6144: the stripe's s[q + 4] (16, 32:
# the last stripe ends the stage), the word tail's s[q + 1] (20: stripe then
# word; 35: two stripes, then a byte tail only), the byte tail at the
# stage's end (17, 19, 31).  A string that ends on the stage's last byte
# starts at -len mod 4, so these give start & 3 in {0, 3, 1}; 18 and 34 are
# added for start & 3 == 2.
STAGE_LAST_LENS = (16, 17, 18, 19, 20, 31, 32, 34, 35)
LONG_LENS = (6145, 70001)
FILLER = 6200                 # one string that alone passes the stage


class HashFixture:
    """A run of whole tiles for the hash kernel (most fixtures: one tile).
    strings[variant] is the run's strings for a layout variant ("single":
    64 per tile; "pairs", "pairs_name", "pairs_value": 128 per tile, name
    and value alternating); residues the alignments of the run's first byte;
    want[r] whether its tiles are staged at residue r (one bool for all of
    them), spans[r] the exact span of its first tile where the fixture
    names one; last: the run ends in a partial tile and must end the
    batch."""

    def __init__(self, name, strings, want, edge, spans=None, twin=None,
                 last=False):
        self.name, self.strings, self.want, self.edge = name, strings, want, edge
        self.residues = tuple(want)
        self.spans, self.twin, self.last = spans or {}, twin, last

    def variants(self):
        return tuple(self.strings)

    def __repr__(self):
        return self.name


def is_pairs(variant):
    return variant != "single"


def _rb(rng, n):
    return rng.randbytes(n)


def _split(rng, total, k):
    """k lengths >= 0 that sum to total (some of them 0)"""
    cuts = sorted(rng.randint(0, total) for _ in range(k - 1))
    return [b - a for a, b in zip([0] + cuts, cuts + [total])]


def hash_ordinary(rng, pairs, tiles=2):
    """ordinary tiles for the hash kernel: random bytes, 8..40 a string
    (at most 128 * 40 = 5120 bytes a tile: staged at any residue)"""
    return [_rb(rng, rng.randint(8, 40))
            for _ in range(TS * tiles * (2 if pairs else 1))]


def lengths_run(rng, pairs, filler):
    """Strings of every length 0..96 starting on every residue 0..15 (of a
    run whose first byte is on residue 0), one after the other with no gap:
    where no missing (length, residue) starts at the current residue, a
    string of the set is repeated.  pairs: every (length, residue) once as
    a name and once as a value.  Without filler every tile stays below the
    stage (a string that would take it past ~6000 bytes waits, an empty one
    takes its place); with filler every tile holds one string of FILLER
    bytes, on a lane that moves from tile to tile.  The last tile is filled
    up with repeats."""
    roles = 2 if pairs else 1
    per = TS * roles
    need = {(p, r): set(range(97)) for p in range(roles) for r in range(16)}
    left = 97 * 16 * roles
    out, pos, tile_bytes = [], 0, 0
    while left or len(out) % per:
        i = len(out) % per
        if i == 0:
            tile_bytes = 0
        if filler and i == (7 * (len(out) // per) + 3) % per:
            out.append(_rb(rng, FILLER))
            pos += FILLER
            continue
        room = 96 if filler else min(96, 6000 - tile_bytes)
        p, r = len(out) % roles, pos % 16
        # the next string's role and residue after a string of length l
        def after(l):
            return len(need[((p + 1) % roles, (r + l) % 16)])
        cand = [l for l in need[(p, r)] if l <= room]
        if cand:
            best = max(after(l) for l in cand)
            l = rng.choice([l for l in cand if after(l) == best])
            need[(p, r)].discard(l)
            left -= 1
        elif room >= 16:
            best = max(after(l) for l in range(1, 17))
            l = rng.choice([l for l in range(1, 17) if after(l) == best])
        else:
            l = 0
        out.append(_rb(rng, l))
        pos += l
        tile_bytes += l
    return out


def _hash_fixtures():
    rng = random.Random(20242)
    fx = []

    def add(*a, **k):
        fx.append(HashFixture(*a, **k))

    def both(make):
        return {v: make(is_pairs(v)) for v in LAYOUTS}

    def cnt_of(pairs):
        return TS * (2 if pairs else 1)

    # span <= kHashCap: exactly 6144 bytes, the last string ending the stage
    for ll in STAGE_LAST_LENS:
        s = both(lambda pairs: [_rb(rng, n) for n in
                                _split(rng, HASH_STAGE - ll, cnt_of(pairs) - 1)]
                 + [_rb(rng, ll)])
        add("hash_stage6144_len%d" % ll, s, {0: True},
            "span <= kHashCap, at it: 6144 bytes at residue 0, n16 = 384, "
            "the last string (%d bytes, start & 3 = %d) ends on the stage's "
            "last byte" % (ll, -ll & 3), spans={0: HASH_STAGE},
            twin="hash_stage6160_len%d" % ll)
        add("hash_stage6160_len%d" % ll, s, {5: False},
            "span <= kHashCap, past it: the same tile at residue 5, span "
            "6160, hashed from global memory", spans={5: HASH_STAGE + 16},
            twin="hash_stage6144_len%d" % ll)
    # the largest skew on both sides of the edge
    s = both(lambda pairs: [_rb(rng, n) for n in
                            _split(rng, HASH_STAGE - 15 - 21,
                                   cnt_of(pairs) - 1)] + [_rb(rng, 21)])
    add("hash_stage_res15", s, {15: True}, "first byte at residue 15, last "
        "byte the stage's last: skew 15, span 6144", spans={15: HASH_STAGE},
        twin="hash_stage_res15_over")
    s1 = {v: x[:-1] + [x[-1] + _rb(rng, 1)] for v, x in s.items()}
    add("hash_stage_res15_over", s1, {15: False}, "the same one byte longer: "
        "span 6160", spans={15: HASH_STAGE + 16}, twin="hash_stage_res15")
    # one string that passes the stage alone, in the first or the last lane
    for nm, lane in (("first", 0), ("last", 63)):
        for ln in LONG_LENS:
            def short(k):
                return [_rb(rng, rng.choice([0, 0, 1, 3, 7, 12, 20, 33]))
                        for _ in range(k)]
            st = {"single": short(lane) + [_rb(rng, ln)] + short(63 - lane)}
            for role in (0, 1):
                x = short(128)
                x[2 * lane + role] = _rb(rng, ln)
                st["pairs_" + ("name", "value")[role]] = x
            add("hash_%s_lane_long_%d" % (nm, ln), st, {0: False, 5: False},
                "a string of %d bytes in lane %d (pairs: as a name, as a "
                "value), short and empty ones beside it" % (ln, lane))
    # partial last tiles: HashOffs::load's clamped lanes, last()
    for cnt in (1, 2, 63):
        for staged in (True, False):
            def mk(pairs):
                x = [_rb(rng, rng.choice([0, 2, 9, 17, 30, 41]))
                     for _ in range(cnt * (2 if pairs else 1))]
                if not staged:
                    x[rng.randrange(len(x))] = _rb(rng, FILLER)
                return x
            add("hash_partial_%d_%s" % (cnt, "staged" if staged else "glb"),
                both(mk), {0: staged, 5: staged}, "a last tile of %d, %s"
                % (cnt, "staged" if staged else "past the stage"), last=True)
    # length x alignment, through LDS and through global memory
    add("hash_lengths", both(lambda pairs: lengths_run(rng, pairs, False)),
        {0: True}, "every length 0..96 at every start residue 0..15, staged "
        "tiles (HashLds)")
    add("hash_lengths_glb", both(lambda pairs: lengths_run(rng, pairs, True)),
        {0: False}, "the same with one string of 6200 bytes in every tile: "
        "unstaged tiles (HashGlb)")
    return fx


HASH = _hash_fixtures()
HASH_BY_NAME = {f.name: f for f in HASH}


def pack_around(pre, run, post, residue, pad_front=True):
    """pre + run + post packed, the run's first byte on `residue`: by
    pad_front bytes in front of the data (to_dev) or, pad_front False, by
    that many more bytes on the last string of pre -> (data, off, pad,
    first tile of the run is at string index len(pre))"""
    p = (residue - sum(len(s) for s in pre)) % 16
    if not pad_front:
        pre = pre[:-1] + [pre[-1] + bytes(range(100, 100 + p))]
        p = 0
    data, off = pack(pre + list(run) + post)
    return data, off, p


def hash_batch_of(f, variant, residue, pad_front=True):
    """(data, off, pad_front, first tile, tiles) of fixture f's run in
    layout `variant` between two ordinary tiles on either side (none after
    a run that ends in a partial tile); off has n + 1 entries (single) or
    2n + 1 (pairs)"""
    pairs = is_pairs(variant)
    rng = random.Random(len(f.name) * 139 + residue + 7 * len(variant))
    pre = hash_ordinary(rng, pairs)
    post = [] if f.last else hash_ordinary(rng, pairs)
    run = f.strings[variant]
    per = TS * (2 if pairs else 1)
    assert f.last or len(run) % per == 0
    data, off, pad = pack_around(pre, run, post, residue, pad_front)
    ti = len(pre) // per
    assert (int(off[len(pre)]) + pad) % 16 == residue
    return data, off, pad, ti, -(-len(run) // per)


def hash_oracle(data, off, pairs, seed):
    """the oracle's hashes: (name_hash, nameval_hash) or (hash,)"""
    if pairs:
        return O.xxh32_headers(data, off, seed)
    raw = data.tobytes()
    return (np.array([O.xxh32(raw[int(off[i]):int(off[i + 1])], seed)
                      for i in range(len(off) - 1)], dtype=np.uint32),)


CHAIN_TILES = 640             # full tiles of the chain batch
CHAIN_LAST = 37               # headers (strings) in its partial last tile


def hash_chain(pairs):
    """The multi-round batch: CHAIN_TILES full tiles and a last one of
    CHAIN_LAST.  Every HASH fixture that is made of whole tiles is spliced
    in once, at each of its residues (a few bytes more on the string in
    front put it there); every other tile is staged (token-sized strings)
    or not by a fixed-seed coin, the unstaged ones alternately one string of
    6200 bytes among short ones and equal strings of about 50 (pairs) or
    100 (single) bytes.  -> (data, off, [(fixture, residue, first tile)],
    plan): plan[t] is what tile t was built to be (True staged, False not;
    a fixture's tiles: its want); 16-byte-aligned buffer, off[0] = 0."""
    rng = random.Random(4099 + pairs)
    per = TS * (2 if pairs else 1)
    runs = []
    for f in HASH:
        if f.last:
            continue
        for v in f.variants():
            if is_pairs(v) == pairs:
                for r in f.residues:
                    runs.append((f, r, f.strings[v]))
    n_fix = sum(len(s) // per for _, _, s in runs)
    n_gen = CHAIN_TILES - n_fix
    assert n_gen >= 2 * len(runs) + 300
    # a run goes in after every `gap` generic tiles (never first)
    gap = n_gen // (len(runs) + 1)
    strs, where, plan, pos, alt, g = [], [], [], 0, 0, 0

    def generic():
        nonlocal alt
        if rng.random() < 0.5:
            plan.append(True)
            return [_rb(rng, rng.randint(8, 40)) for _ in range(per)]
        plan.append(False)
        alt ^= 1
        if alt:
            x = [_rb(rng, rng.choice([0, 3, 8, 15, 22])) for _ in range(per)]
            x[rng.randrange(TS) * (per // TS) + (per // TS - 1)] = \
                _rb(rng, FILLER)
            return x
        return [_rb(rng, rng.randint(48, 53) * (2 if not pairs else 1))
                for _ in range(per)]

    for f, r, run in runs:
        for _ in range(gap):
            t = generic()
            strs += t
            pos += sum(len(s) for s in t)
            g += 1
        p = (r - pos) % 16
        strs[-1] = strs[-1] + _rb(rng, p)
        pos += p
        assert pos % 16 == r and len(strs) % per == 0
        where.append((f, r, len(strs) // per))
        strs += run
        plan += [f.want[r]] * (len(run) // per)
        pos += sum(len(s) for s in run)
    while g < n_gen:
        strs += generic()
        g += 1
    assert len(strs) == CHAIN_TILES * per
    strs += [_rb(rng, rng.randint(8, 40))
             for _ in range(CHAIN_LAST * (per // TS))]
    plan.append(True)
    data, off = pack(strs)
    return data, off, where, plan


def transitions(staged, w):
    """how often each (staged[t], staged[t + w]) occurs"""
    c = {(a, b): 0 for a in (True, False) for b in (True, False)}
    for a, b in zip(staged, staged[w:]):
        c[(a, b)] += 1
    return c
