"""The model of qhuff_static_lookup / qhuff_encode_headers: which field line
the reference's encoder writes for a header when the dynamic table is not
used, and its bytes.

Nothing here comes from the library.  A header's line is chosen by the
reference's rule (lsqpack.c:1671-1715, 1835-1866) restated over the
reference's own tables as data (tests/golden/static_lookup.json: the four
arrays of lsqpack.c:629-716; tests/golden/qpack_static_table.json): hash the
name and the value with the reference's XXH32 -- the compiled
deps/xxhash/xxhash.c in oracle/_ref where that was built, as test_xxh32.py
loads it, else its restatement oracle_lib.xxh32, which test_xxh32.py pins to
the reference's vectors -- probe, compare.  The line's bytes are
qpack_frames.enc_int + oracle_lib.enc_enc_str (lsqpack.c:2033-2039,
2061-2076, 2110-2125), a section's the prefix 00 00 (lsqpack.c:1277, 1296)
and its lines."""
import ctypes as C
import functools
import json
import os
import random

import numpy as np

import _paths  # noqa: F401
import oracle_lib as O
import qpack_frames as Q

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REF_SO = os.path.join(O.ROOT, "oracle", "_ref", "libxxh32_ref.so")

INDEXED, NAMEREF, LITERAL = 0, 1, 2      # QHUFF_LINE_*
NONE = 0xFF                              # QHUFF_STATIC_NONE
NEVER = 1                                # QHUFF_HDR_NEVER_INDEX

with open(os.path.join(G, "static_lookup.json")) as f:
    FIX = json.load(f)
with open(os.path.join(G, "qpack_static_table.json")) as f:
    STATIC = [(n.encode("latin-1"), v.encode("latin-1"))
              for n, v in json.load(f)["static_table"]]
SEED = FIX["seed"]
NAME2ID, NAMEVAL2ID = FIX["name2id_plus_one"], FIX["nameval2id_plus_one"]
NMASK = (1 << FIX["name_width"]) - 1
NVMASK = (1 << FIX["nameval_width"]) - 1
assert FIX["name_shift"] == 0 == FIX["nameval_shift"]
assert len(NAME2ID) == 512 == len(NAMEVAL2ID) and len(STATIC) == 99


@functools.lru_cache(maxsize=None)
def _ref():
    if not os.path.exists(REF_SO):
        return None
    L = C.CDLL(REF_SO)
    L.XXH32.restype = C.c_uint
    L.XXH32.argtypes = [C.c_char_p, C.c_size_t, C.c_uint]
    return L


def xxh32(s, seed):
    """the reference's XXH32 (see the module's docstring)"""
    L = _ref()
    return L.XXH32(s, len(s), seed) if L is not None else O.xxh32(s, seed)


def hashes(name, value):
    h1 = xxh32(name, SEED)
    return h1, xxh32(value, h1)


def lookup(name, value):
    """-> (name_hash, nameval_hash, kind, static id): find_in_static_full,
    else lsqpack_find_in_static_headers (lsqpack.c:721-764)"""
    h1, h2 = hashes(name, value)
    i = NAMEVAL2ID[h2 & NVMASK]
    if i and STATIC[i - 1] == (name, value):
        return h1, h2, INDEXED, i - 1
    i = NAME2ID[h1 & NMASK]
    if i and STATIC[i - 1][0] == name:
        return h1, h2, NAMEREF, i - 1
    return h1, h2, LITERAL, NONE


def line(name, value, never=0):
    """the field line's bytes -> (bytes, kind, id)"""
    _, _, kind, i = lookup(name, value)
    n = 1 if never & NEVER else 0
    if kind == INDEXED:
        return Q.enc_int(0xC0, i, 6), kind, i
    if kind == NAMEREF:
        return (Q.enc_int(0x50 | n << 5, i, 4) + O.enc_enc_str(7, value),
                kind, i)
    return (O.enc_enc_str(3, name, 0x20 | n << 4) + O.enc_enc_str(7, value),
            kind, i)


class Headers:
    """header lists, one section each -> the call's arrays and what it must
    give back.  sections: [[(name, value) or (name, value, flags), ...], ...]"""

    def __init__(self, sections, flags=True):
        self.sections = [[(h[0], h[1], h[2] if len(h) > 2 else 0) for h in s]
                         for s in sections]
        hs = [h for s in self.sections for h in s]
        self.n, self.m = len(hs), len(self.sections)
        parts = [x for h in hs for x in h[:2]]
        self.off = np.zeros(2 * self.n + 1, dtype=np.uint32)
        np.cumsum([len(p) for p in parts], out=self.off[1:])
        self.data = np.frombuffer(b"".join(parts), dtype=np.uint8).copy()
        self.sec_hdr = np.zeros(self.m + 1, dtype=np.uint32)
        np.cumsum([len(s) for s in self.sections], out=self.sec_hdr[1:])
        self.hflags = (np.array([h[2] for h in hs], dtype=np.uint8)
                       if flags else None)
        if not flags:
            assert not any(h[2] for h in hs)

    @functools.cached_property
    def lines(self):
        return [[line(*h) for h in s] for s in self.sections]

    @functools.cached_property
    def want_sections(self):
        return [b"\0\0" + b"".join(x[0] for x in s) for s in self.lines]

    @property
    def want(self):
        return b"".join(self.want_sections)

    @functools.cached_property
    def want_sec_out(self):
        o = np.zeros(self.m + 1, dtype=np.uint32)
        np.cumsum([len(s) for s in self.want_sections], out=o[1:])
        return o

    @functools.cached_property
    def want_kind(self):
        return np.array([x[1] for s in self.lines for x in s], dtype=np.uint8)

    @functools.cached_property
    def want_id(self):
        return np.array([x[2] for s in self.lines for x in s], dtype=np.uint8)

    @property
    def bound(self):
        # qhuff_encode_wire_bound(in_bytes, 2n + 2m), include/qhuff.h
        return ((30 * len(self.data) + 7) // 8
                + 13 * (2 * self.n + 2 * self.m) + 16)


def pack_pairs(pairs):
    """[(name, value)] -> (data, off [2n + 1])"""
    h = Headers([pairs])
    return h.data, h.off


# ---- near misses, found by search ------------------------------------------------

ALPHA = b"abcdefghijklmnopqrstuvwxyz-:0123456789"


def _rand(rng, n):
    return bytes(rng.choice(ALPHA) for _ in range(n))


@functools.lru_cache(maxsize=None)
def near_misses():
    """{label: [(name, value)]}: headers that reach each compare of the
    lookup and fail it (or just pass).  Searched with the oracle's XXH32 for
    speed; the expectation for every one of them is lookup()'s."""
    rng = random.Random(20260)
    out = {}
    names = sorted({n for n, _ in STATIC})

    def name_slot(s):
        return NAME2ID[O.xxh32(s, SEED) & NMASK]

    # a name on an occupied name2id slot, of another length than its entry
    got = []
    while len(got) < 12:
        s = _rand(rng, rng.randrange(1, 24))
        i = name_slot(s)
        if i and len(STATIC[i - 1][0]) != len(s):
            got.append((s, _rand(rng, rng.randrange(0, 9))))
    out["name_slot_other_length"] = got
    # ... of its entry's length: random bytes, and the entry's name with
    # another last byte (the compare runs to the name's end)
    got = []
    while len(got) < 6:
        s = _rand(rng, rng.choice((3, 4, 5, 6, 7, 10, 13)))
        i = name_slot(s)
        if i and len(STATIC[i - 1][0]) == len(s) and STATIC[i - 1][0] != s:
            got.append((s, b"v"))
    out["name_slot_same_length"] = got
    got = []
    for nm in names:
        i0 = name_slot(nm)
        for x in range(256):
            s = nm[:-1] + bytes([x])
            if s != nm and name_slot(s) == i0:
                got.append((s, STATIC[i0 - 1][1]))
                break
    assert len(got) >= 8
    out["name_last_byte"] = got
    # a proper prefix of a static name, a static name and one byte more,
    # and any static name with another last byte wherever it lands
    out["name_prefix"] = [(nm[:-1], b"1") for nm in names[::5]]
    out["name_plus_one"] = [(nm + b"s", b"1") for nm in names[::5]]
    out["name_changed"] = [(nm[:-1] + bytes([nm[-1] ^ 1]), b"")
                           for nm in names[::7]]

    def nv_slot(nm, v):
        return NAMEVAL2ID[O.xxh32(v, O.xxh32(nm, SEED)) & NVMASK]

    # name + value on an occupied nameval2id slot whose entry has this name:
    # a value of another length, and the entry's value with another last byte
    by_name = {}
    for i, (nm, v) in enumerate(STATIC):
        by_name.setdefault(nm, []).append(i)
    multi = [nm for nm in names if len(by_name[nm]) >= 3]
    got = []
    while len(got) < 10:
        nm = rng.choice(multi)
        v = _rand(rng, rng.randrange(0, 30))
        i = nv_slot(nm, v)
        if i and STATIC[i - 1][0] == nm and len(STATIC[i - 1][1]) != len(v):
            got.append((nm, v))
    out["value_slot_other_length"] = got
    got = []
    for i, (nm, v) in enumerate(STATIC):
        if not v:
            continue
        for x in range(256):
            w = v[:-1] + bytes([x])
            if w != v and nv_slot(nm, w) == i + 1:
                got.append((nm, w))
                break
    assert len(got) >= 12
    out["value_last_byte"] = got
    # an empty value against ":authority" (INDEXED 0) and "age" (NAMEREF 2),
    # an empty name, an upper-case name
    out["empty_value"] = [(b":authority", b""), (b"age", b"")]
    out["empty_name"] = [(b"", b""), (b"", b"x"), (b"", b"GET")]
    out["upper_case"] = [(b":METHOD", b"GET"), (b":Method", b"GET"),
                         (b":method", b"get")]
    # every entry, and every entry with a changed value
    out["entries"] = list(STATIC)
    out["entries_other_value"] = [(nm, v + b"x") for nm, v in STATIC]
    return out


def near_miss_pairs():
    return [p for _, ps in sorted(near_misses().items()) for p in ps]


# ---- the reference's own vectors ------------------------------------------------------

# test/test_qpack.c:47, :64, :83 (header bytes only: its encoder-stream bytes
# belong to the dynamic table), :129; the flags are those of the C source,
# which the golden file does not carry: they are read back from the N bit
VECTORS = ("47", "64", "83", "129")


def reference_vectors():
    """[(source line, [(name, value, flags)], prefix + header bytes)]"""
    with open(os.path.join(G, "kat_header_blocks.json")) as f:
        hb = json.load(f)["header_blocks"]
    out = []
    for k in hb:
        ln = k["source"].rsplit(":", 1)[1]
        if ln not in VECTORS:
            continue
        body = bytes.fromhex(k["header"])
        b0 = body[0]
        never = (b0 >> 5 & 1) if b0 & 0xC0 == 0x40 else \
            (b0 >> 4 & 1) if b0 & 0xE0 == 0x20 else 0
        hs = [(bytes.fromhex(n), bytes.fromhex(v), never)
              for n, v in k["headers"]]
        assert len(hs) == 1 and k["prefix"] == "0000"
        out.append((ln, hs, b"\0\0" + body))
    assert [v[0] for v in out] == list(VECTORS)
    assert [v[1][0][2] for v in out] == [0, 1, 0, 1]     # LQEF_NEVER_INDEX
    return out
