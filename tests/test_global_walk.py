"""Strings past the 3,072-byte stage, which every decode-family kernel walks
in global memory with the one decoder (decode_string over DecGlb,
qhuff_decode_impl.h): window_walk() and tail_lookup() behind a source that
loads no dword past the string's last byte.

Each input is one Huffman string of more than limits.STAGE bytes among a
tile of short token strings: the smallest input at which the global walk
can still go wrong.  Expected values are the oracle's (huff_decode,
decode_batch, decoded_prefix, huff_decode_chunked); the generators are
checked on the CPU (test_generators), where limits.classify() /
classify_svc() also say that every input reaches the path it is meant for.
"""
import functools
import os
import random

import numpy as np
import pytest

import _paths  # noqa: F401
import limits as L
import oracle_lib as O
import qhuff
import test_stream_decode as TS
import test_wire_decode as TW
from test_frames import field_line
from test_limits import _torch, codec, gpu_decode  # noqa: F401
from test_lsqpack_shim import oracle_decode, shim, shim_decode  # noqa: F401
from test_service_limits import check_dec, svc  # noqa: F401

L0 = L.STAGE + 1                 # the shortest string past the stage
LANE = 29                        # the long string's lane in its tile
EOS = 256


def code_str(sym):
    c, n = O.code_of(sym)
    return format(c, "0%db" % n)


def bits_of(syms):
    return "".join(code_str(s) for s in syms)


def to_bytes(bits):
    assert len(bits) % 8 == 0
    return bytes(int(bits[i:i + 8], 2) for i in range(0, len(bits), 8))


def tokens_until(rng, nbits, ok=lambda bits: True):
    """random token symbols of at least nbits code bits in all, ending where
    ok(bits) holds (code lengths of 5..8 bits reach every residue)"""
    s, bits = [], 0
    while bits < nbits or not ok(bits):
        s.append(rng.choice(L.TOKEN))
        bits += L.CODE_LEN[s[-1]]
    return s, bits


# ---- D: one string per way of being rejected, each longer than the stage ----

@functools.lru_cache(maxsize=None)
def rejected():
    """name -> (string, symbols decoded before the error, whether the error
    is the EOS code)"""
    rng = random.Random(3073)
    out = {}
    # the EOS code after five symbols
    head = [rng.choice(L.TOKEN) for _ in range(5)]
    rest, _ = tokens_until(rng, 8 * L0)
    bits = bits_of(head) + code_str(EOS) + bits_of(rest)
    out["eos_early"] = (to_bytes(bits + "1" * (-len(bits) % 8)), bytes(head),
                        True)
    # the EOS code within the last 32 bits: at most two bits of padding
    s, n = tokens_until(rng, 8 * L0, lambda b: (-(b + 30)) % 8 <= 2)
    bits = bits_of(s) + code_str(EOS)
    pad = -len(bits) % 8
    assert pad <= 2
    out["eos_late"] = (to_bytes(bits + "1" * pad), bytes(s), True)
    # a long code cut off by the end of the string: k of its bits, a zero
    # among them and 13 or more, so that the walk meets it as a long code
    long_sym = next(x for x in range(256) if L.CODE_LEN[x] >= 21
                    and "0" in code_str(x)[:16])
    s, n = tokens_until(rng, 8 * L0, lambda b: (-b) % 8 + 16 <= 20)
    k = (-n) % 8 + 16
    assert 13 <= k < L.CODE_LEN[long_sym] and "0" in code_str(long_sym)[:k]
    out["past_end"] = (to_bytes(bits_of(s) + code_str(long_sym)[:k]), bytes(s),
                       False)
    # padding that is not all ones; padding of eight or more ones
    h = L.token_huff(L0, rng)
    out["pad_zero"] = (L.invalid_same_len(h), O.huff_decode(h)[1], False)
    h = L.token_huff(L0, rng)
    out["pad_ones"] = (h + b"\xff", O.huff_decode(h)[1], False)
    return out


REJECTED = ("eos_early", "eos_late", "past_end", "pad_zero", "pad_ones")


@functools.lru_cache(maxsize=None)
def valid(n):
    return L.token_huff(n, random.Random(n))


@functools.lru_cache(maxsize=None)
def long_codes():
    """C: a string past the stage, two symbols in five with codes of 14 to
    30 bits, the last symbol one of them with 1..7 bits of padding"""
    rng = random.Random(14)
    longs = [x for x in range(256) if L.CODE_LEN[x] >= 14]
    s, bits = [], 0
    while bits < 8 * L0:
        s.append(rng.choice(longs) if rng.random() < 0.4
                 else rng.choice(L.TOKEN))
        bits += L.CODE_LEN[s[-1]]
    last = next(x for x in longs if (bits + L.CODE_LEN[x]) % 8)
    s.append(last)
    h = O.huffman_enc(bytes(s))
    assert O.huff_decode(h) == (O.OK, bytes(s))
    return h, bytes(s)


def straddlers(syms, res):
    """the long codes of syms that cross a dword boundary when the string's
    first byte is at res (mod 4)"""
    n, pos = 0, 8 * res
    for c in syms:
        ln = L.CODE_LEN[c]
        n += ln >= 14 and pos // 32 != (pos + ln - 1) // 32
        pos += ln
    return n


# ---- batches: the long string in a tile of token strings --------------------------

@functools.lru_cache(maxsize=None)
def batch(h, lane=LANE, res=0):
    """two ordinary tiles, a tile with h in `lane`, two ordinary tiles; the
    padding in front puts h's first byte on res (mod 4) of an aligned
    buffer.  -> data, off, pad, h's index, the oracle's result"""
    rng = random.Random(len(h) + 64 * lane)
    pre, tile, post = (L.token_tiles(rng), L.token_tiles(rng, 1),
                       L.token_tiles(rng))
    tile[lane] = h
    strings = pre + tile + post
    data, off = L.pack(strings)
    i = len(pre) + lane
    pad = (res - int(off[i])) % 4 + 4 * (lane % 4)
    assert (pad + int(off[i])) % 4 == res
    return data, off, pad, i, O.decode_batch(data, off)


def tiles_of(b, lean=False):
    data, off, pad, i, want = b
    sizes = np.diff(want[1].astype(np.int64))
    return L.classify(off.astype(np.int64) + pad, 0, sizes, lean=lean)


def check_path(b, into_slot, path):
    """the string's tile: past the stage, the string a lone unit (full
    kernel: written into the slot or only counted; the tile's path), the
    lean kernel's tile slow; every other tile ordinary"""
    data, off, pad, i, want = b
    ti, lane = divmod(i, L.TS)
    for lean in (False, True):
        info = tiles_of(b, lean)
        for j, t in enumerate(info):
            if j != ti:
                assert t["staged"] and t["path"] == "fast"
        assert not info[ti]["staged"]
        if lean:
            assert info[ti]["path"] == "slow" and not info[ti]["units"]
            continue
        u = [u for u in info[ti]["units"] if u["lo"] == lane]
        assert len(u) == 1 and u[0]["lone"] and u[0]["into_slot"] == into_slot
        assert info[ti]["path"] == path


# B: the lone branch's two arms: the string's bound against the slot
L_IN = max(n for n in range(L0, L.BIG_SLOT) if 8 * n // 5 + 1 <= L.BIG_SLOT)
ARMS = ((L_IN, True, "slot"), (L_IN + 1, False, "slow"))

# A: the first byte at each residue of a dword, and the last byte at each
PLACEMENTS = [(res, L0 + k) for res in range(4) for k in range(4)]


# ---- H: the generators, on the CPU ----------------------------------------------------

def test_generators():
    assert L_IN == 7679 and 8 * (L_IN + 1) // 5 + 1 == L.BIG_SLOT + 1
    # A
    assert sorted({(r, (r + n - 1) % 4) for r, n in PLACEMENTS}) \
        == [(a, b) for a in range(4) for b in range(4)]
    for res, n in PLACEMENTS:
        h = valid(n)
        assert len(h) == n > L.STAGE and O.huff_decode(h)[0] == O.OK
        b = batch(h, LANE, res)
        assert (b[2] + int(b[1][b[3]])) % 4 == res
        check_path(b, True, "slot")
    # B
    for n, into, path in ARMS:
        assert O.huff_decode(valid(n))[0] == O.OK
        check_path(batch(valid(n), 0, 0), into, path)
    # C
    h, s = long_codes()
    assert len(h) > L.STAGE and L.CODE_LEN[s[-1]] >= 14
    assert 1 <= 8 * len(h) - L.code_bits(s) <= 7
    for res in range(4):
        assert straddlers(s, res) > 100
        check_path(batch(h, LANE, res), True, "slot")
    # D
    assert sorted(rejected()) == sorted(REJECTED)
    for name in REJECTED:
        h, pre, eos = rejected()[name]
        assert len(h) > L.STAGE and O.huff_decode(h) == (O.ERROR, b"")
        assert O.decoded_prefix(h) == (pre, eos), name
        left = "".join(format(x, "08b") for x in h)[L.code_bits(pre):]
        if name == "eos_early":
            assert len(pre) == 5 and len(left) > 8 * L.STAGE
        elif name == "eos_late":
            assert 30 <= len(left) <= 32 and set(left) == {"1"}
        elif name == "past_end":
            assert 16 <= len(left) <= 20 and "0" in left
        elif name == "pad_zero":
            assert 1 <= len(left) <= 7 and left[-1] == "0"
        else:
            assert 9 <= len(left) <= 15 and set(left) == {"1"}
        b = batch(h)
        assert list(np.nonzero(b[4][2])[0]) == [b[3]]
        check_path(b, True, "slot")
        data, off, want = svc_call(h)
        p = L.classify_svc(off, np.diff(want[1].astype(np.int64)))
        assert [x["route"] for x in p] == ["direct", "scratch", "direct"]
        assert p[1]["path"] == "slow" and not p[1]["staged"]
        assert off[-1] <= L.SVC_MAX_BYTES
    # F, G
    for name in ("valid",) + REJECTED:
        s = wire_shape(name)
        assert s.lits[LANE].len > L.STAGE and s.lits[LANE].huffman
    for name, max_len, status in wire_limit_cases():
        s = wire_limit_shape(name)[0]
        a, v = s.lits[63], s.lits[64]
        assert a.kind == qhuff.LIT_NAME and a.huffman and a.len > L.STAGE
        assert v.kind == qhuff.LIT_VALUE and v.instr == a.instr
        assert TW.tile_staged(s.lits, 0)[:2] == [False, True]
    h, text, cuts = stream_string()
    assert len(cuts) >= 3
    for c in cuts:
        assert c > L.STAGE and len(h) - c > L.STAGE
        assert O.huff_decode_chunked(h, c, len(text) + 8, len(text) + 8) \
            == (O.OK, text)


# ---- GPU ---------------------------------------------------------------------------------

@pytest.fixture(scope="module", params=["lean", "full", "auto"])
def kcodec(request):
    """a codec pinned to each kernel variant (the variable set only around
    the constructor, as test_kernel_variants)"""
    _torch()
    old = os.environ.get("QHUFF_KERNELS")
    os.environ["QHUFF_KERNELS"] = request.param
    try:
        c = qhuff.Codec(0)
    finally:
        if old is None:
            del os.environ["QHUFF_KERNELS"]
        else:
            os.environ["QHUFF_KERNELS"] = old
    yield c
    c.close()


def check_batch(c, b, what):
    data, off, pad, i, (o_out, o_off, o_st) = b
    g_out, g_off, g_st = gpu_decode(c, data, off, pad)
    assert np.array_equal(g_st, o_st), what
    assert np.array_equal(g_off, o_off), what
    assert np.array_equal(g_out, o_out), what
    return g_off, g_st


@pytest.mark.gpu
def test_alignment_of_start_and_end(kcodec):
    """A: the string's first byte at each residue of a dword (0: the walk's
    set-up without a shift) and its last byte at each (the guard's cut)"""
    for res, n in PLACEMENTS:
        check_batch(kcodec, batch(valid(n), LANE, res), (res, n))


@pytest.mark.gpu
def test_lone_branch_arms(kcodec):
    """B: the full kernel's lone string written into the slot (its bound
    fits) or counted, then written by the slow tile (one byte more)"""
    for n, into, path in ARMS:
        check_batch(kcodec, batch(valid(n), 0, 0), n)


@pytest.mark.gpu
def test_long_codes_across_dwords(kcodec):
    """C: codes of 14 to 30 bits across the dword boundaries of global
    memory, the last symbol one of them"""
    h, s = long_codes()
    for res in range(4):
        data, off, pad, i, want = b = batch(h, LANE, res)
        g_off, _ = check_batch(kcodec, b, res)
        assert int(g_off[i + 1]) - int(g_off[i]) == len(s)


@pytest.mark.gpu
@pytest.mark.parametrize("name", REJECTED)
def test_rejections(kcodec, name):
    """D: status ERROR and no output bytes, the strings around it intact"""
    data, off, pad, i, want = b = batch(rejected()[name][0])
    g_off, g_st = check_batch(kcodec, b, name)
    assert g_st[i] == qhuff.DEC_ERROR and g_off[i + 1] == g_off[i]
    assert int(g_st.sum()) == 1


@functools.lru_cache(maxsize=None)
def svc_call(h):
    rng = random.Random(len(h))
    t = L.token_tiles(rng, 1)
    data, off = L.pack(t[:5] + [h] + t[5:10])
    return data, off, O.decode_batch(data, off)


@pytest.mark.gpu
@pytest.mark.parametrize("name", REJECTED)
def test_rejections_service(svc, name):
    """D through the service: the string is a piece of its own, sized and
    decoded in device scratch by slow_tile_at"""
    data, off, want = svc_call(rejected()[name][0])
    st = check_dec(svc, data, off, want, name)
    assert list(st) == [0] * 5 + [1] + [0] * 5
    assert want[1][6] == want[1][5]


@pytest.mark.gpu
@pytest.mark.parametrize("name", REJECTED)
def test_keep_kernel_prefix(shim, name):
    """E: the per-string decode replays the reference over the bytes the
    Keep kernel decoded before the error (the walk emits up to two symbols
    a step): (status, dst, n_dst, n_src) at dst_len n - 1, n, n + 1"""
    h, pre, _ = rejected()[name]
    n = len(pre)
    for dst_len in (n - 1, n, n + 1):
        got = shim_decode(shim, h, dst_len)
        want = oracle_decode(h, dst_len)
        assert got == want, (name, dst_len, got[0], got[2:], want[0], want[2:])


# ---- F: the wire kernel ------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def wire_shape(name):
    """64 literals, lane 29 a Huffman literal past the stage: valid, or one
    of the rejected strings"""
    rng = random.Random(29)
    big = valid(L0 + 2) if name == "valid" else rejected()[name][0]
    buf, lits = b"", []
    for i in range(TW.TILE):
        s, h = (big, True) if i == LANE else TW.mixed(rng, i)
        lits.append(TW.lit(len(buf), s, h))
        buf += s + bytes(rng.randrange(4))
    return TW.Shape(buf, lits, staged=False, unstaged=True)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("valid",) + REJECTED)
def test_wire_literal_past_the_stage(codec, name):
    s = wire_shape(name)
    outs, status = TW.check_both(codec, s)
    for l, o, st in zip(s.lits, outs, status):
        payload = s.buf[l.pos:l.pos + l.len]
        if l.huffman:
            ost, w = O.huff_decode(payload)
            assert (st, o) == ((0, w) if ost == O.OK else (1, b""))
        else:
            assert (st, o) == (0, payload)
    assert status[LANE] == (0 if name == "valid" else 1)


N_VALUE = 100


@functools.lru_cache(maxsize=None)
def wire_limit_shape(name):
    """a NAME literal past the stage on lane 63 of a tile and its VALUE on
    lane 0 of the next -> (Shape, the NAME's decoded length or None)"""
    nm = valid(L0 + 27) if name == "valid" else rejected()[name][0]
    buf, lits = b"", []

    def add(blk):
        nonlocal buf, lits
        rc, ls = qhuff.scan_field_section(blk, len(buf))
        assert rc == qhuff.OK
        buf += blk
        lits += ls

    k = 0
    while len(lits) % TW.TILE != 63:
        add(b"\x00\x00\x45" + field_line(0, 7, b"v%d" % k))
        k += 1
    add(b"\x00\x00" + field_line(0x20, 3, nm, huffman=True)
        + field_line(0, 7, TW.a_payload(N_VALUE), huffman=True))
    add(b"\x00\x00\x45" + field_line(0, 7, b"end"))
    st, out = O.huff_decode(nm)
    return TW.Shape(buf, lits), len(out) if st == O.OK else None


def wire_limit_cases():
    n = wire_limit_shape("valid")[1]
    return (("valid", n + N_VALUE, [0, 0]), ("valid", n + N_VALUE - 1, [0, 1]),
            ("pad_zero", N_VALUE + 10, [1, 0]))


@pytest.mark.gpu
def test_wire_limit_counts_the_name_in_global_memory(codec):
    """the VALUE's limit needs its NAME's decoded length, and the NAME is
    the previous tile's last literal, past the stage: wire_limit_rare walks
    it in global memory (an invalid NAME counts for nothing)"""
    for name, max_len, want in wire_limit_cases():
        s = wire_limit_shape(name)[0]
        outs, status = TW.check_both(codec, s, max_len)
        assert status[63:65] == want, (name, max_len)
        assert not any(status[:63]) and not any(status[65:])


# ---- G: the stream kernel -----------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def stream_string():
    """token text, a 30-bit code, token text, each run past the stage: cut
    at the bytes inside the long code, the first piece ends in the middle
    of it and the second starts on a node that is not the root"""
    rng = random.Random(30)
    a, na = tokens_until(rng, 8 * L0 + 64)
    b, _ = tokens_until(rng, 8 * L0 + 64)
    text = bytes(a) + L.B30[:1] + bytes(b)
    h = O.huffman_enc(text)
    assert O.huff_decode(h) == (O.OK, text)
    cuts = [c for c in range(len(h)) if na < 8 * c < na + 30]
    return h, text, cuts


@pytest.mark.gpu
def test_stream_chunks_past_the_stage(codec):
    h, text, cuts = stream_string()
    nodes = TS.node_set_pairs()
    pairs = []
    for t, c in enumerate(cuts):
        pairs += nodes[63 * t:63 * t + 63] + [(h[:c], h[c:])]
    st = TS.run_rounds(codec, TS.two_rounds(pairs))
    assert (st[0] == qhuff.DEC_MORE).all() and (st[1] == qhuff.DEC_OK).all()
    # the two launches' bytes, against the oracle's chunked decode
    state = np.zeros((len(pairs), 2), dtype=np.uint8)
    got = [b""] * len(pairs)
    for k, flag in ((0, 0), (1, qhuff.STREAM_FINAL)):
        flags = np.full(len(pairs), flag, dtype=np.uint8)
        outs, status, state, _ = TS.gpu_round(codec, [p[k] for p in pairs],
                                              state, flags)
        got = [g + o for g, o in zip(got, outs)]
    for t, c in enumerate(cuts):
        cap = len(text) + 8
        assert (O.OK, got[64 * t + 63]) == O.huff_decode_chunked(h, c, cap, cap)
