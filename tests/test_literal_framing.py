"""Literal framing at every boundary of the length integer, on each path that
writes it (framing.py has the cases, the batches and the paths).

CPU part: every case's expectation is qpack_frames.enc_int(H << p, L, p) +
payload, which is what the oracle gives; limits.classify_enc puts every
fixture tile on the path its batch is named for, at every padding the GPU
part runs at; and on every path each (prefix, length, kind) the path can
hold starts on each byte residue of an output dword.  GPU part: the batches
through qhuff_encode_batch (default, lean and full kernels, three paddings,
and mode 0 as the control), its host form (staged and registered), the
two-context host form cut inside the fixture tiles, the service one fixture
tile a call, qhuff_encode_wire and its host form for the 16 KB literals
behind an integer and for the boundary integers on the tiles off the dense
path, four strings of 2 MB for the header's fifth byte, and the
literals read back where the encoder put them by qhuff_decode_wire.
Everything is compared with the oracle, bytes and offsets.
"""
import functools
import random
import time

import numpy as np
import pytest

import _paths  # noqa: F401
import framing as F
import limits as L
import oracle_lib as O
import qhuff
import qpack_frames as Q
from test_encode_wire import Batch as WireBatch
from test_encode_wire import allowed_first, check_both, item
from test_limits import _torch, codec, to_dev, vcodec  # noqa: F401
from test_service_limits import check_enc, svc  # noqa: F401

NAMES = list(F.batches())


# ---- CPU ---------------------------------------------------------------------------

def framed(c, first=0):
    payload = O.huffman_enc(c.s) if c.huff else c.s
    assert len(payload) == c.L
    return Q.enc_int(first | c.huff << c.p, c.L, c.p) + payload


def test_cases_are_the_integer_coder_plus_payload():
    """1: header bytes and H bit as listed; the oracle's literal is enc_int
    (pinned to the reference's integer vectors) + the payload"""
    cs = F.cases()
    assert len(cs) == 54
    for p in F.PREFIXES:
        mask = (1 << p) - 1
        assert F.lengths(p) == [(mask - 1, 1), (mask, 2), (mask + 127, 2),
                                (mask + 128, 3), (mask + 16383, 3),
                                (mask + 16384, 4)]
    for c in cs + F.big_cases():
        hb = O.enc_str_size(c.s)
        if c.kind == "longer":
            assert len(c.s) == c.L < hb
        else:
            assert (hb, len(c.s)) == (c.L, c.L + (c.kind == "shorter")), c[:3]
        assert c.huff == (c.kind == "shorter")
        w = framed(c)
        assert len(w) == c.hdr + c.L, c[:3]
        assert O.enc_enc_str(c.p, c.s, 0, dst_len=len(c.s) + 16) == w, c[:3]
        assert F.lit_size(c.p, c.s) == len(w)
        lit = Q.read_literal(w, 0, c.p)
        assert (lit["huffman"], lit["end"]) == (c.huff, len(w))
    assert [c.hdr for c in F.big_cases()] == [4, 4, 5, 5]
    assert [c.kind for c in F.big_cases()] == ["shorter", "equal"] * 2


@pytest.mark.parametrize("name", NAMES + ["big_p5"])
def test_batches_reach_their_paths(name):
    """2: the model on every batch, full and lean, at every padding"""
    b = F.big_batch() if name == "big_p5" else F.batches()[name]
    want, oo = b.want(b.p)
    assert int(oo[b.fixture_tiles()[0] * L.TS]) % 4 == 0
    fixture = {ti: lanes for ti, _, lanes in b.tiles}
    assert sorted(fixture) == list(range(2, 2 + len(fixture)))
    assert len(b.strings) == L.TS * (4 + len(fixture))
    for pad in F.PADS if name != "big_p5" else (0,):
        for lean in (False, True):
            info = b.model(pad, lean)
            for j, t in enumerate(info):
                if j in fixture:
                    assert F.expect(b.path, t, fixture[j], lean) is None, \
                        (name, pad, lean, j, F.expect(b.path, t, fixture[j],
                                                      lean))
                    assert t["total"] % 4 == 0
                else:
                    assert t["staged"] and t["path"] == "fast", (pad, lean, j)
    # every case where the batch says, framed as test 1 has it
    raw = want.tobytes()
    for ti, lead, lanes in b.tiles:
        for lane, c in lanes:
            i = ti * L.TS + lane
            assert b.strings[i] is c.s and c.p == b.p
            assert raw[oo[i]:oo[i + 1]] == framed(c)
        assert b.strings[ti * L.TS:ti * L.TS + lead] == [b""] * lead


@pytest.mark.parametrize("path", list(F.PATHS))
def test_every_case_at_every_start_residue(path):
    """3: per path, (prefix, length, kind, residue of the first byte) over
    the batches behind it is the whole product for the lengths the path
    holds; the other lengths are named with their reason"""
    names, lean = F.BEHIND[path]
    got = set()
    for n in names:
        for p in F.PREFIXES:
            b = F.batches()["%s_p%d" % (n, p)]
            # (the batch is on this path: test 2, with this `lean`)
            got |= set(b.reached())
    full = {(p, n, kind, r) for p in F.PREFIXES for n in F.holds(path, p)
            for kind in F.KINDS for r in range(4)}
    assert got == full, sorted(full - got)[:5]
    held = {n for p in F.PREFIXES for n in F.holds(path, p)}
    left = {n for p in F.PREFIXES for n, _ in F.lengths(p)} - held
    assert left and F.PATHS[path][2]             # (named, with a reason)
    if path == "g":
        b = F.big_batch()
        assert sorted(x[:3] for x in b.reached()) \
            == sorted(c[:3] for c in F.big_cases()) and F.BIG_NOTE


# ---- the encode_wire batches -------------------------------------------------------

def int_only(nbytes):
    """an item of nbytes bytes without a literal (8-bit prefix)"""
    return [item(), item(0, 8), item(255, 8), item(255 + 128, 8)][nbytes]


def ordinary_items(rng, n):
    """integers on both sides of every boundary on every prefix width, each
    with a short literal behind it: tiles of the dense path (put_int into
    the out stage, for the integer and through emit_prefix)"""
    strs, its = [], []
    for i in range(n):
        ib = 1 + i % 8
        m = (1 << ib) - 1
        v = (m - 1, m, m + 127, m + 128, m + 16383, m + 16384)[(i // 8) % 6]
        sb = (3, 5, 7)[i % 3]
        its.append(item(v, ib, 0, sb, allowed_first(sb) if i & 1 else 0))
        strs.append(F._tokens(rng, rng.randint(8, 40)))
    return strs, its


def _tuned(strs, its):
    """an integer-only item appended that makes the output a multiple of 4"""
    total = WireBatch(strs, its).total
    return strs + [b""], its + [int_only(-total % 4)]


@functools.lru_cache(maxsize=None)
def wire_batch(p):
    """two ordinary tiles, one tile per (kind, r) with the two 16 KB cases,
    each behind an integer of three and four bytes in its own item and
    behind an integer-only item of r bytes, two ordinary tiles -> (Batch,
    [(item index, case, bytes of integer in front)])"""
    rng = random.Random(70 + p)
    first = allowed_first(p)
    strs, its = ordinary_items(rng, 2 * L.TS - 1)
    strs, its = _tuned(strs, its)
    where = []
    for kind in F.KINDS:
        c1, c2 = F.group(p, kind, True)
        mid = [F._tokens(rng, rng.randint(8, 40)) for _ in range(2)]
        for r in range(4):
            t0 = len(strs)
            ts = [b"", c1.s] + mid + [c2.s]
            ti = [int_only(r), item(15 + 128, 4, 0x50, p, first),
                  item(str_bits=7), item(9, 6, 0x80),
                  item(7 + 16384, 3, 0x08, p, first)]
            where += [(t0 + 1, c1, 3), (t0 + 4, c2, 4)]
            ts, ti = _tuned(ts, ti)
            fill = L.TS - len(ts)
            strs += ts + [b""] * fill
            its += ti + [item()] * fill
    s2, i2 = ordinary_items(rng, 2 * L.TS)
    return WireBatch(strs + s2, its + i2), where


@pytest.mark.parametrize("p", F.PREFIXES)
def test_wire_batches(p):
    """the 16 KB literals of encode_wire: out-of-line tiles between dense
    ones, each literal behind an integer, on every start residue"""
    b, where = wire_batch(p)
    tiles = b.n // L.TS
    assert b.paths(0) == ["dense"] * 2 + ["in"] * (tiles - 4) + ["dense"] * 2
    got = set()
    for i, c, ilen in where:
        it = b.items[i]
        assert len(Q.enc_int(it.int_first, it.ival, it.int_bits)) == ilen
        assert b.want[i][ilen:] == framed(c, allowed_first(p))
        got.add((c.L, c.kind, (int(b.want_off[i]) + ilen) % 4))
    assert got == {(n, k, r) for n in F.holds("g", p) for k in F.KINDS
                   for r in range(4)}
    # the dense tiles' integers: every boundary on every prefix width
    seen = {(it.int_bits, len(Q.enc_int(0, it.ival, it.int_bits)))
            for it in b.items[:L.TS]}
    assert seen >= {(ib, k) for ib in range(1, 9) for k in (1, 2, 3, 4)}


WIRE_PATHS = ("in", "out", "lane")       # encode_wire's tiles off the dense path
CYCLE = 48                               # ordinary_items: 8 widths x 6 values


def _forced_tile(rng, path, r):
    """one tile on `path`: an integer-only item of r bytes, ordinary_items'
    whole cycle, what forces the path, the tuner, nothing up to 64"""
    strs, its = ordinary_items(rng, CYCLE)
    if path == "in":
        # one string that passes the stage alone: every item from global memory
        strs.append(F._tokens(rng, 3100))
        its.append(item(str_bits=7))
    elif path == "out":
        # raw literals: 2880 bytes and their headers, 120 bytes of integers
        # (staged: 2976 bytes of input and at most 30 around them)
        strs = [F._raw(rng, 60) for _ in its]
        strs += [F._tokens(rng, 16) for _ in range(6)]
        its += [item(str_bits=7)] * 6
    else:
        # 24 strings of 40 30-bit codes: 28800 dense bits of the 24640
        strs = [bytes(rng.choice(L.B30) for _ in range(40)) if i & 1 else s
                for i, s in enumerate(strs)]
    strs, its = _tuned([b""] + strs, [int_only(r)] + its)
    fill = L.TS - len(strs)
    return strs + [b""] * fill, its + [item()] * fill


@functools.lru_cache(maxsize=None)
def wire_path_batch(r):
    """a dense tile, one tile on each of WIRE_PATHS with every integer of the
    cycle r bytes past a dword of the output, a dense tile -> Batch"""
    rng = random.Random(170 + r)
    strs, its = _tuned(*ordinary_items(rng, L.TS - 1))
    for path in WIRE_PATHS:
        s, i = _forced_tile(rng, path, r)
        strs, its = strs + s, its + i
    s2, i2 = ordinary_items(rng, L.TS)
    return WireBatch(strs + s2, its + i2)


@pytest.mark.parametrize("r", range(4))
def test_wire_path_batches(r):
    """every integer boundary on every prefix width on each encode_wire path
    off the dense one, at output residue r"""
    b = wire_path_batch(r)
    assert b.n == 5 * L.TS
    for res in range(16):
        assert b.paths(res) == ["dense"] + list(WIRE_PATHS) + ["dense"], res
    full = {(ib, k) for ib in range(1, 9) for k in (1, 2, 3, 4)}
    for j, path in enumerate(WIRE_PATHS, 1):
        t0 = j * L.TS
        assert int(b.want_off[t0]) % 4 == 0 and len(b.want[t0]) == r
        cyc = b.items[t0 + 1:t0 + 1 + CYCLE]
        seen = {(it.int_bits, len(Q.enc_int(0, it.ival, it.int_bits)))
                for it in cyc}
        assert seen >= full, (path, sorted(full - seen))
        assert {it.str_bits for it in cyc} == set(F.PREFIXES)
        assert int(b.want_off[t0 + 1]) % 4 == r


# ---- GPU ---------------------------------------------------------------------------

def gpu_encode(c, b, pad, mode):
    torch = _torch()
    d, o = to_dev(b.data, b.off, b.pad + pad)
    out, out_off = c.encode(d, o, mode)
    torch.cuda.synchronize()
    assert c.device_error() == 0
    g_off = out_off.cpu().numpy().view(np.uint32)
    return out, out[:int(g_off[-1])].cpu().numpy(), g_off


def check(b, mode, g_out, g_off, what):
    o_out, o_off = b.want(mode)
    assert np.array_equal(g_off, o_off), (b, mode, what)
    assert np.array_equal(g_out, o_out), (b, mode, what)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_encode_batch(vcodec, name):
    """qhuff_encode_batch on each kernel variant, with 0, 3 and 5 more bytes
    in front of the input; mode 0, which has no header, as the control"""
    b = F.batches()[name]
    for pad in F.PADS:
        _, g_out, g_off = gpu_encode(vcodec, b, pad, b.p)
        check(b, b.p, g_out, g_off, pad)
    _, g_out, g_off = gpu_encode(vcodec, b, 0, 0)
    check(b, 0, g_out, g_off, "control")
    assert [int(x) for x in np.diff(g_off.astype(np.int64))] \
        == [(L.code_bits(s) + 7) // 8 for s in b.strings]


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_encode_batch_host(codec, name):
    """qhuff_encode_batch_host, through the pinned stage and with the
    caller's buffers registered"""
    b = F.batches()[name]
    n = len(b.off) - 1
    out, oo = codec.encode_host(b.data, b.off, b.p)
    check(b, b.p, out, oo, "staged")
    e = np.zeros(qhuff.encode_bound(int(b.off[-1]), n, b.p), dtype=np.uint8)
    eo = np.zeros(n + 1, dtype=np.uint32)
    with qhuff.registered(b.data, b.off, e, eo):
        out, oo = codec.encode_host(b.data, b.off, b.p, out=e, out_off=eo)
    check(b, b.p, out, oo, "registered")
    assert codec.device_error() == 0


@pytest.fixture(scope="module")
def two_codecs():
    _torch()
    cs = [qhuff.Codec(0) for _ in range(2)]
    yield cs
    for c in cs:
        c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_encode_batch_host_multi(two_codecs, name):
    """two contexts, the cut inside the fixture tiles: the second shard's
    tiles are other groups of 64 strings than the batch's"""
    b = F.batches()[name]
    cut = int(qhuff.shard_cuts(b.off, 2)[1])
    ft = b.fixture_tiles()
    assert ft[0] * L.TS < cut < (ft[-1] + 1) * L.TS
    out, oo = qhuff.encode_host_multi(two_codecs, b.data, b.off, b.p)
    check(b, b.p, out, oo, cut)
    for c in two_codecs:
        assert c.device_error() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_service_one_tile_a_call(svc, name):
    """qhuff_svc_encode: each fixture tile a call of its own, served by the
    resident kernel (none of them by the host path)"""
    b = F.batches()[name]
    host0 = svc.svc.stats()[2]
    for ti in b.fixture_tiles():
        data, off = b.tile_call(ti)
        assert int(off[-1]) <= L.SVC_MAX_BYTES
        check_enc(svc, data, off, b.p, O.encode_batch(data, off, b.p),
                  (name, ti))
    assert svc.svc.stats()[2] == host0


@pytest.mark.gpu
@pytest.mark.parametrize("p", F.PREFIXES)
def test_encode_wire_long_literals(codec, p):
    """qhuff_encode_wire and its host form: literals of mask + 16383 and
    mask + 16384 bytes with instruction bits on their first byte, behind an
    integer, on every start residue"""
    b, where = wire_batch(p)
    out, oo = check_both(codec, b)
    for i, c, ilen in where:
        assert out[oo[i] + ilen:oo[i + 1]] == framed(c, allowed_first(p))


@pytest.mark.gpu
@pytest.mark.parametrize("r", range(4))
def test_encode_wire_integers_off_the_dense_path(codec, r):
    """qhuff_encode_wire and its host form: the integers of the cycle on the
    tiles coded out of line (from global memory, from the stage) and on the
    tile packed item per lane, on every start residue"""
    check_both(codec, wire_path_batch(r))


@pytest.mark.gpu
def test_two_megabyte_strings(codec):
    """the header's fifth byte: payloads of 31 + 2^21 - 1 and 31 + 2^21
    bytes, Huffman and the tie, one device launch and one host call"""
    b = F.big_batch()
    t0 = time.perf_counter()
    _, g_out, g_off = gpu_encode(codec, b, 0, 5)
    check(b, 5, g_out, g_off, "device")
    out, oo = codec.encode_host(b.data, b.off, 5)
    check(b, 5, out, oo, "host")
    print("two_megabyte_strings: %.2f s" % (time.perf_counter() - t0))
    raw = out.tobytes()
    (ti, _, lanes), = b.tiles
    for lane, c in lanes:
        i = ti * L.TS + lane
        assert raw[oo[i]:oo[i] + c.hdr] == Q.enc_int(c.huff << 5, c.L, 5)
        assert int(oo[i + 1]) - int(oo[i]) == c.hdr + c.L


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_read_back(codec, name):
    """every literal of the encoder's output cut by read_literal and decoded
    in place by qhuff_decode_wire: the strings again, status 0"""
    torch = _torch()
    b = F.batches()[name]
    out, g_out, g_off = gpu_encode(codec, b, 0, b.p)
    wire = g_out.tobytes()
    lits = []
    for i in range(len(b.strings)):
        a = int(g_off[i])
        lit = Q.read_literal(wire, a, b.p)
        assert lit["end"] == int(g_off[i + 1])
        hdr = lit["end"] - a - len(lit["payload"])
        lits.append(qhuff.Literal(a + hdr, len(lit["payload"]), lit["huffman"],
                                  b.p, qhuff.LIT_VALUE, hdr, a))
    assert qhuff.literals_check(lits) == (qhuff.OK, None)
    if b.path == "g":
        walked = [l.len for l in lits if l.huffman and l.len > L.STAGE]
        mask = (1 << b.p) - 1
        assert sorted(set(walked)) == [mask + 16383, mask + 16384]
        assert len(walked) == 8
    dec, doo, st = codec.decode_wire(
        out, torch.from_numpy(qhuff.literals_array(lits)).cuda(),
        qhuff.MAX_STRLEN, bound=qhuff.literals_bound(lits))
    torch.cuda.synchronize()
    assert codec.device_error() == 0
    assert not st.cpu().numpy().any()
    assert np.array_equal(doo.cpu().numpy().view(np.uint32), b.off)
    assert np.array_equal(dec[:int(b.off[-1])].cpu().numpy(), b.data)
