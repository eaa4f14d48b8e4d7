"""The resident service (qhuff_svc_*, qhuff_service.hip) at its piece cuts and
on its own tile paths (limits.py: svc_pieces, classify_svc, SVC_DECODE,
SVC_ENCODE).

The service runs the batch kernels' policies in combinations no batch kernel
executes: a tile loop of its own with no big-tile slot behind it, the
cooperative decode followed by DecPolicyT::emit or by dec_slow_tile from the
stage, a host cutter in front of it and copy2 around the one string that
passes the stage.

CPU part: the cutter's transcription against the library's own
(qhuff_svc_pieces), and every fixture -- the batch kernels' DECODE / ENCODE
tiles and the SVC_* calls -- on the path it is named for under the service
model.  GPU part: every fixture as a call of its own, the one-piece tiles
grouped 16 to a call (more pieces than slots), the edge twins after fillers
that leave every slot, scratch area and LDS region full of another request's
bytes, and decode against encode from two threads; all bit-exact against the
oracle (bytes, out_off, status), on a Codec and a Service of the file's own
so that the service's counters are this file's."""
import ctypes as C
import random
import threading

import numpy as np
import pytest

import _paths  # noqa: F401
import limits as L
import oracle_lib as O
import qhuff

MODES = (0, 3, 5, 7)

# ---- the calls and their oracle results, built once ------------------------------

_dec, _enc = {}, {}


def strings_of(f):
    return f.tile if isinstance(f, L.Fixture) else f.strings


def dec_call(f):
    """(data, off, (out, out_off, status) of the oracle, classify_svc)"""
    if f.name not in _dec:
        data, off = L.pack(strings_of(f))
        want = O.decode_batch(data, off)
        info = L.classify_svc(off, np.diff(want[1].astype(np.int64)))
        _dec[f.name] = (data, off, want, info)
    return _dec[f.name]


def enc_call(f, mode):
    """(data, off, (out, out_off) of the oracle, classify_svc_enc)"""
    k = (f.name, mode)
    if k not in _enc:
        data, off = L.pack(strings_of(f))
        want = O.encode_batch(data, off, mode)
        info = L.classify_svc_enc(data, off, mode,
                                  np.diff(want[1].astype(np.int64)))
        _enc[k] = (data, off, want, info)
    return _enc[k]


ALL_DECODE = L.DECODE + L.SVC_DECODE
ALL_ENCODE = L.ENCODE + L.SVC_ENCODE


def one_piece(f):
    """a tile the cutter leaves whole: 64 strings within 3072 bytes"""
    s = strings_of(f)
    return len(s) == L.TS and sum(map(len, s)) <= L.STAGE


DEC_TILES = [f for f in ALL_DECODE if one_piece(f)]
ENC_TILES = [f for f in ALL_ENCODE if one_piece(f)]


# ---- CPU: the cutter ---------------------------------------------------------------

def lib_pieces(off, max_pieces=None):
    """(rc, cuts, n_pieces) of qhuff_svc_pieces, called raw"""
    off = np.ascontiguousarray(off, dtype=np.uint32)
    n = len(off) - 1
    if max_pieces is None:
        max_pieces = max(n, 1)
    cuts = np.full(max_pieces + 2, 0xdeadbeef, dtype=np.uint32)
    k = C.c_uint32(12345)
    rc = qhuff.lib().qhuff_svc_pieces(off.ctypes.data_as(C.c_void_p), n,
                                      cuts.ctypes.data_as(C.c_void_p),
                                      max_pieces, C.byref(k))
    assert cuts[max_pieces + 1] == 0xdeadbeef    # max_pieces + 1 entries
    return rc, [int(x) for x in cuts[:max_pieces + 1]], k.value


def same_cuts(off):
    want = L.svc_pieces(off)
    rc, cuts, k = lib_pieces(off)
    assert rc == qhuff.OK
    if want is None:
        assert k == 0
        assert qhuff.svc_pieces(off) == [0]
        return None
    assert k == len(want) - 1 and cuts[:k + 1] == want, (want, cuts[:k + 1])
    assert qhuff.svc_pieces(off) == want
    # every piece: at most 64 strings within 3072 bytes, or one string
    o = [int(x) for x in off]
    for a, b in zip(want, want[1:]):
        assert a < b <= a + L.TS
        assert o[b] - o[a] <= L.STAGE or b == a + 1
    return want


@pytest.mark.parametrize("f", ALL_DECODE + ALL_ENCODE, ids=repr)
def test_pieces_of_the_fixtures(f):
    data, off = L.pack(strings_of(f))
    cuts = same_cuts(off)
    assert cuts is not None
    # the cutter reads differences only: the same cuts behind other strings
    assert L.svc_pieces(off + np.uint32(7777)) == cuts
    assert lib_pieces(off + np.uint32(7777))[1][:len(cuts)] == cuts


def test_pieces_of_the_cut_cases():
    """the issue's cut cases, as offsets alone"""
    def cuts_of(lens):
        off = np.zeros(len(lens) + 1, dtype=np.uint32)
        np.cumsum(lens, out=off[1:])
        return same_cuts(off)
    assert cuts_of([64] * 48 + [10]) == [0, 48, 49]            # 3072 | 10
    assert cuts_of([64] * 47 + [65, 10]) == [0, 47, 49]        # 3008 | 75
    assert cuts_of([3] * 65) == [0, 64, 65]
    assert cuts_of([0] * 64 + [5]) == [0, 64, 65]
    assert cuts_of([3072] + [0] * 70) == [0, 64, 71]
    assert cuts_of([3073] + [0] * 70) == [0, 1, 65, 71]
    assert cuts_of([0] * 70) == [0, 64, 70]
    assert cuts_of([0]) == [0, 1]
    assert cuts_of([3072]) == [0, 1] and cuts_of([3073]) == [0, 1]
    assert cuts_of([1, 3072]) == [0, 1, 2]
    assert cuts_of([0, 3072]) == [0, 2]
    assert cuts_of([65536]) == [0, 1]
    assert cuts_of([3073, 3073, 1]) == [0, 1, 2, 3]
    assert cuts_of([48] * 64) == [0, 64] and cuts_of([48] * 65) == [0, 64, 65]
    assert cuts_of([49] * 64) == [0, 62, 64]                   # 3038 | 98
    assert cuts_of([64] * 1024) == [48 * i for i in range(22)] + [1024]
    assert cuts_of([]) == [0]


def test_pieces_of_random_offsets():
    """a few hundred seeded offset arrays whose lengths lie near 0, 48, 64,
    1536, 3072 and 3073"""
    rng = random.Random(3072)
    near = (0, 48, 64, 1536, 3072, 3073)
    multi = 0
    for case in range(400):
        n = rng.choice((1, 2, 3, 63, 64, 65, 66, 127, 128, 129, 200))
        big = rng.random() < 0.5
        lens, room = [], L.SVC_MAX_BYTES
        for _ in range(n):
            c = rng.choice(near if big else near[:3])
            x = max(0, c + rng.randint(-2, 2))
            if rng.random() < 0.3:
                x = 0
            x = min(x, room)
            room -= x
            lens.append(x)
        off = np.zeros(n + 1, dtype=np.uint32)
        np.cumsum(lens, out=off[1:])
        off += np.uint32(rng.choice((0, 1, 15, 4096, 1 << 31)))
        cuts = same_cuts(off)
        multi += len(cuts) > 2
    assert multi > 200


def test_pieces_errors_and_host_path():
    lib = qhuff.lib()
    assert "qhuff_svc_pieces" in qhuff.EXPORTS
    assert "#define QHUFF_FEATURE_SVC_PIECES 1" in open(qhuff.HEADER).read()
    off = np.array([0, 5, 9], dtype=np.uint32)
    cuts = np.zeros(4, dtype=np.uint32)
    k = C.c_uint32()
    p = lambda a: a.ctypes.data_as(C.c_void_p)          # noqa: E731
    assert lib.qhuff_svc_pieces(None, 2, p(cuts), 2, C.byref(k)) == qhuff.EINVAL
    assert lib.qhuff_svc_pieces(p(off), 2, None, 2, C.byref(k)) == qhuff.EINVAL
    assert lib.qhuff_svc_pieces(p(off), 2, p(cuts), 2, None) == qhuff.EINVAL
    # decreasing offsets, anywhere
    assert lib_pieces([0, 5, 3])[0] == qhuff.EINVAL
    assert lib_pieces([5, 3])[0] == qhuff.EINVAL
    assert lib_pieces([0] * 70 + [9, 8])[0] == qhuff.EINVAL
    with pytest.raises(qhuff.QhuffError):
        qhuff.svc_pieces([0, 5, 3])
    # more pieces than max_pieces: the count needed, the first cuts
    lens = [64] * 48 * 3 + [1]
    off = np.zeros(len(lens) + 1, dtype=np.uint32)
    np.cumsum(lens, out=off[1:])
    assert L.svc_pieces(off) == [0, 48, 96, 144, 145]
    for mp in (0, 1, 3):
        rc, cuts, k = lib_pieces(off, mp)
        assert rc == qhuff.ERANGE and k == 4
        assert cuts[:mp + 1] == [0, 48, 96, 144][:mp + 1]
    rc, cuts, k = lib_pieces(off, 4)
    assert rc == qhuff.OK and k == 4 and cuts == [0, 48, 96, 144, 145]
    # the host path: more strings or bytes than a slot holds
    assert lib_pieces([0] * (L.SVC_MAX_STRINGS + 1))[::2] == (qhuff.OK, 16)
    assert lib_pieces([0] * (L.SVC_MAX_STRINGS + 2))[::2] == (qhuff.OK, 0)
    assert L.svc_pieces([0] * (L.SVC_MAX_STRINGS + 2)) is None
    assert lib_pieces([0, L.SVC_MAX_BYTES])[::2] == (qhuff.OK, 1)
    assert lib_pieces([0, L.SVC_MAX_BYTES + 1])[::2] == (qhuff.OK, 0)
    assert lib_pieces([9, 9 + L.SVC_MAX_BYTES + 1], 0)[::2] == (qhuff.OK, 0)
    assert L.svc_pieces([0, L.SVC_MAX_BYTES + 1]) is None
    assert L.classify_svc([0, L.SVC_MAX_BYTES + 1], [0]) is None
    # no strings
    assert lib_pieces([0], 0) == (qhuff.OK, [0], 0)


# ---- CPU: the fixtures against the service model ----------------------------------

def model_of(f):
    if f.mode is None:
        data, off, want, info = dec_call(f)
    else:
        data, off, want, info = enc_call(f, f.mode)
    return info


@pytest.mark.parametrize("f", L.SVC_DECODE + L.SVC_ENCODE, ids=repr)
def test_svc_fixtures_reach_their_paths(f):
    """Every item of every piece the fixture names (SvcFixture.want), the
    statuses it promises, and its twin on the other side."""
    info = model_of(f)
    assert len(info) == len(f.want), (f, info)
    for p, w in zip(info, f.want):
        for k, v in w.items():
            assert p[k] == v, (f, k, p[k], v, f.edge)
        if f.mode is None and p["route"] == "direct":
            assert p["slot_end"] <= p["arena_cap"], (f, p)
        assert (p["route"] == "direct") == p["staged"]
    if f.mode is None:
        o_out, o_off, o_st = dec_call(f)[2]
        assert int(o_st.sum()) == f.bad
        if f.name.endswith("_invalid"):
            assert len(o_out) == 0
    by = L.SVC_DECODE_BY_NAME if f.mode is None else L.SVC_ENCODE_BY_NAME
    if f.twin:
        g = by[f.twin]
        assert g.twin == f.name and g.want != f.want, (f, g)
        gi = model_of(g)
        shape = lambda i: [(p["n"], p["bytes"], p["route"], p["path"],  # noqa: E731
                            p.get("passes_in"), p.get("passes_out"))
                           for p in i]
        assert shape(gi) != shape(info), (f, g)


def test_svc_fixture_arithmetic():
    """What the service fixtures' names promise, in numbers."""
    D, E = L.SVC_DECODE_BY_NAME, L.SVC_ENCODE_BY_NAME
    # copy2's pass holds 512 chunks, the chunk of offsets among them
    for size, chunks, passes in ((8176, 512, 1), (8177, 513, 2),
                                 (16368, 1024, 2), (16369, 1025, 3),
                                 (3088, 194, 1), (3089, 195, 1)):
        p = dec_call(D["svc_scr%d_maxexp" % size])[3][0]
        assert (p["copy_in"], p["passes_in"]) == (chunks, passes)
        p = enc_call(E["svc_scr%d_enc_b30" % size], 0)[3][0]
        assert (p["copy_in"], p["passes_in"]) == (chunks, passes)
    for name, case in (("svc_back%d", dec_call), ("svc_enc_back%d",
                                                  lambda f: enc_call(f, 0))):
        by = D if case is dec_call else E
        a, b = (case(by[name % k])[3][0] for k in (8192, 8193))
        assert (a["total"], a["copy_out"], a["passes_out"]) == (8192, 512, 1)
        assert (b["total"], b["copy_out"], b["passes_out"]) == (8193, 513, 2)
    assert dec_call(D["svc_back8192"])[3][0]["bytes"] == 5120
    # the worst expansions, both inside the slot's output region
    p = dec_call(D["svc_scr65536_maxexp"])[3][0]
    assert p["total"] == 104857
    p = enc_call(E["svc_scr65536_enc_b30"], 0)[3][0]
    assert p["total"] == 245760 and p["passes_out"] == 30
    # mode 7 on 30-bit codes: the raw fallback, 65536 bytes and their length
    out, oo = enc_call(E["svc_scr65536_enc_b30"], 7)[2]
    assert int(oo[1]) == 65536 + 4 and not out[0] & 0x80
    assert bytes(out[4:]) == E["svc_scr65536_enc_b30"].strings[0]
    # 3072 bytes of 30-bit codes: 92160 code bits, not dense, 11520 bytes
    p = enc_call(E["svc_one3072_enc_b30"], 0)[3][0]
    assert (p["se"], p["dense"], p["total"]) == (92160, False, 11520)
    # the cooperative twins: 130 bytes in lane 17, well inside the stage
    for name, total in (("svc_coop_out3008", 3008), ("svc_coop_out3009", 3009)):
        p = dec_call(D[name])[3][0]
        assert p["total"] == total and p["bytes"] < 2048
        assert p["arena"] == "var" and p["segs"] == (16,) and p["S"] == 64
    # one string of 3072 bytes: 24576 bits over 64 - 1 lanes are 391, so
    # S = 416 (a multiple of 32) and 24576 // 416 = 59 segments
    p = dec_call(D["svc_one3072_ssi"])[3][0]
    assert p["S"] == 416 and p["segs"] == (59,)


def test_batch_fixtures_under_the_service():
    """The batch kernels' fixtures (limits.DECODE / ENCODE) as service calls:
    where each one lands under the service model, by name."""
    D, E = L.DECODE_BY_NAME, L.ENCODE_BY_NAME

    def dec1(name):
        info = dec_call(D[name])[3]
        assert len(info) == 1 and info[0]["route"] == "direct", name
        assert info[0]["n"] == 64 and info[0]["staged"]
        return info[0]

    def enc1(name, mode=None):
        f = E[name]
        info = enc_call(f, f.mode if mode is None else mode)[3]
        assert len(info) == 1 and info[0]["route"] == "direct", name
        return info[0]

    p = dec1("coop129")
    assert p["path"] == "fast" and p["coop"] == (31, 32)
    assert dec1("coop128")["coop"] == () and dec1("coop128")["path"] == "fast"
    seen = {"c504": 0, "c3024": 0}
    for f in L.DECODE:
        if f.key is None:
            continue
        if f.name.startswith("coop63_504"):
            # the branch of DecPolicyT::emit that only the service runs
            p = dec1(f.name)
            assert p["path"] == "fast" and p["segs"] == (63,)
            assert p["coop"] == f.special
            seen["c504"] += 1
        elif f.name.startswith(("coop63_3024", "coop_k", "coop23")):
            # dec_slow_tile from the stage, after the cooperative phase
            p = dec1(f.name)
            assert p["path"] == "slow" and p["coop"] == f.special
            assert sum(p["segs"]) <= 64
            seen["c3024"] += 1
    assert seen == {"c504": 9, "c3024": 13}
    assert dec1("coop23")["segs"] == (1,) * 23
    assert dec1("out3008")["path"] == "fast" and dec1("out3008")["total"] == 3008
    assert dec1("out3009")["path"] == "slow" and dec1("out3009")["total"] == 3009
    assert dec1("fix66")["arena"] == "fixed" and dec1("var67")["arena"] == "var"
    assert dec1("fix66")["path"] == dec1("var67")["path"] == "fast"
    p = dec1("arena_full")
    assert p["bytes"] == L.STAGE and p["path"] == "slow" and p["arena"] == "var"
    assert p["slot_end"] <= p["arena_cap"]
    assert dec1("copy64_65")["path"] == "slow"   # (no copy_out here: no slot)
    # an invalid cooperative string: its tile of few bytes is emitted fast
    assert dec1("coop63_3024_0_lane63_invalid")["path"] == "fast"
    for mode, path in ((0, "slow"), (7, "fast")):
        for bits, dense in ((24512, True), (24513, True), (24576, True),
                            (24577, False)):
            p = enc1("enc_dense%d_mode%d" % (bits, mode))
            assert (p["se"], p["dense"], p["path"]) == (bits, dense, path)
    assert enc1("enc_out3008")["path"] == "fast"
    assert enc1("enc_out3009")["path"] == "slow"
    p = enc1("enc_coop1024_1025")
    assert p["path"] == "fast" and p["dense"] and p["coop"] == (41,)
    # Not at an edge here -- the service has no 12288-byte slot, and a string
    # past the stage is a scratch piece whatever its bound: only the pieces
    # the cutter gives them are pinned.
    shape = lambda i: [(p["n"], p["bytes"], p["route"]) for p in i]  # noqa: E731
    for name in ("slot12288", "slot12289"):
        extra = name == "slot12289"
        assert shape(dec_call(D[name])[3]) == [
            (25, 3000, "direct"), (25, 3000, "direct"),
            (14, 1680 + extra, "direct")]
    assert shape(dec_call(D["glob7679_lane0"])[3]) == [
        (1, 7679, "scratch"), (63, 2, "direct")]
    assert shape(dec_call(D["glob7680_lane0"])[3]) == [
        (1, 7680, "scratch"), (63, 2, "direct")]
    assert shape(dec_call(D["glob7679_lane63_run1"])[3]) == [
        (63, 1, "direct"), (1, 7679, "scratch")]
    assert shape(dec_call(D["glob7679_lane63_run2"])[3]) == [
        (63, 2, "direct"), (1, 7679, "scratch")]
    for name in ("enc_slot12288", "enc_slot12289"):
        assert shape(enc_call(E[name], 0)[3]) == [(51, 3060, "direct"),
                                                  (13, 780, "direct")]
    # every other tile of the batch kernels is one direct piece
    many = {"slot12288", "slot12289", "slot12288_invalid", "enc_slot12288",
            "enc_slot12289"} | {f.name for f in L.DECODE
                                if f.name.startswith("glob")}
    assert {f.name for f in L.DECODE + L.ENCODE if not one_piece(f)} == many
    assert len(DEC_TILES) >= 36 and len(ENC_TILES) >= 11


def grouped(tiles, per_call=16):
    """the tiles' strings, 16 tiles a call -> [(strings, tiles of the call)]"""
    calls = []
    for i in range(0, len(tiles), per_call):
        part = tiles[i:i + per_call]
        calls.append(([s for f in part for s in strings_of(f)], part))
    return calls


def test_grouped_calls_are_cut_at_the_fixtures():
    """A concatenation of one-piece tiles is cut exactly at the tiles -- by
    the model and by the library -- and 16 of them are more pieces than a
    default service has slots."""
    for tiles in (DEC_TILES, ENC_TILES + ENC_TILES[:16 - len(ENC_TILES)]):
        for strs, part in grouped(tiles):
            data, off = L.pack(strs)
            want = [L.TS * i for i in range(len(part) + 1)]
            assert L.svc_pieces(off) == want == qhuff.svc_pieces(off)
    assert len(grouped(DEC_TILES)[0][1]) == 16 > L.SVC_SLOTS
    assert len(ENC_TILES) < 16 <= 2 * len(ENC_TILES)


# ---- GPU -------------------------------------------------------------------------

def _torch():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("gpu test without a GPU")
    return torch


class Counted:
    """the file's service, its calls counted"""

    def __init__(self, svc):
        self.svc, self.calls, self.mu = svc, 0, threading.Lock()
        self.stats0 = svc.stats()

    def _count(self):
        with self.mu:
            self.calls += 1

    def decode(self, data, off):
        self._count()
        return self.svc.decode(data, off)

    def encode(self, data, off, mode):
        self._count()
        return self.svc.encode(data, off, mode)


@pytest.fixture(scope="module")
def svc():
    _torch()
    c = qhuff.Codec(0)
    s = c.service()
    yield Counted(s)
    s.close()
    c.close()


def check_dec(svc, data, off, want, what):
    out, oo, st = svc.decode(data, off)
    o_out, o_off, o_st = want
    assert np.array_equal(st, o_st), what
    assert np.array_equal(oo, o_off), what
    assert np.array_equal(out, o_out), what
    return st


def check_enc(svc, data, off, mode, want, what):
    out, oo = svc.encode(data, off, mode)
    o_out, o_off = want
    assert np.array_equal(oo, o_off), (what, mode)
    assert np.array_equal(out, o_out), (what, mode)


def run_dec(svc, f):
    data, off, want, _ = dec_call(f)
    return check_dec(svc, data, off, want, f)


def run_enc(svc, f, mode):
    data, off, want, _ = enc_call(f, mode)
    check_enc(svc, data, off, mode, want, f)


@pytest.mark.gpu
@pytest.mark.parametrize("f", ALL_DECODE, ids=repr)
def test_svc_decode_fixture(svc, f):
    """each decode fixture as a call of its own"""
    st = run_dec(svc, f)
    if isinstance(f, L.Fixture):
        bad = len(f.special) if f.key is None else 0
    else:
        bad = f.bad
    assert int(st.sum()) == bad


@pytest.mark.gpu
@pytest.mark.parametrize("f", ALL_ENCODE, ids=repr)
def test_svc_encode_fixture(svc, f):
    """each encode fixture as a call of its own, in its own mode and in all
    four"""
    for mode in (f.mode,) + MODES:
        run_enc(svc, f, mode)


@pytest.mark.gpu
def test_svc_empty_pieces(svc):
    """pieces of zero bytes, through decode and every encode mode"""
    for name in ("svc_all_empty", "svc_empty64_one", "svc_3072_empties"):
        run_dec(svc, L.SVC_DECODE_BY_NAME[name])
        for mode in MODES:
            run_enc(svc, L.SVC_ENCODE_BY_NAME[name.replace("svc_", "svc_enc_")],
                    mode)


@pytest.mark.gpu
def test_svc_decode_grouped(svc):
    """the one-piece decode tiles 16 to a call: more pieces than slots, so
    several rounds, the waves of the workgroup on different paths at once"""
    for _ in range(2):
        for strs, part in grouped(DEC_TILES):
            data, off = L.pack(strs)
            assert len(qhuff.svc_pieces(off)) == len(part) + 1
            st = check_dec(svc, data, off, O.decode_batch(data, off), part)
            assert int(st.sum()) == sum(len(f.special) for f in part
                                        if f.name.endswith("_invalid"))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_svc_encode_grouped(svc, mode):
    tiles = ENC_TILES + ENC_TILES[:16 - len(ENC_TILES)]
    (strs, part), = grouped(tiles)
    data, off = L.pack(strs)
    assert len(qhuff.svc_pieces(off)) == 17
    want = O.encode_batch(data, off, mode)
    for _ in range(2):
        check_enc(svc, data, off, mode, want, part)


# the edge twins that follow a filler
STALE_DEC = ["out3008", "out3009", "svc_coop_out3008", "svc_coop_out3009",
             "fix66", "var67", "coop63_504_ssi_lane29", "coop63_3024_0_lane63",
             "svc_one3072_maxexp", "svc_one3073_maxexp",
             "svc_one3072_token_invalid", "svc_one3073_token_invalid",
             "svc_scr8176_ssi", "svc_scr8177_ssi", "svc_scr8176_maxexp_invalid",
             "svc_scr8177_maxexp_invalid"]
STALE_ENC = ["enc_out3008", "enc_out3009", "enc_dense24576_mode0",
             "enc_dense24577_mode0", "enc_dense24576_mode7",
             "enc_dense24577_mode7", "svc_one3072_enc_token",
             "svc_one3073_enc_token", "svc_one3072_enc_b30",
             "svc_one3073_enc_b30", "svc_scr8176_enc_f5", "svc_scr8177_enc_f5",
             "svc_scr8176_enc_b30", "svc_scr8177_enc_b30"]

_fill = {}


def filler(byte, size, op):
    """21 strings of `size` bytes, every byte `byte`, with the oracle's
    result: 21 pieces, so with the service idle every slot gets one"""
    k = (byte, size, op)
    if k not in _fill:
        data = np.full(21 * size, byte, dtype=np.uint8)
        off = (np.arange(22) * size).astype(np.uint32)
        assert L.svc_pieces(off) == list(range(22))
        assert len(L.svc_pieces(off)) - 1 >= L.SVC_SLOTS
        want = O.encode_batch(data, off, 0) if op == "encode" else \
            O.decode_batch(data, off)
        _fill[k] = (data, off, want)
    return _fill[k]


@pytest.mark.gpu
@pytest.mark.parametrize("byte", [0xff, 0x00], ids=["ff", "00"])
@pytest.mark.parametrize("op", ["encode", "decode"])
def test_svc_stale_state(svc, op, byte):
    """Before every edge twin a filler pair leaves all of a request's state
    full of another request's bytes: 21 strings of 3072 bytes (direct: the
    slots' input regions and, encoded through the slow path, their output
    regions) and 21 of 3073 (the scratch areas) -- as encode or as decode, so
    that a decode fixture follows an encode in the same wave's LDS union and
    the other way round.  Fillers and fixtures all equal the oracle."""
    def fill():
        for size in (3072, 3073):
            data, off, want = filler(byte, size, op)
            if op == "encode":
                check_enc(svc, data, off, 0, want, ("filler", size))
            else:
                check_dec(svc, data, off, want, ("filler", size))

    by = dict(L.DECODE_BY_NAME, **L.SVC_DECODE_BY_NAME)
    for name in STALE_DEC:
        fill()
        run_dec(svc, by[name])
    by = dict(L.ENCODE_BY_NAME, **L.SVC_ENCODE_BY_NAME)
    for name in STALE_ENC:
        fill()
        run_enc(svc, by[name], by[name].mode)


def test_stale_fillers():
    """(CPU) what the fillers are: 0xff bytes are 26-bit codes, 9984 bytes a
    string through the slow path; as Huffman input both bytes are rejected"""
    for size in (3072, 3073):
        for byte in (0xff, 0x00):
            data, off, (out, oo) = filler(byte, size, "encode")
            info = L.classify_svc_enc(data, off, 0, np.diff(oo.astype(np.int64)))
            assert len(info) == 21
            assert {p["route"] for p in info} == {
                "direct" if size == 3072 else "scratch"}
            assert {p["path"] for p in info} == {"slow"}
            st = filler(byte, size, "decode")[2][2]
            assert st.all()
    assert int(filler(0xff, 3072, "encode")[2][1][1]) == 9984
    names = set(L.DECODE_BY_NAME) | set(L.SVC_DECODE_BY_NAME) \
        | set(L.ENCODE_BY_NAME) | set(L.SVC_ENCODE_BY_NAME)
    assert set(STALE_DEC + STALE_ENC) <= names


@pytest.mark.gpu
def test_svc_decode_against_encode(svc):
    """one thread runs the decode fixtures, another the encode fixtures,
    three passes each at the same time"""
    for f in ALL_DECODE:                     # (the oracle's results first)
        dec_call(f)
    for f in ALL_ENCODE:
        enc_call(f, f.mode)
    errors = []

    def worker(run, fixtures):
        try:
            for _ in range(3):
                for f in fixtures:
                    run(f)
        except Exception as e:                      # noqa: BLE001
            errors.append(repr(e)[:400])

    th = [threading.Thread(target=worker,
                           args=(lambda f: run_dec(svc, f), ALL_DECODE)),
          threading.Thread(target=worker,
                           args=(lambda f: run_enc(svc, f, f.mode),
                                 ALL_ENCODE))]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in th)
    assert not errors, errors[:3]


@pytest.mark.gpu
def test_svc_none_took_the_host_path(svc):
    """every call of this file was served by the kernel"""
    served0, _, fb0 = svc.stats0
    served, launches, fb = svc.svc.stats()
    assert fb == fb0 == 0
    assert svc.calls > 0 and served - served0 == svc.calls
