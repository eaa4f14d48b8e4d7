"""The layout model where the path trace needs it (CPU): the lean kernels'
classification, the cooperative decode's expected fail mask and rounds per
tile, and the model written as a trace record (limits.classify(lean=True),
coop_expect, trace_expect / trace_expect_enc, trace_records).
tests/test_path_trace.py holds the kernels' own records against these on the
GPU."""
import numpy as np
import pytest

import _paths  # noqa: F401
import limits as L
import oracle_lib as O
from test_limits import dec_case, enc_case


def lean_dec(f, r):
    data, off, pad, ti, (o_out, o_off, o_st), full = dec_case(f, r)
    sizes = np.diff(o_off.astype(np.int64))
    return full, L.classify(off.astype(np.int64) + pad, 0, sizes, lean=True), ti


def lean_enc(f, r, mode):
    data, off, pad, ti, (o_out, o_off), full = enc_case(f, r, mode)
    sizes = np.diff(o_off.astype(np.int64))
    lean = L.classify_enc(bytes(pad) + data.tobytes(),
                          off.astype(np.int64) + pad, 0, mode, sizes, lean=True)
    return full, lean, ti


@pytest.mark.parametrize("f", L.DECODE, ids=repr)
def test_lean_decode_classification(f):
    """The lean decode kernel on every decode fixture: fast iff staged and
    the output <= 3008, otherwise slow; nothing for the whole wave, no slot,
    no unit off the stage; a staged tile's arena as in the full kernel."""
    for r in f.residues:
        full, lean, ti = lean_dec(f, r)
        assert len(full) == len(lean) == 5
        for j, (a, b) in enumerate(zip(full, lean)):
            assert b["staged"] == a["staged"] and b["total"] == a["total"]
            want = "fast" if a["staged"] and a["total"] <= 3008 else "slow"
            assert b["path"] == want, (f, r, j)
            assert L.k_coop(b) == () and b["copy_out"] == []
            assert len(b["units"]) == (1 if a["staged"] else 0)
            if a["staged"]:
                assert L.k_arena(b) == L.k_arena(a)
            if j != ti:
                assert b == a                # an ordinary tile: both alike
        # where the full kernel needs a slot or the wave, the lean one does not
        # leave the out stage less often: fast there implies fast or slot here
        if lean[ti]["path"] == "fast":
            assert full[ti]["path"] in ("fast", "slot")
    D = L.DECODE_BY_NAME
    assert lean_dec(D["out3008"], 0)[1][2]["path"] == "fast"
    assert lean_dec(D["out3009"], 0)[1][2]["path"] == "slow"
    assert lean_dec(D["coop129"], 0)[1][2]["path"] == "fast"
    assert lean_dec(D["arena_full"], 0)[1][2]["path"] == "slow"


@pytest.mark.parametrize("f", L.ENCODE, ids=repr)
def test_lean_encode_classification(f):
    for r in f.residues:
        for mode in (0, 7):
            full, lean, ti = lean_enc(f, r, mode)
            for j, (a, b) in enumerate(zip(full, lean)):
                want = "fast" if a["staged"] and a["total"] <= 3008 else "slow"
                assert (b["staged"], b["path"]) == (a["staged"], want)
                assert b["coop"] == [] and len(b["units"]) == int(a["staged"])
                if a["staged"]:
                    assert b["dense"] == a["dense"]
                    assert b["units"][0]["dense"] == a["dense"]
    E = L.ENCODE_BY_NAME
    assert lean_enc(E["enc_out3008"], 0, 0)[1][2]["path"] == "fast"
    assert lean_enc(E["enc_out3009"], 0, 0)[1][2]["path"] == "slow"
    assert lean_enc(E["enc_coop1024_1025"], 0, 0)[1][2]["path"] == "fast"


@pytest.mark.parametrize("f", [f for f in L.DECODE
                               if f.name.startswith(("coop63", "coop_k"))
                               and f.key is not None], ids=repr)
def test_coop_expect_reproduces_the_fixture_rounds(f):
    """coop_expect on the fixtures of test_coop_fixture_rounds: no fails,
    the unit's S, and the largest of its strings' rounds -- 60..64 for the
    periodic strings in 63 segments, at most 4 for the random ones."""
    info = dec_case(f, f.residues[0])[5][2]
    u = info["units"][0]
    fail, S, rounds = L.coop_expect(f.tile, info)
    each = [L.coop_model(f.tile[i], u["S"]) for i in f.special]
    assert fail == 0 and S == u["S"]
    assert rounds == max(r[1] for r in each)
    if f.name.startswith("coop63"):
        assert S == 8 * len(f.tile[f.special[0]]) // 63
        assert rounds <= 4 if "rand" in f.name else 60 <= rounds <= 64
    else:
        assert rounds <= 64


@pytest.mark.parametrize("f", [f for f in L.DECODE if f.key is None], ids=repr)
def test_coop_expect_fails_exactly_the_invalid_lanes(f):
    """Every *_invalid fixture: the model hands back exactly the invalid
    strings among the cooperative ones, and no other."""
    info = dec_case(f, f.residues[0])[5][2]
    coop = set(L.k_coop(info))
    fail, S, rounds = L.coop_expect(f.tile, info)
    assert fail == L._mask(i for i in f.special if i in coop), f
    if f.name.startswith(("coop129", "coop63")):
        assert coop and fail and S is not None
        # the rounds of a rejected string count: B is over before W rejects
        twin = L.DECODE_BY_NAME[f.name[:-len("_invalid")]]
        ti = dec_case(twin, twin.residues[0])[5][2]
        if f.name.startswith("coop63"):
            assert rounds == L.coop_expect(twin.tile, ti)[2] >= 60
    else:
        assert not coop and fail == 0 and S is None and rounds is None


def test_trace_expect_on_the_twins():
    """The model as a record tells the two sides of every edge apart."""
    D = L.DECODE_BY_NAME

    def rec(name, r=0, lean=False):
        f = D[name]
        full, ln, ti = lean_dec(f, r)
        return L.trace_expect(f.tile, (ln if lean else full)[ti])
    assert (rec("fix66")["var"], rec("var67")["var"]) == (0, 1)
    assert (rec("out3008")["path"], rec("out3009")["path"]) == ("fast", "slot")
    assert rec("coop128")["coop"] == 0
    assert rec("coop129")["coop"] == (1 << 31) | (1 << 32)
    assert rec("coop129")["path"] == "slot" and rec("coop129")["fail"] == 0
    assert (rec("slot12288")["path"], rec("slot12289")["path"]) == ("slot", "slow")
    assert rec("slot12288")["units"] >= 3 and not rec("slot12288")["staged"]
    for a, b in (("glob7679_lane0", "glob7680_lane0"),
                 ("glob7679_lane63_run1", "glob7679_lane63_run2")):
        assert (rec(a)["path"], rec(b)["path"]) == ("slot", "slow")
        assert rec(a)["lone"] == rec(b)["lone"] == 1
    a0, a5 = rec("arena_full", 0), rec("arena_full", 5)
    assert (a0["staged"], a0["units"], a0["var"]) == (True, 1, 1)
    assert (a5["staged"], a5["units"], a5["lone"]) == (False, 2, 0)
    c23 = rec("coop23")
    assert bin(c23["coop"]).count("1") == 23 and c23["S"] == 608
    assert c23["fail"] == 0
    lean = rec("coop129", lean=True)
    assert (lean["coop"], lean["S"], lean["path"]) == (0, None, "fast")
    E = L.ENCODE_BY_NAME

    def erec(name, mode, r=0):
        f = E[name]
        return L.trace_expect_enc(enc_case(f, r, mode)[5][2])
    for mode, path in ((0, "slot"), (7, "fast")):
        got = [erec("enc_dense%d_mode%d" % (b, mode), mode)
               for b in (24512, 24513, 24576, 24577)]
        assert [g["dense"] for g in got] == [1, 1, 1, 0]
        assert all(g["path"] == path and g["units"] == 1 for g in got)
    assert erec("enc_coop1024_1025", 0)["enc_coop"] == 1 << 41


def test_trace_records_layout():
    """trace_records() against the record's layout (qhuff_device.h
    PathTrace): one word set by hand per field."""
    w = np.zeros(2 * L.TRACE_WORDS, dtype=np.uint64)
    w[0] = 1 | 2 | (2 << 2)
    w[1] = 3 | (1 << 16) | (2 << 32) | (4 << 48)
    w[2], w[3] = (1 << 63) | 5, 1 << 40
    w[4] = 608 | (61 << 32) | (1 << 63)
    w[5] = 1 << 41
    w[8] = 1 | (3 << 2)
    a, b = L.trace_records(w)
    assert a == {"written": 1, "staged": True, "path": "slot", "units": 3,
                 "lone": 1, "var": 2, "dense": 4, "coop": (1 << 63) | 5,
                 "fail": 1 << 40, "S": 608, "rounds": 61, "enc_coop": 1 << 41}
    assert (b["staged"], b["path"], b["S"], b["rounds"]) == (False, "slow",
                                                             None, None)
    assert O.OK == 0


@pytest.mark.parametrize("kind", ["decode", "encode"])
def test_tile_paths_agree_with_classify(kind):
    """qhuff.workload.tile_paths (the shares bench.py prints) and
    limits.classify / classify_enc are two restatements of the same kernel
    rules: equal on every tile of the combined limits batches, big tiles
    with cooperative strings or whole-wave copies in their units included."""
    from qhuff import workload as W
    from test_limits import combined_case
    data, off, where, want, info = combined_case(kind)
    if kind == "decode":
        p = W.tile_paths(want[0], want[1], off)
        fast = [t["staged"] and t["total"] <= L.OUT_FAST for t in info]
        assert list(p["dec_staged"]) == [t["staged"] for t in info]
        assert list(p["dec_fast"]) == fast
        assert list(p["coop"]) == [bool(L.k_coop(t)) for t in info]
        assert list(p["var_arena"]) == [
            f and t["units"][0]["arena"] == "var" for f, t in zip(fast, info)]
        assert sum(p["coop"] & ~p["dec_staged"]) == 0   # (none in units here)
    else:
        p = W.tile_paths(data, off, want[1])
        fast = [t["path"] == "fast" for t in info]
        assert list(p["enc_staged"]) == [t["staged"] for t in info]
        assert list(p["enc_fast"]) == fast
        assert list(p["dense"]) == [f and t["dense"] for f, t in zip(fast, info)]
        assert list(p["enc_coop"]) == [bool(t["coop"]) for t in info]
    assert any(fast) and not all(fast)


def test_tile_paths_count_the_units_of_big_tiles():
    """a tile past the stage whose units hold a string for the whole wave
    (decode) or a payload the wave copies (encode) counts as cooperative;
    one whose long string alone passes the stage does not"""
    from qhuff import workload as W
    short = [b"x" * 10] * 31
    big = short + [b"ab" * 150] + short + [b"e" * 2600]      # two units
    lone = [b"x" * 10] * 63 + [b"q" * 5000]
    data, off = W.pack(big + lone)
    h, ho = O.encode_batch(data, off, 0)
    p = W.tile_paths(data, off, ho)
    assert list(p["enc_staged"]) == [False, False]
    assert list(p["enc_coop"]) == [True, False]
    assert list(p["dec_staged"]) == [True, False]
    info = L.classify_enc(data.tobytes(), off, 0, 0, np.diff(ho.astype(np.int64)))
    assert [bool(t["coop"]) for t in info] == [True, False]
    # decode: the 5000 'q' (6-bit codes: 3750 bytes) alone passes the stage
    assert list(p["coop"]) == [True, False]
    dinfo = L.classify(ho, 0, np.diff(off.astype(np.int64)))
    assert [bool(L.k_coop(t)) for t in dinfo] == [True, False]
