"""Decode and encode at the exact limits of their LDS layouts (limits.py).

CPU part: every fixture reaches the path it is named for -- by the layout
model, limits.classify / classify_enc -- and its twin on the other side of
the edge is classified the other way.  GPU part: the kernels on those
fixtures, bit-exact against the oracle (bytes, out_off, status), on the
default codec and with QHUFF_KERNELS=lean / full.  Each fixture is one tile
between two ordinary tiles on either side, its first byte on the residue
(mod 16) it names; its id says which edge and side it sits on
(Fixture.edge has the words).  (A batch of five tiles is spread one tile to
a wave, so the neighbours here are neighbours in the batch, in the offsets
and in the look-back, not pending tiles of the same wave: those need a
batch of more tiles than the grid has waves, test_gpu_parity.py's sizes.)"""
import os

import numpy as np
import pytest

import _paths  # noqa: F401
import limits as L
import oracle_lib as O

# ---- the batches and their oracle results, built once --------------------------

_dec, _enc = {}, {}


def dec_case(f, residue):
    k = (f.name, residue)
    if k not in _dec:
        data, off, pad, ti = L.decode_batch_of(f, residue)
        o_out, o_off, o_st = O.decode_batch(data, off)
        sizes = np.diff(o_off.astype(np.int64))
        info = L.classify(off.astype(np.int64) + pad, 0, sizes)
        _dec[k] = (data, off, pad, ti, (o_out, o_off, o_st), info)
    return _dec[k]


def enc_case(f, residue, mode):
    k = (f.name, residue, mode)
    if k not in _enc:
        data, off, pad, ti = L.encode_batch_of(f, residue)
        o_out, o_off = O.encode_batch(data, off, mode)
        sizes = np.diff(o_off.astype(np.int64))
        info = L.classify_enc(bytes(pad) + data.tobytes(),
                              off.astype(np.int64) + pad, 0, mode, sizes)
        _enc[k] = (data, off, pad, ti, (o_out, o_off), info)
    return _enc[k]


# ---- CPU: the fixtures against the model -----------------------------------------

def _ordinary(info, ti):
    for j, t in enumerate(info):
        if j != ti:
            assert t["staged"] and t["path"] == "fast", (j, t)


@pytest.mark.parametrize("f", L.DECODE + L.ENCODE, ids=repr)
def test_fixtures_reach_their_paths(f):
    """The exact property each fixture is named for (Fixture.key / want, at
    every residue it is run at), the other side for its twin, and for every
    unit the last slot's end inside the arena."""
    dec = f.mode is None
    by_name = L.DECODE_BY_NAME if dec else L.ENCODE_BY_NAME
    for r in f.residues:
        if dec:
            data, off, pad, ti, (o_out, o_off, o_st), info = dec_case(f, r)
        else:
            data, off, pad, ti, _, info = enc_case(f, r, f.mode)
        _ordinary(info, ti)
        t = info[ti]
        if dec:
            for u in t["units"]:
                if not u["lone"]:
                    assert u["slot_end"] <= u["arena_cap"], (f, r, u)
        if f.key is None:
            # *_invalid: status 1 and size 0 on exactly the special lanes
            st = o_st[ti * L.TS:(ti + 1) * L.TS]
            sz = np.diff(o_off.astype(np.int64))[ti * L.TS:(ti + 1) * L.TS]
            assert sorted(np.nonzero(st)[0]) == sorted(f.special), f
            assert not sz[list(f.special)].any()
            assert not o_st[:ti * L.TS].any() and not o_st[(ti + 1) * L.TS:].any()
            continue
        assert f.key(t) == f.want[r], (f, r, f.key(t), f.edge)
        if f.twin:
            g = by_name[f.twin]
            assert g.twin == f.name and g.key is f.key
            gi = (dec_case(g, r) if dec else enc_case(g, r, g.mode))[5]
            assert g.key(gi[ti]) == g.want[r] != f.want[r], (f, g, r)


def test_fixture_arithmetic():
    """What the fixtures' names promise, in numbers."""
    # a 66-byte string fills 105 bytes + the emitter's 2 of its 108-byte
    # stride; a 67-byte one would not fit
    assert 8 * 66 // 5 + 2 <= L.FIX_STRIDE < 8 * 67 // 5 + 2
    D = L.DECODE_BY_NAME
    t = dec_case(D["fix66"], 0)[5][2]
    assert t["total"] == 2804 and t["path"] == "fast"
    assert dec_case(D["out3008"], 0)[5][2]["total"] == 3008
    assert dec_case(D["out3009"], 0)[5][2]["total"] == 3009
    # arena_full: span exactly 3072 at residue 0, the last slot's end two
    # bytes past its bound and still below kVarArenaBytes
    data, off, pad, ti, _, info = dec_case(D["arena_full"], 0)
    a, b = int(off[ti * 64]) + pad, int(off[ti * 64 + 64]) + pad
    assert a % 16 == 0 and b - a == L.STAGE
    u = info[ti]["units"][0]
    assert u["arena"] == "var" and u["slot_end"] == 5042 <= L.VAR_ARENA == 5059
    assert info[ti]["total"] > L.OUT_FAST
    units5 = dec_case(D["arena_full"], 5)[5][2]["units"]
    assert len(units5) == 2 and not any(u["lone"] for u in units5)
    # slot12288: several units, none lone
    for r in (0, 5):
        t = dec_case(D["slot12288"], r)[5][2]
        assert t["total"] == 12288 and len(t["units"]) >= 3
        assert dec_case(D["slot12289"], r)[5][2]["total"] == 12289
    # the string walked in global memory: run + bound on either side
    for name, run, bound in (("glob7679_lane0", 0, 12287),
                             ("glob7680_lane0", 0, 12289),
                             ("glob7679_lane63_run1", 1, 12287),
                             ("glob7679_lane63_run2", 2, 12287)):
        for r in (0, 5):
            t = dec_case(D[name], r)[5][2]
            lone = [u for u in t["units"] if u["lone"]]
            assert len(lone) == 1
            assert (lone[0]["run"], lone[0]["bound"]) == (run, bound)
            assert lone[0]["into_slot"] == (run + bound <= L.BIG_SLOT)
    assert dec_case(D["glob7679_lane0"], 0)[5][2]["total"] == 12288
    # encode
    E = L.ENCODE_BY_NAME
    assert enc_case(E["enc_out3008"], 0, 0)[5][2]["total"] == 3008
    assert enc_case(E["enc_out3009"], 0, 0)[5][2]["total"] == 3009
    for mode, path in ((0, "slot"), (7, "fast")):
        for bits in (24512, 24513, 24576, 24577):
            t = enc_case(E["enc_dense%d_mode%d" % (bits, mode)], 0, mode)[5][2]
            assert t["se"] == bits and t["path"] == path
            assert t["staged"]
    for r in (0, 5):
        assert enc_case(E["enc_slot12288"], r, 0)[5][2]["total"] == 12288
        assert enc_case(E["enc_slot12289"], r, 0)[5][2]["total"] == 12289
        assert enc_case(E["enc_coop1024_1025"], r, 0)[5][2]["path"] == "fast"


@pytest.mark.parametrize("f", [f for f in L.DECODE
                               if f.name.startswith(("coop63", "coop_k"))
                               and f.key is not None], ids=repr)
def test_coop_fixture_rounds(f):
    """The cooperative model (test_coop_model.coop_model) on the fixtures'
    long strings, with the tile's S: the oracle's bytes; 60 rounds or more
    of B for a periodic string in 63 segments (the kernel's guard is 64),
    at most 4 for a random one."""
    u = dec_case(f, f.residues[0])[5][2]["units"][0]
    for lane in f.special:
        h = f.tile[lane]
        r = L.coop_model(h, u["S"])
        assert r is not None and r[0] == O.huff_decode(h)[1]
        if f.name.startswith("coop63"):
            assert u["segs"] == [63]
            if "rand" in f.name:
                assert r[1] <= 4
            else:
                assert 60 <= r[1] <= 64
        else:
            assert r[1] <= 64


_comb = {}


def combined_case(kind):
    """limits.combined over the decode fixtures, or the mode-0 encode ones,
    with the oracle's result and the model's tiles"""
    if kind not in _comb:
        if kind == "decode":
            data, off, where = L.combined(L.DECODE)
            want = O.decode_batch(data, off)
            info = L.classify(off, 0, np.diff(want[1].astype(np.int64)))
        else:
            data, off, where = L.combined(L.ENCODE, raw=True, repeat=3)
            want = O.encode_batch(data, off, 0)
            info = L.classify_enc(data.tobytes(), off, 0, 0,
                                  np.diff(want[1].astype(np.int64)))
        _comb[kind] = (data, off, where, want, info)
    return _comb[kind]


@pytest.mark.parametrize("kind", ["decode", "encode"])
def test_combined_batch_keeps_the_paths(kind):
    """The fixtures strung into one batch still sit where they are named
    for, each at each of its residues, and every tile between them is an
    ordinary fast one."""
    data, off, where, want, info = combined_case(kind)
    assert 100 < len(info) < 400
    special = {ti for _, _, ti in where}
    for j, t in enumerate(info):
        if j not in special:
            assert t["staged"] and t["path"] == "fast", j
    for f, r, ti in where:
        assert int(off[ti * L.TS]) % 16 == r
        if f.key is not None:
            assert f.key(info[ti]) == f.want[r], (f, r)


# ---- GPU -------------------------------------------------------------------------

def _torch():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("gpu test without a GPU")
    return torch


@pytest.fixture(scope="module", params=["default", "lean", "full"])
def vcodec(request):
    """The module's codec, and one pinned to each kernel variant (the
    variable set only around the constructor, as test_kernel_variants)."""
    import qhuff
    _torch()
    if request.param == "default":
        c = qhuff.Codec(0)
    else:
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


@pytest.fixture(scope="module")
def codec():
    import qhuff
    _torch()
    c = qhuff.Codec(0)
    yield c
    c.close()


def to_dev(data, off, pad):
    torch = _torch()
    d = torch.zeros(len(data) + pad + 16, dtype=torch.uint8, device="cuda")
    assert d.data_ptr() % 16 == 0            # the residues are the model's
    d[pad:pad + len(data)] = torch.from_numpy(data).cuda()
    o = torch.from_numpy(off.astype(np.int64) + pad).to(torch.int32).cuda()
    return d, o


def gpu_decode(c, data, off, pad):
    torch = _torch()
    d, o = to_dev(data, off, pad)
    out, out_off, status = c.decode(d, o)
    torch.cuda.synchronize()
    assert c.device_error() == 0
    oo = out_off.cpu().numpy().view(np.uint32)
    return out[:int(oo[-1])].cpu().numpy(), oo, status.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("f", L.DECODE, ids=repr)
def test_decode_limits(vcodec, f):
    """Bytes, offsets and statuses of the oracle on every decode fixture, at
    each of its residues."""
    for r in f.residues:
        data, off, pad, ti, (o_out, o_off, o_st), _ = dec_case(f, r)
        g_out, g_off, g_st = gpu_decode(vcodec, data, off, pad)
        assert np.array_equal(g_st, o_st), (f, r)
        assert np.array_equal(g_off, o_off), (f, r)
        assert np.array_equal(g_out, o_out), (f, r)


@pytest.mark.gpu
@pytest.mark.parametrize("f", L.ENCODE, ids=repr)
def test_encode_limits(codec, f):
    """The oracle's bytes and offsets on every encode fixture in modes 0 and
    7, and the mode-0 result decoded back to the input."""
    torch = _torch()
    for r in f.residues:
        for mode in (0, 7):
            data, off, pad, ti, (o_out, o_off), _ = enc_case(f, r, mode)
            d, o = to_dev(data, off, pad)
            out, out_off = codec.encode(d, o, mode)
            torch.cuda.synchronize()
            assert codec.device_error() == 0
            g_off = out_off.cpu().numpy().view(np.uint32)
            g_out = out[:int(g_off[-1])].cpu().numpy()
            assert np.array_equal(g_off, o_off), (f, r, mode)
            assert np.array_equal(g_out, o_out), (f, r, mode)
            if mode == 0:
                b_out, b_off, b_st = gpu_decode(codec, g_out, g_off, 0)
                assert not b_st.any()
                assert np.array_equal(b_off, off - off[0])
                assert np.array_equal(b_out, data)


@pytest.fixture(scope="module", params=["full", "lean"])
def small_grid_codec(request):
    """a codec whose grid is 1 % of the resident one (a few workgroups), so
    that a batch of a few hundred tiles is claimed by tickets and every
    wave holds pending tiles while it codes the next"""
    import qhuff
    _torch()
    env = {"QHUFF_GRID_PCT": "1", "QHUFF_KERNELS": request.param}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        c = qhuff.Codec(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    yield c
    c.close()


@pytest.mark.gpu
def test_decode_limits_among_pending_tiles(small_grid_codec):
    """every decode fixture at every residue in one batch on a grid of a few
    workgroups: big tiles, cooperative tiles and slow tiles between pending
    ones (parked outputs, the slot ring), twice"""
    data, off, where, (o_out, o_off, o_st), _ = combined_case("decode")
    for _ in range(2):
        g_out, g_off, g_st = gpu_decode(small_grid_codec, data, off, 0)
        assert np.array_equal(g_st, o_st)
        assert np.array_equal(g_off, o_off)
        assert np.array_equal(g_out, o_out)


@pytest.mark.gpu
def test_encode_limits_among_pending_tiles(small_grid_codec):
    torch = _torch()
    data, off, where, (o_out, o_off), _ = combined_case("encode")
    d, o = to_dev(data, off, 0)
    for _ in range(2):
        out, out_off = small_grid_codec.encode(d, o, 0)
        torch.cuda.synchronize()
        assert small_grid_codec.device_error() == 0
        g_off = out_off.cpu().numpy().view(np.uint32)
        assert np.array_equal(g_off, o_off)
        assert np.array_equal(out[:int(g_off[-1])].cpu().numpy(), o_out)
