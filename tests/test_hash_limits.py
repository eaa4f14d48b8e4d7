"""The header-hash kernel at the limits of its own layout (limits.HASH) and
across the rounds of its prefetch chain.

CPU part: every fixture sits on the side of the stage edge it is named for
-- by the layout model, limits.classify_hash -- and the chain batch holds
every hand-over between a staged and an unstaged tile at every stride a
grid could give.  GPU part: qhuff_xxh32_headers and qhuff_xxh32_batch on
the fixtures, bit-exact against the oracle, with three seeds; the chain
batch on a context whose hash grid is 1 % of the resident one, where the
diagnostic qhuff_grid_waves says how many rounds a wave runs; the same
batch on the default grid; the host path, which moves the residues."""
import os

import numpy as np
import pytest

import _paths  # noqa: F401
import limits as L
import oracle_lib as O
from test_limits import _torch, to_dev

SEEDS = (O.XXH_SEED, 0, 0xffffffff)

# ---- the batches and their oracle results, built once --------------------------

_case, _want, _chain = {}, {}, {}


def hash_case(f, variant, residue, pad_front=True):
    k = (f.name, variant, residue, pad_front)
    if k not in _case:
        data, off, pad, ti, nt = L.hash_batch_of(f, variant, residue, pad_front)
        info = L.classify_hash(off.astype(np.int64) + pad, 0,
                               L.is_pairs(variant))
        _case[k] = (data, off, pad, ti, nt, info)
    return _case[k]


def hash_want(f, variant, residue, seed, pad_front=True):
    k = (f.name, variant, residue, seed, pad_front)
    if k not in _want:
        data, off = hash_case(f, variant, residue, pad_front)[:2]
        _want[k] = L.hash_oracle(data, off, L.is_pairs(variant), seed)
    return _want[k]


def chain_case(pairs):
    if pairs not in _chain:
        data, off, where, plan = L.hash_chain(pairs)
        _chain[pairs] = (data, off, where, plan,
                         L.classify_hash(off, 0, pairs),
                         L.hash_oracle(data, off, pairs, O.XXH_SEED))
    return _chain[pairs]


# ---- CPU: the fixtures against the model -----------------------------------------

@pytest.mark.parametrize("f", L.HASH, ids=repr)
def test_hash_fixtures_reach_their_side(f):
    """Each fixture's tiles are staged or not as it says, in every layout
    and at every residue it is run at, with the span it names; its twin is
    the same strings on the other side; the ordinary tiles around it are
    staged; a partial tile ends the batch with the count it names."""
    for v in f.variants():
        pairs = L.is_pairs(v)
        per = L.TS * (2 if pairs else 1)
        for r in f.residues:
            data, off, pad, ti, nt, info = hash_case(f, v, r)
            assert len(info) == ti + nt + (0 if f.last else 2) and ti == 2
            for j, t in enumerate(info):
                if j < ti or j >= ti + nt:
                    assert t["staged"] and t["cnt"] == L.TS, (f, v, r, j, t)
                else:
                    assert t["staged"] == f.want[r], (f, v, r, j, t)
                    assert t["n16"] * 16 == t["span"]
            if r in f.spans:
                assert info[ti]["span"] == f.spans[r], (f, v, r)
            if f.last:
                assert info[-1]["cnt"] == len(f.strings[v]) * L.TS // per < L.TS
    if f.twin:
        g = L.HASH_BY_NAME[f.twin]
        assert g.twin == f.name
        assert [g.want[r] for r in g.residues] == [not f.want[r]
                                                   for r in f.residues]
        for v in f.variants():
            a, b = b"".join(f.strings[v]), b"".join(g.strings[v])
            assert a == b or (len(a) + 1 == len(b) and b.startswith(a)) \
                or (len(b) + 1 == len(a) and a.startswith(b))


def test_hash_fixture_arithmetic():
    """What the fixtures' names promise, in numbers."""
    H = L.HASH_BY_NAME
    assert {16, 17, 19, 20, 31, 32, 35} <= set(L.STAGE_LAST_LENS)
    assert {-ll & 3 for ll in L.STAGE_LAST_LENS} == {0, 1, 2, 3}
    assert min(L.STAGE_LAST_LENS) >= 16
    for ll in L.STAGE_LAST_LENS:
        f, g = H["hash_stage6144_len%d" % ll], H["hash_stage6160_len%d" % ll]
        for v in L.LAYOUTS:
            per = L.TS * (2 if L.is_pairs(v) else 1)
            data, off, pad, ti, nt, info = hash_case(f, v, 0)
            a, b = int(off[ti * per]) + pad, int(off[(ti + 1) * per]) + pad
            assert a % 16 == 0 and b - a == L.HASH_STAGE
            # every lane's every chunk live: Chunks::load's clamp on its edge
            assert info[ti]["n16"] == 384 == L.TS * L.HASH_NCH
            last = int(off[(ti + 1) * per - 1]) + pad
            assert b - last == ll and (last - a) & 3 == -ll & 3
            # the last stripe's s[q + 4] and the last word's s[q + 1] are
            # slack words: past the stage, inside HashWave::s
            q = (L.HASH_STAGE - 16) // 4 + 4 if ll % 16 == 0 else None
            if q is not None:
                assert L.HASH_STAGE // 4 <= q < L.HASH_STAGE // 4 \
                    + L.HASH_SLACK_WORDS
            t5 = hash_case(g, v, 5)[5][2]
            assert t5["span"] == L.HASH_STAGE + 16 and not t5["staged"]
    for name, span in (("hash_stage_res15", 6144), ("hash_stage_res15_over",
                                                    6160)):
        for v in L.LAYOUTS:
            per = L.TS * (2 if L.is_pairs(v) else 1)
            data, off, pad, ti, nt, info = hash_case(H[name], v, 15)
            a, b = int(off[ti * per]) + pad, int(off[(ti + 1) * per]) + pad
            assert a % 16 == 15 and (b % 16 == 0) == (span == 6144)
            assert info[ti]["span"] == span
    for ln in L.LONG_LENS:
        assert ln > L.HASH_STAGE
        for nm, lane in (("first", 0), ("last", 63)):
            f = H["hash_%s_lane_long_%d" % (nm, ln)]
            assert set(f.variants()) == {"single", "pairs_name", "pairs_value"}
            assert len(f.strings["single"][lane]) == ln
            assert len(f.strings["pairs_name"][2 * lane]) == ln
            assert len(f.strings["pairs_value"][2 * lane + 1]) == ln
            for v in f.variants():
                lens = sorted(len(s) for s in f.strings[v])
                assert lens[0] == 0 and lens[-2] < 64
    assert sorted(n for n in H if n.startswith("hash_partial")) == sorted(
        "hash_partial_%d_%s" % (c, s) for c in (1, 2, 63)
        for s in ("staged", "glb"))


@pytest.mark.parametrize("name", ["hash_lengths", "hash_lengths_glb"])
def test_hash_lengths_cover(name):
    """Every length 0..96 starts on every residue 0..15 of the placed batch
    -- in the pairs layout once as a name and once as a value -- with no
    gap between the strings; the unstaged build holds one string of 6200
    bytes in every tile."""
    f = L.HASH_BY_NAME[name]
    for v in L.LAYOUTS:
        roles = 2 if L.is_pairs(v) else 1
        per = L.TS * roles
        data, off, pad, ti, nt, info = hash_case(f, v, 0)
        o = off.astype(np.int64) + pad
        assert int(o[-1]) - int(o[0]) == len(data)           # no gaps
        seen = set()
        for i in range(ti * per, (ti + nt) * per):
            ln = int(o[i + 1] - o[i])
            if ln <= 96:
                seen.add((i % roles, ln, int(o[i]) % 16))
        assert seen == {(p, ln, r) for p in range(roles) for ln in range(97)
                        for r in range(16)}, (name, v)
        for t in range(ti, ti + nt):
            lens = np.diff(o[t * per:(t + 1) * per + 1])
            assert (lens == L.FILLER).sum() == (1 if name.endswith("glb")
                                                else 0)
            assert ((lens <= 96) | (lens == L.FILLER)).all()
        assert 20 <= nt <= 30


@pytest.mark.parametrize("pairs", [True, False], ids=["headers", "batch"])
def test_hash_chain_batch(pairs):
    """The chain batch: 640 full tiles and one of 37; every tile staged or
    not as it was built to be, every fixture on its residue; and for every
    stride w a grid of at most 640 / 3 waves can give, each hand-over
    (staged or not -> staged or not) between tiles t and t + w occurs at
    least 32 times."""
    data, off, where, plan, info, _ = chain_case(pairs)
    per = L.TS * (2 if pairs else 1)
    assert len(info) == L.CHAIN_TILES + 1 == len(plan)
    assert [t["cnt"] for t in info] == [L.TS] * L.CHAIN_TILES + [L.CHAIN_LAST]
    assert [t["staged"] for t in info] == plan
    assert 2_500_000 < len(data) < 4_500_000
    names = {f.name for f, _, _ in where}
    assert names == {f.name for f in L.HASH if not f.last}
    for f, r, ti in where:
        assert int(off[ti * per]) % 16 == r
        if r in f.spans:
            assert info[ti]["span"] == f.spans[r]
    staged = plan[:L.CHAIN_TILES]
    for w in range(1, L.CHAIN_TILES // 3 + 1):
        c = L.transitions(staged, w)
        assert min(c.values()) >= 32, (w, c)


# ---- GPU -------------------------------------------------------------------------

def _open(env):
    """a codec opened with the variables of env set around the constructor
    only"""
    import qhuff
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
    c = _open({})
    yield c
    c.close()


@pytest.fixture(scope="module")
def small_grid_codec():
    c = _open({"QHUFF_GRID_PCT": "1"})
    yield c
    c.close()


def gpu_hash(c, d, o, pairs, seed):
    """qhuff_xxh32_headers / qhuff_xxh32_batch on device tensors -> the
    hashes as uint32 arrays, (name, nameval) or (hash,)"""
    torch = _torch()
    got = c.xxh32_headers(d, o, seed) if pairs else (c.xxh32(d, o, seed),)
    torch.cuda.synchronize()
    assert c.device_error() == 0
    return tuple(h.cpu().numpy().view(np.uint32) for h in got)


def same(got, want):
    return len(got) == len(want) and all(
        np.array_equal(g, w) for g, w in zip(got, want))


def wrong_lengths(off, pairs, got, want):
    """(for the message of a failure) the lengths of the strings whose hash
    is wrong -- a value's only where its name's, its seed, is right"""
    ln = np.diff(off.astype(np.int64))
    if not pairs:
        return sorted(set(ln[got[0] != want[0]].tolist()))
    n1 = got[0] != want[0]
    return sorted(set(ln[0::2][n1].tolist())
                  | set(ln[1::2][~n1 & (got[1] != want[1])].tolist()))


@pytest.mark.gpu
@pytest.mark.parametrize("f", L.HASH, ids=repr)
def test_hash_limits(codec, f):
    """The oracle's hashes on every fixture: both calls (every layout
    variant), each residue, the reference's seed, 0 and 0xffffffff."""
    for v in f.variants():
        pairs = L.is_pairs(v)
        for r in f.residues:
            data, off, pad = hash_case(f, v, r)[:3]
            d, o = to_dev(data, off, pad)
            for seed in SEEDS:
                got = gpu_hash(codec, d, o, pairs, seed)
                want = hash_want(f, v, r, seed)
                ok = same(got, want)
                assert ok, (f, v, r, seed, "wrong lengths",
                                         wrong_lengths(off, pairs, got, want))


def _run_chain(c):
    for pairs in (True, False):
        data, off, where, plan, info, want = chain_case(pairs)
        d, o = to_dev(data, off, 0)
        for _ in range(2):
            got = gpu_hash(c, d, o, pairs, O.XXH_SEED)
            bad = [int(np.flatnonzero(g != w)[0]) // L.TS
                   for g, w in zip(got, want) if not np.array_equal(g, w)]
            ok = same(got, want)
            assert ok, ("first wrong tile", pairs, bad)


@pytest.mark.gpu
def test_hash_chain_small_grid(small_grid_codec):
    """Every wave of a grid of 1 % hashes at least three tiles, staged and
    unstaged ones in every order, the edge fixtures among them and a partial
    tile at the end: both calls, twice, bit-exact with the oracle."""
    import qhuff
    W = small_grid_codec.grid_waves(qhuff.KIND_HASH)
    print("hash grid waves at QHUFF_GRID_PCT=1:", W)
    assert W > 0 and 3 * W <= L.CHAIN_TILES, W
    _run_chain(small_grid_codec)


@pytest.mark.gpu
def test_hash_chain_default_grid(codec, small_grid_codec):
    """the same batch on the resident grid: the same hashes; the diagnostic
    reports every kind's grid, the knob shrinks each, and another kind or no
    context is QHUFF_EINVAL"""
    import qhuff
    for kind in (qhuff.KIND_ENCODE, qhuff.KIND_DECODE, qhuff.KIND_HASH):
        full = codec.grid_waves(kind)
        assert full > 0
        assert 0 < small_grid_codec.grid_waves(kind) < full
    lib = qhuff.lib()
    assert lib.qhuff_grid_waves(codec._ctx, 3) == qhuff.EINVAL
    assert lib.qhuff_grid_waves(codec._ctx, -1) == qhuff.EINVAL
    assert lib.qhuff_grid_waves(None, qhuff.KIND_HASH) == qhuff.EINVAL
    _run_chain(codec)


def test_grid_waves_rejects_null():
    """(no device needed) the diagnostic is exported, bound and announced"""
    import qhuff
    assert "qhuff_grid_waves" in qhuff.EXPORTS
    assert qhuff.lib().qhuff_grid_waves(None, qhuff.KIND_HASH) == qhuff.EINVAL
    hdr = open(qhuff.HEADER).read()
    assert "#define QHUFF_FEATURE_GRID_WAVES 1" in hdr
    assert "#define QHUFF_ABI_VERSION 7" in hdr


HOST = [f for f in L.HASH if f.name.startswith(("hash_stage6144",
                                                "hash_stage6160",
                                                "hash_lengths"))]


def test_hash_host_fixtures_keep_their_side():
    """(CPU) the host path copies the bytes from off[0] on to a 16-byte-
    aligned stage, so a tile's residue there is its distance from off[0]:
    with the fixture put on its residue by a longer string in front (no
    padding) and off[0] = 7, the model at base residue -7 gives the
    fixture's side."""
    for f in HOST:
        for r in f.residues:
            data, off, pad, ti, nt, _ = hash_case(f, "pairs", r, False)
            assert pad == 0 and off[0] == 0
            info = L.classify_hash(off.astype(np.int64) + 7, -7 % 16, True)
            assert all(t["staged"] == f.want[r] for t in info[ti:ti + nt])
            assert all(t["staged"] for t in info[:ti] + info[ti + nt:])
            if r in f.spans:
                assert info[ti]["span"] == f.spans[r]


@pytest.mark.gpu
def test_hash_limits_host_path():
    """qhuff_xxh32_headers_host on the stage-edge fixtures and the length x
    alignment ones, off[0] = 7, on a fresh context (its staging grows from
    nothing, then again for the longer batches)"""
    c = _open({})
    try:
        for f in HOST:
            for r in f.residues:
                data, off = hash_case(f, "pairs", r, False)[:2]
                d7 = np.concatenate([np.full(7, 0xA5, np.uint8), data])
                got = c.xxh32_headers_host(d7, off + np.uint32(7))
                assert c.device_error() == 0
                want = hash_want(f, "pairs", r, O.XXH_SEED, False)
                ok = same(got, want)
                assert ok, (f, r)
    finally:
        c.close()
