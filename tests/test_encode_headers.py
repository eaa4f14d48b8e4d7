"""qhuff_encode_headers / qhuff_encode_headers_host: header lists to field
sections against the static table in one call (include/qhuff.h).

Expectations: tests/headers_model.py (the reference's rule over its own
tables, qpack_frames.enc_int + oracle_lib.enc_enc_str), never the library.
Every shape runs through the device-pointer and the host form and is checked
for out, sec_out, kind and static_id."""
import ctypes as C
import functools
import os
import random

import numpy as np
import pytest

import _paths  # noqa: F401
import headers_model as M
import limits as L
import oracle_lib as O
import qhuff
import qpack_frames as Q
from test_buffer_contract import FILLS, Arena

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TILE = L.TS


# ---- shapes ------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def pool():
    return M.near_miss_pairs()


def headers(n, seed, flags="alt"):
    """n headers from the near-miss pool and noise; flags: "alt" (N bit on
    every other header), "rand" or None (all 0)"""
    rng = random.Random(seed)
    out = []
    for i in range(n):
        nm, v = rng.choice(pool()) if rng.random() < 0.8 else \
            (M._rand(rng, rng.randrange(0, 20)), M._rand(rng, rng.randrange(0, 40)))
        f = 0 if flags is None else (i & 1) if flags == "alt" else \
            rng.randrange(4)            # (bits above bit 0 are not the N bit)
        out.append((nm, v, f))
    return out


def split(hs, cuts):
    """hs cut at the header indices `cuts` (repeats: empty sections)"""
    cuts = [0] + list(cuts) + [len(hs)]
    return [hs[a:b] for a, b in zip(cuts, cuts[1:])]


@functools.lru_cache(maxsize=None)
def shape(name):
    if name == "m1":
        return M.Headers([headers(150, 1)])
    if name == "each_own":                     # every header its own section
        return M.Headers([[h] for h in headers(200, 2)])
    if name == "empties":                      # first, last and adjacent
        return M.Headers(split(headers(140, 3), [0, 0, 5, 70, 70, 70, 140, 140]))
    if name == "boundaries":
        # on lanes 0, 1 and 63 of a tile and across a tile edge
        return M.Headers(split(headers(4 * TILE + 9, 4),
                               [1, TILE - 1, TILE, TILE + 1, 2 * TILE - 1,
                                2 * TILE + 1, 3 * TILE, 3 * TILE + 63]))
    if name == "three_tiles":                  # one section spanning three
        return M.Headers(split(headers(5 * TILE, 5), [TILE - 3, 4 * TILE + 2]))
    if name == "no_flags":
        return M.Headers(split(headers(130, 6, None), [64, 65]), flags=False)
    if name == "rand_flags":
        return M.Headers(split(headers(130, 7, "rand"), [3, 100]))
    if name == "many_empties":                 # more than 64 starts in a tile
        return M.Headers(split(headers(70, 8), [2] * 150 + [40] * 3))
    if name.startswith("n"):                   # counts, sections of 16
        n = int(name[1:])
        return M.Headers(split(headers(n, 50 + n), range(16, n, 16)))
    raise KeyError(name)


SHAPES = ("m1", "each_own", "empties", "boundaries", "three_tiles", "no_flags",
          "rand_flags", "many_empties", "n1", "n63", "n64", "n65", "n513")


def test_shapes_are_what_they_are_named():
    h = shape("empties")
    lens = np.diff(h.sec_hdr).tolist()
    assert lens[0] == 0 and lens[-1] == 0 and lens[1] == 0 and 0 in lens[4:6]
    assert b"".join(h.want_sections[:2]) == b"\0\0\0\0"
    b = set(shape("boundaries").sec_hdr.tolist())
    assert {1, 63, 64, 65, 127, 129, 192, 255} <= b
    assert shape("no_flags").hflags is None
    assert set(shape("rand_flags").hflags.tolist()) == {0, 1, 2, 3}
    assert shape("many_empties").m > 150
    for name in SHAPES:
        h = shape(name)
        assert set(h.want_kind.tolist()) == {0, 1, 2} or h.n < 20, name
        assert len(h.want) == h.want_sec_out[-1] <= h.bound
    # the N bit shows in the bytes
    a = M.Headers([[(b"dude", b"x", 1), (b"age", b"7", 1)]]).want
    b = M.Headers([[(b"dude", b"x", 0), (b"age", b"7", 2)]]).want
    assert a != b and a[2] == 0x30 | b[2] and len(a) == len(b)


def test_bound_formula():
    for in_bytes, n, m in ((0, 0, 0), (1, 1, 1), (4096, 64, 5), (1 << 20, 9, 0)):
        assert qhuff.encode_headers_bound(in_bytes, n, m) \
            == qhuff.encode_wire_bound(in_bytes, 2 * n + 2 * m)
    assert shape("m1").bound == qhuff.encode_headers_bound(
        len(shape("m1").data), 150, 1)


# ---- GPU ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def codec():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("gpu test without a GPU")
    c = qhuff.Codec(0)
    yield c
    c.close()


def dev(a, pad=0):
    import torch
    a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    t = torch.zeros(len(a) + pad + 16, dtype=torch.uint8, device="cuda")
    if len(a):
        t[pad:pad + len(a)] = torch.from_numpy(a).cuda()
    return t


def dev_i32(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).cuda()


def run_device(codec, h, pad=0, stream=None):
    d = dev(h.data, pad)
    off = dev_i32((h.off.astype(np.uint64) + pad).astype(np.uint32))
    fl = dev(h.hflags)[:max(h.n, 1)] if h.hflags is not None else None
    return codec.encode_headers(d, off, dev_i32(h.sec_hdr), fl, stream=stream)


def fetch(res):
    out, so, kind, sid = res
    so = so.cpu().numpy().view(np.uint32)
    return (out[:int(so[-1])].cpu().numpy().tobytes(), so,
            kind.cpu().numpy(), sid.cpu().numpy())


def check(h, got):
    out, so, kind, sid = got
    assert np.array_equal(so, h.want_sec_out)
    assert np.array_equal(kind, h.want_kind)
    assert np.array_equal(sid, h.want_id)
    assert bytes(out) == h.want


def check_both(codec, h, pads=(0,)):
    import torch
    for pad in pads:
        res = run_device(codec, h, pad)
        torch.cuda.synchronize()
        assert codec.device_error() == 0
        check(h, fetch(res))
    out, so, kind, sid = codec.encode_headers_host(h.data, h.off, h.sec_hdr,
                                                   h.hflags)
    check(h, (out.tobytes(), so, kind, sid))


@pytest.mark.gpu
def test_reference_vectors(codec):
    """test_qpack.c:47, :64, :129 give prefix + header byte for byte; the
    headers of :83 give its header bytes (its encoder-stream bytes are the
    dynamic table's)"""
    vec = M.reference_vectors()
    for ln, hs, body in vec:
        h = M.Headers([hs])
        assert h.want == body
        check_both(codec, h)
    # and the four as four sections of one call
    h = M.Headers([hs for _, hs, _ in vec])
    assert h.want == b"".join(body for _, _, body in vec)
    check_both(codec, h)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SHAPES)
def test_section_shapes(codec, name):
    """out, sec_out, kind and static_id of every shape, device form at data
    residues 0, 1 and 15 and host form"""
    check_both(codec, shape(name), pads=(0, 1, 15))


@functools.lru_cache(maxsize=None)
def corpus():
    lists = []
    for fn in ("fb-req.qif", "netbsd.qif"):
        with open(os.path.join(G, "data", fn), "rb") as f:
            lists += Q.qif_header_lists(f.read())
    return M.Headers(lists, flags=False)


def test_corpus_has_all_three_kinds():
    h = corpus()
    assert h.m > 100 and h.n > 1000
    assert set(h.want_kind.tolist()) == {M.INDEXED, M.NAMEREF, M.LITERAL}


@pytest.mark.gpu
def test_round_trip_qif(codec):
    """the QIF header lists, one section a list: byte-exact, and decoded back
    every section is OK and its literals are the names and values of the
    lines the model did not index"""
    h = corpus()
    check_both(codec, h)
    out, so, kind, sid = codec.encode_headers_host(h.data, h.off, h.sec_hdr)
    res = codec.decode_sections_host(out, so, qhuff.SCAN_FIELD_SECTION,
                                     qhuff.MAX_STRLEN)
    ret, lits, lit_off, rc, consumed, dec, doo, st = res
    assert ret == qhuff.OK and not rc.any() and not st.any()
    assert np.array_equal(consumed, np.diff(so))
    want = []
    for sec in h.sections:
        for nm, v, _ in sec:
            k = M.lookup(nm, v)[2]
            if k == M.LITERAL:
                want.append(nm)
            if k != M.INDEXED:
                want.append(v)
    dec = dec.tobytes()
    assert [dec[doo[i]:doo[i + 1]] for i in range(len(doo) - 1)] == want


@pytest.mark.gpu
def test_unstaged_tiles(codec):
    """tiles on the lookup kernel's global-memory path (a value past the
    hash stage in them), static names at their first and last lanes, between
    staged tiles: the items those lanes write, and their long values through
    the encode launch"""
    from test_static_lookup import unstaged_batch
    pairs = unstaged_batch()
    h = M.Headers(split(pairs, range(50, len(pairs), 50)), flags=False)
    for r in (0, 15):
        info = L.classify_hash(h.off.astype(np.int64) + r, 0, True)
        assert [t["staged"] for t in info] == [True, False] * 3
    check_both(codec, h, pads=(0, 15))


@pytest.mark.gpu
def test_small_grid_every_wave_several_tiles():
    """a context whose hash grid is 1 %: every wave of the lookup launch
    runs three tiles or more through its prefetch chain, the sections'
    search and the prefix items with it"""
    from test_hash_limits import _open
    c = _open({"QHUFF_GRID_PCT": "1"})
    try:
        W = c.grid_waves(qhuff.KIND_HASH)
        base = shape("boundaries")
        k = -(-(3 * W * TILE + 1) // base.n)
        h = Repeated(base, k)
        assert W > 0 and h.n > 3 * W * TILE and k < 400
        for _ in range(2):
            check_both(c, h)
    finally:
        c.close()


def specs(h, k, r_in, out_bytes):
    return [("in", len(h.data), r_in),
            ("off", 4 * (2 * h.n + 1), 4 * (k % 4)),
            ("hflags", h.n, (3 * k + 1) % 16),
            ("sec_hdr", 4 * (h.m + 1), 4 * ((k + 1) % 4)),
            ("out", out_bytes, (7 * k + 3) % 16),
            ("sec_out", 4 * (h.m + 1), 4 * ((k + 2) % 4)),
            ("kind", h.n, (5 * k + 2) % 16),
            ("static_id", h.n, (k + 9) % 16)]


def contract_call(codec, h, host, k, r_in, fill):
    import torch
    ar = Arena(specs(h, k, r_in, len(h.want)), seed=7000 + 16 * k + r_in)
    ar.put("in", h.data)
    ar.put("off", h.off)
    ar.put("hflags", h.hflags if h.hflags is not None
           else np.zeros(h.n, np.uint8))
    ar.put("sec_hdr", h.sec_hdr)
    ar.neighbours("in", fill)
    ar.commit(not host)
    fl = "hflags" if h.hflags is not None else None
    if host:
        rc = qhuff.lib().qhuff_encode_headers_host(
            codec._ctx, ar.addr("in"), ar.addr("off"), h.n,
            ar.addr(fl) if fl else None, ar.addr("sec_hdr"), h.m,
            ar.addr("out"), ar.addr("sec_out"), ar.addr("kind"),
            ar.addr("static_id"))
        assert rc == qhuff.OK
    else:
        codec.encode_headers_into(ar.ptr("in"), ar.ptr("off"), h.n,
                                  ar.ptr(fl) if fl else None,
                                  ar.ptr("sec_hdr"), h.m, ar.ptr("out"),
                                  ar.ptr("sec_out"), ar.ptr("kind"),
                                  ar.ptr("static_id"))
        torch.cuda.synchronize()
        assert codec.device_error() == 0
    return ar, ar.after()


@pytest.mark.gpu
@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
@pytest.mark.parametrize("name", ["n0m0", "n0m3", "n65", "empties", "no_flags",
                                  "boundaries"])
def test_buffer_contract(codec, name, host):
    """`out` of exactly sec_out[m] bytes and every array at its exact size in
    a dirty guarded arena: the expected bytes, and nothing else written"""
    h = {"n0m0": lambda: M.Headers([]),
         "n0m3": lambda: M.Headers([[], [], []])}.get(name,
                                                      lambda: shape(name))()
    if name == "n0m3":
        assert h.want == b"\0\0" * 3 and h.want_sec_out.tolist() == [0, 2, 4, 6]
    for k, fill in enumerate(FILLS):
        k += 3 * host
        ar, img = contract_call(codec, h, host, k, (0, 1, 15)[k % 3], fill)
        assert np.array_equal(ar.get(img, "sec_out", np.uint32), h.want_sec_out)
        assert ar.get(img, "out").tobytes() == h.want
        assert np.array_equal(ar.get(img, "kind"), h.want_kind)
        assert np.array_equal(ar.get(img, "static_id"), h.want_id)
        ar.check(img, {"out": len(h.want), "sec_out": 4 * (h.m + 1),
                       "kind": h.n, "static_id": h.n})


@pytest.mark.gpu
def test_optional_outputs_null(codec):
    import torch
    h = shape("n65")
    d, off = dev(h.data), dev_i32(h.off)
    out = torch.empty(h.bound, dtype=torch.uint8, device="cuda")
    so = torch.empty(h.m + 1, dtype=torch.int32, device="cuda")
    codec.encode_headers_into(d, off, h.n, dev(h.hflags), dev_i32(h.sec_hdr),
                              h.m, out, so)
    torch.cuda.synchronize()
    so = so.cpu().numpy().view(np.uint32)
    assert np.array_equal(so, h.want_sec_out)
    assert out[:int(so[-1])].cpu().numpy().tobytes() == h.want
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    o = np.zeros(h.bound, np.uint8)
    s = np.zeros(h.m + 1, np.uint32)
    assert qhuff.lib().qhuff_encode_headers_host(
        codec._ctx, p(h.data), p(h.off), h.n, p(h.hflags), p(h.sec_hdr), h.m,
        p(o), p(s), None, None) == qhuff.OK
    assert np.array_equal(s, h.want_sec_out)
    assert o[:s[-1]].tobytes() == h.want


@pytest.mark.gpu
def test_argument_errors(codec):
    h = shape("n65")
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    out = np.full(h.bound, 0xA5, np.uint8)
    so = np.full(h.m + 1, 0xA5A5A5A5, np.uint32)
    kind, sid = np.full(h.n, 0xA5, np.uint8), np.full(h.n, 0xA5, np.uint8)

    def call(ctx=codec._ctx, data=p(h.data), off=h.off, n=h.n,
             sec_hdr=h.sec_hdr, m=h.m, o=p(out), s=p(so)):
        return qhuff.lib().qhuff_encode_headers_host(
            ctx, data, p(off) if off is not None else None, n, p(h.hflags),
            p(sec_hdr) if sec_hdr is not None else None, m, o, s, p(kind),
            p(sid))

    E = qhuff.EINVAL
    assert call(ctx=None) == E and call(data=None) == E
    assert call(off=None) == E and call(sec_hdr=None) == E
    assert call(o=None) == E and call(s=None) == E
    bad = h.off.copy()
    bad[40] = bad[39] - 1 if bad[39] else bad[41] + 1
    assert call(off=bad) == E
    for i, v in ((0, 1), (2, 100), (h.m, h.n - 1), (h.m, h.n + 1)):
        sh = h.sec_hdr.copy()
        sh[i] = v
        assert call(sec_hdr=sh) == E, (i, v)
    # 2n + 2m past 32 bits: refused before anything is read
    assert call(n=0x7fffffff, m=0x7fffffff) == qhuff.ERANGE
    assert qhuff.encode_headers_bound(1 << 31, 1, 1) > 0xffffffff
    # nothing was written by the refused calls, and the context is as good
    assert (out == 0xA5).all() and (so == 0xA5A5A5A5).all()
    assert (kind == 0xA5).all() and (sid == 0xA5).all()
    check_both(codec, h)
    L_ = qhuff.lib()
    assert L_.qhuff_encode_headers(None, None, None, 0, None, None, 0, None,
                                   None, None, None, None) == E


@pytest.mark.gpu
def test_bound_range_error(codec):
    """a bound past 32 bits is QHUFF_ERANGE: one header whose value's
    offsets claim 2 GB (the check comes before any byte is read)"""
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    off = np.array([0, 3, 0x90000000], np.uint32)
    sh = np.array([0, 1], np.uint32)
    so = np.zeros(2, np.uint32)
    byte = np.zeros(16, np.uint8)
    assert qhuff.lib().qhuff_encode_headers_host(
        codec._ctx, p(byte), p(off), 1, None, p(sh), 1, p(byte), p(so), None,
        None) == qhuff.ERANGE


@pytest.mark.gpu
def test_scratch_reuse_and_streams(codec):
    """two calls of different sizes on one context (the scratch grows), then
    two on two streams without a synchronisation between them; the lookup is
    timed as a hash launch and the encode as an encode launch"""
    import torch
    c = qhuff.Codec(0)
    try:
        small, big = shape("n65"), M.Headers(split(headers(9000, 77),
                                                   range(16, 9000, 16)))
        for h in (small, big, small):
            check_both(c, h)
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(s1):
            ra = run_device(c, big, stream=s1)
        with torch.cuda.stream(s2):
            rb = run_device(c, small, stream=s2)
        torch.cuda.synchronize()
        assert c.device_error() == 0
        check(big, fetch(ra))
        check(small, fetch(rb))
        c.timing(True)
        try:
            c.timing_read()
            r = run_device(c, small)
            torch.cuda.synchronize()
            t = c.timing_read()
        finally:
            c.timing(False)
        assert [k for k, _ in t] == [qhuff.KIND_HASH, qhuff.KIND_ENCODE]
        check(small, fetch(r))
    finally:
        c.close()


class Repeated:
    """header lists h, k times over: the sections are independent, so the
    expectation is h's, k times"""

    def __init__(self, h, k):
        self.n, self.m = h.n * k, h.m * k
        self.data = np.tile(h.data, k)
        step = np.arange(k, dtype=np.uint64)[:, None]
        self.off = np.concatenate(
            [(h.off[None, :-1] + step * len(h.data)).reshape(-1),
             [k * len(h.data)]]).astype(np.uint32)
        self.sec_hdr = np.concatenate(
            [(h.sec_hdr[None, :-1] + step * h.n).reshape(-1),
             [self.n]]).astype(np.uint32)
        self.hflags = np.tile(h.hflags, k)
        self.want = h.want * k
        self.want_sec_out = np.concatenate(
            [(h.want_sec_out[None, :-1] + step * len(h.want)).reshape(-1),
             [len(self.want)]]).astype(np.uint32)
        self.want_kind = np.tile(h.want_kind, k)
        self.want_id = np.tile(h.want_id, k)


def test_repeated_is_the_model_s():
    h = M.Headers(split(headers(40, 9), [7, 7, 30]))
    r = Repeated(h, 3)
    g = M.Headers(h.sections * 3)
    assert r.want == g.want and np.array_equal(r.want_sec_out, g.want_sec_out)
    assert np.array_equal(r.off, g.off) and np.array_equal(r.sec_hdr, g.sec_hdr)
    assert np.array_equal(r.data, g.data)
    assert np.array_equal(r.want_kind, g.want_kind)


@pytest.mark.gpu
def test_memory_released_at_close():
    """the scratch, 16 bytes an item, is the context's: allocated by the
    first call, and device memory after qhuff_close is what it was before
    qhuff_open (test_memory.py's measure)"""
    import torch
    from test_memory import MB, free_bytes
    h = Repeated(M.Headers(split(headers(2000, 78), range(16, 2000, 16))), 160)
    scratch = 16 * (2 * h.n + 2 * h.m)
    assert scratch > 10 * MB
    warm = qhuff.Codec(0)
    try:
        d, off, sh, fl = (dev(h.data), dev_i32(h.off), dev_i32(h.sec_hdr),
                          dev(h.hflags))
        out = torch.empty(qhuff.encode_headers_bound(len(h.data), h.n, h.m),
                          dtype=torch.uint8, device="cuda")
        so = torch.empty(h.m + 1, dtype=torch.int32, device="cuda")
        kind, sid = (torch.empty(h.n, dtype=torch.uint8, device="cuda")
                     for _ in range(2))

        def run(c):
            c.encode_headers_into(d, off, h.n, fl, sh, h.m, out, so, kind, sid)
            torch.cuda.synchronize()
            assert c.device_error() == 0

        run(warm)
        check(h, fetch((out, so, kind, sid)))
        before = free_bytes()
        c = qhuff.Codec(0)
        try:
            run(c)
            used = before - free_bytes()
            assert scratch <= used <= scratch + 16 * MB, used / MB
        finally:
            c.close()
        assert abs(before - free_bytes()) <= 2 * MB
    finally:
        warm.close()
