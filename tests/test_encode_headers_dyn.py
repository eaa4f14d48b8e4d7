"""qhuff_dyn_lookup / qhuff_encode_headers_dyn: header lists to field sections
against the dynamic table's entries.

CPU (unmarked): the model (headers_dyn_enc_model.py) pinned on the interop
files -- every section's committed header list encoded in the window the
section was decoded in and decoded again with headers_dyn_model.section -- and
on two known answers that are RFC 9204's examples; qhuff_dyn_lookup_cpu (the
kernel's lookup source on the host) against the model on every case the GPU
tests run; tests/c/lookup_dyn_san.cpp under ASan + UBSan.

GPU (-m gpu): every case array for array against the model (bytes, sec_out,
kind, static_id, dyn_id) and read back through qhuff_decode_headers_dyn_host
with the same table and windows."""
import ctypes as C
import functools
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import _paths  # noqa: F401
import headers_dyn_enc_model as E
import headers_dyn_model as D
import headers_model as HM
import qhuff
from test_buffer_contract import FILLS, Arena, Ptr

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
IDX, NREF, LIT, DYN = E.INDEXED, E.NAMEREF, E.LITERAL, E.LINE_DYN
NEVER = HM.NEVER


# ---- the model pinned ----------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def replay(name):
    return D.Replay(name)


def interop_sections(name):
    """-> (Replay, Encoded of the file's QIF lists in the sections' windows)"""
    r = replay(name)
    lists = r.qif_lists(name)
    return r, E.Encoded([list(l) for l in lists], r.table, win=r.win,
                        flags=False)


def test_model_round_trip_on_the_interop_streams(record_property):
    """all 34 sections: the committed QIF list encoded in the window the
    section was decoded in decodes (headers_dyn_model.section) to that list,
    kind / dyn_id self-consistent; the sizes are recorded beside the
    reference's, not asserted: the reference also inserts and may refuse to
    risk"""
    total = 0
    for name in sorted(D.INTEROP):
        r, e = interop_sections(name)
        sizes = []
        for s, (lo, hi) in enumerate(r.win):
            sec = e.want_sections[s]
            rc, lines = D.section(sec, lo, hi, r.max_entries)
            assert rc == D.OK, (name, s)
            dec = D.Decoded([sec], r.table, [(lo, hi)])
            assert dec.headers == [(h[0], h[1]) for h in e.h.sections[s]]
            a, b = e.sec_hdr[s], e.sec_hdr[s + 1]
            assert [l.kind for l in lines] == e.want_kind[a:b].tolist()
            assert [D.DYN_NONE if l.dyn is None else l.dyn for l in lines] \
                == e.want_dyn[a:b].tolist()
            for l, (nm, v, _) in zip(lines, e.h.sections[s]):
                if l.dyn is not None:
                    ent = r.table.entry(l.dyn)
                    assert lo <= l.dyn < hi and ent[0] == nm
                    assert l.kind != IDX | DYN or ent[1] == v
            sizes.append((len(sec), len(r.sections[s])))
            total += 1
        record_property(name + "_sizes_model_vs_reference", json.dumps(sizes))
        assert (e.want_dyn != D.DYN_NONE).any()
    assert total == 34


RFC_A = [(b":authority", b"www.example.com"), (b":path", b"/sample/path")]
RFC_B = RFC_A + [(b"custom-key", b"custom-value"), RFC_A[0]]


def rfc_cases():
    return [
        (E.Encoded([RFC_A], D.Table(RFC_A, 0, 6), [(0, 2)], [0]),
         "03811011"),
        (E.Encoded([[RFC_A[0], (b":path", b"/"),
                     (b"custom-key", b"custom-value")]],
                   D.Table(RFC_B, 0, 6), None, [4]), "050080c181")]


def test_known_answers():
    """RFC 9204 B.2 (two post-base indexed lines under Base 0) and B.4's
    table with a duplicate (the newer of two equal entries, a static line, a
    dynamic one)"""
    for e, want in rfc_cases():
        assert e.want.hex() == want
    assert rfc_cases()[1][0].want_dyn.tolist() == [3, D.DYN_NONE, 2]


def test_abi():
    lib = qhuff.lib()
    for s in ("qhuff_dyn_lookup", "qhuff_dyn_lookup_host",
              "qhuff_dyn_lookup_cpu", "qhuff_dyn_index_slots",
              "qhuff_encode_headers_dyn_bound", "qhuff_encode_headers_dyn",
              "qhuff_encode_headers_dyn_host"):
        assert s in qhuff.EXPORTS and getattr(lib, s)
    with open(os.path.join(ROOT, "include", "qhuff.h")) as f:
        h = f.read()
    for k, v in (("QHUFF_FEATURE_ENCODE_HEADERS_DYN", "1"),
                 ("QHUFF_ABI_VERSION", "7")):
        assert h.split("#define %s " % k)[1].split()[0] == v
    assert lib.qhuff_abi_version() == 7
    for b, n, m in ((0, 0, 0), (1000, 7, 3), (5, 0, 9)):
        assert qhuff.encode_headers_dyn_bound(b, n, m) \
            == qhuff.encode_headers_bound(b, n, m)
    # the capacity rule: the smallest power of two >= 2d, at least 64
    for d in (0, 1, 31, 32, 33, 64, 65, 300, 1 << 20):
        s = qhuff.dyn_index_slots(d)
        assert s >= max(64, 2 * d) and s & (s - 1) == 0
        assert s == 64 or s // 2 < 2 * d


# ---- the cases -------------------------------------------------------------------------

def ent(k, v=None):
    return (b"x-e%d" % k, b"v%d" % k if v is None else v)


def table_of(d, first=0, me=None):
    return D.Table([ent(k) for k in range(d)], first,
                   max(d, 8) if me is None else me)


def fill(k):
    """a header no table holds"""
    return (b"x-lit-%d" % k, b"w%d" % k)


BIG = table_of(256, 0, 128)


def all_forms():
    """every line form in one section under Base 4 of 8 entries: indexed
    static / dynamic / post-base, name reference static / dynamic / post-base
    with N = 0 and 1, literal with N = 0 and 1"""
    t = table_of(8)
    sec = [(b":method", b"GET"), ent(1), ent(6),
           (b":path", b"/x", 0), (b":path", b"/y", NEVER),
           ent(2, b"other") + (0,), ent(2, b"other2") + (NEVER,),
           ent(5, b"other") + (0,), ent(5, b"") + (NEVER,),
           fill(0) + (0,), fill(1) + (NEVER,), ent(1) + (NEVER,)]
    return E.Encoded([sec], t, [(0, 8)], [4])


def int_edges():
    secs, win, base = [], [], []

    def add(sec, w, b):
        secs.append(sec)
        win.append(w)
        base.append(b)
    for r in (62, 63, 64):            # 6-bit relative index
        add([ent(79 - r)], (0, 80), 80)
    for r in (14, 15, 16):            # 4-bit name reference
        add([ent(79 - r, b"o")], (0, 80), 80)
    for r in (14, 15, 16):            # 4-bit post-base index
        add([ent(10 + r)], (0, 80), 10)
    for r in (6, 7, 8):               # 3-bit post-base name reference
        add([ent(10 + r, b"o", ) + (NEVER,)], (0, 80), 10)
    for dlt in (126, 127, 128):       # Delta Base, S = 0: Base - RIC
        add([ent(9)], (0, 100), 10 + dlt)
    for dlt in (126, 127, 128):       # S = 1: RIC - Base - 1
        add([ent(199)], (100, 200), 200 - 1 - dlt)
    for ric in (253, 254, 255):       # encoded RIC 254 / 255 / 256
        add([ent(ric - 1)], (130, 256), None)
    base = [w[1] if b is None else b for w, b in zip(win, base)]
    return E.Encoded(secs, BIG, win, base)


def ric_wrap(first):
    """max_entries = 4: RIC = first + 4 passes through multiples of 8"""
    t = D.Table([ent(first + k) for k in range(4)], first, 4)
    return E.Encoded([[fill(0), ent(first + 3)], [ent(first + 1, b"o")]], t)


T16 = table_of(16)


def tiles(n, refs, cuts=()):
    """n headers in sections cut at `cuts`, all literals but those at `refs`
    (full matches of entry i % 16)"""
    hs = [ent(i % 16) if i in refs else fill(i) for i in range(n)]
    b = [0] + list(cuts) + [n]
    return E.Encoded([hs[x:y] for x, y in zip(b, b[1:])], T16)


def choice_cases():
    dup = D.Table([ent(0), ent(1), ent(0), ent(2), ent(0), ent(3)], 0, 8)
    one_name = D.Table([(b"x-same", b"val%02d" % k) for k in range(50)], 0, 64)
    mixed = D.Table([(b"x-abc", b"12345"), (b"x-abcd", b"1"),
                     (b"x-e", b""), (b":method", b"GET"),
                     (b":path", b"/dyn"), (b"x-abc", b"1234"),
                     (b"x-abc", b"12346")], 0, 8)
    q = [ent(0), ent(0, b"other")]
    return {
        # the equal entries 0, 2, 4: windows without the newest, the oldest,
        # all of them, and with two of them
        "dup": E.Encoded([q] * 6, dup, [(0, 6), (0, 4), (1, 6), (1, 2),
                                        (3, 4), (2, 5)]),
        "one_name": E.Encoded(
            [[(b"x-same", b"val33"), (b"x-same", b"none")]] * 3, one_name,
            [(0, 50), (34, 50), (7, 33)]),
        "mixed": E.Encoded([[
            (b"x-ab", b"12345"), (b"x-abcde", b"1"),     # prefix / longer name
            (b"x-abc", b"12346"), (b"x-abc", b"12347"),  # last byte
            (b"x-abc", b"1234"), (b"x-abc", b"123456"),  # only the length
            (b"x-e", b""), (b"x-e", b"v"), (b"", b""),   # empty value
            (b":method", b"GET"),                        # static wins: full
            (b":path", b"/dyn"),                         # dynamic full first
            (b":path", b"/other")]], mixed),             # static name wins
    }


def _search(want, slots, what, start=0):
    """the first `want` (k, name, value) from k = start on whose name hash
    (what = 1) or name+value hash (2) falls in slot slots - 1"""
    out, k = [], start
    while len(out) < want:
        nm, v = b"x-s%d" % k, b"c"
        h1 = HM.xxh32(nm, HM.SEED)
        h = h1 if what == 1 else HM.xxh32(v, h1)
        if h & (slots - 1) == slots - 1:
            out.append((nm, v))
        k += 1
        assert k < start + 20000
    return out


@functools.lru_cache(maxsize=None)
def index_cases():
    import oracle_lib as O
    assert HM.xxh32(b"abc", 7) == O.xxh32(b"abc", 7)
    out = {}
    slots = qhuff.dyn_index_slots(8)
    assert slots == 64 == qhuff.dyn_index_slots(32)
    assert qhuff.dyn_index_slots(33) == 128 == qhuff.dyn_index_slots(64)
    # four entries each whose hashes fall in the last slot of either index:
    # their probe runs wrap the array's end
    by_name = _search(4, slots, 1)
    by_nv = _search(4, slots, 2, 10000)
    t = D.Table(by_name + by_nv, 5, 8)
    qs = [x for e in by_name + by_nv for x in (e, (e[0], b"other"))]
    out["collide_wrap"] = E.Encoded([qs, qs], t, [(5, 13), (7, 11)])
    for d in (1, 2, 32, 33):
        t = table_of(d, 3)
        out["d%d" % d] = E.Encoded(
            [[ent(0), ent(d - 1), ent(d), ent(d // 2, b"o"), fill(d)]], t)
    t = table_of(300, 1000, 128)
    out["d300_mid"] = E.Encoded(
        [[ent(k) for k in (0, 85, 86, 150, 213, 214, 299)]
         + [ent(k, b"o") for k in (85, 86, 213, 214)]], t, [(1086, 1214)])
    return out


BIG_V = bytes(range(256)) * 28               # 7 KB: past kHashCap (6 KB)


@functools.lru_cache(maxsize=None)
def reader_cases():
    t = D.Table([ent(0), (b"x-big", BIG_V), ent(2),
                 (b"x-big2", BIG_V[:-1] + b"!")], 0, 8)
    small = [fill(i) if i % 5 else ent(2) for i in range(64)]
    big = [fill(i) for i in range(60)] + [(b"x-big", BIG_V), ent(0),
                                          (b"x-big2", BIG_V),
                                          (b"x-big", BIG_V[:-1])]
    return {"unstaged": E.Encoded([big], t),
            "staged_then_not": E.Encoded([small + big[:30], big[30:] + small],
                                         t)}


@functools.lru_cache(maxsize=None)
def tile_cases():
    out = {}
    for n in (63, 64, 65, 127, 128, 129):
        out["n%d" % n] = tiles(n, {0, n - 1}, (n // 2,))
    for name, at in (("first", 0), ("last", 191), ("middle", 100)):
        out["three_tiles_" + name] = tiles(192, {at})
    # two sections meeting on a tile edge, references either side; empty
    # sections between them and behind n
    out["edge_meet"] = tiles(160, {62, 63, 64, 65, 159},
                             (10, 64, 64, 64, 100, 160, 160))
    out["sections_200"] = tiles(200, set(range(0, 200, 3)), range(1, 200))
    out["one_of_5000"] = tiles(5000, {3777})
    return out


def all_cases():
    c = {"forms": all_forms(), "int_edges": int_edges(),
         "rfc_a": rfc_cases()[0][0], "rfc_b": rfc_cases()[1][0]}
    for f in range(3, 13):
        c["ric_wrap_%d" % f] = ric_wrap(f)
    c.update(choice_cases())
    c.update(index_cases())
    c.update(reader_cases())
    c.update(tile_cases())
    return c


CASES = sorted(["forms", "int_edges", "rfc_a", "rfc_b", "dup", "one_name",
                "mixed", "collide_wrap", "d1", "d2", "d32", "d33", "d300_mid",
                "unstaged", "staged_then_not", "n63", "n64", "n65", "n127",
                "n128", "n129", "three_tiles_first", "three_tiles_last",
                "three_tiles_middle", "edge_meet", "sections_200",
                "one_of_5000"] + ["ric_wrap_%d" % f for f in range(3, 13)])


@functools.lru_cache(maxsize=None)
def case(name):
    c = all_cases()
    assert sorted(c) == CASES
    return c[name]


def test_cases_are_what_they_claim():
    f = case("forms")
    assert set(f.want_kind.tolist()) == {IDX, NREF, LIT, IDX | DYN, NREF | DYN}
    first = [E.line(h[0], h[1], h[2], f.table, 0, 8, 4)[0][0]
             for h in f.h.sections[0]]
    assert first[0] & 0xC0 == 0xC0 and first[9] & 0xF0 == 0x20 \
        and first[10] & 0xF0 == 0x30
    assert first[1:9] + first[11:] == [0x82, 0x12, 0x51, 0x71, 0x41, 0x61,
                                       0x01, 0x09, 0x82]
    ie = case("int_edges")
    secs = ie.want_sections
    assert [len(s) for s in secs[0:3]] == [3, 4, 4]      # 62 | 63 +0 | 63 +1
    assert [s[1] for s in secs[12:15]] == [126, 127, 127]
    assert [s[1] for s in secs[15:18]] == [0x80 | 126, 0xFF, 0xFF]
    assert [s[0] for s in secs[18:21]] == [254, 255, 255]
    assert len(secs[20]) == len(secs[18]) + 1
    encs = [case("ric_wrap_%d" % k).want_sections[0][0] for k in range(3, 13)]
    assert encs == [(k + 4) % 8 + 1 for k in range(3, 13)] and 1 in encs
    d = case("dup")
    assert d.want_dyn.tolist()[0::2] == [4, 2, 4, D.DYN_NONE, D.DYN_NONE, 4]
    assert d.want_dyn.tolist()[1::2] == [0, 0, 2, D.DYN_NONE, D.DYN_NONE, 2]
    o = case("one_name")
    assert o.want_dyn.tolist() == [33, 0, 34, 34, 7, 7]
    assert o.want_kind.tolist() == [IDX | DYN] + [NREF | DYN] * 5
    m = case("mixed")
    assert m.want_kind.tolist() == [LIT, LIT, IDX | DYN, NREF | DYN,
                                    IDX | DYN, NREF | DYN, IDX | DYN,
                                    NREF | DYN, LIT, IDX, IDX | DYN, NREF]
    cw = case("collide_wrap")
    assert (cw.want_dyn[:16] != D.DYN_NONE).all()
    assert (cw.want_dyn[16:] != D.DYN_NONE).sum() == 8
    u = case("unstaged")
    assert u.want_kind.tolist()[-4:] == [IDX | DYN, IDX | DYN, NREF | DYN,
                                         NREF | DYN]
    assert (case("one_of_5000").want_dyn != D.DYN_NONE).sum() == 1
    assert case("edge_meet").m == 8 and case("sections_200").m == 200


def sections_pairs(e):
    return [[(h[0], h[1]) for h in s] for s in e.h.sections]


@pytest.mark.parametrize("name", CASES)
def test_cpu_lookup_equals_model(name):
    """qhuff_dyn_lookup_cpu, section by section in the section's window: the
    two hashes, kind, static_id and dyn_id are the model's"""
    e = case(name)
    for pairs, (lo, hi) in zip(sections_pairs(e), e.wins):
        if not pairs:
            continue
        data, off = HM.pack_pairs(pairs)
        got = qhuff.dyn_lookup_cpu(data, off, e.tab, (lo, hi))
        assert got[0] == qhuff.OK
        for g, w in zip(got[1:], E.lookup(pairs, e.table, lo, hi)):
            assert np.array_equal(g, w)


def test_cpu_lookup_on_the_interop_lists_and_static_vectors():
    for name in sorted(D.INTEROP):
        r, e = interop_sections(name)
        for pairs, (lo, hi) in zip(sections_pairs(e), e.wins):
            data, off = HM.pack_pairs(pairs)
            got = qhuff.dyn_lookup_cpu(data, off, e.tab, (lo, hi))
            assert got[0] == qhuff.OK
            for g, w in zip(got[1:], E.lookup(pairs, e.table, lo, hi)):
                assert np.array_equal(g, w)
    # without a table, with max_entries = 0 and with an empty window it is
    # the static lookup
    pairs = HM.near_miss_pairs()
    data, off = HM.pack_pairs(pairs)
    want = qhuff.static_lookup_cpu(data, off)
    t = table_of(8)
    for tab, win in (((None, None, 0, 8), None),
                     ((t.data, t.off, 0, 0), None),
                     ((t.data, t.off, 0, 8), (3, 3))):
        got = qhuff.dyn_lookup_cpu(data, off, tab, win)
        assert got[0] == qhuff.OK and (got[5] == D.DYN_NONE).all()
        for g, w in zip(got[1:5], want):
            assert np.array_equal(g, w)


def test_cpu_lookup_errors():
    t = table_of(8, 4)
    data, off = HM.pack_pairs([ent(1)])
    tab = (t.data, t.off, 4, 8)
    for win in ((3, 8), (6, 5), (4, 13)):
        assert qhuff.dyn_lookup_cpu(data, off, tab, win)[0] == qhuff.EINVAL
    assert qhuff.dyn_lookup_cpu(data, off, (t.data, t.off, 4, 4),
                                (4, 9))[0] == qhuff.EINVAL      # wider than 4
    bad = t.off.copy()
    bad[3] = bad[2] - 1
    assert qhuff.dyn_lookup_cpu(data, off, (t.data, bad, 4, 8))[0] \
        == qhuff.EINVAL
    assert qhuff.dyn_lookup_cpu(data, off, (t.data, t.off, 0xFFFFFFF9, 8))[0] \
        == qhuff.ERANGE


def test_lookup_source_under_sanitizers(tmp_path):
    """tests/c/lookup_dyn_san.cpp with its own main, g++ ASan + UBSan, run as
    a child process: the index build and the lookup over exactly-sized heap
    buffers, on the rule's inputs and on windows, Bases and offsets outside
    it (the clamps)"""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed for the sanitizer build"
    exe = str(tmp_path / "lookup_dyn_san")
    subprocess.run(
        [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=all", "-o", exe,
         os.path.join(HERE, "c", "lookup_dyn_san.cpp"),
         os.path.join(ROOT, "ls-qpack_amd", "csrc", "qhuff_frames.cpp")],
        check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2000:])
    assert "ok" in r.stdout


# ---- GPU -------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def codec():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("gpu test without a GPU")
    c = qhuff.Codec(0)
    yield c
    c.close()


def check_encoded(e, got):
    ret, out, so, kind, sid, did = got
    assert ret == qhuff.OK
    assert np.array_equal(so, e.want_sec_out)
    assert out.tobytes() == e.want
    assert np.array_equal(kind, e.want_kind)
    assert np.array_equal(sid, e.want_id)
    assert np.array_equal(did, e.want_dyn)


def read_back(codec, e, out, so):
    """qhuff_decode_headers_dyn_host on the output, same table and windows"""
    res = codec.decode_headers_dyn_host(out, so, e.tab, e.sec_win,
                                        max_hdrs=max(e.n, 1))
    assert res[0] == qhuff.OK and not res[2].any()
    assert np.array_equal(res[1], e.sec_hdr)
    assert np.array_equal(res[3], e.want_kind)
    assert np.array_equal(res[4], e.want_id)
    assert np.array_equal(res[6], e.want_dyn)
    assert res[7].tobytes() == e.data.tobytes()
    assert np.array_equal(res[8], e.off) and not res[9].any()


def check_host(codec, e):
    got = codec.encode_headers_dyn_host(e.data, e.off, e.sec_hdr, e.tab,
                                        e.sec_win, e.sec_base, e.hflags)
    check_encoded(e, got)
    read_back(codec, e, got[1], got[2])


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_cases(codec, name):
    """every form, the integer edges, the RIC's wrap and its reduction
    across tiles and sections, the choice among entries, the index's
    collisions, wrap and sizes, the readers: against the model and read
    back"""
    check_host(codec, case(name))


def dev(a, dtype=None):
    import torch
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a.copy()).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["forms", "edge_meet", "d300_mid"])
def test_device_form_and_lookup(codec, name):
    """the device-pointer calls on torch tensors, and qhuff_dyn_lookup /
    _host section by section in the section's window"""
    import torch
    e = case(name)
    t = e.table
    res = codec.encode_headers_dyn(dev(e.data), dev(e.off), dev(e.sec_hdr),
                                   dev(t.data), dev(t.off), t.first,
                                   t.max_entries, dev(e.sec_win),
                                   dev(e.sec_base), dev(e.hflags))
    torch.cuda.synchronize()
    assert codec.device_error() == 0
    out, so, kind, sid, did = [x.cpu().numpy() for x in res]
    so, did = so.view(np.uint32), did.view(np.uint32)
    check_encoded(e, (qhuff.OK, out[:so[-1]], so, kind, sid, did))
    for pairs, (lo, hi) in zip(sections_pairs(e), e.wins):
        if not pairs:
            continue
        data, off = HM.pack_pairs(pairs)
        want = E.lookup(pairs, t, lo, hi)
        got = codec.dyn_lookup_host(data, off, e.tab, (lo, hi))
        assert got[0] == qhuff.OK
        for g, w in zip(got[1:], want):
            assert np.array_equal(g, w)
        got = codec.dyn_lookup(dev(data), dev(off), dev(t.data), dev(t.off),
                               t.first, t.max_entries, (lo, hi))
        torch.cuda.synchronize()
        for g, w in zip(got, want):
            assert np.array_equal(g.cpu().numpy().view(w.dtype), w)


@pytest.mark.gpu
def test_differential_with_the_static_call(codec):
    """d = 0, max_entries = 0 and an empty window: the bytes and arrays of
    qhuff_encode_headers_host on headers_model's near misses and reference
    vectors"""
    nm = HM.near_miss_pairs()
    secs = [nm[i:i + 100] for i in range(0, len(nm), 100)] \
        + [v[1] for v in HM.reference_vectors()]
    h = HM.Headers(secs)
    want = codec.encode_headers_host(h.data, h.off, h.sec_hdr, h.hflags)
    assert want[0].tobytes() == h.want
    lits = [x for x in nm if HM.lookup(*x)[2] == LIT][:2]
    nref = [x for x in nm if HM.lookup(*x)[2] == NREF][:1]
    t = D.Table(lits + [(b":method", b"GET")] + nref, 2, 8)
    m = h.m
    for tab, win in (((None, None, 0, 8), None), ((None, None, 7, 0), None),
                     ((t.data, t.off, 2, 0), None),
                     ((t.data, t.off, 2, 8), [(4, 4)] * m),
                     ((t.data, t.off, 2, 8), [(2, 2)] * m)):
        sw = None if win is None else np.array(win, np.uint32).reshape(-1)
        got = codec.encode_headers_dyn_host(h.data, h.off, h.sec_hdr, tab, sw,
                                            None, h.hflags)
        assert got[0] == qhuff.OK
        assert got[1].tobytes() == want[0].tobytes()
        assert np.array_equal(got[2], want[1])
        assert np.array_equal(got[3], want[2])
        assert np.array_equal(got[4], want[3])
        assert (got[5] == D.DYN_NONE).all()
    # and with the table in view some of them become dynamic lines
    e = E.Encoded(secs, t)
    assert (e.want_dyn != D.DYN_NONE).sum() >= 3
    check_host(codec, e)


@pytest.mark.gpu
def test_interop_round_trip_on_the_device(codec):
    """the 34 sections' QIF lists in one batch per file with per-section
    windows, encoded and decoded again on the device: the QIF lists"""
    total = 0
    for name in sorted(D.INTEROP):
        r, e = interop_sections(name)
        check_host(codec, e)
        total += e.m
    assert total == 34


@pytest.mark.gpu
def test_state_between_calls(codec):
    """one context: a table with references, the same headers with d = 0,
    another table -- a stale index or an uncleared word of the Required
    Insert Count would show -- and the same sequence on two streams"""
    import torch
    a = case("edge_meet")
    none = E.Encoded(a.h.sections, D.Table([], 0, 16))
    other = E.Encoded(a.h.sections,
                      D.Table([ent(k) for k in range(15, -1, -1)], 40, 16))
    assert (none.want_dyn == D.DYN_NONE).all()
    assert not np.array_equal(other.want_dyn, a.want_dyn)
    for e in (a, none, other, a):
        check_host(codec, e)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    res = []
    for k, e in enumerate((a, none, other, a, other, none)):
        t = e.table
        with torch.cuda.stream(streams[k % 2]):
            args = [dev(x) for x in (e.data, e.off, e.sec_hdr)]
            tabs = [dev(t.data) if t.d else None, dev(t.off) if t.d else None]
        streams[k % 2].synchronize()
        res.append((e, codec.encode_headers_dyn(
            *args, *tabs, t.first, t.max_entries, hflags=dev(e.hflags),
            stream=streams[k % 2]), args, tabs))
    torch.cuda.synchronize()
    assert codec.device_error() == 0
    for e, r, _, _ in res:
        out, so, kind, sid, did = [x.cpu().numpy() for x in r]
        so, did = so.view(np.uint32), did.view(np.uint32)
        check_encoded(e, (qhuff.OK, out[:so[-1]], so, kind, sid, did))


HIGH = 0x80000000


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["edge_meet", "staged_then_not"])
def test_offsets_with_top_bit_set(codec, name):
    """header and table offsets with bit 31 set, `in` and the table's bytes
    that far before the data: device form (data at address residues 0 and
    15) and host form"""
    import torch
    e = case(name)
    t = e.table
    for r in (0, 15):
        off = (e.off.astype(np.uint64) + np.uint64(HIGH + r)).astype(np.uint32)
        toff = (t.off.astype(np.uint64) + np.uint64(HIGH + 16 + r)) \
            .astype(np.uint32)
        d = dev(np.concatenate([np.zeros(r, np.uint8), e.data,
                                np.zeros(16, np.uint8)]))
        td = dev(np.concatenate([np.zeros(16 + r, np.uint8), t.data]))
        n, m = e.n, e.m
        out = torch.empty(e.bound, dtype=torch.uint8, device="cuda")
        so = torch.empty(m + 1, dtype=torch.int32, device="cuda")
        kind, sid = (torch.empty(n, dtype=torch.uint8, device="cuda")
                     for _ in range(2))
        did = torch.empty(n, dtype=torch.int32, device="cuda")
        toff_d = dev(toff)
        tab = qhuff.DynTable(td.data_ptr() - HIGH, toff_d.data_ptr(), t.d,
                             t.first, t.max_entries)
        codec.encode_headers_dyn_into(
            Ptr(d.data_ptr() - HIGH), dev(off), n, dev(e.hflags),
            dev(e.sec_hdr), m, tab, dev(e.sec_win), dev(e.sec_base), out, so,
            kind, sid, did)
        torch.cuda.synchronize()
        assert codec.device_error() == 0
        so_h = so.cpu().numpy().view(np.uint32)
        check_encoded(e, (qhuff.OK, out[:int(so_h[-1])].cpu().numpy(), so_h,
                          kind.cpu().numpy(), sid.cpu().numpy(),
                          did.cpu().numpy().view(np.uint32)))
        # host form: it rebases by -off[0] itself
        p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        hd = np.concatenate([e.data, np.zeros(16, np.uint8)])
        htd = np.concatenate([t.data, np.zeros(16, np.uint8)])
        ht = qhuff.DynTable(htd.ctypes.data - HIGH - 16 - r,
                            toff.ctypes.data, t.d, t.first, t.max_entries)
        o = np.zeros(e.bound, np.uint8)
        s = np.zeros(m + 1, np.uint32)
        k2, i2 = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        d2 = np.zeros(n, np.uint32)
        rc = qhuff.lib().qhuff_encode_headers_dyn_host(
            codec._ctx, hd.ctypes.data - HIGH - r, p(off), n,
            p(e.hflags) if e.hflags is not None else None, p(e.sec_hdr), m,
            C.byref(ht), p(e.sec_win) if e.sec_win is not None else None,
            p(e.sec_base) if e.sec_base is not None else None, p(o), p(s),
            p(k2), p(i2), p(d2))
        check_encoded(e, (rc, o[:s[-1]], s, k2, i2, d2))


def specs(e, k, r_in):
    t = e.table
    r = lambda i: (0, 1, 3, 15)[(k + i) % 4]  # noqa: E731
    return [("in", len(e.data), r_in), ("off", 4 * (2 * e.n + 1), 4 * r(0) % 16),
            ("hflags", e.n, r(1)), ("sec_hdr", 4 * (e.m + 1), 4),
            ("tab", len(t.data), r(2)), ("tab_off", 4 * (2 * t.d + 1), 8),
            ("sec_win", 8 * e.m, 12), ("sec_base", 4 * e.m, 4),
            ("out", len(e.want), r(3)), ("sec_out", 4 * (e.m + 1), 4),
            ("kind", e.n, r(4)), ("static_id", e.n, r(5)),
            ("dyn_id", 4 * e.n, 4 * r(6) % 16)]


@pytest.mark.gpu
@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
@pytest.mark.parametrize("name", ["forms", "edge_meet", "n0m3", "n65"])
def test_buffer_contract(codec, name, host):
    """every array at its exact size and misaligned in a dirty guarded
    arena: out[0 .. sec_out[m]), sec_out and the optional arrays are written
    and nothing else; dyn_id, kind and static_id null in turn"""
    import torch
    e = {"n0m3": lambda: E.Encoded([[], [], []], T16, [(0, 16)] * 3, [5] * 3),
         "n65": lambda: E.Encoded(case("n65").h.sections, T16,
                                  [(0, 16), (2, 9)], [16, 4])}.get(
                                      name, lambda: case(name))()
    t = e.table
    opt = ("kind", "static_id", "dyn_id")
    for k, fill_ in enumerate(FILLS + FILLS[:1]):
        null = opt[k] if k < 3 else None
        ar = Arena(specs(e, k, (0, 1, 15, 7)[k]), seed=9100 + 8 * k + host)
        ar.put("in", e.data)
        ar.put("off", e.off)
        ar.put("hflags", e.hflags)
        ar.put("sec_hdr", e.sec_hdr)
        ar.put("tab", t.data)
        ar.put("tab_off", t.off)
        ar.put("sec_win", e.sec_win if e.sec_win is not None
               else np.array(e.wins, np.uint32))
        ar.put("sec_base", e.sec_base if e.sec_base is not None
               else np.array(e.bases, np.uint32))
        ar.neighbours("in", fill_)
        ar.neighbours("tab", fill_)
        ar.commit(not host)
        tab = qhuff.DynTable(ar.addr("tab"), ar.addr("tab_off"), t.d, t.first,
                             t.max_entries)
        o = lambda nme: None if nme == null else ar.addr(nme)  # noqa: E731
        args = (ar.addr("in"), ar.addr("off"), e.n, ar.addr("hflags"),
                ar.addr("sec_hdr"), e.m, C.byref(tab), ar.addr("sec_win"),
                ar.addr("sec_base"), ar.addr("out"), ar.addr("sec_out"),
                o("kind"), o("static_id"), o("dyn_id"))
        if host:
            rc = qhuff.lib().qhuff_encode_headers_dyn_host(codec._ctx, *args)
        else:
            rc = qhuff.lib().qhuff_encode_headers_dyn(codec._ctx, *args, None)
            torch.cuda.synchronize()
            assert codec.device_error() == 0
        assert rc == qhuff.OK
        img = ar.after()
        assert np.array_equal(ar.get(img, "sec_out", np.uint32),
                              e.want_sec_out)
        assert ar.get(img, "out").tobytes() == e.want
        wr = {"out": len(e.want), "sec_out": 4 * (e.m + 1)}
        for nme, w, dt in (("kind", e.want_kind, np.uint8),
                           ("static_id", e.want_id, np.uint8),
                           ("dyn_id", e.want_dyn, np.uint32)):
            if nme != null:
                assert np.array_equal(ar.get(img, nme, dt), w)
                wr[nme] = w.nbytes
        ar.check(img, wr)


@pytest.mark.gpu
def test_host_form_errors(codec):
    """each QHUFF_EINVAL / QHUFF_ERANGE clause, with nothing written"""
    e = case("n65")
    t = e.table
    L = qhuff.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    out = np.full(e.bound, 0xA5, np.uint8)
    so = np.full(e.m + 1, 0xA5A5A5A5, np.uint32)
    kind, sid = np.full(e.n, 0xA5, np.uint8), np.full(e.n, 0xA5, np.uint8)
    did = np.full(e.n, 0xA5A5A5A5, np.uint32)
    good = dict(ctx=codec._ctx, data=p(e.data), off=e.off, n=e.n,
                fl=p(e.hflags), sh=e.sec_hdr, m=e.m,
                tab=(t.data, t.off, t.first, t.max_entries, True),
                win=None, base=None, out=p(out), so=p(so))

    def call(**kw):
        a = dict(good, **kw)
        td, toff, first, me, have = a["tab"]
        tab = qhuff.DynTable(td.ctypes.data if td is not None else None,
                             toff.ctypes.data if toff is not None else None,
                             (len(t.off) - 1) // 2, first, me)
        opt = lambda x: None if x is None else p(np.ascontiguousarray(  # noqa: E731
            x, dtype=np.uint32))
        keep = [opt(a["off"]), opt(a["sh"]), opt(a["win"]), opt(a["base"])]
        return L.qhuff_encode_headers_dyn_host(
            a["ctx"], a["data"], keep[0], a["n"], a["fl"], keep[1], a["m"],
            C.byref(tab) if have else None, keep[2], keep[3], a["out"],
            a["so"], p(kind), p(sid), p(did))

    assert call() == qhuff.OK
    out[:] = 0xA5
    so[:] = 0xA5A5A5A5
    kind[:] = sid[:] = 0xA5
    did[:] = 0xA5A5A5A5
    EI, ER = qhuff.EINVAL, qhuff.ERANGE
    whole = [(0, 16)] * e.m
    bad_off = e.off.copy()
    bad_off[5] = bad_off[4] - 1
    bad_toff = t.off.copy()
    bad_toff[7] = bad_toff[6] - 1
    sh = e.sec_hdr
    clauses = [
        (EI, dict(ctx=None)), (EI, dict(data=None)), (EI, dict(off=None)),
        (EI, dict(sh=None)), (EI, dict(out=None)), (EI, dict(so=None)),
        (EI, dict(tab=(t.data, t.off, 0, 16, False))),
        (EI, dict(tab=(None, t.off, 0, 16, True))),
        (EI, dict(tab=(t.data, None, 0, 16, True))),
        (EI, dict(off=bad_off)),
        (EI, dict(sh=[1] + sh.tolist()[1:])),
        (EI, dict(sh=sh.tolist()[:-1] + [e.n - 1])),
        (EI, dict(sh=[0, e.n, e.n - 1][:e.m + 1] if e.m == 2 else sh)),
        (EI, dict(tab=(t.data, bad_toff, 0, 16, True))),
        (EI, dict(win=[(0, 17)] + whole[1:])),          # past first + d
        (EI, dict(win=[(9, 8)] + whole[1:])),           # hi < lo
        (EI, dict(tab=(t.data, t.off, 4, 16, True),
                  win=[(3, 8)] + [(4, 20)] * (e.m - 1))),   # lo < first
        (EI, dict(tab=(t.data, t.off, 0, 8, True),
                  win=[(0, 9)] + [(0, 8)] * (e.m - 1))),    # > max_entries
        (EI, dict(tab=(t.data, t.off, 0, 8, True))),        # whole table > 8
        (EI, dict(base=[17] + [0] * (e.m - 1))),        # Base past first + d
        (ER, dict(tab=(t.data, t.off, 0xFFFFFFF0, 16, True))),
    ]
    for want, kw in clauses:
        assert call(**kw) == want, kw
        assert (out == 0xA5).all() and (so == 0xA5A5A5A5).all()
        assert (kind == 0xA5).all() and (sid == 0xA5).all()
        assert (did == 0xA5A5A5A5).all()
    # 2n + 2m past 32 bits: rejected before anything is read
    one = np.zeros(1, np.uint32)
    assert L.qhuff_encode_headers_dyn_host(
        codec._ctx, p(e.data), p(one), 0x7FFFFFFF, None, p(one), 0x7FFFFFFF,
        C.byref(qhuff.DynTable(None, None, 0, 0, 8)), None, None, p(out),
        p(so), None, None, None) == ER
    # the lookup's host form
    data, off = HM.pack_pairs([ent(1)])
    for win in ((0, 17), (5, 4)):
        assert codec.dyn_lookup_host(data, off, e.tab, win)[0] == EI
    assert codec.dyn_lookup_host(
        data, off, (t.data, t.off, 0xFFFFFFF0, 16))[0] == ER
