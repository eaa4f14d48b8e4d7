"""qhuff_scan_headers on the device and through qhuff_scan_headers_host, on
the inputs only qhuff_scan_headers_cpu saw (tests/test_decode_headers.py's
CPU half): non-OK sections of every cause, sections rejected after they had
counted lines, batches past one round of the top launch, max_hdrs cuts, every
placement of the read window -- and qhuff_decode_headers on what the scan
leaves for such batches, and on descriptors outside the rule.

Expected values: tests/headers_decode_model.py (D.Decoded), one model run a
case shared by the device and the host parametrisation; never the library.
Every comparison is exact.  Every scan runs with all its buffers carved from
one dirty arena (test_buffer_contract.Arena), each at its exact size -- strs
32 * min(n, max_hdrs) bytes: the seven outputs are compared and every other
byte of the arena must be unchanged.

CPU half (unmarked): what the batches built here hold, by the model, so that
no parametrisation covers less than its name says."""
import functools
import random

import numpy as np
import pytest

import _paths  # noqa: F401
import headers_decode_model as D
import limits as L
import qhuff
import scan_cases as S
from test_buffer_contract import Arena
from test_decode_headers import (DYNAMIC, FIELD_CASES, LONG_NAME, LONG_VAL,
                                 MAXS, PROTO, TRUNC, bad_static_id_sections,
                                 check_decode, check_host, check_scan,
                                 dynamic_form_sections,
                                 every_static_id_sections, fetch_device,
                                 indexed, literal, nameref, ordinary,
                                 rc_order_cases, run_device, sec)

COUNT_CASES = tuple("count%d" % m for m in S.COUNTS)
E = qhuff
ALL_RC = {E.OK, E.ETRUNC, E.EPROTO, D.ENOTSUP}
WG = S.SCAN_BLOCK                # sections a workgroup
M3 = 3 * WG + 5                  # three full workgroups and a short fourth


# ---- batches --------------------------------------------------------------------

def double_walk():
    """-> (sections, {index: (rc, k, bytes of its last line)}): every third
    section is k good lines, k over 1 .. 40, and then one that rejects it
    -- a dynamic form,
    a static index of 99, a line cut inside its value, an integer past 64
    bits -- so the count walk has counted k lines when it gives up; the
    sections between them are OK with 0 to 20 headers"""
    rng = random.Random(31)
    dyn = list(DYNAMIC.values())
    secs, rejected = [], {}
    for i in range(M3):
        if i % 3 != 1:
            secs.append(sec(*ordinary(rng, rng.randint(0, 20))))
            continue
        j = i // 3
        k = 1 + j % 40
        bad, rc = ((dyn[j // 4 % 4], D.ENOTSUP), (indexed(99), E.EPROTO),
                   (TRUNC, E.ETRUNC), (PROTO, E.EPROTO))[(j + j // 40) % 4]
        secs.append(sec(*ordinary(rng, k), bad))
        rejected[i] = (rc, k, len(bad))
    return secs, rejected


def cut_sections():
    """M3 sections with 0 to 12 headers, one in eight of them rejected behind
    its lines; the sections each side of the second workgroup's base and one
    of the third workgroup hold five headers"""
    rng = random.Random(37)
    bads = (TRUNC, PROTO, indexed(99), DYNAMIC["nameref_t0"])
    secs = []
    for i in range(M3):
        fixed = i in (WG - 1, WG, 2 * WG + 88)
        lines = ordinary(rng, 5 if fixed else rng.randint(0, 12))
        if not fixed and rng.randrange(8) == 0:
            lines.append(bads[rng.randrange(4)])
        secs.append(sec(*lines))
    return secs


def static_forms_section():
    """one static-only section: the three line kinds with one-byte and
    multi-byte indices and lengths, Huffman and raw, N set and clear"""
    rng = random.Random(41)
    return sec(indexed(1), indexed(98), nameref(3, b"abc"),
               nameref(98, L.symbols(220, rng), 1, 1),
               literal(L.symbols(2, rng), b"value", 1, 0),
               literal(b"long-name", L.symbols(300, rng), 0, 1, 1),
               indexed(62), nameref(15, b""), literal(b"", b""))


def static_prefix_sections():
    """every prefix of static_forms_section: those that end between two lines
    are OK and have headers (S.every_prefix_sections has a Required Insert
    Count: none of its prefixes has any)"""
    return S.prefixes(static_forms_section())


def _pairs(cases):
    return [c for c, _ in cases]


BATCHES = {
    "every_static_id": every_static_id_sections,
    "bad_static_ids": bad_static_id_sections,
    "dynamic_forms": dynamic_form_sections,
    "rc_order": lambda: _pairs(rc_order_cases()),
    "double_walk": lambda: double_walk()[0],
    "cuts": cut_sections,
    "static_prefix_sections": static_prefix_sections,
}
RC_BATCHES = ("every_static_id", "bad_static_ids", "dynamic_forms",
              "rc_order", "double_walk")
PLACED = ("every_prefix_sections", "static_prefix_sections")
MIXED = ("havoc_sections", "fuzz_as_sections", "double_walk")


@functools.lru_cache(maxsize=None)
def sections(name):
    if name.startswith("count"):
        return tuple(S.counted(int(name[5:]))[1])
    if name in BATCHES:
        return tuple(BATCHES[name]())
    mode, chunks = S.CASES[name]()
    assert mode == S.FIELD
    return tuple(chunks)


@functools.lru_cache(maxsize=None)
def decoded(name, a0=0, max_len=MAXS):
    """the model's outputs for batch `name`, its first section at offset a0"""
    return D.Decoded(sections(name), max_len, a0=a0)


def caps(name):
    """the max_hdrs values of batch `name`: none and one, the count and each
    side of it, and cuts where the write kernel's workgroups meet them"""
    d = decoded(name)
    n, ho = d.n, d.hdr_off
    out = [0, 1, n - 1, n, n + 1]
    if name == "cuts":
        base = int(ho[WG])                        # the second workgroup's
        out += [base - 1, base, base + 1, int(ho[2 * WG + 88]) + 2]
    else:
        big = int(np.argmax(np.diff(ho.astype(np.int64))))
        out += [int(ho[big]) + 1, int(ho[big]) + 10000, int(ho[big + 1]) - 1]
    return out


def beside_rejected(d):
    """the headers just before and just behind each section that is not OK"""
    at = set()
    for s in np.flatnonzero(d.rc):
        at |= {int(d.hdr_off[s]) - 1, int(d.hdr_off[s])}
    return sorted(i for i in at if 0 <= i < d.n)


# ---- CPU: what the batches hold ---------------------------------------------------

@pytest.mark.parametrize("name", ("fuzz_as_sections", "havoc_sections",
                                  "double_walk", "cuts"))
def test_batches_hold_every_result(name):
    d = decoded(name)
    assert set(d.rc.tolist()) == ALL_RC
    assert d.n > 300 and beside_rejected(d)


@pytest.mark.parametrize("m", S.COUNTS)
def test_count_batches_hold_what_short_does(m):
    """S.SHORT has no dynamic form and no bad index: OK sections with no, one
    and two literals and truncated ones -- with and without headers, side by
    side, from 63 sections on"""
    d = decoded("count%d" % m)
    assert d.m == m
    if m >= 63:
        assert set(d.rc.tolist()) == {E.OK, E.ETRUNC}
        per = np.diff(d.hdr_off.astype(np.int64))
        assert set(per.tolist()) == {0, 1}
        assert (per[d.rc == 0] == 0).any()
    if m > WG * S.SCAN_TOP:
        # headers past the top launch's first round
        assert d.hdr_off[WG * S.SCAN_TOP] > 50000
    if m > WG * (S.SCAN_TOP + 1):
        assert d.hdr_off[-1] > d.hdr_off[WG * (S.SCAN_TOP + 1)] \
            > d.hdr_off[WG * S.SCAN_TOP]


def test_prefix_batches():
    """the issue's placement batch never has a header: its sections carry a
    Required Insert Count; the static-only one has, at every line's end"""
    d = decoded("every_prefix_sections")
    assert d.n == 0 and set(d.rc.tolist()) == {E.ETRUNC, D.ENOTSUP}
    d = decoded("static_prefix_sections")
    assert set(d.rc.tolist()) == {E.OK, E.ETRUNC}
    per = np.diff(d.hdr_off.astype(np.int64))
    assert sorted(set(per.tolist())) == list(range(10))
    assert set(d.kind.tolist()) == {0, 1, 2} and set(d.hflags.tolist()) == {0, 1}
    assert d.strs["huffman"].any() and (d.strs["len"] > 127).any()


def test_double_walk_model():
    """the rejected sections: k lines that are good on their own, the
    expected rc, no header; the others OK"""
    secs, rejected = double_walk()
    d = decoded("double_walk")
    assert d.m == M3 >= 3 * WG + 5 and len(rejected) == (M3 + 1) // 3
    assert {k for _, k, _ in rejected.values()} == set(range(1, 41))
    assert len({(rc, k % 4) for rc, k, _ in rejected.values()}) == 12
    per = np.diff(d.hdr_off.astype(np.int64))
    for i, s in enumerate(secs):
        if i not in rejected:
            assert d.rc[i] == 0 and 0 <= per[i] <= 20
            continue
        rc, k, tail = rejected[i]
        assert d.rc[i] == rc and per[i] == 0
        # (without its last line: OK, k headers)
        head = D.section(s[:-tail])
        assert head[0] == 0 and len(head[1]) == k
    ok = per[d.rc == 0]
    assert {0, 1, 20} <= set(ok.tolist())


def test_cut_batch_model():
    d = decoded("cuts")
    per = np.diff(d.hdr_off.astype(np.int64))
    assert d.m == M3 and per.max() == 12
    assert (per[d.rc == 0] == 0).any() and (d.rc != 0).sum() > 50
    assert per[WG - 1] == per[WG] == per[2 * WG + 88] == 5
    c = caps("cuts")
    assert len(set(c)) == len(c) == 9 and max(c) == d.n + 1
    inside = c[-1]
    s = int(np.searchsorted(d.hdr_off, inside, side="right")) - 1
    assert 2 * WG <= s < 3 * WG and d.hdr_off[s] < inside < d.hdr_off[s + 1]
    # the one long lane of `skewed`
    d = decoded("skewed")
    per = np.diff(d.hdr_off.astype(np.int64))
    big = int(np.argmax(per))
    assert per[big] == 20480 and d.n == 20480 + 21
    c = caps("skewed")
    assert len(set(c)) == len(c)
    assert sum(d.hdr_off[big] < x < d.hdr_off[big + 1] for x in c) == 3


# ---- one scan in an arena --------------------------------------------------------

def run(kind, codec, d, residue=0, fill="random", max_hdrs=None,
        optional=True, strs=True, seed=1):
    """One scan of Decoded `d` by `kind` ("dev", "host", or "cpu": the
    walker's CPU form, which checks this harness): the wire bytes at
    an address of `residue` mod 16 with `fill` bytes around them, the offsets
    starting at d.a0, the other arrays at residues that vary with `seed`;
    `optional`: kind, static_id and hflags are there; `strs` False: a null
    strs (max_hdrs must be 0).  Checks the return value, the outputs and the
    arena, -> (arena, image)."""
    m, n = d.m, d.n
    cap = n if max_hdrs is None else max_hdrs
    k = min(n, cap)
    assert strs or cap == 0
    nb = k if optional else 0
    q = seed % 4
    specs = [("buf", len(d.wire), residue), ("sec_off", 4 * (m + 1), 4 * q),
             ("strs", 32 * k, 4 * ((q + 1) % 4)),
             ("hdr_off", 4 * (m + 1), 4 * ((q + 2) % 4)),
             ("rc", 4 * m, 4 * ((q + 3) % 4)), ("kind", nb, (5 * seed + 2) % 16),
             ("static_id", nb, (seed + 9) % 16),
             ("hflags", nb, (3 * seed + 1) % 16)]
    ar = Arena(specs, seed)
    ar.put("buf", np.frombuffer(d.wire, dtype=np.uint8))
    ar.put("sec_off", d.sec_off)
    ar.neighbours("buf", fill)
    ar.commit(kind == "dev")
    opt = lambda name: ar.addr(name) if optional else None  # noqa: E731
    args = (ar.addr("buf", back=d.a0), ar.addr("sec_off"), m,
            ar.addr("strs") if strs else None, cap, ar.addr("hdr_off"),
            ar.addr("rc"), opt("kind"), opt("static_id"), opt("hflags"))
    lib = qhuff.lib()
    want = E.ERANGE if n > cap else E.OK
    if kind == "cpu":
        assert lib.qhuff_scan_headers_cpu(*args) == want
    elif kind == "host":
        assert lib.qhuff_scan_headers_host(codec._ctx, *args) == want
    else:
        import torch
        assert lib.qhuff_scan_headers(codec._ctx, *args,
                                      codec._stream(None)) == E.OK
        torch.cuda.synchronize()
        assert codec.device_error() == 0
    img = ar.after()
    got_strs = ar.get(img, "strs")
    if not np.array_equal(got_strs, d.str_bytes(cap)):
        bad = int(np.flatnonzero(got_strs != d.str_bytes(cap))[0]) // 16
        raise AssertionError("descriptor %d: %r, want %r" % (
            bad, got_strs.view(D.HSTR)[bad], d.strs[bad]))
    hdr_off = ar.get(img, "hdr_off", np.uint32)
    rc = ar.get(img, "rc", np.int32)
    assert int(hdr_off[m]) == n
    if optional:
        # (the device form has no ERANGE: `want` stands for its return value)
        check_scan(d, (want, got_strs, hdr_off, rc, ar.get(img, "kind"),
                       ar.get(img, "static_id"), ar.get(img, "hflags")), cap)
    else:
        assert np.array_equal(hdr_off, d.hdr_off) and np.array_equal(rc, d.rc)
    ar.check(img, {"hdr_off": 4 * (m + 1), "rc": 4 * m, "strs": 32 * k,
                   "kind": nb, "static_id": nb, "hflags": nb})
    return ar, img


def test_cpu_harness():
    """run() itself, on the walker's CPU form: a batch of each test below"""
    run("cpu", None, decoded("count0"))
    run("cpu", None, decoded("double_walk"), residue=15, seed=2)
    for a0 in (0, 7):
        run("cpu", None, decoded("static_prefix_sections", a0),
            residue=(5 * a0) % 16, fill="ff", seed=3 + a0)
    for j, cap in enumerate(caps("cuts")):
        run("cpu", None, decoded("cuts"), max_hdrs=cap, seed=10 + j,
            optional=j % 2 == 0)
    run("cpu", None, decoded("cuts"), max_hdrs=0, optional=False, strs=False)


@pytest.fixture(scope="module")
def codec():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("gpu test without a GPU")
    c = qhuff.Codec(0)
    yield c
    assert c.device_error() == 0
    c.close()


KINDS = ("dev", "host")


# ---- the case tables ------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", FIELD_CASES + COUNT_CASES)
def test_gpu_cases(codec, name, kind):
    run(kind, codec, decoded(name), seed=len(name))


# ---- result codes, ids, the walk that runs twice ---------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", RC_BATCHES)
def test_gpu_results_and_ids(codec, name, kind):
    for r in (0, 1, 15):
        run(kind, codec, decoded(name), residue=r, seed=40 + r)


# ---- placement ------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fill", ("ff", "zero"))
@pytest.mark.parametrize("name", PLACED)
def test_gpu_placement(codec, name, fill, kind):
    """sec_off[0] at every residue a0, the data at residue 5 * a0: every
    pairing of the window's first block and the offsets, hostile bytes
    either side of the wire data"""
    for a0 in range(16):
        run(kind, codec, decoded(name, a0), residue=(5 * a0) % 16, fill=fill,
            seed=60 + a0)


# ---- max_hdrs ---------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ("cuts", "skewed"))
def test_gpu_max_hdrs(codec, name, kind):
    """strs, kind, static_id and hflags hold exactly min(n, max_hdrs) headers
    (the arena), hdr_off[m] is n whatever the cap"""
    d = decoded(name)
    for j, cap in enumerate(caps(name)):
        run(kind, codec, d, max_hdrs=cap, residue=(3 * j) % 16, seed=80 + j)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("cuts", "skewed"))
def test_gpu_max_hdrs_without_the_optional_arrays(codec, name):
    d = decoded(name)
    for j, cap in enumerate(caps(name)):
        run("dev", codec, d, max_hdrs=cap, optional=False, seed=100 + j)
    run("dev", codec, d, max_hdrs=0, optional=False, strs=False, seed=120)


# ---- mixed batches through the decode ---------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", MIXED)
def test_gpu_mixed_batch_host_call(codec, name):
    """qhuff_decode_headers_host: rc, hdr_off, the per-header arrays, out /
    off / status and the hashes -- the reference's for every header next to a
    rejected section"""
    want = decoded(name)
    assert (want.rc != 0).sum() > 30
    # (the scan alone first: a wrong descriptor fails here and is not decoded)
    run("host", codec, want, seed=130)
    d = check_host(codec, sections(name), also=beside_rejected(want))
    assert np.array_equal(d.rc, want.rc) and d.n == want.n


@pytest.mark.gpu
@pytest.mark.parametrize("max_len", (MAXS, 0, 20))
@pytest.mark.parametrize("name", MIXED)
def test_gpu_mixed_batch_decodes_where_it_is(codec, name, max_len):
    """the device scan's descriptors decoded where the scan left them"""
    import torch
    for pad in (0, 15):
        d = decoded(name, pad, max_len)
        # (the scan alone first, as above)
        run("dev", codec, d, residue=pad, seed=131)
        res = run_device(codec, d, max_len)
        torch.cuda.synchronize()
        assert codec.device_error() == 0
        scan, dec = fetch_device(d, res)
        check_scan(d, scan)
        check_decode(d, dec)
    if max_len == 20:
        assert d.status.any() and not d.status.all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("havoc_sections", "double_walk"))
def test_gpu_mixed_batch_cap_too_small(codec, name):
    """max_hdrs = n - 1: QHUFF_ERANGE, hdr_off and rc valid, out / off /
    status and the hashes as they were"""
    import ctypes as C
    d = decoded(name)
    n, m = d.n, d.m
    buf = np.frombuffer(d.wire, dtype=np.uint8)
    arrs = {"hdr_off": np.full(m + 1, 0xA5, np.uint32),
            "rc": np.full(m, 0xA5, np.int32), "kind": np.full(n, 0xA5, np.uint8),
            "sid": np.full(n, 0xA5, np.uint8), "hf": np.full(n, 0xA5, np.uint8),
            "out": np.full(D.bound(len(buf), n), 0xA5, np.uint8),
            "off": np.full(2 * n + 1, 0xA5, np.uint32),
            "st": np.full(2 * n, 0xA5, np.uint8),
            "h1": np.full(n, 0xA5, np.uint32), "h2": np.full(n, 0xA5, np.uint32)}
    before = {k: v.copy() for k, v in arrs.items()}
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    ret = qhuff.lib().qhuff_decode_headers_host(
        codec._ctx, p(buf), p(d.sec_off), m, MAXS, n - 1, p(arrs["hdr_off"]),
        p(arrs["rc"]), p(arrs["kind"]), p(arrs["sid"]), p(arrs["hf"]),
        p(arrs["out"]), p(arrs["off"]), p(arrs["st"]), p(arrs["h1"]),
        p(arrs["h2"]))
    assert ret == E.ERANGE
    assert np.array_equal(arrs["hdr_off"], d.hdr_off)
    assert np.array_equal(arrs["rc"], d.rc)
    for k in ("out", "off", "st", "h1", "h2"):
        assert np.array_equal(arrs[k], before[k]), k


# ---- descriptors outside the rule -------------------------------------------------

def masked_tile(unstaged):
    """32 headers in one tile: the longest static value and name, indexed
    lines and name references to rewrite, ordinary lines between them; a
    static string on lane 0 and on lane 63.  unstaged: a 4 KB value puts the
    tile past the stage"""
    rng = random.Random(43)
    hv = L.symbols(30, rng)
    lines = [indexed(LONG_VAL), indexed(LONG_NAME), nameref(LONG_NAME, b"v"),
             indexed(5), indexed(17), nameref(40, hv, 1), indexed(60)] \
        + ordinary(rng, 12) \
        + [nameref(1, bytes(4096 if unstaged else 9))] \
        + ordinary(rng, 11) + [indexed(98)]
    assert len(lines) == 32
    return sec(*lines)


def rewrites():
    """{string: (field, value)} inside what include/qhuff.h promises to
    tolerate (qhuff_hdrdec_impl.h hm_static: bit 0 of source; hm_value: bit 1
    of kind; hm_id: static_id clamped to 98; a STATIC string's len read as
    0).  All but the last are STATIC strings; no WIRE string's pos or len
    changes."""
    return {0: ("static_id", 99), 1: ("static_id", 255), 2: ("static_id", 200),
            6: ("source", 3), 7: ("source", 2),
            8: ("kind", D.NAME | 0xFC), 9: ("kind", D.VALUE | 0xFC),
            4: ("len", 1000), 13: ("len", 1000), 63: ("len", 1000),
            10: ("static_id", 99), 62: ("source", 3),
            # a WIRE value's kind (never read)
            11: ("kind", D.VALUE | 0xFC)}


def test_masked_tile_model():
    for unstaged in (False, True):
        d = D.Decoded([masked_tile(unstaged)])
        assert d.n == 32 and len(D.layout(d)) == 1
        assert D.layout(d)[0]["staged"] == (not unstaged)
        for s, (field, _) in rewrites().items():
            assert d.strs["source"][s] == (D.WIRE if s == 11 else D.STATIC_SRC)
        assert not d.status.any()


@pytest.mark.gpu
@pytest.mark.parametrize("unstaged", (False, True), ids=("staged", "unstaged"))
def test_gpu_masking_clause(codec, unstaged):
    """descriptors rewritten by hand inside the promise: the other strings
    keep the model's bytes and statuses, off does not decrease, a rewritten
    STATIC string has at most 53 bytes, and nothing is written outside
    out[0 .. off[2n]), off and status"""
    import torch
    d = D.Decoded([masked_tile(unstaged)])
    n = d.n
    for r, seed in ((0, 140), (15, 141)):
        # the scan's own descriptors
        ar, img = run("dev", codec, d, residue=r, seed=seed)
        strs = ar.get(img, "strs").copy().view(D.HSTR)
        for s, (field, value) in rewrites().items():
            strs[field][s] = value
        assert np.array_equal(strs["pos"], d.strs["pos"])
        wire = d.strs["source"] == D.WIRE
        assert np.array_equal(strs["len"][wire], d.strs["len"][wire])
        specs = [("buf", len(d.wire), r), ("strs", 32 * n, 4),
                 ("out", d.bound, 7), ("off", 4 * (2 * n + 1), 8),
                 ("status", 2 * n, 3)]
        ar = Arena(specs, seed + 10)
        ar.put("buf", np.frombuffer(d.wire, dtype=np.uint8))
        ar.put("strs", strs)
        ar.neighbours("buf", "ff")
        ar.commit(True)
        codec.decode_headers_into(ar.ptr("buf"), ar.ptr("strs"), n, MAXS,
                                  ar.ptr("out"), ar.ptr("off"),
                                  ar.ptr("status"))
        torch.cuda.synchronize()
        assert codec.device_error() == 0
        img = ar.after()
        off = ar.get(img, "off", np.uint32).astype(np.int64)
        st = ar.get(img, "status")
        out = ar.get(img, "out")
        assert off[0] == 0 and (np.diff(off) >= 0).all()
        assert off[-1] <= d.bound
        ar.check(img, {"out": int(off[-1]), "off": 4 * (2 * n + 1),
                       "status": 2 * n})
        for s in range(2 * n):
            if s in rewrites():
                if s != 11:
                    assert off[s + 1] - off[s] <= 53, s
                continue
            assert out[off[s]:off[s + 1]].tobytes() == d.strings[s], s
            assert st[s] == d.status[s], s
