"""qhuff_scan_headers_dyn / qhuff_decode_headers_dyn / _host on the device
against the model (tests/headers_dyn_model.py), byte for byte.

The test to show: the three committed interop streams, whose sections name
dynamic entries, decode in one batch each -- every section in the window it
had at its place in the file -- to the header lists of the committed QIF
files.  Before these calls the library could give back none of them.

No test here feeds descriptors, offsets or windows outside the rule: the
walker's clamps are tested on the CPU (tests/test_scan_headers_dyn.py)."""
import ctypes as C
import random

import numpy as np
import pytest

import _paths  # noqa: F401
import headers_dyn_model as D
import qhuff
from test_buffer_contract import FILLS, Arena
from test_scan_headers_dyn import (ME, check_scan, cpu, dynamic_sections,
                                   entries, named, replay, replayed, table_arg)

MAXS = D.MAX_STRLEN


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
    a = np.array(a).view(np.uint8).reshape(-1)       # (a writable copy)
    t = torch.zeros(len(a) + pad + 16, dtype=torch.uint8, device="cuda")
    if len(a):
        t[pad:pad + len(a)] = torch.from_numpy(a).cuda()
    return t


def dev_i32(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).cuda()


def check_decode(d, got):
    out, off, st = got
    assert np.array_equal(off, d.off)
    assert np.array_equal(st, d.status)
    assert bytes(out) == d.data


def run_device(codec, d, max_len=MAXS):
    """scan + decode on device pointers; d.a0 is the wire's residue, the
    table's pad its bytes' residue (the tensor's base is 16-byte aligned)"""
    import torch
    t = d.table
    buf = dev(np.frombuffer(d.wire, dtype=np.uint8), d.a0)
    so = dev_i32(d.sec_off)
    toff = dev_i32(t.off) if t.d else None
    win = dev_i32(d.sec_win) if d.sec_win is not None else None
    dyn = torch.from_numpy(t.data.copy()).cuda() if len(t.bytes) else None
    assert dyn is None or dyn.data_ptr() % 16 == 0
    scan = codec.scan_headers_dyn(buf, so, toff, t.first, t.max_entries, win,
                                  d.n)
    dec = codec.decode_headers_dyn(buf, scan[0], d.n, dyn, t.longest, max_len,
                                   wire_bytes=len(d.wire))
    torch.cuda.synchronize()
    assert codec.device_error() == 0
    strs, hdr_off, rc, kind, sid, hf, did = scan
    out, off, st = dec
    off = off.cpu().numpy().view(np.uint32)
    n = d.n
    assert len(out) == d.bound
    return ((qhuff.OK, strs.cpu().numpy()[:32 * n],
             hdr_off.cpu().numpy().view(np.uint32), rc.cpu().numpy(),
             kind.cpu().numpy()[:n], sid.cpu().numpy()[:n],
             hf.cpu().numpy()[:n], did.cpu().numpy().view(np.uint32)[:n]),
            (out[:int(off[-1])].cpu().numpy().tobytes(), off,
             st.cpu().numpy()))


def check_host(codec, d, max_len=MAXS):
    wire = np.frombuffer(bytes(d.a0) + d.wire, dtype=np.uint8)
    ret, hdr_off, rc, kind, sid, hf, did, out, off, st, h1, h2 = \
        codec.decode_headers_dyn_host(wire, d.sec_off, table_arg(d.table),
                                      d.sec_win, max_len, d.n, hashes=True)
    check_scan(d, (ret, d.str_bytes(), hdr_off, rc, kind, sid, hf, did))
    check_decode(d, (out.tobytes(), off, st))
    g1, g2 = codec.xxh32_headers_host(
        np.concatenate([out, np.zeros(16, np.uint8)]), off)
    assert np.array_equal(h1, g1) and np.array_equal(h2, g2)
    check_scan(d, codec.scan_headers_dyn_host(wire, d.sec_off,
                                              table_arg(d.table), d.sec_win,
                                              d.n))


def check_both(codec, sections, ents, win=None, max_len=MAXS, first=0,
               pads=((0, 0), (1, 15), (15, 1)), me=ME):
    """device pointers at each (wire residue, table residue), then the host
    call; -> the model at the last residues"""
    for a0, pad in pads:
        d = D.Decoded(sections, D.Table(ents, first, me, pad=pad), win,
                      max_len, a0=a0)
        scan, dec = run_device(codec, d, max_len)
        check_scan(d, scan)
        check_decode(d, dec)
    check_host(codec, d, max_len)
    return d


# ---- the reference's own data ---------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(D.INTEROP))
def test_interop_file_decodes_to_its_qif(codec, name):
    """one batch a file, every section with its own window: the QIF's lists"""
    r, d = replay(name), replayed(name)
    wire = np.frombuffer(d.wire, dtype=np.uint8)
    ret, hdr_off, rc, kind, sid, hf, did, out, off, st = \
        codec.decode_headers_dyn_host(wire, d.sec_off, table_arg(r.table),
                                      r.sec_win, 0)
    assert ret == qhuff.OK and rc.tolist() == [qhuff.OK] * len(r.sections)
    assert not st.any()
    out = out.tobytes()
    s = [out[off[i]:off[i + 1]] for i in range(len(off) - 1)]
    hdrs = [(s[2 * i], s[2 * i + 1]) for i in range(len(s) // 2)]
    lists = [hdrs[hdr_off[i]:hdr_off[i + 1]] for i in range(len(r.sections))]
    assert lists == r.qif_lists(name)
    check_scan(d, (ret, d.str_bytes(), hdr_off, rc, kind, sid, hf, did))
    # and through the device-pointer calls
    scan, dec = run_device(codec, d, 0)
    check_scan(d, scan)
    check_decode(d, dec)


# ---- the device scan equals the _cpu form -------------------------------------------

def scan_sections(m):
    rng = random.Random(61)
    pool = dynamic_sections() + [s for n in sorted(D.INTEROP)
                                 for s in replay(n).sections]
    # (sections made for the whole table of 40, too)
    pool += [named(40), named(38, 35, D.indexed_post(1)),
             named(40, lines=D.indexed_dyn(5) + D.nameref_dyn(7, b"v"))]
    pool += [s[:-1] for s in pool[:6]] + [b"", b"\x00"]
    secs, win = [], []
    for i in range(m):
        secs.append(pool[rng.randrange(len(pool))])
        lo = rng.randrange(0, 20)
        win.append((4, 12) if i & 1 else (lo, rng.randrange(lo, 41)))
    return secs, win


T40 = D.Table(entries(40), 0, ME)


@pytest.mark.gpu
@pytest.mark.parametrize("windows", [True, False], ids=["sec_win", "whole"])
@pytest.mark.parametrize("m", [255, 256, 257])
def test_device_scan_equals_cpu(codec, m, windows):
    import torch
    secs, win = scan_sections(m)
    d = D.Decoded(secs, T40, win if windows else None, a0=5)
    assert len(set(d.rc.tolist())) >= 4 and d.n > 100
    want = cpu(d)
    check_scan(d, want)
    buf = dev(np.frombuffer(d.wire, dtype=np.uint8), d.a0)
    so, toff = dev_i32(d.sec_off), dev_i32(T40.off)
    sw = dev_i32(d.sec_win) if windows else None
    got = codec.scan_headers_dyn(buf, so, toff, 0, ME, sw, d.n)
    torch.cuda.synchronize()
    strs, hdr_off, rc, kind, sid, hf, did = [x.cpu().numpy() for x in got]
    check_scan(d, (qhuff.OK, strs, hdr_off.view(np.uint32), rc, kind, sid, hf,
                   did.view(np.uint32)))
    # max_hdrs cuts, and each optional output NULL in turn
    cap = d.n - 7
    A = 0x5A
    for null in (None, "kind", "static_id", "hflags", "dyn_id"):
        o = {"strs": torch.full((32 * cap,), A, dtype=torch.uint8, device="cuda"),
             "hdr_off": torch.zeros(m + 1, dtype=torch.int32, device="cuda"),
             "rc": torch.zeros(m, dtype=torch.int32, device="cuda"),
             "kind": torch.full((cap,), A, dtype=torch.uint8, device="cuda"),
             "static_id": torch.full((cap,), A, dtype=torch.uint8, device="cuda"),
             "hflags": torch.full((cap,), A, dtype=torch.uint8, device="cuda"),
             "dyn_id": torch.zeros(cap, dtype=torch.int32, device="cuda")}
        a = dict(o)
        if null:
            a[null] = None
        codec.scan_headers_dyn_into(buf, so, m, toff, 40, 0, ME, sw, a["strs"],
                                    cap, a["hdr_off"], a["rc"], a["kind"],
                                    a["static_id"], a["hflags"], a["dyn_id"])
        torch.cuda.synchronize()
        h = {k: v.cpu().numpy() for k, v in o.items()}
        assert np.array_equal(h["strs"], d.str_bytes(cap))
        assert np.array_equal(h["hdr_off"].view(np.uint32), d.hdr_off)
        assert np.array_equal(h["rc"], d.rc)
        for k, w in (("kind", d.kind), ("static_id", d.static_id),
                     ("hflags", d.hflags)):
            assert np.array_equal(h[k], w[:cap]) if k != null \
                else (h[k] == A).all()
        assert np.array_equal(h["dyn_id"].view(np.uint32), d.dyn_id[:cap]) \
            if null != "dyn_id" else not h["dyn_id"].any()


# ---- the decode launch ---------------------------------------------------------------

LENS = (0, 1, 3, 4, 5, 63, 64, 65, 255)


def pat(n, seed):
    return bytes((seed * 37 + 11 * i + i // 7) % 251 for i in range(n))


def len_entries(big=False):
    """names and values of every length of LENS (and one of 4 KB)"""
    e = [(pat(a, 2 * i), pat(LENS[(i + 4) % len(LENS)], 2 * i + 1))
         for i, a in enumerate(LENS)]
    e += [(b"x-last", pat(33, 99))]
    if big:
        e.insert(4, (b"big", pat(4096, 7)))
    return e


def one_section(ents, lines):
    """the lines behind one that names the table's last entry"""
    return named(len(ents)) + b"".join(lines)


def mixed_lines(ents, k, rng):
    d = len(ents)
    out = []
    for i in range(k):
        j = rng.randrange(d)
        out.append((lambda: D.indexed_dyn(d - 1 - j),
                    lambda: D.nameref_dyn(d - 1 - j, pat(rng.randrange(40), i),
                                          never=i & 1, huffman=i & 2),
                    lambda: D.indexed_static(rng.randrange(99)),
                    lambda: D.nameref_static(rng.randrange(99), pat(9, i),
                                             huffman=1),
                    lambda: D.literal(pat(rng.randrange(1, 20), i), pat(30, i),
                                      huffman=i & 1),
                    lambda: D.indexed_dyn(d - 1 - i % d))[i % 6]())
    return out


def tiles(d):
    return D.layout(d, d.a0)


@pytest.mark.gpu
def test_mixed_tiles_every_entry_length(codec):
    """tiles of 32 headers mixing WIRE (Huffman and raw), STATIC and DYN, every
    entry length, entry 0 and entry d - 1, table bytes at residues 0, 1, 15"""
    rng = random.Random(71)
    ents = len_entries()
    secs = [one_section(ents, mixed_lines(ents, 70, rng)),
            one_section(ents, [D.indexed_dyn(i) for i in range(len(ents))])]
    d = check_both(codec, secs, ents, me=64)
    assert d.rc.tolist() == [0, 0] and d.n == 71 + 1 + len(ents)
    assert {0, len(ents) - 1} <= set(d.dyn_id.tolist())
    assert set(d.strs["source"].tolist()) == {0, 1, 2}
    assert all(t["staged"] for t in tiles(d)) and tiles(d)[0]["fast"]


@pytest.mark.gpu
def test_entry_past_the_stage(codec):
    """a 4 KB entry: its tile leaves through the out-of-line path, table to
    global memory, among WIRE and STATIC strings; then a tile without it"""
    rng = random.Random(72)
    ents = len_entries(big=True)
    d0 = len(ents)
    lines = mixed_lines(ents, 20, rng) + [D.indexed_dyn(d0 - 1 - 4)] \
        + [D.nameref_dyn(d0 - 1 - 4, b"v")] + mixed_lines(ents, 50, rng)
    d = check_both(codec, [one_section(ents, lines)], ents, me=64)
    lay = tiles(d)
    assert not lay[0]["fast"] and lay[0]["staged"] and lay[0]["dyn"] >= 4096
    assert d.table.longest == 4099 and d.bound > 4099 * d.n


@pytest.mark.gpu
def test_tile_of_64_dyn_strings_and_dyn_names(codec):
    ents = len_entries()[:8]
    k = len(ents)
    # 32 indexed dynamic lines: 64 DYN strings, no wire bytes in the tile
    s0 = named(k) + b"".join(D.indexed_dyn(i % k) for i in range(31))
    # DYN names with WIRE values
    s1 = D.prefix_for(k, k, 64) + b"".join(
        D.nameref_dyn(i % k, pat(i, i), huffman=i & 1) for i in range(32))
    d = check_both(codec, [s0, s1], ents, me=64)
    assert d.n == 64 and (d.strs["source"][:64] == D.DYN_SRC).all()
    assert (d.strs["source"][64::2] == D.DYN_SRC).all()
    assert (d.strs["source"][65::2] == D.WIRE).all()


@pytest.mark.gpu
@pytest.mark.parametrize("total", [D.OUT_FAST, D.OUT_FAST + 1])
def test_out_stage_counts_dynamic_bytes(codec, total):
    """the stage's edge reached by dynamic bytes alone"""
    ents = [(pat(47, i), pat(47 + (i == 9 and total > D.OUT_FAST), i + 50))
            for i in range(32)]
    s = D.prefix_for(32, 32, 64) + b"".join(D.indexed_dyn(i) for i in range(32))
    d = check_both(codec, [s, s], ents, me=64)
    lay = tiles(d)
    assert [t["out"] for t in lay] == [total] * 2 == [t["dyn"] for t in lay]
    assert [t["fast"] for t in lay] == [total <= D.OUT_FAST] * 2


@pytest.mark.gpu
def test_limit_with_dynamic_strings(codec):
    """max_len on both sides: a DYN name + a WIRE value, an indexed dynamic
    line, and a 64-DYN tile where every value goes"""
    ents = [(pat(10, 1), pat(20, 2)), (pat(3, 3), pat(0, 4)),
            (pat(70, 5), pat(70, 6))]
    lines = [D.nameref_dyn(2, pat(5, 7)), D.indexed_dyn(2),
             D.nameref_dyn(2, pat(5, 8), huffman=1), D.indexed_dyn(1),
             D.indexed_dyn(0), D.indexed_static(2)] * 6
    sec = one_section(ents, lines)
    want = {15: 0, 14: 1, 30: 0, 29: 1, 9: 1, 140: 0, 139: 1, 69: 1}
    for max_len, first_bad in want.items():
        d = check_both(codec, [sec], ents, max_len=max_len, me=64,
                       pads=((0, 0), (3, 5)))
        st = d.status.reshape(-1, 2)
        if max_len in (15, 14):          # name 10 + value 5
            assert st[1].tolist() == [0, first_bad]
        if max_len in (30, 29):          # name 10 + value 20
            assert st[2].tolist() == [0, first_bad]
        if max_len == 9:                 # the name alone is over
            assert st[2].tolist() == [1, 1] and st[1].tolist() == [1, 0]
        if max_len in (140, 139, 69):    # 70 + 70
            assert st[0].tolist() == [max_len == 69, first_bad]


@pytest.mark.gpu
def test_large_first_and_empty_table(codec):
    k = 12
    first = (1 << 32) - 1 - k
    ins = first + k
    secs = [named(ins, lines=D.indexed_dyn(k - 1) + D.nameref_dyn(3, b"v")),
            named(ins, lines=D.indexed_dyn(k)),
            named(ins - 2, ins - 5, D.indexed_post(0))]
    d = check_both(codec, secs, entries(k), first=first)
    assert d.rc.tolist() == [D.OK, D.EPROTO, D.OK]
    d = check_both(codec, [D.prefix(0) + D.indexed_static(2)
                           + D.literal(b"a", b"b"), D.prefix(1)
                           + D.indexed_dyn(0)], [])
    assert d.rc.tolist() == [D.OK, D.EPROTO] and d.n == 2


# ---- the calls' contract ----------------------------------------------------------

def contract_case(name):
    ents = len_entries()[:6]
    if name == "n0m0":
        return [], ents
    if name == "n0m2":
        return [D.prefix(0), D.prefix_for(7, 7, 64) + D.indexed_dyn(0)], ents
    rng = random.Random(73)
    return [one_section(ents, mixed_lines(ents, 32, rng)), b"\0",
            one_section(ents, [])], ents


@pytest.mark.gpu
@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
@pytest.mark.parametrize("name", ["n0m0", "n0m2", "n34"])
def test_buffer_contract(codec, name, host):
    """every array at its exact size in a dirty guarded arena: the expected
    bytes, and nothing else written; n = 0 writes only off[0]"""
    import torch
    for k, fill in enumerate(FILLS):
        k += 3 * host
        r = (0, 1, 15)[k % 3]
        secs, ents = contract_case(name)
        t = D.Table(ents, 0, 64)
        d = D.Decoded(secs, t, a0=0)
        n, m = d.n, d.m
        assert (n, m) == {"n0m0": (0, 0), "n0m2": (0, 2), "n34": (34, 3)}[name]
        specs = [("buf", len(d.wire), r), ("sec_off", 4 * (m + 1), 4 * (k % 4)),
                 ("tab", len(t.bytes), (r + 7) % 16),
                 ("tab_off", 4 * (2 * t.d + 1), 4 * ((k + 1) % 4)),
                 ("strs", 32 * n, 4 * ((k + 1) % 4)),
                 ("hdr_off", 4 * (m + 1), 4 * ((k + 2) % 4)),
                 ("rc", 4 * m, 4 * ((k + 3) % 4)), ("kind", n, (5 * k + 2) % 16),
                 ("static_id", n, (k + 9) % 16), ("hflags", n, (3 * k + 1) % 16),
                 ("dyn_id", 4 * n, 4 * ((k + 2) % 4)),
                 ("out", len(d.data), (7 * k + 3) % 16),
                 ("off", 4 * (2 * n + 1), 4 * (k % 4)),
                 ("status", 2 * n, (k + 5) % 16), ("h1", 4 * n, 4 * (k % 4)),
                 ("h2", 4 * n, 4 * ((k + 1) % 4))]
        ar = Arena(specs, seed=9000 + 16 * k)
        ar.put("buf", np.frombuffer(d.wire, dtype=np.uint8))
        ar.put("sec_off", d.sec_off)
        ar.put("tab", t.data)
        ar.put("tab_off", t.off)
        ar.neighbours("buf", fill)
        ar.neighbours("tab", fill)
        ar.commit(not host)
        written = {"hdr_off": 4 * (m + 1), "rc": 4 * m, "kind": n,
                   "static_id": n, "hflags": n, "dyn_id": 4 * n,
                   "out": len(d.data), "off": 4 * (2 * n + 1), "status": 2 * n}
        tt = qhuff.DynTable(ar.addr("tab"), ar.addr("tab_off"), t.d, 0, 64)
        if host:
            rc = qhuff.lib().qhuff_decode_headers_dyn_host(
                codec._ctx, ar.addr("buf"), ar.addr("sec_off"), m, C.byref(tt),
                None, MAXS, n, ar.addr("hdr_off"), ar.addr("rc"),
                ar.addr("kind"), ar.addr("static_id"), ar.addr("hflags"),
                ar.addr("dyn_id"), ar.addr("out"), ar.addr("off"),
                ar.addr("status"), ar.addr("h1"), ar.addr("h2"))
            assert rc == qhuff.OK
            written.update({"h1": 4 * n, "h2": 4 * n})
        else:
            codec.scan_headers_dyn_into(
                ar.ptr("buf"), ar.ptr("sec_off"), m, ar.ptr("tab_off"), t.d, 0,
                64,
                None, ar.ptr("strs"), n, ar.ptr("hdr_off"), ar.ptr("rc"),
                ar.ptr("kind"), ar.ptr("static_id"), ar.ptr("hflags"),
                ar.ptr("dyn_id"))
            codec.decode_headers_dyn_into(ar.ptr("buf"), ar.ptr("strs"), n,
                                          MAXS, ar.ptr("tab"), len(t.bytes),
                                          ar.ptr("out"), ar.ptr("off"),
                                          ar.ptr("status"))
            torch.cuda.synchronize()
            assert codec.device_error() == 0
            written["strs"] = 32 * n
        img = ar.after()
        ar.check(img, written)
        assert np.array_equal(ar.get(img, "hdr_off", np.uint32), d.hdr_off)
        assert np.array_equal(ar.get(img, "rc", np.int32), d.rc)
        assert np.array_equal(ar.get(img, "kind"), d.kind)
        assert np.array_equal(ar.get(img, "dyn_id", np.uint32), d.dyn_id)
        assert np.array_equal(ar.get(img, "off", np.uint32), d.off)
        assert np.array_equal(ar.get(img, "status"), d.status)
        assert ar.get(img, "out").tobytes() == d.data
        if not host:
            assert np.array_equal(ar.get(img, "strs"), d.str_bytes())


@pytest.mark.gpu
def test_host_argument_checks(codec):
    d = replayed("netbsd")
    t = d.table
    wire = np.frombuffer(d.wire, dtype=np.uint8)
    ok = codec.scan_headers_dyn_host(wire, d.sec_off, table_arg(t), d.sec_win,
                                     d.n)
    check_scan(d, ok)
    off = t.off.copy()
    off[5] = off[4] - 1
    assert codec.scan_headers_dyn_host(wire, d.sec_off, (t.data, off, 0, ME),
                                       d.sec_win, d.n)[0] == qhuff.EINVAL
    win = d.sec_win.copy()
    win[6:8] = (5, 4)
    assert codec.scan_headers_dyn_host(wire, d.sec_off, table_arg(t), win,
                                       d.n)[0] == qhuff.EINVAL
    assert codec.scan_headers_dyn_host(
        wire, d.sec_off, (t.data, t.off, (1 << 32) - t.d, ME), None,
        d.n)[0] == qhuff.ERANGE
    with pytest.raises(qhuff.QhuffError):
        codec.decode_headers_dyn_host(wire, d.sec_off, table_arg(t), win, 0,
                                      d.n)
    # n > max_hdrs: nothing decoded
    r = codec.decode_headers_dyn_host(wire, d.sec_off, table_arg(t),
                                      d.sec_win, 0, d.n - 1)
    assert r[0] == qhuff.ERANGE and np.array_equal(r[1], d.hdr_off)
    check_host(codec, d, 0)
