"""Field sections and encoder streams scanned for their literals in batches:
qhuff_scan_sections (device pointers), qhuff_scan_sections_host,
qhuff_decode_sections_host and qhuff_scan_sections_cpu (the kernels' walker
source run on the host).

Expected values: tests/scan_cases.py -- the Python restatement of the
reference's framing rules (qpack_frames.ref_scan_*) per chunk, which the
host scanners are checked against there too; never the code under test.
Every call runs with all its buffers carved from one dirty arena
(test_buffer_contract.Arena), `lits` at its exact size: all five outputs are
compared byte for byte and every other byte of the arena must be unchanged.

CPU half: every case through qhuff_scan_sections_cpu, and a stand-alone
program (tests/c/scan_san.cpp + qhuff_frames.cpp, g++ with ASan/UBSan) over
the golden streams, the fuzz corpora and a seeded havoc of each.  GPU half:
the same cases through the device-pointer and the host-pointer form, the
descriptors decoded by qhuff_decode_wire where they are, and the composite
call."""
import ctypes as C
import functools
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import _paths  # noqa: F401
import qhuff
import qpack_frames as Q
import scan_cases as S
from test_buffer_contract import Arena

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIELD, STREAM = S.FIELD, S.STREAM
SMALL = ("interop_sections", "interop_encoder", "fuzz_as_sections",
         "fuzz_as_encoder", "kat_blocks", "kat_encoder",
         "every_prefix_sections", "every_prefix_stream", "kat_int_sections",
         "kat_int_stream", "int24_sections", "nonminimal_sections",
         "nonminimal_stream", "declared_sections", "declared_stream",
         "alloc_clamp", "skewed", "long_stream", "long_value",
         "havoc_sections", "havoc_stream")
BIG = ("int24_stream", "five_byte_sections")
COUNT_CASES = tuple("count%d" % m for m in S.COUNTS)


# ---- one call in an arena ----------------------------------------------------

def run(kind, codec, ex, residue=0, fill="random", max_lits=None, a0=0,
        stream=None, no_consumed=False, seed=1):
    """One scan of Expect `ex` by `kind` ("cpu", "dev" or "host"), the wire
    bytes at an address of `residue` mod 16 with `fill` bytes around them
    and the offsets starting at a0; checks the return value, the outputs
    and the arena, -> (arena, image)."""
    if a0 != ex.a0:
        raise AssertionError("Expect built for another a0")
    m, total = ex.m, ex.total
    cap = total if max_lits is None else max_lits
    specs = [("buf", len(ex.wire), residue), ("sec_off", 4 * (m + 1), 4),
             ("lits", 16 * cap, 8), ("lit_off", 4 * (m + 1), 12),
             ("rc", 4 * m, 4), ("consumed", 4 * m, 8)]
    ar = Arena(specs, seed)
    ar.put("buf", np.frombuffer(ex.wire, dtype=np.uint8))
    ar.put("sec_off", ex.sec_off)
    ar.neighbours("buf", fill)
    ar.commit(kind == "dev")
    used = None if no_consumed else ar.addr("consumed")
    args = (ar.addr("buf", back=a0), ar.addr("sec_off"), m, ex.mode,
            ar.addr("lits"), cap, ar.addr("lit_off"), ar.addr("rc"), used)
    L = qhuff.lib()
    if kind == "cpu":
        ret = L.qhuff_scan_sections_cpu(*args)
    elif kind == "host":
        ret = L.qhuff_scan_sections_host(codec._ctx, *args)
    else:
        import torch
        ret = L.qhuff_scan_sections(codec._ctx, *args,
                                    codec._stream(stream))
        (stream or torch.cuda.current_stream()).synchronize()
    if kind == "dev":
        assert ret == qhuff.OK
    else:
        assert ret == (qhuff.ERANGE if total > cap else qhuff.OK)
    img = ar.after()
    n = min(total, cap)
    assert np.array_equal(ar.get(img, "lit_off", np.uint32), ex.lit_off)
    assert np.array_equal(ar.get(img, "rc", np.int32), ex.rc)
    if not no_consumed:
        assert np.array_equal(ar.get(img, "consumed", np.uint32), ex.consumed)
    got = ar.get(img, "lits", np.uint8, 16 * n)
    if not np.array_equal(got, ex.lit_bytes(cap)):
        bad = int(np.flatnonzero(got != ex.lit_bytes(cap))[0]) // 16
        raise AssertionError("descriptor %d: %r, want %r" % (
            bad, got.view(S.LIT)[bad], ex.lits[bad]))
    ar.check(img, {"lit_off": 4 * (m + 1) if m else 4, "rc": 4 * m,
                   "consumed": 0 if no_consumed else 4 * m, "lits": 16 * n})
    return ar, img


def test_symbols_and_header():
    L = qhuff.lib()
    for name in ("qhuff_scan_sections", "qhuff_scan_sections_host",
                 "qhuff_decode_sections_host", "qhuff_scan_sections_cpu"):
        assert hasattr(L, name) and name in qhuff.EXPORTS
    with open(os.path.join(ROOT, "include", "qhuff.h")) as f:
        h = f.read()
    for name, value in (("QHUFF_FEATURE_SCAN_DEVICE", 1), ("QHUFF_KIND_SCAN", 3),
                        ("QHUFF_SCAN_FIELD_SECTION", 0),
                        ("QHUFF_SCAN_ENCODER_STREAM", 1),
                        ("QHUFF_ABI_VERSION", 7)):
        assert re.search(r"^#define\s+%s\s+%d\b" % (name, value), h, re.M), name
    assert (qhuff.KIND_SCAN, FIELD, STREAM) == (3, 0, 1)


def test_block_constants_match_the_source():
    with open(os.path.join(ROOT, "ls-qpack_amd", "csrc",
                           "qhuff_kernels.h")) as f:
        src = f.read()
    assert "constexpr uint32_t kScanBlock = %d;" % S.SCAN_BLOCK in src
    assert "constexpr uint32_t kScanTop = %d;" % S.SCAN_TOP in src


def test_fuzz_mix():
    """the statuses the model gives the 324 fuzz records as field sections:
    no status path is untested"""
    ex = S.case("fuzz_as_sections")
    assert ex.m == 324
    assert [int((ex.rc == v).sum()) for v in
            (qhuff.OK, qhuff.ETRUNC, qhuff.EPROTO)] == [290, 30, 4]
    assert S.case("interop_sections").m == 34
    assert S.case("interop_encoder").m == 31
    # the encoder-stream statuses, and chunks that end inside an instruction
    ex = S.case("fuzz_as_encoder")
    assert (ex.rc == qhuff.EPROTO).sum() == 8
    assert (ex.consumed[ex.rc == 0] < np.diff(ex.sec_off)[ex.rc == 0]).any()


# ---- CPU: the walker's logic through qhuff_scan_sections_cpu -----------------

@pytest.mark.parametrize("name", SMALL + BIG + COUNT_CASES)
def test_cpu_cases(name):
    run("cpu", None, S.case(name))


@pytest.mark.parametrize("fill", ("ff", "zero"))
@pytest.mark.parametrize("mode", ("sections", "stream"))
def test_cpu_placement(mode, fill):
    mode_, chunks = S.CASES["every_prefix_" + mode]()
    for r in range(16):
        run("cpu", None, S.Expect(mode_, chunks, a0=r), residue=(5 * r) % 16,
            fill=fill, a0=r)


@pytest.mark.parametrize("name", ("every_prefix_sections",
                                  "every_prefix_stream", "skewed"))
def test_cpu_capacity(name):
    ex = S.case(name)
    for cap in (ex.total, ex.total - 1, 0):
        run("cpu", None, ex, max_lits=cap)


def test_cpu_consumed_may_be_null_in_field_mode():
    run("cpu", None, S.case("interop_sections"), no_consumed=True)


def check_wrapper(got, ex, cap=None):
    """(ret, lits, lit_off, rc, consumed) of a Python wrapper against ex"""
    ret, lits, lit_off, rc, used = got
    assert ret == (qhuff.ERANGE if cap is not None and ex.total > cap
                   else qhuff.OK)
    assert np.array_equal(lits, ex.lit_bytes(cap))
    assert np.array_equal(lit_off, ex.lit_off) and np.array_equal(rc, ex.rc)
    assert np.array_equal(used, ex.consumed)


@pytest.mark.parametrize("name", ("every_prefix_sections",
                                  "every_prefix_stream", "count0"))
def test_cpu_python_wrapper(name):
    """qhuff.scan_sections_cpu: its own sizing (max_lits None: a count pass
    first), an exact and a short max_lits"""
    ex = S.case(name)
    src = np.frombuffer(ex.wire + bytes(16), dtype=np.uint8)
    check_wrapper(qhuff.scan_sections_cpu(src, ex.sec_off, ex.mode), ex)
    for cap in (ex.total, max(ex.total - 1, 0)):
        check_wrapper(qhuff.scan_sections_cpu(src, ex.sec_off, ex.mode, cap),
                      ex, cap)


def _args(buf, sec_off, m, mode, lits, cap, lit_off, rc, used):
    return [buf, sec_off, m, mode, lits, cap, lit_off, rc, used]


def bad_argument_calls(ar, mode=FIELD):
    """(what, argument list) of calls that must return QHUFF_EINVAL and
    write nothing: each pointer null in turn, a bad mode"""
    m = (ar.reg["sec_off"][1] // 4) - 1
    cap = ar.reg["lits"][1] // 16
    good = _args(ar.addr("buf"), ar.addr("sec_off"), m, mode,
                 ar.addr("lits"), cap, ar.addr("lit_off"), ar.addr("rc"),
                 ar.addr("consumed"))
    out = []
    for k, what in ((0, "buf"), (1, "sec_off"), (4, "lits"), (6, "lit_off"),
                    (7, "rc")):
        a = list(good)
        a[k] = None
        out.append((what + " null", a))
    a = list(good)
    a[3], a[8] = STREAM, None
    out.append(("consumed null in encoder-stream mode", a))
    for bad in (2, 7, 0xFFFFFFFF):
        a = list(good)
        a[3] = bad
        out.append(("mode %d" % bad, a))
    return out


def _arg_arena(device, decreasing=False):
    ex = S.case("interop_sections")
    specs = [("buf", len(ex.wire), 0), ("sec_off", 4 * (ex.m + 1), 4),
             ("lits", 16 * ex.total, 8), ("lit_off", 4 * (ex.m + 1), 12),
             ("rc", 4 * ex.m, 4), ("consumed", 4 * ex.m, 8)]
    ar = Arena(specs, 9)
    ar.put("buf", np.frombuffer(ex.wire, dtype=np.uint8))
    off = ex.sec_off.copy()
    if decreasing:
        off[5] = off[4] - 1
    ar.put("sec_off", off)
    return ar.commit(device)


def test_cpu_arguments():
    L = qhuff.lib()
    ar = _arg_arena(False)
    for what, a in bad_argument_calls(ar):
        assert L.qhuff_scan_sections_cpu(*a) == qhuff.EINVAL, what
    ar.check(ar.after(), {})
    ar = _arg_arena(False, decreasing=True)
    good = bad_argument_calls(ar)[0][1]
    good[0] = ar.addr("buf")
    assert L.qhuff_scan_sections_cpu(*good) == qhuff.EINVAL
    ar.check(ar.after(), {})


# ---- CPU: the stand-alone sanitizer program ----------------------------------

def _records(path, chunks):
    with open(path, "wb") as f:
        for c in chunks:
            f.write(struct.pack("<I", len(c)) + c)


def test_cpu_walker_under_sanitizers(tmp_path):
    """tests/c/scan_san.cpp with its own main, g++ ASan + UBSan: the golden
    streams, the fuzz corpora and a seeded havoc of each, packed with no
    padding in exactly-sized heap buffers"""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed for the sanitizer build"
    exe = str(tmp_path / "scan_san")
    subprocess.run(
        [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=all", "-o", exe,
         os.path.join(HERE, "c", "scan_san.cpp"),
         os.path.join(ROOT, "ls-qpack_amd", "csrc", "qhuff_frames.cpp")],
        check=True, timeout=300)
    sets = {
        "sections": S.interop_sections()[1], "encoder": S.interop_encoder()[1],
        "fuzz": S.fuzz_payloads(),
        "kats": S.kat_blocks()[1] + S.kat_encoder()[1],
        "prefix_f": S.every_prefix_sections()[1],
        "prefix_s": S.every_prefix_stream()[1],
        "ints": S.kat_int_sections()[1] + S.kat_int_stream()[1]
        + S.int24_sections()[1] + S.declared_sections()[1]
        + S.declared_stream()[1] + S.nonminimal_sections()[1],
    }
    sets["havoc_golden"] = S.havoc(sets["sections"] + sets["encoder"], 3000, 5)
    sets["havoc_fuzz"] = S.havoc(sets["fuzz"], 3000, 6)
    files = []
    for name, chunks in sets.items():
        files.append(str(tmp_path / (name + ".rec")))
        _records(files[-1], chunks)
    p = subprocess.run([exe] + files, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-4000:]
    assert p.stdout.count("chunks") == 2 * len(files)


# ---- GPU -------------------------------------------------------------------------

@pytest.fixture(scope="module")
def codec():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("gpu test without a GPU")
    c = qhuff.Codec(0)
    yield c
    assert c.device_error() == 0
    c.close()


def literals_of(ex):
    return list((qhuff.Literal * max(ex.total, 1)).from_buffer_copy(
        ex.lits.tobytes() or bytes(16)))[:ex.total]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ("dev", "host"))
@pytest.mark.parametrize("name", SMALL + BIG + COUNT_CASES)
def test_gpu_cases(codec, name, kind):
    run(kind, codec, S.case(name))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("interop_sections", "interop_encoder",
                                  "fuzz_as_sections", "fuzz_as_encoder",
                                  "kat_blocks", "kat_encoder"))
def test_gpu_descriptors_decode_where_they_are(codec, name):
    """qhuff_decode_wire on the device scan's descriptors, never copied to
    the host, against qhuff_decode_literals_ex on the host scanners'"""
    import torch
    ex = S.case(name)
    max_len = qhuff.MAX_STRLEN if ex.mode == FIELD else 0
    buf = torch.from_numpy(np.frombuffer(ex.wire + bytes(16),
                                         dtype=np.uint8).copy()).cuda()
    off = torch.from_numpy(ex.sec_off.view(np.int32)).cuda()
    lits, lit_off, rc, used = codec.scan_sections(buf, off, ex.mode,
                                                  max_lits=ex.total)
    assert int(lit_off[-1]) == ex.total
    out, out_off, status = codec.decode_wire(
        buf, lits[:16 * ex.total], max_len,
        bound=qhuff.literals_bound(ex.lit_bytes()))
    torch.cuda.synchronize()
    want, wstatus = codec.decode_literals_host(ex.wire, literals_of(ex),
                                               max_len)
    oo = out_off.cpu().numpy().view(np.uint32)
    o = out.cpu().numpy()
    assert np.array_equal(status.cpu().numpy(), wstatus)
    assert [o[oo[i]:oo[i + 1]].tobytes() for i in range(ex.total)] == want
    assert oo[0] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ("dev", "host"))
@pytest.mark.parametrize("fill", ("ff", "zero"))
@pytest.mark.parametrize("mode", ("sections", "stream"))
def test_gpu_placement(codec, mode, fill, kind):
    mode_, chunks = S.CASES["every_prefix_" + mode]()
    for r in range(16):
        run(kind, codec, S.Expect(mode_, chunks, a0=r), residue=(5 * r) % 16,
            fill=fill, a0=r)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ("dev", "host"))
@pytest.mark.parametrize("name", ("every_prefix_sections",
                                  "every_prefix_stream", "skewed"))
def test_gpu_capacity(codec, name, kind):
    ex = S.case(name)
    for cap in (ex.total, ex.total - 1, 0):
        run(kind, codec, ex, max_lits=cap)


@pytest.mark.gpu
def test_gpu_consumed_may_be_null_in_field_mode(codec):
    run("dev", codec, S.case("interop_sections"), no_consumed=True)
    run("host", codec, S.case("interop_sections"), no_consumed=True)


@pytest.mark.gpu
def test_gpu_other_stream_and_back_to_back(codec):
    """a non-default stream; then two device-form calls of different sizes
    with no host synchronisation between them (they share the scratch)"""
    import torch
    st = torch.cuda.Stream()
    run("dev", codec, S.case("every_prefix_sections"), stream=st)
    a, b = S.case("five_byte_sections"), S.case("every_prefix_stream")
    outs = []
    for ex in (a, b, a):
        buf = torch.from_numpy(np.frombuffer(ex.wire + bytes(16),
                                             dtype=np.uint8).copy()).cuda()
        off = torch.from_numpy(ex.sec_off.view(np.int32)).cuda()
        outs.append((ex, buf, off))
    torch.cuda.synchronize()
    res = [codec.scan_sections(buf, off, ex.mode, max_lits=ex.total,
                               stream=(st if k == 1 else None))
           for k, (ex, buf, off) in enumerate(outs)]
    torch.cuda.synchronize()
    for (ex, _, _), (lits, lit_off, rc, used) in zip(outs, res):
        assert np.array_equal(lit_off.cpu().numpy().view(np.uint32), ex.lit_off)
        assert np.array_equal(rc.cpu().numpy(), ex.rc)
        assert np.array_equal(used.cpu().numpy().view(np.uint32), ex.consumed)
        assert np.array_equal(lits[:16 * ex.total].cpu().numpy(),
                              ex.lit_bytes())


@pytest.mark.gpu
def test_gpu_scratch_regrows_with_work_in_flight():
    """a fresh context: a small scan allocates the scratch, a large one
    right behind it, with no synchronisation, frees and regrows it
    (scan_prepare), then a small one again"""
    import torch
    c = qhuff.Codec(0)
    cases = [S.case("every_prefix_stream"), S.case("five_byte_sections"),
             S.case("every_prefix_sections")]
    assert cases[0].m < 4096 < cases[1].m
    ins = []
    for ex in cases:
        buf = torch.from_numpy(np.frombuffer(ex.wire + bytes(16),
                                             dtype=np.uint8).copy()).cuda()
        ins.append((ex, buf, torch.from_numpy(ex.sec_off.view(np.int32)).cuda()))
    torch.cuda.synchronize()
    res = [c.scan_sections(buf, off, ex.mode, max_lits=ex.total)
           for ex, buf, off in ins]
    torch.cuda.synchronize()
    for (ex, _, _), (lits, lit_off, rc, used) in zip(ins, res):
        assert np.array_equal(lit_off.cpu().numpy().view(np.uint32), ex.lit_off)
        assert np.array_equal(rc.cpu().numpy(), ex.rc)
        assert np.array_equal(used.cpu().numpy().view(np.uint32), ex.consumed)
        assert np.array_equal(lits[:16 * ex.total].cpu().numpy(),
                              ex.lit_bytes())
    assert c.device_error() == 0
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("every_prefix_sections",
                                  "every_prefix_stream", "count0"))
def test_gpu_python_wrappers(codec, name):
    """Codec.scan_sections_host and Codec.scan_sections with their own
    sizing (max_lits None: a count pass first) and with a short max_lits"""
    import torch
    ex = S.case(name)
    src = np.frombuffer(ex.wire + bytes(16), dtype=np.uint8)
    check_wrapper(codec.scan_sections_host(src, ex.sec_off, ex.mode), ex)
    cap = max(ex.total - 1, 0)
    check_wrapper(codec.scan_sections_host(src, ex.sec_off, ex.mode, cap),
                  ex, cap)
    lits, lit_off, rc, used = codec.scan_sections(
        torch.from_numpy(src.copy()).cuda(),
        torch.from_numpy(ex.sec_off.view(np.int32)).cuda(), ex.mode)
    torch.cuda.synchronize()
    assert lits.numel() == 16 * max(ex.total, 1)
    check_wrapper((qhuff.OK, lits[:16 * ex.total].cpu().numpy(),
                   lit_off.cpu().numpy().view(np.uint32), rc.cpu().numpy(),
                   used.cpu().numpy().view(np.uint32)), ex)


@pytest.mark.gpu
def test_gpu_timing_kind(codec):
    import torch
    ex = S.case("interop_sections")
    buf = torch.from_numpy(np.frombuffer(ex.wire + bytes(16),
                                         dtype=np.uint8).copy()).cuda()
    off = torch.from_numpy(ex.sec_off.view(np.int32)).cuda()
    codec.timing(True)
    codec.scan_sections(buf, off, ex.mode, max_lits=ex.total)
    torch.cuda.synchronize()
    t = codec.timing_read()
    codec.timing(False)
    assert [k for k, _ in t] == [qhuff.KIND_SCAN] * 3
    assert all(us > 0 for _, us in t)
    L = qhuff.lib()
    assert L.qhuff_kernel_variant(codec._ctx, qhuff.KIND_SCAN) == qhuff.EINVAL
    assert L.qhuff_grid_waves(codec._ctx, qhuff.KIND_SCAN) == qhuff.EINVAL


@pytest.mark.gpu
def test_gpu_arguments(codec):
    L = qhuff.lib()
    st = codec._stream(None)
    ar = _arg_arena(True)
    for what, a in bad_argument_calls(ar):
        assert L.qhuff_scan_sections(codec._ctx, *a, st) == qhuff.EINVAL, what
    good = list(bad_argument_calls(ar)[0][1])
    good[0] = ar.addr("buf")
    assert L.qhuff_scan_sections(None, *good, st) == qhuff.EINVAL
    ar.check(ar.after(), {})
    for dec in (False, True):
        ar = _arg_arena(False, decreasing=dec)
        calls = bad_argument_calls(ar)
        if dec:
            good = list(calls[0][1])
            good[0] = ar.addr("buf")
            calls = [("decreasing offsets", good)]
        for what, a in calls:
            assert L.qhuff_scan_sections_host(codec._ctx, *a) \
                == qhuff.EINVAL, what
            out = [ar.addr("lits"), ar.addr("lit_off"), ar.addr("rc")]
            assert L.qhuff_decode_sections_host(
                codec._ctx, *a[:4], 0, *a[4:], *out) == qhuff.EINVAL, what
        ar.check(ar.after(), {})


# ---- GPU: the composite --------------------------------------------------------

@functools.lru_cache(maxsize=None)
def qif_sections(n_sections=3000, seed=77):
    """field sections of the QIF header lists, their lines framed by
    qhuff_encode_wire_host (needs a GPU), a two-byte prefix each; one in 16
    with a byte near its start set to 0xFF, one in 16 with an indexed line
    of index 2^24 (a protocol error whatever follows) in front of its first
    line, one in 16 cut short"""
    import random
    lists = []
    for name in S.STREAMS:
        lists += Q.qif_header_lists(S._read("data/%s.qif" % name))
    rng = random.Random(seed)
    strings, items, cuts = [], [], [0]
    for s in range(n_sections):
        for name, value in lists[rng.randrange(len(lists))]:
            k = rng.randrange(4)
            if k == 0:                       # indexed line
                strings.append(b"")
                items.append(qhuff.Item(rng.randrange(99), 6, 0xC0, 0, 0))
            elif k == 1:                     # literal, static name reference
                strings.append(value)
                items.append(qhuff.Item(rng.randrange(99), 4, 0x50, 7, 0))
            else:                            # literal with literal name
                strings += [name, value]
                items += [qhuff.Item(0, 0, 0, 3, 0x20),
                          qhuff.Item(0, 0, 0, 7, 0)]
        cuts.append(len(items))
    off = np.zeros(len(strings) + 1, dtype=np.uint32)
    np.cumsum([len(x) for x in strings], out=off[1:])
    data = np.frombuffer(b"".join(strings) + bytes(16), dtype=np.uint8)
    c = qhuff.Codec(0)
    out, oo = c.encode_wire_host(data, off, items)
    c.close()
    out = out.tobytes()
    chunks = []
    for s in range(n_sections):
        sec = bytearray(b"\0\0" + out[oo[cuts[s]]:oo[cuts[s + 1]]])
        if s % 16 == 3:
            sec[rng.randrange(2, min(len(sec), 40))] = 0xFF
        elif s % 16 == 7:
            sec[2:2] = Q.enc_int(0x80, 1 << 24, 6)
        elif s % 16 == 11:
            del sec[rng.randrange(2, len(sec)):]
        chunks.append(bytes(sec))
    return chunks


@functools.lru_cache(maxsize=None)
def qif_expect():
    return S.Expect(FIELD, qif_sections())


@pytest.mark.gpu
@pytest.mark.parametrize("max_len", (qhuff.MAX_STRLEN, 0))
def test_gpu_decode_sections_host(codec, max_len):
    """the whole decode path in one call against the host scanners per chunk
    followed by qhuff_decode_wire_host over the concatenated descriptors"""
    ex = qif_expect()
    assert ex.total > 10000 and (ex.rc == qhuff.OK).sum() > 2400
    # every status path: the sections with the 2^24 index, those cut short
    assert (ex.rc == qhuff.EPROTO).sum() >= ex.m // 16
    assert (ex.rc == qhuff.ETRUNC).sum() >= ex.m // 32
    src = np.frombuffer(ex.wire + bytes(16), dtype=np.uint8)
    ret, lits, lit_off, rc, used, out, out_off, status = \
        codec.decode_sections_host(src, ex.sec_off, FIELD, max_len,
                                   max_lits=ex.total)
    assert ret == qhuff.OK
    assert np.array_equal(lit_off, ex.lit_off)
    assert np.array_equal(rc, ex.rc) and np.array_equal(used, ex.consumed)
    assert np.array_equal(lits, ex.lit_bytes())
    want, wstatus = codec.decode_wire_host(ex.wire, literals_of(ex), max_len)
    assert np.array_equal(status, wstatus)
    assert out_off[0] == 0 and len(out) == out_off[-1]
    assert [out[out_off[i]:out_off[i + 1]].tobytes()
            for i in range(ex.total)] == want
    assert (wstatus == 0).sum() > 10000
    # too few descriptors: the scan's results, nothing decoded
    ret, lits, lit_off, rc, used, out, out_off, status = \
        codec.decode_sections_host(src, ex.sec_off, FIELD, max_len,
                                   max_lits=ex.total - 1)
    assert ret == qhuff.ERANGE and out is None
    assert np.array_equal(lit_off, ex.lit_off) and np.array_equal(rc, ex.rc)
    assert np.array_equal(lits, ex.lit_bytes(ex.total - 1))


@pytest.mark.gpu
def test_gpu_decode_sections_host_without_literals(codec):
    """chunks but no literal: index-only, empty and truncated sections, with
    max_lits 0 and null lits, out and status; then the wrapper's own sizing"""
    chunks = [b"\0\0\xC1", b"\0\0", b"", b"\0\0\xFF", b"\0\0\x11\x82"] * 30
    ex = S.Expect(FIELD, chunks)
    assert ex.total == 0 and (ex.rc == qhuff.ETRUNC).any()
    src = np.frombuffer(ex.wire + bytes(16), dtype=np.uint8)
    lit_off = np.full(ex.m + 1, 7, dtype=np.uint32)
    rc = np.full(ex.m, 7, dtype=np.int32)
    out_off = np.full(1, 7, dtype=np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    ret = qhuff.lib().qhuff_decode_sections_host(
        codec._ctx, p(src), p(ex.sec_off), ex.m, FIELD, qhuff.MAX_STRLEN,
        None, 0, p(lit_off), p(rc), None, None, p(out_off), None)
    assert ret == qhuff.OK and out_off[0] == 0
    assert np.array_equal(lit_off, ex.lit_off) and np.array_equal(rc, ex.rc)
    ret, lits, lit_off, rc, used, out, out_off, status = \
        codec.decode_sections_host(src, ex.sec_off, FIELD, qhuff.MAX_STRLEN)
    assert ret == qhuff.OK and len(lits) == len(out) == len(status) == 0
    assert list(out_off) == [0] and np.array_equal(used, ex.consumed)


@pytest.mark.gpu
def test_gpu_decode_sections_host_sizes_itself(codec):
    """max_lits None: the wrapper scans for the count first"""
    ex = S.case("interop_sections")
    src = np.frombuffer(ex.wire + bytes(16), dtype=np.uint8)
    ret, lits, lit_off, rc, used, out, out_off, status = \
        codec.decode_sections_host(src, ex.sec_off, FIELD, qhuff.MAX_STRLEN)
    assert ret == qhuff.OK and np.array_equal(lits, ex.lit_bytes())
    want, wstatus = codec.decode_wire_host(ex.wire, literals_of(ex),
                                           qhuff.MAX_STRLEN)
    assert np.array_equal(status, wstatus)
    assert [out[out_off[i]:out_off[i + 1]].tobytes()
            for i in range(ex.total)] == want


@pytest.mark.gpu
def test_gpu_decode_sections_host_encoder_stream(codec):
    ex = S.case("interop_encoder")
    src = np.frombuffer(ex.wire + bytes(16), dtype=np.uint8)
    ret, lits, lit_off, rc, used, out, out_off, status = \
        codec.decode_sections_host(src, ex.sec_off, STREAM, 0,
                                   max_lits=ex.total)
    assert ret == qhuff.OK and np.array_equal(lits, ex.lit_bytes())
    assert np.array_equal(used, ex.consumed)
    want, wstatus = codec.decode_wire_host(ex.wire, literals_of(ex), 0)
    assert np.array_equal(status, wstatus)
    assert [out[out_off[i]:out_off[i + 1]].tobytes()
            for i in range(ex.total)] == want
    # no chunk at all
    ret, lits, lit_off, *_ = codec.decode_sections_host(
        np.zeros(16, dtype=np.uint8), np.zeros(1, dtype=np.uint32), STREAM)
    assert ret == qhuff.OK and list(lit_off) == [0] and len(lits) == 0
