"""The host path's chunked pipeline (host_batch, qhuff_hostpath.cpp) at every
chunk cut.

qhuff_*_batch_host and the *_host_multi calls cut a batch into K string
ranges, one per 2^QHUFF_HOST_CHUNK_SHIFT bytes of input (default 23: 8 MB),
and move them on three streams with a schedule that runs one and two chunks
behind.  At the default shift K >= 2 needs 16 MB of input.  Here

  * (CPU) the plan itself, exported as qhuff_host_chunks: K at the shift's
    multiples, the cap at 16, the clamp to n, the cuts, the `small` verdict
    at its exact 4 MB boundary -- and, for every shape the GPU tests run,
    the K, the per-chunk strings, input bytes and oracle output totals its
    docstring claims (test_shapes_reach_their_paths);
  * (GPU) fresh child processes started with QHUFF_HOST_CHUNK_SHIFT=16, where
    128 KB to 1.2 MB of input reach K = 2 .. 16, the clamp, empty and
    zero-total chunks and the sliced out_off rebase (host_chunks_child.py
    has the shapes and the child).  Every call runs in a guarded, dirty
    arena with exact sizes; the child records digests of what it got, the
    tests here compare them with the CPU oracle's bytes, offsets and
    statuses.  Three children, one after the other: shift 16 with the
    default copy workers (staged, registered in / out / both, *_host_multi
    with 2 and 3 contexts), shift 16 with QHUFF_HOST_THREADS=1 (no worker
    threads), shift 21 with 3 threads (chunk copies split over them);
  * (GPU, this process, default shift) a batch either side of the 4 MB
    `small` boundary, staged and registered."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import _paths  # noqa: F401
import host_chunks_child as H
import oracle_lib as O
import qhuff

HERE = os.path.dirname(os.path.abspath(__file__))
C16, C21 = H.C16, H.C21
# a child's time limit: four times its wall time measured on MI355X
# (c16 5.8 s, c16_t1 4.1 s, c21_t3 3.2 s; the module 16.4 s), at least 60 s
TIMEOUT = {"c16": 60, "c16_t1": 60, "c21_t3": 60}


# ---- CPU: the plan --------------------------------------------------------------

def plan(off, op=0, shift=0):
    """(cut, small) of qhuff_host_chunks for an encode mode or "dec\""""
    return qhuff.host_chunks(off, op != "dec", 0 if op == "dec" else op, shift)


def raw_plan(enc, mode, off, n, shift, small=True):
    cut = np.full(17, 0xdeadbeef, dtype=np.uint32)
    sm = C.c_uint32(77)
    rc = qhuff.lib().qhuff_host_chunks(
        enc, mode, off.ctypes.data_as(C.c_void_p) if off is not None else None,
        n, shift, cut.ctypes.data_as(C.c_void_p),
        C.byref(sm) if small else None)
    return rc, cut, sm.value


@pytest.mark.parametrize("op", [0, 7, "dec"])
@pytest.mark.parametrize("shift", [16, 23])
def test_k_at_the_shifts_multiples(shift, op):
    """2C - 1, 2C, 16C - 1, 16C and 17C + 1 bytes give K = 1, 2, 15, 16, 16"""
    c = 1 << shift
    for in_bytes, want in ((2 * c - 1, 1), (2 * c, 2), (16 * c - 1, 15),
                           (16 * c, 16), (17 * c + 1, 16), (c - 1, 1), (0, 1),
                           (3 * c - 1, 2), (3 * c, 3)):
        off = H.offsets(H.spread(in_bytes, 641, shift))
        cut, small = plan(off, op, shift)
        assert len(cut) - 1 == want, (in_bytes, cut)
        assert cut == [641 * i // want for i in range(want + 1)]
        # (in_off[0] != 0 changes nothing)
        assert plan(off + np.uint32(12345), op, shift) == (cut, small)


def test_shift_out_of_range_counts_as_23():
    off = H.offsets(H.spread(5 << 23, 100, 0))
    want = plan(off, "dec", 23)
    assert len(want[0]) - 1 == 5
    for shift in (1, 15, 31, 32, 64, 0xffffffff):
        assert plan(off, "dec", shift) == want, shift
    # 16 and 30 are the first and the last accepted
    assert len(plan(H.offsets([3 << 16]), "dec", 16)[0]) - 1 == 1    # (n = 1)
    assert len(plan(H.offsets([1 << 16] * 3), "dec", 16)[0]) - 1 == 3
    assert len(plan(H.offsets([1 << 30] * 2), "dec", 30)[0]) - 1 == 2
    assert len(plan(H.offsets([1 << 30] * 2), "dec", 29)[0]) - 1 == 2  # (n = 2)
    assert len(plan(H.offsets([1 << 28] * 8), "dec", 29)[0]) - 1 == 4


def test_process_shift_is_the_environments():
    """chunk_shift 0: QHUFF_HOST_CHUNK_SHIFT as this process was started
    with, 23 without it"""
    e = os.environ.get("QHUFF_HOST_CHUNK_SHIFT")
    v = int(e, 0) if e else 23
    own = v if 16 <= v <= 30 else 23
    off = H.offsets(H.spread((3 << own) + 1, 100, 0))
    assert plan(off, "dec", 0) == plan(off, "dec", own)
    assert len(plan(off, "dec", 0)[0]) - 1 == 3


def test_more_chunks_than_strings_clamps_to_n():
    c = C16
    for lens, want in (([3 * c, 3 * c], [0, 1, 2]), ([2 * c], [0, 1]),
                       ([20 * c], [0, 1]), ([5 * c, 0, 0], [0, 1, 2, 3]),
                       ([c] * 15 + [5 * c], list(range(17))),
                       ([7 * c] * 3, [0, 1, 2, 3])):
        for op in (0, "dec"):
            assert plan(H.offsets(lens), op, 16)[0] == want, lens


def test_no_strings_is_one_chunk():
    for base in (0, 7, 0xfffffff0):
        for op in (0, 7, "dec"):
            assert plan(np.array([base], np.uint32), op, 16) == ([0, 0], True)
    rc, cut, small = raw_plan(1, 0, np.array([9], np.uint32), 0, 16)
    assert (rc, list(cut[:3]), small) == (1, [0, 0, 0xdeadbeef], 1)


def test_cuts_are_n_i_over_k():
    """monotone, cut[0] = 0, cut[K] = n, entries past K + 1 untouched"""
    rng = np.random.default_rng(5)
    for _ in range(200):
        n = int(rng.integers(1, 5000))
        in_bytes = int(rng.integers(0, 20 * C16))
        off = H.offsets(H.spread(in_bytes, n, n)) + np.uint32(rng.integers(0, 99))
        rc, cut, _ = raw_plan(0, 0, off, n, 16)
        k = max(1, min(in_bytes >> 16, 16, n))
        assert rc == k
        got = cut[:k + 1].astype(np.int64)
        assert got[0] == 0 and got[-1] == n and (np.diff(got) >= 0).all()
        assert list(got) == [n * i // k for i in range(k + 1)]
        assert (cut[k + 1:] == 0xdeadbeef).all()


def test_bad_arguments():
    off = np.array([0, 5, 9], np.uint32)
    assert raw_plan(1, 0, None, 2, 16)[0] == qhuff.EINVAL
    assert qhuff.lib().qhuff_host_chunks(1, 0, off.ctypes.data_as(C.c_void_p),
                                         2, 16, None, None) == qhuff.EINVAL
    for mode in (1, 2, 4, 6, 8):
        assert raw_plan(1, mode, off, 2, 16)[0] == qhuff.EINVAL
        assert raw_plan(0, mode, off, 2, 16)[0] == 1     # (decode: not read)
    assert raw_plan(1, 0, np.array([9, 5], np.uint32), 1, 16)[0] == qhuff.EINVAL
    assert raw_plan(1, 0, off, 2, 16, small=False)[0] == 1
    # the chunks' bounds together past 2^32 - 1: what the call itself returns
    big = H.offsets([1 << 30] * 2)
    assert raw_plan(1, 0, big, 2, 30)[0] == qhuff.ERANGE
    assert raw_plan(0, 0, big, 2, 30)[0] == 2


def test_exported_and_announced():
    assert "qhuff_host_chunks" in qhuff.EXPORTS
    hdr = open(qhuff.HEADER).read()
    assert "#define QHUFF_FEATURE_HOST_CHUNKS 1" in hdr
    assert "#define QHUFF_ABI_VERSION 7" in hdr


@pytest.mark.parametrize("op,n", [(0, 30_011), (7, 20_011), ("dec", 60_013),
                                  (0, 1), ("dec", 1)])
def test_small_flips_at_4mb(op, n):
    """`small` is K == 1 and up16(bound) <= 4 MB: the two batches whose
    rounded bounds are 4 MB and 4 MB + 16, from the bound functions"""
    x0, x1 = H.edge_bytes(op, n, False), H.edge_bytes(op, n, True)
    assert x1 == x0 + 1 < 8 << 20
    assert H.up16(H.bound_of(op, x0, n)) == 4 << 20
    assert H.up16(H.bound_of(op, x1, n)) == (4 << 20) + 16
    assert plan(H.offsets(H.spread(x0, n, 1)), op, 23) == ([0, n], True)
    assert plan(H.offsets(H.spread(x1, n, 1)), op, 23) == ([0, n], False)
    # never with two chunks, however small the bound
    assert plan(H.offsets(H.spread(2 * C16, 100, 1)), op, 16)[1] is False


# ---- the shapes, and what each is claimed to reach ------------------------------

@functools.lru_cache(maxsize=None)
def want(name, op):
    """the oracle's (out, out_off, status or None) for a shape, once"""
    data, off = H.shape(name).inputs(op)
    if op == "dec":
        return O.decode_batch(data, off)
    return O.encode_batch(data, off, op) + (None,)


@functools.lru_cache(maxsize=None)
def want_digests(name, op):
    out, oo, st = want(name, op)
    return {"total": int(oo[-1]), "out": H.digest(out), "off": H.digest(oo),
            "status": None if st is None else H.digest(st)}


def chunk_facts(name, op):
    """from the diagnostic (at the shape's shift, on the offsets the call
    gets) and the oracle: K, small, strings / input bytes / output bytes a
    chunk"""
    s = H.shape(name)
    cut, small = plan(s.call_off(), op, s.shift)
    cut = np.array(cut)
    oo = want(name, op)[1].astype(np.int64)
    off = s.off.astype(np.int64)
    return dict(K=len(cut) - 1, small=small, cut=cut,
                strings=list(np.diff(cut)),
                in_bytes=list(off[cut[1:]] - off[cut[:-1]]),
                tot=list(oo[cut[1:]] - oo[cut[:-1]]))


# name: (total input bytes, n, K, what else is claimed)
CLAIMS = {
    "k1_top": (2 * C16 - 1, 3001, 1, "small"),
    "k2_bottom": (2 * C16, 3001, 2, "strings 1500 1501"),
    "k15_top": (16 * C16 - 1, 24001, 15, "ragged"),
    "k16": (16 * C16, 24007, 16, "ragged"),
    "k16_capped": (17 * C16 + 1, 25013, 16, "ragged"),
    "clamp_n2": (6 * C16, 2, 2, "strings 1 1"),
    "clamp_n1": (2 * C16, 1, 1, "small"),
    "empty_first": (4 * C16 + 77, 4004, 4, "empty 0"),
    "empty_mid": (4 * C16 + 77, 4004, 4, "empty 2"),
    "empty_last": (4 * C16 + 77, 4004, 4, "empty 3"),
    "all_error_chunk": (3 * C16 + 1000, 4500, 3, "rejected 1"),
    "skewed": (9 * C16 + 100, 9000, 9, "skewed"),
    "sparse": (None, 200_000, 2, "strings 100000 100000"),
    "offset5": (3 * C16 + 5, 2003, 3, "back 5"),
    "high_offset": (3 * C16 + 5, 2003, 3, "back %d" % 0xF0000000),
    "corrupt1pc": (4 * C16 + 9, 6007, 4, "corrupt"),
    "big4": (4 * C21, 200_003, 4, "big"),
    "big5": (5 * C21 + 1, 250_007, 5, "big"),
    "edge_enc_small": (None, 30_011, 1, "small"),
    "edge_enc_past": (None, 30_011, 1, "past"),
    "edge_dec_small": (None, 60_013, 1, "small"),
    "edge_dec_past": (None, 60_013, 1, "past"),
}


def is_prime(n):
    return n > 1 and all(n % i for i in range(2, int(n ** 0.5) + 1))


@pytest.mark.parametrize("name", sorted(H.BUILDERS))
def test_shapes_reach_their_paths(name):
    """(CPU) every shape reaches the chunk count, the empty chunk, the
    zero-total chunk and the slice count it is for -- from qhuff_host_chunks
    and the oracle alone"""
    in_bytes, n, K, what = CLAIMS[name]
    s = H.shape(name)
    assert s.n == n and (in_bytes is None or s.in_bytes == in_bytes)
    ops = H.ops_of(name)
    for op in ops:
        assert len(s.inputs(op)[0]) == s.in_bytes    # the same plan for all
        f = chunk_facts(name, op)
        assert f["K"] == K and sum(f["strings"]) == n
        assert f["small"] == (what == "small")
        assert K == max(1, min(s.in_bytes >> s.shift, 16, n))
        bounds = [H.up16(H.bound_of(op, b, m))
                  for b, m in zip(f["in_bytes"], f["strings"])]
        assert all(t <= b for t, b in zip(f["tot"], bounds))
        # the rebase of a registered out_off runs in slices of 65,536 strings
        slices = [-(-m // H.SLICE) for m in f["strings"]]
        assert max(slices) == (2 if name == "sparse" else 1)
        if what.startswith("strings"):
            assert f["strings"] == [int(x) for x in what.split()[1:]]
        if what == "ragged":
            assert is_prime(n) and len(set(f["strings"])) == 2
            assert min(f["in_bytes"]) > 0 and min(f["tot"]) > 0
        if what.startswith("empty"):
            j = int(what.split()[1])
            assert f["strings"] == [1001] * 4
            assert [b == 0 for b in f["in_bytes"]] == [i == j for i in range(4)]
            # mode 0 and decode: nothing to bring back; mode 7: a byte a string
            assert f["tot"][j] == (1001 if op == 7 else 0)
            assert all(t > 1001 for i, t in enumerate(f["tot"]) if i != j)
        if what.startswith("rejected"):
            st = want(name, op)[2]
            assert f["strings"] == [1500] * 3 and min(f["in_bytes"]) > C16 - 500
            assert f["tot"][1] == 0 and f["tot"][0] > 0 and f["tot"][2] > 0
            assert st[1500:3000].all() and not st[:1500].any() \
                and not st[3000:].any()
        if what == "skewed":
            assert f["strings"] == [1000] * 9
            assert f["in_bytes"][0] >= 0.9 * s.in_bytes - 1
            assert bounds[0] > 40 * max(bounds[1:]) and min(f["tot"]) > 0
        if what.startswith("back"):
            assert int(s.call_off()[0]) == s.back == int(what.split()[1])
            assert int(s.call_off()[-1]) == s.back + s.in_bytes < 1 << 32
        if what == "corrupt":
            st = want(name, op)[2]
            hit = np.zeros(n, bool)
            hit[::97] = True
            assert not st[~hit].any() and st[hit].sum() >= 0.5 * hit.sum()
            oo = want(name, op)[1]
            assert (np.diff(oo.astype(np.int64))[st == 1] == 0).all()
            for i in range(K):                       # rejects in every chunk
                assert st[f["cut"][i]:f["cut"][i + 1]].any()
        if what == "big":                            # past the pool's slice
            assert min(f["in_bytes"]) > 1 << 20 and min(f["tot"]) > 1 << 20
        if what in ("small", "past") and name.startswith("edge"):
            assert H.up16(H.bound_of(op, s.in_bytes, n)) == \
                (4 << 20) + (16 if what == "past" else 0)
            # (the default shift: these run in the test process itself)
            assert s.shift == 23
    if name in ("clamp_n2", "clamp_n1"):
        # one long string a chunk: each chunk's launch is hinted `full`
        assert qhuff.batch_needs_full(s.off) == 1


# per shard of the *_host_multi calls: (strings, K) -- the shard cut by
# qhuff_shard_cuts, each shard planned from its own offsets
MULTI_CLAIMS = {
    ("k16_capped", 2): [(12379, 8), (12634, 8)],
    ("k16_capped", 3): [(8253, 5), (8320, 5), (8440, 5)],
    ("skewed", 2): [(556, 4), (8444, 4)],
    ("skewed", 3): [(371, 3), (370, 2), (8259, 2)],
    ("empty_mid", 2): [(1496, 2), (2508, 2)],
    ("empty_mid", 3): [(994, 1), (1005, 1), (2005, 1)],
    ("clamp_n2", 2): [(1, 1), (1, 1)],
    ("clamp_n2", 3): [(1, 1), (1, 1), (0, 1)],
}


@pytest.mark.parametrize("name,g", sorted(MULTI_CLAIMS))
def test_multi_shapes_reach_their_paths(name, g):
    """(CPU) the shards of the multi cases: chunked shards with unequal
    chunks (k16_capped, skewed), a shard that starts with empty strings
    (empty_mid), a shard of no strings beside one-string shards (clamp_n2,
    g = 3)"""
    s = H.shape(name)
    sc = [int(x) for x in qhuff.shard_cuts(s.off, g)]
    got = []
    for k in range(g):
        sub = s.off[sc[k]:sc[k + 1] + 1]
        for op in (0, 7, "dec"):
            cut, small = plan(sub, op, 16)
            assert small == (len(cut) == 2)      # (no bound here passes 4 MB)
        got.append((sc[k + 1] - sc[k], len(cut) - 1))
    assert got == MULTI_CLAIMS[(name, g)]
    if name == "skewed" and g == 2:
        # shard 1: its first chunk holds the heavy strings left over
        sub = s.off[sc[1]:].astype(np.int64)
        cut = plan(s.off[sc[1]:], 0, 16)[0]
        b = [sub[cut[i + 1]] - sub[cut[i]] for i in range(4)]
        assert b[0] > 10 * max(b[1:])


def test_case_lists():
    """every shift-16 shape runs staged and registered three ways in the
    first child and staged in the second; ids are unique"""
    for which, _, _ in H.CONFIGS:
        ids = H.LISTS[which]
        assert len(set(ids)) == len(ids)
        for case in ids:
            name, op, variant = case.split("/")
            assert name in H.BUILDERS and (op == "dec" or int(op) in (0, 7))
            if variant[0] == "m":
                assert variant[1] in "23" and variant[3:] in ("staged", "reg")
            else:
                assert variant in H.REGISTERED
    for name in H.SHIFT16:
        for op in H.ops_of(name):
            for v in H.SINGLE:
                assert "%s/%s/%s" % (name, op, v) in H.LISTS["c16"]
            assert "%s/%s/staged" % (name, op) in H.LISTS["c16_t1"]
    assert sum("registered_too_small" in c for c in H.LISTS["c16"]) == 1
    assert [c for _, c, _ in H.CONFIGS] == [16, 16, 21]
    assert [t for _, _, t in H.CONFIGS] == [None, 1, 3]


# ---- GPU: the children ----------------------------------------------------------

def child_env(shift, threads):
    """the parent's environment plus only the two variables"""
    env = dict(os.environ)
    env["QHUFF_HOST_CHUNK_SHIFT"] = str(shift)
    env.pop("QHUFF_HOST_THREADS", None)
    if threads is not None:
        env["QHUFF_HOST_THREADS"] = str(threads)
    return env


@pytest.fixture(scope="module")
def children(tmp_path_factory):
    """the three children, one after the other -> {list: {case: record}};
    a child that fails, dies or runs out of time fails the fixture, and no
    further child is started"""
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("gpu test without a GPU")
    out = tmp_path_factory.mktemp("host_chunks")
    records, secs = {}, {}
    for which, shift, threads in H.CONFIGS:
        path = str(out / (which + ".jsonl"))
        t0 = time.perf_counter()
        try:
            r = subprocess.run(
                [sys.executable, os.path.join(HERE, "host_chunks_child.py"),
                 which, str(shift), path],
                env=child_env(shift, threads), timeout=TIMEOUT[which],
                capture_output=True, text=True)
        except subprocess.TimeoutExpired:
            pytest.fail("child %s ran out of time (%d s)"
                        % (which, TIMEOUT[which]))
        secs[which] = time.perf_counter() - t0
        recs = [json.loads(l) for l in open(path)] if os.path.exists(path) \
            else []
        if r.returncode != 0:
            pytest.fail("child %s: exit status %d after %d records (last: %r)"
                        "\n%s" % (which, r.returncode, len(recs),
                                  recs[-1:] or None, r.stderr[-2000:]))
        records[which] = {x["id"]: x for x in recs}
    print("host_chunks children, wall seconds: "
          + ", ".join("%s %.1f" % kv for kv in secs.items()))
    return records


@pytest.mark.gpu
@pytest.mark.parametrize("which,shift,threads", H.CONFIGS,
                         ids=[c[0] for c in H.CONFIGS])
def test_child_cuts_by_its_shift(children, which, shift, threads):
    """the child's first act: qhuff_host_chunks with chunk_shift 0 agrees
    with the explicit shift, and it ran every case of its list"""
    rec = children[which]["_shift"]
    assert rec["rc"] == 0 and rec["own"] == rec["explicit"]
    assert len(rec["own"]) - 1 == 5
    assert rec["threads"] == (None if threads is None else str(threads))
    assert set(children[which]) == set(H.LISTS[which]) | {"_shift"}


CHILD_CASES = [(w, c) for w, _, _ in H.CONFIGS for c in H.LISTS[w]]


@pytest.mark.gpu
@pytest.mark.parametrize("which,case", CHILD_CASES,
                         ids=["%s-%s" % wc for wc in CHILD_CASES])
def test_chunked_call_matches_oracle(children, which, case):
    """one host-memory call of a child: QHUFF_OK, the oracle's out_off,
    bytes and statuses, no byte written outside them (guards, inputs, `out`
    past its total), no device error"""
    rec = children[which][case]
    name, op, _ = case.split("/")
    w = want_digests(name, op if op == "dec" else int(op))
    assert rec["rc"] == qhuff.OK and not any(rec["dev_err"])
    assert rec["total"] == w["total"]
    assert rec["off"] == w["off"], "out_off differs"
    assert rec["out"] == w["out"], "output bytes differ"
    assert rec.get("status") == w["status"], "statuses differ"
    assert rec["stray"] == 0, rec["stray_first"]


# ---- GPU: either side of the `small` boundary, in this process ------------------

@pytest.fixture(scope="module")
def codecs():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("gpu test without a GPU")
    cs = [qhuff.Codec(0)]
    yield cs
    for c in cs:
        c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", H.EDGES)
def test_small_boundary(codecs, name):
    """the default shift: the last batch that takes the one-synchronisation
    path (registered outputs are staged there) and the first that does not
    (registered outputs are written directly), staged and registered: the
    oracle's results and clean guards in all four"""
    s = H.shape(name)
    op, = H.ops_of(name)
    # this process cuts as the shape assumes (no variable, or 23)
    assert plan(s.call_off(), op, 0) == ([0, s.n], name.endswith("small"))
    w = want_digests(name, op)
    for k, variant in enumerate(("staged", "reg_both", "reg_out", "staged")):
        rec = H.run_case("%s/%s/%s" % (name, op, variant), k, codecs)
        assert rec["rc"] == qhuff.OK and not any(rec["dev_err"])
        assert rec["total"] == w["total"], variant
        assert rec["off"] == w["off"], variant
        assert rec["out"] == w["out"], variant
        assert rec.get("status") == w["status"], variant
        assert rec["stray"] == 0, (variant, rec["stray_first"])
