"""The path each tile takes, from the kernels' own record, against the layout
model (GPU).

Every other GPU test compares bytes, offsets and statuses with the oracle;
but the kernels are built from pairs of paths that give the same bytes (out
stage, big-tile slot or slow tile; staged or in units; fixed or variable
arena; dense stream or per-lane packing; a long string decoded by the wave,
or again by its lane because the wave's result was rejected), and a kernel
that takes the slow side too early still passes all of those.  The
path-trace build (libqhuff_trace.so, built by build(); QH_PATH_TRACE,
qhuff_device.h PathTrace) records per tile which side it took.  Three child
processes load it (path_trace_child.py: the full kernels, the lean ones, and
a grid of 1 % for tiles coded between pending ones), hold every launch
against the oracle first and then every tile's record against
limits.classify / classify_enc, coop_expect and workload.tile_paths.  Here:
the children's verdicts, and what the records themselves must say on the
two sides of every edge -- told apart by the kernel, not by the model.

The trace build is the product's source with the define on: this pins the
source-level decisions and the model, not the product binary's code
generation ("The path trace")."""
import json
import os
import subprocess
import sys
import time

import pytest

import _paths  # noqa: F401
import limits as L
import path_trace_child as PT

HERE = os.path.dirname(os.path.abspath(__file__))
TIMEOUT = 240               # seconds a child (a few hundred small launches)


def child_env(config):
    env = dict(os.environ)
    for k in ("QHUFF_KERNELS", "QHUFF_GRID_PCT", "QHUFF_GRID_WG_PER_CU"):
        env.pop(k, None)
    env.update(PT.CONFIGS[config])
    env["QHUFF_LIB"] = PT.trace_lib()
    return env


@pytest.fixture(scope="module")
def children(tmp_path_factory):
    """the three children, one after the other -> {config: {case: record}};
    a missing trace library, or a child that dies or runs out of time, fails
    the fixture and no further child is started"""
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("gpu test without a GPU")
    if not os.path.exists(PT.trace_lib()):
        pytest.fail("no %s: build() makes it (make trace)" % PT.trace_lib())
    out = tmp_path_factory.mktemp("path_trace")
    records, secs = {}, {}
    for config in PT.CONFIGS:
        path = str(out / (config + ".jsonl"))
        t0 = time.perf_counter()
        try:
            r = subprocess.run(
                [sys.executable, os.path.join(HERE, "path_trace_child.py"),
                 config, path], env=child_env(config), timeout=TIMEOUT,
                capture_output=True, text=True)
        except subprocess.TimeoutExpired:
            pytest.fail("child %s ran out of time (%d s)" % (config, TIMEOUT))
        secs[config] = time.perf_counter() - t0
        recs = [json.loads(l) for l in open(path)] if os.path.exists(path) \
            else []
        if r.returncode != 0:
            pytest.fail("child %s: exit status %d after %d cases (last: %r)\n%s"
                        % (config, r.returncode, len(recs), recs[-1:] or None,
                           r.stderr[-2000:]))
        records[config] = {x["id"]: x for x in recs}
    print("path_trace children, wall seconds: "
          + ", ".join("%s %.1f" % kv for kv in secs.items()))
    return records


@pytest.mark.gpu
@pytest.mark.parametrize("config", list(PT.CONFIGS))
def test_records_match_the_model(children, config):
    """every case of the child: the oracle's output, then every tile's
    record equal to the model's, field by field"""
    got = children[config]
    assert list(got) == PT.case_ids(config)
    wrong = [c["id"] for c in got.values() if not c["oracle_ok"]]
    assert not wrong, "the trace build's output differs from the oracle's"
    errors = [e for c in got.values() for e in c["errors"]]
    assert not errors, "%d fields differ:\n%s" % (len(errors),
                                                  "\n".join(errors[:60]))


def rec(children, config, cid):
    r = children[config][cid]["rec"]
    assert r is not None and r["written"] == 1, cid
    return r


def mask(lanes):
    return L._mask(lanes)


@pytest.mark.gpu
def test_decode_twins_are_told_apart(children):
    """the two sides of every decode edge by the kernel's own record (full
    kernel), at every residue the pair is run at"""
    def both(a, b, key):
        fa, fb = L.DECODE_BY_NAME[a], L.DECODE_BY_NAME[b]
        assert fa.residues == fb.residues
        return [(key(rec(children, "full", "dec/%s/%d" % (a, r))),
                 key(rec(children, "full", "dec/%s/%d" % (b, r))))
                for r in fa.residues]
    for x in both("fix66", "var67", lambda r: (r["units"], r["var"], r["path"])):
        assert x == ((1, 0, "fast"), (1, 1, "fast"))
    for x in both("out3008", "out3009", lambda r: (r["staged"], r["path"])):
        assert x == ((True, "fast"), (True, "slot"))
    for x in both("coop128", "coop129", lambda r: (r["coop"], r["fail"])):
        assert x == ((0, 0), (mask((31, 32)), 0))
    for x in both("slot12288", "slot12289", lambda r: (r["staged"], r["path"])):
        assert x == ((False, "slot"), (False, "slow"))
    for a, b in (("glob7679_lane0", "glob7680_lane0"),
                 ("glob7679_lane63_run1", "glob7679_lane63_run2")):
        for x in both(a, b, lambda r: (r["lone"], r["path"])):
            assert x == ((1, "slot"), (1, "slow"))
    a0 = rec(children, "full", "dec/arena_full/0")
    a5 = rec(children, "full", "dec/arena_full/5")
    assert (a0["staged"], a0["units"], a0["var"], a0["path"]) \
        == (True, 1, 1, "slot")
    assert (a5["staged"], a5["units"], a5["lone"], a5["path"]) \
        == (False, 2, 0, "slot")


@pytest.mark.gpu
def test_cooperative_fixtures_by_the_record(children):
    """coop63: 60..64 trips of B for the periodic strings, at most 4 for the
    random ones; coop23: 23 lanes, S = 608; no fails on a valid string (the
    numbers themselves are held against the model in the child)"""
    for f in L.DECODE:
        if f.key is None or not f.name.startswith(("coop63", "coop_k",
                                                    "coop23", "coop129")):
            continue
        for r in f.residues:
            x = rec(children, "full", "dec/%s/%d" % (f.name, r))
            assert x["coop"] != 0 and x["fail"] == 0, (f, r)
            assert x["path"] == "slot" and x["staged"], (f, r)
            if f.name.startswith("coop63"):
                assert x["coop"] == mask(f.special)
                assert x["S"] == 8 * len(f.tile[f.special[0]]) // 63
                if "rand" in f.name:
                    assert x["rounds"] <= 4, (f, r, x["rounds"])
                else:
                    assert 60 <= x["rounds"] <= 64, (f, r, x["rounds"])
            # the lean kernel leaves every string to its lane
            y = rec(children, "lean", "dec/%s/%d" % (f.name, r))
            assert (y["coop"], y["fail"], y["S"]) == (0, 0, None)
    x = rec(children, "full", "dec/coop23/0")
    assert bin(x["coop"]).count("1") == 23 and x["S"] == 608


@pytest.mark.gpu
@pytest.mark.parametrize("f", [f for f in L.DECODE if f.key is None], ids=repr)
def test_invalid_strings_fail_and_only_they(children, f):
    """every *_invalid fixture: the fail mask is its invalid cooperative
    lanes (their statuses 1: the child's oracle comparison)"""
    from test_limits import dec_case
    r = f.residues[0]
    coop = set(L.k_coop(dec_case(f, r)[5][2]))
    x = rec(children, "full", "dec/%s/%d" % (f.name, r))
    assert x["coop"] == mask(coop)
    assert x["fail"] == mask(i for i in f.special if i in coop)
    assert children["full"]["dec/%s/%d" % (f.name, r)]["oracle_ok"]


@pytest.mark.gpu
def test_encode_edges_are_told_apart(children):
    for config in ("full", "lean"):
        for mode, path in ((0, "slot" if config == "full" else "slow"),
                           (7, "fast")):
            got = [rec(children, config,
                       "enc/enc_dense%d_mode%d/0/%d" % (b, mode, mode))
                   for b in (24512, 24513, 24576, 24577)]
            assert [g["dense"] for g in got] == [1, 1, 1, 0], (config, mode)
            assert all(g["staged"] and g["units"] == 1 and g["path"] == path
                       for g in got)
    for r in (0, 5):
        x = rec(children, "full", "enc/enc_coop1024_1025/%d/0" % r)
        assert (x["path"], x["dense"], x["enc_coop"]) == ("fast", 1, 1 << 41)
        y = rec(children, "lean", "enc/enc_coop1024_1025/%d/0" % r)
        assert (y["path"], y["dense"], y["enc_coop"]) == ("fast", 1, 0)
    a = rec(children, "full", "enc/enc_out3008/0/0")
    b = rec(children, "full", "enc/enc_out3009/0/0")
    assert (a["path"], b["path"]) == ("fast", "slot")
    for r in (0, 5):
        a = rec(children, "full", "enc/enc_slot12288/%d/0" % r)
        b = rec(children, "full", "enc/enc_slot12289/%d/0" % r)
        assert (a["staged"], a["path"]) == (False, "slot")
        assert (b["staged"], b["path"]) == (False, "slow")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["decode", "encode"])
def test_a_record_does_not_depend_on_the_queue(children, kind):
    """a fixture's tile coded between pending tiles on the small grid has
    the record it has as one of five tiles spread over the grid"""
    comb = children["small"]["comb/" + kind]["rec"]
    assert comb and len(comb) >= 10
    for key, x in comb.items():
        cid = ("dec/%s" % key) if kind == "decode" else \
            "enc/%s/0" % key
        assert x == rec(children, "full", cid), key


@pytest.mark.gpu
def test_real_content_is_decoded_by_the_wave(children):
    """the inputs of test_decode_cooperative_*: cooperative strings in every
    one, failed ones only where the batch holds invalid strings"""
    got = {k: children["full"]["coop/" + k]["rec"] for k in PT.COOP_REAL}
    for k in ("token", "all", "long"):
        assert got[k]["coop_strings"] >= 24 and got[k]["failed"] == 0, k
    assert got["many"]["coop_strings"] > 300
    assert got["invalid"]["coop_strings"] == 120
    assert 20 < got["invalid"]["failed"] < 120
    assert got["all"]["max_rounds"] <= 64
