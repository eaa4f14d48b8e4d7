"""The path each tile of qhuff_decode_headers_dyn takes, read from the
path-trace build (libqhuff_trace.so) in a child process, against the layout
model (headers_dyn_model.layout): the 3008 / 3009-byte tiles whose output is
dynamic bytes alone and the tile with the 4 KB entry sit on the side the
model names, and every record's dynamic-byte count is the model's.
tests/test_decode_headers_dyn.py checks the bytes."""
import json
import os
import subprocess
import sys

import pytest

import _paths  # noqa: F401
import headers_dyn_model as D
import headers_dyn_trace_child as H

HERE = os.path.dirname(os.path.abspath(__file__))
TIMEOUT = 120


def test_cases_sit_on_their_sides():
    """the model's own verdicts for the cases (CPU)"""
    cs = H.cases()
    want = {"out3008": (True, True, 3008), "out3009": (True, False, 3009),
            "dyn64": (True, True, None)}
    for cid, (staged, fast, dyn) in want.items():
        p = D.layout(H.model(cs[cid]), cs[cid][2])
        assert len(p) == 1, cid
        assert (p[0]["staged"], p[0]["fast"]) == (staged, fast), cid
        assert p[0]["dyn"] == p[0]["out"] and dyn in (None, p[0]["dyn"]), cid
    p = D.layout(H.model(cs["entry4k"]), cs["entry4k"][2])
    assert len(p) == 1 and p[0]["staged"] and not p[0]["fast"]
    assert p[0]["dyn"] >= 4099 and p[0]["out"] > p[0]["dyn"]
    p = D.layout(H.model(cs["three_tiles"]), cs["three_tiles"][2])
    assert len(p) == 3 and all(t["fast"] and 0 < t["dyn"] < t["out"] for t in p)


@pytest.fixture(scope="module")
def records(tmp_path_factory):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("gpu test without a GPU")
    if not os.path.exists(H.trace_lib()):
        pytest.fail("no %s: build() makes it (make trace)" % H.trace_lib())
    path = str(tmp_path_factory.mktemp("headers_dyn_trace") / "records.jsonl")
    env = dict(os.environ)
    for k in ("QHUFF_KERNELS", "QHUFF_GRID_PCT", "QHUFF_GRID_WG_PER_CU"):
        env.pop(k, None)
    env["QHUFF_LIB"] = H.trace_lib()
    try:
        r = subprocess.run(
            [sys.executable, os.path.join(HERE, "headers_dyn_trace_child.py"),
             path], env=env, timeout=TIMEOUT, capture_output=True, text=True)
    except subprocess.TimeoutExpired:
        pytest.fail("the child ran out of time (%d s)" % TIMEOUT)
    recs = [json.loads(l) for l in open(path)] if os.path.exists(path) else []
    if r.returncode != 0:
        pytest.fail("child: exit status %d after %d cases\n%s"
                    % (r.returncode, len(recs), r.stderr[-2000:]))
    return {x["id"]: x for x in recs}


@pytest.mark.gpu
def test_records_match_the_model(records):
    cs = H.cases()
    assert set(records) == set(cs)
    for cid, case in cs.items():
        assert records[cid]["ok"], cid
        assert records[cid]["tiles"] == H.expect(H.model(case)), cid
