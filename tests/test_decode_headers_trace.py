"""The path each tile of qhuff_decode_headers takes, read from the path-trace
build (libqhuff_trace.so) in a child process, against the layout model
(headers_decode_model.layout): staged or not, fast or out of line, fixed or
placed arena slots -- on each side of the kernel's three comparisons (a
66 / 67-byte literal beside static strings, 3008 / 3009 bytes of output most
of them static, a wire span of 3072 / 3073 bytes), a tile without wire bytes
and one past the stage.  tests/test_decode_headers.py checks the bytes; this
file checks that the tiles built for an edge sit on the side they are named
for."""
import json
import os
import subprocess
import sys

import pytest

import _paths  # noqa: F401
import headers_decode_model as D
import headers_trace_child as H

HERE = os.path.dirname(os.path.abspath(__file__))
TIMEOUT = 120


def test_cases_sit_on_their_sides():
    """the model's own verdicts for the cases (CPU)"""
    want = {"wire_free": (True, True, True), "unstaged": (False, False, False),
            "arena66": (True, True, True), "arena67": (True, True, False),
            "out3008": (True, True, False), "out3009": (True, False, False),
            "span3072": (True, True, False), "span3073": (False, False, False)}
    cs = H.cases()
    for cid, (staged, fast, fixed) in want.items():
        secs, a0 = cs[cid]
        p = D.layout(D.Decoded(secs, a0=a0))
        assert len(p) == 1, cid
        assert (p[0]["staged"], p[0]["fast"], p[0]["fixed"]) \
            == (staged, fast, fixed), cid
    secs, a0 = cs["three_tiles"]
    assert len(D.layout(D.Decoded(secs, a0=a0))) == 3


@pytest.fixture(scope="module")
def records(tmp_path_factory):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("gpu test without a GPU")
    if not os.path.exists(H.trace_lib()):
        pytest.fail("no %s: build() makes it (make trace)" % H.trace_lib())
    path = str(tmp_path_factory.mktemp("headers_trace") / "records.jsonl")
    env = dict(os.environ)
    for k in ("QHUFF_KERNELS", "QHUFF_GRID_PCT", "QHUFF_GRID_WG_PER_CU"):
        env.pop(k, None)
    env["QHUFF_LIB"] = H.trace_lib()
    try:
        r = subprocess.run(
            [sys.executable, os.path.join(HERE, "headers_trace_child.py"),
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
    for cid, (secs, a0) in cs.items():
        assert records[cid]["ok"], cid
        assert records[cid]["tiles"] == H.expect(D.Decoded(secs, a0=a0)), cid
