"""bench.py's plain / --full split and --dump-outputs: the sampling helper on
the CPU, and one small plain run on the GPU whose dumped outputs are the
oracle's encode of the seeded batch and that batch itself."""
import json
import os
import sys

import numpy as np
import pytest

from _paths import ROOT

sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_full_is_off_by_default():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert not a.full and a.dump_outputs is None and a.steps == 7
    assert bench.parse(["--full"]).full
    assert bench.parse(["--dump-outputs", "d"]).dump_outputs == "d"


def test_dump_sample_is_fixed_and_bounded():
    assert bench.dump_sample(np, 100, 100) is None
    a = bench.dump_sample(np, 1000, 64)
    b = bench.dump_sample(np, 1000, 64)
    assert a.shape == (64,) and np.array_equal(a, b)
    assert a.min() >= 0 and a.max() < 1000 and np.all(np.diff(a) >= 0)


def test_dump_outputs_types_and_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET", 4000)
    small = np.arange(100, dtype=np.uint8)
    big = np.arange(5000, dtype=np.uint32) * 70000       # beyond float32
    bench.dump_outputs(np, str(tmp_path / "o"), {
        "small": (small, np.float32), "big": (big, np.float64)})
    s = np.load(tmp_path / "o" / "small.npy")
    b = np.load(tmp_path / "o" / "big.npy")
    assert s.dtype == np.float32 and np.array_equal(s, small)
    assert b.dtype == np.float64 and b.shape == (250,)    # 2000 B share / 8
    assert np.array_equal(b, big[bench.dump_sample(np, 5000, 250)])
    assert s.nbytes + b.nbytes <= 4000


@pytest.mark.gpu
def test_plain_run_dumps_last_step(tmp_path, capsys):
    import oracle_lib
    import qhuff
    n = 5000
    bench.main(["--gpus", "1", "--steps", "3", "--warmup", "2", "--n", str(n),
                "--dump-outputs", str(tmp_path)])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 2 and d["full"] is False
    assert d["unit"] == "GB/s" and d["higher_is_better"] and d["dtype"] == "u8"
    assert d["ms_per_step"] > 0 and d["roundtrip_ok"] and not d["device_error"]
    raw = d["config"]["raw_bytes_per_gpu"]
    assert d["value"] == pytest.approx(2 * raw / d["ms_per_step"] / 1e6,
                                       rel=1e-2)
    # the legs beside the headline figure did not run
    for k in ("xxh32_headers", "host_path", "workloads", "two_streams"):
        assert k not in d
    assert d["cpu_baseline"] is None

    data, off = qhuff.synth_batch(n, seed=0x9E3779B97F4A7C15)
    r_out, r_off = oracle_lib.encode_batch(data, off, 0)
    got = {f[:-4]: np.load(os.path.join(tmp_path, f))
           for f in os.listdir(tmp_path)}
    assert sorted(got) == ["dec_out", "dec_out_off", "dec_status", "enc_out",
                           "enc_out_off"]
    assert got["enc_out"].dtype == np.float32
    assert got["enc_out_off"].dtype == np.float64
    assert np.array_equal(got["enc_out"], r_out)
    assert np.array_equal(got["enc_out_off"], r_off)
    assert np.array_equal(got["dec_out"], data)
    assert np.array_equal(got["dec_out_off"], off)
    assert got["dec_status"].shape == (n,) and not got["dec_status"].any()
