"""The replicated super-tile flags (kLbReplicas, qhuff_device.h): every
publish writes all replicas, a wave polls one.  Each GPU case runs once per
pinned replica (QHUFF_LB_REPLICA=r: every wave polls replica r) and once with
the replica chosen by workgroup, so a replica that a publish, the workspace
layout or the wrap's memset misses is one every look-back of some run reads:
it shows as a wrong offset or as a spin error.  Every launch is compared
whole with the oracle through test_lookback's Launch (out_off[0..n], the
statuses, every output byte, sentinels behind them, no device error).
DESIGN section 4, "Replicated super flags"."""
import os
import re

import numpy as np
import pytest

import _paths  # noqa: F401
import lookback as B
import qhuff
from test_lookback import _run_plan, open_codec, run_checked

E, D = qhuff.KIND_ENCODE, qhuff.KIND_DECODE


def replicas():
    """kLbReplicas: the default of QH_LB_REPLICAS in qhuff_device.h"""
    path = os.path.join(qhuff.PKG_ROOT, "csrc", "qhuff_device.h")
    with open(path) as f:
        m = re.search(r"^#define QH_LB_REPLICAS (\d+)$", f.read(), re.M)
    return int(m.group(1))


R = replicas()
PINS = ["auto"] + list(range(R))


def pin_env(pin, **more):
    env = dict(more)
    if pin != "auto":
        env["QHUFF_LB_REPLICA"] = str(pin)
    return env


def sflag_stride(cap_super):
    """u64 words between two replicas (sflag_stride, qhuff_device.h)"""
    return (cap_super + 31) & ~31


# ---- CPU ---------------------------------------------------------------------------

def test_replica_count_and_knob():
    assert R in (4, 8, 16)
    with open(qhuff.LIB_PATH, "rb") as f:
        assert b"QHUFF_LB_REPLICA\0" in f.read()


def test_replica_stride_is_whole_lines():
    for caps in (1, 31, 32, 33, 64, 65, 129, 130, 256, 16384):
        st = sflag_stride(caps)
        assert st >= caps and st % 32 == 0 and st - caps < 32
    # the cases below: three super tiles; 130 (two polled windows and a
    # third); growth 2 -> 65 -> 129 super tiles on the 4096-tile floor
    assert B.supers(129) == 3 and B.in_super(129, 2) == 1
    assert B.supers(8257) == 130 and 64 * 8256 + 64 >= 64 * (64 * 129) + 64
    tw, sw = B.windows(8257 - 1)
    assert None not in sw[0] and None not in sw[1] and sw[2][0] == 0
    assert [c for _, c, _ in B.cap_after([65, 4097, 65, 8193])] == \
        [64, 65, 65, 129]


def slow_pred(T, last, tile):
    """tiny(T, last) with the 64 strings of `tile` about 4 KB each: the
    tiles behind it spin on its aggregate and on its super tile's flag"""
    base = B.tiny(T, last)
    a, b = base.tile(tile)
    assert b - a == B.TS
    rng = np.random.default_rng([T, last, tile, 4096])
    lens = np.diff(base.off.astype(np.int64))
    lens[a:b] = rng.integers(4000, 4097, B.TS)
    data, off = B._pack(lens, rng)
    return B.Batch(data, off, "tiny(%d,%d)+4k@%d" % (T, last, tile))


SLOW_T, SLOW_LAST, SLOW_AT = 200, 40, 5


def test_slow_predecessor_shape():
    b = slow_pred(SLOW_T, SLOW_LAST, SLOW_AT)
    assert b.T == SLOW_T and SLOW_AT < B.SUPER and b.T - SLOW_AT - 1 >= 130
    a, e = b.tile(SLOW_AT)
    assert (np.diff(b.off.astype(np.int64))[a:e] >= 4000).all()
    assert B.tile_paths(b, SLOW_AT) == ("slow", "slow")
    assert B.tile_paths(b, SLOW_AT + 1) == ("fast", "fast")


# ---- GPU ---------------------------------------------------------------------------

@pytest.fixture(scope="module", params=PINS)
def pinned(request):
    c = open_codec(pin_env(request.param))
    yield c
    c.close()


@pytest.mark.gpu
def test_three_super_tiles_partial_last(pinned):
    """2 * 4096 + 1 strings: super tiles 0 and 1 whole, super tile 2 of one
    tile of one string, which publishes and reads on its own"""
    run_checked(pinned, B.tiny(129, 1))


@pytest.mark.gpu
def test_more_than_two_windows(pinned):
    """8257 tiles, 130 super tiles: both windows polled with the tile window
    and a third one come from the wave's replica"""
    run_checked(pinned, B.tiny(8257, 64))


@pytest.mark.gpu
@pytest.mark.parametrize("kernels", ["full", "lean"])
@pytest.mark.parametrize("pin", PINS)
def test_slow_predecessor(pin, kernels):
    """a tile of 64 strings of 4 KB in super tile 0 and 194 tiles of tiny
    strings behind it: they spin, and re-poll their replica, until it and
    then super tile 0 are published"""
    c = open_codec(pin_env(pin, QHUFF_KERNELS=kernels))
    try:
        run_checked(c, slow_pred(SLOW_T, SLOW_LAST, SLOW_AT))
    finally:
        c.close()


def _sizes_plan(sizes):
    """alternating encode / decode launches of the twins of `sizes` tiles
    (equal sizes alternate k = 1 and 3: other bytes in every prefix)"""
    seen, plan = {}, []
    for i, T in enumerate(sizes):
        k = (1, 3)[seen.get(T, 0) % 2]
        seen[T] = seen.get(T, 0) + 1
        plan.append(((E, D)[i % 2], B.twin(T, 64, k)))
    return plan


def _one_stream(env, plan):
    import torch
    c = open_codec(env)
    try:
        _run_plan(c, plan, False, [torch.cuda.Stream()])
    finally:
        c.close()


STALE = (4097, 65, 4097, 4097, 65, 4097, 65, 4097)


@pytest.mark.gpu
@pytest.mark.parametrize("pin", PINS)
def test_stale_epochs(pin):
    """large, small, large on one context and one stream with no host
    synchronisation between: the small launch leaves the large one's flags
    of super tiles 2..64 in every replica, one epoch old, for the next"""
    _one_stream(pin_env(pin), _sizes_plan(STALE[:3]))


@pytest.mark.gpu
@pytest.mark.parametrize("pin", PINS)
def test_stale_epochs_across_the_wrap(pin):
    """the same on a context opened four launches before the 22-bit epoch
    wrap (QHUFF_EPOCH0, as test_lookback.test_epoch_wrap): both parities,
    then the launch that memsets the workspace -- every replica -- and
    restarts at epoch 1, then three more"""
    wraps = [w for _, w in B.epochs(B.EPOCH_LAST - 4, len(STALE))]
    assert wraps.index(True) == 4 and sum(wraps) == 1
    _one_stream(pin_env(pin, QHUFF_EPOCH0=str(B.EPOCH_LAST - 4)),
                _sizes_plan(STALE))


@pytest.mark.gpu
@pytest.mark.parametrize("pin", PINS)
def test_workspace_growth(pin):
    """65, 4097, 65, 8193, 4097 tiles on one context: cap_super 64 -> 65 ->
    129, so the replicas' stride (64 -> 96 -> 160 words) and the place of
    every replica but the first change with the workspace"""
    sizes = (65, 4097, 65, 8193, 4097)
    assert [sflag_stride(c) for _, c, _ in B.cap_after(sizes)] == \
        [64, 96, 96, 160, 160]
    _one_stream(pin_env(pin), _sizes_plan(sizes))
