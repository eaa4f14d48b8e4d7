"""qhuff_encode_headers / qhuff_encode_headers_host at the edges of the
header encoder's own index arithmetic (ls-qpack_amd/csrc/qhuff_lookup.hip):
the wave's 64-ary search of sec_hdr, the lane's search of the 63 boundaries
the wave holds and its walk past them, the prefix items of the sections that
start in a tile (the last tile's clause for those that start at n), and the
grid-stride loops of the two small kernels.

Expectations: tests/headers_model.py, never the library; every GPU case runs
the device-pointer and the host form (check_both of test_encode_headers.py:
out, sec_out, kind, static_id, device_error() == 0).

None of that arithmetic runs on the CPU, and a batch that has drifted off its
edge would still pass.  So `section_layout` restates, from the kernel's
comments and the call's contract (bisect and plain loops), what each 64-header
tile has to find -- sa, sb, every lane's count c among the held boundaries,
whether and how far it walks, the search's passes -- and the unmarked tests
pin, batch by batch, that the batch holds the property it is named for."""
import bisect
import ctypes as C
import functools
import random

import numpy as np
import pytest

import _paths  # noqa: F401
import headers_model as M
import limits as L
import qhuff
from test_buffer_contract import FILLS, Arena, Ptr
from test_encode_headers import (Repeated, check, check_both, contract_call,
                                 dev, dev_i32, fetch, headers, pool, shape,
                                 split)

TILE = L.TS
HELD = TILE - 1               # boundaries a lane searches before it walks
GRID = 1024 * 256             # threads of the two small kernels' capped grid


# ---- the layout model --------------------------------------------------------------

def search_passes(m, ans):
    """-> (passes, answer) of a 64-ary search of a non-decreasing list of m
    section starts for "how many are < x", when `ans` of them are (x > 0).
    The answer lies in [lo, hi] = [0, m]; a pass probes 64 indices evenly
    spaced from lo, ceil((hi - lo) / 64) apart (those below hi), and keeps
    what lies behind the last probe that is < x, up to the next probe.  It
    ends when the range is empty or no probe is < x.  (Index i is < x exactly
    when i < ans: the list's values do not matter.)"""
    lo, hi, passes = 0, m, 0
    while hi > lo:
        passes += 1
        step = -(-(hi - lo) // 64)
        if ans == lo:                   # no probe is < x
            break
        q = (ans - 1 - lo) // step      # the last probe below the answer
        lo, hi = lo + q * step + 1, min(lo + (q + 1) * step, hi)
    assert lo == ans
    return passes, lo


def deepest(m):
    """the most passes any answer in [0, m] takes: a pass leaves at most
    ceil(m / 64) - 1 candidates between two probes"""
    return 0 if m == 0 else 1 + deepest(-(-m // 64) - 1)


def first_pass_edge(m, sa):
    """sa is the first or the last answer of one of the first pass's
    sub-ranges (or 0).  On the first the next pass finds no probe < x and
    ends the search; on the last all of its probes are."""
    step = -(-m // 64)
    return sa % step in (0, 1 % step)


def section_layout(sec_hdr, n):
    """per 64-header tile of a call with section starts sec_hdr[0 .. m - 1]
    (sec_hdr[m] = n):
      s0, cnt  its first header, its headers; last: it holds header n - 1
      sa       sections that start before s0
      sb       sections that start at or before its last header; m on the
               last tile (which also takes those that start at n)
      rounds   64-section rounds of its prefix items, one section a lane
      passes   of the 64-ary search for sa (none for s0 = 0)
      c[lane]  min(63, starts among sec_hdr[sa ...] at or before the lane's
               header): what the lane finds among the 63 held boundaries
      walk[lane]  None if c < 63, else the steps it walks on in memory
      own[lane]   sections that start at or before its header (sa + c + walk;
               its items go to 2j + 2 * own)"""
    starts = [int(x) for x in sec_hdr]
    m = len(starts) - 1
    assert starts[m] == n and (m == 0 or starts[0] == 0)
    starts = starts[:m]
    tiles = []
    for s0 in range(0, n, TILE):
        cnt = min(TILE, n - s0)
        last = s0 + cnt == n
        sa = bisect.bisect_left(starts, s0)
        sb = m if last else bisect.bisect_right(starts, s0 + cnt - 1)
        c, walk, own = [], [], []
        for j in range(s0, s0 + cnt):
            o = bisect.bisect_right(starts, j)
            own.append(o)
            c.append(min(HELD, o - sa))
            walk.append(o - sa - HELD if o - sa >= HELD else None)
        tiles.append({"s0": s0, "cnt": cnt, "last": last, "sa": sa, "sb": sb,
                      "rounds": -(-(sb - sa) // TILE),
                      "passes": search_passes(m, sa)[0] if s0 else 0,
                      "c": c, "walk": walk, "own": own})
    return tiles


def test_search_passes_model():
    """the pass counts the issue's section counts sit beside: 64 sections
    take one pass and 65 two; 4,096 and 4,097 both take two (a first pass of
    step 65 leaves 64 candidates, one more pass; the third comes at 4,161);
    262,143 to 262,215 take three.  deepest() is the maximum over every
    answer, by brute force up to 4,300."""
    assert [deepest(m) for m in (1, 63, 64, 65, 4095, 4096, 4097, 4160, 4161,
                                 262143, 262144, 262145, 262215)] \
        == [1, 1, 1, 2, 2, 2, 2, 2, 3, 3, 3, 3, 3]
    for m in list(range(1, 200)) + [4095, 4096, 4097, 4160, 4161, 4300]:
        got = [search_passes(m, a)[0] for a in range(m + 1)]
        assert max(got) == deepest(m) and got[0] == 1, m


def test_section_layout_against_a_linear_scan():
    """section_layout on random section lists: a lane's section by a plain
    loop over all starts, the sections a tile must prefix by membership"""
    rng = random.Random(11)
    for _ in range(60):
        n = rng.randrange(1, 300)
        m = rng.choice((1, 2, 70, 150, 400))
        st = sorted([0] + [rng.choice((rng.randrange(n + 1), n // 2, n))
                           for _ in range(m - 1)])
        lay = section_layout(st + [n], n)
        assert len(lay) == -(-n // TILE)
        seen = []
        for t in lay:
            for lane in range(t["cnt"]):
                j = t["s0"] + lane
                o = sum(1 for s in st if s <= j)
                assert t["own"][lane] == o
                assert t["sa"] + t["c"][lane] + (t["walk"][lane] or 0) == o
                assert (t["walk"][lane] is None) == (t["c"][lane] < HELD)
            mine = [s for s in range(m)
                    if t["s0"] <= st[s] < t["s0"] + t["cnt"]
                    or (t["last"] and st[s] == n)]
            assert mine == list(range(t["sa"], t["sb"]))
            seen += mine
        assert seen == list(range(m))             # every section's prefix, once


# ---- part 2: section counts at the search's and the grids' edges ---------------------

COUNTS = (63, 64, 65, 4095, 4096, 4097, 262143, 262144, 262145, 262145 + 70)
COUNT_N = 200


def count_targets(m):
    """(sa of tile 1, sa of tile 2): a deepest-pass answer strictly inside
    (0, m), then an answer on a sub-range edge of the first pass -- the last
    of a sub-range for even m, the first of one for odd m"""
    step = -(-m // 64)
    edge = 20 * step + (m & 1 if step > 1 else 0)
    deep = next(a for a in range(edge // 2, edge)
                if search_passes(m, a)[0] == deepest(m))
    return deep, edge


@functools.lru_cache(maxsize=None)
def count_starts(m):
    """sec_hdr of m sections over 200 headers (four tiles).  A uniform draw
    over [0, n] cannot give sa = m (that needs every section to start before
    the last tile) or put an sa on a sub-range edge, so the count of starts
    in each tile is set by construction -- count_targets(m) before tiles 1
    and 2, all m before tile 3 -- and only their places within the tile come
    from the seeded generator; the repeats are the empty sections."""
    a1, a2 = count_targets(m)
    rng = np.random.default_rng(m)
    parts = [np.sort(rng.integers(64 * t, 64 * (t + 1), k))
             for t, k in enumerate((a1, a2 - a1, m - a2))]
    st = np.concatenate(parts + [[COUNT_N]]).astype(np.uint32)
    st[0] = 0
    return st


@functools.lru_cache(maxsize=4)
def count_batch(m):
    st = count_starts(m)
    rng = random.Random(300 + m)
    hs = [rng.choice(pool()) + (i & 1,) for i in range(COUNT_N)]
    h = M.Headers(split(hs, st[1:-1].tolist()))
    assert np.array_equal(h.sec_hdr, st) and h.m == m and h.n == COUNT_N
    return h


@pytest.mark.parametrize("m", COUNTS)
def test_count_batches_sit_on_their_edges(m):
    """tile 0 answers sa = 0 (no search), tile 1 an sa strictly inside
    (0, m) that takes the most passes a list of m can take, tile 2 an sa on a
    sub-range edge of the first pass, tile 3 (the last, 8 headers) sa = m;
    every tile but the last has more than 63 starts once m allows, so its
    lanes walk"""
    st = count_starts(m)
    assert len(st) == m + 1 and (np.diff(st.astype(np.int64)) >= 0).all()
    lay = section_layout(st, COUNT_N)
    a1, a2 = count_targets(m)
    assert [t["sa"] for t in lay] == [0, a1, a2, m]
    assert 0 < a1 < a2 < m
    assert [t["passes"] for t in lay][:2] == [0, deepest(m)]
    assert first_pass_edge(m, a2)
    if m > 64:
        # odd m: the first of a sub-range, the second pass ends the search
        # with no probe < x; even m: the last of one, every later pass has
        # all its probes < x
        assert lay[2]["passes"] == (2 if m & 1 else deepest(m))
    assert lay[3]["last"] and lay[3]["cnt"] == 8
    assert lay[3]["sa"] == lay[3]["sb"] == m and lay[3]["rounds"] == 0
    assert [t["sb"] for t in lay[:3]] == [a1, a2, m]
    if m > 4 * TILE:
        assert all(t["rounds"] > 1 for t in lay[:3])
        assert all(max(w for w in t["walk"] if w is not None) > 1
                   for t in lay[:3])
    if m >= 262143:
        assert deepest(m) == 3
    # the two small kernels' loop over s <= m: a second round from m = GRID on
    assert (m + 1 > GRID) == (m >= 262144)


class NoHeaders:
    """m sections without a header: m prefixes (numpy, not the model's
    per-section loop)"""

    def __init__(self, m):
        self.n, self.m = 0, m
        self.data = np.zeros(0, np.uint8)
        self.off = np.zeros(1, np.uint32)
        self.sec_hdr = np.zeros(m + 1, np.uint32)
        self.hflags = None
        self.want = b"\0\0" * m
        self.want_sec_out = (2 * np.arange(m + 1)).astype(np.uint32)
        self.want_kind = self.want_id = np.zeros(0, np.uint8)


def test_no_headers_is_the_model_s():
    h, g = NoHeaders(5), M.Headers([[]] * 5)
    assert h.want == g.want and np.array_equal(h.want_sec_out, g.want_sec_out)
    assert np.array_equal(h.sec_hdr, g.sec_hdr) and np.array_equal(h.off, g.off)


# ---- part 3: the lane's own search ---------------------------------------------------

LANE_N = 2 * TILE + 9
LANE_KS = (62, 63, 64, 65)
LANES = (40, 0, 63)


def lane_batch(lane, k):
    """three tiles; in the middle one exactly k sections start at or before
    `lane` -- k - 1 empty ones and the one that holds it, all on its header
    -- and none after it: the next ordinary sections start in the last tile
    (so lanes lane .. 63 all see the same k)"""
    p = TILE + lane
    return M.Headers(split(headers(LANE_N, 400 + 64 * k + lane),
                           [20, 50] + [p] * k + [130, 133]))


EDGE_SHAPES = {"lane%d_k%d" % (ln, k): functools.partial(lane_batch, ln, k)
               for ln in LANES for k in LANE_KS}
# 100 sections (99 empty ones and the one that holds it) exactly on tile 1's
# first header; tile 1 is the last, partial tile
EDGE_SHAPES["edge64"] = lambda: M.Headers(
    split(headers(100, 431), [30] + [64] * 100 + [70]))
# a run of empty sections on either side of a tile edge
EDGE_SHAPES["straddle"] = lambda: M.Headers(
    split(headers(LANE_N, 432), [63] * 40 + [64] * 40))

# ---- part 4: trailing empty sections --------------------------------------------------

TRAIL_N = (64, 128, 137)
TRAIL_T = (1, 63, 64, 65, 200)


def trail_batch(n, t):
    """t sections that start at n, behind three ordinary ones"""
    return M.Headers(split(headers(n, 500 + n + t), [10, n - 20] + [n] * t))


for _n in TRAIL_N:
    for _t in TRAIL_T:
        EDGE_SHAPES["trail_n%d_t%d" % (_n, _t)] = \
            functools.partial(trail_batch, _n, _t)
_ONE = [(b":method", b"GET", 1)]
EDGE_SHAPES["only_last"] = lambda: M.Headers([[]] * 299 + [_ONE])
EDGE_SHAPES["only_first"] = lambda: M.Headers([_ONE] + [[]] * 299)


@functools.lru_cache(maxsize=None)
def edge_shape(name):
    return EDGE_SHAPES[name]()


def lay_of(h):
    return section_layout(h.sec_hdr, h.n)


@pytest.mark.parametrize("lane", LANES)
@pytest.mark.parametrize("k", LANE_KS)
def test_lane_batches_hold_k_starts(lane, k):
    """middle tile: lanes before `lane` find c = 0, lanes lane .. 63 find
    c = k for k <= 62 and do not walk, c = 63 otherwise and walk 0, 1 and 2
    steps for k = 63, 64, 65"""
    h = edge_shape("lane%d_k%d" % (lane, k))
    assert h.n == LANE_N and h.m == k + 5
    lay = lay_of(h)
    assert [t["cnt"] for t in lay] == [64, 64, 9]
    t = lay[1]
    assert t["sa"] == 3 and t["sb"] == 3 + k
    assert t["rounds"] == (2 if k == 65 else 1)     # k = 64: one full round
    assert t["c"][:lane] == [0] * lane
    assert t["c"][lane:] == [min(k, 63)] * (64 - lane)
    want = None if k <= 62 else k - 63
    assert t["walk"][lane:] == [want] * (64 - lane)
    assert t["walk"][:lane] == [None] * lane
    # tile 0 ends inside the section that starts at 50; the last tile's two
    # ordinary starts are found without a walk
    assert lay[0]["sb"] == 3 == lay[1]["sa"] and lay[2]["sa"] == 3 + k
    assert set(lay[2]["walk"]) == {None} and max(lay[2]["c"]) == 2


def test_runs_on_a_tile_edge():
    """edge64: all 100 sections that start on header 64 are tile 1's (the strict
    < of sections_before): tile 0's sb is tile 1's sa, tile 1 is the last,
    partial one and every one of its lanes walks.  straddle: 40 empty
    sections on header 63 are tile 0's, 40 on header 64 tile 1's.  lane 0's
    batches are the same edge with k starts."""
    h = edge_shape("edge64")
    lay = lay_of(h)
    assert [t["cnt"] for t in lay] == [64, 36] and h.m == 103
    assert lay[0]["sa"] == 0 and lay[0]["sb"] == 2 == lay[1]["sa"]
    assert lay[1]["sb"] == h.m and lay[1]["rounds"] == 2
    assert lay[1]["walk"][:6] == [100 - 63] * 6      # then header 70's start
    assert lay[1]["walk"][6:] == [101 - 63] * 30
    assert int(h.sec_hdr[2]) == 64 == int(h.sec_hdr[101])
    h = edge_shape("straddle")
    lay = lay_of(h)
    assert lay[0]["sb"] == 41 == lay[1]["sa"] and lay[1]["sb"] == 81
    assert lay[0]["c"][62:] == [1, 41] and lay[1]["c"] == [40] * 64
    assert lay[2]["sa"] == lay[2]["sb"] == 81 == h.m
    for k in LANE_KS:
        lay = lay_of(edge_shape("lane0_k%d" % k))
        assert lay[0]["sb"] == lay[1]["sa"] == 3
        assert int(edge_shape("lane0_k%d" % k).sec_hdr[3]) == 64


@pytest.mark.parametrize("n", TRAIL_N)
@pytest.mark.parametrize("t", TRAIL_T)
def test_trail_batches_end_in_t_empty_sections(n, t):
    """the last tile's sb is m though none of the t sections starts at one
    of its headers; it is a full tile for n = 64 and 128; from t = 63 on its
    prefix loop takes a second round by t = 65 at the latest (t = 200: four),
    and t = 63 or 64 make one round of exactly 64 sections"""
    h = edge_shape("trail_n%d_t%d" % (n, t))
    assert h.m == 3 + t and (h.sec_hdr[3:] == n).all() and h.sec_hdr[2] < n
    assert h.want[-2 * t:] == b"\0\0" * t
    lay = lay_of(h)
    last = lay[-1]
    assert last["last"] and last["sb"] == h.m
    assert last["cnt"] == (64 if n % 64 == 0 else n % 64)
    by_header = bisect.bisect_right(h.sec_hdr[:h.m].tolist(), n - 1)
    assert by_header == 3 == h.m - t                # what lane cnt - 1 finds
    assert last["rounds"] == -(-(h.m - last["sa"]) // 64)
    # the tile's sections: the ordinary ones that start in it and the t
    assert h.m - last["sa"] == t + {64: 3, 128: 1, 137: 0}[n]
    assert last["rounds"] == {1: 1, 63: 2 if n == 64 else 1,
                              64: 1 if n == 137 else 2, 65: 2, 200: 4}[t]
    assert set(last["walk"]) == {None}              # no lane counts them


def test_single_header_batches():
    """only_last: 300 starts on header 0, the lane walks from 63 to 300;
    only_first: 299 sections start at n = 1"""
    h = edge_shape("only_last")
    (t,) = lay_of(h)
    assert (h.n, h.m) == (1, 300) and t["c"] == [63] and t["walk"] == [237]
    assert h.want[:598] == b"\0\0" * 299 and len(h.want) > 600
    h = edge_shape("only_first")
    (t,) = lay_of(h)
    assert t["c"] == [1] and t["walk"] == [None] and t["sb"] == 300
    assert t["rounds"] == 5 and h.want[-598:] == b"\0\0" * 299


@functools.lru_cache(maxsize=None)
def small_grid_base():
    """three full tiles: 65 starts on lane 40 of tile 1, 70 on lane 5 of
    tile 2; repeated, two tiles of every three have more than 64 starts"""
    return M.Headers(split(headers(3 * TILE, 433),
                           [20, 50] + [TILE + 40] * 65 + [2 * TILE + 5] * 70
                           + [2 * TILE + 30]))


def heavy_tiles(h):
    return [i for i, t in enumerate(lay_of(h)) if t["sb"] - t["sa"] > TILE]


def test_small_grid_base_layout():
    h = small_grid_base()
    lay = lay_of(h)
    assert [t["cnt"] for t in lay] == [64, 64, 64]
    assert heavy_tiles(h) == [1, 2]
    assert lay[1]["walk"][40:] == [2] * 24 and lay[2]["walk"][5] == 7
    r = Repeated(h, 4)
    assert heavy_tiles(r) == [1, 2, 4, 5, 7, 8, 10, 11]
    g = M.Headers(h.sections * 4)
    assert r.want == g.want and np.array_equal(r.sec_hdr, g.sec_hdr)


# ---- part 5: offsets with bit 31 set ---------------------------------------------------

HIGH = 0x80000000


@functools.lru_cache(maxsize=None)
def high_shape(name):
    if name == "boundaries":
        return shape("boundaries")
    from test_static_lookup import unstaged_batch
    pairs = unstaged_batch()
    return M.Headers(split(pairs, range(50, len(pairs), 50)), flags=False)


def test_high_offsets_stay_in_32_bits():
    for name in ("boundaries", "unstaged"):
        h = high_shape(name)
        for r in (0, 15):
            off = h.off.astype(np.uint64) + np.uint64(HIGH + r)
            assert off[0] >> 31 == 1 and off[-1] < 1 << 32
    h = high_shape("unstaged")
    for r in (0, 15):       # the data's address residue is r (see high_call)
        info = L.classify_hash(h.off.astype(np.int64) + r, 0, True)
        assert [t["staged"] for t in info] == [True, False] * 3


# ---- GPU -----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def codec():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("gpu test without a GPU")
    c = qhuff.Codec(0)
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("m", COUNTS)
def test_section_counts(codec, m):
    """sections_before's passes (lo += (c - 1) * step + 1, hi = min(top,
    hi), the c == 0 exit) with the answers 0, m, a deepest one and one on a
    first-pass edge; the `k += 64` prefix loop over up to 87,000 sections a
    tile; from m = 262,144 the second round of qhuff_secout_kernel's
    `s <= m` loop"""
    check_both(codec, count_batch(m))


@pytest.mark.gpu
@pytest.mark.parametrize("m", (262143, 262144, 262145))
def test_no_header_section_counts(codec, m):
    """n = 0: qhuff_empty_sections_kernel's `s <= m` loop on its capped
    grid, one round for m + 1 = 262,144 and a second one past it"""
    check_both(codec, NoHeaders(m))


def guarded(codec, h, host, k):
    """one contract_call of test_encode_headers.py: every array at its exact
    size in a dirty guarded arena, the expected bytes and nothing else"""
    ar, img = contract_call(codec, h, host, k, (0, 1, 15)[k % 3],
                            FILLS[k % 3])
    assert np.array_equal(ar.get(img, "sec_out", np.uint32), h.want_sec_out)
    assert ar.get(img, "out").tobytes() == h.want
    assert np.array_equal(ar.get(img, "kind"), h.want_kind)
    assert np.array_equal(ar.get(img, "static_id"), h.want_id)
    ar.check(img, {"out": len(h.want), "sec_out": 4 * (h.m + 1),
                   "kind": h.n, "static_id": h.n})


@pytest.mark.gpu
@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
def test_stride_loops_write_exactly_their_arrays(codec, host):
    """m = 262,144 with 200 headers and with none: sec_out of exactly m + 1
    words and out of exactly sec_out[m] bytes between guards -- the second
    round of both small kernels' loops ends at s = m"""
    guarded(codec, count_batch(262144), host, 0 + 3 * host)
    guarded(codec, NoHeaders(262144), host, 1 + 3 * host)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(EDGE_SHAPES))
def test_edge_shapes(codec, name):
    """lane*_k*: the last index of the ds_bpermute search (c = 62), `if (c ==
    63)` and a `while (s1 < a.m && sh[s1] <= j)` that ends at once, after
    one and after two steps.  edge64 / straddle / lane0: the strict `<` of
    sections_before and sb from lane cnt - 1.  trail_*: `last ? a.m : ...`
    with s0 + cnt == a.n on a full tile, write_prefix's `sh < a.n ? sh :
    a.n` and the prefix loop's further rounds.  only_*: one header under 300
    sections."""
    check_both(codec, edge_shape(name), pads=(0, 15))


@pytest.mark.gpu
@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
def test_trailing_sections_buffer_contract(codec, host):
    """n = 128 (a full last tile) with 1, 63, 64, 65 and 200 sections that
    start at n: exact sizes in a dirty guarded arena, the three fills and
    data residues 0, 1 and 15"""
    for t in TRAIL_T:
        h = edge_shape("trail_n128_t%d" % t)
        for k in range(3):
            guarded(codec, h, host, k + 3 * host)


@pytest.mark.gpu
def test_small_grid_heavy_tiles_second_and_third():
    """a context whose hash grid is 1 %: every wave runs three tiles or
    more, and tiles with more than 64 starts (the walk, two prefix rounds)
    are among those a wave reaches second and third, behind the prefetch
    chain's o_cur = o_nxt hand-over"""
    from test_hash_limits import _open
    c = _open({"QHUFF_GRID_PCT": "1"})
    try:
        W = c.grid_waves(qhuff.KIND_HASH)
        base = small_grid_base()
        k = W + 1
        h = Repeated(base, k)
        assert 3 <= W < 1000 and h.n // TILE == 3 * k > 3 * W
        heavy = heavy_tiles(h)
        assert any(W <= t < 2 * W for t in heavy)
        assert any(2 * W <= t < 3 * W for t in heavy)
        for _ in range(2):
            check_both(c, h)
    finally:
        c.close()


def high_call(codec, h, r, host):
    """the call with `off` + 0x80000000 + r and `in` that far before the
    data (the device data at address residue r) -> (out, sec_out, kind,
    static_id) as check() takes them"""
    import torch
    off = (h.off.astype(np.uint64) + np.uint64(HIGH + r)).astype(np.uint32)
    bound = qhuff.encode_headers_bound(len(h.data), h.n, h.m)
    if host:
        data = np.concatenate([h.data, np.zeros(16, np.uint8)])
        p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        out = np.zeros(bound, np.uint8)
        so = np.zeros(h.m + 1, np.uint32)
        kind, sid = np.zeros(h.n, np.uint8), np.zeros(h.n, np.uint8)
        rc = qhuff.lib().qhuff_encode_headers_host(
            codec._ctx, data.ctypes.data - HIGH - r, p(off), h.n,
            p(h.hflags) if h.hflags is not None else None, p(h.sec_hdr), h.m,
            p(out), p(so), p(kind), p(sid))
        assert rc == qhuff.OK
        return out[:so[-1]].tobytes(), so, kind, sid
    d = dev(h.data, r)
    out = torch.empty(bound, dtype=torch.uint8, device="cuda")
    so = torch.empty(h.m + 1, dtype=torch.int32, device="cuda")
    kind, sid = (torch.empty(h.n, dtype=torch.uint8, device="cuda")
                 for _ in range(2))
    fl = dev(h.hflags)[:h.n] if h.hflags is not None else None
    codec.encode_headers_into(Ptr(d.data_ptr() - HIGH), dev_i32(off), h.n, fl,
                              dev_i32(h.sec_hdr), h.m, out, so, kind, sid)
    torch.cuda.synchronize()
    assert codec.device_error() == 0
    return fetch((out, so, kind, sid))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["boundaries", "unstaged"])
def test_offsets_with_top_bit_set(codec, name):
    """uint32 offsets with bit 31 set, through o_cur.a / .m into str_off
    and write_prefix's `at`, into tile_span and HashGlb of the lookup launch
    and into the encode launch (staged and, for the unstaged batch's long
    values, its out-of-line tile); the host form rebases by -off[0] itself.
    The same offsets through qhuff_static_lookup and its host form."""
    import torch
    from test_static_lookup import model_arrays, same
    h = high_shape(name)
    pairs = [(nm, v) for s in h.sections for nm, v, _ in s]
    want = model_arrays(pairs)
    for r in (0, 15):
        for host in (False, True):
            check(h, high_call(codec, h, r, host))
        off = (h.off.astype(np.uint64) + np.uint64(HIGH + r)).astype(np.uint32)
        d = dev(h.data, r)
        got = [torch.full((h.n,), 0x5A, dtype=dt, device="cuda")
               for dt in (torch.int32, torch.int32, torch.uint8, torch.uint8)]
        codec.static_lookup_into(Ptr(d.data_ptr() - HIGH), dev_i32(off), h.n,
                                 *got)
        torch.cuda.synchronize()
        assert codec.device_error() == 0
        assert same([g.cpu().numpy() for g in got], want), r
        data = np.concatenate([h.data, np.zeros(16, np.uint8)])
        res = [np.zeros(h.n, np.uint32), np.zeros(h.n, np.uint32),
               np.zeros(h.n, np.uint8), np.zeros(h.n, np.uint8)]
        assert qhuff.lib().qhuff_static_lookup_host(
            codec._ctx, data.ctypes.data - HIGH - r,
            off.ctypes.data_as(C.c_void_p), h.n,
            *[a.ctypes.data_as(C.c_void_p) for a in res]) == qhuff.OK
        assert same(res, want), r


@pytest.mark.gpu
@pytest.mark.parametrize("given", ["name_hash", "nameval_hash"])
def test_lookup_with_one_hash_null(codec, given):
    """qhuff_static_lookup with one of the two hash outputs null (`if
    (a.h1)` / `if (a.h2)` apart): the one given is the model's, and the
    array that stands where the other would be, poisoned, is untouched"""
    import torch
    from test_static_lookup import mixed_pairs, model_arrays
    pairs = mixed_pairs(130, 7)
    data, off = M.pack_pairs(pairs)
    want = model_arrays(pairs)
    n = len(pairs)
    ar = Arena([("in", len(data), 3), ("off", 4 * len(off), 4),
                ("name_hash", 4 * n, 8), ("nameval_hash", 4 * n, 12),
                ("kind", n, 1), ("static_id", n, 7)], seed=8100)
    ar.put("in", data)
    ar.put("off", off)
    ar.commit(True)
    h = {given: ar.addr(given)}
    rc = qhuff.lib().qhuff_static_lookup(
        codec._ctx, ar.addr("in"), ar.addr("off"), n, h.get("name_hash"),
        h.get("nameval_hash"), ar.addr("kind"), ar.addr("static_id"),
        codec._stream(None))
    assert rc == qhuff.OK
    torch.cuda.synchronize()
    assert codec.device_error() == 0
    img = ar.after()
    assert np.array_equal(ar.get(img, given, np.uint32),
                          want[0 if given == "name_hash" else 1])
    assert np.array_equal(ar.get(img, "kind"), want[2])
    assert np.array_equal(ar.get(img, "static_id"), want[3])
    ar.check(img, {given: 4 * n, "kind": n, "static_id": n})


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(EDGE_SHAPES))
def test_edge_shapes_round_trip(codec, name):
    """qhuff_encode_headers_host and back through qhuff_decode_headers_host:
    the header lists come back equal, and every section's header count is
    diff(sec_hdr), 0 for each empty one"""
    h = edge_shape(name)
    out, so, kind, sid = codec.encode_headers_host(h.data, h.off, h.sec_hdr,
                                                   h.hflags)
    assert out.tobytes() == h.want
    ret, hdr_off, rc, dkind, dsid, hf, dec, doff, status = \
        codec.decode_headers_host(out, so)
    assert ret == qhuff.OK and not rc.any() and not status.any()
    assert np.array_equal(hdr_off, h.sec_hdr)
    counts = np.diff(hdr_off.astype(np.int64))
    assert np.array_equal(counts, [len(s) for s in h.sections])
    assert (counts == 0).sum() == sum(1 for s in h.sections if not s) > 0
    assert dec.tobytes() == h.data.tobytes() and np.array_equal(doff, h.off)
    assert np.array_equal(dkind, kind) and np.array_equal(dsid, sid)
    # the N bit comes back wherever a line carries one
    lit = h.want_kind != M.INDEXED
    assert np.array_equal(hf[lit] & M.NEVER, h.hflags[lit] & M.NEVER)
