"""The rule that tapers a grouped launch (csrc/host/launch_options.h: frame_taper_table), on the CPU.

The rule as the header states it.  The tile costs are binned like the tile order: bin = (2047 - min(cost, max_cost) * 2047
// max_cost) // 32, 64 bins, bin 0 the heaviest; count[b] tiles and weight[b] = the sum of max(cost - floor, 0) over them.
Bins are visited heaviest first, empty ones skipped; with R(b) = the weight of bin b and of every later bin, bin b takes
the LARGEST g of G, ceil(G / 2), ceil(G / 4), ..., 1 with g * alpha * waves * weight[b] <= n * R(b) * count[b]; weight 0
takes G.  Neighbours of equal g merge into a segment {first rank, g, first item}; a segment's tiles are ceil(n / g) items
each.  More than 8 segments: merge the bins in pairs and start again.  G <= 1, n < 2 or no resident waves: one segment of
G.  The expected tables below were worked out by hand from that sentence; the properties are checked over a grid."""
import ctypes as C

import numpy as np
import pytest

FRAME_TAPER = 7              # RT_TEST_RULE_FRAME_TAPER
WORDS, HEAD, MAX_SEGMENTS = 28, 4, 8
MAX_COST, FLOOR = 2560, 512  # 64 pixels x 8 samples x 5 segments; 64 x 8: what a complete primary table serves
WAVES = 5120


def table(rt, costs, n, G, waves=WAVES, alpha=2, max_cost=MAX_COST, floor=FLOOR):
    L = rt.load_test()
    words = np.concatenate([np.asarray(costs, np.uint32), np.zeros(WORDS, np.uint32)])   # the costs, then room for the table
    inp, out = (C.c_int64 * 8)(n, G, waves, max_cost, floor, len(costs), words.ctypes.data, alpha), (C.c_int64 * 2)()
    rc = L.rt_test_launch_rule(FRAME_TAPER, C.byref(inp), C.byref(out))
    assert rc == 0, (rc, L.rt_last_error(None))
    t = [int(w) for w in words[len(costs):]]
    assert out[0] == t[0] and out[1] == alpha
    return t


def segments(t):
    return [tuple(t[HEAD + 3 * k:HEAD + 3 * k + 3]) for k in range(t[0])]


def padded(head, segs):
    flat = list(head) + [w for s in segs for w in s]
    return flat + [0] * (WORDS - len(flat))


def halvings(G):
    out = [G]
    while out[-1] > 1:
        out.append((out[-1] + 1) // 2)
    return out


def test_tables_worked_out_by_hand(rt):
    # four tiles in four bins -- 2560 -> bin 0, 1536 -> 2047 - 1228 = 819 -> 25, 1024 -> 2047 - 818 = 1229 -> 38,
    # 768 -> 2047 - 614 = 1433 -> 44 --, effective costs 2048, 1024, 512, 256; one resident wave, alpha 1, n = 8, G = 8:
    #   bin 0: R = 3840: 8 x 2048 = 16384 <= 8 x 3840 = 30720 -> 8
    #   bin 25: R = 1792: 8 x 1024 <= 14336 -> 8         bin 38: R = 768: 8 x 512 <= 6144 -> 8      bin 44: R = 256 -> 8
    assert table(rt, [2560, 1536, 1024, 768], 8, 8, waves=1, alpha=1) == padded((1, 4, 8, 8), [(0, 8, 0)])
    # two resident waves: bin 0: 16 x 2048 = 32768 > 30720, 4: 16384 <= 30720 -> 4; bin 25: 16 x 1024 > 14336, 4: 8192 -> 4;
    # bin 38: 16 x 512 = 8192 > 6144, 4: 4096 -> 4; bin 44: 16 x 256 = 4096 > 2048, 4: 2048 <= 2048 -> 4
    assert table(rt, [2560, 1536, 1024, 768], 8, 8, waves=2, alpha=1) == padded((1, 8, 8, 8), [(0, 4, 0)])
    # alpha 3, one wave, n = 4, G = 8 (groups of 8, 4: one item per tile; of 2: two; of 1: four):
    #   bin 0: 24 x 2048 = 49152 > 4 x 3840 = 15360; 4: 24576 >; 2: 12288 <= -> 2
    #   bin 25: 24 x 1024 = 24576 > 7168; 4: 12288 >; 2: 6144 <= -> 2
    #   bin 38: 24 x 512 = 12288 > 3072; 4: 6144 >; 2: 3072 <= -> 2        bin 44: 6144 > 1024; 3072 >; 2: 1536 >; -> 1
    assert table(rt, [2560, 1536, 1024, 768], 4, 8, waves=1, alpha=3) == padded((2, 10, 4, 8), [(0, 2, 0), (3, 1, 6)])
    # the order of the costs does not matter, only their bins: the ranks are the tile order's
    assert table(rt, [768, 2560, 1024, 1536], 4, 8, waves=1, alpha=3) == padded((2, 10, 4, 8), [(0, 2, 0), (3, 1, 6)])
    # sky behind the box: three tiles at the floor (512 -> 2047 - 409 = 1638 -> bin 51, effective cost 0) keep G -- a table
    # that is not monotone; n = 4, G = 8: their items are one per tile
    assert table(rt, [512, 2560, 1536, 512, 1024, 768, 512], 4, 8, waves=1, alpha=3) == \
        padded((3, 13, 4, 8), [(0, 2, 0), (3, 1, 6), (4, 8, 10)])
    # two tiles share bin 0 (2560 and 2559 -> 2047 - 2046 = 1 -> 0): weight 4095, count 2, R = 4095 + 1024 = 5119;
    # n = 5, G = 5, one wave, alpha 2: 10 x 4095 = 40950 <= 5 x 5119 x 2 = 51190 -> 5; bin 25: 10 x 1024 > 5 x 1024,
    # 3: 6144 >, 2: 4096 <= 5120 -> 2 (three items of 2 + 2 + 1 frames)
    assert table(rt, [2560, 1536, 2559], 5, 5, waves=1, alpha=2) == padded((2, 5, 5, 5), [(0, 5, 0), (2, 2, 2)])


def test_the_single_segment(rt):
    costs = [2560, 1536, 1024, 768, 512]
    for n in (1, 2, 7, 64):
        assert table(rt, costs, n, 1) == padded((1, 5 * n, n, 1), [(0, 1, 0)])             # G = 1: an item per tile and frame
        for G in (2, 5, 8):
            assert table(rt, costs, n, G, waves=0) == padded((1, 5 * -(-n // G), n, G), [(0, G, 0)])   # no resident waves known
    assert table(rt, costs, 1, 8) == padded((1, 5, 1, 8), [(0, 8, 0)])                     # a batch of one frame
    assert table(rt, costs, 0, 8) == padded((1, 0, 0, 8), [(0, 8, 0)])
    assert table(rt, [], 20, 5) == padded((1, 0, 20, 5), [(0, 5, 0)])                      # no tiles
    assert table(rt, [300, 512, 0], 20, 5) == padded((1, 12, 20, 5), [(0, 5, 0)])          # nothing above the floor


def profiles(n_tiles, seed):
    r = np.random.RandomState(seed)
    yield "equal", [1500] * n_tiles
    yield "sky", [512] * n_tiles
    yield "two levels", [int(x) for x in np.where(r.rand(n_tiles) < 0.4, 512, r.randint(513, 2561, n_tiles))]
    yield "ramp", [int(x) for x in np.linspace(0, 2600, n_tiles)]
    yield "one heavy", [600] * (n_tiles - 1) + [2560] if n_tiles else []
    yield "saw", [int(x) for x in (np.arange(n_tiles) % 64) * 40 + 513]


@pytest.mark.parametrize("n_tiles", [0, 1, 6, 63, 4080, 32400])
def test_every_table_covers_every_tile_and_frame_once(rt, n_tiles):
    checked = 0
    for name, costs in profiles(n_tiles, n_tiles):
        cost_sorted = sorted((min(c, MAX_COST) for c in costs), reverse=True)
        for n in (range(1, 65) if n_tiles <= 63 else (1, 2, 7, 20, 33, 64)):
            for G in sorted({1, 2, 5, min(8, n), min(16, n)} & set(range(1, n + 1))) or [1]:
                for waves, alpha in ((WAVES, 1), (WAVES, 2), (WAVES, 8), (100, 4), (1, 1), (0, 2)):
                    t = table(rt, costs, n, G, waves, alpha)
                    segs, what = segments(t), (name, n, G, waves, alpha)
                    assert 1 <= len(segs) <= MAX_SEGMENTS and t[2:4] == [n, G], what
                    assert t[HEAD + 3 * len(segs):] == [0] * (WORDS - HEAD - 3 * len(segs)), what
                    # ranks: from 0, strictly ascending, inside the tiles; items: contiguous, a segment's tiles x ceil(n / g)
                    assert segs[0][0] == 0 and segs[0][2] == 0, what
                    item = 0
                    for k, (rank, g, first) in enumerate(segs):
                        nxt = segs[k + 1][0] if k + 1 < len(segs) else n_tiles
                        assert g in halvings(G), what
                        assert first == item and (k == 0 or rank > segs[k - 1][0]) and rank <= nxt <= n_tiles, what
                        assert k == 0 or g != segs[k - 1][1], what
                        item += (nxt - rank) * -(-n // g)
                    assert t[1] == item, what
                    # every (tile, frame) pair exactly once: decode every item as the kernel does
                    if n_tiles <= 6 or (n_tiles <= 63 and (n < 4 or n % 7 == 0)):
                        seen = set()
                        for i in range(item):
                            rank, g, first = [s for s in segs if s[2] <= i][-1]
                            per = -(-n // g)
                            tile, f0 = rank + (i - first) // per, (i - first) % per * g
                            for f in range(f0, min(f0 + g, n)):
                                assert (tile, f) not in seen, what
                                seen.add((tile, f))
                        assert len(seen) == n_tiles * n, what
                    # no effective cost: the head size (the order puts those tiles last)
                    for k, (rank, g, first) in enumerate(segs):
                        nxt = segs[k + 1][0] if k + 1 < len(segs) else n_tiles
                        if nxt > rank and cost_sorted[rank] <= FLOOR:
                            assert g == G, what
                    if G == 1 or waves == 0 or n < 2:
                        assert segs == [(0, G, 0)], what
                    checked += 1
    assert checked > 100
