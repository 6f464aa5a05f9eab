"""The planner of the graph build's key-range passes (gap2seq_amd/csrc/pass_plan.cpp) through g2s_test_plan_passes: a
histogram over consecutive key ranges is cut, in order, into passes of at most `cap` keys.  CPU only; the passes
themselves run in tests/test_gpu_build_passes.py."""
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gap2seq_amd import lib as P  # noqa: E402


def _greedy(hist, cap):
    """the cut by brute force: a pass is closed in front of the first bin that would take it beyond cap"""
    first, cur = [], []
    for b, h in enumerate(hist):
        if b == 0 or sum(cur) + h > cap:
            first.append(b)
            cur = []
        cur.append(h)
    over = [b for b, h in enumerate(hist) if h > cap]
    return first, (over[0] if over else None)


def _passes(hist, first):
    ends = first[1:] + [len(hist)]
    return [hist[a:b] for a, b in zip(first, ends)]


def _check_cover(hist, first):
    assert first[0] == 0 and first == sorted(set(first)) and first[-1] < len(hist)  # in order, every bin in one pass


def test_uniform_histogram():
    hist = [10] * 4096
    for cap in (10, 25, 1000, 4095, 40960 - 1):
        first, over = P.test_plan_passes(hist, cap)
        assert over is None
        _check_cover(hist, first)
        sums = [sum(p) for p in _passes(hist, first)]
        assert max(sums) <= cap and sum(sums) == sum(hist)
        assert all(s == (cap // 10) * 10 for s in sums[:-1])  # every pass but the last is as full as bins allow
        assert len(first) == -(-4096 // (cap // 10))


def test_empty_bins_at_the_ends_and_in_the_middle():
    hist = [0, 0, 0, 5, 5, 0, 0, 0, 0, 5, 5, 5, 0, 0]
    first, over = P.test_plan_passes(hist, 10)
    assert over is None
    _check_cover(hist, first)
    assert [sum(p) for p in _passes(hist, first)] == [10, 10, 5]
    assert first == [0, 9, 11]  # empty bins join the open pass
    assert P.test_plan_passes([0] * 7, 3) == ([0], None)
    assert P.test_plan_passes([0, 0, 4], 4) == ([0], None)


def test_a_bin_equal_to_cap_stands_alone():
    hist = [3, 7, 2, 0, 1]
    first, over = P.test_plan_passes(hist, 7)
    assert over is None
    assert first == [0, 1, 2]
    assert [sum(p) for p in _passes(hist, first)] == [3, 7, 3]


def test_a_bin_beyond_cap_is_reported():
    hist = [3, 2, 8, 0, 1, 9]
    first, over = P.test_plan_passes(hist, 7)
    assert over == 2
    assert first == [0, 2, 3, 5]  # the oversized bin alone: even the empty bin behind it opens a new pass
    assert _passes(hist, first)[1] == [8] and _passes(hist, first)[3] == [9]
    first, over = P.test_plan_passes([0, 0, 8], 7)
    assert (first, over) == ([0, 2], 2)  # (the bins in front of it: a pass without keys)


def test_cap_of_the_total_gives_one_pass():
    rr = random.Random(5)
    hist = [rr.randrange(0, 50) for _ in range(300)]
    assert P.test_plan_passes(hist, sum(hist)) == ([0], None)
    assert P.test_plan_passes(hist, sum(hist) + 12345) == ([0], None)
    assert P.test_plan_passes(hist, 2 ** 64 - 1) == ([0], None)
    assert len(P.test_plan_passes(hist, sum(hist) - 1)[0]) == 2


def test_against_the_brute_force_cut():
    rr = random.Random(20240607)
    for _ in range(300):
        nb = rr.choice([1, 2, 3, 16, 64, 257, 1024])
        top = rr.choice([1, 3, 100, 10 ** 6, 2 ** 40])
        hist = [0 if rr.random() < 0.3 else rr.randrange(0, top + 1) for _ in range(nb)]
        cap = rr.choice([1, max(1, top // 2), top, 3 * top, max(1, sum(hist) // 5)])
        first, over = P.test_plan_passes(hist, cap)
        assert (first, over) == _greedy(hist, cap), (hist, cap)
        _check_cover(hist, first)
        for p in _passes(hist, first):
            assert sum(p) <= cap or len(p) == 1
