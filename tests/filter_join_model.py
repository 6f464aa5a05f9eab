"""tests/filter_join_model.py — a brute-force model of the batched read filter's joins, written from the definitions in
gap2seq_amd/csrc/readfilter_gaps.hpp (FilterRows, FilterWindow, FilterJoin) and from neither implementation: every
window is tested against every row; there is no index, no sort key, no packed (bit, gap) word and no longest span.

For gap g with windows w0 (left), w1 (right), w2 (around):
    in_window(r, w)  w.tid >= 0, w.beg < w.end, ref_id[r] == w.tid, pos[r] < w.end, end[r] > w.beg
    B_g              { h_own[r] % bits : r mate-unmapped (flag & 8), in_window(r, w0) or in_window(r, w1) }
    list 1           every (g, r) with h_mate[r] % bits in B_g, over ALL rows
    list 2           every (g, r) with in_window(r, w2) and h_own[r] % bits not in B_g
both in ascending (g, r) order, every pair once.  nb is the size of the filter multiset before de-duplication: one
item per (window, mate-unmapped row in it), so a row in both flank windows counts twice; nu = sum |B_g|.

The bits are computed with Python integers (a 64-bit modulo cannot wrap here); numpy only compares: the positions are
held as int64 and the bits as uint64, and no arithmetic is done on either."""
import numpy as np

OK, ERR_NOMEM = 0, -5
MATE_UNMAPPED = 8


def run(case):
    """case: dict with ref_id, pos, end, flag, h_own, h_mate (lists of Python ints), bits, windows (3 (tid, beg, end)
    a gap), max_pairs.  Returns a dict: rc, list1, list2 (lists of (gap, row)), nb, nu, n1, n2 and what the case
    builders assert their properties with (per gap: the rows and the taken rows of every window)."""
    nr, bits, win = len(case["pos"]), case["bits"], case["windows"]
    n = len(win) // 3
    res = dict(rc=OK, list1=[], list2=[], nb=0, nu=0, n1=0, n2=0, in_win=[], taken=[], both_flanks=0, in_both_lists=0,
               max_bit=-1)
    if not nr or not bits or not n:
        return res
    assert n * nr <= 25_000_000, "keep gaps x rows small enough for a brute-force model"
    own = [h % bits for h in case["h_own"]]
    mate = [h % bits for h in case["h_mate"]]
    assert max(own + mate) < 1 << 64
    own_a, mate_a = np.array(own, dtype=np.uint64), np.array(mate, dtype=np.uint64)
    ref = np.array(case["ref_id"], dtype=np.int64)
    pos = np.array(case["pos"], dtype=np.int64)
    end = np.array(case["end"], dtype=np.int64)
    mu = (np.array(case["flag"], dtype=np.int64) & MATE_UNMAPPED) != 0
    none = np.zeros(nr, dtype=bool)

    def in_window(w):
        tid, beg, e = w
        if tid < 0 or beg >= e:
            return none
        assert -(1 << 62) < beg and e < (1 << 62)
        return (ref == tid) & (pos < np.int64(e)) & (end > np.int64(beg))

    list1, list2 = [], []
    for g in range(n):
        m0, m1, m2 = (in_window(win[3 * g + w]) for w in range(3))
        t0, t1 = m0 & mu, m1 & mu
        c0, c1 = int(t0.sum()), int(t1.sum())
        res["nb"] += c0 + c1
        B = set(own[r] for r in np.flatnonzero(t0 | t1)) if c0 + c1 else set()
        res["nu"] += len(B)
        if B:
            res["max_bit"] = max(res["max_bit"], max(B))
            Ba = np.array(sorted(B), dtype=np.uint64)
            r1 = np.flatnonzero(np.isin(mate_a, Ba))
            keep = m2 & ~np.isin(own_a, Ba)
        else:
            r1 = ()
            keep = m2
        r2 = np.flatnonzero(keep) if m2 is not none else ()
        list1.extend((g, int(r)) for r in r1)
        list2.extend((g, int(r)) for r in r2)
        res["in_win"].append((int(m0.sum()), int(m1.sum()), int(m2.sum())))
        res["taken"].append((c0, c1, len(r2)))
        res["both_flanks"] += bool(m0.any() and m1.any())
        if len(r1) and len(r2):
            res["in_both_lists"] += len(set(int(r) for r in r1) & set(int(r) for r in r2))
    res["n1"], res["n2"] = len(list1), len(list2)
    if res["nb"] + res["n1"] + res["n2"] > case["max_pairs"]:  # (the three checks of the joins: the sums only grow)
        res["rc"] = ERR_NOMEM
        return res
    res["list1"], res["list2"] = list1, list2
    return res
