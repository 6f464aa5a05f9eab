"""tests/filter_join_cases.py — the inputs of the join-level tests of the batched read filter, shared by
tests/test_filter_join.py (host joins) and tests/test_gpu_filter_join.py (device joins).  A case is a dict of rows
(ref_id, pos, end, flag, h_own, h_mate), the longest span, the filter's bits, three windows a gap and the pair cap — what
g2s_test_filter_join takes — and tests/filter_join_model.py says what the joins must return for it.

Every case is built from random.Random(seed) alone, and every named case asserts, WITH THE MODEL, the property it is
named for (a case that stopped exercising its edge fails in the builder, on the CPU, before any join runs)."""
import random

import filter_join_model as M

INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
PAIRED, UNMAPPED, MATE_UNMAPPED, READ1, READ2, SECONDARY, SUPPLEMENTARY = 1, 4, 8, 64, 128, 256, 2048
NO_CAP = 1 << 40
HUGE_BITS = 5 * ((1 << 32) - 2)  # the documented limit: fewer than 2^32 - 1 records, five bits a record
NONE = (-1, 0, 0)                # a window that holds nothing


def make(name, rows, windows, bits, max_pairs=NO_CAP):
    """rows: (ref_id, pos, end, flag, h_own, h_mate); max_span as pass A of the filter computes it"""
    assert len(windows) % 3 == 0
    for r in rows:
        assert INT32_MIN <= r[1] <= INT32_MAX and -1 <= r[0] <= INT32_MAX and r[2] > r[1] and 0 <= r[4] < 1 << 64 and 0 <= r[5] < 1 << 64
    case = dict(name=name, ref_id=[r[0] for r in rows], pos=[r[1] for r in rows], end=[r[2] for r in rows],
                flag=[r[3] for r in rows], h_own=[r[4] for r in rows], h_mate=[r[5] for r in rows],
                max_span=max([1] + [r[2] - r[1] for r in rows if r[0] >= 0]), bits=bits, windows=list(windows),
                max_pairs=max_pairs)
    case["model"] = M.run(case)
    return case


def long_tailed(rng):
    return rng.choice([1, rng.randrange(1, 151), rng.randrange(1, 151), rng.randrange(1, 151), rng.randrange(150, 3000),
                       rng.randrange(3000, 60000) if rng.random() < 0.2 else 50])


def library(rng, nr, nrefs, hash_of, span=None, scale=None, p_mu=0.25, p_copy=0.05, p_unplaced=0.03):
    """nr rows of a paired library in coordinate order: pairs with both ends mapped, pairs with one end unmapped and
    placed at its mate (end = pos + 1), secondary / supplementary copies of a record (the same two hashes again) and
    records without a reference.  hash_of() draws a name's hash."""
    span = span or (lambda: rng.randrange(1, 151))
    scale = scale or max(200, 12 * nr // nrefs)
    rows = []
    while len(rows) < nr:
        a, b = hash_of(), hash_of()
        u = rng.random()
        if u < p_unplaced:
            rows.append((-1, rng.choice([-1, 0, rng.randrange(scale), INT32_MAX]), 0, PAIRED | UNMAPPED | MATE_UNMAPPED | READ1, a, b))
            rows[-1] = rows[-1][:2] + (rows[-1][1] + 1,) + rows[-1][3:]
            continue
        tid, p = rng.randrange(nrefs), rng.randrange(scale)
        if u < p_unplaced + p_mu:
            rows.append((tid, p, p + span(), PAIRED | MATE_UNMAPPED | READ1, a, b))
            rows.append((tid, p, p + 1, PAIRED | UNMAPPED | READ2, b, a))
        else:
            q = p + rng.randrange(0, 400)
            rows.append((tid, p, p + span(), PAIRED | READ1, a, b))
            rows.append((tid, q, q + span(), PAIRED | READ2 | 16, b, a))
        if rng.random() < p_copy:
            src = rows[rng.randrange(len(rows))]
            if src[0] >= 0:
                p2 = rng.randrange(scale)
                rows.append((src[0], p2, p2 + span(), src[3] | rng.choice([SECONDARY, SUPPLEMENTARY]), src[4], src[5]))
    rows = rows[:nr]
    rows.sort(key=lambda r: (r[0] if r[0] >= 0 else 1 << 40, r[1]))
    return rows


def windows_at_rows(rng, rows, n, width=lambda rng: rng.randrange(1, 400)):
    """three windows a gap, drawn relative to the rows' positions so that they hit; now and then an empty, an invalid
    or a far window"""
    placed = [r for r in rows if r[0] >= 0] or [(0, 0, 1)]
    out = []
    for _ in range(n):
        tid, p = rng.choice(placed)[:2]
        for w in range(3):
            u = rng.random()
            if u < 0.08:
                out.append(rng.choice([NONE, (tid, p, p), (tid, p + 5, p), (tid + 50, p, p + 100)]))
            else:
                beg = p + rng.randrange(-300, 300)
                out.append((tid, beg, beg + width(rng)))
    return out


def small_hash(rng, k):
    return lambda: rng.randrange(k)


def any_hash(rng):
    return lambda: rng.getrandbits(64)


# ---- the named cases

def dense_collisions():
    out = []
    for bits in (1, 2, 7):
        rng = random.Random(100 + bits)
        rows = library(rng, 300, 2, any_hash(rng), p_mu=0.4)
        c = make("dense-bits%d" % bits, rows, windows_at_rows(rng, rows, 36, lambda rng: rng.randrange(1000, 1800)), bits)
        m = c["model"]
        assert m["nb"] >= 3 * m["nu"] > 0, (m["nb"], m["nu"])                     # U de-duplicates heavily
        assert m["n1"] >= 0.5 * 300 * 36, m["n1"]                                 # list 1 close to rows x gaps
        assert m["n2"] <= 0.5 * sum(w[2] for w in m["in_win"]) and m["n2"] < m["n1"]  # list 2 mostly suppressed
        out.append(c)
    return out


def high_bits():
    rng = random.Random(7)
    bits = HUGE_BITS
    special = [0, 1, 1 << 32, bits - 2, bits - 1]
    rows = []
    for i, h in enumerate(special):  # a mate-unmapped read whose own bit is h, its mate, and a far read colliding with it
        other = rng.randrange(bits)
        rows.append((0, 1000 + 10 * i, 1050 + 10 * i, PAIRED | MATE_UNMAPPED | READ1, h, other))
        rows.append((0, 1000 + 10 * i, 1001 + 10 * i, PAIRED | UNMAPPED | READ2, other, h))
        rows.append((1, 5000 + i, 5050 + i, PAIRED | READ2, rng.randrange(bits), h))
        rows.append((0, 1200 + i, 1250 + i, PAIRED | READ1, h, rng.randrange(bits)))      # in the flanks, in the filter
        rows.append((0, 1200 + i, 1250 + i, PAIRED | READ1, h ^ 4, rng.randrange(bits)))  # in the flanks, not in it
    lib_rng = random.Random(8)
    rows += library(lib_rng, 400, 2, lambda: lib_rng.randrange(bits))
    rows.sort(key=lambda r: (r[0] if r[0] >= 0 else 1 << 40, r[1]))
    assert all(r[4] < bits and r[5] < bits for r in rows)  # hash % bits == hash
    win = []
    for g in range(12):
        win += [(0, 990 + 10 * (g % 5), 1100), (0, 1005, 1015 + g), (0, 1100, 1300)]
    win += windows_at_rows(rng, rows, 20)
    c = make("high-bits", rows, win, bits)
    m = c["model"]
    assert m["max_bit"] == bits - 1 and (m["max_bit"] << 29) >= 1 << 63     # a (bit, gap) pair beyond 2^63
    top = [r for r in range(len(rows)) if rows[r][5] == bits - 1]
    assert len(top) >= 2 and all((0, r) in m["list1"] for r in top)         # mates of bit `bits - 1` find their range
    assert m["n2"] > 0 and m["nb"] > m["nu"]
    return [c]


def overlapping_flanks():
    rng = random.Random(11)
    rows = library(rng, 200, 1, any_hash(rng), scale=3000)
    a, b = rng.getrandbits(64), rng.getrandbits(64)
    rows += [(0, 1500, 1550, PAIRED | MATE_UNMAPPED | READ1, a, b),                       # in both windows below
             (0, 1480, 1530, PAIRED | MATE_UNMAPPED | READ1 | SECONDARY, a, b),           # the same name twice more:
             (0, 1560, 1600, PAIRED | MATE_UNMAPPED | READ1 | SUPPLEMENTARY, a, b),       # secondary, supplementary
             (0, 1500, 1501, PAIRED | UNMAPPED | READ2, b, a)]
    rows.sort(key=lambda r: (r[0] if r[0] >= 0 else 1 << 40, r[1]))
    win = [(0, 1400, 1540), (0, 1520, 1700), (0, 1300, 1800),
           (0, 1450, 1520), (0, 1450, 1520), (0, 0, 3000),        # the two flank windows identical
           (0, 1540, 1541), (0, 1000, 1560), NONE]
    c = make("overlapping-flanks", rows, win + windows_at_rows(rng, rows, 10), 5 * len(rows))
    m = c["model"]
    assert m["both_flanks"] >= 3 and m["nb"] > m["nu"]
    assert all(w[0] > 0 and w[1] > 0 for w in m["in_win"][:3])
    return [c]


def spans():
    rng = random.Random(13)
    rows = [(0, 1000, 1_001_000, PAIRED | MATE_UNMAPPED | READ1, 17, 18), (0, 1000, 1001, PAIRED | UNMAPPED | READ2, 18, 17)]
    hashes = iter(range(100, 1 << 30))
    for _ in range(3000):
        p = rng.randrange(0, 1_100_000)
        rows.append((0, p, p + rng.randrange(1, 151), PAIRED | (MATE_UNMAPPED if rng.random() < 0.3 else 0) | READ1,
                     next(hashes), next(hashes)))
    rows.sort(key=lambda r: (r[0], r[1]))
    win = []
    for beg in (900_000, 500_000, 1_000_990, 1_000_999, 1_001_000, 2000, 999, 1000):
        win += [(0, beg, beg + 100), (0, beg + 50, beg + 60), (0, beg - 200, beg + 200)]
    win += [NONE, NONE, (0, 700_000, 700_010)]
    c = make("span-1e6", rows, win, 5 * len(rows))
    m = c["model"]
    assert c["max_span"] == 1_000_000
    long_row = rows.index((0, 1000, 1_001_000, PAIRED | MATE_UNMAPPED | READ1, 17, 18))
    assert rows[long_row + 1][4] == 18
    for g in range(4):  # far windows take the long row; the short rows the widened range sweeps in are rejected
        beg, e = win[3 * g][1:]
        swept = sum(1 for r in rows if beg - c["max_span"] < r[1] < e)
        assert swept >= 1000 and 1 <= m["in_win"][g][0] <= 60, (swept, m["in_win"][g])
        assert (g, long_row + 1) in m["list1"]   # (the long row's mate: the long row is in the filter of gap g)
    assert (4, long_row + 1) not in m["list1"]   # [1 001 000, ...) begins at the long row's end: not in it
    assert all((g, long_row + 1) in m["list1"] and (g, long_row) not in m["list2"] for g in (5, 6, 7))
    assert (8, long_row) in m["list2"]           # in the flanks of a gap whose filter is empty
    rng = random.Random(14)
    rows1 = []
    for i in range(600):  # every row a placed unmapped read: end = pos + 1
        p = rng.randrange(0, 500)
        rows1.append((rng.randrange(2), p, p + 1, PAIRED | UNMAPPED | (MATE_UNMAPPED if i % 3 == 0 else 0) | READ1,
                      rng.getrandbits(64), rng.getrandbits(64)))
    rows1.sort(key=lambda r: (r[0], r[1]))
    c1 = make("span-1", rows1, windows_at_rows(rng, rows1, 40, lambda rng: rng.randrange(1, 6)), 5 * len(rows1))
    assert c1["max_span"] == 1 and c1["model"]["nb"] > 0 and c1["model"]["n2"] > 0
    return [c, c1]


def coordinates():
    rng = random.Random(17)
    h = any_hash(rng)
    rows = []
    T = 5
    for tid in (T - 1, T, T + 1, 70_000, 69_999):
        for p in (-1, 0, INT32_MAX - 1, INT32_MAX, INT32_MIN, 1 << 30):
            for sp in (1, 100):
                a, b = h(), h()
                rows.append((tid, p, p + sp, PAIRED | MATE_UNMAPPED | READ1, a, b))
                rows.append((tid, p, p + 1, PAIRED | UNMAPPED | READ2, b, a))
    for p in (-1, 0, 12345, INT32_MAX, INT32_MIN):  # no reference, any position
        rows.append((-1, p, p + 1, PAIRED | UNMAPPED | MATE_UNMAPPED | READ1, h(), h()))
        rows.append((-1, p, p + 77, PAIRED | MATE_UNMAPPED | READ2, h(), h()))
    rng.shuffle(rows)
    spots = [(-5, (1 << 31) + 5), (0, 1 << 40), (INT32_MIN - 10, 10), (-(1 << 40), 1), (-(1 << 40), 1 << 40),
             (INT32_MAX, (1 << 31) + 5), (INT32_MAX - 1, INT32_MAX), ((1 << 31) + 5, (1 << 31) + 50), (-1, 0), (-2, -1),
             (0, 1), (INT32_MIN, INT32_MIN + 1), (INT32_MIN - 100, INT32_MIN + 50), ((1 << 30) - 10, (1 << 30) + 10),
             (5, 5), (10, 5), ((1 << 40), (1 << 40) + 9)]
    win = []
    for tid in (T, 70_000):
        for i, (beg, e) in enumerate(spots):
            b2, e2 = spots[(i + 1) % len(spots)]
            win += [(tid, beg, e), (tid, b2, e2), (tid, beg, e)]
    win += [(-1, 0, 1 << 40), (-1, -5, 5), (-1, 0, 1 << 40), (T, 7, 7), (T, 9, 3), (T, 1 << 40, 0)]
    win += [(T + 2, -(1 << 40), 1 << 40)] * 3 + [(T - 2, -(1 << 40), 1 << 40)] * 3   # references without a row
    c = make("coordinates", rows, win, 5 * len(rows))
    m = c["model"]
    assert c["max_span"] == 100
    # a reference holds 24 rows: 6 positions x (a read of span 1, one of span 100, and their two placed mates)
    assert m["in_win"][0][0] == 20     # [-5, 2^31 + 5): all but the four at INT32_MIN
    assert m["in_win"][1][0] == 17     # [0, 2^40): of those at -1 only the span-100 read reaches 0
    assert m["in_win"][4][0] == 24     # [-2^40, 2^40)
    assert m["in_win"][7][0] == 2      # [2^31 + 5, 2^31 + 50): the span-100 reads at INT32_MAX - 1 and INT32_MAX
    assert m["in_win"][2][0] == 12 and m["in_win"][3][0] == 12     # beg - max_span + 1 < INT32_MIN: -1, 0, INT32_MIN
    g_ff = 2 * len(spots)
    assert m["in_win"][g_ff] == (0, 0, 0) and m["in_win"][g_ff + 1] == (0, 0, 0)   # tid -1; beg >= end
    assert m["in_win"][g_ff + 2] == (0, 0, 0) and m["in_win"][g_ff + 3] == (0, 0, 0)
    assert any(w[0] > 0 for w in m["in_win"][len(spots):2 * len(spots)])           # tid 70 000
    return [c]


def row_order():
    rng = random.Random(19)
    base = library(rng, 500, 2, any_hash(rng), scale=300, p_copy=0.15)
    for i in range(100):  # a hundred rows at one (ref_id, pos): their order inside a gap is the row order
        base.append((0, 50, 50 + 1 + i % 7, PAIRED | READ1 | (MATE_UNMAPPED if i % 3 == 0 else 0), rng.getrandbits(64), rng.getrandbits(64)))
    base.sort(key=lambda r: (r[0] if r[0] >= 0 else 1 << 40, r[1]))
    win = [(0, 40, 60)] * 3 + windows_at_rows(rng, base, 50)
    bits = 5 * len(base)
    out = [make("order-sorted", base, win, bits)]
    want = out[0]["model"]
    assert want["n1"] > 100 and want["n2"] > 100 and want["in_win"][0][2] >= 100 and want["taken"][0][0] >= 34
    perm = list(range(len(base)))
    rng.shuffle(perm)
    for label, p in (("order-shuffled", perm), ("order-reversed", list(range(len(base)))[::-1])):
        c = make(label, [base[i] for i in p], win, bits)
        for key in ("list1", "list2"):  # the same lists up to the renumbering of the rows
            assert sorted((g, p[r]) for g, r in c["model"][key]) == want[key], label
        out.append(c)
    return out


EDGE_COUNTS = (0, 1, 63, 64, 65, 127, 128, 129, 1000)


def wave_edges():
    """One reference per construction, every row of it a candidate of the window [0, 10^6) in position order, so the
    rank of a row on its reference is its place (chunk, lane) in the joins' walk.  Mode 0 takes the mate-unmapped
    rows; mode 1 takes the rows whose name is not in the gap's filter — the filter here holds the one name SUPPRESSED
    (hash 1), put there by a mate-unmapped row on reference 0 that window 0 of the mode 1 gaps covers."""
    rows = [(0, 10, 60, PAIRED | MATE_UNMAPPED | READ1, 1, 2)]
    win, expect = [], []
    fresh = iter(range(1000, 1 << 30))
    tid = 1

    def reference(pattern):  # pattern[i]: row i of the reference is taken
        nonlocal tid
        for i, t in enumerate(pattern):
            # mode 0: taken = mate unmapped; mode 1: not taken = own hash 1 (in the filter)
            rows.append((tid, 2 * i, 2 * i + 1 + i % 3, PAIRED | READ1 | (MATE_UNMAPPED if t else 0), next(fresh), next(fresh)))
        win.extend([(tid, 0, 10 ** 6), NONE, NONE])
        expect.append((0, len(pattern), sum(pattern)))
        tid += 1
        for i, t in enumerate(pattern):
            rows.append((tid, 2 * i, 2 * i + 1 + i % 3, PAIRED | READ1, next(fresh) if t else 1, next(fresh)))
        win.extend([(0, 0, 100), NONE, (tid, 0, 10 ** 6)])
        expect.append((1, len(pattern), sum(pattern)))
        tid += 1

    rng = random.Random(23)
    for c in EDGE_COUNTS:
        reference([True] * c)                       # c candidates, all taken
        pat = [True] * c + [False] * (c + 7)        # c taken among 2c + 7 candidates
        rng.shuffle(pat)
        reference(pat)
        reference([False] * c)                      # c candidates, none taken
    lanes = {"lane0": [i == 0 for i in range(64)], "lane63": [i == 63 for i in range(64)],
             "alternating": [i % 2 == 0 for i in range(64)], "odd": [i % 2 == 1 for i in range(64)],
             "second-chunk-lane0": [False] * 64 + [True] + [False] * 63, "first-chunk-lane63-then-all": [i >= 63 for i in range(128)]}
    for pat in lanes.values():
        reference(pat)
    case = make("wave-edges", rows, win, 5 * len(rows))
    m = case["model"]
    for g, (mode, cand, taken) in enumerate(expect):
        if mode == 0:
            assert m["in_win"][g][0] == cand and m["taken"][g][0] == taken, (g, m["in_win"][g], m["taken"][g])
        else:
            assert m["in_win"][g][2] == cand and m["taken"][g][2] == taken, (g, m["in_win"][g], m["taken"][g])
    for mode in (0, 1):
        assert set(EDGE_COUNTS) <= set(e[1] for e in expect if e[0] == mode)
        assert set(EDGE_COUNTS) <= set(e[2] for e in expect if e[0] == mode and e[1] > e[2])
    return [case]


GAP_COUNTS = (1, 2, 3, 4, 5, 255, 256, 257, 65_535, 65_536, 65_537)


def gap_counts():
    out = []
    for n in GAP_COUNTS:
        rng = random.Random(1000 + n)
        rows = library(rng, 200, 2, any_hash(rng), scale=2000)
        few = windows_at_rows(rng, rows, min(n, 64))
        win = []
        for g in range(n):
            if n <= 300 or g >= n - 3 or g % 1021 == 0 or (g & (g - 1)) == 0:
                win += few[3 * (g % (len(few) // 3)):][:3]
            else:  # light gaps: one narrow window each
                p = rng.randrange(2000)
                win += [NONE, (g % 2, p, p + 3), NONE] if g % 5 else [(g % 2, p, p + 3), NONE, NONE]
        win[-3:] = [(0, 0, 2000), (1, 0, 2000), (0, 500, 1500)]   # the last gap owns pairs in both lists
        c = make("gaps-%d" % n, rows, win, 5 * len(rows))
        m = c["model"]
        assert m["list1"][-1][0] == n - 1 and m["list2"][-1][0] == n - 1
        assert n < 4 or (m["list1"][0][0] < n // 2 and m["list2"][0][0] < n // 2)
        out.append(c)
    return out


def degenerate():
    rng = random.Random(29)
    mapped = [r[:3] + (r[3] & ~MATE_UNMAPPED,) + r[4:] for r in library(rng, 300, 2, any_hash(rng))]
    c0 = make("no-filter-rows", mapped, windows_at_rows(rng, mapped, 30), 5 * len(mapped))
    assert c0["model"]["nb"] == 0 and c0["model"]["n1"] == 0 and c0["model"]["n2"] > 0
    # nb > 0, n1 = 0: the names in the filter are nobody's mate name
    rows = [(0, 10 * i, 10 * i + 50, PAIRED | MATE_UNMAPPED | READ1, 2 * i, 2 * i + 1001) for i in range(100)]
    c1 = make("no-mates", rows, windows_at_rows(rng, rows, 20), 5000)
    assert c1["model"]["nb"] > 0 and c1["model"]["n1"] == 0 and c1["model"]["n2"] > 0
    rows = library(rng, 300, 2, any_hash(rng))
    win = windows_at_rows(rng, rows, 30)
    for g in range(30):
        win[3 * g + 2] = rng.choice([NONE, (0, 7, 7), (0, 9, 2)])
    c2 = make("no-flank-rows", rows, win, 5 * len(rows))
    assert c2["model"]["nb"] > 0 and c2["model"]["n1"] > 0 and c2["model"]["n2"] == 0
    full = [(0, 0, 1 << 20)] * 3
    c3 = make("no-rows", [], full * 4, 100)
    c4 = make("no-gaps", rows, [], 5 * len(rows))
    c5 = make("no-bits", rows, windows_at_rows(rng, rows, 5), 0)
    for c in (c3, c4, c5):
        assert c["model"]["rc"] == M.OK and c["model"]["list1"] == [] and c["model"]["list2"] == []
    # one row and one gap: every scan is over one element.  In the filter, the row is its own mate's bit (one list 1
    # pair) and its flank window gives nothing (a total of zero behind a scan that ran); out of it, only list 2 has it
    one = [(0, 90, 120), NONE, (0, 50, 200)]
    c6 = make("one-row-one-gap", [(0, 100, 150, PAIRED | MATE_UNMAPPED | READ1, 7, 12)], one, 5)
    assert (c6["model"]["nb"], c6["model"]["n1"], c6["model"]["n2"]) == (1, 1, 0)
    c7 = make("one-row-one-gap-flank", [(0, 100, 150, PAIRED | READ1, 7, 12)], one, 5)
    assert (c7["model"]["nb"], c7["model"]["n1"], c7["model"]["n2"]) == (0, 0, 1)
    return [c0, c1, c2, c3, c4, c5, c6, c7]


def pair_cap():
    rng = random.Random(31)
    rows = library(rng, 400, 2, any_hash(rng))
    win = windows_at_rows(rng, rows, 25)
    bits = 5 * len(rows)
    m = make("cap-free", rows, win, bits)["model"]
    nb, n1, n2 = m["nb"], m["n1"], m["n2"]
    assert nb > 1 and n1 > 0 and n2 > 0
    out = []
    for label, cap, rc in (("cap-nb-1", nb - 1, M.ERR_NOMEM), ("cap-nb+n1-1", nb + n1 - 1, M.ERR_NOMEM),
                           ("cap-nb+n1+n2-1", nb + n1 + n2 - 1, M.ERR_NOMEM), ("cap-exact", nb + n1 + n2, M.OK),
                           ("cap-nb", nb, M.ERR_NOMEM), ("cap-nb+n1", nb + n1, M.ERR_NOMEM)):
        c = make(label, rows, win, bits, max_pairs=cap)
        assert c["model"]["rc"] == rc
        out.append(c)
    assert out[3]["model"]["list1"] == m["list1"] and out[3]["model"]["list2"] == m["list2"]
    return out


SWEEP = 40


def sweep():
    out = []
    for seed in range(SWEEP):
        rng = random.Random(5000 + seed)
        nr, n, nrefs = rng.randrange(1, 5001), rng.randrange(1, 301), rng.randrange(1, 5)
        kind = ("small", "5nr", "huge")[seed % 3]
        bits = {"small": rng.randrange(1, 64), "5nr": 5 * nr, "huge": HUGE_BITS}[kind]
        hash_of = any_hash(rng) if kind != "huge" or seed % 2 else (lambda: rng.randrange(HUGE_BITS - 3, HUGE_BITS + 3) if rng.random() < 0.1 else rng.getrandbits(64))
        rows = library(rng, nr, nrefs, hash_of, span=lambda: long_tailed(rng))
        if seed % 4 == 1:
            rng.shuffle(rows)
        wide = seed % 5 == 0
        win = windows_at_rows(rng, rows, n, (lambda rng: rng.randrange(1, 4000)) if wide else (lambda rng: rng.randrange(1, 400)))
        out.append(make("sweep-%02d-%s" % (seed, kind), rows, win, bits))
    ms = [c["model"] for c in out]
    assert any(m["nb"] > m["nu"] for m in ms)
    assert any(m["both_flanks"] for m in ms)
    assert any(m["in_both_lists"] for m in ms)
    assert any(max(max(t) for t in m["taken"]) > 64 for m in ms)
    assert sum(1 for m in ms if m["n1"] and m["n2"]) >= SWEEP * 3 // 4
    return out


_CASES = None


def named_cases():
    return (dense_collisions() + high_bits() + overlapping_flanks() + spans() + coordinates() + row_order() + wave_edges() +
            gap_counts() + degenerate() + pair_cap())


def all_cases():
    """every case, built (and its model run) once a process"""
    global _CASES
    if _CASES is None:
        _CASES = named_cases() + sweep()
        assert len(set(c["name"] for c in _CASES)) == len(_CASES)
    return _CASES


def sweep_cases():
    return [c for c in all_cases() if c["name"].startswith("sweep-")]


def run(P, case, device=-1, threads=1):
    """the hook on a case -> (rc, list 1, list 2, message)"""
    return P.test_filter_join(case["ref_id"], case["pos"], case["end"], case["flag"], case["h_own"], case["h_mate"],
                              case["max_span"], case["bits"], case["windows"], case["max_pairs"], device=device,
                              threads=threads)


def check(P, case, device=-1, threads=1):
    """exact equality with the model: the return code and both lists; the cap's message where the cap is hit"""
    rc, l1, l2, msg = run(P, case, device=device, threads=threads)
    m = case["model"]
    assert rc == m["rc"], (case["name"], rc, msg)
    if m["rc"] == M.ERR_NOMEM:
        assert "cap" in msg, msg
    assert len(l1) == len(m["list1"]) and len(l2) == len(m["list2"]), (case["name"], len(l1), len(m["list1"]), len(l2), len(m["list2"]))
    assert l1 == m["list1"], (case["name"], "list 1", first_difference(l1, m["list1"]))
    assert l2 == m["list2"], (case["name"], "list 2", first_difference(l2, m["list2"]))
    return rc, l1, l2


def first_difference(a, b):
    for i, (x, y) in enumerate(zip(a, b)):
        if x != y:
            return i, x, y
    return min(len(a), len(b)), None, None
