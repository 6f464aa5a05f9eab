"""GPU tests of the WALK COUNTS of phase D3 (run with `-m gpu` on an MI355X): g2s_d3_tables counts the rand() draws of a
draw-dependent gap's traceback for every place of the stream it can start at — a wave per (gap, deviation) by pointer
jumping over the closure's segments, or a thread per deviation by a serial walk (closures of more than 512 segments, long
lists, short lists with large tables).  Closures DESIGNED for the shapes where the jumping can go wrong go through the product's kernel by a
hook (g2s_test_d3_tables) and are compared entry by entry, bad verdicts included, with a plain restatement of the host's
serial count (post.cpp: seg_count_draws, with the checks of the host's traceback); whole lists on real graphs — short and
long, with and without guessed tracebacks, closures with many parents — against the oracle, ended on the device."""
import pytest

import cases
from test_gpu_parity import _check_batch, _compare_with_oracle_in_parallel, _gaps, _parse_scaffolds

pytestmark = pytest.mark.gpu

NONE = 0xFFFF
SOURCE = 0x4      # G2S_SUB_SOURCE
ORDERED = 0x100   # G2S_SEG_ORDERED


# ---------------------------------------------------------------------------------------------------------------------
# the serial count, from post.cpp: seg_count_draws — one state at a time down the closure, a draw per state passed and
# per parent taken — with what makes a walk the host's business (d3_device.hip: a bad walk's entry is 0 and counted)
# ---------------------------------------------------------------------------------------------------------------------
def _parents(seg):
    _, p01, p23, _ = seg
    return [p for p in (p01 & 0xFFFF, p01 >> 16, p23 & 0xFFFF, p23 >> 16) if p != NONE]


def _serial_draws(segs, n_len, lens, start_seg, rnd, at0):
    """(draws, bad) of the traceback whose first draw is value at0 of the stream `rnd` (nothing exists behind it)"""
    ns = len(segs)
    avail = len(rnd) - at0
    if avail < 1:
        return 1, True
    draws = 1
    pick = (rnd[at0] >> 1) % n_len
    d2 = lens[pick]
    i = (start_seg >> (16 * pick)) & 0xFFFF
    if i == NONE or i >= ns or d2 < 0:
        return draws, True
    t = d2 - (segs[i][0] & 0xFFFF)  # the walk begins at depth len: state len - d0 of its start segment
    if t < 0:
        return draws, True
    for _ in range(ns + 1):  # (a traceback descends: it enters a segment once)
        dl, _, _, fl = segs[i]
        draws += t  # the states t .. 1 of this segment: a draw each
        d2 -= t
        if fl & SOURCE:
            return draws, False
        if d2 <= 0:  # no depth below and no left-flank k-mer
            return draws, True
        ps = _parents(segs[i])
        if not ps or (len(ps) > 1 and not fl & ORDERED) or draws >= avail:
            return draws, True
        rv = rnd[at0 + draws] >> 1
        draws += 1
        i = ps[0] if len(ps) == 1 else ps[rv % len(ps)]
        if i >= ns:
            return draws, True
        d2 -= 1
        t = (segs[i][0] >> 16) - 1  # a parent is entered at its last state
    return draws, True


def _expected(segs, n_len, lens, start_seg, rnd, base, R, dmin, dspread):
    ent, bad = [], []
    for d in range(R + 1):
        draws, b = _serial_draws(segs, n_len, lens, start_seg, rnd, base + d)
        dev = draws - dmin
        b = b or dev < 0 or dev > dspread
        ent.append(0 if b else dev)
        bad.append(1 if b else 0)
    return ent, bad


def _compare(product, segs, n_len, lens, start_seg, rnd, base, R, dmin, dspread, want_bad=None):
    want = _expected(segs, n_len, lens, start_seg, rnd, base, R, dmin, dspread)
    ent, bad, anomalies = product.test_d3_tables(0, segs, n_len, lens[0], lens[1], start_seg, rnd, base, R, dmin, dspread)
    assert bad == want[1], "bad verdicts differ at deviations %r" % [d for d in range(R + 1) if bad[d] != want[1][d]][:10]
    assert ent == want[0], "entries differ at deviations %r" % [d for d in range(R + 1) if ent[d] != want[0][d]][:10]
    assert (anomalies > 0) == any(want[1])
    if want_bad is not None:  # (the case is what it was designed to be)
        assert want[1] == want_bad
    return want


def _stream(seed, n):
    rng = cases.SplitMix(seed)
    return [rng.next() & 0xFFFFFFFF for _ in range(n)]


def _seg(d0, ln, parents, flags):
    p = list(parents) + [NONE] * (4 - len(parents))
    return ((d0 & 0xFFFF) | (ln << 16), p[0] | (p[1] << 16), p[2] | (p[3] << 16), flags)


def _chain(ns, seed, src_d0=2):
    """ns segments of 1 to 3 states with one parent each, segment 0 on top (three states: both path lengths start in
    it), the last a source at depth src_d0; depths as a closure has them: a parent's last state lies one below its
    child's first."""
    rng = cases.SplitMix(seed)
    lens = [3] + [rng.randint(1, 3) for _ in range(ns - 1)]
    d0 = [0] * ns
    d0[ns - 1] = src_d0
    for j in range(ns - 2, -1, -1):
        d0[j] = d0[j + 1] + lens[j + 1]
    return [_seg(d0[j], lens[j], [j + 1] if j + 1 < ns else [], SOURCE if j + 1 == ns else 0) for j in range(ns)]


def _ladder(m, levels, seed, holes=False):
    """Segment 0 on top, then `levels` levels of m segments; every segment above the last level has the m segments of the
    next level as its ORDERED parents, in an order of its own; every third segment of a middle level and the whole last
    level are sources.  The draws of a walk depend on the level at which it meets a source: on the values drawn."""
    rng = cases.SplitMix(seed)
    ln = [rng.randint(1, 3) for _ in range(levels + 1)]
    ln[0] = 3
    d0 = [0] * (levels + 1)
    d0[levels] = 1
    for lv in range(levels - 1, -1, -1):
        d0[lv] = d0[lv + 1] + ln[lv + 1]
    ids = lambda lv: [0] if lv == 0 else [1 + (lv - 1) * m + x for x in range(m)]
    segs = []
    for lv in range(levels + 1):
        for x, _ in enumerate(ids(lv)):
            last = lv == levels
            ps = [] if last else ids(lv + 1)
            ps = ps[x % m:] + ps[:x % m]
            if holes and len(ps) == 3:  # (an empty slot between parents: the slots that hold a segment count)
                ps = [ps[0], NONE, ps[1], ps[2]]
            src = last or (lv > 0 and (lv * m + x) % 3 == 0)
            segs.append(_seg(d0[lv], ln[lv], ps, ORDERED | (SOURCE if src else 0)))
    return segs


def _span(segs, lens, n_len):
    """(dmin, dspread) that hold every count a walk down `segs` can come to: 1 + len - (depth of a source)"""
    src = [s[0] & 0xFFFF for s in segs if s[3] & SOURCE]
    lo = 1 + min(lens[:n_len]) - max(src)
    hi = 1 + max(lens[:n_len]) - min(src)
    return max(lo, 1), hi - max(lo, 1)


@pytest.mark.parametrize("ns", [1, 2, 63, 64, 65, 192, 193, 512, 513])
def test_chains_of_single_parents(product, ns):
    """Chains at the edges of the kernel's ways: one squaring or none, the last closure whose pointers stay in registers
    (64), the first in LDS, the last of the trace kernel's LDS (192), the last and the first beyond a lane's eight
    segments (512; 513: the serial walk over the records, unchanged) — with two path lengths that start at different
    states, picked by bit 1 of the first value, which differs from deviation to deviation."""
    segs = _chain(ns, 100 + ns)
    top = segs[0][0] & 0xFFFF
    lens = (top + 2, top)
    dmin, dspread = _span(segs, lens, 2)
    rnd = _stream(ns, 16 + 12 + lens[0] + 8)
    want = _compare(product, segs, 2, lens, 0, rnd, 11, 12, dmin, dspread)
    assert not any(want[1]) and sorted(set(want[0])) == [0, 2]  # (both lengths were picked)


@pytest.mark.parametrize("m", [2, 3, 4])
@pytest.mark.parametrize("R", [0, 1, 255, 256, 257])
def test_ladders_of_ordered_parents(product, m, R):
    """2, 3 and 4 ordered parents a segment (three: with an empty slot between them), sources at several levels: different
    deviations take different paths to different counts; 1 and 2 path lengths; deviation counts at the edges of a tile
    of 256."""
    segs = _ladder(m, 7, 31 * m + R, holes=True)
    top = segs[0][0] & 0xFFFF
    n_len = 1 + (m + R) % 2
    lens = (top + 1, top + 2)
    dmin, dspread = _span(segs, lens, n_len)
    rnd = _stream(1000 * m + R, 5 + R + dmin + dspread + 8)
    want = _compare(product, segs, n_len, lens, 0, rnd, 5, R, dmin, dspread)
    assert not any(want[1])
    if R >= 255:
        assert len(set(want[0])) >= 3


@pytest.mark.parametrize("m,levels", [(4, 40), (3, 80), (2, 255)])
def test_ladders_beyond_one_lanes_segment(product, m, levels):
    """The same with 161, 241 and 511 segments: several segments a lane, the pointers in LDS, choices at every hop"""
    segs = _ladder(m, levels, m * levels)
    top = segs[0][0] & 0xFFFF
    lens = (top + 2, top)
    dmin, dspread = _span(segs, lens, 2)
    rnd = _stream(m + levels, 3 + 40 + dmin + dspread + 8)
    want = _compare(product, segs, 2, lens, 0, rnd, 3, 40, dmin, dspread)
    assert not any(want[1]) and len(set(want[0])) >= 3


@pytest.mark.parametrize("ns", [12, 80])
@pytest.mark.parametrize("what", ["unordered", "depth0", "start_deep", "parent_id", "stream_end", "cycle", "no_start"])
def test_every_bad_verdict(product, what, ns):
    """Each way a walk can be the host's business, by construction, in a closure of one segment a lane and in one of
    several: the entry is 0 and flagged, and the list's anomaly counter says so."""
    segs = _chain(ns, 7 * ns)
    top = segs[0][0] & 0xFFFF
    lens = [top + 2, top + 1]
    n_len, start, base, R = 1, 0, 9, 9
    dmin, dspread = _span(segs, lens, 1)
    rnd = _stream(ns, base + R + dmin + dspread + 8)
    bad = [1] * (R + 1)
    mid = ns // 2
    if what == "unordered":  # two parents, their order not established: GATB's predecessor order is the host's to find
        d, p01, p23, f = segs[mid]
        segs[mid] = (d, (mid + 1) | ((mid + 2) << 16), p23, f & ~ORDERED)
    elif what == "depth0":  # the walk reaches depth 0 and no left-flank k-mer
        segs = _chain(ns, 7 * ns, src_d0=0)
        segs[-1] = segs[-1][:3] + (0,)
        top = segs[0][0] & 0xFFFF
        lens = [top + 2, top + 1]
        dmin, dspread = _span(_chain(ns, 7 * ns, src_d0=0), lens, 1)
    elif what == "start_deep":  # the start segment lies deeper than the path is long
        lens = [top - 1, top - 1]
        dmin, dspread = 1, top + 4
    elif what == "parent_id":  # a parent that is no segment of the closure
        d, _, p23, f = segs[mid]
        segs[mid] = (d, ns | (NONE << 16), p23, f)
    elif what == "stream_end":  # the stream ends one word before the last draw of the last deviation
        last_choice = 1 + lens[0] - (segs[-2][0] & 0xFFFF)  # the draw made at the first state of the segment above the source
        rnd = rnd[:base + R + last_choice]
        bad = [0] * R + [1]
    elif what == "cycle":  # two segments that point at each other
        d, _, p23, f = segs[mid + 1]
        segs[mid + 1] = (d, mid | (NONE << 16), p23, f)
    elif what == "no_start":  # the path length has no start segment
        start = NONE
    _compare(product, segs, n_len, lens, start, rnd, base, R, dmin, dspread, want_bad=bad)


# ---------------------------------------------------------------------------------------------------------------------
# whole lists, against the oracle, ended on the device
# ---------------------------------------------------------------------------------------------------------------------
def _key(r):
    return (r.count, r.left_fuz, r.right_fuz, r.flags, r.draws, r.fill, r.fill_len, tuple(r.substats), r.phaseC_count,
            tuple(r.lengths), r.backtrace_msg)


@pytest.fixture(scope="module")
def v3_genome(product, oracle):
    reads = product.G2S.synth_genome(200000, 3, 20240101)
    seqs = [ln for ln in reads.splitlines() if not ln.startswith(">")]
    og = oracle.OracleGraph(seqs, 31, 1)
    pg = product.Graph.from_seqs(seqs, 31, 1)
    yield reads, og, pg
    pg.free()
    og.free()


def _list_on_the_device(product, oracle, v3, ngaps, seed=5):
    reads, og, pg = v3
    gaps = _parse_scaffolds(product.G2S.synth_gaps(reads, 31, 10, ngaps, 100, 900, 20240103))
    sess = product.Session(pg, 0, d_err=500, randseed=seed)
    try:
        res, tm = sess.fill_batch(_gaps(product, gaps), True, pinned=True)
    finally:
        sess.destroy()
    # (a bad verdict of a walk sends the list to the host path, whose results would be equal too: it must not have)
    assert tm.resident_launches == 1 and tm.resident_fallbacks == 0
    assert tm.draw_dependent_gaps > 0 and tm.d3_table_entries >= tm.draw_dependent_gaps
    compared, q7 = _compare_with_oracle_in_parallel(product, oracle, og, gaps, res, 500, seed, threads=16)
    assert compared + q7 + sum(1 for r in res if r.count == -1) == ngaps and compared > ngaps * 9 // 10
    return [_key(r) for r in res], tm


def test_a_short_list_against_the_oracle(product, oracle, monkeypatch, v3_genome):
    """600 gaps: the two-wave fill kernel, the short list's phase D3 — its tables a wave per entry —, guesses on"""
    for v in ("G2S_TRACE_GUESS", "G2S_DEVICE_D2", "G2S_TRACE_WAVES"):
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv("G2S_RESIDENT", "1")
    _, tm = _list_on_the_device(product, oracle, v3_genome, 600)
    # (a short list's kernel goes by wave up to 128 tiles — d3_device.hip: D3_WAVE_TILES; a gap of R + 1 entries has
    # (R + 256) // 256 tiles, so the list has at most draw-dependent gaps + entries // 256: the tables went by wave)
    assert tm.draw_dependent_gaps + tm.d3_table_entries // 256 <= 128


def test_a_long_list_against_the_oracle_with_and_without_guesses(product, oracle, monkeypatch, v3_genome):
    """3 500 gaps: the one-wave fill kernel, the long list's phase D3 (classify / scan / tables — the host launches the
    by-tile kernel for every list of more than 3 072 gaps — / blocks / chain / hand-off), with G2S_TRACE_GUESS at its default
    and at 0: each the oracle's, and each other's"""
    for v in ("G2S_TRACE_GUESS", "G2S_DEVICE_D2", "G2S_TRACE_WAVES"):
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv("G2S_RESIDENT", "1")
    a, _ = _list_on_the_device(product, oracle, v3_genome, 3500)
    monkeypatch.setenv("G2S_TRACE_GUESS", "0")
    b, tb = _list_on_the_device(product, oracle, v3_genome, 3500)
    assert tb.guessed_in_fill_gaps == 0
    assert a == b


def test_a_toy_graph_with_tandem_repeats(product, oracle, monkeypatch):
    """k = 11, tandem repeats, 300 gaps: closures with many parents, cyclic ones among them"""
    monkeypatch.setenv("G2S_RESIDENT", "1")
    monkeypatch.setenv("G2S_DEVICE_D2", "1")
    seqs = cases.toy_genome(5, 6000, 11, repeats=2, tandem=1, inverted=0, snp_every=97)
    gaps = cases.cut_gaps(5, seqs[0], 11, fuz=3, ngaps=300, min_len=1, max_len=80, d_err=31)
    c, f, tm, _, _ = _check_batch(product, oracle, seqs, 11, gaps, 31)
    assert tm.resident_launches == 1 and tm.resident_fallbacks == 0
    assert tm.draw_dependent_gaps > 0 and c > 200 and f > 50
