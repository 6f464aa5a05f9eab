"""The pending-event limit of both segment kernels and every capacity of the large variant g2s_fill_segw (run with
`-m gpu` on an MI355X).  The planted gaps of cases.FRONTIER_EDGES and cases.SEGW_EDGES sit one below, on and one above
the 64 event lanes of g2s_fill_seg / g2s_fill_seg2, the ring of G2S_SEGX_PE = 1024 event slots, G2S_SEGX_CAP = 16384
logged segments and G2S_SEGX_EA = 6144 right-set entries, and on both sides of M = 8, 64, 512 and 4096 merged
intervals, where the search of the right set reads one more level.  tests/test_seg_model.py proves on the host that
each gap is where the tables say; here every case asserts from the library's own records (G2S_SEG_DUMP, g2s_timing)
that the kernels count the same and route the gap accordingly, and that what they computed is the oracle's, field
by field, on every route.  What the dump does not carry (M, the peak of pending events, sweeps of the event table)
is the model's: the exact equality of entries, segments, rounds, flags and results ties the model to the kernels."""
import pytest

import cases
from test_gpu_edges import _seg_dump
from test_gpu_parity import _check_batch

pytestmark = pytest.mark.gpu
K = 31
E = 10
OVF_A, OVF_B, WHY_FRONTIER, WHY_LOG, WHY_RS = 0x4, 0x8, 0x100, 0x400, 0x800
REASONS = OVF_A | OVF_B | WHY_FRONTIER | WHY_LOG | WHY_RS
PATH_VARS = ("G2S_NO_SEG_TIER", "G2S_NO_SEGX_TIER", "G2S_FORCE_SEGX", "G2S_SEG_WAVES", "G2S_RESIDENT", "G2S_HOST_BUILD")
FRONTIER = sorted(cases.FRONTIER_EDGES)
# The frontier rows are one list on one graph among 100 ordinary gaps (the segment tier packs a list's closures into
# a buffer of 64 segments a gap on average, the large variant into 2048 a gap, each with a full log to spare: the
# largest closure here, 5 205 segments, fits a list of its own).  Every row of SEGW_EDGES is a list of its own: the
# three rows around a capacity share their sequences, and M holds on the row's own graph only.
GROUPS = {"frontier": FRONTIER}
GROUPS.update({name: [name] for name in sorted(cases.SEGW_EDGES)})


def _group(name, monkeypatch):
    for v in PATH_VARS:
        monkeypatch.delenv(v, raising=False)
    names = GROUPS[name]
    if any("M" in cases.LIMIT_EDGES[n][2] for n in names):
        monkeypatch.setenv("G2S_HOST_BUILD", "1")  # (M depends on the numbering of the unitigs: the host build's)
    seqs, gaps, idx = cases.limit_edge_list(names, pad=100 if name == "frontier" else 0)
    return names, seqs, gaps, idx


def _regular_tier(w):
    """Overflow and reason bits a row leaves the regular tier with (0: it stays).  The right set is counted first;
    in phase B a full log is seen at the head of a round, a child without a lane at its end: the log rows meet the
    log long before their 65th event (tests/test_seg_model.py: reg_first)."""
    if w["nA"] > 256:
        return OVF_A | WHY_RS
    if w["nseg"] > 16000:
        return OVF_B | WHY_LOG
    if w["ev"] > 64:
        return OVF_B | WHY_FRONTIER
    assert w["nseg"] <= 512
    return 0


def _large_variant(w):
    if w["nA"] > 6144:
        return OVF_A | WHY_RS
    if w["nseg"] > 16384:
        return OVF_B | WHY_LOG
    if w["ring"] > 1024:
        return OVF_B | WHY_FRONTIER
    return 0


def _seg_dump_rounds(product, monkeypatch, tmp_path, seqs, gaps, waves):
    """test_gpu_edges' _seg_dump with roundsB beside (nA, nseg, flags) of every dump line."""
    _, tm, res = _seg_dump(product, monkeypatch, tmp_path, seqs, gaps, waves, E)
    recs = {}
    for line in open(tmp_path / ("dump_%s.txt" % waves)):
        w = line.split()
        if w[0] == "gap":
            recs.setdefault(int(w[1]), []).append((int(w[3]), int(w[5]), int(w[7], 16), int(w[11])))
    return recs, tm, res


@pytest.mark.parametrize("waves", ["1", "2"])
@pytest.mark.parametrize("group", sorted(GROUPS))
def test_limit_edges_route_by_the_kernels_own_counts(product, monkeypatch, tmp_path, group, waves):
    """The dump of every fill kernel that ran the gap: a row that stays has the model's entries, segments and rounds
    and no flag; a row over a limit carries that limit's overflow and reason bits and no other, and appears once more
    in the next tier's dump; a row that leaves the large variant too is finished by the HBM tier."""
    names, seqs, gaps, idx = _group(group, monkeypatch)
    recs, tm, res = _seg_dump_rounds(product, monkeypatch, tmp_path, seqs, gaps, waves)
    assert tm.watchdog_gaps == 0
    in_large = left = 0
    for i, name in zip(idx, names):
        w = cases.LIMIT_EDGES[name][2]
        got = recs.get(i)
        assert got, "%s: no record in the dump" % name
        print(name, waves, got)
        want = [_regular_tier(w)]
        if want[0]:
            want.append(_large_variant(w))
        assert len(got) == len(want), (name, got)
        for (nA, nseg, flags, gen), reasons in zip(got, want):
            assert flags & REASONS == reasons, (name, got)
            if not reasons:
                assert (nA, nseg, gen) == (w["nA"], w["nseg"], w["gen"]), (name, got)
            elif reasons & OVF_B:  # (phase A went through: its count is the model's)
                assert nA == w["nA"], (name, got)
        in_large += len(want) == 2 and not want[1]
        left += len(want) == 2 and want[1] != 0
        assert res[i].phaseC_count == w.get("count", cases.MAX_PATHS), name
    assert tm.segx_tier_gaps == in_large and tm.seg_tier_gaps == len(gaps) - in_large - left
    assert tm.lds_tier_gaps == 0
    if left:
        assert tm.launches_left_dp >= 1


ROUTES = ["default", "segx", "res", "nosegx"]


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("group", sorted(GROUPS))
def test_limit_edges_equal_the_oracle_on_every_route(product, oracle, monkeypatch, group, route):
    """Every row, field by field (count, fill text and case, fuz, draws, subgraph statistics), on the default route,
    with every gap in the large variant (G2S_FORCE_SEGX=1), in resident mode, and without the large variant
    (G2S_NO_SEGX_TIER=1: what the regular tier cannot hold goes straight to the HBM tier)."""
    names, seqs, gaps, idx = _group(group, monkeypatch)
    monkeypatch.setenv("G2S_RESIDENT", "1" if route == "res" else "0")
    if route == "segx":
        monkeypatch.setenv("G2S_FORCE_SEGX", "1")
    elif route == "nosegx":
        monkeypatch.setenv("G2S_NO_SEGX_TIER", "1")
    c, f, tm, _, _ = _check_batch(product, oracle, seqs, K, gaps, E)
    assert c == len(gaps) and tm.watchdog_gaps == 0 and tm.lds_tier_gaps == 0
    wants = [cases.LIMIT_EDGES[n][2] for n in names]
    if route == "segx":
        left = sum(_large_variant(w) != 0 for w in wants)
        assert (tm.seg_tier_gaps, tm.segx_tier_gaps) == (0, len(gaps) - left)
    elif route == "nosegx":
        left = sum(_regular_tier(w) != 0 for w in wants)
        assert (tm.seg_tier_gaps, tm.segx_tier_gaps) == (len(gaps) - left, 0)
    else:
        left = sum(_regular_tier(w) != 0 and _large_variant(w) != 0 for w in wants)
        assert tm.seg_tier_gaps + tm.segx_tier_gaps == len(gaps) - left
    if left and route != "res":
        assert tm.launches_left_dp >= 1
    if route == "res":  # (resident mode has no HBM tier: a list with a gap that leaves both kernels runs again on the host path)
        assert (tm.resident_launches, tm.resident_fallbacks) == ((0, 1) if left else (1, 0))


def test_limit_edges_inside_a_long_resident_list(product, oracle, monkeypatch):
    """The frontier rows and the search-level rows spread over a list of 300 ordinary gaps on one graph, in resident
    mode: finished on the device without falling back, and equal to the oracle.  (On a shared graph the unitigs are
    numbered differently: the search-level rows keep their entries and segments, not their exact M.  ring1025 leaves
    both segment kernels and resident mode has no HBM tier: it is in test_limit_edges_equal_the_oracle_on_every_route's
    resident list, which falls back, and not in this one.)"""
    for v in PATH_VARS:
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv("G2S_RESIDENT", "1")
    names = [n for n in FRONTIER + sorted(n for n in cases.SEGW_EDGES if n.startswith("iv"))
             if not (_regular_tier(cases.LIMIT_EDGES[n][2]) and _large_variant(cases.LIMIT_EDGES[n][2]))]
    assert len(names) == len(FRONTIER) - 1 + 8
    seqs, gaps, idx = cases.limit_edge_list(names, pad=300)
    assert len(gaps) == 300 + len(names)
    c, f, tm, _, _ = _check_batch(product, oracle, seqs, K, gaps, E)
    assert c == len(gaps) and tm.watchdog_gaps == 0 and tm.lds_tier_gaps == 0
    assert (tm.resident_launches, tm.resident_fallbacks) == (1, 0)
    assert tm.seg_tier_gaps + tm.segx_tier_gaps == len(gaps)
