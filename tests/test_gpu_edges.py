"""The fill kernels at their per-gap capacities (run with `-m gpu` on an MI355X).  The planted gaps of
cases.EDGE_LADDERS sit one below, on and one above every limit at which a gap changes branch, tier or packing:
the 64-lane chunks of the segment log, the 192 segments up to which the fill kernel analyses the closure itself,
G2S_SEG_CAP = 512 logged segments, 64 * G2S_SEG_ASETS = 256 right-set entries, g2s_d2_small's 256 closure segments,
the path count's saturation at MAX_PATHS = 2^30 - 2; beside them D = lmf + rmf + gap + d_err at 32766 / 32767 /
32768 (16-bit depths) and fuz 31 / 32 (32 seeds and targets).  tests/test_seg_model.py proves on the host that each
gap is where the table says.  Every case asserts where the gap went, from the library's own records (G2S_SEG_DUMP,
G2S_D2_LOG, g2s_timing), and that what it computed is the oracle's, field by field."""
import os

import pytest

import cases
from d2_witness import _d2_log
from test_gpu_parity import _check_batch, _gaps

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
K = 31
E = 10
NAMES = sorted(cases.EDGE_LADDERS)
OVF_A, OVF_B, WHY_LOG, WHY_RS = 0x4, 0x8, 0x400, 0x800


def _want(name):
    return cases.EDGE_LADDERS[name][1]


def _seg_dump(product, monkeypatch, tmp_path, seqs, gaps, waves, e=E):
    """One list on the host path with G2S_SEG_DUMP set: {gap index: [(nA, nseg, flags) per fill kernel that ran
    the gap, in launch order]}, timing."""
    path = tmp_path / ("dump_%s.txt" % waves)
    monkeypatch.setenv("G2S_SEG_DUMP", str(path))
    monkeypatch.setenv("G2S_SEG_DUMP_BRIEF", "1")
    monkeypatch.setenv("G2S_SEG_WAVES", waves)
    monkeypatch.setenv("G2S_RESIDENT", "0")
    pg = product.Graph.from_seqs(seqs, K, 1)
    sess = product.Session(pg, 0, d_err=e, randseed=5)
    try:
        res, tm = sess.fill_batch(_gaps(product, gaps), True)
    finally:
        sess.destroy()
        pg.free()
        for v in ("G2S_SEG_DUMP", "G2S_SEG_DUMP_BRIEF", "G2S_SEG_WAVES", "G2S_RESIDENT"):
            monkeypatch.delenv(v)
    recs = {}
    for line in open(path):
        w = line.split()
        if w[0] == "gap":
            recs.setdefault(int(w[1]), []).append((int(w[3]), int(w[5]), int(w[7], 16)))
    return recs, tm, res


@pytest.mark.parametrize("waves", ["1", "2"])
def test_edge_ladders_route_by_the_kernels_own_counts(product, monkeypatch, tmp_path, waves):
    """The segment tier's dump: every planted gap has the model's right-set entries and logged segments; at 513
    segments and at 257 entries (only there) the tier gives up with the overflow flag and the reason, and the large
    variant takes the gap with the same counts."""
    seqs, gaps, idx = cases.edge_ladder_list(NAMES, pad=100)
    recs, tm, res = _seg_dump(product, monkeypatch, tmp_path, seqs, gaps, waves)
    assert tm.watchdog_gaps == 0
    big = []
    for i, name in zip(idx, NAMES):
        w = _want(name)
        got = recs.get(i)
        assert got, "%s: no record in the dump" % name
        nA, nseg, flags = got[0]
        if w["nseg"] > 512:
            assert flags & (OVF_B | WHY_LOG) == OVF_B | WHY_LOG and not flags & OVF_A, (name, got)
            assert nA == w["nA"] and nseg <= 512, (name, got)
        elif w["nA"] > 256:
            assert flags & (OVF_A | WHY_RS) == OVF_A | WHY_RS and not flags & OVF_B, (name, got)
        else:
            assert (nA, nseg) == (w["nA"], w["nseg"]) and not flags & (OVF_A | OVF_B), (name, got)
            assert len(got) == 1, (name, got)
            continue
        big.append(name)
        assert len(got) == 2, (name, got)
        assert got[1][:2] == (w["nA"], w["nseg"]) and not got[1][2] & (OVF_A | OVF_B), (name, got)
    assert sorted(big) == ["rs257", "seg513"]
    assert tm.segx_tier_gaps == 2 and tm.seg_tier_gaps == len(gaps) - 2
    assert tm.lds_tier_gaps == 0 and tm.retried_gaps == 0
    for i, name in zip(idx, NAMES):
        assert res[i].phaseC_count == _want(name).get("count", cases.MAX_PATHS), name


@pytest.fixture(params=["seg", "seg1", "res", "segx", "hbm"])
def edge_tier(request, monkeypatch):
    """The kernel tiers of test_gpu_parity's `tier`, and the segment tier on one wave per gap ("seg1": the
    kernel with the pairwise cross-check of 65 to 192 segments)."""
    for v in ("G2S_NO_SEG_TIER", "G2S_FORCE_SEGX", "G2S_SEG_WAVES"):
        monkeypatch.delenv(v, raising=False)
    p = request.param
    monkeypatch.setenv("G2S_RESIDENT", "1" if p == "res" else "0")
    if p == "seg1":
        monkeypatch.setenv("G2S_SEG_WAVES", "1")
    elif p == "segx":
        monkeypatch.setenv("G2S_FORCE_SEGX", "1")
    elif p == "hbm":
        monkeypatch.setenv("G2S_NO_SEG_TIER", "1")
    return p


def _tier_counts(tier, tm, n):
    if tier in ("seg", "seg1", "res"):
        assert tm.seg_tier_gaps + tm.segx_tier_gaps == n and tm.segx_tier_gaps == 2, (tm.seg_tier_gaps, tm.segx_tier_gaps)
    elif tier == "segx":
        assert tm.segx_tier_gaps == n
    else:
        assert tm.seg_tier_gaps == 0 and tm.segx_tier_gaps == 0 and tm.lds_tier_gaps == 0
        assert tm.launches_left_dp >= 1
    if tier == "res":
        assert tm.resident_launches == 1 and tm.resident_fallbacks == 0


def test_edge_ladders_equal_the_oracle_on_every_tier(product, oracle, edge_tier):
    """Every planted gap, in one list, on every tier: count (exact below 2^30 - 2, saturated from 2^30 on), fill
    text and case, fuz, draws and subgraph statistics are the oracle's."""
    seqs, gaps, idx = cases.edge_ladder_list(NAMES, pad=100)
    c, f, tm, _, _ = _check_batch(product, oracle, seqs, K, gaps, E)
    assert c == len(gaps)
    _tier_counts(edge_tier, tm, len(gaps))


def test_segment_tier_overflows_are_finished_by_the_hbm_tier(product, oracle, monkeypatch):
    """Without the large variant the two planted overflows (seg513, rs257) leave the segment tier with their flags
    and go straight to the HBM tier, at odd k as at even k: every gap of the list equals the oracle."""
    for v in ("G2S_NO_SEG_TIER", "G2S_FORCE_SEGX", "G2S_SEG_WAVES"):
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv("G2S_RESIDENT", "0")
    monkeypatch.setenv("G2S_NO_SEGX_TIER", "1")
    seqs, gaps, idx = cases.edge_ladder_list(NAMES, pad=100)
    c, f, tm, _, _ = _check_batch(product, oracle, seqs, K, gaps, E)
    assert tm.seg_tier_gaps == len(gaps) - 2
    assert tm.segx_tier_gaps == 0 and tm.lds_tier_gaps == 0
    assert tm.launches_left_dp >= 1
    assert tm.watchdog_gaps == 0
    assert c == len(gaps)


COUNT_LADDERS = ["paths2^29", "paths2^30", "paths2^31", "seg64", "seg65"]


@pytest.mark.parametrize("skip,allp", [(False, False), (True, True)])
def test_count_ladders_best_only_and_skip_rule(product, oracle, edge_tier, skip, allp):
    """The count ladders with -best-only and with the skip rule (where the resident path's closure cap moves to
    512): the counts are exact, every other field is the oracle's."""
    seqs, gaps, _ = cases.edge_ladder_list(COUNT_LADDERS + ["seg192", "seg193", "seg512"], pad=40)
    c, f, tm, _, _ = _check_batch(product, oracle, seqs, K, gaps, E, skip, allp)
    assert c == len(gaps)
    if edge_tier == "res":
        assert tm.resident_launches == 1 and tm.resident_fallbacks == 0


D2_LADDERS = ["seg191", "seg192", "seg193", "cl255", "cl256", "cl257", "indel20"]


def test_d2_instantiation_by_closure_size(product, tmp_path):
    """Up to 192 logged segments the fill kernel analyses the closure itself and no D2 kernel sees it; from 193 on
    (and a closure with a k-mer at several depths) g2s_d2_small takes it up to 256 closure segments on paths to a
    sink and passes 257 on, to g2s_d2_big, or to the host with G2S_D2_BIG=0."""
    for big in ("1", "0"):
        by = _d2_log(tmp_path, D2_LADDERS, G2S_D2_BIG=big)
        assert by["seg191"] == [] and by["seg192"] == [], big
        for name in ("seg193", "cl255", "cl256", "indel20"):
            assert [(x["kernel"], x["rc"]) for x in by[name]] == [(0, 0)], (big, name, by[name])
        want = [(0, True), (1, False)] if big == "1" else [(0, True)]
        assert [(x["kernel"], x["rc"] != 0) for x in by["cl257"]] == want, (big, by["cl257"])


@pytest.mark.parametrize("how", ["device", "big"])
def test_d2_on_the_device_equals_the_oracle(product, oracle, monkeypatch, how):
    monkeypatch.setenv("G2S_DEVICE_D2", "1")
    monkeypatch.setenv("G2S_RESIDENT", "1")
    if how == "big":
        monkeypatch.setenv("G2S_D2_BIG", "2")
    seqs, gaps, _ = cases.edge_ladder_list(D2_LADDERS + ["seg512", "seg513", "rs257"], pad=100)
    c, f, tm, _, _ = _check_batch(product, oracle, seqs, K, gaps, E)
    assert c == len(gaps) and tm.resident_launches == 1 and tm.resident_fallbacks == 0


def test_edge_gaps_inside_a_long_resident_list(product, oracle, monkeypatch):
    """The planted gaps spread over a list of 300 ordinary gaps: the list is finished on the device (resident
    mode, g2s_d3_*) without falling back, and equals the oracle; the same list on the host path too.  (With gaps
    deeper than 2 500 levels the list counts as deep, and a resident launch starts its longest gaps in the large
    variant at once; without that early launch exactly the two planted overflows take it.)"""
    seqs, gaps, _ = cases.edge_ladder_list(NAMES, pad=300)
    assert len(gaps) == 300 + len(NAMES)
    for resident, early in (("1", True), ("1", False), ("0", True)):
        monkeypatch.setenv("G2S_RESIDENT", resident)
        if not early:
            monkeypatch.setenv("G2S_NO_EARLY_SEGW", "1")
        c, f, tm, _, _ = _check_batch(product, oracle, seqs, K, gaps, E)
        monkeypatch.delenv("G2S_NO_EARLY_SEGW", raising=False)
        assert c == len(gaps) and tm.watchdog_gaps == 0
        if resident == "1":
            assert tm.resident_launches == 1 and tm.resident_fallbacks == 0
        assert tm.seg_tier_gaps + tm.segx_tier_gaps == len(gaps) and tm.lds_tier_gaps == 0, (resident, early)
        if early:
            assert tm.segx_tier_gaps >= 2, (resident, tm.segx_tier_gaps)
        if not early or resident == "0":
            assert tm.segx_tier_gaps == 2, (resident, early, tm.segx_tier_gaps)


def _deep_ladder():
    """8 paths of 32 750 steps: the gap record's claimed length g sets D = lmf + rmf + g + d_err."""
    lad = cases.bubble_ladder(201, K, 3, 32, lead=16000, tail=16654)
    assert lad["gap"]["true_len"] + K == 32750
    return lad


@pytest.mark.parametrize("tier", ["default", "segx", "hbm"])
def test_depth_limit_of_the_segment_tiers(product, oracle, monkeypatch, tier):
    """D = 32766 is the deepest gap the segment tiers take (16-bit depths, 0x7FFF / 0x8000 reserved); 32767 and
    32768 go to the HBM tier.  Equal to the oracle on every path."""
    monkeypatch.setenv("G2S_RESIDENT", "0")
    if tier == "segx":
        monkeypatch.setenv("G2S_FORCE_SEGX", "1")
    elif tier == "hbm":
        monkeypatch.setenv("G2S_NO_SEG_TIER", "1")
    lad = _deep_ladder()
    gaps = []
    for D in (32766, 32767, 32768):
        g = dict(lad["gap"])
        g["gap_len"] = D - g["lmf"] - g["rmf"] - E
        gaps.append(g)
    modes = ((False, True), (False, False), (True, True)) if tier == "default" else ((False, True),)
    for skip, allp in modes:
        c, f, tm, _, _ = _check_batch(product, oracle, lad["seqs"], K, gaps, E, skip, allp)
        assert c == f == 3 and tm.watchdog_gaps == 0
        if tier == "default":
            assert (tm.seg_tier_gaps, tm.segx_tier_gaps, tm.lds_tier_gaps) == (1, 0, 0)
        elif tier == "segx":
            assert (tm.seg_tier_gaps, tm.segx_tier_gaps, tm.lds_tier_gaps) == (0, 1, 0)
        else:
            assert (tm.seg_tier_gaps, tm.segx_tier_gaps, tm.lds_tier_gaps) == (0, 0, 0)
        assert tm.launches_left_dp >= 1


@pytest.mark.parametrize("tier", ["default", "segx", "hbm"])
def test_fuz_31_and_32(product, oracle, monkeypatch, tier):
    """lmf, rmf = 31 is the last fuz the segment tiers hold (32 seeds, 32 targets in lanes); lmf = 32 or rmf = 32 goes
    to the HBM tier."""
    monkeypatch.setenv("G2S_RESIDENT", "0")
    if tier == "segx":
        monkeypatch.setenv("G2S_FORCE_SEGX", "1")
    elif tier == "hbm":
        monkeypatch.setenv("G2S_NO_SEG_TIER", "1")
    lad = cases.bubble_ladder(202, K, 5, 32, lead=100, tail=100, fuz=32)
    g0 = lad["gap"]
    gaps = []
    for lmf, rmf in ((31, 31), (32, 31), (31, 32), (32, 32)):
        gaps.append(dict(left=g0["left"][32 - lmf:], right=g0["right"][:K + rmf], gap_len=g0["gap_len"], lmf=lmf, rmf=rmf))
    for skip, allp in ((False, True), (False, False), (True, True)):
        c, f, tm, _, _ = _check_batch(product, oracle, lad["seqs"], K, gaps, E, skip, allp)
        assert c == f == 4 and tm.watchdog_gaps == 0
        if tier == "default":
            assert (tm.seg_tier_gaps, tm.segx_tier_gaps, tm.lds_tier_gaps, tm.retried_gaps) == (1, 0, 0, 0)
        elif tier == "segx":
            assert (tm.seg_tier_gaps, tm.segx_tier_gaps, tm.lds_tier_gaps) == (0, 1, 0)
        else:
            assert (tm.seg_tier_gaps, tm.segx_tier_gaps, tm.lds_tier_gaps) == (0, 0, 0)
        assert tm.launches_left_dp >= 1
