"""GPU tests of the SUMS in g2s_timing (run with `-m gpu` on an MI355X): a list that is cut — into the groups of a
team, the groups of g2s_fill_sets, the shares of ranks — reports, for every figure that is additive per gap, what one
session reports that fills the same list in one g2s_fill_batch call on the same path family (host path against
G2S_RESIDENT=0, resident mode against resident mode).  The one-session call runs none of the sums (g2s_api.hip:
timing_add and its callers); how a list is cut cannot change a per-gap total.

The list is short on purpose: inside a team's list resident mode takes groups of any length, and 96 gaps in groups of
32 are three groups and two barriers, in groups of 40 a ragged last group.

(case, field) pairs that did NOT equal the one-session figure when these tests were first run, against the sums as
they were before timing_add (96 gaps; every other pair of every case below, and of the sliced list in
test_gpu_resident.py::test_long_lists_go_slice_by_slice, was equal then and is asserted equal):

  case                     field         measured then                          asserted
  -----------------------  ------------  -------------------------------------  ------------------------------------------
  fill_sets, host path     seg_segments  0 against 1158: g2s_fill_sets' own     the one-session figure: timing_add adds
  fill_sets, resident                    sum did not add the field              every additive field
  fill_sets, host path     fill_bytes    49341 against 49338, and equal to the  the sum of fill_len over the call's own
  fill_sets, resident                    sum of fill_len over its results       results — by design: every gap of a set
                                                                                list draws from a fresh stream, the gaps of
                                                                                one g2s_fill_batch call share one, so the
                                                                                two calls need not trace the same paths

Nothing here looks at ms_* fields or at guessed_groups_resent: they depend on timing."""
import ctypes as C
import threading

import pytest

from test_gpu_parity import _gaps, _parse_scaffolds
from test_gpu_resident import _ThreadComm, _key

pytestmark = pytest.mark.gpu

COUNTERS = ("xA", "sA", "xB", "sB", "xD", "sD", "flank_bytes", "fill_bytes", "seg_segments", "draw_dependent_gaps",
            "host_finished_gaps")


def checked_fields(t):
    """The figures of a g2s_timing that are additive per gap (the three tiers' gap counts as one figure: which tier
    takes a gap is the path's business, that exactly one takes it is not)."""
    d = {f: int(getattr(t, f)) for f in COUNTERS}
    d["tier_gaps"] = int(t.seg_tier_gaps) + int(t.segx_tier_gaps) + int(t.lds_tier_gaps)
    return d


def _sum(ds):
    return {f: sum(d[f] for d in ds) for f in ds[0]}


def _compare(case, got, want, instead=None):
    """Every checked figure of `got` against `want`; `instead`: the figures of the table above, by field."""
    print("%s: got %r\n%s: one session %r" % (case, got, case, want))
    expect = dict(want)
    expect.update(instead or {})
    assert got == expect, {f: (got[f], expect[f]) for f in got if got[f] != expect[f]}


@pytest.fixture(scope="module")
def work(product):
    """The list, and one session's results and figures on it: host path, resident mode, and (a graph of one read set)
    the same two for the set list.  Computed once, read by every case."""
    reads = product.G2S.synth_genome(60000, 3, 20240101)
    seqs = [ln for ln in reads.splitlines() if not ln.startswith(">")]
    gaps = _gaps(product, _parse_scaffolds(product.G2S.synth_gaps(reads, 31, 10, 96, 100, 900, 20240103)))
    assert len(gaps) == 96
    w = dict(product=product, gaps=gaps, graph=product.Graph.from_seqs(seqs, 31, 1), sets=product.Graph.from_sets([seqs], 31, 1))
    with pytest.MonkeyPatch.context() as m:
        for which, graph in (("list", w["graph"]), ("sets", w["sets"])):
            for resident in ("0", "1"):
                m.setenv("G2S_RESIDENT", resident)
                s = product.Session(graph, 0, d_err=500, randseed=9)
                res, tm = s.fill_batch_onecall(gaps, want_timing=True)
                s.destroy()
                assert tm.team_groups == 0 and tm.resident_launches == int(resident) and tm.resident_fallbacks == 0
                w[which, resident] = ([_key(r) for r in res], checked_fields(tm))
    assert w["list", "0"][0] == w["list", "1"][0] and w["sets", "0"][0] == w["sets", "1"][0]
    yield w
    w["graph"].free()
    w["sets"].free()


def _team(work, monkeypatch, resident, group, pinned):
    product, gaps = work["product"], work["gaps"]
    monkeypatch.setenv("G2S_RESIDENT", resident)
    team = [product.Session(work["graph"], 0, d_err=500, randseed=9) for _ in range(3)]
    try:
        got, tm = product.team_fill(team, gaps, group_size=group, want_timing=True, pinned=pinned)
    finally:
        for s in team:
            s.destroy()
    assert [_key(r) for r in got] == work["list", resident][0]
    assert tm.team_groups == 3 and tm.team_sessions == 3
    return tm


@pytest.mark.parametrize("group", [32, 40])
def test_team_on_the_host_path_sums_its_groups(work, monkeypatch, group):
    tm = _team(work, monkeypatch, "0", group, False)
    assert tm.resident_launches == 0
    _compare("team, host path, groups of %d" % group, checked_fields(tm), work["list", "0"][1])


@pytest.mark.parametrize("group", [32, 40])
def test_team_gathered_on_the_lead_sums_its_groups(work, monkeypatch, group):
    tm = _team(work, monkeypatch, "1", group, False)
    assert tm.resident_launches == 1 and tm.resident_fallbacks == 0 and tm.team_d3_sharded == 0
    _compare("team, gathered, groups of %d" % group, checked_fields(tm), work["list", "1"][1])


def test_team_with_phase_d3_sharded_sums_its_groups(work, monkeypatch):
    tm = _team(work, monkeypatch, "1", 32, True)
    assert tm.resident_launches == 1 and tm.resident_fallbacks == 0 and tm.team_d3_sharded == 1
    _compare("team, sharded", checked_fields(tm), work["list", "1"][1])


@pytest.mark.parametrize("resident", ["0", "1"])
def test_fill_sets_sums_its_groups(work, monkeypatch, resident):
    """A session without helpers whose group size is 48 (g2s_session_set_team with no helpers: team_group_for returns
    the size it was given): g2s_fill_sets cuts the 96 gaps into two groups."""
    product, gaps = work["product"], work["gaps"]
    monkeypatch.setenv("G2S_RESIDENT", resident)
    want_res, want = work["sets", resident]
    s = product.Session(work["sets"], 0, d_err=500, randseed=9)
    try:
        whole, tw = s.fill_sets(gaps, [0] * len(gaps), want_timing=True)
        s.set_team([], 48)
        got, tm = s.fill_sets(gaps, [0] * len(gaps), want_timing=True)
    finally:
        s.destroy()
    assert [_key(r) for r in got] == [_key(r) for r in whole]  # (groups change nothing: every gap is on its own)
    assert tw.resident_launches == int(resident) and tm.resident_launches == 2 * int(resident) and tm.resident_fallbacks == 0
    # (the same searches as the one session's, whatever the gaps then draw)
    assert [k[0] for k in want_res] == [r.count for r in got]
    _compare("fill_sets, resident %s" % resident, checked_fields(tm), want, {"fill_bytes": sum(r.fill_len for r in got)})


def test_shares_on_ranks_of_their_own_sum_to_the_list(work, monkeypatch):
    from gap2seq_amd import shard
    product, gaps, world = work["product"], work["gaps"], 3
    monkeypatch.setenv("G2S_RESIDENT", "1")
    lib = product.load_library()
    sessions = [product.Session(work["graph"], 0, d_err=500, randseed=9) for _ in range(world)]
    table, barrier = [None] * world, threading.Barrier(world)
    out, errs = [None] * world, []

    def rank_main(r):
        try:
            comm = _ThreadComm(r, world, table, barrier)
            lo, hi = shard.share_bounds(len(gaps), world)[r]
            arr, keep = product._gap_array(gaps[lo:hi])
            n = hi - lo
            nbytes = lib.g2s_team_arena_bytes(sessions[r].h, arr, n)
            abuf, rbuf = product.HostBuffer(max(1, nbytes)), product.HostBuffer(C.sizeof(product.g2s_result) * n)
            res = rbuf.array(product.g2s_result, n)
            draws = shard.fill_share(product, sessions[r], comm, arr, n, res, C.cast(abuf.p, C.c_void_p), nbytes)
            assert draws is not None and draws > 0
            raw = abuf.raw
            out[r] = ([_key(product.FillResult(res[i], raw)) for i in range(n)], checked_fields(sessions[r].last_timing()))
            abuf.free(); rbuf.free()
        except BaseException as e:  # noqa: B902 (a failing rank must not leave the others at the barrier)
            errs.append((r, repr(e)))
            barrier.abort()

    th = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for s in sessions:
        s.destroy()
    assert not errs, errs
    assert sum((o[0] for o in out), []) == work["list", "1"][0]
    _compare("shares", _sum([o[1] for o in out]), work["list", "1"][1])
