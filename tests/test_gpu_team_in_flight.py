"""GPU tests of LISTS IN FLIGHT OVER A TEAM (run with `-m gpu` on an MI355X): a lead session with helpers
(g2s_session_set_team, G2S_GROUP_PER_SESSION) and g2s_fill_begin / g2s_fill_end.  A list long enough for one share per
session, in page-locked buffers, no record cut by a share boundary, has step 1 of every share — look-ups, fill kernel,
classes, totals — queued on the share's device at g2s_fill_begin, on the member's session or on a twin of it;
g2s_fill_end waits for the totals and runs the tables and the tracebacks, which overlap step 1 of the lists begun
behind.  Everything else a team is given waits for g2s_fill_end as before.  The results are those of ONE session filling
the same lists one after the other, whatever the depth, the team's size and the switch G2S_TEAM_IN_FLIGHT.  (The
sessions of a team share device 0 here: the logic is the one of N GPUs, the timing is not.)"""
import ctypes as C
import itertools

import pytest

from test_gpu_parity import _gaps, _parse_scaffolds
from test_gpu_resident import _key

pytestmark = pytest.mark.gpu

K = 31
D_ERR = 500
_nonce = itertools.count(1)


def _genome(product, ngaps):
    """the branching genome of the team tests, its sequences, and `ngaps` gaps over it as parsed records"""
    reads = product.G2S.synth_genome(200000, 3, 20240101)
    seqs = [ln for ln in reads.splitlines() if not ln.startswith(">")]
    text = product.G2S.synth_gaps(reads, K, 10, ngaps, 100, 900, 20240103)
    return seqs, _parse_scaffolds(text), text


def _solo(product, pg, lists, seed):
    """what one plain session gives for the lists, one after the other (and leaves the session open: the stream goes on)"""
    s = product.Session(pg, 0, d_err=D_ERR, randseed=seed)
    want = [[_key(r) for r in s.fill_batch_onecall(L, pinned=True)] if L else [] for L in lists]
    return s, want


class _Bufs:
    """a list's gap array, results and fill arena: page-locked (g2s_host_alloc) or pageable"""

    def __init__(self, product, sess, gaps, pinned):
        lib = product.load_library()
        self.product, self.n, self.pinned = product, len(gaps), pinned
        self.arr, self.keep = product._gap_array(gaps)
        self.nbytes = lib.g2s_team_arena_bytes(sess.h, self.arr, self.n)
        if pinned:
            self.arena = product.HostBuffer(max(1, self.nbytes))
            self.rbuf = product.HostBuffer(C.sizeof(product.g2s_result) * max(1, self.n))
            self.res = self.rbuf.array(product.g2s_result, max(1, self.n))
            self.ap = C.cast(self.arena.p, C.c_void_p)
        else:
            self.arena = C.create_string_buffer(max(1, self.nbytes))
            self.rbuf = None
            self.res = (product.g2s_result * max(1, self.n))()
            self.ap = C.cast(self.arena, C.c_void_p)

    def begin(self, sess):
        return self.product.load_library().g2s_fill_begin(sess.h, self.arr, self.n, self.res, self.ap, self.nbytes)

    def keys(self):
        raw = self.arena.raw
        return [_key(self.product.FillResult(self.res[i], raw)) for i in range(self.n)]

    def free(self):
        if self.rbuf is not None:
            self.rbuf.free()
            self.arena.free()
            self.rbuf = None


def _drain(product, lead):
    lib = product.load_library()
    while lib.g2s_fill_in_flight(lead.h) > 0:
        lib.g2s_fill_end(lead.h)


def _stream(product, lead, spec, depth):
    """The lists of `spec` ((gaps, pinned) pairs) through g2s_fill_begin / g2s_fill_end on `lead`, `depth` in flight:
    begin until the depth is reached, then end one, begin one.  Returns, per list: its results' keys, the timing behind
    its g2s_fill_end, and (lists in flight, lists launched) behind its g2s_fill_begin."""
    lib = product.load_library()
    bufs = [_Bufs(product, lead, gaps, pinned) for gaps, pinned in spec]
    timings, counts = [], []
    try:
        for i, b in enumerate(bufs):
            if lib.g2s_fill_in_flight(lead.h) == depth:
                product._check(lib.g2s_fill_end(lead.h))
                timings.append(lead.last_timing())
            product._check(b.begin(lead))
            counts.append((lib.g2s_fill_in_flight(lead.h), lib.g2s_fill_in_flight_launched(lead.h)))
        while lib.g2s_fill_in_flight(lead.h) > 0:
            product._check(lib.g2s_fill_end(lead.h))
            timings.append(lead.last_timing())
        return [b.keys() for b in bufs], timings, counts
    finally:
        _drain(product, lead)  # (an error between begin and end: the lists still write into these buffers)
        for b in bufs:
            b.free()


def _team(product, pg, nsess, seed):
    team = [product.Session(pg, 0, d_err=D_ERR, randseed=seed) for _ in range(nsess)]
    team[0].set_team(team[1:], product.G2S_GROUP_PER_SESSION)
    return team


def _destroy(sessions):
    for s in sessions:
        s.destroy()


@pytest.mark.parametrize("nsess,depth", [(2, 2), (2, 3), (3, 2), (3, 3)])
def test_team_lists_in_flight_equal_list_by_list(product, monkeypatch, nsess, depth):
    """Five lists — two long page-locked ones (step 1 queued at g2s_fill_begin), a 300-gap one (the lead alone), a long
    one in pageable buffers (the gathered form: it waits for g2s_fill_end) and an empty one — with two and with three in
    flight, over teams of two and three sessions: every list as one session gives it, and the lead's stream behind
    them where the one session's stands."""
    monkeypatch.delenv("G2S_RESIDENT", raising=False)
    monkeypatch.delenv("G2S_TEAM_IN_FLIGHT", raising=False)
    seqs, gl, _ = _genome(product, 4200)
    allg = _gaps(product, gl)
    lists = [allg[:2100], allg[2100:4200], allg[:300], allg[1000:3100], []]
    pinned = [True, True, True, False, True]
    pg = product.Graph.from_seqs(seqs, K, 1)
    team = []
    try:
        solo, want = _solo(product, pg, lists, 13)
        tail = [_key(r) for r in solo.fill_batch_onecall(allg[300:700], pinned=True)]
        solo.destroy()
        team = _team(product, pg, nsess, 13)
        got, timings, counts = _stream(product, team[0], list(zip(lists, pinned)), depth)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == w, "list %d" % i
        assert [_key(r) for r in team[0].fill_batch_onecall(allg[300:700], pinned=True)] == tail
        # the two long page-locked lists ended sharded on the sessions their step 1 ran on; the pageable one gathered
        for i in (0, 1):
            assert timings[i].team_d3_sharded == 1 and timings[i].team_groups == nsess and timings[i].resident_fallbacks == 0
        assert timings[3].team_d3_sharded == 0 and timings[3].team_groups == nsess
        assert counts[0] == (1, 1) and counts[1] == (2, 2)
        assert all(inflight <= depth for inflight, _ in counts)
    finally:
        _destroy(team)
        pg.free()


def test_the_fill_is_queued_at_begin(product, monkeypatch):
    """g2s_fill_in_flight_launched: a long page-locked list begun on a team of two has its fill kernels queued on both
    shares before g2s_fill_begin returns, a second one too; with G2S_TEAM_IN_FLIGHT=0 none is, and the results are the
    same; either way the lists end sharded over the team.  On a session without a team the call counts the lists whose
    fill kernel g2s_fill_begin launched."""
    monkeypatch.delenv("G2S_RESIDENT", raising=False)
    monkeypatch.delenv("G2S_TEAM_IN_FLIGHT", raising=False)
    seqs, gl, _ = _genome(product, 4200)
    allg = _gaps(product, gl)
    lists = [allg[:2100], allg[2100:4200]]
    pg = product.Graph.from_seqs(seqs, K, 1)
    team = []
    try:
        solo, want = _solo(product, pg, lists, 17)
        solo.destroy()
        for switch, launched in ((None, [(1, 1), (2, 2)]), ("0", [(1, 0), (2, 0)]), ("1", [(1, 1), (2, 2)])):
            if switch is None:
                monkeypatch.delenv("G2S_TEAM_IN_FLIGHT", raising=False)
            else:
                monkeypatch.setenv("G2S_TEAM_IN_FLIGHT", switch)
            team = _team(product, pg, 2, 17)
            got, timings, counts = _stream(product, team[0], [(L, True) for L in lists], 3)
            assert counts == launched, switch
            assert got == want, switch
            for tm in timings:
                assert tm.team_d3_sharded == 1 and tm.team_groups == 2 and tm.team_sessions == 2, switch
                assert tm.resident_fallbacks == 0 and tm.resident_launches == 1, switch
            assert team[0].in_flight() == 0 and team[0].in_flight_launched() == 0
            _destroy(team)
            team = []
        monkeypatch.delenv("G2S_TEAM_IN_FLIGHT", raising=False)
        # one session, no team: its pre-launched lists (a 100-gap list is not one for the device: begun, not launched)
        one = product.Session(pg, 0, d_err=D_ERR, randseed=17)
        team = [one]
        got, _, counts = _stream(product, one, [(lists[0], True), (allg[:100], True), (lists[1][:900], True)], 3)
        assert counts == [(1, 1), (2, 1), (3, 2)]
        assert got[0] == want[0]
    finally:
        _destroy(team)
        pg.free()


def test_a_record_cut_by_a_share_boundary_waits_for_its_end(product, monkeypatch):
    """A long list whose gap at the share boundary carries a skip rule (the record goes on across the boundary) is not
    one for the sharded form: it is begun, not launched, between two lists that are — and all three are the one
    session's."""
    monkeypatch.delenv("G2S_RESIDENT", raising=False)
    monkeypatch.delenv("G2S_TEAM_IN_FLIGHT", raising=False)
    seqs, gl, _ = _genome(product, 4200)
    allg = _gaps(product, gl)
    cut = _gaps(product, gl[1000:3100])  # (objects of its own: the rule is this list's)
    cut[1050].skip_dep = 5               # (2 100 gaps over two sessions: the second share begins at gap 1 050)
    lists = [allg[:2100], cut, allg[2100:4200]]
    pg = product.Graph.from_seqs(seqs, K, 1)
    team = []
    try:
        solo, want = _solo(product, pg, lists, 19)
        solo.destroy()
        team = _team(product, pg, 2, 19)
        got, timings, counts = _stream(product, team[0], [(L, True) for L in lists], 3)
        assert counts == [(1, 1), (2, 1), (3, 2)]
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == w, "list %d" % i
        assert timings[0].team_d3_sharded == 1 and timings[2].team_d3_sharded == 1
        assert timings[1].team_d3_sharded == 0  # (the gathered form took it)
    finally:
        _destroy(team)
        pg.free()


def test_a_list_in_front_that_leaves_the_devices(product, monkeypatch):
    """Three long lists in flight on a team of two; the first wait for a traceback behind their begin is told to give up
    (G2S_RESIDENT_TEST_FALLBACK=rel:0 — a share of the FIRST list: its two shares' waits are the first two).  That list
    is run again off the sharded form; the two behind it were begun before it ended, keep their step 1 and end sharded on
    the devices, from where the lead's generator stands after the first.  All three are the one session's."""
    monkeypatch.delenv("G2S_RESIDENT", raising=False)
    monkeypatch.delenv("G2S_TEAM_IN_FLIGHT", raising=False)
    monkeypatch.delenv("G2S_RESIDENT_TEST_FALLBACK", raising=False)
    seqs, gl, _ = _genome(product, 4200)
    allg = _gaps(product, gl)
    lists = [allg[:2100], allg[2100:4200], allg[1000:3100]]
    lib = product.load_library()
    pg = product.Graph.from_seqs(seqs, K, 1)
    team, bufs = [], []
    try:
        solo, want = _solo(product, pg, lists, 23)
        tail = [_key(r) for r in solo.fill_batch_onecall(allg[:300], pinned=True)]
        solo.destroy()
        team = _team(product, pg, 2, 23)
        lead = team[0]
        bufs = [_Bufs(product, lead, L, True) for L in lists]
        for b in bufs:
            product._check(b.begin(lead))
        assert (lead.in_flight(), lead.in_flight_launched()) == (3, 3)
        # (the wait counter is the process's and restarts when the value changes: atoi reads the 0, the rest makes the
        # value one no test has set before)
        monkeypatch.setenv("G2S_RESIDENT_TEST_FALLBACK", "rel:0 #%d" % next(_nonce))
        timings = []
        for b in bufs:
            product._check(lib.g2s_fill_end(lead.h))
            timings.append(lead.last_timing())
        monkeypatch.delenv("G2S_RESIDENT_TEST_FALLBACK")
        assert timings[0].team_d3_sharded == 0 and timings[0].resident_fallbacks >= 1
        for tm in timings[1:]:
            assert tm.team_d3_sharded == 1 and tm.team_groups == 2 and tm.resident_fallbacks == 0 and tm.resident_launches == 1
        for i, (b, w) in enumerate(zip(bufs, want)):
            assert b.keys() == w, "list %d" % i
        assert [_key(r) for r in lead.fill_batch_onecall(allg[:300], pinned=True)] == tail
    finally:
        monkeypatch.delenv("G2S_RESIDENT_TEST_FALLBACK", raising=False)
        if team:
            _drain(product, team[0])
        for b in bufs:
            b.free()
        _destroy(team)
        pg.free()


def test_refusals_with_a_team_list_in_flight(product, monkeypatch):
    """While the lead has a list in flight, the lead AND its helpers refuse what would use their buffers or move the
    stream (G2S_ERR_STATE, nothing changed); a fourth g2s_fill_begin is G2S_ERR_ARG as on one session; after the lists
    have ended the calls work again."""
    monkeypatch.delenv("G2S_RESIDENT", raising=False)
    monkeypatch.delenv("G2S_TEAM_IN_FLIGHT", raising=False)
    seqs, gl, _ = _genome(product, 4200)
    allg = _gaps(product, gl)
    lists = [allg[:2100], allg[2100:4200], allg[1000:3100]]
    lib = product.load_library()
    pg = product.Graph.from_seqs(seqs, K, 1)
    team, bufs = [], []
    try:
        solo, want = _solo(product, pg, lists, 29)
        solo.destroy()
        team = _team(product, pg, 2, 29)
        lead, helper = team
        bufs = [_Bufs(product, lead, L, True) for L in lists]
        extra = _Bufs(product, lead, allg[:300], True)
        bufs.append(extra)
        product._check(bufs[0].begin(lead))
        assert lead.in_flight_launched() == 1
        ap = C.cast(extra.arena.p, C.c_char_p)
        refused = [
            lib.g2s_fill_batch(lead.h, extra.arr, extra.n, extra.res, ap, extra.nbytes),
            lib.g2s_session_srand(lead.h, 99),
            lib.g2s_session_set_team(lead.h, (product._VP * 1)(helper.h), 1, 0),
            lib.g2s_fill_batch(helper.h, extra.arr, extra.n, extra.res, ap, extra.nbytes),
            lib.g2s_session_srand(helper.h, 99),
        ]
        assert refused == [product.G2S_ERR_STATE] * len(refused)
        assert b"in flight" in lib.g2s_last_error()
        assert extra.begin(helper) == product.G2S_ERR_STATE  # (nor does the helper begin a list of its own)
        product._check(bufs[1].begin(lead))
        product._check(bufs[2].begin(lead))
        assert extra.begin(lead) == -1  # (G2S_ERR_ARG: G2S_MAX_IN_FLIGHT lists are in flight already)
        assert (lead.in_flight(), lead.in_flight_launched()) == (3, 3)
        _drain_checked(product, lead)
        for i, w in enumerate(want):
            assert bufs[i].keys() == w, "list %d" % i
        # no list in flight any more: the same calls work, on the helper and on the lead
        product._check(lib.g2s_session_srand(helper.h, 29))
        product._check(lib.g2s_fill_batch(helper.h, extra.arr, extra.n, extra.res, ap, extra.nbytes))
        on_helper = extra.keys()
        product._check(lib.g2s_session_srand(lead.h, 29))
        product._check(lib.g2s_session_set_team(lead.h, (product._VP * 1)(helper.h), 1, product.G2S_GROUP_PER_SESSION))
        product._check(lib.g2s_fill_batch(lead.h, extra.arr, extra.n, extra.res, ap, extra.nbytes))
        assert extra.keys() == on_helper == want[0][:300]
    finally:
        if team:
            _drain(product, team[0])
        for b in bufs:
            b.free()
        _destroy(team)
        pg.free()


def _drain_checked(product, lead):
    lib = product.load_library()
    while lib.g2s_fill_in_flight(lead.h) > 0:
        product._check(lib.g2s_fill_end(lead.h))


def test_destroy_with_team_lists_in_flight(product, monkeypatch):
    """Two long lists begun on a team of two and never ended: destroying the lead waits for their kernels on every
    session they run on and drops them, the helpers go afterwards, and a fresh team on the same graph fills a list as
    one session does."""
    monkeypatch.delenv("G2S_RESIDENT", raising=False)
    monkeypatch.delenv("G2S_TEAM_IN_FLIGHT", raising=False)
    seqs, gl, _ = _genome(product, 4200)
    allg = _gaps(product, gl)
    lists = [allg[:2100], allg[2100:4200]]
    pg = product.Graph.from_seqs(seqs, K, 1)
    team, bufs = [], []
    try:
        solo, want = _solo(product, pg, lists[:1], 31)
        solo.destroy()
        team = _team(product, pg, 2, 31)
        bufs = [_Bufs(product, team[0], L, True) for L in lists]
        for b in bufs:
            product._check(b.begin(team[0]))
        assert team[0].in_flight_launched() == 2
        team[0].destroy()  # (returns: the kernels are waited for, the lists dropped)
        team[1].destroy()
        for b in bufs:     # (nothing writes into them any more)
            b.free()
        bufs = []
        team = _team(product, pg, 2, 31)
        got, timings, counts = _stream(product, team[0], [(lists[0], True)], 3)
        assert got == want and counts == [(1, 1)] and timings[0].team_d3_sharded == 1
    finally:
        for b in bufs:
            b.free()
        _destroy(team)
        pg.free()


def test_execute_stream_over_a_team(product, monkeypatch):
    """g2s_execute_scaffolds_stream on a lead with one helper, batches of 1 100 gaps (a record per gap: the next batch
    is begun before this one is ended and replayed): FASTA and log are those of a session without a team, and when a
    batch's text leaves (on_log) the batch behind it has its fill kernels queued on both sessions."""
    monkeypatch.delenv("G2S_RESIDENT", raising=False)
    monkeypatch.delenv("G2S_TEAM_IN_FLIGHT", raising=False)
    seqs, gl, text = _genome(product, 3400)
    lib = product.load_library()
    pg = product.Graph.from_seqs(seqs, K, 1)
    team = []
    try:
        one = product.Session(pg, 0, d_err=D_ERR, randseed=37)
        fas, lgs, ngaps, nfilled = one.execute_scaffolds_stream(text, K, 1100, solid=1)
        one.destroy()
        want = ("".join(fas), "".join(lgs), ngaps, nfilled)
        assert ngaps == 3400 and nfilled > 1500 and len(lgs) >= 3
        team = _team(product, pg, 2, 37)
        lead = team[0]
        fa, lg, launched = [], [], []

        def on_log(t, n, u):
            lg.append(C.string_at(t, n).decode("ascii"))
            launched.append(lib.g2s_fill_in_flight_launched(lead.h))

        on_fa = product.TEXT_FN(lambda t, n, u: fa.append(C.string_at(t, n).decode("ascii")))
        on_lg = product.TEXT_FN(on_log)
        o = product.g2s_run_opts(K, 1, 10, 1, 20.0)
        gaps, filled = C.c_int32(0), C.c_int32(0)
        product._check(lib.g2s_execute_scaffolds_stream(lead.h, C.byref(o), b"reads.fa", b"filled.fa", text.encode("ascii"), 1100,
                                                        on_fa, on_lg, None, C.byref(gaps), C.byref(filled)))
        assert ("".join(fa), "".join(lg), gaps.value, filled.value) == want
        assert 1 in launched, launched
        assert lead.in_flight() == 0
    finally:
        _destroy(team)
        pg.free()
