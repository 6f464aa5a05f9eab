"""tests/trace_cases.py — designed tracebacks: planted gaps for the code that turns a closure into the fill text
(g2s_d3_trace in gap2seq_amd/csrc/d3_device.hip, the fill wave's own tracer in fill_seg.hip, post.cpp on the host),
one below, on and one above every bound that code names.  tests/trace_model.py says which way a gap goes;
tests/test_trace_cases.py proves on the CPU that every row is what it says; tests/test_gpu_trace_designed.py runs the
lists on the device.

Every row is ONE gap of cases.bubble_ladder at k = 31, fuz 3, with a seed of its own, so that the rows of a list share
one graph.  What sets the numbers:
  a backbone without bubbles is one path; every in-tip cuts its unitig, so T in-tips give T + 1 closure segments and a
  traceback of T + 1 hops, whatever is drawn (the fill wave traces such a gap outright: G2S_DEVA_TRACED);
  one SNP bubble in front of the tips adds its two arms and the stretch in front: T + 4 segments, T + 3 hops, and a
  choice (the fill wave can only guess: G2S_DEVA_SPEC; with guesses off the trace kernel chases the chain unguessed);
  run = J makes the bubble's arms J' + k unsafe states long: J' + 1 lower-case bases, the first exactly k below the
  safe base above the run;
  a deletion of two bases near the right flank, with the claimed length one short, gives two path lengths
  (len, len - 2), the first always the longer (:1125-1126 lists base + err in front of base - err);
  lead = -2 opens the first bubble inside the left seeds: one arm's traceback ends at depth 1, the other's at 3.

ROWS[name] = dict(list, gen (bubble_ladder's arguments), dgap (added to the claimed length), copies (how often the gap
stands in its list: every copy begins at another place of the rand() stream), want).  want holds the designed values:
  ncl    closure segments          hops   (fewest, most) segments a traceback enters, per path length
  len    phase C's path lengths    sure   the fill wave's tracer takes the gap outright (no choice, one length, one stop)
  stops  the depths a traceback can end at (left_fuz = lmf - stop), where the design is about them
  way    {d_err: route of trace_model.route} where the design is about the route
  low    (first, last) index of the fill text's lower-case stretch, where the design is about case
LISTS[name] = dict(d_errs, skip (the list runs with the skip rule), pads, env (what the device legs need))."""
import cases
import trace_model as TM

K, FUZ = 31, 3


def _tips(first, n):
    return tuple(range(first, first + n))


def _path(seed, hops, true_len):
    """One path of `hops` closure segments and hops: hops - 1 in-tips, a base apart, from offset 3 on."""
    return dict(seed=seed, k=K, m=0, spacing=32, lead=true_len, in_tips=_tips(3, hops - 1))


def _bubble(seed, hops, true_len):
    """One SNP bubble right behind the left flank, then hops - 3 in-tips behind its arms: hops + 1 segments."""
    return dict(seed=seed, k=K, m=1, spacing=32, lead=1, tail=true_len - 2, in_tips=_tips(2 + K + 1, hops - 3))


def _run(seed, run, step, lead, tail):
    return dict(seed=seed, k=K, m=1, spacing=32 + run, lead=lead, tail=tail, run=run, run_step=step)


ROWS = {}


def _row(name, lst, gen, want, copies=1, dgap=0):
    ROWS[name] = dict(list=lst, gen=gen, want=want, copies=copies, dgap=dgap)


# ---- the chain of segments: 63 / 64 / 65 hops (true length 138: the list's map_cap is 188 at -dist-error 10) ---------
# L * ncl against 2 * map_cap: 63 segments 378, 64 384, 65 455 (L = 7), 66 462.  map_cap 188 (d_err 10): all chase;
# 192 (d_err 14): 63 and 64 jump — 64 ON the bound, 6 * 64 = 2 * 192 —, 65 and 66 still chase; 240 (d_err 60): all jump.
_W64 = {63: {10: "chase", 14: "jump", 60: "jump"}, 64: {10: "chase", 14: "jump", 60: "jump"},
        65: {10: "chase", 14: "chase", 60: "jump"}, 66: {10: "chase", 14: "chase", 60: "jump"}}
_row("p1", "chain64", _path(1001, 1, 138), dict(ncl=1, hops=[(1, 1)], len=[172], sure=True, way={10: "jump", 14: "jump", 60: "jump"}), 2)
_row("p2", "chain64", _path(1002, 2, 138), dict(ncl=2, hops=[(2, 2)], len=[172], sure=True, way={10: "jump", 14: "jump", 60: "jump"}), 2)
for _h in (63, 64, 65):
    _row("p%d" % _h, "chain64", _path(1000 + _h, _h, 138), dict(ncl=_h, hops=[(_h, _h)], len=[172], sure=True, way=_W64[_h]), 2)
    _row("b%d" % _h, "chain64", _bubble(1100 + _h, _h, 138), dict(ncl=_h + 1, hops=[(_h, _h)], len=[172], sure=False, way=_W64[_h + 1]), 16)
# ---- 127 / 128 / 129 hops (true length 170).  127 segments 889, 128 896, 129 1032 (L = 8), 130 1040.  map_cap 220
# (d_err 10) and 444 (d_err 233): all chase — 444 is the largest map_cap at which 127 and 128 segments chase —; 448
# (d_err 237): 127 and 128 jump, 128 ON the bound (7 * 128 = 2 * 448); 520 (d_err 308): all jump.
_W128 = {127: {10: "chase", 233: "chase", 237: "jump", 308: "jump"}, 128: {10: "chase", 233: "chase", 237: "jump", 308: "jump"},
         129: {10: "chase", 233: "chase", 237: "chase", 308: "jump"}, 130: {10: "chase", 233: "chase", 237: "chase", 308: "jump"}}
for _h in (127, 128, 129):
    _row("p%d" % _h, "chain128", _path(1000 + _h, _h, 170), dict(ncl=_h, hops=[(_h, _h)], len=[204], sure=True, way=_W128[_h]), 2)
    _row("b%d" % _h, "chain128", _bubble(1100 + _h, _h, 170), dict(ncl=_h + 1, hops=[(_h, _h)], len=[204], sure=False, way=_W128[_h + 1]), 16)
# ---- the case rule across lanes and waves.  With at most 256 bases a thread of the four-wave kernel holds one base,
# thread t the t-th from the top of the fill; `safe` is the thread of the safe base above the run, `bottom` that of
# the run's lowest state: same wave; 61, 64 and 65 lanes up (the wave in front; the safe base at thread 50, so that
# threads 64 to 80 are upper case only by the word of the wave in front: from the top of the fill, which counts as
# safe, they are more than k away); two and three waves in front (121 and 181 lanes up); a fill of more than
# 256 bases (two bases a thread, six a lane of the one-wave kernels); an SNP's run of k states inside ONE lane's
# stretch of 35 bases of a one-wave kernel (the fill wave's tracer and G2S_TRACE_WAVES=1).
_row("r61same", "case", _run(1201, 30, 30, 20, 64), dict(ncl=4, hops=[(3, 3)], len=[149], sure=False, low=(20, 50), safe=64, bottom=125), 16)
_row("r61cross", "case", _run(1202, 30, 30, 20, 50), dict(ncl=4, hops=[(3, 3)], len=[135], sure=False, low=(20, 50), safe=50, bottom=111), 16)
_row("r64", "case", _run(1203, 33, 11, 20, 50), dict(ncl=4, hops=[(3, 3)], len=[138], sure=False, low=(20, 53), safe=50, bottom=114), 16)
_row("r65", "case", _run(1204, 34, 17, 20, 50), dict(ncl=4, hops=[(3, 3)], len=[139], sure=False, low=(20, 54), safe=50, bottom=115), 16)
_row("r121", "case", _run(1205, 90, 30, 20, 50), dict(ncl=4, hops=[(3, 3)], len=[195], sure=False, low=(20, 110), safe=50, bottom=171), 16)
# (200 bases: the safe base in wave 0, the run's lowest state at thread 231 in wave 3, which reads all three words)
_row("r181", "case", _run(1208, 150, 30, 20, 50), dict(ncl=4, hops=[(3, 3)], len=[255], sure=False, low=(20, 170), safe=50, bottom=231), 16)
_row("r331", "case", _run(1206, 300, 30, 20, 20), dict(ncl=4, hops=[(3, 3)], len=[375], sure=False, low=(20, 320), per=2), 16)
_row("snp35", "case", dict(seed=1207, k=K, m=1, spacing=32, lead=1014, tail=1191), dict(ncl=4, hops=[(3, 3)], len=[2240], sure=False, low=(1014, 1014), per1=35), 16)
# ---- two path lengths, and tracebacks that end at different depths of the left fuz
_row("two-lengths", "lens", dict(seed=1301, k=K, m=1, spacing=32, lead=60, tail=5, indel=True, indel_every=1, del_len=2),
     dict(ncl=5, hops=[(3, 3), (3, 3)], len=[101, 99], sure=False, stops=[[3], [3]]), 16, dgap=-1)
_row("two-stops", "lens", dict(seed=1302, k=K, m=1, spacing=32, lead=-2, tail=60),
     dict(ncl=5, hops=[(2, 4)], len=[93], sure=False, stops=[[1, 3]]), 16)
_row("two-lengths-two-stops", "lens", dict(seed=1303, k=K, m=2, spacing=40, lead=-2, tail=5, indel=True, indel_every=2, del_len=2),
     dict(ncl=9, hops=[(4, 6), (4, 6)], len=[79, 77], sure=False, stops=[[1, 3], [1, 3]]), 16, dgap=-1)
# (a closure with two path lengths holds the reached k-mer at two depths: the fill kernel does not analyse it, and its
# wave guesses such a gap only under the skip rule, where nothing is analysed — the same three rows on a list with
# -skip-confident: there the guess is the longer length, and the copies that draw the shorter are sent again)
for _n in ("two-lengths", "two-stops", "two-lengths-two-stops"):
    ROWS[_n + "/skip"] = dict(ROWS[_n], list="lens-skip", gen=dict(ROWS[_n]["gen"], seed=ROWS[_n]["gen"]["seed"] + 50))
# ---- the fill wave's tracer at its bounds (fill_seg.hip: nrec <= 256, nh >= 256 gives up, len0 <= 4096).  Closures of
# 255 to 257 segments are the fill kernel's own only under the skip rule (without it the kernel analyses up to 192
# logged segments itself and leaves the rest to phase D2): that list runs with -skip-confident.
for _h in (255, 256, 257):
    _row("rec%d" % _h, "fillcap", _path(1400 + _h, _h, 600), dict(ncl=_h, hops=[(_h, _h)], len=[634], sure=True, takes=_h <= 256), 4)
for _n in (4095, 4096, 4097):
    _row("len%d" % _n, "deep", dict(seed=1500 + _n, k=K, m=0, spacing=32, lead=_n - K - FUZ),
         dict(ncl=1, hops=[(1, 1)], len=[_n], sure=True, takes=_n <= 4096), 2)
# ---- the walk through device memory (`big`: more closure segments than the trace kernel's 192, analysed by g2s_d2_*)
# at 63 / 64 / 65 and 128 hops: an indel ladder of 18 bubbles (closure segments grow with the square of the deletions, hops
# with the bubbles: 37) with in-tips in front of its first bubble, where every k-mer has one depth: +1 segment, +1 hop.
# (128 hops: 91 in-tips, 287 segments — more than g2s_d2_small's 256: g2s_d2_big's, which the list runs behind it)
for _h in (63, 64, 65, 128):
    _row("big%d" % _h, "big", dict(seed=1600 + _h, k=K, m=18, spacing=32, indel=True, lead=_h - 37 + 40, in_tips=_tips(3, _h - 37)),
         dict(ncl=_h + 159, hops=[(_h, _h)], len=[_h + 582], sure=False, way={10: "big", 100: "big"}), 2)
# ---- the gap's runs in LDS or in device memory (2 * n_runs <= map_cap): a path of 401 segments, analysed by
# g2s_d2_big as a DAG — a run a segment, two where a sink splits one: 401 to 403 runs.  map_cap 752 (d_err 10): device
# memory; 840 (d_err 100): LDS.
_row("runs401", "big", _path(1701, 401, 700), dict(ncl=401, hops=[(401, 401)], len=[734], sure=True, way={10: "big", 100: "big"}), 2)

LISTS = {
    "chain64": dict(d_errs=(10, 14, 60), skip=False, pads=220, env={}),
    "chain128": dict(d_errs=(10, 233, 237, 308), skip=False, pads=220, env={}),
    "case": dict(d_errs=(10,), skip=False, pads=150, env={}),
    "lens": dict(d_errs=(10,), skip=False, pads=210, env={}),
    "lens-skip": dict(d_errs=(10,), skip=True, pads=210, env={}),
    "fillcap": dict(d_errs=(10,), skip=True, pads=250, env={}),
    # (a deep list of 256 gaps and more starts its longest gaps in the large variant, which has no tracer:
    # G2S_NO_EARLY_SEGW=1 keeps them in the regular tier — g2s_api.hip, resident_launch_fill)
    "deep": dict(d_errs=(10,), skip=False, pads=256, env=dict(G2S_NO_EARLY_SEGW="1")),
    "big": dict(d_errs=(10, 100), skip=False, pads=256, env=dict(G2S_DEVICE_D2="1", G2S_D2_BIG="1")),
}
_BUILT, _LISTS = {}, {}


def names_of(lst):
    return [n for n in ROWS if ROWS[n]["list"] == lst]


def row(name):
    """dict(seqs, gap, want, copies) of one row; built once a process."""
    if name not in _BUILT:
        r = ROWS[name]
        lad = cases.bubble_ladder(**r["gen"])
        gap = dict(lad["gap"])
        gap["gap_len"] += r["dgap"]
        _BUILT[name] = dict(seqs=lad["seqs"], gap=gap, want=r["want"], copies=r["copies"])
    return _BUILT[name]


def trace_list(lst):
    """One list on one graph: (haplotypes, gaps, {row: [indices of its copies]}).  The pads are short plain gaps of a
    genome of their own (5 to 30 bases: below every planted gap's lmf + rmf + gap_len, so that the planted gaps set
    the list's dmax); the copies of the planted gaps are spread evenly among them, a copy of every row in turn."""
    if lst in _LISTS:
        return _LISTS[lst]
    names = names_of(lst)
    seqs = []
    for n in names:
        seqs += row(n)["seqs"]
    genome = cases.random_dna(cases.SplitMix(4242 + len(lst)), 30000)
    seqs.append(genome)
    npad = LISTS[lst]["pads"]
    gaps = cases.cut_gaps(41, genome, K, fuz=FUZ, ngaps=npad, min_len=5, max_len=30, d_err=10, vary_fuz=False)
    planted = []
    for c in range(max(ROWS[n]["copies"] for n in names)):
        planted += [n for n in names if c < ROWS[n]["copies"]]
    idx = {n: [] for n in names}
    step = max(1, npad // len(planted))
    for j, n in enumerate(planted):
        at = min(len(gaps), 1 + j * (step + 1))
        gaps.insert(at, row(n)["gap"])
    for i, g in enumerate(gaps):
        for n in names:
            if g is row(n)["gap"]:
                idx[n].append(i)
    _LISTS[lst] = (seqs, gaps, idx)
    return _LISTS[lst]


def long_chain_list():
    """More than 768 gaps holding the rows of both chain lists (the long list's one-wave kernel behind g2s_d3_handoff):
    (haplotypes, gaps, {row: indices})."""
    a, b = trace_list("chain64"), trace_list("chain128")
    seqs = a[0] + b[0]
    gaps = list(a[1]) + list(b[1])
    genome = cases.random_dna(cases.SplitMix(4300), 30000)
    seqs.append(genome)
    gaps += cases.cut_gaps(43, genome, K, fuz=FUZ, ngaps=300, min_len=5, max_len=30, d_err=10, vary_fuz=False)
    idx = dict(a[2])
    idx.update({n: [len(a[1]) + i for i in v] for n, v in b[2].items()})
    return seqs, gaps, idx


_ROUTES = {}


def list_routes(product, seqs, gaps, d_err, skip=False, by_runs=False, key=None):
    """trace_model.route of every gap of a list at one -dist-error, by the segment tier's model: ([route, or None for a gap
    without a path], the list's dmax).  The same gap record (the copies of a planted gap) is modelled once."""
    import seg_model as M
    from test_seg_model import _model_gap
    if key is not None and key in _ROUTES:
        return _ROUTES[key]
    dmax = TM.list_dmax(gaps, d_err)
    pg = product.Graph.from_seqs(seqs, K, 1)
    out, seen = [], {}
    try:
        tb = M.Tables(product, pg)
        for g in gaps:
            if id(g) not in seen:
                mg = _model_gap(pg, K, g, d_err, True, skip)
                m = M.fill_model(tb, mg)
                assert not m.q7
                r = None
                if m.c_count > 0 and m.lengths:
                    # (the regular tier's capacities, cases.EDGE_LADDERS and FRONTIER_EDGES: a gap beyond one runs again
                    # in the large variant)
                    n_a = len(M.right_entries(tb, mg))
                    regular = n_a <= 256 and m.n_seg <= 512 and m.max_pending <= 64
                    r = TM.route(m.compact, mg.targets[m.reached_j], m.lengths, dmax, seg_cap=TM.SEG_CAP_SKIP if skip else TM.SEG_CAP,
                                 by_runs=by_runs, logged=m.n_seg, skip=skip, regular=regular)
                    r["nseg"], r["nA"] = m.n_seg, n_a
                seen[id(g)] = r
            out.append(seen[id(g)])
    finally:
        pg.free()
    if key is not None:
        _ROUTES[key] = (out, dmax)
    return out, dmax


def fill_counts(routes, guess):
    """(traced, guessed): the gaps the fill waves' tracer writes outright (G2S_DEVA_TRACED) and, with every gap allowed
    to guess (G2S_GUESS_PERCENT=100 on a two-wave list), as a guess (G2S_DEVA_SPEC)."""
    traced = sum(1 for r in routes if r and r["fill"]["takes"] and r["fill"]["sure"])
    guessed = sum(1 for r in routes if r and r["fill"]["takes"] and not r["fill"]["sure"]) if guess else 0
    return traced, guessed
