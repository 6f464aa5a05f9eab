"""tests/trace_model.py — which way a gap's traceback takes through the code that turns a closure into fill text,
restated from the sources: g2s_d3_trace (gap2seq_amd/csrc/d3_device.hip, "(i) The chain of segments"), the fill wave's
own tracer (fill_seg.hip, "the traceback of a gap whose path is its only one") and the list's sizes (g2s_api.hip:
dmax, map_cap, seg_cap).  TEST INFRASTRUCTURE: it imports nothing from the product; its input is the closure of
tests/seg_model.py (fill_model(...).compact: one 8-word record per closure segment, children before parents) or any
closure in that layout.

The trace kernel finds the chain of segments a traceback enters in one of four ways:
  big     the closure has more segments than seg_cap (192; 512 under the skip rule) and g2s_d2_* analysed it: the walk
          goes through the records in device memory, a round trip a hop
  jump    L * nsegs <= 2 * map_cap, L = ceil(log2 nsegs): pointer jumping, the tables in the base map's room
  chase   hop by hop through LDS; a gap whose fill wave guessed hashes the chain as it goes (one masked store a hop),
          any other keeps hop h in lane h & 63 and stores 64 hops at a time
and then checks the hops' depths by a scan, 64 hops a step.  map_cap belongs to the LIST: (dmax + 5) & ~3 with dmax the
largest lmf + rmf + gap_len + d_err of its gaps."""
NOPAR = 0xFFFF
SUB_SOURCE = 4
SEG_CAP = 192
SEG_CAP_SKIP = 512       # G2S_SEG_CAP: the trace kernel's closure room under the skip rule
FILL_TRACE_HOPS = 256    # fill_seg.hip: nh >= 256 gives up
FILL_TRACE_LEN = 4096    # len0 <= 4096
FILL_TRACE_REC = 256     # nrec <= 256
FILL_ANALYSED_SEGS = 192  # the fill kernel analyses closures of up to 192 LOGGED segments itself
DEEP = 2500              # g2s_api.hip: a list with a gap of D >= 2500 is deep


def gap_d(gap, d_err):
    return gap["lmf"] + gap["rmf"] + gap["gap_len"] + d_err


def list_dmax(gaps, d_err):
    """g2s_api.hip, size_range: the largest lmf + rmf + gap_len + d_err of the list"""
    return max(gap_d(g, d_err) for g in gaps)


def map_cap_of(dmax):
    """g2s_api.hip: P.map_cap = (dmax + 2 + 3) & ~3"""
    return (dmax + 5) & ~3


def parents_of(rec):
    p01, p23 = rec[4], rec[5]
    return [p for p in (p01 & 0xFFFF, p01 >> 16, p23 & 0xFFFF, p23 >> 16) if p != NOPAR]


def _seg_pos(v0, length, node):
    if (node ^ v0) & 1:
        return -1
    t = (node - v0) // 2 if (v0 & 1) == 0 else (v0 - node) // 2
    return t if 0 <= t < length else -1


def starts_of(compact, reached, lengths):
    """[(segment, state)] of the traceback start of each path length: the closure segment that holds the reached
    target at depth `length` (seg_model: own_t)."""
    out = []
    for ln in lengths:
        found = None
        for i, rec in enumerate(compact):
            d0, n = rec[1] & 0xFFFF, rec[1] >> 16
            t = _seg_pos(rec[0], n, reached)
            if t >= 0 and d0 + t == ln:
                assert found is None, "two starts for one length"
                found = (i, t)
        assert found is not None, "no start for length %d" % ln
        out.append(found)
    return out


def hop_range(compact, start):
    """(fewest, most) segments a traceback enters from `start` down to a source, over every choice of parents, and the
    stop depths (depth of the source's first state) it can end at.  A traceback enters the start segment, then from a
    segment's first state one of its parents, until a source."""
    memo = {}
    for i in range(len(compact) - 1, start - 1, -1):  # (children before parents: a parent's index is the larger)
        rec = compact[i]
        if rec[6] & SUB_SOURCE:
            memo[i] = (1, 1, frozenset([rec[1] & 0xFFFF]))
        else:
            ps = parents_of(rec)
            assert ps and all(p > i for p in ps), "a closure segment without a way on, or a parent in front of its child"
            sub = [memo[p] for p in ps]
            memo[i] = (1 + min(s[0] for s in sub), 1 + max(s[1] for s in sub), frozenset().union(*[s[2] for s in sub]))
    return memo[start]


def has_choice(compact):
    """fill_seg.hip: `choice` — an entry of the traceback closure with more than one parent"""
    return any((rec[3] >> 16) != 0x7FFF and len(parents_of(rec)) > 1 and not rec[6] & SUB_SOURCE for rec in compact)


def closure_is_dag(compact):
    """fill_seg.hip, "phase D2 for closures without a repeated k-mer": no two segments' parts on a path to a sink
    overlap in k-mer index, i.e. no k-mer stands at two depths of the subgraph.  Only such a closure is analysed by the
    fill kernel itself (two path lengths never are: the reached k-mer has both depths)."""
    ivs = []
    for rec in compact:
        ts = rec[3] & 0x7FFF
        if ts != 0x7FFF:
            x = rec[0] >> 1
            ivs.append((x - ts, x) if rec[0] & 1 else (x, x + ts))
    ivs.sort()
    return all(b[0] > a[1] for a, b in zip(ivs, ivs[1:]))


def route(compact, reached, lengths, dmax, seg_cap=SEG_CAP, by_runs=False, logged=None, skip=False, regular=True):
    """Where the traceback of one gap goes.  compact, reached (the oriented node of the reached target), lengths: the
    gap's closure and phase C's outcome; dmax: the list's; seg_cap: 192, or 512 with the skip rule; by_runs: g2s_d2_*
    analysed the closure (G2S_DEVICE_D2=1: more than 192 logged segments or a k-mer at several depths); logged: the
    segments the left DP logged (seg_model: n_seg), for the fill wave's tracer; regular: the gap stays in the regular segment tier (at most 256 right-set entries, 512 logged segments,
    64 pending events: the large variant, which takes the others, has no tracer).  Returns a dict:
      ncl, ncl_s (the segments on a path to a sink), map_cap, big, nsegs, L, jump, way ("big" | "jump" | "chase" |
      "host"; which of the two chases a chasing gap takes is the fill wave's doing: the guessed one where it guessed)
      hops: [(fewest, most)] per path length, stops: the depths a traceback can end at, per path length
      fill: dict(sure, nh, len0, nrec, takes) — the fill wave's tracer: `takes` says whether it writes the gap
      (outright when sure, as a guess otherwise and only when it may guess)"""
    ncl = len(compact)
    map_cap = map_cap_of(dmax)
    big = ncl > seg_cap and by_runs
    nsegs = ncl if big else min(ncl, seg_cap)
    L = (nsegs - 1).bit_length() if nsegs > 1 else 0
    jump = (not big) and L * nsegs <= 2 * map_cap
    starts = starts_of(compact, reached, lengths)
    hr = [hop_range(compact, s[0]) for s in starts]
    if ncl > seg_cap and not by_runs:
        way = "host"  # (d3_device.hip: td.nsegs > seg_cap without runs is a bad walk)
    elif big:
        way = "big"
    elif jump:
        way = "jump"
    else:
        way = "chase"
    choice = has_choice(compact)
    stops0 = hr[0][2]
    sure = (not choice) and len(lengths) == 1 and len(stops0) == 1
    nlog = ncl if logged is None else logged
    dag = closure_is_dag(compact)
    analysed = regular and (skip or (nlog <= FILL_ANALYSED_SEGS and dag))
    nh = hr[0][1] if sure else None
    takes = (analysed and 1 <= lengths[0] <= FILL_TRACE_LEN and ncl <= FILL_TRACE_REC
             and (nh is None or nh <= FILL_TRACE_HOPS))
    ncl_s = sum(1 for rec in compact if (rec[3] & 0x7FFF) != 0x7FFF)  # segments on a path to a sink: what g2s_d2_* logs
    return dict(ncl=ncl, ncl_s=ncl_s, map_cap=map_cap, big=big, nsegs=nsegs, L=L, jump=jump, way=way,
                hops=[(h[0], h[1]) for h in hr], stops=[sorted(h[2]) for h in hr],
                fill=dict(sure=sure, choice=choice, dag=dag, regular=regular, nh=nh, len0=lengths[0], nrec=ncl, takes=takes))
