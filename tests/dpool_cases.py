"""Cases of the device-held read pools (g2s_filter_reads_gaps_dpool, g2s_graph_build_dpool_reach) shared by
tests/test_device_pool.py (host-held handles, no device) and tests/test_gpu_device_pool.py (device-held handles): BAM
libraries whose pools have the properties the hand-over has to keep, pools that hold given sequences, and the comparison
of a handle with the host pool of the same call."""
import functools
import random

import bamwriter as BW
import pool_cases as PC

G2S_ERR_ARG = -1
KS = (31, 63, 95, 30)   # the three key widths, and an even k (predecessor table)


@functools.lru_cache(maxsize=None)
def designed_library():
    """(bam, gaps): a 1 500-pair library with a gap in the scaffolds (mate-unmapped reads around it, reverse-strand
    mates, 2% reads with an ambiguity code), a gap named three times and a wider one over it, and at the file's end
    unplaced records: one without bases, reads of 51 and 50 bases, a reverse-strand one, one of every 4-bit code."""
    refs, recs, _ = BW.simulate_library(43, n_scaffolds=2, scaffold_len=12000, gap=(6000, 250), pairs=1500, unmapped_pairs=40)
    rng = random.Random(44)
    gaps = [(rng.choice(refs)[0], rng.randrange(500, 11500), rng.choice([-1, 0, rng.randrange(1, 400)]),
             rng.choice([-1, 0, rng.randrange(1, 150)])) for _ in range(40)] + [("scaf0", 6000, 250, 60), ("nosuch", 10, 5, 5)]
    gaps += [("scaf0", 6000, 250, 60), ("scaf0", 6010, 250, 300), ("scaf0", 6000, 250, 60)]
    # flanks that reach over the left window: the unmapped mates placed there are in list 1 (their mate's name is in the
    # gap's filter) and in list 2 (they lie on the flank)
    gaps.append(("scaf0", 6010, 250, 450))
    dna = "".join(rng.choice("ACGT") for _ in range(51))
    extra = [BW.record("nobases", 4 | 1 | 64 | 8, -1, -1, "", ""),
             BW.record("odd", 4 | 1 | 128 | 8, -1, -1, "", dna),
             BW.record("even", 4 | 1 | 64 | 8, -1, -1, "", dna[:50]),
             BW.record("reverse", 4 | 16 | 1 | 128 | 8, -1, -1, "", dna[:37]),
             BW.record("codes", 4 | 1 | 64 | 8, -1, -1, "", "=ACMGRSVTWYHKDBN" + dna[:7])]
    return BW.bam_bytes(refs, list(recs) + extra, block=5000), gaps


def assert_designed_properties(pool, n_gaps):
    """the cases designed_library exists for, read off the host pool of the call"""
    seqs = pool.seqs
    gap_reads = [list(pool.gap_reads(i)) for i in range(n_gaps)]
    times = {}
    for g in gap_reads:
        for r in set(g):
            times[r] = times.get(r, 0) + 1
    assert max(times.values()) >= 3                                 # a read three gaps select
    assert any(len(set(g)) < len(g) for g in gap_reads)              # a read twice in one gap (its lists 1 and 2)
    assert set(pool.unmapped) & set(times)                           # an unmapped read that a gap selected too
    assert b"" in seqs                                               # a record without bases
    assert any(len(s) % 2 for s in seqs) and any(len(s) and len(s) % 2 == 0 for s in seqs)
    names = pool.names
    codes = seqs[names.index(b"codes/1")]
    assert codes.startswith(b"NACNGNNNTNNNNNNN")                     # codes outside 1, 2, 4, 8 read N
    rev = seqs[names.index(b"reverse/2")]
    odd = seqs[names.index(b"odd/2")]
    assert rev == BW.revcomp(odd[:37].decode()).encode()             # a reverse-strand read, as sequenced


def assert_same_pool(dp, pool, n_gaps):
    """every array of the handle's view against the host pool's (made with names), and every read"""
    import numpy as np
    p = pool.p.contents
    n = pool.n_reads
    assert dp.n_reads == n and dp.total == pool.total and dp.bases_is_null and dp.names_is_null
    assert list(dp.base_off) == p.base_off[0:n + 1]
    assert list(dp.name_off) == p.name_off[0:n + 1]
    assert list(dp.gap_begin) == p.gap_begin[0:n_gaps + 1]
    assert list(dp.gap_read) == p.gap_read[0:p.gap_begin[n_gaps]]
    assert list(dp.unmapped_read) == list(pool.unmapped)
    assert dp.base_off.dtype == np.uint64 and dp.gap_read.dtype == np.uint32
    seqs = pool.seqs
    for r in range(n):
        assert dp.read(r) == seqs[r], r


def pool_bam(seqs, name="q"):
    """a BAM whose unmapped reads are `seqs` in order: filtered with no gaps and unmapped=True, the pool holds them,
    read r being seqs[r]"""
    recs = [BW.record("%s%05d" % (name, i), 4 | 1 | 64 | 8, -1, -1, "", s) for i, s in enumerate(seqs)]
    return BW.bam_bytes([("s", 1000)], recs, block=5000)


def split_workload(k, mode):
    """PC.pool_workload with its pool cut in two: (seqs, set_lists, shared, set_shared, cut).  Between the workload's
    sequences the pools hold reads no list names (a strict subset is in use: holes in the source, starts that are no
    multiple of 16) and a read without bases; indices are those of the padded pool."""
    seqs, set_lists, shared, set_shared = PC.pool_workload(k, mode)
    rng = random.Random(k)
    padded, new = [], {}
    for i, s in enumerate(seqs):
        padded.append("".join(rng.choice("ACGT") for _ in range(rng.randrange(1, 40))))   # (in no list)
        if i == 3:
            padded.append("")
        new[i] = len(padded)
        padded.append(s)
    set_lists = [[new[i] for i in lst] for lst in set_lists]
    shared = [new[i] for i in shared]
    set_lists[7] = set_lists[7] + [new[3] - 1]   # (the read without bases, beside the read shorter than k)
    return padded, set_lists, shared, set_shared, new[4]


def reach_for(product, seqs, set_lists, k, d_err=100):
    """a sound reach record for every other set with reads: flanks from the set's first read"""
    reach = []
    for s, lst in enumerate(set_lists):
        text = seqs[lst[0]] if lst else ""
        if s % 2 or len(text) < 2 * k + 40:
            reach.append(None)
            continue
        gap = product.Gap(text[:k + 5], text[k + 35:2 * k + 40], 30, 5, 5)
        reach.append((gap, product.reach_radius(gap, d_err)))
    return reach
