"""The batched read filter (g2s_filter_reads_gaps, gap2seq_amd/csrc/readfilter_gaps.cpp) on its host path: the reads of
N gaps of one library in two passes over the BAM, every gap's output equal to the per-gap filter's (g2s_filter_reads)
and to the restatement's (oracle/readfilter_ref.py).  CPU only; tests/test_gpu_readfilter_gaps.py runs the same cases
with the joins on the device."""
import os
import random
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import bamwriter as BW  # noqa: E402
import filter_gap_cases as FC  # noqa: E402
import readfilter_ref as REF  # noqa: E402
from gap2seq_amd import lib as P  # noqa: E402


@pytest.mark.parametrize("case", FC.all_cases(), ids=lambda c: c[0])
def test_every_gap_equals_the_per_gap_filter(case):
    _, bam, mean, sd, gaps = case
    want = FC.expected(P, bam, mean, sd, gaps)
    got, stats = P.filter_reads_gaps(bam, mean, sd, gaps, device=-1)
    assert stats["on_device"] == 0 and stats["file_passes"] == 2
    assert len(got) == len(gaps)
    for g, w, x in zip(gaps, want, got):
        assert x == w, g


NEW_LIBRARIES = ("sd-negative", "long-span", "mixed-lengths", "repeated-names", "placed-at-minus-one", "many-scaffolds",
                 "high-coordinates")


@pytest.mark.parametrize("case", [c for c in FC.all_cases() if c[0].startswith(NEW_LIBRARIES)], ids=lambda c: c[0])
def test_the_per_gap_filters_pass_over_the_file_agrees_too(case, monkeypatch):
    """the per-gap filter without its candidate list (G2S_FILTER_MAX_CANDS=0: the windows applied in a pass over the
    file) on the libraries whose windows and spans are unusual: the restatement's answer again"""
    _, bam, mean, sd, gaps = case
    monkeypatch.setenv("G2S_FILTER_MAX_CANDS", "0")
    FC.expected(P, bam, mean, sd, gaps)


def test_golden_batch_covers_the_committed_answers():
    """All the committed calls (tests/golden/readfilter_cases.json) through the batched call, against the answers
    committed with them — the unmapped reads from the same two passes included."""
    import base64
    import json
    g = json.load(open(os.path.join(HERE, "golden", "readfilter_cases.json")))
    bam = base64.b64decode(g["bam_base64"])
    n = 0
    for c in g["calls"]:
        a = c["args"]
        gap = (a["scaffold"], a["breakpoint"], a.get("gap_length", -1), a.get("flank_length", -1))
        got, stats, un = P.filter_reads_gaps(bam, a["mean"], a["std_dev"], [gap], device=-1, unmapped=True)
        want = (c["fasta"], c["stdout"], c["stderr"])
        if a.get("unmapped_only"):
            assert un[:3] == want and un[4] == g["records"]
        else:
            assert got[0][:3] == want and got[0][4] == g["records"]
        n += 1
    assert n == len(g["calls"])


def test_the_empty_right_hand_window_holds_nothing(monkeypatch):
    """std_dev 0: the right-hand window is [x, x).  A mate-unmapped read spanning x must not enter the filter — on the
    per-gap filter's candidate path (default) and on its pass over the file (G2S_FILTER_MAX_CANDS=0) alike, as in the
    restatement, and in the batched filter."""
    bam, mean, sd, gaps = FC.empty_window_library()
    for cands in (None, "0"):
        if cands is None:
            monkeypatch.delenv("G2S_FILTER_MAX_CANDS", raising=False)
        else:
            monkeypatch.setenv("G2S_FILTER_MAX_CANDS", cands)
        for scaf, bp, gl, fl in gaps:
            got = P.filter_reads(bam, mean=mean, std_dev=sd, scaffold=scaf, breakpoint=bp, gap_length=gl, flank_length=fl)
            want = REF.read_filter(bam, mean, sd, scaf, bp, gl, fl)
            assert got[:3] == want, (cands, bp, fl)
            assert ">a/2\n" not in got[0]
    monkeypatch.delenv("G2S_FILTER_MAX_CANDS", raising=False)
    got, _ = P.filter_reads_gaps(bam, mean, sd, gaps, device=-1)
    assert [x[:3] for x in got] == [REF.read_filter(bam, mean, sd, *g) for g in gaps]


def test_a_hash_collision_extracts_the_colliding_read():
    bam, mean, sd, gaps, header = FC.collision()
    got, _ = P.filter_reads_gaps(bam, mean, sd, gaps, device=-1)
    assert header in got[0][0] and header in got[1][0] and header not in got[2][0]
    assert [x[:3] for x in got] == [REF.read_filter(bam, mean, sd, *g) for g in gaps]


def test_passes_do_not_grow_with_the_gaps():
    bam, scafs, _ = FC.simulated(7, pairs=300)
    rng = random.Random(7)
    gaps = FC.mixed_gaps(rng, scafs, 495)
    one, s1 = P.filter_reads_gaps(bam, 300, 20, gaps[:1], device=-1)
    many, s500 = P.filter_reads_gaps(bam, 300, 20, gaps, device=-1)
    assert len(gaps) == 500 and s1["file_passes"] == s500["file_passes"] == 2
    assert many[0] == one[0]
    want = FC.expected(P, bam, 300, 20, gaps, restatement=False)
    assert many == want
    assert sum(x[3] for x in many) > 500


def test_unmapped_reads_come_from_the_same_passes():
    for seed in (1, 2):
        bam, scafs, gaps = FC.simulated(seed, shuffle=seed == 2)
        got, stats, un = P.filter_reads_gaps(bam, 300, 20, gaps, device=-1, unmapped=True)
        assert stats["file_passes"] == 2
        want = P.filter_reads(bam, mean=300, std_dev=20, scaffold="0", breakpoint=0, gap_length=0, unmapped_only=True)
        assert un == want and un[3] > 0
        assert un[:3] == REF.read_filter(bam, 300, 20, "0", 0, 0, -1, True)
    none, _, un = P.filter_reads_gaps(bam, 300, 20, [], device=-1, unmapped=True)
    assert none == [] and un == want


def test_threads_and_bgzf_layout_do_not_change_the_answer():
    refs, recs, _ = BW.simulate_library(12, n_scaffolds=2, pairs=600)
    gaps = FC.mixed_gaps(random.Random(12), ["scaf0", "scaf1"], 40)
    results = []
    for block, threads in ((65280, 1), (600, 7), (333, 3)):
        bam = BW.bam_bytes(refs, recs, block=block)
        results.append(P.filter_reads_gaps(bam, 300, 20, gaps, device=-1, threads=threads)[0])
    assert results[0] == results[1] == results[2]
    assert results[0] == FC.expected(P, BW.bam_bytes(refs, recs), 300, 20, gaps, restatement=False)


def test_path_and_bytes_agree(tmp_path):
    bam, _, gaps = FC.simulated(3)
    path = tmp_path / "lib.bam"
    path.write_bytes(bam)
    assert P.filter_reads_gaps(str(path), 300, 20, gaps, device=-1)[0] == P.filter_reads_gaps(bam, 300, 20, gaps, device=-1)[0]


def test_host_switch_and_missing_device_fall_back_to_the_host(monkeypatch):
    bam, _, gaps = FC.simulated(2, shuffle=True)
    want = FC.expected(P, bam, 300, 20, gaps, restatement=False)
    monkeypatch.setenv("G2S_HOST_FILTER", "1")
    got, stats = P.filter_reads_gaps(bam, 300, 20, gaps, device=0)
    assert stats["on_device"] == 0 and got == want
    monkeypatch.delenv("G2S_HOST_FILTER")
    got, stats = P.filter_reads_gaps(bam, 300, 20, gaps, device=1 << 20)  # (no such device)
    assert stats["on_device"] == 0 and got == want


def test_errors_are_reported(monkeypatch, tmp_path):
    bam, _, gaps = FC.simulated(1)
    with pytest.raises(P.G2SError):
        P.filter_reads_gaps(str(tmp_path / "missing.bam"), 300, 20, gaps, device=-1)
    with pytest.raises(P.G2SError):
        P.filter_reads_gaps(bam[:len(bam) // 2], 300, 20, gaps, device=-1)
    monkeypatch.setenv("G2S_FILTER_MAX_PAIRS", "3")  # the pair cap: G2S_ERR_NOMEM, never a partial answer
    with pytest.raises(P.G2SError) as e:
        P.filter_reads_gaps(bam, 300, 20, gaps, device=-1)
    assert "cap" in str(e.value)
