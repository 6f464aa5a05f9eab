"""Gap2Seq-libraries end to end: the wrapper's libraries flow (Gap2Seq.py -l, :133-218) in one process, against a
Python restatement of the wrapper's per-gap flow — the reads of every gap and library from oracle/readfilter_ref.py,
every library's unmapped reads when the threshold asks for them, a graph of those reads alone in the CPU oracle and its
execute_single with the same seed.  The output file and the `Filled X out of Y gaps` line must be identical."""
import os
import random
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import bamwriter as BW  # noqa: E402
import oracle_lib as O  # noqa: E402
import readfilter_ref as REF  # noqa: E402

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "gap2seq_amd", "Gap2Seq-libraries")
K, FUZ, SOLID, DERR, SEED = 31, 10, 1, 100, 3


def _seqs(fasta):
    out, cur = [], None
    for ln in fasta.splitlines():
        if ln.startswith(">"):
            if cur is not None:
                out.append(cur)
            cur = ""
        elif cur is not None:
            cur += ln
    if cur is not None:
        out.append(cur)
    return out


def _grep_bytes(fasta):
    """grep '^[^>;]' | wc -c (Gap2Seq.py:156-159)"""
    n = 0
    for ln in fasta.splitlines(keepends=True):
        if ln and ln[0] not in ">;\n":
            n += len(ln)
    return n


def _parse_gap(record, bed_line):
    """Gap2Seq.py:246-262"""
    lines = record.split("\n")
    comment, gap = lines[0], "".join(lines[1:])
    left = gap[:gap.upper().find("N")]
    right = gap[gap.upper().rfind("N") + 1:]
    cols = bed_line.rstrip().split("\t")
    return dict(comment=comment, left=left, right=right, flank=min(len(left), len(right)),
                gap=len(gap) - len(left) - len(right), scaffold=cols[0], bp=int(cols[1]) + len(left))


def _restatement(libs, records, bed_lines):
    unmapped = [REF.read_filter(data, mean, sd, "0", 0, gap_length=0, unmapped_only=True)[0] for data, mean, sd, _ in libs]
    threshold = sum(t for _, _, _, t in libs)
    out, ok = "", 0
    for rec, bl in zip(records, bed_lines):
        g = _parse_gap(rec, bl)
        reads, flen = [], 0
        for data, mean, sd, _ in libs:
            fa = REF.read_filter(data, mean, sd, g["scaffold"], g["bp"], gap_length=g["gap"], flank_length=g["flank"])[0]
            reads += _seqs(fa)
            flen += _grep_bytes(fa)
        if flen / g["gap"] < threshold:
            for fa in unmapped:
                reads += _seqs(fa)
        fill = g["left"] + "N" * g["gap"] + g["right"]
        if reads:
            og = O.OracleGraph(reads, K, SOLID)
            try:
                fa, _ = O.execute_single(og, g["left"], g["right"], g["gap"], K, solid=SOLID, d_err=DERR, max_fuz=FUZ,
                                         randseed=SEED)
            finally:
                og.free()
            fill = "".join(ln for ln in fa.splitlines() if not ln.startswith(">"))
        ok += "N" not in fill and "n" not in fill
        out += g["comment"] + "\n" + fill + "\n"
    return out, "Filled %i out of %i gaps" % (ok, len(records))


def test_libraries_command_line_matches_the_wrapper_flow(product, tmp_path):
    assert os.access(EXE, os.X_OK), "Gap2Seq-libraries was not built"
    length = 3000
    rng = random.Random(21)
    genome = "".join(rng.choice("ACGT") for _ in range(length))  # (simulate_library's first draws)
    libs = []
    for i, (pairs, mean, sd, thr) in enumerate([(500, 300, 20, 0.0), (200, 250, 30, 1000.0)]):
        refs, recs, _ = BW.simulate_library(21, n_scaffolds=1, scaffold_len=length, pairs=pairs, mean=mean, sd=sd,
                                            unmapped_pairs=15, ambiguous=0.0)
        data = BW.bam_bytes(refs, recs)
        (tmp_path / ("lib%d.bam" % i)).write_bytes(data)
        libs.append((data, mean, sd, thr))
    fl = K + FUZ
    # (bp, gap length, N or n, bases of the genome between the flanks beyond the gap's length: the last gap claims a
    # length no path has, it stays unfilled)
    gaps = [(1400, 200, "N", 0), (700, 100, "N", 0), (2200, 150, "n", 0), (1000, 40, "N", 0), (2600, 80, "N", 0),
            (450, 60, "N", 400)]
    records, bed = [], []
    for j, (bp, gl, ch, extra) in enumerate(gaps):
        seq = genome[bp - fl:bp] + ch * gl + genome[bp + gl + extra:bp + gl + extra + fl]
        records.append(">scaf0 scaffold 0 contig %d gap %d\n%s\n" % (j, j, seq))
        bed.append("scaf0\t%d\t%d\n" % (bp - fl, bp + gl + extra + fl))
    (tmp_path / "gaps.fa").write_text("".join(records))
    (tmp_path / "gaps.bed").write_text("".join(bed))
    (tmp_path / "libs.txt").write_text("".join("%s\t%d\t%d\t%g\n" % (tmp_path / ("lib%d.bam" % i), m, s, t)
                                               for i, (_, m, s, t) in enumerate(libs)))
    run = subprocess.run([EXE, "-libraries", str(tmp_path / "libs.txt"), "-gaps", str(tmp_path / "gaps.fa"), "-bed",
                          str(tmp_path / "gaps.bed"), "-filled", str(tmp_path / "out.fa"), "-k", str(K), "-fuz", str(FUZ),
                          "-solid", str(SOLID), "-dist-error", str(DERR), "-randseed", str(SEED)],
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    want_text, want_line = _restatement(libs, [r.rstrip("\n") for r in records], bed)
    assert (tmp_path / "out.fa").read_text() == want_text
    assert run.stdout.strip().splitlines()[-1] == want_line
    assert want_line == "Filled %d out of %d gaps" % (len(gaps) - 1, len(gaps))
