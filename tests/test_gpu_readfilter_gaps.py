"""The batched read filter with its joins on the MI355X (gap2seq_amd/csrc/readfilter_gpu.hip): the cases of
tests/test_readfilter_gaps.py with device 0, a library of 2 x 10^5 pairs and 2 000 gaps where the device and the host
joins give the same bytes for every gap, and Gap2Seq-libraries (one batched call per library) on more gaps and
libraries than tests/test_gpu_libraries.py, against a restatement of the wrapper's per-gap flow."""
import os
import random
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import bamwriter as BW  # noqa: E402
import filter_gap_cases as FC  # noqa: E402
import oracle_lib as O  # noqa: E402
import readfilter_ref as REF  # noqa: E402

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "gap2seq_amd", "Gap2Seq-libraries")


@pytest.mark.parametrize("case", FC.all_cases(), ids=lambda c: c[0])
def test_device_joins_equal_the_per_gap_filter(product, case):
    _, bam, mean, sd, gaps = case
    want = FC.expected(product, bam, mean, sd, gaps)
    got, stats = product.filter_reads_gaps(bam, mean, sd, gaps, device=0)
    assert stats["on_device"] == 1 and stats["file_passes"] == 2
    for g, w, x in zip(gaps, want, got):
        assert x == w, g
    assert len(got) == len(gaps)


def test_device_collision_and_unmapped(product):
    bam, mean, sd, gaps, header = FC.collision()
    got, stats, un = product.filter_reads_gaps(bam, mean, sd, gaps, device=0, unmapped=True)
    assert stats["on_device"] == 1 and header in got[0][0]
    assert un == product.filter_reads(bam, mean=mean, std_dev=sd, scaffold="0", breakpoint=0, gap_length=0, unmapped_only=True)


def test_device_passes_do_not_grow_with_the_gaps(product):
    bam, scafs, _ = FC.simulated(7, pairs=300)
    gaps = FC.mixed_gaps(random.Random(7), scafs, 495)
    _, s1 = product.filter_reads_gaps(bam, 300, 20, gaps[:1], device=0)
    many, s500 = product.filter_reads_gaps(bam, 300, 20, gaps, device=0)
    assert s1["file_passes"] == s500["file_passes"] == 2 and s500["on_device"] == 1
    assert many == FC.expected(product, bam, 300, 20, gaps, restatement=False)


def test_large_library_device_equals_host(product):
    """2 x 10^5 pairs on 8 scaffolds, records shuffled out of coordinate order, 2 000 gaps: every gap's bytes from the
    device joins equal the host joins'; a sample of gaps against the per-gap filter."""
    rng = random.Random(31)
    refs, recs, _ = BW.simulate_library(31, n_scaffolds=8, scaffold_len=60000, gap=(30000, 300), pairs=25000,
                                        unmapped_pairs=200, ambiguous=0.01)
    recs = list(recs)
    rng.shuffle(recs)
    bam = BW.bam_bytes(refs, recs)
    scafs = [r[0] for r in refs]
    gaps = []
    for i in range(2000):
        gaps.append((rng.choice(scafs + ["nosuch"] if i % 97 == 0 else scafs), rng.randrange(0, 60000),
                     rng.choice([-1, 0, rng.randrange(1, 500)]), rng.choice([-1, 0, rng.randrange(1, 200)])))
    dev, sd_ = product.filter_reads_gaps(bam, 300, 20, gaps, device=0)
    host, sh = product.filter_reads_gaps(bam, 300, 20, gaps, device=-1)
    assert sd_["on_device"] == 1 and sh["on_device"] == 0 and sd_["file_passes"] == 2
    assert dev == host
    assert sum(x[3] for x in dev) > 10000
    for i in range(0, 2000, 250):
        s, bp, gl, fl = gaps[i]
        assert dev[i] == product.filter_reads(bam, mean=300, std_dev=20, scaffold=s, breakpoint=bp, gap_length=gl,
                                              flank_length=fl), gaps[i]


# ---- Gap2Seq-libraries: the wrapper's per-gap flow restated (as tests/test_gpu_libraries.py builds it)

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
    return sum(len(ln) for ln in fasta.splitlines(keepends=True) if ln and ln[0] not in ">;\n")


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


@pytest.mark.parametrize("filter_device", [None, "-1"])
def test_libraries_with_batched_filtering_match_the_wrapper_flow(product, tmp_path, filter_device):
    assert os.access(EXE, os.X_OK), "Gap2Seq-libraries was not built"
    length = 6000
    rng = random.Random(23)
    genome = "".join(rng.choice("ACGT") for _ in range(length))  # (simulate_library's first draws)
    libs = []
    for i, (pairs, mean, sd, thr) in enumerate([(900, 300, 20, 0.0), (400, 250, 30, 0.5), (600, 350, 0, 1000.0)]):
        refs, recs, _ = BW.simulate_library(23, n_scaffolds=1, scaffold_len=length, gap=(3000, 200), pairs=pairs, mean=mean,
                                            sd=sd, unmapped_pairs=10, ambiguous=0.0)
        data = BW.bam_bytes(refs, recs, block=[65280, 5000, 700][i])
        (tmp_path / ("lib%d.bam" % i)).write_bytes(data)
        libs.append((data, mean, sd, thr))
    fl = K + FUZ
    gaps = [(3000, 200, "N", 0), (700, 100, "N", 0), (2200, 150, "n", 0), (1000, 40, "N", 0), (4600, 80, "N", 0),
            (5200, 120, "N", 0), (3900, 60, "n", 0), (1600, 90, "N", 0), (450, 60, "N", 400), (5600, 30, "N", 0),
            (2600, 70, "N", 0), (4200, 50, "N", 250)]
    records, bed = [], []
    for j, (bp, gl, ch, extra) in enumerate(gaps):
        seq = genome[bp - fl:bp] + ch * gl + genome[bp + gl + extra:bp + gl + extra + fl]
        records.append(">scaf0 scaffold 0 contig %d gap %d\n%s\n" % (j, j, seq))
        bed.append("scaf0\t%d\t%d\n" % (bp - fl, bp + gl + extra + fl))
    (tmp_path / "gaps.fa").write_text("".join(records))
    (tmp_path / "gaps.bed").write_text("".join(bed))
    (tmp_path / "libs.txt").write_text("".join("%s\t%d\t%d\t%g\n" % (tmp_path / ("lib%d.bam" % i), m, s, t)
                                               for i, (_, m, s, t) in enumerate(libs)))
    argv = [EXE, "-libraries", str(tmp_path / "libs.txt"), "-gaps", str(tmp_path / "gaps.fa"), "-bed",
            str(tmp_path / "gaps.bed"), "-filled", str(tmp_path / "out.fa"), "-k", str(K), "-fuz", str(FUZ),
            "-solid", str(SOLID), "-dist-error", str(DERR), "-randseed", str(SEED)]
    if filter_device is not None:
        argv += ["-filter-device", filter_device]
    run = subprocess.run(argv, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    want_text, want_line = _restatement(libs, [r.rstrip("\n") for r in records], bed)
    assert (tmp_path / "out.fa").read_text() == want_text
    assert run.stdout.strip().splitlines()[-1] == want_line
    assert int(want_line.split()[1]) >= len(gaps) - 3
