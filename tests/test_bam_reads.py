"""BAM files as read files of the graph build, the part that needs no device (gap2seq_amd/csrc/bam_reads.h): a BAM
file is told by its bytes, the host route's text is the model's (tests/bam_reads_cases.py), the graph is
Graph.from_seqs' of the model's reads, alone and in a mixed list, and a broken file is an error that names it."""
import pytest

import bam_reads_cases as B
import bamwriter
import fastx_model as M
from test_reads_text import _assert_same_graph

CASES = B.cases()


@pytest.fixture(autouse=True)
def host_build(monkeypatch):
    monkeypatch.setenv("G2S_HOST_BUILD", "1")


@pytest.mark.parametrize("name,data,recs,pieces", CASES, ids=[c[0] for c in CASES])
def test_host_text_is_the_models(product, name, data, recs, pieces):
    want = B.text(recs)
    for device in (-1, -2):  # (there is no line machine for BAM: both are the reader's walk)
        assert product.reads_text(data, device=device) == want
        info, bam = product.last_reads_load(), product.last_reads_bam()
        assert (info["files"], info["positions"], info["records"], info["on_device"]) == (1, len(want), len(B.reads(recs)), 0)
        assert info["inflate"] == ["zlib"]
        assert bam == dict(files=1, kept=len(B.reads(recs)), skipped=len(recs) - len(B.reads(recs)), kernels=0,
                           reason="not asked", anomaly=0)


def _same_tables(product, g, ref):
    a, b = product.test_graph_tables(g), product.test_graph_tables(ref)
    assert g.num_kmers == ref.num_kmers and bytes(a[0]) == bytes(b[0]) and bytes(a[1]) == bytes(b[1])


@pytest.mark.parametrize("k", [31, 32])
def test_from_files_on_the_host(product, tmp_path, k):
    genome, recs = B.graph_reads(k)
    reads = B.reads(recs)
    assert len(reads) < len(recs) and "" in reads
    path = tmp_path / "reads.bam"
    path.write_bytes(bamwriter.bam_bytes(B.REFS, recs, block=5000))
    ref = product.Graph.from_seqs(reads, k, 2)
    g = product.Graph.from_files(str(path), k, 2)
    try:
        info, bam = product.last_reads_load(), product.last_reads_bam()
        assert (info["files"], info["records"], info["on_device"], info["inflate"]) == (1, len(reads), 0, ["zlib"])
        assert info["positions"] == sum(len(r) + 1 for r in reads) == product.test_last_solid_count()["positions"]
        assert (bam["files"], bam["kept"], bam["skipped"], bam["kernels"]) == (1, len(reads), len(recs) - len(reads), 0)
        assert g.num_kmers > 1000
        _same_tables(product, g, ref)
        _assert_same_graph(g, ref, k, [genome], 5)
    finally:
        g.free()
        ref.free()


@pytest.mark.parametrize("k", [31, 32])
def test_from_files_mixed_list_on_the_host(product, tmp_path, k):
    """a.fq.gz,b.bam,c.fa: the text is the files' texts in list order"""
    genome, recs = B.graph_reads(k)
    third = len(recs) // 3
    first, last = B.reads(recs[:third]), B.reads(recs[2 * third:])
    a, b, c = tmp_path / "a.fq.gz", tmp_path / "b.bam", tmp_path / "c.fa"
    a.write_bytes(M.gz(M.fastq(first)))
    b.write_bytes(bamwriter.bam_bytes(B.REFS, recs[third:2 * third]))
    c.write_bytes(M.fasta(last, 60))
    reads = first + B.reads(recs[third:2 * third]) + last
    assert sorted(reads) == sorted(B.reads(recs))
    ref = product.Graph.from_seqs(reads, k, 2)
    g = product.Graph.from_files("%s,%s,%s" % (a, b, c), k, 2)
    try:
        info = product.last_reads_load()
        assert (info["files"], info["records"], info["inflate"]) == (3, len(reads), ["zlib", "zlib", "none"])
        assert info["positions"] == sum(len(r) + 1 for r in reads)
        assert product.last_reads_bam()["files"] == 1
        _same_tables(product, g, ref)
        _assert_same_graph(g, ref, k, [genome], 6)
    finally:
        g.free()
        ref.free()


def _broken(damage):
    recs = B.length_records()
    if damage == "truncated":  # (the file ends inside a member)
        return bamwriter.bam_bytes(B.REFS, recs, block=3000, eof=False)[:-20]
    if damage == "corrupt-member":  # (a flipped byte in the deflate bytes of a member behind the header's)
        whole = bamwriter.bam_bytes(B.REFS, recs, block=3000)
        first = len(bamwriter.bam_bytes(B.REFS, []))
        assert len(whole) > first + 2000
        data = bytearray(whole)
        data[len(data) // 2] ^= 0x55
        return bytes(data)
    assert damage == "cut-record"  # (every member is whole; the stream ends inside the last record)
    raw_end = b"".join(recs)[:-7]
    hdr = bamwriter.bam_bytes(B.REFS, [], eof=False)
    return hdr + bamwriter.bgzf(raw_end, block=3000)


@pytest.mark.parametrize("damage", ["truncated", "corrupt-member", "cut-record"])
def test_broken_bam_is_an_error_naming_the_file(product, tmp_path, damage):
    data = _broken(damage)
    path = tmp_path / "damaged.bam"
    path.write_bytes(data)
    with pytest.raises(product.G2SError) as e:
        product.Graph.from_files(str(path), 31, 2).free()
    assert "damaged.bam" in str(e.value)
    with pytest.raises(product.G2SError):
        product.reads_text(data, device=-1)


def test_bgzf_fastq_is_still_fastx(product):
    reads = B.reads(B.length_records())
    fq = M.fastq([r for r in reads if r])
    assert product.reads_text(bamwriter.bgzf(fq, block=500), device=-1) == M.text(fq)
    assert product.last_reads_bam()["files"] == 0


def test_plain_gzip_that_begins_with_bam_is_still_fastx(product):
    """the magic alone does not make a BAM file: the first member must be a BGZF member"""
    data = b"BAM\x01\n>r\nACGTTGCA\n>s\nGGA\n"
    want = M.text(data)
    assert want == b"ACGTTGCANGGAN"
    assert product.reads_text(M.gz(data), device=-1) == want
    assert product.last_reads_bam()["files"] == 0
    # (the same bytes in BGZF members are a BAM file by definition — and one whose header does not parse)
    with pytest.raises(product.G2SError):
        product.reads_text(bamwriter.bgzf(data), device=-1)
