"""The streaming form of the BAM read route (gap2seq_amd/csrc/bam_reads.h), the part that needs no device: the host
routes stream nothing, and the switch that asks for streaming does not reach them."""
import pytest

import bam_reads_cases as B
import bamwriter
from test_reads_text import _assert_same_graph

SWITCHES = ("G2S_HOST_BUILD", "G2S_HOST_READS", "G2S_HOST_INFLATE", "G2S_BUILD_PIECE_BYTES", "G2S_BUILD_RESIDENT_CAP",
            "G2S_BUILD_BAM_STREAM")


@pytest.fixture(autouse=True)
def no_switches(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


def _same_tables(product, g, ref):
    a, b = product.test_graph_tables(g), product.test_graph_tables(ref)
    assert g.num_kmers == ref.num_kmers and bytes(a[0]) == bytes(b[0]) and bytes(a[1]) == bytes(b[1])


def test_the_host_routes_stream_nothing(product, tmp_path, monkeypatch):
    genome, recs = B.graph_reads(31)
    reads = B.reads(recs)
    path = tmp_path / "reads.bam"
    path.write_bytes(bamwriter.bam_bytes(B.REFS, recs, block=5000))
    monkeypatch.setenv("G2S_HOST_BUILD", "1")
    ref = product.Graph.from_seqs(reads, 31, 2)
    graphs = [ref]
    try:
        for switches in (dict(G2S_HOST_BUILD="1"), dict(G2S_HOST_READS="1"),
                         dict(G2S_HOST_READS="1", G2S_BUILD_BAM_STREAM="1"), dict(G2S_HOST_BUILD="1", G2S_BUILD_BAM_STREAM="1")):
            for name in SWITCHES:
                monkeypatch.delenv(name, raising=False)
            for name, value in switches.items():
                monkeypatch.setenv(name, value)
            g = product.Graph.from_files(str(path), 31, 2)
            graphs.append(g)
            load, bam = product.last_reads_load(), product.last_reads_bam()
            assert product.last_reads_bam_stream() == dict(streamed_files=0, windows=0, peak_device_bytes=0)
            assert (load["on_device"], load["inflate"], load["records"]) == (0, ["zlib"], len(reads))
            assert (bam["files"], bam["kept"], bam["kernels"], bam["reason"]) == (1, len(reads), 0, "not asked")
            _same_tables(product, g, ref)
            _assert_same_graph(g, ref, 31, [genome], 21)
    finally:
        for g in graphs:
            g.free()


def test_the_host_text_streams_nothing(product, monkeypatch):
    monkeypatch.setenv("G2S_BUILD_BAM_STREAM", "1")
    recs = B.length_records()
    data = bamwriter.bam_bytes(B.REFS, recs, block=100)
    assert product.reads_text(data, device=-1) == B.text(recs)
    assert product.last_reads_bam_stream() == dict(streamed_files=0, windows=0, peak_device_bytes=0)
    assert product.last_reads_bam()["reason"] == "not asked"
