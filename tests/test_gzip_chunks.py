"""The chunked inflate of plain gzip files (gap2seq_amd/csrc/gzip_chunks.h) compiled for the host — gzip_inflate(...,
device=-2): the same finder, decoder, chain, resolve and CRC the kernels run, chunk by chunk — against Python's zlib, on
the designed files of gzip_cases.py.  tests/test_gpu_gzip_chunks.py puts the kernels to the same cases.

Expected outcomes.  A window that does not reach the file's end needs a second block start to hand the stream on, so
"too few starts" is a right answer wherever a window can be shorter than the distance between two starts; zlib's blocks
of this FASTQ text are 19 - 30 KB of compressed bytes (every ~16 K symbols), so a window of 64 KiB and more always holds
one and must complete, and a shorter one may give the file back — with no bytes."""
import pytest

import gzip_cases as G

LEVELS, CHUNKS, WINDOWS = (1, 6, 9), (4096, 16384, 65536), (2, 5, 0)


def must_complete(chunk, window):
    return window == 0 or chunk * (window - 1) >= 65536


def inflate_checked(product, data, payload, device, chunk, window, complete):
    got, outcome = product.gzip_inflate(data, device, chunk, window)
    stats = product.last_reads_gzip()
    print(device, chunk, window, outcome, stats)
    if complete:
        assert outcome == "done"
    assert outcome in ("done", "too few starts")
    assert got == (payload if outcome == "done" else b"")
    return outcome, stats


def test_designs_are_what_zlib_reads():
    G.self_check()


def test_zlib_is_device_minus_one(product):
    got, outcome = product.gzip_inflate(G.fastq_gz(6), -1)
    assert (got, outcome) == (G.fastq_text(), "done")


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("level", LEVELS)
def test_fastq_text(product, level, chunk, window):
    data, payload = G.fastq_gz(level), G.fastq_text()
    outcome, st = inflate_checked(product, data, payload, -2, chunk, window, must_complete(chunk, window))
    if outcome != "done":
        return
    assert st["members"] == 1
    if window == 0:  # (a shorter window ends at its last start, in the middle of a chunk, which then counts for neither)
        assert st["chunks"] == -(-(len(data) - 18) // chunk)
    if chunk == 65536:
        assert st["absorbed"] <= 2  # (one wave doing everything would pass the bytes, not this)
    if chunk == 4096:
        assert st["absorbed"] > st["chunks"] // 2 and st["starts_found"] >= 20


def check_design_stats(st, starts, chunk, n_file):
    want = G.model_found(starts, chunk, n_file - 18)
    assert st["starts_found"] == len(want), (st, sorted(want))
    assert st["absorbed"] == st["chunks"] - 1 - len(want)


@pytest.mark.parametrize("chunk,window", [(4096, 0), (4096, 17), (16384, 0), (65536, 0)])
def test_history_across_chunks(product, chunk, window):
    """distances 32 768, 32 767 and 1 on a chunk's first byte, sources that cross into the chunk in front, chunks that give
    exactly 32 768, 32 767, 100 and no bytes: gzip_cases.history_design"""
    data, payload, starts, notes = G.history_design()
    found = G.model_found(starts, G.CH, len(data) - 18)
    # the design holds: every named block is the first start of a chunk of its own
    assert all(starts[i] in found.values() for i in notes.values())
    outcome, st = inflate_checked(product, data, payload, -2, chunk, window, True)
    if window == 0:
        check_design_stats(st, starts, chunk, len(data))


@pytest.mark.parametrize("window", [0, 3])
def test_markers_of_markers(product, window):
    data, payload, starts = G.relay_design()
    assert len(G.model_found(starts, 16384, len(data) - 18)) >= 6
    outcome, st = inflate_checked(product, data, payload, -2, 16384, window, True)
    if window == 0:
        check_design_stats(st, starts, 16384, len(data))


@pytest.mark.parametrize("name,data,payload,members", G.member_cases(), ids=[c[0] for c in G.member_cases()])
@pytest.mark.parametrize("window", [0, 4])
def test_members(product, name, data, payload, members, window):
    outcome, st = inflate_checked(product, data, payload, -2, 4096, window, True)
    assert st["members"] == members


@pytest.mark.parametrize("name,data,payload", G.startless_cases(), ids=[c[0] for c in G.startless_cases()])
def test_no_usable_start(product, name, data, payload):
    """stored, fixed, one dynamic block: a window behind which the file goes on cannot hand it on; the whole file in one
    window is one chunk's work and right (the loader's rule of a quarter gives such a file to zlib: the GPU tests)"""
    got, outcome = product.gzip_inflate(data, -2, 4096, 2)
    assert (got, outcome) == (b"", "too few starts")
    got, outcome = product.gzip_inflate(data, -2, 4096, 0)
    assert (got, outcome) == (payload, "done") and product.last_reads_gzip()["starts_found"] == 0


@pytest.mark.parametrize("name,data,payload", G.flushed_cases(), ids=[c[0] for c in G.flushed_cases()])
def test_flushed_streams(product, name, data, payload):
    outcome, st = inflate_checked(product, data, payload, -2, 4096, 4, True)
    assert st["starts_found"] * 2 >= st["chunks"]


def test_a_false_start_is_a_boundary_mismatch(product):
    data, payload, false_bit = G.false_start_design()
    got, outcome = product.gzip_inflate(data, -2, 4096, 0)
    assert (got, outcome) == (b"", "boundary mismatch")
    # (chunks so large that the image is no chunk's first candidate: the file is fine)
    assert product.gzip_inflate(data, -2, 65536, 0) == (payload, "done")


def test_a_full_slot(product, monkeypatch):
    data, payload = G.repeated_line()
    monkeypatch.setenv("G2S_GZIP_SLOT_RATIO", "8")
    assert product.gzip_inflate(data, -2, 4096, 0) == (b"", "slot full")
    monkeypatch.setenv("G2S_GZIP_SLOT_RATIO", "1024")
    assert product.gzip_inflate(data, -2, 4096, 0) == (payload, "done")


@pytest.mark.parametrize("how", ["truncated", "flipped-deflate-byte", "flipped-crc-byte"])
def test_damage_is_given_back(product, how):
    data = G.damaged(G.small_blocks_gz(G.fastq_text()[:150000]), how)
    got, outcome = product.gzip_inflate(data, -2, 4096, 0)
    assert got == b"" and outcome in ("corrupt", "trailer", "boundary mismatch")
    with pytest.raises(product.G2SError):
        product.gzip_inflate(data, -1)


def test_the_mode_is_a_switch(product, monkeypatch, tmp_path):
    """asking returns the previous mode, and the host loader keeps its route whatever is asked"""
    import fastx_model as M
    old = product.set_device_gzip(1)
    try:
        assert old == -1 and product.set_device_gzip(0) == 1 and product.set_device_gzip(1) == 0
        monkeypatch.setenv("G2S_HOST_BUILD", "1")
        path = tmp_path / "reads.fq.gz"
        path.write_bytes(G.small_blocks_gz(M.fastq(M.base_reads()[1])))
        product.Graph.from_files(str(path), 31, 2).free()
        assert product.last_reads_load()["inflate"] == ["zlib"] and product.last_reads_gzip()["files"] == 0
    finally:
        product.set_device_gzip(-1)
