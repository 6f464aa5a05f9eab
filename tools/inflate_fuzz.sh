#!/bin/bash
# CPU only: builds tools/inflate_fuzz.cpp with AddressSanitizer and UndefinedBehaviorSanitizer and runs it on the
# designed and corrupt members of tests/inflate_cases.py and on seeded random mutations; then gap2seq_amd/csrc/gzip_chunks.h
# (the chunked inflate of plain gzip files, compiled for the host) on the deflate streams of tests/gzip_cases.py's files and
# on M seeded mutations of them.  Usage: tools/inflate_fuzz.sh [N [M]]
set -e
cd "$(dirname "$0")/.."
T=$(mktemp -d)
trap 'rm -rf "$T"' EXIT
${CXX:-c++} -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all tools/inflate_fuzz.cpp -lz -o "$T/inflate_fuzz"
python - "$T" <<'PY'
import os, sys
sys.path.insert(0, "tests")
import inflate_cases as IC
t = sys.argv[1]
open(os.path.join(t, "valid.bgzf"), "wb").write(IC.valid_file()[0])
open(os.path.join(t, "corrupt.bgzf"), "wb").write(b"".join(m for _, m in IC.corrupt_cases()))
open(os.path.join(t, "corpus.bgzf"), "wb").write(IC.random_corpus()[0])
# gzip_cases.py's files as raw deflate streams (cases 1 - 6; the FASTQ text cut to a few blocks, so that a run stays short)
import zlib
import gzip_cases as G
fq = G.fastq_text()[:250000]
streams = [G.raw_deflate(fq, level=lv) for lv in (1, 6, 9)]
for file in (G.history_design()[0], G.relay_design()[0], G.false_start_design()[0]):
    streams.append(file[10:-8])
streams += [G.raw_deflate(fq[:60000], level=6, mem_level=4), G.raw_deflate(b"")]                       # (members)
streams += [G.raw_deflate(fq[:60000], level=0), G.raw_deflate(fq[:60000], strategy=zlib.Z_FIXED)]      # (no usable start)
streams += [G.raw_deflate(fq[:100000], flush_every=10000, flush=f) for f in (zlib.Z_SYNC_FLUSH, zlib.Z_FULL_FLUSH)]
for i, d in enumerate(streams):
    open(os.path.join(t, "stream%02d.deflate" % i), "wb").write(d)
PY
"$T/inflate_fuzz" --mutations "${1:-4000}" "$T/valid.bgzf" "$T/corrupt.bgzf" "$T/corpus.bgzf" --deflate "${2:-300}" "$T"/stream*.deflate
