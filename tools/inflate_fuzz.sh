#!/bin/bash
# CPU only: builds tools/inflate_fuzz.cpp with AddressSanitizer and UndefinedBehaviorSanitizer and runs it on the
# designed and corrupt members of tests/inflate_cases.py and on seeded random mutations.  Usage: tools/inflate_fuzz.sh [N]
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
PY
"$T/inflate_fuzz" --mutations "${1:-4000}" "$T/valid.bgzf" "$T/corrupt.bgzf" "$T/corpus.bgzf"
