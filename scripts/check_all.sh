#!/usr/bin/env bash
# One-command verification (no GPU needed): build all extensions, run the
# CPU protocol suite, then the ASAN/UBSAN and TSAN passes. GPU tiers
# (`pytest -m gpu`, bench.py) run on an MI355X box.
set -euo pipefail
cd "$(dirname "$0")/.."

echo "== build =="
python setup.py build_ext --inplace
python build_hip.py
python build_ffi.py

echo "== CPU suite =="
python -m pytest tests -q -m "not gpu"

echo "== sanitizers =="
# the GPU model encoder's element functions, as a stand-alone host program
mkdir -p build
g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
    -Ixaynet_amd/csrc scripts/model_codec_sanitize.cpp -o build/model_codec_sanitize
build/model_codec_sanitize
# and the decoder's (mc_span / mc_read) over valid, truncated and corrupted words
g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
    -Ixaynet_amd/csrc scripts/model_decode_sanitize.cpp -o build/model_decode_sanitize
build/model_decode_sanitize
# the exact float unmask's element function (ur_round), float and double, L = 1..5
g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
    -Ixaynet_amd/csrc scripts/unmask_round_sanitize.cpp -o build/unmask_round_sanitize
build/unmask_round_sanitize
bash scripts/sanitize.sh
bash scripts/tsan.sh

echo "check_all: OK"
