#!/bin/bash
# Packing variants of the lexicon scoring kernel for scripts/lexicon_bench.py: -DLEX_PACK=0 one word per wave, 1 two words per wave where both have
# S <= 32, 2 also four words per wave where all have S <= 16.  The product library is built with the default in csrc/lexicon.hip.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
O=$ROOT/scripts/_trace; mkdir -p $O
cd $ROOT/crnn-ocr-lite_amd/csrc
for k in 0 1 2; do
  hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -I $ROOT/include -DLEX_PACK=$k lexicon.hip -o $O/liblex_pack$k.so
done
ls -la $O/liblex_pack*.so
