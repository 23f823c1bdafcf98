#!/bin/bash
# Tile variants of the lexicon shortlist's distance kernel for scripts/lexicon_shortlist_bench.py: -DNEAR_WORDS_PER_THREAD=k, a workgroup builds the
# sample's match masks once for 256 k words.  The product library is built with the default in csrc/lexicon_nearest.hip.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
O=$ROOT/scripts/_trace; mkdir -p $O
cd $ROOT/crnn-ocr-lite_amd/csrc
for k in 1 2 8; do
  hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -I $ROOT/include -DNEAR_WORDS_PER_THREAD=$k lexicon_nearest.hip -o $O/libnear_wpt$k.so
done
ls -la $O/libnear_wpt*.so
