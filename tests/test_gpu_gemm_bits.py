"""The tile GEMM entry points give the bits recorded in tests/golden/gemm_bits.npz.

The tile GEMM is what the `*_equals_the_tile_kernel` tests hold the faster kernels against, and the tests of the tile kernels themselves
compare with torch to a tolerance, so neither sees a change of a few bits in it.  The fixture was recorded by tests/golden/make_gemm_bits.py
from commit 137e5be, the last one at which the fp32, bf16 and plane kernels shared one translation unit and a positional launcher; it holds
outputs only (small ones whole, larger ones as a sha256 and their first 16 words) and the return code of every call, refused ones included.
The inputs come from seeds.  The fixture belongs to the compiler it was recorded with (stored in the file and printed when something
differs): with another compiler it is to be recorded again from a commit known to be good -- not skipped."""
import importlib.util
import os

import numpy as np
import pytest

GOLD_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLD_DIR, "gemm_bits.npz")


def _generator():
    spec = importlib.util.spec_from_file_location("make_gemm_bits", os.path.join(GOLD_DIR, "make_gemm_bits.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def test_the_fixture_holds_every_case_of_the_generator():
    gen = _generator()
    gold, _ = gen.load(FIXTURE)
    assert os.path.getsize(FIXTURE) < gen.MAX_BYTES
    names = [n for n, _, _ in gen.cases()]
    assert len(names) == len(set(names)) == 658
    assert sorted(n + " code" for n in names) == sorted(k for k in gold if k.endswith(" code"))
    for n in names:                                           # every case recorded at least one output beside its return code
        assert any(k.startswith(n + " ") and not k.endswith(" code") for k in gold), n
    refused = [n for n in names if n.startswith("refused")]
    assert len(refused) == 32 and all(int(gold[n + " code"][0]) in (gen.ERR_ARG, gen.ERR_UNSUPPORTED) for n in refused)
    assert all(int(gold[n + " code"][0]) == 0 for n in names if not n.startswith("refused"))


@pytest.mark.gpu
def test_every_recorded_output_has_the_same_bits():
    gen = _generator()
    gold, recorded_with = gen.load(FIXTURE)
    got = {k: gen.summary(a) for k, a in gen.arrays().items()}
    assert sorted(got) == sorted(gold)
    differ = []
    for name in sorted(got):
        a, b = got[name], gold[name]
        if not gen.same(a, b):
            if isinstance(a, tuple) and isinstance(b, tuple):
                differ.append("%s (digest; first words %s, recorded %s)" % (name, a[1][:4].tolist(), b[1][:4].tolist()))
            elif isinstance(a, tuple) or isinstance(b, tuple) or a.shape != b.shape:
                differ.append("%s (size)" % name)
            else:
                differ.append("%s (%d of %d words)" % (name, int((a != b).sum()), b.size))
    assert not differ, "bits differ from the fixture in %d of %d arrays: %s\nfixture recorded with:\n%s\nthis machine:\n%s" % (
        len(differ), len(got), "; ".join(differ[:40]), recorded_with, gen.hipcc_version())
