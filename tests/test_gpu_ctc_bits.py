"""-m gpu test: the softmax, CTC loss, lexicon, alignment and decode entry points give the bits recorded in tests/golden/ctc_bits.npz.

The loss, lexicon and alignment kernels take their arithmetic from one header (csrc/ctc_core.h), so the tests that hold them against each other
cannot see a mistake they share.  The fixture was recorded by tests/golden/make_ctc_bits.py from the last commit at which each kernel carried its
own copy; it holds outputs only, the inputs come from the seeds of tests/lexicon_ref.py.  Bits are compared as int32, NaN patterns included.  The
fixture belongs to the compiler it was recorded with (stored in the file and printed when something differs): another compiler may round expf /
logf differently, and then the fixture is to be recorded again from a commit known to be good -- not skipped."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLD_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _generator():
    spec = importlib.util.spec_from_file_location("make_ctc_bits", os.path.join(GOLD_DIR, "make_ctc_bits.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def test_every_recorded_output_has_the_same_bits():
    gen = _generator()
    gold, recorded_with = gen.load(os.path.join(GOLD_DIR, "ctc_bits.npz"))
    got = gen.arrays()
    assert sorted(got) == sorted(gold)
    assert len(got) == 4 * (13 + 2 * 12 + 5)                  # per alphabet: 13 softmax arrays, 12 per skip, 5 of the decoders
    differ = []
    for name in sorted(got):
        a, b = got[name], gold[name]
        if a.dtype != b.dtype or a.shape != b.shape or not np.array_equal(gen.bits(a), gen.bits(b)):
            n = int((gen.bits(a) != gen.bits(b)).sum()) if a.shape == b.shape and a.dtype == b.dtype else -1
            differ.append("%s (%d of %d elements)" % (name, n, b.size))
    assert not differ, "bits differ from the fixture in %d of %d arrays: %s\nfixture recorded with:\n%s\nthis machine:\n%s" % (
        len(differ), len(got), "; ".join(differ), recorded_with, gen.hipcc_version())

