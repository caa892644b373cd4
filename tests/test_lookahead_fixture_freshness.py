"""The committed fixtures of tests/golden/lookahead are what the committed generator produces from the UNMODIFIED reference: where
the reference package is installed (oracle/ref_stub.py), environment 0 of every fixture is regenerated -- reset, warm-up, one deep
copy per candidate sequence, K steps each -- and compared with the committed file bit for bit.  (Every file is held to its digest in
tests/test_lookahead_host.py, with or without the reference.)"""
import importlib.util
import os
import sys

import numpy as np
import pytest

from oracle import ref_stub
from tests import lookahead_util as lu

needs_reference = [pytest.mark.reference, pytest.mark.skipif(not ref_stub.reference_available(), reason="needs the reference package")]
PER_ENV = ("branch_time", "reward", "terminated", "truncated", "crashed", "returns", "q", "best_action")


def _generator():
    mod = sys.modules.get("make_golden_lookahead")
    if mod is None:
        spec = importlib.util.spec_from_file_location("make_golden_lookahead", os.path.join(lu.DIR, "make_golden_lookahead.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules["make_golden_lookahead"] = mod
        spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("name", [pytest.param(n, marks=needs_reference) for n in lu.FIXTURES])
def test_env0_regenerates_bit_for_bit(name):
    got = _generator().generate(name, only_envs={0})
    with np.load(os.path.join(lu.DIR, name + ".npz")) as z:
        assert set(got) == set(z.files)
        for k in z.files:
            a, b = np.asarray(got[k]), z[k]
            if k.startswith("init_") or k in PER_ENV:
                a, b = a[0], b[0]
            elif k == "meta":
                a, b = a[1:], b[1:]
            assert a.dtype == b.dtype and a.shape == b.shape, k
            np.testing.assert_array_equal(a.view(np.uint64) if a.dtype == np.float64 else a, b.view(np.uint64) if b.dtype == np.float64 else b,
                                          err_msg=k)
