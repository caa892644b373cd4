"""The committed fixtures under tests/golden are what the committed generators produce from the UNMODIFIED reference.

Every generator records, next to each fixture it writes, a digest of the fixture's arrays and of the sources that made it
(tests/golden/MANIFEST.json, tests/golden_util.record_fixture).  Everywhere, every committed fixture is held to its entry: a
fixture edited by hand, or a generator edited without regenerating what it makes, fails here.  Where the reference package is
installed (oracle/ref_stub.py), env 0 of every fixture is also regenerated and compared with the committed file, array by array,
bit for bit (the recorded traces of tests/golden/live and the shortest paths: whole).

The planner's fixtures (tests/golden/ttc, with a manifest of their own next to them) are held the same way: every committed file
to its digest, and env 0 regenerated where the reference is installed."""
import importlib.util
import json
import os

import numpy as np
import pytest

from oracle import ref_stub
from tests import golden_util

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MANIFEST = golden_util.load_manifest()
_mods = {}


def _generator(fname):
    if fname not in _mods:
        spec = importlib.util.spec_from_file_location(fname[:-3], os.path.join(GOLDEN, fname))
        _mods[fname] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(_mods[fname])
    return _mods[fname]


def _assert_bits_equal(a, b, k):
    assert a.dtype == b.dtype, (k, a.dtype, b.dtype)
    if a.dtype.kind == "f":
        np.testing.assert_array_equal(a.view(np.uint64 if a.dtype == np.float64 else np.uint32),
                                      b.view(np.uint64 if b.dtype == np.float64 else np.uint32), err_msg=k)  # bits, NaNs included
    else:
        np.testing.assert_array_equal(a, b, err_msg=k)


def _regenerated_env0_matches(fname, name, z):
    gen = _generator(fname)
    sc = next(s for s in gen.SCENARIOS if s["name"] == name)
    fresh = gen.run_scenario(sc, only_envs=[0])
    assert set(fresh) == set(z.files), sorted(set(fresh) ^ set(z.files))
    n_arrays = 0
    for k, a in fresh.items():
        a, b = np.asarray(a), z[k]
        if k == "meta":
            a, b = a[1:], b[1:]   # (meta[0] = number of envs)
        elif a.shape != b.shape:  # the env axis: the committed array holds all envs (or the first `frames_for`), the fresh one env 0
            diff = [ax for ax in range(a.ndim) if a.shape[ax] != b.shape[ax]]
            assert a.ndim == b.ndim and len(diff) == 1 and a.shape[diff[0]] == 1, (k, a.shape, b.shape)
            b = np.take(b, [0], axis=diff[0])
        _assert_bits_equal(a, b, k)
        n_arrays += 1
    assert n_arrays > 40


def _regenerated_whole_matches(entry, name, z):
    if entry["path"].endswith(".json"):
        gen = _generator("make_golden_routes.py")
        fresh = golden_util.json_fixture_arrays(gen.shortest_paths())
    else:
        gen = _generator("make_golden_live.py")
        fresh = gen.run_scenario(next(s for s in gen.SCENARIOS if s["name"] == name))
    assert set(fresh) == set(z.files if hasattr(z, "files") else z), name
    for k, a in fresh.items():
        assert np.asarray(a).shape == z[k].shape, (k, np.asarray(a).shape, z[k].shape)
        _assert_bits_equal(np.asarray(a), z[k], k)


@pytest.mark.parametrize("name", sorted(MANIFEST))
def test_env0_of_the_committed_fixture_is_what_the_generator_makes(name):
    entry = MANIFEST[name]
    z = golden_util.fixture_arrays(entry["path"])
    regenerate = f"regenerate it with `python tests/golden/{os.path.basename(entry['sources'][0])} {name}` (needs the reference)"
    assert golden_util.arrays_digest(z) == entry["arrays_sha256"], f"{entry['path']} is not what its generator wrote: {regenerate}"
    assert golden_util.sources_digest(entry["sources"]) == entry["sources_sha256"], \
        f"{' / '.join(entry['sources'])} changed since {entry['path']} was made: {regenerate}"
    if not ref_stub.reference_available():
        return   # (the digests above are what a checkout without the reference can hold the fixture to)
    fname = os.path.basename(entry["sources"][0])
    if fname in ("make_golden.py", "make_golden_merge.py", "make_golden_intersection.py"):
        names = {s["name"] for f in ("make_golden.py", "make_golden_merge.py", "make_golden_intersection.py")
                 for s in _generator(f).SCENARIOS}
        assert names <= set(MANIFEST), f"scenarios without a committed fixture: {sorted(names - set(MANIFEST))}"
        _regenerated_env0_matches(fname, name, z)
    else:
        _regenerated_whole_matches(entry, name, z)


# ---- tests/golden/ttc: the time-to-collision grid / finite-MDP fixtures (make_golden_ttc.py, its own MANIFEST.json) ------------
TTC = os.path.join(GOLDEN, "ttc")
with open(os.path.join(TTC, "MANIFEST.json")) as _f:
    TTC_MANIFEST = json.load(_f)


def _ttc_digest(z):  # (make_golden_control.digest restated: the generator imports the reference)
    import hashlib
    h = hashlib.sha256()
    for k in sorted(z.files):
        a = z[k]
        h.update(k.encode())
        h.update(str(a.dtype).encode() + str(a.shape).encode())
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def test_every_ttc_fixture_has_a_manifest_entry():
    from tests.ttc_util import FIXTURES
    assert sorted(TTC_MANIFEST) == sorted(FIXTURES) == sorted(f[:-4] for f in os.listdir(TTC) if f.endswith(".npz"))


@pytest.mark.parametrize("name", sorted(TTC_MANIFEST))
def test_env0_of_the_committed_ttc_fixture_is_what_the_generator_makes(name):
    with np.load(os.path.join(TTC, name + ".npz")) as z:
        assert _ttc_digest(z) == TTC_MANIFEST[name], \
            f"ttc/{name}.npz is not what its generator wrote: regenerate it with `python tests/golden/ttc/make_golden_ttc.py {name}`"
        if not ref_stub.reference_available():
            return
        gen = _generator(os.path.join("ttc", "make_golden_ttc.py"))
        assert set(gen.NAMES) == set(TTC_MANIFEST), f"scenarios without a committed fixture: {sorted(set(gen.NAMES) ^ set(TTC_MANIFEST))}"
        fresh = gen.generate(name, only_envs={0})
        assert set(fresh) == set(z.files), sorted(set(fresh) ^ set(z.files))
        for k, a in fresh.items():
            a, b = np.asarray(a), z[k]
            if k == "meta":
                a, b = a[1:], b[1:]   # (meta[0] = number of envs)
            elif a.shape != b.shape:  # the env axis: the committed array holds all envs, the fresh one env 0
                diff = [ax for ax in range(a.ndim) if a.shape[ax] != b.shape[ax]]
                assert a.ndim == b.ndim and len(diff) == 1 and a.shape[diff[0]] == 1, (k, a.shape, b.shape)
                b = np.take(b, [0], axis=diff[0])
            _assert_bits_equal(a, b, k)
