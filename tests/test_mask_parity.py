"""The action-mask kernel (csrc/hwy_mask.h) against the reference's ``get_available_actions()``: every recorded state of every
fixture of tests/golden/masks is written onto the engine (teacher-forced) and the kernel's table must equal the reference's
exactly -- on the CPU emulation of the kernel source and, marked ``gpu``, on the MI355X.  The generator keeps every recorded
controlled vehicle 1e-6 from the thresholds of ``is_reachable_from``, so nothing hangs on rounding."""
import numpy as np
import pytest

from highwayenv_amd import _abi
from tests import mask_util
from tests.mask_util import BACKENDS, FIXTURES, MaskGolden


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_masks(name, backend):
    g = MaskGolden(name)
    cfg = g.hwy_config()
    assert (cfg.num_vehicles, cfg.num_agents, _abi.num_actions(cfg)) == (g.N, g.A, g.n_ids)
    eng = mask_util.make_engine(backend, cfg)
    for index in g.indices():
        eng.set_state(g.state(index))
        got = eng.action_mask()
        assert got.dtype == bool and got.shape == (g.E, g.A, g.n_ids)
        np.testing.assert_array_equal(got, g.mask(index), err_msg=f"{name}: state {index}")


def test_fixtures_cover_what_they_are_for():
    """The properties the fixtures were recorded for hold in the reference's own tables."""
    def table(name):
        g = MaskGolden(name)
        return np.concatenate([g.mask(i)[None] for i in g.indices()]).reshape(-1, g.n_ids), g
    m, _ = table("mask_lanes1")
    assert not m[:, 0].any() and not m[:, 2].any() and m[:, 1].all()            # one lane: no lane action, ever
    m, _ = table("mask_speeds2")
    assert not (m[:, 3] & m[:, 4]).any() and (m[:, 3] | m[:, 4]).all()          # two speeds: exactly one of FASTER / SLOWER
    m, _ = table("mask_speeds8")
    assert (m[:, 3] & m[:, 4]).any()
    for name in ("mask_longi", "mask_lat", "mask_intersection", "mask_intersection_ma"):
        m, g = table(name)
        assert g.n_ids == 3 and m[:, 1].all() and not m[:, 0].all() and m[:, 0].any()
    g = MaskGolden("mask_placed")     # (left, 0), (left, top), (right, 0), (right, top) at reset
    np.testing.assert_array_equal(g.mask(None)[:, 0], [[0, 1, 1, 1, 0], [0, 1, 1, 0, 1], [1, 1, 0, 1, 0], [1, 1, 0, 0, 1]])
    # merge-v0: on ("b", "c", 1) the lane to the right exists, is in reach and is forbidden -- LANE_RIGHT stays unavailable, while
    # it is available to the ego of environment 1 on ("b", "c", 0)
    g = MaskGolden("mask_merge")
    tab = __import__("highwayenv_amd.merge", fromlist=["merge"]).table_from_config(g.hwy_config())
    on_bc1 = 0
    for i in g.indices():
        st = g.state(i)
        for e in range(g.E):
            lane = int(st["lane"][e, 0])
            if tab["road_lanes"][lane] == 3 and tab["id"][lane] == 1:
                assert tab["forbidden"][lane + 1] and not g.mask(i)[e, 0, 2]
                on_bc1 += 1
    assert on_bc1 >= 2
    lanes_seen = {int(g.state(i)["lane"][0, 0]) for i in g.indices()}
    assert len({int(tab["road"][k]) for k in lanes_seen}) >= 3                  # a -> b, b -> c and c -> d


def test_direct_control_is_refused():
    from tests.emu import emu
    cfg = _abi.make_config(dict(_abi.highway_fast_default_config(), action={"type": "DiscreteAction"}), 2, fast=True)
    assert emu.mask_status(cfg) == _abi.HWY_ERR_UNSUPPORTED
    with pytest.raises(NotImplementedError):
        emu.EmuEngine(cfg).action_mask()


def _reference_present() -> bool:
    from oracle import ref_stub
    return ref_stub.reference_available()


@pytest.mark.skipif(not _reference_present(), reason="the reference package is not present")
def test_live_reference_random_configurations():
    """Where the reference is present: random configurations run through the generator's own recorder (the unmodified reference,
    its knife-edge assertion included) and compared like the fixtures."""
    from tests.emu import emu
    gen = mask_util.generator()
    rng = np.random.default_rng(2024)
    for k in range(6):
        lanes, n_speeds = int(rng.integers(1, 6)), int(rng.integers(2, 7))
        speeds = (15.0 + np.cumsum(rng.uniform(1.5, 4.0, n_speeds))).round(2).tolist()
        env_id = ["highway-fast-v0", "merge-generic-v0", "merge-v0"][k % 3]
        config = {"action": {"type": "DiscreteMetaAction", "target_speeds": speeds}}
        if env_id != "merge-v0":
            config.update(lanes_count=lanes if env_id == "highway-fast-v0" else min(max(lanes, 2), 4), vehicles_count=int(rng.integers(4, 12)))
        sc = dict(name=f"live{k}", env=env_id, config=config, seeds=[int(s) for s in rng.integers(0, 1000, 2)], steps=8,
                  action_seed=int(rng.integers(0, 1000)))
        g = MaskGolden(sc["name"], gen.run(sc))
        cfg = g.hwy_config()
        for index in g.indices():
            np.testing.assert_array_equal(emu.action_mask(cfg, g.state(index)), g.mask(index), err_msg=f"{sc}: state {index}")


def test_manifest_matches_the_fixtures():
    """MANIFEST.json holds the digest of every fixture's arrays (names, dtypes, shapes and raw bytes in name order)."""
    import hashlib
    import json
    import os
    manifest = json.load(open(os.path.join(mask_util.MASK_DIR, "MANIFEST.json")))
    assert sorted(manifest) == sorted(FIXTURES)
    for name in FIXTURES:
        z, h = MaskGolden(name).z, hashlib.sha256()
        for k in sorted(z):
            a = np.asarray(z[k])
            h.update(k.encode())
            h.update(str(a.dtype).encode() + str(a.shape).encode())
            h.update(np.ascontiguousarray(a).tobytes())
        assert h.hexdigest() == manifest[name], name
