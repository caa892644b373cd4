"""The Lidar door (csrc/hwy_lidar_door.h) against the UNMODIFIED reference on every scenario family: for every fixture of
tests/golden/lidar_door and every recorded state, ``set_state``, call the door on an engine configured with Kinematics, compare with
the reference's ``LidarObservation`` of that state -- float32, same shape, every value finite, ZERO cells off by more than
``OBS_ATOL`` = 1e-6 (tests/lidar_util.py).  All recorded states of a fixture are one batch: E x (steps + 1) environments (at most
39), N = 6 (merge-v0), 43 slots x 4 agents (merge-generic), 32 slots (intersection), 31 (highway); cells 1, 16, 20, 24, 32, 65, 256.

On the ``door_ix*`` fixtures the yardstick after a step is the recorded ``observation_type.observe()`` called AFTER ``step()``:
``IntersectionEnv.step`` observes BEFORE ``_clear_vehicles()`` / ``_spawn_vehicle()`` (intersection_env.py:136-140), the door sees
the list AFTER them.  That the fixtures really hold such a step is asserted here too."""
import numpy as np
import pytest

from highwayenv_amd import _abi
from tests import lidar_door_util as U

_cases = {}


def case(name: str) -> U.DoorCase:
    if name not in _cases:
        _cases[name] = U.DoorCase(name)
    return _cases[name]


@pytest.mark.parametrize("backend", U.BACKENDS)
@pytest.mark.parametrize("name", U.FIXTURES)
def test_every_recorded_state_vs_reference(backend, name):
    c = case(name)
    eng = c.engine(backend)
    c.check(eng, backend)
    eng.close()


@pytest.mark.parametrize("name", U.IX)
def test_intersection_fixtures_hold_the_documented_difference(name):
    """At least one recorded step whose ``step()`` observation differs from ``observe()`` called after it, and at least one step
    at which the list shrinks or grows: the reason why ``HighwayVectorEnv(lidar_observation=...)`` refuses the intersection ids."""
    d = U.arrays(name)
    differs = np.abs(d["obs"].astype(np.float64) - d["observe"]).max(axis=(2, 3, 4)) > U.OBS_ATOL  # [steps, E]
    assert differs.any()
    counts = np.concatenate([d["init_present"].sum(-1)[None], d["next_present"].sum(-1)])
    assert (np.diff(counts, axis=0) != 0).any()
    # ... and where the list did not change within range, the two agree: the difference is the list, not the kernel
    assert (~differs).any()


def test_crafted_roads_are_what_they_are_for():
    """door_crafted on the reference's own answer: the Obstacle wins the tie of road 0 (it is traced last), the absent slot of road 7
    is not hit, the Obstacle beyond the range of road 4 is skipped and the one within it (road 5) traced, road 6 holds a negative
    centre distance."""
    d = U.arrays("door_crafted")
    o = d["obs0"][:, 0]
    assert d["ties"].tolist()[:2] == [1, 1]
    assert o[0, 0].tolist() == [30.0, -25.0]
    assert (o[4] == 60.0).all() and (o[5] != 60.0).any()
    assert o[6].min() < 0
    assert o[7, 0].tolist() == [27.5, -5.0] and d["init_present"][7].tolist() == [1, 1, 0, 1, 1, 1]
    assert (d["init_obstacle"][:, -1] == 1).all() and d["margins"].min() >= 1e-9


@pytest.mark.parametrize("backend", U.BACKENDS)
def test_pass_boundary_and_a_lone_observer(backend):
    """N = 1 (nothing to trace: every cell at the range), and N = 64 / 65 (one pass / two passes of 64 obstacles): the same vehicles
    in the same order give the same trace, whatever N pads them to -- the extra slots stand beyond the range."""
    c = case(U.CELLS)
    g, p = c.g, c.params[2]  # 256 cells
    one = dict(g.config, vehicles_count=0)
    eng = U.make_engine(backend, _abi.make_config(one, 2, fast=True))
    st = _abi.alloc_state(2, 1)
    st["x"][...], st["y"][...], st["speed"][...] = 100.0, 4.0, 25.0
    st["flags"][...] = _abi.F_CONTROLLED
    eng.set_state(st)
    alone = eng.lidar_observe(p)
    assert alone.shape == (2, 1, 256, 2) and (alone == np.float32(1.0)).all()
    eng.close()
    base = g.state("init")
    want = c.data["obs0_c256"]
    for n in (64, 65):
        cfg = _abi.make_config(dict(g.config, vehicles_count=n - 1), g.E, fast=True)
        st = _abi.alloc_state(g.E, n)
        assert int(cfg.agent_index[0]) == 0  # (the ego is slot 0, as in the fixture's 31)
        for k in st:
            if k != "time":
                st[k][:, :g.N] = base[k]
        st["x"][:, g.N:] = 1e5 + 10.0 * np.arange(n - g.N)  # beyond every range
        st["flags"][:, g.N:] = _abi.F_CHECK_COLLISIONS
        eng = U.make_engine(backend, cfg)
        eng.set_state(st)
        U.assert_same(eng.lidar_observe(p), want, f"N={n} {backend}")
        eng.close()
