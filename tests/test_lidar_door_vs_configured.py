"""The Lidar door against the configured LidarObservation: every fixture of the EXISTING tests/golden/lidar (the highway scenario:
IDM, Linear and direct-control families, two agents, N = 101, crashes, the hand-placed roads) run through the door on an engine
configured with **Kinematics**.  The result must equal the fixture's ``obs0`` / ``obs`` under the project's criterion (float32,
shape, finite, zero cells off by more than 1e-6) and be BIT FOR BIT (uint32 view) what a Lidar-configured engine's own kernel
(csrc/hwy_lidar.h) writes for the same state: the arithmetic is the same statement for statement.  On the emulation and on the GPU.
Cells > 64 have no such twin; they are held to ``door_cells`` (tests/test_lidar_door_parity.py)."""
import numpy as np
import pytest

from highwayenv_amd import _abi
from tests import lidar_door_util as U
from tests.lidar_util import FIXTURES, LidarGolden


@pytest.mark.parametrize("backend", U.BACKENDS)
@pytest.mark.parametrize("name", FIXTURES)
def test_door_on_a_kinematics_engine_is_the_configured_trace(backend, name):
    g = LidarGolden(name)
    lidar_cfg = g.hwy_config()
    obs = g.config["observation"]
    inner = obs.get("observation_config", obs)
    params = _abi.lidar_door_params(inner.get("cells", 16), inner.get("maximum_range", 60), inner.get("normalize", True))
    assert (params.cells, params.maximum_range, params.normalize) == (lidar_cfg.lidar_cells, lidar_cfg.lidar_max_range, lidar_cfg.lidar_normalize)
    k = LidarGolden(name)
    k.config["observation"] = {"type": "Kinematics"} if g.A == 1 else {"type": "MultiAgentObservation", "observation_config": {"type": "Kinematics"}}
    kin_cfg = k.hwy_config()
    assert kin_cfg.obs_type == _abi.OBS_KINEMATICS and lidar_cfg.obs_type == _abi.OBS_LIDAR
    door, twin = U.make_engine(backend, kin_cfg), U.make_engine(backend, lidar_cfg)
    for index in [None] + list(range(g.steps)):
        prefix = "init" if index is None else "step"
        k.load(door, prefix, index)
        g.load(twin, prefix, index)
        got = door.lidar_observe(params)
        U.assert_same(got, g.reference_obs(index), f"{name} {prefix} {index} [{backend}]")
        own = np.ascontiguousarray(twin.observe())
        assert own.dtype == np.float32 and own.shape == got.shape
        np.testing.assert_array_equal(np.ascontiguousarray(got).view(np.uint32), own.view(np.uint32),
                                      err_msg=f"{name} {prefix} {index} [{backend}]: the door and the configured kernel differ in a bit")
        # ... and the door on the Lidar-configured engine itself: next to the configured type, the same bits
        np.testing.assert_array_equal(np.ascontiguousarray(twin.lidar_observe(params)).view(np.uint32), own.view(np.uint32))
    door.close()
    twin.close()
