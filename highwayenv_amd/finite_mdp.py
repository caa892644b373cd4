"""Host side of ``to_finite_mdp`` (the reference's envs/common/finite_mdp.py:17-101): the tables of the deterministic MDP over a
time-to-collision grid that came from the device (csrc/hwy_ttc.h), built in numpy for ONE environment -- what the reference hands
to ``finite_mdp.mdp.DeterministicMDP``.  No ``finite_mdp`` package is needed: ``FiniteMDP`` carries the same attributes.

The planner kernel solves this MDP without ever materialising the tables; they exist for the reference's host-side planners
(value iteration, MCTS, robust planners) that take ``env.to_finite_mdp()``.
"""
from __future__ import annotations

import numpy as np

NUM_ACTIONS = 5  # DiscreteMetaAction.ACTIONS_ALL: LANE_LEFT, IDLE, LANE_RIGHT, FASTER, SLOWER


class FiniteMDP:
    """``finite_mdp.mdp.DeterministicMDP(transition, reward, terminal, state=state)`` plus ``original_shape``, as attributes."""

    def __init__(self, transition, reward, terminal, state, original_shape):
        self.transition = transition          # int [S, 5]: next state of (state, action)
        self.reward = reward                  # f64 [S, 5]
        self.terminal = terminal              # bool [S]
        self.state = state                    # raveled (speed_index, lane, 0)
        self.original_shape = original_shape  # (V, L, T)

    def value_iteration(self, gamma: float = 1.0):
        """The fixed point of V <- max_a(reward + gamma * where(terminal, 0, V[transition])) (T + 1 sweeps from zeros reach it:
        every transition raises the time index) and its Q table [S, 5]."""
        value = np.zeros(self.reward.shape[0])
        for _ in range(self.original_shape[2] + 1):
            q = self.reward + gamma * np.where(self.terminal[:, None], 0.0, value[self.transition])
            value = q.max(axis=1)
        return value, q


def transition_table(shape) -> np.ndarray:
    """transition_model / clip_position (finite_mdp.py:166-203) for every (state, action): IDLE moves one time step on, LANE_LEFT /
    LANE_RIGHT also change the lane, FASTER / SLOWER also change the speed index at time 0 only; everything clipped to the grid."""
    V, L, T = shape
    h, i, j = np.meshgrid(np.arange(V), np.arange(L), np.arange(T), indexing="ij")
    dh = np.zeros((V, L, T, NUM_ACTIONS), int)
    di = np.zeros((V, L, T, NUM_ACTIONS), int)
    di[..., 0], di[..., 2] = -1, 1
    dh[..., 3], dh[..., 4] = (j == 0), -(j == 0).astype(int)
    nh = np.clip(h[..., None] + dh, 0, V - 1)
    ni = np.clip(i[..., None] + di, 0, L - 1)
    nj = np.clip(j[..., None] + 1, 0, T - 1) + np.zeros_like(dh)
    return np.ravel_multi_index((nh, ni, nj), shape).reshape(V * L * T, NUM_ACTIONS)


def build(grid: np.ndarray, speed_index: int, lane: int, config: dict) -> FiniteMDP:
    """The MDP of finite_mdp.py:47-97 over ``grid`` f64 [V, L, T] for a vehicle at (speed_index, lane): the reward table is evaluated
    left to right like the reference's expression, so it carries the same bits."""
    grid = np.asarray(grid, np.float64)
    V, L, T = grid.shape
    state = int(np.ravel_multi_index((speed_index, lane, 0), grid.shape))
    lanes = np.arange(L) / max(L - 1, 1)
    speeds = np.arange(V) / max(V - 1, 1)
    state_reward = (config["collision_reward"] * grid + config["right_lane_reward"] * (lanes[None, :, None] + np.zeros_like(grid))
                    + config["high_speed_reward"] * (speeds[:, None, None] + np.zeros_like(grid)))
    lcr = config.get("lane_change_reward", 0)
    action_reward = np.array([lcr, 0, lcr, 0, 0], np.float64)
    reward = np.ravel(state_reward)[:, None] + action_reward[None, :]
    terminal = np.ravel((grid == 1) | (np.arange(T) == T - 1)[None, None, :])
    return FiniteMDP(transition_table(grid.shape), reward, terminal, state, grid.shape)
