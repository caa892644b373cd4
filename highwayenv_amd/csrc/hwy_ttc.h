// hwy_ttc.h -- the time-to-collision grid and the finite-MDP planner of the highway scenario (AbstractEnv.to_finite_mdp,
// envs/common/abstract.py:452-453 -> envs/common/finite_mdp.py:17-203), a kernel of its own.
//
// No step / reset / observe kernel is touched: this kernel is launched on the engine's stream after whatever ran last and reads the
// state planes the Lidar kernel reads (x, heading, speed, the packed words for lane / speed index / flags) and the agent indices.
//
// One 64-wide wavefront per (environment, agent):
//   phase 1, lane == other vehicle, in passes of 64 up to HWY_MAX_VEHICLES: compute_ttc_grid (finite_mdp.py:125-162) restated.  For
//     every speed index v < V the three collision points (0, cost 1), (-margin, 1/2), (+margin, 1/2) give a time to collision, both
//     quantisations int(ttc / tq) and int(ceil(ttc / tq)) are kept where 0 <= time < T, and the cell (v, other's lane, time) takes
//     the maximum cost: an LDS atomic max on a cost code (0, 1 = 1/2, 2 = 1), which does not depend on the order of the vehicles;
//   phase 2: the grid goes to HBM as f32 [V][L][T] (values exactly 0, 1/2, 1), coalesced;
//   phase 3 (PLAN): finite_mdp (:51-90) solved exactly.  Every transition (transition_model / clip_position, :166-203) raises the
//     time index by one, so the fixed point of V <- max_a(reward + gamma * where(terminal, 0, V[transition])) is reached by ONE
//     backward sweep j = T - 1 .. 0 with thread == (speed, lane) state (at most 8 x 16 = 128 states: two per thread), the j + 1
//     slice of V double-buffered in LDS.  At j == 0 the thread that owns the controlled vehicle's state (speed_index, lane, 0) writes
//     Q(state, .) and its first maximum (numpy's argmax).
// Divisions are the IEEE ones (no reciprocal substitutes).  Products and sums that are separate numpy operations in the reference are
// separate statements here, so -ffp-contract=on fuses none of them: the reward table and the value sweep are bit for bit what numpy
// computes from the reference's tables.  The grid is a set of integer decisions on ttc / tq: it equals the reference's wherever no
// candidate sits within rounding of an integer (sin / cos are hwy_math.h's, <= 2 ulp; with headings of exactly 0 the arithmetic is
// the reference's own).
//
// Like hwy_lidar.h this header includes no HIP runtime: hwy_kernels_ttc.hip includes <hip/hip_runtime.h> first, the CPU emulation
// (tests/emu/emu_ttc.cpp) its shim, hip_emu.h.  The launch rule is hwy_launch_units.h's (select_ttc), for both.
#pragma once

#include <stdint.h>
#include <string.h>

#include "../../include/hwy_engine.h"
#include "hwy_device.h"

namespace hwy {

#define HWY_TTC_MARGIN (HWY_VEH_LENGTH / 2 + HWY_VEH_LENGTH / 2)  // other.LENGTH / 2 + vehicle.LENGTH / 2 (finite_mdp.py:130)
#define HWY_TTC_MAX_CELLS (HWY_MAX_TARGET_SPEEDS * HWY_MAX_LANES * HWY_MAX_TTC_STEPS)
#define HWY_TTC_SMALL_CELLS 1024  // the LDS class most configurations fit (highway-fast-v0: 3 x 3 x 10; policy_frequency 5: 3 x 4 x 50)
#define HWY_TTC_STATES (HWY_MAX_TARGET_SPEEDS * HWY_MAX_LANES)

struct TtcParams {
  const double *x, *heading, *speed;  // [E][pitch]
  const int32_t *packed;              // [E][pitch]
  float *grid;                        // [rows][V][L][T], may be null when planning
  int32_t *action;                    // [rows]      (PLAN)
  double *q;                          // [rows][5]   (PLAN, may be null)
  int32_t N, A, pitch, V, L, T;
  int32_t agent_index[HWY_MAX_AGENTS];
  double target_speeds[HWY_MAX_TARGET_SPEEDS];
  double tq, gamma, lane_change_reward;
  double collision_reward, right_lane_reward, high_speed_reward;
};

// host side: what the entry points accept (include/hwy_engine.h: hwy_ttc_params).  Shared by hwy_engine.hip and the CPU emulation.
inline int ttc_validate(const hwy_config &c, const hwy_ttc_params *tp, const char **why) {
  *why = "";
  if (!tp) { *why = "params is NULL"; return HWY_ERR_INVALID_ARG; }
  if (c.scenario != HWY_SCENARIO_HIGHWAY) { *why = "the finite-MDP planner runs on the highway scenario only"; return HWY_ERR_UNSUPPORTED; }
  if (c.ego_control != HWY_EGO_META) {
    *why = "the finite-MDP planner needs a DiscreteMetaAction ego (a plain Vehicle has no target_speeds)";
    return HWY_ERR_UNSUPPORTED;
  }
  if (c.action_set != HWY_ACTIONS_ALL) {
    *why = "the finite-MDP planner needs both action axes (the five-action table)";
    return HWY_ERR_UNSUPPORTED;
  }
  if (!(tp->time_quantization > 0) || !(tp->time_quantization < 1e30) || !(tp->horizon >= 0) || !(tp->horizon < 1e30)) {
    *why = "horizon and time_quantization must be finite, time_quantization positive";
    return HWY_ERR_INVALID_ARG;
  }
  if (tp->time_steps < 1 || tp->time_steps > HWY_MAX_TTC_STEPS) { *why = "time_steps must be in [1,64]"; return HWY_ERR_INVALID_ARG; }
  const double steps = tp->horizon / tp->time_quantization;  // int(horizon / time_quantization)
  if (!(steps < HWY_MAX_TTC_STEPS + 1) || (int32_t)steps != tp->time_steps) {
    *why = "time_steps is not int(horizon / time_quantization)";
    return HWY_ERR_INVALID_ARG;
  }
  if (!(tp->gamma > -1e30 && tp->gamma < 1e30) || !(tp->lane_change_reward > -1e30 && tp->lane_change_reward < 1e30)) {
    *why = "gamma and lane_change_reward must be finite";
    return HWY_ERR_INVALID_ARG;
  }
  return HWY_OK;
}

// host side: the arguments of a config over the planes the kernel reads ([E][pitch] each) and the outputs
inline TtcParams ttc_params(const hwy_config &c, const hwy_ttc_params &tp, const double *x, const double *heading, const double *speed,
                            const int32_t *packed, int pitch, float *grid, int32_t *action, double *q) {
  TtcParams p;
  memset(&p, 0, sizeof p);
  p.x = x; p.heading = heading; p.speed = speed;
  p.packed = packed;
  p.grid = grid; p.action = action; p.q = q;
  p.N = c.num_vehicles; p.A = c.num_agents; p.pitch = pitch;
  p.V = c.num_target_speeds; p.L = c.lanes_count; p.T = tp.time_steps;
  for (int a = 0; a < HWY_MAX_AGENTS; ++a) p.agent_index[a] = a < c.num_agents ? c.agent_index[a] : 0;
  for (int v = 0; v < HWY_MAX_TARGET_SPEEDS; ++v) p.target_speeds[v] = c.target_speeds[v];
  p.tq = tp.time_quantization; p.gamma = tp.gamma; p.lane_change_reward = tp.lane_change_reward;
  p.collision_reward = c.collision_reward; p.right_lane_reward = c.right_lane_reward; p.high_speed_reward = c.high_speed_reward;
  return p;
}
inline int ttc_cells(const hwy_config &c, const hwy_ttc_params &tp) { return c.num_target_speeds * c.lanes_count * tp.time_steps; }

// utils.not_zero (utils.py:50-56), eps = 1e-2
__device__ inline double ttc_not_zero(double x) {
  const double eps = 1e-2;
  if (fabs(x) > eps) return x;
  return x >= 0 ? eps : -eps;
}
// grid[speed_index, lane, time] = np.maximum(grid[speed_index, lane, time], cost) on the cost code
__device__ inline void ttc_mark(int32_t *cells, int index, int32_t code) {
  __hip_atomic_fetch_max(&cells[index], code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ inline double ttc_cost(int32_t code) { return code == 2 ? 1.0 : (code == 1 ? 0.5 : 0.0); }

// CELLS: capacity of the grid in LDS (one dword per cell); PLAN: phase 3
template <int CELLS, bool PLAN>
__global__ void __launch_bounds__(64) hwy_ttc_kernel(const TtcParams p) {
  __shared__ int32_t sh_cell[CELLS];
  __shared__ double sh_value[PLAN ? 2 : 1][PLAN ? HWY_TTC_STATES : 1];
  const int lane = threadIdx.x;
  const int e = (int)blockIdx.x / p.A, a = (int)blockIdx.x % p.A;
  const size_t row = (size_t)e * p.pitch;
  const int me = p.agent_index[a];
  const int V = p.V, L = p.L, T = p.T;
  const int cells = V * L * T;
  for (int k = lane; k < cells; k += 64) sh_cell[k] = 0;  // np.zeros((V, L, T))
  __syncthreads();

  // ---- phase 1: lane == other vehicle ------------------------------------------------------------------------------------------
  const double ex = p.x[row + me];
  double esn, ecs;
  sincos_bounded(p.heading[row + me], &esn, &ecs);  // vehicle.direction
  const double horizon_steps = (double)T;
  for (int base = 0; base < p.N; base += 64) {
    const int j = base + lane;
    if (j >= p.N || j == me) continue;
    const int32_t w = p.packed[row + j];
    const int other_lane = word_lane(w);
    if ((word_flags(w) & HWY_F_ABSENT) || other_lane >= L) continue;
    const double ospeed = p.speed[row + j];
    double osn, ocs;
    sincos_bounded(p.heading[row + j], &osn, &ocs);
    // np.dot(other.direction, vehicle.direction)
    const double d0 = ocs * ecs;
    const double d1 = osn * esn;
    const double dot = d0 + d1;
    const double projected = ospeed * dot;          // other_projected_speed
    const double gap = p.x[row + j] - ex;           // vehicle.lane_distance_to(other): direction is exactly (1, 0)
    for (int v = 0; v < V; ++v) {
      const double ego_speed = p.target_speeds[v];  // vehicle.index_to_speed(speed_index)
      if (ego_speed == ospeed) continue;
      const double closing = ttc_not_zero(ego_speed - projected);
      const int cell0 = (v * L + other_lane) * T;
      for (int m = 0; m < 3; ++m) {                 // collision_points = [(0, 1), (-margin, 0.5), (margin, 0.5)]
        const double shift = m == 0 ? 0.0 : (m == 1 ? -HWY_TTC_MARGIN : HWY_TTC_MARGIN);
        const int32_t code = m == 0 ? 2 : 1;
        const double distance = gap + shift;
        const double ttc = distance / closing;
        if (ttc < 0) continue;
        const double steps = ttc / p.tq;
        if (!(steps < horizon_steps)) continue;     // int(steps) >= T: both quantisations are out of range (tested in f64:
                                                    // not_zero keeps steps finite, but it can exceed int32)
        ttc_mark(sh_cell, cell0 + (int)steps, code);
        const double up = ceil(steps);
        if (up < horizon_steps) ttc_mark(sh_cell, cell0 + (int)up, code);
      }
    }
  }
  __syncthreads();

  // ---- phase 2: the grid, f32 [V][L][T] -------------------------------------------------------------------------------------------
  if (p.grid) {
    float *out = p.grid + (size_t)blockIdx.x * cells;
    for (int k = lane; k < cells; k += 64) out[k] = (float)ttc_cost(sh_cell[k]);
  }

  // ---- phase 3: the backward sweep of the value iteration ---------------------------------------------------------------------------
  if (PLAN) {
    const int states = V * L;
    const int32_t wme = p.packed[row + me];
    int my_h = word_speed_index(wme), my_i = word_lane(wme);  // grid_state = (speed_index, lane_index[2], 0)
    my_h = my_h < V ? my_h : V - 1;
    my_i = my_i < L ? my_i : L - 1;
    const int lane_div = L - 1 > 1 ? L - 1 : 1, speed_div = V - 1 > 1 ? V - 1 : 1;
    for (int j = T - 1; j >= 0; --j) {
      const double *next = sh_value[(j + 1) & 1];
      double *cur = sh_value[j & 1];
      for (int s = lane; s < states; s += 64) {
        const int h = s / L, i = s % L;
        const int32_t code = sh_cell[s * T + j];
        // state_reward = collision_reward * grid + right_lane_reward * lanes + high_speed_reward * speeds, left to right
        const double lanes = (double)i / (double)lane_div;
        const double speeds = (double)h / (double)speed_div;
        const double r0 = p.collision_reward * ttc_cost(code);
        const double r1 = p.right_lane_reward * lanes;
        const double r2 = p.high_speed_reward * speeds;
        const double r01 = r0 + r1;
        const double state_reward = r01 + r2;
        const bool terminal = code == 2 || j == T - 1;  // collision | end_of_horizon
        // transition_model: IDLE by default; LEFT / RIGHT move a lane; FASTER / SLOWER change the speed where j == 0; all clipped
        const int il = i > 0 ? i - 1 : 0, ir = i < L - 1 ? i + 1 : L - 1;
        const int hf = (j == 0 && h < V - 1) ? h + 1 : h, hs = (j == 0 && h > 0) ? h - 1 : h;
        const int nxt[5] = {h * L + il, s, h * L + ir, hf * L + i, hs * L + i};
        double qa[5], best = 0.0;
        int arg = 0;
        for (int k = 0; k < 5; ++k) {
          const double action_reward = (k == 0 || k == 2) ? p.lane_change_reward : 0.0;
          const double reward = state_reward + action_reward;
          const double future = terminal ? 0.0 : next[nxt[k]];
          const double discounted = p.gamma * future;
          qa[k] = reward + discounted;
          if (k == 0 || qa[k] > best) { best = qa[k]; arg = k; }
        }
        cur[s] = best;
        if (j == 0 && h == my_h && i == my_i) {
          p.action[blockIdx.x] = arg;
          if (p.q)
            for (int k = 0; k < 5; ++k) p.q[(size_t)blockIdx.x * 5 + k] = qa[k];
        }
      }
      __syncthreads();
    }
  }
}

}  // namespace hwy
