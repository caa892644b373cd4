// hwy_collision_obs.h -- the TimeToCollision observation of the highway scenario (TimeToCollisionObservation.observe,
// envs/common/observation.py:115-152), a kernel of its own, and the sequences of launches of the entry points around it.
//
// No step / reset / observe kernel is touched: the kernel is launched on the engine's stream after whatever ran last and reads the
// planes hwy_ttc_kernel reads (x, heading, speed, the packed words for lane / speed index / flags) and the agent indices.
//
// The reference computes compute_ttc_grid (finite_mdp.py:104-163), f64 [V][L][T], pads the lane axis with ones on both sides and
// takes the lanes lane - 1 .. lane + 1, repeats the first and the last row of the speed axis and takes the speeds
// speed_index - 1 .. speed_index + 1, and casts to float32.  For V >= 2 that is
//   obs[a][b][t] = 1.0                                                          where lane + b - 1 is outside [0, L)
//                = grid[clamp(speed_index + a - 1, 0, V - 1)][lane + b - 1][t]  otherwise
// (V == 1: numpy's duplicate fancy index in `repeats[[0, -1]] += ...` makes the reference return (2, 3, T); refused.)
//
// One 64-wide wavefront per (environment, agent) computes ONLY the window: nine rows of at most HWY_MAX_TTC_STEPS cells in LDS,
// 576 dwords whatever V and L are -- no capacity classes.
//   phase 0: the rows of the lanes in range start at cost code 0, the rows of the lanes out of range at the code of 1.0;
//   phase 1, lane == other vehicle, in passes of 64: vehicles that are the observer, absent or in a lane outside the window are
//     skipped; for the rest the candidate arithmetic of hwy_ttc.h's phase 1, statement for statement (so that -ffp-contract=on
//     fuses the same things and a knife edge falls the same way as in the grid kernel), for the three CLAMPED window speeds, with
//     an LDS atomic max on the cost code, which does not depend on the order of the vehicles;
//   phase 2: float32 [3][3][T] to HBM, coalesced.
// Barriers between the phases; every loop is bounded by N, 3 and T; nothing waits on another workgroup.
//
// Like hwy_ttc.h this header includes no HIP runtime: hwy_kernels_collision_obs.hip includes <hip/hip_runtime.h> first, the CPU
// emulation (tests/emu/emu_ttc_obs.cpp) its shim, hip_emu.h.  The launch rule is hwy_launch_units.h's (select_collision_obs).
#pragma once

#include <stdint.h>
#include <string.h>

#include "../../include/hwy_engine.h"
#include "hwy_device.h"
#include "hwy_ttc.h"  // ttc_not_zero, ttc_mark, ttc_cost, HWY_TTC_MARGIN (not edited: tests/test_ttc_mutations.py patches its text)

namespace hwy {

#define HWY_COLLISION_OBS_SIDE 3                                                        // obs_speeds == obs_lanes == 3
#define HWY_COLLISION_OBS_ROWS (HWY_COLLISION_OBS_SIDE * HWY_COLLISION_OBS_SIDE)        // (window speed, window lane) rows
#define HWY_COLLISION_OBS_CELLS (HWY_COLLISION_OBS_ROWS * HWY_MAX_TTC_STEPS)            // LDS dwords of the kernel: 576

struct CollisionObsParams {
  const double *x, *heading, *speed;  // [E][pitch]
  const int32_t *packed;              // [E][pitch]
  float *obs;                         // [rows][3][3][T]
  int32_t N, A, pitch, V, L, T;
  int32_t agent_index[HWY_MAX_AGENTS];
  double target_speeds[HWY_MAX_TARGET_SPEEDS];
  double tq;
};

// host side: what the entry points accept (include/hwy_engine.h: hwy_ttc_observe_device; gamma and lane_change_reward of
// hwy_ttc_params are not read).  Shared by hwy_engine.hip and the CPU emulation.
inline int ttc_obs_validate(const hwy_config &c, const hwy_ttc_params *tp, const char **why) {
  *why = "";
  if (!tp) { *why = "params is NULL"; return HWY_ERR_INVALID_ARG; }
  if (c.scenario != HWY_SCENARIO_HIGHWAY) { *why = "the TimeToCollision observation runs on the highway scenario only"; return HWY_ERR_UNSUPPORTED; }
  if (c.ego_control != HWY_EGO_META) {
    *why = "the TimeToCollision observation needs a DiscreteMetaAction ego (a plain Vehicle has no speed_index: the reference raises there too)";
    return HWY_ERR_UNSUPPORTED;
  }
  if (c.num_target_speeds < 2) {
    *why = "the TimeToCollision observation needs at least 2 target speeds (with one, numpy's duplicate fancy index in "
           "`repeats[[0, -1]] += ...` makes the reference return shape (2, 3, T))";
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
  return HWY_OK;
}

// floats of one (environment, agent) row of the observation
inline size_t collision_obs_len(const hwy_ttc_params &tp) { return (size_t)HWY_COLLISION_OBS_ROWS * (size_t)tp.time_steps; }

// host side: the arguments of a config over the planes the kernel reads ([E][pitch] each) and the output
inline CollisionObsParams collision_obs_params(const hwy_config &c, const hwy_ttc_params &tp, const double *x, const double *heading,
                                               const double *speed, const int32_t *packed, int pitch, float *obs) {
  CollisionObsParams p;
  memset(&p, 0, sizeof p);
  p.x = x; p.heading = heading; p.speed = speed;
  p.packed = packed;
  p.obs = obs;
  p.N = c.num_vehicles; p.A = c.num_agents; p.pitch = pitch;
  p.V = c.num_target_speeds; p.L = c.lanes_count; p.T = tp.time_steps;
  for (int a = 0; a < HWY_MAX_AGENTS; ++a) p.agent_index[a] = a < c.num_agents ? c.agent_index[a] : 0;
  for (int v = 0; v < HWY_MAX_TARGET_SPEEDS; ++v) p.target_speeds[v] = c.target_speeds[v];
  p.tq = tp.time_quantization;
  return p;
}

// CELLS: the window's capacity in LDS, HWY_COLLISION_OBS_CELLS (a template so that the header can be included by several translation units)
template <int CELLS>
__global__ void __launch_bounds__(64) hwy_collision_obs_kernel(const CollisionObsParams p) {
  __shared__ int32_t sh_cell[CELLS];
  const int lane = threadIdx.x;
  const int e = (int)blockIdx.x / p.A, a = (int)blockIdx.x % p.A;
  const size_t row = (size_t)e * p.pitch;
  const int me = p.agent_index[a];
  const int V = p.V, L = p.L, T = p.T;
  const int cells = HWY_COLLISION_OBS_ROWS * T;
  const int32_t wme = p.packed[row + me];
  int my_h = word_speed_index(wme);  // vehicle.speed_index
  my_h = my_h < V ? my_h : V - 1;
  const int lane0 = word_lane(wme) - HWY_COLLISION_OBS_SIDE / 2;  // the lane of window column 0 (may be -1)

  // ---- phase 0: np.zeros for the lanes of the road, the padding of ones either side of it ------------------------------------
  for (int k = lane; k < cells; k += 64) {
    const int wl = lane0 + (k / T) % HWY_COLLISION_OBS_SIDE;
    sh_cell[k] = (wl >= 0 && wl < L) ? 0 : 2;
  }
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
    const int wb = other_lane - lane0;  // the window column of the other's lane
    if ((word_flags(w) & HWY_F_ABSENT) || other_lane >= L || wb < 0 || wb >= HWY_COLLISION_OBS_SIDE) continue;
    const double ospeed = p.speed[row + j];
    double osn, ocs;
    sincos_bounded(p.heading[row + j], &osn, &ocs);
    // np.dot(other.direction, vehicle.direction)
    const double d0 = ocs * ecs;
    const double d1 = osn * esn;
    const double dot = d0 + d1;
    const double projected = ospeed * dot;          // other_projected_speed
    const double gap = p.x[row + j] - ex;           // vehicle.lane_distance_to(other): direction is exactly (1, 0)
    for (int wa = 0; wa < HWY_COLLISION_OBS_SIDE; ++wa) {
      int v = my_h + wa - HWY_COLLISION_OBS_SIDE / 2;  // np.repeat of the first and the last row: the clamped speed index
      v = v < 0 ? 0 : (v > V - 1 ? V - 1 : v);
      const double ego_speed = p.target_speeds[v];  // vehicle.index_to_speed(speed_index)
      if (ego_speed == ospeed) continue;
      const double closing = ttc_not_zero(ego_speed - projected);
      const int cell0 = (wa * HWY_COLLISION_OBS_SIDE + wb) * T;
      for (int m = 0; m < 3; ++m) {                 // collision_points = [(0, 1), (-margin, 0.5), (margin, 0.5)]
        const double shift = m == 0 ? 0.0 : (m == 1 ? -HWY_TTC_MARGIN : HWY_TTC_MARGIN);
        const int32_t code = m == 0 ? 2 : 1;
        const double distance = gap + shift;
        const double ttc = distance / closing;
        if (ttc < 0) continue;
        const double steps = ttc / p.tq;
        if (!(steps < horizon_steps)) continue;     // int(steps) >= T: both quantisations are out of range (tested in f64)
        ttc_mark(sh_cell, cell0 + (int)steps, code);
        const double up = ceil(steps);
        if (up < horizon_steps) ttc_mark(sh_cell, cell0 + (int)up, code);
      }
    }
  }
  __syncthreads();

  // ---- phase 2: the window, f32 [3][3][T] ------------------------------------------------------------------------------------------
  float *out = p.obs + (size_t)blockIdx.x * cells;
  for (int k = lane; k < cells; k += 64) out[k] = (float)ttc_cost(sh_cell[k]);
}

// ---- host side: the sequences of launches, written ONCE for hwy_engine.hip and the CPU emulation -------------------------------------
// hwy_step_same_step_ttc_device.  `ops` supplies the launches -- step() (the family's step launch with auto-reset on; its own
// observation goes to a buffer the engine owns), mask(final), observe() (this header's kernel into the call's obs plane), stash()
// (hwy_final_kernel with rows of 9 * T floats per agent), respawn() -- each returning 0 or the status the call returns.
//   1 step   2 mask of the terminal state (if asked for)   3 observe: the terminal window goes into obs   4 stash: the rows of the
//   environments that ended go to final_obs   5 re-spawn   6 observe: the window of the state the call leaves   7 mask (if asked for)
// Rows of environments that did not end come out of 6 as they came out of 3: the same state, the same code.
template <typename Ops>
inline int ttc_obs_same_step_sequence(Ops &&ops, bool final_action_mask, bool action_mask) {
  if (int rc = ops.step()) return rc;
  if (final_action_mask)
    if (int rc = ops.mask(true)) return rc;
  if (int rc = ops.observe()) return rc;
  if (int rc = ops.stash()) return rc;
  if (int rc = ops.respawn()) return rc;
  if (int rc = ops.observe()) return rc;
  if (action_mask)
    if (int rc = ops.mask(false)) return rc;
  return 0;
}

// hwy_rollout_ttc_device: k_steps (step launch, observe launch) pairs on block k of every plane -- the launches of k_steps single
// calls, the same results by construction.  ops.step(k), ops.observe(k).
template <typename Ops>
inline int ttc_obs_rollout_sequence(Ops &&ops, int32_t k_steps) {
  for (int32_t k = 0; k < k_steps; ++k) {
    if (int rc = ops.step(k)) return rc;
    if (int rc = ops.observe(k)) return rc;
  }
  return 0;
}

}  // namespace hwy
