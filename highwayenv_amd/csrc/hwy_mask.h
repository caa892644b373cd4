// hwy_mask.h -- the action mask of DiscreteMetaAction (AbstractEnv.get_available_actions, envs/common/abstract.py:357 ->
// DiscreteMetaAction.get_available_actions, envs/common/action.py:262-298), a kernel of its own.
//
// No step / reset / observe kernel is touched: this kernel is launched on the engine's stream after whatever ran last and reads the
// state planes the Lidar and TTC kernels read (x, y, the packed words for lane / speed index / flags -- the intersection's in the
// layout of hwy_ix.h) and the agent indices; on the road-network families (MergeEnv, MergeGenericEnv) also the lane table of the
// config, which travels in the kernel's arguments.
//
// One THREAD per (environment, agent): the rule is a handful of compares.  The threads of a wavefront cover different environments,
// so the reads of one plane are 64 different rows (one per environment), not one row 64 wide.
//
// mask u8 [E][A][n_ids], 1 = available, columns in the order of the engine's action table (hwy_config.action_set):
//   HWY_ACTIONS_ALL    LANE_LEFT 0, IDLE 1, LANE_RIGHT 2, FASTER 3, SLOWER 4
//   HWY_ACTIONS_LONGI  SLOWER 0, IDLE 1, FASTER 2                       (the intersection scenario always)
//   HWY_ACTIONS_LAT    LANE_LEFT 0, IDLE 1, LANE_RIGHT 2
// The rule, on the vehicle's CURRENT lane_index (not its target lane):
//   IDLE        always
//   LANE_LEFT   `lateral`, lane _id - 1 exists on the vehicle's road (RoadNetwork.side_lanes, road/road.py:200-211) and
//               is_reachable_from(position) (road/lane.py:104-118): not forbidden, |lateral| <= 2 * width_at(s), 0 <= s < length +
//               VEHICLE_LENGTH, in the candidate lane's own local coordinates
//   LANE_RIGHT  the same with _id + 1
//   FASTER      `longitudinal` and speed_index < target_speeds.size - 1
//   SLOWER      `longitudinal` and speed_index > 0
// Lane geometry: StraightLane.local_coordinates with direction (1, 0) is (x - x0, y - y0); SineLane subtracts amplitude * sin(pulsation
// * s + phase) from the lateral -- the arithmetic of hwy_net.h's net_lat / net_reachable and of hwy_device.h's straight-road form,
// read from the config's table instead of the step kernels' LDS copy (this kernel uses no LDS).
//
// Like hwy_lidar.h this header includes no HIP runtime: hwy_kernels_mask.hip includes <hip/hip_runtime.h> first, the CPU emulation
// (tests/emu/emu_mask.cpp) its shim, hip_emu.h.  The launch rule is hwy_launch_units.h's (select_mask), for both.
#pragma once

#include <stdint.h>
#include <string.h>

#include "../../include/hwy_engine.h"
#include "hwy_device.h"
#include "hwy_ix.h"  // the intersection's packed word (ix_word_*)

namespace hwy {

#define HWY_MASK_BLOCK 256  // threads of a workgroup: four wavefronts of (environment, agent) pairs

struct MaskParams {
  const double *x, *y;     // [E][pitch]
  const int32_t *packed;   // [E][pitch]
  uint8_t *mask;           // [rows][n_ids]
  int32_t rows, N, A, pitch;
  int32_t scenario, action_set, n_ids, n_ts;
  int32_t lanes_count, n_lanes, pad_[2];
  int32_t agent_index[HWY_MAX_AGENTS];
  double lane_width, road_length;
  hwy_lane lane[HWY_MAX_LANES];  // road-network scenarios (unused entries zero; the highway and the intersection read none of it:
                                 // one struct for the three families keeps one kernel, and 1.5 KB of arguments are within the limit)
};

// the action table of a config: the intersection scenario always acts on the longitudinal one (intersection_env.py:14)
inline int mask_action_set(const hwy_config &c) { return c.scenario == HWY_SCENARIO_INTERSECTION ? HWY_ACTIONS_LONGI : c.action_set; }
inline int mask_num_ids(const hwy_config &c) { return HWY_NUM_ACTIONS(mask_action_set(c)); }

// host side: what the entry points accept.  Shared by hwy_engine.hip and the CPU emulation.
inline int mask_validate(const hwy_config &c, const char **why) {
  *why = "";
  if (c.ego_control != HWY_EGO_META) {
    *why = "get_available_actions needs a DiscreteMetaAction ego (ActionType.get_available_actions raises NotImplementedError)";
    return HWY_ERR_UNSUPPORTED;
  }
  return HWY_OK;
}

// host side: the arguments of a config over the planes the kernel reads ([E][pitch] each) and the output
inline MaskParams mask_params(const hwy_config &c, const double *x, const double *y, const int32_t *packed, int pitch, uint8_t *mask) {
  MaskParams p;
  memset(&p, 0, sizeof p);
  p.x = x; p.y = y; p.packed = packed; p.mask = mask;
  p.rows = c.num_envs * c.num_agents; p.N = c.num_vehicles; p.A = c.num_agents; p.pitch = pitch;
  p.scenario = c.scenario; p.action_set = mask_action_set(c); p.n_ids = mask_num_ids(c); p.n_ts = c.num_target_speeds;
  p.lanes_count = c.lanes_count;
  for (int a = 0; a < HWY_MAX_AGENTS; ++a) p.agent_index[a] = a < c.num_agents ? c.agent_index[a] : 0;
  p.lane_width = c.lane_width; p.road_length = c.road_length;
  if (c.scenario == HWY_SCENARIO_MERGE || c.scenario == HWY_SCENARIO_MERGE_GENERIC) {
    p.n_lanes = c.net_lanes < HWY_MAX_LANES ? c.net_lanes : HWY_MAX_LANES;
    for (int k = 0; k < p.n_lanes; ++k) p.lane[k] = c.net[k];
  }
  return p;
}

// AbstractLane.is_reachable_from (lane.py:104-118) of lane `l` of an x-aligned network
__device__ inline bool mask_reachable(const hwy_lane &l, double x, double y) {
  if (l.forbidden) return false;
  const double s = x - l.x0;
  double lat = y - l.y0;
  if (l.amplitude != 0.0) {  // SineLane.local_coordinates (lane.py:267-269)
    double sn, cs;
    sincos_bounded(l.pulsation * s + l.phase, &sn, &cs);
    lat = lat - l.amplitude * sn;
  }
  return fabs(lat) <= 2 * l.width && 0 <= s && s < l.length + HWY_VEH_LENGTH;
}
// ... and of lane `k` of the straight road (lane k is centred on y = k * lane_width, road.py:291-321)
__device__ inline bool mask_reachable_straight(const MaskParams &p, int k, double x, double y) {
  return fabs(y - k * p.lane_width) <= 2 * p.lane_width && 0 <= x && x < p.road_length + HWY_VEH_LENGTH;
}

// BLOCK: threads per workgroup (a template so that the header can be included by several translation units)
template <int BLOCK>
__global__ void __launch_bounds__(BLOCK) hwy_mask_kernel(const MaskParams p) {
  const int r = (int)blockIdx.x * BLOCK + (int)threadIdx.x;  // (environment, agent)
  if (r >= p.rows) return;
  const int e = r / p.A, a = r % p.A;
  const size_t row = (size_t)e * p.pitch;
  // the controlled vehicle's slot: agent_index[a], except on the intersection, whose list is re-compacted while an episode runs --
  // there agent a is the a-th slot that carries HWY_F_CONTROLLED
  int me = -1;
  if (p.scenario == HWY_SCENARIO_INTERSECTION) {
    int seen = 0;
    for (int j = 0; j < p.N; ++j) {
      const int f = ix_word_flags(p.packed[row + j]);
      const bool mine = !(f & HWY_F_ABSENT) && (f & HWY_F_CONTROLLED);
      if (mine && seen == a && me < 0) me = j;
      seen += mine ? 1 : 0;
    }
  } else {
    me = p.agent_index[a];
    me = me < p.N ? me : -1;
  }
  const bool lateral = p.action_set != HWY_ACTIONS_LONGI, longitudinal = p.action_set != HWY_ACTIONS_LAT;
  bool left = false, right = false, faster = false, slower = false;
  if (me >= 0) {
    const int32_t w = p.packed[row + me];
    const bool ix = p.scenario == HWY_SCENARIO_INTERSECTION;  // (its word holds 5-bit lane indices: hwy_ix.h)
    const int lane = ix ? ix_word_lane(w) : word_lane(w), sidx = ix ? ix_word_speed_index(w) : word_speed_index(w);
    if (lateral && p.scenario == HWY_SCENARIO_HIGHWAY) {
      const double x = p.x[row + me], y = p.y[row + me];
      left = lane > 0 && mask_reachable_straight(p, lane - 1, x, y);
      right = lane < p.lanes_count - 1 && mask_reachable_straight(p, lane + 1, x, y);
    } else if (lateral && p.scenario != HWY_SCENARIO_INTERSECTION && lane < p.n_lanes) {  // (lane: an unsigned field, never negative)
      const double x = p.x[row + me], y = p.y[row + me];
      const int id = p.lane[lane].id, count = p.lane[lane].road_lanes;  // side_lanes: the same (from, to), _id -+ 1
      // (lane - 1 and lane + 1 are table entries of the same road: lanes of one road are consecutive, ordered by id)
      left = id > 0 && lane - 1 >= 0 && mask_reachable(p.lane[lane - 1], x, y);
      right = id < count - 1 && lane + 1 < p.n_lanes && mask_reachable(p.lane[lane + 1], x, y);
    }
    faster = longitudinal && sidx < p.n_ts - 1;
    slower = longitudinal && sidx > 0;
  }
  uint8_t *out = p.mask + (size_t)r * p.n_ids;
  if (p.action_set == HWY_ACTIONS_LONGI) {
    out[0] = slower ? 1 : 0; out[1] = 1; out[2] = faster ? 1 : 0;
  } else {
    out[0] = left ? 1 : 0; out[1] = 1; out[2] = right ? 1 : 0;
    if (p.action_set == HWY_ACTIONS_ALL) { out[3] = faster ? 1 : 0; out[4] = slower ? 1 : 0; }
  }
}

}  // namespace hwy
