// hwy_park.h -- the parking scenario (envs/parking_env.py: ParkingEnv) on the device: goal-conditioned continuous control.
//
// One THREAD per environment, 256-thread workgroups, no LDS, no cross-lane traffic: a parking step is one moving rectangle (the
// ContinuousAction ego, a plain Vehicle), up to 26 resting ones and four walls -- a few hundred f64 operations per frame, where the
// step kernels of hwy_device.h spend a wavefront per environment on IDM and MOBIL.  The planes are [field][E] (include/hwy_park.h),
// so that a wavefront's loads and stores coalesce.
//
// Per policy step (AbstractEnv.step / _simulate, abstract.py:259-310): time += 1 / policy_frequency; ContinuousAction.act on the
// first frame (hwy_act.h: act_map, float32 operation by operation); then `frames` times Road.act (nothing: no vehicle here has a
// policy), Road.step = every Vehicle.step, then the collision pass in the reference's list order (road.py:475-481).
//
// Ego frame = Vehicle.step (kinematics.py:130-153) through the device functions the direct-control kernels use: the sticky
// clip_actions (direct_clip_actions), tan(beta) = tan(steering) / 2 once per step (direct_begin_step), cos / sin(heading + beta)
// by angle addition against the cached cos / sin of the heading, the impact displacement at the start of the next step,
// direct_speed_update (product and sum in two statements: the speed is compared bit for bit), sincos_bounded.
// A parked vehicle's Vehicle.step moves nothing (action (0, 0), speed 0, and a crashed one gets -1.0 * 0) except by a pending impact.
//
// Collisions.  Road.vehicles = [ego, parked 0 .. n-1], Road.objects = [goal Landmark, walls]; the Landmark is not solid: a pair
// with it sets its `hit`, which nothing observable reads, so it is skipped.
//   * ego x parked: the reference's own spherical pre-check (objects.py:124-127) from the SPOT of every set bit of the occupancy
//     mask -- arithmetic only, no load.  Only where one passes (or a vehicle has been struck before) the list-order loop below runs:
//     it reads the list order and runs the literal SAT (park_pair_collide: sat_axis with both bodies' half extents).
//   * ego x walls: the same pre-check with the wall's diagonal, then the SAT.  The whole translation goes to the vehicle
//     (objects.py:106-107); between two vehicles each gets a signed half (objects.py:111-112).
//   * pairs of RESTING bodies are skipped, because they are provably (False, False): two never-struck parked vehicles stand on
//     spots 4 m apart with 2 m wide, parallel bodies and zero speed -- 2 m of clear space on the lateral axis, which is a SAT normal
//     of both; a never-struck vehicle reaches |y| <= 16.5 and |x| <= 27, the inner faces of the walls are at |y| = 20.5 and
//     |x| = 34.5 -- 4 m and 7.5 m clear on a wall's own normal.  (The pre-check sphere does NOT dismiss vehicle x long wall:
//     37.7 m of radius; it is the SAT that separates them.)
//   * once a vehicle has been struck (an impact or a crash was assigned to it) it is a general body: its position lives in the
//     `parked` planes, and every pair that contains a struck body is evaluated literally, in list order.  A rare path: loops.
//
// End of step: KinematicsGoalObservation (observation.py:535-560) float32 [3][6] = observation, achieved_goal, desired_goal, each
// the six features DIVIDED by `scales`; reward f64 = -sqrt(dot(|achieved - desired|, w)) + collision_reward * crashed (sqrt for
// np.power(., 0.5): they differ in the last bit now and then, far inside the 1e-9 the reward is held to); is_success = goal reward >
// -success_goal_reward; terminated = crashed or success; truncated = time >= duration.
//
// K steps per launch: the loop over policy steps is inside the kernel, the state stays in registers; the arithmetic of a step
// does not depend on K, so K steps in one launch are bit-identical to K launches.
//
// Episode start (park_begin_episode), the rule of ParkingEnv._create_vehicles on the project's Philox stream (seed, episode):
//   block (0, episode, 0): u0 -> heading = 2 pi u0; u1 -> the goal;   block (1 + i / 2, episode, 0): u(i mod 2) -> parked vehicle i
//   ego spot = get_closest_lane_index((0, 0), heading): every lane is 10 m ahead of the origin, the two columns next to x = 0
//   (spots 6, 7 and 20, 21) are 2 m aside, and the first of equal distances wins (np.argmin): spot 6 when |wrap(h - pi/2)| <=
//   |wrap(h + pi/2)|, else spot 20.  A choice among n free spots is the min(floor(u n), n - 1)-th free spot in spot order (the
//   reference's empty_spots list keeps lanes_dict order).  With no spot free the vehicle is skipped (`continue`).
//
// Like hwy_act.h this header includes no HIP runtime: hwy_kernels_park.hip and hwy_park.hip include <hip/hip_runtime.h> first.
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/hwy_park.h"
#include "hwy_device.h"
#include "hwy_act.h"

namespace hwy {

#define HWY_PARK_BLOCK 256
#define HWY_PARK_COS_HALF_PI 6.123233995736766e-17  // np.cos(+-np.pi / 2): the lanes' and the upright walls' cos(heading)
#define HWY_PARK_HALF_PI 1.5707963267948966

struct ParkParams {
  double *ego;      // [HWY_PARK_EGO_F64][E]
  int32_t *ints;    // [HWY_PARK_INTS][E]
  uint8_t *order;   // [26][E]
  double *parked;   // [HWY_PARK_PARKED_F64][26][E]
  const float *actions;  // [k_steps][E][2]
  float *obs;            // [E][3][6] or null
  double *reward;        // [E] or null
  uint8_t *flags;        // [E] or null
  double *step_reward;   // [k_steps][E] or null
  uint8_t *step_flags;   // [k_steps][E] or null
  const uint8_t *mask;   // reset kernel: [E] or null
  const uint64_t *seeds; // reset kernel: [E] or null
  int32_t E, k_steps, frames, add_walls, vehicles_count, autoreset;
  uint64_t base_seed;
  double dt, policy_dt, duration, w[6], scales[6], success, collision_reward, a0, a1, s0, s1;
};

// host side: what hwy_park_create accepts (include/hwy_park.h: scope)
inline int park_validate(const hwy_park_config *c, const char **why) {
  *why = "";
#define HWY_PARK_BAD(msg) do { *why = msg; return HWY_PARK_ERR_INVALID_ARG; } while (0)
  if (!c) HWY_PARK_BAD("config is NULL");
  if (c->struct_size != (int32_t)sizeof(hwy_park_config)) HWY_PARK_BAD("struct_size != sizeof(hwy_park_config)");
  if (c->num_envs < 1 || c->num_envs > (1 << 24)) HWY_PARK_BAD("num_envs must be in [1, 2^24]");
  if (c->vehicles_count < 0 || c->vehicles_count > HWY_PARK_MAX_PARKED) HWY_PARK_BAD("vehicles_count must be in [0, 26]");
  if (c->frames < 1 || c->frames > HWY_PARK_MAX_FRAMES) HWY_PARK_BAD("frames per policy step must be in [1, 15]");
  if (!(c->dt > 0.0) || !(c->dt < 1e3) || !(c->policy_dt > 0.0) || !(c->policy_dt < 1e6)) HWY_PARK_BAD("dt and policy_dt must be positive and finite");
  if (!(fabs(c->duration) < 1e300)) HWY_PARK_BAD("duration must be finite");
  for (int k = 0; k < 6; ++k) {
    if (!(fabs(c->reward_weights[k]) < 1e300)) HWY_PARK_BAD("reward_weights must be finite");
    if (!(fabs(c->scales[k]) < 1e300) || c->scales[k] == 0.0) HWY_PARK_BAD("scales must be finite and non-zero");
  }
  if (!(fabs(c->success_goal_reward) < 1e300) || !(fabs(c->collision_reward) < 1e300)) HWY_PARK_BAD("success_goal_reward and collision_reward must be finite");
  for (int k = 0; k < 2; ++k) {
    if (!(fabs(c->acceleration_range[k]) < 1e6)) HWY_PARK_BAD("acceleration_range must be finite");
    if (!(fabs(c->steering_range[k]) <= HWY_ACT_MAX_STEERING)) HWY_PARK_BAD("steering_range must lie within +-pi/3");
  }
#undef HWY_PARK_BAD
  return HWY_PARK_OK;
}

inline ParkParams park_params(const hwy_park_config &c) {
  ParkParams p;
  memset(&p, 0, sizeof p);
  p.E = c.num_envs; p.k_steps = 1; p.frames = c.frames; p.add_walls = c.add_walls ? 1 : 0; p.vehicles_count = c.vehicles_count;
  p.autoreset = c.autoreset ? 1 : 0; p.base_seed = c.base_seed;
  p.dt = c.dt; p.policy_dt = c.policy_dt; p.duration = c.duration;
  for (int k = 0; k < 6; ++k) { p.w[k] = c.reward_weights[k]; p.scales[k] = c.scales[k]; }
  p.success = c.success_goal_reward; p.collision_reward = c.collision_reward;
  p.a0 = c.acceleration_range[0]; p.a1 = c.acceleration_range[1]; p.s0 = c.steering_range[0]; p.s1 = c.steering_range[1];
  return p;
}

// ---- geometry of the lot (ParkingEnv._create_road, spots = 14, width 4, y_offset 10, length 8) ------------------------------------
__device__ inline double park_spot_x(int k) { return 4.0 * (double)(k < 14 ? k : k - 14) - 26.0; }  // (k + 1 - 7) * 4.0 - 2.0, exact
__device__ inline double park_spot_y(int k) { return k < 14 ? 14.0 : -14.0; }                      // lane.position(4, 0)
__device__ inline double park_spot_sin(int k) { return k < 14 ? 1.0 : -1.0; }                      // heading +-pi/2

// one rectangle with its own size: a = the reference's `self` (earlier in the list), b = `other`
struct ParkBody {
  double x, y, v, c, s, hl, hw, diag;
};
// RoadObject._is_colliding + utils.are_polygons_intersecting (objects.py:122-138, utils.py:196-241): pair_collide_body of
// hwy_device.h with both bodies' half extents and diagonals -- the same order of the eight normals, the same tie rule, the same
// swept test.  Returns bit 0 intersecting, bit 1 will_intersect; the translation in (*tx, *ty) when will_intersect.
__device__ inline int park_pair_collide(const ParkBody &A, const ParkBody &B, double dt, double *tx, double *ty) {
  const double dx = B.x - A.x, dy = B.y - A.y;
  *tx = 0;
  *ty = 0;
  if (sqrt(dx * dx + dy * dy) > (A.diag + B.diag) / 2 + A.v * dt) return 0;  // the pre-check, with `self`'s speed
  const double ddx = A.v * A.c * dt - B.v * B.c * dt, ddy = A.v * A.s * dt - B.v * B.s * dt;
  const double cdx = A.x - B.x, cdy = A.y - B.y;
  const double cr = fabs(A.c * B.c + A.s * B.s), sr = fabs(B.s * A.c - B.c * A.s);
  SatAcc acc{3, __builtin_inf(), 0.0, 0.0, 8};
  // -u_a, +w_a, +u_a, -w_a, -u_b, +w_b, +u_b, -w_b (positions 0 .. 7)
  sat_axis(acc, A.c, A.s, A.x * A.c + A.y * A.s, A.hl, B.x * A.c + B.y * A.s, B.hl * cr + B.hw * sr, A.c * ddx + A.s * ddy, cdx, cdy, 2, 0);
  HWY_SAT_FENCE();
  sat_axis(acc, -A.s, A.c, A.y * A.c - A.x * A.s, A.hw, B.y * A.c - B.x * A.s, B.hl * sr + B.hw * cr, A.c * ddy - A.s * ddx, cdx, cdy, 1, 3);
  HWY_SAT_FENCE();
  sat_axis(acc, B.c, B.s, A.x * B.c + A.y * B.s, A.hl * cr + A.hw * sr, B.x * B.c + B.y * B.s, B.hl, B.c * ddx + B.s * ddy, cdx, cdy, 6, 4);
  HWY_SAT_FENCE();
  sat_axis(acc, -B.s, B.c, A.y * B.c - A.x * B.s, A.hl * sr + A.hw * cr, B.y * B.c - B.x * B.s, B.hw, B.c * ddy - B.s * ddx, cdx, cdy, 5, 7);
  if (acc.flags & 2) {
    *tx = acc.min_distance * acc.axx;
    *ty = acc.min_distance * acc.axy;
  }
  return acc.flags;
}

// wall w of ParkingEnv._create_vehicles: y = -21, y = +21 (70 x 1, heading 0), x = -35, x = +35 (42 x 1, heading pi / 2)
__device__ inline ParkBody park_wall(int w) {
  if (w < 2) return ParkBody{0.0, w == 0 ? -21.0 : 21.0, 0.0, 1.0, 0.0, 35.0, 0.5, sqrt(70.0 * 70.0 + 1.0 * 1.0)};
  return ParkBody{w == 2 ? -35.0 : 35.0, 0.0, 0.0, HWY_PARK_COS_HALF_PI, 1.0, 21.0, 0.5, sqrt(42.0 * 42.0 + 1.0 * 1.0)};
}

// ---- one environment in registers ------------------------------------------------------------------------------------------------------
struct ParkEnv {
  double x, y, h, v, accel, steer, impx, impy, time, sn, cs;
  int32_t flags, steps, episode, goal;
  uint32_t occ, struck, pcrashed, pimpact;
};
__device__ inline ParkEnv park_load(const ParkParams &p, int e) {
  ParkEnv s;
  const size_t E = (size_t)p.E;
  s.x = p.ego[HWY_PARK_X * E + e]; s.y = p.ego[HWY_PARK_Y * E + e]; s.h = p.ego[HWY_PARK_HEADING * E + e];
  s.v = p.ego[HWY_PARK_SPEED * E + e]; s.accel = p.ego[HWY_PARK_ACCEL * E + e]; s.steer = p.ego[HWY_PARK_STEER * E + e];
  s.impx = p.ego[HWY_PARK_IMPACT_X * E + e]; s.impy = p.ego[HWY_PARK_IMPACT_Y * E + e]; s.time = p.ego[HWY_PARK_TIME * E + e];
  s.flags = p.ints[HWY_PARK_I_FLAGS * E + e]; s.steps = p.ints[HWY_PARK_I_STEPS * E + e];
  s.episode = p.ints[HWY_PARK_I_EPISODE * E + e]; s.goal = p.ints[HWY_PARK_I_GOAL * E + e];
  s.occ = (uint32_t)p.ints[HWY_PARK_I_OCCUPIED * E + e]; s.struck = (uint32_t)p.ints[HWY_PARK_I_STRUCK * E + e];
  s.pcrashed = (uint32_t)p.ints[HWY_PARK_I_PCRASHED * E + e]; s.pimpact = (uint32_t)p.ints[HWY_PARK_I_PIMPACT * E + e];
  sincos_bounded(s.h, &s.sn, &s.cs);
  return s;
}
__device__ inline void park_store(const ParkParams &p, int e, const ParkEnv &s) {
  const size_t E = (size_t)p.E;
  p.ego[HWY_PARK_X * E + e] = s.x; p.ego[HWY_PARK_Y * E + e] = s.y; p.ego[HWY_PARK_HEADING * E + e] = s.h;
  p.ego[HWY_PARK_SPEED * E + e] = s.v; p.ego[HWY_PARK_ACCEL * E + e] = s.accel; p.ego[HWY_PARK_STEER * E + e] = s.steer;
  p.ego[HWY_PARK_IMPACT_X * E + e] = s.impx; p.ego[HWY_PARK_IMPACT_Y * E + e] = s.impy; p.ego[HWY_PARK_TIME * E + e] = s.time;
  p.ints[HWY_PARK_I_FLAGS * E + e] = s.flags; p.ints[HWY_PARK_I_STEPS * E + e] = s.steps;
  p.ints[HWY_PARK_I_EPISODE * E + e] = s.episode; p.ints[HWY_PARK_I_GOAL * E + e] = s.goal;
  p.ints[HWY_PARK_I_OCCUPIED * E + e] = (int32_t)s.occ; p.ints[HWY_PARK_I_STRUCK * E + e] = (int32_t)s.struck;
  p.ints[HWY_PARK_I_PCRASHED * E + e] = (int32_t)s.pcrashed; p.ints[HWY_PARK_I_PIMPACT * E + e] = (int32_t)s.pimpact;
}
// where a body of work keeps the planes of its struck bodies and the stored steering angle the direct-control functions write: the
// advance kernel its environment's own column of ParkParams::parked ({p.parked, E, e, e}), a planner's candidate a private column
// (hwy_park_cem.h), so that nothing it strikes reaches the environment it started from
struct ParkSlot {
  double *planes;  // [HWY_PARK_PARKED_F64][26][stride]
  size_t stride, at;
  size_t ctl;      // the entry of DirectArgs::ctl_steer
};
// plane f of parked vehicle i
__device__ inline double &park_plane(const ParkSlot &q, int f, int i) {
  return q.planes[((size_t)f * HWY_PARK_MAX_PARKED + i) * q.stride + q.at];
}
// parked vehicle i of the list as a body: from its spot, or from the planes once it has been struck
__device__ inline ParkBody park_parked_body(const ParkParams &p, int e, const ParkSlot &q, const ParkEnv &s, int i) {
  const int k = p.order[(size_t)i * p.E + e];
  ParkBody b{park_spot_x(k), park_spot_y(k), 0.0, HWY_PARK_COS_HALF_PI, park_spot_sin(k), HWY_VEH_LENGTH / 2, HWY_VEH_WIDTH / 2,
             sqrt(HWY_VEH_LENGTH * HWY_VEH_LENGTH + HWY_VEH_WIDTH * HWY_VEH_WIDTH)};
  if ((s.struck >> i) & 1u) {
    b.x = park_plane(q, 0, i);
    b.y = park_plane(q, 1, i);
  }
  return b;
}
// a collision verdict r != 0 on parked vehicle i: from now on it is a general body (its position moves into the planes) ...
__device__ inline void park_strike(const ParkSlot &q, ParkEnv &s, int i, const ParkBody &b, int r, double ix, double iy) {
  const uint32_t bit = 1u << i;
  if (!(s.struck & bit)) {
    park_plane(q, 0, i) = b.x;
    park_plane(q, 1, i) = b.y;
    s.struck |= bit;
  }
  if (r & 2) {  // ... with a pending impact (applied by its next Vehicle.step)
    park_plane(q, 2, i) = ix;
    park_plane(q, 3, i) = iy;
    s.pimpact |= bit;
  }
  if (r & 1) s.pcrashed |= bit;
}

// ---- one frame: Road.step(dt) ---------------------------------------------------------------------------------------------------------
// e: the environment whose list order is read; q: where its struck bodies live
__device__ inline void park_frame(const ParkParams &p, int e, const ParkSlot &q, ParkEnv &s, EgoControls &ctl, const DirectArgs &da) {
  const double dt = p.dt;
  {  // Vehicle.step of the ego
    const bool crashed0 = (s.flags & HWY_PARK_F_CRASHED) != 0;
    const EgoControls now = direct_clip_actions(da, q.ctl, ctl, s.v, crashed0);
    if (crashed0) s.steer = 0.0;
    const double tb = now.tb;
    const double cb = fast_rsqrt(1.0 + tb * tb), sb = tb * cb;
    const double vx = s.v * (s.cs * cb - s.sn * sb), vy = s.v * (s.sn * cb + s.cs * sb);
    s.x += vx * dt;
    s.y += vy * dt;
    if (s.flags & HWY_PARK_F_HAS_IMPACT) {
      s.x += s.impx;
      s.y += s.impy;
      s.flags = (s.flags | HWY_PARK_F_CRASHED) & ~HWY_PARK_F_HAS_IMPACT;
      s.impx = s.impy = 0.0;
    }
    s.h += s.v * sb * (1.0 / (HWY_VEH_LENGTH / 2)) * dt;
    s.v = direct_speed_update(s.v, now.accel, dt);
    sincos_bounded(s.h, &s.sn, &s.cs);
  }
  // Vehicle.step of the parked vehicles: only a pending impact moves one
  for (uint32_t m = s.pimpact; m; m &= m - 1) {
    const int i = __ffs((int)m) - 1;
    park_plane(q, 0, i) += park_plane(q, 2, i);
    park_plane(q, 1, i) += park_plane(q, 3, i);
    park_plane(q, 2, i) = 0.0;
    park_plane(q, 3, i) = 0.0;
    s.pcrashed |= 1u << i;
  }
  s.pimpact = 0;

  // ---- collisions, in the reference's list order ----
  const double diag_v = sqrt(HWY_VEH_LENGTH * HWY_VEH_LENGTH + HWY_VEH_WIDTH * HWY_VEH_WIDTH);
  const ParkBody ego{s.x, s.y, s.v, s.cs, s.sn, HWY_VEH_LENGTH / 2, HWY_VEH_WIDTH / 2, diag_v};
  const int n = __popc(s.occ);
  double tx, ty;
  // ego x parked: the pre-check from the spots; the list-order loop only where it passes or a body has left its spot
  bool listed = s.struck != 0;
  const double sphere = (diag_v + diag_v) / 2 + s.v * dt;
  for (uint32_t m = s.occ; m; m &= m - 1) {
    const int k = __ffs((int)m) - 1;
    const double dx = park_spot_x(k) - s.x, dy = park_spot_y(k) - s.y;
    listed = listed || !(sqrt(dx * dx + dy * dy) > sphere);
  }
  if (listed) {
    for (int i = 0; i < n; ++i) {
      const ParkBody b = park_parked_body(p, e, q, s, i);
      const int r = park_pair_collide(ego, b, dt, &tx, &ty);
      if (!r) continue;
      if (r & 2) {  // two vehicles: a signed half each
        s.impx = tx / 2;
        s.impy = ty / 2;
        s.flags |= HWY_PARK_F_HAS_IMPACT;
      }
      if (r & 1) s.flags |= HWY_PARK_F_CRASHED;
      park_strike(q, s, i, b, r, -tx / 2, -ty / 2);
    }
  }
  // ego x walls: the whole translation goes to the vehicle
  if (p.add_walls) {
    for (int w = 0; w < 4; ++w) {
      const int r = park_pair_collide(ego, park_wall(w), dt, &tx, &ty);
      if (r & 2) {
        s.impx = tx;
        s.impy = ty;
        s.flags |= HWY_PARK_F_HAS_IMPACT;
      }
      if (r & 1) s.flags |= HWY_PARK_F_CRASHED;
    }
  }
  // pairs that contain a struck body (resting pairs: provably (False, False), see the head of the file)
  if (s.struck) {
    for (int i = 0; i < n; ++i) {
      const ParkBody a = park_parked_body(p, e, q, s, i);
      for (int j = i + 1; j < n; ++j) {
        if (!(((s.struck >> i) | (s.struck >> j)) & 1u)) continue;
        const ParkBody b = park_parked_body(p, e, q, s, j);
        const int r = park_pair_collide(a, b, dt, &tx, &ty);
        if (!r) continue;
        park_strike(q, s, i, a, r, tx / 2, ty / 2);
        park_strike(q, s, j, b, r, -tx / 2, -ty / 2);
      }
      if (p.add_walls && ((s.struck >> i) & 1u)) {
        for (int w = 0; w < 4; ++w) {
          const int r = park_pair_collide(a, park_wall(w), dt, &tx, &ty);
          if (r) park_strike(q, s, i, a, r, tx, ty);
        }
      }
    }
  }
}

// ---- KinematicsGoalObservation and the weighted distance of compute_reward ------------------------------------------------------------
// obs (may be null): float32 [3][6] of this environment.  Returns dot(|achieved - desired|, w).
__device__ inline double park_observe(const ParkParams &p, const ParkEnv &s, float *obs) {
  const double f[6] = {s.x, s.y, s.v * s.cs, s.v * s.sn, s.cs, s.sn};  // Vehicle.to_dict: x, y, vx, vy, cos_h, sin_h
  const double g[6] = {park_spot_x(s.goal), park_spot_y(s.goal), 0.0, 0.0, HWY_PARK_COS_HALF_PI, park_spot_sin(s.goal)};
  double d = 0.0;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const double a = f[k] / p.scales[k], b = g[k] / p.scales[k];
    if (obs) {
      obs[k] = (float)a;
      obs[6 + k] = (float)a;
      obs[12 + k] = (float)b;
    }
    d += fabs(a - b) * p.w[k];
  }
  return d;
}

// ---- one policy step of an environment that is not re-spawned: AbstractEnv.step with the action pair (v0, v1) -----------------------
// Returns the step's HWY_PARK_S_* bits, the reward in *reward and (obs non-null) the observation.  A non-finite pair keeps the stored
// controls.  The one definition behind the advance kernel and the planner's candidates (hwy_park_cem.h).
__device__ inline int park_policy_step(const ParkParams &p, int e, const ParkSlot &q, ParkEnv &s, const DirectArgs &da, float v0, float v1,
                                       float *obs, double *reward) {
  const bool acted = __builtin_isfinite(v0) && __builtin_isfinite(v1);
  const double act_accel = act_map(v0, p.a0, p.a1), act_steer = act_map(v1, p.s0, p.s1);
  EgoControls ctl = direct_begin_step(da, q.ctl, s.accel, s.steer, acted, act_accel, act_steer);
  if (acted) s.steer = act_steer;
  s.time += p.policy_dt;
  for (int f = 0; f < p.frames; ++f) park_frame(p, e, q, s, ctl, da);
  s.accel = ctl.accel;
  s.steps += 1;
  const double goal_reward = -sqrt(park_observe(p, s, obs));
  const bool crashed = (s.flags & HWY_PARK_F_CRASHED) != 0;
  const bool success = goal_reward > -p.success;
  *reward = goal_reward + p.collision_reward * (crashed ? 1.0 : 0.0);
  const int out = ((crashed || success) ? HWY_PARK_S_TERMINATED : 0) | (s.time >= p.duration ? HWY_PARK_S_TRUNCATED : 0) |
                  (success ? HWY_PARK_S_SUCCESS : 0) | (crashed ? HWY_PARK_S_CRASHED : 0);
  if (out & (HWY_PARK_S_TERMINATED | HWY_PARK_S_TRUNCATED)) s.flags |= HWY_PARK_F_DONE;
  return out;
}

// ---- episode start: ParkingEnv._create_vehicles on the Philox stream of (seed, episode) ---------------------------------------------
// the n-th (from 0) set bit of m
__device__ inline int park_nth_bit(uint32_t m, int n) {
  for (; n > 0; --n) m &= m - 1;
  return __ffs((int)m) - 1;
}
__device__ inline int park_choice(double u, int n) {
  const int k = (int)(u * (double)n);
  return k < n - 1 ? k : n - 1;
}
__device__ inline void park_begin_episode(const ParkParams &p, int e, ParkEnv &s, uint64_t seed, uint32_t episode) {
  double u0, u1;
  philox_uniform2(seed, 0u, episode, 0u, &u0, &u1);
  s.x = 0.0; s.y = 0.0; s.v = 0.0; s.accel = 0.0; s.steer = 0.0; s.impx = 0.0; s.impy = 0.0; s.time = 0.0;
  s.h = (2.0 * HWY_PI) * u0;
  sincos_bounded(s.h, &s.sn, &s.cs);
  s.flags = 0; s.steps = 0; s.episode = (int32_t)episode;
  s.struck = 0; s.pcrashed = 0; s.pimpact = 0;
  // the ego's own spot: get_closest_lane_index((0, 0), heading); 12 = |lateral| 2 + 10 m ahead of the lane's start
  const double d_up = 12.0 + fabs(wrap_to_pi(s.h - HWY_PARK_HALF_PI)), d_lo = 12.0 + fabs(wrap_to_pi(s.h - (-HWY_PARK_HALF_PI)));
  uint32_t free_spots = (1u << HWY_PARK_SPOTS) - 1u;
  free_spots &= ~(1u << (d_lo < d_up ? 20 : 6));
  s.goal = park_nth_bit(free_spots, park_choice(u1, HWY_PARK_SPOTS - 1));
  free_spots &= ~(1u << s.goal);
  s.occ = 0;
  int n = 0;
  for (int i = 0; i < p.vehicles_count; ++i) {
    const int n_free = HWY_PARK_SPOTS - 2 - n;
    if (n_free <= 0) continue;
    if (!(i & 1)) philox_uniform2(seed, 1u + (uint32_t)(i >> 1), episode, 0u, &u0, &u1);
    const int k = park_nth_bit(free_spots, park_choice((i & 1) ? u1 : u0, n_free));
    free_spots &= ~(1u << k);
    s.occ |= 1u << k;
    p.order[(size_t)n * p.E + e] = (uint8_t)k;
    ++n;
  }
}

// ---- kernels ------------------------------------------------------------------------------------------------------------------------------
template <int BLOCK>
__global__ void __launch_bounds__(BLOCK) hwy_park_advance_kernel(const ParkParams p) {
  const int e = (int)blockIdx.x * BLOCK + (int)threadIdx.x;
  if (e >= p.E) return;
  ParkEnv s = park_load(p, e);
  DirectArgs da;  // (only the two planes are read: the stored pair of this environment)
  da.ctl_accel = p.ego + (size_t)HWY_PARK_ACCEL * p.E;
  da.ctl_steer = p.ego + (size_t)HWY_PARK_STEER * p.E;
  const ParkSlot slot{p.parked, (size_t)p.E, (size_t)e, (size_t)e};
  double reward = 0.0;
  int out = 0;
  for (int k = 0; k < p.k_steps; ++k) {
    float *const obs = (p.obs && k == p.k_steps - 1) ? p.obs + (size_t)e * 18 : nullptr;
    if (p.autoreset && (s.flags & HWY_PARK_F_DONE)) {  // NextStep: the action is not used, the new episode's first observation
      park_begin_episode(p, e, s, p.base_seed + (uint64_t)e, (uint32_t)s.episode + 1u);
      park_observe(p, s, obs);
      reward = 0.0;
      out = 0;
    } else {
      const float *a = p.actions + ((size_t)k * p.E + e) * 2;
      out = park_policy_step(p, e, slot, s, da, a[0], a[1], obs, &reward);
    }
    if (p.step_reward) p.step_reward[(size_t)k * p.E + e] = reward;
    if (p.step_flags) p.step_flags[(size_t)k * p.E + e] = (uint8_t)out;
  }
  if (p.reward) p.reward[e] = reward;
  if (p.flags) p.flags[e] = (uint8_t)out;
  park_store(p, e, s);
}

// device reset of the masked environments (episode 0 of seeds[e] or base_seed + e) and / or the observation of the state as it is
template <int BLOCK, bool RESET>
__global__ void __launch_bounds__(BLOCK) hwy_park_reset_kernel(const ParkParams p) {
  const int e = (int)blockIdx.x * BLOCK + (int)threadIdx.x;
  if (e >= p.E) return;
  ParkEnv s = park_load(p, e);
  if (RESET && (!p.mask || p.mask[e])) {
    park_begin_episode(p, e, s, p.seeds ? p.seeds[e] : p.base_seed + (uint64_t)e, 0u);
    park_store(p, e, s);
  }
  if (p.obs) park_observe(p, s, p.obs + (size_t)e * 18);
}

// ParkingEnv.compute_reward (p = 0.5) of m rows: -sqrt(dot(|achieved - desired|, w)); one thread per row
struct ParkGoalParams {
  const double *achieved, *desired;  // [m][6]
  double *out;                       // [m]
  long long m;
  double w[6];
};
template <int BLOCK>
__global__ void __launch_bounds__(BLOCK) hwy_park_goal_reward_kernel(const ParkGoalParams g) {
  const long long r = (long long)blockIdx.x * BLOCK + (long long)threadIdx.x;
  if (r >= g.m) return;
  double d = 0.0;
#pragma unroll
  for (int k = 0; k < 6; ++k) d += fabs(g.achieved[r * 6 + k] - g.desired[r * 6 + k]) * g.w[k];
  g.out[r] = -sqrt(d);
}

}  // namespace hwy
