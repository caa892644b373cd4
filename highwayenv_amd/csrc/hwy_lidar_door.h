// hwy_lidar_door.h -- LidarObservation.trace + observe (envs/common/observation.py:702-769) of ANY engine's current state, through
// a door of its own: a kernel, parameters (hwy_lidar_params, include/hwy_engine.h) and entry points next to whatever observation
// type the engine was created with.  No step / reset / observe kernel is touched and hwy_lidar.h's kernel keeps its text; this
// kernel is launched on the engine's stream after whatever ran last and reads the planes that one reads (x, y, heading, speed,
// the packed words for the flags) and the agent indices.
//
// The structure is hwy_lidar_kernel's: one 64-wide wavefront per (environment, agent), passes of 64 obstacles, phase 1 with one
// lane per obstacle into LDS (the same 92 bytes per obstacle, 5888 B per workgroup), phase 2 with the lanes on the cells, folding
// sequentially IN LIST ORDER; the arithmetic is that kernel's statement for statement (its inline helpers are called, separate
// products and sums, IEEE division and square root, divisions by zero kept, hwy_math.h's sincos_bounded / atan2_bounded), so that
// for a highway state and cells <= 64 the two kernels write the same bits.  Four things generalise:
//   observer     agent_index[a] on the highway and the merge scenarios; on the intersection, whose list is re-compacted while an
//                episode runs, the a-th slot that is not HWY_F_ABSENT and carries HWY_F_CONTROLLED (hwy_mask.h finds it the same
//                way): N <= 64 there, so one ballot and a select of the a-th set bit.  No such slot: every cell stays at the range.
//   obstacles    every slot that is not HWY_F_ABSENT and is not the observer, in slot order -- the reference's
//                `road.vehicles + road.objects` (DESIGN.md section 3 has the argument: the merge scenarios keep the Obstacle in
//                the last slot, the intersection's compaction keeps the order of the list and has no objects)
//   dimensions   a slot with HWY_F_OBSTACLE is 2 m x 2 m (Obstacle.LENGTH = WIDTH = 2), everything else 5 m x 2 m: only
//                rect_corners' half-length changes, WIDTH / 2 is 1.0 for both
//   cells        up to HWY_LIDAR_DOOR_MAX_CELLS = 256: lane c owns cells c, c + 64, c + 128, c + 192 (CPL cells per lane), each
//                with its own ray and (distance, velocity) pair IN REGISTERS; the LDS of phase 1 is read by broadcast, once per
//                obstacle for all the cells of a lane, so four cells per lane cost no LDS and no extra LDS traffic.  The 8-bit
//                fields of the packed word (centre | start << 8 | end << 16) hold 0..255.  Every cell folds its candidates in
//                list order, the centre candidate before the ray candidate of the same obstacle, as before.
//
// Like hwy_lidar.h this header includes no HIP runtime: hwy_kernels_lidar_door.hip includes <hip/hip_runtime.h> first, the CPU
// emulation (tests/emu/emu_lidar_door.cpp) its shim, hip_emu.h.  The launch rule is hwy_launch_units.h's (select_lidar_door).
#pragma once

#include <stdint.h>
#include <string.h>

#include "../../include/hwy_engine.h"
#include "hwy_device.h"
#include "hwy_ix.h"     // ix_word_flags: the intersection's packed word
#include "hwy_lidar.h"  // lidar_fold, lidar_dot2, lidar_norm2, lidar_angle_to_index, lidar_interval_distance, LIDAR_* (not edited)

namespace hwy {

#define HWY_LIDAR_DOOR_UNIT  // (hwy_launch_units.h: this unit's kernel is in the translation unit)
#define HWY_LIDAR_DOOR_MAX_CELLS HWY_MAX_LIDAR_DOOR_CELLS
#define HWY_LIDAR_DOOR_MAX_RANGE 3.4028234663852886e38  // FLT_MAX: the range is cast to float32
#define HWY_OBSTACLE_LENGTH 2.0  // Obstacle.LENGTH (vehicle/objects.py:215-222); its WIDTH is HWY_VEH_WIDTH

struct LidarDoorParams {
  const double *x, *y, *heading, *speed;  // [E][pitch]
  const int32_t *packed;                  // [E][pitch]
  float *obs;                             // [rows][A][cells][2]
  int32_t N, A, pitch, cells, scenario;
  int32_t agent_index[HWY_MAX_AGENTS];
  double max_range;
};

// host side: what the entry points accept (include/hwy_engine.h: hwy_lidar_observe_device, hwy_rollout_lidar_device).  Shared by
// hwy_engine.hip and the CPU emulation.  `has_state`: the engine has been reset (or given a state); `rollout`: the K-step door.
inline int lidar_door_validate(const hwy_config &c, const hwy_lidar_params *lp, bool has_state, bool rollout, const char **why) {
  *why = "";
  if (!lp) { *why = "params is NULL"; return HWY_ERR_INVALID_ARG; }
  if (lp->cells < 1 || lp->cells > HWY_LIDAR_DOOR_MAX_CELLS) { *why = "cells must be in [1,256]"; return HWY_ERR_INVALID_ARG; }
  // "finite": as the float32 the grid holds it in (np.ones(..., float32) * maximum_range), i.e. at most FLT_MAX; NaN fails both tests.
  // _abi.lidar_door_params states the same rule.
  if (!(lp->maximum_range > 0) || !(lp->maximum_range <= HWY_LIDAR_DOOR_MAX_RANGE)) {
    *why = "maximum_range must be positive and finite as a float32 (at most FLT_MAX)";
    return HWY_ERR_INVALID_ARG;
  }
  if (lp->normalize != 0 && lp->normalize != 1) { *why = "normalize must be 0 or 1"; return HWY_ERR_INVALID_ARG; }
  if (!has_state) { *why = "the engine has not been reset: there is no state to observe"; return HWY_ERR_INVALID_ARG; }
  if (rollout && c.scenario == HWY_SCENARIO_INTERSECTION) {
    *why = "on the intersection the reference observes BEFORE it clears and spawns vehicles and a kernel behind the step sees the list "
           "AFTER: the trace is observe() called after step(), not the observation step() returns";
    return HWY_ERR_UNSUPPORTED;
  }
  return HWY_OK;
}

// floats of one (environment, agent) row of the observation
inline size_t lidar_door_len(const hwy_lidar_params &lp) { return (size_t)lp.cells * 2; }

// host side: the arguments of a config over the four planes it reads ([E][pitch] each), the packed words and the output
inline LidarDoorParams lidar_door_params(const hwy_config &c, const hwy_lidar_params &lp, const double *x, const double *y,
                                         const double *heading, const double *speed, const int32_t *packed, int pitch, float *obs) {
  LidarDoorParams p;
  memset(&p, 0, sizeof p);
  p.x = x; p.y = y; p.heading = heading; p.speed = speed;
  p.packed = packed;
  p.obs = obs;
  p.N = c.num_vehicles; p.A = c.num_agents; p.pitch = pitch; p.cells = lp.cells; p.scenario = c.scenario;
  for (int a = 0; a < HWY_MAX_AGENTS; ++a) p.agent_index[a] = a < c.num_agents ? c.agent_index[a] : 0;
  p.max_range = lp.maximum_range;
  return p;
}

// NORMALIZE: LidarObservation(normalize=True), `obs /= self.maximum_range` (observation.py:706-707)
// CPL: cells per lane, 1 (cells <= 64: hwy_lidar_kernel's arrangement) or 4 (cells <= 256)
template <bool NORMALIZE, int CPL>
__global__ void __launch_bounds__(64) hwy_lidar_any_kernel(const LidarDoorParams p) {
  __shared__ double sh[LIDAR_PLANES][64];
  __shared__ int32_t sh_word[64];  // bit 31: the obstacle is traced; centre cell | start << 8 | end << 16
  const int lane = threadIdx.x;
  const int e = (int)blockIdx.x / p.A, a = (int)blockIdx.x % p.A;
  const size_t row = (size_t)e * p.pitch;
  const bool ix = p.scenario == HWY_SCENARIO_INTERSECTION;  // (its word holds the flags elsewhere: hwy_ix.h)
  int me = p.agent_index[a];
  if (ix) {  // the a-th present slot that carries HWY_F_CONTROLLED; N <= 64: one ballot
    const int f = lane < p.N ? ix_word_flags(p.packed[row + lane]) : HWY_F_ABSENT;
    unsigned long long mine = __ballot(!(f & HWY_F_ABSENT) && (f & HWY_F_CONTROLLED));
    for (int k = 0; k < a; ++k) mine &= mine - 1;
    me = mine ? __ffsll((long long)mine) - 1 : -1;
  }
  me = me < p.N ? me : -1;
  const int cells = p.cells;
  const double R = p.max_range;
  const double cell_angle = 2 * HWY_PI / cells;  // self.angle = 2 * np.pi / self.cells
  // observer: origin = position, origin_velocity = speed * [cos(heading), sin(heading)] (objects.py: RoadObject.velocity)
  const int mes = me < 0 ? 0 : me;
  const double ox = p.x[row + mes], oy = p.y[row + mes];
  double osn, ocs;
  sincos_bounded(p.heading[row + mes], &osn, &ocs);
  const double ospeed = p.speed[row + mes];
  const double ovx = ospeed * ocs, ovy = ospeed * osn;
  // my cells (phase 2): direction = [cos(index * angle), sin(index * angle)], ray = [origin, origin + maximum_range * direction]
  double dsn[CPL], dcs[CPL], qrx[CPL], qry[CPL], ray_len[CPL];
  lidar_cell_t gd[CPL], gv[CPL];
#pragma unroll
  for (int i = 0; i < CPL; ++i) {
    sincos_bounded((double)(lane + 64 * i) * cell_angle, &dsn[i], &dcs[i]);
    const double reach_x = R * dcs[i], reach_y = R * dsn[i];
    const double qx = ox + reach_x, qy = oy + reach_y;
    qrx[i] = qx - ox; qry[i] = qy - oy;  // q - r
    ray_len[i] = lidar_norm2(qrx[i], qry[i]);
    gd[i] = (lidar_cell_t)R; gv[i] = (lidar_cell_t)R;  // np.ones(..., float32) * maximum_range
  }

  for (int base = 0; base < p.N; base += 64) {
    // ---- phase 1: lane == obstacle ------------------------------------------------------------------------------------------
    const int j = base + lane;
    int32_t word = 0;
    const int flags = j < p.N ? (ix ? ix_word_flags(p.packed[row + j]) : word_flags(p.packed[row + j])) : HWY_F_ABSENT;
    if (me >= 0 && j < p.N && j != me && !(flags & HWY_F_ABSENT)) {
      const double px = p.x[row + j], py = p.y[row + j];
      double sn, cs;
      sincos_bounded(p.heading[row + j], &sn, &cs);
      const double speed = p.speed[row + j];
      const double dx = px - ox, dy = py - oy;
      const double center_distance = lidar_norm2(dx, dy);
      // rect_corners (utils.py:128-157): rotation @ [-hl - hw, -hl + hw, +hl + hw, +hl - hw] + center; a, b, c, d in that order
      const double hl = ((flags & HWY_F_OBSTACLE) ? HWY_OBSTACLE_LENGTH : HWY_VEH_LENGTH) / 2, hw = HWY_VEH_WIDTH / 2;
      const double lx[4] = {-hl, -hl, hl, hl}, ly[4] = {-hw, hw, hw, -hw};
      double cx[4], cy[4], ang[4];
      for (int k = 0; k < 4; ++k) {
        const double x1 = cs * lx[k], x2 = -sn * ly[k];
        const double y1 = sn * lx[k], y2 = cs * ly[k];
        cx[k] = (x1 + x2) + px;
        cy[k] = (y1 + y2) + py;
        ang[k] = atan2_bounded(cy[k] - oy, cx[k] - ox) + cell_angle / 2;  // position_to_angle
      }
      const bool in_range = !(center_distance > R);  // the CENTRE decides, whatever the corners do (observation.py:717-719)
      if (in_range) {
        const int center_index = lidar_angle_to_index(atan2_bounded(dy, dx) + cell_angle / 2, cell_angle, cells);
        const double distance = center_distance - HWY_VEH_WIDTH / 2;  // obstacle.WIDTH / 2: 1.0 for a vehicle and an Obstacle
        const double vx = speed * cs, vy = speed * sn;
        const double rvx = vx - ovx, rvy = vy - ovy;  // obstacle.velocity - origin_velocity
        double min_angle = fmin(fmin(ang[0], ang[1]), fmin(ang[2], ang[3]));
        double max_angle = fmax(fmax(ang[0], ang[1]), fmax(ang[2], ang[3]));
        if (min_angle < -HWY_PI / 2 && HWY_PI / 2 < max_angle) {  // the corners wrap around +-pi
          const double t = min_angle;
          min_angle = max_angle;
          max_angle = t + 2 * HWY_PI;
        }
        const int start = lidar_angle_to_index(min_angle, cell_angle, cells), end = lidar_angle_to_index(max_angle, cell_angle, cells);
        // distance_to_rect, the part that is the same for every ray: u = (b - a) / |b - a|, v = (d - a) / |d - a|, r = origin
        double ux = cx[1] - cx[0], uy = cy[1] - cy[0], vxx = cx[3] - cx[0], vyy = cy[3] - cy[0];
        const double nu = lidar_norm2(ux, uy), nv = lidar_norm2(vxx, vyy);
        ux = ux / nu; uy = uy / nu; vxx = vxx / nv; vyy = vyy / nv;
        sh[LIDAR_U_X][lane] = ux; sh[LIDAR_U_Y][lane] = uy; sh[LIDAR_V_X][lane] = vxx; sh[LIDAR_V_Y][lane] = vyy;
        sh[LIDAR_AU][lane] = lidar_dot2(cx[0] - ox, cy[0] - oy, ux, uy);
        sh[LIDAR_BU][lane] = lidar_dot2(cx[1] - ox, cy[1] - oy, ux, uy);
        sh[LIDAR_AV][lane] = lidar_dot2(cx[0] - ox, cy[0] - oy, vxx, vyy);
        sh[LIDAR_DV][lane] = lidar_dot2(cx[3] - ox, cy[3] - oy, vxx, vyy);
        sh[LIDAR_RVX][lane] = rvx; sh[LIDAR_RVY][lane] = rvy;
        sh[LIDAR_CDIST][lane] = distance;
        word = (int32_t)(0x80000000u | (unsigned)center_index | ((unsigned)start << 8) | ((unsigned)end << 16));
      }
    }
    sh_word[lane] = word;
    __syncthreads();
    // ---- phase 2: lane == cell(s); the obstacles of the pass in list order ---------------------------------------------------------
    if (lane < cells) {
      const int n = p.N - base < 64 ? p.N - base : 64;
      for (int k = 0; k < n; ++k) {
        const int32_t w = sh_word[k];
        if (w >= 0) continue;
        const int center_index = w & 0xff, start = (w >> 8) & 0xff, end = (w >> 16) & 0xff;
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
          const int c = lane + 64 * i;
          if (CPL > 1 && c >= cells) continue;
          // np.arange(start, end + 1) if start < end else [start .. cells - 1] + [0 .. end] (the corners wrap around cell 0)
          const bool in_sector = start < end ? (c >= start && c <= end) : (c >= start || c <= end);
          if (c != center_index && !in_sector) continue;
          const double rvx = sh[LIDAR_RVX][k], rvy = sh[LIDAR_RVY][k];
          const double velocity = lidar_dot2(rvx, rvy, dcs[i], dsn[i]);  // (obstacle.velocity - origin_velocity).dot(direction)
          if (c == center_index) lidar_fold(gd[i], gv[i], sh[LIDAR_CDIST][k], velocity);
          if (!in_sector) continue;
          // utils.distance_to_rect (utils.py:388-416), divisions by zero kept
          const double rqu = lidar_dot2(qrx[i], qry[i], sh[LIDAR_U_X][k], sh[LIDAR_U_Y][k]);
          const double rqv = lidar_dot2(qrx[i], qry[i], sh[LIDAR_V_X][k], sh[LIDAR_V_Y][k]);
          const double u0 = sh[LIDAR_AU][k] / rqu, u1 = sh[LIDAR_BU][k] / rqu;
          const double v0 = sh[LIDAR_AV][k] / rqv, v1 = sh[LIDAR_DV][k] / rqv;
          const double i1_lo = rqu >= 0 ? u0 : u1, i1_hi = rqu >= 0 ? u1 : u0;
          const double i2_lo = rqv >= 0 ? v0 : v1, i2_hi = rqv >= 0 ? v1 : v0;
          if (lidar_interval_distance(i1_lo, i1_hi, i2_lo, i2_hi) <= 0 && lidar_interval_distance(0, 1, i1_lo, i1_hi) <= 0 &&
              lidar_interval_distance(0, 1, i2_lo, i2_hi) <= 0) {
            const double first = i2_lo > i1_lo ? i2_lo : i1_lo;  // Python's max(interval_1[0], interval_2[0])
            lidar_fold(gd[i], gv[i], first * ray_len[i], velocity);
          }  // else: np.inf, which never passes `<=`
        }
      }
    }
    __syncthreads();
  }
  const float rf = (float)R;
#pragma unroll
  for (int i = 0; i < CPL; ++i) {
    const int c = lane + 64 * i;
    if (c >= cells) continue;
    float *out = p.obs + (((size_t)blockIdx.x) * cells + c) * 2;
    float od = (float)gd[i], ov = (float)gv[i];
    if (NORMALIZE) {  // on the float32 grid: a correctly rounded f32 division
      od = od / rf;
      ov = ov / rf;
    }
    out[0] = od;
    out[1] = ov;
  }
}

// ---- host side: the sequence of launches of hwy_rollout_lidar_device, written ONCE for hwy_engine.hip and the CPU emulation ----------
// k_steps (step launch, observe launch) pairs on block k of every plane -- the launches of k_steps single calls, the same results
// by construction.  ops.step(k), ops.observe(k), each returning 0 or the status the call returns.
template <typename Ops>
inline int lidar_door_rollout_sequence(Ops &&ops, int32_t k_steps) {
  for (int32_t k = 0; k < k_steps; ++k) {
    if (int rc = ops.step(k)) return rc;
    if (int rc = ops.observe(k)) return rc;
  }
  return 0;
}

}  // namespace hwy
