// hwy_act.h -- ContinuousAction.act (envs/common/action.py:136-163) for the plain-Vehicle egos of a direct-control engine, a kernel
// of its own: a float action of every (environment, agent) -> the stored (acceleration, steering) pair the direct step kernels
// drive on (DirectArgs::ctl_accel / ctl_steer, the planes of hwy_set_controls).
//
// No step / reset / observe kernel is touched.  DiscreteAction.act(i) is ContinuousAction.act(all_actions[i]) (action.py:189-196):
// where a DiscreteAction step looks the pair up in the engine's table on its first frame, a continuous step has this kernel write
// the pair and then runs the SAME step launch with no action ids -- the direct kernels then continue with the stored pair, which is
// Vehicle.act(dict) followed by the frames (what hwy_step_frames(actions = NULL) does today).
//
// One THREAD per (environment, agent) row r:
//   actions    f32 [rows][size]   size 2: throttle, steering; size 1: the one controlled axis
//   ctl_accel  f64 [rows]         ctl_steer f64 [rows]
//
// The mapping is ContinuousAction.get_action (action.py:136-158) as the reference computes it for a FLOAT32 action -- the dtype its
// space Box(-1, 1, (size,), float32) declares.  Under NumPy 2 every operation of utils.lmap (utils.py:31-33) then runs in float32,
// the Python-float range ends rounded to float32 where they meet the array value:
//   x   = min(max(v, -1f), 1f)            np.clip
//   r   = (float)(y1 - y0)                the difference in double, then rounded
//   t   = ((x + 1f) * r) / 2f             three float32 operations, each rounded
//   out = (double)((float)y0 + t)         float32 add; Vehicle.clip_actions float()s it (kinematics.py:159-160)
// Every operation is rounded on its own: the build contracts a * b + c written in ONE expression (-ffp-contract=on), so act_map
// below is one statement per operation, like direct_speed_update (hwy_device.h) for the same reason.
// An axis that is not controlled stores 0.0 (get_action's integer 0).  The range ends travel as the doubles the config holds; they
// are not re-derived from DirectArgs::accel_axis / steer_axis, whose entries are float32-rounded already.
// A row with a non-finite component leaves BOTH stored values of the row as they are -- the rule hwy_step_device has for an id
// outside the table; the host-pointer entry points reject such input before anything runs (HWY_ERR_ACTION).
// Nothing is skipped for an environment that awaits its next-step re-spawn: the episode start that follows zeroes its controls
// (Vehicle.__init__), as it does after a DiscreteAction step.
//
// Like hwy_mask.h this header includes no HIP runtime: hwy_kernels_act.hip includes <hip/hip_runtime.h> first, the CPU emulation
// (tests/emu/emu_continuous.cpp) its shim, hip_emu.h.  The launch rule is hwy_launch_units.h's (select_act_continuous), for both.
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/hwy_engine.h"

namespace hwy {

#define HWY_ACT_BLOCK 256  // threads of a workgroup: four wavefronts of (environment, agent) rows
#define HWY_ACT_MAX_STEERING (3.141592653589793 / 3.0)  // Vehicle.MAX_STEERING_ANGLE: what hwy_create holds steer_axis to

struct ActParams {
  const float *actions;           // [rows][size]
  double *ctl_accel, *ctl_steer;  // [rows] each
  int32_t rows, A, size, longitudinal, lateral, pad_;
  double accel_y0, accel_y1, steer_y0, steer_y1;  // ContinuousAction.acceleration_range / steering_range, as configured
};

// components of one action: 2 with both axes, 1 with one (action.py:117)
inline int act_size(const hwy_continuous_params &cp) { return (cp.longitudinal ? 1 : 0) + (cp.lateral ? 1 : 0); }

// host side: what the entry points accept.  Shared by hwy_engine.hip and the CPU emulation.
inline int act_validate(const hwy_config &c, const hwy_continuous_params *cp, const char **why) {
  *why = "";
  if (c.ego_control != HWY_EGO_DIRECT) {
    *why = "the engine's controlled vehicles store no controls (ego_control is HWY_EGO_META)";
    return HWY_ERR_INVALID_ARG;
  }
  if (!cp) {
    *why = "params must be non-NULL";
    return HWY_ERR_INVALID_ARG;
  }
  if (!cp->longitudinal && !cp->lateral) {  // action.py:108-111
    *why = "either longitudinal and/or lateral control must be enabled";
    return HWY_ERR_INVALID_ARG;
  }
  for (int k = 0; k < 2; ++k) {
    if (!(fabs(cp->acceleration_range[k]) < 1e6)) {
      *why = "acceleration_range must be finite";
      return HWY_ERR_INVALID_ARG;
    }
    if (!(fabs(cp->steering_range[k]) <= HWY_ACT_MAX_STEERING)) {  // (tan_bounded covers +-pi/3, like steer_axis)
      *why = "steering_range must lie within +-pi/3";
      return HWY_ERR_INVALID_ARG;
    }
  }
  return HWY_OK;
}

// host side: true when every one of the n floats is finite (the host-pointer entry points: HWY_ERR_ACTION otherwise)
inline bool act_all_finite(const float *a, size_t n) {
  for (size_t k = 0; k < n; ++k)
    if (!isfinite(a[k])) return false;
  return true;
}

// host side: the arguments of a config over the action rows and the planes of the stored controls (acceleration [E][A] | steering
// [E][A], the layout of hwy_params.h: direct_args)
inline ActParams act_params(const hwy_config &c, const hwy_continuous_params &cp, const float *actions, double *controls) {
  ActParams p;
  memset(&p, 0, sizeof p);
  p.actions = actions;
  p.ctl_accel = controls;
  p.ctl_steer = controls ? controls + (size_t)c.num_envs * c.num_agents : nullptr;
  p.rows = c.num_envs * c.num_agents; p.A = c.num_agents; p.size = act_size(cp);
  p.longitudinal = cp.longitudinal ? 1 : 0; p.lateral = cp.lateral ? 1 : 0;
  p.accel_y0 = cp.acceleration_range[0]; p.accel_y1 = cp.acceleration_range[1];
  p.steer_y0 = cp.steering_range[0]; p.steer_y1 = cp.steering_range[1];
  return p;
}

// utils.lmap(np.clip(v, -1, 1), [-1, 1], [y0, y1]) of a float32 v, operation by operation in float32 (see the head of the file)
__device__ inline double act_map(float v, double y0, double y1) {
  const float x = fminf(fmaxf(v, -1.0f), 1.0f);
  const float r = (float)(y1 - y0);
  const float s = x + 1.0f;
  const float m = s * r;
  const float t = m / 2.0f;
  const float o = (float)y0 + t;
  return (double)o;
}

// BLOCK: threads per workgroup (a template so that the header can be included by several translation units)
template <int BLOCK>
__global__ void __launch_bounds__(BLOCK) hwy_act_continuous_kernel(const ActParams p) {
  const int r = (int)blockIdx.x * BLOCK + (int)threadIdx.x;  // (environment, agent)
  if (r >= p.rows) return;
  const float *a = p.actions + (size_t)r * p.size;
  const float v0 = a[0], v1 = p.size > 1 ? a[1] : 0.0f;
  if (!__builtin_isfinite(v0) || !__builtin_isfinite(v1)) return;  // the stored pair stays
  double accel = 0.0, steer = 0.0;
  if (p.longitudinal) accel = act_map(v0, p.accel_y0, p.accel_y1);
  if (p.lateral) steer = act_map(p.longitudinal ? v1 : v0, p.steer_y0, p.steer_y1);
  p.ctl_accel[r] = accel;
  p.ctl_steer[r] = steer;
}

}  // namespace hwy
