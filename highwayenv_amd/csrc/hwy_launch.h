// hwy_launch.h -- host-visible launch functions of the kernels in hwy_kernels.hip, hwy_kernels_linear.hip and
// hwy_kernels_direct.hip: one overload per kernel family, chosen by the type of its parameter struct; and of the add-on units
// (hwy_kernels_lidar.hip, _ttc.hip, _lookahead.hip, _opd.hip, _mask.hip, _act.hip, _cem.hip, _collision_obs.hip, _lidar_door.hip).  Each is the shared selection layer (hwy_launch_family.h,
// hwy_launch_rules.h; the add-on units: hwy_launch_units.h) with the HIP backend below.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include "hwy_launch_family.h"
#include "hwy_net.h"
#include "hwy_ix.h"
#include "hwy_lidar.h"
#include "hwy_ttc.h"
#include "hwy_lookahead.h"
#include "hwy_opd.h"
#include "hwy_mask.h"
#include "hwy_act.h"
#include "hwy_cem.h"
#include "hwy_collision_obs.h"
#include "hwy_lidar_door.h"
#include "hwy_same_step.h"
#include "hwy_launch_units.h"

namespace hwy {
// The HIP backend of the selection layer (hwy_launch_family.h, hwy_launch_rules.h, hwy_launch_units.h), for the kernel translation
// units.
struct HipBackend {
  // Kernel timing (hwy_profile_enable, the turn tuner): every launch goes through hipExtLaunchKernelGGL, which records the DISPATCH's
  // own begin and end timestamps into the two events of the Launch -- the same clock readings rocprofv3 --kernel-trace reports, with
  // no stream overhead between them (events recorded around a launch with hipEventRecord also measure ~3 us of command processing).
  // Null events (the normal case): a plain launch.
  template <typename K, typename... A>
  static hipError_t launch(K kernel, unsigned grid, int block, int lds, const Launch &l, const A &...a) {
    hipExtLaunchKernelGGL(kernel, dim3(grid), dim3(block), lds, l.stream, l.start, l.stop, 0, a...);
    return hipGetLastError();
  }
  // The add-on units (hwy_launch_units.h): a plain launch, never the timed path.
  template <typename K, typename A>
  static hipError_t launch_plain(K kernel, unsigned grid, int block, int lds, hipStream_t stream, const A &a) {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), lds, stream, a);
    return hipGetLastError();
  }
  // How many workgroups of a kernel the device holds at once (occupancy x compute units): the issue-priority turns (hwy_wave.h:
  // WaveTurn) only pay when the whole grid is resident.
  template <typename K>
  static int resident(K kernel, int block, int lds) {
    int per_cu = 0, dev = 0;
    hipDeviceProp_t prop;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, block, lds) != hipSuccess) return 0;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return 0;
    return per_cu * prop.multiProcessorCount;
  }
  template <typename Fn>
  static auto pick_wpe(int v, Fn &&fn) { return dispatch_1_4(v, fn); }
};
// the shape kernels of the one-wavefront step (hwy_wave.h: FixedShape) and their launch: hwy_kernels_shapes.hip
extern template hipError_t launch_step_shape<HipBackend>(int, const StepParams &, const Launch &);
// One overload per kernel family, chosen by the type of its parameter struct; `l`: hwy_launch_family.h.
// Straight road, IDM traffic and meta-actions (hwy_kernels.hip): the one-wavefront kernel for N <= 64, the wide kernel of hwy_wave2.h
// for 64 < N <= 256 with the Kinematics observation, the workgroup kernel otherwise or when forced.
// The Linear traffic family (hwy_config.traffic_model == HWY_TRAFFIC_LINEAR, hwy_kernels_linear.hip) and direct ego control
// (hwy_config.ego_control == HWY_EGO_DIRECT, hwy_kernels_direct.hip): the one-wavefront kernel for N <= 64 (unless
// force_block_kernel), the workgroup kernel otherwise -- hwy_wave2.h is IDM-only and has no DirectEgo form.
// Road-network scenarios (hwy_net.h) and the intersection scenario (hwy_ix.h): one wavefront per environment.
hipError_t launch_step(const StepParams &p, const Launch &l);
hipError_t launch_step(const LinearParams &lp, const Launch &l);
hipError_t launch_step(const DirectParams &dp, const Launch &l);
hipError_t launch_step(const NetParams &np, const Launch &l);
hipError_t launch_step(const IxParams &ip, const Launch &l);
// s.k_steps policy steps per launch (hwy_rollout_device)
hipError_t launch_rollout(const StepParams &p, const Launch &l);
hipError_t launch_rollout(const LinearParams &lp, const Launch &l);
hipError_t launch_rollout(const DirectParams &dp, const Launch &l);
hipError_t launch_rollout(const NetParams &np, const Launch &l);
hipError_t launch_rollout(const IxParams &ip, const Launch &l);
hipError_t launch_reset(const StepParams &p, const Launch &l);
hipError_t launch_reset(const LinearParams &lp, const Launch &l);
hipError_t launch_reset(const DirectParams &dp, const Launch &l);
hipError_t launch_reset(const NetParams &np, const Launch &l);
hipError_t launch_reset(const IxParams &ip, const Launch &l);
// the re-spawn of the environments that ended in the step launch before it (hwy_step_same_step_device; hwy_kernels_respawn.hip).
// The intersection scenario has none: its next episodes are pre-warmed in shadow planes (the entry point refuses it before).
hipError_t launch_respawn(const StepParams &p, const Launch &l);
hipError_t launch_respawn(const LinearParams &lp, const Launch &l);
hipError_t launch_respawn(const DirectParams &dp, const Launch &l);
hipError_t launch_respawn(const NetParams &np, const Launch &l);
inline hipError_t launch_respawn(const IxParams &, const Launch &) { return hipErrorInvalidValue; }
// (the observation of a straight road does not depend on the traffic model or the ego control)
hipError_t launch_observe(const StepParams &p, const Launch &l);
inline hipError_t launch_observe(const LinearParams &lp, const Launch &l) { return launch_observe(lp.s, l); }
inline hipError_t launch_observe(const DirectParams &dp, const Launch &l) { return launch_observe(dp.s, l); }
hipError_t launch_observe(const NetParams &np, const Launch &l);
hipError_t launch_observe(const IxParams &ip, const Launch &l);
// workgroups of the step kernel the device holds at once (0 = unknown / not applicable)
int step_resident_blocks(const StepParams &p, const Launch &l);
int step_resident_blocks(const LinearParams &lp, const Launch &l);
int step_resident_blocks(const DirectParams &dp, const Launch &l);
int step_resident_blocks(const NetParams &np, const Launch &l);
inline int step_resident_blocks(const IxParams &, const Launch &) { return 0; }
// LidarObservation of the current state (hwy_lidar.h): `rows` = environments x agents wavefronts, row r -> lp.obs + r * cells * 2
hipError_t launch_lidar(const LidarParams &lp, bool normalize, int rows, hipStream_t stream);
// Time-to-collision grid of the current state and, with `plan`, the value iteration on it (hwy_ttc.h): `rows` = environments x agents
// wavefronts, row r -> tp.grid + r * V * L * T, tp.action + r, tp.q + r * 5
hipError_t launch_ttc(const TtcParams &tp, bool plan, int rows, hipStream_t stream);
// Environment fork (hwy_lookahead.h: a gather copy between the planes of two engines, fp.dst_envs workgroups) and the fold of a
// rollout's outputs into returns, per-action maxima and the best first action / branch (sp.groups wavefronts)
hipError_t launch_fork(const ForkParams &fp, hipStream_t stream);
hipError_t launch_score(const ScoreParams &sp, hipStream_t stream);
// One step of the optimistic planner's tree (hwy_opd.h: ingest, backup, selection or the plan; op.E wavefronts)
hipError_t launch_opd(const OpdParams &op, hipStream_t stream);
// Action mask of the current state (hwy_mask.h, hwy_kernels_mask.hip: one thread per (environment, agent), row r -> mp.mask + r * n_ids)
hipError_t launch_mask(const MaskParams &mp, hipStream_t stream);
// ContinuousAction.act into the stored controls of a direct-control engine (hwy_act.h, hwy_kernels_act.hip: one thread per (environment,
// agent), row r of ap.actions -> ap.ctl_accel[r], ap.ctl_steer[r])
hipError_t launch_act_continuous(const ActParams &ap, hipStream_t stream);
// The CEM planner's two kernels (hwy_cem.h, hwy_kernels_cem.hip): the samples of iteration cp.iter (one thread per (environment, branch,
// step)) and the refit behind the score kernel (cp.E wavefronts)
hipError_t launch_cem_sample(const CemParams &cp, hipStream_t stream);
hipError_t launch_cem_refit(const CemParams &cp, hipStream_t stream);
// TimeToCollision observation of the current state (hwy_collision_obs.h, hwy_kernels_collision_obs.hip): `rows` = environments x agents
// wavefronts, row r -> cp.obs + r * 9 * T
hipError_t launch_collision_obs(const CollisionObsParams &cp, int rows, hipStream_t stream);
// Lidar through a door of its own (hwy_lidar_door.h, hwy_kernels_lidar_door.hip): `rows` = environments x agents wavefronts, row r ->
// lp.obs + r * cells * 2
hipError_t launch_lidar_door(const LidarDoorParams &lp, bool normalize, int rows, hipStream_t stream);
// SameStep stash (hwy_same_step.h, hwy_kernels_final.hip: one workgroup per environment, the rows of those that ended -> the final planes)
hipError_t launch_final(const FinalParams &fp, hipStream_t stream);
hipError_t launch_math_probe(int op, const double *in, double *out, long long n, hipStream_t stream);
}  // namespace hwy
