// hwy_launch_units.h -- arguments -> (precondition check, kernel instantiation, grid, block, LDS) of the add-on kernel units beside
// the step kernels -- the Lidar trace (hwy_lidar.h), the TTC grid and planner (hwy_ttc.h), fork and score (hwy_lookahead.h), the OPD
// tree (hwy_opd.h), the action mask (hwy_mask.h), the continuous action (hwy_act.h), the CEM planner (hwy_cem.h) the TimeToCollision observation (hwy_collision_obs.h) and the Lidar door (hwy_lidar_door.h) -- written ONCE for the product and for the
// CPU emulation of tests/emu, like hwy_launch_family.h for the step families.  Host code only, generic over the thing that launches: a backend B with one member
//   B::launch_plain(kernel, grid, block, lds, stream, args)   enqueue / run the kernel; no dispatch timestamps (those of
//                                                             hwy_profile_* belong to the step kernel)
// hwy_launch.h: HipBackend (hipLaunchKernelGGL); tests/emu/hip_emu.h: emu::PlainBackend (emu::launch).  Nothing here needs
// hwy::Launch or a step kernel's header.
// A unit's section compiles when the unit's kernel header has been included BEFORE this one (each kernel translation unit and each
// emulator library holds the kernels of one unit and includes no other unit's headers), so: include the unit header(s), then this.
// Every function refuses arguments outside what its kernel is built for with hipErrorInvalidValue and launches nothing then.
// hipError_t / hipStream_t come from the HIP runtime (the emulation: from hip_emu.h).

// ---- LidarObservation (hwy_lidar.h): `rows` (environment, agent) pairs, one wavefront each, row r -> lp.obs + r * cells * 2 ---------
#if defined(HWY_LIDAR_UNIT) && !defined(HWY_LAUNCH_LIDAR_UNIT)
#define HWY_LAUNCH_LIDAR_UNIT
namespace hwy {
template <typename B> hipError_t select_lidar(const LidarParams &lp, bool normalize, int rows, hipStream_t stream) {
  if (rows < 1 || lp.cells < 1 || lp.cells > HWY_MAX_LIDAR_CELLS) return hipErrorInvalidValue;
  return normalize ? B::launch_plain(hwy_lidar_kernel<true>, rows, 64, 0, stream, lp)
                   : B::launch_plain(hwy_lidar_kernel<false>, rows, 64, 0, stream, lp);
}
}  // namespace hwy
#endif

// ---- time-to-collision grid and, with `plan`, the value iteration on it (hwy_ttc.h): `rows` (environment, agent) pairs, one
// wavefront each.  The grid lives in LDS at one dword per cell: two capacity classes, so that the common shapes (<= 1024 cells: 4 KB)
// keep many workgroups per CU and only the largest grids (up to 8 x 16 x 64 cells: 32 KB) pay for theirs.
#if defined(HWY_TTC_SMALL_CELLS) && !defined(HWY_LAUNCH_TTC_UNIT)
#define HWY_LAUNCH_TTC_UNIT
namespace hwy {
template <typename B> hipError_t select_ttc(const TtcParams &tp, bool plan, int rows, hipStream_t stream) {
  const int cells = tp.V * tp.L * tp.T;
  if (rows < 1 || tp.V < 1 || tp.V > HWY_MAX_TARGET_SPEEDS || tp.L < 1 || tp.L > HWY_MAX_LANES || tp.T < 1 || tp.T > HWY_MAX_TTC_STEPS ||
      tp.N < 1 || tp.N > HWY_MAX_VEHICLES || (plan ? !tp.action : !tp.grid))
    return hipErrorInvalidValue;
  const bool small = cells <= HWY_TTC_SMALL_CELLS;
  if (plan) return small ? B::launch_plain(hwy_ttc_kernel<HWY_TTC_SMALL_CELLS, true>, rows, 64, 0, stream, tp)
                         : B::launch_plain(hwy_ttc_kernel<HWY_TTC_MAX_CELLS, true>, rows, 64, 0, stream, tp);
  return small ? B::launch_plain(hwy_ttc_kernel<HWY_TTC_SMALL_CELLS, false>, rows, 64, 0, stream, tp)
               : B::launch_plain(hwy_ttc_kernel<HWY_TTC_MAX_CELLS, false>, rows, 64, 0, stream, tp);
}
}  // namespace hwy
#endif

// ---- environment fork (hwy_lookahead.h: one workgroup per destination environment) and the fold of a rollout's outputs (one
// wavefront per environment group) -------------------------------------------------------------------------------------------------
#if defined(HWY_FORK_THREADS) && !defined(HWY_LAUNCH_LOOKAHEAD_UNIT)
#define HWY_LAUNCH_LOOKAHEAD_UNIT
namespace hwy {
template <typename B> hipError_t select_fork(const ForkParams &fp, hipStream_t stream) {
  if (fp.dst_envs < 1 || fp.src_envs < 1 || fp.branches < 1 || fp.pitch < 1 || fp.n_f64 < 0 || fp.n_f64 > HWY_FORK_MAX_F64_PLANES ||
      fp.n_i32 < 0 || fp.n_i32 > HWY_FORK_MAX_I32_PLANES || fp.A < 1 || 2 * fp.A > HWY_FORK_THREADS ||
      (!fp.src_env && (long long)fp.src_envs * fp.branches < fp.dst_envs))
    return hipErrorInvalidValue;
  return B::launch_plain(hwy_fork_kernel<HWY_FORK_THREADS>, fp.dst_envs, HWY_FORK_THREADS, 0, stream, fp);
}
template <typename B> hipError_t select_score(const ScoreParams &sp, hipStream_t stream) {
  if (sp.groups < 1 || sp.branches < 1 || sp.K < 1 || sp.A < 1 || sp.n_ids < 1 || sp.n_ids > HWY_SCORE_MAX_IDS || !sp.reward ||
      !sp.terminated || !sp.truncated)
    return hipErrorInvalidValue;
  return B::launch_plain(hwy_score_kernel<HWY_SCORE_MAX_IDS>, sp.groups, 64, 0, stream, sp);
}
}  // namespace hwy
#endif

// ---- one step of the optimistic planner's tree (hwy_opd.h: ingest, backup, selection or the plan; op.E wavefronts); masked when the
// two arrays of the masked search are set ----------------------------------------------------------------------------------------------
#if defined(HWY_OPD_MAX_NODES) && !defined(HWY_LAUNCH_OPD_UNIT)
#define HWY_LAUNCH_OPD_UNIT
namespace hwy {
template <typename B> hipError_t select_opd(const OpdParams &op, hipStream_t stream) {
  if (op.E < 1 || op.n < 1 || op.X < 1 || op.x < 0 || op.x > op.X || op.M != 1 + op.X * op.n || op.M > HWY_OPD_MAX_NODES || !op.ret ||
      !op.disc || !op.upper0 || !op.done || !op.expanded_node || !op.reward || !op.terminated || !op.truncated || !op.gather_src ||
      !op.scatter_src || !op.root_src || !op.actions || !op.action)
    return hipErrorInvalidValue;
  if ((op.child_mask != nullptr) != (op.created != nullptr)) return hipErrorInvalidValue;
  return op.created ? B::launch_plain(hwy_opd_masked_kernel<HWY_OPD_MAX_NODES>, op.E, 64, 0, stream, op)
                    : B::launch_plain(hwy_opd_kernel<HWY_OPD_MAX_NODES>, op.E, 64, 0, stream, op);
}
}  // namespace hwy
#endif

// ---- action mask (hwy_mask.h): mp.rows (environment, agent) pairs, one thread each, row r -> mp.mask + r * n_ids ---------------------
#if defined(HWY_MASK_BLOCK) && !defined(HWY_LAUNCH_MASK_UNIT)
#define HWY_LAUNCH_MASK_UNIT
namespace hwy {
template <typename B> hipError_t select_mask(const MaskParams &mp, hipStream_t stream) {
  if (mp.rows < 1 || mp.A < 1 || mp.N < 1 || mp.N > mp.pitch || mp.n_lanes < 0 || mp.n_lanes > HWY_MAX_LANES || !mp.x || !mp.y ||
      !mp.packed || !mp.mask || mp.n_ids != HWY_NUM_ACTIONS(mp.action_set))
    return hipErrorInvalidValue;
  const int blocks = (mp.rows + HWY_MASK_BLOCK - 1) / HWY_MASK_BLOCK;
  return B::launch_plain(hwy_mask_kernel<HWY_MASK_BLOCK>, blocks, HWY_MASK_BLOCK, 0, stream, mp);
}
}  // namespace hwy
#endif

// ---- continuous action (hwy_act.h): ap.rows (environment, agent) rows, one thread each, row r -> ap.ctl_accel[r], ap.ctl_steer[r] ------
#if defined(HWY_ACT_BLOCK) && !defined(HWY_LAUNCH_ACT_UNIT)
#define HWY_LAUNCH_ACT_UNIT
namespace hwy {
template <typename B> hipError_t select_act_continuous(const ActParams &ap, hipStream_t stream) {
  if (ap.rows < 1 || ap.A < 1 || ap.rows % ap.A != 0 || !ap.actions || !ap.ctl_accel || !ap.ctl_steer || (!ap.longitudinal && !ap.lateral) ||
      ap.size != (ap.longitudinal ? 1 : 0) + (ap.lateral ? 1 : 0))
    return hipErrorInvalidValue;
  const int blocks = (ap.rows + HWY_ACT_BLOCK - 1) / HWY_ACT_BLOCK;
  return B::launch_plain(hwy_act_continuous_kernel<HWY_ACT_BLOCK>, blocks, HWY_ACT_BLOCK, 0, stream, ap);
}
}  // namespace hwy
#endif

// ---- CEM planner (hwy_cem.h): the sample kernel, one thread per (environment, branch, step) of iteration cp.iter, and the refit, one
// wavefront per environment behind the score kernel that wrote cp.ret -------------------------------------------------------------------
#if defined(HWY_CEM_BLOCK) && !defined(HWY_LAUNCH_CEM_UNIT)
#define HWY_LAUNCH_CEM_UNIT
namespace hwy {
inline bool cem_shape_ok(const CemParams &cp) {
  return cp.E >= 1 && cp.B >= 1 && cp.B <= HWY_CEM_MAX_POP && cp.K >= 1 && cp.K <= HWY_CEM_MAX_HORIZON && (cp.size == 1 || cp.size == 2) &&
         cp.M >= 1 && cp.M <= cp.B && cp.I >= 1 && cp.I <= HWY_CEM_MAX_ITERATIONS && cp.iter >= 0 && cp.iter < cp.I &&
         (long long)cp.E * cp.B <= 0x7fffffffll && cp.actions && cp.mean && cp.stddev;
}
template <typename B> hipError_t select_cem_sample(const CemParams &cp, hipStream_t stream) {
  if (!cem_shape_ok(cp)) return hipErrorInvalidValue;
  const long long threads = (long long)cp.E * cp.B * cp.K;
  const long long blocks = (threads + HWY_CEM_BLOCK - 1) / HWY_CEM_BLOCK;
  if (blocks > 0x7fffffffll) return hipErrorInvalidValue;
  return B::launch_plain(hwy_cem_sample_kernel<HWY_CEM_BLOCK>, (unsigned)blocks, HWY_CEM_BLOCK, 0, stream, cp);
}
template <typename B> hipError_t select_cem_refit(const CemParams &cp, hipStream_t stream) {
  if (!cem_shape_ok(cp) || !cp.ret || !cp.best_return || !cp.best_sequence || !cp.action) return hipErrorInvalidValue;
  return B::launch_plain(hwy_cem_refit_kernel<HWY_CEM_MAX_POP>, cp.E, 64, 0, stream, cp);
}
}  // namespace hwy
#endif

// ---- TimeToCollision observation (hwy_collision_obs.h): `rows` (environment, agent) pairs, one wavefront each, row r ->
// cp.obs + r * 9 * T.  The window's nine rows live in LDS at one dword per cell (static, 576 dwords): one class for every V and L.
#if defined(HWY_COLLISION_OBS_CELLS) && !defined(HWY_LAUNCH_COLLISION_OBS_UNIT)
#define HWY_LAUNCH_COLLISION_OBS_UNIT
namespace hwy {
template <typename B> hipError_t select_collision_obs(const CollisionObsParams &cp, int rows, hipStream_t stream) {
  if (rows < 1 || cp.A < 1 || rows % cp.A != 0 || cp.V < 2 || cp.V > HWY_MAX_TARGET_SPEEDS || cp.L < 1 || cp.L > HWY_MAX_LANES || cp.T < 1 ||
      cp.T > HWY_MAX_TTC_STEPS || cp.N < 1 || cp.N > HWY_MAX_VEHICLES || cp.N > cp.pitch || !cp.x || !cp.heading || !cp.speed || !cp.packed ||
      !cp.obs)
    return hipErrorInvalidValue;
  return B::launch_plain(hwy_collision_obs_kernel<HWY_COLLISION_OBS_CELLS>, rows, 64, 0, stream, cp);
}
}  // namespace hwy
#endif

// ---- Lidar through a door of its own (hwy_lidar_door.h): `rows` (environment, agent) pairs, one wavefront each, row r ->
// lp.obs + r * cells * 2.  Cells per lane: 1 up to 64 cells (hwy_lidar_kernel's arrangement), 4 up to 256.  The observer of an
// intersection state is found by one ballot: N <= 64 there.
#if defined(HWY_LIDAR_DOOR_UNIT) && !defined(HWY_LAUNCH_LIDAR_DOOR_UNIT)
#define HWY_LAUNCH_LIDAR_DOOR_UNIT
namespace hwy {
template <typename B> hipError_t select_lidar_door(const LidarDoorParams &lp, bool normalize, int rows, hipStream_t stream) {
  if (rows < 1 || lp.A < 1 || lp.A > HWY_MAX_AGENTS || rows % lp.A != 0 || lp.cells < 1 || lp.cells > HWY_LIDAR_DOOR_MAX_CELLS || lp.N < 1 ||
      lp.N > HWY_MAX_VEHICLES || lp.N > lp.pitch || (lp.scenario == HWY_SCENARIO_INTERSECTION && lp.N > 64) || !(lp.max_range > 0) || !lp.x ||
      !lp.y || !lp.heading || !lp.speed || !lp.packed || !lp.obs)
    return hipErrorInvalidValue;
  if (lp.cells <= 64)
    return normalize ? B::launch_plain(hwy_lidar_any_kernel<true, 1>, rows, 64, 0, stream, lp)
                     : B::launch_plain(hwy_lidar_any_kernel<false, 1>, rows, 64, 0, stream, lp);
  return normalize ? B::launch_plain(hwy_lidar_any_kernel<true, 4>, rows, 64, 0, stream, lp)
                   : B::launch_plain(hwy_lidar_any_kernel<false, 4>, rows, 64, 0, stream, lp);
}
}  // namespace hwy
#endif

// ---- SameStep stash (hwy_same_step.h): fp.E workgroups, one per environment; the workgroup size by the length of a row ---------------
#if defined(HWY_FINAL_BLOCK) && !defined(HWY_LAUNCH_FINAL_UNIT)
#define HWY_LAUNCH_FINAL_UNIT
namespace hwy {
template <typename B> hipError_t select_final(const FinalParams &fp, hipStream_t stream) {
  if (fp.E < 1 || fp.A < 1 || fp.row_floats < 1 || !fp.done || !fp.final_mask || !fp.obs || !fp.final_obs ||
      (fp.info_speed != nullptr) != (fp.final_info_speed != nullptr) || (fp.info_crashed != nullptr) != (fp.final_info_crashed != nullptr) ||
      (fp.vec4 && fp.row_floats % 4 != 0))
    return hipErrorInvalidValue;
  return fp.row_floats <= HWY_FINAL_SMALL_FLOATS ? B::launch_plain(hwy_final_kernel<HWY_FINAL_BLOCK>, fp.E, HWY_FINAL_BLOCK, 0, stream, fp)
                                                 : B::launch_plain(hwy_final_kernel<HWY_FINAL_BLOCK_LARGE>, fp.E, HWY_FINAL_BLOCK_LARGE, 0, stream, fp);
}
}  // namespace hwy
#endif
