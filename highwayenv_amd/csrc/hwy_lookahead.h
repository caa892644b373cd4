// hwy_lookahead.h -- the two kernels of the simulator-based planning seam of the highway scenario: what the reference's planners do
// with copy.deepcopy(env) (AbstractEnv.__deepcopy__, envs/common/abstract.py:455) followed by env.step on the copy.
//
//   hwy_fork_kernel   a gather copy of environment state between two engines: destination environment j takes every plane a later
//                     step can read from source environment src_env[j] (or j / branches).  One workgroup per destination
//                     environment, thread == column along the pitch: every destination byte is written once, with coalesced
//                     f64 / i32 stores; the `branches` reads of one source row hit L2 after the first.  Columns >= N are copied as
//                     they are.  A source index outside [0, src_envs) copies nothing (the device form does not validate them).
//   hwy_score_kernel  folds the outputs of a K-step rollout of E x branches environments (environment e * branches + b == branch b
//                     of group e) into discounted returns, their maximum per first action and the best first action / branch.
//                     One 64-wide wavefront per group, lane == branch in passes of 64.  The maxima are taken on an order-preserving
//                     integer key of the f64 return with LDS atomic max, and the index among the holders of a maximum with LDS
//                     atomic min (the idiom of hwy_ix.h's closest-lane search): neither depends on the order of lanes or passes,
//                     and the tie rule is "lowest index wins" (numpy's argmax).
//
// The return of a branch: an episode that ends is absorbing -- the terminal step's reward counts, nothing after it does (the branch
// engine runs with auto-reset off, so the step kernels go on stepping the wreck).  The product d * r and the sum g + t are separate
// statements, so -ffp-contract=on fuses nothing: the returns are bit for bit what numpy computes by the same recurrence.
//
// Like hwy_ttc.h this header includes no HIP runtime: hwy_kernels_lookahead.hip includes <hip/hip_runtime.h> first, the CPU
// emulation (tests/emu/emu_lookahead.cpp, emu_opd.cpp) its shim, hip_emu.h.  The launch rules of the two kernels are
// hwy_launch_units.h's, for both.
#pragma once

#include <stdint.h>
#include <string.h>

#include "../../include/hwy_engine.h"

namespace hwy {

#define HWY_FORK_MAX_F64_PLANES (9 + HWY_BEHAVIOR_PARAMS)  // the nine state planes + the Linear family's behaviour planes
#define HWY_FORK_MAX_I32_PLANES 4                          // the engine: `packed`; the CPU emulation: lane | target | speed index | flags
#define HWY_FORK_THREADS 256
#define HWY_SCORE_MAX_IDS 256                              // HWY_MAX_ACTIONS_PER_AXIS squared

struct ForkParams {
  const double *src_f64[HWY_FORK_MAX_F64_PLANES];  // [src_envs][pitch] each
  double *dst_f64[HWY_FORK_MAX_F64_PLANES];        // [dst_envs][pitch]
  const int32_t *src_i32[HWY_FORK_MAX_I32_PLANES];
  int32_t *dst_i32[HWY_FORK_MAX_I32_PLANES];
  const double *src_controls;   // [2][src_envs][A] (direct ego control), or null
  double *dst_controls;         // [2][dst_envs][A]
  const double *src_time;       // [src_envs]
  double *dst_time;
  const uint32_t *src_episode;  // [src_envs]
  uint32_t *dst_episode;
  uint8_t *dst_done;            // [dst_envs], cleared
  const int32_t *src_env;       // [dst_envs] or null: j / branches
  int32_t n_f64, n_i32, pitch, A, branches, src_envs, dst_envs;
};

struct ScoreParams {
  const int32_t *first_action;  // [E * branches][A]
  const double *reward;         // [K][E * branches][A]
  const uint8_t *terminated, *truncated;  // [K][E * branches]
  double *ret;                  // [E][branches][A]  (may be null)
  double *q;                    // [E][n_ids]        (may be null)
  int32_t *best_action;         // [E]               (may be null)
  int32_t *best_branch;         // [E][A]            (may be null)
  double gamma;
  int32_t K, branches, A, n_ids, groups;
};

// ids of the configured action table: [0, n)
inline int lookahead_num_ids(const hwy_config &c) {
  if (c.ego_control == HWY_EGO_DIRECT) return c.n_accel * c.n_steer;
  return c.scenario == HWY_SCENARIO_INTERSECTION ? 3 : HWY_NUM_ACTIONS(c.action_set);
}

// host side: what hwy_fork_device accepts (include/hwy_engine.h).  Shared by hwy_engine.hip and the CPU emulation.
inline int fork_validate(const hwy_config &dst, const hwy_config &src, bool same_engine, int32_t branches, bool has_src_env, const char **why) {
  *why = "";
  if (dst.scenario != HWY_SCENARIO_HIGHWAY || src.scenario != HWY_SCENARIO_HIGHWAY) {
    *why = "environments are forked on the highway scenario only (the merge and intersection scenarios are outside the hot-path scope)";
    return HWY_ERR_UNSUPPORTED;
  }
  if (same_engine) { *why = "dst and src must be different engines"; return HWY_ERR_INVALID_ARG; }
  if (branches < 1) { *why = "branches must be >= 1"; return HWY_ERR_INVALID_ARG; }
  hwy_config a = dst, b = src;  // equal in every field that is not num_envs or tune_*
  hwy_config *both[2] = {&a, &b};
  for (hwy_config *c : both) {
    c->num_envs = 0;
    c->tune_block_kernel = c->tune_waves_per_eu = c->tune_ix_no_helpers = c->tune_ix_no_prewarm = 0;
    c->tune_extra_lds = c->tune_prio_shift = c->tune_ix_prewarm_frames = 0;
    c->tune_reserved[0] = 0;
  }
  if (memcmp(&a, &b, sizeof a) != 0) { *why = "the two engines' configs differ in a field other than num_envs / tune_*"; return HWY_ERR_INVALID_ARG; }
  if (!has_src_env && (int64_t)dst.num_envs != (int64_t)src.num_envs * branches) {
    *why = "dst.num_envs must be src.num_envs * branches when no source indices are given";
    return HWY_ERR_INVALID_ARG;
  }
  return HWY_OK;
}

// host side: what hwy_score_device accepts
inline int score_validate(const hwy_config &c, int32_t k_steps, int32_t branches, double gamma, bool has_first, bool has_reward_and_flags,
                          bool has_q, bool has_best_action, const char **why) {
  *why = "";
  if (c.scenario != HWY_SCENARIO_HIGHWAY) {
    *why = "action sequences are scored on the highway scenario only (the merge and intersection scenarios are outside the hot-path scope)";
    return HWY_ERR_UNSUPPORTED;
  }
  if (k_steps < 1) { *why = "k_steps must be >= 1"; return HWY_ERR_INVALID_ARG; }
  if (branches < 1 || c.num_envs % branches != 0) { *why = "branches must be >= 1 and divide num_envs"; return HWY_ERR_INVALID_ARG; }
  if (!(gamma > -1e30 && gamma < 1e30)) { *why = "gamma must be finite"; return HWY_ERR_INVALID_ARG; }
  if (!has_reward_and_flags) { *why = "reward / terminated / truncated must be non-NULL"; return HWY_ERR_INVALID_ARG; }
  if ((has_q || has_best_action) && c.num_agents > 1) { *why = "q and best_action need a single agent (A == 1)"; return HWY_ERR_INVALID_ARG; }
  if ((has_q || has_best_action) != has_first) { *why = "first_action must be NULL iff q and best_action are NULL"; return HWY_ERR_INVALID_ARG; }
  if (lookahead_num_ids(c) > HWY_SCORE_MAX_IDS) { *why = "action table too large"; return HWY_ERR_INVALID_ARG; }
  return HWY_OK;
}

// host side: the planes of ONE engine that a fork reads or writes ([envs][pitch] each, envs = cfg->num_envs).  The engine passes its
// packed words (n_i32 = 1: whole words, the rank hint travels), the CPU emulation its four integer planes lane | target | speed
// index | flags (n_i32 = 4).
struct ForkView {
  const hwy_config *cfg;
  double *f64[9];      // x | y | heading | speed | timer | target_speed | delta | impact_x | impact_y
  double *behavior;    // [HWY_BEHAVIOR_PARAMS][envs][pitch] of a Linear engine
  int32_t *i32[HWY_FORK_MAX_I32_PLANES];
  int32_t n_i32;
  double *controls;    // [2][envs][A] of a direct-control engine
  double *time;        // [envs]
  uint32_t *episode;   // [envs]
  uint8_t *done;       // [envs]
  int32_t pitch;
};
// ... and the arguments of a fork between two of them (fork_validate has passed: the configs agree)
inline ForkParams fork_params(const ForkView &dst, const ForkView &src, int32_t branches, const int32_t *src_env) {
  ForkParams p;
  memset(&p, 0, sizeof p);
  const size_t splane = (size_t)src.cfg->num_envs * src.pitch, dplane = (size_t)dst.cfg->num_envs * dst.pitch;
  for (int f = 0; f < 9; ++f) { p.src_f64[f] = src.f64[f]; p.dst_f64[f] = dst.f64[f]; }
  p.n_f64 = 9;
  if (dst.cfg->traffic_model == HWY_TRAFFIC_LINEAR)
    for (int f = 0; f < HWY_BEHAVIOR_PARAMS; ++f, ++p.n_f64) { p.src_f64[9 + f] = src.behavior + f * splane; p.dst_f64[9 + f] = dst.behavior + f * dplane; }
  for (int f = 0; f < dst.n_i32; ++f) { p.src_i32[f] = src.i32[f]; p.dst_i32[f] = dst.i32[f]; }
  p.n_i32 = dst.n_i32;
  if (dst.cfg->ego_control == HWY_EGO_DIRECT) { p.src_controls = src.controls; p.dst_controls = dst.controls; }
  p.src_time = src.time; p.dst_time = dst.time;
  p.src_episode = src.episode; p.dst_episode = dst.episode;
  p.dst_done = dst.done;
  p.src_env = src_env;
  p.pitch = dst.pitch; p.A = dst.cfg->num_agents; p.branches = branches;
  p.src_envs = src.cfg->num_envs; p.dst_envs = dst.cfg->num_envs;
  return p;
}
// host side: the arguments of the fold of a K-step rollout of a config's environments (score_validate has passed)
inline ScoreParams score_params(const hwy_config &c, int32_t k_steps, int32_t branches, double gamma, const int32_t *first_action,
                                const double *reward, const uint8_t *terminated, const uint8_t *truncated, double *ret, double *q,
                                int32_t *best_action, int32_t *best_branch) {
  ScoreParams p;
  memset(&p, 0, sizeof p);
  p.first_action = first_action; p.reward = reward; p.terminated = terminated; p.truncated = truncated;
  p.ret = ret; p.q = q; p.best_action = best_action; p.best_branch = best_branch;
  p.gamma = gamma;
  p.K = k_steps; p.branches = branches; p.A = c.num_agents; p.n_ids = lookahead_num_ids(c);
  p.groups = c.num_envs / branches;
  return p;
}

// ---- hwy_fork_kernel -------------------------------------------------------------------------------------------------------------------
// (templates, like hwy_ttc_kernel: only the translation unit that launches them holds their code)
template <int THREADS>
__global__ void __launch_bounds__(THREADS) hwy_fork_kernel(const ForkParams p) {
  const int j = (int)blockIdx.x, t = (int)threadIdx.x;
  const int s = p.src_env ? p.src_env[j] : j / p.branches;
  if (s < 0 || s >= p.src_envs) return;  // (workgroup-uniform)
  const int pitch = p.pitch;
  const size_t so = (size_t)s * pitch, dof = (size_t)j * pitch;
  for (int f = 0; f < p.n_f64; ++f) {
    const double *src = p.src_f64[f] + so;
    double *dst = p.dst_f64[f] + dof;
    for (int c = t; c < pitch; c += THREADS) dst[c] = src[c];
  }
  for (int f = 0; f < p.n_i32; ++f) {
    const int32_t *src = p.src_i32[f] + so;
    int32_t *dst = p.dst_i32[f] + dof;
    for (int c = t; c < pitch; c += THREADS) dst[c] = src[c];
  }
  if (p.src_controls && t < 2 * p.A) {  // acceleration | steering of every agent
    const int half = t / p.A, a = t % p.A;
    p.dst_controls[(size_t)half * p.dst_envs * p.A + (size_t)j * p.A + a] = p.src_controls[(size_t)half * p.src_envs * p.A + (size_t)s * p.A + a];
  }
  if (t == 0) {
    p.dst_time[j] = p.src_time[s];
    p.dst_episode[j] = p.src_episode[s];
    p.dst_done[j] = 0;
  }
}

// ---- hwy_score_kernel ------------------------------------------------------------------------------------------------------------------
// order-preserving key: a < b  <=>  score_key(a) < score_key(b) for every pair of non-NaN doubles (-0.0 never occurs: g starts at +0.0
// and a round-to-nearest sum is -0.0 only when both terms are)
__device__ inline unsigned long long score_key(double g) {
  const unsigned long long bits = (unsigned long long)__double_as_longlong(g);
  return (bits >> 63) ? ~bits : (bits | 0x8000000000000000ull);
}
__device__ inline double score_unkey(unsigned long long key) {
  const unsigned long long bits = (key >> 63) ? (key & 0x7fffffffffffffffull) : ~key;
  return __longlong_as_double((long long)bits);
}
#define HWY_SCORE_KEY_NEG_INF 0x000fffffffffffffull  // score_key(-inf)

// the discounted return of branch environment `env`, agent a
__device__ inline double score_return(const ScoreParams &p, size_t env, int a) {
  const size_t envs = (size_t)p.groups * p.branches;
  double g = 0.0, d = 1.0;
  bool alive = true;
  for (int k = 0; k < p.K; ++k) {
    const size_t at = (size_t)k * envs + env;
    if (alive) {
      const double t = d * p.reward[at * p.A + a];
      g = g + t;
    }
    alive = alive && !(p.terminated[at] | p.truncated[at]);
    d = d * p.gamma;
  }
  return g;
}

// IDS: capacity of the per-action slots in LDS
template <int IDS>
__global__ void __launch_bounds__(64) hwy_score_kernel(const ScoreParams p) {
  __shared__ unsigned long long sh_q[IDS];  // per first action: key of the maximal return
  __shared__ unsigned long long sh_top[2];                // key of the maximum over the branches | over the first actions
  __shared__ int32_t sh_arg[2];                           // lowest branch | lowest first action holding it
  const int lane = (int)threadIdx.x, e = (int)blockIdx.x;
  const int B = p.branches, A = p.A, n_ids = p.n_ids;
  const bool by_action = p.first_action != nullptr;       // (A == 1: score_validate)
  for (int a = 0; a < A; ++a) {
    for (int i = lane; i < n_ids; i += 64) sh_q[i] = HWY_SCORE_KEY_NEG_INF;
    if (lane < 2) { sh_top[lane] = 0ull; sh_arg[lane] = 0x7fffffff; }
    __syncthreads();
    // the maxima: over the branches, and per first action
    for (int base = 0; base < B; base += 64) {
      const int b = base + lane;
      if (b >= B) continue;
      const size_t env = (size_t)e * B + b;
      const double g = score_return(p, env, a);
      if (p.ret) p.ret[env * A + a] = g;
      const unsigned long long key = score_key(g);
      __hip_atomic_fetch_max(&sh_top[0], key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (by_action) {
        const int first = p.first_action[env * A];
        if (first >= 0 && first < n_ids) __hip_atomic_fetch_max(&sh_q[first], key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
    }
    __syncthreads();
    // the lowest branch among the holders of the maximum; the maximum over the first actions
    for (int base = 0; base < B; base += 64) {
      const int b = base + lane;
      if (b >= B) continue;
      const unsigned long long key = score_key(score_return(p, (size_t)e * B + b, a));
      if (key == sh_top[0]) __hip_atomic_fetch_min(&sh_arg[0], b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    if (by_action)
      for (int i = lane; i < n_ids; i += 64) __hip_atomic_fetch_max(&sh_top[1], sh_q[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __syncthreads();
    if (by_action)
      for (int i = lane; i < n_ids; i += 64) {
        if (sh_q[i] == sh_top[1]) __hip_atomic_fetch_min(&sh_arg[1], i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (p.q) p.q[(size_t)e * n_ids + i] = score_unkey(sh_q[i]);
      }
    __syncthreads();
    if (lane == 0) {
      if (p.best_branch) p.best_branch[(size_t)e * A + a] = sh_arg[0];
      if (by_action && p.best_action) p.best_action[e] = sh_arg[1];
    }
    __syncthreads();  // (the next agent's pass clears the slots)
  }
}

}  // namespace hwy
