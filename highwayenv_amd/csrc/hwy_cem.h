// hwy_cem.h -- sampling MPC for the continuous egos of a direct-control engine: the cross-entropy method (CEM) on the device, one
// search per environment, restated exactly in DESIGN.md ("CEM on the device").  Like OPD (hwy_opd.h) this is a restatement of the
// algorithm, not parity with any package; the simulation is the engine's own (fork -> K x (act, step) -> score).
//
//   hwy_cem_sample_kernel   one THREAD per (environment e, branch b, step k).  One Philox-4x32-10 block, counter
//                           {e, b, iteration * HWY_CEM_MAX_HORIZON + k, "HWCM"}, key = seed, gives two uniforms (the 53-bit rule of
//                           philox_uniform2); Box-Muller in f64 on hwy_math.h's log_pos (argument 1 - u0 in [2^-53, 1]: positive
//                           normal) and sincos_bounded (angle 2 pi u1 reduced to [-pi, pi)) gives two normals: the cosine one is the
//                           throttle's, the sine one the steering's; with one controlled axis the cosine one alone.  Branch 0 has
//                           z = 0: it IS the current mean.  x = (float)min(max(mean + std * z, -1), 1) goes to [k][e * B + b][size]
//                           of the work engine's action block, the layout hwy_rollout_continuous_device reads.
//   hwy_cem_refit_kernel    one 64-wide WAVEFRONT per environment, behind the score kernel that wrote ret [E][B].  The keys of the
//                           returns (score_key) go to LDS; rank(b) = #{b': key' > key, or key' == key and b' < b} is a strict total
//                           order, the elites are rank < M, compacted into ascending branch order with ballot + popcount (no atomic
//                           whose order could matter).  Lanes own the (k, c) columns in passes of 64 and refit in f64 over the
//                           elites in ascending branch order, one rounded operation per statement:
//                             m = (sum x) / M;  v = (sum (x - m)^2) / M;  s = sqrt(v)
//                             mean' = alpha * m + (1 - alpha) * mean;  std' = max(min_std, alpha * s + (1 - alpha) * std)
//                           (IEEE divide and sqrt: a NumPy restatement is bit-exact, tests/cem_util.py).  The best sequence of the
//                           search is replaced only when the iteration's top key is STRICTLY greater (the earliest iteration wins;
//                           within an iteration rank 0 is the lowest branch among the holders of the maximum).  The last iteration
//                           writes the action: step 0 of the best sequence.  An optional output records every iteration's
//                           elite branches [I][E][M], ascending.
//
// Products and sums are separate statements everywhere, so -ffp-contract=on fuses nothing.
// Like hwy_act.h this header includes no HIP runtime: hwy_kernels_cem.hip includes <hip/hip_runtime.h> first, the CPU emulation
// (tests/emu/emu_cem.cpp) its shim, hip_emu.h.  The launch rules are hwy_launch_units.h's (select_cem_sample, select_cem_refit) and
// the sequence of launches of a plan is cem_iterate's below, for both.
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/hwy_engine.h"
#include "hwy_act.h"
#include "hwy_device.h"     // philox4x32_10, hwy_math.h
#include "hwy_lookahead.h"  // score_key, fork_validate

namespace hwy {

#define HWY_CEM_BLOCK 256                   // threads of a workgroup of the sample kernel
#define HWY_CEM_STREAM_TAG 0x4857434Du      // "HWCM": counter word 3 of every draw (the spawn's is "HWY1": no stream is shared)
#define HWY_CEM_REFIT_LDS_CAP (HWY_CEM_MAX_POP * 12 + 64)  // keys (8 B) + compacted elites (4 B) per branch, + the top branch

struct CemParams {
  float *actions;            // [K][E * B][size]: the work engine's action block
  const double *init_mean;   // [E][K][size] or null (zeros): the mean before the first refit
  double *mean, *stddev;     // [E][K][size]: written by every refit, read by the next iteration
  double *noise;             // [I][E][B][K][size] or null
  float *samples;            // [I][E][B][K][size] or null
  int32_t *elites;           // [I][E][M] or null: every iteration's elite branches, ascending
  const double *ret;         // [E][B]: the score kernel's returns of this iteration
  double *best_return;       // [E]
  float *best_sequence;      // [E][K][size]
  float *action;             // [E][size]
  double init_std, min_std, alpha;
  uint64_t seed;
  int32_t E, B, K, size, M, I, iter, pad_;
};

// host side: what hwy_cem_plan_device accepts (include/hwy_engine.h).  Shared by hwy_engine.hip and the CPU emulation.
inline int cem_validate(const hwy_config &src, const hwy_config &work, const hwy_continuous_params *cp, const hwy_cem_params *params,
                        bool has_action, const char **why) {
  *why = "";
  if (src.scenario != HWY_SCENARIO_HIGHWAY) {
    *why = "CEM plans on the highway scenario only (the merge and intersection scenarios are outside the hot-path scope)";
    return HWY_ERR_UNSUPPORTED;
  }
  if (src.ego_control != HWY_EGO_DIRECT) {
    *why = "CEM plans continuous controls: it needs a direct-control ego (ego_control is HWY_EGO_META)";
    return HWY_ERR_UNSUPPORTED;
  }
  if (src.num_agents != 1) {
    *why = "CEM plans for a single agent (joint searches are outside the hot-path scope; hwy_score_rollout_continuous serves several)";
    return HWY_ERR_UNSUPPORTED;
  }
  if (const int rc = act_validate(src, cp, why)) return rc;
  if (!params) { *why = "cem params is NULL"; return HWY_ERR_INVALID_ARG; }
  if (!has_action) { *why = "action must be non-NULL"; return HWY_ERR_INVALID_ARG; }
  if (params->population < 1 || params->population > HWY_CEM_MAX_POP) { *why = "population must be in [1, HWY_CEM_MAX_POP]"; return HWY_ERR_INVALID_ARG; }
  if (params->elites < 1 || params->elites > params->population) { *why = "elites must be in [1, population]"; return HWY_ERR_INVALID_ARG; }
  if (params->iterations < 1 || params->iterations > HWY_CEM_MAX_ITERATIONS) { *why = "iterations must be in [1, HWY_CEM_MAX_ITERATIONS]"; return HWY_ERR_INVALID_ARG; }
  if (params->horizon < 1 || params->horizon > HWY_CEM_MAX_HORIZON) { *why = "horizon must be in [1, HWY_CEM_MAX_HORIZON]"; return HWY_ERR_INVALID_ARG; }
  if (!(params->gamma > -1e30 && params->gamma < 1e30)) { *why = "gamma must be finite"; return HWY_ERR_INVALID_ARG; }
  if (!(params->init_std >= 0.0 && params->init_std < 1e30)) { *why = "init_std must be finite and >= 0"; return HWY_ERR_INVALID_ARG; }
  if (!(params->min_std >= 0.0 && params->min_std < 1e30)) { *why = "min_std must be finite and >= 0"; return HWY_ERR_INVALID_ARG; }
  if (!(params->alpha >= 0.0 && params->alpha <= 1.0)) { *why = "alpha must be in [0, 1]"; return HWY_ERR_INVALID_ARG; }
  if ((int64_t)work.num_envs != (int64_t)src.num_envs * params->population) {
    *why = "work.num_envs must be src.num_envs * population";
    return HWY_ERR_INVALID_ARG;
  }
  return fork_validate(work, src, false, params->population, false, why);  // (the two configs agree)
}

// host side: true when every one of the n doubles is finite (the host-pointer entry point: HWY_ERR_ACTION otherwise)
inline bool cem_all_finite(const double *a, size_t n) {
  for (size_t k = 0; k < n; ++k)
    if (!isfinite(a[k])) return false;
  return true;
}

// host side: the planner's own arrays (the layout of CemParams' fields of the same names) ...
struct CemArrays {
  float *actions;
  const double *init_mean;
  double *mean, *stddev;
  double *noise;
  float *samples;
  double *best_return;
  float *best_sequence;
  float *action;
  int32_t *elites;
};
// ... and the arguments of the two kernels over them and the score kernel's returns (cem_validate has passed); p.iter is the launch's own
inline CemParams cem_params(const hwy_cem_params &params, const hwy_continuous_params &cp, int32_t num_envs, const CemArrays &a,
                            const double *ret) {
  CemParams p;
  memset(&p, 0, sizeof p);
  p.actions = a.actions; p.init_mean = a.init_mean; p.mean = a.mean; p.stddev = a.stddev; p.noise = a.noise; p.samples = a.samples; p.elites = a.elites;
  p.ret = ret; p.best_return = a.best_return; p.best_sequence = a.best_sequence; p.action = a.action;
  p.init_std = params.init_std; p.min_std = params.min_std; p.alpha = params.alpha; p.seed = params.seed;
  p.E = num_envs; p.B = params.population; p.K = params.horizon; p.size = act_size(cp); p.M = params.elites; p.I = params.iterations;
  return p;
}

// host side: THE sequence of a plan -- per iteration the sample kernel, the parent's state into all B work environments of e, the K
// (act, step) pairs of the work engine on the block the sample kernel wrote, the fold of their outputs into ret, the refit.  Generic
// over what enqueues (hwy_engine.hip: hwy_cem_plan_device, on work's stream) or runs (tests/emu/emu_cem.cpp) the operations, each
// returning 0 or the status the plan ends with:
//   ops.sample(const CemParams &)   hwy_cem_sample_kernel
//   ops.fork(branches)              hwy_fork_device(work, src, branches, NULL)
//   ops.rollout(k_steps)            hwy_rollout_continuous_device(work, k_steps) on p.actions
//   ops.score(k_steps, branches)    hwy_score_device(work, ..., first_action NULL, ..., ret)
//   ops.refit(const CemParams &)    hwy_cem_refit_kernel
template <typename Ops>
int cem_iterate(CemParams p, Ops &&ops) {
  for (int32_t i = 0; i < p.I; ++i) {
    p.iter = i;
    if (int rc = ops.sample(p)) return rc;
    if (int rc = ops.fork(p.B)) return rc;
    if (int rc = ops.rollout(p.K)) return rc;
    if (int rc = ops.score(p.K, p.B)) return rc;
    if (int rc = ops.refit(p)) return rc;
  }
  return HWY_OK;
}

// two uniforms in [0, 1) with 53 random bits each (philox_uniform2's rule) from the block of (environment, branch, draw)
__host__ __device__ inline void cem_uniform2(uint64_t seed, uint32_t env, uint32_t branch, uint32_t draw, double *u0, double *u1) {
  uint32_t c[4] = {env, branch, draw, HWY_CEM_STREAM_TAG};
  philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  const uint64_t a = ((uint64_t)c[0] << 32) | c[1], b = ((uint64_t)c[2] << 32) | c[3];
  *u0 = (double)(a >> 11) * (1.0 / 9007199254740992.0);
  *u1 = (double)(b >> 11) * (1.0 / 9007199254740992.0);
}

// Box-Muller: two independent standard normals from two uniforms of [0, 1).  |z| <= sqrt(2 * 53 ln 2) < 8.6.
__device__ inline void cem_normal2(double u0, double u1, double *z_cos, double *z_sin) {
  const double w = 1.0 - u0;                  // in [2^-53, 1]: a positive normal double (log_pos's domain)
  const double l = log_pos(w);
  const double q = -2.0 * l;                  // >= 0
  const double r = sqrt(q);
  double a = 6.283185307179586 * u1;          // [0, 2 pi)
  if (a >= 3.141592653589793) a = a - 6.283185307179586;  // [-pi, pi): sincos_bounded's domain with room to spare
  double sn, cs;
  sincos_bounded(a, &sn, &cs);
  *z_cos = r * cs;
  *z_sin = r * sn;
}

// the mean / std a launch of iteration p.iter starts from
__device__ inline double cem_mean_in(const CemParams &p, size_t col) {
  return p.iter == 0 ? (p.init_mean ? p.init_mean[col] : 0.0) : p.mean[col];
}
__device__ inline double cem_std_in(const CemParams &p, size_t col) { return p.iter == 0 ? p.init_std : p.stddev[col]; }

// BLOCK: threads per workgroup (a template so that the header can be included by several translation units)
template <int BLOCK>
__global__ void __launch_bounds__(BLOCK) hwy_cem_sample_kernel(const CemParams p) {
  const long long t = (long long)blockIdx.x * BLOCK + (long long)threadIdx.x;  // k * (E * B) + e * B + b
  const long long EB = (long long)p.E * p.B;
  if (t >= EB * p.K) return;
  const int k = (int)(t / EB);
  const long long eb = t % EB;
  const int e = (int)(eb / p.B), b = (int)(eb % p.B);
  double z[2] = {0.0, 0.0};
  if (b > 0) {
    double u0, u1;
    cem_uniform2(p.seed, (uint32_t)e, (uint32_t)b, (uint32_t)(p.iter * HWY_CEM_MAX_HORIZON + k), &u0, &u1);
    cem_normal2(u0, u1, &z[0], &z[1]);
  }
  const size_t dbg = ((((size_t)p.iter * p.E + e) * p.B + b) * p.K + k) * p.size;
  for (int c = 0; c < p.size; ++c) {
    const size_t col = ((size_t)e * p.K + k) * p.size + c;
    const double m = cem_mean_in(p, col), sd = cem_std_in(p, col);
    const double d = sd * z[c];
    const double y = m + d;
    const float x = (float)fmin(fmax(y, -1.0), 1.0);
    p.actions[((size_t)k * EB + eb) * p.size + c] = x;
    if (p.noise) p.noise[dbg + c] = z[c];
    if (p.samples) p.samples[dbg + c] = x;
  }
}

// POP: capacity of the per-branch slots in LDS
template <int POP>
__global__ void __launch_bounds__(64) hwy_cem_refit_kernel(const CemParams p) {
  __shared__ unsigned long long sh_key[POP];  // key of every branch's return
  __shared__ int32_t sh_elite[POP];           // the elites, ascending branch order
  __shared__ int32_t sh_top;                  // the branch of rank 0
  const int lane = (int)threadIdx.x, e = (int)blockIdx.x;
  const int B = p.B, M = p.M, K = p.K, size = p.size;
  const size_t EB = (size_t)p.E * B, row = (size_t)e * B;
  for (int b = lane; b < B; b += 64) sh_key[b] = score_key(p.ret[row + b]);
  const double best_before = p.iter == 0 ? 0.0 : p.best_return[e];  // (read by every lane before lane 0 rewrites it)
  __syncthreads();

  // ---- 1. ranks; the elites compacted in ascending branch order ------------------------------------------------------------------
  int placed = 0;  // (wavefront-uniform) elites of the earlier passes
  for (int base = 0; base < B; base += 64) {
    const int b = base + lane;
    int rank = 0x7fffffff;
    if (b < B) {
      const unsigned long long mine = sh_key[b];
      rank = 0;
      for (int o = 0; o < B; ++o) {
        const unsigned long long other = sh_key[o];
        rank += (other > mine || (other == mine && o < b)) ? 1 : 0;
      }
    }
    const bool elite = rank < M;
    const unsigned long long votes = __ballot(elite ? 1 : 0);
    if (elite) sh_elite[placed + __popcll(votes & ((1ull << lane) - 1ull))] = b;
    if (rank == 0) sh_top = b;  // (one lane of one pass: the ranks are a strict total order)
    placed += __popcll(votes);
  }
  __syncthreads();

  // ---- 2. the best sequence of the search: replaced when this iteration's top is STRICTLY better ---------------------------------------
  if (p.elites)
    for (int j = lane; j < M; j += 64) p.elites[((size_t)p.iter * p.E + e) * M + j] = sh_elite[j];
  const int top = sh_top;
  const unsigned long long top_key = sh_key[top];
  const bool improved = p.iter == 0 || top_key > score_key(best_before);
  const bool last = p.iter == p.I - 1;
  if (lane == 0 && improved) p.best_return[e] = score_unkey(top_key);

  // ---- 3. the refit, a (k, c) column per lane ------------------------------------------------------------------------------------------
  const double count = (double)M;
  for (int col = lane; col < K * size; col += 64) {
    const int k = col / size, c = col % size;
    const float *plane = p.actions + ((size_t)k * EB + row) * size + c;  // + b * size: branch b
    double sum = 0.0;
    for (int j = 0; j < M; ++j) {
      const double x = (double)plane[(size_t)sh_elite[j] * size];
      sum = sum + x;
    }
    const double m = sum / count;
    double acc = 0.0;
    for (int j = 0; j < M; ++j) {
      const double x = (double)plane[(size_t)sh_elite[j] * size];
      const double d = x - m;
      const double q = d * d;
      acc = acc + q;
    }
    const double v = acc / count;
    const double s = sqrt(v);
    const size_t at = (size_t)e * K * size + col;
    const double mean_old = cem_mean_in(p, at), std_old = cem_std_in(p, at);
    const double keep = 1.0 - p.alpha;
    const double m_new = p.alpha * m;
    const double m_old = keep * mean_old;
    p.mean[at] = m_new + m_old;
    const double s_new = p.alpha * s;
    const double s_old = keep * std_old;
    const double s_mix = s_new + s_old;
    p.stddev[at] = fmax(p.min_std, s_mix);
    const float x_top = plane[(size_t)top * size];
    if (improved) p.best_sequence[at] = x_top;
    if (last && k == 0) p.action[(size_t)e * size + c] = improved ? x_top : p.best_sequence[at];
  }
}

}  // namespace hwy
