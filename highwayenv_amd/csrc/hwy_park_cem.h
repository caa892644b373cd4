// hwy_park_cem.h -- sampling MPC on the parking scenario: the cross-entropy method of hwy_cem.h (DESIGN.md "CEM on the device"), the
// whole search of every environment in ONE launch (DESIGN.md "CEM on parking: one launch").
//
// A parking environment is one thread's worth of state (hwy_park.h: ParkEnv), so a search needs no work engine: one 64-wide
// WAVEFRONT per environment, every lane a candidate.  hwy_park_cem_kernel<SAMPLE>:
//   * grid = E workgroups of 64 threads.  The parent's ParkEnv is loaded once (every lane issues the same address) and is NEVER
//     written.  Candidate b = pass * 64 + lane, ceil(B / 64) passes per iteration; a lane with b >= B idles through the pass and
//     reaches every barrier and ballot.
//   * SAMPLE: the action pair of step k is drawn inline, by the rule of hwy_cem_sample_kernel and nothing else -- Philox counter
//     {e, b, i * HWY_CEM_MAX_HORIZON + k, "HWCM"}, key = seed, cem_normal2 (cosine: throttle, sine: steering), branch 0 has z = 0,
//     x = (float)min(max(mean + std * z, -1), 1) with the product and the sum in separate statements; mean and std are read from
//     LDS, x goes to the LDS sample table f32 [B][K][2] (dynamic LDS: 8 B K bytes, at most 32 KB).
//     !SAMPLE (score mode): the pair is read from actions f32 [E][B][K][2]; one pass over the candidates, no refit.
//   * the rollout of a lane is park_policy_step -- the advance kernel's branch for an environment that is not re-spawned -- K times,
//     in registers; the handle's autoreset setting is not read, a parent flagged done is stepped as it is.  The return is
//     score_return's recurrence (t = d * r; g = g + t; d = d * gamma, separate statements); the step that terminates or truncates is
//     the last that counts, and the lane stops simulating there -- unless the per-step outputs of score mode are asked for, which
//     record every step as an advance of K steps without autoreset would.
//   * struck bodies: park_strike and park_frame write planes, and a candidate must not write the parent's.  Lane (e, lane) owns a
//     column of a block f64 [4][26][E * 64] of the handle (ParkSlot); at the start of a pass it copies the parent's planes of the
//     parent's struck bits (a rare loop).  The list order is read from the parent.  Not per candidate: a pass's bodies are dead
//     once its return is known.  Not LDS: 53 KB per wavefront would cap a CU at three waves.
//   * rank and refit follow hwy_cem_refit_kernel statement for statement: the keys of the B returns in LDS, rank(b) = #{b': key' >
//     key, or key' == key and b' < b}, elites = rank < M compacted in ascending branch order by ballot + popcount; lane col = k * 2
//     + c (2 K <= 64 columns: one pass) refits its column in f64 over the elites in that order from the LDS sample table, one rounded
//     operation per statement; the best sequence of the search (LDS) is replaced only by a STRICTLY greater top key; the last
//     iteration writes action = best_sequence[0].
// Products and sums are separate statements, so -ffp-contract=on fuses nothing here.
// Like hwy_park.h this header includes no HIP runtime: hwy_kernels_park.hip and hwy_park.hip include <hip/hip_runtime.h> first.
#pragma once

#include "hwy_park.h"
#include "hwy_cem.h"  // cem_uniform2, cem_normal2; hwy_lookahead.h: score_key

namespace hwy {

#define HWY_PARK_CEM_WAVE 64  // threads of a workgroup = candidates of a pass; the columns 2 K of the refit fit one pass

struct ParkCemParams {
  ParkParams park;           // the parent's planes (read only) and the scenario's constants
  double *planes;            // [HWY_PARK_PARKED_F64][26][E * 64]: the struck bodies of lane (e, lane)
  // score mode
  const float *actions;      // [E][B][K][2]
  double *ret;               // [E][B]
  double *step_reward;       // [E][B][K] or null
  uint8_t *step_flags;       // [E][B][K] or null (HWY_PARK_S_*)
  // the search
  const double *init_mean;   // [E][K][2] or null (zeros)
  float *action;             // [E][2]
  double *best_return;       // [E] or null
  double *mean, *stddev;     // [E][K][2] or null
  float *best_sequence;      // [E][K][2] or null
  double *noise;             // [I][E][B][K][2] or null
  float *samples;            // [I][E][B][K][2] or null
  double *returns;           // [I][E][B] or null
  int32_t *elites;           // [I][E][M] or null
  double gamma, init_std, min_std, alpha;
  uint64_t seed;
  int32_t B, K, M, I;
};

// host side: what hwy_park_cem_plan(_device) and hwy_park_score(_device) accept (include/hwy_park.h): parking's own caps
inline int park_cem_validate(const hwy_cem_params *c, const char **why) {
  *why = "";
#define HWY_PARK_CEM_BAD(msg) do { *why = msg; return HWY_PARK_ERR_INVALID_ARG; } while (0)
  if (!c) HWY_PARK_CEM_BAD("cem params is NULL");
  if (c->population < 1 || c->population > HWY_PARK_CEM_MAX_POP) HWY_PARK_CEM_BAD("population must be in [1, HWY_PARK_CEM_MAX_POP = 256]");
  if (c->elites < 1 || c->elites > c->population) HWY_PARK_CEM_BAD("elites must be in [1, population]");
  if (c->horizon < 1 || c->horizon > HWY_PARK_CEM_MAX_HORIZON) HWY_PARK_CEM_BAD("horizon must be in [1, HWY_PARK_CEM_MAX_HORIZON = 32]");
  if (c->population * c->horizon > HWY_PARK_CEM_MAX_SAMPLES)
    HWY_PARK_CEM_BAD("population * horizon must be at most HWY_PARK_CEM_MAX_SAMPLES = 4096 (the sample table of a search: 32 KB of LDS)");
  if (c->iterations < 1 || c->iterations > HWY_PARK_CEM_MAX_ITERATIONS) HWY_PARK_CEM_BAD("iterations must be in [1, HWY_PARK_CEM_MAX_ITERATIONS = 16]");
  if (!(c->gamma > -1e30 && c->gamma < 1e30)) HWY_PARK_CEM_BAD("gamma must be finite");
  if (!(c->init_std >= 0.0 && c->init_std < 1e30)) HWY_PARK_CEM_BAD("init_std must be finite and >= 0");
  if (!(c->min_std >= 0.0 && c->min_std < 1e30)) HWY_PARK_CEM_BAD("min_std must be finite and >= 0");
  if (!(c->alpha >= 0.0 && c->alpha <= 1.0)) HWY_PARK_CEM_BAD("alpha must be in [0, 1]");
#undef HWY_PARK_CEM_BAD
  return HWY_PARK_OK;
}
inline size_t park_cem_plane_bytes(int32_t num_envs) {
  return sizeof(double) * HWY_PARK_PARKED_F64 * HWY_PARK_MAX_PARKED * HWY_PARK_CEM_WAVE * (size_t)num_envs;
}
inline size_t park_cem_lds_bytes(const ParkCemParams &q) { return sizeof(float) * 2 * (size_t)q.B * q.K; }

// x = (float)min(max(mean + std * z, -1), 1), hwy_cem_sample_kernel's statements
__device__ inline float park_cem_draw(double m, double sd, double z) {
  const double d = sd * z;
  const double y = m + d;
  return (float)fmin(fmax(y, -1.0), 1.0);
}

template <bool SAMPLE>
__global__ void __launch_bounds__(HWY_PARK_CEM_WAVE) hwy_park_cem_kernel(const ParkCemParams q) {
  extern __shared__ float sh_x[];                                // the sample table [B][K][2] (SAMPLE)
  __shared__ double sh_mean[HWY_PARK_CEM_WAVE], sh_std[HWY_PARK_CEM_WAVE];  // [K][2]
  __shared__ unsigned long long sh_key[HWY_PARK_CEM_MAX_POP];    // key of every branch's return
  __shared__ int32_t sh_elite[HWY_PARK_CEM_MAX_POP];             // the elites, ascending branch order
  __shared__ float sh_best[HWY_PARK_CEM_WAVE];                   // the best sequence of the search [K][2]
  __shared__ int32_t sh_top;                                     // the branch of rank 0
  const ParkParams &p = q.park;
  const int lane = (int)threadIdx.x, e = (int)blockIdx.x;
  const int B = q.B, K = q.K, M = q.M, cols = 2 * q.K;
  const ParkEnv parent = park_load(p, e);
  const ParkSlot slot{q.planes, (size_t)p.E * HWY_PARK_CEM_WAVE, (size_t)e * HWY_PARK_CEM_WAVE + lane, 0};
  double ctl_sink;  // the stored steering angle the direct-control functions write: ParkEnv::steer carries it, the parent's plane is not touched
  DirectArgs da;
  da.ctl_accel = &ctl_sink;
  da.ctl_steer = &ctl_sink;
  const bool details = !SAMPLE && (q.step_reward || q.step_flags);
  if (SAMPLE) {
    if (lane < cols) {
      sh_mean[lane] = q.init_mean ? q.init_mean[(size_t)e * cols + lane] : 0.0;
      sh_std[lane] = q.init_std;
    }
    __syncthreads();
  }
  unsigned long long best_key = 0;  // (wavefront-uniform) key of the best return of the search
  const int iterations = SAMPLE ? q.I : 1;
  for (int it = 0; it < iterations; ++it) {
    // ---- 1. the candidates: sample and roll out, a pass of 64 at a time ---------------------------------------------------------------
    for (int base = 0; base < B; base += HWY_PARK_CEM_WAVE) {
      const int b = base + lane;
      if (b >= B) continue;  // (no barrier and no ballot inside a pass)
      ParkEnv s = parent;
      for (uint32_t m = parent.struck; m; m &= m - 1) {
        const int i = __ffs((int)m) - 1;
        for (int f = 0; f < HWY_PARK_PARKED_F64; ++f) park_plane(slot, f, i) = p.parked[((size_t)f * HWY_PARK_MAX_PARKED + i) * p.E + e];
      }
      const size_t eb = (size_t)e * B + b;
      double g = 0.0, d = 1.0;
      bool alive = true;
      for (int k = 0; k < K; ++k) {
        float v0, v1;
        if (SAMPLE) {
          double z0 = 0.0, z1 = 0.0;
          if (b > 0) {
            double u0, u1;
            cem_uniform2(q.seed, (uint32_t)e, (uint32_t)b, (uint32_t)(it * HWY_CEM_MAX_HORIZON + k), &u0, &u1);
            cem_normal2(u0, u1, &z0, &z1);
          }
          v0 = park_cem_draw(sh_mean[2 * k], sh_std[2 * k], z0);
          v1 = park_cem_draw(sh_mean[2 * k + 1], sh_std[2 * k + 1], z1);
          sh_x[(b * K + k) * 2] = v0;
          sh_x[(b * K + k) * 2 + 1] = v1;
          const size_t dbg = ((((size_t)it * p.E + e) * B + b) * K + k) * 2;
          if (q.noise) {
            q.noise[dbg] = z0;
            q.noise[dbg + 1] = z1;
          }
          if (q.samples) {
            q.samples[dbg] = v0;
            q.samples[dbg + 1] = v1;
          }
        } else {
          const float *a = q.actions + (eb * K + k) * 2;
          v0 = a[0];
          v1 = a[1];
        }
        if (alive || details) {
          double r;
          const int out = park_policy_step(p, e, slot, s, da, v0, v1, nullptr, &r);
          if (details) {
            if (q.step_reward) q.step_reward[eb * K + k] = r;
            if (q.step_flags) q.step_flags[eb * K + k] = (uint8_t)out;
          }
          if (alive) {
            const double t = d * r;
            g = g + t;
            alive = !(out & (HWY_PARK_S_TERMINATED | HWY_PARK_S_TRUNCATED));
          }
        }
        d = d * q.gamma;
      }
      if (SAMPLE) {
        sh_key[b] = score_key(g);
        if (q.returns) q.returns[((size_t)it * p.E + e) * B + b] = g;
      } else {
        q.ret[eb] = g;
      }
    }
    if (!SAMPLE) break;
    __syncthreads();

    // ---- 2. ranks; the elites compacted in ascending branch order ---------------------------------------------------------------------
    int placed = 0;  // (wavefront-uniform) elites of the earlier passes
    for (int base = 0; base < B; base += HWY_PARK_CEM_WAVE) {
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

    // ---- 3. the best sequence of the search: replaced when this iteration's top is STRICTLY better ----------------------------------
    if (q.elites)
      for (int j = lane; j < M; j += HWY_PARK_CEM_WAVE) q.elites[((size_t)it * p.E + e) * M + j] = sh_elite[j];
    const int top = sh_top;
    const unsigned long long top_key = sh_key[top];
    const bool improved = it == 0 || top_key > best_key;
    if (improved) best_key = top_key;

    // ---- 4. the refit, a (k, c) column per lane ---------------------------------------------------------------------------------------
    if (lane < cols) {
      const int col = lane;
      const double count = (double)M;
      double sum = 0.0;
      for (int j = 0; j < M; ++j) {
        const double x = (double)sh_x[sh_elite[j] * cols + col];
        sum = sum + x;
      }
      const double m = sum / count;
      double acc = 0.0;
      for (int j = 0; j < M; ++j) {
        const double x = (double)sh_x[sh_elite[j] * cols + col];
        const double dx = x - m;
        const double sq = dx * dx;
        acc = acc + sq;
      }
      const double v = acc / count;
      const double sd = sqrt(v);
      const double mean_old = sh_mean[col], std_old = sh_std[col];
      const double keep = 1.0 - q.alpha;
      const double m_new = q.alpha * m;
      const double m_old = keep * mean_old;
      sh_mean[col] = m_new + m_old;
      const double s_new = q.alpha * sd;
      const double s_old = keep * std_old;
      const double s_mix = s_new + s_old;
      sh_std[col] = fmax(q.min_std, s_mix);
      if (improved) sh_best[col] = sh_x[top * cols + col];
    }
    __syncthreads();  // mean, std and the sample table are the next iteration's
  }
  if (!SAMPLE) return;
  if (lane < cols) {
    const size_t at = (size_t)e * cols + lane;
    if (q.mean) q.mean[at] = sh_mean[lane];
    if (q.stddev) q.stddev[at] = sh_std[lane];
    if (q.best_sequence) q.best_sequence[at] = sh_best[lane];
    if (lane < 2) q.action[(size_t)e * 2 + lane] = sh_best[lane];
  }
  if (lane == 0 && q.best_return) q.best_return[e] = score_unkey(best_key);
}

}  // namespace hwy
