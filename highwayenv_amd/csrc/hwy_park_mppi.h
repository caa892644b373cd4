// hwy_park_mppi.h -- sampling MPC on the parking scenario by MPPI (model-predictive path integral control, Williams et al. 2017), the
// whole search of every environment in ONE launch (DESIGN.md "MPPI on parking").  A second planner next to hwy_park_cem.h: the same
// simulator in registers (park_policy_step), the same white noise and the same struck-body block, another search.  Every candidate
// is kept: the mean moves to the softmax-weighted average of all B samples, so there is no ranking and no elite set.
//
// hwy_park_mppi_kernel<DEBUG> (true: the launch was given a debug buffer), grid = E workgroups of one 64-wide wavefront:
//   * candidate b = pass * 64 + lane, ceil(B / 64) passes per iteration; a lane with b >= B skips the pass's body and reaches every
//     barrier and every shuffle with the identity (key 0, weight 0).  The parent's ParkEnv is loaded once and NEVER written.
//   * noise: the white z[k] is hwy_park_cem_kernel's -- Philox counter {e, b, i * HWY_CEM_MAX_HORIZON + k, "HWCM"}, key = seed,
//     cem_normal2 (cosine: throttle, sine: steering), candidate 0 has z = 0.  It is coloured per axis by an AR(1) filter carried in two
//     registers: n[0] = z[0]; t1 = beta * n[k-1]; t2 = beta_c * z[k]; n[k] = t1 + t2, with beta_c = sqrt(1 - beta^2) computed on the host.
//   * sample: x = park_cem_draw(u[k][c], noise_std, n[k][c]) into the LDS sample table f32 [B][K][2] (dynamic LDS: 8 B K bytes).
//   * rollout and return: hwy_park_cem_kernel's SAMPLE mode statement for statement (t = d * r; g = g + t; d = d * gamma; the step
//     that ends the episode is the last that counts); struck bodies go to the lane's ParkSlot column of the handle's block.
//   * weights: the return goes to sh_w[b] and its score_key into a per-lane running maximum; one xor-shuffle reduction of the keys
//     after the passes gives g_max.  The lane that rolled candidate b out then replaces sh_w[b] by w = exp_bounded((g - g_max) /
//     temperature) -- each weight is computed once -- and adds w and w * w to lane sums that two shuffle reductions finish (eta, and
//     the effective sample size eta^2 / sum w^2).
//   * update: the 2 K <= 64 columns are padded to a power of two P and the wavefront splits into 64 / P lane groups; group j sums
//     w_b * x_b[col] over b = j, j + 64 / P, ... from LDS, an xor-shuffle over the group bits combines them, and group 0 writes
//     u[col] = alpha * (sum / eta) + (1 - alpha) * u[col].  At the default K = 8 that is 4 groups of 16 candidates, not 64 serial terms.
// Products, sums and quotients are separate statements, so -ffp-contract=on fuses nothing here.
// Like hwy_park.h this header includes no HIP runtime: hwy_kernels_park.hip and hwy_park.hip include <hip/hip_runtime.h> first.
#pragma once

#include "hwy_park_cem.h"  // park_cem_draw, park_cem_plane_bytes, HWY_PARK_CEM_WAVE; hwy_cem.h: cem_uniform2, cem_normal2; score_key

namespace hwy {

struct ParkMppiParams {
  ParkParams park;           // the parent's planes (read only) and the scenario's constants
  double *planes;            // [HWY_PARK_PARKED_F64][26][E * 64]: the struck bodies of lane (e, lane)
  const double *init_mean;   // [E][K][2] or null (zeros)
  float *action;             // [E][2]
  double *best_return;       // [E] or null
  double *mean;              // [E][K][2] or null
  double *weights_ess;       // [E] or null
  double *noise;             // [I][E][B][K][2] or null: the coloured n
  float *samples;            // [I][E][B][K][2] or null
  double *returns, *weights; // [I][E][B] or null
  double *mean_history;      // [I + 1][E][K][2] or null
  double gamma, noise_std, temperature, beta, beta_c, alpha;
  uint64_t seed;
  int32_t B, K, I;
};

// host side: what hwy_park_mppi_plan(_device) accept (include/hwy_park.h); the caps are the CEM search's
inline int park_mppi_validate(const hwy_park_mppi_params *c, const char **why) {
  *why = "";
#define HWY_PARK_MPPI_BAD(msg) do { *why = msg; return HWY_PARK_ERR_INVALID_ARG; } while (0)
  if (!c) HWY_PARK_MPPI_BAD("mppi params is NULL");
  if (c->struct_size != (int32_t)sizeof(hwy_park_mppi_params)) HWY_PARK_MPPI_BAD("struct_size is not sizeof(hwy_park_mppi_params)");
  if (c->population < 1 || c->population > HWY_PARK_CEM_MAX_POP) HWY_PARK_MPPI_BAD("population must be in [1, HWY_PARK_CEM_MAX_POP = 256]");
  if (c->horizon < 1 || c->horizon > HWY_PARK_CEM_MAX_HORIZON) HWY_PARK_MPPI_BAD("horizon must be in [1, HWY_PARK_CEM_MAX_HORIZON = 32]");
  if (c->population * c->horizon > HWY_PARK_CEM_MAX_SAMPLES)
    HWY_PARK_MPPI_BAD("population * horizon must be at most HWY_PARK_CEM_MAX_SAMPLES = 4096 (the sample table of a search: 32 KB of LDS)");
  if (c->iterations < 1 || c->iterations > HWY_PARK_CEM_MAX_ITERATIONS) HWY_PARK_MPPI_BAD("iterations must be in [1, HWY_PARK_CEM_MAX_ITERATIONS = 16]");
  if (!(c->gamma > -1e30 && c->gamma < 1e30)) HWY_PARK_MPPI_BAD("gamma must be finite");
  if (!(c->noise_std >= 0.0 && c->noise_std < 1e30)) HWY_PARK_MPPI_BAD("noise_std must be finite and >= 0");
  if (!(c->temperature > 0.0 && c->temperature < 1e30)) HWY_PARK_MPPI_BAD("temperature must be finite and > 0");
  if (!(c->beta >= 0.0 && c->beta < 1.0)) HWY_PARK_MPPI_BAD("beta must be in [0, 1)");
  const double unit = c->beta * c->beta + c->beta_c * c->beta_c;
  if (!(c->beta_c > 0.0 && unit > 1.0 - 1e-9 && unit < 1.0 + 1e-9)) HWY_PARK_MPPI_BAD("beta_c must be sqrt(1 - beta * beta)");
  if (!(c->alpha >= 0.0 && c->alpha <= 1.0)) HWY_PARK_MPPI_BAD("alpha must be in [0, 1]");
#undef HWY_PARK_MPPI_BAD
  return HWY_PARK_OK;
}
inline size_t park_mppi_lds_bytes(const ParkMppiParams &q) { return sizeof(float) * 2 * (size_t)q.B * q.K; }

// xor-shuffle reductions over the wavefront: the lanes whose indices differ in the bits >= `from` are combined, every lane gets the result
__device__ inline unsigned long long mppi_wave_max(unsigned long long v) {
  for (int off = HWY_PARK_CEM_WAVE / 2; off; off >>= 1) {
    const unsigned long long o = __shfl_xor(v, off, HWY_PARK_CEM_WAVE);
    v = o > v ? o : v;
  }
  return v;
}
__device__ inline double mppi_wave_sum(double v, int from) {
  for (int off = HWY_PARK_CEM_WAVE / 2; off >= from; off >>= 1) {
    const double o = __shfl_xor(v, off, HWY_PARK_CEM_WAVE);
    v = v + o;
  }
  return v;
}

template <bool DEBUG>  // DEBUG: the debug buffers may be given; false compiles their stores out of the hot path
__global__ void __launch_bounds__(HWY_PARK_CEM_WAVE) hwy_park_mppi_kernel(const ParkMppiParams q) {
  extern __shared__ float sh_x[];                  // the sample table [B][K][2]
  __shared__ double sh_u[HWY_PARK_CEM_WAVE];       // the mean [K][2]
  __shared__ double sh_w[HWY_PARK_CEM_MAX_POP];    // the return of every candidate, then its weight
  const ParkParams &p = q.park;
  const int lane = (int)threadIdx.x, e = (int)blockIdx.x;
  const int B = q.B, K = q.K, cols = 2 * q.K;
  const ParkEnv parent = park_load(p, e);
  const ParkSlot slot{q.planes, (size_t)p.E * HWY_PARK_CEM_WAVE, (size_t)e * HWY_PARK_CEM_WAVE + lane, 0};
  double ctl_sink;  // the stored steering angle the direct-control functions write: ParkEnv::steer carries it, the parent's plane is not touched
  DirectArgs da;
  da.ctl_accel = &ctl_sink;
  da.ctl_steer = &ctl_sink;
  // the update's split: column `col` of lane group `grp`, `groups` candidates side by side
  int padded = 2;
  while (padded < cols) padded <<= 1;
  const int groups = HWY_PARK_CEM_WAVE / padded, col = lane & (padded - 1), grp = lane / padded;
  const size_t hist = (size_t)p.E * cols;  // one mean of every environment
  if (lane < cols) {
    const double u0 = q.init_mean ? q.init_mean[(size_t)e * cols + lane] : 0.0;
    sh_u[lane] = u0;
    if (DEBUG && q.mean_history) q.mean_history[(size_t)e * cols + lane] = u0;
  }
  __syncthreads();
  unsigned long long best_key = 0;  // (wavefront-uniform) key of the best return of the search; 0 is below every key
  double eta = 1.0, sq = 1.0;       // (wavefront-uniform) the last iteration's sum of the weights and of their squares
  for (int it = 0; it < q.I; ++it) {
    // ---- 1. the candidates: colour, sample and roll out, a pass of 64 at a time -------------------------------------------------------
    unsigned long long top_key = 0;  // this lane's candidates
    for (int base = 0; base < B; base += HWY_PARK_CEM_WAVE) {
      const int b = base + lane;
      if (b >= B) continue;  // (no barrier and no shuffle inside a pass)
      ParkEnv s = parent;
      for (uint32_t m = parent.struck; m; m &= m - 1) {
        const int i = __ffs((int)m) - 1;
        for (int f = 0; f < HWY_PARK_PARKED_F64; ++f) park_plane(slot, f, i) = p.parked[((size_t)f * HWY_PARK_MAX_PARKED + i) * p.E + e];
      }
      double g = 0.0, d = 1.0, n0 = 0.0, n1 = 0.0;
      bool alive = true;
      for (int k = 0; k < K; ++k) {
        double z0 = 0.0, z1 = 0.0;
        if (b > 0) {
          double u0, u1;
          cem_uniform2(q.seed, (uint32_t)e, (uint32_t)b, (uint32_t)(it * HWY_CEM_MAX_HORIZON + k), &u0, &u1);
          cem_normal2(u0, u1, &z0, &z1);
        }
        if (k == 0) {
          n0 = z0;
          n1 = z1;
        } else {
          const double t10 = q.beta * n0;
          const double t20 = q.beta_c * z0;
          n0 = t10 + t20;
          const double t11 = q.beta * n1;
          const double t21 = q.beta_c * z1;
          n1 = t11 + t21;
        }
        const float v0 = park_cem_draw(sh_u[2 * k], q.noise_std, n0);
        const float v1 = park_cem_draw(sh_u[2 * k + 1], q.noise_std, n1);
        sh_x[(b * K + k) * 2] = v0;
        sh_x[(b * K + k) * 2 + 1] = v1;
        const size_t dbg = ((((size_t)it * p.E + e) * B + b) * K + k) * 2;
        if (DEBUG && q.noise) {
          q.noise[dbg] = n0;
          q.noise[dbg + 1] = n1;
        }
        if (DEBUG && q.samples) {
          q.samples[dbg] = v0;
          q.samples[dbg + 1] = v1;
        }
        if (alive) {
          double r;
          const int out = park_policy_step(p, e, slot, s, da, v0, v1, nullptr, &r);
          const double t = d * r;
          g = g + t;
          alive = !(out & (HWY_PARK_S_TERMINATED | HWY_PARK_S_TRUNCATED));
        }
        d = d * q.gamma;
      }
      sh_w[b] = g;
      const unsigned long long key = score_key(g);
      top_key = key > top_key ? key : top_key;
      if (DEBUG && q.returns) q.returns[((size_t)it * p.E + e) * B + b] = g;
    }

    // ---- 2. the weights, each by the lane that holds its return ------------------------------------------------------------------------
    top_key = mppi_wave_max(top_key);
    best_key = top_key > best_key ? top_key : best_key;
    const double g_max = score_unkey(top_key);
    double w_sum = 0.0, w_sq = 0.0;
    for (int base = 0; base < B; base += HWY_PARK_CEM_WAVE) {
      const int b = base + lane;
      if (b >= B) continue;
      const double below = sh_w[b] - g_max;
      const double a = below / q.temperature;
      const double w = exp_bounded(a);
      sh_w[b] = w;
      const double ww = w * w;
      w_sum = w_sum + w;
      w_sq = w_sq + ww;
      if (DEBUG && q.weights) q.weights[((size_t)it * p.E + e) * B + b] = w;
    }
    eta = mppi_wave_sum(w_sum, 1);  // >= 1: the best candidate's weight is exp(0)
    sq = mppi_wave_sum(w_sq, 1);
    __syncthreads();  // the weights and the sample table are every lane's now

    // ---- 3. the update: lane group grp sums candidates grp, grp + groups, ... of column col ---------------------------------------------
    double acc = 0.0;
    if (col < cols)
      for (int b = grp; b < B; b += groups) {
        const double x = (double)sh_x[b * cols + col];
        const double wx = sh_w[b] * x;
        acc = acc + wx;
      }
    acc = mppi_wave_sum(acc, padded);
    if (lane < cols) {  // group 0: col == lane
      const double m = acc / eta;
      const double keep = 1.0 - q.alpha;
      const double m_new = q.alpha * m;
      const double m_old = keep * sh_u[lane];
      const double u = m_new + m_old;
      sh_u[lane] = u;
      if (DEBUG && q.mean_history) q.mean_history[(size_t)(it + 1) * hist + (size_t)e * cols + lane] = u;
    }
    __syncthreads();  // the mean is the next iteration's; its samples and weights overwrite this one's
  }
  if (lane < cols) {
    const double u = sh_u[lane];
    if (q.mean) q.mean[(size_t)e * cols + lane] = u;
    if (lane < 2) q.action[(size_t)e * 2 + lane] = (float)fmin(fmax(u, -1.0), 1.0);
  }
  if (lane == 0) {
    if (q.best_return) q.best_return[e] = score_unkey(best_key);
    if (q.weights_ess) {
      const double eta2 = eta * eta;
      q.weights_ess[e] = eta2 / sq;
    }
  }
}

}  // namespace hwy
