// hwy_park.hip -- C-ABI host side of the parking scenario (include/hwy_park.h): an opaque handle that owns the planes of E
// environments and one HIP stream.  The device-pointer entry points enqueue on that stream and return; the host-pointer forms
// stage through device buffers of the handle and synchronise.  No CPU implementation: without a GPU hwy_park_create fails.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "hwy_park.h"
#include "hwy_park_cem.h"
#include "hwy_park_mppi.h"

namespace hwy {
hipError_t launch_park_cem(const ParkCemParams &q, bool sample, hipStream_t stream);
hipError_t launch_park_mppi(const ParkMppiParams &q, hipStream_t stream);
hipError_t launch_park_advance(const ParkParams &p, hipStream_t stream);
hipError_t launch_park_reset(const ParkParams &p, bool reset, hipStream_t stream);
hipError_t launch_park_goal_reward(const ParkGoalParams &g, hipStream_t stream);
}  // namespace hwy

struct hwy_park {
  hwy_park_config cfg{};
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  double *d_ego = nullptr, *d_parked = nullptr;
  int32_t *d_ints = nullptr;
  uint8_t *d_order = nullptr;
  // outputs and inputs of the host-pointer forms
  float *d_obs = nullptr;
  double *d_reward = nullptr;
  uint8_t *d_flags = nullptr, *d_mask = nullptr;
  uint64_t *d_seeds = nullptr;
  char *d_roll = nullptr;  // actions | step_reward | step_flags of k steps, grown on demand
  size_t roll_bytes = 0;
  double *d_goal = nullptr;  // achieved | desired | out of m rows, grown on demand
  size_t goal_rows = 0;
  double *d_plan = nullptr;  // the candidates' struck bodies of hwy_park_cem_plan / hwy_park_score, allocated by the first call
  char *d_stage = nullptr;   // inputs and outputs of their host-pointer forms, grown on demand
  size_t stage_bytes = 0;
  std::string err;
};

static thread_local std::string g_park_create_error;

#define PARK_HIP(p, call)                                              \
  do {                                                                 \
    hipError_t _e = (call);                                            \
    if (_e != hipSuccess) {                                            \
      (p)->err = std::string(#call) + ": " + hipGetErrorString(_e);    \
      return HWY_PARK_ERR_HIP;                                         \
    }                                                                  \
  } while (0)

static int park_fail(hwy_park *p, int code, const std::string &msg) {
  if (p) p->err = msg; else g_park_create_error = msg;
  return code;
}
static size_t ego_bytes(const hwy_park *p) { return sizeof(double) * HWY_PARK_EGO_F64 * p->cfg.num_envs; }
static size_t ints_bytes(const hwy_park *p) { return sizeof(int32_t) * HWY_PARK_INTS * p->cfg.num_envs; }
static size_t order_bytes(const hwy_park *p) { return (size_t)HWY_PARK_MAX_PARKED * p->cfg.num_envs; }
static size_t parked_bytes(const hwy_park *p) { return sizeof(double) * HWY_PARK_PARKED_F64 * HWY_PARK_MAX_PARKED * p->cfg.num_envs; }

static hwy::ParkParams params_of(const hwy_park *p) {
  hwy::ParkParams q = hwy::park_params(p->cfg);
  q.ego = p->d_ego; q.ints = p->d_ints; q.order = p->d_order; q.parked = p->d_parked;
  return q;
}

extern "C" const char *hwy_park_last_error(const hwy_park *p) { return p ? p->err.c_str() : g_park_create_error.c_str(); }

extern "C" int hwy_park_destroy(hwy_park *p) {
  if (!p) return HWY_PARK_OK;
  (void)hipSetDevice(p->device);
  if (p->stream) (void)hipStreamSynchronize(p->stream);
  void *blocks[] = {p->d_ego, p->d_parked, p->d_ints, p->d_order, p->d_obs, p->d_reward, p->d_flags, p->d_mask, p->d_seeds, p->d_roll, p->d_goal, p->d_plan, p->d_stage};
  for (void *b : blocks)
    if (b) (void)hipFree(b);
  if (p->own_stream && p->stream) (void)hipStreamDestroy(p->stream);
  delete p;
  return HWY_PARK_OK;
}

extern "C" int hwy_park_create(const hwy_park_config *cfg, int device, void *stream, hwy_park **out) {
  if (!out) return park_fail(nullptr, HWY_PARK_ERR_INVALID_ARG, "out is NULL");
  *out = nullptr;
  const char *why = "";
  if (int rc = hwy::park_validate(cfg, &why)) return park_fail(nullptr, rc, why);
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n < 1)
    return park_fail(nullptr, HWY_PARK_ERR_NO_DEVICE, "no MI355X / HIP device available (there is no CPU fallback)");
  if (device < 0 || device >= n) return park_fail(nullptr, HWY_PARK_ERR_INVALID_ARG, "device index out of range");
  hwy_park *p = new hwy_park();
  p->cfg = *cfg;
  p->device = device;
#define PARK_CREATE(call)                                                                        \
  do {                                                                                           \
    hipError_t _e = (call);                                                                      \
    if (_e != hipSuccess) {                                                                      \
      g_park_create_error = std::string(#call) + ": " + hipGetErrorString(_e);                   \
      hwy_park_destroy(p);                                                                       \
      return HWY_PARK_ERR_HIP;                                                                   \
    }                                                                                            \
  } while (0)
  PARK_CREATE(hipSetDevice(device));
  if (stream) p->stream = (hipStream_t)stream;
  else {
    PARK_CREATE(hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking));
    p->own_stream = true;
  }
  const size_t E = (size_t)cfg->num_envs;
  PARK_CREATE(hipMalloc((void **)&p->d_ego, ego_bytes(p)));
  PARK_CREATE(hipMalloc((void **)&p->d_ints, ints_bytes(p)));
  PARK_CREATE(hipMalloc((void **)&p->d_order, order_bytes(p)));
  PARK_CREATE(hipMalloc((void **)&p->d_parked, parked_bytes(p)));
  PARK_CREATE(hipMalloc((void **)&p->d_obs, sizeof(float) * 18 * E));
  PARK_CREATE(hipMalloc((void **)&p->d_reward, sizeof(double) * E));
  PARK_CREATE(hipMalloc((void **)&p->d_flags, E));
  PARK_CREATE(hipMalloc((void **)&p->d_mask, E));
  PARK_CREATE(hipMalloc((void **)&p->d_seeds, sizeof(uint64_t) * E));
  PARK_CREATE(hipMemset(p->d_ego, 0, ego_bytes(p)));
  PARK_CREATE(hipMemset(p->d_ints, 0, ints_bytes(p)));
  PARK_CREATE(hipMemset(p->d_order, 0, order_bytes(p)));
  PARK_CREATE(hipMemset(p->d_parked, 0, parked_bytes(p)));
  PARK_CREATE(hipDeviceSynchronize());
#undef PARK_CREATE
  *out = p;
  return HWY_PARK_OK;
}

extern "C" int hwy_park_sync(hwy_park *p) {
  if (!p) return HWY_PARK_ERR_INVALID_ARG;
  PARK_HIP(p, hipSetDevice(p->device));
  PARK_HIP(p, hipStreamSynchronize(p->stream));
  return HWY_PARK_OK;
}

extern "C" int hwy_park_set_autoreset(hwy_park *p, int32_t enabled, uint64_t base_seed) {
  if (!p) return HWY_PARK_ERR_INVALID_ARG;
  p->cfg.autoreset = enabled ? 1 : 0;
  p->cfg.base_seed = base_seed;
  return HWY_PARK_OK;
}

extern "C" int hwy_park_set_state(hwy_park *p, const double *ego, const int32_t *ints, const uint8_t *order, const double *parked) {
  if (!p || !ego || !ints || !order || !parked) return park_fail(p, HWY_PARK_ERR_INVALID_ARG, "hwy_park_set_state: NULL argument");
  const size_t E = (size_t)p->cfg.num_envs;
  for (size_t e = 0; e < E; ++e) {  // what the kernel indexes by: checked here, not on the device
    const uint32_t occ = (uint32_t)ints[HWY_PARK_I_OCCUPIED * E + e];
    const int n = __builtin_popcount(occ);
    const int goal = ints[HWY_PARK_I_GOAL * E + e];
    if ((occ >> HWY_PARK_SPOTS) || n > HWY_PARK_MAX_PARKED || goal < 0 || goal >= HWY_PARK_SPOTS)
      return park_fail(p, HWY_PARK_ERR_INVALID_ARG, "hwy_park_set_state: occupancy mask or goal spot out of range");
    for (int k = HWY_PARK_I_STRUCK; k <= HWY_PARK_I_PIMPACT; ++k)
      if (n < 32 && ((uint32_t)ints[k * E + e] >> n))
        return park_fail(p, HWY_PARK_ERR_INVALID_ARG, "hwy_park_set_state: a list mask has a bit beyond the parked vehicles");
    for (int i = 0; i < n; ++i)
      if (order[(size_t)i * E + e] >= HWY_PARK_SPOTS || !((occ >> order[(size_t)i * E + e]) & 1u))
        return park_fail(p, HWY_PARK_ERR_INVALID_ARG, "hwy_park_set_state: order names a spot that is not occupied");
  }
  PARK_HIP(p, hipSetDevice(p->device));
  PARK_HIP(p, hipMemcpyAsync(p->d_ego, ego, ego_bytes(p), hipMemcpyHostToDevice, p->stream));
  PARK_HIP(p, hipMemcpyAsync(p->d_ints, ints, ints_bytes(p), hipMemcpyHostToDevice, p->stream));
  PARK_HIP(p, hipMemcpyAsync(p->d_order, order, order_bytes(p), hipMemcpyHostToDevice, p->stream));
  PARK_HIP(p, hipMemcpyAsync(p->d_parked, parked, parked_bytes(p), hipMemcpyHostToDevice, p->stream));
  PARK_HIP(p, hipStreamSynchronize(p->stream));
  return HWY_PARK_OK;
}

extern "C" int hwy_park_get_state(hwy_park *p, double *ego, int32_t *ints, uint8_t *order, double *parked) {
  if (!p || !ego || !ints || !order || !parked) return park_fail(p, HWY_PARK_ERR_INVALID_ARG, "hwy_park_get_state: NULL argument");
  PARK_HIP(p, hipSetDevice(p->device));
  PARK_HIP(p, hipMemcpyAsync(ego, p->d_ego, ego_bytes(p), hipMemcpyDeviceToHost, p->stream));
  PARK_HIP(p, hipMemcpyAsync(ints, p->d_ints, ints_bytes(p), hipMemcpyDeviceToHost, p->stream));
  PARK_HIP(p, hipMemcpyAsync(order, p->d_order, order_bytes(p), hipMemcpyDeviceToHost, p->stream));
  PARK_HIP(p, hipMemcpyAsync(parked, p->d_parked, parked_bytes(p), hipMemcpyDeviceToHost, p->stream));
  PARK_HIP(p, hipStreamSynchronize(p->stream));
  return HWY_PARK_OK;
}

static int observe_or_reset(hwy_park *p, bool reset, const uint8_t *mask, const uint64_t *seeds, float *obs) {
  const size_t E = (size_t)p->cfg.num_envs;
  PARK_HIP(p, hipSetDevice(p->device));
  hwy::ParkParams q = params_of(p);
  if (mask) {
    PARK_HIP(p, hipMemcpyAsync(p->d_mask, mask, E, hipMemcpyHostToDevice, p->stream));
    q.mask = p->d_mask;
  }
  if (seeds) {
    PARK_HIP(p, hipMemcpyAsync(p->d_seeds, seeds, sizeof(uint64_t) * E, hipMemcpyHostToDevice, p->stream));
    q.seeds = p->d_seeds;
  }
  q.obs = obs ? p->d_obs : nullptr;
  PARK_HIP(p, hwy::launch_park_reset(q, reset, p->stream));
  if (obs) PARK_HIP(p, hipMemcpyAsync(obs, p->d_obs, sizeof(float) * 18 * E, hipMemcpyDeviceToHost, p->stream));
  PARK_HIP(p, hipStreamSynchronize(p->stream));
  return HWY_PARK_OK;
}

extern "C" int hwy_park_reset(hwy_park *p, const uint8_t *mask, const uint64_t *seeds, float *obs) {
  if (!p) return HWY_PARK_ERR_INVALID_ARG;
  return observe_or_reset(p, true, mask, seeds, obs);
}

extern "C" int hwy_park_observe(hwy_park *p, float *obs) {
  if (!p || !obs) return park_fail(p, HWY_PARK_ERR_INVALID_ARG, "hwy_park_observe: NULL argument");
  return observe_or_reset(p, false, nullptr, nullptr, obs);
}

extern "C" int hwy_park_advance_device(hwy_park *p, int32_t k_steps, const float *d_actions, float *d_obs, double *d_reward,
                                       uint8_t *d_flags, double *d_step_reward, uint8_t *d_step_flags) {
  if (!p || !d_actions) return park_fail(p, HWY_PARK_ERR_INVALID_ARG, "hwy_park_advance_device: NULL argument");
  if (k_steps < 1 || k_steps > (1 << 16)) return park_fail(p, HWY_PARK_ERR_INVALID_ARG, "hwy_park_advance_device: k_steps must be in [1, 65536]");
  PARK_HIP(p, hipSetDevice(p->device));
  hwy::ParkParams q = params_of(p);
  q.k_steps = k_steps; q.actions = d_actions; q.obs = d_obs; q.reward = d_reward; q.flags = d_flags;
  q.step_reward = d_step_reward; q.step_flags = d_step_flags;
  PARK_HIP(p, hwy::launch_park_advance(q, p->stream));
  return HWY_PARK_OK;
}

extern "C" int hwy_park_advance(hwy_park *p, int32_t k_steps, const float *actions, float *obs, double *reward, uint8_t *flags,
                                double *step_reward, uint8_t *step_flags) {
  if (!p || !actions) return park_fail(p, HWY_PARK_ERR_INVALID_ARG, "hwy_park_advance: NULL argument");
  if (k_steps < 1 || k_steps > (1 << 16)) return park_fail(p, HWY_PARK_ERR_INVALID_ARG, "hwy_park_advance: k_steps must be in [1, 65536]");
  const size_t E = (size_t)p->cfg.num_envs, rows = (size_t)k_steps * E;
  if (!hwy::act_all_finite(actions, rows * 2)) return park_fail(p, HWY_PARK_ERR_ACTION, "hwy_park_advance: non-finite action");
  PARK_HIP(p, hipSetDevice(p->device));
  const size_t off_reward = rows * 2 * sizeof(float), off_flags = off_reward + rows * sizeof(double), need = off_flags + rows;
  if (need > p->roll_bytes) {
    PARK_HIP(p, hipStreamSynchronize(p->stream));
    if (p->d_roll) PARK_HIP(p, hipFree(p->d_roll));
    p->d_roll = nullptr;
    p->roll_bytes = 0;
    PARK_HIP(p, hipMalloc((void **)&p->d_roll, need));
    p->roll_bytes = need;
  }
  float *d_actions = (float *)p->d_roll;
  double *d_sr = (double *)(p->d_roll + off_reward);
  uint8_t *d_sf = (uint8_t *)(p->d_roll + off_flags);
  PARK_HIP(p, hipMemcpyAsync(d_actions, actions, rows * 2 * sizeof(float), hipMemcpyHostToDevice, p->stream));
  if (int rc = hwy_park_advance_device(p, k_steps, d_actions, p->d_obs, p->d_reward, p->d_flags, step_reward ? d_sr : nullptr,
                                       step_flags ? d_sf : nullptr))
    return rc;
  if (obs) PARK_HIP(p, hipMemcpyAsync(obs, p->d_obs, sizeof(float) * 18 * E, hipMemcpyDeviceToHost, p->stream));
  if (reward) PARK_HIP(p, hipMemcpyAsync(reward, p->d_reward, sizeof(double) * E, hipMemcpyDeviceToHost, p->stream));
  if (flags) PARK_HIP(p, hipMemcpyAsync(flags, p->d_flags, E, hipMemcpyDeviceToHost, p->stream));
  if (step_reward) PARK_HIP(p, hipMemcpyAsync(step_reward, d_sr, rows * sizeof(double), hipMemcpyDeviceToHost, p->stream));
  if (step_flags) PARK_HIP(p, hipMemcpyAsync(step_flags, d_sf, rows, hipMemcpyDeviceToHost, p->stream));
  PARK_HIP(p, hipStreamSynchronize(p->stream));
  return HWY_PARK_OK;
}

extern "C" int hwy_park_goal_reward_device(hwy_park *p, int64_t m, const double *d_achieved, const double *d_desired, double *d_out) {
  if (!p || !d_achieved || !d_desired || !d_out) return park_fail(p, HWY_PARK_ERR_INVALID_ARG, "hwy_park_goal_reward_device: NULL argument");
  if (m < 0 || m > ((int64_t)1 << 36)) return park_fail(p, HWY_PARK_ERR_INVALID_ARG, "hwy_park_goal_reward_device: m out of range");
  if (m == 0) return HWY_PARK_OK;
  PARK_HIP(p, hipSetDevice(p->device));
  hwy::ParkGoalParams g;
  g.achieved = d_achieved; g.desired = d_desired; g.out = d_out; g.m = m;
  for (int k = 0; k < 6; ++k) g.w[k] = p->cfg.reward_weights[k];
  PARK_HIP(p, hwy::launch_park_goal_reward(g, p->stream));
  return HWY_PARK_OK;
}

extern "C" int hwy_park_goal_reward(hwy_park *p, int64_t m, const double *achieved, const double *desired, double *out) {
  if (!p || !achieved || !desired || !out) return park_fail(p, HWY_PARK_ERR_INVALID_ARG, "hwy_park_goal_reward: NULL argument");
  if (m < 0 || m > ((int64_t)1 << 28)) return park_fail(p, HWY_PARK_ERR_INVALID_ARG, "hwy_park_goal_reward: m out of range");
  if (m == 0) return HWY_PARK_OK;
  PARK_HIP(p, hipSetDevice(p->device));
  if ((size_t)m > p->goal_rows) {
    PARK_HIP(p, hipStreamSynchronize(p->stream));
    if (p->d_goal) PARK_HIP(p, hipFree(p->d_goal));
    p->d_goal = nullptr;
    p->goal_rows = 0;
    PARK_HIP(p, hipMalloc((void **)&p->d_goal, sizeof(double) * 13 * (size_t)m));
    p->goal_rows = (size_t)m;
  }
  double *d_a = p->d_goal, *d_d = d_a + 6 * (size_t)m, *d_o = d_d + 6 * (size_t)m;
  PARK_HIP(p, hipMemcpyAsync(d_a, achieved, sizeof(double) * 6 * m, hipMemcpyHostToDevice, p->stream));
  PARK_HIP(p, hipMemcpyAsync(d_d, desired, sizeof(double) * 6 * m, hipMemcpyHostToDevice, p->stream));
  if (int rc = hwy_park_goal_reward_device(p, m, d_a, d_d, d_o)) return rc;
  PARK_HIP(p, hipMemcpyAsync(out, d_o, sizeof(double) * m, hipMemcpyDeviceToHost, p->stream));
  PARK_HIP(p, hipStreamSynchronize(p->stream));
  return HWY_PARK_OK;
}

// ---- sampling MPC (hwy_park_cem.h): one launch per search / per scoring pass ------------------------------------------------------------
static int plan_block(hwy_park *p) {  // the candidates' struck bodies
  if (!p->d_plan) PARK_HIP(p, hipMalloc((void **)&p->d_plan, hwy::park_cem_plane_bytes(p->cfg.num_envs)));
  return HWY_PARK_OK;
}
static int stage_block(hwy_park *p, size_t need) {
  if (need <= p->stage_bytes) return HWY_PARK_OK;
  PARK_HIP(p, hipStreamSynchronize(p->stream));
  if (p->d_stage) PARK_HIP(p, hipFree(p->d_stage));
  p->d_stage = nullptr;
  p->stage_bytes = 0;
  PARK_HIP(p, hipMalloc((void **)&p->d_stage, need));
  p->stage_bytes = need;
  return HWY_PARK_OK;
}
// the layout of a staging block: 8-byte items first; take() returns an offset, or npos for an item that is not wanted
struct ParkStage {
  static constexpr size_t npos = ~(size_t)0;
  size_t bytes = 0;
  size_t take(size_t n, bool want) {
    if (!want) return npos;
    const size_t at = bytes;
    bytes += (n + 7) & ~(size_t)7;
    return at;
  }
};
template <typename T>
static T *staged(hwy_park *p, size_t off) { return off == ParkStage::npos ? nullptr : (T *)(p->d_stage + off); }

static hwy::ParkCemParams cem_params_of(const hwy_park *p, const hwy_cem_params &c) {
  hwy::ParkCemParams q;
  memset(&q, 0, sizeof q);
  q.park = params_of(p);
  q.planes = p->d_plan;
  q.gamma = c.gamma; q.init_std = c.init_std; q.min_std = c.min_std; q.alpha = c.alpha; q.seed = c.seed;
  q.B = c.population; q.K = c.horizon; q.M = c.elites; q.I = c.iterations;
  return q;
}
static hwy_cem_params score_shape(int32_t branches, int32_t k_steps, double gamma) {  // a scoring pass under the search's caps
  hwy_cem_params c;
  memset(&c, 0, sizeof c);
  c.population = branches; c.elites = 1; c.iterations = 1; c.horizon = k_steps; c.gamma = gamma; c.alpha = 1.0;
  return c;
}

extern "C" int hwy_park_cem_plan_device(hwy_park *p, const hwy_cem_params *cem, const double *d_init_mean, float *d_action,
                                        double *d_best_return, double *d_mean, double *d_std, float *d_best_sequence, double *d_noise,
                                        float *d_samples, double *d_returns, int32_t *d_elites) {
  if (!p) return HWY_PARK_ERR_INVALID_ARG;
  const char *why = "";
  if (int rc = hwy::park_cem_validate(cem, &why)) return park_fail(p, rc, std::string("hwy_park_cem_plan: ") + why);
  if (!d_action) return park_fail(p, HWY_PARK_ERR_INVALID_ARG, "hwy_park_cem_plan: action must be non-NULL");
  PARK_HIP(p, hipSetDevice(p->device));
  if (int rc = plan_block(p)) return rc;
  hwy::ParkCemParams q = cem_params_of(p, *cem);
  q.init_mean = d_init_mean; q.action = d_action; q.best_return = d_best_return; q.mean = d_mean; q.stddev = d_std;
  q.best_sequence = d_best_sequence; q.noise = d_noise; q.samples = d_samples; q.returns = d_returns; q.elites = d_elites;
  PARK_HIP(p, hwy::launch_park_cem(q, true, p->stream));
  return HWY_PARK_OK;
}

extern "C" int hwy_park_cem_plan(hwy_park *p, const hwy_cem_params *cem, const double *init_mean, float *action, double *best_return,
                                 double *mean, double *stddev, float *best_sequence, double *noise, float *samples, double *returns,
                                 int32_t *elites) {
  if (!p) return HWY_PARK_ERR_INVALID_ARG;
  const char *why = "";
  if (int rc = hwy::park_cem_validate(cem, &why)) return park_fail(p, rc, std::string("hwy_park_cem_plan: ") + why);
  if (!action) return park_fail(p, HWY_PARK_ERR_INVALID_ARG, "hwy_park_cem_plan: action must be non-NULL");
  const size_t E = (size_t)p->cfg.num_envs, cols = E * cem->horizon * 2, I = (size_t)cem->iterations;
  const size_t draws = I * E * cem->population * cem->horizon * 2, rets = I * E * cem->population, el = I * E * cem->elites;
  if (init_mean && !hwy::cem_all_finite(init_mean, cols)) return park_fail(p, HWY_PARK_ERR_ACTION, "hwy_park_cem_plan: non-finite init_mean");
  PARK_HIP(p, hipSetDevice(p->device));
  ParkStage st;
  const size_t o_init = st.take(cols * 8, init_mean), o_best = st.take(E * 8, best_return), o_mean = st.take(cols * 8, mean);
  const size_t o_std = st.take(cols * 8, stddev), o_noise = st.take(draws * 8, noise), o_rets = st.take(rets * 8, returns);
  const size_t o_action = st.take(E * 2 * 4, true), o_seq = st.take(cols * 4, best_sequence), o_samples = st.take(draws * 4, samples);
  const size_t o_elites = st.take(el * 4, elites);
  if (int rc = stage_block(p, st.bytes)) return rc;
  if (init_mean) PARK_HIP(p, hipMemcpyAsync(p->d_stage + o_init, init_mean, cols * 8, hipMemcpyHostToDevice, p->stream));
  if (int rc = hwy_park_cem_plan_device(p, cem, staged<double>(p, o_init), staged<float>(p, o_action), staged<double>(p, o_best),
                                        staged<double>(p, o_mean), staged<double>(p, o_std), staged<float>(p, o_seq),
                                        staged<double>(p, o_noise), staged<float>(p, o_samples), staged<double>(p, o_rets),
                                        staged<int32_t>(p, o_elites)))
    return rc;
  const struct { void *dst; size_t off, bytes; } back[] = {
      {action, o_action, E * 2 * 4}, {best_return, o_best, E * 8}, {mean, o_mean, cols * 8}, {stddev, o_std, cols * 8},
      {best_sequence, o_seq, cols * 4}, {noise, o_noise, draws * 8}, {samples, o_samples, draws * 4}, {returns, o_rets, rets * 8},
      {elites, o_elites, el * 4}};
  for (const auto &b : back)
    if (b.dst) PARK_HIP(p, hipMemcpyAsync(b.dst, p->d_stage + b.off, b.bytes, hipMemcpyDeviceToHost, p->stream));
  PARK_HIP(p, hipStreamSynchronize(p->stream));
  return HWY_PARK_OK;
}

extern "C" int hwy_park_score_device(hwy_park *p, int32_t branches, int32_t k_steps, double gamma, const float *d_actions, double *d_ret,
                                     double *d_step_reward, uint8_t *d_step_flags) {
  if (!p) return HWY_PARK_ERR_INVALID_ARG;
  const hwy_cem_params shape = score_shape(branches, k_steps, gamma);
  const char *why = "";
  if (int rc = hwy::park_cem_validate(&shape, &why)) return park_fail(p, rc, std::string("hwy_park_score (population = branches, horizon = k_steps): ") + why);
  if (!d_actions || !d_ret) return park_fail(p, HWY_PARK_ERR_INVALID_ARG, "hwy_park_score: actions and ret must be non-NULL");
  PARK_HIP(p, hipSetDevice(p->device));
  if (int rc = plan_block(p)) return rc;
  hwy::ParkCemParams q = cem_params_of(p, shape);
  q.actions = d_actions; q.ret = d_ret; q.step_reward = d_step_reward; q.step_flags = d_step_flags;
  PARK_HIP(p, hwy::launch_park_cem(q, false, p->stream));
  return HWY_PARK_OK;
}

extern "C" int hwy_park_score(hwy_park *p, int32_t branches, int32_t k_steps, double gamma, const float *actions, double *ret,
                              double *step_reward, uint8_t *step_flags) {
  if (!p) return HWY_PARK_ERR_INVALID_ARG;
  const hwy_cem_params shape = score_shape(branches, k_steps, gamma);
  const char *why = "";
  if (int rc = hwy::park_cem_validate(&shape, &why)) return park_fail(p, rc, std::string("hwy_park_score (population = branches, horizon = k_steps): ") + why);
  if (!actions || !ret) return park_fail(p, HWY_PARK_ERR_INVALID_ARG, "hwy_park_score: actions and ret must be non-NULL");
  const size_t rows = (size_t)p->cfg.num_envs * branches, steps = rows * k_steps;
  if (!hwy::act_all_finite(actions, steps * 2)) return park_fail(p, HWY_PARK_ERR_ACTION, "hwy_park_score: non-finite action");
  PARK_HIP(p, hipSetDevice(p->device));
  ParkStage st;
  const size_t o_ret = st.take(rows * 8, true), o_sr = st.take(steps * 8, step_reward), o_act = st.take(steps * 2 * 4, true);
  const size_t o_sf = st.take(steps, step_flags);
  if (int rc = stage_block(p, st.bytes)) return rc;
  PARK_HIP(p, hipMemcpyAsync(p->d_stage + o_act, actions, steps * 2 * 4, hipMemcpyHostToDevice, p->stream));
  if (int rc = hwy_park_score_device(p, branches, k_steps, gamma, staged<float>(p, o_act), staged<double>(p, o_ret),
                                     staged<double>(p, o_sr), staged<uint8_t>(p, o_sf)))
    return rc;
  PARK_HIP(p, hipMemcpyAsync(ret, p->d_stage + o_ret, rows * 8, hipMemcpyDeviceToHost, p->stream));
  if (step_reward) PARK_HIP(p, hipMemcpyAsync(step_reward, p->d_stage + o_sr, steps * 8, hipMemcpyDeviceToHost, p->stream));
  if (step_flags) PARK_HIP(p, hipMemcpyAsync(step_flags, p->d_stage + o_sf, steps, hipMemcpyDeviceToHost, p->stream));
  PARK_HIP(p, hipStreamSynchronize(p->stream));
  return HWY_PARK_OK;
}

// ---- MPPI (hwy_park_mppi.h): one launch per search.  The parameters are checked before the handle, so a refusal needs no device ---------
extern "C" int hwy_park_mppi_plan_device(hwy_park *p, const hwy_park_mppi_params *mppi, const double *d_init_mean, float *d_action,
                                         double *d_best_return, double *d_mean, double *d_weights_ess, double *d_noise, float *d_samples,
                                         double *d_returns, double *d_weights, double *d_mean_history) {
  const char *why = "";
  if (int rc = hwy::park_mppi_validate(mppi, &why)) return park_fail(p, rc, std::string("hwy_park_mppi_plan: ") + why);
  if (!p) return park_fail(nullptr, HWY_PARK_ERR_INVALID_ARG, "hwy_park_mppi_plan: the handle is NULL");
  if (!d_action) return park_fail(p, HWY_PARK_ERR_INVALID_ARG, "hwy_park_mppi_plan: action must be non-NULL");
  PARK_HIP(p, hipSetDevice(p->device));
  if (int rc = plan_block(p)) return rc;
  hwy::ParkMppiParams q;
  memset(&q, 0, sizeof q);
  q.park = params_of(p);
  q.planes = p->d_plan;
  q.init_mean = d_init_mean; q.action = d_action; q.best_return = d_best_return; q.mean = d_mean; q.weights_ess = d_weights_ess;
  q.noise = d_noise; q.samples = d_samples; q.returns = d_returns; q.weights = d_weights; q.mean_history = d_mean_history;
  q.gamma = mppi->gamma; q.noise_std = mppi->noise_std; q.temperature = mppi->temperature; q.beta = mppi->beta; q.beta_c = mppi->beta_c;
  q.alpha = mppi->alpha; q.seed = mppi->seed;
  q.B = mppi->population; q.K = mppi->horizon; q.I = mppi->iterations;
  PARK_HIP(p, hwy::launch_park_mppi(q, p->stream));
  return HWY_PARK_OK;
}

extern "C" int hwy_park_mppi_plan(hwy_park *p, const hwy_park_mppi_params *mppi, const double *init_mean, float *action, double *best_return,
                                  double *mean, double *weights_ess, double *noise, float *samples, double *returns, double *weights,
                                  double *mean_history) {
  const char *why = "";
  if (int rc = hwy::park_mppi_validate(mppi, &why)) return park_fail(p, rc, std::string("hwy_park_mppi_plan: ") + why);
  if (!p) return park_fail(nullptr, HWY_PARK_ERR_INVALID_ARG, "hwy_park_mppi_plan: the handle is NULL");
  if (!action) return park_fail(p, HWY_PARK_ERR_INVALID_ARG, "hwy_park_mppi_plan: action must be non-NULL");
  const size_t E = (size_t)p->cfg.num_envs, cols = E * mppi->horizon * 2, I = (size_t)mppi->iterations;
  const size_t draws = I * E * mppi->population * mppi->horizon * 2, rets = I * E * mppi->population, hist = (I + 1) * cols;
  if (init_mean && !hwy::cem_all_finite(init_mean, cols)) return park_fail(p, HWY_PARK_ERR_ACTION, "hwy_park_mppi_plan: non-finite init_mean");
  PARK_HIP(p, hipSetDevice(p->device));
  ParkStage st;
  const size_t o_init = st.take(cols * 8, init_mean), o_best = st.take(E * 8, best_return), o_mean = st.take(cols * 8, mean);
  const size_t o_ess = st.take(E * 8, weights_ess), o_noise = st.take(draws * 8, noise), o_rets = st.take(rets * 8, returns);
  const size_t o_w = st.take(rets * 8, weights), o_hist = st.take(hist * 8, mean_history), o_action = st.take(E * 2 * 4, true);
  const size_t o_samples = st.take(draws * 4, samples);
  if (int rc = stage_block(p, st.bytes)) return rc;
  if (init_mean) PARK_HIP(p, hipMemcpyAsync(p->d_stage + o_init, init_mean, cols * 8, hipMemcpyHostToDevice, p->stream));
  if (int rc = hwy_park_mppi_plan_device(p, mppi, staged<double>(p, o_init), staged<float>(p, o_action), staged<double>(p, o_best),
                                         staged<double>(p, o_mean), staged<double>(p, o_ess), staged<double>(p, o_noise),
                                         staged<float>(p, o_samples), staged<double>(p, o_rets), staged<double>(p, o_w),
                                         staged<double>(p, o_hist)))
    return rc;
  const struct { void *dst; size_t off, bytes; } back[] = {
      {action, o_action, E * 2 * 4}, {best_return, o_best, E * 8}, {mean, o_mean, cols * 8}, {weights_ess, o_ess, E * 8},
      {noise, o_noise, draws * 8}, {samples, o_samples, draws * 4}, {returns, o_rets, rets * 8}, {weights, o_w, rets * 8},
      {mean_history, o_hist, hist * 8}};
  for (const auto &b : back)
    if (b.dst) PARK_HIP(p, hipMemcpyAsync(b.dst, p->d_stage + b.off, b.bytes, hipMemcpyDeviceToHost, p->stream));
  PARK_HIP(p, hipStreamSynchronize(p->stream));
  return HWY_PARK_OK;
}
