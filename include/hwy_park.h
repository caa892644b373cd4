/* hwy_park.h -- C-ABI of the parking scenario (the reference's ParkingEnv, envs/parking_env.py): goal-conditioned continuous
 * control, E environments of ONE moving rectangle (the ContinuousAction ego), up to 26 resting ones and four walls, advanced by
 * a kernel of its own (csrc/hwy_park.h: one THREAD per environment).  A door next to the engine of hwy_engine.h: an opaque handle
 * of its own, exported from the same shared library; hwy_config and the engine's ABI version are not involved.  Sampling MPC on it
 * (hwy_park_cem_plan, hwy_park_score: csrc/hwy_park_cem.h, one WAVEFRONT per environment, a candidate per lane) takes the engine's
 * hwy_cem_params; nothing else of hwy_engine.h is used.
 *
 * Scope (hwy_park_create returns HWY_PARK_ERR_INVALID_ARG outside it, before anything reaches the device): one controlled vehicle,
 * vehicles_count 0 .. 26, walls or none, 1 .. 15 frames per policy step, the six default features in their default order, a
 * ContinuousAction with both axes and clip, any acceleration_range, a steering_range within +-pi/3.
 *
 * State, struct-of-arrays over environments ([field][E]; the host forms below take and return exactly these planes):
 *   ego     f64 [HWY_PARK_EGO_F64][E]   x, y, heading, speed, stored acceleration, stored steering, impact_x, impact_y, time
 *   ints    i32 [HWY_PARK_INTS][E]      flags (HWY_PARK_F_*), policy steps, episode, goal spot, occupancy mask over the 28 spots,
 *                                       and three masks over the LIST index of the parked vehicles: struck, crashed, has_impact
 *   order   u8  [26][E]                 spot of the i-th parked vehicle of Road.vehicles (i < popcount(occupancy))
 *   parked  f64 [HWY_PARK_PARKED_F64][26][E]   x, y, impact_x, impact_y of parked vehicle i; read and written only once its
 *                                       struck bit is set (a vehicle that was never struck is fully described by its spot; heading and
 *                                       speed of a parked vehicle never change: its action is (0, 0) and its speed 0)
 * Spot k: k < 14 is lane ("a", "b", k) (y = +14, heading +pi/2), k >= 14 lane ("b", "c", k - 14) (y = -14, heading -pi/2);
 * x = 4 (k mod 14) - 26: the order of RoadNetwork.lanes_dict().
 */
#ifndef HWY_PARK_H
#define HWY_PARK_H

#include <stddef.h>
#include <stdint.h>

#include "hwy_engine.h" /* hwy_cem_params */

#ifdef __cplusplus
extern "C" {
#endif

#define HWY_PARK_SPOTS 28
#define HWY_PARK_MAX_PARKED 26
#define HWY_PARK_MAX_FRAMES 15
#define HWY_PARK_EGO_F64 9
#define HWY_PARK_INTS 8
#define HWY_PARK_PARKED_F64 4

enum { HWY_PARK_OK = 0, HWY_PARK_ERR_INVALID_ARG = 1, HWY_PARK_ERR_HIP = 2, HWY_PARK_ERR_NO_DEVICE = 4, HWY_PARK_ERR_ACTION = 5 };
/* ints plane 0 */
enum { HWY_PARK_F_CRASHED = 1, HWY_PARK_F_HAS_IMPACT = 2, HWY_PARK_F_DONE = 4 };
/* planes of `ego` and of `ints` */
enum { HWY_PARK_X = 0, HWY_PARK_Y, HWY_PARK_HEADING, HWY_PARK_SPEED, HWY_PARK_ACCEL, HWY_PARK_STEER, HWY_PARK_IMPACT_X,
       HWY_PARK_IMPACT_Y, HWY_PARK_TIME };
enum { HWY_PARK_I_FLAGS = 0, HWY_PARK_I_STEPS, HWY_PARK_I_EPISODE, HWY_PARK_I_GOAL, HWY_PARK_I_OCCUPIED, HWY_PARK_I_STRUCK,
       HWY_PARK_I_PCRASHED, HWY_PARK_I_PIMPACT };
/* bits of the optional per-step flag bytes of hwy_park_advance */
enum { HWY_PARK_S_TERMINATED = 1, HWY_PARK_S_TRUNCATED = 2, HWY_PARK_S_SUCCESS = 4, HWY_PARK_S_CRASHED = 8 };

typedef struct hwy_park_config {
  int32_t struct_size;   /* sizeof(hwy_park_config) */
  int32_t num_envs;
  int32_t vehicles_count; /* 0 .. 26 (the reference `continue`s once no spot is free: 26 is every spot) */
  int32_t add_walls;
  int32_t frames;        /* simulation_frequency // policy_frequency, 1 .. 15 */
  int32_t autoreset;     /* NextStep: an environment that ended is re-spawned by the next advance call */
  double dt;             /* 1 / simulation_frequency */
  double policy_dt;      /* 1 / policy_frequency: what AbstractEnv.step adds to `time` */
  double duration;
  double reward_weights[6];
  double scales[6];
  double success_goal_reward, collision_reward;
  double acceleration_range[2], steering_range[2]; /* of the ContinuousAction (NOT the config's top-level "steering_range") */
  uint64_t base_seed;    /* device reset and auto-reset: environment e draws from (base_seed + e, episode) */
} hwy_park_config;

typedef struct hwy_park hwy_park;

/* stream: a hipStream_t the handle enqueues on, or NULL (it creates one). */
int hwy_park_create(const hwy_park_config *cfg, int device, void *stream, hwy_park **out);
int hwy_park_destroy(hwy_park *p);
const char *hwy_park_last_error(const hwy_park *p);
/* Device reset of the environments with mask[e] != 0 (NULL: all): episode 0 of (seeds[e] or base_seed + e) on the Philox stream,
 * the first observation into obs (host, float32 [E][3][6], may be NULL). */
int hwy_park_reset(hwy_park *p, const uint8_t *mask, const uint64_t *seeds, float *obs);
/* Auto-reset (NextStep) on or off and the seed its re-spawns draw from; replaces the config's two fields. */
int hwy_park_set_autoreset(hwy_park *p, int32_t enabled, uint64_t base_seed);
int hwy_park_set_state(hwy_park *p, const double *ego, const int32_t *ints, const uint8_t *order, const double *parked);
int hwy_park_get_state(hwy_park *p, double *ego, int32_t *ints, uint8_t *order, double *parked);
/* k_steps >= 1 policy steps in ONE launch, bit-identical to k_steps launches.  actions: float32 [k_steps][E][2].  Outputs of the
 * last step: obs float32 [E][3][6] (observation, achieved_goal, desired_goal), reward f64 [E], flags u8 [E] (HWY_PARK_S_*);
 * step_reward f64 [k_steps][E] and step_flags u8 [k_steps][E] may be NULL.  The host form rejects non-finite actions
 * (HWY_PARK_ERR_ACTION); on the device form such a row keeps its stored controls.  The device form enqueues on the handle's stream
 * and returns; no host round trip. */
int hwy_park_advance(hwy_park *p, int32_t k_steps, const float *actions, float *obs, double *reward, uint8_t *flags,
                     double *step_reward, uint8_t *step_flags);
int hwy_park_advance_device(hwy_park *p, int32_t k_steps, const float *d_actions, float *d_obs, double *d_reward, uint8_t *d_flags,
                            double *d_step_reward, uint8_t *d_step_flags);
int hwy_park_observe(hwy_park *p, float *obs);
/* ParkingEnv.compute_reward (p = 0.5) of m rows of six features: -sqrt(dot(|achieved - desired|, reward_weights)), f64 [m]. */
int hwy_park_goal_reward_device(hwy_park *p, int64_t m, const double *d_achieved, const double *d_desired, double *d_out);
int hwy_park_goal_reward(hwy_park *p, int64_t m, const double *achieved, const double *desired, double *out);
int hwy_park_sync(hwy_park *p);

/* ---- sampling MPC (csrc/hwy_park_cem.h): a cross-entropy-method search of every environment in ONE launch --------------------
 * The parameters are hwy_engine.h's hwy_cem_params under parking's own, tighter caps: population 1 .. HWY_PARK_CEM_MAX_POP, elites
 * 1 .. population, horizon 1 .. HWY_PARK_CEM_MAX_HORIZON, population * horizon <= HWY_PARK_CEM_MAX_SAMPLES, iterations 1 ..
 * HWY_PARK_CEM_MAX_ITERATIONS, gamma finite, init_std and min_std finite and >= 0, alpha in [0, 1]; HWY_PARK_ERR_INVALID_ARG with a
 * reason in hwy_park_last_error otherwise.  The environments of the handle are the parents: they are read, never written; the
 * handle's autoreset setting is not read, an environment that has ended is stepped as it is.  Candidates keep the bodies they
 * strike in a block of the handle, f64 [4][26][64 E] (53 248 bytes per environment), allocated by the first call.
 *
 * hwy_park_cem_plan_device: DEVICE pointers, enqueued on the handle's stream, no host round trip.  d_init_mean f64 [E][K][2] or NULL
 * (zeros; not validated here).  d_action f32 [E][2]: step 0 of the best sequence.  Optional (NULL: not written): d_best_return f64
 * [E], d_mean / d_std f64 [E][K][2], d_best_sequence f32 [E][K][2], d_noise f64 and d_samples f32 [I][E][B][K][2], d_returns f64
 * [I][E][B], d_elites i32 [I][E][M] (every iteration's elite branches, ascending).
 * hwy_park_cem_plan: the same with HOST pointers; stages, HWY_PARK_ERR_ACTION for a non-finite init_mean before anything runs,
 * synchronises.
 * hwy_park_score_device: the discounted returns d_ret f64 [E][B] of B = branches given sequences of K = k_steps action pairs,
 * d_actions f32 [E][B][K][2], each stepped from its environment's current state; an episode that ends within a sequence is
 * absorbing.  Optional d_step_reward f64 [E][B][K] and d_step_flags u8 [E][B][K] (HWY_PARK_S_*) of every step, as an advance of K
 * steps without autoreset gives them.  A non-finite pair keeps the stored controls.  The caps are the search's (population =
 * branches, horizon = k_steps).  hwy_park_score: HOST pointers; HWY_PARK_ERR_ACTION for non-finite actions before anything runs. */
#define HWY_PARK_CEM_MAX_POP 256
#define HWY_PARK_CEM_MAX_HORIZON 32
#define HWY_PARK_CEM_MAX_SAMPLES 4096  /* population * horizon: the sample table in LDS, 32 KB */
#define HWY_PARK_CEM_MAX_ITERATIONS 16
int hwy_park_cem_plan_device(hwy_park *p, const hwy_cem_params *cem, const double *d_init_mean, float *d_action, double *d_best_return,
                             double *d_mean, double *d_std, float *d_best_sequence, double *d_noise, float *d_samples,
                             double *d_returns, int32_t *d_elites);
int hwy_park_cem_plan(hwy_park *p, const hwy_cem_params *cem, const double *init_mean, float *action, double *best_return,
                      double *mean, double *stddev, float *best_sequence, double *noise, float *samples, double *returns,
                      int32_t *elites);
int hwy_park_score_device(hwy_park *p, int32_t branches, int32_t k_steps, double gamma, const float *d_actions, double *d_ret,
                          double *d_step_reward, uint8_t *d_step_flags);
int hwy_park_score(hwy_park *p, int32_t branches, int32_t k_steps, double gamma, const float *actions, double *ret,
                   double *step_reward, uint8_t *step_flags);

/* ---- MPPI (csrc/hwy_park_mppi.h): a model-predictive path integral search of every environment in ONE launch ------------------
 * A second planner on the same simulator, white noise, caps and struck-body block as the CEM search.  Per environment, with a mean
 * u f64 [K][2] (d_init_mean or zeros): every iteration draws B candidates x = (float)clip(u + noise_std * n, -1, 1), where n is the
 * CEM search's white noise z coloured per axis by n[0] = z[0], n[k] = beta * n[k-1] + beta_c * z[k] (candidate 0: n = 0), rolls
 * each out to its discounted return g, weighs it w = exp((g - max g) / temperature) and moves the mean to
 * u = alpha * (sum w x / sum w) + (1 - alpha) * u.  The action is (float)clip(u[0], -1, 1) after the last iteration.
 * population, horizon, their product and iterations under the HWY_PARK_CEM_MAX_* caps, gamma finite, noise_std finite and >= 0,
 * temperature finite and > 0, 0 <= beta < 1, beta_c = sqrt(1 - beta * beta) computed by the caller in double, alpha in [0, 1];
 * HWY_PARK_ERR_INVALID_ARG with a reason in hwy_park_last_error otherwise (checked before the handle: hwy_park_last_error(NULL)
 * holds the reason when p is NULL).
 *
 * hwy_park_mppi_plan_device: DEVICE pointers, enqueued on the handle's stream, no host round trip.  d_action f32 [E][2].  Optional
 * (NULL: not written): d_best_return f64 [E] (the highest return any candidate of the search reached), d_mean f64 [E][K][2],
 * d_weights_ess f64 [E] (the effective sample size (sum w)^2 / sum w^2 of the last iteration), d_noise f64 (the coloured n) and
 * d_samples f32 [I][E][B][K][2], d_returns and d_weights f64 [I][E][B], d_mean_history f64 [I + 1][E][K][2] (the mean before
 * iteration 0 and after every iteration).
 * hwy_park_mppi_plan: the same with HOST pointers; stages, HWY_PARK_ERR_ACTION for a non-finite init_mean before anything runs,
 * synchronises. */
typedef struct hwy_park_mppi_params {
  int32_t struct_size;   /* sizeof(hwy_park_mppi_params) */
  int32_t population, iterations, horizon;
  double gamma, noise_std, temperature;
  double beta, beta_c;   /* beta_c = sqrt(1 - beta * beta) */
  double alpha;
  uint64_t seed;
} hwy_park_mppi_params;
int hwy_park_mppi_plan_device(hwy_park *p, const hwy_park_mppi_params *mppi, const double *d_init_mean, float *d_action,
                              double *d_best_return, double *d_mean, double *d_weights_ess, double *d_noise, float *d_samples,
                              double *d_returns, double *d_weights, double *d_mean_history);
int hwy_park_mppi_plan(hwy_park *p, const hwy_park_mppi_params *mppi, const double *init_mean, float *action, double *best_return,
                       double *mean, double *weights_ess, double *noise, float *samples, double *returns, double *weights,
                       double *mean_history);

#ifdef __cplusplus
}
#endif
#endif
