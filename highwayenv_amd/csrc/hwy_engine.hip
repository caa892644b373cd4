// hwy_engine.hip -- C-ABI host side of the MI355X HighwayEnv step engine (include/hwy_engine.h).
//
// Owns the device-resident struct-of-arrays of E environments x N vehicles, one HIP stream,
// pinned staging buffers for the host-pointer entry points, and HIP-event kernel timing.
// There is deliberately NO CPU implementation behind these entry points: without a GPU
// hwy_create fails with HWY_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <algorithm>
#include <string>
#include <vector>

#include "../../include/hwy_engine.h"
#include "hwy_comm.h"
#include "hwy_launch.h"
#include "hwy_act.h"
#include "hwy_mask.h"
#include "hwy_params.h"

using hwy::StepParams;

struct hwy_engine {
  hwy_config cfg{};
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  int pitch = 0;
  bool force_block_kernel = false;  // hwy_config.tune_block_kernel: use the generic workgroup kernel even for N <= 64
  int waves_per_eu = 3;  // register-allocation variant of the step kernel (hwy_config.tune_waves_per_eu)
  int rollout_waves_per_eu = 3;  // ... and of the multi-step kernel (hwy_rollout_device)
  int prio_shift = 0;    // issue-priority turns of the step kernels (hwy_config.tune_prio_shift; 0 = off)
  // device state
  double *d_f64 = nullptr;   // 9 fields x E x pitch
  double *d_behavior = nullptr;  // HWY_TRAFFIC_LINEAR: HWY_BEHAVIOR_PARAMS planes x E x pitch (hwy_set_behavior)
  double *d_controls = nullptr;  // HWY_EGO_DIRECT: stored acceleration | steering of every agent, 2 x E x A (hwy_set_controls)
  int32_t *d_packed = nullptr;
  long long *d_route = nullptr;     // intersection scenario: planned routes [E x pitch] (64-bit route words)
  int32_t *d_road_steps = nullptr;  // intersection scenario: RegulatedRoad.steps [E]
  hwy_glane *d_gnet = nullptr;      // intersection scenario: lane table
  double *d_shadow_f64 = nullptr;   // intersection scenario, pre-warming of next episodes: second copy of the planes
  int32_t *d_shadow_packed = nullptr, *d_shadow_meta = nullptr;
  long long *d_shadow_route = nullptr;
  unsigned long long *d_counters = nullptr;  // [HWY_CTR_COUNT] (hwy_get_counters)
  uint16_t *d_block_env = nullptr;           // [E] hwy_set_block_order (nullptr: workgroup b steps environment b)
  double *d_time = nullptr;
  uint8_t *d_done = nullptr;
  uint32_t *d_episode = nullptr;
  // device I/O buffers for the host-pointer entry points
  int32_t *d_actions = nullptr;
  // step outputs of the host-pointer entry points live in ONE device block (reward | speed | obs | term | trunc |
  // crashed) mirrored by one pinned host block, so that hwy_step needs a single D2H copy
  char *d_out = nullptr;
  char *d_roll = nullptr;  // hwy_rollout (host pointers): K blocks of actions + outputs, grown on demand
  size_t roll_bytes = 0;
  size_t out_bytes = 0, off_reward = 0, off_speed = 0, off_obs = 0, off_term = 0, off_trunc = 0, off_crashed = 0;
  float *d_obs = nullptr;
  double *d_reward = nullptr, *d_info_speed = nullptr;
  uint8_t *d_term = nullptr, *d_trunc = nullptr, *d_info_crashed = nullptr;
  uint8_t *d_mask = nullptr;
  uint64_t *d_seeds = nullptr;
  int32_t *d_grid_ws = nullptr;  // OccupancyGrid workspace [E][A][2][W*H]
  // outputs of the host-pointer planner entry points (hwy_ttc_grid / hwy_mdp_plan), allocated on first use
  float *d_ttc_grid = nullptr;   // [E][A][ttc_cells]
  int ttc_cells = 0;
  int32_t *d_plan_action = nullptr;  // [E][A]
  double *d_plan_q = nullptr;        // [E][A][5]
  // output of the host-pointer form of the action mask (hwy_action_mask), allocated on first use
  uint8_t *d_action_mask = nullptr;  // [E][A][n_ids]
  // the observation doors (hwy_collision_obs.h, hwy_lidar_door.h), allocated on first use: the step's own observation (the step
  // kernels keep writing the engine's obs_type, so the shape kernels stay the launch; nobody reads it) and the TimeToCollision host
  // form's output
  float *d_door_step_obs = nullptr;  // [E][A][obs_len]
  float *d_ttc_obs = nullptr;       // [E][A][9 * HWY_MAX_TTC_STEPS]
  // the Lidar door (hwy_lidar_door.h): the host form's output, allocated on first use; whether the planes hold a state at all
  // (hwy_reset, hwy_set_state or a fork into this engine has run)
  float *d_lidar_door_obs = nullptr;  // [E][A][HWY_MAX_LIDAR_DOOR_CELLS][2]
  bool has_state = false;
  // hwy_fork / hwy_fork_device: the uploaded source indices [E] (host form) and the event that orders this engine's stream behind
  // the source engine's, both created on first use
  int32_t *d_fork_src = nullptr;
  hipEvent_t fork_event = nullptr;
  // hwy_opd_plan_device (this engine as `tree`): the trees' bookkeeping, the index arrays of the forks, the work engine's action
  // plane and the host form's outputs, in one block allocated on first use
  char *d_opd = nullptr;
  size_t opd_bytes = 0;
  // hwy_cem_plan_device (this engine as `work`): the action block the sample kernel writes, the rollout's outputs, the returns, the
  // search's mean / std / best sequence and the host form's outputs, in one block allocated on first use
  char *d_cem = nullptr;
  size_t cem_bytes = 0;
  // pinned host staging
  void *h_pinned = nullptr;
  size_t h_pinned_bytes = 0;
  // auto-reset
  int autoreset = 0;
  hwy::ResetParams rp{};
  // profiling
  int profiling = 0;        // 0 = off, k > 0 = HIP events around every k-th step-kernel launch
  int64_t launch_counter = 0;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> events;
  size_t events_used = 0;
  double prof_ms = 0.0;
  int64_t prof_launches = 0;
  // self-selection of the issue-priority turn (hwy_config.tune_prio_shift == 0 and turns apply): the first full-step launches are
  // timed with the dispatch's own timestamps, the candidates interleaved (drift of the workload cancels), the best one is kept
  struct TurnTuner {
    enum { IDLE = 0, SAMPLING = 1, DONE = 2 };
    int state = IDLE, stage = 0, launches = 0;
    int cand[5] = {0, 0, 0, 0, 0};
    double ms[5] = {0, 0, 0, 0, 0};
    int n[5] = {0, 0, 0, 0, 0};
    std::vector<std::pair<hipEvent_t, hipEvent_t>> events;
    std::vector<int> which;
  } tuner;
  hwy::Comm *comm = nullptr;  // hwy_comm_init
  std::string err;
};

static thread_local std::string g_create_error;

#define HWY_HIP(eng, call)                                                                        \
  do {                                                                                            \
    hipError_t _e = (call);                                                                       \
    if (_e != hipSuccess) {                                                                       \
      (eng)->err = std::string(#call) + ": " + hipGetErrorString(_e);                             \
      return HWY_ERR_HIP;                                                                         \
    }                                                                                             \
  } while (0)

static int fail(hwy_engine *eng, int code, const std::string &msg) {
  if (eng) eng->err = msg; else g_create_error = msg;
  return code;
}

// ---- the engine picks the length of an issue-priority turn itself ---------------------------------------------------------------
// Scheduling only: no result depends on the turn (tests/test_engine_parity.py compares turn variants bit for bit).
// Candidates: 0.75 / 0.875 / 1 / 1.125 / 1.25 x the scenario default, in units of 64 clock ticks (the linear encoding of
// tune_prio_shift), visited round-robin over the first (HWY_TUNE_ROUNDS + 1) x 5 full-step launches, each timed by the dispatch's own
// begin / end timestamps (hipExtLaunchKernelGGL: the events of hwy_profile_*); one synchronisation at the end of a stage.  If the
// best candidate sits at an end of the range, one more stage is centred there (at most HWY_TUNE_STAGES).  While hwy_profile_enable
// is on the tuner pauses.
#define HWY_TUNE_ROUNDS 16
#define HWY_TUNE_STAGES 3
static int turn_in_ticks64(int turn) {  // the linear unit of either encoding (0 = not expressible: a turn below 64 x 64 ticks)
  if (turn >= 64) return turn;
  if (turn >= 12 && turn <= 26) return 1 << (turn - 6);
  return 0;
}
static void tuner_arm(hwy_engine *eng, int centre_turn) {
  auto &t = eng->tuner;
  const int k = turn_in_ticks64(centre_turn);
  if (k < 64) { t.state = hwy_engine::TurnTuner::DONE; return; }
  static const int eighths[5] = {6, 7, 8, 9, 10};
  for (int c = 0; c < 5; ++c) {
    t.cand[c] = std::min(std::max(64, k * eighths[c] / 8), 1 << 20);
    t.ms[c] = 0.0;
    t.n[c] = 0;
  }
  t.launches = 0;
  t.which.clear();
  t.state = hwy_engine::TurnTuner::SAMPLING;
}
static int tuner_finish_stage(hwy_engine *eng) {
  auto &t = eng->tuner;
  HWY_HIP(eng, hipStreamSynchronize(eng->stream));
  for (size_t k = 0; k < t.which.size(); ++k) {
    float ms = 0;
    HWY_HIP(eng, hipEventElapsedTime(&ms, t.events[k].first, t.events[k].second));
    if (k < 5) continue;  // the first round: every candidate's first launch follows another turn's launch pattern
    t.ms[t.which[k]] += ms;
    t.n[t.which[k]]++;
  }
  int best = 2;
  for (int c = 0; c < 5; ++c)
    if (t.n[c] > 0 && t.n[best] > 0 && t.ms[c] / t.n[c] < t.ms[best] / t.n[best]) best = c;
  eng->prio_shift = t.cand[best];
  const bool at_end = (best == 0 && t.cand[0] > 64) || (best == 4 && t.cand[4] < (1 << 20));
  if (at_end && ++t.stage < HWY_TUNE_STAGES) tuner_arm(eng, t.cand[best]);
  else t.state = hwy_engine::TurnTuner::DONE;
  return HWY_OK;
}

extern "C" int hwy_abi_version(void) { return HWY_ABI_VERSION; }
extern "C" size_t hwy_config_size(void) { return sizeof(hwy_config); }
extern "C" int hwy_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}
extern "C" const char *hwy_status_string(int status) {
  switch (status) {
    case HWY_OK: return "ok";
    case HWY_ERR_INVALID_ARG: return "invalid argument";
    case HWY_ERR_HIP: return "HIP runtime error";
    case HWY_ERR_UNSUPPORTED: return "unsupported configuration";
    case HWY_ERR_NO_DEVICE: return "no MI355X / HIP device available (there is no CPU fallback)";
    case HWY_ERR_ACTION: return "action id outside the configured action table";
    default: return "unknown status";
  }
}
extern "C" const char *hwy_last_error(const hwy_engine *eng) {
  return eng ? eng->err.c_str() : g_create_error.c_str();
}

static int validate(const hwy_config *c, std::string &why) {
  char buf[256];
#define BAD(...) do { snprintf(buf, sizeof buf, __VA_ARGS__); why = buf; return HWY_ERR_INVALID_ARG; } while (0)
  if (!c) BAD("config is NULL");
  if (c->abi_version != HWY_ABI_VERSION) BAD("abi_version %d != %d", c->abi_version, HWY_ABI_VERSION);
  if (c->num_envs < 1) BAD("num_envs must be >= 1");
  if (c->num_vehicles < 1 || c->num_vehicles > HWY_MAX_VEHICLES) BAD("num_vehicles must be in [1,%d]", HWY_MAX_VEHICLES);
  if (c->num_agents < 1 || c->num_agents > HWY_MAX_AGENTS || c->num_agents > c->num_vehicles) BAD("num_agents out of range");
  for (int a = 0; a < c->num_agents; ++a)
    if (c->agent_index[a] < 0 || c->agent_index[a] >= c->num_vehicles) BAD("agent_index[%d] out of range", a);
  if (c->lanes_count < 1 || c->lanes_count > HWY_MAX_LANES) BAD("lanes_count must be in [1,%d]", HWY_MAX_LANES);
  if (c->frames_per_step < 0) BAD("frames_per_step must be >= 0");
  if (c->action_set < HWY_ACTIONS_ALL || c->action_set > HWY_ACTIONS_LAT) BAD("action_set must be HWY_ACTIONS_ALL / _LONGI / _LAT");
  if (c->tune_extra_lds < 0 || c->tune_extra_lds > 65536) BAD("tune_extra_lds must be in [0,65536]");
  if (c->tune_ix_prewarm_frames < 0) BAD("tune_ix_prewarm_frames must be >= 0");
  if (c->tune_waves_per_eu < 0 || c->tune_waves_per_eu > 4) BAD("tune_waves_per_eu must be in [0,4]");
  if (c->tune_block_kernel < 0 || c->tune_block_kernel > 2) BAD("tune_block_kernel must be 0 (engine's choice), 1 (workgroup kernel) or 2 (one-wavefront kernels)");
  if (c->tune_prio_shift < -1 || (c->tune_prio_shift > 30 && c->tune_prio_shift < 64) || c->tune_prio_shift > (1 << 20))
    BAD("tune_prio_shift must be -1 (off), 0 (engine's choice), 1..30 (a turn of 2^k clock ticks) or 64..2^20 (a turn of k x 64 ticks)");
  if (c->obs_vehicles < 1 || c->obs_vehicles > c->num_vehicles + 64) BAD("obs_vehicles out of range");
  if (c->obs_type != HWY_OBS_KINEMATICS && c->obs_type != HWY_OBS_OCCUPANCY_GRID && c->obs_type != HWY_OBS_LIDAR) BAD("unknown obs_type");
  if (c->obs_type == HWY_OBS_LIDAR) {
    if (c->scenario != HWY_SCENARIO_HIGHWAY) BAD("the Lidar observation runs on the highway scenario only");
    if (c->lidar_cells < 1 || c->lidar_cells > HWY_MAX_LIDAR_CELLS) BAD("lidar_cells must be in [1,%d]", HWY_MAX_LIDAR_CELLS);
    if (!(c->lidar_max_range > 0) || !(c->lidar_max_range < 1e30)) BAD("lidar_max_range must be positive and finite");
    if (c->lidar_normalize != 0 && c->lidar_normalize != 1) BAD("lidar_normalize must be 0 or 1");
  }
  if (c->obs_type == HWY_OBS_OCCUPANCY_GRID) {
    if (c->grid_shape[0] < 1 || c->grid_shape[1] < 1 || (int64_t)c->grid_shape[0] * c->grid_shape[1] > HWY_MAX_GRID_CELLS)
      BAD("grid_shape must hold 1..%d cells", HWY_MAX_GRID_CELLS);
    if (!(c->grid_step[0] > 0) || !(c->grid_step[1] > 0)) BAD("grid_step must be positive");
  }
  if (c->obs_features < 1 || c->obs_features > HWY_MAX_FEATURES) BAD("obs_features out of range");
  for (int f = 0; f < c->obs_features; ++f)
    if (c->obs_feature_ids[f] < 0 || c->obs_feature_ids[f] >= HWY_FEAT_COUNT ||
        (c->obs_feature_ids[f] == HWY_FEAT_ON_ROAD && c->obs_type != HWY_OBS_OCCUPANCY_GRID)) BAD("unknown feature id");
  if (c->num_target_speeds < 2 || c->num_target_speeds > HWY_MAX_TARGET_SPEEDS) BAD("num_target_speeds must be in [2,%d]", HWY_MAX_TARGET_SPEEDS);
  if (!(c->dt > 0) || !(c->policy_dt > 0)) BAD("dt and policy_dt must be positive");
  if (!(c->lane_width > 0) || !(c->road_length > 0)) BAD("lane_width and road_length must be positive");
  if (c->traffic_model != HWY_TRAFFIC_IDM && c->traffic_model != HWY_TRAFFIC_LINEAR) BAD("unknown traffic_model %d", c->traffic_model);
  if (c->traffic_model == HWY_TRAFFIC_LINEAR) {
    if (c->scenario != HWY_SCENARIO_HIGHWAY) BAD("the Linear traffic family runs on the highway scenario only");
    if (c->traffic_time_wanted != hwy::LinearTraffic::TIME_WANTED) BAD("traffic_time_wanted of the Linear family is 2.5");
    if (!(c->traffic_lc_min_acc_gain >= 0.0 && c->traffic_lc_min_acc_gain < 1e3)) BAD("traffic_lc_min_acc_gain out of range");
  }
  if (c->ego_control != HWY_EGO_META && c->ego_control != HWY_EGO_DIRECT) BAD("unknown ego_control %d", c->ego_control);
  if (c->ego_control == HWY_EGO_DIRECT) {
    if (c->scenario != HWY_SCENARIO_HIGHWAY) BAD("direct ego control runs on the highway scenario only");
    if (c->traffic_model != HWY_TRAFFIC_IDM) BAD("direct ego control runs with IDM traffic only");
    if (c->n_accel < 1 || c->n_accel > HWY_MAX_ACTIONS_PER_AXIS || c->n_steer < 1 || c->n_steer > HWY_MAX_ACTIONS_PER_AXIS)
      BAD("n_accel and n_steer must be in [1,%d]", HWY_MAX_ACTIONS_PER_AXIS);
    for (int k = 0; k < c->n_accel; ++k)
      if (!(std::fabs(c->accel_axis[k]) < 1e6)) BAD("accel_axis[%d] must be finite", k);
    for (int k = 0; k < c->n_steer; ++k)  // (tan_bounded covers +-pi/3, the reference's MAX_STEERING_ANGLE)
      if (!(std::fabs(c->steer_axis[k]) <= HWY_PI / 3.0)) BAD("steer_axis[%d] must be within +-pi/3", k);
  }
  if (c->scenario == HWY_SCENARIO_INTERSECTION) {
    if (c->num_agents > 4) BAD("the intersection scenario holds 1..4 controlled vehicles (one per access road)");
    if (c->num_vehicles < 4 || c->num_vehicles > 64) BAD("the intersection scenario needs 4..64 slots (one wavefront per environment)");
    if (c->gnet_lanes < 1 || c->gnet_lanes > HWY_MAX_GLANES) BAD("gnet_lanes must be in [1,%d]", HWY_MAX_GLANES);
    if (c->destination < -1 || c->destination > 3) BAD("destination must be the k of \"o\" + k, 0..3, or -1 for a random one");
    if (c->initial_vehicle_count < 1) BAD("initial_vehicle_count must be positive");
    for (int k = 0; k < 4; ++k)
      if (c->access_lane[k] < 0 || c->access_lane[k] >= c->gnet_lanes || c->exit_of[k] < 0 || c->exit_of[k] >= c->gnet_lanes)
        BAD("access_lane / exit_of out of range");
    for (int k = 0; k < c->gnet_lanes; ++k) {
      const hwy_glane &l = c->gnet[k];
      if (!(l.length > 0) || !(l.width > 0)) BAD("gnet[%d]: length and width must be positive", k);
      if (l.kind == 1 && !(l.radius > 0)) BAD("gnet[%d]: radius must be positive", k);
      for (int q = 0; q < k; ++q)
        if (c->gnet[q].from_node == l.from_node && c->gnet[q].to_node == l.to_node) BAD("gnet[%d]: every road holds one lane", k);
    }
  } else if (c->scenario != HWY_SCENARIO_HIGHWAY) {
    if (c->scenario != HWY_SCENARIO_MERGE && c->scenario != HWY_SCENARIO_MERGE_GENERIC) BAD("unknown scenario %d", c->scenario);
    if (c->num_vehicles < 3 || c->num_vehicles > 64) BAD("road-network scenarios need 3..64 slots (one wavefront per environment)");
    if (c->net_lanes < 1 || c->net_lanes > HWY_MAX_LANES) BAD("net_lanes must be in [1,%d]", HWY_MAX_LANES);
    if (c->merge_lane >= c->net_lanes) BAD("merge_lane out of range");
    if (c->net_lanes < 3 * c->lanes_count + 3) BAD("merge networks hold 3*lanes_count + 3 lanes");
    for (int a = 0; a < c->num_agents; ++a)
      if (c->agent_index[a] != a) BAD("road-network scenarios keep agent a in slot a");
    for (int k = 0; k < c->net_lanes; ++k) {
      const hwy_lane &l = c->net[k];
      if (!(l.length > 0) || !(l.width > 0)) BAD("net[%d]: length and width must be positive", k);
      if (l.road_first < 0 || l.road_lanes < 1 || l.road_first + l.road_lanes > c->net_lanes || l.id != k - l.road_first ||
          l.id >= l.road_lanes) BAD("net[%d]: inconsistent road_first / road_lanes / id", k);
      if (l.next_first >= 0 && (l.next_lanes < 1 || l.next_first + l.next_lanes > c->net_lanes)) BAD("net[%d]: successor road out of range", k);
    }
  }
#undef BAD
  return HWY_OK;
}

static void fill_params(const hwy_engine *eng, StepParams &p) {
  hwy::params_from_config(eng->cfg, eng->pitch, p);
  hwy::bind_planes(eng->d_f64, (size_t)eng->cfg.num_envs * eng->pitch, p.st);
  p.st.packed = eng->d_packed; p.st.time = eng->d_time; p.st.done = eng->d_done; p.st.episode = eng->d_episode;
  p.autoreset = eng->autoreset;
  p.rp = eng->rp;
  p.grid_ws = eng->d_grid_ws;
  hwy::set_prio_turn(p, eng->prio_shift);
  p.block_env = eng->d_block_env;
  p.counters = eng->d_counters;
}

static bool is_ix(const hwy_engine *eng) { return eng->cfg.scenario == HWY_SCENARIO_INTERSECTION; }
static bool is_linear(const hwy_engine *eng) { return eng->cfg.traffic_model == HWY_TRAFFIC_LINEAR; }
static bool is_direct(const hwy_engine *eng) { return eng->cfg.ego_control == HWY_EGO_DIRECT; }
static bool is_lidar(const hwy_engine *eng) { return eng->cfg.obs_type == HWY_OBS_LIDAR; }
// ids of the configured action table: [0, n)
static int num_action_ids(const hwy_engine *eng) {
  if (is_direct(eng)) return eng->cfg.n_accel * eng->cfg.n_steer;
  return eng->cfg.scenario == HWY_SCENARIO_INTERSECTION ? 3 : HWY_NUM_ACTIONS(eng->cfg.action_set);
}
static bool is_net(const hwy_engine *eng) { return eng->cfg.scenario != HWY_SCENARIO_HIGHWAY && !is_ix(eng); }
static void fill_ix(const hwy_engine *eng, const StepParams &p, hwy::IxParams &ip) {
  hwy::ix_params_from_config(eng->cfg, p, ip);
  ip.lanes = eng->d_gnet;
  ip.route = eng->d_route;
  ip.counters = eng->d_counters;
  ip.road_steps = eng->d_road_steps;
  if (eng->d_shadow_meta) {
    hwy::bind_planes(eng->d_shadow_f64, (size_t)eng->cfg.num_envs * eng->pitch, ip.shadow);
    ip.shadow.packed = eng->d_shadow_packed;
    ip.shadow_route = eng->d_shadow_route;
    ip.shadow_meta = eng->d_shadow_meta;
  }
}
// forget every pre-warmed episode (seeds / episode counters / the state they would follow have changed)
static hipError_t invalidate_shadows(hwy_engine *eng) {
  if (!eng->d_shadow_meta) return hipSuccess;
  return hipMemsetAsync(eng->d_shadow_meta, 0xff, (size_t)eng->cfg.num_envs * 4 * sizeof(int32_t), eng->stream);
}
// THE place that knows the kernel families: builds the parameter struct of the engine's family around p (intersection: IxParams,
// road network: NetParams, Linear traffic: LinearParams, direct ego control: DirectParams, else p itself: IDM with meta-actions) and
// hands it to fn, which calls the overload of hwy_launch.h it wants.
template <typename Fn>
static auto with_family(const hwy_engine *eng, const StepParams &p, Fn &&fn) {
  if (is_ix(eng)) {
    hwy::IxParams ip;
    fill_ix(eng, p, ip);
    return fn(ip);
  }
  if (is_net(eng)) {
    hwy::NetParams np;
    hwy::net_params_from_config(eng->cfg, p, np);
    return fn(np);
  }
  if (is_linear(eng)) return fn(hwy::LinearParams{p, hwy::linear_args(eng->cfg, eng->d_behavior, eng->pitch)});
  if (is_direct(eng)) return fn(hwy::DirectParams{p, hwy::direct_args(eng->cfg, eng->d_controls)});
  return fn(p);
}
// start / stop: the events the launch records its dispatch's begin / end timestamps into (timed_launch)
static hwy::Launch launch_of(const hwy_engine *eng, hipEvent_t start = nullptr, hipEvent_t stop = nullptr) {
  return {eng->cfg.num_envs, eng->stream, eng->waves_per_eu, eng->rollout_waves_per_eu, eng->force_block_kernel, eng->cfg.tune_extra_lds,
          start, stop};
}
// One launch of the engine's family -- its step kernel (p.full_step / p.n_frames as bound by the caller), its reset or its observe
// kernel, with the observation going to p.obs -- and, on a Lidar engine, the trace behind it: the family's kernel runs with a null
// `obs` (the observe kernel has nothing else to do and is not launched), then hwy_lidar.h's kernel observes the state it left.
// RESPAWN (hwy_step_same_step_device): the family's re-spawn kernel for the environments the step launch before it marked done.
enum Stage { STEP, RESET, OBSERVE, RESPAWN };
static hipError_t launch_stage(const hwy_engine *eng, Stage stage, StepParams p, hipEvent_t start = nullptr, hipEvent_t stop = nullptr) {
  float *obs = p.obs;
  if (is_lidar(eng)) p.obs = nullptr;
  const hwy::Launch l = launch_of(eng, start, stop);
  hipError_t e = hipSuccess;
  if (stage == STEP) e = with_family(eng, p, [&](const auto &a) { return hwy::launch_step(a, l); });
  else if (stage == RESET) e = with_family(eng, p, [&](const auto &a) { return hwy::launch_reset(a, l); });
  else if (stage == RESPAWN) e = with_family(eng, p, [&](const auto &a) { return hwy::launch_respawn(a, l); });
  else if (!is_lidar(eng)) e = with_family(eng, p, [&](const auto &a) { return hwy::launch_observe(a, l); });
  if (e != hipSuccess || !is_lidar(eng) || !obs) return e;
  const size_t plane = (size_t)eng->cfg.num_envs * eng->pitch;
  const double *f = eng->d_f64;
  const hwy::LidarParams lp = hwy::lidar_params(eng->cfg, f, f + plane, f + 2 * plane, f + 3 * plane, eng->d_packed, eng->pitch, obs);
  return hwy::launch_lidar(lp, eng->cfg.lidar_normalize != 0, eng->cfg.num_envs * eng->cfg.num_agents, eng->stream);
}

// rows of the per-agent planes (actions, reward, info) of one policy step, and floats of its observation
static size_t num_agent_rows(const hwy_config &c) { return (size_t)c.num_envs * c.num_agents; }
static size_t num_obs_floats(const hwy_config &c) { return num_agent_rows(c) * hwy::obs_len(c); }

template <typename T>
static hipError_t alloc_zeroed(T *&ptr, size_t bytes, hipStream_t stream) {
  const hipError_t e = hipMalloc((void **)&ptr, bytes);
  return e != hipSuccess ? e : hipMemsetAsync(ptr, 0, bytes, stream);
}

extern "C" int hwy_create(const hwy_config *cfg, int device, void *stream, hwy_engine **out) {
  if (!out) return fail(nullptr, HWY_ERR_INVALID_ARG, "out is NULL");
  *out = nullptr;
  std::string why;
  if (int rc = validate(cfg, why)) return fail(nullptr, rc, why);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
    return fail(nullptr, HWY_ERR_NO_DEVICE, "no HIP device visible: the engine has no CPU fallback");
  if (device < 0 || device >= ndev) return fail(nullptr, HWY_ERR_INVALID_ARG, "device index out of range");
  hwy_engine *eng = new (std::nothrow) hwy_engine();
  if (!eng) return fail(nullptr, HWY_ERR_HIP, "out of host memory");
  eng->cfg = *cfg;
  eng->device = device;
  eng->pitch = (cfg->num_vehicles + 7) & ~7;  // 64-byte aligned rows of f64
  eng->force_block_kernel = hwy::force_block_kernel(*cfg);  // hwy_config.tune_block_kernel resolved (hwy_params.h)
  // road-network kernel: 128 VGPRs, 4 waves/SIMD, no spills.
  // intersection kernel with helper lanes (N <= 32, hwy_ix.h): 150 VGPRs, but 20.2 KB of LDS per one-wavefront workgroup keep it
  // at 2 per SIMD.  Without them (N > 32, or tune_ix_no_helpers): 128 VGPRs / 16.7 KB (2048 x 30: 371.9 us against 285.1)
  if (cfg->scenario == HWY_SCENARIO_INTERSECTION) {
    const bool helpers = cfg->num_vehicles <= 32 && !cfg->tune_ix_no_helpers;
    eng->waves_per_eu = (cfg->num_envs > 2048 && !helpers) ? 3 : 2;
  }
  else if (cfg->scenario != HWY_SCENARIO_HIGHWAY) eng->waves_per_eu = 4;
  else {
    // highway scenario.  One-wavefront kernels (N <= 64; 99 VGPRs ego-only, 113 full-pairwise: every allocation variant gets the
    // same registers since the build stopped hoisting literals, build.py; that every variant of every kernel COMPUTES the same,
    // the spilling 4-wave workgroup builds included, is tests/test_kernel_variants.py, bit for bit on the device).
    // Workgroup kernel (N > 64, ceil(N / 64) wavefronts per environment): 146 .. 154 VGPRs at 3 waves/SIMD, 128 with 18 .. 30
    // spilled at 4 -- the 4-wave build pays as soon as the grid no longer fits 3 resident wavefronts per SIMD (1024 x 101:
    // 159.2 / 164.4 us; 2048 x 101: 273.2 / 209.6 us)
    hipDeviceProp_t prop;
    const int simds = (hipGetDeviceProperties(&prop, device) == hipSuccess ? prop.multiProcessorCount : 256) * 4;
    const long long waves = (long long)cfg->num_envs * ((cfg->num_vehicles + 63) / 64);
    eng->waves_per_eu = waves > 3LL * simds ? 4 : 3;
    // (64 < N <= 128 with the Kinematics observation runs the wide kernel, hwy_wave2.h: ONE build, <2, 2> -- 245 VGPRs, two
    //  resident wavefronts per SIMD --, which this variable and hwy_config.tune_waves_per_eu do not select among)
  }
  if (cfg->tune_waves_per_eu >= 1 && cfg->tune_waves_per_eu <= 4) eng->waves_per_eu = cfg->tune_waves_per_eu;
  eng->rollout_waves_per_eu = eng->waves_per_eu;
  auto bail = [&](hipError_t e, const char *what) {
    g_create_error = std::string(what) + ": " + hipGetErrorString(e);
    hwy_destroy(eng);
    return HWY_ERR_HIP;
  };
  hipError_t e;
  if ((e = hipSetDevice(device)) != hipSuccess) return bail(e, "hipSetDevice");
  if (stream) {
    eng->stream = (hipStream_t)stream;
  } else {
    if ((e = hipStreamCreateWithFlags(&eng->stream, hipStreamNonBlocking)) != hipSuccess) return bail(e, "hipStreamCreate");
    eng->own_stream = true;
  }
  const size_t E = cfg->num_envs, plane = E * eng->pitch;
  const size_t n_act = num_agent_rows(*cfg), n_obs = num_obs_floats(*cfg);
  // ALLOC: device memory; ALLOC0: ... zeroed (on the engine's stream: synchronised below)
#define ALLOC(ptr, bytes) if ((e = hipMalloc((void **)&(ptr), (bytes))) != hipSuccess) return bail(e, "hipMalloc " #ptr)
#define ALLOC0(ptr, bytes) if ((e = alloc_zeroed((ptr), (bytes), eng->stream)) != hipSuccess) return bail(e, "hipMalloc / hipMemset " #ptr)
  if (cfg->traffic_model == HWY_TRAFFIC_LINEAR) ALLOC0(eng->d_behavior, plane * HWY_BEHAVIOR_PARAMS * sizeof(double));
  if (cfg->ego_control == HWY_EGO_DIRECT) ALLOC0(eng->d_controls, 2 * n_act * sizeof(double));
  if (cfg->scenario == HWY_SCENARIO_INTERSECTION) {
    ALLOC0(eng->d_route, plane * sizeof(long long));
    ALLOC0(eng->d_road_steps, E * sizeof(int32_t));
    ALLOC(eng->d_gnet, sizeof(hwy_glane) * HWY_MAX_GLANES);
    if ((e = hipMemcpy(eng->d_gnet, cfg->gnet, sizeof(hwy_glane) * HWY_MAX_GLANES, hipMemcpyHostToDevice)) != hipSuccess) return bail(e, "hipMemcpy");
    if (!(cfg->flags & HWY_C_HOST_TRAFFIC) && !cfg->tune_ix_no_prewarm) {  // (tuning: every auto-reset runs its warm-up inline)
      ALLOC0(eng->d_shadow_f64, plane * 9 * sizeof(double));
      ALLOC(eng->d_shadow_packed, plane * sizeof(int32_t));
      ALLOC(eng->d_shadow_route, plane * sizeof(long long));
      ALLOC(eng->d_shadow_meta, E * 4 * sizeof(int32_t));
      if ((e = invalidate_shadows(eng)) != hipSuccess) return bail(e, "hipMemset");
    }
  }
  ALLOC0(eng->d_counters, HWY_CTR_COUNT * sizeof(unsigned long long));
  ALLOC0(eng->d_f64, plane * 9 * sizeof(double));
  ALLOC0(eng->d_packed, plane * sizeof(int32_t));
  ALLOC0(eng->d_time, E * sizeof(double));
  ALLOC0(eng->d_done, E);
  ALLOC0(eng->d_episode, E * sizeof(uint32_t));
  ALLOC(eng->d_actions, n_act * sizeof(int32_t));
  {
    auto up = [](size_t v) { return (v + 63) & ~(size_t)63; };
    size_t off = 0;
    eng->off_reward = off;  off = up(off + n_act * sizeof(double));
    eng->off_speed = off;   off = up(off + n_act * sizeof(double));
    eng->off_obs = off;     off = up(off + n_obs * sizeof(float));
    eng->off_term = off;    off = up(off + E);
    eng->off_trunc = off;   off = up(off + E);
    eng->off_crashed = off; off = up(off + n_act);
    eng->out_bytes = off;
  }
  ALLOC(eng->d_out, eng->out_bytes);
  eng->d_reward = (double *)(eng->d_out + eng->off_reward);
  eng->d_info_speed = (double *)(eng->d_out + eng->off_speed);
  eng->d_obs = (float *)(eng->d_out + eng->off_obs);
  eng->d_term = (uint8_t *)(eng->d_out + eng->off_term);
  eng->d_trunc = (uint8_t *)(eng->d_out + eng->off_trunc);
  eng->d_info_crashed = (uint8_t *)(eng->d_out + eng->off_crashed);
  ALLOC(eng->d_mask, E);
  ALLOC(eng->d_seeds, E * sizeof(uint64_t));
  if (cfg->obs_type == HWY_OBS_OCCUPANCY_GRID) ALLOC(eng->d_grid_ws, hwy::grid_ws_len(*cfg) * sizeof(int32_t));
#undef ALLOC0
#undef ALLOC
  // pinned staging: the largest of {state SoA, step I/O}
  const size_t state_bytes = plane * (9 * sizeof(double) + sizeof(int32_t) + sizeof(long long)) + E * (sizeof(double) + sizeof(int32_t));
  const size_t io_bytes = eng->out_bytes + n_act * 4 + E * 9 + 64;
  eng->h_pinned_bytes = state_bytes > io_bytes ? state_bytes : io_bytes;
  if ((e = hipHostMalloc(&eng->h_pinned, eng->h_pinned_bytes, hipHostMallocDefault)) != hipSuccess) return bail(e, "hipHostMalloc");
  if ((e = hipStreamSynchronize(eng->stream)) != hipSuccess) return bail(e, "hipStreamSynchronize");
  eng->rp = hwy::default_reset_params(*cfg);
  // issue-priority turns: on by default only where the whole grid of the step kernel is resident at once
  if (cfg->tune_prio_shift > 0) eng->prio_shift = cfg->tune_prio_shift;
  else if (cfg->tune_prio_shift == 0) {
    StepParams probe;
    hwy::params_from_config(*cfg, eng->pitch, probe);
    const int resident = with_family(eng, probe, [&](const auto &a) { return hwy::step_resident_blocks(a, launch_of(eng)); });
    // the turn that pays is about a sixth of a wavefront's lifetime, i.e. it grows with the frames of a policy step: 2^14 ticks
    // for the 5 frames of highway-fast-v0 (13: 47.0 us, 14: 44.96, 15: 47.7), 2^16 for the 15 frames of highway-v0 (14: 134.3
    // us, 15 / 16: 133.3) and of the merge scenarios (config 5: 14: 313.8, 16 / 17: 296.0, 18: 314.8; merge-v0: 14: 178.2,
    // 15 / 16: 172.7, 17: 182.1) and of the workgroup kernel, whose wavefronts take turns by workgroup (config-3 shard 1024 x 101:
    // off 161.1, 16: 159.4; 2048 x 101: 214.8 / 207.6) -- profiles/r03_history.md
    int shift = HWY_DEFAULT_PRIO_SHIFT;
    for (int f = 7; f <= cfg->frames_per_step && shift < 18; f *= 2) ++shift;  // +1 from 7 frames on, +2 from 14 on, ...
    // Round 5: the optimum is sharp and does not sit on a power of two (turns of k x 64 ticks, tune_prio_shift >= 64; all on the final
    // build, tools/r05_call16.sh .. 18.sh).  One-wavefront highway kernel: 5 frames 224 .. 256 (x 64 ticks: 40.4 us; 192: 40.9,
    // 288: 40.9, 2^15: 42.9); 15 frames 768 (107.5 us; 384: 107.7, 512: 109.6, 2^16: 111.3) -- a turn of 51 x 64 ticks per frame.
    // merge-generic (config 5): 832 (222.5 us; 768: 223.0, 2^16: 226.2); merge-v0 keeps 2^16 (149.3 us; 768 .. 960: 150 .. 152).
    int turn = shift;
    if (cfg->scenario == HWY_SCENARIO_HIGHWAY && cfg->num_vehicles <= 64 && !eng->force_block_kernel)
      turn = std::max(64, 256 * cfg->frames_per_step / 5);
    else if (cfg->scenario == HWY_SCENARIO_MERGE_GENERIC)
      turn = std::max(64, 832 * cfg->frames_per_step / 15);
    if (turn >= 64) turn = std::min(turn, 1 << 20);  // (the validated range of the linear encoding, whatever frames_per_step is)
    eng->prio_shift = (resident > 0 && cfg->num_envs <= resident) ? turn : 0;
    // The optimum is sharp and depends on (envs, vehicles, frames) -- profiles/r05_history.md section 10: up to 7 % between neighbours --
    // and the defaults above were swept on BASELINE's shapes only: the engine refines its own choice on its first launches
    // (tuner_*: below).  An explicit tune_prio_shift (> 0, or -1 = off) is never touched.
    if (eng->prio_shift > 0) tuner_arm(eng, eng->prio_shift);
  }
  *out = eng;
  return HWY_OK;
}

extern "C" int hwy_destroy(hwy_engine *eng) {
  if (!eng) return HWY_OK;
  (void)hipSetDevice(eng->device);
  if (eng->stream) (void)hipStreamSynchronize(eng->stream);
  if (eng->comm) { hwy::comm_destroy(eng->comm); eng->comm = nullptr; }
  for (auto &pr : eng->events) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
  for (auto &pr : eng->tuner.events) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
  void *ptrs[] = {eng->d_f64, eng->d_packed, eng->d_time, eng->d_done, eng->d_episode, eng->d_actions, eng->d_out, eng->d_roll,
                  eng->d_mask, eng->d_seeds, eng->d_grid_ws, eng->d_route, eng->d_road_steps, eng->d_gnet,
                  eng->d_shadow_f64, eng->d_shadow_packed, eng->d_shadow_route, eng->d_shadow_meta, eng->d_counters, eng->d_block_env,
                  eng->d_behavior, eng->d_controls, eng->d_ttc_grid, eng->d_plan_action, eng->d_plan_q, eng->d_fork_src, eng->d_opd, eng->d_cem, eng->d_action_mask,
                  eng->d_door_step_obs, eng->d_ttc_obs, eng->d_lidar_door_obs};
  for (void *q : ptrs) if (q) (void)hipFree(q);
  if (eng->fork_event) (void)hipEventDestroy(eng->fork_event);
  if (eng->h_pinned) (void)hipHostFree(eng->h_pinned);
  if (eng->own_stream && eng->stream) (void)hipStreamDestroy(eng->stream);
  delete eng;
  return HWY_OK;
}

// ---- state injection / inspection -----------------------------------------------------------------
static void pack_rows(const hwy_engine *eng, const double *src, double *dst) {  // [E][N] -> [E][pitch]
  const int E = eng->cfg.num_envs, N = eng->cfg.num_vehicles, P = eng->pitch;
  for (int e = 0; e < E; ++e) {
    std::memcpy(dst + (size_t)e * P, src + (size_t)e * N, sizeof(double) * N);
    for (int i = N; i < P; ++i) dst[(size_t)e * P + i] = 0.0;
  }
}
static void unpack_rows(const hwy_engine *eng, const double *src, double *dst) {  // [E][pitch] -> [E][N]
  const int E = eng->cfg.num_envs, N = eng->cfg.num_vehicles, P = eng->pitch;
  for (int e = 0; e < E; ++e) std::memcpy(dst + (size_t)e * N, src + (size_t)e * P, sizeof(double) * N);
}

extern "C" int hwy_set_state(hwy_engine *eng, const hwy_state *h) {
  if (!eng || !h) return HWY_ERR_INVALID_ARG;
  const double *fields[9] = {h->x, h->y, h->heading, h->speed, h->timer, h->target_speed, h->delta, h->impact_x, h->impact_y};
  for (auto f : fields) if (!f) return fail(eng, HWY_ERR_INVALID_ARG, "hwy_set_state: NULL field");
  if (!h->lane || !h->target_lane || !h->speed_index || !h->flags || !h->time)
    return fail(eng, HWY_ERR_INVALID_ARG, "hwy_set_state: NULL field");
  HWY_HIP(eng, hipSetDevice(eng->device));
  const int E = eng->cfg.num_envs, N = eng->cfg.num_vehicles, P = eng->pitch;
  const size_t plane = (size_t)E * P;
  const int n_lane_ids = is_ix(eng) ? eng->cfg.gnet_lanes : is_net(eng) ? eng->cfg.net_lanes : eng->cfg.lanes_count;
  if (is_ix(eng) && (!h->route || !h->road_steps)) return fail(eng, HWY_ERR_INVALID_ARG, "hwy_set_state: route / road_steps are required by the intersection scenario");
  for (size_t k = 0; k < (size_t)E * N; ++k) {
    if (h->lane[k] < 0 || h->lane[k] >= n_lane_ids || h->target_lane[k] < 0 || h->target_lane[k] >= n_lane_ids)
      return fail(eng, HWY_ERR_INVALID_ARG, "hwy_set_state: lane index out of range");
    if (h->speed_index[k] < 0 || h->speed_index[k] >= eng->cfg.num_target_speeds)
      return fail(eng, HWY_ERR_INVALID_ARG, "hwy_set_state: speed_index out of range");
  }
  double *stage = (double *)eng->h_pinned;
  for (int f = 0; f < 9; ++f) pack_rows(eng, fields[f], stage + f * plane);
  int32_t *pk = (int32_t *)(stage + 9 * plane);
  for (int e = 0; e < E; ++e)
    for (int i = 0; i < P; ++i) {
      const size_t k = (size_t)e * N + i;
      if (is_ix(eng)) pk[(size_t)e * P + i] = i < N ? hwy::ix_pack_word(h->lane[k], h->target_lane[k], h->speed_index[k], h->flags[k])
                                                    : hwy::ix_pack_word(0, 0, 0, HWY_F_ABSENT);
      else pk[(size_t)e * P + i] = i < N ? hwy::pack_word(h->lane[k], h->target_lane[k], h->speed_index[k], h->flags[k], i) : 0;
    }
  double *tm = (double *)(pk + plane);
  std::memcpy(tm, h->time, sizeof(double) * E);
  if (is_ix(eng)) {
    long long *rt = (long long *)(tm + E);
    int32_t *rs = (int32_t *)(rt + plane);
    for (int e = 0; e < E; ++e)
      for (int i = 0; i < P; ++i) rt[(size_t)e * P + i] = i < N ? (long long)h->route[(size_t)e * N + i] : 0;
    std::memcpy(rs, h->road_steps, sizeof(int32_t) * E);
    HWY_HIP(eng, hipMemcpyAsync(eng->d_route, rt, plane * sizeof(long long), hipMemcpyHostToDevice, eng->stream));
    HWY_HIP(eng, hipMemcpyAsync(eng->d_road_steps, rs, E * sizeof(int32_t), hipMemcpyHostToDevice, eng->stream));
  }
  HWY_HIP(eng, hipMemcpyAsync(eng->d_f64, stage, plane * 9 * sizeof(double), hipMemcpyHostToDevice, eng->stream));
  HWY_HIP(eng, hipMemcpyAsync(eng->d_packed, pk, plane * sizeof(int32_t), hipMemcpyHostToDevice, eng->stream));
  HWY_HIP(eng, hipMemcpyAsync(eng->d_time, tm, E * sizeof(double), hipMemcpyHostToDevice, eng->stream));
  HWY_HIP(eng, hipMemsetAsync(eng->d_done, 0, E, eng->stream));
  HWY_HIP(eng, hipStreamSynchronize(eng->stream));
  eng->has_state = true;
  return HWY_OK;
}

extern "C" int hwy_get_state(hwy_engine *eng, hwy_state *h) {
  if (!eng || !h) return HWY_ERR_INVALID_ARG;
  HWY_HIP(eng, hipSetDevice(eng->device));
  const int E = eng->cfg.num_envs, N = eng->cfg.num_vehicles, P = eng->pitch;
  const size_t plane = (size_t)E * P;
  double *stage = (double *)eng->h_pinned;
  int32_t *pk = (int32_t *)(stage + 9 * plane);
  double *tm = (double *)(pk + plane);
  HWY_HIP(eng, hipMemcpyAsync(stage, eng->d_f64, plane * 9 * sizeof(double), hipMemcpyDeviceToHost, eng->stream));
  HWY_HIP(eng, hipMemcpyAsync(pk, eng->d_packed, plane * sizeof(int32_t), hipMemcpyDeviceToHost, eng->stream));
  HWY_HIP(eng, hipMemcpyAsync(tm, eng->d_time, E * sizeof(double), hipMemcpyDeviceToHost, eng->stream));
  long long *rt = (long long *)(tm + E);
  int32_t *rs = (int32_t *)(rt + plane);
  if (is_ix(eng)) {
    HWY_HIP(eng, hipMemcpyAsync(rt, eng->d_route, plane * sizeof(long long), hipMemcpyDeviceToHost, eng->stream));
    HWY_HIP(eng, hipMemcpyAsync(rs, eng->d_road_steps, E * sizeof(int32_t), hipMemcpyDeviceToHost, eng->stream));
  }
  HWY_HIP(eng, hipStreamSynchronize(eng->stream));
  double *fields[9] = {h->x, h->y, h->heading, h->speed, h->timer, h->target_speed, h->delta, h->impact_x, h->impact_y};
  for (int f = 0; f < 9; ++f) if (fields[f]) unpack_rows(eng, stage + f * plane, fields[f]);
  // one path for both packed-word layouts (hwy_device.h, hwy_ix.h)
  auto unpack = [&](auto lane_of, auto target_of, auto speed_index_of, auto flags_of) {
    for (int e = 0; e < E; ++e)
      for (int i = 0; i < N; ++i) {
        const int32_t w = pk[(size_t)e * P + i];
        const size_t k = (size_t)e * N + i;
        const int fl = flags_of(w);
        if (h->lane) h->lane[k] = lane_of(w);
        if (h->target_lane) h->target_lane[k] = target_of(w);
        if (h->speed_index) h->speed_index[k] = speed_index_of(w);
        if (h->flags) h->flags[k] = fl;
        if (is_ix(eng) && h->route) h->route[k] = (int64_t)rt[(size_t)e * P + i];
        // the step kernel maintains nothing but the flag word of an empty slot (intersection scenario), and the impact pair only
        // while its flag is set (Vehicle.impact is None otherwise)
        if (is_ix(eng) && (fl & HWY_F_ABSENT)) {
          for (int f = 0; f < 9; ++f) if (fields[f]) fields[f][k] = 0.0;
          if (h->lane) h->lane[k] = 0;
          if (h->target_lane) h->target_lane[k] = 0;
          if (h->speed_index) h->speed_index[k] = 0;
          if (h->flags) h->flags[k] = HWY_F_ABSENT;
          if (h->route) h->route[k] = 0;
        } else if (!(fl & HWY_F_HAS_IMPACT)) {
          if (h->impact_x) h->impact_x[k] = 0.0;
          if (h->impact_y) h->impact_y[k] = 0.0;
        }
      }
  };
  if (is_ix(eng)) {
    unpack(hwy::ix_word_lane, hwy::ix_word_target, hwy::ix_word_speed_index, hwy::ix_word_flags);
    if (h->road_steps) std::memcpy(h->road_steps, rs, sizeof(int32_t) * E);
  } else {
    unpack(hwy::word_lane, hwy::word_target, hwy::word_speed_index, hwy::word_flags);
  }
  if (h->time) std::memcpy(h->time, tm, sizeof(double) * E);
  return HWY_OK;
}

// ---- per-vehicle behaviour parameters (HWY_TRAFFIC_LINEAR) ----------------------------------------------
// host [E][N][HWY_BEHAVIOR_PARAMS] <-> device planes [k][E][pitch]
extern "C" int hwy_set_behavior(hwy_engine *eng, const double *params) {
  if (!eng || !params) return HWY_ERR_INVALID_ARG;
  if (!is_linear(eng)) return fail(eng, HWY_ERR_INVALID_ARG, "hwy_set_behavior: the engine's traffic model has no per-vehicle parameters");
  HWY_HIP(eng, hipSetDevice(eng->device));
  const int E = eng->cfg.num_envs, N = eng->cfg.num_vehicles, P = eng->pitch;
  const size_t plane = (size_t)E * P;
  std::vector<double> h(plane * HWY_BEHAVIOR_PARAMS, 0.0);
  for (int e = 0; e < E; ++e)
    for (int i = 0; i < N; ++i)
      for (int q = 0; q < HWY_BEHAVIOR_PARAMS; ++q) h[q * plane + (size_t)e * P + i] = params[((size_t)e * N + i) * HWY_BEHAVIOR_PARAMS + q];
  HWY_HIP(eng, hipMemcpyAsync(eng->d_behavior, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, eng->stream));
  HWY_HIP(eng, hipStreamSynchronize(eng->stream));
  return HWY_OK;
}
extern "C" int hwy_get_behavior(hwy_engine *eng, double *params) {
  if (!eng || !params) return HWY_ERR_INVALID_ARG;
  if (!is_linear(eng)) return fail(eng, HWY_ERR_INVALID_ARG, "hwy_get_behavior: the engine's traffic model has no per-vehicle parameters");
  HWY_HIP(eng, hipSetDevice(eng->device));
  const int E = eng->cfg.num_envs, N = eng->cfg.num_vehicles, P = eng->pitch;
  const size_t plane = (size_t)E * P;
  std::vector<double> h(plane * HWY_BEHAVIOR_PARAMS);
  HWY_HIP(eng, hipMemcpyAsync(h.data(), eng->d_behavior, h.size() * sizeof(double), hipMemcpyDeviceToHost, eng->stream));
  HWY_HIP(eng, hipStreamSynchronize(eng->stream));
  for (int e = 0; e < E; ++e)
    for (int i = 0; i < N; ++i)
      for (int q = 0; q < HWY_BEHAVIOR_PARAMS; ++q) params[((size_t)e * N + i) * HWY_BEHAVIOR_PARAMS + q] = h[q * plane + (size_t)e * P + i];
  return HWY_OK;
}

// ---- stored controls of the agents (HWY_EGO_DIRECT) ---------------------------------------------------------
extern "C" int hwy_set_controls(hwy_engine *eng, const double *acceleration, const double *steering) {
  if (!eng || !acceleration || !steering) return HWY_ERR_INVALID_ARG;
  if (!is_direct(eng)) return fail(eng, HWY_ERR_INVALID_ARG, "hwy_set_controls: the engine's controlled vehicles store no controls (ego_control is HWY_EGO_META)");
  const size_t n = (size_t)eng->cfg.num_envs * eng->cfg.num_agents;
  for (size_t k = 0; k < n; ++k)
    if (!(std::fabs(steering[k]) <= HWY_PI / 3.0)) return fail(eng, HWY_ERR_INVALID_ARG, "hwy_set_controls: steering must be within +-pi/3");
  HWY_HIP(eng, hipSetDevice(eng->device));
  std::vector<double> h(2 * n);
  std::memcpy(h.data(), acceleration, n * sizeof(double));
  std::memcpy(h.data() + n, steering, n * sizeof(double));
  HWY_HIP(eng, hipMemcpyAsync(eng->d_controls, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, eng->stream));
  HWY_HIP(eng, hipStreamSynchronize(eng->stream));
  return HWY_OK;
}
extern "C" int hwy_get_controls(hwy_engine *eng, double *acceleration, double *steering) {
  if (!eng || !acceleration || !steering) return HWY_ERR_INVALID_ARG;
  if (!is_direct(eng)) return fail(eng, HWY_ERR_INVALID_ARG, "hwy_get_controls: the engine's controlled vehicles store no controls (ego_control is HWY_EGO_META)");
  const size_t n = (size_t)eng->cfg.num_envs * eng->cfg.num_agents;
  HWY_HIP(eng, hipSetDevice(eng->device));
  std::vector<double> h(2 * n);
  HWY_HIP(eng, hipMemcpyAsync(h.data(), eng->d_controls, h.size() * sizeof(double), hipMemcpyDeviceToHost, eng->stream));
  HWY_HIP(eng, hipStreamSynchronize(eng->stream));
  std::memcpy(acceleration, h.data(), n * sizeof(double));
  std::memcpy(steering, h.data() + n, n * sizeof(double));
  return HWY_OK;
}

// ---- kernel timing ----------------------------------------------------------------------------------
// pair k of a pool of launch events, created on first use
static int event_pair(hwy_engine *eng, std::vector<std::pair<hipEvent_t, hipEvent_t>> &pool, size_t k, std::pair<hipEvent_t, hipEvent_t> &out) {
  while (pool.size() <= k) {
    hipEvent_t a, b;
    HWY_HIP(eng, hipEventCreate(&a));
    HWY_HIP(eng, hipEventCreate(&b));
    pool.emplace_back(a, b);
  }
  out = pool[k];
  return HWY_OK;
}
// the step launch of the engine's family (launch_stage), timed by the turn tuner or by hwy_profile_* when either wants it
static int timed_launch(hwy_engine *eng, const StepParams &p) {
  auto &tn = eng->tuner;
  std::pair<hipEvent_t, hipEvent_t> ev;
  if (tn.state == hwy_engine::TurnTuner::SAMPLING && !eng->profiling && p.full_step) {
    const int c = tn.launches % 5;
    if (int rc = event_pair(eng, tn.events, (size_t)tn.launches, ev)) return rc;
    StepParams q = p;
    hwy::set_prio_turn(q, tn.cand[c]);
    HWY_HIP(eng, launch_stage(eng, STEP, q, ev.first, ev.second));
    tn.which.push_back(c);
    if (++tn.launches == 5 * (HWY_TUNE_ROUNDS + 1)) return tuner_finish_stage(eng);
    return HWY_OK;
  }
  if (!eng->profiling || (eng->launch_counter++ % eng->profiling) != 0) {
    HWY_HIP(eng, launch_stage(eng, STEP, p));
    return HWY_OK;
  }
  if (int rc = event_pair(eng, eng->events, eng->events_used, ev)) return rc;
  eng->events_used++;
  HWY_HIP(eng, launch_stage(eng, STEP, p, ev.first, ev.second));  // the dispatch's own begin / end timestamps (hwy_launch.h)
  return HWY_OK;
}
static int drain_events(hwy_engine *eng) {
  HWY_HIP(eng, hipStreamSynchronize(eng->stream));
  for (size_t k = 0; k < eng->events_used; ++k) {
    float ms = 0;
    HWY_HIP(eng, hipEventElapsedTime(&ms, eng->events[k].first, eng->events[k].second));
    eng->prof_ms += ms;
    eng->prof_launches++;
  }
  eng->events_used = 0;
  return HWY_OK;
}
extern "C" int hwy_get_prio_turn(hwy_engine *eng, int32_t *turn, int32_t *state) {
  if (!eng) return HWY_ERR_INVALID_ARG;
  if (turn) *turn = eng->prio_shift;
  if (state) *state = eng->tuner.state;
  return HWY_OK;
}
extern "C" int hwy_profile_enable(hwy_engine *eng, int32_t enabled) {
  if (!eng) return HWY_ERR_INVALID_ARG;
  HWY_HIP(eng, hipSetDevice(eng->device));
  if (int rc = drain_events(eng)) return rc;
  eng->profiling = enabled > 0 ? enabled : 0;
  eng->launch_counter = 0;
  if (enabled) { eng->prof_ms = 0.0; eng->prof_launches = 0; }
  return HWY_OK;
}
extern "C" int hwy_profile_read(hwy_engine *eng, double *total_ms, int64_t *launches) {
  if (!eng) return HWY_ERR_INVALID_ARG;
  HWY_HIP(eng, hipSetDevice(eng->device));
  if (int rc = drain_events(eng)) return rc;
  if (total_ms) *total_ms = eng->prof_ms;
  if (launches) *launches = eng->prof_launches;
  return HWY_OK;
}

// ---- stepping ------------------------------------------------------------------------------------------
// the arguments of a full policy step around the caller's I/O planes
static void bind_full_step(const hwy_engine *eng, StepParams &p, const int32_t *d_actions, float *d_obs, double *d_reward,
                           uint8_t *d_terminated, uint8_t *d_truncated, double *d_info_speed, uint8_t *d_info_crashed) {
  fill_params(eng, p);
  p.n_frames = eng->cfg.frames_per_step;
  p.full_step = 1;
  p.actions = d_actions; p.obs = d_obs; p.reward = d_reward; p.terminated = d_terminated; p.truncated = d_truncated;
  p.info_speed = d_info_speed; p.info_crashed = d_info_crashed;
}
// The one full-step launch behind hwy_step_device and hwy_step_continuous_device: the family's step kernel around the caller's
// planes, timed when the tuner or hwy_profile_* wants it.  d_actions: the action ids, or NULL -- the direct kernels then drive on
// with the stored controls (the continuous door wrote them just before on this stream).  The device is set, the planes are checked.
static int enqueue_full_step(hwy_engine *eng, const int32_t *d_actions, float *d_obs, double *d_reward, uint8_t *d_terminated,
                             uint8_t *d_truncated, double *d_info_speed, uint8_t *d_info_crashed) {
  StepParams p;
  bind_full_step(eng, p, d_actions, d_obs, d_reward, d_terminated, d_truncated, d_info_speed, d_info_crashed);
  if (eng->profiling && eng->events_used >= 65536)
    if (int rc = drain_events(eng)) return rc;
  return timed_launch(eng, p);
}

extern "C" int hwy_step_device(hwy_engine *eng, const int32_t *d_actions, float *d_obs, double *d_reward,
                               uint8_t *d_terminated, uint8_t *d_truncated, double *d_info_speed,
                               uint8_t *d_info_crashed) {
  if (!eng) return HWY_ERR_INVALID_ARG;
  if (!d_actions || !d_obs || !d_reward || !d_terminated || !d_truncated)
    return fail(eng, HWY_ERR_INVALID_ARG, "hwy_step_device: actions/obs/reward/terminated/truncated must be non-NULL");
  HWY_HIP(eng, hipSetDevice(eng->device));
  return enqueue_full_step(eng, d_actions, d_obs, d_reward, d_terminated, d_truncated, d_info_speed, d_info_crashed);
}

extern "C" int hwy_rollout_device(hwy_engine *eng, int32_t k_steps, const int32_t *d_actions, float *d_obs, double *d_reward,
                                  uint8_t *d_terminated, uint8_t *d_truncated, double *d_info_speed, uint8_t *d_info_crashed) {
  if (!eng) return HWY_ERR_INVALID_ARG;
  if (k_steps < 1) return fail(eng, HWY_ERR_INVALID_ARG, "hwy_rollout_device: k_steps must be >= 1");
  if (!d_actions || !d_obs || !d_reward || !d_terminated || !d_truncated)
    return fail(eng, HWY_ERR_INVALID_ARG, "hwy_rollout_device: actions/obs/reward/terminated/truncated must be non-NULL");
  if (k_steps > 1 && is_ix(eng) && (eng->cfg.flags & HWY_C_HOST_TRAFFIC))  // the host clears / spawns BETWEEN policy steps
    return fail(eng, HWY_ERR_INVALID_ARG, "hwy_rollout_device: k_steps > 1 needs device traffic (HWY_C_HOST_TRAFFIC is set: "
                                          "_clear_vehicles / _spawn_vehicle run on the host between steps)");
  HWY_HIP(eng, hipSetDevice(eng->device));
  StepParams p;
  if (is_lidar(eng)) {
    // k_steps x (step launch + lidar launch): step k's observation is of the state after step k, so the steps cannot share a launch.
    // The launches are those of k_steps hwy_step_device calls on block k of every plane (untimed): the same results by construction.
    const size_t E = eng->cfg.num_envs, EA = num_agent_rows(eng->cfg), n_obs = num_obs_floats(eng->cfg);
    for (int k = 0; k < k_steps; ++k) {
      bind_full_step(eng, p, d_actions + k * EA, d_obs + k * n_obs, d_reward + k * EA, d_terminated + k * E, d_truncated + k * E,
                     d_info_speed ? d_info_speed + k * EA : nullptr, d_info_crashed ? d_info_crashed + k * EA : nullptr);
      HWY_HIP(eng, launch_stage(eng, STEP, p));
    }
    return HWY_OK;
  }
  // K steps in ONE launch, every family.  The intersection kernel: STEP blocks only (no shadow is advanced during the launch; an
  // environment that ends in it warms its next episode up inline -- WHEN the warm-up frames are computed cannot change a result)
  bind_full_step(eng, p, d_actions, d_obs, d_reward, d_terminated, d_truncated, d_info_speed, d_info_crashed);
  p.k_steps = k_steps;
  p.num_envs = eng->cfg.num_envs;
  HWY_HIP(eng, with_family(eng, p, [&](const auto &a) { return hwy::launch_rollout(a, launch_of(eng)); }));
  return HWY_OK;
}

// The host-pointer form of a K-step call (hwy_rollout, hwy_rollout_continuous): the validated actions (`act_bytes` per step) up into
// the engine's rollout block, `run` on the device pointers of that block, the outputs down; synchronises.  The device is set.
template <typename Run>
static int rollout_through_host(hwy_engine *eng, size_t K, const void *actions, size_t act_bytes, float *obs, double *reward,
                                uint8_t *terminated, uint8_t *truncated, double *info_speed, uint8_t *info_crashed, Run &&run) {
  const size_t n_act = num_agent_rows(eng->cfg), n_obs = num_obs_floats(eng->cfg), E = eng->cfg.num_envs;
  auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  const size_t o_act = 0, o_rew = up(K * act_bytes), o_spd = o_rew + up(K * n_act * 8), o_obs = o_spd + up(K * n_act * 8),
               o_term = o_obs + up(K * n_obs * 4), o_trunc = o_term + up(K * E), o_crash = o_trunc + up(K * E),
               total = o_crash + up(K * n_act);
  if (total > eng->roll_bytes) {
    HWY_HIP(eng, hipStreamSynchronize(eng->stream));
    if (eng->d_roll) (void)hipFree(eng->d_roll);
    eng->d_roll = nullptr;
    eng->roll_bytes = 0;
    HWY_HIP(eng, hipMalloc((void **)&eng->d_roll, total));
    eng->roll_bytes = total;
  }
  char *d = eng->d_roll;
  HWY_HIP(eng, hipMemcpyAsync(d + o_act, actions, K * act_bytes, hipMemcpyHostToDevice, eng->stream));
  if (int rc = run((const void *)(d + o_act), (float *)(d + o_obs), (double *)(d + o_rew), (uint8_t *)(d + o_term), (uint8_t *)(d + o_trunc),
                   (double *)(d + o_spd), (uint8_t *)(d + o_crash)))
    return rc;
  HWY_HIP(eng, hipMemcpyAsync(obs, d + o_obs, K * n_obs * 4, hipMemcpyDeviceToHost, eng->stream));
  HWY_HIP(eng, hipMemcpyAsync(reward, d + o_rew, K * n_act * 8, hipMemcpyDeviceToHost, eng->stream));
  HWY_HIP(eng, hipMemcpyAsync(terminated, d + o_term, K * E, hipMemcpyDeviceToHost, eng->stream));
  HWY_HIP(eng, hipMemcpyAsync(truncated, d + o_trunc, K * E, hipMemcpyDeviceToHost, eng->stream));
  if (info_speed) HWY_HIP(eng, hipMemcpyAsync(info_speed, d + o_spd, K * n_act * 8, hipMemcpyDeviceToHost, eng->stream));
  if (info_crashed) HWY_HIP(eng, hipMemcpyAsync(info_crashed, d + o_crash, K * n_act, hipMemcpyDeviceToHost, eng->stream));
  HWY_HIP(eng, hipStreamSynchronize(eng->stream));
  return HWY_OK;
}

extern "C" int hwy_rollout(hwy_engine *eng, int32_t k_steps, const int32_t *actions, float *obs, double *reward,
                           uint8_t *terminated, uint8_t *truncated, double *info_speed, uint8_t *info_crashed) {
  if (!eng) return HWY_ERR_INVALID_ARG;
  if (k_steps < 1) return fail(eng, HWY_ERR_INVALID_ARG, "hwy_rollout: k_steps must be >= 1");
  if (!actions || !obs || !reward || !terminated || !truncated)
    return fail(eng, HWY_ERR_INVALID_ARG, "hwy_rollout: actions/obs/reward/terminated/truncated must be non-NULL");
  if (k_steps > 1 && is_ix(eng) && (eng->cfg.flags & HWY_C_HOST_TRAFFIC))
    return fail(eng, HWY_ERR_INVALID_ARG, "hwy_rollout: k_steps > 1 needs device traffic (HWY_C_HOST_TRAFFIC is set)");
  const size_t n_act = num_agent_rows(eng->cfg), K = (size_t)k_steps;
  const int max_action = num_action_ids(eng) - 1;
  for (size_t k = 0; k < K * n_act; ++k)  // the reference's KeyError / IndexError, before anything is simulated (action.py:260,195)
    if (actions[k] < 0 || actions[k] > max_action) return fail(eng, HWY_ERR_ACTION, "action id out of range");
  HWY_HIP(eng, hipSetDevice(eng->device));
  return rollout_through_host(eng, K, actions, n_act * 4, obs, reward, terminated, truncated, info_speed, info_crashed,
                              [&](const void *d_act, float *d_obs, double *d_rew, uint8_t *d_term, uint8_t *d_trunc, double *d_spd, uint8_t *d_crash) {
                                return hwy_rollout_device(eng, k_steps, (const int32_t *)d_act, d_obs, d_rew, d_term, d_trunc, d_spd, d_crash);
                              });
}

extern "C" int hwy_step(hwy_engine *eng, const int32_t *actions, float *obs, double *reward, uint8_t *terminated,
                        uint8_t *truncated, double *info_speed, uint8_t *info_crashed) {
  if (!eng) return HWY_ERR_INVALID_ARG;
  if (!actions || !obs || !reward || !terminated || !truncated)
    return fail(eng, HWY_ERR_INVALID_ARG, "hwy_step: actions/obs/reward/terminated/truncated must be non-NULL");
  const size_t n_act = num_agent_rows(eng->cfg), n_obs = num_obs_floats(eng->cfg);
  const size_t E = eng->cfg.num_envs;
  // the reference raises KeyError for an unknown meta-action before touching the simulation (action.py:260)
  const int max_action = num_action_ids(eng) - 1;  // IntersectionEnv.ACTIONS has 3 entries (intersection_env.py:14)
  for (size_t k = 0; k < n_act; ++k)
    if (actions[k] < 0 || actions[k] > max_action)
      return fail(eng, HWY_ERR_ACTION, is_direct(eng) ? "action id outside the throttle x steering table" : max_action == 2 ? "meta-action outside [0,3)" : "meta-action outside [0,5)");
  HWY_HIP(eng, hipSetDevice(eng->device));
  // pinned layout: [mirror of the device output block][actions]
  char *h_out = (char *)eng->h_pinned;
  int32_t *h_act = (int32_t *)(h_out + eng->out_bytes);
  std::memcpy(h_act, actions, n_act * 4);
  HWY_HIP(eng, hipMemcpyAsync(eng->d_actions, h_act, n_act * 4, hipMemcpyHostToDevice, eng->stream));
  if (int rc = hwy_step_device(eng, eng->d_actions, eng->d_obs, eng->d_reward, eng->d_term, eng->d_trunc,
                               eng->d_info_speed, eng->d_info_crashed))
    return rc;
  HWY_HIP(eng, hipMemcpyAsync(h_out, eng->d_out, eng->out_bytes, hipMemcpyDeviceToHost, eng->stream));
  HWY_HIP(eng, hipStreamSynchronize(eng->stream));
  std::memcpy(obs, h_out + eng->off_obs, n_obs * 4);
  std::memcpy(reward, h_out + eng->off_reward, n_act * 8);
  std::memcpy(terminated, h_out + eng->off_term, E);
  std::memcpy(truncated, h_out + eng->off_trunc, E);
  if (info_speed) std::memcpy(info_speed, h_out + eng->off_speed, n_act * 8);
  if (info_crashed) std::memcpy(info_crashed, h_out + eng->off_crashed, n_act);
  return HWY_OK;
}

extern "C" int hwy_step_frames(hwy_engine *eng, const int32_t *actions, int32_t n_frames) {
  if (!eng || n_frames < 0) return HWY_ERR_INVALID_ARG;
  HWY_HIP(eng, hipSetDevice(eng->device));
  const size_t n_act = num_agent_rows(eng->cfg);
  StepParams p;
  fill_params(eng, p);
  p.n_frames = n_frames;
  p.full_step = 0;
  p.autoreset = 0;
  if (actions) {
    for (size_t k = 0; k < n_act; ++k)
      if (actions[k] < 0 || actions[k] >= num_action_ids(eng)) return fail(eng, HWY_ERR_ACTION, "action id out of range");
    std::memcpy(eng->h_pinned, actions, n_act * 4);
    HWY_HIP(eng, hipMemcpyAsync(eng->d_actions, eng->h_pinned, n_act * 4, hipMemcpyHostToDevice, eng->stream));
    p.actions = eng->d_actions;
  }
  p.reward = eng->d_reward; p.terminated = eng->d_term; p.truncated = eng->d_trunc;
  if (int rc = timed_launch(eng, p)) return rc;
  HWY_HIP(eng, hipStreamSynchronize(eng->stream));
  return HWY_OK;
}

extern "C" int hwy_observe(hwy_engine *eng, float *obs) {
  if (!eng || !obs) return HWY_ERR_INVALID_ARG;
  HWY_HIP(eng, hipSetDevice(eng->device));
  const size_t n_obs = num_obs_floats(eng->cfg);
  StepParams p;
  fill_params(eng, p);
  p.obs = eng->d_obs;
  p.reward = eng->d_reward; p.terminated = eng->d_term; p.truncated = eng->d_trunc;
  HWY_HIP(eng, launch_stage(eng, OBSERVE, p));
  HWY_HIP(eng, hipMemcpyAsync(eng->h_pinned, eng->d_obs, n_obs * 4, hipMemcpyDeviceToHost, eng->stream));
  HWY_HIP(eng, hipStreamSynchronize(eng->stream));
  std::memcpy(obs, eng->h_pinned, n_obs * 4);
  return HWY_OK;
}

// ---- reset --------------------------------------------------------------------------------------------------
static int set_reset_params(hwy_engine *eng, double ego_spacing, double vehicles_density, int32_t initial_lane_id) {
  if (!(ego_spacing > 0) || !(vehicles_density > 0)) return fail(eng, HWY_ERR_INVALID_ARG, "spacing/density must be positive");
  if (initial_lane_id >= eng->cfg.lanes_count) return fail(eng, HWY_ERR_INVALID_ARG, "initial_lane_id out of range");
  hwy::set_reset_args(eng->rp, ego_spacing, vehicles_density, initial_lane_id);
  return HWY_OK;
}

extern "C" int hwy_reset(hwy_engine *eng, const uint8_t *mask, const uint64_t *seeds, double ego_spacing,
                         double vehicles_density, int32_t initial_lane_id, float *obs) {
  if (!eng) return HWY_ERR_INVALID_ARG;
  if (int rc = set_reset_params(eng, ego_spacing, vehicles_density, initial_lane_id)) return rc;
  HWY_HIP(eng, hipSetDevice(eng->device));
  const size_t E = eng->cfg.num_envs;
  const size_t n_obs = num_obs_floats(eng->cfg);
  StepParams p;
  fill_params(eng, p);
  char *base = (char *)eng->h_pinned;
  if (seeds) {
    std::memcpy(base, seeds, E * 8);
    HWY_HIP(eng, hipMemcpyAsync(eng->d_seeds, base, E * 8, hipMemcpyHostToDevice, eng->stream));
    p.reset_seeds = eng->d_seeds;
  }
  if (mask) {
    std::memcpy(base + E * 8, mask, E);
    HWY_HIP(eng, hipMemcpyAsync(eng->d_mask, base + E * 8, E, hipMemcpyHostToDevice, eng->stream));
    p.reset_mask = eng->d_mask;
  }
  p.obs = eng->d_obs;  // (a Lidar engine traces every row; only the masked ones are copied out below)
  p.reward = eng->d_reward; p.terminated = eng->d_term; p.truncated = eng->d_trunc;
  HWY_HIP(eng, launch_stage(eng, RESET, p));
  HWY_HIP(eng, hipStreamSynchronize(eng->stream));
  eng->has_state = true;
  if (obs) {
    HWY_HIP(eng, hipMemcpyAsync(eng->h_pinned, eng->d_obs, n_obs * 4, hipMemcpyDeviceToHost, eng->stream));
    HWY_HIP(eng, hipStreamSynchronize(eng->stream));
    const size_t per_env = n_obs / E;
    const float *src = (const float *)eng->h_pinned;
    for (size_t e = 0; e < E; ++e)
      if (!mask || mask[e]) std::memcpy(obs + e * per_env, src + e * per_env, per_env * 4);
  }
  return HWY_OK;
}

extern "C" int hwy_set_autoreset(hwy_engine *eng, int32_t enabled, uint64_t base_seed, double ego_spacing,
                                 double vehicles_density, int32_t initial_lane_id) {
  if (!eng) return HWY_ERR_INVALID_ARG;
  if (int rc = set_reset_params(eng, ego_spacing, vehicles_density, initial_lane_id)) return rc;
  eng->autoreset = enabled ? 1 : 0;
  if (eng->rp.base_seed != base_seed) {  // pre-warmed next episodes were drawn from the old seeds
    HWY_HIP(eng, hipSetDevice(eng->device));
    HWY_HIP(eng, invalidate_shadows(eng));
  }
  eng->rp.base_seed = base_seed;
  return HWY_OK;
}

extern "C" int hwy_debug_math(hwy_engine *eng, int32_t op, const double *in, double *out, int64_t n) {
  if (!eng || !in || !out || n < 0 || op < 0 || (op > 12 && (op < 20 || op > 33) && (op < 40 || op > 42))) return HWY_ERR_INVALID_ARG;
  // op 40 (wave_max_u32) is a DPP reduction that is only correct with all 64 lanes of every wavefront enabled
  if (op == 40 && n % 64 != 0) return fail(eng, HWY_ERR_INVALID_ARG, "hwy_debug_math: op 40 takes whole wavefronts (n % 64 == 0)");
  if (n == 0) return HWY_OK;
  HWY_HIP(eng, hipSetDevice(eng->device));
  double *d_in = nullptr, *d_out = nullptr;
  HWY_HIP(eng, hipMalloc((void **)&d_in, n * sizeof(double)));
  if (hipMalloc((void **)&d_out, n * sizeof(double)) != hipSuccess) { (void)hipFree(d_in); return fail(eng, HWY_ERR_HIP, "hipMalloc"); }
  hipError_t e = hipMemcpyAsync(d_in, in, n * sizeof(double), hipMemcpyHostToDevice, eng->stream);
  if (e == hipSuccess) e = hwy::launch_math_probe(op, d_in, d_out, (long long)n, eng->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, n * sizeof(double), hipMemcpyDeviceToHost, eng->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(eng->stream);
  (void)hipFree(d_in);
  (void)hipFree(d_out);
  if (e != hipSuccess) return fail(eng, HWY_ERR_HIP, std::string("hwy_debug_math: ") + hipGetErrorString(e));
  return HWY_OK;
}

extern "C" int hwy_get_counters(hwy_engine *eng, uint64_t *out, int32_t n, int32_t reset) {
  if (!eng || !out || n < 0) return HWY_ERR_INVALID_ARG;
  HWY_HIP(eng, hipSetDevice(eng->device));
  unsigned long long host[HWY_CTR_COUNT];
  HWY_HIP(eng, hipMemcpyAsync(host, eng->d_counters, sizeof host, hipMemcpyDeviceToHost, eng->stream));
  if (reset) HWY_HIP(eng, hipMemsetAsync(eng->d_counters, 0, sizeof host, eng->stream));
  HWY_HIP(eng, hipStreamSynchronize(eng->stream));
  for (int k = 0; k < n && k < HWY_CTR_COUNT; ++k) out[k] = host[k];
  return HWY_OK;
}

extern "C" int hwy_set_block_order(hwy_engine *eng, const int32_t *env_of_block) {
  if (!eng) return HWY_ERR_INVALID_ARG;
  HWY_HIP(eng, hipSetDevice(eng->device));
  const int E = eng->cfg.num_envs;
  if (!env_of_block) {  // back to the identity
    HWY_HIP(eng, hipStreamSynchronize(eng->stream));
    if (eng->d_block_env) { HWY_HIP(eng, hipFree(eng->d_block_env)); eng->d_block_env = nullptr; }
    return HWY_OK;
  }
  if (eng->cfg.scenario != HWY_SCENARIO_HIGHWAY || eng->cfg.num_vehicles > 64 || eng->force_block_kernel || E > 65535)
    return fail(eng, HWY_ERR_INVALID_ARG, "hwy_set_block_order: only the one-wavefront step kernel (highway scenario, N <= 64, "
                                          "at most 65535 environments) takes a workgroup order");
  std::vector<uint8_t> seen((size_t)E, 0);
  std::vector<uint16_t> tab((size_t)E);
  for (int b = 0; b < E; ++b) {
    const int32_t e = env_of_block[b];
    if (e < 0 || e >= E || seen[(size_t)e]) return fail(eng, HWY_ERR_INVALID_ARG, "hwy_set_block_order: not a permutation of 0 .. num_envs - 1");
    seen[(size_t)e] = 1;
    tab[(size_t)b] = (uint16_t)e;
  }
  if (!eng->d_block_env) HWY_HIP(eng, hipMalloc((void **)&eng->d_block_env, (size_t)E * sizeof(uint16_t)));
  HWY_HIP(eng, hipMemcpyAsync(eng->d_block_env, tab.data(), (size_t)E * sizeof(uint16_t), hipMemcpyHostToDevice, eng->stream));
  HWY_HIP(eng, hipStreamSynchronize(eng->stream));  // (tab is a local)
  return HWY_OK;
}

extern "C" int hwy_comm_unique_id(uint8_t *id) {
  if (!id) return fail(nullptr, HWY_ERR_INVALID_ARG, "id is NULL");
  std::string err;
  const int rc = hwy::comm_unique_id(id, err);
  return rc ? fail(nullptr, rc, err) : HWY_OK;
}
extern "C" int hwy_comm_init(hwy_engine *eng, const uint8_t *id, int32_t rank, int32_t world) {
  if (!eng || !id || world < 1 || rank < 0 || rank >= world) return HWY_ERR_INVALID_ARG;
  if (eng->comm) return fail(eng, HWY_ERR_INVALID_ARG, "hwy_comm_init: this engine already has a communicator");
  HWY_HIP(eng, hipSetDevice(eng->device));
  std::string err;
  const int rc = hwy::comm_init(&eng->comm, id, rank, world, err);
  return rc ? fail(eng, rc, err) : HWY_OK;
}
extern "C" int hwy_gather(hwy_engine *eng, const void *d_send, void *d_recv, size_t bytes, int32_t root) {
  if (!eng || !d_send) return HWY_ERR_INVALID_ARG;
  if (!eng->comm) return fail(eng, HWY_ERR_INVALID_ARG, "hwy_gather: call hwy_comm_init first");
  if (root < 0 || root >= hwy::comm_world(eng->comm)) return fail(eng, HWY_ERR_INVALID_ARG, "hwy_gather: root out of range");
  if (hwy::comm_rank(eng->comm) == root && !d_recv) return fail(eng, HWY_ERR_INVALID_ARG, "hwy_gather: d_recv is NULL on the root");
  HWY_HIP(eng, hipSetDevice(eng->device));
  std::string err;
  const int rc = hwy::comm_gather(eng->comm, d_send, d_recv, bytes, root, eng->stream, err);
  return rc ? fail(eng, rc, err) : HWY_OK;
}
extern "C" int hwy_comm_destroy(hwy_engine *eng) {
  if (!eng) return HWY_ERR_INVALID_ARG;
  if (eng->comm) {
    (void)hipSetDevice(eng->device);
    (void)hipStreamSynchronize(eng->stream);
    hwy::comm_destroy(eng->comm);
    eng->comm = nullptr;
  }
  return HWY_OK;
}

// ---- time-to-collision grid and finite-MDP planner (hwy_ttc.h) -------------------------------------------------------------------
static int ttc_check(hwy_engine *eng, const hwy_ttc_params *params, const char *who) {
  const char *why = "";
  if (const int rc = hwy::ttc_validate(eng->cfg, params, &why)) return fail(eng, rc, std::string(who) + ": " + why);
  return HWY_OK;
}
static hipError_t ttc_launch(const hwy_engine *eng, const hwy_ttc_params &tp, bool plan, float *d_grid, int32_t *d_action, double *d_q) {
  const size_t plane = (size_t)eng->cfg.num_envs * eng->pitch;
  const double *f = eng->d_f64;  // planes: x | y | heading | speed | ...
  const hwy::TtcParams p = hwy::ttc_params(eng->cfg, tp, f, f + 2 * plane, f + 3 * plane, eng->d_packed, eng->pitch, d_grid, d_action, d_q);
  return hwy::launch_ttc(p, plan, (int)num_agent_rows(eng->cfg), eng->stream);
}
// the engine's own output buffers of the host-pointer forms (the grid's size depends on the call's time_steps)
static int ttc_buffers(hwy_engine *eng, int cells) {
  const size_t rows = num_agent_rows(eng->cfg);
  if (eng->ttc_cells < cells) {
    if (eng->d_ttc_grid) { HWY_HIP(eng, hipStreamSynchronize(eng->stream)); HWY_HIP(eng, hipFree(eng->d_ttc_grid)); eng->d_ttc_grid = nullptr; }
    eng->ttc_cells = 0;
    HWY_HIP(eng, hipMalloc((void **)&eng->d_ttc_grid, rows * cells * sizeof(float)));
    eng->ttc_cells = cells;
  }
  if (!eng->d_plan_action) HWY_HIP(eng, hipMalloc((void **)&eng->d_plan_action, rows * sizeof(int32_t)));
  if (!eng->d_plan_q) HWY_HIP(eng, hipMalloc((void **)&eng->d_plan_q, rows * 5 * sizeof(double)));
  return HWY_OK;
}

extern "C" int hwy_ttc_grid_device(hwy_engine *eng, const hwy_ttc_params *params, float *d_grid) {
  if (!eng) return HWY_ERR_INVALID_ARG;
  if (int rc = ttc_check(eng, params, "hwy_ttc_grid_device")) return rc;
  if (!d_grid) return fail(eng, HWY_ERR_INVALID_ARG, "hwy_ttc_grid_device: grid must be non-NULL");
  HWY_HIP(eng, hipSetDevice(eng->device));
  HWY_HIP(eng, ttc_launch(eng, *params, false, d_grid, nullptr, nullptr));
  return HWY_OK;
}

extern "C" int hwy_ttc_grid(hwy_engine *eng, const hwy_ttc_params *params, float *grid) {
  if (!eng) return HWY_ERR_INVALID_ARG;
  if (int rc = ttc_check(eng, params, "hwy_ttc_grid")) return rc;
  if (!grid) return fail(eng, HWY_ERR_INVALID_ARG, "hwy_ttc_grid: grid must be non-NULL");
  HWY_HIP(eng, hipSetDevice(eng->device));
  const int cells = hwy::ttc_cells(eng->cfg, *params);
  if (int rc = ttc_buffers(eng, cells)) return rc;
  HWY_HIP(eng, ttc_launch(eng, *params, false, eng->d_ttc_grid, nullptr, nullptr));
  HWY_HIP(eng, hipMemcpyAsync(grid, eng->d_ttc_grid, num_agent_rows(eng->cfg) * cells * sizeof(float), hipMemcpyDeviceToHost, eng->stream));
  HWY_HIP(eng, hipStreamSynchronize(eng->stream));
  return HWY_OK;
}

extern "C" int hwy_mdp_plan_device(hwy_engine *eng, const hwy_ttc_params *params, int32_t *d_action, double *d_q, float *d_grid) {
  if (!eng) return HWY_ERR_INVALID_ARG;
  if (int rc = ttc_check(eng, params, "hwy_mdp_plan_device")) return rc;
  if (!d_action) return fail(eng, HWY_ERR_INVALID_ARG, "hwy_mdp_plan_device: action must be non-NULL");
  HWY_HIP(eng, hipSetDevice(eng->device));
  HWY_HIP(eng, ttc_launch(eng, *params, true, d_grid, d_action, d_q));
  return HWY_OK;
}

extern "C" int hwy_mdp_plan(hwy_engine *eng, const hwy_ttc_params *params, int32_t *action, double *q, float *grid) {
  if (!eng) return HWY_ERR_INVALID_ARG;
  if (int rc = ttc_check(eng, params, "hwy_mdp_plan")) return rc;
  if (!action) return fail(eng, HWY_ERR_INVALID_ARG, "hwy_mdp_plan: action must be non-NULL");
  HWY_HIP(eng, hipSetDevice(eng->device));
  const int cells = hwy::ttc_cells(eng->cfg, *params);
  const size_t rows = num_agent_rows(eng->cfg);
  if (int rc = ttc_buffers(eng, cells)) return rc;
  HWY_HIP(eng, ttc_launch(eng, *params, true, grid ? eng->d_ttc_grid : nullptr, eng->d_plan_action, q ? eng->d_plan_q : nullptr));
  HWY_HIP(eng, hipMemcpyAsync(action, eng->d_plan_action, rows * sizeof(int32_t), hipMemcpyDeviceToHost, eng->stream));
  if (q) HWY_HIP(eng, hipMemcpyAsync(q, eng->d_plan_q, rows * 5 * sizeof(double), hipMemcpyDeviceToHost, eng->stream));
  if (grid) HWY_HIP(eng, hipMemcpyAsync(grid, eng->d_ttc_grid, rows * cells * sizeof(float), hipMemcpyDeviceToHost, eng->stream));
  HWY_HIP(eng, hipStreamSynchronize(eng->stream));
  return HWY_OK;
}

// ---- environment fork and rollout scoring (hwy_lookahead.h) --------------------------------------------------------------------------
static int fork_check(hwy_engine *dst, hwy_engine *src, int32_t branches, bool has_src_env, const char *who) {
  if (!dst) return HWY_ERR_INVALID_ARG;
  if (!src) return fail(dst, HWY_ERR_INVALID_ARG, std::string(who) + ": src is NULL");
  const char *why = "";
  if (const int rc = hwy::fork_validate(dst->cfg, src->cfg, dst == src, branches, has_src_env, &why)) return fail(dst, rc, std::string(who) + ": " + why);
  if (dst->device != src->device) return fail(dst, HWY_ERR_INVALID_ARG, std::string(who) + ": the two engines are on different devices");
  return HWY_OK;
}

// the engine's planes as a fork sees them: whole packed words (the rank hint travels)
static hwy::ForkView fork_view(const hwy_engine *eng) {
  hwy::ForkView v;
  memset(&v, 0, sizeof v);
  v.cfg = &eng->cfg;
  const size_t plane = (size_t)eng->cfg.num_envs * eng->pitch;
  for (int f = 0; f < 9; ++f) v.f64[f] = eng->d_f64 + f * plane;
  v.behavior = eng->d_behavior;
  v.i32[0] = eng->d_packed;
  v.n_i32 = 1;
  v.controls = eng->d_controls;
  v.time = eng->d_time; v.episode = eng->d_episode; v.done = eng->d_done;
  v.pitch = eng->pitch;
  return v;
}

extern "C" int hwy_fork_device(hwy_engine *dst, hwy_engine *src, int32_t branches, const int32_t *d_src_env) {
  if (int rc = fork_check(dst, src, branches, d_src_env != nullptr, "hwy_fork_device")) return rc;
  HWY_HIP(dst, hipSetDevice(dst->device));
  if (dst->stream != src->stream) {  // what src's stream holds so far comes first
    if (!dst->fork_event) HWY_HIP(dst, hipEventCreateWithFlags(&dst->fork_event, hipEventDisableTiming));
    HWY_HIP(dst, hipEventRecord(dst->fork_event, src->stream));
    HWY_HIP(dst, hipStreamWaitEvent(dst->stream, dst->fork_event, 0));
  }
  const hwy::ForkParams p = hwy::fork_params(fork_view(dst), fork_view(src), branches, d_src_env);
  HWY_HIP(dst, hwy::launch_fork(p, dst->stream));
  dst->has_state = dst->has_state || src->has_state;
  return HWY_OK;
}

extern "C" int hwy_fork(hwy_engine *dst, hwy_engine *src, int32_t branches, const int32_t *src_env) {
  if (!src_env) return hwy_fork_device(dst, src, branches, nullptr);
  if (int rc = fork_check(dst, src, branches, true, "hwy_fork")) return rc;
  const size_t E = dst->cfg.num_envs;
  for (size_t j = 0; j < E; ++j)
    if (src_env[j] < 0 || src_env[j] >= src->cfg.num_envs) return fail(dst, HWY_ERR_INVALID_ARG, "hwy_fork: source index outside [0, src.num_envs)");
  HWY_HIP(dst, hipSetDevice(dst->device));
  if (!dst->d_fork_src) HWY_HIP(dst, hipMalloc((void **)&dst->d_fork_src, E * sizeof(int32_t)));
  std::memcpy(dst->h_pinned, src_env, E * sizeof(int32_t));
  HWY_HIP(dst, hipMemcpyAsync(dst->d_fork_src, dst->h_pinned, E * sizeof(int32_t), hipMemcpyHostToDevice, dst->stream));
  if (int rc = hwy_fork_device(dst, src, branches, dst->d_fork_src)) return rc;
  HWY_HIP(dst, hipStreamSynchronize(dst->stream));  // (the staging buffer is the engine's)
  return HWY_OK;
}

extern "C" int hwy_score_device(hwy_engine *eng, int32_t k_steps, int32_t branches, double gamma, const int32_t *d_first_action,
                                const double *d_reward, const uint8_t *d_terminated, const uint8_t *d_truncated, double *d_return,
                                double *d_q, int32_t *d_best_action, int32_t *d_best_branch) {
  if (!eng) return HWY_ERR_INVALID_ARG;
  const char *why = "";
  if (const int rc = hwy::score_validate(eng->cfg, k_steps, branches, gamma, d_first_action != nullptr, d_reward && d_terminated && d_truncated,
                                         d_q != nullptr, d_best_action != nullptr, &why))
    return fail(eng, rc, std::string("hwy_score_device: ") + why);
  HWY_HIP(eng, hipSetDevice(eng->device));
  const hwy::ScoreParams p = hwy::score_params(eng->cfg, k_steps, branches, gamma, d_first_action, d_reward, d_terminated, d_truncated,
                                               d_return, d_q, d_best_action, d_best_branch);
  HWY_HIP(eng, hwy::launch_score(p, eng->stream));
  return HWY_OK;
}

extern "C" int hwy_score_rollout(hwy_engine *eng, int32_t k_steps, int32_t branches, double gamma, const int32_t *actions,
                                 double *reward, uint8_t *terminated, uint8_t *truncated, double *ret, double *q,
                                 int32_t *best_action, int32_t *best_branch) {
  if (!eng) return HWY_ERR_INVALID_ARG;
  const bool single = eng->cfg.num_agents == 1;
  const char *why = "";
  if (const int rc = hwy::score_validate(eng->cfg, k_steps, branches, gamma, single, true, q != nullptr, best_action != nullptr, &why))
    return fail(eng, rc, std::string("hwy_score_rollout: ") + why);
  if (!actions) return fail(eng, HWY_ERR_INVALID_ARG, "hwy_score_rollout: actions must be non-NULL");
  const size_t n_act = num_agent_rows(eng->cfg), n_obs = num_obs_floats(eng->cfg);
  const size_t EB = eng->cfg.num_envs, K = (size_t)k_steps, E = EB / branches, ids = (size_t)num_action_ids(eng);
  for (size_t k = 0; k < K * n_act; ++k)  // like hwy_rollout, before anything is simulated
    if (actions[k] < 0 || actions[k] >= (int32_t)ids) return fail(eng, HWY_ERR_ACTION, "action id out of range");
  HWY_HIP(eng, hipSetDevice(eng->device));
  auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  const size_t o_act = 0, o_rew = up(K * n_act * 4), o_obs = o_rew + up(K * n_act * 8), o_term = o_obs + up(K * n_obs * 4),
               o_trunc = o_term + up(K * EB), o_ret = o_trunc + up(K * EB), o_q = o_ret + up(n_act * 8), o_ba = o_q + up(E * ids * 8),
               o_bb = o_ba + up(E * 4), total = o_bb + up(E * eng->cfg.num_agents * 4);
  if (total > eng->roll_bytes) {
    HWY_HIP(eng, hipStreamSynchronize(eng->stream));
    if (eng->d_roll) (void)hipFree(eng->d_roll);
    eng->d_roll = nullptr;
    eng->roll_bytes = 0;
    HWY_HIP(eng, hipMalloc((void **)&eng->d_roll, total));
    eng->roll_bytes = total;
  }
  char *d = eng->d_roll;
  HWY_HIP(eng, hipMemcpyAsync(d + o_act, actions, K * n_act * 4, hipMemcpyHostToDevice, eng->stream));
  if (int rc = hwy_rollout_device(eng, k_steps, (const int32_t *)(d + o_act), (float *)(d + o_obs), (double *)(d + o_rew),
                                  (uint8_t *)(d + o_term), (uint8_t *)(d + o_trunc), nullptr, nullptr))
    return rc;
  // single agent: q and the best first action are always folded (first_action and they go together)
  if (int rc = hwy_score_device(eng, k_steps, branches, gamma, single ? (const int32_t *)(d + o_act) : nullptr, (const double *)(d + o_rew),
                                (const uint8_t *)(d + o_term), (const uint8_t *)(d + o_trunc), (double *)(d + o_ret),
                                single ? (double *)(d + o_q) : nullptr, single ? (int32_t *)(d + o_ba) : nullptr, (int32_t *)(d + o_bb)))
    return rc;
  if (reward) HWY_HIP(eng, hipMemcpyAsync(reward, d + o_rew, K * n_act * 8, hipMemcpyDeviceToHost, eng->stream));
  if (terminated) HWY_HIP(eng, hipMemcpyAsync(terminated, d + o_term, K * EB, hipMemcpyDeviceToHost, eng->stream));
  if (truncated) HWY_HIP(eng, hipMemcpyAsync(truncated, d + o_trunc, K * EB, hipMemcpyDeviceToHost, eng->stream));
  if (ret) HWY_HIP(eng, hipMemcpyAsync(ret, d + o_ret, n_act * 8, hipMemcpyDeviceToHost, eng->stream));
  if (q) HWY_HIP(eng, hipMemcpyAsync(q, d + o_q, E * ids * 8, hipMemcpyDeviceToHost, eng->stream));
  if (best_action) HWY_HIP(eng, hipMemcpyAsync(best_action, d + o_ba, E * 4, hipMemcpyDeviceToHost, eng->stream));
  if (best_branch) HWY_HIP(eng, hipMemcpyAsync(best_branch, d + o_bb, E * eng->cfg.num_agents * 4, hipMemcpyDeviceToHost, eng->stream));
  HWY_HIP(eng, hipStreamSynchronize(eng->stream));
  return HWY_OK;
}

// ---- optimistic planning, one tree per environment (hwy_opd.h) -------------------------------------------------------------------------
extern "C" int hwy_action_mask_device(hwy_engine *eng, uint8_t *d_mask);  // (below)
// `waiter`'s stream continues behind what `signaler`'s stream holds so far
static int stream_after(hwy_engine *waiter, hwy_engine *signaler) {
  if (waiter->stream == signaler->stream) return HWY_OK;
  if (!waiter->fork_event) HWY_HIP(waiter, hipEventCreateWithFlags(&waiter->fork_event, hipEventDisableTiming));
  HWY_HIP(waiter, hipEventRecord(waiter->fork_event, signaler->stream));
  HWY_HIP(waiter, hipStreamWaitEvent(waiter->stream, waiter->fork_event, 0));
  return HWY_OK;
}

static int opd_check(hwy_engine *src, hwy_engine *tree, hwy_engine *work, const hwy_opd_params *params, bool has_action, const char *who) {
  if (!src) return HWY_ERR_INVALID_ARG;
  if (!tree || !work) return fail(src, HWY_ERR_INVALID_ARG, std::string(who) + ": tree / work is NULL");
  if (src == tree || src == work || tree == work) return fail(src, HWY_ERR_INVALID_ARG, std::string(who) + ": src, tree and work must be three engines");
  const char *why = "";
  if (const int rc = hwy::opd_validate(src->cfg, tree->cfg, work->cfg, params, has_action, &why)) return fail(src, rc, std::string(who) + ": " + why);
  if (tree->autoreset || work->autoreset) return fail(src, HWY_ERR_INVALID_ARG, std::string(who) + ": tree and work must run with auto-reset off");
  if (tree->device != src->device || work->device != src->device) return fail(src, HWY_ERR_INVALID_ARG, std::string(who) + ": the three engines are on different devices");
  return HWY_OK;
}

// a failure of a call on `tree` / `work` is reported on `src`, the engine the caller asks
static int opd_forward(hwy_engine *src, hwy_engine *other, int rc) {
  if (rc != HWY_OK && other != src) src->err = other->err;
  return rc;
}

// the block of `tree` that holds the planner's arrays: ret | disc | upper0 [E][M] f64, expanded_node [E][X], gather_src [E n],
// scatter_src | root_src [E M], actions [E n], done [E][M] u8, then the host form's outputs: action [E], value | upper [E] f64,
// sequence [E][X], expanded [E]
struct OpdLayout {
  size_t ret, disc, up0, node, gather, scatter, root, act, done, o_action, o_value, o_upper, o_sequence, o_expanded, created, child_mask, total;
};
static OpdLayout opd_layout(size_t E, size_t n, size_t M, size_t X) {
  auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  OpdLayout l;
  l.ret = 0; l.disc = l.ret + up(E * M * 8); l.up0 = l.disc + up(E * M * 8); l.node = l.up0 + up(E * M * 8);
  l.gather = l.node + up(E * X * 4); l.scatter = l.gather + up(E * n * 4); l.root = l.scatter + up(E * M * 4);
  l.act = l.root + up(E * M * 4); l.done = l.act + up(E * n * 4); l.o_action = l.done + up(E * M);
  l.o_value = l.o_action + up(E * 4); l.o_upper = l.o_value + up(E * 8); l.o_sequence = l.o_upper + up(E * 8);
  l.o_expanded = l.o_sequence + up(E * X * 4); l.created = l.o_expanded + up(E * 4);
  l.child_mask = l.created + up(E * M); l.total = l.child_mask + up(E * n * n);  // (the masked search's two arrays, at the end)
  return l;
}
static int opd_block(hwy_engine *src, hwy_engine *tree, hwy_engine *work, const OpdLayout &l) {
  if (l.total <= tree->opd_bytes) return HWY_OK;
  HWY_HIP(src, hipStreamSynchronize(work->stream));  // (a smaller block may still be in use)
  if (tree->d_opd) (void)hipFree(tree->d_opd);
  tree->d_opd = nullptr;
  tree->opd_bytes = 0;
  HWY_HIP(src, hipMalloc((void **)&tree->d_opd, l.total));
  tree->opd_bytes = l.total;
  return HWY_OK;
}

extern "C" int hwy_opd_plan_device(hwy_engine *src, hwy_engine *tree, hwy_engine *work, const hwy_opd_params *params, int32_t *d_action,
                                   double *d_value, double *d_upper, int32_t *d_sequence, int32_t *d_expanded) {
  if (int rc = opd_check(src, tree, work, params, d_action != nullptr, "hwy_opd_plan_device")) return rc;
  HWY_HIP(src, hipSetDevice(src->device));
  const size_t E = src->cfg.num_envs, n = params->n_ids, M = params->nodes, X = params->budget / params->n_ids;
  const OpdLayout l = opd_layout(E, n, M, X);
  if (int rc = opd_block(src, tree, work, l)) return rc;
  char *d = tree->d_opd;
  const hwy::OpdTree t = {(double *)(d + l.ret), (double *)(d + l.disc), (double *)(d + l.up0), (uint8_t *)(d + l.done),
                          (int32_t *)(d + l.node), (int32_t *)(d + l.gather), (int32_t *)(d + l.scatter), (int32_t *)(d + l.root),
                          (int32_t *)(d + l.act), (uint8_t *)(d + l.created), (uint8_t *)(d + l.child_mask)};
  const hwy::OpdParams p = hwy::opd_params(*params, (int32_t)E, t, work->d_reward, work->d_term, work->d_trunc,
                                           hwy::OpdPlan{d_action, d_value, d_upper, d_sequence, d_expanded});
  // the operations of hwy_opd.h's sequence on the three engines' streams; a failure of a call on `tree` / `work` is reported on
  // `src`, the engine the caller asks
  struct Ops {
    hwy_engine *eng[3];  // by hwy::OpdEngine
    uint8_t *child_mask;
    int after(int waiter, int signaler) { return opd_forward(eng[0], eng[waiter], stream_after(eng[waiter], eng[signaler])); }
    int kernel(const hwy::OpdParams &p) {
      HWY_HIP(eng[0], hwy::launch_opd(p, eng[hwy::OPD_WORK]->stream));
      return HWY_OK;
    }
    int fork(int dst, int src, int32_t branches, const int32_t *src_env) {
      return opd_forward(eng[0], eng[dst], hwy_fork_device(eng[dst], eng[src], branches, src_env));
    }
    int mask() { return opd_forward(eng[0], eng[hwy::OPD_WORK], hwy_action_mask_device(eng[hwy::OPD_WORK], child_mask)); }
    int step(const int32_t *actions) {
      hwy_engine *w = eng[hwy::OPD_WORK];
      return opd_forward(eng[0], w, hwy_step_device(w, actions, w->d_obs, w->d_reward, w->d_term, w->d_trunc, nullptr, nullptr));
    }
  };
  return hwy::opd_expand(p, Ops{{src, tree, work}, t.child_mask});
}

extern "C" int hwy_opd_plan(hwy_engine *src, hwy_engine *tree, hwy_engine *work, const hwy_opd_params *params, int32_t *action, double *value,
                            double *upper, int32_t *sequence, int32_t *expanded) {
  if (int rc = opd_check(src, tree, work, params, action != nullptr, "hwy_opd_plan")) return rc;
  HWY_HIP(src, hipSetDevice(src->device));
  const size_t E = src->cfg.num_envs, X = params->budget / params->n_ids;
  const OpdLayout l = opd_layout(E, params->n_ids, params->nodes, X);
  if (int rc = opd_block(src, tree, work, l)) return rc;
  char *d = tree->d_opd;
  if (int rc = hwy_opd_plan_device(src, tree, work, params, (int32_t *)(d + l.o_action), (double *)(d + l.o_value), (double *)(d + l.o_upper),
                                   (int32_t *)(d + l.o_sequence), (int32_t *)(d + l.o_expanded)))
    return rc;
  HWY_HIP(src, hipMemcpyAsync(action, d + l.o_action, E * 4, hipMemcpyDeviceToHost, work->stream));
  if (value) HWY_HIP(src, hipMemcpyAsync(value, d + l.o_value, E * 8, hipMemcpyDeviceToHost, work->stream));
  if (upper) HWY_HIP(src, hipMemcpyAsync(upper, d + l.o_upper, E * 8, hipMemcpyDeviceToHost, work->stream));
  if (sequence) HWY_HIP(src, hipMemcpyAsync(sequence, d + l.o_sequence, E * X * 4, hipMemcpyDeviceToHost, work->stream));
  if (expanded) HWY_HIP(src, hipMemcpyAsync(expanded, d + l.o_expanded, E * 4, hipMemcpyDeviceToHost, work->stream));
  HWY_HIP(src, hipStreamSynchronize(work->stream));
  if (tree->stream != work->stream) HWY_HIP(src, hipStreamSynchronize(tree->stream));  // (the last scatter)
  return HWY_OK;
}

// ---- action mask (hwy_mask.h) ------------------------------------------------------------------------------------------------------
static int mask_check(hwy_engine *eng, const void *out, const char *who) {
  if (!eng) return HWY_ERR_INVALID_ARG;
  if (!out) return fail(eng, HWY_ERR_INVALID_ARG, std::string(who) + ": mask must be non-NULL");
  const char *why = "";
  if (const int rc = hwy::mask_validate(eng->cfg, &why)) return fail(eng, rc, std::string(who) + ": " + why);
  return HWY_OK;
}

extern "C" int hwy_action_mask_device(hwy_engine *eng, uint8_t *d_mask) {
  if (int rc = mask_check(eng, d_mask, "hwy_action_mask_device")) return rc;
  HWY_HIP(eng, hipSetDevice(eng->device));
  const size_t plane = (size_t)eng->cfg.num_envs * eng->pitch;
  const double *f = eng->d_f64;  // planes: x | y | heading | speed | ...
  const hwy::MaskParams p = hwy::mask_params(eng->cfg, f, f + plane, eng->d_packed, eng->pitch, d_mask);
  HWY_HIP(eng, hwy::launch_mask(p, eng->stream));
  return HWY_OK;
}

extern "C" int hwy_action_mask(hwy_engine *eng, uint8_t *mask) {
  if (int rc = mask_check(eng, mask, "hwy_action_mask")) return rc;
  HWY_HIP(eng, hipSetDevice(eng->device));
  const size_t bytes = num_agent_rows(eng->cfg) * (size_t)hwy::mask_num_ids(eng->cfg);
  if (!eng->d_action_mask) HWY_HIP(eng, hipMalloc((void **)&eng->d_action_mask, bytes));
  if (int rc = hwy_action_mask_device(eng, eng->d_action_mask)) return rc;
  HWY_HIP(eng, hipMemcpyAsync(mask, eng->d_action_mask, bytes, hipMemcpyDeviceToHost, eng->stream));
  HWY_HIP(eng, hipStreamSynchronize(eng->stream));
  return HWY_OK;
}

// ---- SameStep autoreset on the device (hwy_same_step.h) -----------------------------------------------------------------------------
// The body of hwy_step_same_step_device and hwy_step_same_step_continuous_device.  The ids door: d_actions, cp NULL.  The continuous
// door: cp and d_continuous, d_actions NULL -- the act launch goes first, and the step launch runs with no ids on the pair it stored.
// What every SameStep door does once its own arguments (the continuous params, the TimeToCollision params) are accepted and before
// its first launch: hwy_same_step.h's validation, the planes, the mask pointers (what hwy_action_mask_device answers for this
// engine), the device, room for the timing events.
static int same_step_begin(hwy_engine *eng, const char *who, const void *d_actions, const float *d_obs, const double *d_reward,
                           const uint8_t *d_terminated, const uint8_t *d_truncated, const double *d_info_speed, const uint8_t *d_info_crashed,
                           const float *d_final_obs, const double *d_final_info_speed, const uint8_t *d_final_info_crashed,
                           const uint8_t *d_final_mask, uint8_t *d_action_mask, uint8_t *d_final_action_mask) {
  const char *why = "";
  if (const int rc = hwy::same_step_validate(eng->cfg, eng->autoreset != 0, d_final_obs != nullptr, d_final_mask != nullptr, &why))
    return fail(eng, rc, std::string(who) + ": " + why);
  if (!d_actions || !d_obs || !d_reward || !d_terminated || !d_truncated)
    return fail(eng, HWY_ERR_INVALID_ARG, std::string(who) + ": actions/obs/reward/terminated/truncated must be non-NULL");
  if ((d_final_info_speed && !d_info_speed) || (d_final_info_crashed && !d_info_crashed))
    return fail(eng, HWY_ERR_INVALID_ARG, std::string(who) + ": a final info plane needs the info plane it is copied from");
  if (d_action_mask || d_final_action_mask)
    if (int rc = mask_check(eng, d_action_mask ? d_action_mask : d_final_action_mask, who)) return rc;
  HWY_HIP(eng, hipSetDevice(eng->device));
  if (eng->profiling && eng->events_used >= 65536)
    if (int rc = drain_events(eng)) return rc;
  return HWY_OK;
}
static int same_step_enqueue(hwy_engine *eng, const char *who, const int32_t *d_actions, const hwy_continuous_params *cp,
                             const float *d_continuous, float *d_obs, double *d_reward, uint8_t *d_terminated, uint8_t *d_truncated,
                             double *d_info_speed, uint8_t *d_info_crashed, float *d_final_obs, double *d_final_info_speed,
                             uint8_t *d_final_info_crashed, uint8_t *d_final_mask, uint8_t *d_action_mask, uint8_t *d_final_action_mask,
                             bool continuous) {
  if (!eng) return HWY_ERR_INVALID_ARG;
  const char *why = "";
  if (continuous)
    if (const int rc = hwy::act_validate(eng->cfg, cp, &why)) return fail(eng, rc, std::string(who) + ": " + why);
  if (int rc = same_step_begin(eng, who, continuous ? (const void *)d_continuous : (const void *)d_actions, d_obs, d_reward, d_terminated,
                               d_truncated, d_info_speed, d_info_crashed, d_final_obs, d_final_info_speed, d_final_info_crashed, d_final_mask,
                               d_action_mask, d_final_action_mask))
    return rc;
  if (continuous) HWY_HIP(eng, hwy::launch_act_continuous(hwy::act_params(eng->cfg, *cp, d_continuous, eng->d_controls), eng->stream));
  struct Ops {
    hwy_engine *eng;
    StepParams p;  // the full step around the caller's planes: the step launch's and the re-spawn's arguments
    hwy::FinalParams fp;
    uint8_t *action_mask, *final_action_mask;
    int step() { return timed_launch(eng, p); }  // exactly hwy_step_device's launch: it writes done[e]
    int mask(bool final) { return hwy_action_mask_device(eng, final ? final_action_mask : action_mask); }
    int stash() {
      HWY_HIP(eng, hwy::launch_final(fp, eng->stream));
      return HWY_OK;
    }
    int respawn() {
      HWY_HIP(eng, launch_stage(eng, RESPAWN, p));
      return HWY_OK;
    }
  } ops{eng, {}, {}, d_action_mask, d_final_action_mask};
  bind_full_step(eng, ops.p, d_actions, d_obs, d_reward, d_terminated, d_truncated, d_info_speed, d_info_crashed);
  ops.fp = hwy::final_params(eng->cfg, hwy::obs_len(eng->cfg), eng->d_done, d_final_mask, d_obs, d_final_obs, d_info_speed,
                             d_final_info_speed, d_info_crashed, d_final_info_crashed);
  return hwy::same_step_sequence(ops, d_final_action_mask != nullptr, d_action_mask != nullptr);
}
extern "C" int hwy_step_same_step_device(hwy_engine *eng, const int32_t *d_actions, float *d_obs, double *d_reward, uint8_t *d_terminated,
                                         uint8_t *d_truncated, double *d_info_speed, uint8_t *d_info_crashed, float *d_final_obs,
                                         double *d_final_info_speed, uint8_t *d_final_info_crashed, uint8_t *d_final_mask,
                                         uint8_t *d_action_mask, uint8_t *d_final_action_mask) {
  return same_step_enqueue(eng, "hwy_step_same_step_device", d_actions, nullptr, nullptr, d_obs, d_reward, d_terminated, d_truncated,
                           d_info_speed, d_info_crashed, d_final_obs, d_final_info_speed, d_final_info_crashed, d_final_mask, d_action_mask,
                           d_final_action_mask, false);
}

// ---- TimeToCollision observation (hwy_collision_obs.h) ---------------------------------------------------------------------------------
static int ttc_obs_check(hwy_engine *eng, const hwy_ttc_params *params, const void *out, const char *who) {
  if (!eng) return HWY_ERR_INVALID_ARG;
  const char *why = "";
  if (const int rc = hwy::ttc_obs_validate(eng->cfg, params, &why)) return fail(eng, rc, std::string(who) + ": " + why);
  if (!out) return fail(eng, HWY_ERR_INVALID_ARG, std::string(who) + ": obs must be non-NULL");
  return HWY_OK;
}
static hipError_t ttc_obs_launch(const hwy_engine *eng, const hwy_ttc_params &tp, float *d_obs) {
  const size_t plane = (size_t)eng->cfg.num_envs * eng->pitch;
  const double *f = eng->d_f64;  // planes: x | y | heading | speed | ...
  const hwy::CollisionObsParams p = hwy::collision_obs_params(eng->cfg, tp, f, f + 2 * plane, f + 3 * plane, eng->d_packed, eng->pitch, d_obs);
  return hwy::launch_collision_obs(p, (int)num_agent_rows(eng->cfg), eng->stream);
}
// the buffer the step's own observation goes to (a null `obs` would take the step off its shape kernel)
static int door_step_obs(hwy_engine *eng) {
  if (!eng->d_door_step_obs) HWY_HIP(eng, hipMalloc((void **)&eng->d_door_step_obs, num_obs_floats(eng->cfg) * sizeof(float)));
  return HWY_OK;
}

extern "C" int hwy_ttc_observe_device(hwy_engine *eng, const hwy_ttc_params *params, float *d_obs) {
  if (int rc = ttc_obs_check(eng, params, d_obs, "hwy_ttc_observe_device")) return rc;
  HWY_HIP(eng, hipSetDevice(eng->device));
  HWY_HIP(eng, ttc_obs_launch(eng, *params, d_obs));
  return HWY_OK;
}

extern "C" int hwy_ttc_observe(hwy_engine *eng, const hwy_ttc_params *params, float *obs) {
  if (int rc = ttc_obs_check(eng, params, obs, "hwy_ttc_observe")) return rc;
  HWY_HIP(eng, hipSetDevice(eng->device));
  const size_t rows = num_agent_rows(eng->cfg);
  if (!eng->d_ttc_obs) HWY_HIP(eng, hipMalloc((void **)&eng->d_ttc_obs, rows * HWY_COLLISION_OBS_CELLS * sizeof(float)));
  HWY_HIP(eng, ttc_obs_launch(eng, *params, eng->d_ttc_obs));
  HWY_HIP(eng, hipMemcpyAsync(obs, eng->d_ttc_obs, rows * hwy::collision_obs_len(*params) * sizeof(float), hipMemcpyDeviceToHost, eng->stream));
  HWY_HIP(eng, hipStreamSynchronize(eng->stream));
  return HWY_OK;
}

extern "C" int hwy_rollout_ttc_device(hwy_engine *eng, const hwy_ttc_params *params, int32_t k_steps, const int32_t *d_actions, float *d_obs,
                                      double *d_reward, uint8_t *d_terminated, uint8_t *d_truncated, double *d_info_speed,
                                      uint8_t *d_info_crashed) {
  static const char *who = "hwy_rollout_ttc_device";
  if (int rc = ttc_obs_check(eng, params, d_obs, who)) return rc;
  if (k_steps < 1) return fail(eng, HWY_ERR_INVALID_ARG, std::string(who) + ": k_steps must be >= 1");
  if (!d_actions || !d_reward || !d_terminated || !d_truncated)
    return fail(eng, HWY_ERR_INVALID_ARG, std::string(who) + ": actions/reward/terminated/truncated must be non-NULL");
  HWY_HIP(eng, hipSetDevice(eng->device));
  if (int rc = door_step_obs(eng)) return rc;
  struct Ops {
    hwy_engine *eng;
    const hwy_ttc_params *tp;
    const int32_t *actions;
    float *obs;
    double *reward;
    uint8_t *term, *trunc;
    double *speed;
    uint8_t *crashed;
    int step(int32_t k) {  // exactly hwy_step_device's launch on block k
      const size_t E = eng->cfg.num_envs, EA = num_agent_rows(eng->cfg);
      return enqueue_full_step(eng, actions + k * EA, eng->d_door_step_obs, reward + k * EA, term + k * E, trunc + k * E,
                               speed ? speed + k * EA : nullptr, crashed ? crashed + k * EA : nullptr);
    }
    int observe(int32_t k) {
      HWY_HIP(eng, ttc_obs_launch(eng, *tp, obs + (size_t)k * num_agent_rows(eng->cfg) * hwy::collision_obs_len(*tp)));
      return HWY_OK;
    }
  } ops{eng, params, d_actions, d_obs, d_reward, d_terminated, d_truncated, d_info_speed, d_info_crashed};
  return hwy::ttc_obs_rollout_sequence(ops, k_steps);
}

extern "C" int hwy_step_same_step_ttc_device(hwy_engine *eng, const hwy_ttc_params *params, const int32_t *d_actions, float *d_obs,
                                             double *d_reward, uint8_t *d_terminated, uint8_t *d_truncated, double *d_info_speed,
                                             uint8_t *d_info_crashed, float *d_final_obs, double *d_final_info_speed,
                                             uint8_t *d_final_info_crashed, uint8_t *d_final_mask, uint8_t *d_action_mask,
                                             uint8_t *d_final_action_mask) {
  static const char *who = "hwy_step_same_step_ttc_device";
  if (!eng) return HWY_ERR_INVALID_ARG;
  const char *why = "";
  if (const int rc = hwy::ttc_obs_validate(eng->cfg, params, &why)) return fail(eng, rc, std::string(who) + ": " + why);
  if (int rc = same_step_begin(eng, who, d_actions, d_obs, d_reward, d_terminated, d_truncated, d_info_speed, d_info_crashed, d_final_obs,
                               d_final_info_speed, d_final_info_crashed, d_final_mask, d_action_mask, d_final_action_mask))
    return rc;
  if (int rc = door_step_obs(eng)) return rc;
  struct Ops {
    hwy_engine *eng;
    const hwy_ttc_params *tp;
    float *obs;
    StepParams p;  // the full step around the caller's planes, its own observation into the engine's buffer
    hwy::FinalParams fp;
    uint8_t *action_mask, *final_action_mask;
    int step() { return timed_launch(eng, p); }
    int mask(bool final) { return hwy_action_mask_device(eng, final ? final_action_mask : action_mask); }
    int observe() {
      HWY_HIP(eng, ttc_obs_launch(eng, *tp, obs));
      return HWY_OK;
    }
    int stash() {
      HWY_HIP(eng, hwy::launch_final(fp, eng->stream));
      return HWY_OK;
    }
    int respawn() {
      HWY_HIP(eng, launch_stage(eng, RESPAWN, p));
      return HWY_OK;
    }
  } ops{eng, params, d_obs, {}, {}, d_action_mask, d_final_action_mask};
  bind_full_step(eng, ops.p, d_actions, eng->d_door_step_obs, d_reward, d_terminated, d_truncated, d_info_speed, d_info_crashed);
  ops.fp = hwy::final_params(eng->cfg, hwy::collision_obs_len(*params), eng->d_done, d_final_mask, d_obs, d_final_obs, d_info_speed,
                             d_final_info_speed, d_info_crashed, d_final_info_crashed);
  return hwy::ttc_obs_same_step_sequence(ops, d_final_action_mask != nullptr, d_action_mask != nullptr);
}

// ---- Lidar through a door of its own (hwy_lidar_door.h) -----------------------------------------------------------------------------
static int lidar_door_check(hwy_engine *eng, const hwy_lidar_params *params, const void *out, bool rollout, const char *who) {
  if (!eng) return HWY_ERR_INVALID_ARG;
  const char *why = "";
  if (const int rc = hwy::lidar_door_validate(eng->cfg, params, eng->has_state, rollout, &why)) return fail(eng, rc, std::string(who) + ": " + why);
  if (!out) return fail(eng, HWY_ERR_INVALID_ARG, std::string(who) + ": obs must be non-NULL");
  return HWY_OK;
}
static hipError_t lidar_door_launch(const hwy_engine *eng, const hwy_lidar_params &lp, float *d_obs) {
  const size_t plane = (size_t)eng->cfg.num_envs * eng->pitch;
  const double *f = eng->d_f64;  // planes: x | y | heading | speed | ...
  const hwy::LidarDoorParams p = hwy::lidar_door_params(eng->cfg, lp, f, f + plane, f + 2 * plane, f + 3 * plane, eng->d_packed, eng->pitch, d_obs);
  return hwy::launch_lidar_door(p, lp.normalize != 0, (int)num_agent_rows(eng->cfg), eng->stream);
}

extern "C" int hwy_lidar_observe_device(hwy_engine *eng, const hwy_lidar_params *params, float *d_obs) {
  if (int rc = lidar_door_check(eng, params, d_obs, false, "hwy_lidar_observe_device")) return rc;
  HWY_HIP(eng, hipSetDevice(eng->device));
  HWY_HIP(eng, lidar_door_launch(eng, *params, d_obs));
  return HWY_OK;
}

extern "C" int hwy_lidar_observe(hwy_engine *eng, const hwy_lidar_params *params, float *obs) {
  if (int rc = lidar_door_check(eng, params, obs, false, "hwy_lidar_observe")) return rc;
  HWY_HIP(eng, hipSetDevice(eng->device));
  const size_t rows = num_agent_rows(eng->cfg);
  if (!eng->d_lidar_door_obs) HWY_HIP(eng, hipMalloc((void **)&eng->d_lidar_door_obs, rows * HWY_LIDAR_DOOR_MAX_CELLS * 2 * sizeof(float)));
  HWY_HIP(eng, lidar_door_launch(eng, *params, eng->d_lidar_door_obs));
  HWY_HIP(eng, hipMemcpyAsync(obs, eng->d_lidar_door_obs, rows * hwy::lidar_door_len(*params) * sizeof(float), hipMemcpyDeviceToHost, eng->stream));
  HWY_HIP(eng, hipStreamSynchronize(eng->stream));
  return HWY_OK;
}

extern "C" int hwy_rollout_lidar_device(hwy_engine *eng, const hwy_lidar_params *params, int32_t k_steps, const int32_t *d_actions, float *d_obs,
                                        double *d_reward, uint8_t *d_terminated, uint8_t *d_truncated, double *d_info_speed,
                                        uint8_t *d_info_crashed) {
  static const char *who = "hwy_rollout_lidar_device";
  if (int rc = lidar_door_check(eng, params, d_obs, true, who)) return rc;
  if (k_steps < 1) return fail(eng, HWY_ERR_INVALID_ARG, std::string(who) + ": k_steps must be >= 1");
  if (!d_actions || !d_reward || !d_terminated || !d_truncated)
    return fail(eng, HWY_ERR_INVALID_ARG, std::string(who) + ": actions/reward/terminated/truncated must be non-NULL");
  HWY_HIP(eng, hipSetDevice(eng->device));
  if (int rc = door_step_obs(eng)) return rc;
  struct Ops {
    hwy_engine *eng;
    const hwy_lidar_params *lp;
    const int32_t *actions;
    float *obs;
    double *reward;
    uint8_t *term, *trunc;
    double *speed;
    uint8_t *crashed;
    int step(int32_t k) {  // exactly hwy_step_device's launch on block k
      const size_t E = eng->cfg.num_envs, EA = num_agent_rows(eng->cfg);
      return enqueue_full_step(eng, actions + k * EA, eng->d_door_step_obs, reward + k * EA, term + k * E, trunc + k * E,
                               speed ? speed + k * EA : nullptr, crashed ? crashed + k * EA : nullptr);
    }
    int observe(int32_t k) {
      HWY_HIP(eng, lidar_door_launch(eng, *lp, obs + (size_t)k * num_agent_rows(eng->cfg) * hwy::lidar_door_len(*lp)));
      return HWY_OK;
    }
  } ops{eng, params, d_actions, d_obs, d_reward, d_terminated, d_truncated, d_info_speed, d_info_crashed};
  return hwy::lidar_door_rollout_sequence(ops, k_steps);
}

// ---- continuous throttle and steering of a direct-control engine (hwy_act.h) -------------------------------------------------------
// what every continuous entry point checks first: the engine, the params (hwy_act.h: act_validate) and the action pointer
static int act_check(hwy_engine *eng, const hwy_continuous_params *cp, const void *actions, const char *who) {
  if (!eng) return HWY_ERR_INVALID_ARG;
  const char *why = "";
  if (const int rc = hwy::act_validate(eng->cfg, cp, &why)) return fail(eng, rc, std::string(who) + ": " + why);
  if (!actions) return fail(eng, HWY_ERR_INVALID_ARG, std::string(who) + ": actions must be non-NULL");
  return HWY_OK;
}
// the host-pointer doors: a NaN or an infinity is no action of the Box (the device forms leave such a row's stored pair as it is)
static int act_check_finite(hwy_engine *eng, const hwy_continuous_params *cp, const float *actions, size_t steps, const char *who) {
  if (!hwy::act_all_finite(actions, steps * num_agent_rows(eng->cfg) * (size_t)hwy::act_size(*cp)))
    return fail(eng, HWY_ERR_ACTION, std::string(who) + ": a continuous action must be finite");
  return HWY_OK;
}
static size_t act_floats(const hwy_engine *eng, const hwy_continuous_params &cp) { return num_agent_rows(eng->cfg) * (size_t)hwy::act_size(cp); }

extern "C" int hwy_act_continuous_device(hwy_engine *eng, const hwy_continuous_params *params, const float *d_actions) {
  if (int rc = act_check(eng, params, d_actions, "hwy_act_continuous_device")) return rc;
  HWY_HIP(eng, hipSetDevice(eng->device));
  HWY_HIP(eng, hwy::launch_act_continuous(hwy::act_params(eng->cfg, *params, d_actions, eng->d_controls), eng->stream));
  return HWY_OK;
}

// the device block the host-pointer doors stage their actions in: the head of the rollout block (grown on demand)
static int act_stage(hwy_engine *eng, const float *actions, size_t bytes, const float **d_out) {
  if (bytes > eng->roll_bytes) {
    HWY_HIP(eng, hipStreamSynchronize(eng->stream));
    if (eng->d_roll) (void)hipFree(eng->d_roll);
    eng->d_roll = nullptr;
    eng->roll_bytes = 0;
    HWY_HIP(eng, hipMalloc((void **)&eng->d_roll, bytes));
    eng->roll_bytes = bytes;
  }
  HWY_HIP(eng, hipMemcpyAsync(eng->d_roll, actions, bytes, hipMemcpyHostToDevice, eng->stream));
  *d_out = (const float *)eng->d_roll;
  return HWY_OK;
}

extern "C" int hwy_act_continuous(hwy_engine *eng, const hwy_continuous_params *params, const float *actions) {
  static const char *who = "hwy_act_continuous";
  if (int rc = act_check(eng, params, actions, who)) return rc;
  if (int rc = act_check_finite(eng, params, actions, 1, who)) return rc;
  HWY_HIP(eng, hipSetDevice(eng->device));
  const float *d_actions = nullptr;
  if (int rc = act_stage(eng, actions, act_floats(eng, *params) * sizeof(float), &d_actions)) return rc;
  if (int rc = hwy_act_continuous_device(eng, params, d_actions)) return rc;
  HWY_HIP(eng, hipStreamSynchronize(eng->stream));
  return HWY_OK;
}

extern "C" int hwy_step_continuous_device(hwy_engine *eng, const hwy_continuous_params *params, const float *d_actions, float *d_obs,
                                          double *d_reward, uint8_t *d_terminated, uint8_t *d_truncated, double *d_info_speed,
                                          uint8_t *d_info_crashed) {
  if (int rc = act_check(eng, params, d_actions, "hwy_step_continuous_device")) return rc;
  if (!d_obs || !d_reward || !d_terminated || !d_truncated)
    return fail(eng, HWY_ERR_INVALID_ARG, "hwy_step_continuous_device: obs/reward/terminated/truncated must be non-NULL");
  HWY_HIP(eng, hipSetDevice(eng->device));
  HWY_HIP(eng, hwy::launch_act_continuous(hwy::act_params(eng->cfg, *params, d_actions, eng->d_controls), eng->stream));
  return enqueue_full_step(eng, nullptr, d_obs, d_reward, d_terminated, d_truncated, d_info_speed, d_info_crashed);
}

extern "C" int hwy_step_same_step_continuous_device(hwy_engine *eng, const hwy_continuous_params *params, const float *d_actions,
                                                    float *d_obs, double *d_reward, uint8_t *d_terminated, uint8_t *d_truncated,
                                                    double *d_info_speed, uint8_t *d_info_crashed, float *d_final_obs,
                                                    double *d_final_info_speed, uint8_t *d_final_info_crashed, uint8_t *d_final_mask,
                                                    uint8_t *d_action_mask, uint8_t *d_final_action_mask) {
  return same_step_enqueue(eng, "hwy_step_same_step_continuous_device", nullptr, params, d_actions, d_obs, d_reward, d_terminated,
                           d_truncated, d_info_speed, d_info_crashed, d_final_obs, d_final_info_speed, d_final_info_crashed, d_final_mask,
                           d_action_mask, d_final_action_mask, true);
}

extern "C" int hwy_rollout_continuous_device(hwy_engine *eng, const hwy_continuous_params *params, int32_t k_steps, const float *d_actions,
                                             float *d_obs, double *d_reward, uint8_t *d_terminated, uint8_t *d_truncated,
                                             double *d_info_speed, uint8_t *d_info_crashed) {
  static const char *who = "hwy_rollout_continuous_device";
  if (int rc = act_check(eng, params, d_actions, who)) return rc;
  if (k_steps < 1) return fail(eng, HWY_ERR_INVALID_ARG, std::string(who) + ": k_steps must be >= 1");
  if (!d_obs || !d_reward || !d_terminated || !d_truncated)
    return fail(eng, HWY_ERR_INVALID_ARG, std::string(who) + ": obs/reward/terminated/truncated must be non-NULL");
  HWY_HIP(eng, hipSetDevice(eng->device));
  // k_steps x (act launch + step launch) on block k of every plane: step k's stored pair comes from action k, so the steps cannot
  // share a launch without a rollout kernel that reads the float buffer.  The launches are those of k_steps
  // hwy_step_continuous_device calls: the same results by construction.
  const size_t E = eng->cfg.num_envs, EA = num_agent_rows(eng->cfg), n_obs = num_obs_floats(eng->cfg), n_a = act_floats(eng, *params);
  for (size_t k = 0; k < (size_t)k_steps; ++k) {
    HWY_HIP(eng, hwy::launch_act_continuous(hwy::act_params(eng->cfg, *params, d_actions + k * n_a, eng->d_controls), eng->stream));
    if (int rc = enqueue_full_step(eng, nullptr, d_obs + k * n_obs, d_reward + k * EA, d_terminated + k * E, d_truncated + k * E,
                                   d_info_speed ? d_info_speed + k * EA : nullptr, d_info_crashed ? d_info_crashed + k * EA : nullptr))
      return rc;
  }
  return HWY_OK;
}

// the host-pointer doors (hwy_step_continuous: one step): the validated actions up, hwy_rollout_continuous_device, the outputs down
static int rollout_continuous_host(hwy_engine *eng, const char *who, const hwy_continuous_params *params, int32_t k_steps,
                                   const float *actions, float *obs, double *reward, uint8_t *terminated, uint8_t *truncated,
                                   double *info_speed, uint8_t *info_crashed) {
  if (int rc = act_check(eng, params, actions, who)) return rc;
  if (k_steps < 1) return fail(eng, HWY_ERR_INVALID_ARG, std::string(who) + ": k_steps must be >= 1");
  if (!obs || !reward || !terminated || !truncated)
    return fail(eng, HWY_ERR_INVALID_ARG, std::string(who) + ": obs/reward/terminated/truncated must be non-NULL");
  if (int rc = act_check_finite(eng, params, actions, (size_t)k_steps, who)) return rc;
  HWY_HIP(eng, hipSetDevice(eng->device));
  return rollout_through_host(eng, (size_t)k_steps, actions, act_floats(eng, *params) * sizeof(float), obs, reward, terminated, truncated,
                              info_speed, info_crashed,
                              [&](const void *d_act, float *d_obs, double *d_rew, uint8_t *d_term, uint8_t *d_trunc, double *d_spd, uint8_t *d_crash) {
                                return hwy_rollout_continuous_device(eng, params, k_steps, (const float *)d_act, d_obs, d_rew, d_term, d_trunc,
                                                                     d_spd, d_crash);
                              });
}
extern "C" int hwy_rollout_continuous(hwy_engine *eng, const hwy_continuous_params *params, int32_t k_steps, const float *actions,
                                      float *obs, double *reward, uint8_t *terminated, uint8_t *truncated, double *info_speed,
                                      uint8_t *info_crashed) {
  return rollout_continuous_host(eng, "hwy_rollout_continuous", params, k_steps, actions, obs, reward, terminated, truncated, info_speed,
                                 info_crashed);
}
extern "C" int hwy_step_continuous(hwy_engine *eng, const hwy_continuous_params *params, const float *actions, float *obs, double *reward,
                                   uint8_t *terminated, uint8_t *truncated, double *info_speed, uint8_t *info_crashed) {
  return rollout_continuous_host(eng, "hwy_step_continuous", params, 1, actions, obs, reward, terminated, truncated, info_speed, info_crashed);
}

// ---- the float door into fork / rollout / score, and the CEM planner on top of it (hwy_cem.h) --------------------------------------
extern "C" int hwy_score_rollout_continuous(hwy_engine *eng, const hwy_continuous_params *params, int32_t k_steps, int32_t branches,
                                            double gamma, const float *actions, double *reward, uint8_t *terminated, uint8_t *truncated,
                                            double *ret, int32_t *best_branch) {
  static const char *who = "hwy_score_rollout_continuous";
  if (int rc = act_check(eng, params, actions, who)) return rc;
  const char *why = "";
  if (const int rc = hwy::score_validate(eng->cfg, k_steps, branches, gamma, false, true, false, false, &why))
    return fail(eng, rc, std::string(who) + ": " + why);
  if (int rc = act_check_finite(eng, params, actions, (size_t)k_steps, who)) return rc;  // before anything is simulated
  const size_t n_row = num_agent_rows(eng->cfg), n_obs = num_obs_floats(eng->cfg), n_a = act_floats(eng, *params);
  const size_t EB = eng->cfg.num_envs, K = (size_t)k_steps, E = EB / branches, A = eng->cfg.num_agents;
  HWY_HIP(eng, hipSetDevice(eng->device));
  auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  const size_t o_act = 0, o_rew = up(K * n_a * 4), o_obs = o_rew + up(K * n_row * 8), o_term = o_obs + up(K * n_obs * 4),
               o_trunc = o_term + up(K * EB), o_ret = o_trunc + up(K * EB), o_bb = o_ret + up(n_row * 8), total = o_bb + up(E * A * 4);
  if (total > eng->roll_bytes) {
    HWY_HIP(eng, hipStreamSynchronize(eng->stream));
    if (eng->d_roll) (void)hipFree(eng->d_roll);
    eng->d_roll = nullptr;
    eng->roll_bytes = 0;
    HWY_HIP(eng, hipMalloc((void **)&eng->d_roll, total));
    eng->roll_bytes = total;
  }
  char *d = eng->d_roll;
  HWY_HIP(eng, hipMemcpyAsync(d + o_act, actions, K * n_a * 4, hipMemcpyHostToDevice, eng->stream));
  if (int rc = hwy_rollout_continuous_device(eng, params, k_steps, (const float *)(d + o_act), (float *)(d + o_obs), (double *)(d + o_rew),
                                             (uint8_t *)(d + o_term), (uint8_t *)(d + o_trunc), nullptr, nullptr))
    return rc;
  if (int rc = hwy_score_device(eng, k_steps, branches, gamma, nullptr, (const double *)(d + o_rew), (const uint8_t *)(d + o_term),
                                (const uint8_t *)(d + o_trunc), (double *)(d + o_ret), nullptr, nullptr, (int32_t *)(d + o_bb)))
    return rc;
  if (reward) HWY_HIP(eng, hipMemcpyAsync(reward, d + o_rew, K * n_row * 8, hipMemcpyDeviceToHost, eng->stream));
  if (terminated) HWY_HIP(eng, hipMemcpyAsync(terminated, d + o_term, K * EB, hipMemcpyDeviceToHost, eng->stream));
  if (truncated) HWY_HIP(eng, hipMemcpyAsync(truncated, d + o_trunc, K * EB, hipMemcpyDeviceToHost, eng->stream));
  if (ret) HWY_HIP(eng, hipMemcpyAsync(ret, d + o_ret, n_row * 8, hipMemcpyDeviceToHost, eng->stream));
  if (best_branch) HWY_HIP(eng, hipMemcpyAsync(best_branch, d + o_bb, E * A * 4, hipMemcpyDeviceToHost, eng->stream));
  HWY_HIP(eng, hipStreamSynchronize(eng->stream));
  return HWY_OK;
}

static int cem_check(hwy_engine *src, hwy_engine *work, const hwy_continuous_params *cp, const hwy_cem_params *params, bool has_action,
                     const char *who) {
  if (!src) return HWY_ERR_INVALID_ARG;
  if (!work) return fail(src, HWY_ERR_INVALID_ARG, std::string(who) + ": work is NULL");
  if (src == work) return fail(src, HWY_ERR_INVALID_ARG, std::string(who) + ": src and work must be two engines");
  const char *why = "";
  if (const int rc = hwy::cem_validate(src->cfg, work->cfg, cp, params, has_action, &why)) return fail(src, rc, std::string(who) + ": " + why);
  if (work->autoreset) return fail(src, HWY_ERR_INVALID_ARG, std::string(who) + ": work must run with auto-reset off");
  if (work->device != src->device) return fail(src, HWY_ERR_INVALID_ARG, std::string(who) + ": the two engines are on different devices");
  return HWY_OK;
}

// the block of `work` that holds the planner's arrays: actions f32 [K][EB][size], the rollout's reward f64 [K][EB] | obs | terminated |
// truncated [K][EB], ret f64 [EB], mean | std f64 [E][K][size], best_return f64 [E], best_sequence f32 [E][K][size], then the host
// form's: init_mean f64 [E][K][size], action f32 [E][size], noise f64 | samples f32 [I][E][B][K][size] | elites i32 [I][E][M] (when
// asked for)
struct CemLayout {
  size_t act, rew, obs, term, trunc, ret, mean, sd, best_ret, best_seq, init_mean, action, noise, samples, elites, total;
};
static CemLayout cem_layout(const hwy_engine *work, size_t E, size_t B, size_t K, size_t size, size_t I, size_t M, bool debug) {
  auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  const size_t EB = E * B, cols = E * K * size, dbg = debug ? I * EB * K * size : 0;
  CemLayout l;
  l.act = 0; l.rew = up(K * EB * size * 4); l.obs = l.rew + up(K * EB * 8); l.term = l.obs + up(K * num_obs_floats(work->cfg) * 4);
  l.trunc = l.term + up(K * EB); l.ret = l.trunc + up(K * EB); l.mean = l.ret + up(EB * 8); l.sd = l.mean + up(cols * 8);
  l.best_ret = l.sd + up(cols * 8); l.best_seq = l.best_ret + up(E * 8); l.init_mean = l.best_seq + up(cols * 4);
  l.action = l.init_mean + up(cols * 8); l.noise = l.action + up(E * size * 4); l.samples = l.noise + up(dbg * 8);
  l.elites = l.samples + up(dbg * 4);
  l.total = l.elites + up(debug ? I * E * M * 4 : 0);
  return l;
}
static int cem_block(hwy_engine *src, hwy_engine *work, const CemLayout &l) {
  if (l.total <= work->cem_bytes) return HWY_OK;
  HWY_HIP(src, hipStreamSynchronize(work->stream));  // (a smaller block may still be in use)
  if (work->d_cem) (void)hipFree(work->d_cem);
  work->d_cem = nullptr;
  work->cem_bytes = 0;
  HWY_HIP(src, hipMalloc((void **)&work->d_cem, l.total));
  work->cem_bytes = l.total;
  return HWY_OK;
}

extern "C" int hwy_cem_plan_device(hwy_engine *src, hwy_engine *work, const hwy_continuous_params *params, const hwy_cem_params *cem,
                                   const double *d_init_mean, float *d_action, double *d_best_return, double *d_mean, double *d_std,
                                   float *d_best_sequence, double *d_noise, float *d_samples, int32_t *d_elites) {
  if (int rc = cem_check(src, work, params, cem, d_action != nullptr, "hwy_cem_plan_device")) return rc;
  HWY_HIP(src, hipSetDevice(src->device));
  const size_t E = src->cfg.num_envs, B = cem->population, K = cem->horizon, size = hwy::act_size(*params), I = cem->iterations;
  // (a block laid out for the host form's debug arrays stays valid: the planner's own arrays come first in either layout)
  const CemLayout l = cem_layout(work, E, B, K, size, I, (size_t)cem->elites, false);
  if (int rc = cem_block(src, work, l)) return rc;
  char *d = work->d_cem;
  const hwy::CemArrays a = {(float *)(d + l.act), d_init_mean, d_mean ? d_mean : (double *)(d + l.mean), d_std ? d_std : (double *)(d + l.sd),
                            d_noise, d_samples, d_best_return ? d_best_return : (double *)(d + l.best_ret),
                            d_best_sequence ? d_best_sequence : (float *)(d + l.best_seq), d_action, d_elites};
  const hwy::CemParams p = hwy::cem_params(*cem, *params, (int32_t)E, a, (const double *)(d + l.ret));
  // the operations of hwy_cem.h's sequence, all on work's stream (the fork orders it behind src's); a failure of a call on `work` is
  // reported on `src`, the engine the caller asks
  struct Ops {
    hwy_engine *src, *work;
    const hwy_continuous_params *cp;
    double gamma;
    char *d;
    CemLayout l;
    int sample(const hwy::CemParams &p) {
      HWY_HIP(src, hwy::launch_cem_sample(p, work->stream));
      return HWY_OK;
    }
    int fork(int32_t branches) { return opd_forward(src, work, hwy_fork_device(work, src, branches, nullptr)); }
    int rollout(int32_t k_steps) {
      return opd_forward(src, work, hwy_rollout_continuous_device(work, cp, k_steps, (const float *)(d + l.act), (float *)(d + l.obs),
                                                                  (double *)(d + l.rew), (uint8_t *)(d + l.term), (uint8_t *)(d + l.trunc),
                                                                  nullptr, nullptr));
    }
    int score(int32_t k_steps, int32_t branches) {
      return opd_forward(src, work, hwy_score_device(work, k_steps, branches, gamma, nullptr, (const double *)(d + l.rew),
                                                     (const uint8_t *)(d + l.term), (const uint8_t *)(d + l.trunc), (double *)(d + l.ret),
                                                     nullptr, nullptr, nullptr));
    }
    int refit(const hwy::CemParams &p) {
      HWY_HIP(src, hwy::launch_cem_refit(p, work->stream));
      return HWY_OK;
    }
  };
  if (int rc = opd_forward(src, work, stream_after(work, src))) return rc;  // (d_init_mean may come from src's stream)
  if (int rc = hwy::cem_iterate(p, Ops{src, work, params, cem->gamma, d, l})) return rc;
  return stream_after(src, work);  // the parent is not stepped before the last fork has read it, nor the action read before it is written
}

extern "C" int hwy_cem_plan(hwy_engine *src, hwy_engine *work, const hwy_continuous_params *params, const hwy_cem_params *cem,
                            const double *init_mean, float *action, double *best_return, double *mean, double *stddev,
                            float *best_sequence, double *noise, float *samples, int32_t *elites) {
  static const char *who = "hwy_cem_plan";
  if (int rc = cem_check(src, work, params, cem, action != nullptr, who)) return rc;
  const size_t E = src->cfg.num_envs, B = cem->population, K = cem->horizon, size = hwy::act_size(*params), I = cem->iterations;
  const size_t cols = E * K * size, dbg = I * E * B * K * size;
  if (init_mean && !hwy::cem_all_finite(init_mean, cols)) return fail(src, HWY_ERR_ACTION, std::string(who) + ": init_mean must be finite");
  HWY_HIP(src, hipSetDevice(src->device));
  const CemLayout l = cem_layout(work, E, B, K, size, I, (size_t)cem->elites, noise || samples || elites);
  if (int rc = cem_block(src, work, l)) return rc;
  char *d = work->d_cem;
  if (init_mean) HWY_HIP(src, hipMemcpyAsync(d + l.init_mean, init_mean, cols * 8, hipMemcpyHostToDevice, work->stream));
  if (int rc = hwy_cem_plan_device(src, work, params, cem, init_mean ? (const double *)(d + l.init_mean) : nullptr, (float *)(d + l.action),
                                   (double *)(d + l.best_ret), (double *)(d + l.mean), (double *)(d + l.sd), (float *)(d + l.best_seq),
                                   noise ? (double *)(d + l.noise) : nullptr, samples ? (float *)(d + l.samples) : nullptr,
                                   elites ? (int32_t *)(d + l.elites) : nullptr))
    return rc;
  HWY_HIP(src, hipMemcpyAsync(action, d + l.action, E * size * 4, hipMemcpyDeviceToHost, work->stream));
  if (best_return) HWY_HIP(src, hipMemcpyAsync(best_return, d + l.best_ret, E * 8, hipMemcpyDeviceToHost, work->stream));
  if (mean) HWY_HIP(src, hipMemcpyAsync(mean, d + l.mean, cols * 8, hipMemcpyDeviceToHost, work->stream));
  if (stddev) HWY_HIP(src, hipMemcpyAsync(stddev, d + l.sd, cols * 8, hipMemcpyDeviceToHost, work->stream));
  if (best_sequence) HWY_HIP(src, hipMemcpyAsync(best_sequence, d + l.best_seq, cols * 4, hipMemcpyDeviceToHost, work->stream));
  if (noise) HWY_HIP(src, hipMemcpyAsync(noise, d + l.noise, dbg * 8, hipMemcpyDeviceToHost, work->stream));
  if (samples) HWY_HIP(src, hipMemcpyAsync(samples, d + l.samples, dbg * 4, hipMemcpyDeviceToHost, work->stream));
  if (elites) HWY_HIP(src, hipMemcpyAsync(elites, d + l.elites, I * E * (size_t)cem->elites * 4, hipMemcpyDeviceToHost, work->stream));
  HWY_HIP(src, hipStreamSynchronize(work->stream));
  return HWY_OK;
}

extern "C" int hwy_sync(hwy_engine *eng) {
  if (!eng) return HWY_ERR_INVALID_ARG;
  HWY_HIP(eng, hipSetDevice(eng->device));
  HWY_HIP(eng, hipStreamSynchronize(eng->stream));
  return HWY_OK;
}
