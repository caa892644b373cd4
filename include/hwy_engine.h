/*
 * hwy_engine.h -- C-ABI of the MI355X-native batched HighwayEnv step engine.
 *
 * The reference (Farama-Foundation/HighwayEnv) has no FFI: its hot path is the
 * Python method seam
 *
 *     AbstractEnv.step      highway_env/envs/common/abstract.py:259-285
 *       AbstractEnv._simulate                              :287-317
 *         ActionType.act    envs/common/action.py:259-260  (DiscreteMetaAction)
 *         Road.act          road/road.py:464-467
 *         Road.step         road/road.py:469-481
 *       KinematicObservation.observe   envs/common/observation.py:234-276
 *       HighwayEnv._reward/_is_terminated/_is_truncated  envs/highway_env.py:100-151
 *     AbstractEnv.reset     envs/common/abstract.py:219-249  (HighwayEnv._create_vehicles :72-98)
 *
 * Each entry point below names the reference interface it replaces.  All
 * functions are extern "C", take plain pointers and sizes, return 0 on success
 * or a negative hwy_status; the message of the last failure on an engine is
 * available through hwy_last_error().  One host thread per engine; calls on one
 * engine must be serialised; engines on different GPUs are independent.
 *
 * Data model.  E environments x N vehicles (vehicle index == position in the
 * reference's Road.vehicles list; controlled vehicles are where
 * HighwayEnv._create_vehicles puts them, index 0 for a single agent).  All
 * floating-point state is f64 like the reference (vehicle/objects.py:43);
 * observations are f32 (observation.py:276).  Host-side arrays are row-major
 * [E][N] (state), [E][A][V][F] (Kinematics obs), [E][A][F][W][H] (OccupancyGrid obs) or
 * [E][A][cells][2] (Lidar obs), [E][A] (actions) unless stated otherwise.
 */
#ifndef HWY_ENGINE_H
#define HWY_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HWY_ABI_VERSION 8

#define HWY_MAX_AGENTS 16
#define HWY_MAX_FEATURES 16
#define HWY_MAX_TARGET_SPEEDS 8
#define HWY_MAX_LANES 16
#define HWY_MAX_VEHICLES 256
#define HWY_MAX_GRID_CELLS 65536
#define HWY_MAX_GLANES 24  /* lanes of a general (any direction / circular) road network: HWY_SCENARIO_INTERSECTION */
#define HWY_MAX_ACTIONS_PER_AXIS 16 /* DiscreteAction(actions_per_axis): points per axis of the throttle x steering table */
#define HWY_MAX_LIDAR_CELLS 64 /* LidarObservation(cells): one lane of a wavefront per cell */
#define HWY_MAX_LIDAR_DOOR_CELLS 256 /* hwy_lidar_params.cells: up to four cells per lane of a wavefront */
#define HWY_MAX_TTC_STEPS 64 /* time cells of the time-to-collision grid (hwy_ttc_params.time_steps) */
#define HWY_MAX_ROUTE 11   /* remaining roads of a planned route kept per vehicle (64-bit route word, 5 bits per road) */

typedef enum hwy_status {
  HWY_OK = 0,
  HWY_ERR_INVALID_ARG = -1,
  HWY_ERR_HIP = -2,
  HWY_ERR_UNSUPPORTED = -3,
  HWY_ERR_NO_DEVICE = -4,
  HWY_ERR_ACTION = -5 /* action id outside the configured table: the reference raises KeyError (DiscreteMetaAction,
                         action.py:260) or IndexError (DiscreteAction, action.py:195) */
} hwy_status;

/* per-vehicle flag bits (hwy_state.flags) */
enum {
  HWY_F_CRASHED = 1,          /* RoadObject.crashed            vehicle/objects.py:64  */
  HWY_F_HAS_IMPACT = 2,       /* Vehicle.impact is not None    vehicle/kinematics.py:47,145-148 */
  HWY_F_CHECK_COLLISIONS = 4, /* RoadObject.check_collisions   vehicle/objects.py:61 (HighwayEnvFast clears it, highway_env.py:177-182) */
  HWY_F_CONTROLLED = 8,       /* MDPVehicle (ego) instead of IDMVehicle */
  /* road-network scenarios (hwy_config.scenario != HWY_SCENARIO_HIGHWAY) only: */
  HWY_F_OBSTACLE = 16,        /* the slot is an Obstacle of Road.objects (vehicle/objects.py:215-222): 2 m x 2 m,
                                 never acts or moves; slots of obstacles come AFTER every vehicle slot, like
                                 `self.vehicles + self.objects` in road.py:531 */
  HWY_F_ABSENT = 32,          /* empty slot: MergeGenericEnv's rejection-sampled spawn (merge_env.py:336-352)
                                 creates a different number of vehicles per episode; IntersectionEnv clears and spawns
                                 vehicles between policy steps (intersection_env.py:136-140) */
  HWY_F_YIELDING = 64         /* HWY_SCENARIO_INTERSECTION: RegulatedRoad made the vehicle yield (is_yielding,
                                 road/regulation.py:60-68); YIELD_DURATION is 0, so yield_timer is never read */
};

/* config flag bits (hwy_config.flags) */
enum {
  HWY_C_NORMALIZE_REWARD = 1, /* config["normalize_reward"]   highway_env.py:108-116 */
  HWY_C_OFFROAD_TERMINAL = 2, /* config["offroad_terminal"]   highway_env.py:141-147 */
  HWY_C_OBS_ABSOLUTE = 4,     /* KinematicObservation.absolute      observation.py:167 */
  HWY_C_OBS_NORMALIZE = 8,    /* KinematicObservation.normalize     observation.py:169 */
  HWY_C_OBS_CLIP = 16,        /* KinematicObservation.clip          observation.py:170 */
  HWY_C_OBS_SEE_BEHIND = 32,  /* KinematicObservation.see_behind    observation.py:171 */
  HWY_C_EGO_ONLY_COLLISIONS = 64, /* HighwayEnvFast: spawned traffic has check_collisions=False (highway_env.py:177-182) */
  HWY_C_GRID_ALIGN = 128,     /* OccupancyGridObservation.align_to_vehicle_axes  observation.py:294,431-435 */
  HWY_C_CONNECTED_LANES = 512, /* Road.neighbour_vehicles_connected_lanes (road.py:483-547; merge-v1, merge-generic-v1): the
                                 leader / follower search on a lane also looks at hwy_lane.connected */
  HWY_C_OBS_UNSORTED = 1024,  /* KinematicObservation(order="shuffled") (observation.py:245,273-274): close_objects_to(sort=False)
                                 keeps the first vehicles_count - 1 eligible objects in LIST order; the shuffle of the rows
                                 itself draws from env.np_random and is done by the host side of the binding */
  HWY_C_OBS_VEHICLES_ONLY = 2048, /* KinematicObservation(include_obstacles=False) (observation.py:172,246): objects of
                                 Road.objects (the merge scenarios' Obstacle) are not observed */
  HWY_C_OBS_INTENTIONS = 4096, /* KinematicObservation(observe_intentions=True) (observation.py:171,253): the cos_d / sin_d features
                                (Vehicle.destination_direction, kinematics.py:211-235) of the OTHER vehicles too, not only the
                                observer's own; only vehicles with a route have a destination (HWY_SCENARIO_INTERSECTION) */
  HWY_C_GRID_IMAGE = 8192,    /* OccupancyGridObservation(as_image=True) (observation.py:296,408-409): every cell holds
                                 uint8(((clip(value, -1, 1) + 1) / 2) * 255) -- written as an integer-valued f32, 0 for an empty
                                 (NaN) cell -- instead of the value */
  HWY_C_HOST_TRAFFIC = 256    /* HWY_SCENARIO_INTERSECTION: the HOST clears / spawns vehicles between policy steps (the
                                 reference-stream mode of highwayenv_amd/intersection.py); otherwise the step kernel does
                                 it on Philox draws */
};

/* observation feature ids (Vehicle.to_dict keys, vehicle/kinematics.py:237-261) */
enum {
  HWY_FEAT_PRESENCE = 0, HWY_FEAT_X, HWY_FEAT_Y, HWY_FEAT_VX, HWY_FEAT_VY, HWY_FEAT_HEADING,
  HWY_FEAT_COS_H, HWY_FEAT_SIN_H, HWY_FEAT_COS_D, HWY_FEAT_SIN_D, HWY_FEAT_LONG_OFF,
  HWY_FEAT_LAT_OFF, HWY_FEAT_ANG_OFF,
  HWY_FEAT_ON_ROAD, /* OccupancyGrid only: the on-road layer (observation.py:454-484) */
  HWY_FEAT_COUNT
};

/* traffic models (hwy_config.traffic_model): the behaviour class of the non-controlled vehicles, config["other_vehicles_type"]
 * (envs/common/abstract.py:105).  HWY_SCENARIO_HIGHWAY only; the other scenarios take HWY_TRAFFIC_IDM. */
enum {
  HWY_TRAFFIC_IDM = 0,    /* IDMVehicle (vehicle/behavior.py:12-347): IDM + MOBIL, DELTA drawn per vehicle */
  HWY_TRAFFIC_LINEAR = 1  /* LinearVehicle / AggressiveVehicle / DefensiveVehicle (behavior.py:350-585): acceleration and steering
                             linear in 3 + 2 parameters drawn per vehicle (hwy_set_behavior), TIME_WANTED 2.5; the three classes differ
                             only in LANE_CHANGE_MIN_ACC_GAIN (hwy_config.traffic_lc_min_acc_gain) */
};
#define HWY_BEHAVIOR_PARAMS 5 /* per vehicle: ACCELERATION_PARAMETERS[3], STEERING_PARAMETERS[2] (behavior.py:406-416) */

/* ego control (hwy_config.ego_control): what an action id means to a controlled vehicle.  HWY_SCENARIO_HIGHWAY with
 * HWY_TRAFFIC_IDM only takes HWY_EGO_DIRECT. */
enum {
  HWY_EGO_META = 0,  /* DiscreteMetaAction (action.py:199-284): the ego is an MDPVehicle, ids index hwy_config.action_set */
  HWY_EGO_DIRECT = 1 /* DiscreteAction (action.py:165-196), the quantised ContinuousAction: the ego is a plain Vehicle
                        (kinematics.py) -- no target lane, no target speed, no controller -- and id a means acceleration
                        accel_axis[a / n_steer] and steering angle steer_axis[a % n_steer], stored on the vehicle and clipped
                        there frame by frame (Vehicle.clip_actions, kinematics.py:155-168: hwy_set_controls) */
};

/* observation types (hwy_config.obs_type) */
enum {
  HWY_OBS_KINEMATICS = 0,
  HWY_OBS_OCCUPANCY_GRID = 1,
  HWY_OBS_LIDAR = 2 /* LidarObservation (observation.py:678-769), HWY_SCENARIO_HIGHWAY only (every traffic model and ego control
                       of it): obs is f32 [E][A][cells][2] = (distance, relative radial speed) per angular cell.  Traced by a
                       kernel of its own (csrc/hwy_lidar.h) launched on the engine's stream AFTER the step / reset kernel, which
                       runs with a null observation pointer and is otherwise the Kinematics engine's, unchanged:
                         hwy_step / hwy_step_device   the family's step kernel, then the lidar kernel;
                         hwy_reset, hwy_observe       their own work, then the lidar kernel (hwy_observe: the lidar kernel alone);
                         hwy_rollout / _device        k_steps x (step launch + lidar launch), NOT one multi-step launch: step k's
                                                      observation is of the state after step k, which a K-step launch has
                                                      overwritten by its end.  Results equal k_steps calls of hwy_step_device, bit
                                                      for bit, like everywhere else.
                       Auto-reset is next-step (hwy_set_autoreset): the state a step leaves behind is the one its observation is
                       of, also when that step re-spawned the environment.  obs_vehicles / obs_features / obs_feature_ids /
                       obs_range_* are not read (obs_vehicles and obs_features must still be >= 1) */
};

/* scenarios (hwy_config.scenario) */
enum {
  HWY_SCENARIO_HIGHWAY = 0, /* HighwayEnv / HighwayEnvFast: one straight road, lanes_count lanes (highway_env.py:59-70) */
  HWY_SCENARIO_MERGE = 1,   /* MergeEnv: x-aligned road network in hwy_config.net (merge_env.py:90-160), 3 + 1 traffic vehicles */
  HWY_SCENARIO_MERGE_GENERIC = 2, /* MergeGenericEnv (merge_env.py:233-363): same kernels, rejection-sampled spawn */
  HWY_SCENARIO_INTERSECTION = 3   /* IntersectionEnv (intersection_env.py): general lane table hwy_config.gnet, planned
                                     routes, RegulatedRoad, vehicles cleared / spawned between policy steps; meta-actions
                                     are {0: SLOWER, 1: IDLE, 2: FASTER} (intersection_env.py:14) */
};

/*
 * One lane of a GENERAL RoadNetwork (HWY_SCENARIO_INTERSECTION): a StraightLane of any direction (road/lane.py:159-213)
 * or a CircularLane (road/lane.py:311-369).  Table order == iteration order of get_closest_lane_index (road.py:55-71).
 * Every road (from, to) of such a network holds ONE lane, so a planned route is a list of table indices.
 */
typedef struct hwy_glane {
  int32_t kind;                       /* 0 StraightLane, 1 CircularLane */
  int32_t direction;                  /* CircularLane.direction: +1 clockwise, -1 otherwise */
  int32_t priority;                   /* lane.priority (RegulatedRoad.respect_priorities, regulation.py:70-86) */
  int32_t forbidden;
  int32_t from_node, to_node;         /* graph node ids; the lanes leaving a node are the candidates of next_lane */
  int32_t exit_lane;                  /* "il" in lane_index[0] and "o" in lane_index[1] (intersection_env.py:328-331,341-344) */
  int32_t reserved;
  double sx, sy;                      /* StraightLane.start */
  double heading, dirx, diry;         /* StraightLane.heading (arctan2), .direction */
  double cx, cy, radius, start_phase; /* CircularLane.center / radius / start_phase */
  double length, width, speed_limit;
} hwy_glane;

/*
 * One lane of an x-aligned RoadNetwork (road/road.py:16-38): StraightLane (road/lane.py:150-233) when
 * amplitude == 0, else SineLane (road/lane.py:236-283).  direction == (1, 0) for every lane, so
 * local_coordinates(p) = (p.x - x0, p.y - y0 [- amplitude*sin(pulsation*(p.x - x0) + phase)]).
 * Table order == iteration order of RoadNetwork.get_closest_lane_index (road.py:55-71: graph[from][to][id]),
 * which is what its argmin tie-break depends on; lanes of one road (from, to) are consecutive, ordered by id.
 */
typedef struct hwy_lane {
  double x0, y0;                      /* lane.start */
  double length;                      /* |end - start| */
  double width;                       /* AbstractLane.DEFAULT_WIDTH = 4 */
  double amplitude, pulsation, phase; /* SineLane; amplitude == 0 => StraightLane */
  double speed_limit;                 /* lane.speed_limit (20 unless given, lane.py:166) */
  int32_t road;                       /* id of the (from, to) pair */
  int32_t id;                         /* lane id on that road: lane_index[2] */
  int32_t road_first;                 /* table index of lane 0 of the same road */
  int32_t road_lanes;                 /* len(graph[from][to]) */
  int32_t next_first;                 /* table index of lane 0 of the road that starts at `to`, -1 if none */
  int32_t next_lanes;                 /* its lane count (RoadNetwork.next_lane, road.py:73-127) */
  int32_t forbidden;                  /* lane.forbidden (is_reachable_from, lane.py:110-111) */
  int32_t connected;                  /* bit K: lane K is searched together with this lane when HWY_C_CONNECTED_LANES is
                                         set -- the lane itself, lane `id` (else 0) of the successor road, lane `id` (else 0) of
                                         every road ending where this one starts (road.py:508-529) */
} hwy_lane;

/* meta-actions: DiscreteMetaAction.ACTIONS_ALL, envs/common/action.py:204 */
enum { HWY_LANE_LEFT = 0, HWY_IDLE = 1, HWY_LANE_RIGHT = 2, HWY_FASTER = 3, HWY_SLOWER = 4 };
/* hwy_config.action_set: ACTIONS_ALL / ACTIONS_LONGI / ACTIONS_LAT (action.py:204-210) */
enum { HWY_ACTIONS_ALL = 0, HWY_ACTIONS_LONGI = 1, HWY_ACTIONS_LAT = 2 };
/* id in the configured table -> id in ACTIONS_ALL (what the kernels and the oracle act on).  An id outside the table maps
 * to HWY_IDLE in all three tables: hwy_step (host pointers) rejects such ids with HWY_ERR_ACTION before any launch -- the
 * reference's KeyError (action.py:260) -- but hwy_step_device cannot look at device memory without a synchronisation, so an
 * on-GPU policy that emits an out-of-table id gets IDLE, never another table's action. */
#define HWY_ACTION_TO_ALL(set, a)                                                                          \
  ((set) == HWY_ACTIONS_LONGI ? ((a) == 0 ? HWY_SLOWER : ((a) == 2 ? HWY_FASTER : HWY_IDLE))                \
                              : ((unsigned)(a) <= ((set) == HWY_ACTIONS_LAT ? 2u : 4u) ? (a) : HWY_IDLE))
#define HWY_NUM_ACTIONS(set) ((set) == HWY_ACTIONS_ALL ? 5 : 3)

/*
 * Flat POD derived from the reference's config dict
 * (HighwayEnv.default_config, highway_env.py:25-53; AbstractEnv.default_config,
 * abstract.py:101-125; KinematicObservation.__init__, observation.py:160-197).
 */
typedef struct hwy_config {
  int32_t abi_version;                 /* = HWY_ABI_VERSION */
  int32_t num_envs;                    /* E */
  int32_t num_vehicles;                /* N = vehicles_count + controlled_vehicles */
  int32_t num_agents;                  /* A = controlled_vehicles (HWY_SCENARIO_INTERSECTION: 1..4, MultiAgentIntersectionEnv) */
  int32_t agent_index[HWY_MAX_AGENTS]; /* index of each controlled vehicle in the vehicle list (HWY_SCENARIO_INTERSECTION: unused --
                                          its list is re-compacted while an episode runs, so agent a is the a-th slot that carries
                                          HWY_F_CONTROLLED) */
  int32_t lanes_count;                 /* L: lane k is centred on y = k*lane_width (road.py:291-321); merge: highway lanes */
  int32_t frames_per_step;             /* T = simulation_frequency // policy_frequency (abstract.py:289-291) */
  int32_t flags;                       /* HWY_C_* */
  int32_t obs_vehicles;                /* V = observation.vehicles_count */
  int32_t obs_features;                /* F */
  int32_t obs_feature_ids[HWY_MAX_FEATURES];
  int32_t num_target_speeds;           /* MDPVehicle.target_speeds (controller.py:259,287-291) */
  int32_t action_set;                  /* DiscreteMetaAction(longitudinal, lateral) (action.py:204-253): which table the action
                                          ids index -- HWY_ACTIONS_ALL (5 ids), HWY_ACTIONS_LONGI {0 SLOWER, 1 IDLE, 2 FASTER},
                                          HWY_ACTIONS_LAT {0 LANE_LEFT, 1 IDLE, 2 LANE_RIGHT}.  HWY_SCENARIO_INTERSECTION always
                                          uses the longitudinal table (intersection_env.py:14) */
  double target_speeds[HWY_MAX_TARGET_SPEEDS];
  double dt;                           /* 1 / simulation_frequency  (abstract.py:307) */
  double policy_dt;                    /* 1 / policy_frequency      (abstract.py:274) */
  double duration;                     /* config["duration"] [s]    (highway_env.py:149-151) */
  double lane_width;                   /* AbstractLane.DEFAULT_WIDTH = 4 (lane.py:16) */
  double road_length;                  /* 10000 (road.py:296) */
  double speed_limit;                  /* 30 (highway_env.py:63) */
  double collision_reward, right_lane_reward, high_speed_reward; /* highway_env.py:38-45 */
  double reward_speed_range[2];        /* highway_env.py:46 */
  double perception_distance;          /* AbstractEnv.PERCEPTION_DISTANCE = 5*MAX_SPEED (abstract.py:58) */
  double obs_range_x[2], obs_range_y[2], obs_range_vx[2], obs_range_vy[2]; /* observation.py:214-226 */
  /* OccupancyGridObservation (observation.py:279-499): obs is f32 [E][A][F][W][H]; features = obs_feature_ids
   * (to_dict keys + HWY_FEAT_ON_ROAD); features_range in obs_range_* (default: vx, vy only, +-inf = absent) */
  int32_t obs_type;                    /* HWY_OBS_* */
  int32_t grid_shape[2];               /* W, H = floor((grid_size[:,1] - grid_size[:,0]) / grid_step) */
  int32_t reserved1;
  double grid_min[2];                  /* grid_size[:,0] */
  double grid_step[2];                 /* grid_step */
  /* road-network scenarios (ABI v3).  scenario == HWY_SCENARIO_HIGHWAY ignores everything below. */
  int32_t scenario;                    /* HWY_SCENARIO_* */
  int32_t net_lanes;                   /* entries used in net[] (<= HWY_MAX_LANES) */
  int32_t merge_lane;                  /* table index of ("b","c",2) -- literally id 2, merge_env.py:72 -- whose vehicles
                                          pay the altruistic penalty of MergeEnv._rewards (:68-75); -1 if absent */
  int32_t reserved2;
  double merge_end_x;                  /* _is_terminated: ego x > 370 (merge_env.py:79) / end_position (:369) */
  double merging_speed_reward;         /* merge_env.py:35 */
  double lane_change_reward;           /* merge_env.py:36 */
  hwy_lane net[HWY_MAX_LANES];
  /* HWY_SCENARIO_INTERSECTION (ABI v4) */
  int32_t gnet_lanes;                  /* entries used in gnet[] */
  int32_t initial_vehicle_count;       /* config["initial_vehicle_count"] (device reset, intersection_env.py:232-290) */
  int32_t destination;                 /* k of config["destination"] == "o" + k (the ego's route, intersection_env.py:262-275);
                                          -1: config["destination"] is None -- "o" + str(np_random.integers(1, 4)) per episode
                                          (:295-297), drawn by the device reset on its own counter-based stream */
  int32_t reserved3;
  int32_t access_lane[4];              /* table index of ("o" + k, "ir" + k, 0): where _spawn_vehicle puts new traffic */
  int32_t exit_of[4];                  /* table index of ("il" + k, "o" + k, 0): the last road of a route to "o" + k */
  double spawn_probability;            /* config["spawn_probability"] */
  double arrived_reward;               /* config["arrived_reward"] */
  double idm_distance_wanted, idm_time_wanted, idm_comfort_acc_max, idm_comfort_acc_min; /* set on the vehicle class by
                                          IntersectionEnv._make_vehicles (intersection_env.py:243-247): 7, 1.5, 6, -3 */
  hwy_glane gnet[HWY_MAX_GLANES];
  int64_t gnet_routes[HWY_MAX_GLANES][4]; /* ControlledVehicle.plan_route_to("o" + k) (controller.py:71-87) for a vehicle on lane L:
                                          the route word (hwy_state.route encoding) of the roads AFTER L on the shortest path from
                                          L's end node to "o" + k -- RoadNetwork.shortest_path (road.py:159-188: breadth-first,
                                          neighbours in sorted name order), planned by the host once per network; length 0 = no path */
  /* Tuning (ABI v5; 0 everywhere = the engine's own choice).  These replace the process-global environment variables
   * earlier builds read with getenv: a knob now belongs to ONE engine and is part of its documented configuration.
   * None of them changes any result (tests/test_engine_parity.py, tests/test_ix_parity.py compare the variants). */
  int32_t tune_block_kernel;           /* 0: the engine's choice -- one wavefront per environment for N <= 128 (hwy_wave.h for N <= 64,
                                          hwy_wave2.h with two vehicles per thread for 64 < N <= 128 and the Kinematics observation), the
                                          generic workgroup kernel (hwy_device.h) beyond; 1: the workgroup kernel everywhere; 2: the
                                          one-wavefront kernels wherever they exist (hwy_wave2.h with three / four vehicles per thread
                                          for N <= 192 / 256: bit-identical, measured slower than the workgroup kernel there).
                                          HWY_TRAFFIC_LINEAR: hwy_wave.h for N <= 64 unless 1, the workgroup kernel beyond (hwy_wave2.h
                                          is IDM-only: 2 is the engine's choice) */
  int32_t tune_waves_per_eu;           /* 1..4: register-allocation variant (resident wavefronts per SIMD) of the step kernel;
                                          no effect where the wide kernel runs (64 < N <= 128, Kinematics: one build, hwy_wave2.h) */
  int32_t tune_ix_no_helpers;          /* 1: HWY_SCENARIO_INTERSECTION with N <= 32 runs 32-thread workgroups (no helper lanes) */
  int32_t tune_ix_no_prewarm;          /* 1: HWY_SCENARIO_INTERSECTION auto-resets run their warm-up frames inline */
  int32_t tune_extra_lds;              /* bytes of dynamic LDS per workgroup of the one-wavefront step kernel (<= 65536):
                                          fewer resident wavefronts per SIMD, the rest dispatched as wavefronts retire */
  int32_t tune_prio_shift;             /* one-wavefront step kernels: wavefronts sharing a SIMD take turns at the top issue
                                          priority (s_setprio), a turn lasting 2^shift clock ticks of s_memtime for
                                          1 <= shift <= 30, or shift x 64 ticks for 64 <= shift <= 2^20 (turn lengths
                                          between the powers of two: the optimum is sharp, profiles/r05_history.md);
                                          -1 = off (hardware order: oldest wavefront first), 0 = the engine's default
                                          (a turn of ~7 us for the 5 frames of highway-fast-v0, longer with more frames)
                                          when the whole grid of the step kernel is resident at once (occupancy x
                                          compute units >= num_envs), else off */
  int32_t tune_ix_prewarm_frames;      /* HWY_SCENARIO_INTERSECTION auto-reset: warm-up frames of the NEXT episode advanced per
                                          launch by the pre-warming workgroup of an environment (0 = a third of frames_per_step) */
  int32_t tune_reserved[1];
  /* Traffic model (ABI v6).  The Linear family runs on the one-wavefront kernel (hwy_wave.h) for N <= 64 and on the
   * workgroup kernel (hwy_device.h) beyond; the two-vehicles-per-thread kernel (hwy_wave2.h) exists for HWY_TRAFFIC_IDM only. */
  int32_t traffic_model;               /* HWY_TRAFFIC_* */
  int32_t reserved4;
  double traffic_lc_min_acc_gain;      /* LANE_CHANGE_MIN_ACC_GAIN of the traffic class: 0.2 IDM / Linear, 1.0 Aggressive /
                                          Defensive (behavior.py:45,563,575) */
  double traffic_time_wanted;          /* TIME_WANTED of the traffic class: 1.5 IDM, 2.5 the Linear family (behavior.py:34,387);
                                          must be the model's own constant (the kernels compile it in) */
  /* Ego control (ABI v7) */
  int32_t ego_control;                 /* HWY_EGO_* */
  int32_t n_accel, n_steer;            /* HWY_EGO_DIRECT: points on the throttle / steering axis, 1..HWY_MAX_ACTIONS_PER_AXIS each
                                          (1 = the axis is not controlled: its one value is the integer 0 of action.py:147-156);
                                          action ids run over [0, n_accel * n_steer), throttle major like
                                          itertools.product(*axes) (action.py:193-194) */
  int32_t reserved5;
  double accel_axis[HWY_MAX_ACTIONS_PER_AXIS]; /* PHYSICAL values [m/s^2] / [rad]: the host evaluates the reference's own float32 */
  double steer_axis[HWY_MAX_ACTIONS_PER_AXIS]; /* expressions (linspace of the Box bounds, clip, utils.lmap) and widens the results,
                                                  so the kernels do no float32 arithmetic; |steer_axis| <= pi / 3 */
  /* LidarObservation (ABI v8; read when obs_type == HWY_OBS_LIDAR, otherwise ignored) */
  int32_t lidar_cells;                 /* cells, 1..HWY_MAX_LIDAR_CELLS: cell k looks along k * 2 pi / cells */
  int32_t lidar_normalize;             /* normalize: the float32 grid is divided by float32(maximum_range) (observation.py:706-707) */
  double lidar_max_range;              /* maximum_range [m], > 0 and finite: an obstacle whose CENTRE is farther is not traced;
                                          a cell nothing was traced into holds (maximum_range, maximum_range) */
} hwy_config;

/*
 * Struct-of-arrays view of the full simulation state in HOST memory, each
 * vehicle array [E*N] row-major, `time` [E].  Used by hwy_set_state /
 * hwy_get_state (the reference equivalent is reaching into
 * env.road.vehicles[i].{position,heading,speed,lane_index,target_lane_index,
 * crashed,impact,timer,DELTA,target_speed,speed_index}).  Any pointer may be
 * NULL in hwy_get_state (field skipped); all must be non-NULL in hwy_set_state.
 * HWY_SCENARIO_INTERSECTION: for a slot whose flags hold HWY_F_ABSENT only `flags` is meaningful -- the step kernel
 * neither reads nor writes the other planes of an empty slot.
 */
typedef struct hwy_state {
  double *x, *y, *heading, *speed;      /* RoadObject.position/heading/speed     objects.py:42-45 */
  double *timer;                        /* IDMVehicle.timer                      behavior.py:64   */
  double *target_speed;                 /* ControlledVehicle.target_speed        controller.py:47 */
  double *delta;                        /* IDMVehicle.DELTA (randomize_behavior) behavior.py:66-69 */
  double *impact_x, *impact_y;          /* Vehicle.impact (valid iff HWY_F_HAS_IMPACT) */
  int32_t *lane;                        /* lane_index[2]; road-network scenarios: index into hwy_config.net */
  int32_t *target_lane;                 /* target_lane_index[2]; likewise        */
  int32_t *speed_index;                 /* MDPVehicle.speed_index (controlled vehicles) */
  int32_t *flags;                       /* HWY_F_* */
  double *time;                         /* AbstractEnv.time [E]                  abstract.py:274 */
  /* HWY_SCENARIO_INTERSECTION only (ABI v4; ignored / may be NULL otherwise): */
  int64_t *route;                       /* ControlledVehicle.route [E*N]: r_k << 5k for k < len (r_k = gnet index of the k-th
                                           remaining road, 5 bits each, len <= HWY_MAX_ROUTE) | len << 56
                                           (controller.py:71-87, road.py:98-106) */
  int32_t *road_steps;                  /* RegulatedRoad.steps [E] (regulation.py:36-40) */
} hwy_state;

typedef struct hwy_engine hwy_engine; /* opaque */

/* Library-level queries (usable without a GPU). */
int hwy_abi_version(void);
size_t hwy_config_size(void);            /* sizeof(hwy_config): lets a binding check its struct layout */
int hwy_device_count(void);              /* number of visible HIP devices, 0 if none / no driver */
const char *hwy_status_string(int status);

/*
 * Engine lifetime.  Replaces AbstractEnv.__init__ (abstract.py:60-89) for E
 * batched environments.  `stream` is an existing hipStream_t (e.g. PyTorch's
 * current stream) or NULL for an engine-owned stream.  The engine owns all
 * device memory.  Fails with HWY_ERR_NO_DEVICE when no GPU is present -- there
 * is no CPU fallback.
 */
int hwy_create(const hwy_config *cfg, int device, void *stream, hwy_engine **out);
int hwy_destroy(hwy_engine *eng);
const char *hwy_last_error(const hwy_engine *eng); /* eng may be NULL: last hwy_create failure */

/* Parity injection / inspection: H2D and D2H of the whole SoA (synchronous). */
int hwy_set_state(hwy_engine *eng, const hwy_state *host);
int hwy_get_state(hwy_engine *eng, hwy_state *host);

/*
 * Reset.  Replaces AbstractEnv.reset -> HighwayEnv._reset (abstract.py:219-249,
 * highway_env.py:55-98) for the environments whose mask byte is non-zero (NULL
 * mask = all), spawning traffic ON THE DEVICE with the reference's spawn rule
 * (Vehicle.create_random, kinematics.py:50-104) driven by a counter-based RNG
 * keyed by seeds[e].  The random stream is NOT numpy's PCG64 stream; the
 * stream-identical reset is host-side (highwayenv_amd/spawn.py) + hwy_set_state.
 * `ego_spacing`/`vehicles_density`/`initial_lane_id` (-1 = random) are the
 * config entries of the same names.  Writes the first observation if obs != NULL
 * (host pointer, [E][A][V][F] -- the observation's own shape; rows of unmasked envs untouched).
 */
int hwy_reset(hwy_engine *eng, const uint8_t *mask, const uint64_t *seeds, double ego_spacing,
              double vehicles_density, int32_t initial_lane_id, float *obs);

/*
 * One batched policy step == AbstractEnv.step for every environment:
 * T x { action_type.act (first frame); road.act(); road.step(dt) } + observe +
 * reward + terminated + truncated + info{speed,crashed}.
 *   actions    int32 [E][A]   in   DiscreteMetaAction ids (HWY_EGO_DIRECT: DiscreteAction ids)
 *   obs        f32   [E][A][V][F]   (OccupancyGrid: [E][A][F][W][H]; Lidar: [E][A][cells][2])
 *   reward     f64   [E][A]   (single-agent envs: the reference's scalar reward)
 *   terminated u8    [E]
 *   truncated  u8    [E]
 *   info_speed f64   [E][A], info_crashed u8 [E][A]    (may be NULL)
 *              info_crashed bit 0 = vehicle.crashed; the intersection scenario
 *              also sets bit 1 = has_arrived(vehicle) (intersection_env.py:340-345),
 *              so that agents_terminated = (byte != 0) (:119-121)
 * hwy_step takes HOST pointers (H2D actions, kernels, D2H results, synchronises).
 * hwy_step_device takes DEVICE pointers, only enqueues on the engine's stream
 * and does not synchronise -- the path for on-GPU policies, RCCL gathers and
 * the benchmark's HBM-resident timing.  It does NOT validate the action ids
 * (hwy_step does: HWY_ERR_ACTION): an id outside the configured table acts as
 * IDLE (HWY_ACTION_TO_ALL), where the reference raises KeyError.  HWY_EGO_DIRECT: an id outside [0, n_accel * n_steer)
 * leaves the vehicle's stored controls as they are (hwy_step: HWY_ERR_ACTION, the reference's IndexError -- also for a
 * negative id, which Python's list lookup would wrap).
 */
int hwy_step(hwy_engine *eng, const int32_t *actions, float *obs, double *reward,
             uint8_t *terminated, uint8_t *truncated, double *info_speed, uint8_t *info_crashed);
/*
 * k_steps consecutive policy steps with pre-staged actions (abstract.py:259-285, k times): open-loop rollouts, action repeat,
 * planners that score action sequences.  DEVICE pointers, block k of every plane belongs to step k:
 *   d_actions int32 [K][E][A], d_obs f32 [K][E][A][V][F], d_reward f64 [K][E][A], d_terminated / d_truncated u8 [K][E],
 *   d_info_speed f64 [K][E][A], d_info_crashed u8 [K][E][A] (the last two may be NULL).
 * Results are those of k_steps calls of hwy_step_device, bit for bit (auto-reset included: an environment that ends in step k
 * is re-spawned in step k + 1 when hwy_set_autoreset is on).  The k steps run in ONE launch of the scenario's multi-step kernel:
 * the dispatch and, above all, the wait for the slowest SIMD at the end of every step are paid once per call.  (Intersection: the
 * launch holds no pre-warming blocks, an environment that ends in it prepares its next episode inline -- same results.)  Enqueues
 * on the engine's stream, does not synchronise, does not validate action ids (see hwy_step_device).
 * HWY_ERR_INVALID_ARG for k_steps > 1 on an intersection engine configured with HWY_C_HOST_TRAFFIC: there the host runs
 * _clear_vehicles / _spawn_vehicle between policy steps (intersection_env.py:199-203), which a K-step launch would skip.
 */
int hwy_rollout_device(hwy_engine *eng, int32_t k_steps, const int32_t *d_actions, float *d_obs, double *d_reward,
                       uint8_t *d_terminated, uint8_t *d_truncated, double *d_info_speed, uint8_t *d_info_crashed);
/* The same through HOST pointers (validates the action ids like hwy_step: HWY_ERR_ACTION; H2D, launch(es), D2H, synchronises). */
int hwy_rollout(hwy_engine *eng, int32_t k_steps, const int32_t *actions, float *obs, double *reward,
                uint8_t *terminated, uint8_t *truncated, double *info_speed, uint8_t *info_crashed);
int hwy_step_device(hwy_engine *eng, const int32_t *d_actions, float *d_obs, double *d_reward,
                    uint8_t *d_terminated, uint8_t *d_truncated, double *d_info_speed,
                    uint8_t *d_info_crashed);

/*
 * Debug / parity: advance `n_frames` simulation frames (Road.act + Road.step)
 * without observing.  If actions != NULL (host, [E][A]) the meta-action is
 * applied on the first of those frames (abstract.py:294-304).  `time` is not
 * advanced.
 */
int hwy_step_frames(hwy_engine *eng, const int32_t *actions, int32_t n_frames);

/*
 * Per-vehicle behaviour parameters of the Linear traffic family (hwy_config.traffic_model == HWY_TRAFFIC_LINEAR):
 * LinearVehicle.ACCELERATION_PARAMETERS[0..2] and STEERING_PARAMETERS[0..2] as drawn by randomize_behavior (behavior.py:406-416),
 * host array f64 [E][N][HWY_BEHAVIOR_PARAMS] (controlled vehicles: unused).  hwy_reset and the auto-reset draw them on the device;
 * the stream-identical reset of the host side (highwayenv_amd/spawn.py) hands them in with hwy_set_behavior after hwy_set_state.
 * Synchronous.  HWY_ERR_INVALID_ARG on an IDM engine (it has no such parameters).
 */
int hwy_set_behavior(hwy_engine *eng, const double *params);
int hwy_get_behavior(hwy_engine *eng, double *params);

/*
 * The controls stored on the controlled vehicles of a HWY_EGO_DIRECT engine (Vehicle.action, kinematics.py:120-127): the
 * acceleration AFTER Vehicle.clip_actions wrote into it (kinematics.py:155-168: beyond +-MAX_SPEED the stored value becomes
 * min / max(a, bound - speed) and STAYS so for the rest of the policy step; crashed: -1.0 * speed, steering 0) and the steering
 * angle, host arrays f64 [E][A].  They outlive a frame: hwy_step_frames(actions = NULL) continues with them, an action replaces
 * them on the first frame of a step.  Zero after hwy_reset and after an auto-reset (Vehicle.__init__).  Synchronous.
 * HWY_ERR_INVALID_ARG on a HWY_EGO_META engine.
 */
int hwy_set_controls(hwy_engine *eng, const double *acceleration, const double *steering);
int hwy_get_controls(hwy_engine *eng, double *acceleration, double *steering);

/* KinematicObservation / OccupancyGridObservation / LidarObservation.observe for the current state (host pointer out). */
int hwy_observe(hwy_engine *eng, float *obs);

/*
 * Auto-reset (gymnasium vector "next-step" mode): when enabled, an environment
 * that returned terminated|truncated is re-spawned on the device at the start
 * of the following hwy_step* call (its action for that step is ignored and the
 * returned obs is the reset obs, reward 0).  seeds advance per episode.
 */
int hwy_set_autoreset(hwy_engine *eng, int32_t enabled, uint64_t base_seed, double ego_spacing,
                      double vehicles_density, int32_t initial_lane_id);

/*
 * Time-to-collision grid and finite-MDP planner (additive to ABI v8: hwy_config keeps its layout).  Replaces
 * AbstractEnv.to_finite_mdp (envs/common/abstract.py:452-453) -> finite_mdp / compute_ttc_grid / transition_model / clip_position
 * (envs/common/finite_mdp.py:17-203) for every (environment, agent) at once, in a kernel of its own (csrc/hwy_ttc.h) that reads the
 * state planes on the engine's stream after whatever was launched last.
 * HWY_SCENARIO_HIGHWAY with a HWY_EGO_META ego on the five-action table (HWY_ACTIONS_ALL) only; every traffic model, observation
 * type and N.  HWY_ERR_UNSUPPORTED for the other scenarios, for a HWY_EGO_DIRECT ego (a plain Vehicle has no target_speeds: the
 * reference fails there too) and for HWY_ACTIONS_LONGI / _LAT (the reference builds a 5-column reward table next to a 3-column
 * transition table there).
 *   horizon, time_quantization   finite_mdp(env, time_quantization, horizon); to_finite_mdp passes 1 / policy_frequency
 *   time_steps                   int(horizon / time_quantization) as the HOST evaluates the reference's expression
 *                                (finite_mdp.py:122-124), 1..HWY_MAX_TTC_STEPS; HWY_ERR_INVALID_ARG otherwise, or when it is not
 *                                what the two doubles give
 *   gamma                        discount of the value iteration (the reference's agents configure it; finite)
 *   lane_change_reward           config["lane_change_reward"] (finite_mdp.py:72-78; HighwayEnv.default_config: 0)
 * The grid has V = num_target_speeds speeds x L = lanes_count lanes x T = time_steps cells, values exactly 0, 0.5 or 1.
 */
typedef struct hwy_ttc_params {
  double horizon, time_quantization, gamma, lane_change_reward;
  int32_t time_steps;
  int32_t reserved;
} hwy_ttc_params;
/*
 * compute_ttc_grid (finite_mdp.py:104-163) with `vehicle` = every controlled vehicle in turn: d_grid f32 [E][A][V][L][T], DEVICE
 * pointer; enqueues on the engine's stream and does not synchronise (like hwy_step_device).
 */
int hwy_ttc_grid_device(hwy_engine *eng, const hwy_ttc_params *params, float *d_grid);
/* The same into a HOST pointer; synchronises. */
int hwy_ttc_grid(hwy_engine *eng, const hwy_ttc_params *params, float *grid);
/*
 * finite_mdp (finite_mdp.py:17-101) solved exactly: the deterministic MDP over the grid's (speed, lane, time) states with
 * transition_model / clip_position (:166-203), the reward table of :58-83 and the terminal states of :85-90, by one backward sweep
 * over the time axis -- the fixed point of V <- max_a(reward + gamma * where(terminal, 0, V[transition])), bit for bit what numpy
 * computes from the reference's tables.  From state = (speed_index, lane_index[2], 0) of each controlled vehicle (:47-49):
 *   d_action int32 [E][A]     argmax_a Q(state, a), the first maximum (meta-action ids of HWY_ACTIONS_ALL: feed hwy_step_device)
 *   d_q      f64   [E][A][5]  Q(state, .)                      (may be NULL)
 *   d_grid   f32   [E][A][V][L][T]  the grid it planned on      (may be NULL)
 * DEVICE pointers; enqueues on the engine's stream and does not synchronise.
 */
int hwy_mdp_plan_device(hwy_engine *eng, const hwy_ttc_params *params, int32_t *d_action, double *d_q, float *d_grid);
/* The same into HOST pointers (q and grid may be NULL); synchronises. */
int hwy_mdp_plan(hwy_engine *eng, const hwy_ttc_params *params, int32_t *action, double *q, float *grid);

/*
 * TimeToCollision observation (additive to ABI v8: hwy_config keeps its layout and hwy_config.obs_type gains no value -- the
 * observation comes through these entry points, next to whatever obs_type the engine was created with).  Replaces
 * TimeToCollisionObservation.observe (envs/common/observation.py:115-152) for every (environment, agent) at once, in a kernel of its
 * own (csrc/hwy_collision_obs.h) that computes only the window the reference slices out of compute_ttc_grid: float32 [3][3][T],
 *   obs[a][b][t] = 1.0                                                          where lane + b - 1 is outside [0, lanes_count)
 *                = grid[clamp(speed_index + a - 1, 0, V - 1)][lane + b - 1][t]  otherwise
 * with values exactly 0, 0.5 or 1.  `params` is the planner's hwy_ttc_params: horizon, time_quantization (the observation uses
 * 1 / policy_frequency) and time_steps = int(horizon / time_quantization) are read and checked as there; gamma and
 * lane_change_reward are IGNORED by these entry points (any value, NaN included).
 * HWY_SCENARIO_HIGHWAY with a HWY_EGO_META ego only; any action_set, traffic model, obs_type and N.  HWY_ERR_UNSUPPORTED for the
 * other scenarios, for a HWY_EGO_DIRECT ego (a plain Vehicle has no speed_index: the reference raises there too) and for
 * num_target_speeds < 2 (numpy's duplicate fancy index makes the reference return shape (2, 3, T) there); HWY_ERR_INVALID_ARG for a
 * NULL params or output and for the horizon / time_quantization / time_steps the planner rejects.  hwy_last_error has the reason.
 *
 * hwy_ttc_observe_device: the state as it stands, d_obs f32 [E][A][3][3][T], DEVICE pointer; enqueues on the engine's stream and
 * does not synchronise.  hwy_ttc_observe: the same into a HOST pointer; synchronises.
 */
int hwy_ttc_observe_device(hwy_engine *eng, const hwy_ttc_params *params, float *d_obs);
int hwy_ttc_observe(hwy_engine *eng, const hwy_ttc_params *params, float *obs);
/*
 * SameStep autoreset with the window as the observation.  The planes are those of hwy_step_same_step_device, except that d_obs and
 * d_final_obs are [E][A][3][3][T].  In order, on the engine's stream: the step launch; the mask of the terminal state (if
 * d_final_action_mask); the observe launch (the terminal window goes into d_obs); the stash (rows of the environments that ended go
 * to the final planes, the others are not written); the re-spawn; the observe launch again; the mask (if d_action_mask).  Refuses
 * what hwy_step_same_step_device and hwy_ttc_observe_device refuse.
 */
int hwy_step_same_step_ttc_device(hwy_engine *eng, const hwy_ttc_params *params, const int32_t *d_actions, float *d_obs, double *d_reward,
                                  uint8_t *d_terminated, uint8_t *d_truncated, double *d_info_speed, uint8_t *d_info_crashed,
                                  float *d_final_obs, double *d_final_info_speed, uint8_t *d_final_info_crashed, uint8_t *d_final_mask,
                                  uint8_t *d_action_mask, uint8_t *d_final_action_mask);
/*
 * k_steps (step launch, observe launch) pairs in one call, block k of every plane belonging to step k: d_actions [K][E][A],
 * d_obs [K][E][A][3][3][T], d_reward [K][E][A], d_terminated / d_truncated [K][E], the info planes [K][E][A] or NULL.  NextStep
 * auto-reset between the steps when hwy_set_autoreset enabled it.  k_steps == 1 is the single step whose observation is
 * the window; bit for bit the results of k_steps such calls.  The step's own Kinematics / Lidar / OccupancyGrid observation goes to a
 * buffer the engine owns (allocated on first use).
 */
int hwy_rollout_ttc_device(hwy_engine *eng, const hwy_ttc_params *params, int32_t k_steps, const int32_t *d_actions, float *d_obs,
                           double *d_reward, uint8_t *d_terminated, uint8_t *d_truncated, double *d_info_speed, uint8_t *d_info_crashed);

/*
 * Lidar through a door of its own (additive to ABI v8: hwy_config keeps its layout; obs_type HWY_OBS_LIDAR stays what it was, on the
 * highway scenario and up to HWY_MAX_LIDAR_CELLS cells).  Replaces LidarObservation.trace + observe (envs/common/observation.py:
 * 702-769) of the state as it stands for every (environment, agent) at once, in a kernel of its own (csrc/hwy_lidar_door.h), next to
 * whatever obs_type the engine was created with: float32 [cells][2] = (distance, relative radial speed) per cell, divided by
 * maximum_range when `normalize`.  Every scenario, ego control, traffic model and obs_type.  Every slot that is not HWY_F_ABSENT and
 * is not the observer is traced, in slot order (the reference's road.vehicles + road.objects); a slot with HWY_F_OBSTACLE is 2 m x 2 m.
 * HWY_SCENARIO_INTERSECTION: agent a observes from the a-th present slot that carries HWY_F_CONTROLLED.  The reference's
 * IntersectionEnv.step observes BEFORE it clears and spawns vehicles (intersection_env.py:136-140); this call sees the list AFTER
 * them, so behind a step it is what observation_type.observe() returns when called after step(), NOT the observation step() returned.
 * HWY_ERR_INVALID_ARG: NULL params or output, cells outside 1..HWY_MAX_LIDAR_DOOR_CELLS, maximum_range not positive or above FLT_MAX (the grid holds it as a float32),
 * normalize not 0 or 1, an engine that was never reset (hwy_reset / hwy_set_state / a fork into it).  hwy_last_error has the reason.
 */
typedef struct hwy_lidar_params {
  int32_t cells;        /* 1..HWY_MAX_LIDAR_DOOR_CELLS: cell k looks along k * 2 pi / cells */
  int32_t normalize;    /* 0 / 1: divide by maximum_range */
  double maximum_range; /* metres; positive, at most FLT_MAX */
} hwy_lidar_params;
/* d_obs f32 [E][A][cells][2], DEVICE pointer; one launch on the engine's stream; does not synchronise. */
int hwy_lidar_observe_device(hwy_engine *eng, const hwy_lidar_params *params, float *d_obs);
/* The same into a HOST pointer; synchronises. */
int hwy_lidar_observe(hwy_engine *eng, const hwy_lidar_params *params, float *obs);
/*
 * k_steps (step launch, observe launch) pairs in one call, block k of every plane belonging to step k: d_actions [K][E][A],
 * d_obs [K][E][A][cells][2], d_reward [K][E][A], d_terminated / d_truncated [K][E], the info planes [K][E][A] or NULL.  NextStep
 * auto-reset between the steps when hwy_set_autoreset enabled it.  k_steps == 1 is the single step whose observation is the trace;
 * bit for bit the results of k_steps such calls.  The step's own configured observation goes to a buffer the engine owns (allocated
 * on first use).  HWY_ERR_UNSUPPORTED on HWY_SCENARIO_INTERSECTION (see above: the trace behind a step is not step()'s observation).
 */
int hwy_rollout_lidar_device(hwy_engine *eng, const hwy_lidar_params *params, int32_t k_steps, const int32_t *d_actions, float *d_obs,
                             double *d_reward, uint8_t *d_terminated, uint8_t *d_truncated, double *d_info_speed, uint8_t *d_info_crashed);

/*
 * Environment fork and scoring of action sequences (additive to ABI v8: hwy_config keeps its layout).  The device form of the
 * reference's simulator-based planning seam: copy.deepcopy(env) (AbstractEnv.__deepcopy__, envs/common/abstract.py:455) and
 * env.step on the copy (scripts/highway_planning.ipynb).  HWY_SCENARIO_HIGHWAY only -- every traffic model, ego control, observation
 * type, agent count and N; a merge or intersection engine returns HWY_ERR_UNSUPPORTED (the intersection draws traffic while it runs
 * and keeps shadow episodes).  Kernels of their own (csrc/hwy_lookahead.h); no step / reset / observe kernel is touched.
 *
 * hwy_fork_device: environment j of `dst` becomes a copy of environment d_src_env[j] of `src` (d_src_env: DEVICE pointer, int32
 * [dst.num_envs]), or of environment j / branches when d_src_env is NULL.  Copied: everything a later step of `dst` can read -- the
 * nine f64 planes, the packed words whole (rank hint included), the Linear family's behaviour planes, the stored controls of a
 * HWY_EGO_DIRECT ego [E][A], `time` and the episode counter; the "ended, awaits its re-spawn" mark of `dst` is cleared (a source
 * environment that awaits its NextStep re-spawn is forked as it stands: stepping the copy continues the ended episode, which is
 * what stepping the reference after `done` gives).  Columns >= N of the pitch are copied as they are.
 * Accepted: dst != src, both on the same device, both highway engines, configs equal in every field that is not num_envs or tune_*,
 * branches >= 1, and dst.num_envs == src.num_envs * branches when d_src_env is NULL (with d_src_env any dst.num_envs); anything
 * else is HWY_ERR_INVALID_ARG with a reason in hwy_last_error(dst).  The indices behind d_src_env are NOT validated (hwy_fork
 * does): an index outside [0, src.num_envs) leaves that destination environment as it was.
 * The copy is enqueued on dst's stream and does not synchronise (like hwy_step_device); when the two streams differ, dst's stream
 * first waits on an event recorded on src's stream.  `src` is only read: the caller keeps later WRITES to src (a step on another
 * stream) behind the copy.
 */
int hwy_fork_device(hwy_engine *dst, hwy_engine *src, int32_t branches, const int32_t *d_src_env);
/* The same with HOST indices (src_env may be NULL), validated: HWY_ERR_INVALID_ARG for one outside [0, src.num_envs); synchronises. */
int hwy_fork(hwy_engine *dst, hwy_engine *src, int32_t branches, const int32_t *src_env);
/*
 * Fold the outputs of a k_steps rollout (hwy_rollout_device, auto-reset off) of an engine of E * branches environments -- environment
 * e * branches + b is branch b of group e -- into discounted returns and a decision.  Return of branch b, agent a:
 *     g = 0; d = 1; alive = true
 *     for k in 0 .. K-1:  if alive: t = d * r[k]; g = g + t
 *                         alive = alive && !(terminated[k] | truncated[k]);  d = d * gamma
 * (product and sum round separately; an episode that ends is absorbing: its terminal reward counts, nothing after it does).
 *   d_first_action int32 [E*branches][A]  block 0 of the rollout's actions; NULL iff d_q and d_best_action are NULL
 *   d_reward       f64   [K][E*branches][A],  d_terminated / d_truncated u8 [K][E*branches]
 *   d_return       f64   [E][branches][A]   g                                                          (may be NULL)
 *   d_q            f64   [E][n_ids]         max of g over the branches of group e whose first action is i, -inf where none starts
 *                                           with i; n_ids = size of the action table (5, 3 or n_accel * n_steer)   (A == 1; may be NULL)
 *   d_best_action  int32 [E]                the first maximum of d_q[e] (numpy's argmax)                 (A == 1; may be NULL)
 *   d_best_branch  int32 [E][A]             the lowest branch holding the maximal g of agent a           (may be NULL)
 * HWY_ERR_INVALID_ARG: k_steps < 1, branches < 1 or not a divisor of num_envs, a non-finite gamma, a NULL input plane, d_q or
 * d_best_action with A > 1.  First actions outside the table (not validated here) count for no d_q column.  A NaN reward is outside
 * the contract.  DEVICE pointers; enqueues on the engine's stream and does not synchronise.
 */
int hwy_score_device(hwy_engine *eng, int32_t k_steps, int32_t branches, double gamma, const int32_t *d_first_action,
                     const double *d_reward, const uint8_t *d_terminated, const uint8_t *d_truncated, double *d_return,
                     double *d_q, int32_t *d_best_action, int32_t *d_best_branch);
/*
 * hwy_rollout_device + hwy_score_device through HOST pointers: actions int32 [K][E*branches][A] are validated like hwy_rollout
 * (HWY_ERR_ACTION), uploaded, rolled out and folded; every output may be NULL (reward [K][E*branches][A], terminated / truncated
 * [K][E*branches], then the outputs of hwy_score_device; q and best_action with A == 1 only).  Synchronises.
 */
int hwy_score_rollout(hwy_engine *eng, int32_t k_steps, int32_t branches, double gamma, const int32_t *actions,
                      double *reward, uint8_t *terminated, uint8_t *truncated, double *ret, double *q,
                      int32_t *best_action, int32_t *best_branch);

/*
 * Optimistic planning of deterministic systems (OPD, Hren & Munos 2008), one tree per environment (additive to ABI v8): the budgeted
 * tree search that scripts/highway_planning.ipynb runs on copy.deepcopy(env) + env.step, entirely on the device.  Kernel of its own
 * (csrc/hwy_opd.h); the simulation is hwy_step_device, the state moves by hwy_fork_device.  HWY_SCENARIO_HIGHWAY, a single agent,
 * either ego control (3, 5 or n_accel * n_steer action ids), every traffic model and observation type.
 *   n = n_ids; X = budget / n expansions; nodes = M = 1 + X * n.  Node 0 is the root (the current state of `src`); expansion x creates
 *   node 1 + x * n + a for action a.
 *   root:   lower = 0, disc = 1, upper = bound, not done
 *   child of p by a: the state of p stepped once with a (auto-reset off), r its reward:
 *           t = disc_p * r;  lower = lower_p + t;  disc = disc_p * gamma;  done = terminated | truncated;
 *           upper = done ? lower : lower + disc * bound     (every product and sum rounds on its own: lower is the return
 *           hwy_score_device gives the node's action sequence, bit for bit)
 *   backup after each expansion: value lower / upper of an expanded node = the maximum over its children
 *   selection: the leaf of the largest value upper, ties to the lowest node index; when that leaf is done the tree is solved: this and
 *           every later expansion is void (nothing is created)
 *   bound = 1 / (1 - gamma), evaluated by the caller in f64.
 * `tree` and `work` are engines of src.num_envs * nodes and src.num_envs * n_ids environments with src's config (as hwy_fork_device
 * wants them) and auto-reset off: tree environment e * M + i holds the state of node i, work environment e * n + a steps child a.
 *   d_action   int32 [E]      argmax over the root's children of value lower, ties to the lowest id
 *   d_value    f64   [E]      value lower of the root                                   (may be NULL)
 *   d_upper    f64   [E]      value upper of the root                                   (may be NULL)
 *   d_sequence int32 [E][X]   the argmax-lower children from the root to a leaf, then -1  (may be NULL)
 *   d_expanded int32 [E]      expansions made (< X: the tree was solved)                (may be NULL)
 * HWY_ERR_UNSUPPORTED off the highway and for several agents; HWY_ERR_INVALID_ARG unless 0 < gamma < 1, bound positive and finite,
 * n_ids the size of the action table, budget >= n_ids, nodes == 1 + X * n <= 1024, HWY_C_NORMALIZE_REWARD set (the bound assumes
 * rewards in [0, 1]), the three engines distinct and on one device, and tree / work of those sizes with auto-reset off.
 * DEVICE pointers.  Enqueues X x (hwy_opd_kernel, gather tree -> work, step of work, scatter work -> tree) and one more kernel launch
 * without a host round trip and does not synchronise; the outputs are ordered on work's stream (streams that differ are chained by
 * events, as in hwy_fork_device).  `src` is only read; the tree's bookkeeping lives in device memory owned by `tree`, allocated by
 * the first call.
 * flags & HWY_OPD_MASKED (a HWY_EGO_META ego; HWY_ERR_UNSUPPORTED otherwise): a node's unavailable actions (hwy_action_mask_device
 * of its state) get no child.  X, the node numbering and every rule above stay: the slot 1 + x * n + a of an unavailable action stays
 * reserved and counts as never created; backup, selection, the root's argmax and the greedy sequence run over created children only
 * (IDLE always exists).  Per expansion one more small launch: the mask kernel on `work` after the gather, whose n copies of the
 * leaf's state give that leaf's mask; the next tree launch (hwy_opd_masked_kernel) ingests only the available children.
 */
enum { HWY_OPD_MASKED = 1 }; /* hwy_opd_params.flags */
typedef struct hwy_opd_params {
  int32_t budget, n_ids, nodes;
  int32_t flags;                /* 0: every node gets all n_ids children; HWY_OPD_MASKED: see above; any other bit: HWY_ERR_INVALID_ARG */
  double gamma, bound;
} hwy_opd_params;
int hwy_opd_plan_device(hwy_engine *src, hwy_engine *tree, hwy_engine *work, const hwy_opd_params *params, int32_t *d_action,
                        double *d_value, double *d_upper, int32_t *d_sequence, int32_t *d_expanded);
/* The same into HOST pointers (all but action may be NULL); synchronises. */
int hwy_opd_plan(hwy_engine *src, hwy_engine *tree, hwy_engine *work, const hwy_opd_params *params, int32_t *action, double *value,
                 double *upper, int32_t *sequence, int32_t *expanded);

/*
 * Action mask (additive to ABI v8: hwy_config keeps its layout).  AbstractEnv.get_available_actions (envs/common/abstract.py:357) ->
 * DiscreteMetaAction.get_available_actions (envs/common/action.py:262-298) for every (environment, agent) at once, in a kernel of
 * its own (csrc/hwy_mask.h) that reads the state planes on the engine's stream after whatever was launched last.
 *   d_mask  uint8 [E][A][n_ids]  1 = the action is available, 0 = it is not; columns in the order of the engine's action table
 *           (hwy_config.action_set: HWY_ACTIONS_ALL {LANE_LEFT, IDLE, LANE_RIGHT, FASTER, SLOWER}, HWY_ACTIONS_LONGI {SLOWER, IDLE,
 *           FASTER}, HWY_ACTIONS_LAT {LANE_LEFT, IDLE, LANE_RIGHT}; HWY_SCENARIO_INTERSECTION: the longitudinal table)
 * IDLE is always available; LANE_LEFT / LANE_RIGHT when the table has the lateral axis, the lane _id -/+ 1 exists on the road of the
 * vehicle's CURRENT lane_index (RoadNetwork.side_lanes, road/road.py:200-211) and is_reachable_from(position) (road/lane.py:104-118:
 * not forbidden, |lateral| <= 2 * width, 0 <= s < length + 5); FASTER / SLOWER when the table has the longitudinal axis and
 * speed_index < num_target_speeds - 1 / speed_index > 0.
 * All three scenario families with a HWY_EGO_META ego; HWY_ERR_UNSUPPORTED for HWY_EGO_DIRECT (the reference's
 * ActionType.get_available_actions raises NotImplementedError); HWY_ERR_INVALID_ARG for a NULL pointer.
 * DEVICE pointer; enqueues on the engine's stream and does not synchronise (like hwy_step_device).
 */
int hwy_action_mask_device(hwy_engine *eng, uint8_t *d_mask);
/* The same into a HOST pointer; synchronises. */
int hwy_action_mask(hwy_engine *eng, uint8_t *mask);

int hwy_sync(hwy_engine *eng); /* hipStreamSynchronize on the engine stream */

/*
 * Event counters of an engine since creation (or since the last call with reset != 0); synchronises the stream.
 * HWY_SCENARIO_INTERSECTION, device traffic mode: IntersectionEnv._spawn_vehicle (intersection_env.py:324-352) appends to
 * an unbounded list; the engine has hwy_config.num_vehicles slots per environment and DROPS a spawn that finds them all
 * taken.  HWY_CTR_IX_SPAWNS counts the spawns performed, HWY_CTR_IX_SPAWNS_DROPPED the ones dropped (initial traffic,
 * the per-step spawn and the pre-warmed next episodes alike), so a caller can size max_vehicles until the second is 0.
 * `out` receives min(n, HWY_CTR_COUNT) values.
 */
/* HWY_CTR_NONFINITE_STORES (every scenario): vehicles written back by a step / frames launch with a non-finite position,
 * heading or speed -- 0 in any healthy run; a NaN handed in through hwy_set_state (or produced by a defect) shows up here. */
enum { HWY_CTR_IX_SPAWNS = 0, HWY_CTR_IX_SPAWNS_DROPPED = 1, HWY_CTR_NONFINITE_STORES = 2, HWY_CTR_COUNT = 8 };
int hwy_get_counters(hwy_engine *eng, uint64_t *out, int32_t n, int32_t reset);

/*
 * Placement of the environments on the GPU's SIMDs (tuning; never changes a result).  Environments are independent
 * (the reference steps them in separate processes: scripts/sb3_highway_ppo.py:16-18), so WHICH workgroup of a launch steps
 * environment e is free: with env_of_block[b] = e (host pointer, a permutation of 0 .. num_envs - 1) workgroup b of every
 * following hwy_step* / hwy_step_device launch steps environment e; all inputs and outputs stay indexed by environment.
 * NULL restores the identity.  One-wavefront step kernel only (HWY_SCENARIO_HIGHWAY, num_vehicles <= 64); synchronises.
 */
int hwy_set_block_order(hwy_engine *eng, const int32_t *env_of_block);

/*
 * Shapes of the one-wavefront step kernel (tuning; never changes a result).  A policy step of HWY_SCENARIO_HIGHWAY with IDM traffic
 * and meta-actions whose structure is that of a registered configuration -- highway-fast-v0 on 3 or 4 lanes, highway-v0 on 4 lanes:
 * one agent, the default Kinematics observation, three target speeds, the five-action table, auto-reset on, every output plane
 * bound -- runs a build of the kernel compiled for that structure; every other launch (another configuration, hwy_step_frames, a
 * step without actions or info planes, an engine before hwy_set_autoreset, hwy_rollout*) runs the generic kernel.
 * hwy_step_shapes(on): 1 = as above (the default, unless the environment holds HWY_STEP_SHAPES=0 when the library is first used),
 * 0 = every launch runs the generic kernel, any other value = no change; returns the setting that was in force.  Process-wide.
 * hwy_last_step_shape(): which build the last step launch of a straight-road engine ran: 0 = generic, 1 = highway-fast-v0 / 3
 * lanes, 2 = highway-fast-v0 / 4 lanes, 3 = highway-v0 / 4 lanes.  The reference has no counterpart (one Python code path:
 * envs/common/abstract.py:287-317).
 */
int hwy_step_shapes(int on);
int hwy_last_step_shape(void);

/*
 * Self-test hook: evaluate one of the step kernel's own math routines (csrc/hwy_math.h -- bounded-domain
 * log / exp / sincos / asin, Newton-refined v_rcp_f64 / v_rsq_f64, floor-mod angle wrap) on n doubles on
 * the device.  Host pointers.  op: 0 log_pos, 1 exp_bounded, 2 sin, 3 cos, 4 asin_bounded, 5 fast_rcp, 8 atan_fd,
 * 9 atan2_bounded(x, 0.75), 10 atan2_bounded(0.5, x), 11 atan2_bounded(-0.5, x), 12 tan_bounded (|x| <= pi/3, the Linear
 * traffic family's steering),
 * 6 fast_rsqrt, 7 wrap_to_pi; 20 .. 33: the paired forms (log_pos2, exp_bounded2, sincos_bounded2, asin_bounded2, fast_rcp2,
 * fast_rsqrt2: first / second result, see math_probe in csrc/hwy_device.h), which must equal the scalar ones bit for bit.
 * 40 / 41: the collision walk's reach bound (hwy_device.h: the wavefront's maximum of reach_key -- call with whole wavefronts, n a
 * multiple of 64 --, and the double a key is rounded up to).  42: x * x - 1.0 in one source expression -- which arithmetic the
 * build has (fused under -ffp-contract=on, rounded twice under off: tests/test_strict_arithmetic.py).
 * Lets the accuracy claims (<= 2 ulp on the stated domains) be checked on the GPU.
 */
int hwy_debug_math(hwy_engine *eng, int32_t op, const double *in, double *out, int64_t n);

/*
 * Kernel timing of the step kernel of hwy_step / hwy_step_device / hwy_step_frames calls with HIP events on the
 * engine's stream: the launch (hipExtLaunchKernelGGL) records the DISPATCH's own begin and end timestamps into
 * the pair, i.e. what rocprofv3 --kernel-trace reports for it (events recorded around the launch with
 * hipEventRecord also measure ~3 us of command processing).  `enabled`: 0 = off, k > 0 = time every k-th
 * launch.  hwy_profile_read synchronises and returns the accumulated kernel time and the number of TIMED
 * launches since the last hwy_profile_enable(eng, k > 0).
 */
int hwy_profile_enable(hwy_engine *eng, int32_t enabled);
int hwy_profile_read(hwy_engine *eng, double *total_ms, int64_t *launches);

/*
 * The issue-priority turn in use (the encoding of hwy_config.tune_prio_shift: 0 = none, 1..30 = 2^k clock ticks, >= 64 = k x 64
 * ticks) and the state of the engine's own selection: with tune_prio_shift == 0 and a scenario whose wavefronts take turns, the
 * engine times its first 85 full-step launches per stage (five turn lengths around the scenario default, interleaved; the dispatch
 * timestamps of hwy_profile_*) and keeps the fastest -- scheduling only, no result depends on it.  state: 0 = no selection (explicit
 * value, turns off, or a kernel without turns), 1 = still sampling, 2 = chosen.  The reference has no counterpart (a CPU
 * single-thread loop: envs/common/abstract.py:287-317); this is the knob a `configure()`d shape other than BASELINE's needs
 * (envs/highway_env.py:25-53).
 */
int hwy_get_prio_turn(hwy_engine *eng, int32_t *turn, int32_t *state);

/*
 * Multi-GPU, one process (and one engine) per GPU.  The reference's only vectorisation is gymnasium's process-level
 * vector env (tests/envs/test_gym.py:158-165); here the environments are block-partitioned over the engines of a node,
 * nothing is exchanged while stepping, and the per-step (obs | reward | done) blocks of every rank are gathered to a root
 * rank with ONE RCCL collective over xGMI (ncclGather, rccl.h:745), enqueued on the engine's stream.
 *   hwy_comm_unique_id  rank 0 only; the caller ships the HWY_COMM_ID_BYTES bytes to every other rank (MPI, a TCP store, ...)
 *   hwy_comm_init       collective over all `world` ranks; librccl is loaded on first use (HWY_ERR_UNSUPPORTED if absent)
 *   hwy_gather          `bytes` bytes from device pointer d_send of every rank -> d_recv[rank * bytes ...] on `root`
 *                       (d_recv is ignored on the other ranks); asynchronous: hwy_sync or stream order makes it visible
 * A caller that keeps its buffers in a framework (PyTorch) may use that framework's collectives instead
 * (highwayenv_amd/dist.py does, bench.py --comm abi uses these entry points).
 */
#define HWY_COMM_ID_BYTES 128
int hwy_comm_unique_id(uint8_t *id);
int hwy_comm_init(hwy_engine *eng, const uint8_t *id, int32_t rank, int32_t world);
int hwy_gather(hwy_engine *eng, const void *d_send, void *d_recv, size_t bytes, int32_t root);
int hwy_comm_destroy(hwy_engine *eng);

/*
 * SameStep autoreset on the device (additive to ABI v8: hwy_config keeps its layout).  gymnasium's vector autoreset mode "SameStep"
 * (gymnasium/vector/vector_env.py: AutoresetMode.SAME_STEP; the reference's vectorisation test asks for it, tests/envs/test_gym.py):
 * the step that ends an episode returns the FIRST observation of the next one, and the terminal observation and info on the side.
 * hwy_step_device's arguments, then
 *   d_final_obs           f32 the observation's own shape [E][A]...   rows of the environments that ended: the terminal observation
 *   d_final_info_speed    f64 [E][A]   (may be NULL)                  likewise the terminal info
 *   d_final_info_crashed  u8  [E][A]   (may be NULL)
 *   d_final_mask          u8  [E]      1 = the environment ended in this call (terminated | truncated), 0 = it did not
 *   d_action_mask         u8  [E][A][n_ids]  (may be NULL)  hwy_action_mask_device of the state the call leaves
 *   d_final_action_mask   u8  [E][A][n_ids]  (may be NULL)  ... of the state the step left, before any re-spawn: the terminal state's
 *                                                           mask in the rows of the environments that ended
 * One call enqueues, in order on the engine's stream: the family's ordinary step launch, exactly as hwy_step_device issues it with
 * auto-reset on (a Lidar engine: + the trace); the mask kernel into d_final_action_mask; the stash kernel (csrc/hwy_same_step.h) --
 * d_final_mask[e] = done[e] for every e, and for the ones that ended their rows of d_obs, d_info_speed, d_info_crashed copied to
 * the final planes, the rows of the others NOT written at all (the caller reads them under the mask); the family's re-spawn kernel,
 * which starts the next episode of every environment that ended exactly as the next-step auto-reset would at the following call
 * (seed base_seed + e, episode counter + 1, the same spawn rule, the Linear family's parameter draws, a direct-control ego's stored
 * controls zeroed), observes it into d_obs, writes the new ego's d_info_speed and d_info_crashed = 0 and clears the "ended" mark --
 * d_reward, d_terminated and d_truncated of the row are NOT touched, they stay the ending step's; a Lidar engine: the trace again;
 * the mask kernel into d_action_mask.  Episode k of environment e is therefore the same episode, bit for bit, under this call and
 * under hwy_step_device's next-step auto-reset.  No environment is ever "ended, awaiting its re-spawn" between two calls.
 * hwy_set_autoreset must have enabled auto-reset (it supplies base_seed and the spawn arguments): HWY_ERR_INVALID_ARG otherwise, and
 * for a NULL d_final_obs / d_final_mask or a final info plane without its info plane.  Either mask pointer on an engine without a
 * DiscreteMetaAction ego: what hwy_action_mask_device returns.  HWY_SCENARIO_HIGHWAY (every traffic model, ego control, observation
 * type, agent count and N) and the merge scenarios; HWY_ERR_UNSUPPORTED for HWY_SCENARIO_INTERSECTION, whose next episodes are
 * pre-warmed in shadow planes keyed to the episode counter.
 * DEVICE pointers; only enqueues and does not synchronise (like hwy_step_device); action ids are not validated (see there).
 */
int hwy_step_same_step_device(hwy_engine *eng, const int32_t *d_actions, float *d_obs, double *d_reward, uint8_t *d_terminated,
                              uint8_t *d_truncated, double *d_info_speed, uint8_t *d_info_crashed, float *d_final_obs,
                              double *d_final_info_speed, uint8_t *d_final_info_crashed, uint8_t *d_final_mask,
                              uint8_t *d_action_mask, uint8_t *d_final_action_mask);

/*
 * Continuous throttle and steering for the plain-Vehicle egos of a HWY_EGO_DIRECT engine (additive to ABI v8: hwy_config keeps its
 * layout).  ContinuousAction.act (envs/common/action.py:136-163): a float action in [-1, 1]^size per (environment, agent) -- size 2
 * with both axes (throttle first, then steering), 1 with one -- is clipped, mapped onto the configured ranges and stored as the
 * vehicle's (acceleration, steering) pair, the planes of hwy_set_controls.  DiscreteAction is nothing but this on a grid
 * (action.py:189-196), so the simulation is the engine's own: every entry point below is the act kernel (csrc/hwy_act.h:
 * hwy_act_continuous_kernel, one thread per row) followed on the engine's stream by the EXISTING step launch with no action ids,
 * which then drives on with the stored pair.  No step kernel reads a float buffer.
 * The mapping is the reference's for a FLOAT32 action, the dtype of its Box(-1, 1, (size,), float32): np.clip and every operation of
 * utils.lmap in float32, the range ends rounded to float32 where they meet the value, the result widened to double
 * (csrc/hwy_act.h states the steps); an axis that is not controlled stores 0.0.  Bit for bit the reference's stored action.
 */
typedef struct hwy_continuous_params {
  double acceleration_range[2]; /* ContinuousAction.acceleration_range (default (-5, 5.0)), as configured: not float32-rounded */
  double steering_range[2];     /* ContinuousAction.steering_range (default (-pi/4, pi/4)); both ends within +-pi/3 */
  int32_t longitudinal;         /* 0 / 1: the throttle axis is controlled */
  int32_t lateral;              /* 0 / 1: the steering axis is controlled; at least one of the two */
} hwy_continuous_params;
/*
 * Every entry point validates `params` the same way: HWY_ERR_INVALID_ARG on a HWY_EGO_META engine (its vehicles store no controls),
 * for a NULL pointer, non-finite ranges, a steering end beyond +-pi/3 or no controlled axis.
 *
 * hwy_act_continuous_device: the act launch alone.  d_actions f32 [E][A][size], DEVICE pointer; enqueues and does not synchronise.
 * A row with a non-finite component (NaN, +-inf) leaves BOTH stored values of that row as they are -- the rule hwy_step_device
 * has for an id outside the table; the DEVICE forms do not validate the values.  Nothing is skipped for an environment that awaits its
 * next-step re-spawn: the episode start that follows zeroes its controls, as after a DiscreteAction step.
 * hwy_act_continuous: the same from a HOST pointer (HWY_ERR_ACTION for a non-finite component, before anything runs); synchronises.
 */
int hwy_act_continuous_device(hwy_engine *eng, const hwy_continuous_params *params, const float *d_actions);
int hwy_act_continuous(hwy_engine *eng, const hwy_continuous_params *params, const float *actions);
/*
 * One policy step: the act launch, then exactly hwy_step_device's launch with no ids (the same kernel, timing and auto-reset).  The
 * remaining arguments are hwy_step_device's.  Enqueues on the engine's stream and does not synchronise.
 */
int hwy_step_continuous_device(hwy_engine *eng, const hwy_continuous_params *params, const float *d_actions, float *d_obs,
                               double *d_reward, uint8_t *d_terminated, uint8_t *d_truncated, double *d_info_speed,
                               uint8_t *d_info_crashed);
/* The same through HOST pointers, like hwy_step (HWY_ERR_ACTION for a non-finite component; H2D, launches, D2H, synchronises). */
int hwy_step_continuous(hwy_engine *eng, const hwy_continuous_params *params, const float *actions, float *obs, double *reward,
                        uint8_t *terminated, uint8_t *truncated, double *info_speed, uint8_t *info_crashed);
/*
 * SameStep autoreset: the act launch, then hwy_step_same_step_device's sequence with no ids (step, stash, re-spawn).  The remaining
 * arguments and errors are that entry point's; either mask pointer: what hwy_action_mask_device returns (a direct ego has no mask).
 */
int hwy_step_same_step_continuous_device(hwy_engine *eng, const hwy_continuous_params *params, const float *d_actions, float *d_obs,
                                         double *d_reward, uint8_t *d_terminated, uint8_t *d_truncated, double *d_info_speed,
                                         uint8_t *d_info_crashed, float *d_final_obs, double *d_final_info_speed,
                                         uint8_t *d_final_info_crashed, uint8_t *d_final_mask, uint8_t *d_action_mask,
                                         uint8_t *d_final_action_mask);
/*
 * k_steps policy steps with pre-staged actions: d_actions f32 [K][E][A][size], block k of every output plane belongs to step k as in
 * hwy_rollout_device.  ONE call enqueues k_steps (act, step) pairs with no host round trip; the results are those of k_steps calls of
 * hwy_step_continuous_device, bit for bit, next-step auto-reset included.  The one-launch K-step form of hwy_rollout_device would
 * need a rollout kernel that reads the float buffer -- a new kernel of the step family; out of scope here.
 * hwy_rollout_continuous: the same through HOST pointers (HWY_ERR_ACTION for a non-finite component; synchronises).
 */
int hwy_rollout_continuous_device(hwy_engine *eng, const hwy_continuous_params *params, int32_t k_steps, const float *d_actions,
                                  float *d_obs, double *d_reward, uint8_t *d_terminated, uint8_t *d_truncated, double *d_info_speed,
                                  uint8_t *d_info_crashed);
int hwy_rollout_continuous(hwy_engine *eng, const hwy_continuous_params *params, int32_t k_steps, const float *actions, float *obs,
                           double *reward, uint8_t *terminated, uint8_t *truncated, double *info_speed, uint8_t *info_crashed);

/*
 * The float door into fork / rollout / score (additive to ABI v8).  hwy_score_rollout_continuous is the host-pointer twin of
 * hwy_score_rollout for a HWY_EGO_DIRECT engine: `eng` holds E * branches environments (environment e * branches + b == branch b of
 * group e, already forked), actions f32 [K][E * branches][A][size] are validated like hwy_rollout_continuous (HWY_ERR_ACTION for a
 * non-finite component, before anything runs), uploaded, rolled out by hwy_rollout_continuous_device into the engine's rollout block
 * and folded by hwy_score_device with d_first_action == NULL (a float sequence has no first action id: no q, no best_action).
 * Outputs (HOST pointers, each may be NULL): reward f64 [K][E * branches][A], terminated / truncated u8 [K][E * branches],
 * ret f64 [E][branches][A], best_branch i32 [E][A].  Synchronises.  No kernel of its own.
 */
int hwy_score_rollout_continuous(hwy_engine *eng, const hwy_continuous_params *params, int32_t k_steps, int32_t branches, double gamma,
                                 const float *actions, double *reward, uint8_t *terminated, uint8_t *truncated, double *ret,
                                 int32_t *best_branch);

/*
 * Sampling MPC by the cross-entropy method, one search per environment, on the device (csrc/hwy_cem.h; DESIGN.md "CEM on the
 * device").  Per iteration i: hwy_cem_sample_kernel draws `population` sequences of `horizon` float actions around the current mean
 * (branch 0 IS the mean) into the action block of `work`; hwy_fork_device(work, src, population); hwy_rollout_continuous_device(work,
 * horizon); hwy_score_device(work, ..., first_action NULL) folds the returns; hwy_cem_refit_kernel refits mean and std to the
 * `elites` best sequences and keeps the best sequence seen.  Everything is enqueued on work's stream with no host round trip; src's
 * stream continues behind it.  `work`: an engine of src.num_envs * population environments, same config, same device, auto-reset
 * off; its planner arrays live in a block of its own, grown on demand.  src is left as it was.
 * Scope: HWY_SCENARIO_HIGHWAY, HWY_EGO_DIRECT, a single agent (hwy_score_rollout_continuous serves several), every observation type;
 * HWY_ERR_UNSUPPORTED otherwise, HWY_ERR_INVALID_ARG for parameters outside the caps below, each with a reason in hwy_last_error(src).
 */
#define HWY_CEM_MAX_POP 1024    /* population: the keys of one environment's returns in LDS (8 KB) */
#define HWY_CEM_MAX_HORIZON 64  /* horizon; also the stride of the iteration in the Philox counter */
#define HWY_CEM_MAX_ITERATIONS 1024
typedef struct hwy_cem_params {
  int32_t population; /* B: sequences per iteration, 1 .. HWY_CEM_MAX_POP */
  int32_t elites;     /* M: 1 .. population */
  int32_t iterations; /* I: 1 .. HWY_CEM_MAX_ITERATIONS */
  int32_t horizon;    /* K: 1 .. HWY_CEM_MAX_HORIZON */
  double gamma;       /* discount of the return, finite */
  double init_std;    /* std of every component before the first refit, >= 0 */
  double min_std;     /* floor of the refitted std, >= 0 */
  double alpha;       /* smoothing: new = alpha * fitted + (1 - alpha) * old, in [0, 1] */
  uint64_t seed;      /* Philox key */
} hwy_cem_params;
/*
 * hwy_cem_plan_device: DEVICE pointers.  d_init_mean f64 [E][K][size] or NULL (zeros; not validated here).  d_action f32 [E][size]:
 * step 0 of the best sequence.  Optional (NULL: not written / kept in work's block): d_best_return f64 [E], d_mean / d_std f64
 * [E][K][size] (after the last refit), d_best_sequence f32 [E][K][size], d_noise f64 / d_samples f32 [I][E][B][K][size] (what the
 * sample kernel drew and wrote), d_elites i32 [I][E][M] (every iteration's elite branches, ascending).  d_init_mean may be produced
 * on src's stream: work's stream waits for what src's stream holds before the first sample.  Enqueues and does not synchronise.
 * hwy_cem_plan: the same through HOST pointers (HWY_ERR_ACTION for a non-finite init_mean, before anything runs); synchronises.
 */
int hwy_cem_plan_device(hwy_engine *src, hwy_engine *work, const hwy_continuous_params *params, const hwy_cem_params *cem,
                        const double *d_init_mean, float *d_action, double *d_best_return, double *d_mean, double *d_std,
                        float *d_best_sequence, double *d_noise, float *d_samples, int32_t *d_elites);
int hwy_cem_plan(hwy_engine *src, hwy_engine *work, const hwy_continuous_params *params, const hwy_cem_params *cem,
                 const double *init_mean, float *action, double *best_return, double *mean, double *stddev, float *best_sequence,
                 double *noise, float *samples, int32_t *elites);

#ifdef __cplusplus
}
#endif
#endif /* HWY_ENGINE_H */
