// hwy_lidar.h -- LidarObservation (envs/common/observation.py:678-769) of the highway scenario, a kernel of its own.
//
// The step / reset / observe kernels of the three straight-road families (IDM, the Linear family, direct ego control) stay exactly
// as they are: on a Lidar engine they run with a null `obs`, and this kernel is launched after them on the engine's stream.  It
// reads the state planes (x, y, heading, speed, the packed words for the presence flag) and the agent indices and writes
// obs f32 [E][A][cells][2] = (distance, relative radial speed) per cell.
//
// One 64-wide wavefront per (environment, agent), in passes of 64 obstacles for N up to HWY_MAX_VEHICLES:
//   phase 1, lane == obstacle: everything of trace() that does not depend on the cell -- the range test on the CENTRE, the centre
//     candidate (cell, distance, radial velocity), rect_corners, the five atan2 (centre + four corners), both wrap rules, the sector
//     [start, end], and the cell-independent half of utils.distance_to_rect (the unit vectors u, v and the four numerators) -- goes
//     to LDS, 92 bytes per obstacle (5.9 KB per workgroup: 16 workgroups fit in the 160 KB of a CU);
//   phase 2, lane == cell: lane c walks the obstacles of the pass IN LIST ORDER (LDS broadcast reads, no bank conflicts) and folds
//     the candidates of its cell -- the centre candidate before the ray candidate of the same obstacle -- into its (distance,
//     velocity) pair exactly as the reference's loop does: the pair is float32, a candidate is taken when its f64 distance is <= the
//     float32-rounded stored value.  The fold is the reference's sequential fold by construction (no parallel reformulation of
//     the `<=` against a rounded value is needed), so ties go to the later obstacle and a candidate a hair above the stored f32
//     loses even when it rounds to the same f32.
// utils.distance_to_rect (utils.py:388-416) keeps its divisions by zero in IEEE form: on a highway most headings are exactly 0, the
// ray of cell 0 (and, once `origin + range * direction - origin` has absorbed sin(pi), of cell cells/2) is parallel to a rectangle
// side, rqu or rqv is exactly 0 and the intervals hold +-inf or NaN; interval_distance and Python's max() are evaluated as written.
// Divisions and square roots are the IEEE ones (no reciprocal substitutes); products and sums of the reference's separate numpy
// operations are separate statements here, so -ffp-contract=on fuses none of them.  atan2 / sin / cos are hwy_math.h's (<= 2 ulp,
// the same code on the GPU and in the CPU emulation).
//
// Like hwy_device.h this header includes no HIP runtime: hwy_kernels_lidar.hip includes <hip/hip_runtime.h> first, the CPU
// emulation (tests/emu/emu_lidar.cpp) its shim, hip_emu.h.  The launch rule is hwy_launch_units.h's (select_lidar), for both.
#pragma once

#include <stdint.h>
#include <string.h>

#include "../../include/hwy_engine.h"
#include "hwy_device.h"

namespace hwy {

#define HWY_LIDAR_UNIT  // (hwy_launch_units.h: this unit's kernel is in the translation unit)

struct LidarParams {
  const double *x, *y, *heading, *speed;  // [E][pitch]
  const int32_t *packed;                  // [E][pitch]
  float *obs;                             // [rows][A][cells][2]
  int32_t N, A, pitch, cells;
  int32_t agent_index[HWY_MAX_AGENTS];
  double max_range;
};
// host side: the arguments of a config over the four planes it reads ([E][pitch] each), the packed words and the output
inline LidarParams lidar_params(const hwy_config &c, const double *x, const double *y, const double *heading, const double *speed,
                                const int32_t *packed, int pitch, float *obs) {
  LidarParams lp;
  memset(&lp, 0, sizeof lp);
  lp.x = x; lp.y = y; lp.heading = heading; lp.speed = speed;
  lp.packed = packed;
  lp.obs = obs;
  lp.N = c.num_vehicles; lp.A = c.num_agents; lp.pitch = pitch; lp.cells = c.lidar_cells;
  for (int a = 0; a < HWY_MAX_AGENTS; ++a) lp.agent_index[a] = a < c.num_agents ? c.agent_index[a] : 0;
  lp.max_range = c.lidar_max_range;
  return lp;
}

// the type of a grid cell: np.ones((cells, 2), dtype=np.float32) (observation.py:712)
typedef float lidar_cell_t;

// utils.interval_distance (utils.py:188-193)
__device__ inline double lidar_interval_distance(double min_a, double max_a, double min_b, double max_b) {
  return min_a < min_b ? min_b - max_a : min_a - max_b;
}
// `if distance <= self.grid[index, DISTANCE]: self.grid[index, :] = [distance, velocity]` (observation.py:723-726, 751-753)
__device__ inline void lidar_fold(lidar_cell_t &gd, lidar_cell_t &gv, double distance, double velocity) {
  if (distance <= (double)gd) {
    gd = (lidar_cell_t)distance;
    gv = (lidar_cell_t)velocity;
  }
}
// LidarObservation.angle_to_index: int(np.floor(angle / self.angle)) % self.cells (Python's non-negative modulo)
__device__ inline int lidar_angle_to_index(double angle, double cell_angle, int cells) {
  const int k = (int)floor(angle / cell_angle) % cells;
  return k < 0 ? k + cells : k;
}
// np.linalg.norm of a 2-vector: sqrt(x.dot(x))
__device__ inline double lidar_norm2(double vx, double vy) {
  const double a = vx * vx;
  const double b = vy * vy;
  return sqrt(a + b);
}
// a @ b of 2-vectors: numpy's dot accumulates the products onto +0.0, one after the other (so -0.0 + -0.0 comes out as +0.0)
__device__ inline double lidar_dot2(double ax, double ay, double bx, double by) {
  const double a = ax * bx;
  const double b = ay * by;
  double sum = 0.0;
  sum = sum + a;
  sum = sum + b;
  return sum;
}

enum { LIDAR_U_X = 0, LIDAR_U_Y, LIDAR_V_X, LIDAR_V_Y, LIDAR_AU, LIDAR_BU, LIDAR_AV, LIDAR_DV, LIDAR_RVX, LIDAR_RVY, LIDAR_CDIST,
       LIDAR_PLANES };

// NORMALIZE: LidarObservation(normalize=True), `obs /= self.maximum_range` (observation.py:706-707)
template <bool NORMALIZE>
__global__ void __launch_bounds__(64) hwy_lidar_kernel(const LidarParams p) {
  __shared__ double sh[LIDAR_PLANES][64];
  __shared__ int32_t sh_word[64];  // bit 31: the obstacle is traced; centre cell | start << 8 | end << 16
  const int lane = threadIdx.x;
  const int e = (int)blockIdx.x / p.A, a = (int)blockIdx.x % p.A;
  const size_t row = (size_t)e * p.pitch;
  const int me = p.agent_index[a];
  const int cells = p.cells;
  const double R = p.max_range;
  const double cell_angle = 2 * HWY_PI / cells;  // self.angle = 2 * np.pi / self.cells
  // observer: origin = position, origin_velocity = speed * [cos(heading), sin(heading)] (objects.py: RoadObject.velocity)
  const double ox = p.x[row + me], oy = p.y[row + me];
  double osn, ocs;
  sincos_bounded(p.heading[row + me], &osn, &ocs);
  const double ospeed = p.speed[row + me];
  const double ovx = ospeed * ocs, ovy = ospeed * osn;
  // my cell (phase 2): direction = [cos(index * angle), sin(index * angle)], ray = [origin, origin + maximum_range * direction]
  double dsn, dcs;
  sincos_bounded((double)lane * cell_angle, &dsn, &dcs);
  const double reach_x = R * dcs, reach_y = R * dsn;
  const double qx = ox + reach_x, qy = oy + reach_y;
  const double qrx = qx - ox, qry = qy - oy;  // q - r
  const double ray_len = lidar_norm2(qrx, qry);
  lidar_cell_t gd = (lidar_cell_t)R, gv = (lidar_cell_t)R;  // np.ones(..., float32) * maximum_range

  for (int base = 0; base < p.N; base += 64) {
    // ---- phase 1: lane == obstacle ------------------------------------------------------------------------------------------
    const int j = base + lane;
    int32_t word = 0;
    if (j < p.N && j != me && !(word_flags(p.packed[row + j]) & HWY_F_ABSENT)) {
      const double px = p.x[row + j], py = p.y[row + j];
      double sn, cs;
      sincos_bounded(p.heading[row + j], &sn, &cs);
      const double speed = p.speed[row + j];
      const double dx = px - ox, dy = py - oy;
      const double center_distance = lidar_norm2(dx, dy);
      // rect_corners (utils.py:128-157): rotation @ [-hl - hw, -hl + hw, +hl + hw, +hl - hw] + center; a, b, c, d in that order
      const double hl = HWY_VEH_LENGTH / 2, hw = HWY_VEH_WIDTH / 2;
      const double lx[4] = {-hl, -hl, hl, hl}, ly[4] = {-hw, hw, hw, -hw};
      double cx[4], cy[4], ang[4];
      for (int k = 0; k < 4; ++k) {
        const double x1 = cs * lx[k], x2 = -sn * ly[k];
        const double y1 = sn * lx[k], y2 = cs * ly[k];
        cx[k] = (x1 + x2) + px;
        cy[k] = (y1 + y2) + py;
        ang[k] = atan2_bounded(cy[k] - oy, cx[k] - ox) + cell_angle / 2;  // position_to_angle
      }
      const bool in_range = !(center_distance > R);  // the CENTRE decides, whatever the corners do (observation.py:717-719)
      if (in_range) {
        const int center_index = lidar_angle_to_index(atan2_bounded(dy, dx) + cell_angle / 2, cell_angle, cells);
        const double distance = center_distance - HWY_VEH_WIDTH / 2;
        const double vx = speed * cs, vy = speed * sn;
        const double rvx = vx - ovx, rvy = vy - ovy;  // obstacle.velocity - origin_velocity
        double min_angle = fmin(fmin(ang[0], ang[1]), fmin(ang[2], ang[3]));
        double max_angle = fmax(fmax(ang[0], ang[1]), fmax(ang[2], ang[3]));
        if (min_angle < -HWY_PI / 2 && HWY_PI / 2 < max_angle) {  // the corners wrap around +-pi
          const double t = min_angle;
          min_angle = max_angle;
          max_angle = t + 2 * HWY_PI;
        }
        const int start = lidar_angle_to_index(min_angle, cell_angle, cells), end = lidar_angle_to_index(max_angle, cell_angle, cells);
        // distance_to_rect, the part that is the same for every ray: u = (b - a) / |b - a|, v = (d - a) / |d - a|, r = origin
        double ux = cx[1] - cx[0], uy = cy[1] - cy[0], vxx = cx[3] - cx[0], vyy = cy[3] - cy[0];
        const double nu = lidar_norm2(ux, uy), nv = lidar_norm2(vxx, vyy);
        ux = ux / nu; uy = uy / nu; vxx = vxx / nv; vyy = vyy / nv;
        sh[LIDAR_U_X][lane] = ux; sh[LIDAR_U_Y][lane] = uy; sh[LIDAR_V_X][lane] = vxx; sh[LIDAR_V_Y][lane] = vyy;
        sh[LIDAR_AU][lane] = lidar_dot2(cx[0] - ox, cy[0] - oy, ux, uy);
        sh[LIDAR_BU][lane] = lidar_dot2(cx[1] - ox, cy[1] - oy, ux, uy);
        sh[LIDAR_AV][lane] = lidar_dot2(cx[0] - ox, cy[0] - oy, vxx, vyy);
        sh[LIDAR_DV][lane] = lidar_dot2(cx[3] - ox, cy[3] - oy, vxx, vyy);
        sh[LIDAR_RVX][lane] = rvx; sh[LIDAR_RVY][lane] = rvy;
        sh[LIDAR_CDIST][lane] = distance;
        word = (int32_t)(0x80000000u | (unsigned)center_index | ((unsigned)start << 8) | ((unsigned)end << 16));
      }
    }
    sh_word[lane] = word;
    __syncthreads();
    // ---- phase 2: lane == cell; the obstacles of the pass in list order -----------------------------------------------------------
    if (lane < cells) {
      const int n = p.N - base < 64 ? p.N - base : 64;
      for (int k = 0; k < n; ++k) {
        const int32_t w = sh_word[k];
        if (w >= 0) continue;
        const int center_index = w & 0xff, start = (w >> 8) & 0xff, end = (w >> 16) & 0xff;
        // np.arange(start, end + 1) if start < end else [start .. cells - 1] + [0 .. end] (the corners wrap around cell 0)
        const bool in_sector = start < end ? (lane >= start && lane <= end) : (lane >= start || lane <= end);
        if (lane != center_index && !in_sector) continue;
        const double rvx = sh[LIDAR_RVX][k], rvy = sh[LIDAR_RVY][k];
        const double velocity = lidar_dot2(rvx, rvy, dcs, dsn);  // (obstacle.velocity - origin_velocity).dot(direction)
        if (lane == center_index) lidar_fold(gd, gv, sh[LIDAR_CDIST][k], velocity);
        if (!in_sector) continue;
        // utils.distance_to_rect (utils.py:388-416), divisions by zero kept
        const double rqu = lidar_dot2(qrx, qry, sh[LIDAR_U_X][k], sh[LIDAR_U_Y][k]);
        const double rqv = lidar_dot2(qrx, qry, sh[LIDAR_V_X][k], sh[LIDAR_V_Y][k]);
        const double u0 = sh[LIDAR_AU][k] / rqu, u1 = sh[LIDAR_BU][k] / rqu;
        const double v0 = sh[LIDAR_AV][k] / rqv, v1 = sh[LIDAR_DV][k] / rqv;
        const double i1_lo = rqu >= 0 ? u0 : u1, i1_hi = rqu >= 0 ? u1 : u0;
        const double i2_lo = rqv >= 0 ? v0 : v1, i2_hi = rqv >= 0 ? v1 : v0;
        if (lidar_interval_distance(i1_lo, i1_hi, i2_lo, i2_hi) <= 0 && lidar_interval_distance(0, 1, i1_lo, i1_hi) <= 0 &&
            lidar_interval_distance(0, 1, i2_lo, i2_hi) <= 0) {
          const double first = i2_lo > i1_lo ? i2_lo : i1_lo;  // Python's max(interval_1[0], interval_2[0])
          lidar_fold(gd, gv, first * ray_len, velocity);
        }  // else: np.inf, which never passes `<=`
      }
    }
    __syncthreads();
  }
  if (lane < cells) {
    float *out = p.obs + (((size_t)blockIdx.x) * cells + lane) * 2;
    const float rf = (float)R;
    float od = (float)gd, ov = (float)gv;
    if (NORMALIZE) {  // on the float32 grid: a correctly rounded f32 division
      od = od / rf;
      ov = ov / rf;
    }
    out[0] = od;
    out[1] = ov;
  }
}

}  // namespace hwy
