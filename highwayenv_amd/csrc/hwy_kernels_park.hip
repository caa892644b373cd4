// hwy_kernels_park.hip -- gfx950 translation unit of the parking scenario's kernels (hwy_park.h: hwy_park_advance_kernel,
// hwy_park_reset_kernel, hwy_park_goal_reward_kernel, one thread per environment / row; hwy_park_cem.h: hwy_park_cem_kernel and
// hwy_park_mppi.h: hwy_park_mppi_kernel, one wavefront per environment) and their launch functions.  Its own
// translation unit so that every kernel of the other units keeps its code and its register allocation.
#include <hip/hip_runtime.h>

#include "hwy_park.h"
#include "hwy_park_cem.h"
#include "hwy_park_mppi.h"

namespace hwy {

static inline unsigned park_blocks(long long n) { return (unsigned)((n + HWY_PARK_BLOCK - 1) / HWY_PARK_BLOCK); }

hipError_t launch_park_advance(const ParkParams &p, hipStream_t stream) {
  hwy_park_advance_kernel<HWY_PARK_BLOCK><<<dim3(park_blocks(p.E)), dim3(HWY_PARK_BLOCK), 0, stream>>>(p);
  return hipGetLastError();
}

// reset = true: the masked environments start episode 0; the observation of every environment goes to p.obs if it is given
hipError_t launch_park_reset(const ParkParams &p, bool reset, hipStream_t stream) {
  if (reset) hwy_park_reset_kernel<HWY_PARK_BLOCK, true><<<dim3(park_blocks(p.E)), dim3(HWY_PARK_BLOCK), 0, stream>>>(p);
  else hwy_park_reset_kernel<HWY_PARK_BLOCK, false><<<dim3(park_blocks(p.E)), dim3(HWY_PARK_BLOCK), 0, stream>>>(p);
  return hipGetLastError();
}

// one wavefront per environment; sample = true: the whole search (dynamic LDS: the sample table), false: one scoring pass
hipError_t launch_park_cem(const ParkCemParams &q, bool sample, hipStream_t stream) {
  const dim3 grid((unsigned)q.park.E), block(HWY_PARK_CEM_WAVE);
  if (sample) hwy_park_cem_kernel<true><<<grid, block, park_cem_lds_bytes(q), stream>>>(q);
  else hwy_park_cem_kernel<false><<<grid, block, 0, stream>>>(q);
  return hipGetLastError();
}

// one wavefront per environment: the whole MPPI search (dynamic LDS: the sample table)
hipError_t launch_park_mppi(const ParkMppiParams &q, hipStream_t stream) {
  const dim3 grid((unsigned)q.park.E), block(HWY_PARK_CEM_WAVE);
  if (q.noise || q.samples || q.returns || q.weights || q.mean_history) hwy_park_mppi_kernel<true><<<grid, block, park_mppi_lds_bytes(q), stream>>>(q);
  else hwy_park_mppi_kernel<false><<<grid, block, park_mppi_lds_bytes(q), stream>>>(q);
  return hipGetLastError();
}

hipError_t launch_park_goal_reward(const ParkGoalParams &g, hipStream_t stream) {
  hwy_park_goal_reward_kernel<HWY_PARK_BLOCK><<<dim3(park_blocks(g.m)), dim3(HWY_PARK_BLOCK), 0, stream>>>(g);
  return hipGetLastError();
}

}  // namespace hwy
