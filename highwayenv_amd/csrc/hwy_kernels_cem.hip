// hwy_kernels_cem.hip -- gfx950 translation unit of the CEM planner's kernels (hwy_cem.h: hwy_cem_sample_kernel, one thread per
// (environment, branch, step); hwy_cem_refit_kernel, one wavefront per environment) and their launch functions.  Its own translation
// unit so that every kernel of the other units keeps its code and its register allocation.
#include <hip/hip_runtime.h>

#include "hwy_cem.h"
#include "hwy_launch.h"

namespace hwy {

// the unit's rules (hwy_launch_units.h) with the HIP backend
hipError_t launch_cem_sample(const CemParams &cp, hipStream_t stream) { return select_cem_sample<HipBackend>(cp, stream); }
hipError_t launch_cem_refit(const CemParams &cp, hipStream_t stream) { return select_cem_refit<HipBackend>(cp, stream); }

}  // namespace hwy
