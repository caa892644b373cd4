// hwy_kernels_lookahead.hip -- gfx950 translation unit of the environment fork and the rollout scoring kernels (hwy_lookahead.h:
// hwy_fork_kernel, one workgroup per destination environment; hwy_score_kernel, one wavefront per environment group) and their
// launch functions.  Its own translation unit so that every kernel of the other units keeps its code and its register allocation.
#include <hip/hip_runtime.h>

#include "hwy_lookahead.h"
#include "hwy_launch.h"

namespace hwy {

// the unit's rules (hwy_launch_units.h) with the HIP backend
hipError_t launch_fork(const ForkParams &fp, hipStream_t stream) { return select_fork<HipBackend>(fp, stream); }
hipError_t launch_score(const ScoreParams &sp, hipStream_t stream) { return select_score<HipBackend>(sp, stream); }

}  // namespace hwy
