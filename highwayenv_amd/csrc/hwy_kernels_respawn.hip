// hwy_kernels_respawn.hip -- gfx950 translation unit of the SameStep re-spawn kernels (hwy_device.h: hwy_respawn_kernel,
// hwy_respawn_linear_kernel, hwy_respawn_direct_kernel; hwy_wave.h: hwy_respawn_wave_kernel, _linear_kernel, _direct_kernel;
// hwy_wave2.h: hwy_respawn_wide_kernel; hwy_net.h: hwy_net_respawn_kernel) and their launch functions, one overload per kernel
// family like launch_reset.  The kernels sit beside the reset and step kernels in the headers; they are instantiated HERE, in a
// translation unit of their own, so that every step, rollout, reset and observe kernel of hwy_kernels.hip, hwy_kernels_linear.hip and
// hwy_kernels_direct.hip keeps its code and its register allocation.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#define HWY_HAVE_SETPRIO 1  // (as in the units of the step kernels: one set of definitions of the shared device functions)
#include "hwy_device.h"
#include "hwy_wave.h"
#include "hwy_wave2.h"
#include "hwy_net.h"
#include "hwy_ix.h"
#include "hwy_launch.h"
#include "hwy_launch_rules.h"

namespace hwy {

hipError_t launch_respawn(const StepParams &p, const Launch &l) { return select_respawn<HipBackend>(p, l); }
hipError_t launch_respawn(const LinearParams &lp, const Launch &l) { return select_respawn<HipBackend>(lp, l); }
hipError_t launch_respawn(const DirectParams &dp, const Launch &l) { return select_respawn<HipBackend>(dp, l); }
hipError_t launch_respawn(const NetParams &np, const Launch &l) { return select_respawn<HipBackend>(np, l); }

}  // namespace hwy
