// hwy_kernels.hip -- gfx950 translation unit: instantiates the fused step / reset /
// observe kernels of hwy_device.h and exposes plain launch functions to the C-ABI host
// (hwy_engine.hip).  Build: highwayenv_amd/build.py (hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=on ...).
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#define HWY_HAVE_SETPRIO 1  // s_setprio / s_memtime / s_getreg exist on the device (not in the CPU emulation of tests/emu)
#include "hwy_device.h"
#include "hwy_wave.h"
#include "hwy_wave2.h"
#include "hwy_net.h"
#include "hwy_ix.h"
#include "hwy_launch.h"
#include "hwy_launch_rules.h"

namespace hwy {

// Which kernel a launch runs (wide_kernel_applies and every other rule): hwy_launch_rules.h, hwy_launch_family.h.
hipError_t launch_step(const StepParams &p, const Launch &l) { return select_step<HipBackend>(p, l, false); }
hipError_t launch_rollout(const StepParams &p, const Launch &l) { return select_step<HipBackend>(p, l, true); }
hipError_t launch_reset(const StepParams &p, const Launch &l) { return select_reset<HipBackend>(p, l); }
hipError_t launch_observe(const StepParams &p, const Launch &l) { return select_observe<HipBackend>(p, l); }
int step_resident_blocks(const StepParams &p, const Launch &l) { return select_resident_blocks<HipBackend>(p, l); }

hipError_t launch_step(const NetParams &np, const Launch &l) { return select_step<HipBackend>(np, l, false); }
hipError_t launch_rollout(const NetParams &np, const Launch &l) { return select_step<HipBackend>(np, l, true); }
hipError_t launch_reset(const NetParams &np, const Launch &l) { return select_reset<HipBackend>(np, l); }
hipError_t launch_observe(const NetParams &np, const Launch &l) { return select_observe<HipBackend>(np, l); }
int step_resident_blocks(const NetParams &np, const Launch &l) { return select_resident_blocks<HipBackend>(np, l); }

hipError_t launch_step(const IxParams &ip, const Launch &l) { return select_step<HipBackend>(ip, l, false); }
hipError_t launch_rollout(const IxParams &ip, const Launch &l) { return select_step<HipBackend>(ip, l, true); }
hipError_t launch_reset(const IxParams &ip, const Launch &l) { return select_reset<HipBackend>(ip, l); }
hipError_t launch_observe(const IxParams &ip, const Launch &l) { return select_observe<HipBackend>(ip, l); }

__global__ void hwy_math_probe_kernel(int op, const double *in, double *out, long long n) {
  const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
  if (k < n) out[k] = math_probe(op, in[k]);
}
hipError_t launch_math_probe(int op, const double *in, double *out, long long n, hipStream_t stream) {
  hipExtLaunchKernelGGL(hwy_math_probe_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, nullptr, nullptr, 0, op, in, out, n);
  return hipGetLastError();
}

}  // namespace hwy
