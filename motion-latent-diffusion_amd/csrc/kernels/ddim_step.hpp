// The scheduler steps of the modular path (mldhip_ddim_step / mldhip_ddim_step_eta): one DDIM update of n elements outside the fused loops.
// C linkage and last in the translation unit (../mldhip.hip includes this file behind the engine): the two kernels keep the unmangled names and the
// place in the code object they have always had, so kernel-hash dumps of consecutive builds compare equal (tools/kernel_hashes.py).
#pragma once
#include "elementwise.hpp"
#include "novae.hpp"

using namespace mld;

extern "C" {
// stochastic DDIM step (mldhip_ddim_step_eta): one thread per Philox quad; z = noise[i] (injected) or element i of Philox(seed, step)
__global__ void ddim_step_eta_kernel(const float* eps, const float* x, const float* noise, float* out, long long n, DdimCoef c, DdimEta k,
                                     unsigned long long seed, unsigned step) {
  const long long nq = (n + 3) / 4;
  for (long long qd = (long long)blockIdx.x * blockDim.x + threadIdx.x; qd < nq; qd += (long long)gridDim.x * blockDim.x) {
    float z[4] = {0.f, 0.f, 0.f, 0.f};
    if (!noise) philox_normal4(seed, step, (unsigned long long)qd, z);
    for (int j = 0; j < 4; ++j) {
      const long long i = qd * 4 + j;
      if (i >= n) break;
      const float x0 = (x[i] - c.sqrt_1mat * eps[i]) / c.sqrt_at;
      float y = c.sqrt_ap * x0 + k.c_eps * eps[i];
      y += k.sigma * (noise ? noise[i] : z[j]);
      out[i] = y;
    }
  }
}

__global__ void ddim_step_kernel(const float* eps, const float* x, float* out, long long n, DdimCoef c) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const float x0 = (x[i] - c.sqrt_1mat * eps[i]) / c.sqrt_at;
    out[i] = c.sqrt_ap * x0 + c.sqrt_1map * eps[i];
  }
}
}  // extern "C"
