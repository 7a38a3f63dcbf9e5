// The noise stream of the batched MD step kernels (snet_mdstep.hip, snet_mdnpt.hip): Philox4x32-10 of Salmon, Moraes, Dror,
// Shaw, "Parallel random numbers: as easy as 1, 2, 3", SC11 (the Random123 constants) through Box-Muller, keyed by the seed and
// counted by (atom index within its system, the caller's system id, the system's step, stream tag).  The rule is written out in
// include/snet_hip.h (snet_mdb_step) and restated in fp64 numpy in tests/md_ref.py.
#pragma once
#include "snet_common.h"

namespace snet {

constexpr double TWO_PI = 6.283185307179586;
// stream tags (the counter's fourth word): the Langevin thermostat, the velocity draw, the barostat of snet_mdb_npt_step
constexpr uint32_t STREAM_THERMOSTAT = 0u, STREAM_INIT = 1u, STREAM_BAROSTAT = 2u;

struct Philox {
  uint32_t w[4];
};

__device__ __forceinline__ Philox philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    if (r > 0) {
      k0 += 0x9E3779B9u;
      k1 += 0xBB67AE85u;
    }
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
  }
  return Philox{{c0, c1, c2, c3}};
}

// three standard normals of atom `a` of system `sys` at step `step`: Box-Muller on u_k = (w_k + 0.5) 2^-32 in (0, 1)
__device__ __forceinline__ void normals3(uint64_t seed, uint32_t a, uint32_t sys, uint32_t step, uint32_t tag, double (&xi)[3]) {
  const Philox p = philox4x32_10(a, sys, step, tag, (uint32_t)(seed & 0xffffffffull), (uint32_t)(seed >> 32));
  double u[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) u[k] = ((double)p.w[k] + 0.5) * 2.3283064365386963e-10;   // 2^-32, exact
  const double r0 = sqrt(-2.0 * log(u[0])), r1 = sqrt(-2.0 * log(u[2]));
  double s, c;
  sincos(TWO_PI * u[1], &s, &c);
  xi[0] = r0 * c;
  xi[1] = r0 * s;
  xi[2] = r1 * cos(TWO_PI * u[3]);
}

}  // namespace snet
