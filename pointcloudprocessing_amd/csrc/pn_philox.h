// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): the counter-based generator behind
// pn_mesh_sample's draws and pn_plane_segment's hypotheses.  Integer operations only, so its bits are the NumPy oracle's
// (tests/mesh_sample_oracle.py, philox4x32).
#pragma once
#include "pn_common.h"

namespace pn {

constexpr unsigned PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u, PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;

__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned (&x)[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned h0 = __umulhi(PHILOX_M0, c0), l0 = PHILOX_M0 * c0;
    const unsigned h1 = __umulhi(PHILOX_M1, c2), l1 = PHILOX_M1 * c2;
    c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
    k0 += PHILOX_W0; k1 += PHILOX_W1;
  }
  x[0] = c0; x[1] = c1; x[2] = c2; x[3] = c3;
}

}  // namespace pn
