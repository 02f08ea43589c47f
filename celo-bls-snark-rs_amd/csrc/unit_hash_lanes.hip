// Translation unit: the many-lane kernel of the composite hasher's CRH (pedersen.h), launched by pedersen_crh_locked of unit_hash.hip.  A unit,
// and so a code object, of its own: beside k_pedersen_crh in unit_hash.hip's it made that kernel, instruction for instruction the same, 4 % slower on
// the bulk call of 65 536 x 127 B; apart, unit_hash.hip's device code is what it was.
#include "pedersen.h"
#include <hip/hip_runtime.h>
#include "runtime.h"
#include "units.h"
// two waves per SIMD, as the kernels of unit_hash.hip
#ifndef FROW_OCC
#define FROW_OCC __attribute__((amdgpu_waves_per_eu(2, 2)))
#endif
namespace celo {
// L lanes per message (a power of two, 2 .. CRH_BLOCK), CRH_BLOCK / L messages per workgroup (pedersen.h): lane l sums the chunks l (mod L)
// straight from the caller's bytes, the L partials are folded through the dynamic LDS (CRH_BLOCK slots of CRH_SLOT_WORDS words: 64 KB, two
// workgroups per CU) and lane 0 of each message writes its 48 bytes.  Every lane of the workgroup walks every round of the fold: the
// barriers stand outside the lane tests, and the lanes of messages past n carry the identity to the last of them.
__global__ void __launch_bounds__(CRH_BLOCK) FROW_OCC
k_pedersen_crh_lanes(const EdPoint* __restrict__ gens, const uint8_t* __restrict__ msgs, const uint64_t* __restrict__ off, uint8_t* __restrict__ out, uint32_t n, uint32_t L) {
  extern __shared__ __attribute__((aligned(16))) uint32_t crh_lds[];
  const uint32_t lane = threadIdx.x & (L - 1);
  const uint64_t i = (uint64_t)blockIdx.x * (CRH_BLOCK / L) + threadIdx.x / L;
  const bool live = i < n;
  EdPoint acc = ed_zero();
  if (live) acc = pedersen_crh_lane_sum(gens, PtrBytes{msgs + off[i], (size_t)(off[i + 1] - off[i])}, lane, L);
  uint32_t* mine = crh_lds + (size_t)threadIdx.x * CRH_SLOT_WORDS;   // slot `lane` of this message: its partner of a round is s slots on
  ed_store(mine, acc);
  for (uint32_t s = L >> 1; s; s >>= 1) {
    __syncthreads();
    if (lane < s) {                                                  // read this round: slots [s, 2 s); written: slots [0, s)
      acc = ed_add(acc, ed_load(mine + (size_t)s * CRH_SLOT_WORDS));
      if (s > 1) ed_store(mine, acc);
    }
  }
  if (live && lane == 0) {
    uint8_t h[48];
    pedersen_crh_finish(acc, h);
    for (int j = 0; j < 48; j++) out[(size_t)i * 48 + j] = h[j];
  }
}
void crh_lanes_launch(uint32_t grid, hipStream_t st, const EdPoint* gens, const uint8_t* msgs, const uint64_t* off, uint8_t* out, uint32_t n, uint32_t L) {
  hipLaunchKernelGGL(k_pedersen_crh_lanes, dim3(grid), dim3(CRH_BLOCK), CRH_BLOCK * CRH_SLOT_WORDS * 4, st, gens, msgs, off, out, n, L);
}
}  // namespace celo
