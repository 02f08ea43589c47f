// Translation unit: Groth16 verification over BLS12-377 for m proofs under one verifying key (groth16_verify_unit.h instantiated for G16Bls):
// the check of the hash-helper proof (crates/epoch-snark/src/api/prover.rs:83-118) that a prover pipeline makes before it spends the large
// BW6-761 proof on it.  A unit of its own so that the lane kernels of the 14-limb field are built, and reported in the build's resource
// remarks, apart from the 28-limb ones.  DESIGN.md section 6h.
#include "groth16_verify_unit.h"

namespace celo {
template struct G16Api<G16Bls>;
}  // namespace celo
