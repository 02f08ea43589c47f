// Translation unit: BLS12-377 pairing kernels + engine (see pairing.h).
#include "pairing.h"
#include "units.h"

namespace celo {
static EnginePool<PairingEngine<PP377>>& pool_377() { static auto* p = new EnginePool<PairingEngine<PP377>>(); return *p; }
static Last<PairingTimings> tm_last_377;

int pairing_run_377(const uint64_t* g1, const uint8_t* inf1, const uint64_t* g2, const uint8_t* inf2, const uint32_t* offsets, size_t m,
                    uint8_t* is_one, uint64_t* gt, int mode) {
  if (int rc = api_enter()) return rc;
  auto e = pool_377().lease();
  const int rc = e->run(g1, inf1, g2, inf2, offsets, m, is_one, gt, mode, e->own_stream());
  if (!rc && m) tm_last_377.note(e->tm);
  return rc;
}
int pairing_stage_377(uint32_t k, size_t m, PairingStage* st) {
  if (int rc = api_enter()) return rc;
  typedef EnginePool<PairingEngine<PP377>>::Lease L;
  L* l = new L(pool_377().lease());
  PairingEngine<PP377>::Staged sg;
  if ((*l)->stage(k, m, &sg)) { delete l; return 1; }
  *st = {l, sg.d_g1, sg.d_g2, sg.d_i1, sg.d_i2, (*l)->own_stream()};
  return 0;
}
int pairing_run_staged_377(PairingStage* st, const uint32_t* offsets, size_t m, uint8_t* is_one, float* kernel_ms) {
  typedef EnginePool<PairingEngine<PP377>>::Lease L;
  L* l = (L*)st->lease;
  if (!l) return 2;
  int rc = 0;
  if (offsets) {
    rc = (*l)->run_staged(offsets, m, true, true, is_one, nullptr, 0, st->stream);
    if (!rc && m) {
      tm_last_377.note((*l)->tm);
      if (kernel_ms) *kernel_ms = (*l)->tm.total;
    }
  }
  delete l;
  st->lease = nullptr;
  return rc;
}
int pairing_timings_377(float ms[4]) {
  const PairingTimings tm = tm_last_377.read();
  ms[0] = tm.miller; ms[1] = tm.product; ms[2] = tm.final_exp; ms[3] = tm.total;
  return 0;
}
}  // namespace celo
