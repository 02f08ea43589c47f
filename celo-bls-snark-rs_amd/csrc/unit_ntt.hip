// Translation unit: NTTs over Fr(BW6-761) and Fr(BLS12-377) (see ntt.h).
#include "ntt.h"
#include "units.h"

namespace celo {
template <class FR> struct NttUnit {
  static EnginePool<NttEngine<FR>>& pool() { static auto* p = new EnginePool<NttEngine<FR>>(); return *p; }
};
static Last<NttTimings> tm_last_ntt;    // last transform of either field

template <class FR>
int ntt_run(uint64_t* data, unsigned log_n, const uint64_t* omega, const uint64_t* coset, int coset_after, const uint64_t* scale, int dev, void* stream) {
  if (int rc = api_enter()) return rc;
  if (!data || !omega) return 2;
  auto e = NttUnit<FR>::pool().lease();      // an engine keeps the twiddle table of its last (omega, n): repeated transforms reuse it
  const int rc = dev ? e->run_device(data, log_n, omega, coset, coset_after, scale, (hipStream_t)stream)
                     : e->run_host(data, log_n, omega, coset, coset_after, scale, e->own_stream());
  if (!rc) tm_last_ntt.note(e->tm);
  return rc;
}
template int ntt_run<Fr761>(uint64_t*, unsigned, const uint64_t*, const uint64_t*, int, const uint64_t*, int, void*);
template int ntt_run<Fr377>(uint64_t*, unsigned, const uint64_t*, const uint64_t*, int, const uint64_t*, int, void*);
int ntt_timings(float ms[4], int* passes) {
  const NttTimings tm = tm_last_ntt.read();
  ms[0] = tm.load; ms[1] = tm.passes; ms[2] = tm.store; ms[3] = tm.total;
  if (passes) *passes = tm.npasses;
  return 0;
}
}  // namespace celo
