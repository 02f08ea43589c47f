// Stand-alone address / undefined-behaviour check of csrc/hashbits.h (tests/test_hashbits_host.py builds it with -fsanitize=address,undefined
// and runs it as a subprocess): the size query, the CSR writer into arrays of exactly the sizes it reports, and the host twin of the
// assignment and the public inputs, at m = 1 and 3.  Exit code 0 and "hashbits ok" on success.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include "hashbits.h"

using namespace celo;

static int run(size_t m) {
  HbSizes s;
  if (hb_sizes(m, &s)) return 1;
  // heap arrays of the exact sizes: one entry past any of them is a report
  std::unique_ptr<uint64_t[]> rp[3], val[3];
  std::unique_ptr<uint32_t[]> col[3];
  uint64_t* rpp[3];
  uint32_t* colp[3];
  uint64_t* valp[3];
  for (int k = 0; k < 3; k++) {
    rp[k].reset(new uint64_t[s.n_constraints + 1]);
    col[k].reset(new uint32_t[s.nnz[k]]);
    val[k].reset(new uint64_t[4 * s.nnz[k]]);
    rpp[k] = rp[k].get(); colp[k] = col[k].get(); valp[k] = val[k].get();
  }
  if (hb_write_csr(m, rpp, colp, valp)) return 2;
  for (int k = 0; k < 3; k++) {
    if (rpp[k][0] != 0 || rpp[k][s.n_constraints] != s.nnz[k]) return 3;
    for (uint64_t e = 0; e < s.nnz[k]; e++) if (colp[k][e] >= s.n_vars) return 4;
  }
  std::unique_ptr<uint8_t[]> rows(new uint8_t[48 * m]);
  for (size_t i = 0; i < 48 * m; i++) rows[i] = (uint8_t)(i * 37 + 11);
  std::unique_ptr<uint64_t[]> z(new uint64_t[4 * s.n_vars]), pub(new uint64_t[4 * (s.n_inputs - 1)]);
  for (int order = 0; order < 2; order++) {
    if (hb_assignment_host(rows.get(), m, order, z.get())) return 5;
    if (hb_public_inputs_host(rows.get(), 1, m, order, pub.get())) return 6;
    for (uint64_t c = 0; c + 1 < s.n_inputs; c++) {      // the instance rows of z are the Montgomery forms of the canonical ones
      uint64_t mont[4];
      hb_to_mont(pub.get() + 4 * c, mont);
      for (int j = 0; j < 4; j++) if (mont[j] != z[4 * (1 + c) + j]) return 7;
    }
  }
  printf("m=%zu constraints=%llu vars=%llu inputs=%llu nnz=%llu/%llu/%llu log_n=%llu stride=%llu\n", m, (unsigned long long)s.n_constraints,
         (unsigned long long)s.n_vars, (unsigned long long)s.n_inputs, (unsigned long long)s.nnz[0], (unsigned long long)s.nnz[1], (unsigned long long)s.nnz[2],
         (unsigned long long)s.log_n, (unsigned long long)s.stride);
  return 0;
}

int main() {
  for (size_t m : {size_t(1), size_t(3)}) if (int rc = run(m)) { fprintf(stderr, "hashbits: m = %zu failed at step %d\n", m, rc); return rc; }
  printf("hashbits ok\n");
  return 0;
}
