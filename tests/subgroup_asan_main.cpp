// Stand-alone address / undefined-behaviour check of the row validator (csrc/check.h) and of both forms of the BW6-761 subgroup test
// (csrc/wire761.h), built by tests/test_subgroup_host.py with -fsanitize=address,undefined and run as a subprocess; every buffer a heap
// array of its exact size.
//   argv[1]: the group (0 / 1: BLS12-377 G1 / G2, 2 / 3: BW6-761 G1 / G2); argv[2]: n; argv[3]: a file of n rows (12 or 24 u64) and n flag bytes
// Prints the n statuses of level 1, those of level 2, and "subgroup ok" when, for BW6-761, the ladder gives the statuses of the
// endomorphism form.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include "check.h"

using namespace celo;

template <int CG> static int run(const uint64_t* xy, const uint8_t* inf, size_t n) {
  const WireConsts& k = wire_consts();
  std::unique_ptr<uint8_t[]> st(new uint8_t[n]), st_ladder(new uint8_t[n]);
  for (int level = 1; level <= 2; level++) {
    for (size_t i = 0; i < n; i++) {
      const uint64_t* row = xy + i * check_row_words(CG);
      st[i] = check_row<CG>(row, inf[i] != 0, level, k, false);
      st_ladder[i] = check_row<CG>(row, inf[i] != 0, level, k, true);
    }
    for (size_t i = 0; i < n; i++) printf("%d%c", (int)st[i], i + 1 == n ? '\n' : ' ');
    for (size_t i = 0; i < n; i++) if (st[i] != st_ladder[i]) return 4;
  }
  printf("subgroup ok\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  const int cg = atoi(argv[1]);
  const size_t n = (size_t)atol(argv[2]);
  if (cg < 0 || cg > 3 || n == 0) return 2;
  const size_t words = n * check_row_words(cg);
  std::unique_ptr<uint64_t[]> xy(new uint64_t[words]);
  std::unique_ptr<uint8_t[]> inf(new uint8_t[n]);
  FILE* f = fopen(argv[3], "rb");
  if (!f || fread(xy.get(), 8, words, f) != words || fread(inf.get(), 1, n, f) != n) return 3;
  fclose(f);
  switch (cg) {
    case 0: return run<0>(xy.get(), inf.get(), n);
    case 1: return run<1>(xy.get(), inf.get(), n);
    case 2: return run<2>(xy.get(), inf.get(), n);
    default: return run<3>(xy.get(), inf.get(), n);
  }
}
