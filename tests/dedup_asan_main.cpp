// Stand-alone address / undefined-behaviour check of the key de-duplication table (csrc/dedup.h), built by tests/test_dedup_host.py with
// -fsanitize=address,undefined and run as a subprocess; every buffer a heap array of its exact size.
//   argv[1]: the key size (48 or 96); argv[2]: n; argv[3]: slack_log; argv[4]: max_probes; argv[5]: a file of n keys
// Prints U, then the n representatives, then "dedup ok" when the contract holds: rep[i] <= i, key rep[i] has the bytes of key i,
// rep[rep[i]] == rep[i], the list holds exactly the representatives and rank inverts it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include "dedup.h"

using namespace celo;

template <int KB> static int run(const uint8_t* keys, uint32_t n, int slack_log, uint32_t max_probes) {
  const uint64_t S = dedup_slots(n, slack_log);
  std::unique_ptr<uint32_t[]> owner(new uint32_t[S]), first(new uint32_t[S]), slot_of(new uint32_t[n]), rep(new uint32_t[n]), list(new uint32_t[n]), rank(new uint32_t[n]);
  const uint32_t U = dedup_host<KB>(keys, n, slack_log, max_probes, owner.get(), first.get(), slot_of.get(), rep.get(), list.get(), rank.get());
  printf("%u\n", U);
  for (uint32_t i = 0; i < n; i++) printf("%u%c", rep[i], i + 1 == n ? '\n' : ' ');
  if (U == 0 || U > n) return 4;
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t r = rep[i];
    if (r > i || rep[r] != r || memcmp(keys + (size_t)r * KB, keys + (size_t)i * KB, KB) != 0) return 5;
    if (slot_of[i] != DEDUP_NONE && (slot_of[i] >= S || first[slot_of[i]] != r)) return 6;
    if ((r == i) != (rank[i] != DEDUP_NONE)) return 7;
    if (r == i && (rank[i] >= U || list[rank[i]] != i)) return 8;
    if (dedup_hash<KB, false>(keys + (size_t)i * KB) != dedup_hash<KB, false>(keys + (size_t)r * KB)) return 9;
  }
  printf("dedup ok\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 6) return 2;
  const int kb = atoi(argv[1]), slack_log = atoi(argv[3]);
  const long n = atol(argv[2]), probes = atol(argv[4]);
  if ((kb != 48 && kb != 96) || n <= 0 || n > (1 << 24) || slack_log < 0 || slack_log > DEDUP_SLACK_MAX || probes < 1 || probes > DEDUP_PROBES_MAX) return 2;
  std::unique_ptr<uint8_t[]> keys(new uint8_t[(size_t)n * kb]);
  FILE* f = fopen(argv[5], "rb");
  if (!f || fread(keys.get(), (size_t)kb, (size_t)n, f) != (size_t)n) return 3;
  fclose(f);
  return kb == 96 ? run<96>(keys.get(), (uint32_t)n, slack_log, (uint32_t)probes) : run<48>(keys.get(), (uint32_t)n, slack_log, (uint32_t)probes);
}
