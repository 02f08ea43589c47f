// Stand-alone address / undefined-behaviour check of the many-lane input sum of csrc/groth16_verify.h (tests/test_groth16_wide_host.py
// builds it with -fsanitize=address,undefined and runs it as a subprocess): g16_lane_sum and the fold through L / 2 slots as
// k_g16_inputs_lanes<G16Bls> walks them, at L = 256 with 130 inputs (lanes 130 .. 255 carry the identity), every buffer a heap array of
// its exact size.
//   argv[1]: a file of 131 gamma_abc rows (12 u64 each, affine arkworks limbs) followed by 130 inputs (4 u64 each, canonical)
// Prints the sum as 12 hexadecimal u64 (a zero row for the identity), the one-lane sum of g16_input_row likewise, and "g16 lanes ok" when
// the two agree.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include "groth16_verify.h"

using namespace celo;
typedef G16Bls C;
typedef C::F F;

static void print_row(const Xyzz<F>& a) {
  uint64_t row[12] = {};
  Affine<F> r;
  if (fb_to_affine(a, r)) { r.x.to_ark(row); r.y.to_ark(row + 6); }
  for (int k = 0; k < 12; k++) printf("%016llx%c", (unsigned long long)row[k], k == 11 ? '\n' : ' ');
}

int main(int argc, char** argv) {
  constexpr uint32_t N_IN = 130, L = 256;
  constexpr int c = 4, FW = F::WORDS;
  if (argc != 2) return 2;
  const size_t n_u64 = (size_t)(N_IN + 1) * 12 + (size_t)N_IN * 4;
  std::unique_ptr<uint64_t[]> in(new uint64_t[n_u64]);
  FILE* f = fopen(argv[1], "rb");
  if (!f || fread(in.get(), 8, n_u64, f) != n_u64) return 3;
  fclose(f);
  const uint64_t *abc = in.get(), *x = in.get() + (size_t)(N_IN + 1) * 12;
  const int W = fb_windows(C::SCALAR_BITS, c);
  const uint32_t H = 1u << (c - 1), E = (uint32_t)W * H;
  std::unique_ptr<uint32_t[]> table(new uint32_t[(size_t)N_IN * E * 2 * FW]), abc0(new uint32_t[2 * FW]);
  std::unique_ptr<uint8_t[]> tinf(new uint8_t[(size_t)N_IN * E]);
  fb_store_entry(abc0.get(), Affine<F>{F::norm(F::from_ark(abc)), F::norm(F::from_ark(abc + 6))});
  for (size_t j = 0; j < N_IN; j++) {
    const uint64_t* gen = abc + (j + 1) * 12;
    const Affine<F> g = {F::norm(F::from_ark(gen)), F::norm(F::from_ark(gen + 6))};
    for (int w = 0; w < W; w++) {
      Affine<F> b = {F::zero(), F::zero()};
      const bool okb = fb_to_affine(fb_window_base(g, w, c), b);
      for (uint32_t d = 1; d <= H; d++) {
        const size_t e = j * E + (size_t)w * H + d - 1;
        Affine<F> r = {F::zero(), F::zero()};
        const bool ok = okb && fb_to_affine(fb_table_entry(b, d), r);
        fb_store_entry(&table[e * 2 * FW], r);
        tinf[e] = ok ? 0 : 1;
      }
    }
  }
  // phase 1, then the rounds: lanes [s, 2 s) store into slot lane - s, lanes [0, s) add slot lane
  const size_t SW = agg_slot_words<F>();
  std::unique_ptr<Xyzz<F>[]> acc(new Xyzz<F>[L]);
  std::unique_ptr<uint4[]> slots(new uint4[(L / 2) * SW / 4]);
  uint32_t* sl = reinterpret_cast<uint32_t*>(slots.get());
  uint32_t bad = 0;
  for (uint32_t l = 0; l < L; l++) {
    uint32_t b = 0;
    acc[l] = g16_lane_sum<C>(x, N_IN, l, L, abc0.get(), false, table.get(), tinf.get(), c, W, &b);
    bad |= b;
  }
  for (uint32_t s = L >> 1; s; s >>= 1) {
    for (uint32_t l = s; l < 2 * s; l++) g16_fold_put<F>(sl, acc[l], l, s);
    for (uint32_t l = 0; l < s; l++) g16_fold_take<F>(acc[l], sl, l);
  }
  uint32_t bad1 = 0;
  const Xyzz<F> one = g16_input_row<C>(x, N_IN, abc0.get(), false, table.get(), tinf.get(), c, W, &bad1);
  print_row(acc[0]);
  print_row(one);
  Affine<F> p, q;
  const bool ip = fb_to_affine(acc[0], p), iq = fb_to_affine(one, q);
  uint64_t rp[12] = {}, rq[12] = {};
  if (ip) { p.x.to_ark(rp); p.y.to_ark(rp + 6); }
  if (iq) { q.x.to_ark(rq); q.y.to_ark(rq + 6); }
  for (int k = 0; k < 12; k++) if (rp[k] != rq[k]) return 4;
  if (ip != iq || bad != bad1) return 5;
  printf("bad=%u\ng16 lanes ok\n", bad);
  return 0;
}
