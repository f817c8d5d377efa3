// A plain C++ program over the host-only headers of MiniBatchKMeans.fit (gdd_minibatch.hpp, gdd_rng.hpp,
// gdd_carve.hpp): the host's reassignment decision on the cases of tests/test_minibatch_plan_host.py,
// each checked against the rule restated here, and the pinned staging layout's carve (every field inside
// the buffer, none overlapping). Built with -fsanitize=address,undefined by that test and run directly.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <utility>
#include <vector>

#include "gdd_minibatch.hpp"

using namespace gdd;

#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::printf("%s:%d: %s failed\n", __FILE__, __LINE__, #cond);   \
      std::exit(1);                                                   \
    }                                                                 \
  } while (0)

static int g_argsorts = 0;
static void argsort(const float* w, int64_t k, int64_t* out) {  // a stable order: ties by index
  ++g_argsorts;
  std::iota(out, out + k, (int64_t)0);
  std::stable_sort(out, out + k, [w](int64_t a, int64_t b) { return w[a] < w[b]; });
}

static MTState seeded(uint32_t seed) {  // init_genrand
  MTState s{};
  s.key[0] = seed;
  for (int i = 1; i < 624; ++i) s.key[i] = 1812433253u * (s.key[i - 1] ^ (s.key[i - 1] >> 30)) + (uint32_t)i;
  s.pos = 624;
  return s;
}

static void decision(const std::vector<float>& counts, int64_t bs, bool want_argsort) {
  const int k = (int)counts.size();
  const float ratio = 0.01f;
  const float thr = ratio * *std::max_element(counts.begin(), counts.end());
  std::vector<char> to(k);
  int64_t due = 0;
  for (int c = 0; c < k; ++c) due += to[c] = counts[c] < thr;
  CHECK((2 * due > bs) == want_argsort);
  if (want_argsort) {  // the bs / 2 smallest stay due
    std::vector<int64_t> order(k);
    argsort(counts.data(), k, order.data());
    --g_argsorts;
    for (int64_t q = bs / 2; q < k; ++q) to[order[q]] = 0;
    due = std::count(to.begin(), to.end(), 1);
  }
  MTState st = seeded(5), st_ref = st;
  LegacyRNG rng(&st), rng_ref(&st_ref);
  std::vector<int64_t> pairs(2 * (size_t)k, -1);
  std::vector<float> out(k, -1.f);
  bool any_zero = false;
  const int before = g_argsorts;
  const int64_t n = mb_reassign_decide(counts.data(), k, bs, ratio, rng, argsort, pairs.data(), out.data(), &any_zero);
  CHECK(n == due);
  CHECK((g_argsorts - before == 1) == want_argsort);
  std::vector<int64_t> perm;
  if (due) perm = rng_ref.permutation(bs);
  CHECK(std::equal(st.key, st.key + 624, st_ref.key) && st.pos == st_ref.pos);  // drawn only when some are due
  float mn = INFINITY;
  for (int c = 0; c < k; ++c)
    if (!to[c]) mn = std::min(mn, counts[c]);
  bool zero = false;
  int64_t q = 0;
  for (int c = 0; c < k; ++c) {
    CHECK(out[c] == (to[c] ? mn : counts[c]));
    zero |= out[c] == 0.f;
    if (to[c]) {
      CHECK(pairs[2 * q] == c && pairs[2 * q + 1] == perm[q]);
      ++q;
    }
  }
  CHECK(any_zero == zero);
}

static void layout(int k, int64_t bs, int64_t isz, int T) {
  const size_t need = fit_host(nullptr, 0, k, bs, isz, T, nullptr);
  std::vector<char> buf(need);
  FitHost h;
  CHECK(fit_host(buf.data(), need, k, bs, isz, T, &h) == need);
  const size_t u = (size_t)std::max(k - 1, 1) * T;
  std::vector<std::pair<char*, size_t>> f = {
      {(char*)h.rows, 8 * (size_t)kChunkCap * bs}, {(char*)h.uniforms, 8 * u}, {(char*)h.init_idx, 8 * (size_t)isz},
      {(char*)h.val_idx, 8 * (size_t)isz},         {(char*)h.counts, 4 * (size_t)k}, {(char*)h.counts_new, 4 * (size_t)k},
      {(char*)h.pairs, 16 * (size_t)k},            {(char*)h.w, sizeof(FitHostWords)}};
  std::sort(f.begin(), f.end());
  for (size_t i = 0; i < f.size(); ++i) {
    CHECK(f[i].first >= buf.data() && f[i].first + f[i].second <= buf.data() + need);
    CHECK((f[i].first - buf.data()) % 256 == 0);
    if (i) CHECK(f[i - 1].first + f[i - 1].second <= f[i].first);
    std::fill(f[i].first, f[i].first + f[i].second, (char)i);  // every byte is the buffer's own
  }
  // the words' own fields, in the struct and apart
  FitHostWords* w = h.w;
  CHECK((char*)&w->mt + sizeof(DevMT) <= (char*)w + sizeof(FitHostWords));
  CHECK((char*)&w->state >= (char*)&w->ewa + sizeof(double) && (char*)w->chunk >= (char*)&w->state + sizeof(MBState));
  CHECK((char*)&w->mt >= (char*)w->chunk + sizeof(w->chunk) && sizeof(w->chunk) == 64);
}

int main() {
  std::vector<float> big(40);
  for (int c = 0; c < 40; ++c) big[c] = 50.f + (float)((c * 37) % 40);
  decision(big, 1000, false);  // nothing due
  std::vector<float> some = big;
  some[2] = 0.f, some[9] = 0.25f, some[31] = 0.5f;
  decision(some, 1000, false);
  std::vector<float> half(big.begin(), big.begin() + 20), over = half, left = big;
  std::fill(half.begin(), half.begin() + 10, 0.f);  // b = 20: exactly int(0.5 b) due
  decision(half, 20, false);
  std::fill(over.begin(), over.begin() + 11, 0.f);  // one more: the argsort branch
  decision(over, 20, true);
  std::vector<float> ties(40, 64.f);
  ties[0] = 6400.f;
  ties[4] = ties[5] = 0.01f * 6400.f;  // at the threshold: not below it
  ties[6] = std::nextafter(ties[4], 0.f);
  decision(ties, 1000, false);
  decision(std::vector<float>(17, 5.f), 1000, false);  // all equal
  std::fill(left.begin(), left.begin() + 30, 0.f);  // zeros left after the argsort branch
  decision(left, 20, true);
  decision(std::vector<float>{3.f}, 7, false);  // k = 1
  layout(454, 1000, 3000, 8);  // arxiv
  layout(769, 1000, 3000, 8);  // Reddit
  layout(50, 50, 50, 5);
  layout(1, 1, 1, 2);
  std::printf("ok\n");
  return 0;
}
