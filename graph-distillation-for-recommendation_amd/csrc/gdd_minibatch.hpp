// gdd_minibatch.hpp — the host-only part of MiniBatchKMeans.fit (no HIP, so a plain C++ program can
// test it: tests/host/mb_reassign_main.cpp): the device loop's state block, the fit's pinned staging
// layout, the device segment's step schedule and the host's reassignment decision.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "gdd.h"
#include "gdd_carve.hpp"
#include "gdd_rng.hpp"

namespace gdd {

// MiniBatchKMeans early stopping on the device (gdd_minibatch_state_bytes(), zero-initialised):
// _mini_batch_convergence's state and the two words the host loop reads back
struct MBState {
  double ewa, ewa_min;
  int32_t stop_at;  // 0 while running, s+1 once the test fired at step s
  int32_t has_ewa, has_min, no_improvement;
  int32_t handoff;  // s+1 once step s's reassignment needs the host (np.argsort branch)
  int32_t pad[3];
};
static_assert(offsetof(MBState, stop_at) == 16, "gdd.h documents stop_at at offset 16");
static_assert(offsetof(MBState, handoff) == 32 && sizeof(MBState) == 48, "MBState layout");

constexpr int64_t kMaxBatch = 13312;  // 12*b bytes of LDS per update block (<= 156 KiB)
// minibatch_step_dev flag: the step has no tail for step_i - 1 (the first step of a device segment
// resumed after host steps, whose convergence tests the host already ran)
constexpr int kStepNoTail = 1 << 16;

// ---- the fit's pinned staging (caller-owned, page-locked) ------------------------------------------
constexpr int kChunkCap = 64;  // host-loop steps whose batch indices are drawn and copied at once

struct FitHostWords {  // the small read-backs
  int32_t stop;         // MBState::stop_at alone
  float inertia;        // an initialisation's inertia on the validation set
  double ewa;           // MBState::ewa at the end
  MBState state;        // the whole block after a device segment
  int32_t chunk[4][4];  // per chunk in flight: stop_at .. no_improvement
  DevMT mt;             // the generator on its way to and from the device
};

struct FitHost {
  int64_t* rows;       // kChunkCap x bs batch indices (host segment)
  double* uniforms;    // (k - 1) x T k-means++ draws
  int64_t* init_idx;   // isz
  int64_t* val_idx;    // isz
  float* counts;       // k weight sums, read back at a host reassignment
  float* counts_new;   // k weight sums after it
  int64_t* pairs;      // k (cluster, batch position)
  FitHostWords* w;
};

// the layout, measured (null base) and carved by the same walk; returns the bytes it needs
inline size_t fit_host(void* base, size_t cap, int k, int64_t bs, int64_t isz, int T, FitHost* h) {
  Carver cv(base, cap);
  FitHost f;
  f.rows = cv.take<int64_t>((size_t)kChunkCap * bs);
  f.uniforms = cv.take<double>((size_t)std::max(k - 1, 1) * T);
  f.init_idx = cv.take<int64_t>(isz);
  f.val_idx = cv.take<int64_t>(isz);
  f.counts = cv.take<float>(k);
  f.counts_new = cv.take<float>(k);
  f.pairs = cv.take<int64_t>(2 * (size_t)k);
  f.w = cv.take<FitHostWords>(1);
  if (h) *h = f;
  return align256(cv.off);
}

// ---- the device segment's step schedule --------------------------------------------------------------
// Steps [i0, n_steps) on the device. rr_base: the last reassignment step (the next ones every
// ceil(10k / bs) steps from it); norms_valid0: the workspace norms match step i0's centres.
struct MbSegment {  // no padding: it is part of the graph-replay key
  int64_t i0, rr_base, n_steps, bs;
  int32_t k;
  float ratio;
  int32_t norms_valid0, pad;
};
static_assert(sizeof(MbSegment) == 48, "MbSegment has no padding");

struct MbSched {
  bool reassign, has_next;
  int flags;         // GDD_STEP_* | kStepNoTail
  int c, rows, mt;   // this step's C_old = C[c] (C_new the other), rows buffer, and generator slot
};

inline MbSched mb_schedule(const MbSegment& g, int64_t st) {
  // _random_reassign (:2029-2043): n_since grows by b per step and fires (then resets) at >= 10k,
  // i.e. every p = ceil(10k / b) steps; a reassignment leaves no zero count (gdd_fit.hip)
  const int64_t period = (10 * (int64_t)g.k + g.bs - 1) / g.bs;
  MbSched s;
  s.reassign = g.ratio > 0.f && st >= g.rr_base && (st - g.rr_base) % period == 0;
  s.has_next = st + 1 < g.n_steps;
  // only the segment's first step has no tail (its predecessor's convergence test ran on the host)
  s.flags = GDD_STEP_CONVERGE | ((st > g.i0 || g.norms_valid0) ? GDD_STEP_NORMS_VALID : 0) |
            ((st == g.i0 && g.i0 > 0) ? kStepNoTail : 0);
  s.c = (int)(st % 2);
  s.rows = (int)(st & 1);
  s.mt = (int)(st % 3);
  return s;
}

// one step as bits, for gdd_minibatch_schedule
inline int32_t mb_schedule_bits(const MbSched& s) {
  return (s.reassign ? GDD_SCHED_REASSIGN : 0) | (s.has_next ? GDD_SCHED_HAS_NEXT : 0) |
         ((s.flags & GDD_STEP_NORMS_VALID) ? GDD_SCHED_NORMS_VALID : 0) |
         ((s.flags & kStepNoTail) ? GDD_SCHED_NO_TAIL : 0) | (s.c << 4) | (s.rows << 5) | (s.mt << 6);
}

// ---- the host's reassignment decision ---------------------------------------------------------------
// _mini_batch_step's reassignment branch (:1640-1667) after the step's update, numpy float32
// semantics: the centres below ratio x max, the argsort branch when more than b/2 of them are due,
// the permutation draw (only when some centre is due), and the weight-sum fill with the minimum of
// the others. pairs[2q], pairs[2q + 1]: the q-th reassigned cluster and the batch position of its new
// centre. Returns the number of pairs, or -1 where the argsort branch has no callback.
inline int64_t mb_reassign_decide(const float* counts, int k, int64_t bs, float ratio, LegacyRNG& rng,
                                  void (*argsort_cb)(const float*, int64_t, int64_t*), int64_t* pairs,
                                  float* counts_new, bool* any_zero) {
  float wmax = counts[0];
  for (int c = 1; c < k; ++c) wmax = std::max(wmax, counts[c]);
  const float thr = ratio * wmax;
  std::vector<char> to(k);
  int64_t cnt = 0;
  for (int c = 0; c < k; ++c) cnt += to[c] = counts[c] < thr;
  if ((double)cnt > 0.5 * (double)bs) {
    if (!argsort_cb) return -1;
    std::vector<int64_t> order(k);
    argsort_cb(counts, k, order.data());  // np.argsort(weight_sums) (quicksort order)
    for (int64_t q = (int64_t)(0.5 * (double)bs); q < k; ++q) to[order[q]] = 0;
    cnt = 0;
    for (int c = 0; c < k; ++c) cnt += to[c];
  }
  if (cnt) {
    const std::vector<int64_t> perm = rng.permutation(bs);  // choice(bs, replace=False, size=cnt)
    int64_t q = 0;
    for (int c = 0; c < k; ++c)
      if (to[c]) {
        pairs[2 * q] = c;
        pairs[2 * q + 1] = perm[q];
        ++q;
      }
  }
  float mn = 0.f;
  bool first_min = true;
  for (int c = 0; c < k; ++c)
    if (!to[c] && (first_min || counts[c] < mn)) {
      mn = counts[c];
      first_min = false;
    }
  *any_zero = false;
  for (int c = 0; c < k; ++c) {
    counts_new[c] = to[c] ? mn : counts[c];
    *any_zero |= counts_new[c] == 0.f;
  }
  return cnt;
}

}  // namespace gdd
