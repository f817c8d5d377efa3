// gdd_fit.hip — native host loop of MiniBatchKMeans.fit (sklearn/cluster/_kmeans.py:2046-2200).
//
// One fit is a sequence of phases over one context (struct Fit): the initialisation, then device
// segments (draws, scheduled reassignments and the convergence test on the device, one host round
// trip per 16-step chunk) and, where a reassignment needs np.argsort, a hand-off step and host-driven
// steps (numpy-legacy draws from gdd_rng.hpp, chunked H2D of the batch indices through pinned
// memory, the O(k) decision of gdd_minibatch.hpp, one sync per reassignment step), then the finish.
// Draw order, reassignment rule, early-stopping and the RNG state left behind are sklearn's (one
// OpenMP thread). DESIGN.md §4 (MiniBatch update, convergence, reassignment) names the paths.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gdd_common.hpp"
#include "gdd_devrng.hpp"
#include "gdd_rng.hpp"

namespace gdd {
namespace {

__global__ void k_gather_rows(int64_t m, int dim, const float* __restrict__ X,
                              const int64_t* __restrict__ idx, float* __restrict__ out) {
  const int64_t total = m * dim;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = t / dim;
    out[t] = X[idx[r] * dim + (t - r * dim)];
  }
}

// C[dst[j]] = X[rows[src[j]]]  (centers_new[to_reassign] = X_batch[new_centers], :1655-1662)
__global__ void k_reassign_rows(int m, int dim, const float* __restrict__ X,
                                const int64_t* __restrict__ rows, const int64_t* __restrict__ pairs,
                                float* __restrict__ C) {
  const int j = blockIdx.x;
  if (j >= m) return;
  const int64_t dst = pairs[2 * j], src = rows[pairs[2 * j + 1]];
  for (int f = threadIdx.x; f < dim; f += blockDim.x) C[dst * dim + f] = X[src * dim + f];
}

struct FitWs {
  float* Xi;
  void* kpp_ws;
  size_t kpp_bytes;
  void* step_ws;
  size_t step_bytes;
  MBState* state;
  float* counts;
  float* C[2];
  int64_t* rows_d;
  int32_t* labels_b;
  int64_t* pairs;
  double* uniforms;
  int64_t* init_idx;
  int64_t* val_idx;
  int32_t* val_labels;
  float* val_sq;
  float* sq;
  float* scalar;
  void* assign_ws;
  size_t assign_bytes;
  DevMT* mtb;  // 3 device MT states: slot s % 3 = the generator after step s's draws
};

size_t fit_ws(void* base, size_t cap, int64_t n, int dim, int k, int64_t bs, int64_t isz, int T,
              FitWs* w) {
  Carver cv(base, cap);
  FitWs f;
  f.Xi = cv.take<float>((size_t)isz * dim);
  f.kpp_bytes = gdd_kmeans_plusplus_ws_bytes_k(isz, dim, T, k);
  f.kpp_ws = cv.take<char>(f.kpp_bytes);
  f.step_bytes = gdd_minibatch_step_ws_bytes(bs, k);
  f.step_ws = cv.take<char>(f.step_bytes);
  f.state = cv.take<MBState>(1);
  f.counts = cv.take<float>(k);
  f.C[0] = cv.take<float>((size_t)k * dim);
  f.C[1] = cv.take<float>((size_t)k * dim);
  f.rows_d = cv.take<int64_t>((size_t)kChunkCap * bs);
  f.labels_b = cv.take<int32_t>(bs);
  f.pairs = cv.take<int64_t>(2 * (size_t)k);
  f.uniforms = cv.take<double>((size_t)std::max(k - 1, 1) * T);
  f.init_idx = cv.take<int64_t>(isz);
  f.val_idx = cv.take<int64_t>(isz);
  f.val_labels = cv.take<int32_t>(isz);
  f.val_sq = cv.take<float>(isz);
  f.sq = cv.take<float>(n);
  f.scalar = cv.take<float>(4);
  f.assign_bytes = gdd_kmeans_assign_ws_bytes(std::max(n, isz));
  f.assign_ws = cv.take<char>(f.assign_bytes);
  f.mtb = cv.take<DevMT>(3);
  if (w) *w = f;
  return cv.off + 1024;
}

int local_trials(int k) { return 2 + (int)std::log((double)k); }

// The loop a fit takes (gdd_minibatch_fit_path names it). Device-resident (any k whose reassignment
// swap table fits the LDS): the batch draws, the scheduled reassignments and the convergence test
// run on the device with one host round trip per chunk of steps (overlapped with the next chunk).
enum FitPath { FIT_INVALID, FIT_HOST, FIT_DEV_CHAIN, FIT_DEV_PAR };

FitPath fit_path(int64_t n, int dim, int k, int64_t batch_size) {
  if (!(n > 0 && dim > 0 && dim <= 512 && k > 0 && k <= n && batch_size > 0)) return FIT_INVALID;
  const MbStepPlan p = mb_step_plan(std::min(batch_size, n), dim, k, 0);
  if (!p.ok || local_trials(k) > 16) return FIT_INVALID;
  if (getenv("GDD_HOST_LOOP") != nullptr || p.rs_form < 0) return FIT_HOST;
  return p.rs_form == kRsParCopy ? FIT_DEV_PAR : FIT_DEV_CHAIN;
}

// one fit: the call's shapes and buffers, then the step loop's variables
struct Fit {
  int64_t n;
  int dim;
  const float* X;
  int k;
  int64_t bs, isz;
  int T, n_init;
  int64_t n_steps;
  float ratio;
  void (*argsort_cb)(const float*, int64_t, int64_t*);
  MTState* rng_state;
  LegacyRNG rng;
  gdd_stream_t stream;
  hipStream_t s;
  bool dev_ok;
  FitWs w;
  FitHost h;
  MbStep mb;
  int64_t i = 0;           // the next step
  int64_t stop_step = -1;  // the step the convergence test stopped at
  int64_t rr_base = 0;     // the last reassignment step
  int64_t n_since = 0;     // _random_reassign's sample count since then (host segments)
  bool any_zero = true;    // some weight sum is zero: sklearn reassigns at every such step
  bool norms_valid = false;  // the workspace norms match the next step's centres
};

// ---- validation subset and initialisations (:2128-2163) ----------------------------------------
int fit_init(Fit& f) {
  const FitWs& w = f.w;
  const int64_t n = f.n, isz = f.isz;
  const int k = f.k, dim = f.dim, T = f.T;
  hipStream_t s = f.s;
  f.rng.randint(0, n, isz, f.h.val_idx);  // validation_indices
  GDD_HIP(hipMemcpyAsync(w.val_idx, f.h.val_idx, sizeof(int64_t) * isz, hipMemcpyHostToDevice, s));
  float best_inertia = 0.f;
  bool have_best = false;
  for (int init = 0; init < f.n_init; ++init) {
    const float* Xi = f.X;
    if (isz < n) {
      f.rng.randint(0, n, isz, f.h.init_idx);
      GDD_HIP(hipMemcpyAsync(w.init_idx, f.h.init_idx, sizeof(int64_t) * isz, hipMemcpyHostToDevice, s));
      k_gather_rows<<<(unsigned)std::min<int64_t>((isz * dim + 255) / 256, 4096), 256, 0, s>>>(
          isz, dim, f.X, w.init_idx, w.Xi);
      GDD_LAUNCHED();
      Xi = w.Xi;
    }
    const int64_t first = f.rng.choice_uniform_weights(isz);
    for (int c = 0; c < k - 1; ++c)
      for (int t = 0; t < T; ++t) f.h.uniforms[(size_t)c * T + t] = f.rng.next_double();
    if (k > 1)
      GDD_HIP(hipMemcpyAsync(w.uniforms, f.h.uniforms, sizeof(double) * (size_t)(k - 1) * T,
                             hipMemcpyHostToDevice, s));
    float* cand = (f.n_init > 1 && init > 0) ? w.C[1] : w.C[0];
    int rc = gdd_kmeans_plusplus(isz, dim, Xi, nullptr, k, T, first, w.uniforms, cand, w.init_idx,
                                 w.kpp_ws, w.kpp_bytes, f.stream);
    if (rc) return rc;
    if (f.n_init > 1) {  // inertia on the validation set (_labels_inertia_threadpool_limit)
      rc = gdd_row_norms(k, dim, cand, reinterpret_cast<float*>(w.pairs), f.stream);
      if (rc) return rc;
      rc = gdd_kmeans_assign(isz, dim, f.X, w.val_idx, k, cand, reinterpret_cast<float*>(w.pairs),
                             w.val_labels, w.val_sq, w.assign_ws, w.assign_bytes, f.stream);
      if (rc) return rc;
      rc = gdd_inertia(isz, w.val_sq, nullptr, w.scalar, f.stream);
      if (rc) return rc;
      GDD_HIP(hipMemcpyAsync(&f.h.w->inertia, w.scalar, sizeof(float), hipMemcpyDeviceToHost, s));
      GDD_HIP(hipStreamSynchronize(s));
      const float inertia = f.h.w->inertia;
      if (!have_best || inertia < best_inertia) {
        best_inertia = inertia;
        have_best = true;
        if (cand != w.C[0])
          GDD_HIP(hipMemcpyAsync(w.C[0], cand, sizeof(float) * (size_t)k * dim,
                                 hipMemcpyDeviceToDevice, s));
      }
    }
  }
  GDD_HIP(hipMemsetAsync(w.counts, 0, sizeof(float) * k, s));
  GDD_HIP(hipMemsetAsync(w.state, 0, sizeof(MBState), s));
  return GDD_OK;
}

// the device's state block read back into the pinned mirror (with the weight sums, for a host
// reassignment), and the stream drained
int read_state(Fit& f, bool with_counts) {
  GDD_HIP(hipMemcpyAsync(&f.h.w->state, f.w.state, sizeof(MBState), hipMemcpyDeviceToHost, f.s));
  if (with_counts)
    GDD_HIP(hipMemcpyAsync(f.h.counts, f.w.counts, sizeof(float) * f.k, hipMemcpyDeviceToHost, f.s));
  GDD_HIP(hipStreamSynchronize(f.s));
  return GDD_OK;
}

// _mini_batch_step's reassignment branch on the host after the step's update (read_state has the
// weight sums): the decision (mb_reassign_decide), then the row copies and the weight-sum reset
int host_reassign(Fit& f, const int64_t* rows, float* c_new) {
  const int64_t cnt = mb_reassign_decide(f.h.counts, f.k, f.bs, f.ratio, f.rng, f.argsort_cb, f.h.pairs,
                                         f.h.counts_new, &f.any_zero);
  if (cnt < 0) return fail(GDD_E_INVALID, "mbk_fit: argsort callback required (k > b/2)");
  if (cnt) {
    GDD_HIP(hipMemcpyAsync(f.w.pairs, f.h.pairs, sizeof(int64_t) * 2 * cnt, hipMemcpyHostToDevice, f.s));
    k_reassign_rows<<<(unsigned)cnt, 64, 0, f.s>>>((int)cnt, f.dim, f.X, rows, f.w.pairs, c_new);
    GDD_LAUNCHED();
    f.norms_valid = false;  // reassigned rows: the next step recomputes the norms
  }
  GDD_HIP(hipMemcpyAsync(f.w.counts, f.h.counts_new, sizeof(float) * f.k, hipMemcpyHostToDevice, f.s));
  return GDD_OK;
}

// The step loop with every draw and decision on the device. Per step s: the assignment launch (plus
// a workgroup finishing step s-1 — its batch inertia and convergence test — and, unless s
// reassigns, a workgroup drawing batch s+1), the update launch, and at scheduled reassignment steps
// the reassignment launch (which then draws batch s+1). Chunks of kDevChunk steps are enqueued back
// to back; the host reads the stop word of chunk c while chunk c+1 runs. Smaller chunks leave fewer
// no-op launches after the stop but give the host a shorter runway: 8, 12 and 16 measured equal
// within the box's noise, 4 slower.
constexpr int kDevChunk = 16;

// the launches of steps [c0, c0 + m) of segment g: every argument follows from mb_schedule and the
// fit's buffers
int enqueue_steps(const Fit& f, const MbSegment& g, int64_t c0, int64_t m, hipStream_t cs) {
  const FitWs& w = f.w;
  for (int64_t st = c0; st < c0 + m; ++st) {
    const MbSched q = mb_schedule(g, st);
    const int64_t* rows = w.rows_d + q.rows * f.bs;
    DevMT* mt = w.mtb + q.mt;
    // the next batch into the other rows buffer, the generator after it into the next slot
    const RngNext next =
        q.has_next ? RngNext{mt, w.mtb + (q.mt + 1) % 3, w.rows_d + (q.rows ^ 1) * f.bs, f.n, f.bs} : RngNext{};
    float* c_new = w.C[q.c ^ 1];
    int rc = minibatch_step_dev(f.mb, f.X, rows, w.C[q.c], c_new, w.counts, w.labels_b, (int)st, q.flags,
                                next, cs);  // at reassignment steps: a speculative draw
    if (rc) return rc;
    if (q.reassign) {
      rc = mb_reassign_launch(f.mb, (int)st, f.ratio, f.X, rows, c_new, w.counts, mt, mt, next, cs);
      if (rc) return rc;
    }
    if (!q.has_next) {  // the last step's inertia and convergence test (otherwise in step st + 1)
      rc = mb_loop_end(f.mb, (int)st, cs);
      if (rc) return rc;
    }
  }
  return GDD_OK;
}

// Steps [f.i, n_steps) on the device. Ends at the last step, at the convergence stop (f.stop_step)
// or at *handoff_step, a step whose reassignment needs the host (more than b/2 centres due:
// np.argsort's branch) — that step's update has run, its tail and reassignment have not, and the
// generator (written back to the caller's) is after its batch draws.
int fit_device_segment(Fit& f, int64_t* handoff_step) {
  const FitWs& w = f.w;
  hipStream_t s = f.s;
  MbSegment seg{};
  seg.i0 = f.i, seg.rr_base = f.rr_base, seg.n_steps = f.n_steps, seg.bs = f.bs;
  seg.k = f.k, seg.ratio = f.ratio, seg.norms_valid0 = f.norms_valid ? 1 : 0;
  // the host RNG state (after the initialisation draws, or after the host's step i0 - 1) becomes
  // the device slot of step i0 - 1
  DevMT* h_mt = &f.h.w->mt;
  std::memcpy(h_mt->key, f.rng_state->key, sizeof(h_mt->key));
  h_mt->pos = f.rng_state->pos;
  h_mt->pad = 0;
  DevMT* mt_prev = w.mtb + (seg.i0 + 2) % 3;
  GDD_HIP(hipMemcpyAsync(mt_prev, h_mt, sizeof(DevMT), hipMemcpyHostToDevice, s));
  int rc = mb_rng_launch(mt_prev, w.mtb + seg.i0 % 3, f.n, f.bs, w.rows_d + (seg.i0 & 1) * f.bs, s);
  if (rc) return rc;
  rc = mb_loop_begin(f.mb, s);
  if (rc) return rc;
  // one chunk in flight before the host waits for the oldest one's stop word (two or three measured
  // equal: each extra chunk only adds a chunk of no-op launches after a stop)
  constexpr int lookahead = 1;
  hipEvent_t ev[4];
  for (int q = 0; q < 4; ++q) GDD_HIP(hipEventCreateWithFlags(&ev[q], hipEventDisableTiming));
  struct EvGuard {
    hipEvent_t* e;
    ~EvGuard() {
      for (int q = 0; q < 4; ++q) (void)hipEventDestroy(e[q]);
    }
  } guard{ev};
  // a chunk is replayed as a recorded graph (replay_or_run) keyed by everything its launches' arguments
  // follow from: the buffers, the shapes, the segment and the chunk's steps
  struct {
    const void* ptr[9];
    MbSegment seg;
    int64_t n, dim, max_ni, step_bytes, c0, m;
  } key;
  std::memset(&key, 0, sizeof(key));
  const void* ptrs[9] = {f.X, w.rows_d, w.C[0], w.C[1], w.counts, w.labels_b, w.state, w.step_ws, w.mtb};
  std::memcpy(key.ptr, ptrs, sizeof(ptrs));
  key.seg = seg;
  key.n = f.n, key.dim = f.dim, key.max_ni = f.mb.max_ni, key.step_bytes = (int64_t)w.step_bytes;
  int64_t i = seg.i0, chunk = 0;
  while (i < f.n_steps) {
    const int64_t m = std::min<int64_t>(kDevChunk, f.n_steps - i);
    key.c0 = i, key.m = m;
    rc = replay_or_run("minibatch_chunk", &key, sizeof(key), s,
                       [&](hipStream_t cs) { return enqueue_steps(f, seg, i, m, cs); });
    if (rc) return rc;
    i += m;
    // this chunk's stop word and no-improvement count, read back while the next chunks run
    const int slot = (int)(chunk & 3);
    GDD_HIP(hipMemcpyAsync(f.h.w->chunk[slot], &w.state->stop_at, sizeof(f.h.w->chunk[slot]),
                           hipMemcpyDeviceToHost, s));
    GDD_HIP(hipEventRecord(ev[slot], s));
    if (chunk >= lookahead) {
      const int old = (int)((chunk - lookahead) & 3);
      GDD_HIP(hipEventSynchronize(ev[old]));
      if (f.h.w->chunk[old][0]) break;  // the later kernels already enqueued are no-ops
    }
    ++chunk;
  }
  rc = read_state(f, false);
  if (rc) return rc;
  const MBState& st = f.h.w->state;
  *handoff_step = -1;
  if (st.handoff && st.handoff == st.stop_at)
    *handoff_step = st.handoff - 1;
  else if (st.stop_at)
    f.stop_step = st.stop_at - 1;
  const int64_t last = *handoff_step >= 0 ? *handoff_step : (f.stop_step >= 0 ? f.stop_step : f.n_steps - 1);
  // the caller's RandomState ends where sklearn's does: after the draws of the last step (at a
  // handoff: after that step's batch draws, before its reassignment's)
  GDD_HIP(hipMemcpyAsync(h_mt, w.mtb + last % 3, sizeof(DevMT), hipMemcpyDeviceToHost, s));
  GDD_HIP(hipStreamSynchronize(s));
  std::memcpy(f.rng_state->key, h_mt->key, sizeof(h_mt->key));
  f.rng_state->pos = h_mt->pos;
  return GDD_OK;
}

// Step h, handed over by the device: its update ran there; its convergence test (the tail the next
// launch would have run) and its reassignment run here, in sklearn's order of effects. The host
// then runs steps while some weight sum is zero (sklearn reassigns at every such step).
int fit_handoff(Fit& f, int64_t h) {
  const FitWs& w = f.w;
  GDD_HIP(hipMemsetAsync(&w.state->stop_at, 0, sizeof(int32_t), f.s));
  GDD_HIP(hipMemsetAsync(&w.state->handoff, 0, sizeof(int32_t), f.s));
  int rc = mb_loop_end(f.mb, (int)h, f.s);
  if (rc) return rc;
  rc = read_state(f, true);
  if (rc) return rc;
  const int32_t stop_at = f.h.w->state.stop_at;
  f.norms_valid = true;  // the device update left ||C_new||^2 behind
  rc = host_reassign(f, w.rows_d + (h & 1) * f.bs, w.C[(h + 1) % 2]);
  if (rc) return rc;
  GDD_HIP(hipStreamSynchronize(f.s));  // the pinned staging's H2D copies are done
  if (stop_at) f.stop_step = stop_at - 1;  // converged at h (after its reassignment, as sklearn)
  f.i = h + 1;
  f.n_since = 0;
  f.rr_base = h;
  return GDD_OK;
}

// Host-driven steps from f.i: the batch draws of up to kChunkCap steps (to the next reassignment
// step) copied at once, one sync per reassignment step and one per chunk. *resume_dev: no weight sum
// is left at zero, so the next reassignments are periodic again.
int fit_host_segment(Fit& f, bool* resume_dev) {
  const FitWs& w = f.w;
  hipStream_t s = f.s;
  const MTState snapshot = *f.rng_state;
  std::vector<char> chunk_rr;
  while (f.i + (int64_t)chunk_rr.size() < f.n_steps && (int)chunk_rr.size() < kChunkCap) {
    f.rng.randint(0, f.n, f.bs, f.h.rows + chunk_rr.size() * f.bs);
    f.n_since += f.bs;
    const bool rr = f.any_zero || f.n_since >= 10 * (int64_t)f.k;  // _random_reassign (:2029-2043)
    if (rr) f.n_since = 0;
    chunk_rr.push_back(rr ? 1 : 0);
    if (rr) break;
  }
  const int m = (int)chunk_rr.size();
  // the previous chunk's copy has been consumed (stream order) before we overwrite h.rows: the
  // sync at the end of every chunk guarantees it
  GDD_HIP(hipMemcpyAsync(w.rows_d, f.h.rows, sizeof(int64_t) * (size_t)m * f.bs, hipMemcpyHostToDevice, s));
  *resume_dev = false;
  for (int j = 0; j < m; ++j) {
    const int64_t st = f.i + j;
    float* c_new = w.C[(st + 1) % 2];
    const int64_t* rows = w.rows_d + (size_t)j * f.bs;
    const int flags = GDD_STEP_CONVERGE | (f.norms_valid ? GDD_STEP_NORMS_VALID : 0);
    int rc = mb_step_run(f.mb, f.X, rows, w.C[st % 2], c_new, w.counts, w.labels_b, (int)st, flags, s);
    if (rc) return rc;
    f.norms_valid = true;  // the step left ||c_new||^2 behind
    if (chunk_rr[j] && f.ratio > 0.f) {
      rc = read_state(f, true);
      if (rc) return rc;
      const int32_t stop_at = f.h.w->state.stop_at;
      if (stop_at && stop_at - 1 < st) {  // stopped earlier in this chunk: step st never ran
        f.stop_step = stop_at - 1;
        break;
      }
      rc = host_reassign(f, rows, c_new);
      if (rc) return rc;
      if (stop_at) f.stop_step = stop_at - 1;
      if (stop_at == 0 && !f.any_zero && f.dev_ok) {
        *resume_dev = true;
        f.rr_base = st;
      }
    }
  }
  if (f.stop_step < 0) {
    const int rc = read_state(f, false);
    if (rc) return rc;
    if (f.h.w->state.stop_at) f.stop_step = f.h.w->state.stop_at - 1;
  } else {
    // also after a reassignment step's sync: its H2D copies out of the caller's pinned staging
    // (pairs, counts_new) are still queued, and that buffer may be reused once we return
    GDD_HIP(hipStreamSynchronize(s));
  }
  if (f.stop_step >= 0 && f.stop_step < f.i + m - 1) {
    // sklearn drew batch indices only up to the stopping step: rewind the generator
    *f.rng_state = snapshot;
    for (int64_t q = f.i; q <= f.stop_step; ++q) f.rng.randint(0, f.n, f.bs, f.h.rows);
  }
  f.i += m;
  *resume_dev = *resume_dev && f.stop_step < 0;
  return GDD_OK;
}

// centres out, the final labels pass + inertia (:2191-2197), the EWA
int fit_finish(Fit& f, int compute_labels, float* centers_out, int32_t* labels_out, float* inertia_out,
               int64_t* n_steps_out, double* ewa_out) {
  const FitWs& w = f.w;
  const int64_t n = f.n;
  const int64_t last = f.stop_step >= 0 ? f.stop_step : f.n_steps - 1;
  *n_steps_out = last + 1;
  const float* C = w.C[(last + 1) % 2];
  GDD_HIP(hipMemcpyAsync(centers_out, C, sizeof(float) * (size_t)f.k * f.dim, hipMemcpyDeviceToDevice, f.s));
  if (compute_labels) {
    int rc = gdd_row_norms(f.k, f.dim, C, reinterpret_cast<float*>(w.pairs), f.stream);
    if (rc) return rc;
    rc = gdd_kmeans_assign(n, f.dim, f.X, nullptr, f.k, C, reinterpret_cast<float*>(w.pairs), labels_out,
                           w.sq, w.assign_ws, w.assign_bytes, f.stream);
    if (rc) return rc;
    if (compute_labels == 2) {  // per-sample squared distances for the caller's own inertia fold
      GDD_HIP(hipMemcpyAsync(inertia_out, w.sq, sizeof(float) * (size_t)n, hipMemcpyDeviceToDevice, f.s));
    } else {
      rc = gdd_inertia(n, w.sq, nullptr, inertia_out, f.stream);
      if (rc) return rc;
    }
  }
  if (ewa_out) {  // after the labels pass is enqueued, so the device never idles on this read
    GDD_HIP(hipMemcpyAsync(&f.h.w->ewa, &w.state->ewa, sizeof(double), hipMemcpyDeviceToHost, f.s));
    GDD_HIP(hipStreamSynchronize(f.s));
    *ewa_out = f.h.w->ewa;
  }
  return GDD_OK;
}

}  // namespace
}  // namespace gdd

using namespace gdd;

extern "C" size_t gdd_minibatch_kmeans_fit_ws_bytes(int64_t n, int dim, int k, int64_t batch_size,
                                                   int64_t init_size) {
  const int64_t bs = std::min<int64_t>(batch_size, n);
  return fit_ws(nullptr, 0, n, dim, k, bs, init_size, local_trials(k), nullptr);
}

extern "C" size_t gdd_minibatch_kmeans_fit_host_ws_bytes(int64_t n, int k, int64_t batch_size,
                                                         int64_t init_size) {
  const int64_t bs = std::min<int64_t>(batch_size, n);
  return fit_host(nullptr, 0, k, bs, init_size, local_trials(k), nullptr);
}

extern "C" const char* gdd_minibatch_fit_path(int64_t n, int dim, int k, int64_t batch_size) {
  static const char* const names[] = {"invalid", "host", "dev/chain", "dev/par"};
  return names[fit_path(n, dim, k, batch_size)];
}

extern "C" int gdd_minibatch_schedule(int64_t i0, int64_t rr_base, int norms_valid0, int64_t n_steps, int k,
                                      int64_t batch_size, float reassignment_ratio, int64_t m, int32_t* out) {
  GDD_REQUIRE(i0 >= 0 && k > 0 && batch_size > 0 && m >= 0 && (m == 0 || out), "minibatch_schedule: bad arguments");
  MbSegment g{};
  g.i0 = i0, g.rr_base = rr_base, g.n_steps = n_steps, g.bs = batch_size;
  g.k = k, g.ratio = reassignment_ratio, g.norms_valid0 = norms_valid0 ? 1 : 0;
  for (int64_t j = 0; j < m; ++j) out[j] = mb_schedule_bits(mb_schedule(g, i0 + j));
  return GDD_OK;
}

extern "C" int gdd_minibatch_reassign_host(const float* weight_sums, int k, int64_t batch_size,
                                           float reassignment_ratio, void* rng,
                                           void (*argsort_cb)(const float*, int64_t, int64_t*), int64_t* pairs,
                                           int64_t* n_pairs, float* weight_sums_out, int* any_zero) {
  GDD_REQUIRE(weight_sums && k > 0 && batch_size > 0 && rng && pairs && n_pairs && weight_sums_out && any_zero,
              "minibatch_reassign_host: bad arguments");
  LegacyRNG r(static_cast<MTState*>(rng));
  bool zero = false;
  *n_pairs = mb_reassign_decide(weight_sums, k, batch_size, reassignment_ratio, r, argsort_cb, pairs,
                                weight_sums_out, &zero);
  *any_zero = zero;
  GDD_REQUIRE(*n_pairs >= 0, "minibatch_reassign_host: argsort callback required");
  return GDD_OK;
}

// The phases: initialisation; then device segments, each ended by the last step, the convergence
// stop or a hand-off; a hand-off step finishes on the host, which steps on while some weight sum is
// zero and then resumes the device. A reassignment leaves no empty cluster unless more than b/2
// centres are due (then np.argsort decides which stay), so the reassignment steps are periodic
// (every ceil(10k/b) steps from the last one) as long as that branch does not fire — always when
// k <= b/2.
extern "C" int gdd_minibatch_kmeans_fit(
    int64_t n, int dim, const float* X, int k, int64_t batch_size, int max_iter,
    int max_no_improvement, float reassignment_ratio, int64_t init_size, int n_init,
    int compute_labels, void* rng_state, void (*argsort_cb)(const float*, int64_t, int64_t*),
    float* centers_out, int32_t* labels_out, float* inertia_out, int64_t* n_steps_out,
    double* ewa_out, void* ws, size_t ws_bytes, void* host_ws, size_t host_ws_bytes,
    gdd_stream_t stream) {
  GDD_REQUIRE(n > 0 && dim > 0 && dim <= 512 && k > 0 && k <= n, "mbk_fit: bad shape");
  GDD_REQUIRE(batch_size > 0 && max_iter >= 0 && n_init >= 1 && init_size >= k && init_size <= n,
              "mbk_fit: bad parameters");
  GDD_REQUIRE(X && rng_state && centers_out && n_steps_out && ws, "mbk_fit: null pointer");
  GDD_REQUIRE(!compute_labels || (labels_out && inertia_out), "mbk_fit: labels/inertia needed");
  const int64_t bs = std::min<int64_t>(batch_size, n);
  const int T = local_trials(k);
  GDD_REQUIRE(T <= 16, "mbk_fit: k too large for the k-means++ trial count");
  GDD_REQUIRE(bs <= kMaxBatch, "minibatch: batch %lld exceeds %lld", (long long)bs, (long long)kMaxBatch);
  MTState* mt = static_cast<MTState*>(rng_state);
  Fit f{n, dim, X, k, bs, init_size, T, n_init, ((int64_t)max_iter * n) / bs, reassignment_ratio, argsort_cb,
        mt, LegacyRNG(mt), stream, to_hip(stream), fit_path(n, dim, k, batch_size) != FIT_HOST};
  if (fit_ws(ws, ws_bytes, n, dim, k, bs, f.isz, T, &f.w) > ws_bytes)
    return fail(GDD_E_WORKSPACE, "mbk_fit: workspace too small");
  // pinned staging (caller-owned): batch indices of one chunk, k-means++ uniforms, small read-backs
  GDD_REQUIRE(host_ws && host_ws_bytes >= fit_host(host_ws, host_ws_bytes, k, bs, f.isz, T, &f.h),
              "mbk_fit: pinned host workspace too small");
  int rc = mb_step_open("mbk_fit", bs, dim, k, n, max_no_improvement, X, f.w.C[0], f.w.state, f.w.step_ws,
                        f.w.step_bytes, &f.mb);
  if (rc) return rc;
  rc = fit_init(f);
  if (rc) return rc;
  // ---- the step loop (:2168-2189) -----------------------------------------------------------------
  bool use_dev = f.dev_ok;
  while (f.i < f.n_steps && f.stop_step < 0) {
    if (use_dev) {
      int64_t handoff = -1;
      rc = fit_device_segment(f, &handoff);
      if (rc) return rc;
      if (handoff < 0) break;  // ran to the end or stopped
      rc = fit_handoff(f, handoff);
      if (rc) return rc;
      use_dev = !f.any_zero;
    } else {
      rc = fit_host_segment(f, &use_dev);
      if (rc) return rc;
    }
  }
  return fit_finish(f, compute_labels, centers_out, labels_out, inertia_out, n_steps_out, ewa_out);
}

// ---- host RNG exposure for parity tests (numpy legacy RandomState draws) ---------------------------
extern "C" int gdd_rng_randint(void* state, int64_t low, int64_t high, int64_t count, int64_t* out) {
  GDD_REQUIRE(state && out && high > low && count >= 0, "rng_randint: bad arguments");
  LegacyRNG(static_cast<MTState*>(state)).randint(low, high, count, out);
  return GDD_OK;
}

extern "C" int gdd_rng_random_sample(void* state, int64_t count, double* out) {
  GDD_REQUIRE(state && out && count >= 0, "rng_random_sample: bad arguments");
  LegacyRNG r(static_cast<MTState*>(state));
  for (int64_t i = 0; i < count; ++i) out[i] = r.next_double();
  return GDD_OK;
}

extern "C" int gdd_rng_permutation(void* state, int64_t n, int64_t* out) {
  GDD_REQUIRE(state && out && n >= 0, "rng_permutation: bad arguments");
  std::vector<int64_t> p = LegacyRNG(static_cast<MTState*>(state)).permutation(n);
  std::copy(p.begin(), p.end(), out);
  return GDD_OK;
}

extern "C" int gdd_rng_choice_unit_weights(void* state, int64_t n, int64_t* out) {
  GDD_REQUIRE(state && out && n > 0, "rng_choice: bad arguments");
  out[0] = LegacyRNG(static_cast<MTState*>(state)).choice_uniform_weights(n);
  return GDD_OK;
}
