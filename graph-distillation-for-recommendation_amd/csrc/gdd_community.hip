// gdd_community.hip — a community node order for the relabelled propagation ("Community
// order"): deterministic synchronous label propagation over the CSR structure, then the nodes sorted
// by (label, id). Integer work only, so the result is a pure function of the structure.
//
// One sweep (k_lpa_sweep): row r takes the most frequent label among {lab[r]} and lab[c] of its first
// min(deg, 256) entries c != r with deg[c] <= 256, ties to the smallest label. A stored label word
// carries "this node is a hub" (deg > 256) in its top bit (node ids are below 2^31), so the one
// 4-byte gather per entry answers both "what label" and "does it vote". Every row has one writer; the
// only atomic is the sweep's integer count of changed labels, one add per wave.
//
// A wave owns four consecutive rows at a time (a quad) and walks quads grid-stride:
//   all four rows <= 16 entries  one pass, 16 lanes per row: a vote per lane, counted by comparing
//                                against the segment's lanes (ds_bpermute);
//   a pair of rows <= 32 entries one pass, 32 lanes per row, same counting;
//   a row of 17/33 .. 64 entries the whole wave: a vote per lane, counted with readlane (the votes of
//                                all such rows and pairs of the quad are loaded before any is counted);
//   a row of 65 .. 256 entries   the votes are sorted in the wave's LDS slice (bitonic, 128 or 256
//                                slots) and every run start takes its length by binary search.
// The winner is the maximum of a packed (count, 2^31-1 - label) key. The row's own vote is not stored
// with the others: it adds one to its label's count and stands as a (1, own label) candidate.
#include <climits>

#include "gdd_common.hpp"

namespace gdd {
namespace {

constexpr int kThreads = 256;  // 4 waves
constexpr int kCap = 256;
constexpr uint32_t kHub = 0x80000000u;
constexpr uint32_t kNone = 0xFFFFFFFFu;  // "no vote": sorts behind every label
constexpr int kBlocksPerCu = 8, kCus = 256;

__device__ __forceinline__ uint64_t vote_key(int count, uint32_t label) {
  return ((uint64_t)(uint32_t)count << 32) | (uint64_t)(0x7FFFFFFFu - label);
}
__device__ __forceinline__ uint32_t key_label(uint64_t key) {
  return 0x7FFFFFFFu - (uint32_t)(key & 0xFFFFFFFFull);
}
__device__ __forceinline__ uint64_t max_u64(uint64_t a, uint64_t b) { return a > b ? a : b; }

// LDS hand-over inside one wave: its DS instructions execute in order, so only the compiler and the
// outstanding-counter wait need telling
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// labels start as the node id; a row whose rowptr pair is not inside [0, nnz] is flagged and is
// treated as empty by every sweep
__global__ void k_lpa_init(int64_t n, int64_t nnz, const int32_t* __restrict__ rowptr,
                           uint32_t* __restrict__ lab, int32_t* __restrict__ bad) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n) return;
  const int32_t b = rowptr[v], e = rowptr[v + 1];
  uint32_t w = (uint32_t)v;
  if (b < 0 || e < b || (int64_t)e > nnz)
    atomicOr(bad, 1);
  else if (e - b > kCap)
    w |= kHub;
  lab[v] = w;
}

// the vote of entry p of row r (kNone: the diagonal, a hub column, an out-of-range column)
__device__ __forceinline__ uint32_t load_vote(int32_t p, int64_t r, int64_t n,
                                              const int32_t* __restrict__ col,
                                              const uint32_t* __restrict__ lab_in,
                                              int32_t* __restrict__ bad) {
  const int32_t c = col[p];
  if ((uint32_t)c >= (uint64_t)n) {
    atomicOr(bad, 2);
    return kNone;
  }
  if (c == r) return kNone;
  const uint32_t w = lab_in[c];
  return (w & kHub) ? kNone : w;
}

// Rows of at most W entries, W lanes per row: 64 / W rows of the quad at once (slots slot0 ..). b / len /
// self are the quad's row records, held by lanes 0..3. load_short fetches this lane's vote; count_short
// gives every lane its row's winner. They are two calls so that a quad's loads are all in flight before
// the first count waits for one.
template <int W>
__device__ __forceinline__ uint32_t load_short(int lane, int slot0, int32_t b, int32_t len, int64_t r0,
                                               int64_t n, const int32_t* __restrict__ col,
                                               const uint32_t* __restrict__ lab_in,
                                               int32_t* __restrict__ bad) {
  const int slot = slot0 + lane / W, j = lane % W;
  const int32_t bb = __shfl(b, slot), ll = __shfl(len, slot);
  return j < ll ? load_vote(bb + j, r0 + slot, n, col, lab_in, bad) : kNone;
}

template <int W>
__device__ __forceinline__ uint32_t count_short(int lane, int slot0, int32_t len, uint32_t self, uint32_t v) {
  const int slot = slot0 + lane / W;
  const uint32_t sf = __shfl(self, slot) & ~kHub;
  int cnt = 0;
  if (W == 64) {
    const int lu = __builtin_amdgcn_readfirstlane(__shfl(len, slot));  // one row: wave-uniform
    for (int jj = 0; jj < lu; ++jj) cnt += (uint32_t)__builtin_amdgcn_readlane((int)v, jj) == v;
  } else {
    const int base = lane & ~(W - 1);
#pragma unroll 8  // fully unrolled it costs 128 VGPRs (4 waves/SIMD)
    for (int jj = 0; jj < W; ++jj) cnt += (uint32_t)__shfl((int)v, base + jj) == v;
  }
  uint64_t key = vote_key(1, sf);
  if (v != kNone) key = max_u64(key, vote_key(cnt + (v == sf), v));
#pragma unroll
  for (int o = W / 2; o > 0; o >>= 1) key = max_u64(key, (uint64_t)__shfl_xor((unsigned long long)key, o));
  return key_label(key);
}

// A row of 65 .. 256 entries (slot `slot` of the quad), by the whole wave through its LDS slice.
__device__ __forceinline__ uint32_t pass_sorted(int lane, int slot, int32_t b, int32_t len, uint32_t self,
                                                int64_t r0, int64_t n, const int32_t* __restrict__ col,
                                                const uint32_t* __restrict__ lab_in,
                                                int32_t* __restrict__ bad, uint32_t* sm) {
  const int32_t bb = __shfl(b, slot), ll = __shfl(len, slot);
  const uint32_t sf = __shfl(self, slot) & ~kHub;
  const int S = ll <= 128 ? 128 : 256;
  for (int i = lane; i < S; i += 64) sm[i] = i < ll ? load_vote(bb + i, r0 + slot, n, col, lab_in, bad) : kNone;
  wave_sync();
  for (int k = 2; k <= S; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = lane; t < S / 2; t += 64) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;
        const uint32_t x = sm[i], y = sm[p];
        if ((x > y) == ((i & k) == 0)) {
          sm[i] = y;
          sm[p] = x;
        }
      }
      wave_sync();
    }
  }
  uint64_t key = vote_key(1, sf);
  for (int i = lane; i < S; i += 64) {
    const uint32_t v = sm[i];
    if (v != kNone && (i == 0 || sm[i - 1] != v)) {  // a run start: its end by binary search
      int lo = i + 1, hi = S;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (sm[mid] == v)
          lo = mid + 1;
        else
          hi = mid;
      }
      key = max_u64(key, vote_key(lo - i + (v == sf), v));
    }
  }
  wave_sync();  // the slice is reused by the next long row
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) key = max_u64(key, (uint64_t)__shfl_xor((unsigned long long)key, o));
  return key_label(key);
}

// cnt: three words used in rotation — sweep s adds to cnt[s % 3], reads cnt[(s - 1) % 3] and clears
// cnt[(s + 1) % 3] for the next sweep. A sweep that follows a zero-change sweep only copies the labels
// across and leaves its own word at zero, so every later sweep does the same.
__global__ __launch_bounds__(kThreads) void k_lpa_sweep(int64_t n, int64_t nnz,
                                                        const int32_t* __restrict__ rowptr,
                                                        const int32_t* __restrict__ col,
                                                        const uint32_t* __restrict__ lab_in,
                                                        uint32_t* __restrict__ lab_out,
                                                        int32_t* __restrict__ cnt, int sweep,
                                                        int32_t* __restrict__ bad) {
  __shared__ uint32_t s_sort[kThreads / 64][kCap];
  if (blockIdx.x == 0 && threadIdx.x == 0) cnt[(sweep + 1) % 3] = 0;
  if (sweep > 0 &&
      __hip_atomic_load(cnt + (sweep - 1) % 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) {
    const int64_t step = (int64_t)gridDim.x * kThreads;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += step) lab_out[i] = lab_in[i];
    return;
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t* sm = s_sort[w];
  const int64_t nwaves = (int64_t)gridDim.x * (kThreads / 64);
  const int64_t nquads = (n + 3) >> 2;
  int changed = 0;
  for (int64_t q = (int64_t)blockIdx.x * (kThreads / 64) + w; q < nquads; q += nwaves) {
    const int64_t r0 = q << 2;
    int32_t b = 0, len = 0;
    uint32_t self = 0;
    if (lane < 4 && r0 + lane < n) {
      const int32_t rb = rowptr[r0 + lane], re = rowptr[r0 + lane + 1];
      if (!(rb < 0 || re < rb || (int64_t)re > nnz)) {  // else flagged by k_lpa_init: an empty row
        b = rb;
        len = re - rb < kCap ? re - rb : kCap;
      }
      self = lab_in[r0 + lane];
    }
    const int32_t l0 = __shfl(len, 0), l1 = __shfl(len, 1), l2 = __shfl(len, 2), l3 = __shfl(len, 3);
    const int32_t m01 = l0 > l1 ? l0 : l1, m23 = l2 > l3 ? l2 : l3;
    // lane s < 4 ends up with row s's winner and writes it
    uint32_t win = 0;
    if ((m01 > m23 ? m01 : m23) <= 16) {
      const uint32_t v = load_short<16>(lane, 0, b, len, r0, n, col, lab_in, bad);
      const uint32_t x = count_short<16>(lane, 0, len, self, v);
      win = (uint32_t)__shfl((int)x, (lane & 3) << 4);
    } else {
      const int32_t ls[4] = {l0, l1, l2, l3};
      const bool pair[2] = {m01 <= 32, m23 <= 32};
      uint32_t v[4];  // v[p]: the pair's votes (32 lanes per row); else v[s]: row s's, if it has <= 64
#pragma unroll
      for (int p = 0; p < 4; p += 2) {
        if (pair[p >> 1]) {
          v[p] = load_short<32>(lane, p, b, len, r0, n, col, lab_in, bad);
        } else {
#pragma unroll
          for (int s = p; s < p + 2; ++s)
            if (ls[s] <= 64) v[s] = load_short<64>(lane, s, b, len, r0, n, col, lab_in, bad);
        }
      }
#pragma unroll
      for (int p = 0; p < 4; p += 2) {
        if (pair[p >> 1]) {
          const uint32_t x = count_short<32>(lane, p, len, self, v[p]);
          const uint32_t y = (uint32_t)__shfl((int)x, (lane & 1) << 5);
          if ((lane & ~1) == p) win = y;
        } else {
#pragma unroll
          for (int s = p; s < p + 2; ++s) {
            const uint32_t x = ls[s] <= 64 ? count_short<64>(lane, s, len, self, v[s])
                                           : pass_sorted(lane, s, b, len, self, r0, n, col, lab_in, bad, sm);
            if (lane == s) win = x;
          }
        }
      }
    }
    if (lane < 4 && r0 + lane < n) {  // self: the row's stored word (hub bit + old label)
      lab_out[r0 + lane] = win | (self & kHub);
      changed += win != (self & ~kHub);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) changed += __shfl_xor(changed, o);
  if (lane == 0 && changed) atomicAdd(cnt + sweep % 3, changed);
}

// the sort's input: key = final label (hub bit dropped), value = node id
__global__ void k_lpa_keys(int64_t n, const uint32_t* __restrict__ lab, int32_t* __restrict__ keys,
                           int32_t* __restrict__ iota, int32_t* __restrict__ labels) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n) return;
  const int32_t l = (int32_t)(lab[v] & ~kHub);
  keys[v] = l;
  iota[v] = (int32_t)v;
  if (labels) labels[v] = l;
}

__global__ void k_rho_scatter(int64_t n, const int32_t* __restrict__ order, int32_t* __restrict__ rho) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const int32_t v = order[j];
  if ((uint32_t)v < (uint64_t)n) rho[v] = (int32_t)j;
}

unsigned grid1(int64_t n, int t = kThreads) { return (unsigned)((n + t - 1) / t); }

int bits_for(int64_t n) {
  int b = 1;
  while (b < 31 && (int64_t(1) << b) < n) ++b;
  return b;
}

}  // namespace
}  // namespace gdd

using namespace gdd;

extern "C" size_t gdd_community_order_ws_bytes(int64_t n, int64_t nnz) {
  (void)nnz;
  if (n < 0) n = 0;
  return align256(sizeof(int32_t) * (size_t)n) * 6 + align256(sizeof(int32_t) * 4) + sort_pairs_ws_bytes(n) +
         1024;
}

extern "C" int gdd_community_order(int64_t n, int64_t nnz, const int32_t* rowptr, const int32_t* col,
                                   int sweeps, int32_t* rho, int32_t* labels, int32_t* changed, void* ws,
                                   size_t ws_bytes, gdd_stream_t stream) {
  GDD_REQUIRE(n >= 0 && n < INT_MAX && nnz >= 0 && nnz < INT_MAX, "community_order: bad shape");
  GDD_REQUIRE(sweeps >= 0, "community_order: sweeps must be >= 0");
  GDD_REQUIRE(n == 0 || (rowptr && rho && ws), "community_order: null pointer");
  GDD_REQUIRE(nnz == 0 || col, "community_order: null pointer");
  hipStream_t s = to_hip(stream);
  Carver cv(ws, ws_bytes);
  uint32_t* lab_a = cv.take<uint32_t>(n);
  uint32_t* lab_b = cv.take<uint32_t>(n);
  int32_t* keys = cv.take<int32_t>(n);
  int32_t* keys_out = cv.take<int32_t>(n);
  int32_t* iota = cv.take<int32_t>(n);
  int32_t* order = cv.take<int32_t>(n);
  int32_t* words = cv.take<int32_t>(4);  // cnt[3], bad
  const size_t sb = sort_pairs_ws_bytes(n);
  char* sort_ws = cv.take<char>(sb);
  if (!cv.ok()) return fail(GDD_E_WORKSPACE, "community_order: workspace too small");
  if (n == 0) return GDD_OK;
  if (changed && sweeps > 0) GDD_HIP(hipMemsetAsync(changed, 0, sizeof(int32_t) * (size_t)sweeps, s));
  GDD_HIP(hipMemsetAsync(words, 0, sizeof(int32_t) * 4, s));
  int32_t* bad = words + 3;
  k_lpa_init<<<grid1(n), kThreads, 0, s>>>(n, nnz, rowptr, lab_a, bad);
  GDD_LAUNCHED();
  const int64_t quad_blocks = ((n + 3) / 4 + kThreads / 64 - 1) / (kThreads / 64);
  const unsigned blocks = (unsigned)(quad_blocks < kBlocksPerCu * kCus ? quad_blocks : kBlocksPerCu * kCus);
  uint32_t *in = lab_a, *out = lab_b;
  for (int t = 0; t < sweeps; ++t) {
    k_lpa_sweep<<<blocks, kThreads, 0, s>>>(n, nnz, rowptr, col, in, out, words, t, bad);
    GDD_LAUNCHED();
    if (changed)
      GDD_HIP(hipMemcpyAsync(changed + t, words + t % 3, sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    uint32_t* tmp = in;
    in = out;
    out = tmp;
  }
  k_lpa_keys<<<grid1(n), kThreads, 0, s>>>(n, in, keys, iota, labels);
  GDD_LAUNCHED();
  int rc = sort_pairs_i32(keys, keys_out, iota, order, n, bits_for(n), sort_ws, sb, s);
  if (rc) return rc;
  k_rho_scatter<<<grid1(n), kThreads, 0, s>>>(n, order, rho);
  GDD_LAUNCHED();
  int32_t h_bad = 0;
  GDD_HIP(hipMemcpyAsync(&h_bad, bad, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  GDD_HIP(hipStreamSynchronize(s));
  if (h_bad)
    return fail(GDD_E_INVALID, "community_order: %s out of range (no vote cast; the order is not meaningful)",
                (h_bad & 1) ? "a rowptr pair" : "a column index");
  return GDD_OK;
}
