// gdd_topk.hip — ranked top-K recommendation lists, full-ranking positions and the ranking metrics
// (Rankformer/code/model.py:252-343 evaluate: score GEMM, training mask, torch.topk; :27-53 test:
// precision, recall, NDCG).
//
// The item-tile stream (TileStream below) is what gdd_score_topk and gdd_score_positions share: no
// score is ever written to memory. A workgroup of four waves owns 16 users, four per wave. The item
// table streams through LDS in tiles of 64 rows (staged once for the 16 users), lane l of every wave
// scores item l of the tile against the wave's four users, whose rows are read through wave-uniform
// pointers (scalar loads: the user values are SGPR operands of the fmas and cost no LDS bandwidth,
// which the per-lane item reads need); with d % 4 == 0 the next tile is fetched into registers while
// the current one is scored. The score of (user, item) is one fmaf chain over f = 0 .. d-1 from +0:
// float4 LDS reads of the item row feed the chain in ascending f, the d % 4 tail is read one by one.
// A user's mask row (ascending columns) is followed by a cursor: the lanes of the wave flag the
// columns that fall into the tile, and a flagged item scores mask_value. The two kernels differ in
// what they do with the key of (user, item) only:
//   * k_score_topk keeps a running top-K per user: thr, the K-th largest key seen at the last
//     selection (0 before the first), and an append buffer of `cap` keys in LDS (cap = the power of
//     two >= K + 64, at least 128). A key above thr is appended (ballot + prefix count: the wave
//     owns its users, no atomics); when a further tile might not fit (cnt + 64 > cap) the wave sorts
//     the buffer (bitonic, descending), keeps the first K and raises thr to the K-th. Keys are
//     unique (score_key holds the item id), so the final sorted K do not depend on arrival order.
//   * k_score_positions counts, for given target items, the items whose key is above the target's:
//     see "Full-ranking positions" below.
//
// gdd_cluster_expand_topk / gdd_cluster_positions: the same lists and positions for a condensed
// model (every user of a cluster shares a row, every item of a cluster a score) from its cluster
// tables, one wave per user (k_cluster_expand_topk; k_cluster_scores, k_cluster_rank_rows,
// k_cluster_positions).
//
// gdd_rank_metrics: one wave per user finds the hit flag of every rank by binary search in the
// user's sorted test row, one lane per cut-off sums DCG and IDCG in rank order in fp64; a second,
// one-workgroup launch adds the users in a fixed order.
//
// Written once for all of them: the bitonic sort (bitonic_sort_desc: a wave or a workgroup, with
// or without a payload), the search in an ascending row (lower_bound), the range check of a row of
// ids (row_out_of_range) and, on the host, the argument ranges (check_ranges) and the choice of a
// stream kernel's form (stream_kernel).
#include <climits>

#include "gdd_common.hpp"

namespace gdd {
namespace {

constexpr int kTkThreads = 256;
constexpr int kTkUW = 4;                              // users per wave
constexpr int kTkUsers = kTkUW * (kTkThreads / 64);   // users per workgroup
constexpr int kTkItems = 64;                          // items per tile: one per lane
constexpr int kTkMaxK = 256;
constexpr int kMaxDimTk = 256;                        // gdd_rank_max_dim()
constexpr int kMetMaxNk = 8;

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

// LDS traffic between the lanes of one wave: order it without a workgroup barrier
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// bitonic sort of key[0 .. cap) (cap a power of two >= 2), descending, by the NT threads t0 = 0 ..
// NT-1 that `sync` orders (a wave: wave_sync, a workgroup: __syncthreads); also(i, p) swaps the
// payload of two keys that change places
template <int NT, class Sync, class Also>
__device__ __forceinline__ void bitonic_sort_desc(uint64_t* key, int cap, int t0, Sync sync, Also also) {
  for (int k = 2; k <= cap; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = t0; t < (cap >> 1); t += NT) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        const int p = i | j;
        const uint64_t a = key[i], b = key[p];
        const bool swap = (i & k) == 0 ? a < b : a > b;
        if (swap) {
          key[i] = b;
          key[p] = a;
          also(i, p);
        }
      }
      sync();
    }
  }
}
template <int NT, class Sync>
__device__ __forceinline__ void bitonic_sort_desc(uint64_t* key, int cap, int t0, Sync sync) {
  bitonic_sort_desc<NT>(key, cap, t0, sync, [](int, int) {});
}

// sort the cnt appended keys, keep the K largest, raise the threshold to the K-th
__device__ __forceinline__ void wave_select(uint64_t* buf, int cap, int K, int& cnt, uint64_t& thr, int lane) {
  for (int t = cnt + lane; t < cap; t += 64) buf[t] = 0;  // below every key
  wave_sync();
  bitonic_sort_desc<64>(buf, cap, lane, [] { wave_sync(); });
  if (cnt >= K) {
    cnt = K;
    thr = buf[K - 1];
  }
}

// the first place of [lo, hi) at which `before` does not hold (hi: none); it holds on a prefix
template <class Before>
__device__ __forceinline__ int32_t partition_point(int32_t lo, int32_t hi, Before before) {
  while (lo < hi) {
    const int32_t mid = (int32_t)(((int64_t)lo + hi) >> 1);
    if (before(mid)) lo = mid + 1; else hi = mid;
  }
  return lo;
}
// the first entry of the ascending row col[lo .. hi) that is not below x (hi: none)
__device__ __forceinline__ int32_t lower_bound(const int32_t* __restrict__ col, int32_t lo, int32_t hi, int32_t x) {
  return partition_point(lo, hi, [&](int32_t e) { return col[e] < x; });
}
// whether item is in the ascending row col[lo .. hi)
__device__ __forceinline__ bool row_has(const int32_t* __restrict__ col, int32_t lo, int32_t hi, int32_t item) {
  const int32_t e = lower_bound(col, lo, hi, item);
  return e < hi && col[e] == item;
}

// one wave over the ids col[lo .. hi): the ballot of the lanes that met one outside [0, n) or one
// that `ok` rejects (a mask or target row with such an id is dropped whole)
template <class Ok>
__device__ __forceinline__ uint64_t row_out_of_range(const int32_t* __restrict__ col, int32_t lo, int32_t hi,
                                                     int64_t n, int lane, Ok ok) {
  bool out = false;
  for (int32_t e = lo + lane; e < hi; e += 64) {
    const int32_t c = col[e];
    out |= c < 0 || c >= n || !ok(c);
  }
  return __ballot(out);
}
__device__ __forceinline__ uint64_t row_out_of_range(const int32_t* __restrict__ col, int32_t lo, int32_t hi,
                                                     int64_t n, int lane) {
  return row_out_of_range(col, lo, hi, n, lane, [](int32_t) { return true; });
}

// row stride of the LDS tables in floats: a multiple of 4 (float4 reads) with S/4 odd, so the eight
// lanes of a ds_read_b128 group fall on distinct banks
__host__ __device__ inline int tk_stride(int d) {
  int s = (d + 3) & ~3;
  if (((s >> 2) & 1) == 0) s += 4;
  return s;
}
inline int tk_cap(int K) {
  int c = 128;
  while (c < K + kTkItems) c <<= 1;
  return c;
}
// LDS of the tile stream: the tile, a flag per thread, the U row of each user
inline size_t stream_lds(int d) {
  return sizeof(float) * (size_t)kTkItems * tk_stride(d) + sizeof(int32_t) * (kTkThreads + kTkUsers);
}
inline size_t tk_lds(int d, int K) { return sizeof(uint64_t) * kTkUsers * (size_t)tk_cap(K) + stream_lds(d); }

typedef float f32x4 __attribute__((ext_vector_type(4)));

// the thread's share of a tile of n4 float4 starting at src, into registers
template <int NP>
__device__ __forceinline__ void tk_fetch(f32x4 (&pre)[NP > 0 ? NP : 1], const float* __restrict__ src, int n4,
                                         int tid) {
#pragma unroll
  for (int p = 0; p < NP; ++p)
    if (tid + p * kTkThreads < n4) pre[p] = reinterpret_cast<const f32x4*>(src)[tid + p * kTkThreads];
}

// The item-tile stream of a workgroup (file header). A kernel calls init once, set_mask per user
// slot, then per pass over the items start() and, for every tile i0 = 0, 64, ...: stage (two
// workgroup barriers: before the tile is overwritten and after), score, and masked for each user
// slot j it still ranks (a wave-uniform choice).
// NP > 0: d % 4 == 0, V 16-byte aligned and a tile is at most NP float4 per thread: the next tile is
// fetched into registers before the current one is scored, so its latency hides behind the scoring
// and the upkeep of the keys. NP == 0: any d and alignment, a tile is staged float by float.
template <int NP>
struct TileStream {
  int tid, lane, wave, d, S, q, d4;  // q: float4 per row
  int64_t I;
  const float* V;
  const int32_t* mask_col;
  float* s_v;             // kTkItems x S
  int32_t* s_flag;        // one per thread
  int32_t* s_row;         // U row of each user of the workgroup, -1: none
  const float* vrow;      // the lane's item row in s_v
  const float* ug[kTkUW];  // the wave's user rows
  f32x4 pre[NP > 0 ? NP : 1];
  int pre_off[NP > 0 ? NP : 1];  // LDS float offset of the thread's p-th float4 of a tile
  int32_t cur[kTkUW], end[kTkUW];  // the mask row from the first column not yet passed
  int64_t nxt[kTkUW];              // the column at cur (wave-uniform), INT64_MAX past the row's end

  // resolves the workgroup's users (one workgroup barrier); lds: stream_lds(d) bytes, returns its end
  __device__ __forceinline__ int32_t* init(float* lds, int64_t B, int64_t I_, int d_, const int32_t* __restrict__ users,
                                           const float* __restrict__ U, int64_t nu, const float* __restrict__ V_,
                                           const int32_t* __restrict__ mask_col_) {
    tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    d = d_, S = tk_stride(d), q = d >> 2, d4 = d & ~3;
    I = I_, V = V_, mask_col = mask_col_;
    s_v = lds;
    s_flag = reinterpret_cast<int32_t*>(s_v + kTkItems * S);
    s_row = s_flag + kTkThreads;
    if (tid < kTkUsers) {
      const int64_t b = (int64_t)blockIdx.x * kTkUsers + tid;
      int32_t row = -1;
      if (b < B) {
        const int64_t r = users ? (int64_t)users[b] : b;
        if (r >= 0 && r < nu) row = (int32_t)r;
      }
      s_row[tid] = row;
    }
    __syncthreads();
    vrow = s_v + lane * S;
    // the wave's user rows through wave-uniform pointers: scalar loads, no LDS traffic for them
#pragma unroll
    for (int j = 0; j < kTkUW; ++j) {
      const int32_t row = uni(s_row[uni(wave) * kTkUW + j]);
      ug[j] = U + (int64_t)(row >= 0 ? row : 0) * d;  // no valid row: row 0 stands in, the kernel drops the user
      set_mask(j, 0, 0);
    }
    if (NP > 0) {
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        const int idx = tid + p * kTkThreads, r = idx / q;
        pre_off[p] = r * S + 4 * (idx - r * q);
      }
    }
    return s_row + kTkUsers;
  }

  // user slot j's mask row is mask_col[lo .. hi), followed from lo
  __device__ __forceinline__ void set_mask(int j, int32_t lo, int32_t hi) {
    cur[j] = lo;
    end[j] = hi;
    nxt[j] = lo < hi ? (int64_t)mask_col[lo] : (int64_t)INT64_MAX;
  }

  // before a pass over the items: the first tile into registers
  __device__ __forceinline__ void start() {
    if (NP > 0) tk_fetch<NP>(pre, V, (int)(I < kTkItems ? I : kTkItems) * q, tid);
  }

  // tile i0 into LDS (and the next one into registers); returns its number of rows
  __device__ __forceinline__ int stage(int64_t i0) {
    const int rows = (int)(I - i0 < kTkItems ? I - i0 : kTkItems);
    __syncthreads();  // the previous tile has been scored
    if (NP > 0) {
#pragma unroll
      for (int p = 0; p < NP; ++p)
        if (tid + p * kTkThreads < rows * q) *reinterpret_cast<f32x4*>(s_v + pre_off[p]) = pre[p];
      if (i0 + kTkItems < I) {
        const int64_t left = I - i0 - kTkItems;
        tk_fetch<NP>(pre, V + (i0 + kTkItems) * d, (int)(left < kTkItems ? left : kTkItems) * q, tid);
      }
    } else {
      const float* src = V + i0 * d;
      for (int idx = tid; idx < rows * d; idx += kTkThreads) {
        const int r = idx / d, f = idx - r * d;
        s_v[r * S + f] = src[idx];
      }
    }
    __syncthreads();
    return rows;
  }

  // acc[j] = the chain score of the lane's item of the staged tile against the wave's user j
  __device__ __forceinline__ void score(int rows, float (&acc)[kTkUW]) const {
#pragma unroll
    for (int j = 0; j < kTkUW; ++j) acc[j] = 0.f;
    if (lane < rows) {
      for (int f = 0; f < d4; f += 4) {
        const float4 v = *reinterpret_cast<const float4*>(vrow + f);
#pragma unroll
        for (int j = 0; j < kTkUW; ++j) {
          const float* u = ug[j] + f;
          float a = acc[j];
          a = __builtin_fmaf(u[0], v.x, a);
          a = __builtin_fmaf(u[1], v.y, a);
          a = __builtin_fmaf(u[2], v.z, a);
          a = __builtin_fmaf(u[3], v.w, a);
          acc[j] = a;
        }
      }
      for (int f = d4; f < d; ++f) {
        const float v = vrow[f];
#pragma unroll
        for (int j = 0; j < kTkUW; ++j) acc[j] = __builtin_fmaf(ug[j][f], v, acc[j]);
      }
    }
  }

  // whether user slot j's mask row holds the lane's item of tile i0; moves the cursor past the tile
  __device__ __forceinline__ bool masked(int j, int64_t i0) {
    const int64_t tile_end = i0 + kTkItems;
    bool m = false;
    if (nxt[j] < tile_end) {  // wave-uniform
      s_flag[tid] = 0;
      wave_sync();
      for (;;) {
        const int32_t e = cur[j] + lane;
        const int64_t c = e < end[j] ? (int64_t)mask_col[e] : (int64_t)INT64_MAX;
        const bool in = c < tile_end;
        if (in && c >= i0) s_flag[wave * 64 + (int)(c - i0)] = 1;
        const int n = __popcll(__ballot(in));
        cur[j] += n;
        if (n < 64) break;
      }
      wave_sync();
      m = s_flag[tid] != 0;
      wave_sync();
      nxt[j] = cur[j] < end[j] ? (int64_t)mask_col[cur[j]] : (int64_t)INT64_MAX;
    }
    return m;
  }
};

// The tile stream with a running top-K per user (file header). A user without a valid row or with
// a mask column outside [0, I) is streamed like the others and its list dropped at the end.
template <int NP>
__global__ __launch_bounds__(kTkThreads) void k_score_topk(
    int64_t B, int64_t I, int d, int K, int cap, const int32_t* __restrict__ users,
    const float* __restrict__ U, int64_t nu, const float* __restrict__ V,
    const int32_t* __restrict__ mask_ptr, const int32_t* __restrict__ mask_col, float mask_value,
    int32_t* __restrict__ top_item, float* __restrict__ top_score, int32_t* __restrict__ bad) {
  extern __shared__ __align__(16) unsigned char tk_smem[];
  uint64_t* s_keys = reinterpret_cast<uint64_t*>(tk_smem);  // kTkUsers x cap
  TileStream<NP> ts;
  ts.init(reinterpret_cast<float*>(s_keys + (size_t)kTkUsers * cap), B, I, d, users, U, nu, V, mask_col);
  const int lane = ts.lane, wave = ts.wave;
  const int64_t b0 = (int64_t)blockIdx.x * kTkUsers;

  bool live[kTkUW], dead[kTkUW];
  int cnt[kTkUW];
  uint64_t thr[kTkUW];
#pragma unroll
  for (int j = 0; j < kTkUW; ++j) {
    const int ul = wave * kTkUW + j;
    const int64_t b = b0 + ul;
    live[j] = b < B;
    dead[j] = live[j] && ts.s_row[ul] < 0;
    cnt[j] = 0;
    thr[j] = 0;
    if (live[j] && mask_ptr) {
      const int32_t lo = mask_ptr[b], hi = mask_ptr[b + 1];
      if (row_out_of_range(mask_col, lo, hi, I, lane)) dead[j] = true;
      ts.set_mask(j, lo, hi);
    }
    if (dead[j] && bad && lane == 0) atomicAdd(bad, 1);
  }

  ts.start();
  for (int64_t i0 = 0; i0 < I; i0 += kTkItems) {
    const int rows = ts.stage(i0);
    float acc[kTkUW];
    ts.score(rows, acc);
    const int64_t item = i0 + lane;
#pragma unroll
    for (int j = 0; j < kTkUW; ++j) {
      if (!live[j]) continue;  // wave-uniform
      uint64_t* buf = s_keys + (size_t)(wave * kTkUW + j) * cap;
      const bool masked = ts.masked(j, i0);
      if (cnt[j] + kTkItems > cap) wave_select(buf, cap, K, cnt[j], thr[j], lane);
      const uint64_t key = score_key(masked ? mask_value : acc[j], item);
      const bool cand = lane < rows && key > thr[j];
      const uint64_t bal = __ballot(cand);
      if (cand) buf[cnt[j] + __popcll(bal & ((1ull << lane) - 1ull))] = key;
      cnt[j] += __popcll(bal);
    }
  }

#pragma unroll
  for (int j = 0; j < kTkUW; ++j) {
    if (!live[j]) continue;
    const int64_t b = b0 + wave * kTkUW + j;
    uint64_t* buf = s_keys + (size_t)(wave * kTkUW + j) * cap;
    wave_select(buf, cap, K, cnt[j], thr[j], lane);
    for (int r = lane; r < K; r += 64) {
      const uint64_t key = buf[r];
      top_item[b * K + r] = dead[j] ? -1 : score_key_item(key);
      if (top_score) top_score[b * K + r] = dead[j] ? __builtin_nanf("") : score_key_value(key);
    }
  }
}

// the high word of score_key: larger score -> larger word, +0 above -0 as in the keys
__device__ __forceinline__ uint32_t score_ord(float v) { return (uint32_t)(score_key(v, 0) >> 32); }

// the member range of item cluster c in mem_item (I entries), clamped
__device__ __forceinline__ void mem_range(const int32_t* __restrict__ mem_ptr, int64_t c, int64_t I, int32_t& lo,
                                          int32_t& hi) {
  const int64_t lo64 = mem_ptr[c], hi64 = mem_ptr[c + 1];
  lo = (int32_t)(lo64 < 0 ? 0 : lo64 > I ? I : lo64);
  hi = (int32_t)(hi64 < lo ? lo : hi64 > I ? I : hi64);
}

// the cluster kernels' user b: false if its id is outside [0, nu) or its row g of the per-cluster
// tables outside [0, G)
__device__ __forceinline__ bool cluster_user(const int32_t* __restrict__ users, int64_t nu,
                                             const int32_t* __restrict__ cl_row, int64_t G, int64_t b, int64_t& g) {
  const int64_t r = users ? (int64_t)users[b] : b;
  g = cl_row[b];
  return r >= 0 && r < nu && g >= 0 && g < G;
}

// gdd_cluster_expand_topk: one wave per user, no workgroup barrier. The user's ranked item clusters
// (row g of cl_item / cl_score, L entries) are walked in order, 64 at a time into registers (id,
// score, member range), each cluster's members 64 at a time: a member found in the user's mask row
// (binary search) is dropped, the first K others are appended with the cluster's score. The walk
// stops once K appended-or-thresholded members beat the next cluster's score in key order; the
// mask row's first K items then enter with mask_value, and one select gives the list.
constexpr int kCxThreads = 256;
constexpr int kCxUsers = kCxThreads / 64;
__global__ __launch_bounds__(kCxThreads) void k_cluster_expand_topk(
    int64_t B, int64_t I, int64_t num_ci, int L, int K, int cap, const int32_t* __restrict__ users, int64_t nu,
    const int32_t* __restrict__ cl_row, int64_t G, const int32_t* __restrict__ cl_item,
    const float* __restrict__ cl_score, const int32_t* __restrict__ mem_ptr,
    const int32_t* __restrict__ mem_item, const int32_t* __restrict__ mask_ptr,
    const int32_t* __restrict__ mask_col, float mask_value, int32_t* __restrict__ top_item,
    float* __restrict__ top_score, int32_t* __restrict__ incomplete, int32_t* __restrict__ n_incomplete,
    int32_t* __restrict__ bad) {
  extern __shared__ __align__(16) unsigned char cx_smem[];
  const int lane = threadIdx.x & 63, wave = uni(threadIdx.x >> 6);
  const int64_t b = (int64_t)blockIdx.x * kCxUsers + wave;
  if (b >= B) return;  // wave-uniform
  uint64_t* buf = reinterpret_cast<uint64_t*>(cx_smem) + (size_t)wave * cap;
  const uint64_t below = (1ull << lane) - 1ull;

  int64_t g;
  bool dead = !cluster_user(users, nu, cl_row, G, b, g);
  int32_t mp0 = 0, mp1 = 0;
  if (mask_ptr) {
    mp0 = mask_ptr[b];
    mp1 = mask_ptr[b + 1];
    if (row_out_of_range(mask_col, mp0, mp1, I, lane)) dead = true;
  }
  const int32_t* ci_row = cl_item + (dead ? 0 : g) * L;
  const float* cs_row = cl_score + (dead ? 0 : g) * L;
  // a cluster id outside the membership CSR is not dereferenced either
  if (!dead && row_out_of_range(ci_row, 0, L, num_ci, lane)) dead = true;
  if (dead) {
    for (int t = lane; t < K; t += 64) {
      top_item[b * K + t] = -1;
      if (top_score) top_score[b * K + t] = __builtin_nanf("");
    }
    if (lane == 0) {
      incomplete[b] = 0;
      if (bad) atomicAdd(bad, 1);
    }
    return;
  }

  int cnt = 0;
  uint64_t thr = 0;
  int tot = 0;  // unmasked members examined so far, at most K per cluster
  int gt = 0;   // those of clusters scoring strictly above the current one
  uint32_t prev = 0;
  bool complete = false;
  for (int j0 = 0; j0 < L && !complete; j0 += 64) {
    const int t = j0 + lane;
    float s_l = 0.f;
    uint32_t so_l = 0, nx_l = 0;
    int32_t mb_l = 0, me_l = 0;
    if (t < L) {
      s_l = cs_row[t];
      so_l = score_ord(s_l);
      nx_l = t + 1 < L ? score_ord(cs_row[t + 1]) : so_l;  // past the list: an unseen cluster may tie the last
      mem_range(mem_ptr, ci_row[t], I, mb_l, me_l);
    }
    const int nb = L - j0 < 64 ? L - j0 : 64;
    for (int jj = 0; jj < nb; ++jj) {
      const float s = __int_as_float(uni(__float_as_int(__shfl(s_l, jj))));
      const uint32_t so = (uint32_t)uni((int)__shfl(so_l, jj)), nx = (uint32_t)uni((int)__shfl(nx_l, jj));
      const int32_t mb = uni(__shfl(mb_l, jj)), me = uni(__shfl(me_l, jj));
      if (j0 + jj > 0 && so != prev) gt = tot;
      prev = so;
      int taken = 0;
      for (int32_t e0 = mb; e0 < me && taken < K; e0 += 64) {
        const int32_t e = e0 + lane;
        bool ok = e < me;
        int32_t item = 0;
        if (ok) {
          item = mem_item[e];
          ok = !row_has(mask_col, mp0, mp1, item);
        }
        const uint64_t bal = __ballot(ok);
        const int room = K - taken;
        const bool take = ok && __popcll(bal & below) < room;  // the cluster's K lowest unmasked ids
        const int n = __popcll(bal);
        if (cnt + 64 > cap) wave_select(buf, cap, K, cnt, thr, lane);
        const uint64_t key = score_key(s, item);
        const bool cand = take && key > thr;
        const uint64_t cb = __ballot(cand);
        if (cand) buf[cnt + __popcll(cb & below)] = key;
        cnt += __popcll(cb);
        taken += n < room ? n : room;
      }
      tot += taken;
      if ((so > nx ? tot : gt) >= K) {
        complete = true;
        break;
      }
    }
  }
  if (L == num_ci) complete = true;  // every cluster was seen

  const int nm = mp1 - mp0 < K ? mp1 - mp0 : K;  // the masked items: one score, so the K lowest ids
  for (int m0 = 0; m0 < nm; m0 += 64) {
    if (cnt + 64 > cap) wave_select(buf, cap, K, cnt, thr, lane);
    const int t = m0 + lane;
    const uint64_t key = t < nm ? score_key(mask_value, mask_col[mp0 + t]) : 0;
    const bool cand = t < nm && key > thr;
    const uint64_t cb = __ballot(cand);
    if (cand) buf[cnt + __popcll(cb & below)] = key;
    cnt += __popcll(cb);
  }
  wave_select(buf, cap, K, cnt, thr, lane);
  for (int t = lane; t < K; t += 64) {
    const uint64_t key = buf[t];
    top_item[b * K + t] = score_key_item(key);
    if (top_score) top_score[b * K + t] = score_key_value(key);
  }
  if (lane == 0) {
    incomplete[b] = complete ? 0 : 1;
    if (!complete) atomicAdd(n_incomplete, 1);
  }
}

// ---------------------------------------------------------------------------------------------
// Full-ranking positions: pos(b, t) = #{ i : key(b, i) > key(b, t) } for the targets of a CSR.
//
// k_score_positions runs the tile stream once per chunk of kRpChunk targets of its users; per chunk
//   * pre-pass: one lane per target computes the target's own key with the same chain (its row of V
//     gathered from memory), the masked flag by binary search in the mask row; the wave sorts the
//     keys descending (bitonic) with the target's place in the chunk as payload;
//   * streaming pass over all items: each lane counts by binary search the targets whose key is not
//     below its item's key, p, and adds one to integer bucket p in LDS (the item ranks above the
//     sorted targets p, p + 1, ...); an item at or below every target adds nothing;
//   * the inclusive prefix sum of the buckets is the position of each sorted target.
// The wave owns its users: LDS integer atomics between its own lanes, no float atomics, no
// workspace. A workgroup passes over V once per chunk of its longest row.
// ---------------------------------------------------------------------------------------------
constexpr int kRpChunk = 256;  // targets of one user per pass over the items; the payload is a byte

inline size_t rp_lds(int d) {
  return (sizeof(uint64_t) + sizeof(int32_t) + sizeof(uint8_t)) * (size_t)kTkUsers * kRpChunk + stream_lds(d) +
         sizeof(int32_t) * kTkUsers;
}

template <int NP>
__global__ __launch_bounds__(kTkThreads) void k_score_positions(
    int64_t B, int64_t I, int d, const int32_t* __restrict__ users, const float* __restrict__ U, int64_t nu,
    const float* __restrict__ V, const int32_t* __restrict__ mask_ptr, const int32_t* __restrict__ mask_col,
    float mask_value, const int32_t* __restrict__ tg_ptr, const int32_t* __restrict__ tg_col,
    int32_t* __restrict__ pos, int32_t* __restrict__ bad) {
  extern __shared__ __align__(16) unsigned char rp_smem[];
  uint64_t* s_keys = reinterpret_cast<uint64_t*>(rp_smem);  // kTkUsers x kRpChunk
  TileStream<NP> ts;
  int32_t* s_cnt = ts.init(reinterpret_cast<float*>(s_keys + (size_t)kTkUsers * kRpChunk), B, I, d, users, U, nu, V,
                           mask_col);                         // kTkUsers x kRpChunk
  int32_t* s_len = s_cnt + kTkUsers * kRpChunk;               // targets of each user to rank
  uint8_t* s_idx = reinterpret_cast<uint8_t*>(s_len + kTkUsers);  // kTkUsers x kRpChunk
  const int lane = ts.lane, wave = ts.wave;
  const int64_t b0 = (int64_t)blockIdx.x * kTkUsers;

  // the wave's users: mask and target rows, checked once (a column outside [0, I) kills the row)
  bool live[kTkUW];
  int32_t mb[kTkUW], me[kTkUW], tb[kTkUW], tn[kTkUW];
#pragma unroll
  for (int j = 0; j < kTkUW; ++j) {
    const int ul = wave * kTkUW + j;
    const int64_t b = b0 + ul;
    live[j] = b < B;
    bool dead = live[j] && ts.s_row[ul] < 0;
    mb[j] = me[j] = tb[j] = tn[j] = 0;
    if (live[j]) {
      uint64_t out = 0;
      if (mask_ptr) {
        mb[j] = mask_ptr[b];
        me[j] = mask_ptr[b + 1];
        out = row_out_of_range(mask_col, mb[j], me[j], I, lane);
      }
      tb[j] = tg_ptr[b];
      const int32_t te = tg_ptr[b + 1];
      tn[j] = te > tb[j] ? te - tb[j] : 0;
      out |= row_out_of_range(tg_col, tb[j], tb[j] + tn[j], I, lane);
      if (out) dead = true;
      if (dead) {
        for (int32_t e = lane; e < tn[j]; e += 64) pos[tb[j] + e] = -1;
        if (bad && lane == 0) atomicAdd(bad, 1);
        live[j] = false;
      }
    }
    if (lane == 0) s_len[ul] = live[j] ? tn[j] : 0;
  }
  __syncthreads();
  int maxlen = 0;
#pragma unroll
  for (int u = 0; u < kTkUsers; ++u) maxlen = s_len[u] > maxlen ? s_len[u] : maxlen;

  for (int c0 = 0; c0 < maxlen; c0 += kRpChunk) {  // uniform over the workgroup
    int n[kTkUW], capn[kTkUW];
#pragma unroll
    for (int j = 0; j < kTkUW; ++j) {
      const int ul = wave * kTkUW + j;
      n[j] = 0;
      capn[j] = 2;
      if (live[j] && tn[j] > c0) n[j] = tn[j] - c0 < kRpChunk ? tn[j] - c0 : kRpChunk;
      if (n[j] == 0) continue;  // wave-uniform
      while (capn[j] < n[j]) capn[j] <<= 1;
      uint64_t* keys = s_keys + ul * kRpChunk;
      uint8_t* idx = s_idx + ul * kRpChunk;
      for (int i = lane; i < capn[j]; i += 64) {
        uint64_t key = 0;  // below every key
        if (i < n[j]) {
          const int32_t t = tg_col[tb[j] + c0 + i];
          const float* v = V + (int64_t)t * d;
          float a = 0.f;
          for (int f = 0; f < d; ++f) a = __builtin_fmaf(ts.ug[j][f], v[f], a);
          key = score_key(row_has(mask_col, mb[j], me[j], t) ? mask_value : a, t);
        }
        keys[i] = key;
        idx[i] = (uint8_t)i;
        s_cnt[ul * kRpChunk + i] = 0;
      }
      wave_sync();
      bitonic_sort_desc<64>(keys, capn[j], lane, [] { wave_sync(); }, [&](int i, int p) {
        const uint8_t x = idx[i];
        idx[i] = idx[p];
        idx[p] = x;
      });
      ts.set_mask(j, mb[j], me[j]);
    }

    ts.start();
    for (int64_t i0 = 0; i0 < I; i0 += kTkItems) {
      const int rows = ts.stage(i0);
      float acc[kTkUW];
      ts.score(rows, acc);
      const int64_t item = i0 + lane;
#pragma unroll
      for (int j = 0; j < kTkUW; ++j) {
        if (n[j] == 0) continue;  // wave-uniform
        const int ul = wave * kTkUW + j;
        const bool masked = ts.masked(j, i0);
        if (lane < rows) {
          const uint64_t key = score_key(masked ? mask_value : acc[j], item);
          const uint64_t* keys = s_keys + ul * kRpChunk;
          int p = 0;  // the sorted targets at or above this item's key
          for (int s = capn[j] >> 1; s > 0; s >>= 1)
            if (keys[p + s - 1] >= key) p += s;
          if (keys[p] >= key) ++p;
          if (p < n[j]) atomicAdd(&s_cnt[ul * kRpChunk + p], 1);
        }
      }
    }

#pragma unroll
    for (int j = 0; j < kTkUW; ++j) {
      if (n[j] == 0) continue;
      const int ul = wave * kTkUW + j;
      wave_sync();
      int carry = 0;
      for (int seg = 0; seg < n[j]; seg += 64) {
        const int i = seg + lane;
        int v = i < n[j] ? s_cnt[ul * kRpChunk + i] : 0;
        for (int o = 1; o < 64; o <<= 1) {
          const int up = __shfl_up(v, o);
          if (lane >= o) v += up;
        }
        v += carry;
        if (i < n[j]) pos[tb[j] + c0 + (int)s_idx[ul * kRpChunk + i]] = v;
        carry = __shfl(v, 63);
      }
      wave_sync();  // the next chunk's pre-pass overwrites the buckets
    }
  }
}

// S[g, c] = the chain score of user cluster groups[g] against item cluster c (G x num_ci): lane =
// item cluster, four user clusters per wave through scalar loads. A group outside [0, num_cu) is
// not read (its row is zeros; k_cluster_positions drops the users of such a row).
constexpr int kCsGroups = 16;
__global__ __launch_bounds__(256) void k_cluster_scores(int64_t G, int64_t num_cu, int64_t num_ci, int d,
                                                        int64_t n_ctiles, const int32_t* __restrict__ groups,
                                                        const float* __restrict__ cu_z,
                                                        const float* __restrict__ ci_z, float* __restrict__ S) {
  const int lane = threadIdx.x & 63, wave = uni(threadIdx.x >> 6);
  const int64_t gt = blockIdx.x / n_ctiles, ct = blockIdx.x - gt * n_ctiles;
  const int64_t c = ct * 64 + lane;
  const int64_t g0 = gt * kCsGroups + wave * 4;
  const float* ug[4];
  bool ok[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int64_t r = g0 + j < G ? (int64_t)groups[g0 + j] : -1;
    ok[j] = r >= 0 && r < num_cu;
    ug[j] = cu_z + (ok[j] ? r : 0) * d;
  }
  if (c >= num_ci) return;
  const float* v = ci_z + c * d;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int f = 0; f < d; ++f) {
    const float x = v[f];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = __builtin_fmaf(ug[j][f], x, acc[j]);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (g0 + j < G) S[(g0 + j) * num_ci + c] = ok[j] ? acc[j] : 0.f;
}

// the members mem_item[lo .. hi) (ascending) with an id below t
__device__ __forceinline__ int members_below(const int32_t* __restrict__ mem_item, int32_t lo, int32_t hi,
                                             int32_t t) {
  return lower_bound(mem_item, lo, hi, t) - lo;
}
// a masked item mi whose cluster scores om: counted where mask_value puts it, not where its cluster did
__device__ __forceinline__ int mask_shift(uint32_t omv, uint32_t om, uint32_t ot, int32_t mi, int32_t t) {
  const bool as_masked = omv > ot || (omv == ot && mi < t);
  const bool as_member = om > ot || (om == ot && mi < t);
  return (int)as_masked - (int)as_member;
}

// Row g of the score table in ranked order, once per user cluster: sc[g, k] is the item cluster at
// place k (descending score word, ties by ascending cluster id), pre[g, k] the members of the
// clusters before place k (num_ci + 1 entries). One workgroup per row, a bitonic sort of at most
// kCpSortMax keys in LDS, then a block scan of the sizes.
constexpr int kCpSortMax = 4096;  // 32 KiB of keys
constexpr int kCpThreads = 256;
__global__ __launch_bounds__(kCpThreads) void k_cluster_rank_rows(int64_t I, int num_ci, int cap,
                                                                  const float* __restrict__ S,
                                                                  const int32_t* __restrict__ mem_ptr,
                                                                  int32_t* __restrict__ sc, int32_t* __restrict__ pre) {
  extern __shared__ __align__(16) unsigned char cp_smem[];
  __shared__ int32_t s_part[kCpThreads];
  uint64_t* keys = reinterpret_cast<uint64_t*>(cp_smem);  // cap
  const int tid = threadIdx.x;
  const int64_t g = blockIdx.x;
  const float* srow = S + g * num_ci;
  for (int c = tid; c < cap; c += kCpThreads) keys[c] = c < num_ci ? score_key(srow[c], c) : 0;  // 0: below every key
  __syncthreads();
  bitonic_sort_desc<kCpThreads>(keys, cap, tid, [] { __syncthreads(); });
  const int per = (num_ci + kCpThreads - 1) / kCpThreads;  // consecutive places per thread
  const int k0 = tid * per < num_ci ? tid * per : num_ci;
  const int k1 = k0 + per < num_ci ? k0 + per : num_ci;
  int sum = 0;
  for (int k = k0; k < k1; ++k) {
    int32_t lo, hi;
    mem_range(mem_ptr, score_key_item(keys[k]), I, lo, hi);
    sum += hi - lo;
  }
  s_part[tid] = sum;
  __syncthreads();
  int base = 0;
  for (int i = 0; i < tid; ++i) base += s_part[i];
  for (int k = k0; k < k1; ++k) {
    const int32_t c = score_key_item(keys[k]);
    int32_t lo, hi;
    mem_range(mem_ptr, c, I, lo, hi);
    sc[g * num_ci + k] = c;
    pre[g * (num_ci + 1) + k] = base;
    base += hi - lo;
    if (k == num_ci - 1) pre[g * (num_ci + 1) + num_ci] = base;
  }
}

// gdd_cluster_positions: one wave per user. With o_t the score word of the target (mask_value's if
// it is masked, else its cluster's): a cluster above o_t adds its size, a cluster at o_t its members
// below t (binary search in mem_item), and each item of the mask row is counted where mask_value puts
// it instead of where its cluster did.
//   RANKED (num_ci <= kCpSortMax, rows ranked by k_cluster_rank_rows): one lane per target. The
//   clusters above o_t are a prefix of the ranked row, found by binary search, and their sizes one
//   entry of pre; only the tied clusters that follow and the mask row are walked.
//   Otherwise: one target after the other, the lanes over all clusters and then over the mask row,
//   with an integer wave sum.
template <bool RANKED>
__global__ __launch_bounds__(kCxThreads) void k_cluster_positions(
    int64_t B, int64_t I, int64_t num_cu, int64_t num_ci, const int32_t* __restrict__ users, int64_t nu,
    const int32_t* __restrict__ cl_row, int64_t G, const int32_t* __restrict__ groups,
    const float* __restrict__ S, const int32_t* __restrict__ sc, const int32_t* __restrict__ pre,
    const int32_t* __restrict__ i2ci, const int32_t* __restrict__ mem_ptr,
    const int32_t* __restrict__ mem_item, const int32_t* __restrict__ mask_ptr,
    const int32_t* __restrict__ mask_col, float mask_value, const int32_t* __restrict__ tg_ptr,
    const int32_t* __restrict__ tg_col, int32_t* __restrict__ pos, int32_t* __restrict__ bad) {
  const int lane = threadIdx.x & 63, wave = uni(threadIdx.x >> 6);
  const int64_t b = (int64_t)blockIdx.x * kCxUsers + wave;
  if (b >= B) return;  // wave-uniform

  int64_t g;
  bool dead = !cluster_user(users, nu, cl_row, G, b, g);
  if (!dead) {
    const int64_t gr = groups[g];
    dead = gr < 0 || gr >= num_cu;
  }
  // an item id outside [0, I) or an item's cluster outside [0, num_ci) kills the row
  const auto in_cluster = [&](int32_t c) {
    const int32_t k = i2ci[c];
    return k >= 0 && k < num_ci;
  };
  int32_t mp0 = 0, mp1 = 0;
  uint64_t out = 0;
  if (mask_ptr) {
    mp0 = mask_ptr[b];
    mp1 = mask_ptr[b + 1];
    out = row_out_of_range(mask_col, mp0, mp1, I, lane, in_cluster);
  }
  const int32_t tb = tg_ptr[b];
  const int32_t te = tg_ptr[b + 1] > tb ? tg_ptr[b + 1] : tb;
  out |= row_out_of_range(tg_col, tb, te, I, lane, in_cluster);
  if (out) dead = true;
  if (dead) {
    for (int32_t e = tb + lane; e < te; e += 64) pos[e] = -1;
    if (bad && lane == 0) atomicAdd(bad, 1);
    return;
  }

  const float* srow = S + g * num_ci;
  const uint32_t omv = score_ord(mask_value);
  if (RANKED) {
    const int32_t* scr = sc + g * num_ci;
    const int32_t* prer = pre + g * (num_ci + 1);
    for (int32_t e = tb + lane; e < te; e += 64) {
      const int32_t t = tg_col[e];
      const uint32_t ot = row_has(mask_col, mp0, mp1, t) ? omv : score_ord(srow[i2ci[t]]);
      // the ranked clusters above o_t: places [0, a)
      const int32_t a = partition_point(0, (int32_t)num_ci, [&](int32_t k) { return score_ord(srow[scr[k]]) > ot; });
      int acc = prer[a];
      for (int32_t k = a; k < num_ci; ++k) {  // the tied clusters
        const int32_t c = scr[k];
        if (score_ord(srow[c]) != ot) break;
        int32_t lo, hi;
        mem_range(mem_ptr, c, I, lo, hi);
        acc += members_below(mem_item, lo, hi, t);
      }
      for (int32_t m = mp0; m < mp1; ++m) {
        const int32_t mi = mask_col[m];
        acc += mask_shift(omv, score_ord(srow[i2ci[mi]]), ot, mi, t);
      }
      pos[e] = acc;
    }
    return;
  }
  for (int32_t e = tb; e < te; ++e) {  // wave-uniform
    const int32_t t = uni(tg_col[e]);
    const uint32_t ot = row_has(mask_col, mp0, mp1, t) ? omv : score_ord(srow[i2ci[t]]);
    int acc = 0;
    for (int64_t c = lane; c < num_ci; c += 64) {
      const uint32_t oc = score_ord(srow[c]);
      if (oc < ot) continue;
      int32_t lo, hi;
      mem_range(mem_ptr, c, I, lo, hi);
      acc += oc > ot ? hi - lo : members_below(mem_item, lo, hi, t);
    }
    for (int32_t m = mp0 + lane; m < mp1; m += 64) {
      const int32_t mi = mask_col[m];
      acc += mask_shift(omv, score_ord(srow[i2ci[mi]]), ot, mi, t);
    }
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (lane == 0) pos[e] = acc;
  }
}

// per_user[b] = (precision, recall, ndcg) x nk of user b's list; one wave per user
constexpr int kMetThreads = 256;
__global__ __launch_bounds__(kMetThreads) void k_rank_metrics(
    int64_t B, int K, const int32_t* __restrict__ top_item, const int32_t* __restrict__ te_ptr,
    const int32_t* __restrict__ te_col, const int32_t* __restrict__ te_deg, int nk,
    const int32_t* __restrict__ topks, const double* __restrict__ inv_log2, double* __restrict__ per_user) {
  __shared__ uint64_t s_hit[kMetThreads / 64][kTkMaxK / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t b = (int64_t)blockIdx.x * (kMetThreads / 64) + wave;
  if (b >= B) return;
  const int32_t beg = te_ptr[b], fin = te_ptr[b + 1];
  const int64_t n = te_deg ? (int64_t)te_deg[b] : (int64_t)(fin - beg);
  for (int g = 0; g < kTkMaxK / 64; ++g) {
    const int r = g * 64 + lane;
    const bool hit = r < K && n > 0 && row_has(te_col, beg, fin, top_item[b * K + r]);
    const uint64_t bal = __ballot(hit);
    if (lane == 0) s_hit[wave][g] = bal;
  }
  wave_sync();
  if (lane < nk) {
    const int k = topks[lane] < 1 ? 1 : (topks[lane] > K ? K : topks[lane]);  // never past the list
    double pre = 0.0, rec = 0.0, ndcg = 0.0;
    if (n > 0) {
      const int64_t cut = n < k ? n : (int64_t)k;
      int hits = 0;
      double dcg = 0.0, idcg = 0.0;
      for (int r = 0; r < k; ++r) {
        if ((s_hit[wave][r >> 6] >> (r & 63)) & 1ull) {
          ++hits;
          dcg += inv_log2[r];
        }
        if (r < cut) idcg += inv_log2[r];
      }
      pre = (double)hits / (double)k;
      rec = (double)hits / (double)cut;
      ndcg = dcg / idcg;
    }
    double* o = per_user + b * 3 * nk;
    o[lane] = pre;
    o[nk + lane] = rec;
    o[2 * nk + lane] = ndcg;
  }
}

// sums[c] = sum over users of per_user[b][c], c < 3 nk, in a fixed order: thread t adds users
// t, t + 256, ... in ascending order, then a pairwise tree over the 256 partial sums
__global__ __launch_bounds__(kMetThreads) void k_rank_metric_sums(
    int64_t B, int nc, const double* __restrict__ per_user, const int32_t* __restrict__ te_ptr,
    const int32_t* __restrict__ te_deg, double* __restrict__ sums, int64_t* __restrict__ count) {
  __shared__ double s_part[kMetThreads];
  __shared__ long long s_cnt[kMetThreads];
  const int tid = threadIdx.x;
  for (int c = 0; c <= nc; ++c) {  // c == nc: the count
    double a = 0.0;
    long long m = 0;
    for (int64_t b = tid; b < B; b += kMetThreads) {
      if (c < nc) {
        a += per_user[b * nc + c];
      } else {
        const int64_t n = te_deg ? (int64_t)te_deg[b] : (int64_t)(te_ptr[b + 1] - te_ptr[b]);
        m += n > 0 ? 1 : 0;
      }
    }
    s_part[tid] = a;
    s_cnt[tid] = m;
    __syncthreads();
    for (int o = kMetThreads / 2; o > 0; o >>= 1) {
      if (tid < o) {
        s_part[tid] = s_part[tid] + s_part[tid + o];
        s_cnt[tid] += s_cnt[tid + o];
      }
      __syncthreads();
    }
    if (tid == 0) {
      if (c < nc) sums[c] = s_part[0];
      else count[0] = (int64_t)s_cnt[0];
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------
// Host
// ---------------------------------------------------------------------------------------------

// the ranges every entry point `who` puts on its sizes: B, I, nu (and G, num_ci of the cluster entry
// points; the others pass 0 and 1) within int32, the width d and the list length K where it has one
int check_ranges(const char* who, int64_t B, int64_t I, int64_t nu, const int* d, const int* K, int64_t G = 0,
                 int64_t num_ci = 1) {
  GDD_REQUIRE(B >= 0 && B < INT32_MAX && I >= 1 && I < INT32_MAX && nu >= 1 && nu < INT32_MAX && G >= 0 &&
                  G < INT32_MAX && num_ci >= 1 && num_ci < INT32_MAX,
              "%s: B=%lld I=%lld nu=%lld G=%lld num_ci=%lld unsupported", who, (long long)B, (long long)I,
              (long long)nu, (long long)G, (long long)num_ci);
  GDD_REQUIRE(!d || (*d >= 1 && *d <= kMaxDimTk), "%s: d=%d outside [1, %d]", who, d ? *d : 0, kMaxDimTk);
  GDD_REQUIRE(!K || (*K >= 1 && *K <= kTkMaxK && *K <= I), "%s: K=%d outside [1, min(%d, I=%lld)]", who,
              K ? *K : 0, kTkMaxK, (long long)I);
  return GDD_OK;
}

// the form of a tile-stream kernel (forms: NP = 0, 4, 8, 16) for a width and an item table, with
// its dynamic LDS limit raised where the launch needs more than 64 KiB
template <class Kern>
int stream_kernel(Kern* const (&forms)[4], int d, const float* V, size_t lds, Kern*& kern) {
  const bool vec = (d & 3) == 0 && (reinterpret_cast<uintptr_t>(V) & 15) == 0;
  kern = forms[!vec ? 0 : d <= 64 ? 1 : d <= 128 ? 2 : 3];
  if (lds > 65536)
    GDD_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  return GDD_OK;
}

}  // namespace
}  // namespace gdd

using namespace gdd;

extern "C" int gdd_score_topk(int64_t B, int64_t I, int d, int K, const int32_t* users, const float* U,
                              int64_t nu, const float* V, const int32_t* mask_ptr, const int32_t* mask_col,
                              float mask_value, int32_t* top_item, float* top_score, int32_t* bad,
                              gdd_stream_t stream) {
  if (const int rc = check_ranges("score_topk", B, I, nu, &d, &K)) return rc;
  if (B == 0) return GDD_OK;
  GDD_REQUIRE(U && V && top_item, "score_topk: null pointer");
  GDD_REQUIRE(!mask_ptr || mask_col, "score_topk: mask_ptr without mask_col");
  static constexpr decltype(&k_score_topk<0>) forms[4] = {k_score_topk<0>, k_score_topk<4>, k_score_topk<8>,
                                                         k_score_topk<16>};
  const size_t lds = tk_lds(d, K);
  decltype(&k_score_topk<0>) kern;
  if (const int rc = stream_kernel(forms, d, V, lds, kern)) return rc;
  const unsigned grid = (unsigned)((B + kTkUsers - 1) / kTkUsers);
  kern<<<grid, kTkThreads, lds, to_hip(stream)>>>(B, I, d, K, tk_cap(K), users, U, nu, V, mask_ptr, mask_col,
                                                  mask_value, top_item, top_score, bad);
  GDD_LAUNCHED();
  return GDD_OK;
}

extern "C" int gdd_cluster_expand_topk(int64_t B, int64_t I, int64_t num_ci, int L, int K, const int32_t* users,
                                       int64_t nu, const int32_t* cl_row, int64_t G, const int32_t* cl_item,
                                       const float* cl_score, const int32_t* mem_ptr, const int32_t* mem_item,
                                       const int32_t* mask_ptr, const int32_t* mask_col, float mask_value,
                                       int32_t* top_item, float* top_score, int32_t* incomplete,
                                       int32_t* n_incomplete, int32_t* bad, gdd_stream_t stream) {
  if (const int rc = check_ranges("cluster_expand_topk", B, I, nu, nullptr, &K, G, num_ci)) return rc;
  GDD_REQUIRE(L >= 1 && L <= kTkMaxK && L <= num_ci, "cluster_expand_topk: L=%d outside [1, min(%d, num_ci=%lld)]",
              L, kTkMaxK, (long long)num_ci);
  if (B == 0) return GDD_OK;
  GDD_REQUIRE(cl_row && cl_item && cl_score && mem_ptr && mem_item && top_item && incomplete && n_incomplete,
              "cluster_expand_topk: null pointer");
  GDD_REQUIRE(!mask_ptr || mask_col, "cluster_expand_topk: mask_ptr without mask_col");
  const int cap = tk_cap(K);
  const size_t lds = sizeof(uint64_t) * kCxUsers * (size_t)cap;  // at most 16 KiB
  const unsigned grid = (unsigned)((B + kCxUsers - 1) / kCxUsers);
  k_cluster_expand_topk<<<grid, kCxThreads, lds, to_hip(stream)>>>(
      B, I, num_ci, L, K, cap, users, nu, cl_row, G, cl_item, cl_score, mem_ptr, mem_item, mask_ptr, mask_col,
      mask_value, top_item, top_score, incomplete, n_incomplete, bad);
  GDD_LAUNCHED();
  return GDD_OK;
}

extern "C" int gdd_rank_metrics(int64_t B, int K, const int32_t* top_item, const int32_t* te_ptr,
                                const int32_t* te_col, const int32_t* te_deg, int nk, const int32_t* topks,
                                const double* inv_log2, double* per_user, double* sums, int64_t* count,
                                gdd_stream_t stream) {
  GDD_REQUIRE(B >= 0 && B < INT32_MAX && K >= 1 && K <= kTkMaxK && nk >= 1 && nk <= kMetMaxNk,
              "rank_metrics: B=%lld K=%d nk=%d unsupported", (long long)B, K, nk);
  GDD_REQUIRE(topks && inv_log2 && sums && count && (B == 0 || (top_item && te_ptr && per_user)),
              "rank_metrics: null pointer");
  hipStream_t s = to_hip(stream);
  if (B > 0) {
    const unsigned grid = (unsigned)((B + kMetThreads / 64 - 1) / (kMetThreads / 64));
    k_rank_metrics<<<grid, kMetThreads, 0, s>>>(B, K, top_item, te_ptr, te_col, te_deg, nk, topks, inv_log2,
                                                per_user);
    GDD_LAUNCHED();
  }
  k_rank_metric_sums<<<1, kMetThreads, 0, s>>>(B, 3 * nk, per_user, te_ptr, te_deg, sums, count);
  GDD_LAUNCHED();
  return GDD_OK;
}

extern "C" int gdd_score_positions(int64_t B, int64_t I, int d, const int32_t* users, const float* U, int64_t nu,
                                   const float* V, const int32_t* mask_ptr, const int32_t* mask_col,
                                   float mask_value, const int32_t* tg_ptr, const int32_t* tg_col, int32_t* pos,
                                   int32_t* bad, gdd_stream_t stream) {
  if (const int rc = check_ranges("score_positions", B, I, nu, &d, nullptr)) return rc;
  if (B == 0) return GDD_OK;
  GDD_REQUIRE(U && V && tg_ptr, "score_positions: null pointer");
  GDD_REQUIRE(!mask_ptr || mask_col, "score_positions: mask_ptr without mask_col");
  static constexpr decltype(&k_score_positions<0>) forms[4] = {k_score_positions<0>, k_score_positions<4>,
                                                              k_score_positions<8>, k_score_positions<16>};
  const size_t lds = rp_lds(d);
  decltype(&k_score_positions<0>) kern;
  if (const int rc = stream_kernel(forms, d, V, lds, kern)) return rc;
  const unsigned grid = (unsigned)((B + kTkUsers - 1) / kTkUsers);
  kern<<<grid, kTkThreads, lds, to_hip(stream)>>>(B, I, d, users, U, nu, V, mask_ptr, mask_col, mask_value,
                                                  tg_ptr, tg_col, pos, bad);
  GDD_LAUNCHED();
  return GDD_OK;
}

// workspace: the score of every (user cluster, item cluster), G x num_ci floats; then, where the rows
// are ranked (num_ci <= kCpSortMax), the ranked cluster ids (G x num_ci) and the prefix sizes
// (G x (num_ci + 1))
extern "C" size_t gdd_cluster_positions_ws_bytes(int64_t G, int64_t num_ci) {
  if (G < 0 || num_ci < 0) return 0;
  const size_t table = sizeof(float) * (size_t)G * (size_t)num_ci;
  return num_ci <= kCpSortMax ? 3 * table + sizeof(int32_t) * (size_t)G : table;
}

extern "C" int gdd_cluster_positions(int64_t B, int64_t I, int64_t num_cu, int64_t num_ci, int d,
                                     const float* cu_z, const float* ci_z, const int32_t* users, int64_t nu,
                                     const int32_t* cl_row, int64_t G, const int32_t* groups,
                                     const int32_t* i2ci, const int32_t* mem_ptr, const int32_t* mem_item,
                                     const int32_t* mask_ptr, const int32_t* mask_col, float mask_value,
                                     const int32_t* tg_ptr, const int32_t* tg_col, int32_t* pos, int32_t* bad,
                                     void* ws, size_t ws_bytes, gdd_stream_t stream) {
  GDD_REQUIRE(num_cu >= 1 && num_cu < INT32_MAX, "cluster_positions: num_cu=%lld unsupported", (long long)num_cu);
  if (const int rc = check_ranges("cluster_positions", B, I, nu, &d, nullptr, G, num_ci)) return rc;
  if (B == 0) return GDD_OK;
  GDD_REQUIRE(cu_z && ci_z && cl_row && groups && i2ci && mem_ptr && mem_item && tg_ptr && G >= 1,
              "cluster_positions: null pointer");
  GDD_REQUIRE(!mask_ptr || mask_col, "cluster_positions: mask_ptr without mask_col");
  GDD_REQUIRE(ws && ws_bytes >= gdd_cluster_positions_ws_bytes(G, num_ci),
              "cluster_positions: workspace of %zu bytes, %zu needed", ws_bytes,
              gdd_cluster_positions_ws_bytes(G, num_ci));
  const int64_t n_ctiles = (num_ci + 63) / 64, n_gtiles = (G + kCsGroups - 1) / kCsGroups;
  GDD_REQUIRE(n_ctiles * n_gtiles < INT32_MAX, "cluster_positions: G x num_ci too large for one launch");
  float* S = static_cast<float*>(ws);
  hipStream_t s = to_hip(stream);
  k_cluster_scores<<<(unsigned)(n_ctiles * n_gtiles), 256, 0, s>>>(G, num_cu, num_ci, d, n_ctiles, groups, cu_z,
                                                                   ci_z, S);
  GDD_LAUNCHED();
  const unsigned grid = (unsigned)((B + kCxUsers - 1) / kCxUsers);
  if (num_ci <= kCpSortMax) {
    int32_t* sc = reinterpret_cast<int32_t*>(S + G * num_ci);
    int32_t* pre = sc + G * num_ci;
    int cap = 2;
    while (cap < num_ci) cap <<= 1;
    k_cluster_rank_rows<<<(unsigned)G, kCpThreads, sizeof(uint64_t) * cap, s>>>(I, (int)num_ci, cap, S, mem_ptr, sc,
                                                                                pre);
    GDD_LAUNCHED();
    k_cluster_positions<true><<<grid, kCxThreads, 0, s>>>(B, I, num_cu, num_ci, users, nu, cl_row, G, groups, S, sc,
                                                          pre, i2ci, mem_ptr, mem_item, mask_ptr, mask_col,
                                                          mask_value, tg_ptr, tg_col, pos, bad);
  } else {
    k_cluster_positions<false><<<grid, kCxThreads, 0, s>>>(B, I, num_cu, num_ci, users, nu, cl_row, G, groups, S,
                                                           nullptr, nullptr, i2ci, mem_ptr, mem_item, mask_ptr,
                                                           mask_col, mask_value, tg_ptr, tg_col, pos, bad);
  }
  GDD_LAUNCHED();
  return GDD_OK;
}
