// gdd_rankformer.hip — the two row passes behind the Rankformer teacher's layer (Rankformer/code/
// rec.py:143-274; DESIGN.md "Rankformer teacher"). The layer is linear attention over the bipartite
// interaction graph: per stored pair one dot product and one scalar weight, plus a few d x d global
// terms that stay library GEMMs. The reference evaluates it with ~14 gathered index_add scatters
// (float atomics on a GPU); here every output element has one owner and a summation order fixed by
// the CSR alone, so two runs give the same bits.
//   * gdd_rank_rowpass: per row r and stored entry e = (r, c): s_e = <Q_r, K_c>, and the row sums
//     s_sum_r = sum s_e, SK_r = sum K_c, SV_r = sum V_c, A_r = sum s_e V_c;
//   * gdd_rank_wsum: Y_r = sum w_e V_c, and optionally ta_r = sum a_e, tb_r = sum b_e.
// Work split: the ENTRIES, not the rows, are cut into chunks of kChunk consecutive entries, one wave
// each (lane = feature, up to kJMax features per lane), so a popular item with thousands of users is
// spread over as many waves as its length asks for. A wave walks the rows its chunk meets; a row
// that lies wholly inside the chunk is written to the output directly, the (at most two) rows cut
// by the chunk's ends go to the chunk's two partial slots (slot 0: the row started before the
// chunk; slot 1: it runs past the chunk's end). A second launch, one thread per (row, feature),
// zeroes the empty rows and adds a cut row's partials in chunk order.
#include <climits>

#include "gdd_common.hpp"

namespace gdd {
namespace {

constexpr int kChunk = 32;    // entries per wave
constexpr int kJMax = 4;      // features per lane
constexpr int kMaxDim = 64 * kJMax;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;  // the same bits in every lane (a + b == b + a)
}

// the non-empty row that holds entry e: the last r with rowptr[r] <= e
__device__ __forceinline__ int64_t row_of(const int32_t* __restrict__ rowptr, int64_t n_rows, int64_t e) {
  int64_t lo = 0, hi = n_rows;  // first index in [0, n_rows] with rowptr[idx] > e
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if ((int64_t)rowptr[mid] <= e) lo = mid + 1; else hi = mid;
  }
  return lo - 1;
}

// floats per partial slot
__host__ __device__ inline int64_t rowpass_slot(int d) { return 3 * (int64_t)d + 1; }
__host__ __device__ inline int64_t wsum_slot(int d) { return (int64_t)d + 2; }

template <int J>
__global__ __launch_bounds__(kThreads) void k_rowpass(
    int64_t n_rows, int64_t n_cols, int64_t nnz, const int32_t* __restrict__ rowptr,
    const int32_t* __restrict__ col, int d, const float* __restrict__ Q, const float* __restrict__ K,
    const float* __restrict__ V, float* __restrict__ s_out, float* __restrict__ s_sum,
    float* __restrict__ SK, float* __restrict__ SV, float* __restrict__ A, float* __restrict__ part,
    int32_t* __restrict__ bad) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  const int64_t b = w * kChunk;
  if (b >= nnz) return;
  const int64_t e_end = b + kChunk < nnz ? b + kChunk : nnz;
  int64_t r = row_of(rowptr, n_rows, b);
  int64_t e = b;
  while (e < e_end && r >= 0 && r < n_rows) {
    const int64_t rs = rowptr[r], re = rowptr[r + 1];
    const int64_t seg_end = re < e_end ? re : e_end;
    if (seg_end <= e) break;  // a rowptr that does not ascend: stop instead of spinning
    float q[J], sk[J], sv[J], a[J], ssum = 0.f;
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const int f = lane + 64 * j;
      q[j] = f < d ? Q[r * d + f] : 0.f;
      sk[j] = sv[j] = a[j] = 0.f;
    }
    for (; e < seg_end; e += 4) {
      int32_t c[4];
      bool ok[4];
      float kk[4][J], vv[4][J];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        c[u] = e + u < seg_end ? col[e + u] : -1;
        ok[u] = c[u] >= 0 && c[u] < n_cols;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int j = 0; j < J; ++j) {
          const int f = lane + 64 * j;
          const bool in = ok[u] && f < d;
          kk[u][j] = in ? K[(int64_t)c[u] * d + f] : 0.f;
          vv[u][j] = in ? V[(int64_t)c[u] * d + f] : 0.f;
        }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (e + u >= seg_end) break;  // wave-uniform
        float p = 0.f;
#pragma unroll
        for (int j = 0; j < J; ++j) p = __builtin_fmaf(q[j], kk[u][j], p);
        p = wave_sum(p);
        if (!ok[u]) {  // not read; reported, and left out of the sums
          if (lane == 0) {
            s_out[e + u] = __builtin_nanf("");
            if (bad) atomicOr(bad, 1);
          }
          continue;
        }
        if (lane == 0) s_out[e + u] = p;
        ssum += p;
#pragma unroll
        for (int j = 0; j < J; ++j) {
          sk[j] += kk[u][j];
          sv[j] += vv[u][j];
          a[j] = __builtin_fmaf(p, vv[u][j], a[j]);
        }
      }
    }
    e = seg_end;
    if (rs >= b && re <= e_end) {
      if (lane == 0) s_sum[r] = ssum;
#pragma unroll
      for (int j = 0; j < J; ++j) {
        const int f = lane + 64 * j;
        if (f < d) {
          SK[r * d + f] = sk[j];
          SV[r * d + f] = sv[j];
          A[r * d + f] = a[j];
        }
      }
    } else {
      float* p = part + (2 * w + (rs < b ? 0 : 1)) * rowpass_slot(d);
      if (lane == 0) p[0] = ssum;
#pragma unroll
      for (int j = 0; j < J; ++j) {
        const int f = lane + 64 * j;
        if (f < d) {
          p[1 + f] = sk[j];
          p[1 + d + f] = sv[j];
          p[1 + 2 * d + f] = a[j];
        }
      }
    }
    // the next non-empty row (empty rows between are the fix-up pass's)
    ++r;
    if (e < e_end && r < n_rows && (int64_t)rowptr[r + 1] <= e) r = row_of(rowptr, n_rows, e);
  }
}

// one thread per (row, feature): zero an empty row, add a cut row's partials in chunk order
__global__ __launch_bounds__(kThreads) void k_rowpass_fix(int64_t n_rows, int64_t nnz, int d,
                                                          const int32_t* __restrict__ rowptr,
                                                          const float* __restrict__ part,
                                                          float* __restrict__ s_sum, float* __restrict__ SK,
                                                          float* __restrict__ SV, float* __restrict__ A) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_rows * d) return;
  const int64_t r = t / d;
  const int f = (int)(t - r * d);
  const int64_t rs = rowptr[r], re = rowptr[r + 1];
  if (re <= rs) {
    if (f == 0) s_sum[r] = 0.f;
    SK[t] = SV[t] = A[t] = 0.f;
    return;
  }
  if (rs < 0 || re > nnz) return;  // a rowptr outside the entries: no partial slot to read
  const int64_t k0 = rs / kChunk, k1 = (re - 1) / kChunk;
  if (k0 == k1) return;  // written whole by its chunk's wave
  float ss = 0.f, sk = 0.f, sv = 0.f, a = 0.f;
  for (int64_t k = k0; k <= k1; ++k) {
    const float* p = part + (2 * k + (k == k0 ? 1 : 0)) * rowpass_slot(d);
    if (f == 0) ss += p[0];
    sk += p[1 + f];
    sv += p[1 + d + f];
    a += p[1 + 2 * d + f];
  }
  if (f == 0) s_sum[r] = ss;
  SK[t] = sk;
  SV[t] = sv;
  A[t] = a;
}

template <int J>
__global__ __launch_bounds__(kThreads) void k_wsum(
    int64_t n_rows, int64_t n_cols, int64_t nnz, const int32_t* __restrict__ rowptr,
    const int32_t* __restrict__ col, int d, const float* __restrict__ wt, const float* __restrict__ V,
    const float* __restrict__ ea, const float* __restrict__ eb, float* __restrict__ Y,
    float* __restrict__ ta, float* __restrict__ tb, float* __restrict__ part, int32_t* __restrict__ bad) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  const int64_t b = w * kChunk;
  if (b >= nnz) return;
  const int64_t e_end = b + kChunk < nnz ? b + kChunk : nnz;
  int64_t r = row_of(rowptr, n_rows, b);
  int64_t e = b;
  while (e < e_end && r >= 0 && r < n_rows) {
    const int64_t rs = rowptr[r], re = rowptr[r + 1];
    const int64_t seg_end = re < e_end ? re : e_end;
    if (seg_end <= e) break;
    float y[J], sa = 0.f, sb = 0.f;
#pragma unroll
    for (int j = 0; j < J; ++j) y[j] = 0.f;
    for (; e < seg_end; e += 4) {
      int32_t c[4];
      bool ok[4];
      float we[4], vv[4][J];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const bool in = e + u < seg_end;
        c[u] = in ? col[e + u] : -1;
        ok[u] = c[u] >= 0 && c[u] < n_cols;
        we[u] = in ? wt[e + u] : 0.f;
        if (in && !ok[u] && lane == 0 && bad) atomicOr(bad, 1);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int j = 0; j < J; ++j) {
          const int f = lane + 64 * j;
          vv[u][j] = ok[u] && f < d ? V[(int64_t)c[u] * d + f] : 0.f;
        }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (e + u >= seg_end) break;
        if (!ok[u]) continue;
        if (ea) sa += ea[e + u];
        if (eb) sb += eb[e + u];
#pragma unroll
        for (int j = 0; j < J; ++j) y[j] = __builtin_fmaf(we[u], vv[u][j], y[j]);
      }
    }
    e = seg_end;
    if (rs >= b && re <= e_end) {
      if (lane == 0) {
        if (ta) ta[r] = sa;
        if (tb) tb[r] = sb;
      }
#pragma unroll
      for (int j = 0; j < J; ++j) {
        const int f = lane + 64 * j;
        if (f < d) Y[r * d + f] = y[j];
      }
    } else {
      float* p = part + (2 * w + (rs < b ? 0 : 1)) * wsum_slot(d);
      if (lane == 0) {
        p[0] = sa;
        p[1] = sb;
      }
#pragma unroll
      for (int j = 0; j < J; ++j) {
        const int f = lane + 64 * j;
        if (f < d) p[2 + f] = y[j];
      }
    }
    ++r;
    if (e < e_end && r < n_rows && (int64_t)rowptr[r + 1] <= e) r = row_of(rowptr, n_rows, e);
  }
}

__global__ __launch_bounds__(kThreads) void k_wsum_fix(int64_t n_rows, int64_t nnz, int d,
                                                       const int32_t* __restrict__ rowptr,
                                                       const float* __restrict__ part, float* __restrict__ Y,
                                                       float* __restrict__ ta, float* __restrict__ tb) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_rows * d) return;
  const int64_t r = t / d;
  const int f = (int)(t - r * d);
  const int64_t rs = rowptr[r], re = rowptr[r + 1];
  if (re <= rs) {
    if (f == 0) {
      if (ta) ta[r] = 0.f;
      if (tb) tb[r] = 0.f;
    }
    Y[t] = 0.f;
    return;
  }
  if (rs < 0 || re > nnz) return;  // a rowptr outside the entries: no partial slot to read
  const int64_t k0 = rs / kChunk, k1 = (re - 1) / kChunk;
  if (k0 == k1) return;
  float y = 0.f, sa = 0.f, sb = 0.f;
  for (int64_t k = k0; k <= k1; ++k) {
    const float* p = part + (2 * k + (k == k0 ? 1 : 0)) * wsum_slot(d);
    if (f == 0) {
      sa += p[0];
      sb += p[1];
    }
    y += p[2 + f];
  }
  if (f == 0) {
    if (ta) ta[r] = sa;
    if (tb) tb[r] = sb;
  }
  Y[t] = y;
}

int64_t n_chunks(int64_t nnz) { return (nnz + kChunk - 1) / kChunk; }
unsigned chunk_grid(int64_t nnz) { return (unsigned)((n_chunks(nnz) + kWaves - 1) / kWaves); }
unsigned elem_grid(int64_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

int check_shape(const char* who, int64_t n_rows, int64_t n_cols, int64_t nnz, int d) {
  GDD_REQUIRE(n_rows >= 0 && n_cols >= 0 && nnz >= 0 && nnz < INT_MAX && n_rows < INT_MAX &&
                  n_cols < INT_MAX && n_rows * (int64_t)kMaxDim < ((int64_t)1 << 40),
              "%s: bad shape", who);
  GDD_REQUIRE(d >= 1 && d <= kMaxDim, "%s: d=%d outside [1, %d]", who, d, kMaxDim);
  return GDD_OK;
}

}  // namespace
}  // namespace gdd

using namespace gdd;

extern "C" int gdd_rank_max_dim(void) { return kMaxDim; }

extern "C" size_t gdd_rank_ws_bytes(int64_t nnz, int d) {
  if (nnz < 0 || d < 1) return 256;
  return align256(sizeof(float) * (size_t)(2 * n_chunks(nnz) * rowpass_slot(d))) + 256;
}

extern "C" int gdd_rank_rowpass(int64_t n_rows, int64_t n_cols, int64_t nnz, const int32_t* rowptr,
                                const int32_t* col, int d, const float* Q, const float* K, const float* V,
                                float* s_out, float* s_sum, float* SK, float* SV, float* A, int32_t* bad,
                                void* ws, size_t ws_bytes, gdd_stream_t stream) {
  int rc = check_shape("rank_rowpass", n_rows, n_cols, nnz, d);
  if (rc) return rc;
  if (n_rows == 0) return GDD_OK;
  GDD_REQUIRE(rowptr && Q && s_sum && SK && SV && A, "rank_rowpass: null pointer");
  GDD_REQUIRE(nnz == 0 || (col && K && V && s_out && ws), "rank_rowpass: null pointer");
  if (ws_bytes < gdd_rank_ws_bytes(nnz, d)) return fail(GDD_E_WORKSPACE, "rank_rowpass: workspace too small");
  hipStream_t s = to_hip(stream);
  float* part = static_cast<float*>(ws);
  if (nnz > 0) {
    const unsigned g = chunk_grid(nnz);
#define GDD_RP(J)                                                                                   \
  k_rowpass<J><<<g, kThreads, 0, s>>>(n_rows, n_cols, nnz, rowptr, col, d, Q, K, V, s_out, s_sum, SK, \
                                      SV, A, part, bad)
    switch ((d + 63) / 64) {
      case 1: GDD_RP(1); break;
      case 2: GDD_RP(2); break;
      case 3: GDD_RP(3); break;
      default: GDD_RP(4); break;
    }
#undef GDD_RP
    GDD_LAUNCHED();
  }
  k_rowpass_fix<<<elem_grid(n_rows * d), kThreads, 0, s>>>(n_rows, nnz, d, rowptr, part, s_sum, SK, SV, A);
  GDD_LAUNCHED();
  return GDD_OK;
}

extern "C" int gdd_rank_wsum(int64_t n_rows, int64_t n_cols, int64_t nnz, const int32_t* rowptr,
                             const int32_t* col, int d, const float* w, const float* V, const float* a,
                             const float* b, float* Y, float* ta, float* tb, int32_t* bad, void* ws,
                             size_t ws_bytes, gdd_stream_t stream) {
  int rc = check_shape("rank_wsum", n_rows, n_cols, nnz, d);
  if (rc) return rc;
  if (n_rows == 0) return GDD_OK;
  GDD_REQUIRE(rowptr && Y, "rank_wsum: null pointer");
  GDD_REQUIRE(nnz == 0 || (col && w && V && ws), "rank_wsum: null pointer");
  GDD_REQUIRE((!a || ta) && (!b || tb), "rank_wsum: edge scalars without an output");
  if (ws_bytes < gdd_rank_ws_bytes(nnz, d)) return fail(GDD_E_WORKSPACE, "rank_wsum: workspace too small");
  hipStream_t s = to_hip(stream);
  float* part = static_cast<float*>(ws);
  // an edge array of no entries has no address (a caller's empty tensor is a null pointer): with
  // nnz == 0 a row sum that was asked for is all zeros, not left unwritten
  float* ta_o = (a || nnz == 0) ? ta : nullptr;
  float* tb_o = (b || nnz == 0) ? tb : nullptr;
  if (nnz > 0) {
    const unsigned g = chunk_grid(nnz);
#define GDD_WS(J)                                                                                  \
  k_wsum<J><<<g, kThreads, 0, s>>>(n_rows, n_cols, nnz, rowptr, col, d, w, V, a, b, Y, ta_o, tb_o, part, \
                                   bad)
    switch ((d + 63) / 64) {
      case 1: GDD_WS(1); break;
      case 2: GDD_WS(2); break;
      case 3: GDD_WS(3); break;
      default: GDD_WS(4); break;
    }
#undef GDD_WS
    GDD_LAUNCHED();
  }
  k_wsum_fix<<<elem_grid(n_rows * d), kThreads, 0, s>>>(n_rows, nnz, d, rowptr, part, Y, ta_o, tb_o);
  GDD_LAUNCHED();
  return GDD_OK;
}
