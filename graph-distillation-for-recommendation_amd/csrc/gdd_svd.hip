// gdd_svd.hip — device truncated SVD of the recommender's interaction matrix (distill_recsys.py
// :124-155, compute_svd_embeddings), all in fp64: block subspace iteration with Rayleigh-Ritz.
//
// One plain step is W = A V, Z = Aᵀ W, V = CholeskyQR2(Z) with A the interaction matrix oriented so
// that V lives on its smaller side; gdd_svd_segment enqueues `steps` of them back to back. The host
// (gdd/svd.py) only runs the b x b eigenproblem of the check steps and reads the residuals and the
// breakdown flag there. DESIGN.md "Device truncated SVD" has the algorithm and the summation orders:
//   spmm      every output element is one mul-then-add chain from +0 in CSR entry order (no fma);
//   gram      row blocks of W, each summed rows-ascending by one wave (4 rows per MFMA), the blocks'
//             partial tiles then added in block order; only tiles on or above the diagonal are
//             computed and the reduction mirrors them, so G is symmetric bit for bit;
//   tsmm      the inner index ascending, 4 per MFMA;
//   residual  row blocks summed rows-ascending, partials added in block order.
// No floating-point atomics anywhere, so two calls on the same input give the same bits.
#include <algorithm>
#include <climits>

#include "gdd_common.hpp"

namespace gdd {
namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int kMaxB = 128;        // a b x b fp64 matrix (odd row stride) fits the 160 KiB LDS
constexpr int kGramMaxBlocks = 256;
constexpr int kResidRows = 64;
// the Gram kernel's default form: 0 = v_mfma_f64_16x16x4_f64, 1 = plain fp64 fma
// (profiles/svd_device.json has both times)
constexpr int kGramDefaultForm = 0;

unsigned grid1(int64_t n, int t) { return (unsigned)((n + t - 1) / t); }

// ---- Y = A X -----------------------------------------------------------------------------------
// one wave per (row, 64 output columns): the row is wave-uniform, so its column indices and values
// come through the scalar cache, 8 entries ahead of the chain that consumes them
__global__ __launch_bounds__(256) void k_spmm_f64(int64_t n_rows, int64_t n_cols,
                                                  const int32_t* __restrict__ rowptr,
                                                  const int32_t* __restrict__ col,
                                                  const float* __restrict__ val, int b, int nchunk,
                                                  const double* __restrict__ X, double* __restrict__ Y) {
  const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t row64 = w / nchunk;
  if (row64 >= n_rows) return;
  const int row = __builtin_amdgcn_readfirstlane((int)row64);
  const int chunk = __builtin_amdgcn_readfirstlane((int)(w - row64 * nchunk));
  const int c = chunk * 64 + (threadIdx.x & 63);
  const bool live = c < b;
  const int cc = live ? c : 0;
  const int32_t p0 = rowptr[row], p1 = rowptr[row + 1];
  const uint32_t nc = (uint32_t)n_cols;
  double acc = 0.0;
  int32_t p = p0;
  for (; p + 8 <= p1; p += 8) {
    int32_t j[8];
    double a[8], x[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      j[u] = col[p + u];
      a[u] = val ? (double)val[p + u] : 1.0;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) x[u] = (uint32_t)j[u] < nc ? X[(int64_t)j[u] * b + cc] : 0.0;  // never read outside X
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if ((uint32_t)j[u] < nc) acc = acc + a[u] * x[u];
  }
  for (; p < p1; ++p) {
    const int32_t j = col[p];
    if ((uint32_t)j >= nc) continue;
    const double a = val ? (double)val[p] : 1.0;
    acc = acc + a * X[(int64_t)j * b + cc];
  }
  if (live) Y[(int64_t)row * b + c] = acc;
}

// ---- G = Wᵀ W ----------------------------------------------------------------------------------
// grid (row blocks, tile pairs ib <= jb), one wave each; part[rb] is a bp x bp image of which only
// the computed tiles are written (and read).
__device__ __forceinline__ void pair_of(int p, int nt, int& ib, int& jb) {
  ib = 0;
  while (p >= nt - ib) {
    p -= nt - ib;
    ++ib;
  }
  jb = ib + p;
}

__global__ __launch_bounds__(64) void k_gram_mfma(int64_t n, int b, int nt, int64_t rb_rows,
                                                  const double* __restrict__ W,
                                                  double* __restrict__ part) {
  int ib, jb;
  pair_of(blockIdx.y, nt, ib, jb);
  const int lane = threadIdx.x, kk = lane >> 4, c = lane & 15;
  const int ci = ib * 16 + c, cj = jb * 16 + c;
  const bool vi = ci < b, vj = cj < b;
  const int64_t r0 = (int64_t)blockIdx.x * rb_rows, r1 = r0 + rb_rows < n ? r0 + rb_rows : n;
  d4 acc = {0.0, 0.0, 0.0, 0.0};
  // A[i][k] = W[r + k][16 ib + i] on lane (i = lane & 15, k = lane >> 4), B[k][j] likewise
  for (int64_t r = r0; r < r1; r += 4) {
    const int64_t rr = r + kk;
    const bool in = rr < r1;
    const double a = (in && vi) ? W[rr * b + ci] : 0.0;
    const double bb = (in && vj) ? W[rr * b + cj] : 0.0;
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bb, acc, 0, 0, 0);
  }
  const int bp = nt * 16;
  double* out = part + (int64_t)blockIdx.x * bp * bp;
  // C/D of the f64 form: col = lane & 15, row = (lane >> 4) + 4 reg
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) out[(int64_t)(ib * 16 + kk + 4 * reg) * bp + jb * 16 + c] = acc[reg];
}

__global__ __launch_bounds__(64) void k_gram_fma(int64_t n, int b, int nt, int64_t rb_rows,
                                                 const double* __restrict__ W,
                                                 double* __restrict__ part) {
  int ib, jb;
  pair_of(blockIdx.y, nt, ib, jb);
  const int lane = threadIdx.x, q = lane >> 4, c = lane & 15;
  const int cj = jb * 16 + c;
  const bool vj = cj < b;
  const int64_t r0 = (int64_t)blockIdx.x * rb_rows, r1 = r0 + rb_rows < n ? r0 + rb_rows : n;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 2
  for (int64_t r = r0; r < r1; ++r) {
    const double bj = vj ? W[r * b + cj] : 0.0;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int ci = ib * 16 + q + 4 * reg;
      const double ai = ci < b ? W[r * b + ci] : 0.0;
      acc[reg] = fma(ai, bj, acc[reg]);
    }
  }
  const int bp = nt * 16;
  double* out = part + (int64_t)blockIdx.x * bp * bp;
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) out[(int64_t)(ib * 16 + q + 4 * reg) * bp + jb * 16 + c] = acc[reg];
}

__global__ __launch_bounds__(256) void k_gram_reduce(int nrb, int b, int bp, const double* __restrict__ part,
                                                     double* __restrict__ G) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= b * b) return;
  const int i = idx / b, j = idx - i * b;
  if (i > j) return;
  double s = 0.0;
  for (int rb = 0; rb < nrb; ++rb) s = s + part[((int64_t)rb * bp + i) * bp + j];
  G[i * b + j] = s;
  G[j * b + i] = s;
}

struct GramPlan {
  int nt, bp, nrb;
  int64_t rb_rows;
};
GramPlan gram_plan(int64_t n, int b) {
  GramPlan g;
  g.nt = (b + 15) / 16;
  g.bp = g.nt * 16;
  int64_t nrb = std::min<int64_t>((n + 255) / 256, kGramMaxBlocks);
  if (nrb < 1) nrb = 1;
  int64_t rows = (n + nrb - 1) / nrb;
  rows = (rows + 3) & ~int64_t(3);
  g.rb_rows = rows;
  g.nrb = (int)((n + rows - 1) / rows);
  return g;
}
size_t gram_ws(int64_t n, int b) {
  const GramPlan g = gram_plan(n, b);
  return align256(sizeof(double) * (size_t)g.nrb * g.bp * g.bp) + 256;
}

int gram_dev(int64_t n, int b, const double* W, double* G, int form, void* ws, size_t ws_bytes,
             hipStream_t s) {
  const GramPlan g = gram_plan(n, b);
  Carver cv(ws, ws_bytes);
  double* part = cv.take<double>((size_t)g.nrb * g.bp * g.bp);
  if (!cv.ok()) return fail(GDD_E_WORKSPACE, "gram_f64: workspace too small");
  const dim3 grid((unsigned)g.nrb, (unsigned)(g.nt * (g.nt + 1) / 2));
  if (form < 0) form = kGramDefaultForm;
  if (form == 0)
    k_gram_mfma<<<grid, 64, 0, s>>>(n, b, g.nt, g.rb_rows, W, part);
  else
    k_gram_fma<<<grid, 64, 0, s>>>(n, b, g.nt, g.rb_rows, W, part);
  GDD_LAUNCHED();
  k_gram_reduce<<<grid1((int64_t)b * b, 256), 256, 0, s>>>(g.nrb, b, g.bp, part, G);
  GDD_LAUNCHED();
  return GDD_OK;
}

// ---- out = W Q (Q b x b) -----------------------------------------------------------------------
// one block per 16 rows, one wave per 16 output columns
__global__ __launch_bounds__(512) void k_tsmm_mfma(int64_t n, int b, const double* __restrict__ W,
                                                   const double* __restrict__ Q,
                                                   double* __restrict__ out) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, kk = lane >> 4, c = lane & 15;
  const int64_t r0 = (int64_t)blockIdx.x * 16;
  const int64_t ra = r0 + c;  // A[i][k] = W[r0 + i][k0 + k] on lane (i = lane & 15, k = lane >> 4)
  const int cq = w * 16 + c;  // B[k][j] = Q[k0 + k][16 w + j]
  const bool va = ra < n, vq = cq < b;
  d4 acc = {0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < b; k0 += 4) {
    const int k = k0 + kk;
    const bool in = k < b;
    const double a = (in && va) ? W[ra * b + k] : 0.0;
    const double q = (in && vq) ? Q[k * b + cq] : 0.0;
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, q, acc, 0, 0, 0);
  }
  if (!vq) return;
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const int64_t r = r0 + kk + 4 * reg;
    if (r < n) out[r * b + cq] = acc[reg];
  }
}

int tsmm_dev(int64_t n, int b, const double* W, const double* Q, double* out, hipStream_t s) {
  const int nt = (b + 15) / 16;
  k_tsmm_mfma<<<grid1(n, 16), 64 * nt, 0, s>>>(n, b, W, Q, out);
  GDD_LAUNCHED();
  return GDD_OK;
}

// ---- Cholesky G = Rᵀ R and R⁻¹, one workgroup, G in the LDS -------------------------------------
// Row elimination of [G | I] in place: step j subtracts f_i = A[j][i] (1 / d_j) times row j from every
// row i > j, d_j = A[j][j] being the Cholesky pivot L[j][j]². The trailing matrix lives in the upper
// triangle (symmetry gives the multipliers from row j itself), the multiplier matrix E = D^1/2 L⁻¹
// in the strict lower one where G has been eliminated, so row j is read-only in step j and a step
// needs one barrier. R⁻¹[k][j] = E[j][k] / sqrt(d_j). A pivot at or below b 2^-52 max diag (or NaN) is
// a breakdown: *flag = 1 and Rinv = I, so that the product that follows leaves its block unchanged.
constexpr int kCholThreads = 1024;
__global__ __launch_bounds__(kCholThreads) void k_chol_inv(int b, const double* __restrict__ G,
                                                           double* __restrict__ Rinv,
                                                           int32_t* __restrict__ flag) {
  extern __shared__ double sm[];
  const int ld = b | 1;
  double* A = sm;  // b x ld
  __shared__ double s_thresh;
  const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
  for (int e = tid; e < b * b; e += kCholThreads) A[(e / b) * ld + (e % b)] = G[e];
  if (tid < 64) {  // max is order-free
    double mx = 0.0;
    for (int i = tid; i < b; i += 64) mx = fmax(mx, G[i * b + i]);
    for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o));
    if (tid == 0) s_thresh = (double)b * 0x1p-52 * mx;
  }
  __syncthreads();
  const double thresh = s_thresh;
  bool bad = false;
  for (int j = 0; j < b; ++j) {
    const double d = A[j * ld + j];
    if (!(d > thresh)) {  // the same value on every thread
      bad = true;
      break;
    }
    const double* rj = A + j * ld;
    const double rd = 1.0 / d;
    double rk[4];  // this thread's four columns of row j (b <= 128 = 4 x 32)
#pragma unroll
    for (int u = 0; u < 4; ++u) rk[u] = tx + 32 * u < b ? rj[tx + 32 * u] : 0.0;
    for (int i = j + 1 + ty; i < b; i += 32) {
      const double f = rj[i] * rd;
      double* ri = A + i * ld;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int k = tx + 32 * u;
        if (k < b && (k <= j || k >= i)) ri[k] = k == j ? -f : fma(-f, rk[u], ri[k]);
      }
    }
    __syncthreads();
  }
  if (bad) {
    for (int e = tid; e < b * b; e += kCholThreads) Rinv[e] = (e / b == e % b) ? 1.0 : 0.0;
    if (tid == 0) *flag = 1;
    return;
  }
  for (int e = tid; e < b * b; e += kCholThreads) {
    const int k = e / b, j = e % b;
    const double s = sqrt(A[j * ld + j]);
    Rinv[e] = k < j ? A[j * ld + k] / s : (k == j ? 1.0 / s : 0.0);
  }
}

size_t chol_lds(int b) { return sizeof(double) * ((size_t)b * (b | 1)); }

int chol_dev(int b, const double* G, double* Rinv, int32_t* flag, hipStream_t s) {
  const size_t lds = chol_lds(b);
  if (lds > 65536)
    GDD_HIP(hipFuncSetAttribute((const void*)k_chol_inv, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lds));
  k_chol_inv<<<1, kCholThreads, lds, s>>>(b, G, Rinv, flag);
  GDD_LAUNCHED();
  return GDD_OK;
}

// ---- CholeskyQR2: two passes of gram, Cholesky-and-inverse, Z R⁻¹ ------------------------------
struct QrWs {
  double *T, *G, *Rinv;
  void* gram;
  size_t gram_bytes;
};
size_t qr_ws(int64_t n, int b) {
  return align256(sizeof(double) * (size_t)n * b) + 2 * align256(sizeof(double) * (size_t)b * b) +
         gram_ws(n, b) + 1024;
}
bool qr_carve(Carver& cv, int64_t n, int b, QrWs& w) {
  w.T = cv.take<double>((size_t)n * b);
  w.G = cv.take<double>((size_t)b * b);
  w.Rinv = cv.take<double>((size_t)b * b);
  w.gram_bytes = gram_ws(n, b);
  w.gram = cv.take<char>(w.gram_bytes);
  return cv.ok();
}
int cholqr2_dev(int64_t n, int b, const double* Z, double* V, int32_t* flag, const QrWs& w,
                hipStream_t s) {
  int rc;
  if ((rc = gram_dev(n, b, Z, w.G, -1, w.gram, w.gram_bytes, s))) return rc;
  if ((rc = chol_dev(b, w.G, w.Rinv, flag, s))) return rc;
  if ((rc = tsmm_dev(n, b, Z, w.Rinv, w.T, s))) return rc;
  if ((rc = gram_dev(n, b, w.T, w.G, -1, w.gram, w.gram_bytes, s))) return rc;
  if ((rc = chol_dev(b, w.G, w.Rinv, flag, s))) return rc;
  return tsmm_dev(n, b, w.T, w.Rinv, V, s);
}

int spmm_dev(int64_t n_rows, int64_t n_cols, const int32_t* rowptr, const int32_t* col,
             const float* val, int b, const double* X, double* Y, hipStream_t s) {
  const int nchunk = (b + 63) / 64;
  k_spmm_f64<<<grid1(n_rows * nchunk, 4), 256, 0, s>>>(n_rows, n_cols, rowptr, col, val, b, nchunk, X, Y);
  GDD_LAUNCHED();
  return GDD_OK;
}

// ---- residuals r_j = ||Z_j - lam_j V_j||_2, j < k ----------------------------------------------
__global__ __launch_bounds__(128) void k_resid_part(int64_t n, int b, int k, const double* __restrict__ Z,
                                                    const double* __restrict__ V,
                                                    const double* __restrict__ lam,
                                                    double* __restrict__ part) {
  const int j = threadIdx.x;
  if (j >= k) return;
  const int64_t r0 = (int64_t)blockIdx.x * kResidRows, r1 = r0 + kResidRows < n ? r0 + kResidRows : n;
  const double l = lam[j];
  double s = 0.0;
  for (int64_t r = r0; r < r1; ++r) {
    const double d = Z[r * b + j] - l * V[r * b + j];
    s = s + d * d;
  }
  part[(int64_t)blockIdx.x * k + j] = s;
}
__global__ __launch_bounds__(128) void k_resid_fin(int nrb, int k, const double* __restrict__ part,
                                                   double* __restrict__ r) {
  const int j = threadIdx.x;
  if (j >= k) return;
  double s = 0.0;
  for (int rb = 0; rb < nrb; ++rb) s = s + part[(int64_t)rb * k + j];
  r[j] = sqrt(s);
}

// ---- finalise: sign convention, 1/sigma, sqrt(sigma) scaling, fp32 cast --------------------------
// sign[j] makes the entry of small-side column j with the largest magnitude positive (lowest row on ties)
__global__ __launch_bounds__(256) void k_svd_sign(int64_t n, int b, const double* __restrict__ V,
                                                  double* __restrict__ sign) {
  __shared__ double s_abs[256];
  __shared__ long long s_idx[256];
  const int j = blockIdx.x, tid = threadIdx.x;
  double best = -1.0;
  long long bi = 0;
  for (int64_t r = tid; r < n; r += 256) {
    const double a = fabs(V[r * b + j]);
    if (a > best) {  // rows ascending per thread: the first of equals stays
      best = a;
      bi = r;
    }
  }
  s_abs[tid] = best;
  s_idx[tid] = bi;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) {
      const double a = s_abs[tid + h];
      const long long i = s_idx[tid + h];
      if (a > s_abs[tid] || (a == s_abs[tid] && i < s_idx[tid])) {
        s_abs[tid] = a;
        s_idx[tid] = i;
      }
    }
    __syncthreads();
  }
  if (tid == 0) sign[j] = (s_abs[0] >= 0.0 && V[s_idx[0] * b + j] < 0.0) ? -1.0 : 1.0;
}

__global__ __launch_bounds__(256) void k_svd_final(int64_t n, int b, int k, int big,
                                                   const double* __restrict__ X,
                                                   const double* __restrict__ lam,
                                                   const double* __restrict__ sign,
                                                   double* __restrict__ out, float* __restrict__ emb) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n * k) return;
  const int64_t r = idx / k;
  const int j = (int)(idx - r * k);
  const double sigma = sqrt(fmax(lam[j], 0.0));
  double x = sign[j] * X[r * b + j];
  if (big) x = sigma > 0.0 ? x / sigma : 0.0;
  if (out) out[idx] = x;
  if (emb) emb[idx] = (float)(x * sqrt(fmax(sigma, 1e-12)));
}
__global__ void k_svd_sigma(int k, const double* __restrict__ lam, double* __restrict__ S) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < k) S[j] = sqrt(fmax(lam[j], 0.0));
}

bool shape_ok(int64_t n, int b) { return n > 0 && n < INT_MAX && b > 0 && b <= kMaxB && n * b < ((int64_t)1 << 38); }

}  // namespace
}  // namespace gdd

using namespace gdd;

extern "C" int gdd_svd_max_block(void) { return kMaxB; }

extern "C" int gdd_spmm_f64(int64_t n_rows, int64_t n_cols, const int32_t* rowptr, const int32_t* col,
                            const float* val, int b, const double* X, double* Y, gdd_stream_t stream) {
  GDD_REQUIRE(shape_ok(n_rows, b) && n_cols > 0 && n_cols < INT_MAX, "spmm_f64: bad shape");
  GDD_REQUIRE(rowptr && col && X && Y, "spmm_f64: null pointer");
  return spmm_dev(n_rows, n_cols, rowptr, col, val, b, X, Y, to_hip(stream));
}

extern "C" size_t gdd_gram_f64_ws_bytes(int64_t n_rows, int b) {
  if (!shape_ok(n_rows, b)) return 0;
  return gram_ws(n_rows, b);
}

extern "C" int gdd_gram_f64(int64_t n_rows, int b, const double* W, double* G, int form, void* ws,
                            size_t ws_bytes, gdd_stream_t stream) {
  GDD_REQUIRE(shape_ok(n_rows, b) && form >= -1 && form <= 1, "gram_f64: bad shape");
  GDD_REQUIRE(W && G && ws, "gram_f64: null pointer");
  return gram_dev(n_rows, b, W, G, form, ws, ws_bytes, to_hip(stream));
}

extern "C" int gdd_tsmm_f64(int64_t n_rows, int b, const double* W, const double* Q, double* out,
                            gdd_stream_t stream) {
  GDD_REQUIRE(shape_ok(n_rows, b), "tsmm_f64: bad shape");
  GDD_REQUIRE(W && Q && out && out != W, "tsmm_f64: null or aliased pointer");
  return tsmm_dev(n_rows, b, W, Q, out, to_hip(stream));
}

extern "C" int gdd_chol_inv_f64(int b, const double* G, double* Rinv, int32_t* flag,
                                gdd_stream_t stream) {
  static_assert(kMaxB <= 4 * 32, "k_chol_inv keeps four columns per thread");
  GDD_REQUIRE(b > 0 && b <= kMaxB, "chol_inv_f64: b must be in 1 .. 128");
  GDD_REQUIRE(G && Rinv && flag, "chol_inv_f64: null pointer");
  return chol_dev(b, G, Rinv, flag, to_hip(stream));
}

extern "C" size_t gdd_cholqr2_ws_bytes(int64_t n_rows, int b) {
  if (!shape_ok(n_rows, b)) return 0;
  return qr_ws(n_rows, b);
}

extern "C" int gdd_cholqr2_f64(int64_t n_rows, int b, const double* Z, double* V, int32_t* flag,
                               void* ws, size_t ws_bytes, gdd_stream_t stream) {
  GDD_REQUIRE(shape_ok(n_rows, b), "cholqr2_f64: bad shape");
  GDD_REQUIRE(Z && V && flag && ws, "cholqr2_f64: null pointer");
  Carver cv(ws, ws_bytes);
  QrWs w;
  if (!qr_carve(cv, n_rows, b, w)) return fail(GDD_E_WORKSPACE, "cholqr2_f64: workspace too small");
  return cholqr2_dev(n_rows, b, Z, V, flag, w, to_hip(stream));
}

extern "C" size_t gdd_svd_segment_ws_bytes(int64_t n_big, int64_t n_small, int b) {
  if (!shape_ok(n_big, b) || !shape_ok(n_small, b)) return 0;
  return qr_ws(n_small, b);
}

extern "C" int gdd_svd_segment(int64_t n_big, int64_t n_small, const int32_t* rowptr, const int32_t* col,
                               const float* val, const int32_t* rowptr_t, const int32_t* col_t,
                               const float* val_t, int b, int steps, double* V, double* W, double* Z,
                               int32_t* flag, void* ws, size_t ws_bytes, gdd_stream_t stream) {
  GDD_REQUIRE(shape_ok(n_big, b) && shape_ok(n_small, b) && steps >= 0, "svd_segment: bad shape");
  GDD_REQUIRE(rowptr && col && rowptr_t && col_t && V && W && Z && flag && ws, "svd_segment: null pointer");
  hipStream_t s = to_hip(stream);
  Carver cv(ws, ws_bytes);
  QrWs w;
  if (!qr_carve(cv, n_small, b, w)) return fail(GDD_E_WORKSPACE, "svd_segment: workspace too small");
  for (int i = 0; i < steps; ++i) {
    int rc;
    if ((rc = spmm_dev(n_big, n_small, rowptr, col, val, b, V, W, s))) return rc;
    if ((rc = spmm_dev(n_small, n_big, rowptr_t, col_t, val_t, b, W, Z, s))) return rc;
    if ((rc = cholqr2_dev(n_small, b, Z, V, flag, w, s))) return rc;
  }
  return GDD_OK;
}

extern "C" size_t gdd_svd_residuals_ws_bytes(int64_t n, int k) {
  if (n <= 0 || k <= 0) return 0;
  return align256(sizeof(double) * (size_t)((n + kResidRows - 1) / kResidRows) * k) + 256;
}

extern "C" int gdd_svd_residuals(int64_t n, int b, int k, const double* Z, const double* V,
                                 const double* lam, double* r, void* ws, size_t ws_bytes,
                                 gdd_stream_t stream) {
  GDD_REQUIRE(shape_ok(n, b) && k > 0 && k <= b, "svd_residuals: bad shape");
  GDD_REQUIRE(Z && V && lam && r && ws, "svd_residuals: null pointer");
  hipStream_t s = to_hip(stream);
  const int nrb = (int)((n + kResidRows - 1) / kResidRows);
  Carver cv(ws, ws_bytes);
  double* part = cv.take<double>((size_t)nrb * k);
  if (!cv.ok()) return fail(GDD_E_WORKSPACE, "svd_residuals: workspace too small");
  k_resid_part<<<nrb, 128, 0, s>>>(n, b, k, Z, V, lam, part);
  GDD_LAUNCHED();
  k_resid_fin<<<1, 128, 0, s>>>(nrb, k, part, r);
  GDD_LAUNCHED();
  return GDD_OK;
}

extern "C" int gdd_svd_finalize(int64_t n_small, int64_t n_big, int b, int k, const double* V,
                                const double* W, const double* lam, double* S, double* V_out,
                                double* U_out, float* emb_small, float* emb_big, double* sign,
                                gdd_stream_t stream) {
  GDD_REQUIRE(shape_ok(n_small, b) && shape_ok(n_big, b) && k > 0 && k <= b, "svd_finalize: bad shape");
  GDD_REQUIRE(V && W && lam && S && sign, "svd_finalize: null pointer");
  hipStream_t s = to_hip(stream);
  k_svd_sign<<<k, 256, 0, s>>>(n_small, b, V, sign);
  GDD_LAUNCHED();
  k_svd_sigma<<<1, 128, 0, s>>>(k, lam, S);
  GDD_LAUNCHED();
  if (V_out || emb_small) {
    k_svd_final<<<grid1(n_small * k, 256), 256, 0, s>>>(n_small, b, k, 0, V, lam, sign, V_out, emb_small);
    GDD_LAUNCHED();
  }
  if (U_out || emb_big) {
    k_svd_final<<<grid1(n_big * k, 256), 256, 0, s>>>(n_big, b, k, 1, W, lam, sign, U_out, emb_big);
    GDD_LAUNCHED();
  }
  return GDD_OK;
}
