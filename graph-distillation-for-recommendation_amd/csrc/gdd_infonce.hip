// gdd_infonce.hip — the Rankformer teacher's contrastive loss (Rankformer/code/model.py:10-24 InfoNCE,
// :449-465 its use in the loss) as two streaming passes that never store a logit (DESIGN.md
// "Contrastive loss"). A, Y are B x d fp32 row-major, l_rc = inv_tau <A_r, Y_c>:
//   * gdd_infonce_rows: lse_r = log sum_c exp(l_rc), diag_r = l_rr, R_r = sum_c P_rc Y_c with
//     P_rc = exp(l_rc - lse_r) (online softmax: running maximum, running sum, R rescaled when the
//     maximum rises);
//   * gdd_infonce_cols: C_c = sum_r G_r P_rc A_r, P recomputed from the lse the row pass wrote.
// One kernel body serves both. A workgroup of 4 waves owns 128 rows of its RESIDENT matrix (A in the
// row pass, Y in the column pass), 32 per wave, held in registers as the B operand of
// v_mfma_f32_32x32x2_f32. The STREAMED matrix (Y / A) goes through the LDS in tiles of 32 rows in
// ascending order, the next tile's global loads in flight while the current one is used (not at
// DP = 256, where the staging registers do not fit beside the operands). Per tile a
// wave computes the 32 x 32 score tile with the streamed index on the accumulator's rows (registers)
// and its own rows on the lanes, so
//   - a reduction over the streamed index is 16 register operations and one exchange of the lane
//     halves, and
//   - the weight tile is, as it stands, the A operand of the second product
//     out[own][f] += sum_streamed w[streamed][own] * tile[streamed][f],
//     whose B operand is read from the same LDS tile. No score, weight or probability leaves the
//     registers.
// The f32-input MFMA is a k-ordered fmaf chain, so <A_r, Y_c> is the chain over f = 0 .. d-1 starting
// from +0 in both passes (fma(y, a, s) in the row pass, fma(a, y, s) in the column pass: the same
// bits), every sum has a fixed order, there are no atomics and no workspace: two runs give the same
// bits. Features are padded with zeros to DP (a multiple of 32, one instantiation each); rows past B
// are zeros in the LDS and -inf logits (row pass) or zero weights (column pass).
// The diagonal term is added last. The gradients are R_r - Y_r and C_c - G_c A_c, and with y close to
// x (what a contrastive pair is) P_rr is close to 1: R_r is mostly Y_r, C_c mostly G_c A_c, and the
// difference keeps whatever rounding the large term picked up on its way through a B-term chain
// (measured: 5.4 x the reference's fp32 error at B = 65, the reference subtracts the identity from
// P before its product). So both passes leave the diagonal element out of the chain and add
// P_rr Y_r (G_c P_cc A_c) to the finished sum: one rounding of the large term, which the
// subtraction then removes almost exactly. P_rr comes from the row pass's running sums (pd): from
// the fp32 lse the column pass could only recover it to u |lse|.
#include <climits>

#include "gdd_common.hpp"

namespace gdd {
namespace {

constexpr int kThreadsNce = 256;
constexpr int kWavesNce = kThreadsNce / 64;
constexpr int kOwnRows = 32 * kWavesNce;  // resident rows per workgroup
constexpr int kTileRows = 32;             // streamed rows per LDS tile
constexpr int kMaxDimNce = 256;           // gdd_rank_max_dim()

typedef float f32x16 __attribute__((ext_vector_type(16)));

// accumulator register g of lane half h holds row acc_row(g, h) of the 32 x 32 tile (column = lane & 31)
__device__ __forceinline__ int acc_row(int g, int h) { return (g & 3) + 8 * (g >> 2) + 4 * h; }

template <int DP, bool COLS>
__global__ __launch_bounds__(kThreadsNce) void k_infonce(
    int64_t B, int d, const float* __restrict__ Own, const float* __restrict__ Str, float inv_tau,
    const float* __restrict__ lse_in, const float* __restrict__ G, const float* __restrict__ pd_in,
    float* __restrict__ lse_out, float* __restrict__ diag, float* __restrict__ pd_out,
    float* __restrict__ Out) {
  constexpr int LD = DP + 1;  // odd row stride: the 32 rows of a ds_read_b32 fall on 32 banks
  constexpr int NR = kTileRows / kWavesNce, NC = (DP + 63) / 64;
  constexpr int NF = DP / 32;
  __shared__ float tile[kTileRows * LD];
  __shared__ float rowsc[2 * kTileRows];  // column pass: lse and G of the streamed rows

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, h = lane >> 5;
  const int64_t own0 = (int64_t)blockIdx.x * kOwnRows + wave * 32;
  const int64_t mine = own0 + li;  // this lane's resident row

  // resident operand: k-step s reads feature 2s + h
  float own[DP / 2];
#pragma unroll
  for (int s = 0; s < DP / 2; ++s) {
    const int f = 2 * s + h;
    own[s] = (mine < B && f < d) ? Own[mine * d + f] : 0.f;
  }

  f32x16 out[NF];
#pragma unroll
  for (int ft = 0; ft < NF; ++ft)
#pragma unroll
    for (int g = 0; g < 16; ++g) out[ft][g] = 0.f;
  float m_run = -INFINITY, sum_run = 0.f, pd_run = 0.f;
  const bool want_out = Out != nullptr;

  const int64_t nt = (B + kTileRows - 1) / kTileRows;
  // staging: wave w takes rows w, w + 4, .. of the tile (a wave-uniform row base), lane = feature
  float stage[NR][NC], stage_sc = 0.f;
  auto fetch = [&](int64_t t) {
    const int64_t r0 = t * kTileRows;
#pragma unroll
    for (int i = 0; i < NR; ++i) {
      const int64_t r = r0 + wave + kWavesNce * i;
      const float* __restrict__ src = Str + r * d;
#pragma unroll
      for (int j = 0; j < NC; ++j) {
        const int f = lane + 64 * j;
        stage[i][j] = (r < B && f < d) ? src[f] : 0.f;
      }
    }
    if (COLS && tid < 2 * kTileRows) {
      const int64_t r = r0 + (tid & 31);
      stage_sc = r < B ? (tid < kTileRows ? lse_in[r] : G[r]) : 0.f;
    }
  };
  // the next tile is fetched ahead where its 32 staging registers fit beside the operands (DP < 256)
  constexpr bool AHEAD = DP < 256;
  if (AHEAD) fetch(0);
  for (int64_t t = 0; t < nt; ++t) {
    __syncthreads();  // the previous tile's readers are done
    if (!AHEAD) fetch(t);
#pragma unroll
    for (int i = 0; i < NR; ++i)
#pragma unroll
      for (int j = 0; j < NC; ++j) {
        const int f = lane + 64 * j;
        if (f < DP) tile[(wave + kWavesNce * i) * LD + f] = stage[i][j];
      }
    if (COLS && tid < 2 * kTileRows) rowsc[tid] = stage_sc;
    __syncthreads();
    if (AHEAD && t + 1 < nt) fetch(t + 1);

    // score tile: acc[streamed row][own row] = sum_f tile[row][f] * own[f], f ascending
    f32x16 acc;
#pragma unroll
    for (int g = 0; g < 16; ++g) acc[g] = 0.f;
#pragma unroll
    for (int s = 0; s < DP / 2; ++s) {
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(tile[li * LD + 2 * s + h], own[s], acc, 0, 0, 0);
      if ((s & 7) == 7) __builtin_amdgcn_sched_barrier(0);  // keeps the LDS reads from piling up in VGPRs
    }

    float w[16];
    if (COLS) {
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        const int r = acc_row(g, h);
        w[g] = rowsc[kTileRows + r] * expf(inv_tau * acc[g] - rowsc[r]);
        if (t * kTileRows + r == mine) w[g] = 0.f;  // the diagonal term is added last, from pd
      }
    } else {
      const int64_t c0 = t * kTileRows;
      float mt = -INFINITY;
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        const int64_t c = c0 + acc_row(g, h);
        float v = inv_tau * acc[g];
        if (c == mine && mine < B) diag[mine] = v;
        v = c < B ? v : -INFINITY;
        w[g] = v;
        mt = fmaxf(mt, v);
      }
      mt = fmaxf(mt, __shfl_xor(mt, 32));  // every tile has a column below B: finite
      const float m_new = fmaxf(m_run, mt);
      const float scale = expf(m_run - m_new);  // 0 on the first tile
      float ps = 0.f, pdt = 0.f;
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        w[g] = expf(w[g] - m_new);
        ps += w[g];
        if (c0 + acc_row(g, h) == mine) {  // the diagonal term is kept apart and added last
          pdt = w[g];
          w[g] = 0.f;
        }
      }
      ps = ps + __shfl_xor(ps, 32);  // a + b == b + a: both halves hold the same bits
      pdt = pdt + __shfl_xor(pdt, 32);  // one half holds it, the other 0
      sum_run = sum_run * scale + ps;
      pd_run = pd_run * scale + pdt;
      if (want_out && __any(m_new != m_run)) {
#pragma unroll
        for (int g = 0; g < 16; ++g) {
          const float sc = __shfl(scale, acc_row(g, h));
#pragma unroll
          for (int ft = 0; ft < NF; ++ft) out[ft][g] *= sc;
        }
      }
      m_run = m_new;
    }

    if (want_out) {
#pragma unroll
      for (int ft = 0; ft < NF; ++ft) {
#pragma unroll
        for (int g = 0; g < 16; ++g)
          out[ft] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[g], tile[acc_row(g, h) * LD + ft * 32 + li],
                                                         out[ft], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }

  // the diagonal's share: P_rr from the running sums (row pass), G_c P_cc from pd (column pass)
  float dshare = 0.f;
  if (COLS) {
    if (mine < B) dshare = G[mine] * pd_in[mine];
  } else {
    dshare = pd_run / sum_run;
    if (h == 0 && mine < B) {
      lse_out[mine] = m_run + logf(sum_run);
      if (pd_out) pd_out[mine] = dshare;
    }
  }
  if (want_out) {
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      const int r = acc_row(g, h);
      const float den = COLS ? 1.f : __shfl(sum_run, r);
      const float ds = __shfl(dshare, r);
      const int64_t row = own0 + r;
#pragma unroll
      for (int ft = 0; ft < NF; ++ft) {
        const int f = ft * 32 + li;
        if (row < B && f < d) {
          const float off = COLS ? out[ft][g] : out[ft][g] / den;
          Out[row * d + f] = off + ds * Str[row * d + f];  // Str's own row: Y_r (rows), A_c (columns)
        }
      }
    }
  }
}

template <bool COLS>
int launch(int64_t B, int d, const float* Own, const float* Str, float inv_tau, const float* lse_in,
           const float* G, const float* pd_in, float* lse_out, float* diag, float* pd_out, float* Out,
           hipStream_t s) {
  const unsigned g = (unsigned)((B + kOwnRows - 1) / kOwnRows);
#define GDD_NCE(DP) \
  k_infonce<DP, COLS><<<g, kThreadsNce, 0, s>>>(B, d, Own, Str, inv_tau, lse_in, G, pd_in, lse_out, diag, \
                                                pd_out, Out)
  if (d <= 32) GDD_NCE(32);
  else if (d <= 64) GDD_NCE(64);
  else if (d <= 128) GDD_NCE(128);
  else if (d <= 192) GDD_NCE(192);
  else GDD_NCE(256);
#undef GDD_NCE
  GDD_LAUNCHED();
  return GDD_OK;
}

int check_nce(const char* who, int64_t B, int d, float inv_tau) {
  GDD_REQUIRE(B >= 0 && B <= INT_MAX, "%s: B outside [0, 2^31)", who);
  GDD_REQUIRE(d >= 1 && d <= kMaxDimNce, "%s: d=%d outside [1, %d]", who, d, kMaxDimNce);
  GDD_REQUIRE(inv_tau > 0.f && inv_tau <= 3.0e38f, "%s: inv_tau must be positive and finite", who);
  return GDD_OK;
}

}  // namespace
}  // namespace gdd

using namespace gdd;

extern "C" size_t gdd_infonce_ws_bytes(int64_t B, int d) {
  (void)B;
  (void)d;
  return 0;  // no column split: nothing to merge
}

extern "C" int gdd_infonce_rows(int64_t B, int d, const float* A, const float* Y, float inv_tau, float* lse,
                                float* diag, float* pd, float* R, void* ws, size_t ws_bytes,
                                gdd_stream_t stream) {
  (void)ws;
  int rc = check_nce("infonce_rows", B, d, inv_tau);
  if (rc) return rc;
  if (ws_bytes < gdd_infonce_ws_bytes(B, d)) return fail(GDD_E_WORKSPACE, "infonce_rows: workspace too small");
  if (B == 0) return GDD_OK;
  GDD_REQUIRE(A && Y && lse && diag, "infonce_rows: null pointer");
  GDD_REQUIRE(!R || pd, "infonce_rows: R without pd (the column pass needs both)");
  return launch<false>(B, d, A, Y, inv_tau, nullptr, nullptr, nullptr, lse, diag, pd, R, to_hip(stream));
}

extern "C" int gdd_infonce_cols(int64_t B, int d, const float* A, const float* Y, float inv_tau,
                                const float* lse, const float* pd, const float* G, float* C, void* ws,
                                size_t ws_bytes, gdd_stream_t stream) {
  (void)ws;
  int rc = check_nce("infonce_cols", B, d, inv_tau);
  if (rc) return rc;
  if (ws_bytes < gdd_infonce_ws_bytes(B, d)) return fail(GDD_E_WORKSPACE, "infonce_cols: workspace too small");
  if (B == 0) return GDD_OK;
  GDD_REQUIRE(A && Y && lse && pd && G && C, "infonce_cols: null pointer");
  return launch<true>(B, d, Y, A, inv_tau, lse, G, pd, nullptr, nullptr, nullptr, C, to_hip(stream));
}
