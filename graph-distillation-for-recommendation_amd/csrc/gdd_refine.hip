// gdd_refine.hip — the recommender's refinement epoch (distill_recsys.py:640-733) as a fixed chain
// of plain launches: the LightGCN forward over the condensed graph (:316-350), the BPR loss with its
// regularisers (:353-384) and the KD term (:698-708), the whole backward, and manual_adam_step
// (:402-439). No autograd graph, no index_add_, no floating-point atomic: every sum is a chain or a
// tree in a fixed order, so two runs from the same state give the same bits.
//
// Users and items are one list of N = num_cu + num_ci "nodes" (user r -> r, item c -> num_cu + c);
// every per-row kernel is one wave per node over both sides, lanes over the features (d <= 256: up
// to four per lane). With w = softplus(logit) + 1e-8, sq[n] = sqrt(deg[n] + 1e-8) and
// norm_e = w_e / (sq[u_e] * sq[i_e]) (formed on the fly, the same expression everywhere):
//   1 k_edge_w     per edge: w, sigmoid(logit)
//   2 k_degrees    per node: deg as a lane-strided sum + xor tree (items through perm), sq, row |w|^2
//   3 k_spmm x L   forward: lay[l][n] = sum_e norm_e * lay[l-1][other(e)] (fma chain in row order);
//                  layer 0 = emb + delta is formed while it is read; the layer sum becomes the mean
//   4 k_triplets   16 lanes per triplet: scores, loss term, coef = sigmoid(s_neg - s_pos) / B
//   5 k_seed       per node: d loss / d mean table from the triplets grouped by row, + KD, / (L+1)
//   6 k_spmm x L   backward: A[l-1][n] = seed[n] + sum_e norm_e * A[l][other(e)]
//   7 k_edge_dn    per edge: d loss / d norm_e, one fma chain over the layers and features
//   8 k_degrad     per node: d loss / d deg
//   9 k_final      per parameter element: the chain through norm, w and softplus, the regulariser
//                  gradients, then Adam (or the gradients stored); one more block folds the loss
// Row ids read from the triplets, their groups and the graph are range-checked before they index
// anything: a bad one is skipped and sets *bad (the gdd_edge_dots convention).
#include <climits>
#include <cmath>
#include <vector>

#include "gdd_common.hpp"

namespace gdd {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxDim = 256;  // gdd.rankformer.MAX_DIM
constexpr int kFpl = kMaxDim / 64;  // features per lane
constexpr int kGather = 16;  // k_spmm: row entries whose gathers are issued together
constexpr int kTripLanes = 16;
constexpr int kTripPerBlock = kThreads / kTripLanes;

unsigned grid1(int64_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

struct Shape {
  int nu, ni, N, d, L, B;
  int64_t E;
  const int32_t *rowptr, *col, *cu, *rowptr_t, *col_t, *perm;
};
struct Params {
  float *ue, *ie, *ud, *id, *logit;
};
struct Batch {  // one epoch's record (gdd_bpr_group)
  const int32_t *u, *pos, *neg, *uptr, *uidx, *iptr, *ient;
};
struct Ws {
  float *w, *sig, *dn;  // [E]
  float *sq, *hd;       // [N]
  float *lay, *A;       // [(L+1) N d]; A[L] is the seed
  float* sum;           // [N d] layer sum, then the mean tables
  float* coef;          // [B]
  double *tpart, *rpart, *wpart;  // loss partials: triplet blocks, nodes, user rows
  int32_t* bad;
};
struct AdamC {
  float lr, b1, b2, a1, a2, bc1, bc2, eps;
};
struct Scal {  // host-computed factors
  float inv_b, reg, reg2_b, dreg, dreg2, wreg2, kd_u, kd_i, kdg_u, kdg_i, inv_l1;
  double wreg;
};

template <class T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ __forceinline__ void flag(int32_t* bad, int bit) {
  if (bad) atomicOr(bad, bit);
}

// a CSR row's entry range, checked against [0, cap]
__device__ __forceinline__ bool row_range(const int32_t* __restrict__ rp, int r, int64_t cap, int& beg,
                                          int& end, int32_t* bad) {
  beg = rp[r];
  end = rp[r + 1];
  if (beg < 0 || end < beg || end > cap) {
    flag(bad, 2);
    beg = end = 0;
    return false;
  }
  return true;
}

// entry p of node n's row: the B-order edge id, the user and the item; false if an id is out of range
__device__ __forceinline__ bool edge_of(const Shape& g, bool user, int r, int p, int& eb, int& ur, int& ic,
                                        int32_t* bad) {
  if (user) {
    eb = p;
    ur = r;
    ic = g.col[p];
  } else {
    eb = g.perm[p];
    ur = g.col_t[p];
    ic = r;
  }
  if (eb < 0 || eb >= g.E || ur < 0 || ur >= g.nu || ic < 0 || ic >= g.ni) {
    flag(bad, 2);
    return false;
  }
  return true;
}

__device__ __forceinline__ float edge_norm(float w, float squ, float sqi) { return w / (squ * sqi); }

// layer 0 of node n, feature f: emb + delta (distill_recsys.py:324-325)
__device__ __forceinline__ float layer0(const Shape& g, const Params& p, int n, int f) {
  if (n < g.nu) return p.ue[(int64_t)n * g.d + f] + p.ud[(int64_t)n * g.d + f];
  const int64_t o = (int64_t)(n - g.nu) * g.d + f;
  return p.ie[o] + p.id[o];
}

__device__ __forceinline__ float softplus_f(float x) { return x > 20.f ? x : log1pf(expf(x)); }
__device__ __forceinline__ float sigmoid_f(float x) { return 1.f / (1.f + expf(-x)); }

__global__ __launch_bounds__(kThreads) void k_edge_w(int64_t E, const float* __restrict__ logit,
                                                     float* __restrict__ w, float* __restrict__ sig) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  const float x = logit[e];
  w[e] = softplus_f(x) + 1e-8f;
  sig[e] = sigmoid_f(x);
}

__global__ __launch_bounds__(kThreads) void k_degrees(Shape g, Ws s) {
  const int n = blockIdx.x * kWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (n >= g.N) return;
  const bool user = n < g.nu;
  const int r = user ? n : n - g.nu;
  int beg, end;
  row_range(user ? g.rowptr : g.rowptr_t, r, g.E, beg, end, s.bad);
  float deg = 0.f;
  double q = 0.0;
  for (int p = beg + lane; p < end; p += 64) {
    int eb, ur, ic;
    if (!edge_of(g, user, r, p, eb, ur, ic, s.bad)) continue;
    const float w = s.w[eb];
    deg += w;
    q += (double)w * (double)w;
  }
  deg = wave_sum(deg);
  q = wave_sum(q);
  if (lane == 0) {
    s.sq[n] = sqrtf(deg + 1e-8f);
    if (user) s.wpart[r] = q;
  }
}

// L == 0: the mean tables are layer 0
__global__ __launch_bounds__(kThreads) void k_layer0(Shape g, Params p, Ws s) {
  const int n = blockIdx.x * kWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (n >= g.N) return;
  for (int f = lane; f < g.d; f += 64) {
    const float x = layer0(g, p, n, f);
    s.lay[(int64_t)n * g.d + f] = x;
    s.sum[(int64_t)n * g.d + f] = x;
  }
}

enum { kFwdFirst = 0, kFwd = 1, kBwd = 2 };
// out[n] = base[n] + sum over n's row of norm_e * X[other end of e]  (one wave per node)
//   kFwdFirst: X = layer 0 formed from the parameters; base = n's own layer 0 (also stored)
//   kFwd:      X = lay[l-1]; base = the layer sum so far; at l == L the sum becomes the mean
//   kBwd:      X = A[l]; base = the seed A[L]; out = A[l-1]
template <int MODE>
__global__ __launch_bounds__(kThreads) void k_spmm(Shape g, Params p, Ws s, int l) {
  const int n = blockIdx.x * kWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (n >= g.N) return;
  const bool user = n < g.nu;
  const int r = user ? n : n - g.nu, d = g.d;
  const int64_t tbl = (int64_t)g.N * d;
  const float* X = MODE == kBwd ? s.A + tbl * l : s.lay + tbl * (l - 1);
  int beg, end;
  row_range(user ? g.rowptr : g.rowptr_t, r, g.E, beg, end, s.bad);
  float acc[kFpl];
#pragma unroll
  for (int k = 0; k < kFpl; ++k) acc[k] = 0.f;
  // 64 entries at a time: each lane resolves one entry (ids, norm), then the wave walks them in row
  // order with the entry broadcast from its lane, so the gathers of successive entries are independent
  // loads behind one fma chain. A bad entry contributes 0 * (the node's own row).
  for (int base = beg; base < end; base += 64) {
    int my_other = n;
    float my_nrm = 0.f;
    if (base + lane < end) {
      int eb, ur, ic;
      if (edge_of(g, user, r, base + lane, eb, ur, ic, s.bad)) {
        my_nrm = edge_norm(s.w[eb], s.sq[ur], s.sq[g.nu + ic]);
        my_other = user ? g.nu + ic : ur;
      }
    }
    const int cnt = end - base < 64 ? end - base : 64;
    // kGather entries' gathers in flight, then their fmas in row order; past the row's end a slot is
    // nrm = x = 0, which leaves the chain's value as it is
    for (int j = 0; j < cnt; j += kGather) {
      float nrm[kGather], x[kGather][kFpl];
#pragma unroll
      for (int q = 0; q < kGather; ++q) {
        const bool live = j + q < cnt;  // wave-uniform
        const int other = live ? __shfl(my_other, j + q) : n;
        nrm[q] = live ? __shfl(my_nrm, j + q) : 0.f;
#pragma unroll
        for (int k = 0; k < kFpl; ++k) {
          const int f = lane + 64 * k;
          x[q][k] = live && f < d ? (MODE == kFwdFirst ? layer0(g, p, other, f) : X[(int64_t)other * d + f]) : 0.f;
        }
      }
#pragma unroll
      for (int q = 0; q < kGather; ++q)
#pragma unroll
        for (int k = 0; k < kFpl; ++k) acc[k] = __builtin_fmaf(nrm[q], x[q][k], acc[k]);
    }
  }
#pragma unroll
  for (int k = 0; k < kFpl; ++k) {
    const int f = lane + 64 * k;
    if (f >= d) continue;
    const int64_t o = (int64_t)n * d + f;
    if (MODE == kBwd) {
      s.A[tbl * (l - 1) + o] = s.A[tbl * g.L + o] + acc[k];
    } else {
      float base;
      if (MODE == kFwdFirst) {
        base = layer0(g, p, n, f);
        s.lay[o] = base;
      } else {
        base = s.sum[o];
      }
      s.lay[tbl * l + o] = acc[k];
      const float t = base + acc[k];
      s.sum[o] = l == g.L ? t / (float)(g.L + 1) : t;
    }
  }
}

// per triplet (16 lanes): pos/neg scores, softplus(s_neg - s_pos) / B + the sampled rows' regulariser,
// coef = sigmoid(s_neg - s_pos) / B; block partial of the loss terms in triplet order
__global__ __launch_bounds__(kThreads) void k_triplets(Shape g, Params p, Batch b, Ws s, Scal c) {
  __shared__ double s_term[kTripPerBlock];
  const int grp = threadIdx.x / kTripLanes, sub = threadIdx.x % kTripLanes;
  const int t = blockIdx.x * kTripPerBlock + grp, d = g.d;
  double term = 0.0;
  if (t < g.B) {
    const int u = b.u[t], ip = b.pos[t], in = b.neg[t];
    if (u < 0 || u >= g.nu || ip < 0 || ip >= g.ni || in < 0 || in >= g.ni) {
      if (sub == 0) {
        flag(s.bad, 1);
        s.coef[t] = 0.f;
      }
    } else {
      const float* zu = s.sum + (int64_t)u * d;
      const float* zp = s.sum + (int64_t)(g.nu + ip) * d;
      const float* zn = s.sum + (int64_t)(g.nu + in) * d;
      const float* eu = p.ue + (int64_t)u * d;
      const float* ep = p.ie + (int64_t)ip * d;
      const float* en = p.ie + (int64_t)in * d;
      float sp = 0.f, sn = 0.f, rg = 0.f;
      for (int f = sub; f < d; f += kTripLanes) {
        const float a = zu[f];
        sp = __builtin_fmaf(a, zp[f], sp);
        sn = __builtin_fmaf(a, zn[f], sn);
        rg = __builtin_fmaf(eu[f], eu[f], rg);
        rg = __builtin_fmaf(ep[f], ep[f], rg);
        rg = __builtin_fmaf(en[f], en[f], rg);
      }
#pragma unroll
      for (int o = kTripLanes / 2; o >= 1; o >>= 1) {
        sp += __shfl_xor(sp, o);
        sn += __shfl_xor(sn, o);
        rg += __shfl_xor(rg, o);
      }
      const float x = sn - sp;
      if (sub == 0) s.coef[t] = sigmoid_f(x) * c.inv_b;
      term = ((double)softplus_f(x) + (double)c.reg * (double)rg) * (double)c.inv_b;
    }
  }
  if (sub == 0) s_term[grp] = term;
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = 0.0;
    for (int i = 0; i < kTripPerBlock; ++i) a += s_term[i];
    s.tpart[blockIdx.x] = a;
  }
}

// per node: the seed of the backward, A[L][n] = (d loss / d mean table)[n] / (L+1), from the triplets
// grouped by row (chain in triplet order) plus the KD gradient; the node's share of the delta
// regulariser and the KD loss goes to rpart[n]
__global__ __launch_bounds__(kThreads) void k_seed(Shape g, Params p, Batch b, const float* __restrict__ tu,
                                                   const float* __restrict__ ti, Ws s, Scal c) {
  const int n = blockIdx.x * kWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (n >= g.N) return;
  const bool user = n < g.nu;
  const int r = user ? n : n - g.nu, d = g.d;
  int beg, end;
  row_range(user ? b.uptr : b.iptr, r, user ? g.B : 2 * (int64_t)g.B, beg, end, s.bad);
  float acc[kFpl];
#pragma unroll
  for (int k = 0; k < kFpl; ++k) acc[k] = 0.f;
  // as k_spmm: each lane resolves one entry of the group (its coefficient and the rows it reads), the
  // wave then walks the entries in order. Users: coef * (z[neg] - z[pos]); items: -+coef * z[user].
  // A bad entry contributes 0 * (the node's own row).
  for (int base = beg; base < end; base += 64) {
    int my_a = n, my_b = n;
    float my_c = 0.f;
    if (base + lane < end) {
      const int ent = user ? b.uidx[base + lane] : b.ient[base + lane];
      const int t = user ? ent : ent >> 1;
      if (ent < 0 || t >= g.B) {
        flag(s.bad, 1);
      } else {
        const int u = b.u[t], ip = b.pos[t], in = b.neg[t];
        if (!(u < 0 || u >= g.nu || ip < 0 || ip >= g.ni || in < 0 || in >= g.ni)) {  // else k_triplets flagged it
          const float cf = s.coef[t];
          my_c = user || (ent & 1) ? cf : -cf;
          my_a = user ? g.nu + in : u;
          my_b = g.nu + ip;
        }
      }
    }
    const int cnt = end - base < 64 ? end - base : 64;
    for (int j = 0; j < cnt; ++j) {
      const float cf = __shfl(my_c, j);
      const float* za = s.sum + (int64_t)__shfl(my_a, j) * d;
      const float* zb = s.sum + (int64_t)__shfl(my_b, j) * d;
#pragma unroll
      for (int k = 0; k < kFpl; ++k) {
        const int f = lane + 64 * k;
        if (f < d) acc[k] = __builtin_fmaf(cf, user ? za[f] - zb[f] : za[f], acc[k]);
      }
    }
  }
  const float* teach = user ? tu : ti;
  const float* delta = user ? p.ud : p.id;
  const float kdg = user ? c.kdg_u : c.kdg_i;
  const double kdl = user ? (double)c.kd_u : (double)c.kd_i;
  const int64_t tbl = (int64_t)g.N * d;
  double part = 0.0;
#pragma unroll
  for (int k = 0; k < kFpl; ++k) {
    const int f = lane + 64 * k;
    if (f >= d) continue;
    const int64_t o = (int64_t)n * d + f;
    float a = acc[k];
    const float dl = delta[(int64_t)r * d + f];
    part += (double)c.dreg * (double)dl * (double)dl;
    if (teach) {
      const float diff = s.sum[o] - teach[(int64_t)r * d + f];
      a = __builtin_fmaf(kdg, diff, a);
      part += kdl * (double)diff * (double)diff;
    }
    s.A[tbl * g.L + o] = a * c.inv_l1;
  }
  part = wave_sum(part);
  if (lane == 0) s.rpart[n] = part;
}

// a = fma chain of x[f] * y[f] onto a, f ascending; d a multiple of 4, x and y 16-byte aligned
__device__ __forceinline__ float dot_chain4(const float* __restrict__ x, const float* __restrict__ y, int d,
                                            float a) {
  const float4* x4 = reinterpret_cast<const float4*>(x);
  const float4* y4 = reinterpret_cast<const float4*>(y);
#pragma unroll 4
  for (int q = 0; q < d / 4; ++q) {
    const float4 u = x4[q], v = y4[q];
    a = __builtin_fmaf(u.x, v.x, a);
    a = __builtin_fmaf(u.y, v.y, a);
    a = __builtin_fmaf(u.z, v.z, a);
    a = __builtin_fmaf(u.w, v.w, a);
  }
  return a;
}

// d loss / d norm_e = sum_l <A[l][u], lay[l-1][i]> + <A[l][i], lay[l-1][u]>: one fma chain, layers then
// features ascending
__global__ __launch_bounds__(kThreads) void k_edge_dn(Shape g, Ws s) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= g.E) return;
  const int ur = g.cu[e], ic = g.col[e], d = g.d;
  if (ur < 0 || ur >= g.nu || ic < 0 || ic >= g.ni) {
    flag(s.bad, 2);
    s.dn[e] = 0.f;
    return;
  }
  const int64_t tbl = (int64_t)g.N * d, ou = (int64_t)ur * d, oi = (int64_t)(g.nu + ic) * d;
  float a = 0.f;
  for (int l = 1; l <= g.L; ++l) {
    const float* Al = s.A + tbl * l;
    const float* Xl = s.lay + tbl * (l - 1);
    if ((d & 3) == 0) {  // rows are 16-byte aligned: the same chain from 16-byte loads
      a = dot_chain4(Al + ou, Xl + oi, d, a);
      a = dot_chain4(Al + oi, Xl + ou, d, a);
    } else {
      for (int f = 0; f < d; ++f) a = __builtin_fmaf(Al[ou + f], Xl[oi + f], a);
      for (int f = 0; f < d; ++f) a = __builtin_fmaf(Al[oi + f], Xl[ou + f], a);
    }
  }
  s.dn[e] = a;
}

// d loss / d deg[n] = -(sum over n's row of dn_e * norm_e) / (2 (deg[n] + 1e-8))
__global__ __launch_bounds__(kThreads) void k_degrad(Shape g, Ws s) {
  const int n = blockIdx.x * kWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (n >= g.N) return;
  const bool user = n < g.nu;
  const int r = user ? n : n - g.nu;
  int beg, end;
  row_range(user ? g.rowptr : g.rowptr_t, r, g.E, beg, end, s.bad);
  float a = 0.f;
  for (int p = beg + lane; p < end; p += 64) {
    int eb, ur, ic;
    if (!edge_of(g, user, r, p, eb, ur, ic, s.bad)) continue;
    a = __builtin_fmaf(s.dn[eb], edge_norm(s.w[eb], s.sq[ur], s.sq[g.nu + ic]), a);
  }
  a = wave_sum(a);
  if (lane == 0) {
    const float q = s.sq[n];
    s.hd[n] = -a / (2.f * (q * q));
  }
}

__device__ __forceinline__ float* p_at(const Params& p, int which) {
  return which == 0 ? p.ue : which == 1 ? p.ie : which == 2 ? p.ud : which == 3 ? p.id : p.logit;
}

// manual_adam_step (distill_recsys.py:402-439) on one element
__device__ __forceinline__ void adam_one(float g, float* p, float* m, float* v, const AdamC& a) {
  const float mn = __builtin_fmaf(g, a.a1, *m * a.b1);
  const float vn = __builtin_fmaf(g * g, a.a2, *v * a.b2);
  *m = mn;
  *v = vn;
  *p = *p + (-a.lr) * ((mn / a.bc1) / (sqrtf(vn / a.bc2) + a.eps));
}

struct Five {
  float* p[5];  // user_emb, item_emb, user_delta, item_delta, edge_logit
};

// the gradient of every parameter element (i < E: edge_logit; then the emb tables of all nodes; then
// the delta tables), stored (ADAM false) or applied; the block after the last folds the loss
template <bool ADAM>
__global__ __launch_bounds__(kThreads) void k_final(Shape g, Params p, Batch b, Ws s, Scal c, Five grad,
                                                    Five mom1, Five mom2, AdamC ad, int n_tpart,
                                                    float* __restrict__ loss_out) {
  __shared__ double s_red[kThreads];
  if (blockIdx.x == gridDim.x - 1) {
    double a = 0.0;
    for (int i = threadIdx.x; i < n_tpart; i += kThreads) a += s.tpart[i];
    for (int i = threadIdx.x; i < g.N; i += kThreads) a += s.rpart[i];
    for (int i = threadIdx.x; i < g.nu; i += kThreads) a += c.wreg * s.wpart[i];
    s_red[threadIdx.x] = a;
    __syncthreads();
    for (int o = kThreads / 2; o >= 1; o >>= 1) {
      if ((int)threadIdx.x < o) s_red[threadIdx.x] += s_red[threadIdx.x + o];
      __syncthreads();
    }
    if (threadIdx.x == 0 && loss_out) *loss_out = (float)s_red[0];
    return;
  }
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t tbl = (int64_t)g.N * g.d;
  if (i >= g.E + 2 * tbl) return;
  int which;
  int64_t off;
  float gr;
  if (i < g.E) {
    which = 4;
    off = i;
    const int ur = g.cu[i], ic = g.col[i];
    if (ur < 0 || ur >= g.nu || ic < 0 || ic >= g.ni) {
      flag(s.bad, 2);
      gr = 0.f;
    } else {
      const float dw = s.dn[i] / (s.sq[ur] * s.sq[g.nu + ic]) + s.hd[ur] + s.hd[g.nu + ic] + c.wreg2 * s.w[i];
      gr = dw * s.sig[i];
    }
  } else {
    const int64_t j = i - g.E;
    const bool is_delta = j >= tbl;
    const int64_t q = is_delta ? j - tbl : j;
    const int n = (int)(q / g.d);
    const bool user = n < g.nu;
    which = (is_delta ? 2 : 0) + (user ? 0 : 1);
    off = user ? q : q - (int64_t)g.nu * g.d;
    const float a0 = s.A[q];
    const float x = p_at(p, which)[off];
    if (is_delta) {
      gr = __builtin_fmaf(c.dreg2, x, a0);
    } else {
      const int r = user ? n : n - g.nu;
      int beg, end;
      row_range(user ? b.uptr : b.iptr, r, user ? g.B : 2 * (int64_t)g.B, beg, end, s.bad);
      gr = __builtin_fmaf(c.reg2_b * (float)(end - beg), x, a0);
    }
  }
  if (ADAM) {
    adam_one(gr, p_at(p, which) + off, mom1.p[which] + off, mom2.p[which] + off, ad);
  } else {
    grad.p[which][off] = gr;
  }
}

// gdd_refine_adam: Adam over caller-supplied gradients
__global__ __launch_bounds__(kThreads) void k_adam(int64_t n, const float* __restrict__ g, float* __restrict__ p,
                                                   float* __restrict__ m, float* __restrict__ v, AdamC ad) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) adam_one(g[i], p + i, m + i, v + i, ad);
}

}  // namespace
}  // namespace gdd

using namespace gdd;

namespace {

int64_t batch_words(int64_t B, int nu, int ni) { return 6 * B + nu + ni + 2; }

Batch batch_at(const int32_t* rec, int64_t B, int nu, int ni) {
  Batch b;
  b.u = rec;
  b.pos = rec + B;
  b.neg = rec + 2 * B;
  b.uptr = rec + 3 * B;
  b.uidx = b.uptr + nu + 1;
  b.iptr = b.uidx + B;
  b.ient = b.iptr + ni + 1;
  return b;
}

int check_problem(const gdd_refine_problem* p, const char* who) {
  GDD_REQUIRE(p, "%s: null problem", who);
  GDD_REQUIRE(p->num_cu > 0 && p->num_ci > 0 && p->E >= 0 && p->E < INT_MAX && p->L >= 0 && p->L <= 64 &&
                  p->B > 0 && p->B < (1 << 30),
              "%s: bad shape", who);
  GDD_REQUIRE(p->d >= 1 && p->d <= kMaxDim, "%s: d=%d outside [1, %d] (use the torch backend)", who, p->d,
              kMaxDim);
  GDD_REQUIRE(((int64_t)p->num_cu + p->num_ci) * p->d * (p->L + 1) < INT_MAX, "%s: tables too large", who);
  GDD_REQUIRE(p->rowptr && p->rowptr_t && p->user_emb && p->item_emb && p->user_delta && p->item_delta &&
                  (p->E == 0 || (p->col && p->cu && p->col_t && p->perm && p->edge_logit)),
              "%s: null pointer", who);
  GDD_REQUIRE((p->t_user == nullptr) == (p->t_item == nullptr), "%s: one teacher table without the other", who);
  return GDD_OK;
}

Ws carve_ws(const gdd_refine_problem* p, Carver& cv) {
  const int64_t N = (int64_t)p->num_cu + p->num_ci, tbl = N * p->d, E = p->E;
  Ws s;
  s.w = cv.take<float>(E);
  s.sig = cv.take<float>(E);
  s.dn = cv.take<float>(E);
  s.sq = cv.take<float>(N);
  s.hd = cv.take<float>(N);
  s.lay = cv.take<float>(tbl * (p->L + 1));
  s.A = cv.take<float>(tbl * (p->L + 1));
  s.sum = cv.take<float>(tbl);
  s.coef = cv.take<float>(p->B);
  s.tpart = cv.take<double>((p->B + kTripPerBlock - 1) / kTripPerBlock);
  s.rpart = cv.take<double>(N);
  s.wpart = cv.take<double>(p->num_cu);
  s.bad = cv.take<int32_t>(1);
  return s;
}

AdamC adam_consts(const gdd_refine_adam* a, int64_t step) {
  AdamC c;
  c.lr = (float)a->lr;
  c.b1 = (float)a->beta1;
  c.b2 = (float)a->beta2;
  c.a1 = (float)(1.0 - a->beta1);
  c.a2 = (float)(1.0 - a->beta2);
  c.bc1 = (float)(1.0 - std::pow(a->beta1, (double)step));
  c.bc2 = (float)(1.0 - std::pow(a->beta2, (double)step));
  c.eps = (float)a->eps;
  return c;
}

// one epoch's chain. adam null: the gradients go to `grads`
int enqueue_epoch(const gdd_refine_problem* p, const Ws& s, const int32_t* rec, const gdd_refine_adam* adam,
                  int64_t step, float* const* grads, float* loss_out, hipStream_t st) {
  Shape g;
  g.nu = p->num_cu;
  g.ni = p->num_ci;
  g.N = g.nu + g.ni;
  g.d = p->d;
  g.L = p->L;
  g.B = (int)p->B;
  g.E = p->E;
  g.rowptr = p->rowptr;
  g.col = p->col;
  g.cu = p->cu;
  g.rowptr_t = p->rowptr_t;
  g.col_t = p->col_t;
  g.perm = p->perm;
  const Params pr{p->user_emb, p->item_emb, p->user_delta, p->item_delta, p->edge_logit};
  const Batch b = batch_at(rec, p->B, g.nu, g.ni);
  const double reg = p->reg_lambda, kd = p->t_user ? (double)p->kd_lambda : 0.0;
  Scal c;
  c.inv_b = (float)(1.0 / (double)p->B);
  c.reg = (float)reg;
  c.reg2_b = (float)(2.0 * reg / (double)p->B);
  c.dreg = (float)(reg * 1e-3 / (double)g.N);
  c.dreg2 = (float)(2.0 * reg * 1e-3 / (double)g.N);
  c.wreg = reg * 1e-6;
  c.wreg2 = (float)(2.0 * reg * 1e-6);
  c.kd_u = (float)(kd / ((double)g.nu * g.d));
  c.kd_i = (float)(kd / ((double)g.ni * g.d));
  c.kdg_u = (float)(2.0 * kd / ((double)g.nu * g.d));
  c.kdg_i = (float)(2.0 * kd / ((double)g.ni * g.d));
  c.inv_l1 = (float)(1.0 / (double)(g.L + 1));
  const unsigned node_grid = (unsigned)((g.N + kWaves - 1) / kWaves);
  const int n_tpart = (g.B + kTripPerBlock - 1) / kTripPerBlock;

  if (g.E > 0) {
    k_edge_w<<<grid1(g.E), kThreads, 0, st>>>(g.E, pr.logit, s.w, s.sig);
    GDD_LAUNCHED();
  }
  k_degrees<<<node_grid, kThreads, 0, st>>>(g, s);
  GDD_LAUNCHED();
  if (g.L == 0) {
    k_layer0<<<node_grid, kThreads, 0, st>>>(g, pr, s);
    GDD_LAUNCHED();
  }
  for (int l = 1; l <= g.L; ++l) {
    if (l == 1) {
      k_spmm<kFwdFirst><<<node_grid, kThreads, 0, st>>>(g, pr, s, l);
    } else {
      k_spmm<kFwd><<<node_grid, kThreads, 0, st>>>(g, pr, s, l);
    }
    GDD_LAUNCHED();
  }
  k_triplets<<<(unsigned)n_tpart, kThreads, 0, st>>>(g, pr, b, s, c);
  GDD_LAUNCHED();
  k_seed<<<node_grid, kThreads, 0, st>>>(g, pr, b, p->t_user, p->t_item, s, c);
  GDD_LAUNCHED();
  for (int l = g.L; l >= 1; --l) {
    k_spmm<kBwd><<<node_grid, kThreads, 0, st>>>(g, pr, s, l);
    GDD_LAUNCHED();
  }
  if (g.E > 0) {
    k_edge_dn<<<grid1(g.E), kThreads, 0, st>>>(g, s);
    GDD_LAUNCHED();
  }
  k_degrad<<<node_grid, kThreads, 0, st>>>(g, s);
  GDD_LAUNCHED();
  const int64_t total = g.E + 2 * (int64_t)g.N * g.d;
  Five gr{}, m1{}, m2{};
  if (adam) {
    for (int i = 0; i < 5; ++i) {
      m1.p[i] = adam->m[i];
      m2.p[i] = adam->v[i];
    }
    k_final<true><<<grid1(total) + 1, kThreads, 0, st>>>(g, pr, b, s, c, gr, m1, m2, adam_consts(adam, step),
                                                        n_tpart, loss_out);
  } else {
    for (int i = 0; i < 5; ++i) gr.p[i] = grads[i];
    k_final<false><<<grid1(total) + 1, kThreads, 0, st>>>(g, pr, b, s, c, gr, m1, m2, AdamC{}, n_tpart, loss_out);
  }
  GDD_LAUNCHED();
  return GDD_OK;
}

int check_adam(const gdd_refine_problem* p, const gdd_refine_adam* a, const char* who) {
  GDD_REQUIRE(a, "%s: null Adam state", who);
  for (int i = 0; i < 5; ++i)
    GDD_REQUIRE((a->m[i] && a->v[i]) || (i == 4 && p->E == 0), "%s: null moment table", who);
  return GDD_OK;
}

}  // namespace

extern "C" int64_t gdd_refine_batch_words(int64_t B, int num_cu, int num_ci) {
  return batch_words(B, num_cu, num_ci);
}

extern "C" size_t gdd_refine_ws_bytes(const gdd_refine_problem* p) {
  if (check_problem(p, "refine_ws_bytes")) return 0;
  Carver cv(nullptr, 0);
  carve_ws(p, cv);
  return align256(cv.off) + 256;
}

extern "C" int gdd_refine_grads(const gdd_refine_problem* p, const int32_t* batch, float* loss_out,
                                float* g_user_emb, float* g_item_emb, float* g_user_delta,
                                float* g_item_delta, float* g_edge_logit, int32_t* bad, void* ws,
                                size_t ws_bytes, gdd_stream_t stream) {
  if (int rc = check_problem(p, "refine_grads")) return rc;
  GDD_REQUIRE(batch && loss_out && g_user_emb && g_item_emb && g_user_delta && g_item_delta && ws &&
                  (p->E == 0 || g_edge_logit),
              "refine_grads: null pointer");
  Carver cv(ws, ws_bytes);
  Ws s = carve_ws(p, cv);
  if (!cv.ok()) return fail(GDD_E_WORKSPACE, "refine_grads: workspace too small");
  hipStream_t st = to_hip(stream);
  GDD_HIP(hipMemsetAsync(s.bad, 0, sizeof(int32_t), st));
  float* grads[5] = {g_user_emb, g_item_emb, g_user_delta, g_item_delta, g_edge_logit};
  if (int rc = enqueue_epoch(p, s, batch, nullptr, 0, grads, loss_out, st)) return rc;
  if (bad) GDD_HIP(hipMemcpyAsync(bad, s.bad, sizeof(int32_t), hipMemcpyDeviceToDevice, st));
  return GDD_OK;
}

extern "C" int gdd_refine_adam_step(const gdd_refine_problem* p, const float* g_user_emb,
                                    const float* g_item_emb, const float* g_user_delta,
                                    const float* g_item_delta, const float* g_edge_logit,
                                    const gdd_refine_adam* adam, int64_t step, gdd_stream_t stream) {
  if (int rc = check_problem(p, "refine_adam_step")) return rc;
  if (int rc = check_adam(p, adam, "refine_adam_step")) return rc;
  GDD_REQUIRE(step >= 1, "refine_adam_step: step must be >= 1");
  GDD_REQUIRE(g_user_emb && g_item_emb && g_user_delta && g_item_delta && (p->E == 0 || g_edge_logit),
              "refine_adam_step: null gradient");
  const AdamC c = adam_consts(adam, step);
  const int64_t nu = (int64_t)p->num_cu * p->d, ni = (int64_t)p->num_ci * p->d;
  const float* g[5] = {g_user_emb, g_item_emb, g_user_delta, g_item_delta, g_edge_logit};
  float* prm[5] = {p->user_emb, p->item_emb, p->user_delta, p->item_delta, p->edge_logit};
  const int64_t n[5] = {nu, ni, nu, ni, p->E};
  for (int i = 0; i < 5; ++i) {
    if (n[i] == 0) continue;
    k_adam<<<grid1(n[i]), kThreads, 0, to_hip(stream)>>>(n[i], g[i], prm[i], adam->m[i], adam->v[i], c);
    GDD_LAUNCHED();
  }
  return GDD_OK;
}

extern "C" int gdd_refine_epochs(const gdd_refine_problem* p, const gdd_refine_adam* adam,
                                 const int32_t* batches, int64_t first_step, int n_epochs, float* losses,
                                 int32_t* bad, void* ws, size_t ws_bytes, gdd_stream_t stream) {
  if (int rc = check_problem(p, "refine_epochs")) return rc;
  if (int rc = check_adam(p, adam, "refine_epochs")) return rc;
  GDD_REQUIRE(first_step >= 1 && n_epochs >= 0, "refine_epochs: bad step range");
  if (n_epochs == 0) return GDD_OK;
  GDD_REQUIRE(batches && losses && ws, "refine_epochs: null pointer");
  Carver cv(ws, ws_bytes);
  Ws s = carve_ws(p, cv);
  if (!cv.ok()) return fail(GDD_E_WORKSPACE, "refine_epochs: workspace too small");
  hipStream_t st = to_hip(stream);
  GDD_HIP(hipMemsetAsync(s.bad, 0, sizeof(int32_t), st));
  const int64_t words = batch_words(p->B, p->num_cu, p->num_ci);
  for (int ep = 0; ep < n_epochs; ++ep)
    if (int rc = enqueue_epoch(p, s, batches + words * ep, adam, first_step + ep, nullptr, losses + ep, st))
      return rc;
  if (bad) GDD_HIP(hipMemcpyAsync(bad, s.bad, sizeof(int32_t), hipMemcpyDeviceToDevice, st));
  return GDD_OK;
}

// Host only. One epoch's record from its triplets: the ids as int32, the triplet indices grouped by
// user and the (triplet, sign) entries 2t + s (s = 0 positive, 1 negative) grouped by item, both by a
// stable counting sort (inside a row: ascending entry, i.e. triplet order).
extern "C" int gdd_bpr_group(int64_t B, int num_cu, int num_ci, const int64_t* u, const int64_t* pos,
                             const int64_t* neg, int32_t* record) {
  GDD_REQUIRE(B > 0 && B < (1 << 30) && num_cu > 0 && num_ci > 0, "bpr_group: bad shape");
  GDD_REQUIRE(u && pos && neg && record, "bpr_group: null pointer");
  for (int64_t t = 0; t < B; ++t)
    GDD_REQUIRE(u[t] >= 0 && u[t] < num_cu && pos[t] >= 0 && pos[t] < num_ci && neg[t] >= 0 && neg[t] < num_ci,
                "bpr_group: triplet %lld has an id out of range", (long long)t);
  int32_t* ru = record;
  int32_t* rp = record + B;
  int32_t* rn = record + 2 * B;
  int32_t* uptr = record + 3 * B;
  int32_t* uidx = uptr + num_cu + 1;
  int32_t* iptr = uidx + B;
  int32_t* ient = iptr + num_ci + 1;
  for (int i = 0; i <= num_cu; ++i) uptr[i] = 0;
  for (int i = 0; i <= num_ci; ++i) iptr[i] = 0;
  for (int64_t t = 0; t < B; ++t) {
    ru[t] = (int32_t)u[t];
    rp[t] = (int32_t)pos[t];
    rn[t] = (int32_t)neg[t];
    ++uptr[u[t] + 1];
    ++iptr[pos[t] + 1];
    ++iptr[neg[t] + 1];
  }
  for (int i = 0; i < num_cu; ++i) uptr[i + 1] += uptr[i];
  for (int i = 0; i < num_ci; ++i) iptr[i + 1] += iptr[i];
  // fill with the row starts as cursors, then shift them back
  for (int64_t t = 0; t < B; ++t) {
    uidx[uptr[ru[t]]++] = (int32_t)t;
    ient[iptr[rp[t]]++] = (int32_t)(2 * t);
    ient[iptr[rn[t]]++] = (int32_t)(2 * t + 1);
  }
  for (int i = num_cu; i > 0; --i) uptr[i] = uptr[i - 1];
  uptr[0] = 0;
  for (int i = num_ci; i > 0; --i) iptr[i] = iptr[i - 1];
  iptr[0] = 0;
  return GDD_OK;
}
