// The soft-Dice (+ CE) losses of the registry variants: one statistics pass, one gradient
// pass and one host driver (soft_dice_loss), with a finaliser kernel per reference formula
// between the two passes.  HBM-bound; reductions are fixed-order (per-block partials summed
// in order), so every result is deterministic.
//   SwinUNETR / UNETR  LitSwinUNETR_Published._loss (models.py:910-928):
//     L = (1-w) * (1 - mean_{b, c>=sc} 2 I/(P+G+eps)) + w * CE(ignore),
//     I = sum_v m p g, P = sum_v m p, G = sum_v g,  m = [y != ignore],
//     g = onehot(y with ignored -> 0),  p = softmax(logits).
//   R2UNet3D           k_r2u_dice_final below
//   ResUNet++          k_rupp_loss_final below
//   3DUNet wrapper     k_unet3d_loss_final below (per-voxel and per-class CE weights)
//   nnU-Net Dice + CE  k_nnunet_loss_final below (squared-probability denominator)
// The two passes are templates <WT, SQ>: WT reads a voxel weight and a class weight per voxel
// into the CE term, SQ adds the statistic Q_k = sum_v m p_k^2 and a Dice gradient term in p.
// Either one also masks labels outside [0, K) and keeps masked voxels out of G altogether;
// <false, false> is the three older kinds' code, unchanged.
#include "plan_base.h"

#include <math.h>

#include <algorithm>

namespace spff {

constexpr int DL_T = 256, DL_GRID = 256, DL_KMAX = 32;
// Per (block, sample) partial sums of I_k = sum p_k g_k, P_k = sum p_k, G_k =
// sum g_k (g = one-hot of the label, ignored voxels counted at class 0 with p =
// 0, as the oracle's one_hot of the zero-filled labels), the CE sum and the
// valid count.  A wave stages 64 voxels' logit rows in its LDS slice
// (coalesced), each lane turns its row into p in place, then lane l sums
// column k = l % K over the rows r = l / K (mod 64 / K) -- three scalar
// accumulators per lane instead of 3 K-arrays per thread.
template <bool WT, bool SQ>
__global__ __launch_bounds__(DL_T) void k_dice_stats(const float* __restrict__ x,
                                                     const int64_t* __restrict__ lab, int64_t vps,
                                                     int K, int ignore,
                                                     const float* __restrict__ cwt,
                                                     const float* __restrict__ vwt,
                                                     double* __restrict__ part) {
  constexpr bool EXT = WT || SQ;
  constexpr int NS = SQ ? 4 : 3;
  extern __shared__ __attribute__((aligned(16))) float dsm[];
  const int b = blockIdx.y;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  float* sx = dsm + wv * 64 * K;
  int* ys = reinterpret_cast<int*>(dsm + (DL_T / 64) * 64 * K) + wv * 64;
  const int nset = 64 / K, kcol = lane % K, rset = lane / K;
  const bool colane = rset < nset;
  float I = 0.f, P = 0.f, G = 0.f, Q = 0.f;
  double ce = 0.0, usum = 0.0;
  unsigned cnt = 0;
  const int64_t ngroups = (vps + 63) / 64;
  for (int64_t grp = (int64_t)blockIdx.x * (DL_T / 64) + wv; grp < ngroups;
       grp += (int64_t)gridDim.x * (DL_T / 64)) {
    const int64_t v0 = grp * 64;
    const int nv = (int)(vps - v0 < 64 ? vps - v0 : 64);
    wave_copy_rows(sx, x + ((int64_t)b * vps + v0) * K, nv * K, lane);
    wave_lds_sync();
    if (lane < nv) {
      const int64_t y = lab[(int64_t)b * vps + v0 + lane];
      bool valid = y != ignore;
      if constexpr (EXT) valid = valid && y >= 0 && y < K;
      float* xv = sx + lane * K;
      float m = -INFINITY;
      for (int k = 0; k < K; ++k) m = fmaxf(m, xv[k]);
      const int yl = valid ? (int)y : 0;
      const float xy = xv[yl];
      float ssum = 0.f;
      for (int k = 0; k < K; ++k) {  // exp once, kept in the row
        const float e = expf(xv[k] - m);
        xv[k] = e;
        ssum += e;
      }
      if (valid) {
        if constexpr (WT) {  // (w[y] nll) u, the reference's order; sum m u beside it
          const float u = vwt ? vwt[(int64_t)b * vps + v0 + lane] : 1.f;
          const float wy = cwt ? cwt[yl] : 1.f;
          ce += (double)(wy * (m + logf(ssum) - xy) * u);
          usum += (double)u;
        } else {
          ce += (double)(m + logf(ssum) - xy);
          ++cnt;
        }
      }
      const float inv = 1.f / ssum;
      for (int k = 0; k < K; ++k) xv[k] = valid ? xv[k] * inv : 0.f;
      ys[lane] = EXT && !valid ? -1 : yl;  // -1: no column's hit
    }
    wave_lds_sync();
    if (colane) {
      for (int r = rset; r < nv; r += nset) {
        const float p = sx[r * K + kcol];
        const bool hit = ys[r] == kcol;
        I += hit ? p : 0.f;
        P += p;
        G += hit ? 1.f : 0.f;
        if constexpr (SQ) Q += p * p;
      }
    }
    wave_lds_sync();  // the next group overwrites the slice
  }
  __shared__ float rq[NS][DL_T];
  __shared__ double red[DL_T];
  rq[0][threadIdx.x] = colane ? I : 0.f;
  rq[1][threadIdx.x] = colane ? P : 0.f;
  rq[2][threadIdx.x] = colane ? G : 0.f;
  if constexpr (SQ) rq[3][threadIdx.x] = colane ? Q : 0.f;
  const int nq = NS * K + 2;
  double* out = part + ((int64_t)b * gridDim.x + blockIdx.x) * nq;
  for (int q = 0; q < 2; ++q) {
    red[threadIdx.x] = q == 0 ? ce : WT ? usum : (double)cnt;
    __syncthreads();
    for (int st = DL_T / 2; st > 0; st >>= 1) {
      if (threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
      __syncthreads();
    }
    if (threadIdx.x == 0) out[NS * K + q] = red[0];
    __syncthreads();
  }
  if (threadIdx.x < NS * K) {  // (quantity, class): waves, then row sets, in order
    const int w = threadIdx.x / K, k = threadIdx.x % K;
    double t = 0.0;
    for (int ww = 0; ww < DL_T / 64; ++ww)
      for (int j = 0; j < nset; ++j) t += (double)rq[w][ww * 64 + j * K + k];
    out[threadIdx.x] = t;
  }
}

// per (b, q) column sums of the k_dice_stats partials, one workgroup each, fixed tree
__global__ __launch_bounds__(256) void k_dice_sum(const double* __restrict__ part, int nblk,
                                                  int nq, double* __restrict__ tot) {
  const int b = blockIdx.y, q = blockIdx.x;
  double s = 0.0;
  for (int j = threadIdx.x; j < nblk; j += 256) s += part[((int64_t)b * nblk + j) * nq + q];
  __shared__ double red[256];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x == 0) tot[(int64_t)b * nq + q] = red[0];
}

// coef[b][k][2] = (alpha, beta): dL/dp_k = m * (alpha g_k + beta) for k >= sc;
// out4 = [ce, loss, dice_loss, N_valid]; scal[0] = w / N_valid (the CE gradient scale)
__global__ void k_dice_final(const double* __restrict__ tot, int B, int K, int sc, double w,
                             float* __restrict__ coef, float* __restrict__ out4,
                             double* __restrict__ scal) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const int nq = 3 * K + 2;
  double ce = 0.0, N = 0.0, dsum = 0.0;
  const int nc = K - sc;
  for (int b = 0; b < B; ++b) {
    const double* q = tot + (int64_t)b * nq;
    for (int k = 0; k < K; ++k) {
      const double I = q[k], P = q[K + k], G = q[2 * K + k];
      float a = 0.f, be = 0.f;
      if (k >= sc && nc > 0) {
        const double den = P + G + 1e-6;
        dsum += 2.0 * I / den;
        a = (float)(-2.0 * (1.0 - w) / ((double)B * nc * den));
        be = (float)(2.0 * (1.0 - w) * I / ((double)B * nc * den * den));
      }
      coef[((int64_t)b * K + k) * 2 + 0] = a;
      coef[((int64_t)b * K + k) * 2 + 1] = be;
    }
    ce += q[3 * K];
    N += q[3 * K + 1];
  }
  const double dice_loss = nc > 0 ? 1.0 - dsum / ((double)B * nc) : 0.0;
  const double cem = N > 0 ? ce / N : NAN;  // F.cross_entropy: 0/0 -> nan
  out4[0] = (float)cem;
  out4[1] = (float)((1.0 - w) * dice_loss + w * cem);
  out4[2] = (float)dice_loss;
  out4[3] = (float)N;
  scal[0] = N > 0 ? w / N : 0.0;
}

// ------------------------------------ foreground-only soft Dice (R2UNet3D) --
// LitR2UNet3D_Published._dice_only_loss_with_logits, multi-class branch, from the totals of
// k_dice_stats / k_dice_sum (I_k, P_k, G_k per sample; for k >= 1 G_k counts valid voxels
// only, the ignored ones being filed under class 0).  Sample b is kept iff sum_{k>=1} G_k > 0;
// over the n kept samples and the nc = K - 1 foreground classes
//   dice = (2 I + eps) / (P + G + eps),  loss = 1 - mean dice,
// and the coefficients k_dice_grad consumes (dL/dp_k = m (alpha g_k + beta)) are
//   alpha = -2 / (n nc den),  beta = (2 I + eps) / (n nc den^2),  den = P + G + eps,
// zero for k = 0 and for dropped samples.  No CE term: scal[0] = 0.  No sample kept: every
// coefficient is zero, so dlogits = 0, and loss = dice = 0.
// out4 = [dice_mean, loss, kept_samples, N_valid].  One thread: B K <= a few hundred terms,
// summed in (b, k) order.
__global__ void k_r2u_dice_final(const double* __restrict__ tot, int B, int K,
                                 float* __restrict__ coef, float* __restrict__ out4,
                                 double* __restrict__ scal) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const int nq = 3 * K + 2, nc = K - 1;
  const double eps = 1e-6;
  int n = 0;
  double N = 0.0;
  for (int b = 0; b < B; ++b) {
    const double* q = tot + (int64_t)b * nq;
    double fg = 0.0;
    for (int k = 1; k < K; ++k) fg += q[2 * K + k];
    if (fg > 0.0) ++n;
    N += q[3 * K + 1];
  }
  double dsum = 0.0;
  for (int b = 0; b < B; ++b) {
    const double* q = tot + (int64_t)b * nq;
    double fg = 0.0;
    for (int k = 1; k < K; ++k) fg += q[2 * K + k];
    const bool kept = fg > 0.0;
    for (int k = 0; k < K; ++k) {
      float a = 0.f, be = 0.f;
      if (kept && k >= 1) {
        const double I = q[k], den = q[K + k] + q[2 * K + k] + eps;
        const double w = 1.0 / ((double)n * nc);
        dsum += (2.0 * I + eps) / den;
        a = (float)(-2.0 * w / den);
        be = (float)((2.0 * I + eps) * w / (den * den));
      }
      coef[((int64_t)b * K + k) * 2 + 0] = a;
      coef[((int64_t)b * K + k) * 2 + 1] = be;
    }
  }
  const double dice = n > 0 ? dsum / ((double)n * nc) : 0.0;
  out4[0] = (float)dice;
  out4[1] = n > 0 ? (float)(1.0 - dice) : 0.f;
  out4[2] = (float)n;
  out4[3] = (float)N;
  scal[0] = 0.0;
}

// ------------------------------ batch-pooled soft Dice + CE (ResUNet++) --
// dice_ce_loss_with_metrics: I_k, P_k, G_k pooled over the whole batch (the per-sample
// totals of k_dice_stats / k_dice_sum added in sample order), classes k >= sc,
//   dice_k = (2 I_k + eps) / (P_k + G_k + eps),  loss = dw (1 - mean_k dice_k) + cw CE.
// k_dice_stats files the ignored voxels under class 0 of G; the reference's one-hot drops
// them, so with the background included (sc = 0) G_0 -= V - N_valid.  The coefficients
// k_dice_grad consumes (dL/dp_k = m (alpha g_k + beta)) are the same for every sample:
//   alpha = -2 dw / (nc den),  beta = dw (2 I + eps) / (nc den^2),  den = P + G + eps;
// scal[0] = cw / N_valid (the CE gradient scale).  out4 = [ce, loss, dice_mean, N_valid].
__global__ void k_rupp_loss_final(const double* __restrict__ tot, int B, int K, int sc, double V,
                                  double cw, double dw, float* __restrict__ coef,
                                  float* __restrict__ out4, double* __restrict__ scal) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const int nq = 3 * K + 2, nc = K - sc;
  const double eps = 1e-6;
  double ce = 0.0, N = 0.0;
  for (int b = 0; b < B; ++b) {
    ce += tot[(int64_t)b * nq + 3 * K];
    N += tot[(int64_t)b * nq + 3 * K + 1];
  }
  double dsum = 0.0;
  for (int k = 0; k < K; ++k) {
    double I = 0.0, P = 0.0, G = 0.0;
    for (int b = 0; b < B; ++b) {
      const double* q = tot + (int64_t)b * nq;
      I += q[k]; P += q[K + k]; G += q[2 * K + k];
    }
    if (k == 0) G -= V - N;
    float a = 0.f, be = 0.f;
    if (k >= sc) {
      const double den = P + G + eps;
      dsum += (2.0 * I + eps) / den;
      a = (float)(-2.0 * dw / ((double)nc * den));
      be = (float)(dw * (2.0 * I + eps) / ((double)nc * den * den));
    }
    for (int b = 0; b < B; ++b) {
      coef[((int64_t)b * K + k) * 2 + 0] = a;
      coef[((int64_t)b * K + k) * 2 + 1] = be;
    }
  }
  const double dice = dsum / (double)nc;
  const double cem = N > 0 ? ce / N : NAN;  // F.cross_entropy: 0/0 -> nan
  out4[0] = (float)cem;
  out4[1] = (float)(dw * (1.0 - dice) + cw * cem);
  out4[2] = (float)dice;
  out4[3] = (float)N;
  scal[0] = N > 0 ? cw / N : 0.0;
}

// ------------------- voxel- and class-weighted CE + per-sample soft Dice (3DUNet wrapper) --
// LitCicek3DUNet_DepthAdapter_Published._weighted_softmax_ce + ._dice_loss, from the totals of
// k_dice_stats<true, false> (the CE slot holds sum m u w[y] nll, the count slot sum m u; masked
// voxels are in no G_k, so G needs no correction):
//   ce = sum m u w[y] nll / max(sum m u, 1),
//   dice_loss = 1 - mean_{b, k >= sc} 2 I / (P + G + eps),  loss = cw ce + dw dice_loss.
// coef[b][k][2] as k_dice_final with (1 - w) -> dw; scal[0] = cw / max(sum m u, 1), which the
// gradient pass scales by the voxel's u w[y].  out4 = [ce, loss, dice_loss, sum m u].
__global__ void k_unet3d_loss_final(const double* __restrict__ tot, int B, int K, int sc,
                                    double cw, double dw, float* __restrict__ coef,
                                    float* __restrict__ out4, double* __restrict__ scal) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const int nq = 3 * K + 2, nc = K - sc;
  double ce = 0.0, U = 0.0, dsum = 0.0;
  for (int b = 0; b < B; ++b) {
    const double* q = tot + (int64_t)b * nq;
    for (int k = 0; k < K; ++k) {
      const double I = q[k], P = q[K + k], G = q[2 * K + k];
      float a = 0.f, be = 0.f;
      if (k >= sc) {
        const double den = P + G + 1e-6;
        dsum += 2.0 * I / den;
        a = (float)(-2.0 * dw / ((double)B * nc * den));
        be = (float)(2.0 * dw * I / ((double)B * nc * den * den));
      }
      coef[((int64_t)b * K + k) * 2 + 0] = a;
      coef[((int64_t)b * K + k) * 2 + 1] = be;
    }
    ce += q[3 * K];
    U += q[3 * K + 1];
  }
  const double den = U > 1.0 ? U : 1.0;  // clamp_min(1)
  const double dice_loss = 1.0 - dsum / ((double)B * nc);
  const double cem = ce / den;
  out4[0] = (float)cem;
  out4[1] = (float)(cw * cem + dw * dice_loss);
  out4[2] = (float)dice_loss;
  out4[3] = (float)U;
  scal[0] = cw / den;
}

// ------------------------------------ nnU-Net soft Dice + CE (models.dice_ce_loss) --
// soft_dice_loss_from_logits + F.cross_entropy, from the totals of k_dice_stats<false, true>
// (I_k, P_k, G_k, Q_k = sum m p_k^2 per sample; nq = 4 K + 2), pooled over the batch:
//   dice_k = (2 I_k + eps) / (Q_k + G_k + eps), eps = 1e-5, k >= sc,
//   loss = cw CE + dw (1 - mean_k dice_k).
// coef[b][k][3] = (alpha, 0, gamma), the same for every sample: dL/dp_k = m (alpha g_k +
// gamma p_k), alpha = -2 dw / (nc den), gamma = 2 dw (2 I + eps) / (nc den^2).
// scal[0] = cw / N_valid.  out4 = [ce, loss, dice_mean, N_valid].
__global__ void k_nnunet_loss_final(const double* __restrict__ tot, int B, int K, int sc,
                                    double cw, double dw, float* __restrict__ coef,
                                    float* __restrict__ out4, double* __restrict__ scal) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const int nq = 4 * K + 2, nc = K - sc;
  const double eps = 1e-5;
  double ce = 0.0, N = 0.0;
  for (int b = 0; b < B; ++b) {
    ce += tot[(int64_t)b * nq + 4 * K];
    N += tot[(int64_t)b * nq + 4 * K + 1];
  }
  double dsum = 0.0;
  for (int k = 0; k < K; ++k) {
    double I = 0.0, G = 0.0, Q = 0.0;
    for (int b = 0; b < B; ++b) {
      const double* q = tot + (int64_t)b * nq;
      I += q[k]; G += q[2 * K + k]; Q += q[3 * K + k];
    }
    float a = 0.f, ga = 0.f;
    if (k >= sc) {
      const double den = Q + G + eps;
      dsum += (2.0 * I + eps) / den;
      a = (float)(-2.0 * dw / ((double)nc * den));
      ga = (float)(2.0 * dw * (2.0 * I + eps) / ((double)nc * den * den));
    }
    for (int b = 0; b < B; ++b) {
      float* c = coef + ((int64_t)b * K + k) * 3;
      c[0] = a; c[1] = 0.f; c[2] = ga;
    }
  }
  const double dice = dsum / (double)nc;
  const double cem = N > 0 ? ce / N : NAN;  // F.cross_entropy: 0/0 -> nan
  out4[0] = (float)cem;
  out4[1] = (float)(cw * cem + dw * (1.0 - dice));
  out4[2] = (float)dice;
  out4[3] = (float)N;
  scal[0] = N > 0 ? cw / N : 0.0;
}

// dlogits = p (G - <p, G>) + c (p - g), G_k = alpha_k g_k + beta_k (SQ: + gamma_k p_k, three
// coefficients per class), c = scal[0] (WT: times the voxel's weight and its class's); rows
// staged per wave as in k_dice_stats, overwritten in place, stored coalesced
template <bool WT, bool SQ>
__global__ __launch_bounds__(DL_T) void k_dice_grad(const float* __restrict__ x,
                                                    const int64_t* __restrict__ lab, int64_t vps,
                                                    int64_t V, int K, int ignore,
                                                    const float* __restrict__ cwt,
                                                    const float* __restrict__ vwt,
                                                    const float* __restrict__ coef,
                                                    const double* __restrict__ scal,
                                                    float* __restrict__ dx) {
  extern __shared__ __attribute__((aligned(16))) float dsm[];
  const float wN = (float)scal[0];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  float* sx = dsm + wv * 64 * K;
  const int64_t ngroups = (V + 63) / 64;
  for (int64_t grp = (int64_t)blockIdx.x * (DL_T / 64) + wv; grp < ngroups;
       grp += (int64_t)gridDim.x * (DL_T / 64)) {
    const int64_t v0 = grp * 64;
    const int nv = (int)(V - v0 < 64 ? V - v0 : 64);
    wave_copy_rows(sx, x + v0 * K, nv * K, lane);
    wave_lds_sync();
    if (lane < nv) {
      const int64_t v = v0 + lane;
      const int64_t y = lab[v];
      float* xv = sx + lane * K;  // logits in, dlogits out (in place)
      bool masked = y == ignore;
      if constexpr (WT || SQ) masked = masked || y < 0 || y >= K;
      if (masked) {
        for (int k = 0; k < K; ++k) xv[k] = 0.f;
      } else {
        const int yi = (int)y;
        float m = -INFINITY;
        for (int k = 0; k < K; ++k) m = fmaxf(m, xv[k]);
        float ssum = 0.f;
        for (int k = 0; k < K; ++k) {  // exp once, kept in the row
          const float e = expf(xv[k] - m);
          xv[k] = e;
          ssum += e;
        }
        const float inv = 1.f / ssum;
        float cv = wN;
        if constexpr (WT) cv *= (vwt ? vwt[v] : 1.f) * (cwt ? cwt[yi] : 1.f);
        float pg = 0.f;
        if constexpr (SQ) {
          const float* cf = coef + (int64_t)(v / vps) * K * 3;
          for (int k = 0; k < K; ++k) {
            const float pk = xv[k] * inv;
            pg += pk * (cf[3 * k] * (k == yi ? 1.f : 0.f) + cf[3 * k + 1] + cf[3 * k + 2] * pk);
          }
          for (int k = 0; k < K; ++k) {
            const float pk = xv[k] * inv;
            const float Gk = cf[3 * k] * (k == yi ? 1.f : 0.f) + cf[3 * k + 1] + cf[3 * k + 2] * pk;
            xv[k] = pk * (Gk - pg) + cv * (pk - (k == yi ? 1.f : 0.f));
          }
        } else {
          const float2* cf = reinterpret_cast<const float2*>(coef) + (int64_t)(v / vps) * K;
          for (int k = 0; k < K; ++k) {
            const float2 c = cf[k];
            pg += xv[k] * inv * (c.x * (k == yi ? 1.f : 0.f) + c.y);
          }
          for (int k = 0; k < K; ++k) {
            const float2 c = cf[k];
            const float pk = xv[k] * inv;
            const float Gk = c.x * (k == yi ? 1.f : 0.f) + c.y;
            xv[k] = pk * (Gk - pg) + cv * (pk - (k == yi ? 1.f : 0.f));
          }
        }
      }
    }
    wave_lds_sync();
    wave_copy_rows(dx + v0 * K, sx, nv * K, lane);
    wave_lds_sync();  // the next group overwrites the slice
  }
}

// statistics per class (I, P, G[, Q]) and coefficients per class of a kind
static int dice_nstat(DiceKind kind) { return kind == DICE_NNUNET ? 4 : 3; }
static int dice_ncoef(DiceKind kind) { return kind == DICE_NNUNET ? 3 : 2; }

// ws: [B DL_GRID nq] partials, [B nq] totals, 8 scalars (doubles), then coef [B][K][ncoef];
// nq = 3 K + 2 and ncoef = 2 but for DICE_NNUNET (4 K + 2, 3)
size_t dice_ce_ws_bytes(int B, int K, DiceKind kind) {
  return ((size_t)B * (DL_GRID + 1) * (dice_nstat(kind) * K + 2) + 8) * sizeof(double) +
         (size_t)B * K * dice_ncoef(kind) * sizeof(float) + 64;
}

hipError_t soft_dice_loss(const DiceFinal& f, const float* logits, const int64_t* labels, int B,
                          int64_t vps, int K, int use_ignore, int ignore, float* out4,
                          float* dlogits, void* ws, hipStream_t s) {
  if (K < (f.kind == DICE_SWIN ? 1 : 2) || K > DL_KMAX || B < 1 || vps < 1)
    return hipErrorInvalidValue;
  // no mask: a label value no voxel carries (labels are class indices, >= 0)
  const int ign = use_ignore ? ignore : -1;
  const int nq = dice_nstat(f.kind) * K + 2;
  const int64_t V = (int64_t)B * vps;
  double* part = static_cast<double*>(ws);
  double* tot = part + (size_t)B * DL_GRID * nq;
  double* scal = tot + (size_t)B * nq;
  float* coef = reinterpret_cast<float*>(scal + 8);
  const size_t lds = (size_t)(DL_T / 64) * 64 * (K + 1) * sizeof(float);
  hipError_t e;
  const auto stats = f.kind == DICE_UNET3D   ? k_dice_stats<true, false>
                     : f.kind == DICE_NNUNET ? k_dice_stats<false, true>
                                             : k_dice_stats<false, false>;
  const auto grad = f.kind == DICE_UNET3D   ? k_dice_grad<true, false>
                    : f.kind == DICE_NNUNET ? k_dice_grad<false, true>
                                            : k_dice_grad<false, false>;
  hipLaunchKernelGGL(stats, dim3(DL_GRID, B), dim3(DL_T), lds, s, logits, labels, vps, K, ign,
                     f.class_w, f.voxel_w, part);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(k_dice_sum, dim3(nq, B), dim3(256), 0, s, part, DL_GRID, nq, tot);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  switch (f.kind) {
    case DICE_SWIN:
      hipLaunchKernelGGL(k_dice_final, dim3(1), dim3(64), 0, s, tot, B, K, f.sc, f.cw, coef, out4,
                         scal);
      break;
    case DICE_R2U:
      hipLaunchKernelGGL(k_r2u_dice_final, dim3(1), dim3(64), 0, s, tot, B, K, coef, out4, scal);
      break;
    case DICE_RUPP:
      hipLaunchKernelGGL(k_rupp_loss_final, dim3(1), dim3(64), 0, s, tot, B, K, f.sc, (double)V,
                         f.cw, f.dw, coef, out4, scal);
      break;
    case DICE_UNET3D:
      hipLaunchKernelGGL(k_unet3d_loss_final, dim3(1), dim3(64), 0, s, tot, B, K, f.sc, f.cw, f.dw,
                         coef, out4, scal);
      break;
    case DICE_NNUNET:
      hipLaunchKernelGGL(k_nnunet_loss_final, dim3(1), dim3(64), 0, s, tot, B, K, f.sc, f.cw, f.dw,
                         coef, out4, scal);
      break;
  }
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(grad, dim3((unsigned)std::min<int64_t>((V + DL_T - 1) / DL_T, 2048)),
                     dim3(DL_T), lds, s, logits, labels, vps, V, K, ign, f.class_w, f.voxel_w, coef,
                     scal, dlogits);
  return hipGetLastError();
}

// The C entry points of the two kinds that belong to no plan.
static int loss_args(const void* logits, const void* labels, int B, int64_t vps, int K,
                     const void* out4, const void* dlogits, const void* ws) {
  if (K < 2 || K > DL_KMAX) return plan_fail(SPFF_EINVAL, "num_classes must be 2..32");
  if (B < 1 || vps < 1) return plan_fail(SPFF_EINVAL, "invalid batch / vox_per_sample");
  if (!logits || !labels || !out4 || !dlogits || !ws) return plan_fail(SPFF_EINVAL, "null argument");
  return SPFF_OK;
}

}  // namespace spff

using namespace spff;

extern "C" {

size_t spff_unet3d_loss_ws_bytes(int batch, int num_classes) {
  return dice_ce_ws_bytes(batch, num_classes, DICE_UNET3D);
}

int spff_unet3d_loss(const float* logits, const int64_t* labels, int batch, int64_t vox_per_sample,
                     int num_classes, int use_ignore, int ignore_index,
                     const float* class_weights, const float* voxel_weights, int include_bg,
                     double ce_weight, double dice_weight, float* out4, float* dlogits, void* ws,
                     void* stream) {
  PLAN_CK(loss_args(logits, labels, batch, vox_per_sample, num_classes, out4, dlogits, ws));
  PLAN_HIPCK(soft_dice_loss({DICE_UNET3D, include_bg ? 0 : 1, ce_weight, dice_weight, class_weights,
                             voxel_weights},
                            logits, labels, batch, vox_per_sample, num_classes, use_ignore,
                            ignore_index, out4, dlogits, ws, static_cast<hipStream_t>(stream)));
  return SPFF_OK;
}

size_t spff_nnunet_loss_ws_bytes(int batch, int num_classes) {
  return dice_ce_ws_bytes(batch, num_classes, DICE_NNUNET);
}

int spff_nnunet_loss(const float* logits, const int64_t* labels, int batch, int64_t vox_per_sample,
                     int num_classes, int use_ignore, int ignore_index, int include_bg,
                     double ce_weight, double dice_weight, float* out4, float* dlogits, void* ws,
                     void* stream) {
  PLAN_CK(loss_args(logits, labels, batch, vox_per_sample, num_classes, out4, dlogits, ws));
  PLAN_HIPCK(soft_dice_loss({DICE_NNUNET, include_bg ? 0 : 1, ce_weight, dice_weight}, logits,
                            labels, batch, vox_per_sample, num_classes, use_ignore, ignore_index,
                            out4, dlogits, ws, static_cast<hipStream_t>(stream)));
  return SPFF_OK;
}

}  // extern "C"
