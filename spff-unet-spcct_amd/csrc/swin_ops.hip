// Row-wise and elementwise kernels of the SwinUNETR variant (swin.hip): layer
// norm (Swin blocks, patch merging, proj_out), the legacy PatchMerging gather /
// scatter and the UnetResBlock residual + LeakyReLU (the loss: soft_dice.hip).
// Semantics: oracle/swin_oracle.py (MONAI 1.5.2, parity unpinned).  All
// HBM-bound; reductions are fixed-order (wave shuffles, then per-block partials
// summed in order) so every result is deterministic.
#include "spff_internal.h"
#include "swin_internal.h"

#include <math.h>

namespace spff {

namespace {
inline int cdiv(int a, int b) { return (a + b - 1) / b; }
inline int64_t cdiv64(int64_t a, int64_t b) { return (a + b - 1) / b; }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// legacy PatchMerging slice offsets (d, h, w) of cat slot q (MONAI's x0..x7)
__device__ __forceinline__ void merge_off(int q, int& od, int& oh, int& ow) {
  // (0,0,0),(1,0,0),(0,1,0),(0,0,1),(1,0,1),(0,1,0),(0,0,1),(1,1,1)
  constexpr int tab = (0 << 0) | (4 << 3) | (2 << 6) | (1 << 9) | (5 << 12) | (2 << 15) |
                      (1 << 18) | (7 << 21);
  const int t = (tab >> (3 * q)) & 7;
  od = t >> 2; oh = (t >> 1) & 1; ow = t & 1;
}

// row geometry of a layer-norm input: MODE 0 = rows x[m*ldx + c];
// MODE 1 = the merge gather: coarse row m of [B][D/2][H/2][W/2], channel
// c = q*Cf + cf read from the fine grid x[B][D][H][W][Cf]
struct LnSrc {
  const float* x; int ldx, Cf, D, H, W;
};
// split into a per-row base and a per-channel offset so the (64-bit) row
// decomposition runs once per row, not once per element
template <int MODE>
__device__ __forceinline__ int64_t ln_base(const LnSrc& s, int64_t m) {
  if (MODE == 0) return m * s.ldx;
  const int Wl = s.W >> 1, Hl = s.H >> 1, Dl = s.D >> 1;
  int64_t t = m;
  const int w = (int)(t % Wl); t /= Wl;
  const int h = (int)(t % Hl); t /= Hl;
  const int d = (int)(t % Dl);
  const int64_t b = t / Dl;
  return (((b * s.D + 2 * d) * s.H + 2 * h) * (int64_t)s.W + 2 * w) * s.Cf;
}
template <int MODE>
__device__ __forceinline__ int64_t ln_off(const LnSrc& s, int c) {
  if (MODE == 0) return c;
  const int q = c / s.Cf, cf = c - q * s.Cf;
  int od, oh, ow;
  merge_off(q, od, oh, ow);
  return ((int64_t)(od * s.H + oh) * s.W + ow) * s.Cf + cf;
}
constexpr int LN_NJ = 12;  // channels per lane: C <= 768
}  // namespace

// one wave per row: y = (x - mean) * rstd * g + b  (g, b null: no affine)
template <int MODE>
__global__ __launch_bounds__(256) void k_ln_fwd(LnSrc src, int C, const float* __restrict__ g,
                                                const float* __restrict__ bta, float* __restrict__ y,
                                                int ldy, float* __restrict__ mu,
                                                float* __restrict__ rs, int64_t M) {
  const int lane = threadIdx.x & 63;
  const int64_t m = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= M) return;
  float v[LN_NJ];
  float s = 0.f;
  const float* xr = src.x + ln_base<MODE>(src, m);
#pragma unroll
  for (int j = 0; j < LN_NJ; ++j) {
    const int c = lane + 64 * j;
    v[j] = c < C ? xr[ln_off<MODE>(src, c)] : 0.f;
    s += v[j];
  }
  const float mean = wave_sum(s) / (float)C;
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < LN_NJ; ++j) {
    const int c = lane + 64 * j;
    const float dl = c < C ? v[j] - mean : 0.f;
    q += dl * dl;
  }
  const float rstd = 1.f / sqrtf(wave_sum(q) / (float)C + 1e-5f);
#pragma unroll
  for (int j = 0; j < LN_NJ; ++j) {
    const int c = lane + 64 * j;
    if (c < C) {
      float o = (v[j] - mean) * rstd;
      if (g) o = o * g[c] + bta[c];
      y[m * ldy + c] = o;
    }
  }
  if (lane == 0) {
    mu[m] = mean;
    rs[m] = rstd;
  }
}

// dx = rstd * (dy*g - mean(dy*g) - xhat * mean(dy*g*xhat)) [+ res]; per-block
// partial sums of dy*xhat and dy (dgamma, dbeta) over the block's rows
// rows per block: a multiple of the 4 waves, shrunk (as a function of M only,
// so the partial-sum order stays fixed) until the grid has >= 4096 blocks
inline int ln_rpb(int64_t M) {
  int r = 128;
  while (r > 8 && cdiv64(M, r) < 4096) r >>= 1;
  return r;
}
template <int MODE>
__global__ __launch_bounds__(256) void k_ln_bwd(LnSrc src, int C, const float* __restrict__ g,
                                                const float* __restrict__ mu,
                                                const float* __restrict__ rs,
                                                const float* __restrict__ dy, int lddy,
                                                float* __restrict__ dx, int lddx,
                                                const float* __restrict__ res, int ldres,
                                                float* __restrict__ part, int64_t M,
                                                int rpb) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float pg[LN_NJ], pb[LN_NJ];
#pragma unroll
  for (int j = 0; j < LN_NJ; ++j) pg[j] = pb[j] = 0.f;
  const int64_t r0 = (int64_t)blockIdx.x * rpb;
  int64_t off[LN_NJ];
#pragma unroll
  for (int j = 0; j < LN_NJ; ++j) {
    const int c = lane + 64 * j;
    off[j] = c < C ? ln_off<MODE>(src, c) : 0;
  }
  for (int rr = wave; rr < rpb; rr += 4) {
    const int64_t m = r0 + rr;
    if (m >= M) break;
    const float mean = mu[m], rstd = rs[m];
    const float* xr = src.x + ln_base<MODE>(src, m);
    float xh[LN_NJ], gd[LN_NJ];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < LN_NJ; ++j) {
      const int c = lane + 64 * j;
      xh[j] = 0.f; gd[j] = 0.f;
      if (c < C) {
        const float d = dy[m * lddy + c];
        xh[j] = (xr[off[j]] - mean) * rstd;
        gd[j] = g ? d * g[c] : d;
        pg[j] += d * xh[j];
        pb[j] += d;
      }
      s1 += gd[j];
      s2 += gd[j] * xh[j];
    }
    const float c1 = wave_sum(s1) / (float)C, c2 = wave_sum(s2) / (float)C;
#pragma unroll
    for (int j = 0; j < LN_NJ; ++j) {
      const int c = lane + 64 * j;
      if (c < C) {
        float o = rstd * (gd[j] - c1 - xh[j] * c2);
        if (res) o += res[m * ldres + c];
        dx[m * lddx + c] = o;
      }
    }
  }
  if (!part) return;
  __shared__ float red[4][2][64 * LN_NJ];
#pragma unroll
  for (int j = 0; j < LN_NJ; ++j) {
    red[wave][0][lane + 64 * j] = pg[j];
    red[wave][1][lane + 64 * j] = pb[j];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * C; i += 256) {
    const int qq = i / C, c = i - qq * C;
    const float t = ((red[0][qq][c] + red[1][qq][c]) + red[2][qq][c]) + red[3][qq][c];
    part[((int64_t)blockIdx.x * 2 + qq) * C + c] = t;
  }
}

// Narrow rows (C = 12, 24: the first Swin stages): one THREAD per row, the row in
// registers (float4 loads), no cross-lane reductions; 64 lanes cover 64 rows.
template <int C>
__global__ __launch_bounds__(256) void k_ln_fwd_t(const float* __restrict__ x, int ldx,
                                                  const float* __restrict__ g,
                                                  const float* __restrict__ bta,
                                                  float* __restrict__ y, int ldy,
                                                  float* __restrict__ mu, float* __restrict__ rs,
                                                  int64_t M) {
  const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (m >= M) return;
  float v[C];
#pragma unroll
  for (int c = 0; c < C; c += 4) {
    const float4 t = *reinterpret_cast<const float4*>(x + m * ldx + c);
    v[c] = t.x; v[c + 1] = t.y; v[c + 2] = t.z; v[c + 3] = t.w;
  }
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) s += v[c];
  const float mean = s / (float)C;
  float q = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) q += (v[c] - mean) * (v[c] - mean);
  const float rstd = 1.f / sqrtf(q / (float)C + 1e-5f);
#pragma unroll
  for (int c = 0; c < C; c += 4) {
    float o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      o[k] = (v[c + k] - mean) * rstd;
      if (g) o[k] = o[k] * g[c + k] + bta[c + k];
    }
    *reinterpret_cast<float4*>(y + m * ldy + c) = make_float4(o[0], o[1], o[2], o[3]);
  }
  mu[m] = mean;
  rs[m] = rstd;
}

constexpr int LNT_R = 8;  // rows per thread (strided by 256): 2048 rows per block
template <int C>
__global__ __launch_bounds__(256) void k_ln_bwd_t(const float* __restrict__ x, int ldx,
                                                  const float* __restrict__ g,
                                                  const float* __restrict__ mu,
                                                  const float* __restrict__ rs,
                                                  const float* __restrict__ dy, int lddy,
                                                  float* __restrict__ dx, int lddx,
                                                  const float* __restrict__ res, int ldres,
                                                  float* __restrict__ part, int64_t M) {
  float pg[C], pb[C];
#pragma unroll
  for (int c = 0; c < C; ++c) pg[c] = pb[c] = 0.f;
  for (int r = 0; r < LNT_R; ++r) {
    const int64_t m = (int64_t)blockIdx.x * 256 * LNT_R + r * 256 + threadIdx.x;
    if (m >= M) break;
    const float mean = mu[m], rstd = rs[m];
    float xh[C], gd[C];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int c = 0; c < C; c += 4) {
      const float4 tx = *reinterpret_cast<const float4*>(x + m * ldx + c);
      const float4 td = *reinterpret_cast<const float4*>(dy + m * lddy + c);
      const float xv[4] = {tx.x, tx.y, tx.z, tx.w}, dv[4] = {td.x, td.y, td.z, td.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        xh[c + k] = (xv[k] - mean) * rstd;
        gd[c + k] = g ? dv[k] * g[c + k] : dv[k];
        pg[c + k] += dv[k] * xh[c + k];
        pb[c + k] += dv[k];
        s1 += gd[c + k];
        s2 += gd[c + k] * xh[c + k];
      }
    }
    const float c1 = s1 / (float)C, c2 = s2 / (float)C;
#pragma unroll
    for (int c = 0; c < C; c += 4) {
      float o[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] = rstd * (gd[c + k] - c1 - xh[c + k] * c2);
      if (res) {
        const float4 t = *reinterpret_cast<const float4*>(res + m * ldres + c);
        o[0] += t.x; o[1] += t.y; o[2] += t.z; o[3] += t.w;
      }
      *reinterpret_cast<float4*>(dx + m * lddx + c) = make_float4(o[0], o[1], o[2], o[3]);
    }
  }
  if (!part) return;
  __shared__ float red[2 * C][257];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    red[c][threadIdx.x] = pg[c];
    red[C + c][threadIdx.x] = pb[c];
  }
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (threadIdx.x < st)
      for (int i = 0; i < 2 * C; ++i) red[i][threadIdx.x] += red[i][threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x < 2 * C) part[(int64_t)blockIdx.x * 2 * C + threadIdx.x] = red[threadIdx.x][0];
}

// out[i] (+)= sum over k < n of part[k*stride + i] (i < count): one workgroup per
// column, each thread a strided partial sum over k, then a fixed LDS tree --
// deterministic, and parallel over k (n runs to thousands of blocks / windows).
// map = 1: out index of column i = (i % R) * nh + i / R (bias-table transpose);
// map = 2: i = h*2hd + e2 -> C + h*hd + e2 (k part) or 2C + h*hd + e2 - hd (v part).
struct ColMap {
  int mode, R, nh, hd, C;
};
__global__ __launch_bounds__(256) void k_col_reduce(const float* __restrict__ part, int n,
                                                    int64_t stride, float* __restrict__ out,
                                                    int acc, ColMap mp) {
  const int i = blockIdx.x;
  float s = 0.f;
  for (int k = threadIdx.x; k < n; k += 256) s += part[(int64_t)k * stride + i];
  __shared__ float red[256];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x) return;
  int o = i;
  if (mp.mode == 1) {
    o = (i % mp.R) * mp.nh + i / mp.R;
  } else if (mp.mode == 2) {
    const int h = i / (2 * mp.hd), e2 = i % (2 * mp.hd);
    o = e2 < mp.hd ? mp.C + h * mp.hd + e2 : 2 * mp.C + h * mp.hd + (e2 - mp.hd);
  }
  out[o] = acc ? out[o] + red[0] : red[0];
}

hipError_t col_reduce_map(const float* part, int n, int64_t stride, int count, float* out,
                          int acc, int mode, int R, int nh, int hd, int C, hipStream_t s) {
  hipLaunchKernelGGL(k_col_reduce, dim3(count), dim3(256), 0, s, part, n, stride, out, acc,
                     ColMap{mode, R, nh, hd, C});
  return hipGetLastError();
}

hipError_t col_reduce(const float* part, int n, int64_t stride, int count, float* out, int acc,
                      hipStream_t s) {
  return col_reduce_map(part, n, stride, count, out, acc, 0, 1, 1, 1, 0, s);
}

hipError_t ln_fwd(const float* x, int ldx, int C, const float* g, const float* b, float* y,
                  int ldy, float* mu, float* rs, int64_t M, hipStream_t s) {
  if (C > 64 * LN_NJ) return hipErrorInvalidValue;
  const bool vec = ldx % 4 == 0 && ldy % 4 == 0;
  if (vec && (C == 12 || C == 24)) {
    const dim3 gr((unsigned)cdiv64(M, 256));
    if (C == 12)
      hipLaunchKernelGGL(k_ln_fwd_t<12>, gr, dim3(256), 0, s, x, ldx, g, b, y, ldy, mu, rs, M);
    else
      hipLaunchKernelGGL(k_ln_fwd_t<24>, gr, dim3(256), 0, s, x, ldx, g, b, y, ldy, mu, rs, M);
    return hipGetLastError();
  }
  LnSrc src{x, ldx, C, 0, 0, 0};
  hipLaunchKernelGGL(k_ln_fwd<0>, dim3((unsigned)cdiv64(M, 4)), dim3(256), 0, s, src, C, g, b, y,
                     ldy, mu, rs, M);
  return hipGetLastError();
}

hipError_t ln_merge_fwd(const float* xf, int Cf, int B, int D, int H, int W, const float* g,
                        const float* b, float* y, float* mu, float* rs, hipStream_t s) {
  const int C = 8 * Cf;
  if (C > 64 * LN_NJ || D % 2 || H % 2 || W % 2) return hipErrorInvalidValue;
  const int64_t M = (int64_t)B * (D / 2) * (H / 2) * (W / 2);
  LnSrc src{xf, Cf, Cf, D, H, W};
  hipLaunchKernelGGL(k_ln_fwd<1>, dim3((unsigned)cdiv64(M, 4)), dim3(256), 0, s, src, C, g, b, y,
                     C, mu, rs, M);
  return hipGetLastError();
}

size_t ln_bwd_ws_bytes(int64_t M, int C) {
  return (size_t)std::max(cdiv64(M, ln_rpb(M)), cdiv64(M, 256 * LNT_R)) * 2 * C * sizeof(float);
}

// dgb (may be null): [2][C] = dgamma, dbeta (written)
hipError_t ln_bwd(const float* x, int ldx, int C, const float* g, const float* mu,
                  const float* rs, const float* dy, int lddy, float* dx, int lddx,
                  const float* res, int ldres, float* dgb, float* ws, int64_t M, hipStream_t s) {
  if (C > 64 * LN_NJ) return hipErrorInvalidValue;
  const bool vec = ldx % 4 == 0 && lddy % 4 == 0 && lddx % 4 == 0 && (!res || ldres % 4 == 0);
  if (vec && (C == 12 || C == 24)) {
    const int64_t nbt = cdiv64(M, 256 * LNT_R);
    float* pt = dgb ? ws : nullptr;
    if (C == 12)
      hipLaunchKernelGGL(k_ln_bwd_t<12>, dim3((unsigned)nbt), dim3(256), 0, s, x, ldx, g, mu, rs,
                         dy, lddy, dx, lddx, res, ldres, pt, M);
    else
      hipLaunchKernelGGL(k_ln_bwd_t<24>, dim3((unsigned)nbt), dim3(256), 0, s, x, ldx, g, mu, rs,
                         dy, lddy, dx, lddx, res, ldres, pt, M);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !dgb) return e;
    return col_reduce(ws, (int)nbt, 2 * C, 2 * C, dgb, 0, s);
  }
  LnSrc src{x, ldx, C, 0, 0, 0};
  const int rpb = ln_rpb(M);
  const int64_t nb = cdiv64(M, rpb);
  hipLaunchKernelGGL(k_ln_bwd<0>, dim3((unsigned)nb), dim3(256), 0, s, src, C, g, mu, rs, dy, lddy,
                     dx, lddx, res, ldres, dgb ? ws : nullptr, M, rpb);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || !dgb) return e;
  return col_reduce(ws, (int)nb, 2 * C, 2 * C, dgb, 0, s);
}

hipError_t ln_merge_bwd(const float* xf, int Cf, int B, int D, int H, int W, const float* g,
                        const float* mu, const float* rs, const float* dy, float* dcat, float* dgb,
                        float* ws, hipStream_t s) {
  const int C = 8 * Cf;
  const int64_t M = (int64_t)B * (D / 2) * (H / 2) * (W / 2);
  LnSrc src{xf, Cf, Cf, D, H, W};
  const int rpb = ln_rpb(M);
  const int64_t nb = cdiv64(M, rpb);
  hipLaunchKernelGGL(k_ln_bwd<1>, dim3((unsigned)nb), dim3(256), 0, s, src, C, g, mu, rs, dy, C,
                     dcat, C, nullptr, 0, ws, M, rpb);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return col_reduce(ws, (int)nb, 2 * C, 2 * C, dgb, 0, s);
}

// gradient of the merge gather: fine token (b, d, h, w) channel cf receives every
// cat slot q whose offset equals its parity (two for (0,1,0) / (0,0,1), none for
// (1,1,0) / (0,1,1))
__global__ void k_unmerge(const float* __restrict__ dcat, int Cf, int B, int D, int H, int W,
                          float* __restrict__ dxf, int64_t total) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int cf = (int)(i % Cf);
    int64_t t = i / Cf;
    const int w = (int)(t % W); t /= W;
    const int h = (int)(t % H); t /= H;
    const int d = (int)(t % D);
    const int64_t b = t / D;
    const int64_t m = ((b * (D / 2) + d / 2) * (H / 2) + h / 2) * (int64_t)(W / 2) + w / 2;
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      int od, oh, ow;
      merge_off(q, od, oh, ow);
      if (od == (d & 1) && oh == (h & 1) && ow == (w & 1)) s += dcat[m * (8 * Cf) + q * Cf + cf];
    }
    dxf[i] = s;
  }
}

hipError_t unmerge(const float* dcat, int Cf, int B, int D, int H, int W, float* dxf,
                   hipStream_t s) {
  const int64_t total = (int64_t)B * D * H * W * Cf;
  hipLaunchKernelGGL(k_unmerge, dim3((unsigned)std::min<int64_t>(cdiv64(total, 256), 16384)),
                     dim3(256), 0, s, dcat, Cf, B, D, H, W, dxf, total);
  return hipGetLastError();
}

// ----------------------------------------------------- UnetResBlock tail --
// z = y2*al2[b,c] + de2[b,c] + (y3 ? y3*al3 + de3 : r);  out = lrelu(z)
// bwd: dz = dout * slope(z)
template <bool BWD>
__global__ __launch_bounds__(256) void k_res_act(const float* __restrict__ y2,
                                                 const float* __restrict__ al2,
                                                 const float* __restrict__ de2,
                                                 const float* __restrict__ y3,
                                                 const float* __restrict__ al3,
                                                 const float* __restrict__ de3,
                                                 const float* __restrict__ r,
                                                 const float* __restrict__ dout,
                                                 float* __restrict__ out, int C, int64_t vps,
                                                 int64_t n4) {
  const int C4 = C >> 2;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C4) * 4;
    const int64_t v = i / C4;
    const int b = (int)(v / vps);
    const float4 a = *reinterpret_cast<const float4*>(y2 + 4 * i);
    const float4 q = y3 ? *reinterpret_cast<const float4*>(y3 + 4 * i)
                        : *reinterpret_cast<const float4*>(r + 4 * i);
    const float av[4] = {a.x, a.y, a.z, a.w}, qv[4] = {q.x, q.y, q.z, q.w};
    float o[4];
    float4 gd = make_float4(0.f, 0.f, 0.f, 0.f);
    if (BWD) gd = *reinterpret_cast<const float4*>(dout + 4 * i);
    const float gv[4] = {gd.x, gd.y, gd.z, gd.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int bc = b * C + c + j;
      float z = av[j] * al2[bc] + de2[bc];
      z += y3 ? qv[j] * al3[bc] + de3[bc] : qv[j];
      o[j] = BWD ? (z > 0.f ? gv[j] : 0.01f * gv[j]) : (z > 0.f ? z : 0.01f * z);
    }
    *reinterpret_cast<float4*>(out + 4 * i) = make_float4(o[0], o[1], o[2], o[3]);
  }
}

hipError_t res_act(const float* y2, const float* al2, const float* de2, const float* y3,
                   const float* al3, const float* de3, const float* r, const float* dout,
                   float* out, Vol v, int C, hipStream_t s) {
  if (C % 4) return hipErrorInvalidValue;
  const int64_t n4 = nvox(v) * C / 4, vps = (int64_t)v.D * v.H * v.W;
  const dim3 g((unsigned)std::min<int64_t>(cdiv64(n4, 256), 16384));
  if (dout)
    hipLaunchKernelGGL(k_res_act<true>, g, dim3(256), 0, s, y2, al2, de2, y3, al3, de3, r, dout,
                       out, C, vps, n4);
  else
    hipLaunchKernelGGL(k_res_act<false>, g, dim3(256), 0, s, y2, al2, de2, y3, al3, de3, r, dout,
                       out, C, vps, n4);
  return hipGetLastError();
}

}  // namespace spff
