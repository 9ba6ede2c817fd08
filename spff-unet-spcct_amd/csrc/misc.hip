// Layout conversion, MaxPool3d((1,2,2)) forward/backward and small utilities.
// Reference: MaxPool3d(P=(1,2,2)) models.py:661-665 (pool only in H,W: F6).
#include "spff_internal.h"

#include <algorithm>
#include <cstdint>
#include <math.h>

namespace spff {

static inline int cdiv(int a, int b) { return (a + b - 1) / b; }

// x [B][C][D][H][W] (reference layout) -> y [B][D][H][W][ldy], channels C..ldy-1 = 0.
// One thread per voxel; the channel row leaves as 16-byte stores (ldy % 4 == 0: every
// engine input has ldy = 8), the C plane reads are coalesced across the wave.
template <bool V4>
__global__ void k_ncdhw_to_ndhwc(const float* __restrict__ x, float* __restrict__ y, int B,
                                 int64_t S, int C, int ldy) {
  const int64_t V = (int64_t)B * S;
  for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < V;
       v += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = v / S, sp = v % S;
    const float* xi = x + b * C * S + sp;
    float* o = y + v * ldy;
    if constexpr (V4) {
      for (int c = 0; c < ldy; c += 4) {
        float4 q;
        q.x = c < C ? xi[(int64_t)c * S] : 0.f;
        q.y = c + 1 < C ? xi[(int64_t)(c + 1) * S] : 0.f;
        q.z = c + 2 < C ? xi[(int64_t)(c + 2) * S] : 0.f;
        q.w = c + 3 < C ? xi[(int64_t)(c + 3) * S] : 0.f;
        *reinterpret_cast<float4*>(o + c) = q;
      }
    } else {
      for (int c = 0; c < ldy; ++c) o[c] = c < C ? xi[(int64_t)c * S] : 0.f;
    }
  }
}

hipError_t ncdhw_to_ndhwc(const float* x, float* y, Vol vol, int C, int ldy, hipStream_t s) {
  const int64_t S = (int64_t)vol.D * vol.H * vol.W;
  const int64_t V = vol.B * S;
  int grid = (int)std::min<int64_t>((V + 255) / 256, 8192);
  if (ldy % 4 == 0 && reinterpret_cast<uintptr_t>(y) % 16 == 0)
    hipLaunchKernelGGL(k_ncdhw_to_ndhwc<true>, dim3(grid), dim3(256), 0, s, x, y, vol.B, S, C, ldy);
  else
    hipLaunchKernelGGL(k_ncdhw_to_ndhwc<false>, dim3(grid), dim3(256), 0, s, x, y, vol.B, S, C, ldy);
  return hipGetLastError();
}

// ---------------------------------------------------------------- maxpool --
// Tie rule = PyTorch CPU max_pool: scan (dh,dw) in row-major order, replace on
// strictly greater or NaN, so the FIRST max wins.  idx = dh*2 + dw.
__global__ void k_maxpool_fwd(const float* __restrict__ x, float* __restrict__ y,
                              uint8_t* __restrict__ idx, Vol in, int C) {
  const int Ho = in.H / 2, Wo = in.W / 2, C4 = C / 4;
  const int64_t total = (int64_t)in.B * in.D * Ho * Wo * C4;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C4) * 4;
    int64_t t = i / C4;
    const int wo = (int)(t % Wo); t /= Wo;
    const int ho = (int)(t % Ho); t /= Ho;  // t = b*D + d
    const int64_t vin = (t * in.H + 2 * ho) * in.W + 2 * wo;
    float best[4];
    uint8_t bi[4] = {0, 0, 0, 0};
    {
      const float4 v = *reinterpret_cast<const float4*>(x + vin * C + c);
      best[0] = v.x; best[1] = v.y; best[2] = v.z; best[3] = v.w;
    }
#pragma unroll
    for (int k = 1; k < 4; ++k) {
      const int64_t vv = vin + (k >> 1) * in.W + (k & 1);
      const float4 v = *reinterpret_cast<const float4*>(x + vv * C + c);
      const float vs[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (vs[j] > best[j] || isnan(vs[j])) { best[j] = vs[j]; bi[j] = (uint8_t)k; }
    }
    const int64_t vo = i / C4;
    *reinterpret_cast<float4*>(y + vo * C + c) = make_float4(best[0], best[1], best[2], best[3]);
    *reinterpret_cast<uchar4*>(idx + vo * C + c) = make_uchar4(bi[0], bi[1], bi[2], bi[3]);
  }
}

hipError_t maxpool_fwd(const float* x, float* y, uint8_t* idx, Vol in, int C, hipStream_t s) {
  if (C % 4) return hipErrorInvalidValue;
  const int64_t total = (int64_t)in.B * in.D * (in.H / 2) * (in.W / 2) * (C / 4);
  int grid = (int)std::min<int64_t>((total + 255) / 256, 16384);
  hipLaunchKernelGGL(k_maxpool_fwd, dim3(grid), dim3(256), 0, s, x, y, idx, in, C);
  return hipGetLastError();
}

// dx[v_in][c] = dskip[v_in*ld + c] + (argmax hit ? dp[v_out][c] : 0)
__global__ void k_maxpool_bwd_add(const float* __restrict__ dp, const uint8_t* __restrict__ idx,
                                  const float* __restrict__ dskip, int ldskip,
                                  float* __restrict__ dx, Vol in, int C) {
  const int Ho = in.H / 2, Wo = in.W / 2, C4 = C / 4;
  const int64_t total = (int64_t)in.B * in.D * in.H * in.W * C4;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C4) * 4;
    const int64_t v = i / C4;
    int64_t t = v;
    const int w = (int)(t % in.W); t /= in.W;
    const int h = (int)(t % in.H); t /= in.H;
    float o[4] = {0.f, 0.f, 0.f, 0.f};
    if (dskip) {
      const float* p = dskip + v * ldskip + c;
      o[0] = p[0]; o[1] = p[1]; o[2] = p[2]; o[3] = p[3];
    }
    const int ho = h >> 1, wo = w >> 1;
    if (ho < Ho && wo < Wo) {
      const int64_t vo = (t * Ho + ho) * Wo + wo;
      const uint8_t k = (uint8_t)((h & 1) * 2 + (w & 1));
      const uchar4 ix = *reinterpret_cast<const uchar4*>(idx + vo * C + c);
      const float4 g = *reinterpret_cast<const float4*>(dp + vo * C + c);
      if (ix.x == k) o[0] += g.x;
      if (ix.y == k) o[1] += g.y;
      if (ix.z == k) o[2] += g.z;
      if (ix.w == k) o[3] += g.w;
    }
    *reinterpret_cast<float4*>(dx + v * C + c) = make_float4(o[0], o[1], o[2], o[3]);
  }
}

hipError_t maxpool_bwd_add(const float* dp, const uint8_t* idx, const float* dskip, int ldskip,
                           float* dx, Vol in, int C, hipStream_t s) {
  if (C % 4) return hipErrorInvalidValue;
  const int64_t total = (int64_t)in.B * in.D * in.H * in.W * (C / 4);
  int grid = (int)std::min<int64_t>((total + 255) / 256, 16384);
  hipLaunchKernelGGL(k_maxpool_bwd_add, dim3(grid), dim3(256), 0, s, dp, idx, dskip, ldskip, dx,
                     in, C);
  return hipGetLastError();
}

// ------------------------------------------------ _cat trilinear fallback --
// ATen upsample_trilinear3d, align_corners=False, output size given: per axis
// scale = in / out (fp32), src = scale (o + 0.5) - 0.5 clamped at 0, i0 = (int) src,
// i1 = i0 + (i0 < in - 1), l1 = src - i0, l0 = 1 - l1.  Depth in == out makes the
// depth source index exactly d (weights 1, 0), so only (h, w) interpolate.  The
// value is accumulated as ATen's CPU kernel nests it: h outer, w inner.
__device__ __forceinline__ void lin_src(int o, int in, int out, int& i0, int& i1, float& l0,
                                        float& l1) {
  const float scale = (float)in / (float)out;
  float src = scale * ((float)o + 0.5f) - 0.5f;
  src = src < 0.f ? 0.f : src;
  i0 = (int)src;
  if (i0 > in - 1) i0 = in - 1;
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l1 = src - (float)i0;
  l0 = 1.f - l1;
}

__global__ void k_resize_hw_fwd(const float* __restrict__ x, float* __restrict__ y, Vol in,
                                int Ho, int Wo, int C) {
  const int C4 = C / 4;
  const int64_t total = (int64_t)in.B * in.D * Ho * Wo * C4;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C4) * 4;
    int64_t t = i / C4;
    const int wo = (int)(t % Wo); t /= Wo;
    const int ho = (int)(t % Ho); t /= Ho;  // t = b*D + d
    int h0, h1, w0, w1;
    float lh0, lh1, lw0, lw1;
    lin_src(ho, in.H, Ho, h0, h1, lh0, lh1);
    lin_src(wo, in.W, Wo, w0, w1, lw0, lw1);
    const float* r0 = x + ((t * in.H + h0) * in.W) * C + c;
    const float* r1 = x + ((t * in.H + h1) * in.W) * C + c;
    const float4 a = *reinterpret_cast<const float4*>(r0 + (int64_t)w0 * C);
    const float4 b = *reinterpret_cast<const float4*>(r0 + (int64_t)w1 * C);
    const float4 e = *reinterpret_cast<const float4*>(r1 + (int64_t)w0 * C);
    const float4 f = *reinterpret_cast<const float4*>(r1 + (int64_t)w1 * C);
    float4 o;
    o.x = (a.x * lw0 + b.x * lw1) * lh0 + (e.x * lw0 + f.x * lw1) * lh1;
    o.y = (a.y * lw0 + b.y * lw1) * lh0 + (e.y * lw0 + f.y * lw1) * lh1;
    o.z = (a.z * lw0 + b.z * lw1) * lh0 + (e.z * lw0 + f.z * lw1) * lh1;
    o.w = (a.w * lw0 + b.w * lw1) * lh0 + (e.w * lw0 + f.w * lw1) * lh1;
    *reinterpret_cast<float4*>(y + (i / C4) * C + c) = o;
  }
}

// output rows o in [lo, hi] that can read input row i (scale = in / out <= ~1)
__device__ __forceinline__ void lin_range(int i, int in, int out, int& lo, int& hi) {
  const float inv = (float)out / (float)in;
  lo = max(0, (int)floorf(((float)i - 1.f + 0.5f) * inv - 0.5f) - 1);
  hi = min(out - 1, (int)ceilf(((float)i + 1.f + 0.5f) * inv - 0.5f) + 1);
}

// dx[i] = sum over the outputs that read input (h, w) of lambda_h lambda_w dy, gathered
// in (ho, h0-then-h1, wo, w0-then-w1) order -- deterministic, no atomics
__global__ void k_resize_hw_bwd(const float* __restrict__ dy, float* __restrict__ dx, Vol in,
                                int Ho, int Wo, int C) {
  const int C4 = C / 4;
  const int64_t total = (int64_t)in.B * in.D * in.H * in.W * C4;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C4) * 4;
    int64_t t = i / C4;
    const int wi = (int)(t % in.W); t /= in.W;
    const int hi = (int)(t % in.H); t /= in.H;
    int hlo, hhi, wlo, whi;
    lin_range(hi, in.H, Ho, hlo, hhi);
    lin_range(wi, in.W, Wo, wlo, whi);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int ho = hlo; ho <= hhi; ++ho) {
      int h0, h1, w0, w1;
      float lh0, lh1, lw0, lw1;
      lin_src(ho, in.H, Ho, h0, h1, lh0, lh1);
      for (int hs = 0; hs < 2; ++hs) {
        if ((hs ? h1 : h0) != hi) continue;
        const float lh = hs ? lh1 : lh0;
        for (int wo = wlo; wo <= whi; ++wo) {
          lin_src(wo, in.W, Wo, w0, w1, lw0, lw1);
          const float4 g = *reinterpret_cast<const float4*>(
              dy + ((t * Ho + ho) * (int64_t)Wo + wo) * C + c);
          for (int ws = 0; ws < 2; ++ws) {
            if ((ws ? w1 : w0) != wi) continue;
            const float wgt = lh * (ws ? lw1 : lw0);
            acc.x += g.x * wgt; acc.y += g.y * wgt; acc.z += g.z * wgt; acc.w += g.w * wgt;
          }
        }
      }
    }
    *reinterpret_cast<float4*>(dx + (i / C4) * C + c) = acc;
  }
}

hipError_t resize_hw_fwd(const float* x, float* y, Vol in, int Ho, int Wo, int C, hipStream_t s) {
  const int64_t total = (int64_t)in.B * in.D * Ho * Wo * (C / 4);
  const int grid = (int)std::min<int64_t>((total + 255) / 256, 16384);
  hipLaunchKernelGGL(k_resize_hw_fwd, dim3(grid), dim3(256), 0, s, x, y, in, Ho, Wo, C);
  return hipGetLastError();
}

hipError_t resize_hw_bwd(const float* dy, float* dx, Vol in, int Ho, int Wo, int C,
                         hipStream_t s) {
  const int64_t total = (int64_t)in.B * in.D * in.H * in.W * (C / 4);
  const int grid = (int)std::min<int64_t>((total + 255) / 256, 16384);
  hipLaunchKernelGGL(k_resize_hw_bwd, dim3(grid), dim3(256), 0, s, dy, dx, in, Ho, Wo, C);
  return hipGetLastError();
}

// --------------------------------------------------------- maxpool 2x2x2 --
// nn.MaxPool3d(2) (reference Cicek3DUNet pool1..pool4, models.py:728-731):
// scan (dd, dh, dw) in row-major order, replace on strictly greater or NaN, so
// the FIRST max wins (ATen CPU max_pool3d).  idx = (dd*2 + dh)*2 + dw.  Odd
// extents floor like PyTorch (the trailing plane/row/column is never read).
__global__ void k_maxpool3_fwd(const float* __restrict__ x, float* __restrict__ y,
                               uint8_t* __restrict__ idx, Vol in, int C) {
  const int Do = in.D / 2, Ho = in.H / 2, Wo = in.W / 2, C4 = C / 4;
  const int64_t total = (int64_t)in.B * Do * Ho * Wo * C4;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C4) * 4;
    int64_t t = i / C4;
    const int wo = (int)(t % Wo); t /= Wo;
    const int ho = (int)(t % Ho); t /= Ho;
    const int dd = (int)(t % Do);
    const int64_t b = t / Do;
    const int64_t vin = ((b * in.D + 2 * dd) * in.H + 2 * ho) * in.W + 2 * wo;
    float best[4];
    uint8_t bi[4] = {0, 0, 0, 0};
    {
      const float4 v = *reinterpret_cast<const float4*>(x + vin * C + c);
      best[0] = v.x; best[1] = v.y; best[2] = v.z; best[3] = v.w;
    }
#pragma unroll
    for (int k = 1; k < 8; ++k) {
      const int64_t vv = vin + (int64_t)(k >> 2) * in.H * in.W + ((k >> 1) & 1) * in.W + (k & 1);
      const float4 v = *reinterpret_cast<const float4*>(x + vv * C + c);
      const float vs[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (vs[j] > best[j] || isnan(vs[j])) { best[j] = vs[j]; bi[j] = (uint8_t)k; }
    }
    const int64_t vo = i / C4;
    *reinterpret_cast<float4*>(y + vo * C + c) = make_float4(best[0], best[1], best[2], best[3]);
    *reinterpret_cast<uchar4*>(idx + vo * C + c) = make_uchar4(bi[0], bi[1], bi[2], bi[3]);
  }
}

hipError_t maxpool3_fwd(const float* x, float* y, uint8_t* idx, Vol in, int C, hipStream_t s) {
  if (C % 4) return hipErrorInvalidValue;
  const int64_t total = (int64_t)in.B * (in.D / 2) * (in.H / 2) * (in.W / 2) * (C / 4);
  int grid = (int)std::min<int64_t>((total + 255) / 256, 16384);
  hipLaunchKernelGGL(k_maxpool3_fwd, dim3(grid), dim3(256), 0, s, x, y, idx, in, C);
  return hipGetLastError();
}

// dx[v_in][c] = dskip[v_in*ld + c] + (argmax hit ? dp[v_out][c] : 0)
__global__ void k_maxpool3_bwd_add(const float* __restrict__ dp, const uint8_t* __restrict__ idx,
                                   const float* __restrict__ dskip, int ldskip,
                                   float* __restrict__ dx, Vol in, int C) {
  const int Do = in.D / 2, Ho = in.H / 2, Wo = in.W / 2, C4 = C / 4;
  const int64_t total = (int64_t)in.B * in.D * in.H * in.W * C4;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C4) * 4;
    const int64_t v = i / C4;
    int64_t t = v;
    const int w = (int)(t % in.W); t /= in.W;
    const int h = (int)(t % in.H); t /= in.H;
    const int d = (int)(t % in.D);
    const int64_t b = t / in.D;
    float o[4] = {0.f, 0.f, 0.f, 0.f};
    if (dskip) {
      const float* p = dskip + v * ldskip + c;
      o[0] = p[0]; o[1] = p[1]; o[2] = p[2]; o[3] = p[3];
    }
    const int dd = d >> 1, ho = h >> 1, wo = w >> 1;
    if (dd < Do && ho < Ho && wo < Wo) {
      const int64_t vo = ((b * Do + dd) * Ho + ho) * Wo + wo;
      const uint8_t k = (uint8_t)(((d & 1) * 2 + (h & 1)) * 2 + (w & 1));
      const uchar4 ix = *reinterpret_cast<const uchar4*>(idx + vo * C + c);
      const float4 g = *reinterpret_cast<const float4*>(dp + vo * C + c);
      if (ix.x == k) o[0] += g.x;
      if (ix.y == k) o[1] += g.y;
      if (ix.z == k) o[2] += g.z;
      if (ix.w == k) o[3] += g.w;
    }
    *reinterpret_cast<float4*>(dx + v * C + c) = make_float4(o[0], o[1], o[2], o[3]);
  }
}

hipError_t maxpool3_bwd_add(const float* dp, const uint8_t* idx, const float* dskip, int ldskip,
                            float* dx, Vol in, int C, hipStream_t s) {
  if (C % 4) return hipErrorInvalidValue;
  const int64_t total = (int64_t)in.B * in.D * in.H * in.W * (C / 4);
  int grid = (int)std::min<int64_t>((total + 255) / 256, 16384);
  hipLaunchKernelGGL(k_maxpool3_bwd_add, dim3(grid), dim3(256), 0, s, dp, idx, dskip, ldskip, dx,
                     in, C);
  return hipGetLastError();
}

// ------------------------------------------------------- depth resampling --
// F.interpolate(x, size=(Dout, H, W), mode="trilinear", align_corners=False)
// with H, W unchanged (reference _resize_depth_like / _resize_logits_depth_like,
// models.py:153-163): the H/W factors are exactly 1 (source index = output
// index, weights 1 and 0), so it is linear interpolation along D with ATen's
// source index: src = max(0, (Din/Dout)*(d + 0.5) - 0.5) in fp32,
// i0 = floor(src), i1 = min(i0 + 1, Din - 1), w1 = src - i0, w0 = 1 - w1 (lin_src above).

// input: x [B][C][Din][H][W] (reference layout) -> y [B][Dout][H][W][ldy]
// (channel-last, channels C..ldy-1 zero) in one pass
__global__ void k_resize_d_ncdhw_to_ndhwc(const float* __restrict__ x, float* __restrict__ y,
                                          int B, int C, int Din, int Dout, int HW, int ldy) {
  const int64_t V = (int64_t)B * Dout * HW;
  for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < V;
       v += (int64_t)gridDim.x * blockDim.x) {
    const int hw = (int)(v % HW);
    const int64_t t = v / HW;
    const int d = (int)(t % Dout);
    const int64_t b = t / Dout;
    int i0, i1;
    float w0, w1;
    lin_src(d, Din, Dout, i0, i1, w0, w1);
    float* o = y + v * ldy;
    for (int c = 0; c < ldy; ++c) {
      float r = 0.f;
      if (c < C) {
        const float* xc = x + (b * C + c) * (int64_t)Din * HW + hw;
        r = w0 * xc[(int64_t)i0 * HW] + w1 * xc[(int64_t)i1 * HW];
      }
      o[c] = r;
    }
  }
}

hipError_t resize_d_ncdhw_to_ndhwc(const float* x, float* y, int B, int C, int Din, int Dout,
                                   int H, int W, int ldy, hipStream_t s) {
  const int64_t V = (int64_t)B * Dout * H * W;
  int grid = (int)std::min<int64_t>((V + 255) / 256, 8192);
  hipLaunchKernelGGL(k_resize_d_ncdhw_to_ndhwc, dim3(grid), dim3(256), 0, s, x, y, B, C, Din,
                     Dout, H * W, ldy);
  return hipGetLastError();
}

// channel-last rows of K values: y[b][d][hw][:] = w0 x[b][i0][hw][:] + w1 x[b][i1][hw][:]
__global__ void k_resize_d_rows(const float* __restrict__ x, float* __restrict__ y, int B, int K,
                                int Din, int Dout, int HW) {
  const int64_t total = (int64_t)B * Dout * HW * K;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int k = (int)(i % K);
    int64_t t = i / K;
    const int hw = (int)(t % HW);
    t /= HW;
    const int d = (int)(t % Dout);
    const int64_t b = t / Dout;
    int i0, i1;
    float w0, w1;
    lin_src(d, Din, Dout, i0, i1, w0, w1);
    const float* xb = x + b * (int64_t)Din * HW * K + (int64_t)hw * K + k;
    y[i] = w0 * xb[(int64_t)i0 * HW * K] + w1 * xb[(int64_t)i1 * HW * K];
  }
}

// adjoint of k_resize_d_rows (dx[b][i][hw][:] = sum over output depths d that
// read i of their weight * dy[b][d][hw][:]), gathered per input depth in
// increasing d order: deterministic, no atomics
__global__ void k_resize_d_rows_bwd(const float* __restrict__ dy, float* __restrict__ dx, int B,
                                    int K, int Din, int Dout, int HW) {
  const int64_t total = (int64_t)B * Din * HW * K;
  const float inv = (float)Dout / (float)Din;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int k = (int)(i % K);
    int64_t t = i / K;
    const int hw = (int)(t % HW);
    t /= HW;
    const int di = (int)(t % Din);
    const int64_t b = t / Din;
    // output depths whose source lies in (di - 1, di + 1), widened by one
    int dlo = (int)floorf(((float)di - 0.5f) * inv - 0.5f) - 1;
    int dhi = (int)ceilf(((float)di + 1.5f) * inv - 0.5f) + 1;
    dlo = dlo < 0 ? 0 : dlo;
    dhi = dhi > Dout - 1 ? Dout - 1 : dhi;
    if (di == 0) dlo = 0;                 // clamped sources (src < 0) land on 0
    if (di == Din - 1) dhi = Dout - 1;    // i1 clamps to the last input depth
    const float* gb = dy + b * (int64_t)Dout * HW * K + (int64_t)hw * K + k;
    float acc = 0.f;
    for (int d = dlo; d <= dhi; ++d) {
      int i0, i1;
      float w0, w1;
      lin_src(d, Din, Dout, i0, i1, w0, w1);
      const float g = gb[(int64_t)d * HW * K];
      if (i0 == di) acc += w0 * g;
      if (i1 == di) acc += w1 * g;
    }
    dx[i] = acc;
  }
}

hipError_t resize_d_rows(const float* x, float* y, int B, int K, int Din, int Dout, int H, int W,
                         hipStream_t s) {
  const int64_t total = (int64_t)B * Dout * H * W * K;
  int grid = (int)std::min<int64_t>((total + 255) / 256, 16384);
  hipLaunchKernelGGL(k_resize_d_rows, dim3(grid), dim3(256), 0, s, x, y, B, K, Din, Dout, H * W);
  return hipGetLastError();
}
hipError_t resize_d_rows_bwd(const float* dy, float* dx, int B, int K, int Din, int Dout, int H,
                             int W, hipStream_t s) {
  const int64_t total = (int64_t)B * Din * H * W * K;
  int grid = (int)std::min<int64_t>((total + 255) / 256, 16384);
  hipLaunchKernelGGL(k_resize_d_rows_bwd, dim3(grid), dim3(256), 0, s, dy, dx, B, K, Din, Dout,
                     H * W);
  return hipGetLastError();
}

// x *= *scale.  The scale is the upstream gradient of a scalar loss, 1 whenever the loss is
// the last op before backward(): then every workgroup returns after one scalar load (the
// logits-sized pass, 2 x 218 MB at config 2, is skipped) -- a uniform branch on device data,
// no host sync.
__global__ void k_scale(float* x, int64_t n, const float* scale) {
  const float a = *scale;
  if (a == 1.f) return;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    x[i] *= a;
}

hipError_t scale_by_dev(float* x, int64_t n, const float* scale, hipStream_t s) {
  int grid = (int)std::min<int64_t>((n + 255) / 256, 8192);
  hipLaunchKernelGGL(k_scale, dim3(grid), dim3(256), 0, s, x, n, scale);
  return hipGetLastError();
}

// dst[i] += scale * src[i].  The plans' one accumulate pass: a shared parameter's per-step
// gradients in a fixed order (scale 2 for R2UNet3D's doubled IN affine), the sum of two
// gradient branches (scale 1: d + 1 s and fma(1, s, d) round alike).  HBM-bound
// elementwise pass, float4 body + scalar tail.
__global__ __launch_bounds__(256) void k_accumulate(float* __restrict__ dst,
                                                    const float* __restrict__ src, int64_t n,
                                                    float scale, int vec) {
  const int64_t n4 = vec ? n >> 2 : 0;  // vec: both operands 16-byte aligned
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  float4* d4 = reinterpret_cast<float4*>(dst);
  const float4* s4 = reinterpret_cast<const float4*>(src);
  for (int64_t i = i0; i < n4; i += stride) {
    float4 d = d4[i];
    const float4 v = s4[i];
    d.x += scale * v.x; d.y += scale * v.y; d.z += scale * v.z; d.w += scale * v.w;
    d4[i] = d;
  }
  for (int64_t i = 4 * n4 + i0; i < n; i += stride) dst[i] += scale * src[i];
}

hipError_t accumulate(float* dst, const float* src, int64_t n, float scale, hipStream_t s) {
  // (workspace slots are 256-byte aligned and the plans' channel counts are multiples of 4:
  //  the float4 body is the usual path)
  const int vec = !((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src)) & 15);
  const int64_t work = vec ? (n + 3) / 4 : n;
  const unsigned grid = (unsigned)std::min<int64_t>((work + 255) / 256, 4096);
  hipLaunchKernelGGL(k_accumulate, dim3(std::max(grid, 1u)), dim3(256), 0, s, dst, src, n, scale,
                     vec);
  return hipGetLastError();
}

// hipMemsetAsync replacement for the step's stream-ordered zeroing (counters, amax slots,
// accumulators): a kernel node, so that a HIP-graph capture of the step replays it like the
// step's other kernels (scripts/graph_probe3.py: with hipMemsetAsync inside the captured
// step, the first replay matched the eager step and later ones read stale counters and
// amax slots).  bytes and p must be multiples of 4.
template <typename T>
__global__ void k_fill(T* __restrict__ p, int64_t n, T v) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    p[i] = v;
}

hipError_t fill32_async(void* p, size_t bytes, unsigned value, hipStream_t s) {
  if (bytes == 0) return hipSuccess;
  if ((bytes & 3) || (reinterpret_cast<uintptr_t>(p) & 3)) return hipErrorInvalidValue;
  if (!((bytes | reinterpret_cast<uintptr_t>(p)) & 15)) {
    const int64_t n = (int64_t)(bytes / 16);
    const int grid = (int)std::min<int64_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(k_fill<uint4>, dim3(grid), dim3(256), 0, s, static_cast<uint4*>(p), n,
                       make_uint4(value, value, value, value));
  } else {
    const int64_t n = (int64_t)(bytes / 4);
    const int grid = (int)std::min<int64_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(k_fill<unsigned>, dim3(grid), dim3(256), 0, s, static_cast<unsigned*>(p),
                       n, value);
  }
  return hipGetLastError();
}

}  // namespace spff
