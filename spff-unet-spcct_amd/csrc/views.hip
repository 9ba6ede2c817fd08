// The qualitative views of the reference's figures on the device:
// _prediction_views_and_mip (train.py:649-671; the callback's copy, train.py:933-951), the
// input's centre frame and maximum-intensity projection (train.py:616-634) and the five
// panels of VisualizeEveryNEpochsBuffered._render_buffer (train.py:1071-1119; test.py's
// overlays draw the same panels).  The reference copies the logits to the host and runs a
// per-slice numpy softmax there; here the logits are read once where they lie.
//
//   k_pred_views   a wave per 64 consecutive pixels of one sample's H x W plane and one
//                  range of depth slices, a lane per pixel.  A slice's 64 rows are one
//                  contiguous span of 64 K floats: the wave loads it as float4 quads into
//                  registers one slice ahead, hands it through its LDS slice, and every
//                  lane then reads its own row.  Per voxel the reference's fp32 softmax
//                  (max-subtracted expf summed in class order, a true division by
//                  sum + 1e-8f); the K running maxima over depth stay in registers.  The
//                  wave that meets slice D / 2 writes the centre class map and confidence.
//   k_pred_finish  depth split over n > 1 workgroup ranges: every range leaves a slab
//                  [B][H W][K] of partial maxima, the finisher takes their maximum and the
//                  class map of the projection.  A maximum does not depend on the order or
//                  the grouping of its operands, so every split gives the same bits.  The
//                  workspace holds as many slabs as the kernel's own split; a forced larger
//                  split runs in rounds that fold into mip_prob.  Every slab entry is
//                  written before it is read: the workspace needs no clearing.
//   k_input_views / k_image_range, k_overlay_rgb: the input's two grey images with their
//                  value ranges, and the strip of five panels.
// No allocation, no host synchronisation: a captured graph replays every call.
#include "spff_internal.h"
#include <math.h>

namespace spff {

namespace {

constexpr int PV_T = 256;  // threads per workgroup
constexpr int PV_WAVES = PV_T / 64;
constexpr int PV_MAX_K = 32;
typedef float f32x4 __attribute__((ext_vector_type(4)));
// the kernel's own depth split: enough waves to fill the chip, slabs at most a quarter
// of the logits' bytes (each slab entry is written once and read once)
constexpr int64_t PV_TARGET_WAVES = 4096;
constexpr int PV_MIN_SLICES = 8;

struct ViewsGeo {
  int B, D, H, W, K;
  int64_t HW, ngroups;  // pixels per sample, groups of 64 pixels per sample
  int auto_split, slabs;
  size_t slab_floats, bytes;
};

ViewsGeo views_geo(int B, int D, int H, int W, int K) {
  ViewsGeo g;
  g.B = B; g.D = D; g.H = H; g.W = W; g.K = K;
  g.HW = (int64_t)H * W;
  g.ngroups = (g.HW + 63) / 64;
  const int64_t waves = (int64_t)B * g.ngroups;
  int64_t n = (PV_TARGET_WAVES + waves - 1) / waves;
  const int64_t cap = D / PV_MIN_SLICES > 1 ? D / PV_MIN_SLICES : 1;
  if (n > cap) n = cap;
  g.auto_split = (int)n;
  g.slabs = g.auto_split;  // (one slab at least: a forced split needs it)
  g.slab_floats = (size_t)B * (size_t)g.HW * (size_t)K;
  g.bytes = (size_t)g.slabs * g.slab_floats * sizeof(float) + 64;
  return g;
}

// One voxel row of the lane's pixel: the reference's softmax, the running maxima and, at
// the centre slice, the class map and confidence.  KT: the register tile of classes.
template <int KT>
__device__ __forceinline__ void pv_row(const float* __restrict__ xr, int K, float (&mx)[KT],
                                       bool centre, uint8_t* __restrict__ center_pred,
                                       float* __restrict__ alpha_center) {
  float e[KT];
  float m = -INFINITY;
#pragma unroll
  for (int k = 0; k < KT; ++k) {
    e[k] = k < K ? xr[k] : -INFINITY;
    m = fmaxf(m, e[k]);
  }
  float ssum = 0.f;
#pragma unroll
  for (int k = 0; k < KT; ++k) {
    if (k < K) {
      e[k] = expf(e[k] - m);
      ssum += e[k];
    }
  }
  const float den = ssum + 1e-8f;
  float best = -1.f;
  int arg = 0;
#pragma unroll
  for (int k = 0; k < KT; ++k) {
    if (k < K) {
      const float p = e[k] / den;
      mx[k] = fmaxf(mx[k], p);
      if (p > best) {  // strict: the first maximum wins
        best = p;
        arg = k;
      }
    }
  }
  if (centre) {
    *center_pred = (uint8_t)arg;
    *alpha_center = best;
  }
}

// KT: 16 or 32, K <= KT.  Split s of nsplit covers the slices [s D / nsplit,
// (s + 1) D / nsplit).  Wave w = (b, s, group): groups fastest, so neighbouring waves read
// neighbouring spans.  slab == nullptr (nsplit == 1): the maxima go to mip_prob and their
// class map to mip_pred.
template <int KT>
__global__ __launch_bounds__(PV_T) void k_pred_views(const float* __restrict__ x, ViewsGeo g,
                                                     int nsplit, int s0, int scount,
                                                     uint8_t* __restrict__ center_pred,
                                                     float* __restrict__ alpha_center,
                                                     float* __restrict__ mip_prob,
                                                     uint8_t* __restrict__ mip_pred,
                                                     float* __restrict__ slab) {
  extern __shared__ __attribute__((aligned(16))) float vsm[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int K = g.K;
  const int64_t wid = (int64_t)blockIdx.x * PV_WAVES + wv;
  const int64_t per_b = (int64_t)scount * g.ngroups;
  if (wid >= per_b * g.B) return;  // (no workgroup barrier below: waves are independent)
  const int b = (int)(wid / per_b);
  const int64_t r = wid % per_b;
  const int sl = (int)(r / g.ngroups);  // slab index of this round
  const int s = s0 + sl;
  const int64_t p0 = (r % g.ngroups) * 64;
  const int nv = (int)(g.HW - p0 < 64 ? g.HW - p0 : 64);
  const int d0 = (int)((int64_t)s * g.D / nsplit), d1 = (int)((int64_t)(s + 1) * g.D / nsplit);
  const int mid = g.D / 2;
  float* sx = vsm + (size_t)wv * 64 * K;
  const int n = nv * K;
  const int64_t dstride = g.HW * K;
  const float* rows = x + ((int64_t)b * g.D + d0) * dstride + p0 * K;
  const int64_t opix = (int64_t)b * g.HW + p0 + lane;
  const float* xr = sx + lane * K;
  float mx[KT];
#pragma unroll
  for (int k = 0; k < KT; ++k) mx[k] = 0.f;
  // quads when every slice's span starts on 16 bytes and is whole quads
  const bool vec = ((((uintptr_t)rows) | ((uintptr_t)(dstride * sizeof(float)))) & 15) == 0 &&
                   (n & 3) == 0;
  if (vec) {
    constexpr int NQ = KT / 4;  // 64 KT floats = 64 lanes x NQ quads
    const int n4 = n >> 2;
    // (clamped unconditional loads, predicated stores: a conditionally loaded register
    // array goes to scratch)
    int qi[NQ];
    f32x4 q[NQ];
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
      qi[j] = lane + 64 * j < n4 ? lane + 64 * j : n4 - 1;
      q[j] = reinterpret_cast<const f32x4*>(rows)[qi[j]];
    }
    for (int d = d0; d < d1; ++d) {
#pragma unroll
      for (int j = 0; j < NQ; ++j)
        if (lane + 64 * j < n4) reinterpret_cast<f32x4*>(sx)[lane + 64 * j] = q[j];
      // the next slice's loads fly under this slice's arithmetic (the last slice once more)
      if (d + 1 < d1) rows += dstride;
#pragma unroll
      for (int j = 0; j < NQ; ++j) q[j] = reinterpret_cast<const f32x4*>(rows)[qi[j]];
      wave_lds_sync();
      if (lane < nv) pv_row<KT>(xr, K, mx, d == mid, center_pred + opix, alpha_center + opix);
      wave_lds_sync();  // the next slice overwrites the wave's LDS slice
    }
  } else {
    for (int d = d0; d < d1; ++d) {
      for (int i = lane; i < n; i += 64) sx[i] = rows[i];
      wave_lds_sync();
      if (lane < nv) pv_row<KT>(xr, K, mx, d == mid, center_pred + opix, alpha_center + opix);
      wave_lds_sync();
      rows += dstride;
    }
  }
  // the maxima leave through the LDS slice, so the stores cover one contiguous span
  if (lane < nv) {
    float best = -1.f;
    int arg = 0;
#pragma unroll
    for (int k = 0; k < KT; ++k) {
      if (k < K) {
        sx[lane * K + k] = mx[k];
        if (mx[k] > best) {
          best = mx[k];
          arg = k;
        }
      }
    }
    if (!slab) mip_pred[opix] = (uint8_t)arg;
  }
  wave_lds_sync();
  float* dst = slab ? slab + (size_t)sl * g.slab_floats : mip_prob;
  dst += ((int64_t)b * g.HW + p0) * K;
  for (int i = lane; i < n; i += 64) dst[i] = sx[i];
}

// 64 pixels per workgroup: the maximum over the round's slabs (and over mip_prob when an
// earlier round left its maxima there), then the class map of the projection.
__global__ __launch_bounds__(PV_T) void k_pred_finish(const float* __restrict__ slab,
                                                      int scount, size_t slab_floats,
                                                      int64_t npix, int K, int fold,
                                                      float* __restrict__ mip_prob,
                                                      uint8_t* __restrict__ mip_pred) {
  __shared__ float sm[64 * PV_MAX_K];
  const int64_t p0 = (int64_t)blockIdx.x * 64;
  const int nv = (int)(npix - p0 < 64 ? npix - p0 : 64);
  const int n = nv * K;
  for (int i = threadIdx.x; i < n; i += PV_T) {
    const int64_t o = p0 * K + i;
    float m = fold ? mip_prob[o] : 0.f;
    for (int s = 0; s < scount; ++s) m = fmaxf(m, slab[(size_t)s * slab_floats + o]);
    mip_prob[o] = m;
    sm[i] = m;
  }
  __syncthreads();
  if ((int)threadIdx.x < nv) {
    const float* r = sm + threadIdx.x * K;
    float best = -1.f;
    int arg = 0;
    for (int k = 0; k < K; ++k) {
      if (r[k] > best) {
        best = r[k];
        arg = k;
      }
    }
    mip_pred[p0 + threadIdx.x] = (uint8_t)arg;
  }
}

// a thread per pixel of channel 0: the centre frame and the maximum over depth
__global__ __launch_bounds__(PV_T) void k_input_views(const float* __restrict__ x, int C, int D,
                                                      int64_t HW, int64_t npix,
                                                      float* __restrict__ center,
                                                      float* __restrict__ mip) {
  const int64_t i = (int64_t)blockIdx.x * PV_T + threadIdx.x;
  if (i >= npix) return;
  const int64_t b = i / HW, p = i % HW;
  const float* col = x + b * C * D * HW + p;
  float m = col[0];
#pragma unroll 8
  for (int d = 1; d < D; ++d) m = fmaxf(m, col[(int64_t)d * HW]);
  center[i] = col[(int64_t)(D / 2) * HW];
  mip[i] = m;
}

// workgroup (image, b): range[b][2 image + {0, 1}] = min, max of the image's H W values
__global__ __launch_bounds__(1024) void k_image_range(const float* __restrict__ center,
                                                      const float* __restrict__ mip, int64_t HW,
                                                      float* __restrict__ range) {
  __shared__ float slo[1024], shi[1024];
  const int img = blockIdx.x & 1;
  const int64_t b = blockIdx.x >> 1;
  const float* v = (img ? mip : center) + b * HW;
  float lo = INFINITY, hi = -INFINITY;
  for (int64_t i = threadIdx.x; i < HW; i += 1024) {
    lo = fminf(lo, v[i]);
    hi = fmaxf(hi, v[i]);
  }
  slo[threadIdx.x] = lo;
  shi[threadIdx.x] = hi;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      slo[threadIdx.x] = fminf(slo[threadIdx.x], slo[threadIdx.x + o]);
      shi[threadIdx.x] = fmaxf(shi[threadIdx.x], shi[threadIdx.x + o]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    range[b * 4 + 2 * img] = slo[0];
    range[b * 4 + 2 * img + 1] = shi[0];
  }
}

__device__ __forceinline__ float grey_of(float v, float lo, float hi) {
  return hi == lo ? 0.f : rintf(255.f * (v - lo) / (hi - lo));
}

// a thread per pixel of the strip [B][H][5 W]: panel = column / W
__global__ __launch_bounds__(PV_T) void k_overlay_rgb(const float* __restrict__ center,
                                                      const float* __restrict__ mip,
                                                      const float* __restrict__ range,
                                                      const int64_t* __restrict__ labels,
                                                      const uint8_t* __restrict__ center_pred,
                                                      const uint8_t* __restrict__ mip_pred,
                                                      const float* __restrict__ alpha_center,
                                                      const uint8_t* __restrict__ colors, int K,
                                                      int H, int W, int64_t total,
                                                      uint8_t* __restrict__ rgb) {
  const int64_t i = (int64_t)blockIdx.x * PV_T + threadIdx.x;
  if (i >= total) return;
  const int W5 = 5 * W;
  const int col = (int)(i % W5);
  const int64_t bh = i / W5;  // b H + h
  const int64_t b = bh / H;
  const int panel = col / W;
  const int64_t px = bh * W + (col - panel * W);
  const float* rg = range + b * 4;
  const float g = panel == 3 ? grey_of(mip[px], rg[2], rg[3]) : grey_of(center[px], rg[0], rg[1]);
  float a = 0.f;
  int cls = 0;
  if (panel == 1) {
    const int64_t y = labels ? labels[px] : 255;
    if (y >= 0 && y < K && y != 255) {  // any other label leaves the grey pixel
      a = 0.85f;
      cls = (int)y;
    }
  } else if (panel == 2) {
    a = 0.85f;
    cls = center_pred[px];
  } else if (panel == 3) {
    a = 0.85f;
    cls = mip_pred[px];
  } else if (panel == 4) {
    a = 0.8f * fminf(fmaxf(alpha_center[px], 0.35f), 1.f);
    cls = center_pred[px];
  }
  uint8_t* o = rgb + i * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c)
    o[c] = (uint8_t)(a == 0.f ? g : rintf((1.f - a) * g + a * (float)colors[cls * 3 + c]));
}

}  // namespace

hipError_t pred_views(const float* logits, const ViewsGeo& g, int depth_split,
                      uint8_t* center_pred, float* alpha_center, float* mip_prob,
                      uint8_t* mip_pred, void* ws, hipStream_t s) {
  const int nsplit = depth_split > 0 ? depth_split : g.auto_split;
  float* slab = nsplit > 1 ? static_cast<float*>(ws) : nullptr;
  const size_t lds = (size_t)PV_WAVES * 64 * g.K * sizeof(float);
  const int64_t npix = (int64_t)g.B * g.HW;
  for (int s0 = 0; s0 < nsplit; s0 += g.slabs) {
    const int sc = nsplit - s0 < g.slabs ? nsplit - s0 : g.slabs;
    const int64_t waves = (int64_t)g.B * sc * g.ngroups;
    const dim3 grid((unsigned)((waves + PV_WAVES - 1) / PV_WAVES));
    if (g.K <= 16)
      hipLaunchKernelGGL(k_pred_views<16>, grid, dim3(PV_T), lds, s, logits, g, nsplit, s0, sc,
                         center_pred, alpha_center, mip_prob, mip_pred, slab);
    else
      hipLaunchKernelGGL(k_pred_views<32>, grid, dim3(PV_T), lds, s, logits, g, nsplit, s0, sc,
                         center_pred, alpha_center, mip_prob, mip_pred, slab);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (slab) {
      hipLaunchKernelGGL(k_pred_finish, dim3((unsigned)((npix + 63) / 64)), dim3(PV_T), 0, s, slab,
                         sc, g.slab_floats, npix, g.K, s0 > 0 ? 1 : 0, mip_prob, mip_pred);
      if ((e = hipGetLastError()) != hipSuccess) return e;
    }
  }
  return hipSuccess;
}

}  // namespace spff

// =================================================================== C ABI ==
using namespace spff;

namespace {
const char* views_extent_check(int B, int D, int H, int W) {
  if (B < 1 || D < 1 || H < 1 || W < 1) return "an extent below 1";
  // workgroup ids are 32-bit: a wave per 64 pixels and depth range, a thread per strip pixel
  if ((double)B * D * ((double)H * W / 64.0 + 1.0) >= 2147483647.0 ||
      (double)B * H * W * 5.0 >= 2147483647.0 * 256.0)
    return "more than 2^31 workgroups";
  return nullptr;
}
const char* pred_views_check(int B, int D, int H, int W, int K) {
  if (K < 1 || K > PV_MAX_K) return "num_classes must be 1..32";
  return views_extent_check(B, D, H, W);
}
int views_einval(const char* fn, const char* what) {
  static thread_local char buf[160];
  snprintf(buf, sizeof buf, "%s: %s", fn, what);
  return set_error(SPFF_EINVAL, buf);
}
}  // namespace

extern "C" {

size_t spff_pred_views_ws_bytes(int B, int D, int H, int W, int num_classes) {
  if (pred_views_check(B, D, H, W, num_classes)) return 0;
  return views_geo(B, D, H, W, num_classes).bytes;
}

int spff_pred_views(const float* logits, int B, int D, int H, int W, int num_classes,
                    int depth_split, uint8_t* center_pred, float* alpha_center, float* mip_prob,
                    uint8_t* mip_pred, void* ws, void* stream) {
  if (const char* m = pred_views_check(B, D, H, W, num_classes))
    return views_einval("spff_pred_views", m);
  if (depth_split < 0 || depth_split > D)
    return views_einval("spff_pred_views", "depth_split must be 0 (automatic) or 1..D");
  if (!logits || !center_pred || !alpha_center || !mip_prob || !mip_pred || !ws)
    return views_einval("spff_pred_views", "null argument");
  const hipError_t e = pred_views(logits, views_geo(B, D, H, W, num_classes), depth_split,
                                  center_pred, alpha_center, mip_prob, mip_pred, ws,
                                  static_cast<hipStream_t>(stream));
  return e == hipSuccess ? SPFF_OK : set_error(SPFF_EHIP, hipGetErrorString(e));
}

int spff_input_views(const float* x, int B, int C, int D, int H, int W, float* center, float* mip,
                     float* range, void* stream) {
  if (C < 1) return views_einval("spff_input_views", "an extent below 1");
  if (const char* m = views_extent_check(B, D, H, W)) return views_einval("spff_input_views", m);
  if (!x || !center || !mip || !range) return views_einval("spff_input_views", "null argument");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t HW = (int64_t)H * W, npix = (int64_t)B * HW;
  hipLaunchKernelGGL(k_input_views, dim3((unsigned)((npix + PV_T - 1) / PV_T)), dim3(PV_T), 0, s, x,
                     C, D, HW, npix, center, mip);
  hipLaunchKernelGGL(k_image_range, dim3((unsigned)(2 * B)), dim3(1024), 0, s, center, mip, HW,
                     range);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? SPFF_OK : set_error(SPFF_EHIP, hipGetErrorString(e));
}

int spff_overlay_rgb(const float* center, const float* mip, const float* range,
                     const int64_t* labels_center, const uint8_t* center_pred,
                     const uint8_t* mip_pred, const float* alpha_center, const uint8_t* colors,
                     int B, int H, int W, int num_classes, uint8_t* rgb, void* stream) {
  if (num_classes < 1 || num_classes > PV_MAX_K)
    return views_einval("spff_overlay_rgb", "num_classes must be 1..32");
  if (const char* m = views_extent_check(B, 1, H, W)) return views_einval("spff_overlay_rgb", m);
  if (!center || !mip || !range || !center_pred || !mip_pred || !alpha_center || !colors || !rgb)
    return views_einval("spff_overlay_rgb", "null argument");
  const int64_t total = (int64_t)B * H * W * 5;
  hipLaunchKernelGGL(k_overlay_rgb, dim3((unsigned)((total + PV_T - 1) / PV_T)), dim3(PV_T), 0,
                     static_cast<hipStream_t>(stream), center, mip, range, labels_center,
                     center_pred, mip_pred, alpha_center, colors, num_classes, H, W, total, rgb);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? SPFF_OK : set_error(SPFF_EHIP, hipGetErrorString(e));
}

}  // extern "C"
