// Three-axis trilinear resampling of channel-last volumes and its adjoint (UNETR: the Lit
// wrapper resamples the padded input to the network grid and the logits back), plus the
// 16^3 patch gather of the ViT patch embedding.
//
// Index rule: ATen upsample_trilinear3d, align_corners=False, output size given.  Per axis
// scale = in / out (fp32), src = max(0, scale (o + 0.5) - 0.5), i0 = (int) src,
// i1 = i0 + (i0 < in - 1), l1 = src - i0, l0 = 1 - l1; an axis with in == out reads
// i0 = i1 = o with weights 1 and 0, so it comes out bit-exact.  The value is nested as ATen
// nests it: depth outer, then height, width innermost.
#include "swin_internal.h"
#include "spff.h"

#include <algorithm>

namespace spff {

namespace {

struct Lin3 {
  int i0, i1;
  float l0, l1;
};

__device__ __forceinline__ Lin3 lin3(int o, int in, int out) {
  Lin3 r;
  if (in == out) {
    r.i0 = r.i1 = o;
    r.l0 = 1.f;
    r.l1 = 0.f;
    return r;
  }
  const float scale = (float)in / (float)out;
  float src = scale * ((float)o + 0.5f) - 0.5f;
  src = src < 0.f ? 0.f : src;
  r.i0 = (int)src;
  if (r.i0 > in - 1) r.i0 = in - 1;
  r.i1 = r.i0 + (r.i0 < in - 1 ? 1 : 0);
  r.l1 = src - (float)r.i0;
  r.l0 = 1.f - r.l1;
  return r;
}

// the outputs [lo, hi) that read input i: i1(o) and i0(o) do not decrease with o, so they
// are the o with i1(o) >= i and i0(o) <= i
__device__ __forceinline__ void lin3_touch(int i, int in, int out, int& lo, int& hi) {
  if (in == out) {
    lo = i;
    hi = i + 1;
    return;
  }
  int g = (int)floorf(((float)i - 0.5f) * ((float)out / (float)in));
  g = g < 0 ? 0 : (g > out ? out : g);
  while (g > 0 && lin3(g - 1, in, out).i1 >= i) --g;
  while (g < out && lin3(g, in, out).i1 < i) ++g;
  lo = g;
  while (g < out && lin3(g, in, out).i0 <= i) ++g;
  hi = g;
}

// weight of input i in output o
__device__ __forceinline__ float lin3_w(const Lin3& a, int i) {
  return (a.i0 == i ? a.l0 : 0.f) + (a.i1 == i ? a.l1 : 0.f);
}

struct Grid3 {
  int B, C, Di, Hi, Wi, Do, Ho, Wo;
};

__device__ __forceinline__ float tri(const float* __restrict__ p, int64_t sd, int64_t sh,
                                     int64_t sw, const Lin3& d, const Lin3& h, const Lin3& w) {
  const float* d0 = p + d.i0 * sd;
  const float* d1 = p + d.i1 * sd;
  const float a = h.l0 * (w.l0 * d0[h.i0 * sh + w.i0 * sw] + w.l1 * d0[h.i0 * sh + w.i1 * sw]) +
                  h.l1 * (w.l0 * d0[h.i1 * sh + w.i0 * sw] + w.l1 * d0[h.i1 * sh + w.i1 * sw]);
  const float b = h.l0 * (w.l0 * d1[h.i0 * sh + w.i0 * sw] + w.l1 * d1[h.i0 * sh + w.i1 * sw]) +
                  h.l1 * (w.l0 * d1[h.i1 * sh + w.i0 * sw] + w.l1 * d1[h.i1 * sh + w.i1 * sw]);
  return d.l0 * a + d.l1 * b;
}

// x [B][Di][Hi][Wi][C] -> y [B][Do][Ho][Wo][C]
__global__ void k_resize3d_fwd(const float* __restrict__ x, float* __restrict__ y, Grid3 g) {
  const int64_t total = (int64_t)g.B * g.Do * g.Ho * g.Wo * g.C;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % g.C);
    int64_t t = i / g.C;
    const int wo = (int)(t % g.Wo); t /= g.Wo;
    const int ho = (int)(t % g.Ho); t /= g.Ho;
    const int od = (int)(t % g.Do); t /= g.Do;  // t = b
    const Lin3 d = lin3(od, g.Di, g.Do), h = lin3(ho, g.Hi, g.Ho), w = lin3(wo, g.Wi, g.Wo);
    const int64_t sw = g.C, sh = sw * g.Wi, sd = sh * g.Hi;
    y[i] = tri(x + t * sd * g.Di + c, sd, sh, sw, d, h, w);
  }
}

// x [B][C][Di][Hi][Wi] -> y [B][Do][Ho][Wo][ldy], channels C .. ldy - 1 zero
__global__ void k_resize3d_ncdhw_in(const float* __restrict__ x, float* __restrict__ y, Grid3 g,
                                    int ldy) {
  const int64_t total = (int64_t)g.B * g.Do * g.Ho * g.Wo * ldy;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % ldy);
    int64_t t = i / ldy;
    const int wo = (int)(t % g.Wo); t /= g.Wo;
    const int ho = (int)(t % g.Ho); t /= g.Ho;
    const int od = (int)(t % g.Do); t /= g.Do;
    float v = 0.f;
    if (c < g.C) {
      const Lin3 d = lin3(od, g.Di, g.Do), h = lin3(ho, g.Hi, g.Ho), w = lin3(wo, g.Wi, g.Wo);
      const int64_t sw = 1, sh = g.Wi, sd = sh * g.Hi;
      v = tri(x + (t * g.C + c) * sd * g.Di, sd, sh, sw, d, h, w);
    }
    y[i] = v;
  }
}

// dx [B][Di][Hi][Wi][C] = R^T dy: every input voxel sums the outputs that read it, in
// (depth, height, width) order of the outputs -- no atomics
__global__ void k_resize3d_bwd(const float* __restrict__ dy, float* __restrict__ dx, Grid3 g) {
  const int64_t total = (int64_t)g.B * g.Di * g.Hi * g.Wi * g.C;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % g.C);
    int64_t t = i / g.C;
    const int wi = (int)(t % g.Wi); t /= g.Wi;
    const int hi = (int)(t % g.Hi); t /= g.Hi;
    const int di = (int)(t % g.Di); t /= g.Di;
    int dlo, dhi, hlo, hhi, wlo, whi;
    lin3_touch(di, g.Di, g.Do, dlo, dhi);
    lin3_touch(hi, g.Hi, g.Ho, hlo, hhi);
    lin3_touch(wi, g.Wi, g.Wo, wlo, whi);
    const float* p = dy + t * g.Do * g.Ho * g.Wo * g.C + c;
    float acc = 0.f;
    for (int od = dlo; od < dhi; ++od) {
      const float wd = lin3_w(lin3(od, g.Di, g.Do), di);
      for (int oh = hlo; oh < hhi; ++oh) {
        const float wdh = wd * lin3_w(lin3(oh, g.Hi, g.Ho), hi);
        const float* row = p + ((int64_t)od * g.Ho + oh) * g.Wo * g.C;
        for (int ow = wlo; ow < whi; ++ow) {
          const float wt = wdh * lin3_w(lin3(ow, g.Wi, g.Wo), wi);
          acc = fmaf(wt, row[(int64_t)ow * g.C], acc);
        }
      }
    }
    dx[i] = acc;
  }
}

// x [B][D][H][W][ldx] -> rows [B (D/16)(H/16)(W/16)][cin 4096] in (c, kd, kh, kw) order
__global__ void k_patchify16(const float* __restrict__ x, int ldx, int cin, int B, int D, int H,
                             int W, float* __restrict__ rows) {
  const int64_t total = (int64_t)B * D * H * W * cin;
  const int pd = D / 16, ph = H / 16, pw = W / 16;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    int64_t t = i;
    const int kw = (int)(t & 15); t >>= 4;
    const int kh = (int)(t & 15); t >>= 4;
    const int kd = (int)(t & 15); t >>= 4;
    const int c = (int)(t % cin); t /= cin;
    const int tw = (int)(t % pw); t /= pw;
    const int th = (int)(t % ph); t /= ph;
    const int td = (int)(t % pd); t /= pd;  // t = b
    const int64_t v = ((t * D + td * 16 + kd) * H + th * 16 + kh) * W + tw * 16 + kw;
    rows[i] = x[v * ldx + c];
  }
}

inline int grid_for(int64_t total) { return (int)std::min<int64_t>((total + 255) / 256, 65536); }

}  // namespace

hipError_t resize3d_fwd(const float* x, float* y, int B, int C, int Di, int Hi, int Wi, int Do,
                        int Ho, int Wo, hipStream_t s) {
  const Grid3 g{B, C, Di, Hi, Wi, Do, Ho, Wo};
  const int64_t total = (int64_t)B * Do * Ho * Wo * C;
  hipLaunchKernelGGL(k_resize3d_fwd, dim3(grid_for(total)), dim3(256), 0, s, x, y, g);
  return hipGetLastError();
}

hipError_t resize3d_bwd(const float* dy, float* dx, int B, int C, int Di, int Hi, int Wi, int Do,
                        int Ho, int Wo, hipStream_t s) {
  const Grid3 g{B, C, Di, Hi, Wi, Do, Ho, Wo};
  const int64_t total = (int64_t)B * Di * Hi * Wi * C;
  hipLaunchKernelGGL(k_resize3d_bwd, dim3(grid_for(total)), dim3(256), 0, s, dy, dx, g);
  return hipGetLastError();
}

hipError_t resize3d_ncdhw_in(const float* x, float* y, int ldy, int B, int C, int Di, int Hi,
                             int Wi, int Do, int Ho, int Wo, hipStream_t s) {
  if (ldy < C) return hipErrorInvalidValue;
  const Grid3 g{B, C, Di, Hi, Wi, Do, Ho, Wo};
  const int64_t total = (int64_t)B * Do * Ho * Wo * ldy;
  hipLaunchKernelGGL(k_resize3d_ncdhw_in, dim3(grid_for(total)), dim3(256), 0, s, x, y, g, ldy);
  return hipGetLastError();
}

hipError_t patchify16(const float* x, int ldx, int cin, int B, int D, int H, int W, float* rows,
                      hipStream_t s) {
  if (D % 16 || H % 16 || W % 16 || cin > ldx) return hipErrorInvalidValue;
  const int64_t total = (int64_t)B * D * H * W * cin;
  hipLaunchKernelGGL(k_patchify16, dim3(grid_for(total)), dim3(256), 0, s, x, ldx, cin, B, D, H, W,
                     rows);
  return hipGetLastError();
}

}  // namespace spff

// =================================================================== C ABI ==
using namespace spff;

namespace {
bool grid_ok(int B, int C, int Di, int Hi, int Wi, int Do, int Ho, int Wo) {
  return B >= 1 && C >= 1 && Di >= 1 && Hi >= 1 && Wi >= 1 && Do >= 1 && Ho >= 1 && Wo >= 1;
}
}  // namespace

extern "C" {

int spff_resize3d_fwd(const float* x, float* y, int batch, int channels, int din, int hin,
                      int win, int dout, int hout, int wout, void* stream) {
  if (!grid_ok(batch, channels, din, hin, win, dout, hout, wout) || !x || !y)
    return set_error(SPFF_EINVAL, "spff_resize3d_fwd: bad argument");
  const hipError_t e = resize3d_fwd(x, y, batch, channels, din, hin, win, dout, hout, wout,
                                    static_cast<hipStream_t>(stream));
  return e == hipSuccess ? SPFF_OK : set_error(SPFF_EHIP, hipGetErrorString(e));
}

int spff_resize3d_bwd(const float* dy, float* dx, int batch, int channels, int din, int hin,
                      int win, int dout, int hout, int wout, void* stream) {
  if (!grid_ok(batch, channels, din, hin, win, dout, hout, wout) || !dy || !dx)
    return set_error(SPFF_EINVAL, "spff_resize3d_bwd: bad argument");
  const hipError_t e = resize3d_bwd(dy, dx, batch, channels, din, hin, win, dout, hout, wout,
                                    static_cast<hipStream_t>(stream));
  return e == hipSuccess ? SPFF_OK : set_error(SPFF_EHIP, hipGetErrorString(e));
}

}  // extern "C"
