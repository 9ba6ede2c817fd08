// ResUNet++ variant: the residual 3D U-Net with an ASPP bottleneck, SE-gated skips and
// attention gates behind the registry entry "ResUNet++" (LitResUNetPP3D_Published around
// ResUNetPP3D_backbone).
//
// Graph, levels l = 0..4 halve D, H, W (MaxPool3d(2)), channels C_l = base << l:
//   e1 = ru(x); e2 = ru(pool(e1)); e3 = ru(pool(e2)); e4 = ru(pool(e3))
//   b  = b_aspp_out(aspp(b_aspp_in(pool(e4))))
//   u4 = up4(b);  s4 = ag4(u4, se4(e4)); d4 = ru([u4 | s4])      (likewise levels 3, 2)
//   u1 = up1(d2); d1 = ru([u1 | se1(e1)]); logits = head(d1)
// ru(cin -> C):  s = skip(x) (1x1x1 without bias, or x itself when cin == C)
//                a1 = relu(IN1(c1(x)));  out = relu(IN2(c2(a1)) + s)
// aspp(C):       cat_r conv3x3x3(x, dilation = padding = r), r = 1, 2, 4, 8 -> 1x1x1 -> relu
// se(C):         x * sigmoid(W2 relu(W1 mean_dhw(x) + b1) + b2)
// ag(u, g):      u * sigmoid(psi(relu(W_x u + W_g g)))   -- the reference passes the
//                up-sampled tensor first and the gate multiplies its first argument, so the
//                encoder features reach the decoder only through the gate's hidden row.
//
// What runs where.  The undilated convs, InstanceNorm statistics, ReLU applies, pools,
// up-convs, head and every 1x1x1 conv run on the engine's kernels (conv3d_run /
// conv3d_wgrad in the plan's SPFF_MATH_*, slab_reduce + in_mean / in_rstd, act_apply,
// linear_*, maxpool3_*, upconv_*, head_*); [u | s] is read through two-source views.  New
// here: the dilated conv (forward / input gradient / weight gradient, fp32 MFMA under every
// math: it runs at 1/16 resolution), the residual tail and its mask and the SE gate.  The
// attention gate is attn_gate.hip's, shared with the SPFF plan's gated skips.
//
// Residual tail backward.  dz = dout [out > 0] is written once (k_rupp_mask): it is the
// skip path's gradient and, being already masked by the block's output, enters IN2's
// backward as a plain gradient -- RED_BWD_IN / in_bwd_apply with slope 1 on both sides of
// zero, so no mask of IN2(y2) is applied.
//
// Attention gate (attn_gate.hip).  The hidden row is one GEMM over the two-source view [u | se(e)] with the
// weight [W_x | W_g] and the bias b_x + b_g; its ReLU output att [V][C/2] is stored, as is
// psi (one float per voxel).  The backward forms dpsi per voxel, reduces psi's weight
// gradient in a fixed two-stage order, forms the hidden row's gradient from att's signs
// and hands it to linear_wgrad2 / linear_dgrad2.
//
// Order of every accumulation is fixed (single stream, ordered partial sums): two runs give
// the same bits.
#include "plan_ops.h"

#include <algorithm>
#include <string>
#include <vector>

using namespace spff;

namespace {

constexpr int NLVL = 5, NUNIT = 10, NUP = 4, NBR = 4, NSE = 4, NAG = 3;

typedef float f32x4 __attribute__((ext_vector_type(4)));

unsigned ew_grid(int64_t work) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>((work + 255) / 256, 8192));
}

// ------------------------------------------------------------- dilated conv --
// live taps of a launch: tap t = (kd * 3 + kh) * 3 + kw is dropped when r |k - 1| >= the
// axis extent, i.e. when it reads padding for every output voxel
struct DilTaps {
  int n;
  int t[27];
};
DilTaps dil_taps(const Vol& v, int r) {
  DilTaps T;
  T.n = 0;
  for (int t = 0; t < 27; ++t) {
    const int kd = t / 9 - 1, kh = (t / 3) % 3 - 1, kw = t % 3 - 1;
    if ((kd && r >= v.D) || (kh && r >= v.H) || (kw && r >= v.W)) continue;
    T.t[T.n++] = t;
  }
  return T;
}

// P[tap][co][ci] = w[co][ci][tap]: rows of Cin contiguous floats for the forward's B
// operand, columns of it for the input gradient's
__global__ __launch_bounds__(256) void k_dil_pack(const float* __restrict__ w,
                                                  float* __restrict__ P, int Cout, int Cin) {
  const int64_t n = (int64_t)27 * Cout * Cin, cc = (int64_t)Cout * Cin;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t t = i / cc, r = i - t * cc;
    P[i] = w[r * 27 + t];
  }
}

// Implicit GEMM on v_mfma_f32_16x16x4_f32: a wave owns 16 voxels x 32 output channels.
// Lane l supplies A[voxel l & 15][k = 4 (l >> 4) + q] (one float4 of the input row per 16
// reduction channels) and B[k][column l & 15]; the four k of a quad go through four MFMAs.
// DG = false: y[v][n] = sum_tap sum_k x[v + r off(tap)][k] P[tap][n][k]      (K = Cin, N = Cout)
// DG = true:  y[v][n] = sum_tap sum_k x[v - r off(tap)][k] P[tap][k][n]      (K = Cout, N = Cin)
// acc: add to y (the ASPP's four input gradients, branch after branch on one stream).
template <bool DG>
__global__ __launch_bounds__(256) void k_dil_conv(const float* __restrict__ x, int ldx,
                                                  const float* __restrict__ P,
                                                  float* __restrict__ y, int ldy, Vol vol, int K,
                                                  int N, int r, int acc, DilTaps taps) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int i = lane & 15, kg = lane >> 4;
  const int64_t V = (int64_t)vol.B * vol.D * vol.H * vol.W;
  const int64_t v0 = ((int64_t)blockIdx.x * 4 + wv) * 16;
  if (v0 >= V) return;  // wave-uniform
  const int n0 = blockIdx.y * 32;
  const int ntile = n0 + 16 < N ? 2 : 1;
  const int64_t v = v0 + i;
  const bool vin = v < V;
  int b = 0, d = 0, h = 0, w = 0;
  if (vin) {
    int64_t t = v;
    w = (int)(t % vol.W); t /= vol.W;
    h = (int)(t % vol.H); t /= vol.H;
    d = (int)(t % vol.D);
    b = (int)(t / vol.D);
  }
  f32x4 c[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  const int step = DG ? -r : r;
  for (int ti = 0; ti < taps.n; ++ti) {
    const int t = taps.t[ti];
    const int dd = d + step * (t / 9 - 1), hh = h + step * ((t / 3) % 3 - 1),
              ww = w + step * (t % 3 - 1);
    const bool inb = vin && (unsigned)dd < (unsigned)vol.D && (unsigned)hh < (unsigned)vol.H &&
                     (unsigned)ww < (unsigned)vol.W;
    const float* row = x + ((((int64_t)b * vol.D + dd) * vol.H + hh) * vol.W + ww) * ldx;
    const float* Pt = P + (int64_t)t * K * N;
    for (int k0 = 0; k0 < K; k0 += 16) {
      const int kk = k0 + 4 * kg;
      const bool kin = kk < K;
      float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
      if (inb && kin) a = *reinterpret_cast<const float4*>(row + kk);
      for (int nt = 0; nt < ntile; ++nt) {
        const int n = n0 + nt * 16 + i;
        float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (n < N && kin) {
          if (!DG) {
            bv = *reinterpret_cast<const float4*>(Pt + (int64_t)n * K + kk);
          } else {
            const float* q = Pt + (int64_t)kk * N + n;
            bv = make_float4(q[0], q[N], q[2 * (int64_t)N], q[3 * (int64_t)N]);
          }
        }
        c[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, bv.x, c[nt], 0, 0, 0);
        c[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, bv.y, c[nt], 0, 0, 0);
        c[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, bv.z, c[nt], 0, 0, 0);
        c[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, bv.w, c[nt], 0, 0, 0);
      }
    }
  }
  // C/D map: column l & 15, row 4 (l >> 4) + reg
  for (int nt = 0; nt < ntile; ++nt) {
    const int n = n0 + nt * 16 + i;
    if (n >= N) continue;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int64_t vv = v0 + 4 * kg + q;
      if (vv >= V) continue;
      float* o = y + vv * ldy + n;
      *o = acc ? *o + c[nt][q] : c[nt][q];
    }
  }
}

// dw[co][ci][tap] = sum_v dy[v][co] x[v + r off(tap)][ci] for the live taps (the others are
// zeroed by the caller).  One workgroup per (16 ci, 16 co, tap): its four waves take the
// voxel groups 16 (4 j + wave) .. in turn, a quad of voxels per MFMA, and their partial
// tiles are added in wave order through LDS -- a fixed order.
__global__ __launch_bounds__(256) void k_dil_wgrad(const float* __restrict__ x, int ldx,
                                                   const float* __restrict__ dy, int ldy,
                                                   float* __restrict__ dw, Vol vol, int Cin,
                                                   int Cout, int r, DilTaps taps) {
  __shared__ float red[4][64][4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int i = lane & 15, kg = lane >> 4;
  const int ci0 = blockIdx.x * 16, co0 = blockIdx.y * 16;
  const int t = taps.t[blockIdx.z];
  const int od = r * (t / 9 - 1), oh = r * ((t / 3) % 3 - 1), ow = r * (t % 3 - 1);
  const int64_t V = (int64_t)vol.B * vol.D * vol.H * vol.W;
  const int co = co0 + i, ci = ci0 + i;
  f32x4 c = {0.f, 0.f, 0.f, 0.f};
  for (int64_t vb = (int64_t)wv * 16; vb < V; vb += 64) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t v = vb + 4 * u + kg;
      float a = 0.f, bq = 0.f;
      if (v < V) {
        if (co < Cout) a = dy[v * ldy + co];
        int64_t q = v;
        const int w = (int)(q % vol.W); q /= vol.W;
        const int h = (int)(q % vol.H); q /= vol.H;
        const int d = (int)(q % vol.D);
        const int b = (int)(q / vol.D);
        const int dd = d + od, hh = h + oh, ww = w + ow;
        if (ci < Cin && (unsigned)dd < (unsigned)vol.D && (unsigned)hh < (unsigned)vol.H &&
            (unsigned)ww < (unsigned)vol.W)
          bq = x[((((int64_t)b * vol.D + dd) * vol.H + hh) * vol.W + ww) * ldx + ci];
      }
      c = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bq, c, 0, 0, 0);
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) red[wv][lane][q] = c[q];
  __syncthreads();
  if (wv == 0 && ci < Cin) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int row = co0 + 4 * kg + q;
      if (row >= Cout) continue;
      const float s = ((red[0][lane][q] + red[1][lane][q]) + red[2][lane][q]) + red[3][lane][q];
      dw[((int64_t)row * Cin + ci) * 27 + t] = s;
    }
  }
}

hipError_t dil_pack(const float* w, float* P, int Cin, int Cout, hipStream_t s) {
  hipLaunchKernelGGL(k_dil_pack, dim3(ew_grid((int64_t)27 * Cin * Cout)), dim3(256), 0, s, w, P,
                     Cout, Cin);
  return hipGetLastError();
}
// forward (dgrad = false: x has Cin channels, y Cout) or input gradient (dgrad = true: x = dy
// with Cout channels, y = dx with Cin); P from dil_pack
hipError_t dil_run(const float* x, int ldx, const float* P, float* y, int ldy, const Vol& v,
                   int Cin, int Cout, int r, bool dgrad, int acc, hipStream_t s) {
  const DilTaps T = dil_taps(v, r);
  const int N = dgrad ? Cin : Cout, K = dgrad ? Cout : Cin;
  const dim3 grid((unsigned)((nvox(v) + 63) / 64), (unsigned)((N + 31) / 32));
  if (dgrad)
    hipLaunchKernelGGL(k_dil_conv<true>, grid, dim3(256), 0, s, x, ldx, P, y, ldy, v, K, N, r, acc, T);
  else
    hipLaunchKernelGGL(k_dil_conv<false>, grid, dim3(256), 0, s, x, ldx, P, y, ldy, v, K, N, r, acc, T);
  return hipGetLastError();
}
hipError_t dil_wgrad(const float* x, int ldx, const float* dy, int ldy, float* dw, const Vol& v,
                     int Cin, int Cout, int r, hipStream_t s) {
  const DilTaps T = dil_taps(v, r);
  if (T.n < 27) {
    hipError_t e = spff::zero_async(dw, (size_t)27 * Cin * Cout * sizeof(float), s);
    if (e != hipSuccess) return e;
  }
  const dim3 grid((unsigned)((Cin + 15) / 16), (unsigned)((Cout + 15) / 16), (unsigned)T.n);
  hipLaunchKernelGGL(k_dil_wgrad, grid, dim3(256), 0, s, x, ldx, dy, ldy, dw, v, Cin, Cout, r, T);
  return hipGetLastError();
}

// ---------------------------------------------------- elementwise kernels --
// out = relu(y2 al[b,c] + de[b,c] + s): the residual unit's tail in one pass
__global__ __launch_bounds__(256) void k_rupp_tail(const float* __restrict__ y2,
                                                   const float* __restrict__ al,
                                                   const float* __restrict__ de,
                                                   const float* __restrict__ sk,
                                                   float* __restrict__ out, int64_t n4, int C4,
                                                   int64_t vps) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t v = i / C4;
    const int c = (int)(i - v * C4) * 4;
    const int64_t bc = (v / vps) * (C4 * 4) + c;
    const float4 y = reinterpret_cast<const float4*>(y2)[i];
    const float4 s = reinterpret_cast<const float4*>(sk)[i];
    const float4 a = *reinterpret_cast<const float4*>(al + bc);
    const float4 e = *reinterpret_cast<const float4*>(de + bc);
    float4 o;
    o.x = fmaxf(y.x * a.x + e.x + s.x, 0.f);
    o.y = fmaxf(y.y * a.y + e.y + s.y, 0.f);
    o.z = fmaxf(y.z * a.z + e.z + s.z, 0.f);
    o.w = fmaxf(y.w * a.w + e.w + s.w, 0.f);
    reinterpret_cast<float4*>(out)[i] = o;
  }
}
// dz = g [out > 0] (dz may alias g)
__global__ __launch_bounds__(256) void k_rupp_mask(const float* __restrict__ g,
                                                   const float* __restrict__ out,
                                                   float* __restrict__ dz, int64_t n4) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4;
       i += (int64_t)gridDim.x * blockDim.x) {
    const float4 a = reinterpret_cast<const float4*>(g)[i];
    const float4 o = reinterpret_cast<const float4*>(out)[i];
    float4 z;
    z.x = o.x > 0.f ? a.x : 0.f; z.y = o.y > 0.f ? a.y : 0.f;
    z.z = o.z > 0.f ? a.z : 0.f; z.w = o.w > 0.f ? a.w : 0.f;
    reinterpret_cast<float4*>(dz)[i] = z;
  }
}
__global__ __launch_bounds__(256) void k_rupp_relu(float* __restrict__ x, int64_t n4) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4;
       i += (int64_t)gridDim.x * blockDim.x) {
    float4 a = reinterpret_cast<float4*>(x)[i];
    a.x = fmaxf(a.x, 0.f); a.y = fmaxf(a.y, 0.f); a.z = fmaxf(a.z, 0.f); a.w = fmaxf(a.w, 0.f);
    reinterpret_cast<float4*>(x)[i] = a;
  }
}

// ------------------------------------------------------------------- SE gate --
// per sample: hid = relu(W1 mean + b1) [Hd], gate = sigmoid(W2 hid + b2) [C]
__global__ __launch_bounds__(256) void k_se_gate(const float* __restrict__ mean,
                                                 const float* __restrict__ w1,
                                                 const float* __restrict__ b1,
                                                 const float* __restrict__ w2,
                                                 const float* __restrict__ b2,
                                                 float* __restrict__ hid, float* __restrict__ gate,
                                                 int C, int Hd) {
  extern __shared__ float sh[];  // [Hd]
  const int b = blockIdx.x;
  const float* m = mean + (int64_t)b * C;
  for (int j = threadIdx.x; j < Hd; j += blockDim.x) {
    float s = b1[j];
    for (int c = 0; c < C; ++c) s += w1[(int64_t)j * C + c] * m[c];
    s = fmaxf(s, 0.f);
    sh[j] = s;
    hid[(int64_t)b * Hd + j] = s;
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    float s = b2[c];
    for (int j = 0; j < Hd; ++j) s += w2[(int64_t)c * Hd + j] * sh[j];
    gate[(int64_t)b * C + c] = 1.f / (1.f + expf(-s));
  }
}
// out = x gate[b,c]  (one pass; see DESIGN: the scaled tensor has three readers)
__global__ __launch_bounds__(256) void k_se_scale(const float* __restrict__ x,
                                                  const float* __restrict__ gate,
                                                  float* __restrict__ out, int64_t n4, int C4,
                                                  int64_t vps) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t v = i / C4;
    const int c = (int)(i - v * C4) * 4;
    const float4 g = *reinterpret_cast<const float4*>(gate + (v / vps) * (C4 * 4) + c);
    float4 a = reinterpret_cast<const float4*>(x)[i];
    a.x *= g.x; a.y *= g.y; a.z *= g.z; a.w *= g.w;
    reinterpret_cast<float4*>(out)[i] = a;
  }
}
// From sums[b][c][d][2] (q1 = sum_hw dse x): dgate, then the two FCs' backward.  One
// workgroup walks the samples in order, so the parameter gradients add up in sample order.
// dmean[b][c] = (W1^T dhid)[c] / N, the pooled mean's share of dx per voxel.
__global__ __launch_bounds__(256) void k_se_bwd(const float* __restrict__ sums,
                                                const float* __restrict__ mean,
                                                const float* __restrict__ hid,
                                                const float* __restrict__ gate,
                                                const float* __restrict__ w1,
                                                const float* __restrict__ w2,
                                                float* __restrict__ dw1, float* __restrict__ db1,
                                                float* __restrict__ dw2, float* __restrict__ db2,
                                                float* __restrict__ dmean, int B, int C, int Hd,
                                                int D, float invN) {
  extern __shared__ float sh[];  // dpre [C], dh [Hd]
  float* dpre = sh;
  float* dh = sh + C;
  for (int b = 0; b < B; ++b) {
    const float* hb = hid + (int64_t)b * Hd;
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
      const float* q = sums + ((int64_t)b * C + c) * D * 2;
      float s = 0.f;
      for (int d = 0; d < D; ++d) s += q[2 * d + 1];
      const float g = gate[(int64_t)b * C + c];
      const float dp = s * g * (1.f - g);
      dpre[c] = dp;
      db2[c] = b ? db2[c] + dp : dp;
      for (int j = 0; j < Hd; ++j) {
        const float t = dp * hb[j];
        dw2[(int64_t)c * Hd + j] = b ? dw2[(int64_t)c * Hd + j] + t : t;
      }
    }
    __syncthreads();
    for (int j = threadIdx.x; j < Hd; j += blockDim.x) {
      float s = 0.f;
      for (int c = 0; c < C; ++c) s += w2[(int64_t)c * Hd + j] * dpre[c];
      s = hb[j] > 0.f ? s : 0.f;
      dh[j] = s;
      db1[j] = b ? db1[j] + s : s;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
      const float m = mean[(int64_t)b * C + c];
      float s = 0.f;
      for (int j = 0; j < Hd; ++j) {
        const float t = dh[j] * m;
        dw1[(int64_t)j * C + c] = b ? dw1[(int64_t)j * C + c] + t : t;
        s += w1[(int64_t)j * C + c] * dh[j];
      }
      dmean[(int64_t)b * C + c] = s * invN;
    }
    __syncthreads();
  }
}
// dx = dse gate[b,c] + dmean[b,c], in place
__global__ __launch_bounds__(256) void k_se_bwd_apply(float* __restrict__ g,
                                                      const float* __restrict__ gate,
                                                      const float* __restrict__ dmean, int64_t n4,
                                                      int C4, int64_t vps) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t v = i / C4;
    const int c = (int)(i - v * C4) * 4;
    const int64_t bc = (v / vps) * (C4 * 4) + c;
    const float4 s = *reinterpret_cast<const float4*>(gate + bc);
    const float4 m = *reinterpret_cast<const float4*>(dmean + bc);
    float4 a = reinterpret_cast<float4*>(g)[i];
    a.x = a.x * s.x + m.x; a.y = a.y * s.y + m.y; a.z = a.z * s.z + m.z; a.w = a.w * s.w + m.w;
    reinterpret_cast<float4*>(g)[i] = a;
  }
}

struct PUnit {
  std::string name;
  int lvl, Cin, C;
  bool skip;
  Conv3 cv[2];
  int64_t g1 = -1, b1 = -1, g2 = -1, b2 = -1, wsk = -1;
  size_t y1, a1, y2, out, pk_sk = 0;
  Stat4 s1, s2;
};
struct PSe {
  int C, Hd, lvl;
  int64_t w1, b1, w2, b2;
  size_t mean, hid, gate, dmean, out;
};
struct PAg {
  int C, I, lvl;
  int64_t wx, bx, wg, bg, wpsi, bpsi;
  size_t wcat, bcat, pk, att, psi, s, dwcat, dbcat;
};

}  // namespace

struct spff_rupp : PlanBase {
  spff_rupp_cfg cfg;
  Vol vol[NLVL];
  int f, K, ldx;
  PUnit un[NUNIT];  // e1..e4, b_aspp_in, b_aspp_out, d4..d1
  UpConv up[NUP];   // up4..up1
  PSe se[NSE];      // se1..se4
  PAg ag[NAG];      // ag4, ag3, ag2
  int64_t w_br[NBR] = {}, w_proj = -1, head_w = -1, head_b = -1;
  size_t br_pk[NBR] = {}, cat = 0, dcat = 0, proj_pk = 0, aspp_out = 0;
  size_t head_pk = 0, x_cl = 0, pool[4] = {}, pidx[4] = {};
  size_t red_ws = 0, red_out = 0, kk1 = 0, kk2 = 0, wg_ws = 0, wt = 0, db_scr = 0;
  static constexpr bool pkb = false;  // every conv image is packed before its conv, into wt
  static constexpr size_t wsl = 0;
  size_t ones = 0, zeros = 0, ag_part = 0;
  size_t G_out = 0, G_s = 0, G_1 = 0, G_2 = 0, G_dx = 0, G_ds = 0, dskip[4] = {};
};

namespace {

const int DIL[NBR] = {1, 2, 4, 8};

void reg_unit(spff_rupp* p, PUnit& u) {
  const int C = u.C;
  const std::string n = "backbone." + u.name;
  u.cv[0] = reg_conv(p, n + ".c1.weight", u.Cin, C);
  u.g1 = p->reg(n + ".n1.weight", {C});
  u.b1 = p->reg(n + ".n1.bias", {C});
  u.cv[1] = reg_conv(p, n + ".c2.weight", C, C);
  u.g2 = p->reg(n + ".n2.weight", {C});
  u.b2 = p->reg(n + ".n2.bias", {C});
  if (u.skip) u.wsk = p->reg(n + ".skip.weight", {C, u.Cin, 1, 1, 1});
}

int build(spff_rupp* p) {
  const spff_rupp_cfg& c = p->cfg;
  if (c.batch < 1 || c.depth < 1 || c.height < 1 || c.width < 1)
    return plan_fail(SPFF_EINVAL, "invalid batch / depth / height / width");
  if (c.in_ch < 1 || c.in_ch > 8) return plan_fail(SPFF_EINVAL, "in_ch must be 1..8");
  if (c.num_classes < 2 || c.num_classes > 32)
    return plan_fail(SPFF_EINVAL, "num_classes must be 2..32");
  if (c.base < 8 || c.base % 8) return plan_fail(SPFF_EINVAL, "base must be a multiple of 8");
  if (c.math < SPFF_MATH_F32 || c.math > SPFF_MATH_F16X3)
    return plan_fail(SPFF_EINVAL, "math must be one of SPFF_MATH_*");
  if (c.depth % 16 || c.height % 16 || c.width % 16)
    return plan_fail(SPFF_ESHAPE,
                 "D, H and W must be multiples of 16 (four MaxPool3d(2) whose outputs are "
                 "concatenated with the ConvTranspose3d outputs); the Lit wrapper pads");
  if ((int64_t)(c.depth / 16) * (c.height / 16) * (c.width / 16) < 2)
    return plan_fail(SPFF_ESHAPE,
                 "the bottleneck would hold one voxel per sample: InstanceNorm3d needs more "
                 "than one (the reference raises there)");
  p->f = c.base;
  p->K = c.num_classes;
  p->ldx = 8;
  for (int l = 0; l < NLVL; ++l)
    p->vol[l] = Vol{c.batch, c.depth >> l, c.height >> l, c.width >> l};
  const int f = p->f, B = c.batch;
  const char* names[NUNIT] = {"e1", "e2", "e3", "e4", "b_aspp_in", "b_aspp_out",
                              "d4", "d3", "d2", "d1"};
  const int lvl[NUNIT] = {0, 1, 2, 3, 4, 4, 3, 2, 1, 0};
  const int cin[NUNIT] = {c.in_ch, f, 2 * f, 4 * f, 8 * f, 16 * f, 16 * f, 8 * f, 4 * f, 2 * f};
  const int cc[NUNIT] = {f, 2 * f, 4 * f, 8 * f, 16 * f, 16 * f, 8 * f, 4 * f, 2 * f, f};
  for (int i = 0; i < NUNIT; ++i) {
    PUnit& u = p->un[i];
    u.name = names[i];
    u.lvl = lvl[i];
    u.Cin = cin[i];
    u.C = cc[i];
    u.skip = u.Cin != u.C;
  }
  // registration order of ResUNetPP3D_backbone.__init__, then the Lit head
  for (int i = 0; i < 5; ++i) reg_unit(p, p->un[i]);
  const int C4 = 16 * f;
  for (int r = 0; r < NBR; ++r)
    p->w_br[r] = p->reg("backbone.b_aspp.branches." + std::to_string(r) + ".weight",
                        {C4, C4, 3, 3, 3});
  p->w_proj = p->reg("backbone.b_aspp.proj.0.weight", {C4, NBR * C4, 1, 1, 1});
  reg_unit(p, p->un[5]);
  for (int i = 0; i < NSE; ++i) {
    PSe& s = p->se[i];
    s.C = f << i;
    s.Hd = std::max(1, s.C / 16);
    s.lvl = i;
    const std::string n = "backbone.se" + std::to_string(i + 1) + ".fc.";
    s.w1 = p->reg(n + "0.weight", {s.Hd, s.C, 1, 1, 1});
    s.b1 = p->reg(n + "0.bias", {s.Hd});
    s.w2 = p->reg(n + "2.weight", {s.C, s.Hd, 1, 1, 1});
    s.b2 = p->reg(n + "2.bias", {s.C});
  }
  for (int u = 0; u < NUP; ++u) {
    UpConv& U = p->up[u];
    U.Cin = 16 * f >> u;
    U.Cout = 8 * f >> u;
    U.Llow = 4 - u;
    const std::string lv = std::to_string(4 - u);
    U.w = p->reg("backbone.up" + lv + ".weight", {U.Cin, U.Cout, 2, 2, 2});
    U.b = p->reg("backbone.up" + lv + ".bias", {U.Cout});
    if (u < NAG) {
      PAg& a = p->ag[u];
      a.C = U.Cout;
      a.I = a.C / 2;
      a.lvl = 3 - u;
      const std::string n = "backbone.ag" + lv + ".";
      a.wx = p->reg(n + "W_x.weight", {a.I, a.C, 1, 1, 1});
      a.bx = p->reg(n + "W_x.bias", {a.I});
      a.wg = p->reg(n + "W_g.weight", {a.I, a.C, 1, 1, 1});
      a.bg = p->reg(n + "W_g.bias", {a.I});
      a.wpsi = p->reg(n + "psi.weight", {1, a.I, 1, 1, 1});
      a.bpsi = p->reg(n + "psi.bias", {1});
    }
    reg_unit(p, p->un[6 + u]);
  }
  p->head_w = p->reg("head.weight", {p->K, f, 1, 1, 1});
  p->head_b = p->reg("head.bias", {p->K});

  // ---- workspace ----
  const Vol& v0 = p->vol[0];
  p->x_cl = p->alloc(nvox(v0) * p->ldx * sizeof(float));
  size_t red_ws = 0, red_out = 0, wg = 0, wt = 0;
  for (int i = 0; i < NUNIT; ++i) {
    PUnit& u = p->un[i];
    const Vol& v = p->vol[u.lvl];
    const int64_t M = nvox(v);
    const size_t act = M * u.C * sizeof(float);
    const size_t bc = (size_t)B * u.C * sizeof(float);
    u.y1 = p->alloc(act);
    u.a1 = p->alloc(act);
    u.y2 = p->alloc(act);
    u.out = p->alloc(act);
    u.s1 = stat_alloc(p, bc);
    u.s2 = stat_alloc(p, bc);
    const int kin = i == 0 ? p->ldx : u.Cin;
    if (u.skip) {
      u.pk_sk = p->alloc(head_pack_floats(kin, u.C) * sizeof(float));
      wg = std::max(wg, linear_wgrad_ws_bytes(M, u.Cin, u.C));
    }
    red_ws = std::max(red_ws, slab_reduce_ws_bytes(v, u.C, 2));
    red_out = std::max(red_out, (size_t)B * u.C * v.D * 2 * sizeof(float));
    wg = std::max(wg, conv3d_wgrad_ws_bytes(v, 3, u.Cin, u.C));
    wg = std::max(wg, conv3d_wgrad_ws_bytes(v, 3, u.C, u.C));
    wg = std::max(wg, conv3d_splitk_bytes(v, 3, u.Cin, u.C));
    wg = std::max(wg, conv3d_splitk_bytes(v, 3, u.C, u.C));
    wt = std::max(wt, conv3d_pack_bytes(3, u.Cin, u.C));
    wt = std::max(wt, conv3d_pack_bytes(3, u.C, u.C));
  }
  {  // ASPP
    const int64_t M = nvox(p->vol[4]);
    for (int r = 0; r < NBR; ++r) p->br_pk[r] = p->alloc((size_t)27 * C4 * C4 * sizeof(float));
    p->cat = p->alloc(M * NBR * C4 * sizeof(float));
    p->dcat = p->alloc(M * NBR * C4 * sizeof(float));
    p->proj_pk = p->alloc(head_pack_floats(NBR * C4, C4) * sizeof(float));
    p->aspp_out = p->alloc(M * C4 * sizeof(float));
    wg = std::max(wg, linear_wgrad_ws_bytes(M, NBR * C4, C4));
  }
  for (int i = 0; i < NSE; ++i) {
    PSe& s = p->se[i];
    const size_t bc = (size_t)B * s.C * sizeof(float);
    s.mean = p->alloc(bc);
    s.gate = p->alloc(bc);
    s.dmean = p->alloc(bc);
    s.hid = p->alloc((size_t)B * s.Hd * sizeof(float));
    s.out = p->alloc(nvox(p->vol[i]) * s.C * sizeof(float));
  }
  for (int i = 0; i < NAG; ++i) {
    PAg& a = p->ag[i];
    const int64_t M = nvox(p->vol[a.lvl]);
    a.wcat = p->alloc((size_t)a.I * 2 * a.C * sizeof(float));
    a.dwcat = p->alloc((size_t)a.I * 2 * a.C * sizeof(float));
    a.bcat = p->alloc((size_t)a.I * sizeof(float));
    a.dbcat = p->alloc((size_t)a.I * sizeof(float));
    a.pk = p->alloc(head_pack_floats(2 * a.C, a.I) * sizeof(float));
    a.att = p->alloc(M * a.I * sizeof(float));
    a.psi = p->alloc(M * sizeof(float));
    a.s = p->alloc(M * a.C * sizeof(float));
    wg = std::max(wg, linear_wgrad_ws_bytes(M, 2 * a.C, a.I));
  }
  p->ag_part = p->alloc((size_t)AG_NB * (4 * f + 1) * sizeof(float));
  for (int l = 0; l < 4; ++l) {
    const Vol& vl = p->vol[l + 1];
    const int C = f << l;
    p->pool[l] = p->alloc(nvox(vl) * C * sizeof(float));
    p->pidx[l] = p->alloc(nvox(vl) * C);
  }
  for (int u = 0; u < NUP; ++u) {
    UpConv& U = p->up[u];
    up_alloc(p, U);
    wg = std::max(wg, upconv_wgrad_ws_bytes(p->vol[U.Llow], U.Cin, U.Cout, UP_NS));
  }
  p->head_pk = p->alloc(head_pack_floats(f, p->K) * sizeof(float));
  wg = std::max(wg, head_wgrad_ws_bytes(nvox(v0), f, p->K));
  p->red_ws = p->alloc(red_ws);
  p->red_out = p->alloc(red_out);
  p->kk1 = p->alloc((size_t)B * 16 * f * sizeof(float));
  p->kk2 = p->alloc((size_t)B * 16 * f * sizeof(float));
  p->ones = p->alloc((size_t)B * 16 * f * sizeof(float));
  p->zeros = p->alloc((size_t)B * 16 * f * sizeof(float));
  p->wg_ws = p->alloc(wg);
  p->wt = p->alloc(wt);
  p->db_scr = p->alloc((size_t)16 * f * sizeof(float));
  size_t gmax = 0;  // max over levels of V_l * C_l
  for (int l = 0; l < NLVL; ++l)
    gmax = std::max(gmax, (size_t)nvox(p->vol[l]) * (size_t)(f << l) * sizeof(float));
  p->G_out = p->alloc(gmax);
  p->G_s = p->alloc(gmax);
  p->G_1 = p->alloc(gmax);
  p->G_2 = p->alloc(gmax);
  p->G_dx = p->alloc(gmax);
  p->G_ds = p->alloc(gmax);
  for (int l = 0; l < 4; ++l)
    p->dskip[l] = p->alloc(nvox(p->vol[l]) * (f << l) * sizeof(float));
  return SPFF_OK;
}

#define EW(kernel, work, ...)                                                              \
  do {                                                                                     \
    hipLaunchKernelGGL(kernel, dim3(ew_grid(work)), dim3(256), 0, p->st, __VA_ARGS__);     \
    PLAN_HIPCK(hipGetLastError());                                                         \
  } while (0)

int fwd_unit(spff_rupp* p, PUnit& u, const Src2& in, int kin) {
  const Vol& v = p->vol[u.lvl];
  const int C = u.C;
  const int64_t M = nvox(v);
  const float* sk = in.p0;  // identity skip: cin == C, one source with pitch C
  if (u.skip) {
    float* pk = p->F(u.pk_sk);
    PLAN_HIPCK(head_pack(p->P(u.wsk), pk, pk + head_pack_dgrad_offset(kin, C), u.Cin, C, p->st));
    PLAN_HIPCK(linear_fwd2(in, kin, pk, nullptr, p->F(p->G_s), C, C, M, p->st));
    sk = p->F(p->G_s);
  }
  PLAN_CK(conv_run(p, u.cv[0], false, in, dst1(p->F(u.y1), C), v));
  PLAN_CK(in_fwd(p, v, C, p->F(u.y1), u.s1, p->P(u.g1), p->P(u.b1)));
  PLAN_HIPCK(act_apply(p->F(u.y1), p->F(u.a1), p->F(u.s1.al), p->F(u.s1.de), nullptr, nullptr, v, C,
                   p->st, 0.f));
  PLAN_CK(conv_run(p, u.cv[1], false, src1(p->F(u.a1), C), dst1(p->F(u.y2), C), v));
  PLAN_CK(in_fwd(p, v, C, p->F(u.y2), u.s2, p->P(u.g2), p->P(u.b2)));
  EW(k_rupp_tail, M * C / 4, p->F(u.y2), p->F(u.s2.al), p->F(u.s2.de), sk, p->F(u.out),
     M * C / 4, C / 4, M / v.B);
  return SPFF_OK;
}

// dout -> parameter gradients and (dx != null) the input gradient, overwritten
int bwd_unit(spff_rupp* p, PUnit& u, const float* dout, const Dst2* dx, const Src2& in, int kin) {
  const Vol& v = p->vol[u.lvl];
  const int C = u.C, math = p->cfg.math;
  const int64_t M = nvox(v);
  float* dz = p->F(p->G_s);
  float* g1 = p->F(p->G_1);
  float* g2 = p->F(p->G_2);
  float* wgs = p->F(p->wg_ws);
  EW(k_rupp_mask, M * C / 4, dout, p->F(u.out), dz, M * C / 4);
  PLAN_CK(in_bwd(p, v, C, p->F(u.y2), dz, g1, u.s2, p->P(u.g2), p->DP(u.g2), p->DP(u.b2), 1.f));
  PLAN_HIPCK(conv3d_wgrad(src1(p->F(u.a1), C), g1, C, p->DP(u.cv[1].w), v, 3, C, C, math, wgs, p->st));
  PLAN_CK(conv_run(p, u.cv[1], true, src1(g1, C), dst1(g2, C), v));
  PLAN_CK(in_bwd(p, v, C, p->F(u.y1), g2, g2, u.s1, p->P(u.g1), p->DP(u.g1), p->DP(u.b1), 0.f));
  PLAN_HIPCK(conv3d_wgrad(in, g2, C, p->DP(u.cv[0].w), v, 3, u.Cin, C, math, wgs, p->st));
  if (dx) PLAN_CK(conv_run(p, u.cv[0], true, src1(g2, C), *dx, v));
  if (u.skip) {
    PLAN_HIPCK(linear_wgrad2(in, u.Cin, dz, C, C, p->DP(u.wsk), p->F(p->db_scr), M, wgs, p->st));
    if (dx)
      PLAN_HIPCK(linear_dgrad2(dz, C, C, p->F(u.pk_sk) + head_pack_dgrad_offset(kin, C), *dx, u.Cin,
                           M, 1, p->st));
  } else if (dx) {
    PLAN_HIPCK(accumulate(dx->p0, dz, M * C, 1.f, p->st));
  }
  return SPFF_OK;
}

int se_fwd(spff_rupp* p, PSe& s, const float* x) {
  const Vol& v = p->vol[s.lvl];
  const int64_t M = nvox(v);
  RedArgs a{};
  a.y = x;
  PLAN_HIPCK(slab_reduce(RED_SUM, a, v, s.C, p->F(p->red_out), p->F(p->red_ws), p->st));
  PLAN_HIPCK(in_mean(p->F(p->red_out), p->F(s.mean), v, s.C, p->st));
  hipLaunchKernelGGL(k_se_gate, dim3(v.B), dim3(256), s.Hd * sizeof(float), p->st, p->F(s.mean),
                     p->P(s.w1), p->P(s.b1), p->P(s.w2), p->P(s.b2), p->F(s.hid), p->F(s.gate),
                     s.C, s.Hd);
  PLAN_HIPCK(hipGetLastError());
  EW(k_se_scale, M * s.C / 4, x, p->F(s.gate), p->F(s.out), M * s.C / 4, s.C / 4, M / v.B);
  return SPFF_OK;
}

// g (the gradient at se(x), [V][C]) -> the gradient at x, in place; parameter gradients
int se_bwd(spff_rupp* p, PSe& s, const float* x, float* g) {
  const Vol& v = p->vol[s.lvl];
  const int64_t M = nvox(v);
  RedArgs a{};
  a.y = x; a.g = g; a.al = p->F(p->ones); a.de = p->F(p->zeros); a.neg = 1.f;
  PLAN_HIPCK(slab_reduce(RED_BWD_TAIL, a, v, s.C, p->F(p->red_out), p->F(p->red_ws), p->st));
  hipLaunchKernelGGL(k_se_bwd, dim3(1), dim3(256), (s.C + s.Hd) * sizeof(float), p->st,
                     p->F(p->red_out), p->F(s.mean), p->F(s.hid), p->F(s.gate), p->P(s.w1),
                     p->P(s.w2), p->DP(s.w1), p->DP(s.b1), p->DP(s.w2), p->DP(s.b2),
                     p->F(s.dmean), v.B, s.C, s.Hd, v.D, 1.f / (float)(M / v.B));
  PLAN_HIPCK(hipGetLastError());
  EW(k_se_bwd_apply, M * s.C / 4, g, p->F(s.gate), p->F(s.dmean), M * s.C / 4, s.C / 4, M / v.B);
  return SPFF_OK;
}

// the gate's tensors for the shared implementation (attn_gate.hip); the unit's backward is
// done with G_1 / G_2 when the gate's runs, so they hold its scratch
AttnGate ag_view(const spff_rupp* p, const PAg& a) {
  AttnGate g{};
  g.C = a.C; g.I = a.I; g.M = nvox(p->vol[a.lvl]);
  g.wx = p->P(a.wx); g.bx = p->P(a.bx); g.wg = p->P(a.wg); g.bg = p->P(a.bg);
  g.wpsi = p->P(a.wpsi); g.bpsi = p->P(a.bpsi);
  if (p->dprm) {
    g.dwx = p->DP(a.wx); g.dbx = p->DP(a.bx); g.dwg = p->DP(a.wg); g.dbg = p->DP(a.bg);
    g.dwpsi = p->DP(a.wpsi); g.dbpsi = p->DP(a.bpsi);
  }
  g.wcat = p->F(a.wcat); g.bcat = p->F(a.bcat); g.pk = p->F(a.pk); g.att = p->F(a.att);
  g.psi = p->F(a.psi); g.s = p->F(a.s); g.dwcat = p->F(a.dwcat); g.dbcat = p->F(a.dbcat);
  g.dhid = p->F(p->G_1); g.dpp = p->F(p->G_2); g.part = p->F(p->ag_part);
  g.wgs = p->F(p->wg_ws);
  return g;
}

int ag_fwd(spff_rupp* p, PAg& a, const float* u, const float* g) {
  PLAN_HIPCK(attn_gate_fwd(ag_view(p, a), u, g, p->st));
  return SPFF_OK;
}

// ds (the gradient at s = u psi) -> du += (its share), dg (written), parameter gradients
int ag_bwd(spff_rupp* p, PAg& a, const float* u, const float* g, const float* ds, float* du,
           float* dg) {
  PLAN_HIPCK(attn_gate_bwd(ag_view(p, a), u, g, ds, du, dg, p->st));
  return SPFF_OK;
}

int forward(spff_rupp* p, const float* x, float* logits) {
  const spff_rupp_cfg& c = p->cfg;
  const int f = p->f, C4 = 16 * f;
  const Vol& v0 = p->vol[0];
  const Vol& v4 = p->vol[4];
  const int64_t M4 = nvox(v4);
  PLAN_HIPCK(ncdhw_to_ndhwc(x, p->F(p->x_cl), v0, c.in_ch, p->ldx, p->st));
  PLAN_HIPCK(fill32_async(p->F(p->ones), (size_t)c.batch * C4 * sizeof(float), 0x3f800000u, p->st));
  PLAN_HIPCK(spff::zero_async(p->F(p->zeros), (size_t)c.batch * C4 * sizeof(float), p->st));
  PUnit* U = p->un;
  Src2 in = src1(p->F(p->x_cl), p->ldx);
  int kin = p->ldx;
  for (int l = 0; l < 4; ++l) {
    PLAN_CK(fwd_unit(p, U[l], in, kin));
    PLAN_HIPCK(maxpool3_fwd(p->F(U[l].out), p->F(p->pool[l]),
                        reinterpret_cast<uint8_t*>(p->ws + p->pidx[l]), p->vol[l], f << l, p->st));
    PLAN_CK(se_fwd(p, p->se[l], p->F(U[l].out)));
    in = src1(p->F(p->pool[l]), f << l);
    kin = f << l;
  }
  PLAN_CK(fwd_unit(p, U[4], in, kin));
  for (int r = 0; r < NBR; ++r) {
    PLAN_HIPCK(dil_pack(p->P(p->w_br[r]), p->F(p->br_pk[r]), C4, C4, p->st));
    PLAN_HIPCK(dil_run(p->F(U[4].out), C4, p->F(p->br_pk[r]), p->F(p->cat) + r * C4, NBR * C4, v4, C4,
                   C4, DIL[r], false, 0, p->st));
  }
  {
    float* pk = p->F(p->proj_pk);
    PLAN_HIPCK(head_pack(p->P(p->w_proj), pk, pk + head_pack_dgrad_offset(NBR * C4, C4), NBR * C4, C4,
                     p->st));
    PLAN_HIPCK(linear_fwd(p->F(p->cat), NBR * C4, NBR * C4, pk, nullptr, p->F(p->aspp_out), C4, C4,
                      M4, nullptr, 0, p->st));
    EW(k_rupp_relu, M4 * C4 / 4, p->F(p->aspp_out), M4 * C4 / 4);
  }
  PLAN_CK(fwd_unit(p, U[5], src1(p->F(p->aspp_out), C4), C4));
  const float* prev = p->F(U[5].out);
  for (int u = 0; u < NUP; ++u) {
    UpConv& Up = p->up[u];
    const int lvl = 3 - u, C = Up.Cout;
    PLAN_CK(up_fwd(p, Up, prev, p->P(Up.b), p->cfg.math));
    const float* second = p->F(p->se[lvl].out);
    if (u < NAG) {
      PLAN_CK(ag_fwd(p, p->ag[u], p->F(Up.out), p->F(p->se[lvl].out)));
      second = p->F(p->ag[u].s);
    }
    PUnit& d = U[6 + u];
    PLAN_CK(fwd_unit(p, d, Src2{p->F(Up.out), second, C, C, C}, 2 * C));
    prev = p->F(d.out);
  }
  return head_fwd_packed(p, p->head_w, p->head_b, prev, logits);
}

int backward(spff_rupp* p, const float* dl) {
  const int f = p->f, C4 = 16 * f;
  const Vol& v4 = p->vol[4];
  const int64_t M4 = nvox(v4);
  PUnit* U = p->un;
  float* wgs = p->F(p->wg_ws);
  PLAN_CK(head_bwd(p, p->head_w, p->head_b, p->F(U[9].out), dl, p->F(p->G_out)));
  for (int lvl = 0; lvl < 4; ++lvl) {  // d1 <- up1 <- d2 ... <- up4
    const int u = 3 - lvl;
    PUnit& d = U[6 + u];
    UpConv& Up = p->up[u];
    const int C = d.C;
    const bool gated = u < NAG;
    const float* second = gated ? p->F(p->ag[u].s) : p->F(p->se[lvl].out);
    // [u | s]: the gradient of u into G_dx; of s into G_ds (gated) or straight into the
    // SE output's gradient
    Dst2 dx{p->F(p->G_dx), gated ? p->F(p->G_ds) : p->F(p->dskip[lvl]), C, C, C};
    PLAN_CK(bwd_unit(p, d, p->F(p->G_out), &dx, Src2{p->F(Up.out), second, C, C, C}, 2 * C));
    if (gated)
      PLAN_CK(ag_bwd(p, p->ag[u], p->F(Up.out), p->F(p->se[lvl].out), p->F(p->G_ds), p->F(p->G_dx),
                 p->F(p->dskip[lvl])));
    PLAN_CK(se_bwd(p, p->se[lvl], p->F(U[lvl].out), p->F(p->dskip[lvl])));
    const float* below = u == 0 ? p->F(U[5].out) : p->F(U[6 + u - 1].out);
    PLAN_CK(up_bwd(p, Up, below, p->F(p->G_dx), p->DP(Up.b), p->F(p->G_out), p->cfg.math));
  }
  {  // bottleneck
    Dst2 dx = dst1(p->F(p->G_dx), C4);
    PLAN_CK(bwd_unit(p, U[5], p->F(p->G_out), &dx, src1(p->F(p->aspp_out), C4), C4));
    float* dz = p->F(p->G_s);
    EW(k_rupp_mask, M4 * C4 / 4, p->F(p->G_dx), p->F(p->aspp_out), dz, M4 * C4 / 4);
    PLAN_HIPCK(linear_wgrad(p->F(p->cat), NBR * C4, NBR * C4, dz, C4, C4, p->DP(p->w_proj),
                        p->F(p->db_scr), M4, wgs, p->st));
    PLAN_HIPCK(linear_dgrad(dz, C4, C4, p->F(p->proj_pk) + head_pack_dgrad_offset(NBR * C4, C4),
                        p->F(p->dcat), NBR * C4, NBR * C4, M4, nullptr, p->st));
    for (int r = 0; r < NBR; ++r) {  // input gradients summed in branch order 0..3
      const float* dy = p->F(p->dcat) + r * C4;
      PLAN_HIPCK(dil_wgrad(p->F(U[4].out), C4, dy, NBR * C4, p->DP(p->w_br[r]), v4, C4, C4, DIL[r],
                       p->st));
      PLAN_HIPCK(dil_run(dy, NBR * C4, p->F(p->br_pk[r]), p->F(p->G_out), C4, v4, C4, C4, DIL[r], true,
                     r > 0, p->st));
    }
    Dst2 dxi = dst1(p->F(p->G_dx), 8 * f);
    PLAN_CK(bwd_unit(p, U[4], p->F(p->G_out), &dxi, src1(p->F(p->pool[3]), 8 * f), 8 * f));
  }
  for (int l = 3; l >= 0; --l) {
    const int C = f << l;
    PLAN_HIPCK(maxpool3_bwd_add(p->F(p->G_dx), reinterpret_cast<const uint8_t*>(p->ws + p->pidx[l]),
                            p->F(p->dskip[l]), C, p->F(p->dskip[l]), p->vol[l], C, p->st));
    if (l > 0) {
      Dst2 dx = dst1(p->F(p->G_dx), C / 2);
      PLAN_CK(bwd_unit(p, U[l], p->F(p->dskip[l]), &dx, src1(p->F(p->pool[l - 1]), C / 2), C / 2));
    } else {
      PLAN_CK(bwd_unit(p, U[0], p->F(p->dskip[0]), nullptr, src1(p->F(p->x_cl), p->ldx), p->ldx));
    }
  }
  return SPFF_OK;
}

int dil_args(int ldx, int ldy, int B, int D, int H, int W, int cin, int cout, int r) {
  if (B < 1 || D < 1 || H < 1 || W < 1) return plan_fail(SPFF_EINVAL, "invalid B / D / H / W");
  if (cin < 4 || cout < 4 || cin % 4 || cout % 4)
    return plan_fail(SPFF_EINVAL, "cin and cout must be multiples of 4");
  if (ldx % 4 || ldx < cin || ldy % 4 || ldy < cout)
    return plan_fail(SPFF_EINVAL, "ldx / ldy must be multiples of 4 covering cin / cout");
  if (r != 1 && r != 2 && r != 4 && r != 8) return plan_fail(SPFF_EINVAL, "dilation must be 1, 2, 4 or 8");
  return SPFF_OK;
}

}  // namespace

// =================================================================== C ABI ==
extern "C" {

int spff_rupp_create(const spff_rupp_cfg* cfg, spff_rupp** out) {
  return plan_create(cfg, out, build);
}

void spff_rupp_destroy(spff_rupp* p) { delete p; }

int spff_rupp_num_params(const spff_rupp* p) { return p ? (int)p->params.size() : 0; }

int spff_rupp_param_info(const spff_rupp* p, int i, const char** name, int* ndim, int64_t shape[5],
                         int64_t* offset, int64_t* numel) {
  if (!p) return plan_fail(SPFF_EINVAL, "param index");
  return plan_param_info(p->params, i, name, ndim, shape, offset, numel);
}

int64_t spff_rupp_param_floats(const spff_rupp* p) { return p ? p->nparam : 0; }
size_t spff_rupp_workspace_bytes(const spff_rupp* p) { return p ? p->total : 0; }

int spff_rupp_forward(spff_rupp* p, const float* x, const float* params, float* logits, void* ws,
                      void* stream) {
  if (!p || !x || !params || !logits || !ws) return plan_fail(SPFF_EINVAL, "null argument");
  p->bind(ws, params, nullptr, stream);
  return forward(p, x, logits);
}

int spff_rupp_backward(spff_rupp* p, const float* dlogits, const float* params, float* dparams,
                       void* ws, void* stream) {
  if (!p || !dlogits || !params || !dparams || !ws) return plan_fail(SPFF_EINVAL, "null argument");
  p->bind(ws, params, dparams, stream);
  return backward(p, dlogits);
}

int spff_rupp_saved_tensor(const spff_rupp* p, void* ws, const char* name, const float** ptr,
                           int64_t* nv, int* ch) {
  if (!p || !ws || !name || !ptr) return plan_fail(SPFF_EINVAL, "null argument");
  const std::string n(name);
  const SavedOut ret{ws, ptr, nv, ch};
  for (int i = 0; i < NUNIT; ++i) {
    const PUnit& u = p->un[i];
    const Vol& v = p->vol[u.lvl];
    if (n == u.name + ".a1") return ret(u.a1, v, u.C);
    if (n == u.name + ".out") return ret(u.out, v, u.C);
  }
  if (n == "b_aspp.out") return ret(p->aspp_out, p->vol[4], 16 * p->f);
  for (int i = 0; i < NAG; ++i)
    if (n == "ag" + std::to_string(4 - i) + ".att")
      return ret(p->ag[i].att, p->vol[p->ag[i].lvl], p->ag[i].I);
  return plan_fail(SPFF_EINVAL, "unknown saved tensor " + n);
}

size_t spff_rupp_loss_ws_bytes(int batch, int num_classes) {
  return dice_ce_ws_bytes(batch, num_classes);
}

int spff_rupp_loss(const float* logits, const int64_t* labels, int batch, int64_t vox_per_sample,
                   int num_classes, int use_ignore, int ignore_index, int include_bg,
                   double ce_weight, double dice_weight, float* out4, float* dlogits, void* ws,
                   void* stream) {
  if (!logits || !labels || !out4 || !dlogits || !ws) return plan_fail(SPFF_EINVAL, "null argument");
  if (batch < 1 || vox_per_sample < 1) return plan_fail(SPFF_EINVAL, "invalid batch / vox_per_sample");
  if (num_classes < 2 || num_classes > 32) return plan_fail(SPFF_EINVAL, "num_classes must be 2..32");
  PLAN_HIPCK(soft_dice_loss({DICE_RUPP, include_bg ? 0 : 1, ce_weight, dice_weight}, logits, labels,
                        batch, vox_per_sample, num_classes, use_ignore, ignore_index, out4, dlogits,
                        ws, static_cast<hipStream_t>(stream)));
  return SPFF_OK;
}

size_t spff_conv3d_dil_ws_bytes(int cin, int cout) {
  return (size_t)27 * std::max(cin, 0) * std::max(cout, 0) * sizeof(float) + 256;
}

int spff_conv3d_dil_fwd(const float* x, int ldx, const float* w, float* y, int ldy, int B, int D,
                        int H, int W, int cin, int cout, int dilation, void* ws, void* stream) {
  if (!x || !w || !y || !ws) return plan_fail(SPFF_EINVAL, "null argument");
  PLAN_CK(dil_args(ldx, ldy, B, D, H, W, cin, cout, dilation));
  hipStream_t s = static_cast<hipStream_t>(stream);
  float* P = static_cast<float*>(ws);
  PLAN_HIPCK(dil_pack(w, P, cin, cout, s));
  PLAN_HIPCK(dil_run(x, ldx, P, y, ldy, Vol{B, D, H, W}, cin, cout, dilation, false, 0, s));
  return SPFF_OK;
}

int spff_conv3d_dil_dgrad(const float* dy, int ldy, const float* w, float* dx, int ldx, int B,
                          int D, int H, int W, int cin, int cout, int dilation, int accumulate,
                          void* ws, void* stream) {
  if (!dy || !w || !dx || !ws) return plan_fail(SPFF_EINVAL, "null argument");
  PLAN_CK(dil_args(ldx, ldy, B, D, H, W, cin, cout, dilation));
  hipStream_t s = static_cast<hipStream_t>(stream);
  float* P = static_cast<float*>(ws);
  PLAN_HIPCK(dil_pack(w, P, cin, cout, s));
  PLAN_HIPCK(dil_run(dy, ldy, P, dx, ldx, Vol{B, D, H, W}, cin, cout, dilation, true,
                 accumulate ? 1 : 0, s));
  return SPFF_OK;
}

int spff_conv3d_dil_wgrad(const float* x, int ldx, const float* dy, int ldy, float* dw, int B,
                          int D, int H, int W, int cin, int cout, int dilation, void* ws,
                          void* stream) {
  if (!x || !dy || !dw) return plan_fail(SPFF_EINVAL, "null argument");
  (void)ws;
  PLAN_CK(dil_args(ldx, ldy, B, D, H, W, cin, cout, dilation));
  PLAN_HIPCK(dil_wgrad(x, ldx, dy, ldy, dw, Vol{B, D, H, W}, cin, cout, dilation,
                   static_cast<hipStream_t>(stream)));
  return SPFF_OK;
}

}  // extern "C"
