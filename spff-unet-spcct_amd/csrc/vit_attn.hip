// Global multi-head self-attention of a ViT block (UNETR): every token attends to all n
// tokens of its sample, heads of hd in {16, 32, 64} channels, no bias table, n <= 512.
//
//   S = scale Q K^T, P = softmax(S) over the n keys, O = P V;  lse = log sum exp(S)
//   backward: D_i = dO_i . O_i, P recomputed from lse, dS = P (dO V^T - D),
//             dQ = scale dS K, dK = scale dS^T Q, dV = P^T dO
//
// Arithmetic: the fp32-input MFMA (v_mfma_f32_16x16x4_f32), whose result is bit for bit a
// k-ordered fmaf chain, so every product is exact fp32 with no operand split.  One
// workgroup (4 waves) owns a (sample, head, 64-row tile); a wave owns 16 rows.  The
// products are taken transposed (S^T = K Q^T: keys on the accumulator rows, the query on
// the lane), so the softmax statistics of a query are one value per lane, and P^T / dS^T
// leave the accumulator already laid out as the B operand of the next product (k = key)
// with no trip through LDS.  The other side of each product (K and V for the forward and
// dQ, Q and dO for dK / dV) sits in LDS in chunks of 256 rows: a 216-token head is one
// chunk, loaded once.  The forward takes two sweeps (row maximum, then exp / sum / PV), so
// P is exp(s - max) of the final maximum as in a plain softmax, with no rescaling.
// Every sum has a fixed order (key tiles, then the four lane groups); no atomics.
#include "swin_internal.h"
#include "spff.h"

#include <cmath>

namespace spff {

namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int VA_KC = 256;       // LDS chunk: rows of K / V (or Q / dO)
constexpr int VA_ROWS = 64;      // rows per workgroup = 4 waves x 16
constexpr int VA_THREADS = 256;

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// rows [r0, r0 + rows) of src [n][ld] (HD columns from src) -> dst [rows][stride]; rows
// beyond n are zero
template <int HD>
__device__ __forceinline__ void fill_rows(float* dst, int stride, const float* __restrict__ src,
                                          int64_t ld, int r0, int n, int rows) {
  constexpr int V4 = HD / 4;
  for (int i = threadIdx.x; i < rows * V4; i += VA_THREADS) {
    const int r = i / V4, c = (i % V4) * 4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r0 + r < n) v = *reinterpret_cast<const float4*>(src + (int64_t)(r0 + r) * ld + c);
    float* d = dst + r * stride + c;
    d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
  }
}

__device__ __forceinline__ int chunk_rows(int n, int r0) {
  const int left = (n - r0 + 15) & ~15;
  return left < VA_KC ? left : VA_KC;
}

// LDS row strides: the [row = lane & 15][k = lane >> 4] operand read is conflict-free at
// stride = 2 mod 32 words, the [row = 4 (lane >> 4) + r][col = lane & 15] read at 4 mod 8
template <int HD>
__global__ __launch_bounds__(VA_THREADS) void k_vit_attn_fwd(const float* __restrict__ qkv,
                                                             float* __restrict__ O,
                                                             float* __restrict__ lse, int n, int C,
                                                             int nh, float scale) {
  constexpr int SK = HD + 2, SV = HD + 4, NS = HD / 4, ND = HD / 16;
  __shared__ float sK[VA_KC * SK];
  __shared__ float sV[VA_KC * SV];
  const int b = blockIdx.z, h = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  const int qrow = blockIdx.x * VA_ROWS + wave * 16 + lr;
  const int64_t ld = 3 * (int64_t)C;
  const float* base = qkv + (int64_t)b * n * ld + h * HD;
  float qr[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) qr[s] = qrow < n ? base[(int64_t)qrow * ld + 4 * s + lg] : 0.f;
  const int nch = (n + VA_KC - 1) / VA_KC;
  float m = -INFINITY, lsum = 0.f;
  f32x4 oacc[ND];
#pragma unroll
  for (int d = 0; d < ND; ++d) oacc[d] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int sweep = 0; sweep < 2; ++sweep) {
    for (int ch = 0; ch < nch; ++ch) {
      const int k0 = ch * VA_KC;
      const int rows = chunk_rows(n, k0);
      if (nch > 1 || sweep == 0) {
        __syncthreads();
        fill_rows<HD>(sK, SK, base + C, ld, k0, n, rows);
        fill_rows<HD>(sV, SV, base + 2 * C, ld, k0, n, rows);
        __syncthreads();
      }
      for (int jt = 0; jt < rows; jt += 16) {
        f32x4 acc{0.f, 0.f, 0.f, 0.f};
        const float* kp = sK + (jt + lr) * SK + lg;
#pragma unroll
        for (int s = 0; s < NS; ++s) acc = mfma4(kp[4 * s], qr[s], acc);
        // acc[r] = S^T[key jt + 4 lg + r][query lr]
        const int key = k0 + jt + 4 * lg;
        if (sweep == 0) {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (key + r < n) m = fmaxf(m, acc[r] * scale);
        } else {
          float p[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            p[r] = key + r < n ? expf(acc[r] * scale - m) : 0.f;
            lsum += p[r];
          }
          const float* vp = sV + (jt + 4 * lg) * SV + lr;
#pragma unroll
          for (int d = 0; d < ND; ++d)
#pragma unroll
            for (int r = 0; r < 4; ++r) oacc[d] = mfma4(vp[r * SV + 16 * d], p[r], oacc[d]);
        }
      }
    }
    if (sweep == 0) {
      m = fmaxf(m, __shfl_xor(m, 16));
      m = fmaxf(m, __shfl_xor(m, 32));
    }
  }
  lsum += __shfl_xor(lsum, 16);
  lsum += __shfl_xor(lsum, 32);
  if (qrow < n) {
    // oacc[d][r] = sum_j P V [query lr][channel 16 d + 4 lg + r]
    float* op = O + ((int64_t)b * n + qrow) * C + h * HD + 4 * lg;
#pragma unroll
    for (int d = 0; d < ND; ++d)
      *reinterpret_cast<float4*>(op + 16 * d) = make_float4(
          oacc[d][0] / lsum, oacc[d][1] / lsum, oacc[d][2] / lsum, oacc[d][3] / lsum);
    if (lg == 0) lse[((int64_t)b * nh + h) * n + qrow] = m + logf(lsum);
  }
}

// D [B][nh][n] = dO . O over the head's channels, in channel order
__global__ void k_vit_attn_dot(const float* __restrict__ O, const float* __restrict__ dO,
                               float* __restrict__ D, int B, int n, int C, int nh, int hd) {
  const int64_t total = (int64_t)B * nh * n;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int q = (int)(i % n);
    const int h = (int)((i / n) % nh);
    const int64_t b = i / ((int64_t)n * nh);
    const int64_t o = (b * n + q) * C + h * hd;
    float acc = 0.f;
    for (int d = 0; d < hd; ++d) acc = fmaf(dO[o + d], O[o + d], acc);
    D[i] = acc;
  }
}

// dQ: as the forward, one sweep (P from lse); K is read both ways, V as the first operand
template <int HD>
__global__ __launch_bounds__(VA_THREADS) void k_vit_attn_bwd_q(
    const float* __restrict__ qkv, const float* __restrict__ dO, const float* __restrict__ lse,
    const float* __restrict__ D, float* __restrict__ dqkv, int n, int C, int nh, float scale) {
  constexpr int SK = HD + 4, SV = HD + 2, NS = HD / 4, ND = HD / 16;
  __shared__ float sK[VA_KC * SK];
  __shared__ float sV[VA_KC * SV];
  const int b = blockIdx.z, h = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  const int qrow = blockIdx.x * VA_ROWS + wave * 16 + lr;
  const int64_t ld = 3 * (int64_t)C;
  const float* base = qkv + (int64_t)b * n * ld + h * HD;
  const float* dob = dO + (int64_t)b * n * C + h * HD;
  float qr[NS], gr[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    qr[s] = qrow < n ? base[(int64_t)qrow * ld + 4 * s + lg] : 0.f;
    gr[s] = qrow < n ? dob[(int64_t)qrow * C + 4 * s + lg] : 0.f;
  }
  const int64_t si = ((int64_t)b * nh + h) * n + qrow;
  const float lq = qrow < n ? lse[si] : 0.f;
  const float dq = qrow < n ? D[si] : 0.f;
  f32x4 acc_q[ND];
#pragma unroll
  for (int d = 0; d < ND; ++d) acc_q[d] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int nch = (n + VA_KC - 1) / VA_KC;
  for (int ch = 0; ch < nch; ++ch) {
    const int k0 = ch * VA_KC;
    const int rows = chunk_rows(n, k0);
    __syncthreads();
    fill_rows<HD>(sK, SK, base + C, ld, k0, n, rows);
    fill_rows<HD>(sV, SV, base + 2 * C, ld, k0, n, rows);
    __syncthreads();
    for (int jt = 0; jt < rows; jt += 16) {
      f32x4 as{0.f, 0.f, 0.f, 0.f}, ap{0.f, 0.f, 0.f, 0.f};
      const float* kp = sK + (jt + lr) * SK + lg;
      const float* vp = sV + (jt + lr) * SV + lg;
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        as = mfma4(kp[4 * s], qr[s], as);
        ap = mfma4(vp[4 * s], gr[s], ap);
      }
      const int key = k0 + jt + 4 * lg;
      float ds[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = (key + r < n && qrow < n) ? expf(as[r] * scale - lq) : 0.f;
        ds[r] = p * (ap[r] - dq);
      }
      const float* kt = sK + (jt + 4 * lg) * SK + lr;
#pragma unroll
      for (int d = 0; d < ND; ++d)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc_q[d] = mfma4(kt[r * SK + 16 * d], ds[r], acc_q[d]);
    }
  }
  if (qrow < n) {
    float* op = dqkv + ((int64_t)b * n + qrow) * ld + h * HD + 4 * lg;
#pragma unroll
    for (int d = 0; d < ND; ++d)
      *reinterpret_cast<float4*>(op + 16 * d) = make_float4(
          acc_q[d][0] * scale, acc_q[d][1] * scale, acc_q[d][2] * scale, acc_q[d][3] * scale);
  }
}

// dK, dV: a wave owns 16 keys (K, V rows in registers), the queries' Q, dO, lse and D pass
// through LDS in chunks; queries are summed in ascending order
template <int HD>
__global__ __launch_bounds__(VA_THREADS) void k_vit_attn_bwd_kv(
    const float* __restrict__ qkv, const float* __restrict__ dO, const float* __restrict__ lse,
    const float* __restrict__ D, float* __restrict__ dqkv, int n, int C, int nh, float scale) {
  constexpr int SQ = HD + 4, NS = HD / 4, ND = HD / 16;
  __shared__ float sQ[VA_KC * SQ];
  __shared__ float sG[VA_KC * SQ];
  __shared__ float sL[VA_KC];
  __shared__ float sD[VA_KC];
  const int b = blockIdx.z, h = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  const int krow = blockIdx.x * VA_ROWS + wave * 16 + lr;
  const int64_t ld = 3 * (int64_t)C;
  const float* base = qkv + (int64_t)b * n * ld + h * HD;
  const float* dob = dO + (int64_t)b * n * C + h * HD;
  const int64_t sb = ((int64_t)b * nh + h) * n;
  float kr[NS], vr[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    kr[s] = krow < n ? base[(int64_t)krow * ld + C + 4 * s + lg] : 0.f;
    vr[s] = krow < n ? base[(int64_t)krow * ld + 2 * C + 4 * s + lg] : 0.f;
  }
  f32x4 acc_k[ND], acc_v[ND];
#pragma unroll
  for (int d = 0; d < ND; ++d) {
    acc_k[d] = f32x4{0.f, 0.f, 0.f, 0.f};
    acc_v[d] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const int nch = (n + VA_KC - 1) / VA_KC;
  for (int ch = 0; ch < nch; ++ch) {
    const int i0 = ch * VA_KC;
    const int rows = chunk_rows(n, i0);
    __syncthreads();
    fill_rows<HD>(sQ, SQ, base, ld, i0, n, rows);
    fill_rows<HD>(sG, SQ, dob, C, i0, n, rows);
    for (int i = threadIdx.x; i < rows; i += VA_THREADS) {
      sL[i] = i0 + i < n ? lse[sb + i0 + i] : 0.f;
      sD[i] = i0 + i < n ? D[sb + i0 + i] : 0.f;
    }
    __syncthreads();
    for (int it = 0; it < rows; it += 16) {
      f32x4 as{0.f, 0.f, 0.f, 0.f}, ap{0.f, 0.f, 0.f, 0.f};
      const float* qp = sQ + (it + lr) * SQ + lg;
      const float* gp = sG + (it + lr) * SQ + lg;
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        as = mfma4(qp[4 * s], kr[s], as);
        ap = mfma4(gp[4 * s], vr[s], ap);
      }
      // as[r] = S[query it + 4 lg + r][key lr]
      const int qi = it + 4 * lg;
      float p[4], ds[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        p[r] = (i0 + qi + r < n && krow < n) ? expf(as[r] * scale - sL[qi + r]) : 0.f;
        ds[r] = p[r] * (ap[r] - sD[qi + r]);
      }
      const float* qt = sQ + qi * SQ + lr;
      const float* gt = sG + qi * SQ + lr;
#pragma unroll
      for (int d = 0; d < ND; ++d)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          acc_v[d] = mfma4(gt[r * SQ + 16 * d], p[r], acc_v[d]);
          acc_k[d] = mfma4(qt[r * SQ + 16 * d], ds[r], acc_k[d]);
        }
    }
  }
  if (krow < n) {
    float* op = dqkv + ((int64_t)b * n + krow) * ld + h * HD + 4 * lg;
#pragma unroll
    for (int d = 0; d < ND; ++d) {
      *reinterpret_cast<float4*>(op + C + 16 * d) = make_float4(
          acc_k[d][0] * scale, acc_k[d][1] * scale, acc_k[d][2] * scale, acc_k[d][3] * scale);
      *reinterpret_cast<float4*>(op + 2 * C + 16 * d) =
          make_float4(acc_v[d][0], acc_v[d][1], acc_v[d][2], acc_v[d][3]);
    }
  }
}

}  // namespace

const char* vit_geo_check(int B, int n, int C, int nh) {
  if (B < 1 || n < 1 || C < 1 || nh < 1)
    return "ViT attention: batch, tokens, hidden and heads must be positive";
  if (C % nh) return "ViT attention: hidden must be a multiple of heads";
  const int hd = C / nh;
  if (hd != 16 && hd != 32 && hd != 64) return "ViT attention: head width must be 16, 32 or 64";
  if (n > 512) return "ViT attention: at most 512 tokens";
  if (B > 65535 || nh > 65535) return "ViT attention: batch and heads must stay below 65536";
  return nullptr;
}

VitGeo vit_geo(int B, int n, int C, int nh) {
  VitGeo g{};
  g.B = B; g.n = n; g.C = C; g.nh = nh;
  g.hd = nh > 0 ? C / nh : 0;
  g.scale = g.hd > 0 ? (float)std::pow((double)g.hd, -0.5) : 0.f;
  return g;
}

size_t vit_attn_ws_bytes(const VitGeo& g) { return (size_t)g.B * g.nh * g.n * sizeof(float); }

#define SPFF_VIT_HD(X) X(16) X(32) X(64)

hipError_t vit_attn_fwd(const float* qkv, const VitGeo& g, float* O, float* lse, hipStream_t s) {
  if (vit_geo_check(g.B, g.n, g.C, g.nh)) return hipErrorInvalidValue;
  const dim3 grid((g.n + VA_ROWS - 1) / VA_ROWS, g.nh, g.B);
  switch (g.hd) {
#define X(HD)                                                                                  \
  case HD:                                                                                     \
    hipLaunchKernelGGL(k_vit_attn_fwd<HD>, grid, dim3(VA_THREADS), 0, s, qkv, O, lse, g.n, g.C, \
                       g.nh, g.scale);                                                         \
    break;
    SPFF_VIT_HD(X)
#undef X
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t vit_attn_bwd(const float* qkv, const float* O, const float* dO, const float* lse,
                        const VitGeo& g, float* dqkv, float* ws, hipStream_t s) {
  if (vit_geo_check(g.B, g.n, g.C, g.nh)) return hipErrorInvalidValue;
  const int64_t rows = (int64_t)g.B * g.nh * g.n;
  hipLaunchKernelGGL(k_vit_attn_dot, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, O, dO,
                     ws, g.B, g.n, g.C, g.nh, g.hd);
  const dim3 grid((g.n + VA_ROWS - 1) / VA_ROWS, g.nh, g.B);
  switch (g.hd) {
#define X(HD)                                                                                   \
  case HD:                                                                                      \
    hipLaunchKernelGGL(k_vit_attn_bwd_q<HD>, grid, dim3(VA_THREADS), 0, s, qkv, dO, lse, ws,    \
                       dqkv, g.n, g.C, g.nh, g.scale);                                          \
    hipLaunchKernelGGL(k_vit_attn_bwd_kv<HD>, grid, dim3(VA_THREADS), 0, s, qkv, dO, lse, ws,   \
                       dqkv, g.n, g.C, g.nh, g.scale);                                          \
    break;
    SPFF_VIT_HD(X)
#undef X
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace spff

// =================================================================== C ABI ==
using namespace spff;

extern "C" {

size_t spff_vit_attn_ws_bytes(int batch, int tokens, int heads) {
  if (batch < 1 || tokens < 1 || heads < 1) return 0;
  return (size_t)batch * heads * tokens * sizeof(float);
}

int spff_vit_attn_fwd(const float* qkv, int batch, int tokens, int hidden, int heads, float* out,
                      float* lse, void* stream) {
  if (const char* m = vit_geo_check(batch, tokens, hidden, heads)) return set_error(SPFF_EINVAL, m);
  if (!qkv || !out || !lse) return set_error(SPFF_EINVAL, "spff_vit_attn_fwd: null argument");
  const hipError_t e = vit_attn_fwd(qkv, vit_geo(batch, tokens, hidden, heads), out, lse,
                                    static_cast<hipStream_t>(stream));
  return e == hipSuccess ? SPFF_OK : set_error(SPFF_EHIP, hipGetErrorString(e));
}

int spff_vit_attn_bwd(const float* qkv, const float* out, const float* dout, const float* lse,
                      int batch, int tokens, int hidden, int heads, float* dqkv, void* ws,
                      void* stream) {
  if (const char* m = vit_geo_check(batch, tokens, hidden, heads)) return set_error(SPFF_EINVAL, m);
  if (!qkv || !out || !dout || !lse || !dqkv || !ws)
    return set_error(SPFF_EINVAL, "spff_vit_attn_bwd: null argument");
  const hipError_t e = vit_attn_bwd(qkv, out, dout, lse, vit_geo(batch, tokens, hidden, heads),
                                    dqkv, static_cast<float*>(ws),
                                    static_cast<hipStream_t>(stream));
  return e == hipSuccess ? SPFF_OK : set_error(SPFF_EHIP, hipGetErrorString(e));
}

}  // extern "C"
