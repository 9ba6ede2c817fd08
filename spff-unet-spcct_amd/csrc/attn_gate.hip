// The attention gate of the gated skips (reference AttentionGate / AttentionGate3d), shared by
// the ResUNet++ plan and the SPFF plan's use_skip_gate:
//   s = u psi,  psi = sigmoid(w_psi . relu(W_x u + W_g g + b_x + b_g) + b_psi)
// on channel-last rows u, g [M][C]: the gate multiplies its FIRST argument (the up-conv
// output), the second reaches the result only through the hidden row.  The hidden row is
// one GEMM over the two-source view [u | g] with [W_x | W_g] and bias b_x + b_g (linear_*);
// the kernels here do the per-voxel rest.  Every sum has a fixed order.
#include "spff_internal.h"

#include <algorithm>

namespace spff {

namespace {

unsigned ew_grid(int64_t work) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>((work + 255) / 256, 8192));
}

// wcat [I][2C] = [W_x | W_g], bcat = b_x + b_g
__global__ __launch_bounds__(256) void k_ag_cat(const float* __restrict__ wx,
                                                const float* __restrict__ wg,
                                                const float* __restrict__ bx,
                                                const float* __restrict__ bg,
                                                float* __restrict__ wcat, float* __restrict__ bcat,
                                                int I, int C) {
  const int n = I * 2 * C;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int j = i / (2 * C), c = i - j * 2 * C;
    wcat[i] = c < C ? wx[j * C + c] : wg[j * C + c - C];
    if (i < I) bcat[i] = bx[i] + bg[i];
  }
}
// the reverse for the gradients: dW_x, dW_g from dwcat; db_x = db_g = dbcat
__global__ __launch_bounds__(256) void k_ag_split(const float* __restrict__ dwcat,
                                                  const float* __restrict__ dbcat,
                                                  float* __restrict__ dwx, float* __restrict__ dwg,
                                                  float* __restrict__ dbx, float* __restrict__ dbg,
                                                  int I, int C) {
  const int n = I * 2 * C;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int j = i / (2 * C), c = i - j * 2 * C;
    if (c < C) dwx[j * C + c] = dwcat[i];
    else dwg[j * C + c - C] = dwcat[i];
    if (i < I) { dbx[i] = dbcat[i]; dbg[i] = dbcat[i]; }
  }
}
// per voxel: att = relu(hidden row) in place, psi = sigmoid(w_psi . att + b_psi),
// s = u psi
__global__ __launch_bounds__(256) void k_ag_fwd(float* __restrict__ att,
                                                const float* __restrict__ wpsi,
                                                const float* __restrict__ bpsi,
                                                const float* __restrict__ u,
                                                float* __restrict__ psi, float* __restrict__ s,
                                                int64_t V, int I, int C) {
  for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < V;
       v += (int64_t)gridDim.x * blockDim.x) {
    float4* a = reinterpret_cast<float4*>(att + v * I);
    float t = bpsi[0];
    for (int j = 0; j < I / 4; ++j) {
      float4 q = a[j];
      q.x = fmaxf(q.x, 0.f); q.y = fmaxf(q.y, 0.f); q.z = fmaxf(q.z, 0.f); q.w = fmaxf(q.w, 0.f);
      a[j] = q;
      t += wpsi[4 * j] * q.x;
      t += wpsi[4 * j + 1] * q.y;
      t += wpsi[4 * j + 2] * q.z;
      t += wpsi[4 * j + 3] * q.w;
    }
    const float p = 1.f / (1.f + expf(-t));
    psi[v] = p;
    const float4* ur = reinterpret_cast<const float4*>(u + v * C);
    float4* sr = reinterpret_cast<float4*>(s + v * C);
    for (int c = 0; c < C / 4; ++c) {
      float4 q = ur[c];
      q.x *= p; q.y *= p; q.z *= p; q.w *= p;
      sr[c] = q;
    }
  }
}
// per voxel: du += ds psi;  dpp = (ds . u) psi (1 - psi)
__global__ __launch_bounds__(256) void k_ag_bwd_vox(const float* __restrict__ ds,
                                                    const float* __restrict__ u,
                                                    float* __restrict__ du,
                                                    const float* __restrict__ psi,
                                                    float* __restrict__ dpp, int64_t V, int C) {
  for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < V;
       v += (int64_t)gridDim.x * blockDim.x) {
    const float p = psi[v];
    const float4* dr = reinterpret_cast<const float4*>(ds + v * C);
    const float4* ur = reinterpret_cast<const float4*>(u + v * C);
    float4* gr = reinterpret_cast<float4*>(du + v * C);
    float t = 0.f;
    for (int c = 0; c < C / 4; ++c) {
      const float4 a = dr[c], q = ur[c];
      float4 g = gr[c];
      t += a.x * q.x; t += a.y * q.y; t += a.z * q.z; t += a.w * q.w;
      g.x += a.x * p; g.y += a.y * p; g.z += a.z * p; g.w += a.w * p;
      gr[c] = g;
    }
    dpp[v] = t * p * (1.f - p);
  }
}
// part[blk][j] = sum over the block's voxels of dpp[v] att[v][j] (j < I), part[blk][I] =
// sum dpp[v]: thread (g, j) walks voxels g, g + ngc, ... of the block's chunk, then the
// groups are added in order
__global__ __launch_bounds__(256) void k_ag_wpsi_part(const float* __restrict__ att,
                                                      const float* __restrict__ dpp,
                                                      float* __restrict__ part, int64_t V, int I) {
  __shared__ float sh[256];
  __shared__ float sb[256];
  const int64_t chunk = (V + gridDim.x - 1) / gridDim.x;
  const int64_t vb = (int64_t)blockIdx.x * chunk, ve = min(V, vb + chunk);
  for (int j0 = 0; j0 < I; j0 += 256) {
    const int Ic = min(I - j0, 256);
    const int g = threadIdx.x / Ic, j = threadIdx.x - g * Ic;
    const int ngc = max(1, 256 / Ic);
    float s = 0.f, sp = 0.f;
    if (g < ngc) {
      for (int64_t v = vb + g; v < ve; v += ngc) {
        const float d = dpp[v];
        s += d * att[v * I + j0 + j];
        sp += d;
      }
    }
    sh[threadIdx.x] = s;
    sb[threadIdx.x] = sp;
    __syncthreads();
    if (threadIdx.x < Ic) {
      float t = 0.f;
      for (int q = 0; q < ngc; ++q) t += sh[q * Ic + threadIdx.x];
      part[(int64_t)blockIdx.x * (I + 1) + j0 + threadIdx.x] = t;
      if (j0 == 0 && threadIdx.x == 0) {
        float tb = 0.f;
        for (int q = 0; q < ngc; ++q) tb += sb[q * Ic];
        part[(int64_t)blockIdx.x * (I + 1) + I] = tb;
      }
    }
    __syncthreads();
  }
}
// dwpsi[j] = sum_blk part[blk][j], dbpsi = sum_blk part[blk][I], in block order
__global__ __launch_bounds__(256) void k_ag_wpsi_fin(const float* __restrict__ part, int nblk,
                                                     float* __restrict__ dwpsi,
                                                     float* __restrict__ dbpsi, int I) {
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j <= I; j += gridDim.x * blockDim.x) {
    float s = 0.f;
    for (int q = 0; q < nblk; ++q) s += part[(int64_t)q * (I + 1) + j];
    if (j < I) dwpsi[j] = s;
    else dbpsi[0] = s;
  }
}
// dhid[v][j] = dpp[v] w_psi[j] [att > 0]: the hidden row's gradient
__global__ __launch_bounds__(256) void k_ag_dhid(const float* __restrict__ att,
                                                 float* __restrict__ dhid,
                                                 const float* __restrict__ dpp,
                                                 const float* __restrict__ wpsi, int64_t n4,
                                                 int I4) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t v = i / I4;
    const int j = (int)(i - v * I4) * 4;
    const float d = dpp[v];
    const float4 w = *reinterpret_cast<const float4*>(wpsi + j);
    float4 a = reinterpret_cast<const float4*>(att)[i];
    a.x = a.x > 0.f ? d * w.x : 0.f; a.y = a.y > 0.f ? d * w.y : 0.f;
    a.z = a.z > 0.f ? d * w.z : 0.f; a.w = a.w > 0.f ? d * w.w : 0.f;
    reinterpret_cast<float4*>(dhid)[i] = a;
  }
}

#define AG_EW(kernel, work, ...)                                                       \
  do {                                                                                 \
    hipLaunchKernelGGL(kernel, dim3(ew_grid(work)), dim3(256), 0, s, __VA_ARGS__);     \
    const hipError_t _e = hipGetLastError();                                           \
    if (_e != hipSuccess) return _e;                                                   \
  } while (0)
#define AG_CK(expr)                    \
  do {                                 \
    const hipError_t _e = (expr);      \
    if (_e != hipSuccess) return _e;   \
  } while (0)

}  // namespace

hipError_t attn_gate_fwd(const AttnGate& a, const float* u, const float* g, hipStream_t s) {
  const int64_t M = a.M;
  const int C = a.C, I = a.I;
  AG_EW(k_ag_cat, (int64_t)I * 2 * C, a.wx, a.wg, a.bx, a.bg, a.wcat, a.bcat, I, C);
  AG_CK(head_pack(a.wcat, a.pk, a.pk + head_pack_dgrad_offset(2 * C, I), 2 * C, I, s));
  AG_CK(linear_fwd2(Src2{u, g, C, C, C}, 2 * C, a.pk, a.bcat, a.att, I, I, M, s));
  AG_EW(k_ag_fwd, M, a.att, a.wpsi, a.bpsi, u, a.psi, a.s, M, I, C);
  return hipSuccess;
}

hipError_t attn_gate_bwd(const AttnGate& a, const float* u, const float* g, const float* ds,
                         float* du, float* dg, hipStream_t s) {
  const int64_t M = a.M;
  const int C = a.C, I = a.I;
  AG_EW(k_ag_bwd_vox, M, ds, u, du, a.psi, a.dpp, M, C);
  const int nb = (int)std::min<int64_t>(AG_NB, (M + 255) / 256);
  hipLaunchKernelGGL(k_ag_wpsi_part, dim3(nb), dim3(256), 0, s, a.att, a.dpp, a.part, M, I);
  AG_CK(hipGetLastError());
  hipLaunchKernelGGL(k_ag_wpsi_fin, dim3(1), dim3(256), 0, s, a.part, nb, a.dwpsi, a.dbpsi, I);
  AG_CK(hipGetLastError());
  AG_EW(k_ag_dhid, M * I / 4, a.att, a.dhid, a.dpp, a.wpsi, M * I / 4, I / 4);
  const Src2 in{u, g, C, C, C};
  AG_CK(linear_wgrad2(in, 2 * C, a.dhid, I, I, a.dwcat, a.dbcat, M, a.wgs, s));
  AG_EW(k_ag_split, (int64_t)I * 2 * C, a.dwcat, a.dbcat, a.dwx, a.dwg, a.dbx, a.dbg, I, C);
  AG_CK(zero_async(dg, M * C * sizeof(float), s));
  AG_CK(linear_dgrad2(a.dhid, I, I, a.pk + head_pack_dgrad_offset(2 * C, I),
                      Dst2{du, dg, C, C, C}, 2 * C, M, 1, s));
  return hipSuccess;
}

}  // namespace spff
