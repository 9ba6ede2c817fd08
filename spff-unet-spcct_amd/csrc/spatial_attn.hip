// CBAM spatial attention of the SPCT core (reference SpatialAttention3D, models.py:434-446)
// on channel-last rows x [V][C], V = B D H W:
//
//   m[v] = [mean_c x[v,c], max_c x[v,c]]
//   a[v] = sigmoid(conv3d(m, W[1][2][3][7][7], zero padding (1,3,3) of m, no bias))
//   y[v,c] = x[v,c] a[v]
//
// and its backward
//
//   da[v] = sum_c dy[v,c] x[v,c],  dt = da a (1 - a)
//   dm = the stencil's input gradient of dt, dW its weight gradient (294 sums over V)
//   dx[v,c] = dy[v,c] a[v] + dm[v,0] / C + [c = argmax_c x[v,.]] dm[v,1]
//
// Passes.  Forward: k_sa_stats (reads x once: mean, max and the lowest argmax of a row),
// k_sa_stencil_fwd, k_sa_scale (reads x, writes y).  Backward: k_sa_bwd_dot (reads dy and x),
// k_sa_stencil_bwd (dm and the per-tile weight-gradient partials from one staged dt tile),
// k_sa_rows_reduce (the partials, 64 rows per block and level), k_sa_bwd_dx (reads dy,
// writes dx).  The stencil has two input channels and one output: a direct LDS-tiled
// stencil, one workgroup per (b, d, 16 x 16 tile of H x W) staging the three depth planes
// with a 3-voxel rim, the 294 weights in LDS.
//
// Every sum has a fixed order (a lane's chunks in order, then an xor tree over the lanes of
// a row; the stencil's taps in (channel, kd, kh, kw) order; a tile's voxels in row order;
// the tiles in index order, 64 at a level), so two runs give the same bits.  No atomics.
#include "spff_internal.h"
#include "spff.h"

#include <algorithm>
#include <string>

namespace spff {

namespace {

constexpr int SA_KD = 3, SA_KH = 7, SA_KW = 7;
constexpr int SA_TAPS = SA_KD * SA_KH * SA_KW;  // per input channel
constexpr int SA_NW = 2 * SA_TAPS;              // 294 weights
constexpr int SA_T = 16;                        // tile edge in H and W
constexpr int SA_R = SA_T + SA_KH - 1;          // staged edge (3-voxel rim each side)
constexpr int SA_PLANE = SA_R * SA_R;
constexpr int SA_NT = SA_T * SA_T;              // threads per stencil workgroup
constexpr int SA_ROWS = 64;                     // partial rows one reduce block sums
static_assert(SA_KH == SA_KW && SA_NT == 256 && SA_TAPS <= SA_NT, "tile / tap layout");

// lanes that share one row: the largest power of two <= C / 4, at most 64
inline int sa_lanes(int C) {
  int L = 1;
  while (2 * L <= C / 4 && L < 64) L *= 2;
  return L;
}
inline int grid_for(int64_t blocks) {
  return (int)std::max<int64_t>(1, std::min<int64_t>(blocks, 1 << 20));
}

// map[v] = (mean, max) and idx[v] = the lowest c with x[v,c] = max.  L lanes per row; lane j
// reads the float4 chunks j, j + L, ...
__global__ void __launch_bounds__(256)
k_sa_stats(const float* __restrict__ x, int64_t V, int C, int L, float* __restrict__ map,
           int* __restrict__ idx) {
  const int sub = threadIdx.x & (L - 1);
  const int vpb = 256 / L;
  const int nq = C >> 2;
  for (int64_t v0 = (int64_t)blockIdx.x * vpb; v0 < V; v0 += (int64_t)gridDim.x * vpb) {
    const int64_t v = v0 + threadIdx.x / L;
    float s = 0.f, mx = 0.f;
    int mi = 0;
    if (v < V) {
      const float4* r = reinterpret_cast<const float4*>(x + v * C);
      float4 t = r[sub];  // L <= nq: every lane owns a chunk
      mx = t.x;
      mi = 4 * sub;
      for (int q = sub;;) {
        s += t.x; s += t.y; s += t.z; s += t.w;
        if (t.x > mx) { mx = t.x; mi = 4 * q; }
        if (t.y > mx) { mx = t.y; mi = 4 * q + 1; }
        if (t.z > mx) { mx = t.z; mi = 4 * q + 2; }
        if (t.w > mx) { mx = t.w; mi = 4 * q + 3; }
        q += L;
        if (q >= nq) break;
        t = r[q];
      }
    }
    for (int o = L >> 1; o; o >>= 1) {
      const float s2 = __shfl_xor(s, o), m2 = __shfl_xor(mx, o);
      const int i2 = __shfl_xor(mi, o);
      // both partners add the same two values in lane order, so they agree
      s = (sub & o) ? s2 + s : s + s2;
      if (m2 > mx || (m2 == mx && i2 < mi)) { mx = m2; mi = i2; }
    }
    if (v < V && sub == 0) {
      reinterpret_cast<float2*>(map)[v] = make_float2(s / (float)C, mx);
      idx[v] = mi;
    }
  }
}

// dt[v] = (sum_c dy[v,c] x[v,c]) a (1 - a), rows shared by L lanes as above
__global__ void __launch_bounds__(256)
k_sa_bwd_dot(const float* __restrict__ dy, const float* __restrict__ x,
             const float* __restrict__ attn, int64_t V, int C, int L, float* __restrict__ dt) {
  const int sub = threadIdx.x & (L - 1);
  const int vpb = 256 / L;
  const int nq = C >> 2;
  for (int64_t v0 = (int64_t)blockIdx.x * vpb; v0 < V; v0 += (int64_t)gridDim.x * vpb) {
    const int64_t v = v0 + threadIdx.x / L;
    float s = 0.f;
    if (v < V) {
      const float4* rx = reinterpret_cast<const float4*>(x + v * C);
      const float4* rg = reinterpret_cast<const float4*>(dy + v * C);
      for (int q = sub; q < nq; q += L) {
        const float4 a = rx[q], g = rg[q];
        s = fmaf(g.x, a.x, s); s = fmaf(g.y, a.y, s);
        s = fmaf(g.z, a.z, s); s = fmaf(g.w, a.w, s);
      }
    }
    for (int o = L >> 1; o; o >>= 1) {
      const float s2 = __shfl_xor(s, o);
      s = (sub & o) ? s2 + s : s + s2;
    }
    if (v < V && sub == 0) {
      const float a = attn[v];
      dt[v] = s * a * (1.f - a);
    }
  }
}

struct SaTile {
  int b, d, h0, w0;  // the tile's first row / column
};
__device__ __forceinline__ SaTile sa_tile(int D, int th, int tw) {
  int64_t t = blockIdx.x;
  SaTile r;
  r.w0 = (int)(t % tw) * SA_T; t /= tw;
  r.h0 = (int)(t % th) * SA_T; t /= th;
  r.d = (int)(t % D);
  r.b = (int)(t / D);
  return r;
}

// attn[v] = sigmoid(sum_{ch,kd,kh,kw} m[d+kd-1, h+kh-3, w+kw-3][ch] W[ch][kd][kh][kw])
__global__ void __launch_bounds__(SA_NT)
k_sa_stencil_fwd(const float* __restrict__ map, const float* __restrict__ w, int D, int H, int W,
                 int th, int tw, float* __restrict__ attn) {
  __shared__ float sm[2 * SA_KD * SA_PLANE + SA_NW];
  float* sw = sm + 2 * SA_KD * SA_PLANE;
  const SaTile t = sa_tile(D, th, tw);
  const int tid = threadIdx.x;
  for (int i = tid; i < SA_NW; i += SA_NT) sw[i] = w[i];
  for (int i = tid; i < SA_KD * SA_PLANE; i += SA_NT) {
    const int kd = i / SA_PLANE, r = i - kd * SA_PLANE;
    const int dd = t.d + kd - 1, hh = t.h0 - 3 + r / SA_R, ww = t.w0 - 3 + r % SA_R;
    float2 m = make_float2(0.f, 0.f);
    if ((unsigned)dd < (unsigned)D && (unsigned)hh < (unsigned)H && (unsigned)ww < (unsigned)W)
      m = reinterpret_cast<const float2*>(map)[(((int64_t)t.b * D + dd) * H + hh) * W + ww];
    sm[kd * SA_PLANE + r] = m.x;
    sm[(SA_KD + kd) * SA_PLANE + r] = m.y;
  }
  __syncthreads();
  const int ly = tid / SA_T, lx = tid % SA_T;
  const int h = t.h0 + ly, wv = t.w0 + lx;
  if (h >= H || wv >= W) return;
  float acc = 0.f;
  for (int ch = 0; ch < 2; ++ch)
    for (int kd = 0; kd < SA_KD; ++kd) {
      if ((unsigned)(t.d + kd - 1) >= (unsigned)D) continue;  // a plane of padding: zeros
      const float* pl = sm + (ch * SA_KD + kd) * SA_PLANE + ly * SA_R + lx;
      const float* wk = sw + (ch * SA_KD + kd) * SA_KH * SA_KW;
#pragma unroll
      for (int kh = 0; kh < SA_KH; ++kh)
#pragma unroll
        for (int kw = 0; kw < SA_KW; ++kw)
          acc = fmaf(pl[kh * SA_R + kw], wk[kh * SA_KW + kw], acc);
    }
  attn[(((int64_t)t.b * D + t.d) * H + h) * W + wv] = 1.f / (1.f + expf(-acc));
}

// One staged dt tile (three depth planes, 3-voxel rim, zero outside the volume) gives both
//   dm[u][ch] = sum_k dt[u - k + pad] W[ch][k]                      (every voxel u of the tile)
//   part[tile][ch 147 + k] = sum_{u in tile} m[u][ch] dt[u - k + pad]   (thread k < 147)
// and the tiles' rows sum to dW: every (u, k) pair lies in exactly one tile.
__global__ void __launch_bounds__(SA_NT)
k_sa_stencil_bwd(const float* __restrict__ dt, const float* __restrict__ map,
                 const float* __restrict__ w, int D, int H, int W, int th, int tw,
                 float* __restrict__ dm, float* __restrict__ part) {
  __shared__ float sm[SA_KD * SA_PLANE + SA_NW + 2 * SA_NT];
  float* sw = sm + SA_KD * SA_PLANE;
  float* sc = sw + SA_NW;  // the tile's own m: [2][256]
  const SaTile t = sa_tile(D, th, tw);
  const int tid = threadIdx.x;
  for (int i = tid; i < SA_NW; i += SA_NT) sw[i] = w[i];
  for (int i = tid; i < SA_KD * SA_PLANE; i += SA_NT) {
    const int j = i / SA_PLANE, r = i - j * SA_PLANE;
    const int dd = t.d + j - 1, hh = t.h0 - 3 + r / SA_R, ww = t.w0 - 3 + r % SA_R;
    float g = 0.f;
    if ((unsigned)dd < (unsigned)D && (unsigned)hh < (unsigned)H && (unsigned)ww < (unsigned)W)
      g = dt[(((int64_t)t.b * D + dd) * H + hh) * W + ww];
    sm[i] = g;
  }
  const int ly = tid / SA_T, lx = tid % SA_T;
  const int h = t.h0 + ly, wv = t.w0 + lx;
  const bool in = h < H && wv < W;
  const int64_t v = (((int64_t)t.b * D + t.d) * H + h) * W + wv;
  {
    float2 m = make_float2(0.f, 0.f);
    if (in) m = reinterpret_cast<const float2*>(map)[v];
    sc[tid] = m.x;
    sc[SA_NT + tid] = m.y;
  }
  __syncthreads();
  if (in) {
    // dt[d - kd + 1] is staged plane 2 - kd; row h - kh + 3 is staged row ly + 6 - kh
    float a0 = 0.f, a1 = 0.f;
    for (int kd = 0; kd < SA_KD; ++kd) {
      if ((unsigned)(t.d + 1 - kd) >= (unsigned)D) continue;
      const float* pl = sm + (SA_KD - 1 - kd) * SA_PLANE + (ly + SA_KH - 1) * SA_R + lx + SA_KW - 1;
      const float* w0 = sw + kd * SA_KH * SA_KW;
      const float* w1 = w0 + SA_TAPS;
#pragma unroll
      for (int kh = 0; kh < SA_KH; ++kh)
#pragma unroll
        for (int kw = 0; kw < SA_KW; ++kw) {
          const float g = pl[-kh * SA_R - kw];
          a0 = fmaf(g, w0[kh * SA_KW + kw], a0);
          a1 = fmaf(g, w1[kh * SA_KW + kw], a1);
        }
    }
    reinterpret_cast<float2*>(dm)[v] = make_float2(a0, a1);
  }
  if (tid < SA_TAPS) {
    const int kd = tid / (SA_KH * SA_KW), kh = (tid / SA_KW) % SA_KH, kw = tid % SA_KW;
    const float* pl = sm + (SA_KD - 1 - kd) * SA_PLANE + (SA_KH - 1 - kh) * SA_R + SA_KW - 1 - kw;
    float p0 = 0.f, p1 = 0.f;
    for (int uy = 0; uy < SA_T; ++uy) {  // a row's 16 products first, then the rows
      float r0 = 0.f, r1 = 0.f;
#pragma unroll
      for (int ux = 0; ux < SA_T; ++ux) {
        const float g = pl[uy * SA_R + ux];
        r0 = fmaf(sc[uy * SA_T + ux], g, r0);
        r1 = fmaf(sc[SA_NT + uy * SA_T + ux], g, r1);
      }
      p0 += r0;
      p1 += r1;
    }
    float* row = part + (int64_t)blockIdx.x * SA_NW;
    row[tid] = p0;
    row[SA_TAPS + tid] = p1;
  }
}

// out[g][k] = sum of in[j][k] over the rows j of group g (SA_ROWS rows, in order)
__global__ void __launch_bounds__(320)
k_sa_rows_reduce(const float* __restrict__ in, int64_t n, float* __restrict__ out) {
  const int k = threadIdx.x;
  if (k >= SA_NW) return;
  const int64_t j0 = (int64_t)blockIdx.x * SA_ROWS, j1 = j0 + SA_ROWS < n ? j0 + SA_ROWS : n;
  float s = 0.f;
  for (int64_t j = j0; j < j1; ++j) s += in[j * SA_NW + k];
  out[(int64_t)blockIdx.x * SA_NW + k] = s;
}

// y[v][c] = x[v][c] a[v] (y may be x: no __restrict__ on the pair)
__global__ void __launch_bounds__(256)
k_sa_scale(const float* x, const float* __restrict__ attn, int64_t nq, int cq, float* y) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nq; i += (int64_t)gridDim.x * 256) {
    const float a = attn[i / cq];
    float4 t = reinterpret_cast<const float4*>(x)[i];
    t.x *= a; t.y *= a; t.z *= a; t.w *= a;
    reinterpret_cast<float4*>(y)[i] = t;
  }
}

// dx[v][c] = dy[v][c] a[v] + dm[v][0] / C + [c = idx[v]] dm[v][1] (dx may be dy)
__global__ void __launch_bounds__(256)
k_sa_bwd_dx(const float* dy, const float* __restrict__ attn, const float* __restrict__ dm,
            const int* __restrict__ idx, int64_t nq, int cq, float* dx) {
  const float C = (float)(4 * cq);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nq; i += (int64_t)gridDim.x * 256) {
    const int64_t v = i / cq;
    const int c = (int)(i - v * cq) * 4;
    const float a = attn[v];
    const float2 g = reinterpret_cast<const float2*>(dm)[v];
    const float mean = g.x / C;
    const int hit = idx[v] - c;  // 0..3: the row's max lies in this chunk
    float4 t = reinterpret_cast<const float4*>(dy)[i];
    t.x = fmaf(t.x, a, mean) + (hit == 0 ? g.y : 0.f);
    t.y = fmaf(t.y, a, mean) + (hit == 1 ? g.y : 0.f);
    t.z = fmaf(t.z, a, mean) + (hit == 2 ? g.y : 0.f);
    t.w = fmaf(t.w, a, mean) + (hit == 3 ? g.y : 0.f);
    reinterpret_cast<float4*>(dx)[i] = t;
  }
}

inline int64_t sa_tiles(const Vol& v) {
  return (int64_t)v.B * v.D * ((v.H + SA_T - 1) / SA_T) * ((v.W + SA_T - 1) / SA_T);
}
inline size_t up256(size_t n) { return (n + 255) / 256 * 256; }

}  // namespace

hipError_t sa_stats(const float* x, int64_t V, int C, float* map, int* idx, hipStream_t s) {
  if (C < 8 || C % 8 || V < 1) return hipErrorInvalidValue;
  const int L = sa_lanes(C);
  const int64_t blocks = (V + 256 / L - 1) / (256 / L);
  hipLaunchKernelGGL(k_sa_stats, dim3(grid_for(blocks)), dim3(256), 0, s, x, V, C, L, map, idx);
  return hipGetLastError();
}

hipError_t sa_attn(const float* map, const float* w, Vol v, float* attn, hipStream_t s) {
  const int64_t tiles = sa_tiles(v);
  if (tiles < 1 || tiles > INT32_MAX) return hipErrorInvalidValue;
  const int th = (v.H + SA_T - 1) / SA_T, tw = (v.W + SA_T - 1) / SA_T;
  hipLaunchKernelGGL(k_sa_stencil_fwd, dim3((unsigned)tiles), dim3(SA_NT), 0, s, map, w, v.D, v.H,
                     v.W, th, tw, attn);
  return hipGetLastError();
}

hipError_t sa_scale(const float* x, const float* attn, int64_t V, int C, float* y, hipStream_t s) {
  if (C < 4 || C % 4 || V < 1) return hipErrorInvalidValue;
  const int64_t nq = V * (C / 4);
  hipLaunchKernelGGL(k_sa_scale, dim3(grid_for((nq + 255) / 256)), dim3(256), 0, s, x, attn, nq,
                     C / 4, y);
  return hipGetLastError();
}

// ws = [dt V | dm 2V | partial rows: tiles x 294 | ceil(tiles / 64) x 294]
size_t sa_bwd_ws_bytes(Vol v) {
  const int64_t V = nvox(v), tiles = sa_tiles(v);
  return up256(V * sizeof(float)) + up256(2 * V * sizeof(float)) +
         up256(tiles * SA_NW * sizeof(float)) +
         up256((tiles + SA_ROWS - 1) / SA_ROWS * SA_NW * sizeof(float));
}

hipError_t sa_bwd(const float* dy, const float* x, const float* w, const float* attn,
                  const float* map, const int* idx, Vol v, int C, float* dx, float* dw, void* ws,
                  hipStream_t s) {
  const int64_t V = nvox(v), tiles = sa_tiles(v);
  if (C < 8 || C % 8 || V < 1 || tiles > INT32_MAX) return hipErrorInvalidValue;
  char* p = static_cast<char*>(ws);
  float* dt = reinterpret_cast<float*>(p);
  p += up256(V * sizeof(float));
  float* dm = reinterpret_cast<float*>(p);
  p += up256(2 * V * sizeof(float));
  float* pa = reinterpret_cast<float*>(p);
  p += up256(tiles * SA_NW * sizeof(float));
  float* pb = reinterpret_cast<float*>(p);
  const int L = sa_lanes(C);
  const int64_t blocks = (V + 256 / L - 1) / (256 / L);
  hipLaunchKernelGGL(k_sa_bwd_dot, dim3(grid_for(blocks)), dim3(256), 0, s, dy, x, attn, V, C, L,
                     dt);
  const int th = (v.H + SA_T - 1) / SA_T, tw = (v.W + SA_T - 1) / SA_T;
  hipLaunchKernelGGL(k_sa_stencil_bwd, dim3((unsigned)tiles), dim3(SA_NT), 0, s, dt, map, w, v.D,
                     v.H, v.W, th, tw, dm, pa);
  // the tiles' rows, 64 to one at a level, between the two partial buffers; the last level
  // (one group) writes dw
  const float* in = pa;
  float* spare = pb;
  for (int64_t n = tiles;;) {
    const int64_t groups = (n + SA_ROWS - 1) / SA_ROWS;
    float* out = groups == 1 ? dw : spare;
    hipLaunchKernelGGL(k_sa_rows_reduce, dim3((unsigned)groups), dim3(320), 0, s, in, n, out);
    if (groups == 1) break;
    spare = const_cast<float*>(in);  // at most n / 64 rows of it are written next
    in = out;
    n = groups;
  }
  const int64_t nq = V * (C / 4);
  hipLaunchKernelGGL(k_sa_bwd_dx, dim3(grid_for((nq + 255) / 256)), dim3(256), 0, s, dy, attn, dm,
                     idx, nq, C / 4, dx);
  return hipGetLastError();
}

}  // namespace spff

// =================================================================== C ABI ==
using namespace spff;

namespace {
int sa_args(const char* what, int B, int D, int H, int W, int C) {
  if (B < 1 || D < 1 || H < 1 || W < 1 || C < 8 || C % 8)
    return set_error(SPFF_EINVAL, (std::string(what) + ": B, D, H, W must be positive and C a "
                                                       "positive multiple of 8").c_str());
  if ((int64_t)B * D * H * W > (int64_t)1 << 40)
    return set_error(SPFF_EINVAL, (std::string(what) + ": volume too large").c_str());
  return SPFF_OK;
}
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
}  // namespace

extern "C" {

size_t spff_spatial_attn_ws_bytes(int B, int D, int H, int W, int C) {
  if (sa_args("spff_spatial_attn_ws_bytes", B, D, H, W, C) != SPFF_OK) return 0;
  return sa_bwd_ws_bytes(Vol{B, D, H, W});
}

int spff_spatial_attn_fwd(const float* x, const float* w, int B, int D, int H, int W, int C,
                          float* y, float* attn, float* map, int32_t* idx, void* ws,
                          void* stream) {
  (void)ws;  // the forward needs none; the argument keeps the two calls alike
  const int r = sa_args("spff_spatial_attn_fwd", B, D, H, W, C);
  if (r != SPFF_OK) return r;
  if (!x || !w || !y || !attn || !map || !idx)
    return set_error(SPFF_EINVAL, "spff_spatial_attn_fwd: null argument");
  if (!aligned16(x) || !aligned16(y) || !aligned16(map))
    return set_error(SPFF_EINVAL, "spff_spatial_attn_fwd: x, y and map must be 16-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const Vol v{B, D, H, W};
  hipError_t e = sa_stats(x, nvox(v), C, map, idx, s);
  if (e == hipSuccess) e = sa_attn(map, w, v, attn, s);
  if (e == hipSuccess) e = sa_scale(x, attn, nvox(v), C, y, s);
  return e == hipSuccess ? SPFF_OK : set_error(SPFF_EHIP, hipGetErrorString(e));
}

int spff_spatial_attn_bwd(const float* dy, const float* x, const float* w, const float* attn,
                          const float* map, const int32_t* idx, int B, int D, int H, int W, int C,
                          float* dx, float* dw, void* ws, void* stream) {
  const int r = sa_args("spff_spatial_attn_bwd", B, D, H, W, C);
  if (r != SPFF_OK) return r;
  if (!dy || !x || !w || !attn || !map || !idx || !dx || !dw || !ws)
    return set_error(SPFF_EINVAL, "spff_spatial_attn_bwd: null argument");
  if (!aligned16(dy) || !aligned16(x) || !aligned16(dx) || !aligned16(map) || !aligned16(ws))
    return set_error(SPFF_EINVAL,
                     "spff_spatial_attn_bwd: dy, x, dx, map and ws must be 16-byte aligned");
  const hipError_t e = sa_bwd(dy, x, w, attn, map, idx, Vol{B, D, H, W}, C, dx, dw, ws,
                              static_cast<hipStream_t>(stream));
  return e == hipSuccess ? SPFF_OK : set_error(SPFF_EHIP, hipGetErrorString(e));
}

}  // extern "C"
