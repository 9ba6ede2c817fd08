// Sliding-window inference with separable window weights on the device.
//
//   k_tile_gather      a thread per element of the staging batch [n][C][rd][rh][rw]: window w
//                      of the volume [C][D][H][W], mirrored along the axes of its flip bits.
//   k_tile_accumulate  acc[v][k] += w(v) s[v][k] for the windows of one call, in table order.
//                      The launch covers the bounding box of the call's windows: a wave per
//                      64 consecutive x of one (z, y) row of the box.  The row's (x, k) run is
//                      contiguous in acc and in every tile, so the wave copies its acc span
//                      into its LDS slice (float4 when aligned), then for each window of the
//                      table that covers (z, y) copies the tile's span beside it, a lane per
//                      voxel adds its row (softmax = 1: the row's fp32 softmax first), and the
//                      span goes back in one pass.  acc is read and written once per call
//                      however many windows overlap, and a voxel's sum is one chain of fmaf in
//                      table order: the same bits for every split of the table into calls.
//   k_tile_finalize    one read of acc: the first-maximum class byte (spff_confusion's rule: a
//                      NaN counts as the largest), with labels the (pred, label) cell of a
//                      per-workgroup LDS histogram that leaves by 64-bit atomics (bounded
//                      grid, k_head_mask_s's pattern), and, when asked, scores = acc / norm
//                      with norm = flips nz[z] ny[y] nx[x] written back through the LDS slice.
// A flipped window is gathered mirrored and accumulated mirrored back.  The window table
// travels by value in the kernel arguments; every window is validated on the host before
// any device call, so no kernel receives a window it could leave the volume with.
// No allocation, no host synchronisation: a captured graph replays every call.
#include "spff_internal.h"
#include <math.h>

namespace spff {

namespace {

constexpr int TL_MAX_WINDOWS = SPFF_TILE_MAX_WINDOWS;
constexpr int TL_MAX_K = 32;
constexpr int TL_GATHER_T = 256;
constexpr int TL_ACC_T = 128;  // two waves, each an acc and a tile slice of 64 K floats
constexpr int TL_ACC_WAVES = TL_ACC_T / 64;
constexpr int TL_FIN_T = 256;
constexpr int TL_FIN_WAVES = TL_FIN_T / 64;
constexpr unsigned TL_FIN_GRID = 1024;  // (with labels every workgroup ends in atomics)

struct TileTable {
  int32_t w[TL_MAX_WINDOWS][4];  // z0, y0, x0, flip bits
};

__global__ __launch_bounds__(TL_GATHER_T) void k_tile_gather(const float* __restrict__ x, int C,
                                                             int D, int H, int W, TileTable t,
                                                             int rd, int rh, int rw, int64_t total,
                                                             float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * TL_GATHER_T + threadIdx.x;
  if (i >= total) return;
  int tx = (int)(i % rw);
  int64_t r = i / rw;
  int ty = (int)(r % rh);
  r /= rh;
  int tz = (int)(r % rd);
  r /= rd;
  const int c = (int)(r % C);
  const int w = (int)(r / C);
  const int f = t.w[w][3];
  if (f & 1) tz = rd - 1 - tz;
  if (f & 2) ty = rh - 1 - ty;
  if (f & 4) tx = rw - 1 - tx;
  out[i] = x[(((int64_t)c * D + t.w[w][0] + tz) * H + t.w[w][1] + ty) * W + t.w[w][2] + tx];
}

struct AccGeo {
  int n, rd, rh, rw, K, D, H, W;
  int bz0, by0, bx0, bd, bh, bw;  // the bounding box of the call's windows
  int gx;                         // groups of 64 x per box row
};

__global__ __launch_bounds__(TL_ACC_T) void k_tile_accumulate(const float* __restrict__ tiles,
                                                              TileTable t, AccGeo g,
                                                              const float* __restrict__ wz,
                                                              const float* __restrict__ wy,
                                                              const float* __restrict__ wx,
                                                              int softmax,
                                                              float* __restrict__ acc) {
  extern __shared__ __attribute__((aligned(16))) float tsm[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int K = g.K;
  const int64_t wid = (int64_t)blockIdx.x * TL_ACC_WAVES + wv;
  if (wid >= (int64_t)g.bd * g.bh * g.gx) return;  // (no workgroup barrier below)
  const int gi = (int)(wid % g.gx);
  const int64_t row = wid / g.gx;
  const int y = g.by0 + (int)(row % g.bh), z = g.bz0 + (int)(row / g.bh);
  const int xa = g.bx0 + gi * 64;
  const int nv = g.bx0 + g.bw - xa < 64 ? g.bx0 + g.bw - xa : 64;
  float* sa = tsm + (size_t)wv * 2 * 64 * K;  // the acc span
  float* st = sa + 64 * K;                    // one window's tile span
  float* arow = acc + (((int64_t)z * g.H + y) * g.W + xa) * K;
  bool loaded = false;
  for (int w = 0; w < g.n; ++w) {
    const int z0 = t.w[w][0], y0 = t.w[w][1], x0 = t.w[w][2], f = t.w[w][3];
    int tz = z - z0, ty = y - y0;
    if (tz < 0 || tz >= g.rd || ty < 0 || ty >= g.rh) continue;
    const int xs = xa > x0 ? xa : x0;
    const int xe = xa + nv < x0 + g.rw ? xa + nv : x0 + g.rw;
    if (xs >= xe) continue;
    if (!loaded) {  // (a wave of the box that no window covers touches nothing)
      wave_copy_rows(sa, arow, nv * K, lane);
      loaded = true;
    }
    if (f & 1) tz = g.rd - 1 - tz;
    if (f & 2) ty = g.rh - 1 - ty;
    const int cnt = xe - xs;
    const int t0 = (f & 4) ? g.rw - (xe - x0) : xs - x0;  // the span's first tile column
    const float* trow = tiles + ((((int64_t)w * g.rd + tz) * g.rh + ty) * g.rw + t0) * K;
    wave_copy_rows(st, trow, cnt * K, lane);
    wave_lds_sync();
    if (lane < cnt) {
      const int tx = t0 + lane;
      const int xv = (f & 4) ? x0 + g.rw - 1 - tx : x0 + tx;
      const float wgt = (wz[tz] * wy[ty]) * wx[tx];
      float* s = st + lane * K;
      float* a = sa + (xv - xa) * K;
      if (softmax) {
        // exp(x - max) summed in class order, then a true division (rank.hip, views.hip)
        float m = -INFINITY;
        for (int k = 0; k < K; ++k) m = fmaxf(m, s[k]);
        float ssum = 0.f;
        for (int k = 0; k < K; ++k) {
          const float e = expf(s[k] - m);
          s[k] = e;
          ssum += e;
        }
        for (int k = 0; k < K; ++k) a[k] = fmaf(wgt, s[k] / ssum, a[k]);
      } else {
        for (int k = 0; k < K; ++k) a[k] = fmaf(wgt, s[k], a[k]);
      }
    }
    wave_lds_sync();  // the next window overwrites the tile span
  }
  if (loaded) wave_copy_rows(arow, sa, nv * K, lane);
}

struct FinGeo {
  int D, H, W, K;
  int64_t V;
};

__global__ __launch_bounds__(TL_FIN_T) void k_tile_finalize(const float* acc, FinGeo g,
                                                            const float* __restrict__ nz,
                                                            const float* __restrict__ ny,
                                                            const float* __restrict__ nx,
                                                            float flips,
                                                            uint8_t* __restrict__ mask,
                                                            float* scores,
                                                            const int64_t* __restrict__ lab,
                                                            int use_ignore, int ignore,
                                                            unsigned long long* __restrict__ conf) {
  // [waves][64 K] float rows | [K (K + 1)] unsigned histogram | [256] class bytes
  extern __shared__ __attribute__((aligned(16))) float fsm[];
  const int K = g.K, K1 = K + 1;
  unsigned* hist = reinterpret_cast<unsigned*>(fsm + TL_FIN_WAVES * 64 * K);
  uint8_t* pm = reinterpret_cast<uint8_t*>(hist + ((K * K1 + 3) & ~3));
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  float* sx = fsm + wv * 64 * K;
  if (lab)
    for (int i = threadIdx.x; i < K * K1; i += TL_FIN_T) hist[i] = 0;
  __syncthreads();
  const bool m16 = !(reinterpret_cast<uintptr_t>(mask) & 15);
  const int64_t ngroups = (g.V + 63) / 64;
  for (int64_t grp = (int64_t)blockIdx.x * TL_FIN_WAVES + wv; grp < ngroups;
       grp += (int64_t)gridDim.x * TL_FIN_WAVES) {
    const int64_t v0 = grp * 64;
    const int nv = (int)(g.V - v0 < 64 ? g.V - v0 : 64);
    const int64_t yl = (lab && lane < nv) ? lab[v0 + lane] : 0;  // (overlaps the row copy)
    wave_copy_rows(sx, acc + v0 * K, nv * K, lane);
    wave_lds_sync();
    if (lane < nv) {
      float* xr = sx + lane * K;
      float m = xr[0];
      int am = 0;
      for (int k = 1; k < K; ++k) {
        const float v = xr[k];
        if (v > m || (isnan(v) && !isnan(m))) { m = v; am = k; }
      }
      pm[threadIdx.x] = (uint8_t)am;
      if (lab && (!use_ignore || yl != ignore))
        atomicAdd(&hist[am * K1 + ((yl < 0 || yl >= K) ? K : (int)yl)], 1u);
      if (scores) {
        const int64_t v = v0 + lane;
        const int xi = (int)(v % g.W);
        const int64_t r = v / g.W;
        const float norm = ((flips * nz[r / g.H]) * ny[r % g.H]) * nx[xi];
        for (int k = 0; k < K; ++k) xr[k] = xr[k] / norm;
      }
    }
    wave_lds_sync();
    if (scores) wave_copy_rows(scores + v0 * K, sx, nv * K, lane);
    if (m16 && nv == 64) {
      if (lane < 4)
        reinterpret_cast<uint4*>(mask + v0)[lane] = reinterpret_cast<const uint4*>(pm + wv * 64)[lane];
    } else if (lane < nv) {
      mask[v0 + lane] = pm[threadIdx.x];
    }
    wave_lds_sync();  // the next group overwrites the slice and the bytes
  }
  if (lab) {
    __syncthreads();
    for (int i = threadIdx.x; i < K * K1; i += TL_FIN_T)
      if (hist[i]) atomicAdd(&conf[i], (unsigned long long)hist[i]);
  }
}

int tile_error(int code, const char* fn, const char* what) {
  static thread_local char buf[200];
  snprintf(buf, sizeof buf, "%s: %s", fn, what);
  return set_error(code, buf);
}

// The table's own checks, shared by gather and accumulate: SPFF_EINVAL first, then
// SPFF_ESHAPE; 0 when every window lies wholly inside the volume.
int tile_table_check(const char* fn, const int32_t* windows, int n, int rd, int rh, int rw, int D,
                     int H, int W, TileTable* t) {
  if (n < 1 || n > TL_MAX_WINDOWS) return tile_error(SPFF_EINVAL, fn, "n must be 1..64 windows");
  if (!windows) return tile_error(SPFF_EINVAL, fn, "null argument");
  if (D < 1 || H < 1 || W < 1 || rd < 1 || rh < 1 || rw < 1)
    return tile_error(SPFF_EINVAL, fn, "an extent below 1");
  for (int i = 0; i < n; ++i)
    if (windows[4 * i + 3] < 0 || windows[4 * i + 3] > 7)
      return tile_error(SPFF_EINVAL, fn, "flip bits must be 0..7");
  if (rd > D || rh > H || rw > W)
    return tile_error(SPFF_ESHAPE, fn, "the window is larger than the volume");
  for (int i = 0; i < n; ++i) {
    const int32_t* w = windows + 4 * i;
    if (w[0] < 0 || w[1] < 0 || w[2] < 0 || w[0] > D - rd || w[1] > H - rh || w[2] > W - rw)
      return tile_error(SPFF_ESHAPE, fn, "a window is not wholly inside the volume");
    for (int j = 0; j < 4; ++j) t->w[i][j] = w[j];
  }
  for (int i = n; i < TL_MAX_WINDOWS; ++i)
    for (int j = 0; j < 4; ++j) t->w[i][j] = 0;
  return SPFF_OK;
}

int tile_hip(hipError_t e) {
  return e == hipSuccess ? SPFF_OK : set_error(SPFF_EHIP, hipGetErrorString(e));
}

}  // namespace

}  // namespace spff

// =================================================================== C ABI ==
using namespace spff;

extern "C" {

int spff_tile_gather(const float* x, int C, int D, int H, int W, const int32_t* windows, int n,
                     int rd, int rh, int rw, float* out, void* stream) {
  const char* fn = "spff_tile_gather";
  TileTable t;
  if (!x || !out) return tile_error(SPFF_EINVAL, fn, "null argument");
  if (C < 1) return tile_error(SPFF_EINVAL, fn, "an extent below 1");
  if (int rc = tile_table_check(fn, windows, n, rd, rh, rw, D, H, W, &t)) return rc;
  const int64_t total = (int64_t)n * C * rd * rh * rw;
  const int64_t blocks = (total + TL_GATHER_T - 1) / TL_GATHER_T;
  if (blocks >= 2147483647LL || (double)C * D * H * W >= 9.0e18)
    return tile_error(SPFF_ESHAPE, fn, "more than 2^31 workgroups");
  hipLaunchKernelGGL(k_tile_gather, dim3((unsigned)blocks), dim3(TL_GATHER_T), 0,
                     static_cast<hipStream_t>(stream), x, C, D, H, W, t, rd, rh, rw, total, out);
  return tile_hip(hipGetLastError());
}

int spff_tile_accumulate(const float* tiles, const int32_t* windows, int n, int rd, int rh, int rw,
                         int K, int D, int H, int W, const float* wz, const float* wy,
                         const float* wx, int softmax, float* acc, void* stream) {
  const char* fn = "spff_tile_accumulate";
  TileTable t;
  if (K < 2 || K > TL_MAX_K) return tile_error(SPFF_EINVAL, fn, "K must be 2..32");
  if (!tiles || !wz || !wy || !wx || !acc) return tile_error(SPFF_EINVAL, fn, "null argument");
  if (int rc = tile_table_check(fn, windows, n, rd, rh, rw, D, H, W, &t)) return rc;
  AccGeo g;
  g.n = n; g.rd = rd; g.rh = rh; g.rw = rw; g.K = K; g.D = D; g.H = H; g.W = W;
  int lo[3] = {t.w[0][0], t.w[0][1], t.w[0][2]}, hi[3] = {t.w[0][0], t.w[0][1], t.w[0][2]};
  for (int i = 1; i < n; ++i)
    for (int j = 0; j < 3; ++j) {
      lo[j] = t.w[i][j] < lo[j] ? t.w[i][j] : lo[j];
      hi[j] = t.w[i][j] > hi[j] ? t.w[i][j] : hi[j];
    }
  g.bz0 = lo[0]; g.by0 = lo[1]; g.bx0 = lo[2];
  g.bd = hi[0] - lo[0] + rd; g.bh = hi[1] - lo[1] + rh; g.bw = hi[2] - lo[2] + rw;
  g.gx = (g.bw + 63) / 64;
  const int64_t waves = (int64_t)g.bd * g.bh * g.gx;
  const int64_t blocks = (waves + TL_ACC_WAVES - 1) / TL_ACC_WAVES;
  if (blocks >= 2147483647LL) return tile_error(SPFF_ESHAPE, fn, "more than 2^31 workgroups");
  const size_t lds = (size_t)TL_ACC_WAVES * 2 * 64 * K * sizeof(float);
  hipLaunchKernelGGL(k_tile_accumulate, dim3((unsigned)blocks), dim3(TL_ACC_T), lds,
                     static_cast<hipStream_t>(stream), tiles, t, g, wz, wy, wx, softmax ? 1 : 0,
                     acc);
  return tile_hip(hipGetLastError());
}

int spff_tile_finalize(const float* acc, int D, int H, int W, int K, const float* nz,
                       const float* ny, const float* nx, float flips, uint8_t* mask,
                       float* scores, const int64_t* labels, int use_ignore, int ignore_index,
                       int64_t* conf, void* stream) {
  const char* fn = "spff_tile_finalize";
  if (K < 2 || K > TL_MAX_K) return tile_error(SPFF_EINVAL, fn, "K must be 2..32");
  if (!acc || !mask || (scores && (!nz || !ny || !nx)))
    return tile_error(SPFF_EINVAL, fn, "null argument");
  if ((labels == nullptr) != (conf == nullptr))
    return tile_error(SPFF_EINVAL, fn, "conf must be null exactly when labels is");
  if (D < 1 || H < 1 || W < 1) return tile_error(SPFF_EINVAL, fn, "an extent below 1");
  if (scores && !(flips >= 1.f)) return tile_error(SPFF_EINVAL, fn, "flips must be >= 1");
  hipStream_t s = static_cast<hipStream_t>(stream);
  FinGeo g;
  g.D = D; g.H = H; g.W = W; g.K = K;
  g.V = (int64_t)D * H * W;
  if (conf) {
    const hipError_t e = zero_async(conf, sizeof(int64_t) * K * (K + 1), s);
    if (e != hipSuccess) return tile_hip(e);
  }
  const int64_t want = (g.V + TL_FIN_T - 1) / TL_FIN_T;
  const unsigned grid = (unsigned)(want < (int64_t)TL_FIN_GRID ? want : (int64_t)TL_FIN_GRID);
  const size_t lds = (size_t)TL_FIN_WAVES * 64 * K * sizeof(float) +
                     (size_t)((K * (K + 1) + 3) & ~3) * sizeof(unsigned) + TL_FIN_T;
  hipLaunchKernelGGL(k_tile_finalize, dim3(grid), dim3(TL_FIN_T), lds, s, acc, g, nz, ny, nx,
                     flips, mask, scores, labels, use_ignore ? 1 : 0, ignore_index,
                     reinterpret_cast<unsigned long long*>(conf));
  return tile_hip(hipGetLastError());
}

}  // extern "C"
