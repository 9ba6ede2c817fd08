// 3x3x3 convolution weight gradient on the bf16 matrix cores with the exact
// 3-plane (bf16x6) or 2-plane (bf16x3) operand split of conv3d_x.hip.
//
// Replaces the weight gradient of nn.Conv3d(cin, cout, (ksd,3,3),
// padding=(ksd//2,1,1), bias=False) (reference models.py:616-618):
//   dW[co][ci][tap] = sum_v x[v + off(tap)][ci] * dy[v][co].
//
// MFMA v_mfma_f32_16x16x32_bf16 (f16x3: the fp16 one): rows = 16 (tap, channel) -- one tap
// x 16 channels (CI 16) or two taps x 8 (CI 8) -- cols = 16 out channels, k = 32 voxels
// = two W-rows of the 1 x 8 x 16 voxel tile.  Both operands need the voxel axis in
// their k slots while the LDS images are channel-last ([plane][pos][CI] halo,
// [plane][voxel][CO] dy tile, exactly as global memory): ds_read_b64_tr_b16 gathers
// them transposed -- every lane supplies the address of 4 contiguous channels of
// one voxel, so each row's tap offset and channel base are free per lane and no
// shifted copies are needed.
//
// 256 threads (4 waves), two workgroups per CU so one workgroup's staging (fp32
// loads, exact split, LDS stores) overlaps the other's MFMAs; the next tile's new
// halo plane / dy are register-prefetched during the current tile's MFMAs.
// Output: the fp32 partial slabs of conv3d.hip's wgrad
// ([split][tap][kpad][npad]), summed in fixed order by k_wgrad_reduce.
#include "spff_internal.h"
#include "bf16split.h"

#include <type_traits>

namespace spff {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short i16x4 __attribute__((ext_vector_type(4)));

static inline int cdiv(int a, int b) { return (a + b - 1) / b; }
static inline int rup(int a, int b) { return cdiv(a, b) * b; }

namespace {
constexpr int WX_TH = 8, WX_TW = 16, WX_TV = WX_TH * WX_TW, WX_CO = 32;
// k-step (W-row pair) loop unroll of k_conv3d_wgrad_x16
constexpr int WX_UNROLL = 4;
// the same for two-plane operands (bf16x3, f16x3): unrolled 4 deep the compiler hoists the
// fragment reads of later k-steps (fewer MFMAs per step) into 256 VGPRs + 11-23 spilled;
// 2 deep: 218 VGPRs, no spill
constexpr int WX_UNROLL2 = 2;

__device__ __forceinline__ unsigned short bfbits(__bf16 v) {
  return __builtin_bit_cast(unsigned short, v);
}
template <int NS>
__device__ __forceinline__ void split4(const float4& v, uint2 (&o)[nplanes(NS)]) {
  split4_pk<NS>(v, o);  // bf16split.h
}

typedef __attribute__((address_space(3))) i16x4 lds_i16x4;
__device__ __forceinline__ i16x4 tr_read(const unsigned short* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4*)(p));
}
__device__ __forceinline__ bf16x8 frag(const i16x4& lo, const i16x4& hi) {
  typedef short i16x8 __attribute__((ext_vector_type(8)));
  i16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8, v);
}
}  // namespace

// ------------------------------------------------------ 16x16x32 wgrad --
// CO (16 or 32): the Cout block of a workgroup; 16 for Cout <= 16 (the SwinUNETR's C = 12
// convs ran 12 of 32 columns)
// A workgroup walks 1 x 8 x 16 voxel tiles (WX_TH x WX_TW), staging each tile's halo
// ([plane][pos][CI]) and dy ([plane][voxel][CO]) fp32 -> split planes -> LDS through
// registers, and writes its sums as one fp32 partial slab [split][tap][kpad][npad].  The
// MFMA is v_mfma_f32_16x16x32_bf16: rows = 16 (tap, channel) -- one tap x 16 channels
// (CI 16) or two taps x 8 (CI 8), so 27 x 16 = 432 rows are 27 blocks with no
// padding, 7 / 7 / 7 / 6 over the 4 waves -- cols = 16 Cout (two col blocks of the 32),
// k = 32 voxels = two W-rows of the 1 x 8 x 16 tile.
// k-group g (lanes 16g..16g+15) takes W-row 2ks + (g >> 1), w = 8s + 4(g & 1) + q
// for read s = 0, 1 and transpose row q: a 32-lane half then reads 8 consecutive
// halo positions (conflict-free on the channel-last [pos][CI] image), and B reads
// 8 consecutive voxels of the dy image whose 16-byte chunks are XOR-swizzled by
// voxel bit 2 (chunk ^= ((v >> 2) & 1) << 1) so those 8 rows of 64 B hit 64
// distinct banks.
// HR: height-sharded input (the stencil's rows h = -1 / h = H from Src2::rlo / rhi, as in
// k_conv3d_fwd_x); a separate instantiation
// ACT: x is y1 read through the fused input activation (x.al / x.de: lrelu(IN(y1)), the
// 32-channel convs of conv3d_fuses_act) -- a separate instantiation, so the plain kernels
// carry neither its per-tile coefficient loads nor its validity bookkeeping
template <int KD, int CI, int NS, int NJMAX, bool HR, int CO, bool ACT>
__global__ __launch_bounds__(256, 2) void k_conv3d_wgrad_x16(
    Src2 x, const float* __restrict__ dy, int lddy, float* __restrict__ part, Vol vol, int Cin,
    int kpad, int Cout, int npad, int tilesH, int tilesW, int ntiles, int tps, int nblk,
    const unsigned* __restrict__ xmx, const unsigned* __restrict__ ymx) {
  constexpr int HD = KD, HH = WX_TH + 2, HWD = WX_TW + 2;
  constexpr int NPOS = HD * HH * HWD;
  constexpr int T = KD * 9;
  constexpr int CQ = CI / 4;                              // float4 per halo position
  constexpr int PPOS = HH * HWD;                           // positions per depth plane
  constexpr int NP = (PPOS * CQ + 255) / 256;              // plane float4 per thread
  constexpr int NY = WX_TV * (CO / 4) / 256;            // dy float4 per thread (= 4)
  constexpr int NCB = CO / 16;                          // 16-wide col blocks (2)
  // operand planes; HF: two fp16 planes of the scaled operands (NS_F16, bf16split.h)
  constexpr int NPL = nplanes(NS);
  constexpr bool HF = NS == NS_F16;
  // R4 (f16x3, 3x3x3): a 4-slot plane ring and two dy buffers (78 KB, still two
  // workgroups per CU), so the next tile's plane and dy go to slots the current tile does
  // not read: one barrier per tile instead of the write-after-read pair
  constexpr bool R4 = HF && KD == 3;
  constexpr int NSL = R4 ? 4 : KD;           // plane slots of the halo ring
  constexpr int NPOSA = NSL * PPOS;          // halo image positions per split plane
  constexpr int YB = NPL * WX_TV * CO;       // one dy buffer (elements)
  __shared__ __attribute__((aligned(16))) unsigned short Xs[NPL * NPOSA * CI];
  __shared__ __attribute__((aligned(16))) unsigned short Ys[(R4 ? 2 : 1) * YB];
  int ybuf = 0;  // dy buffer of the current tile (R4)
  // HF: x scaled by 2^ex (*xmx: max |x|), dy by 2^ey (*ymx: max |dy|)
  const int ex = HF ? f16_scale_exp(*xmx) : 0;
  const int ey = HF ? f16_scale_exp(*ymx) : 0;
  const float sx = exp2i(ex), sy = exp2i(ey);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, q = (lane & 15) >> 2, pq = lane & 3;
  // XCD-aware order: blocks b and b + 8 share an XCD, so XCD group b % 8 runs the
  // (ci, co) blocks of one voxel range back to back -- every x / dy tile is fetched
  // from HBM once and re-read by the other channel blocks from that XCD's L2
  const int nci = kpad / CI, ncb = nci * (npad / CO);
  const int rk = blockIdx.x >> 3;
  const int cbk = rk % ncb;
  const int split = (rk / ncb) * 8 + (blockIdx.x & 7);
  if (split * tps >= ntiles) return;  // padding block (uniform)
  const int ci_base = (cbk % nci) * CI, co0 = (cbk / nci) * CO;
  const int D = vol.D, H = vol.H, W = vol.W;

  // row blocks of this wave: wave, wave + 4, ...; nj of them (uniform per wave)
  const int nj = (nblk - wave + 3) / 4;
  // lane-constant A address (elements; plane 0, k-step 0, read 0) per block: transpose
  // column block pq = rows 4pq..4pq+3 of the block = tap (16 blk + 4pq) / CI, channels
  // (16 blk + 4pq) % CI ..; transpose row q = voxel (W-row g >> 1, w 4(g & 1) + q)
  int aoff[NJMAX];
#pragma unroll
  for (int j = 0; j < NJMAX; ++j) {
    const int r0 = 16 * (wave + 4 * j) + 4 * pq;
    int t = r0 / CI;
    const int ch0 = r0 % CI;
    if (t >= T) t = 0;  // padding rows: any valid address (never stored)
    const int kd = t / 9, kh = (t / 3) % 3, kw = t % 3;
    aoff[j] = ((kd * HH + kh + (g >> 1)) * HWD + kw + 4 * (g & 1) + q) * CI + ch0;
  }
  // B: voxel (W-row g >> 1, w 4(g & 1) + q), co 16 cb + 4 pq, chunk-swizzled
  const int bsw = CO == 32 ? (g & 1) << 1 : 0;  // (16-wide rows: 32 B, no swizzle)
  const int bv = (g >> 1) * WX_TW + 4 * (g & 1) + q;
  int boff[NCB];
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb)
    boff[cb] = bv * CO + (((2 * cb + (pq >> 1)) ^ bsw) << 3) + 4 * (pq & 1);

  f32x4 acc[NJMAX][NCB];
#pragma unroll
  for (int j = 0; j < NJMAX; ++j)
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[j][cb][r] = 0.f;

  // Rolling depth-plane halo: tiles run depth-fastest, so tile d0 + 1 of the same
  // (b, h, w) column needs only ONE new plane (gd = d0 + 1 + KD / 2) beside the KD - 1
  // it shares with tile d0.  Plane gd lives in slot (gd + 3) % KD of the halo image; the
  // register pipeline carries one plane (+ dy) per tile, and a column's first tile
  // stages its other KD - 1 planes synchronously.
  float4 hreg[NP], yreg[NY];
  float4 xal = make_float4(1.f, 1.f, 1.f, 1.f), xde = make_float4(0.f, 0.f, 0.f, 0.f);
  const int tbeg = split * tps;
  const int tend = min(ntiles, tbeg + tps);
  // The tile the register pipeline fetches, walked incrementally: decoded once, then d0 + 1
  // per tile and a roll-over to the next (b, h, w) column by compares and adds (uniform).
  int wb, wthi, wtwi, wd0;
  {
    int t = tbeg;
    wd0 = t % D; t /= D;
    wtwi = t % tilesW; t /= tilesW;
    wthi = t % tilesH;
    wb = t / tilesH;
  }
  // Column-invariant load state.  Within a column only the depth plane moves, so every
  // h / w / channel test, the Src2 pointer choice and the in-plane offsets are taken once
  // per column (set_column): a lane's x loads are xcol (its batch, source and channel quad)
  // + plane * xpl + xo[k], its dy loads the uniform ycol + plane * ypl (+ a uniform row
  // stride per k) + yo.  Invalid positions load from a clamped valid address of the same
  // column and are zeroed at the stash (hmc / yl, ymk), depth validity is uniform: no load
  // is conditional.  (Byte offsets in 32 bits: the host checks the plane sizes.)
  constexpr int YC4 = CO / 4;                  // dy float4 per voxel
  constexpr int YRS = 256 / YC4 / WX_TW;       // tile rows between a thread's dy loads
  const int yrw = __builtin_amdgcn_readfirstlane(tid / (YC4 * WX_TW));  // its first row
  const char* xcol = nullptr;
  const char* ycol = nullptr;
  const char* rlc = nullptr;   // HR: the boundary rows of this column's batch
  const char* rhc = nullptr;
  int xpl = 0;                 // bytes per depth plane of this lane's x source
  const int ypl = H * W * lddy * 4;
  const int yrs = YRS * W * lddy * 4;
  uint32_t xo[NP], yo = 0;
  unsigned hmc = 0;            // bit k: load k is a valid (not padding) position
  unsigned rlm = 0, rhm = 0;   // HR: bit k: load k reads x.rlo / x.rhi
  unsigned ymk = 0;            // bit k: dy load k is a row inside the volume (uniform)
  bool yl = false;             // this lane's dy column and channels are inside
  auto set_column = [&]() {
    const int b = wb, h0 = wthi * WX_TH, w0 = wtwi * WX_TW;
    const int c = ci_base + 4 * (tid % CQ);
    const bool cv = c < Cin;
    const int cc = cv ? c : 0;
    const bool s0 = cc < x.split;
    const int ldl = s0 ? x.ld0 : x.ld1;
    xcol = reinterpret_cast<const char*>((s0 ? x.p0 + cc : x.p1 + (cc - x.split)) +
                                         (int64_t)b * D * H * W * ldl);
    xpl = H * W * ldl * 4;
    if constexpr (HR) {
      rlc = reinterpret_cast<const char*>(x.rlo + (int64_t)b * D * W * x.ldr);
      rhc = reinterpret_cast<const char*>(x.rhi + (int64_t)b * D * W * x.ldr);
    }
    if constexpr (ACT) {
      // the fused activation's coefficients of this column's batch and this thread's 4
      // channels (a clamped channel where c >= Cin)
      const int64_t o = (int64_t)b * x.ld0 + cc;
      xal = *reinterpret_cast<const float4*>(x.al + o);
      xde = *reinterpret_cast<const float4*>(x.de + o);
    }
    hmc = 0; rlm = 0; rhm = 0;
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      const int i = tid + 256 * k;
      const int pos = i / CQ;
      const int hw = pos % HWD, hh = pos / HWD;
      const int gh = h0 + hh - 1, gw = w0 + hw - 1;
      const bool wc = i < PPOS * CQ && (unsigned)gw < (unsigned)W && cv;
      uint32_t o = (uint32_t)((h0 * W + w0) * ldl * 4);  // (the tile's first voxel: valid)
      if (wc && (unsigned)gh < (unsigned)H) {
        o = (uint32_t)((gh * W + gw) * ldl * 4);
        hmc |= 1u << k;
      }
      if constexpr (HR) {
        if (wc && ((gh == -1 && x.rlo) || (gh == H && x.rhi))) {
          o = (uint32_t)((gw * x.ldr + c) * 4);
          hmc |= 1u << k;
          if (gh < 0) rlm |= 1u << k; else rhm |= 1u << k;
        }
      }
      xo[k] = o;
    }
    // dy: voxel kv = tid / YC4 + k * (256 / YC4) = row yrw + k YRS, column (tid / YC4) % 16
    const int hv = min(WX_TH, H - h0);
    const int col = (tid / YC4) % WX_TW, c4 = tid % YC4;
    const bool wv = w0 + col < W, ov = co0 + 4 * c4 < Cout;
    yl = wv && ov;
    yo = (uint32_t)(((min(yrw, hv - 1) * W + (wv ? col : 0)) * lddy + (ov ? 4 * c4 : 0)) * 4);
    ymk = 0;
#pragma unroll
    for (int k = 0; k < NY; ++k)
      if (yrw + YRS * k < hv) ymk |= 1u << k;
    ycol = reinterpret_cast<const char*>(dy + ((((int64_t)b * D) * H + h0) * W + w0) * lddy + co0);
  };
  // the walker's next tile; true where it starts a new column
  auto advance = [&]() {
    if (++wd0 < D) return false;
    wd0 = 0;
    if (++wtwi == tilesW) {
      wtwi = 0;
      if (++wthi == tilesH) { wthi = 0; ++wb; }
    }
    return true;
  };
  // (the fused input activation is applied at the store, not here: applied to each load as
  // it arrived, it made the prefetch wait for every load in turn before the MFMAs)
  unsigned hm = 0;  // bit k: hreg[k] is a valid (not padding) position
  // depth plane gd of the walker's column (a clamped plane where gd is padding: m = 0)
  auto load_plane = [&](int gd, float4 (&r)[NP], unsigned& m) {
    const bool dv = (unsigned)(gd + vol.dh) < (unsigned)(D + 2 * vol.dh) &&
                    !((gd < 0 && x.zlo) || (gd >= D && x.zhi));
    const int gdc = dv ? gd : min(max(gd, 0), D - 1);
    const char* xt = xcol + (int64_t)gdc * xpl;
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      const char* p = xt;
      if constexpr (HR) {
        const int64_t ro = (int64_t)gdc * (W * x.ldr * 4);
        if ((rlm >> k) & 1u) p = rlc + ro;
        if ((rhm >> k) & 1u) p = rhc + ro;
      }
      r[k] = *reinterpret_cast<const float4*>(p + xo[k]);
    }
    m = dv ? hmc : 0u;
  };
  auto store_plane = [&](int gd, const float4 (&r)[NP], unsigned m) {
    unsigned short* dst = Xs + (R4 ? ((gd + 4) & 3) : ((gd + 3) % KD)) * PPOS * CI;
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      const int i = tid + 256 * k;
      if (i < PPOS * CQ) {
        uint2 o[NPL];
        float4 v = r[k];
        if constexpr (ACT) {  // lrelu(IN(y)) (of valid positions: padding is zeroed below)
          v.x = v.x * xal.x + xde.x; v.x = v.x > 0.f ? v.x : 0.01f * v.x;
          v.y = v.y * xal.y + xde.y; v.y = v.y > 0.f ? v.y : 0.01f * v.y;
          v.z = v.z * xal.z + xde.z; v.z = v.z > 0.f ? v.z : 0.01f * v.z;
          v.w = v.w * xal.w + xde.w; v.w = v.w > 0.f ? v.w : 0.01f * v.w;
        }
        // padding positions were loaded from a clamped address: zero
        if (!((m >> k) & 1u)) v = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (HF) v = make_float4(v.x * sx, v.y * sx, v.z * sx, v.w * sx);
        split4<NS>(v, o);
#pragma unroll
        for (int p = 0; p < NPL; ++p)
          *reinterpret_cast<uint2*>(dst + p * NPOSA * CI + 4 * i) = o[p];
      }
    }
  };
  // the walker's tile: its new plane and its dy, from a uniform base + the lane's offset
  auto fetch = [&]() {
    load_plane(wd0 + KD / 2, hreg, hm);
    const char* yt = ycol + (int64_t)wd0 * ypl;
#pragma unroll
    for (int k = 0; k < NY; ++k) {
      const char* yk = yt + (((ymk >> k) & 1u) ? k * yrs : 0);  // (rows past H: row 0)
      yreg[k] = *reinterpret_cast<const float4*>(yk + yo);
    }
  };
  auto stash = [&](int d0, bool negate, int yb) {
    store_plane(d0 + KD / 2, hreg, hm);
#pragma unroll
    for (int k = 0; k < NY; ++k) {
      const int i = tid + 256 * k;
      const int c4 = i % (CO / 4), kv = i / (CO / 4);
      uint2 o[NPL];
      const float ys = HF ? (negate ? -sy : sy) : (negate ? -1.f : 1.f);
      // (voxels and channels outside were loaded from a clamped address: zero)
      const float4 yr = (yl && ((ymk >> k) & 1u)) ? yreg[k] : make_float4(0.f, 0.f, 0.f, 0.f);
      const float4 yv = make_float4(yr.x * ys, yr.y * ys, yr.z * ys, yr.w * ys);
      split4<NS>(yv, o);
      const int off = kv * CO + (((c4 >> 1) ^ (CO == 32 ? ((kv >> 2) & 1) << 1 : 0)) << 3) + 4 * (c4 & 1);
#pragma unroll
      for (int p = 0; p < NPL; ++p)
        *reinterpret_cast<uint2*>(Ys + yb * YB + p * WX_TV * CO + off) = o[p];
    }
  };

  auto compute = [&](auto NJc, int d0) {
    constexpr int NJ = decltype(NJc)::value;
    // aoff[j] addresses plane kd as slot kd; tap kd reads gd = d0 + kd - KD / 2, in slot
    // (kd + rot) % KD with rot = (d0 - KD / 2 + 3) % KD
    // (R4: tap kd reads gd = d0 + kd - 1 in slot (gd + 4) & 3)
    constexpr int PL = PPOS * CI;
    const int rot = (d0 - KD / 2 + 3) % KD;
    int ab[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      if constexpr (R4) {
        const int kd = aoff[j] >= 2 * PL ? 2 : aoff[j] >= PL ? 1 : 0;
        ab[j] = aoff[j] + (((d0 + kd + 3) & 3) - kd) * PL;
      } else {
        ab[j] = aoff[j] + (aoff[j] >= (KD - rot) * PL ? (rot - KD) * PL : rot * PL);
      }
    }
    const unsigned short* Yc = Ys + (R4 ? ybuf * YB : 0);
    constexpr int KSU = NPL == 2 ? WX_UNROLL2 : WX_UNROLL;
#pragma unroll KSU
    for (int ks = 0; ks < WX_TH / 2; ++ks) {
      bf16x8 bq[NCB][NPL];
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
        for (int p = 0; p < NPL; ++p) {
          const unsigned short* yb = Yc + p * WX_TV * CO + 2 * ks * WX_TW * CO + boff[cb];
          bq[cb][p] = frag(tr_read(yb), tr_read(yb + 8 * CO));
        }
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        bf16x8 aq[NPL];
#pragma unroll
        for (int p = 0; p < NPL; ++p) {
          const unsigned short* xb = Xs + p * NPOSA * CI + 2 * ks * HWD * CI + ab[j];
          aq[p] = frag(tr_read(xb), tr_read(xb + 8 * CI));
        }
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) {
          f32x4 c = acc[j][cb];
          if constexpr (NPL == 3) {
            c = mfma16x32<HF>(aq[1], bq[cb][1], c);
            c = mfma16x32<HF>(aq[0], bq[cb][2], c);
            c = mfma16x32<HF>(aq[2], bq[cb][0], c);
          }
          if constexpr (NPL >= 2) {
            c = mfma16x32<HF>(aq[0], bq[cb][1], c);
            c = mfma16x32<HF>(aq[1], bq[cb][0], c);
          }
          c = mfma16x32<HF>(aq[0], bq[cb][0], c);
          acc[j][cb] = c;
        }
      }
    }
  };

  // first tile of a column (the walker's): its other planes d0 - KD / 2 .. d0 + KD / 2 - 1
  auto stage_column = [&](int d0) {
#pragma unroll
    for (int hd = 0; hd < KD - 1; ++hd) {
      float4 r[NP];
      unsigned m;
      load_plane(d0 + hd - KD / 2, r, m);
      store_plane(d0 + hd - KD / 2, r, m);
    }
  };
  // Every iteration fetches unconditionally: after the last tile the walker stays where it
  // is, and the dummy fetch reloads that tile (valid addresses, never stashed).
  set_column();
  if constexpr (R4) {
    // tile t computes from ring slots and dy buffer (t - tbeg) & 1, while tile t + 1's
    // plane / dy are fetched and stored to the slot / buffer it does not read; a new
    // column's two extra planes overwrite slots the tile before may read: one more barrier
    fetch();
    stage_column(wd0);
    stash(wd0, false, 0);
    for (int tile = tbeg; tile < tend; ++tile) {
      if (tile != tbeg) {
#pragma unroll
        for (int j = 0; j < NJMAX; ++j)
#pragma unroll
          for (int cb = 0; cb < NCB; ++cb) acc[j][cb] = -acc[j][cb];
      }
      __syncthreads();  // this tile's plane / dy visible; every wave is past tile - 1
      const int d0 = wd0;
      ybuf = (tile - tbeg) & 1;
      const bool more = tile + 1 < tend;
      bool newcol = false;
      if (more) {
        newcol = advance();
        if (newcol) set_column();
      }
      fetch();
      if (nj == NJMAX) compute(std::integral_constant<int, NJMAX>{}, d0);
      else if constexpr (NJMAX > 1) compute(std::integral_constant<int, NJMAX - 1>{}, d0);
      if (more) {
        if (newcol) {
          __syncthreads();  // every wave is past this tile's reads of the ring
          stage_column(wd0);
        }
        stash(wd0, ((tile + 1 - tbeg) & 1) != 0, ybuf ^ 1);
      }
    }
  } else {
  fetch();
  for (int tile = tbeg; tile < tend; ++tile) {
    // sign-alternating accumulation (conv3d_x.hip)
    if (tile != tbeg) {
#pragma unroll
      for (int j = 0; j < NJMAX; ++j)
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) acc[j][cb] = -acc[j][cb];
    }
    __syncthreads();  // previous compute done reading LDS
    const int d0 = wd0;
    if (KD > 1 && (tile == tbeg || d0 == 0)) stage_column(d0);
    stash(d0, ((tile - tbeg) & 1) != 0, 0);
    __syncthreads();
    if (tile + 1 < tend && advance()) set_column();
    fetch();
    if (nj == NJMAX) compute(std::integral_constant<int, NJMAX>{}, d0);
    else if constexpr (NJMAX > 1) compute(std::integral_constant<int, NJMAX - 1>{}, d0);
  }
  }

  if (tend > tbeg && ((tend - 1 - tbeg) & 1)) {
#pragma unroll
    for (int j = 0; j < NJMAX; ++j)
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb) acc[j][cb] = -acc[j][cb];
  }

  // partial slab [split][tap][kpad][npad]: output row 4 g + r of block blk = tap
  // (16 blk + row) / CI, channel (16 blk + row) % CI; col = co 16 cb + (lane & 15)
#pragma unroll
  for (int j = 0; j < NJMAX; ++j) {
    const int blk = wave + 4 * j;
    if (j >= nj || blk >= nblk) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * blk + 4 * g + r;
      const int t = row / CI;
      if (t >= T) continue;
      const int ci = ci_base + row % CI;
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb)
        part[(((int64_t)split * T + t) * kpad + ci) * npad + co0 + 16 * cb + (lane & 15)] =
            HF ? ldexpf(acc[j][cb][r], -(ex + ey)) : acc[j][cb][r];
    }
  }
}

// ------------------------------------------------------------------ host --
namespace {
struct WxPlan {
  int ci, co, kpad, npad, tilesH, tilesW, ntiles, nsplit, tps;
};
WxPlan wx_plan(Vol vol, int Cin, int Cout) {
  WxPlan p;
  p.ci = Cin <= 8 ? 8 : 16;
  p.co = Cout <= 16 ? 16 : WX_CO;
  p.kpad = rup(Cin, p.ci);
  p.npad = rup(Cout, p.co);
  p.tilesH = cdiv(vol.H, WX_TH);
  p.tilesW = cdiv(vol.W, WX_TW);
  p.ntiles = vol.B * vol.D * p.tilesH * p.tilesW;
  const int nout = (p.kpad / p.ci) * (p.npad / p.co);
  // two workgroups per CU: aim at 2 rounds of 512, >= 4 tiles per workgroup.  A workgroup
  // runs tiles [split tps, split tps + tps) depth-fastest: it decodes its first tile once,
  // walks on by d0 + 1 / column roll-over, and re-derives its lanes' load offsets and masks
  // only where a column starts (k_conv3d_wgrad_x16: set_column)
  int nsplit = std::max(1, cdiv(1024, nout));
  nsplit = std::min(nsplit, std::max(1, p.ntiles / 4));
  p.tps = cdiv(p.ntiles, nsplit);
  p.nsplit = cdiv(p.ntiles, p.tps);
  return p;
}
}  // namespace

// partial slabs, then (SPFF_MATH_F16X3) the two operand-scale slots [max |x|, max |dy|]
static size_t wx_main_bytes(Vol vol, int KD, int Cin, int Cout) {
  WxPlan p = wx_plan(vol, Cin, Cout);
  return ((size_t)p.nsplit * KD * 9 * p.kpad * p.npad * sizeof(float) + 255) & ~(size_t)255;
}
size_t conv3d_wgrad_x_ws_bytes(Vol vol, int KD, int Cin, int Cout) {
  return wx_main_bytes(vol, KD, Cin, Cout) + 256;
}

hipError_t conv3d_wgrad_x(const Src2& x, const float* dy, int lddy, float* dw, Vol vol, int KD,
                          int Cin, int Cout, int math, float* ws, hipStream_t s,
                          const unsigned* xmax, const unsigned* ymax) {
  if (lddy % 4) return hipErrorInvalidValue;
  // k_conv3d_wgrad_x16 keeps a lane's byte offsets inside one depth plane in 32 bits
  const int64_t ldmax = std::max<int64_t>({x.ld0, x.ld1, lddy, x.rows() ? x.ldr : 0});
  if ((int64_t)vol.H * vol.W * ldmax * 4 >= ((int64_t)1 << 31)) return hipErrorInvalidValue;
  WxPlan p = wx_plan(vol, Cin, Cout);
  dim3 grid(8 * cdiv(p.nsplit, 8) * (p.kpad / p.ci) * (p.npad / p.co));
  const bool x3 = math == SPFF_MATH_BF16X3;
  const bool hf = math == SPFF_MATH_F16X3;
  unsigned* sl = reinterpret_cast<unsigned*>(reinterpret_cast<char*>(ws) +
                                             wx_main_bytes(vol, KD, Cin, Cout));
  if (hf) {  // operand maxima: the caller's precomputed slots, else computed here
    if (!xmax || !ymax) {
      hipError_t e = spff::zero_async(sl, 2 * sizeof(unsigned), s);
      if (e != hipSuccess) return e;
    }
    if (!xmax) {
      hipError_t e = absmax_src(x, vol, Cin, true, sl, s);
      if (e != hipSuccess) return e;
      xmax = sl;
    }
    if (!ymax) {
      hipError_t e = absmax_src(src1(dy, lddy), vol, Cout, false, sl + 1, s);
      if (e != hipSuccess) return e;
      ymax = sl + 1;
    }
  }
  // 16-row blocks: nblk = ceil(T CI / 16); NJMAX = ceil(nblk / 4):
  // KD3/CI16 27 -> 7, KD3/CI8 14 -> 4, KD1/CI16 9 -> 3, KD1/CI8 5 -> 2
  const int nblk = cdiv(KD * 9 * p.ci, 16);
  // (the fused input activation only on 32-wide output tiles: conv3d_fuses_act's C = 32)
  if (x.al && p.co != 32) return hipErrorInvalidValue;
#define WX_LAUNCH_C(KD_, CI_, NS_, NJ_, HR_, CO_, ACT_)                                          \
  hipLaunchKernelGGL((k_conv3d_wgrad_x16<KD_, CI_, NS_, NJ_, HR_, CO_, ACT_>), grid, dim3(256),  \
                     0, s, x, dy, lddy, ws, vol, Cin, p.kpad, Cout, p.npad, p.tilesH, p.tilesW,  \
                     p.ntiles, p.tps, nblk, xmax, ymax)
#define WX_LAUNCH(KD_, CI_, NS_, NJ_)                                                            \
  do {                                                                                           \
    if (p.co == 16) {                                                                            \
      if (x.rows()) WX_LAUNCH_C(KD_, CI_, NS_, NJ_, true, 16, false);                            \
      else WX_LAUNCH_C(KD_, CI_, NS_, NJ_, false, 16, false);                                    \
    } else if (x.al) {                                                                           \
      if (x.rows()) WX_LAUNCH_C(KD_, CI_, NS_, NJ_, true, 32, true);                             \
      else WX_LAUNCH_C(KD_, CI_, NS_, NJ_, false, 32, true);                                     \
    } else {                                                                                     \
      if (x.rows()) WX_LAUNCH_C(KD_, CI_, NS_, NJ_, true, 32, false);                            \
      else WX_LAUNCH_C(KD_, CI_, NS_, NJ_, false, 32, false);                                    \
    }                                                                                            \
  } while (0)
  if (KD == 3) {
    if (p.ci == 16) {
      if (hf) WX_LAUNCH(3, 16, NS_F16, 7);
      else if (x3) WX_LAUNCH(3, 16, 2, 7);
      else WX_LAUNCH(3, 16, 3, 7);
    } else {
      if (hf) WX_LAUNCH(3, 8, NS_F16, 4);
      else if (x3) WX_LAUNCH(3, 8, 2, 4);
      else WX_LAUNCH(3, 8, 3, 4);
    }
  } else {
    if (p.ci == 16) {
      if (hf) WX_LAUNCH(1, 16, NS_F16, 3);
      else if (x3) WX_LAUNCH(1, 16, 2, 3);
      else WX_LAUNCH(1, 16, 3, 3);
    } else {
      if (hf) WX_LAUNCH(1, 8, NS_F16, 2);
      else if (x3) WX_LAUNCH(1, 8, 2, 2);
      else WX_LAUNCH(1, 8, 3, 2);
    }
  }
#undef WX_LAUNCH
#undef WX_LAUNCH_C
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return conv3d_wgrad_reduce(ws, dw, p.nsplit, KD * 9, p.kpad, p.npad, Cin, Cout, s);
}

}  // namespace spff
