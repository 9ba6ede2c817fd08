// Exact, tie-aware ranking metrics on the device: the PR-AUC and ROC-AUC of the
// reference's test-only block (BaseLitModel._shared_step, models.py:510-584; per volume
// in train.py:773-798), which the reference computes with scikit-learn on the host
// (precision_recall_curve + auc, roc_auc_score), one sort per class.
//
// A segment is the set of (score, is_positive) pairs of one class over the whole batch
// (pooled), of one (sample, class), or -- the micro row, models.py:552-563 -- of the
// classes 1..K-1 concatenated.  Per segment:
//   1. k_rank_keys: softmax of the row (max-subtracted expf as in k_dice_grad and k_loss,
//      but divided as torch divides) and key = (fp32 bits of the score << 1) | is_positive.
//      A score is finite and >= 0, so its top bit is clear and the unsigned key order is
//      the score order;
//      the positives of every segment are counted with integer atomics.
//   2. four LSD radix passes of 8 bits over ping-pong key buffers.  A tile of the segment
//      belongs to one workgroup: k_rank_hist counts its digits in LDS, k_rank_scan turns
//      the segment's [digit][tile] counts into start offsets, k_rank_scatter ranks the keys
//      of a tile stably (wave match by ballots, per-wave running digit counts in LDS) and
//      stores them.  A segment of one tile needs no counts in memory: its workgroup scans
//      its own histogram.
//   3. one pass over the sorted keys from the highest score down: an inclusive sum-scan of
//      the positive bit and a max-scan of (group start, positives before it), whose
//      carries cross workgroups through k_rank_curve<false> (a tile's totals) and
//      k_rank_carry (their scan over the tiles).  At the last key of every group of equal
//      scores k_rank_curve<true> adds
//        roc: (fp_g - fp_{g-1}) (tp_g + tp_{g-1})               exact 64-bit integers
//        pr : (tp_g - tp_{g-1}) / P * (p_g + p_{g-1}) / 2       fp64, p_0 = 1
//      The integer sum is order-free; the fp64 terms are reduced by a fixed tree per tile
//      and k_rank_final adds the tiles in index order, so two runs give the same bits.
// Segments without a positive or without a negative are skipped after step 1 (NaN rows).
// No host synchronisation, no allocation: all state lives in the caller's workspace.
#include "spff_internal.h"
#include <math.h>

namespace spff {

namespace {

typedef unsigned long long u64;

constexpr int RK_T = 256;          // threads per workgroup
constexpr int RK_WAVES = RK_T / 64;
constexpr int RK_SUB = 4 * RK_T;   // keys per workgroup step, four per thread
constexpr int RK_UNIT = 4096;      // a tile is a multiple of this many keys
constexpr int RK_STAGE_K = 32;     // rows are staged in LDS up to this K (32 KiB)

// Segments 0 .. nu-1 have ulen keys each and lie back to back; segment nu (the micro row,
// pooled mode) follows them with mlen keys.  Tiles of `tile` keys, one workgroup each:
// workgroup s * utps + t is tile t of segment s, the micro segment's tiles come last.
struct RankGeo {
  int K, nu, per_sample;
  int64_t ulen, mlen, tile, utps, mtps, nblk, total;
  int64_t hist_entries;                               // 256 per tile of a multi-tile segment
  size_t off_b, off_hist, off_npos, off_roc, off_tile, bytes;  // workspace layout
  bool multi;                                         // some segment has more than one tile
};

struct RankSeg {
  int64_t seg, t, off, len, tps, tbase, hbase;
};

__host__ __device__ inline RankSeg rank_seg_of(const RankGeo& g, int64_t seg) {
  RankSeg r;
  r.seg = seg;
  r.t = 0;
  if (seg < g.nu) {
    r.off = seg * g.ulen; r.len = g.ulen; r.tps = g.utps;
    r.tbase = seg * g.utps;
    r.hbase = seg * g.utps * 256;
  } else {
    r.off = (int64_t)g.nu * g.ulen; r.len = g.mlen; r.tps = g.mtps;
    r.tbase = (int64_t)g.nu * g.utps;
    r.hbase = g.utps > 1 ? (int64_t)g.nu * g.utps * 256 : 0;
  }
  return r;
}

__device__ __forceinline__ RankSeg rank_seg_of_block(const RankGeo& g) {
  const int64_t blk = blockIdx.x;
  const int64_t nub = (int64_t)g.nu * g.utps;
  RankSeg r = rank_seg_of(g, blk < nub ? blk / g.utps : g.nu);
  r.t = blk < nub ? blk % g.utps : blk - nub;
  return r;
}

// a segment with no positive or no negative has no curve
__device__ __forceinline__ bool rank_skip(const u64* npos, const RankSeg& s) {
  const u64 P = npos[s.seg];
  return P == 0 || P == (u64)s.len;
}

__device__ __forceinline__ u64 shfl_up64(u64 v, int d) {
  const unsigned lo = __shfl_up((unsigned)v, (unsigned)d);
  const unsigned hi = __shfl_up((unsigned)(v >> 32), (unsigned)d);
  return ((u64)hi << 32) | lo;
}

// Scan over the workgroup's RK_T values in thread order (sum, or max of unsigned values:
// identity 0 for both): excl = the scan of the threads before this one, total = all.
// Every thread calls it; sm holds RK_WAVES values and is free again on return.
template <bool MAX>
__device__ __forceinline__ void block_scan(u64 v, u64* sm, u64& excl, u64& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  u64 inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const u64 t = shfl_up64(inc, d);
    if (lane >= d) inc = MAX ? (t > inc ? t : inc) : inc + t;
  }
  u64 prev = shfl_up64(inc, 1);
  if (lane == 0) prev = 0;
  if (lane == 63) sm[w] = inc;
  __syncthreads();
  u64 wp = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < RK_WAVES; ++i) {
    const u64 x = sm[i];
    if (i < w) wp = MAX ? (x > wp ? x : wp) : wp + x;
    tot = MAX ? (x > tot ? x : tot) : tot + x;
  }
  __syncthreads();
  excl = MAX ? (prev > wp ? prev : wp) : wp + prev;
  total = tot;
}

// ---------------------------------------------------------------- 1. the keys ---
// One wave per 64 consecutive voxels of a sample, a lane per voxel.  Up to RK_STAGE_K the
// rows go through the wave's LDS slice (coalesced loads, as k_dice_grad); above it each
// lane reads its row from memory.  Key stores are coalesced per class.
__global__ __launch_bounds__(RK_T) void k_rank_keys(const float* __restrict__ x,
                                                    const int64_t* __restrict__ lab, int64_t V,
                                                    int K, int from_logits, int per_sample,
                                                    int64_t n, int gx, int stage,
                                                    unsigned* __restrict__ keys,
                                                    u64* __restrict__ npos) {
  extern __shared__ __attribute__((aligned(16))) float rsm[];
  __shared__ unsigned pc[SPFF_MAX_CLASSES];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t b = blockIdx.x / gx;
  const int bx = blockIdx.x % gx;
  float* sx = rsm + (size_t)wv * 64 * K;
  for (int i = threadIdx.x; i < K; i += RK_T) pc[i] = 0;
  __syncthreads();
  const int64_t ngroups = (V + 63) / 64;
  for (int64_t grp = (int64_t)bx * RK_WAVES + wv; grp < ngroups; grp += (int64_t)gx * RK_WAVES) {
    const int64_t v0 = grp * 64;
    const int nv = (int)(V - v0 < 64 ? V - v0 : 64);
    const float* rows = x + (b * V + v0) * K;
    if (stage) {
      wave_copy_rows(sx, rows, nv * K, lane);
      wave_lds_sync();
    }
    if (lane < nv) {
      const float* xr = stage ? sx + lane * K : rows + (int64_t)lane * K;
      const int64_t gv = b * V + v0 + lane;
      const int64_t y = lab[gv];
      const int yi = (y >= 0 && y < K) ? (int)y : -1;  // any other label: a negative
      if (yi >= 0) atomicAdd(&pc[yi], 1u);
      // softmax as torch computes it on the host (the reference's probs, models.py:512):
      // exp(x - max) summed in class order, then a true division -- not the reciprocal
      // multiply of the loss kernels, which rounds differently and would split or merge
      // groups of equal scores that the reference sees
      float m = 0.f, ssum = 1.f;
      if (from_logits) {
        m = -INFINITY;
        for (int k = 0; k < K; ++k) m = fmaxf(m, xr[k]);
        ssum = 0.f;
        for (int k = 0; k < K; ++k) ssum += expf(xr[k] - m);
      }
      for (int k = 0; k < K; ++k) {
        const float p = from_logits ? expf(xr[k] - m) / ssum : xr[k];
        unsigned bits = __float_as_uint(p);
        if (bits == 0x80000000u) bits = 0u;  // -0.0 ranks as +0.0
        const unsigned key = (bits << 1) | (k == yi ? 1u : 0u);
        if (per_sample) {
          keys[(b * K + k) * V + v0 + lane] = key;
        } else {
          keys[(int64_t)k * n + gv] = key;
          if (k >= 1) keys[(int64_t)(K + k - 1) * n + gv] = key;
        }
      }
    }
    if (stage) wave_lds_sync();  // the next group overwrites the slice
  }
  __syncthreads();
  for (int c = threadIdx.x; c < K; c += RK_T) {
    const unsigned cnt = pc[c];
    if (!cnt) continue;
    atomicAdd(&npos[per_sample ? b * K + c : (int64_t)c], (u64)cnt);
    if (!per_sample && c >= 1) atomicAdd(&npos[K], (u64)cnt);
  }
}

// ------------------------------------------------------------- 2. the radix sort ---
__global__ __launch_bounds__(RK_T) void k_rank_hist(RankGeo g, const unsigned* __restrict__ in,
                                                    int shift, const u64* __restrict__ npos,
                                                    unsigned* __restrict__ hist) {
  const RankSeg s = rank_seg_of_block(g);
  if (s.tps <= 1 || rank_skip(npos, s)) return;
  __shared__ unsigned h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  const int64_t j0 = s.t * g.tile;
  const int64_t j1 = j0 + g.tile < s.len ? j0 + g.tile : s.len;
  for (int64_t j = j0 + threadIdx.x; j < j1; j += RK_T)
    atomicAdd(&h[(in[s.off + j] >> shift) & 255u], 1u);
  __syncthreads();
  hist[s.hbase + (int64_t)threadIdx.x * s.tps + s.t] = h[threadIdx.x];
}

// in place: counts [digit][tile] of one segment -> the position, inside the segment, of the
// first key of that tile with that digit
__global__ __launch_bounds__(RK_T) void k_rank_scan(RankGeo g, const u64* __restrict__ npos,
                                                    unsigned* __restrict__ hist) {
  const RankSeg s = rank_seg_of(g, blockIdx.x);
  if (s.tps <= 1 || rank_skip(npos, s)) return;
  __shared__ u64 sm[RK_WAVES];
  unsigned* h = hist + s.hbase;
  const int64_t E = 256 * s.tps;
  u64 carry = 0;
  for (int64_t base = 0; base < E; base += RK_SUB) {
    const int64_t i0 = base + 4 * (int64_t)threadIdx.x;
    unsigned v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = i0 + i < E ? h[i0 + i] : 0u;
    u64 ex, tot;
    block_scan<false>((u64)v[0] + v[1] + v[2] + v[3], sm, ex, tot);
    u64 run = carry + ex;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i0 + i < E) h[i0 + i] = (unsigned)run;
      run += v[i];
    }
    carry += tot;
  }
}

__global__ __launch_bounds__(RK_T) void k_rank_scatter(RankGeo g, const unsigned* __restrict__ in,
                                                       unsigned* __restrict__ out, int shift,
                                                       const u64* __restrict__ npos,
                                                       const unsigned* __restrict__ hist) {
  const RankSeg s = rank_seg_of_block(g);
  if (rank_skip(npos, s)) return;
  __shared__ unsigned run[256];             // next position of each digit, in the segment
  __shared__ unsigned wcnt[RK_WAVES][256];  // per-wave digit counts, then start positions
  __shared__ u64 sm[RK_WAVES];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t j0 = s.t * g.tile;
  const int64_t j1 = j0 + g.tile < s.len ? j0 + g.tile : s.len;
  const unsigned* kin = in + s.off;
  if (s.tps > 1) {
    run[threadIdx.x] = hist[s.hbase + (int64_t)threadIdx.x * s.tps + s.t];
  } else {
    run[threadIdx.x] = 0;
    __syncthreads();
    for (int64_t j = j0 + threadIdx.x; j < j1; j += RK_T)
      atomicAdd(&run[(kin[j] >> shift) & 255u], 1u);
    __syncthreads();
    u64 ex, tot;
    block_scan<false>((u64)run[threadIdx.x], sm, ex, tot);
    run[threadIdx.x] = (unsigned)ex;
  }
  for (int64_t base = j0; base < j1; base += RK_SUB) {
#pragma unroll
    for (int w = 0; w < RK_WAVES; ++w) wcnt[w][threadIdx.x] = 0;
    __syncthreads();  // (also orders the writes of run above / below before its readers)
    unsigned key[4], lr[4];
    int dig[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      // wave wv owns keys [base + 256 wv, +256): four runs of 64, in order
      const int64_t j = base + wv * 256 + i * 64 + lane;
      const bool ok = j < j1;
      key[i] = ok ? kin[j] : 0u;
      const int d = (int)((key[i] >> shift) & 255u);
      dig[i] = ok ? d : -1;
      // the lanes of this run with the same digit
      u64 peers = __ballot(ok);
#pragma unroll
      for (int bit = 0; bit < 8; ++bit) {
        const bool on = (d >> bit) & 1;
        const u64 bb = __ballot(on);
        peers &= on ? bb : ~bb;
      }
      const unsigned before = (unsigned)__popcll(peers & ((1ull << lane) - 1ull));
      const unsigned old = ok ? wcnt[wv][d] : 0u;
      lr[i] = old + before;
      wave_lds_sync();
      if (ok && before == 0) wcnt[wv][d] = old + (unsigned)__popcll(peers);
      wave_lds_sync();
    }
    __syncthreads();
    {
      unsigned b = run[threadIdx.x];
#pragma unroll
      for (int w = 0; w < RK_WAVES; ++w) {
        const unsigned t = wcnt[w][threadIdx.x];
        wcnt[w][threadIdx.x] = b;
        b += t;
      }
      run[threadIdx.x] = b;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (dig[i] < 0) continue;
      const int64_t pos = (int64_t)wcnt[wv][dig[i]] + lr[i];
      if (pos < s.len) out[s.off + pos] = key[i];
    }
    __syncthreads();
  }
}

// -------------------------------------------------------------- 3. the curves ---
// Position j counts from the highest score: key_j = sorted[len - 1 - j].  Tile state, three
// 64-bit words per tile: k_rank_curve<false> leaves {positives of the tile, packed last
// group start of the tile}; k_rank_carry replaces them by the carries into the tile
// {positives before it, last group start before it, positives before that start};
// k_rank_curve<true> leaves the tile's PR partial in word 0.
// packed = (start index in the tile + 1) << 32 | positives of the tile before the start;
// 0 = the tile has no start.  Both halves grow with j, so "the last start" is a max.
template <bool FINAL>
__global__ __launch_bounds__(RK_T) void k_rank_curve(RankGeo g,
                                                     const unsigned* __restrict__ keys,
                                                     const u64* __restrict__ npos,
                                                     u64* __restrict__ tstate,
                                                     u64* __restrict__ rocnum,
                                                     double* __restrict__ out) {
  const RankSeg s = rank_seg_of_block(g);
  if ((!FINAL && s.tps <= 1) || rank_skip(npos, s)) return;
  __shared__ u64 sm[RK_WAVES];
  __shared__ double dred[RK_T];
  __shared__ u64 ured[RK_T];
  const unsigned* kseg = keys + s.off;
  const int64_t len = s.len;
  const int64_t j0 = s.t * g.tile;
  const int64_t j1 = j0 + g.tile < len ? j0 + g.tile : len;
  u64* ts = tstate + (s.tbase + s.t) * 3;
  u64 tp_base = 0, s_in = 0, tpx_in = 0;
  if (FINAL && s.tps > 1) {
    tp_base = ts[0];
    s_in = ts[1];
    tpx_in = ts[2];
  }
  const double P = (double)npos[s.seg];
  u64 csum = 0, clast = 0;  // of this tile so far: positives, packed last start
  u64 roc = 0;
  double pr = 0.0;
  for (int64_t base = j0; base < j1; base += RK_SUB) {
    const int64_t jb = base + 4 * (int64_t)threadIdx.x;
    unsigned kk[6];  // the scores at jb - 1 .. jb + 4
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const int64_t j = jb - 1 + i;
      kk[i] = (j >= 0 && j < len) ? kseg[len - 1 - j] : 0u;
    }
    bool ok[4], st[4], en[4];
    unsigned pos[4];
    unsigned tsum = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t j = jb + i;
      ok[i] = j < j1;
      st[i] = ok[i] && (j == 0 || (kk[i] >> 1) != (kk[i + 1] >> 1));
      en[i] = ok[i] && (j == len - 1 || (kk[i + 2] >> 1) != (kk[i + 1] >> 1));
      pos[i] = ok[i] ? (kk[i + 1] & 1u) : 0u;
      tsum += pos[i];
    }
    u64 ex, tot;
    block_scan<false>((u64)tsum, sm, ex, tot);
    u64 before[4], pk[4], pmax = 0;  // positives of the tile before element i
    {
      u64 r = csum + ex;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        before[i] = r;
        r += pos[i];
        pk[i] = st[i] ? (((u64)(jb + i - j0 + 1)) << 32) | before[i] : 0ull;
        pmax = pk[i] > pmax ? pk[i] : pmax;
      }
    }
    u64 lex, ltot;
    block_scan<true>(pmax, sm, lex, ltot);
    if (FINAL) {
      u64 cur = lex > clast ? lex : clast;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        cur = pk[i] > cur ? pk[i] : cur;
        if (!en[i]) continue;
        const u64 j = (u64)(jb + i);
        const u64 tp = tp_base + before[i] + pos[i];
        u64 gs, tpp;  // the group's first position, positives before it
        if (cur) {
          gs = (u64)j0 + (cur >> 32) - 1;
          tpp = tp_base + (cur & 0xffffffffull);
        } else {
          gs = s_in;
          tpp = tpx_in;
        }
        const u64 fp = j + 1 - tp, fpp = gs - tpp;
        roc += (fp - fpp) * (tp + tpp);
        const double pprev = gs == 0 ? 1.0 : (double)tpp / (double)gs;
        const double pg = (double)tp / (double)(j + 1);
        pr += ((double)tp / P - (double)tpp / P) * (pg + pprev) * 0.5;
      }
    }
    csum += tot;
    clast = ltot > clast ? ltot : clast;
  }
  if (!FINAL) {
    if (threadIdx.x == 0) {
      ts[0] = csum;
      ts[1] = clast;
    }
    return;
  }
  dred[threadIdx.x] = pr;
  ured[threadIdx.x] = roc;
  __syncthreads();
  for (int o = RK_T / 2; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
      dred[threadIdx.x] += dred[threadIdx.x + o];
      ured[threadIdx.x] += ured[threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  if (s.tps > 1) {
    ts[0] = (u64)__double_as_longlong(dred[0]);
    atomicAdd(&rocnum[s.seg], ured[0]);
  } else {
    const double N = (double)len - P;
    double* o = out + s.seg * 4;
    o[0] = dred[0];
    o[1] = (double)ured[0] / (2.0 * P * N);
    o[2] = P;
    o[3] = N;
  }
}

__global__ __launch_bounds__(RK_T) void k_rank_carry(RankGeo g, const u64* __restrict__ npos,
                                                     u64* __restrict__ tstate) {
  const RankSeg s = rank_seg_of(g, blockIdx.x);
  if (s.tps <= 1 || rank_skip(npos, s)) return;
  __shared__ u64 sm[RK_WAVES];
  u64 csum = 0, cs = 0, cx = 0;  // carries: positives, last start + 1, positives before it
  for (int64_t base = 0; base < s.tps; base += RK_T) {
    const int64_t t = base + threadIdx.x;
    const bool ok = t < s.tps;
    u64* ts = tstate + (s.tbase + (ok ? t : 0)) * 3;
    const u64 a = ok ? ts[0] : 0ull, l = ok ? ts[1] : 0ull;
    u64 ex, tot;
    block_scan<false>(a, sm, ex, tot);
    const u64 tpb = csum + ex;
    const u64 gs1 = l ? (u64)t * (u64)g.tile + (l >> 32) : 0ull;  // global start + 1
    const u64 gx = l ? tpb + (l & 0xffffffffull) : 0ull;
    u64 sex, stot, xex, xtot;
    block_scan<true>(gs1, sm, sex, stot);
    block_scan<true>(gx, sm, xex, xtot);
    const u64 s1 = sex > cs ? sex : cs;
    if (ok) {
      ts[0] = tpb;
      ts[1] = s1 ? s1 - 1 : 0ull;  // (tile 0 starts a group at position 0)
      ts[2] = xex > cx ? xex : cx;
    }
    csum += tot;
    cs = stot > cs ? stot : cs;
    cx = xtot > cx ? xtot : cx;
  }
}

// the rows of the segments that k_rank_curve did not finish: NaN for a segment without a
// curve, and the sum over the tiles, in index order, of a multi-tile segment
__global__ __launch_bounds__(RK_T) void k_rank_final(RankGeo g, const u64* __restrict__ npos,
                                                     const u64* __restrict__ tstate,
                                                     const u64* __restrict__ rocnum,
                                                     double* __restrict__ out) {
  const RankSeg s = rank_seg_of(g, blockIdx.x);
  const double P = (double)npos[s.seg], N = (double)s.len - P;
  double* o = out + s.seg * 4;
  if (rank_skip(npos, s)) {
    if (threadIdx.x == 0) {
      o[0] = NAN;
      o[1] = NAN;
      o[2] = P;
      o[3] = N;
    }
    return;
  }
  if (s.tps <= 1) return;
  __shared__ double red[RK_T];
  double t = 0.0;
  for (int64_t i = threadIdx.x; i < s.tps; i += RK_T)
    t += __longlong_as_double((long long)tstate[(s.tbase + i) * 3]);
  red[threadIdx.x] = t;
  __syncthreads();
  for (int st = RK_T / 2; st > 0; st >>= 1) {
    if (threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    o[0] = red[0];
    o[1] = (double)rocnum[s.seg] / (2.0 * P * N);
    o[2] = P;
    o[3] = N;
  }
}

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Workspace: two key buffers, the digit counts of the multi-tile segments, the positives
// per segment and, when a segment has more than one tile, the ROC numerators and tile
// state.  The tile grows with K and with the longest segment, which keeps the counts under
// the 8 bytes per voxel the key buffers of the pooled mode leave of 16 K bytes per voxel.
RankGeo rank_geo(int batch, int64_t V, int K, int per_sample) {
  RankGeo g;
  const int64_t n = (int64_t)batch * V;
  g.K = K;
  g.per_sample = per_sample;
  g.nu = per_sample ? batch * K : K;
  g.ulen = per_sample ? V : n;
  g.mlen = per_sample ? 0 : (int64_t)(K - 1) * n;
  const int64_t maxlen = g.mlen > g.ulen ? g.mlen : g.ulen;
  int64_t m = (maxlen + (int64_t)RK_UNIT * 1024 - 1) / ((int64_t)RK_UNIT * 1024);
  if (!per_sample && m < (2 * K - 1 + 23) / 24) m = (2 * K - 1 + 23) / 24;
  if (m < 1) m = 1;
  g.tile = m * RK_UNIT;
  g.utps = (g.ulen + g.tile - 1) / g.tile;
  g.mtps = (g.mlen + g.tile - 1) / g.tile;
  g.nblk = (int64_t)g.nu * g.utps + g.mtps;
  g.total = (int64_t)g.nu * g.ulen + g.mlen;
  g.multi = g.utps > 1 || g.mtps > 1;
  g.hist_entries = (g.utps > 1 ? (int64_t)g.nu * g.utps * 256 : 0) + (g.mtps > 1 ? g.mtps * 256 : 0);
  size_t o = 0;
  o = align_up(o + (size_t)g.total * 4, 16);
  g.off_b = o;
  o = align_up(o + (size_t)g.total * 4, 16);
  g.off_hist = o;
  o = align_up(o + (size_t)g.hist_entries * 4, 16);
  g.off_npos = o;
  o += (size_t)(g.nu + 1) * 8;
  g.off_roc = o;
  if (g.multi) o += (size_t)(g.nu + 1) * 8;
  g.off_tile = o;
  if (g.multi) o += (size_t)g.nblk * 24;
  g.bytes = o + 64;
  return g;
}

}  // namespace

hipError_t rank_auc(const float* scores, const int64_t* labels, int batch, int64_t V, int K,
                    int from_logits, int per_sample, double* out, void* ws, hipStream_t s) {
  const RankGeo g = rank_geo(batch, V, K, per_sample);
  char* w = static_cast<char*>(ws);
  unsigned* ka = reinterpret_cast<unsigned*>(w);
  unsigned* kb = reinterpret_cast<unsigned*>(w + g.off_b);
  unsigned* hist = reinterpret_cast<unsigned*>(w + g.off_hist);
  u64* npos = reinterpret_cast<u64*>(w + g.off_npos);
  u64* roc = reinterpret_cast<u64*>(w + g.off_roc);
  u64* tst = reinterpret_cast<u64*>(w + g.off_tile);
  hipError_t e;
  // npos and the ROC numerators are adjacent: one fill
  if ((e = zero_async(npos, (size_t)(g.nu + 1) * 8 * (g.multi ? 2 : 1), s)) != hipSuccess) return e;
  const int stage = K <= RK_STAGE_K;
  const int64_t ngroups = (V + 63) / 64;
  int64_t gx = (ngroups + RK_WAVES - 1) / RK_WAVES;
  const int64_t cap = 2048 / batch > 1 ? 2048 / batch : 1;
  if (gx > cap) gx = cap;
  hipLaunchKernelGGL(k_rank_keys, dim3((unsigned)(gx * batch)), dim3(RK_T),
                     stage ? (size_t)RK_WAVES * 64 * K * sizeof(float) : 0, s, scores, labels, V, K,
                     from_logits, per_sample, (int64_t)batch * V, (int)gx, stage, ka, npos);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  const unsigned nseg = (unsigned)(g.nu + 1);  // (the pooled micro row; an empty segment else)
  unsigned* src = ka;
  unsigned* dst = kb;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 8 * pass;
    if (g.multi) {
      hipLaunchKernelGGL(k_rank_hist, dim3((unsigned)g.nblk), dim3(RK_T), 0, s, g, src, shift,
                         npos, hist);
      hipLaunchKernelGGL(k_rank_scan, dim3(nseg), dim3(RK_T), 0, s, g, npos, hist);
    }
    hipLaunchKernelGGL(k_rank_scatter, dim3((unsigned)g.nblk), dim3(RK_T), 0, s, g, src, dst,
                       shift, npos, hist);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    unsigned* t = src;
    src = dst;
    dst = t;
  }
  // (four passes: the sorted keys are back in the first buffer)
  if (g.multi) {
    hipLaunchKernelGGL(k_rank_curve<false>, dim3((unsigned)g.nblk), dim3(RK_T), 0, s, g, src, npos,
                       tst, roc, out);
    hipLaunchKernelGGL(k_rank_carry, dim3(nseg), dim3(RK_T), 0, s, g, npos, tst);
  }
  hipLaunchKernelGGL(k_rank_curve<true>, dim3((unsigned)g.nblk), dim3(RK_T), 0, s, g, src, npos, tst,
                     roc, out);
  const unsigned nrows = per_sample ? (unsigned)g.nu : nseg;
  hipLaunchKernelGGL(k_rank_final, dim3(nrows), dim3(RK_T), 0, s, g, npos, tst, roc, out);
  return hipGetLastError();
}

}  // namespace spff

// =================================================================== C ABI ==
using namespace spff;

namespace {
const char* rank_args_check(int batch, int64_t vps, int K) {
  if (batch < 1) return "spff_rank_auc: batch must be >= 1";
  if (vps < 1) return "spff_rank_auc: vox_per_sample must be >= 1";
  if (K < 1 || K > SPFF_MAX_CLASSES) return "spff_rank_auc: num_classes must be 1..SPFF_MAX_CLASSES";
  // positions inside a segment are 32-bit, workgroup ids too
  const double longest = (double)batch * (double)vps * (K > 2 ? K - 1 : 1);
  if (longest >= 4294967296.0 || (double)batch * K >= 2147483647.0)
    return "spff_rank_auc: a segment of 2^32 keys or more";
  return nullptr;
}
}  // namespace

extern "C" {

size_t spff_rank_auc_ws_bytes(int batch, int64_t vox_per_sample, int num_classes, int per_sample) {
  if (rank_args_check(batch, vox_per_sample, num_classes)) return 0;
  return rank_geo(batch, vox_per_sample, num_classes, per_sample != 0).bytes;
}

int spff_rank_auc(const float* scores, const int64_t* labels, int batch, int64_t vox_per_sample,
                  int num_classes, int from_logits, int per_sample, double* out, void* ws,
                  void* stream) {
  if (const char* m = rank_args_check(batch, vox_per_sample, num_classes))
    return set_error(SPFF_EINVAL, m);
  if (!scores || !labels || !out || !ws) return set_error(SPFF_EINVAL, "spff_rank_auc: null argument");
  const hipError_t e = rank_auc(scores, labels, batch, vox_per_sample, num_classes, from_logits != 0,
                                per_sample != 0, out, ws, static_cast<hipStream_t>(stream));
  return e == hipSuccess ? SPFF_OK : set_error(SPFF_EHIP, hipGetErrorString(e));
}

}  // extern "C"
