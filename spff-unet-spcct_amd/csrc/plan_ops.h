// The steps every convolutional variant plan performs (unet3d.hip, r2unet.hip, resunetpp.hip
// and, through res_block.h, swin.hip and unetr.hip), written once: the InstanceNorm
// statistics slot with its forward / backward sequences, the 3x3x3 conv descriptor with its
// weight preparation, the 2x2x2 transposed conv, the 1x1x1 head and the five-level U-Net
// loops.  Function templates on the plan type P, internal to the including translation
// unit (namespace spff, anonymous); no kernels.  P derives from PlanBase (plan_base.h) and
// provides, under these names, what the functions it calls read:
//   every function     cfg.math, Vol vol[], wg_ws
//   in_fwd / in_bwd    red_ws, red_out; kk1, kk2 [B maxC] (backward)
//   Conv3 functions    pkb ? wsl [one max |w| slot per conv] : wt (alloc_convs sizes them)
//   head_* / unet5_*   f, K, head_pk
//   unet5_*            blk[9] (each with lvl, C, out), UpConv up[4], pool[4], pidx[4],
//                      dskip[4], G_out, G_dx, x_cl, ldx
#pragma once
#include "plan_base.h"

#include <string>

namespace spff {
namespace {

// ---------------------------------------------------------- InstanceNorm --
struct Stat4 {  // per (b, c): the statistics and the apply coefficients y al + de
  size_t mean, rstd, al, de;
};
template <class P>
Stat4 stat_alloc(P* p, size_t bytes) {
  return Stat4{p->alloc(bytes), p->alloc(bytes), p->alloc(bytes), p->alloc(bytes)};
}

// InstanceNorm3d statistics of y [V][C] per (b, c) and the apply coefficients
// al = gamma rstd, de = beta - mean al
template <class P>
int in_fwd(P* p, const Vol& v, int C, const float* y, const Stat4& s, const float* gamma,
           const float* beta) {
  RedArgs a{};
  a.y = y;
  PLAN_HIPCK(slab_reduce(RED_SUM, a, v, C, p->F(p->red_out), p->F(p->red_ws), p->st));
  PLAN_HIPCK(in_mean(p->F(p->red_out), p->F(s.mean), v, C, p->st));
  a.mean = p->F(s.mean);
  PLAN_HIPCK(slab_reduce(RED_SQDEV, a, v, C, p->F(p->red_out), p->F(p->red_ws), p->st));
  PLAN_HIPCK(in_rstd(p->F(p->red_out), gamma, beta, p->F(s.mean), p->F(s.rstd), p->F(s.al),
                     p->F(s.de), v, C, p->st));
  return SPFF_OK;
}

// InstanceNorm backward: dy = rstd gamma (dr - k1 - xhat k2) with dr = g slope(y al + de).
// neg is the slope below zero of the activation that follows the norm: 0 for ReLU, 0.01
// for LeakyReLU, 1 when g is already the gradient at the norm's output.  dy may alias g.
template <class P>
int in_bwd(P* p, const Vol& v, int C, const float* y, const float* g, float* dy, const Stat4& s,
           const float* gamma, float* dgamma, float* dbeta, float neg) {
  RedArgs a{};
  a.y = y; a.g = g; a.mean = p->F(s.mean); a.rstd = p->F(s.rstd);
  a.al = p->F(s.al); a.de = p->F(s.de); a.neg = neg;
  PLAN_HIPCK(slab_reduce(RED_BWD_IN, a, v, C, p->F(p->red_out), p->F(p->red_ws), p->st));
  PLAN_HIPCK(in_bwd_stats(p->F(p->red_out), gamma, dgamma, dbeta, p->F(p->kk1), p->F(p->kk2), v, C,
                          p->st));
  PLAN_HIPCK(in_bwd_apply(y, g, dy, p->F(s.mean), p->F(s.rstd), p->F(s.al), p->F(s.de), gamma,
                          nullptr, nullptr, p->F(p->kk1), p->F(p->kk2), v, C, p->st, neg));
  return SPFF_OK;
}

// ------------------------------------------------------------ 3x3x3 conv --
// A bias-free Conv3d(3, padding 1).  A block type holds its convs as `Conv3 cv[n]`, in
// forward order; alloc_convs / prep_convs walk an array of such blocks.
struct Conv3 {
  int64_t w = -1;
  int Cin = 0, C = 0;
  bool dx = true;              // false: its input needs no gradient (the network's input)
  size_t pk_f = 0, pk_d = 0;   // batched images: forward, input gradient (dx only)
  int slot = 0;                // its max |w| slot in wsl
};
template <class P>
Conv3 reg_conv(P* p, const std::string& name, int Cin, int C) {
  Conv3 c;
  c.w = p->reg(name, {C, Cin, 3, 3, 3});
  c.Cin = Cin;
  c.C = C;
  return c;
}

// Where the conv images live.  Arithmetics that pack split images (pkb): per block the
// forward images in conv order, then the input-gradient images in reverse order, and one
// max |w| slot per conv; otherwise one scratch image of wt_bytes, packed before each conv.
template <class P, class B>
void alloc_convs(P* p, B* first, int count, size_t wt_bytes) {
  p->pkb = conv3d_packs_batched(p->cfg.math);
  if (!p->pkb) {
    p->wt = p->alloc(wt_bytes);
    return;
  }
  constexpr int N = (int)(sizeof(first->cv) / sizeof(Conv3));
  int slot = 0;
  for (B* b = first; b != first + count; ++b) {
    for (int k = 0; k < N; ++k) {
      Conv3& c = b->cv[k];
      c.pk_f = p->alloc(conv3d_pack_bytes(3, c.Cin, c.C));
      c.slot = slot++;
    }
    for (int k = N - 1; k >= 0; --k) {
      Conv3& c = b->cv[k];
      if (c.dx) c.pk_d = p->alloc(conv3d_pack_bytes(3, c.Cin, c.C));
    }
  }
  p->wsl = p->alloc(slot * sizeof(unsigned));
}

// batched plans: every conv's max |w| (f16x3) in one launch, then every conv image (forward
// and input gradient) in one more, at the forward start -- the weights do not change
// between a step's forward and backward.  The jobs follow the order of alloc_convs.
// Otherwise nothing: conv_image packs before each conv (max + pack launches).
template <class P, class B>
int prep_convs(P* p, B* first, int count) {
  if (!p->pkb) return SPFF_OK;
  const int math = p->cfg.math;
  const bool f16 = math == SPFF_MATH_F16X3;
  constexpr int N = (int)(sizeof(first->cv) / sizeof(Conv3));
  unsigned* sl = reinterpret_cast<unsigned*>(p->ws + p->wsl);
  auto wm = [&](const Conv3& c) { return f16 ? sl + c.slot : nullptr; };
  PrepJobs pj;
  PackJobs kj;
  if (f16) PLAN_HIPCK(spff::zero_async(sl, (size_t)count * N * sizeof(unsigned), p->st));
  for (B* b = first; b != first + count; ++b) {
    bool ok = true;
    for (int k = 0; k < N && f16; ++k) {
      const Conv3& c = b->cv[k];
      ok = ok && prep_absmax(&pj, p->P(c.w), (int64_t)c.C * c.Cin * 27, wm(c));
    }
    for (int k = 0; k < N; ++k) {
      const Conv3& c = b->cv[k];
      ok = ok && conv3d_pack_job(&kj, p->P(c.w), p->F(c.pk_f), 3, c.Cin, c.C, false, wm(c));
    }
    for (int k = N - 1; k >= 0; --k) {
      const Conv3& c = b->cv[k];
      if (c.pk_d)
        ok = ok && conv3d_pack_job(&kj, p->P(c.w), p->F(c.pk_d), 3, c.Cin, c.C, true, wm(c));
    }
    if (!ok) return plan_fail(SPFF_EINVAL, "weight preparation table overflow");
  }
  PLAN_HIPCK(prep_run(pj, p->st));
  PLAN_HIPCK(conv3d_pack_many(kj, math, p->st));
  return SPFF_OK;
}

// a conv's image (forward or input gradient) and its max |w| slot: the batched image, else
// packed now into the scratch image
template <class P>
int conv_image(P* p, const Conv3& c, bool dgrad, const Vol& v, const float** img,
               const unsigned** wmax) {
  if (p->pkb) {
    const size_t pk = dgrad ? c.pk_d : c.pk_f;
    if (!pk) return plan_fail(SPFF_EINVAL, "no batched image for this conv");
    *img = p->F(pk);
    *wmax = p->cfg.math == SPFF_MATH_F16X3
                ? reinterpret_cast<const unsigned*>(p->ws + p->wsl) + c.slot
                : nullptr;
    return SPFF_OK;
  }
  PLAN_HIPCK(conv3d_pack(p->P(c.w), p->F(p->wt), v, 3, c.Cin, c.C, dgrad, p->cfg.math, p->st));
  *img = p->F(p->wt);
  *wmax = nullptr;
  return SPFF_OK;
}

// y = conv(x) (dgrad: x = dy with C channels, y = dx with Cin) in the plan's arithmetic
template <class P>
int conv_run(P* p, const Conv3& c, bool dgrad, const Src2& x, const Dst2& y, const Vol& v) {
  const float* img;
  const unsigned* wmax;
  PLAN_CK(conv_image(p, c, dgrad, v, &img, &wmax));
  PLAN_HIPCK(conv3d_run(x, img, y, v, 3, c.Cin, c.C, dgrad, p->cfg.math, p->st, p->F(p->wg_ws),
                        nullptr, 0, wmax));
  return SPFF_OK;
}

// -------------------------------------------------- 2x2x2 transposed conv --
// ConvTranspose3d(k = s = 2) from level Llow to Llow - 1, as a GEMM over 8 sub-lattices
struct UpConv {
  int Cin, Cout, Llow;
  int64_t w = -1, b = -1;
  size_t pk, out;
};
constexpr int UP_NS = 8;

template <class P>
void up_alloc(P* p, UpConv& U) {
  U.out = p->alloc(fbytes(nvox(p->vol[U.Llow - 1]) * U.Cout));
  U.pk = p->alloc(fbytes(upconv_pack_floats(U.Cin, U.Cout, UP_NS)));
}
// U.out = up(x) + bias; packs the forward and input-gradient images
template <class P>
int up_fwd(P* p, UpConv& U, const float* x, const float* bias, int math = SPFF_MATH_F32) {
  float* pk = p->F(U.pk);
  PLAN_HIPCK(upconv_pack(p->P(U.w), pk, pk + upconv_pack_dgrad_offset(U.Cin, U.Cout, UP_NS), U.Cin,
                         U.Cout, p->st, UP_NS));
  PLAN_HIPCK(upconv_fwd(x, pk, bias, p->F(U.out), p->vol[U.Llow], U.Cin, U.Cout, p->st, UP_NS,
                        math));
  return SPFF_OK;
}
// dout [high][Cout] -> the weight and bias gradients and (dx non-null) dx [low][Cin], written
template <class P>
int up_bwd(P* p, UpConv& U, const float* x, const float* dout, float* dbias, float* dx,
           int math = SPFF_MATH_F32) {
  PLAN_HIPCK(upconv_wgrad(x, dout, U.Cout, p->DP(U.w), dbias, p->vol[U.Llow], U.Cin, U.Cout,
                          p->F(p->wg_ws), p->st, UP_NS, math));
  if (dx) {
    const float* wd = p->F(U.pk) + upconv_pack_dgrad_offset(U.Cin, U.Cout, UP_NS);
    PLAN_HIPCK(upconv_dgrad(dout, U.Cout, wd, dx, p->vol[U.Llow], U.Cin, U.Cout, p->st, UP_NS, math));
  }
  return SPFF_OK;
}

// ----------------------------------------------------------- 1x1x1 head --
// y [V0][K] = x [V0][f] . W^T + b; packs the forward and input-gradient images into head_pk
template <class P>
int head_fwd_packed(P* p, int64_t w, int64_t b, const float* x, float* y) {
  float* hp = p->F(p->head_pk);
  PLAN_HIPCK(head_pack(p->P(w), hp, hp + head_pack_dgrad_offset(p->f, p->K), p->f, p->K, p->st));
  PLAN_HIPCK(head_fwd(x, hp, p->P(b), y, nvox(p->vol[0]), p->f, p->K, p->st, p->cfg.math));
  return SPFF_OK;
}
template <class P>
int head_bwd(P* p, int64_t w, int64_t b, const float* x, const float* dy, float* dx) {
  const int64_t V0 = nvox(p->vol[0]);
  PLAN_HIPCK(head_wgrad(x, dy, p->DP(w), p->DP(b), V0, p->f, p->K, p->F(p->wg_ws), p->st));
  PLAN_HIPCK(head_dgrad(dy, p->F(p->head_pk) + head_pack_dgrad_offset(p->f, p->K), dx, V0, p->f,
                        p->K, p->st, p->cfg.math));
  return SPFF_OK;
}

// ------------------------------------------------- five-level U-Net loops --
// blk: e1..e4, bottleneck, d4..d1; up: up4..up1; channels f << level.
//   e(l+1) = blk(pool(e l)); d l = blk([up(d(l+1)) | e l]); y = head(d1)
// fwd(block, in, kin) runs a block on `in` (kin channels in all); bwd(block, dout, dx, in)
// turns dout into the block's parameter gradients and (dx non-null) its input gradient.
template <class P, class Fwd>
int unet5_forward(P* p, int64_t head_w, int64_t head_b, float* y, Fwd fwd) {
  const int f = p->f;
  auto* B = p->blk;
  Src2 in = src1(p->F(p->x_cl), p->ldx);
  int kin = p->ldx;
  for (int l = 0; l < 4; ++l) {
    PLAN_CK(fwd(B[l], in, kin));
    PLAN_HIPCK(maxpool3_fwd(p->F(B[l].out), p->F(p->pool[l]),
                            reinterpret_cast<uint8_t*>(p->ws + p->pidx[l]), p->vol[l], f << l, p->st));
    in = src1(p->F(p->pool[l]), f << l);
    kin = f << l;
  }
  PLAN_CK(fwd(B[4], in, kin));
  const float* prev = p->F(B[4].out);
  for (int u = 0; u < 4; ++u) {
    UpConv& U = p->up[u];
    PLAN_CK(up_fwd(p, U, prev, p->P(U.b), p->cfg.math));
    // torch.cat([up(x), skip], dim=1) read in place through the two-source view
    PLAN_CK(fwd(B[5 + u], Src2{p->F(U.out), p->F(B[3 - u].out), U.Cout, U.Cout, U.Cout},
                2 * U.Cout));
    prev = p->F(B[5 + u].out);
  }
  return head_fwd_packed(p, head_w, head_b, prev, y);
}

template <class P, class Bwd>
int unet5_backward(P* p, int64_t head_w, int64_t head_b, const float* dy, Bwd bwd) {
  const int f = p->f;
  auto* B = p->blk;
  PLAN_CK(head_bwd(p, head_w, head_b, p->F(B[8].out), dy, p->F(p->G_out)));
  for (int k = 0; k < 4; ++k) {  // d1 <- up1 <- d2 ... <- up4
    auto& d = B[8 - k];
    UpConv& U = p->up[3 - k];
    const int C = d.C, lvl = d.lvl;
    Dst2 dx{p->F(p->G_dx), p->F(p->dskip[lvl]), C, C, C};
    PLAN_CK(bwd(d, p->F(p->G_out), &dx, Src2{p->F(U.out), p->F(B[lvl].out), C, C, C}));
    PLAN_CK(up_bwd(p, U, p->F(B[7 - k].out), p->F(p->G_dx), p->DP(U.b), p->F(p->G_out),
                   p->cfg.math));
  }
  {
    Dst2 dx = dst1(p->F(p->G_dx), 8 * f);
    PLAN_CK(bwd(B[4], p->F(p->G_out), &dx, src1(p->F(p->pool[3]), 8 * f)));
  }
  for (int l = 3; l >= 0; --l) {
    const int C = f << l;
    PLAN_HIPCK(maxpool3_bwd_add(p->F(p->G_dx), reinterpret_cast<const uint8_t*>(p->ws + p->pidx[l]),
                                p->F(p->dskip[l]), C, p->F(p->dskip[l]), p->vol[l], C, p->st));
    if (l > 0) {
      Dst2 dx = dst1(p->F(p->G_dx), C / 2);
      PLAN_CK(bwd(B[l], p->F(p->dskip[l]), &dx, src1(p->F(p->pool[l - 1]), C / 2)));
    } else {
      PLAN_CK(bwd(B[0], p->F(p->dskip[0]), nullptr, src1(p->F(p->x_cl), p->ldx)));
    }
  }
  return SPFF_OK;
}

}  // namespace
}  // namespace spff
