// The pieces that the MONAI-style plans (swin.hip, unetr.hip) share: packed Linear / 1x1
// conv, UnetResBlock and 2x2x2 transposed-conv descriptors, and the UnetResBlock forward /
// backward schedule on the engine's convs and InstanceNorm kernels.  Everything here is
// internal to the including translation unit (namespace spff, anonymous).  A plan type P
// derives from PlanBase (plan_base.h: F / P / DP, reg, alloc, ws, st, PLAN_HIPCK / PLAN_CK)
// and provides, under these names:
//   cfg.math; Vol vol[]; RB rb[P::kNRB]; int maxC
//   workspace offsets ones, zeros [maxC], dummy [2 maxC], red_ws, red_out, kk1, kk2 [B maxC],
//   wg_ws, cst, G_dz, G_dy2, G_da1, and pkb ? rb[i].pk[] + wsl [kNRB][2] : wt, sized as
//   build() of swin.hip / unetr.hip sizes them
#pragma once
#include "plan_base.h"
#include "swin_internal.h"

#include <algorithm>
#include <string>
#include <vector>

namespace spff {
namespace {

struct Lin {  // nn.Linear / 1x1 conv W [N][K] (+ b)
  int64_t w = -1, b = -1;
  int K = 0, N = 0;
  size_t pk = 0;  // packed wf | wd
};

struct RB {
  std::string name;
  int L, Cin, C;
  bool has3;
  int64_t w1 = -1, w2 = -1;
  Lin c3;
  size_t y1, a1, y2, y3, out;
  size_t st[3][4];  // (mean, rstd, al, de) of the IN after conv1, conv2, conv3
  size_t pk[4] = {0, 0, 0, 0};  // batched conv images: w1 fwd, w2 fwd, w2 dgrad, w1 dgrad
};

struct Up {
  int Cin, Cout, Llow;
  int64_t w = -1;
  size_t pk, out;
};

template <class P>
void reg_lin(P* p, Lin& l, const std::string& name, int K, int N, bool bias,
             std::vector<int64_t> wshape = {}) {
  l.K = K;
  l.N = N;
  if (wshape.empty()) wshape = {N, K};
  l.w = p->reg(name + ".weight", wshape);
  if (bias) l.b = p->reg(name + ".bias", {N});
  l.pk = p->alloc(head_pack_floats(K, N) * sizeof(float));
}

template <class P>
void reg_rb(P* p, RB& r, const std::string& name, int L, int Cin, int C) {
  r.name = name;
  r.L = L;
  r.Cin = Cin;
  r.C = C;
  r.has3 = Cin != C;
  r.w1 = p->reg(name + ".conv1.conv.weight", {C, Cin, 3, 3, 3});
  r.w2 = p->reg(name + ".conv2.conv.weight", {C, C, 3, 3, 3});
  if (r.has3) reg_lin(p, r.c3, name + ".conv3.conv", Cin, C, false, {C, Cin, 1, 1, 1});
}

// affine-free InstanceNorm3d statistics of y [V][C] -> (mean, rstd, al, de)
template <class P>
int in_stats(P* p, const Vol& v, int C, size_t y, const size_t* st4) {
  RedArgs a{};
  a.y = p->F(y);
  PLAN_HIPCK(slab_reduce(RED_SUM, a, v, C, p->F(p->red_out), p->F(p->red_ws), p->st));
  PLAN_HIPCK(in_mean(p->F(p->red_out), p->F(st4[0]), v, C, p->st));
  a.mean = p->F(st4[0]);
  PLAN_HIPCK(slab_reduce(RED_SQDEV, a, v, C, p->F(p->red_out), p->F(p->red_ws), p->st));
  PLAN_HIPCK(in_rstd(p->F(p->red_out), p->F(p->ones), p->F(p->zeros), p->F(st4[0]), p->F(st4[1]),
                 p->F(st4[2]), p->F(st4[3]), v, C, p->st));
  return SPFF_OK;
}

// batched plans: every conv's max |w| (f16x3) in one launch, then every conv image
// (forward and input gradient; 39 for SwinUNETR, 31 for UNETR) in one more, at the forward start -- the weights do not
// change between a step's forward and backward (the up-conv / linear images are packed up
// front the same way).  Otherwise conv3d_pack before each conv (max + pack launches).
template <class P>
int prep_weights(P* p) {
  if (!p->pkb) return SPFF_OK;
  const int math = p->cfg.math;
  const bool f16 = math == SPFF_MATH_F16X3;
  unsigned* sl = reinterpret_cast<unsigned*>(p->ws + p->wsl);
  PrepJobs pj;
  PackJobs kj;
  if (f16) PLAN_HIPCK(spff::zero_async(sl, P::kNRB * 2 * sizeof(unsigned), p->st));
  for (int i = 0; i < P::kNRB; ++i) {
    RB& r = p->rb[i];
    unsigned* w1 = f16 ? sl + 2 * i : nullptr;
    unsigned* w2 = f16 ? sl + 2 * i + 1 : nullptr;
    bool ok = true;
    if (f16) {
      ok = ok && prep_absmax(&pj, p->P(r.w1), (int64_t)r.C * r.Cin * 27, w1);
      ok = ok && prep_absmax(&pj, p->P(r.w2), (int64_t)r.C * r.C * 27, w2);
    }
    ok = ok && conv3d_pack_job(&kj, p->P(r.w1), p->F(r.pk[0]), 3, r.Cin, r.C, false, w1);
    ok = ok && conv3d_pack_job(&kj, p->P(r.w2), p->F(r.pk[1]), 3, r.C, r.C, false, w2);
    ok = ok && conv3d_pack_job(&kj, p->P(r.w2), p->F(r.pk[2]), 3, r.C, r.C, true, w2);
    if (r.pk[3]) ok = ok && conv3d_pack_job(&kj, p->P(r.w1), p->F(r.pk[3]), 3, r.Cin, r.C, true, w1);
    if (!ok) return plan_fail(SPFF_EINVAL, "weight preparation table overflow");
  }
  PLAN_HIPCK(prep_run(pj, p->st));
  PLAN_HIPCK(conv3d_pack_many(kj, math, p->st));
  return SPFF_OK;
}
// conv k of residual block r (0: w1 fwd, 1: w2 fwd, 2: w2 dgrad, 3: w1 dgrad): its image
// (the batched one, else packed now into the scratch image) and its max |w| slot
template <class P>
int conv_image(P* p, const RB& r, int k, const Vol& v, const float** img,
               const unsigned** wmax) {
  const bool c1 = k == 0 || k == 3;
  const int ri = (int)(&r - p->rb);
  if (p->pkb) {
    if (!r.pk[k]) return plan_fail(SPFF_EINVAL, "no batched image for this conv");
    *img = p->F(r.pk[k]);
    *wmax = p->cfg.math == SPFF_MATH_F16X3
                ? reinterpret_cast<const unsigned*>(p->ws + p->wsl) + 2 * ri + (c1 ? 0 : 1)
                : nullptr;
    return SPFF_OK;
  }
  PLAN_HIPCK(conv3d_pack(p->P(c1 ? r.w1 : r.w2), p->F(p->wt), v, 3, c1 ? r.Cin : r.C, r.C, k >= 2,
                     p->cfg.math, p->st));
  *img = p->F(p->wt);
  *wmax = nullptr;
  return SPFF_OK;
}

// 3x3x3 conv k (0 / 1) of r + (fused where the kernel allows) IN statistics
template <class P>
int conv_in(P* p, const Src2& in, const RB& r, int k, const Vol& v, int Cin, int C,
            size_t y, const size_t* st4) {
  const int math = p->cfg.math;
  const float* img;
  const unsigned* wmax;
  PLAN_CK(conv_image(p, r, k, v, &img, &wmax));
  const bool fuse = conv3d_fuses_stats(v, 3, Cin, C, math);
  PLAN_HIPCK(conv3d_run(in, img, dst1(p->F(y), C), v, 3, Cin, C, false, math, p->st,
                    p->F(p->wg_ws), fuse ? p->F(p->cst) : nullptr, 0, wmax));
  if (fuse) {
    PLAN_HIPCK(conv3d_in_stats_fin(p->F(p->cst), v, 3, Cin, C, math, p->F(p->ones), p->F(p->zeros),
                               p->F(st4[0]), p->F(st4[1]), p->F(st4[2]), p->F(st4[3]), p->st));
    return SPFF_OK;
  }
  return in_stats(p, v, C, y, st4);
}

template <class P>
int rb_fwd(P* p, RB& r, const Src2& in, const float* ident) {
  const Vol& v = p->vol[r.L];
  const int C = r.C;
  PLAN_CK(conv_in(p, in, r, 0, v, r.Cin, C, r.y1, r.st[0]));
  PLAN_HIPCK(act_apply(p->F(r.y1), p->F(r.a1), p->F(r.st[0][2]), p->F(r.st[0][3]), nullptr, nullptr, v,
                   C, p->st));
  PLAN_CK(conv_in(p, src1(p->F(r.a1), C), r, 1, v, C, C, r.y2, r.st[1]));
  if (r.has3) {
    float* pk = p->F(r.c3.pk);
    PLAN_HIPCK(head_pack(p->P(r.c3.w), pk, pk + head_pack_dgrad_offset(r.Cin, C), r.Cin, C, p->st));
    PLAN_HIPCK(linear_fwd2(in, r.Cin, pk, nullptr, p->F(r.y3), C, C, nvox(v), p->st));
    PLAN_CK(in_stats(p, v, C, r.y3, r.st[2]));
  }
  PLAN_HIPCK(res_act(p->F(r.y2), p->F(r.st[1][2]), p->F(r.st[1][3]), r.has3 ? p->F(r.y3) : nullptr,
                 p->F(r.st[2][2]), p->F(r.st[2][3]), ident, nullptr, p->F(r.out), v, C, p->st));
  return SPFF_OK;
}

// IN (+ activation slope neg) backward: dy = IN'(g * slope(r)) for r = y*al + de
template <class P>
int in_bwd(P* p, const Vol& v, int C, size_t y, const float* g, float* dy,
           const size_t* st4, float neg) {
  RedArgs a{};
  a.y = p->F(y); a.g = g; a.mean = p->F(st4[0]); a.rstd = p->F(st4[1]);
  a.al = p->F(st4[2]); a.de = p->F(st4[3]); a.neg = neg;
  PLAN_HIPCK(slab_reduce(RED_BWD_IN, a, v, C, p->F(p->red_out), p->F(p->red_ws), p->st));
  float* dm = p->F(p->dummy);
  PLAN_HIPCK(in_bwd_stats(p->F(p->red_out), p->F(p->ones), dm, dm + p->maxC, p->F(p->kk1),
                      p->F(p->kk2), v, C, p->st));
  PLAN_HIPCK(in_bwd_apply(p->F(y), g, dy, p->F(st4[0]), p->F(st4[1]), p->F(st4[2]), p->F(st4[3]),
                      p->F(p->ones), nullptr, nullptr, p->F(p->kk1), p->F(p->kk2), v, C, p->st,
                      neg));
  return SPFF_OK;
}

// dsrc (may be null): written (conv1 dgrad), then the shortcut's gradient added
template <class P>
int rb_bwd(P* p, RB& r, const float* dout, const Src2& in, const float* ident,
           const Dst2* dsrc) {
  const Vol& v = p->vol[r.L];
  const int C = r.C, math = p->cfg.math;
  const int64_t V = nvox(v);
  float* dz = p->F(p->G_dz);
  float* dy2 = p->F(p->G_dy2);
  float* da1 = p->F(p->G_da1);
  PLAN_HIPCK(res_act(p->F(r.y2), p->F(r.st[1][2]), p->F(r.st[1][3]), r.has3 ? p->F(r.y3) : nullptr,
                 p->F(r.st[2][2]), p->F(r.st[2][3]), ident, dout, dz, v, C, p->st));
  PLAN_CK(in_bwd(p, v, C, r.y2, dz, dy2, r.st[1], 1.f));
  PLAN_HIPCK(conv3d_wgrad(src1(p->F(r.a1), C), dy2, C, p->DP(r.w2), v, 3, C, C, math, p->F(p->wg_ws),
                      p->st));
  const float* img;
  const unsigned* wmax;
  PLAN_CK(conv_image(p, r, 2, v, &img, &wmax));
  PLAN_HIPCK(conv3d_run(src1(dy2, C), img, dst1(da1, C), v, 3, C, C, true, math, p->st,
                    p->F(p->wg_ws), nullptr, 0, wmax));
  PLAN_CK(in_bwd(p, v, C, r.y1, da1, da1, r.st[0], 0.01f));
  PLAN_HIPCK(conv3d_wgrad(in, da1, C, p->DP(r.w1), v, 3, r.Cin, C, math, p->F(p->wg_ws), p->st));
  if (dsrc) {
    PLAN_CK(conv_image(p, r, 3, v, &img, &wmax));
    PLAN_HIPCK(conv3d_run(src1(da1, C), img, *dsrc, v, 3, r.Cin, C, true, math, p->st,
                      p->F(p->wg_ws), nullptr, 0, wmax));
  }
  if (r.has3) {
    PLAN_CK(in_bwd(p, v, C, r.y3, dz, dy2, r.st[2], 1.f));
    PLAN_HIPCK(linear_wgrad2(in, r.Cin, dy2, C, C, p->DP(r.c3.w), p->F(p->dummy), V, p->F(p->wg_ws),
                         p->st));
    if (dsrc) {
      const float* wd = p->F(r.c3.pk) + head_pack_dgrad_offset(r.Cin, C);
      PLAN_HIPCK(linear_dgrad2(dy2, C, C, wd, *dsrc, r.Cin, V, 1, p->st));
    }
  } else if (dsrc) {
    PLAN_HIPCK(add_inplace(dsrc->p0, dz, V * C, p->st));
  }
  return SPFF_OK;
}

}  // namespace
}  // namespace spff
