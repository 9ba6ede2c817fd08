// MONAI's UnetResBlock as the MONAI-style plans (swin.hip, unetr.hip) run it: the packed
// Linear / 1x1 conv descriptor, the block descriptor and its forward / backward schedule on
// the engine's convs and affine-free InstanceNorm.  The plan-generic steps (statistics slot,
// InstanceNorm forward / backward, conv descriptor and weight preparation, transposed conv)
// come from plan_ops.h.  Everything here is internal to the including translation unit
// (namespace spff, anonymous).  A plan type P derives from PlanBase and provides, beside
// what plan_ops.h lists:
//   RB rb[]; int maxC
//   workspace offsets ones, zeros [maxC], dummy [2 maxC] (the affine-free norm's gamma, beta
//   and the sink of its dgamma / dbeta), cst, G_dz, G_dy2, G_da1, sized as build() of
//   swin.hip / unetr.hip sizes them
#pragma once
#include "plan_ops.h"
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
  Conv3 cv[2];
  Lin c3;
  size_t y1, a1, y2, y3, out;
  Stat4 st[3];  // of the IN after conv1, conv2, conv3
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
  r.cv[0] = reg_conv(p, name + ".conv1.conv.weight", Cin, C);
  r.cv[1] = reg_conv(p, name + ".conv2.conv.weight", C, C);
  if (r.has3) reg_lin(p, r.c3, name + ".conv3.conv", Cin, C, false, {C, Cin, 1, 1, 1});
}

// the block's activations and statistics slots
template <class P>
void rb_alloc(P* p, RB& r) {
  const size_t act = fbytes(nvox(p->vol[r.L]) * r.C);
  r.y1 = p->alloc(act);
  r.a1 = p->alloc(act);
  r.y2 = p->alloc(act);
  r.y3 = r.has3 ? p->alloc(act) : 0;
  r.out = p->alloc(act);
  for (Stat4& s : r.st) s = stat_alloc(p, fbytes((int64_t)p->cfg.batch * r.C));
}

// 3x3x3 conv c + (fused where the kernel allows) affine-free IN statistics
template <class P>
int conv_in(P* p, const Src2& in, const Conv3& c, const Vol& v, size_t y, const Stat4& s) {
  const int math = p->cfg.math;
  const float* img;
  const unsigned* wmax;
  PLAN_CK(conv_image(p, c, false, v, &img, &wmax));
  const bool fuse = conv3d_fuses_stats(v, 3, c.Cin, c.C, math);
  PLAN_HIPCK(conv3d_run(in, img, dst1(p->F(y), c.C), v, 3, c.Cin, c.C, false, math, p->st,
                    p->F(p->wg_ws), fuse ? p->F(p->cst) : nullptr, 0, wmax));
  if (fuse) {
    PLAN_HIPCK(conv3d_in_stats_fin(p->F(p->cst), v, 3, c.Cin, c.C, math, p->F(p->ones),
                               p->F(p->zeros), p->F(s.mean), p->F(s.rstd), p->F(s.al), p->F(s.de),
                               p->st));
    return SPFF_OK;
  }
  return in_fwd(p, v, c.C, p->F(y), s, p->F(p->ones), p->F(p->zeros));
}

template <class P>
int rb_fwd(P* p, RB& r, const Src2& in, const float* ident) {
  const Vol& v = p->vol[r.L];
  const int C = r.C;
  PLAN_CK(conv_in(p, in, r.cv[0], v, r.y1, r.st[0]));
  PLAN_HIPCK(act_apply(p->F(r.y1), p->F(r.a1), p->F(r.st[0].al), p->F(r.st[0].de), nullptr, nullptr, v,
                   C, p->st));
  PLAN_CK(conv_in(p, src1(p->F(r.a1), C), r.cv[1], v, r.y2, r.st[1]));
  if (r.has3) {
    float* pk = p->F(r.c3.pk);
    PLAN_HIPCK(head_pack(p->P(r.c3.w), pk, pk + head_pack_dgrad_offset(r.Cin, C), r.Cin, C, p->st));
    PLAN_HIPCK(linear_fwd2(in, r.Cin, pk, nullptr, p->F(r.y3), C, C, nvox(v), p->st));
    PLAN_CK(in_fwd(p, v, C, p->F(r.y3), r.st[2], p->F(p->ones), p->F(p->zeros)));
  }
  PLAN_HIPCK(res_act(p->F(r.y2), p->F(r.st[1].al), p->F(r.st[1].de), r.has3 ? p->F(r.y3) : nullptr,
                 p->F(r.st[2].al), p->F(r.st[2].de), ident, nullptr, p->F(r.out), v, C, p->st));
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
  // affine-free IN (+ activation slope neg) backward: gamma = 1, dgamma / dbeta discarded
  auto in_bwd1 = [&](size_t y, const float* g, float* dy, const Stat4& s, float neg) {
    float* dm = p->F(p->dummy);
    return in_bwd(p, v, C, p->F(y), g, dy, s, p->F(p->ones), dm, dm + p->maxC, neg);
  };
  PLAN_HIPCK(res_act(p->F(r.y2), p->F(r.st[1].al), p->F(r.st[1].de), r.has3 ? p->F(r.y3) : nullptr,
                 p->F(r.st[2].al), p->F(r.st[2].de), ident, dout, dz, v, C, p->st));
  PLAN_CK(in_bwd1(r.y2, dz, dy2, r.st[1], 1.f));
  PLAN_HIPCK(conv3d_wgrad(src1(p->F(r.a1), C), dy2, C, p->DP(r.cv[1].w), v, 3, C, C, math,
                      p->F(p->wg_ws), p->st));
  PLAN_CK(conv_run(p, r.cv[1], true, src1(dy2, C), dst1(da1, C), v));
  PLAN_CK(in_bwd1(r.y1, da1, da1, r.st[0], 0.01f));
  PLAN_HIPCK(conv3d_wgrad(in, da1, C, p->DP(r.cv[0].w), v, 3, r.Cin, C, math, p->F(p->wg_ws), p->st));
  if (dsrc) PLAN_CK(conv_run(p, r.cv[0], true, src1(da1, C), *dsrc, v));
  if (r.has3) {
    PLAN_CK(in_bwd1(r.y3, dz, dy2, r.st[2], 1.f));
    PLAN_HIPCK(linear_wgrad2(in, r.Cin, dy2, C, C, p->DP(r.c3.w), p->F(p->dummy), V, p->F(p->wg_ws),
                         p->st));
    if (dsrc) {
      const float* wd = p->F(r.c3.pk) + head_pack_dgrad_offset(r.Cin, C);
      PLAN_HIPCK(linear_dgrad2(dy2, C, C, wd, *dsrc, r.Cin, V, 1, p->st));
    }
  } else if (dsrc) {
    PLAN_HIPCK(accumulate(dsrc->p0, dz, V * C, 1.f, p->st));
  }
  return SPFF_OK;
}

}  // namespace
}  // namespace spff
