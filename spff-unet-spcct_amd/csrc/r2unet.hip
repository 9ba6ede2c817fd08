// R2UNet3D variant: the recurrent residual 3D U-Net behind the registry entry
// "R2UNet3D" (LitR2UNet3D_Published around R2UNet3D_backbone).
//
// Graph, levels l = 0..4 halve D, H, W (MaxPool3d(2)), channels C_l = base << l:
//   e1 = blk(x); e2 = blk(pool(e1)); e3 = blk(pool(e2)); e4 = blk(pool(e3)); b = blk(pool(e4))
//   d4 = blk([up4(b) | e4]); d3 = blk([up3(d4) | e3]); d2 = blk([up2(d3) | e2])
//   d1 = blk([up1(d2) | e1]); logits = head(d1)          (head: 1x1x1 conv + bias)
// Block(cin -> C, t):
//   x1 = inp(x)                                  1x1x1, no bias
//   r_0 = x1, h_0 = 0;  r_k = relu(IN_ru(conv(r_{k-1} + h_{k-1}))), h_k = r_k,  k = 1..t
//   s  = x1 + out(r_t)                           1x1x1, no bias, residual operand of the GEMM
//   o  = relu(IN_bn(s))
// conv (3x3x3, no bias) and IN_ru (affine) are shared by the t steps.
//
// The doubling fold.  Step 1 convolves x1; every later step convolves r + h = 2 r_{k-1}.
// relu(2 z) = 2 relu(z) exactly in fp32, so a step k < t is normalised with the doubled
// affine (2 gamma, 2 beta) -- its coefficients come out as (2 al, 2 de), bitwise -- and its
// activation pass writes a_k = 2 r_k, the next conv's input, directly: no pass for r + h, no
// second tensor.  Step t uses (gamma, beta) and writes a_t = r_t.  In the backward a step
// k < t is then an InstanceNorm with affine (2 gamma, 2 beta): its dgamma / dbeta are
// doubled as they are accumulated, and its conv weight gradient needs no factor (its input
// a_{k-1} already carries it).
//
// Accumulation order.  The shared conv weight and IN_ru affine receive t contributions.
// Step t writes the gradient, steps t-1 .. 1 go to a scratch tensor and are added in that
// order by accumulate() on the plan's stream: one fixed order, bitwise repeatable.
//
// Everything else runs on the engine's kernels: conv3d_run / conv3d_wgrad (any
// SPFF_MATH_*), slab_reduce + in_mean / in_rstd per (b, c) (InstanceNorm, eps 1e-5, biased
// variance), act_apply / in_bwd_apply with ReLU's zero slope, linear_* for the bias-free
// 1x1x1 convs (two-source [up | skip] views, residual operand), maxpool3_*, the 2x2x2
// upconv_* GEMMs and head_*.  Level 0's inp has in_ch (1..8) input channels: it runs on the
// same GEMM through the input's zero-padded 8-channel rows (x_cl) and a weight image whose
// rows past in_ch are zero; no dedicated kernel.
// Saved for backward per block: x1, y_k (raw conv outputs), a_k, s, o, the statistics and
// the pool argmax bytes.
#include "plan_ops.h"

#include <algorithm>
#include <string>
#include <vector>

using namespace spff;

namespace {

constexpr int NLVL = 5, NBLK = 9, NUP = 4, TMAX = 8;

struct RBlk {
  std::string name;
  int lvl, Cin, C;
  int64_t w_inp = -1, g_ru = -1, b_ru = -1, w_out = -1, g_bn = -1, b_bn = -1;
  Conv3 cv[1];               // the recurrent unit's conv, shared by the t steps
  size_t x1, y[TMAX], a[TMAX], s, out;
  Stat4 st[TMAX], bn;
  size_t gb2 = 0;            // [2][C]: 2 gamma_ru, 2 beta_ru (t > 1)
  size_t pk_inp, pk_out;     // head_pack images of the two 1x1x1 convs
};

// gb2 = [2 gamma | 2 beta]: the affine of the recurrence's steps k < t
__global__ void k_r2u_double(const float* __restrict__ gamma, const float* __restrict__ beta,
                             float* __restrict__ gb2, int C) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < C) {
    gb2[c] = 2.f * gamma[c];
    gb2[C + c] = 2.f * beta[c];
  }
}

}  // namespace

struct spff_r2u : PlanBase {
  spff_r2u_cfg cfg;
  Vol vol[NLVL];
  int f, K, ldx, t;
  RBlk blk[NBLK];  // e1..e4, b, d4..d1
  UpConv up[NUP];  // up4, up3, up2, up1
  int64_t head_w = -1, head_b = -1;
  size_t head_pk = 0, x_cl = 0, pool[4] = {}, pidx[4] = {};
  size_t red_ws = 0, red_out = 0, kk1 = 0, kk2 = 0, wg_ws = 0, wt = 0;
  size_t tmp_w = 0, tmp_gb = 0, db_scr = 0;
  bool pkb = false;
  size_t wsl = 0;  // SPFF_MATH_F16X3 max |w| per block's conv (batched plans)
  size_t G_out = 0, G_s = 0, G_1 = 0, G_2 = 0, G_dx = 0, dskip[4] = {};
};

namespace {

void reg_block(spff_r2u* p, RBlk& b) {
  const int C = b.C;
  const std::string n = "backbone." + b.name;
  b.w_inp = p->reg(n + ".inp.weight", {C, b.Cin, 1, 1, 1});
  b.cv[0] = reg_conv(p, n + ".ru.conv.weight", C, C);
  b.g_ru = p->reg(n + ".ru.inn.weight", {C});
  b.b_ru = p->reg(n + ".ru.inn.bias", {C});
  b.w_out = p->reg(n + ".out.weight", {C, C, 1, 1, 1});
  b.g_bn = p->reg(n + ".bn.weight", {C});
  b.b_bn = p->reg(n + ".bn.bias", {C});
}

int build(spff_r2u* p) {
  const spff_r2u_cfg& c = p->cfg;
  if (c.batch < 1 || c.depth < 1 || c.height < 1 || c.width < 1)
    return plan_fail(SPFF_EINVAL, "invalid batch / depth / height / width");
  if (c.in_ch < 1 || c.in_ch > 8) return plan_fail(SPFF_EINVAL, "in_ch must be 1..8");
  if (c.num_classes < 2 || c.num_classes > 32)
    return plan_fail(SPFF_EINVAL, "num_classes must be 2..32 (the sigmoid branch, K = 1, is not built)");
  if (c.base < 8 || c.base % 8) return plan_fail(SPFF_EINVAL, "base must be a multiple of 8");
  if (c.t < 1 || c.t > TMAX) return plan_fail(SPFF_EINVAL, "t must be 1..8");
  if (c.math < SPFF_MATH_F32 || c.math > SPFF_MATH_F16X3)
    return plan_fail(SPFF_EINVAL, "math must be one of SPFF_MATH_*");
  if (c.depth % 16 || c.height % 16 || c.width % 16)
    return plan_fail(SPFF_ESHAPE,
                 "D, H and W must be multiples of 16 (four MaxPool3d(2) whose outputs are "
                 "concatenated with the ConvTranspose3d outputs); the Lit wrapper pads");
  p->f = c.base;
  p->K = c.num_classes;
  p->t = c.t;
  p->ldx = 8;
  for (int l = 0; l < NLVL; ++l)
    p->vol[l] = Vol{c.batch, c.depth >> l, c.height >> l, c.width >> l};
  const int f = p->f, T = p->t;
  const char* names[NBLK] = {"e1", "e2", "e3", "e4", "b", "d4", "d3", "d2", "d1"};
  const int lvl[NBLK] = {0, 1, 2, 3, 4, 3, 2, 1, 0};
  const int cin[NBLK] = {c.in_ch, f, 2 * f, 4 * f, 8 * f, 16 * f, 8 * f, 4 * f, 2 * f};
  const int cc[NBLK] = {f, 2 * f, 4 * f, 8 * f, 16 * f, 8 * f, 4 * f, 2 * f, f};
  for (int i = 0; i < NBLK; ++i) {
    RBlk& b = p->blk[i];
    b.name = names[i];
    b.lvl = lvl[i];
    b.Cin = cin[i];
    b.C = cc[i];
  }
  // registration order of R2UNet3D_backbone.__init__, then the Lit head
  for (int i = 0; i < 5; ++i) reg_block(p, p->blk[i]);
  const char* upn[NUP] = {"up4", "up3", "up2", "up1"};
  for (int u = 0; u < NUP; ++u) {
    UpConv& U = p->up[u];
    U.Cin = 16 * f >> u;
    U.Cout = 8 * f >> u;
    U.Llow = 4 - u;
    U.w = p->reg(std::string("backbone.") + upn[u] + ".weight", {U.Cin, U.Cout, 2, 2, 2});
    U.b = p->reg(std::string("backbone.") + upn[u] + ".bias", {U.Cout});
    reg_block(p, p->blk[5 + u]);
  }
  p->head_w = p->reg("head.weight", {p->K, f, 1, 1, 1});
  p->head_b = p->reg("head.bias", {p->K});

  // ---- workspace ----
  const Vol& v0 = p->vol[0];
  const int B = c.batch;
  p->x_cl = p->alloc(nvox(v0) * p->ldx * sizeof(float));
  size_t red_ws = 0, red_out = 0, wg = 0, wt = 0;
  for (int i = 0; i < NBLK; ++i) {
    RBlk& b = p->blk[i];
    const Vol& v = p->vol[b.lvl];
    const int64_t M = nvox(v);
    const size_t act = M * b.C * sizeof(float);
    const size_t bc = (size_t)B * b.C * sizeof(float);
    b.x1 = p->alloc(act);
    for (int k = 0; k < T; ++k) {
      b.y[k] = p->alloc(act);
      b.a[k] = p->alloc(act);
      b.st[k] = stat_alloc(p, bc);
    }
    b.s = p->alloc(act);
    b.out = p->alloc(act);
    b.bn = stat_alloc(p, bc);
    if (T > 1) b.gb2 = p->alloc((size_t)2 * b.C * sizeof(float));
    // the GEMM reads level 0's input through its 8-channel rows: same image size
    b.pk_inp = p->alloc(head_pack_floats(i == 0 ? p->ldx : b.Cin, b.C) * sizeof(float));
    b.pk_out = p->alloc(head_pack_floats(b.C, b.C) * sizeof(float));
    red_ws = std::max(red_ws, slab_reduce_ws_bytes(v, b.C, 2));
    red_out = std::max(red_out, (size_t)B * b.C * v.D * 2 * sizeof(float));
    wg = std::max(wg, conv3d_wgrad_ws_bytes(v, 3, b.C, b.C));
    wg = std::max(wg, conv3d_splitk_bytes(v, 3, b.C, b.C));
    wg = std::max(wg, linear_wgrad_ws_bytes(M, b.Cin, b.C));
    wg = std::max(wg, linear_wgrad_ws_bytes(M, b.C, b.C));
    wt = std::max(wt, conv3d_pack_bytes(3, b.C, b.C));
  }
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
  p->wg_ws = p->alloc(wg);
  p->tmp_w = p->alloc((size_t)16 * f * 16 * f * 27 * sizeof(float));
  p->tmp_gb = p->alloc((size_t)2 * 16 * f * sizeof(float));
  p->db_scr = p->alloc((size_t)16 * f * sizeof(float));
  alloc_convs(p, p->blk, NBLK, wt);
  size_t gmax = 0;  // max over levels of V_l * C_l
  for (int l = 0; l < NLVL; ++l)
    gmax = std::max(gmax, (size_t)nvox(p->vol[l]) * (size_t)(f << l) * sizeof(float));
  p->G_out = p->alloc(gmax);
  p->G_s = p->alloc(gmax);
  p->G_1 = p->alloc(gmax);
  p->G_2 = p->alloc(gmax);
  p->G_dx = p->alloc(gmax);
  for (int l = 0; l < 4; ++l)
    p->dskip[l] = p->alloc(nvox(p->vol[l]) * (f << l) * sizeof(float));
  return SPFF_OK;
}

// the weights' derived images at the forward start (they do not change between a step's
// forward and backward): the 1x1x1 GEMM images, the doubled IN affine and, for the split
// arithmetics, the conv images (forward and input gradient) in one launch pair
int prep_weights(spff_r2u* p) {
  for (int i = 0; i < NBLK; ++i) {
    RBlk& b = p->blk[i];
    const int kin = i == 0 ? p->ldx : b.Cin;
    float* pi = p->F(b.pk_inp);
    float* po = p->F(b.pk_out);
    // (level 0: head_pack zero-fills rows in_ch .. 31 of the forward image, which the
    //  8-channel rows of x_cl meet with zeros of their own)
    PLAN_HIPCK(head_pack(p->P(b.w_inp), pi, pi + head_pack_dgrad_offset(kin, b.C), b.Cin, b.C, p->st));
    PLAN_HIPCK(head_pack(p->P(b.w_out), po, po + head_pack_dgrad_offset(b.C, b.C), b.C, b.C, p->st));
    if (p->t > 1) {
      hipLaunchKernelGGL(k_r2u_double, dim3((b.C + 255) / 256), dim3(256), 0, p->st,
                         p->P(b.g_ru), p->P(b.b_ru), p->F(b.gb2), b.C);
      PLAN_HIPCK(hipGetLastError());
    }
  }
  return prep_convs(p, p->blk, NBLK);
}

// affine of recurrence step k (0-based): doubled for every step but the last
const float* ru_gamma(const spff_r2u* p, const RBlk& b, int k) {
  return k < p->t - 1 ? p->F(b.gb2) : p->P(b.g_ru);
}
const float* ru_beta(const spff_r2u* p, const RBlk& b, int k) {
  return k < p->t - 1 ? p->F(b.gb2) + b.C : p->P(b.b_ru);
}

int fwd_block(spff_r2u* p, RBlk& b, const Src2& in, int kin) {
  const Vol& v = p->vol[b.lvl];
  const int C = b.C;
  const int64_t M = nvox(v);
  PLAN_HIPCK(linear_fwd2(in, kin, p->F(b.pk_inp), nullptr, p->F(b.x1), C, C, M, p->st));
  const float* cur = p->F(b.x1);
  for (int k = 0; k < p->t; ++k) {
    PLAN_CK(conv_run(p, b.cv[0], false, src1(cur, C), dst1(p->F(b.y[k]), C), v));
    PLAN_CK(in_fwd(p, v, C, p->F(b.y[k]), b.st[k], ru_gamma(p, b, k), ru_beta(p, b, k)));
    PLAN_HIPCK(act_apply(p->F(b.y[k]), p->F(b.a[k]), p->F(b.st[k].al), p->F(b.st[k].de), nullptr,
                     nullptr, v, C, p->st, 0.f));
    cur = p->F(b.a[k]);
  }
  PLAN_HIPCK(linear_fwd(cur, C, C, p->F(b.pk_out), nullptr, p->F(b.s), C, C, M, p->F(b.x1), C, p->st));
  PLAN_CK(in_fwd(p, v, C, p->F(b.s), b.bn, p->P(b.g_bn), p->P(b.b_bn)));
  PLAN_HIPCK(act_apply(p->F(b.s), p->F(b.out), p->F(b.bn.al), p->F(b.bn.de), nullptr, nullptr, v, C,
                   p->st, 0.f));
  return SPFF_OK;
}

int bwd_block(spff_r2u* p, RBlk& b, const float* dout, const Dst2* dx, const Src2& in) {
  const Vol& v = p->vol[b.lvl];
  const int C = b.C, math = p->cfg.math, T = p->t;
  const int64_t M = nvox(v);
  const int64_t nw = (int64_t)C * C * 27;
  float* ds = p->F(p->G_s);
  float* g = p->F(p->G_1);
  float* gn = p->F(p->G_2);
  float* wgs = p->F(p->wg_ws);
  // o = relu(IN_bn(s)): ds, which is also the residual branch's share of dx1
  PLAN_CK(in_bwd(p, v, C, p->F(b.s), dout, ds, b.bn, p->P(b.g_bn), p->DP(b.g_bn), p->DP(b.b_bn),
                 0.f));
  // s = x1 + out(a_t)
  PLAN_HIPCK(linear_wgrad(p->F(b.a[T - 1]), C, C, ds, C, C, p->DP(b.w_out), p->F(p->db_scr), M, wgs,
                      p->st));
  PLAN_HIPCK(linear_dgrad(ds, C, C, p->F(b.pk_out) + head_pack_dgrad_offset(C, C), g, C, C, M, nullptr,
                      p->st));
  // the recurrence, steps t .. 1: g holds dL/da_k
  for (int k = T - 1; k >= 0; --k) {
    const bool last = k == T - 1;
    float* dgam = last ? p->DP(b.g_ru) : p->F(p->tmp_gb);
    float* dbet = last ? p->DP(b.b_ru) : p->F(p->tmp_gb) + C;
    PLAN_CK(in_bwd(p, v, C, p->F(b.y[k]), g, g, b.st[k], ru_gamma(p, b, k), dgam, dbet, 0.f));
    if (!last) {  // affine (2 gamma, 2 beta): d/dgamma = 2 d/d(2 gamma)
      PLAN_HIPCK(accumulate(p->DP(b.g_ru), dgam, C, 2.f, p->st));
      PLAN_HIPCK(accumulate(p->DP(b.b_ru), dbet, C, 2.f, p->st));
    }
    const float* xin = k == 0 ? p->F(b.x1) : p->F(b.a[k - 1]);
    float* dw = last ? p->DP(b.cv[0].w) : p->F(p->tmp_w);
    PLAN_HIPCK(conv3d_wgrad(src1(xin, C), g, C, dw, v, 3, C, C, math, wgs, p->st));
    if (!last) PLAN_HIPCK(accumulate(p->DP(b.cv[0].w), dw, nw, 1.f, p->st));
    PLAN_CK(conv_run(p, b.cv[0], true, src1(g, C), dst1(gn, C), v));
    std::swap(g, gn);
  }
  // x1 feeds the recurrent unit and the residual: dx1 = ds + (the unit's input gradient)
  PLAN_HIPCK(accumulate(ds, g, M * C, 1.f, p->st));
  PLAN_HIPCK(linear_wgrad2(in, b.Cin, ds, C, C, p->DP(b.w_inp), p->F(p->db_scr), M, wgs, p->st));
  if (dx)
    PLAN_HIPCK(linear_dgrad2(ds, C, C, p->F(b.pk_inp) + head_pack_dgrad_offset(b.Cin, C), *dx, b.Cin,
                         M, 0, p->st));
  return SPFF_OK;
}

int forward(spff_r2u* p, const float* x, float* logits) {
  PLAN_HIPCK(ncdhw_to_ndhwc(x, p->F(p->x_cl), p->vol[0], p->cfg.in_ch, p->ldx, p->st));
  PLAN_CK(prep_weights(p));
  return unet5_forward(p, p->head_w, p->head_b, logits, [&](RBlk& b, const Src2& in, int kin) {
    return fwd_block(p, b, in, kin);
  });
}

int backward(spff_r2u* p, const float* dl) {
  return unet5_backward(p, p->head_w, p->head_b, dl,
                        [&](RBlk& b, const float* dout, const Dst2* dx, const Src2& in) {
                          return bwd_block(p, b, dout, dx, in);
                        });
}

}  // namespace

// =================================================================== C ABI ==
extern "C" {

int spff_r2u_create(const spff_r2u_cfg* cfg, spff_r2u** out) {
  return plan_create(cfg, out, build);
}

void spff_r2u_destroy(spff_r2u* p) { delete p; }

int spff_r2u_num_params(const spff_r2u* p) { return p ? (int)p->params.size() : 0; }

int spff_r2u_param_info(const spff_r2u* p, int i, const char** name, int* ndim, int64_t shape[5],
                        int64_t* offset, int64_t* numel) {
  if (!p) return plan_fail(SPFF_EINVAL, "param index");
  return plan_param_info(p->params, i, name, ndim, shape, offset, numel);
}

int64_t spff_r2u_param_floats(const spff_r2u* p) { return p ? p->nparam : 0; }
size_t spff_r2u_workspace_bytes(const spff_r2u* p) { return p ? p->total : 0; }

int spff_r2u_forward(spff_r2u* p, const float* x, const float* params, float* logits, void* ws,
                     void* stream) {
  if (!p || !x || !params || !logits || !ws) return plan_fail(SPFF_EINVAL, "null argument");
  p->bind(ws, params, nullptr, stream);
  return forward(p, x, logits);
}

int spff_r2u_backward(spff_r2u* p, const float* dlogits, const float* params, float* dparams,
                      void* ws, void* stream) {
  if (!p || !dlogits || !params || !dparams || !ws) return plan_fail(SPFF_EINVAL, "null argument");
  p->bind(ws, params, dparams, stream);
  return backward(p, dlogits);
}

int spff_r2u_saved_tensor(const spff_r2u* p, void* ws, const char* name, const float** ptr,
                          int64_t* nv, int* ch) {
  if (!p || !ws || !name || !ptr) return plan_fail(SPFF_EINVAL, "null argument");
  const std::string n(name);
  const SavedOut ret{ws, ptr, nv, ch};
  for (int i = 0; i < NBLK; ++i) {
    const RBlk& b = p->blk[i];
    const Vol& v = p->vol[b.lvl];
    if (n == b.name + ".x1") return ret(b.x1, v, b.C);
    if (n == b.name + ".out") return ret(b.out, v, b.C);
    for (int k = 0; k < p->t; ++k)
      if (n == b.name + ".ru" + std::to_string(k + 1)) return ret(b.a[k], v, b.C);
  }
  return plan_fail(SPFF_EINVAL, "unknown saved tensor " + n);
}

size_t spff_r2u_dice_loss_ws_bytes(int batch, int num_classes) {
  return dice_ce_ws_bytes(batch, num_classes);
}

int spff_r2u_dice_loss(const float* logits, const int64_t* labels, int batch,
                       int64_t vox_per_sample, int num_classes, int use_ignore, int ignore_index,
                       float* out4, float* dlogits, void* ws, void* stream) {
  if (!logits || !labels || !out4 || !dlogits || !ws) return plan_fail(SPFF_EINVAL, "null argument");
  if (batch < 1 || vox_per_sample < 1) return plan_fail(SPFF_EINVAL, "invalid batch / vox_per_sample");
  if (num_classes < 2 || num_classes > 32)
    return plan_fail(SPFF_EINVAL, "num_classes must be 2..32 (the sigmoid branch, K = 1, is not built)");
  PLAN_HIPCK(soft_dice_loss({DICE_R2U}, logits, labels, batch, vox_per_sample, num_classes,
                        use_ignore, ignore_index, out4, dlogits, ws,
                        static_cast<hipStream_t>(stream)));
  return SPFF_OK;
}

}  // extern "C"
