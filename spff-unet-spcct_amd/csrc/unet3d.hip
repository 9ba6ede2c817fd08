// 3D U-Net baseline variant (BASELINE config 3): the Cicek et al. 3D U-Net of
// the reference's "3DUNet" registry entry (config.py:283-311), behind
// LitCicek3DUNet_DepthAdapter_Published (models.py:756-853).
//
// Graph (Cicek3DUNet.forward, models.py:743-753), levels l = 0..4 halve D, H, W:
//   e1 = enc1(x); e2 = enc2(pool(e1)); e3 = enc3(pool(e2)); e4 = enc4(pool(e3))
//   b  = bott(pool(e4))
//   d4 = dec4([up4(b) | e4]); d3 = dec3([up3(d4) | e3]); d2 = dec2([up2(d3) | e2])
//   d1 = dec1([up1(d2) | e1]); logits = out(d1)
// Block (models.py:721-726): y1 = conv(x); a1 = relu(BN(y1)); y2 = conv(a1);
// out = relu(BN(y2)), Conv3d(3, padding 1, bias=False) since use_bn=True.
// The depth adapter (models.py:771-777) resamples the input's D to target_depth
// before the backbone and the logits back afterwards (misc.hip).
//
// Everything runs on the SPFF engine's kernels: the 3x3x3 convs of
// conv3d_x.hip / conv3d_wgx.hip (any SPFF_MATH_*), the per-(b,c,d) slab
// reductions of norm.hip finalised per channel for BatchNorm, act_apply /
// in_bwd_apply with ReLU's zero slope, the ConvTranspose GEMMs of gemm.hip with
// 8 sub-lattices, and the 2x2x2 max pool of misc.hip.  Saved for backward:
// y1, a1, y2, out per block, the pool argmax bytes and the statistics.
#include "plan_ops.h"

#include <string>
#include <vector>

using namespace spff;

namespace {

constexpr int NLVL = 5, NBLK = 9, NUP = 4;
constexpr double BN_MOM = 0.1, BN_EPS = 1e-5;  // nn.BatchNorm3d defaults

struct UBlk {
  std::string name;
  int lvl, Cin, C;
  Conv3 cv[2];
  int64_t g1 = -1, b1 = -1, g2 = -1, b2 = -1;      // params
  int64_t rm1 = -1, rv1 = -1, rm2 = -1, rv2 = -1;  // buffers
  size_t y1, a1, y2, out;
  Stat4 s1, s2;
};

}  // namespace

struct spff_unet3d : PlanBase {
  spff_unet3d_cfg cfg;
  Vol vol[NLVL];
  int f, K, ldx, Dt;
  std::vector<ParamEnt> bufs;  // BatchNorm running statistics: the second flat buffer
  int64_t nbuf = 0;
  UBlk blk[NBLK];  // enc1..enc4, bott, dec4..dec1
  UpConv up[NUP];  // up4, up3, up2, up1
  int64_t out_w = -1, out_b = -1;
  size_t head_pk = 0, x_cl = 0, pool[4] = {}, pidx[4] = {};
  size_t red_ws = 0, red_out = 0, kk1 = 0, kk2 = 0, wg_ws = 0, wt = 0;
  bool pkb = false;  // conv images packed in one batch at the forward start
  size_t wsl = 0;    // SPFF_MATH_F16X3 max |w| per conv (batched plans)
  size_t G_out = 0, G_dy2 = 0, G_da1 = 0, G_dx = 0, dskip[4] = {}, logit_t = 0, dl_t = 0;
  bool last_training = true;
  // synchronised BatchNorm (spff_unet3d_set_sync_bn): the per-channel batch moments and the
  // backward's two per-channel sums are all-reduced (fp64) over the data-parallel group, so
  // every rank normalises with the GLOBAL batch statistics (torch.nn.SyncBatchNorm); world
  // 1 or no table: per-replica statistics, as DDP without SyncBN
  Coll co;
  size_t bnp = 0;  // fp64 per-channel partials [2][16 f]
  float* buf = nullptr;  // per call, beside PlanBase's

  float* BF(int64_t off) const { return off < 0 || !buf ? nullptr : buf + off; }
  int64_t regb(const std::string& name, int64_t n) {
    bufs.push_back(ParamEnt{name, {n}, nbuf, n});
    nbuf += n;
    return nbuf - n;
  }
};

namespace {

void reg_block(spff_unet3d* p, UBlk& b) {
  const int C = b.C;
  // nn.Sequential(conv, BN, ReLU, conv, BN, ReLU): indices 0, 1, 3, 4
  b.cv[0] = reg_conv(p, b.name + ".0.weight", b.Cin, C);
  b.g1 = p->reg(b.name + ".1.weight", {C});
  b.b1 = p->reg(b.name + ".1.bias", {C});
  b.cv[1] = reg_conv(p, b.name + ".3.weight", C, C);
  b.g2 = p->reg(b.name + ".4.weight", {C});
  b.b2 = p->reg(b.name + ".4.bias", {C});
  b.rm1 = p->regb(b.name + ".1.running_mean", C);
  b.rv1 = p->regb(b.name + ".1.running_var", C);
  b.rm2 = p->regb(b.name + ".4.running_mean", C);
  b.rv2 = p->regb(b.name + ".4.running_var", C);
}

int build(spff_unet3d* p) {
  const spff_unet3d_cfg& c = p->cfg;
  if (c.batch < 1 || c.in_ch < 1 || c.depth < 1 || c.num_classes < 1 ||
      c.num_classes > SPFF_MAX_CLASSES)
    return plan_fail(SPFF_EINVAL, "invalid batch/in_ch/depth/num_classes (K must be 1..SPFF_MAX_CLASSES)");
  if (c.base < 8 || c.base % 8) return plan_fail(SPFF_EINVAL, "base must be a multiple of 8");
  if (c.in_ch > 64) return plan_fail(SPFF_EINVAL, "in_ch > 64 not supported");
  if (c.math < SPFF_MATH_F32 || c.math > SPFF_MATH_F16X3)
    return plan_fail(SPFF_EINVAL, "math must be one of SPFF_MATH_*");
  if (c.target_depth < 0) return plan_fail(SPFF_EINVAL, "target_depth must be >= 0");
  p->Dt = c.target_depth > 0 ? c.target_depth : c.depth;
  if (p->Dt % 16 || c.height % 16 || c.width % 16 || c.height < 16 || c.width < 16)
    return plan_fail(SPFF_ESHAPE,
                 "backbone D, H and W must be multiples of 16 (four MaxPool3d(2) whose outputs "
                 "torch.cat with the ConvTranspose3d outputs, models.py:743-752)");
  p->f = c.base;
  p->K = c.num_classes;
  p->ldx = rup(c.in_ch, 8);
  for (int l = 0; l < NLVL; ++l)
    p->vol[l] = Vol{c.batch, p->Dt >> l, c.height >> l, c.width >> l};
  const int f = p->f;
  const char* names[NBLK] = {"enc1", "enc2", "enc3", "enc4", "bott",
                             "dec4", "dec3", "dec2", "dec1"};
  const int lvl[NBLK] = {0, 1, 2, 3, 4, 3, 2, 1, 0};
  const int cin[NBLK] = {c.in_ch, f, 2 * f, 4 * f, 8 * f, 16 * f, 8 * f, 4 * f, 2 * f};
  const int cc[NBLK] = {f, 2 * f, 4 * f, 8 * f, 16 * f, 8 * f, 4 * f, 2 * f, f};
  for (int i = 0; i < NBLK; ++i) {
    UBlk& b = p->blk[i];
    b.name = names[i];
    b.lvl = lvl[i];
    b.Cin = cin[i];
    b.C = cc[i];
  }
  // registration order of Cicek3DUNet.__init__ (models.py:727-741)
  for (int i = 0; i < 5; ++i) reg_block(p, p->blk[i]);
  p->blk[0].cv[0].dx = false;  // the network's input
  const char* upn[NUP] = {"up4", "up3", "up2", "up1"};
  for (int u = 0; u < NUP; ++u) {
    UpConv& U = p->up[u];
    U.Cin = 16 * f >> u;
    U.Cout = 8 * f >> u;
    U.Llow = 4 - u;
    U.w = p->reg(std::string(upn[u]) + ".weight", {U.Cin, U.Cout, 2, 2, 2});
    U.b = p->reg(std::string(upn[u]) + ".bias", {U.Cout});
    reg_block(p, p->blk[5 + u]);
  }
  p->out_w = p->reg("out.weight", {p->K, f, 1, 1, 1});
  p->out_b = p->reg("out.bias", {p->K});

  // ---- workspace ----
  const Vol& v0 = p->vol[0];
  const int B = c.batch;
  p->x_cl = p->alloc(nvox(v0) * p->ldx * sizeof(float));
  size_t red_ws = 0, red_out = 0, wg = 0, wt = 0;
  for (int i = 0; i < NBLK; ++i) {
    UBlk& b = p->blk[i];
    const Vol& v = p->vol[b.lvl];
    const size_t act = nvox(v) * b.C * sizeof(float);
    b.y1 = p->alloc(act);
    b.a1 = p->alloc(act);
    b.y2 = p->alloc(act);
    b.out = p->alloc(act);
    const size_t bc = (size_t)B * b.C * sizeof(float);
    b.s1 = stat_alloc(p, bc);
    b.s2 = stat_alloc(p, bc);
    red_ws = std::max(red_ws, slab_reduce_ws_bytes(v, b.C, 2));
    red_out = std::max(red_out, (size_t)B * b.C * v.D * 2 * sizeof(float));
    wg = std::max(wg, conv3d_wgrad_ws_bytes(v, 3, b.Cin, b.C));
    wg = std::max(wg, conv3d_wgrad_ws_bytes(v, 3, b.C, b.C));
    wg = std::max(wg, conv3d_splitk_bytes(v, 3, b.Cin, b.C));
    wg = std::max(wg, conv3d_splitk_bytes(v, 3, b.C, b.C));
    wt = std::max(wt, conv3d_pack_bytes(3, b.Cin, b.C));
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
  p->bnp = p->alloc((size_t)2 * 16 * f * sizeof(double));
  p->wg_ws = p->alloc(wg);
  alloc_convs(p, p->blk, NBLK, wt);
  size_t gmax = 0;  // max over levels of V_l * C_l (the bottleneck has 16 f channels)
  for (int l = 0; l < NLVL; ++l)
    gmax = std::max(gmax, (size_t)nvox(p->vol[l]) * (size_t)(f << l) * sizeof(float));
  p->G_out = p->alloc(gmax);
  p->G_dy2 = p->alloc(gmax);
  p->G_da1 = p->alloc(gmax);
  p->G_dx = p->alloc(gmax);
  for (int l = 0; l < 4; ++l)
    p->dskip[l] = p->alloc(nvox(p->vol[l]) * (f << l) * sizeof(float));
  if (p->Dt != c.depth) {
    p->logit_t = p->alloc(nvox(v0) * p->K * sizeof(float));
    p->dl_t = p->alloc(nvox(v0) * p->K * sizeof(float));
  }
  return SPFF_OK;
}

// BatchNorm3d over a conv output y (models.py:720): batch statistics + running
// update in training, running statistics in eval
int bn_fwd(spff_unet3d* p, const Vol& v, int C, size_t y, const Stat4& s, int64_t g, int64_t b,
           int64_t rm, int64_t rv, bool training) {
  if (!training) {
    PLAN_HIPCK(bn_eval(p->BF(rm), p->BF(rv), p->P(g), p->P(b), p->F(s.mean), p->F(s.rstd), p->F(s.al),
                   p->F(s.de), BN_EPS, v.B, C, p->st));
    return SPFF_OK;
  }
  RedArgs a{};
  a.y = p->F(y);
  PLAN_HIPCK(slab_reduce(RED_SUM, a, v, C, p->F(p->red_out), p->F(p->red_ws), p->st));
  if (p->co.on()) {  // SyncBN: global moments (same fp64 per-channel sums, then the group's)
    double* part = reinterpret_cast<double*>(p->ws + p->bnp);
    const double N = (double)nvox(v) * p->co.world;  // every rank runs the plan's shape
    PLAN_HIPCK(bn_partial(p->F(p->red_out), part, v, C, 1, p->st));
    PLAN_HIPCK(p->co.sum_f64(part, C, p->st));
    PLAN_HIPCK(bn_mean_fin(part, p->F(s.mean), v.B, C, N, p->st));
    a.mean = p->F(s.mean);
    PLAN_HIPCK(slab_reduce(RED_SQDEV, a, v, C, p->F(p->red_out), p->F(p->red_ws), p->st));
    PLAN_HIPCK(bn_partial(p->F(p->red_out), part, v, C, 1, p->st));
    PLAN_HIPCK(p->co.sum_f64(part, C, p->st));
    PLAN_HIPCK(bn_rstd_fin(part, p->P(g), p->P(b), p->F(s.mean), p->F(s.rstd), p->F(s.al), p->F(s.de),
                       p->BF(rm), p->BF(rv), BN_MOM, BN_EPS, v.B, C, N, p->st));
    return SPFF_OK;
  }
  PLAN_HIPCK(bn_mean(p->F(p->red_out), p->F(s.mean), v, C, p->st));
  a.mean = p->F(s.mean);
  PLAN_HIPCK(slab_reduce(RED_SQDEV, a, v, C, p->F(p->red_out), p->F(p->red_ws), p->st));
  PLAN_HIPCK(bn_rstd(p->F(p->red_out), p->P(g), p->P(b), p->F(s.mean), p->F(s.rstd), p->F(s.al), p->F(s.de),
                 p->BF(rm), p->BF(rv), BN_MOM, BN_EPS, v, C, p->st));
  return SPFF_OK;
}

int fwd_block(spff_unet3d* p, UBlk& b, const Src2& in, bool training) {
  const Vol& v = p->vol[b.lvl];
  const int C = b.C;
  PLAN_CK(conv_run(p, b.cv[0], false, in, dst1(p->F(b.y1), C), v));
  PLAN_CK(bn_fwd(p, v, C, b.y1, b.s1, b.g1, b.b1, b.rm1, b.rv1, training));
  PLAN_HIPCK(act_apply(p->F(b.y1), p->F(b.a1), p->F(b.s1.al), p->F(b.s1.de), nullptr, nullptr, v, C,
                   p->st, 0.f));
  PLAN_CK(conv_run(p, b.cv[1], false, src1(p->F(b.a1), C), dst1(p->F(b.y2), C), v));
  PLAN_CK(bn_fwd(p, v, C, b.y2, b.s2, b.g2, b.b2, b.rm2, b.rv2, training));
  PLAN_HIPCK(act_apply(p->F(b.y2), p->F(b.out), p->F(b.s2.al), p->F(b.s2.de), nullptr, nullptr, v, C,
                   p->st, 0.f));
  return SPFF_OK;
}

// BatchNorm + ReLU backward: dy = rstd*gamma*(dr - k1 - xhat*k2), dr = g*[r > 0]
int bn_bwd(spff_unet3d* p, const Vol& v, int C, size_t y, const float* g, float* dy,
           const Stat4& s, int64_t gamma, int64_t beta) {
  RedArgs a{};
  a.y = p->F(y); a.g = g; a.mean = p->F(s.mean); a.rstd = p->F(s.rstd);
  a.al = p->F(s.al); a.de = p->F(s.de); a.neg = 0.f;
  PLAN_HIPCK(slab_reduce(RED_BWD_IN, a, v, C, p->F(p->red_out), p->F(p->red_ws), p->st));
  if (p->co.on() && p->last_training) {
    // SyncBN: k1, k2 from the group's sums; dgamma / dbeta are this rank's partial sums
    // (the flat gradient is SUM-all-reduced afterwards, like every other parameter's)
    double* part = reinterpret_cast<double*>(p->ws + p->bnp);
    PLAN_HIPCK(bn_partial(p->F(p->red_out), part, v, C, 2, p->st));
    PLAN_HIPCK(bn_bwd_dgb_part(part, p->DP(gamma), p->DP(beta), C, p->st));
    PLAN_HIPCK(p->co.sum_f64(part, 2 * (int64_t)C, p->st));
    PLAN_HIPCK(bn_bwd_fin(part, p->F(p->kk1), p->F(p->kk2), v.B, C, (double)nvox(v) * p->co.world,
                      p->st));
  } else {
    PLAN_HIPCK(bn_bwd_stats(p->F(p->red_out), p->DP(gamma), p->DP(beta), p->F(p->kk1), p->F(p->kk2),
                        v, C, p->st, p->last_training ? 0 : 1));
  }
  PLAN_HIPCK(in_bwd_apply(p->F(y), g, dy, p->F(s.mean), p->F(s.rstd), p->F(s.al), p->F(s.de), p->P(gamma),
                      nullptr, nullptr, p->F(p->kk1), p->F(p->kk2), v, C, p->st, 0.f));
  return SPFF_OK;
}

int bwd_block(spff_unet3d* p, UBlk& b, const float* dout, const Dst2* dx, const Src2& in) {
  const Vol& v = p->vol[b.lvl];
  const int C = b.C, math = p->cfg.math;
  float* dy2 = p->F(p->G_dy2);
  float* da1 = p->F(p->G_da1);
  PLAN_CK(bn_bwd(p, v, C, b.y2, dout, dy2, b.s2, b.g2, b.b2));
  PLAN_HIPCK(conv3d_wgrad(src1(p->F(b.a1), C), dy2, C, p->DP(b.cv[1].w), v, 3, C, C, math,
                      p->F(p->wg_ws), p->st));
  PLAN_CK(conv_run(p, b.cv[1], true, src1(dy2, C), dst1(da1, C), v));
  PLAN_CK(bn_bwd(p, v, C, b.y1, da1, da1, b.s1, b.g1, b.b1));
  PLAN_HIPCK(conv3d_wgrad(in, da1, C, p->DP(b.cv[0].w), v, 3, b.Cin, C, math, p->F(p->wg_ws), p->st));
  if (dx) PLAN_CK(conv_run(p, b.cv[0], true, src1(da1, C), *dx, v));
  return SPFF_OK;
}

int forward(spff_unet3d* p, const float* x, float* logits, bool training) {
  const spff_unet3d_cfg& c = p->cfg;
  const Vol& v0 = p->vol[0];
  if (p->Dt != c.depth)  // _resize_depth_like (models.py:153-157)
    PLAN_HIPCK(resize_d_ncdhw_to_ndhwc(x, p->F(p->x_cl), c.batch, c.in_ch, c.depth, p->Dt, c.height,
                                   c.width, p->ldx, p->st));
  else
    PLAN_HIPCK(ncdhw_to_ndhwc(x, p->F(p->x_cl), v0, c.in_ch, p->ldx, p->st));
  PLAN_CK(prep_convs(p, p->blk, NBLK));
  float* lt = p->Dt != c.depth ? p->F(p->logit_t) : logits;
  PLAN_CK(unet5_forward(p, p->out_w, p->out_b, lt, [&](UBlk& b, const Src2& in, int) {
    return fwd_block(p, b, in, training);
  }));
  if (p->Dt != c.depth)  // _resize_logits_depth_like (models.py:159-163)
    PLAN_HIPCK(resize_d_rows(lt, logits, c.batch, p->K, p->Dt, c.depth, c.height, c.width, p->st));
  p->last_training = training;
  return SPFF_OK;
}

int backward(spff_unet3d* p, const float* dl) {
  const spff_unet3d_cfg& c = p->cfg;
  const float* d16 = dl;
  if (p->Dt != c.depth) {
    PLAN_HIPCK(resize_d_rows_bwd(dl, p->F(p->dl_t), c.batch, p->K, p->Dt, c.depth, c.height,
                             c.width, p->st));
    d16 = p->F(p->dl_t);
  }
  return unet5_backward(p, p->out_w, p->out_b, d16,
                        [&](UBlk& b, const float* dout, const Dst2* dx, const Src2& in) {
                          return bwd_block(p, b, dout, dx, in);
                        });
}

}  // namespace

// =================================================================== C ABI ==
extern "C" {

int spff_unet3d_create(const spff_unet3d_cfg* cfg, spff_unet3d** out) {
  return plan_create(cfg, out, build);
}

void spff_unet3d_destroy(spff_unet3d* p) { delete p; }

int spff_unet3d_num_params(const spff_unet3d* p) { return p ? (int)p->params.size() : 0; }

int spff_unet3d_param_info(const spff_unet3d* p, int i, const char** name, int* ndim,
                           int64_t shape[5], int64_t* offset, int64_t* numel) {
  if (!p) return plan_fail(SPFF_EINVAL, "param index");
  return plan_param_info(p->params, i, name, ndim, shape, offset, numel);
}

int64_t spff_unet3d_param_floats(const spff_unet3d* p) { return p ? p->nparam : 0; }
int spff_unet3d_num_buffers(const spff_unet3d* p) { return p ? (int)p->bufs.size() : 0; }

int spff_unet3d_buffer_info(const spff_unet3d* p, int i, const char** name, int64_t* offset,
                            int64_t* numel) {
  if (!p) return plan_fail(SPFF_EINVAL, "buffer index");
  return plan_param_info(p->bufs, i, name, nullptr, nullptr, offset, numel, "buffer index");
}

int64_t spff_unet3d_buffer_floats(const spff_unet3d* p) { return p ? p->nbuf : 0; }
size_t spff_unet3d_workspace_bytes(const spff_unet3d* p) { return p ? p->total : 0; }

int spff_unet3d_forward(spff_unet3d* p, const float* x, const float* params, float* buffers,
                        int training, float* logits, void* ws, void* stream) {
  if (!p || !x || !params || !buffers || !logits || !ws) return plan_fail(SPFF_EINVAL, "null argument");
  p->bind(ws, params, nullptr, stream);
  p->buf = buffers;
  p->co.failed = nullptr;
  const int rc = forward(p, x, logits, training != 0);
  if (p->co.failed) return plan_fail(SPFF_ECOLL, std::string("SyncBN ") + p->co.failed + " failed");
  return rc;
}

int spff_unet3d_set_sync_bn(spff_unet3d* p, const spff_coll* coll, int world) {
  if (!p) return plan_fail(SPFF_EINVAL, "null plan");
  if (!coll || world <= 1) {
    p->co = Coll{};
    return SPFF_OK;
  }
  if (!coll->allreduce) return plan_fail(SPFF_EINVAL, "spff_coll needs allreduce");
  p->co = Coll{};
  p->co.world = world;
  p->co.ctx = coll->ctx;
  p->co.allreduce = coll->allreduce;
  p->co.halo = coll->halo;
  return SPFF_OK;
}

int spff_unet3d_backward(spff_unet3d* p, const float* dlogits, const float* params,
                         float* dparams, void* ws, void* stream) {
  if (!p || !dlogits || !params || !dparams || !ws) return plan_fail(SPFF_EINVAL, "null argument");
  p->bind(ws, params, dparams, stream);
  p->co.failed = nullptr;
  const int rc = backward(p, dlogits);
  if (p->co.failed) return plan_fail(SPFF_ECOLL, std::string("SyncBN ") + p->co.failed + " failed");
  return rc;
}

int spff_unet3d_saved_tensor(const spff_unet3d* p, void* ws, const char* name, const float** ptr,
                             int64_t* nv, int* ch) {
  if (!p || !ws || !name || !ptr) return plan_fail(SPFF_EINVAL, "null argument");
  const std::string n(name);
  const SavedOut ret{ws, ptr, nv, ch};
  if (n == "x_cl") return ret(p->x_cl, p->vol[0], p->ldx);
  for (int i = 0; i < NBLK; ++i) {
    const UBlk& b = p->blk[i];
    const Vol& v = p->vol[b.lvl];
    if (n == b.name + ".y1") return ret(b.y1, v, b.C);
    if (n == b.name + ".a1") return ret(b.a1, v, b.C);
    if (n == b.name + ".y2") return ret(b.y2, v, b.C);
    if (n == b.name + ".out") return ret(b.out, v, b.C);
  }
  for (int l = 0; l < 4; ++l)
    if (n == "pool" + std::to_string(l + 1)) return ret(p->pool[l], p->vol[l + 1], p->f << l);
  const char* upn[NUP] = {"up4", "up3", "up2", "up1"};
  for (int u = 0; u < NUP; ++u)
    if (n == upn[u]) return ret(p->up[u].out, p->vol[p->up[u].Llow - 1], p->up[u].Cout);
  return plan_fail(SPFF_EINVAL, "unknown saved tensor " + n);
}

int spff_loss_ex(const float* logits, const int64_t* labels, int64_t nv, int K, int ignore,
                 double smooth, const int64_t* count_override, const float* class_weights,
                 int clamp_denominator, float* out4, float* dlogits, int64_t* conf, void* ws,
                 void* stream) {
  if (!logits || !labels || !out4 || !dlogits || !conf || !ws)
    return plan_fail(SPFF_EINVAL, "null argument");
  if (K < 1 || K > SPFF_MAX_CLASSES)
    return plan_fail(SPFF_EINVAL, "num_classes must be 1..SPFF_MAX_CLASSES");
  PLAN_HIPCK(loss_fwd(logits, labels, nv, K, ignore, smooth, count_override, out4, dlogits, conf,
                  static_cast<float*>(ws), static_cast<hipStream_t>(stream), class_weights,
                  clamp_denominator));
  return SPFF_OK;
}

}  // extern "C"
