// UNETR variant: the reference's "UNETR" registry entry (config.py:316-339) =
// LitUNETR_Published (models.py:1006-1115) around UNETR_Published, i.e. MONAI 1.5.2's UNETR
// with a 16^3 conv patch embedding, a learnable position embedding, twelve pre-norm ViT
// blocks (global attention, exact GELU), InstanceNorm and res_block.  Semantics restated
// in tests/_unetr_oracle.py (parity unpinned: MONAI is not available offline).
//
// Grids: L0 = the network grid img (D, H, W), Ll = L0 / 2^l, tokens at L4 (n = |L4| per
// sample).  Every tensor is channel-last rows, so MONAI's proj_feat is a view.
//   xr = input, resampled to img when the padded input has another size (trilinear)
//   tok = PatchEmbed16(xr) + b + pos;  h(i+1) = Block_i(h i), h0 = tok;  hN = LN(h12)
//   Block: x1 = t + OutProj(Attn(LN1 t));  x2 = x1 + W2 gelu(W1 LN2 x1)
//   hidden_states_out[i] = Block_i's output = h(i+1)
//   enc1 = RB(xr)                                          L0, f
//   enc2 = RB(T(RB(T(T(hs[3])))))                          L1, 2f
//   enc3 = RB(T(T(hs[6])))                                 L2, 4f
//   enc4 = T(hs[9])                                        L3, 8f
//   dec5 = UP(hN, enc4), dec4 = UP(dec5, enc3), dec3 = UP(dec4, enc2), dec2 = UP(dec3, enc1)
//   logits = Conv1x1(dec2) + b, resampled back to the padded size when it differs
//   T: ConvTranspose3d k = s = 2 without bias;  RB / UP: see res_block.h / swin.hip
// The unused cross-attention parameters that MONAI >= 1.4 registers in every block are not
// part of the flat buffer.
#include "res_block.h"

using namespace spff;

namespace {

constexpr int NBLK = 12, NRB = 8, NUP = 10, NLV = 5;
// classes of the library-wide timer (spff_conv_prof_*) beyond the convs' 0 .. 2 and the
// loss's 3, 4: the token path (patch embedding, blocks, final norm; forward and backward)
// and the three resampling passes
constexpr int PROF_VIT = 5, PROF_RESAMPLE = 6;

struct Blk {
  int64_t n1w, n1b, n2w, n2b;
  Lin l1, l2, proj, qkv;
  size_t n1, mu1, rs1, qkvb, O, lse, x1, n2, mu2, rs2, hpre, hact, x2;
};

}  // namespace

struct spff_unetr : PlanBase {
  spff_unetr_cfg cfg;
  Vol vol[NLV];
  int f, K, ldx, hid, mlp, nh, n;  // n: tokens per sample
  bool resample = false;
  VitGeo geo;
  int64_t pos = -1, nfw = -1, nfb = -1;
  Lin pe;
  Blk blk[NBLK];
  // rb: enc1, enc2.blocks.0.1, enc2.blocks.1.1, enc3.blocks.0.1, dec5, dec4, dec3, dec2
  RB rb[NRB];
  // up: enc2.init, enc2.b0, enc2.b1, enc3.init, enc3.b0, enc4.init, dec5 .. dec2
  UpConv up[NUP];
  Lin head;
  size_t x_cl = 0, rows = 0, tok = 0, hN = 0, nmu = 0, nrs = 0, lg = 0;
  size_t ones = 0, zeros = 0, dummy = 0, red_ws = 0, red_out = 0, kk1 = 0, kk2 = 0, wg_ws = 0,
         wt = 0, cst = 0;
  bool pkb = false;
  size_t wsl = 0;
  size_t G_out = 0, G_dz = 0, G_dy2 = 0, G_da1 = 0, G_up = 0;
  size_t d_enc[4] = {}, d_tap[3] = {}, d_hN = 0, d_lg = 0;
  size_t S_a = 0, S_b = 0, S_c = 0, S_qkv = 0, S_h = 0;
  int maxC = 0;
};

namespace {

void reg_up(spff_unetr* p, UpConv& U, const std::string& name, int Cin, int Cout, int Llow) {
  U.Cin = Cin;
  U.Cout = Cout;
  U.Llow = Llow;
  U.w = p->reg(name + ".conv.weight", {Cin, Cout, 2, 2, 2});
}

int build(spff_unetr* p) {
  const spff_unetr_cfg& c = p->cfg;
  if (c.batch < 1 || c.in_ch != 1 || c.num_classes < 1 || c.num_classes > 32)
    return plan_fail(SPFF_EINVAL, "invalid batch / in_ch (1: the registry's) / num_classes (1..32)");
  if (c.depth < 16 || c.height < 16 || c.width < 16 || c.depth % 16 || c.height % 16 ||
      c.width % 16)
    return plan_fail(SPFF_EINVAL, "UNETR: the padded input's D, H, W must be multiples of 16 "
                              "(LitUNETR_Published pads to a multiple of 16)");
  for (int k = 0; k < 3; ++k)
    if (c.img[k] < 16 || c.img[k] % 16)
      return plan_fail(SPFF_EINVAL, "UNETR: img must be multiples of the 16^3 patch");
  if (c.feature_size < 8 || c.feature_size % 8)
    return plan_fail(SPFF_EINVAL, "feature_size must be a positive multiple of 8");
  if (c.hidden < 16 || c.hidden > 768 || c.heads < 1 || c.hidden % c.heads)
    return plan_fail(SPFF_EINVAL, "UNETR: hidden (<= 768) must be a multiple of heads");
  if (c.mlp_dim < 4 || c.mlp_dim % 4) return plan_fail(SPFF_EINVAL, "mlp_dim must be a multiple of 4");
  if (c.math < SPFF_MATH_F32 || c.math > SPFF_MATH_F16X3)
    return plan_fail(SPFF_EINVAL, "math must be one of SPFF_MATH_*");
  const int B = c.batch;
  for (int l = 0; l < NLV; ++l) p->vol[l] = Vol{B, c.img[0] >> l, c.img[1] >> l, c.img[2] >> l};
  p->n = p->vol[4].D * p->vol[4].H * p->vol[4].W;
  if (const char* m = vit_geo_check(B, p->n, c.hidden, c.heads)) return plan_fail(SPFF_EINVAL, m);
  p->geo = vit_geo(B, p->n, c.hidden, c.heads);
  p->resample = c.depth != c.img[0] || c.height != c.img[1] || c.width != c.img[2];
  p->f = c.feature_size;
  p->K = c.num_classes;
  p->ldx = rup(c.in_ch, 8);
  p->hid = c.hidden;
  p->mlp = c.mlp_dim;
  p->nh = c.heads;
  const int f = p->f, Hd = p->hid, n = p->n;
  const int64_t T = (int64_t)B * n;
  const int pk = 4096 * c.in_ch;
  // ---- parameters, in MONAI UNETR registration order (a module's own parameters first)
  p->pos = p->reg("vit.patch_embedding.position_embeddings", {1, n, Hd});
  reg_lin(p, p->pe, "vit.patch_embedding.patch_embeddings", pk, Hd, true,
          {Hd, c.in_ch, 16, 16, 16});
  for (int i = 0; i < NBLK; ++i) {
    Blk& b = p->blk[i];
    const std::string s = "vit.blocks." + std::to_string(i) + ".";
    reg_lin(p, b.l1, s + "mlp.linear1", Hd, p->mlp, true);
    reg_lin(p, b.l2, s + "mlp.linear2", p->mlp, Hd, true);
    b.n1w = p->reg(s + "norm1.weight", {Hd});
    b.n1b = p->reg(s + "norm1.bias", {Hd});
    reg_lin(p, b.proj, s + "attn.out_proj", Hd, Hd, true);
    reg_lin(p, b.qkv, s + "attn.qkv", Hd, 3 * Hd, false);
    b.n2w = p->reg(s + "norm2.weight", {Hd});
    b.n2b = p->reg(s + "norm2.bias", {Hd});
  }
  p->nfw = p->reg("vit.norm.weight", {Hd});
  p->nfb = p->reg("vit.norm.bias", {Hd});
  RB* R = p->rb;
  UpConv* U = p->up;
  reg_rb(p, R[0], "encoder1.layer", 0, c.in_ch, f);
  R[0].cv[0].dx = false;  // the network's input
  reg_up(p, U[0], "encoder2.transp_conv_init", Hd, 2 * f, 4);
  reg_up(p, U[1], "encoder2.blocks.0.0", 2 * f, 2 * f, 3);
  reg_rb(p, R[1], "encoder2.blocks.0.1", 2, 2 * f, 2 * f);
  reg_up(p, U[2], "encoder2.blocks.1.0", 2 * f, 2 * f, 2);
  reg_rb(p, R[2], "encoder2.blocks.1.1", 1, 2 * f, 2 * f);
  reg_up(p, U[3], "encoder3.transp_conv_init", Hd, 4 * f, 4);
  reg_up(p, U[4], "encoder3.blocks.0.0", 4 * f, 4 * f, 3);
  reg_rb(p, R[3], "encoder3.blocks.0.1", 2, 4 * f, 4 * f);
  reg_up(p, U[5], "encoder4.transp_conv_init", Hd, 8 * f, 4);
  const char* dn[4] = {"decoder5", "decoder4", "decoder3", "decoder2"};
  const int uci[4] = {Hd, 8 * f, 4 * f, 2 * f};
  const int uco[4] = {8 * f, 4 * f, 2 * f, f};
  for (int u = 0; u < 4; ++u) {
    reg_up(p, U[6 + u], std::string(dn[u]) + ".transp_conv", uci[u], uco[u], 4 - u);
    reg_rb(p, R[4 + u], std::string(dn[u]) + ".conv_block", 3 - u, 2 * uco[u], uco[u]);
  }
  reg_lin(p, p->head, "out.conv.conv", f, p->K, true, {p->K, f, 1, 1, 1});

  // ---- workspace
  const Vol& v0 = p->vol[0];
  p->x_cl = p->alloc(fbytes(nvox(v0) * p->ldx));
  p->rows = p->alloc(fbytes(T * pk));
  p->tok = p->alloc(fbytes(T * Hd));
  p->hN = p->alloc(fbytes(T * Hd));
  p->nmu = p->alloc(fbytes(T));
  p->nrs = p->alloc(fbytes(T));
  if (p->resample) {
    p->lg = p->alloc(fbytes(nvox(v0) * p->K));
    p->d_lg = p->alloc(fbytes(nvox(v0) * p->K));
  }
  int maxC = std::max(std::max(3 * Hd, p->mlp), 16 * f);
  size_t red_ws = 0, red_out = 0, wg = 0, wt = 0, cst = 0, gmax = 0;
  for (int i = 0; i < NBLK; ++i) {
    Blk& b = p->blk[i];
    b.n1 = p->alloc(fbytes(T * Hd));
    b.mu1 = p->alloc(fbytes(T));
    b.rs1 = p->alloc(fbytes(T));
    b.qkvb = p->alloc(fbytes(T * 3 * Hd));
    b.O = p->alloc(fbytes(T * Hd));
    b.lse = p->alloc(fbytes((int64_t)B * p->nh * n));
    b.x1 = p->alloc(fbytes(T * Hd));
    b.n2 = p->alloc(fbytes(T * Hd));
    b.mu2 = p->alloc(fbytes(T));
    b.rs2 = p->alloc(fbytes(T));
    b.hpre = p->alloc(fbytes(T * p->mlp));
    b.hact = p->alloc(fbytes(T * p->mlp));
    b.x2 = p->alloc(fbytes(T * Hd));
  }
  wg = std::max(wg, vit_attn_ws_bytes(p->geo));
  wg = std::max(wg, linear_wgrad_ws_bytes(T, Hd, 3 * Hd));
  wg = std::max(wg, linear_wgrad_ws_bytes(T, Hd, Hd));
  wg = std::max(wg, linear_wgrad_ws_bytes(T, Hd, p->mlp));
  wg = std::max(wg, linear_wgrad_ws_bytes(T, p->mlp, Hd));
  wg = std::max(wg, linear_wgrad_ws_bytes(T, pk, Hd));
  wg = std::max(wg, ln_bwd_ws_bytes(T, Hd));
  p->S_a = p->alloc(fbytes(T * Hd));
  p->S_b = p->alloc(fbytes(T * Hd));
  p->S_c = p->alloc(fbytes(T * Hd));
  p->S_qkv = p->alloc(fbytes(T * 3 * Hd));
  p->S_h = p->alloc(fbytes(T * p->mlp));
  for (int k = 0; k < 3; ++k) p->d_tap[k] = p->alloc(fbytes(T * Hd));
  p->d_hN = p->alloc(fbytes(T * Hd));
  for (int i = 0; i < NRB; ++i) {
    RB& r = R[i];
    const Vol& v = p->vol[r.L];
    const int64_t V = nvox(v);
    const int C = r.C;
    rb_alloc(p, r);
    red_ws = std::max(red_ws, slab_reduce_ws_bytes(v, C, 2));
    red_out = std::max(red_out, fbytes((int64_t)B * C * v.D * 2));
    wg = std::max(wg, conv3d_wgrad_ws_bytes(v, 3, r.Cin, C));
    wg = std::max(wg, conv3d_wgrad_ws_bytes(v, 3, C, C));
    wg = std::max(wg, conv3d_splitk_bytes(v, 3, r.Cin, C));
    wg = std::max(wg, conv3d_splitk_bytes(v, 3, C, C));
    wg = std::max(wg, conv3d_splitk_bytes(v, 3, C, r.Cin));
    if (r.has3) wg = std::max(wg, linear_wgrad_ws_bytes(V, r.Cin, C));
    wt = std::max(wt, conv3d_pack_bytes(3, r.Cin, C));
    wt = std::max(wt, conv3d_pack_bytes(3, C, C));
    cst = std::max(cst, conv3d_stats_bytes(v, 3, r.Cin, C));
    cst = std::max(cst, conv3d_stats_bytes(v, 3, C, C));
    gmax = std::max(gmax, fbytes(V * std::max(C, r.Cin)));
    maxC = std::max(maxC, std::max(C, r.Cin));
  }
  for (int u = 0; u < NUP; ++u) {
    UpConv& X = U[u];
    const int64_t Vh = nvox(p->vol[X.Llow - 1]);
    up_alloc(p, X);
    wg = std::max(wg, upconv_wgrad_ws_bytes(p->vol[X.Llow], X.Cin, X.Cout, 8));
    gmax = std::max(gmax, fbytes(Vh * X.Cout));
    gmax = std::max(gmax, fbytes(nvox(p->vol[X.Llow]) * X.Cin));
  }
  wg = std::max(wg, linear_wgrad_ws_bytes(nvox(v0), f, p->K));
  p->maxC = maxC;
  p->ones = p->alloc(fbytes(maxC));
  p->zeros = p->alloc(fbytes(maxC));
  p->dummy = p->alloc(fbytes(2 * maxC));
  p->red_ws = p->alloc(red_ws);
  p->red_out = p->alloc(red_out);
  p->kk1 = p->alloc(fbytes((int64_t)B * maxC));
  p->kk2 = p->alloc(fbytes((int64_t)B * maxC));
  p->wg_ws = p->alloc(wg);
  alloc_convs(p, R, NRB, wt);
  p->cst = p->alloc(cst);
  p->G_out = p->alloc(gmax);
  p->G_dz = p->alloc(gmax);
  p->G_dy2 = p->alloc(gmax);
  p->G_da1 = p->alloc(gmax);
  p->G_up = p->alloc(gmax);
  // skip gradients: enc1 (L0, f), enc2 (L1, 2f), enc3 (L2, 4f), enc4 (L3, 8f)
  for (int l = 0; l < 4; ++l) p->d_enc[l] = p->alloc(fbytes(nvox(p->vol[l]) * (f << l)));
  return SPFF_OK;
}

int pack_lin(spff_unetr* p, const Lin& l) {
  float* pk = p->F(l.pk);
  PLAN_HIPCK(head_pack(p->P(l.w), pk, pk + head_pack_dgrad_offset(l.K, l.N), l.K, l.N, p->st));
  return SPFF_OK;
}
const float* wd_of(spff_unetr* p, const Lin& l) {
  return p->F(l.pk) + head_pack_dgrad_offset(l.K, l.N);
}

// the MONAI transposed convs have no bias: zeros forward, dummy takes the bias gradient
int up_fwd(spff_unetr* p, UpConv& U, const float* x) { return up_fwd(p, U, x, p->F(p->zeros)); }
int up_bwd(spff_unetr* p, UpConv& U, const float* x, const float* dout, float* dx) {
  return up_bwd(p, U, x, dout, p->F(p->dummy), dx);
}

int block_fwd(spff_unetr* p, Blk& b, const float* tin) {
  const int64_t T = (int64_t)p->cfg.batch * p->n;
  const int C = p->hid, M = p->mlp;
  hipStream_t st = p->st;
  PLAN_HIPCK(ln_fwd(tin, C, C, p->P(b.n1w), p->P(b.n1b), p->F(b.n1), C, p->F(b.mu1), p->F(b.rs1), T,
                st));
  PLAN_CK(pack_lin(p, b.qkv));
  PLAN_HIPCK(linear_fwd(p->F(b.n1), C, C, p->F(b.qkv.pk), nullptr, p->F(b.qkvb), 3 * C, 3 * C, T,
                    nullptr, 0, st));
  PLAN_HIPCK(vit_attn_fwd(p->F(b.qkvb), p->geo, p->F(b.O), p->F(b.lse), st));
  PLAN_CK(pack_lin(p, b.proj));
  PLAN_HIPCK(linear_fwd(p->F(b.O), C, C, p->F(b.proj.pk), p->P(b.proj.b), p->F(b.x1), C, C, T, tin, C,
                    st));
  PLAN_HIPCK(ln_fwd(p->F(b.x1), C, C, p->P(b.n2w), p->P(b.n2b), p->F(b.n2), C, p->F(b.mu2),
                p->F(b.rs2), T, st));
  PLAN_CK(pack_lin(p, b.l1));
  PLAN_HIPCK(linear_fwd_gelu(p->F(b.n2), C, C, p->F(b.l1.pk), p->P(b.l1.b), p->F(b.hpre), p->F(b.hact),
                         M, T, st));
  PLAN_CK(pack_lin(p, b.l2));
  PLAN_HIPCK(linear_fwd(p->F(b.hact), M, M, p->F(b.l2.pk), p->P(b.l2.b), p->F(b.x2), C, C, T,
                    p->F(b.x1), C, st));
  return SPFF_OK;
}

// A = d x2 [T][C] (overwritten) -> dtin (written)
int block_bwd(spff_unetr* p, Blk& b, const float* tin, float* A, float* dtin) {
  const int64_t T = (int64_t)p->cfg.batch * p->n;
  const int C = p->hid, M = p->mlp;
  hipStream_t st = p->st;
  float* wg = p->F(p->wg_ws);
  float* Bf = p->F(p->S_b);
  float* Cf = p->F(p->S_c);
  float* dh = p->F(p->S_h);
  float* dq = p->F(p->S_qkv);
  // MLP: x2 = x1 + L2(gelu(L1(LN2(x1))))
  PLAN_HIPCK(linear_wgrad(p->F(b.hact), M, M, A, C, C, p->DP(b.l2.w), p->DP(b.l2.b), T, wg, st));
  PLAN_HIPCK(linear_dgrad(A, C, C, wd_of(p, b.l2), dh, M, M, T, p->F(b.hpre), st));
  PLAN_HIPCK(linear_wgrad(p->F(b.n2), C, C, dh, M, M, p->DP(b.l1.w), p->DP(b.l1.b), T, wg, st));
  PLAN_HIPCK(linear_dgrad(dh, M, M, wd_of(p, b.l1), Bf, C, C, T, nullptr, st));  // Bf = d n2
  // d x1 = d x2 + LN2'(d n2)  (into Cf)
  PLAN_HIPCK(ln_bwd(p->F(b.x1), C, C, p->P(b.n2w), p->F(b.mu2), p->F(b.rs2), Bf, C, Cf, C, A, C,
                p->DP(b.n2w), wg, T, st));
  // attention: x1 = t + OutProj(O)
  PLAN_HIPCK(linear_wgrad(p->F(b.O), C, C, Cf, C, C, p->DP(b.proj.w), p->DP(b.proj.b), T, wg, st));
  PLAN_HIPCK(linear_dgrad(Cf, C, C, wd_of(p, b.proj), A, C, C, T, nullptr, st));  // A = dO
  PLAN_HIPCK(vit_attn_bwd(p->F(b.qkvb), p->F(b.O), A, p->F(b.lse), p->geo, dq, wg, st));
  PLAN_HIPCK(linear_dgrad(dq, 3 * C, 3 * C, wd_of(p, b.qkv), Bf, C, C, T, nullptr, st));  // d n1
  PLAN_HIPCK(linear_wgrad(p->F(b.n1), C, C, dq, 3 * C, 3 * C, p->DP(b.qkv.w), p->F(p->dummy), T, wg,
                      st));
  // d t = d x1 + LN1'(d n1)
  PLAN_HIPCK(ln_bwd(tin, C, C, p->P(b.n1w), p->F(b.mu1), p->F(b.rs1), Bf, C, dtin, C, Cf, C,
                p->DP(b.n1w), wg, T, st));
  return SPFF_OK;
}

const float* block_in(spff_unetr* p, int i) { return i ? p->F(p->blk[i - 1].x2) : p->F(p->tok); }

int forward(spff_unetr* p, const float* x, float* logits) {
  const spff_unetr_cfg& c = p->cfg;
  const int f = p->f, Hd = p->hid, n = p->n, B = c.batch;
  const Vol& v0 = p->vol[0];
  const int64_t T = (int64_t)B * n;
  hipStream_t st = p->st;
  PLAN_HIPCK(spff::fill32_async(p->F(p->ones), (size_t)p->maxC * 4, 0x3f800000u, st));
  PLAN_HIPCK(spff::zero_async(p->F(p->zeros), fbytes(p->maxC), st));
  if (p->resample) {
    CProf pr(PROF_RESAMPLE, 0.0, st);
    PLAN_HIPCK(resize3d_ncdhw_in(x, p->F(p->x_cl), p->ldx, B, c.in_ch, c.depth, c.height, c.width,
                             v0.D, v0.H, v0.W, st));
  } else {
    PLAN_HIPCK(ncdhw_to_ndhwc(x, p->F(p->x_cl), v0, c.in_ch, p->ldx, st));
  }
  CProf pv(PROF_VIT, 0.0, st);
  // patch embedding: rows of 16^3 patches through the Linear GEMM, + bias + position
  const int pk = p->pe.K;
  PLAN_HIPCK(patchify16(p->F(p->x_cl), p->ldx, c.in_ch, B, v0.D, v0.H, v0.W, p->F(p->rows), st));
  PLAN_CK(pack_lin(p, p->pe));
  for (int b = 0; b < B; ++b)
    PLAN_HIPCK(linear_fwd(p->F(p->rows) + (int64_t)b * n * pk, pk, pk, p->F(p->pe.pk), p->P(p->pe.b),
                      p->F(p->tok) + (int64_t)b * n * Hd, Hd, Hd, n, p->P(p->pos), Hd, st));
  for (int i = 0; i < NBLK; ++i) PLAN_CK(block_fwd(p, p->blk[i], block_in(p, i)));
  PLAN_HIPCK(ln_fwd(p->F(p->blk[NBLK - 1].x2), Hd, Hd, p->P(p->nfw), p->P(p->nfb), p->F(p->hN), Hd,
                p->F(p->nmu), p->F(p->nrs), T, st));
  pv.end();
  PLAN_CK(prep_convs(p, p->rb, NRB));
  RB* R = p->rb;
  UpConv* U = p->up;
  PLAN_CK(rb_fwd(p, R[0], src1(p->F(p->x_cl), p->ldx), nullptr));
  // encoder2: hs[3] -> T -> (T, RB) -> (T, RB)
  PLAN_CK(up_fwd(p, U[0], p->F(p->blk[3].x2)));
  PLAN_CK(up_fwd(p, U[1], p->F(U[0].out)));
  PLAN_CK(rb_fwd(p, R[1], src1(p->F(U[1].out), 2 * f), p->F(U[1].out)));
  PLAN_CK(up_fwd(p, U[2], p->F(R[1].out)));
  PLAN_CK(rb_fwd(p, R[2], src1(p->F(U[2].out), 2 * f), p->F(U[2].out)));
  // encoder3: hs[6] -> T -> (T, RB)
  PLAN_CK(up_fwd(p, U[3], p->F(p->blk[6].x2)));
  PLAN_CK(up_fwd(p, U[4], p->F(U[3].out)));
  PLAN_CK(rb_fwd(p, R[3], src1(p->F(U[4].out), 4 * f), p->F(U[4].out)));
  // encoder4: hs[9] -> T
  PLAN_CK(up_fwd(p, U[5], p->F(p->blk[9].x2)));
  const float* prev = p->F(p->hN);
  const float* skip[4] = {p->F(U[5].out), p->F(R[3].out), p->F(R[2].out), p->F(R[0].out)};
  for (int u = 0; u < 4; ++u) {
    UpConv& X = U[6 + u];
    PLAN_CK(up_fwd(p, X, prev));
    RB& r = R[4 + u];
    PLAN_CK(rb_fwd(p, r, Src2{p->F(X.out), skip[u], X.Cout, X.Cout, X.Cout}, nullptr));
    prev = p->F(r.out);
  }
  PLAN_CK(pack_lin(p, p->head));
  float* net = p->resample ? p->F(p->lg) : logits;
  PLAN_HIPCK(linear_fwd(prev, f, f, p->F(p->head.pk), p->P(p->head.b), net, p->K, p->K, nvox(v0),
                    nullptr, 0, st));
  if (p->resample) {
    CProf pr(PROF_RESAMPLE, 0.0, st);
    PLAN_HIPCK(resize3d_fwd(net, logits, B, p->K, v0.D, v0.H, v0.W, c.depth, c.height, c.width, st));
  }
  return SPFF_OK;
}

int backward(spff_unetr* p, const float* dl) {
  const spff_unetr_cfg& c = p->cfg;
  const int f = p->f, Hd = p->hid, n = p->n, B = c.batch;
  const Vol& v0 = p->vol[0];
  const int64_t T = (int64_t)B * n;
  hipStream_t st = p->st;
  RB* R = p->rb;
  UpConv* U = p->up;
  float* wg = p->F(p->wg_ws);
  float* Gout = p->F(p->G_out);
  float* dup = p->F(p->G_up);
  if (p->resample) {
    CProf pr(PROF_RESAMPLE, 0.0, st);
    PLAN_HIPCK(resize3d_bwd(dl, p->F(p->d_lg), B, p->K, v0.D, v0.H, v0.W, c.depth, c.height, c.width,
                        st));
    dl = p->F(p->d_lg);
  }
  PLAN_HIPCK(linear_wgrad(p->F(R[7].out), f, f, dl, p->K, p->K, p->DP(p->head.w), p->DP(p->head.b),
                      nvox(v0), wg, st));
  PLAN_HIPCK(linear_dgrad(dl, p->K, p->K, wd_of(p, p->head), Gout, f, f, nvox(v0), nullptr, st));
  // decoders: dec2 (R7) <- up <- dec3 (R6) <- up <- dec4 (R5) <- up <- dec5 (R4) <- up <- hN
  float* dskip[4] = {p->F(p->d_enc[3]), p->F(p->d_enc[2]), p->F(p->d_enc[1]), p->F(p->d_enc[0])};
  const float* skip[4] = {p->F(U[5].out), p->F(R[3].out), p->F(R[2].out), p->F(R[0].out)};
  for (int u = 3; u >= 0; --u) {
    UpConv& X = U[6 + u];
    RB& r = R[4 + u];
    Dst2 dx{dup, dskip[u], X.Cout, X.Cout, X.Cout};
    PLAN_CK(rb_bwd(p, r, Gout, Src2{p->F(X.out), skip[u], X.Cout, X.Cout, X.Cout}, nullptr, &dx));
    const float* xlow = u == 0 ? p->F(p->hN) : p->F(R[4 + u - 1].out);
    PLAN_CK(up_bwd(p, X, xlow, dup, u == 0 ? p->F(p->d_hN) : Gout));
  }
  // encoder4: d enc4 -> d hs[9]
  PLAN_CK(up_bwd(p, U[5], p->F(p->blk[9].x2), p->F(p->d_enc[3]), p->F(p->d_tap[2])));
  // encoder3: d enc3 -> RB -> T -> T -> d hs[6]
  {
    Dst2 dx = dst1(dup, 4 * f);
    PLAN_CK(rb_bwd(p, R[3], p->F(p->d_enc[2]), src1(p->F(U[4].out), 4 * f), p->F(U[4].out), &dx));
    PLAN_CK(up_bwd(p, U[4], p->F(U[3].out), dup, Gout));
    PLAN_CK(up_bwd(p, U[3], p->F(p->blk[6].x2), Gout, p->F(p->d_tap[1])));
  }
  // encoder2: d enc2 -> RB -> T -> RB -> T -> T -> d hs[3]
  {
    Dst2 dx = dst1(dup, 2 * f);
    PLAN_CK(rb_bwd(p, R[2], p->F(p->d_enc[1]), src1(p->F(U[2].out), 2 * f), p->F(U[2].out), &dx));
    PLAN_CK(up_bwd(p, U[2], p->F(R[1].out), dup, Gout));
    PLAN_CK(rb_bwd(p, R[1], Gout, src1(p->F(U[1].out), 2 * f), p->F(U[1].out), &dx));
    PLAN_CK(up_bwd(p, U[1], p->F(U[0].out), dup, Gout));
    PLAN_CK(up_bwd(p, U[0], p->F(p->blk[3].x2), Gout, p->F(p->d_tap[0])));
  }
  PLAN_CK(rb_bwd(p, R[0], p->F(p->d_enc[0]), src1(p->F(p->x_cl), p->ldx), nullptr, nullptr));
  // ViT: A = gradient of the residual stream; the taps join at blocks 9, 6, 3
  float* A = p->F(p->S_a);
  CProf pv(PROF_VIT, 0.0, st);
  PLAN_HIPCK(ln_bwd(p->F(p->blk[NBLK - 1].x2), Hd, Hd, p->P(p->nfw), p->F(p->nmu), p->F(p->nrs),
                p->F(p->d_hN), Hd, A, Hd, nullptr, 0, p->DP(p->nfw), wg, T, st));
  float* dtin = p->F(p->d_hN);  // free from here on
  for (int i = NBLK - 1; i >= 0; --i) {
    if (i == 9) PLAN_HIPCK(accumulate(A, p->F(p->d_tap[2]), T * Hd, 1.f, st));
    if (i == 6) PLAN_HIPCK(accumulate(A, p->F(p->d_tap[1]), T * Hd, 1.f, st));
    if (i == 3) PLAN_HIPCK(accumulate(A, p->F(p->d_tap[0]), T * Hd, 1.f, st));
    PLAN_CK(block_bwd(p, p->blk[i], block_in(p, i), A, dtin));
    std::swap(A, dtin);
  }
  // A = d tok: patch-embedding weight / bias, and the position embedding summed over the
  // batch in sample order
  PLAN_HIPCK(linear_wgrad(p->F(p->rows), p->pe.K, p->pe.K, A, Hd, Hd, p->DP(p->pe.w), p->DP(p->pe.b),
                      T, wg, st));
  PLAN_HIPCK(col_reduce(A, B, (int64_t)n * Hd, n * Hd, p->DP(p->pos), 0, st));
  return SPFF_OK;
}

}  // namespace

// =================================================================== C ABI ==
extern "C" {

int spff_unetr_create(const spff_unetr_cfg* cfg, spff_unetr** out) {
  return plan_create(cfg, out, build);
}

void spff_unetr_destroy(spff_unetr* p) { delete p; }

int spff_unetr_num_params(const spff_unetr* p) { return p ? (int)p->params.size() : 0; }

int spff_unetr_param_info(const spff_unetr* p, int i, const char** name, int* ndim,
                          int64_t shape[5], int64_t* offset, int64_t* numel) {
  if (!p) return plan_fail(SPFF_EINVAL, "param index");
  return plan_param_info(p->params, i, name, ndim, shape, offset, numel);
}

int64_t spff_unetr_param_floats(const spff_unetr* p) { return p ? p->nparam : 0; }
size_t spff_unetr_workspace_bytes(const spff_unetr* p) { return p ? p->total : 0; }

int spff_unetr_forward(spff_unetr* p, const float* x, const float* params, float* logits,
                       void* ws, void* stream) {
  if (!p || !x || !params || !logits || !ws) return plan_fail(SPFF_EINVAL, "null argument");
  p->bind(ws, params, nullptr, stream);
  return forward(p, x, logits);
}

int spff_unetr_backward(spff_unetr* p, const float* dlogits, const float* params, float* dparams,
                        void* ws, void* stream) {
  if (!p || !dlogits || !params || !dparams || !ws) return plan_fail(SPFF_EINVAL, "null argument");
  p->bind(ws, params, dparams, stream);
  return backward(p, dlogits);
}

int spff_unetr_saved_tensor(const spff_unetr* p, void* ws, const char* name, const float** ptr,
                            int64_t* nv, int* ch) {
  if (!p || !ws || !name || !ptr) return plan_fail(SPFF_EINVAL, "null argument");
  const std::string s(name);
  const SavedOut ret{ws, ptr, nv, ch};
  const int64_t T = (int64_t)p->cfg.batch * p->n;
  if (s == "tok") return ret(p->tok, T, p->hid);
  if (s == "h3") return ret(p->blk[3].x2, T, p->hid);
  if (s == "h6") return ret(p->blk[6].x2, T, p->hid);
  if (s == "h9") return ret(p->blk[9].x2, T, p->hid);
  if (s == "hN") return ret(p->hN, T, p->hid);
  const RB* R = p->rb;
  const UpConv* U = p->up;
  auto rbout = [&](const RB& r) { return ret(r.out, nvox(p->vol[r.L]), r.C); };
  if (s == "enc1") return rbout(R[0]);
  if (s == "enc2") return rbout(R[2]);
  if (s == "enc3") return rbout(R[3]);
  if (s == "enc4") return ret(U[5].out, nvox(p->vol[3]), U[5].Cout);
  if (s == "dec5") return rbout(R[4]);
  if (s == "dec4") return rbout(R[5]);
  if (s == "dec3") return rbout(R[6]);
  if (s == "dec2") return rbout(R[7]);
  for (int i = 0; i < NBLK; ++i) {
    const Blk& b = p->blk[i];
    const std::string pre = "block" + std::to_string(i) + ".";
    if (s == pre + "qkv") return ret(b.qkvb, T, 3 * p->hid);
    if (s == pre + "O") return ret(b.O, T, p->hid);
    if (s == pre + "x1") return ret(b.x1, T, p->hid);
    if (s == pre + "out") return ret(b.x2, T, p->hid);
  }
  for (int i = 0; i < NRB; ++i) {
    const RB& r = R[i];
    const int64_t V = nvox(p->vol[r.L]);
    if (s == r.name + ".y1") return ret(r.y1, V, r.C);
    if (s == r.name + ".a1") return ret(r.a1, V, r.C);
    if (s == r.name + ".y2") return ret(r.y2, V, r.C);
    if (r.has3 && s == r.name + ".y3") return ret(r.y3, V, r.C);
    if (s == r.name + ".out") return rbout(r);
  }
  return plan_fail(SPFF_EINVAL, "unknown saved tensor " + s);
}

}  // extern "C"
