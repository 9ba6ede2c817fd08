// Host-side sanitizer driver for the C ABI ("an ASan/UBSan CPU build of
// the C ABI").  Built by scripts/asan_build.sh with the host half of every HIP
// translation unit under -fsanitize=address,undefined; runs with no GPU and makes no
// device call: it creates and destroys a plan for every BASELINE.json configuration
// (and the sharded / ragged / ablation variants) and for each of the five variant plans
// (3DUNet, SwinUNETR, UNETR, R2UNet3D, ResUNet++), walks the flat parameter layout, asks
// for an index past the end and a negative one, sizes every workspace, resolves every
// saved-tensor family (and an unknown name) against a dummy workspace pointer, and checks
// that malformed configurations are rejected with an error.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "spff.h"

static int g_fail = 0;
#define EXPECT(c, ...)                              \
  do {                                              \
    if (!(c)) {                                     \
      std::fprintf(stderr, "FAIL %s:%d ", __FILE__, __LINE__); \
      std::fprintf(stderr, __VA_ARGS__);            \
      std::fprintf(stderr, "\n");                   \
      ++g_fail;                                     \
    }                                               \
  } while (0)

static spff_cfg cfg_of(int B, int Cin, int D, int H, int W, int K, int base = 32, int world = 1,
                       int rank = 0, int axis = 0, int mem = SPFF_MEM_AUTO, int math = SPFF_MATH_BF16X6,
                       int efilm = 1, int fgate = 1, int se = 1, int specse = 1) {
  spff_cfg c;
  std::memset(&c, 0, sizeof c);
  c.batch = B; c.in_ch = Cin; c.depth = D; c.height = H; c.width = W;
  c.num_classes = K; c.base = base; c.ksd = 3;
  c.use_efilm = efilm; c.use_fgate = fgate; c.use_se = se; c.use_specse = specse;
  c.math = math; c.shard_world = world; c.shard_rank = rank; c.shard_axis = axis;
  c.memory_mode = mem;
  return c;
}

static const char* kSaved[] = {
    "x_cl", "grad.out", "grad.dy2", "grad.da1", "grad.dx", "enc1.y1", "enc1.y2", "enc1.out",
    "enc1.a1", "enc1.al1", "enc1.de1", "enc1.al2", "enc1.de2", "enc2.y1", "enc3.y2", "bott.y1",
    "bott.out", "dec3.y1", "dec3.out", "dec2.y2", "dec1.y1", "dec1.out", "pool1", "pool2",
    "pool3", "up3", "up2", "up1", "no.such.tensor"};

static void plan_case(const char* tag, const spff_cfg& c) {
  spff_plan* p = nullptr;
  const int rc = spff_plan_create(&c, &p);
  EXPECT(rc == SPFF_OK && p, "%s: spff_plan_create rc %d (%s)", tag, rc, spff_last_error());
  if (!p) return;
  const int n = spff_num_params(p);
  EXPECT(n > 0, "%s: %d params", tag, n);
  int64_t end = 0;
  for (int i = 0; i < n; ++i) {
    const char* name = nullptr;
    int nd = 0;
    int64_t shape[5] = {0, 0, 0, 0, 0}, off = -1, numel = -1;
    EXPECT(spff_param_info(p, i, &name, &nd, shape, &off, &numel) == SPFF_OK, "%s: param %d", tag, i);
    int64_t prod = 1;
    for (int k = 0; k < nd; ++k) prod *= shape[k];
    EXPECT(name && std::strlen(name) > 0 && nd >= 1 && nd <= 5 && prod == numel && off == end,
           "%s: param %d %s layout", tag, i, name ? name : "?");
    end = off + numel;
  }
  EXPECT(end == spff_param_floats(p), "%s: flat size", tag);
  const char* nm = nullptr;
  int nd = 0;
  int64_t sh[5], off, numel;
  EXPECT(spff_param_info(p, n, &nm, &nd, sh, &off, &numel) != SPFF_OK, "%s: index past end", tag);
  EXPECT(spff_param_info(p, -1, &nm, &nd, sh, &off, &numel) != SPFF_OK, "%s: negative index", tag);
  const size_t ws = spff_workspace_bytes(p);
  EXPECT(ws > 0, "%s: workspace", tag);
  // saved-tensor lookups are pointer arithmetic on the workspace (never dereferenced)
  static char dummy[16];
  for (const char* s : kSaved) {
    const float* ptr = nullptr;
    int64_t nv = 0;
    int ch = 0;
    if (spff_saved_tensor(p, dummy, s, &ptr, &nv, &ch) == SPFF_OK) {
      const size_t o = (size_t)((const char*)ptr - dummy);
      EXPECT(o + (size_t)nv * ch * 4 <= ws, "%s: saved %s [%zu + %lld] outside the workspace",
             tag, s, o, (long long)nv * ch * 4);
    }
  }
  EXPECT(spff_saved_tensor(p, dummy, "no.such.tensor", nullptr, nullptr, nullptr) != SPFF_OK,
         "%s: unknown saved name", tag);
  std::printf("  %-44s params %3d  floats %9lld  workspace %8.2f GiB\n", tag, n,
              (long long)spff_param_floats(p), ws / 1073741824.0);
  spff_plan_destroy(p);
}

static void reject(const char* tag, const spff_cfg& c) {
  spff_plan* p = nullptr;
  const int rc = spff_plan_create(&c, &p);
  EXPECT(rc != SPFF_OK && !p, "%s: malformed config accepted", tag);
  if (p) spff_plan_destroy(p);
}

// The five variant plans export the same nine entry points under their own prefix.
template <class P, class Cfg>
struct Abi {
  const char* what;
  int (*create)(const Cfg*, P**);
  void (*destroy)(P*);
  int (*num_params)(const P*);
  int (*param_info)(const P*, int, const char**, int*, int64_t*, int64_t*, int64_t*);
  int64_t (*param_floats)(const P*);
  size_t (*workspace_bytes)(const P*);
  int (*saved)(const P*, void*, const char*, const float**, int64_t*, int*);
};
#define ABI(P) \
  Abi<P, P##_cfg> { #P, P##_create, P##_destroy, P##_num_params, P##_param_info, \
                    P##_param_floats, P##_workspace_bytes, P##_saved_tensor }

// create, parameter walk, both bad indices, workspace, every name of `saved` (all must
// resolve inside the workspace) plus an unknown one and a null result pointer, destroy;
// `more` sees the live plan (3DUNet: its buffer table)
template <class P, class Cfg, class More>
static void variant_case(const Abi<P, Cfg>& a, const char* tag, const Cfg& c,
                         const std::vector<std::string>& saved, More more) {
  P* p = nullptr;
  const int rc = a.create(&c, &p);
  EXPECT(rc == SPFF_OK && p, "%s %s: create rc %d (%s)", a.what, tag, rc, spff_last_error());
  if (!p) return;
  const int n = a.num_params(p);
  EXPECT(n > 0, "%s %s: %d params", a.what, tag, n);
  int64_t end = 0;
  for (int i = 0; i < n; ++i) {
    const char* name = nullptr;
    int nd = 0;
    int64_t shape[5] = {0, 0, 0, 0, 0}, off = -1, numel = -1;
    EXPECT(a.param_info(p, i, &name, &nd, shape, &off, &numel) == SPFF_OK, "%s %s: param %d",
           a.what, tag, i);
    int64_t prod = 1;
    for (int k = 0; k < nd; ++k) prod *= shape[k];
    EXPECT(name && std::strlen(name) > 0 && nd >= 1 && nd <= 5 && prod == numel && off == end,
           "%s %s: param %d %s layout", a.what, tag, i, name ? name : "?");
    end = off + numel;
  }
  EXPECT(end == a.param_floats(p), "%s %s: flat size", a.what, tag);
  const char* nm = nullptr;
  int nd = 0;
  int64_t sh[5], off, numel;
  EXPECT(a.param_info(p, n, &nm, &nd, sh, &off, &numel) != SPFF_OK, "%s %s: index past end",
         a.what, tag);
  EXPECT(a.param_info(p, -1, &nm, &nd, sh, &off, &numel) != SPFF_OK, "%s %s: negative index",
         a.what, tag);
  EXPECT(a.param_info(nullptr, 0, &nm, &nd, sh, &off, &numel) != SPFF_OK, "%s: null plan", a.what);
  const size_t ws = a.workspace_bytes(p);
  EXPECT(ws > 0, "%s %s: workspace", a.what, tag);
  static char dummy[16];
  const float* ptr = nullptr;
  int64_t nv = 0;
  int ch = 0;
  for (const std::string& s : saved) {
    const int r = a.saved(p, dummy, s.c_str(), &ptr, &nv, &ch);
    EXPECT(r == SPFF_OK, "%s %s: saved %s (%s)", a.what, tag, s.c_str(), spff_last_error());
    if (r != SPFF_OK) continue;
    const size_t o = (size_t)((const char*)ptr - dummy);
    EXPECT(nv > 0 && ch > 0 && o + (size_t)nv * ch * 4 <= ws,
           "%s %s: saved %s [%zu + %lld] outside the workspace", a.what, tag, s.c_str(), o,
           (long long)nv * ch * 4);
  }
  EXPECT(a.saved(p, dummy, "no.such.tensor", &ptr, &nv, &ch) != SPFF_OK, "%s %s: unknown saved name",
         a.what, tag);
  EXPECT(a.saved(p, dummy, saved.empty() ? "x" : saved[0].c_str(), nullptr, &nv, &ch) != SPFF_OK,
         "%s %s: null result pointer", a.what, tag);
  more(p);
  std::printf("  %-44s params %3d  floats %9lld  workspace %8.2f GiB\n", tag, n,
              (long long)a.param_floats(p), ws / 1073741824.0);
  a.destroy(p);
}
template <class P, class Cfg>
static void variant_case(const Abi<P, Cfg>& a, const char* tag, const Cfg& c,
                         const std::vector<std::string>& saved) {
  variant_case(a, tag, c, saved, [](P*) {});
}

template <class P, class Cfg>
static void variant_reject(const Abi<P, Cfg>& a, const char* tag, const Cfg& c) {
  P* p = nullptr;
  const int rc = a.create(&c, &p);
  EXPECT(rc != SPFF_OK && !p, "%s %s: malformed config accepted", a.what, tag);
  if (p) a.destroy(p);
  EXPECT(a.create(nullptr, &p) != SPFF_OK && a.create(&c, nullptr) != SPFF_OK, "%s: null argument",
         a.what);
}

// names x suffixes, e.g. {"e1", "e2"} x {".x1", ".out"}
static std::vector<std::string> cross(std::initializer_list<const char*> names,
                                      std::initializer_list<const char*> suffixes) {
  std::vector<std::string> out;
  for (const char* n : names)
    for (const char* s : suffixes) out.push_back(std::string(n) + s);
  return out;
}
static std::vector<std::string> operator+(std::vector<std::string> a,
                                          const std::vector<std::string>& b) {
  a.insert(a.end(), b.begin(), b.end());
  return a;
}

int main() {
  std::printf("SPFF plans (BASELINE.json configs and variants):\n");
  plan_case("config1 registry 1x1x5x64x64 K9", cfg_of(1, 1, 5, 64, 64, 9));
  plan_case("config2 headline 2x5x128^3 K13", cfg_of(2, 5, 128, 128, 128, 13));
  plan_case("config2 f32", cfg_of(2, 5, 128, 128, 128, 13, 32, 1, 0, 0, SPFF_MEM_AUTO, SPFF_MATH_F32));
  plan_case("config2 lean", cfg_of(2, 5, 128, 128, 128, 13, 32, 1, 0, 0, SPFF_MEM_LEAN));
  plan_case("config4 whole 1x5x512^3 (lean)", cfg_of(1, 5, 512, 512, 512, 13));
  for (int r : {0, 3, 7})
    plan_case(("config4 depth-shard 8 rank " + std::to_string(r)).c_str(),
              cfg_of(1, 5, 64, 512, 512, 13, 32, 8, r, SPFF_SHARD_DEPTH));
  for (int r : {0, 1})
    plan_case(("registry height-shard 2 rank " + std::to_string(r)).c_str(),
              cfg_of(1, 1, 5, 256, 512, 13, 32, 2, r, SPFF_SHARD_HEIGHT));
  plan_case("ragged 1x5x4x18x20 (trilinear _cat)", cfg_of(1, 5, 4, 18, 20, 9, 8));
  plan_case("ablation no efilm/fgate", cfg_of(1, 5, 8, 32, 32, 9, 8, 1, 0, 0, 0, 1, 0, 0, 1, 1));
  plan_case("ablation no se/specse", cfg_of(1, 5, 8, 32, 32, 9, 8, 1, 0, 0, 0, 1, 1, 1, 0, 0));
  reject("H < 8", cfg_of(1, 1, 5, 4, 64, 13));
  plan_case("K 40 base 24 (fx5)", cfg_of(1, 5, 6, 24, 24, 40, 24));
  {
    spff_cfg g = cfg_of(1, 5, 8, 16, 16, 9, 8);
    g.efilm_hidden = 24;
    g.efilm_pe_dims = 11;
    g.fgate_learn_phase = 1;
    plan_case("gates hidden 24 pe_dims 11 learn_phase (fx6)", g);
    g.efilm_hidden = 65;
    reject("efilm hidden 65", g);
    g.efilm_hidden = 24;
    g.efilm_pe_dims = 1;
    reject("efilm pe_dims 1", g);
  }
  reject("K > SPFF_MAX_CLASSES", cfg_of(1, 1, 5, 64, 64, SPFF_MAX_CLASSES + 1));
  reject("base 20", cfg_of(1, 1, 5, 64, 64, 13, 20));
  reject("depth shard batch 2", cfg_of(2, 1, 8, 64, 64, 13, 32, 2, 0, SPFF_SHARD_DEPTH));
  reject("height shard 60 rows", cfg_of(1, 1, 5, 60, 512, 13, 32, 2, 0, SPFF_SHARD_HEIGHT));
  reject("bad shard axis", cfg_of(1, 1, 5, 64, 512, 13, 32, 2, 0, 2));
  reject("rank >= world", cfg_of(1, 5, 64, 64, 64, 13, 32, 2, 2, SPFF_SHARD_DEPTH));
  EXPECT(spff_plan_create(nullptr, nullptr) != SPFF_OK, "null cfg");
  spff_plan_destroy(nullptr);
  EXPECT(spff_loss_ws_bytes(2LL * 128 * 128 * 128, 13) > 0, "loss ws");
  EXPECT(spff_conv3d_ws_bytes(2, 128, 128, 128, 32, 32, 3) >= 0, "conv ws");

  std::printf("3DUNet (BASELINE configs[2]):\n");
  {
    const auto A = ABI(spff_unet3d);
    spff_unet3d_cfg c;
    std::memset(&c, 0, sizeof c);
    c.batch = 4; c.in_ch = 1; c.depth = 5; c.height = 96; c.width = 96;
    c.target_depth = 16; c.num_classes = 13; c.base = 32; c.math = SPFF_MATH_BF16X6;
    const auto saved = cross({"enc1", "enc4", "bott", "dec4", "dec1"}, {".y1", ".a1", ".y2", ".out"}) +
                       cross({"x_cl", "pool1", "pool4", "up4", "up1"}, {""});
    variant_case(A, "4x1x5x96^2 -> 16", c, saved, [](spff_unet3d* u) {
      int64_t bend = 0;
      const int nb = spff_unet3d_num_buffers(u);
      for (int i = 0; i < nb; ++i) {
        const char* name; int64_t off, numel;
        EXPECT(spff_unet3d_buffer_info(u, i, &name, &off, &numel) == SPFF_OK && off == bend,
               "unet3d buffer %d", i);
        bend = off + numel;
      }
      EXPECT(bend == spff_unet3d_buffer_floats(u), "unet3d buffer size");
      const char* name; int64_t off, numel;
      EXPECT(spff_unet3d_buffer_info(u, nb, &name, &off, &numel) != SPFF_OK &&
             spff_unet3d_buffer_info(u, -1, &name, &off, &numel) != SPFF_OK, "unet3d buffer index");
    });
    c.math = SPFF_MATH_F32;
    variant_case(A, "4x1x5x96^2 -> 16 f32", c, saved);
    c.height = 90;  // not a multiple of 16
    variant_reject(A, "H 90", c);
    c.height = 96; c.base = 12;
    variant_reject(A, "base 12", c);
  }

  std::printf("SwinUNETR (BASELINE configs[4]):\n");
  {
    const auto A = ABI(spff_swin);
    spff_swin_cfg c;
    std::memset(&c, 0, sizeof c);
    c.batch = 2; c.in_ch = 1; c.depth = 128; c.height = 128; c.width = 128;
    c.num_classes = 13; c.feature_size = 12; c.window = 7;
    c.heads[0] = 1; c.heads[1] = 2; c.heads[2] = 4; c.heads[3] = 8;
    c.mlp_ratio = 2.0f; c.math = SPFF_MATH_BF16X6;
    const auto saved =
        cross({"t0", "t4", "hs0", "hs4", "grad.t0", "grad.t4", "up5", "up1"}, {""}) +
        cross({"stage0", "stage3"}, {".n1", ".qkv", ".O", ".x1", ".hpre", ".x2", ".mn"}) +
        cross({"encoder1.layer", "decoder5.conv_block", "decoder1.conv_block"},
              {".y1", ".a1", ".y2", ".y3", ".out", ".al1", ".de1", ".al2", ".de2", ".al3", ".de3"}) +
        cross({"encoder2.layer", "encoder10.layer"}, {".y1", ".a1", ".y2", ".out", ".al2", ".de2"});
    variant_case(A, "2x1x128^3", c, saved);
    c.batch = 1; c.depth = 32; c.height = 32; c.width = 64; c.feature_size = 4;
    c.math = SPFF_MATH_F32;
    variant_case(A, "1x1x32x32x64 feature 4 f32", c, saved);
    c.depth = 48;
    variant_reject(A, "D 48", c);
    c.depth = 32; c.width = 32;
    variant_reject(A, "one bottleneck voxel", c);
    c.width = 64; c.window = 8;
    variant_reject(A, "window 8", c);
    EXPECT(spff_swin_loss_ws_bytes(2, 13) > 0, "swin loss ws");
  }

  std::printf("UNETR:\n");
  {
    const auto A = ABI(spff_unetr);
    spff_unetr_cfg c;
    std::memset(&c, 0, sizeof c);
    c.batch = 1; c.in_ch = 1; c.depth = 32; c.height = 32; c.width = 32;
    c.img[0] = c.img[1] = c.img[2] = 32;
    c.num_classes = 4; c.feature_size = 8; c.hidden = 128; c.mlp_dim = 256; c.heads = 2;
    c.math = SPFF_MATH_F16X3;
    const auto saved =
        cross({"tok", "h3", "h6", "h9", "hN", "enc1", "enc2", "enc3", "enc4", "dec5", "dec4", "dec3",
               "dec2"}, {""}) +
        cross({"block0", "block11"}, {".qkv", ".O", ".x1", ".out"}) +
        cross({"encoder1.layer", "decoder5.conv_block", "decoder2.conv_block"},
              {".y1", ".a1", ".y2", ".y3", ".out"}) +
        cross({"encoder2.blocks.0.1", "encoder2.blocks.1.1", "encoder3.blocks.0.1"},
              {".y1", ".a1", ".y2", ".out"});
    variant_case(A, "1x1x32^3 hidden 128", c, saved);
    c.depth = 48; c.height = 48; c.width = 64;  // resampled to img and back
    c.math = SPFF_MATH_F32;
    variant_case(A, "1x1x48x48x64 -> 32^3 f32", c, saved);
    c.depth = c.height = c.width = 32;
    {
      spff_unetr_cfg b = c;
      b.img[0] = 40;
      variant_reject(A, "img 40", b);
      b = c; b.hidden = 130; b.heads = 4;
      variant_reject(A, "hidden 130 heads 4", b);
      b = c; b.hidden = 256;
      variant_reject(A, "head width 128", b);
      b = c; b.hidden = 96; b.heads = 4;
      variant_reject(A, "head width 24", b);
      b = c; b.img[0] = b.img[1] = 128; b.img[2] = 160;
      variant_reject(A, "640 tokens", b);
      b = c; b.depth = 40;
      variant_reject(A, "D 40", b);
      b = c; b.in_ch = 2;
      variant_reject(A, "in_ch 2", b);
    }
  }

  std::printf("R2UNet3D:\n");
  {
    const auto A = ABI(spff_r2u);
    spff_r2u_cfg c;
    std::memset(&c, 0, sizeof c);
    c.batch = 1; c.in_ch = 1; c.depth = 16; c.height = 32; c.width = 32;
    c.num_classes = 13; c.base = 16; c.t = 2; c.math = SPFF_MATH_F16X3;
    const auto blocks = {"e1", "e2", "e3", "e4", "b", "d4", "d3", "d2", "d1"};
    variant_case(A, "1x1x16x32x32 base 16 t 2", c, cross(blocks, {".x1", ".out", ".ru1", ".ru2"}));
    {
      spff_r2u_cfg w = c;
      w.in_ch = 8; w.num_classes = 32; w.base = 24; w.t = 3; w.math = SPFF_MATH_F32;
      variant_case(A, "1x8x16x32x32 base 24 t 3 f32", w,
                   cross(blocks, {".x1", ".out", ".ru1", ".ru2", ".ru3"}));
      EXPECT([&] {  // a recurrence step past t is not a saved tensor
        spff_r2u* p = nullptr;
        if (spff_r2u_create(&c, &p) != SPFF_OK) return false;
        static char dummy[16];
        const float* ptr;
        const int r = spff_r2u_saved_tensor(p, dummy, "e1.ru3", &ptr, nullptr, nullptr);
        spff_r2u_destroy(p);
        return r != SPFF_OK;
      }(), "r2u: e1.ru3 resolved at t 2");
    }
    const struct { const char* tag; int spff_r2u_cfg::*field; int value; } bad[] = {
        {"H 24", &spff_r2u_cfg::height, 24},   {"base 12", &spff_r2u_cfg::base, 12},
        {"t 0", &spff_r2u_cfg::t, 0},          {"t 9", &spff_r2u_cfg::t, 9},
        {"K 1", &spff_r2u_cfg::num_classes, 1}, {"K 33", &spff_r2u_cfg::num_classes, 33},
        {"in_ch 9", &spff_r2u_cfg::in_ch, 9},  {"D 5", &spff_r2u_cfg::depth, 5},
        {"math 7", &spff_r2u_cfg::math, 7}};
    for (const auto& b : bad) {
      spff_r2u_cfg x = c;
      x.*b.field = b.value;
      variant_reject(A, b.tag, x);
    }
    EXPECT(spff_r2u_dice_loss_ws_bytes(2, 13) > 0, "r2u loss ws");
  }

  std::printf("ResUNet++:\n");
  {
    const auto A = ABI(spff_rupp);
    spff_rupp_cfg c;
    std::memset(&c, 0, sizeof c);
    c.batch = 1; c.in_ch = 1; c.depth = 16; c.height = 32; c.width = 32;
    c.num_classes = 13; c.base = 16; c.math = SPFF_MATH_F16X3;
    const auto saved = cross({"e1", "e2", "e3", "e4", "b_aspp_in", "b_aspp_out", "d4", "d3", "d2", "d1"},
                             {".a1", ".out"}) +
                       cross({"b_aspp.out", "ag4.att", "ag3.att", "ag2.att"}, {""});
    variant_case(A, "1x1x16x32x32 base 16", c, saved);
    {
      spff_rupp_cfg w = c;
      w.in_ch = 8; w.num_classes = 32; w.base = 24; w.math = SPFF_MATH_F32;
      variant_case(A, "1x8x16x32x32 base 24 f32", w, saved);
      w = c; w.num_classes = 2; w.depth = 32; w.height = 16; w.width = 16;
      variant_case(A, "1x1x32x16x16 K 2", w, saved);
    }
    const struct { const char* tag; int spff_rupp_cfg::*field; int value; } bad[] = {
        {"D 24", &spff_rupp_cfg::depth, 24},   {"H 24", &spff_rupp_cfg::height, 24},
        {"W 24", &spff_rupp_cfg::width, 24},   {"base 12", &spff_rupp_cfg::base, 12},
        {"in_ch 0", &spff_rupp_cfg::in_ch, 0}, {"in_ch 9", &spff_rupp_cfg::in_ch, 9},
        {"K 1", &spff_rupp_cfg::num_classes, 1}, {"K 33", &spff_rupp_cfg::num_classes, 33}};
    for (const auto& b : bad) {
      spff_rupp_cfg x = c;
      x.*b.field = b.value;
      variant_reject(A, b.tag, x);
    }
    {
      spff_rupp_cfg x = c;
      x.height = x.width = 16;  // 16^3: one bottleneck voxel per sample
      variant_reject(A, "16^3", x);
    }
    EXPECT(spff_rupp_loss_ws_bytes(2, 13) > 0, "rupp loss ws");
  }
  std::printf(g_fail ? "asan_plans: %d FAILURES\n" : "asan_plans: ok\n", g_fail);
  return g_fail ? 1 : 0;
}
