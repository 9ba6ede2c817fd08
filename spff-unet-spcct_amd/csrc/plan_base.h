// The scaffolding every engine plan shares (engine.hip, unet3d.hip, swin.hip, unetr.hip,
// r2unet.hip, resunetpp.hip): the parameter table, the workspace bump allocator, the
// per-call bindings with their accessors, the error helper / macro pair and the bodies of
// the C ABI functions that do not depend on the plan's graph.  Host-only, no kernels.
// A plan derives from PlanBase, adds `cfg` and its own descriptors, and supplies build(),
// forward(), backward() and the names of its saved tensors (DESIGN "Plan scaffolding").
#pragma once
#include "spff_internal.h"
#include "spff.h"

#include <string>
#include <vector>

namespace spff {

// PLAN_HIPCK / PLAN_CK return the C ABI's error code from the enclosing function.
inline int plan_fail(int code, const std::string& m) { return set_error(code, m.c_str()); }
#define PLAN_HIPCK(expr)                                                                   \
  do {                                                                                     \
    hipError_t _e = (expr);                                                                \
    if (_e != hipSuccess)                                                                  \
      return plan_fail(SPFF_EHIP, std::string(#expr) + " -> " + hipGetErrorString(_e));    \
  } while (0)
#define PLAN_CK(expr)               \
  do {                              \
    int _r = (expr);                \
    if (_r != SPFF_OK) return _r;   \
  } while (0)

inline int rup(int a, int b) { return (a + b - 1) / b * b; }
inline size_t fbytes(int64_t n) { return (size_t)n * sizeof(float); }

struct ParamEnt {  // one flat-buffer entry: parameters, and unet3d.hip's buffers
  std::string name;
  std::vector<int64_t> shape;
  int64_t off, numel;
};

struct PlanBase {
  std::vector<ParamEnt> params;
  int64_t nparam = 0;  // floats of the flat parameter buffer
  size_t total = 0;    // workspace bytes
  // per call
  char* ws = nullptr;
  const float* prm = nullptr;
  float* dprm = nullptr;
  hipStream_t st = nullptr;

  float* F(size_t off) const { return reinterpret_cast<float*>(ws + off); }
  // an offset of -1 is "this plan has no such parameter": null, never prm - 1
  const float* P(int64_t off) const { return off < 0 ? nullptr : prm + off; }
  float* DP(int64_t off) const { return off < 0 ? nullptr : dprm + off; }
  size_t alloc(size_t bytes) {  // 256-byte bump
    size_t o = total;
    total += (bytes + 255) / 256 * 256;
    return o;
  }
  int64_t reg(const std::string& name, std::vector<int64_t> shape) {
    int64_t n = 1;
    for (auto s : shape) n *= s;
    params.push_back(ParamEnt{name, shape, nparam, n});
    nparam += n;
    return nparam - n;
  }
  void bind(void* ws_, const float* params_, float* dparams_, void* stream) {
    ws = static_cast<char*>(ws_);
    prm = params_;
    dprm = dparams_;
    st = static_cast<hipStream_t>(stream);
  }
};

// spff_*_param_info / spff_unet3d_buffer_info (which passes no ndim / shape)
inline int plan_param_info(const std::vector<ParamEnt>& tab, int i, const char** name, int* ndim,
                           int64_t shape[5], int64_t* offset, int64_t* numel,
                           const char* what = "param index") {
  if (i < 0 || i >= (int)tab.size()) return plan_fail(SPFF_EINVAL, what);
  const ParamEnt& e = tab[i];
  if (name) *name = e.name.c_str();
  if (ndim) *ndim = (int)e.shape.size();
  if (shape)
    for (int k = 0; k < 5; ++k) shape[k] = k < (int)e.shape.size() ? e.shape[k] : 1;
  if (offset) *offset = e.off;
  if (numel) *numel = e.numel;
  return SPFF_OK;
}

// spff_*_create: build(p) validates cfg, registers the parameters and sizes the workspace
template <class P, class Cfg, class Build>
int plan_create(const Cfg* cfg, P** out, Build build) {
  if (!cfg || !out) return plan_fail(SPFF_EINVAL, "null argument");
  P* p = new P();
  p->cfg = *cfg;
  const int r = build(p);
  if (r != SPFF_OK) {
    delete p;
    return r;
  }
  *out = p;
  return SPFF_OK;
}

// the (pointer, rows, channels) triple of spff_*_saved_tensor
struct SavedOut {
  const void* ws;
  const float** ptr;
  int64_t* nv;
  int* ch;
  int operator()(size_t off, int64_t rows, int c) const {
    *ptr = reinterpret_cast<const float*>(static_cast<const char*>(ws) + off);
    if (nv) *nv = rows;
    if (ch) *ch = c;
    return SPFF_OK;
  }
  int operator()(size_t off, const Vol& v, int c) const { return (*this)(off, nvox(v), c); }
};

}  // namespace spff
