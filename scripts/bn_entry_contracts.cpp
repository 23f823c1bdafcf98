// Argument contracts of the BatchNorm entry points, without a GPU: every call below is refused by a host check before any launch, and its return code is
// printed.  Run it on two builds of the library and compare the outputs (profiles/conv_units_refactor.txt):
//     g++ -std=c++17 -I include scripts/bn_entry_contracts.cpp -ldl -o /tmp/bn_contracts && /tmp/bn_contracts crnn-ocr-lite_amd/libcrnn_mi355x.so
// Pointers are made-up addresses (nothing dereferences them on the host).  Left out because they would reach a launch: every pattern on crnn_bn_bwd_ex and
// crnn_bn_act_pool_drop_ex (they check nothing), a null gamma / dgamma / dbeta / scratch anywhere, and a misaligned qmax on crnn_bn_act_pool_drop_qmax_ex
// (it selects the one-channel-per-thread kernel instead of refusing).
#include <dlfcn.h>
#include <stdint.h>
#include <stdio.h>
#include "crnn_mi355x.h"

#define SYM(name) decltype(&name) name##_p = (decltype(&name))dlsym(h, #name); if (!name##_p) { fprintf(stderr, "missing %s\n", #name); return 2; }
#define SHOW(what, call) printf("%-34s %-36s %d\n", fn, what, (int)(call))

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s path/to/libcrnn_mi355x.so\n", argv[0]); return 2; }
  void* h = dlopen(argv[1], RTLD_NOW);
  if (!h) { fprintf(stderr, "%s\n", dlerror()); return 2; }
  SYM(crnn_bn_bwd_apply_ex) SYM(crnn_bn_bwd_planes_ex) SYM(crnn_bn_bwd_apply_planes_ex) SYM(crnn_bn_bwd_qmax_ex) SYM(crnn_bn_act_pool_drop_qmax_ex)
  SYM(crnn_bn_bwd_finalize)
  float* const F = (float*)0x10000;            // 16-byte aligned stand-ins
  void* const X = (void*)0x20000; void* const G = (void*)0x30000; void* const DX = (void*)0x40000; void* const PL = (void*)0x50000;
  void* const Q = (void*)0x60000; void* const Y = (void*)0x70000;
  void* const PL_ODD = (void*)0x50004; void* const Q_ODD = (void*)0x60004;
  const int B = 2, H = 6, W = 8, C = 16; const long n = (long)B * H * W * C;
  const char* fn;

  fn = "crnn_bn_bwd_apply_ex";
  for (int dt = 0; dt < 2; ++dt) {
    SHOW(dt ? "null x (bf16)" : "null x", crnn_bn_bwd_apply_ex_p(0, G, F, F, DX, B, H, W, C, 1, 1, 0.f, 0, 0, dt, 0));
    SHOW(dt ? "null g (bf16)" : "null g", crnn_bn_bwd_apply_ex_p(X, 0, F, F, DX, B, H, W, C, 1, 1, 0.f, 0, 0, dt, 0));
    SHOW(dt ? "null bnstate (bf16)" : "null bnstate", crnn_bn_bwd_apply_ex_p(X, G, 0, F, DX, B, H, W, C, 1, 1, 0.f, 0, 0, dt, 0));
    SHOW(dt ? "null coef (bf16)" : "null coef", crnn_bn_bwd_apply_ex_p(X, G, F, 0, DX, B, H, W, C, 1, 1, 0.f, 0, 0, dt, 0));
    SHOW(dt ? "null dx (bf16)" : "null dx", crnn_bn_bwd_apply_ex_p(X, G, F, F, 0, B, H, W, C, 1, 1, 0.f, 0, 0, dt, 0));
  }

  fn = "crnn_bn_bwd_planes_ex";
  const float* const Xf = (const float*)X; const float* const Gf = (const float*)G;
  SHOW("null x", crnn_bn_bwd_planes_ex_p(0, Gf, F, F, PL, n, 2, F, F, F, F, B, H, W, C, 1, 1, 0.f, 0, 0, 0));
  SHOW("null g", crnn_bn_bwd_planes_ex_p(Xf, 0, F, F, PL, n, 2, F, F, F, F, B, H, W, C, 1, 1, 0.f, 0, 0, 0));
  SHOW("null bnstate", crnn_bn_bwd_planes_ex_p(Xf, Gf, 0, F, PL, n, 2, F, F, F, F, B, H, W, C, 1, 1, 0.f, 0, 0, 0));
  SHOW("null coef", crnn_bn_bwd_planes_ex_p(Xf, Gf, F, F, PL, n, 2, F, F, F, 0, B, H, W, C, 1, 1, 0.f, 0, 0, 0));
  SHOW("null dx_planes", crnn_bn_bwd_planes_ex_p(Xf, Gf, F, F, 0, n, 2, F, F, F, F, B, H, W, C, 1, 1, 0.f, 0, 0, 0));
  SHOW("planes = 1", crnn_bn_bwd_planes_ex_p(Xf, Gf, F, F, PL, n, 1, F, F, F, F, B, H, W, C, 1, 1, 0.f, 0, 0, 0));
  SHOW("planes = 4", crnn_bn_bwd_planes_ex_p(Xf, Gf, F, F, PL, n, 4, F, F, F, F, B, H, W, C, 1, 1, 0.f, 0, 0, 0));
  SHOW("misaligned dx_planes", crnn_bn_bwd_planes_ex_p(Xf, Gf, F, F, PL_ODD, n, 2, F, F, F, F, B, H, W, C, 1, 1, 0.f, 0, 0, 0));
  SHOW("plane_stride too small", crnn_bn_bwd_planes_ex_p(Xf, Gf, F, F, PL, n - 4, 3, F, F, F, F, B, H, W, C, 1, 1, 0.f, 0, 0, 0));
  SHOW("plane_stride % 4", crnn_bn_bwd_planes_ex_p(Xf, Gf, F, F, PL, n + 2, 3, F, F, F, F, B, H, W, C, 1, 1, 0.f, 0, 0, 0));
  SHOW("C % 4", crnn_bn_bwd_planes_ex_p(Xf, Gf, F, F, PL, n, 2, F, F, F, F, B, H, W, 3, 1, 1, 0.f, 0, 0, 0));
  SHOW("misaligned x", crnn_bn_bwd_planes_ex_p(Xf + 1, Gf, F, F, PL, n, 2, F, F, F, F, B, H, W, C, 1, 1, 0.f, 0, 0, 0));

  fn = "crnn_bn_bwd_apply_planes_ex";
  SHOW("null x", crnn_bn_bwd_apply_planes_ex_p(0, Gf, F, F, PL, n, 2, B, H, W, C, 1, 1, 0.f, 0, 0, 0));
  SHOW("null g", crnn_bn_bwd_apply_planes_ex_p(Xf, 0, F, F, PL, n, 2, B, H, W, C, 1, 1, 0.f, 0, 0, 0));
  SHOW("null bnstate", crnn_bn_bwd_apply_planes_ex_p(Xf, Gf, 0, F, PL, n, 2, B, H, W, C, 1, 1, 0.f, 0, 0, 0));
  SHOW("null coef", crnn_bn_bwd_apply_planes_ex_p(Xf, Gf, F, 0, PL, n, 2, B, H, W, C, 1, 1, 0.f, 0, 0, 0));
  SHOW("null dx_planes", crnn_bn_bwd_apply_planes_ex_p(Xf, Gf, F, F, 0, n, 2, B, H, W, C, 1, 1, 0.f, 0, 0, 0));
  SHOW("planes = 1", crnn_bn_bwd_apply_planes_ex_p(Xf, Gf, F, F, PL, n, 1, B, H, W, C, 1, 1, 0.f, 0, 0, 0));
  SHOW("misaligned dx_planes", crnn_bn_bwd_apply_planes_ex_p(Xf, Gf, F, F, PL_ODD, n, 3, B, H, W, C, 1, 1, 0.f, 0, 0, 0));
  SHOW("plane_stride too small", crnn_bn_bwd_apply_planes_ex_p(Xf, Gf, F, F, PL, n - 4, 2, B, H, W, C, 1, 1, 0.f, 0, 0, 0));
  SHOW("misaligned coef", crnn_bn_bwd_apply_planes_ex_p(Xf, Gf, F, F + 1, PL, n, 2, B, H, W, C, 1, 1, 0.f, 0, 0, 0));

  fn = "crnn_bn_bwd_qmax_ex";
  for (int dt = 0; dt < 2; ++dt) {
    SHOW(dt ? "null x (bf16)" : "null x", crnn_bn_bwd_qmax_ex_p(0, Q, G, F, F, DX, 0, 0, 0, F, F, F, F, B, H, W, C, 2, 2, 0.f, 0, 0, dt, 0));
    SHOW(dt ? "null g (bf16)" : "null g", crnn_bn_bwd_qmax_ex_p(X, Q, 0, F, F, DX, 0, 0, 0, F, F, F, F, B, H, W, C, 2, 2, 0.f, 0, 0, dt, 0));
    SHOW(dt ? "null bnstate (bf16)" : "null bnstate", crnn_bn_bwd_qmax_ex_p(X, Q, G, 0, F, DX, 0, 0, 0, F, F, F, F, B, H, W, C, 2, 2, 0.f, 0, 0, dt, 0));
    SHOW(dt ? "null coef (bf16)" : "null coef", crnn_bn_bwd_qmax_ex_p(X, Q, G, F, F, DX, 0, 0, 0, F, F, F, 0, B, H, W, C, 2, 2, 0.f, 0, 0, dt, 0));
    SHOW(dt ? "dx and dx_planes (bf16)" : "dx and dx_planes", crnn_bn_bwd_qmax_ex_p(X, Q, G, F, F, DX, PL, n, 2, F, F, F, F, B, H, W, C, 2, 2, 0.f, 0, 0, dt, 0));
    SHOW(dt ? "qmax, 2x1 window (bf16)" : "qmax, 2x1 window", crnn_bn_bwd_qmax_ex_p(X, Q, G, F, F, DX, 0, 0, 0, F, F, F, F, B, H, W, C, 2, 1, 0.f, 0, 0, dt, 0));
    SHOW(dt ? "qmax, no window (bf16)" : "qmax, no window", crnn_bn_bwd_qmax_ex_p(X, Q, G, F, F, DX, 0, 0, 0, F, F, F, F, B, H, W, C, 1, 1, 0.f, 0, 0, dt, 0));
    SHOW(dt ? "qmax, ragged height (bf16)" : "qmax, ragged height", crnn_bn_bwd_qmax_ex_p(X, Q, G, F, F, DX, 0, 0, 0, F, F, F, F, B, 5, W, C, 2, 2, 0.f, 0, 0, dt, 0));
    SHOW(dt ? "misaligned qmax (bf16)" : "misaligned qmax", crnn_bn_bwd_qmax_ex_p(X, Q_ODD, G, F, F, DX, 0, 0, 0, F, F, F, F, B, H, W, C, 1, 2, 0.f, 0, 0, dt, 0));
  }
  SHOW("planes with bf16", crnn_bn_bwd_qmax_ex_p(X, 0, G, F, F, 0, PL, n, 2, F, F, F, F, B, H, W, C, 1, 1, 0.f, 0, 0, 1, 0));
  SHOW("planes with bf16 and qmax", crnn_bn_bwd_qmax_ex_p(X, Q, G, F, F, 0, PL, n, 3, F, F, F, F, B, H, W, C, 2, 2, 0.f, 0, 0, 1, 0));
  SHOW("planes = 1", crnn_bn_bwd_qmax_ex_p(X, 0, G, F, F, 0, PL, n, 1, F, F, F, F, B, H, W, C, 1, 1, 0.f, 0, 0, 0, 0));
  SHOW("misaligned dx_planes", crnn_bn_bwd_qmax_ex_p(X, 0, G, F, F, 0, PL_ODD, n, 2, F, F, F, F, B, H, W, C, 1, 1, 0.f, 0, 0, 0, 0));
  SHOW("plane_stride too small", crnn_bn_bwd_qmax_ex_p(X, Q, G, F, F, 0, PL, n - 4, 2, F, F, F, F, B, H, W, C, 2, 2, 0.f, 0, 0, 0, 0));
  SHOW("planes, C % 4", crnn_bn_bwd_qmax_ex_p(X, 0, G, F, F, 0, PL, n, 2, F, F, F, F, B, H, W, 3, 1, 1, 0.f, 0, 0, 0, 0));

  fn = "crnn_bn_act_pool_drop_qmax_ex";
  for (int dti = 0; dti < 2; ++dti)
    for (int dto = 0; dto < 2; ++dto) {
      char tag[64];
      snprintf(tag, sizeof tag, "null x (in %d, out %d)", dti, dto); SHOW(tag, crnn_bn_act_pool_drop_qmax_ex_p(0, F, Y, Q, B, H, W, C, 2, 2, 0.f, 0, 0, dti, dto, 0));
      snprintf(tag, sizeof tag, "null bnstate (in %d, out %d)", dti, dto); SHOW(tag, crnn_bn_act_pool_drop_qmax_ex_p(X, 0, Y, Q, B, H, W, C, 2, 2, 0.f, 0, 0, dti, dto, 0));
      snprintf(tag, sizeof tag, "null qmax (in %d, out %d)", dti, dto); SHOW(tag, crnn_bn_act_pool_drop_qmax_ex_p(X, F, Y, 0, B, H, W, C, 2, 2, 0.f, 0, 0, dti, dto, 0));
      snprintf(tag, sizeof tag, "qmax, 2x1 window (in %d, out %d)", dti, dto); SHOW(tag, crnn_bn_act_pool_drop_qmax_ex_p(X, F, Y, Q, B, H, W, C, 2, 1, 0.f, 0, 0, dti, dto, 0));
      snprintf(tag, sizeof tag, "qmax, no window (in %d, out %d)", dti, dto); SHOW(tag, crnn_bn_act_pool_drop_qmax_ex_p(X, F, 0, Q, B, H, W, C, 1, 1, 0.f, 0, 0, dti, dto, 0));
      snprintf(tag, sizeof tag, "qmax, 2^31 elements (in %d, out %d)", dti, dto); SHOW(tag, crnn_bn_act_pool_drop_qmax_ex_p(X, F, Y, Q, 4096, 1024, 1024, 512, 2, 2, 0.f, 0, 0, dti, dto, 0));
    }

  fn = "crnn_bn_bwd_finalize";
  SHOW("null partials", crnn_bn_bwd_finalize_p(0, 4, C, 96, F, F, F, 0));
  SHOW("nparts = 0", crnn_bn_bwd_finalize_p(F, 0, C, 96, F, F, F, 0));
  SHOW("C = 0", crnn_bn_bwd_finalize_p(F, 4, 0, 96, F, F, F, 0));
  SHOW("count = 0", crnn_bn_bwd_finalize_p(F, 4, C, 0, F, F, F, 0));
  SHOW("null dgamma", crnn_bn_bwd_finalize_p(F, 4, C, 96, 0, F, F, 0));
  SHOW("null dbeta", crnn_bn_bwd_finalize_p(F, 4, C, 96, F, 0, F, 0));
  SHOW("null coef", crnn_bn_bwd_finalize_p(F, 4, C, 96, F, F, 0, 0));
  return 0;
}
