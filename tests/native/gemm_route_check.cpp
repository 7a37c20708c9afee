// csrc/gemm_route.hpp on the host (no GPU): the kernel that serves every GEMM the model issues, at dim 512 and dim 1024, for a full
// batch (M = 8 x 1040 rows) and the sampler's half batch (4 x 1040), vbx_gemm_select paths 0-4, VBX_GEMM5 on / off.
// The expected kernels were written down from the launches of the code BEFORE the rules moved into gemm_route.hpp: its kernel traces
// of the train step and of the 4-interval sample at both widths (profiles/refactor_dispatch_*_launches.txt show the same tables),
// profiles/r06_train_step_kernel_stats.txt, and its per-kernel eligibility rules for the arms no trace covers.
#include <cstdio>
#include <cstring>
#include "../../voicebox-pytorch_amd/csrc/gemm_route.hpp"

enum { G3 = VBX_GEMM_KERNEL_GEMM3, G4 = VBX_GEMM_KERNEL_GEMM4, G5 = VBX_GEMM_KERNEL_GEMM5, T64 = VBX_GEMM_KERNEL_BM64,
       T128 = VBX_GEMM_KERNEL_BM128, T160 = VBX_GEMM_KERNEL_BM160 };

static int fails = 0;
static char placeholder[64] __attribute__((aligned(16)));

struct Cfg { int D, batch; };
static const Cfg cfgs[4] = {{512, 8}, {512, 4}, {1024, 8}, {1024, 4}};

// per GEMM and configuration: the gemm.hip tile that serves it when only those kernels are selected (path 1), and the automatic
// choice (path 0) with VBX_GEMM5 on / off
struct Row {
  const char* name;
  int tile[4], auto_g5[4], auto_tiled[4];
};
static const Row rows[] = {
    //                      128-wide kernels only        automatic, gemm5 on         automatic, VBX_GEMM5=0
    {"to_embed",           {T160, T160, T160, T160},    {T160, T160, T160, T160},   {T160, T160, T160, T160}},
    {"to_qkv (training)",  {T128, T128, T128, T128},    {G5, G5, T128, T128},       {T128, T128, T128, T128}},
    {"to_qkv (inference)", {T128, T128, T128, T128},    {G5, G5, T128, T128},       {T128, T128, T128, T128}},
    {"to_out",             {T160, T160, T160, T160},    {T160, T160, T160, T160},   {T160, T160, T160, T160}},
    {"ff_in (training)",   {T128, T128, T128, T128},    {G5, G5, T128, T128},       {T128, T128, T128, T128}},
    {"ff_in (inference)",  {T128, T128, T128, T128},    {G5, G5, G4, G4},           {G4, G4, G4, G4}},
    {"ff_out",             {T160, T160, T160, T160},    {T160, T160, T160, T160},   {T160, T160, T160, T160}},
    {"to_pred",            {T160, T160, T160, T160},    {T160, T160, T160, T160},   {T160, T160, T160, T160}},
    {"dgrad to_pred",      {T160, T160, T160, T160},    {T160, T160, T160, T160},   {T160, T160, T160, T160}},
    {"dgrad ff_out",       {T128, T64, T160, T160},     {G4, T64, T160, T160},      {G4, T64, T160, T160}},
    {"dgrad ff_in",        {T160, T160, T160, T160},    {T160, T160, T160, T160},   {T160, T160, T160, T160}},
    {"dgrad to_out",       {T128, T160, T160, T160},    {G4, T160, T160, T160},     {G4, T160, T160, T160}},
    {"dgrad to_qkv",       {T160, T160, T160, T160},    {T160, T160, T160, T160},   {T160, T160, T160, T160}},
    {"wgrad to_qkv",       {T128, T128, T128, T128},    {T128, T128, T128, T128},   {T128, T128, T128, T128}},
    {"wgrad to_out",       {T128, T128, T128, T128},    {T128, T128, T128, T128},   {T128, T128, T128, T128}},
    {"wgrad ff_in",        {T128, T128, T128, T128},    {T128, T128, T128, T128},   {T128, T128, T128, T128}},
    {"wgrad ff_out",       {T128, T128, T128, T128},    {T128, T128, T128, T128},   {T128, T128, T128, T128}},
    {"wgrad to_embed",     {T128, T128, T128, T128},    {T128, T128, T128, T128},   {T128, T128, T128, T128}},
    {"wgrad to_pred",      {T128, T128, T128, T128},    {T128, T128, T128, T128},   {T128, T128, T128, T128}},
};

// the descriptor runtime.hip builds for that GEMM (bench.py's model: 16 heads of 64, 1024 frames + 16 register tokens, dim_in = dim)
static vbx_gemm_desc desc_of(const char* name, const Cfg& c) {
  const int D = c.D, I = 16 * 64, Fp = ((D * 4 * 2 / 3) + 63) / 64 * 64, Np = 1040, M = c.batch * Np, M0 = c.batch * 1024;
  vbx_gemm_desc d;
  memset(&d, 0, sizeof(d));
  void* p = placeholder;
  d.A = p; d.B = p; d.C = p;
  auto dims = [&](int mode, int epi, int m, int n, int k) { d.mode = mode; d.epilogue = epi; d.M = m; d.N = n; d.K = k; };
  auto nt_f32 = [&](int m, int n, int k) { dims(VBX_GEMM_NT, VBX_EPI_F32, m, n, k); d.lda = d.ldb = k; d.ldc = n; d.f16 = 1; };
  auto nn = [&](int m, int n, int k) { dims(VBX_GEMM_NN, VBX_EPI_BF16, m, n, k); d.lda = k; d.ldb = d.ldc = n; };
  auto tn = [&](int i, int j, int k) { dims(VBX_GEMM_TN, VBX_EPI_SPLITK, i, j, k); d.lda = i; d.ldb = j; d.splits = 3; };
  const bool training = strstr(name, "(training)") != nullptr;
  if (!strcmp(name, "to_embed")) nt_f32(M0, D, 2 * D);
  else if (!strncmp(name, "to_qkv", 6)) {
    dims(VBX_GEMM_NT, VBX_EPI_QKV, M, 3 * I, D); d.lda = d.ldb = D; d.f16 = 1; d.Np = Np; d.H = 16; d.qk_scale = 8.f;
    d.q_gamma = d.k_gamma = d.rot_cos = d.rot_sin = (const float*)p; d.q16 = d.k16 = d.v16 = p;
    if (training) { d.qb = d.kb = d.v = p; d.q_rnorm = d.k_rnorm = (float*)p; }
  } else if (!strcmp(name, "to_out")) nt_f32(M, D, I);
  else if (!strncmp(name, "ff_in", 5)) {
    dims(VBX_GEMM_NT, VBX_EPI_GEGLU, M, 2 * Fp, D); d.lda = d.ldb = D; d.ldc = Fp; d.f16 = 1; d.bias = (const float*)p;
    if (training) d.C2 = d.C3 = p;
  } else if (!strcmp(name, "ff_out")) nt_f32(M, D, Fp);
  else if (!strcmp(name, "to_pred")) nt_f32(M0, D, D);
  else if (!strcmp(name, "dgrad to_pred")) nn(M0, D, D);
  else if (!strcmp(name, "dgrad ff_out")) nn(M, Fp, D);
  else if (!strcmp(name, "dgrad ff_in")) nn(M, D, 2 * Fp);
  else if (!strcmp(name, "dgrad to_out")) nn(M, I, D);
  else if (!strcmp(name, "dgrad to_qkv")) nn(M, D, 3 * I);
  else if (!strcmp(name, "wgrad to_qkv")) tn(3 * I, D, M);
  else if (!strcmp(name, "wgrad to_out")) tn(D, I, M);
  else if (!strcmp(name, "wgrad ff_in")) tn(2 * Fp, D, M);
  else if (!strcmp(name, "wgrad ff_out")) tn(D, Fp, M);
  else if (!strcmp(name, "wgrad to_embed")) tn(D, 2 * D, M0);
  else if (!strcmp(name, "wgrad to_pred")) tn(D, D, M0);
  else { printf("FAIL unknown GEMM %s\n", name); fails++; }
  return d;
}

static void expect(const char* what, const vbx_gemm_desc& d, const gemm_route::Facts& f, int want) {
  const int got = gemm_route::route(&d, f);
  if (got != want) {
    if (fails < 40) printf("FAIL %s, path %d, gemm5 %d, %d CUs: kernel %d, expected %d\n", what, f.path, (int)f.gemm5, f.cus, got, want);
    fails++;
  }
}

int main() {
  int checked = 0;
  for (const Row& r : rows)
    for (int ci = 0; ci < 4; ci++) {
      const vbx_gemm_desc d = desc_of(r.name, cfgs[ci]);
      char what[96];
      snprintf(what, sizeof(what), "%s, dim %d, batch %d", r.name, cfgs[ci].D, cfgs[ci].batch);
      for (int g5 = 0; g5 < 2; g5++) {
        const bool tn = d.mode == VBX_GEMM_TN;
        expect(what, d, {0, g5 != 0, 256}, g5 ? r.auto_g5[ci] : r.auto_tiled[ci]);
        expect(what, d, {1, g5 != 0, 256}, r.tile[ci]);
        expect(what, d, {2, g5 != 0, 256}, G3);                    // the 256 x 256 tile serves every one of them
        expect(what, d, {3, g5 != 0, 256}, tn ? r.tile[ci] : G4);  // the 128 x 256 tile every NT / NN one
        expect(what, d, {4, g5 != 0, 256}, r.auto_g5[ci]);         // automatic with gemm5 on whatever the preset says
        checked += 5;
      }
    }
  // what makes gemm5 pass a descriptor on: fewer CUs than weight panels (vbx_gemm5_cu_limit; to_qkv has 12 panels of 256 features),
  // an operand that is not 16-byte aligned, only some of the backward's copies
  vbx_gemm_desc q = desc_of("to_qkv (inference)", cfgs[0]);
  expect("to_qkv on a 128-CU share", q, {0, true, 128}, G5);
  expect("to_qkv on 8 CUs", q, {0, true, 8}, T128);
  q.A = placeholder + 8;
  expect("to_qkv, A not 16-byte aligned", q, {0, true, 256}, T128);
  q = desc_of("to_qkv (training)", cfgs[0]);
  q.q_rnorm = nullptr;
  expect("to_qkv with some of the backward's copies", q, {0, true, 256}, T128);
  checked += 4;
  if (fails) { printf("%d of %d routes differ\n", fails, checked); return 1; }
  printf("gemm route check ok: %d routes\n", checked);
  return 0;
}
