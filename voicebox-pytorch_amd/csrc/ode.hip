// ODE solver kernels of the sampler (solver.py RKSampler / Dopri5Sampler; torchdiffeq.odeint's euler, rk4 and dopri5 restated in
// tests/ode_ref.py).  Everything here is memory-bound: float4 loads and stores over the [B, N, D] state, grid-stride loops.  No kernel
// reads a host scalar that changes between replays of a captured graph: fixed grids take their coefficients and times from device
// tables indexed by a device counter, dopri5 from its fp64 step state (VBX_DP_*), which only the controller kernel writes.
//
// The error norm is deterministic and takes two launches: per-workgroup fp64 partial sums into a slab, then ONE workgroup sums the
// slab in a fixed order and runs the controller.  No float atomics, no hand-off between workgroups inside a launch: the kernel
// boundary makes the slab visible.
//
// Contraction is off for this file: every combination is the plain fp32 sum of fp32 products (as torch evaluates y0 + dt * f0), so a
// one-stage combination is bit-identical to the host's.
#pragma clang fp contract(off)
#include "common.hpp"

namespace {

constexpr int kMaxStages = VBX_ODE_MAX_STAGES;
constexpr int kNormThreads = 256;
constexpr int kNormMaxBlocks = 1024;

struct OdeTerms {
  const float* k[kMaxStages];
  float c[kMaxStages];
};

inline int ode_grid(long n4, int cap = 4096) {
  long b = (n4 + 255) / 256;
  return (int)(b > cap ? cap : (b < 1 ? 1 : b));
}

// the next fp32 value towards -inf (torch.nextafter(t, t - 1) for finite t)
VBX_DEV float prev_float(float x) {
  if (x != x || x == -__builtin_inff()) return x;
  if (x == 0.0f) return -__uint_as_float(1u);
  const unsigned u = __float_as_uint(x);
  return __uint_as_float(x > 0.0f ? u - 1u : u + 1u);
}

VBX_DEV float4 ld4(const float* p, long i) { return reinterpret_cast<const float4*>(p)[i]; }
VBX_DEV void st4(float* p, long i, float4 v) { reinterpret_cast<float4*>(p)[i] = v; }
VBX_DEV float4 operator+(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
VBX_DEV float4 operator-(float4 a, float4 b) { return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }
VBX_DEV float4 operator*(float4 a, float s) { return make_float4(a.x * s, a.y * s, a.z * s, a.w * s); }
VBX_DEV float4 operator*(float s, float4 a) { return make_float4(s * a.x, s * a.y, s * a.z, s * a.w); }

// coefficients of one combination: a row of the fixed-grid table (row counter * stride + row, ld floats per row), or -- state !=
// NULL -- beta_j * fp32(state[dt_slot]) as torchdiffeq's _runge_kutta_step forms them (dt cast to the state's dtype first)
VBX_DEV void load_coefs(float* c, const OdeTerms& t, int S, const float* table, int ld, const int* counter, int stride, int row,
                        const double* state, int dt_slot) {
  if (state) {
    const float dt = (float)state[dt_slot];
    for (int j = 0; j < S; j++) c[j] = t.c[j] * dt;
  } else {
    const float* r = table + ((long)counter[0] * stride + row) * ld;
    for (int j = 0; j < S; j++) c[j] = r[j];
  }
}

// sum_j c_j k_j[i] in stage order
VBX_DEV float4 stage_sum(const OdeTerms& t, const float* c, int S, long i) {
  float4 acc = ld4(t.k[0], i) * c[0];
  for (int j = 1; j < S; j++) acc = acc + ld4(t.k[j], i) * c[j];
  return acc;
}

// out = y + sum_j c_j k_j
__global__ void ode_combine_kernel(float* out, const float* y, OdeTerms t, int S, const float* table,
                                   int ld, const int* counter, int stride, int row, const double* state, int dt_slot, long n4) {
  float c[kMaxStages];
  load_coefs(c, t, S, table, ld, counter, stride, row, state, dt_slot);
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x)
    st4(out, i, ld4(y, i) + stage_sum(t, c, S, i));
}

// times[b] for every b: a table entry (fixed grids) or a dopri5 stage time derived from the fp64 step state
__global__ void ode_time_kernel(float* __restrict__ times, int B, const float* table, const int* counter, int stride, int slot,
                                const double* state, float alpha, int mode) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  float t;
  if (mode == VBX_ODE_TIME_TABLE) {
    t = table[(long)counter[0] * stride + slot];
  } else if (mode == VBX_ODE_TIME_STAGE) {  // fp32(t0) + alpha * fp32(dt), in fp32
    t = (float)state[VBX_DP_T] + alpha * (float)state[VBX_DP_DT];
  } else if (mode == VBX_ODE_TIME_END) {    // c = 1: fp32(t0 + dt), then the next fp32 value towards -inf (Perturb.PREV)
    t = prev_float((float)(state[VBX_DP_T] + state[VBX_DP_DT]));
  } else {                                  // VBX_ODE_TIME_PROBE: the initial-step probe at fp32(t0 + h0)
    t = (float)(state[VBX_DP_T] + state[VBX_DP_H0]);
  }
  times[b] = t;
}

// one workgroup's fixed-order tree over kNormThreads values (two lanes of sums)
VBX_DEV void block_sum2(double& a, double& b, double* sa, double* sb) {
  const int tid = threadIdx.x;
  sa[tid] = a;
  sb[tid] = b;
  __syncthreads();
  for (int s = kNormThreads / 2; s > 0; s >>= 1) {
    if (tid < s) {
      sa[tid] += sa[tid + s];
      sb[tid] += sb[tid + s];
    }
    __syncthreads();
  }
  a = sa[0];
  b = sb[0];
}

// Launch 1 of the norm: slab[block][2] = per-workgroup fp64 sums of squares.
//   ERROR: (err / tol)^2, err = sum_j (c_j fp32(dt)) k_j (k1 .. k7, never stored), tol = atol + rtol max(|y0|, |y1|)   (lane 0)
//   INIT0: (y0 / scale)^2 (lane 0) and (f0 / scale)^2 (lane 1), scale = atol + |y0| rtol, f0 = k[0]
//   INIT1: ((f1 - f0) / scale)^2 (lane 0), f0 = k[0], f1 = k[1]
// LENS (vbx_ode_norm_lens): the state is [B][N][D] with frame4 = D / 4 float4 per frame and batch4 = N * D / 4 per batch row; a frame
// at or past lens[b] is padding and is not read -- same grid, same order, so at full lengths the sums are those of the plain kernel.
template <bool LENS>
__global__ __launch_bounds__(kNormThreads) void ode_norm_partials_kernel(double* __restrict__ slab, int mode, const float* y0,
                                                                         const float* y1, OdeTerms t, int S, const double* state,
                                                                         long n4, const int* __restrict__ lens, long batch4, int frame4) {
  __shared__ double sa[kNormThreads], sb[kNormThreads];
  const float atol = (float)state[VBX_DP_ATOL], rtol = (float)state[VBX_DP_RTOL];
  float c[kMaxStages];
  if (mode == VBX_ODE_NORM_ERROR) load_coefs(c, t, S, nullptr, 0, nullptr, 0, 0, state, VBX_DP_DT);
  double a = 0.0, b = 0.0;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    if (LENS) {
      const long row = i / batch4;
      if ((i - row * batch4) / frame4 >= lens[row]) continue;
    }
    const float4 u = ld4(y0, i);
    if (mode == VBX_ODE_NORM_ERROR) {
      const float4 v = ld4(y1, i), e = stage_sum(t, c, S, i);
      const float q[4] = {e.x / (atol + rtol * fmaxf(fabsf(u.x), fabsf(v.x))), e.y / (atol + rtol * fmaxf(fabsf(u.y), fabsf(v.y))),
                          e.z / (atol + rtol * fmaxf(fabsf(u.z), fabsf(v.z))), e.w / (atol + rtol * fmaxf(fabsf(u.w), fabsf(v.w)))};
      for (int j = 0; j < 4; j++) a += (double)q[j] * (double)q[j];
    } else {
      const float s[4] = {atol + fabsf(u.x) * rtol, atol + fabsf(u.y) * rtol, atol + fabsf(u.z) * rtol, atol + fabsf(u.w) * rtol};
      const float4 f0 = ld4(t.k[0], i);
      if (mode == VBX_ODE_NORM_INIT0) {
        const float p[4] = {u.x / s[0], u.y / s[1], u.z / s[2], u.w / s[3]};
        const float r[4] = {f0.x / s[0], f0.y / s[1], f0.z / s[2], f0.w / s[3]};
        for (int j = 0; j < 4; j++) {
          a += (double)p[j] * (double)p[j];
          b += (double)r[j] * (double)r[j];
        }
      } else {
        const float4 d = ld4(t.k[1], i) - f0;
        const float p[4] = {d.x / s[0], d.y / s[1], d.z / s[2], d.w / s[3]};
        for (int j = 0; j < 4; j++) a += (double)p[j] * (double)p[j];
      }
    }
  }
  block_sum2(a, b, sa, sb);
  if (threadIdx.x == 0) {
    slab[2 * blockIdx.x] = a;
    slab[2 * blockIdx.x + 1] = b;
  }
}

// Launch 2: one workgroup sums the slab in a fixed order (thread i: entries i, i + 256, ...; then the tree) and runs the controller.
// lens != NULL: the mean is over the kept elements, n = row_elems * sum_b lens[b].
__global__ __launch_bounds__(kNormThreads) void ode_control_kernel(double* __restrict__ state, const double* __restrict__ slab,
                                                                   int nblocks, long n, int mode, int nfe_per_eval,
                                                                   const int* __restrict__ lens, int B, int row_elems) {
  __shared__ double sa[kNormThreads], sb[kNormThreads];
  if (lens) {
    long frames = 0;
    for (int i = 0; i < B; i++) frames += lens[i];
    n = frames * row_elems;
  }
  double a = 0.0, b = 0.0;
  for (int i = threadIdx.x; i < nblocks; i += kNormThreads) {
    a += slab[2 * i];
    b += slab[2 * i + 1];
  }
  block_sum2(a, b, sa, sb);
  if (threadIdx.x != 0) return;
  double* s = state;
  if (mode == VBX_ODE_CTRL_INIT0) {  // _select_initial_step: d0, d1 -> h0 (fp32, as torch evaluates it on fp32 norms)
    const float d0 = (float)sqrt(a / (double)n), d1 = (float)sqrt(b / (double)n);
    const float h0 = (d0 < 1e-5f || d1 < 1e-5f) ? 1e-6f : 0.01f * d0 / d1;
    s[VBX_DP_H0] = (double)h0;
    s[VBX_DP_D1] = (double)d1;
    s[VBX_DP_NFE] += nfe_per_eval;  // f0
    return;
  }
  if (mode == VBX_ODE_CTRL_INIT1) {  // d2 -> h1 -> the first step min(100 h0, h1)
    const float h0 = (float)s[VBX_DP_H0], d1 = (float)s[VBX_DP_D1];
    const float d2 = (float)sqrt(a / (double)n) / h0;
    const float h1 = (d1 <= 1e-15f && d2 <= 1e-15f) ? fmaxf(1e-6f, h0 * 1e-3f) : powf(0.01f / fmaxf(d1, d2), 1.0f / 5.0f);
    s[VBX_DP_DT] = (double)fminf(100.0f * h0, h1);
    s[VBX_DP_NFE] += nfe_per_eval;  // the probe
    return;
  }
  // VBX_ODE_CTRL_STEP: accept / reject, the next step size (_optimal_step_size: safety 0.9, ifactor 10, dfactor 0.2, order 5)
  const double ratio = sqrt(a / (double)n), dt = s[VBX_DP_DT], t = s[VBX_DP_T];
  s[VBX_DP_RATIO] = ratio;
  s[VBX_DP_NFE] += 6.0 * nfe_per_eval;
  if (!(ratio == ratio) || ratio > 1e300) {  // non-finite state or error: the host raises
    s[VBX_DP_BAD] = 1.0;
    s[VBX_DP_LAST] = 0.0;
    return;
  }
  const bool accept = ratio <= 1.0;
  double dt_next;
  if (ratio == 0.0) {
    dt_next = dt * 10.0;
  } else {
    const double dfactor = ratio < 1.0 ? 1.0 : 0.2;
    dt_next = dt * fmin(10.0, fmax(0.9 / pow(ratio, 1.0 / 5.0), dfactor));
  }
  if (accept) {
    s[VBX_DP_T0] = t;
    s[VBX_DP_T1] = t + dt;
    s[VBX_DP_DT32] = (double)(float)dt;
    s[VBX_DP_T] = t + dt;
    s[VBX_DP_ACCEPTED] += 1.0;
    s[VBX_DP_DONE] = (t + dt >= s[VBX_DP_TEND]) ? 1.0 : 0.0;
  } else {
    s[VBX_DP_REJECTED] += 1.0;
  }
  s[VBX_DP_LAST] = accept ? 1.0 : 0.0;
  s[VBX_DP_DT] = dt_next;
  if (!(s[VBX_DP_T] + dt_next > s[VBX_DP_T])) s[VBX_DP_BAD] = 2.0;  // underflow in dt
}

// accepted and not finished: y <- y1, k1 <- k7 (FSAL).  The last accepted step keeps y0, y1 and k1 .. k7 for the dense output.
__global__ void ode_commit_kernel(float* __restrict__ y, float* __restrict__ k1, const float* __restrict__ y1,
                                  const float* __restrict__ k7, const double* __restrict__ state, long n4) {
  if (state[VBX_DP_LAST] == 0.0 || state[VBX_DP_DONE] != 0.0) return;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    st4(y, i, ld4(y1, i));
    st4(k1, i, ld4(k7, i));
  }
}

// torchdiffeq's _interp_fit + _interp_evaluate at t_end inside the last accepted step [t0, t1]:
// y_mid = y0 + sum_j (mid_j dt) k_j; y(x) = e + d x + c x^2 + b x^3 + a x^4, x = fp32((t_end - t0) / (t1 - t0))
__global__ void ode_dense_kernel(float* __restrict__ out, const float* __restrict__ y0, const float* __restrict__ y1, OdeTerms t,
                                 const double* __restrict__ state, long n4) {
  float c[kMaxStages];
  load_coefs(c, t, kMaxStages, nullptr, 0, nullptr, 0, 0, state, VBX_DP_DT32);
  const float dt = (float)state[VBX_DP_DT32];
  const float x = (float)((state[VBX_DP_TEND] - state[VBX_DP_T0]) / (state[VBX_DP_T1] - state[VBX_DP_T0]));
  const float x2 = x * x, x3 = x2 * x, x4 = x3 * x;
  const float dt2 = 2.0f * dt;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    const float4 u = ld4(y0, i), v = ld4(y1, i), f0 = ld4(t.k[0], i), f1 = ld4(t.k[kMaxStages - 1], i);
    const float4 ym = u + stage_sum(t, c, kMaxStages, i);
    const float4 qa = dt2 * (f1 - f0) - 8.0f * (v + u) + 16.0f * ym;
    const float4 qb = dt * (5.0f * f0 - 3.0f * f1) + 18.0f * u + 14.0f * v - 32.0f * ym;
    const float4 qc = dt * (f1 - 4.0f * f0) - 11.0f * u - 5.0f * v + 16.0f * ym;
    const float4 qd = dt * f0;
    st4(out, i, u + qd * x + qc * x2 + qb * x3 + qa * x4);
  }
}

// x[b][n][:] = 0 for n >= lens[b]
__global__ void zero_tail_rows_kernel(float* __restrict__ x, const int* __restrict__ lens, long total, long ND, int D) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long b = i / ND;
    if ((i - b * ND) / D >= lens[b]) x[i] = 0.f;
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

bool load_terms(OdeTerms& t, const float* const* k, const float* c, int S) {
  for (int j = 0; j < kMaxStages; j++) {
    t.k[j] = nullptr;
    t.c[j] = 0.f;
  }
  for (int j = 0; j < S; j++) {
    if (!k[j] || !aligned16(k[j])) return false;
    t.k[j] = k[j];
    t.c[j] = c ? c[j] : 0.f;
  }
  return true;
}

int norm_blocks(long n4) { return ode_grid(n4, kNormMaxBlocks); }

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int vbx_ode_combine(float* out, const float* y, const float* const* k, int S, const float* table, int ld,
                               const int* counter, int stride, int row, long n, void* stream) {
  OdeTerms t;
  VBX_REQUIRE(out && y && k && table && counter && S >= 1 && S <= kMaxStages && ld >= S && stride >= 1 && row >= 0 && n > 0 &&
                  n % 4 == 0 && aligned16(out) && aligned16(y) && load_terms(t, k, nullptr, S),
              "vbx_ode_combine: bad args");
  hipLaunchKernelGGL(ode_combine_kernel, dim3(ode_grid(n / 4)), dim3(256), 0, ST, out, y, t, S, table, ld, counter, stride, row,
                     nullptr, 0, n / 4);
  VBX_LAUNCH_CHECK();
  return 0;
}

extern "C" int vbx_ode_combine_dp(float* out, const float* y, const float* const* k, const float* beta, int S, const double* state,
                                  int dt_slot, long n, void* stream) {
  OdeTerms t;
  VBX_REQUIRE(out && y && k && beta && state && S >= 1 && S <= kMaxStages && (dt_slot == VBX_DP_DT || dt_slot == VBX_DP_H0) &&
                  n > 0 && n % 4 == 0 && aligned16(out) && aligned16(y) && load_terms(t, k, beta, S),
              "vbx_ode_combine_dp: bad args");
  hipLaunchKernelGGL(ode_combine_kernel, dim3(ode_grid(n / 4)), dim3(256), 0, ST, out, y, t, S, nullptr, 0, nullptr, 0, 0, state,
                     dt_slot, n / 4);
  VBX_LAUNCH_CHECK();
  return 0;
}

extern "C" int vbx_ode_stage_time(float* times, int B, const float* table, const int* counter, int stride, int slot, void* stream) {
  VBX_REQUIRE(times && table && counter && B > 0 && stride >= 1 && slot >= 0 && slot < stride, "vbx_ode_stage_time: bad args");
  hipLaunchKernelGGL(ode_time_kernel, dim3(cdiv(B, 64)), dim3(64), 0, ST, times, B, table, counter, stride, slot, nullptr, 0.f,
                     (int)VBX_ODE_TIME_TABLE);
  VBX_LAUNCH_CHECK();
  return 0;
}

extern "C" int vbx_ode_stage_time_dp(float* times, int B, const double* state, float alpha, int mode, void* stream) {
  VBX_REQUIRE(times && state && B > 0 && mode >= VBX_ODE_TIME_STAGE && mode <= VBX_ODE_TIME_PROBE, "vbx_ode_stage_time_dp: bad args");
  hipLaunchKernelGGL(ode_time_kernel, dim3(cdiv(B, 64)), dim3(64), 0, ST, times, B, nullptr, nullptr, 0, 0, state, alpha, mode);
  VBX_LAUNCH_CHECK();
  return 0;
}

extern "C" long vbx_ode_norm_slab_doubles(long n) { return 2L * norm_blocks(n / 4); }

// lens == NULL: the whole state (vbx_ode_norm); else the state is [B][n / (B row_elems)][row_elems] and frames >= lens[b] are left out
static int ode_norm_impl(double* state, double* slab, int mode, const float* y0, const float* y1, const float* const* k, const float* c,
                         int S, long n, int nfe_per_eval, const int* lens, int B, int row_elems, void* stream) {
  OdeTerms t;
  const bool err = mode == VBX_ODE_NORM_ERROR;
  const int need = err ? S : (mode == VBX_ODE_NORM_INIT0 ? 1 : 2);
  VBX_REQUIRE(state && slab && y0 && k && mode >= VBX_ODE_NORM_ERROR && mode <= VBX_ODE_NORM_INIT1 && S == need &&
                  S <= kMaxStages && (!err || (y1 && c && aligned16(y1))) && n > 0 && n % 4 == 0 && aligned16(y0) &&
                  load_terms(t, k, c, S) && nfe_per_eval >= 1,
              "vbx_ode_norm: bad args");
  VBX_REQUIRE(!lens || (B > 0 && row_elems > 0 && row_elems % 4 == 0 && n % ((long)B * row_elems) == 0),
              "vbx_ode_norm_lens: the state must be [B][N][row_elems] with row_elems a multiple of 4");
  const int nb = norm_blocks(n / 4);
  if (lens)
    hipLaunchKernelGGL(ode_norm_partials_kernel<true>, dim3(nb), dim3(kNormThreads), 0, ST, slab, mode, y0, y1, t, S, state, n / 4, lens,
                       n / B / 4, row_elems / 4);
  else
    hipLaunchKernelGGL(ode_norm_partials_kernel<false>, dim3(nb), dim3(kNormThreads), 0, ST, slab, mode, y0, y1, t, S, state, n / 4,
                       nullptr, 0L, 0);
  VBX_LAUNCH_CHECK();
  const int ctrl = err ? VBX_ODE_CTRL_STEP : (mode == VBX_ODE_NORM_INIT0 ? VBX_ODE_CTRL_INIT0 : VBX_ODE_CTRL_INIT1);
  hipLaunchKernelGGL(ode_control_kernel, dim3(1), dim3(kNormThreads), 0, ST, state, slab, nb, n, ctrl, nfe_per_eval, lens, B, row_elems);
  VBX_LAUNCH_CHECK();
  return 0;
}

extern "C" int vbx_ode_norm(double* state, double* slab, int mode, const float* y0, const float* y1, const float* const* k,
                            const float* c, int S, long n, int nfe_per_eval, void* stream) {
  return ode_norm_impl(state, slab, mode, y0, y1, k, c, S, n, nfe_per_eval, nullptr, 0, 0, stream);
}

extern "C" int vbx_ode_norm_lens(double* state, double* slab, int mode, const float* y0, const float* y1, const float* const* k,
                                 const float* c, int S, long n, int nfe_per_eval, const int* lens, int B, int row_elems, void* stream) {
  return ode_norm_impl(state, slab, mode, y0, y1, k, c, S, n, nfe_per_eval, lens, B, row_elems, stream);
}

extern "C" int vbx_zero_tail_rows(float* x, const int* lens, int B, int N, int D, void* stream) {
  VBX_REQUIRE(x && lens && B > 0 && N > 0 && D > 0, "vbx_zero_tail_rows: bad args");
  const long total = (long)B * N * D;
  hipLaunchKernelGGL(zero_tail_rows_kernel, dim3(ode_grid(total)), dim3(256), 0, ST, x, lens, total, (long)N * D, D);
  VBX_LAUNCH_CHECK();
  return 0;
}

extern "C" int vbx_ode_commit(float* y, float* k1, const float* y1, const float* k7, const double* state, long n, void* stream) {
  VBX_REQUIRE(y && k1 && y1 && k7 && state && n > 0 && n % 4 == 0 && aligned16(y) && aligned16(k1) && aligned16(y1) && aligned16(k7),
              "vbx_ode_commit: bad args");
  hipLaunchKernelGGL(ode_commit_kernel, dim3(ode_grid(n / 4)), dim3(256), 0, ST, y, k1, y1, k7, state, n / 4);
  VBX_LAUNCH_CHECK();
  return 0;
}

extern "C" int vbx_ode_dense(float* out, const float* y0, const float* y1, const float* const* k, const float* mid,
                             const double* state, long n, void* stream) {
  OdeTerms t;
  VBX_REQUIRE(out && y0 && y1 && k && mid && state && n > 0 && n % 4 == 0 && aligned16(out) && aligned16(y0) && aligned16(y1) &&
                  load_terms(t, k, mid, kMaxStages),
              "vbx_ode_dense: bad args");
  hipLaunchKernelGGL(ode_dense_kernel, dim3(ode_grid(n / 4)), dim3(256), 0, ST, out, y0, y1, t, state, n / 4);
  VBX_LAUNCH_CHECK();
  return 0;
}
