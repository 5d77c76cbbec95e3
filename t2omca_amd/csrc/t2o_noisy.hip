// t2o_noisy.hip — the NoisyNet Q head of TransformerAgent (transf_agent.py:37-39,
// args.action_selector == "noisy-new": q_basic is a NoisyLinear).
//
// utils.noisy_liner does not ship with the reference, so the layer is this
// project's DECLARED definition (parity-unpinned; DESIGN.md §5, restated in fp64 in
// tests/noisy_model.py): the independent-Gaussian NoisyNet layer as PyMARL2 uses it,
//
//   q = (u_w + s_w ⊙ ε_w) h + (u_b + s_b ⊙ ε_b),   ε ~ N(0, 1) per element,
//
// with u_w [NA][E], u_b [NA] the means (the plain q_basic.weight / bias) and s_w, s_b
// the sigmas.  The head is a separate E -> NA linear layer on the agent's hidden
// token, so it runs here beside the fused agent kernels, which stay as they are: the
// agent unroll writes h, these kernels overwrite its q, and in the backward they
// turn dL/dq[action] into dL/dh for the agent BPTT, which then runs without a q
// gradient.  Everything is fp32 in both learner precisions (h is fp32 already; bf16
// operands stop at the fused kernels).
//
// Noise.  Counter-based like every other draw (env_spec.uniforms): element k of
// step t — k = n·E + e for ε_w[n][e], k = NA·E + n for ε_b[n] — is Box–Muller on
//   u1 = U(seed', env = t, draw = c·4096 + 2k),  u2 = U(seed', t, c·4096 + 2k + 1),
//   seed' = (4·seed + kind) mod 2^64,
//   z = sqrt(−2 ln(1 − u1)) · cos(2π u2)   in fp64, rounded once to fp32,
// c the caller's call counter, kind 0 learner online / 1 learner target / 2 runner /
// 3 module forward.  NA·(E+1) <= 2048 keeps 2k + 1 < 4096, t < 2^24 and c < 2^28
// keep (t << 40) | draw inside 64 bits.
//
// Kernels (wave64, no atomics, no allocation, no synchronisation):
//   noise_kernel     one thread per (t, k)
//   noisy_fwd_kernel a workgroup takes rows b·A + a of one step t, stages that step's
//                    effective W_t, b_t in LDS once, and streams h with 16-byte loads:
//                    LPR = 4 / 8 / 16 lanes share a row (one float4 of it each), the
//                    NA dot products are summed across them by xor shuffles
//   noisy_bwd_kernel same lane map; gh_out = gh_in + g·W_t[action], and the weight
//                    gradient partials of (step, row part) accumulate in LDS, one
//                    private [NA][E+1] block per row slot, summed over the slots in
//                    slot order: a fixed order, so the result is bit-identical run to
//                    run and does not depend on the step ranges of the calls
//   noisy_wgrad_kernel  one wave per weight element: Σ_t over the partials (lane l
//                    takes t = l, l + 64, ...; xor butterfly), += into the caller's slots
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/t2omca.h"

namespace {

constexpr int NOISY_MAXE = 64, NOISY_MAXNA = 16, NOISY_MAXA = 64;
constexpr int NOISY_THREADS = 256;
constexpr int NOISY_PART_ROWS = 1024;  // rows of one step per backward workgroup
constexpr int NOISY_MAX_PARTS = 8;

// env_spec.uniforms
__device__ __forceinline__ double noisy_uniform(uint64_t seed, int64_t env, int64_t idx) {
  uint64_t x = ((uint64_t)env << 40) | (uint64_t)idx;
  x ^= seed * 0xD1B54A32D192ED03ull;
  uint64_t z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z = z ^ (z >> 31);
  return (double)(z >> 11) * 0x1.0p-53;
}

__global__ void noise_kernel(float* __restrict__ eps_w, float* __restrict__ eps_b, uint64_t seedp, int64_t counter,
                             int E, int NA, int t0, int t1) {
  const int NW = NA * E, NK = NW + NA;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)(t1 - t0) * NK) return;
  const int t = t0 + (int)(i / NK), k = (int)(i % NK);
  const int64_t d = counter * 4096 + 2 * k;
  const double u1 = noisy_uniform(seedp, t, d), u2 = noisy_uniform(seedp, t, d + 1);
  const double z = sqrt(-2.0 * log(1.0 - u1)) * cos(6.283185307179586 * u2);
  if (k < NW)
    eps_w[(int64_t)t * NW + k] = (float)z;
  else
    eps_b[(int64_t)t * NA + (k - NW)] = (float)z;
}

// floats [e0, e0 + 4) of a row of E (zeros past E); VEC: E % 4 == 0 and the base 16-byte aligned
template <bool VEC>
__device__ __forceinline__ float4 load4(const float* __restrict__ row, int e0, int E) {
  if (VEC) return e0 < E ? *reinterpret_cast<const float4*>(row + e0) : make_float4(0.f, 0.f, 0.f, 0.f);
  float4 v;
  v.x = e0 + 0 < E ? row[e0 + 0] : 0.f;
  v.y = e0 + 1 < E ? row[e0 + 1] : 0.f;
  v.z = e0 + 2 < E ? row[e0 + 2] : 0.f;
  v.w = e0 + 3 < E ? row[e0 + 3] : 0.f;
  return v;
}

template <bool VEC>
__device__ __forceinline__ void store4(float* __restrict__ row, int e0, int E, float4 v) {
  if (VEC) {
    if (e0 < E) *reinterpret_cast<float4*>(row + e0) = v;
    return;
  }
  if (e0 + 0 < E) row[e0 + 0] = v.x;
  if (e0 + 1 < E) row[e0 + 1] = v.y;
  if (e0 + 2 < E) row[e0 + 2] = v.z;
  if (e0 + 3 < E) row[e0 + 3] = v.w;
}

// W_t = u_w + s_w ⊙ ε_w[t] into Ws [NA][EP] (columns past E zero)
__device__ __forceinline__ void stage_weights(float* Ws, int EP, const float* __restrict__ u_w,
                                              const float* __restrict__ s_w, const float* __restrict__ eps_w, int t,
                                              int E, int NA) {
  for (int i = threadIdx.x; i < NA * EP; i += blockDim.x) {
    const int n = i / EP, e = i % EP;
    float w = 0.f;
    if (e < E) {
      w = u_w[n * E + e];
      if (eps_w) w = fmaf(s_w[n * E + e], eps_w[((int64_t)t * NA + n) * E + e], w);
    }
    Ws[i] = w;
  }
}

struct FwdP {
  const float *h, *u_w, *u_b, *s_w, *s_b, *eps_w, *eps_b;
  float* q;
  int h_ts, q_ts, B, A, E, NA, t0;
};

template <int LPR, bool VEC>
__global__ __launch_bounds__(NOISY_THREADS) void noisy_fwd_kernel(FwdP p) {
  constexpr int EP = LPR * 4, S = NOISY_THREADS / LPR;
  __shared__ __attribute__((aligned(16))) float Ws[NOISY_MAXNA * EP];
  __shared__ float Bs[NOISY_MAXNA];
  const int t = p.t0 + blockIdx.y, E = p.E, NA = p.NA, A = p.A;
  stage_weights(Ws, EP, p.u_w, p.s_w, p.eps_w, t, E, NA);
  if ((int)threadIdx.x < NA) {
    const int n = threadIdx.x;
    float b = p.u_b[n];
    if (p.eps_b) b = fmaf(p.s_b[n], p.eps_b[(int64_t)t * NA + n], b);
    Bs[n] = b;
  }
  __syncthreads();
  const int s = threadIdx.x / LPR, j = threadIdx.x % LPR;
  const int R = p.B * A;
  // (the trip count is the same for every lane of the workgroup: the shuffles below need whole groups)
  for (int r0 = blockIdx.x * S; r0 < R; r0 += gridDim.x * S) {
    const int r = r0 + s;
    const bool ok = r < R;
    const int b = ok ? r / A : 0, a = ok ? r % A : 0;
    float4 hv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ok) hv = load4<VEC>(p.h + (((int64_t)b * p.h_ts + t) * A + a) * E, 4 * j, E);
    float* qrow = p.q + (((int64_t)b * p.q_ts + t) * A + a) * NA;
    for (int n = 0; n < NA; ++n) {
      const float4 w = *reinterpret_cast<const float4*>(&Ws[n * EP + 4 * j]);
      float acc = fmaf(hv.w, w.w, fmaf(hv.z, w.z, fmaf(hv.y, w.y, hv.x * w.x)));
#pragma unroll
      for (int m = LPR / 2; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, LPR);
      if (ok && j == n % LPR) qrow[n] = acc + Bs[n];
    }
  }
}

struct BwdP {
  const float* gchosen;
  const int64_t* actions;
  int64_t act_sb, act_st;
  const float *h, *u_w, *s_w, *eps_w, *gh_in;
  float *gh_out, *gpart;
  int h_ts, B, T, A, E, NA, t_lo;
};

// grid (steps, parts); blockDim.x = S * LPR threads; dynamic LDS: Ws [NA][EP], Gs [S][NA][EP], Gb [S][NA]
template <int LPR, bool VEC>
__global__ __launch_bounds__(NOISY_THREADS) void noisy_bwd_kernel(BwdP p) {
  constexpr int EP = LPR * 4;
  extern __shared__ __attribute__((aligned(16))) float noisy_smem[];
  const int S = blockDim.x / LPR;
  const int t = p.t_lo + blockIdx.x, part = blockIdx.y, P = gridDim.y;
  const int E = p.E, NA = p.NA, A = p.A;
  float* Ws = noisy_smem;
  float* Gs = Ws + NA * EP;
  float* Gb = Gs + S * NA * EP;
  stage_weights(Ws, EP, p.u_w, p.s_w, p.eps_w, t, E, NA);
  for (int i = threadIdx.x; i < S * NA * EP + S * NA; i += blockDim.x) Gs[i] = 0.f;  // (Gb follows Gs)
  __syncthreads();
  const int s = threadIdx.x / LPR, j = threadIdx.x % LPR;
  const int R = p.B * A;
  const int chunk = (R + P - 1) / P;
  const int r_lo = part * chunk, r_hi = min(R, r_lo + chunk);
  for (int r = r_lo + s; r < r_hi; r += S) {
    const int b = r / A, a = r % A;
    const int64_t row = ((int64_t)b * p.T + t) * A + a;
    float g = p.gchosen[row];
    int64_t act = p.actions[b * p.act_sb + t * p.act_st + a];
    if (act < 0 || act >= NA) {  // (never in a valid batch; keeps the LDS index in bounds)
      act = 0;
      g = 0.f;
    }
    const float4 hv = load4<VEC>(p.h + (((int64_t)b * p.h_ts + t) * A + a) * E, 4 * j, E);
    const float4 w = *reinterpret_cast<const float4*>(&Ws[(int)act * EP + 4 * j]);
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (p.gh_in) o = load4<VEC>(p.gh_in + row * E, 4 * j, E);
    o.x = fmaf(g, w.x, o.x);
    o.y = fmaf(g, w.y, o.y);
    o.z = fmaf(g, w.z, o.z);
    o.w = fmaf(g, w.w, o.w);
    store4<VEC>(p.gh_out + row * E, 4 * j, E, o);
    // this slot's private accumulator: only its LPR lanes touch it, each its own float4
    float4* acc = reinterpret_cast<float4*>(&Gs[(s * NA + (int)act) * EP + 4 * j]);
    float4 c = *acc;
    c.x = fmaf(g, hv.x, c.x);
    c.y = fmaf(g, hv.y, c.y);
    c.z = fmaf(g, hv.z, c.z);
    c.w = fmaf(g, hv.w, c.w);
    *acc = c;
    if (j == 0) Gb[s * NA + (int)act] += g;
  }
  __syncthreads();
  const int NK = NA * (E + 1);
  float* out = p.gpart + ((int64_t)t * P + part) * NK;
  for (int i = threadIdx.x; i < NK; i += blockDim.x) {
    const int n = i / (E + 1), e = i % (E + 1);
    float sum = 0.f;
    for (int k = 0; k < S; ++k) sum += e < E ? Gs[(k * NA + n) * EP + e] : Gb[k * NA + n];
    out[i] = sum;
  }
}

__global__ __launch_bounds__(NOISY_THREADS) void noisy_wgrad_kernel(const float* __restrict__ gpart,
                                                                     const float* __restrict__ eps_w,
                                                                     const float* __restrict__ eps_b,
                                                                     float* __restrict__ du_w, float* __restrict__ du_b,
                                                                     float* __restrict__ ds_w, float* __restrict__ ds_b,
                                                                     int T, int P, int E, int NA) {
  const int NK = NA * (E + 1);
  const int k = blockIdx.x * (NOISY_THREADS / 64) + threadIdx.x / 64, lane = threadIdx.x % 64;
  if (k >= NK) return;  // (whole waves leave together)
  const int n = k / (E + 1), e = k % (E + 1);
  float su = 0.f, ss = 0.f;
  for (int t = lane; t < T; t += 64) {
    float g = 0.f;
    for (int q = 0; q < P; ++q) g += gpart[((int64_t)t * P + q) * NK + k];
    su += g;
    if (eps_w) ss = fmaf(e < E ? eps_w[((int64_t)t * NA + n) * E + e] : eps_b[(int64_t)t * NA + n], g, ss);
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    su += __shfl_xor(su, m, 64);
    ss += __shfl_xor(ss, m, 64);
  }
  if (lane == 0) {
    if (e < E) {
      du_w[n * E + e] += su;
      if (eps_w) ds_w[n * E + e] += ss;
    } else {
      du_b[n] += su;
      if (eps_w) ds_b[n] += ss;
    }
  }
}

bool shape_ok(int B, int A, int E, int NA) {
  return B >= 1 && A >= 1 && A <= NOISY_MAXA && E >= 1 && E <= NOISY_MAXE && NA >= 1 && NA <= NOISY_MAXNA &&
         (int64_t)B * A < (1ll << 31);
}

int lanes_per_row(int E) { return E <= 16 ? 4 : E <= 32 ? 8 : 16; }

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int parts(int B, int A) {
  const int64_t R = (int64_t)B * A;
  const int64_t P = (R + NOISY_PART_ROWS - 1) / NOISY_PART_ROWS;
  return (int)(P < 1 ? 1 : P > NOISY_MAX_PARTS ? NOISY_MAX_PARTS : P);
}

}  // namespace

extern "C" int t2o_noise_normal(const t2o_noise_args* a, void* stream) {
  if (!a || !a->eps_w || !a->eps_b) return T2O_EINVAL;
  if (a->E < 1 || a->NA < 1 || (int64_t)a->NA * (a->E + 1) > 2048 || a->kind < 0 || a->kind > 3) return T2O_EINVAL;
  if (a->counter < 0 || a->counter >= (1ll << 28)) return T2O_EINVAL;
  if (a->t0 < 0 || a->t1 <= a->t0 || a->t1 > a->T || a->T > (1 << 24)) return T2O_EINVAL;
  const uint64_t seedp = a->seed * 4ull + (uint64_t)a->kind;  // mod 2^64
  const int64_t n = (int64_t)(a->t1 - a->t0) * a->NA * (a->E + 1);
  hipLaunchKernelGGL(noise_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a->eps_w,
                     a->eps_b, seedp, a->counter, a->E, a->NA, a->t0, a->t1);
  return (int)hipGetLastError();
}

extern "C" int t2o_noisy_head_fwd(const t2o_noisy_fwd_args* a, void* stream) {
  if (!a || !a->h || !a->u_w || !a->u_b || !a->q) return T2O_EINVAL;
  if ((a->eps_w == nullptr) != (a->eps_b == nullptr)) return T2O_EINVAL;
  if (a->eps_w && (!a->s_w || !a->s_b)) return T2O_EINVAL;
  if (!shape_ok(a->B, a->A, a->E, a->NA)) return T2O_EINVAL;
  if (a->t0 < 0 || a->t1 <= a->t0 || a->t1 > a->h_ts || a->t1 > a->q_ts) return T2O_EINVAL;
  const FwdP p{a->h, a->u_w, a->u_b, a->s_w, a->s_b, a->eps_w, a->eps_b, a->q,
               a->h_ts, a->q_ts, a->B, a->A, a->E, a->NA, a->t0};
  const int lpr = lanes_per_row(a->E), S = NOISY_THREADS / lpr;
  const bool vec = a->E % 4 == 0 && aligned16(a->h);
  const int64_t R = (int64_t)a->B * a->A;
  const int64_t gx = (R + S - 1) / S;
  const dim3 grid((unsigned)(gx > 64 ? 64 : gx), (unsigned)(a->t1 - a->t0)), block(NOISY_THREADS);
  hipStream_t st = (hipStream_t)stream;
#define T2O_NOISY_FWD(L, V) hipLaunchKernelGGL((noisy_fwd_kernel<L, V>), grid, block, 0, st, p)
  if (lpr == 4) {
    if (vec) T2O_NOISY_FWD(4, true); else T2O_NOISY_FWD(4, false);
  } else if (lpr == 8) {
    if (vec) T2O_NOISY_FWD(8, true); else T2O_NOISY_FWD(8, false);
  } else {
    if (vec) T2O_NOISY_FWD(16, true); else T2O_NOISY_FWD(16, false);
  }
#undef T2O_NOISY_FWD
  return (int)hipGetLastError();
}

extern "C" int t2o_noisy_head_parts(int B, int A) {
  if (B < 1 || A < 1 || A > NOISY_MAXA || (int64_t)B * A >= (1ll << 31)) return T2O_EINVAL;
  return parts(B, A);
}

extern "C" int t2o_noisy_head_bwd(const t2o_noisy_bwd_args* a, void* stream) {
  if (!a || !a->gchosen || !a->actions || !a->h || !a->u_w || !a->gh_out || !a->gpart) return T2O_EINVAL;
  if (a->eps_w && !a->s_w) return T2O_EINVAL;
  if (!shape_ok(a->B, a->A, a->E, a->NA) || a->T < 1) return T2O_EINVAL;
  const int t_hi = a->t_hi <= 0 ? a->T : a->t_hi;
  if (a->t_lo < 0 || t_hi <= a->t_lo || t_hi > a->T || a->T > a->h_ts) return T2O_EINVAL;
  const BwdP p{a->gchosen, a->actions, a->act_sb, a->act_st, a->h, a->u_w, a->s_w, a->eps_w, a->gh_in,
               a->gh_out, a->gpart, a->h_ts, a->B, a->T, a->A, a->E, a->NA, a->t_lo};
  const int lpr = lanes_per_row(a->E), EP = lpr * 4;
  // the workgroup size depends on the shape only (never on the step range): 256 threads,
  // halved until the row slots' private accumulators fit 64 KB of LDS
  int threads = NOISY_THREADS;
  auto lds = [&](int th) { return (size_t)(a->NA * EP + (th / lpr) * a->NA * (EP + 1)) * sizeof(float); };
  while (threads > 64 && lds(threads) > 60 * 1024) threads /= 2;
  const bool vec = a->E % 4 == 0 && aligned16(a->h) && aligned16(a->gh_out) && aligned16(a->gh_in);
  const dim3 grid((unsigned)(t_hi - a->t_lo), (unsigned)parts(a->B, a->A)), block(threads);
  hipStream_t st = (hipStream_t)stream;
#define T2O_NOISY_BWD(L, V) hipLaunchKernelGGL((noisy_bwd_kernel<L, V>), grid, block, lds(threads), st, p)
  if (lpr == 4) {
    if (vec) T2O_NOISY_BWD(4, true); else T2O_NOISY_BWD(4, false);
  } else if (lpr == 8) {
    if (vec) T2O_NOISY_BWD(8, true); else T2O_NOISY_BWD(8, false);
  } else {
    if (vec) T2O_NOISY_BWD(16, true); else T2O_NOISY_BWD(16, false);
  }
#undef T2O_NOISY_BWD
  return (int)hipGetLastError();
}

extern "C" int t2o_noisy_head_wgrad(const t2o_noisy_wgrad_args* a, void* stream) {
  if (!a || !a->gpart || !a->du_w || !a->du_b) return T2O_EINVAL;
  if ((a->eps_w == nullptr) != (a->eps_b == nullptr)) return T2O_EINVAL;
  if (a->eps_w && (!a->ds_w || !a->ds_b)) return T2O_EINVAL;
  if (!shape_ok(a->B, a->A, a->E, a->NA) || a->T < 1) return T2O_EINVAL;
  const int NK = a->NA * (a->E + 1), per = NOISY_THREADS / 64;
  hipLaunchKernelGGL(noisy_wgrad_kernel, dim3((unsigned)((NK + per - 1) / per)), dim3(NOISY_THREADS), 0,
                     (hipStream_t)stream, a->gpart, a->eps_w, a->eps_b, a->du_w, a->du_b, a->ds_w, a->ds_b, a->T,
                     parts(a->B, a->A), a->E, a->NA);
  return (int)hipGetLastError();
}
