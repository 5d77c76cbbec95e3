// t2o_rnn.hip — the GRU agent of the QMIX baselines (agent: rnn).
//
// No agent but the transformer ships with the reference, so this is the project's
// DECLARED definition after PyMARL2's modules/agents/n_rnn_agent.RNNAgent with
// use_layer_norm = False (parity-unpinned; DESIGN.md §5, restated in fp64 in
// tests/rnn_model.py).  Per agent row and step, gates in torch.nn.GRUCell's order:
//
//   x  = relu(fc1 · in + b1)
//   r  = σ(W_ir x + b_ir + W_hr h + b_hr)       z = σ(W_iz x + b_iz + W_hz h + b_hz)
//   n  = tanh(W_in x + b_in + r ⊙ (W_hn h + b_hn))
//   h' = (1 − z) ⊙ n + z ⊙ h                    q = fc2 · h' + b2
//
// in = [obs ; onehot(action at t−1) ; onehot(agent)] (BasicMAC._build_inputs; either
// one-hot optional).  No input matrix is materialised: the forward adds the one-hots'
// fc1 columns to the pre-activation, the weight gradient builds the columns it needs.
//
// Parameters are read straight from the flat buffer in registration order (fc1.weight,
// fc1.bias, rnn.weight_ih, rnn.weight_hh, rnn.bias_ih, rnn.bias_hh, fc2.weight,
// fc2.bias).  All arithmetic is fp32 on v_mfma_f32_16x16x4_f32 in the T-layout of
// t2o_common.hpp (lane (g, c): row c, features 16t + 4g + r), operands placed as in
// t2o_qmix.hip.
//
//   in kernel     time-parallel, rows (b, t, a), one wave per 16-row tile, grid.y the
//                 network: x [rows][H] and gi = W_ih x + b_ih [rows][3H].
//   rec kernel    one wave (one workgroup) per tile of 16 (b, a) sequences; W_hh and
//                 fc2 staged in LDS (rows padded by 4 floats against bank conflicts);
//                 loops over t: gh = W_hh h + b_hh, the gates, h', q.
//   bptt kernel   the reverse loop of one network: recomputes the gates from gi,
//                 h_{t-1} and W_hh, leaves per row [dr, dz, dn, dn ⊙ r] (the gradients
//                 of gi, and of gh's n gate) in the work buffer; W_hhᵀ is read from
//                 the same LDS copy (matvec_t's scalar reads).
//   dx kernel     time-parallel: dpre = (W_ihᵀ dgi) ⊙ [x > 0] into the work row.
//   dw kernel     the weight gradients Σ_rows P[row][o] Q[row][k], one 16-output tile
//                 against up to RN_KG 16-column tiles per task; four waves' accumulators
//                 are summed through LDS in wave order and every element of the
//                 workgroup's slab is written exactly once: a fixed order, no atomics.
//                 t2o_reduce_slabs sums the slabs.
#include "t2o_common.hpp"

namespace {

using namespace t2o;

constexpr int RN_THREADS = 256, RN_WAVES = 4;
constexpr int RN_MAXA = 64, RN_MAXNA = 16, RN_MAX_SLABS = 64, RN_SLAB_TILES = 8;
constexpr int RN_MAXIN = 9 * RN_MAXA + RN_MAXNA + RN_MAXA;  // the widest built input
constexpr int RN_KG = 8;   // k tiles of one dw task
constexpr int RN_PAD = 4;  // LDS row padding (floats)

struct ROff {
  int64_t W1, b1, Wih, Whh, bih, bhh, W2, b2, total;
};

__host__ __device__ inline ROff roff(int IN, int H, int NA) {
  ROff o;
  int64_t p = 0;
  o.W1 = p, p += (int64_t)H * IN;
  o.b1 = p, p += H;
  o.Wih = p, p += (int64_t)3 * H * H;
  o.Whh = p, p += (int64_t)3 * H * H;
  o.bih = p, p += 3 * H;
  o.bhh = p, p += 3 * H;
  o.W2 = p, p += (int64_t)NA * H;
  o.b2 = p, p += NA;
  o.total = p;
  return o;
}

// how a row's input vector is built
struct InP {
  const float* obs;
  int64_t obs_sb, obs_st;
  const int64_t* actions;
  int64_t act_sb, act_st;
  int A, OBS, NA, IN, la, id, shift;
};

// the action whose one-hot row (b, t, a) carries, -1 for none
T2O_DEV int last_action(const InP& p, int b, int t, int a) {
  const int tt = t - 1 + p.shift;
  if (!p.la || !p.actions || tt < 0) return -1;
  const int64_t v = p.actions[b * p.act_sb + tt * p.act_st + a];
  return v < 0 || v >= p.NA ? -1 : (int)v;
}

// element k < IN of the input of row (b, t, a)
T2O_DEV float in_val(const InP& p, int b, int t, int a, int k) {
  if (k < p.OBS) return p.obs[b * p.obs_sb + t * p.obs_st + (int64_t)a * p.OBS + k];
  k -= p.OBS;
  if (p.la) {
    if (k < p.NA) return last_action(p, b, t, a) == k ? 1.f : 0.f;
    k -= p.NA;
  }
  return k == a ? 1.f : 0.f;
}

template <bool VEC>
T2O_DEV f4 ldw4(const float* p) {
  if (VEC) return ld4(p);
  return f4{p[0], p[1], p[2], p[3]};
}

T2O_DEV float sigmoidf(float x) { return 1.f / (1.f + expf(-x)); }

T2O_DEV f4 bias4(const float* __restrict__ b, int t) {
  const int g = lane_g();
  return f4{b[16 * t + 4 * g], b[16 * t + 4 * g + 1], b[16 * t + 4 * g + 2], b[16 * t + 4 * g + 3]};
}

// ---------------------------------------------------------------------------
// in kernel
struct InKP {
  InP in;
  const float* params[2];
  float* x[2];
  float* gi[2];
  int B, T1, t0, t1, H;
};

template <int HT, bool VEC>
__global__ __launch_bounds__(RN_THREADS) void rnn_in_kernel(InKP p) {
  constexpr int H = 16 * HT;
  const int net = blockIdx.y;
  const int Tn = p.t1 - p.t0, A = p.in.A, OBS = p.in.OBS, IN = p.in.IN;
  const int64_t R = (int64_t)p.B * Tn * A;
  const int64_t row0 = ((int64_t)blockIdx.x * RN_WAVES + wave_id()) * 16;
  if (row0 >= R) return;  // (whole waves leave; no workgroup barrier below)
  const int c = lane_c(), g = lane_g();
  const int64_t r = row0 + c;
  const bool live = r < R;
  const int64_t rr = live ? r : R - 1;  // padding rows read the last row
  const int a = (int)(rr % A);
  const int64_t bt = rr / A;
  const int t = p.t0 + (int)(bt % Tn), b = (int)(bt / Tn);
  const int64_t row = ((int64_t)b * p.T1 + t) * A + a;
  const ROff o = roff(IN, H, p.in.NA);
  const float* P = p.params[net];
  const float* W1 = P + o.W1;
  // fc1: the bias, the one-hots' columns, then the observation on the MFMA
  const int act = last_action(p.in, b, t, a);
  const int idc = p.in.id ? OBS + (p.in.la ? p.in.NA : 0) + a : -1;
  f4 x[HT];
#pragma unroll
  for (int j = 0; j < HT; ++j) {
    x[j] = bias4(P + o.b1, j);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float* w = W1 + (int64_t)(16 * j + 4 * g + q) * IN;
      if (act >= 0) x[j][q] += w[OBS + act];
      if (idc >= 0) x[j][q] += w[idc];
    }
  }
  const float* ob = p.in.obs + b * p.in.obs_sb + t * p.in.obs_st + (int64_t)a * OBS;
  for (int k0 = 0; k0 < OBS; k0 += 16) {
    f4 v;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int k = k0 + 4 * g + s;
      const float u = ob[min(k, OBS - 1)];
      v[s] = k < OBS ? u : 0.f;
    }
#pragma unroll
    for (int j = 0; j < HT; ++j) {
      const float* w = W1 + (int64_t)(16 * j + c) * IN;
#pragma unroll
      for (int s = 0; s < 4; ++s) x[j] = mfma4(w[min(k0 + 4 * g + s, OBS - 1)], v[s], x[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < HT; ++j)
#pragma unroll
    for (int q = 0; q < 4; ++q) x[j][q] = fmaxf(x[j][q], 0.f);
  if (p.x[net] && live) {
#pragma unroll
    for (int j = 0; j < HT; ++j) st4(p.x[net] + row * H + 16 * j + 4 * g, x[j]);
  }
  // gi = W_ih x + b_ih
  const float* Wih = P + o.Wih;
  float* gi = p.gi[net] + row * 3 * H;
#pragma unroll
  for (int j = 0; j < 3 * HT; ++j) {
    f4 acc = bias4(P + o.bih, j);
    const float* w = Wih + (int64_t)(16 * j + c) * H + 4 * g;
#pragma unroll
    for (int i = 0; i < HT; ++i) {
      const f4 wf = ldw4<VEC>(w + 16 * i);
#pragma unroll
      for (int s = 0; s < 4; ++s) acc = mfma4(wf[s], x[i][s], acc);
    }
    if (live) st4(gi + 16 * j + 4 * g, acc);
  }
}

// ---------------------------------------------------------------------------
// the recurrence
struct RecP {
  const float* params[2];
  const float* h0[2];
  int64_t h0_sb;
  const float* gi[2];
  float* h[2];
  float* q[2];
  int B, T1, t0, t1, A, NA, IN;
};

// W_hh [3H][H] and fc2 (rows past NA zero) into LDS with rows of H + RN_PAD floats
template <int H>
T2O_DEV void stage_rec_weights(float* lw, float* lf, const float* __restrict__ P, const ROff& o, int NA) {
  constexpr int LD = H + RN_PAD;
  for (int i = threadIdx.x; i < 3 * H * H; i += blockDim.x) lw[(i / H) * LD + i % H] = P[o.Whh + i];
  for (int i = threadIdx.x; i < 16 * H; i += blockDim.x) lf[(i / H) * LD + i % H] = i / H < NA ? P[o.W2 + i] : 0.f;
  __syncthreads();
}

// the three gate pre-activations of gh for feature tile j: W_hh[gate·H + 16j + c][:] · h + b_hh
template <int HT>
T2O_DEV void gh_tile(const float* lw, const f4* bhh, int j, const f4* h, f4& ar, f4& az, f4& an) {
  constexpr int H = 16 * HT, LD = H + RN_PAD;
  const int c = lane_c(), g = lane_g();
  ar = bhh[j], az = bhh[HT + j], an = bhh[2 * HT + j];
  const float* w = lw + (16 * j + c) * LD + 4 * g;
#pragma unroll
  for (int i = 0; i < HT; ++i) {
    const f4 wr = ld4(w + 16 * i), wz = ld4(w + H * LD + 16 * i), wn = ld4(w + 2 * H * LD + 16 * i);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      ar = mfma4(wr[s], h[i][s], ar);
      az = mfma4(wz[s], h[i][s], az);
      an = mfma4(wn[s], h[i][s], an);
    }
  }
}

template <int HT>
__global__ __launch_bounds__(64) void rnn_rec_kernel(RecP p) {
  constexpr int H = 16 * HT, LD = H + RN_PAD;
  __shared__ __attribute__((aligned(16))) float lw[3 * H * LD];
  __shared__ __attribute__((aligned(16))) float lf[16 * LD];
  const int net = blockIdx.y;
  const int A = p.A, NA = p.NA;
  const ROff o = roff(p.IN, H, NA);
  const float* P = p.params[net];
  stage_rec_weights<H>(lw, lf, P, o, NA);
  const int c = lane_c(), g = lane_g();
  const int64_t N = (int64_t)p.B * A;
  const int64_t n = (int64_t)blockIdx.x * 16 + c;
  const bool live = n < N;
  const int64_t nn = live ? n : N - 1;  // padding sequences repeat the last one
  const int b = (int)(nn / A), a = (int)(nn % A);
  f4 bhh[3 * HT], h[HT], b2;
#pragma unroll
  for (int j = 0; j < 3 * HT; ++j) bhh[j] = bias4(P + o.bhh, j);
#pragma unroll
  for (int q = 0; q < 4; ++q) b2[q] = P[o.b2 + min(4 * g + q, NA - 1)];
  const float* h0 = p.h0[net];
#pragma unroll
  for (int j = 0; j < HT; ++j) h[j] = h0 ? ld4(h0 + b * p.h0_sb + (int64_t)a * H + 16 * j + 4 * g) : zero4();
  for (int t = p.t0; t < p.t1; ++t) {
    const int64_t row = ((int64_t)b * p.T1 + t) * A + a;
    const float* gi = p.gi[net] + row * 3 * H + 4 * g;
    f4 hn[HT];
#pragma unroll
    for (int j = 0; j < HT; ++j) {
      T2O_FENCE();  // one tile's weight fragments live at a time
      f4 ar, az, an;
      gh_tile<HT>(lw, bhh, j, h, ar, az, an);
      const f4 gr = ld4(gi + 16 * j), gz = ld4(gi + H + 16 * j), gn = ld4(gi + 2 * H + 16 * j);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float r = sigmoidf(gr[q] + ar[q]), z = sigmoidf(gz[q] + az[q]);
        const float nv = tanhf(gn[q] + r * an[q]);
        hn[j][q] = (1.f - z) * nv + z * h[j][q];
      }
    }
    f4 qa = b2;
#pragma unroll
    for (int i = 0; i < HT; ++i) {
      h[i] = hn[i];
      const f4 wf = ld4(lf + c * LD + 16 * i + 4 * g);
#pragma unroll
      for (int s = 0; s < 4; ++s) qa = mfma4(wf[s], h[i][s], qa);
    }
    if (live) {
#pragma unroll
      for (int j = 0; j < HT; ++j) st4(p.h[net] + row * H + 16 * j + 4 * g, h[j]);
      float* qo = p.q[net] + row * NA;
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (4 * g + q < NA) qo[4 * g + q] = qa[q];
    }
  }
}

// ---------------------------------------------------------------------------
// backward
struct BwdP {
  InP in;
  const float* params;
  const float* h0;
  int64_t h0_sb;
  const float *x, *gi, *h;  // the forward's, rows (b·Ts + t)·A + a
  const float* gchosen;     // [B][T][A] with in.actions at t, or
  const float* gq;          // [B][T][A][NA]
  int64_t ch_sb, ch_st;     // strides of the chosen actions (in.actions' base, unshifted)
  const float* gh;          // [B][T][A][H] or null
  float* gh0;
  float* work;              // rows (b·T + t)·A + a of 5H floats: dr, dz, dn, dn ⊙ r, dpre
  float* slabs;
  int64_t ntiles;
  int B, T, Ts, H, tps;
};

T2O_DEV int chosen_action(const BwdP& p, int b, int t, int a) {
  const int64_t v = p.in.actions[b * p.ch_sb + t * p.ch_st + a];
  return v < 0 ? 0 : v >= p.in.NA ? p.in.NA - 1 : (int)v;  // (never in a valid batch; keeps the load in bounds)
}

template <int HT>
__global__ __launch_bounds__(64) void rnn_bptt_kernel(BwdP p) {
  constexpr int H = 16 * HT, LD = H + RN_PAD, WS = 5 * H;
  __shared__ __attribute__((aligned(16))) float lw[3 * H * LD];
  __shared__ __attribute__((aligned(16))) float lf[16 * LD];
  const int A = p.in.A, NA = p.in.NA;
  const ROff o = roff(p.in.IN, H, NA);
  const float* P = p.params;
  stage_rec_weights<H>(lw, lf, P, o, NA);
  const int c = lane_c(), g = lane_g();
  const int64_t N = (int64_t)p.B * A;
  const int64_t n = (int64_t)blockIdx.x * 16 + c;
  const bool live = n < N;
  const int64_t nn = live ? n : N - 1;
  const int b = (int)(nn / A), a = (int)(nn % A);
  f4 bhh[3 * HT], carry[HT];
#pragma unroll
  for (int j = 0; j < 3 * HT; ++j) bhh[j] = bias4(P + o.bhh, j);
#pragma unroll
  for (int j = 0; j < HT; ++j) carry[j] = zero4();
  for (int t = p.T - 1; t >= 0; --t) {
    const int64_t frow = ((int64_t)b * p.Ts + t) * A + a, wrow = ((int64_t)b * p.T + t) * A + a;
    f4 hp[HT], dh[HT];
#pragma unroll
    for (int j = 0; j < HT; ++j) {
      if (t > 0) hp[j] = ld4(p.h + (frow - A) * H + 16 * j + 4 * g);
      else hp[j] = p.h0 ? ld4(p.h0 + b * p.h0_sb + (int64_t)a * H + 16 * j + 4 * g) : zero4();
      dh[j] = carry[j];
      if (p.gh) dh[j] += ld4(p.gh + wrow * H + 16 * j + 4 * g);
    }
    if (p.gchosen) {
      const float gc = p.gchosen[wrow];
      const float* f = lf + chosen_action(p, b, t, a) * LD + 4 * g;
#pragma unroll
      for (int j = 0; j < HT; ++j) dh[j] += gc * ld4(f + 16 * j);
    }
    if (p.gq) {
      for (int k = 0; k < NA; ++k) {
        const float gk = p.gq[wrow * NA + k];
        const float* f = lf + k * LD + 4 * g;
#pragma unroll
        for (int j = 0; j < HT; ++j) dh[j] += gk * ld4(f + 16 * j);
      }
    }
    const float* gi = p.gi + frow * 3 * H + 4 * g;
    float* wk = p.work + wrow * WS + 4 * g;
    f4 dgh[3 * HT];
#pragma unroll
    for (int j = 0; j < HT; ++j) {
      T2O_FENCE();  // one tile's weight fragments live at a time
      f4 ar, az, an;
      gh_tile<HT>(lw, bhh, j, hp, ar, az, an);
      const f4 gr = ld4(gi + 16 * j), gz = ld4(gi + H + 16 * j), gn = ld4(gi + 2 * H + 16 * j);
      f4 dni;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float r = sigmoidf(gr[q] + ar[q]), z = sigmoidf(gz[q] + az[q]);
        const float nv = tanhf(gn[q] + r * an[q]);
        const float d = dh[j][q];
        const float dpn = d * (1.f - z) * (1.f - nv * nv);
        const float dpz = d * (hp[j][q] - nv) * z * (1.f - z);
        const float dpr = dpn * an[q] * r * (1.f - r);
        dgh[j][q] = dpr, dgh[HT + j][q] = dpz, dgh[2 * HT + j][q] = dpn * r;
        dni[q] = dpn;
        carry[j][q] = d * z;
      }
      if (live) {
        st4(wk + 16 * j, dgh[j]);
        st4(wk + H + 16 * j, dgh[HT + j]);
        st4(wk + 2 * H + 16 * j, dni);
        st4(wk + 3 * H + 16 * j, dgh[2 * HT + j]);
      }
    }
    // carry += W_hhᵀ dgh
#pragma unroll
    for (int jo = 0; jo < HT; ++jo) {
      f4 acc = carry[jo];
#pragma unroll
      for (int i = 0; i < 3 * HT; ++i) {
        T2O_FENCE();
#pragma unroll
        for (int s = 0; s < 4; ++s) acc = mfma4(lw[(16 * i + 4 * g + s) * LD + 16 * jo + c], dgh[i][s], acc);
      }
      carry[jo] = acc;
    }
  }
  if (p.gh0 && live) {
#pragma unroll
    for (int j = 0; j < HT; ++j) st4(p.gh0 + nn * H + 16 * j + 4 * g, carry[j]);
  }
}

// dpre = (W_ihᵀ dgi) ⊙ [x > 0], rows (b, t < T, a)
template <int HT>
__global__ __launch_bounds__(RN_THREADS) void rnn_dx_kernel(BwdP p) {
  constexpr int H = 16 * HT, WS = 5 * H;
  const int A = p.in.A;
  const int64_t R = (int64_t)p.B * p.T * A;
  const int64_t row0 = ((int64_t)blockIdx.x * RN_WAVES + wave_id()) * 16;
  if (row0 >= R) return;
  const int c = lane_c(), g = lane_g();
  const int64_t r = row0 + c;
  const bool live = r < R;
  const int64_t rr = live ? r : R - 1;
  const int64_t bt = rr / A;
  const int64_t frow = ((bt / p.T) * p.Ts + bt % p.T) * A + rr % A;
  const float* Wih = p.params + roff(p.in.IN, H, p.in.NA).Wih;
  float* wk = p.work + rr * WS + 4 * g;
  f4 gx[HT];
#pragma unroll
  for (int i = 0; i < HT; ++i) gx[i] = zero4();
  for (int j = 0; j < 3 * HT; ++j) {
    const f4 gv = ld4(wk + 16 * j);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const float* w = Wih + (int64_t)(16 * j + 4 * g + s) * H + c;
#pragma unroll
      for (int i = 0; i < HT; ++i) gx[i] = mfma4(w[16 * i], gv[s], gx[i]);
    }
  }
  if (live) {
#pragma unroll
    for (int i = 0; i < HT; ++i) {
      const f4 xv = ld4(p.x + frow * H + 16 * i + 4 * g);
      f4 d;
#pragma unroll
      for (int q = 0; q < 4; ++q) d[q] = xv[q] > 0.f ? gx[i][q] : 0.f;
      st4(wk + 4 * H + 16 * i, d);
    }
  }
}

// one task: a 16-row tile of outputs against up to RN_KG 16-column tiles of k
struct DwTask {
  int pkind, pcol, no;  // P: 0 a work column / 1 the Q gradient scattered to its action; valid outputs
  int qkind;            // Q: 0 x, 1 h_{t-1}, 2 the input, 3 h_t
  int nk, k0;           // Q's width, the task's first column
  int64_t wdst, bdst;   // slab offsets of W[o0][0] and its bias (-1: another task writes it)
};

__host__ __device__ inline int dw_tasks(int IN, int H) {
  const int KGn = ((IN + 15) / 16 + RN_KG - 1) / RN_KG;
  return 6 * (H / 16) + (H / 16) * KGn + 1;
}

__device__ inline DwTask dw_task(int y, const ROff& o, int IN, int H, int NA) {
  const int HT = H / 16, KGn = ((IN + 15) / 16 + RN_KG - 1) / RN_KG;
  if (y < 3 * HT) return DwTask{0, 16 * y, 16, 0, H, 0, o.Wih + (int64_t)16 * y * H, o.bih + 16 * y};
  y -= 3 * HT;
  if (y < 3 * HT)  // dgh: dr, dz, then dn ⊙ r
    return DwTask{0, y < 2 * HT ? 16 * y : 16 * y + H, 16, 1, H, 0, o.Whh + (int64_t)16 * y * H, o.bhh + 16 * y};
  y -= 3 * HT;
  if (y < HT * KGn) {
    const int ot = y / KGn, kg = y % KGn;
    return DwTask{0, 4 * H + 16 * ot, 16, 2, IN, kg * RN_KG * 16, o.W1 + (int64_t)16 * ot * IN,
                  kg == 0 ? o.b1 + 16 * ot : -1};
  }
  return DwTask{1, 0, NA, 3, H, 0, o.W2, o.b2};
}

__global__ __launch_bounds__(RN_THREADS) void rnn_dw_kernel(BwdP p) {
  constexpr int NACC = RN_KG + 1;
  __shared__ f4 red[RN_WAVES * NACC * 64];
  const int slab = blockIdx.x, wv = wave_id();
  const int c = lane_c(), g = lane_g(), lane = threadIdx.x & 63;
  const int A = p.in.A, NA = p.in.NA, IN = p.in.IN, H = p.H, WS = 5 * H;
  const ROff o = roff(IN, H, NA);
  const DwTask t = dw_task(blockIdx.y, o, IN, H, NA);
  const int ldw = t.qkind == 2 ? IN : H;
  const int nkt = min(RN_KG, (t.nk - t.k0 + 15) / 16);
  const int64_t R = (int64_t)p.B * p.T * A;
  f4 acc[NACC];
#pragma unroll
  for (int j = 0; j < NACC; ++j) acc[j] = zero4();
  const int64_t lo = (int64_t)slab * p.tps, hi = min(lo + p.tps, p.ntiles);
  for (int64_t tile = lo + wv; tile < hi; tile += RN_WAVES) {
    const int64_t row0 = tile * 16;
    f4 pa;
    int bb[4], tt[4], aa[4];
    int64_t fr[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int64_t row = row0 + 4 * g + s;
      const bool live = row < R;
      const int64_t rr = live ? row : R - 1;  // (padding rows: P is 0 there)
      const int64_t bt = rr / A;
      aa[s] = (int)(rr % A), tt[s] = (int)(bt % p.T), bb[s] = (int)(bt / p.T);
      fr[s] = ((int64_t)bb[s] * p.Ts + tt[s]) * A + aa[s];
      float v;
      if (t.pkind == 0) v = p.work[rr * WS + t.pcol + c];
      else if (p.gq) v = p.gq[rr * NA + min(c, NA - 1)];
      else v = chosen_action(p, bb[s], tt[s], aa[s]) == c ? p.gchosen[rr] : 0.f;
      pa[s] = live && c < t.no ? v : 0.f;
    }
#pragma unroll
    for (int j = 0; j < RN_KG; ++j) {
      if (j < nkt) {
        const int k = t.k0 + 16 * j + c, kk = min(k, t.nk - 1);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          float v;
          if (t.qkind == 0) v = p.x[fr[s] * H + kk];
          else if (t.qkind == 3) v = p.h[fr[s] * H + kk];
          else if (t.qkind == 2) v = in_val(p.in, bb[s], tt[s], aa[s], kk);
          else if (tt[s] > 0) v = p.h[(fr[s] - A) * H + kk];
          else v = p.h0 ? p.h0[bb[s] * p.h0_sb + (int64_t)aa[s] * H + kk] : 0.f;
          acc[j] = mfma4(pa[s], k < t.nk ? v : 0.f, acc[j]);
        }
      }
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) acc[RN_KG] = mfma4(pa[s], 1.f, acc[RN_KG]);
  }
#pragma unroll
  for (int j = 0; j < NACC; ++j) red[(wv * NACC + j) * 64 + lane] = acc[j];
  __syncthreads();
  float* out = p.slabs + (int64_t)slab * o.total;
  for (int idx = threadIdx.x; idx < NACC * 64; idx += RN_THREADS) {
    const int j = idx / 64, l = idx % 64, lc = l & 15, lg = l >> 4;
    f4 v = red[j * 64 + l];
#pragma unroll
    for (int w = 1; w < RN_WAVES; ++w) v += red[(w * NACC + j) * 64 + l];
    if (j < RN_KG) {
      const int k = t.k0 + 16 * j + lc;
      if (j < nkt && k < t.nk) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (4 * lg + r < t.no) out[t.wdst + (int64_t)(4 * lg + r) * ldw + k] = v[r];
      }
    } else if (lc == 0 && t.bdst >= 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (4 * lg + r < t.no) out[t.bdst + 4 * lg + r] = v[r];
    }
  }
}

// ---------------------------------------------------------------------------
bool dims_ok(int A, int OBS, int NA, int H) {
  return A >= 1 && A <= RN_MAXA && OBS >= 1 && OBS <= RN_MAXIN && NA >= 1 && NA <= RN_MAXNA && (H == 32 || H == 64);
}

bool rows_ok(int B, int T, int A) { return B >= 1 && T >= 1 && A >= 1 && (int64_t)B * T * A < (1ll << 27); }

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int in_width(int OBS, int NA, int A, int la, int id) { return OBS + (la ? NA : 0) + (id ? A : 0); }

int slabs_of(int B, int T, int A) {
  const int64_t ntiles = ((int64_t)B * T * A + 15) / 16;
  const int64_t n = ntiles / RN_SLAB_TILES;
  return (int)(n < 1 ? 1 : n > RN_MAX_SLABS ? RN_MAX_SLABS : n);
}

}  // namespace

extern "C" int64_t t2o_rnn_param_count(int IN, int H, int NA) {
  if (IN < 1 || IN > RN_MAXIN || NA < 1 || NA > RN_MAXNA || (H != 32 && H != 64))
    return T2O_EINVAL;
  return roff(IN, H, NA).total;
}

extern "C" int t2o_rnn_fwd(const t2o_rnn_fwd_args* a, void* stream) {
  if (!a || !a->params_on || !a->obs || !a->gi_on || !a->q_on || !a->h_on) return T2O_EINVAL;
  if (!dims_ok(a->A, a->OBS, a->NA, a->H) || !rows_ok(a->B, a->T1, a->A)) return T2O_EINVAL;
  if (a->t0 < 0 || a->t1 <= a->t0 || a->t1 > a->T1) return T2O_EINVAL;
  const bool two = a->params_tg != nullptr;
  if (two && (!a->gi_tg || !a->q_tg || !a->h_tg)) return T2O_EINVAL;
  const float* outs[] = {a->x_on, a->gi_on, a->h_on, a->gi_tg, a->h_tg, a->h0_on, a->h0_tg};
  for (const float* q : outs)
    if (!aligned16(q)) return T2O_EINVAL;
  if ((a->h0_on || a->h0_tg) && a->h0_sb % 4) return T2O_EINVAL;
  const int IN = in_width(a->OBS, a->NA, a->A, a->last_action, a->agent_id);
  if (IN > RN_MAXIN) return T2O_EINVAL;
  InKP k{};
  k.in = InP{a->obs, a->obs_sb, a->obs_st, a->actions, a->act_sb, a->act_st, a->A, a->OBS, a->NA, IN,
             a->last_action ? 1 : 0, a->agent_id ? 1 : 0, a->act_shift};
  k.params[0] = a->params_on, k.params[1] = a->params_tg;
  k.x[0] = a->x_on, k.x[1] = nullptr;
  k.gi[0] = a->gi_on, k.gi[1] = a->gi_tg;
  k.B = a->B, k.T1 = a->T1, k.t0 = a->t0, k.t1 = a->t1, k.H = a->H;
  hipStream_t st = (hipStream_t)stream;
  const int64_t ntiles = ((int64_t)a->B * (a->t1 - a->t0) * a->A + 15) / 16;
  const dim3 grid((unsigned)((ntiles + RN_WAVES - 1) / RN_WAVES), two ? 2 : 1);
  const bool vec = aligned16(a->params_on) && (!two || aligned16(a->params_tg));
  if (a->H == 64) {
    if (vec) hipLaunchKernelGGL((rnn_in_kernel<4, true>), grid, dim3(RN_THREADS), 0, st, k);
    else hipLaunchKernelGGL((rnn_in_kernel<4, false>), grid, dim3(RN_THREADS), 0, st, k);
  } else {
    if (vec) hipLaunchKernelGGL((rnn_in_kernel<2, true>), grid, dim3(RN_THREADS), 0, st, k);
    else hipLaunchKernelGGL((rnn_in_kernel<2, false>), grid, dim3(RN_THREADS), 0, st, k);
  }
  RecP r{};
  r.params[0] = a->params_on, r.params[1] = a->params_tg;
  r.h0[0] = a->h0_on, r.h0[1] = a->h0_tg, r.h0_sb = a->h0_sb;
  r.gi[0] = a->gi_on, r.gi[1] = a->gi_tg;
  r.h[0] = a->h_on, r.h[1] = a->h_tg;
  r.q[0] = a->q_on, r.q[1] = a->q_tg;
  r.B = a->B, r.T1 = a->T1, r.t0 = a->t0, r.t1 = a->t1, r.A = a->A, r.NA = a->NA, r.IN = IN;
  const dim3 rgrid((unsigned)(((int64_t)a->B * a->A + 15) / 16), two ? 2 : 1);
  if (a->H == 64) hipLaunchKernelGGL((rnn_rec_kernel<4>), rgrid, dim3(64), 0, st, r);
  else hipLaunchKernelGGL((rnn_rec_kernel<2>), rgrid, dim3(64), 0, st, r);
  return (int)hipGetLastError();
}

extern "C" int t2o_rnn_bwd_slabs(int B, int T, int A) {
  if (!rows_ok(B, T, A)) return T2O_EINVAL;
  return slabs_of(B, T, A);
}

extern "C" int64_t t2o_rnn_bwd_work_floats(int B, int T, int A, int H) {
  if (!rows_ok(B, T, A) || (H != 32 && H != 64)) return T2O_EINVAL;
  return (int64_t)B * T * A * 5 * H;
}

extern "C" int t2o_rnn_bwd(const t2o_rnn_bwd_args* a, void* stream) {
  if (!a || !a->params || !a->obs || !a->x || !a->gi || !a->h || !a->work || !a->gslabs) return T2O_EINVAL;
  if (!dims_ok(a->A, a->OBS, a->NA, a->H) || a->T > a->Ts || !rows_ok(a->B, a->Ts, a->A) || a->T < 1)
    return T2O_EINVAL;
  if ((a->gchosen != nullptr) == (a->gq != nullptr)) return T2O_EINVAL;  // exactly one form of dL/dq
  if (a->gchosen && !a->actions) return T2O_EINVAL;
  const float* al[] = {a->x, a->gi, a->h, a->h0, a->gh, a->gh0, a->work};
  for (const float* q : al)
    if (!aligned16(q)) return T2O_EINVAL;
  if (a->h0 && a->h0_sb % 4) return T2O_EINVAL;
  if (a->work_floats < t2o_rnn_bwd_work_floats(a->B, a->T, a->A, a->H)) return T2O_EINVAL;
  const int nslab = slabs_of(a->B, a->T, a->A);
  if (a->max_slabs < nslab) return T2O_EINVAL;
  const int IN = in_width(a->OBS, a->NA, a->A, a->last_action, a->agent_id);
  if (IN > RN_MAXIN) return T2O_EINVAL;
  const int64_t R = (int64_t)a->B * a->T * a->A, ntiles = (R + 15) / 16;
  BwdP p{};
  p.in = InP{a->obs, a->obs_sb, a->obs_st, a->actions, a->act_sb, a->act_st, a->A, a->OBS, a->NA, IN,
             a->last_action ? 1 : 0, a->agent_id ? 1 : 0, a->act_shift};
  p.params = a->params, p.h0 = a->h0, p.h0_sb = a->h0_sb;
  p.x = a->x, p.gi = a->gi, p.h = a->h;
  p.gchosen = a->gchosen, p.gq = a->gq, p.ch_sb = a->act_sb, p.ch_st = a->act_st;
  p.gh = a->gh, p.gh0 = a->gh0, p.work = a->work, p.slabs = a->gslabs;
  p.ntiles = ntiles, p.B = a->B, p.T = a->T, p.Ts = a->Ts, p.H = a->H;
  p.tps = (int)((ntiles + nslab - 1) / nslab);
  hipStream_t st = (hipStream_t)stream;
  const dim3 sgrid((unsigned)(((int64_t)a->B * a->A + 15) / 16));
  const dim3 rgrid((unsigned)((ntiles + RN_WAVES - 1) / RN_WAVES));
  if (a->H == 64) {
    hipLaunchKernelGGL((rnn_bptt_kernel<4>), sgrid, dim3(64), 0, st, p);
    hipLaunchKernelGGL((rnn_dx_kernel<4>), rgrid, dim3(RN_THREADS), 0, st, p);
  } else {
    hipLaunchKernelGGL((rnn_bptt_kernel<2>), sgrid, dim3(64), 0, st, p);
    hipLaunchKernelGGL((rnn_dx_kernel<2>), rgrid, dim3(RN_THREADS), 0, st, p);
  }
  hipLaunchKernelGGL(rnn_dw_kernel, dim3((unsigned)nslab, (unsigned)dw_tasks(IN, a->H)), dim3(RN_THREADS), 0, st, p);
  return (int)hipGetLastError();
}
