// t2o_qmix.hip — the QMIX and VDN mixers of TDLearner (mixer: qmix / vdn).
//
// Neither mixer ships with the reference (n_transf_mixer.py only), so both are this
// project's DECLARED definitions after PyMARL2's modules/mixers/nmix.py and vdn.py
// (parity-unpinned; DESIGN.md §5, restated in fp64 in tests/qmix_model.py).  Per
// (episode, step) row, with state s [S] and the agents' q [A]:
//
//   h1 = relu(W1a s + c1a)      w1 = pos(W1b h1 + c1b).view(A, M)     hyper_w1
//   b1 = Wb1 s + cb1                                                  hyper_b1
//   h2 = relu(W2a s + c2a)      w2 = pos(W2b h2 + c2b)                hyper_w2
//   h3 = relu(W3a s + c3a)      b2 = W3b h3 + c3b                     hyper_b2
//   y  = elu(q · w1 + b1) · w2 + b2
//
// Rows are independent (no recurrence).  A wave owns a tile of 16 rows in the
// T-layout of t2o_common.hpp (lane (g, c): row c, features 16t + 4g + r): the three
// GEMMs S -> {H, M, H, M}, H -> A·M and H -> M run on v_mfma_f32_16x16x4_f32 with the
// out-features on the MFMA's M axis, so each layer's result is the next one's B
// operand where it lies.  Weights come straight from the flat parameters through L2
// (at 64 AGVs the first layers are 390 KB and W1b 512 KB: neither fits LDS), W1b one
// agent chunk [M][H] at a time, and w1 is consumed from the accumulators
// (pre += q_a · pos(w1[a, :])): it is never written to memory.
//
// Backward, of one network:
//   rows kernel   recomputes the row tile's forward, then dL/dq and the gradients of
//                 every pre-activation; the agent loop runs again for dL/dh1
//                 (W1b chunkᵀ · dL/dw1raw).  It leaves the row's small activations
//                 (h1, h2, h3, the first layers' pre-activation gradients, dL/dw2raw,
//                 gy: 4H + 4M + 4 floats) in the work buffer, rows padded to whole
//                 tiles with zero gradients.
//   dW1b kernel   grid (slab, agent): the agent chunk outer, the slab's row tiles
//                 inner.  w1raw of the chunk is recomputed TRANSPOSED (rows on the
//                 MFMA's M axis), which is the A-operand layout of the contraction
//                 over rows dW1b[a] += Gᵀ h1, so nothing moves between lanes; the
//                 chunk's dW lives in accumulators and is stored once.
//   dW rows kernel  the other weight gradients, Σ_rows P[row][o] Q[row][k] over the
//                 saved activations and the states, one 16-row tile per MFMA K sweep.
// Both weight-gradient kernels sum their four waves' accumulators through LDS in
// wave order and write every element of the workgroup's slab exactly once: a fixed
// order, no atomics.  t2o_reduce_slabs sums the slabs.
#include "t2o_common.hpp"

namespace {

using namespace t2o;

constexpr int QM_THREADS = 256, QM_WAVES = 4;
constexpr int QM_MAXA = 64, QM_MAXS = 1024, QM_MAX_SLABS = 64, QM_SLAB_TILES = 8;
constexpr int QM_KG = 8;  // k tiles of one dW-rows task

struct QOff {
  int64_t W1a, c1a, W1b, c1b, Wb1, cb1, W2a, c2a, W2b, c2b, W3a, c3a, W3b, c3b, total;
};

__host__ __device__ inline QOff qoff(int A, int S, int M, int H) {
  QOff o;
  int64_t p = 0;
  o.W1a = p, p += (int64_t)H * S;
  o.c1a = p, p += H;
  o.W1b = p, p += (int64_t)A * M * H;
  o.c1b = p, p += (int64_t)A * M;
  o.Wb1 = p, p += (int64_t)M * S;
  o.cb1 = p, p += M;
  o.W2a = p, p += (int64_t)H * S;
  o.c2a = p, p += H;
  o.W2b = p, p += (int64_t)M * H;
  o.c2b = p, p += M;
  o.W3a = p, p += (int64_t)M * S;
  o.c3a = p, p += M;
  o.W3b = p, p += M;
  o.c3b = p, p += 1;
  o.total = p;
  return o;
}

// columns of a work row
struct WCol {
  int h1, h2, h3, g1, gw2, gy, ws;
};
__host__ __device__ inline WCol wcol(int M, int H) {
  WCol w;
  w.h1 = 0, w.h2 = H, w.h3 = 2 * H;
  w.g1 = 2 * H + M;  // [gz1 H][gpre M][gz2 H][gz3 M]
  w.gw2 = 4 * H + 3 * M;
  w.gy = 4 * H + 4 * M;
  w.ws = 4 * H + 4 * M + 4;
  return w;
}

template <bool VEC>
T2O_DEV f4 ldw4(const float* p) {
  if (VEC) return ld4(p);
  return f4{p[0], p[1], p[2], p[3]};
}

T2O_DEV float gsum(float v) {  // Σ over the four lane groups of a row
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}

T2O_DEV f4 relu4(f4 v) { return f4{fmaxf(v[0], 0.f), fmaxf(v[1], 0.f), fmaxf(v[2], 0.f), fmaxf(v[3], 0.f)}; }

// ---------------------------------------------------------------------------
// Q selection
struct SelP {
  const float *q_on, *q_tg;
  const int64_t* actions;
  int64_t act_sb, act_st;
  const int32_t* avail;
  int64_t av_sb, av_st;
  float *qv_on, *qv_tg;
  int q_ts, NA, qmode_on, qmode_tg, B, T_on, T_tg, A;
};

__global__ __launch_bounds__(256) void qsel_kernel(SelP p) {
  const int net = blockIdx.y;
  const int T = net ? p.T_tg : p.T_on, mode = net ? p.qmode_tg : p.qmode_on;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)p.B * T * p.A) return;
  const int a = (int)(i % p.A);
  const int64_t bt = i / p.A;
  const int t = (int)(bt % T), b = (int)(bt / T);
  const int NA = p.NA;
  const int64_t qrow = (((int64_t)b * p.q_ts + t) * p.A + a) * NA;
  int act = 0;
  if (mode == 1) {
    const int64_t v = p.actions[b * p.act_sb + t * p.act_st + a];
    act = v < 0 ? 0 : v >= NA ? NA - 1 : (int)v;  // (never in a valid batch; keeps the load in bounds)
  } else {
    const int32_t* av = p.avail ? p.avail + b * p.av_sb + t * p.av_st + (int64_t)a * NA : nullptr;
    float best = -INFINITY;
    for (int k = 0; k < NA; ++k) {
      const float v = (av && av[k] == 0) ? -9999999.0f : p.q_on[qrow + k];
      if (k == 0 || v > best) {  // first max wins
        best = v;
        act = k;
      }
    }
  }
  (net ? p.qv_tg : p.qv_on)[i] = (net ? p.q_tg : p.q_on)[qrow + act];
}

// y[row] = Σ_a qv[row][a], in agent order
__global__ __launch_bounds__(256) void rowsum_kernel(const float* __restrict__ qv, float* __restrict__ y, int64_t R,
                                                     int A) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= R) return;
  float s = 0.f;
  for (int a = 0; a < A; ++a) s += qv[i * A + a];
  y[i] = s;
}

__global__ __launch_bounds__(256) void vdn_bwd_kernel(const float* __restrict__ gy, float* __restrict__ gqv, int64_t n,
                                                      int A) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) gqv[i] = gy[i / A];
}

// ---------------------------------------------------------------------------
// the row tile's forward
struct RowP {
  const float* params[2];
  const float* states;
  int64_t st_sb, st_st;
  const float* qv[2];
  float* y[2];
  int T[2];
  int B, A, S, M, H, pf;
  float pb;
  // backward only
  const float* gy;
  float* gqv;
  float* work;
};

template <int MT, int HT>
struct RowAct {
  f4 z1[HT], z2[HT], z3[MT], pre[MT], w2raw[MT];
  float b2;
};

// acc[t] += W[16t + c][k0 + 4g + s] · x[s]  (W [16·NT][S] row-major; columns past S clamped: x is 0 there)
template <int NT>
T2O_DEV void lin_s(const float* __restrict__ W, int S, int k0, f4 x, f4* acc) {
  const int c = lane_c(), g = lane_g();
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const float* w = W + (int64_t)(16 * t + c) * S;
#pragma unroll
    for (int s = 0; s < 4; ++s) acc[t] = mfma4(w[min(k0 + 4 * g + s, S - 1)], x[s], acc[t]);
  }
}

template <int NT>
T2O_DEV void bias_init(const float* __restrict__ b, f4* acc) {
  const int g = lane_g();
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[t][r] = b[16 * t + 4 * g + r];
}

// out[t] (+)= W[16t + c][:] · h  for NT out tiles of W [.][16·HT], h in the T-layout
template <int NT, int HT, bool VEC>
T2O_DEV void lin_h(const float* __restrict__ W, const f4* h, f4* acc) {
  const int c = lane_c(), g = lane_g();
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const float* w = W + (int64_t)(16 * t + c) * (16 * HT) + 4 * g;
#pragma unroll
    for (int i = 0; i < HT; ++i) {
      const f4 wf = ldw4<VEC>(w + 16 * i);
#pragma unroll
      for (int s = 0; s < 4; ++s) acc[t] = mfma4(wf[s], h[i][s], acc[t]);
    }
  }
}

// gh[i] += Wᵀ · gv: W [16·MT][16·HT] row-major, gv [MT] in the T-layout, gh [HT]
template <int MT, int HT>
T2O_DEV void lin_ht(const float* __restrict__ W, const f4* gv, f4* gh) {
  const int c = lane_c(), g = lane_g();
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const float* w = W + (int64_t)(16 * t + 4 * g + s) * (16 * HT) + c;
#pragma unroll
      for (int i = 0; i < HT; ++i) gh[i] = mfma4(w[16 * i], gv[t][s], gh[i]);
    }
}

template <int MT, int HT, bool VEC>
T2O_DEV void row_forward(const RowP& p, int net, int64_t row, int64_t R, RowAct<MT, HT>& r) {
  const int g = lane_g();
  const int S = p.S, A = p.A, T = p.T[net];
  constexpr int M = 16 * MT, H = 16 * HT;
  const QOff o = qoff(A, S, M, H);
  const float* P = p.params[net];
  const int64_t rr = row < R ? row : R - 1;  // padding rows read the last row
  const float* st = p.states + (rr / T) * p.st_sb + (rr % T) * p.st_st;
  bias_init<HT>(P + o.c1a, r.z1);
  bias_init<MT>(P + o.cb1, r.pre);
  bias_init<HT>(P + o.c2a, r.z2);
  bias_init<MT>(P + o.c3a, r.z3);
  for (int k0 = 0; k0 < S; k0 += 16) {
    f4 x;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int k = k0 + 4 * g + s;
      const float v = st[min(k, S - 1)];
      x[s] = k < S ? v : 0.f;
    }
    lin_s<HT>(P + o.W1a, S, k0, x, r.z1);
    lin_s<MT>(P + o.Wb1, S, k0, x, r.pre);
    lin_s<HT>(P + o.W2a, S, k0, x, r.z2);
    lin_s<MT>(P + o.W3a, S, k0, x, r.z3);
  }
  f4 h1[HT], h2[HT];
#pragma unroll
  for (int i = 0; i < HT; ++i) h1[i] = relu4(r.z1[i]), h2[i] = relu4(r.z2[i]);
  bias_init<MT>(P + o.c2b, r.w2raw);
  lin_h<MT, HT, VEC>(P + o.W2b, h2, r.w2raw);
  float b2 = 0.f;
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int q = 0; q < 4; ++q) b2 = fmaf(fmaxf(r.z3[t][q], 0.f), P[o.W3b + 16 * t + 4 * g + q], b2);
  r.b2 = gsum(b2) + P[o.c3b];
  const float* qrow = p.qv[net] + rr * A;
  for (int a = 0; a < A; ++a) {
    f4 w[MT];
    bias_init<MT>(P + o.c1b + (int64_t)a * M, w);
    lin_h<MT, HT, VEC>(P + o.W1b + (int64_t)a * M * H, h1, w);
    const float qa = qrow[a];
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
      for (int q = 0; q < 4; ++q) r.pre[t][q] = fmaf(qa, posf(w[t][q], p.pf, p.pb), r.pre[t][q]);
  }
}

template <int MT, int HT, bool VEC>
__global__ __launch_bounds__(QM_THREADS) void qmix_fwd_kernel(RowP p) {
  const int net = blockIdx.y;
  const int64_t R = (int64_t)p.B * p.T[net];
  const int64_t row0 = ((int64_t)blockIdx.x * QM_WAVES + wave_id()) * 16;
  if (row0 >= R) return;  // (whole waves leave; no workgroup barrier below)
  const int64_t row = row0 + lane_c();
  RowAct<MT, HT> r;
  row_forward<MT, HT, VEC>(p, net, row, R, r);
  float y = 0.f;
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float x = r.pre[t][q];
      y = fmaf(x > 0.f ? x : expm1f(x), posf(r.w2raw[t][q], p.pf, p.pb), y);
    }
  y = gsum(y) + r.b2;
  if (lane_g() == 0 && row < R) p.y[net][row] = y;
}

// ---------------------------------------------------------------------------
// backward, rows
template <int NT>
T2O_DEV void store_t(float* wrow, int col, const f4* v) {
  const int g = lane_g();
#pragma unroll
  for (int t = 0; t < NT; ++t) *reinterpret_cast<f4*>(wrow + col + 16 * t + 4 * g) = v[t];
}

template <int MT, int HT, bool VEC>
__global__ __launch_bounds__(QM_THREADS) void qmix_bwd_rows_kernel(RowP p) {
  const int64_t R = (int64_t)p.B * p.T[0];
  const int64_t row0 = ((int64_t)blockIdx.x * QM_WAVES + wave_id()) * 16;
  if (row0 >= R) return;
  const int g = lane_g();
  const int64_t row = row0 + lane_c();
  const bool live = row < R;
  constexpr int M = 16 * MT, H = 16 * HT;
  const int A = p.A;
  const QOff o = qoff(A, p.S, M, H);
  const WCol wc = wcol(M, H);
  const float* P = p.params[0];
  RowAct<MT, HT> r;
  row_forward<MT, HT, VEC>(p, 0, row, R, r);
  const float gy = live ? p.gy[row] : 0.f;  // padding rows: every gradient below is 0
  f4 gpre[MT], gw2[MT], gz3[MT], h3[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float x = r.pre[t][q];
      const float hid = x > 0.f ? x : expm1f(x), dhid = x > 0.f ? 1.f : expf(x);
      float w2, dw2;
      posd(r.w2raw[t][q], p.pf, p.pb, w2, dw2);
      gpre[t][q] = gy * w2 * dhid;
      gw2[t][q] = gy * hid * dw2;
      gz3[t][q] = r.z3[t][q] > 0.f ? gy * P[o.W3b + 16 * t + 4 * g + q] : 0.f;
      h3[t][q] = fmaxf(r.z3[t][q], 0.f);
    }
  f4 gh1[HT], gh2[HT], h1[HT], h2[HT];
#pragma unroll
  for (int i = 0; i < HT; ++i) gh1[i] = zero4(), gh2[i] = zero4(), h1[i] = relu4(r.z1[i]), h2[i] = relu4(r.z2[i]);
  lin_ht<MT, HT>(P + o.W2b, gw2, gh2);
  const int64_t rr = live ? row : R - 1;
  const float* qrow = p.qv[0] + rr * A;
  for (int a = 0; a < A; ++a) {
    f4 w[MT], gw[MT];
    bias_init<MT>(P + o.c1b + (int64_t)a * M, w);
    lin_h<MT, HT, VEC>(P + o.W1b + (int64_t)a * M * H, h1, w);
    const float qa = qrow[a];
    float gq = 0.f;
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float w1, dw1;
        posd(w[t][q], p.pf, p.pb, w1, dw1);
        gq = fmaf(gpre[t][q], w1, gq);
        gw[t][q] = qa * gpre[t][q] * dw1;
      }
    gq = gsum(gq);
    if (g == 0 && live) p.gqv[row * A + a] = gq;
    lin_ht<MT, HT>(P + o.W1b + (int64_t)a * M * H, gw, gh1);
  }
#pragma unroll
  for (int i = 0; i < HT; ++i)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      gh1[i][q] = r.z1[i][q] > 0.f ? gh1[i][q] : 0.f;
      gh2[i][q] = r.z2[i][q] > 0.f ? gh2[i][q] : 0.f;
    }
  float* wrow = p.work + row * wc.ws;  // (the work buffer holds whole tiles)
  store_t<HT>(wrow, wc.h1, h1);
  store_t<HT>(wrow, wc.h2, h2);
  store_t<MT>(wrow, wc.h3, h3);
  store_t<HT>(wrow, wc.g1, gh1);
  store_t<MT>(wrow, wc.g1 + H, gpre);
  store_t<HT>(wrow, wc.g1 + H + M, gh2);
  store_t<MT>(wrow, wc.g1 + 2 * H + M, gz3);
  store_t<MT>(wrow, wc.gw2, gw2);
  if (g == 0) *reinterpret_cast<f4*>(wrow + wc.gy) = f4{gy, 0.f, 0.f, 0.f};
}

// ---------------------------------------------------------------------------
// backward, weight gradients
struct DwP {
  const float* params;
  const float* states;
  int64_t st_sb, st_st;
  const float* qv;
  const float* work;
  float* slabs;
  int64_t R, ntiles;
  int T, A, S, M, H, pf, tps;  // tps: row tiles per slab
  float pb;
};

// Σ over the waves, in wave order, of NACC accumulators per wave staged in red [QM_WAVES][NACC][64]
template <int NACC>
T2O_DEV f4 wave_total(const f4* red, int j, int lane) {
  f4 v = red[(0 * NACC + j) * 64 + lane];
#pragma unroll
  for (int w = 1; w < QM_WAVES; ++w) v += red[(w * NACC + j) * 64 + lane];
  return v;
}

template <int MT, int HT, bool VEC>
__global__ __launch_bounds__(QM_THREADS) void qmix_dw1b_kernel(DwP p) {
  constexpr int M = 16 * MT, H = 16 * HT, NACC = MT * HT + MT;
  __shared__ f4 red[QM_WAVES * NACC * 64];
  const int slab = blockIdx.x, a = blockIdx.y, wv = wave_id();
  const int c = lane_c(), g = lane_g(), lane = threadIdx.x & 63;
  const QOff o = qoff(p.A, p.S, M, H);
  const WCol wc = wcol(M, H);
  const float* Wc = p.params + o.W1b + (int64_t)a * M * H;
  f4 wf[MT][HT], dW[MT][HT], db[MT];
  float bias[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    bias[mt] = p.params[o.c1b + (int64_t)a * M + 16 * mt + c];
    db[mt] = zero4();
#pragma unroll
    for (int i = 0; i < HT; ++i) {
      wf[mt][i] = ldw4<VEC>(Wc + (int64_t)(16 * mt + c) * H + 16 * i + 4 * g);
      dW[mt][i] = zero4();
    }
  }
  const int64_t lo = (int64_t)slab * p.tps, hi = min(lo + p.tps, p.ntiles);
  for (int64_t tile = lo + wv; tile < hi; tile += QM_WAVES) {
    const int64_t row0 = tile * 16;
    const float* wk = p.work + row0 * wc.ws;
    f4 ha[HT];
#pragma unroll
    for (int i = 0; i < HT; ++i) ha[i] = ld4(wk + (int64_t)c * wc.ws + wc.h1 + 16 * i + 4 * g);
    float q4[4];
    f4 hb[HT];  // h1[row0 + 4g + s][16i + c]
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      q4[s] = p.qv[min(row0 + 4 * g + s, p.R - 1) * p.A + a];
#pragma unroll
      for (int i = 0; i < HT; ++i) hb[i][s] = wk[(int64_t)(4 * g + s) * wc.ws + wc.h1 + 16 * i + c];
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      // w1raw[row0 + 4g + r][a·M + 16mt + c]: rows on the M axis
      f4 d = f4{bias[mt], bias[mt], bias[mt], bias[mt]};
#pragma unroll
      for (int i = 0; i < HT; ++i)
#pragma unroll
        for (int s = 0; s < 4; ++s) d = mfma4(ha[i][s], wf[mt][i][s], d);
      f4 gw;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const float gp = wk[(int64_t)(4 * g + s) * wc.ws + wc.g1 + H + 16 * mt + c];
        gw[s] = q4[s] * gp * dposf(d[s], p.pf, p.pb);
      }
#pragma unroll
      for (int s = 0; s < 4; ++s) {
#pragma unroll
        for (int i = 0; i < HT; ++i) dW[mt][i] = mfma4(gw[s], hb[i][s], dW[mt][i]);
        db[mt] = mfma4(gw[s], 1.f, db[mt]);
      }
    }
  }
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
    for (int i = 0; i < HT; ++i) red[(wv * NACC + mt * HT + i) * 64 + lane] = dW[mt][i];
    red[(wv * NACC + MT * HT + mt) * 64 + lane] = db[mt];
  }
  __syncthreads();
  float* out = p.slabs + (int64_t)slab * o.total;
  for (int idx = threadIdx.x; idx < NACC * 64; idx += QM_THREADS) {
    const int j = idx / 64, l = idx % 64, lc = l & 15, lg = l >> 4;
    const f4 v = wave_total<NACC>(red, j, l);
    if (j < MT * HT) {
      const int mt = j / HT, i = j % HT;
#pragma unroll
      for (int r = 0; r < 4; ++r) out[o.W1b + ((int64_t)a * M + 16 * mt + 4 * lg + r) * H + 16 * i + lc] = v[r];
    } else if (lc == 0) {
      const int mt = j - MT * HT;
#pragma unroll
      for (int r = 0; r < 4; ++r) out[o.c1b + (int64_t)a * M + 16 * mt + 4 * lg + r] = v[r];
    }
  }
}

// one task: a 16-row tile of outputs o against up to QM_KG 16-column tiles of k
struct DwTask {
  int pcol, no;       // P: work column of the tile's first output, valid outputs (16, or 1)
  int qstate, qcol;   // Q: the states, or a work column
  int nk, k0;         // Q's width, the task's first column
  int64_t wdst, bdst; // slab offsets of W[o0][0] and its bias (-1: another task writes it)
  int ldw;
};

__device__ inline DwTask dw_task(int y, const QOff& o, const WCol& wc, int S, int M, int H) {
  const int KT = (S + 15) / 16, KGn = (KT + QM_KG - 1) / QM_KG;
  const int nA = (2 * H + 2 * M) / 16 * KGn;
  DwTask t;
  if (y < nA) {
    const int ot = y / KGn, kg = y % KGn, oc = 16 * ot;
    int64_t w, b;
    int row;
    if (oc < H) w = o.W1a, b = o.c1a, row = oc;
    else if (oc < H + M) w = o.Wb1, b = o.cb1, row = oc - H;
    else if (oc < 2 * H + M) w = o.W2a, b = o.c2a, row = oc - H - M;
    else w = o.W3a, b = o.c3a, row = oc - 2 * H - M;
    t = DwTask{wc.g1 + oc, 16, 1, 0, S, kg * QM_KG * 16, w + (int64_t)row * S, kg == 0 ? b + row : -1, S};
  } else if (y < nA + M / 16) {
    const int mt = y - nA;
    t = DwTask{wc.gw2 + 16 * mt, 16, 0, wc.h2, H, 0, o.W2b + (int64_t)16 * mt * H, o.c2b + 16 * mt, H};
  } else {
    t = DwTask{wc.gy, 1, 0, wc.h3, M, 0, o.W3b, o.c3b, M};
  }
  return t;
}

__global__ __launch_bounds__(QM_THREADS) void qmix_dwrows_kernel(DwP p) {
  constexpr int NACC = QM_KG + 1;
  __shared__ f4 red[QM_WAVES * NACC * 64];
  const int slab = blockIdx.x, wv = wave_id();
  const int c = lane_c(), g = lane_g(), lane = threadIdx.x & 63;
  const QOff o = qoff(p.A, p.S, p.M, p.H);
  const WCol wc = wcol(p.M, p.H);
  const DwTask t = dw_task(blockIdx.y, o, wc, p.S, p.M, p.H);
  const int nkt = min(QM_KG, (t.nk - t.k0 + 15) / 16);
  f4 acc[NACC];
#pragma unroll
  for (int j = 0; j < NACC; ++j) acc[j] = zero4();
  const int64_t lo = (int64_t)slab * p.tps, hi = min(lo + p.tps, p.ntiles);
  for (int64_t tile = lo + wv; tile < hi; tile += QM_WAVES) {
    const int64_t row0 = tile * 16;
    f4 pa;
    const float* qrow[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int64_t row = row0 + 4 * g + s;
      const float* wr = p.work + row * wc.ws;
      const float v = wr[t.pcol + (c < t.no ? c : 0)];
      pa[s] = c < t.no ? v : 0.f;
      if (t.qstate) {
        const int64_t rr = row < p.R ? row : p.R - 1;  // (padding rows: P is 0 there)
        qrow[s] = p.states + (rr / p.T) * p.st_sb + (rr % p.T) * p.st_st;
      } else {
        qrow[s] = wr + t.qcol;
      }
    }
#pragma unroll
    for (int j = 0; j < QM_KG; ++j) {
      if (j < nkt) {
        const int k = t.k0 + 16 * j + c;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const float v = qrow[s][min(k, t.nk - 1)];
          acc[j] = mfma4(pa[s], k < t.nk ? v : 0.f, acc[j]);
        }
      }
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) acc[QM_KG] = mfma4(pa[s], 1.f, acc[QM_KG]);
  }
#pragma unroll
  for (int j = 0; j < NACC; ++j) red[(wv * NACC + j) * 64 + lane] = acc[j];
  __syncthreads();
  float* out = p.slabs + (int64_t)slab * o.total;
  for (int idx = threadIdx.x; idx < NACC * 64; idx += QM_THREADS) {
    const int j = idx / 64, l = idx % 64, lc = l & 15, lg = l >> 4;
    const f4 v = wave_total<NACC>(red, j, l);
    if (j < QM_KG) {
      const int k = t.k0 + 16 * j + lc;
      if (j < nkt && k < t.nk) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (4 * lg + r < t.no) out[t.wdst + (int64_t)(4 * lg + r) * t.ldw + k] = v[r];
      }
    } else if (lc == 0 && t.bdst >= 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (4 * lg + r < t.no) out[t.bdst + 4 * lg + r] = v[r];
    }
  }
}

// ---------------------------------------------------------------------------
bool dims_ok(int A, int S, int M, int H) {
  return A >= 1 && A <= QM_MAXA && S >= 1 && S <= QM_MAXS && (M == 16 || M == 32) && (H == 32 || H == 64);
}

bool rows_ok(int B, int T) { return B >= 1 && T >= 1 && (int64_t)B * T < (1ll << 27); }

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int slabs_of(int B, int T) {
  const int64_t ntiles = ((int64_t)B * T + 15) / 16;
  const int64_t n = ntiles / QM_SLAB_TILES;
  return (int)(n < 1 ? 1 : n > QM_MAX_SLABS ? QM_MAX_SLABS : n);
}

// kernel<MT, HT, VEC> for (M, H) in {16, 32} x {32, 64}
#define T2O_QMIX_DISPATCH(KERNEL, M, H, VEC, ...)                                              \
  do {                                                                                         \
    if ((M) == 32 && (H) == 64) {                                                              \
      if (VEC) hipLaunchKernelGGL((KERNEL<2, 4, true>), __VA_ARGS__);                          \
      else hipLaunchKernelGGL((KERNEL<2, 4, false>), __VA_ARGS__);                             \
    } else if ((M) == 32) {                                                                    \
      if (VEC) hipLaunchKernelGGL((KERNEL<2, 2, true>), __VA_ARGS__);                          \
      else hipLaunchKernelGGL((KERNEL<2, 2, false>), __VA_ARGS__);                             \
    } else if ((H) == 64) {                                                                    \
      if (VEC) hipLaunchKernelGGL((KERNEL<1, 4, true>), __VA_ARGS__);                          \
      else hipLaunchKernelGGL((KERNEL<1, 4, false>), __VA_ARGS__);                             \
    } else {                                                                                   \
      if (VEC) hipLaunchKernelGGL((KERNEL<1, 2, true>), __VA_ARGS__);                          \
      else hipLaunchKernelGGL((KERNEL<1, 2, false>), __VA_ARGS__);                             \
    }                                                                                          \
  } while (0)

}  // namespace

extern "C" int t2o_q_select(const t2o_q_select_args* a, void* stream) {
  if (!a || !a->q_on || !a->qv_on) return T2O_EINVAL;
  if (a->B < 1 || a->T_on < 1 || a->A < 1 || a->A > QM_MAXA || a->n_actions < 1 || a->n_actions > 1024)
    return T2O_EINVAL;
  if (a->q_ts < a->T_on || (int64_t)a->B * a->q_ts >= (1ll << 27)) return T2O_EINVAL;
  if (a->qmode_on != 1 && a->qmode_on != 2) return T2O_EINVAL;
  const bool two = a->q_tg != nullptr;
  if (two && (!a->qv_tg || a->T_tg < 1 || a->T_tg > a->q_ts || (a->qmode_tg != 1 && a->qmode_tg != 2)))
    return T2O_EINVAL;
  if ((a->qmode_on == 1 || (two && a->qmode_tg == 1)) && !a->actions) return T2O_EINVAL;
  if (a->y_tg && !two) return T2O_EINVAL;
  const SelP p{a->q_on, a->q_tg, a->actions, a->act_sb, a->act_st, a->avail, a->av_sb, a->av_st, a->qv_on, a->qv_tg,
               a->q_ts, a->n_actions, a->qmode_on, two ? a->qmode_tg : 0, a->B, a->T_on, two ? a->T_tg : 0, a->A};
  hipStream_t st = (hipStream_t)stream;
  const int Tmax = two && a->T_tg > a->T_on ? a->T_tg : a->T_on;
  const int64_t n = (int64_t)a->B * Tmax * a->A;
  hipLaunchKernelGGL(qsel_kernel, dim3((unsigned)((n + 255) / 256), two ? 2 : 1), dim3(256), 0, st, p);
  if (a->y_on) {
    const int64_t R = (int64_t)a->B * a->T_on;
    hipLaunchKernelGGL(rowsum_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, st, a->qv_on, a->y_on, R, a->A);
  }
  if (a->y_tg) {
    const int64_t R = (int64_t)a->B * a->T_tg;
    hipLaunchKernelGGL(rowsum_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, st, a->qv_tg, a->y_tg, R, a->A);
  }
  return (int)hipGetLastError();
}

extern "C" int64_t t2o_qmix_param_count(int A, int S, int M, int H) {
  if (!dims_ok(A, S, M, H)) return T2O_EINVAL;
  return qoff(A, S, M, H).total;
}

extern "C" int t2o_qmix_fwd(const t2o_qmix_fwd_args* a, void* stream) {
  if (!a || !a->params_on || !a->states || !a->qv_on || !a->y_on) return T2O_EINVAL;
  if (!dims_ok(a->A, a->S, a->M, a->H) || !rows_ok(a->B, a->T_on)) return T2O_EINVAL;
  if (a->pos_func < T2O_POS_ABS || a->pos_func > T2O_POS_IDENTITY) return T2O_EINVAL;
  const bool two = a->params_tg != nullptr;
  if (two && (!a->qv_tg || !a->y_tg || !rows_ok(a->B, a->T_tg))) return T2O_EINVAL;
  RowP p{};
  p.params[0] = a->params_on, p.params[1] = a->params_tg;
  p.states = a->states, p.st_sb = a->st_sb, p.st_st = a->st_st;
  p.qv[0] = a->qv_on, p.qv[1] = a->qv_tg;
  p.y[0] = a->y_on, p.y[1] = a->y_tg;
  p.T[0] = a->T_on, p.T[1] = two ? a->T_tg : 0;
  p.B = a->B, p.A = a->A, p.S = a->S, p.M = a->M, p.H = a->H, p.pf = a->pos_func, p.pb = a->pos_beta;
  const int Tmax = two && a->T_tg > a->T_on ? a->T_tg : a->T_on;
  const int64_t ntiles = ((int64_t)a->B * Tmax + 15) / 16;
  const dim3 grid((unsigned)((ntiles + QM_WAVES - 1) / QM_WAVES), two ? 2 : 1), block(QM_THREADS);
  const bool vec = aligned16(a->params_on) && (!two || aligned16(a->params_tg));
  T2O_QMIX_DISPATCH(qmix_fwd_kernel, a->M, a->H, vec, grid, block, 0, (hipStream_t)stream, p);
  return (int)hipGetLastError();
}

extern "C" int t2o_qmix_bwd_slabs(int B, int T) {
  if (!rows_ok(B, T)) return T2O_EINVAL;
  return slabs_of(B, T);
}

extern "C" int64_t t2o_qmix_bwd_work_floats(int B, int T, int M, int H) {
  if (!rows_ok(B, T) || !dims_ok(1, 1, M, H)) return T2O_EINVAL;
  return (((int64_t)B * T + 15) / 16) * 16 * wcol(M, H).ws;
}

extern "C" int t2o_qmix_bwd(const t2o_qmix_bwd_args* a, void* stream) {
  if (!a || !a->params || !a->states || !a->qv || !a->work) return T2O_EINVAL;
  if (a->phase < 0 || a->phase > 2) return T2O_EINVAL;
  if (a->phase != 2 && (!a->gy || !a->gqv)) return T2O_EINVAL;
  if (a->phase != 1 && !a->gslabs) return T2O_EINVAL;
  if (!dims_ok(a->A, a->S, a->M, a->H) || !rows_ok(a->B, a->T)) return T2O_EINVAL;
  if (a->pos_func < T2O_POS_ABS || a->pos_func > T2O_POS_IDENTITY) return T2O_EINVAL;
  if (!aligned16(a->work) || a->work_floats < t2o_qmix_bwd_work_floats(a->B, a->T, a->M, a->H)) return T2O_EINVAL;
  const int nslab = slabs_of(a->B, a->T);
  if (a->phase != 1 && a->max_slabs < nslab) return T2O_EINVAL;
  const int64_t R = (int64_t)a->B * a->T, ntiles = (R + 15) / 16;
  const bool vec = aligned16(a->params);
  hipStream_t st = (hipStream_t)stream;
  const dim3 block(QM_THREADS);
  if (a->phase != 2) {
    RowP p{};
    p.params[0] = a->params, p.states = a->states, p.st_sb = a->st_sb, p.st_st = a->st_st;
    p.qv[0] = a->qv, p.T[0] = a->T;
    p.B = a->B, p.A = a->A, p.S = a->S, p.M = a->M, p.H = a->H, p.pf = a->pos_func, p.pb = a->pos_beta;
    p.gy = a->gy, p.gqv = a->gqv, p.work = a->work;
    const dim3 grid((unsigned)((ntiles + QM_WAVES - 1) / QM_WAVES));
    T2O_QMIX_DISPATCH(qmix_bwd_rows_kernel, a->M, a->H, vec, grid, block, 0, st, p);
  }
  if (a->phase != 1) {
    const int tps = (int)((ntiles + nslab - 1) / nslab);
    const DwP p{a->params, a->states, a->st_sb, a->st_st, a->qv, a->work, a->gslabs, R, ntiles,
                a->T, a->A, a->S, a->M, a->H, a->pos_func, tps, a->pos_beta};
    T2O_QMIX_DISPATCH(qmix_dw1b_kernel, a->M, a->H, vec, dim3((unsigned)nslab, (unsigned)a->A), block, 0, st, p);
    const int KT = (a->S + 15) / 16, KGn = (KT + QM_KG - 1) / QM_KG;
    const int tasks = (2 * a->H + 2 * a->M) / 16 * KGn + a->M / 16 + 1;
    hipLaunchKernelGGL(qmix_dwrows_kernel, dim3((unsigned)nslab, (unsigned)tasks), block, 0, st, p);
  }
  return (int)hipGetLastError();
}

extern "C" int t2o_vdn_bwd(const float* gy, float* gqv, int B, int T, int A, void* stream) {
  if (!gy || !gqv || !rows_ok(B, T) || A < 1 || A > QM_MAXA) return T2O_EINVAL;
  const int64_t n = (int64_t)B * T * A;
  hipLaunchKernelGGL(vdn_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, gy, gqv, n,
                     A);
  return (int)hipGetLastError();
}
