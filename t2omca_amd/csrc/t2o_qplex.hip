// t2o_qplex.hip — the QPLEX duelling mixer of TDLearner (mixer: dmaq / qplex).
//
// QPLEX does not ship with the reference (n_transf_mixer.py only): this is the project's
// DECLARED definition after PyMARL2's modules/mixers/dmaq_general.py, dmaq_si_weight.py
// and learners/dmaq_qatten_learner.py at qplex.yaml's defaults (parity-unpinned;
// DESIGN.md §5, restated in fp64 in tests/qplex_model.py).  Per (episode, step) row, with
// state s [S], the agents' q [A], their maxima m [A] and the joint action u [A]:
//
//   w   = |hyper_w_final(s)| + 1e-10          v = V(s)
//   d   = [s ; onehot(u_0) ; ... ; onehot(u_{A-1})]
//   κ_k = |key_k(s)| + 1e-10    α_k = sigmoid(agents_k(s))    β_k = sigmoid(action_k(d))
//   λ   = Σ_k κ_k · α_k ⊙ β_k
//   y_v = Σ_a (w_a q_a + v_a)     y_adv = Σ_a sg[w_a (q_a − m_a)] · (λ_a − 1)
//
// Every network is Linear(in, Hx), ReLU, Linear(Hx, out): 2 + 3K "blocks" in the
// parameter order (hyper_w_final, V, key_0.., agents_0.., action_0..), each its first
// weight [Hx][in], first bias, second weight [out][Hx], second bias.
//
// Rows are independent.  A wave owns a tile of 16 rows in the T-layout of
// t2o_common.hpp (lane (g, c): row c, features 16t + 4g + r); both layers of every block
// run on v_mfma_f32_16x16x4_f32 with the out-features on the MFMA's M axis, one block at
// a time (its hidden vector never leaves registers; w, v, λ never go to memory).  Weights
// come straight from the flat parameters through L2.  The second weights are read 16
// bytes at a time where the block's own matrix is 16-byte aligned and 4 bytes at a time
// otherwise (the key extractors hold an odd number of floats, so the alignment changes
// from block to block whatever the buffer's).  The one-hot part of d enters the action
// extractors' first layer as a gather-add of A weight columns per row.
//
// Backward, of one network:
//   rows kernel   recomputes the row tile's forward block by block and leaves, per block,
//                 its hidden vector h, the gradient of its first layer's pre-activation
//                 and of its output in the work buffer (rows padded to whole tiles with
//                 zero gradients), and dL/dq = gy · w.  The stop-gradient: c = w (q − m)
//                 is a constant, so hyper_w_final gets gy · q · sign alone.
//   dW kernel     every weight gradient as Σ_rows P[row][o] Q[row][k], one 16-row tile per
//                 MFMA K sweep: Q is the states, a saved hidden vector, or (the one-hot
//                 columns of the action extractors' first weight) one-hot fragments built
//                 in registers from u.  The four waves' accumulators are summed through
//                 LDS in wave order and every element of the workgroup's slab is written
//                 exactly once: a fixed order, no atomics.  t2o_reduce_slabs sums the slabs.
#include "t2o_common.hpp"

namespace {

using namespace t2o;

constexpr int QP_THREADS = 256, QP_WAVES = 4;
constexpr int QP_MAXA = 64, QP_MAXS = 1024, QP_MAXNA = 16, QP_MAXK = 10, QP_MAX_SLABS = 64, QP_SLAB_TILES = 8;
constexpr int QP_KG = 8;  // k tiles of one dW task
constexpr float QP_EPS = 1e-10f;

struct QpDims {
  int A, S, NA, H, HA, K;
};

// one Linear(in, hx), ReLU, Linear(hx, nout)
struct QpBlk {
  int64_t W0, b0, W2, b2;
  int ld, hx, nout, onehot;
};

__host__ __device__ inline int64_t qp_n01(const QpDims& d) { return (int64_t)d.H * d.S + d.H + (int64_t)d.A * d.H + d.A; }
__host__ __device__ inline int64_t qp_nkey(const QpDims& d) { return (int64_t)d.HA * d.S + d.HA + d.HA + 1; }
__host__ __device__ inline int64_t qp_nag(const QpDims& d) { return (int64_t)d.HA * d.S + d.HA + (int64_t)d.A * d.HA + d.A; }
__host__ __device__ inline int64_t qp_nac(const QpDims& d) {
  return (int64_t)d.HA * (d.S + d.A * d.NA) + d.HA + (int64_t)d.A * d.HA + d.A;
}
__host__ __device__ inline int64_t qp_total(const QpDims& d) {
  return 2 * qp_n01(d) + d.K * (qp_nkey(d) + qp_nag(d) + qp_nac(d));
}
__host__ __device__ inline int qp_nblk(const QpDims& d) { return 2 + 3 * d.K; }

__host__ __device__ inline QpBlk qp_blk(const QpDims& d, int b) {
  QpBlk k;
  int64_t base;
  k.ld = d.S, k.hx = d.HA, k.nout = d.A, k.onehot = 0;
  if (b < 2) {
    base = b * qp_n01(d), k.hx = d.H;
  } else if (b < 2 + d.K) {
    base = 2 * qp_n01(d) + (b - 2) * qp_nkey(d), k.nout = 1;
  } else if (b < 2 + 2 * d.K) {
    base = 2 * qp_n01(d) + d.K * qp_nkey(d) + (b - 2 - d.K) * qp_nag(d);
  } else {
    base = 2 * qp_n01(d) + d.K * (qp_nkey(d) + qp_nag(d)) + (b - 2 - 2 * d.K) * qp_nac(d);
    k.ld = d.S + d.A * d.NA, k.onehot = 1;
  }
  k.W0 = base;
  k.b0 = k.W0 + (int64_t)k.hx * k.ld;
  k.W2 = k.b0 + k.hx;
  k.b2 = k.W2 + (int64_t)k.nout * k.hx;
  return k;
}

// a work row: per block [h hx][gz hx][gout AP], AP = A rounded up to whole 16-tiles
__host__ __device__ inline int qp_ap(const QpDims& d) { return (d.A + 15) / 16 * 16; }
__host__ __device__ inline int qp_wcol(const QpDims& d, int b) {
  const int n0 = 2 * d.H + qp_ap(d), n1 = 2 * d.HA + qp_ap(d);
  return b < 2 ? b * n0 : 2 * n0 + (b - 2) * n1;
}
__host__ __device__ inline int qp_ws(const QpDims& d) { return qp_wcol(d, qp_nblk(d)); }

T2O_DEV float gsum(float v) {  // Σ over the four lane groups of a row
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}

T2O_DEV float sgnf(float x) { return x > 0.f ? 1.f : x < 0.f ? -1.f : 0.f; }
T2O_DEV float sigmf(float x) { return 1.f / (1.f + expf(-x)); }
__host__ __device__ inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// ---------------------------------------------------------------------------
// selection: the chosen Q, the avail-masked maximum of the network's own Q, the action
struct SelP {
  const float* q[2];
  const int64_t* actions;
  int64_t act_sb, act_st;
  const int32_t* avail;
  int64_t av_sb, av_st;
  float* qv[2];
  float* qmax[2];
  int32_t* act[2];
  int q_ts, NA, mode[2], B, T[2], A;
};

__global__ __launch_bounds__(256) void qplex_sel_kernel(SelP p) {
  const int net = blockIdx.y;
  const int T = p.T[net], mode = p.mode[net];
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)p.B * T * p.A) return;
  const int a = (int)(i % p.A);
  const int64_t bt = i / p.A;
  const int t = (int)(bt % T), b = (int)(bt / T);
  const int NA = p.NA;
  const int64_t qrow = (((int64_t)b * p.q_ts + t) * p.A + a) * NA;
  const int32_t* av = p.avail ? p.avail + b * p.av_sb + t * p.av_st + (int64_t)a * NA : nullptr;
  const float* own = p.q[net];
  int act = 0;
  float best = 0.f, mx = 0.f;
  for (int k = 0; k < NA; ++k) {
    const bool off = av && av[k] == 0;
    const float vo = off ? -9999999.0f : own[qrow + k];
    if (k == 0 || vo > mx) mx = vo;
    if (mode == 2) {
      const float v = off ? -9999999.0f : p.q[0][qrow + k];
      if (k == 0 || v > best) {  // first max wins
        best = v;
        act = k;
      }
    }
  }
  if (mode == 1) {
    const int64_t v = p.actions[b * p.act_sb + t * p.act_st + a];
    act = v < 0 ? 0 : v >= NA ? NA - 1 : (int)v;  // (never in a valid batch; keeps the load in bounds)
  }
  p.qv[net][i] = own[qrow + act];
  p.qmax[net][i] = mx;
  p.act[net][i] = act;
}

// ---------------------------------------------------------------------------
// the pieces of a block on a 16-row tile
template <int NT>
T2O_DEV void bias_init(const float* __restrict__ b, f4* acc) {
  const int g = lane_g();
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[t][r] = b[16 * t + 4 * g + r];
}

// z = W0[:, :S] s + b0: W0 [16·HT][ld] row-major (columns past S clamped: x is 0 there)
template <int HT>
T2O_DEV void hidden(const float* __restrict__ P, const QpBlk& k, int S, const float* __restrict__ st, f4* z) {
  const int c = lane_c(), g = lane_g();
  bias_init<HT>(P + k.b0, z);
  const float* W = P + k.W0;
  for (int k0 = 0; k0 < S; k0 += 16) {
    f4 x;
    int col[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int kk = k0 + 4 * g + s;
      col[s] = min(kk, S - 1);
      const float v = st[col[s]];
      x[s] = kk < S ? v : 0.f;
    }
#pragma unroll
    for (int t = 0; t < HT; ++t) {
      const float* w = W + (int64_t)(16 * t + c) * k.ld;
#pragma unroll
      for (int s = 0; s < 4; ++s) z[t] = mfma4(w[col[s]], x[s], z[t]);
    }
  }
}

// z += Σ_a W0[:, S + a·NA + u_a]: the one-hot columns of d, a gather-add in agent order
template <int HT>
T2O_DEV void onehot_add(const float* __restrict__ P, const QpBlk& k, const QpDims& d, const int32_t* __restrict__ urow,
                        f4* z) {
  const int g = lane_g();
  const float* W = P + k.W0 + d.S + (int64_t)(4 * g) * k.ld;
  for (int a = 0; a < d.A; ++a) {
    const int u = min(max(urow[a], 0), d.NA - 1);
    const float* w = W + a * d.NA + u;
#pragma unroll
    for (int t = 0; t < HT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) z[t][r] += w[(int64_t)(16 * t + r) * k.ld];
  }
}

template <int HT>
T2O_DEV void relu_t(const f4* z, f4* h) {
#pragma unroll
  for (int i = 0; i < HT; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) h[i][r] = fmaxf(z[i][r], 0.f);
}

// out[t] = W2[16t + c][:] · h + b2 for the A outputs (rows past A clamped: masked by the caller)
template <int HT, int AT, bool VEC>
T2O_DEV void lin_out_(const float* __restrict__ W2, const float* __restrict__ b2, int A, const f4* h, f4* out) {
  const int c = lane_c(), g = lane_g();
#pragma unroll
  for (int t = 0; t < AT; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) out[t][r] = b2[min(16 * t + 4 * g + r, A - 1)];
    const float* w = W2 + (int64_t)min(16 * t + c, A - 1) * (16 * HT) + 4 * g;
#pragma unroll
    for (int i = 0; i < HT; ++i) {
      f4 wf;
      if (VEC) wf = ld4(w + 16 * i);
      else wf = f4{w[16 * i], w[16 * i + 1], w[16 * i + 2], w[16 * i + 3]};
#pragma unroll
      for (int s = 0; s < 4; ++s) out[t] = mfma4(wf[s], h[i][s], out[t]);
    }
  }
}

template <int HT, int AT>
T2O_DEV void lin_out(const float* __restrict__ W2, const float* __restrict__ b2, int A, const f4* h, f4* out) {
  if (al16(W2)) lin_out_<HT, AT, true>(W2, b2, A, h, out);  // (uniform: the block's own alignment)
  else lin_out_<HT, AT, false>(W2, b2, A, h, out);
}

// gh += W2ᵀ · gv: W2 [A][16·HT], gv [AT] in the T-layout (0 at the agents past A)
template <int HT, int AT>
T2O_DEV void lin_out_t(const float* __restrict__ W2, int A, const f4* gv, f4* gh) {
  const int c = lane_c(), g = lane_g();
#pragma unroll
  for (int t = 0; t < AT; ++t)
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const float* w = W2 + (int64_t)min(16 * t + 4 * g + s, A - 1) * (16 * HT) + c;
#pragma unroll
      for (int i = 0; i < HT; ++i) gh[i] = mfma4(w[16 * i], gv[t][s], gh[i]);
    }
}

template <int HT>
T2O_DEV float lin_key(const float* __restrict__ W2, float b2, const f4* h) {
  const int g = lane_g();
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < HT; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) s = fmaf(h[i][r], W2[16 * i + 4 * g + r], s);
  return gsum(s) + b2;
}

// a block's pre-activation hidden vector z and its raw output (A outputs, or the key's scalar in out[0][0])
template <int HT, int AT>
T2O_DEV void blk_fwd(const float* __restrict__ P, const QpDims& d, int b, const float* __restrict__ st,
                     const int32_t* __restrict__ urow, f4* z, f4* out, float& key) {
  const QpBlk k = qp_blk(d, b);
  hidden<HT>(P, k, d.S, st, z);
  if (k.onehot) onehot_add<HT>(P, k, d, urow, z);
  f4 h[HT];
  relu_t<HT>(z, h);
  if (k.nout == 1) key = lin_key<HT>(P + k.W2, P[k.b2], h);
  else lin_out<HT, AT>(P + k.W2, P + k.b2, d.A, h, out);
}

template <int AT>
T2O_DEV void blk_fwd_rt(const float* __restrict__ P, const QpDims& d, int b, const float* __restrict__ st,
                        const int32_t* __restrict__ urow, f4* out, float& key) {
  f4 z[4];
  if ((b < 2 ? d.H : d.HA) == 64) blk_fwd<4, AT>(P, d, b, st, urow, z, out, key);
  else blk_fwd<2, AT>(P, d, b, st, urow, z, out, key);
}

// ---------------------------------------------------------------------------
// forward
struct FwdP {
  const float* params[2];
  const float* states;
  int64_t st_sb, st_st;
  const float* qv[2];
  const float* qmax[2];
  const int32_t* act[2];
  float* y[2];
  int T[2];
  int B, parts;
  QpDims d;
};

template <int AT>
__global__ __launch_bounds__(QP_THREADS) void qplex_fwd_kernel(FwdP p) {
  const int net = blockIdx.y;
  const int T = p.T[net];
  const int64_t R = (int64_t)p.B * T;
  const int64_t row0 = ((int64_t)blockIdx.x * QP_WAVES + wave_id()) * 16;
  if (row0 >= R) return;  // (whole waves leave; no workgroup barrier below)
  const int g = lane_g();
  const int64_t row = row0 + lane_c();
  const int64_t rr = row < R ? row : R - 1;  // padding rows read the last row
  const QpDims d = p.d;
  const int A = d.A;
  const float* P = p.params[net];
  const float* st = p.states + (rr / T) * p.st_sb + (rr % T) * p.st_st;
  const int32_t* urow = (p.parts & 2) ? p.act[net] + rr * A : nullptr;
  f4 w[AT], q[AT];
  float key = 0.f;
  blk_fwd_rt<AT>(P, d, 0, st, urow, w, key);
#pragma unroll
  for (int t = 0; t < AT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int a = 16 * t + 4 * g + r;
      w[t][r] = a < A ? fabsf(w[t][r]) + QP_EPS : 0.f;  // (agents past A: every term below is 0)
      q[t][r] = a < A ? p.qv[net][rr * A + a] : 0.f;
    }
  float y = 0.f;
  if (p.parts & 1) {
    f4 v[AT];
    blk_fwd_rt<AT>(P, d, 1, st, urow, v, key);
#pragma unroll
    for (int t = 0; t < AT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) y += 16 * t + 4 * g + r < A ? fmaf(w[t][r], q[t][r], v[t][r]) : 0.f;
  }
  if (p.parts & 2) {
    f4 lam[AT];
#pragma unroll
    for (int t = 0; t < AT; ++t) lam[t] = zero4();
    for (int k = 0; k < d.K; ++k) {
      f4 al[AT], be[AT];
      blk_fwd_rt<AT>(P, d, 2 + k, st, urow, al, key);
      const float kap = fabsf(key) + QP_EPS;
      blk_fwd_rt<AT>(P, d, 2 + d.K + k, st, urow, al, key);
      blk_fwd_rt<AT>(P, d, 2 + 2 * d.K + k, st, urow, be, key);
#pragma unroll
      for (int t = 0; t < AT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) lam[t][r] = fmaf(kap, sigmf(al[t][r]) * sigmf(be[t][r]), lam[t][r]);
    }
#pragma unroll
    for (int t = 0; t < AT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int a = 16 * t + 4 * g + r;
        const float m = a < A ? p.qmax[net][rr * A + a] : 0.f;
        y += a < A ? w[t][r] * (q[t][r] - m) * (lam[t][r] - 1.f) : 0.f;
      }
  }
  y = gsum(y);
  if (g == 0 && row < R) p.y[net][row] = y;
}

// ---------------------------------------------------------------------------
// backward, rows
struct RowsP {
  const float* params;
  const float* states;
  int64_t st_sb, st_st;
  const float* qv;
  const float* qmax;
  const int32_t* act;
  const float* gy;
  float* gqv;
  float* work;
  int T, B, parts;
  QpDims d;
};

template <int NT>
T2O_DEV void store_t(float* wrow, int col, const f4* v) {
  const int g = lane_g();
#pragma unroll
  for (int t = 0; t < NT; ++t) *reinterpret_cast<f4*>(wrow + col + 16 * t + 4 * g) = v[t];
}

// from a block's z and the gradient of its output: h, gz = [z > 0] · W2ᵀ gout, gout into the work row
template <int HT, int AT>
T2O_DEV void blk_bwd(const float* __restrict__ P, const QpDims& d, int b, const f4* z, const f4* gout, float gkey,
                     float* wrow) {
  const QpBlk k = qp_blk(d, b);
  const int g = lane_g();
  f4 h[HT], gh[HT], go[AT];
  relu_t<HT>(z, h);
  if (k.nout == 1) {
#pragma unroll
    for (int i = 0; i < HT; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) gh[i][r] = P[k.W2 + 16 * i + 4 * g + r] * gkey;
#pragma unroll
    for (int t = 0; t < AT; ++t) go[t] = zero4();
    if (g == 0) go[0][0] = gkey;
  } else {
#pragma unroll
    for (int i = 0; i < HT; ++i) gh[i] = zero4();
#pragma unroll
    for (int t = 0; t < AT; ++t) go[t] = gout[t];
    lin_out_t<HT, AT>(P + k.W2, d.A, go, gh);
  }
#pragma unroll
  for (int i = 0; i < HT; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) gh[i][r] = z[i][r] > 0.f ? gh[i][r] : 0.f;
  const int col = qp_wcol(d, b);
  store_t<HT>(wrow, col, h);
  store_t<HT>(wrow, col + k.hx, gh);
  store_t<AT>(wrow, col + 2 * k.hx, go);
}

struct RowCtx {
  const float* P;
  const float* st;
  const int32_t* urow;
  float* wrow;
};

// blocks 0 and 1 (hidden width H): w, dL/dq, the gradients of hyper_w_final and V; returns w
template <int HT, int AT>
T2O_DEV void rows_head(const RowCtx& x, const QpDims& d, float gyv, const f4* q, bool live, float* gq, f4* w) {
  const int g = lane_g(), A = d.A;
  f4 z[HT], go[AT];
  float key = 0.f;
  blk_fwd<HT, AT>(x.P, d, 0, x.st, x.urow, z, w, key);
#pragma unroll
  for (int t = 0; t < AT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int a = 16 * t + 4 * g + r;
      const float raw = w[t][r];
      w[t][r] = a < A ? fabsf(raw) + QP_EPS : 0.f;
      go[t][r] = a < A ? gyv * q[t][r] * sgnf(raw) : 0.f;
      if (a < A && live) gq[a] = gyv * w[t][r];
    }
  blk_bwd<HT, AT>(x.P, d, 0, z, go, 0.f, x.wrow);
  f4 v[AT];
  blk_fwd<HT, AT>(x.P, d, 1, x.st, x.urow, z, v, key);
#pragma unroll
  for (int t = 0; t < AT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) go[t][r] = 16 * t + 4 * g + r < A ? gyv : 0.f;
  blk_bwd<HT, AT>(x.P, d, 1, z, go, 0.f, x.wrow);
}

// kernel k of si_weight (hidden width HA): glam = dL/dλ, 0 at the agents past A
template <int HT, int AT>
T2O_DEV void rows_si(const RowCtx& x, const QpDims& d, int k, const f4* glam) {
  f4 zk[HT], za[HT], zb[HT], al[AT], be[AT], none[AT];
  float key = 0.f, unused = 0.f;
  blk_fwd<HT, AT>(x.P, d, 2 + k, x.st, x.urow, zk, none, key);
  blk_fwd<HT, AT>(x.P, d, 2 + d.K + k, x.st, x.urow, za, al, unused);
  blk_fwd<HT, AT>(x.P, d, 2 + 2 * d.K + k, x.st, x.urow, zb, be, unused);
  const float kap = fabsf(key) + QP_EPS;
  float gk = 0.f;
  f4 ga[AT], gb[AT];
#pragma unroll
  for (int t = 0; t < AT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float a_ = sigmf(al[t][r]), b_ = sigmf(be[t][r]), gl = glam[t][r];
      gk = fmaf(gl, a_ * b_, gk);
      ga[t][r] = gl * kap * b_ * a_ * (1.f - a_);
      gb[t][r] = gl * kap * a_ * b_ * (1.f - b_);
    }
  gk = gsum(gk) * sgnf(key);
  blk_bwd<HT, AT>(x.P, d, 2 + k, zk, none, gk, x.wrow);
  blk_bwd<HT, AT>(x.P, d, 2 + d.K + k, za, ga, 0.f, x.wrow);
  blk_bwd<HT, AT>(x.P, d, 2 + 2 * d.K + k, zb, gb, 0.f, x.wrow);
}

template <int AT>
__global__ __launch_bounds__(QP_THREADS) void qplex_bwd_rows_kernel(RowsP p) {
  const int T = p.T;
  const int64_t R = (int64_t)p.B * T;
  const int64_t row0 = ((int64_t)blockIdx.x * QP_WAVES + wave_id()) * 16;
  if (row0 >= R) return;
  const int g = lane_g();
  const int64_t row = row0 + lane_c();
  const bool live = row < R;
  const int64_t rr = live ? row : R - 1;
  const QpDims d = p.d;
  const int A = d.A;
  RowCtx x;
  x.P = p.params;
  x.st = p.states + (rr / T) * p.st_sb + (rr % T) * p.st_st;
  x.urow = p.act + rr * A;
  x.wrow = p.work + row * qp_ws(d);  // (the work buffer holds whole tiles)
  const float gy = live ? p.gy[row] : 0.f;  // padding rows: every gradient below is 0
  const float gyv = (p.parts & 1) ? gy : 0.f, gya = (p.parts & 2) ? gy : 0.f;
  f4 q[AT], w[AT], glam[AT];
#pragma unroll
  for (int t = 0; t < AT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int a = 16 * t + 4 * g + r;
      q[t][r] = a < A ? p.qv[rr * A + a] : 0.f;
    }
  float* gq = p.gqv + rr * A;
  if (d.H == 64) rows_head<4, AT>(x, d, gyv, q, live, gq, w);
  else rows_head<2, AT>(x, d, gyv, q, live, gq, w);
#pragma unroll
  for (int t = 0; t < AT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int a = 16 * t + 4 * g + r;
      const float m = a < A ? p.qmax[rr * A + a] : 0.f;
      glam[t][r] = a < A ? gya * (w[t][r] * (q[t][r] - m)) : 0.f;  // c = w (q − m): a constant
    }
  for (int k = 0; k < d.K; ++k) {
    if (d.HA == 64) rows_si<4, AT>(x, d, k, glam);
    else rows_si<2, AT>(x, d, k, glam);
  }
}

// ---------------------------------------------------------------------------
// backward, weight gradients
struct DwP {
  const float* states;
  int64_t st_sb, st_st;
  const int32_t* act;
  const float* work;
  float* slabs;
  int64_t R, ntiles;
  int T, tps;  // tps: row tiles per slab
  QpDims d;
};

// one task: a 16-row tile of outputs o against up to QP_KG 16-column tiles of k
struct DwTask {
  int pcol, no;        // P: work column of the tile's first output, valid outputs
  int qmode, qcol;     // Q: 0 a work column, 1 the states, 2 the one-hot of the actions
  int nk, k0;          // Q's width, the task's first column
  int64_t wdst, bdst;  // slab offsets of W[o0][0] and its bias (-1: another task writes it)
  int ldw;
};

__host__ __device__ inline int qp_kgn(int n) { return ((n + 15) / 16 + QP_KG - 1) / QP_KG; }

// the tasks of block b: first weight against the states, its one-hot columns, second weight
__host__ __device__ inline int qp_blk_tasks(const QpDims& d, const QpBlk& k) {
  const int ht = k.hx / 16;
  return ht * qp_kgn(d.S) + (k.onehot ? ht * qp_kgn(d.A * d.NA) : 0) + (k.nout == 1 ? 1 : (d.A + 15) / 16);
}

__host__ __device__ inline int qp_tasks(const QpDims& d) {
  int n = 0;
  for (int b = 0; b < qp_nblk(d); ++b) n += qp_blk_tasks(d, qp_blk(d, b));
  return n;
}

__device__ inline DwTask dw_task(int y, const QpDims& d) {
  const int KGs = qp_kgn(d.S), KGo = qp_kgn(d.A * d.NA);
  int b = 0;
  QpBlk k = qp_blk(d, 0);
  for (;; ++b) {  // (y < qp_tasks(d): the grid's size)
    k = qp_blk(d, b);
    const int n = qp_blk_tasks(d, k);
    if (y < n || b == qp_nblk(d) - 1) break;
    y -= n;
  }
  const int col = qp_wcol(d, b), ht = k.hx / 16;
  if (y < ht * KGs) {
    const int ot = y / KGs, kg = y % KGs;
    return DwTask{col + k.hx + 16 * ot, 16, 1, 0, d.S, kg * QP_KG * 16, k.W0 + (int64_t)16 * ot * k.ld,
                  kg == 0 ? k.b0 + 16 * ot : -1, k.ld};
  }
  y -= ht * KGs;
  if (k.onehot && y < ht * KGo) {
    const int ot = y / KGo, kg = y % KGo;
    return DwTask{col + k.hx + 16 * ot, 16, 2, 0, d.A * d.NA, kg * QP_KG * 16, k.W0 + (int64_t)16 * ot * k.ld + d.S,
                  -1, k.ld};
  }
  if (k.onehot) y -= ht * KGo;
  const int no = k.nout - 16 * y;
  return DwTask{col + 2 * k.hx + 16 * y, no < 16 ? no : 16, 0, col, k.hx, 0, k.W2 + (int64_t)16 * y * k.hx,
                k.b2 + 16 * y, k.hx};
}

__global__ __launch_bounds__(QP_THREADS) void qplex_dw_kernel(DwP p) {
  constexpr int NACC = QP_KG + 1;
  __shared__ f4 red[QP_WAVES * NACC * 64];
  const int slab = blockIdx.x, wv = wave_id();
  const int c = lane_c(), g = lane_g(), lane = threadIdx.x & 63;
  const QpDims d = p.d;
  const int ws = qp_ws(d);
  const DwTask t = dw_task(blockIdx.y, d);
  const int nkt = min(QP_KG, (t.nk - t.k0 + 15) / 16);
  f4 acc[NACC];
#pragma unroll
  for (int j = 0; j < NACC; ++j) acc[j] = zero4();
  const int64_t lo = (int64_t)slab * p.tps, hi = min(lo + p.tps, p.ntiles);
  for (int64_t tile = lo + wv; tile < hi; tile += QP_WAVES) {
    const int64_t row0 = tile * 16;
    f4 pa;
    const float* qrow[4];
    const int32_t* urow[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int64_t row = row0 + 4 * g + s;
      const float* wr = p.work + row * ws;
      const float v = wr[t.pcol + (c < t.no ? c : 0)];
      pa[s] = c < t.no ? v : 0.f;
      const int64_t rr = row < p.R ? row : p.R - 1;  // (padding rows: P is 0 there)
      qrow[s] = t.qmode == 1 ? p.states + (rr / p.T) * p.st_sb + (rr % p.T) * p.st_st : wr + t.qcol;
      urow[s] = p.act + rr * d.A;
    }
#pragma unroll
    for (int j = 0; j < QP_KG; ++j) {
      if (j < nkt) {
        const int k = t.k0 + 16 * j + c, kc = min(k, t.nk - 1);
        if (t.qmode == 2) {
          // one-hot operand fragments on the MFMA K axis: Q[row][a·NA + n] = [u[row][a] == n]
          const int a = kc / d.NA, n = kc % d.NA;
#pragma unroll
          for (int s = 0; s < 4; ++s)
            acc[j] = mfma4(pa[s], (k < t.nk && urow[s][a] == n) ? 1.f : 0.f, acc[j]);
        } else {
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            const float v = qrow[s][kc];
            acc[j] = mfma4(pa[s], k < t.nk ? v : 0.f, acc[j]);
          }
        }
      }
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) acc[QP_KG] = mfma4(pa[s], 1.f, acc[QP_KG]);
  }
#pragma unroll
  for (int j = 0; j < NACC; ++j) red[(wv * NACC + j) * 64 + lane] = acc[j];
  __syncthreads();
  float* out = p.slabs + (int64_t)slab * qp_total(d);
  for (int idx = threadIdx.x; idx < NACC * 64; idx += QP_THREADS) {
    const int j = idx / 64, l = idx % 64, lc = l & 15, lg = l >> 4;
    f4 v = red[(0 * NACC + j) * 64 + l];
#pragma unroll
    for (int w = 1; w < QP_WAVES; ++w) v += red[(w * NACC + j) * 64 + l];
    if (j < QP_KG) {
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
bool dims_ok(int A, int S, int NA, int H, int HA, int K) {
  return A >= 1 && A <= QP_MAXA && S >= 1 && S <= QP_MAXS && NA >= 1 && NA <= QP_MAXNA && (H == 32 || H == 64) &&
         (HA == 32 || HA == 64) && K >= 1 && K <= QP_MAXK;
}

bool rows_ok(int B, int T) { return B >= 1 && T >= 1 && (int64_t)B * T < (1ll << 27); }

int slabs_of(int B, int T) {
  const int64_t ntiles = ((int64_t)B * T + 15) / 16;
  const int64_t n = ntiles / QP_SLAB_TILES;
  return (int)(n < 1 ? 1 : n > QP_MAX_SLABS ? QP_MAX_SLABS : n);
}

// kernel<AT> for the A's 16-tiles
#define T2O_QPLEX_DISPATCH(KERNEL, A, ...)                                   \
  do {                                                                       \
    if ((A) <= 16) hipLaunchKernelGGL((KERNEL<1>), __VA_ARGS__);             \
    else if ((A) <= 32) hipLaunchKernelGGL((KERNEL<2>), __VA_ARGS__);        \
    else if ((A) <= 48) hipLaunchKernelGGL((KERNEL<3>), __VA_ARGS__);        \
    else hipLaunchKernelGGL((KERNEL<4>), __VA_ARGS__);                       \
  } while (0)

}  // namespace

extern "C" int64_t t2o_qplex_param_count(int A, int S, int NA, int H, int HA, int K) {
  if (!dims_ok(A, S, NA, H, HA, K)) return T2O_EINVAL;
  return qp_total(QpDims{A, S, NA, H, HA, K});
}

extern "C" int t2o_qplex_select(const t2o_qplex_select_args* a, void* stream) {
  if (!a || !a->q_on || !a->qv_on || !a->qmax_on || !a->act_on) return T2O_EINVAL;
  if (a->B < 1 || a->T_on < 1 || a->A < 1 || a->A > QP_MAXA || a->n_actions < 1 || a->n_actions > QP_MAXNA)
    return T2O_EINVAL;
  if (a->q_ts < a->T_on || (int64_t)a->B * a->q_ts >= (1ll << 27)) return T2O_EINVAL;
  if (a->qmode_on != 1 && a->qmode_on != 2) return T2O_EINVAL;
  const bool two = a->q_tg != nullptr;
  if (two && (!a->qv_tg || !a->qmax_tg || !a->act_tg || a->T_tg < 1 || a->T_tg > a->q_ts ||
              (a->qmode_tg != 1 && a->qmode_tg != 2)))
    return T2O_EINVAL;
  if ((a->qmode_on == 1 || (two && a->qmode_tg == 1)) && !a->actions) return T2O_EINVAL;
  SelP p{};
  p.q[0] = a->q_on, p.q[1] = a->q_tg;
  p.actions = a->actions, p.act_sb = a->act_sb, p.act_st = a->act_st;
  p.avail = a->avail, p.av_sb = a->av_sb, p.av_st = a->av_st;
  p.qv[0] = a->qv_on, p.qv[1] = a->qv_tg, p.qmax[0] = a->qmax_on, p.qmax[1] = a->qmax_tg;
  p.act[0] = a->act_on, p.act[1] = a->act_tg;
  p.q_ts = a->q_ts, p.NA = a->n_actions, p.mode[0] = a->qmode_on, p.mode[1] = two ? a->qmode_tg : 0;
  p.B = a->B, p.T[0] = a->T_on, p.T[1] = two ? a->T_tg : 0, p.A = a->A;
  const int Tmax = two && a->T_tg > a->T_on ? a->T_tg : a->T_on;
  const int64_t n = (int64_t)a->B * Tmax * a->A;
  hipLaunchKernelGGL(qplex_sel_kernel, dim3((unsigned)((n + 255) / 256), two ? 2 : 1), dim3(256), 0,
                     (hipStream_t)stream, p);
  return (int)hipGetLastError();
}

extern "C" int t2o_qplex_fwd(const t2o_qplex_fwd_args* a, void* stream) {
  if (!a || !a->params_on || !a->states || !a->qv_on || !a->y_on) return T2O_EINVAL;
  if (!dims_ok(a->A, a->S, a->NA, a->H, a->HA, a->K) || !rows_ok(a->B, a->T_on)) return T2O_EINVAL;
  if (a->parts < 1 || a->parts > 3) return T2O_EINVAL;
  const bool adv = (a->parts & 2) != 0;
  if (adv && (!a->qmax_on || !a->act_on)) return T2O_EINVAL;
  const bool two = a->params_tg != nullptr;
  if (two && (!a->qv_tg || !a->y_tg || !rows_ok(a->B, a->T_tg) || (adv && (!a->qmax_tg || !a->act_tg))))
    return T2O_EINVAL;
  FwdP p{};
  p.params[0] = a->params_on, p.params[1] = a->params_tg;
  p.states = a->states, p.st_sb = a->st_sb, p.st_st = a->st_st;
  p.qv[0] = a->qv_on, p.qv[1] = a->qv_tg, p.qmax[0] = a->qmax_on, p.qmax[1] = a->qmax_tg;
  p.act[0] = a->act_on, p.act[1] = a->act_tg;
  p.y[0] = a->y_on, p.y[1] = a->y_tg;
  p.T[0] = a->T_on, p.T[1] = two ? a->T_tg : 0;
  p.B = a->B, p.parts = a->parts;
  p.d = QpDims{a->A, a->S, a->NA, a->H, a->HA, a->K};
  const int Tmax = two && a->T_tg > a->T_on ? a->T_tg : a->T_on;
  const int64_t ntiles = ((int64_t)a->B * Tmax + 15) / 16;
  const dim3 grid((unsigned)((ntiles + QP_WAVES - 1) / QP_WAVES), two ? 2 : 1), block(QP_THREADS);
  T2O_QPLEX_DISPATCH(qplex_fwd_kernel, a->A, grid, block, 0, (hipStream_t)stream, p);
  return (int)hipGetLastError();
}

extern "C" int t2o_qplex_bwd_slabs(int B, int T) {
  if (!rows_ok(B, T)) return T2O_EINVAL;
  return slabs_of(B, T);
}

extern "C" int64_t t2o_qplex_bwd_work_floats(int B, int T, int A, int H, int HA, int K) {
  if (!rows_ok(B, T) || !dims_ok(A, 1, 1, H, HA, K)) return T2O_EINVAL;
  return (((int64_t)B * T + 15) / 16) * 16 * qp_ws(QpDims{A, 1, 1, H, HA, K});
}

extern "C" int t2o_qplex_bwd(const t2o_qplex_bwd_args* a, void* stream) {
  if (!a || !a->params || !a->states || !a->qv || !a->qmax || !a->act || !a->work) return T2O_EINVAL;
  if (a->phase < 0 || a->phase > 2 || a->parts < 1 || a->parts > 3) return T2O_EINVAL;
  if (a->phase != 2 && (!a->gy || !a->gqv)) return T2O_EINVAL;
  if (a->phase != 1 && !a->gslabs) return T2O_EINVAL;
  if (!dims_ok(a->A, a->S, a->NA, a->H, a->HA, a->K) || !rows_ok(a->B, a->T)) return T2O_EINVAL;
  if (!al16(a->work) || a->work_floats < t2o_qplex_bwd_work_floats(a->B, a->T, a->A, a->H, a->HA, a->K))
    return T2O_EINVAL;
  const int nslab = slabs_of(a->B, a->T);
  if (a->phase != 1 && a->max_slabs < nslab) return T2O_EINVAL;
  const QpDims d{a->A, a->S, a->NA, a->H, a->HA, a->K};
  const int64_t R = (int64_t)a->B * a->T, ntiles = (R + 15) / 16;
  hipStream_t st = (hipStream_t)stream;
  const dim3 block(QP_THREADS);
  if (a->phase != 2) {
    RowsP p{};
    p.params = a->params, p.states = a->states, p.st_sb = a->st_sb, p.st_st = a->st_st;
    p.qv = a->qv, p.qmax = a->qmax, p.act = a->act, p.gy = a->gy, p.gqv = a->gqv, p.work = a->work;
    p.T = a->T, p.B = a->B, p.parts = a->parts, p.d = d;
    const dim3 grid((unsigned)((ntiles + QP_WAVES - 1) / QP_WAVES));
    T2O_QPLEX_DISPATCH(qplex_bwd_rows_kernel, a->A, grid, block, 0, st, p);
  }
  if (a->phase != 1) {
    DwP p{};
    p.states = a->states, p.st_sb = a->st_sb, p.st_st = a->st_st, p.act = a->act, p.work = a->work;
    p.slabs = a->gslabs, p.R = R, p.ntiles = ntiles, p.T = a->T;
    p.tps = (int)((ntiles + nslab - 1) / nslab), p.d = d;
    hipLaunchKernelGGL(qplex_dw_kernel, dim3((unsigned)nslab, (unsigned)qp_tasks(d)), block, 0, st, p);
  }
  return (int)hipGetLastError();
}
