// t2o_stats.hip — the logged training / evaluation statistics, summed on the device.
//
// The reference's runner ends every run by summing the terminated envs' info
// dicts and the episode returns (parallel_runner.py:202-210) and logs their means
// (:223-231); a PyMARL2 NQLearner logs the masked means of |td|, Qtot and the
// targets every learner_log_interval steps.  Both are plain sums over a few
// thousand values, so each entry point is ONE workgroup:
//   * every thread sums the elements tid, tid + STAT_THREADS, ... in fp64,
//   * a wave sums its 64 lanes with an xor butterfly (shuffles on doubles),
//   * thread 0 adds the STAT_WAVES wave sums in wave order.
// No atomics and no dependence on the grid: the summation tree is a function of
// the element count alone, so a logged value is bit-identical run to run and on
// any device.
#include "t2o_common.hpp"

namespace {

constexpr int STAT_THREADS = 1024;
constexpr int STAT_WAVES = STAT_THREADS / 64;

// Sum NV per-thread doubles over the workgroup; the totals are valid in thread 0.
template <int NV>
__device__ void block_sum_f64(double (&v)[NV], double (*red)[NV]) {
#pragma unroll
  for (int k = 0; k < NV; ++k)
    for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o);
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  if (l == 0) {
#pragma unroll
    for (int k = 0; k < NV; ++k) red[w][k] = v[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      double s = red[0][k];
      for (int i = 1; i < STAT_WAVES; ++i) s += red[i][k];
      v[k] = s;
    }
  }
}

// sums: 0 returns; then over terminated envs 1 reward, 2..5 info[0..3], 6 count, 7..8 info[4..5]
constexpr int EP_SUMS = T2O_EP_STATS - 1;

__global__ __launch_bounds__(STAT_THREADS) void episode_stats_kernel(const double* __restrict__ reward,
                                                                     const double* __restrict__ info,
                                                                     const uint8_t* __restrict__ terminated,
                                                                     const double* __restrict__ returns, int64_t n,
                                                                     double* __restrict__ acc) {
  __shared__ double red[STAT_WAVES][EP_SUMS];
  double v[EP_SUMS];
#pragma unroll
  for (int k = 0; k < EP_SUMS; ++k) v[k] = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += STAT_THREADS) {
    v[0] += returns[i];
    if (terminated[i] != 0) {  // (an unterminated env's task_completion_* are NaN: never read)
      const double* r = info + i * 6;
      v[1] += reward[i];
      v[2] += r[0];
      v[3] += r[1];
      v[4] += r[2];
      v[5] += r[3];
      v[6] += 1.0;
      v[7] += r[4];
      v[8] += r[5];
    }
  }
  block_sum_f64<EP_SUMS>(v, red);
  if (threadIdx.x == 0) {
    acc[0] += (double)n;
#pragma unroll
    for (int k = 0; k < EP_SUMS; ++k) acc[1 + k] += v[k];
  }
}

// one 0/1 mask element of the given storage type as double
__device__ double mask_f64(const void* p, int64_t i, int dt) {
  switch (dt) {
    case T2O_DT_U8: return (double)static_cast<const uint8_t*>(p)[i];
    case T2O_DT_I32: return (double)static_cast<const int32_t*>(p)[i];
    case T2O_DT_I64: return (double)static_cast<const int64_t*>(p)[i];
    default: return (double)static_cast<const float*>(p)[i];
  }
}

__global__ __launch_bounds__(STAT_THREADS) void td_stats_kernel(t2o_td_stats_args a) {
  __shared__ double red[STAT_WAVES][4];
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  const int64_t T = a.T, n = (int64_t)a.B * T;
  for (int64_t i = threadIdx.x; i < n; i += STAT_THREADS) {
    const int64_t b = i / T, t = i - b * T;
    // mask[b][t] = filled[t] * (t == 0 ? 1 : 1 - term[t-1]), as t2o_td_loss
    double m = a.filled ? mask_f64(a.filled, b * a.fl_sb + t * a.fl_st, a.filled_dtype) : 1.0;
    if (t > 0 && a.term) m *= 1.0 - mask_f64(a.term, b * a.tm_sb + (t - 1) * a.tm_st, a.term_dtype);
    const double q = (double)a.qtot[i], g = (double)a.targets[i];
    v[0] += m;
    v[1] += fabs(q - g) * m;
    v[2] += q * m;
    v[3] += g * m;
  }
  block_sum_f64<4>(v, red);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) a.out[k] = v[k];
  }
}

}  // namespace

extern "C" int t2o_episode_stats(const double* reward, const double* info, const uint8_t* terminated,
                                 const double* returns, int64_t n, double* acc, void* stream) {
  if (!reward || !info || !terminated || !returns || !acc || n < 1) return T2O_EINVAL;
  hipLaunchKernelGGL(episode_stats_kernel, dim3(1), dim3(STAT_THREADS), 0, (hipStream_t)stream, reward, info,
                     terminated, returns, n, acc);
  return (int)hipGetLastError();
}

extern "C" int t2o_td_stats(const t2o_td_stats_args* a, void* stream) {
  if (!a || !a->qtot || !a->targets || !a->out || a->B < 1 || a->T < 1) return T2O_EINVAL;
  auto dt_ok = [](int dt) { return dt == T2O_DT_F32 || dt == T2O_DT_U8 || dt == T2O_DT_I32 || dt == T2O_DT_I64; };
  if (!dt_ok(a->term_dtype) || !dt_ok(a->filled_dtype)) return T2O_EINVAL;
  hipLaunchKernelGGL(td_stats_kernel, dim3(1), dim3(STAT_THREADS), 0, (hipStream_t)stream, *a);
  return (int)hipGetLastError();
}
