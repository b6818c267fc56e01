// BatchNorm statistics shared by the ranks of a process group (torch.nn.SyncBatchNorm semantics), for both BatchNorm pipelines:
// bn.hip (fp32 [N, C], C <= 256) and mlp_layers.hip (activations [N, 128] in bf16 or fp32 storage).  Stage one of either pipeline
// (its per-workgroup fp32 column sums, shifted by row 0 in the forward) is unchanged; its finish is split in two around ONE
// all-reduce that the caller runs:
//
//   record (per rank)   partials -> a double record of R = 2 C + 1 entries: [n_r | a[C] | b[C]]
//                       forward:  a = mean_r = shift + t1 / n_r,  b = M2_r = t2 - t1^2 / n_r
//                       backward: a = sum gu,  b = sum gu xhat  (xhat with the GLOBAL mean / invstd of the forward); the same two
//                       sums as floats are this rank's dbeta / dgamma
//   merge (every rank)  records [world][R] -> the finish's outputs, in the same layout.  Forward: Chan's pairwise update in rank
//                       order (d = mean_b - mean_a, M2 = M2_a + M2_b + d^2 n_a n_b / n) -> mean, biased var = M2 / N, invstd,
//                       scale = gamma invstd, shift = beta - mean scale, and the running-buffer update with the GLOBAL N.
//                       Backward: the sums added in rank order -> gs = gamma invstd, k1 = sum dbeta / N, k2 = sum dgamma / N.
//
// Both stages only see partials or records, so one pair of kernels serves the three storages.  Deterministic (fixed-order sums in
// double), no atomics, no allocation, no host synchronisation: the launches can sit in a captured graph.
#pragma once

#include "common.hpp"

namespace mlqem {

constexpr int kSyncThreads = 256;

// One workgroup per output column (opitch of them; columns >= C write zeros to o1 / o2 and no record entry).  partial:
// [nblocks][2][pitch] floats; shift: the per-column shift of the forward sums (MODE 0).  MODE 1 also writes this rank's sums
// as floats to o1 (s1 = dbeta) and o2 (s2 = dgamma) when they are given.
template <int MODE>
__global__ __launch_bounds__(kSyncThreads) void bn_sync_record_kernel(const float* __restrict__ partial, int nblocks, int pitch,
                                                                      int64_t N, int C, const float* __restrict__ shift,
                                                                      double* __restrict__ rec, float* __restrict__ o1,
                                                                      float* __restrict__ o2) {
  __shared__ double s_t[2][kSyncThreads];
  const int c = blockIdx.x, j = threadIdx.x;
  if (c >= C) {
    if (j == 0 && o1) o1[c] = 0.f;
    if (j == 0 && o2) o2[c] = 0.f;
    return;
  }
  double t1 = 0.0, t2 = 0.0;
  for (int b = j; b < nblocks; b += kSyncThreads) {
    t1 += (double)partial[((int64_t)b * 2 + 0) * pitch + c];
    t2 += (double)partial[((int64_t)b * 2 + 1) * pitch + c];
  }
  s_t[0][j] = t1;
  s_t[1][j] = t2;
  __syncthreads();
#pragma unroll
  for (int half = kSyncThreads / 2; half >= 1; half >>= 1) {      // a fixed tree over the thread sums
    if (j < half) { s_t[0][j] += s_t[0][j + half]; s_t[1][j] += s_t[1][j + half]; }
    __syncthreads();
  }
  if (j != 0) return;
  t1 = s_t[0][0];
  t2 = s_t[1][0];
  const double n = (double)N;
  if (c == 0) rec[0] = n;
  if (MODE == 0) {
    double m2 = t2 - t1 * t1 / n;
    if (m2 < 0.0) m2 = 0.0;
    rec[1 + c] = (double)shift[c] + t1 / n;
    rec[1 + C + c] = m2;
  } else {
    rec[1 + c] = t1;
    rec[1 + C + c] = t2;
    if (o1) o1[c] = (float)t1;
    if (o2) o2[c] = (float)t2;
  }
}

// One thread per output column; columns in [C, opitch) get zeros.  rec: [world][2 C + 1] doubles, merged in rank order (a rank
// with no rows -- an all-zero record -- is skipped).
// MODE 0 -> o1..o5 = mean, biased var, invstd, scale, shift; running buffers (when given) and the batch counter updated once.
// MODE 1 -> o3..o5 = gs = gamma invstd_in, k1, k2 (o1 / o2 are the record stage's local sums and are not touched).
template <int MODE>
__global__ __launch_bounds__(kSyncThreads) void bn_sync_merge_kernel(const double* __restrict__ rec, int world, int C, int opitch,
                                                                     const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                     const float* __restrict__ invstd_in, float eps, float* __restrict__ o1,
                                                                     float* __restrict__ o2, float* __restrict__ o3, float* __restrict__ o4,
                                                                     float* __restrict__ o5, float* __restrict__ run_mean,
                                                                     float* __restrict__ run_var, float momentum,
                                                                     long long* __restrict__ batches) {
  const int c = blockIdx.x * kSyncThreads + threadIdx.x;
  if (c >= opitch) return;
  if (c >= C) {
    if (MODE == 0) { o1[c] = 0.f; o2[c] = 0.f; }
    o3[c] = 0.f; o4[c] = 0.f; o5[c] = 0.f;
    return;
  }
  const int64_t R = 2 * (int64_t)C + 1;
  double n = 0.0, a = 0.0, b = 0.0;
  for (int r = 0; r < world; ++r) {
    const double* q = rec + r * R;
    const double nb = q[0];
    if (!(nb > 0.0)) continue;
    if (MODE == 0) {
      const double nn = n + nb, d = q[1 + c] - a;
      a += d * (nb / nn);
      b += q[1 + C + c] + d * d * (n * nb / nn);
      n = nn;
    } else {
      n += nb;
      a += q[1 + c];
      b += q[1 + C + c];
    }
  }
  const float g = gamma ? gamma[c] : 1.f;
  if (MODE == 0) {
    const double var = n > 0.0 ? b / n : 0.0;
    const float is = (float)(1.0 / sqrt(var + (double)eps));
    const float sc = g * is;
    o1[c] = (float)a; o2[c] = (float)var; o3[c] = is; o4[c] = sc; o5[c] = (beta ? beta[c] : 0.f) - (float)a * sc;
    if (run_mean) {
      const float unbias = n > 1.0 ? (float)n / (float)(n - 1.0) : 1.f;
      run_mean[c] = (1.f - momentum) * run_mean[c] + momentum * (float)a;
      run_var[c] = (1.f - momentum) * run_var[c] + momentum * ((float)var * unbias);
    }
    if (batches && c == 0) *batches += 1;
  } else {
    o3[c] = g * invstd_in[c];
    o4[c] = n > 0.0 ? (float)(a / n) : 0.f;
    o5[c] = n > 0.0 ? (float)(b / n) : 0.f;
  }
}

}  // namespace mlqem
