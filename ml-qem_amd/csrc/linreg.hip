// Linear least squares on encode_data rows: the fit's streaming pass (mlqem_linreg_moments_f32) and scoring (mlqem_linreg_predict_f32).
//
// Moments.  With A = [1 | x | y] (n x D, D = 1 + F + K) the call forms M = A^T A in float64.  The float32 inputs are widened to
// fp64 before they are multiplied, so every product is exact (24 + 24 bits <= 53) and only the additions round.
//   * The output is cut into 64 x 64 tiles and only the tiles of the lower triangle (ti >= tj) are computed; the final kernel writes
//     M[i, j] and M[j, i] from the same sum, so the matrix is symmetric to the last bit.
//   * The rows are cut into `splits` chunks of `chunk_rows` rows; both are functions of (n, F, K) alone (moments_plan).  Workgroup
//     (tile, split) walks its chunk in slabs of 32 rows: the slab's columns of the two tiles are staged in LDS as float32 (coalesced
//     256-byte reads along a row, the next slab's fetched while this one is multiplied; rows past n and columns past D are staged
//     as zeros, column 0 as 1).  Each of the four waves owns a 32 x 32 quarter of the tile as 2 x 2 blocks of
//     v_mfma_f64_16x16x4_f64 and feeds it four slab rows at a time, in row order.  (fp64 vector FMAs on 4 x 4 register blocks
//     took 1.32-1.41 x the time on the device: DESIGN.md section 3.5.)
//   * A workgroup's tile goes to the caller's workspace ([tile][split][64][64] doubles); mlqem_linreg_moments_workspace_bytes sizes
//     it.  The final kernel adds the splits of every entry in a fixed order (onto the old value when `accumulate`).  No atomics: the
//     order of every sum is fixed by (n, F, K), and two calls give the same bits.
// Every load is unconditional: a lane past the data reads a clamped address and a select discards the value.
//
// Predict.  out[r, k] = intercept[k] + sum_j coef[k, j] x[r, j]: one thread per row holds the K sums in registers and adds the
// columns in order j = 0 .. F-1 with fp64 FMAs, so a row's result depends on nothing but that row.  A workgroup of 256 rows stages
// 32 columns at a time in LDS (coalesced reads; row stride 33 words, so the per-row reads that follow hit 64 different banks) next
// to the matching 32 x KT block of coefficients (zero for k >= K).  No workspace, no atomics.
#include "common.hpp"

namespace mlqem {
namespace {

constexpr int kLinregMaxF = 512, kLinregMaxK = 16;
constexpr int kMomTile = 64;        // output tile edge: 2 x 2 waves x (2 x 2) MFMA blocks of 16 x 16
constexpr int kMomSlab = 32;        // rows staged at once
constexpr int kMomTargetGroups = 1024;   // workgroups a large fit is spread over (4 per compute unit)
constexpr int kMomMinChunk = 256;   // rows per split at least: a split's 32 KB tile of partials must be worth writing

struct MomentsPlan { int tiles_1d, tiles; int64_t chunk_rows, splits; };

// a function of (n, F, K) only: the partition of the rows is part of the result's bits
inline MomentsPlan moments_plan(int64_t n, int F, int K) {
  MomentsPlan p;
  const int D = 1 + F + K;
  p.tiles_1d = (D + kMomTile - 1) / kMomTile;
  p.tiles = p.tiles_1d * (p.tiles_1d + 1) / 2;
  const int64_t max_splits = std::max<int64_t>(1, kMomTargetGroups / p.tiles);
  int64_t chunk = std::max<int64_t>(kMomMinChunk, ceil_div(std::max<int64_t>(n, 1), max_splits));
  p.chunk_rows = ceil_div(chunk, kMomSlab) * kMomSlab;
  p.splits = std::max<int64_t>(1, ceil_div(n, p.chunk_rows));
  return p;
}

// Column g of A for this lane: where it lives and whether it exists.  g == 0 is the column of ones.
struct MomColumn { const float* base; int64_t ld; bool data, one; };
__device__ __forceinline__ MomColumn mom_column(int g, const float* x, int64_t ldx, const float* y, int64_t ldy, int F, int K) {
  MomColumn c;
  const bool in_x = g <= F;                                 // g = 0 reads x's first column and discards it
  const int col = in_x ? min(max(g - 1, 0), F - 1) : min(g - 1 - F, K - 1);
  c.base = (in_x ? x : y) + col;
  c.ld = in_x ? ldx : ldy;
  c.data = g >= 1 && g < 1 + F + K;
  c.one = g == 0;
  return c;
}

constexpr int kMomStride = kMomTile + 16;   // a wave reads 4 rows x 16 columns at once: 16 words of shift keep the rows on different banks
typedef double mom_d4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(kBlock) void linreg_moments_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ y,
                                                                int64_t ldy, int64_t n_rows, int F, int K, int tiles_1d,
                                                                int64_t chunk_rows, int64_t splits, double* __restrict__ partial) {
  __shared__ __align__(16) float sa[kMomSlab][kMomStride];
  __shared__ __align__(16) float sb[kMomSlab][kMomStride];
  const int tid = threadIdx.x;
  // tile = ti (ti + 1) / 2 + tj, ti >= tj
  const int tile = blockIdx.x;
  int ti = 0;
  while ((ti + 1) * (ti + 2) / 2 <= tile) ++ti;             // at most 9 steps (tiles_1d <= 9)
  const int tj = tile - ti * (ti + 1) / 2;
  const int64_t split = blockIdx.y;
  const int64_t row_beg = split * chunk_rows;
  const int64_t row_end = min(row_beg + chunk_rows, n_rows);

  const int c = tid & (kMomTile - 1), r0 = tid >> 6;        // staging: lane = column, wave = row of a group of four
  const MomColumn ca = mom_column(ti * kMomTile + c, x, ldx, y, ldy, F, K);
  const MomColumn cb = mom_column(tj * kMomTile + c, x, ldx, y, ldy, F, K);

  // wave (wi, wj) owns the 32 x 32 quarter of the tile: 2 x 2 blocks of v_mfma_f64_16x16x4_f64.  Operand layout: lane l gives
  // A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15] -- here both are slab[k][column] -- and gets C[(l >> 4) + 4 reg][l & 15].
  const int lane = tid & (kWave - 1), wave = tid >> 6;
  const int wi = wave >> 1, wj = wave & 1, kk = lane >> 4, lc = lane & 15;
  mom_d4 acc[2][2];
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int q = 0; q < 2; ++q) acc[p][q] = (mom_d4){0.0, 0.0, 0.0, 0.0};

  // the next slab's words are fetched into registers while this one is multiplied
  float va[kMomSlab / 4], vb[kMomSlab / 4];
#pragma unroll
  for (int i = 0; i < kMomSlab / 4; ++i) {
    const int64_t row = min(row_beg + r0 + 4 * i, n_rows - 1);
    va[i] = ca.base[row * ca.ld];
    vb[i] = cb.base[row * cb.ld];                           // the diagonal tile reads the same words again: they are in L1
  }
  for (int64_t slab = row_beg; slab < row_end; slab += kMomSlab) {
#pragma unroll
    for (int i = 0; i < kMomSlab / 4; ++i) {
      const bool live = slab + r0 + 4 * i < row_end;
      sa[r0 + 4 * i][c] = live ? (ca.data ? va[i] : (ca.one ? 1.f : 0.f)) : 0.f;
      sb[r0 + 4 * i][c] = live ? (cb.data ? vb[i] : (cb.one ? 1.f : 0.f)) : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kMomSlab / 4; ++i) {                // past the chunk's end: a clamped row, never staged
      const int64_t row = min(slab + kMomSlab + r0 + 4 * i, n_rows - 1);
      va[i] = ca.base[row * ca.ld];
      vb[i] = cb.base[row * cb.ld];
    }
#pragma unroll
    for (int k0 = 0; k0 < kMomSlab; k0 += 4) {
      double a[2], b[2];
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        a[p] = (double)sa[k0 + kk][32 * wi + 16 * p + lc];
        b[p] = (double)sb[k0 + kk][32 * wj + 16 * p + lc];
      }
#pragma unroll
      for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int q = 0; q < 2; ++q) acc[p][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[p], b[q], acc[p][q], 0, 0, 0);
    }
    __syncthreads();
  }
  double* dst = partial + ((int64_t)tile * splits + split) * (kMomTile * kMomTile);
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg)
        dst[(32 * wi + 16 * p + kk + 4 * reg) * kMomTile + 32 * wj + 16 * q + lc] = acc[p][q][reg];
}

// The splits of every entry of the lower-triangle tiles, added in a fixed order: 16 threads share an entry, thread g adds the g-th
// run of ceil(splits / 16) splits in split order, thread 0 then adds the 16 runs in run order (onto the old value when `accumulate`)
// and writes both triangles.  A thread past its run reads a clamped split and adds 0.0, which changes nothing.
constexpr int kRedRuns = 16, kRedEntries = kBlock / kRedRuns;
__global__ __launch_bounds__(kBlock) void linreg_moments_reduce_kernel(const double* __restrict__ partial, int64_t splits, int D,
                                                                       int accumulate, double* __restrict__ moments) {
  __shared__ double runs[kRedRuns][kRedEntries];
  const int tile = blockIdx.x;
  int ti = 0;
  while ((ti + 1) * (ti + 2) / 2 <= tile) ++ti;
  const int tj = tile - ti * (ti + 1) / 2;
  const int el = threadIdx.x & (kRedEntries - 1), run = threadIdx.x / kRedEntries;
  const int e = blockIdx.y * kRedEntries + el;              // entry of the 64 x 64 tile
  const double* src = partial + (int64_t)tile * splits * (kMomTile * kMomTile) + e;
  const int i = ti * kMomTile + (e >> 6), j = tj * kMomTile + (e & 63);
  const bool mine = run == 0 && i < D && j <= i;            // the others read a clamped entry and drop it
  const double old = accumulate ? moments[(int64_t)min(i, D - 1) * D + min(j, D - 1)] : 0.0;
  const int64_t per = ceil_div(splits, (int64_t)kRedRuns), s_beg = run * per;
  double sum = 0.0;
  for (int64_t t = 0; t < per; t += 4) {                    // four loads in flight, added in split order
    double v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = src[min(s_beg + t + u, splits - 1) * (kMomTile * kMomTile)];
#pragma unroll
    for (int u = 0; u < 4; ++u) sum += (t + u < per && s_beg + t + u < splits) ? v[u] : 0.0;
  }
  runs[run][el] = sum;
  __syncthreads();
  if (mine) {
    double total = old;
#pragma unroll
    for (int g = 0; g < kRedRuns; ++g) total += runs[g][el];
    moments[(int64_t)i * D + j] = total;
    moments[(int64_t)j * D + i] = total;
  }
}

constexpr int kPredCols = 32;       // columns staged at once
constexpr int kPredStride = kPredCols + 1;

template <int KT>
__global__ __launch_bounds__(kBlock) void linreg_predict_kernel(const float* __restrict__ x, int64_t ldx, int64_t n_rows, int F,
                                                                const double* __restrict__ coef, const double* __restrict__ intercept,
                                                                int K, double* __restrict__ out) {
  __shared__ float xs[kBlock * kPredStride];
  __shared__ double cs[kPredCols * KT];
  const int tid = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * kBlock;
  double acc[KT];
#pragma unroll
  for (int k = 0; k < KT; ++k) acc[k] = intercept[min(k, K - 1)];

  for (int j0 = 0; j0 < F; j0 += kPredCols) {
    const int cols = min(kPredCols, F - j0);
    {
      const int c = tid & (kPredCols - 1), r = tid >> 5;      // 32 lanes along a row: 128-byte reads
      const int col = min(j0 + c, F - 1);
      float v[kPredCols];
#pragma unroll
      for (int i = 0; i < kPredCols; ++i) v[i] = x[min(row0 + r + 8 * i, n_rows - 1) * ldx + col];
#pragma unroll
      for (int i = 0; i < kPredCols; ++i) xs[(r + 8 * i) * kPredStride + c] = v[i];
    }
    for (int e = tid; e < kPredCols * KT; e += kBlock) {
      const int j = e / KT, k = e - j * KT;
      const double w = coef[(int64_t)min(k, K - 1) * F + min(j0 + j, F - 1)];
      cs[e] = (k < K && j < cols) ? w : 0.0;
    }
    __syncthreads();
    for (int j = 0; j < cols; ++j) {
      const double xv = (double)xs[tid * kPredStride + j];
#pragma unroll
      for (int k = 0; k < KT; ++k) acc[k] = fma(cs[j * KT + k], xv, acc[k]);
    }
    __syncthreads();
  }
  if (row0 + tid < n_rows) {
#pragma unroll
    for (int k = 0; k < KT; ++k)
      if (k < K) out[(row0 + tid) * K + k] = acc[k];
  }
}

template <int KT>
void launch_predict(int64_t blocks, hipStream_t s, const float* x, int64_t ldx, int64_t n_rows, int F, const double* coef,
                    const double* intercept, int K, double* out) {
  hipLaunchKernelGGL(linreg_predict_kernel<KT>, dim3((unsigned)blocks), dim3(kBlock), 0, s, x, ldx, n_rows, F, coef, intercept, K, out);
}

}  // namespace
}  // namespace mlqem

using namespace mlqem;

extern "C" size_t mlqem_linreg_moments_workspace_bytes(int64_t n_rows, int F, int K) {
  if (n_rows < 0 || F < 1 || K < 1 || F > kLinregMaxF || K > kLinregMaxK) return 0;
  const MomentsPlan p = moments_plan(n_rows, F, K);
  return (size_t)p.tiles * (size_t)p.splits * kMomTile * kMomTile * sizeof(double);
}

extern "C" int mlqem_linreg_moments_f32(const float* x, int64_t ldx, const float* y, int64_t ldy, int64_t n_rows, int F, int K,
                                        double* moments, int accumulate, void* workspace, size_t workspace_bytes,
                                        mlqem_stream_t stream) {
  begin_launches();
  if (n_rows < 0 || F < 1 || K < 1 || ldx < F || ldy < K) return MLQEM_ERR_BAD_ARG;
  if (F > kLinregMaxF || K > kLinregMaxK) return MLQEM_ERR_UNSUPPORTED;
  const int D = 1 + F + K;
  if (n_rows == 0) {
    if (accumulate) return MLQEM_OK;
    if (!moments) return MLQEM_ERR_BAD_ARG;
    if (hipMemsetAsync(moments, 0, (size_t)D * D * sizeof(double), as_stream(stream)) != hipSuccess) return MLQEM_ERR_LAUNCH;
    return launch_status();
  }
  if (workspace_bytes < mlqem_linreg_moments_workspace_bytes(n_rows, F, K)) return MLQEM_ERR_WORKSPACE;
  if (!x || !y || !moments || !workspace || !aligned_to(workspace, 16) || !aligned_to(moments, 8)) return MLQEM_ERR_BAD_ARG;
  const MomentsPlan p = moments_plan(n_rows, F, K);
  if (p.splits > 65535) return MLQEM_ERR_UNSUPPORTED;        // unreachable below 2^31 rows a tile: splits <= 1024
  double* partial = static_cast<double*>(workspace);
  hipLaunchKernelGGL(linreg_moments_kernel, dim3((unsigned)p.tiles, (unsigned)p.splits), dim3(kBlock), 0, as_stream(stream), x, ldx, y,
                     ldy, n_rows, F, K, p.tiles_1d, p.chunk_rows, p.splits, partial);
  hipLaunchKernelGGL(linreg_moments_reduce_kernel, dim3((unsigned)p.tiles, kMomTile * kMomTile / kRedEntries), dim3(kBlock), 0,
                     as_stream(stream), partial, p.splits, D, accumulate, moments);
  return launch_status();
}

extern "C" int mlqem_linreg_predict_f32(const float* x, int64_t ldx, int64_t n_rows, int F, const double* coef, const double* intercept,
                                        int K, double* out, mlqem_stream_t stream) {
  begin_launches();
  if (n_rows < 0 || F < 1 || K < 1 || ldx < F) return MLQEM_ERR_BAD_ARG;
  if (F > kLinregMaxF || K > kLinregMaxK) return MLQEM_ERR_UNSUPPORTED;
  if (n_rows == 0) return MLQEM_OK;
  if (!x || !coef || !intercept || !out) return MLQEM_ERR_BAD_ARG;
  const int64_t blocks = ceil_div(n_rows, (int64_t)kBlock);
  if (blocks > 0x7FFFFFFFll) return MLQEM_ERR_UNSUPPORTED;
  hipStream_t s = as_stream(stream);
  if (K == 1) launch_predict<1>(blocks, s, x, ldx, n_rows, F, coef, intercept, K, out);
  else if (K == 2) launch_predict<2>(blocks, s, x, ldx, n_rows, F, coef, intercept, K, out);
  else if (K <= 4) launch_predict<4>(blocks, s, x, ldx, n_rows, F, coef, intercept, K, out);
  else if (K <= 8) launch_predict<8>(blocks, s, x, ldx, n_rows, F, coef, intercept, K, out);
  else launch_predict<16>(blocks, s, x, ldx, n_rows, F, coef, intercept, K, out);
  return launch_status();
}
