// Gradient-boosted regression trees (squared error): scoring a fitted ensemble (mlqem_boost_predict_f32) and the step between two
// stages of a fit (mlqem_boost_update_f64).  include/mlqem_hip.h has the contracts.
//
// Scoring.  The ensemble is stored as a forest is (16-byte node records in pre-order, tree_ptr, float64 values [N, 1]) and the walk is
// the forest kernel's: a workgroup of 256 threads owns a tile of R consecutive rows (64, 16 or 4), stages their feature rows in LDS
// (row stride F | 1 words), and thread (row = tid % R, slot = tid / R) walks four trees of a chunk of 4 * 256 / R stages at once --
// unconditional 16-byte loads on clamped indices, predicated selects, a wave-uniform trip count of at most max_depth.  The leaves of the
// chunk go to LDS; after a barrier thread `row` (tid < R) alone adds them IN STAGE ORDER into the float64 register that holds its row's
// running sum, one rounded multiply and one rounded add per stage:  acc = acc + lr * value  (scikit-learn's predict_stages).  So the sum
// does not depend on R, on n_rows or on the call, bit for bit; no atomics, no workspace.  With `staged` the thread stores its running
// sum after every stage at staged[stage * lds + row]: the R threads of a tile write R consecutive doubles of one output row.
//
// Update.  One thread per training row walks the stage's tree in the fit workspace's own numbering (node_i = feature, left, right,
// rows; float64 thresholds compared with the widened float32 x, as scikit-learn compares) for at most max_depth + 1 steps, every index
// clamped to the node count; a tree of at most 511 nodes is staged in LDS first.  Then raw += lr * value[leaf] (a multiply, then an
// add) and resid = y - raw.  The same launch reduces four float64 sums over its 256 rows in a fixed order (a shuffle tree within a
// wave, then wave 0 .. 3 through LDS) and writes them as one record of `partial`: nothing is added across workgroups here.
#include "common.hpp"

#pragma clang fp contract(off)   // the contracts are stated operation by operation: no fused multiply-add

namespace mlqem {
namespace {

constexpr int kBoostWalks = 4;                            // trees a thread walks at once
constexpr int kBoostChunkItems = kBlock * kBoostWalks;    // (stage, row) leaves of one chunk: 4 KB of LDS
constexpr int kBoostXBytes = 48 * 1024;                   // LDS budget of the staged rows
constexpr int kBoostLdsNodes = 511;                       // the largest tree the update kernel stages in LDS (depth 8)

typedef int boost_i4 __attribute__((ext_vector_type(4)));

template <bool XLDS>
__global__ __launch_bounds__(kBlock) void boost_predict_kernel(const float* __restrict__ x, int64_t ldx, int64_t n_rows, int F,
                                                               const boost_i4* __restrict__ nodes,
                                                               const int64_t* __restrict__ tree_ptr, int T,
                                                               const double* __restrict__ values, int max_depth, int log_r,
                                                               double init, double lr, double* __restrict__ out,
                                                               double* __restrict__ staged, int64_t lds) {
  extern __shared__ int boost_smem[];
  int* leaves = boost_smem;                                              // [4 S][R]
  float* xs = reinterpret_cast<float*>(boost_smem + kBoostChunkItems);   // [R][F | 1] when XLDS
  const int tid = threadIdx.x;
  const int R = 1 << log_r, S = kBlock >> log_r, TC = S * kBoostWalks;
  const int row = tid & (R - 1), slot = tid >> log_r;
  const int64_t row0 = (int64_t)blockIdx.x * R;
  const int stride = F | 1;

  if (XLDS) {
    for (int r = tid >> 6; r < R; r += kBlock / kWave) {
      const bool live = row0 + r < n_rows;
      const float* src = x + (live ? row0 + r : 0) * ldx;
      for (int f = tid & (kWave - 1); f < F; f += kWave) xs[r * stride + f] = live ? src[f] : 0.f;
    }
    __syncthreads();
  }
  // rows past the end walk row n_rows - 1 (or the zeros staged above); nothing of theirs is stored
  const float* xrow = XLDS ? xs + row * stride : x + min(row0 + row, n_rows - 1) * ldx;
  const bool owner = tid < R;                     // the thread that owns row `tid` of the tile (row == tid then)
  const bool stored = owner && row0 + tid < n_rows;
  double acc = init;

  for (int t0 = 0; t0 < T; t0 += TC) {
    int64_t base[kBoostWalks];
    int last[kBoostWalks], at[kBoostWalks];
#pragma unroll
    for (int j = 0; j < kBoostWalks; ++j) {
      const int t = min(t0 + slot + S * j, T - 1);   // a slot past the last stage walks the last tree again: loads stay unconditional
      base[j] = tree_ptr[t];
      last[j] = max((int)(tree_ptr[t + 1] - base[j]) - 1, 0);
      at[j] = 0;
    }
    for (int d = 0; d < max_depth; ++d) {
      boost_i4 nd[kBoostWalks];
#pragma unroll
      for (int j = 0; j < kBoostWalks; ++j) nd[j] = nodes[base[j] + at[j]];
      bool inner = false;
#pragma unroll
      for (int j = 0; j < kBoostWalks; ++j) {
        const bool is_leaf = nd[j].y < 0;
        const int f = min(max(nd[j].y, 0), F - 1);
        const float xv = xrow[f];
        const int child = xv <= __builtin_bit_cast(float, nd[j].x) ? at[j] + 1 : nd[j].z;
        at[j] = is_leaf ? at[j] : (int)min((unsigned)child, (unsigned)last[j]);
        inner |= !is_leaf;
      }
      if (!__any(inner)) break;
    }
#pragma unroll
    for (int j = 0; j < kBoostWalks; ++j) {
      const int orig = nodes[base[j] + at[j]].w;
      leaves[(slot + S * j) * R + row] = (int)min((unsigned)orig, (unsigned)last[j]);
    }
    __syncthreads();

    const int tc = min(TC, T - t0);
    if (owner) {
      int c = 0;
      for (; c + 4 <= tc; c += 4) {   // four gathers in flight, added in stage order
        double v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = values[tree_ptr[t0 + c + u] + leaves[(c + u) * R + tid]];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const double step = lr * v[u];
          acc = acc + step;
          if (staged && stored) staged[(int64_t)(t0 + c + u) * lds + row0 + tid] = acc;
        }
      }
      for (; c < tc; ++c) {
        const double step = lr * values[tree_ptr[t0 + c] + leaves[c * R + tid]];
        acc = acc + step;
        if (staged && stored) staged[(int64_t)(t0 + c) * lds + row0 + tid] = acc;
      }
    }
    __syncthreads();
  }
  if (stored) out[row0 + tid] = acc;
}

// Sum over the 64 lanes of a wave, the same tree of additions for every wave and call.
__device__ __forceinline__ double boost_wave_sum(double v) {
#pragma unroll
  for (int d = kWave / 2; d >= 1; d >>= 1) v = v + __shfl_down(v, d, kWave);
  return v;
}

template <bool TLDS>
__global__ __launch_bounds__(kBlock) void boost_update_kernel(const float* __restrict__ x, int64_t ldx, int64_t n_rows, int F,
                                                              const boost_i4* __restrict__ node_i, const double* __restrict__ node_thr,
                                                              const double* __restrict__ node_value, int n_nodes, int max_depth,
                                                              double lr, const double* __restrict__ y, double* __restrict__ raw,
                                                              double* __restrict__ resid, const int32_t* __restrict__ mask,
                                                              double* __restrict__ partial) {
  __shared__ boost_i4 sh_i[TLDS ? kBoostLdsNodes : 1];
  __shared__ double sh_thr[TLDS ? kBoostLdsNodes : 1], sh_val[TLDS ? kBoostLdsNodes : 1];
  __shared__ double sh_sum[kBlock / kWave][4];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid >> 6;
  const int last = (TLDS ? min(n_nodes, kBoostLdsNodes) : n_nodes) - 1;   // n_nodes >= 1 (checked by the launcher)
  if (TLDS) {
    for (int i = tid; i <= last; i += kBlock) {
      sh_i[i] = node_i[i];
      sh_thr[i] = node_thr[i];
      sh_val[i] = node_value[i];
    }
    __syncthreads();
  }
  const boost_i4* ni = TLDS ? sh_i : node_i;
  const double* nthr = TLDS ? sh_thr : node_thr;
  const double* nval = TLDS ? sh_val : node_value;

  const int64_t r = (int64_t)blockIdx.x * kBlock + tid;
  const bool live = r < n_rows;
  const int64_t rc = min(r, n_rows - 1);          // a thread past the end walks the last row; nothing of it is stored or summed
  const float* xrow = x + rc * ldx;
  int at = 0;
  for (int step = 0; step <= max_depth; ++step) {
    const boost_i4 nd = ni[at];                   // feature (or -2), left, right, rows
    const bool is_leaf = nd.y < 0 || nd.z < 0;
    const int f = min(max(nd.x, 0), F - 1);
    const bool go_left = (double)xrow[f] <= nthr[at];
    const int child = go_left ? nd.y : nd.z;
    at = is_leaf ? at : min(max(child, 0), last);
    if (!__any(!is_leaf)) break;
  }
  const double yv = y[rc], before = raw[rc];
  const double step = lr * nval[at];
  const double after = before + step;
  const double res_before = yv - before, res_after = yv - after;
  const bool in_bag = mask ? mask[rc] != 0 : true;
  if (live) {
    raw[r] = after;
    resid[r] = res_after;
  }
  double sums[4];
  sums[0] = live && in_bag ? res_after * res_after : 0.0;      // in-bag squared residual after the update
  sums[1] = live && !in_bag ? res_before * res_before : 0.0;   // out-of-bag, before
  sums[2] = live && !in_bag ? res_after * res_after : 0.0;     // out-of-bag, after
  sums[3] = live && in_bag ? 1.0 : 0.0;                        // in-bag rows
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const double s = boost_wave_sum(sums[j]);
    if (lane == 0) sh_sum[wv][j] = s;
  }
  __syncthreads();
  if (tid < 4) {
    double s = sh_sum[0][tid];
#pragma unroll
    for (int w = 1; w < kBlock / kWave; ++w) s = s + sh_sum[w][tid];
    partial[(int64_t)blockIdx.x * 4 + tid] = s;
  }
}

}  // namespace
}  // namespace mlqem

using namespace mlqem;

extern "C" int mlqem_boost_predict_f32(const float* x, int64_t ldx, int64_t n_rows, int F, const mlqem_forest_node* nodes,
                                       const int64_t* tree_ptr, int n_stages, const double* values, int max_depth, double init,
                                       double lr, double* out, double* staged, int64_t lds, mlqem_stream_t stream) {
  static_assert(sizeof(mlqem_forest_node) == 16, "one 16-byte load per node");
  begin_launches();
  if (n_rows < 0 || F < 1 || n_stages < 1 || max_depth < 0 || ldx < F || (staged && lds < n_rows)) return MLQEM_ERR_BAD_ARG;
  if (F > 32767) return MLQEM_ERR_UNSUPPORTED;
  if (n_rows == 0) return MLQEM_OK;
  if (!x || !nodes || !tree_ptr || !values || !out || !aligned_to(nodes, 16)) return MLQEM_ERR_BAD_ARG;
  // the forest kernel's tiles: 64 rows once that still makes >= 512 workgroups, fewer rows and more tree slots below
  int log_r = n_rows >= 32768 ? 6 : n_rows >= 8192 ? 4 : 2;
  const size_t row_bytes = (size_t)(F | 1) * sizeof(float);
  while (log_r > 2 && (row_bytes << log_r) > (size_t)kBoostXBytes) log_r -= 2;
  const bool x_lds = (row_bytes << log_r) <= (size_t)kBoostXBytes;
  const int64_t blocks = ceil_div(n_rows, (int64_t)1 << log_r);
  if (blocks > 0x7FFFFFFFll) return MLQEM_ERR_UNSUPPORTED;
  const size_t smem = kBoostChunkItems * sizeof(int) + (x_lds ? (row_bytes << log_r) : 0);
  const boost_i4* nd = reinterpret_cast<const boost_i4*>(nodes);
  auto kernel = x_lds ? boost_predict_kernel<true> : boost_predict_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kBlock), smem, as_stream(stream), x, ldx, n_rows, F, nd, tree_ptr, n_stages,
                     values, max_depth, log_r, init, lr, out, staged, lds);
  return launch_status();
}

extern "C" int64_t mlqem_boost_update_blocks(int64_t n_rows) { return n_rows < 1 ? 0 : ceil_div(n_rows, (int64_t)kBlock); }

extern "C" int mlqem_boost_update_f64(const float* x, int64_t ldx, int64_t n_rows, int F, const int32_t* node_i, const double* node_thr,
                                      const double* node_value, int n_nodes, int max_depth, double lr, const double* y, double* raw,
                                      double* resid, const int32_t* mask, double* partial, mlqem_stream_t stream) {
  begin_launches();
  if (n_rows < 1 || F < 1 || n_nodes < 1 || max_depth < 0 || ldx < F) return MLQEM_ERR_BAD_ARG;
  if (F > 32767 || n_rows > (1 << 22)) return MLQEM_ERR_UNSUPPORTED;
  if (!x || !node_i || !node_thr || !node_value || !y || !raw || !resid || !partial || !aligned_to(node_i, 16)) return MLQEM_ERR_BAD_ARG;
  const int64_t blocks = ceil_div(n_rows, (int64_t)kBlock);
  const boost_i4* ni = reinterpret_cast<const boost_i4*>(node_i);
  auto kernel = n_nodes <= kBoostLdsNodes ? boost_update_kernel<true> : boost_update_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kBlock), 0, as_stream(stream), x, ldx, n_rows, F, ni, node_thr, node_value,
                     n_nodes, max_depth, lr, y, raw, resid, mask, partial);
  return launch_status();
}
