// Batched regression-forest inference (mlqem_forest_predict_f32): out[r, :] = (1 / T) sum_t values[leaf_t(x_r), :].
//
// Node layout (include/mlqem_hip.h has the contract): 16-byte records {thr32, feature, right, orig}, every tree in depth-first
// pre-order, so the left child of node i is node i + 1 and one 16-byte load per level brings all a step needs.  thr32 is the model's
// float64 threshold rounded toward minus infinity, which makes the fp32 `x <= thr32` take the branch of the float64 compare for
// every float32 x.  A leaf has feature = -1 and right = itself.  NaN features compare false and go right.
//
// Shape of the kernel.  A workgroup of 256 threads owns a tile of R consecutive rows (R = 64, 16 or 4: the launcher takes the
// largest that still gives every compute unit work) and stages their feature rows in LDS once (row stride F | 1 words: lanes of a wave
// hold different rows, an odd stride spreads them over the banks).  Thread (row = tid % R, slot = tid / R) then walks trees
// slot, slot + S, slot + 2 S, slot + 3 S (S = 256 / R) of a chunk of 4 S trees AT ONCE: four independent chains of
// (node load -> x[feature] LDS read -> select) per lane, because a single chain leaves the lane idle for a load round trip per level.
// With R = 64 a wave walks ONE tree for 64 rows: near the root all lanes read the same record.  Node records are read from global
// memory (a 100-300 tree forest of the demos is 0.3-2 MB: resident in an XCD's 4 MB L2).
// Every step is predicated selects under a wave-uniform trip count: the loop runs until no lane of the wave is at an inner node, and
// never more than max_depth times.  Every index taken from a record is clamped (child to the tree, feature to F), so no node table
// makes the kernel spin or read out of range.
// The leaves of the chunk go to LDS ([tree of chunk][row], 4 KB); after a barrier thread (row, k) adds their values in TREE ORDER into
// a float64 register that lives across chunks.  The sum is therefore the same for every R and every n_rows, bit for bit, and there is
// no floating-point atomic and no workspace.
//
// The out-of-bag entry (mlqem_forest_predict_oob_f32) is the same kernel with OOB = true: out[r, :] is the mean over the trees t with
// counts[t, r] == 0 only.  A (row, tree) pair that is in the bag is "at a leaf" from step 0, so it never holds the wave's trip count
// open, and its slot of the LDS leaf array holds -1; the accumulating thread reads `values` at a clamped index, selects 0.0 for such a
// slot and counts its row's out-of-bag trees in an integer register, which divides the sum once.  The counts load is unconditional
// on a clamped (tree, row) and masked by a select; with R = 64 a wave reads 64 consecutive counts of one tree.
#include "common.hpp"

namespace mlqem {
namespace {

constexpr int kForestWalks = 4;                      // trees a thread walks at once (a power of two)
constexpr int kForestChunkItems = kBlock * kForestWalks;   // (tree, row) leaves of one chunk: 1024 int32 = 4 KB of LDS
constexpr int kForestXBytes = 48 * 1024;             // LDS budget of the staged rows: with the leaves, under the 64 KB a launch gets
constexpr int kForestMaxAcc = 4;                     // (row, k) sums per thread: R K / 256 <= 64 * 16 / 256

typedef int forest_i4 __attribute__((ext_vector_type(4)));

template <bool XLDS, bool OOB>
__global__ __launch_bounds__(kBlock) void forest_predict_kernel(const float* __restrict__ x, int64_t ldx, int64_t n_rows, int F,
                                                                const forest_i4* __restrict__ nodes,
                                                                const int64_t* __restrict__ tree_ptr, int T,
                                                                const double* __restrict__ values, int K, int max_depth, int log_r,
                                                                double* __restrict__ out, int32_t* __restrict__ leaf_out,
                                                                const int32_t* __restrict__ counts, int64_t ldc,
                                                                int32_t* __restrict__ n_oob) {
  extern __shared__ int forest_smem[];
  int* leaves = forest_smem;                                             // [4 S][R]
  float* xs = reinterpret_cast<float*>(forest_smem + kForestChunkItems);   // [R][F | 1] when XLDS
  const int tid = threadIdx.x;
  const int R = 1 << log_r, S = kBlock >> log_r, TC = S * kForestWalks;
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

  // the (row, k) sums this thread owns: item e = tid + 256 m of the R K items, k fastest
  int acc_row[kForestMaxAcc], acc_k[kForestMaxAcc];
  double acc[kForestMaxAcc];
  int acc_n[kForestMaxAcc];   // OOB: the out-of-bag trees of the row so far
#pragma unroll
  for (int m = 0; m < kForestMaxAcc; ++m) {
    const int e = tid + kBlock * m;
    acc_row[m] = e / K;
    acc_k[m] = e - acc_row[m] * K;
    acc[m] = 0.0;
    acc_n[m] = 0;
  }
  const int64_t crow = OOB ? min(row0 + row, n_rows - 1) : 0;   // the row whose counts this thread reads, clamped

  for (int t0 = 0; t0 < T; t0 += TC) {
    int64_t base[kForestWalks];
    int last[kForestWalks], at[kForestWalks];
    bool in_bag[kForestWalks];
#pragma unroll
    for (int j = 0; j < kForestWalks; ++j) {
      const int t = min(t0 + slot + S * j, T - 1);   // a slot past the last tree walks the last tree again: loads stay unconditional
      base[j] = tree_ptr[t];
      last[j] = max((int)(tree_ptr[t + 1] - base[j]) - 1, 0);
      at[j] = 0;
      if (OOB) {   // any non-zero count is in the bag; so is a lane past the last row or the last tree (nothing of it is used)
        const int32_t cnt = counts[(int64_t)t * ldc + crow];
        in_bag[j] = (cnt != 0) | (t0 + slot + S * j >= T) | (row0 + row >= n_rows);
      } else {
        in_bag[j] = false;
      }
    }
    for (int d = 0; d < max_depth; ++d) {
      forest_i4 nd[kForestWalks];
#pragma unroll
      for (int j = 0; j < kForestWalks; ++j) nd[j] = nodes[base[j] + at[j]];
      bool inner = false;
#pragma unroll
      for (int j = 0; j < kForestWalks; ++j) {
        const bool is_leaf = OOB ? (nd[j].y < 0) | in_bag[j] : nd[j].y < 0;
        const int f = min(max(nd[j].y, 0), F - 1);
        const float xv = xrow[f];
        const int child = xv <= __builtin_bit_cast(float, nd[j].x) ? at[j] + 1 : nd[j].z;
        at[j] = is_leaf ? at[j] : (int)min((unsigned)child, (unsigned)last[j]);
        inner |= !is_leaf;
      }
      if (!__any(inner)) break;
    }
#pragma unroll
    for (int j = 0; j < kForestWalks; ++j) {
      const int orig = nodes[base[j] + at[j]].w;
      const int lf = (int)min((unsigned)orig, (unsigned)last[j]);
      leaves[(slot + S * j) * R + row] = OOB && in_bag[j] ? -1 : lf;
    }
    __syncthreads();

    const int tc = min(TC, T - t0);
#pragma unroll
    for (int m = 0; m < kForestMaxAcc; ++m) {
      if (tid + kBlock * m < R * K) {
        const int r = acc_row[m], k = acc_k[m];
        int c = 0;
        for (; c + 4 <= tc; c += 4) {   // four gathers in flight, added in tree order
          double v[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int lf = leaves[(c + u) * R + r];
            v[u] = values[(tree_ptr[t0 + c + u] + (OOB ? max(lf, 0) : lf)) * K + k];
            if (OOB) {
              v[u] = lf < 0 ? 0.0 : v[u];
              acc_n[m] += lf >= 0;
            }
          }
          acc[m] += v[0]; acc[m] += v[1]; acc[m] += v[2]; acc[m] += v[3];
        }
        for (; c < tc; ++c) {
          const int lf = leaves[c * R + r];
          const double v = values[(tree_ptr[t0 + c] + (OOB ? max(lf, 0) : lf)) * K + k];
          acc[m] += OOB && lf < 0 ? 0.0 : v;
          if (OOB) acc_n[m] += lf >= 0;
        }
      }
    }
    if (leaf_out) {
      const int log_tc = 31 - __builtin_clz(TC);   // TC = kForestChunkItems / R, a power of two
      for (int e = tid; e < kForestChunkItems; e += kBlock) {
        const int c = e & (TC - 1), r = e >> log_tc;
        if (c < tc && row0 + r < n_rows) leaf_out[(row0 + r) * T + t0 + c] = leaves[c * R + r];
      }
    }
    __syncthreads();
  }

#pragma unroll
  for (int m = 0; m < kForestMaxAcc; ++m) {
    if (tid + kBlock * m < R * K && row0 + acc_row[m] < n_rows) {
      if (OOB) {   // a row no tree left out gets 0.0 (scikit-learn's oob_prediction_ does the same)
        out[(row0 + acc_row[m]) * K + acc_k[m]] = acc_n[m] > 0 ? acc[m] / (double)max(acc_n[m], 1) : 0.0;
        if (acc_k[m] == 0) n_oob[row0 + acc_row[m]] = acc_n[m];
      } else {
        out[(row0 + acc_row[m]) * K + acc_k[m]] = acc[m] / (double)T;
      }
    }
  }
}

}  // namespace
}  // namespace mlqem

using namespace mlqem;

namespace {

// Both entries: the checks, the tile and the launch.  `oob` selects the instantiation that reads counts and writes n_oob.
int forest_predict_launch(const float* x, int64_t ldx, int64_t n_rows, int F, const mlqem_forest_node* nodes, const int64_t* tree_ptr,
                          int T, const double* values, int K, int max_depth, bool oob, const int32_t* counts, int64_t ldc, double* out,
                          int32_t* n_oob, int32_t* leaf, mlqem_stream_t stream) {
  static_assert(sizeof(mlqem_forest_node) == 16, "one 16-byte load per node");
  begin_launches();
  if (n_rows < 0 || F < 1 || T < 1 || K < 1 || max_depth < 0 || ldx < F || (oob && ldc < n_rows)) return MLQEM_ERR_BAD_ARG;
  if (K > 16 || F > 32767) return MLQEM_ERR_UNSUPPORTED;
  if (n_rows == 0) return MLQEM_OK;
  if (!x || !nodes || !tree_ptr || !values || !out || !aligned_to(nodes, 16) || (oob && (!counts || !n_oob))) return MLQEM_ERR_BAD_ARG;
  // rows per workgroup: 64 once that still makes >= 512 workgroups (two per compute unit), fewer rows and more tree slots below
  int log_r = n_rows >= 32768 ? 6 : n_rows >= 8192 ? 4 : 2;
  const size_t row_bytes = (size_t)(F | 1) * sizeof(float);
  while (log_r > 2 && (row_bytes << log_r) > (size_t)kForestXBytes) log_r -= 2;
  const bool x_lds = (row_bytes << log_r) <= (size_t)kForestXBytes;
  const int64_t blocks = ceil_div(n_rows, (int64_t)1 << log_r);
  if (blocks > 0x7FFFFFFFll) return MLQEM_ERR_UNSUPPORTED;
  const size_t lds = kForestChunkItems * sizeof(int) + (x_lds ? (row_bytes << log_r) : 0);
  const forest_i4* nd = reinterpret_cast<const forest_i4*>(nodes);
  auto kernel = oob ? (x_lds ? forest_predict_kernel<true, true> : forest_predict_kernel<false, true>)
                    : (x_lds ? forest_predict_kernel<true, false> : forest_predict_kernel<false, false>);
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kBlock), lds, as_stream(stream), x, ldx, n_rows, F, nd, tree_ptr, T, values, K,
                     max_depth, log_r, out, leaf, counts, ldc, n_oob);
  return launch_status();
}

}  // namespace

extern "C" int mlqem_forest_predict_f32(const float* x, int64_t ldx, int64_t n_rows, int F, const mlqem_forest_node* nodes,
                                        const int64_t* tree_ptr, int T, const double* values, int K, int max_depth, double* out,
                                        int32_t* leaf, mlqem_stream_t stream) {
  return forest_predict_launch(x, ldx, n_rows, F, nodes, tree_ptr, T, values, K, max_depth, false, nullptr, 0, out, nullptr, leaf, stream);
}

extern "C" int mlqem_forest_predict_oob_f32(const float* x, int64_t ldx, int64_t n_rows, int F, const mlqem_forest_node* nodes,
                                            const int64_t* tree_ptr, int T, const double* values, int K, int max_depth,
                                            const int32_t* counts, int64_t ldc, double* out, int32_t* n_oob, int32_t* leaf,
                                            mlqem_stream_t stream) {
  return forest_predict_launch(x, ldx, n_rows, F, nodes, tree_ptr, T, values, K, max_depth, true, counts, ldc, out, n_oob, leaf, stream);
}
