// Growing regression forests on the device (mlqem_forest_fit_*): exact CART with squared error, scikit-learn's best splitter
// restated, level by level for a chunk of Tc trees and all F features at once.  include/mlqem_hip.h has the contract and the rule.
//
// State (mlqem_forest_fit_state, all buffers the caller's).  The column order of x is the same for every tree (a bag changes the
// weights only), so ONE stable argsort per column (`order`) serves the whole fit.  Per (tree, feature) there is a ROW LIST: the
// in-bag rows of the live nodes, sorted by that feature within every node.  The live nodes of a level are SEGMENTS of the list: they
// are contiguous, hold the same rows in every feature's list and come in the same order, so one per-position segment id [Tc, n] and
// one segment table [Tc, n] serve all F lists.  A level is four launches:
//   stats      (a workgroup per tree)           W, sum w y^2 and S[K] of every segment, summed in the list order of the feature the
//                                               segment's parent split on (feature 0 for the root)
//   search     (a workgroup per tree, feature)  walks the list in tiles of 256 positions with segmented inclusive scans of w and
//                                               w y_k in fp64 (running sums carried from tile to tile), scores the candidate after
//                                               every position and reduces (score, position) per segment with a segmented max-scan
//   select     (a workgroup per tree)           a thread per segment: leaf tests, argmax over the features in feature order, the
//                                               threshold, the node record; children and their places in the next lists are numbered
//                                               by exclusive scans in segment order.  With max_features < F the argmax runs over
//                                               the node's own feature subset instead (select_subset: the same body, a keyed
//                                               permutation of the features per node, walked until m features and a candidate are seen)
//   partition  (a workgroup per tree, feature)  stable partition of every split segment into its children (ranks by a segmented
//                                               scan of the go-left flags); the rows of segments that became leaves are dropped
// Row lists, segment ids and segment tables are double buffered (level & 1 reads, the other half is written).
//
// Every sum is a scan whose association depends on the tile size and the positions alone: no atomics, the same bits from call to
// call and for every chunking (a tree never reads another tree's state).  Every loop's trip count comes from a launch argument (n,
// F, K; the cycle walk of a feature permutation: 4^h <= 4 F) or from a level counter clamped to n; every index read from a
// workspace buffer (row, segment, feature, node, position, destination) is clamped before it addresses memory, so a corrupted
// workspace gives a wrong forest -- which the host validation of the finished node table then sees -- never an out-of-range
// access.  Loads are unconditional on clamped indices and masked by selects afterwards.  No workgroup waits for another.
#include <math.h>

#include "common.hpp"

#pragma clang fp contract(off)   // sums and scores are the written operations: no fused multiply-add moves a near-tie

namespace mlqem {
namespace {

constexpr double kFitEps = 2.220446049250313e-16;   // a node at or below this impurity is a leaf
constexpr float kFitFeatureGap = 1e-7f;             // two feature values closer than this do not separate
constexpr int kFitMaxK = 16;

typedef int fit_i4 __attribute__((ext_vector_type(4)));

struct FitBest { double score; int pos; };

struct FitAddD {
  using T = double;
  __device__ static T id() { return 0.0; }
  __device__ static T op(T earlier, T later) { return earlier + later; }
  __device__ static T up(T v, int d) { return __shfl_up(v, d, kWave); }
};
struct FitAddI {
  using T = int;
  __device__ static T id() { return 0; }
  __device__ static T op(T earlier, T later) { return earlier + later; }
  __device__ static T up(T v, int d) { return __shfl_up(v, d, kWave); }
};
struct FitMaxB {   // the better candidate; on equal scores the earlier (lower position) one
  using T = FitBest;
  __device__ static T id() { return FitBest{-INFINITY, -1}; }
  __device__ static T op(T earlier, T later) { return later.score > earlier.score ? later : earlier; }
  __device__ static T up(T v, int d) { return FitBest{__shfl_up(v.score, d, kWave), __shfl_up(v.pos, d, kWave)}; }
};

// Segmented inclusive scan over the 256 positions of a tile, continuing the previous tiles' scan: position 0 combines with *carry
// unless it is a segment head, and the last position leaves its result in *carry.  All 256 threads call it (a position past the end
// passes Op::id() and head = false).  sh_v[4] / sh_f[4] are scratch in LDS.  Within a wave: six shuffle steps (Hillis-Steele with the
// head flags OR-ed along); across the four waves: the wave totals go through LDS and every thread combines those before its own.
template <class Op>
__device__ __forceinline__ typename Op::T fit_scan(typename Op::T v, bool head, typename Op::T* carry, typename Op::T* sh_v, int* sh_f) {
  using T = typename Op::T;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid >> 6;
  if (tid == 0 && !head) v = Op::op(*carry, v);
  int f = head ? 1 : 0;
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const T u = Op::up(v, d);
    const int fu = __shfl_up(f, d, kWave);
    if (lane >= d) {
      if (!f) v = Op::op(u, v);
      f |= fu;
    }
  }
  if (lane == kWave - 1) { sh_v[wv] = v; sh_f[wv] = f; }
  __syncthreads();
  T pre = Op::id();
#pragma unroll
  for (int j = 0; j < kBlock / kWave - 1; ++j) {
    if (j < wv) pre = sh_f[j] ? sh_v[j] : Op::op(pre, sh_v[j]);
  }
  if (!f && wv > 0) v = Op::op(pre, v);
  if (tid == kBlock - 1) *carry = v;
  __syncthreads();
  return v;
}

__device__ __forceinline__ int fit_clamp(int v, int lo, int hi) { return min(max(v, lo), hi); }

struct FitLevel { int nseg, m, nodes; };
__device__ __forceinline__ FitLevel fit_level(const mlqem_forest_fit_state& s, int buf, int t) {
  const int n = (int)s.n;
  const fit_i4 v = reinterpret_cast<const fit_i4*>(s.level)[(size_t)buf * s.Tc + t];
  FitLevel l;
  l.m = fit_clamp(v.y, 0, n);
  l.nseg = fit_clamp(v.x, 0, l.m);          // every live segment holds a row
  l.nodes = fit_clamp(v.z, 1, 2 * n - 1);
  return l;
}

// ---- init: the root's row lists ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void fit_init_kernel(mlqem_forest_fit_state s) {
  __shared__ int sh_v[4], sh_f[4], sh_carry;
  const int tid = threadIdx.x, n = (int)s.n;
  const int t = blockIdx.x / s.F, f = blockIdx.x - t * s.F;
  const int32_t* ord = s.order + (size_t)f * n;
  const int32_t* cnt = s.counts + (size_t)t * n;
  int32_t* list = s.rows + ((size_t)t * s.F + f) * n;   // buffer 0
  if (tid == 0) sh_carry = 0;
  __syncthreads();
  for (int base = 0; base < n; base += kBlock) {
    const int j = base + tid;
    const int r = fit_clamp(ord[min(j, n - 1)], 0, n - 1);
    const bool in_bag = j < n && cnt[r] > 0;
    const int at = fit_scan<FitAddI>(in_bag ? 1 : 0, false, &sh_carry, sh_v, sh_f) - 1;
    if (in_bag) {
      list[fit_clamp(at, 0, n - 1)] = r;
      if (f == 0) s.segid[(size_t)t * n + fit_clamp(at, 0, n - 1)] = 0;
    }
  }
  if (f == 0 && tid == 0) {
    const int m = sh_carry;   // written before the scan's closing barrier
    reinterpret_cast<fit_i4*>(s.level)[t] = fit_i4{1, m, 1, 0};
    reinterpret_cast<fit_i4*>(s.seg_i)[(size_t)t * n] = fit_i4{0, m, 0, 0};
  }
}

// ---- stats: W, sum w y^2, S[K] of every live segment ------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void fit_stats_kernel(mlqem_forest_fit_state s, int buf) {
  __shared__ double sh_v[4], sh_carry[kFitMaxK + 2];
  __shared__ int sh_f[4];
  const int tid = threadIdx.x, n = (int)s.n, K = s.K, F = s.F;
  const int t = blockIdx.x;
  const FitLevel lv = fit_level(s, buf, t);
  if (lv.nseg == 0) return;
  const size_t tb = (size_t)buf * s.Tc + t;
  const int32_t* segid = s.segid + tb * n;
  const fit_i4* segi = reinterpret_cast<const fit_i4*>(s.seg_i) + tb * n;
  const int32_t* cnt = s.counts + (size_t)t * n;
  double* stat = s.seg_stat + (size_t)t * n * (K + 2);
  if (tid < kFitMaxK + 2) sh_carry[tid] = 0.0;
  __syncthreads();
  for (int base = 0; base < lv.m; base += kBlock) {
    const int p = base + tid, pc = min(p, lv.m - 1);
    const bool valid = p < lv.m;
    const int sg = fit_clamp(segid[pc], 0, lv.nseg - 1);
    const fit_i4 si = segi[sg];                       // start, rows, node, the feature whose list orders the sums
    const int f = fit_clamp(si.w, 0, F - 1);
    const int r = fit_clamp(s.rows[(tb * F + f) * n + pc], 0, n - 1);
    const double w = valid ? (double)cnt[r] : 0.0;
    const bool head = valid && p == si.x, last = valid && p == si.x + si.y - 1;
    const double* yr = s.y + (size_t)r * K;
    double q = 0.0;
    for (int k = 0; k < K; ++k) q += (w * yr[k]) * yr[k];
    double* out = stat + (size_t)sg * (K + 2);
    const double W = fit_scan<FitAddD>(w, head, &sh_carry[0], sh_v, sh_f);
    const double Q = fit_scan<FitAddD>(q, head, &sh_carry[1], sh_v, sh_f);
    if (last) { out[0] = W; out[1] = Q; }
    for (int k = 0; k < K; ++k) {
      const double S = fit_scan<FitAddD>(w * yr[k], head, &sh_carry[2 + k], sh_v, sh_f);
      if (last) out[2 + k] = S;
    }
  }
}

// ---- search: the best candidate of every (tree, feature, segment) ------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void fit_search_kernel(mlqem_forest_fit_state s, int buf) {
  __shared__ double sh_v[4], sh_carry[kFitMaxK + 1];
  __shared__ FitBest sh_b[4], sh_bcarry;
  __shared__ int sh_f[4];
  const int tid = threadIdx.x, n = (int)s.n, K = s.K, F = s.F;
  const int t = blockIdx.x / F, f = blockIdx.x - t * F;
  const FitLevel lv = fit_level(s, buf, t);
  if (lv.nseg == 0) return;
  const size_t tb = (size_t)buf * s.Tc + t;
  const int32_t* segid = s.segid + tb * n;
  const fit_i4* segi = reinterpret_cast<const fit_i4*>(s.seg_i) + tb * n;
  const int32_t* list = s.rows + (tb * F + f) * n;
  const int32_t* cnt = s.counts + (size_t)t * n;
  const double* stat = s.seg_stat + (size_t)t * n * (K + 2);
  const size_t cand = ((size_t)t * F + f) * n;
  if (tid < kFitMaxK + 1) sh_carry[tid] = 0.0;
  if (tid == 0) sh_bcarry = FitMaxB::id();
  __syncthreads();
  for (int base = 0; base < lv.m; base += kBlock) {
    const int p = base + tid, pc = min(p, lv.m - 1);
    const bool valid = p < lv.m;
    const int sg = fit_clamp(segid[pc], 0, lv.nseg - 1);
    const fit_i4 si = segi[sg];
    const int r = fit_clamp(list[pc], 0, n - 1);
    const int rn = fit_clamp(list[min(p + 1, lv.m - 1)], 0, n - 1);
    const float v = s.x[(size_t)r * s.ldx + f], vn = s.x[(size_t)rn * s.ldx + f];
    const double w = valid ? (double)cnt[r] : 0.0;
    const bool head = valid && p == si.x, last = valid && p == si.x + si.y - 1;
    const double* yr = s.y + (size_t)r * K;
    const double* tot = stat + (size_t)sg * (K + 2);
    const double wl = fit_scan<FitAddD>(w, head, &sh_carry[0], sh_v, sh_f);
    double acc_l = 0.0, acc_r = 0.0;
    for (int k = 0; k < K; ++k) {
      const double sl = fit_scan<FitAddD>(w * yr[k], head, &sh_carry[1 + k], sh_v, sh_f);
      const double sr = tot[2 + k] - sl;
      acc_l += sl * sl;
      acc_r += sr * sr;
    }
    // the candidate that separates this position from the next one of its segment
    const int n_left = p - si.x + 1, n_right = si.y - n_left;
    const bool is_cand = valid && !last && n_right >= 1 && vn > v + kFitFeatureGap && n_left >= s.min_samples_leaf &&
                         n_right >= s.min_samples_leaf;
    const double score = acc_l / wl + acc_r / (tot[0] - wl);
    FitBest b = is_cand ? FitBest{score, p + 1} : FitMaxB::id();
    b = fit_scan<FitMaxB>(b, head, &sh_bcarry, sh_b, sh_f);
    if (last) {
      s.cand_score[cand + sg] = b.score;
      s.cand_pos[cand + sg] = b.pos;
    }
  }
}

// ---- select: leaf or split, node records, the next level's segments ----------------------------------------------------------------
// The per-node feature order of max_features < F (include/mlqem_hip.h states the rule): a Feistel permutation of [0, 4^h) keyed by
// (seed, forest tree, node), walked along its cycle until it lands below F.  All arithmetic is uint32.
struct FitSubset { int m, h; uint32_t seed, tree_base; };

__device__ __forceinline__ uint32_t fit_mix(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
  return x;
}

__device__ __forceinline__ uint32_t fit_feistel(uint32_t v, uint32_t key, int h) {
  const uint32_t mask = (1u << h) - 1u;
  uint32_t l = v >> h, r = v & mask;
#pragma unroll
  for (uint32_t round = 0; round < 8; ++round) {
    const uint32_t nr = l ^ (fit_mix(r ^ key ^ (round * 0x9e3779b9u)) & mask);
    l = r;
    r = nr;
  }
  return (l << h) | r;
}

// pi(i) of the node with this key: at most D = 4^h steps along the cycle of i (E is a bijection of [0, D) and i < F, so the cycle
// returns below F), clamped to F - 1 whatever the arguments.  No memory is touched: the lane-varying trip count guards no load.
__device__ __forceinline__ int fit_perm(uint32_t i, uint32_t key, int h, int F) {
  const uint32_t D = 1u << (2 * h);
  uint32_t v = fit_feistel(i & (D - 1u), key, h);
  for (uint32_t step = 1; step < D && v >= (uint32_t)F; ++step) v = fit_feistel(v, key, h);
  return (int)min(v, (uint32_t)(F - 1));
}

// One body for both kernels: kSubset = false searches every feature (fit_select_kernel), kSubset = true the node's own subset
// (fit_select_subset_kernel); leaf tests, threshold, node record and the two numbering scans are the same code.  The state comes
// by value, as the kernels get it: so the plain kernel compiles to the instructions it had before the body was shared.
template <bool kSubset>
__device__ __forceinline__ void fit_select_body(mlqem_forest_fit_state s, int buf, int depth, FitSubset sub) {
  __shared__ int sh_v[4], sh_f[4], sh_carry[2];
  const int tid = threadIdx.x, n = (int)s.n, K = s.K, F = s.F;
  const int t = blockIdx.x;
  const int max_nodes = 2 * n - 1;
  const FitLevel lv = fit_level(s, buf, t);
  fit_i4* next_level = reinterpret_cast<fit_i4*>(s.level) + (size_t)(buf ^ 1) * s.Tc + t;
  if (lv.nseg == 0) {
    if (tid == 0) *next_level = fit_i4{0, 0, lv.nodes, 0};
    return;
  }
  const size_t tb = (size_t)buf * s.Tc + t, tn = (size_t)(buf ^ 1) * s.Tc + t;
  const fit_i4* segi = reinterpret_cast<const fit_i4*>(s.seg_i) + tb * n;
  fit_i4* segi_next = reinterpret_cast<fit_i4*>(s.seg_i) + tn * n;
  const double* stat = s.seg_stat + (size_t)t * n * (K + 2);
  fit_i4* split_i = reinterpret_cast<fit_i4*>(s.split_i) + (size_t)t * n;
  double* split_thr = s.split_thr + (size_t)t * n;
  fit_i4* node_i = reinterpret_cast<fit_i4*>(s.node_i) + (size_t)t * max_nodes;
  double* node_thr = s.node_thr + (size_t)t * max_nodes;
  double* node_value = s.node_value + (size_t)t * max_nodes * K;
  if (tid < 2) sh_carry[tid] = 0;
  __syncthreads();
  for (int base = 0; base < lv.nseg; base += kBlock) {
    const int sg = base + tid, sc = min(sg, lv.nseg - 1);
    const bool valid = sg < lv.nseg;
    const fit_i4 si = segi[sc];
    const int start = fit_clamp(si.x, 0, lv.m - 1), rows = fit_clamp(si.y, 1, lv.m - start);
    const int node = fit_clamp(si.z, 0, max_nodes - 1);
    const double* tot = stat + (size_t)sc * (K + 2);
    const double W = tot[0];
    double impurity = tot[1] / W;
    for (int k = 0; k < K; ++k) {
      const double mean = tot[2 + k] / W;
      impurity -= mean * mean;
    }
    impurity /= (double)K;
    bool leaf = depth >= s.max_depth || rows < s.min_samples_split || rows < 2 * s.min_samples_leaf || impurity <= kFitEps;
    double best = -INFINITY;
    int best_pos = -1, best_f = -1;
    if constexpr (!kSubset) {
      for (int f = 0; f < F; ++f) {   // feature order: on equal scores the lowest feature keeps the split
        const size_t at = ((size_t)t * F + f) * n + sc;
        const double score = s.cand_score[at];
        const int pos = s.cand_pos[at];
        const bool better = pos >= 0 && score > best;
        best = better ? score : best;
        best_pos = better ? pos : best_pos;
        best_f = better ? f : best_f;
      }
    } else {
      // The node visits pi(0), pi(1), ... and stops after the smallest count >= m at which a visited feature has a candidate.  Every
      // lane runs to the largest count of its wave (the exit is a wave vote, so no load sits behind a lane-varying branch): a lane
      // that is done keeps loading at its clamped address and masks what it read.  A lane that is a leaf anyway visits nothing.
      const uint32_t key = fit_mix(fit_mix(fit_mix(sub.seed) ^ (sub.tree_base + (uint32_t)t)) ^ (uint32_t)node);
      bool done = !valid || leaf;
      int with_cand = 0;
      for (int i = 0; i < F; ++i) {
        if (__all(done)) break;
        const int f = fit_perm((uint32_t)i, key, sub.h, F);
        const size_t at = ((size_t)t * F + f) * n + sc;
        const double score = s.cand_score[at];
        const int pos = s.cand_pos[at];
        const bool has = !done && pos >= 0;
        const bool better = has && (score > best || (score == best && f < best_f));   // equal scores: the lowest feature
        best = better ? score : best;
        best_pos = better ? pos : best_pos;
        best_f = better ? f : best_f;
        with_cand += has ? 1 : 0;
        done = done || (i + 1 >= sub.m && with_cand > 0);
      }
    }
    leaf = leaf || best_f < 0 || rows < 2;
    const bool split = valid && !leaf;
    const int f = fit_clamp(best_f, 0, F - 1);
    const int pos = fit_clamp(best_pos, start + 1, max(start + rows - 1, start + 1));   // the first position of the right child
    const int32_t* list = s.rows + (tb * F + f) * n;
    const int ra = fit_clamp(list[min(pos - 1, n - 1)], 0, n - 1), rb = fit_clamp(list[min(pos, n - 1)], 0, n - 1);
    const double va = (double)s.x[(size_t)ra * s.ldx + f], vb = (double)s.x[(size_t)rb * s.ldx + f];
    double thr = va / 2.0 + vb / 2.0;
    if (thr == vb || isinf(thr)) thr = va;
    const int n_left = pos - start;
    const int rank = fit_scan<FitAddI>(split ? 1 : 0, false, &sh_carry[0], sh_v, sh_f) - (split ? 1 : 0);
    const int dst = fit_scan<FitAddI>(split ? rows : 0, false, &sh_carry[1], sh_v, sh_f) - (split ? rows : 0);
    const int child_seg = 2 * rank, child_node = lv.nodes + 2 * rank;
    if (valid) {
      node_i[node] = split ? fit_i4{f, child_node, child_node + 1, rows} : fit_i4{-2, -1, -1, rows};
      node_thr[node] = split ? thr : -2.0;
      for (int k = 0; k < K; ++k) node_value[(size_t)node * K + k] = tot[2 + k] / W;
      split_i[sc] = split ? fit_i4{f, dst, n_left, child_seg} : fit_i4{-1, 0, 0, 0};
      split_thr[sc] = thr;
    }
    if (split && child_seg + 1 < n && child_node + 1 < max_nodes) {
      segi_next[child_seg] = fit_i4{dst, n_left, child_node, f};
      segi_next[child_seg + 1] = fit_i4{dst + n_left, rows - n_left, child_node + 1, f};
    }
  }
  if (tid == 0) {   // the carries hold the totals (written before the scans' closing barriers)
    const int splits = fit_clamp(sh_carry[0], 0, (max_nodes - lv.nodes) / 2);
    *next_level = fit_i4{2 * splits, sh_carry[1], lv.nodes + 2 * splits, 0};
  }
}

__global__ __launch_bounds__(kBlock) void fit_select_kernel(mlqem_forest_fit_state s, int buf, int depth) {
  fit_select_body<false>(s, buf, depth, FitSubset{});
}

__global__ __launch_bounds__(kBlock) void fit_select_subset_kernel(mlqem_forest_fit_state s, int buf, int depth, FitSubset sub) {
  fit_select_body<true>(s, buf, depth, sub);
}

// ---- partition: the next level's row lists -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void fit_partition_kernel(mlqem_forest_fit_state s, int buf) {
  __shared__ int sh_v[4], sh_f[4], sh_carry;
  const int tid = threadIdx.x, n = (int)s.n, F = s.F;
  const int t = blockIdx.x / F, f = blockIdx.x - t * F;
  const FitLevel lv = fit_level(s, buf, t);
  if (lv.nseg == 0) return;
  const size_t tb = (size_t)buf * s.Tc + t, tn = (size_t)(buf ^ 1) * s.Tc + t;
  const int32_t* segid = s.segid + tb * n;
  int32_t* segid_next = s.segid + tn * n;
  const fit_i4* segi = reinterpret_cast<const fit_i4*>(s.seg_i) + tb * n;
  const fit_i4* split_i = reinterpret_cast<const fit_i4*>(s.split_i) + (size_t)t * n;
  const double* split_thr = s.split_thr + (size_t)t * n;
  const int32_t* list = s.rows + (tb * F + f) * n;
  int32_t* list_next = s.rows + (tn * F + f) * n;
  if (tid == 0) sh_carry = 0;
  __syncthreads();
  for (int base = 0; base < lv.m; base += kBlock) {
    const int p = base + tid, pc = min(p, lv.m - 1);
    const bool valid = p < lv.m;
    const int sg = fit_clamp(segid[pc], 0, lv.nseg - 1);
    const fit_i4 si = segi[sg];
    const fit_i4 sp = split_i[sg];                    // split feature or -1, first destination, rows going left, left child's segment
    const int r = fit_clamp(list[pc], 0, n - 1);
    const bool split = valid && sp.x >= 0;
    const float xv = s.x[(size_t)r * s.ldx + fit_clamp(sp.x, 0, F - 1)];
    const bool left = (double)xv <= split_thr[sg];
    const bool head = valid && p == si.x;
    const int lefts = fit_scan<FitAddI>(split && left ? 1 : 0, head, &sh_carry, sh_v, sh_f);   // of the segment, up to and with p
    const int rights = p - si.x + 1 - lefts;
    const int dst = fit_clamp(left ? sp.y + lefts - 1 : sp.y + sp.z + rights - 1, 0, n - 1);
    if (split) {
      list_next[dst] = r;
      if (f == 0) segid_next[dst] = sp.w + (left ? 0 : 1);
    }
  }
}

int fit_check(const mlqem_forest_fit_state* s) {
  if (!s) return MLQEM_ERR_BAD_ARG;
  if (s->n < 1 || s->F < 1 || s->K < 1 || s->Tc < 1 || s->ldx < s->F || s->min_samples_split < 2 || s->min_samples_leaf < 1 ||
      s->max_depth < 0)
    return MLQEM_ERR_BAD_ARG;
  if (s->n > (1 << 22) || s->K > kFitMaxK || s->F > 32767 || (int64_t)s->Tc * s->F > 0x7FFFFFFFll) return MLQEM_ERR_UNSUPPORTED;
  if (!s->x || !s->y || !s->counts || !s->order || !s->rows || !s->segid || !s->level || !s->seg_i || !s->seg_stat ||
      !s->cand_score || !s->cand_pos || !s->split_i || !s->split_thr || !s->node_i || !s->node_thr || !s->node_value)
    return MLQEM_ERR_BAD_ARG;
  if (!aligned_to(s->level, 16) || !aligned_to(s->seg_i, 16) || !aligned_to(s->split_i, 16) || !aligned_to(s->node_i, 16))
    return MLQEM_ERR_BAD_ARG;
  return MLQEM_OK;
}

}  // namespace
}  // namespace mlqem

using namespace mlqem;

extern "C" size_t mlqem_forest_fit_tree_bytes(int64_t n, int F, int K) {
  if (n < 1 || F < 1 || K < 1) return 0;
  const size_t N = (size_t)n, nodes = 2 * N - 1;
  return 2 * (size_t)F * N * 4      // rows
         + 2 * N * 4                // segid
         + 2 * 16                   // level
         + 2 * N * 16               // seg_i
         + N * (size_t)(K + 2) * 8  // seg_stat
         + (size_t)F * N * 12       // cand_score, cand_pos
         + N * 16 + N * 8           // split_i, split_thr
         + nodes * 16 + nodes * 8 + nodes * (size_t)K * 8;   // node_i, node_thr, node_value
}

extern "C" int mlqem_forest_fit_init(const mlqem_forest_fit_state* s, mlqem_stream_t stream) {
  begin_launches();
  if (const int code = fit_check(s)) return code;
  hipLaunchKernelGGL(fit_init_kernel, dim3((unsigned)(s->Tc * s->F)), dim3(kBlock), 0, as_stream(stream), *s);
  return launch_status();
}

extern "C" int mlqem_forest_fit_stats(const mlqem_forest_fit_state* s, int level, mlqem_stream_t stream) {
  begin_launches();
  if (const int code = fit_check(s)) return code;
  if (level < 0) return MLQEM_ERR_BAD_ARG;
  hipLaunchKernelGGL(fit_stats_kernel, dim3((unsigned)s->Tc), dim3(kBlock), 0, as_stream(stream), *s, level & 1);
  return launch_status();
}

extern "C" int mlqem_forest_fit_search(const mlqem_forest_fit_state* s, int level, mlqem_stream_t stream) {
  begin_launches();
  if (const int code = fit_check(s)) return code;
  if (level < 0) return MLQEM_ERR_BAD_ARG;
  hipLaunchKernelGGL(fit_search_kernel, dim3((unsigned)(s->Tc * s->F)), dim3(kBlock), 0, as_stream(stream), *s, level & 1);
  return launch_status();
}

extern "C" int mlqem_forest_fit_select(const mlqem_forest_fit_state* s, int level, mlqem_stream_t stream) {
  begin_launches();
  if (const int code = fit_check(s)) return code;
  if (level < 0) return MLQEM_ERR_BAD_ARG;
  hipLaunchKernelGGL(fit_select_kernel, dim3((unsigned)s->Tc), dim3(kBlock), 0, as_stream(stream), *s, level & 1, level);
  return launch_status();
}

extern "C" int mlqem_forest_fit_select_subset(const mlqem_forest_fit_state* s, int level, int max_features, uint32_t seed,
                                              int64_t tree_base, mlqem_stream_t stream) {
  begin_launches();
  if (const int code = fit_check(s)) return code;
  if (level < 0 || max_features < 1 || tree_base < 0) return MLQEM_ERR_BAD_ARG;
  if (max_features >= s->F) {   // every feature is visited: the plain kernel, bit for bit
    hipLaunchKernelGGL(fit_select_kernel, dim3((unsigned)s->Tc), dim3(kBlock), 0, as_stream(stream), *s, level & 1, level);
    return launch_status();
  }
  int bits = 0;   // h = max(1, ceil(bit_length(F - 1) / 2)): F <= 4^h <= 4 F, and F <= 32767 keeps h <= 8
  while (bits < 31 && ((s->F - 1) >> bits) != 0) ++bits;
  const FitSubset sub{max_features, bits < 2 ? 1 : (bits + 1) / 2, seed, (uint32_t)tree_base};
  hipLaunchKernelGGL(fit_select_subset_kernel, dim3((unsigned)s->Tc), dim3(kBlock), 0, as_stream(stream), *s, level & 1, level, sub);
  return launch_status();
}

extern "C" int mlqem_forest_fit_partition(const mlqem_forest_fit_state* s, int level, mlqem_stream_t stream) {
  begin_launches();
  if (const int code = fit_check(s)) return code;
  if (level < 0) return MLQEM_ERR_BAD_ARG;
  hipLaunchKernelGGL(fit_partition_kernel, dim3((unsigned)(s->Tc * s->F)), dim3(kBlock), 0, as_stream(stream), *s, level & 1);
  return launch_status();
}
