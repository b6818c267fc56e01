// Measurement shots of Clifford circuits of up to 512 qubits under the depolarising + readout model, by Pauli-frame sampling
// (mlqem_clifford_sample_f64): no state vector.  include/mlqem_hip.h has the contract, the rule of every draw included; a host
// interpreter restates it and the device equals it to the last bit.  Four kernels per call, on one stream:
//   pullback_kernel   a thread per (group, qubit): P_q = U^dagger B_q U by clifford.hip's backward step (clf_step, noise records
//                     ignored), its x words, z words and sign stored as a ROW of 2 W + 1 words.  REG / LDS split as in walk_kernel.
//   reference_kernel  a wave per group: the rows in LDS (n = 512: 512 x 33 words + 512 pivot slots = 68 KB), Gaussian elimination
//                     over the x parts in qubit order, lanes over the words of a row product, a wave reduction for its sign; gives
//                     the reference outcome m.  Serial in q by construction.
//   frames_kernel     the hot path: a thread per shot, workgroups over (group, block of 256 shots).  The frame is the lane's eight
//                     words in registers (W <= 4, compile-time selects, no scratch) or its LDS column (W <= 16).  Records are loaded
//                     four ahead with their thresholds; one Philox block serves two records and is skipped where neither is a noise
//                     record (the records are the same for every lane of the workgroup).  Term sums: a wave reduction, then one
//                     integer atomic per (wave, term) into the zeroed buffer.  Loads unconditional on clamped indices, stores
//                     predicated.
//   finish_kernel     a thread per circuit: estimates, values, variances in mlqem_sim_sample_f64's fused multiply-add order.
// No float atomics, no host read: capturable.
#include "clifford_words.hpp"
#include "sim_ctx.hpp"

namespace mlqem {
namespace {

constexpr uint32_t kFrmDomainZ = 0u << 30, kFrmDomainNoise = 1u << 30, kFrmDomainReadout = 2u << 30;
// pivot slots + rows of the widest group: (512 + 512 * 33) words
constexpr size_t kFrmRefMaxLds = (size_t)(MLQEM_CLIFFORD_MAX_QUBITS + MLQEM_CLIFFORD_MAX_QUBITS * (2 * kClfMaxWords + 1)) * 4;

__device__ __forceinline__ int frm_wave_sum(int v) {
#pragma unroll
  for (int d = kWave / 2; d >= 1; d >>= 1) v = v + __shfl_down(v, d, kWave);
  return v;   // lane 0 has the sum
}

template <class T> __device__ __forceinline__ T frm_clamp(T v, T lo, T hi) { return min(max(v, lo), hi); }

// the (circuit, n, W) of group g, everything clamped
struct FrmGroup { int c, n, W; };
template <bool REG>
__device__ __forceinline__ FrmGroup frm_group(int g, int n_circuits, const int32_t* __restrict__ n_qubits,
                                              const int32_t* __restrict__ group_circ, int max_qubits) {
  FrmGroup out;
  out.c = frm_clamp(group_circ[g], 0, n_circuits - 1);
  out.n = min(frm_clamp(n_qubits[out.c], 1, REG ? 32 * kClfRegWords : 32 * kClfMaxWords), max_qubits);
  out.W = (out.n + 31) >> 5;
  return out;
}

template <bool REG>
__global__ __launch_bounds__(kBlock) void pullback_kernel(int n_circuits, const int32_t* __restrict__ n_qubits,
                                                          const int64_t* __restrict__ op_ptr, const clf_i4* __restrict__ ops,
                                                          int64_t n_ops, const int32_t* __restrict__ group_circ,
                                                          const int32_t* __restrict__ group_mask, int n_groups,
                                                          const int32_t* __restrict__ ids, const uint32_t* __restrict__ masks,
                                                          int64_t n_masks, const int64_t* __restrict__ row_ptr,
                                                          uint32_t* __restrict__ rows, int64_t n_rows, int max_qubits) {
  constexpr int WCAP = REG ? kClfRegWords : kClfMaxWords;
  __shared__ uint32_t lds[REG ? 1 : 2 * kClfMaxWords * kBlock];
  const int g = frm_clamp(ids[blockIdx.x], 0, n_groups - 1);
  const FrmGroup gr = frm_group<REG>(g, n_circuits, n_qubits, group_circ, max_qubits);
  const int c = gr.c, n = gr.n, W = gr.W;
  const int q = (int)blockIdx.y * kBlock + (int)threadIdx.x;
  const bool live = q < n;
  const int qa = min(q, n - 1), wq = qa >> 5, bq = qa & 31;
  const int64_t gm = group_mask[g];
  const uint32_t bxw = masks[frm_clamp(gm + wq, (int64_t)0, n_masks - 1)];
  const uint32_t bzw = masks[frm_clamp(gm + W + wq, (int64_t)0, n_masks - 1)];
  const uint32_t lx = ((bxw >> bq) & 1u) << bq, lz = ((bzw >> bq) & 1u) << bq;   // B_q: the basis letter on qubit q alone
  ClfWords<REG> p(lds, threadIdx.x);
  if constexpr (REG) {
#pragma unroll
    for (int w = 0; w < WCAP; ++w) p.init(w, w == wq ? lx : 0u, w == wq ? lz : 0u);
  } else {
    for (int w = 0; w < W; ++w) p.init(w, w == wq ? lx : 0u, w == wq ? lz : 0u);
  }
  const int64_t ob = frm_clamp(op_ptr[c], (int64_t)0, n_ops), oe = frm_clamp(op_ptr[c + 1], ob, n_ops);
  uint32_t sign = 0;
  double factor = 1.0;   // dead: noise records are ignored here
  for (int64_t k = oe - 1; k >= ob; k -= kClfChunk) {
    clf_i4 r[kClfChunk];
#pragma unroll
    for (int j = 0; j < kClfChunk; ++j) r[j] = ops[max(k - j, ob)];
#pragma unroll
    for (int j = 0; j < kClfChunk; ++j) {
      if (k - j < ob) break;
      clf_step<REG, false>(p, sign, factor, n, r[j], 1.0, false);
    }
  }
  const int S = 2 * W + 1;
  const int64_t rb = row_ptr[g];
  const int64_t base = rb + (int64_t)qa * S;
  if (live && rb >= 0 && base + S <= n_rows) {
    if constexpr (REG) {
#pragma unroll
      for (int w = 0; w < WCAP; ++w)
        if (w < W) {
          rows[base + w] = p.getx(w);
          rows[base + W + w] = p.getz(w);
        }
    } else {
      for (int w = 0; w < W; ++w) {
        rows[base + w] = p.getx(w);
        rows[base + W + w] = p.getz(w);
      }
    }
    rows[base + 2 * W] = sign & 1u;
  }
}

// One wave per group.  LDS: piv[32 Wm] (the row whose lowest x bit is at that position, or -1), then the group's rows; word 2 W
// of a row is sign | v << 1 once the row is a pivot.
__global__ __launch_bounds__(kWave) void reference_kernel(int n_circuits, const int32_t* __restrict__ n_qubits,
                                                          const int32_t* __restrict__ group_circ, int n_groups,
                                                          const int64_t* __restrict__ row_ptr, const uint32_t* __restrict__ rows,
                                                          int64_t n_rows, const int64_t* __restrict__ ref_ptr,
                                                          uint32_t* __restrict__ reference, int64_t n_ref, int max_qubits) {
  extern __shared__ uint32_t frm_lds[];
  const int g = min((int)blockIdx.x, n_groups - 1);
  const FrmGroup gr = frm_group<false>(g, n_circuits, n_qubits, group_circ, max_qubits);
  const int n = gr.n, W = gr.W, S = 2 * W + 1;
  const int lane = (int)threadIdx.x;
  int* piv = reinterpret_cast<int*>(frm_lds);
  uint32_t* L = frm_lds + 32 * ((max_qubits + 31) >> 5);
  const int64_t rb = row_ptr[g];
  const int64_t base = rb >= 0 && rb + (int64_t)n * S <= n_rows ? rb : 0;
  for (int i = lane; i < n * S; i += kWave) L[i] = rows[min(base + i, n_rows - 1)];
  for (int i = lane; i < 32 * W; i += kWave) piv[i] = -1;
  sim_sync<false>();
  uint32_t mword = 0;   // lane w < W: word w of the reference outcome
  for (int q = 0; q < n; ++q) {
    uint32_t* row = L + q * S;
    const int wl = min(lane, W - 1);
    uint32_t x1 = lane < W ? row[wl] : 0u, z1 = lane < W ? row[W + wl] : 0u;
    uint32_t sign = row[2 * W] & 1u, acc = 0u, mbit = 0u;
    for (int it = 0; it <= 32 * W; ++it) {   // every product raises the row's lowest x bit: at most 32 W of them
      const unsigned long long has = __ballot(x1 != 0u);
      if (!has) {   // +-Z_T, and Z_T = +1 on |0..0>
        mbit = sign ^ acc;
        break;
      }
      const int lw = __ffsll(has) - 1;
      const uint32_t word = (uint32_t)__builtin_amdgcn_readlane((int)x1, lw);
      const int pos = lw * 32 + __ffs((int)word) - 1;
      const int pv = piv[pos];
      if (pv < 0 || pv >= q) {   // (pv >= q: never for a table this kernel wrote) the row becomes the pivot of `pos`, m_q = 0
        if (lane < W) {
          row[wl] = x1;
          row[W + wl] = z1;
        }
        if (lane == 0) {
          row[2 * W] = sign | (acc << 1);
          piv[pos] = q;
        }
        break;
      }
      const uint32_t* prow = L + pv * S;
      const uint32_t x2 = lane < W ? prow[wl] : 0u, z2 = lane < W ? prow[W + wl] : 0u;
      const uint32_t tail = prow[2 * W];
      // Aaronson-Gottesman: the exponent of i the letters of (x1, z1) . (x2, z2) pick up, +1 and -1 counted apart
      const uint32_t plus = (x1 & z1 & z2 & ~x2) | (x1 & ~z1 & z2 & x2) | (~x1 & z1 & x2 & ~z2);
      const uint32_t minus = (x1 & z1 & x2 & ~z2) | (x1 & ~z1 & z2 & ~x2) | (~x1 & z1 & x2 & z2);
      const int total = __builtin_amdgcn_readfirstlane(frm_wave_sum(__popc(plus) - __popc(minus)));
      sign ^= (tail & 1u) ^ ((uint32_t)(total >> 1) & 1u);
      acc ^= (tail >> 1) & 1u;
      x1 ^= x2;
      z1 ^= z2;
    }
    mword |= lane == (q >> 5) ? mbit << (q & 31) : 0u;
    sim_sync<false>();
  }
  const int64_t rf = ref_ptr[g];
  if (lane < W && rf >= 0 && rf + W <= n_ref) reference[rf + lane] = mword;
}

// One record applied to the frame: U F U^dagger for a gate record (the inverse of the stored table, the sign dropped), a random
// Pauli for a noise record that is hit.  (v_lo, v_hi): the record's 64-bit draw.
template <bool REG>
__device__ __forceinline__ void frm_step(ClfWords<REG>& p, const int n, const clf_i4 rec, const uint64_t T, const uint32_t v_lo,
                                         const uint32_t v_hi) {
  const int kind = rec.x & 15;
  if (kind == MLQEM_CLIFFORD_OP_C1 || kind == MLQEM_CLIFFORD_OP_C2) {
    uint32_t sign = 0;
    double factor = 1.0;
    clf_step<REG, true>(p, sign, factor, n, rec, 1.0, true);
  } else if (kind == MLQEM_CLIFFORD_OP_DEPOL1 || kind == MLQEM_CLIFFORD_OP_DEPOL2) {
    const int q0 = min((rec.x >> 4) & 1023, n - 1), q1 = min((rec.x >> 14) & 1023, n - 1);
    const uint64_t v = (uint64_t)v_lo | ((uint64_t)v_hi << 32);
    const bool hit = (v >> 4) < T;
    const uint32_t pl = hit ? v_lo & (kind == MLQEM_CLIFFORD_OP_DEPOL2 ? 15u : 3u) : 0u;
    p.flip(q0 >> 5, (pl & 1u) << (q0 & 31), ((pl >> 1) & 1u) << (q0 & 31));
    if (kind == MLQEM_CLIFFORD_OP_DEPOL2) p.flip(q1 >> 5, ((pl >> 2) & 1u) << (q1 & 31), ((pl >> 3) & 1u) << (q1 & 31));
  }
}

// Word w of the outcome, written over the frame's x word (a function on the words, not a closure around them: see clf_step).
template <bool REG>
__device__ __forceinline__ void frm_outcome(ClfWords<REG>& p, const int w, const int W, const int full, const uint32_t part,
                                            const int64_t gm, const int64_t rf, const uint32_t* __restrict__ reference,
                                            const int64_t n_ref, const uint32_t* __restrict__ masks, const int64_t n_masks) {
  const uint32_t m = reference[frm_clamp(rf + w, (int64_t)0, n_ref - 1)];
  const uint32_t bx = masks[frm_clamp(gm + w, (int64_t)0, n_masks - 1)];
  const uint32_t bz = masks[frm_clamp(gm + W + w, (int64_t)0, n_masks - 1)];
  const uint32_t keep = w < full ? ~0u : w == full ? part : 0u;
  const uint32_t x = p.getx(w), z = p.getz(w);
  p.init(w, (m ^ (x & bz) ^ (z & bx)) & keep, z);
}

template <bool REG>
__global__ __launch_bounds__(kBlock) void frames_kernel(
    int n_circuits, const int32_t* __restrict__ n_qubits, const int64_t* __restrict__ op_ptr, const clf_i4* __restrict__ ops,
    int64_t n_ops, const uint64_t* __restrict__ thresh, int64_t n_thresh, const int64_t* __restrict__ ro_ptr,
    const int64_t* __restrict__ group_ptr, const int32_t* __restrict__ group_circ, const int32_t* __restrict__ group_mask, int n_groups,
    const int32_t* __restrict__ ids, const uint32_t* __restrict__ masks, int64_t n_masks, const int64_t* __restrict__ gterm_ptr,
    const int32_t* __restrict__ gterm, int64_t n_gterm, const int32_t* __restrict__ term_mask, int64_t n_terms,
    const int64_t* __restrict__ run_keys, int shots, uint32_t seed_lo, uint32_t seed_hi, int max_qubits, int nblk,
    const int64_t* __restrict__ ref_ptr, const uint32_t* __restrict__ reference, int64_t n_ref, uint32_t* __restrict__ bits,
    int64_t n_bits, int32_t* __restrict__ term_sums) {
  constexpr int WCAP = REG ? kClfRegWords : kClfMaxWords;
  __shared__ uint32_t lds[REG ? 1 : 2 * kClfMaxWords * kBlock];
  const int slot = (int)(blockIdx.x / (unsigned)nblk), blk = (int)(blockIdx.x - (unsigned)slot * (unsigned)nblk);
  const int g = frm_clamp(ids[slot], 0, n_groups - 1);
  const FrmGroup gr = frm_group<REG>(g, n_circuits, n_qubits, group_circ, max_qubits);
  const int c = gr.c, n = gr.n, W = gr.W;
  const int gl = (int)((int64_t)g - frm_clamp(group_ptr[c], (int64_t)0, (int64_t)g)) & (MLQEM_CLIFFORD_MAX_GROUPS - 1);
  const int s = blk * kBlock + (int)threadIdx.x;   // < 2^20: shots <= 2^20 and nblk = ceil(shots / 256)
  const bool live = s < shots;
  const int64_t key = run_keys[c];
  const uint32_t key_lo = (uint32_t)(uint64_t)key, key_hi = (uint32_t)((uint64_t)key >> 32);
  const uint32_t c2 = (uint32_t)s | ((uint32_t)gl << 20);
  const int full = n >> 5;
  const uint32_t part = (1u << (n & 31)) - 1u;   // word `full` keeps these bits (0 when n is a multiple of 32)

  // the frame: x = 0, z = Philox words masked to n
  ClfWords<REG> p(lds, threadIdx.x);
  if constexpr (REG) {
    uint32_t x[4];
    philox4x32_10(key_lo, key_hi, c2, kFrmDomainZ, seed_lo, seed_hi, x);
#pragma unroll
    for (int w = 0; w < WCAP; ++w) p.init(w, 0u, w < full ? x[w] : w == full ? x[w] & part : 0u);
  } else {
    for (int wb = 0; 4 * wb < W; ++wb) {
      uint32_t x[4];
      philox4x32_10(key_lo, key_hi, c2, kFrmDomainZ | (uint32_t)wb, seed_lo, seed_hi, x);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int w = 4 * wb + e;
        if (w < W) p.init(w, 0u, w < full ? x[e] : w == full ? x[e] & part : 0u);
      }
    }
  }

  // the records, first to last, four per wait on memory; record i (counted from the circuit's first) draws words 2 (i & 1) and
  // 2 (i & 1) + 1 of block i >> 1, and a pair without a noise record draws nothing
  const int64_t ob = frm_clamp(op_ptr[c], (int64_t)0, n_ops), oe = frm_clamp(op_ptr[c + 1], ob, n_ops);
  for (int64_t k = ob; k < oe; k += kClfChunk) {
    clf_i4 r[kClfChunk];
    uint64_t T[kClfChunk];
#pragma unroll
    for (int j = 0; j < kClfChunk; ++j) r[j] = ops[min(k + j, oe - 1)];
#pragma unroll
    for (int j = 0; j < kClfChunk; ++j) T[j] = thresh[frm_clamp((int64_t)r[j].y, (int64_t)0, n_thresh - 1)];
#pragma unroll
    for (int h = 0; h < kClfChunk / 2; ++h) {
      const int k0 = r[2 * h].x & 15, k1 = r[2 * h + 1].x & 15;
      const bool noise0 = k + 2 * h < oe && (k0 == MLQEM_CLIFFORD_OP_DEPOL1 || k0 == MLQEM_CLIFFORD_OP_DEPOL2);
      const bool noise1 = k + 2 * h + 1 < oe && (k1 == MLQEM_CLIFFORD_OP_DEPOL1 || k1 == MLQEM_CLIFFORD_OP_DEPOL2);
      uint32_t x[4] = {0u, 0u, 0u, 0u};
      if (noise0 || noise1)
        philox4x32_10(key_lo, key_hi, c2, kFrmDomainNoise | (uint32_t)(((k - ob) >> 1) + h), seed_lo, seed_hi, x);
      if (k + 2 * h < oe) frm_step<REG>(p, n, r[2 * h], T[2 * h], x[0], x[1]);
      if (k + 2 * h + 1 < oe) frm_step<REG>(p, n, r[2 * h + 1], T[2 * h + 1], x[2], x[3]);
    }
  }

  // outcome bits, kept in the x words: m ^ (x & bz) ^ (z & bx)
  const int64_t gm = group_mask[g], rf = ref_ptr[g];
  if constexpr (REG) {
#pragma unroll
    for (int w = 0; w < WCAP; ++w)   // words past W: keep = 0, the clamped loads are masked out
      frm_outcome<REG>(p, w, W, full, part, gm, rf, reference, n_ref, masks, n_masks);
  } else {
    for (int w = 0; w < W; ++w) frm_outcome<REG>(p, w, W, full, part, gm, rf, reference, n_ref, masks, n_masks);
  }

  // readout: qubit q draws word q & 3 of block q >> 2 and flips iff it is below the threshold of its own bit
  const int64_t ro = ro_ptr[c];
  if (ro >= 0) {
    for (int qb = 0; 4 * qb < n; ++qb) {
      uint32_t x[4];
      philox4x32_10(key_lo, key_hi, c2, kFrmDomainReadout | (uint32_t)qb, seed_lo, seed_hi, x);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int q = 4 * qb + e;
        if (q < n) {
          const uint64_t t0 = thresh[frm_clamp(ro + 2 * q, (int64_t)0, n_thresh - 1)];
          const uint64_t t1 = thresh[frm_clamp(ro + 2 * q + 1, (int64_t)0, n_thresh - 1)];
          const uint32_t bit = (p.getx(q >> 5) >> (q & 31)) & 1u;
          const uint32_t flip = (uint64_t)x[e] < (bit ? t1 : t0) ? 1u : 0u;
          p.flip(q >> 5, flip << (q & 31), 0u);
        }
      }
    }
  }

  if (bits != nullptr) {
    const int64_t bb = rf * (int64_t)shots + (int64_t)s * W;
    if (live && rf >= 0 && bb + W <= n_bits) {
      if constexpr (REG) {
#pragma unroll
        for (int w = 0; w < WCAP; ++w)
          if (w < W) bits[bb + w] = p.getx(w);
      } else {
        for (int w = 0; w < W; ++w) bits[bb + w] = p.getx(w);
      }
    }
  }

  // S_t += sum over the block's shots of (-1)^popcount(bits & support_t)
  const int64_t tb = frm_clamp(gterm_ptr[g], (int64_t)0, n_gterm), te = frm_clamp(gterm_ptr[g + 1], tb, n_gterm);
  for (int64_t i = tb; i < te; ++i) {
    const int64_t t = frm_clamp((int64_t)gterm[i], (int64_t)0, n_terms - 1);
    const int64_t tm = term_mask[t];
    uint32_t par = 0;
    if constexpr (REG) {
#pragma unroll
      for (int w = 0; w < WCAP; ++w) par ^= p.getx(w) & masks[frm_clamp(tm + min(w, W - 1), (int64_t)0, n_masks - 1)];   // x words past W are 0
    } else {
      for (int w = 0; w < W; ++w) par ^= p.getx(w) & masks[frm_clamp(tm + w, (int64_t)0, n_masks - 1)];
    }
    const int sum = frm_wave_sum(live ? 1 - 2 * (int)(__popc(par) & 1) : 0);
    if ((threadIdx.x & (kWave - 1)) == 0) atomicAdd(&term_sums[t], sum);
  }
}

__global__ __launch_bounds__(kBlock) void frames_finish_kernel(int64_t n_circuits, const int64_t* __restrict__ term_ptr,
                                                               const double* __restrict__ coeff, int64_t n_terms,
                                                               const int32_t* __restrict__ term_sums, int shots,
                                                               double* __restrict__ term_values, double* __restrict__ values,
                                                               double* __restrict__ variance) {
  const int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (c >= n_circuits) return;
  const int64_t tb = frm_clamp(term_ptr[c], (int64_t)0, n_terms), te = frm_clamp(term_ptr[c + 1], tb, n_terms);
  sample_value_variance(coeff, tb, te, values[c], variance[c], [&](int64_t t) {
    const double tv = (double)term_sums[t] / (double)shots;
    term_values[t] = tv;
    return tv;
  });
}

}  // namespace
}  // namespace mlqem

using namespace mlqem;

extern "C" int mlqem_clifford_sample_f64(int64_t n_circuits, const int32_t* n_qubits, const int64_t* op_ptr, const mlqem_clifford_op* ops,
                                         int64_t n_ops, const uint64_t* thresh, int64_t n_thresh, const int64_t* ro_ptr,
                                         const int64_t* group_ptr, const int32_t* group_circ, const int32_t* group_mask,
                                         int64_t n_groups, const int32_t* ids, int64_t n_reg, int64_t n_lds, const uint32_t* masks,
                                         int64_t n_masks, const int64_t* term_ptr, const double* coeff, const int32_t* term_mask,
                                         int64_t n_terms, const int64_t* gterm_ptr, const int32_t* gterm, int64_t n_gterm,
                                         const int64_t* run_keys, int64_t shots, uint64_t seed, int32_t max_qubits,
                                         const int64_t* row_ptr, uint32_t* rows, int64_t n_rows, const int64_t* ref_ptr,
                                         uint32_t* reference, int64_t n_ref, uint32_t* bits, int64_t n_bits, int32_t* term_sums,
                                         double* term_values, double* values, double* variance, mlqem_stream_t stream) {
  begin_launches();
  if (n_circuits < 0 || n_ops < 0 || n_groups < 0 || n_reg < 0 || n_lds < 0 || n_terms < 0 || n_gterm < 0 || n_rows < 0 || n_ref < 0 ||
      n_bits < 0 || n_thresh < kClfPad || n_masks < kClfPad || shots < 1 || shots > MLQEM_SIM_MAX_SHOTS || max_qubits < 1 ||
      max_qubits > MLQEM_CLIFFORD_MAX_QUBITS || n_reg + n_lds != n_groups)
    return MLQEM_ERR_BAD_ARG;
  const int64_t nblk = ceil_div(shots, (int64_t)kBlock);
  if (n_circuits > 0x7FFFFFFFll || n_groups > 0x7FFFFFFFll || n_thresh > 0x7FFFFFFFll || n_masks > 0x7FFFFFFFll ||
      n_terms > 0x7FFFFFFFll || n_gterm > 0x7FFFFFFFll || n_groups * nblk > 0x7FFFFFFFll)
    return MLQEM_ERR_UNSUPPORTED;
  if (n_circuits == 0) return MLQEM_OK;
  if (n_groups < 1 || n_rows < 1 || n_ref < 1) return MLQEM_ERR_BAD_ARG;   // every circuit has a group
  if (!n_qubits || !op_ptr || !thresh || !ro_ptr || !group_ptr || !group_circ || !group_mask || !ids || !masks || !term_ptr ||
      !gterm_ptr || !run_keys || !row_ptr || !rows || !ref_ptr || !reference || !values || !variance || (n_ops > 0 && !ops) ||
      (n_terms > 0 && (!coeff || !term_mask || !term_sums || !term_values)) || (n_gterm > 0 && (!gterm || n_terms == 0)))
    return MLQEM_ERR_BAD_ARG;
  if (!aligned_to(ops, 16) || !aligned_to(thresh, 8)) return MLQEM_ERR_BAD_ARG;
  if (!ensure_dynamic_lds(reference_kernel, kFrmRefMaxLds)) return MLQEM_ERR_LAUNCH;
  const clf_i4* oi = reinterpret_cast<const clf_i4*>(ops);
  const hipStream_t st = as_stream(stream);
  const int B = (int)n_circuits, G = (int)n_groups, mq = (int)max_qubits;
  if (n_terms > 0 && hipMemsetAsync(term_sums, 0, (size_t)n_terms * sizeof(int32_t), st) != hipSuccess) return MLQEM_ERR_LAUNCH;
  if (n_reg > 0)
    hipLaunchKernelGGL((pullback_kernel<true>), dim3((unsigned)n_reg, 1), dim3(kBlock), 0, st, B, n_qubits, op_ptr, oi, n_ops,
                       group_circ, group_mask, G, ids, masks, n_masks, row_ptr, rows, n_rows, mq);
  if (n_lds > 0)
    hipLaunchKernelGGL((pullback_kernel<false>), dim3((unsigned)n_lds, (unsigned)ceil_div((int64_t)mq, (int64_t)kBlock)), dim3(kBlock),
                       0, st, B, n_qubits, op_ptr, oi, n_ops, group_circ, group_mask, G, ids + n_reg, masks, n_masks, row_ptr, rows,
                       n_rows, mq);
  const int wm = (mq + 31) >> 5;
  const size_t ref_lds = (size_t)(32 * wm + mq * (2 * wm + 1)) * 4;
  hipLaunchKernelGGL(reference_kernel, dim3((unsigned)n_groups), dim3(kWave), ref_lds, st, B, n_qubits, group_circ, G, row_ptr, rows,
                     n_rows, ref_ptr, reference, n_ref, mq);
  const uint32_t seed_lo = (uint32_t)seed, seed_hi = (uint32_t)(seed >> 32);
  const int64_t nb = bits ? n_bits : 0;
  if (n_reg > 0)
    hipLaunchKernelGGL((frames_kernel<true>), dim3((unsigned)(n_reg * nblk)), dim3(kBlock), 0, st, B, n_qubits, op_ptr, oi, n_ops,
                       thresh, n_thresh, ro_ptr, group_ptr, group_circ, group_mask, G, ids, masks, n_masks, gterm_ptr, gterm, n_gterm,
                       term_mask, n_terms, run_keys, (int)shots, seed_lo, seed_hi, mq, (int)nblk, ref_ptr, reference, n_ref, bits, nb,
                       term_sums);
  if (n_lds > 0)
    hipLaunchKernelGGL((frames_kernel<false>), dim3((unsigned)(n_lds * nblk)), dim3(kBlock), 0, st, B, n_qubits, op_ptr, oi, n_ops,
                       thresh, n_thresh, ro_ptr, group_ptr, group_circ, group_mask, G, ids + n_reg, masks, n_masks, gterm_ptr, gterm,
                       n_gterm, term_mask, n_terms, run_keys, (int)shots, seed_lo, seed_hi, mq, (int)nblk, ref_ptr, reference, n_ref,
                       bits, nb, term_sums);
  hipLaunchKernelGGL(frames_finish_kernel, dim3((unsigned)ceil_div(n_circuits, (int64_t)kBlock)), dim3(kBlock), 0, st, n_circuits,
                     term_ptr, coeff, n_terms, term_sums, (int)shots, term_values, values, variance);
  return launch_status();
}
