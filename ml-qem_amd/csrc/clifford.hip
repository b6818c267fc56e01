// Clifford circuits of any width up to 512 qubits, a batch per call (mlqem_clifford_run_f64): a Pauli observable is carried BACKWARDS
// through the circuit's records as a Pauli (Heisenberg picture), so a (circuit, Pauli) unit costs O(records) bit operations and a
// few bytes of state, whatever the width.  include/mlqem_hip.h has the contract and the record layouts.
//
// walk_kernel: one thread per unit.  The lane keeps the Pauli as W = ceil(n / 32) x words and W z words (letter of qubit q: bit q of
// x | bit q of z << 1, so I = 0, X = 1, Z = 2, Y = 3, Y being the Hermitian letter), a sign bit and `factor`, the product of the
// keep = 1 - lambda of every depolarising record that met a non-identity letter.  Records are walked from the circuit's last to its
// first, four per wait on memory; units are ordered by circuit, so the lanes of a wave mostly load the same 16 bytes.  Two
// instantiations:
//   REG = true    W <= 4 (n <= 128): the eight words are registers; a word is picked and updated with compile-time selects (an array
//                 indexed with a run-time word number would go to scratch);
//   REG = false   W <= 16 (n <= 512): the words live in LDS at word * 256 + lane (stride 1 across lanes: no bank conflict, and a lane
//                 only ever touches its own column, so there is no barrier), 32 KB per workgroup.
// Loads are unconditional on clamped indices and only the two final stores are predicated; a malformed record computes garbage and
// reads nothing out of range.
// combine_kernel: a wave per circuit.  Lanes stride over the circuit's terms, each adding weight * unit in `comb` order; after a
// barrier lane 0 adds coeff * term in term order.  Products and sums are separately rounded (no contraction), so the host can repeat
// them bit for bit.  No atomics, no workspace, nothing read back.
#include "common.hpp"

namespace mlqem {
namespace {

constexpr int kClfRegWords = MLQEM_CLIFFORD_REG_QUBITS / 32;   // 4
constexpr int kClfMaxWords = MLQEM_CLIFFORD_MAX_QUBITS / 32;   // 16
constexpr int kClfPad = MLQEM_CLIFFORD_PAD;
constexpr int kClfChunk = 4;   // records a lane loads ahead of walking them

typedef int clf_i4 __attribute__((ext_vector_type(4)));

template <bool REG> struct ClfWords;

template <> struct ClfWords<true> {
  uint32_t x0, x1, x2, x3, z0, z1, z2, z3;
  __device__ __forceinline__ ClfWords(uint32_t*, int) {}
  __device__ __forceinline__ void init(int w, uint32_t x, uint32_t z) {
    if (w == 0) { x0 = x; z0 = z; }
    if (w == 1) { x1 = x; z1 = z; }
    if (w == 2) { x2 = x; z2 = z; }
    if (w == 3) { x3 = x; z3 = z; }
  }
  __device__ __forceinline__ uint32_t getx(int w) const { return w == 0 ? x0 : w == 1 ? x1 : w == 2 ? x2 : x3; }
  __device__ __forceinline__ uint32_t getz(int w) const { return w == 0 ? z0 : w == 1 ? z1 : w == 2 ? z2 : z3; }
  __device__ __forceinline__ void flip(int w, uint32_t dx, uint32_t dz) {
    x0 ^= w == 0 ? dx : 0u; x1 ^= w == 1 ? dx : 0u; x2 ^= w == 2 ? dx : 0u; x3 ^= w == 3 ? dx : 0u;
    z0 ^= w == 0 ? dz : 0u; z1 ^= w == 1 ? dz : 0u; z2 ^= w == 2 ? dz : 0u; z3 ^= w == 3 ? dz : 0u;
  }
  __device__ __forceinline__ uint32_t any_x(int) const { return x0 | x1 | x2 | x3; }
};

template <> struct ClfWords<false> {
  uint32_t* col;   // this lane's column: x word w at col[w * kBlock], z word w at col[(kClfMaxWords + w) * kBlock]
  __device__ __forceinline__ ClfWords(uint32_t* lds, int tid) : col(lds + tid) {}
  __device__ __forceinline__ void init(int w, uint32_t x, uint32_t z) {
    col[w * kBlock] = x;
    col[(kClfMaxWords + w) * kBlock] = z;
  }
  __device__ __forceinline__ uint32_t getx(int w) const { return col[w * kBlock]; }
  __device__ __forceinline__ uint32_t getz(int w) const { return col[(kClfMaxWords + w) * kBlock]; }
  __device__ __forceinline__ void flip(int w, uint32_t dx, uint32_t dz) {
    col[w * kBlock] ^= dx;
    col[(kClfMaxWords + w) * kBlock] ^= dz;
  }
  __device__ __forceinline__ uint32_t any_x(int W) const {
    uint32_t acc = 0;
    for (int w = 0; w < W; ++w) acc |= col[w * kBlock];
    return acc;
  }
};

template <bool REG>
__global__ __launch_bounds__(kBlock) void walk_kernel(int n_circuits, const int32_t* __restrict__ n_qubits,
                                                      const int64_t* __restrict__ op_ptr, const clf_i4* __restrict__ ops, int64_t n_ops,
                                                      const double* __restrict__ pool, int64_t n_pool,
                                                      const clf_i4* __restrict__ units, int64_t first_unit, int64_t n_here,
                                                      const uint32_t* __restrict__ masks, int64_t n_masks,
                                                      double* __restrict__ unit_ideal, double* __restrict__ unit_noisy) {
  constexpr int WCAP = REG ? kClfRegWords : kClfMaxWords;
  __shared__ uint32_t lds[REG ? 1 : 2 * kClfMaxWords * kBlock];
  const int64_t slot = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const bool live = slot < n_here;
  const int64_t u = first_unit + (live ? slot : n_here - 1);   // n_here >= 1: the launcher launches nothing otherwise
  const clf_i4 unit = units[u];
  const int c = min(max(unit.x, 0), n_circuits - 1);
  const int n = min(max(n_qubits[c], 1), 32 * WCAP);
  const int W = (n + 31) >> 5;
  ClfWords<REG> p(lds, threadIdx.x);
  const auto load_word = [&](int w) {   // words past W are zero (REG keeps all four)
    const int64_t ix = min(max((int64_t)unit.y + w, (int64_t)0), n_masks - 1);
    const int64_t iz = min(max((int64_t)unit.y + W + w, (int64_t)0), n_masks - 1);
    const uint32_t x = masks[ix], z = masks[iz];
    p.init(w, w < W ? x : 0u, w < W ? z : 0u);
  };
  if constexpr (REG) {
#pragma unroll
    for (int w = 0; w < WCAP; ++w) load_word(w);
  } else {
    for (int w = 0; w < W; ++w) load_word(w);
  }
  const int64_t ob = min(max(op_ptr[c], (int64_t)0), n_ops), oe = min(max(op_ptr[c + 1], ob), n_ops);
  uint32_t sign = 0;
  double factor = 1.0;
  // kClfChunk records at a time: their loads, then the loads of the pool entries they name, are in flight together, so a lane waits
  // for memory twice per chunk and not twice per record (the walk itself is a serial chain through the lane's words)
  for (int64_t k = oe - 1; k >= ob; k -= kClfChunk) {
    clf_i4 r[kClfChunk];
    double keep[kClfChunk];
#pragma unroll
    for (int j = 0; j < kClfChunk; ++j) r[j] = ops[max(k - j, ob)];
#pragma unroll
    for (int j = 0; j < kClfChunk; ++j) keep[j] = pool[min(max((int64_t)r[j].y, (int64_t)0), n_pool - 1)];
#pragma unroll
    for (int j = 0; j < kClfChunk; ++j) {
      if (k - j < ob) break;
      const int kind = r[j].x & 15;
      const int q0 = min((r[j].x >> 4) & 1023, n - 1), q1 = min((r[j].x >> 14) & 1023, n - 1);
      const int w0 = q0 >> 5, b0 = q0 & 31, w1 = q1 >> 5, b1 = q1 & 31;
      const uint32_t a = ((p.getx(w0) >> b0) & 1u) | (((p.getz(w0) >> b0) & 1u) << 1);
      const bool two = kind == MLQEM_CLIFFORD_OP_C2 || kind == MLQEM_CLIFFORD_OP_DEPOL2;
      const uint32_t b = two ? ((p.getx(w1) >> b1) & 1u) | (((p.getz(w1) >> b1) & 1u) << 1) : 0u;
      const uint32_t pq = a | (b << 2);
      if (kind == MLQEM_CLIFFORD_OP_C1) {
        const uint32_t img = a ? ((uint32_t)r[j].y >> (3 * (a ? a - 1 : 0u))) & 7u : 0u;   // letter | sign << 2; I stays I
        const uint32_t d = (img & 3u) ^ a;
        sign ^= img >> 2;
        p.flip(w0, (d & 1u) << b0, (d >> 1) << b0);
      } else if (kind == MLQEM_CLIFFORD_OP_C2) {
        const uint32_t e = pq ? pq - 1 : 0u;
        const uint64_t tab = (uint64_t)(uint32_t)r[j].y | ((uint64_t)(uint32_t)r[j].z << 32);
        const uint32_t img = pq ? (uint32_t)(tab >> (4 * e)) & 15u : 0u;
        const uint32_t d = img ^ pq;
        sign ^= pq ? ((uint32_t)r[j].w >> e) & 1u : 0u;
        p.flip(w0, (d & 1u) << b0, ((d >> 1) & 1u) << b0);
        p.flip(w1, ((d >> 2) & 1u) << b1, ((d >> 3) & 1u) << b1);
      } else if (kind == MLQEM_CLIFFORD_OP_DEPOL1 || kind == MLQEM_CLIFFORD_OP_DEPOL2) {
        factor = pq ? factor * keep[j] : factor;
      }
    }
  }
  const double ideal = p.any_x(W) ? 0.0 : (sign & 1u) ? -1.0 : 1.0;
  if (live) {
    unit_ideal[u] = ideal;
    unit_noisy[u] = ideal * factor;
  }
}

__global__ __launch_bounds__(kWave) void combine_kernel(int n_circuits, const int64_t* __restrict__ term_ptr,
                                                        const double* __restrict__ coeff, int64_t n_terms,
                                                        const int64_t* __restrict__ comb_ptr, const int32_t* __restrict__ comb_unit,
                                                        const double* __restrict__ comb_weight, int64_t n_comb,
                                                        const double* __restrict__ unit_ideal, const double* __restrict__ unit_noisy,
                                                        int64_t n_units, double* __restrict__ ideal_terms,
                                                        double* __restrict__ noisy_terms, double* __restrict__ ideal_values,
                                                        double* __restrict__ noisy_values) {
#pragma clang fp contract(off)
  const int c = blockIdx.x;
  const int64_t tb = min(max(term_ptr[c], (int64_t)0), n_terms), te = min(max(term_ptr[c + 1], tb), n_terms);
  for (int64_t t = tb + threadIdx.x; t < te; t += kWave) {
    const int64_t jb = min(max(comb_ptr[t], (int64_t)0), n_comb), je = min(max(comb_ptr[t + 1], jb), n_comb);
    double si = 0.0, sn = 0.0;
    for (int64_t j = jb; j < je; ++j) {
      const int64_t uu = min(max((int64_t)comb_unit[j], (int64_t)0), n_units - 1);
      si = si + comb_weight[2 * j] * unit_ideal[uu];
      sn = sn + comb_weight[2 * j + 1] * unit_noisy[uu];
    }
    ideal_terms[t] = si;
    noisy_terms[t] = sn;
  }
  __threadfence_block();
  __syncthreads();
  if (threadIdx.x == 0) {
    double vi = 0.0, vn = 0.0;
    for (int64_t t = tb; t < te; ++t) {
      vi = vi + coeff[t] * ideal_terms[t];
      vn = vn + coeff[t] * noisy_terms[t];
    }
    ideal_values[c] = vi;
    noisy_values[c] = vn;
  }
}

}  // namespace
}  // namespace mlqem

using namespace mlqem;

extern "C" int mlqem_clifford_run_f64(int64_t n_circuits, const int32_t* n_qubits, const int64_t* op_ptr, const mlqem_clifford_op* ops,
                                      int64_t n_ops, const double* pool, int64_t n_pool, const mlqem_clifford_unit* units,
                                      int64_t n_reg, int64_t n_lds, const uint32_t* masks, int64_t n_masks, const int64_t* term_ptr,
                                      const double* coeff, int64_t n_terms, const int64_t* comb_ptr, const int32_t* comb_unit,
                                      const double* comb_weight, int64_t n_comb, double* unit_ideal, double* unit_noisy,
                                      double* ideal_terms, double* noisy_terms, double* ideal_values, double* noisy_values,
                                      mlqem_stream_t stream) {
  static_assert(sizeof(mlqem_clifford_op) == 16 && sizeof(mlqem_clifford_unit) == 16, "one 16-byte load per record");
  begin_launches();
  if (n_circuits < 0 || n_ops < 0 || n_terms < 0 || n_reg < 0 || n_lds < 0 || n_comb < 0 || n_pool < kClfPad || n_masks < kClfPad)
    return MLQEM_ERR_BAD_ARG;
  const int64_t n_units = n_reg + n_lds;
  if (n_circuits > 0x7FFFFFFFll || n_units > 0x7FFFFFFFll || n_pool > 0x7FFFFFFFll || n_masks > 0x7FFFFFFFll)
    return MLQEM_ERR_UNSUPPORTED;
  if (n_circuits == 0) return MLQEM_OK;
  if (!n_qubits || !op_ptr || !pool || !masks || !term_ptr || !ideal_values || !noisy_values || (n_ops > 0 && !ops) ||
      (n_units > 0 && (!units || !unit_ideal || !unit_noisy)) ||
      (n_terms > 0 && (!coeff || !comb_ptr || !ideal_terms || !noisy_terms)) || (n_comb > 0 && (!comb_unit || !comb_weight)))
    return MLQEM_ERR_BAD_ARG;
  if (n_comb > 0 && n_units == 0) return MLQEM_ERR_BAD_ARG;   // a combine entry needs a unit to name
  if (!aligned_to(ops, 16) || !aligned_to(units, 16)) return MLQEM_ERR_BAD_ARG;
  const clf_i4* oi = reinterpret_cast<const clf_i4*>(ops);
  const clf_i4* ui = reinterpret_cast<const clf_i4*>(units);
  if (n_reg > 0) {
    hipLaunchKernelGGL((walk_kernel<true>), dim3((unsigned)ceil_div(n_reg, (int64_t)kBlock)), dim3(kBlock), 0, as_stream(stream),
                       (int)n_circuits, n_qubits, op_ptr, oi, n_ops, pool, n_pool, ui, (int64_t)0, n_reg, masks, n_masks, unit_ideal,
                       unit_noisy);
  }
  if (n_lds > 0) {
    hipLaunchKernelGGL((walk_kernel<false>), dim3((unsigned)ceil_div(n_lds, (int64_t)kBlock)), dim3(kBlock), 0, as_stream(stream),
                       (int)n_circuits, n_qubits, op_ptr, oi, n_ops, pool, n_pool, ui, n_reg, n_lds, masks, n_masks, unit_ideal,
                       unit_noisy);
  }
  hipLaunchKernelGGL(combine_kernel, dim3((unsigned)n_circuits), dim3(kWave), 0, as_stream(stream), (int)n_circuits, term_ptr, coeff,
                     n_terms, comb_ptr, comb_unit, comb_weight, n_comb, unit_ideal, unit_noisy, n_units, ideal_terms, noisy_terms,
                     ideal_values, noisy_values);
  return launch_status();
}
