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
// FOLD = true (mlqem_clifford_run_folded_f64, zero-noise extrapolation): a thread per (noise factor, unit) walks the SCHEDULE of
// its (factor, circuit) run, entries (k << 1) | dagger naming the circuit's records; a daggered C1 / C2 record applies the inverse
// table, found in the record as it is read (the table is a signed permutation: the entry that holds the current letters).  Three
// dependent loads per entry (entry -> record -> pool value), the four of a chunk in flight together at each level.
// combine_kernel: a wave per (circuit, noise factor).  Lanes stride over the circuit's terms, each adding weight * unit in `comb` order; after a
// barrier lane 0 adds coeff * term in term order.  Products and sums are separately rounded (no contraction), so the host can repeat
// them bit for bit.  No atomics, no workspace, nothing read back.
#include "clifford_words.hpp"

namespace mlqem {
namespace {

// ClfWords (the lane's Pauli words), clf_find_c1 / clf_find_c2 and clf_step live in clifford_words.hpp, which clifford_frames.hip
// shares.
// FOLD = false walks the circuit's records from the last to the first (mlqem_clifford_run_f64); FOLD = true walks the schedule of
// run (f, circuit of the unit) from its last entry to its first (mlqem_clifford_run_folded_f64): slot = f * n_here + the unit's
// place in this part, so the units of one circuit stay adjacent and the lanes of a wave still mostly load the same bytes.
template <bool REG, bool FOLD>
__global__ __launch_bounds__(kBlock) void walk_kernel(int n_circuits, const int32_t* __restrict__ n_qubits,
                                                      const int64_t* __restrict__ op_ptr, const clf_i4* __restrict__ ops, int64_t n_ops,
                                                      const double* __restrict__ pool, int64_t n_pool,
                                                      const clf_i4* __restrict__ units, int64_t first_unit, int64_t n_here,
                                                      const uint32_t* __restrict__ masks, int64_t n_masks,
                                                      double* __restrict__ unit_ideal, double* __restrict__ unit_noisy,
                                                      int n_factors, int64_t n_units, const int64_t* __restrict__ sched_ptr,
                                                      const int32_t* __restrict__ sched, int64_t n_sched) {
  constexpr int WCAP = REG ? kClfRegWords : kClfMaxWords;
  __shared__ uint32_t lds[REG ? 1 : 2 * kClfMaxWords * kBlock];
  const int64_t slot = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t n_slots = FOLD ? (int64_t)n_factors * n_here : n_here;
  const bool live = slot < n_slots;
  const int64_t at = live ? slot : n_slots - 1;   // n_here >= 1 (and n_factors >= 1): the launcher launches nothing otherwise
  const int64_t fac = FOLD ? at / n_here : 0;
  const int64_t u = first_unit + (FOLD ? at - fac * n_here : at);
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
  if constexpr (!FOLD) {
    // kClfChunk records at a time: their loads, then the loads of the pool entries they name, are in flight together, so a lane
    // waits for memory twice per chunk and not twice per record (the walk itself is a serial chain through the lane's words)
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
        clf_step<REG, FOLD>(p, sign, factor, n, r[j], keep[j], false);
      }
    }
  } else {
    // run r = f * B + c; a circuit without records skips its entries (so every record index below is inside [ob, oe - 1])
    const int64_t n_runs = (int64_t)n_factors * n_circuits;
    const int64_t run = min(max(fac * n_circuits + c, (int64_t)0), n_runs - 1);
    const int64_t sb = min(max(sched_ptr[run], (int64_t)0), n_sched);
    const int64_t se = oe > ob ? min(max(sched_ptr[run + 1], sb), n_sched) : sb;
    const int64_t last = oe - ob - 1;
    // three dependent loads per entry (entry -> record -> pool value); the four of a chunk are in flight together at each level
    for (int64_t i = se - 1; i >= sb; i -= kClfChunk) {
      int32_t e[kClfChunk];
      clf_i4 r[kClfChunk];
      double keep[kClfChunk];
#pragma unroll
      for (int j = 0; j < kClfChunk; ++j) e[j] = sched[max(i - j, sb)];
#pragma unroll
      for (int j = 0; j < kClfChunk; ++j) r[j] = ops[ob + min(max((int64_t)(e[j] >> 1), (int64_t)0), last)];
#pragma unroll
      for (int j = 0; j < kClfChunk; ++j) keep[j] = pool[min(max((int64_t)r[j].y, (int64_t)0), n_pool - 1)];
#pragma unroll
      for (int j = 0; j < kClfChunk; ++j) {
        if (i - j < sb) break;
        clf_step<REG, FOLD>(p, sign, factor, n, r[j], keep[j], (e[j] & 1) != 0);
      }
    }
  }
  const double ideal = p.any_x(W) ? 0.0 : (sign & 1u) ? -1.0 : 1.0;
  if (live) {
    const int64_t out = FOLD ? fac * n_units + u : u;
    unit_ideal[out] = ideal;
    unit_noisy[out] = ideal * factor;
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
  const int64_t f = blockIdx.y;   // the noise factor: row f of every [F][.] buffer (0 for the unfolded run)
  unit_ideal += f * n_units;
  unit_noisy += f * n_units;
  ideal_terms += f * n_terms;
  noisy_terms += f * n_terms;
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
    ideal_values[f * n_circuits + c] = vi;
    noisy_values[f * n_circuits + c] = vn;
  }
}

}  // namespace
}  // namespace mlqem

using namespace mlqem;

// The two entry points share their checks and launches: `sched_ptr == nullptr` is the plain run (n_factors = 1).
static int clifford_run_impl(bool fold, int64_t n_circuits, int64_t n_factors, const int32_t* n_qubits, const int64_t* op_ptr,
                             const mlqem_clifford_op* ops, int64_t n_ops, const double* pool, int64_t n_pool,
                             const mlqem_clifford_unit* units, int64_t n_reg, int64_t n_lds, const uint32_t* masks, int64_t n_masks,
                             const int64_t* term_ptr, const double* coeff, int64_t n_terms, const int64_t* comb_ptr,
                             const int32_t* comb_unit, const double* comb_weight, int64_t n_comb, const int64_t* sched_ptr,
                             const int32_t* sched, int64_t n_sched, double* unit_ideal, double* unit_noisy, double* ideal_terms,
                             double* noisy_terms, double* ideal_values, double* noisy_values, mlqem_stream_t stream) {
  static_assert(sizeof(mlqem_clifford_op) == 16 && sizeof(mlqem_clifford_unit) == 16, "one 16-byte load per record");
  begin_launches();
  if (n_circuits < 0 || n_ops < 0 || n_terms < 0 || n_reg < 0 || n_lds < 0 || n_comb < 0 || n_pool < kClfPad || n_masks < kClfPad ||
      n_factors < 1 || n_sched < 0)
    return MLQEM_ERR_BAD_ARG;
  const int64_t n_units = n_reg + n_lds;
  if (n_circuits > 0x7FFFFFFFll || n_units > 0x7FFFFFFFll || n_pool > 0x7FFFFFFFll || n_masks > 0x7FFFFFFFll ||
      n_factors > 0x7FFFFFFFll || n_sched > 0x7FFFFFFFll)
    return MLQEM_ERR_UNSUPPORTED;
  // grid.y carries the factor in the combine; F * B and F * units stay below 2^31 so that a block count fits a grid dimension
  if (n_factors > 65535 || n_factors * n_circuits > 0x7FFFFFFFll || n_factors * n_units > 0x7FFFFFFFll) return MLQEM_ERR_UNSUPPORTED;
  if (n_circuits == 0) return MLQEM_OK;
  if (!n_qubits || !op_ptr || !pool || !masks || !term_ptr || !ideal_values || !noisy_values || (n_ops > 0 && !ops) ||
      (n_units > 0 && (!units || !unit_ideal || !unit_noisy)) ||
      (n_terms > 0 && (!coeff || !comb_ptr || !ideal_terms || !noisy_terms)) || (n_comb > 0 && (!comb_unit || !comb_weight)))
    return MLQEM_ERR_BAD_ARG;
  if (fold && (!sched_ptr || (n_sched > 0 && !sched))) return MLQEM_ERR_BAD_ARG;
  if (n_comb > 0 && n_units == 0) return MLQEM_ERR_BAD_ARG;   // a combine entry needs a unit to name
  if (!aligned_to(ops, 16) || !aligned_to(units, 16)) return MLQEM_ERR_BAD_ARG;
  const clf_i4* oi = reinterpret_cast<const clf_i4*>(ops);
  const clf_i4* ui = reinterpret_cast<const clf_i4*>(units);
  const int F = (int)n_factors;
  if (n_reg > 0) {
    const dim3 grid((unsigned)ceil_div(n_factors * n_reg, (int64_t)kBlock));
    if (fold)
      hipLaunchKernelGGL((walk_kernel<true, true>), grid, dim3(kBlock), 0, as_stream(stream), (int)n_circuits, n_qubits, op_ptr, oi,
                         n_ops, pool, n_pool, ui, (int64_t)0, n_reg, masks, n_masks, unit_ideal, unit_noisy, F, n_units, sched_ptr,
                         sched, n_sched);
    else
      hipLaunchKernelGGL((walk_kernel<true, false>), grid, dim3(kBlock), 0, as_stream(stream), (int)n_circuits, n_qubits, op_ptr, oi,
                         n_ops, pool, n_pool, ui, (int64_t)0, n_reg, masks, n_masks, unit_ideal, unit_noisy, F, n_units, sched_ptr,
                         sched, n_sched);
  }
  if (n_lds > 0) {
    const dim3 grid((unsigned)ceil_div(n_factors * n_lds, (int64_t)kBlock));
    if (fold)
      hipLaunchKernelGGL((walk_kernel<false, true>), grid, dim3(kBlock), 0, as_stream(stream), (int)n_circuits, n_qubits, op_ptr, oi,
                         n_ops, pool, n_pool, ui, n_reg, n_lds, masks, n_masks, unit_ideal, unit_noisy, F, n_units, sched_ptr, sched,
                         n_sched);
    else
      hipLaunchKernelGGL((walk_kernel<false, false>), grid, dim3(kBlock), 0, as_stream(stream), (int)n_circuits, n_qubits, op_ptr, oi,
                         n_ops, pool, n_pool, ui, n_reg, n_lds, masks, n_masks, unit_ideal, unit_noisy, F, n_units, sched_ptr, sched,
                         n_sched);
  }
  hipLaunchKernelGGL(combine_kernel, dim3((unsigned)n_circuits, (unsigned)n_factors), dim3(kWave), 0, as_stream(stream),
                     (int)n_circuits, term_ptr, coeff, n_terms, comb_ptr, comb_unit, comb_weight, n_comb, unit_ideal, unit_noisy,
                     n_units, ideal_terms, noisy_terms, ideal_values, noisy_values);
  return launch_status();
}

extern "C" int mlqem_clifford_run_f64(int64_t n_circuits, const int32_t* n_qubits, const int64_t* op_ptr, const mlqem_clifford_op* ops,
                                      int64_t n_ops, const double* pool, int64_t n_pool, const mlqem_clifford_unit* units,
                                      int64_t n_reg, int64_t n_lds, const uint32_t* masks, int64_t n_masks, const int64_t* term_ptr,
                                      const double* coeff, int64_t n_terms, const int64_t* comb_ptr, const int32_t* comb_unit,
                                      const double* comb_weight, int64_t n_comb, double* unit_ideal, double* unit_noisy,
                                      double* ideal_terms, double* noisy_terms, double* ideal_values, double* noisy_values,
                                      mlqem_stream_t stream) {
  return clifford_run_impl(false, n_circuits, 1, n_qubits, op_ptr, ops, n_ops, pool, n_pool, units, n_reg, n_lds, masks, n_masks,
                           term_ptr, coeff, n_terms, comb_ptr, comb_unit, comb_weight, n_comb, nullptr, nullptr, 0, unit_ideal,
                           unit_noisy, ideal_terms, noisy_terms, ideal_values, noisy_values, stream);
}

extern "C" int mlqem_clifford_run_folded_f64(int64_t n_circuits, int64_t n_factors, const int32_t* n_qubits, const int64_t* op_ptr,
                                             const mlqem_clifford_op* ops, int64_t n_ops, const double* pool, int64_t n_pool,
                                             const mlqem_clifford_unit* units, int64_t n_reg, int64_t n_lds, const uint32_t* masks,
                                             int64_t n_masks, const int64_t* term_ptr, const double* coeff, int64_t n_terms,
                                             const int64_t* comb_ptr, const int32_t* comb_unit, const double* comb_weight,
                                             int64_t n_comb, const int64_t* sched_ptr, const int32_t* sched, int64_t n_sched,
                                             double* unit_ideal, double* unit_noisy, double* ideal_terms, double* noisy_terms,
                                             double* ideal_values, double* noisy_values, mlqem_stream_t stream) {
  return clifford_run_impl(true, n_circuits, n_factors, n_qubits, op_ptr, ops, n_ops, pool, n_pool, units, n_reg, n_lds, masks,
                           n_masks, term_ptr, coeff, n_terms, comb_ptr, comb_unit, comb_weight, n_comb, sched_ptr, sched, n_sched,
                           unit_ideal, unit_noisy, ideal_terms, noisy_terms, ideal_values, noisy_values, stream);
}
