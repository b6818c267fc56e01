// Exact simulation of small circuits, a batch per launch (mlqem_sim_run_f64).  include/mlqem_hip.h has the contract and the record
// layouts.
//
// A circuit's state lives in LDS from |0..0> to its last expectation value and never touches global memory: complex float64
// amplitudes (re, im), either an n-qubit state vector (2^n entries) or an n-qubit density matrix kept as a 2n-bit vector (4^n entries,
// index = row | col << n).  One code path serves both: an op acts on `nbits` index bits, and in density mode a unitary U on qubit q is
// U on bit q followed by conj(U) on bit q + n, both from the one record.
//
// Two instantiations.  WG = false: a wave per circuit, four circuits per 256-thread workgroup, each wave owning a 4 KB slice (256
// amplitudes: 8-qubit vectors, 4-qubit density matrices).  The op loops of the four waves have different trip counts, so nothing in
// this variant is a workgroup barrier: a pass ends with a wavefront fence (LDS instructions of one wave execute in issue order; the
// fence only keeps the compiler from moving them).  WG = true: a workgroup per circuit, 2 048 amplitudes = 32 KB (11-qubit vectors,
// 5-qubit density matrices), a barrier after every pass.
//
// Passes.  Every op is one or two passes over the state; within a pass a thread owns disjoint entries, so passes need no ordering
// inside.  Loads are unconditional on clamped indices (every index is also masked to the amplitude count, so a malformed record
// computes garbage and faults nothing); only stores are predicated; trip counts depend on the amplitude count alone.
//   pair       a 2x2 matrix on bit b: entries (i, i | 1 << b)                        general one-qubit gates, readout (on the diagonal)
//   element    entry i times a factor of its own bits                                diagonal one-qubit gates, cz
//   gather     v = state[perm(i)], fence, state[i] = v                               cx, swap (row and column bits in one go)
//   quad       a 4x4 matrix on bits (a, b); the one-qubit depolarising map on (q, q + n)
//   hex        the two-qubit depolarising map on (a, b, a + n, b + n): 16 entries, closed form
//   noise      NOISE1 / NOISE2: the depolarising map followed by thermal relaxation of the gate's qubits, fused into one quad or
//              hex pass (a thread of noise2 takes one of the four 4-entry parts of a 4 x 4 block, so it holds what quad holds)
// Expectation values are reduced in a fixed order: lane-strided partial sums, a shuffle tree, then the waves in order through LDS.
//
// Folded runs (mlqem_sim_run_folded_f64) are two more instantiations of the same template: a run walks a schedule of
// (op index << 1) | dagger entries over its circuit's records instead of the records in order, and a daggered entry applies the
// record's inverse, formed by swapping and negating components as they are read (no arithmetic, so no new rounding).  The two
// instantiations mlqem_sim_run_f64 launches compile to the instructions they had before the schedules existed.
// mlqem_zne_combine_f64 is the weighted sum over the noise factors that extrapolates to zero noise.
//
// Measurement shots.  mlqem_sim_run_measured_f64 and its folded twin are four more instantiations (MEAS = true): a MEASURE record
// stores the state's outcome probabilities, one pass that leaves the state as it is and ends in the barrier every pass ends in (the
// next record writes the state).  mlqem_sim_sample_f64 is a kernel of its own (sample_kernel): it reads those probabilities from
// global memory, keeps a CDF and the counts in LDS -- not the 32 KB state -- and draws the shots with Philox4x32-10;
// sample_finish_kernel then adds up values and variances.
//
// SimCtx (the passes), the record decode, the norm pass, the switch over the record kinds, the state's types and Philox4x32-10
// live in sim_ctx.hpp: sim_bound.hip (runs of templates) and sim_traj.hip (quantum trajectories) call the same copy.
#include "sim_ctx.hpp"

namespace mlqem {
namespace {

// FOLD = false: circuit ids[slot] runs its ops in order (mlqem_sim_run_f64).  FOLD = true: ids holds RUN numbers r = f * B + c, and
// run r walks the schedule sched[sched_ptr[r] .. sched_ptr[r + 1]) of entries (k << 1) | dagger over circuit c's ops
// (mlqem_sim_run_folded_f64); its outputs go to row f.  The four waves of a workgroup of the wave variant then have trip counts that
// differ by the ratio of the noise factors: as before, nothing in that variant is a workgroup barrier.
//
// MEAS = true (mlqem_sim_run_measured_f64 and its folded twin): the program ends with a measurement tail of circ[c].w records
// (basis rotations / MEASURE / inverse rotations per group) after its readout ops, norm is taken before the readout ops AND the
// tail, and a MEASURE record stores the state's outcome probabilities -- one pass that reads the state and leaves it as it is.  The
// MEAS = false instantiations never read the five trailing arguments and compile to the instructions they had without them.
//
// Occupancy.  The wave variants are bound by registers (7 waves per SIMD plain, 6 folded), the workgroup variants by their 32 KB of
// LDS (4).  amdgpu_waves_per_eu states those figures, so that a pass added to the switch cannot lower them unnoticed: the compiler
// keeps each instantiation inside the register budget of its figure, and a pass that does not fit shows up as scratch.
template <bool WG, bool FOLD, bool MEAS = false>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(WG ? 4 : FOLD ? 6 : 7))) void sim_kernel(int B, const sim_i4* __restrict__ circ, const int64_t* __restrict__ op_ptr,
                                                     const sim_i4* __restrict__ ops, int64_t n_ops,
                                                     const double* __restrict__ params, int64_t n_params,
                                                     const int64_t* __restrict__ term_ptr, const sim_i4* __restrict__ terms,
                                                     const double* __restrict__ coeff, int64_t n_terms,
                                                     const int32_t* __restrict__ ids, int count, double* __restrict__ term_values,
                                                     double* __restrict__ values, double* __restrict__ norm, int n_runs,
                                                     const int64_t* __restrict__ sched_ptr, const int32_t* __restrict__ sched,
                                                     int64_t n_sched, const int64_t* __restrict__ group_ptr = nullptr,
                                                     const int64_t* __restrict__ prob_ptr = nullptr, int64_t n_groups = 0,
                                                     int64_t n_outcomes = 0, double* __restrict__ probs = nullptr) {
  __shared__ sim_c state[WG ? kSimMaxAmps : kBlock / kWave * kSimWaveAmps];
  __shared__ double red[8];
  SimCtx<WG> cx;
  const int slot = cx.begin(state, red);
  if (slot >= count) return;   // a wave of a partly filled workgroup: wave-uniform, and this variant has no workgroup barrier
  const int tid = cx.tid;
  const int run = FOLD ? __builtin_amdgcn_readfirstlane(min(max(ids[slot], 0), n_runs - 1)) : 0;
  const int c = FOLD ? run % B : __builtin_amdgcn_readfirstlane(min(max(ids[slot], 0), B - 1));
  const int row = FOLD ? run / B : 0;   // the noise factor's row of the outputs
  const sim_i4 info = circ[c];   // n_qubits, mode, trailing readout ops, reserved
  const bool density = info.y != 0;
  constexpr int kMaxBits = WG ? 11 : 8;
  const int n = __builtin_amdgcn_readfirstlane(min(max(info.x, 1), density ? kMaxBits / 2 : kMaxBits));
  const int nbits = density ? 2 * n : n, A = 1 << nbits;
  cx.nbits = nbits;
  cx.A = A;
  const int64_t ob = min(max(op_ptr[c], (int64_t)0), n_ops), oe = min(max(op_ptr[c + 1], ob), n_ops);
  const int n_op = __builtin_amdgcn_readfirstlane((int)min(oe - ob, (int64_t)0x7FFFFFFF));
  int64_t sb = 0;
  int n_step = n_op;   // steps this run takes: its ops, or the entries of its schedule
  if (FOLD) {
    sb = min(max(sched_ptr[run], (int64_t)0), n_sched);
    const int64_t se = min(max(sched_ptr[run + 1], sb), n_sched);
    n_step = __builtin_amdgcn_readfirstlane((int)min(se - sb, (int64_t)0x7FFFFFFF));
  }
  // steps before the readout ops (and the measurement tail after them): Tr rho is taken there
  const int n_main = n_step - min(min(max(info.z, 0), n_step) + (MEAS ? min(max(info.w, 0), n_step) : 0), n_step);

  for (int i = tid; i < A; i += cx.T) cx.st[i] = sim_c{i == 0 ? 1.0 : 0.0, 0.0};
  sim_sync<WG>();

  double nrm = 0.0;
  for (int k = 0; k <= n_step; ++k) {
    if (k == n_main) {   // <psi|psi> or Tr rho, before any readout op
      nrm = sim_norm(cx, n, density);
      if (WG) __syncthreads();   // red[0..3] is free again
    }
    if (k == n_step) break;
    int at = k;
    bool dg = false;   // apply the inverse of the record
    if (FOLD) {
      if (n_op == 0) continue;   // nothing an entry could name (wave-uniform; workgroup-uniform in the workgroup variant)
      const int entry = __builtin_amdgcn_readfirstlane(sched[sb + k]);
      at = min(max(entry >> 1, 0), n_op - 1);
      dg = entry & 1;
    }
    const sim_i4 op = ops[ob + at];   // kind, q0, q1, offset into params
    const SimRec rec = sim_decode(op, n, params, n_params);
    if constexpr (MEAS) {
      if (rec.kind == MLQEM_SIM_OP_MEASURE) {   // probabilities of the 2^n outcomes: |psi_j|^2, or Re rho_jj
        const int64_t g = __builtin_amdgcn_readfirstlane(op.w);   // the group's number in prob_ptr
        const int64_t gb = min(max(group_ptr[c], (int64_t)0), n_groups), ge = min(max(group_ptr[c + 1], gb), n_groups);
        const int64_t pb = prob_ptr[min(max(g, (int64_t)0), n_groups)];   // prob_ptr has n_groups + 1 entries
        const int M = 1 << n, mul = density ? M + 1 : 1;
        // a slot that is not one of this circuit's groups, or a range that leaves the pool: the pass runs and stores nothing
        const bool ok = g >= gb && g < ge && pb >= 0 && pb <= n_outcomes - M;
        double* out = probs + (FOLD ? (int64_t)row * n_outcomes : (int64_t)0) + (ok ? pb : (int64_t)0);
        for (int i0 = 0; i0 < M; i0 += cx.T) {
          const int i = i0 + tid;
          const sim_c v = cx.st[((i & (M - 1)) * mul) & (A - 1)];
          const double pr = density ? v.x : v.x * v.x + v.y * v.y;
          if (ok && i < M) out[i] = pr;
        }
        sim_sync<WG>();   // the next record may overwrite entries another wave of the workgroup has not read yet
        continue;
      }
    }
    sim_apply_fixed<FOLD>(cx, rec, n, density, dg);
  }

  // Pauli terms: P|j> = i^ny (-1)^popcount(j & z) |j ^ x>
  const int64_t tb = min(max(term_ptr[c], (int64_t)0), n_terms), te = min(max(term_ptr[c + 1], tb), n_terms);
  const int n_term = __builtin_amdgcn_readfirstlane((int)min(te - tb, (int64_t)0x7FFFFFFF));
  const int qmask = (1 << n) - 1, cnt = density ? 1 << n : A;
  double total = 0.0;
  for (int t = 0; t < n_term; ++t) {
    const sim_i4 term = terms[tb + t];   // xmask, zmask, number of Y factors, reserved
    const int xm = __builtin_amdgcn_readfirstlane(term.x & qmask), zm = __builtin_amdgcn_readfirstlane(term.y & qmask);
    const int ny = __builtin_amdgcn_readfirstlane(term.z & 3);
    double part = 0.0;
    for (int i0 = 0; i0 < cnt; i0 += cx.T) {
      const int i = i0 + tid, j = i & (cnt - 1);
      sim_c v;
      if (density) {
        v = cx.st[(j | ((j ^ xm) << n)) & (A - 1)];                  // rho[j, j ^ x]
      } else {
        const sim_c a = cx.st[(j ^ xm) & (A - 1)], b = cx.st[j];     // conj(psi[j ^ x]) psi[j]
        v = sim_c{a.x * b.x + a.y * b.y, a.x * b.y - a.y * b.x};
      }
      double re = ny == 0 ? v.x : ny == 1 ? -v.y : ny == 2 ? -v.x : v.y;   // Re(i^ny v)
      re = __popc(j & zm) & 1 ? -re : re;
      part = part + (i < cnt ? re : 0.0);
    }
    const double tv = cx.reduce(part, t & 1);
    if (tid == 0) {
      term_values[(FOLD ? (int64_t)row * n_terms : (int64_t)0) + tb + t] = tv;
      total = total + coeff[tb + t] * tv;
    }
  }
  if (tid == 0) {
    values[(FOLD ? (int64_t)row * B : (int64_t)0) + c] = total;
    norm[(FOLD ? (int64_t)row * B : (int64_t)0) + c] = nrm;
  }
}

// Zero-noise extrapolation of exact values is a weighted sum over the noise factors.  Thread i < n_terms writes mitigated term i;
// thread c < B forms the same sums again for its own terms (the same operations in the same order, so the same bits) and adds
// coeff * term in term order.  Every product is a fused multiply-add, written out so that the order is the source's.
__device__ __forceinline__ double zne_term(const double* __restrict__ tv, const double* __restrict__ w, int F, int64_t n_terms, int64_t t) {
  double acc = w[0] * tv[t];
  for (int f = 1; f < F; ++f) acc = __builtin_fma(w[f], tv[(int64_t)f * n_terms + t], acc);
  return acc;
}

__global__ __launch_bounds__(kBlock) void zne_combine_kernel(int F, const double* __restrict__ tv, const double* __restrict__ w,
                                                             const int64_t* __restrict__ term_ptr, const double* __restrict__ coeff,
                                                             int64_t n_terms, int64_t B, double* __restrict__ mterms,
                                                             double* __restrict__ mvalues) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < n_terms) mterms[i] = zne_term(tv, w, F, n_terms, i);
  if (i < B) {
    const int64_t tb = min(max(term_ptr[i], (int64_t)0), n_terms), te = min(max(term_ptr[i + 1], tb), n_terms);
    double total = 0.0;
    for (int64_t t = tb; t < te; ++t) total = __builtin_fma(coeff[t], zne_term(tv, w, F, n_terms, t), total);
    mvalues[i] = total;
  }
}

// Exponential extrapolation (mlqem_zne_combine_exp_f64): a straight line through (factor, ln|value|), evaluated at zero noise and
// exponentiated, where the term's values are all nonzero with one sign; 0 where they are all 0; the linear sum and a fallback flag
// anywhere else (a zero among nonzeros, mixed signs, a NaN).  The same thread layout and fixed order as zne_combine_kernel.
__device__ __forceinline__ double zne_exp_term(const double* __restrict__ tv, const double* __restrict__ w, int F, int64_t n_terms,
                                               int64_t t, int& fallback) {
  int pos = 0, neg = 0, zero = 0;
  for (int f = 0; f < F; ++f) {
    const double v = tv[(int64_t)f * n_terms + t];
    pos += v > 0.0;
    neg += v < 0.0;
    zero += v == 0.0;
  }
  fallback = 0;
  if (pos == F || neg == F) {
    double acc = w[0] * log(fabs(tv[t]));
    for (int f = 1; f < F; ++f) acc = __builtin_fma(w[f], log(fabs(tv[(int64_t)f * n_terms + t])), acc);
    const double m = exp(acc);
    return neg == F ? -m : m;
  }
  if (zero == F) return 0.0;
  fallback = 1;
  return zne_term(tv, w, F, n_terms, t);
}

__global__ __launch_bounds__(kBlock) void zne_combine_exp_kernel(int F, const double* __restrict__ tv, const double* __restrict__ w,
                                                                 const int64_t* __restrict__ term_ptr,
                                                                 const double* __restrict__ coeff, int64_t n_terms, int64_t B,
                                                                 double* __restrict__ mterms, double* __restrict__ mvalues,
                                                                 int32_t* __restrict__ fallback) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < n_terms) {
    int fb;
    mterms[i] = zne_exp_term(tv, w, F, n_terms, i, fb);
    fallback[i] = fb;
  }
  if (i < B) {
    const int64_t tb = min(max(term_ptr[i], (int64_t)0), n_terms), te = min(max(term_ptr[i + 1], tb), n_terms);
    double total = 0.0;
    for (int64_t t = tb; t < te; ++t) {
      int fb;
      total = __builtin_fma(coeff[t], zne_exp_term(tv, w, F, n_terms, t, fb), total);
    }
    mvalues[i] = total;
  }
}

// ---- measurement shots (mlqem_sim_sample_f64) ----------------------------------------------------------------------------------------
__device__ __forceinline__ int sim_wave_sum_int(int v) {
#pragma unroll
  for (int d = kWave / 2; d >= 1; d >>= 1) v = v + __shfl_down(v, d, kWave);
  return v;
}

// One (noise factor, group) pair per wave (WG = false: at most 256 outcomes, four pairs per workgroup, no workgroup barrier) or per
// workgroup (WG = true: up to 2 048).  The pair's CDF (float64) and counts (int32) live in LDS; the probabilities come from global
// memory, where a MEASURE record left them.  include/mlqem_hip.h states the CDF order and the sampling rule.
template <bool WG>
__global__ __launch_bounds__(kBlock) void sample_kernel(int B, int F, const sim_i4* __restrict__ circ, const int64_t* __restrict__ term_ptr,
                                                        const sim_i4* __restrict__ terms, int64_t n_terms,
                                                        const int64_t* __restrict__ group_ptr, const int32_t* __restrict__ term_group,
                                                        const int64_t* __restrict__ prob_ptr, const int32_t* __restrict__ group_circ,
                                                        int n_groups, int64_t n_outcomes, const double* __restrict__ probs,
                                                        const int64_t* __restrict__ run_keys, int shots, uint32_t seed_lo,
                                                        uint32_t seed_hi, const int32_t* __restrict__ units, int count,
                                                        int32_t* __restrict__ counts, double* __restrict__ term_values) {
  constexpr int T = WG ? kBlock : kWave;
  constexpr int kMaxM = WG ? kSimMaxAmps : kSimWaveAmps, kPer = WG ? 1 : kBlock / kWave;
  __shared__ double cdf_s[kPer * kMaxM];
  __shared__ double tot_s[kPer * (kMaxM / 8)];
  __shared__ int cnt_s[kPer * kMaxM];
  __shared__ int red_s[kBlock / kWave];
  const int slot = WG ? (int)blockIdx.x : __builtin_amdgcn_readfirstlane((int)blockIdx.x * (kBlock / kWave) + ((int)threadIdx.x >> 6));
  if (slot >= count) return;   // wave-uniform; the wave variant has no workgroup barrier
  const int tid = WG ? (int)threadIdx.x : (int)threadIdx.x & (kWave - 1);
  const int part = WG ? 0 : (int)threadIdx.x >> 6;
  double* cdf = cdf_s + part * kMaxM;
  double* tot = tot_s + part * (kMaxM / 8);
  int* cnt = cnt_s + part * kMaxM;

  const int rg = __builtin_amdgcn_readfirstlane(min(max(units[slot], 0), F * n_groups - 1));   // f * n_groups + g, F * n_groups < 2^31
  const int f = rg / n_groups, g = rg % n_groups;
  const int c = __builtin_amdgcn_readfirstlane(min(max(group_circ[g], 0), B - 1));
  const int n = __builtin_amdgcn_readfirstlane(min(max(circ[c].x, 1), WG ? 11 : 8));
  const int M = 1 << n;
  const int gl = g - (int)min(max(group_ptr[c], (int64_t)0), (int64_t)g);   // the group inside its circuit
  const int64_t pb = prob_ptr[g];
  const bool ok = pb >= 0 && pb <= n_outcomes - M;   // a range that leaves the pool: clamped loads, no store of counts
  const int64_t base = ok ? pb : 0;
  const double* p = probs + (int64_t)f * n_outcomes;

  // CDF: chunks of 8 consecutive outcomes (one chunk of M when M < 8), each summed left to right; the chunk totals prefix-summed
  // left to right; cdf[j] = (total of the chunks before j's) + (running sum inside j's chunk up to j)
  const int L = min(M, 8), C = M / L;   // C <= 256 = T (workgroup), C <= 32 (wave)
  double run[8];
  {
    const int k = min(tid, C - 1);
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const double v = p[min(base + k * L + min(i, L - 1), n_outcomes - 1)];
      acc = acc + (i < L && v > 0.0 ? v : 0.0);   // p_j <- max(p_j, 0); a NaN counts as 0
      run[i] = acc;
    }
    if (tid < C) tot[tid] = acc;
  }
  for (int j = tid; j < M; j += T) cnt[j] = 0;
  sim_sync<WG>();
  {
    double before = 0.0;
    for (int i = 0; i < C; ++i) {
      const double t = tot[i];
      before = i < tid ? before + t : before;
    }
    if (tid < C) {
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (i < L) cdf[tid * L + i] = before + run[i];
    }
  }
  sim_sync<WG>();

  const double total = cdf[M - 1];
  int j_last = 0;   // #{i : cdf[i] < total}: an outcome of probability 0 at the end of the range is never drawn
  for (int step = M >> 1; step >= 1; step >>= 1)
    if (cdf[j_last + step - 1] < total) j_last += step;
  const int64_t key = run_keys[(int64_t)f * B + c];
  const uint32_t key_lo = (uint32_t)(uint64_t)key, key_hi = (uint32_t)((uint64_t)key >> 32);
  const int n_pair = (shots + 1) >> 1;   // a Philox block serves shots 2 i (words 0, 1) and 2 i + 1 (words 2, 3)
  for (int i0 = 0; i0 < n_pair; i0 += T) {
    const int i = i0 + tid;
    if (i < n_pair) {
      uint32_t x[4];
      philox4x32_10((uint32_t)i, (uint32_t)gl, key_lo, key_hi, seed_lo, seed_hi, x);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        if (2 * i + h < shots) {
          // u = ((x0 >> 5) 2^26 + (x1 >> 6)) 2^-53: 53 bits, every step exact
          const double u = ((double)(x[2 * h] >> 5) * 67108864.0 + (double)(x[2 * h + 1] >> 6)) * 0x1p-53;
          const double target = u * total;
          int j = 0;   // #{i : cdf[i] <= target}, capped at M - 1 and then at j_last
          for (int step = M >> 1; step >= 1; step >>= 1)
            if (cdf[j + step - 1] <= target) j += step;
          atomicAdd(&cnt[min(j, j_last)], 1);
        }
      }
    }
  }
  sim_sync<WG>();

  if (ok)
    for (int j = tid; j < M; j += T) counts[(int64_t)f * n_outcomes + pb + j] = cnt[j];

  // the group's terms: S_t = sum_j counts_j (-1)^popcount(j & support_t), an integer; estimate = S_t / shots
  const int64_t tb = min(max(term_ptr[c], (int64_t)0), n_terms), te = min(max(term_ptr[c + 1], tb), n_terms);
  const int n_term = __builtin_amdgcn_readfirstlane((int)min(te - tb, (int64_t)0x7FFFFFFF));
  const int qmask = M - 1;
  for (int t = 0; t < n_term; ++t) {
    if (__builtin_amdgcn_readfirstlane(term_group[tb + t]) != gl) continue;   // uniform over the wave / workgroup
    const sim_i4 term = terms[tb + t];
    const int support = __builtin_amdgcn_readfirstlane((term.x | term.y) & qmask);
    int part_sum = 0;
    for (int j = tid; j < M; j += T) part_sum += __popc(j & support) & 1 ? -cnt[j] : cnt[j];
    int s = sim_wave_sum_int(part_sum);
    if (WG) {
      if ((tid & (kWave - 1)) == 0) red_s[tid >> 6] = s;
      __syncthreads();
      s = red_s[0] + red_s[1] + red_s[2] + red_s[3];
      __syncthreads();   // red_s is free again
    }
    if (tid == 0) term_values[(int64_t)f * n_terms + tb + t] = (double)s / (double)shots;
  }
}

// values and variances of the sampled runs: one thread per run r = f * B + c, terms in order, a fused multiply-add per term
__global__ __launch_bounds__(kBlock) void sample_finish_kernel(int B, int64_t n_runs, const int64_t* __restrict__ term_ptr,
                                                               const double* __restrict__ coeff, int64_t n_terms,
                                                               const double* __restrict__ term_values, double* __restrict__ values,
                                                               double* __restrict__ variance) {
  const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (r >= n_runs) return;
  const int64_t c = r % B, f = r / B;
  const int64_t tb = min(max(term_ptr[c], (int64_t)0), n_terms), te = min(max(term_ptr[c + 1], tb), n_terms);
  sample_value_variance(coeff, tb, te, values[r], variance[r], [&](int64_t t) { return term_values[f * n_terms + t]; });
}

}  // namespace
}  // namespace mlqem

using namespace mlqem;

extern "C" int mlqem_sim_run_f64(int64_t n_circuits, const int32_t* circ, const int64_t* op_ptr, const mlqem_sim_op* ops, int64_t n_ops,
                                 const double* params, int64_t n_params, const int64_t* term_ptr, const mlqem_sim_term* terms,
                                 const double* coeff, int64_t n_terms, const int32_t* ids, int64_t n_wave, int64_t n_wg,
                                 double* term_values, double* values, double* norm, mlqem_stream_t stream) {
  begin_launches();
  if (!sim_batch_sizes(n_circuits, n_ops, n_params, n_terms, n_wave, n_wg)) return MLQEM_ERR_BAD_ARG;
  if (n_wave + n_wg > n_circuits) return MLQEM_ERR_BAD_ARG;
  if (n_circuits > 0x7FFFFFFFll || n_params > 0x7FFFFFFFll) return MLQEM_ERR_UNSUPPORTED;
  if (n_wave + n_wg == 0) return MLQEM_OK;
  SimBatchPtrs b;
  if (int code = sim_batch_buffers(circ, op_ptr, ops, n_ops, params, term_ptr, terms, coeff, n_terms, ids, b)) return code;
  if (!values || !norm || (n_terms > 0 && !term_values)) return MLQEM_ERR_BAD_ARG;
  sim_launch_pair(ids, n_wave, n_wg, 1, [&](auto wg, dim3 grid, const int32_t* id, int count) {
    hipLaunchKernelGGL((sim_kernel<decltype(wg)::value, false>), grid, dim3(kBlock), 0, as_stream(stream), (int)n_circuits, b.circ, op_ptr,
                       b.ops, n_ops, params, n_params, term_ptr, b.terms, coeff, n_terms, id, count, term_values, values, norm, 0,
                       (const int64_t*)nullptr, (const int32_t*)nullptr, (int64_t)0);
  });
  return launch_status();
}

extern "C" int mlqem_sim_run_folded_f64(int64_t n_circuits, int64_t n_factors, const int32_t* circ, const int64_t* op_ptr,
                                        const mlqem_sim_op* ops, int64_t n_ops, const double* params, int64_t n_params,
                                        const int64_t* term_ptr, const mlqem_sim_term* terms, const double* coeff, int64_t n_terms,
                                        const int64_t* sched_ptr, const int32_t* sched, int64_t n_sched, const int32_t* ids,
                                        int64_t n_wave, int64_t n_wg, double* term_values, double* values, double* norm,
                                        mlqem_stream_t stream) {
  begin_launches();
  if (!sim_batch_sizes(n_circuits, n_ops, n_params, n_terms, n_wave, n_wg) || n_factors < 1 || n_sched < 0) return MLQEM_ERR_BAD_ARG;
  if (n_circuits > 0x7FFFFFFFll || n_factors > 0x7FFFFFFFll || n_params > 0x7FFFFFFFll || n_sched > 0x7FFFFFFFll)
    return MLQEM_ERR_UNSUPPORTED;
  const int64_t n_runs = n_factors * n_circuits;   // both below 2^31: no overflow
  if (n_runs > 0x7FFFFFFFll) return MLQEM_ERR_UNSUPPORTED;
  if (n_wave + n_wg > n_runs) return MLQEM_ERR_BAD_ARG;
  if (n_wave + n_wg == 0) return MLQEM_OK;
  SimBatchPtrs b;
  if (int code = sim_batch_buffers(circ, op_ptr, ops, n_ops, params, term_ptr, terms, coeff, n_terms, ids, b)) return code;
  if (!sched_ptr || !values || !norm || (n_sched > 0 && !sched) || (n_terms > 0 && !term_values)) return MLQEM_ERR_BAD_ARG;
  if (!aligned_to(sched_ptr, 8) || !aligned_to(sched, 4)) return MLQEM_ERR_BAD_ARG;
  sim_launch_pair(ids, n_wave, n_wg, 1, [&](auto wg, dim3 grid, const int32_t* id, int count) {
    hipLaunchKernelGGL((sim_kernel<decltype(wg)::value, true>), grid, dim3(kBlock), 0, as_stream(stream), (int)n_circuits, b.circ, op_ptr,
                       b.ops, n_ops, params, n_params, term_ptr, b.terms, coeff, n_terms, id, count, term_values, values, norm,
                       (int)n_runs, sched_ptr, sched, n_sched);
  });
  return launch_status();
}

extern "C" int mlqem_zne_combine_f64(int64_t n_factors, int64_t n_circuits, const double* term_values, const double* weights,
                                     const int64_t* term_ptr, const double* coeff, int64_t n_terms, double* mitigated_terms,
                                     double* mitigated_values, mlqem_stream_t stream) {
  begin_launches();
  if (n_factors < 1 || n_circuits < 0 || n_terms < 0) return MLQEM_ERR_BAD_ARG;
  if (n_factors > 0x7FFFFFFFll || n_circuits > 0x7FFFFFFFll || n_terms > 0x7FFFFFFFll) return MLQEM_ERR_UNSUPPORTED;
  if (n_circuits == 0 && n_terms == 0) return MLQEM_OK;
  if (!weights || (n_circuits > 0 && (!term_ptr || !mitigated_values)) || (n_terms > 0 && (!term_values || !coeff || !mitigated_terms)))
    return MLQEM_ERR_BAD_ARG;
  const int64_t blocks = ceil_div(n_circuits > n_terms ? n_circuits : n_terms, (int64_t)kBlock);
  hipLaunchKernelGGL(zne_combine_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, as_stream(stream), (int)n_factors, term_values, weights,
                     term_ptr, coeff, n_terms, n_circuits, mitigated_terms, mitigated_values);
  return launch_status();
}

extern "C" int mlqem_zne_combine_exp_f64(int64_t n_factors, int64_t n_circuits, const double* term_values, const double* weights,
                                         const int64_t* term_ptr, const double* coeff, int64_t n_terms, double* mitigated_terms,
                                         double* mitigated_values, int32_t* fallback, mlqem_stream_t stream) {
  begin_launches();
  if (n_factors < 2 || n_circuits < 0 || n_terms < 0) return MLQEM_ERR_BAD_ARG;   // a line needs two points
  if (n_factors > 0x7FFFFFFFll || n_circuits > 0x7FFFFFFFll || n_terms > 0x7FFFFFFFll) return MLQEM_ERR_UNSUPPORTED;
  if (n_circuits == 0 && n_terms == 0) return MLQEM_OK;
  if (!weights || (n_circuits > 0 && (!term_ptr || !mitigated_values)) ||
      (n_terms > 0 && (!term_values || !coeff || !mitigated_terms || !fallback)))
    return MLQEM_ERR_BAD_ARG;
  const int64_t blocks = ceil_div(n_circuits > n_terms ? n_circuits : n_terms, (int64_t)kBlock);
  hipLaunchKernelGGL(zne_combine_exp_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, as_stream(stream), (int)n_factors, term_values,
                     weights, term_ptr, coeff, n_terms, n_circuits, mitigated_terms, mitigated_values, fallback);
  return launch_status();
}

// The two measured entry points share their checks and launches: `sched_ptr == nullptr` is the plain run (n_factors = 1).
static int sim_run_measured_impl(bool fold, int64_t n_circuits, int64_t n_factors, const int32_t* circ, const int64_t* op_ptr,
                                 const mlqem_sim_op* ops, int64_t n_ops, const double* params, int64_t n_params, const int64_t* term_ptr,
                                 const mlqem_sim_term* terms, const double* coeff, int64_t n_terms, const int64_t* group_ptr,
                                 const int64_t* prob_ptr, int64_t n_groups, int64_t n_outcomes, const int64_t* sched_ptr,
                                 const int32_t* sched, int64_t n_sched, const int32_t* ids, int64_t n_wave, int64_t n_wg,
                                 double* term_values, double* values, double* norm, double* probs, mlqem_stream_t stream) {
  begin_launches();
  if (!sim_batch_sizes(n_circuits, n_ops, n_params, n_terms, n_wave, n_wg) || n_factors < 1 || n_sched < 0 || n_groups < 0 || n_outcomes < 0)
    return MLQEM_ERR_BAD_ARG;
  if (n_circuits > 0x7FFFFFFFll || n_factors > 0x7FFFFFFFll || n_params > 0x7FFFFFFFll || n_sched > 0x7FFFFFFFll ||
      n_groups > 0x7FFFFFFFll)
    return MLQEM_ERR_UNSUPPORTED;
  const int64_t n_runs = n_factors * n_circuits;   // both below 2^31: no overflow
  if (n_runs > 0x7FFFFFFFll) return MLQEM_ERR_UNSUPPORTED;
  if (n_wave + n_wg > n_runs) return MLQEM_ERR_BAD_ARG;
  if (n_wave + n_wg == 0) return MLQEM_OK;
  SimBatchPtrs b;
  if (int code = sim_batch_buffers(circ, op_ptr, ops, n_ops, params, term_ptr, terms, coeff, n_terms, ids, b)) return code;
  if (!group_ptr || !prob_ptr || !values || !norm || (fold && (!sched_ptr || (n_sched > 0 && !sched))) || (n_terms > 0 && !term_values) ||
      (n_outcomes > 0 && !probs))
    return MLQEM_ERR_BAD_ARG;
  if (!aligned_to(sched_ptr, 8) || !aligned_to(sched, 4) || !aligned_to(group_ptr, 8) || !aligned_to(prob_ptr, 8) || !aligned_to(probs, 8))
    return MLQEM_ERR_BAD_ARG;
  sim_launch_pair(ids, n_wave, n_wg, 1, [&](auto wg, dim3 grid, const int32_t* id, int count) {
    auto kernel = fold ? sim_kernel<decltype(wg)::value, true, true> : sim_kernel<decltype(wg)::value, false, true>;
    hipLaunchKernelGGL(kernel, grid, dim3(kBlock), 0, as_stream(stream), (int)n_circuits, b.circ, op_ptr, b.ops, n_ops, params, n_params,
                       term_ptr, b.terms, coeff, n_terms, id, count, term_values, values, norm, (int)n_runs, sched_ptr, sched, n_sched,
                       group_ptr, prob_ptr, n_groups, n_outcomes, probs);
  });
  return launch_status();
}

extern "C" int mlqem_sim_run_measured_f64(int64_t n_circuits, const int32_t* circ, const int64_t* op_ptr, const mlqem_sim_op* ops,
                                          int64_t n_ops, const double* params, int64_t n_params, const int64_t* term_ptr,
                                          const mlqem_sim_term* terms, const double* coeff, int64_t n_terms, const int64_t* group_ptr,
                                          const int64_t* prob_ptr, int64_t n_groups, int64_t n_outcomes, const int32_t* ids,
                                          int64_t n_wave, int64_t n_wg, double* term_values, double* values, double* norm,
                                          double* probs, mlqem_stream_t stream) {
  return sim_run_measured_impl(false, n_circuits, 1, circ, op_ptr, ops, n_ops, params, n_params, term_ptr, terms, coeff, n_terms,
                               group_ptr, prob_ptr, n_groups, n_outcomes, nullptr, nullptr, 0, ids, n_wave, n_wg, term_values, values,
                               norm, probs, stream);
}

extern "C" int mlqem_sim_run_folded_measured_f64(int64_t n_circuits, int64_t n_factors, const int32_t* circ, const int64_t* op_ptr,
                                                 const mlqem_sim_op* ops, int64_t n_ops, const double* params, int64_t n_params,
                                                 const int64_t* term_ptr, const mlqem_sim_term* terms, const double* coeff,
                                                 int64_t n_terms, const int64_t* group_ptr, const int64_t* prob_ptr, int64_t n_groups,
                                                 int64_t n_outcomes, const int64_t* sched_ptr, const int32_t* sched, int64_t n_sched,
                                                 const int32_t* ids, int64_t n_wave, int64_t n_wg, double* term_values, double* values,
                                                 double* norm, double* probs, mlqem_stream_t stream) {
  return sim_run_measured_impl(true, n_circuits, n_factors, circ, op_ptr, ops, n_ops, params, n_params, term_ptr, terms, coeff, n_terms,
                               group_ptr, prob_ptr, n_groups, n_outcomes, sched_ptr, sched, n_sched, ids, n_wave, n_wg, term_values,
                               values, norm, probs, stream);
}

extern "C" int mlqem_sim_sample_f64(int64_t n_circuits, int64_t n_factors, const int32_t* circ, const int64_t* term_ptr,
                                    const mlqem_sim_term* terms, const double* coeff, int64_t n_terms, const int64_t* group_ptr,
                                    const int32_t* term_group, const int64_t* prob_ptr, const int32_t* group_circ, int64_t n_groups,
                                    int64_t n_outcomes, const double* probs, const int64_t* run_keys, int64_t shots, uint64_t seed,
                                    const int32_t* units, int64_t n_wave, int64_t n_wg, int32_t* counts, double* term_values,
                                    double* values, double* variance, mlqem_stream_t stream) {
  begin_launches();
  if (n_circuits < 0 || n_factors < 1 || n_terms < 0 || n_groups < 0 || n_outcomes < 0 || n_wave < 0 || n_wg < 0) return MLQEM_ERR_BAD_ARG;
  if (shots < 1 || shots > MLQEM_SIM_MAX_SHOTS) return MLQEM_ERR_BAD_ARG;
  if (n_circuits > 0x7FFFFFFFll || n_factors > 0x7FFFFFFFll || n_groups > 0x7FFFFFFFll) return MLQEM_ERR_UNSUPPORTED;
  const int64_t n_runs = n_factors * n_circuits, n_units = n_factors * n_groups;   // factors below 2^31: no overflow
  if (n_runs > 0x7FFFFFFFll || n_units > 0x7FFFFFFFll) return MLQEM_ERR_UNSUPPORTED;
  if (n_wave + n_wg != n_units) return MLQEM_ERR_BAD_ARG;   // every (factor, group) pair is sampled: the values need all of them
  if (n_circuits == 0) return MLQEM_OK;
  if (n_groups < 1 || n_outcomes < 1) return MLQEM_ERR_BAD_ARG;   // a circuit has at least one group of at least two outcomes
  if (!circ || !term_ptr || !group_ptr || !prob_ptr || !group_circ || !probs || !run_keys || !units || !counts || !values || !variance ||
      (n_terms > 0 && (!terms || !coeff || !term_group || !term_values)))
    return MLQEM_ERR_BAD_ARG;
  if (!aligned_to(circ, 16) || !aligned_to(terms, 16) || !aligned_to(probs, 8) || !aligned_to(run_keys, 8)) return MLQEM_ERR_BAD_ARG;
  const sim_i4* ci = reinterpret_cast<const sim_i4*>(circ);
  const sim_i4* ti = reinterpret_cast<const sim_i4*>(terms);
  const uint32_t seed_lo = (uint32_t)seed, seed_hi = (uint32_t)(seed >> 32);
  sim_launch_pair(units, n_wave, n_wg, 1, [&](auto wg, dim3 grid, const int32_t* unit, int count) {
    hipLaunchKernelGGL((sample_kernel<decltype(wg)::value>), grid, dim3(kBlock), 0, as_stream(stream), (int)n_circuits, (int)n_factors, ci,
                       term_ptr, ti, n_terms, group_ptr, term_group, prob_ptr, group_circ, (int)n_groups, n_outcomes, probs, run_keys,
                       (int)shots, seed_lo, seed_hi, unit, count, counts, term_values);
  });
  hipLaunchKernelGGL(sample_finish_kernel, dim3((unsigned)ceil_div(n_runs, (int64_t)kBlock)), dim3(kBlock), 0, as_stream(stream),
                     (int)n_circuits, n_runs, term_ptr, coeff, n_terms, term_values, values, variance);
  return launch_status();
}
