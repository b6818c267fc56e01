// Quantum-trajectory simulation of noisy circuits, a batch per call (mlqem_sim_run_trajectories_f64).  include/mlqem_hip.h has the
// contract: the unravelling of every noise record, the selection rule, the Philox counter layout and the outputs.
//
// A circuit under noise whose density matrix does not fit the LDS state (6 .. 11 qubits) still has a state VECTOR that does.  So
// the circuit runs as T pure-state trajectories: gate records act as in vector mode, and at every noise record ONE Kraus operator
// is drawn and applied.  The state, the passes and the rules are sim.hip's (sim_ctx.hpp): complex float64 amplitudes in LDS, loads
// unconditional on clamped and masked indices, only stores predicated, trip counts that depend on the amplitude count alone, a
// malformed record computes garbage and faults nothing.
//
// Work unit: one (circuit, trajectory) pair.  WG = false: a wave per unit, four units per 256-thread workgroup on 4 KB each and no
// workgroup barrier (the four waves draw different operators, so their pass counts differ).  WG = true: a workgroup per unit, 32 KB,
// a barrier after every pass.  Unit u of a launch is trajectory u % T of the launch's circuit u / T.
//
// Every lane of a unit computes the same uniform from the same counter, and the populations a relaxation draw depends on are
// broadcast from the fixed-order reduction, so every branch on a draw is wave-uniform (workgroup-uniform in the workgroup variant:
// its threads read the same four wave sums from LDS and add them in the same order).
//
// Two passes are new.  pauli: st'[i] = i^ny (-1)^popcount(j & z) st[j], j = i ^ x, for a Pauli string on one or two qubits; a thread
// owns the pair (i, i ^ x), swaps and negates components, no arithmetic.  populations: the sums of |amplitude|^2 over the two
// values of one qubit, reduced in the fixed order of SimCtx::reduce.  A relaxation's operator is a real 2x2 matrix through
// SimCtx::pair.
#include "sim_ctx.hpp"

namespace mlqem {
namespace {

template <bool WG> struct TrajCtx {
  SimCtx<WG>& cx;
  int n, traj;
  uint32_t key_lo, key_hi, seed_lo, seed_hi;

  // u = ((x0 >> 5) 2^26 + (x1 >> 6)) 2^-53 of the Philox block (step, sub << 24 | trajectory, run key); the same in every lane
  __device__ __forceinline__ double uniform(int step, int sub) const {
    uint32_t x[4];
    philox4x32_10((uint32_t)step, ((uint32_t)sub << 24) | (uint32_t)traj, key_lo, key_hi, seed_lo, seed_hi, x);
    return ((double)(x[0] >> 5) * 67108864.0 + (double)(x[1] >> 6)) * 0x1p-53;
  }

  static __device__ __forceinline__ double bcast(double v) {   // lane 0's value, as a scalar
    const uint64_t b = __builtin_bit_cast(uint64_t, v);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)b), hi = __builtin_amdgcn_readfirstlane((uint32_t)(b >> 32));
    return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
  }

  // i^ny v, negated where `neg`: components swapped and negated, exact
  static __device__ __forceinline__ sim_c turn(sim_c v, int ny, bool neg) {
    sim_c r = ny == 0 ? v : ny == 1 ? sim_c{-v.y, v.x} : ny == 2 ? sim_c{-v.x, -v.y} : sim_c{v.y, -v.x};
    return neg ? sim_c{-r.x, -r.y} : r;
  }

  // the Pauli string (xm, zm, ny): P|j> = i^ny (-1)^popcount(j & zm) |j ^ xm>.  One pass.
  __device__ __forceinline__ void pauli(int xm, int zm, int ny) {
    const int A = cx.A, tid = cx.tid;
    constexpr int T = SimCtx<WG>::T;
    if (xm == 0) {   // diagonal (wave-uniform): a sign per entry
      cx.element([&](int i) { return sim_c{__popc(i & zm) & 1 ? -1.0 : 1.0, 0.0}; });
      return;
    }
    const int b = __ffs(xm) - 1, np = A >> 1;   // bit b splits the state into the pairs (i0, i0 ^ xm)
    for (int p0 = 0; p0 < np; p0 += T) {
      const int p = p0 + tid;
      const bool live = p < np;
      const int i0 = insert0(min(p, np - 1), b) & (A - 1), i1 = (i0 ^ xm) & (A - 1);
      const sim_c a0 = cx.st[i0], a1 = cx.st[i1];
      const sim_c r0 = turn(a1, ny, __popc(i1 & zm) & 1), r1 = turn(a0, ny, __popc(i0 & zm) & 1);
      if (live) {
        cx.st[i0] = r0;
        cx.st[i1] = r1;
      }
    }
    sim_sync<WG>();
  }

  // the depolarising draw on one qubit (two = false) or on the pair: identity, or one of the 3 / 15 Pauli strings.  The running
  // sum is s_0 = 1 - m w, s_k = s_(k-1) + w with w = lam / (m + 1), m = 3 or 15; the first s_k > u is taken, else the last.
  __device__ __forceinline__ void depolarise(int step, bool two, int q0, int q1, double lam) {
    if (!(lam != 0.0)) return;   // lambda = 0: no draw, no pass (wave-uniform: lam comes from the record)
    const double u = uniform(step, 0);
    const int m = two ? 15 : 3;
    const double w = two ? lam * 0.0625 : lam * 0.25;
    double run = 1.0 - (double)m * w;
    int code = 0;
    while (code < m && !(run > u)) {
      run = run + w;
      ++code;
    }
    code = __builtin_amdgcn_readfirstlane(code);
    if (code == 0) return;
    const int la = two ? code & 3 : code, lb = two ? code >> 2 : 0;   // letters: 0 I, 1 X, 2 Y, 3 Z
    const int xm = ((la == 1 || la == 2) << q0) | ((lb == 1 || lb == 2) << q1), zm = ((la >= 2) << q0) | ((lb >= 2) << q1);
    pauli(xm, zm, (la == 2) + (lb == 2));
  }

  // thermal relaxation (g, c, p1) of qubit q: the populations, one uniform, one of six Kraus operators over the root of its own
  // probability as a real 2x2 matrix
  __device__ __forceinline__ void relax(int step, int sub, int q, double g, double c, double p1) {
    const int A = cx.A, tid = cx.tid, np = A >> 1;
    constexpr int T = SimCtx<WG>::T;
    double s0 = 0.0, s1 = 0.0;
    for (int p0 = 0; p0 < np; p0 += T) {
      const int p = p0 + tid;
      const bool live = p < np;
      const int i0 = insert0(min(p, np - 1), q) & (A - 1), i1 = (i0 | (1 << q)) & (A - 1);
      const sim_c a0 = cx.st[i0], a1 = cx.st[i1];
      s0 = s0 + (live ? a0.x * a0.x + a0.y * a0.y : 0.0);
      s1 = s1 + (live ? a1.x * a1.x + a1.y * a1.y : 0.0);
    }
    const double P0 = bcast(cx.reduce(s0, 0)), P1 = bcast(cx.reduce(s1, 1));
    const double S = P0 + P1, pa = P0 / S, pb = P1 / S;   // the populations of |0> and |1>
    const double c2 = c * c, d = fmax(0.0, (1.0 - g) - c2), w0 = 1.0 - p1;
    const double k0 = pa + c2 * pb, k3 = c2 * pa + pb;
    const double pr[6] = {w0 * k0, w0 * (g * pb), w0 * (d * pb), p1 * k3, p1 * (g * pa), p1 * (d * pa)};
    const double u = uniform(step, sub);
    double run = 0.0;
    int pick = -1, last = -1;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      run = run + pr[j];
      if (pick < 0 && run > u) pick = j;
      if (pr[j] > 0.0) last = j;
    }
    pick = __builtin_amdgcn_readfirstlane(pick >= 0 ? pick : max(last, 0));
    // K / sqrt(its probability): the weight and, for a jump, g or d cancel
    const double den = pick == 0 ? k0 : pick == 3 ? k3 : (pick == 1 || pick == 2) ? pb : pa;
    const double r = 1.0 / sqrt(den);
    const double m00 = pick == 0 || pick == 5 ? r : pick == 3 ? c * r : 0.0, m01 = pick == 1 ? r : 0.0, m10 = pick == 4 ? r : 0.0,
                 m11 = pick == 3 || pick == 2 ? r : pick == 0 ? c * r : 0.0;
    cx.pair(n, q, sim_c{m00, 0.0}, sim_c{m01, 0.0}, sim_c{m10, 0.0}, sim_c{m11, 0.0}, 1);
  }
};

// Occupancy.  The wave variant fits 64 VGPRs and its 16.5 KB of LDS per workgroup allow nine workgroups a CU, so it states the 8
// waves per SIMD the hardware has; the workgroup variant is bound by its 32 KB of LDS and states 4, as sim_kernel's (DESIGN.md 3.13
// has the compiler's figures).  A pass that does not fit its figure's register budget shows up as scratch.
template <bool WG>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(WG ? 4 : 8))) void traj_kernel(
    int B, const sim_i4* __restrict__ circ, const int64_t* __restrict__ op_ptr, const sim_i4* __restrict__ ops, int64_t n_ops,
    const double* __restrict__ params, int64_t n_params, const int64_t* __restrict__ term_ptr, const sim_i4* __restrict__ terms,
    int64_t n_terms, const int32_t* __restrict__ ids, int n_ids, int T, const int64_t* __restrict__ run_keys, uint32_t seed_lo,
    uint32_t seed_hi, double* __restrict__ traj_terms, double* __restrict__ traj_norm) {
  constexpr int kMaxBits = WG ? 11 : 8, kPer = WG ? 1 : kBlock / kWave;
  __shared__ sim_c state[WG ? kSimMaxAmps : kBlock / kWave * kSimWaveAmps];
  __shared__ double red[8];
  __shared__ double ro_s[kPer * 2 * kMaxBits];   // r[q] = (factor of bit 0, factor of bit 1) of the readout channel
  SimCtx<WG> cx;
  const int slot = WG ? (int)blockIdx.x : __builtin_amdgcn_readfirstlane((int)blockIdx.x * (kBlock / kWave) + ((int)threadIdx.x >> 6));
  if (slot >= n_ids * T) return;   // a wave of a partly filled workgroup: wave-uniform, and this variant has no workgroup barrier
  cx.tid = WG ? (int)threadIdx.x : (int)threadIdx.x & (kWave - 1);
  cx.st = WG ? state : state + ((int)threadIdx.x >> 6) * kSimWaveAmps;
  cx.red = red;
  double* ro = WG ? ro_s : ro_s + ((int)threadIdx.x >> 6) * 2 * kMaxBits;
  const int tid = cx.tid;
  const int ci = slot / T, traj = slot - ci * T;
  const int c = __builtin_amdgcn_readfirstlane(min(max(ids[ci], 0), B - 1));
  const sim_i4 info = circ[c];   // n_qubits, mode (2 here; not read), trailing readout ops, reserved
  const int n = __builtin_amdgcn_readfirstlane(min(max(info.x, 1), kMaxBits));
  const int A = 1 << n;
  cx.nbits = n;
  cx.A = A;
  const int64_t ob = min(max(op_ptr[c], (int64_t)0), n_ops), oe = min(max(op_ptr[c + 1], ob), n_ops);
  const int n_step = __builtin_amdgcn_readfirstlane((int)min(oe - ob, (int64_t)0x7FFFFFFF));
  const int n_ro = min(max(info.z, 0), n_step), n_main = n_step - n_ro;
  const int64_t key = run_keys[c];
  TrajCtx<WG> tc{cx, n, traj, (uint32_t)(uint64_t)key, (uint32_t)((uint64_t)key >> 32), seed_lo, seed_hi};

  for (int i = tid; i < A; i += cx.T) cx.st[i] = sim_c{i == 0 ? 1.0 : 0.0, 0.0};
  if (tid < 2 * kMaxBits) ro[tid] = tid & 1 ? -1.0 : 1.0;
  sim_sync<WG>();

  for (int k = 0; k < n_step; ++k) {
    const sim_i4 op = ops[ob + k];   // kind, q0, q1, offset into params
    const int kind = __builtin_amdgcn_readfirstlane(op.x);
    const int q0 = __builtin_amdgcn_readfirstlane(min(max(op.y, 0), n - 1)), q1 = __builtin_amdgcn_readfirstlane(min(max(op.z, 0), n - 1));
    const int64_t po = min((int64_t)max(op.w, 0), n_params - kSimParamPad);
    const double* m = params + po;
    if (k >= n_main) {   // the trailing records: readout fills the table, the state stays as it is
      if (kind == MLQEM_SIM_OP_READOUT && tid == 0) {   // m = (p01, p10)
        ro[2 * q0] = 1.0 - 2.0 * m[1];
        ro[2 * q0 + 1] = -(1.0 - 2.0 * m[0]);
      }
      continue;
    }
    switch (kind) {
      case MLQEM_SIM_OP_U1:
        cx.pair(n, q0, sim_c{m[0], m[1]}, sim_c{m[2], m[3]}, sim_c{m[4], m[5]}, sim_c{m[6], m[7]}, 1);
        break;
      case MLQEM_SIM_OP_DIAG1: {
        const sim_c d0{m[0], m[1]}, d1{m[2], m[3]};
        cx.element([&](int i) { return (i >> q0) & 1 ? d1 : d0; });
        break;
      }
      case MLQEM_SIM_OP_CZ: {
        const int mrow = (1 << q0) | (1 << q1);
        cx.element([&](int i) { return sim_c{(i & mrow) == mrow ? -1.0 : 1.0, 0.0}; });
        break;
      }
      case MLQEM_SIM_OP_CX:
        cx.gather([&](int i) { return i ^ (((i >> q0) & 1) << q1); });
        break;
      case MLQEM_SIM_OP_SWAP:
        cx.gather([&](int i) { return i ^ ((((i >> q0) ^ (i >> q1)) & 1) * ((1 << q0) | (1 << q1))); });
        break;
      case MLQEM_SIM_OP_U2:
        cx.quad(q0, q1, m, false);
        break;
      case MLQEM_SIM_OP_DEPOL1:
        tc.depolarise(k, false, q0, q0, m[0]);
        break;
      case MLQEM_SIM_OP_DEPOL2:
        tc.depolarise(k, true, q0, q1, m[0]);
        break;
      case MLQEM_SIM_OP_NOISE1:
        tc.depolarise(k, false, q0, q0, m[0]);
        tc.relax(k, 1, q0, m[1], m[2], m[3]);
        break;
      case MLQEM_SIM_OP_NOISE2:
        tc.depolarise(k, true, q0, q1, m[0]);
        tc.relax(k, 1, q0, m[1], m[2], m[3]);
        tc.relax(k, 2, q1, m[4], m[5], m[6]);
        break;
      default:
        break;
    }
  }
  sim_sync<WG>();   // the readout table is complete

  double nrm;
  {   // <psi|psi>
    double part = 0.0;
    for (int i0 = 0; i0 < A; i0 += cx.T) {
      const int i = i0 + tid;
      const sim_c v = cx.st[i & (A - 1)];
      part = part + (i < A ? v.x * v.x + v.y * v.y : 0.0);
    }
    nrm = cx.reduce(part, 0);
    if (WG) __syncthreads();   // red[0..3] is free again
  }

  // Pauli terms: P|j> = i^ny (-1)^popcount(j & z) |j ^ x>; a term without X or Y under the readout channel takes the table's factors
  const int64_t tb = min(max(term_ptr[c], (int64_t)0), n_terms), te = min(max(term_ptr[c + 1], tb), n_terms);
  const int n_term = __builtin_amdgcn_readfirstlane((int)min(te - tb, (int64_t)0x7FFFFFFF));
  const int qmask = A - 1;
  for (int t = 0; t < n_term; ++t) {
    const sim_i4 term = terms[tb + t];   // xmask, zmask, number of Y factors, reserved
    const int xm = __builtin_amdgcn_readfirstlane(term.x & qmask), zm = __builtin_amdgcn_readfirstlane(term.y & qmask);
    const int ny = __builtin_amdgcn_readfirstlane(term.z & 3);
    double part = 0.0;
    if (xm == 0 && n_ro > 0) {   // wave-uniform
      for (int i0 = 0; i0 < A; i0 += cx.T) {
        const int i = i0 + tid, j = i & (A - 1);
        const sim_c v = cx.st[j];
        double f = v.x * v.x + v.y * v.y;
        for (int q = 0; q < n; ++q) {
          const double rq = ro[2 * q + ((j >> q) & 1)];
          f = (zm >> q) & 1 ? f * rq : f;
        }
        part = part + (i < A ? f : 0.0);
      }
    } else {
      for (int i0 = 0; i0 < A; i0 += cx.T) {
        const int i = i0 + tid, j = i & (A - 1);
        const sim_c a = cx.st[(j ^ xm) & (A - 1)], b = cx.st[j];     // conj(psi[j ^ x]) psi[j]
        const sim_c v = sim_c{a.x * b.x + a.y * b.y, a.x * b.y - a.y * b.x};
        double re = ny == 0 ? v.x : ny == 1 ? -v.y : ny == 2 ? -v.x : v.y;   // Re(i^ny v)
        re = __popc(j & zm) & 1 ? -re : re;
        part = part + (i < A ? re : 0.0);
      }
    }
    const double tv = cx.reduce(part, t & 1);
    if (tid == 0) traj_terms[(int64_t)traj * n_terms + tb + t] = tv;
  }
  if (tid == 0) traj_norm[(int64_t)traj * B + c] = nrm;
}

// Means and standard errors over the trajectories, in trajectory order.  Thread i < n_terms takes term i (its reads of row t of
// traj_terms are coalesced); thread i < B takes circuit i: its per-trajectory value is sum coeff * term in term order (a fused
// multiply-add per term, from 0.0), formed again in the second pass with the same operations, so the same bits.
__global__ __launch_bounds__(kBlock) void traj_finish_kernel(int64_t B, int64_t n_terms, int T, const int64_t* __restrict__ term_ptr,
                                                             const double* __restrict__ coeff, const double* __restrict__ traj_terms,
                                                             const double* __restrict__ traj_norm, double* __restrict__ term_values,
                                                             double* __restrict__ term_se, double* __restrict__ values,
                                                             double* __restrict__ se, double* __restrict__ norm) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const double count = (double)T, pairs = (double)T * (double)(T - 1);
  if (i < n_terms) {
    const TrajStat s = traj_term_stats(traj_terms, n_terms, T, i);
    term_values[i] = s.mean;
    term_se[i] = s.se;
  }
  if (i < B) {
    const int64_t tb = min(max(term_ptr[i], (int64_t)0), n_terms), te = min(max(term_ptr[i + 1], tb), n_terms);
    double acc = 0.0, nacc = 0.0, m2 = 0.0;
    for (int t = 0; t < T; ++t) {
      acc = acc + traj_value(coeff, traj_terms, n_terms, t, tb, te);
      nacc = nacc + traj_norm[(int64_t)t * B + i];
    }
    const double mean = acc / count;
    for (int t = 0; t < T; ++t) {
      const double d = traj_value(coeff, traj_terms, n_terms, t, tb, te) - mean;
      m2 = __builtin_fma(d, d, m2);
    }
    values[i] = mean;
    se[i] = T > 1 ? sqrt(m2 / pairs) : 0.0;
    norm[i] = nacc / count;
  }
}

}  // namespace
}  // namespace mlqem

using namespace mlqem;

extern "C" int mlqem_sim_run_trajectories_f64(int64_t n_circuits, const int32_t* circ, const int64_t* op_ptr, const mlqem_sim_op* ops,
                                              int64_t n_ops, const double* params, int64_t n_params, const int64_t* term_ptr,
                                              const mlqem_sim_term* terms, const double* coeff, int64_t n_terms, const int32_t* ids,
                                              int64_t n_wave, int64_t n_wg, const int64_t* run_keys, int64_t trajectories, uint64_t seed,
                                              double* traj_term_values, double* traj_norm, double* term_values, double* term_std_error,
                                              double* values, double* std_error, double* norm, mlqem_stream_t stream) {
  begin_launches();
  if (!sim_batch_sizes(n_circuits, n_ops, n_params, n_terms, n_wave, n_wg)) return MLQEM_ERR_BAD_ARG;
  if (trajectories < 1 || trajectories > MLQEM_SIM_MAX_TRAJECTORIES) return MLQEM_ERR_BAD_ARG;
  if (n_circuits > 0x7FFFFFFFll || n_params > 0x7FFFFFFFll || n_terms > 0x7FFFFFFFll) return MLQEM_ERR_UNSUPPORTED;
  if (n_circuits * trajectories > 0x7FFFFFFFll) return MLQEM_ERR_UNSUPPORTED;   // a unit's number is an int
  if (n_wave + n_wg != n_circuits) return MLQEM_ERR_BAD_ARG;   // the finish kernel reads every circuit's trajectories
  if (n_circuits == 0) return MLQEM_OK;
  SimBatchPtrs b;
  if (int code = sim_batch_buffers(circ, op_ptr, ops, n_ops, params, term_ptr, terms, coeff, n_terms, ids, b)) return code;
  if (!run_keys || !traj_norm || !values || !std_error || !norm || (n_terms > 0 && (!traj_term_values || !term_values || !term_std_error)))
    return MLQEM_ERR_BAD_ARG;
  if (!aligned_to(run_keys, 8)) return MLQEM_ERR_BAD_ARG;
  const uint32_t seed_lo = (uint32_t)seed, seed_hi = (uint32_t)(seed >> 32);
  const int T = (int)trajectories;
  sim_launch_pair(ids, n_wave, n_wg, trajectories, [&](auto wg, dim3 grid, const int32_t* id, int count) {
    hipLaunchKernelGGL((traj_kernel<decltype(wg)::value>), grid, dim3(kBlock), 0, as_stream(stream), (int)n_circuits, b.circ, op_ptr, b.ops,
                       n_ops, params, n_params, term_ptr, b.terms, n_terms, id, count, T, run_keys, seed_lo, seed_hi, traj_term_values,
                       traj_norm);
  });
  const int64_t rows = n_circuits > n_terms ? n_circuits : n_terms;
  hipLaunchKernelGGL(traj_finish_kernel, dim3((unsigned)ceil_div(rows, (int64_t)kBlock)), dim3(kBlock), 0, as_stream(stream), n_circuits,
                     n_terms, T, term_ptr, coeff, traj_term_values, traj_norm, term_values, term_std_error, values, std_error, norm);
  return launch_status();
}
