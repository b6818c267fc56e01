// Matrix-product-state simulation of circuits on a line, a batch per call (mlqem_mps_run_f64, mlqem_mps_terms_f64,
// mlqem_mps_finish_f64; mlqem_mps_run_folded_f64 walks a fold schedule over the same records: zero-noise extrapolation), and
// measurement shots from the states it leaves (mlqem_mps_sample_f64, mlqem_mps_sample_finish_f64: the kernels after
// mps_finish_kernel).  include/mlqem_hip.h has the contract: the records, the keep rule, the certificate, the draws.
//
// Work unit of the run kernel: one (circuit, trajectory) pair, a workgroup each.  The site tensors A[q] (chi_l x 2 x chi_r complex
// float64, entry (l, s, r) at (l * 2 + s) * chi + r, chi = max_bond) live in the unit's slice of a global workspace; the bond sizes
// live in LDS while the unit runs and are written behind the tensors at its end.  A one-site record is a 2x2 matrix on s.  A
// two-site record on bond (q, q + 1) forms theta (2 chi_l x 2 chi_r) in LDS, column-major with the row count as leading dimension, so
// that a lane's row of one column is 16 contiguous bytes per lane (one conflict-free 16-byte LDS read), applies the 4x4 matrix,
// keeps a copy of theta in the workspace, and orthogonalises the columns of the LDS copy by one-sided (Hestenes) Jacobi rotations.
// Disjoint column pairs of a round go to the four waves; lane = row; every dot product is a wave reduction in a fixed order
// (shuffle tree, lane 0 broadcast), so every branch on one is wave-uniform.  The column norms are the singular values squared; the
// kept, normalised columns are A[q] and A[q + 1] = A[q]^dagger theta from the copy: no V, no division by a small singular value
// of anything that is kept below the cutoff.  Moving the orthogonality centre is the same primitive with the identity as the
// gate (the keep rule with its cap included: a move cannot raise a bond above chi, so the cap never binds there); to the left it
// runs on theta transposed.  A decomposition that still rotates in its last allowed sweep is counted in the unit's stats.
// Thermal relaxation (the NOISE1 / NOISE2 records, plain runs only) is a quantum jump on one site: its Kraus operator is no unitary,
// so the centre is moved to the qubit first, where the populations are a plain sum over that site's tensor (MpsState::relax).
// A Pauli twirl (the TWIRL_OPEN / TWIRL_CLOSE records, plain and folded runs) is two one-site letters before a gate and their
// image under the ideal gate after its noise, drawn per unit: no decomposition, no move of the centre, nothing in the certificate.
//
// LDS: theta at chi = 32 is 64 x 64 x 16 B = 64 KiB, plus 3 KiB of tables: two workgroups a CU on the 160 KiB of gfx950.
//
// Safety: every site index is clamped to the circuit, every bond size to 1 .. chi, every parameter offset to the pool, the sort
// permutation to the column count; a malformed record or a non-finite matrix computes garbage inside the unit's own slice.
#include "sim_ctx.hpp"

namespace mlqem {
namespace {

constexpr int kMpsMaxBond = MLQEM_MPS_MAX_BOND;       // 32
constexpr int kMpsMaxQubits = MLQEM_MPS_MAX_QUBITS;   // 512
constexpr int kMpsCols = 2 * kMpsMaxBond;             // rows and columns of theta at most
constexpr int kMpsSweeps = MLQEM_MPS_SWEEPS;          // the sweep cap
constexpr int kMpsStats = MLQEM_MPS_STATS;           // float64 per unit of traj_stats
constexpr double kMpsTol2 = MLQEM_MPS_JACOBI_TOL2;        // a pair is rotated where |a^dagger b|^2 > 1e-28 |a|^2 |b|^2
constexpr double kMpsNull = MLQEM_MPS_JACOBI_NULL;        // and both columns hold more than this part of theta's weight

__device__ __forceinline__ double mps_bcast(double v) {   // lane 0's value, as a scalar
  const uint64_t b = __builtin_bit_cast(uint64_t, v);
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)b), hi = __builtin_amdgcn_readfirstlane((uint32_t)(b >> 32));
  return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ double mps_sum(double v) { return mps_bcast(sim_wave_sum(v)); }
__device__ __forceinline__ double norm2(sim_c v) { return v.x * v.x + v.y * v.y; }
__device__ __forceinline__ sim_c cconj(sim_c v) { return sim_c{v.x, -v.y}; }

__host__ __device__ inline int64_t mps_dims_bytes(int max_q) { return ((int64_t)(max_q + 1) * 4 + 15) / 16 * 16; }
__host__ __device__ inline int64_t mps_unit_bytes(int max_q, int chi) {
  return mps_dims_bytes(max_q) + 16 * ((int64_t)max_q * 2 * chi * chi + 4 * (int64_t)chi * chi);
}

struct MpsState {
  sim_c* A;       // the unit's site tensors, site q at A + q * S
  sim_c* stash;   // theta before the rotations, ROW-major [R][C]
  sim_c* th;      // LDS: theta, column-major [C][R]
  double* sig;    // LDS [64]: column norms squared
  int* perm;      // LDS [64]: columns in descending order of sig
  int* dims;      // LDS [n + 1]: bond sizes, dims[0] = dims[n] = 1
  int* flag;      // LDS: a rotation happened in this sweep
  int chi, S, tid, lane, wave;
  double cutoff, discarded, bound;
  int bond, decompositions, unconverged, sweeps;

  // a 2x2 matrix (row-major complex) on the physical index of site q
  __device__ __forceinline__ void one_site(int q, sim_c m00, sim_c m01, sim_c m10, sim_c m11) {
    const int dl = dims[q], dr = dims[q + 1];
    sim_c* a = A + (int64_t)q * S;
    for (int it = tid; it < dl * dr; it += kBlock) {
      const int l = it / dr, r = it - l * dr;
      const sim_c a0 = a[(l * 2) * chi + r], a1 = a[(l * 2 + 1) * chi + r];
      a[(l * 2) * chi + r] = cmac(cmul(m00, a0), m01, a1);
      a[(l * 2 + 1) * chi + r] = cmac(cmul(m10, a0), m11, a1);
    }
    __syncthreads();
  }

  // the letter 1 X, 2 Y, 3 Z on site q (0: nothing)
  __device__ __forceinline__ void pauli(int q, int letter) {
    const sim_c o{0.0, 0.0}, p{1.0, 0.0}, n{-1.0, 0.0}, pi{0.0, 1.0}, ni{0.0, -1.0};
    if (letter == 1) one_site(q, o, p, p, o);
    if (letter == 2) one_site(q, o, ni, pi, o);
    if (letter == 3) one_site(q, p, o, o, n);
  }

  // Thermal relaxation (g, c, p1) of site q, which HOLDS THE ORTHOGONALITY CENTRE (the caller moved it there), with the uniform u:
  // the populations P_s = sum_(l, r) |A[q][l, s, r]|^2 (a thread's entries in stride order, the shuffle tree, the four waves in
  // order by every thread: the same bits everywhere), the six outcomes of the trajectory contract against their running sum, the
  // chosen operator over the root of its own state-given probability as a real 2x2 matrix of norm t.  Every barrier here is
  // reached by the whole workgroup: the trip count depends on the bond sizes alone and the outcome is the same in every thread.
  __device__ __forceinline__ void relax(int q, double g, double c, double p1, double u) {
    const int dl = dims[q], dr = dims[q + 1], items = dl * dr;
    const sim_c* a = A + (int64_t)q * S;
    double s0 = 0.0, s1 = 0.0;
    for (int it0 = 0; it0 < items; it0 += kBlock) {
      const int it = it0 + tid, ic = min(it, items - 1);
      const int l = ic / dr, r = ic - l * dr;
      const sim_c a0 = a[(l * 2) * chi + r], a1 = a[(l * 2 + 1) * chi + r];
      s0 = s0 + (it < items ? norm2(a0) : 0.0);
      s1 = s1 + (it < items ? norm2(a1) : 0.0);
    }
    s0 = mps_sum(s0);
    s1 = mps_sum(s1);
    if (lane == 0) {
      sig[wave] = s0;
      sig[kBlock / kWave + wave] = s1;
    }
    __syncthreads();   // sig is free here: bond_op and one_site end with a barrier, and the next writer stands behind one_site's
    const double P0 = ((sig[0] + sig[1]) + sig[2]) + sig[3], P1 = ((sig[4] + sig[5]) + sig[6]) + sig[7];
    const double sum = P0 + P1, pa = P0 / sum, pb = P1 / sum;
    const double c2 = c * c, d = fmax(0.0, (1.0 - g) - c2), w0 = 1.0 - p1;
    const double k0 = pa + c2 * pb, k3 = c2 * pa + pb;
    const double pr[6] = {w0 * k0, w0 * (g * pb), w0 * (d * pb), p1 * k3, p1 * (g * pa), p1 * (d * pa)};
    double run = 0.0;
    int pick = -1, last = -1;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      run = run + pr[j];
      if (pick < 0 && run > u) pick = j;
      if (pr[j] > 0.0) last = j;
    }
    pick = __builtin_amdgcn_readfirstlane(pick >= 0 ? pick : max(last, 0));
    const double den = pick == 0 ? k0 : pick == 3 ? k3 : (pick == 1 || pick == 2) ? pb : pa;
    const double t = 1.0 / sqrt(den);   // the operator norm of what is applied (c <= 1)
    const double m00 = pick == 0 || pick == 5 ? t : pick == 3 ? c * t : 0.0, m01 = pick == 1 ? t : 0.0, m10 = pick == 4 ? t : 0.0,
                 m11 = pick == 3 || pick == 2 ? t : pick == 0 ? c * t : 0.0;
    one_site(q, sim_c{m00, 0.0}, sim_c{m01, 0.0}, sim_c{m10, 0.0}, sim_c{m11, 0.0});
    bound = t * bound;   // the certificate scales with the operator; `discarded` stays the sum of the eps
  }

  // The bond primitive on sites (q, q + 1): theta = A[q] A[q + 1], the 4x4 matrix g (null: none; `orient`: its basis index is
  // bit(q + 1) + 2 bit(q), else bit(q) + 2 bit(q + 1)), the decomposition, the keep rule.  left = false: A[q] takes the orthonormal
  // columns and the centre ends on q + 1; left = true: theta is decomposed transposed, A[q + 1] takes orthonormal rows and the
  // centre ends on q.  FOLD with `dagger`: g's conjugate transpose, read from the same record by swapped strides and a flipped sign.
  template <bool FOLD = false>
  __device__ __forceinline__ void bond_op(int q, const double* g, int orient, bool left, int dagger = 0) {
    const int dl = dims[q], dm = dims[q + 1], dr = dims[q + 2];
    sim_c* aq = A + (int64_t)q * S;
    sim_c* aq1 = aq + S;
    const int rows_t = 2 * dl, cols_t = 2 * dr;                       // of theta
    const int R = left ? cols_t : rows_t, C = left ? rows_t : cols_t;   // of the matrix that is decomposed
    for (int it = tid; it < dl * dr; it += kBlock) {
      const int l = it / dr, r = it - l * dr;
      sim_c t[4] = {sim_c{0.0, 0.0}, sim_c{0.0, 0.0}, sim_c{0.0, 0.0}, sim_c{0.0, 0.0}};   // t[s0 + 2 s1]
      for (int m = 0; m < dm; ++m) {
        const sim_c a0 = aq[(l * 2) * chi + m], a1 = aq[(l * 2 + 1) * chi + m];
        const sim_c b0 = aq1[(m * 2) * chi + r], b1 = aq1[(m * 2 + 1) * chi + r];
        t[0] = cmac(t[0], a0, b0);
        t[1] = cmac(t[1], a1, b0);
        t[2] = cmac(t[2], a0, b1);
        t[3] = cmac(t[3], a1, b1);
      }
      sim_c o[4] = {t[0], t[1], t[2], t[3]};
      if (g != nullptr) {
        const int rs = FOLD && dagger ? 2 : 8, cs = FOLD && dagger ? 8 : 2;   // strides of a row and of a column in the record
        const double sg = FOLD && dagger ? -1.0 : 1.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int gk = orient ? ((k & 1) << 1) | (k >> 1) : k;
          sim_c acc{0.0, 0.0};
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int gj = orient ? ((j & 1) << 1) | (j >> 1) : j;
            if constexpr (FOLD) {
              acc = cmac(acc, sim_c{g[rs * gk + cs * gj], sg * g[rs * gk + cs * gj + 1]}, t[j]);
            } else {
              acc = cmac(acc, sim_c{g[8 * gk + 2 * gj], g[8 * gk + 2 * gj + 1]}, t[j]);
            }
          }
          o[k] = acc;
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int row = l * 2 + (k & 1), col = (k >> 1) * dr + r;
        const int rr = left ? col : row, cc = left ? row : col;
        th[cc * R + rr] = o[k];
        stash[rr * C + cc] = o[k];
      }
    }
    __syncthreads();

    // one-sided Jacobi: cyclic sweeps over the round-robin schedule of ce = C rounded up to even players (player ce - 1 stays, the
    // others rotate); round r pairs (r, ce - 1) and ((r + p) mod (ce - 1), (r - p) mod (ce - 1)), p = 1 .. ce / 2 - 1
    const int ce = C + (C & 1), mo = ce - 1, half = ce >> 1;
    const bool live = lane < R;
    const int lr = min(lane, R - 1);
    // theta's weight (rotations keep it), summed by every thread in column order: workgroup-uniform.  A column at or below
    // kMpsNull of it is the rounding of the dot products: rotating it orthogonalises nothing, only shrinks it sweep after sweep
    // into the denormals, where the test below loses its meaning and the sweeps run to the cap
    for (int col = wave; col < C; col += kBlock / kWave) {
      const double s2 = mps_sum(live ? norm2(th[col * R + lr]) : 0.0);
      if (lane == 0) sig[col] = s2;
    }
    __syncthreads();
    double weight = 0.0;
    for (int col = 0; col < C; ++col) weight = weight + sig[col];
    const double null2 = kMpsNull * weight;
    __syncthreads();   // sig is written again below
    int rotated = 1, done = 0;
    for (int sweep = 0; sweep < kMpsSweeps; ++sweep) {
      if (tid == 0) *flag = 0;
      __syncthreads();
      for (int round = 0; round < mo; ++round) {
        for (int p = wave; p < half; p += kBlock / kWave) {
          const int a = p == 0 ? mo : (round + p) % mo, b = p == 0 ? round : (round - p + mo) % mo;
          const int i = min(a, b), j = max(a, b);
          if (j >= C) continue;   // the bye of an odd column count: wave-uniform
          const sim_c x = th[i * R + lr], y = th[j * R + lr];
          const double alpha = mps_sum(live ? norm2(x) : 0.0), beta = mps_sum(live ? norm2(y) : 0.0);
          const double gre = mps_sum(live ? x.x * y.x + x.y * y.y : 0.0), gim = mps_sum(live ? x.x * y.y - x.y * y.x : 0.0);
          const double g2 = gre * gre + gim * gim;
          if (g2 > kMpsTol2 * alpha * beta && fmin(alpha, beta) > null2) {   // wave-uniform: all are lane 0's sums or LDS values
            const double gabs = sqrt(g2), zeta = (beta - alpha) / (2.0 * gabs);
            const double tt = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
            const double c = 1.0 / sqrt(1.0 + tt * tt), s = c * tt;
            const sim_c ph{gre / gabs, gim / gabs};   // e^(i phi) of a^dagger b
            const sim_c xn = c * x - s * cmul(cconj(ph), y), yn = s * cmul(ph, x) + c * y;
            if (live) {
              th[i * R + lr] = xn;
              th[j * R + lr] = yn;
            }
            if (lane == 0) *flag = 1;
          }
        }
        __syncthreads();
      }
      rotated = *flag;
      done = sweep + 1;
      __syncthreads();
      if (!rotated) break;   // workgroup-uniform: every thread read the same flag between two barriers
    }

    for (int col = wave; col < C; col += kBlock / kWave) {
      const double s2 = mps_sum(live ? norm2(th[col * R + lr]) : 0.0);
      if (lane == 0) sig[col] = s2;
    }
    if (tid < kMpsCols) perm[tid] = min(tid, C - 1);
    __syncthreads();
    int rank = 0;
    if (tid < C) {
      const double mine = sig[tid];
      for (int i = 0; i < C; ++i) {
        const double other = sig[i];
        rank += (other > mine || (other == mine && i < tid)) ? 1 : 0;
      }
    }
    __syncthreads();
    if (tid < C) perm[min(rank, C - 1)] = tid;
    __syncthreads();

    // the keep rule, by every thread on the same LDS values in the same order: workgroup-uniform
    double total = 0.0;
    for (int r = 0; r < C; ++r) total = total + sig[min(max(perm[r], 0), C - 1)];
    const int kmax = min(min(R, C), chi);
    int k = 0;
    double kept = 0.0;
    for (int r = 0; r < kmax; ++r) {
      const double s2 = sig[min(max(perm[r], 0), C - 1)];
      if (!(s2 > cutoff * total)) break;
      kept = kept + s2;
      k = r + 1;
    }
    if (k == 0) {   // a zero or non-finite theta: keep one column, so that the sizes stay valid
      k = 1;
      kept = sig[min(max(perm[0], 0), C - 1)];
    }
    double dropped = 0.0;
    for (int r = k; r < C; ++r) dropped = dropped + sig[min(max(perm[r], 0), C - 1)];
    const double eps = total > 0.0 ? dropped / total : 0.0;
    const double scale = kept > 0.0 ? sqrt(total / kept) : 1.0;
    discarded = discarded + eps;
    bound = bound + sqrt(2.0 * eps);
    bond = max(bond, k);
    ++decompositions;
    unconverged += rotated ? 1 : 0;   // the last allowed sweep still rotated
    sweeps = max(sweeps, done);

    // the orthonormal factor: column perm[kk] over its norm
    for (int it = tid; it < R * k; it += kBlock) {
      const int row = it / k, kk = it - row * k;
      const int pk = min(max(perm[kk], 0), C - 1);
      const double s2 = sig[pk];
      const sim_c u = th[pk * R + row] * (s2 > 0.0 ? 1.0 / sqrt(s2) : 0.0);
      if (left) {   // row = s1 * dr + r
        const int s1 = row / dr, r = row - s1 * dr;
        aq1[(kk * 2 + s1) * chi + r] = u;
      } else {      // row = l * 2 + s0
        aq[row * chi + kk] = u;
      }
    }
    // the other factor: (orthonormal factor)^dagger times the stashed theta, rescaled to the norm before truncation
    for (int it = tid; it < k * C; it += kBlock) {
      const int kk = it / C, cc = it - kk * C;
      const int pk = min(max(perm[kk], 0), C - 1);
      const double s2 = sig[pk];
      sim_c acc{0.0, 0.0};
      for (int row = 0; row < R; ++row) acc = cmac(acc, cconj(th[pk * R + row]), stash[row * C + cc]);
      acc = acc * (s2 > 0.0 ? scale / sqrt(s2) : 0.0);
      if (left) {   // cc = l * 2 + s0
        aq[cc * chi + kk] = acc;
      } else {      // cc = s1 * dr + r
        const int s1 = cc / dr, r = cc - s1 * dr;
        aq1[(kk * 2 + s1) * chi + r] = acc;
      }
    }
    __syncthreads();
    if (tid == 0) dims[q + 1] = k;
    __syncthreads();
  }
};

// lambda's draw of noise record `index`: the code 0 .. m of the chosen Pauli string (0: identity)
__device__ __forceinline__ int mps_draw(int index, int traj, uint32_t key_lo, uint32_t key_hi, uint32_t seed_lo, uint32_t seed_hi, bool two,
                                        double lam) {
  if (!(lam != 0.0)) return 0;
  uint32_t x[4];
  philox4x32_10((uint32_t)index, (uint32_t)traj, key_lo, key_hi, seed_lo, seed_hi, x);
  const double u = ((double)(x[0] >> 5) * 67108864.0 + (double)(x[1] >> 6)) * 0x1p-53;
  const int m = two ? 15 : 3;
  const double w = two ? lam * 0.0625 : lam * 0.25;
  double run = 1.0 - (double)m * w;
  int code = 0;
  while (code < m && !(run > u)) {
    run = run + w;
    ++code;
  }
  return __builtin_amdgcn_readfirstlane(code);
}

// the uniform of sub-draw `sub` (1: the relaxation of the gate's first qubit, 2: of its second) of noise record `index`
__device__ __forceinline__ double mps_uniform(int index, int sub, int traj, uint32_t key_lo, uint32_t key_hi, uint32_t seed_lo,
                                              uint32_t seed_hi) {
  uint32_t x[4];
  philox4x32_10((uint32_t)index, ((uint32_t)sub << 24) | (uint32_t)traj, key_lo, key_hi, seed_lo, seed_hi, x);
  return ((double)(x[0] >> 5) * 67108864.0 + (double)(x[1] >> 6)) * 0x1p-53;
}

// the code 0 .. 15 of twirl `index` (sub-draw 3): the top four bits of the first word, so a host reproduces it as an integer
__device__ __forceinline__ int mps_twirl_draw(int index, int traj, uint32_t key_lo, uint32_t key_hi, uint32_t seed_lo, uint32_t seed_hi) {
  uint32_t x[4];
  philox4x32_10((uint32_t)index, (3u << 24) | (uint32_t)traj, key_lo, key_hi, seed_lo, seed_hi, x);
  return __builtin_amdgcn_readfirstlane((int)(x[0] >> 28));
}

// FOLD = false: circuit circ_first + cl runs its records in order (mlqem_mps_run_f64).  FOLD = true (mlqem_mps_run_folded_f64):
// `circ_first` counts RUNS r = f * B + c, and run r walks the schedule sched[sched_ptr[r] .. sched_ptr[r + 1]) of entries
// (k << 1) | dagger over circuit c's records; run_keys and traj_stats have one row per run.  The noise index counts the noise
// entries as the run executes them, so a run draws what the plain kernel draws on the schedule written out.
template <bool FOLD>
__global__ __launch_bounds__(kBlock) void mps_run_kernel(int B, const int32_t* __restrict__ n_qubits, const int64_t* __restrict__ op_ptr,
                                                         const sim_i4* __restrict__ ops, int64_t n_ops, const double* __restrict__ params,
                                                         int64_t n_params, const int64_t* __restrict__ run_keys, int circ_first, int traj_first,
                                                         int traj_count, uint32_t seed_lo, uint32_t seed_hi, int chi, double cutoff,
                                                         int max_q, char* __restrict__ workspace, double* __restrict__ traj_stats,
                                                         int n_runs, const int64_t* __restrict__ sched_ptr, const int32_t* __restrict__ sched,
                                                         int64_t n_sched) {
  __shared__ sim_c th[kMpsCols * kMpsCols];
  __shared__ double sig[kMpsCols];
  __shared__ int perm[kMpsCols];
  __shared__ int dims[kMpsMaxQubits + 2];
  __shared__ int flag;
  const int unit = (int)blockIdx.x, cl = unit / traj_count, tl = unit - cl * traj_count;
  const int run = FOLD ? min(max(circ_first + cl, 0), n_runs - 1) : 0;
  const int c = FOLD ? run % B : min(max(circ_first + cl, 0), B - 1), traj = traj_first + tl;
  const int row = FOLD ? run : c, rows = FOLD ? n_runs : B;   // of run_keys and traj_stats
  const int n = min(max(n_qubits[c], 1), max_q);
  const int tid = (int)threadIdx.x;
  char* base = workspace + (int64_t)unit * mps_unit_bytes(max_q, chi);
  MpsState st;
  st.A = reinterpret_cast<sim_c*>(base + mps_dims_bytes(max_q));
  st.S = 2 * chi * chi;
  st.stash = st.A + (int64_t)max_q * st.S;
  st.th = th;
  st.sig = sig;
  st.perm = perm;
  st.dims = dims;
  st.flag = &flag;
  st.chi = chi;
  st.tid = tid;
  st.lane = tid & (kWave - 1);
  st.wave = tid >> 6;
  st.cutoff = cutoff;
  st.discarded = 0.0;
  st.bound = 0.0;
  st.bond = 1;
  st.decompositions = 0;
  st.unconverged = 0;
  st.sweeps = 0;

  for (int q = tid; q <= n; q += kBlock) dims[q] = 1;
  for (int q = tid; q < n; q += kBlock) {   // |0>: (l, s, r) = (0, 0, 0) is 1, (0, 1, 0) is 0
    st.A[(int64_t)q * st.S] = sim_c{1.0, 0.0};
    st.A[(int64_t)q * st.S + chi] = sim_c{0.0, 0.0};
  }
  __syncthreads();

  const int64_t ob = min(max(op_ptr[c], (int64_t)0), n_ops), oe = min(max(op_ptr[c + 1], ob), n_ops);
  const int n_op = (int)min(oe - ob, (int64_t)0x7FFFFFFF);
  int64_t sb = 0;
  int n_step = n_op;   // steps this run takes: its records, or the entries of its schedule
  if (FOLD) {
    sb = min(max(sched_ptr[run], (int64_t)0), n_sched);
    const int64_t se = min(max(sched_ptr[run + 1], sb), n_sched);
    n_step = n_op > 0 ? (int)min(se - sb, (int64_t)0x7FFFFFFF) : 0;   // a circuit without records skips its entries
  }
  const int64_t key = run_keys[row];
  const uint32_t key_lo = (uint32_t)(uint64_t)key, key_hi = (uint32_t)((uint64_t)key >> 32);
  int centre = 0, noise_index = 0;
  int twirl_index = 0, twirl_code = 0;   // the TWIRL_CLOSE entries executed so far, the code of the latest TWIRL_OPEN: scalars
  for (int k = 0; k < n_step; ++k) {
    int at = k, dg = 0;   // dg: apply the record's conjugate transpose
    if (FOLD) {
      const int entry = __builtin_amdgcn_readfirstlane(sched[sb + k]);
      at = min(max(entry >> 1, 0), n_op - 1);
      dg = entry & 1;
    }
    const sim_i4 op = ops[ob + at];   // kind, site, orientation, offset into params
    const int kind = __builtin_amdgcn_readfirstlane(op.x);
    const int orient = __builtin_amdgcn_readfirstlane(op.z) & 1;
    const int64_t po = min((int64_t)max(op.w, 0), n_params - kSimParamPad);
    const double* m = params + po;
    if (kind == MLQEM_MPS_OP_U1 || kind == MLQEM_MPS_OP_DEPOL1) {
      const int q = __builtin_amdgcn_readfirstlane(min(max(op.y, 0), n - 1));
      if (kind == MLQEM_MPS_OP_U1) {
        if constexpr (FOLD) {   // the off-diagonal entries swapped and every imaginary part times -1 where daggered
          const int i01 = dg ? 4 : 2, i10 = dg ? 2 : 4;
          const double sg = dg ? -1.0 : 1.0;
          st.one_site(q, sim_c{m[0], sg * m[1]}, sim_c{m[i01], sg * m[i01 + 1]}, sim_c{m[i10], sg * m[i10 + 1]}, sim_c{m[6], sg * m[7]});
        } else {
          st.one_site(q, sim_c{m[0], m[1]}, sim_c{m[2], m[3]}, sim_c{m[4], m[5]}, sim_c{m[6], m[7]});
        }
      } else {
        st.pauli(q, mps_draw(noise_index, traj, key_lo, key_hi, seed_lo, seed_hi, false, m[0]));
        ++noise_index;
      }
    } else if ((kind == MLQEM_MPS_OP_U2 || kind == MLQEM_MPS_OP_DEPOL2) && n >= 2) {
      const int q = __builtin_amdgcn_readfirstlane(min(max(op.y, 0), n - 2));
      if (kind == MLQEM_MPS_OP_U2) {
        while (centre < q) {
          st.template bond_op<FOLD>(centre, nullptr, 0, false);
          ++centre;
        }
        while (centre > q) {
          st.template bond_op<FOLD>(centre - 1, nullptr, 0, true);
          --centre;
        }
        st.template bond_op<FOLD>(q, m, orient, false, dg);
        centre = q + 1;
      } else {
        const int code = mps_draw(noise_index, traj, key_lo, key_hi, seed_lo, seed_hi, true, m[0]);
        ++noise_index;
        st.pauli(orient ? q + 1 : q, code & 3);    // the letter of the gate's first qubit
        st.pauli(orient ? q : q + 1, code >> 2);   // and of its second
      }
    } else if ((kind == MLQEM_MPS_OP_TWIRL_OPEN || kind == MLQEM_MPS_OP_TWIRL_CLOSE) && n >= 2) {
      // a Pauli twirl around a gate and its noise: OPEN draws the pair, CLOSE applies its image under the ideal gate from the
      // record's table.  Kind, code and index are workgroup-uniform, so `pauli` (whose one_site ends in a barrier) is reached by
      // every thread alike; a dagger bit is ignored, no centre moves, nothing enters the certificate
      const int q = __builtin_amdgcn_readfirstlane(min(max(op.y, 0), n - 2));
      int code;
      if (kind == MLQEM_MPS_OP_TWIRL_OPEN) {
        code = twirl_code = mps_twirl_draw(twirl_index, traj, key_lo, key_hi, seed_lo, seed_hi);
      } else {
        code = __builtin_amdgcn_readfirstlane((int)fmin(fmax(m[twirl_code], 0.0), 15.0));   // a NaN entry: 0
        ++twirl_index;
      }
      st.pauli(orient ? q + 1 : q, code & 3);
      st.pauli(orient ? q : q + 1, code >> 2);
    } else if (kind == MLQEM_MPS_OP_NOISE1 || (kind == MLQEM_MPS_OP_NOISE2 && n >= 2)) {
      if constexpr (!FOLD) {   // the host refuses these kinds on folded runs: the folded kernel skips them as any unknown kind
        // the centre to site `to`, one site at a time: the two loops of a U2 record
        auto move_to = [&](int to) {
          while (centre < to) {
            st.template bond_op<false>(centre, nullptr, 0, false);
            ++centre;
          }
          while (centre > to) {
            st.template bond_op<false>(centre - 1, nullptr, 0, true);
            --centre;
          }
        };
        // one record, one noise index: the depolarising draw of DEPOL1 / DEPOL2 (sub-draw 0), then one relaxation per qubit.  On a
        // pair the SITE order follows the centre (the lower site first where the centre is at or below it, else the upper one:
        // after a U2 the centre is on the upper site, which then costs no move); the sub-draw and the triple follow the GATE's
        // qubit: the site q + orient is q0 (sub-draw 1, m[1 .. 3]), the other q1 (sub-draw 2, m[4 .. 6])
        const int two = kind == MLQEM_MPS_OP_NOISE2 ? 1 : 0;
        const int q = __builtin_amdgcn_readfirstlane(min(max(op.y, 0), n - 1 - two));
        const int code = mps_draw(noise_index, traj, key_lo, key_hi, seed_lo, seed_hi, two != 0, m[0]);
        st.pauli(two && orient ? q + 1 : q, code & 3);
        st.pauli(orient ? q : q + 1, two ? code >> 2 : 0);
        const int upper_first = two && centre > q ? 1 : 0;   // workgroup-uniform, as the centre is
#pragma unroll 1
        for (int step = 0; step <= two; ++step) {
          const int up = two ? step ^ upper_first : 0;   // this step's site is q + up
          const int second = two ? up ^ orient : 0;      // 0: the gate's q0, 1: its q1
          move_to(q + up);
          st.relax(q + up, m[1 + 3 * second], m[2 + 3 * second], m[3 + 3 * second],
                   mps_uniform(noise_index, 1 + second, traj, key_lo, key_hi, seed_lo, seed_hi));
        }
        ++noise_index;
      }
    }
  }
  int* gdims = reinterpret_cast<int*>(base);
  for (int q = tid; q <= n; q += kBlock) gdims[q] = dims[q];
  if (tid == 0) {
    double* out = traj_stats + ((int64_t)traj * rows + row) * kMpsStats;
    out[0] = st.discarded;
    out[1] = st.bound;
    out[2] = (double)st.bond;
    out[3] = (double)st.decompositions;
    out[4] = (double)st.unconverged;
    out[5] = (double)st.sweeps;
  }
}

// <psi|O|psi> by contracting left to right: E <- sum A[q]^dagger O_q A[q] E.  NORM: all-I operators, one workgroup per unit, writes
// traj_norm; else one workgroup per (unit, term), divides by the unit's norm.
template <bool NORM>
__global__ __launch_bounds__(kBlock) void mps_terms_kernel(int B, const int32_t* __restrict__ n_qubits, int circ_first, int circ_count,
                                                           int traj_first, int traj_count, int chi, int max_q,
                                                           const char* __restrict__ workspace, int64_t term_first, int64_t term_count,
                                                           int64_t n_terms, const int32_t* __restrict__ term_circ,
                                                           const int64_t* __restrict__ term_off, const uint8_t* __restrict__ letters,
                                                           int64_t n_letters, const int64_t* __restrict__ site_ptr,
                                                           const double* __restrict__ readout, int64_t n_sites, double* __restrict__ traj_terms,
                                                           double* __restrict__ traj_norm) {
  __shared__ sim_c E[kMpsMaxBond * kMpsMaxBond];
  __shared__ sim_c F[kMpsMaxBond * 2 * kMpsMaxBond];
  const int tid = (int)threadIdx.x;
  const int64_t per = NORM ? (int64_t)circ_count : term_count;
  const int tl = (int)((int64_t)blockIdx.x / per);
  const int64_t item = (int64_t)blockIdx.x - (int64_t)tl * per;
  const int64_t t = term_first + item;
  const int c = NORM ? min(max(circ_first + (int)item, 0), B - 1)
                     : min(max(term_circ[min(t, n_terms - 1)], circ_first), min(circ_first + circ_count, B) - 1);
  const int traj = traj_first + tl;
  const int unit = (c - circ_first) * traj_count + tl;
  const int n = min(max(n_qubits[c], 1), max_q);
  const char* base = workspace + (int64_t)unit * mps_unit_bytes(max_q, chi);
  const int* gdims = reinterpret_cast<const int*>(base);
  const sim_c* A = reinterpret_cast<const sim_c*>(base + mps_dims_bytes(max_q));
  const int S = 2 * chi * chi;
  const int64_t lo = NORM ? 0 : min(max(term_off[min(t, n_terms - 1)], (int64_t)0), max(n_letters - n, (int64_t)0));
  const int64_t sb = min(max(site_ptr[c], (int64_t)0), max(n_sites - n, (int64_t)0));
  if (tid == 0) E[0] = sim_c{1.0, 0.0};
  __syncthreads();
  for (int q = 0; q < n; ++q) {
    const int dl = min(max(gdims[q], 1), chi), dr = min(max(gdims[q + 1], 1), chi);
    const sim_c* a = A + (int64_t)q * S;
    const int letter = NORM ? 0 : (int)(letters[min(lo + q, n_letters - 1)] & 3);
    const int64_t sq = min(sb + q, n_sites - 1);
    const double ra = readout[2 * sq], rb = readout[2 * sq + 1];   // the Z slot of a measured qubit: a Z + b I
    const double z0 = ra + rb, z1 = rb - ra;
    for (int it = tid; it < dl * 2 * dr; it += kBlock) {   // F[l', s, r] = sum_l E[l', l] A[l, s, r]
      const int lp = it / (2 * dr), rem = it - lp * 2 * dr, s = rem / dr, r = rem - s * dr;
      sim_c acc{0.0, 0.0};
      for (int l = 0; l < dl; ++l) acc = cmac(acc, E[lp * kMpsMaxBond + l], a[(l * 2 + s) * chi + r]);
      F[(lp * 2 + s) * kMpsMaxBond + r] = acc;
    }
    __syncthreads();
    sim_c out[(kMpsMaxBond * kMpsMaxBond + kBlock - 1) / kBlock];
#pragma unroll
    for (int j = 0; j < (kMpsMaxBond * kMpsMaxBond + kBlock - 1) / kBlock; ++j) {   // E'[r', r] = sum conj(A[l', s', r']) (O F)[l', s', r]
      const int it = tid + j * kBlock;
      sim_c acc{0.0, 0.0};
      if (it < dr * dr) {
        const int rp = it / dr, r = it - rp * dr;
        for (int lp = 0; lp < dl; ++lp) {
          const sim_c f0 = F[(lp * 2) * kMpsMaxBond + r], f1 = F[(lp * 2 + 1) * kMpsMaxBond + r];
          sim_c g0 = f0, g1 = f1;
          if (letter == 1) {
            g0 = f1;
            g1 = f0;
          } else if (letter == 2) {   // Y = [[0, -i], [i, 0]]
            g0 = sim_c{f1.y, -f1.x};
            g1 = sim_c{-f0.y, f0.x};
          } else if (letter == 3) {
            g0 = z0 * f0;
            g1 = z1 * f1;
          }
          acc = cmac(acc, cconj(a[(lp * 2) * chi + rp]), g0);
          acc = cmac(acc, cconj(a[(lp * 2 + 1) * chi + rp]), g1);
        }
      }
      out[j] = acc;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < (kMpsMaxBond * kMpsMaxBond + kBlock - 1) / kBlock; ++j) {
      const int it = tid + j * kBlock;
      if (it < dr * dr) E[(it / dr) * kMpsMaxBond + (it - (it / dr) * dr)] = out[j];
    }
    __syncthreads();
  }
  if (tid == 0) {
    if (NORM) {
      traj_norm[(int64_t)traj * B + c] = E[0].x;
    } else {
      traj_terms[(int64_t)traj * n_terms + t] = E[0].x / traj_norm[(int64_t)traj * B + c];
    }
  }
}

// Means and standard errors over the trajectories, in trajectory order, from the functions mlqem_sim_run_trajectories_f64 forms
// them with (sim_ctx.hpp); the discarded weight and the certificate are means, the bond a maximum.
__global__ __launch_bounds__(kBlock) void mps_finish_kernel(int64_t B, int64_t n_terms, int T, const int64_t* __restrict__ term_ptr,
                                                            const double* __restrict__ coeff, const double* __restrict__ traj_terms,
                                                            const double* __restrict__ traj_norm, const double* __restrict__ traj_stats,
                                                            double* __restrict__ term_values, double* __restrict__ term_se,
                                                            double* __restrict__ values, double* __restrict__ se, double* __restrict__ norm,
                                                            double* __restrict__ discarded, double* __restrict__ error_bound,
                                                            int32_t* __restrict__ bond) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const double count = (double)T, pairs = (double)T * (double)(T - 1);
  if (i < n_terms) {
    const TrajStat s = traj_term_stats(traj_terms, n_terms, T, i);
    term_values[i] = s.mean;
    term_se[i] = s.se;
  }
  if (i < B) {
    const int64_t tb = min(max(term_ptr[i], (int64_t)0), n_terms), te = min(max(term_ptr[i + 1], tb), n_terms);
    double acc = 0.0, nacc = 0.0, dacc = 0.0, bacc = 0.0, m2 = 0.0, most = 1.0;
    for (int t = 0; t < T; ++t) {
      acc = acc + traj_value(coeff, traj_terms, n_terms, t, tb, te);
      nacc = nacc + traj_norm[(int64_t)t * B + i];
      const double* s = traj_stats + ((int64_t)t * B + i) * kMpsStats;
      dacc = dacc + s[0];
      bacc = bacc + s[1];
      most = fmax(most, s[2]);
    }
    const double mean = acc / count;
    for (int t = 0; t < T; ++t) {
      const double d = traj_value(coeff, traj_terms, n_terms, t, tb, te) - mean;
      m2 = __builtin_fma(d, d, m2);
    }
    values[i] = mean;
    se[i] = T > 1 ? sqrt(m2 / pairs) : 0.0;
    norm[i] = nacc / count;
    discarded[i] = dacc / count;
    error_bound[i] = bacc / count;
    bond[i] = (int32_t)fmin(most, (double)kMpsMaxBond);
  }
}

// ---- shots (mlqem_mps_sample_f64, mlqem_mps_sample_finish_f64) ------------------------------------------------------------------------
// Perfect sampling: the right environments once per unit, then one sweep over the sites per shot, each bit drawn from its
// conditional probability.  Nothing here relies on the gauge: the weights are formed against the environments.
constexpr int kMpsShotBlock = MLQEM_MPS_SHOT_BLOCK;                 // 16 shots a workgroup
constexpr int kMpsWaveShots = kMpsShotBlock / (kBlock / kWave);     // 4 of them a wave, in registers side by side
constexpr int kMpsMaxWords = (kMpsMaxQubits + 31) / 32;             // 16 words of packed bits a shot
static_assert(kMpsWaveShots * (kBlock / kWave) == kMpsShotBlock && kWave == 2 * kMpsMaxBond, "a lane per (s, r), four shots a wave");

__host__ __device__ inline int64_t mps_env_unit_bytes(int max_q, int chi) { return 16 * ((int64_t)max_q * 2 * chi * chi); }

// the value lane `from` (a constant) holds, as a scalar
template <int from> __device__ __forceinline__ double mps_lane(double v) {
  const uint64_t b = __builtin_bit_cast(uint64_t, v);
  const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)b, from), hi = __builtin_amdgcn_readlane((uint32_t)(b >> 32), from);
  return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}
// the sum over the lane's half of the wave (32 lanes), a butterfly in a fixed order: every lane of a half ends with the same bits
__device__ __forceinline__ double mps_half_sum(double v) {
#pragma unroll
  for (int d = kMpsMaxBond / 2; d >= 1; d >>= 1) v = v + __shfl_xor(v, d, kWave);
  return v;
}
__device__ __forceinline__ sim_c mps_other_half(sim_c v) { return sim_c{__shfl_xor(v.x, kMpsMaxBond, kWave), __shfl_xor(v.y, kMpsMaxBond, kWave)}; }
// the physical components (v0, v1) of a lane pair in the basis of `letter` (1 X: (v0 +- v1) c, 2 Y: (v0 -+ i v1) c); `mine` is the
// lane's own component, s its index
__device__ __forceinline__ sim_c mps_mix(sim_c mine, int s, int letter) {
  const sim_c other = mps_other_half(mine);
  const sim_c v0 = s ? other : mine, v1 = s ? mine : other;
  const sim_c w1 = letter == 2 ? sim_c{v1.y, -v1.x} : v1;   // -i v1 for Y
  const sim_c r = s ? v0 - w1 : v0 + w1;
  return 0.7071067811865476 * r;
}

// Right environments of one (circuit, trajectory) unit, a workgroup each, right to left: R[n] = [1], G[q][l, s, r'] = sum_r
// A[q][l, s, r] R[q + 1][r, r'] (written to `env` in the layout of the site tensors), R[q][l, l'] = sum_(s, r') G[q][l, s, r']
// conj(A[q][l', s, r']).  Every sum runs in index order.
__global__ __launch_bounds__(kBlock) void mps_env_kernel(int B, const int32_t* __restrict__ n_qubits, int circ_first, int traj_count, int chi,
                                                         int max_q, const char* __restrict__ workspace, char* __restrict__ env) {
  __shared__ sim_c R[kMpsMaxBond * kMpsMaxBond];
  __shared__ sim_c Gl[kMpsMaxBond * 2 * kMpsMaxBond];
  const int tid = (int)threadIdx.x, unit = (int)blockIdx.x, cl = unit / traj_count;
  const int c = min(max(circ_first + cl, 0), B - 1);
  const int n = min(max(n_qubits[c], 1), max_q);
  const char* base = workspace + (int64_t)unit * mps_unit_bytes(max_q, chi);
  const int* gdims = reinterpret_cast<const int*>(base);
  const sim_c* A = reinterpret_cast<const sim_c*>(base + mps_dims_bytes(max_q));
  sim_c* G = reinterpret_cast<sim_c*>(env + (int64_t)unit * mps_env_unit_bytes(max_q, chi));
  const int S = 2 * chi * chi;
  if (tid == 0) R[0] = sim_c{1.0, 0.0};
  __syncthreads();
  for (int q = n - 1; q >= 0; --q) {
    const int dl = min(max(gdims[q], 1), chi), dr = min(max(gdims[q + 1], 1), chi);
    const sim_c* a = A + (int64_t)q * S;
    sim_c* g = G + (int64_t)q * S;
    const int items = dl * 2 * dr;
    for (int it0 = 0; it0 < items; it0 += kBlock) {
      const int it = it0 + tid, ic = min(it, items - 1);
      const int row = ic / dr, rp = ic - row * dr;   // row = l * 2 + s
      sim_c acc{0.0, 0.0};
      for (int r = 0; r < dr; ++r) acc = cmac(acc, a[row * chi + r], R[r * kMpsMaxBond + rp]);
      if (it < items) {
        Gl[row * kMpsMaxBond + rp] = acc;
        g[row * chi + rp] = acc;
      }
    }
    __syncthreads();
    for (int it0 = 0; it0 < dl * dl; it0 += kBlock) {   // R is read above only: the barrier before this loop frees it
      const int it = it0 + tid, ic = min(it, dl * dl - 1);
      const int l = ic / dl, lp = ic - l * dl;
      sim_c acc{0.0, 0.0};
      for (int s = 0; s < 2; ++s)
        for (int rp = 0; rp < dr; ++rp) acc = cmac(acc, Gl[(l * 2 + s) * kMpsMaxBond + rp], cconj(a[(lp * 2 + s) * chi + rp]));
      if (it < dl * dl) R[l * kMpsMaxBond + lp] = acc;
    }
    __syncthreads();
  }
}

// One workgroup per (measurement group, trajectory of the chunk, block of kMpsShotBlock of that trajectory's shots).  The sites
// run in the outer loop: A[q] and G[q] are staged into LDS once for the block, then every wave advances its four shots, lane =
// (s, r): a = sum_l v[l] A[l, s, r], g = sum_l v[l] G[l, s, r], the basis letter mixes s, p_b = sum_r Re(g_b[r] conj(a_b[r])) over
// the lane's half, the draw of include/mlqem_hip.h, v <- a_b / sqrt(p_b).  v (a row of V per shot) is read and written by its own
// wave only.  A lane with r >= chi_r reads lane chi_r - 1's entries and adds nothing.
__global__ __launch_bounds__(kBlock) void mps_sample_kernel(
    int B, const int32_t* __restrict__ n_qubits, int circ_first, int circ_count, int traj_first, int traj_count, int T, int chi, int max_q,
    const char* __restrict__ workspace, const char* __restrict__ env, int64_t group_first, int64_t n_groups,
    const int64_t* __restrict__ group_ptr, const int32_t* __restrict__ group_circ, const int64_t* __restrict__ group_off,
    const uint8_t* __restrict__ basis, int64_t n_basis, const int64_t* __restrict__ site_ptr, const double* __restrict__ flip,
    int64_t n_sites, const int64_t* __restrict__ ref_ptr, const int64_t* __restrict__ gterm_ptr, const int32_t* __restrict__ gterm,
    int64_t n_terms, const int32_t* __restrict__ term_mask, const uint32_t* __restrict__ masks, int64_t n_masks,
    const int64_t* __restrict__ run_keys, int shots, int n_blocks, uint32_t seed_lo, uint32_t seed_hi, int32_t* __restrict__ term_sums,
    uint32_t* __restrict__ bits, int64_t n_bits) {
  __shared__ sim_c Al[kMpsMaxBond * 2 * kMpsMaxBond];
  __shared__ sim_c Gl[kMpsMaxBond * 2 * kMpsMaxBond];
  __shared__ sim_c V[kMpsShotBlock * kMpsMaxBond];
  __shared__ uint32_t words[kMpsShotBlock * kMpsMaxWords];
  const int tid = (int)threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  const int64_t rest = (int64_t)blockIdx.x / n_blocks;
  const int sb = (int)((int64_t)blockIdx.x - rest * n_blocks), tl = (int)(rest % traj_count);
  const int64_t g = min(max(group_first + rest / traj_count, (int64_t)0), n_groups - 1);
  const int c = min(max(group_circ[g], circ_first), min(circ_first + circ_count, B) - 1);
  const int traj = traj_first + tl, unit = (c - circ_first) * traj_count + tl;
  const int n = min(max(n_qubits[c], 1), max_q), W = (n + 31) >> 5;
  const int per = traj < shots ? (shots - traj + T - 1) / T : 0;   // the shots traj, traj + T, ... below `shots`
  const int first = sb * kMpsShotBlock, count = min(max(per - first, 0), kMpsShotBlock);
  if (count == 0) return;   // workgroup-uniform, before any barrier
  const uint32_t glocal = (uint32_t)(g - min(max(group_ptr[c], (int64_t)0), g)) & (MLQEM_MPS_MAX_GROUPS - 1);
  const int64_t key = run_keys[c];
  const uint32_t key_lo = (uint32_t)(uint64_t)key, key_hi = (uint32_t)((uint64_t)key >> 32);
  const int64_t lo = min(max(group_off[g], (int64_t)0), max(n_basis - n, (int64_t)0));
  const int64_t sbase = min(max(site_ptr[c], (int64_t)0), max(n_sites - n, (int64_t)0));
  const char* base = workspace + (int64_t)unit * mps_unit_bytes(max_q, chi);
  const int* gdims = reinterpret_cast<const int*>(base);
  const sim_c* A = reinterpret_cast<const sim_c*>(base + mps_dims_bytes(max_q));
  const sim_c* G = reinterpret_cast<const sim_c*>(env + (int64_t)unit * mps_env_unit_bytes(max_q, chi));
  const int S = 2 * chi * chi;
  const int s = lane >> 5, r = lane & (kMpsMaxBond - 1);
  if (tid < kMpsShotBlock) V[tid * kMpsMaxBond] = sim_c{1.0, 0.0};
  uint32_t word[kMpsWaveShots];
#pragma unroll
  for (int j = 0; j < kMpsWaveShots; ++j) word[j] = 0u;
  for (int q = 0; q < n; ++q) {
    const int dl = min(max(gdims[q], 1), chi), dr = min(max(gdims[q + 1], 1), chi);
    const sim_c* a = A + (int64_t)q * S;
    const sim_c* gq = G + (int64_t)q * S;
    __syncthreads();   // the last site's reads of Al and Gl are over (first site: V is set)
    for (int it = tid; it < dl * 2 * chi; it += kBlock) {
      Al[it] = a[it];
      Gl[it] = gq[it];
    }
    __syncthreads();
    const int letter = (int)(basis[min(lo + q, n_basis - 1)] & 3);
    const int64_t sq = min(sbase + q, n_sites - 1);
    const double flip0 = flip[2 * sq], flip1 = flip[2 * sq + 1];
    const bool live = r < dr;
    const int col = s * chi + min(r, dr - 1);
    sim_c av[kMpsWaveShots], gv[kMpsWaveShots];
#pragma unroll
    for (int j = 0; j < kMpsWaveShots; ++j) av[j] = gv[j] = sim_c{0.0, 0.0};
    for (int l = 0; l < dl; ++l) {
      const sim_c ae = Al[l * 2 * chi + col], ge = Gl[l * 2 * chi + col];
#pragma unroll
      for (int j = 0; j < kMpsWaveShots; ++j) {
        const sim_c v = V[(wave * kMpsWaveShots + j) * kMpsMaxBond + l];
        av[j] = cmac(av[j], v, ae);
        gv[j] = cmac(gv[j], v, ge);
      }
    }
    if (letter == 1 || letter == 2) {   // workgroup-uniform
#pragma unroll
      for (int j = 0; j < kMpsWaveShots; ++j) {
        av[j] = mps_mix(av[j], s, letter);
        gv[j] = mps_mix(gv[j], s, letter);
      }
    }
#pragma unroll
    for (int j = 0; j < kMpsWaveShots; ++j) {
      const double sum = mps_half_sum(live ? gv[j].x * av[j].x + gv[j].y * av[j].y : 0.0);
      const double p0 = mps_lane<0>(sum), p1 = mps_lane<kMpsMaxBond>(sum);
      const double w0 = p0 > 0.0 ? p0 : 0.0, w1 = p1 > 0.0 ? p1 : 0.0;   // a NaN weight counts as 0
      const int shot = traj + (first + wave * kMpsWaveShots + j) * T;
      uint32_t x[4];
      philox4x32_10(0x80000000u | (glocal << 9) | (uint32_t)q, (uint32_t)shot, key_lo, key_hi, seed_lo, seed_hi, x);
      const double u = ((double)(x[0] >> 5) * 67108864.0 + (double)(x[1] >> 6)) * 0x1p-53;
      const double u2 = ((double)(x[2] >> 5) * 67108864.0 + (double)(x[3] >> 6)) * 0x1p-53;
      const double target = u * (w0 + w1);
      const int b = __builtin_amdgcn_readfirstlane((target < w0 || !(w1 > 0.0)) ? 0 : 1);
      const uint32_t reported = (uint32_t)b ^ (u2 < (b ? flip1 : flip0) ? 1u : 0u);
      word[j] |= reported << (q & 31);
      const double root = sqrt(b ? p1 : p0);
      if (live && s == b) V[(wave * kMpsWaveShots + j) * kMpsMaxBond + r] = sim_c{av[j].x / root, av[j].y / root};
    }
    if ((q & 31) == 31 || q == n - 1) {
#pragma unroll
      for (int j = 0; j < kMpsWaveShots; ++j) {
        if (lane == 0) words[(wave * kMpsWaveShots + j) * kMpsMaxWords + (q >> 5)] = word[j];
        word[j] = 0u;
      }
    }
  }
  __syncthreads();
  const int64_t rb = min(max(ref_ptr[g], (int64_t)0), (int64_t)0x7FFFFFFF) * shots;
  if (bits != nullptr) {
    for (int it = tid; it < count * W; it += kBlock) {
      const int sh = it / W, w = it - sh * W;
      const int64_t at = rb + (int64_t)(traj + (first + sh) * T) * W + w;
      if (at < n_bits) bits[at] = words[sh * kMpsMaxWords + w];
    }
  }
  // S_t of the group's terms over the block's shots: one integer atomic per (term, block)
  const int64_t tb = min(max(gterm_ptr[g], (int64_t)0), n_terms), te = min(max(gterm_ptr[g + 1], tb), n_terms);
  for (int64_t i0 = tb; i0 < te; i0 += kBlock) {
    const int64_t i = i0 + tid;
    const int t = min(max(gterm[min(i, n_terms - 1)], 0), (int)(n_terms - 1));
    const int64_t tm = term_mask[t];
    int sum = 0;
    for (int sh = 0; sh < count; ++sh) {
      uint32_t par = 0u;
      for (int w = 0; w < W; ++w) par ^= words[sh * kMpsMaxWords + w] & masks[min(max(tm + w, (int64_t)0), n_masks - 1)];
      sum += 1 - 2 * (int)(__popc(par) & 1);
    }
    if (i < te) atomicAdd(&term_sums[t], sum);
  }
}

// term_values = S_t / shots, values and variance with the expressions of mlqem_sim_sample_f64 (sample_value_variance)
__global__ __launch_bounds__(kBlock) void mps_sample_finish_kernel(int64_t n_circuits, const int64_t* __restrict__ term_ptr,
                                                                   const double* __restrict__ coeff, int64_t n_terms,
                                                                   const int32_t* __restrict__ term_sums, int shots,
                                                                   double* __restrict__ term_values, double* __restrict__ values,
                                                                   double* __restrict__ variance) {
  const int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (c >= n_circuits) return;
  const int64_t tb = min(max(term_ptr[c], (int64_t)0), n_terms), te = min(max(term_ptr[c + 1], tb), n_terms);
  sample_value_variance(coeff, tb, te, values[c], variance[c], [&](int64_t t) {
    const double tv = (double)term_sums[t] / (double)shots;
    term_values[t] = tv;
    return tv;
  });
}

bool mps_shape_ok(int64_t n_circuits, int64_t circ_first, int64_t circ_count, int64_t traj_first, int64_t traj_count, int64_t trajectories,
                  int64_t max_bond, int64_t max_qubits) {
  return n_circuits >= 1 && circ_first >= 0 && circ_count >= 1 && circ_first + circ_count <= n_circuits && traj_first >= 0 &&
         traj_count >= 1 && traj_first + traj_count <= trajectories && trajectories <= MLQEM_SIM_MAX_TRAJECTORIES && max_bond >= 1 &&
         max_bond <= kMpsMaxBond && max_qubits >= 1 && max_qubits <= kMpsMaxQubits;
}

}  // namespace
}  // namespace mlqem

using namespace mlqem;

extern "C" size_t mlqem_mps_workspace_bytes(int64_t max_qubits, int64_t max_bond, int64_t n_units) {
  if (max_qubits < 1 || max_qubits > kMpsMaxQubits || max_bond < 1 || max_bond > kMpsMaxBond || n_units < 0) return 0;
  return (size_t)(mps_unit_bytes((int)max_qubits, (int)max_bond) * n_units);
}

extern "C" int mlqem_mps_run_f64(int64_t n_circuits, const int32_t* n_qubits, const int64_t* op_ptr, const mlqem_sim_op* ops, int64_t n_ops,
                                 const double* params, int64_t n_params, const int64_t* run_keys, int64_t circ_first, int64_t circ_count,
                                 int64_t traj_first, int64_t traj_count, int64_t trajectories, uint64_t seed, int64_t max_bond, double cutoff,
                                 int64_t max_qubits, void* workspace, size_t workspace_bytes, double* traj_stats, mlqem_stream_t stream) {
  begin_launches();
  if (n_circuits == 0) return MLQEM_OK;
  if (n_ops < 0 || n_params < kSimParamPad || !(cutoff >= 0.0) || !(cutoff < 1.0)) return MLQEM_ERR_BAD_ARG;
  if (!mps_shape_ok(n_circuits, circ_first, circ_count, traj_first, traj_count, trajectories, max_bond, max_qubits)) return MLQEM_ERR_BAD_ARG;
  if (n_circuits > 0x7FFFFFFFll || n_params > 0x7FFFFFFFll || circ_count * traj_count > 0x7FFFFFFFll) return MLQEM_ERR_UNSUPPORTED;
  if (!n_qubits || !op_ptr || !params || !run_keys || !workspace || !traj_stats || (n_ops > 0 && !ops)) return MLQEM_ERR_BAD_ARG;
  if (!aligned_to(ops, 16) || !aligned_to(workspace, 16) || !aligned_to(run_keys, 8)) return MLQEM_ERR_BAD_ARG;
  if (workspace_bytes < mlqem_mps_workspace_bytes(max_qubits, max_bond, circ_count * traj_count)) return MLQEM_ERR_WORKSPACE;
  hipLaunchKernelGGL((mps_run_kernel<false>), dim3((unsigned)(circ_count * traj_count)), dim3(kBlock), 0, as_stream(stream), (int)n_circuits,
                     n_qubits, op_ptr, reinterpret_cast<const sim_i4*>(ops), n_ops, params, n_params, run_keys, (int)circ_first,
                     (int)traj_first, (int)traj_count, (uint32_t)seed, (uint32_t)(seed >> 32), (int)max_bond, cutoff, (int)max_qubits,
                     static_cast<char*>(workspace), traj_stats, 0, (const int64_t*)nullptr, (const int32_t*)nullptr, (int64_t)0);
  return launch_status();
}

extern "C" int mlqem_mps_run_folded_f64(int64_t n_circuits, int64_t n_factors, const int32_t* n_qubits, const int64_t* op_ptr,
                                        const mlqem_sim_op* ops, int64_t n_ops, const double* params, int64_t n_params,
                                        const int64_t* sched_ptr, const int32_t* sched, int64_t n_sched, const int64_t* run_keys,
                                        int64_t run_first, int64_t run_count, int64_t traj_first, int64_t traj_count, int64_t trajectories,
                                        uint64_t seed, int64_t max_bond, double cutoff, int64_t max_qubits, void* workspace,
                                        size_t workspace_bytes, double* traj_stats, mlqem_stream_t stream) {
  begin_launches();
  if (n_circuits == 0) return MLQEM_OK;
  if (n_ops < 0 || n_params < kSimParamPad || n_sched < 0 || n_factors < 1 || n_circuits < 1 || !(cutoff >= 0.0) || !(cutoff < 1.0))
    return MLQEM_ERR_BAD_ARG;
  if (n_circuits > 0x7FFFFFFFll || n_factors > 0x7FFFFFFFll || n_circuits * n_factors > 0x7FFFFFFFll || n_params > 0x7FFFFFFFll ||
      n_sched > 0x7FFFFFFFll)
    return MLQEM_ERR_UNSUPPORTED;
  const int64_t n_runs = n_circuits * n_factors;
  if (!mps_shape_ok(n_runs, run_first, run_count, traj_first, traj_count, trajectories, max_bond, max_qubits)) return MLQEM_ERR_BAD_ARG;
  if (run_count * traj_count > 0x7FFFFFFFll) return MLQEM_ERR_UNSUPPORTED;
  if (!n_qubits || !op_ptr || !params || !sched_ptr || !run_keys || !workspace || !traj_stats || (n_ops > 0 && !ops) || (n_sched > 0 && !sched))
    return MLQEM_ERR_BAD_ARG;
  if (!aligned_to(ops, 16) || !aligned_to(workspace, 16) || !aligned_to(run_keys, 8) || !aligned_to(sched_ptr, 8) || !aligned_to(sched, 4))
    return MLQEM_ERR_BAD_ARG;
  if (workspace_bytes < mlqem_mps_workspace_bytes(max_qubits, max_bond, run_count * traj_count)) return MLQEM_ERR_WORKSPACE;
  hipLaunchKernelGGL((mps_run_kernel<true>), dim3((unsigned)(run_count * traj_count)), dim3(kBlock), 0, as_stream(stream), (int)n_circuits,
                     n_qubits, op_ptr, reinterpret_cast<const sim_i4*>(ops), n_ops, params, n_params, run_keys, (int)run_first,
                     (int)traj_first, (int)traj_count, (uint32_t)seed, (uint32_t)(seed >> 32), (int)max_bond, cutoff, (int)max_qubits,
                     static_cast<char*>(workspace), traj_stats, (int)n_runs, sched_ptr, sched, n_sched);
  return launch_status();
}

extern "C" int mlqem_mps_terms_f64(int64_t n_circuits, const int32_t* n_qubits, int64_t circ_first, int64_t circ_count, int64_t traj_first,
                                   int64_t traj_count, int64_t trajectories, int64_t max_bond, int64_t max_qubits, const void* workspace,
                                   size_t workspace_bytes, int64_t term_first, int64_t term_count, int64_t n_terms, const int32_t* term_circ,
                                   const int64_t* term_off, const uint8_t* letters, int64_t n_letters, const int64_t* site_ptr,
                                   const double* readout, int64_t n_sites, double* traj_term_values, double* traj_norm,
                                   mlqem_stream_t stream) {
  begin_launches();
  if (n_circuits == 0) return MLQEM_OK;
  if (!mps_shape_ok(n_circuits, circ_first, circ_count, traj_first, traj_count, trajectories, max_bond, max_qubits)) return MLQEM_ERR_BAD_ARG;
  if (term_first < 0 || term_count < 0 || n_terms < 0 || term_first + term_count > n_terms || n_letters < 0 || n_sites < 1)
    return MLQEM_ERR_BAD_ARG;
  if (n_circuits > 0x7FFFFFFFll || n_terms > 0x7FFFFFFFll || circ_count * traj_count > 0x7FFFFFFFll || term_count * traj_count > 0x7FFFFFFFll)
    return MLQEM_ERR_UNSUPPORTED;
  if (!n_qubits || !workspace || !site_ptr || !readout || !traj_norm ||
      (term_count > 0 && (!term_circ || !term_off || !letters || !traj_term_values || n_letters < 1)))
    return MLQEM_ERR_BAD_ARG;
  if (!aligned_to(workspace, 16)) return MLQEM_ERR_BAD_ARG;
  if (workspace_bytes < mlqem_mps_workspace_bytes(max_qubits, max_bond, circ_count * traj_count)) return MLQEM_ERR_WORKSPACE;
  const char* ws = static_cast<const char*>(workspace);
  hipLaunchKernelGGL((mps_terms_kernel<true>), dim3((unsigned)(circ_count * traj_count)), dim3(kBlock), 0, as_stream(stream), (int)n_circuits,
                     n_qubits, (int)circ_first, (int)circ_count, (int)traj_first, (int)traj_count, (int)max_bond, (int)max_qubits, ws,
                     term_first, term_count, n_terms, term_circ, term_off, letters, n_letters, site_ptr, readout, n_sites, traj_term_values,
                     traj_norm);
  if (term_count > 0) {
    hipLaunchKernelGGL((mps_terms_kernel<false>), dim3((unsigned)(term_count * traj_count)), dim3(kBlock), 0, as_stream(stream),
                       (int)n_circuits, n_qubits, (int)circ_first, (int)circ_count, (int)traj_first, (int)traj_count, (int)max_bond,
                       (int)max_qubits, ws, term_first, term_count, n_terms, term_circ, term_off, letters, n_letters, site_ptr, readout,
                       n_sites, traj_term_values, traj_norm);
  }
  return launch_status();
}

extern "C" int mlqem_mps_finish_f64(int64_t n_circuits, int64_t n_terms, int64_t trajectories, const int64_t* term_ptr, const double* coeff,
                                    const double* traj_term_values, const double* traj_norm, const double* traj_stats, double* term_values,
                                    double* term_std_error, double* values, double* std_error, double* norm, double* discarded,
                                    double* error_bound, int32_t* bond, mlqem_stream_t stream) {
  begin_launches();
  if (n_circuits < 0 || n_terms < 0 || trajectories < 1 || trajectories > MLQEM_SIM_MAX_TRAJECTORIES) return MLQEM_ERR_BAD_ARG;
  if (n_circuits > 0x7FFFFFFFll || n_terms > 0x7FFFFFFFll) return MLQEM_ERR_UNSUPPORTED;
  if (n_circuits == 0) return MLQEM_OK;
  if (!term_ptr || !traj_norm || !traj_stats || !values || !std_error || !norm || !discarded || !error_bound || !bond ||
      (n_terms > 0 && (!coeff || !traj_term_values || !term_values || !term_std_error)))
    return MLQEM_ERR_BAD_ARG;
  const int64_t rows = n_circuits > n_terms ? n_circuits : n_terms;
  hipLaunchKernelGGL(mps_finish_kernel, dim3((unsigned)ceil_div(rows, (int64_t)kBlock)), dim3(kBlock), 0, as_stream(stream), n_circuits, n_terms,
                     (int)trajectories, term_ptr, coeff, traj_term_values, traj_norm, traj_stats, term_values, term_std_error, values,
                     std_error, norm, discarded, error_bound, bond);
  return launch_status();
}

extern "C" size_t mlqem_mps_sample_workspace_bytes(int64_t max_qubits, int64_t max_bond, int64_t n_units) {
  if (max_qubits < 1 || max_qubits > kMpsMaxQubits || max_bond < 1 || max_bond > kMpsMaxBond || n_units < 0) return 0;
  return (size_t)(mps_env_unit_bytes((int)max_qubits, (int)max_bond) * n_units);
}

extern "C" int mlqem_mps_sample_f64(int64_t n_circuits, const int32_t* n_qubits, int64_t circ_first, int64_t circ_count, int64_t traj_first,
                                    int64_t traj_count, int64_t trajectories, int64_t max_bond, int64_t max_qubits, const void* workspace,
                                    size_t workspace_bytes, void* sample_workspace, size_t sample_workspace_bytes, int64_t group_first,
                                    int64_t group_count, int64_t n_groups, int64_t max_groups, const int64_t* group_ptr,
                                    const int32_t* group_circ, const int64_t* group_off, const uint8_t* basis, int64_t n_basis,
                                    const int64_t* site_ptr, const double* flip, int64_t n_sites, const int64_t* ref_ptr,
                                    const int64_t* gterm_ptr, const int32_t* gterm, int64_t term_first, int64_t term_count, int64_t n_terms,
                                    const int32_t* term_mask, const uint32_t* masks, int64_t n_masks, const int64_t* run_keys, int64_t shots,
                                    uint64_t seed, int32_t* term_sums, uint32_t* bits, int64_t n_bits, mlqem_stream_t stream) {
  begin_launches();
  if (n_circuits == 0) return MLQEM_OK;
  if (shots < 1 || shots > MLQEM_SIM_MAX_SHOTS) return MLQEM_ERR_BAD_ARG;
  if (!mps_shape_ok(n_circuits, circ_first, circ_count, traj_first, traj_count, trajectories, max_bond, max_qubits)) return MLQEM_ERR_BAD_ARG;
  if (group_first < 0 || group_count < 1 || n_groups < 1 || group_first + group_count > n_groups || max_groups < 1 || n_basis < 1 ||
      n_sites < 1 || term_first < 0 || term_count < 0 || n_terms < 0 || term_first + term_count > n_terms || n_masks < 0 || n_bits < 0)
    return MLQEM_ERR_BAD_ARG;
  if (max_groups > MLQEM_MPS_MAX_GROUPS) return MLQEM_ERR_UNSUPPORTED;
  const int64_t per = (shots + trajectories - 1) / trajectories, n_blocks = (per + kMpsShotBlock - 1) / kMpsShotBlock;
  if (n_circuits > 0x7FFFFFFFll || n_groups > 0x7FFFFFFFll || n_terms > 0x7FFFFFFFll || n_masks > 0x7FFFFFFFll ||
      circ_count * traj_count > 0x7FFFFFFFll || group_count > 0x7FFFFFFFll / (traj_count * n_blocks))
    return MLQEM_ERR_UNSUPPORTED;
  if (!n_qubits || !workspace || !sample_workspace || !group_ptr || !group_circ || !group_off || !basis || !site_ptr || !flip || !ref_ptr ||
      !gterm_ptr || !run_keys || (n_terms > 0 && (!gterm || !term_mask || !masks || !term_sums || n_masks < 1)) || (n_bits > 0 && !bits))
    return MLQEM_ERR_BAD_ARG;
  if (!aligned_to(workspace, 16) || !aligned_to(sample_workspace, 16) || !aligned_to(run_keys, 8) || !aligned_to(flip, 8))
    return MLQEM_ERR_BAD_ARG;
  const int64_t units = circ_count * traj_count;
  if (workspace_bytes < mlqem_mps_workspace_bytes(max_qubits, max_bond, units) ||
      sample_workspace_bytes < mlqem_mps_sample_workspace_bytes(max_qubits, max_bond, units))
    return MLQEM_ERR_WORKSPACE;
  const hipStream_t st = as_stream(stream);
  const char* ws = static_cast<const char*>(workspace);
  char* env = static_cast<char*>(sample_workspace);
  // the chunk that holds a circuit's first trajectories zeroes its sums; the chunks of its other trajectories add to them
  if (traj_first == 0 && term_count > 0 &&
      hipMemsetAsync(term_sums + term_first, 0, (size_t)term_count * sizeof(int32_t), st) != hipSuccess)
    return MLQEM_ERR_LAUNCH;
  hipLaunchKernelGGL(mps_env_kernel, dim3((unsigned)units), dim3(kBlock), 0, st, (int)n_circuits, n_qubits, (int)circ_first, (int)traj_count,
                     (int)max_bond, (int)max_qubits, ws, env);
  hipLaunchKernelGGL(mps_sample_kernel, dim3((unsigned)(group_count * traj_count * n_blocks)), dim3(kBlock), 0, st, (int)n_circuits, n_qubits,
                     (int)circ_first, (int)circ_count, (int)traj_first, (int)traj_count, (int)trajectories, (int)max_bond, (int)max_qubits, ws,
                     env, group_first, n_groups, group_ptr, group_circ, group_off, basis, n_basis, site_ptr, flip, n_sites, ref_ptr, gterm_ptr,
                     gterm, n_terms, term_mask, masks, n_masks, run_keys, (int)shots, (int)n_blocks, (uint32_t)seed, (uint32_t)(seed >> 32),
                     term_sums, n_bits > 0 ? bits : nullptr, n_bits);
  return launch_status();
}

extern "C" int mlqem_mps_sample_finish_f64(int64_t n_circuits, int64_t n_terms, int64_t shots, const int64_t* term_ptr, const double* coeff,
                                           const int32_t* term_sums, double* term_values, double* values, double* variance,
                                           mlqem_stream_t stream) {
  begin_launches();
  if (n_circuits < 0 || n_terms < 0 || shots < 1 || shots > MLQEM_SIM_MAX_SHOTS) return MLQEM_ERR_BAD_ARG;
  if (n_circuits > 0x7FFFFFFFll || n_terms > 0x7FFFFFFFll) return MLQEM_ERR_UNSUPPORTED;
  if (n_circuits == 0) return MLQEM_OK;
  if (!term_ptr || !values || !variance || (n_terms > 0 && (!coeff || !term_sums || !term_values))) return MLQEM_ERR_BAD_ARG;
  hipLaunchKernelGGL(mps_sample_finish_kernel, dim3((unsigned)ceil_div(n_circuits, (int64_t)kBlock)), dim3(kBlock), 0, as_stream(stream),
                     n_circuits, term_ptr, coeff, n_terms, term_sums, (int)shots, term_values, values, variance);
  return launch_status();
}
