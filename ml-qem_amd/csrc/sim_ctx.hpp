// What the simulator's kernels share (sim.hip: exact runs, folded runs, measurement shots; sim_bound.hip: runs of templates;
// sim_traj.hip: quantum trajectories; the finish kernels of mps.hip and clifford_frames.hip).  sim.hip's header comment states the
// rules of a pass.  Here lives the ONE copy of
//   the LDS state's types, the passes of SimCtx and its unit prologue (SimCtx::begin),
//   the record decode (sim_decode), the <psi|psi> / Tr rho pass (sim_norm) and the switch over the fixed record kinds
//   (sim_apply_fixed): sim_kernel and bound_kernel call them; traj_kernel keeps its own text of all four, which was faster
//   (DESIGN.md 3.13), and the term loop stays in each kernel (see the note below the switch),
//   a term's mean and standard error over trajectories and a trajectory's value (traj_term_stats, traj_value: traj_finish_kernel,
//   mps_finish_kernel, which keep their own two passes over the trajectories around traj_value, with their other sums in them) and
//   the value / variance sums of sampled runs (sample_value_variance: sample_finish_kernel, frames_finish_kernel),
//   the Philox4x32-10 generator,
//   and, for the host side of the entry points, the checks of a lowered batch's arguments (sim_batch_sizes, sim_batch_buffers) and the
//   wave-grid / workgroup-grid launch pair (sim_launch_pair).
// A record kind or a pass added to the switch reaches sim_kernel and bound_kernel: bound_kernel's promise of sim_kernel's bits for
// a template without parameterised records rests on both calling the same text (and on its copy of the term loop).  Everything here is in an unnamed namespace, so each
// translation unit has its own copy.
#pragma once
#include "common.hpp"

#include <type_traits>

namespace mlqem {
namespace {

constexpr int kSimWaveAmps = MLQEM_SIM_WAVE_AMPS;   // 256: a wave's slice
constexpr int kSimMaxAmps = MLQEM_SIM_MAX_AMPS;     // 2048: a workgroup's state, 32 KB
constexpr int kSimParamPad = 32;                    // doubles the longest record reads (a 4x4 complex matrix)

typedef double sim_c __attribute__((ext_vector_type(2)));   // (re, im): one 16-byte LDS access
typedef int sim_i4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ sim_c cmul(sim_c a, sim_c b) { return sim_c{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
__device__ __forceinline__ sim_c cmac(sim_c acc, sim_c a, sim_c b) {
  return sim_c{acc.x + (a.x * b.x - a.y * b.y), acc.y + (a.x * b.y + a.y * b.x)};
}
// index g with a zero bit inserted at position b
__device__ __forceinline__ int insert0(int g, int b) { return ((g >> b) << (b + 1)) | (g & ((1 << b) - 1)); }

template <bool WG> __device__ __forceinline__ void sim_sync() {
  if (WG) {
    __syncthreads();
  } else {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
}

__device__ __forceinline__ double sim_wave_sum(double v) {
#pragma unroll
  for (int d = kWave / 2; d >= 1; d >>= 1) v = v + __shfl_down(v, d, kWave);
  return v;
}

template <bool WG> struct SimCtx {
  static constexpr int T = WG ? kBlock : kWave;   // threads on one circuit
  sim_c* st;
  double* red;   // [2][4] wave sums of the workgroup variant
  int tid, nbits, A;

  // The unit's number: the workgroup's (WG), or four waves a workgroup with the wave's own 4 KB slice of `state`.  The number is
  // wave-uniform, so a kernel may return on it for a wave of a partly filled workgroup: the wave variant has no workgroup barrier.
  __device__ __forceinline__ int begin(sim_c* state, double* red8) {
    const int slot = WG ? (int)blockIdx.x : __builtin_amdgcn_readfirstlane((int)blockIdx.x * (kBlock / kWave) + ((int)threadIdx.x >> 6));
    tid = WG ? (int)threadIdx.x : (int)threadIdx.x & (kWave - 1);
    st = WG ? state : state + ((int)threadIdx.x >> 6) * kSimWaveAmps;
    red = red8;
    return slot;
  }

  // a 2x2 matrix on bit b of the first `bits` index bits; the entry of index i sits at i * mul, which lets the readout op walk the
  // diagonal of a density matrix (mul = 1 + 2^n) with the same code
  __device__ __forceinline__ void pair(int bits, int b, sim_c m00, sim_c m01, sim_c m10, sim_c m11, int mul) {
    const int np = (1 << bits) >> 1;
    for (int p0 = 0; p0 < np; p0 += T) {
      const int p = p0 + tid;
      const bool live = p < np;
      const int i0 = (insert0(min(p, np - 1), b) * mul) & (A - 1), i1 = (i0 | ((1 << b) * mul)) & (A - 1);
      const sim_c a0 = st[i0], a1 = st[i1];
      const sim_c r0 = cmac(cmul(m00, a0), m01, a1), r1 = cmac(cmul(m10, a0), m11, a1);
      if (live) {
        st[i0] = r0;
        st[i1] = r1;
      }
    }
    sim_sync<WG>();
  }

  // a 4x4 matrix on bits (a, b), basis index = bit a + 2 bit b; `tr` reads the record transposed (with conj: its inverse)
  __device__ __forceinline__ void quad(int a, int b, const double* m, bool conj, bool tr = false) {
    const double s = conj ? -1.0 : 1.0;
    const int rs = tr ? 2 : 8, cs = tr ? 8 : 2;   // strides of a row and of a column in the record
    const int lo = min(a, b), hi = max(a, b), ng = A >> 2;
    for (int g0 = 0; g0 < ng; g0 += T) {
      const int g = g0 + tid;
      const bool live = g < ng;
      const int base = insert0(insert0(min(g, ng - 1), lo), hi);
      int idx[4];
      sim_c e[4], r[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        idx[k] = (base | ((k & 1) << a) | ((k >> 1) << b)) & (A - 1);
        e[k] = st[idx[k]];
      }
#pragma unroll
      for (int row = 0; row < 4; ++row) {
        r[row] = cmul(sim_c{m[rs * row], s * m[rs * row + 1]}, e[0]);
#pragma unroll
        for (int col = 1; col < 4; ++col) r[row] = cmac(r[row], sim_c{m[rs * row + cs * col], s * m[rs * row + cs * col + 1]}, e[col]);
      }
      if (live) {
#pragma unroll
        for (int k = 0; k < 4; ++k) st[idx[k]] = r[k];
      }
    }
    sim_sync<WG>();
  }

  // entry i times f(i)
  template <class F> __device__ __forceinline__ void element(F&& factor) {
    for (int i0 = 0; i0 < A; i0 += T) {
      const int i = i0 + tid;
      const bool live = i < A;
      const int ic = i & (A - 1);
      const sim_c v = cmul(st[ic], factor(ic));
      if (live) st[ic] = v;
    }
    sim_sync<WG>();
  }

  // state[i] = old state[perm(i)]
  template <class F> __device__ __forceinline__ void gather(F&& perm) {
    constexpr int kMax = (WG ? kSimMaxAmps : kSimWaveAmps) / T;
    sim_c v[kMax];
#pragma unroll
    for (int k = 0; k < kMax; ++k) v[k] = st[perm((k * T + tid) & (A - 1)) & (A - 1)];
    sim_sync<WG>();
#pragma unroll
    for (int k = 0; k < kMax; ++k)
      if (k * T + tid < A) st[k * T + tid] = v[k];
    sim_sync<WG>();
  }

  // rho -> (1 - lam) rho + lam Tr_q(rho) (x) I/2 on qubit q of an n-qubit density matrix
  __device__ __forceinline__ void depol1(int n, int q, double lam) {
    const int ng = A >> 2, cb = q + n;
    const double keep = 1.0 - lam, mix = 0.5 * lam;
    for (int g0 = 0; g0 < ng; g0 += T) {
      const int g = g0 + tid;
      const bool live = g < ng;
      const int base = insert0(insert0(min(g, ng - 1), q), cb);
      const int i00 = base & (A - 1), i10 = (base | (1 << q)) & (A - 1), i01 = (base | (1 << cb)) & (A - 1),
                i11 = (base | (1 << q) | (1 << cb)) & (A - 1);
      const sim_c e00 = st[i00], e10 = st[i10], e01 = st[i01], e11 = st[i11];
      const sim_c tr = e00 + e11;
      if (live) {
        st[i00] = keep * e00 + mix * tr;
        st[i10] = keep * e10;
        st[i01] = keep * e01;
        st[i11] = keep * e11 + mix * tr;
      }
    }
    sim_sync<WG>();
  }

  // the same over the pair (a, b): 4 x 4 blocks, the four diagonal entries share their sum
  __device__ __forceinline__ void depol2(int n, int a, int b, double lam) {
    const int lo = min(a, b), hi = max(a, b), ng = A >> 4;
    const double keep = 1.0 - lam, mix = 0.25 * lam;
    for (int g0 = 0; g0 < ng; g0 += T) {
      const int g = g0 + tid;
      const bool live = g < ng;
      const int base = insert0(insert0(insert0(insert0(min(g, max(ng - 1, 0)), lo), hi), lo + n), hi + n);
      int idx[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const int r = k & 3, c = k >> 2;
        idx[k] = (base | ((r & 1) << lo) | ((r >> 1) << hi) | ((c & 1) << (lo + n)) | ((c >> 1) << (hi + n))) & (A - 1);
      }
      const sim_c tr = ((st[idx[0]] + st[idx[5]]) + st[idx[10]]) + st[idx[15]];
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        sim_c v = keep * st[idx[k]];
        if ((k & 3) == (k >> 2)) v = v + mix * tr;
        if (live) st[idx[k]] = v;
      }
    }
    sim_sync<WG>();
  }

  // thermal relaxation of one qubit on the two diagonal entries (a = rho_00, b = rho_11) of its 2x2 block: the population g of the
  // block's trace is reset, 1 - p1 of it to |0> and p1 to |1>.  g = 0 multiplies by 1.0 and adds 0.0 * tr: an exact identity.
  template <class V> static __device__ __forceinline__ void relax_diag(V& a, V& b, double stay, double to0, double to1) {
    const V tr = a + b;
    a = stay * a + to0 * tr;
    b = stay * b + to1 * tr;
  }

  // one fused noise record on qubit q: depol1's closed form with lam, then relaxation (g, c, p1) of the same 2x2 block -- the
  // diagonal through relax_diag, the two coherences times c.  One read and one write of the state.
  __device__ __forceinline__ void noise1(int n, int q, double lam, double g, double c, double p1) {
    const int ng = A >> 2, cb = q + n;
    const double keep = 1.0 - lam, mix = 0.5 * lam, stay = 1.0 - g, to0 = g * (1.0 - p1), to1 = g * p1;
    for (int g0 = 0; g0 < ng; g0 += T) {
      const int gi = g0 + tid;
      const bool live = gi < ng;
      const int base = insert0(insert0(min(gi, ng - 1), q), cb);
      const int i00 = base & (A - 1), i10 = (base | (1 << q)) & (A - 1), i01 = (base | (1 << cb)) & (A - 1),
                i11 = (base | (1 << q) | (1 << cb)) & (A - 1);
      const sim_c e00 = st[i00], e10 = st[i10], e01 = st[i01], e11 = st[i11];
      const sim_c tr = e00 + e11;
      sim_c d00 = keep * e00 + mix * tr, d11 = keep * e11 + mix * tr;
      relax_diag(d00, d11, stay, to0, to1);
      if (live) {
        st[i00] = d00;
        st[i10] = c * (keep * e10);
        st[i01] = c * (keep * e01);
        st[i11] = d11;
      }
    }
    sim_sync<WG>();
  }

  // the same over the gate's pair: depol2's closed form with lam, then relaxation (g, c, p1) of qubit a (m[1..3]) and of qubit b
  // (m[4..6]).  Relaxation of one qubit acts inside a fixed value of the other qubit's row and column bits, and it mixes two
  // entries only where its own row and column bit agree (the populations); where they differ (the coherences) it scales.  So the
  // 16 entries (ra, rb, ca, cb) of a 4 x 4 block fall into four parts of four that never meet, by whether a's bits agree and
  // whether b's do, and a thread takes one PART, not one block: four entries x[ja + 2 jb] in registers, as in noise1, and every
  // lane busy.  In a part the step along ja is relax_diag -- with (1 - g, g (1 - p1), g p1) where a's bits agree and with
  // (c, 0, 0) where they differ (c x + 0.0 * tr: the scaling) -- and the same along jb.  Only the part where both agree holds the
  // block's diagonal: its own four entries are the trace, and the other parts add 0.0 times theirs.  Every entry is read once
  // and written once by the thread that owns it.
  __device__ __forceinline__ void noise2(int n, int a, int b, const double* m) {
    const int lo = min(a, b), hi = max(a, b), nu = A >> 2;   // units: (block, part)
    const int ra = 1 << a, rb = 1 << b, ca = 1 << (a + n), cb = 1 << (b + n);
    for (int u0 = 0; u0 < nu; u0 += T) {
      const int u = u0 + tid;
      const bool live = u < nu;
      const int uc = min(u, max(nu - 1, 0));
      const bool off_a = uc & 1, off_b = uc & 2;   // the part: a's (b's) row and column bit differ
      const int base = insert0(insert0(insert0(insert0(uc >> 2, lo), hi), lo + n), hi + n);
      int idx[4];
      sim_c x[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int ja = k & 1, jb = k >> 1;
        const int bits_a = off_a ? (ja ? ca : ra) : (ja ? ra | ca : 0), bits_b = off_b ? (jb ? cb : rb) : (jb ? rb | cb : 0);
        idx[k] = (base | bits_a | bits_b) & (A - 1);
        x[k] = st[idx[k]];
      }
      const double lam = m[0], keep = 1.0 - lam, mix = off_a || off_b ? 0.0 : 0.25 * lam;
      const double ga = m[1], stay_a = off_a ? m[2] : 1.0 - ga, to1_a = off_a ? 0.0 : ga * m[3], to0_a = off_a ? 0.0 : ga * (1.0 - m[3]);
      const double gb = m[4], stay_b = off_b ? m[5] : 1.0 - gb, to1_b = off_b ? 0.0 : gb * m[6], to0_b = off_b ? 0.0 : gb * (1.0 - m[6]);
      // the maps are real: the real parts, then the imaginary parts, each four doubles updated in place
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        double v0 = h ? x[0].y : x[0].x, v1 = h ? x[1].y : x[1].x, v2 = h ? x[2].y : x[2].x, v3 = h ? x[3].y : x[3].x;
        const double tr = ((v0 + v1) + v2) + v3;
        v0 = keep * v0 + mix * tr;
        v1 = keep * v1 + mix * tr;
        v2 = keep * v2 + mix * tr;
        v3 = keep * v3 + mix * tr;
        relax_diag(v0, v1, stay_a, to0_a, to1_a);
        relax_diag(v2, v3, stay_a, to0_a, to1_a);
        relax_diag(v0, v2, stay_b, to0_b, to1_b);
        relax_diag(v1, v3, stay_b, to0_b, to1_b);
        if (h) {
          x[0].y = v0, x[1].y = v1, x[2].y = v2, x[3].y = v3;
        } else {
          x[0].x = v0, x[1].x = v1, x[2].x = v2, x[3].x = v3;
        }
      }
      if (live) {
#pragma unroll
        for (int k = 0; k < 4; ++k) st[idx[k]] = x[k];
      }
    }
    sim_sync<WG>();
  }

  // fixed-order sum of one double per thread: a shuffle tree, then wave 0 .. 3 in order.  Thread 0 holds the result (every thread of
  // the workgroup variant does).  `slot` alternates between two sets of wave sums, so one barrier per reduction is enough.
  __device__ __forceinline__ double reduce(double part, int slot) {
    const double w = sim_wave_sum(part);
    if (!WG) return w;
    if ((tid & (kWave - 1)) == 0) red[slot * 4 + (tid >> 6)] = w;
    __syncthreads();
    return ((red[slot * 4] + red[slot * 4 + 1]) + red[slot * 4 + 2]) + red[slot * 4 + 3];
  }
};

// One record, decoded: kind, q0, q1 (clamped to the circuit's qubits) and its values in the pool (the offset clamped so that the
// longest record stays inside the padding).  All four are wave-uniform.
struct SimRec {
  int kind, q0, q1;
  const double* m;
};

__device__ __forceinline__ SimRec sim_decode(const sim_i4 op, int n, const double* __restrict__ params, int64_t n_params) {
  const int kind = __builtin_amdgcn_readfirstlane(op.x);
  const int q0 = __builtin_amdgcn_readfirstlane(min(max(op.y, 0), n - 1)), q1 = __builtin_amdgcn_readfirstlane(min(max(op.z, 0), n - 1));
  const int64_t po = min((int64_t)max(op.w, 0), n_params - kSimParamPad);
  return SimRec{kind, q0, q1, params + po};
}

// <psi|psi> or Tr rho, reduced in the fixed order through slot 0 of `red`: the caller of the workgroup variant follows it with a
// barrier before red[0..3] is written again
template <bool WG> __device__ __forceinline__ double sim_norm(SimCtx<WG>& cx, int n, bool density) {
  const int A = cx.A, tid = cx.tid;
  double part = 0.0;
  const int cnt = density ? 1 << n : A, mul = density ? (1 << n) + 1 : 1;
  for (int i0 = 0; i0 < cnt; i0 += cx.T) {
    const int i = i0 + tid;
    const sim_c v = cx.st[((i & (cnt - 1)) * mul) & (A - 1)];
    const double add = density ? v.x : v.x * v.x + v.y * v.y;
    part = part + (i < cnt ? add : 0.0);
  }
  return cx.reduce(part, 0);
}

// The fixed record kinds (U1 .. NOISE2) as passes over the state; `dg` applies the record's inverse (folded runs, FOLD = true).
// A caller that passes `density = false` or `dg = false` as a literal compiles without the branches they guard.
template <bool FOLD, bool WG> __device__ __forceinline__ void sim_apply_fixed(SimCtx<WG>& cx, const SimRec& rec, int n, bool density, bool dg) {
  const int nbits = cx.nbits, kind = rec.kind, q0 = rec.q0, q1 = rec.q1;
  const double* m = rec.m;
  switch (kind) {
    case MLQEM_SIM_OP_U1:
      if (FOLD) {   // the inverse swaps the off-diagonal entries and negates the imaginary parts: no arithmetic, no rounding
        const int o01 = dg ? 4 : 2, o10 = dg ? 2 : 4;
        const sim_c u00{m[0], dg ? -m[1] : m[1]}, u01{m[o01], dg ? -m[o01 + 1] : m[o01 + 1]},
            u10{m[o10], dg ? -m[o10 + 1] : m[o10 + 1]}, u11{m[6], dg ? -m[7] : m[7]};
        cx.pair(nbits, q0, u00, u01, u10, u11, 1);
        if (density) cx.pair(nbits, q0 + n, sim_c{u00.x, -u00.y}, sim_c{u01.x, -u01.y}, sim_c{u10.x, -u10.y}, sim_c{u11.x, -u11.y}, 1);
        break;
      }
      cx.pair(nbits, q0, sim_c{m[0], m[1]}, sim_c{m[2], m[3]}, sim_c{m[4], m[5]}, sim_c{m[6], m[7]}, 1);
      if (density) cx.pair(nbits, q0 + n, sim_c{m[0], -m[1]}, sim_c{m[2], -m[3]}, sim_c{m[4], -m[5]}, sim_c{m[6], -m[7]}, 1);
      break;
    case MLQEM_SIM_OP_DIAG1: {
      const sim_c d0{m[0], dg ? -m[1] : m[1]}, d1{m[2], dg ? -m[3] : m[3]};
      if (density) {
        cx.element([&](int i) {   // d[row bit] conj(d[column bit])
          const bool r = (i >> q0) & 1, cc = (i >> (q0 + n)) & 1;
          return cmul(sim_c{r ? d1.x : d0.x, r ? d1.y : d0.y}, sim_c{cc ? d1.x : d0.x, cc ? -d1.y : -d0.y});
        });
      } else {
        cx.element([&](int i) { return (i >> q0) & 1 ? d1 : d0; });
      }
      break;
    }
    case MLQEM_SIM_OP_CZ: {
      const int mrow = (1 << q0) | (1 << q1), mcol = density ? mrow << n : 0;
      cx.element([&](int i) {
        const bool neg = ((i & mrow) == mrow) != (density && (i & mcol) == mcol);
        return sim_c{neg ? -1.0 : 1.0, 0.0};
      });
      break;
    }
    case MLQEM_SIM_OP_CX:
      cx.gather([&](int i) {
        int j = i ^ (((i >> q0) & 1) << q1);
        if (density) j ^= ((i >> (q0 + n)) & 1) << (q1 + n);
        return j;
      });
      break;
    case MLQEM_SIM_OP_SWAP:
      cx.gather([&](int i) {
        int j = i ^ ((((i >> q0) ^ (i >> q1)) & 1) * ((1 << q0) | (1 << q1)));
        if (density) j ^= (((i >> (q0 + n)) ^ (i >> (q1 + n))) & 1) * (((1 << q0) | (1 << q1)) << n);
        return j;
      });
      break;
    case MLQEM_SIM_OP_U2:
      cx.quad(q0, q1, m, dg, dg);   // the inverse: the record read transposed and conjugated
      if (density) cx.quad(q0 + n, q1 + n, m, !dg, dg);
      break;
    case MLQEM_SIM_OP_DEPOL1:
      if (density) cx.depol1(n, q0, m[0]);
      break;
    case MLQEM_SIM_OP_DEPOL2:
      if (density) cx.depol2(n, q0, q1, m[0]);
      break;
    case MLQEM_SIM_OP_READOUT:
      if (density)   // [[1 - p10, p01], [p10, 1 - p01]] on bit q0 of the diagonal; m = (p01, p10)
        cx.pair(n, q0, sim_c{1.0 - m[1], 0.0}, sim_c{m[0], 0.0}, sim_c{m[1], 0.0}, sim_c{1.0 - m[0], 0.0}, (1 << n) + 1);
      break;
    case MLQEM_SIM_OP_NOISE1:   // never inverted: a schedule's dagger bit is ignored, as for the depolarising kinds
      if (density) cx.noise1(n, q0, m[0], m[1], m[2], m[3]);
      break;
    case MLQEM_SIM_OP_NOISE2:
      if (density) cx.noise2(n, q0, q1, m);
      break;
    default:
      break;
  }
}

// The Pauli-term loop that follows the passes is not here: each kernel keeps its own copy, because as a shared function it changed
// the code the compiler emits for the passes of the workgroup variant and cost time (DESIGN.md 3.13 has the figures).

// Mean and standard error sqrt(M2 / (T (T - 1))) (0 at T = 1) of term i over the T trajectories, in trajectory order: a sum, then
// the squared deviations from the mean in a second pass, a fused multiply-add each
struct TrajStat {
  double mean, se;
};

__device__ __forceinline__ TrajStat traj_term_stats(const double* __restrict__ traj_terms, int64_t n_terms, int T, int64_t i) {
  const double count = (double)T, pairs = (double)T * (double)(T - 1);   // the callers' own: one copy after inlining
  double acc = 0.0, m2 = 0.0;
  for (int t = 0; t < T; ++t) acc = acc + traj_terms[(int64_t)t * n_terms + i];
  const double mean = acc / count;
  for (int t = 0; t < T; ++t) {
    const double d = traj_terms[(int64_t)t * n_terms + i] - mean;
    m2 = __builtin_fma(d, d, m2);
  }
  return TrajStat{mean, T > 1 ? sqrt(m2 / pairs) : 0.0};
}

// One trajectory's value of a circuit: sum coeff * term over its terms tb .. te in term order, a fused multiply-add per term from
// 0.0.  The finish kernels form it in both passes over the trajectories with these operations, so with the same bits.
__device__ __forceinline__ double traj_value(const double* __restrict__ coeff, const double* __restrict__ traj_terms, int64_t n_terms, int t,
                                             int64_t tb, int64_t te) {
  double v = 0.0;
  for (int64_t k = tb; k < te; ++k) v = __builtin_fma(coeff[k], traj_terms[(int64_t)t * n_terms + k], v);
  return v;
}

// Value sum coeff * tv and variance sum coeff^2 (1 - tv^2) of one sampled run over its terms tb .. te, in term order, a fused
// multiply-add per term; tv = estimate(t) is the term's sampled estimate
template <class F>
__device__ __forceinline__ void sample_value_variance(const double* __restrict__ coeff, int64_t tb, int64_t te, double& value, double& variance,
                                                      F&& estimate) {
  double val = 0.0, var = 0.0;
  for (int64_t t = tb; t < te; ++t) {
    const double tv = estimate(t), cf = coeff[t];
    val = __builtin_fma(cf, tv, val);
    var = __builtin_fma(cf * cf, __builtin_fma(-tv, tv, 1.0), var);
  }
  value = val;
  variance = var;
}

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): ten rounds of two 32 x 32 -> 64 products,
// the key bumped by the Weyl constants between rounds.
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t (&x)[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  x[0] = c0;
  x[1] = c1;
  x[2] = c2;
  x[3] = c3;
}

// ---- the host side of an entry point that takes a lowered batch ------------------------------------------------------------------------
// An entry point checks in this order: sim_batch_sizes and its own sizes (MLQEM_ERR_BAD_ARG), its own limit on n_wave + n_wg and what
// it does not support, the return of MLQEM_OK for a call without units (which may come with null buffers), then sim_batch_buffers
// and its own buffers.  That is why the batch's checks are two functions: the first runs before that return, the second after it.

// the counts of a lowered batch and of its units: none negative, and a pool that ends with its padding
inline bool sim_batch_sizes(int64_t n_circuits, int64_t n_ops, int64_t n_params, int64_t n_terms, int64_t n_wave, int64_t n_wg) {
  return n_circuits >= 0 && n_ops >= 0 && n_terms >= 0 && n_wave >= 0 && n_wg >= 0 && n_params >= kSimParamPad;
}

struct SimBatchPtrs {   // the three record arrays as the kernels read them: one 16-byte load per record
  const sim_i4 *circ, *ops, *terms;
};

// The buffers of a lowered batch: MLQEM_ERR_BAD_ARG for a missing one (`ops`, and `terms` with `coeff`, may be null where their
// count is 0) or a record array off its 16 bytes, else MLQEM_OK and the cast pointers.  `ids` is the call's list of units.
inline int sim_batch_buffers(const int32_t* circ, const int64_t* op_ptr, const mlqem_sim_op* ops, int64_t n_ops, const double* params,
                             const int64_t* term_ptr, const mlqem_sim_term* terms, const double* coeff, int64_t n_terms, const int32_t* ids,
                             SimBatchPtrs& out) {
  static_assert(sizeof(mlqem_sim_op) == 16 && sizeof(mlqem_sim_term) == 16, "one 16-byte load per record");
  if (!circ || !op_ptr || !params || !term_ptr || !ids || (n_ops > 0 && !ops) || (n_terms > 0 && (!terms || !coeff))) return MLQEM_ERR_BAD_ARG;
  if (!aligned_to(circ, 16) || !aligned_to(ops, 16) || !aligned_to(terms, 16)) return MLQEM_ERR_BAD_ARG;
  out = SimBatchPtrs{reinterpret_cast<const sim_i4*>(circ), reinterpret_cast<const sim_i4*>(ops), reinterpret_cast<const sim_i4*>(terms)};
  return MLQEM_OK;
}

// The launch pair of a call: the first n_wave of `ids` run a wave per unit, four units a workgroup, the other n_wg a workgroup per
// unit; an id stands for `per_id` units (a circuit's trajectories).  launch(wg, grid, ids, count) launches the WG = wg.value
// instantiation over `count` ids; a part without ids is not launched.
template <class F> void sim_launch_pair(const int32_t* ids, int64_t n_wave, int64_t n_wg, int64_t per_id, F&& launch) {
  if (n_wave > 0) launch(std::false_type{}, dim3((unsigned)ceil_div(n_wave * per_id, (int64_t)(kBlock / kWave))), ids, (int)n_wave);
  if (n_wg > 0) launch(std::true_type{}, dim3((unsigned)(n_wg * per_id)), ids + n_wave, (int)n_wg);
}

}  // namespace
}  // namespace mlqem
