// What the simulator's kernels share (sim.hip: exact runs, folded runs, measurement shots; sim_traj.hip: quantum trajectories):
// the LDS state's types, the passes of SimCtx and the Philox4x32-10 generator.  sim.hip's header comment states the rules of a
// pass; everything here is in an unnamed namespace, so each translation unit has its own copy.
#pragma once
#include "common.hpp"

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

}  // namespace
}  // namespace mlqem
