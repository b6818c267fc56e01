// What clifford.hip (the backward walk of a Pauli) and clifford_frames.hip (Pauli-frame sampling) share: a lane's Pauli words in
// registers or in LDS, the inverse of a conjugation table and the step that applies one record.  clifford.hip's header comment
// states the layouts; everything here is in an unnamed namespace, so each translation unit has its own copy.
#pragma once
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

// The record a daggered schedule entry applies is the INVERSE table, formed as the record is read: the table is a signed
// permutation of the local Paulis, so the image of p under the inverse is the entry whose letter field holds p, and its sign bit
// is that entry's.  A table that holds p nowhere (malformed) gives entry 0; an index is never above the table's last entry.
__device__ __forceinline__ uint32_t clf_find_c1(uint32_t tab, uint32_t a) {   // a = 1 .. 3
  return (tab & 3u) == a ? 0u : ((tab >> 3) & 3u) == a ? 1u : ((tab >> 6) & 3u) == a ? 2u : 0u;
}

__device__ __forceinline__ uint32_t clf_find_c2(uint64_t tab, uint32_t pq) {   // pq = 1 .. 15
  // the lowest zero nibble of tab ^ pq pq .. pq: below it no nibble is zero, so no borrow reaches it and the lowest flag is exact
  const uint64_t x = tab ^ (0x1111111111111111ull * (uint64_t)pq);
  const uint64_t zero = (x - 0x1111111111111111ull) & ~x & 0x8888888888888888ull;
  const int at = __ffsll((unsigned long long)zero);   // 0 when there is none, else 4 e + 4
  return at ? min((uint32_t)(at - 1) >> 2, 14u) : 0u;
}

// One record applied to the lane's Pauli (`dagger`: its inverse; only the FOLD instantiations look at the flag).  A function on
// the words themselves, not a lambda around them: a closure holds the words' address, and the register instantiation's words then
// live in scratch.
template <bool REG, bool FOLD>
__device__ __forceinline__ void clf_step(ClfWords<REG>& p, uint32_t& sign, double& factor, const int n, const clf_i4 rec,
                                         const double keep, const bool dagger) {
  const int kind = rec.x & 15;
  const int q0 = min((rec.x >> 4) & 1023, n - 1), q1 = min((rec.x >> 14) & 1023, n - 1);
  const int w0 = q0 >> 5, b0 = q0 & 31, w1 = q1 >> 5, b1 = q1 & 31;
  const uint32_t a = ((p.getx(w0) >> b0) & 1u) | (((p.getz(w0) >> b0) & 1u) << 1);
  const bool two = kind == MLQEM_CLIFFORD_OP_C2 || kind == MLQEM_CLIFFORD_OP_DEPOL2;
  const uint32_t b = two ? ((p.getx(w1) >> b1) & 1u) | (((p.getz(w1) >> b1) & 1u) << 1) : 0u;
  const uint32_t pq = a | (b << 2);
  if (kind == MLQEM_CLIFFORD_OP_C1) {
    uint32_t img = a ? ((uint32_t)rec.y >> (3 * (a ? a - 1 : 0u))) & 7u : 0u;   // letter | sign << 2; I stays I
    if (FOLD && dagger) {
      const uint32_t e = clf_find_c1((uint32_t)rec.y, a);
      img = a ? (e + 1u) | ((((uint32_t)rec.y >> (3 * e + 2)) & 1u) << 2) : 0u;
    }
    const uint32_t d = (img & 3u) ^ a;
    sign ^= img >> 2;
    p.flip(w0, (d & 1u) << b0, (d >> 1) << b0);
  } else if (kind == MLQEM_CLIFFORD_OP_C2) {
    const uint64_t tab = (uint64_t)(uint32_t)rec.y | ((uint64_t)(uint32_t)rec.z << 32);
    uint32_t e = pq ? pq - 1 : 0u;
    uint32_t img = pq ? (uint32_t)(tab >> (4 * e)) & 15u : 0u;
    if (FOLD && dagger) {
      e = clf_find_c2(tab, pq);
      img = pq ? e + 1u : 0u;
    }
    const uint32_t d = img ^ pq;
    sign ^= pq ? ((uint32_t)rec.w >> e) & 1u : 0u;
    p.flip(w0, (d & 1u) << b0, ((d >> 1) & 1u) << b0);
    p.flip(w1, ((d >> 2) & 1u) << b1, ((d >> 3) & 1u) << b1);
  } else if (kind == MLQEM_CLIFFORD_OP_DEPOL1 || kind == MLQEM_CLIFFORD_OP_DEPOL2) {
    factor = pq ? factor * keep : factor;
  }
}

}  // namespace
}  // namespace mlqem
