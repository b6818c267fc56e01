// Parameter binding for the matrix-product-state path (mlqem_mps_bind_f64).  include/mlqem_hip.h has the contract.
//
// Templates are lowered ONCE (blackwater.sim.compile_mps_templates): the records of mlqem_mps_run_f64, and for every U1 / U2 record
// whose matrix depends on a parameter a FACTOR PROGRAM F_k ... F_2 F_1.  A run is (template, row of theta, shifted occurrence or
// -1).  This kernel writes, for the R runs of a call, what compile_mps would have produced for the R bound copies: per run a slice
// of a float64 pool (the matrices of parameterised records formed here, everything else copied) and the template's `ops` rows with
// the pool offset rebased.  mps_run_kernel then runs them as it runs any batch: nothing in mps.hip knows of templates.
//
// Work shape.  R x records pieces, each a handful of small complex products and at most 256 bytes written: the kernel is bound by
// that write.  SIXTEEN LANES TAKE ONE RECORD, lane e the matrix entry e = 4 i + j (a U1 record: its first four lanes), so
//   a wave's store is 4 records x 16 lanes x 16 B = 1 KiB of consecutive addresses where records follow each other in the pool
//     (the ideal lowering: U2 after U2), the widest store there is.  One thread per record would write 32 B pieces 256 B apart
//     and hold the matrix as a runtime-indexed array of 16 complex numbers, which the compiler keeps in scratch;
//   M <- F M needs, in lane (i, j), column j of M: for a 2x2 on a slot one row beside the lane's own, for a fixed 4x4 the four rows,
//     each a cross-lane read inside the 16-lane group (no LDS, no barrier), and a diagonal factor nothing at all;
//   the price is the trig: every lane of a group forms the same sin / cos, so a wave does it for 4 records, not 64.  It is
//     arithmetic under a store-bound kernel (DESIGN.md 3.19 has the resource usage and the measurement).
// All sixteen lanes of a group take the same path (the record and its factors are the group's), so the cross-lane reads only name
// lanes that are active with the reader.
#include "sim_ctx.hpp"

// every product, sum and difference below is rounded on its own: no fma is formed from them (DESIGN.md 3.14 has the fma this avoids)
#pragma clang fp contract(off)

namespace mlqem {
namespace {

constexpr int kBindGroup = 16;                       // lanes on one record
constexpr int kBindRecords = kBlock / kBindGroup;    // records a workgroup takes per step

__device__ __forceinline__ sim_c bind_mul(sim_c a, sim_c b) {
  const double rr = a.x * b.x, ii = a.y * b.y, ri = a.x * b.y, ir = a.y * b.x;
  return sim_c{rr - ii, ri + ir};
}
// acc + a b: the product as bind_mul forms it, then one sum per part
__device__ __forceinline__ sim_c bind_mac(sim_c acc, sim_c a, sim_c b) {
  const sim_c p = bind_mul(a, b);
  return sim_c{acc.x + p.x, acc.y + p.y};
}
__device__ __forceinline__ sim_c bind_lane(sim_c v, int src) {   // the value of lane `src` of the 16-lane group
  return sim_c{__shfl(v.x, src, kBindGroup), __shfl(v.y, src, kBindGroup)};
}

__global__ __launch_bounds__(kBlock) void mps_bind_kernel(
    int C, const int64_t* __restrict__ op_ptr, const sim_i4* __restrict__ ops, int64_t n_ops, const double* __restrict__ params,
    int64_t n_params, const int64_t* __restrict__ pool_ptr, const int64_t* __restrict__ fac_ptr, const sim_i4* __restrict__ fac,
    const double* __restrict__ fac_val, int64_t n_fac, const double* __restrict__ fpool, int64_t n_fpool,
    const int64_t* __restrict__ occ_ptr, const int32_t* __restrict__ occ, int64_t n_occ, const double* __restrict__ theta, int n_rows,
    int ld_theta, const sim_i4* __restrict__ runs, const double* __restrict__ shift, const int64_t* __restrict__ out_op_ptr,
    const int64_t* __restrict__ out_pool_ptr, sim_i4* __restrict__ out_ops, int64_t n_out_ops, double* __restrict__ out_pool,
    int64_t n_out_pool) {
  const int run = (int)blockIdx.x;
  const int grp = (int)threadIdx.x / kBindGroup, e = (int)threadIdx.x & (kBindGroup - 1);
  const sim_i4 rinfo = runs[run];   // template, theta row, shifted occurrence or -1, reserved
  const int c = min(max(rinfo.x, 0), C - 1);
  const int row = min(max(rinfo.y, 0), n_rows - 1);
  const double* theta_row = theta + (int64_t)row * ld_theta;
  const double sh = shift[run];
  const int64_t ob = min(max(op_ptr[c], (int64_t)0), n_ops), oe = min(max(op_ptr[c + 1], ob), n_ops);
  const int n_rec = (int)min(oe - ob, (int64_t)0x7FFFFFFF);
  const int64_t tb = min(max(pool_ptr[c], (int64_t)0), n_params - kSimParamPad);   // the template's slice of params begins here
  const int64_t qb = min(max(occ_ptr[c], (int64_t)0), n_occ), qe = min(max(occ_ptr[c + 1], qb), n_occ);
  int srec = -1, sfac = -1;   // the shifted factor: an occurrence outside the template's is none
  if (rinfo.z >= 0 && (int64_t)rinfo.z < qe - qb) {
    srec = occ[2 * (qb + rinfo.z)];
    sfac = occ[2 * (qb + rinfo.z) + 1];
  }
  const int64_t out_ob = out_op_ptr[run], out_pb = out_pool_ptr[run];

  for (int k = (int)blockIdx.y * kBindRecords + grp; k < n_rec; k += (int)gridDim.y * kBindRecords) {
    const sim_i4 op = ops[ob + k];   // kind, site, orientation, offset into params
    const int kind = op.x;
    const int64_t src = min((int64_t)max(op.w, 0), n_params - kSimParamPad);
    // the run's copy of the record sits where the template's does inside its slice; a slice holds a matrix wherever this lands
    const int64_t po = min(max(out_pb + (src - tb), (int64_t)0), n_out_pool - kSimParamPad);
    const int64_t oo = out_ob + k;
    if (e == 0 && oo >= 0 && oo < n_out_ops) out_ops[oo] = sim_i4{kind, op.y, op.z, (int)po};
    const bool two = kind == MLQEM_MPS_OP_U2;
    if (!two && kind != MLQEM_MPS_OP_U1) {   // DEPOL1 / DEPOL2 (and anything unknown): one value, copied
      if (e == 0) out_pool[po] = params[src];
      continue;
    }
    const int d = two ? 4 : 2;                        // the matrix is d x d
    const int el = two ? e : e & 3;                   // lanes 4 .. 15 of a U1 record shadow its four and store nothing
    const int i = two ? el >> 2 : el >> 1, j = two ? el & 3 : el & 1;
    const int64_t fb = min(max(fac_ptr[ob + k], (int64_t)0), n_fac), fe = min(max(fac_ptr[ob + k + 1], fb), n_fac);
    const int nf = (int)min(fe - fb, (int64_t)0x7FFFFFFF);
    sim_c m = sim_c{params[src + 2 * el], params[src + 2 * el + 1]};   // no factor program: the host matrix, bit for bit
    for (int f = 0; f < nf; ++f) {
      const sim_i4 fi = fac[fb + f];   // kind, slot, parameter, offset into fpool
      if (fi.x == MLQEM_MPS_FACTOR_FIXED) {
        const double* fm = fpool + min((int64_t)max(fi.w, 0), n_fpool - kSimParamPad) + 2 * (i * d);   // row i of F
        if (f == 0) {
          m = sim_c{fm[2 * j], fm[2 * j + 1]};
        } else {   // (F M)[i][j] = sum over k of F[i][k] M[k][j], k ascending
          sim_c acc = bind_mul(sim_c{fm[0], fm[1]}, bind_lane(m, j));
          for (int r = 1; r < d; ++r) acc = bind_mac(acc, sim_c{fm[2 * r], fm[2 * r + 1]}, bind_lane(m, r * d + j));
          m = acc;
        }
        continue;
      }
      const double* fv = fac_val + 2 * (fb + f);   // scale, offset
      const double prod = fv[0] * theta_row[min(max(fi.z, 0), ld_theta - 1)];
      double phi = prod + fv[1];
      phi = (k == srec && f == sfac) ? phi + sh : phi;
      const double arg = fi.x == MLQEM_SIM_OP_PP ? phi : 0.5 * phi;
      double si, co;
      sincos(arg, &si, &co);
      if (fi.x == MLQEM_SIM_OP_PRX || fi.x == MLQEM_SIM_OP_PRY) {
        // a 2x2 g on the slot: bit `bit` of the row index.  (G M)[i][j] = g[b][0] M[i with the bit clear][j] + g[b][1] M[i with it set][j]
        const int bit = two ? min(max(fi.y, 0), 1) : 0, b = (i >> bit) & 1;
        const bool rx = fi.x == MLQEM_SIM_OP_PRX;
        // PRX [[c, -is], [-is, c]]; PRY [[c, -s], [s, c]]
        const sim_c diag{co, 0.0}, off = rx ? sim_c{0.0, -si} : b ? sim_c{si, 0.0} : sim_c{-si, 0.0};
        const sim_c g0 = b ? off : diag, g1 = b ? diag : off;
        if (f == 0) {
          const bool same = (i & ~(1 << bit)) == (j & ~(1 << bit));   // the other bit is untouched
          m = !same ? sim_c{0.0, 0.0} : ((j >> bit) & 1) ? g1 : g0;
        } else {
          const sim_c m0 = bind_lane(m, (i & ~(1 << bit)) * d + j), m1 = bind_lane(m, (i | (1 << bit)) * d + j);
          m = bind_mac(bind_mul(g0, m0), g1, m1);
        }
      } else {
        // a diagonal: PRZ diag(c - is, c + is) and PP diag(1, c + is) by the slot's bit, PRZZ (c - is) on even and (c + is) on odd
        // parity of the two bits
        const int bit = two ? min(max(fi.y, 0), 1) : 0;
        const bool up = fi.x == MLQEM_SIM_OP_PRZZ ? (((i >> 1) ^ i) & 1) != 0 : ((i >> bit) & 1) != 0;
        const sim_c dv = up ? sim_c{co, si} : fi.x == MLQEM_SIM_OP_PP ? sim_c{1.0, 0.0} : sim_c{co, -si};
        if (f == 0) m = i == j ? dv : sim_c{0.0, 0.0};
        else m = bind_mul(dv, m);
      }
    }
    if (e < d * d) {
      double* dst = out_pool + po + 2 * e;
      if ((po & 1) == 0 && aligned_to_dev(out_pool, 16)) {
        *reinterpret_cast<sim_c*>(dst) = m;   // 16 B per lane, a record 256 consecutive bytes
      } else {   // a DEPOL record's single value before it: the matrix sits on an odd offset
        dst[0] = m.x;
        dst[1] = m.y;
      }
    }
  }
}

}  // namespace
}  // namespace mlqem

using namespace mlqem;

extern "C" int mlqem_mps_bind_f64(int64_t n_templates, const int64_t* op_ptr, const mlqem_sim_op* ops, int64_t n_ops, const double* params,
                                  int64_t n_params, const int64_t* pool_ptr, const int64_t* fac_ptr, const int32_t* fac,
                                  const double* fac_val, int64_t n_fac, const double* fpool, int64_t n_fpool, const int64_t* occ_ptr,
                                  const int32_t* occ, int64_t n_occ, const double* theta, int64_t n_rows, int64_t ld_theta,
                                  const int32_t* runs, const double* shift, int64_t n_runs, int64_t max_records,
                                  const int64_t* out_op_ptr, const int64_t* out_pool_ptr, mlqem_sim_op* out_ops, int64_t n_out_ops,
                                  double* out_pool, int64_t n_out_pool, mlqem_stream_t stream) {
  begin_launches();
  if (n_templates < 0 || n_ops < 0 || n_params < kSimParamPad || n_fac < 0 || n_fpool < kSimParamPad || n_occ < 0 || n_rows < 0 ||
      ld_theta < 0 || n_runs < 0 || max_records < 0 || n_out_ops < 0 || n_out_pool < kSimParamPad)
    return MLQEM_ERR_BAD_ARG;
  if (n_templates > 0x7FFFFFFFll || n_params > 0x7FFFFFFFll || n_fpool > 0x7FFFFFFFll || n_fac > 0x7FFFFFFFll || n_occ > 0x7FFFFFFFll ||
      n_rows > 0x7FFFFFFFll || ld_theta > 0x7FFFFFFFll || n_runs > 0x7FFFFFFFll || max_records > 0x7FFFFFFFll || n_out_pool > 0x7FFFFFFFll)
    return MLQEM_ERR_UNSUPPORTED;
  if (n_runs == 0 || max_records == 0) return MLQEM_OK;
  if (n_templates < 1 || n_rows < 1 || ld_theta < 1) return MLQEM_ERR_BAD_ARG;   // a run names a template and a row of >= 1 value
  if (!op_ptr || !params || !pool_ptr || !fac_ptr || !fpool || !occ_ptr || !theta || !runs || !shift || !out_op_ptr || !out_pool_ptr ||
      !out_pool || (n_ops > 0 && !ops) || (n_fac > 0 && (!fac || !fac_val)) || (n_occ > 0 && !occ) || (n_out_ops > 0 && !out_ops))
    return MLQEM_ERR_BAD_ARG;
  if (!aligned_to(ops, 16) || !aligned_to(fac, 16) || !aligned_to(runs, 16) || !aligned_to(out_ops, 16) || !aligned_to(out_pool, 8) ||
      !aligned_to(params, 8) || !aligned_to(fpool, 8) || !aligned_to(fac_val, 8) || !aligned_to(theta, 8) || !aligned_to(shift, 8))
    return MLQEM_ERR_BAD_ARG;
  const unsigned gy = (unsigned)std::min<int64_t>(ceil_div(max_records, (int64_t)kBindRecords), 65535);
  hipLaunchKernelGGL(mps_bind_kernel, dim3((unsigned)n_runs, gy), dim3(kBlock), 0, as_stream(stream), (int)n_templates, op_ptr,
                     reinterpret_cast<const sim_i4*>(ops), n_ops, params, n_params, pool_ptr, fac_ptr, reinterpret_cast<const sim_i4*>(fac),
                     fac_val, n_fac, fpool, n_fpool, occ_ptr, occ, n_occ, theta, (int)n_rows, (int)ld_theta,
                     reinterpret_cast<const sim_i4*>(runs), shift, out_op_ptr, out_pool_ptr, reinterpret_cast<sim_i4*>(out_ops), n_out_ops,
                     out_pool, n_out_pool);
  return launch_status();
}
