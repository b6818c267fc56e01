// Parameter binding on the device (mlqem_sim_run_bound_f64) and the parameter-shift combine (mlqem_sim_shift_combine_f64).
// include/mlqem_hip.h has the contract.
//
// A TEMPLATE is a circuit lowered once, with its free angles left in the program: a parameterised record (PRX, PRY, PRZ, PP, PRZZ)
// owns (parameter index, scale, offset) in the pool instead of a matrix.  A RUN is (template, row of theta, shifted record or -1):
// thousands of bindings of one ansatz share one set of records and differ in a row of float64, and the 2 K shifted runs of a
// parameter-shift gradient differ in 16 bytes each.  The kernel is sim_kernel's (sim.hip) with the run in the place of the circuit:
// the same state in LDS, and for everything but its own parameterised kinds it CALLS what sim_kernel calls -- the prologue, the
// record decode, the norm pass, the switch over the fixed kinds (sim_apply_fixed with FOLD = false), one copy of each in sim_ctx.hpp;
// the term loop is sim_kernel's text, kept here as a copy (sim_ctx.hpp says why).  So a template without parameterised records gives
// the bits of mlqem_sim_run_f64, and a pass added to that switch is added here too.
//
// The matrices.  The angle of a record is uniform over the wave, and a double-precision sin/cos (the device library's: argument
// reduction and two polynomials, some 150 instructions) is long next to a pass over 32 amplitudes.  Two forms, one switch (`form`):
//   TABLE  a trig table in LDS, (cos, sin) per record of the current WINDOW of T records (T = 64 in the wave variant, 256 in the
//          workgroup variant: the threads on one run).  When the op loop enters a window, lane l takes record l of it: if the
//          record is parameterised the lane forms its angle and stores 16 bytes; the op loop reads the pair when it reaches the
//          record (one broadcast LDS read).  A wave whose 64 records hold no parameterised one skips the trig (a wave-uniform
//          ballot).  The window is counted in RECORDS, not in parameterised records: the kernel has the records alone, and the
//          l-th parameterised record could only be found by a scan or from another array, while record l of the window is an
//          address.  So the table needs no ordinal in the record and the lowering stores none.
//   PLAIN  trig per record inside the op loop, every lane computing the same value: the A/B baseline.
// Both compute the same function of the same double, so they agree bit for bit (tests/test_gpu_bound.py asserts it).
//
// Occupancy is stated as in sim_kernel; the compiler's resource usage is in DESIGN.md 3.14.
#include "sim_ctx.hpp"

namespace mlqem {
namespace {

__device__ __forceinline__ bool bound_is_param(int kind) { return kind >= MLQEM_SIM_OP_PRX && kind <= MLQEM_SIM_OP_PRZZ; }

// (cos, sin) of the record's trig argument: phi for PP, 0.5 * phi (an exact product) for the four rotations, with
// phi = scale * theta + offset (+ shift), every step rounded on its own
__device__ __forceinline__ sim_c bound_trig(int kind, const double* __restrict__ m, const double* __restrict__ theta_row, int ld_theta,
                                            bool shifted, double shift) {
  // No contraction: every step is rounded on its own.  The operations are written out under the pragma because the header's
  // __dmul_rn / __dadd_rn are plain `*` and `+` defined outside its reach, and the compiler fuses those into one fma.
#pragma clang fp contract(off)
  const int idx = min(max(__double2int_rz(m[0]), 0), ld_theta - 1);
  const double prod = m[1] * theta_row[idx];
  double phi = prod + m[2];
  phi = shifted ? phi + shift : phi;
  const double arg = kind == MLQEM_SIM_OP_PP ? phi : 0.5 * phi;
  return sim_c{cos(arg), sin(arg)};
}

template <bool WG, bool TABLE>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(WG ? 4 : 7))) void bound_kernel(
    int B, const sim_i4* __restrict__ circ, const int64_t* __restrict__ op_ptr, const sim_i4* __restrict__ ops, int64_t n_ops,
    const double* __restrict__ params, int64_t n_params, const int64_t* __restrict__ term_ptr, const sim_i4* __restrict__ terms,
    const double* __restrict__ coeff, int64_t n_terms, const double* __restrict__ theta, int n_rows, int ld_theta,
    const sim_i4* __restrict__ runs, int n_runs, const double* __restrict__ shift, const int32_t* __restrict__ ids, int count,
    const int64_t* __restrict__ run_term_ptr, int64_t n_out, double* __restrict__ term_values, double* __restrict__ values,
    double* __restrict__ norm) {
  __shared__ sim_c state[WG ? kSimMaxAmps : kBlock / kWave * kSimWaveAmps];
  __shared__ sim_c trig[TABLE ? kBlock : 1];   // the window's (cos, sin): 256 records of a workgroup's run, or 64 per wave
  __shared__ double red[8];
  SimCtx<WG> cx;
  const int slot = cx.begin(state, red);
  if (slot >= count) return;   // a wave of a partly filled workgroup: wave-uniform, and this variant has no workgroup barrier
  const int tid = cx.tid;
  sim_c* tab = WG ? trig : trig + (TABLE ? ((int)threadIdx.x >> 6) * kWave : 0);
  const int run = __builtin_amdgcn_readfirstlane(min(max(ids[slot], 0), n_runs - 1));
  const sim_i4 rinfo = runs[run];   // template, theta row, shifted op, reserved
  const int c = __builtin_amdgcn_readfirstlane(min(max(rinfo.x, 0), B - 1));
  const int row = __builtin_amdgcn_readfirstlane(min(max(rinfo.y, 0), n_rows - 1));
  const double* theta_row = theta + (int64_t)row * ld_theta;
  const double sh = shift[run];
  const sim_i4 info = circ[c];   // n_qubits, mode, trailing readout ops, reserved
  const bool density = info.y != 0;
  constexpr int kMaxBits = WG ? 11 : 8;
  const int n = __builtin_amdgcn_readfirstlane(min(max(info.x, 1), density ? kMaxBits / 2 : kMaxBits));
  const int nbits = density ? 2 * n : n, A = 1 << nbits;
  cx.nbits = nbits;
  cx.A = A;
  const int64_t ob = min(max(op_ptr[c], (int64_t)0), n_ops), oe = min(max(op_ptr[c + 1], ob), n_ops);
  const int n_op = __builtin_amdgcn_readfirstlane((int)min(oe - ob, (int64_t)0x7FFFFFFF));
  const int n_step = n_op;
  const int sop = __builtin_amdgcn_readfirstlane(rinfo.z >= 0 && rinfo.z < n_op ? rinfo.z : -1);   // outside the circuit: none
  const int n_main = n_step - min(max(info.z, 0), n_step);   // steps before the readout ops: Tr rho is taken there

  for (int i = tid; i < A; i += cx.T) cx.st[i] = sim_c{i == 0 ? 1.0 : 0.0, 0.0};
  sim_sync<WG>();

  double nrm = 0.0;
  for (int k = 0; k <= n_step; ++k) {
    if (k == n_main) {   // <psi|psi> or Tr rho, before any readout op
      nrm = sim_norm(cx, n, density);
      if (WG) __syncthreads();   // red[0..3] is free again
    }
    if (k == n_step) break;
    if constexpr (TABLE) {
      if ((k & (cx.T - 1)) == 0) {   // a new window: lane l takes record k + l.  The last read of the old window lies before a
                                     // pass, and a pass ends in the variant's barrier, so the table is free
        const int r = k + tid;
        const sim_i4 rec = ops[ob + min(r, n_op - 1)];
        const bool is_p = r < n_op && bound_is_param(rec.x);
        const double* rm = params + min((int64_t)max(rec.w, 0), n_params - kSimParamPad);
        if (__ballot(is_p) != 0) {   // uniform over the wave
          const sim_c cs = bound_trig(rec.x, rm, theta_row, ld_theta, r == sop, sh);
          if (is_p) tab[tid] = cs;
        }
        sim_sync<WG>();
      }
    }
    const SimRec rec = sim_decode(ops[ob + k], n, params, n_params);   // kind, q0, q1, offset into params
    const int kind = rec.kind, q0 = rec.q0, q1 = rec.q1;
    if (bound_is_param(kind)) {   // uniform over the wave (and the workgroup)
      sim_c cs;
      if constexpr (TABLE) cs = tab[k & (cx.T - 1)];
      else cs = bound_trig(kind, rec.m, theta_row, ld_theta, k == sop, sh);
      const double co = cs.x, si = cs.y;
      if (kind == MLQEM_SIM_OP_PRX) {          // [[c, -is], [-is, c]]
        cx.pair(nbits, q0, sim_c{co, 0.0}, sim_c{0.0, -si}, sim_c{0.0, -si}, sim_c{co, 0.0}, 1);
        if (density) cx.pair(nbits, q0 + n, sim_c{co, 0.0}, sim_c{0.0, si}, sim_c{0.0, si}, sim_c{co, 0.0}, 1);
      } else if (kind == MLQEM_SIM_OP_PRY) {   // [[c, -s], [s, c]]: real, so conj(U) = U
        cx.pair(nbits, q0, sim_c{co, 0.0}, sim_c{-si, 0.0}, sim_c{si, 0.0}, sim_c{co, 0.0}, 1);
        if (density) cx.pair(nbits, q0 + n, sim_c{co, 0.0}, sim_c{-si, 0.0}, sim_c{si, 0.0}, sim_c{co, 0.0}, 1);
      } else if (kind == MLQEM_SIM_OP_PRZZ) {  // diag by the parity of bits q0, q1: one element pass in both modes
        const sim_c d0{co, -si}, d1{co, si};
        if (density) {
          cx.element([&](int i) {
            const bool r = ((i >> q0) ^ (i >> q1)) & 1, cc = ((i >> (q0 + n)) ^ (i >> (q1 + n))) & 1;
            return cmul(sim_c{co, r ? d1.y : d0.y}, sim_c{co, cc ? -d1.y : -d0.y});
          });
        } else {
          cx.element([&](int i) { return ((i >> q0) ^ (i >> q1)) & 1 ? d1 : d0; });
        }
      } else {                                 // PRZ: diag(c - is, c + is); PP: diag(1, c + is) -- DIAG1's pass
        const bool pp = kind == MLQEM_SIM_OP_PP;
        const sim_c d0{pp ? 1.0 : co, pp ? 0.0 : -si}, d1{co, si};
        if (density) {
          cx.element([&](int i) {   // d[row bit] conj(d[column bit])
            const bool r = (i >> q0) & 1, cc = (i >> (q0 + n)) & 1;
            return cmul(sim_c{r ? d1.x : d0.x, r ? d1.y : d0.y}, sim_c{cc ? d1.x : d0.x, cc ? -d1.y : -d0.y});
          });
        } else {
          cx.element([&](int i) { return (i >> q0) & 1 ? d1 : d0; });
        }
      }
      continue;
    }
    sim_apply_fixed<false>(cx, rec, n, density, false);   // the fixed kinds: sim_kernel's passes, from the text sim_kernel runs
  }

  // Pauli terms: P|j> = i^ny (-1)^popcount(j & z) |j ^ x>
  const int64_t tb = min(max(term_ptr[c], (int64_t)0), n_terms), te = min(max(term_ptr[c + 1], tb), n_terms);
  const int n_term = __builtin_amdgcn_readfirstlane((int)min(te - tb, (int64_t)0x7FFFFFFF));
  // the run's slice of term_values: a term past its end, or past the end of the buffer, is computed and not stored
  const int64_t rb = min(max(run_term_ptr[run], (int64_t)0), n_out), re_ = min(max(run_term_ptr[run + 1], rb), n_out);
  const int64_t n_store = re_ - rb;
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
      if (t < n_store) term_values[rb + t] = tv;
      total = total + coeff[tb + t] * tv;
    }
  }
  if (tid == 0) {
    values[run] = total;
    norm[run] = nrm;
  }
}

// grad[b][p] = sum over p's occurrences j in circuit order of (0.5 * scale[k]) * (v_plus[k][b] - v_minus[k][b]), k = occ[j]: from
// 0.0, every difference, product and sum rounded on its own (0.5 * scale is exact)
__global__ __launch_bounds__(kBlock) void shift_combine_kernel(int64_t n_rows, int n_par, int64_t n_occ, const int64_t* __restrict__ occ_ptr,
                                                               const int32_t* __restrict__ occ, const double* __restrict__ scale,
                                                               int64_t n_shift, const double* __restrict__ v_plus,
                                                               const double* __restrict__ v_minus, double* __restrict__ grad) {
  // every difference, product and sum is rounded on its own: written out under the pragma (see bound_trig)
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n_rows * n_par) return;
  int p;
  const int64_t b = split_index(i, n_par, p);
  const int64_t jb = min(max(occ_ptr[p], (int64_t)0), n_occ), je = min(max(occ_ptr[p + 1], jb), n_occ);
  double acc = 0.0;
  for (int64_t j = jb; j < je; ++j) {
    const int64_t k = min(max((int64_t)occ[j], (int64_t)0), n_shift - 1);
    const double d = v_plus[k * n_rows + b] - v_minus[k * n_rows + b];
    const double t = (0.5 * scale[k]) * d;
    acc = acc + t;
  }
  grad[i] = acc;
}

}  // namespace
}  // namespace mlqem

using namespace mlqem;

extern "C" int mlqem_sim_run_bound_f64(int64_t n_templates, const int32_t* circ, const int64_t* op_ptr, const mlqem_sim_op* ops,
                                       int64_t n_ops, const double* params, int64_t n_params, const int64_t* term_ptr,
                                       const mlqem_sim_term* terms, const double* coeff, int64_t n_terms, const double* theta,
                                       int64_t n_rows, int64_t ld_theta, const int32_t* runs, int64_t n_runs, const double* shift,
                                       const int32_t* ids, int64_t n_wave, int64_t n_wg, const int64_t* run_term_ptr,
                                       int64_t n_out_terms, int32_t form, double* term_values, double* values, double* norm,
                                       mlqem_stream_t stream) {
  begin_launches();
  if (!sim_batch_sizes(n_templates, n_ops, n_params, n_terms, n_wave, n_wg) || n_rows < 0 || ld_theta < 0 || n_runs < 0 || n_out_terms < 0 ||
      (form != MLQEM_SIM_BOUND_TABLE && form != MLQEM_SIM_BOUND_PLAIN))
    return MLQEM_ERR_BAD_ARG;
  if (n_wave + n_wg > n_runs) return MLQEM_ERR_BAD_ARG;
  if (n_templates > 0x7FFFFFFFll || n_params > 0x7FFFFFFFll || n_runs > 0x7FFFFFFFll || n_rows > 0x7FFFFFFFll || ld_theta > 0x7FFFFFFFll)
    return MLQEM_ERR_UNSUPPORTED;
  if (n_wave + n_wg == 0) return MLQEM_OK;
  if (n_templates < 1 || n_rows < 1 || ld_theta < 1) return MLQEM_ERR_BAD_ARG;   // a run names a template and a row of >= 1 value
  SimBatchPtrs b;
  if (int code = sim_batch_buffers(circ, op_ptr, ops, n_ops, params, term_ptr, terms, coeff, n_terms, ids, b)) return code;
  if (!theta || !runs || !shift || !run_term_ptr || !values || !norm || (n_out_terms > 0 && !term_values)) return MLQEM_ERR_BAD_ARG;
  if (!aligned_to(runs, 16) || !aligned_to(theta, 8) || !aligned_to(shift, 8) || !aligned_to(run_term_ptr, 8)) return MLQEM_ERR_BAD_ARG;
  const sim_i4* ri = reinterpret_cast<const sim_i4*>(runs);
  sim_launch_pair(ids, n_wave, n_wg, 1, [&](auto wg, dim3 grid, const int32_t* id, int count) {
    auto kernel = form == MLQEM_SIM_BOUND_TABLE ? bound_kernel<decltype(wg)::value, true> : bound_kernel<decltype(wg)::value, false>;
    hipLaunchKernelGGL(kernel, grid, dim3(kBlock), 0, as_stream(stream), (int)n_templates, b.circ, op_ptr, b.ops, n_ops, params, n_params,
                       term_ptr, b.terms, coeff, n_terms, theta, (int)n_rows, (int)ld_theta, ri, (int)n_runs, shift, id, count, run_term_ptr,
                       n_out_terms, term_values, values, norm);
  });
  return launch_status();
}

extern "C" int mlqem_sim_shift_combine_f64(int64_t n_rows, int64_t n_parameters, int64_t n_shifts, const int64_t* occ_ptr,
                                           const int32_t* occ, int64_t n_occ, const double* scale, const double* v_plus,
                                           const double* v_minus, double* grad, mlqem_stream_t stream) {
  begin_launches();
  if (n_rows < 0 || n_parameters < 0 || n_shifts < 0 || n_occ < 0) return MLQEM_ERR_BAD_ARG;
  if (n_rows > 0x7FFFFFFFll || n_parameters > 0x7FFFFFFFll || n_shifts > 0x7FFFFFFFll || n_occ > 0x7FFFFFFFll) return MLQEM_ERR_UNSUPPORTED;
  if (n_rows * n_parameters > 0x7FFFFFFFll * (int64_t)kBlock) return MLQEM_ERR_UNSUPPORTED;
  if (n_rows == 0 || n_parameters == 0) return MLQEM_OK;
  if (!occ_ptr || !grad || (n_occ > 0 && (!occ || n_shifts < 1 || !scale || !v_plus || !v_minus))) return MLQEM_ERR_BAD_ARG;
  hipLaunchKernelGGL(shift_combine_kernel, dim3((unsigned)ceil_div(n_rows * n_parameters, (int64_t)kBlock)), dim3(kBlock), 0,
                     as_stream(stream), n_rows, (int)n_parameters, n_occ, occ_ptr, occ, scale, n_shifts, v_plus, v_minus, grad);
  return launch_status();
}
