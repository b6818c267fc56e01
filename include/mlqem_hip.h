/*
 * mlqem_hip.h -- C ABI of libmlqem_hip.so, the MI355X (gfx950) implementation of the ml-qem
 * expectation-value-regressor hot path.
 *
 * The reference (qiskit-community/ml-qem) has no FFI of its own: its per-batch arithmetic is delegated to
 * torch_geometric / torch-sparse (requirements.txt:1-2).  Each entry point below therefore cites the
 * reference call site whose third-party op it replaces.  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name starts with h_ (host) ; the caller owns all buffers
 *   - fp32 data, int32 indices (int64 only where the reference hands over torch.long edge_index)
 *   - row-major matrices with an explicit leading dimension (elements, not bytes)
 *   - asynchronous on `stream` (a hipStream_t passed as void*); no allocation, no host sync, no global state
 *   - returns 0 on success, a negative MLQEM_ERR_* code otherwise (bad shape, unsupported width, launch error)
 *   - re-entrant across streams and threads
 *
 * Graph layout.  A batch of graphs is the disjoint union of its members: N nodes, graph g owns the node range
 * [graph_ptr[g], graph_ptr[g+1]).  Connectivity is held as TWO CSR structures over the edges that are not
 * self-loops: `in_ptr/in_src` groups edges by destination (forward aggregation), `out_ptr/out_dst` by source
 * (the transpose, used by the backward pass).  Self-loops are not stored as edges: `loops[i]` is the number of
 * (i,i) entries the caller's edge list had, and each layer adds the self term it needs analytically.
 */
#ifndef MLQEM_HIP_H
#define MLQEM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MLQEM_OK 0
#define MLQEM_ERR_BAD_ARG (-1)
#define MLQEM_ERR_UNSUPPORTED (-2)
#define MLQEM_ERR_LAUNCH (-3)
#define MLQEM_ERR_WORKSPACE (-4)

typedef void* mlqem_stream_t; /* hipStream_t */

#define MLQEM_ABI_VERSION 48 /* bumped whenever a signature below changes; bindings compare it at load time */
int mlqem_abi_version(void);
const char* mlqem_error_string(int code);

/* ------------------------------------------------------------------------------------------------------
 * Graph structure.  Replaces what PyG derives inside every conv from `edge_index`
 * (docs/tutorials/gnn.py:104-113 passes the raw [2,E] tensor to TransformerConv / ASAPooling;
 *  blackwater/data/loaders/exp_val.py:33 AddSelfLoops; PyG gcn_norm / get_laplacian / degree).
 * ---------------------------------------------------------------------------------------------------- */

/* Bytes of scratch mlqem_csr_build needs for a graph with N nodes and E edge-list entries. */
size_t mlqem_csr_build_workspace_bytes(int64_t N, int64_t E);

/* edge_index: [2,E] int64 row-major (row 0 = source, row 1 = destination), self-loops allowed.
 * Outputs: in_ptr[N+1], in_src[E] (only the first in_ptr[N] entries are meaningful), out_ptr[N+1], out_dst[E],
 * out_eid[E] (optional: position in in_src[] of the edge each out_dst[] entry stands for; the backward kernels of the
 * edge-softmax ops read per-edge buffers through it), loops[N].  Inside a row the original edge order is kept. */
int mlqem_csr_build(const int64_t* edge_index, int64_t E, int64_t N, int32_t* in_ptr, int32_t* in_src,
                    int32_t* out_ptr, int32_t* out_dst, int32_t* out_eid, int32_t* loops, void* workspace,
                    size_t workspace_bytes, mlqem_stream_t stream);

/* Per-node normalisation scalars of the three Family-A convolutions (docs/tutorials/01_ngem.ipynb cell [9]):
 *   gcn_dinv[i]  = (indeg[i] + 1)^-1/2                     GCNConv, add_remaining_self_loops, degree by destination
 *   sage_rinv[i] = 1 / max(indeg[i] + loops[i], 1)         SAGEConv mean over the raw in-edges (self-loops count)
 *   cheb_dinv[i] = outdeg[i]^-1/2, 0 when outdeg[i] == 0   ChebConv sym normalisation, self-loops removed, degree by source
 * Any output pointer may be NULL. */
int mlqem_graph_norms(const int32_t* in_ptr, const int32_t* out_ptr, const int32_t* loops, int64_t N,
                      float* gcn_dinv, float* sage_rinv, float* cheb_dinv, mlqem_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * CSR aggregation ("scatter-add") -- the roofline kernel.  Replaces the gather x[edge_index[0]] + scatter(...,
 * reduce='sum'|'mean') inside GCNConv / SAGEConv / ChebConv / LEConv propagate (01_ngem.ipynb cell [9];
 * docs/tutorials/gnn.py:85,92 via ASAPooling) and, on the transposed CSR, their backward.
 *
 *   agg[i,:] = rscale[i] * sum_{e in [ptr[i],ptr[i+1])} cscale[idx[e]] * x[idx[e],:]  +  dself[i] * x[i,:]
 *   out[i,:] = act( alpha * agg[i,:] + beta * z[i,:] + bias[:] )
 *
 * cscale / rscale / dself / z / bias may be NULL (meaning 1 / 1 / 0 / absent / absent).
 * ell (optional, [N,2] int32 from mlqem_ell_from_csr for the SAME ptr/idx): the first two col[] entries of every
 * row, (-1 = no such edge, bit 31 of the first = row continues in col[]).  With it the row pointer -> col -> source
 * row dependent chain of the CSR walk shortens to ell -> source row for the 99.8 % of circuit-graph rows that have
 * at most two in-edges; rows with more fall back to ptr/idx, so the result is identical with or without it.
 * Vector width: when x, out (and z) own round_up(C,4) columns per row (leading dimensions multiples of 4, bases
 * 16-byte aligned) the kernel moves 16 bytes per lane and processes the pad columns along; columns never mix, so
 * the pads may hold anything.  16-byte accesses run ~1.4x the rate of 8-byte ones here: C = 12 takes less time
 * than C = 10, so the host lays every activation out with a padded leading dimension.
 * CONTRACT: with 16-byte-aligned rows the columns C .. round_up(C,4)-1 of `out` ARE WRITTEN (scratch values).  A
 * caller whose `out` is a column slice of a wider matrix must pass an unaligned base / a leading dimension that is
 * not a multiple of 4, or use a padded buffer; the Python binding refuses such slices (ops._owns_pad_columns).
 * Dropout mask (drop_p > 0): one splitmix64 hash per GROUP OF FOUR columns of a row, keyed by
 * (seed [+ seed_counter], i * C + (c & ~3)); element (i, c) is dropped when 16-bit field (c & 3) of its group's hash is below
 * floor(drop_p * 65536).  The mask of a (seed, row, column) depends on C alone: not on leading dimensions, alignment or the
 * vector width the launcher picks for them.
 * seed_counter (may be NULL): a device-resident uint64 added (times an odd constant) to `seed` when the dropout mask is
 * drawn -- a launch captured in a hipGraph then draws a fresh mask on every replay as the caller bumps the counter.  Every
 * entry point that takes a seed_counter mixes it in this way; mlqem_linear_f32 takes none (see there).
 * ---------------------------------------------------------------------------------------------------- */
int mlqem_csr_aggregate_f32(const float* x, int64_t ldx, const int32_t* ptr, const int32_t* idx, const int32_t* ell,
                            const float* cscale, const float* rscale, const float* dself, float alpha, float beta,
                            const float* z, int64_t ldz, const float* bias, int act, float drop_p, uint64_t seed,
                            const uint64_t* seed_counter, float* out, int64_t ldo, int64_t N, int C, mlqem_stream_t stream);

/* mlqem_csr_aggregate_f32 AND the pooled means of its output (mlqem_segment_pool_f32 of `out` with `pool_weights`) from ONE
 * pass: the aggregation's workgroups keep their rows of the output in LDS and leave per-(tile, graph) partial sums, added in
 * tile order by the pool's finish kernel (deterministic).  Replaces the last hidden layer of a Family A branch followed by
 * global_mean_pool (01_ngem.ipynb cell [9]; DESIGN section 3: the last conv is folded into the pool) without reading the
 * [N, C] activation a second time.  out_mean / out_wmean: [B, C] (either may be NULL).  Needs the ELL side table and rows of
 * round_up(C, 4) floats (MLQEM_ERR_UNSUPPORTED otherwise: call the two entry points).  gate_bits (optional,
 * mlqem_csr_aggregate_pool_gate_bytes(N, C) bytes, 16-byte aligned): the signs of `out` -- the ReLU / dropout gate
 * mlqem_segment_pool_bwd_f32 applies -- in the launch's own tiling: with R = the rows of a workgroup's tile (512 / ceil(C / 4))
 * and T = ceil(N / R) tiles, first T 16-byte records int32 (graph of the tile's first row, that graph's first row, the next
 * graph's first row, 0), then T x 32 uint64 words: the items (row, 16-byte column slice) of a tile are numbered row-major,
 * item i = 256 k + 64 w + l sets bit l of word (4 k + w) 4 + v of its tile iff out[row, 4 slice + v] > 0 (per-wave ballots: ABI
 * 25; a byte per item until 24); then, for C <= 16 (ABI 36), ceil(N / 2) uint32 words holding the same signs PER NODE, 16 bits each:
 * bit 4 slice + v of node i = out[i, 4 slice + v] > 0 -- what mlqem_pooled_grad_aggregate_f32 gathers.  With gate_bits `out` may be NULL -- a pooled activation whose only other reader is that gate
 * (the last hidden layer of a Family A branch) is then never written to memory.  workspace:
 * mlqem_csr_aggregate_pool_workspace_bytes(N, B, C). */
size_t mlqem_csr_aggregate_pool_workspace_bytes(int64_t N, int64_t B, int C);
size_t mlqem_csr_aggregate_pool_gate_bytes(int64_t N, int C);
int mlqem_csr_aggregate_pool_f32(const float* x, int64_t ldx, const int32_t* ptr, const int32_t* idx, const int32_t* ell,
                                 const float* cscale, const float* rscale, const float* dself, float alpha, float beta,
                                 const float* z, int64_t ldz, const float* bias, int act, float drop_p, uint64_t seed,
                                 const uint64_t* seed_counter, float* out, int64_t ldo, int64_t N, int C,
                                 const float* pool_weights, const int32_t* graph_ptr, int64_t B, float* out_mean,
                                 int64_t ld_mean, float* out_wmean, int64_t ld_wmean, uint8_t* gate_bits, void* workspace,
                                 size_t workspace_bytes, mlqem_stream_t stream);

/* Segment max with the node itself included: out[i,:] = max(x[i,:], max_e x[idx[e],:])
 * (ASAPooling's scatter(..., reduce='max') after add_remaining_self_loops; docs/tutorials/gnn.py:85,92). */
int mlqem_csr_segment_max_f32(const float* x, int64_t ldx, const int32_t* ptr, const int32_t* idx, const int32_t* ell,
                              float* out, int64_t ldo, int64_t N, int C, mlqem_stream_t stream);

/* ell[i] = (col[ptr[i]], col[ptr[i]+1]) with the conventions above; ell: [N,2] int32, 8-byte aligned. */
int mlqem_ell_from_csr(const int32_t* ptr, const int32_t* idx, int64_t N, int32_t* ell, mlqem_stream_t stream);

/* BatchNorm1d in training mode over [N, C] rows: the bn1 / bn2 of MLP2 / MLP3 (docs/tutorials/mlp.py:45-66,87-108) and its
 * autograd; replaces torch.nn.BatchNorm1d's forward / backward kernels for that call site (C <= 256).
 *   forward:  mean[C], var[C] (biased), invstd[C] = rsqrt(var + eps), y = (x - mean) * invstd * gamma + beta
 *   backward: dbeta = sum dy, dgamma = sum dy * xhat, dx = gamma * invstd * (dy - dbeta / N - xhat * dgamma / N)
 * gamma / beta may be NULL (no affine).  Deterministic (per-workgroup partials summed in a fixed order, in double).  The
 * running statistics (momentum, unbiased variance) are the caller's: they are [C]-sized host-side bookkeeping. */
size_t mlqem_batch_norm_workspace_bytes(int64_t N, int C);
int mlqem_batch_norm_train_f32(const float* x, int64_t ldx, int64_t N, int C, const float* gamma, const float* beta, float eps,
                               float* y, int64_t ldy, float* mean, float* var, float* invstd, void* workspace,
                               size_t workspace_bytes, mlqem_stream_t stream);
int mlqem_batch_norm_train_bwd_f32(const float* dy, int64_t ldg, const float* x, int64_t ldx, int64_t N, int C,
                                   const float* gamma, const float* mean, const float* invstd, float* dx, int64_t lddx,
                                   float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes,
                                   mlqem_stream_t stream);

/* BatchNorm1d with statistics shared by the ranks of a process group (torch.nn.SyncBatchNorm semantics, ABI 44): the bn1 / bn2 of a
 * converted MLP2 / MLP3 under data parallelism (docs/tutorials/mlp.py:45-66,87-108).  The finish of the two calls above is split in
 * two around ONE all-reduce(SUM) that the caller runs over a [world][2 C + 1] double buffer in which rank r filled row r (the other
 * rows zero, so the sum is exact and every rank receives the same records bit for bit):
 *   record    mode 0: [n_r | mean_r[C] | M2_r[C]] of this rank's rows x (per-workgroup sums shifted by row 0, finished in double).
 *             mode 1: [n_r | sum dy[C] | sum dy xhat[C]] with xhat from the GLOBAL mean / invstd of the forward; this rank's
 *             dgamma / dbeta (the local sums: the gradient all-reduce averages them like any parameter gradient).
 *   train     records -> mean, biased var, invstd over the union of the ranks' rows (Chan's pairwise merge in rank order), y for
 *             this rank's rows, and (running_mean / running_var / num_batches_tracked, each optional, both buffers or neither) the
 *             running update with the global N: running_var <- (1 - momentum) running_var + momentum var N / (N - 1).
 *   train_bwd records -> dx = gamma invstd (dy - sum_r dbeta_r / N - xhat sum_r dgamma_r / N) for this rank's rows.
 * Same workspace as mlqem_batch_norm_train_f32 (C <= 256); deterministic, no atomics, no allocation, no host synchronisation. */
int mlqem_batch_norm_sync_record_f32(int mode, const float* x, int64_t ldx, const float* dy, int64_t ldg, const float* mean,
                                     const float* invstd, int64_t N, int C, double* record, float* dgamma, float* dbeta,
                                     void* workspace, size_t workspace_bytes, mlqem_stream_t stream);
int mlqem_batch_norm_sync_train_f32(const double* records, int world, const float* x, int64_t ldx, int64_t N, int C,
                                    const float* gamma, const float* beta, float eps, float* y, int64_t ldy, float* mean, float* var,
                                    float* invstd, float* running_mean, float* running_var, float momentum,
                                    int64_t* num_batches_tracked, void* workspace, size_t workspace_bytes, mlqem_stream_t stream);
int mlqem_batch_norm_sync_train_bwd_f32(const double* records, int world, const float* dy, int64_t ldg, const float* x, int64_t ldx,
                                        int64_t N, int C, const float* gamma, const float* mean, const float* invstd, float* dx,
                                        int64_t lddx, void* workspace, size_t workspace_bytes, mlqem_stream_t stream);

/* ----------------------------------------------------------------------------------------------------
 * The two ends of a train step that are not model layers (docs/tutorials/__ml_models.py:100-187:
 * `loss = criterion(out, y); loss.backward(); optimizer.step()` with torch.nn.MSELoss and torch.optim.Adam).
 *
 * mlqem_mse_loss_grad_f32: *loss = mean over the N x C elements of (out - y)^2 and, when g is given,
 *   g = 2 (out - y) / (N C) -- the gradient `loss.backward()` hands to the model's output -- from one pass, one launch; g has
 *   g_rows >= N rows, the rows beyond N (filler rows of a padded batch, which the loss does not see) come out zero;
 *   per-workgroup partial sums added in index order by the workgroup that finishes last (deterministic).
 *   workspace: mlqem_mse_loss_workspace_bytes(); ticket: one zero-initialised unsigned the call leaves at zero.
 * mlqem_adam_step_f32: torch.optim.Adam(betas, eps; amsgrad = False, weight_decay = 0, maximize = False) on ONE flat
 *   buffer of n floats: step <- step + 1; m <- lerp(m, g, 1 - beta1); v <- beta2 v + (1 - beta2) g^2;
 *   p <- p - lr / (1 - beta1^step) * m / (sqrt(v) / sqrt(1 - beta2^step) + eps)  (betas arrive as doubles: 1 - beta and the bias
 *   corrections are formed in double, as torch forms them, the update itself in fp32).  `lr` and `step` (a float, as torch keeps
 *   it) live on the device, so the launch can sit in a captured hipGraph and a scheduler can change the rate between
 *   replays; ticket as above; bump_counter (optional, ABI 42): a device counter the launch's last workgroup increments -- the
 *   trainers' dropout step counter, so that a step needs no launch of its own for it.  Replaces torch's multi-tensor kernel, which runs a buffer of this path's size (1.8 k-180 k
 *   floats) on one workgroup.
 * ---------------------------------------------------------------------------------------------------- */
size_t mlqem_mse_loss_workspace_bytes(void);
int mlqem_mse_loss_grad_f32(const float* out, int64_t ldo, const float* y, int64_t ldy, float* g, int64_t ldg, int64_t N, int C,
                            int64_t g_rows, float* loss, void* workspace, size_t workspace_bytes, unsigned* ticket, mlqem_stream_t stream);
int mlqem_adam_step_f32(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, const float* lr,
                        float* step, double beta1, double beta2, double eps, unsigned* ticket, uint64_t* bump_counter,
                        mlqem_stream_t stream);

/* nn.Sequential(Linear(I, H), [Dropout(p)], Linear(H, O)) as ONE launch per direction: y = dropout(x W1^T + b1) W2^T + b2.
 * Replaces `self.obs_seq(observable)` and `self.body_seq(merged)` of the graph models (01_ngem.ipynb cell [9]; docs/tutorials/
 * gnn.py:94-98,121): heads that see one row per circuit, where every separate GEMM / bias / dropout / weight-gradient launch is
 * pure launch latency.  w1: [H, I], w2: [O, H] row-major (torch's Linear.weight); H <= 16, O <= 8 (MLQEM_ERR_UNSUPPORTED beyond).
 *   forward:  hidden [N, H] = the dropped, rescaled first-layer output (NULL at inference), mask [N] = bit j set when hidden unit
 *             j of the row was kept (required with drop_p > 0 and hidden), y [N, O]; mask keyed by (seed [+ seed_counter], n H + j).
 *   backward: gw1 [H, I], gb1 [H], gw2 [O, H], gb2 [O] (gb1 / gb2 may be NULL) and, when gx is given, gx [N, I] = the gradient of
 *             the input; the row slices of a workgroup meet in LDS and are added in slice order (deterministic, one launch);
 *             workspace / ticket: reserved for a two-stage form (mlqem_seq2_backward_workspace_bytes returns 0; both may be NULL). */
int mlqem_seq2_forward_f32(const float* x, int64_t ldx, int64_t N, int I, const float* w1, const float* b1, int H, const float* w2,
                           const float* b2, int O, float drop_p, uint64_t seed, const uint64_t* seed_counter, float* hidden,
                           uint32_t* mask, float* y, int64_t ldy, mlqem_stream_t stream);
size_t mlqem_seq2_backward_workspace_bytes(int64_t N, int I, int H, int O);
int mlqem_seq2_backward_f32(const float* gy, int64_t ldgy, const float* x, int64_t ldx, int64_t N, int I, const float* w1, int H,
                            const float* w2, int O, const float* hidden, const uint32_t* mask, float drop_p, float* gx, int64_t ldgx,
                            float* gw1, float* gb1, float* gw2, float* gb2, void* workspace, size_t workspace_bytes, unsigned* ticket,
                            mlqem_stream_t stream);

/* gx[n,c] = (y[n,c] > 0) ? g[n,c] * scale : 0  -- backward of ReLU followed by inverted dropout, recovered from the
 * output y (an element that was clamped OR dropped has y == 0 and no gradient either way). */
int mlqem_relu_dropout_bwd_f32(const float* g, int64_t ldg, const float* y, int64_t ldy, float scale, float* gx,
                               int64_t ldgx, int64_t N, int C, mlqem_stream_t stream);

/* y = dropout(relu(x)) (inverted dropout with the mask of mlqem_csr_aggregate_f32's epilogue: one hash per group of four columns,
 * keyed by (seed [+ seed_counter], n*C + (c & ~3)), field c & 3 -- whatever the operands' layout) and, when residual is given,
 * sum = y + residual in the same pass -- the element-wise tail of an MLP2 / MLP3 trunk layer (docs/tutorials/mlp.py:60-66:
 * x1 = drop(relu(bn1(fc1 x))), x2 = drop(relu(bn2(fc2 x1))), x1 + x2) as ONE launch.  y is what the backward needs
 * (mlqem_relu_dropout_bwd_f32 recovers the mask from it); sum may be NULL; seed_counter as in mlqem_csr_aggregate_f32. */
int mlqem_relu_dropout_f32(const float* x, int64_t ldx, float drop_p, uint64_t seed, const uint64_t* seed_counter,
                           const float* residual, int64_t ldr, float* y, int64_t ldy, float* sum, int64_t lds, int64_t N, int C,
                           mlqem_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Dense layers.  Replace torch.nn.Linear / torch_geometric.nn.Linear (docs/tutorials/gnn.py:94-98 body_seq,
 * docs/tutorials/mlp.py:18-108 MLP1/2/3, the per-node projections inside every conv).
 * ---------------------------------------------------------------------------------------------------- */

/* y[n,:] = drop( act( (x[n,:] @ W^T + b [+ y[n,:] if accumulate]) * rowscale[n] ) ),  W: [O,I] row-major as torch
 * stores it (transposed = 0), or the same with x @ W, W: [I,O] (transposed = 1: the data-gradient form gx = gy @ W).
 * b and rowscale may be NULL.  accumulate chains several calls into one sum of products (ChebConv's sum_k lins[k](T_k),
 * SAGEConv's lin_l(mean) + lin_r(x)); the activation belongs on the last call.  act bit 0 = ReLU; drop_p > 0 applies
 * inverted dropout keyed by (seed, n*O + o), one hash per ELEMENT (not the aggregation epilogue's mask).  This entry point takes NO
 * seed_counter: a launch of it captured in a hipGraph repeats its mask on every replay (ChebConv with K = 1 or K > 3 puts its
 * dropout here; the reference configuration, K = 3 / 2, does not).  Column ranges: rowscale applies to outputs o < rs_cols and ReLU/dropout to
 * outputs o >= act_from (-1, -1 = every column), so that one launch can serve several layers that read the same input
 * rows (the three first-layer projections of GCN | Cheb | SAGE).  gate (may be NULL), applied last:
 * y[n,o] = gate[n,o] > 0 ? y[n,o] * gate_scale : 0 -- the backward of a ReLU/dropout epilogue whose output `gate` is this
 * layer's input, folded into the data-gradient GEMM that produces the incoming gradient (no separate masking pass).
 * x_rows (may be NULL): row n of x is row x_rows[n] of the buffer -- the first layers read their input rows straight
 * from the device-resident dataset through the batch's row map (src_node of mlqem_batch_assemble) instead of from a
 * gathered copy; only for calls the lean kernel can express (padded operands, I, O <= 64, no accumulate), else
 * MLQEM_ERR_UNSUPPORTED.
 * Runs on the f32-input matrix cores (v_mfma_f32_16x16x4_f32) for I <= 128. */
int mlqem_linear_f32(const float* x, int64_t ldx, const float* w, int transposed, const float* b,
                     const float* rowscale, float* y, int64_t ldy, int64_t N, int I, int O, int act, int accumulate,
                     float drop_p, uint64_t seed, int rs_cols, int act_from, const float* gate, int64_t ldgate,
                     float gate_scale, const int32_t* x_rows, mlqem_stream_t stream);

/* y = act(x @ W^T + b) (transposed = 0, W: [O, I]) or y = x @ W (transposed = 1, W: [I, O]: the data-gradient form) with
 * both operands rounded to bf16 (nearest-even) in registers and fp32 accumulation on v_mfma_f32_16x16x32_bf16: the "bf16
 * MFMA MLP head" option of the MLP regressors (docs/tutorials/mlp.py:18-108) for BASELINE.json's mixed-corpus
 * configuration.  x, W, y are fp32 in memory; b may be NULL; act bit 0 = ReLU; I <= 256. */
int mlqem_linear_bf16_f32(const float* x, int64_t ldx, const float* w, int transposed, const float* b, float* y, int64_t ldy,
                          int64_t N, int I, int O, int act, mlqem_stream_t stream);

/* gw[o,i] (+)= sum_n bf16(gy[n,o]) * bf16(x[n,i]);  gb[o] (+)= sum_n bf16(gy[n,o])  on the same matrix cores (32 rows per
 * MFMA, fp32 accumulation, deterministic two-stage reduction): with the two entry points above the bf16 head trains
 * end to end on v_mfma_f32_16x16x32_bf16.  workspace: mlqem_linear_wgrad_workspace_bytes(I, O). */
int mlqem_linear_wgrad_bf16_f32(const float* gy, int64_t ldgy, const float* x, int64_t ldx, float* gw, float* gb, int64_t N,
                                int I, int O, int accumulate, void* workspace, size_t workspace_bytes, mlqem_stream_t stream);

#define MLQEM_MAX_COL_PARTS 8

/* A matrix given as up to MLQEM_MAX_COL_PARTS COLUMN BLOCKS in separate buffers: block p is ptr[p][N, cols] (row stride ld[p]) and
 * stands at columns [p*width, p*width + cols) of the concatenation; columns cols..width-1 of a block are padding (read
 * as 0, written as scratch).  For mlqem_linear_parts_f32 width and every ld must be multiples of 4 and every ptr 16-byte
 * aligned (the padded activation layout). */
typedef struct mlqem_col_parts {
  int32_t count, width, cols, reserved;
  void* ptr[MLQEM_MAX_COL_PARTS];
  int64_t ld[MLQEM_MAX_COL_PARTS];
} mlqem_col_parts;

/* Projections over column blocks, the blocks on ONE side:
 *   transposed = 0, fan-out (x->count == 1):  Y_k = X W_k^T + b_k        W_k = w_blocks[k]: [y->cols, x->cols]
 *   transposed = 1, fan-in  (y->count == 1):  Y   = sum_k X_k W_k        W_k = w_blocks[k]: [x->cols, y->cols]
 * Weight blocks are row-major and unpadded, exactly as the layers store them; w_minus_blocks[k] (array or entries may
 * be NULL) is subtracted element-wise from W_k (the Clenshaw form of ChebConv multiplies by W_0 - W_2);
 * bias_blocks[k] (fan-out only, may be NULL): [y->cols]; rowscale_blocks[k] (fan-out only, may be NULL): [N], block k's
 * rows are multiplied by it after the bias (GCNConv's D^-1/2 pre-scaling).  One launch replaces
 *   - the per-term projections of ChebConv / SAGEConv that read the same input rows (lins[k](x), lin_l(x), lin_r(x);
 *     01_ngem.ipynb cell [9]) and
 *   - the sum of per-term data gradients (gx = sum_k g_k W_k)
 * without building the concatenation, whose wide rows would slow the aggregation gathers.  Concatenated width of the
 * input side <= 64 columns.  gate / gate_scale as in mlqem_linear_f32 (fan-in; gate rows padded like Y's). */
int mlqem_linear_parts_f32(const mlqem_col_parts* x, const float* const* w_blocks, const float* const* w_minus_blocks,
                           int transposed, const float* const* bias_blocks, const float* const* rowscale_blocks,
                           const mlqem_col_parts* y, int64_t N, const float* gate, int64_t ldgate, float gate_scale,
                           const int32_t* x_rows, mlqem_stream_t stream);

#define MLQEM_FANOUT_MAX_TABLES 3

/* The fan-out over up to MLQEM_FANOUT_MAX_TABLES INPUT TABLES that share one row map: table[j] is [M, cols] in the padded row
 * layout (ldt % 4 == 0, 16-byte aligned), row n of every input is row x_rows[n] of its table (x_rows == NULL: row n).  The tables
 * are the node features x and products of a graph operator with them that are constants of the dataset (A^ x of GCNConv, L^ x of
 * ChebConv), so that a first layer's aggregation of its projection becomes a projection of the aggregated input.  Output block k
 * (y[k]: [N, out_cols], padded rows) is
 *     Y_k = act((T[w_table[k]] (w[k] - w_minus[k])^T + T[w2_table[k]] (w2_scale[k] * w2[k])^T + bias[k]) * rowscale[k])
 * with the second term, w_minus, bias and rowscale optional (NULL); weights [out_cols, cols] row-major as the layers store them.
 * act[k] != 0: ReLU, then inverted dropout (drop_p > 0) with the mask of mlqem_csr_aggregate_f32's epilogue for C = out_cols -- one
 * hash per group of four columns keyed by n * out_cols + (column & ~3), field column & 3, seed + *seed_counter * 0xD1B54A32D192ED03
 * (seed_counter may be NULL); the key uses the block's logical width, not its leading dimension.  At most
 * MLQEM_MAX_COL_PARTS blocks and as many terms in all; 17 <= cols <= 24, out_cols <= 16 (else MLQEM_ERR_UNSUPPORTED).  Blocks of
 * one term carry the values mlqem_linear_parts_f32 writes for them, bit for bit. */
typedef struct mlqem_fanout_tables {
  int32_t n_tables, n_blocks, cols, out_cols;
  const void* table[MLQEM_FANOUT_MAX_TABLES];
  int64_t ldt[MLQEM_FANOUT_MAX_TABLES];
  void* y[MLQEM_MAX_COL_PARTS];
  int64_t ldy[MLQEM_MAX_COL_PARTS];
  const float* w[MLQEM_MAX_COL_PARTS];
  const float* w_minus[MLQEM_MAX_COL_PARTS];
  const float* w2[MLQEM_MAX_COL_PARTS];
  const float* bias[MLQEM_MAX_COL_PARTS];
  const float* rowscale[MLQEM_MAX_COL_PARTS];
  float w2_scale[MLQEM_MAX_COL_PARTS];
  int32_t w_table[MLQEM_MAX_COL_PARTS], w2_table[MLQEM_MAX_COL_PARTS], act[MLQEM_MAX_COL_PARTS];
} mlqem_fanout_tables;
int mlqem_linear_fanout_tables_f32(const mlqem_fanout_tables* d, int64_t N, const int32_t* x_rows, float drop_p, uint64_t seed,
                                   const uint64_t* seed_counter, mlqem_stream_t stream);

/* The same launch with a CHAINED projection on one of its blocks (an additive symbol, the ABI version is unchanged): after block
 * `block`'s epilogue (bias, row scale, ReLU, dropout) the values a lane holds are the operand of a second product,
 *     Y2 = (Y_block W2^T) * rowscale2            W2: [out_cols, d->out_cols] row-major, out_cols <= 12, rowscale2 optional (NULL)
 * written to y ([N, out_cols], padded rows) by the same launch -- the layer above is projected from registers instead of from a
 * second pass over Y_block (GCN conv2's dinv * (h1 W2^T) from conv1's activation).  Y_block and every other block carry the values
 * of mlqem_linear_fanout_tables_f32, bit for bit; Y2 is the k-ordered fp32 chain over Y_block's d->out_cols columns.
 * chain == NULL is mlqem_linear_fanout_tables_f32. */
typedef struct mlqem_fanout_chain {
  int32_t block, out_cols;
  void* y;
  int64_t ldy;
  const float* w;
  const float* rowscale;
} mlqem_fanout_chain;
int mlqem_linear_fanout_tables_chain_f32(const mlqem_fanout_tables* d, const mlqem_fanout_chain* chain, int64_t N,
                                         const int32_t* x_rows, float drop_p, uint64_t seed, const uint64_t* seed_counter,
                                         mlqem_stream_t stream);

#define MLQEM_FANOUT_POOL_MAX_TABLES 5
#define MLQEM_FANOUT_POOL_MAX_TERMS 3
#define MLQEM_FANOUT_POOL_BLOCKS 3

/* The fan-out with POOLED blocks: up to MLQEM_FANOUT_POOL_MAX_TABLES tables that share one row map (layout and row map as in
 * mlqem_fanout_tables), block k the sum of n_terms[k] <= MLQEM_FANOUT_POOL_MAX_TERMS projections
 *     V_k = act_k(sum_t T[w_table[k][t]] (w_scale[k][t] * (w[k][t] - w_minus[k][t]))^T + bias[k]) * rowscale[k]
 * with its OWN dropout probability drop_p[k] and seed seed[k] (mask and seed counter as in mlqem_linear_fanout_tables_f32).
 * Block 0 is stored (y[0]) and may carry the chain of mlqem_linear_fanout_tables_chain_f32 (chain->block == 0, or chain == NULL): its
 * values and the chain's are those of that entry point, bit for bit.  Blocks 1 and 2 are pooled: the launch leaves
 *     out_mean[k][g] = (1/n_g) sum_{r in g} V_k[r]      out_wmean[k][g] = (1/n_g) sum_r pool_weights[k][r] V_k[r]     ([B, out_cols])
 * over the row ranges graph_ptr[g] .. graph_ptr[g + 1] (graph_ptr[B] == N), and in gate_bits[k] the per-node sign bits of V_k in the
 * per-node section of the gate buffer of mlqem_csr_aggregate_pool_f32 (mlqem_csr_aggregate_pool_gate_bytes(N, out_cols) bytes; 16 bits
 * a node, bit 4 slice + v = V_k[node][4 slice + v] > 0).  The tile records and ballots of that buffer are NOT written: it serves the
 * readers of the per-node section (mlqem_pooled_grad_*, mlqem_linear_wgrad_tables_f32), not mlqem_segment_pool_bwd_f32.  y[k] of a
 * pooled block is optional: with it V_k is stored as well (tests; a pooled block's values otherwise never reach memory).
 * The sums are deterministic and do not depend on the grid: a wave owns 256 consecutive rows at a time and leaves one partial per
 * (tile, graph) in the workspace (pool layout), added in tile order by the pool's finish kernel.  max_groups > 0 caps the grid (tests).
 * Exactly MLQEM_FANOUT_POOL_BLOCKS blocks (else MLQEM_ERR_UNSUPPORTED); 17 <= cols <= 24, out_cols <= 16; out_cols <= 12 with a chain. */
typedef struct mlqem_fanout_pool {
  int32_t n_tables, n_blocks, cols, out_cols;
  const void* table[MLQEM_FANOUT_POOL_MAX_TABLES];
  int64_t ldt[MLQEM_FANOUT_POOL_MAX_TABLES];
  int32_t n_terms[MLQEM_FANOUT_POOL_BLOCKS];
  int32_t max_groups;
  const float* w[MLQEM_FANOUT_POOL_BLOCKS][MLQEM_FANOUT_POOL_MAX_TERMS];
  const float* w_minus[MLQEM_FANOUT_POOL_BLOCKS][MLQEM_FANOUT_POOL_MAX_TERMS];
  float w_scale[MLQEM_FANOUT_POOL_BLOCKS][MLQEM_FANOUT_POOL_MAX_TERMS];
  int32_t w_table[MLQEM_FANOUT_POOL_BLOCKS][MLQEM_FANOUT_POOL_MAX_TERMS];
  const float* bias[MLQEM_FANOUT_POOL_BLOCKS];
  const float* rowscale[MLQEM_FANOUT_POOL_BLOCKS];
  int32_t act[MLQEM_FANOUT_POOL_BLOCKS];
  float drop_p[MLQEM_FANOUT_POOL_BLOCKS];
  uint64_t seed[MLQEM_FANOUT_POOL_BLOCKS];
  void* y[MLQEM_FANOUT_POOL_BLOCKS];
  int64_t ldy[MLQEM_FANOUT_POOL_BLOCKS];
  const float* pool_weights[MLQEM_FANOUT_POOL_BLOCKS];       /* entries 1 and 2 */
  float* out_mean[MLQEM_FANOUT_POOL_BLOCKS];
  int64_t ld_mean[MLQEM_FANOUT_POOL_BLOCKS];
  float* out_wmean[MLQEM_FANOUT_POOL_BLOCKS];
  int64_t ld_wmean[MLQEM_FANOUT_POOL_BLOCKS];
  uint8_t* gate_bits[MLQEM_FANOUT_POOL_BLOCKS];
  const int32_t* graph_ptr;
  int64_t num_graphs;
} mlqem_fanout_pool;
size_t mlqem_linear_fanout_pool_workspace_bytes(int64_t N, int64_t B, int out_cols);
int mlqem_linear_fanout_pool_f32(const mlqem_fanout_pool* d, const mlqem_fanout_chain* chain, int64_t N, const int32_t* x_rows,
                                 const uint64_t* seed_counter, void* workspace, size_t workspace_bytes, mlqem_stream_t stream);

size_t mlqem_linear_wgrad_workspace_bytes(int I, int O);

/* gw[o,i] (+)= sum_n gy[n,o] * x[n,i] ;  gb[o] (+)= sum_n gy[n,o]  (gb may be NULL).  Matrix-core partial sums per
 * workgroup, then a fixed-order reduction: deterministic.  x_rows (may be NULL): row map for x as in mlqem_linear_f32. */
int mlqem_linear_wgrad_f32(const float* gy, int64_t ldgy, const float* x, int64_t ldx, float* gw, float* gb,
                           int64_t N, int I, int O, int accumulate, void* workspace, size_t workspace_bytes,
                           const int32_t* x_rows, mlqem_stream_t stream);

/* The same with gy given as column blocks (O = gy->count * gy->width rows of gw / entries of gb, padding rows are 0):
 * the weight gradients of all terms that share the input x in one pass over x. */
int mlqem_linear_wgrad_parts_f32(const mlqem_col_parts* gy, const float* x, int64_t ldx, float* gw, float* gb, int64_t N,
                                 int I, int accumulate, void* workspace, size_t workspace_bytes, const int32_t* x_rows,
                                 mlqem_stream_t stream);

#define MLQEM_WGRAD_MAX_TABLES 4

/* The weight gradients of TWO gradient blocks against up to MLQEM_WGRAD_MAX_TABLES tables that share one row map, in one pass
 * (an additive symbol, the ABI version is unchanged): table[t] is [M, cols] in the padded row layout with the common leading
 * dimension ldt, row n of every table is row rows[n] (rows == NULL: row n); 16 <= cols <= 31, out_cols <= 16 (else
 * MLQEM_ERR_UNSUPPORTED).  image: [2][16][n_tables][32] floats,
 *     image[b][o][t][i]    = sum_n g_b[n, o] * table[t][rows[n], i]      i < cols
 *     image[b][o][t][cols] = sum_n g_b[n, o]                             (the ones column)
 * every other entry 0 (a pair that pair_mask leaves out: all of its entries).  Pad columns of the tables and of the blocks are not read.  synth == 0: block b is the matrix g[b]
 * ([N, out_cols], leading dimension ldg[b]).  synth != 0: block b is NOT read but computed per element, as
 * mlqem_segment_pool_bwd_f32(gate_bits=) writes it -- gate_bits[b] (the buffer a pooled aggregation of N rows and out_cols columns
 * left), weights[b], g_mean[b] / g_wmean[b] ([num_graphs, >= round_up(out_cols, 4)], either may be NULL), gate_scale[b], graph_ptr
 * -- and the image is bit-equal to the one of the written matrices.  Matrix-core partial sums per workgroup over contiguous row
 * ranges, then a fixed-order reduction: deterministic.  workspace: mlqem_linear_wgrad_tables_workspace_bytes(n_tables). */
typedef struct mlqem_wgrad_tables {
  int32_t n_tables, cols, out_cols, synth;
  const void* table[MLQEM_WGRAD_MAX_TABLES];
  int64_t ldt;
  const float* g[2];
  int64_t ldg[2];
  const void* gate_bits[2];
  const float* weights[2];
  const float* g_mean[2];
  int64_t ld_gmean[2];
  const float* g_wmean[2];
  int64_t ld_gwmean[2];
  float gate_scale[2];
  const int32_t* graph_ptr;
  int64_t num_graphs;
  uint32_t pair_mask; /* bit b * MLQEM_WGRAD_MAX_TABLES + t: the product of block b with table t is wanted; 0: all of them */
} mlqem_wgrad_tables;
size_t mlqem_linear_wgrad_tables_workspace_bytes(int n_tables);
int mlqem_linear_wgrad_tables_f32(const mlqem_wgrad_tables* d, const int32_t* rows, int64_t N, float* image, void* workspace,
                                  size_t workspace_bytes, mlqem_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * The MLP regressor as one forward and one backward launch.  Replaces MLP1.forward and its autograd
 * (docs/tutorials/mlp.py:18-30 == blackwater/library/learning/mlp.py: fc2(relu(fc1(x))); trained by h10_mlp.ipynb cells
 * [10]-[13] on a plain feature matrix, so x needs no gradient).  I <= MLQEM_MLP1_MAX_IN inputs, H <= 128 hidden units,
 * O2 <= MLQEM_MLP1_MAX_OUT outputs; x rows padded to a multiple of 4 floats and 16-byte aligned (ldx % 4 == 0).
 *   forward : h = relu(x W1^T + b1) ; out = h W2^T + b2.  h_stash (optional, [N, MLQEM_MLP1_HIDDEN_PAD], 16-byte aligned)
 *             receives h for the backward: fp32 when bf16 == 0, bf16 (2 bytes per element) when bf16 != 0.
 *   backward: gW1 = gh^T x, gb1 = sum gh, gW2 = gout^T h, gb2 = sum gout with gh = (gout W2) o (h > 0), from ONE pass
 *             over x and the stash; per-workgroup partial sums, fixed-order second stage (deterministic).
 * bf16 == 0: exact fp32 on v_mfma_f32_16x16x4_f32.  bf16 != 0: every GEMM operand rounded to bf16 (nearest-even), fp32
 * accumulation on v_mfma_f32_16x16x32_bf16, the stash kept in bf16 (the "bf16 MFMA MLP head" of the mixed-corpus
 * configuration); gb2 is summed from the unrounded gout.  workspace (both calls; 16-byte aligned): mlqem_mlp1_workspace_bytes(I, O2) -- the
 * forward keeps the W1 fragment image its workgroups copy into LDS there, the backward its partial sums; a forward and a
 * backward on one stream may share it.
 *   The training cell's `loss = MSELoss()(out, y); loss.backward()` (docs/tutorials/__ml_models.py:148-160) folded in: with
 *   `target` [N, O2] the forward also writes gout = 2 (out - target) / (N O2) -- the gradient the backward call takes -- and
 *   leaves its per-workgroup sums of (out - target)^2 in the workspace; the NEXT backward call on the same workspace then
 *   writes *loss_out = mean (out - target)^2 (fixed summation order).  target == NULL / loss_out == NULL: neither. */
#define MLQEM_MLP1_HIDDEN_PAD 128
#define MLQEM_MLP1_MAX_OUT 4
#define MLQEM_MLP1_MAX_IN 175
size_t mlqem_mlp1_workspace_bytes(int I, int O2);
int mlqem_mlp1_forward(const float* x, int64_t ldx, const float* w1, const float* b1, const float* w2, const float* b2,
                       void* h_stash, float* out, int64_t ldo, int64_t N, int I, int H, int O2, int bf16, const float* target,
                       int64_t ldt, float* gout, int64_t ldg, void* workspace, size_t workspace_bytes, mlqem_stream_t stream);
int mlqem_mlp1_backward(const float* gout, int64_t ldg, const float* x, int64_t ldx, const void* h_stash, const float* w2,
                        float* gw1, float* gb1, float* gw2, float* gb2, int64_t N, int I, int H, int O2, int bf16,
                        float* loss_out, void* workspace, size_t workspace_bytes, mlqem_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * MLP2 / MLP3 with bf16 STORAGE (docs/tutorials/mlp.py:33-108 == blackwater/library/learning/mlp.py: fc -> BatchNorm1d -> ReLU ->
 * Dropout blocks with a residual; `mfma = "bf16"`, the "bf16 MFMA MLP head" of the mixed-corpus configuration).  Every
 * activation matrix -- layer outputs and what the backward re-reads -- is [N, MLQEM_MLP1_HIDDEN_PAD] bf16 (256-byte rows,
 * 16-byte aligned, columns beyond the layer's width zero); weights, BatchNorm statistics, parameter gradients and all sums are
 * fp32; GEMM operands are rounded to bf16 (nearest-even) and accumulated in fp32 on v_mfma_f32_16x16x32_bf16.  Dropout masks
 * are counter-based, keyed by (seed + *seed_counter, row * 128 + column), and recomputed in the backward.  All entry points
 * take workspace = mlqem_layer_workspace_bytes() (16-byte aligned); partial sums per workgroup, fixed-order second stages.
 *   gemm      : Y = X W^T + b (transposed = 0, W [U,K]) or Y = X W (+ add) (transposed = 1, W [K,U]: the data gradient);
 *               X fp32 [N,K <= 192] (ldx floats, ldx % 4 == 0) or bf16 [N,128] (K <= 128); Y bf16 [N,128] or fp32 [N,ldy];
 *               relu / drop_p (ABI 42): Y = dropout(relu(.)) in the epilogue, mlqem_layer_gemm_f32's mask -- a block without
 *               BatchNorm (MLP3's fc3, mlp.py:96-104) in one launch; its backward gates by Y > 0 (rowdot_bwd's gate_scale).
 *   colstats 0: batch statistics of y -> mean, biased var, invstd, scale = gamma invstd, shift = beta - mean scale (outputs
 *               are [128]; columns >= C come out 0), and, when running_mean / running_var [C] are given, BatchNorm1d's
 *               update of them in the same launch (running = (1 - momentum) running + momentum batch, variance unbiased,
 *               *num_batches_tracked += 1 when given; N >= 2).
 *   colstats 1: with gu = g o (y scale + shift > 0) o keep / (1 - p): dbeta = sum gu, dgamma = sum gu xhat, gs = gamma invstd,
 *               k1 = dbeta / N, k2 = dgamma / N  (g: bf16 [N,128], or fp32 [N,ldg32] when g32 != NULL).
 *   pointwise 0: out = dropout(relu?(y scale + shift)) (+ res);   1: out = gs (gu - k1 - xhat k2)   (BatchNorm backward).
 *   wgrad     : gw [U,K] = dY^T X, gb [U] = sum dY  (X fp32 [N,K <= 175] or bf16 [N,128], K <= 128).
 *   rowdot    : the final O <= 4 outputs, out = h w^T + b; rowdot_bwd: gh = g w (bf16), gw = g^T h, gb = sum g; with gate_scale > 0
 *               gh = (h > 0 ? gate_scale : 0) g w -- h = dropout(relu(u)) of a block without BatchNorm is its own gate, gh is then
 *               the gradient at u (ABI 25). */
size_t mlqem_layer_workspace_bytes(void);
int mlqem_layer_gemm_bf16(const void* x, int x_is_bf16, int64_t ldx, const float* w, int transposed, const float* b,
                          const void* add_bf16, void* y, int y_is_f32, int64_t ldy, int relu, float drop_p, uint64_t seed,
                          const uint64_t* seed_counter, int64_t N, int K, int U, void* workspace, size_t workspace_bytes,
                          mlqem_stream_t stream);
int mlqem_layer_colstats_bf16(int mode, const void* y, const void* g, const float* g32, int64_t ldg32, const float* scale,
                              const float* shift, const float* mean, const float* invstd, const float* gamma, const float* beta,
                              float eps, int relu, float drop_p, uint64_t seed, const uint64_t* seed_counter, int64_t N, int C,
                              float* o1, float* o2, float* o3, float* o4, float* o5, float* running_mean, float* running_var,
                              float momentum, int64_t* num_batches_tracked, void* workspace, size_t workspace_bytes,
                              mlqem_stream_t stream);
int mlqem_layer_pointwise_bf16(int op, const void* y, const void* g, const float* g32, int64_t ldg32, const void* res,
                               const float* scale, const float* shift, const float* mean, const float* invstd, const float* gs,
                               const float* k1, const float* k2, int relu, float drop_p, uint64_t seed,
                               const uint64_t* seed_counter, void* out, int64_t N, int C, mlqem_stream_t stream);
int mlqem_layer_wgrad_bf16(const void* dy, const void* x, int x_is_bf16, int64_t ldx, float* gw, float* gb, int64_t N, int K, int U,
                           void* workspace, size_t workspace_bytes, mlqem_stream_t stream);
int mlqem_layer_rowdot_bf16(const void* h, const float* w, const float* b, float* out, int64_t ldo, int64_t N, int C, int O,
                            mlqem_stream_t stream);
int mlqem_layer_rowdot_bwd_bf16(const float* g, int64_t ldg, const void* h, const float* w, void* gh, float gate_scale, float* gw,
                                float* gb, int64_t N, int C, int O, void* workspace, size_t workspace_bytes, mlqem_stream_t stream);

/* The same pipeline with fp32 STORAGE (`mfma = "f32"`: the reference's own arithmetic, docs/tutorials/mlp.py:33-108 in torch's
 * default dtype): every activation matrix is [N, MLQEM_MLP1_HIDDEN_PAD] fp32 (512-byte rows, 16-byte aligned, columns beyond the
 * layer's width zero), GEMM operands are NOT rounded (v_mfma_f32_16x16x4_f32).  colstats / pointwise / rowdot / rowdot_bwd:
 * the bf16 entry points' signatures and meaning with fp32 activation matrices for y, g, res, out, h, gh (g32 stays the narrow
 * [N, ldg32] form of the incoming gradient).  Same workspace, same counter-based dropout (keyed by the first of every four columns
 * a lane owns: masks differ from the bf16 pipeline's, forward and backward of one pipeline agree).
 *   gemm_f32  : Y = X W^T + b (transposed = 0, W [U,K]) or Y = X W (+ add [N,128]) (transposed = 1, W [K,U]); X fp32 [N, ldx],
 *               K <= 192 columns used (ldx % 4 == 0; an activation matrix: ldx = 128); Y an activation matrix (y_is_act, ldy = 128,
 *               every column written) or the first U columns of [N, ldy]; U <= 128.  relu / drop_p: the epilogue of a block
 *               without BatchNorm, Y = dropout(relu(.)) (counter-based mask; its backward gates by Y > 0: rowdot_bwd's gate_scale).
 *   wgrad_f32 : gw [U,K] = dY^T X, gb [U] = sum dY; dY an activation matrix, X fp32 [N, ldx], K <= 191. */
int mlqem_layer_gemm_f32(const float* x, int64_t ldx, const float* w, int transposed, const float* b, const float* add, float* y,
                         int y_is_act, int64_t ldy, int relu, float drop_p, uint64_t seed, const uint64_t* seed_counter, int64_t N,
                         int K, int U, void* workspace, size_t workspace_bytes, mlqem_stream_t stream);
int mlqem_layer_colstats_f32(int mode, const void* y, const void* g, const float* g32, int64_t ldg32, const float* scale,
                             const float* shift, const float* mean, const float* invstd, const float* gamma, const float* beta,
                             float eps, int relu, float drop_p, uint64_t seed, const uint64_t* seed_counter, int64_t N, int C,
                             float* o1, float* o2, float* o3, float* o4, float* o5, float* running_mean, float* running_var,
                             float momentum, int64_t* num_batches_tracked, void* workspace, size_t workspace_bytes,
                             mlqem_stream_t stream);
int mlqem_layer_pointwise_f32(int op, const void* y, const void* g, const float* g32, int64_t ldg32, const void* res,
                              const float* scale, const float* shift, const float* mean, const float* invstd, const float* gs,
                              const float* k1, const float* k2, int relu, float drop_p, uint64_t seed,
                              const uint64_t* seed_counter, void* out, int64_t N, int C, mlqem_stream_t stream);
int mlqem_layer_wgrad_f32(const float* dy, const float* x, int64_t ldx, float* gw, float* gb, int64_t N, int K, int U,
                          void* workspace, size_t workspace_bytes, mlqem_stream_t stream);
int mlqem_layer_rowdot_f32(const void* h, const float* w, const float* b, float* out, int64_t ldo, int64_t N, int C, int O,
                           mlqem_stream_t stream);
int mlqem_layer_rowdot_bwd_f32(const float* g, int64_t ldg, const void* h, const float* w, void* gh, float gate_scale, float* gw,
                               float* gb, int64_t N, int C, int O, void* workspace, size_t workspace_bytes, mlqem_stream_t stream);

/* Synced statistics for either storage of the pipeline (torch.nn.SyncBatchNorm semantics under data parallelism, ABI 44; the bn1 /
 * bn2 of a converted MLP2 / MLP3, docs/tutorials/mlp.py:45-66,87-108): colstats' two stages with ONE all-reduce(SUM) of the caller
 * in between, over a [world][2 C + 1] double buffer in which rank r filled row r (zeros elsewhere: exact in any order).
 *   colstats_record_bf16 / _f32  mode 0: [n_r | mean_r[C] | M2_r[C]] of this rank's y (the shifted column sums, finished in
 *               double).  mode 1: [n_r | sum gu[C] | sum gu xhat[C]] with colstats 1's gu and the GLOBAL mean / invstd; dbeta /
 *               dgamma ([128], zeros beyond C) get this rank's sums (the parameter gradients: the gradient all-reduce averages them).
 *               Arguments as colstats'; same workspace.
 *   colstats_merge  records -> colstats' outputs, storage-independent ([128] each, zeros beyond C).  mode 0: o1..o5 = mean, biased
 *               var, invstd, scale, shift over the union of the ranks' rows (Chan's pairwise merge in rank order) and the running
 *               update with the global N (running_* / num_batches_tracked optional).  mode 1: o3..o5 = gs = gamma invstd,
 *               k1 = sum_r dbeta_r / N, k2 = sum_r dgamma_r / N (o1 / o2 unused).
 * The element-wise entry points (pointwise 0 / 1) consume the outputs unchanged.  Deterministic, no atomics, no allocation, no host
 * synchronisation. */
int mlqem_layer_colstats_record_bf16(int mode, const void* y, const void* g, const float* g32, int64_t ldg32, const float* scale,
                                     const float* shift, const float* mean, const float* invstd, int relu, float drop_p, uint64_t seed,
                                     const uint64_t* seed_counter, int64_t N, int C, double* record, float* dbeta, float* dgamma,
                                     void* workspace, size_t workspace_bytes, mlqem_stream_t stream);
int mlqem_layer_colstats_record_f32(int mode, const void* y, const void* g, const float* g32, int64_t ldg32, const float* scale,
                                    const float* shift, const float* mean, const float* invstd, int relu, float drop_p, uint64_t seed,
                                    const uint64_t* seed_counter, int64_t N, int C, double* record, float* dbeta, float* dgamma,
                                    void* workspace, size_t workspace_bytes, mlqem_stream_t stream);
int mlqem_layer_colstats_merge(int mode, const double* records, int world, int C, const float* gamma, const float* beta,
                               const float* invstd, float eps, float* o1, float* o2, float* o3, float* o4, float* o5,
                               float* running_mean, float* running_var, float momentum, int64_t* num_batches_tracked,
                               mlqem_stream_t stream);

/* Backward of a narrow hidden layer (I, O <= 12) in ONE pass over its operands:
 *   gx[n,:] = (x[n,:] > 0 ? gate_scale : 0) * (gy[n,:] @ W)   (gate != 0; plain gy @ W otherwise)      W: [O, I]
 *   gw2[0:O, :] = gy^T x,   gb2[12:12+O] = sum_n gb_src[n,:]   (gw2: [25, I], gb2: [25] -- rows 0..23 in the layout of
 *   mlqem_linear_wgrad_parts_f32 over the two 12-wide blocks [gy | gb_src]; gb_src = NULL means gy)
 *   gw2[24, 0:I] = sum_n gx[n,:]   (the bias gradient of the layer BELOW when an aggregation sits between the two layers, as
 *   with GCNConv: conv1's bias gradient is the column sum of what conv2's backward writes, so the first-layer weight-gradient
 *   pass reads one block less; gb2[24] is written as 0)
 * Replaces the autograd of torch_geometric's GCNConv linear (01_ngem.ipynb cell [9], conv2: gy = the transposed
 * aggregation of the incoming gradient, gb_src = that gradient itself, x = the previous activation whose ReLU/dropout
 * mask is handed over) with one read of gy, x and gb_src instead of two.  Padded 16-byte rows required.
 * workspace: mlqem_linear_wgrad_workspace_bytes(I, 25). */
int mlqem_linear_bwd_fused_f32(const float* gy, int64_t ldgy, const float* gb_src, int64_t ldgbs, const float* x, int64_t ldx,
                               const float* w, int gate, float gate_scale, float* gx, int64_t ldgx, float* gw2, float* gb2,
                               int64_t N, int I, int O, void* workspace, size_t workspace_bytes, mlqem_stream_t stream);

/* mlqem_linear_bwd_fused_f32 that ALSO takes the weight gradient of the layer below against a table (additive symbols, the ABI
 * version is unchanged): with row n of that layer's input being row table_rows[n] of table ([M, T], padded rows, 17 <= T <= 24;
 * table_rows == NULL: row n),
 *   gwt[0:I, 0:T] = gx^T table[table_rows]       (gwt: [I, T] row-major)
 * from the gx tile the pass holds, so gx need not exist in memory: gx == NULL skips its store (GCN conv1 as a projection of the
 * A^ x rows: conv2's backward leaves conv1's weight gradient, and the gated gradient between the two is never written or read).
 * gx (where requested), gw2 and gb2 carry the values of mlqem_linear_bwd_fused_f32, bit for bit.
 * workspace: mlqem_linear_bwd_fused_table_workspace_bytes(I, T). */
size_t mlqem_linear_bwd_fused_table_workspace_bytes(int I, int T);
int mlqem_linear_bwd_fused_table_f32(const float* gy, int64_t ldgy, const float* gb_src, int64_t ldgbs, const float* x, int64_t ldx,
                                     const float* w, int gate, float gate_scale, float* gx, int64_t ldgx, float* gw2, float* gb2,
                                     const float* table, int64_t ldt, const int32_t* table_rows, int T, float* gwt,
                                     int64_t N, int I, int O, void* workspace, size_t workspace_bytes, mlqem_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Pooling over graphs.  Replaces global_mean_pool (docs/tutorials/gnn.py:114; 01_ngem.ipynb cell [9]).
 * ---------------------------------------------------------------------------------------------------- */
/* out_mean[g,:] = (1/n_g) sum_{r in graph g} x[r,:] and/or out_wmean[g,:] = (1/n_g) sum_r weights[r] * x[r,:] over the
 * contiguous row range [graph_ptr[g], graph_ptr[g+1]) of every graph (either output may be NULL, not both; weights may be
 * NULL = 1; an empty graph gives 0).  The weighted form is the last conv layer of a Family A branch folded into its
 * pool: mean_pool(P (h W^T)) = wmean(h) W^T with weights = P^T 1, the column sums of the layer's propagation matrix
 * (01_ngem.ipynb cell [9] puts no non-linearity between conv3 / cheb_conv2 / sage_conv2 and global_mean_pool).
 * Rows are tiled over workgroups (1024 rows each, whatever graph they belong to), per-(tile, graph) partial sums are
 * added in tile order by a second kernel: balanced for graphs of 7 ... 20 000 nodes, deterministic, no atomics.
 * workspace: mlqem_segment_pool_workspace_bytes(N, B, C) bytes. */
size_t mlqem_segment_pool_workspace_bytes(int64_t N, int64_t B, int C);
int mlqem_segment_pool_f32(const float* x, int64_t ldx, const float* weights, const int32_t* graph_ptr, int64_t N, int64_t B,
                           int C, float* out_mean, int64_t ld_mean, float* out_wmean, int64_t ld_wmean, void* workspace,
                           size_t workspace_bytes, mlqem_stream_t stream);
/* Backward: gx[r,:] = (g_mean[g,:] + weights[r] * g_wmean[g,:]) / n_g for every row r of graph g (either gradient may be
 * NULL); gate (may be NULL), applied last: gx = gate[r,:] > 0 ? gx * gate_scale : 0 -- the ReLU/dropout mask of the
 * pooled activation, see mlqem_linear_f32.  16-byte accesses when gx, gate AND the [B,C] gradients own round_up(C,4)
 * columns per row.  gate_bits (instead of gate; needs the 16-byte form and C <= 64): the same mask as the sign bits
 * mlqem_csr_aggregate_pool_f32 leaves for the same N and C (tile records + per-wave ballots, see there) -- the gate then costs
 * half a byte per slice instead of sixteen, read at wave-uniform addresses, and the activation need not exist in memory at all. */
int mlqem_segment_pool_bwd_f32(const float* g_mean, int64_t ld_gmean, const float* g_wmean, int64_t ld_gwmean,
                               const float* weights, const int32_t* graph_ptr, int64_t N, int64_t B, int C,
                               const float* gate, int64_t ldgate, float gate_scale, const uint8_t* gate_bits, float* gx,
                               int64_t ldgx, mlqem_stream_t stream);

/* mlqem_segment_pool_bwd_f32(gate_bits=) followed by mlqem_csr_aggregate_f32 of its result over the transposed structure, in ONE
 * launch that never gathers the [N, C] gradient: the first backward aggregation of a Family A branch (01_ngem.ipynb cell [9]; the
 * reference's autograd through global_mean_pool and the branch's last conv).  A source's row is computed from what defines it -- the
 * 16 gate bits the pooled forward left for the node, its pool weight t_j = weights[j], the aggregation's column scale cscale[j], and the two
 * gradient rows of the row's own graph (edges stay inside a graph):
 *     g[j, :]   = gate(j, :) ? ((g_mean[b, :] + t_j g_wmean[b, :]) / n_b) * gate_scale : 0
 *     out[i, :] = alpha * (rscale[i] * sum_e cscale[idx[e]] * g[idx[e], :] + dself[i] * g[i, :])
 * Both are written (g, optional, for the dense consumers: weight and bias gradients); results equal the two-launch form bit for bit.
 * mlqem_pooled_grad_colsum_f32: sum_j g[j, :] without g -- partial[mlqem_pooled_grad_colsum_groups(N)][round_up(C, 4)], added over the
 * groups by the caller (the bias gradient of a layer whose aggregation did not write g).
 * gate_bits: the buffer mlqem_csr_aggregate_pool_f32 filled for the same N and C.  Needs C <= 16 (mlqem_pooled_grad_aggregate_supported),
 * the ELL side table of (ptr, idx), and 16-byte rows everywhere (ld % 4 == 0, ld >= round_up(C, 4)). */
int mlqem_pooled_grad_aggregate_supported(int C);
int mlqem_pooled_grad_colsum_groups(int64_t N);
int mlqem_pooled_grad_colsum_f32(const uint8_t* gate_bits, const float* weights, const float* g_mean, int64_t ld_gmean, const float* g_wmean,
                                 int64_t ld_gwmean, const int32_t* graph_ptr, int64_t B, float gate_scale, int64_t N, int C, float* partial,
                                 mlqem_stream_t stream);
int mlqem_pooled_grad_aggregate_f32(const uint8_t* gate_bits, const float* weights, const float* cscale, const float* g_mean, int64_t ld_gmean,
                                    const float* g_wmean, int64_t ld_gwmean, const int32_t* graph_ptr, int64_t B, float gate_scale,
                                    const int32_t* ptr, const int32_t* idx, const int32_t* ell, const float* rscale,
                                    const float* dself, float alpha, float* out, int64_t ldo, float* g, int64_t ldg, int64_t N, int C,
                                    mlqem_stream_t stream);

/* What remains of a branch's last conv once it is folded into its pool: out[b, col[t]] (+)= P_t[b, :] . W_t (+ bias[col]),
 * t < n_terms (Family A: GCN one term, Cheb and SAGE two each -> three columns), and its backward:
 * gP_t[b, :] = gout[b, col[t]] * W_t;  gW[t, :] = sum_b gout[b, col[t]] * P_t[b, :];  gb[k] = sum_b gout[b, k].
 * P_t: [B, C] device matrices (row stride ldp[t]); W_t: [C]; bias[k]: one float on the device or NULL.
 * gP, ldgp: HOST arrays of n_terms device pointers / row strides. */
#define MLQEM_HEAD_MAX_TERMS 8
typedef struct mlqem_head_desc {
  int32_t n_terms, n_cols;
  const void* P[MLQEM_HEAD_MAX_TERMS];
  int64_t ldp[MLQEM_HEAD_MAX_TERMS];
  const void* W[MLQEM_HEAD_MAX_TERMS];
  int32_t col[MLQEM_HEAD_MAX_TERMS];
  const void* bias[MLQEM_HEAD_MAX_TERMS];
} mlqem_head_desc;
int mlqem_pooled_head_f32(const mlqem_head_desc* desc, int64_t B, int C, float* out, int64_t ldo, mlqem_stream_t stream);
int mlqem_pooled_head_bwd_f32(const mlqem_head_desc* desc, const float* gout, int64_t ldg, int64_t B, int C, float* const* gP,
                              const int64_t* ldgp, float* gW, float* gb, mlqem_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Batch assembly from a device-resident dataset.  Replaces torch_geometric.loader.DataLoader's collate
 * (Batch.from_data_list; call sites docs/tutorials/gnn.py:293-307, docs/tutorials/__ml_models.py:105-119), which
 * concatenates ~9 attributes of B Data objects on the host every step.
 *
 * Arena (whole dataset, G graphs): x[Ntot,F], nscal[Ntot,K] (per-node scalars, e.g. the three norms), a_gptr[G+1],
 * and the CSR arrays of mlqem_csr_build run over the whole arena (global node ids).
 * Selection: sel[B] graph ids (repeats allowed); b_nptr[B+1] / b_eptr[B+1] = prefix sums of the selected graphs'
 * node / edge counts (host knows them without a sync); Nb = b_nptr[B], Eb = b_eptr[B].
 * Outputs: the batch's x (xb may be NULL: no copy of the feature rows is made and the caller's first layers read them
 * from the arena through src_node, the x_rows argument of the dense entry points), nscal_b -- PLANAR [K, Nb], scalar k of all nodes contiguous, so each is usable as a vector
 * without a strided copy --, src_node[Nb] (arena row of every batch node), both CSR structures (node ids rebased to
 * the batch), loops and, when the arena's ELL side tables a_in_ell / a_out_ell (mlqem_ell_from_csr over the arena)
 * are given, the batch's side tables in_ell_b / out_ell_b [Nb,2] rebased the same way (NULL = not wanted).
 * derived_b (may be NULL; needs K >= 3 with nscal = [gcn_dinv, sage_rinv, cheb_dinv, ...] and a_loops): planar [3, Nb] =
 * gcn_dinv^2 (the (i,i) weight of the GCN operator), loops * sage_rinv (the self share of SAGE's mean), -cheb_dinv -- the
 * per-node scalars the layers derive, written in the same pass instead of by three element-wise kernels per batch.
 * Fixed-shape launches (hipGraph replay over size buckets): Nb must equal b_nptr[B], but Eb may be a CAPACITY >= b_eptr[B];
 * the kernels take the real edge total from b_eptr[B] on the device, so one captured launch serves every selection whose
 * totals fit the bucket (the caller pads the node count with a slice of an edgeless filler graph of the arena).
 * ---------------------------------------------------------------------------------------------------- */
int mlqem_batch_assemble(const float* x, int64_t ldx, int F, const float* nscal, int K, const int32_t* a_gptr,
                         const int32_t* a_in_ptr, const int32_t* a_in_src, const int32_t* a_out_ptr,
                         const int32_t* a_out_dst, const int32_t* a_out_eid, const int32_t* a_loops,
                         const int32_t* a_in_ell, const int32_t* a_out_ell, const int32_t* sel, const int32_t* b_nptr,
                         const int32_t* b_eptr, int64_t B, int64_t Nb, int64_t Eb, float* xb, int64_t ldxb,
                         float* nscal_b, float* derived_b, int32_t* src_node, int32_t* in_ptr_b, int32_t* in_src_b, int32_t* out_ptr_b,
                         int32_t* out_dst_b, int32_t* out_eid_b, int32_t* loops_b, int32_t* in_ell_b, int32_t* out_ell_b,
                         mlqem_stream_t stream);

/* The per-graph inputs of a batch in ONE launch (ABI 40): dst[k][b, :] = src[k][sel[b], :] for up to four fp32 row-major matrices
 * src[k] [G, width[k]] (the dataset's labels y, noisy values, circuit depths and observables; reference collate:
 * torch_geometric DataLoader at docs/tutorials/__ml_models.py:105-119 concatenates them per batch on the host) -- five torch gather
 * launches per step before, which a captured step of 32 four-qubit circuits (~80 launches of ~5 us) feels. */
int mlqem_gather_rows_f32(int count, const float* const* src, const int64_t* width, const int32_t* sel, int64_t B, float* const* dst,
                          mlqem_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Family B (docs/tutorials/gnn.py:70-276): TransformerConv attention and ASAPooling.  Forward kernels.
 * ---------------------------------------------------------------------------------------------------- */

/* TransformerConv(heads=H, concat=True, beta=False, edge_dim=None, root_weight=True) message + aggregate + skip
 * (gnn.py:80-91,104,109).  qkvs[N, 4*H*C] = [query | key | value | skip] from ONE fused projection.
 * out[i, h*C:(h+1)*C] = sum_e softmax_e( q_i.k_src / sqrt(C) ) v_src + skip_i ; softmax over the CSR in-edges of i
 * followed by loops[i] copies of the self-loop (loops may be NULL); denominator + 1e-16 as in PyG.  C <= 32. */
int mlqem_transformer_attention_f32(const float* qkvs, int64_t ld, const int32_t* in_ptr, const int32_t* in_src,
                                    const int32_t* loops, int64_t N, int H, int C, float* out, int64_t ldo,
                                    mlqem_stream_t stream);

/* ASAPooling steps 3-4 (gnn.py:85,92): out[i,:] = sum_e softmax_e(LeakyReLU(a_dst[i] + c_src[src_e])) x[src_e,:]
 * over the CSR in-edges of i plus its own self-loop (add_remaining_self_loops). */
int mlqem_csr_softmax_aggregate_f32(const float* x, int64_t ldx, const int32_t* in_ptr, const int32_t* in_src,
                                    const float* a_dst, const float* c_src, float negative_slope, int64_t N, int C,
                                    float* out, int64_t ldo, mlqem_stream_t stream);

/* ASAPooling step 5, LEConv(D->1) + sigmoid on per-node scalars pqr[N,3] = (lin1 x', lin2 x', lin3 x'):
 * fitness[i] = sigmoid( sum_{e in in(i) + self} (p[src_e] - q[i]) + r[i] ).
 * long_rows (ABI 41) != 0: the graph's rows are long (a coarsened graph): a 16-lane group per row instead of a thread (the sum of a
 * row's p values is then a tree sum, not the entries in order). */
int mlqem_leconv_fitness_f32(const float* pqr, const int32_t* in_ptr, const int32_t* in_src, int64_t N,
                             float* fitness, int long_rows, mlqem_stream_t stream);

/* out[p,:] = x[perm[p],:] * scale[perm[p]]  (x_out = x'[perm] * fitness[perm]; scale may be NULL). */
int mlqem_gather_scale_rows_f32(const float* x, int64_t ldx, const int32_t* perm, const float* scale, int64_t K, int C,
                                float* out, int64_t ldo, mlqem_stream_t stream);

/* Boundaries of the pooled batch on the device (ABI 37): new_graph_ptr[0] = 0, new_graph_ptr[g + 1] = new_graph_ptr[g] +
 * ceil((float)(graph_ptr[g + 1] - graph_ptr[g]) * ratio) -- the k of PyG's topk(x, ratio, batch) (torch_geometric
 * nn/pool/topk_pool.py, called from ASAPooling, reference docs/tutorials/gnn.py:85,92), evaluated in float32 as there.  Replaces
 * the host-side cumsum over per-graph sizes for batches whose sizes the host does not look at (size-stable captured steps).
 * graph_ptr [B + 1], new_graph_ptr [B + 1] int32; 0 < ratio <= 1.  One small launch, no workspace, asynchronous on `stream`. */
int mlqem_pool_keep_ptr(const int32_t* graph_ptr, int64_t B, float ratio, int32_t* new_graph_ptr, mlqem_stream_t stream);

/* ASAPooling step 6 (PyG topk(fitness, ratio, batch)): for graph g keep its new_graph_ptr[g+1]-new_graph_ptr[g]
 * nodes of largest fitness, listed by descending fitness (ties: lower index first), graphs in order.
 * max_graph_nodes: an upper bound on a graph's node count when the caller has one (0: none, N is used) -- it sizes the
 * index field of the sort key, and lets batches of large graphs (>= 1024 nodes on average) go through ONE device-wide radix
 * sort with the graph index in the key's top bits instead of a segmented sort that gives each graph to one workgroup.
 * slot (ABI 41; may be NULL): [N], slot[perm[p]] = p for the K kept centres, -1 elsewhere, written by the same launches (every
 * node is one of the sorted keys).  ASAPooling's backward needs it (x_out = x'[perm] * fitness[perm], gnn.py:105-107,110-112)
 * and the coarsening entry points below read it. */
size_t mlqem_segment_topk_workspace_bytes(int64_t N, int64_t B);
int mlqem_segment_topk(const float* fitness, const int32_t* graph_ptr, const int32_t* new_graph_ptr, int64_t N,
                       int64_t B, int64_t K, int64_t max_graph_nodes, int32_t* perm, int32_t* slot, void* workspace,
                       size_t workspace_bytes, mlqem_stream_t stream);

/* ASAPooling step 7 (torch-sparse S^T A S, remove_diag, coo): only the PATTERN is consumed by the models.
 * Two hops with a sort-unique in between (counting every 3-step path explodes around 100-wire barriers):
 *   hop1_count: slot[N] (cluster id of each kept node, -1 elsewhere), offsets[K+1] = exclusive scan of the (cluster p,
 *               node v) candidates, v reachable in one step from a member of p; offsets[K] = total, read back by the caller
 *   hop1_fill:  keys = p << 32 | v                 -> mlqem_sort_unique_u64 -> M distinct pairs
 *   hop2_count / hop2_fill over those pairs: keys = p << 32 | q for every kept w in N+[v], q = slot[w] != p
 *               -> mlqem_sort_unique_u64 -> the pooled edges in row-major (p, q) order, as SparseTensor.coo() lists them
 *   mlqem_keys_to_edge_index: [2,E] int64 (src = p, dst = q); feed it to mlqem_csr_build. */
size_t mlqem_asap_coarsen_workspace_bytes(int64_t K);   /* for a count call over K items (hop1: clusters, hop2: pairs) */
int mlqem_asap_hop1_count(const int32_t* in_ptr, const int32_t* in_src, const int32_t* out_ptr, const int32_t* out_dst,
                          const int32_t* perm, int64_t N, int64_t K, int32_t* slot, int64_t* offsets, void* workspace,
                          size_t workspace_bytes, mlqem_stream_t stream);
int mlqem_asap_hop1_fill(const int32_t* in_ptr, const int32_t* in_src, const int32_t* out_ptr, const int32_t* out_dst,
                         const int32_t* perm, const int64_t* offsets, int64_t K, uint64_t* keys, mlqem_stream_t stream);
int mlqem_asap_hop2_count(const uint64_t* pairs, int64_t M, const int32_t* out_ptr, const int32_t* out_dst,
                          const int32_t* slot, int64_t* offsets, void* workspace, size_t workspace_bytes,
                          mlqem_stream_t stream);
int mlqem_asap_hop2_fill(const uint64_t* pairs, int64_t M, const int32_t* out_ptr, const int32_t* out_dst,
                         const int32_t* slot, const int64_t* offsets, uint64_t* keys, mlqem_stream_t stream);
size_t mlqem_sort_unique_u64_workspace_bytes(int64_t T);
int mlqem_sort_unique_u64(const uint64_t* keys, int64_t T, uint64_t* out_keys, int64_t* out_count, void* workspace,
                          size_t workspace_bytes, mlqem_stream_t stream);
int mlqem_keys_to_edge_index(const uint64_t* keys, int64_t E, int64_t* edge_index, mlqem_stream_t stream);

/* Coarsened connectivity of LARGE graphs (100-qubit circuits pool to thousands of clusters; their second pooling runs on
 * graphs with hub clusters of hundreds of neighbours, where the two-hop path above sorts ~50 candidate keys per distinct
 * edge), from SORTED LISTS (round 4; the default for large graphs): nothing dense is written
 * to or read from global memory, and the three hops of a cluster's reach are split into per-NODE lists built once --
 * C(v): the kept centres among N+[v]; R(u) / R'(u): the C lists of N+[u] / N-[u] one after the other -- so that a hub's list
 * (a barrier: ~300 entries) is formed once and read, coalesced, by every cluster that contains the hub.  Persistent waves OR a
 * cluster's few lists into two LDS bitsets (row and transposed row), read them out in ascending order and clear them on the
 * way; a structural bound per row (sums of two-hop degree sums, clamped to k_g - 1) places every row in a scratch; degrees ->
 * scans -> the CSR pointers; the fill pass copies the lists to their place and finds every out-entry's twin in the in-row by
 * binary search, one thread per entry.
 *   lists_caps:  totals[4] (device int64) = the totals of the row bounds (out, in) and of the per-node list sizes (out, in):
 *                `capacity` must cover all four when the caller has no structural bound of its own (one 32-byte read);
 *                workspace of mlqem_asap_coarsen_lists_workspace_bytes(N, K, 0, 0);
 *   lists_count: new_in_ptr[K + 1], new_out_ptr[K + 1]; E = stored edges of the input structure (or a bound); slot[N] must
 *                hold slot[perm[p]] = p, -1 elsewhere (mlqem_segment_topk writes it);
 *   lists_fill:  new_in_src / new_out_dst / new_out_eid, each holding edge_capacity entries (new_out_ptr[K] <= edge_capacity
 *                <= capacity), from the SAME workspace; new_out_eid may be NULL (no link pass: the recomputed backward forms
 *                need no out_eid); *overflow (device, may be NULL) = 1 if `capacity` was too small.
 * capacity < 2^32 (places inside the per-node records are 32 bits), else MLQEM_ERR_UNSUPPORTED.
 * kmax <= mlqem_asap_coarsen_lists_max_k() (65 535 clusters per pooled graph), else MLQEM_ERR_UNSUPPORTED.
 * new_loops (may be NULL): [K], zeroed (the coarsened graph lists no self-loops).
 * Replaces the same ASAPooling.forward lines (gnn.py:105-107,110-112; PyG semantics: SURVEY appendix B.2 step 7). */
size_t mlqem_asap_coarsen_lists_workspace_bytes(int64_t N, int64_t K, int64_t E, int64_t capacity);
int mlqem_asap_coarsen_lists_max_k(void);
int mlqem_asap_coarsen_lists_caps(const int32_t* in_ptr, const int32_t* in_src, const int32_t* out_ptr, const int32_t* out_dst,
                                  const int32_t* new_graph_ptr, const int32_t* perm, int64_t N, int64_t K, int64_t B,
                                  int64_t* totals, void* workspace, size_t workspace_bytes, mlqem_stream_t stream);
int mlqem_asap_coarsen_lists_count(const int32_t* in_ptr, const int32_t* in_src, const int32_t* out_ptr, const int32_t* out_dst,
                                   const int32_t* graph_ptr, const int32_t* new_graph_ptr, const int32_t* perm, int64_t N,
                                   int64_t K, int64_t B, int64_t E, int kmax, int64_t capacity, const int32_t* slot,
                                   int32_t* new_in_ptr, int32_t* new_out_ptr, int32_t* new_loops, void* workspace, size_t workspace_bytes,
                                   mlqem_stream_t stream);
int mlqem_asap_coarsen_lists_fill(int64_t N, int64_t K, int64_t E, int64_t capacity, const int32_t* new_in_ptr,
                                  const int32_t* new_out_ptr, int32_t* new_in_src, int32_t* new_out_dst, int32_t* new_out_eid,
                                  int64_t edge_capacity, int32_t* overflow, void* workspace, size_t workspace_bytes,
                                  mlqem_stream_t stream);

/* Coarsened connectivity WITHOUT host read-backs, for batches whose graphs all pool to at most
 * mlqem_asap_coarsen_dense_max_k() clusters (512): the pooled adjacency of every graph is built as a k_g x k_g bit
 * matrix in LDS by one workgroup per graph (idempotent atomicOr: order-independent), device scans of the row / column
 * popcounts give new_in_ptr / new_out_ptr directly, and a second kernel lists rows and columns in ascending order --
 * the same arrays mlqem_csr_build yields from the two-hop path's sorted edge list.  graph_ptr / new_graph_ptr: node
 * ranges of the graphs before / after pooling; perm: the kept centres, graph by graph (mlqem_segment_topk); kmax >= the
 * largest k_g (host knows it: k_g = ceil(ratio * n_g); a bound will do).  new_in_src / new_out_dst / new_out_eid must hold
 * sum_g k_g (k_g - 1) entries; only the first new_in_ptr[K] are written.  new_loops[K] = 0 (no diagonal).
 * slot: [N], slot[perm[p]] = p, -1 elsewhere (mlqem_segment_topk writes it).  Three launches: bit matrices, one scan of both
 * degree vectors, the fill. */
int mlqem_asap_coarsen_dense_max_k(void);
size_t mlqem_asap_coarsen_dense_workspace_bytes(int64_t B, int64_t K, int kmax);
int mlqem_asap_coarsen_dense(const int32_t* in_ptr, const int32_t* in_src, const int32_t* out_ptr, const int32_t* out_dst,
                             const int32_t* graph_ptr, const int32_t* new_graph_ptr, const int32_t* perm, int64_t N, int64_t K,
                             int64_t B, int kmax, const int32_t* slot, int32_t* new_in_ptr, int32_t* new_in_src,
                             int32_t* new_out_ptr, int32_t* new_out_dst, int32_t* new_out_eid, int32_t* new_loops,
                             void* workspace, size_t workspace_bytes, mlqem_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Family B backward.  Edge-softmax gradients are split into a destination-side pass and a source-side pass.  No atomics; every
 * gradient row is written once.  Two forms of the hand-over between the passes:
 *   stored      (out_eid given): the destination side writes per-edge buffers in in-CSR order (E entries, then one self-loop
 *               entry per node at E + row) and the source side reads them through out_eid;
 *   recomputed  (out_eid == NULL, round 4): nothing is kept per edge; the source side recomputes every weight from the
 *               per-row statistics of the forward (and one more per-row number the destination side files), the way
 *               attention backward passes are usually written.  It needs no map from out-entries to in-CSR positions --
 *               ASAPooling's coarsened graphs come without one (linking their 9.7 M entries cost 0.55 ms of an 8.7 ms step) --
 *               and reads [N]-sized arrays where the stored form reads [E]-sized ones.
 * ---------------------------------------------------------------------------------------------------- */

/* Training forward of mlqem_transformer_attention_f32: same result, plus attn_out (the sum before the skip term; since ABI 25
 * written only for rows of MORE THAN FOUR entries, in-edges + self entry: the backward forms what it needs of a shorter row --
 * g . attn_out -- from the row's own entries, so on circuit DAGs attn_out is neither written nor read but for barrier rows;
 * the buffer is opaque to callers, hand it to the backward as it is) and the softmax statistics stat_m / stat_den [N,H]; drop_p > 0 drops attention weights (TransformerConv(dropout=0.1),
 * gnn.py:83,90) with a mask keyed by (seed, in-CSR position, head) -- or, pair_key != 0, by (seed, destination, head, source):
 * the same draw from either end of an edge, for graphs WITHOUT parallel edges (they would share a draw); the recomputed
 * backward needs it.  seed_counter (may be NULL): a device-resident step counter mixed into the seed, so that a launch captured
 * in a hipGraph draws a fresh mask per replay (the backward entry point must be given the same seed, counter and key form).
 * in_ell (optional, ABI 25): the [N,2] side table of mlqem_ell_from_csr over the same in-CSR -- rows of at most two in-edges then
 * reach their key / value rows without the ptr -> idx round trip (same result bit for bit).
 * head_pitch (ABI 25; 0 = C): the channel pitch of a head inside the four parts of qkvs -- and of gqkvs in the backward --
 * i.e. qkvs is [N, 4 H head_pitch] with part p of head h at column (p H + h) head_pitch and zeros in the head_pitch - C pad
 * channels (a projection whose weight and bias rows are padded the same way produces exactly that).  16 for the reference's
 * 15 channels makes every gathered key / value / query segment an aligned 64-byte piece (forward -8 %, backward -7..-17 % on
 * the 100-qubit graphs for 7 % more bytes); out, attn_out and g stay compact [N, H C]; the backward writes zeros into gqkvs' pads. */
int mlqem_transformer_attention_train_f32(const float* qkvs, int64_t ld, const int32_t* in_ptr, const int32_t* in_src,
                                          const int32_t* loops, int64_t N, int64_t E, int H, int C, float drop_p,
                                          uint64_t seed, const uint64_t* seed_counter, int pair_key, const int32_t* in_ell,
                                          int head_pitch, float* out, int64_t ldo, float* attn_out, int64_t lda, float* stat_m,
                                          float* stat_den, mlqem_stream_t stream);

/* gqkvs[N, 4HC] = gradient of [query | key | value | skip] given g = dL/d out.  Stored form: edge_al / edge_gs: scratch
 * [(E+N)*H].  Recomputed form (out_eid == NULL): edge_al: scratch [4*N*H] (16-byte aligned), edge_gs unused (may be NULL); with drop_p > 0 it needs
 * pair_key != 0 (MLQEM_ERR_BAD_ARG otherwise). */
int mlqem_transformer_attention_bwd_f32(const float* qkvs, int64_t ld, const float* g, int64_t ldg,
                                        const float* attn_out, int64_t lda, const float* stat_m, const float* stat_den,
                                        const int32_t* in_ptr, const int32_t* in_src, const int32_t* out_ptr,
                                        const int32_t* out_dst, const int32_t* out_eid, const int32_t* loops, int64_t N,
                                        int64_t E, int H, int C, float drop_p, uint64_t seed, const uint64_t* seed_counter,
                                        int pair_key, int head_pitch, float* gqkvs, int64_t ldq, float* edge_al, float* edge_gs,
                                        mlqem_stream_t stream);

/* Backward of mlqem_csr_softmax_aggregate_f32: gx (+)= d/dx, g_a[N] = d/d a_dst, g_c[N] = d/d c_src.
 * xnew = the forward output, gnew its gradient.  Stored form: edge_al / edge_gp: scratch [E+N].  Recomputed form
 * (out_eid == NULL; C <= 128): edge_al: scratch [4 N], 16-byte aligned; edge_gp unused (may be NULL).
 * tie_count (may be NULL; C <= 128): with xmax = the segment max of x over the same entries (mlqem_csr_segment_max_f32, what
 * ASAPooling computes from the same x: gnn.py:105-107), tie_count[i, c] = the number of entries of row i (sources and i itself) whose
 * value equals xmax[i, c] -- the destination-side walk holds every source row anyway, and mlqem_csr_segment_max_bwd_f32 then
 * needs no walk of its own to split a maximum's gradient among ties.
 * gx_rank1 (may be NULL; C <= 128): a [C] vector r; gx additionally receives g_c[j] * r -- the gradient through the source score
 * c_j = x_j . r (ASAPooling's att on the source half, gnn.py:105-107), which otherwise is a read-modify-write pass over gx.
 * fuse_max_col (may be NULL; stored form with tie_count only; ABI 34): a [C] vector w; the source-side walk then also adds the
 * backward of the segment max whose gradient is g_a (x) w -- gx[j, c] += sum over the destinations i of j, and j itself, with
 * x[j, c] == xmax[i, c] of g_a[i] w[c] / max(tie_count[i, c], 1) -- and mlqem_csr_segment_max_bwd_f32 is not called at all. */
int mlqem_csr_softmax_aggregate_bwd_f32(const float* x, int64_t ldx, const float* xnew, int64_t ldn, const float* gnew,
                                        int64_t ldg, const int32_t* in_ptr, const int32_t* in_src,
                                        const int32_t* out_ptr, const int32_t* out_dst, const int32_t* out_eid,
                                        const float* a_dst, const float* c_src, float negative_slope, int64_t N,
                                        int64_t E, int C, int accumulate, float* gx, int64_t ldgx, float* g_a,
                                        float* g_c, float* edge_al, float* edge_gp, const float* xmax, int64_t ldm,
                                        float* tie_count, int64_t ldt, const float* gx_rank1, const float* fuse_max_col,
                                        mlqem_stream_t stream);

/* Backward of mlqem_csr_segment_max_f32, ACCUMULATING into gx: the gradient of a row's maximum goes to the entries
 * (sources or the row itself) whose value equals it, split evenly among ties (torch scatter_reduce(amax) rule).
 * gmax_row [N] / gmax_col [C] (may be NULL): gmax = gmax_row (x) gmax_col, never formed (needs tie_count; gmax is then unused).
 * gshare: scratch [N, lds >= C].  tie_count (may be NULL): the counts mlqem_csr_softmax_aggregate_bwd_f32 left; the
 * destination-side pass over the in-edges is then an elementwise division. */
int mlqem_csr_segment_max_bwd_f32(const float* x, int64_t ldx, const float* xmax, int64_t ldm, const float* gmax,
                                  int64_t ldg, const int32_t* in_ptr, const int32_t* in_src, const int32_t* out_ptr,
                                  const int32_t* out_dst, int64_t N, int C, float* gx, int64_t ldgx, float* gshare,
                                  int64_t lds, const float* tie_count, int64_t ldt, const float* gmax_row, const float* gmax_col,
                                  mlqem_stream_t stream);

/* Backward of x_out = x'[perm] * fitness[perm] over all N rows (slot[i] = cluster id or -1 from
 * mlqem_asap_hop1_count): gxnew[i,:] = gout[slot[i],:] * fitness[i] (0 for dropped rows), gfit[i] = gout[slot[i]].x'[i]. */
int mlqem_gather_scale_rows_bwd_f32(const float* gout, int64_t ldgo, const float* xnew, int64_t ldn,
                                    const float* fitness, const int32_t* slot, int64_t N, int C, float* gxnew,
                                    int64_t ldgn, float* gfit, mlqem_stream_t stream);

/* ABI 41: mlqem_gather_scale_rows_bwd_f32 as two launches around the fitness backward (ASAPooling.backward, gnn.py:85,92): the first
 * stores gfit[row] = g_out[slot[row]] . x'[row] (0 for rows that were not kept) only; the second forms
 * gxnew[row] = (kept ? g_out[slot[row]] fitness[row] : 0) + sum_{t < K} g3[row, t] w3[t, :]  (K <= 3; w3 compact [K, C]) in ONE store --
 * the gradient through x_out = x'[perm] f[perm] plus the gradient g_pqr W3 through pqr = x' W3^T + b3, which was a read-modify-write
 * GEMM over gxnew.  Rows of at most 64 channels in the padded layout (16-byte rows); MLQEM_ERR_UNSUPPORTED otherwise. */
int mlqem_gather_rows_dot_f32(const float* gout, int64_t ldgo, const float* xnew, int64_t ldn, const int32_t* slot, int64_t N, int C,
                              float* gfit, mlqem_stream_t stream);
int mlqem_scatter_scale_rank_f32(const float* gout, int64_t ldgo, const float* fitness, const int32_t* slot, const float* g3, int64_t ldg3,
                                 const float* w3, int K, int64_t N, int C, float* gxnew, int64_t ldgn, mlqem_stream_t stream);

/* The three tiny weight gradients at the end of ASAPooling's backward in ONE pass (ABI 40): up to three weighted column sums over the
 * same N rows.  Term t: weight columns g[t] [N, ldg[t]] (k[t] <= 3 of them), matrix x[t] [N, ldx[t]] with D columns in 16-byte rows;
 * out [sum k, D] row-major in term order = g[t]^T x[t], bias [sum k] = the column sums of the weights.  Replaces the autograd of
 * ASAPooling's `lin` / `att` / `gnn_score` projections (torch_geometric ASAPooling.forward, called at docs/tutorials/gnn.py:105-112):
 * three [N, k] x [N, D] weight-gradient GEMMs.  Deterministic (fixed-order partial sums).  workspace:
 * mlqem_rank_grad_workspace_bytes(D); D <= 256. */
size_t mlqem_rank_grad_workspace_bytes(int D);
int mlqem_rank_grad_f32(int terms, const float* const* x, const int64_t* ldx, const float* const* g, const int64_t* ldg, const int* k,
                        int64_t N, int D, float* out, float* bias, void* workspace, size_t workspace_bytes, mlqem_stream_t stream);

/* Backward of mlqem_leconv_fitness_f32 onto pqr[N,3]. */
int mlqem_leconv_fitness_bwd_f32(const float* gfit, const float* fitness, const int32_t* in_ptr, const int32_t* out_ptr,
                                 const int32_t* out_dst, int64_t N, float* gpqr, mlqem_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Row order of a coarsened graph (csrc/row_order.hip).  The graph ASAPooling coarsens out of a large circuit
 * (docs/tutorials/gnn.py:85,92,104-112: TransformerConv 2 and ASAPooling 2 of every reference GNN run on it) is a union of dense
 * blocks: rows whose centres are close in program order share nearly all their sources.  The dense-block plans below take their
 * rows in that order.  (ABI <= 38 also exported LDS-staged "tile" kernels built on the same order -- mlqem_tile_plan_build,
 * mlqem_tile_attention_*, mlqem_tile_asap_scores_*: measured slower than the per-edge kernels, superseded by the dense blocks,
 * removed with ABI 39.)
 * ---------------------------------------------------------------------------------------------------- */
/* order[new_graph_ptr[g] + r] = the cluster of graph g whose centre is the r-th kept node of the graph in node order
 * (= program order of a circuit); slot[perm[p]] = p for the kept centres, -1 elsewhere.  One workgroup per graph. */
int mlqem_tile_order_by_position(const int32_t* slot, const int32_t* graph_ptr, const int32_t* new_graph_ptr, int64_t num_graphs,
                                 int32_t* order, mlqem_stream_t stream);

/* ASAPooling's forward up to the fitness projections in one pass, for graphs of short rows (C <= 64): per row the segment max over
 * its in-entries and itself (xmax), the composed score a_dst = w_comp . xmax + b_comp, c_src = att_x . x, the score softmax + cluster
 * sum (xnew) and pqr[N, 3] = xnew W3^T + b3.  Stands for mlqem_csr_segment_max_f32 + mlqem_linear_f32 x 3 +
 * mlqem_csr_softmax_aggregate_f32 of ASAPooling.forward (docs/tutorials/gnn.py:85,92); same outputs. */
int mlqem_asap_scores_fused_f32(const float* x, int64_t ldx, const int32_t* in_ptr, const int32_t* in_src, const float* w_comp,
                                const float* b_comp, const float* att_x, const float* w3, const float* b3, float negative_slope,
                                int64_t N, int C, float* xmax, int64_t ldm, float* a_dst, float* c_src, float* xnew, int64_t ldn,
                                float* pqr, mlqem_stream_t stream);

/* The q / k / v / skip projection of a TransformerConv (docs/tutorials/gnn.py:80-91) writes a head's C channels at a pitch of
 * `pitch` floats when its weight [groups * channels, cols] and bias [groups * channels] have every group of rows spread to that pitch
 * with zero rows between (groups = 4 heads); mlqem_unpad_head_rows_f32 takes the real rows of the padded gradients back.  b, b_padded,
 * gb_padded, gb may be NULL. */
int mlqem_pad_head_rows_f32(const float* w, const float* b, int groups, int channels, int pitch, int cols, float* w_padded,
                            float* b_padded, mlqem_stream_t stream);
/* The same from up to four separate [groups_per_part * channels, cols] matrices (and biases; b or b[k] may be NULL) laid one after the
 * other: the query / key / value / skip projections of a TransformerConv (reference construction docs/tutorials/gnn.py:80-91) as ONE
 * padded weight without a torch.cat in front (ABI 40); pitch == channels gives the plain concatenation. */
int mlqem_pad_head_rows_parts_f32(const float* const* w, const float* const* b, int parts, int groups_per_part, int channels, int pitch,
                                  int cols, float* w_padded, float* b_padded, mlqem_stream_t stream);
int mlqem_unpad_head_rows_f32(const float* gw_padded, const float* gb_padded, int groups, int channels, int pitch, int cols,
                              float* gw, float* gb, mlqem_stream_t stream);

/* The small-tensor algebra around ASAPooling's score and fitness projections (docs/tutorials/gnn.py:85,92: ASAPooling.lin, .att,
 * .gnn_score.lin1/2/3; D = the pooling's channels), one launch per direction instead of ten element-wise launches each:
 *   forward : w_comp[D] = att_q W_lin, b_comp[1] = att_q . b_lin + att_b (the query projection composed into the one-wide score
 *             projection that is its only consumer), att_q[D] / att_x[D] = the halves of att_w[2 D], w3[3 D] = (l1_w; l2_w; l3_w),
 *             b3[3] = (l1_b, 0, l3_b)
 *   backward: g_lin_w[D D], g_lin_b[D], g_att_w[2 D] from g_w_comp[D], g_att_b[1], g_att_x[D] by the chain rule. */
int mlqem_asap_compose_f32(const float* lin_w, const float* lin_b, const float* att_w, const float* att_b, const float* l1_w,
                           const float* l1_b, const float* l2_w, const float* l3_w, const float* l3_b, int D, float* w_comp,
                           float* b_comp, float* att_q, float* att_x, float* w3, float* b3, mlqem_stream_t stream);
int mlqem_asap_compose_bwd_f32(const float* g_w_comp, const float* g_att_b, const float* lin_w, const float* lin_b,
                               const float* att_w, const float* g_att_x, int D, float* g_lin_w, float* g_lin_b, float* g_att_w,
                               mlqem_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Dense blocks (csrc/dense_block.hpp): TransformerConv's edge softmax (docs/tutorials/gnn.py:80-91) over the LONG rows of a
 * structure on the f32 matrix cores.  A block = 16 rows of at least mlqem_dense_plan_min_degree() entries that follow each other
 * in `order` inside one graph x the union of their sources (at most 512 slots), with one bit per cell; the rows of a usable block
 * are flagged in row_flag and left alone by the per-edge kernels, which serve every other row in the same call.
 *
 * mlqem_dense_plan_build, once per structure and direction (in-CSR: forward and destination-side backward; out-CSR: source-side
 * backward):  counter[1] (zero on entry) receives 16 x the number of blocks; lrows[17 * max_blocks] the blocks' rows, then their graphs;
 * records[max_blocks * mlqem_dense_plan_record_ints()] (16-byte aligned) the blocks; row_flag[num_rows] (zero on entry) the flags.
 * max_blocks = mlqem_dense_plan_max_blocks(num_rows, num_graphs).  graph_ptr[num_graphs + 1]: the graphs' ranges of positions in
 * `order` AND of row ids (null order: the rows themselves); max_span: a bound on the rows of one graph (ids beyond 262 144 from a block's first are left to the per-edge kernels).
 * ---------------------------------------------------------------------------------------------------- */
int mlqem_dense_plan_record_ints(void);
int mlqem_dense_plan_min_degree(void);
int64_t mlqem_dense_plan_max_blocks(int64_t num_rows, int64_t num_graphs);
int mlqem_dense_plan_build(const int32_t* ptr, const int32_t* idx, const int32_t* loops, const int32_t* order,
                           const int32_t* graph_ptr, int64_t num_graphs, int64_t num_rows, int64_t max_span, int32_t* counter,
                           int32_t* lrows, int32_t* records, uint8_t* row_flag, mlqem_stream_t stream);
/* 1 when the dense kernels serve this shape: one or two heads of at most 16 channels at a head pitch of 16 */
int mlqem_dense_attention_supported(int H, int C, int head_pitch);
/* mlqem_transformer_attention_train_f32 (pair-keyed dropout draws, no side table) with the rows of the plan's blocks on the matrix
 * cores: same arguments, outputs and statistics.  Two launches: the per-edge kernel over the rows outside the blocks, then the block
 * kernel. */
int mlqem_dense_attention_train_f32(const float* qkvs, int64_t ld, const int32_t* in_ptr, const int32_t* in_src,
                                    const int32_t* loops, int64_t N, int64_t E, int H, int C, float drop_p, uint64_t seed,
                                    const uint64_t* seed_counter, int head_pitch, const int32_t* records, const int32_t* counter,
                                    const uint8_t* row_flag, int64_t max_blocks, float* out, int64_t ldo,
                                    float* attn_out, int64_t lda, float* stat_m, float* stat_den, mlqem_stream_t stream);
/* mlqem_transformer_attention_bwd_f32 in its recomputing form (no out_eid, no per-edge buffers; edge_al: [4 N H] floats, 16-byte
 * aligned) with a plan of the in-CSR for the destination side and one of the out-CSR for the source side.  Four launches, in this
 * order: destination side per-edge rows, destination side blocks, source side per-edge rows, source side blocks.  The source side
 * reads what BOTH destination-side launches file in edge_al. */
int mlqem_dense_attention_bwd_f32(const float* qkvs, int64_t ld, const float* g, int64_t ldg, const float* attn_out, int64_t lda,
                                  const float* stat_m, const float* stat_den, const int32_t* in_ptr, const int32_t* in_src,
                                  const int32_t* out_ptr, const int32_t* out_dst, const int32_t* loops, int64_t N, int64_t E, int H,
                                  int C, float drop_p, uint64_t seed, const uint64_t* seed_counter, int head_pitch,
                                  const int32_t* in_records, const int32_t* in_counter, const uint8_t* in_flag, int64_t in_max_blocks,
                                  const int32_t* out_records, const int32_t* out_counter, const uint8_t* out_flag,
                                  int64_t out_max_blocks, float* gqkvs, int64_t ldq, float* edge_al,
                                  mlqem_stream_t stream);

/* ASAPooling's cluster sums over the same plans (csrc/dense_pool.hip; rows of at most 48 channels: mlqem_dense_pool_supported -- two or
 * three channel tiles of 16; the scans and the backward entry points take D = 29..32 in rows of exactly 32 floats or D = 45..48 in rows of
 * exactly 48, the second pooling of the heads-3/2 and of the heads-5/3 variants, gnn.py:70-276).  The dense attention entry points above
 * take one to three heads.
 * mlqem_csr_softmax_aggregate_f32 with the rows of the plan's blocks on the matrix cores; stat (optional, [N, 2] floats, 8-byte
 * aligned) receives {maximum, 1 / denominator} of the block rows for the backward kernels below. */
int mlqem_dense_pool_supported(int D);
/* The pooling's other walks over the plans, for matrices whose rows are exactly 32 floats (29-32 channels, 16-byte aligned; anything
 * else: MLQEM_ERR_UNSUPPORTED / BAD_ARG, the caller keeps the per-edge entry points):
 *   mlqem_dense_segment_max_f32           = mlqem_csr_segment_max_f32 (the row itself included)
 *   mlqem_dense_softmax_aggregate_bwd_f32 = mlqem_csr_softmax_aggregate_bwd_f32 in its recomputing form with tie counts (edge_al: [4 N]
 *                                           floats, 16-byte aligned); stat: what mlqem_dense_softmax_aggregate_f32 left
 *   mlqem_dense_segment_max_bwd_f32       = mlqem_csr_segment_max_bwd_f32 with tie counts and a rank-one gradient of the maximum */
/* mlqem_leconv_fitness_bwd_f32 with the rows of the OUT structure's plan (lrows / counter / row_flag of mlqem_dense_plan_build) summed
 * by a wave each instead of a thread. */
int mlqem_dense_leconv_fitness_bwd_f32(const float* gfit, const float* fitness, const int32_t* in_ptr, const int32_t* out_ptr,
                                       const int32_t* out_dst, int64_t N, const int32_t* lrows, const int32_t* counter,
                                       const uint8_t* row_flag, int64_t max_blocks, float* gpqr, mlqem_stream_t stream);
int mlqem_dense_segment_max_f32(const float* x, int64_t ldx, const int32_t* in_ptr, const int32_t* in_src, int64_t N, int D,
                                const int32_t* records, const int32_t* counter, const uint8_t* row_flag, int64_t max_blocks, float* out,
                                int64_t ldo, mlqem_stream_t stream);
int mlqem_dense_softmax_aggregate_bwd_f32(const float* x, int64_t ldx, const float* xnew, int64_t ldn, const float* gnew, int64_t ldg,
                                          const int32_t* in_ptr, const int32_t* in_src, const int32_t* out_ptr, const int32_t* out_dst,
                                          const float* a_dst, const float* c_src, float negative_slope, int64_t N, int64_t E, int D,
                                          const float* stat, const int32_t* in_records, const int32_t* in_counter, const uint8_t* in_flag,
                                          int64_t in_max_blocks, const int32_t* out_records, const int32_t* out_counter,
                                          const uint8_t* out_flag, int64_t out_max_blocks, float* gx, int64_t ldgx, float* g_a, float* g_c,
                                          float* edge_al, const float* xmax, int64_t ldm, float* tie_count, int64_t ldt,
                                          const float* gx_rank1, mlqem_stream_t stream);
int mlqem_dense_segment_max_bwd_f32(const float* x, int64_t ldx, const float* xmax, int64_t ldm, const int32_t* in_ptr,
                                    const int32_t* in_src, const int32_t* out_ptr, const int32_t* out_dst, int64_t N, int D, float* gx,
                                    int64_t ldgx, float* gshare, int64_t lds, const float* tie_count, int64_t ldt, const float* gmax_row,
                                    const float* gmax_col, const int32_t* out_records, const int32_t* out_counter, const uint8_t* out_flag,
                                    int64_t out_max_blocks, mlqem_stream_t stream);
int mlqem_dense_softmax_aggregate_f32(const float* x, int64_t ldx, const int32_t* in_ptr, const int32_t* in_src, const float* a_dst,
                                      const float* c_src, float negative_slope, int64_t N, int D, const int32_t* records,
                                      const int32_t* counter, const uint8_t* row_flag, int64_t max_blocks, float* out, int64_t ldo,
                                      float* stat, mlqem_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Host-side native encoder (no GPU needed).  Replaces the Python loops of circuit_to_graph_data_json
 * (blackwater/data/utils.py:198-389) for the part ExpValueEntry.to_pyg_data consumes
 * (blackwater/data/generators/exp_val.py:63-70): the op-node feature matrix and the op->op qubit-wire edges, in the
 * reference's node and edge order, as float64 (the reference holds Python floats).
 * ---------------------------------------------------------------------------------------------------- */
typedef struct mlqem_backend_props {
  int num_qubits;                    /* length of t1 / t2 / readout */
  const double* t1;                  /* seconds, as get_backend_properties_v1 stores them */
  const double* t2;
  const double* readout;
  int num_gate_types;                /* len(properties["gates_set"]); "barrier" and "measure" are appended internally */
  const char* const* gate_names;     /* one-hot column order */
  int num_gate_props;                /* entries of properties["gate_props"] */
  const char* const* gate_keys;      /* "cx_0_1", "sx_3", ... */
  const double* gate_error;
  const double* gate_length;
} mlqem_backend_props;

/* Two-call pattern.  Size query: x == NULL -> *num_nodes, *num_edges, *num_features, *depth are filled.  Fill: pass
 * buffers x[N*F], edge_src[E], edge_dst[E], edge_attr[E*3] (edge_attr may be NULL) with *num_nodes / *num_edges set to
 * their capacities.  Errors: MLQEM_ERR_UNSUPPORTED for a well-formed circuit the encoding does not cover (a gate
 * outside gates_set, a non-barrier gate on more than 3 qubits, more than 3 parameters, a qubit beyond the calibration
 * table: where the reference raises); MLQEM_ERR_BAD_ARG for text that is not OpenQASM 2 (unbalanced or too deeply nested
 * parentheses -- angle expressions nest at most 64 levels --, bad or out-of-range indices, mismatched register sizes,
 * more than 2^20 register bits, truncated statements).  mlqem_encode_last_error() has the message (per thread).  The
 * parser is bounded: no input makes it recurse or allocate beyond these limits (csrc `make asan` runs it under
 * AddressSanitizer / UBSan over a malformed corpus, tests/test_encoder_fuzz.py). */
int mlqem_encode_qasm(const char* qasm, const mlqem_backend_props* props, int use_qubit_features, int use_gate_features,
                      int64_t* num_nodes, int64_t* num_edges, int* num_features, int* depth, double* x,
                      int32_t* edge_src, int32_t* edge_dst, double* edge_attr);
const char* mlqem_encode_last_error(void);

/* The same encoding for ALL circuits of one estimator run() (NgemJob.result loops over them one by one:
 * blackwater/library/ngem/estimator.py:49-84), as the COLLATED batch the models consume (what PyG's Batch.from_data_list makes
 * of the per-circuit Data objects, docs/tutorials/__ml_models.py:105-119), on `threads` host threads (0 = one per core, at
 * most 16).  Two calls, so that the caller owns every output buffer at its exact size:
 *   parse: scans and checks every text; node_ptr[count+1] / edge_ptr[count+1] are the prefix sums of the circuits' node and
 *          edge counts, depths[count] (optional) their depths, *num_features the row width; *handle keeps the parsed circuits.
 *          On an error nothing is kept, *failed (optional) is the index of the first bad circuit and the message names it.
 *   fill:  x[node_ptr[count], F] as float32 (the rounding the reference's torch.tensor(..., dtype=float) applies),
 *          edge_src / edge_dst[edge_ptr[count]] as int64 with each circuit's node offset added (the two rows of edge_index),
 *          batch[node_ptr[count]] (optional) = the circuit index of every node.  May be called more than once.
 *   free:  releases the handle (NULL is fine).
 * Same error codes as mlqem_encode_qasm; same arrays, circuit by circuit (tests/test_native_encoder.py). */
int mlqem_qasm_batch_parse(const char* const* qasm, int64_t count, const mlqem_backend_props* props, int use_qubit_features,
                           int use_gate_features, int threads, void** handle, int64_t* node_ptr, int64_t* edge_ptr,
                           int* depths, int* num_features, int64_t* failed);
int mlqem_qasm_batch_fill(void* handle, int threads, float* x, int64_t* edge_src, int64_t* edge_dst, int64_t* batch);
void mlqem_qasm_batch_free(void* handle);

/* The parsed batch as a COMPACT OP STREAM for device-side expansion (round 4; mlqem_encode_expand below): 16 bytes per op and two
 * bytes per qubit argument instead of the 112 bytes per node of rows and indices mlqem_qasm_batch_fill writes -- a 1024-circuit
 * run() of 100-qubit circuits uploads 0.2 GB instead of 1.3 GB and the host writes a seventh of the bytes.
 *   mlqem_op_rec:  p0 = the first parameter as float32 (what the row holds); q[] = calibration indices (Qubit.index) of up to
 *                  three qargs (unused for barriers); slot = one-hot column; meta = q_cnt (bits 0-1, 0 for a barrier) | barrier
 *                  (bit 2) | p_cnt (bits 4-5); winc = index of the op's first qubit argument in `wires` (the next op's winc, or
 *                  the circuit's wire_ptr end, closes the range).
 *   wires:         the circuit-local wire (flat qubit number) of EVERY qubit argument, op after op -- what the op -> op edges
 *                  are built from (utils.py:334-347: one edge per qubit wire from the previous op on it).
 *   mlqem_x_patch: x[node, col] = value for what the record has no room for (second / third parameters; the calibration entry
 *                  of a gate on three qubits); unused slots hold node = 0xFFFFFFFF.
 * stream_sizes: wire_ptr / patch_ptr [count + 1] = prefix sums of the circuits' wire and patch-slot counts, *max_wires the widest
 * circuit; stream_fill writes the three arrays (node_ptr as from mlqem_qasm_batch_parse).  MLQEM_ERR_UNSUPPORTED beyond 65 535
 * wires / calibration qubits or 2^32 ops. */
typedef struct mlqem_op_rec { float p0; uint16_t q[3]; uint8_t slot; uint8_t meta; uint32_t winc; } mlqem_op_rec;
typedef struct mlqem_x_patch { uint32_t node; uint32_t col; float value; } mlqem_x_patch;
int mlqem_qasm_batch_stream_sizes(void* handle, int64_t* wire_ptr, int64_t* patch_ptr, int* max_wires);
int mlqem_qasm_batch_stream_fill(void* handle, int threads, const int64_t* wire_ptr, const int64_t* patch_ptr, mlqem_op_rec* ops,
                                 uint16_t* wires, mlqem_x_patch* patches);
/* g1[(G + 2) * Q], g2[(G + 2) * Q * Q] (G = num_gate_types, Q = num_qubits): index into gate_error / gate_length of the
 * calibration entry of (one-hot slot, qubit) / (slot, qubit, qubit), -1 where there is none -- the lookups of utils.py:263-269 as
 * tables the device indexes.  Keys naming a qubit >= num_qubits have no place in the tables and are left out: the host string lookup
 * would still find such a key, but no circuit the encoder accepts addresses that qubit (ops on qubits >= num_qubits are refused),
 * so the two lookups agree on every op that can occur. */
int mlqem_props_gate_tables(const mlqem_backend_props* props, int32_t* g1, int32_t* g2);

/* Device-side expansion of the op stream (all pointers device memory): x[N, F] (row stride ldx >= F; F = 3 + num_slots + 9 (qubit
 * features) + 2 (gate features)), edge_src / edge_dst[E] as int64 with node offsets applied (the two rows of edge_index, in the
 * reference's edge order), batch[N] (optional): the arrays mlqem_qasm_batch_fill writes, bit for bit.  ops / wires / patches as
 * above; node_ptr[B + 1] as from mlqem_qasm_batch_parse; W = wire_ptr[B]; E = edge_ptr[B]; t1 / t2 / readout: the calibration
 * table as float32 (the rounding the rows get); g1 / g2: mlqem_props_gate_tables; gate_error / gate_length as float32;
 * num_slots = num_gate_types + 2.  Edges: a stable radix sort of the qubit arguments by (circuit, wire) puts every wire's ops in
 * program order; neighbours are the endpoints of an edge; a source's out-edges are listed latest-inserted first, as the
 * reference's DAG hands them back (blackwater/data/utils.py:334-347).  Asynchronous on `stream`;
 * replaces circuit_to_graph_data_json + ExpValueEntry.to_pyg_data + Batch.from_data_list for a run() of circuits
 * (blackwater/library/ngem/estimator.py:49-84). */
size_t mlqem_encode_expand_workspace_bytes(int64_t N, int64_t W);
int mlqem_encode_expand(const mlqem_op_rec* ops, const uint16_t* wires, const mlqem_x_patch* patches, int64_t num_patches,
                        const int64_t* node_ptr, int64_t N, int64_t W, int64_t E, int64_t B, int max_wires, const float* t1,
                        const float* t2, const float* readout, int num_cal_qubits, const int32_t* g1, const int32_t* g2,
                        const float* gate_error, const float* gate_length, int num_slots, int use_qubit_features,
                        int use_gate_features, float* x, int64_t ldx, int64_t* edge_src, int64_t* edge_dst, int64_t* batch,
                        void* workspace, size_t workspace_bytes, mlqem_stream_t stream);

/* Circuit-level features of the MLP regressors -- the per-circuit part of encode_data / encode_data_v2_ecr
 * (docs/tutorials/mlp.py:111-145 count_gates_by_rotation_angle, :148-252; == blackwater/library/learning/mlp.py) from
 * the same op scan as the graph encoder (host CPU):
 *   gate_counts[i] = number of ops named gate_names[i]                  (QuantumCircuit.count_ops lookups)
 *   angle_hist[b]  = number of one-qubit rx/ry/rz ops whose angle lies in bin b of bin_edges[num_edges]
 *                    (numpy.histogram rule: [e_b, e_b+1), last bin closed; values outside are dropped).
 * The caller passes the edges (numpy.arange(-2pi, 2pi + bin, bin) in the reference) so both sides bin identically. */
int mlqem_circuit_features_qasm(const char* qasm, const char* const* gate_names, int num_gates, const double* bin_edges,
                                int num_edges, int64_t* gate_counts, int64_t* angle_hist);
/* The same for every circuit of one run() (PostProcessedJob.result loops over them: blackwater/library/learning/estimator.py:
 * 220-245) on `threads` host threads (0 = one per core, at most 16): gate_counts[count, num_gates], angle_hist[count,
 * num_edges - 1].  On an error *failed (optional) is the index of the first bad circuit and the message names it. */
int mlqem_circuit_features_qasm_batch(const char* const* qasm, int64_t count, const char* const* gate_names, int num_gates,
                                      const double* bin_edges, int num_edges, int threads, int64_t* gate_counts,
                                      int64_t* angle_hist, int64_t* failed);

/* ------------------------------------------------------------------------------------------------------
 * Regression-forest inference (ABI 45).  Replaces model.predict(X) of a fitted scikit-learn RandomForestRegressor /
 * ExtraTreesRegressor / DecisionTreeRegressor on encode_data rows (blackwater/library/learning/estimator.py:90-148
 * ScikitLearningModelProcessor; docs/tutorials/vqe_rf*.py; docs/demos/demo1_rf_mimic_zne_100q_twirl.ipynb):
 *
 *   out[r, :] = (1 / T) * sum_{t = 0 .. T-1} values[tree_ptr[t] + leaf_t(x[r, :]), :]
 *
 * where leaf_t walks tree t from its root with the rule "go left iff x[r, feature] <= threshold".
 *
 * Node layout.  The nodes of tree t are nodes[tree_ptr[t] .. tree_ptr[t + 1]) in DEPTH-FIRST PRE-ORDER: node 0 is the root and
 * the left child of node i is node i + 1, so a 16-byte record holds everything a step needs (one 16-byte load per level):
 *   thr     the split threshold as float32, rounded TOWARD MINUS INFINITY from the model's float64 threshold.  For a float32 x,
 *           x <= thr64  <=>  x <= thr32 (thr32 is the largest float32 not above thr64), so the fp32 compare takes scikit-learn's
 *           branch on every input; round-to-nearest does not.
 *   feature column of x the node splits on (0 .. F-1), or -1 for a leaf
 *   right   index within the tree (pre-order numbering) of the right child; a leaf holds its own index
 *   orig    index within the tree of this node IN THE CALLER'S ORIGINAL NUMBERING: what `leaf` reports (scikit-learn's
 *           apply()) and the row of `values` a leaf reads -- values[(tree_ptr[t] + orig) * K + k] (float64) keeps the model's order.
 * tree_ptr[T + 1] (int64, device): tree_ptr[0] = 0, strictly increasing (every tree has a root).
 * The walk takes at most max_depth steps (the forest's recorded depth: root = depth 0), whatever the node table holds, and every
 * index it forms from a node record is clamped to the tree / to F: a malformed table gives a wrong answer, never a spin or an
 * out-of-range read.  x is float32 [n_rows, F] with row stride ldx >= F (columns beyond F are never read).  A NaN feature
 * compares false and takes the RIGHT branch (scikit-learn without missing-value support does the same; the encoders emit none).
 * The sum over trees is formed in float64 in tree order, by one thread per (row, output), and divided by T once: results are
 * bit-identical from call to call and do not depend on n_rows or on how rows are tiled over workgroups.  No workspace.
 * leaf (optional): int32 [n_rows, T].  Serves 1 <= K <= 16, 1 <= F <= 32767, T >= 1, trees of any size an int32 indexes
 * (MLQEM_ERR_UNSUPPORTED beyond); n_rows == 0 returns MLQEM_OK without a launch.
 * ---------------------------------------------------------------------------------------------------- */
typedef struct mlqem_forest_node { float thr; int32_t feature; int32_t right; int32_t orig; } mlqem_forest_node;
int mlqem_forest_predict_f32(const float* x, int64_t ldx, int64_t n_rows, int F, const mlqem_forest_node* nodes,
                             const int64_t* tree_ptr, int T, const double* values, int K, int max_depth, double* out,
                             int32_t* leaf, mlqem_stream_t stream);

/* Out-of-bag prediction (ABI 48).  Replaces the oob_prediction_ of RandomForestRegressor(oob_score=True): every row is scored by the
 * trees whose bag does not hold it,
 *
 *   out[r, k] = (1 / n_oob[r]) * sum_{t : counts[t, r] == 0} values[(tree_ptr[t] + leaf_t(x[r, :])) * K + k]
 *
 * with n_oob[r] the number of such trees.  counts is int32 [T][ldc] with ldc >= n_rows (device): counts[t * ldc + r] == 0  <=>  tree
 * t is out of bag for row r.  Any non-zero count means in bag; a count is never used as an index.  A row with n_oob[r] == 0 gets
 * out[r, :] = 0.0 (scikit-learn's behaviour).  out is float64 [n_rows, K], n_oob int32 [n_rows], leaf (optional) int32 [n_rows, T]:
 * the leaf in the model's numbering, or -1 for an in-bag pair.  Nodes, tree_ptr, values, x and max_depth are those of
 * mlqem_forest_predict_f32, and it is the same kernel: an in-bag pair does not walk.
 * The walk takes at most max_depth steps, whatever the node table holds, and every index it forms from a node record or from counts
 * is clamped: a malformed table gives a wrong answer, never a spin or an out-of-range read.  Every load is unconditional on a clamped
 * address and masked by a select, the counts load of a lane past the last row or the last tree included.
 * The sum over trees is formed in float64 in tree order, by one thread per (row, output), and divided by n_oob[r] once: results are
 * bit-identical from call to call and do not depend on n_rows, on how rows are tiled over workgroups (64, 16 or 4 rows) or on ldc.
 * No atomics and no workspace.  With scikit-learn's own bags the result equals its oob_prediction_ bit for bit (it adds in estimator
 * order as well).  Serves 1 <= K <= 16, 1 <= F <= 32767, T >= 1 (MLQEM_ERR_UNSUPPORTED beyond); counts and n_oob non-null and
 * ldc >= n_rows besides the checks of mlqem_forest_predict_f32 (MLQEM_ERR_BAD_ARG); n_rows == 0 returns MLQEM_OK without a launch. */
int mlqem_forest_predict_oob_f32(const float* x, int64_t ldx, int64_t n_rows, int F, const mlqem_forest_node* nodes,
                                 const int64_t* tree_ptr, int T, const double* values, int K, int max_depth,
                                 const int32_t* counts, int64_t ldc, double* out, int32_t* n_oob, int32_t* leaf,
                                 mlqem_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Growing a regression forest (ABI 47).  Replaces RandomForestRegressor(...).fit(X_train, y_train) with scikit-learn's defaults
 * (docs/tutorials/vqe_rf*.py, both demos, h15 / h19 / h21 / h26 / h33 / h36): exact CART with squared error, the best splitter
 * over all features, grown level by level for a chunk of Tc trees at once.  blackwater.native.ops.forest_fit drives it.
 *
 * The rule (scikit-learn 1.7's best splitter with the MSE criterion, restated).  A tree's rows are the rows with counts[t, r] > 0
 * and its weights are the counts; a node's sample count is its number of DISTINCT in-bag rows (a bag handed over as sample
 * weights).  With W = sum w, S_k = sum w y_k, Q = sum w sum_k y_k^2 over the node's rows: value = S / W, impurity =
 * (Q / W - sum_k (S_k / W)^2) / K.  A node at depth d is a leaf when d >= max_depth, rows < min_samples_split,
 * rows < 2 min_samples_leaf, impurity <= 2.220446049250313e-16, or it has no candidate.  A candidate of feature f separates
 * positions p - 1 | p of the node's rows sorted by x[:, f]; it exists where v[p] > v[p - 1] + 1e-7f in float32 and both sides keep
 * min_samples_leaf rows.  Its score is sum_k sl_k^2 / wl + sum_k (S_k - sl_k)^2 / (W - wl) with (wl, sl) the sums of the left
 * side; the highest score wins, on equal scores the lowest feature and then the lowest position (scikit-learn draws the feature
 * order at random).  Any candidate is taken, a zero-gain one included.  threshold = double(v[p - 1]) / 2 + double(v[p]) / 2,
 * replaced by double(v[p - 1]) when that sum equals double(v[p]) or is infinite; rows with x[f] <= threshold go left.
 *
 * mlqem_forest_fit_state: the inputs and the workspace of one chunk of Tc trees, every pointer device memory of the caller.
 *   x float32 [n, F] with row stride ldx >= F, finite; y float64 [n, K], finite; counts int32 [Tc, n] >= 0, every tree with a
 *   positive one; order int32 [F, n]: order[f] = a STABLE argsort of x[:, f] (the same for every tree).
 *   rows [2][Tc][F][n], segid [2][Tc][n], level [2][Tc][4], seg_i [2][Tc][n][4] (int32; level, seg_i 16-byte aligned): the
 *   double-buffered row lists, per-position segment ids, (live segments, live positions, nodes so far, 0) per tree and
 *   (first position, rows, node, feature whose list orders the sums) per live segment.  seg_stat float64 [Tc][n][K + 2] = (W, Q,
 *   S[K]).  cand_score float64 / cand_pos int32 [Tc][F][n]: the best candidate per (tree, feature, segment), cand_pos = p or -1.
 *   split_i int32 [Tc][n][4] (16-byte aligned) = (split feature or -1, first position in the next list, rows going left, left
 *   child's segment) and split_thr float64 [Tc][n] per segment of the level.
 *   Output, per tree at most 2 n - 1 nodes, node 0 the root, children appended level by level: node_i int32 [Tc][2n-1][4]
 *   (16-byte aligned) = (feature or -2, left, right, rows; left = right = -1 for a leaf), node_thr float64 [Tc][2n-1],
 *   node_value float64 [Tc][2n-1][K].  mlqem_forest_fit_tree_bytes(n, F, K) is the sum of these sizes for ONE tree.
 *
 * mlqem_forest_fit_init fills buffer 0 (the root's lists: `order` compacted to the in-bag rows, stable) and level / seg_i of the
 * root.  Level d = 0, 1, ... is then mlqem_forest_fit_stats, _search, _select, _partition with level = d, in this order on one
 * stream; they read buffer d & 1 and write the other.  After _select of level d, level[(d + 1) & 1][t] holds tree t's live
 * segments of level d + 1 and its node count: the caller reads it and stops when no tree has a live segment (at most
 * min(max_depth, n - 1) + 1 levels).  A tree without live segments costs nothing but its workgroups' first load.
 *
 * Determinism: no atomics.  Every sum is a segmented scan over 256-position tiles in list order with the running sums carried
 * from tile to tile, so it depends on (n, F, K, counts) alone: two fits give the same bits, and so does any chunking of the trees
 * (a tree reads no other tree's state).  Safety: every loop is bounded by n, F or K; every index read from the workspace is clamped
 * before it addresses memory; no workgroup waits for another.  Serves 1 <= n <= 2^22, 1 <= F <= 32767, 1 <= K <= 16, Tc F < 2^31
 * (MLQEM_ERR_UNSUPPORTED beyond); min_samples_split >= 2, min_samples_leaf >= 1, max_depth >= 0 and non-null, aligned buffers
 * (MLQEM_ERR_BAD_ARG otherwise), all checked before a launch.  The node table is NOT validated here: ForestRegressor.fit passes it
 * through the same host validation as from_arrays before mlqem_forest_predict_f32 sees it.
 *
 * Feature subsets per node (max_features = m, 1 <= m <= F; an additive symbol, the ABI version is unchanged).  With m == F nothing
 * above changes.  With m < F a node that meets no leaf condition searches a subset of the features:
 *   1. Feature order.  The node has its own permutation pi of 0 .. F-1, a pure function of (seed, t, node, i): t the tree's index
 *      in the WHOLE forest (tree_base + its index in the chunk), node the node's index within its tree in the numbering above (root
 *      0, children appended level by level: the third field of a seg_i record).  All arithmetic is uint32:
 *        mix(x):  x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;  x *= 0x846ca68b;  x ^= x >> 16
 *        key   =  mix(mix(mix(seed) ^ t) ^ node)
 *        h     =  max(1, ceil(bit_length(F - 1) / 2));   mask = 2^h - 1;   D = 4^h        (F <= D <= 4 F)
 *        E(v):    (L, R) = (v >> h, v & mask)
 *                 for r = 0 .. 7:  (L, R) = (R, L ^ (mix(R ^ key ^ (r * 0x9e3779b9)) & mask))
 *                 return (L << h) | R
 *        pi(i) =  the first of E(i), E(E(i)), ... that is below F
 *      E is a bijection of [0, D) (eight Feistel rounds; four leave pair frequencies visibly uneven at small F), so pi is a
 *      bijection of [0, F) by cycle walking; the walk is bounded by D steps and its result clamped to F - 1.
 *   2. Visited features.  The node visits pi(0), pi(1), ... and stops after c features, c the smallest count >= m for which a
 *      visited feature has a candidate (cand_pos >= 0 for this tree, feature and segment).  If no feature has one the node is a leaf.
 *   3. Winner.  Among the visited features the highest score wins; on equal scores the lowest feature index, then the lowest
 *      position.  The threshold and everything downstream are unchanged.
 * Deviation from scikit-learn: it keeps drawing while every visited feature is CONSTANT in the node; here a feature counts only
 * once it has a CANDIDATE.  The two differ only with min_samples_leaf > 1, where scikit-learn may stop at a feature that varies but
 * has no admissible split and this rule goes on drawing.  scikit-learn's random stream is not reproduced: the subsets, like the
 * bags, are the project's own.
 * mlqem_forest_fit_select_subset(state, level, max_features, seed, tree_base, stream) takes the place of mlqem_forest_fit_select in
 * the level's sequence; tree_base is the forest index of the chunk's first tree.  One workgroup per tree, one thread per segment, the
 * same leaf tests, threshold, node record and numbering scans as _select (one body serves both); the visit loop is bounded by F and
 * the cycle walk by D, every feature index is clamped before it addresses cand_score / cand_pos, the loads are unconditional and
 * masked (every lane runs to its wave's largest count), no atomics, no workgroup waits for another.  max_features >= F gives the
 * bits of mlqem_forest_fit_select (it launches that kernel).  The checks of the other entries, and max_features >= 1, tree_base
 * >= 0, level >= 0 (MLQEM_ERR_BAD_ARG), all before a launch.  _search and _partition still walk all F lists: in this layout a per-node
 * subset cannot skip a list, so max_features buys variety between the trees, not time.
 * ---------------------------------------------------------------------------------------------------- */
typedef struct mlqem_forest_fit_state {
  const float* x; int64_t ldx; const double* y; const int32_t* counts; const int32_t* order;
  int64_t n; int32_t F, K, Tc, min_samples_split, min_samples_leaf, max_depth;
  int32_t* rows; int32_t* segid; int32_t* level; int32_t* seg_i; double* seg_stat;
  double* cand_score; int32_t* cand_pos; int32_t* split_i; double* split_thr;
  int32_t* node_i; double* node_thr; double* node_value;
} mlqem_forest_fit_state;
size_t mlqem_forest_fit_tree_bytes(int64_t n, int F, int K);
int mlqem_forest_fit_init(const mlqem_forest_fit_state* state, mlqem_stream_t stream);
int mlqem_forest_fit_stats(const mlqem_forest_fit_state* state, int level, mlqem_stream_t stream);
int mlqem_forest_fit_search(const mlqem_forest_fit_state* state, int level, mlqem_stream_t stream);
int mlqem_forest_fit_select(const mlqem_forest_fit_state* state, int level, mlqem_stream_t stream);
int mlqem_forest_fit_select_subset(const mlqem_forest_fit_state* state, int level, int max_features, uint32_t seed,
                                   int64_t tree_base, mlqem_stream_t stream);
int mlqem_forest_fit_partition(const mlqem_forest_fit_state* state, int level, mlqem_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Gradient-boosted regression trees, squared error (additive symbols, the ABI version is unchanged).  Replaces
 * GradientBoostingRegressor(...).fit / .predict of scikit-learn on encode_data rows (the notebooks that build the random-forest
 * mitigator import it in the same line: h15, h18, h19, h20, h21, h26, h33, h36, demo1, demo2).  blackwater.native.ops.boost_fit /
 * boost_predict and blackwater.nn.BoostedRegressor drive them.  Both kernels are compiled without floating-point contraction: the
 * contracts below are stated operation by operation.
 *
 * mlqem_boost_predict_f32 scores an ensemble stored as mlqem_forest_predict_f32 takes a forest with K = 1 (nodes in pre-order,
 * tree_ptr, values float64 [N]; the walk, the clamps and the thr32 rule are those of the forest kernel):
 *
 *   out[r] = ((init + lr * v_0) + lr * v_1) + ... + lr * v_{n_stages-1},     v_t = values[tree_ptr[t] + leaf_t(x[r, :])]
 *
 * in stage order, one rounded multiply and one rounded add per stage in float64 -- scikit-learn's predict_stages, bit for bit.
 * n_stages <= T (tree_ptr holds at least n_stages + 1 entries): a prefix of the ensemble scores without repacking.  staged
 * (optional): float64 [n_stages][lds], lds >= n_rows, staged[t * lds + r] = the running sum of row r after stage t; the threads of a
 * tile write consecutive rows.  One thread owns a row's sum; loads are unconditional on clamped indices; the walk's trip count is
 * wave-uniform and at most max_depth; no atomics, no workspace; results are bit-identical across calls, n_rows and tile sizes (64, 16
 * or 4 rows a workgroup); capturable in a hipGraph.  Serves 1 <= F <= 32767 (MLQEM_ERR_UNSUPPORTED beyond); n_stages >= 1, ldx >= F,
 * lds >= n_rows with staged, non-null 16-byte aligned nodes (MLQEM_ERR_BAD_ARG); n_rows == 0 returns MLQEM_OK without a launch.
 *
 * mlqem_boost_update_f64 is the step between two stages of a fit.  It reads the stage's tree in the numbering of the fit workspace
 * (mlqem_forest_fit_state with K = 1: node_i = (feature or -2, left, right, rows), node_thr, node_value; n_nodes entries, node 0 the
 * root) and, one thread per row r of x (float32 [n_rows, F], row stride ldx):
 *   leaf    walk from the root, "go left iff double(x[r, feature]) <= node_thr" (scikit-learn's compare), at most max_depth + 1
 *           steps under a wave-uniform exit, every feature clamped to F and every child to n_nodes;
 *   raw[r]   = raw[r] + lr * node_value[leaf]        (a rounded multiply, then a rounded add)
 *   resid[r] = y[r] - raw[r]
 * A tree of at most 511 nodes is staged in LDS, a larger one is read from global memory.  mask (int32 [n_rows] or null = every row):
 * non-zero means the row is in the stage's bag.  The same launch writes ONE record of four float64 sums per workgroup of 256 rows,
 * partial[block * 4 + (0..3)] = (sum over in-bag rows of resid^2 after the update, sum over out-of-bag rows of (y - raw)^2 before it,
 * the same after it, the number of in-bag rows), each summed by a shuffle tree within a wave and then wave 0..3 in order: the same
 * bits from call to call.  mlqem_boost_update_blocks(n_rows) is the number of records (ceil(n_rows / 256)); the caller adds them in
 * block order.  No atomics, no workspace, no workgroup waits for another.  Serves n_rows <= 2^22, F <= 32767
 * (MLQEM_ERR_UNSUPPORTED beyond); n_rows >= 1, n_nodes >= 1, max_depth >= 0, ldx >= F, non-null buffers and a 16-byte aligned node_i
 * (MLQEM_ERR_BAD_ARG), all checked before the launch.
 * ---------------------------------------------------------------------------------------------------- */
int mlqem_boost_predict_f32(const float* x, int64_t ldx, int64_t n_rows, int F, const mlqem_forest_node* nodes,
                            const int64_t* tree_ptr, int n_stages, const double* values, int max_depth, double init, double lr,
                            double* out, double* staged, int64_t lds, mlqem_stream_t stream);
int64_t mlqem_boost_update_blocks(int64_t n_rows);
int mlqem_boost_update_f64(const float* x, int64_t ldx, int64_t n_rows, int F, const int32_t* node_i, const double* node_thr,
                           const double* node_value, int n_nodes, int max_depth, double lr, const double* y, double* raw,
                           double* resid, const int32_t* mask, double* partial, mlqem_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Linear least squares (ABI 46).  Replaces ols.fit(X, y) / ols.predict(X) of a scikit-learn LinearRegression (or Ridge) on
 * encode_data rows (docs/tutorials/h12_ols.ipynb, h17_compare_over_steps.ipynb; ScikitLearningModelProcessor(ols, ...) in the VQE
 * drivers).  The fit is one streaming pass over the rows on the device (the moments below) and a solve of at most 529 x 529 on the
 * host (blackwater.nn.linear_model.solve_moments); scoring is one launch.
 *
 * mlqem_linreg_moments_f32: with A = [1 | x | y] (n_rows x D, D = 1 + F + K) writes moments = A^T A as float64 [D, D], both
 * triangles filled: row 0 holds n, the column sums of x and the column sums of y.  x is float32 [n_rows, F] with row stride
 * ldx >= F, y float32 [n_rows, K] with row stride ldy >= K; columns beyond F and K are never read.  The float32 inputs are
 * widened to fp64 before they are multiplied, so every product is exact (24 + 24 bits <= 53) and only the summation rounds: an
 * entry is within n 2^-53 sum|a_i b_i| of the exact one.
 * Determinism: no atomics.  The rows are cut into chunks whose size is a function of (n_rows, F, K) alone, every chunk's partial
 * sums go to `workspace` (mlqem_linreg_moments_workspace_bytes(n_rows, F, K) bytes, 16-byte aligned; MLQEM_ERR_WORKSPACE when
 * smaller) and a final kernel adds them in chunk order and writes M[i, j] and M[j, i] from the same sum: results are bit-identical
 * from call to call and exactly symmetric.
 * accumulate != 0 adds to what `moments` holds (a streaming fit over shards; a sum over ranks later); accumulate == 0 overwrites.
 * With n_rows == 0 the call writes zeros (accumulate == 0) or nothing (accumulate != 0) and launches no kernel.
 * Serves 1 <= F <= 512 and 1 <= K <= 16 (MLQEM_ERR_UNSUPPORTED beyond).  Negative sizes, ldx < F and ldy < K give
 * MLQEM_ERR_BAD_ARG; all arguments are checked before anything is launched.  Capturable in a hipGraph.
 *
 * mlqem_linreg_predict_f32: out[r, k] = intercept[k] + sum_j coef[k, j] * x[r, j], with coef float64 [K, F] (row-major,
 * scikit-learn's coef_), intercept float64 [K] and out float64 [n_rows, K].  The sum is formed in fp64 with fused multiply-adds in
 * column order j = 0 .. F-1, starting from the intercept, by one thread per row: results are bit-identical from call to call and do
 * not depend on n_rows or on how rows are tiled over workgroups.  No workspace; capturable in a hipGraph; n_rows == 0 returns
 * MLQEM_OK without a launch.  The same F and K limits.
 * ---------------------------------------------------------------------------------------------------- */
size_t mlqem_linreg_moments_workspace_bytes(int64_t n_rows, int F, int K);
int mlqem_linreg_moments_f32(const float* x, int64_t ldx, const float* y, int64_t ldy, int64_t n_rows, int F, int K,
                             double* moments, int accumulate, void* workspace, size_t workspace_bytes, mlqem_stream_t stream);
int mlqem_linreg_predict_f32(const float* x, int64_t ldx, int64_t n_rows, int F, const double* coef, const double* intercept,
                             int K, double* out, mlqem_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Exact simulation of small circuits, a batch per call (an additive symbol, the ABI version is unchanged).  Produces the labels the mitigators learn from: ideal expectation
 * values from a state vector, noisy ones from a density matrix with depolarising and readout ops (the reference gets them from
 * Aer: blackwater/data/generators/exp_val.py, data/utils.py create_estimator_meas_data).  blackwater.sim lowers circuits to this
 * format (compile_programs) and blackwater.native.ops.sim_run calls it.
 *
 * State.  Complex float64 amplitudes (re, im) in LDS for the whole circuit, starting from |0..0>; nothing of it touches global
 * memory.  mode 0: an n-qubit state vector, 2^n amplitudes, qubit q = index bit q (qubit 0 the least significant: qiskit's order).
 * mode 1: an n-qubit density matrix as a 2n-bit vector, 4^n entries, entry rho[r, c] at index r | c << n.
 * Cap: MLQEM_SIM_MAX_AMPS = 2 048 amplitudes (32 KB of LDS): n <= 11 in mode 0, n <= 5 in mode 1.  There is no global-memory path.
 *
 * circ    int32 [n_circuits][4], 16-byte aligned: (n_qubits, mode, r, 0).  The LAST r ops of the circuit are its readout ops:
 *         norm is taken before them.  (The fourth field is 0 here; the measured entry points below read it as the number of
 *         measurement-tail records that follow the readout ops.)
 * op_ptr  int64 [n_circuits + 1]: circuit c owns ops[op_ptr[c] .. op_ptr[c + 1]).
 * ops     mlqem_sim_op [n_ops], 16-byte aligned: (kind, q0, q1, param).  param is the index of the record's first float64 in
 *         `params`.  A unitary in mode 1 acts as U on bit q and conj(U) on bit q + n from the ONE record.
 *           kind                 qubits   params
 *           MLQEM_SIM_OP_U1      q0       8: a 2x2 complex matrix, row-major, (re, im) per entry
 *           MLQEM_SIM_OP_DIAG1   q0       4: diag(d0, d1), (re, im) each                    (rz, p, z, s, t and their inverses)
 *           MLQEM_SIM_OP_CX      q0, q1   -   q0 controls, q1 is flipped
 *           MLQEM_SIM_OP_CZ      q0, q1   -
 *           MLQEM_SIM_OP_SWAP    q0, q1   -
 *           MLQEM_SIM_OP_U2      q0, q1   32: a 4x4 complex matrix, row-major, basis index = bit(q0) + 2 bit(q1)   (ecr, rzz, ...)
 *           MLQEM_SIM_OP_DEPOL1  q0       1: lambda.  rho -> (1 - lambda) rho + lambda Tr_q0(rho) (x) I/2, in closed form: entries
 *                                         whose row and column bit of q0 differ scale by 1 - lambda, the others become
 *                                         (1 - lambda) rho_ii + lambda/2 (rho_00 + rho_11).  Mode 1 only (ignored in mode 0).
 *           MLQEM_SIM_OP_DEPOL2  q0, q1   1: lambda.  The same over both qubits, I/4 and lambda/4 times the sum of the four diagonal
 *                                         entries of a 4x4 block.  Mode 1 only.
 *           MLQEM_SIM_OP_READOUT q0       2: p01 = P(read 0 | prepared 1), p10 = P(read 1 | prepared 0).  The column-stochastic matrix
 *                                         [[1 - p10, p01], [p10, 1 - p01]] on bit q0 of the DIAGONAL of rho; off-diagonal entries
 *                                         are meaningless afterwards, so only I/Z terms may follow.  Mode 1 only.
 *           MLQEM_SIM_OP_NOISE1  q0       4: lambda, g, c, p1.  One fused noise record: MLQEM_SIM_OP_DEPOL1's map with lambda, then
 *                                         thermal relaxation of q0 on the same 2x2 block (e_rc: row bit r, column bit c of q0), with
 *                                         tr = e00 + e11:  e00' = (1 - g) e00 + g (1 - p1) tr,  e11' = (1 - g) e11 + g p1 tr,
 *                                         e01' = c e01,  e10' = c e10.  g = 1 - exp(-t/T1) is the reset probability, c = exp(-t/T2)
 *                                         the factor of the coherences, p1 the excited-state population.  One pass.  lambda = 0
 *                                         leaves the first part an exact identity, g = 0 and c = 1 the second.  Mode 1 only.
 *           MLQEM_SIM_OP_NOISE2  q0, q1   7: lambda, (g, c, p1) of q0, (g, c, p1) of q1.  MLQEM_SIM_OP_DEPOL2's map with lambda, then
 *                                         the relaxation map above on q0 and on q1, in one pass over the 4x4 blocks.  Mode 1 only.
 *         The host keeps 0 <= g, p1 <= 1 and 0 <= c <= sqrt(1 - g) (complete positivity); the kernel uses the values as they are.
 *         An unknown kind is skipped.
 * params  float64 [n_params], n_params >= 32, with 32 values of padding after the last record's (a record's read is clamped to
 *         [0, n_params - 32]).
 * term_ptr int64 [n_circuits + 1]; terms mlqem_sim_term [n_terms], 16-byte aligned: (xmask, zmask, ny, 0) of a Pauli string (bit q of
 *         xmask: X or Y on qubit q; of zmask: Z or Y; ny = the number of Y); coeff float64 [n_terms], the real coefficients.
 *         With P|j> = i^ny (-1)^popcount(j & zmask) |j ^ xmask>:
 *           mode 0   <P> = Re sum_j i^ny (-1)^popcount(j & zmask) conj(psi[j ^ xmask]) psi[j]
 *           mode 1   <P> = Re sum_j i^ny (-1)^popcount(j & zmask) rho[j, j ^ xmask]
 * ids     int32 [n_wave + n_wg]: the circuits this call simulates.  The first n_wave have at most MLQEM_SIM_WAVE_AMPS = 256
 *         amplitudes and run a wave per circuit (four circuits per 256-thread workgroup, each wave on its own 4 KB of LDS, no
 *         workgroup barrier); the other n_wg have 512 .. 2 048 and run a workgroup per circuit (a barrier between passes).  At most
 *         two launches.  A circuit whose amplitude count exceeds its variant's is simulated with n clamped to what fits.
 * Outputs, float64: term_values [n_terms]; values [n_circuits] = sum coeff * term value, added in term order by one thread (0.0 for
 *         a circuit without terms); norm [n_circuits] = <psi|psi> or Tr rho before the readout ops.  Only the entries of the
 *         circuits in `ids` are written.
 * Every sum is formed in a fixed order (lane-strided partial sums, a shuffle tree over the 64 lanes, then wave 0 .. 3): no atomics,
 * and a circuit's results are the same bits alone or in any batch, from call to call.  Every index read from a record is clamped
 * (qubits to n, offsets to their arrays, masks to n bits, amplitude indices to the state), so a malformed record computes
 * garbage and faults nothing.  No workspace, no host read: capturable in a hipGraph.
 * Negative sizes, n_wave + n_wg > n_circuits, n_params < 32, null or misaligned buffers: MLQEM_ERR_BAD_ARG; n_circuits or n_params
 * over 2^31 - 1: MLQEM_ERR_UNSUPPORTED; all checked before anything is launched.  n_wave + n_wg == 0 returns MLQEM_OK without a
 * launch.
 * ---------------------------------------------------------------------------------------------------- */
#define MLQEM_SIM_WAVE_AMPS 256
#define MLQEM_SIM_MAX_AMPS 2048
#define MLQEM_SIM_OP_U1 0
#define MLQEM_SIM_OP_DIAG1 1
#define MLQEM_SIM_OP_CX 2
#define MLQEM_SIM_OP_CZ 3
#define MLQEM_SIM_OP_SWAP 4
#define MLQEM_SIM_OP_U2 5
#define MLQEM_SIM_OP_DEPOL1 6
#define MLQEM_SIM_OP_DEPOL2 7
#define MLQEM_SIM_OP_READOUT 8
/* 9 is MLQEM_SIM_OP_MEASURE (below).  The two fused noise kinds were added without a change of any signature: a program lowered
 * before them never contains them, and its results are the same bits. */
#define MLQEM_SIM_OP_NOISE1 10
#define MLQEM_SIM_OP_NOISE2 11
typedef struct mlqem_sim_op { int32_t kind; int32_t q0; int32_t q1; int32_t param; } mlqem_sim_op;
typedef struct mlqem_sim_term { int32_t xmask; int32_t zmask; int32_t ny; int32_t reserved; } mlqem_sim_term;
int mlqem_sim_run_f64(int64_t n_circuits, const int32_t* circ, const int64_t* op_ptr, const mlqem_sim_op* ops, int64_t n_ops,
                      const double* params, int64_t n_params, const int64_t* term_ptr, const mlqem_sim_term* terms,
                      const double* coeff, int64_t n_terms, const int32_t* ids, int64_t n_wave, int64_t n_wg, double* term_values,
                      double* values, double* norm, mlqem_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Zero-noise extrapolation on the simulator (two additive symbols, the ABI version is unchanged).  A folded circuit is the same
 * records replayed in another order, some as their inverse, so the circuits are lowered ONCE (the buffers of mlqem_sim_run_f64 for
 * n_circuits = B circuits) and every (circuit, noise factor) pair gets a SCHEDULE of 4 bytes per step.  blackwater.sim.zne builds
 * the schedules (build_schedules) and blackwater.native.ops.sim_run_folded / zne_combine call these.
 *
 * mlqem_sim_run_folded_f64.  Run r = f * B + c is circuit c at noise factor f, 0 <= f < n_factors = F.
 * sched_ptr int64 [F * B + 1]; sched int32 [n_sched]: run r owns sched[sched_ptr[r] .. sched_ptr[r + 1]).  An entry is
 *         (k << 1) | dagger with k an op index RELATIVE to op_ptr[c].  The run starts from |0..0> and applies
 *         ops[op_ptr[c] + k] for each entry in order; the LAST circ[c].r entries of a schedule are its readout ops, and norm is
 *         taken before them; then the terms of circuit c are evaluated exactly as in mlqem_sim_run_f64.
 *         dagger = 1 applies the record's inverse, formed from the ONE record by swapping and negating components only (no new
 *         rounding: a run is bit-equal to mlqem_sim_run_f64 on a program whose records were expanded and conjugate-transposed
 *         on the host):
 *           U1, U2           the conjugate transpose of the record's matrix; in mode 1 the column bits get its conjugate, i.e. the
 *                            transpose
 *           DIAG1            conjugated phases
 *           CX, CZ, SWAP     unchanged (self-inverse)
 *           DEPOL*, NOISE*, READOUT  the flag is ignored (a noise record is never inverted)
 * ids     int32 [n_wave + n_wg]: RUN numbers; the wave / workgroup split is by the circuit's amplitude count, as above.
 * Outputs, float64: term_values [F][n_terms], values [F][B], norm [F][B]; only the entries of the runs in `ids` are written.
 * The contract of mlqem_sim_run_f64 holds for the new input too: k is clamped to the circuit's op range (a circuit without ops
 * skips its entries), schedule offsets are clamped to n_sched, run numbers to F * B; an empty schedule leaves |0..0>; a malformed
 * schedule computes garbage and faults nothing.  No atomics, no workspace, no host read: capturable in a hipGraph; a run's bits are
 * the same alone, in any batch and from call to call.  The wave variant has no workgroup barrier, so the four runs of a workgroup
 * may have schedules of any lengths.
 * Negative sizes, n_factors < 1, n_wave + n_wg > F * B, n_params < 32, null or misaligned buffers: MLQEM_ERR_BAD_ARG; n_circuits,
 * n_factors, F * B, n_params or n_sched over 2^31 - 1: MLQEM_ERR_UNSUPPORTED; all checked before anything is launched.
 *
 * mlqem_zne_combine_f64.  Polynomial extrapolation of exact values to zero noise is a weighted sum over the factors (the weights
 * come from the host: blackwater.sim.zne, Extrapolator.weights).  term_values [F][n_terms], weights [F], term_ptr [B + 1], coeff
 * [n_terms] ->  mitigated_terms [n_terms] = sum_f weights[f] * term_values[f][t], added in factor order (w0 * tv0, then one fused
 * multiply-add per further factor);  mitigated_values [B] = sum_t coeff[t] * mitigated term t, added in term order by one thread
 * per circuit (a fused multiply-add per term, from 0.0).  One launch, fixed order, no atomics, no workspace, no host read:
 * capturable.  term_ptr is clamped to n_terms.  n_factors < 1, negative sizes or a null buffer that would be used:
 * MLQEM_ERR_BAD_ARG; a size over 2^31 - 1: MLQEM_ERR_UNSUPPORTED.  n_circuits == 0 and n_terms == 0: MLQEM_OK without a launch.
 * ---------------------------------------------------------------------------------------------------- */
int mlqem_sim_run_folded_f64(int64_t n_circuits, int64_t n_factors, const int32_t* circ, const int64_t* op_ptr, const mlqem_sim_op* ops,
                             int64_t n_ops, const double* params, int64_t n_params, const int64_t* term_ptr,
                             const mlqem_sim_term* terms, const double* coeff, int64_t n_terms, const int64_t* sched_ptr,
                             const int32_t* sched, int64_t n_sched, const int32_t* ids, int64_t n_wave, int64_t n_wg,
                             double* term_values, double* values, double* norm, mlqem_stream_t stream);
int mlqem_zne_combine_f64(int64_t n_factors, int64_t n_circuits, const double* term_values, const double* weights,
                          const int64_t* term_ptr, const double* coeff, int64_t n_terms, double* mitigated_terms,
                          double* mitigated_values, mlqem_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Measurement shots on the simulator (three additive symbols, the ABI version is unchanged).  After a circuit is simulated the
 * device draws `shots` outcomes per measurement basis and returns the counts, the sampled Pauli-term estimates, the sampled
 * observable values and their variances.  blackwater.sim lowers for it (compile_programs(..., shots=)) and
 * blackwater.native.ops.sim_run_measured / sim_run_folded_measured / sim_sample call these.
 *
 * Groups.  The Pauli terms of a circuit are partitioned on the host into GROUPS of qubit-wise commuting terms, one measurement
 * basis (Z, X or Y per qubit) each; circuit c owns groups group_ptr[c] .. group_ptr[c + 1] of n_groups, group g owns the 2^n
 * entries prob_ptr[g] .. prob_ptr[g] + 2^n of a pool of n_outcomes (probs float64, counts int32; outcome j = the measured bit
 * string as an integer, qubit 0 the least significant bit), and term_group int32 [n_terms] is a term's group COUNTED INSIDE ITS
 * CIRCUIT.  group_ptr int64 [n_circuits + 1], prob_ptr int64 [n_groups + 1], group_circ int32 [n_groups] (the circuit of a group).
 *
 * Trailing ops.  circ[c] = (n_qubits, mode, r, m): the LAST r + m ops of a program (or entries of a schedule) are its r readout
 * ops followed by a measurement tail of m records, and norm is taken before all of them.  The tail holds, per group: the basis
 * rotations as ordinary noise-free MLQEM_SIM_OP_U1 records (H for X, H S^dagger for Y), one MLQEM_SIM_OP_MEASURE record, and the
 * inverse rotations, so that the next group and the exact term values see the circuit's own state.  m is read by the measured
 * entry points alone: mlqem_sim_run_f64 / mlqem_sim_run_folded_f64 ignore it and skip a MEASURE record as an unknown kind.
 *
 * MLQEM_SIM_OP_MEASURE (q0 = the group inside its circuit, q1 = 0, param = the group's number g in prob_ptr; it owns no float64).
 * One pass that reads the state and leaves it unmodified: probs[prob_ptr[g] + j] = |psi_j|^2 (mode 0) or Re rho_jj (mode 1) for
 * j < 2^n; a folded run writes row f of probs [F][n_outcomes].  Stores are predicated: a g outside the circuit's own groups, or a
 * prob_ptr[g] with prob_ptr[g] < 0 or prob_ptr[g] + 2^n > n_outcomes, stores nothing (the index into prob_ptr is clamped).
 *
 * mlqem_sim_run_measured_f64 / mlqem_sim_run_folded_measured_f64: mlqem_sim_run_f64 / mlqem_sim_run_folded_f64 with the trailing-op
 * rule above, the three group arguments and the output probs.  Everything else, checks and return codes included, is theirs;
 * n_groups over 2^31 - 1: MLQEM_ERR_UNSUPPORTED; a null group_ptr, prob_ptr or (n_outcomes > 0) probs: MLQEM_ERR_BAD_ARG.
 *
 * mlqem_sim_sample_f64 samples EVERY (noise factor f, group g) pair of F x n_groups (F = n_factors = 1 for plain runs); run
 * r = f * B + c.  units int32 [n_wave + n_wg] lists the pairs as f * n_groups + g, n_wave + n_wg = F * n_groups: the first n_wave
 * have at most 256 outcomes and take a wave each (four per workgroup, no workgroup barrier), the others a workgroup each; the
 * pair's CDF and counts live in LDS.  The split is the caller's to respect (blackwater.sim.SimBatch.sample_units makes it): n is
 * clamped to the variant's cap (8 or 11 qubits), so a pair of more than 256 outcomes listed among the first n_wave samples the first
 * 256 entries of its range only -- memory-safe garbage, MLQEM_OK, like every malformed input of this file.  Per pair, with M = 2^n outcomes and p = probs[f][prob_ptr[g] ..]:
 *   1. p_j <- p_j if p_j > 0, else 0 (a NaN counts as 0).
 *   2. The CDF, in an order that depends on M alone.  L = min(M, 8), C = M / L chunks of L consecutive outcomes.  Inside chunk k:
 *      run_k[0] = p[k L], run_k[i] = run_k[i - 1] + p[k L + i].  tot[k] = run_k[L - 1].  before[0] = 0, before[k] = before[k - 1] +
 *      tot[k - 1].  cdf[k L + i] = before[k] + run_k[i].  (float64 additions, exactly these, in this order; the CDF is
 *      non-decreasing.)
 *   3. Shot s < shots: Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) and counter (s >> 1, the group inside its circuit,
 *      run_key & 0xffffffff, run_key >> 32) gives x0 .. x3; an even s takes (a, b) = (x0, x1), an odd s (x2, x3);
 *      u = ((a >> 5) 2^26 + (b >> 6)) 2^-53.  run_key = run_keys[r], int64 [F * B] from the host (by default r itself; a caller
 *      passes its own so that a circuit draws the same shots alone and in a batch).
 *   4. target = u * cdf[M - 1] (one rounded product);  j = min(#{i : cdf[i] <= target}, j_last),  j_last = #{i : cdf[i] < cdf[M - 1]}
 *      (the second term keeps an outcome of probability 0 unreachable even when the product rounds up to the total).  Both
 *      counts are binary searches in LDS.  counts[j] += 1: integer LDS atomics, order-independent.
 *   5. counts[f][prob_ptr[g] + j] = the int32 counts (row f of [F][n_outcomes]; nothing is stored when the range leaves the pool,
 *      and the loads of p are clamped to it).
 *   6. For every term t of circuit c with term_group[t] == the group: S_t = sum_j counts_j (-1)^popcount(j & (xmask | zmask)), an
 *      integer; term_values[f][t] = (double)S_t / (double)shots (one IEEE division: numpy gives the same bits).  The all-identity
 *      term gives +1.
 * Then one thread per run, terms in order, from 0.0: values[f][c] = fma(coeff_t, term_t, values), variance[f][c] = fma(coeff_t^2,
 * fma(-term_t, term_t, 1), variance) -- sum coeff^2 (1 - term^2), the per-term variance an estimator reports; covariances between
 * the terms of a group are not included.  At most three launches on the stream; no float atomics, no workspace, no host read:
 * capturable.  Counts and estimates are the same bits alone, in any batch and from call to call for equal (seed, run key, group,
 * probabilities).  Everything read from a buffer is clamped (unit numbers, circuits, n to the variant's cap, term ranges).
 * shots outside 1 .. MLQEM_SIM_MAX_SHOTS = 2^20, negative sizes, n_factors < 1, n_wave + n_wg != F * n_groups, n_groups or
 * n_outcomes < 1 with n_circuits > 0, a null or misaligned buffer: MLQEM_ERR_BAD_ARG; n_circuits, n_factors, n_groups, F * B or
 * F * n_groups over 2^31 - 1: MLQEM_ERR_UNSUPPORTED; n_circuits == 0: MLQEM_OK without a launch.
 * ---------------------------------------------------------------------------------------------------- */
#define MLQEM_SIM_OP_MEASURE 9
#define MLQEM_SIM_MAX_SHOTS 1048576
int mlqem_sim_run_measured_f64(int64_t n_circuits, const int32_t* circ, const int64_t* op_ptr, const mlqem_sim_op* ops, int64_t n_ops,
                               const double* params, int64_t n_params, const int64_t* term_ptr, const mlqem_sim_term* terms,
                               const double* coeff, int64_t n_terms, const int64_t* group_ptr, const int64_t* prob_ptr,
                               int64_t n_groups, int64_t n_outcomes, const int32_t* ids, int64_t n_wave, int64_t n_wg,
                               double* term_values, double* values, double* norm, double* probs, mlqem_stream_t stream);
int mlqem_sim_run_folded_measured_f64(int64_t n_circuits, int64_t n_factors, const int32_t* circ, const int64_t* op_ptr,
                                      const mlqem_sim_op* ops, int64_t n_ops, const double* params, int64_t n_params,
                                      const int64_t* term_ptr, const mlqem_sim_term* terms, const double* coeff, int64_t n_terms,
                                      const int64_t* group_ptr, const int64_t* prob_ptr, int64_t n_groups, int64_t n_outcomes,
                                      const int64_t* sched_ptr, const int32_t* sched, int64_t n_sched, const int32_t* ids,
                                      int64_t n_wave, int64_t n_wg, double* term_values, double* values, double* norm, double* probs,
                                      mlqem_stream_t stream);
int mlqem_sim_sample_f64(int64_t n_circuits, int64_t n_factors, const int32_t* circ, const int64_t* term_ptr,
                         const mlqem_sim_term* terms, const double* coeff, int64_t n_terms, const int64_t* group_ptr,
                         const int32_t* term_group, const int64_t* prob_ptr, const int32_t* group_circ, int64_t n_groups,
                         int64_t n_outcomes, const double* probs, const int64_t* run_keys, int64_t shots, uint64_t seed,
                         const int32_t* units, int64_t n_wave, int64_t n_wg, int32_t* counts, double* term_values, double* values,
                         double* variance, mlqem_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Quantum trajectories on the simulator (an additive symbol, the ABI version is unchanged).  A noisy circuit of 6 .. 11 qubits has
 * no density matrix that fits the 2 048-amplitude state, but its state VECTOR fits.  mlqem_sim_run_trajectories_f64 runs every
 * circuit as T = `trajectories` pure-state trajectories: at every noise record it draws ONE Kraus operator and applies it, and the
 * averages over the trajectories estimate the values under the noise model.  blackwater.sim lowers for it
 * (compile_programs(..., trajectories=)) and blackwater.native.ops.sim_run_trajectories calls it.
 *
 * Input.  The buffers of mlqem_sim_run_f64, with the records density mode (mode 1) emits, and circ[c] = (n_qubits, 2, r, 0): mode 2,
 * TRAJECTORY mode, n <= 11, the state a 2^n vector.  The kernels here do not read the mode field (the other entry points read
 * mode != 0 as a density matrix, so the host refuses to hand them such a batch).  ids int32 [n_wave + n_wg] with
 * n_wave + n_wg == n_circuits: every circuit is run; the first n_wave have at most 256 amplitudes.  run_keys int64 [n_circuits];
 * seed uint64; 1 <= trajectories <= MLQEM_SIM_MAX_TRAJECTORIES = 2^20.
 *
 * Work unit: one (circuit, trajectory) pair; a wave per unit (four per workgroup, no workgroup barrier) where 2^n <= 256, else a
 * workgroup per unit; the wave units of the batch come first (one launch each).  Unit u of a launch is trajectory u % T of the
 * launch's circuit ids[u / T].  The rules of mlqem_sim_run_f64 hold: loads unconditional on clamped and masked indices, stores
 * predicated, trip counts that depend on the amplitude count alone, a malformed record computes garbage and faults nothing.
 *
 * Records.  Record k of circuit c (k counted from op_ptr[c]), k < n_ops(c) - r:
 *   U1, DIAG1, CX, CZ, SWAP, U2   as in mode 0 (a coherent error is an ordinary U2 record).
 *   DEPOL1 (lambda) on q0.  lambda == 0: nothing.  Else one uniform u = U(k, 0).  w = lambda / 4; s_0 = 1 - 3 w; s_j = s_(j-1) + w.
 *           The outcome is the first j in 0 .. 3 with s_j > u, else 3.  j = 0: identity, NO pass.  j = 1, 2, 3: the Pauli X, Y, Z
 *           on q0, one pass.
 *   DEPOL2 (lambda) on (q0, q1).  The same with w = lambda / 16, s_0 = 1 - 15 w, j in 0 .. 15.  The pair's code: j = l0 + 4 l1 with
 *           the letter l0 on q0 and l1 on q1, letters 0 = I, 1 = X, 2 = Y, 3 = Z (j = 0 is the identity; j = 1 is X on q0; j = 4 is
 *           X on q1; j = 15 is Z Z).
 *           A Pauli string acts as P|i> = i^ny (-1)^popcount(i & z) |i ^ x> (x: the X and Y letters, z: the Z and Y letters, ny: the
 *           number of Y): components are swapped and negated, nothing is rounded.  The probabilities do not depend on the state,
 *           so no norm is computed.
 *   Relaxation (g, c, p1) of ONE qubit q with sub-draw s.  One pass forms P0 and P1, the sums of |psi_i|^2 over the i with bit q
 *           clear and set (lane-strided partial sums over the pairs (i, i | 1 << q) in pair order, the shuffle tree, the waves in
 *           order: the reduction order of every sum here).  pa = P0 / (P0 + P1), pb = P1 / (P0 + P1).  c2 = c c,
 *           d = max(0, (1 - g) - c2).  Six outcomes, in this order, with their probabilities:
 *             0  K0  = diag(1, c)          (1 - p1) (pa + c2 pb)
 *             1  K1  = sqrt(g) |0><1|      (1 - p1) (g pb)
 *             2  K2  = sqrt(d) |1><1|      (1 - p1) (d pb)
 *             3  K0' = diag(c, 1)          p1 (c2 pa + pb)
 *             4  K1' = sqrt(g) |1><0|      p1 (g pa)
 *             5  K2' = sqrt(d) |0><0|      p1 (d pa)
 *           One uniform u = U(k, s); s_j = s_(j-1) + probability_j from s_(-1) = 0; the outcome is the first j with s_j > u, and
 *           if rounding leaves none, the last j whose probability is > 0.  An outcome of probability exactly 0 is never chosen.
 *           The state is multiplied by the operator over the square root of ITS OWN probability given the state (the weight
 *           1 - p1 or p1 left out), a real 2x2 matrix on bit q, one pair pass: with t = 1 / sqrt(.),
 *             0: diag(t, c t), t from pa + c2 pb      1: t |0><1|, t from pb      2: t |1><1|, t from pb
 *             3: diag(c t, t), t from c2 pa + pb      4: t |1><0|, t from pa      5: t |0><0|, t from pa
 *           (g and d cancel in the jumps).  <psi|psi> keeps its value up to rounding.  Averaged over u this is the map of
 *           MLQEM_SIM_OP_NOISE1's relaxation part: populations (1 - g) rho + g tr (1 - p1, p1), coherences times c; completely
 *           positive exactly where the host demands c <= sqrt(1 - g).
 *   NOISE1 (lambda, g, c, p1) on q0.  DEPOL1's draw with sub-draw 0 (skipped at lambda == 0), then relaxation of q0, sub-draw 1.
 *   NOISE2 (lambda, (g, c, p1) of q0, (g, c, p1) of q1).  DEPOL2's draw (sub-draw 0, skipped at lambda == 0), relaxation of q0
 *           (sub-draw 1), relaxation of q1 (sub-draw 2); each step takes its populations from the state the step before left.
 *   The LAST r records (READOUT: p01, p10 on q0) are not applied to the state.  They fill a table r[q] = (1 - 2 p10, -(1 - 2 p01)),
 *           default (+1, -1).  Where r > 0, a term with xmask == 0 is  sum_i |psi_i|^2 prod_(q in zmask, ascending) r[q][bit q of i],
 *           the exact expectation under the readout channel (no sampling); every other term, and every term where r == 0, is
 *           mode 0's formula.  (The host refuses readout noise beside a term with X or Y.)
 *
 * Randomness.  U(k, s) of trajectory t: Philox4x32-10 with the key (seed & 0xffffffff, seed >> 32) and the counter
 *   (k,  s << 24 | t,  run_key & 0xffffffff,  run_key >> 32),   run_key = run_keys[c], t < 2^20, s in {0, 1, 2};
 * of its words x0 .. x3, u = ((x0 >> 5) 2^26 + (x1 >> 6)) 2^-53, as in mlqem_sim_sample_f64.  Every lane computes the same u, so
 * every branch on a draw is uniform over the unit.  A trajectory therefore depends on (seed, run key, t, the circuit's records)
 * alone: not on the batch, not on the unit's slot, not on T (the first T trajectories of a longer run are the same bits).
 *
 * Outputs, float64.  Per unit: traj_term_values [T][n_terms] (row t: the term values of trajectory t, mode 0's reduction) and
 * traj_norm [T][n_circuits], <psi|psi> after the last record.  Then one finish launch, sums in trajectory order t = 0 .. T - 1 from
 * 0.0: term_values [n_terms] = the mean (sum / T); term_std_error [n_terms] = sqrt(M2 / (T (T - 1))) with M2 = sum (x_t - mean)^2
 * (a second pass, a fused multiply-add per trajectory), 0 at T == 1; values [n_circuits] and std_error [n_circuits] the same over
 * the per-trajectory value v_t = sum coeff * term in term order (a fused multiply-add per term, from 0.0); norm [n_circuits] = the
 * mean of traj_norm.  Values are NOT divided by the norm.  At most three launches; no atomics, no host read: capturable.
 * Negative sizes, trajectories outside 1 .. 2^20, n_wave + n_wg != n_circuits, n_params < 32, a null or misaligned buffer:
 * MLQEM_ERR_BAD_ARG; n_circuits, n_params, n_terms or n_circuits * trajectories over 2^31 - 1: MLQEM_ERR_UNSUPPORTED; all checked
 * before anything is launched.  n_circuits == 0: MLQEM_OK without a launch.
 * ---------------------------------------------------------------------------------------------------- */
#define MLQEM_SIM_MAX_TRAJECTORIES 1048576
int mlqem_sim_run_trajectories_f64(int64_t n_circuits, const int32_t* circ, const int64_t* op_ptr, const mlqem_sim_op* ops,
                                   int64_t n_ops, const double* params, int64_t n_params, const int64_t* term_ptr,
                                   const mlqem_sim_term* terms, const double* coeff, int64_t n_terms, const int32_t* ids,
                                   int64_t n_wave, int64_t n_wg, const int64_t* run_keys, int64_t trajectories, uint64_t seed,
                                   double* traj_term_values, double* traj_norm, double* term_values, double* term_std_error,
                                   double* values, double* std_error, double* norm, mlqem_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Parameter binding on the device (two additive symbols, the ABI version is unchanged).  One ansatz evaluated at many parameter
 * vectors is ONE program and a table of float64: the circuit is lowered once as a TEMPLATE whose free angles stay in the records,
 * and a RUN is (template, row of theta, shifted record).  blackwater.sim.compile_templates lowers templates to this format and
 * blackwater.native.ops.sim_run_bound / sim_shift_combine call these; blackwater.sim.parameter_shift builds gradients on them.
 *
 * mlqem_sim_run_bound_f64.
 * Input.  The buffers of mlqem_sim_run_f64 for n_templates templates, in which five more record kinds may appear.  The 16-byte
 * record is unchanged and the kinds above keep their numbers, so a program without the new kinds is a program of mlqem_sim_run_f64.
 *           kind                 qubits   params
 *           MLQEM_SIM_OP_PRX     q0       3: parameter index (an exactly representable integer), scale, offset
 *           MLQEM_SIM_OP_PRY     q0       3: the same
 *           MLQEM_SIM_OP_PRZ     q0       3: the same
 *           MLQEM_SIM_OP_PP      q0       3: the same
 *           MLQEM_SIM_OP_PRZZ    q0, q1   3: the same
 *         No ordinal is stored: q1 of the one-qubit kinds is 0 and the pool holds the three values alone (the trig table below is
 *         indexed by the record's position in its circuit, which the kernel knows).
 * theta   float64 [n_rows][ld_theta], ld_theta >= 1: the parameter rows.
 * runs    int32 [n_runs][4], 16-byte aligned: (template c, theta row, shifted op or -1, 0).
 * shift   float64 [n_runs].
 * ids     int32 [n_wave + n_wg]: RUN numbers, the runs of templates with at most 256 amplitudes first (a wave each), then the others
 *         (a workgroup each), as in mlqem_sim_run_f64.
 * run_term_ptr int64 [n_runs + 1]: run r owns term_values[run_term_ptr[r] .. run_term_ptr[r + 1]), the terms of its template in
 *         order.  n_out_terms = the length of term_values.
 * form    MLQEM_SIM_BOUND_TABLE or MLQEM_SIM_BOUND_PLAIN: where the sin/cos of a parameterised record is computed (below).  Both
 *         forms return the same bits.
 * Run r simulates the records of template c = runs[r][0] with the row theta[runs[r][1]].  A parameterised record reads
 *           phi = scale * theta[row][index] + offset,   and   phi = phi + shift[r]
 *         if the record's index inside its circuit (0 for the circuit's first record) equals runs[r][2].  Every step is one
 *         rounded float64 operation (a product, a sum, a sum: no fused multiply-add), so a host interpreter forms the same phi bit
 *         for bit.  The gates, with (c, s) = (cos a, sin a) of a = 0.5 * phi (an exact product) for the first four kinds:
 *           PRX   [[c, -i s], [-i s, c]]                        PRY   [[c, -s], [s, c]]
 *           PRZ   diag(c - i s, c + i s)                        PRZZ  c - i s where bits q0 and q1 of the index agree, c + i s else
 *           PP    diag(1, cos phi + i sin phi)
 *         cos and sin are the device library's double-precision functions.  In mode 1 the gate acts as U on bits q and conj(U) on
 *         bits q + n, as every unitary does; PRX and PRY are two pair passes there, the diagonal kinds one element pass in either
 *         mode.
 * Everything else is the contract of mlqem_sim_run_f64: the state stays in LDS from |0..0>; modes 0 and 1; a wave per run up to 256
 * amplitudes without a workgroup barrier, a workgroup per run for 512 .. 2 048; loads unconditional on clamped and masked indices,
 * stores predicated; fixed-order sums, no atomics, no workspace, no host read: capturable in a hipGraph; at most two launches.  The
 * fixed kinds take the passes mlqem_sim_run_f64 takes, so a template without parameterised records gives its bits.  A run's bits
 * depend on (records, theta row, shifted op, shift) alone, not on the other runs of the call.
 * Clamps: a run number to [0, n_runs - 1]; the template to [0, n_templates - 1]; the row to [0, n_rows - 1]; the parameter index
 * (converted towards zero) to [0, ld_theta - 1]; a shifted op outside [0, the circuit's record count) means "none"; run_term_ptr to
 * [0, n_out_terms], and a term beyond the run's slice is computed and not stored; and what mlqem_sim_run_f64 clamps.
 * The trig.  MLQEM_SIM_BOUND_TABLE: a table of (cos, sin) pairs in LDS for the current WINDOW of T consecutive records (T = 64 in the
 * wave variant, 256 in the workgroup variant).  When the op loop enters a window, lane l forms the pair of record l of the window if
 * that record is parameterised (a wave without one skips the trig), and the loop reads the pair when it reaches the record.
 * MLQEM_SIM_BOUND_PLAIN: every lane computes the pair inside the op loop.
 * Outputs, float64: term_values [n_out_terms]; values [n_runs] = sum coeff * term value in term order; norm [n_runs].  Only the
 * entries of the runs in `ids` are written.
 * The checks of mlqem_sim_run_f64 (with n_wave + n_wg > n_runs), and: a negative n_rows, ld_theta, n_runs or n_out_terms, an unknown
 * form, with runs to do n_templates, n_rows or ld_theta < 1 or a null or misaligned theta, runs, shift or run_term_ptr:
 * MLQEM_ERR_BAD_ARG; n_templates, n_params, n_runs, n_rows or ld_theta over 2^31 - 1: MLQEM_ERR_UNSUPPORTED; all before any launch.
 * n_wave + n_wg == 0 returns MLQEM_OK without a launch.
 *
 * mlqem_sim_shift_combine_f64.  The parameter-shift rule: every parameterised gate is exp(-i a G) with G^2 = 1 up to a phase
 * (a = phi / 2; PP is PRZ times a phase), so d<O>/d phi = (<O>(phi + pi/2) - <O>(phi - pi/2)) / 2 exactly, under any noise that
 * does not depend on the angle.  With K shifted records per template (its OCCURRENCES, in circuit order), v_plus / v_minus float64
 * [n_shifts = K][n_rows] the values of the runs shifted by +pi/2 / -pi/2 at occurrence k, scale float64 [K] the occurrence's scale,
 * occ_ptr int64 [n_parameters + 1] and occ int32 [n_occ] the occurrences of every parameter (in circuit order; an entry is clamped to
 * [0, K - 1]):
 *           grad[b][p] = sum over j in [occ_ptr[p], occ_ptr[p + 1]) of (0.5 * scale[k]) * (v_plus[k][b] - v_minus[k][b]),  k = occ[j]
 * by thread (b, p), from 0.0 in the order of j; 0.5 * scale is exact, the difference, the product and the sum are each one rounded
 * float64 operation (no fused multiply-add).  grad float64 [n_rows][n_parameters].  One launch, no atomics, no workspace, no host
 * read: the same bits from call to call, capturable.  Negative sizes, a null buffer that would be used, occurrences without shifts:
 * MLQEM_ERR_BAD_ARG; a size over 2^31 - 1: MLQEM_ERR_UNSUPPORTED.  n_rows == 0 or n_parameters == 0: MLQEM_OK without a launch.
 * ---------------------------------------------------------------------------------------------------- */
#define MLQEM_SIM_OP_PRX 12
#define MLQEM_SIM_OP_PRY 13
#define MLQEM_SIM_OP_PRZ 14
#define MLQEM_SIM_OP_PP 15
#define MLQEM_SIM_OP_PRZZ 16
#define MLQEM_SIM_BOUND_TABLE 0
#define MLQEM_SIM_BOUND_PLAIN 1
int mlqem_sim_run_bound_f64(int64_t n_templates, const int32_t* circ, const int64_t* op_ptr, const mlqem_sim_op* ops, int64_t n_ops,
                            const double* params, int64_t n_params, const int64_t* term_ptr, const mlqem_sim_term* terms,
                            const double* coeff, int64_t n_terms, const double* theta, int64_t n_rows, int64_t ld_theta,
                            const int32_t* runs, int64_t n_runs, const double* shift, const int32_t* ids, int64_t n_wave,
                            int64_t n_wg, const int64_t* run_term_ptr, int64_t n_out_terms, int32_t form, double* term_values,
                            double* values, double* norm, mlqem_stream_t stream);
int mlqem_sim_shift_combine_f64(int64_t n_rows, int64_t n_parameters, int64_t n_shifts, const int64_t* occ_ptr, const int32_t* occ,
                                int64_t n_occ, const double* scale, const double* v_plus, const double* v_minus, double* grad,
                                mlqem_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Clifford circuits of up to MLQEM_CLIFFORD_MAX_QUBITS = 512 qubits, a batch per call (an additive symbol, the ABI version is
 * unchanged).  A Pauli observable is carried BACKWARDS through a Clifford circuit as a Pauli, so its ideal value on |0..0> and its
 * value under the project's depolarising model come from one walk over the records, in O(records) bit operations per (circuit,
 * Pauli) pair: no state vector.  blackwater.sim.clifford lowers circuits to this format (compile_clifford) and
 * blackwater.native.ops.clifford_run calls it.
 *
 * A UNIT is one (circuit, Pauli) pair.  Its Pauli is W = ceil(n / 32) x words followed by W z words in `masks` (bit q % 32 of word
 * q / 32: x set for X or Y on qubit q, z set for Z or Y), i.e. the LETTER of qubit q is l = x | z << 1: I = 0, X = 1, Z = 2, Y = 3,
 * where Y is the Hermitian Pauli Y itself (not i X Z), so the Pauli is (-1)^sign times the product of its letters and nothing else.
 *
 * n_qubits int32 [n_circuits]: clamped to 1 .. 512 (to 1 .. 128 for a unit among the first n_reg).
 * op_ptr   int64 [n_circuits + 1]: circuit c owns ops[op_ptr[c] .. op_ptr[c + 1]), in circuit order.  A unit walks them from the
 *          LAST to the FIRST.
 * ops      mlqem_clifford_op [n_ops], 16-byte aligned: (head, a, b, c) with head = kind | q0 << 4 | q1 << 14 (kind 4 bits, qubits 10
 *          bits each, clamped to n - 1).  With l0 / l1 the unit's letters at q0 / q1:
 *            MLQEM_CLIFFORD_OP_C1      a one-qubit Clifford U.  a holds U^dagger P U for P = X, Z, Y (l0 = 1, 2, 3) as three 3-bit
 *                                      fields, field l0 - 1 at bits 3 (l0 - 1) ..: new letter | s << 2.  l0 becomes the new
 *                                      letter and sign ^= s; l0 = 0 stays.
 *            MLQEM_CLIFFORD_OP_C2      a two-qubit Clifford.  With p = l0 | l1 << 2 (1 .. 15) and e = p - 1: the 4-bit field e of
 *                                      the 64-bit word a | b << 32 is the image's p (new l0 | new l1 << 2), bit e of c its sign.
 *                                      p = 0 stays.
 *            MLQEM_CLIFFORD_OP_DEPOL1  a = index into `pool` of keep = 1 - lambda: factor *= keep if l0 != 0 (the adjoint of
 *                                      rho -> (1 - lambda) rho + lambda Tr_q0(rho) (x) I/2 scales every Pauli that is not the
 *                                      identity on q0 by 1 - lambda and leaves the others).
 *            MLQEM_CLIFFORD_OP_DEPOL2  the same over q0 and q1: factor *= keep if l0 | l1 != 0.
 *          An unknown kind is skipped.  Readout noise is no record: the host applies it to the observable (Z -> a Z + b I), which
 *          is what `comb` below is for.
 * pool     float64 [n_pool], n_pool >= MLQEM_CLIFFORD_PAD = 32 (an index is clamped to [0, n_pool - 1]).
 * units    mlqem_clifford_unit [n_reg + n_lds], 16-byte aligned: (circuit, mask, ny, 0).  mask = index of the unit's first x word in
 *          `masks` (every word index is clamped to [0, n_masks - 1]); ny = the number of Y letters, carried for the host (with
 *          Hermitian letters the kernel has no use for it: a Pauli without x bits has no Y left).  The first n_reg units belong to
 *          circuits of at most MLQEM_CLIFFORD_REG_QUBITS = 128 qubits and keep their eight words in registers; the other n_lds
 *          keep up to 32 words in LDS (word w of lane t at w * 256 + t; 32 KB per 256-thread workgroup).  Units should be ordered
 *          by circuit inside each part, so that the lanes of a wave load the same records.
 * masks    uint32 [n_masks], n_masks >= 32.
 * Per unit: factor = 1, sign = 0; after the walk  ideal = 0 if any x bit is left, else (-1)^sign;  noisy = ideal * factor, factor
 * being multiplied up in walk order, one rounded product per record.  unit_ideal / unit_noisy float64 [n_reg + n_lds] receive them.
 * term_ptr int64 [n_circuits + 1]; coeff float64 [n_terms]; comb_ptr int64 [n_terms + 1]; comb_unit int32 [n_comb] (clamped);
 *          comb_weight float64 [n_comb][2]:  ideal_terms[t] = sum_j comb_weight[j][0] * unit_ideal[comb_unit[j]] and
 *          noisy_terms[t] = sum_j comb_weight[j][1] * unit_noisy[comb_unit[j]] over j in [comb_ptr[t], comb_ptr[t + 1]), from 0.0 in
 *          that order; ideal_values[c] / noisy_values[c] = sum_t coeff[t] * term, from 0.0 in term order (0.0 for a circuit without
 *          terms).  Every product and every sum is rounded on its own (no fused multiply-add).
 * No atomics, no workspace, no host read: capturable in a hipGraph, at most three launches, and a circuit's results are the same
 * bits alone or in any batch.  Every value read from a record is clamped, so a malformed record computes garbage and faults
 * nothing.  Negative sizes, n_pool or n_masks < 32, null or misaligned buffers, combine entries without units: MLQEM_ERR_BAD_ARG; a
 * count over 2^31 - 1: MLQEM_ERR_UNSUPPORTED; all checked before anything is launched.  n_circuits == 0 returns MLQEM_OK without a
 * launch.
 * ---------------------------------------------------------------------------------------------------- */
#define MLQEM_CLIFFORD_MAX_QUBITS 512
#define MLQEM_CLIFFORD_REG_QUBITS 128
#define MLQEM_CLIFFORD_PAD 32
#define MLQEM_CLIFFORD_OP_C1 0
#define MLQEM_CLIFFORD_OP_C2 1
#define MLQEM_CLIFFORD_OP_DEPOL1 2
#define MLQEM_CLIFFORD_OP_DEPOL2 3
typedef struct mlqem_clifford_op { int32_t head; int32_t a; int32_t b; int32_t c; } mlqem_clifford_op;
typedef struct mlqem_clifford_unit { int32_t circuit; int32_t mask; int32_t ny; int32_t reserved; } mlqem_clifford_unit;
int mlqem_clifford_run_f64(int64_t n_circuits, const int32_t* n_qubits, const int64_t* op_ptr, const mlqem_clifford_op* ops,
                           int64_t n_ops, const double* pool, int64_t n_pool, const mlqem_clifford_unit* units, int64_t n_reg,
                           int64_t n_lds, const uint32_t* masks, int64_t n_masks, const int64_t* term_ptr, const double* coeff,
                           int64_t n_terms, const int64_t* comb_ptr, const int32_t* comb_unit, const double* comb_weight,
                           int64_t n_comb, double* unit_ideal, double* unit_noisy, double* ideal_terms, double* noisy_terms,
                           double* ideal_values, double* noisy_values, mlqem_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Zero-noise extrapolation at width (two additive symbols, the ABI version is unchanged).  A folded Clifford circuit is a Clifford
 * circuit: the same records replayed in another order, some as their inverse, and the inverse of a conjugation table is the
 * inverse of a signed permutation.  So the circuits are lowered ONCE (the buffers of mlqem_clifford_run_f64) and every (circuit,
 * noise factor) pair gets a schedule in the format of mlqem_sim_run_folded_f64.  blackwater.sim.zne builds the schedules
 * (build_clifford_schedules) and blackwater.native.ops.clifford_run_folded / zne_combine_exp call these.
 *
 * mlqem_clifford_run_folded_f64.  Run r = f * B + c is circuit c at noise factor f, 0 <= f < n_factors = F.
 * sched_ptr int64 [F * B + 1]; sched int32 [n_sched]: run r owns sched[sched_ptr[r] .. sched_ptr[r + 1]).  An entry is
 *         (k << 1) | dagger with k a record index RELATIVE to op_ptr[c].  The circuit of run r is ops[op_ptr[c] + k] for each entry
 *         in order; a unit of circuit c walks the entries of run (f, c) from the LAST to the FIRST, exactly as
 *         mlqem_clifford_run_f64 walks the records.  There are no trailing entries: readout is no record in this format.
 *         dagger = 1 applies the record's inverse, formed from the ONE record as it is read (a run is bit-equal to
 *         mlqem_clifford_run_f64 on a batch whose records were expanded and inverted on the host):
 *           C1      with l0 != 0: j = the lowest of the three fields whose letter equals l0 (0 if none does); l0 becomes j + 1
 *                   and sign ^= the sign bit of field j
 *           C2      with p != 0: e = the lowest of the 16 nibbles of a | b << 32 that equals p, at most 14 (0 if none does); p
 *                   becomes e + 1 and sign ^= bit e of c
 *           DEPOL*  the flag is ignored
 * Every index is clamped: k to the circuit's record range (a circuit without records skips its entries), schedule offsets to
 * n_sched, the run number to F * B - 1, and what mlqem_clifford_run_f64 clamps; loads are unconditional, only the final stores
 * are predicated; a malformed schedule or table computes garbage and faults nothing.
 * Outputs, float64, row f for noise factor f: unit_ideal, unit_noisy [F][n_reg + n_lds]; ideal_terms, noisy_terms [F][n_terms];
 * ideal_values, noisy_values [F][B], combined per factor exactly as in mlqem_clifford_run_f64.  Folding is the identity without
 * noise, so the ideal rows are equal across factors for well-formed input.  At most three launches (the register walk over F *
 * n_reg runs, the LDS walk over F * n_lds, the combine over F * B); no atomics, no workspace, no host read: capturable; a circuit's
 * bits are the same alone, in any batch and from call to call.
 * The checks of mlqem_clifford_run_f64, and: n_factors < 1, n_sched < 0, a null sched_ptr, a null sched with n_sched > 0:
 * MLQEM_ERR_BAD_ARG; n_factors over 65535, n_sched, F * B or F * (n_reg + n_lds) over 2^31 - 1: MLQEM_ERR_UNSUPPORTED.
 *
 * mlqem_zne_combine_exp_f64.  Exponential extrapolation per Pauli term, with w [F] the weights of the straight-line fit (the
 * degree-1 weights of mlqem_zne_combine_f64, from the host) and v_f = term_values[f][t]:
 *   all v_f > 0 or all v_f < 0   mitigated term = sign * exp(S), S = w_0 ln|v_0|, then one fused multiply-add per further factor
 *   all v_f == 0                 0
 *   anything else                the linear sum of mlqem_zne_combine_f64 (the same operations), and fallback[t] = 1
 * fallback int32 [n_terms] is 0 in the first two cases.  mitigated_values [B] = sum_t coeff[t] * mitigated term t, a fused
 * multiply-add per term from 0.0 in term order, by one thread per circuit.  Under this noise model a Clifford Pauli's value at
 * noise factor x is ideal * F1 * F2^x, which the first case recovers as ideal * F1.  It works on the term values of either
 * folded simulator.  One launch, fixed order, no atomics, no workspace, no host read: capturable.  n_factors < 2, negative sizes
 * or a null buffer that would be used: MLQEM_ERR_BAD_ARG; a size over 2^31 - 1: MLQEM_ERR_UNSUPPORTED; n_circuits == 0 and
 * n_terms == 0: MLQEM_OK without a launch.
 * ---------------------------------------------------------------------------------------------------- */
int mlqem_clifford_run_folded_f64(int64_t n_circuits, int64_t n_factors, const int32_t* n_qubits, const int64_t* op_ptr,
                                  const mlqem_clifford_op* ops, int64_t n_ops, const double* pool, int64_t n_pool,
                                  const mlqem_clifford_unit* units, int64_t n_reg, int64_t n_lds, const uint32_t* masks,
                                  int64_t n_masks, const int64_t* term_ptr, const double* coeff, int64_t n_terms,
                                  const int64_t* comb_ptr, const int32_t* comb_unit, const double* comb_weight, int64_t n_comb,
                                  const int64_t* sched_ptr, const int32_t* sched, int64_t n_sched, double* unit_ideal,
                                  double* unit_noisy, double* ideal_terms, double* noisy_terms, double* ideal_values,
                                  double* noisy_values, mlqem_stream_t stream);
int mlqem_zne_combine_exp_f64(int64_t n_factors, int64_t n_circuits, const double* term_values, const double* weights,
                              const int64_t* term_ptr, const double* coeff, int64_t n_terms, double* mitigated_terms,
                              double* mitigated_values, int32_t* fallback, mlqem_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Measurement shots at width: Pauli-frame sampling of Clifford circuits (an additive symbol, the ABI version is unchanged).  For a
 * Clifford circuit under a Pauli noise model (depolarising records, readout flips) the outcome distribution is sampled EXACTLY from
 * one reference outcome per (circuit, measurement basis) and one Pauli frame of 2 n bits per shot: no state vector, up to 512
 * qubits.  blackwater.sim.frames lowers for it (compile_clifford_frames) and blackwater.native.ops.clifford_sample calls it.
 *
 * Input.  n_qubits, op_ptr, ops: the circuits in the record format of mlqem_clifford_run_f64 (circuit c IS run c).
 * thresh   uint64 [n_thresh], n_thresh >= 32, 8-byte aligned: the integer pool BESIDE the float64 pool of the exact path -- entry i
 *          is T = floor(lambda 2^60) of the depolarising record whose `a` is i (computed by the host with integers, exactly;
 *          lambda = 1 gives 2^60, lambda = 0 gives 0), and a circuit with readout noise owns 2 n further entries (below).  An index
 *          is clamped to [0, n_thresh - 1].
 * ro_ptr   int64 [n_circuits]: -1, or the index in thresh of the circuit's readout table: entry 2 q is floor(p10 2^32) and entry
 *          2 q + 1 is floor(p01 2^32) of qubit q (0 .. 2^32; both 0 for a qubit that is not measured or has no readout noise).
 *          The convention is that of the exact path's Z -> a Z + b I with a = 1 - p01 - p10, b = p01 - p10:
 *          p10 = P(read 1 | the bit is 0), p01 = P(read 0 | the bit is 1).
 * Units.   One sampling unit is a (run, group) pair.  The terms of a circuit are partitioned into qubit-wise commuting GROUPS
 *          (blackwater.sim.measurement_groups); circuit c owns groups group_ptr[c] .. group_ptr[c + 1] of n_groups (at least one,
 *          at most MLQEM_CLIFFORD_MAX_GROUPS = 4 096 each), group_circ int32 [n_groups] is a group's circuit.  With W = ceil(n / 32):
 *          group_mask int32 [n_groups] is the index in `masks` of the group's BASIS, W words bx then W words bz: the letter of
 *          qubit q is bit q of bx | bit q of bz << 1 (X = 1, Z = 2, Y = 3; Z where no term touches the qubit).  There are no
 *          rotation records: the basis enters through these masks alone.
 * ids      int32 [n_reg + n_lds], n_reg + n_lds == n_groups: the groups, those of circuits of at most 128 qubits first (words in
 *          registers), then the others (words in LDS at word * 256 + lane), as in mlqem_clifford_run_f64.
 * masks    uint32 [n_masks], n_masks >= 32 (every index clamped).
 * Terms.   term_ptr int64 [n_circuits + 1], coeff float64 [n_terms]; term_mask int32 [n_terms]: the index in `masks` of the term's
 *          SUPPORT, W words (bit q set: the term is not the identity on q).  gterm_ptr int64 [n_groups + 1], gterm int32 [n_gterm]:
 *          group g owns the terms gterm[gterm_ptr[g] .. gterm_ptr[g + 1]).
 * run_keys int64 [n_circuits]; seed uint64; 1 <= shots <= MLQEM_SIM_MAX_SHOTS = 2^20; max_qubits in 1 .. 512: an upper bound of
 *          every n_qubits[c] (n is clamped to it; it sizes the LDS of the reference kernel).
 * Workspace and outputs, all written by the call:
 *   rows      uint32 [n_rows]; row_ptr int64 [n_groups]: group g owns n rows of 2 W + 1 words from row_ptr[g].
 *   reference uint32 [n_ref]; ref_ptr int64 [n_groups]: the W words of the group's reference outcome m at ref_ptr[g]
 *             (ref_ptr[g] = the sum of W over the groups before g).
 *   bits      uint32, or NULL (nothing is stored): shot s of group g owns the W words at ref_ptr[g] * shots + s * W, i.e. the CSR
 *             pointer of the packed bits [shots][W] per unit is ref_ptr scaled by shots.  n_bits is its length.
 *   term_sums int32 [n_terms]: S_t;  term_values float64 [n_terms];  values, variance float64 [n_circuits].
 *
 * The rule.
 *   1. PULL-BACK.  For group g and qubit q < n: P_q = U^dagger B_q U, B_q the basis letter of q on q alone, by the backward walk
 *      of mlqem_clifford_run_f64 from sign = 0 (noise records are ignored).  Row q of the group = its W x words, W z words and
 *      the sign in one more word.
 *   2. REFERENCE OUTCOME m.  Through q = 0 .. n - 1 in order, with a set of pivot rows keyed by the position of their lowest x
 *      bit, each with a value bit v.  Start with row = P_q, acc = 0.  While the row has an x bit and a pivot exists for its lowest
 *      one: row <- row * pivot, acc ^= v.  The product XORs the x and z words, and its sign is sign ^ sign_pivot ^ ((t >> 1) & 1),
 *      t = sum over the qubits of the Aaronson-Gottesman exponent g(x1, z1, x2, z2) of (row, pivot): 0 for I; z2 - x2 for Y
 *      (x1 z1 = 11); z2 (2 x2 - 1) for X (10); x2 (1 - 2 z2) for Z (01) -- an even number, as the rows commute.  If no x bit is
 *      left the row is +-Z_T, which is +1 on |0..0>: m_q = sign ^ acc.  Otherwise m_q = 0 and the row becomes the pivot of its
 *      lowest x bit with v = acc.
 *   3. DRAWS.  Philox4x32-10 with the key (seed & 0xffffffff, seed >> 32) and the counter
 *        (run_key & 0xffffffff,  run_key >> 32,  s | gl << 20,  domain << 30 | block),   run_key = run_keys[c],
 *      s < 2^20 the shot, gl < 4 096 the group counted inside its circuit, domain 0 = initial z, 1 = noise, 2 = readout, block < 2^30.
 *      A draw depends on (seed, run key, group, shot, domain, ordinal) alone: a circuit gives the same bits alone, in any batch,
 *      for any grid and in a replayed graph.
 *   4. FRAME of shot s.  x = 0; z word w = word w & 3 of block w >> 2 of domain 0, masked to n bits.  Then the records, first to
 *      last; record i is counted from the circuit's first record:
 *        C1 / C2   the frame's letters at the record's qubits are mapped through the INVERSE of the stored table, exactly as a
 *                  daggered entry of mlqem_clifford_run_folded_f64 maps them, the sign ignored (U F U^dagger is wanted and the
 *                  record stores U^dagger P U).
 *        DEPOL1 / DEPOL2   v = word 2 (i & 1) | word 2 (i & 1) + 1 << 32 of block i >> 1 of domain 1.  The record is HIT iff
 *                  v >> 4 < T (its upper 60 bits; T = 2^60 always hits, T = 0 never).  On a hit, letter v & 3 (bit 0: x, bit 1: z)
 *                  is XORed into the frame at q0 and, for DEPOL2, letter (v >> 2) & 3 at q1: a Pauli drawn uniformly from all 4 or
 *                  16, the identity included -- the channel whose adjoint scales a Pauli that is not the identity by 1 - lambda.
 *                  (A block none of whose two records is a noise record is not computed; nothing else reads it.)
 *   5. OUTCOME.  bits word w = (m ^ (x & bz) ^ (z & bx)) masked to n bits: bit q is m_q flipped iff the frame anticommutes with
 *      B_q.  Then, in a circuit with ro_ptr >= 0, for q = 0 .. n - 1: u = word q & 3 of block q >> 2 of domain 2; bit q flips iff
 *      u < the entry of ITS OWN value (entry 2 q for a 0, 2 q + 1 for a 1), compared as 64-bit integers, so 2^32 always flips.
 *   6. ESTIMATES.  S_t = sum over the shots of (-1)^popcount(bits & support_t), an integer (wave-reduced, then integer atomics
 *      into the zeroed buffer: order-independent); term_values[t] = (double)S_t / (double)shots; values and variance as in
 *      mlqem_sim_sample_f64: one thread per circuit, terms in order from 0.0, values = fma(coeff, term, values), variance =
 *      fma(coeff^2, fma(-term, term, 1), variance).
 * Four kernels (the pull-back and the sampler, each in a register and an LDS instantiation; the reference; the finish) and one
 * memset node on the stream, at most seven nodes; no float atomics, no host read: capturable.  Every index read from a buffer is
 * clamped and only stores are predicated (a range that leaves its buffer stores nothing), so malformed input computes garbage and
 * faults nothing.  Negative sizes, shots or max_qubits out of range, n_thresh or n_masks < 32, n_reg + n_lds != n_groups, circuits
 * without a group, a null or misaligned buffer that would be used: MLQEM_ERR_BAD_ARG; a count over 2^31 - 1, n_groups *
 * ceil(shots / 256) included: MLQEM_ERR_UNSUPPORTED; all checked before anything is launched.  n_circuits == 0: MLQEM_OK without
 * a launch.
 * ---------------------------------------------------------------------------------------------------- */
#define MLQEM_CLIFFORD_MAX_GROUPS 4096
int mlqem_clifford_sample_f64(int64_t n_circuits, const int32_t* n_qubits, const int64_t* op_ptr, const mlqem_clifford_op* ops,
                              int64_t n_ops, const uint64_t* thresh, int64_t n_thresh, const int64_t* ro_ptr, const int64_t* group_ptr,
                              const int32_t* group_circ, const int32_t* group_mask, int64_t n_groups, const int32_t* ids,
                              int64_t n_reg, int64_t n_lds, const uint32_t* masks, int64_t n_masks, const int64_t* term_ptr,
                              const double* coeff, const int32_t* term_mask, int64_t n_terms, const int64_t* gterm_ptr,
                              const int32_t* gterm, int64_t n_gterm, const int64_t* run_keys, int64_t shots, uint64_t seed,
                              int32_t max_qubits, const int64_t* row_ptr, uint32_t* rows, int64_t n_rows, const int64_t* ref_ptr,
                              uint32_t* reference, int64_t n_ref, uint32_t* bits, int64_t n_bits, int32_t* term_sums,
                              double* term_values, double* values, double* variance, mlqem_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Matrix-product-state simulation (four additive symbols, the ABI version is unchanged).  A circuit whose two-qubit gates all act
 * on neighbours (q, q + 1) of a line is simulated as a matrix-product state (MPS) with bonds of at most max_bond <=
 * MLQEM_MPS_MAX_BOND = 32: any gate angle, up to MLQEM_MPS_MAX_QUBITS = 512 qubits; exact while no bond needs more than
 * max_bond, and with an a-priori certificate where it truncates.  With Pauli-insertion trajectories the same kernel gives values
 * under a depolarising + readout model.  blackwater.sim.mps lowers for it (compile_mps) and blackwater.native.ops.sim_run_mps /
 * sim_mps_finish call it.
 *
 * Input.  n_qubits int32 [B]; op_ptr int64 [B + 1]; ops mlqem_sim_op [n_ops] = (kind, site, orientation, offset into params);
 * params float64 [n_params], the last 32 padding, as in mlqem_sim_run_f64; run_keys int64 [B].  Site = qubit index.  Kinds:
 *   MLQEM_MPS_OP_U1     a 2x2 matrix (row-major, 4 complex = 8 float64) on the physical index of `site`.  No decomposition.
 *   MLQEM_MPS_OP_U2     a 4x4 matrix (row-major, 16 complex) on the bond (site, site + 1).  orientation 0: its basis index is
 *                       bit(site) + 2 bit(site + 1); orientation 1: bit(site + 1) + 2 bit(site) (a gate whose first qubit is the
 *                       upper one).  A coherent error is such a record; the host may multiply a run of gates confined to one bond
 *                       into one (ideal lowering only, never across a noise record).
 *   MLQEM_MPS_OP_DEPOL1 (lambda) on `site`; MLQEM_MPS_OP_DEPOL2 (lambda) on the bond, orientation as above: q0 = site + orientation
 *                       is the gate's first qubit, q1 the other.  The NOISE records of a circuit are numbered 0, 1, ... in record
 *                       order (lambda == 0 records included).  Noise record i with lambda != 0 draws ONE uniform u (below).
 *                       d = 2 or 4, m = d^2 - 1 = 3 or 15, w = lambda / 4 or lambda / 16 (lambda * 0.25, lambda * 0.0625);
 *                       s_0 = 1 - m w (the product m w rounded, then the difference), s_j = s_(j-1) + w.  The outcome is the
 *                       first j in 0 .. m with s_j > u, else m.  j = 0: nothing (probability 1 - lambda (d^2 - 1) / d^2).  Else
 *                       j = l0 + 4 l1 with the letter l0 on q0 and l1 on q1 (DEPOL1: j = l0), letters 0 I, 1 X, 2 Y, 3 Z, each
 *                       applied as a one-site 2x2 matrix of entries 0, +-1, +-i (nothing is rounded).  lambda == 0: no draw.
 *   MLQEM_MPS_OP_NOISE1 (lambda, g, c, p1) on `site`; MLQEM_MPS_OP_NOISE2 (lambda, (g, c, p1) of q0, (g, c, p1) of q1) on the bond,
 *                       orientation and q0 = site + orientation as for DEPOL2; numbered as their MLQEM_SIM_OP_* twins.  Thermal
 *                       relaxation as quantum jumps (mlqem_mps_run_f64 only: the folded kernel skips them, the host refuses
 *                       them there).  A NOISE record is ONE noise record for the index i, lambda == 0 included.  Inside it:
 *                       first DEPOL1's / DEPOL2's draw with lambda (sub-draw 0; skipped at lambda == 0), then one RELAXATION
 *                       per qubit.  NOISE2: the SITE order of its two relaxations is fixed by the centre: where the centre is
 *                       <= site the lower site goes first, else the upper one (right after a U2 on the bond the centre is on
 *                       site + 1, so the upper site costs no move and the lower one leftward move).  The sub-draw number and
 *                       the triple follow the GATE's qubit -- 1 for q0, 2 for q1 -- not that order.  Relaxations of different
 *                       qubits commute as channels, so the average over the draws is the map of MLQEM_SIM_OP_NOISE2 in either
 *                       order (each step takes its populations from the state the step before left).
 *                       RELAXATION (g, c, p1) of qubit q with sub-draw s:
 *                       1. the centre moves to q, one site at a time, by the two loops of a U2 record (one qubit: no move);
 *                       2. P_s = sum_(l, r) |A[q][l, s, r]|^2, s = 0, 1, reduced in this order: thread j of 256 adds the entries
 *                          (l, r) = l * chi_r + r = j, j + 256, ... in that order from 0.0; the shuffle tree over a wave's 64
 *                          lanes (v += the lane 32, 16, 8, 4, 2, 1 above); the four waves in order ((w0 + w1) + w2) + w3.
 *                          pa = P0 / (P0 + P1), pb = P1 / (P0 + P1), c2 = c c, d = max(0, (1 - g) - c2);
 *                       3. the six outcomes, their probabilities, the uniform u = U(i, s) against their running sum and the
 *                          selection rule are those of mlqem_sim_run_trajectories_f64 (Relaxation, above): the first j with
 *                          s_j > u, else the last j of probability > 0; an outcome of probability exactly 0 is never chosen;
 *                       4. the chosen operator over the root of its own state-given probability, the real 2x2 matrix with the
 *                          factor t = 1 / sqrt(.) tabulated there, is applied to the physical index of A[q].
 *                       Because q holds the centre the other sites stay orthonormal: the state stays canonical, and normalised
 *                       up to rounding.  The applied matrix has operator norm t (c <= 1), and `error_bound` <- t * `error_bound`
 *                       after each relaxation; `discarded` is left alone (see Certificate).
 *   MLQEM_MPS_OP_TWIRL_OPEN / MLQEM_MPS_OP_TWIRL_CLOSE on the bond, orientation and q0 = site + orientation as for DEPOL2 (both
 *                       kernels): a Pauli twirl of what stands between them, drawn per (run, trajectory).  The unit keeps a TWIRL
 *                       INDEX j, 0 at its start, beside and independent of the noise index, and the code of its latest OPEN (0
 *                       before the first).  OPEN reads no params: it draws code = x0 >> 28 (0 .. 15, uniform, the all-identity
 *                       code 0 included) of Philox4x32-10 at the counter (j, 3 << 24 | t, run_key & 0xffffffff, run_key >> 32)
 *                       under the seed's key (sub-draw 3: the depolarising draw is 0, the relaxations 1 and 2, so no other draw
 *                       changes and j may equal a noise index), and applies the letter code & 3 on q0, then code >> 2 on q1,
 *                       as DEPOL2 applies its letters (identity letters: nothing).  An integer: no threshold to sit near.
 *                       CLOSE reads table[0 .. 15] (16 float64; entry c: the code of the pair P' with P' ~ G P_c G^dagger for the
 *                       ideal gate G, signs and phases dropped -- a trajectory is a pure state), applies the letters of
 *                       table[code of the latest OPEN], the entry clamped to 0 .. 15, in the same order, then ++j.  j therefore
 *                       counts the CLOSE records AS EXECUTED: every pass of a folded gate draws its own twirl.  Twirls are
 *                       one-site unitaries: no decomposition, no centre move, nothing added to `discarded` or `error_bound`.
 *                       A dagger bit on either kind is ignored (the host never sets it).  The site is clamped to n - 2; both
 *                       kinds do nothing where n < 2.  A twirled program equals, bit for bit and per trajectory, the program in
 *                       which every OPEN / CLOSE is written out as the U1 records of its two letters (q0's, then q1's, identity
 *                       letters left out, entries 0, +-1, +-i), and the folded contract below extends to the two kinds verbatim.
 *                       mlqem_mps_bind_f64 does not know them (it copies ONE value of a kind it does not know): the host refuses
 *                       such a batch there.
 *   Any other kind is skipped; a two-site record of a one-qubit circuit is skipped.
 * u of noise record i, sub-draw s, trajectory t: Philox4x32-10 with the key (seed & 0xffffffff, seed >> 32) and the counter
 *   (i, s << 24 | t, run_key & 0xffffffff, run_key >> 32), run_key = run_keys[c], t < 2^20; s = 0 for every depolarising draw (the
 *   DEPOL records' bits are what they were), 1 / 2 for the relaxations; u = ((x0 >> 5) 2^26 + (x1 >> 6)) 2^-53.  A unit therefore
 * depends on (seed, run key, t, the circuit's records, max_bond, cutoff) alone: the same bits alone, in any batch, in any split
 * into calls, and in a replayed graph.  No atomics.
 *
 * State.  Site tensors A[q] of shape (chi_l, 2, chi_r), complex float64, |0..0> at the start (all bonds 1), and an orthogonality
 * centre, site 0 at the start.  A U2 record on the bond (q, q + 1):
 *   1. the centre moves to q, one site at a time, by the bond primitive below with the identity as the gate (to the right on the
 *      bond (centre, centre + 1); to the left on (centre - 1, centre), decomposing the transpose);
 *   2. theta[(l, s0), (s1, r)] = sum_m A[q][l, s0, m] A[q + 1][m, s1, r], then the 4x4 matrix on (s0, s1);
 *   3. the columns of theta are orthogonalised by one-sided (Hestenes) Jacobi rotations: cyclic sweeps in the round-robin order
 *      (C columns, C even: round r = 0 .. C - 2 pairs (r, C - 1) and ((r + p) mod (C - 1), (r - p) mod (C - 1)), p = 1 .. C / 2 - 1),
 *      a pair (a, b) rotated where |a^dagger b|^2 > MLQEM_MPS_JACOBI_TOL2 |a|^2 |b|^2 and both |a|^2 and |b|^2 exceed
 *      MLQEM_MPS_JACOBI_NULL = (64 u)^2 of theta's weight (a column below it is the rounding of the dot products; rotations would
 *      only shrink it into the denormals and never end; with a cutoff below MLQEM_MPS_JACOBI_NULL the keep rule may keep such a
 *      column as it is, so keep the cutoff above it), until a sweep rotates nothing or
 *      MLQEM_MPS_SWEEPS sweeps are done (a decomposition whose last allowed sweep still rotated is counted in traj_stats as not
 *      converged: its columns may be short of orthogonal, and so may everything after it); edge bonds (fewer rows than columns) are NOT transposed: their null columns come out with
 *      norm (numerically) zero and the keep rule drops them;
 *   4. sigma_j^2 = the squared norm of column j, sorted descending (ties: the lower column first); total = their sum in that order;
 *   5. KEEP RULE: the longest prefix of at most max_bond columns (and at most min(rows, columns)) with sigma^2 > cutoff * total; at
 *      least one;
 *   6. eps = (sum of the dropped sigma^2, in sorted order) / total is added to `discarded` and sqrt(2 eps) to `error_bound`; the
 *      kept part is rescaled by sqrt(total / kept) to the norm before truncation;
 *   7. A[q] = the kept columns over their norms; 8. A[q + 1] = A[q]^dagger theta, with the theta of step 2, times the rescaling;
 *   9. the centre is q + 1.  The leftward move decomposes theta^T the same way: A[q + 1] takes the orthonormal factor (as rows), A[q]
 *      the other, and the centre is q.  A move is also a decomposition under the same keep rule, max_bond included: the cap
 *      cannot bind there, since the bond a move crosses already has at most max_bond columns and the identity does not raise
 *      theta's rank, so what a move drops is rounding, and it adds that eps to both sums.
 * Certificate.  A truncation replaces the normalised state phi by phi', |phi - phi'| <= sqrt(2 eps); unitaries keep distances, so
 * |psi_exact - psi_mps| <= B = sum sqrt(2 eps) = `error_bound`, and |<O>_exact - <O>_mps| <= 2 B sum|coeff|.  The default cutoff
 * 1e-26 drops the numerically-zero columns of a rank-deficient theta (a cx on a product state); a decomposition that drops only
 * such columns adds at most sqrt(2 * 2 max_bond * cutoff) to B, the floor under `error_bound`.
 *   With NOISE records: a relaxation applies M = K / sqrt(p), |M| = t, which is no unitary: |M x - M y| <= t |x - y|, hence
 * B <- t B.  B then bounds |psi~ - psi_mps| where psi~ is the exact vector carried through the SAME operators M (the ones this
 * trajectory drew, with the MPS's normalisers sqrt(p)); psi~ is not normalised, | |psi~| - 1 | <= B, so its normalised form is
 * within 2 B of psi_mps and |<O>_exact - <O>_mps| <= 4 B sum|coeff| for that trajectory (2 B in the unitary case).  The bound is
 * CONDITIONAL on the operators drawn: the exact state would have drawn them with other probabilities, so it is no bound on the
 * channel average.  Where the bond cap never cuts, B stays at the cutoff's floor (times the t's) and nothing changes.
 *
 * mlqem_mps_run_f64 runs the units (circuit circ_first + u / traj_count, trajectory traj_first + u % traj_count), u < circ_count *
 * traj_count, one workgroup each, into `workspace` (mlqem_mps_workspace_bytes(max_qubits, max_bond, units); max_qubits >= every
 * circuit's width) and writes traj_stats [trajectories][B][MLQEM_MPS_STATS] = (discarded, error_bound, largest bond,
 * decompositions, decompositions that did not converge within MLQEM_MPS_SWEEPS, most sweeps of one decomposition) of each.
 * mlqem_mps_terms_f64 reads the same workspace.  Terms: term t of circuit term_circ[t] is the Pauli string letters[term_off[t] + q],
 * q < n (uint8, 0 I, 1 X, 2 Y, 3 Z).  readout float64 [n_sites][2] holds (a, b) of site site_ptr[c] + q: (1, 0) without readout
 * noise, (1 - p01 - p10, p01 - p10) for a measured qubit with it; a Z slot uses the diagonal operator a Z + b I, an I slot plain
 * I: exact, no term is expanded (the host refuses X / Y beside readout noise).  One launch contracts E <- sum A[q]^dagger A[q] E
 * per unit into traj_norm [trajectories][B]; a second, one workgroup per (unit, term of term_first .. term_first + term_count),
 * contracts with the term's operators and writes traj_term_values [trajectories][n_terms] = that over the unit's norm.
 * mlqem_mps_finish_f64 forms, in trajectory order as mlqem_sim_run_trajectories_f64 does: term_values / term_std_error [n_terms],
 * values / std_error [B] (0 at one trajectory), norm, discarded and error_bound [B] (means) and bond int32 [B] (the maximum).
 * Bad sizes, a null or misaligned buffer: MLQEM_ERR_BAD_ARG; a count over 2^31 - 1: MLQEM_ERR_UNSUPPORTED; a workspace that is too
 * small: MLQEM_ERR_WORKSPACE; all before anything is launched.  No host read: capturable.
 *
 * mlqem_mps_run_folded_f64 (zero-noise extrapolation on this path; an additive symbol, the ABI version is unchanged).  The B
 * circuits are lowered ONCE -- n_qubits, op_ptr, ops and params are those of mlqem_mps_run_f64 and are not replicated per factor --
 * and every (circuit, noise factor) pair gets a schedule in the format of mlqem_sim_run_folded_f64: run r = f * B + c is circuit c
 * at noise factor f, 0 <= f < n_factors = F; sched_ptr int64 [F * B + 1]; run r owns sched[sched_ptr[r] .. sched_ptr[r + 1]), int32
 * entries (k << 1) | dagger with k a record index RELATIVE to op_ptr[c].  blackwater.sim.zne builds them (build_mps_schedules).
 *   Units.  Unit u < run_count * traj_count is (run run_first + u / traj_count, trajectory traj_first + u % traj_count), one
 *     workgroup each; its slice of `workspace` has the layout of mlqem_mps_run_f64's, so mlqem_mps_terms_f64 and
 *     mlqem_mps_finish_f64 read it unchanged when they are called with the F * B runs as a batch of F * B circuits (the per-circuit
 *     arrays n_qubits, term_circ, term_off, site_ptr, term_ptr and coeff tiled F times on the host; letters and readout shared
 *     through the offsets).
 *   Daggers.  dagger = 1 on a U1 / U2 entry applies the conjugate transpose of the record's matrix, formed while the record is
 *     read by swapping indices and flipping the sign of the imaginary parts (a multiplication by -1.0: no rounding); the record's
 *     orientation is unchanged.  On DEPOL1 / DEPOL2 the bit is ignored: a noise record is never inverted.  A coherent-error U2 must
 *     never be scheduled with the bit set; the host guarantees that, the kernel does not check it.
 *   Draws.  The noise index of the draw contract is the ORDINAL of the noise entry as this run executes it (0, 1, 2, ...: an entry
 *     that is scheduled three times draws three times), and the key is run_keys[r], int64 [F * B].  With these two rules a run
 *     equals, bit for bit, mlqem_mps_run_f64 on the program obtained by writing its schedule out (daggered matrices
 *     conjugate-transposed on the host), under the same key.  The twirl index follows the same rule: it is the ordinal of the
 *     TWIRL_CLOSE entry as this run executes it, so a fold unit OPEN, gate | dagger, noise records, CLOSE draws a twirl per pass.
 *   traj_stats is [trajectories][F * B][MLQEM_MPS_STATS], a row per run.
 *   Clamping.  Schedule offsets are clamped to n_sched, k to the circuit's records (a circuit without records skips its
 *     entries), run numbers to F * B; an empty schedule leaves |0..0>; a malformed schedule computes garbage inside the unit's own
 *     slice and faults nothing.
 * Bad sizes (n_factors < 1, n_sched < 0, a run or trajectory range outside F * B runs and `trajectories`), a null or misaligned
 * buffer: MLQEM_ERR_BAD_ARG; F * B, n_params, n_sched or run_count * traj_count over 2^31 - 1: MLQEM_ERR_UNSUPPORTED; a workspace
 * that is too small: MLQEM_ERR_WORKSPACE; all before anything is launched.  No host read: capturable.
 * ---------------------------------------------------------------------------------------------------- */
#define MLQEM_MPS_MAX_BOND 32
#define MLQEM_MPS_MAX_QUBITS 512
#define MLQEM_MPS_SWEEPS 30
#define MLQEM_MPS_STATS 6
#define MLQEM_MPS_JACOBI_TOL2 1e-28
#define MLQEM_MPS_JACOBI_NULL 5.048709793414476e-29
#define MLQEM_MPS_OP_U1 0
#define MLQEM_MPS_OP_U2 5
#define MLQEM_MPS_OP_DEPOL1 6
#define MLQEM_MPS_OP_DEPOL2 7
#define MLQEM_MPS_OP_NOISE1 10
#define MLQEM_MPS_OP_NOISE2 11
#define MLQEM_MPS_OP_TWIRL_OPEN 17  /* free in the MLQEM_SIM_OP_* space too (12 .. 16 are the parameterised kinds) */
#define MLQEM_MPS_OP_TWIRL_CLOSE 18
size_t mlqem_mps_workspace_bytes(int64_t max_qubits, int64_t max_bond, int64_t n_units);
int mlqem_mps_run_f64(int64_t n_circuits, const int32_t* n_qubits, const int64_t* op_ptr, const mlqem_sim_op* ops, int64_t n_ops,
                      const double* params, int64_t n_params, const int64_t* run_keys, int64_t circ_first, int64_t circ_count,
                      int64_t traj_first, int64_t traj_count, int64_t trajectories, uint64_t seed, int64_t max_bond, double cutoff,
                      int64_t max_qubits, void* workspace, size_t workspace_bytes, double* traj_stats, mlqem_stream_t stream);
int mlqem_mps_run_folded_f64(int64_t n_circuits, int64_t n_factors, const int32_t* n_qubits, const int64_t* op_ptr,
                             const mlqem_sim_op* ops, int64_t n_ops, const double* params, int64_t n_params, const int64_t* sched_ptr,
                             const int32_t* sched, int64_t n_sched, const int64_t* run_keys, int64_t run_first, int64_t run_count,
                             int64_t traj_first, int64_t traj_count, int64_t trajectories, uint64_t seed, int64_t max_bond,
                             double cutoff, int64_t max_qubits, void* workspace, size_t workspace_bytes, double* traj_stats,
                             mlqem_stream_t stream);
int mlqem_mps_terms_f64(int64_t n_circuits, const int32_t* n_qubits, int64_t circ_first, int64_t circ_count, int64_t traj_first,
                        int64_t traj_count, int64_t trajectories, int64_t max_bond, int64_t max_qubits, const void* workspace,
                        size_t workspace_bytes, int64_t term_first, int64_t term_count, int64_t n_terms, const int32_t* term_circ,
                        const int64_t* term_off, const uint8_t* letters, int64_t n_letters, const int64_t* site_ptr,
                        const double* readout, int64_t n_sites, double* traj_term_values, double* traj_norm, mlqem_stream_t stream);
int mlqem_mps_finish_f64(int64_t n_circuits, int64_t n_terms, int64_t trajectories, const int64_t* term_ptr, const double* coeff,
                         const double* traj_term_values, const double* traj_norm, const double* traj_stats, double* term_values,
                         double* term_std_error, double* values, double* std_error, double* norm, double* discarded,
                         double* error_bound, int32_t* bond, mlqem_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Shots from a matrix-product state (three additive symbols, the ABI version is unchanged): measurement outcomes of the state
 * that mlqem_mps_run_f64 left in `workspace`, by perfect sampling.  blackwater.sim.mps lowers for it (compile_mps_shots) and
 * blackwater.native.ops.mps_sample / mps_sample_finish call it.  The sampled distribution is that of the TRUNCATED state; its
 * trace distance from the exact state's is at most the run's error_bound.
 *
 * mlqem_mps_sample_f64 takes one chunk of units exactly as mlqem_mps_terms_f64 does (after mlqem_mps_run_f64 on the same chunk and
 * workspace) plus `sample_workspace` (mlqem_mps_sample_workspace_bytes(max_qubits, max_bond, units): n 2 chi^2 16 B per unit).
 * It does not rely on the gauge (the orthogonality centre is not stored):
 *   Environment pass, one workgroup per unit, right to left: R[n] = [1]; G[q][l, s, r'] = sum_r A[q][l, s, r] R[q + 1][r, r'] is
 *   written to sample_workspace; R[q][l, l'] = sum_(s, r') G[q][l, s, r'] conj(A[q][l', s, r']).  Sums in index order, no atomics.
 *   Sampling pass, one workgroup per (group of the chunk, trajectory of the chunk, block of MLQEM_MPS_SHOT_BLOCK = 16 of that
 *   trajectory's shots).  Shot s < shots belongs to trajectory s mod trajectories (T = 1 without noise).  Its left vector v starts
 *   as [1]; at site q = 0, 1, ..., n - 1: a[s, r] = sum_l v[l] A[q][l, s, r] and g[s, r] = sum_l v[l] G[q][l, s, r]; the group's
 *   basis letter at the site mixes the physical index of both (0 I and 3 Z: nothing; 1 X: (a0 + a1) c, (a0 - a1) c; 2 Y:
 *   (a0 - i a1) c, (a0 + i a1) c; c = 0.7071067811865476); the unnormalised weight of outcome b is p_b = sum_r Re(g[b, r]
 *   conj(a[b, r])); one outcome b is drawn (below); v <- a[b, .] / sqrt(p_b), with the true outcome b, not the reported bit.
 * DRAW CONTRACT.  Circuit c with run key k = run_keys[c], group g inside its circuit (g < MLQEM_MPS_MAX_GROUPS = 4 096), shot s,
 * site q: Philox4x32-10 with the key (seed & 0xffffffff, seed >> 32) and the counter (0x80000000 | g << 9 | q, s, k & 0xffffffff,
 * k >> 32) -- the top bit of the first word keeps these draws apart from the noise draws, whose counter is (record index,
 * trajectory, key words).  u = ((x0 >> 5) 2^26 + (x1 >> 6)) 2^-53, u' the same from (x2, x3).  w_b = p_b where p_b > 0, else 0 (a
 * NaN weight counts as 0); target = u * (w0 + w1), one rounded product of the rounded sum; b = 0 if target < w0 or not (w1 > 0),
 * else 1: an outcome of weight zero is unreachable.  The reported bit is b xor (u' < flip[site_ptr[c] + q][b]); flip float64
 * [n_sites][2] is (P(read 1 | 0), P(read 0 | 1)) of a measured qubit with readout noise and (0, 0) otherwise, so the mean of the
 * reported Z is a <Z> + b of the readout table of mlqem_mps_terms_f64.  Bits are packed as mlqem_clifford_sample_f64 packs them:
 * W = ceil(n / 32) uint32 words per (group, shot), bit q in word q >> 5, the words of global group G, shot s at bits[ref_ptr[G] *
 * shots + s * W] (ref_ptr int64 [n_groups + 1], the running sum of W; bits may be null with n_bits = 0).  The bits of a (circuit,
 * group, shot) depend on (seed, run key, group, shot, the circuit's records, max_bond, cutoff, trajectories) alone: the same
 * alone, in any batch, under any split into chunks and in a replayed graph.
 * Groups.  group_ptr int64 [B + 1] (a circuit's groups; max_groups is the largest count of one circuit), group_circ int32
 * [n_groups], group_off int64 [n_groups]: the group's n basis letters basis[group_off[G] + q] (uint8: 0 / 3 Z basis, 1 X, 2 Y);
 * the chunk's groups are group_first .. group_first + group_count (those of its circuits).  Terms: term t has the support
 * masks[term_mask[t] + w], w < W; gterm_ptr int64 [n_groups + 1] / gterm int32 [n_terms] list the terms of a group.  S_t = sum_s
 * (-1)^popcount(bits_s & support_t) is added with integer atomics into term_sums int32 [n_terms]; a call with traj_first == 0
 * first zeroes term_sums[term_first .. term_first + term_count) (the terms of the chunk's circuits) on the stream, so the chunks
 * of one circuit run in trajectory order.  No float atomics.
 * mlqem_mps_sample_finish_f64 forms, with the expressions of mlqem_sim_sample_f64: term_values = (double)S_t / (double)shots,
 * values = fma(coeff, term, values) in term order from 0.0, variance = fma(coeff^2, fma(-term, term, 1), variance).
 * shots outside 1 .. MLQEM_SIM_MAX_SHOTS, bad sizes, a null or misaligned buffer: MLQEM_ERR_BAD_ARG; max_groups over 4 096 or a
 * count over 2^31 - 1: MLQEM_ERR_UNSUPPORTED; a workspace that is too small: MLQEM_ERR_WORKSPACE; all before anything is
 * launched.  No host read: capturable.  Every index read from a buffer is clamped: malformed input computes garbage.
 * ---------------------------------------------------------------------------------------------------- */
#define MLQEM_MPS_SHOT_BLOCK 16
#define MLQEM_MPS_MAX_GROUPS 4096
size_t mlqem_mps_sample_workspace_bytes(int64_t max_qubits, int64_t max_bond, int64_t n_units);
int mlqem_mps_sample_f64(int64_t n_circuits, const int32_t* n_qubits, int64_t circ_first, int64_t circ_count, int64_t traj_first,
                         int64_t traj_count, int64_t trajectories, int64_t max_bond, int64_t max_qubits, const void* workspace,
                         size_t workspace_bytes, void* sample_workspace, size_t sample_workspace_bytes, int64_t group_first,
                         int64_t group_count, int64_t n_groups, int64_t max_groups, const int64_t* group_ptr, const int32_t* group_circ,
                         const int64_t* group_off, const uint8_t* basis, int64_t n_basis, const int64_t* site_ptr, const double* flip,
                         int64_t n_sites, const int64_t* ref_ptr, const int64_t* gterm_ptr, const int32_t* gterm, int64_t term_first,
                         int64_t term_count, int64_t n_terms, const int32_t* term_mask, const uint32_t* masks, int64_t n_masks,
                         const int64_t* run_keys, int64_t shots, uint64_t seed, int32_t* term_sums, uint32_t* bits, int64_t n_bits,
                         mlqem_stream_t stream);
int mlqem_mps_sample_finish_f64(int64_t n_circuits, int64_t n_terms, int64_t shots, const int64_t* term_ptr, const double* coeff,
                                const int32_t* term_sums, double* term_values, double* values, double* variance, mlqem_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Parameter binding for matrix-product states (one additive symbol, the ABI version is unchanged).  Templates are lowered ONCE
 * (blackwater.sim.compile_mps_templates): op_ptr int64 [C + 1], ops [n_ops] and params [n_params] are those of mlqem_mps_run_f64
 * with a template per circuit (the matrix of a parameterised record stands at the placeholder angle 0 and is not read), and
 * pool_ptr int64 [C + 1] names template c's slice params[pool_ptr[c] .. pool_ptr[c + 1]).  mlqem_mps_bind_f64 writes, on the
 * device, the batch that the lowering of the R = n_runs BOUND COPIES would have produced; mlqem_mps_run_f64, _run_folded_f64,
 * _terms_f64, _finish_f64 and _sample_f64 then run on it unchanged.
 * FACTOR PROGRAM.  Record j (global) owns the factors fac_ptr[j] .. fac_ptr[j + 1] (fac_ptr int64 [n_ops + 1]); none: the
 * record is copied.  With factors (U1 and U2 records only) its matrix is F_k ... F_2 F_1, d x d with d = 2 (U1) or 4 (U2: over
 * bit(lower site) + 2 bit(upper site), orientation 0).  fac int32 [n_fac][4] = (kind, slot, parameter, offset), fac_val float64
 * [n_fac][2] = (scale, offset):
 *   kind MLQEM_MPS_FACTOR_FIXED: the d x d matrix fpool[offset ..], row-major (re, im), 8 or 32 float64 (fpool float64 [n_fpool],
 *     n_fpool >= 32: the padding the longest read needs) -- the host product of a maximal run of consecutive fixed gates;
 *   kind MLQEM_SIM_OP_PRX / PRY / PRZ / PP / PRZZ: a PARAM factor on slot 0 (the lower site; the site of a U1 record), 1 (the
 *     upper site) or 2 (the bond: PRZZ).
 * RUNS.  runs int32 [R][4] = (template, theta row, shifted occurrence or -1, reserved) and shift float64 [R], as in
 * mlqem_sim_run_bound_f64; theta float64 [n_rows][ld_theta].  An occurrence is a PARAM factor: template c owns the occurrences
 * occ_ptr[c] .. occ_ptr[c + 1] (int64 [C + 1]), in circuit order, occ int32 [n_occ][2] = (record relative to op_ptr[c], factor
 * inside the record); the run's third entry counts from occ_ptr[c], and one outside the template's occurrences is none.
 * OUTPUT.  Run r gets the records out_ops[out_op_ptr[r] + k] = (kind, site, orientation, P) for the template's records k, with
 * P = out_pool_ptr[r] + (the template's offset - pool_ptr[c]), and the slice of out_pool that starts at out_pool_ptr[r]
 * (out_op_ptr, out_pool_ptr int64 [R]: the running sums of the templates' record and value counts, the caller's; n_out_pool
 * counts 32 values of padding at the end, as `params` does).  max_records: the largest record count of a template that a run
 * names (the launch's second grid dimension is sized by it; records past it are still reached).
 * ARITHMETIC CONTRACT (tests/mps_bound_cases.bind_host follows it operation by operation).  phi = scale * theta[row][parameter]
 * + offset, then + shift[r] if this factor is the run's shifted occurrence: a product and one or two sums, each rounded on its
 * own (the file is compiled under `#pragma clang fp contract(off)`: no fma).  (co, si) = (cos, sin)(0.5 * phi) -- an exact product
 * -- for PRX, PRY, PRZ, PRZZ and (cos, sin)(phi) for PP, as the fixed gates of blackwater/sim/program.py define them.  The
 * factors' matrices: PRX [[co, -i si], [-i si, co]], PRY [[co, -si], [si, co]], PRZ diag(co - i si, co + i si), PP diag(1, co +
 * i si) on the slot's bit of the row index; PRZZ the diagonal with co - i si where the two bits are equal and co + i si where
 * they differ.  M = F_1 (a PARAM factor written out as its d x d matrix, zeros exact), then M <- F M for each further factor:
 *   FIXED   (F M)[i][j] = sum over k = 0 .. d - 1, ascending, of F[i][k] M[k][j], the first product as it is, each further one
 *           added to the sum;
 *   PRX/PRY (G M)[i][j] = g[b][0] M[i0][j] + g[b][1] M[i1][j], b the slot's bit of i, i0 / i1 = i with that bit clear / set:
 *           applied as its 2x2, never as a 4x4 with zeros;
 *   diagonal kinds  (D M)[i][j] = D[i] M[i][j].
 *   A complex product is (a.re b.re - a.im b.im, a.re b.im + a.im b.re), four products, then one difference and one sum; a sum
 *   of complex numbers is one sum per part.  No contraction anywhere.
 * Records without factors, and DEPOL1 / DEPOL2 records, are copied bit for bit.  No atomics, no cross-run data: a run's slice
 * of out_pool and its rows of out_ops depend on (template, theta row, shift) alone -- the same alone, in any batch, under any
 * split into calls and in a replayed graph.  Sixteen lanes form one record, lane e its entry e (csrc/mps_bind.hip says why).
 * Every index read from a buffer is clamped (template, row, parameter, record and factor ranges, pool offsets: an offset is
 * clamped to [0, n - 32] of its pool, so a matrix always fits): malformed input computes garbage, never reads or writes outside a
 * buffer.  A negative size, n_params / n_fpool / n_out_pool < 32, a null or misaligned buffer (ops, fac, runs, out_ops: 16 B;
 * float64 buffers: 8 B), n_templates / n_rows / ld_theta < 1 with runs: MLQEM_ERR_BAD_ARG; a count over 2^31 - 1:
 * MLQEM_ERR_UNSUPPORTED; all before anything is launched.  n_runs == 0 or max_records == 0: MLQEM_OK, nothing is written.
 * No host read: capturable, on one stream with the run that follows.
 * ---------------------------------------------------------------------------------------------------- */
#define MLQEM_MPS_FACTOR_FIXED 0
int mlqem_mps_bind_f64(int64_t n_templates, const int64_t* op_ptr, const mlqem_sim_op* ops, int64_t n_ops, const double* params,
                       int64_t n_params, const int64_t* pool_ptr, const int64_t* fac_ptr, const int32_t* fac, const double* fac_val,
                       int64_t n_fac, const double* fpool, int64_t n_fpool, const int64_t* occ_ptr, const int32_t* occ, int64_t n_occ,
                       const double* theta, int64_t n_rows, int64_t ld_theta, const int32_t* runs, const double* shift, int64_t n_runs,
                       int64_t max_records, const int64_t* out_op_ptr, const int64_t* out_pool_ptr, mlqem_sim_op* out_ops,
                       int64_t n_out_ops, double* out_pool, int64_t n_out_pool, mlqem_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MLQEM_HIP_H */
