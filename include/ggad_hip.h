/*
 * ggad_hip.h -- C ABI of the MI355X-native GGAD hot path (libggad_hip.so).
 *
 * The reference (mala-lab/GGAD) has no FFI / plugin layer: its boundary is the Python
 * class surface.  This header is the C-ABI that sits UNDER that surface:
 * every entry point replaces a group of ATen call sites of the reference (cited per
 * function as file:line relative to the reference tree) and is what a binding in the
 * reference would call (ctypes stub: INTEGRATION.md).
 *
 * Conventions
 *   - plain pointers + sizes only; every pointer is a DEVICE pointer unless the name
 *     ends in _host; no ownership transfer: the caller (PyTorch allocator in the Python
 *     host layer) allocates every input, output and workspace;
 *   - a workspace (`workspace`, `ws`, `scratch`, `part`, `xs_workspace`) carries nothing from call to call and may be larger than
 *     the call needs.  The full-graph entry points state their contract at the parameter: "contents on entry are arbitrary" (any
 *     bit pattern, NaN included; tests/test_dirty_memory_gpu.py and tests/test_handoff_gpu.py hold them to it) or the exact
 *     requirement (ticket words and the TAM head's workspace: zero before the first call);
 *   - all work is enqueued on `stream` (a hipStream_t passed as void*) and is
 *     asynchronous; functions are re-entrant per stream and keep no global mutable
 *     state: the only cross-call state is in buffers the caller passes (counter slots,
 *     optimiser state);
 *   - return value: 0 = success, negative = error (GGAD_E_*), never throws;
 *   - indices are int32, values fp32; row-major;
 *   - graph = CSR (rowptr[n+1], col[nnz]) with sorted, de-duplicated columns per row.
 */
#ifndef GGAD_HIP_H
#define GGAD_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GGAD_OK 0
#define GGAD_E_INVALID (-1)   /* bad argument (null pointer, unsupported size)          */
#define GGAD_E_LAUNCH (-2)    /* HIP launch / runtime error, see ggad_last_error()       */
#define GGAD_E_CAPACITY (-3)  /* caller-provided workspace too small                     */
#define GGAD_E_UNSUPPORTED (-4) /* this entry point does not take the shape; nothing was launched (the documented fallback applies) */

typedef void *ggad_stream_t;  /* hipStream_t */

/* ABI version of this header; bumped on any signature change. */
int ggad_abi_version(void);
/* Text of the last HIP error seen by this thread ("" if none). Host pointer, static storage. */
const char *ggad_last_error(void);
/* Upper limits compiled into the kernels (embedding width, feature width). */
int ggad_max_embed_dim(void);
int ggad_max_feat_dim(void);
/* ggad_max_embed_dim() (64) is the width of the one-lane-per-channel kernels: the fused chain-0 step, the XCD-resident chunk
 * kernel, the one-shot exchange and every comparison handler.  The mini-batch step chain (the ggad_mb_* entry points below)
 * also takes 64 < D <= ggad_mb_wide_max_embed_dim() (256) on the wide chain (csrc/step_wide.hip: a lane owns the channels
 * lane + 64 j).  ggad_mb_wide_supported(D, F) != 0  <=>  1 <= D <= 256 and 1 <= F <= ggad_max_feat_dim() (1024): the wide
 * kernels keep nothing of size F or D*D in LDS or registers, so F is bounded by the plan's gather kernels only.  Every
 * ggad_mb_* entry point that takes (D, F) accepts D > 64 when this predicate holds, with the buffer contracts it has at
 * D <= 64 (at D <= 64 its own limits apply: (4 F D + 512) floats of LDS <= 150 KB); ggad_mb_train_chunk_xchg and
 * ggad_mb_train_chunk_xcd return GGAD_E_INVALID at D > 64 and launch nothing. */
int ggad_mb_wide_max_embed_dim(void);
int ggad_mb_wide_supported(int32_t D, int32_t F);
/* ggad_mb_supported(D, F) != 0  <=>  the one-lane-per-channel chain (chains 0 and 2) takes the shape: 1 <= D <= 64,
 * 1 <= F <= ggad_max_feat_dim() and (4 F D + 512) floats of LDS <= 150 KB, that is F D <= 9472.  A shape it refuses at D <= 64
 * and F <= 1024 trains on the wide chain (chain 3). */
int ggad_mb_supported(int32_t D, int32_t F);

/* ------------------------------------------------------------------------------------
 * Generic device primitives
 * ---------------------------------------------------------------------------------- */

/* out[0..n] = exclusive prefix sum of in[0..n-1] (out[n] = total).  n <= 4,194,304.
 * workspace: int32[ggad_scan_workspace_elems(n)]; contents on entry are arbitrary (tile sums and offsets: never addresses). */
int64_t ggad_scan_workspace_elems(int64_t n);
int ggad_exclusive_scan_i32(const int32_t *in, int32_t *out, int64_t n, int32_t *workspace, ggad_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Mini-batch path (DGraph-Fin): batch sub-graph plan + gather-aggregate
 * Replaces GCNAggregator.forward, src/graphsage.py:295-360 (python set unions, dense
 * B x U and U x U2 masks, sum/sqrt/div normalisation, Embedding gather, mask.mm).
 *
 * A "chunk" is G batches processed together; rows = all batch nodes of the chunk
 * (batch g owns rows [batch_ptr[g], batch_ptr[g+1])).  Batch g uses counter slot g:
 * slot arrays are int32[G * n_nodes], all-zero on entry and all-zero again when
 * ggad_mb_plan_build returns.
 *
 * Entry e (0 <= e < E) is one element j of the closed neighbourhood N(i)+{i} of row i
 * (graphsage.py:305), rows in order, columns ascending.  The "owner" entry of (batch, j)
 * is one entry of that batch with column j; 2-hop rows are stored at owner entries, so
 * the deduplicated set U of graphsage.py:306 is { e : ent_own[e] == e }.
 * ---------------------------------------------------------------------------------- */

/* ---- one chunk plan in ONE host call ------------------------------------------------------------------------------
 * ggad_mb_plan_build replaces, for all batches of a chunk, what GCNAggregator.forward does per batch
 * (src/graphsage.py:295-360): the closed-neighbourhood entry lists (:305-311), the column sums c_j / c'_k of the dense
 * B x U and U x U2 masks (:315,:342), the set of distinct columns U (owner entries), the 1-hop aggregate
 *   x1[i] = sum_{j in N(i)+{i}} feat[j] / (sqrt(r_i) sqrt(c_j))                                              (:314-326)
 * and (train plans) the 2-hop aggregate at owner entries
 *   x2[e] = sum_{k in N(u)} feat[k] / (sqrt(|N(u)|) sqrt(c'_k)),  u = ent_col[e]                              (:335-355).
 * Host part (no device round trip): closed degrees -> entry offsets, the pieces of <= ggad_mb_chunk_len() consecutive
 * entries every row is cut into (the unit of work of the entry-parallel kernels: a 2,000-neighbour hub row is 125
 * independent pieces, not one wave's loop), the permutation "label-0 rows first" of graphsage.py:450 (pos_meta / row_pos,
 * see ggad_mb_loss), all packed into ONE pinned staging block and uploaded with one copy.  Device part: k_expand
 * (entries, c_j histogram, owner election) -> k_gather1c (x1 partials per piece, owner metadata, pair-count storage,
 * per-node owner lists) -> k_combine1_reset (x1 of multi-piece rows; 1-hop counter slots back to zero) and, for train plans,
 * the LDS-counting 2-hop stage: k_seg_transpose -> k_tile_counts -> k_build_groups -> k_gather2_items -> k_gather2_combine
 * (hop2_ldsw.hip), or the device-atomic fallback k_count2 -> k_gather2 -> reset when a chunk exceeds the LDS path's limits
 * (>= 65,536 entries in a batch, >= 2^31 2-hop pairs).  Every floating-point sum has a fixed order; which duplicate entry of
 * (batch, column) becomes the owner is a race, owners are storage locations only (read through ent_own).
 *
 * All buffers are the caller's.  Slot arrays cnt1 / own1 (/ cnt2): int32[max_batches * n_nodes], cnt1 / cnt2 zero on entry
 * and zero again on return.  Counters: int32[8].  The staging block holds, at the element offsets returned in the info
 * struct: batch_ptr[nb+1], batch_ent_ptr[nb+1], nodes[R], labels[R], pos_meta[R], row_pos[R], row_slot[R], ent_ptr[R+1],
 * row_ck_ptr[R+1], ck_rc[C], ck_e0[C]   (ck_rc[c] = (row << 6) | entries of piece c, ck_e0[c] = its first entry). */
typedef struct ggad_mb_plan {
  /* graph on the device: CSR, feature table (rows feat_stride floats apart), ldsw tile table (ggad_mb_tile_offsets) */
  const int32_t *rowptr, *col;
  const float *feat;
  const int32_t *tile_off;
  /* graph on the host: |N(i) + {i}| per node; sum_{k in N(i)+{i}} deg(k) per node (upper bound of the 2-hop pairs) */
  const int32_t *closed_deg_host;
  const int64_t *pair_bound_host;
  /* staging: pinned host block, its device twin, an event of ggad_event_create guarding the host block */
  int32_t *stage_host, *stage;
  void *stage_event;
  /* per-batch counter slots */
  int32_t *cnt1, *own1, *cnt2;
  /* per entry (ent_cap) */
  int32_t *ent_col, *ent_slot, *ent_row, *ent_own, *ent_c1;
  float *x1, *x2;
  float *ck_part;            /* float[ck_cap * ck_part_stride]: per-piece partial sums (shared with the step kernels) */
  /* LDS-counting 2-hop stage (train plans) */
  int32_t *own_deg, *own_rp, *pw_base, *seg_t, *node_head, *own_next, *grp, *items, *counters;
  uint16_t *pc;
  float *part2;
  void *ev_gather0, *ev_gather1; /* optional events recorded around the 2-hop gather launches (roofline timing) */
  int64_t n_nodes, ent_cap, ck_cap, pair_cap, item_cap, part2_cap, stage_cap, seg_cap;
  int32_t feat_dim, feat_stride, max_batches, rows_cap, ck_part_stride;
  int32_t train;             /* 0: inference plan (1-hop only) */
  int32_t hop2;              /* 1: LDS counting ("ldsw"), 2: device atomics ("global") */
  int32_t node_major;        /* ldsw gather: occurrences of a node in the chunk share the fetch of its neighbour rows */
  float mean_nbr_deg;        /* sum deg^2 / sum deg (memset vs walk when the global counters are cleared) */
  int32_t xcd_skip;          /* -1: plain launches.  0..7: the plan kernels leave one XCD to the XCD-resident chunk kernel: the
                                workgroups with blockIdx % 8 == xcd_skip return at once (ggad_xcd_first_of_stream tells which
                                residue the stream's dispatcher puts on which XCD); results do not depend on it */
  void *ev_tile0, *ev_tile1;  /* optional events recorded around k_tile_counts (the pair counting of the LDS 2-hop stage) */
  const int64_t *node_pack_host; /* optional (ABI 6): (closed_deg_host[i] << 40) | pair_bound_host[i] per node -- the sizing pass of
                                    ggad_mb_plan_build then takes ONE cache miss per batch node instead of two (it is on the critical
                                    path of a one-chunk run).  Null: the two tables above are read. */
  const int32_t *tile_start, *col_t; /* optional (ABI 8): the tile-major copy of col and the table of its segment starts
                                        (ggad_mb_tile_major).  With both set the pair counting of the LDS 2-hop stage reads col_t -- a
                                        tile's segments contiguous, its workgroups on one XCD -- instead of 16-byte pieces of rows. */
} ggad_mb_plan;

typedef struct ggad_mb_plan_info {
  int64_t pair_bound;
  int64_t off_batch_ptr, off_batch_ent_ptr, off_nodes, off_labels, off_pos_meta, off_row_pos, off_row_slot, off_ent_ptr,
      off_row_ck_ptr, off_ck_rc, off_ck_e0;
  /* capacities this chunk needs (also filled when the call returns GGAD_E_CAPACITY: grow and call again) */
  int64_t need_rows, need_ents, need_chunks, need_pairs, need_items, need_part2, need_stage, need_seg;
  int32_t n_batches, n_rows, n_ents, n_chunks;
  int32_t mode;              /* 0 inference, 1 ldsw, 2 global */
  int32_t need_cnt2;
} ggad_mb_plan_info;

int32_t ggad_mb_chunk_len(void);          /* 16 */
int32_t ggad_mb_slice_len(void);          /* neighbours per work item of the 2-hop gather */
int32_t ggad_mb_group_words(void);        /* ints per record of grp[] */
/* Options of the node-major 2-hop gather, process-wide (a negative value leaves an option as it is):
 *   mfma_min_batches  builds of at least this many batches take the matrix-core slice when feat_dim = 17 and feat_stride = 32
 *                     (default 0 = always, GGAD_GATHER_MFMA_BATCHES; INT32_MAX = never).  The two slices add the same
 *                     products in different fixed orders: x2 agrees to ~1e-7 relative, not bit for bit.
 *   range_deg         owners with more neighbours are gathered by eighths of the id space, one per XCD (default 0 = off,
 *                     GGAD_RANGE_DEG; values below 256 mean 256).  Measured slower than slices of 256. */
int ggad_mb_set_gather_options(int32_t mfma_min_batches, int32_t range_deg);
int32_t ggad_mb_item_words(void);         /* ints of items[] per unit of item_cap: work items, the list of range-partitioned groups, their range bounds */
int32_t ggad_mb_plan_counter_elems(void); /* ints of ggad_mb_plan::counters (one counter per 64-byte line) */
/* nodes_host: the batches back to back; batch_ptr_host[nb+1]; labels_host (0/1, NULL for inference plans).  Host outputs
 * (each may be NULL): ent_ptr_host_out[R+1], batch_ent_ptr_host_out[nb+1], batch_max_row_host_out[nb]. */
int ggad_mb_plan_build(const ggad_mb_plan *plan, const int64_t *nodes_host, const int32_t *batch_ptr_host, int32_t n_batches,
                       const int64_t *labels_host, ggad_mb_plan_info *info, int64_t *ent_ptr_host_out,
                       int64_t *batch_ent_ptr_host_out, int32_t *batch_max_row_host_out, ggad_stream_t stream);

/* HIP events through the C-ABI (timing of single launches on the stream they run on; guards of pinned staging memory). */
int ggad_event_create(int32_t timing, void **out);
int ggad_event_destroy(void *event);
int ggad_event_record(void *event, ggad_stream_t stream);
int ggad_event_synchronize(void *event);
int ggad_event_elapsed_ms(void *start, void *stop, float *ms_host);

/* out[i] = mean of feat rows over the explicit ragged list seg_col[seg_ptr[i] .. seg_ptr[i+1])
 * (MeanAggregator.forward with host-side sampling, graphsage.py:66-99). */
int ggad_seg_mean(const float *feat, int32_t feat_dim, const int32_t *seg_ptr, const int32_t *seg_col, int32_t n_rows,
                  float *out, ggad_stream_t stream);
/* Same ragged gather with explicit weights: out[i] = sum_e seg_w[e] * feat[seg_col[e]] -- the 2-hop mask of IntraAgg,
 * 1 / (sqrt(row sum) sqrt(column sum)) per element (src/layers.py:227-242). */
int ggad_seg_wsum(const float *feat, int32_t feat_dim, const int32_t *seg_ptr, const int32_t *seg_col, const float *seg_w,
                  int32_t n_rows, float *out, ggad_stream_t stream);

/* Reconstruction term of the mini-batch DOMINANT / AnomalyDAE comparison models, which run on the same 1-hop batch
 * aggregate as GGAD (src/graphsage_dominant.py:154-157,167-171; src/graphsage_anomalydae.py:154-162,172-176):
 *   loss = mean_c sqrt( sum_b w(a[b][c]) * (a[b][c] - t[b][c])^2 ),  w = w_pos where a > 0, else w_neg
 * -- the inner sum runs over the batch axis, as written there (torch.sum(diff, 0)).  a, t: (n_rows, n_cols) row-major.
 * loss: 1 float.  col_sum (n_cols floats, the sums under the root) and da (n_rows * n_cols, d loss / d a) may be NULL. */
int ggad_recon_cols_f32(const float *a, const float *t, int32_t n_rows, int32_t n_cols, float w_pos, float w_neg, float *loss,
                        float *col_sum, float *da, ggad_stream_t stream);
/* out[b] = sqrt( sum_c (a[b][c] - t[b][c])^2 ): the per-node anomaly score of test_recon (src/utils.py:158-159). */
int ggad_recon_rows_f32(const float *a, const float *t, int64_t n_rows, int32_t n_cols, float *out, ggad_stream_t stream);

/* One-class hypersphere loss of the full-graph OCGNN comparison model (ocgnn.py:83-118, :180-184) on the rows idx[0..n_idx)
 * of emb (row-major, h columns; idx NULL = all of the first n_idx rows):
 *   score[i] = ||emb[idx[i]] - center||^2 - r^2,   loss = r^2 + (1 / beta) * mean_i max(score[i], 0)
 * center NULL = the origin.  demb (may be NULL): d loss / d emb, written ONLY on the listed rows -- the caller zero-fills the
 * rest; an index listed twice gets one row's gradient, not the sum (the reference's index lists are duplicate-free). */
int ggad_ocgnn_loss_f32(const float *emb, const int64_t *idx, int64_t n_idx, int32_t h, const float *center, float r, float beta,
                        float *loss, float *score, float *demb, ggad_stream_t stream);

/* ---- full-graph AnomalyDAE (model_AnomalyDAE.py:115-300, anomalyDAE.py): GAT layer + fused reconstruction loss ----------------
 * GAT layer = GATConv of torch_geometric 2.1 with the reference's defaults (one head, slope 0.2, stored self loops removed and one
 * self loop added per node, bias).  Edges run from source r to target i where A_hat[r, i] > 0; target i aggregates over row i
 * of A_hat^T (tptr / tcol / tval).  y = h W^T (N x F) comes from ggad_gemm_f32.
 *   ggad_adae_gat_alpha_f32: als[r] = y_r . a_s, ald[r] = y_r . a_d.
 *   ggad_adae_gat_fwd_f32:   z_i = sum_r softmax_r(leaky(als_r + ald_i)) y_r + bias (bias may be NULL); rmax / rsum = the row's
 *                            softmax max and denominator, kept for the backward.
 *   ggad_adae_gat_bwd_f32:   from g = d loss / d z: dals, dald (N each), dy (N x F); dpre = d loss / d pre-activation per edge,
 *                            float[nnz + N] (slot tptr[i] + i + k: entry k of target row i, the added self loop last); tmap[e] =
 *                            index in A_hat^T of entry e of A_hat (aptr / acol / aval).
 *   ggad_adae_colsum_f32:    out[f] = sum_r w[r] M[r, f] (w NULL: 1) in a fixed order; ws = ggad_adae_colsum_workspace_elems(F)
 *                            floats, contents on entry are arbitrary (every row range stores its sum, an empty one its zero).
 * Reconstruction loss on the rows rows[0..n_rows) (int64, duplicate-free) of z (N x F), with rptr / rcol / rval = the compact CSR
 * of A_hat[rows, :]:
 *   attr_i = ||x_i - xhat_i||, stru_i = sqrt(sum_{j<N} (A_ij - sigmoid(z_i . z_j))^2), score_i = 0.5 attr_i + 0.5 stru_i,
 *   loss = mean_i score_i (loss may be NULL: scoring only).  The N x N matrix is never formed; ws = ggad_adae_stru_fwd_workspace_elems
 *   floats, contents on entry are arbitrary;
 *   s_edge (may be NULL): sigmoid(z_i . z_j) per entry of the compact CSR, what the backward reads.
 * ggad_adae_stru_bwd_f32: dz (N x F, every row written) = d loss / d z scaled by *gloss (device float); pos[j] = position of node
 *   j in rows or -1; tptr (N + 1) / trow / tedge = the entries of the compact CSR grouped by column (row position, entry index);
 *   ws = ggad_adae_stru_bwd_workspace_elems floats, contents on entry are arbitrary; F <= 768.
 * ggad_adae_attr_bwd_f32: dxhat rows `rows` = *gloss (0.5 / n_rows) (xhat - x) / attr (other rows untouched). */
int ggad_adae_gat_alpha_f32(const float *y, const float *a_s, const float *a_d, int32_t n, int32_t F, float *als, float *ald,
                            ggad_stream_t stream);
int ggad_adae_gat_fwd_f32(const int32_t *tptr, const int32_t *tcol, const float *tval, const float *y, const float *als,
                          const float *ald, const float *bias, int32_t n, int32_t F, float *z, float *rmax, float *rsum,
                          ggad_stream_t stream);
int ggad_adae_gat_bwd_f32(const int32_t *tptr, const int32_t *tcol, const float *tval, const int32_t *aptr, const int32_t *acol,
                          const float *aval, const int32_t *tmap, const float *y, const float *als, const float *ald,
                          const float *rmax, const float *rsum, const float *a_s, const float *a_d, const float *g, int32_t n,
                          int32_t F, float *dpre, float *dals, float *dald, float *dy, ggad_stream_t stream);
int64_t ggad_adae_colsum_workspace_elems(int32_t F);
int ggad_adae_colsum_f32(const float *M, const float *w, int64_t n, int32_t F, float *out, float *ws, ggad_stream_t stream);
int64_t ggad_adae_stru_fwd_workspace_elems(int32_t n_rows, int32_t n);
int ggad_adae_stru_fwd_f32(const float *z, int32_t n, int32_t F, const int64_t *rows, int32_t n_rows, const int32_t *rptr,
                           const int32_t *rcol, const float *rval, const float *x, const float *xhat, float *ws, float *s_edge,
                           float *attr, float *stru, float *score, float *loss, ggad_stream_t stream);
int64_t ggad_adae_stru_bwd_workspace_elems(int32_t n_rows, int32_t n, int32_t F);
int ggad_adae_stru_bwd_f32(const float *z, int32_t n, int32_t F, const int64_t *rows, int32_t n_rows, const int32_t *rptr,
                           const int32_t *rcol, const float *rval, const float *s_edge, const int32_t *pos, const int32_t *tptr,
                           const int32_t *trow, const int32_t *tedge, const float *stru, const float *gloss, float *ws, float *dz,
                           ggad_stream_t stream);
int ggad_adae_attr_bwd_f32(const float *x, const float *xhat, const int64_t *rows, int32_t n_rows, int32_t F, const float *attr,
                           const float *gloss, float *dxhat, ggad_stream_t stream);

/* ---- full-graph AEGIS (model_AEGIS.py, aegis.py): the batch-norm heads of its two MLPs and its two losses ----------------------
 * ggad_aegis_bn_fwd_f32: BatchNorm1d in training mode over the M = m1 + m2 rows of two row blocks h1 (m1 x C, row stride ld1) and h2
 *   (m2 x C, ld2; m2 = 0: one block), the statistics of their concatenation, fused with act (0 = ReLU, 1 = sigmoid):
 *     y = act(gamma (h - mean) invstd + beta),  invstd = 1 / sqrt(var + eps), var biased;
 *   mean / invstd (C floats each) are written for the backward; running_mean / running_var (unbiased variance, momentum) and the
 *   int64 num_batches_tracked are updated in place (each may be NULL: not updated).  Output rows k = rows[k] of the concatenation
 *   (rows NULL: k < n_out <= M): y (row stride ldy) when w2 is NULL, else the head p[k] = sigmoid(y . w2 + b2) without y.
 *   M < 2 -> GGAD_E_INVALID (torch: more than 1 value per channel); C != ggad_aegis_bn_channels() -> GGAD_E_UNSUPPORTED, nothing
 *   launched.  Rows are 16-byte aligned (strides multiples of 4).  ws = ggad_aegis_bn_workspace_elems(M, C) floats, contents on entry
 *   are arbitrary (here, at ggad_aegis_bn_bwd_f32 and at ggad_aegis_loss_fwd_f32); ticket = one
 *   int32.  Two launches.
 *   TICKET WORDS, here and at every `ticket` / `tickets` parameter of this header: int32 in device memory that count the workgroups
 *   of a launch as they finish (csrc/handoff.h).  They must be ZERO before the first call; every launch leaves them zero, so they
 *   need no clearing between calls; launches that are ordered on one stream (or in one captured chain) may share them, launches
 *   that can run concurrently may not.
 * ggad_aegis_bn_bwd_f32: the backward of one block (h: M x C, ldh) from dy (M x C, lddy) or, with the head (w2 non-NULL), from p and
 *   dp = d loss / d p: dh (lddh), dgamma, dbeta and dw2 (C), db2 (1).  Same refusals, workspace and ticket.  Two launches.
 * ggad_aegis_loss_fwd_f32: loss_g = mean_{i<n} -max(log1p(-p_i), -100) (BCE against 0) and loss_ae = mean_k ||x_r - zd_r||, r =
 *   rows[k] (x: n x F, zd: row stride ldz >= F); attr[k] = ||x_r - zd_r|| is kept for the backward.  One launch; ws =
 *   ggad_aegis_loss_workspace_elems(n, n_rows); ticket as above (TICKET WORDS).
 * ggad_aegis_loss_bwd_f32: dp[i] = *gloss_g p_i / max(p_i (1 - p_i), 1e-12) / n (dp may be NULL) and dzd (n x ldz, every element
 *   written: *gloss_ae (zd - x) / (n_rows attr) on the listed rows (pos[i] = position in rows or -1) below column F, 0 elsewhere;
 *   dzd may be NULL).  One launch. */
int32_t ggad_aegis_bn_channels(void);
int32_t ggad_aegis_bn_groups(int64_t M);
int32_t ggad_aegis_bn_rows_per_group(void);
int64_t ggad_aegis_bn_workspace_elems(int64_t M, int32_t C);
int ggad_aegis_bn_fwd_f32(const float *h1, int64_t m1, int64_t ld1, const float *h2, int64_t m2, int64_t ld2, int32_t C,
                          const float *gamma, const float *beta, float eps, float momentum, float *running_mean, float *running_var,
                          int64_t *num_batches_tracked, int32_t act, const int64_t *rows, int64_t n_out, float *y, int64_t ldy,
                          const float *w2, const float *b2, float *p, float *mean, float *invstd, float *ws, int32_t *ticket,
                          ggad_stream_t stream);
int ggad_aegis_bn_bwd_f32(const float *h, int64_t M, int64_t ldh, int32_t C, const float *gamma, const float *beta, const float *mean,
                          const float *invstd, int32_t act, const float *dy, int64_t lddy, const float *w2, const float *p,
                          const float *dp, float *dh, int64_t lddh, float *dgamma, float *dbeta, float *dw2, float *db2, float *ws,
                          int32_t *ticket, ggad_stream_t stream);
int64_t ggad_aegis_loss_workspace_elems(int64_t n, int64_t n_rows);
int ggad_aegis_loss_fwd_f32(const float *p, int64_t n, const float *x, int32_t F, const float *zd, int64_t ldz, const int64_t *rows,
                            int64_t n_rows, float *attr, float *loss_g, float *loss_ae, float *ws, int32_t *ticket, ggad_stream_t stream);
int ggad_aegis_loss_bwd_f32(const float *p, int64_t n, const float *gloss_g, float *dp, const float *x, int32_t F, const float *zd,
                            int64_t ldz, const int32_t *pos, int64_t n_rows, const float *attr, const float *gloss_ae, float *dzd,
                            ggad_stream_t stream);

/* ---- full-graph GAAN (model_gaan.py, gaan.py): the edge loss over A_hat --------------------------------------------------------
 * The edge set E holds m entries (erow[e], ecol[e]) in the reference's order: the rows of the duplicate-free row list in list order,
 * each with its columns j ascending where (normalize_adj(A) + I)[i, j] > 0.  emb and z are N x C, row-major, 16-byte aligned.
 * ggad_gaan_edge_fwd_f32: a_e = sigmoid(<emb_i, emb_j>) (written to a_out, m floats, for the backward), a'_e = sigmoid(<z_i, z_j>);
 *   loss[1] = mean_e -max(log1p(-a'_e), -100) (BCE against 0), loss[2] = mean_e -max(log(a_e), -100) (BCE against 1),
 *   loss[0] = (loss[1] + loss[2]) / 2.  ws = ggad_gaan_edge_fwd_workspace_elems(m) floats, contents on entry are arbitrary.  Two launches.
 * ggad_gaan_edge_bwd_f32: dE (N x C, every row written) = G emb + G^T emb with G_e = ((*gloss / 2 / m) (a_e - 1) /
 *   max((1 - a_e) a_e, 1e-12)) (1 - a_e) a_e on E.  pos[k] = position of node k in the row list (-1: absent), rptr (n_rows + 1) the
 *   row list's offsets into E; tptr (N + 1) / trow / tedge: the entries (i, k) of E grouped by k, trow = i, tedge = e, ascending e.
 *   small (n_small) and big (n_big) partition the N nodes: a node of `small` has at most ggad_gaan_bwd_small_count() entries on its
 *   row and column sides together.  One launch.
 * Both: C != ggad_gaan_edge_channels() -> GGAD_E_UNSUPPORTED, nothing launched.  No atomics: every sum has a fixed order. */
int32_t ggad_gaan_edge_channels(void);
int32_t ggad_gaan_bwd_small_count(void);
int64_t ggad_gaan_edge_fwd_workspace_elems(int64_t m);
int ggad_gaan_edge_fwd_f32(const float *emb, const float *z, int64_t n, int32_t C, const int32_t *erow, const int32_t *ecol, int64_t m,
                           float *a_out, float *ws, float *loss, ggad_stream_t stream);
int ggad_gaan_edge_bwd_f32(const float *emb, int64_t n, int32_t C, const int32_t *pos, const int32_t *rptr, const int32_t *ecol,
                           const int32_t *tptr, const int32_t *trow, const int32_t *tedge, const float *a, int64_t m, const float *gloss,
                           const int32_t *small, int64_t n_small, const int32_t *big, int64_t n_big, float *dE, ggad_stream_t stream);

/* ---- full-graph DOMINANT (model_domaint.py, dominant.py): the attribute autoencoder x_ = W2 relu(W1 x + b1) + b2 and its loss -----
 * x is N x F row-major; rows (int64) holds the train list (m >= 1 rows) followed by the test list (t_rows >= 0 rows).  W1 is H x F,
 * W2 F x H (nn.Linear weights), b1 (H), b2 (F).  e_r = ||x_r - x_r_hat||.
 * ggad_dominant_ae_f32: one launch: loss[0] = mean of e over the train rows, score[k] = e of test row k, and the gradients at
 *   d loss = 1 (dW1 H x F, dB1 H, dW2 F x H, dB2 F; every element written).  Only the listed rows are evaluated.  (F, H) outside
 *   ggad_dominant_ae_supported -> GGAD_E_UNSUPPORTED, nothing launched.  ws = ggad_dominant_ae_workspace_elems(m, t_rows, F, H)
 *   floats, contents on entry are arbitrary; tickets = ggad_dominant_tickets() int32 (TICKET WORDS above).  Fixed-order sums, no
 *   float atomics.
 * ggad_dominant_recon_f32: one launch from a computed x_ (xh, N x F): loss[0], score as above and dxh (N x F, every element
 *   written) = (xh - x) / (e m) on the train rows (pos[i] = position of node i in the train list, -1 off it), 0 elsewhere.
 *   ws = ggad_dominant_recon_workspace_elems(n, m, t_rows) floats, contents on entry are arbitrary; ticket = one int32 (TICKET WORDS
 *   above).
 * ggad_dominant_scale_f32: dst[i] = src[i] * g[0] for i < n (g in device memory).  One launch. */
int32_t ggad_dominant_ae_supported(int32_t F, int32_t H);
int32_t ggad_dominant_tickets(void);
int64_t ggad_dominant_ae_workspace_elems(int64_t m, int64_t t_rows, int32_t F, int32_t H);
int ggad_dominant_ae_f32(const float *x, int32_t F, const int64_t *rows, int64_t m, int64_t t_rows, const float *W1, const float *b1,
                         const float *W2, const float *b2, int32_t H, float *score, float *loss, float *dW1, float *dB1, float *dW2,
                         float *dB2, float *ws, int32_t *tickets, ggad_stream_t stream);
int64_t ggad_dominant_recon_workspace_elems(int64_t n, int64_t m, int64_t t_rows);
int ggad_dominant_recon_f32(const float *x, const float *xh, int64_t n, int32_t F, const int64_t *rows, int64_t m, int64_t t_rows,
                            const int32_t *pos, float *score, float *loss, float *dxh, float *ws, int32_t *ticket, ggad_stream_t stream);
int ggad_dominant_scale_f32(const float *src, int64_t n, const float *g, float *dst, ggad_stream_t stream);

/* Device-atomic 2-hop stage (fallback of ggad_mb_plan_build, exported for completeness).  One wave per entry for
 * n_entries_cap entries (a host-side upper bound), true count read from *ent_total (= ent_ptr[n_rows]).
 * cnt2[slot][k] += 1 for every k in N(u), u an owner entry: column sums of the U x U2 mask
 * (graphsage.py:335-348; rows are adj_list.get(u) WITHOUT self union). */
int ggad_mb_count2(const int32_t *rowptr, const int32_t *col, const int32_t *ent_col, const int32_t *ent_slot,
                   const int32_t *ent_total, int64_t n_entries_cap, int64_t n_nodes, const int32_t *own1,
                   int32_t *cnt2, ggad_stream_t stream);
/* x2[e] = sum_{k in N(u)} feat[k] / (sqrt(|N(u)|) sqrt(c'_k)) at owner entries.          graphsage.py:346-355 */
int ggad_mb_gather2(const int32_t *rowptr, const int32_t *col, const float *feat, int32_t feat_dim, int32_t feat_stride,
                    const int32_t *ent_col, const int32_t *ent_slot, const int32_t *ent_own, const int32_t *ent_total,
                    int64_t n_entries_cap, int64_t n_nodes, const int32_t *cnt2, float *x2, ggad_stream_t stream);
/* Restore the counter slots to zero by re-walking the chunk (with_hop2 = 0: only cnt1). */
int ggad_mb_plan_reset(const int32_t *rowptr, const int32_t *col, const int32_t *ent_col, const int32_t *ent_slot,
                       const int32_t *ent_own, const int32_t *ent_total, int64_t n_entries_cap, int64_t n_nodes,
                       int32_t *cnt1, int32_t *cnt2, int32_t with_hop2, ggad_stream_t stream);

/* Static per-node table of the LDS-counting 2-hop stage: tile_off[u][t] = offset inside u's sorted CSR row of its first
 * neighbour with id >= t << ggad_mb_ldsw_tile_shift() (t = 0 .. n_tiles): the neighbours of u inside a tile of 32,768 ids are
 * one contiguous piece of its row.  int32 x ggad_mb_tile_offsets_elems(n_nodes, shift), built once per graph. */
int ggad_mb_ldsw_tile_shift(void);
int ggad_mb_ldsw_max_owners(void);          /* entries of a batch one pass of the LDS tables holds (more: walked in slabs) */
int64_t ggad_mb_tile_offsets_elems(int64_t n_nodes, int32_t tile_shift);
int ggad_mb_tile_offsets(const int32_t *rowptr, const int32_t *col, int64_t n_nodes, int32_t tile_shift, int32_t *tile_off,
                         ggad_stream_t stream);
int64_t ggad_mb_ldsw_seg_elems(int64_t n_nodes, int64_t n_entries_cap);     /* ints of seg_t */
/* Tile-major copy of col for the pair counting (reference op: the duplicate counts of src/graphsage.py:335-348): col_t = the ids of
 * every (node, tile) segment, all segments of a tile contiguous in node order; tile_start[u][t] (same shape as tile_off) = where
 * segment (u, t) begins in col_t.  Built once per graph from tile_off; workspace: int32 x ggad_mb_tile_major_workspace_elems. */
int64_t ggad_mb_tile_major_workspace_elems(int64_t n_nodes, int32_t tile_shift);
int ggad_mb_tile_major(const int32_t *rowptr, const int32_t *col, int64_t n_nodes, int32_t tile_shift, const int32_t *tile_off,
                       int32_t *tile_start, int32_t *col_t, int32_t *workspace, ggad_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Mini-batch path: dense step = GCNEncoder.forward + GCN.loss + backward + Adam
 * Replaces src/graphsage.py:395-454 (projection W, neighbour mean, outlier generation fc,
 * permuted concat), :171-258 (score, BCE, cosine-affinity margin, recon, total),
 * autograd backward and torch.optim.Adam.step (src/model_handler.py:363-364).
 *
 * Parameter block `params` (fp32): w[D] | W[D*F] | fc[D*D]  (= state_dict keys `weight`,
 * `enc.weight`, `enc.fc.weight`), followed by kernel-private transposed copies
 * Wt[F*D] | fcT[D*D]; total ggad_mb_param_block_elems(D,F).  Gradients are packed the same
 * way (first D + D*F + D*D elements): this is the buffer the data-parallel layer
 * all-reduces.
 * ---------------------------------------------------------------------------------- */
int64_t ggad_mb_param_count(int32_t D, int32_t F);       /* D + D*F + D*D               */
int64_t ggad_mb_param_block_elems(int32_t D, int32_t F); /* + transposed copies         */
/* Refresh the transposed copies after the host wrote w/W/fc (load_state_dict). */
int ggad_mb_params_sync(float *params, int32_t D, int32_t F, ggad_stream_t stream);

/* One batch = rows [row0, row0+n_rows) and entries [ent0, ent0+n_ents) of the chunk.
 *
 * ggad_mb_project : h2[e-ent0] = relu(W x2[e]) at owner entries (flat over entries).       graphsage.py:419
 * ggad_mb_fwd_rows: nbar = mean over the closed neighbourhood of h2[owner] (:421), h1 = relu(W x1) (:412)
 *                   and, on label-1 rows, the generated outlier gen = relu(fc nbar) (:428-430). */
int ggad_mb_project(const float *params, int32_t D, int32_t F, const float *x2, const int32_t *ent_own, int32_t ent0,
                    int32_t n_ents, float *h2, ggad_stream_t stream);
int ggad_mb_fwd_rows(const float *params, int32_t D, int32_t F, const float *x1, const float *h2, const int32_t *ent_ptr,
                     const int32_t *ent_own, const int32_t *labels, int32_t row0, int32_t n_rows, int32_t ent0, float *h1,
                     float *nbar, float *gen, ggad_stream_t stream);

/* Batch loss (graphsage.py:174,192-258), two launches (one wave per position, then one wave per row).
 * pos_meta[q] = (src << 2) | (src_is_label1 << 1) | label[q], src = row whose embedding sits at column q
 * of `combined_all` (label-0 rows first, generated outliers last, :450); row_pos[row] = column of that row;
 * labels are paired in ORIGINAL order (quirk 1).
 * Outputs: losses8 = {total, cls, margin, rec, 0.1/n1, margin_active, n0, n1}; the per-row backward
 * coefficients dz / coef_a / coef_g (see ggad_mb_row_coefs) of the TOTAL loss; the partial sums of d w in
 * loss_ws (float[ggad_mb_loss_workspace_elems(n_rows)], consumed by ggad_mb_grad_reduce); optionally the raw
 * gradients d_h1 / d_gen / d_nbar (all three or none).  If step_counter is not NULL it is incremented. */
int64_t ggad_mb_loss_workspace_elems(int32_t n_rows);
int ggad_mb_loss(const float *params, int32_t D, int32_t F, const float *h1, const float *nbar, const float *gen,
                 const int32_t *labels, const int32_t *pos_meta, const int32_t *row_pos, const int32_t *ent_ptr,
                 int32_t row0, int32_t n_rows, float *loss_ws, float *losses8, float *d_h1, float *d_gen, float *d_nbar,
                 float *dz, float *coef_a, float *coef_g, int32_t *step_counter, ggad_stream_t stream);

/* Vector-Jacobian product of project + fwd_rows for arbitrary upstream gradients (layered autograd API):
 *   row_coefs: coef_a = d_h1 [h1>0];  dz = d_gen [gen>0];  coef_g = (d_nbar + fc^T dz) / r
 *   bwd_flat : dW partials, flat over the batch's entries and rows, ggad_mb_bwd_parts() blocks of [F][D]. */
int ggad_mb_row_coefs(const float *params, int32_t D, int32_t F, const int32_t *labels, const int32_t *ent_ptr,
                      int32_t row0, int32_t n_rows, const float *h1, const float *gen, const float *d_h1,
                      const float *d_gen, const float *d_nbar, float *dz, float *coef_a, float *coef_g,
                      ggad_stream_t stream);
int ggad_mb_bwd_parts(void);
int ggad_mb_bwd_flat(int32_t D, int32_t F, const float *x1, const float *x2, const float *h2, const int32_t *ent_own,
                     const int32_t *ent_row, int32_t row0, int32_t n_rows, int32_t ent0, int32_t n_ents,
                     const float *coef_a, const float *coef_g, float *dw_part, ggad_stream_t stream);

/* Reduce the partials into the packed gradient buffer grads[D + D*F + D*D] (w | W | fc). */
int ggad_mb_grad_reduce(int32_t D, int32_t F, const int32_t *pos_meta, int32_t row0, int32_t n_rows,
                        const float *losses8, const float *nbar, const float *dw_part, const float *dz,
                        const float *loss_ws, float *grads, ggad_stream_t stream);

/* torch.optim.Adam.step (betas .9/.999, eps 1e-8, L2 weight decay added to the gradient) on the
 * packed block; grad_scale multiplies the gradient first (1/world_size after an all-reduce sum).
 * Step index is read from *step_counter.  Refreshes the transposed copies. */
int ggad_mb_adam(float *params, float *exp_avg, float *exp_avg_sq, const float *grads, int32_t D, int32_t F,
                 float lr, float weight_decay, float grad_scale, const int32_t *step_counter,
                 ggad_stream_t stream);

/* Whole training step of one batch in one host call.  chain 0 (default): fwd_rows_v (h2 = relu(W x2) computed by the
 * row's workgroup, F == 17) or project -> fwd_rows, then loss_pos -> loss_rows -> bwd_flat -> grad_reduce (5 or 6
 * launches); chain 2: always 6; chain 3: the six launches of the wide chain (csrc/step_wide.hip) at any D that
 * ggad_mb_wide_supported takes -- at D > 64 chains 0 and 2 take it too.
 * Adam is fused into the last launch when fuse_adam != 0 (single GPU); with fuse_adam == 0 the caller all-reduces
 * `grads` and then calls ggad_mb_adam.  All members are device pointers. */
typedef struct ggad_mb_step {
  float *params, *exp_avg, *exp_avg_sq, *grads;
  int32_t *step_counter;
  const float *x1, *x2;
  const int32_t *ent_ptr, *ent_own, *ent_row, *labels, *pos_meta, *row_pos;
  float *h1, *nbar, *gen, *dz, *coef_a, *coef_g;
  float *h2, *dw_part, *loss_ws, *losses8;
  int32_t D, F, row0, n_rows, ent0, n_ents;
  float lr, weight_decay;
  int32_t chain;          /* 0 (default): 5 launches when F == 17 and the batch has no hub row (projection fused into the
                             forward-rows kernel, h2 per ENTRY), else 6; 2: always 6; 3: the wide chain (6 launches) */
  int32_t max_row_entries; /* largest closed neighbourhood among the batch rows (host knowledge; 0 = unknown -> 6 launches) */
  /* optional (all four or none): row-piece tables of the PLAN (staging block of ggad_mb_plan_build) and the
   * partial-sum buffer, float[(chunks of the plan) * 64].  With them a chain-0 batch that holds a hub row takes the
   * chunk-parallel forward (k_fwd_chunks + k_loss_pos_ck: 5 launches, h2 not stored, relu mask recomputed in bwd_flat) instead
   * of project -> fwd_rows -> loss_pos (6 launches). */
  const int32_t *row_ck_ptr, *ck_rc, *ck_e0;
  float *chunk_part;
} ggad_mb_step;
/* dw_part must hold ggad_mb_dw_part_elems(n_rows, D, F) floats (one [F][D] partial per row or per bwd_flat part). */
int64_t ggad_mb_dw_part_elems(int32_t n_rows, int32_t D, int32_t F);
int ggad_mb_train_step(const ggad_mb_step *step, int32_t fuse_adam, ggad_stream_t stream);
/* All steps of a chunk in one host call (the reference's per-batch loop, src/model_handler.py:330-364): batch b covers rows
 * [batch_ptr[b], batch_ptr[b+1]) and entries [batch_ent_ptr[b], batch_ent_ptr[b+1]) -- HOST arrays of n_batches + 1
 * offsets --, its largest row has batch_max_row[b] entries (host, may be NULL), its loss record goes to
 * loss_log + 8 * (log_base + b) (device); everything else is taken from *tmpl. */
int ggad_mb_train_chunk(const ggad_mb_step *tmpl, int32_t n_batches, const int32_t *batch_ptr, const int64_t *batch_ent_ptr,
                        const int32_t *batch_max_row, float *loss_log, int32_t log_base, int32_t fuse_adam,
                        ggad_stream_t stream);
/* Data-parallel form: per batch  backward -> exchange(user) -> Adam with grad_scale (1 / world size).  `exchange` is the
 * caller's all-reduce(SUM) of tmpl->grads, enqueued on `stream` (torch.distributed / RCCL); non-zero return aborts. */
int ggad_mb_train_chunk_dp(const ggad_mb_step *tmpl, int32_t n_batches, const int32_t *batch_ptr, const int64_t *batch_ent_ptr,
                           const int32_t *batch_max_row, float *loss_log, int32_t log_base, float grad_scale,
                           int (*exchange)(void *), void *user, ggad_stream_t stream);

/* One-shot gradient exchange of the data-parallel step (the reference is single-device): buffers in
 * fine-grained device memory, one per rank, exported / imported as HIP IPC handles; the kernel of step s writes this rank's
 * 5,248 gradients into every rank's buffer (over xGMI), raises flags, waits for the peers', sums the W blocks in rank order and
 * applies Adam -- one launch, no collective library call, no host callback (exchange.cpp, k_xchg_adam in step.hip).
 * HOST handle; create -> exchange the ggad_xchg_handle_bytes()-byte handles (e.g. all_gather) -> connect.  A wait that times
 * out (a lost peer) sets the error word read by ggad_xchg_error instead of hanging. */
typedef struct ggad_xchg ggad_xchg;
int ggad_xchg_create(int32_t rank, int32_t world, int64_t n_floats, ggad_xchg **out);
int32_t ggad_xchg_handle_bytes(void);
int ggad_xchg_handle(ggad_xchg *xchg, void *handle_host_out);
int ggad_xchg_connect(ggad_xchg *xchg, const void *handles_host);     /* world x handle bytes, rank order */
int ggad_xchg_error(ggad_xchg *xchg, int32_t *err_host);
int ggad_xchg_destroy(ggad_xchg *xchg);
int ggad_xchg_adam(float *params, float *exp_avg, float *exp_avg_sq, const float *grads, int32_t D, int32_t F, float lr,
                   float weight_decay, float grad_scale, const int32_t *step_counter, ggad_xchg *xchg, ggad_stream_t stream);
/* ggad_mb_train_chunk with the exchange: per batch  backward -> (publish, wait, sum in rank order, Adam x grad_scale). */
int ggad_mb_train_chunk_xchg(const ggad_mb_step *tmpl, int32_t n_batches, const int32_t *batch_ptr, const int64_t *batch_ent_ptr,
                             const int32_t *batch_max_row, float *loss_log, int32_t log_base, float grad_scale, ggad_xchg *xchg,
                             ggad_stream_t stream);

/* XCD-resident chunk kernel (csrc/step_xcd.hip): the dense steps of a WHOLE chunk -- the reference's per-batch loop
 * src/model_handler.py:330-364 (GCNEncoder.forward + GCN.loss src/graphsage.py:395-454,171-258, backward, Adam) -- as ONE
 * launch whose workgroups all stay on one XCD (one shared L2): hand-offs between the phases of a step are plain stores + L2-served
 * loads, barriers are tagged-slot all-gathers inside that L2 (0.43 us), nothing is written back or invalidated between steps.
 * The launch has 8 n_wg workgroups (n_wg = 24, 28 or 32, 0 = 32: the compute units of one XCD the stream may use, the same number on each of its four shader engines); the dispatcher
 * deals exactly n_wg to every XCD, the ones on XCD GGAD_XCD_ID (default 0) stay, the rest leave at once.  Results are
 * deterministic and independent of n_wg's placement; if fewer than n_wg workgroups ever reached that XCD the launch times out
 * (error 2) instead of hanging.  Requirements: F == 17, D <= 64, the row-piece tables of the plan
 * (row_ck_ptr / ck_rc / ck_e0 / chunk_part of ggad_mb_step).  batch_ptr_dev: DEVICE int32[n_batches + 1] row offsets (the
 * staging block of ggad_mb_plan_build holds them); max_rows: rows of the largest batch; n_rows / n_pieces / n_entries: totals of
 * the chunk (rows_cap / pieces_cap: what the workspace was sized for); workspace:
 * float[ggad_mb_xcd_workspace_elems(max_rows, D, F, rows_cap, pieces_cap)], 16-byte aligned.  A whole-chip launch first
 * flattens the plan's tables into one 32-byte record per piece / per position (in the workspace) and copies the x2 row of every
 * owner entry to the other entries of its (batch, column) -- x2 is written, at non-owner entries only; xchg NULL = single GPU, else the one-shot exchange runs
 * inside the reduction phase of every step (grad_scale = 1 / world size).  Workgroups have 512 threads and need a compute unit
 * each: the stream must be able to keep n_wg of them resident on that XCD (ggad_mb_xcd_grid() = the largest grid, 8 x 32).
 * ggad_mb_xcd_status: control words of the last launch on `workspace` (synchronises `stream`): out[0] error (0 ok, 1 barrier
 * time-out, 2 registration time-out; GGAD_XCD_TIMEOUT_S seconds, default 10), out[1] workgroups that stayed, out[2] their XCD,
 * out[3..10] (only with GGAD_XCD_DEBUG=4, else 0) wall clocks of rank 0 in 10 ns ticks: phase A, barrier, R, barrier, C, barrier, E, barrier; out[11..18] sub-phase
 * clocks (diagnostics: they are INCLUDED in the phase that follows them). */
int32_t ggad_mb_xcd_grid(void);
/* XCD on which block 0 of a launch on `stream` runs (block b then runs on XCD (first + b) % 8; a constant of the stream's
 * hardware queue, measured by a one-wave probe launch; synchronises the stream). */
int ggad_xcd_first_of_stream(int32_t *first_host, ggad_stream_t stream);
int64_t ggad_mb_xcd_workspace_elems(int32_t max_rows, int32_t D, int32_t F, int64_t rows_cap, int64_t pieces_cap);
int ggad_mb_train_chunk_xcd(const ggad_mb_step *tmpl, int32_t n_batches, const int32_t *batch_ptr_dev, int32_t max_rows,
                            int32_t n_rows, int32_t n_pieces, int32_t n_ents, int64_t rows_cap, int64_t pieces_cap, float *loss_log,
                            int32_t log_base, float *workspace, float grad_scale, ggad_xchg *xchg, int32_t n_wg, const int32_t *records,
                            ggad_stream_t stream);
/* `records` NULL: the launch builds the chunk's records itself, on `stream`.  Otherwise they were built by ggad_mb_xcd_prepare on a
 * stream of the caller's choice (the plan's: a whole-chip pass that does not belong on the chunk kernel's 28 compute units) into
 * int32[ggad_mb_xcd_record_elems(rows_cap, pieces_cap)] owned by the chunk; the caller orders the two launches (stream / event). */
int64_t ggad_mb_xcd_record_elems(int64_t rows_cap, int64_t pieces_cap);
int ggad_mb_xcd_prepare(const ggad_mb_step *tmpl, int32_t n_batches, const int32_t *batch_ptr_dev, int32_t n_rows, int32_t n_pieces,
                        int32_t n_ents, int64_t rows_cap, int64_t pieces_cap, int32_t *records, ggad_stream_t stream);
int ggad_mb_xcd_status(const float *workspace, int64_t *out19, ggad_stream_t stream);
/* out19[0] of ggad_mb_xcd_status is STICKY: the control block is cleared at every launch, the first error code of any launch since the
 * last ggad_mb_xcd_clear_error(workspace, 0, stream) is not (the caller allocates the workspace zeroed).  code != 0 sets the word as a
 * launch that timed out would: the host's recovery path (ggad_amd/trainer.py: restore the entry snapshot, replay on the launch chain)
 * is tested with it.  Synchronises `stream`. */
int ggad_mb_xcd_clear_error(float *workspace, int32_t code, ggad_stream_t stream);

/* Inference embeddings: h[i] = relu(W x1[i])  (GCNEncoder.forward, train_flag False).   graphsage.py:412 */
int ggad_mb_encode(const float *params, int32_t D, int32_t F, const float *x1, int32_t n_rows, float *h,
                   ggad_stream_t stream);

/* Inference: prob[i] = sigmoid(w . relu(W x1[i]))                   graphsage.py:178-181 */
int ggad_mb_score(const float *params, int32_t D, int32_t F, const float *x1, int32_t n_rows, float *prob,
                  ggad_stream_t stream);

/* Streams restricted to a subset of the compute units (bit i of mask = CU i; n_words 32-bit words).  Used to run the
 * chunk plan (chip-filling gathers) and the dense step chain (tiny dependent launches) side by side on disjoint CUs. */
int ggad_stream_create_cu_mask(const uint32_t *mask, int32_t n_words, ggad_stream_t *out);
int ggad_stream_destroy(ggad_stream_t stream);
int ggad_device_cu_count(int32_t device, int32_t *out);

/* ------------------------------------------------------------------------------------
 * Full-graph path (run.py + model.py): sparse products over the edges instead of dense N x N matrices
 * ---------------------------------------------------------------------------------- */

/* C[M x N] = epilogue(A * B), fp32 on the matrix cores (v_mfma_f32_32x32x2_f32, exact f32).
 * A(m,k) = A[m*sam + k*sak], B(k,n) = B[k*sbk + n*sbn]: NN / NT / TN by strides.  Replaces nn.Linear /
 * torch.mm and their autograd (model.py:27,156,176-180).  bias[N] and relu are optional epilogues.
 * workspace: float[ggad_gemm_workspace_elems(M,N,K)] (0 = no split-K needed; may be NULL); contents on entry are arbitrary: every
 * split stores its whole M x N slice before the reduction reads it, a split whose K range is empty (the ranges are rounded up to 32) zeros. */
int64_t ggad_gemm_workspace_elems(int32_t M, int32_t N, int32_t K);
int ggad_gemm_f32(const float *A, const float *B, float *C, int32_t M, int32_t N, int32_t K, int64_t sam, int64_t sak,
                  int64_t sbk, int64_t sbn, int64_t ldc, const float *bias, int32_t relu, float *workspace,
                  ggad_stream_t stream);

/* Which kernel the last ggad_gemm_f32 / ggad_linear_prelu_f32 call of the CALLING THREAD chose (ABI 11): route | variant << 8.  A
 * host-side record written when the call is made (no synchronisation; it says what was launched, not that it has finished); NONE
 * after a call that launched nothing (M or N zero, invalid arguments, GGAD_E_UNSUPPORTED); after GGAD_E_LAUNCH it names the kernel
 * whose launch failed, or NONE.  Variant:
 *   SLAB / BRES            the template instance: K-steps of 16, (K + 15) / 16
 *   WGRAD_TN               GGAD_GEMM_VARIANT_TN(vp, vq): columns per lane of the two operands
 *   DMA / DMA_SPLITK       GGAD_GEMM_VARIANT_DMA(splits, LDS buffers): splits = 1 without split-K
 *   TILED / TILED_SPLITK   GGAD_GEMM_VARIANT_TILED(splits, vec, tm): vec 0 per-float loads, 1 float4 loads, 2 float4 loads with the
 *                          per-float path at the edges; tm = rows of a workgroup tile (64 or 128)
 *   SMALL, NONE            0 */
enum ggad_gemm_route {
  GGAD_GEMM_ROUTE_NONE = 0,
  GGAD_GEMM_ROUTE_SLAB = 1,            /* k_gemm_slab<KSn> */
  GGAD_GEMM_ROUTE_BRES = 2,            /* k_gemm_bres<KSn> */
  GGAD_GEMM_ROUTE_WGRAD_TN = 3,        /* k_mlp_wgrad + k_mlp_wgrad_reduce */
  GGAD_GEMM_ROUTE_SMALL = 4,           /* k_gemm_small */
  GGAD_GEMM_ROUTE_DMA = 5,             /* k_gemm_dma */
  GGAD_GEMM_ROUTE_DMA_SPLITK = 6,      /* k_gemm_dma into the workspace + k_splitk_reduce */
  GGAD_GEMM_ROUTE_TILED = 7,           /* k_gemm_f32 */
  GGAD_GEMM_ROUTE_TILED_SPLITK = 8     /* k_gemm_f32 into the workspace + k_splitk_reduce */
};
#define GGAD_GEMM_ROUTE_PACK(route, variant) ((int32_t)(route) | (int32_t)(variant) << 8)
#define GGAD_GEMM_VARIANT_TN(vp, vq) ((vp) << 4 | (vq))
#define GGAD_GEMM_VARIANT_DMA(splits, bufs) ((splits) | (bufs) << 8)
#define GGAD_GEMM_VARIANT_TILED(splits, vec, tm) ((splits) | (vec) << 8 | (tm) << 10)
int32_t ggad_gemm_last_route(void);

/* out[r] = act( sum_e val[e] * X[col[e]] + bias ) over CSR rows cut into SEGMENTS of <= ggad_spmm_seg_len()
 * consecutive entries [seg_beg, seg_end): one wave per segment, so a hub row never serialises the launch.
 * seg_out[s] >= 0: the row consists of this one segment and is finished in place (output row seg_out[s]);
 * seg_out[s] < 0: the partial sum goes to part[-seg_out[s] - 1][W] and the row is listed in multi_row / multi_first /
 * multi_count (output row, first slot, number of slots), summed in slot order by a second launch; part holds
 * n_seg x W floats, slots are unique and < n_seg.  The order of the segments in the tables is the launch order and is free.
 * The segment tables are built once per matrix (and per row subset) on the host.  part: contents on entry are arbitrary (a slot is read
 * only behind the store of its segment; an EMPTY segment -- a row without entries -- stores its zero sum like any other).
 * act = PReLU with slope *prelu_a if given; out_pre (optional) receives the pre-activation.  W % 4 == 0.
 * Replaces torch.bmm(adj, .) + bias + PReLU (model.py:31-35), adj[0, abn, :] @ emb (model.py:151-155),
 * the column sums of sim * raw_adj (run.py:182-188, as R^T e_hat) and every transposed product in backward. */
int ggad_spmm_seg_len(void);
int ggad_spmm_csr_f32(const int32_t *col, const float *val, const int32_t *seg_beg, const int32_t *seg_end,
                      const int32_t *seg_out, int32_t n_seg, const int32_t *multi_row, const int32_t *multi_first,
                      const int32_t *multi_count, int32_t n_multi, const float *X, int64_t ldx, int32_t W, const float *bias,
                      const float *prelu_a, float *out, int64_t ldo, float *out_pre, float *part, ggad_stream_t stream);

/* Same product for SPARSE neighbourhoods with a wide operand (Reddit / Photo: ~17 entries per row, W = 300; model.py:31 on those
 * configs): a workgroup owns one slice of 40 columns (8 slices at W = 300: one per XCD, whose L2 then holds its slice of X); every
 * row is finished in place by whoever owns it (no partial sums, no second launch): rows of <= ggad_spmm_rowslice_short() entries by one
 * lane group -- ggad_spmm_rowslice_group() = 6 rows per wave, unit_rows / unit_out: int32[n_units x 6] CSR rows and output rows, -1 =
 * empty slot, the caller groups rows of similar length --, rows of <= ggad_spmm_rowslice_long() entries by one wave (long_rows /
 * long_out), longer ones (hubs) by one workgroup (hub_rows / hub_out).  rowptr: the CSR row pointers (DEVICE).  Same epilogue as
 * ggad_spmm_csr_f32; results agree with it to fp32 round-off. */
int32_t ggad_spmm_rowslice_group(void);
int32_t ggad_spmm_rowslice_short(void);
int32_t ggad_spmm_rowslice_long(void);
int ggad_spmm_rowslice_f32(const int32_t *rowptr, const int32_t *col, const float *val, const int32_t *unit_rows,
                           const int32_t *unit_out, int32_t n_units, const int32_t *long_rows, const int32_t *long_out, int32_t n_long,
                           const int32_t *hub_rows, const int32_t *hub_out, int32_t n_hub, const float *X, int64_t ldx, int32_t W,
                           const float *bias, const float *prelu_a, float *out, int64_t ldo, float *out_pre, ggad_stream_t stream);
/* The same product, LINE-granular and persistent, for operands whose rows are 128-byte aligned (X and ldx * 4 multiples of 128: the
 * producers of the path pad their 300-float rows to 320): a slice = one 128-byte line of a row, a wave = 8 rows, line x of all rows on
 * XCD x, the lines beyond the eighth split by rows over the XCDs, a fixed grid whose waves loop over the XCD's items (k_spmm_rowline
 * in fullgraph.hip; model.py:31 on the sparse configs).  ent: int32 x 2 = (column, bits of the fp32 value) per stored entry in CSR
 * order; n_src_rows * ldx * 4 < 2^32.  Tables of int32 x 4 = (first entry, end, output row, 0):
 * unit_tab 8 consecutive slots per unit of short rows (empty slot: 0, 0, -1; rows of <= ggad_spmm_rowslice_short() entries, longest
 * first), long_tab one per medium row (<= ggad_spmm_rowslice_long() entries), hub_tab one per longer row.  256 <= W <= 512. */
int32_t ggad_spmm_rowline_supported(const float *X, int64_t ldx, int32_t W, int64_t n_src_rows);
int ggad_spmm_rowline_f32(const int32_t *ent, const int32_t *unit_tab, int32_t n_units, const int32_t *long_tab, int32_t n_long,
                          const int32_t *hub_tab, int32_t n_hub, const float *X, int64_t ldx, int32_t W, int64_t n_src_rows,
                          const float *bias, const float *prelu_a, float *out, int64_t ldo, float *out_pre, ggad_stream_t stream);
/* ggad_prelu_bwd_f32 with a row stride for dz (ld_dz >= W, multiple of 4): the gradient a following line-granular product reads. */
int ggad_prelu_bwd_ld_f32(const float *g, const float *z, const float *prelu_a, int32_t M, int32_t W, float *dz, int64_t ld_dz, float *db,
                          float *da, float *workspace, ggad_stream_t stream);
/* The same in ONE launch (ABI 10; autograd of `self.act(out)`, /root/reference/model.py:35): two levels of tickets -- the last workgroup
 * of every group of four adds the group's partial column sums, the last group reduces the group rows -- every sum in a fixed order.
 * `workspace`: ggad_prelu_bwd_one_workspace_elems(M, W) floats; `ticket`: ggad_prelu_bwd_one_tickets() int32 in device memory (TICKET
 * WORDS at ggad_aegis_bn_fwd_f32: zero before the first call, left zero, shared only by stream-ordered launches).  Shapes the vector kernel does not take run
 * the two launches.  workspace: contents on entry are arbitrary. */
int64_t ggad_prelu_bwd_one_workspace_elems(int32_t M, int32_t W);
int32_t ggad_prelu_bwd_one_tickets(void);
int ggad_prelu_bwd_one_f32(const float *g, const float *z, const float *prelu_a, int32_t M, int32_t W, float *dz, int64_t ld_dz, float *db,
                           float *da, float *workspace, int32_t *ticket, ggad_stream_t stream);

/* Same product for dense neighbourhoods (hundreds of neighbours per row, X larger than an XCD's 4 MB L2): X is first
 * re-laid slice-major into xs_workspace (ggad_spmm_sliced_workspace_elems(n_src_rows, W) floats; column slices of 32 floats =
 * one cache line per row), then every workgroup gathers ONE slice, chosen by the XCD it runs on, 8 neighbours per load.  n_src_rows = rows of X.  Same
 * segment tables, epilogue and outputs as ggad_spmm_csr_f32; the summation order inside a segment differs (lane groups
 * take every 8th neighbour), so results agree to fp32 round-off, and are deterministic.  xs_workspace and part: contents on entry are
 * arbitrary, and the buffer may be larger than this call needs (one staging buffer serves products of every width and row count: the
 * lanes of a last, partial slice beyond W are written as zeros and never reach an output; nothing behind n_src_rows rows per slice is read). */
int64_t ggad_spmm_sliced_workspace_elems(int64_t n_src_rows, int32_t W);
int ggad_spmm_sliced_seg_len(void); /* recommended segment length of ITS segment tables (any length is accepted, 0 too: a row without entries) */
int ggad_spmm_sliced_f32(const int32_t *col, const float *val, const int32_t *seg_beg, const int32_t *seg_end,
                         const int32_t *seg_out, int32_t n_seg, const int32_t *multi_row, const int32_t *multi_first,
                         const int32_t *multi_count, int32_t n_multi, const float *X, int64_t ldx, int32_t W, int64_t n_src_rows,
                         float *xs_workspace, const float *bias, const float *prelu_a, float *out, int64_t ldo, float *out_pre,
                         float *part, ggad_stream_t stream);

/* Same product (whole matrix, or a row subset of a matrix without separate diagonal) for dense neighbourhoods whose values factor as value[i][j] = row_scale[i] * col_scale[j]
 * off the diagonal (normalize_adj, utils.py:47-54; scales may be NULL = 1) plus an optional diagonal diag[i] (NULL = none,
 * its entries are then part of the stream): out[i] = act(row_scale[i] * sum_j col_scale[j] X[j] + diag[i] X[i] + bias).
 * A workgroup of ggad_spmm_panel_waves() waves owns (32-float column slice, row block) and walks the operand in panels of
 * ggad_spmm_panel_rows() source rows staged in LDS; the entries are a host-built stream of 16-bit panel row indices (layout at
 * k_spmm_panel in fullgraph.hip; built by ggad_amd/csr.py::Csr.panel_plan): wg_tab[n_wg][2] = (slice, block) or (-1, -1),
 * dir[(block * waves + wave) * n_chunks + chunk][8] = {first oct of the wave's tiles of that panel, 8 x 16-bit counts of the QUADS
 * (4 steps) walked per round: whole octs, then half of the last one}, stream = [oct][8 lane groups][8 steps] uint16, two
 * per uint32, + 8 spare octs, row_tab[(block * waves + wave) * rounds + round][8] = output row (| GGAD_SPMM_PANEL_WIDE) or -1.  xs_workspace as for ggad_spmm_sliced_f32.
 * Deterministic; agrees with the other two kernels to fp32 round-off (the scales are applied outside the sum).  xs_workspace: contents on
 * entry are arbitrary; the rows of a last, partial panel behind n_src_rows are never indexed by the stream. */
/* Host half of its plan (csrc/spmm_panel_build.cpp, host pointers, threads; n_threads <= 0: one per core, 32 at most):
 * round_rows[n_rounds][8] = the 8 rows of a round (-1: none); ggad_spmm_panel_count -> steps_rc[round][panel] = entries of the
 * round's longest row in that panel of panel_rows columns; ggad_spmm_panel_fill writes the entry stream: tile (round, panel)
 * starts at oct tile_oct[round][panel], [oct][lane group][step] 16-bit panel row indices (ceil(steps_rc / 8) octs), empty
 * slots = a zero row (panel_rows / panel_rows + 1), spare_octs zero octs after the last tile.  skip_diag: entries col == row
 * are left out (diag[] of ggad_spmm_panel_f32 carries them).  round_wide[round] != 0 (NULL: none): the round is ONE row (slot 0 of
 * round_rows) dealt over all 8 lane groups -- even panel rows to groups 0 1 4 5, odd to 3 2 7 6 -- and its row_tab entries carry
 * GGAD_SPMM_PANEL_WIDE: the kernel adds the 8 accumulators before its epilogue. */
#define GGAD_SPMM_PANEL_WIDE 0x40000000
int ggad_spmm_panel_count(const int64_t *rowptr, const int32_t *col, int32_t n_rounds, const int32_t *round_rows,
                          const int32_t *round_wide, int32_t skip_diag, int32_t panel_rows, int32_t n_panels, int32_t *steps_rc,
                          int32_t n_threads);
int ggad_spmm_panel_fill(const int64_t *rowptr, const int32_t *col, int32_t n_rounds, const int32_t *round_rows,
                         const int32_t *round_wide, int32_t skip_diag, int32_t panel_rows, int32_t n_panels, const int32_t *steps_rc,
                         const int64_t *tile_oct, uint16_t *stream, int64_t total_octs, int32_t spare_octs, int32_t n_threads);
/* 1: every off-diagonal value[i][j] equals (float)(r[i] * r[j]) to a relative rtol; 0: not; < 0: invalid arguments. */
int ggad_spmm_panel_values_factor(const int64_t *rowptr, const int32_t *col, const float *val, const double *r, int32_t n_rows,
                                  double rtol, int32_t n_threads);
/* 1 when the current device can give a workgroup the panel kernel's 159 KB of LDS (queried and opted into once per device), else 0:
 * ggad_spmm_panel_f32 then returns an error and callers keep the sliced kernel. */
int32_t ggad_spmm_panel_available(void);
int32_t ggad_spmm_panel_rows(void);
int32_t ggad_spmm_panel_waves(void);
int32_t ggad_spmm_panel_rounds(void);
int ggad_spmm_panel_f32(const int32_t *wg_tab, int32_t n_wg, const uint32_t *dir, const uint32_t *stream, const int32_t *row_tab,
                        int32_t n_chunks, const float *col_scale, const float *row_scale, const float *diag, const float *X,
                        int64_t ldx, int32_t W, int64_t n_src_rows, float *xs_workspace, const float *bias, const float *prelu_a,
                        float *out, int64_t ldo, float *out_pre, ggad_stream_t stream_);

/* The same product (replaces torch.bmm(adj, .), model.py:31, under the conditions of ggad_spmm_panel_f32) with the operand slice
 * passing through a RING of ggad_spmm_ring_slots() LDS slots of ggad_spmm_ring_slot_rows() source rows: during phase j the
 * ggad_spmm_ring_walkers() walker waves of a workgroup read the slots j .. j + ggad_spmm_ring_window() - 1 while one more wave
 * stages slot j + slots - 1 by LDS-DMA; one barrier per phase.  The entries are a host-built per-walker list of QUADS (4 steps x 8
 * lane groups x 16-bit LDS row index; layout at k_spmm_ring in fullgraph.hip, built by ggad_amd/csr.py::Csr.ring_plan):
 * wg_tab[n_wg][2] = (slice, block) or (-1, -1); wave_sb[block * walkers + wave][2] = {first super-block (4 quads), count};
 * idx = [super-block][2 halves][8 lane groups][2 quads][4 steps] uint16 (+ one spare super-block); ctl = one byte per quad:
 * bits 0..5 = 4 * accumulator slot (< ggad_spmm_ring_rounds()), bit 6 = last quad of its phase (every walker flags every phase);
 * row_tab[(block * walkers + wave) * rounds + slot][8] = output row (| GGAD_SPMM_PANEL_WIDE) or -1; n_phases = ceil(n_src_rows /
 * slot_rows).  Deterministic; agrees with the other SpMM kernels to fp32 round-off.  xs_workspace: as for ggad_spmm_panel_f32 (contents on
 * entry are arbitrary; the last phase stages a partial slot).
 * Host half (csrc/spmm_ring_build.cpp, host pointers, threads): ggad_spmm_ring_count -> quads_rp[round][phase] = quads the round
 * walks in that phase under the flexible schedule (a lane group without open entry in the slot that is overwritten next walks
 * its next entries anywhere in the window); ggad_spmm_ring_fill writes idx given the absolute first quad of every (round, phase)
 * tile (quad_off), n_sb = super-blocks of idx including the spare one.  round_rows / round_wide / skip_diag as for the panel plan. */
int ggad_spmm_ring_count(const int64_t *rowptr, const int32_t *col, int32_t n_rounds, const int32_t *round_rows,
                         const int32_t *round_wide, int32_t skip_diag, int32_t slot_rows, int32_t n_ring_slots, int32_t window,
                         int32_t n_phases, uint16_t *quads_rp, int32_t n_threads);
int ggad_spmm_ring_fill(const int64_t *rowptr, const int32_t *col, int32_t n_rounds, const int32_t *round_rows,
                        const int32_t *round_wide, int32_t skip_diag, int32_t slot_rows, int32_t n_ring_slots, int32_t window,
                        int32_t n_phases, const uint16_t *quads_rp, const int64_t *quad_off, uint16_t *idx, int64_t n_sb,
                        int32_t n_threads);
int32_t ggad_spmm_ring_available(void);
int32_t ggad_spmm_ring_slot_rows(void);
int32_t ggad_spmm_ring_slots(void);
int32_t ggad_spmm_ring_window(void);
int32_t ggad_spmm_ring_walkers(void);
int32_t ggad_spmm_ring_rounds(void);
/* n_walkers (ABI 10): the walker waves per workgroup the plan was dealt to -- ggad_spmm_ring_walkers() (one loader wave: the whole-matrix
 * products) or ggad_spmm_ring_walkers_subset() (three loader waves: products whose walkers have a handful of steps per phase and would wait
 * for a single, issue-bound loader -- the loss-row products of run.py:182-188 and their transposes). */
int32_t ggad_spmm_ring_walkers_subset(void);
int ggad_spmm_ring_f32(const int32_t *wg_tab, int32_t n_wg, const int32_t *wave_sb, const uint16_t *idx, const uint32_t *ctl,
                       const int32_t *row_tab, int32_t n_phases, int32_t n_walkers, const float *col_scale, const float *row_scale,
                       const float *diag, const float *X, int64_t ldx, int32_t W, int64_t n_src_rows, float *xs_workspace,
                       const float *bias, const float *prelu_a, float *out, int64_t ldo, float *out_pre, ggad_stream_t stream_);

/* Fused scorer MLP (model.py:176-180: f_1 = relu(fc1 x), f_2 = relu(fc2 f_1), f_3 = fc3 f_2; Linear weights [out][in], no bias) on
 * the exact-f32 matrix cores, one launch each way instead of three GEMMs forward and five launches for the data gradients backward
 * (SURVEY.md 2.1 F8 / 8b `mlp_score_f32`).  X: R x H (row stride ldx, multiple of 4, 16-byte aligned); W1: H1 x H, W2: H2 x H1,
 * w3: H2.  fwd writes f1 (R x H1), f2 (R x H2) -- the backward's operands -- and f3 (R).  dgrad: dz2 = (g3 w3^T) [f2 > 0] (R x H2),
 * dz1 = (dz2 W2) [f1 > 0] (R x H1), dx = dz1 W1 (+ dx_add, e.g. another gradient of x; NULL = none), row strides ld_dx / ld_add; the
 * weight gradients dz1^T x, dz2^T f1, g3^T f2 stay ggad_gemm_f32 calls (split over the R rows).  ggad_mlp_score_supported: H <= 512
 * and a multiple of 4, H1 <= 256 and even, H2 <= 128 (else callers take the three GEMMs).  Sums run over k in blocks of 16 with
 * a fixed lane-to-k map: deterministic, equal to a k-ordered product to fp32 round-off. */
int32_t ggad_mlp_score_supported(int32_t H, int32_t H1, int32_t H2);
int ggad_mlp_score_fwd_f32(const float *X, int64_t ldx, int32_t R, int32_t H, int32_t H1, int32_t H2, const float *W1, const float *W2,
                           const float *w3, float *f1, float *f2, float *f3, ggad_stream_t stream);
/* The three WEIGHT gradients of the scorer in one launch + one reduction (ABI 7; they were three split-K ggad_gemm_f32 calls):
 *   dW1 (H1 x H) = dz1^T x,  dW2 (H2 x H1) = dz2^T f1,  dW3 (1 x H2) = g3^T f2      over the same R rows.
 * x: R x H with row stride ldx; dz1, f1: R x H1; dz2, f2: R x H2; g3: R -- all contiguous but x.  Outputs contiguous.  workspace:
 * float[ggad_mlp_score_wgrad_workspace_elems(R, H, H1, H2)], 16-byte aligned (partials per row range, added in range order); contents on
 * entry are arbitrary. */
int64_t ggad_mlp_score_wgrad_workspace_elems(int32_t R, int32_t H, int32_t H1, int32_t H2);
int ggad_mlp_score_wgrad_f32(const float *x, int64_t ldx, const float *dz1, const float *f1, const float *dz2, const float *f2, const float *g3,
                             int32_t R, int32_t H, int32_t H1, int32_t H2, float *dW1, float *dW2, float *dW3, float *workspace,
                             ggad_stream_t stream);
int ggad_mlp_score_dgrad_f32(const float *g3, int32_t R, int32_t H, int32_t H1, int32_t H2, const float *f1, const float *f2,
                             const float *W1, const float *W2, const float *w3, float *dz2, float *dz1, float *dx, int64_t ld_dx,
                             const float *dx_add, int64_t ld_add, ggad_stream_t stream);

/* PReLU backward: dz = g * (z > 0 ? 1 : a); db[W] = column sums of dz; *da = sum g * z * [z <= 0].
 * workspace: float[2 * ggad_prelu_bwd_splits(M) * W], contents on entry are arbitrary.  db / da may be NULL. */
int32_t ggad_prelu_bwd_splits(int32_t M);
int ggad_prelu_bwd_f32(const float *g, const float *z, const float *prelu_a, int32_t M, int32_t W, float *dz, float *db,
                       float *da, float *workspace, ggad_stream_t stream);
/* out = PReLU(z) with slope *prelu_a (model.py:35), for a GCN layer whose aggregate is taken from a cache (no SpMM epilogue) */
int ggad_prelu_fwd_f32(const float *z, const float *prelu_a, int64_t n, float *out, ggad_stream_t stream);
/* z = A W^T + bias and out = PReLU(z) in ONE launch (reference model.py:27-35 with A_hat X cached: nn.Linear, bias, PReLU) when the
 * slab GEMM takes the shape (M >= 4096; K % 4 == 0 in 17..32, 49..64 or 241..320; N % 4 == 0; 16-byte aligned rows): GGAD_OK, or
 * GGAD_E_UNSUPPORTED with nothing launched (run ggad_gemm_f32 + ggad_prelu_fwd_f32 instead).  A: M x K (rows lda floats apart),
 * W: N x K (rows ldw apart), z / out: M x N (rows ldz / ldo apart). */
int ggad_linear_prelu_f32(const float *A, int64_t lda, const float *W, int64_t ldw, const float *bias, const float *prelu_a, int32_t M,
                          int32_t N, int32_t K, float *z, int64_t ldz, float *out, int64_t ldo, ggad_stream_t stream);
/* dz = g * [y > 0] */
int ggad_relu_bwd_f32(const float *g, const float *y, int64_t n, float *dz, ggad_stream_t stream);

/* The head of the training forward from `emb` (N x W) on -- model.py:140-182 -- and its backward, the glue between the products:
 *   head_gather    out[p] = X[idx[p]] (+ add[p])                          emb[abn] + noise                       model.py:141-145
 *   head_combine   out = [X[nrm]; con]                                    torch.cat((emb[normal], emb_con))      :159
 *   head_emb_out   out[i] = abn_pos[i] >= 0 ? con[abn_pos[i]] : X[i]      emb[:, abn, :] = emb_con               :182
 *   head_con_grad  dz = [y > 0] (g_con + g_out[abn] + g_tail)             every gradient that reaches emb_con = relu(fc4(.)), :156
 *   head_emb_grad  d emb[i] = [i not in abn] g_out[i] + [i in normal] g_comb[nrm_pos[i]] + [i in abn] g_abn[abn_pos[i]] + sp[i]
 * abn_pos / nrm_pos: position of node i in the (duplicate-free) index list, -1 if absent.  Gradient terms may be null. */
int ggad_head_gather_f32(const float *X, const int32_t *idx, const float *add, int32_t n, int32_t W, float *out, ggad_stream_t stream);
int ggad_head_combine_f32(const float *X, const int32_t *nrm, int32_t n_nrm, const float *con, int32_t n_con, int32_t W, float *out,
                          ggad_stream_t stream);
/* ABI 10: ggad_head_gather_f32 and the emb[normal] rows of ggad_head_combine_f32 in one launch (model.py:141-145,159: both read rows of
 * emb before anything else of the head runs); and emb[:, abn, :] = emb_con IN PLACE as the reference writes it (model.py:182; abn
 * duplicate-free) instead of a second N x H tensor. */
int ggad_head_rows_f32(const float *X, const int32_t *abn, const float *add, int32_t n_abn, const int32_t *nrm, int32_t n_nrm, int32_t W,
                       float *out_abn, float *out_comb, ggad_stream_t stream);
int ggad_head_emb_put_f32(const float *con, const int32_t *abn, int32_t n_abn, int32_t W, float *X, ggad_stream_t stream);
int ggad_head_emb_out_f32(const float *X, const int32_t *abn_pos, const float *con, int32_t n, int32_t W, float *out,
                          ggad_stream_t stream);
int ggad_head_con_grad_f32(const float *g_con, const float *g_out, const int32_t *abn, const float *g_tail, const float *y, int32_t n,
                           int32_t W, float *dz, ggad_stream_t stream);
int ggad_head_emb_grad_f32(const float *g_out, const int32_t *abn_pos, const int32_t *nrm_pos, const float *g_comb, const float *g_abn,
                           const float *sp, int32_t n, int32_t W, float *out, ggad_stream_t stream);

/* Row L2 normalisation e_hat = e / |e| with 1/0 -> 0 (run.py:177-180) and its vector-Jacobian product. */
int ggad_rownorm_f32(const float *X, int32_t M, int32_t W, float *inv, float *Xn, ggad_stream_t stream);
int ggad_rownorm_bwd_f32(const float *Xn, const float *inv, const float *dXn, int32_t M, int32_t W, float *dX,
                         ggad_stream_t stream);
/* out[e] = || X[row(e)] - X[col[e]] ||_2 per stored entry of a CSR matrix (TAM calc_distance, utils_tam.py:190-199) */
int ggad_edge_dist_f32(const int32_t *rowptr, const int32_t *col, const float *X, int32_t n_rows, int32_t W, float *out,
                       ggad_stream_t stream);
/* out[p] = scale[p] * <A[sel[p]], B[p]>   (affinity_j = r_inv_j <e_hat_j, (R^T e_hat)_j>, run.py:188) */
int ggad_rowdot_f32(const float *A, const int32_t *sel, const float *B, int32_t n, int32_t W, const float *scale, float *out,
                    ggad_stream_t stream);
/* scatter_add = 0: out[p] = coef[p] * X[sel[p]];  1: out[sel[p]] += coef[p] * X[p]  (sel must be duplicate-free) */
int ggad_rows_scale_f32(const float *X, const int32_t *sel, const float *coef, int32_t n, int32_t W, int32_t scatter_add,
                        float *out, ggad_stream_t stream);

/* The scalar part of the loss block of run.py:165-210 and its gradients: logits[L], aff[L] (L = n_normal + n_out,
 * normal_idx entries first), emb_con / emb_abn (n_out x H).  losses4 = {total, margin, bce, rec};
 * d_logits[L]; g_aff[L] = d total / d aff; dD = d total / d (emb_con - emb_abn). */
int64_t ggad_full_loss_workspace_elems(int32_t n_out, int32_t H);   /* floats of `workspace` (partial column sums of the recon term); contents on entry are arbitrary */
int ggad_full_loss_f32(const float *logits, const float *aff, int32_t n_normal, int32_t n_out, const float *emb_con,
                       const float *emb_abn, int32_t H, float margin, float *losses4, float *d_logits, float *g_aff,
                       float *dD, float *workspace, ggad_stream_t stream);
/* Backward of the loss block, every product with the incoming d total (a device scalar) in one launch:
 *   c = g_aff r_inv_J g (what ggad_rows_scale_f32 needs next), d logits = d_logits g, d emb_con = dD g, d emb_abnormal = -dD g. */
int ggad_full_loss_bwd_scale_f32(const float *g_total, const float *g_aff, const float *r_inv_j, const float *d_logits, const float *dD,
                                 int32_t L, int64_t n_rec, float *c, float *dl, float *d_con, float *d_abn, ggad_stream_t stream);

/* Round 6 (ABI 10): the same loss block (run.py:165-210, reference file /root/reference/run.py) with its row-local parts fused --
 * forward: affinity row dots r_inv_J <e_hat[J], S>, the partial column sums of the recon term and, in the last workgroup to finish, BCE,
 * margin, recon, the four loss values and the coefficients (replaces ggad_rowdot_f32 + ggad_full_loss_f32: four launches);
 * backward: c, d logits, xc = c e_hat[J], d emb_con = g (con - abn) kcol, d emb_abnormal = -that (replaces ggad_full_loss_bwd_scale_f32 +
 * ggad_rows_scale_f32);  ggad_rownorm_bwd_add_f32 = ggad_rownorm_bwd_f32 with dXn[r] += c[q] S[q] for r = J[q] folded in (pos_n / pos_a:
 * position of row r in the normal / abnormal segment of J, or -1).  `ticket`: one int32 (TICKET WORDS at ggad_aegis_bn_fwd_f32);
 * `workspace`: ggad_full_loss_fused_workspace_elems floats, contents on entry are arbitrary. */
int64_t ggad_full_loss_fused_workspace_elems(int32_t n_out, int32_t H);
int ggad_full_loss_fused_f32(const float *e_hat, const int32_t *J, const float *S, const float *r_inv_j, int32_t n_normal, int32_t n_out,
                             int32_t H, const float *logits, const float *emb_con, const float *emb_abn, float margin, float *aff,
                             float *kcol, float *losses4, float *d_logits, float *g_aff, float *workspace, int32_t *ticket,
                             ggad_stream_t stream);
int ggad_full_loss_bwd_fused_f32(const float *g_total, const float *g_aff, const float *r_inv_j, const float *d_logits, const float *e_hat,
                                 const int32_t *J, int32_t L, int32_t H, const float *emb_con, const float *emb_abn, const float *kcol,
                                 int32_t n_out, float *c, float *dl, float *xc, float *d_con, float *d_abn, ggad_stream_t stream);
int ggad_rownorm_bwd_add_f32(const float *Xn, const float *inv, const float *dXn, const int32_t *pos_n, const int32_t *pos_a,
                             const float *c, const float *S, int32_t M, int32_t W, float *dX, ggad_stream_t stream);

/* torch.optim.Adam.step on a flat fp32 block; uses step index *step_counter + 1 and (bump_after != 0) advances it. */
int ggad_adam_f32(float *params, float *exp_avg, float *exp_avg_sq, const float *grads, int64_t n, float lr,
                  float weight_decay, int32_t *step_counter, int32_t bump_after, ggad_stream_t stream);
/* The same update (bump_after = 1) for up to ggad_adam_multi_max() tensors: HOST arrays of device pointers / element counts; one step
 * counter per tensor (torch keeps `step` per parameter; parameters without a gradient are left out).  `tickets` (ABI 10; optional):
 * ggad_adam_multi_max() int32 in device memory, zero before the first call and left zero -- the step counters then advance inside the
 * one launch (the last workgroup of a tensor does it); NULL: a second, trailing launch advances them. */
int32_t ggad_adam_multi_max(void);
int ggad_adam_multi_f32(int32_t n_tensors, float *const *params, float *const *exp_avg, float *const *exp_avg_sq,
                        const float *const *grads, const int64_t *n_elems, int32_t *const *step_counters, float lr,
                        float weight_decay, int32_t *tickets, ggad_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Host-side sampler: bit-exact CPython random.shuffle (MT19937 + getrandbits rejection),
 * replaces the python shuffles inside the reference's timed loop
 * (src/model_handler.py:314,341; 28 ms / batch there).  HOST pointers.
 * ---------------------------------------------------------------------------------- */
typedef struct ggad_mt19937 ggad_mt19937;
ggad_mt19937 *ggad_mt_new(void);
void ggad_mt_free(ggad_mt19937 *);
/* random.seed(int) for 0 <= seed < 2^64 (init_by_array over the 32-bit limbs). */
int ggad_mt_seed_u64(ggad_mt19937 *, uint64_t seed);
/* state exchange with random.getstate()[1]: 624 words + index. */
int ggad_mt_set_state(ggad_mt19937 *, const uint32_t *mt624_host, int32_t index);
int ggad_mt_get_state(const ggad_mt19937 *, uint32_t *mt624_host, int32_t *index_host);
/* random.shuffle(list) in place on an int64 array. */
int ggad_mt_shuffle_i64(ggad_mt19937 *, int64_t *data_host, int64_t n);
uint32_t ggad_mt_getrandbits32(ggad_mt19937 *);
/* The two halves of random.shuffle for callers that pipeline them: (1) consume the generator -> targets_out[c] = swap partner
 * of position n - 1 - c (int32[n + 16], data-independent); (2) apply recorded swaps to a list. */
int ggad_mt_shuffle_targets(ggad_mt19937 *, int64_t n, int32_t *targets_host_out);
int ggad_apply_swaps_i64(int64_t *data_host, int64_t n, const int32_t *targets_host);
/* `count` consecutive batches of the reference's stream (src/model_handler.py:310-345: random.shuffle(train) at every
 * epoch start, random.shuffle(pool) before every batch, batch = train[i0:i1] ++ pool[:n_pseudo]) in one call, the
 * generator walk running one shuffle ahead of the swaps in a helper thread.  HOST pointers; train / pool are shuffled in
 * place exactly as the per-shuffle calls would; *in_epoch_io = index of the next batch in its epoch (>= batches_per_epoch:
 * shuffle train first).  out_nodes: count x (batch_size + n_pseudo), out_len[count]. */
int ggad_sched_batches(ggad_mt19937 *, int64_t *train, int64_t n_train, int64_t *pool, int64_t n_pool, int32_t batch_size,
                       int32_t n_pseudo, int32_t batches_per_epoch, int32_t *in_epoch_io, int32_t count, int64_t *out_nodes,
                       int32_t *out_len);
/* Iteration order of the python set built by adding keys[0..n) one by one: strictly ascending, non-negative int32 keys (an int
 * hashes to itself); out holds n ints.  Restated from the set-table rules (sampler.cpp); anything else -> GGAD_E_INVALID. */
int ggad_pyset_order_i32(const int32_t *keys_host, int64_t n, int32_t *out_host);
/* Neighbour sampling of the GraphSAGE baseline (`random.sample(tuple(adj[v]), k)` per row, reference src/graphsage.py:75-78) over a
 * host CSR whose rows are strictly ascending -- the sets the set path samples from are filled in that order.  For each of the n_rows
 * ids of `nodes`, in list order: a row of degree >= k draws a sample, a shorter row is taken whole and consumes no generator output;
 * a node listed twice is sampled twice.  nbr_out: n_rows x k int32, each row sorted ascending and padded with -1; cnt_out: the row
 * lengths.  setsize: 21, plus 4 ** ceil(log(3k, 4)) when k > 5, evaluated by the caller.  The stream depends only on the order of
 * the rows, not on how they are cut into calls.  Ids outside [0, n_nodes), an unsorted row, k < 1: GGAD_E_INVALID before any draw. */
int ggad_mt_sample_rows(ggad_mt19937 *, const int32_t *rowptr_host, const int32_t *col_host, int64_t n_nodes,
                        const int64_t *nodes_host, int64_t n_rows, int32_t k, int32_t setsize, int32_t *nbr_out, int32_t *cnt_out);
/* One epoch of the GraphSAGE device path's schedule in one call, on one generator: random.shuffle(train), then for each of
 * num_batches batches random.shuffle(pool), nodes = train[i0:i1] ++ pool[:n_pseudo] (i0 = b * batch_size, i1 = min(i0 + batch_size,
 * n_train); a pool shorter than n_pseudo is taken whole) and the sample table of those rows drawn as ggad_mt_sample_rows draws it.
 * Batch b is written at table_out + b * stride (stride >= b_max * (3 + k) ints, b_max = batch_size + n_pseudo): nodes[b_max],
 * cnt[b_max], labels[b_max] (labels_host[node], n_nodes int64), nbr[b_max * k]; rows past len_out[b] hold 0 / 0 / 0 / -1.  train and
 * pool end up shuffled in place and the generator where the per-call path leaves them.  Refused with GGAD_E_INVALID before the
 * first draw, generator and arrays untouched: an id outside [0, n_nodes) in train or pool, k < 1, an unsorted CSR row of such an id,
 * a batch of zero rows.  checked != 0: the caller states that an earlier call on the same graph and the same two arrays returned
 * GGAD_OK -- a shuffle moves ids without changing them -- and the two O(n_train + n_pool) scans are skipped. */
int ggad_sage_sched_epoch(ggad_mt19937 *, int64_t *train, int64_t n_train, int64_t *pool, int64_t n_pool, int32_t batch_size,
                          int32_t n_pseudo, int32_t num_batches, const int32_t *rowptr_host, const int32_t *col_host, int64_t n_nodes,
                          const int64_t *labels_host, int32_t k, int32_t setsize, int32_t checked, int32_t *table_out, int64_t stride,
                          int32_t *len_out);

/* ------------------------------------------------------------------------------------
 * torch.randn's CPU stream continued on the DEVICE (rng.hip).  `state`: ggad_mt_state_words() uint32 in device memory -- the 624
 * MT19937 words of torch's CPU generator, then at [624] the number of words of that block already consumed (0..624; 624: the next
 * draw regenerates the block first, which is also what a freshly seeded generator asks for).  One call is what
 * `torch.randn(n) * scale + shift` (float32, n >= 16) computes on the host: it advances `state` in place by n words, or n + 16 when
 * n % 16 != 0 (torch redraws the last 16 outputs), and writes out[i] = normal_i * scale + shift, product and sum rounded
 * separately.  Values agree with the host's to float32 rounding of log / sin / cos, not bit for bit; the state is exact.  Everything
 * stays on the device: a captured launch draws fresh values at every replay.  `scratch`: ggad_mt_randn_scratch_elems(n) uint32
 * (the raw words; contents on entry are arbitrary).  n < 16 (a different algorithm in torch) or a null pointer -> GGAD_E_INVALID, nothing launched.
 * ---------------------------------------------------------------------------------- */
int32_t ggad_mt_state_words(void);
int64_t ggad_mt_randn_scratch_elems(int64_t n);
int ggad_mt_randn_f32(uint32_t *state, float *out, int64_t n, float scale, float shift, uint32_t *scratch, ggad_stream_t stream);

/* ------------------------------------------------------------------------------------
 * PC-GNN comparison model from a CSR relation graph in device memory (pcgnn.hip; reference src/layers.py:62-153,179-244).
 * rowptr / col: int32 CSR of n_nodes rows, every row non-empty, sorted and duplicate-free, every column in [0, n_nodes) (the
 * caller checks once).  batch: n_batch int32 node ids on the device; a node listed twice is two rows.  cap: capacity in rows of
 * every |U|-sized buffer, min(n_nodes, sum of the batch rows' degrees) -- known on the host; |U| itself stays on the device in
 * n_unique[0].  No entry point uses floating-point atomics: equal inputs give equal bits.
 *
 * ggad_pcgnn_plan   U = union of the batch rows in ASCENDING id order: unique[p] (cap ints, -1 past |U|), pos[v] = p for v in U,
 *                   row_count[p] = |N(unique[p])| (0 past |U|), cnt[v] = |{u in U : v in N(u)}|.  scan: ggad_pcgnn_scan_elems(n_nodes)
 *                   ints, all zero on entry and all-zero again on return (the bitmap part).  pos (n_nodes ints, all -1) and cnt
 *                   (n_nodes ints, all 0) are put back by ggad_pcgnn_plan_reset, which walks the same rows.
 * ggad_pcgnn_hop_f32  a[r] = sum over the entries v of CSR row rows[r] of w * feat[v], t[r] = relu(a[r] W) for r < cap; W is
 *                   (feat_dim, embed_dim) row-major.  cnt NULL: w = 1 / |row| (the mean), every one of the cap rows is read.
 *                   cnt given: w = (1 / sqrt |row|) / sqrt cnt[v] in float32, and rows at or past n_rows[0] are written as zeros.
 *                   ggad_pcgnn_supported(feat_dim, embed_dim) = 0: GGAD_E_UNSUPPORTED, nothing launched.
 * ggad_pcgnn_nb_fwd_f32  nb[i] = sum over u in N(batch[i]) of t2[pos[u]] / |N(batch[i])|.
 * ggad_pcgnn_nb_bwd_f32  dz2[p] = [t2[p] > 0] * sum over the i with unique[p] in N(batch[i]), ascending, of dnb[i] / |N(batch[i])|
 *                   for p < |U|, zeros for the other rows up to cap: the transpose of nb_fwd through relu.
 * ---------------------------------------------------------------------------------- */
int32_t ggad_pcgnn_supported(int32_t feat_dim, int32_t embed_dim);
int32_t ggad_pcgnn_max_feat_dim(void);
int64_t ggad_pcgnn_scan_elems(int64_t n_nodes);
int ggad_pcgnn_plan(const int32_t *rowptr, const int32_t *col, int64_t n_nodes, const int32_t *batch, int32_t n_batch, int32_t cap,
                    int32_t *scan, int32_t *pos, int32_t *cnt, int32_t *unique, int32_t *row_count, int32_t *n_unique,
                    ggad_stream_t stream);
int ggad_pcgnn_plan_reset(const int32_t *rowptr, const int32_t *col, int32_t *unique, const int32_t *n_unique, int32_t cap,
                          int32_t *pos, int32_t *cnt, ggad_stream_t stream);
int ggad_pcgnn_hop_f32(const float *feat, int32_t feat_dim, const int32_t *rowptr, const int32_t *col, const int32_t *rows,
                       const int32_t *n_rows, int32_t cap, const int32_t *cnt, const float *w, int32_t embed_dim, float *a, float *t,
                       ggad_stream_t stream);
int ggad_pcgnn_nb_fwd_f32(const float *t2, int32_t embed_dim, const int32_t *rowptr, const int32_t *col, const int32_t *batch,
                          int32_t n_batch, const int32_t *pos, float *nb, ggad_stream_t stream);
int ggad_pcgnn_nb_bwd_f32(const float *dnb, const float *t2, int32_t embed_dim, const int32_t *rowptr, const int32_t *col,
                          const int32_t *batch, int32_t n_batch, const int32_t *unique, const int32_t *n_unique, int32_t cap,
                          float *dz2, ggad_stream_t stream);

/* ------------------------------------------------------------------------------------
 * GraphSAGE comparison model (reference src/graphsage.py:19-154), one optimiser step on a sampled batch (sage.hip).
 * feat: n_nodes x feat_dim table; nodes: n_batch int32 ids; nbr: n_batch x k int32 sample table (ggad_mt_sample_rows; entries at
 * or past cnt[i] are never read); w_enc: embed_dim x 2 feat_dim; w_cls: 2 x embed_dim; labels: n_batch int32 in {0, 1} or NULL.
 *
 * ggad_sage_fwd_f32  combined[i] = [feat[nodes[i]] || sum_j feat[nbr[i][j]] * (1 / cnt[i])] (table order, one fused multiply-add per
 *                    term; cnt[i] = 0 gives 0 * (1 / 0) = NaN in the second half, as ggad_seg_mean does), emb = relu(combined
 *                    w_enc^T), scores = emb w_cls^T.  With labels: loss (1 + n_batch floats) gets the mean cross entropy over the
 *                    batch in loss[0] (lane l of one wave adds rows l, l + 64, ...; the lanes are added in butterfly order) and the
 *                    rows' own cross entropies behind it, dscores = (softmax - onehot) / n_batch; without: both may be NULL.
 * ggad_sage_bwd_f32  d_cls = dscores^T emb, dZ = (dscores w_cls) * [emb > 0], d_enc = dZ^T combined.  Partial sums over
 *                    ggad_sage_bwd_parts() row ranges go to `ws` (ggad_sage_bwd_workspace_elems floats) and are added in range order.
 * No floating-point atomics: equal inputs give equal bits.  ggad_sage_supported(feat_dim, embed_dim, n_classes): 1 <= feat_dim <= 64,
 * 1 <= embed_dim <= ggad_max_embed_dim(), n_classes == 2; anything else is GGAD_E_UNSUPPORTED and nothing is launched.  The caller
 * range-checks the node ids.
 * ---------------------------------------------------------------------------------- */
int32_t ggad_sage_supported(int32_t feat_dim, int32_t embed_dim, int32_t n_classes);
int32_t ggad_sage_bwd_parts(void);
int64_t ggad_sage_bwd_workspace_elems(int32_t feat_dim, int32_t embed_dim);
int ggad_sage_fwd_f32(const float *feat, int32_t feat_dim, const int32_t *nodes, const int32_t *nbr, const int32_t *cnt,
                      int32_t n_batch, int32_t k, const float *w_enc, int32_t embed_dim, const float *w_cls, const int32_t *labels,
                      float *combined, float *emb, float *scores, float *loss, float *dscores, ggad_stream_t stream);
int ggad_sage_bwd_f32(const float *combined, const float *emb, const float *dscores, const float *w_cls, int32_t n_batch,
                      int32_t feat_dim, int32_t embed_dim, float *ws, float *d_enc, float *d_cls, ggad_stream_t stream);
/* The tail of a step in one launch of one workgroup: d_enc / d_cls = the ggad_sage_bwd_parts() partial sums of `ws` added in range
 * order (what ggad_sage_bwd_f32 leaves in its outputs), torch's Adam on both tensors with the arithmetic of ggad_adam_multi_f32 -- in
 * place on the weights, the moments and the two int32 step counters, which are read first and both advanced by one -- and
 * loss_out[0] = the mean of the n_batch row losses in the order of ggad_sage_fwd_f32's loss[0].  No floating-point atomics, no
 * tickets.  ws must hold what k_sage_bwd_part wrote for the same widths. */
int ggad_sage_sum_adam_f32(const float *ws, const float *rowloss, int32_t n_batch, int32_t feat_dim, int32_t embed_dim, float *w_enc,
                           float *m_enc, float *v_enc, int32_t *ctr_enc, float *w_cls, float *m_cls, float *v_cls, int32_t *ctr_cls,
                           float lr, float weight_decay, float *loss_out, ggad_stream_t stream);
/* n_steps optimiser steps enqueued on one stream with no host work between them: per step the forward and the partial backward of
 * ggad_sage_fwd_f32 / ggad_sage_bwd_f32 on the step's slice of an epoch table (the layout of ggad_sage_sched_epoch: step s at
 * table + s * stride, len_host[s] rows, 1 <= len_host[s] <= b_max), then ggad_sage_sum_adam_f32 with loss_log + s.  combined
 * (b_max x 2 feat_dim), emb (b_max x embed_dim), scores and dscores (b_max x 2), rowloss (b_max) and ws are shared by the steps.
 * len_host is read on the HOST while enqueueing: under a stream capture the row counts become constants of the graph. */
int ggad_sage_epoch_f32(const float *feat, int32_t feat_dim, const int32_t *table, int64_t stride, const int32_t *len_host,
                        int32_t n_steps, int32_t b_max, int32_t k, int32_t embed_dim, float *w_enc, float *m_enc, float *v_enc,
                        int32_t *ctr_enc, float *w_cls, float *m_cls, float *v_cls, int32_t *ctr_cls, float lr, float weight_decay,
                        float *combined, float *emb, float *scores, float *rowloss, float *dscores, float *ws, float *loss_log,
                        ggad_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Head and loss of the PC-GNN comparison model behind its relation kernels (pcgnn_head.hip; reference src/layers.py:125-153,
 * src/model.py:25-48).  t1_r / nb_r: the batch embedding and the neighbourhood mean of relation r, n_batch x embed_dim each, rows
 * embed_dim apart; w: 3 embed_dim x embed_dim (InterAgg.weight); w_cls: 2 x embed_dim (PCALayer.weight); labels: n_batch int64 in
 * {0, 1}.
 *   combined = relu([t1_0 t1_1 t1_2] w), neigh = relu([nb_0 nb_1 nb_2] w), affinity_i = <combined_i / |combined_i|, neigh_i / |neigh_i|>
 *   (a row of norm 0 counts as a row of zeros), scores = combined w_cls^T (n_batch x 2),
 *   loss[1] = max(0, 1 - (a0 - a1)) with a0 / a1 the mean affinity of the label-0 / label-1 rows, loss[0] = mean cross entropy of
 *   scores + 5 loss[1].  A batch without a row of one label has a 0 / 0 mean: both entries of loss are NaN, the hinge passes no
 *   gradient and the cross-entropy gradients stay finite, as torch's autograd gives for the reference's expressions.
 * loss NULL: forward only -- scores and affinity are the only stores; labels, ws and every d_* pointer may be NULL.
 * loss given: also the gradients of loss[0]: d_t1_r / d_nb_r (n_batch x embed_dim), d_w (as w), d_cls (as w_cls); ws holds
 * ggad_pcgnn_head_workspace_elems(n_batch, embed_dim) floats and needs no initialisation.  The weight gradients are summed over
 * ggad_pcgnn_head_parts() row ranges in range order; no floating-point atomics anywhere: equal inputs give equal bits.
 * ggad_pcgnn_head_supported(n_batch, embed_dim): n_batch >= 1 and 1 <= embed_dim <= ggad_max_embed_dim(); anything else is
 * GGAD_E_UNSUPPORTED and nothing is launched.
 * ---------------------------------------------------------------------------------- */
int32_t ggad_pcgnn_head_supported(int32_t n_batch, int32_t embed_dim);
int32_t ggad_pcgnn_head_parts(void);
int64_t ggad_pcgnn_head_workspace_elems(int32_t n_batch, int32_t embed_dim);
int ggad_pcgnn_head_f32(const float *t1_0, const float *t1_1, const float *t1_2, const float *nb_0, const float *nb_1, const float *nb_2,
                        const float *w, const float *w_cls, const int64_t *labels, int32_t n_batch, int32_t embed_dim, float *scores,
                        float *affinity, float *loss, float *d_t1_0, float *d_t1_1, float *d_t1_2, float *d_nb_0, float *d_nb_1,
                        float *d_nb_2, float *d_w, float *d_cls, float *ws, ggad_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Mini-batch AEGIS comparison model (reference src/graphsage_aegis.py:167-173, 298-323), the discriminator step on the two 1-hop
 * aggregates of a batch (aegis_mb.hip).  x_feat / x_noise: total_rows x feat_dim tables; batch i owns rows
 * [batch_ptr[i], batch_ptr[i + 1]) of both (B_i rows, 2 <= B_i <= ggad_aegis_mb_max_rows(); a batch outside that is left alone).
 * Parameters: w_enc (64 x feat_dim), w0 (64 x 64), b0, gamma, beta (64), w1 (64), b1 (1).
 *
 * ggad_aegis_mb_fwd_f32   one workgroup per batch.  E = relu([x_feat; x_noise] w_enc^T), H = E w0^T + b0; call 1 over the 2B rows
 *                         and call 2 over the B noise rows: batch statistics (two-pass), sigmoid(BN(H)), p = sigmoid(. w1 + b1).
 *                         mode 0: p_all (2 total_rows floats: batch i at 2 batch_ptr[i], real rows then noise rows), p_gen (total_rows),
 *                         losses (2 per batch: loss_dis, loss_g), stats (256 per batch: mu, unbiased var, mu', unbiased var').
 *                         mode 1: also what the backward reads -- scratch (ggad_aegis_mb_scratch_elems floats, row-indexed like
 *                         p_all) and inv_std (128 per batch).  mode 2: scores only -- p_all gets total_rows floats, the real rows'
 *                         p at their table row; p_gen and losses may be NULL; stats as before.
 * ggad_aegis_mb_bwd_f32   one workgroup, the batch batch_ptr[0 .. 1] (pass batch_ptr + i, stats + 256 i, inv_std + 128 i): the seven
 *                         gradients of loss_dis + loss_g.  Overwrites the scratch of that batch.
 * ggad_aegis_mb_fold_f32  running <- momentum * batch + (1 - momentum) * running for call 1 then call 2 of every batch, in batch
 *                         order; num_batches_tracked (int64, may be NULL) += 2 n_batches.
 * No floating-point atomics, no allocation, no synchronisation: equal inputs give equal bits, eager or replayed.
 * ggad_aegis_mb_supported(feat_dim, embed_dim, max_rows): 1 <= feat_dim <= 64, embed_dim == 64, 2 <= max_rows <=
 * ggad_aegis_mb_max_rows(); anything else is GGAD_E_UNSUPPORTED and nothing is launched.
 * ---------------------------------------------------------------------------------- */
int32_t ggad_aegis_mb_max_rows(void);
int32_t ggad_aegis_mb_supported(int32_t feat_dim, int32_t embed_dim, int32_t max_rows);
int64_t ggad_aegis_mb_scratch_elems(int64_t total_rows);
int ggad_aegis_mb_fwd_f32(const float *x_feat, const float *x_noise, const int32_t *batch_ptr, int32_t n_batches, int32_t total_rows,
                          int32_t max_rows, int32_t feat_dim, int32_t embed_dim, const float *w_enc, const float *w0, const float *b0,
                          const float *gamma, const float *beta, const float *w1, const float *b1, int32_t mode, float *p_all,
                          float *p_gen, float *losses, float *stats, float *scratch, float *inv_std, ggad_stream_t stream);
int ggad_aegis_mb_bwd_f32(const float *x_feat, const float *x_noise, const int32_t *batch_ptr, int32_t total_rows, int32_t max_rows,
                          int32_t feat_dim, int32_t embed_dim, const float *w0, const float *gamma, const float *beta, const float *w1,
                          const float *p_all, const float *p_gen, const float *stats, float *scratch, const float *inv_std,
                          float *d_w_enc, float *d_w0, float *d_b0, float *d_gamma, float *d_beta, float *d_w1, float *d_b1,
                          ggad_stream_t stream);
int ggad_aegis_mb_fold_f32(const float *stats, int32_t n_batches, float momentum, float *running_mean, float *running_var,
                           int64_t *num_batches_tracked, ggad_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Mini-batch DOMINANT / AnomalyDAE comparison models (reference src/graphsage_dominant.py:154-158, 274-276; recon_mb.hip).
 * x1 / target: total_rows x feat_dim tables (the 1-hop aggregate of the plan and the batch rows of the feature table);
 * w_enc (64 x feat_dim), w_fc (feat_dim x 64).  h = relu(x1 w_enc^T), r = relu(h w_fc^T).
 *
 * ggad_recon_mb_steps_f32   n_steps consecutive optimiser steps in ONE launch of ONE workgroup; step s takes the rows
 *                           [batch_ptr[s], batch_ptr[s + 1]) (device int32, ragged batches allowed, 1 <= B_s <= max_rows, the largest
 *                           batch as the host knows it): loss_s = mean_c sqrt(sum_b w(r_bc) (r_bc - t_bc)^2), w = w_pos where r > 0 else
 *                           w_neg, into losses[s]; backward (the ReLU backward selects); Adam with L2 weight decay on w_enc and w_fc,
 *                           the arithmetic of ggad_adam_multi_f32.  Weights and moments are read once and written back once; both step
 *                           counters advance by n_steps.  g_enc / g_fc (may be NULL) receive the LAST step's raw gradients (before
 *                           weight decay).  A batch outside its table or above max_rows is no step: its loss is NaN and the counters do
 *                           not count it.  Fixed summation order, independent of n_steps; no floating-point atomics.
 * ggad_recon_mb_scores_f32  out[b] = sqrt(sum_c (r_bc - t_bc)^2) for every row (test_recon's score); h and r never reach memory.
 * ggad_recon_mb_supported(feat_dim, embed_dim, max_rows): 1 <= feat_dim <= 64, embed_dim == 64, 1 <= max_rows <=
 * ggad_recon_mb_max_rows(feat_dim) (256 up to feat_dim 32, 158 at 64; 0 for a feat_dim outside); anything else is GGAD_E_INVALID
 * and nothing is launched.
 * ---------------------------------------------------------------------------------- */
int32_t ggad_recon_mb_max_rows(int32_t feat_dim);
int32_t ggad_recon_mb_supported(int32_t feat_dim, int32_t embed_dim, int32_t max_rows);
int ggad_recon_mb_steps_f32(const float *x1, const float *target, const int32_t *batch_ptr, int32_t n_steps, int32_t total_rows,
                            int32_t max_rows, int32_t feat_dim, int32_t embed_dim, float *w_enc, float *w_fc, float *m_enc, float *v_enc,
                            float *m_fc, float *v_fc, int32_t *ctr_enc, int32_t *ctr_fc, float lr, float weight_decay, float w_pos,
                            float w_neg, float *losses, float *g_enc, float *g_fc, ggad_stream_t stream);
int ggad_recon_mb_scores_f32(const float *x1, const float *target, int64_t n_rows, int32_t feat_dim, int32_t embed_dim, const float *w_enc,
                             const float *w_fc, float *out, ggad_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Affinity head and loss of the full-graph TAM comparison model (tam.hip; reference tam.py:113-146).  (rowptr, col, val): the CSR of
 * the raw adjacency R over n nodes, which must be symmetric in pattern and values (the backward relies on it); emb: n x h, row-major;
 * r_inv: 1 / column sum of R (inf -> 0); cnt[i]: how often node i occurs in the list of labelled normal nodes (float), k_total = sum cnt.
 *
 *   a_i = r_inv_i <e_hat_i, sum_j v_ij e_hat_j>,  e_hat_i = e_i / |e_i| (zero rows -> 0);   lo = min a, hi = max a;
 *   loss = -(S - k_total lo) / (hi - lo),  S = sum_i cnt_i a_i;   m_i = (a_i - lo) / (hi - lo)   (no guard for hi = lo)
 *
 * ggad_tam_head_fwd_f32  writes a (n), inv (n: 1 / |e_i|), scal = (loss, lo, hi, n_lo, n_hi, S, 0, 0) with n_lo / n_hi the numbers of
 *                        ties at lo / hi, and, if m is not NULL, m (n).  Three launches, four with m.
 * ggad_tam_head_bwd_f32  d_emb (n x h, every element written) = *g * d loss / d emb from the a, scal and inv of the forward call on
 *                        the same emb; ties at lo / hi share their gradient evenly like torch.min / torch.max.  Two launches.
 * Rows with more than ggad_tam_head_hub_len() stored entries are hubs, summed in pieces of that many entries and the pieces added
 * in piece order: hub_rows (n_hub, ascending) must list exactly those rows and hub_piece_ptr (n_hub + 1, starting at 0) the
 * prefix sums of their piece counts ceil(len / hub_len), n_pieces its last value (both may be NULL with n_hub = 0).
 * workspace: ggad_tam_head_workspace_elems(n, h, n_hub, n_pieces) floats, ZERO before the first call (it holds the ticket words,
 * which the kernels leave zero).  No floating-point atomics: equal inputs give equal bits.
 * ggad_tam_head_supported(n, h): n >= 1 and 1 <= h <= ggad_tam_head_max_dim() (256); any other h is GGAD_E_UNSUPPORTED and nothing
 * is launched.
 * ---------------------------------------------------------------------------------- */
int32_t ggad_tam_head_max_dim(void);
int32_t ggad_tam_head_hub_len(void);
int32_t ggad_tam_head_supported(int32_t n, int32_t h);
int64_t ggad_tam_head_workspace_elems(int32_t n, int32_t h, int32_t n_hub, int32_t n_pieces);
int ggad_tam_head_fwd_f32(const int32_t *rowptr, const int32_t *col, const float *val, const float *emb, const float *r_inv,
                          const float *cnt, float k_total, int32_t n, int32_t h, const int32_t *hub_rows, const int32_t *hub_piece_ptr,
                          int32_t n_hub, int32_t n_pieces, float *a, float *scal, float *m, float *inv, float *workspace,
                          ggad_stream_t stream);
int ggad_tam_head_bwd_f32(const int32_t *rowptr, const int32_t *col, const float *val, const float *emb, const float *r_inv,
                          const float *cnt, float k_total, int32_t n, int32_t h, const int32_t *hub_rows, const int32_t *hub_piece_ptr,
                          int32_t n_hub, int32_t n_pieces, const float *a, const float *scal, const float *inv, const float *g,
                          float *d_emb, float *workspace, ggad_stream_t stream);

/* ------------------------------------------------------------------------------------
 * TAM's truncation round on the device (tam_nsgt.hip; reference utils_tam.py:222-240 and :45-53).  (rowptr, col): the CSR of
 * raw = A + I over n nodes, columns sorted inside a row, nnz = rowptr[n] < 2^31 entries, SYMMETRIC pattern; dis: one distance per
 * entry; alive: one byte per entry, non-zero = the entry is in the current graph.  Every launch goes on `stream`; no floating-point
 * atomics; one wave walks one row.
 *
 * ggad_tam_nsgt_transpose_map  tpos[e] = position of entry (j, i) for entry e = (i, j).  *status (device word, zeroed by the call)
 *                              is 0 afterwards if every entry has its mirror; bit 0: some entry has none, bit 1: a column is
 *                              outside [0, n).  tpos of such an entry is e itself, so tpos always stays inside [0, nnz).
 * ggad_tam_nsgt_rowstat        per row over the live entries: cnt = their number, mx = the largest dis (-inf for a row without
 *                              live entries; a NaN distance is ignored), nzcnt = the number with dis != 0.
 * ggad_tam_nsgt_compact        out_rowptr (n + 1) = exclusive scan of counts (n), out_rowptr[n] = their sum, then per row in
 *                              ascending column order:  mode 0: out_val = dis of the live entries with dis != 0 (counts = nzcnt;
 *                              r and out_col may be NULL);  mode 1: out_col = the columns of the live entries, out_val = r[i] * r[j]
 *                              as one rounded fp32 product (counts = cnt).  out_col / out_val hold sum(counts) elements; a row
 *                              never writes at or past out_rowptr[i + 1].  workspace: ggad_scan_workspace_elems(n) int32.
 * ggad_tam_nsgt_cut            keep[e] = alive[e] && !(dis[e] > thr[row of e]), then alive[e] = keep[e] | keep[tpos[e]] (an entry
 *                              survives if either direction does).  Two launches; keep: nnz bytes of scratch, not alive itself.
 * ---------------------------------------------------------------------------------- */
int ggad_tam_nsgt_transpose_map(const int32_t *rowptr, const int32_t *col, int32_t n, int32_t *tpos, int32_t *status,
                                ggad_stream_t stream);
int ggad_tam_nsgt_rowstat(const int32_t *rowptr, const float *dis, const uint8_t *alive, int32_t n, int32_t *cnt, float *mx,
                          int32_t *nzcnt, ggad_stream_t stream);
int ggad_tam_nsgt_compact(const int32_t *rowptr, const int32_t *col, const float *dis, const uint8_t *alive, int32_t n, int32_t mode,
                          const int32_t *counts, const float *r, int32_t *out_rowptr, int32_t *out_col, float *out_val,
                          int32_t *workspace, ggad_stream_t stream);
int ggad_tam_nsgt_cut(const int32_t *rowptr, const float *dis, const int32_t *tpos, const float *thr, int32_t n, int64_t nnz,
                      uint8_t *alive, uint8_t *keep, ggad_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Rank metrics of a binary classifier (rank_metrics.hip): AUROC, average precision and the confusion counts of `score >= thres`
 * from n float32 scores and n uint8 labels (0 / 1), with scikit-learn's definitions (distinct thresholds, tied scores) as exact
 * counts: only the positives are sorted (one workgroup, in LDS), every negative is bucketed against them by binary search into
 * integer histograms.  Four launches on `stream`, no host synchronisation, no floating-point atomics; n <= INT32_MAX.
 *
 * out8 (device, 8 doubles) = {auroc, ap, tp, fp, fn, tn, n_pos, status}; status 0 ok, 1 one class only (auroc NaN; ap 0.0 without
 * positives), 2 n_pos above ggad_rank_metrics_max_pos() (the counts are valid, auroc / ap NaN), 3 a NaN score, 4 a label other
 * than 0/1.  workspace: ggad_rank_metrics_workspace_elems(n) int32 elements, no preparation needed: the workspace is cleared by the
 * launches themselves, so the call is capturable and replayable.
 * ---------------------------------------------------------------------------------- */
int32_t ggad_rank_metrics_max_pos(void);
int64_t ggad_rank_metrics_workspace_elems(int64_t n);          /* int32 elements */
int ggad_rank_metrics_f32(const float *score, const uint8_t *label, int64_t n, float thres, double *out8, int32_t *workspace,
                          ggad_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Exact, deterministic top-k of n float32 scores (topk.hip).  Ranking: score descending; equal scores by ascending position in the
 * input; -0.0 ties with +0.0; +-inf are ordinary values.  With m = min(k, n): out_pos[0..m) the positions of the top m in that order,
 * out_score[j] their scores bit for bit, out_cumpos[j] (may be NULL) the number of label-1 elements among ranks 0..j (label may be
 * NULL: all 0); entries m..k) hold pos -1, score 0, cumpos out_cumpos[m-1] (0 when m = 0).  out_meta (device, 4 int64) = {m, status,
 * P = label-1 elements among all n, elements that tie with rank m-1's score and were left out}; status 0 ok, 3 a NaN score, 4 a label
 * other than 0/1 (the other outputs are then unspecified): the codes of ggad_rank_metrics_f32.
 *
 * 1 <= k <= ggad_topk_max_k() (16,384: the pairs of one workgroup's sort in LDS), 0 <= n <= INT32_MAX; outside: GGAD_E_INVALID and no
 * launch.  Six launches on `stream`, no host synchronisation, integer atomics only, nothing that waits on another workgroup; equal
 * inputs give equal bits.  workspace: ggad_topk_workspace_elems(n, k) int32 elements (0 = refused), no preparation needed: every word
 * a launch reads was written by an earlier launch of the same call, so the call is capturable and replayable.
 * ---------------------------------------------------------------------------------- */
int32_t ggad_topk_max_k(void);
int64_t ggad_topk_workspace_elems(int64_t n, int32_t k);       /* int32 elements; 0 = refused */
int ggad_topk_f32(const float *score, const uint8_t *label, int64_t n, int32_t k, int32_t *out_pos, float *out_score,
                  int32_t *out_cumpos, int64_t *out_meta, int32_t *workspace, ggad_stream_t stream);

/* ------------------------------------------------------------------------------------
 * ggad_topk_f32 above 16,384 ranks, up to ggad_topk_wide_max_k() = 4,194,304 (2^22: one call ranks every node of DGraph-Fin)
 * (topk.hip, behind the same select stage).  Same arguments and same outputs: out_pos int32[k], out_score float32[k], out_cumpos int32[k] or NULL, out_meta
 * int64[4] with the same four words and status codes; entries m..k) are padded as the narrow call pads them (pos -1, score 0, cumpos of
 * the last rank).  The ranking is the same one, and for every k <= ggad_topk_max_k() every output holds the same bits as
 * ggad_topk_f32's.  The select stage is the narrow call's (five launches); the m candidates are then sorted in runs of 2,048 64-bit
 * words (one workgroup each, 16 KB of static LDS), merged by rank in ceil(log2(ceil(m / 2048))) passes between two word buffers,
 * emitted one thread per output slot, and the labels along the ranking are prefix-summed per block of 1,024 ranks behind a fixed-order
 * sum of the blocks before.
 *
 * 1 <= k <= ggad_topk_wide_max_k(), 0 <= n <= INT32_MAX; outside: GGAD_E_INVALID and no launch.  8 + ceil(log2(ceil(m / 2048)))
 * launches on `stream` (19 at the cap), no host synchronisation, no floating-point atomics, no workgroup waits on another; equal inputs
 * give equal bits.  workspace: ggad_topk_wide_workspace_elems(n, k) int32 elements (0 = refused; the narrow call's, two buffers of m
 * 64-bit words and one count per 1,024 ranks: 96 MB at the cap), 8-byte aligned, no preparation needed: every word a launch reads was
 * written by the host or by an earlier launch of the same call, so the call is captured and replayed as one linear chain.
 * ---------------------------------------------------------------------------------- */
int32_t ggad_topk_wide_max_k(void);
int64_t ggad_topk_wide_workspace_elems(int64_t n, int32_t k);  /* int32 elements; 0 = refused */
int ggad_topk_wide_f32(const float *score, const uint8_t *label, int64_t n, int32_t k, int32_t *out_pos, float *out_score,
                       int32_t *out_cumpos, int64_t *out_meta, int32_t *workspace, ggad_stream_t stream);

/* ------------------------------------------------------------------------------------
 * The rank metrics of ggad_rank_metrics_f32 for up to ggad_rank_wide_max_pos() = 1,048,576 positives (rank_metrics.hip): the same
 * formulas, the same out8 and the same status codes.  The positives are sorted in runs of 2,048 (one workgroup each, in LDS) and
 * merged in ceil(log2(runs)) passes; every negative is bucketed against the one tile of 8,192 sorted keys whose range holds it; the
 * sums are made per tile and added in a fixed order.  `pos_cap` is the caller's upper bound on the positives (what k is to ggad_topk_f32): the
 * workspace and every grid follow from (n, pos_cap) alone, so equal inputs give equal bits.  Status 2 = more positives than
 * pos_cap (the counts are valid, auroc / ap NaN).
 *
 * 0 <= n <= INT32_MAX, 1 <= pos_cap <= ggad_rank_wide_max_pos(); outside: GGAD_E_INVALID and no launch.  5 + ceil(log2(ceil(
 * min(pos_cap, n) / 2048))) launches on `stream`, no host synchronisation, integer atomics only, nothing that waits on another
 * workgroup.  workspace: ggad_rank_wide_workspace_elems(n, pos_cap) int32 elements (0 = refused), 16-byte aligned, no preparation
 * needed: every word a launch reads was written by an earlier launch of the same call, so the call is capturable and replayable.
 * ---------------------------------------------------------------------------------- */
int32_t ggad_rank_wide_max_pos(void);
int64_t ggad_rank_wide_workspace_elems(int64_t n, int64_t pos_cap);   /* int32 elements; 0 = refused */
int ggad_rank_wide_f32(const float *score, const uint8_t *label, int64_t n, int64_t pos_cap, float thres, double *out8,
                       int32_t *workspace, ggad_stream_t stream);

/* ------------------------------------------------------------------------------------
 * The operating point of a score: the alert threshold that is best under a criterion, with its exact confusion counts
 * (rank_metrics.hip).  The front is ggad_rank_wide_f32's (scan, sorted runs, merge passes, tile bucket); the last two launches also
 * form, for every run of equal positives pos[s..e], tp = P - s and fp = Nn - L (L = the negatives strictly below it), and take the
 * arg-max.  The distinct positive scores are the complete candidate set: a threshold between two of them only adds false positives
 * to the next positive score above it.  +-0.0 count as one score.
 *
 * criterion (ggad_rank_operating_criteria() = 5 of them), with fn = P - tp and tn = Nn - fp:
 *   0 f1         maximise 2tp / (2tp + fp + fn)                                    compared cross-multiplied in int64 (< 2^54)
 *   1 f1_macro   maximise 0.5 (f1 + 2tn / (2tn + fn + fp)), a zero denominator = 0  compared in float64, each class F1 ONE division
 *   2 gmean      maximise tp tn (reported: sqrt(tp tn / (P Nn)))                    compared in int64 (< 2^51)
 *   3 precision  the greatest recall with (double)tp >= param (double)(tp + fp)     reported: tp / P
 *   4 fpr        the greatest recall with (double)fp <= param (double)Nn            reported: tp / P
 * Equal criterion values: the HIGHER threshold (fewer alerts).  The order of candidates is total, the reduction (per thread, a
 * tree over the workgroup, a tree over the tiles) fixed: equal inputs give equal bits.  param is ignored for 0..2 and must lie in
 * [0, 1] for 3 and 4.
 *
 * out16: [0..7] the eight doubles ggad_rank_wide_f32(score, label, n, pos_cap, thres, ...) writes, bit for bit; [8] the chosen
 * threshold, a positive's float32 score widened (a zero of either sign); [9..12] tp, fp, fn, tn of score >= [8]; [13] the
 * criterion's value; [14] the number of distinct positive scores; [15] status: 0 = chosen, 5 = no candidate meets the constraint
 * ([8] = +inf, tp = fp = 0, fn = P, tn = Nn, [13] = 0), or [7] when [7] != 0 ([8..14] NaN).
 * curve_thres / curve_tp / curve_fp: all NULL, or all pos_cap long; entry j < P = threshold, tp, fp of the run that holds the j-th
 * highest positive (descending, equal inside a tie run, nothing compacted); entries from P on are left untouched.
 *
 * Limits, alignment and workspace rule of ggad_rank_wide_f32 (0 <= n <= INT32_MAX, 1 <= pos_cap <= ggad_rank_wide_max_pos(), 16-byte
 * aligned workspace of ggad_rank_operating_workspace_elems(n, pos_cap) int32 elements, 0 = refused, no preparation needed); outside
 * them, or with an unknown criterion, a param outside [0, 1] (or NaN) for 3 and 4, or one or two curve pointers: GGAD_E_INVALID and
 * no launch.  The same number of launches on `stream`, no host synchronisation, no floating-point atomics, nothing that waits on
 * another workgroup; every word a launch reads was written by an earlier launch of the same call: capturable and replayable.
 * ---------------------------------------------------------------------------------- */
int32_t ggad_rank_operating_criteria(void);
int64_t ggad_rank_operating_workspace_elems(int64_t n, int64_t pos_cap);   /* int32 elements; 0 = refused */
int ggad_rank_operating_f32(const float *score, const uint8_t *label, int64_t n, int64_t pos_cap, float thres, int32_t criterion,
                            double param, double *out16, float *curve_thres, int32_t *curve_tp, int32_t *curve_fp,
                            int32_t *workspace, ggad_stream_t stream);

/* ------------------------------------------------------------------------------------
 * DeLong's variance of the AUROC, and the paired comparison of two score lists on the same labels (rank_metrics.hip).  The front is
 * ggad_rank_wide_f32's.  With m = P positives, n = Nn negatives, +-0.0 one score, and the doubled placements
 *   a_i = 2 #{neg < x_i} + #{neg == x_i} per positive      b_j = 2 #{pos > y_j} + #{pos == y_j} per negative
 * the sums S1 = sum a = sum b (the AUROC numerator), S2 = sum a^2, T2 = sum b^2, N10 = m S2 - S1^2, N01 = n T2 - S1^2 are exact
 * integers (128-bit accumulators: m S2 passes 64 bits at 1.7 M scores) and
 *   var = N10 / (4 n^2 m^2 (m - 1)) + N01 / (4 m^2 n^2 (n - 1)),
 * each numerator converted to float64 once.  For two lists A and B, by element, C10 = sum_i a_i^A a_i^B, C01 = sum_j b_j^A b_j^B,
 *   cov      = (m C10 - S1A S1B) / (4 n^2 m^2 (m - 1)) + (n C01 - S1A S1B) / (4 m^2 n^2 (n - 1))
 *   ND10     = m (S2A + S2B - 2 C10) - (S1A - S1B)^2,  ND01 = n (T2A + T2B - 2 C01) - (S1A - S1B)^2
 *   var_diff = ND10 / (4 n^2 m^2 (m - 1)) + ND01 / (4 m^2 n^2 (n - 1))      (never var_a + var_b - 2 cov in floating point)
 *
 * ggad_rank_delong_f32.  out16: [0..7] the eight doubles of ggad_rank_wide_f32 for the same arguments, bit for bit; [8] var; [9],
 * [10] its positive-side and negative-side terms; [11] sqrt(var); [12..14] 0.0; [15] status.  sums (12 int64): lo, hi limbs of S1,
 * S2, T2, N10, N01, then two zeros.  Status: [7] when [7] != 0 ([8..14] NaN, sums all zero); 6 = fewer than two positives or two
 * negatives, both classes present (the AUROC words and sums valid, [8..11] NaN); else 0 (a variance of exactly 0 included).
 *
 * ggad_rank_delong_pair_f32.  out24: [0..7] A's out8, [8..15] B's; [16] var_a, [17] var_b, [18] cov, [19] var_diff, [20] auroc_a -
 * auroc_b as (S1A - S1B) / (2 m n), [21] z = [20] / sqrt([19]), [22] 0.0, [23] status.  sums (24 int64): limbs of S1A, S1B, S2A, S2B,
 * C10, T2A, T2B, C01, ND10, ND01, then zeros.  Status: the first non-zero of [7], [15] ([16..22] NaN, sums all zero); else 6 as
 * above ([16..21] NaN); else 7 when ND10 == ND01 == 0 (the two lists induce the same placements: z NaN, the rest valid); else 0.
 *
 * Limits, alignment and workspace rule of ggad_rank_wide_f32, with ggad_rank_delong_workspace_elems / _pair_workspace_elems(n,
 * pos_cap) int32 elements (0 = refused); outside them, or with a NULL pointer: GGAD_E_INVALID and no launch.  The single call has
 * ggad_rank_wide_f32's number of launches; the pair runs the front and the terms kernel twice, one cross kernel over the n elements
 * and one final.  No host synchronisation, no floating-point atomics, nothing that waits on another workgroup; every
 * word a launch reads was written by an earlier launch of the same call: capturable and replayable.  Integer sums: equal inputs give
 * equal bits on any grid.
 * ---------------------------------------------------------------------------------- */
int64_t ggad_rank_delong_workspace_elems(int64_t n, int64_t pos_cap);        /* int32 elements; 0 = refused */
int64_t ggad_rank_delong_pair_workspace_elems(int64_t n, int64_t pos_cap);   /* int32 elements; 0 = refused */
int ggad_rank_delong_f32(const float *score, const uint8_t *label, int64_t n, int64_t pos_cap, float thres, double *out16,
                         int64_t *sums, int32_t *workspace, ggad_stream_t stream);
int ggad_rank_delong_pair_f32(const float *score_a, const float *score_b, const uint8_t *label, int64_t n, int64_t pos_cap,
                              float thres, double *out24, int64_t *sums, int32_t *workspace, ggad_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Stratified bootstrap of average precision and AUROC (rank_metrics.hip).  The front and the first eight doubles are
 * ggad_rank_wide_f32's; one more launch makes `reps` replicates, one workgroup each, from the sorted keys of the P positives and the
 * two histograms alone (histU[b]: negatives with exactly b positives at or below them; histE[k]: those of bin k + 1 that tie the run
 * of equal positives ending at k).  Replicate r draws, with Philox4x32-10 (Random123) under key (seed & 0xffffffff, seed >> 32) and
 * counter (j & 0xffffffff, j >> 32, r, stream) -- call j gives draws 2j and 2j + 1 as x = c0 | c1 << 32 and c2 | c3 << 32, a draw
 * over m outcomes is u = (x * m) >> 64 --
 *   stream 0: P draws over m = P, w[u] += 1 (u a sorted rank);
 *   stream 1: Nn draws over m = Nn; with cum the inclusive prefix of histU, b = #{cum <= u}: cU[b] += 1, and cE[b - 1] += 1 when
 *             b >= 1 and u - cum[b - 1] < histE[b - 1];
 * and with L*_k the prefix of cU through k, [s, e] the run of equal keys that holds k and TP*_k = w[s] + ... + w[P - 1]
 *   rep_ap[r]      = (1 / P) sum_k w_k TP*_k / (TP*_k + Nn - L*_k)   (w_k = 0 adds nothing; consecutive ranks per thread, then a tree)
 *   rep_auc_num[r] = sum_k w_k (2 L*_k + cE[e])                      (exact; AUROC* = rep_auc_num[r] / (2 P Nn))
 * The bootstrap is stratified (P and Nn are those of the list in every replicate).  out16: [0..7] ggad_rank_wide_f32's out8 for the
 * same arguments, bit for bit; [8] reps, [9] P, [10] Nn, [11..14] 0.0, [15] status: [7] when [7] != 0; 8 = fewer than two
 * positives or two negatives; 9 = more positives than ggad_rank_bootstrap_max_pos() = 9216 (the replicate's four histograms of
 * P + 1 ints live in one CU's LDS: an error, there is no second route); else 0.  With a status other than 0 every rep_ap is NaN,
 * every rep_auc_num 0.  hist_out: NULL, or reps rows of 3 (pos_cap + 1) int32 that receive w, cU and cE of every replicate at
 * offsets 0, pos_cap + 1 and 2 (pos_cap + 1), zero beyond entry P (for tests).
 * Limits, alignment and workspace rule of ggad_rank_wide_f32 (ggad_rank_bootstrap_workspace_elems(n, pos_cap) int32 elements, 0 =
 * refused); outside them, with reps outside 1 .. ggad_rank_bootstrap_max_reps() = 4096, or with a NULL pointer other than
 * hist_out: GGAD_E_INVALID and no launch.  No host synchronisation, LDS integer atomics only, every word a launch reads was
 * written by an earlier launch of the same call: capturable and replayable; equal arguments give equal bits.
 * ---------------------------------------------------------------------------------- */
int32_t ggad_rank_bootstrap_max_pos(void);
int32_t ggad_rank_bootstrap_max_reps(void);
int64_t ggad_rank_bootstrap_workspace_elems(int64_t n, int64_t pos_cap);     /* int32 elements; 0 = refused */
int ggad_rank_bootstrap_f32(const float *score, const uint8_t *label, int64_t n, int64_t pos_cap, float thres, uint64_t seed,
                            int32_t reps, double *out16, double *rep_ap, int64_t *rep_auc_num, int32_t *hist_out, int32_t *workspace,
                            ggad_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Paired stratified bootstrap of two models' average precision and AUROC on the same labels (rank_metrics.hip).  The run-merge chain
 * runs twice, into two halves of the workspace (out24[0..7] A's out8, [8..15] B's: ggad_rank_wide_f32's bits for the same
 * arguments); one launch then stores, per element, where it falls under either model, and one more makes `reps` replicates, one
 * workgroup each.  The scheme.  Positive number j is the j-th element with label 1 in POSITION order, negative number u the u-th
 * with label 0: position order, not key order, makes an element the same thing under both models.  Replicate r draws P positive
 * numbers on Philox stream 0 (m = P) and Nn negative numbers on stream 1 (m = Nn); generator, key, counter layout and draw rule are
 * ggad_rank_bootstrap_f32's (above: call j gives draws 2j and 2j + 1, a draw over m outcomes is (x * m) >> 64).  For each model M,
 * with pos_M its sorted positive keys,
 *   w_M[rank_M(j)] += 1     rank_M(j) = #{pos_M <  key_M(j)}: a run of equal positives is counted at its FIRST rank (the same real
 *                           AP*, since the bins strictly inside a run are empty; no tie order among equal keys is needed);
 *   cU_M[ub_M(u)] += 1      ub_M(u) = #{pos_M <= key_M(u)}, and cE_M[ub_M(u) - 1] += 1 when the negative ties the positive there;
 * and rep_ap / rep_auc_num follow from (w, cU, cE) by ggad_rank_bootstrap_f32's two formulas in its summation order.  rep_ap and
 * rep_auc_num hold 2 reps words: A's replicates, then B's; replicate r of A and of B are the SAME drawn elements, so
 * rep_ap[r] - rep_ap[reps + r] is a replicate of the difference.  With the same seed a model's replicates here are NOT those of
 * ggad_rank_bootstrap_f32: that call draws sorted ranks and histogram bins, this one elements -- the same distribution, other bits.
 * out24: [16] reps, [17] P, [18] Nn, [19..22] 0.0, [23] status: the first non-zero of [7] and [15]; 8 = fewer than two positives or
 * two negatives; 9 = more positives than ggad_rank_bootstrap_max_pos() = 9216; else 0.  With a status other than 0 every rep_ap is
 * NaN, every rep_auc_num 0.  hist_out: NULL, or reps rows of 6 (pos_cap + 1) int32 that receive w, cU, cE of A, then of B, zero
 * beyond entry P (for tests).
 * Limits, alignment, refusals and workspace rule of ggad_rank_bootstrap_f32 (ggad_rank_bootstrap_pair_workspace_elems(n, pos_cap)
 * int32 elements, 0 = refused: two chains and 2 bytes per element and model).  No host synchronisation, LDS integer atomics only,
 * nothing waits on another workgroup, every word a launch reads was written by an earlier launch of the same call: capturable and
 * replayable; equal arguments give equal bits on any grid.
 * ---------------------------------------------------------------------------------- */
int64_t ggad_rank_bootstrap_pair_workspace_elems(int64_t n, int64_t pos_cap);   /* int32 elements; 0 = refused */
int ggad_rank_bootstrap_pair_f32(const float *score_a, const float *score_b, const uint8_t *label, int64_t n, int64_t pos_cap,
                                 float thres, uint64_t seed, int32_t reps, double *out24, double *rep_ap, int64_t *rep_auc_num,
                                 int32_t *hist_out, int32_t *workspace, ggad_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Keep the best epoch's weights on the device (select.hip): the hand-off "if this epoch's validation metric is the best so far,
 * snapshot the parameters" without a host round trip.  Neither call takes a workspace; each reads only words the host or an earlier
 * launch wrote, so both are capturable and replayable behind ggad_rank_metrics_f32 / ggad_rank_wide_f32 in a captured epoch.
 *
 * ggad_select_decide_f64: one tiny launch.  out8 = what the rank metrics wrote; which = 0 AUROC, 1 AP (anything else: GGAD_E_INVALID,
 *   no launch); state4 (device, 4 doubles) = {best_value, best_epoch, epoch, taken}, initialised by the host to {NaN, -1, 0, 0}.  With
 *   e = epoch: if curve != NULL and e < curve_cap, curve[3e .. 3e+2] = {auroc, ap, status}; taken = (status == 0 && value == value &&
 *   (best_epoch < 0 || value > best_value)) -- strict > in double, an equal later epoch never displaces an earlier one --; if taken,
 *   best_value = value and best_epoch = e; epoch = e + 1.
 * ggad_select_copy_f32: copies src[i] -> dst[i] (numel[i] floats each, i < n) in full if and only if state4[3] == 1, and writes nothing
 *   otherwise.  src / dst / numel are HOST arrays (as in ggad_adam_multi_f32), 1 <= n <= ggad_select_max_tensors() (16), every pointer
 *   4-byte aligned; outside: GGAD_E_INVALID and no launch.  16-byte accesses where source and destination share their offset within a
 *   16-byte line (the first and last 0..3 floats apart), 4-byte accesses otherwise; dst is never read.  It is a launch of its own so
 *   that no workgroup reads a word another one writes: a model of more than 16 tensors is copied in groups after ONE decide.
 * ---------------------------------------------------------------------------------- */
int32_t ggad_select_max_tensors(void);
int ggad_select_decide_f64(const double *out8, int32_t which, double *state4, double *curve, int64_t curve_cap, ggad_stream_t stream);
int ggad_select_copy_f32(int32_t n, const float *const *src, float *const *dst, const int64_t *numel, const double *state4,
                         ggad_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Explain ranked alerts (explain.hip): the exact per-feature and per-neighbour attribution of the inference logit of the mini-batch
 * GGAD model.  With a = W x1_i, z = sum_d w_d relu(a[d]) (the score is sigmoid(z): k_score) and g[f] = sum_d w_d [a[d] > 0] W[d, f]:
 *   z = sum_f g[f] x1_i[f]  =  sum_{j in N(i)+{i}} omega_ij (g . feat[j]),   omega_ij = (1 / sqrt(r_i)) / sqrt(c_j),
 * r_i the size of the closed row of i, c_j the rows (with multiplicity) of row i's slice of `batch_size` ids whose closed row holds j.
 * Both sums are complete -- no baseline, no sampling -- and exact on the ReLU pattern the row has: they explain the logit, not a
 * counterfactual.  One launch, one workgroup per explained position; nothing but the arguments is read (no plan, no cached row).
 *
 * rowptr / col: int32 CSR of n_nodes rows, columns sorted and distinct; feat: n_nodes x F floats, rows F apart; params: the engine's
 * parameter block after ggad_mb_params_sync (D, F as there); ids: the scored list, int64[n], n <= INT32_MAX, its slices are
 * [s, min(n, s + batch_size)) for s = 0, batch_size, ...; positions: int32[K] indices into ids (a position may stand twice);
 * 1 <= m <= ggad_explain_max_nbrs() (32) neighbours are listed per row.  Any D, F of ggad_mb_wide_supported (D <= 256, F <= 1,024);
 * another (D, F, m): GGAD_E_UNSUPPORTED, nothing launched.  Channel d = lane + 64 j belongs to lane `lane` of wave j (the wide
 * convention) at every D.
 * Per position k:  out_logit[k] = z;  out_feature[k * F + f] = g[f] x1[f];  out_closed_size[k] = r;  out_nbr_id / out_nbr_contrib /
 * out_nbr_colcount [k * m + c], c < min(m, r): the c-th greatest t_j = omega_ij (g . feat[j]) -- signed: what pushed the score UP; equal
 * values (-0.0 = +0.0) by ascending id -- with its node id (int64) and c_j; the other slots hold -1 / 0 / 0;  out_rest[k]: the sum of
 * the t_j that are not listed.  Every float sum has one fixed order (x1: pieces of the id-ascending list, fma in ascending j, pieces
 * ascending; a: fma over f ascending; z, g: d ascending; t_j: f ascending; rest: pieces ascending); the c_j are integers counted with
 * integer atomics: equal inputs give equal bits.
 * Rows of up to ggad_explain_lds_rows() (12,288) entries keep ids, counters and contributions in LDS (sized per launch for
 * min(n_rows_max_closed, 12,288) entries: a tight bound leaves room for more workgroups per CU); longer rows keep them in the
 * workspace.  workspace: ggad_explain_workspace_elems(n_rows_max_closed, K, m) int32 elements (0 = refused), no preparation needed,
 * n_rows_max_closed = S >= every explained closed row (deg + 1 bounds it).  After the call: float t_j at [k * S + q], int32 c_j at
 * [K * S + k * S + q], q < r the index in the id-ascending closed row (the rest of the workspace is scratch).
 * out_meta (device, 4 x int64; cleared by the call): {status, rows explained, rows that took the workspace branch, 0}.  status 0: fine;
 * 2: a closed row is longer than n_rows_max_closed (its slot: closed_size = r, everything else padding); 3: a NaN feature or weight on
 * an explained row; 5: a position outside 0..n-1 or an id that is no node (a position's slot: padding, closed_size 0).  The greatest
 * status of any row stands.
 * ---------------------------------------------------------------------------------- */
int32_t ggad_explain_max_nbrs(void);
int32_t ggad_explain_lds_rows(void);
int64_t ggad_explain_workspace_elems(int64_t n_rows_max_closed, int64_t K, int32_t m);   /* int32 elements; 0 = refused */
int ggad_explain_f32(const int32_t *rowptr, const int32_t *col, int32_t n_nodes, const float *feat, const float *params, int32_t D,
                     int32_t F, const int64_t *ids, int64_t n, int32_t batch_size, const int32_t *positions, int32_t K, int32_t m,
                     int32_t n_rows_max_closed, float *out_logit, float *out_feature, int32_t *out_closed_size, int64_t *out_nbr_id,
                     float *out_nbr_contrib, int32_t *out_nbr_colcount, float *out_rest, int64_t *out_meta, int32_t *workspace,
                     ggad_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GGAD_HIP_H */
