/*
 * bbgr.h — C ABI of the MI355X-native LightGCN propagation + BPR training path.
 *
 * One shared library (libbbgr.so, hipcc --offload-arch=gfx950) exports every entry
 * point below. Plain pointers and sizes only: no torch types cross this boundary.
 *
 * Conventions (every entry point):
 *   - Caller-owned DEVICE buffers; no allocation inside hot calls. Entry points that
 *     need scratch take (workspace, workspace_bytes), all by one protocol:
 *     workspace == NULL queries the size into *workspace_bytes (nothing is
 *     launched); a workspace of fewer than that many bytes is refused with
 *     BBGR_ERR_WORKSPACE and the text "<entry>: workspace <have> < <need>
 *     bytes"; a null workspace_bytes is BBGR_ERR_INVALID. A size query may need
 *     a device: where hipcub sizes its own temporary storage (scans, selects,
 *     the larger sorts) it asks the runtime for one.
 *   - Stream-ordered on the hipStream_t passed as `stream` (NULL = default stream).
 *     No host synchronisation except in the entry points documented as "syncs"
 *     (one-time operator planning only).
 *   - Return BBGR_OK (0) or a negative bbgr_status; bbgr_last_error() gives text.
 *   - Re-entrant across distinct streams.
 *   - Index arrays are int32 for CSR structure (nnz < 2^31), int64 for batch
 *     index vectors (they are torch.long in the reference).
 *
 * What each entry point replaces in the reference (paths relative to the
 * reference repo root) is cited on its declaration.
 */
#ifndef BBGR_H
#define BBGR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BBGR_ABI_VERSION 12

typedef enum {
  BBGR_OK = 0,
  BBGR_ERR_INVALID = -1,     /* bad argument (null pointer, size, alignment) */
  BBGR_ERR_UNSUPPORTED = -2, /* valid but not implemented (e.g. emb dim) */
  BBGR_ERR_HIP = -3,         /* a HIP runtime call failed; see bbgr_last_error() */
  BBGR_ERR_WORKSPACE = -4    /* workspace missing or too small */
} bbgr_status;

typedef void *bbgr_stream_t; /* a hipStream_t */

/* ------------------------------------------------------------------------- */
/* Library                                                                    */
/* ------------------------------------------------------------------------- */
int bbgr_abi_version(void);
/* Text for the most recent failure on the calling host thread. */
const char *bbgr_last_error(void);
/* Device properties the planner uses (CU count, arch name). */
int bbgr_device_info(int device, int *cu_count, char *arch_name, int arch_name_len);
/* Blocks until `stream` has drained (the one explicit sync). */
int bbgr_sync(bbgr_stream_t stream);
/* An empty kernel, profile_marker_kernel, of `tag` workgroups (1 <= tag <=   */
/* 1024; ABI 10): bench.py brackets its timed steps with tags 1 / 2 so a      */
/* rocprofv3 trace can be cut at them by dispatch order                       */
/* (tools/summarize_profile.py).                                              */
int bbgr_profile_marker(int32_t tag, bbgr_stream_t stream);

/* ------------------------------------------------------------------------- */
/* CSR structure                                                              */
/*   Replaces: sparse_coo_tensor(...).coalesce() in                           */
/*     Version-2/lighgcn_cu_pop.py:443,450; lightgcn_cu.py:393,397;          */
/*     lightgcn.py:363,372 — and edges_to_user_csr, Version-2:309-327.        */
/*   Duplicate (row,col) pairs are KEPT as repeated entries; summing repeated */
/*   entries in the SpMM is what coalesce()'s value-sum does.                 */
/* ------------------------------------------------------------------------- */

/* Build a row-sorted CSR with columns sorted inside each row (stable:
 * duplicates keep their input order). `perm_out` (nullable) receives, for every
 * CSR slot, the input edge id it came from — used to permute per-edge values.
 * Device arrays: rows[nnz], cols[nnz] -> indptr[n_rows+1], indices[nnz]. */
int bbgr_csr_build(int64_t nnz, const int32_t *rows, const int32_t *cols,
                   int32_t n_rows, int32_t n_cols, int32_t *indptr,
                   int32_t *indices, int32_t *perm_out, void *workspace,
                   size_t *workspace_bytes, bbgr_stream_t stream);

/* Load-balance plan for the SpMM. Rows with degree > long_threshold are cut
 * into chunks of at most chunk_edges edges; each chunk is one 256-thread
 * workgroup. Rows cut into >1 chunk ("split rows") are finished by a fix-up
 * pass. chunks[n_chunks][4] = {row, e_begin, e_end, slot (-1: sole chunk)};
 * split[n_split][4] = {row, slot_begin, n_slots, 0}.                         */
typedef struct {
  int32_t n_rows;
  int32_t n_cols;
  int64_t nnz;
  const int32_t *indptr;  /* [n_rows+1] device */
  const int32_t *indices; /* [nnz] device */
  int32_t long_threshold; /* 0 => default (256) */
  int32_t chunk_edges;    /* 0 => default (2048) */
  int32_t n_chunks;
  int32_t n_split;
  const int32_t *chunks; /* [n_chunks*4] device */
  const int32_t *split;  /* [n_split*4] device */
} bbgr_csr;

/* Counts chunks and split rows for csr->long_threshold / chunk_edges (fills
 * csr-side values into *n_chunks / *n_split). SYNCS `stream` (one-time). */
int bbgr_csr_plan_count(const bbgr_csr *csr, int32_t *n_chunks, int32_t *n_split,
                        void *workspace, size_t *workspace_bytes,
                        bbgr_stream_t stream);
/* Fills chunks[n_chunks*4] and split[n_split*4] (sizes from plan_count). */
int bbgr_csr_plan_build(const bbgr_csr *csr, int32_t *chunks, int32_t *split,
                        void *workspace, size_t *workspace_bytes,
                        bbgr_stream_t stream);

/* out[s] = the slot of b holding the edge of slot s of a, b being a's        */
/* transpose with column-sorted rows (the k-th copy of a duplicate pair maps   */
/* to the k-th copy). One-time; feeds bbgr_mark_slots.                         */
int bbgr_transpose_slots(const bbgr_csr *a, const bbgr_csr *b, int32_t *out,
                         bbgr_stream_t stream);
/* The same map from the two CSR builds' permutations (bbgr_csr_build's      */
/* perm_out of a and of b over ONE edge list: slot -> edge id): out[s] =      */
/* inv(perm_b)[perm_a[s]]. Two O(nnz) passes instead of a binary search per   */
/* edge; equal to bbgr_transpose_slots (the builds' sorts are stable, so the  */
/* k-th copy of a duplicate pair is the k-th in edge order on both sides).    */
/* scratch: nnz int32, distinct from out.                                     */
int bbgr_slots_from_perms(int64_t nnz, const int32_t *perm_a, const int32_t *perm_b,
                          int32_t *out, int32_t *scratch, bbgr_stream_t stream);

/* ------------------------------------------------------------------------- */
/* Vertex order (a one-time relabelling before the CSR build)                 */
/*   The reference indexes users / items in id-map order (Version-2:227-303). */
/*   Numbering the rows of a table by descending degree packs its most        */
/*   gathered rows into one address range: the SpMM then streams the cold     */
/*   rows (bbgr_spmm_args.stream_from) and keeps the hot ones cached. Every   */
/*   operator is permutation-equivariant, so the result is the same model up */
/*   to the row order (and fp32 summation order inside a row).                */
/* ------------------------------------------------------------------------- */
/* degree[j] = number of e < n_ids with ids[e] == j, j < n (exact).           */
int bbgr_degree_count(int64_t n_ids, const int32_t *ids, int32_t n, int32_t *degree,
                      bbgr_stream_t stream);
/* The same with a workspace (query with workspace == NULL): below 4M ids, 8  */
/* replicated counter arrays (one per XCD's workgroups) summed at the end     */
/* (power-law ids contend 8x less; 32*n bytes); from 4M ids on, a radix sort */
/* of the ids, a run-length encode and one scatter of the run lengths (no    */
/* atomics; ~4*n_ids + 8*n bytes + sort scratch). Ids must lie in [0, n).    */
int bbgr_degree_count_ws(int64_t n_ids, const int32_t *ids, int32_t n, int32_t *degree,
                         void *workspace, size_t *workspace_bytes, bbgr_stream_t stream);
/* perm[new] = old id, rank[old] = new id, by descending degree; equal degrees */
/* keep ascending id (stable). Workspace query with workspace == NULL.        */
int bbgr_degree_order(int32_t n, const int32_t *degree, int32_t *perm, int32_t *rank,
                      void *workspace, size_t *workspace_bytes, bbgr_stream_t stream);
/* out[e] = map[ids[e]] for e < n (out may alias ids).                        */
int bbgr_relabel(int64_t n, const int32_t *ids, const int32_t *map, int32_t *out,
                 bbgr_stream_t stream);

/* ------------------------------------------------------------------------- */
/* Operator scale vectors                                                     */
/*   Replaces the numpy weight math of build_message_passing_mats             */
/*   (Version-2/lighgcn_cu_pop.py:429-452), its Method-A variant              */
/*   (version_1/lightgcn_cu_pop_long_tail_exposure.py:362-396),               */
/*   build_cred_weighted_mats (lightgcn_cu.py:368-399) and build_norm_adj     */
/*   (lightgcn.py:352-372).                                                   */
/*                                                                            */
/* Every operator of the reference factors as diag(row) * A * diag(col) over  */
/* the 0/1(+multiplicity) adjacency A:                                        */
/*   item<-user  M = diag(p) A_iu diag(q)      user<-item  M = diag(s) A_ui diag(t)
 *   GS / J : p = t = b, q = c*a, s = a    (a = 1/sqrt(max(deg_u,1)),         */
/*                                          b = 1/sqrt(max(deg_i,1)))         */
/*   Method A: p = t = b*alpha, alpha = 1/log1p(max(deg_i,1))                 */
/*   S (symmetric N x N): p = t = deg_i^-1/2, q = s = deg_u^-1/2 (inf -> 0)   */
/* Outputs (device, fp32): deg_u[U], deg_i[I], p[I], q[U], s[U], t[I],        */
/* pt[I] = p*t, qs[U] = q*s. cred (nullable => all ones) is clipped to [0,1]  */
/* by the caller as the reference loader does.                                */
/* ------------------------------------------------------------------------- */
typedef enum {
  BBGR_OP_GS = 0,       /* Version-2/lighgcn_cu_pop.py (credibility inside messages) */
  BBGR_OP_METHOD_A = 1, /* version_1/lightgcn_cu_pop_long_tail_exposure.py     */
  BBGR_OP_J = 2,        /* lightgcn_cu.py (same weights as GS, Jacobi order)  */
  BBGR_OP_SYM = 3       /* lightgcn.py symmetric normalised adjacency         */
} bbgr_op_kind;

int bbgr_operator_scales(int32_t kind, int32_t n_users, int32_t n_items,
                         const int32_t *indptr_u, const int32_t *indptr_i,
                         const float *cred, float *deg_u, float *deg_i,
                         float *p, float *q, float *s, float *t, float *pt,
                         float *qs, bbgr_stream_t stream);

/* out[e] = scale[indices[e]] for e < nnz: a column scale expanded into CSR
 * slot order, so a chain's first SpMM streams 4 coalesced bytes per edge
 * (weight_mode 1) instead of gathering scale[col] at random (weight_mode 2). */
int bbgr_gather_scale(int64_t nnz, const int32_t *indices, const float *scale,
                      float *out, bbgr_stream_t stream);

/* ------------------------------------------------------------------------- */
/* Fused CSR-SpMM (the hot kernel)                                            */
/*   Replaces torch.sparse.mm at Version-2/lighgcn_cu_pop.py:483-484,         */
/*   lightgcn_cu.py:431,434, lightgcn.py:323 and the autograd backward of     */
/*   each (transposed operator), plus the stack(...).mean(0) layer mean       */
/*   (Version-2:488-489) as a fused accumulate epilogue.                      */
/*                                                                            */
/* For every row r of A:                                                      */
/*   T_r = sum_{e in row r} w_e * x[col_e, :]                                  */
/*        w_e = 1                     (weight_mode 0)                          */
/*        w_e = edge_val[e]           (weight_mode 1, CSR slot order)          */
/*        w_e = col_scale[col_e]*col_scale_s   (weight_mode 2)                 */
/*   y[r]       = ys_r * T_r + as_r * add[r]            (if y   != NULL)      */
/*                ys_r = (y_scale ? y_scale[r] : 1) * y_scale_s               */
/*                as_r = (add_scale ? add_scale[r] : 1) * add_scale_s         */
/*   acc_out[r] = (acc_in[r] + cs_r * T_r) * gamma       (if acc_out != NULL) */
/*                cs_r = (acc_scale ? acc_scale[r] : 1) * acc_scale_s;        */
/*                acc_in NULL => 0                                            */
/* Tables are fp32 row-major with leading dimension ld* (floats, multiple of  */
/* 4, 16-byte aligned base). d in {64, 128, 256}, or 8, 16, 32 for the      */
/* column slices of a column-sharded model (narrow rows: d/4 lanes gather one */
/* row, 16/(d/4) edges per load round, slot sums added by a fixed xor tree).  */
/* src_mask (nullable, [n_cols] bytes): edges whose column is 0 in the mask    */
/*   are skipped — exact when x is zero on those rows (sparse gradients).     */
/* row_mask (nullable, [n_rows] bytes): rows that are 0 are not computed and  */
/*   not written (only the flagged rows of the outputs are needed).           */
/* acc_mask (nullable, [n_rows]): acc_in/acc_out touched only on flagged rows */
/* add_mask (nullable, [n_rows]): add[r] read only on flagged rows (treated   */
/*   as 0 elsewhere — exact when add is zero off the mask).                   */
/* row_list (nullable, int64 [n_row_list]): compute only these rows (short    */
/*   rows on a grid sized by the list; long rows need row_mask set for their  */
/*   chunk workgroups: a row_list without row_mask is rejected when the plan  */
/*   has chunks). Listed rows must be distinct. Launches with any mask or list run as */
/*   `spmm_masked_kernel`, full-CSR launches as `spmm_kernel`.                */
/* use_range != 0: compute only rows [range[0], range[1]), whose long-row     */
/*   chunks are [range[2], range[3]) and split rows [range[4], range[5]) of   */
/*   the plan (all three are row-ordered, so a row range maps to contiguous   */
/*   chunk / split ranges). Lets the sharded step all-reduce item partial     */
/*   sums chunk by chunk, overlapped with the next chunk's SpMM. Combined     */
/*   with row_list (+ row_mask): the short rows are the list's entries (the   */
/*   caller passes the slice of its sorted list inside [range[0], range[1])) */
/*   and the range selects the chunk / split-row sub-ranges only.             */
/* adam_param (nullable): fused optimizer step. The row value the y output    */
/*   would receive (g = ys*T + as*add) is the gradient of that row of         */
/*   adam_param, and bbgr_adam's update (bit for bit: every hyper-parameter, */
/*   from any moments at any step t, host scalars or adam_state) is applied  */
/*   in place to adam_param / adam_exp_avg / adam_exp_avg_sq (row stride      */
/*   adam_ld). y may then be NULL: the gradient table is never written nor    */
/*   re-read (the last backward product of the training step, V2:862-863).   */
/*   Every row of the launch must be computed (no masks / row lists).         */
/* stream_from > 0: source rows with index >= stream_from are gathered with   */
/*   non-temporal (streaming) loads, so they do not evict the rows below it  */
/*   from L2 / Infinity Cache. Meant for a source table in descending-degree  */
/*   order (bbgr_degree_order), where rows [0, stream_from) are the hot set.  */
/*   Results are unchanged; 0 = every row loaded with the default policy.     */
/* stream_out_from > 0: output rows >= stream_out_from are stored streaming   */
/*   (y, and the fused-Adam parameter row), and the fused Adam's moments are  */
/*   streamed in and out: the next product gathers this table, and only its  */
/*   hot prefix (output table in degree order) is worth keeping cached.       */
/* adam_state (nullable, with adam_bc_table): the fused Adam reads its step t */
/*   from device memory (bbgr_step_begin's state[0]) and its bias corrections */
/*   from adam_bc_table[2(t-1)], [2(t-1)+1] instead of the two float fields,  */
/*   so a captured step (hipGraph) replays with the right t every time.       */
/* y_map / acc_map / add_map (nullable, int32 [n_rows]): row maps of the      */
/*   epilogue's tables. CSR row r writes row y_map[r] of y (and updates row   */
/*   y_map[r] of the fused Adam's tables), reads / writes row acc_map[r] of    */
/*   acc_in / acc_out and reads row add_map[r] of add; acc_mask / add_mask    */
/*   index the mapped rows. Scale vectors stay indexed by r. Lets a graph      */
/*   numbered by descending degree serve tables the caller holds in its own    */
/*   (input) order: the drop-in modules' first products gather input-order    */
/*   rows through input-id column indices, and these maps place every        */
/*   input-order output row, so no table is permuted. stream_out_from must be */
/*   0 when y_map is set.                                                      */
/* src_bits (nullable, with src_mask, d >= 64): a bitmap over this CSR's      */
/*   slots, bit e set iff src_mask[indices[e]] != 0 (bbgr_mark_slots of the    */
/*   source rows' edges). The gather then tests liveness on the bitmap (64     */
/*   edges per test) and loads only live edges' indices: a first backward      */
/*   product over a few batch rows' edges stops scanning every index of the  */
/*   row. Results are bitwise those of src_mask alone (same edges, same      */
/*   order); bits of padding: 3 words beyond nnz/32, readable. With src_bits  */
/*   the rows of one chunk (long_threshold < deg <= chunk_edges) are summed by */
/*   the row's lane group in the chunk workgroup's order (bitwise the same):  */
/*   a listed launch must then list them (row_mask alone no longer sums them) */
/* acc_in_map (nullable, int32 [n_rows]): acc_in's own row map — row r reads */
/*   acc_in row acc_in_map[r] while acc_out is placed by acc_map. Lets a chain */
/*   keep its layer-mean accumulator in the graph's (degree) order between    */
/*   layers: the first layer reads the caller's table through its map, the   */
/*   last writes the caller's order, the middle ones touch no map (random    */
/*   256-byte rows cost ~30 % of a user-side product at C4).                  */
/* row_count (nullable, DEVICE int64, with row_list): the list holds           */
/*   min(n_row_list, *row_count) rows; n_row_list is its capacity. For a list  */
/*   built on the stream (a captured step): a fixed grid of short-row          */
/*   workgroups walks it, so the host never reads the length.                  */
/* adam_grad (nullable, with adam_param; ABI 6): the fused Adam's gradient is */
/*   adam_grad_scale * adam_grad[row] (row stride adam_grad_ld) instead of the */
/*   row value, and y is written as usual: an item-row product of the GS      */
/*   backward carries the item table's Adam step, whose gradient (the sparse  */
/*   BPR rows / (K+1) + ego rows) is final before the product runs, so the   */
/*   separate pass over the item table (28 B / parameter) overlaps the        */
/*   product's gathers. Same rounding as bbgr_adam with grad_scale.          */
/* adam_map (nullable, int32 [n_rows]; ABI 7): the fused Adam's rows (param, */
/*   exp_avg, exp_avg_sq and adam_grad) of CSR row r are row adam_map[r]      */
/*   instead of y_map's: a product that writes y in the graph's order while  */
/*   the weights live in the caller's (the drop-in's in-backward item Adam). */
/* adam_moments_unmapped (ABI 9): nonzero keeps exp_avg / exp_avg_sq at the  */
/*   launch's own row r (the graph's order) while the param and adam_grad    */
/*   follow adam_map: the drop-in optimizer stores its moments in the graph's */
/*   order, so only the caller-order weight row is read and written at       */
/*   random (bbgr.optim.FusedAdam converts them at its state_dict boundary). */
/* src_mask_bits (nullable, with src_mask; ABI 10): the same mask packed one */
/*   bit per source row (bit c & 31 of word c >> 5; bbgr_mask_pack), read by */
/*   the per-edge liveness test instead of the bytes: fewer L2 requests for   */
/*   the same test (degree-ordered hub columns share lines). Bitwise the byte */
/*   mask's result.                                                            */
/* adam_mirror (nullable, with adam_moments_unmapped; ABI 10): adam_param is */
/*   then in the launch's row order as well (row r, like the moments), and   */
/*   every updated param row is also stored to adam_mirror row adam_map[r]   */
/*   (y_map[r] without adam_map), stride adam_ld: the drop-in optimizer keeps */
/*   a graph-ordered master copy of a weight table, streamed with its        */
/*   moments, and the caller's table is only written (no random row read).   */
/* tag_out (nullable, int32 [nnz], with tag_mask [n_cols] bytes; ABI 10): a  */
/*   full launch (no masks, list, range or fused Adam) also writes            */
/*   tag_out[e] = indices[e] with bit 31 set where tag_mask[indices[e]] == 0, */
/*   for every slot e of the CSR. src_tagged (nullable, ABI 10): a launch     */
/*   reads its column indices from src_tagged instead, an index with bit 31   */
/*   set being a dead source skipped as src_mask would skip it (so src_mask   */
/*   and src_bits must be NULL): the src-masked backward user product reads   */
/*   the frontier from the copy the forward's first user product wrote, with  */
/*   no mask load between an index and its gather. Bitwise the src_mask       */
/*   launch. Both need a two-row CSR (nnz <= 24 n_rows) and d >= 64.          */
/* partial: n_chunks*d floats followed by n_chunks int32 arrival counters     */
/*   (zero when allocated; each launch leaves them zero): the last chunk of a */
/*   split row to arrive sums the row's partials in chunk order in the same  */
/*   launch (no separate fix-up kernel). Needed when csr->n_split > 0. Two    */
/*   launches that may run at once (different streams) need two buffers.     */
/* ------------------------------------------------------------------------- */
typedef struct {
  int32_t d;
  const float *x;
  int64_t ldx;
  int32_t weight_mode;
  const float *edge_val;
  const float *col_scale;
  float col_scale_s;
  float *y;
  int64_t ldy;
  const float *y_scale;
  float y_scale_s;
  const float *add;
  int64_t ldadd;
  const float *add_scale;
  float add_scale_s;
  const float *acc_in;
  int64_t ldacc_in;
  float *acc_out;
  int64_t ldacc_out;
  const float *acc_scale;
  float acc_scale_s;
  float gamma;
  float *partial;
  const uint8_t *src_mask;
  const uint8_t *row_mask;
  const uint8_t *acc_mask;
  const uint8_t *add_mask;
  const int64_t *row_list;
  int64_t n_row_list;
  int32_t use_range;
  int32_t range[6];
  float *adam_param;
  float *adam_exp_avg;
  float *adam_exp_avg_sq;
  int64_t adam_ld;
  float adam_lr;
  double adam_beta1;   /* doubles (ABI 12): 1 - beta is formed in double, as torch does */
  double adam_beta2;
  float adam_eps;
  float adam_weight_decay;
  float adam_bias_correction1;
  float adam_bias_correction2_sqrt;
  int32_t stream_from;
  int32_t stream_out_from;
  const float *adam_bc_table;
  const int64_t *adam_state;
  const int32_t *y_map;
  const int32_t *acc_map;
  const int32_t *add_map;
  const uint32_t *src_bits;
  const int64_t *row_count;
  const int32_t *acc_in_map;
  const float *adam_grad;
  int64_t adam_grad_ld;
  float adam_grad_scale;
  const int32_t *adam_map;
  int32_t adam_moments_unmapped;
  int32_t *tag_out;
  const uint8_t *tag_mask;
  const int32_t *src_tagged;
  float *adam_mirror;
  const uint32_t *src_mask_bits;
} bbgr_spmm_args;

int bbgr_spmm(const bbgr_csr *csr, const bbgr_spmm_args *args,
              bbgr_stream_t stream);

/* The SpMM epilogue alone, with T read from a dense table t[n_rows, ldt]
 * (args->x / weight fields ignored; row_mask, acc_mask, add_mask honoured). Used after the RCCL all-reduce of
 * per-rank item partial sums in the user-row-sharded multi-GPU step, where
 * the epilogue cannot run before the sum is complete.
 * args->row_list (nullable): t is COMPACT, t[n_row_list, ldt]; its row j is
 * the sum of output row row_list[j] (< n_rows, the output tables' row count).
 * The sparse frontier exchange all-reduces only those rows. */
int bbgr_epilogue(int32_t n_rows, const float *t, int64_t ldt,
                  const bbgr_spmm_args *args, bbgr_stream_t stream);

/* ------------------------------------------------------------------------- */
/* bf16 tables for the forward chain (opt-in; an addition to ABI 12)          */
/*                                                                            */
/* LightGCN's propagation is linear and its backward reads no forward         */
/* activation, so the layer tables whose only reader is the next product's    */
/* gather can be kept in bf16 (2 bytes per element, the upper half of an      */
/* fp32): the gathers move half the bytes. Sums, the layer-mean accumulators  */
/* and everything downstream stay fp32.                                       */
/*                                                                            */
/* The conversion: dst[r, c] = bf16(src[r, c]) for r < n_rows, c < d, round   */
/* to nearest even; bit for bit torch's .to(torch.bfloat16) on finite values, */
/* +-0, subnormals and +-inf; a NaN becomes the quiet NaN 0x7fc0. d is a      */
/* multiple of 4. src: 16-byte aligned, ldsrc >= d, ldsrc % 4 == 0. dst:      */
/* 16-byte aligned, lddst >= d, lddst % 8 == 0 (elements); columns past d are */
/* not written.                                                               */
/* ------------------------------------------------------------------------- */
int bbgr_to_bf16(int64_t n_rows, int32_t d, const float *src, int64_t ldsrc,
                 uint16_t *dst, int64_t lddst, bbgr_stream_t stream);

/* The product on a bf16 source table: io->x [n_cols, ldx] replaces args->x   */
/* and io->y [n_rows, ldy] (nullable) replaces args->y; args->x and args->y   */
/* must be NULL. Every other field is read from args with its meaning above.  */
/*   T_r is accumulated in fp32; y[r] = ys_r * T_r is rounded once (nearest   */
/*   even) to bf16; acc_out = (acc_in + cs_r * T_r) * gamma stays fp32, with  */
/*   acc_scale, acc_mask and the streaming stores as above.                   */
/* Supported subset (the launches of the forward chain):                      */
/*   d in {64, 128, 256}; weight_mode 0 or 1; y_scale, acc_in / acc_out /     */
/*   acc_scale / gamma / acc_mask; row_mask; row_list with n_row_list and     */
/*   row_count; the load-balance plan (long-row chunks, split rows through    */
/*   the fp32 partial workspace, sized as for the fp32 entry); the two-row    */
/*   form for CSRs with nnz <= 24 * n_rows; stream_from / stream_out_from     */
/*   (rows of the 2-byte tables: the same byte budget keeps twice the rows).  */
/* Refused before any launch: BBGR_ERR_UNSUPPORTED for d < 64, weight_mode 2, */
/*   add, the fused Adam fields, src_mask, src_mask_bits, src_bits,           */
/*   src_tagged, tag_out, the row maps and use_range; BBGR_ERR_INVALID for    */
/*   null tables, a set args->x / args->y, or a misaligned table.             */
/* Alignment: io->x and io->y are 16-byte aligned, ldx and ldy (in elements)  */
/*   are >= d and multiples of 8, so every row starts on a 16-byte boundary.  */
/* Relation to the fp32 entry: every output element is the same fp32 sum in   */
/*   the same order as that entry computes on the source widened to fp32      */
/*   (edges in CSR order, chunk and split partials in plan order, the same    */
/*   multiply / fused-multiply-add sequence in the epilogue). acc_out is      */
/*   therefore bitwise that entry's acc_out on the widened table, and y is    */
/*   bitwise that entry's y rounded to bf16.                                  */
typedef struct {
  const uint16_t *x;
  int64_t ldx;
  uint16_t *y;
  int64_t ldy;
} bbgr_spmm_bf16_io;

int bbgr_spmm_bf16(const bbgr_csr *csr, const bbgr_spmm_args *args,
                   const bbgr_spmm_bf16_io *io, bbgr_stream_t stream);

/* ------------------------------------------------------------------------- */
/* Fused BPR loss: gather -> dot -> log-sigmoid -> (+reg, +fair) -> grads     */
/*   Replaces LightGCN.bpr_loss, Version-2/lighgcn_cu_pop.py:495-508          */
/*   (== lightgcn.py:333-349 with ego offset; lightgcn_cu.py:635-648 adds     */
/*   lambda_fair * mean(pop[pos] * pos_score)) and its autograd backward.     */
/*                                                                            */
/* Per triple b (u, p, n):                                                    */
/*   s+ = <uf[u], if[p]>, s- = <uf[u], if[n]>                                 */
/*   parts[3b+0] = -log(sigmoid(s+ - s-) + 1e-12)                             */
/*   parts[3b+1] = |ue[u]|^2 + |ie[p]|^2 + |ie[n]|^2   (ego tables)           */
/*   parts[3b+2] = pop ? pop[p] * s+ : 0                                      */
/* loss = mean(parts0) + reg * mean(parts1) + lambda_fair * mean(parts2).     */
/* If grads requested, with G = dloss ? *dloss : 1 (device scalar):           */
/*   g_uf[u] += .., g_if[p] += .., g_if[n] += ..   (dense tables, atomics)    */
/*   g_ue[u] += 2 reg G/B ue[u], g_ie[p|n] += 2 reg G/B ie[p|n]               */
/* Any grad pointer may be NULL to skip it. Index vectors are int64.          */
/* contrib (nullable, [3*batch rows], ld ldcontrib): deterministic mode. The  */
/*   g_uf / g_if terms are NOT scattered; instead row b receives the user    */
/*   term of triple b, row batch+b its pos-item term, row 2*batch+b its      */
/*   neg-item term (zero rows for skipped triples). bbgr_scatter_add_rows   */
/*   then sums them per destination row in a fixed order (bitwise            */
/*   reproducible training step).                                            */
/* A triple with an index outside [0,n_users) / [0,n_items) (e.g. the        */
/* sampler's -1 for a user without positives) contributes zero everywhere.   */
/* Column-sharded tables (each rank holds d of the model's columns): a first  */
/*   call with scores_out writes this shard's (s+, s-, |ue|^2+|ie+|^2+|ie-|^2) */
/*   per triple and nothing else; the caller sums them over the shards        */
/*   (all-reduce, 12 B per triple) and a second call with scores uses the     */
/*   complete sums for the loss parts and the gradient coefficients, writing  */
/*   this shard's columns of the gradient rows.                               */
/* d: 8, 16, 32, 64, 128 or 256 (narrow widths: column shards).               */
/* ------------------------------------------------------------------------- */
typedef struct {
  int64_t batch;
  int32_t d;
  int64_t n_users;                 /* rows of uf / ue (bounds check) */
  int64_t n_items;                 /* rows of itf / ie (bounds check) */
  const int64_t *users;
  const int64_t *pos;
  const int64_t *neg;
  const float *uf; int64_t lduf;   /* final user table */
  const float *itf; int64_t ldif;  /* final item table */
  const float *ue; int64_t ldue;   /* ego user table */
  const float *ie; int64_t ldie;   /* ego item table */
  const float *pop;                /* nullable, [I] */
  float reg;
  float lambda_fair;
  float *parts;                    /* nullable, [3*batch] */
  const float *dloss;              /* nullable device scalar */
  float *g_uf; int64_t ldguf;
  float *g_if; int64_t ldgif;
  float *g_ue; int64_t ldgue;
  float *g_ie; int64_t ldgie;
  float *contrib; int64_t ldcontrib;
  float *scores_out;               /* nullable, [3*batch]: see below */
  const float *scores;             /* nullable, [3*batch]: see below */
} bbgr_bpr_args;

int bbgr_bpr(const bbgr_bpr_args *args, bbgr_stream_t stream);

/* loss[0] = sum(parts0)/B + reg*sum(parts1)/B + lambda_fair*sum(parts2)/B,
 * fixed-order (deterministic) reduction in one workgroup. */
int bbgr_bpr_reduce(int64_t batch, const float *parts, float reg,
                    float lambda_fair, float *loss, bbgr_stream_t stream);

/* ------------------------------------------------------------------------- */
/* Adam (torch.optim.Adam defaults: amsgrad=False, maximize=False)            */
/*   Replaces opt.step() at Version-2/lighgcn_cu_pop.py:863 (Adam lr=1e-3,    */
/*   :793). Host computes bias_correction1 = 1-beta1^t and                    */
/*   bias_correction2_sqrt = sqrt(1-beta2^t) in double, as torch does.        */
/*   m = lerp(m, g, 1-beta1); v = beta2 v + (1-beta2) g^2;                    */
/*   p -= (lr/bc1) * m / (sqrt(v)/bc2_sqrt + eps)   (+ weight_decay*p in g)   */
/*   with g = grad_scale * grad[i] (1.0 = plain Adam; the GS item gradient    */
/*   gI/(K+1) is folded in this way instead of materialising it).             */
/*   beta1 / beta2 are doubles (ABI 12): 1 - beta is formed in double and     */
/*   rounded once, as torch does; from a float beta it is off by up to 2^-25  */
/*   absolute: measured over 12 steps, 1.3e-5 of exp_avg_sq at beta2 = 0.999  */
/*   and 1.4e-3 at 0.99999.                                                   */
/*   Checked against float64 over 12 steps (tests/test_gpu_adam.py) with      */
/*   non-default betas and eps, weight decay, beta1 = 0, idle rows and        */
/*   grad_scale: the error of update, exp_avg and exp_avg_sq stays within 4x  */
/*   that of torch.optim.Adam on fp32 CPU tensors (+ one fp32 rounding). The  */
/*   roundings are not torch's bit for bit: lr / bc1 is a float division and  */
/*   the moments are updated with explicit fma.                               */
/* ------------------------------------------------------------------------- */
int bbgr_adam(int64_t n, float *param, const float *grad, float *exp_avg,
              float *exp_avg_sq, float lr, double beta1, double beta2, float eps,
              float weight_decay, float grad_scale, float bias_correction1,
              float bias_correction2_sqrt, bbgr_stream_t stream);

/* ------------------------------------------------------------------------- */
/* Device-resident step state (graph-captured training steps)                 */
/*   A training step captured once into a hipGraph (torch.cuda.CUDAGraph) and */
/*   replayed must not bake the host's per-step scalars into kernel args.     */
/*   state[4] int64 on the device: state[0] = Adam step t, state[1] = this    */
/*   step's sampler counter, state[2] = the next one, state[3] = the number   */
/*   of steps bc_table holds (>= 1). bbgr_step_begin (one lane): t += 1;      */
/*   state[1] = state[2]; state[2] += 1 -- the same sequence the host keeps   */
/*   for an eager step (counter used, then incremented).                      */
/*   bc_table[2(t-1)] = 1 - beta1^t, bc_table[2(t-1)+1] = sqrt(1 - beta2^t),  */
/*   computed on the host in double as torch does, rounded to float: the     */
/*   device constants are then bit-identical to the host ones.               */
/*   bbgr_adam_dev / bbgr_sample_dev: bbgr_adam / bbgr_sample with t and the  */
/*   counter read from state. Every reader clamps t to [1, state[3]]: a table */
/*   of >= ~20k steps is exact past its end (both corrections are 1.0f).      */
/* ------------------------------------------------------------------------- */
int bbgr_step_begin(int64_t *state, bbgr_stream_t stream);
int bbgr_adam_dev(int64_t n, float *param, const float *grad, float *exp_avg,
                  float *exp_avg_sq, float lr, double beta1, double beta2, float eps,
                  float weight_decay, float grad_scale, const float *bc_table,
                  const int64_t *state, bbgr_stream_t stream);

/* ------------------------------------------------------------------------- */
/* Row utilities for the fused training step                                  */
/* ------------------------------------------------------------------------- */
/* Row utilities skip negative indices (the sampler's -1 "no item").        */
/* table[idx[k], :d] = 0 for k < n (restores all-zero gradient tables). */
int bbgr_rows_zero(int64_t n, const int64_t *idx, float *table, int64_t ld,
                   int32_t d, bbgr_stream_t stream);
/* dst[idx[k], :] += alpha * src[idx[k], :] (atomic; duplicates sum). */
int bbgr_rows_axpy(int64_t n, const int64_t *idx, float alpha, const float *src,
                   int64_t ldsrc, float *dst, int64_t lddst, int32_t d,
                   bbgr_stream_t stream);

/* dst[idx[k], :d] = src[idx[k], :d] for k < n (ABI 6; idx[k] < 0 skipped,  */
/* repeated rows write the same value). d and both ld multiples of 4, tables */
/* 16-byte aligned. Copies a sparse table's batch rows into another.         */
int bbgr_rows_copy(int64_t n, const int64_t *idx, const float *src, int64_t ldsrc,
                   float *dst, int64_t lddst, int32_t d, bbgr_stream_t stream);

/* dst[k, :d] = src[idx[k], :d] for k < n (zero row where idx[k] < 0). d and
 * both ld multiples of 4, tables 16-byte aligned. Compacts frontier rows for
 * the sparse multi-GPU exchange (the inverse is bbgr_epilogue's row_list). */
int bbgr_rows_gather(int64_t n, const int64_t *idx, const float *src, int64_t ldsrc,
                     float *dst, int64_t lddst, int32_t d, bbgr_stream_t stream);

/* bbgr_scatter_add_rows for DISTINCT indices (ABI 6): dst[idx[k], :d] +=     */
/* (0 + src[k, :d]), the same additions a one-addend segment makes, in one   */
/* launch without the sort (a training batch of distinct users). Negative or */
/* >= n_dst indices are skipped; repeated indices are the caller's error.    */
int bbgr_rows_add_unique(int64_t n, const int64_t *idx, const float *src, int64_t ldsrc,
                         float *dst, int64_t lddst, int32_t d, int64_t n_dst,
                         bbgr_stream_t stream);

/* slot[k] = the first k' <= k with ids[k'] == ids[k], for k < n (ABI 6; ids */
/* in [0, n_rows)). first: int32 [n_rows] scratch holding INT32_MAX at every */
/* row (left so on return). The BPR ego rows' "add into the row of the first */
/* occurrence" without a sort: an atomic minimum per row (order-free, so    */
/* deterministic), a gather, and a reset of the touched rows.              */
int bbgr_first_slot(int64_t n, const int64_t *ids, int64_t n_rows, int32_t *first,
                    int64_t *slot, bbgr_stream_t stream);

/* The ego rows' slots of a batch of B (user, pos, neg) triples in three     */
/* launches (ABI 8; bpr.ego_grad_rows, the drop-in step's BPR backward,      */
/* Version-2/lighgcn_cu_pop.py:389-397):                                      */
/*   iu[b] = clamp(users[b], 0, n_users - 1);                                 */
/*   ii[b] = clamp(pos[b], 0, n_items - 1), ii[B + b] = clamp(neg[b], ...);   */
/*   cu[b] = the first b' with iu[b'] == iu[b], or -1 when any id of triple  */
/*           b lies outside its table;                                        */
/*   sp[b] / sn[b] = the first j with ii[j] == ii[b] / ii[B + b].             */
/* first_u [n_users] / first_i [n_items]: int32 scratch holding INT32_MAX at */
/* every row (left so on return), as bbgr_first_slot's.                       */
int bbgr_ego_slots(int64_t B, const int64_t *users, const int64_t *pos, const int64_t *neg,
                   int64_t n_users, int64_t n_items, int32_t *first_u, int32_t *first_i,
                   int64_t *iu, int64_t *ii, int64_t *cu, int64_t *sp, int64_t *sn,
                   bbgr_stream_t stream);

/* The ego-L2 gradient rows of a batch in first-slot form (ABI 10; the       */
/* drop-in step's BPR backward), from bbgr_ego_slots' outputs: slot s of     */
/* g_u [B, d] (s < B, user iu[s]) and of g_i [2B, d] (item ii[s]) receives    */
/* y = (2 reg dloss / B) * e, e its ego row (ue[iu[s]] / ie[ii[s]]), added n  */
/* times from +0.0, n = the slot's occurrences as a first slot (cu / sp / sn) */
/* among the valid triples (cu[b] >= 0); other slots are written zero. Bitwise */
/* bbgr_bpr's ego rows over the compact tables (identical addends, so its     */
/* float atomics' order cannot matter) without their serialisation on a       */
/* popular item's row. counts: int32 [3B] scratch, zero on entry and return.  */
/* scale: every written row is that sum times scale (one rounding; 1 = the    */
/* sum itself; the in-backward Adam's (K+1) * ego rows without a mul launch). */
/* counts_u_out (nullable, int32 [B]): slot s < B's user count n (0 off the   */
/* first slots), for bbgr_rows_add_slots over the same cu.                    */
/* d in {8, 16, 32, 64, 128, 256}; any other width returns                    */
/* BBGR_ERR_UNSUPPORTED before a launch.                                      */
int bbgr_ego_rows(int64_t B, int32_t d, const int64_t *cu, const int64_t *sp, const int64_t *sn,
                  const int64_t *iu, const int64_t *ii, const float *ue, int64_t ldue,
                  const float *ie, int64_t ldie, const float *dloss, float reg, int32_t *counts,
                  float *g_u, int64_t ldgu, float *g_i, int64_t ldgi, float scale,
                  int32_t *counts_u_out, bbgr_stream_t stream);

/* A row scatter in first-slot form (ABI 10): for every k < n with          */
/* counts[k] > 0 (a leader: counts[k] valid slots k' have slot[k'] == k;    */
/* bbgr_ego_slots' cu and bbgr_ego_rows' counts_u_out), dst[rows[k], :d] +=  */
/* (0 + src[k] + src[k2] + ...) over k and those k' > k in ascending order.  */
/* Bitwise bbgr_scatter_add_rows of the batch's rows (a stable sort's        */
/* segment sums) when the slots of invalid triples (slot -1) hold zero rows, */
/* without the sort (a batch of distinct users: one read per row).          */
int bbgr_rows_add_slots(int64_t n, const int64_t *slot, const int32_t *counts,
                        const int64_t *rows, const float *src, int64_t ldsrc, float *dst,
                        int64_t lddst, int32_t d, int64_t n_dst, bbgr_stream_t stream);

/* out[k] = rank[ids[k]] (rank NULL: ids[k]) for ids[k] in [0, n_rows), else */
/* -1 (ABI 8): a caller's row ids as graph rows in one launch                */
/* (bbgr::propagate_rows' batch lists; the marking kernels skip the -1).     */
int bbgr_graph_rows(int64_t n, const int64_t *ids, int64_t n_rows, const int64_t *rank,
                    int64_t *out, bbgr_stream_t stream);

/* Deterministic index_add_: dst[idx[k], :d] += src[k, :d] for k < n, with   */
/* the addends of each destination row summed in ascending k and added once  */
/* (stable radix sort of idx, then one segment sum per row). Negative or     */
/* >= n_dst indices are skipped. Replaces the autograd scatter of the BPR    */
/* gradient and Tensor.index_add_ (main.py:645-650 scatter_add).             */
int bbgr_scatter_add_rows(int64_t n, const int64_t *idx, const float *src, int64_t ldsrc,
                          float *dst, int64_t lddst, int32_t d, int64_t n_dst,
                          void *workspace, size_t *workspace_bytes, bbgr_stream_t stream);
/* bbgr_scatter_add_rows in two halves (ABI 8), so one sort serves several  */
/* scatters over the same index list (the drop-in backward scatters its     */
/* item rows into two tables and its user rows twice).                      */
/* bbgr_scatter_plan: the stable order of idx into `plan` (device; query    */
/* plan_bytes with plan == NULL: bbgr_scatter_add_rows' workspace size).    */
int bbgr_scatter_plan(int64_t n, const int64_t *idx, int64_t n_dst, void *plan,
                      size_t *plan_bytes, bbgr_stream_t stream);
/* bbgr_scatter_apply: dst[r, :d] += (the ascending sum over k with         */
/* idx[k] == r of src[k, :d], continued over src2[k, :d] when src2 is not    */
/* NULL), each row added once: bitwise bbgr_scatter_add_rows over the        */
/* concatenation [src; src2] with the index list [idx; idx]. n, n_dst and    */
/* idx as planned; the plan may be applied any number of times.             */
int bbgr_scatter_apply(int64_t n, int64_t n_dst, const void *plan, const float *src,
                       int64_t ldsrc, const float *src2, int64_t ldsrc2, float *dst,
                       int64_t lddst, int32_t d, bbgr_stream_t stream);

/* ------------------------------------------------------------------------- */
/* Credibility-GNN edge weights, main.py:677-701:       */
/*   CredModel.ewa_raw: w = max(beta*clamp(attr[:,col_verified],0,1) +       */
/*                              gamma*attr[:,col_align], 0)                  */
/*   CredModel.normalize_per_dst: w~ = w / (sum of w over the edge's dst +   */
/*                                1e-12 (eps))                               */
/* csr: destination-row CSR of the edges (bbgr_csr_build with perm_out);     */
/* perm[k]: input edge id of CSR slot k. w_in (nullable, input-edge order)   */
/* replaces the EWA formula (normalize_per_dst on given weights). Outputs    */
/* (each nullable): w_raw and w_edge in input-edge order, w_csr in CSR order */
/* (the edge values of the aggregation SpMM, CredModel.aggregate = bbgr_spmm */
/* over this CSR). The csr must carry its load-balance plan; per-row sums    */
/* follow it in a fixed order (bitwise deterministic). dst (nullable, input  */
/* order): each edge's destination row; with it w_edge is written by one     */
/* coalesced pass over the edges instead of a scatter through perm.          */
/* Workspace: raw weights in CSR order, per-row sums, chunk partials (+ raw  */
/* weights in input order when w_in and w_raw are both NULL).                */
/* ------------------------------------------------------------------------- */
int bbgr_ewa_normalize(const bbgr_csr *csr, const int32_t *perm, const int32_t *dst,
                       const float *w_in,
                       const float *edge_attr, int64_t lda, int32_t col_verified,
                       int32_t col_align, float beta, float gamma, float eps,
                       float *w_raw, float *w_edge, float *w_csr, void *workspace,
                       size_t *workspace_bytes, bbgr_stream_t stream);

/* mask[idx[k]] = value for k < n; indices outside [0, n_rows) (the sampler's
 * -1, or a caller's stale tail) are skipped. */
int bbgr_mark_rows(int64_t n, const int64_t *idx, uint8_t value, uint8_t *mask,
                   int64_t n_rows, bbgr_stream_t stream);
/* For each listed row r = rows[k]: mask[indices[e]] = value for every edge e of
 * row r (the neighbourhood frontier of a batch). */
int bbgr_mark_neighbors(int64_t n, const int64_t *rows, const int32_t *indptr,
                        const int32_t *indices, uint8_t value, uint8_t *mask,
                        bbgr_stream_t stream);
/* Flag rows in mask and list each newly flagged row once: indptr == NULL —
 * the rows rows[k] (k < n; negative / >= n_rows skipped); else every column
 * indices[e] of every edge e of row rows[k]. A row whose byte was 0 is set to
 * 1 and appended at list[(*count)++] (count: DEVICE int64, list order
 * unspecified; rows already flagged are not listed again). mask: 4-byte
 * aligned, its allocation a whole number of 4-byte words. The frontier of a
 * step as a row list without a scan of the mask (bbgr_spmm_args.row_count). */
int bbgr_mark_list(int64_t n, const int64_t *rows, const int32_t *indptr,
                   const int32_t *indices, uint8_t *mask, int64_t n_rows, int64_t *list,
                   int64_t *count, bbgr_stream_t stream);
/* Slot bitmaps (bbgr_spmm_args.src_bits). tmap = bbgr_transpose_slots of the  */
/* CSR whose rows are listed: for every edge e of row rows[k] (k < n), bit     */
/* tmap[e] of bits is set (set != 0), or its whole 32-bit word cleared          */
/* (set == 0: restores an all-zero bitmap after use). Negative rows skipped.   */
int bbgr_mark_slots(int64_t n, const int64_t *rows, const int32_t *indptr,
                    const int32_t *tmap, uint32_t *bits, int32_t set,
                    bbgr_stream_t stream);
/* A training step's batch bookkeeping in one launch each (ABI 10; the fused  */
/* trainer's frontier step). bbgr_batch_begin = bbgr_mark_rows(users, 1,      */
/* mask_u) + bbgr_mark_list(pos, neg -> mask_i, list) + (user_indptr != NULL) */
/* bbgr_mark_list(every neighbour of the users -> mask_i, list) +            */
/* (slot_bits != NULL) bbgr_mark_slots(users, set); the same masks, list SET */
/* (its order unspecified either way) and bits. bbgr_batch_end restores them:*/
/* mask_u / mask_i bytes of the users, items and neighbours to 0, the slot    */
/* words to 0, *count to 0 (list != NULL), and zeroes the step's sparse       */
/* gradient rows: g_u at the users, g_i and g_side (each nullable) at pos and */
/* neg (d columns). Ids outside the tables (the sampler's -1) are skipped.    */
typedef struct {
  int64_t batch;
  const int64_t *users, *pos, *neg;   /* internal row ids */
  int64_t n_users, n_items;
  const int32_t *user_indptr, *user_indices;   /* user CSR; NULL: no neighbours */
  uint8_t *mask_u, *mask_i;
  int64_t *list, *count;              /* item frontier list (nullable together) */
  const int32_t *slot_map;            /* with slot_bits (nullable together) */
  uint32_t *slot_bits;
  float *g_u, *g_i, *g_side;          /* bbgr_batch_end only, nullable */
  int64_t ld_gu, ld_gi, ld_side;
  int32_t d;
} bbgr_batch_args;
int bbgr_batch_begin(const bbgr_batch_args *args, bbgr_stream_t stream);
/* bits[w] = OR over b < 32 of (mask[32 w + b] != 0) << b, for every word    */
/* w < ceil(n / 32) (ABI 10): a byte mask packed for bbgr_spmm_args.         */
/* src_mask_bits (the bits past n are 0).                                    */
int bbgr_mask_pack(int64_t n, const uint8_t *mask, uint32_t *bits, bbgr_stream_t stream);
int bbgr_batch_end(const bbgr_batch_args *args, bbgr_stream_t stream);
/* The row marking of one bbgr::propagate_rows call in one launch (ABI 11): */
/* the listed users users[k] (k < n_users_listed) and items items[k] (k <    */
/* n_items_listed), caller ids, mapped to graph rows through user_rank /     */
/* item_rank (NULL: the ids are the rows). The same masks, list SETS (orders */
/* unspecified) and counts as bbgr_mark_list(user rows -> mask_u, user_list) */
/* + bbgr_mark_rows(item rows, 1, mask_i) + bbgr_mark_list(item rows ->      */
/* frontier, frontier_list) + (user_indptr != NULL) bbgr_mark_list(every     */
/* neighbour of the user rows in the graph-order user CSR -> frontier,       */
/* frontier_list) + (each nullable) bbgr_mark_rows(users, 1, mask_u_in) and  */
/* bbgr_mark_rows(items, 1, mask_i_in) in the caller's order. Ids outside    */
/* the tables (the sampler's -1) are skipped. mask_u / frontier: 4-byte      */
/* aligned whole words (bbgr_mark_list); the counts are DEVICE int64.        */
typedef struct {
  int64_t n_users_listed, n_items_listed;
  const int64_t *users, *items;                /* caller ids */
  int64_t n_users, n_items;
  const int64_t *user_rank, *item_rank;        /* caller id -> graph row; nullable */
  const int32_t *user_indptr, *user_indices;   /* graph-order user CSR; nullable together */
  uint8_t *mask_u, *mask_i, *frontier;         /* graph order */
  uint8_t *mask_u_in, *mask_i_in;              /* caller order; nullable */
  int64_t *user_list, *user_count, *frontier_list, *frontier_count;
} bbgr_rows_mark_args;
int bbgr_rows_mark(const bbgr_rows_mark_args *args, bbgr_stream_t stream);
/* The same for every CSR row r < n_rows flagged in row_mask: row_mask[r], or
 * row_mask[row_map[r]] when row_map is given (a mask kept in the caller's
 * vertex order over a CSR numbered by descending degree). */
int bbgr_mark_neighbors_of_mask(int64_t n_rows, const uint8_t *row_mask,
                                const int32_t *row_map, const int32_t *indptr,
                                const int32_t *indices, uint8_t value, uint8_t *mask,
                                bbgr_stream_t stream);

/* mask[r] = 1 if row r of x [n_rows, d] (leading dimension ldx) holds a
 * nonzero, else 0 (every row written; -0.0 counts as zero). With a CSR
 * (indptr, indices over the rows of x): nbr_mask[indices[e]] = 1 for every edge
 * of a flagged row (other entries untouched). The gradient support of a
 * backward pass whose caller did not say which rows are live (the registered
 * propagate_backward op: BPR gradients touch only the batch rows). */
int bbgr_row_support(int64_t n_rows, int32_t d, const float *x, int64_t ldx, uint8_t *mask,
                     const int32_t *indptr, const int32_t *indices, uint8_t *nbr_mask,
                     bbgr_stream_t stream);

/* ------------------------------------------------------------------------- */
/* Item exchange over RCCL (the sharded step's per-layer all-reduce of item   */
/* partial sums) for callers without torch.distributed.        */
/* RCCL is resolved at run time (librccl.so.1: the copy already loaded in the */
/* process, else the library path). The communicator is an ncclComm_t.       */
/* ------------------------------------------------------------------------- */
/* id_out: 128 bytes (ncclUniqueId) to hand to every rank (rank 0 creates).  */
int bbgr_comm_unique_id(uint8_t *id_out);
/* Collective over nranks processes (blocks until all have joined); the      */
/* calling thread's current HIP device is the rank's GPU.                    */
int bbgr_comm_init(void **comm_out, int32_t nranks, int32_t rank, const uint8_t *id);
int bbgr_comm_destroy(void *comm);
/* In-place sum over the ranks of items[count] (fp32), stream-ordered.       */
int bbgr_allreduce_items(void *comm, float *items, int64_t count, bbgr_stream_t stream);
/* The sharded step's other collectives on the same communicator (ABI 6), so */
/* a caller can keep EVERY collective of a step on its compute stream, in    */
/* issue order (no hop to a comm stream and back): in-place all-reduce of    */
/* buf[count] and all-gather of count elements per rank into recv[nranks *   */
/* count] (rank-major). dtype: bbgr_dtype; op: bbgr_redop.                   */
typedef enum { BBGR_DT_U8 = 0, BBGR_DT_I32 = 1, BBGR_DT_I64 = 2, BBGR_DT_F32 = 3 } bbgr_dtype;
typedef enum { BBGR_RED_SUM = 0, BBGR_RED_MAX = 1, BBGR_RED_MIN = 2 } bbgr_redop;
int bbgr_comm_allreduce(void *comm, void *buf, int64_t count, int32_t dtype, int32_t op,
                        bbgr_stream_t stream);
int bbgr_comm_allgather(void *comm, const void *send, void *recv, int64_t count,
                        int32_t dtype, bbgr_stream_t stream);

/* ------------------------------------------------------------------------- */
/* Negative / positive sampling                                               */
/*   Replaces the per-user host loop of Version-2/lighgcn_cu_pop.py:835-849:  */
/*   sample_pos_item (:339-343), sample_neg_item_popmix (:349-376),           */
/*   user_has_item (:330-336), uniform sample_neg_item (lightgcn.py:296-300), */
/*   and pop_prob = (deg_i+1)^gamma / (sum + 1e-12)  (:805-810).              */
/* RNG: Philox4x32-10, key = seed, counter = (counter, slot, draw).           */
/* ------------------------------------------------------------------------- */
/* cdf[i] = normalised inclusive prefix sum of (deg_i + 1)^gamma (fp64), the
 * table numpy's Generator.choice(p=pop_prob) searches. */
int bbgr_pop_cdf(int32_t n_items, const int32_t *indptr_i, double gamma,
                 double *cdf, void *workspace, size_t *workspace_bytes,
                 bbgr_stream_t stream);

/* For each b < batch, user u = users[b]:
 *   pos[b] = indices[indptr[u] + floor(U01 * deg_u)]   (-1 if deg_u == 0)
 *   neg[b] = first of <= max_tries candidates not in row u, each drawn from
 *            the pop CDF with probability mix_pop (cdf != NULL) else uniform;
 *            then uniform draws until one is not in row u (capped at
 *            BBGR_NEG_CAP draws; -1 and *fail_count += 1 if none found).
 * indices must be sorted within each row (bbgr_csr_build guarantees it). */
#define BBGR_NEG_CAP 65536
int bbgr_sample(int64_t batch, const int64_t *users, const int32_t *indptr,
                const int32_t *indices, int32_t n_items, const double *cdf,
                float mix_pop, int32_t max_tries, uint64_t seed,
                uint64_t counter, int64_t *pos, int64_t *neg,
                int32_t *fail_count, bbgr_stream_t stream);
int bbgr_sample_dev(int64_t batch, const int64_t *users, const int32_t *indptr,
                    const int32_t *indices, int32_t n_items, const double *cdf,
                    float mix_pop, int32_t max_tries, uint64_t seed,
                    const int64_t *state, int64_t *pos, int64_t *neg,
                    int32_t *fail_count, bbgr_stream_t stream);

/* out = a random permutation of in[0..n) (Philox keys + radix sort), the
 * device form of rng.shuffle(train_users) (Version-2:821). */
int bbgr_shuffle(int64_t n, const int64_t *in, int64_t *out, uint64_t seed,
                 uint64_t counter, void *workspace, size_t *workspace_bytes,
                 bbgr_stream_t stream);

/* Users with at least one edge: out[0..*count) ascending (Version-2:797-798).
 * *count is a DEVICE int64. */
int bbgr_nonempty_rows(int32_t n_rows, const int32_t *indptr, int64_t *out,
                       int64_t *count, void *workspace, size_t *workspace_bytes,
                       bbgr_stream_t stream);

/* Rows flagged in mask[n] (any non-zero byte): out[0..*count) ascending.
 * *count is a DEVICE int64. Same workspace protocol. */
int bbgr_mask_to_list(int64_t n, const uint8_t *mask, int64_t *out, int64_t *count,
                      void *workspace, size_t *workspace_bytes, bbgr_stream_t stream);

/* offs[k] = number of entries of the ascending list[0..*count) below
 * bounds[k] (k < n_bounds; *count is a DEVICE int64): the split of a
 * bbgr_mask_to_list row list at row-range boundaries, computed on the stream
 * so the host copies n_bounds values instead of scanning the mask. */
int bbgr_list_offsets(int32_t n_bounds, const int64_t *bounds, const int64_t *list,
                      const int64_t *count, int64_t *offs, bbgr_stream_t stream);

/* pos[list[j]] = j for j < *count (n_max >= *count: the launch size; list
 * entries < the length of pos; other entries of pos are left alone). With
 * pos as an SpMM's y_map, a row-list product writes listed row list[j]
 * straight to row j of a compact table (the sparse item exchange's payload). */
int bbgr_list_positions(int64_t n_max, const int64_t *list, const int64_t *count,
                        int32_t *pos, bbgr_stream_t stream);

/* ------------------------------------------------------------------------- */
/* Evaluation                                            */
/*   bbgr_eval_sampled replaces evaluate_sampled,                             */
/*   Version-2/lighgcn_cu_pop.py:536-650; bbgr_eval_full replaces             */
/*   evaluate_full_ranking, :652-752 (both + metrics_at_k :514-531,           */
/*   novelty_stats_for_items :390-405).                                       */
/* users[n_users]: the evaluated users (rows of the test CSR that are not     */
/* empty, ascending). group[b]: bit0 = top-pct credibility user, bit1 =       */
/* bottom-pct (make_cred_groups :405-422; nullable).                          */
/* Sampled: pos uniform from the test row, n_neg negatives uniform from       */
/*   [0, n_items) rejecting test and train items (duplicates allowed),        */
/*   1+n_neg candidates scored <uf[u], itf[c]> and ranked descending, ties    */
/*   in candidate order (pos first). Writes pos_rank[n_users],                */
/*   topk[n_users*k_max] (-1 padded), optional cand_out[n_users*(1+n_neg)].   */
/*   cand_in (nullable, ABI 10): the candidates are taken from                */
/*   cand_in[b*(1+n_neg) + c] (c = 0 the positive) instead of drawn; the      */
/*   reference's own numpy stream, drawn by bbgr_eval_draw_candidates.        */
/* Full: every item scored <uf[u], itf[i]> with fp32 MFMA (one fmaf chain    */
/*   per score, components in the order 0, d/2, 1, d/2+1, ...), train items   */
/*   set to -1e9, ranked by (score desc, item asc); topk[n_users*k_max] and   */
/*   optional topk_score[n_users*k_max]. k_max <= 32, d in {64, 128}.         */
/* Both write sums[n_k*11] (double) per K =                                   */
/*   {sum P, sum R, sum NDCG, sum avg log(pop+1), sum avg self-info,          */
/*    sum R over high-cred users, sum R over low-cred users, #high, #low,     */
/*    #evaluated users, #distinct top-K items (coverage numerator)},          */
/* reduced in a fixed order (bitwise reproducible).                           */
/* ------------------------------------------------------------------------- */
typedef struct {
  int64_t n_users;
  const int64_t *users;
  const int32_t *te_indptr;
  const int32_t *te_indices;
  const int32_t *tr_indptr;
  const int32_t *tr_indices;
  const float *uf;
  int64_t lduf;
  const float *itf;
  int64_t ldif;
  int32_t d;
  int32_t n_items;
  int32_t n_neg;           /* sampled only */
  int32_t k_max;
  int32_t n_k;
  int32_t ks[8];
  uint64_t seed;           /* sampled only */
  uint64_t counter;        /* sampled only */
  const float *item_pop;
  float self_info_denom;   /* total_train_interactions + n_items */
  const uint8_t *group;
  int32_t *pos_rank;       /* sampled only */
  int32_t *topk;
  float *topk_score;       /* full only, nullable */
  int32_t *cand_out;       /* sampled only, nullable */
  int32_t *fail_count;     /* sampled only, nullable */
  double *sums;
  const int32_t *cand_in;  /* sampled only, nullable (ABI 10) */
} bbgr_eval_args;

int bbgr_eval_sampled(const bbgr_eval_args *args, void *workspace, size_t *workspace_bytes,
                      bbgr_stream_t stream);
int bbgr_eval_full(const bbgr_eval_args *args, void *workspace, size_t *workspace_bytes,
                   bbgr_stream_t stream);

/* The reference's candidate draws, bit for bit (HOST code, host arrays; ABI  */
/* 10). evaluate_sampled (Version-2/lighgcn_cu_pop.py:554-589, the same loop  */
/* in lightgcn.py:406-429, lightgcn_cu.py:496-519,                            */
/* version_1/lightgcn_cu_pop_long_tail_exposure.py:494-517) draws from        */
/* np.random.default_rng(seed + 999), per evaluated user u in order:          */
/*   pos = gt[rng.integers(0, len(gt))]  (gt = the user's test row)           */
/*   repeat until n_neg: j = rng.integers(0, n_items); skip j if j is in gt   */
/*   or user_has_item(train, u, j) (np.searchsorted in the train row, :330);  */
/*   otherwise append j (duplicates kept).                                    */
/* rng is numpy's PCG64 bit generator state (bit_generator.state: the 128-bit */
/* state and increment, has_uint32, uinteger), advanced in place exactly as   */
/* numpy advances it: scalar integers(0, n) on int64 is Lemire's bounded      */
/* draw on buffered 32-bit outputs (n - 1 < 2^32; 64-bit outputs above).      */
/* cand[b*(1+n_neg) + c]: c = 0 the positive, 1.. the negatives. users must   */
/* have non-empty test rows. Returns BBGR_ERR_INVALID if a user cannot get    */
/* n_neg negatives (the reference's loop would not end).                      */
typedef struct {
  uint64_t state_hi, state_lo;   /* the 128-bit LCG state */
  uint64_t inc_hi, inc_lo;       /* the 128-bit increment (odd) */
  int32_t has_uint32;
  uint32_t uinteger;
} bbgr_pcg64;
int bbgr_eval_draw_candidates(bbgr_pcg64 *rng, int64_t n_users, const int64_t *users,
                              const int64_t *te_indptr, const int64_t *te_indices,
                              const int64_t *tr_indptr, const int64_t *tr_indices,
                              int64_t n_items, int32_t n_neg, int32_t *cand);

/* The metrics reduction of the full protocol over CALLER-SUPPLIED lists       */
/* (added under ABI 12): sums[n_k*11] exactly as bbgr_eval_full forms them,   */
/* from args->topk[n_users*k_max] (entries of -1 are skipped: they hit        */
/* nothing, cover nothing and do not count in the novelty means). The lists   */
/* may come from bbgr_recommend. k_max <= 128; uf / itf / d, the train CSR    */
/* and the sampled-only fields are ignored. Same two-call workspace idiom.    */
int bbgr_eval_lists(const bbgr_eval_args *args, void *workspace, size_t *workspace_bytes,
                    bbgr_stream_t stream);

/* ------------------------------------------------------------------------- */
/* Recommendation lists (added under ABI 12)                                  */
/* The top-k items of users[n_users] (int64 rows of uf, any order, duplicates */
/* allowed; every id in [0, n_user_rows)), 1 <= k <= 128, d in {64, 128,      */
/* 256}. Scores are bbgr_eval_full's: <uf[u], itf[i]> as one fp32 fma chain   */
/* over the components 0, d/2, 1, d/2+1, ... (fp32 MFMA); order is (score     */
/* desc, item asc). Only finite scores rank.                                  */
/* ex_indptr[n_user_rows+1] / ex_indices (nullable together): a CSR over user */
/*   ids of items to leave out, rows sorted ascending, duplicates allowed.    */
/*   Excluded items are dropped, not scored low.                              */
/* item_mask (nullable, uint8 [n_items]): nonzero = eligible.                 */
/* topk[n_users*k] int32, topk_score[n_users*k] float (nullable): a user with */
/*   fewer than k eligible items gets -1 / -INFINITY in the tail.             */
/* k above the kernel's register list depth (16 or 24) runs ceil(k / depth)   */
/* scoring passes, each continuing after the last pair of the one before;     */
/* the result is the exact top-k. workspace == NULL queries the size;         */
/* n_users == 0 returns BBGR_OK without a launch. BBGR_ERR_INVALID names the  */
/* offending field; d outside {64, 128, 256} is BBGR_ERR_UNSUPPORTED.         */
/* ------------------------------------------------------------------------- */
typedef struct {
  int64_t n_users;
  const int64_t *users;
  int64_t n_user_rows;
  const float *uf;
  int64_t lduf;
  const float *itf;
  int64_t ldif;
  int32_t d;
  int32_t n_items;
  int32_t k;
  const int32_t *ex_indptr;
  const int32_t *ex_indices;
  const uint8_t *item_mask;
  int32_t *topk;
  float *topk_score;
} bbgr_recommend_args;

int bbgr_recommend(const bbgr_recommend_args *args, void *workspace, size_t *workspace_bytes,
                   bbgr_stream_t stream);

/* ------------------------------------------------------------------------- */
/* bf16 recommendation lists, and exact fp32 lists by rescoring (opt-in;      */
/* additions to ABI 12)                                                       */
/*                                                                            */
/* bbgr_recommend_bf16: bbgr_recommend on bf16 tables (bbgr_to_bf16's output: */
/* 16-byte aligned, ld >= d, ld % 8 == 0 elements), every other field with    */
/* its meaning above. A score is the fp32-accumulated product of the bf16     */
/* rows (v_mfma_f32_32x32x16_bf16; products of two bf16 are exact in fp32);   */
/* the lists are the exact top-k of THOSE scores, order (score desc, item     */
/* asc), continuation passes and tie groups included. Same two-call workspace */
/* idiom, same refusals; two launches over the same inputs give equal bits.   */
/* ------------------------------------------------------------------------- */
typedef struct {
  int64_t n_users;
  const int64_t *users;
  int64_t n_user_rows;
  const uint16_t *uf;
  int64_t lduf;
  const uint16_t *itf;
  int64_t ldif;
  int32_t d;
  int32_t n_items;
  int32_t k;
  const int32_t *ex_indptr;
  const int32_t *ex_indices;
  const uint8_t *item_mask;
  int32_t *topk;
  float *topk_score;
} bbgr_recommend_bf16_args;

int bbgr_recommend_bf16(const bbgr_recommend_bf16_args *args, void *workspace,
                        size_t *workspace_bytes, bbgr_stream_t stream);

/* out[0] = an upper bound of max_r ||src[r, :]||_2 over the n_rows rows of   */
/* an fp32 table (16-byte aligned, ld >= d, ld % 4 == 0; d a multiple of 4,   */
/* 4 <= d <= 256): per row an fp32 sum of squares in a fixed order (at most   */
/* 20 roundings), its square root, times 1 + 2^-20, plus 2^-58 for squares    */
/* that underflow: never below the true norm, and at most the true norm times */
/* 1 + 2^-19 plus 2^-58.                                                      */
/* A row holding a NaN gives NaN. On the device: no host read, no float       */
/* atomic (an integer max of the non-negative bit patterns: any order gives   */
/* the same bits). n_rows == 0 writes 0.                                      */
int bbgr_row_norm_max(int64_t n_rows, int32_t d, const float *src, int64_t ld, float *out,
                      bbgr_stream_t stream);

/* The fp32 top-k of each user among the k_pre candidates of a bf16 pass, and */
/* the proof that it is the user's fp32 list.                                 */
/*   cand / cand_score [n_users * k_pre]: bbgr_recommend_bf16's topk /        */
/*     topk_score at k = k_pre over the bf16 roundings of uf / itf, with the  */
/*     caller's exclusion and mask (-1 / -INFINITY in the tail of a row).     */
/*   n_max: device scalar, an upper bound of max_i ||itf[i]||_2               */
/*     (bbgr_row_norm_max). 1 <= k <= k_pre <= 128; d in {64, 128, 256}.      */
/* Every candidate is scored with bbgr_recommend's fma chain (components 0,   */
/* d/2, 1, d/2+1, ...), sorted (score desc, item asc); topk / topk_score      */
/* (nullable) [n_users * k] take the first k, -1 / -INFINITY past the end.    */
/* certified[b] = 1 when the row is proven to be bbgr_recommend's row, bit    */
/* for bit: the norms are finite and at most 2^60, every candidate's fp32     */
/* score is finite, and either the candidate row is not full (it holds every  */
/* eligible item) or the k-th fp32 score is strictly greater than             */
/* cand_score[k_pre - 1] + E_u, E_u = eps(d) * ||uf[u]|| * n_max plus the     */
/* underflow terms 2^-121 (||uf[u]|| + n_max) + 2^-116, eps(d) = 1.02 * 2^-7  */
/* + d * 2^-21 (the derivation is in csrc/recommend_bf16.hip). A row with     */
/* certified[b] = 0 must be recomputed by bbgr_recommend. No workspace.       */
typedef struct {
  int64_t n_users;
  const int64_t *users;
  int64_t n_user_rows;
  const float *uf;
  int64_t lduf;
  const float *itf;
  int64_t ldif;
  int32_t d;
  int32_t n_items;
  int32_t k;
  int32_t k_pre;
  const int32_t *cand;
  const float *cand_score;
  const float *n_max;
  int32_t *topk;
  float *topk_score;
  uint8_t *certified;
} bbgr_recommend_rescore_args;

int bbgr_recommend_rescore(const bbgr_recommend_rescore_args *args, bbgr_stream_t stream);

/* ------------------------------------------------------------------------- */
/* SLAS subgraph sampling for the credibility GNN (added under ABI 12)        */
/*   Replaces build_slas_subgraph and its helpers, main.py:727-883: a host    */
/*   loop per seed user, per sampled item and per edge of every subgraph      */
/*   user, three times per training step.                                     */
/* The reference-order CSR (build_csr_from_src, main.py:739-749, a stable     */
/* sort by source): indptr[n_rows+1], and per slot the neighbour id nbr[] and */
/* the input edge id eid[], a row's slots in ascending edge id. One way to    */
/* build it: bbgr_csr_build with the edge id as the column (n_cols = E); its  */
/* indices are then eid[], and nbr[] = dst[eid[]].                            */
/* view: BBGR_SLAS_VIEW_EARLY keeps the slots with ts[eid * ts_stride] <      */
/* split, BBGR_SLAS_VIEW_LATE those with ts >= split (a value equal to split  */
/* is late); ts is one float per edge id (pointer + stride in floats, so a    */
/* column of edge_attr is passed in place) and may be NULL with VIEW_NONE.    */
/* ------------------------------------------------------------------------- */
typedef enum {
  BBGR_SLAS_VIEW_NONE = 0,
  BBGR_SLAS_VIEW_EARLY = 1,
  BBGR_SLAS_VIEW_LATE = 2
} bbgr_slas_view;

/* Similarity profiles (main.py:727-737), fp32 row-major, 1 <= F <= 16:       */
/*   item_norm[i] = item_x[i] / (|item_x[i]|_2 + 1e-12)      [n_items, F]     */
/*   user_mu[u]   = l2n((sum over the slots of row u of item_norm[nbr_u]) /   */
/*                  max(deg_u, 1)), with multiplicity        [n_users, F]     */
/* l2n in the same + 1e-12 form. item_x has leading dimension ldx >= F. The   */
/* sums run in a fixed order without float atomics: two calls, same bits.     */
int bbgr_slas_profiles(int32_t n_users, int32_t n_items, int32_t F, const float *item_x,
                       int64_t ldx, const int32_t *indptr_u, const int32_t *nbr_u,
                       float *item_norm, float *user_mu, bbgr_stream_t stream);

/* A weighted sample without replacement of at most k slots of each listed    */
/* row (slas_sample_items_for_user / slas_sample_users_for_item,              */
/* main.py:758-807; one entry point serves both directions). With m eligible  */
/* slots (after the view filter): m == 0 gives count 0; m <= k gives every    */
/* eligible slot in row order (no randomness); otherwise slot j has the       */
/* weight w_j = exp(kappa * <nbr_profile[nbr_j], row_profile[row]>) in fp32,  */
/* times (1 + upweight) where label[nbr_j] >= 0 (label nullable, int64 per    */
/* neighbour-side id), and the key -log(U_j) / w_j; the k smallest keys win,  */
/* written in ascending key order, equal keys the lower slot first. These     */
/* exponential clocks are successive sampling with probabilities proportional */
/* to w: the distribution of rng.choice(m, k, replace=False, p=w/sum(w)).     */
/* U_j in (0, 1] is the first word of Philox4x32-10 with key = seed and       */
/* counter = {counter, stage, row id, slot position in the row}: a row's      */
/* picks are a pure function of seed, counter, stage and that row, whatever   */
/* else is listed and however the launch is shaped. stage in [0, 255].        */
/* rows[n]: int64 global row ids (outside [0, n_rows): count 0).              */
/* out_nbr / out_eid [n, k] int32, unused entries -1; out_count[n] int32.     */
/* Duplicate edges are separate slots: out_eid never repeats within a row.    */
/* One wave per row, the running best k held one per lane and merged with     */
/* each 64-slot chunk across the lanes; a row above 1024 slots is dealt out   */
/* to the 16 waves of a workgroup (same picks): no row is bound by one lane's */
/* loop, and a hub row not by one wave's.                                     */
/* 1 <= k <= 64, 1 <= F <= 16; n == 0 returns BBGR_OK without a launch.       */
typedef struct {
  int64_t n;
  const int64_t *rows;
  int64_t n_rows;
  const int32_t *indptr;
  const int32_t *nbr;
  const int32_t *eid;
  const float *row_profile;  /* [n_rows, F] */
  const float *nbr_profile;  /* [neighbour-side rows, F] */
  int32_t F;
  float kappa;
  int32_t k;
  const float *ts;           /* nullable with BBGR_SLAS_VIEW_NONE */
  int64_t ts_stride;
  int32_t view;
  float split;
  const int64_t *label;      /* nullable */
  float upweight;
  uint64_t seed;
  uint32_t counter;
  uint32_t stage;
  int32_t *out_nbr;
  int32_t *out_eid;
  int32_t *out_count;
} bbgr_slas_sample_args;
int bbgr_slas_sample(const bbgr_slas_sample_args *args, bbgr_stream_t stream);

/* mask[ids[j]] = value for j < n where 0 <= ids[j] < n_rows: the marking of  */
/* a -1-padded int32 list (bbgr_slas_sample's out_nbr); with                   */
/* bbgr_mask_to_list the ascending distinct ids (np.unique, main.py:815,820). */
int bbgr_mark_ids32(int64_t n, const int32_t *ids, uint8_t value, uint8_t *mask,
                    int64_t n_rows, bbgr_stream_t stream);

/* The induced edge list (main.py:835-856): for each user of users[] in list  */
/* order (distinct global ids), over its row of the user-row CSR in row       */
/* order, every eligible slot (view filter) whose item is sampled             */
/* (item_local[nbr] >= 0; int32 [n_items], -1 = not sampled) emits (position  */
/* of the user in users[], item_local[nbr], eid): the reference's order.      */
/* Two calls over ONE workspace (size query with workspace == NULL):          */
/*   out_edges == NULL: count and exclusive scan; *count (DEVICE int64) =     */
/*     the number of edges, per-user offsets stay in the workspace;           */
/*   out_edges != NULL: fill out_edges[2, capacity] int64 (row 0 local user,  */
/*     row 1 local item) and out_eid[capacity] int64 from those offsets;      */
/*     capacity = the count the caller read (entries past it are dropped).    */
/* n_users_listed == 0 returns BBGR_OK without a launch (*count untouched).   */
typedef struct {
  int64_t n_users_listed;
  const int64_t *users;
  int64_t n_users;            /* rows of the CSR (bounds check) */
  const int32_t *item_local;
  const int32_t *indptr;
  const int32_t *nbr;
  const int32_t *eid;
  const float *ts;
  int64_t ts_stride;
  int32_t view;
  float split;
  int64_t *count;
  int64_t *out_edges;
  int64_t *out_eid;
  int64_t capacity;
} bbgr_slas_induce_args;
int bbgr_slas_induce(const bbgr_slas_induce_args *args, void *workspace,
                     size_t *workspace_bytes, bbgr_stream_t stream);

/* ------------------------------------------------------------------------- */
/* Review columns -> the credibility graph's tensors (main.py:153-196,        */
/* :247-373, :423-570): Ru and label, six behavioural features per user, the  */
/* item features and the edge attributes. Appended; the ABI stays 12.         */
/*                                                                            */
/* A record is one review that has a user, an item and a rating. The columns  */
/* are device arrays of n entries in file order. Ids must lie in [0, n_users) */
/* and [0, n_items): the caller checks them (bbgr.features does, before any   */
/* launch). Ratings are finite. Every sum is taken in double in a fixed order */
/* without float atomics (two calls: the same bits); results are rounded to   */
/* float once, at the store.                                                  */
/* ------------------------------------------------------------------------- */
typedef struct {
  int64_t n;                       /* records, < 2^31 - 1 */
  int32_t n_users;                 /* < 2^31 - 1 */
  int32_t n_items;
  const int32_t *user;
  const int32_t *item;
  const float *rating;
  const int32_t *helpful_vote;
  const uint8_t *verified;         /* 0 / non-zero */
  const int64_t *timestamp;        /* milliseconds */
  const uint8_t *ts_valid;         /* nullable: every record has a timestamp */
  const int32_t *n_tokens;         /* L = tokens of title + " " + text */
  const int32_t *n_unique_tokens;  /* distinct tokens among them */
} bbgr_feat_columns;

/* stats (DEVICE int64 [4]) = {ts_min, ts_max, records with a timestamp, sum  */
/* of n_tokens}; with no timestamp at all ts_min = INT64_MAX and ts_max =     */
/* INT64_MIN. Integer atomics only.                                           */
int bbgr_feat_stats(const bbgr_feat_columns *c, int64_t *stats, bbgr_stream_t stream);

/* The (row, column) pairs of the bucket CSR: for a record with a timestamp   */
/* rows[e] = user, cols[e] = floor(timestamp / 86400000) - floor(ts_min /     */
/* 86400000) (floor division: negative timestamps round down); for one        */
/* without, rows[e] = n_users (a spare row) and cols[e] = 0. *n_cols (HOST)   */
/* receives the column count. A CSR build over n_users + 1 rows and *n_cols   */
/* columns then lists every user's buckets in ascending order. ts_min and     */
/* ts_max are the values bbgr_feat_stats found. BBGR_ERR_INVALID, naming      */
/* timestamp, before any launch when the bucket range does not fit int32.     */
int bbgr_feat_buckets(const bbgr_feat_columns *c, int64_t ts_min, int64_t ts_max,
                      int32_t *rows, int32_t *cols, int32_t *n_cols, bbgr_stream_t stream);

/* Per item, over the reference-order item rows (i_indptr [n_items + 1],      */
/* i_eid [n]: record ids, ascending within a row):                            */
/*   item_x [n_items, 2] = {float(double mean of the raw rating), count}      */
/*   item_rbar [n_items] = the double mean of ri = clamp(round_half_even(     */
/*                         rating), 1, 5): what the users' deviation is from  */
/* An item with no record gets mean 0 and count 0. Size query with            */
/* workspace == NULL.                                                         */
int bbgr_feat_items(const bbgr_feat_columns *c, const int32_t *i_indptr, const int32_t *i_eid,
                    float *item_x, double *item_rbar, void *workspace,
                    size_t *workspace_bytes, bbgr_stream_t stream);

/* Per user, over the reference-order user rows and the bucket CSR's rows:    */
/*   total_reviews = n, helpful_reviews = #(helpful_vote > 5)                 */
/*   Ru = helpful / n; user_y = 1 if Ru >= 0.7, 0 if Ru <= 0.3, else -1       */
/*   user_x [n_users, 7] (USER_FEATURE_KEYS order) = Ru, the natural-log      */
/*     entropy of the histogram of ri (bins 1..5 in order), #(ri in {1, 5}) / */
/*     n, mean |ri - item_rbar[item]|, (records with a timestamp) - (distinct */
/*     buckets), (sum over L > 0 of unique / L) / n, mean |L -                */
/*     global_avg_len|                                                        */
/* A user with no record gets a NaN row, label -1 and zero counts. A row of   */
/* at most 512 records is summed by one lane in file order, a longer one by   */
/* one workgroup in a fixed shape. Size query with workspace == NULL; the     */
/* workspace holds 16 bytes per record (what the pass reads of a record,      */
/* packed by a streaming launch so that the gather by record id touches one   */
/* memory line per record, not five).                                         */
typedef struct {
  const int32_t *u_indptr;    /* [n_users + 1] */
  const int32_t *u_eid;       /* [n] */
  const int32_t *b_indptr;    /* [n_users + 2] (row n_users: no timestamp) */
  const int32_t *b_bucket;    /* [n] sorted within a row */
  const double *item_rbar;    /* [n_items] (bbgr_feat_items) */
  double global_avg_len;      /* sum of n_tokens / max(n, 1) */
  float *user_x;              /* [n_users, 7] */
  int64_t *user_y;            /* [n_users] */
  int32_t *total_reviews;     /* [n_users] */
  int32_t *helpful_reviews;   /* [n_users] */
} bbgr_feat_user_args;
int bbgr_feat_users(const bbgr_feat_columns *c, const bbgr_feat_user_args *args,
                    void *workspace, size_t *workspace_bytes, bbgr_stream_t stream);

/* edge_attr [n, 5] (EDGE_ATTR_KEYS order), in double, rounded at the store:  */
/*   verified, 1 - |rating - item_x[item, 0]| / 4, rating, (timestamp -       */
/*   ts_min) / (ts_max - ts_min) (NaN without a timestamp or when ts_max ==   */
/*   ts_min), helpful_vote. One streaming pass; edge_attr 16-byte aligned.    */
int bbgr_feat_edges(const bbgr_feat_columns *c, const float *item_x, int64_t ts_min,
                    int64_t ts_max, float *edge_attr, bbgr_stream_t stream);

/* ------------------------------------------------------------------------- */
/* The md5 train / val / test split of review records (build_graph_from_jsonl, */
/* lighgcn_cu_pop.py:227-303). Appended; the ABI stays 12. Integer work only:  */
/* two calls give the same bits.                                              */
/* ------------------------------------------------------------------------- */
/* hash32[e] = the first 32 bits of md5 over the bytes user_id[user[e]] + "|"  */
/* + item_id[item[e]]: digest bytes 0..3 read big-endian, Python's             */
/* int(hexdigest[:8], 16). An id table is a byte pool (UTF-8) and offsets      */
/* [n_ids + 1] into it, offsets[0] = 0, non-decreasing, the last at most the   */
/* pool's size; ids of any length (a loop over 64-byte blocks, standard md5    */
/* padding with the 64-bit bit length). keep (nullable, [n]): a record with    */
/* keep[e] == 0 is skipped and hash32[e] left as it was; so is a record whose  */
/* id lies outside its table (the caller checks ids: bbgr.split does, before   */
/* any launch). One launch, no workspace, no synchronisation.                  */
int bbgr_md5_pair_hash(int64_t n, const int32_t *user, const int32_t *item,
                       const uint8_t *user_data, const int64_t *user_offsets, int32_t n_users,
                       const uint8_t *item_data, const int64_t *item_offsets, int32_t n_items,
                       const uint8_t *keep, uint32_t *hash32, bbgr_stream_t stream);

/* The split. A record is positive when positive[e] != 0 or, with positive     */
/* NULL, when rating[e] >= pos_threshold (float32, exact; a NaN is not), and   */
/* its ids lie inside [0, n_users) / [0, n_items). A positive record goes to   */
/* train if hash32[e] < thr_train, to val if hash32[e] < thr_val, else to      */
/* test (integer compares; thr_train <= thr_val <= 2^32).                      */
/*   user_map [n_users], item_map [n_items]: the new id of an old id, numbered */
/*     by first appearance among the positive records in file order; -1 for    */
/*     an id with no positive record                                           */
/*   user_src [U'], item_src [I']: the inverse lists, src[new] = old (room for */
/*     n_users / n_items entries; only the first U' / I' are written)          */
/*   edges [2, ld_edges] (ld_edges >= n): columns [0, E_train) train, then     */
/*     E_val of val, then E_test of test, each in file order; row 0 the new    */
/*     user ids, row 1 the new item ids; repeated pairs stay repeated; the     */
/*     columns from E_train + E_val + E_test on are not written                */
/*   counts (DEVICE int64 [5]) = {E_train, E_val, E_test, U', I'}              */
/* Five launches and two memsets on `stream`; size query with workspace ==      */
/* NULL (one byte per record and 20 bytes per tile of 2048 records).           */
typedef struct {
  int64_t n;                  /* records, < 2^31 - 1 */
  int32_t n_users;            /* < 2^31 - 1 */
  int32_t n_items;
  const int32_t *user;        /* [n] */
  const int32_t *item;        /* [n] */
  const uint8_t *positive;    /* [n], nullable: then rating and pos_threshold */
  const float *rating;        /* [n], read when positive == NULL */
  float pos_threshold;
  const uint32_t *hash32;     /* [n] */
  uint64_t thr_train;
  uint64_t thr_val;
  int32_t *user_map;
  int32_t *item_map;
  int32_t *user_src;
  int32_t *item_src;
  int32_t *edges;
  int64_t ld_edges;
  int64_t *counts;
} bbgr_split_args;
int bbgr_split_edges(const bbgr_split_args *args, void *workspace, size_t *workspace_bytes,
                     bbgr_stream_t stream);

/* ------------------------------------------------------------------------- */
/* Token and distinct-token counts of review text (main.py tokenize():         */
/* re.findall(r"[a-z]+(?:'[a-z]+)?", s.lower()), then len(toks) and            */
/* len(set(toks))) over the UTF-8 bytes of the records. Appended; the ABI      */
/* stays 12. Integer work only: two calls give the same bits.                  */
/* ------------------------------------------------------------------------- */
/* The rule over bytes: a letter is an ASCII A-Za-z (compared as lower case)   */
/* or the byte C4 directly before B0 (U+0130: the letter i; B0 is a            */
/* separator); 0x27 is the apostrophe; every other byte and a record's edge    */
/* are separators. A maximal letter run is attached when exactly one           */
/* apostrophe lies between it and the run before. A run begins a token unless  */
/* it is attached and the run before it began one; then it is that token's     */
/* apostrophe part. U+212A (E2 84 AA, lower() "k") is not handled on the       */
/* device: bbgr_text_count sets recheck for every record that holds it.        */
/* Record r is data[offsets[r], offsets[r + 1]); offsets are clamped into      */
/* [first, last), and no byte outside that range is read as part of a token.   */
typedef struct {
  int64_t n;                 /* records, < 2^31 - 1 */
  const uint8_t *data;       /* DEVICE: records back to back */
  const int64_t *offsets;    /* DEVICE [n + 1], non-decreasing */
  int64_t first, last;       /* HOST copies of offsets[0], offsets[n]; last - first < 2^31 - 1 */
  uint64_t hash_mask;        /* 0: all 64 bits. Tests narrow it to force collisions */
  int32_t *n_tokens;         /* [n] */
  int32_t *n_unique_tokens;  /* [n] */
  uint8_t *recheck;          /* [n] 1: the device does not vouch for this record */
  int64_t *totals;           /* DEVICE int64 [2]: tokens, rechecks */
} bbgr_text_args;
/* n_tokens[r], recheck[r] (1 for a record that holds U+212A, else 0),         */
/* totals[0] = the sum of n_tokens, totals[1] = 0. One wave per record walks   */
/* it in steps of 64 bytes, a byte a lane (coalesced). One memset and one      */
/* launch on `stream`; no workspace.                                           */
int bbgr_text_count(const bbgr_text_args *args, bbgr_stream_t stream);
/* n_unique_tokens[r], after bbgr_text_count on the same args (it reads        */
/* n_tokens and adds to recheck). total_tokens: the host's copy of totals[0];  */
/* it sizes the workspace (32 bytes per token, 4 per record, the sort's own)   */
/* and is at most (last - first + n) / 2: a record of len bytes holds at most  */
/* (len + 1) / 2 tokens, and a record's edge separates without a byte.         */
/* Token offsets by a scan of n_tokens; per token its start and record; a      */
/* 64-bit hash of its normalised bytes (FNV-1a and a finaliser, and-ed with    */
/* hash_mask); a stable segmented radix sort by hash inside each record; then  */
/* per sorted token: a new distinct token where the hash differs from the left */
/* neighbour's, and with equal hashes a comparison of the two tokens'          */
/* normalised bytes and lengths, whose failure sets recheck[r]. An unflagged   */
/* record's count is therefore exact. totals[1] = the number of flagged        */
/* records. Size query with workspace == NULL.                                 */
int bbgr_text_unique(const bbgr_text_args *args, int64_t total_tokens, void *workspace,
                     size_t *workspace_bytes, bbgr_stream_t stream);
/* For measurement (tools/text_bench.py): the launch groups of                 */
/* bbgr_text_unique picked by `stages`, on a workspace the groups before them  */
/* have filled: EMIT the scan, the tokens' starts and hashes; SORT; VERIFY the */
/* counts, the comparison and totals[1]. stages = 7 is bbgr_text_unique. A     */
/* group run on a workspace its predecessors have not filled gives meaningless */
/* counts but stays inside its buffers: offsets, records and token indices     */
/* read from the workspace are clamped or checked before use.                  */
#define BBGR_TEXT_STAGE_EMIT 1
#define BBGR_TEXT_STAGE_SORT 2
#define BBGR_TEXT_STAGE_VERIFY 4
#define BBGR_TEXT_STAGE_ALL 7
int bbgr_text_unique_stages(const bbgr_text_args *args, int64_t total_tokens, int32_t stages,
                            void *workspace, size_t *workspace_bytes, bbgr_stream_t stream);

/* ------------------------------------------------------------------------- */
/* The second feature pipeline (main_v2_.py:291-524): pooled lexical           */
/* diversity, the entropy of temporal gaps (ETG), the share of low ratings     */
/* (RNR), and the v2 forms of four behavioural columns. Appended; the ABI      */
/* stays 12. Sums in double in a fixed order, no float atomics: two calls give */
/* the same bits.                                                              */
/* ------------------------------------------------------------------------- */
/* Distinct normalised tokens over ALL records of a group, after               */
/* bbgr_text_count on the same args (token rule, hash and hash_mask as above). */
/* group [n]: the group of each record (here the user id); a record whose      */
/* group lies outside [0, n_groups) is skipped (the caller checks them:        */
/* bbgr.text does, before any launch).                                         */
/*   group_tokens [n_groups] = the sum of n_tokens over the group's records    */
/*   group_unique [n_groups] = its distinct tokens                             */
/*   group_recheck [n_groups] = 1: the device does not vouch for this group:   */
/*     it owns a record with recheck set, or two of its tokens with equal      */
/*     hashes differ in their bytes                                            */
/*   totals[1] = the number of flagged groups                                  */
/* A group without a record gets 0 / 0 / 0. The token stream is                */
/* bbgr_text_unique's EMIT stage (this call runs it, in the first part of the  */
/* workspace); then a stable radix sort of all tokens by hash, one by group    */
/* over the bits n_groups needs, and per sorted token: a new distinct token    */
/* where the group or the hash differs from the left neighbour's, and with     */
/* both equal a comparison of the two tokens' normalised bytes and lengths. An */
/* unflagged group's count is therefore exact. total_tokens as for             */
/* bbgr_text_unique; one call takes last - first < 2^31 - 1 bytes. Equal       */
/* tokens only have to meet inside a group, so longer text is counted in       */
/* several calls, each on whole groups packed back to back by bbgr_text_gather */
/* with group ids local to the call: every output depends on the multiset of a */
/* group's tokens alone, not on the order of its records, and so equals the    */
/* one-call result bit for bit (bbgr.text.pooled_token_counts, chunk_bytes).   */
/* The workspace holds 40 bytes per token, 4 per record and the sorts' own.    */
/* Size query with workspace == NULL; stream-ordered, no synchronisation.      */
int bbgr_text_unique_pooled(const bbgr_text_args *args, int64_t total_tokens,
                            const int32_t *group, int32_t n_groups, int64_t *group_tokens,
                            int32_t *group_unique, uint8_t *group_recheck, void *workspace,
                            size_t *workspace_bytes, bbgr_stream_t stream);
/* For measurement (tools/text_bench.py): its launch groups picked by `stages` */
/* (BBGR_TEXT_STAGE_*): EMIT the token stream; SORT the two sorts and the      */
/* group keys between them; VERIFY the memsets, the comparison, the per-record */
/* pass and totals[1]. Out-of-range values read from a workspace no earlier    */
/* group has filled are skipped, as in bbgr_text_unique_stages.                */
int bbgr_text_unique_pooled_stages(const bbgr_text_args *args, int64_t total_tokens,
                                   const int32_t *group, int32_t n_groups,
                                   int64_t *group_tokens, int32_t *group_unique,
                                   uint8_t *group_recheck, int32_t stages, void *workspace,
                                   size_t *workspace_bytes, bbgr_stream_t stream);

/* lenlog_sum (DEVICE double [1]) = the sum of log1p(n_tokens) over the        */
/* records: 256 partial sums over a fixed grid, then one workgroup adds them.  */
/* global_avg_lenlog is this / max(n, 1). Size query with workspace == NULL.   */
int bbgr_feat_lenlog(const bbgr_feat_columns *c, double *lenlog_sum, void *workspace,
                     size_t *workspace_bytes, bbgr_stream_t stream);

/* item_mean [n_items] = the double mean of the raw rating over the            */
/* reference-order item rows (bbgr_feat_items rounds the same sum to float);   */
/* 0 for an item with no record. Size query with workspace == NULL.            */
int bbgr_feat_item_means(const bbgr_feat_columns *c, const int32_t *i_indptr,
                         const int32_t *i_eid, double *item_mean, void *workspace,
                         size_t *workspace_bytes, bbgr_stream_t stream);

/* etg [n_users] (double): per record with a timestamp days = (ts >= 10^12 ?   */
/* double(ts) / 1000.0 : double(ts)) / 86400.0 (IEEE double divisions); per    */
/* user over the reference-order user rows the days sorted (a segmented radix  */
/* sort; +inf for a record without a timestamp), bin = min(floor(days[j + 1] - */
/* days[j]), 365), and the natural-log entropy of the bins' histogram over the */
/* non-empty bins in ascending order, p = count / gaps; 0 with fewer than 3    */
/* timestamps. A row of at most 64 records is one lane's (it counts by value), */
/* a longer one a workgroup's with the 366 counters in LDS. The workspace      */
/* holds 16 bytes per record and the sort's own. Size query with workspace ==  */
/* NULL.                                                                       */
int bbgr_feat_gaps(const bbgr_feat_columns *c, const int32_t *u_indptr, const int32_t *u_eid,
                   double *etg, void *workspace, size_t *workspace_bytes, bbgr_stream_t stream);

/* bbgr_feat_users in main_v2_.py's definitions. total_reviews, helpful,       */
/* Ru, user_y and user_x columns 0, 1, 2 as there;                             */
/*   column 3 = mean |rating - item_mean[item]| (raw ratings)                  */
/*   column 4 = ((records with a timestamp) - (distinct buckets)) / n          */
/*   column 5 = group_unique / group_tokens, 0 when the user has no token      */
/*   column 6 = mean |log1p(L) - global_avg_lenlog|                            */
/*   user_extra [n_users, 2] = {RNR = #(ri <= 2) / n, ETG = etg[u]}            */
/* A user with no record gets a NaN row in both tables, label -1 and zero      */
/* counts. Row split, sums and workspace as for bbgr_feat_users.               */
typedef struct {
  const int32_t *u_indptr;      /* [n_users + 1] */
  const int32_t *u_eid;         /* [n] */
  const int32_t *b_indptr;      /* [n_users + 2] (row n_users: no timestamp) */
  const int32_t *b_bucket;      /* [n] sorted within a row */
  const double *item_mean;      /* [n_items] (bbgr_feat_item_means) */
  double global_avg_lenlog;     /* bbgr_feat_lenlog's sum / max(n, 1) */
  const int64_t *group_tokens;  /* [n_users] (bbgr_text_unique_pooled by user) */
  const int32_t *group_unique;  /* [n_users] */
  const double *etg;            /* [n_users] (bbgr_feat_gaps) */
  float *user_x;                /* [n_users, 7] */
  int64_t *user_y;              /* [n_users] */
  int32_t *total_reviews;       /* [n_users] */
  int32_t *helpful_reviews;     /* [n_users] */
  float *user_extra;            /* [n_users, 2] */
} bbgr_feat_user_v2_args;
int bbgr_feat_users_v2(const bbgr_feat_columns *c, const bbgr_feat_user_v2_args *args,
                       void *workspace, size_t *workspace_bytes, bbgr_stream_t stream);

/* ------------------------------------------------------------------------- */
/* The review dump (one JSON object per line) -> per-record columns, id bytes  */
/* and text bytes (features.review_columns_from_jsonl over bytes), and the     */
/* numbering of id strings by first appearance. Appended; the ABI stays 12.    */
/* Integer and exact-double work only: two calls give the same bits.           */
/* ------------------------------------------------------------------------- */
/* The rule over bytes. '\n' and '\r' both end a line; a last line without a   */
/* terminator counts; a line of only spaces and tabs is blank. Per line: the   */
/* string mask from the quotes and the parity of the backslash runs before     */
/* them, the bracket depth outside strings; a ':' at depth 1 outside strings   */
/* ends a top-level key, the string before it; the last occurrence of a key    */
/* wins; deeper keys are ignored. The keys read: user_id, item_key, rating,    */
/* helpful_vote, verified_purchase, timestamp, title, text. Vouched value      */
/* forms: a string of well-formed UTF-8 (Python's strict decoder) without a    */
/* raw byte below 0x20 and with the escapes \" \\ \/ \b \f \n \r \t \uXXXX (a  */
/* high + low \u surrogate pair is one 4-byte code point, a lone surrogate its */
/* 3 surrogatepass bytes); for helpful_vote and timestamp -?(0|[1-9][0-9]*) of */
/* at most 18 digits (helpful_vote inside int32), null or missing = 0 (and     */
/* ts_valid 0); for rating -?(0|[1-9][0-9]*)(\.[0-9]+)? of at most 15 digits   */
/* and no negative zero, the value (double)digits / 10^k cast once to float,   */
/* null or missing skips the record; true / false / null for                   */
/* verified_purchase; a string or null for title and text; a string for the    */
/* ids, where null, missing or "" skips the record. Every value read ends at a */
/* blank, ',' or '}' inside the line. Every other form, a top-level key that holds a backslash, a     */
/* line that does not open with '{', a byte below 0x20 (but a tab outside      */
/* strings), a backslash outside strings, an unterminated string, unbalanced   */
/* brackets, a top-level close other than '}' and bytes after it flag the      */
/* line: status 3, for the caller to parse on the host. Not detected:          */
/* malformed JSON that no value read depends on, while strings and brackets    */
/* balance.                                                                    */
/* Line status: 0 blank, 1 skipped, 2 kept, 3 flagged, 4 kept with the host's  */
/* values (set by the caller between bbgr_jsonl_scan and bbgr_jsonl_offsets:   */
/* the per-line columns hold the values, sizes[l] = {user, item, text, 0}      */
/* bytes and spos[l] = their positions in `side`).                             */
typedef struct {
  int64_t n_bytes;           /* the chunk's bytes, < 2^31 - 1 */
  const uint8_t *data;       /* DEVICE [n_bytes] */
  int64_t n_lines;           /* HOST copy of bbgr_jsonl_count's totals[0] */
  int32_t *line_end;         /* DEVICE [n_lines]: the line's terminator (n_bytes without one) */
  const uint8_t *item_key;   /* DEVICE [item_key_len]: the item id's key */
  int32_t item_key_len;      /* 1 .. 255 */
  uint8_t *status;           /* [n_lines] */
  float *rating;             /* [n_lines] per-line values of kept lines, 0 for others */
  int32_t *helpful_vote;     /* [n_lines] */
  uint8_t *verified;         /* [n_lines] */
  int64_t *timestamp;        /* [n_lines] */
  uint8_t *ts_valid;         /* [n_lines] */
  int32_t *sizes;            /* [n_lines, 4] unescaped bytes of user id, item id, title, text */
  int32_t *spos;             /* [n_lines, 4] their opening quotes in data, -1: null or missing */
  int64_t *totals;           /* DEVICE int64 [4] */
  int64_t *offs;             /* DEVICE int64 [4, n_lines + 1] (bbgr_jsonl_offsets) */
  const uint8_t *side;       /* DEVICE [side_bytes]: the bytes of status-4 lines (nullable) */
  int64_t side_bytes;
  int64_t n_records;         /* HOST copies of offs[0 .. 3][n_lines] */
  int64_t user_bytes, item_bytes, text_bytes;
  float *out_rating;         /* [n_records] the compact columns, file order */
  int32_t *out_helpful;
  uint8_t *out_verified;
  int64_t *out_timestamp;
  uint8_t *out_ts_valid;
  uint8_t *user_data;        /* [user_bytes] the records' user ids back to back */
  int64_t *user_off;         /* [n_records] where record r's begins (the caller appends the total) */
  uint8_t *item_data;        /* [item_bytes] */
  int64_t *item_off;
  uint8_t *text_data;        /* [text_bytes] title + " " + text per record */
  int64_t *text_off;
} bbgr_jsonl_args;
/* totals[0] = the number of lines of data[0, n_bytes); totals[1 .. 3] = 0.    */
/* One wave per 4096 bytes, a ballot of the terminators per 64-byte step. One  */
/* memset and one launch on `stream`; reads n_bytes, data, totals.             */
int bbgr_jsonl_count(const bbgr_jsonl_args *args, bbgr_stream_t stream);
/* line_end[0 .. n_lines): the tiles' counts, their exclusive scan, and each   */
/* terminator written at its rank (a rank outside [0, n_lines) is dropped).    */
/* The workspace holds 8 bytes per 4096 of data and the scan's own. Size query */
/* with workspace == NULL.                                                     */
int bbgr_jsonl_lines(const bbgr_jsonl_args *args, void *workspace, size_t *workspace_bytes,
                     bbgr_stream_t stream);
/* status, the per-line values, sizes and spos of every line, one wave per     */
/* line in 64-byte steps; totals = {blank, skipped, kept, flagged} lines.      */
/* line_end is clamped into [0, n_bytes]. One memset and one launch.           */
int bbgr_jsonl_scan(const bbgr_jsonl_args *args, bbgr_stream_t stream);
/* offs[w][l] = the exclusive sum over the lines before l of: w = 0 kept lines */
/* (status 2 or 4), w = 1 / 2 their user / item id bytes, w = 3 their text     */
/* bytes (title + 1 + text; for status 4 sizes[l][2]); offs[w][n_lines] the    */
/* totals, which the caller reads to size the outputs. Four scans. Size query  */
/* with workspace == NULL.                                                     */
int bbgr_jsonl_offsets(const bbgr_jsonl_args *args, void *workspace, size_t *workspace_bytes,
                       bbgr_stream_t stream);
/* The compact outputs of the kept lines: record offs[0][l] of line l gets the */
/* line's values, its offsets, and its unescaped (status 2) or copied (status  */
/* 4, from side) id and text bytes. Offsets read from offs are clamped into    */
/* the outputs, positions in spos checked against the line and side_bytes. One */
/* launch.                                                                     */
int bbgr_jsonl_write(const bbgr_jsonl_args *args, bbgr_stream_t stream);

/* The n strings data[offsets[r], offsets[r + 1]) (offsets clamped into        */
/* [0, data_bytes]) numbered by first appearance: ids[r] (int32 [n]) the id of */
/* record r's string, first_rec[k] (int32 [n], the first totals[0] entries     */
/* written) the record where id k first appears, totals (DEVICE int64 [2]) =   */
/* {distinct strings, collisions}. A 64-bit hash per string (FNV-1a and a      */
/* finaliser, and-ed with hash_mask; 0: all 64 bits), a stable radix sort of   */
/* (hash, record), per sorted slot a comparison of bytes and length with the   */
/* left neighbour's where the hashes are equal (an unequal pair adds to        */
/* collisions: with collisions != 0 the numbering is not vouched for and the   */
/* caller numbers on the host), run heads, a scan of the heads in record       */
/* order. The workspace holds 44 bytes per record and the sort's own. Size     */
/* query with workspace == NULL; stream-ordered.                               */
int bbgr_ids_number(int64_t n, const uint8_t *data, const int64_t *offsets, int64_t data_bytes,
                    uint64_t hash_mask, int32_t *ids, int32_t *first_rec, int64_t *totals,
                    void *workspace, size_t *workspace_bytes, bbgr_stream_t stream);
/* The id table of bbgr_ids_number's first_rec. With tab_data == NULL:         */
/* tab_offsets (DEVICE int64 [n_ids + 1]) = the exclusive sum of the strings'  */
/* lengths, tab_offsets[n_ids] the table's bytes. With tab_data [tab_bytes]:   */
/* string k copied to tab_offsets[k] (clamped; a first_rec outside [0, n) is   */
/* skipped). Size query with workspace == NULL.                                */
int bbgr_ids_table(int64_t n_ids, const int32_t *first_rec, int64_t n, const uint8_t *data,
                   const int64_t *offsets, int64_t data_bytes, int64_t *tab_offsets,
                   uint8_t *tab_data, int64_t tab_bytes, void *workspace, size_t *workspace_bytes,
                   bbgr_stream_t stream);

/* ------------------------------------------------------------------------- */
/* Pack listed records of a text of any size back to back (bbgr.text regroups  */
/* the records by user with it, so that a chunk of bbgr_text_unique_pooled     */
/* holds whole users). Appended; the ABI stays 12.                             */
/* ------------------------------------------------------------------------- */
typedef struct {
  int64_t n_list;          /* listed records, < 2^31 - 1 */
  const int32_t *records;  /* DEVICE [n_list]: record ids; one outside [0, n) has length 0 */
  int64_t n;               /* records of the source text */
  const uint8_t *data;     /* DEVICE: source bytes, ANY size (64-bit addressing) */
  const int64_t *offsets;  /* DEVICE [n + 1], clamped into [first, last] as bbgr_text_args does */
  int64_t first, last;     /* HOST; last - first is NOT limited here */
  int64_t *out_offsets;    /* DEVICE [n_list + 1]: 0, then the running sum of the lengths */
  uint8_t *out_data;       /* DEVICE [capacity], 16-byte aligned; NULL: offsets and total only */
  int64_t capacity;
  int64_t *total;          /* DEVICE int64 [1] = out_offsets[n_list] */
} bbgr_text_gather_args;
/* Listed record j is copied to out_data[out_offsets[j], out_offsets[j + 1]);  */
/* ids may repeat and come in any order, records may be empty. No byte at or   */
/* beyond min(total, capacity) is written and no address outside               */
/* data[first, last) is loaded. One lane per listed record takes its clamped   */
/* length, hipcub scans the lengths, and the copy is output-centric: a wave    */
/* owns 1 KiB of the packed bytes at a time, finds the records that touch it   */
/* in out_offsets, and each lane assembles one aligned 16-byte word (from one  */
/* unaligned 16-byte load where the word lies in one record). Plain copies:    */
/* two calls give the same bytes. The workspace holds 8 bytes per listed       */
/* record and the scan's own. n_list = 0 returns at once and writes nothing.   */
/* Size query with workspace == NULL; stream-ordered, no synchronisation.      */
int bbgr_text_gather(const bbgr_text_gather_args *args, void *workspace,
                     size_t *workspace_bytes, bbgr_stream_t stream);
/* For measurement (tools/text_bench.py): the same call with the source fetch  */
/* picked by `fetch`. UNALIGNED is bbgr_text_gather: one unaligned 16-byte     */
/* load a word. ALIGNED_PAIR: the one or two 16-byte aligned words that hold   */
/* the 16 bytes and a byte shift, taken where both words lie inside            */
/* data[first, last), else the bytes one by one. The same bytes come out.      */
#define BBGR_TEXT_FETCH_UNALIGNED 0
#define BBGR_TEXT_FETCH_ALIGNED_PAIR 1
int bbgr_text_gather_fetch(const bbgr_text_gather_args *args, int32_t fetch, void *workspace,
                           size_t *workspace_bytes, bbgr_stream_t stream);

/* ------------------------------------------------------------------------- */
/* Blueprint names (SURVEY §8(b)'s ABI sketch), thin forms of the above.      */
/* ------------------------------------------------------------------------- */
/* Y = diag(row_scale) A diag(col_scale) X (either scale NULL = ones), one    */
/* fused launch; acc (nullable, leading dimension ldy): acc += acc_scale * Y  */
/* (the layer-mean accumulation). For plans without split rows               */
/* (A->n_split == 0); otherwise use bbgr_spmm with a partial workspace.       */
int bbgr_spmm_f32(const bbgr_csr *A, const float *X, int64_t ldx, float *Y, int64_t ldy,
                  int32_t d, const float *row_scale, const float *col_scale, float *acc,
                  float acc_scale, bbgr_stream_t stream);
/* = bbgr_bpr (loss parts and gradients in one launch). */
int bbgr_bpr_fwd_bwd(const bbgr_bpr_args *args, bbgr_stream_t stream);
/* = bbgr_adam with the sketch's float betas: 1 - beta then carries the float */
/* beta's rounding (up to 2^-25 absolute; exact for betas a float holds). Use */
/* bbgr_adam for torch's constants.                                           */
int bbgr_adam_f32(int64_t n, float *param, const float *grad, float *exp_avg,
                  float *exp_avg_sq, float lr, float beta1, float beta2, float eps,
                  float weight_decay, float grad_scale, float bias_correction1,
                  float bias_correction2_sqrt, bbgr_stream_t stream);
/* = bbgr_sample (pop-mix negatives + uniform positives). */
int bbgr_negsample(int64_t batch, const int64_t *users, const int32_t *indptr,
                   const int32_t *indices, int32_t n_items, const double *cdf,
                   float mix_pop, int32_t max_tries, uint64_t seed, uint64_t counter,
                   int64_t *pos, int64_t *neg, int32_t *fail_count, bbgr_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* BBGR_H */
