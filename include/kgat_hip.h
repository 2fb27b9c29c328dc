/* kgat_hip.h - C ABI of libkgat_hip.so: KGAT's attentive embedding-propagation path on
 * MI355X (gfx950).  This is the drop-in boundary: every entry point below
 * replaces one DGL 0.4.x kernel family that the reference reaches from models.py, and is
 * exactly what a binding for that call site would bind (ctypes stub: INTEGRATION.md).
 *
 * Conventions
 *  - Plain pointers and sizes only.  Every pointer is a DEVICE pointer (hipMalloc'd or
 *    torch-allocated) unless the parameter name ends in `_host`.  Buffers are borrowed for
 *    the duration of the call; the library allocates nothing persistent and frees nothing
 *    it did not allocate.  Scratch memory is passed in by the caller (`*_workspace_bytes`).
 *  - `stream` is a hipStream_t passed as void* (NULL = the null stream).  All work is
 *    enqueued asynchronously on it; no entry point synchronises the host.
 *  - Return value: 0 on success, negative KGAT_E_* on failure; the message is available
 *    from kgat_last_error() (thread-local).  Nothing throws or aborts across the ABI.
 *  - Indices are int32 (E, N < 2^31); byte offsets are formed in 64 bit.  Feature matrices
 *    are row-major contiguous fp32.  Per-edge arrays are in EDGE-ID order (the order edges
 *    were added, reference dataset.py:116) unless the name says `_csr` (destination-major
 *    CSR position order) - outputs are always fully overwritten.
 *  - Edge direction (reference dataset.py:116, add_edges(t, h)): src = tail t, dst = head h.
 */
#ifndef KGAT_HIP_H_
#define KGAT_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KGAT_ABI_VERSION 16
/* 16: removed the five kgat_bi_interaction_{mul,mul_deferred,train,bwd_input,bwd_weight} entries (call the
 * kgat_aggregator_* entry with KGAT_FORM_BI), flag value 2 of the fused attention (a kernel on 32-group tiles) and the
 * groups-per-tile parameter of kgat_fold_tiles / kgat_att_pack_records. */

enum {
  KGAT_OK = 0,
  KGAT_E_BADARG = -1,      /* null pointer, negative size, inconsistent sizes */
  KGAT_E_UNSUPPORTED = -2, /* e.g. feature width the kernels do not cover */
  KGAT_E_WORKSPACE = -3,   /* workspace too small */
  KGAT_E_HIP = -4          /* a HIP runtime call or launch failed */
};

/* flags for kgat_spmm_umule_sum_f32 */
enum {
  KGAT_SPMM_MUL_SELF = 1, /* out[v,:] *= X[row0+v,:]  (the h * h_neighbor of models.py:66) */
  KGAT_SPMM_DEFER_FINISH = 2 /* the second launch is left to kgat_aggregator_deferred_f32 (see kgat_spmm_tile_edges) */
};

/* algorithm selectors (AUTO picks the tuned kernel; the others exist for A/B and tests) */
enum {
  KGAT_SPMM_ALGO_AUTO = 0,
  KGAT_SPMM_ALGO_MERGE = 1,  /* edge-balanced tiles over the destination-sorted edge array */
  KGAT_SPMM_ALGO_ROWS = 2,   /* one lane group per destination row (optionally degree ordered) */
  KGAT_SPMM_ALGO_GENERIC = 3, /* any feature width, one wavefront per row */
  KGAT_SPMM_ALGO_MERGE1 = 4   /* first form of the merge kernel (shuffle-fed), kept for A/B */
};
enum {
  KGAT_ATT_ALGO_AUTO = 0,
  KGAT_ATT_ALGO_MFMA = 1,   /* v_mfma_f32_16x16x4_f32; d == k in {16,32,64,128} */
  KGAT_ATT_ALGO_GENERIC = 2, /* VALU, any (d,k) with d*k*4 <= 64 KiB */
  KGAT_ATT_ALGO_MFMA_CHUNK = 3 /* the workgroup-chunk MFMA kernel (W_r in LDS) that AUTO takes at d = 128, beyond
                                * 4,096 relations and for tables of 4 GiB and more - selectable so that tests reach it
                                * on small inputs */
};

/* flags for kgat_att_score_fused_f32 and kgat_att_score_folded_f32 */
enum {
  KGAT_ATT_F32_PRODUCTS = 1 /* both products as v_mfma_f32_16x16x4_f32 (the round-1 form) instead of
                             * the default where a kernel has it (fused: d % 32 == 0; folded: d = 128):
                             * every fp32 operand cut by round-to-nearest into three bf16 pieces that
                             * sum to it exactly (|m| <= 2^-8 |x|, |l| <= 2^-16 |x|), the six piece
                             * products of weight >= 2^-16 accumulated in fp32 by
                             * v_mfma_f32_16x16x32_bf16; the three dropped products are together
                             * < 2^-23 of |a*b| (one fp32 ulp), of either sign; error against fp64
                             * measured no larger than the fp32 form's */
};

/* reduce of kgat_copy_reduce_f32 (dgl.function.sum / dgl.function.mean) */
enum {
  KGAT_REDUCE_SUM = 0,
  KGAT_REDUCE_MEAN = 1
};

/* mode of kgat_edge_norm_f32 (the commented-out --adj_type of reference kgat.py:19: "si" / "bi") */
enum {
  KGAT_NORM_SI = 0,  /* random-walk Laplacian D^-1 A: 1 / in-degree of the destination */
  KGAT_NORM_BI = 1   /* symmetric Laplacian D^-1/2 A D^-1/2: 1 / sqrt(out-degree of the source * in-degree of the destination) */
};

/* the aggregator of a KGAT layer (res_type of KGATConv, reference models.py:50-58; the KGAT paper's "Information
 * Aggregation": Bi-Interaction, GCN, GraphSage) - the `form` argument of the kgat_aggregator_* entries */
enum {
  KGAT_FORM_BI = 0,        /* LeakyReLU(W (h * h_N)), W = res_fc_2.weight (d_out x d_in) */
  KGAT_FORM_GCN = 1,       /* LeakyReLU(W (h + h_N)), W = res_fc.weight (d_out x d_in) */
  KGAT_FORM_GRAPHSAGE = 2  /* LeakyReLU(W [h | h_N]), W = res_fc.weight (d_out x 2 d_in): columns [0, d_in) act on h */
};

/* activation of kgat_sage_dense_f32 */
enum {
  KGAT_ACT_NONE = 0,
  KGAT_ACT_RELU = 1
};

typedef void* kgat_stream_t; /* hipStream_t */

int kgat_version(void);
const char* kgat_last_error(void);
/* sha256[:16] of the sources (csrc/ + this header + compiler flags) the library was built from,
 * as the build recipe passed it in; the loader refuses a library whose hash is not the hash of
 * the sources beside it (a stale build would otherwise be called with other argument lists). */
const char* kgat_build_hash(void);

/* ---------------------------------------------------------------- graph structure (G0)
 * Replaces DGL's COO -> in-CSR conversion that runs on the first kernel call on a graph
 * built by reference dataset.py:112-120.  Stable: within a destination row, edge ids
 * ascend.  indptr[N+1], col[E] (source ids), eid[E] (original edge id per CSR position),
 * row_of[E] (destination id per CSR position; may be NULL).
 * Ids outside [0,N) are a caller error (checked by the host wrapper, not on device). */
size_t kgat_csr_from_coo_workspace_bytes(int64_t n_nodes, int64_t n_edges);
int kgat_csr_from_coo(int64_t n_nodes, int64_t n_edges, const int32_t* src, const int32_t* dst,
                      int32_t* indptr, int32_t* col, int32_t* eid, int32_t* row_of,
                      void* workspace, size_t workspace_bytes, kgat_stream_t stream);

/* Replaces the R full-graph g.filter_edges(lambda e: e.data['type'] == i) sweeps of
 * reference models.py:149-150 by one stable grouping: perm[rel_ptr[r] .. rel_ptr[r+1]) are
 * the edge ids of relation r, ascending.  Types outside [0,R) are placed after rel_ptr[R]
 * (the reference loop never visits them). */
size_t kgat_group_by_relation_workspace_bytes(int64_t n_edges, int n_rel);
int kgat_group_by_relation(int64_t n_edges, int n_rel, const int32_t* etype, int32_t* rel_ptr,
                           int32_t* perm, void* workspace, size_t workspace_bytes,
                           kgat_stream_t stream);

/* Inverse of a permutation: inv[perm[i]] = i  (CSR position of each edge id). */
int kgat_invert_permutation(int64_t n, const int32_t* perm, int32_t* inv, kgat_stream_t stream);

/* Row schedule for the row-parallel kernels: a permutation of the CSR rows by descending
 * in-degree (stable), so that the row groups that share a wavefront carry similar work and
 * the heaviest rows start first.  order[N]. */
size_t kgat_row_order_workspace_bytes(int64_t n_rows);
int kgat_row_order_by_degree(int64_t n_rows, const int32_t* indptr, int32_t* order,
                             void* workspace, size_t workspace_bytes, kgat_stream_t stream);

/* ---------------------------------------------------------------- attention score (A1+A2)
 * Replaces the per-relation g.apply_edges(self._att_score, e_idxs) loop of reference
 * models.py:135-152 by one launch over relation-grouped edges:
 *   logits[e] = sum_j (ent[src e] W_R[r])_j * tanh((ent[dst e] W_R[r])_j + rel[r]_j), r = type(e)
 * ent (N,d), W_R (R,d,k), rel (R,k).  rel_ptr/perm come from kgat_group_by_relation;
 * src_g[i] = src[perm[i]], dst_g[i] = dst[perm[i]] (relation-grouped endpoint arrays, built
 * once per graph with kgat_gather_i32).  Edges whose type is outside [0,R) get logit 0 (DGL
 * zero-initialises the column on the first partial write).  logits[E] in edge-id order; if
 * logits_csr is non-NULL the same value is also written in CSR position order through
 * pos_g[i] = CSR position of edge perm[i] (= kgat_gather_i32(perm, csr_pos)). */
int kgat_att_score_f32(int64_t n_nodes, int64_t n_edges, int d, int k, int n_rel,
                       const int32_t* rel_ptr, const int32_t* perm, const int32_t* src_g,
                       const int32_t* dst_g, const float* ent, const float* W_R, const float* rel,
                       float* logits, float* logits_csr, const int32_t* pos_g, int algo,
                       kgat_stream_t stream);

/* Head groups for the split attention path.  Input: a relation-grouped edge list whose
 * relations are internally sorted by destination (group the CSR-ordered edge list by relation:
 * rel_ptr[R+1], dst_g[E]).  Consecutive positions with the same (relation, destination) form
 * one group: gid[E] = group of each position, gptr[R+1] = first group of each relation
 * (gptr[R] = number of groups over the scored relations), g_node[<= E] = destination (head)
 * of each group.  The attention kernels read gid in 16-byte pieces: allocate 16 entries of
 * slack after gid[E-1] holding valid group ids (e.g. 0). */
size_t kgat_head_groups_workspace_bytes(int64_t n_edges);
int kgat_head_groups(int64_t n_edges, int n_rel, const int32_t* rel_ptr, const int32_t* dst_g,
                     int32_t* gid, int32_t* gptr, int32_t* g_node, void* workspace,
                     size_t workspace_bytes, kgat_stream_t stream);

/* Same logits as kgat_att_score_f32, computed in two launches: tanh(ent[h] W_R[r] + rel[r]) once
 * per (head, relation) group into G_tab (n_groups x k floats, caller scratch), then per edge
 * the tail projection and its dot product with the group's row.  The head projection and all
 * tanh work are shared by the edges of a group (3.8 edges per group on the amazon-book-shaped
 * CKG).  Arithmetic per edge is unchanged.  Needs d == k in {16,32,64}
 * (kgat_att_score_split_supported).  logits (edge-id order) or logits_csr may be NULL. */
int kgat_att_score_split_supported(int64_t n_nodes, int d, int k, int n_rel);
int kgat_att_score_split_f32(int64_t n_nodes, int64_t n_edges, int d, int k, int n_rel,
                             const int32_t* rel_ptr, const int32_t* perm, const int32_t* src_g,
                             const int32_t* pos_g, const int32_t* gid, const int32_t* gptr,
                             const int32_t* g_node, int64_t n_groups, const float* ent,
                             const float* W_R, const float* rel, float* G_tab, float* logits,
                             float* logits_csr, kgat_stream_t stream);

/* Folded form of the same logits (reference models.py:135-144, restated).  The logit is bilinear
 * in the tail row: sum_j (ent[t] W_r)_j T_j = ent[t] . (W_r T) with T = tanh(ent[h] W_r + rel[r]),
 * so V[g] = W_r T (a d-vector) is computed once per (head, relation) group into V_tab
 * (n_groups x d floats, caller scratch) and an edge costs one d-length dot product.  Same
 * inputs and outputs as kgat_att_score_split_f32; the contraction order differs from the
 * reference's, so the results agree with the other forms to fp32 rounding (~1e-6 relative to
 * sum_j |t_j T_j|), not bit for bit.  Widths: d == k in {16,32,64,128} (MFMA), or d in {8,16,32}
 * with any k <= 32 (one thread per group; BASELINE configs[0] has d = k = 8).
 * flags: 0 or KGAT_ATT_F32_PRODUCTS. */
int kgat_att_score_folded_supported(int64_t n_nodes, int d, int k, int n_rel);
int kgat_att_score_folded_f32(int64_t n_nodes, int64_t n_edges, int d, int k, int n_rel,
                              const int32_t* rel_ptr, const int32_t* perm, const int32_t* src_g,
                              const int32_t* pos_g, const int32_t* gid, const int32_t* gptr,
                              const int32_t* g_node, int64_t n_groups, const float* ent,
                              const float* W_R, const float* rel, float* V_tab, float* logits,
                              float* logits_csr, int flags, kgat_stream_t stream);

/* Fused folded form: one launch, no V table.  Work tiles (graph-static, kgat_fold_tiles): at most
 * 16 consecutive head groups of one relation and at most `cap` grouped positions; a 16-group
 * block with more positions appears several times with consecutive position ranges.
 *   tiles    int32[4 * kgat_fold_tiles_max(...)]: (relation, first group, first position, end position)
 *   rel_tptr int32[R+1]: first tile of each relation; rel_tptr[R] = number of tiles
 * A wavefront computes a tile's V rows (as kgat_att_score_folded_f32), keeps them in LDS and
 * takes the dot products of the tile's positions itself.  Same logits as the folded form up to
 * the summation order of the d-length dot product (fp32 rounding).  cap: a positive multiple of
 * 64 (256 is the default of the host code).  Needs d == k in {16,32,64,128}; at d = k = 128 (one
 * 512-thread workgroup per CU holding W_r's three bf16 piece images, 96 KB, and a 16 x 128 V patch
 * per wave in LDS) only the bf16-piece products exist. */
int64_t kgat_fold_tiles_max(int64_t n_edges, int64_t n_groups, int n_rel, int cap);
size_t kgat_fold_tiles_workspace_bytes(int64_t n_groups, int n_rel);
int kgat_fold_tiles(int64_t n_edges, int n_rel, int64_t n_groups, const int32_t* rel_ptr, const int32_t* gid,
                    const int32_t* gptr, int cap, int32_t* tiles, int32_t* rel_tptr, void* workspace,
                    size_t workspace_bytes, kgat_stream_t stream);
/* Split of the tiles over the n_parts workgroups of the fused kernel (graph-static, like the
 * tiles): part b owns the contiguous tile range [part_tptr[b], part_tptr[b+1]), chosen on the
 * prefix sum of a per-tile cost
 *   cost_tile + cost_chunk * ceil(max(P - 64, 0) / 64) + (the tile opens its relation ? cost_relation : 0)
 * (P = positions of the tile) so that every workgroup gets the same cost, not the same tile
 * count.  The form follows what per-workgroup clock stamps showed on MI355X (least squares over
 * 3,072 workgroup samples, 1 % rms residual): a tile's MFMA phase is a constant (1,459 ticks of
 * workgroup time), its first 64 positions are free (their rows arrive during the MFMA phase),
 * every further chunk of 64 positions costs 267 ticks, and a relation change inside a
 * workgroup's range - W_r reload, two barriers, the prefetch pipeline of eight waves restarting -
 * costs 10,630 ticks, as much as seven tiles.  t_max = number of rows of `tiles`;
 * part_tptr[n_parts + 1]. */
size_t kgat_fold_tile_parts_workspace_bytes(int64_t t_max);
int kgat_fold_tile_parts(int64_t t_max, int n_rel, const int32_t* tiles, const int32_t* rel_tptr, int n_parts,
                         int cost_tile, int cost_chunk, int cost_relation, int32_t* part_tptr, void* workspace,
                         size_t workspace_bytes, kgat_stream_t stream);
int kgat_att_score_fused_supported(int64_t n_nodes, int d, int k, int n_rel);
/* What the fused kernel reads per grouped position, packed into one int32 (graph-static):
 *   rec_g[p] = src_g[p] | (((gid[p] - gptr[relation of p]) & 15) << 28)
 * i.e. the source (tail) node and the slot of the position's head group inside its 16-group block
 * (tiles are cut out of such blocks, whatever the cap).  Needs n_nodes <= 2^28.  Positions past
 * rel_ptr[R] (never scored) get their source node and slot 0. */
int kgat_att_pack_records(int64_t n_edges, int n_rel, const int32_t* rel_ptr, const int32_t* gptr,
                          const int32_t* gid, const int32_t* src_g, int32_t* rec_g, kgat_stream_t stream);
/* part_tptr / n_parts: the split above (one workgroup per part); NULL / 0: one workgroup per
 * compute unit, equal tile counts.  flags: 0 or KGAT_ATT_F32_PRODUCTS.
 * Outputs (any non-empty subset): logits_g[E] in grouped order (position p of the relation-grouped
 * list; coalesced stores - the form the propagation path takes: kgat_edge_softmax_f32 then reads
 * them through the CSR-position -> grouped-position map, see there), logits_csr[E] in CSR order
 * (needs pos_g), logits[E] in edge-id order (needs perm).  Never-scored positions get 0. */
int kgat_att_score_fused_f32(int64_t n_nodes, int64_t n_edges, int d, int k, int n_rel,
                             const int32_t* rel_ptr, const int32_t* perm, const int32_t* rec_g,
                             const int32_t* pos_g, const int32_t* gptr,
                             const int32_t* g_node, const int32_t* tiles, const int32_t* rel_tptr,
                             const int32_t* part_tptr, int n_parts,
                             const float* ent, const float* W_R, const float* rel, float* logits,
                             float* logits_csr, float* logits_g, int flags, kgat_stream_t stream);
/* Measurement aid: the same launch with every workgroup's start and end time written to part_clocks[2 b], [2 b + 1]
 * (100 MHz ticks of s_memrealtime; part b = workgroup b's tile range).  Same results; needs part_tptr.  (What it
 * showed, scripts/micro/att_rebalance_probe.py: the cost model of kgat_fold_tile_parts leaves the workgroups' end
 * times 8-9 % apart and the pattern repeats - correlation 0.98 run to run -, so ranges re-cut from measured times
 * take 7-9 % off the launch where the calibration and the use share their surroundings; calibrated on the
 * caller's first launches inside the benchmark step the gain was 1.5 %: not adopted.) */
int kgat_att_score_fused_timed_f32(int64_t n_nodes, int64_t n_edges, int d, int k, int n_rel,
                                   const int32_t* rel_ptr, const int32_t* perm, const int32_t* rec_g,
                                   const int32_t* pos_g, const int32_t* gptr,
                                   const int32_t* g_node, const int32_t* tiles, const int32_t* rel_tptr,
                                   const int32_t* part_tptr, int n_parts,
                                   const float* ent, const float* W_R, const float* rel, float* logits,
                                   float* logits_csr, float* logits_g, int flags, long long* part_clocks,
                                   kgat_stream_t stream);

/* ---------------------------------------------------------------- attention score, backward
 * Gradient of the logits above w.r.t. ent, W_R and rel: what autograd computes through the apply_edges loop of
 * reference models.py:135-154 when the caller drops the `with th.no_grad()` around compute_attention.  With
 *   T = tanh(ent[h] W_r + rel[r]),  V = W_r T  (the folded forward's per-group vectors),  g_p = grad of the logit of
 * grouped position p, the sums factorise over the (head, relation) groups G of kgat_head_groups:
 *   A_G = sum_{p in G} g_p ent[src_g[p]]    dP_G = (A_G W_r) * (1 - T_G^2)
 *   grad_ent[src_g[p]] += g_p V_G           grad_ent[h] += dP_G W_r^T
 *   grad_rel[r] += dP_G                     grad_W_R[r] += A_G^T (x) T_G + ent[h]^T (x) dP_G
 * Positions past n_scored = rel_ptr[R] (types outside [0,R): constant logit 0) take no part.  A self-loop gives its
 * node both terms, parallel edges count once each.  T and V are recomputed from ent (the forward saves nothing).
 * Inputs, all graph-static except the last four:
 *   src_g[n_scored], gid[n_scored], gptr[R+1], g_node[n_groups]   as for kgat_att_score_folded_f32
 *   gstart[n_groups+1]   first grouped position of each group; gstart[n_groups] = n_scored
 *   node_ptr[N+1], node_col / node_row / node_wsrc [n_scored + n_groups]   a node-major CSR (kgat_csr_from_coo) of the
 *       entries { node src_g[p], column gid[p], weight index p } for every scored position and
 *       { node g_node[G], column n_groups + G, weight index n_scored } for every group: node_row = node per entry
 *   ent (N,d), W_R (R,d,k), rel (R,k)
 *   grad_logits_g[n_scored + 1]: the logit gradients in grouped order (position p of kgat_group_by_relation) and one
 *       float of room after them, to which the call writes 1.0 (the weight of the per-group entries of the node CSR,
 *       read through node_wsrc) - a buffer of E + 1 floats gathered into serves; what follows element n_scored is not read
 * Outputs, fully written (rows and relations without a contribution are exact zeros; nothing is pre-zeroed by the
 * caller): grad_ent (N,d), grad_W_R (R,d,k), grad_rel (R,k).
 * Launches: kgat_spmm_umule_sum_f32 for A_G (rows = groups); one v_mfma_f32_16x16x4_f32 kernel over tiles of at most 16
 * consecutive groups of one relation that forms T, V, dP, dP W_r^T and the tile's grad W_r / grad rel terms - a
 * workgroup owns a contiguous tile range, accumulates across its tiles of one relation and flushes one partial per
 * relation change (at most n_workgroups + R partials); a fixed-order sum of those partials; kgat_spmm_umule_sum_f32
 * over the node-major CSR for grad_ent (columns index the [V ; dP W_r^T] table).  No float atomics, fixed summation
 * order: bitwise reproducible (on one device model: the workgroup count, and with it the order in which the weight-
 * gradient partials are summed, follows the sizes and the number of compute units).  Widths: d == k in {16,32,64,128}, 0 < R <= 4096, n_nodes * d * 4 < 4 GiB (the bound of
 * the forward's group forms); others return KGAT_E_UNSUPPORTED.  ent, W_R, grad_ent and the workspace 16-byte aligned.
 * Workspace: the three tables (3 n_groups d floats), the partials ((n_workgroups + R) (d k + k) floats) and the
 * aggregation's scratch. */
int kgat_att_score_bwd_supported(int64_t n_nodes, int d, int k, int n_rel);
size_t kgat_att_score_bwd_workspace_bytes(int64_t n_nodes, int64_t n_scored, int64_t n_groups, int d, int k, int n_rel);
int kgat_att_score_bwd_f32(int64_t n_nodes, int64_t n_scored, int64_t n_groups, int d, int k, int n_rel,
                           const int32_t* src_g, const int32_t* gid, const int32_t* gstart, const int32_t* gptr,
                           const int32_t* g_node, const int32_t* node_ptr, const int32_t* node_col,
                           const int32_t* node_row, const int32_t* node_wsrc, const float* ent, const float* W_R,
                           const float* rel, float* grad_logits_g, float* grad_ent, float* grad_W_R,
                           float* grad_rel, void* workspace, size_t workspace_bytes, kgat_stream_t stream);

/* ---------------------------------------------------------------- edge softmax (A3)
 * Replaces dgl.nn.pytorch.softmax.edge_softmax (call site reference models.py:153):
 *   a[e] = exp(s[e] - max_{e'->dst e} s[e']) / sum_{e'->dst e} exp(s[e'] - max)
 * over the incoming edges of each destination, all relations together, for the CSR
 * positions [e_begin, e_end) (the whole graph: 0, E; a destination-range shard: its
 * indptr range).  row_of = destination id per CSR position.
 * Input: logits in edge-id order (logits_in_csr_order = 0; read through eid) or in CSR
 * position order (1).  Outputs (either may be NULL, not both): out in edge-id order (written
 * through eid) and out_csr in CSR order.  eid = original edge id per CSR position.
 * One sweep over the positions (rows finished inside a wavefront's 512- or 1,024-position range
 * are normalised on the spot; the positions of the rows the range cuts are stored as
 * exp(s - partial max)) plus one short launch in which every wavefront combines, for the rows
 * its range cuts, the carry entries of the row's whole chain in a fixed order and rescales its
 * own positions of them (it reads the outputs, not the logits).  No atomics, fixed combination
 * order: bitwise reproducible, no bound on a row's length.  Full ranges move as 16-byte loads /
 * stores when row_of, eid, out_csr (and CSR-ordered logits) are 16-byte aligned and e_begin is a
 * multiple of 4; otherwise position by position, same results.  indptr[N+1] is the CSR row pointer (the extent of a cut row - which
 * wavefronts hold its carries - is read from it); every row that has a position in
 * [e_begin, e_end) must lie inside it completely (true for the whole graph and for a
 * destination-range shard).  Workspace: n_edges = e_end - e_begin. */
size_t kgat_edge_softmax_workspace_bytes(int64_t n_nodes, int64_t n_edges);
int kgat_edge_softmax_f32(int64_t n_nodes, int64_t e_begin, int64_t e_end, const int32_t* indptr,
                          const int32_t* row_of, const int32_t* eid, const float* logits,
                          int logits_in_csr_order, float* out, float* out_csr, void* workspace,
                          size_t workspace_bytes, kgat_stream_t stream);
/* The same operator as three streaming passes (integer-ordered atomic row max, row sum in 2^-40
 * fixed point with 64-bit atomic adds, normalise): an independent implementation kept for
 * cross-checks and A/B timing.  At most 2^24 positions per destination. */
size_t kgat_edge_softmax_3pass_workspace_bytes(int64_t n_nodes);
int kgat_edge_softmax_3pass_f32(int64_t n_nodes, int64_t e_begin, int64_t e_end,
                                const int32_t* row_of, const int32_t* eid, const float* logits,
                                int logits_in_csr_order, float* out, float* out_csr, void* workspace,
                                size_t workspace_bytes, kgat_stream_t stream);

/* Backward of the above (DGL 0.4.x EdgeSoftmax.backward), rows [row0, row0 + n_rows):
 *   grad_s[e] = a[e]*g[e] - a[e] * sum_{e'->dst e} a[e']*g[e'];  arrays in edge-id order
 * (eid != NULL) or CSR order (eid == NULL). */
int kgat_edge_softmax_bwd_f32(int64_t n_rows, int64_t row0, const int32_t* indptr,
                              const int32_t* eid, const float* a, const float* grad_a,
                              float* grad_logits, kgat_stream_t stream);

/* ---------------------------------------------------------------- aggregation (S1, S1b)
 * Replaces g.update_all(fn.u_mul_e('h','w','m'), fn.sum('m','h_neighbor')) of reference
 * models.py:63 (DGL binary_reduce(sum, mul, SRC, EDGE) with (E,1) broadcast):
 *   out[v - row0, :] = sum_{p in [indptr[v], indptr[v+1])} w_p * X[col[p], :]
 * for rows v in [row0, row0 + n_rows), whose CSR positions are [e_begin, e_end) =
 * [indptr[row0], indptr[row0 + n_rows]) (passed by value so the call needs no device read).
 * w_p = w[eid[p]] if eid != NULL (w in edge-id order) else w[p] (w in CSR order).
 * Rows with no in-edge are written as 0.  Summation order is fixed, no float atomics:
 * results are bitwise reproducible.  X has D columns, fp32 row-major, 16-byte aligned.
 * row_of (destination per CSR position) is required by the MERGE algorithm; `order` (a row
 * schedule from kgat_row_order_by_degree over the same row range, entries relative to
 * row0) only applies to ROWS.  workspace: kgat_spmm_workspace_bytes(e_end - e_begin, D).
 * self_out (may be NULL; with KGAT_SPMM_MUL_SELF, CSR-ordered weights, MERGE / AUTO): the launch also
 * writes X[v, :] to self_out[(v - row0) * self_stride + 0..D) - the ego block [h0 | ...] of
 * Model.gnn's readout (models.py:159,168) from the register that already holds the row, instead of a
 * separate copy pass; self_stride in floats, a multiple of 4, self_out 16-byte aligned.
 * Backward w.r.t. X (S1b) is this same call on the CSR of the reversed graph. */
size_t kgat_spmm_workspace_bytes(int64_t n_edges, int D);
int kgat_spmm_umule_sum_f32(int64_t n_rows, int64_t row0, int64_t e_begin, int64_t e_end, int D,
                            const int32_t* indptr, const int32_t* col, const int32_t* row_of,
                            const int32_t* eid, const float* X, const float* w, float* out,
                            const int32_t* order, void* workspace, size_t workspace_bytes,
                            unsigned flags, int algo, float* self_out, int64_t self_stride,
                            kgat_stream_t stream);

/* Measurement aid, not an operator of the path (SURVEY 8d asks for the bound that binds; on the cache-resident CKGs
 * that is the rate at which gathered rows cross the cache fabric, not HBM): reads the rows X[col[p], :] of CSR
 * positions p in [0, n_edges) with the aggregation's access pattern - D / 4 lanes x 16 bytes per row, 8 rows in
 * flight per lane group - and does nothing else (no weights, no output).  sink: a scratch of at least
 * ceil(n_edges / 2048) * 4 x 16 bytes that is never written for finite data.  D in {16, 32, 64, 128}. */
int kgat_gather_probe_f32(int64_t n_edges, int D, const int32_t* col, const float* X, float* sink,
                          kgat_stream_t stream);

/* Gradient of the aggregation w.r.t. the edge weight (DGL backward_rhs of the same op):
 *   grad_w[e] = < X[src e, :], grad_out[dst e, :] >,  edge-id order. */
int kgat_sddmm_dot_f32(int64_t n_edges, int D, const int32_t* src, const int32_t* dst,
                       const float* X, const float* grad_out, float* grad_w,
                       kgat_stream_t stream);

/* ---------------------------------------------------------------- max reducer with argmax (additive within ABI 16)
 * g.update_all(fn.u_mul_e('h','w','m') | fn.copy_src('h','m'), fn.max('m','o')) - DGL's fn.max reducer - and, with the
 * winning edge recorded, the max-times product behind the attention-path explanations of the KGAT paper (section 4.5,
 * figure 4: the walk of highest attention product from an item to a user):
 *   out[v - row0, j] = max over CSR positions p of row v of  w[p] * X[col[p], j]    (w == NULL: X[col[p], j])
 *   arg[v - row0, j] = the edge that attains it: eid[p] (eid != NULL: CSR position -> edge id), else p
 * over rows v in [row0, row0 + n_rows) whose CSR positions are [e_begin, e_end), as kgat_spmm_umule_sum_f32; w is in
 * CSR order.  arg [n_rows x D int32] may be NULL (not written).  Comparison is IEEE > on the fp32 products (-0.0 ties
 * with 0.0); among equal products the smallest edge id (without eid: position) wins and `out` carries its bits.  The
 * identity is -inf: a row of negative products returns a negative maximum.  A row without in-edges: out = 0 (as DGL),
 * arg = -1.  Inputs finite or +-inf; NaN: unspecified.  The sum kernel's tile decomposition (tiles of
 * kgat_spmm_tile_edges edges - any D outside {16, 32, 64, 128}: the D = 64 tile, sixteen columns per pass; a row cut
 * by tile boundaries is completed from the tiles' (value, edge) partials); no atomics, bitwise reproducible.  row_of is
 * required; D in {16, 32, 64, 128}: X, out, arg 16-byte aligned.  workspace: kgat_spmm_max_workspace_bytes of
 * (e_end - e_begin, D).  No backward. */
size_t kgat_spmm_max_workspace_bytes(int64_t n_edges, int D);
int kgat_spmm_umule_max_f32(int64_t n_rows, int64_t row0, int64_t e_begin, int64_t e_end, int D, const int32_t* indptr,
                            const int32_t* col, const int32_t* row_of, const int32_t* eid, const float* X,
                            const float* w, float* out, int32_t* arg, void* workspace, size_t workspace_bytes,
                            kgat_stream_t stream);

/* ---------------------------------------------------------------- top-4 reducer with back-pointers (additive within ABI 16)
 * The k-best max-times product behind explain.attention_paths(top = 2..4): the four walks of highest attention product
 * per (node, query) instead of one.  X is [N x Q x 4] fp32 - Q queries with four slots each, rows of 4 Q floats.  For
 * every row v in [row0, row0 + n_rows), whose CSR positions are [e_begin, e_end), and every query q the candidates are
 *   { (w[p] * X[col[p], q, s], id(p), s) : p a CSR position of row v, s in 0..3 },   id(p) = eid[p] (eid != NULL) or p
 * (w == NULL: times 1.0f; w in CSR order) and the four largest are returned in order:
 *   out      [n_rows x Q x 4 fp32]   the winners' product bits
 *   arg_edge [n_rows x Q x 4 int32]  their ids
 *   arg_slot [n_rows x Q x 4 uint8]  their source slots (a query's four bytes are one 32-bit word)
 * (a, i, r) beats (b, k, s) iff a > b, or a == b and (i < k, or i == k and r < s): IEEE comparison on the fp32 products,
 * -0.0 ties with 0.0; the (id, slot) pairs are distinct, so the order is total and the result does not depend on how
 * the tiles split a row - no atomics, bitwise reproducible.  Nothing is assumed about the order of a source's slots or
 * about signs: the identity is (-inf, INT32_MAX, 4), and every row with an in-edge has four candidates and more.  A row
 * without in-edges: out = 0, arg_edge = -1, arg_slot = 255.  Inputs finite or +-inf; NaN: unspecified.  arg_edge and
 * arg_slot may each be NULL (not written).  Q in {4, 8, 16, 32}, any other Q: KGAT_E_BADARG, as are a null pointer, a
 * negative size and workspace_bytes < kgat_spmm_max4_workspace_bytes(e_end - e_begin, Q).  row_of is required; X, out,
 * arg_edge and the workspace 16-byte aligned, arg_slot 4-byte aligned.  The tiles are kgat_spmm_tile_edges(n, 4 Q)
 * edges.  No backward. */
size_t kgat_spmm_max4_workspace_bytes(int64_t n_edges, int Q);
int kgat_spmm_umule_max4_f32(int64_t n_rows, int64_t row0, int64_t e_begin, int64_t e_end, int Q, const int32_t* indptr,
                             const int32_t* col, const int32_t* row_of, const int32_t* eid, const float* X,
                             const float* w, float* out, int32_t* arg_edge, uint8_t* arg_slot, void* workspace,
                             size_t workspace_bytes, kgat_stream_t stream);

/* ---------------------------------------------------------------- bi-interaction (B1 + B2)
 * Forward of the dense part of KGATConv (reference models.py:66) fused with the readout
 * normalisation (models.py:165-167):  Z = LeakyReLU_slope(P @ W2^T), P = h * h_N (n_rows x d_in,
 * produced by the aggregation with KGAT_SPMM_MUL_SELF), W2 = res_fc_2.weight (d_out x d_in).
 * h_out (n_rows x d_out, may be NULL) receives Z (the input of the next layer); norm_out (may
 * be NULL) receives Z / max(||Z_row||_2, 1e-12) with row stride norm_stride floats (a column
 * slice of the concatenated output).  Widths (kgat_bi_interaction_supported): d_in, d_out in
 * {16, 32, 64, 128} (MFMA kernel), or one of them in {4, 8} with the other in {4, 8, 16, 32} (one
 * lane per row). */
int kgat_bi_interaction_supported(int d_in, int d_out);
int kgat_bi_interaction_f32(int64_t n_rows, int d_in, int d_out, const float* P, const float* W2,
                            float negative_slope, float* h_out, float* norm_out,
                            int64_t norm_stride, kgat_stream_t stream);

/* (The same with the product formed on the way - what the layer runs - is kgat_aggregator_f32 with KGAT_FORM_BI.) */

/* ---------------------------------------------------------------- one KGATConv forward in one pass (S1 + B1 + B2)
 * Replaces reference models.py:63-66 (update_all(u_mul_e, sum); th.mul; res_fc_2; LeakyReLU) and the
 * F.normalize of models.py:165 for the no-grad forward: kgat_spmm_umule_sum_f32 with KGAT_SPMM_MUL_SELF
 * (same arguments, CSR-ordered weights, MERGE algorithm) whose completed rows P = h * h_N never leave the
 * workgroup: they are collected in LDS and take Z = LeakyReLU_slope(P W2^T) (fp32 MFMA) there; h_out /
 * norm_out / norm_stride as kgat_bi_interaction_f32 (norm_out 16-byte aligned, norm_stride a multiple of
 * 4).  Results are bit-identical to the two-launch sequence.  `scratch` (n_rows x d_in floats, contents
 * undefined afterwards) takes the P rows of tiles that span more rows than the LDS buffer holds.
 * Widths (kgat_spmm_bi_fused_supported): d_in, d_out in {16, 32, 64} with d_out <= d_in.
 * workspace: kgat_spmm_workspace_bytes(e_end - e_begin, d_in). */
int kgat_spmm_bi_fused_supported(int d_in, int d_out);
int kgat_spmm_bi_fused_f32(int64_t n_rows, int64_t row0, int64_t e_begin, int64_t e_end, int d_in, int d_out,
                           const int32_t* indptr, const int32_t* col, const int32_t* row_of,
                           const float* X, const float* w, const float* W2, float negative_slope,
                           float* h_out, float* norm_out, int64_t norm_stride, float* scratch,
                           void* workspace, size_t workspace_bytes, float* self_out, int64_t self_stride,
                           kgat_stream_t stream);

/* F.normalize(x, p=2, dim=1, eps=1e-12) of n_rows contiguous d-wide rows (reference
 * models.py:165) into a destination with row stride out_stride floats (a column slice of the
 * concatenated output, models.py:167).  Used where the rows of a layer come back from the
 * multi-GPU exchange and the fused kernel above could not normalise them. */
int kgat_l2_normalize_rows_f32(int64_t n_rows, int d, const float* x, float* out, int64_t out_stride,
                               kgat_stream_t stream);

/* The concatenated readout of Model.gnn (reference models.py:159-168: [h0 | normalize(h1) | ...]) from
 * n_blocks (<= 8) separately held row-major blocks in one pass: block k is n_rows x widths[k]
 * (widths multiples of 4, <= 128; `blocks` and `widths` are HOST arrays, the pointers in `blocks`
 * device pointers), copied as is or L2-normalised per row (normalize[k] != 0, eps 1e-12) into
 * columns [sum of the earlier widths, +widths[k]) of `out` (row stride out_stride floats). */
int kgat_readout_concat_f32(int64_t n_rows, int n_blocks, const float* const* blocks, const int* widths,
                            const int* normalize, float* out, int64_t out_stride, kgat_stream_t stream);

/* Permute a per-edge array: out[i] = in[index[i]]. */
int kgat_gather_f32(int64_t n, const int32_t* index, const float* in, float* out,
                    kgat_stream_t stream);
int kgat_gather_i32(int64_t n, const int32_t* index, const int32_t* in, int32_t* out,
                    kgat_stream_t stream);

/* The same permutation of fp32 values, out[i] = in[src_of[i]], for a permutation src_of that stays the same from call
 * to call (graph-static: CSR position of every edge id and the like), without a random global access: two streaming
 * passes through LDS over a plan the caller builds once per permutation.  With T = kgat_permute_tile, sources cut into
 * chunks and destinations into blocks of T consecutive items, and an intermediate array tmp[n] ordered by
 * (destination block, source position):
 *   slot_a[p]       rank of source position p inside its chunk under the order (destination block, p)
 *   dst_a[c*T + i]  index in tmp of the item at rank i of chunk c
 *   slot_b[j]       offset inside its destination block of the item at tmp[j]
 * (ranks and offsets < T, 16 bit).  Launch 1 writes tmp, launch 2 reads it and writes out; in, out and tmp are three
 * distinct buffers of n floats; slot_a, slot_b, in, out and tmp 16-byte aligned.  Values move as 32-bit words.  A
 * damaged plan gives wrong values, never an access outside the buffers.
 * kgat_permute_supported: 1 while the mean (chunk, block) run T * T / n is at least a 64-byte sector (16 items) -
 * beyond that (n > 16,777,216 at T = 16,384) the passes stop streaming and kgat_gather_f32 stays the form to call;
 * the entry returns KGAT_E_UNSUPPORTED there. */
int kgat_permute_tile(void);
int kgat_permute_supported(int64_t n);
int kgat_permute_f32(int64_t n, const uint16_t* slot_a, const int32_t* dst_a, const uint16_t* slot_b, const float* in,
                     float* out, float* tmp, kgat_stream_t stream);

/* kgat_edge_softmax_f32 (out = NULL, out_csr) followed by kgat_permute_f32 (out_csr -> out) in three launches instead
 * of four, same bits (ABI 16, additive): the sweep; the permutation's bin pass, which also finishes the rows the
 * sweep's ranges cut - it multiplies their provisional values by the row's factor while it holds them and writes the
 * corrected 16-byte pieces back to out_csr in place - and the place pass.  Arguments as those two entries take them:
 * eid is the index map the logits are read through (may be NULL with logits_in_csr_order = 1), slot_a / dst_a / slot_b
 * the plan of the permutation CSR position -> edge id, out (edge-id order), out_csr, tmp and logits four distinct
 * buffers of E floats, workspace of kgat_edge_softmax_workspace_bytes.
 * The _supported companion: 1 when e_begin = 0 (the whole graph: chunk boundaries of the bin pass are then range
 * boundaries of the sweep), kgat_permute_supported holds for E = e_end, and the permutation's tile is a whole number
 * of sweep ranges.  Otherwise, and when slot_a, slot_b, out, out_csr, tmp or workspace is not 16-byte aligned, the
 * entry launches nothing and returns KGAT_E_UNSUPPORTED: the two separate entries remain the form to call. */
int kgat_edge_softmax_permuted_supported(int64_t e_begin, int64_t e_end);
int kgat_edge_softmax_permuted_f32(int64_t n_nodes, int64_t e_begin, int64_t e_end, const int32_t* indptr,
                                   const int32_t* row_of, const int32_t* eid, const float* logits,
                                   int logits_in_csr_order, const uint16_t* slot_a, const int32_t* dst_a,
                                   const uint16_t* slot_b, float* out, float* out_csr, float* tmp, void* workspace,
                                   size_t workspace_bytes, kgat_stream_t stream);

/* ---------------------------------------------------------------- training form of the layer (8f #1)
 * The forward of one KGATConv under autograd is kgat_aggregator_train_f32 (below); these are the pieces around it.
 * kgat_add3_rows_f32: out = (a + b) + c over n_rows x d, a being a column slice (rows of a_stride floats) of a wider
 * matrix: the gradient arriving at the embedding table through Model.gnn's three paths (the ego block of the readout's
 * gradient, the aggregated branch, the elementwise branch of layer 0) in one pass instead of two. */
int kgat_add3_rows_f32(int64_t n_rows, int d, const float* a, int64_t a_stride, const float* b, const float* c, float* out,
                       kgat_stream_t stream);
/* Backward head of the same layer: with y = h_out saved by the forward,
 *   grad_z = [grad_a + grad_b + normalize_bwd(grad_norm; y)] * mask/(1-p) * LeakyReLU'(z)
 * (grad_a, grad_b: gradients arriving at h_out from the next layer, either may be NULL;
 * grad_norm: gradient of the normalised copy, row stride grad_norm_stride, may be NULL).
 * The rest of the backward is dense: grad_P = grad_z W2, grad_W2 = grad_z^T (H * HN), then
 * grad_H = grad_P * HN + A^T (grad_P * H) (kgat_mul2_f32 + the SpMM on the reversed CSR). */
int kgat_bi_interaction_bwd_pre_f32(int64_t n_rows, int d_out, const float* h_out, const float* grad_a,
                                    const float* grad_b, const float* grad_norm, int64_t grad_norm_stride,
                                    float negative_slope, float drop_p, uint64_t seed, int64_t row0, float* grad_z,
                                    kgat_stream_t stream);
/* The same two steps in one pass (round 4) are kgat_aggregator_bwd_input_f32, the weight gradient
 * kgat_aggregator_bwd_weight_f32 (below).  Their widths: d_in, d_out in {16, 32, 64, 128}; the number of per-workgroup
 * partial sums the weight gradient leaves for n_rows rows: */
int kgat_bi_interaction_bwd_input_supported(int d_in, int d_out);
int64_t kgat_bi_interaction_bwd_weight_partials(int64_t n_rows);
/* out_s = the sum of set s's n_partials_s partials (each n_elems_s floats, a multiple of 4, back to back) for up to four
 * sets in ONE launch - the weight gradients of a propagation stack's layers, whose partials
 * kgat_aggregator_bwd_weight_f32 leaves to the caller.  HOST arrays of n_sets entries.  A fixed order of additions
 * (sixteen strided lane sums, then a shuffle tree): bitwise reproducible; not the order of a sequential sum. */
int kgat_sum_partials_f32(int n_sets, const float* const* partials_host, float* const* out_host,
                          const int64_t* n_partials_host, const int64_t* n_elems_host, kgat_stream_t stream);
/* ab = a * b and ac = a * c elementwise in one pass (n a multiple of 4). */
int kgat_mul2_f32(int64_t n, const float* a, const float* b, const float* c, float* ab, float* ac,
                  kgat_stream_t stream);

/* ---------------------------------------------------------------- the KGAT layer's three aggregators
 * The dense part of KGATConv for any `form` (KGAT_FORM_*), i.e. with res_type "Bi", "GCN" or
 * "GraphSage" - the KGAT paper's three aggregators (Wang et al. 2019, "Information Aggregation", eqs. 6-8), whose hook
 * the reference keeps in KGATConv.__init__ (models.py:50-58: res_type, the commented-out res_fc of :55):
 *   GCN:        Z = LeakyReLU_slope((H + HN) W^T),      W = res_fc.weight   (d_out x d_in)
 *   GraphSage:  Z = LeakyReLU_slope([H | HN] W^T),      W = res_fc.weight   (d_out x 2 d_in; columns [0, d_in) act on H)
 *   Bi:         Z = LeakyReLU_slope((H * HN) W^T),      W = res_fc_2.weight (d_out x d_in)
 * HN = update_all(u_mul_e('h','w','m'), sum('m','h_neighbor')) (models.py:63), both H and HN n_rows x d_in.  Widths
 * (kgat_aggregator_supported): Bi as kgat_bi_interaction_supported; GCN and GraphSage d_in, d_out in {16, 32, 64, 128}
 * (others: KGAT_E_UNSUPPORTED - a caller forms those in a library GEMM).
 * kgat_aggregator_f32: the no-grad layer.  The combination is formed while the rows are loaded (round 4), so that the
 * aggregation needs no epilogue (its KGAT_SPMM_MUL_SELF form pays a dependent load per finished row inside the edge
 * loop: 91 vs 78 us on the benchmark graph); h_out / norm_out / norm_stride as kgat_bi_interaction_f32.  self_out (may
 * be NULL): the rows of H are also copied to self_out[row * self_stride + 0..d_in) - the ego block [h0 | ...] of
 * Model.gnn's readout (models.py:159,168); 16-byte aligned, self_stride a multiple of 4 floats.  KGAT_FORM_BI: the same
 * bits as KGAT_SPMM_MUL_SELF + kgat_bi_interaction_f32.
 * kgat_aggregator_deferred_f32: the pair update_all(u_mul_e, sum) -> dense part with one launch less (round 4).  The
 * aggregation's MERGE algorithm cuts the CSR positions into tiles of kgat_spmm_tile_edges(e_end - e_begin, D) edges; a
 * tile leaves its first and its last row as partial sums in the workspace and a second, dependent launch adds them up
 * and zero-fills the rows without in-edges.  With KGAT_SPMM_DEFER_FINISH (plain operator, CSR-ordered weights, MERGE /
 * AUTO, D in {16, 32, 64, 128}) that launch is skipped: those rows of `out` are NOT written, and this entry - the same
 * operator as kgat_aggregator_f32 - forms them on the way from `indptr_rows` (= indptr + row0: the row offsets of the
 * call's rows 0 .. n_rows), the edge range and the untouched workspace, in the second launch's order of additions:
 * bit-identical results.  d_in, d_out in {16, 32, 64, 128}; nothing else may use the workspace between the two calls.
 * (Benchmark graph: the three second launches cost 13 us of a 0.44 ms step; forming their rows costs the dense kernels 6.)
 * kgat_aggregator_train_f32: the forward of one KGATConv under autograd (reference models.py:63-70 with mess_drop
 * active): h_out = dropout_p(LeakyReLU(combine(H, HN) W^T)), norm_out = F.normalize(h_out), self_out as above.  The
 * dropout mask is a counter-based hash of (seed, (row0 + row) * d_out + column): keep <=> hash >= p * 2^32, kept
 * values scaled by 1/(1-p); the backward recomputes it from the same seed.  row0 = global index of the first row when
 * H is a row range of a larger matrix (a destination shard draws the mask of the unsharded layer; 0 otherwise). */
int kgat_spmm_tile_edges(int64_t n_edges, int D);  /* 0: D outside {16, 32, 64, 128} */
int kgat_aggregator_supported(int form, int d_in, int d_out);
int kgat_aggregator_f32(int form, int64_t n_rows, int d_in, int d_out, const float* H, const float* HN, const float* W,
                        float negative_slope, float* h_out, float* norm_out, int64_t norm_stride, float* self_out,
                        int64_t self_stride, kgat_stream_t stream);
int kgat_aggregator_deferred_f32(int form, int64_t n_rows, int d_in, int d_out, const float* H, const float* HN,
                                 const float* W, float negative_slope, float* h_out, float* norm_out,
                                 int64_t norm_stride, float* self_out, int64_t self_stride, const int32_t* indptr_rows,
                                 int64_t e_begin, int64_t e_end, const void* spmm_workspace, int tile_edges,
                                 kgat_stream_t stream);
int kgat_aggregator_train_f32(int form, int64_t n_rows, int d_in, int d_out, const float* H, const float* HN,
                              const float* W, float negative_slope, float drop_p, uint64_t seed, int64_t row0,
                              float* h_out, float* norm_out, int64_t norm_stride, float* self_out, int64_t self_stride,
                              kgat_stream_t stream);
/* Backward of the dense part towards its inputs (the layer under autograd), from grad_z (n_rows x d_out,
 * kgat_bi_interaction_bwd_pre_f32); grad_P = grad_z W is formed per 16-row tile on the fp32 MFMA, never written, and
 *   Bi:        grad_agg = grad_P * H, grad_self = grad_P * HN
 *   GCN:       grad_agg = grad_P (the gradient through h_N and through h alike; grad_self unused, may be NULL)
 *   GraphSage: grad_agg = grad_P[:, d_in:2 d_in] (the h_N half), grad_self = grad_P[:, 0:d_in] (the h half)
 * grad_agg is what the reversed-CSR aggregation then sums; grad_self goes to h directly (both n_rows x d_in).  H and
 * HN are read for Bi only.  Widths (kgat_aggregator_bwd_supported): d_in, d_out in {16, 32, 64, 128}. */
int kgat_aggregator_bwd_supported(int form, int d_in, int d_out);
int kgat_aggregator_bwd_input_f32(int form, int64_t n_rows, int d_in, int d_out, const float* grad_z, const float* W,
                                  const float* H, const float* HN, float* grad_agg, float* grad_self,
                                  kgat_stream_t stream);
/* grad_W = grad_z^T (H * HN) (Bi), grad_z^T (H + HN) (GCN), grad_z^T [H | HN] (GraphSage: d_out x 2 d_in) as per-workgroup
 * partial sums: partials[b] (d_out x d_in row-major, d_out x 2 d_in for GraphSage) is the product over the 64-row slabs
 * b, b + n_partials, ... with n_partials = kgat_bi_interaction_bwd_weight_partials(n_rows); the combination is formed
 * on the way and never written; the caller adds the partials up in any fixed order (kgat_sum_partials_f32). */
int kgat_aggregator_bwd_weight_f32(int form, int64_t n_rows, int d_in, int d_out, const float* grad_z, const float* H,
                                   const float* HN, float* partials, int64_t n_partials, kgat_stream_t stream);

/* ---------------------------------------------------------------- the two-term Bi-Interaction aggregator ("Bi2")
 * (ABI 13) The Bi-Interaction aggregator as the KGAT paper states it (Wang et al. 2019, eq. 8, and the authors' code):
 *   z1 = (H + HN) W1^T   W1 = res_fc.weight   (d_out x d_in; the line the reference keeps commented out, models.py:55)
 *   z2 = (H * HN) W2^T   W2 = res_fc_2.weight (d_out x d_in; the reference's own term, models.py:66)
 *   Z  = LeakyReLU_slope(z1) + LeakyReLU_slope(z2),   out = mess_drop(Z) (one mask on the sum, models.py:70)
 * i.e. KGATConv with res_type "Bi2".  No bias; HN = update_all(u_mul_e('h','w','m'), sum('m','h_neighbor')) (models.py:63).
 * The activation sits between the contractions and the sum: the kernels keep two accumulator sets per 16-row tile and
 * stage both weights in LDS.  Not a `form` of the kgat_aggregator_* entries (two weights, and the backward needs a
 * record those do not have).  Widths (kgat_bi2_supported / kgat_bi2_bwd_supported): d_in, d_out in {16, 32, 64, 128};
 * others: KGAT_E_UNSUPPORTED (a caller forms those in library GEMMs).  All entries are bitwise reproducible from call
 * to call (no atomics) and check their arguments before any device work.
 *
 * kgat_bi2_f32 / kgat_bi2_deferred_f32: the no-grad layer, with the arguments and outputs of kgat_aggregator_f32 /
 * kgat_aggregator_deferred_f32 and W1, W2 in W's place - h_out (n_rows x d_out, may be NULL if norm_out is given), the
 * L2-normalised rows into norm_out (row stride norm_stride: a column slice of the readout), the rows of H into
 * self_out (the ego block).  The deferred entry forms the rows the aggregation's KGAT_SPMM_DEFER_FINISH launch left as
 * tile partials and gives the plain entry's bits.
 * kgat_bi2_train_f32: the training form - hash dropout (drop_p, seed, row0 as kgat_aggregator_train_f32) on the sum
 * of the two terms; h_out is required.  It also writes the SIGN RECORD `signs`, n_rows x d_out bytes (4-byte aligned):
 * bit 0 = (z1 > 0), bit 1 = (z2 > 0) of that element before dropout - the sign of the saved output no longer tells
 * LeakyReLU'(z1) and LeakyReLU'(z2) apart (LeakyReLU'(0) = slope, as in kgat_bi_interaction_bwd_pre_f32). */
int kgat_bi2_supported(int d_in, int d_out);
int kgat_bi2_bwd_supported(int d_in, int d_out);
int kgat_bi2_f32(int64_t n_rows, int d_in, int d_out, const float* H, const float* HN, const float* W1, const float* W2,
                 float negative_slope, float* h_out, float* norm_out, int64_t norm_stride, float* self_out,
                 int64_t self_stride, kgat_stream_t stream);
int kgat_bi2_deferred_f32(int64_t n_rows, int d_in, int d_out, const float* H, const float* HN, const float* W1,
                          const float* W2, float negative_slope, float* h_out, float* norm_out, int64_t norm_stride,
                          float* self_out, int64_t self_stride, const int32_t* indptr_rows, int64_t e_begin,
                          int64_t e_end, const void* spmm_workspace, int tile_edges, kgat_stream_t stream);
int kgat_bi2_train_f32(int64_t n_rows, int d_in, int d_out, const float* H, const float* HN, const float* W1,
                       const float* W2, float negative_slope, float drop_p, uint64_t seed, int64_t row0, float* h_out,
                       uint8_t* signs, float* norm_out, int64_t norm_stride, float* self_out, int64_t self_stride,
                       kgat_stream_t stream);
/* Backward head of the two-term layer (the autograd of F.normalize, mess_drop and the two LeakyReLU): with
 *   g = [grad_a + grad_b + normalize_bwd(grad_norm; h_out)] * keep / (1 - p)
 * exactly as kgat_bi_interaction_bwd_pre_f32 forms it before its last factor, it writes BOTH
 *   grad_z1 = g * LeakyReLU'(z1)   and   grad_z2 = g * LeakyReLU'(z2)      (n_rows x d_out each)
 * with the two slopes read from the training forward's sign record, so that the dense backward kernels read plain
 * gradients.  grad_a / grad_b / grad_norm may be NULL. */
int kgat_bi2_bwd_pre_f32(int64_t n_rows, int d_out, const float* h_out, const uint8_t* signs, const float* grad_a,
                         const float* grad_b, const float* grad_norm, int64_t grad_norm_stride, float negative_slope,
                         float drop_p, uint64_t seed, int64_t row0, float* grad_z1, float* grad_z2,
                         kgat_stream_t stream);
/* Backward towards the inputs: P1 = grad_z1 W1 and P2 = grad_z2 W2 per 16-row tile (never written), and in one pass
 *   grad_agg  = P1 + P2 * H    (what the reversed-CSR aggregation then sums: ONE aggregation per layer)
 *   grad_self = P1 + P2 * HN   (goes to h directly)                        (both n_rows x d_in) */
int kgat_bi2_bwd_input_f32(int64_t n_rows, int d_in, int d_out, const float* grad_z1, const float* grad_z2,
                           const float* W1, const float* W2, const float* H, const float* HN, float* grad_agg,
                           float* grad_self, kgat_stream_t stream);
/* grad_W1 = grad_z1^T (H + HN) and grad_W2 = grad_z2^T (H * HN) as per-workgroup partials, in ONE launch that reads the
 * rows of H and HN once (the slab scheme of kgat_aggregator_bwd_weight_f32): partials_w1[b], partials_w2[b] are d_out x d_in,
 * n_partials = kgat_bi_interaction_bwd_weight_partials of n_rows, the caller adds them (kgat_sum_partials_f32). */
int kgat_bi2_bwd_weight_f32(int64_t n_rows, int d_in, int d_out, const float* grad_z1, const float* grad_z2,
                            const float* H, const float* HN, float* partials_w1, float* partials_w2, int64_t n_partials,
                            kgat_stream_t stream);

/* ---------------------------------------------------------------- GraphSAGE layer (gnn_model = "graphsage")
 * The kernels behind dgl.nn.pytorch.conv.SAGEConv(d_in, d_out, aggregator_type="mean", feat_drop, activation) of
 * reference models.py:98-100,107-109 (DGL 0.4.x SAGEConv.forward on a homogeneous graph):
 *   hd = feat_drop(h);  h_neigh[v] = mean_{u->v} hd[u];  rst = act(fc_self(hd) + fc_neigh(h_neigh)).
 *
 * kgat_copy_reduce_f32 replaces g.update_all(fn.copy_src('h','m'), fn.sum('m','h') | fn.mean('m','h')) (DGL
 * copy_reduce(sum | mean, SRC)):
 *   out[v - row0, :] = reduce_{p in [indptr[v], indptr[v+1])} X[col[p], :]
 * over rows v in [row0, row0 + n_rows) whose CSR positions are [e_begin, e_end), as kgat_spmm_umule_sum_f32 - but no
 * per-edge weight is read.  reduce = KGAT_REDUCE_SUM, or KGAT_REDUCE_MEAN: the fp32 sum divided (true division) by
 * the row's number of positions (multi-edges count); rows without in-edges are written as 0.  A fixed order of
 * additions, no float atomics: bitwise reproducible.  D in {16, 32, 64, 128}: the merge-path kernel (row_of
 * required, X and out 16-byte aligned); any other D: one wavefront per row (row_of not read).
 * workspace: kgat_spmm_workspace_bytes(e_end - e_begin, D).  The backward of the mean w.r.t. X is this call with
 * KGAT_REDUCE_SUM on the CSR of the reversed graph over the rows kgat_sage_bwd_input_f32 writes to grad_agg. */
int kgat_copy_reduce_f32(int64_t n_rows, int64_t row0, int64_t e_begin, int64_t e_end, int D, const int32_t* indptr,
                         const int32_t* col, const int32_t* row_of, const float* X, float* out, int reduce,
                         void* workspace, size_t workspace_bytes, kgat_stream_t stream);

/* The dense part of SAGEConv (fc_self(hd) + fc_neigh(h_neigh), then the activation; reference models.py:99,108) and,
 * on the no-grad readout path, the F.normalize of models.py:165:
 *   Z = act(H W_self^T + HN W_neigh^T + b_self + b_neigh),  act = KGAT_ACT_NONE | KGAT_ACT_RELU
 * H = hd, HN = h_neigh (n_rows x d_in), W_self / W_neigh = fc_self.weight / fc_neigh.weight (d_out x d_in), b_self /
 * b_neigh (d_out, either may be NULL).  h_out (n_rows x d_out, may be NULL) receives Z; norm_out (may be NULL) Z /
 * max(||Z_row||_2, 1e-12) with row stride norm_stride floats; self_out (may be NULL) a copy of H with row stride
 * self_stride (the ego block [h0 | ...] of Model.gnn's readout, models.py:159,168).  Strides multiples of 4 floats,
 * every buffer 16-byte aligned.  fp32 MFMA (v_mfma_f32_16x16x4_f32); widths (kgat_sage_dense_supported): d_in, d_out
 * in {16, 32, 64, 128}, others return KGAT_E_UNSUPPORTED. */
int kgat_sage_dense_supported(int d_in, int d_out);
int kgat_sage_dense_f32(int64_t n_rows, int d_in, int d_out, const float* H, const float* HN, const float* W_self,
                        const float* W_neigh, const float* b_self, const float* b_neigh, int act, float* h_out,
                        float* norm_out, int64_t norm_stride, float* self_out, int64_t self_stride,
                        kgat_stream_t stream);

/* SAGEConv's feat_drop (nn.Dropout of reference models.py:99,108 on the layer input) with the counter hash of
 * kgat_aggregator_train_f32: out = (x + x2) * keep / (1 - drop_p) over n_rows x d elements (x2 may be NULL),
 * keep <=> hash(seed, row * d + column) >= drop_p * 2^32.  Forward: the dropped input, materialised once.  Backward:
 * the same call on the gradient (x, x2 = the gradient's two paths: through fc_self and through the aggregation). */
int kgat_dropout_rows_f32(int64_t n_rows, int d, const float* x, const float* x2, float drop_p, uint64_t seed,
                          float* out, kgat_stream_t stream);

/* Backward of kgat_sage_dense_f32 towards its inputs (reference models.py:99,108 under autograd), from grad_pre =
 * the gradient at the pre-activation (kgat_bi_interaction_bwd_pre_f32 with slope 0 for ReLU, 1 for none, drop_p 0):
 *   grad_self = grad_pre W_self,  grad_agg[v] = (grad_pre W_neigh)[v] / max(indptr[v+1] - indptr[v], 1)
 * (n_rows x d_in each; grad_agg is what kgat_copy_reduce_f32 (sum) then aggregates over the reversed CSR: the
 * gradient through the mean).  indptr: the forward CSR's row offsets.  Widths as kgat_sage_dense_f32. */
int kgat_sage_bwd_input_f32(int64_t n_rows, int d_in, int d_out, const float* grad_pre, const float* W_self,
                            const float* W_neigh, const int32_t* indptr, float* grad_self, float* grad_agg,
                            kgat_stream_t stream);
/* The four parameter gradients as per-workgroup partials: part_self[b] / part_neigh[b] (d_out x d_in) = grad_pre^T H /
 * grad_pre^T HN over the 64-row slabs b, b + n_partials, ...; part_bias[b] (d_out) = the column sums of grad_pre over
 * the same rows (the gradient of b_self and of b_neigh).  n_partials = kgat_bi_interaction_bwd_weight_partials(n_rows);
 * the caller adds the partials (kgat_sum_partials_f32).  Widths as kgat_sage_dense_f32. */
int kgat_sage_bwd_weight_f32(int64_t n_rows, int d_in, int d_out, const float* grad_pre, const float* H,
                             const float* HN, float* part_self, float* part_neigh, float* part_bias, int64_t n_partials,
                             kgat_stream_t stream);

/* ---------------------------------------------------------------- TransR KG step
 * Loss and gradients of reference models.py:114-133 (transR; bmm_maybe_select :13-47,
 * _L2_loss_mean :9-11) for one batch of triplets (h[b], r[b], pos_t[b], neg_t[b]):
 *   a_x = ent[x] W_R[r],  u_x = a_x / max(|a_x|, 1e-12),  u_r = rel[r] / max(|rel[r]|, 1e-12)
 *   loss = mean_b softplus(|u_h+u_r-u_p|^2 - |u_h+u_r-u_n|^2)
 *          + reg_lambda * sum_{v in h,r,p,n} mean_b |u_v|^2 / 2
 * loss: 1 float.  grad_ent (n_nodes x d, dense: rows not in the batch are zeroed, as the
 * reference's non-sparse nn.Embedding gradient), grad_W (R x d x k), grad_rel (R x k): all three
 * or none (NULL: loss only).  Fixed summation orders (sorted batch, no atomics): bitwise
 * reproducible.  Needs d, k multiples of 4 and <= 128, 3*batch <= 8192 (the batch is sorted by one workgroup in
 * LDS), n_rel <= 4096, n_nodes < 2^31 (kgat_transr_supported; beyond it the Python layer takes torch operators). */
int kgat_transr_supported(int64_t n_nodes, int d, int k, int n_rel, int64_t batch);
size_t kgat_transr_workspace_bytes(int64_t batch, int d, int k, int n_rel);
int kgat_transr_loss_grad_f32(int64_t n_nodes, int n_rel, int d, int k, int64_t batch, const int32_t* h,
                              const int32_t* r, const int32_t* pos_t, const int32_t* neg_t, const float* ent,
                              const float* W_R, const float* rel, float reg_lambda, float* loss, float* grad_ent,
                              float* grad_W, float* grad_rel, void* workspace, size_t workspace_bytes,
                              kgat_stream_t stream);
/* The same computation in the two halves autograd asks for.  kgat_transr_forward_f32: the loss, with the per-sample
 * rows and the weight-gradient partials left in `workspace`; kgat_transr_backward_f32 (same batch arrays, same
 * workspace, untouched in between): the three gradients, multiplied by grad_scale[0] - a DEVICE scalar, the gradient
 * arriving at the loss (NULL = 1) - inside the final ordered reductions: no host synchronisation and no extra pass
 * over the dense n_nodes x d gradient (round 4 multiplied the three gradients by it in three torch launches, 22 us
 * of the 0.3 ms KG step).  Same bits as kgat_transr_loss_grad_f32 for grad_scale = 1. */
int kgat_transr_forward_f32(int64_t n_nodes, int n_rel, int d, int k, int64_t batch, const int32_t* h, const int32_t* r,
                            const int32_t* pos_t, const int32_t* neg_t, const float* ent, const float* W_R,
                            const float* rel, float reg_lambda, float* loss, void* workspace, size_t workspace_bytes,
                            kgat_stream_t stream);
int kgat_transr_backward_f32(int64_t n_nodes, int n_rel, int d, int k, int64_t batch, const int32_t* h, const int32_t* r,
                             const int32_t* pos_t, const int32_t* neg_t, const float* grad_scale, float* grad_ent,
                             float* grad_W, float* grad_rel, void* workspace, size_t workspace_bytes,
                             kgat_stream_t stream);

/* The KG phase of an epoch as three-launch iterations (round 6; reference kgat.py:116-136: for every sampled batch
 * transR -> backward -> optimizer.step -> zero_grad; 1,641 iterations per epoch on the amazon-book shape).
 *
 * kgat_transr_presort_f32: the sorts an iteration needs depend only on the batch's ids, so the batches of a whole
 * phase - h, r, pos_t, neg_t as n_batches x batch row-major arrays - are sorted by ONE launch (samples by relation
 * with the chunk table of the weight-gradient partials; the 3 x batch entity ids).  Batch b's result is the block of
 * kgat_transr_sorted_bytes(batch, n_rel) bytes at sorted + b * that.
 *
 * kgat_transr_adam_step_f32: one iteration on batch arrays h .. neg_t (batch ids each) and that batch's `sorted`
 * block: the loss (1 float at `loss`) and the step of torch.optim.Adam on the three parameters the loss reaches -
 * ent (n_nodes x d), W_R (n_rel x d x k), rel (n_rel x k), updated IN PLACE with their moments (`exp_avg_host`,
 * `exp_avg_sq_host`: HOST arrays of three device pointers in that order; `steps_host`: the three step counts AFTER
 * this step).  Dense semantics as kgat_adam_step_f32 (every row of the table moves), without a dense gradient and
 * without a scatter launch: the per-sample kernel writes its three gradient rows at their SORTED positions (the presort
 * also emits the inverse permutation and the run lengths), workgroups in the same launch tag the batch's entities in
 * `row_slot`, n_nodes 64-bit words owned by the caller - zero before the first call, never to be cleared - in which a
 * word is valid for the call whose `tag` it carries (pass a tag in [1, 2^50) that differs from every earlier call's on
 * the same row_slot: a counter), and the Adam launch takes g = 0 for an untagged row and the sum of the row's run, in
 * sorted order, for a tagged one.  The bits of kgat_transr_loss_grad_f32 followed by kgat_adam_step_f32, i.e. of the
 * reference's loss.backward(); optimizer.step().  All pointers 16-byte aligned.  Launches: per-sample kernel (+ tags),
 * weight-gradient partials (a chunk's output tiles shared by up to four workgroups) + loss, Adam. */
size_t kgat_transr_sorted_bytes(int64_t batch, int n_rel);
int kgat_transr_presort_f32(int64_t n_nodes, int n_rel, int64_t n_batches, int64_t batch, const int32_t* h,
                            const int32_t* r, const int32_t* pos_t, const int32_t* neg_t, void* sorted,
                            size_t sorted_bytes, kgat_stream_t stream);
size_t kgat_transr_step_workspace_bytes(int64_t batch, int d, int k, int n_rel);
int kgat_transr_adam_step_f32(int64_t n_nodes, int n_rel, int d, int k, int64_t batch, const int32_t* h, const int32_t* r,
                              const int32_t* pos_t, const int32_t* neg_t, const void* sorted, float* ent, float* W_R,
                              float* rel, float* const* exp_avg_host, float* const* exp_avg_sq_host,
                              const int64_t* steps_host, double lr, double beta1, double beta2, double eps,
                              float reg_lambda, float* loss, uint64_t* row_slot, uint64_t tag, void* workspace,
                              size_t workspace_bytes, kgat_stream_t stream);

/* ---------------------------------------------------------------- evaluation
 * recall@K / ndcg@K of reference metric.py:36-68 (calc_recall_ndcg with one_recall_at_k :5-7, one_dcg_at_k :8-22
 * method 1, one_ndcg_at_k :23-34) for a list of test users, without a users x items score matrix:
 *   score[u][i] = <emb[user_ids[u]], emb[item_ids[i]]>  (metric.py:48; v_mfma_f32_32x32x2_f32: exact fp32 fmaf chains)
 *   score[u][train items of u] = 0.0                     (metric.py:50 - set to 0.0, not removed)
 *   rank = the K first of a descending sort              (metric.py:51; equal scores: lower item position first)
 *   recall[u] = hits / |test items of u| (0 for an empty list), ndcg[u] = dcg / dcg of the user's own sorted hit list
 * `emb` (rows of emb_stride floats, the first F used) holds users and items; an item's POSITION i in item_ids is what
 * the train / test lists hold (the reference indexes `score` with the raw item ids of its dicts).  train_ptr /
 * test_ptr [n_users + 1] + train_items / test_items: CSR over the users in user_ids order, every list ASCENDING.
 * kgat_eval_items_kmajor_f32 first lays the item rows out as MFMA fragments (itemT: kgat_eval_items_elems floats).
 * disc[K] = 1 / log2(k + 2) in fp64 (host-computed, so the device divides by the very values numpy uses).
 * recall_out / ndcg_out: n_users doubles; topk_out (optional, n_users x K): the ranked item positions.
 * Needs 1 <= K <= 32, n_items >= K, F <= ~1100 (kgat_eval_supported).  Bitwise reproducible.
 * (Ranked lists with scores, K up to 128 and further metrics: kgat_eval_topk_f32 / kgat_eval_metrics_at_ks below.) */
int kgat_eval_supported(int F, int K);
int64_t kgat_eval_items_elems(int64_t n_items, int F);
int kgat_eval_items_kmajor_f32(int64_t n_items, int F, const float* emb, int64_t emb_stride, const int32_t* item_ids,
                               float* itemT, kgat_stream_t stream);
size_t kgat_eval_workspace_bytes(int64_t n_users, int64_t n_items, int F, int K);
int kgat_eval_recall_ndcg_f32(int64_t n_users, const int32_t* user_ids, int64_t n_items, int F, const float* emb,
                              int64_t emb_stride, const float* itemT, const int32_t* train_ptr,
                              const int32_t* train_items, const int32_t* test_ptr, const int32_t* test_items, int K,
                              const double* disc, void* workspace, size_t workspace_bytes, double* recall_out,
                              double* ndcg_out, int32_t* topk_out, kgat_stream_t stream);

/* (ABI 14) The ranked list itself, for 1 <= K <= 128, and the metrics of the KGAT paper's table at several cut-offs.
 * kgat_eval_topk_f32 replaces metric.py:48-51 (score, mask, sort - the K first of the descending sort, for every user
 * of user_ids): same inputs and the same total order as kgat_eval_recall_ndcg_f32 (itemT from
 * kgat_eval_items_kmajor_f32); for K <= 32 it launches that entry's sweep, beyond it a sweep over a candidate buffer of
 * 128 (K <= 64) or 156 entries per user (four wavefronts' buffers in a CU's LDS).  topk_items (n_users x K, int32):
 * item POSITIONS in rank order, padded with -1; topk_scores (optional, n_users x K, fp32): their scores, padding -inf.
 *   drop_train == 0 ("mask", metric.py:50): a training item scores 0.0 and can rank; needs n_items >= K.
 *   drop_train != 0 ("drop"): training items are never listed - the list a recommender shows; a user with fewer than K
 *     other items gets padding at the end; any n_items >= 1.
 * kgat_eval_topk_supported: 1 <= K <= 128 and an F whose rows fit beside the buffer (F <= 352 in registers; in LDS
 * F <= ~1100 for K <= 32, ~1000 for K <= 64, ~950 beyond).  Errors before any device work: bad sizes / null pointers
 * KGAT_E_BADARG, K or F outside the range KGAT_E_UNSUPPORTED, workspace_bytes < kgat_eval_topk_workspace_bytes
 * KGAT_E_WORKSPACE (the segments' partial lists: n_users x n_lists x K x 8 bytes).  Bitwise reproducible.
 * kgat_eval_metrics_at_ks replaces metric.py:52-63 for n_ks <= 8 cut-offs ks[j] (a HOST array, ascending, 1 <= ks[j]
 * <= K) over ranked lists topk_items (n_users x K, -1 never hits) and the test lists (CSR, ascending):
 *   out[u][j] = { recall (one_recall_at_k :5-7; 0 for an empty test list), ndcg (one_ndcg_at_k :23-34: the DCG of the
 *   first ks[j] ranks over the DCG of the user's own sorted hit list within them), precision = hits / ks[j],
 *   hit ratio = 1 if any hit else 0 }  - n_users x n_ks x 4 doubles; disc[K] as above, summed in ascending rank order:
 *   for ks[j] <= 32 recall and ndcg equal kgat_eval_recall_ndcg_f32's at K = ks[j] bit for bit. */
int kgat_eval_topk_supported(int F, int K);
size_t kgat_eval_topk_workspace_bytes(int64_t n_users, int64_t n_items, int F, int K);
int kgat_eval_topk_f32(int64_t n_users, const int32_t* user_ids, int64_t n_items, int F, const float* emb,
                       int64_t emb_stride, const float* itemT, const int32_t* train_ptr, const int32_t* train_items,
                       int K, int drop_train, void* workspace, size_t workspace_bytes, int32_t* topk_items,
                       float* topk_scores, kgat_stream_t stream);
int kgat_eval_metrics_at_ks(int64_t n_users, int K, const int32_t* topk_items, const int32_t* test_ptr,
                            const int32_t* test_items, int n_ks, const int32_t* ks, const double* disc, double* out,
                            kgat_stream_t stream);

/* (ABI 16, additive) The exact rank of every held-out item, at any depth: no candidate buffer, so no K.
 * kgat_eval_rank_f32 takes the inputs of kgat_eval_topk_f32 (itemT from kgat_eval_items_kmajor_f32; the train CSR
 * ascending and de-duplicated, n_train = train_ptr[n_users] entries) and the test CSR (ascending positions, duplicates
 * kept, n_test = test_ptr[n_users] entries).  With
 *   s'(u,i) = 0.0f if drop_train == 0 and i is a training item of u (metric.py:50), else score(u,i)   (metric.py:48)
 *   candidates(u) = every item position (drop_train == 0, "mask") | the positions not in train(u) ("drop")
 * above[e] (int32, n_test entries in test-CSR order) for the entry e of user u at item position t is
 *   #{ i in candidates(u), i != t : s'(u,i) > s'(u,t) or (s'(u,i) == s'(u,t) and i < t) }
 * - IEEE compares, -0 equal to +0, the lower position first: the total order of kgat_eval_topk_f32, whose scores
 * score(u,i) has bit for bit (the same v_mfma_f32_32x32x2_f32 chain, k order and zero padding: above[e] < K  <=>
 * topk_items[u][above[e]] == t).  The rank is above + 1.  In drop mode a test entry that is a training item is never
 * ranked: above = -1.  A duplicated test entry gets the same value twice.  target_score (optional, fp32, n_test): s'(u,t).
 * No limit on a user's list length: the lists are processed in groups of 16 thresholds.
 * kgat_eval_rank_supported(F): the widths of kgat_eval_topk_supported at K = 32 (F <= ~1100).  Errors before any
 * device work: bad sizes / null pointers KGAT_E_BADARG, F outside the range KGAT_E_UNSUPPORTED, workspace_bytes <
 * kgat_eval_rank_workspace_bytes KGAT_E_WORKSPACE (the slot table and one fp32 score per train and test entry).
 * Item segments add integer counts into the zeroed output: exact, order-independent, bitwise reproducible.
 * kgat_eval_rank_metrics: per user, over the DISTINCT test items with above >= 0, their 0-based ranks in ascending
 * order a_0 < ... < a_{T-1}, and C = n_candidates[u] (device int32: n_items, or n_items - |train(u)| in drop mode):
 *   out_at_k[u][j] = { recall = hits / |test list with duplicates| (metric.py:5-7,24,61; 0 for an empty list),
 *     ndcg = sum of disc[a] over the hits / sum of disc[0 .. hits) (metric.py:23-34, method 1), precision = hits / ks[j],
 *     hit ratio = 1 if any hit }, hits = #{ a < ks[j] }  - n_users x n_ks x 4 doubles, the definitions of
 *     kgat_eval_metrics_at_ks, for 1 <= n_ks <= 64 cut-offs ks[j] (a HOST array, ascending, 1 <= ks[j] <= n_items);
 *     disc[ks[n_ks - 1]] = 1 / log2(r + 2) in fp64, host-computed, summed in ascending rank order.
 *   out_scalar[u] = { mrr = 1 / (a_0 + 1), ap = (1/T) sum_j (j + 1) / (a_j + 1),
 *     auc = 1 - sum_j (a_j - j) / (T (C - T)) (0 when C == T), mean_rank = (1/T) sum_j (a_j + 1) }; all 0 when T == 0.
 * workspace: kgat_eval_rank_metrics_workspace_bytes(n_test) (the users' ranks, compacted and in ascending order). */
int kgat_eval_rank_supported(int F);
size_t kgat_eval_rank_workspace_bytes(int64_t n_users, int64_t n_items, int F, int64_t n_train, int64_t n_test);
int kgat_eval_rank_f32(int64_t n_users, const int32_t* user_ids, int64_t n_items, int F, const float* emb,
                       int64_t emb_stride, const float* itemT, const int32_t* train_ptr, const int32_t* train_items,
                       int64_t n_train, const int32_t* test_ptr, const int32_t* test_items, int64_t n_test,
                       int drop_train, void* workspace, size_t workspace_bytes, int32_t* above, float* target_score,
                       kgat_stream_t stream);
size_t kgat_eval_rank_metrics_workspace_bytes(int64_t n_test);
int kgat_eval_rank_metrics(int64_t n_users, int64_t n_items, const int32_t* above, const int32_t* test_ptr,
                           const int32_t* test_items, int64_t n_test, const int32_t* n_candidates, int n_ks,
                           const int32_t* ks, const double* disc, void* workspace, size_t workspace_bytes,
                           double* out_at_k, double* out_scalar, kgat_stream_t stream);

/* ---------------------------------------------------------------- edge weights without attention, node dropout (ABI 15)
 * kgat_edge_norm_f32: the weights g.edata['w'] that reference models.py:63 multiplies by when kgat.py:27,139-145 runs
 * with --use_attention False (there nothing ever writes them; the adjacency meant is the Laplacian the commented-out
 * --adj_type of kgat.py:19 names), from the device CSR alone.  For position p of the destination-major CSR (indptr,
 * row_of, col, eid of kgat_csr_from_coo) with destination v = row_of[p] and source u = col[p], in fp32:
 *   KGAT_NORM_SI:  w = 1.f / (float)(indptr[v + 1] - indptr[v])
 *   KGAT_NORM_BI:  w = 1.f / sqrtf((float)(out_indptr[u + 1] - out_indptr[u]) * (float)(indptr[v + 1] - indptr[v]))
 * (IEEE division and square root, no contraction) - out_indptr [n_nodes + 1] is the indptr of the REVERSED graph's CSR
 * (rows = sources; NULL for SI, which reads neither it nor col).  Every edge counts in both of its endpoints' degrees
 * (multi-edges and self-loops as often as they occur), so no weight is infinite or zero.  One Laplacian over all
 * relations: the per-relation normalisation of the original TensorFlow KGAT is not formed.  w_csr [n_edges]: CSR
 * order, coalesced; w_eid (optional, may be NULL; needs eid): w_eid[eid[p]] = w_csr[p].  A node id outside
 * [0, n_nodes) gives NaN and is never used as an index.  One launch; n_edges == 0 launches nothing. */
int kgat_edge_norm_f32(int64_t n_nodes, int64_t n_edges, const int32_t* indptr, const int32_t* row_of,
                       const int32_t* col, const int32_t* eid, const int32_t* out_indptr, int mode, float* w_csr,
                       float* w_eid, kgat_stream_t stream);

/* Node dropout (the KGAT paper's second regulariser beside the message dropout of reference models.py:54,69: entries of
 * the adjacency dropped with probability drop_p, survivors scaled by 1 / (1 - drop_p)) as the dropped copy of one
 * weight stream:
 *   w_out[p] = keep(seed, key[p]) ? w_in[p] * keep_scale : 0,   keep_scale = 1.f / (1.f - drop_p)  (fp32)
 * keep is the counter hash of kgat_aggregator_train_f32 over (row = edge id, d = 1, column 0): keep <=>
 * hash(seed, key[p]) >= drop_p * 2^32.  key [n_edges] holds the edge id at every position of the stream - `eid` of the
 * CSR the stream is ordered by (kgat_csr_from_coo's, or the reversed graph's for the backward stream); NULL: the stream
 * is in edge-id order (key[p] = p).  Keyed by edge id, the calls on the forward and on the reversed stream describe
 * the same surviving edge set.  drop_p in [0, 1); drop_p == 0 copies the bits.  16-byte accesses where key / w_out
 * (and, separately, w_in) are 16-byte aligned; any 4-byte alignment works.  One launch; n_edges == 0 launches nothing. */
int kgat_edge_dropout_f32(int64_t n_edges, const float* w_in, const int32_t* key, float drop_p, uint64_t seed,
                          float* w_out, kgat_stream_t stream);

/* ---------------------------------------------------------------- optimiser of the training loop (8f #1, #3)
 * One step of torch.optim.Adam (reference kgat.py:85: optim.Adam(model.parameters(), lr); amsgrad off, no weight
 * decay) over up to kgat_adam_max_tensors() parameter tensors in ONE launch - dense semantics: every element moves,
 * also where the gradient is zero.  Per element in fp32, in torch's order of operations:
 *   m <- m + (1 - beta1)(g - m);  v <- v beta2 + (1 - beta2) g g;
 *   p <- p - (lr / (1 - beta1^t)) m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
 * `*_host` arrays are HOST arrays of n_tensors entries (device pointers / element counts / the tensor's step count
 * t >= 1 AFTER this step, which may differ between tensors: a parameter that had no gradient in some steps lags).
 * zero_grads != 0 also clears the gradients it has read (optimizer.zero_grad(set_to_none=False) in the same pass). */
int kgat_adam_max_tensors(void);
int kgat_adam_step_f32(int n_tensors, const int64_t* sizes_host, float* const* params_host, float* const* grads_host,
                       float* const* exp_avg_host, float* const* exp_avg_sq_host, const int64_t* steps_host, double lr,
                       double beta1, double beta2, double eps, int zero_grads, kgat_stream_t stream);

/* ---------------------------------------------------------------- global-norm gradient clipping (additive within ABI 16)
 * reference kgat.py:32,162: `--grad_norm` ("norm to clip gradient to") and the call it feeds,
 * th.nn.utils.clip_grad_norm_(model.parameters(), args.grad_norm), between loss.backward() and optimizer.step() of the
 * CF loop.  The semantics of torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2) followed by Adam's step,
 * with every bit determined:
 *   sumsq = sum of g*g over every element of every gradient, in a FIXED order (no float atomics: bitwise reproducible);
 *   norm  = (float)sqrt(sumsq);   coef = fminf((float)max_norm / (norm + 1e-6f), 1.0f)      (fp32 DEVICE scalars)
 *   step:  gs = g * coef (its own rounding), then the element update of kgat_adam_step_f32 on gs.
 * A non-finite norm propagates (torch's error_if_nonfinite=False: a NaN norm gives a NaN coef, as torch.clamp keeps
 * it, where fminf alone would give 1); nothing is read back to the host.
 *
 * kgat_grad_norm_chain (kgat.py:32,162): the longest chain of fp32 additions any one square passes through - 16 serial
 * adds in a lane, 6 + 2 tree levels in the workgroup = 24; the per-chunk sums are then added in double.  The norm's
 * relative error against exact arithmetic is at most gamma(chain + 1) / 2 + 2u, u = 2^-24.
 * kgat_grad_sumsq_partials (kgat.py:32,162): the number of partials kgat_grad_sumsq_f32 writes for these sizes (one per
 * started chunk of 4,096 elements of each tensor); -1 on a bad argument.
 * kgat_grad_sumsq_f32 (kgat.py:32,162): ONE launch over up to kgat_adam_max_tensors() gradient tensors (HOST arrays of
 * sizes / device pointers, as kgat_adam_step_f32); partials[0 .. count) receive one fp32 sum of squares per chunk, in
 * tensor then chunk order.  partials_cap: floats available at `partials` (checked).  16-byte loads where a tensor's
 * pointer is 16-byte aligned, 4-byte loads otherwise - the same bits either way.  More tensors: one call per group,
 * each writing at its own offset of one buffer.
 * kgat_grad_norm_finish_f32 (kgat.py:32,162): ONE workgroup adds partials[0 .. n_partials) in double in a fixed order
 * and writes *norm and *coef (n_partials == 0: norm 0, coef 1).  max_norm finite and > 0.
 * kgat_adam_step_clipped_f32 (kgat.py:32,162): kgat_adam_step_f32 with every gradient element multiplied by the device
 * scalar *grad_coef first.  The stored gradient is READ, not rewritten: with zero_grads == 0 it keeps its unclipped
 * bits (torch's clip scales it in place), with zero_grads != 0 it is cleared.  *grad_coef == 1 gives the bits of
 * kgat_adam_step_f32.
 * kgat_scale_grads_f32 (kgat.py:32,162): ONE launch, g <- g * (*coef) in place over up to kgat_adam_max_tensors()
 * tensors: torch's in-place clip, for optimisers other than the fused one.
 * All: KGAT_E_BADARG on a null pointer, a negative size, more tensors than kgat_adam_max_tensors(), max_norm not finite
 * and > 0, before any device work. */
int kgat_grad_norm_chain(void);
int64_t kgat_grad_sumsq_partials(int n_tensors, const int64_t* sizes_host);
int kgat_grad_sumsq_f32(int n_tensors, const int64_t* sizes_host, float* const* grads_host, float* partials,
                        int64_t partials_cap, kgat_stream_t stream);
int kgat_grad_norm_finish_f32(int64_t n_partials, const float* partials, double max_norm, float* norm, float* coef,
                              kgat_stream_t stream);
int kgat_adam_step_clipped_f32(int n_tensors, const int64_t* sizes_host, float* const* params_host,
                               float* const* grads_host, float* const* exp_avg_host, float* const* exp_avg_sq_host,
                               const int64_t* steps_host, double lr, double beta1, double beta2, double eps,
                               int zero_grads, const float* grad_coef, kgat_stream_t stream);
int kgat_scale_grads_f32(int n_tensors, const int64_t* sizes_host, float* const* grads_host, const float* coef,
                         kgat_stream_t stream);

/* ---------------------------------------------------------------- BPR loss of the CF phase (8f #1)
 * reference models.py:170-178 (get_loss; _L2_loss_mean :9-11) on the readout `emb` (n_nodes rows of emb_stride
 * floats, the first F used; F and emb_stride multiples of 4):
 *   loss = -mean_b logsigmoid(<s_b,p_b> - <s_b,n_b>) + reg_lambda (mean_b |s_b|^2/2 + mean_b |p_b|^2/2 + mean_b |n_b|^2/2)
 * with s, p, n = rows u[b], p[b], n[b] (ids in [0, n_nodes); an id outside makes the loss NaN, nothing is accessed).
 * kgat_bpr_loss_f32: loss (1 float) and coef[batch] = sigmoid(-(x_b)) for the backward.
 * kgat_bpr_grad_f32: d loss / d emb as a DENSE n_nodes x F matrix (rows outside the batch zero - what torch's
 * index backward produces), times grad_scale[0] (DEVICE scalar = the gradient arriving at the loss; NULL = 1): rows
 * that occur several times are summed after a stable sort of the 3 x batch row ids: in sample order inside a window of
 * 32 sorted positions, a row that spans several windows as its window pieces in window order - a fixed order of
 * additions, no float atomics, bitwise reproducible, and bounded work per wavefront whatever the popularity of a row.
 * Same workspace size for both (it depends on F since ABI version 9: the windows' partial rows). */
size_t kgat_bpr_workspace_bytes(int64_t batch, int F);
int kgat_bpr_loss_f32(int64_t n_nodes, int F, const float* emb, int64_t emb_stride, int64_t batch, const int32_t* u,
                      const int32_t* p, const int32_t* n, float reg_lambda, float* loss, float* coef, void* workspace,
                      size_t workspace_bytes, kgat_stream_t stream);
int kgat_bpr_grad_f32(int64_t n_nodes, int F, const float* emb, int64_t emb_stride, int64_t batch, const int32_t* u,
                      const int32_t* p, const int32_t* n, const float* coef, float reg_lambda, const float* grad_scale,
                      float* grad, void* workspace, size_t workspace_bytes, kgat_stream_t stream);

/* ---------------------------------------------------------------- BPR-MF pretraining (ABI 16, additive)
 * The KGAT paper initialises its runs from BPR-MF embeddings: the loss of reference models.py:170-178 with the
 * embedding table itself as the readout, trained by the loop of reference kgat.py:150-168 (sample a batch, get_loss,
 * backward, optimizer.step, zero_grad).  Here that loop is a sequence of three-launch iterations without a dense
 * gradient, as the KG phase's (kgat_transr_presort_f32 / kgat_transr_adam_step_f32 above).
 *
 * kgat_mf_supported: F a multiple of 4 in [4, 256], 1 <= batch with 3 * batch <= 65536 (batch <= 21845),
 * 1 <= n_nodes < 2^31.  Other sizes: KGAT_E_UNSUPPORTED from both entries (the Python layer then runs
 * kgat_bpr_loss_f32 + kgat_bpr_grad_f32 + the optimiser per iteration).
 *
 * kgat_mf_presort_f32: the batches of a whole phase - u, p, n as n_batches x batch row-major arrays - sorted up front,
 * by ONE launch while 3 * batch <= 8192 (batch <= 2730: a workgroup per batch sorts in LDS), beyond it by three (the
 * slice sort and rank merge of kgat_bpr_grad_f32 over all batches, then the run lengths; at most 65,535 batches per
 * call): per batch the stable sort of its 3 x batch row ids taken role-major (i = role * batch + b; ids outside
 * [0, n_nodes) sort as n_nodes), i.e. the order kgat_bpr_grad_f32 sorts them into.  Batch b's result is the block of
 * kgat_mf_sorted_bytes(batch) bytes at sorted + b * that: sorted ids | order | run lengths (at the head of each run of
 * equal ids, 0 elsewhere), 3 x batch int32 each, 256-byte aligned (+ 8 x 3 x batch bytes of sort scratch beyond 8192 ids).
 *
 * kgat_mf_adam_step_f32: one iteration on batch arrays u, p, n (batch ids each) and that batch's `sorted` block: the
 * loss (1 float at `loss`) and the step of torch.optim.Adam on emb (n_nodes x F, contiguous), updated IN PLACE with
 * its moments exp_avg / exp_avg_sq (device pointers); `step` is the step count AFTER this step.  Dense semantics as
 * kgat_adam_step_f32 (every row of the table moves), without the n_nodes x F gradient and its zero fill.  Launches:
 * (1) the per-sample kernel of kgat_bpr_loss_f32; (2) the window kernel of kgat_bpr_grad_f32 writing into a compact
 * 3 x batch x F buffer - a run of equal ids completed inside its window of 32 sorted positions at the position of the
 * run's head, the pieces of a run that crosses window edges in the window's two partial slots -, beside it workgroups
 * that tag the batch's rows in `row_slot` (n_nodes 64-bit words owned by the caller - zero before the first call,
 * never to be cleared - a word is valid for the call whose `tag` it carries: pass a tag in [1, 2^47) that differs from
 * every earlier call's on the same row_slot) and the ordered loss reduction; (3) Adam over every row, g = 0 for an
 * untagged row, else the row's compact sum, or its pieces added in window order starting from the piece in the window
 * where the run begins.  The order of every addition is that of kgat_bpr_loss_f32 / kgat_bpr_grad_f32 (grad_scale
 * NULL) followed by kgat_adam_step_f32: the same bits, i.e. those of the reference's loss.backward();
 * optimizer.step().  emb, the moments, `sorted` and the workspace 16-byte aligned (else KGAT_E_BADARG). */
int kgat_mf_supported(int64_t n_nodes, int F, int64_t batch);
size_t kgat_mf_sorted_bytes(int64_t batch);
int kgat_mf_presort_f32(int64_t n_nodes, int64_t n_batches, int64_t batch, const int32_t* u, const int32_t* p,
                        const int32_t* n, void* sorted, size_t sorted_bytes, kgat_stream_t stream);
size_t kgat_mf_step_workspace_bytes(int64_t batch, int F);
int kgat_mf_adam_step_f32(int64_t n_nodes, int F, int64_t batch, const int32_t* u, const int32_t* p, const int32_t* n,
                          const void* sorted, float* emb, float* exp_avg, float* exp_avg_sq, int64_t step, double lr,
                          double beta1, double beta2, double eps, float reg_lambda, float* loss, uint64_t* row_slot,
                          uint64_t tag, void* workspace, size_t workspace_bytes, kgat_stream_t stream);

/* ---------------------------------------------------------------- TransR link prediction (ABI 16, additive)
 * The filtered rank of a triple's true tail (head) among the entities under the score of reference models.py:120-126,
 * |u_h + u_r - u_t|^2 with the normalisation of the training kernel (u = a / max(|a|, 1e-12), a = e W_r).
 *
 * kgat_transr_project_f32: for i in [0, n_rows), with e_i = ent row (ids ? ids[i] : row0 + i) of n_ent x d floats,
 *     a_i = e_i W_r (W_r: d x k row-major),  u_i = a_i / max(|a_i|, 1e-12),
 *     out[i, :] = u_i + sign * rel_row / max(|rel_row|, 1e-12)      (rel_row NULL: out[i, :] = u_i)
 *     n2[i]     = |u_i|^2  (fp32; 1 up to rounding, exactly 0 for a zero a_i; n2 NULL: not written)
 * out is ROW-MAJOR n_rows x k: the layout kgat_transr_rank_f32 and kgat_eval_topk_f32 read.  sign is +1 or -1
 * (else KGAT_E_BADARG).  fp32 MFMA (v_mfma_f32_16x16x4_f32), W_r staged once per workgroup in LDS.  Widths
 * (kgat_transr_project_supported): d, k in {16, 32, 64, 128} independently, others KGAT_E_UNSUPPORTED.  ent, W_r and
 * out 16-byte aligned.  Without ids the range [row0, row0 + n_rows) must lie inside [0, n_ent) (KGAT_E_BADARG); with
 * ids the caller guarantees ids[i] in [0, n_ent) (the kernel clamps: a bad id reads a wrong row, never outside ent).
 *
 * kgat_transr_rank_f32: n_q query rows q (row-major, k columns) with the entity id t[j] of their true answer;
 * candidates p (n_c x k row-major) with n2[n_c]: the entities [c0, c0 + n_c); a filter in CSR form - query j leaves out
 * the entity ids filter_ids[filter_ptr[j] .. filter_ptr[j + 1]) (ascending; any int32 id is allowed, those
 * outside the candidate range are ignored; n_filter = length of filter_ids) and always its true answer.  With s_i = n2_i - 2 q_j . p_i:
 *     lt[j] = #{ i not left out : s_i <  s_t }        eq[j] = #{ i not left out : s_i == s_t }
 * (int32; the entry zeroes them).  s_t is formed by the same tile routine as every s_i, so a candidate whose row and
 * n2 are bit-identical to the true answer's counts in eq wherever it lies.  Candidate segments run in different
 * workgroups and add integer counts with integer atomics: exact, bitwise reproducible; no workspace.  k in
 * {16, 32, 64, 128} (kgat_transr_rank_supported), others KGAT_E_UNSUPPORTED; n_q, n_c >= 1, c0 >= 0, c0 + n_c below
 * 2^31, q, p, n2 16-byte aligned, no null pointer (filter_ids may be NULL with n_filter = 0): else KGAT_E_BADARG.
 * What only the device can see - t[j] inside [c0, c0 + n_c), filter lists ascending, filter_ptr non-decreasing within
 * [0, n_filter] - is the caller's to guarantee (the Python layer checks it); the kernel clamps every index it derives
 * from them, so a violation gives wrong counts and never an access outside the buffers. */
int kgat_transr_project_supported(int d, int k);
int kgat_transr_project_f32(int64_t n_rows, int64_t n_ent, int d, int k, const float* ent, const int32_t* ids,
                            int64_t row0, const float* W_r, const float* rel_row, float sign, float* out, float* n2,
                            kgat_stream_t stream);
int kgat_transr_rank_supported(int k);
int kgat_transr_rank_f32(int64_t n_q, int64_t n_c, int64_t c0, int k, const float* q, const int32_t* t, const float* p,
                         const float* n2, const int32_t* filter_ptr, const int32_t* filter_ids, int64_t n_filter,
                         int32_t* lt, int32_t* eq, kgat_stream_t stream);

/* ---------------------------------------------------------------- multi-head graph attention (additive within ABI 16)
 * The aggregation of dgl.nn.pytorch.conv.GATConv (DGL 0.4.x, homogeneous graph) and its backward: what
 *   graph.apply_edges(fn.u_add_v('el', 'er', 'e')); e = leaky_relu(e); a = edge_softmax(graph, e)
 *   graph.update_all(fn.u_mul_e('ft', 'a', 'm'), fn.sum('m', 'ft'))              (a = attn_drop(a) in between)
 * computes, in one walk over the destination-major CSR with no edge-sized tensor.  ft [N x H x F], el, er [N x H]:
 *   z[e,h] = el[src e, h] + er[dst e, h];  s = z > 0 ? z : negative_slope z;  m[v,h] = max_{e -> v} s;
 *   p = exp(s - m[dst e, h]);  l[v,h] = sum_{e -> v} p  (dropped edges included, as DGL);
 *   out[v,h,:] = (sum_{e -> v} c[e,h] p ft[src e, h, :]) / l[v,h]   - one correctly rounded division per element;
 * c[e,h] = 0 or 1 / (1 - drop_p): edge e, head h is kept iff the counter hash of the training entries over element
 * (row = edge id, d = H, col = h) says so (ops.dropout_keep_mask(seed, E, H, drop_p)[e, h]); eid maps CSR position ->
 * edge id and is required with drop_p > 0.  Rows without in-edges: out = 0, l = 0.  m, l [N x H] are outputs of the
 * forward and inputs of the backward.  m is formed without a rescale: leaky_relu (0 <= negative_slope <= 1) and the
 * fp32 add are monotone, so m = leaky_relu(max_u el[u,h] + er[v,h]) - kgat_spmm_umule_max_f32 on el, then one pass.
 *
 * kgat_gat_bwd_f32: with sg[v,h] = <g_out[v,h,:], out[v,h,:]>, gamma = <g_out[v,h,:], ft[u,h,:]>, a = p / l,
 *   g_z = a (c gamma - sg[v,h]) (z > 0 ? 1 : negative_slope)
 *   g_er[v,h] = sum_{e -> v} g_z;   g_el[u,h] = sum_{u -> e} g_z;   g_ft[u,h,:] = sum_{u -> e} c a g_out[dst e, h, :]
 * one walk over the forward CSR (g_er) and one over the reversed CSR (rev_*: rows = sources, col = destinations,
 * rev_eid the edge ids; g_ft, g_el), each recomputing a from m and l; nothing edge-sized is stored.
 *
 * All walks use the sum kernel's tile decomposition with partials combined in run and tile order: no atomics, bitwise
 * reproducible.  (H, F) with H F in {16, 32, 64, 128} and F % 4 == 0 (kgat_gat_supported), others KGAT_E_UNSUPPORTED.
 * The whole graph per call: indptr [N + 1], col / row_of / eid [E].  ft, out, g_out, g_ft, el, m and the workspace
 * 16-byte aligned; n_edges * H < 2^32.  Null pointer, negative size, slope or probability out of range:
 * KGAT_E_BADARG; workspace below kgat_gat_workspace_bytes(n_nodes, n_edges, H, F, backward = 0 | 1): KGAT_E_WORKSPACE.
 * Every check precedes any device work. */
int kgat_gat_supported(int H, int F);
size_t kgat_gat_workspace_bytes(int64_t n_nodes, int64_t n_edges, int H, int F, int backward);
int kgat_gat_fwd_f32(int64_t n_nodes, int64_t n_edges, int H, int F, const int32_t* indptr, const int32_t* col,
                     const int32_t* row_of, const int32_t* eid, const float* ft, const float* el, const float* er,
                     float negative_slope, float drop_p, uint64_t seed, float* out, float* m, float* l, void* workspace,
                     size_t workspace_bytes, kgat_stream_t stream);
int kgat_gat_bwd_f32(int64_t n_nodes, int64_t n_edges, int H, int F, const int32_t* indptr, const int32_t* col,
                     const int32_t* row_of, const int32_t* eid, const int32_t* rev_indptr, const int32_t* rev_col,
                     const int32_t* rev_row_of, const int32_t* rev_eid, const float* ft, const float* el, const float* er,
                     const float* m, const float* l, const float* out, const float* g_out, float negative_slope,
                     float drop_p, uint64_t seed, float* g_ft, float* g_el, float* g_er, void* workspace,
                     size_t workspace_bytes, kgat_stream_t stream);

/* ---------------------------------------------------------------- relational graph convolution (additive within ABI 16)
 * The sparse part of dgl.nn.pytorch.conv.RelGraphConv (DGL 0.4.x, regularizer "basis"), aggregate-first.  With
 * W_r = sum_b a[r,b] weight[b] the layer's  h[v] = sum_{e: u->v} norm[e] (x[u] W_{etype e})  is
 *   Z[v,b,:] = sum_{e: u->v} (norm[e] a[etype[e], b]) x[u,:]                                   kgat_rgcn_fwd_f32
 * followed by the caller's GEMM  h = Z.view(N, B D) weight.view(B D, out): a source row (D floats, not B out) is
 * gathered once per edge and feeds B accumulators.  x [N x D], Z and g_Z [N x B x D], a and g_a [R x B] (w_comp, or the
 * R x R identity when B == R), etype int32 and norm float (may be NULL: 1) per edge in the order of the CSR walked.
 *   g_x[u,:] = sum_{u->e} sum_b (norm[e] a[etype[e], b]) g_Z[dst e, b, :]                       kgat_rgcn_bwd_x_f32
 * over the reversed CSR (rows = sources, rev_col = destinations, etype_rev / norm_rev in its order), and
 *   g_a[r,b] = sum_{e: etype[e] = r} norm[e] <x[src e,:], g_Z[dst e, b, :]>                     kgat_rgcn_bwd_coef_f32
 * over the forward CSR.  An edge whose type is outside [0, R) contributes nothing.  Rows without edges: 0.
 *
 * All walks use the sum kernel's tile decomposition with partials combined in run and tile order (bwd_coef: per
 * wavefront tables in LDS added in edge order, then in wavefront, workgroup and chunk order): no atomics, bitwise
 * reproducible; nothing of size E x D or E x B is written.  D in {16, 32, 64, 128}, 1 <= B <= 8, R B <= 4096
 * (kgat_rgcn_supported), others KGAT_E_UNSUPPORTED.  The whole graph per call: indptr [N + 1], col / row_of / etype /
 * norm [E].  x, Z, g_Z, g_x and the scratch 16-byte aligned.  Null pointer, negative size: KGAT_E_BADARG; scratch below
 * kgat_rgcn_scratch_bytes(n_nodes, n_edges, D, B, R, pass = 0 fwd | 1 bwd_x | 2 bwd_coef): KGAT_E_WORKSPACE.  The tiles'
 * partials live inside the scratch.  Every check precedes any device work. */
int kgat_rgcn_supported(int D, int B, int R);
size_t kgat_rgcn_scratch_bytes(int64_t n_nodes, int64_t n_edges, int D, int B, int R, int pass);
int kgat_rgcn_fwd_f32(int64_t n_nodes, int64_t n_edges, int D, int B, int R, const int32_t* indptr, const int32_t* col,
                      const int32_t* row_of, const int32_t* etype_csr, const float* norm_csr, const float* x,
                      const float* a, float* Z, void* scratch, size_t scratch_bytes, kgat_stream_t stream);
int kgat_rgcn_bwd_x_f32(int64_t n_nodes, int64_t n_edges, int D, int B, int R, const int32_t* rev_indptr,
                        const int32_t* rev_col, const int32_t* rev_row_of, const int32_t* etype_rev,
                        const float* norm_rev, const float* g_Z, const float* a, float* g_x, void* scratch,
                        size_t scratch_bytes, kgat_stream_t stream);
int kgat_rgcn_bwd_coef_f32(int64_t n_nodes, int64_t n_edges, int D, int B, int R, const int32_t* indptr,
                           const int32_t* col, const int32_t* row_of, const int32_t* etype_csr, const float* norm_csr,
                           const float* x, const float* g_Z, float* g_a, void* scratch, size_t scratch_bytes,
                           kgat_stream_t stream);

/* ---------------------------------------------------------------- TransE KG embedding: the CFKG baseline (additive within ABI 16)
 * The KGAT paper's CFKG baseline trains a translation model over the collaborative KG.  Its objective here is the
 * reference's `transR` (models.py:114-133, with _L2_loss_mean :9-11) with the projection removed: for a batch
 * (h, r, pos_t, neg_t) with ent (n_nodes x d) and rel (n_rel x d), both contiguous,
 *     u_x = ent[x] / max(|ent[x]|, 1e-12)  (x in h, pos_t, neg_t),   u_r = rel[r] / max(|rel[r]|, 1e-12)
 *     loss = mean_b softplus(|u_h + u_r - u_p|^2 - |u_h + u_r - u_n|^2) + reg_lambda * sum_{v in h,r,p,n} mean_b |u_v|^2 / 2
 * i.e. models.py:114-133 with every W_R[r] = I and d = k.  The gradient goes through the normalisation as autograd's
 * does (F.normalize: a row whose norm is below the clamp gets g / 1e-12).  A sample with an id outside its table reads
 * nothing, makes the loss NaN and contributes no gradient.
 *
 * kgat_transe_supported: d a multiple of 4 in [4, 256], 1 <= batch <= 2730 (3 * batch ids sorted by one workgroup in
 * LDS), 1 <= n_rel <= 4096, 1 <= n_nodes < 2^31.  Other sizes: KGAT_E_UNSUPPORTED from every entry below (the Python
 * layer then runs the torch restatement).
 *
 * kgat_transe_forward_f32 / kgat_transe_backward_f32: the two halves autograd needs (models.py:114-133 under
 * loss.backward()).  The forward sorts the batch (samples by relation, the 3 x batch entity ids), runs the per-sample
 * kernel - d / 4 lanes per sample, 16 bytes per lane and row; the relation's gradient row written at the sample's
 * relation-sorted position, the three entity rows at the sorted positions of their ids - and the chunk sums of the
 * relation rows (at most 64 sorted samples each), and reduces the loss (1 float at `loss`); everything the backward
 * needs stays in `scratch`, which the caller hands to the backward unchanged with the same ids.  The backward writes
 * grad_ent (n_nodes x d, dense: rows outside the batch zero) and grad_rel (n_rel x d, dense), times grad_scale[0] (a
 * DEVICE scalar; NULL: 1).  kgat_transe_loss_grad_f32: both in one call, the same bits.
 *
 * kgat_transe_presort_f32: the sorts of a whole phase's batches - h, r, pos_t, neg_t as n_batches x batch row-major
 * arrays - in ONE launch; batch b's result is the block of kgat_transe_sorted_bytes(batch, n_rel) bytes at sorted + b
 * * that (the block of kgat_transr_presort_f32, which does the work).
 *
 * kgat_transe_adam_step_f32: one iteration (reference kgat.py:116-136: loss -> backward -> optimizer.step -> zero_grad)
 * on batch arrays h .. neg_t and that batch's `sorted` block: the loss and the step of torch.optim.Adam on ent and rel,
 * IN PLACE with their moments (`exp_avg_host`, `exp_avg_sq_host`: HOST arrays of two device pointers, entity table
 * first; `steps_host`: the two step counts AFTER this step).  Dense semantics (every row moves), without a dense
 * gradient: launch one is the per-sample kernel, beside it workgroups that tag the batch's entities in `row_slot`
 * (n_nodes 64-bit words owned by the caller - zero before the first call, never to be cleared - a word is valid for
 * the call whose `tag` it carries: pass a tag in [1, 2^50) that differs from every earlier call's on the same
 * row_slot); launch two the chunk sums + the loss; launch three Adam, with g = 0 for an untagged entity row, else the
 * sum of the row's run, and for a relation row the sum of its chunk rows.
 *
 * Fixed summation orders, the same in every entry: a run of equal entity ids in sorted order from 0; the samples of a
 * relation in sorted order within a chunk from 0, then the chunks in order from 0; the loss as 256 strided sums and a
 * tree over them.  No float atomics: bitwise reproducible, and the fused iteration has the bits of
 * kgat_transe_loss_grad_f32 followed by kgat_adam_step_f32, i.e. of loss.backward(); optimizer.step().
 *
 * All entries: ent, rel, the gradients, the moments, `sorted` and `scratch` 16-byte aligned, null pointer, bad
 * hyperparameter or tag: KGAT_E_BADARG; scratch below kgat_transe_scratch_bytes(batch, d, n_rel) - one size for all of
 * them - or `sorted_bytes` below n_batches blocks: KGAT_E_WORKSPACE.  Every check precedes any device work. */
int kgat_transe_supported(int64_t n_nodes, int d, int n_rel, int64_t batch);
size_t kgat_transe_scratch_bytes(int64_t batch, int d, int n_rel);
size_t kgat_transe_sorted_bytes(int64_t batch, int n_rel);
int kgat_transe_forward_f32(int64_t n_nodes, int n_rel, int d, int64_t batch, const int32_t* h, const int32_t* r,
                            const int32_t* pos_t, const int32_t* neg_t, const float* ent, const float* rel,
                            float reg_lambda, float* loss, void* scratch, size_t scratch_bytes, kgat_stream_t stream);
int kgat_transe_backward_f32(int64_t n_nodes, int n_rel, int d, int64_t batch, const int32_t* h, const int32_t* r,
                             const int32_t* pos_t, const int32_t* neg_t, const float* grad_scale, float* grad_ent,
                             float* grad_rel, void* scratch, size_t scratch_bytes, kgat_stream_t stream);
int kgat_transe_loss_grad_f32(int64_t n_nodes, int n_rel, int d, int64_t batch, const int32_t* h, const int32_t* r,
                              const int32_t* pos_t, const int32_t* neg_t, const float* ent, const float* rel,
                              float reg_lambda, float* loss, float* grad_ent, float* grad_rel, void* scratch,
                              size_t scratch_bytes, kgat_stream_t stream);
int kgat_transe_presort_f32(int64_t n_nodes, int n_rel, int64_t n_batches, int64_t batch, const int32_t* h,
                            const int32_t* r, const int32_t* pos_t, const int32_t* neg_t, void* sorted,
                            size_t sorted_bytes, kgat_stream_t stream);
int kgat_transe_adam_step_f32(int64_t n_nodes, int n_rel, int d, int64_t batch, const int32_t* h, const int32_t* r,
                              const int32_t* pos_t, const int32_t* neg_t, const void* sorted, float* ent, float* rel,
                              float* const* exp_avg_host, float* const* exp_avg_sq_host, const int64_t* steps_host,
                              double lr, double beta1, double beta2, double eps, float reg_lambda, float* loss,
                              uint64_t* row_slot, uint64_t tag, void* scratch, size_t scratch_bytes, kgat_stream_t stream);

/* ---------------------------------------------------------------- Bi-Interaction pooling: the FM / NFM baselines (additive within ABI 16)
 * The KGAT paper's FM and NFM baselines pool the embeddings of a sparse feature set - a user, an item and the
 * entities connected to it.  Feature lists are a CSR over item positions: ids[indptr[j] : indptr[j + 1]] are rows of
 * V (n_nodes x d, contiguous); lists are multisets (a repeated id counts twice).  Pooled set m is
 *     [extra[m]] (left out where extra[m] < 0 or extra is NULL)  +  the list of item position items[m],
 * n positions with the extra first, and
 *     S[m] = sum_f v_f    bi[m] = (S[m]^2 - sum_f v_f^2) / 2    lin[m] = sum_f w_lin[f]    sq[m] = sum_f |v_f|^2
 * (an empty set: zeros).  The two entries replace index_select / index_add_ under autograd (float atomics, tensors of
 * pairs x d) and a full-graph kgat_copy_reduce_f32 of [V | V^2] over every item's list.
 *
 * kgat_bi_pool_fwd_f32: one wavefront per set, d / 4 lanes per row and 16 bytes per lane, G = 256 / d lane groups,
 * four rows in flight per group.  Order of additions: position p belongs to group p mod G; a group adds its rows in
 * ascending position from 0 (v^2 through one fused multiply-add each); the G partials are combined by a butterfly
 * (group g with g ^ G/2, then g ^ G/4, ..., g ^ 1); bi = 0.5 * fma(S, S, -sum v^2); sq is the sum of the d column sums
 * of v^2, ((x + y) + (z + w)) per lane, then a butterfly over the d / 4 lanes.  w_lin, extra, lin, sq may be NULL.  A
 * set whose item position or one of whose ids lies outside its table gets NaN outputs.  Nothing of size pairs x d is
 * written.
 *
 * kgat_bi_pool_bwd_f32: the DENSE gradients grad_V (n_nodes x d) and grad_w (n_nodes; may be NULL) from g_bi (n_sets
 * x d), g_lin, g_sq (n_sets each; each of the three may be NULL: zero) and the forward's S:
 *     grad_V[f] = sum over the occurrences of f in the sets m of  g_bi[m] * (S[m] - v_f) + 2 g_sq[m] v_f
 *     grad_w[f] = sum over the same occurrences of g_lin[m]
 * Every row is written exactly once, rows no set touches are 0.  rev_indptr (n_nodes + 1) / rev_items is the reversed
 * CSR: the item positions that hold feature f, ascending, once per occurrence.  The entry sorts `items` and `extra`
 * (stable, one workgroup each) into runs of sets per item / per extra id, whose first positions go into two tables in
 * the scratch that a memset refills first; then one wavefront per row f walks f's run as an extra followed by its
 * reversed list, numbers the hits in that order (within a run in ascending m), gives hit h to lane group h mod G,
 * which adds its terms in ascending h from 0, and combines the groups with the butterfly above.  A row with more than
 * 256 sources (a feature that most items carry) is left to a second launch - its id goes through an integer counter
 * into a list whose order reaches no sum - where 16 wavefronts share it: look k (64 sources) belongs to wavefront
 * k mod 16, each wavefront numbers and adds its own hits as above, and the 16 sums are added in wavefront order from 0.
 * No float atomics: both entries are bitwise reproducible.
 *
 * kgat_bi_pool_supported(d, n_sets): d in {16, 32, 64, 128} and 1 <= n_sets <= 8192 (the sets one workgroup sorts in
 * LDS); others KGAT_E_UNSUPPORTED from both entries (the Python layer then runs the torch restatement).  n_nodes,
 * n_items in [1, 2^31), n_pairs in [0, 2^31), no negative size, no null pointer other than the optional ones, V, S,
 * bi, g_bi, grad_V and the scratch 16-byte aligned: else KGAT_E_BADARG.  Scratch below
 * kgat_bi_pool_scratch_bytes(n_sets, n_items, n_nodes, n_pairs): KGAT_E_WORKSPACE.  Every check precedes any device work. */
int kgat_bi_pool_supported(int d, int64_t n_sets);
size_t kgat_bi_pool_scratch_bytes(int64_t n_sets, int64_t n_items, int64_t n_nodes, int64_t n_pairs);
int kgat_bi_pool_fwd_f32(int64_t n_sets, int d, int64_t n_nodes, int64_t n_items, int64_t n_pairs, const float* V,
                         const float* w_lin, const int32_t* indptr, const int32_t* ids, const int32_t* items,
                         const int32_t* extra, float* S, float* bi, float* lin, float* sq, kgat_stream_t stream);
int kgat_bi_pool_bwd_f32(int64_t n_sets, int d, int64_t n_nodes, int64_t n_items, int64_t n_pairs, const float* V,
                         const int32_t* rev_indptr, const int32_t* rev_items, const int32_t* items, const int32_t* extra,
                         const float* g_bi, const float* g_lin, const float* g_sq, const float* S, float* grad_V,
                         float* grad_w, void* scratch, size_t scratch_bytes, kgat_stream_t stream);

/* ---------------------------------------------------------------- ripple-set attention: the RippleNet baseline (additive within ABI 16)
 * RippleNet (Wang et al., CIKM 2018), the KGAT paper's path-based baseline, attends with one item vector over a user's
 * ripple set of every hop: n_memory triples (h_i, r_i, t_i) of the knowledge graph.  The sets are graph-static int32
 * arrays mem_h, mem_r, mem_t of shape [n_users, n_hop, n_memory]; inside every (user, hop) the triples are sorted
 * ascending by (r, h, t), so equal relations are consecutive - the backward relies on it.  For sample b with user
 * users[b], hop `hop` and the query table U (n_samples x n_rel x d, contiguous; U[b, r] = v_b R_r, a matmul of the caller):
 *     s_i = <U[b, r_i], ent[h_i]>      p[b] = softmax_i(s) (maximum subtracted)      o[b] = sum_i p_i ent[t_i]
 * and, given g_o (n_samples x d):
 *     gp_i = <ent[t_i], g_o[b]>        gl[b, i] = p_i (gp_i - sum_j p_j gp_j)
 *     grad_U[b, r] = sum_{i : r_i = r} gl_i ent[h_i]      (+0.0 rows for the relations the set lacks)
 * The gradient towards ent - grad_ent[t_i] += p_i g_o[b], grad_ent[h_i] += gl_i U[b, r_i] - is two incidence lists the
 * caller sums with kgat_csr_from_coo + kgat_spmm_umule_sum_f32; no entry here forms it.
 *
 * Both entries: one wavefront per sample, d / 4 lanes per row and 16 bytes per lane, G = 256 / d lane groups, four rows
 * in flight per group; nothing of size n_samples x n_memory x d is written.
 * kgat_ripple_hop_fwd_f32 writes o (n_samples x d) and p (n_samples x n_memory).  Order of additions: slot i belongs to
 * group i mod G.  A logit is, per lane, fma(x3, q3, fma(x2, q2, fma(x1, q1, x0 * q0))) over its four columns, then a
 * butterfly over the d / 4 lanes of the group (strides d / 8, ..., 1).  Softmax: lane j of the wavefront holds slots j and
 * j + 64, adds e_j + e_{j + 64}, and a butterfly over the 64 lanes (strides 32, ..., 1) gives the sum; p = e / sum.  o: a
 * group adds p_i * ent[t_i], one fma per column, in ascending i from 0; the G partials are combined by a butterfly
 * (group g with g ^ G/2, then g ^ G/4, ..., g ^ 1).  The first four tail rows of every group are requested before the
 * softmax's reductions.
 * kgat_ripple_hop_bwd_f32 writes gl (n_samples x n_memory) and EVERY row of grad_U (n_samples x n_rel x d) exactly
 * once - no memset.  gp as the logits above; lane j forms fma(p_{j + 64}, gp_{j + 64}, p_j * gp_j) and the 64-lane
 * butterfly gives sum_j p_j gp_j.  Relation r belongs to group r mod G, which finds r's run of slots (two binary
 * searches) and adds gl_i * ent[h_i], one fma per column, in ascending i from the run's first slot; groups are not
 * combined.  U is part of the argument list (it is checked) and is not read.
 * No float atomics: both entries are bitwise reproducible.  A sample whose user id lies outside [0, n_users), or whose
 * set holds an id outside [0, n_nodes) / [0, n_rel), reads nothing there and gets NaN outputs.
 *
 * kgat_ripple_supported(d, n_memory, n_rel, n_samples): d in {16, 32, 64, 128}, 1 <= n_memory <= 128, 1 <= n_rel <=
 * 4096, 1 <= n_samples with (n_samples + 3) / 4 workgroups inside the grid; others KGAT_E_UNSUPPORTED from both entries
 * (the Python layer then runs the torch restatement).  Negative size, n_hop < 1, hop outside [0, n_hop), n_nodes or
 * n_users outside [1, 2^31), a null pointer, ent / U / o / g_o / grad_U not 16-byte aligned: KGAT_E_BADARG.  Every
 * check precedes any device work. */
int kgat_ripple_supported(int d, int n_memory, int n_rel, int64_t n_samples);
int kgat_ripple_hop_fwd_f32(int64_t n_samples, int d, int n_memory, int n_rel, int n_hop, int hop, int64_t n_nodes,
                            int64_t n_users, const float* ent, const float* U, const int32_t* mem_h, const int32_t* mem_r,
                            const int32_t* mem_t, const int32_t* users, float* o, float* p, kgat_stream_t stream);
int kgat_ripple_hop_bwd_f32(int64_t n_samples, int d, int n_memory, int n_rel, int n_hop, int hop, int64_t n_nodes,
                            int64_t n_users, const float* ent, const float* U, const int32_t* mem_h, const int32_t* mem_r,
                            const int32_t* mem_t, const int32_t* users, const float* p, const float* g_o, float* grad_U,
                            float* gl, kgat_stream_t stream);

/* ---------------------------------------------------------------- all-pairs NFM evaluation: MLP scores into top-K (additive within ABI 16)
 * The K best unseen items of every user under a one-hidden-layer NFM, y(u, i) = w0 + w_lin[u] + lin_i + sum_j h_j
 * relu(pre[u, i, j]), without a users x items tensor.  With (P, T, lin) the pooled item side (bi({u} + F(i)) = v_u * P_i +
 * T_i) the caller passes itemT = kgat_eval_items_kmajor_f32(emb = P, F = d, item_ids = 0 .. n_items - 1), C = T W1^T +
 * b1 (n_items x hidden, row-major, contiguous), W1 (hidden x d, row-major, contiguous), h (hidden), item_lin (n_items),
 * V with row stride v_stride (user_ids are rows of V), the users' ascending training lists as a CSR over positions in
 * user_ids (train_ptr: n_users + 1) of item positions, and optionally user_const (n_users; w0 + w_lin[u]).
 *
 * The arithmetic, to the operation order (all fp32, inputs finite):
 *     a[j, c]  = fl(W1[j, c] * V[user, c])                                             one multiply
 *     pre[j]   = fma(a[j, d-1], P_i[d-1], ... fma(a[j, 1], P_i[1], fma(a[j, 0], P_i[0], C_i[j])))   ascending c from C
 *                (v_mfma_f32_32x32x2_f32: an exact fmaf chain in k order)
 *     r[j]     = max(pre[j], 0)
 *     s_i      = A + B, where hidden unit j = 32 b + 8 q + 4 m + e (e < 4, m < 2, q < 4, b < hidden / 32) belongs to
 *                half m, A (m = 0) and B (m = 1) each start from 0 and add their units by p = fma(h_j, r[j], p) in
 *                ascending (b, q, e)
 *     key_i    = s_i + item_lin[i]
 *     score    = key_i + user_const[u]   (key_i itself where user_const is NULL), formed once per listed item
 * Items are ordered by (key descending, IEEE compare with -0 = +0; equal keys: ascending item position); training
 * items are never listed; a user with fewer than K unseen items gets -1 / -inf at the end of topk_items /
 * topk_scores (n_users x K each; topk_scores may be NULL).  The order is total and no float atomic is used: the lists
 * are bitwise reproducible and independent of how the entry cuts the items into segments, of the other users of the
 * call, and of K as far as the shorter list reaches.  A user id may repeat.
 *
 * The entry lays C out in the scratch (a lane's sixteen accumulator values as 16-byte loads), sweeps one user per
 * wavefront over item tiles of 32 (one 16-byte fragment load feeds 4 x hidden / 32 MFMAs), keeps per user a candidate
 * buffer of 256 entries in LDS that a selection prunes to K, and merges the segments' lists with one wavefront per user.
 *
 * kgat_nfm_eval_supported(d, hidden, K): d in {16, 32, 64, 128}, hidden in {32, 64}, 1 <= K <= 128.  hidden = 16 is served
 * by the caller padding W1's rows, C's columns and h with zeros to 32 (exact: 0 * relu(0) = 0); hidden = 128 and deeper
 * MLPs are not offered.  n_users < 0, n_items outside [1, 2^31 - 32), v_stride < d, a null pointer other than
 * user_const / topk_scores / train_items (no training item at all), itemT or scratch not 16-byte aligned: KGAT_E_BADARG; outside the envelope:
 * KGAT_E_UNSUPPORTED; scratch below kgat_nfm_eval_scratch_bytes(n_users, n_items, d, hidden, K): KGAT_E_WORKSPACE.
 * Every check precedes any device work. */
int kgat_nfm_eval_supported(int d, int hidden, int K);
size_t kgat_nfm_eval_scratch_bytes(int64_t n_users, int64_t n_items, int d, int hidden, int K);
int kgat_nfm_eval_topk_f32(int64_t n_users, const int32_t* user_ids, int64_t n_items, int d, int hidden, const float* V,
                           int64_t v_stride, const float* W1, const float* itemT, const float* C, const float* h,
                           const float* item_lin, const float* user_const, const int32_t* train_ptr,
                           const int32_t* train_items, int K, void* scratch, size_t scratch_bytes, int32_t* topk_items,
                           float* topk_scores, kgat_stream_t stream);

/* ---------------------------------------------------------------- all-pairs RippleNet evaluation: attention scores into top-K (additive within ABI 16)
 * The K best unseen items of every user under RippleNet, without a users x items tensor.  For the user's hop k
 * (0-based, n_hop hops of n_memory = M triples (h_i, r_i, t_i) each; mem_h / mem_r / mem_t: n_users x n_hop x M, int32,
 * the relations of a set ascending) and an item with row v_0 = ent[item]:
 *     key[k, i, :] = R_{r_i} ent[h_i]                  R_r = relation_emb[r] as a d x d row-major matrix
 *     s_i = <v_k, key[k, i]>    p = softmax_i(s)    o_k = sum_i p_i ent[t_i]
 *     v_{k+1} = o_k | v_k + o_k | W o_k | W (v_k + o_k)        mode 0..3; (W x)[a] = sum_c W[a, c] x[c], W d x d row-major
 *     y = <v_H, o_{H-1}>   or   <v_H, sum_k o_k>               (all_hops != 0)
 *
 * kgat_eval_ripple_keys_f32 writes keys (n_call x n_hop x M x d, contiguous) for the users user_ids[0 .. n_call):
 *     key[a] = fma(R[a, d-1], h[d-1], ... fma(R[a, 1], h[1], fma(R[a, 0], h[0], 0)))      ascending c from 0, all fp32
 * A user id outside [0, n_users) reads nothing and gets zeros; a set entry outside [0, n_nodes) / [0, n_rel) reads
 * nothing and gets NaN.
 *
 * kgat_eval_ripple_topk_f32 takes itemT = kgat_eval_items_kmajor_f32(emb = the ranked item rows, F = d, item_ids =
 * 0 .. n_items - 1), the key table of the SAME user_ids, ent (n_nodes x d, contiguous) and mem_t for the tail rows, W
 * (may be NULL for modes 0 and 1), and the users' ascending training lists as a CSR over positions in user_ids
 * (train_ptr: n_call + 1) of item positions.  The arithmetic, to the operation order (all fp32, inputs finite), per
 * (user, item); every sum over an index below is a chain of v_mfma_f32_32x32x2_f32 steps in ascending index order
 * from 0 (an exact fmaf chain in k order, as in the NFM block above):
 *     s_i   = sum_c key[k, i, c] v_k[c]                                   c ascending from 0, start 0
 *     mx    = max_i s_i                                                   over the M slots (exact)
 *     e_i   = exp(s_i - mx)                                               the fast exponential (v_exp_f32 of x log2 e)
 *     sum   = A + B, A over the even slots and B over the odd slots, each from 0 in ascending slot order, one add each
 *     p_i   = e_i * fl(1 / sum)
 *     o_k[c] = sum_i ent[t_i][c] p_i                                      i ascending from 0, start 0
 *     x     = o_k (modes 0, 2), fl(v_k + o_k) (modes 1, 3);  v_{k+1} = x (modes 0, 1), sum_c W[a, c] x[c] (modes 2, 3)
 *     z     = o_{H-1}, or with all_hops fl(.. fl(fl(0 + o_0) + o_1) ..)
 *     y     = A + B, A over the even columns and B over the odd columns, each p = fma(v_H[c], z[c], p) from 0 ascending
 * Slots are padded to a multiple of 32 inside the kernel; a padded slot is masked by its index and has e = 0 exactly.
 * Items are ordered by (y descending, IEEE compare with -0 = +0; equal y: ascending item position); training items
 * are never listed; a user with fewer than K unseen items gets -1 / -inf at the end of topk_items / topk_scores
 * (n_call x K each; topk_scores may be NULL).  The order is total and no float atomic is used: the lists are bitwise
 * reproducible and independent of how the entry cuts the items into segments, of the other users of the call, and of
 * K as far as the shorter list reaches.  A user id may repeat; one outside [0, n_users) gets an empty list.
 *
 * The entry runs one workgroup per (user, item segment): the user's keys, tail rows and W are laid out in LDS as MFMA
 * A operands once, four wavefronts split the segment's item tiles of 32, every product has the item on the lane and
 * takes the previous accumulator registers as its B operand; each wavefront keeps a candidate buffer of 256 entries
 * that a selection prunes to K, and one wavefront per user merges the lists.
 *
 * kgat_eval_ripple_supported(d, n_memory, n_hop, mode, K): d in {16, 32, 64}, 1 <= n_memory <= 64, n_hop in {1, 2}, mode
 * 0..3, 1 <= K <= 128 (d = 128, longer sets and deeper hops are not offered).  n_call < 0, n_items outside [1, 2^31 -
 * 32), n_nodes / n_users outside [1, 2^31), n_rel < 1, a null pointer other than topk_scores / train_items (no training
 * item at all) / W (modes 0, 1), ent / relation_emb / keys / itemT / scratch not 16-byte aligned: KGAT_E_BADARG;
 * outside the envelope: KGAT_E_UNSUPPORTED; scratch below kgat_eval_ripple_scratch_bytes(n_call, n_items, d,
 * n_memory, n_hop, K): KGAT_E_WORKSPACE.  Every check precedes any device work. */
int kgat_eval_ripple_supported(int d, int n_memory, int n_hop, int mode, int K);
int kgat_eval_ripple_keys_f32(int64_t n_call, const int32_t* user_ids, int d, int n_memory, int n_hop, int n_rel,
                              int64_t n_nodes, int64_t n_users, const float* ent, const float* relation_emb,
                              const int32_t* mem_h, const int32_t* mem_r, float* keys, kgat_stream_t stream);
size_t kgat_eval_ripple_scratch_bytes(int64_t n_call, int64_t n_items, int d, int n_memory, int n_hop, int K);
int kgat_eval_ripple_topk_f32(int64_t n_call, const int32_t* user_ids, int64_t n_items, int d, int n_memory, int n_hop,
                              int mode, int all_hops, int64_t n_nodes, int64_t n_users, const float* itemT,
                              const float* keys, const float* ent, const int32_t* mem_t, const float* W,
                              const int32_t* train_ptr, const int32_t* train_items, int K, void* scratch,
                              size_t scratch_bytes, int32_t* topk_items, float* topk_scores, kgat_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* KGAT_HIP_H_ */
