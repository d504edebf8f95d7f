/*
 * gaib.h -- C ABI of the MI355X (gfx950) GNN aggregation engine.
 *
 * This is the drop-in boundary.  The reference has no FFI layer: its
 * "operator API" is a set of C++ declarations whose definitions the GPU Makefile target
 * takes from .cu files (src/gnn/Makefile:56-77).  The host-side C++ mirror of those
 * declarations lives in include/{gnn,layers,utils}/ of this repo and is implemented
 * ENTIRELY on top of the functions below; every entry point cites the reference
 * interface (file:line under /root/reference) it replaces.
 *
 * Conventions
 *   - plain C types only; all pointers named d_* are DEVICE pointers (HBM), h_* host.
 *   - every function returns GAIB_OK (0) or a negative gaib_status; gaib_last_error()
 *     gives the message.  The C++ mirror turns non-zero into the reference's
 *     print-and-exit (include/utils/cutils.h:18-28,133-174).
 *   - all work is enqueued on the context's HIP stream; nothing synchronises unless
 *     the name says so (the reference syncs after every launch: cutils.h:18-28).
 *   - feature matrices are row-major fp32 [nv x len]; row offsets are 64-bit (the
 *     reference's uint32 `dst*len`, graph_operations.h:100,105, overflows at N*D>2^32).
 */
#ifndef GAIB_H
#define GAIB_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  GAIB_OK = 0,
  GAIB_ERR_INVALID = -1, /* bad argument / shape */
  GAIB_ERR_HIP = -2,     /* a HIP runtime call failed */
  GAIB_ERR_NOMEM = -3,
  GAIB_ERR_ASYMMETRIC = -4, /* edge_transpose: reverse edge missing (math_functions.cpp:70 assert) */
  GAIB_ERR_UNSUPPORTED = -5,
  GAIB_ERR_COMM = -6 /* a collective failed, a peer reported a failure or did not arrive in time */
} gaib_status;

typedef struct gaib_ctx gaib_ctx;     /* device + stream + workspace              */
typedef struct gaib_graph gaib_graph; /* CSR in HBM + normalisers + row schedules */

const char* gaib_last_error(void);
const char* gaib_version(void);

/* ---- context -------------------------------------------------------------------------
 * replaces the static cuBLAS/cuSPARSE/cuRAND handle holder `gpu_context`
 * (include/gnn/gpu_context.h:4-16, src/utilities/random.cpp:62-80).
 * `stream` is a hipStream_t (NULL = the device's null stream); it is borrowed. */
int gaib_device_count(int* h_count); /* visible devices (initialises the HIP runtime: rank processes only, never a launcher) */
int gaib_ctx_create(int device, void* stream, gaib_ctx** out);
int gaib_ctx_destroy(gaib_ctx* ctx);
int gaib_ctx_set_stream(gaib_ctx* ctx, void* stream);
/* switch the context to a (non-blocking) stream of its own, created once and destroyed with the context: for callers
 * without a stream to lend -- the null stream cannot be recorded by gaib_capture_begin */
int gaib_ctx_own_stream(gaib_ctx* ctx);
int gaib_sync(gaib_ctx* ctx); /* CudaTest()'s cudaDeviceSynchronize, cutils.h:18-28 */
/* Side stream for work that is independent of the calls that follow it (the weight-gradient GEMM
 * next to the aggregation of the input gradient: an MFMA-bound and an HBM-bound kernel overlap).
 *   gaib_side_begin: everything enqueued so far is a dependency of the side stream; calls go to the
 *                    side stream (with its own scratch) from here ...
 *   gaib_side_end:   ... to here; calls go to the main stream again, which does NOT wait.
 *   gaib_side_wait:  the main stream waits for the side section.  Buffers the side section reads or
 *                    writes must not be written on the main stream between end and wait.
 * One side section at a time (begin after begin without wait is an error). */
int gaib_side_begin(gaib_ctx* ctx);
int gaib_side_end(gaib_ctx* ctx);
int gaib_side_wait(gaib_ctx* ctx);
/* HIP graphs: record a call sequence once, replay it with one launch.  The 2-layer, 16-column models of the
 * reference's shipped datasets (cora / citeseer, inputs/) are launch bound -- an epoch is ~40 kernels of a few
 * microseconds -- where the reference's GPU build pays a cudaDeviceSynchronize per op (cutils.h:18-28).
 *   gaib_capture_begin: every call on this context is RECORDED on its stream from here (nothing runs) ...
 *   gaib_capture_end:   ... to here; *out replays the sequence.  gaib_capture_abort drops an open capture.
 * Inside a capture, calls that wait for the stream or allocate return GAIB_ERR_INVALID with a message (gaib_sync,
 * gaib_memcpy_h2d/d2h, metrics with host results, a workspace or lazily built graph table that does not exist
 * yet): run the sequence once eagerly first.  Pointers and by-value scalars are frozen in the recording; per-replay
 * state lives in device memory (gaib_adam_step_dev, gaib_dropout_dev, gaib_masked_*_dev, gaib_memcpy_d2h_async).  The context must
 * own a real stream (not the null stream), without a side section or kernel timing switched on.
 * Scratch: a recording holds the addresses of the context's internal workspaces.  While any gaib_exec of a context
 * is alive, a workspace that has to grow (a later, larger call outside the replay) is kept allocated next to its
 * replacement and released with the last gaib_exec -- replays stay valid.  A gaib_exec is launched on the context it
 * was recorded on, and destroyed before it (gaib_ctx_destroy refuses otherwise). */
typedef struct gaib_exec gaib_exec;
int gaib_capture_begin(gaib_ctx* ctx);
int gaib_capture_end(gaib_ctx* ctx, gaib_exec** out);
int gaib_capture_abort(gaib_ctx* ctx);
int gaib_exec_launch(gaib_ctx* ctx, gaib_exec* exec);
int gaib_exec_elapsed_ms(gaib_exec* exec, float* h_ms); /* device time of the last launch; after gaib_sync */
int64_t gaib_exec_nodes(const gaib_exec* exec); /* graph nodes recorded (kernels, memsets, copies) */
int gaib_exec_destroy(gaib_exec* exec);

/* ---- memory: float/uint/uint8_malloc_device, *_free_device, copy_*_device, copy_float_host,
 * init_const_gpu  (include/utils/math_functions.hh:161-173, math_functions.cu:12-14;
 * templates malloc_device<T>/copy_async_device<T>, include/utils/cutils.h:193-202) ---- */
int gaib_malloc(gaib_ctx* ctx, size_t bytes, void** d_ptr);
int gaib_free(gaib_ctx* ctx, void* d_ptr);
int gaib_memcpy_h2d(gaib_ctx* ctx, void* d_dst, const void* h_src, size_t bytes);
int gaib_memcpy_d2h(gaib_ctx* ctx, void* h_dst, const void* d_src, size_t bytes); /* syncs */
int gaib_memcpy_d2d(gaib_ctx* ctx, void* d_dst, const void* d_src, size_t bytes);
/* pinned host memory and a stream-ordered read-back into it (valid after the next gaib_sync) */
int gaib_host_alloc(gaib_ctx* ctx, size_t bytes, void** h_ptr);
int gaib_host_free(gaib_ctx* ctx, void* h_ptr);
int gaib_memcpy_d2h_async(gaib_ctx* ctx, void* h_pinned_dst, const void* d_src, size_t bytes);
int gaib_fill_f32(gaib_ctx* ctx, int64_t n, float value, float* d_x);
/* x <- alpha * x  (scale, math_functions.cpp:336-356 / scal_gpu; the partitioned trainer rescales the loss gradient
 * from 1/(local range) to 1/(global range), softmax_loss_layer.cpp:31) */
int gaib_scale_f32(gaib_ctx* ctx, int64_t n, float alpha, float* d_x);
/* bf16 feature tables: raw bf16 bits in uint16_t.  f32 -> bf16 rounds to nearest, ties to even (torch's .to(torch.bfloat16)):
 * subnormals kept, finite values past the largest bf16 round to +-inf; a NaN stays a quiet NaN of the same sign (upper half
 * of its bits, quiet bit set).  bf16 -> f32 is exact (bits << 16).  in and out must not alias. */
int gaib_cast_f32_bf16(gaib_ctx* ctx, int64_t n, const float* d_in, uint16_t* d_out);
int gaib_cast_bf16_f32(gaib_ctx* ctx, int64_t n, const uint16_t* d_in, float* d_out);
/* gaib_cast_f32_bf16 into rows with a stride: d_in is dense fp32 [rows x len], d_out bf16 bits [rows x ld_out], ld_out >= len.
 * Columns < len carry gaib_cast_f32_bf16's rounding, columns len .. ld_out - 1 are written as +0.0; ld_out == len gives the bits
 * of gaib_cast_f32_bf16.  One pass; 16-byte stores where ld_out % 8 == 0 and d_out is 16-B aligned.  The table the _ld
 * aggregation calls below gather from, at the stride gaib_bf16_row_stride names. */
int gaib_cast_f32_bf16_rows(gaib_ctx* ctx, int64_t rows, int len, const float* d_in, int64_t ld_out, uint16_t* d_out);

/* Zero-suppressed tables ("zs"): a row of 128 floats as 384 bytes on a 128-byte boundary -- two 64-bit masks (M0: bit l set when
 * column 2l holds anything but bit pattern 0x00000000; M1: the same for column 2l + 1), then pairs of fp32 bit patterns: dword
 * 4 + 2k is the k-th kept value of the even columns, dword 5 + 2k the k-th of the odd columns; the rest of the row is 0.  -0.0,
 * NaN, inf and subnormals are kept, so unpacking reproduces every bit.  Either half holds up to 46 values: a row with more in
 * one half keeps only its masks and is read from the dense table, which stays valid.
 * gaib_pack_zs: d_in [rows x 128] fp32 (8-B aligned) -> d_zs [rows x 384 B] (128-B aligned); d_overflow (may be NULL): a device
 * word the number of over-capacity rows is ADDED to.  gaib_unpack_zs: the inverse, d_dense being the table the image was made
 * from (read for over-capacity rows only).  len != 128: GAIB_ERR_UNSUPPORTED. */
int gaib_pack_zs(gaib_ctx* ctx, int64_t rows, int len, const float* d_in, void* d_zs, uint32_t* d_overflow);
int gaib_unpack_zs(gaib_ctx* ctx, int64_t rows, int len, const void* d_zs, const float* d_dense, float* d_out);
/* Wide zero-suppressed tables: rows of 256 floats, packed as one image per 128-column K-slab of the aggregation, slab-major:
 * d_zs [2][rows][384 B] (128-B aligned).  Image s is bit for bit what gaib_pack_zs writes for columns 128 s .. 128 s + 127 of d_in
 * (same format, 46 values per half of a half row); one pass over d_in [rows x 256] (8-B aligned).  d_overflow (may be NULL): the
 * number of over-capacity ROW-SLABS is ADDED to it -- a row over capacity in both slabs counts twice.  gaib_unpack_zs_wide: the
 * inverse, d_dense [rows x 256] being the table the image was made from.  len != 256: GAIB_ERR_UNSUPPORTED, nothing written. */
int gaib_pack_zs_wide(gaib_ctx* ctx, int64_t rows, int len, const float* d_in, void* d_zs, uint32_t* d_overflow);
int gaib_unpack_zs_wide(gaib_ctx* ctx, int64_t rows, int len, const void* d_zs, const float* d_dense, float* d_out);

/* ---- graph: LearningGraph's device half (include/gnn/lgraph.h:20-277) ------------------
 * gaib_graph_create  = alloc_on_device + copy_to_gpu (src/gnn/lgraph.cu:51-92).
 *   rowptr: nv+1 entries of `rowptr_bits` (32: index_t as LearningGraph holds it; 64: as
 *   graph.vertex.bin stores it, reader.cpp:446-454); colidx: ne uint32 (graph.edge.bin).
 *   src_on_device != 0 means the two arrays are already in HBM (they are copied).
 *   Rows must be sorted by column id (lgraph.h:185 / math_functions.cpp:32-44 need it). */
int gaib_graph_create(gaib_ctx* ctx, int64_t nv, int64_t ne, const void* rowptr, int rowptr_bits,
                      const uint32_t* colidx, int src_on_device, gaib_graph** out);
/* Rectangular variant for a vertex-range partition (modelled on
 * PartitionedGraph::edgecut_induced_partition1D, src/partitioner/graph_partition.cc:128-178):
 * nv owned rows, column ids index a feature table of nc >= nv rows (owned rows first, halo
 * rows after).  add_selfloop / edge_transpose / GAT need a square graph. */
int gaib_graph_create_rect(gaib_ctx* ctx, int64_t nv, int64_t nc, int64_t ne, const void* rowptr,
                           int rowptr_bits, const uint32_t* colidx, int src_on_device,
                           gaib_graph** out);
/* Partitioned graphs: a halo column's local degree is truncated, so the normalisers come from
 * the GLOBAL graph: d_row_vdata / d_row_inv_deg [nv] (NULL = derive from this graph's rowptr; pass
 * them when the rows hold only part of their edges, i.e. the owned-/halo-column split graphs),
 * d_col_vdata [nc] (deg^-1/2), d_col_inv_deg [nc] (1/deg).  Arrays are copied. */
int gaib_graph_set_vertex_norm(gaib_ctx* ctx, gaib_graph* g, const float* d_row_vdata,
                               const float* d_row_inv_deg, const float* d_col_vdata,
                               const float* d_col_inv_deg);
int gaib_graph_destroy(gaib_graph* g);
/* LearningGraph::add_selfloop (lgraph.h:185-218) as a device-side rebuild. */
int gaib_graph_add_selfloop(gaib_ctx* ctx, const gaib_graph* g, gaib_graph** out);
/* Opt-in relabelling: the same graph under a new vertex numbering computed on the device from the graph alone
 * (GAIB_ORDER_DEGREE: hubs first; GAIB_ORDER_BFS: breadth-first levels from the highest-degree vertex; GAIB_ORDER_CM:
 * Cuthill-McKee inside those levels).  A numbering with
 * locality is worth up to 1.2-1.6x to the aggregation; the library never relabels on its own.  Every
 * row keeps the ORDER of its edges, so aggregation outputs are bit-identical once un-permuted.
 *   d_new_of_old [nv] (required), d_old_of_new [nv] (may be NULL): int64 device arrays the call fills.
 *   features in the new numbering:  gaib_gather_rows(ctx, nv, d_old_of_new, len, x_old, x_new)
 *   outputs back in the old one:     gaib_gather_rows(ctx, nv, d_new_of_old, len, y_new, y_old)
 * The reference has no counterpart (its reader keeps the file's numbering, reader.cpp:414-457). */
#define GAIB_ORDER_DEGREE 1
#define GAIB_ORDER_BFS 2
#define GAIB_ORDER_CM 3 /* the BFS levels, inside a level by the position of the first parent (Cuthill-McKee) */
int gaib_graph_reorder(gaib_ctx* ctx, gaib_graph* g, int method, gaib_graph** out, int64_t* d_new_of_old,
                       int64_t* d_old_of_new);
/* A relabelled graph's rows keep their edge order, i.e. their column ids are NOT ascending: it is an aggregation-only
 * graph -- gaib_edge_transpose / GAIB_W_EDGE_T / the GAT backward entry points, which derive the reverse-edge permutation
 * from sorted rows (math_functions.cpp:32-44), refuse it with GAIB_ERR_UNSUPPORTED.  gaib_graph_sort_rows sorts every row's
 * column ids (in place; per-edge caches are rebuilt on demand): everything runs on it, and aggregation results are then equal
 * to the original numbering's up to fp32 summation order instead of bit for bit. */
int gaib_graph_sort_rows(gaib_ctx* ctx, gaib_graph* g);
/* The subgraph a vertex set induces on g, built on the device -- what the sampled path of the trainer rebuilds every epoch.
 *   kept [n_kept]: vertex ids of g, STRICTLY ASCENDING, every id < nv; host memory, or device memory with kept_on_device != 0.
 *   GAIB_INDUCE_RELABEL : n_kept rows; row k holds the kept neighbours of kept[k], renumbered by their position in `kept`
 *                         (Sampler::generateSubgraph, src/gnn/sampler.cpp).  n_kept == nv reproduces g's CSR.
 *   GAIB_INDUCE_KEEP_IDS: nv rows under g's own ids; the row of a dropped vertex is empty, a kept row keeps its kept neighbours
 *                         (LearningGraph::generate_masked_graph).
 * *out is an ordinary square graph: every row keeps the ORDER of its surviving edges (sorted rows stay sorted), self loops
 * survive.  d_rows_out (device int64 [n_kept], may be NULL) receives the kept ids widened: the index list gaib_gather_rows /
 * gaib_gather_rows_u8 take for the feature / label rows.  n_kept == 0 is valid (a graph of 0 rows; nv empty rows in KEEP_IDS).
 * Refusals create nothing and leave the graph's cached bitmap reusable: a rectangular g -> GAIB_ERR_UNSUPPORTED; a list that is
 * not strictly ascending or holds an id >= nv -> GAIB_ERR_INVALID (found on the device; the bad id is never used as an
 * address; d_rows_out may then be partly written); inside a recording -> GAIB_ERR_INVALID (the call allocates and waits once).
 * Cost: one stream wait and one 16-byte read-back (edge count + flag) per call; work proportional to the kept rows' edges, plus
 * nv / 8 bytes cleared (the membership bitmap cached on g; KEEP_IDS also writes its nv + 1 row pointers).  DESIGN.md 10. */
#define GAIB_INDUCE_RELABEL 0
#define GAIB_INDUCE_KEEP_IDS 1
int gaib_graph_induce(gaib_ctx* ctx, gaib_graph* g, int64_t n_kept, const uint32_t* kept, int kept_on_device, int mode,
                      gaib_graph** out, int64_t* d_rows_out);
int64_t gaib_graph_nv(const gaib_graph* g);
int64_t gaib_graph_ne(const gaib_graph* g);
int64_t gaib_graph_nc(const gaib_graph* g); /* columns = rows of the feature table its column ids index (nv unless rectangular) */
const int64_t* gaib_graph_rowptr(const gaib_graph* g);  /* device, int64[nv+1] */
const uint32_t* gaib_graph_colidx(const gaib_graph* g); /* device, uint32[ne]  */
/* compute_vertex_data (lgraph.cpp:22-34 / lgraph.cu:94-105): deg^-1/2, 0 for isolated. */
int gaib_graph_compute_vertex_data(gaib_ctx* ctx, gaib_graph* g);
const float* gaib_graph_vertex_data(const gaib_graph* g); /* device float[nv] or NULL */
/* compute_edge_data (lgraph.cpp:6-20 / lgraph.cu:107-140): 1/(sqrt(d_i)*sqrt(d_j)). */
int gaib_graph_compute_edge_data(gaib_ctx* ctx, gaib_graph* g);
const float* gaib_graph_edge_data(const gaib_graph* g); /* device float[ne] or NULL */
/* device bytes held by the graph (CSR + normalisers + schedules) */
int64_t gaib_graph_device_bytes(const gaib_graph* g);

/* ---- sparse aggregation (the hot loop) -------------------------------------------------
 * out[i,:] = sum_{e in row i} w_e * in[col_e,:]      (out is fully overwritten)
 *   GAIB_W_GCN    w_e = vd[i]*vd[col_e]      GCN_Aggregator::aggregate/d_aggregate
 *                                            (gcn_aggregator.cpp:23-77; .cu:14-51)
 *   GAIB_W_MEAN   w_e = 1/deg(i)             SAGE_Aggregator::aggregate   (sage_aggregator.cpp:7-30)
 *   GAIB_W_MEAN_T w_e = 1/deg(col_e)         SAGE_Aggregator::d_aggregate (sage_aggregator.cpp:32-54)
 *   GAIB_W_EDGE   w_e = d_edge_w[e]          update_all (gat_aggregator.cpp:26-45), spmm()
 *                                            (math_functions.cpp:207-220; cusparseSpMM .cu:407-410)
 *   GAIB_W_EDGE_T w_e = d_edge_w[rev(e)]     symmetric_csr_transpose + update_all fused
 *                                            (gat_aggregator.cpp:175,198)
 * Rows of degree <= the heavy-row threshold are summed in CSR order with a separate
 * multiply and add (bit-identical to the OpenMP loop); longer rows are split over the
 * waves of a workgroup and combined through LDS in a fixed order. */
typedef enum {
  GAIB_W_GCN = 0,
  GAIB_W_MEAN = 1,
  GAIB_W_MEAN_T = 2,
  GAIB_W_EDGE = 3,
  GAIB_W_EDGE_T = 4
} gaib_weight_kind;
int gaib_spmm(gaib_ctx* ctx, gaib_graph* g, int weight_kind, const float* d_edge_w, int len,
              const float* d_in, float* d_out);
/* out[i,:] += ... : the second half of a split aggregation (owned-column edges first with
 * gaib_spmm, halo-column edges added once the halo rows have arrived). */
int gaib_spmm_acc(gaib_ctx* ctx, gaib_graph* g, int weight_kind, const float* d_edge_w, int len,
                  const float* d_in, float* d_out);
/* general form: flags = GAIB_ACCUMULATE (out += ...) | GAIB_RELU (relu_gpu fused into the store:
 * the layers apply the activation right after the aggregation / GEMM, gcn_layer.cpp:27) */
#define GAIB_ACCUMULATE 1
#define GAIB_RELU 2
#define GAIB_AGG_SCRATCH 4 /* gaib_spmm_gemm: d_agg is scratch, its contents after the call are unspecified */
#define GAIB_OVERLAPS_TRANSFER 8 /* gaib_spmm_gemm*: a halo exchange is in flight on the communicator's stream while this call
                                  * runs (between gaib_halo_exchange_begin and _end).  The fused kernel is one persistent
                                  * workgroup per CU that holds the CU's registers until its last tile; under RCCL it then leaves
                                  * "comm_reserve_cus" CUs to the send / recv kernels: the option (or GAIB_COMM_RESERVE_CUS) where one is set
                                  * -- an explicit 0 included, -1 = unset --, else gaib_comm_init's default for its transport (32
                                  * under RCCL with > 1 rank, 0 on the peer-to-peer pull); at most num_cus - 64 */
int gaib_spmm_ex(gaib_ctx* ctx, gaib_graph* g, int weight_kind, const float* d_edge_w, int len,
                 const float* d_in, float* d_out, int flags);
/* gaib_spmm_ex over a bf16 table: d_in is [nc x len] bf16 bits (row-major), d_out fp32 [nv x len], flags as for gaib_spmm_ex.
 * Every gathered element is widened exactly and the sums are gaib_spmm_ex's (same weights, CSR order, separate multiply and
 * add, same heavy-row split and fixed combine order, same ordered-chunk rule), so the result is BIT-IDENTICAL to gaib_spmm_ex
 * on the table widened to fp32 (gaib_cast_bf16_f32) -- for d_in 8-B aligned and d_out 16-B aligned (otherwise a dense
 * graph that gaib_spmm_ex aggregates by ordered chunks is aggregated row by row: deterministic, the CSR-order sum).
 * Single-head weights (GAIB_W_GCN / _MEAN / _MEAN_T / _EDGE / _EDGE_T); square and rectangular graphs.  A graph with a row
 * map (a row class of a partition, gaib_graph_split_classes): GAIB_ERR_UNSUPPORTED.  A table of >= 4 GB in bf16 is gathered
 * with 64-bit addresses. */
int gaib_spmm_bf16(gaib_ctx* ctx, gaib_graph* g, int weight_kind, const float* d_edge_w, int len, const uint16_t* d_in,
                   float* d_out, int flags);
/* bf16 tables with a row stride.  The time of a gather follows the 128-byte lines a row touches: packed bf16 rows of 47 (94 B)
 * or 100 columns (200 B) touch 1.72 / 2.55 lines on average, rows that start on line boundaries 1 / 2.
 * gaib_bf16_row_stride: *ld = the stride (elements) a table of len columns should be cast to for graph g -- the row bytes
 * rounded up to 64 where that saves more than 10 % of the lines (64 at len 47, 128 at len 100), else len (64, 128, 200, 256,
 * ...); always len for len <= 16, on a graph with ne <= 4 nc or with a row map, and under option "spmm_bf16_pad" = 0.
 * gaib_spmm_bf16_ld: gaib_spmm_bf16 on d_in = [nc x ld] bf16 bits whose first len columns are the table.  ld == len, or
 * ld > len with ld % 4 == 0 (rows keep the table's 8-B alignment); anything else is GAIB_ERR_INVALID before any launch.  The
 * columns behind len are never read into a result (they may hold anything).  Lane layout, ordered chunks, heavy threshold and
 * column slabs are chosen on len as in the dense call, so d_out is BIT-IDENTICAL to gaib_spmm_bf16 on the same values stored
 * densely; ld enters the gather addresses, the buffer-descriptor size nc * ld * 2 and the 4 GB test only.  Profile keys and
 * algorithmic bytes (2 len per gathered row) are the dense call's.  Refusals as gaib_spmm_bf16. */
int gaib_bf16_row_stride(gaib_ctx* ctx, gaib_graph* g, int len, int64_t* ld);
int gaib_spmm_bf16_ld(gaib_ctx* ctx, gaib_graph* g, int weight_kind, const float* d_edge_w, int len, int64_t ld,
                      const uint16_t* d_in, float* d_out, int flags);
/* multi-head attention weights: d_edge_w is [ne][heads]; column c uses head c / (len/heads).
 * weight_kind must be GAIB_W_EDGE or GAIB_W_EDGE_T when heads > 1. */
int gaib_spmm_mh(gaib_ctx* ctx, gaib_graph* g, int weight_kind, const float* d_edge_w, int heads,
                 int len, const float* d_in, float* d_out, int flags);

/* ---- GAT attention pieces ---------------------------------------------------------------
 * gaib_gat_scores: GAT_Aggregator::aggregate's score pass (gat_aggregator.cpp:60-92;
 *   compute_attn_score_warp, graph_operations.h:250-337): per edge
 *   temp = a_l.h[i] + a_r.h[col_e]; scores = leaky_relu(temp, eps); norm = row softmax.
 *   The d_* edge arrays [ne] are written; d_scores may be NULL for 1, 2, 4, 8 or 16 heads (it is
 *   leaky_relu(temp) and nothing in backward reads it), and so may d_temp_scores: backward reads only
 *   its sign, which gaib_gat_softmax_bwd_alpha_re forms again from the per-vertex dots. */
int gaib_gat_scores(gaib_ctx* ctx, gaib_graph* g, int len, const float* d_h, const float* d_alpha_l,
                    const float* d_alpha_r, float epsilon, float* d_temp_scores, float* d_scores,
                    float* d_norm_scores);
/* Multi-head forms (BASELINE config "reddit GAT 2-layer 8-head"; the reference is single-head,
 * include/gnn/aggregator.h:62-65): `heads` independent attentions on the column slices
 * [h*len/heads, (h+1)*len/heads); alpha vectors stay [len]; every edge array is [ne][heads].
 * heads == 1 is exactly the single-head entry point. */
int gaib_gat_scores_mh(gaib_ctx* ctx, gaib_graph* g, int len, int heads, const float* d_h,
                       const float* d_alpha_l, const float* d_alpha_r, float epsilon,
                       float* d_temp_scores, float* d_scores, float* d_norm_scores);
int gaib_sddmm_mh(gaib_ctx* ctx, gaib_graph* g, int len, int heads, const float* d_grad,
                  const float* d_feat, float* d_out_e);
int gaib_gat_softmax_bwd_alpha_mh(gaib_ctx* ctx, gaib_graph* g, int len, int heads, const float* d_feat,
                                  const float* d_norm_scores, const float* d_norm_scores_grad,
                                  const float* d_temp_scores, float epsilon, float* d_scores,
                                  float* d_alpha_lgrad, float* d_alpha_rgrad);
int gaib_edge_transpose_mh(gaib_ctx* ctx, gaib_graph* g, int heads, const float* d_in_e, float* d_out_e);
/* SDDMM (gat_aggregator.cpp:106-113; compute_scores_grad_warp, graph_operations.h:191-223):
 *   d_out_e[e] = <grad[i,:], feat[col_e,:]> */
int gaib_sddmm(gaib_ctx* ctx, gaib_graph* g, int len, const float* d_grad, const float* d_feat,
               float* d_out_e);
/* softmax backward + leaky-relu' + alpha gradients (gat_aggregator.cpp:121-167;
 *   compute_alpha_grad_warp, graph_operations.h:396-467).  d_scores[e] is overwritten with
 *   d(softmax) like the reference does; d_alpha_lgrad/d_alpha_rgrad [len] are overwritten.
 *   Deterministic (no float atomics). */
int gaib_gat_softmax_bwd_alpha(gaib_ctx* ctx, gaib_graph* g, int len, const float* d_feat,
                               const float* d_norm_scores, const float* d_norm_scores_grad,
                               const float* d_temp_scores, float epsilon, float* d_scores,
                               float* d_alpha_lgrad, float* d_alpha_rgrad);
/* general form: H heads; d_scores (the softmax-input gradient ds) may be NULL when the caller does not read it;
 * d_grad_rows / d_fwd_out_rows (both or neither, [nv x len]): the gradient and the forward output of the
 * aggregation -- sum_e p_e dp_e is then taken per vertex as <grad_i, out_i> and the edge arrays are read once;
 * d_norm_scores_t (optional, [ne][heads]) receives the transposed attention p[rev(e)] (symmetric_csr_transpose,
 * gat_aggregator.cpp:172-175), produced in the pass that already walks rev: the gradient aggregation can then read
 * it linearly (GAIB_W_EDGE) instead of through the permutation (GAIB_W_EDGE_T). */
int gaib_gat_softmax_bwd_alpha_ex(gaib_ctx* ctx, gaib_graph* g, int len, int heads, const float* d_feat,
                                  const float* d_norm_scores, const float* d_norm_scores_grad,
                                  const float* d_temp_scores, float epsilon, float* d_scores,
                                  float* d_alpha_lgrad, float* d_alpha_rgrad, const float* d_grad_rows,
                                  const float* d_fwd_out_rows, float* d_norm_scores_t);
/* the same without the temp_scores array (1, 2, 4, 8 or 16 heads): leaky-relu' needs only the sign of
 * temp = a_l.h[i] + a_r.h[col_e], formed again from d_feat and the alpha vectors (4 + 4*heads bytes per edge out of the
 * caches instead of 4*heads written in forward and read here through HBM).  Same results bit for bit. */
int gaib_gat_softmax_bwd_alpha_re(gaib_ctx* ctx, gaib_graph* g, int len, int heads, const float* d_feat,
                                  const float* d_alpha_l, const float* d_alpha_r, const float* d_norm_scores,
                                  const float* d_norm_scores_grad, float epsilon, float* d_scores,
                                  float* d_alpha_lgrad, float* d_alpha_rgrad, const float* d_grad_rows,
                                  const float* d_fwd_out_rows, float* d_norm_scores_t);
/* The whole edge side of GAT_Aggregator::d_aggregate (gat_aggregator.cpp:99-200: SDDMM, softmax backward + leaky-relu',
 * alpha gradients, transpose, gradient aggregation) in ONE sweep over the edges.  d_fwd_out is the aggregation's forward
 * output (sum_e p_e dp_e of a row == <grad_i, out_i>); d_grad_out [nv x len] must not alias an input.  Nothing per edge is
 * written: the per-edge arrays dp / ds / p^T of the staged entry points do not exist on this path.  The attention comes
 * from d_norm_scores [ne][heads], or -- when d_row_stats (gaib_gat_forward_fused) is given -- is formed again.  Applies to
 * len == 32, 64 or 128 (8, 16 or 32 lanes x 4 columns per edge; the reference's GAT covers len <= 128, global.h:58) with 1, 2, 4,
 * 8 or 16 heads of at least 4 columns, on any graph (option "gat_fused_bwd": -1 or 1 = whenever the shape fits, 0 = never);
 * otherwise returns GAIB_ERR_UNSUPPORTED without touching anything and the caller uses the staged entry points. */
int gaib_gat_backward_fused(gaib_ctx* ctx, gaib_graph* g, int len, int heads, const float* d_feat, const float* d_grad,
                            const float* d_fwd_out, const float* d_alpha_l, const float* d_alpha_r,
                            const float* d_norm_scores, const float* d_row_stats, float epsilon, float* d_grad_out,
                            float* d_alpha_lgrad, float* d_alpha_rgrad);
/* GAT_Aggregator::aggregate (gat_aggregator.cpp:57-97) in ONE sweep: scores, edge softmax (online: running maximum and
 * sum per chunk, combined per row) and the attention-weighted aggregation; d_out = act(P h), and d_row_stats
 * [nv][heads][2] = (row maximum of the leaky-relu'd scores, 1 / row sum of exp) is everything backward needs to form the
 * attention again: pass it to gaib_gat_backward_fused as d_row_stats (d_norm_scores may then be NULL) and no [ne][heads]
 * array exists at all.  Same cover as gaib_gat_backward_fused (option "gat_fused_fwd"); GAIB_ERR_UNSUPPORTED otherwise. */
int gaib_gat_forward_fused(gaib_ctx* ctx, gaib_graph* g, int len, int heads, const float* d_h, const float* d_alpha_l,
                           const float* d_alpha_r, float epsilon, int relu, float* d_out, float* d_row_stats);
/* MULTI-HEAD ROWS WIDER THAN 128 COLUMNS (option "gat_fused_wide", default 0).  Heads are independent in everything the two
 * sweeps compute, so a row of len = S * w columns with heads = S * Hs heads is S independent problems of w columns and Hs heads
 * in column windows of the same tables.  gaib_gat_fused_slabs is the shape rule, a pure function (no context, no device): it
 * returns S and writes w through `width` (which may be NULL): (len, 1) where the one-sweep kernels apply as they are; else the
 * first w of 128, 64, 32 with len % w == 0, S = len / w >= 2, heads % S == 0 and (w, heads / S) a shape of those kernels; else
 * 0 (w = 0).  (256, 8) -> 2 slabs of 128; (512, 8) -> 4 of 128; (256, 64) -> 4 of 64; (256, 1) -> 0: a single head wider than
 * 128 columns stays staged.
 * With the option at 1, gaib_gat_forward_fused and gaib_gat_backward_fused (row-statistics form: d_row_stats != NULL) accept
 * every shape with S >= 2 on square graphs, fp32 tables, under today's other conditions (16-byte aligned buffers, "gat_fused_fwd"
 * / "gat_fused_bwd" != 0, ne > 0; else GAIB_ERR_UNSUPPORTED with nothing touched); with the option at 0 they return what they
 * always returned.  A wide call is a loop over the slabs on the context's stream, each slab the narrow call's own kernel sequence
 * at (w, Hs) on strided rows: slab s covers columns [s w, (s + 1) w) of the tables and of the alpha vectors and gradients, and
 * heads [s Hs, (s + 1) Hs) of d_row_stats, all in their full-width layouts [nv][len] / [nv][heads][2] -- so its outputs there
 * are BIT-IDENTICAL to the narrow call at (len = w, heads = Hs) on contiguous copies of the windows, under the same options.
 * "gat_chunk_xcd" is honoured, "gat_fused_unroll" = 8 where w == 64; "gat_bwd_pk" and "gat_interleave" are ignored (the chunk
 * kernel over the three separate tables runs, as in the _drop calls).  Profile: one record per call under "gat_fwd_fused" /
 * "gat_bwd_fused", the narrow byte formula at (w, Hs) times S (column ids count S times).
 * The _drop calls are covered too, see gaib_gat_forward_fused_drop_win below, and so are the _bf16 and _drop_bf16 calls (see
 * there).  Not covered, today's behaviour at these shapes whatever the option says: the _rect calls, gaib_gat_score_signs, a
 * single head wider than 128 columns, the packed-math sweep. */
int gaib_gat_fused_slabs(int len, int heads, int* width);
/* The one-sweep forward and backward over bf16 TABLES (layer-library option "gat_bf16").
 * Tables: d_h_bf16 / d_feat_bf16 / d_grad_bf16 hold raw bf16 bits, [nv x len], 8-byte aligned.  EVERY read of h and grad is taken
 * from them and widened exactly: own rows and gathered rows in the sweep, grad in the row dots <grad_v, out_v>, h in the alpha
 * gradients.  Everything else (alpha vectors, forward output, row statistics, the per-vertex records inside the sweep) is fp32.
 * Outputs: fp32, and BIT-IDENTICAL to gaib_gat_forward_fused / gaib_gat_backward_fused (row-statistics form) called on the
 * tables widened to fp32 (gaib_cast_bf16_f32) under the same options: "gat_fused_unroll", "gat_chunk_xcd" and "gat_bwd_pk" are
 * honoured exactly as by the fp32 calls -- with gat_bwd_pk = 1 the result has the bits of the fp32 packed-math sweep, over a
 * table row of len dwords (h_k in the low half, grad_k in the high half) followed by the fp32 records, 4 len + 16 heads bytes,
 * the table below 4 GB; on a shape the packed-math sweep does not cover (a head of 32 lanes) the option changes nothing, as
 * in fp32.  "gat_interleave" is ignored by the bf16 calls (it changes no bits in fp32 either).
 * Cover and refusals are those of the fp32 calls: len 32 / 64 / 128 with 1, 2, 4, 8 or 16 heads of >= 4 columns, square graphs
 * only (no _rect forms), options "gat_fused_fwd" / "gat_fused_bwd" = 0 switch them off, a misaligned buffer (bf16 tables: 8
 * bytes, fp32 buffers: 16) -> GAIB_ERR_UNSUPPORTED with nothing touched; a graph without rows is handled as by the fp32 calls
 * (forward: GAIB_ERR_UNSUPPORTED; backward: zero alpha gradients, GAIB_OK).  d_row_stats == NULL in backward is
 * GAIB_ERR_INVALID: there is no attention-array form.
 * Profile: the launches are timed under the fp32 calls' keys "gat_fwd_fused" / "gat_bwd_fused" with the fp32 byte formula, so
 * the achieved rate of such a row is a work rate in dense (fp32) bytes.
 * WIDE ROWS: with option "gat_fused_wide" = 1 both calls also accept every shape where gaib_gat_fused_slabs(len, heads) gives
 * S >= 2, under their other conditions, and run the slab loop of the fp32 wide calls on the bf16 tables: slab s gathers from
 * column s * w of the tables with the row stride len (2 s w bytes: a multiple of 64, the 8-byte loads stay aligned).  Outputs:
 * BIT-IDENTICAL to the wide gaib_gat_forward_fused / gaib_gat_backward_fused on the widened tables; "gat_chunk_xcd" is honoured,
 * "gat_fused_unroll" = 8 where w == 64, "gat_bwd_pk" is ignored at these shapes (as by the fp32 wide calls); the profile record
 * carries the wide byte formula.  With the option at 0 the calls answer at these shapes as they always did. */
int gaib_gat_forward_fused_bf16(gaib_ctx* ctx, gaib_graph* g, int len, int heads, const uint16_t* d_h_bf16,
                                const float* d_alpha_l, const float* d_alpha_r, float epsilon, int relu, float* d_out,
                                float* d_row_stats);
int gaib_gat_backward_fused_bf16(gaib_ctx* ctx, gaib_graph* g, int len, int heads, const uint16_t* d_feat_bf16,
                                 const uint16_t* d_grad_bf16, const float* d_fwd_out, const float* d_alpha_l,
                                 const float* d_alpha_r, const float* d_row_stats, float epsilon, float* d_grad_out,
                                 float* d_alpha_lgrad, float* d_alpha_rgrad);
/* The one-sweep forward and backward under ATTENTION DROPOUT (layer-library option "gat_fused_drop"), fp32 tables.
 * The weight of (edge e, head k) is w = mask * scale with mask = u01(seed, e * heads + k) > drop_rate: EXACTLY the mask
 * gaib_dropout(n = ne * heads, scale, drop_rate, seed, ..) draws for element e * heads + k of an [ne][heads] array (e = the
 * edge's position in the graph's CSR), formed inside the sweep -- no [ne][heads] array exists on this path either.
 * Forward: d_out = act(sum_e p_e w_e h_c).  The softmax does not see the mask: d_row_stats are the bits gaib_gat_forward_fused
 * writes.  Backward (row-statistics form only): dp_e = w_e <grad_i, h_c>, and through the reverse edge r = rev(e) dp_r =
 * w_r <grad_c, h_i> and d_grad_out_i = sum_e p_r w_r grad_c; d_fwd_out is the DROPPED forward output (sum_e p_e dp_e of a row is
 * still <grad_i, out_i>).  With drop_rate = 0 and scale = 1 every output has the bits of the undropped calls.
 * Cover and refusals are those of gaib_gat_forward_fused / gaib_gat_backward_fused: len 32 / 64 / 128 with 1, 2, 4, 8 or 16 heads
 * of >= 4 columns, 16-byte aligned buffers, options "gat_fused_fwd" / "gat_fused_bwd" = 0 -> GAIB_ERR_UNSUPPORTED with nothing
 * touched; "gat_fused_unroll" and "gat_chunk_xcd" are honoured as there (same bits); "gat_bwd_pk" and "gat_interleave" are
 * ignored; a graph without rows: forward GAIB_ERR_UNSUPPORTED, backward zero alpha gradients and GAIB_OK.  Further: a rectangular
 * graph -> GAIB_ERR_UNSUPPORTED (a rank cannot name the reverse edge's index on another rank); a graph whose reverse-edge
 * permutation cannot be built -> that error, from forward and backward alike; drop_rate outside [0, 1) and d_row_stats == NULL
 * in backward -> GAIB_ERR_INVALID.  Profile keys and byte formulas: "gat_fwd_fused" / "gat_bwd_fused" of the undropped calls. */
int gaib_gat_forward_fused_drop(gaib_ctx* ctx, gaib_graph* g, int len, int heads, const float* d_h, const float* d_alpha_l,
                                const float* d_alpha_r, float epsilon, int relu, float drop_rate, float scale, uint64_t seed,
                                float* d_out, float* d_row_stats);
int gaib_gat_backward_fused_drop(gaib_ctx* ctx, gaib_graph* g, int len, int heads, const float* d_feat, const float* d_grad,
                                 const float* d_fwd_out, const float* d_alpha_l, const float* d_alpha_r,
                                 const float* d_row_stats, float epsilon, float drop_rate, float scale, uint64_t seed,
                                 float* d_grad_out, float* d_alpha_lgrad, float* d_alpha_rgrad);
/* The _drop calls over bf16 TABLES (layer-library options "gat_bf16" with "gat_fused_drop"): argument order of the _drop calls,
 * the tables as in the _bf16 calls (raw bf16 bits, row-major [nv][len], 8-byte aligned); records, statistics, alpha vectors and
 * all outputs are fp32.  Every output is BIT-IDENTICAL to gaib_gat_forward_fused_drop / gaib_gat_backward_fused_drop on the
 * tables widened to fp32 under the same options and the same (drop_rate, scale, seed): the masks are those gaib_dropout draws
 * over [ne][heads], d_row_stats does not see the mask, drop_rate = 0 with scale = 1 gives the bits of the undropped _bf16 calls.
 * Cover and refusals are those of the _drop calls (square graphs, a buildable reverse-edge permutation asked for by forward and
 * backward alike, "gat_fused_fwd" / "gat_fused_bwd" = 0 or a misaligned buffer -> GAIB_ERR_UNSUPPORTED with nothing touched;
 * d_row_stats == NULL, drop_rate outside [0, 1), an aliased output -> GAIB_ERR_INVALID; a graph without rows as there), and with
 * option "gat_fused_wide" = 1 the shapes with S >= 2 slabs are accepted as by the _drop calls, each slab with its head window
 * (heads, s * Hs) of the mask.  "gat_chunk_xcd" and "gat_fused_unroll" are honoured, "gat_bwd_pk" and "gat_interleave" ignored.
 * Profile: keys and byte formulas of the corresponding fp32 _drop call. */
int gaib_gat_forward_fused_drop_bf16(gaib_ctx* ctx, gaib_graph* g, int len, int heads, const uint16_t* d_h_bf16,
                                     const float* d_alpha_l, const float* d_alpha_r, float epsilon, int relu, float drop_rate,
                                     float scale, uint64_t seed, float* d_out, float* d_row_stats);
int gaib_gat_backward_fused_drop_bf16(gaib_ctx* ctx, gaib_graph* g, int len, int heads, const uint16_t* d_feat_bf16,
                                      const uint16_t* d_grad_bf16, const float* d_fwd_out, const float* d_alpha_l,
                                      const float* d_alpha_r, const float* d_row_stats, float epsilon, float drop_rate, float scale,
                                      uint64_t seed, float* d_grad_out, float* d_alpha_lgrad, float* d_alpha_rgrad);
/* ATTENTION DROPOUT THROUGH A HEAD WINDOW OF THE MASK, and the _drop calls on rows wider than 128 columns.
 * The _win calls are the _drop calls at the same narrow shapes (len 32 / 64 / 128, contiguous tables [nv][len]) whose `heads`
 * heads are heads [mask_head0, mask_head0 + heads) of a row of mask_heads heads: the mask of (edge e, local head k) is the one
 * gaib_dropout draws for element e * mask_heads + mask_head0 + k (the index is formed in 64 bits).  With mask_heads == heads and
 * mask_head0 == 0 every output has the bits of the _drop call.  mask_head0 < 0 or mask_head0 + heads > mask_heads ->
 * GAIB_ERR_INVALID; cover, options, profile and every other refusal are those of the _drop calls.
 * With option "gat_fused_wide" = 1, gaib_gat_forward_fused_drop and gaib_gat_backward_fused_drop accept every shape where
 * gaib_gat_fused_slabs(len, heads) gives S >= 2, under the _drop calls' other conditions (square graphs, fp32 tables, 16-byte
 * aligned buffers, "gat_fused_fwd" / "gat_fused_bwd" != 0, ne > 0, a buildable reverse-edge permutation; else the _drop calls'
 * answer with nothing touched); with the option at 0 they answer as they always did.  The call is the slab loop of the undropped
 * wide calls: slab s is the window sequence at (w, Hs, mask_heads = heads, mask_head0 = s * Hs) on strided rows, so in its
 * columns and heads the outputs are BIT-IDENTICAL to the _win call on contiguous copies of the column windows, and the masks are
 * those of the [ne][heads] array of the full row.  d_row_stats has the bits of the undropped wide call; drop_rate = 0 with
 * scale = 1 gives the undropped wide call's bits everywhere.  "gat_chunk_xcd" is honoured, "gat_fused_unroll" = 8 where w == 64.
 * Profile: one record per call under "gat_fwd_fused" / "gat_bwd_fused" with the wide byte formula. */
int gaib_gat_forward_fused_drop_win(gaib_ctx* ctx, gaib_graph* g, int len, int heads, const float* d_h, const float* d_alpha_l,
                                    const float* d_alpha_r, float epsilon, int relu, float drop_rate, float scale, uint64_t seed,
                                    int mask_heads, int mask_head0, float* d_out, float* d_row_stats);
int gaib_gat_backward_fused_drop_win(gaib_ctx* ctx, gaib_graph* g, int len, int heads, const float* d_feat, const float* d_grad,
                                     const float* d_fwd_out, const float* d_alpha_l, const float* d_alpha_r,
                                     const float* d_row_stats, float epsilon, float drop_rate, float scale, uint64_t seed,
                                     int mask_heads, int mask_head0, float* d_grad_out, float* d_alpha_lgrad,
                                     float* d_alpha_rgrad);
/* Test / diagnostic: d_sign_out [ne][heads] (uint8) = (t_e > 0) of every pre-activation score a_l.h[i] + a_r.h[col_e]
 * EXACTLY as the one-sweep kernels form it.  leaky_relu' jumps at 0, so a score within rounding of zero takes either
 * slope in two correct fp32 evaluations; a comparison of the alpha gradients with an fp64 evaluation imposes these signs
 * on it to measure arithmetic only (the counterpart of running backward on the oracle's relu mask).  d_h [nc x len]. */
int gaib_gat_score_signs(gaib_ctx* ctx, gaib_graph* g, int len, int heads, const float* d_h, const float* d_alpha_l,
                         const float* d_alpha_r, uint8_t* d_sign_out);
/* The one-sweep forward / backward on a rank's RECTANGULAR graph (rows = owned vertices, columns = [owned | halo]; tables
 * [nc x len] with the owned rows first).  In a structurally symmetric graph the in-edges of an owned vertex are the
 * reverses of its out-edges, so rs_i, cs_i and the aggregated gradient of i follow from i's own edge list given the halo
 * vertices' h rows, grad rows and records rec[v][h] = (<grad_v, out_v>_h, row maximum, 1 / row sum, 0): two
 * forward-direction halo exchanges (grad rows, records = 4 * heads floats per vertex) and one sweep -- no transposed
 * structure, no reverse exchange.  phase: -1 = everything; 0 = only the chunks over owned columns (may run while the halo
 * rows are still arriving: it reads owned rows only); 1 = the remaining chunks + the per-row combination (phase 0's
 * partial results wait in the context's workspace: no other call on the context in between).  The alpha gradients cover
 * the owned rows; the caller sums them over the ranks.  Same shape cover as gaib_gat_backward_fused (len 32 / 64 / 128; 1, 2,
 * 4, 8 or 16 heads of >= 4 columns; options gat_fused_fwd / gat_fused_bwd = 0 switch them off), else GAIB_ERR_UNSUPPORTED.
 * A graph WITHOUT rows (a rank of a partition with fewer vertices than ranks) is accepted with NULL buffers: the answer --
 * GAIB_OK or GAIB_ERR_UNSUPPORTED -- then follows from len, heads and the option alone, i.e. it is what the ranks that do have
 * rows get (the two paths differ in their halo exchanges: all ranks must take the same one), nothing is written except zero
 * alpha gradients. */
int gaib_gat_forward_fused_rect(gaib_ctx* ctx, gaib_graph* g, int len, int heads, const float* d_tab, const float* d_alpha_l,
                                const float* d_alpha_r, float epsilon, int relu, float* d_out, float* d_row_stats, int phase);
int gaib_gat_backward_rec(gaib_ctx* ctx, int64_t nv, int len, int heads, const float* d_grad, const float* d_fwd_out,
                          const float* d_row_stats, float* d_rec);
int gaib_gat_backward_fused_rect(gaib_ctx* ctx, gaib_graph* g, int len, int heads, const float* d_feat_tab,
                                 const float* d_grad_tab, const float* d_rec_tab, const float* d_alpha_l,
                                 const float* d_alpha_r, float epsilon, float* d_grad_out, float* d_alpha_lgrad,
                                 float* d_alpha_rgrad, int phase);
/* GAT backward on a RECTANGULAR graph (a rank's rows over [owned | halo] columns), where the reverse
 * edge of (i -> c) lives on another rank and the reverse-edge permutation is replaced by the rank's transposed local
 * structure (rows = owned + halo vertices, columns = owned rows; include/gnn/partition.h).  gaib_gat_scores_mh and
 * gaib_sddmm_mh take rectangular graphs as they are (d_h / d_feat = the [nc x len] column table).
 *   gaib_gat_softmax_bwd_rows: the row side of gat_aggregator.cpp:121-167 -- g_e = d(softmax) * leaky-relu' into
 *     d_g_out [ne][heads], its row sums into d_rs_out [nv][heads];
 *   gaib_edge_gather_perm: d_out_e[k] = d_in_e[perm[k]] for [ne][heads] edge arrays (g and p in transposed order);
 *   gaib_edge_rowsum: d_out_rows[v] = sum of an edge array over row v (column sums of g = row sums over the transpose);
 *   gaib_gat_alpha_grads: alpha_l' = sum_v rs[v] x[v], alpha_r' = sum_v cs[v] x[v] over nv rows (graph_operations.h:
 *     396-467 regrouped by vertex; fixed two-level reduction, no atomics).
 * The transposed aggregation is gaib_spmm_mh on the transposed graph followed by gaib_halo_reduce. */
int gaib_gat_softmax_bwd_rows(gaib_ctx* ctx, gaib_graph* g, int heads, const float* d_norm_scores,
                              const float* d_norm_scores_grad, const float* d_temp_scores, float epsilon,
                              float* d_g_out, float* d_rs_out);
int gaib_edge_gather_perm(gaib_ctx* ctx, int64_t ne, int heads, const uint32_t* d_perm, const float* d_in_e,
                          float* d_out_e);
int gaib_edge_rowsum(gaib_ctx* ctx, gaib_graph* g, int heads, const float* d_in_e, float* d_out_rows);
int gaib_gat_alpha_grads(gaib_ctx* ctx, int64_t nv, int len, int heads, const float* d_x, const float* d_rs,
                         const float* d_cs, float* d_alpha_lgrad, float* d_alpha_rgrad);
/* symmetric_csr_transpose (math_functions.cpp:46-74; csr2csc math_functions.cu:345-358):
 *   d_out_e[rev(e)] = d_in_e[e].  The reverse-edge permutation is built once per graph. */
int gaib_edge_transpose(gaib_ctx* ctx, gaib_graph* g, const float* d_in_e, float* d_out_e);

/* ---- row classes of a vertex-range partition ---------------------------------------------------------
 * The reference partitioner's local graph marks the owned (master) rows and appends the halo vertices behind them
 * (src/partitioner/graph_partition.cc:70-80,128-178, include/graph_partition.h:21-22,36-37).  An owned row whose edges all
 * stay inside the range -- an INTERIOR row -- needs nothing from the exchange; only BOUNDARY rows wait for the halo rows.
 * gaib_graph_split_classes cuts a rank's owned-column graph and halo-column graph (same rows, gaib_graph_set_vertex_norm
 * applied to both) into class graphs.  Each is COMPACT -- row k is the k-th row of the class, ascending -- and carries a
 * row map: every aggregation entry point (gaib_spmm*, gaib_spmm_gemm*) treats row k of such a graph as row map[k] of its
 * [n_rows x len] output / partial-sum / rows2 matrices, so the classes of one partition fill disjoint rows of the same
 * matrices.  Edge order inside a row is kept: the sums are those of the graphs the classes were cut from.
 *   *interior : rows without halo-column edges                               columns: owned
 *   *bnd_own  : the boundary rows' owned-column edges                        columns: owned
 *   *bnd_halo : the boundary rows' halo-column edges                         columns: halo
 *   *bnd_full : both, per row [owned-column ..., halo-column ...]              columns: [owned | halo]: halo id + n_own
 * Any of the four out pointers may be NULL (not built).  h_n_boundary / h_boundary_edges (optional): boundary rows and
 * their edges.  Class graphs take GAIB_W_GCN / _MEAN / _MEAN_T / single-head _EDGE weights.
 * flags: GAIB_SPLIT_ALL_BOUNDARY = every row counts as a boundary row (*interior gets no rows): where next to no row is
 * interior, one pass over all rows of bnd_full beats two launches. */
#define GAIB_SPLIT_ALL_BOUNDARY 1
int gaib_graph_split_classes(gaib_ctx* ctx, const gaib_graph* g_own, const gaib_graph* g_halo, gaib_graph** interior,
                             gaib_graph** bnd_own, gaib_graph** bnd_halo, gaib_graph** bnd_full, int64_t* h_n_boundary,
                             int64_t* h_boundary_edges, int flags);
/* ---- pieces of a halo-column graph (round 6; the exchange in time slices: gaib_halo_set_pieces below) ------------------
 * Cuts a rank's halo-column graph (gaib_graph_create_rect + gaib_graph_set_vertex_norm; also a *bnd_halo row class) into
 * n_pieces graphs over the SAME rows, column space and normalisers: piece k holds, row by row and in the row's edge order,
 * the edges whose column lies in one of piece k's column ranges -- range j = [h_range_begin[j], h_range_end[j]) of the
 * column space belongs to piece h_range_piece[j]; ranges are disjoint and every edge's column lies in one (else
 * GAIB_ERR_INVALID).  With the ranges of gaib_halo_piece_ranges, piece k reads exactly the rows of the halo table that have
 * landed after gaib_halo_exchange_wait_piece(k): aggregate piece 0, 1, ... in GAIB_ACCUMULATE mode as they arrive (the last
 * one may carry the dense product) -- a row's terms are then added piece by piece, inside a piece in column order: with ONE
 * peer the order of the uncut graph (same bits on rows below the heavy threshold), with several the piece-major order of
 * the same terms.  out: n_pieces graphs (the caller destroys each). */
#define GAIB_GRAPH_MAX_PIECES 16
int gaib_graph_split_pieces(gaib_ctx* ctx, const gaib_graph* g, int n_pieces, int n_ranges, const int64_t* h_range_begin,
                            const int64_t* h_range_end, const int* h_range_piece, gaib_graph** out);
/* the row map by hand (uint32 [nv] device array, copied; n_out_rows = rows of the matrices it indexes; NULL removes it) */
int gaib_graph_set_row_map(gaib_ctx* ctx, gaib_graph* g, const uint32_t* d_row_map, int64_t n_out_rows);
const uint32_t* gaib_graph_row_map(const gaib_graph* g); /* device, uint32[nv], or NULL */
/* Aggregation over TWO feature tables: column ids below n_first index d_in, the others d_in2 (row id - n_first) -- a
 * rank's own rows and the halo table behind them, two allocations read side by side in one pass over [owned | halo]
 * (bnd_full above, n_first = n_own).  Otherwise gaib_spmm_ex / gaib_spmm_gemm(2) (d_rows2 / d_W2: both or NULL). */
int gaib_spmm_2t(gaib_ctx* ctx, gaib_graph* g, int weight_kind, const float* d_edge_w, int len, const float* d_in,
                 const float* d_in2, int64_t n_first, float* d_out, int flags);
int gaib_spmm_gemm_2t(gaib_ctx* ctx, gaib_graph* g, int weight_kind, const float* d_edge_w, int len_in, const float* d_in,
                      const float* d_in2, int64_t n_first, float* d_agg, const float* d_W, int transW, const float* d_rows2,
                      const float* d_W2, int len_out, float* d_out, int flags);
/* 1 if gaib_spmm_gemm(2) would run this shape as ONE kernel (shape only: widths, weight kind, the option "spmm_fuse").
 * The classes of a partition fill one output: all of them take the fused kernel or none does -- on a class graph
 * gaib_spmm_gemm* returns GAIB_ERR_UNSUPPORTED for a shape this says 0 to, and the caller aggregates class by class
 * and multiplies all rows at once. */
int gaib_spmm_gemm_fusable(gaib_ctx* ctx, int weight_kind, int len_in, int len_out, int dual);

/* ---- aggregation fused with the dense product: the `din <= dout` branch of the layers
 * (gcn_layer.cpp:19-24, sage_layer.cpp:25-34): agg = A.in (gaib_spmm semantics, [nv x len_in]),
 * out = act(agg . op(W)), op(W) = W [len_in x len_out] or, with transW, W^T for W [len_out x len_in]
 * (the input-gradient product of backward).  For len_in in {64, 128} and len_out % 16 == 0 the product
 * runs on the matrix cores inside the aggregating wave (no second pass over agg); other shapes run
 * gaib_spmm + gaib_sgemm.  flags: GAIB_RELU, GAIB_AGG_SCRATCH, GAIB_ACCUMULATE (d_agg holds partial sums that
 * this call continues -- the halo half of a partitioned aggregation).  d_agg must always be a valid
 * [nv x len_in] buffer.  Option "spmm_fuse" = 0 forces the two-kernel path. */
int gaib_spmm_gemm(gaib_ctx* ctx, gaib_graph* g, int weight_kind, const float* d_edge_w,
                   int len_in, const float* d_in, float* d_agg, const float* d_W, int transW,
                   int len_out, float* d_out, int flags);

/* the same with a second, row-local product in the store: out = act(agg . op(W) + rows2 . op(W2)), rows2 [nv x len_in],
 * W2 shaped like W -- the self term of a SAGE layer (sage_layer.cpp:22 forward, :50 backward) without its own pass. */
int gaib_spmm_gemm2(gaib_ctx* ctx, gaib_graph* g, int weight_kind, const float* d_edge_w,
                    int len_in, const float* d_in, float* d_agg, const float* d_W, int transW,
                    const float* d_rows2, const float* d_W2, int len_out, float* d_out, int flags);

/* gaib_spmm_gemm / gaib_spmm_gemm2 over a bf16 table: d_in is [nc x len_in] bf16 bits (row-major, as gaib_spmm_bf16);
 * d_agg, d_W, d_rows2, d_W2 and d_out are fp32.  flags: GAIB_RELU, GAIB_AGG_SCRATCH, GAIB_ACCUMULATE.
 * d_agg (unless GAIB_AGG_SCRATCH) and d_out are BIT-IDENTICAL to gaib_spmm_gemm(2) called with the same arguments and options
 * on the table widened to fp32 (gaib_cast_bf16_f32), for d_in 8-B aligned and d_agg 16-B aligned: the call takes the route
 * the fp32 call would take on that table -- the fused kernel, two 128-column K-slabs, the neighbour product fused and the self
 * term as an accumulating GEMM, ordered chunks + gaib_sgemm_ex on a dense graph, gaib_spmm_bf16 + gaib_sgemm_ex on a shape that
 * does not fuse or with "spmm_fuse" = 0 -- and runs it with a bf16 gather (half the gathered bytes; widened exactly in
 * registers, no fp32 copy of the table).  Partial sums, op(W), the product and all stores are fp32.
 * A graph with a row map (a row class of a partition): GAIB_ERR_UNSUPPORTED; GAIB_OVERLAPS_TRANSFER: GAIB_ERR_INVALID
 * (partitions aggregate fp32 tables).  A table of >= 4 GB in bf16 is gathered with 64-bit addresses. */
/* gaib_spmm_gemm / gaib_spmm_gemm2 gathering from the zero-suppressed image d_zs of d_in (gaib_pack_zs over the same g->nc rows):
 * three 128-byte lines per gathered row instead of four.  Masked columns enter every row sum as w * (+0.0), in the order of the
 * dense call: d_agg (unless GAIB_AGG_SCRATCH) and d_out are bit-identical to gaib_spmm_gemm(2) on d_in, which stays the source of
 * over-capacity rows.  Covers the one-launch fused route of a whole graph: len_in == 128, GCN / MEAN / MEAN_T / single-head EDGE
 * weights, op(W) in LDS beside 8-row strips (one product) or two products that fit LDS together, a table below 4 GB, "spmm_addr_mode" != 2,
 * and a graph the dense call runs in its row form off the global tile counter (not the edge stream of short rows -- fewer than 12
 * edges per row, or "spmm_flat" = 1 --, not the XCD-affine supply of a numbering with locality).  Anything
 * else -- another width, a graph with a row map, a dense graph the ordered chunks would take, "spmm_fuse" = 0 -- returns
 * GAIB_ERR_UNSUPPORTED before anything is launched: call the dense function.
 * len_in == 256 with d_zs a WIDE image (gaib_pack_zs_wide): covers the K-slab route the dense call takes at that width -- whole
 * graph, "spmm_fuse" != 0, not the ordered chunks, a [len_out x 128] slab of op(W) in LDS beside 8- or 2-row strips -- under the
 * same conditions (row form: 12 edges per row or "spmm_flat" = 0; global tile counter; table below 4 GB; "spmm_addr_mode" != 2;
 * image 128-B aligned).  Each slab launch gathers its slab's image, three lines per half row instead of four; with two products
 * the self term follows as the dense route's accumulating gaib_sgemm_ex.  Same bit-identity contract.  Widths 129 .. 255 are
 * refused: a second slab narrower than 128 columns has no packed form. */
/* gaib_spmm_gemm_zs_route: would the packed call (two products when d_rows2 != NULL) be taken?  GAIB_OK or GAIB_ERR_UNSUPPORTED
 * from the route information alone -- nothing is launched or read: ask before packing. */
int gaib_spmm_gemm_zs_route(gaib_ctx* ctx, gaib_graph* g, int weight_kind, int len_in, const float* d_in, const void* d_zs,
                            float* d_agg, const float* d_rows2, int len_out, float* d_out);
int gaib_spmm_gemm_zs(gaib_ctx* ctx, gaib_graph* g, int weight_kind, const float* d_edge_w, int len_in, const float* d_in,
                      const void* d_zs, float* d_agg, const float* d_W, int transW, int len_out, float* d_out, int flags);
int gaib_spmm_gemm2_zs(gaib_ctx* ctx, gaib_graph* g, int weight_kind, const float* d_edge_w, int len_in, const float* d_in,
                       const void* d_zs, float* d_agg, const float* d_W, int transW, const float* d_rows2, const float* d_W2,
                       int len_out, float* d_out, int flags);

int gaib_spmm_gemm_bf16(gaib_ctx* ctx, gaib_graph* g, int weight_kind, const float* d_edge_w, int len_in,
                        const uint16_t* d_in, float* d_agg, const float* d_W, int transW, int len_out, float* d_out,
                        int flags);
int gaib_spmm_gemm2_bf16(gaib_ctx* ctx, gaib_graph* g, int weight_kind, const float* d_edge_w, int len_in,
                         const uint16_t* d_in, float* d_agg, const float* d_W, int transW, const float* d_rows2,
                         const float* d_W2, int len_out, float* d_out, int flags);
/* ... over d_in = [nc x ld] bf16 bits (the contract of gaib_spmm_bf16_ld: ld == len_in, or ld > len_in with ld % 4 == 0): the
 * route -- fused, K-slabs, fused + accumulating GEMM, ordered chunks, two kernels, the edge stream -- is the dense call's, chosen
 * on len_in; d_agg and d_out are bit-identical to it, the columns behind len_in reach no output. */
int gaib_spmm_gemm_bf16_ld(gaib_ctx* ctx, gaib_graph* g, int weight_kind, const float* d_edge_w, int len_in, int64_t ld,
                           const uint16_t* d_in, float* d_agg, const float* d_W, int transW, int len_out, float* d_out,
                           int flags);
int gaib_spmm_gemm2_bf16_ld(gaib_ctx* ctx, gaib_graph* g, int weight_kind, const float* d_edge_w, int len_in, int64_t ld,
                            const uint16_t* d_in, float* d_agg, const float* d_W, int transW, const float* d_rows2,
                            const float* d_W2, int len_out, float* d_out, int flags);
/* ---- fp8 feature tables with per-row scales (opt-in) ----
 * Elements: OCP e4m3 "fn", the encoding of torch.float8_e4m3fn -- 1-4-3, bias 7, largest finite 448, no infinities, NaN = 0x7f /
 * 0xff.  A table is raw uint8_t [rows x ld], ld the row stride in BYTES, with a float [rows] array of row scales next to it.
 * gaib_fp8_row_stride (pure: no device, no graph): *ld = len where len % 128 == 0; else the next power of two >= max(len, 4) for
 * len <= 128; else len rounded up to a multiple of 128.  With the table on a 128-byte boundary no row of <= 128 columns
 * straddles a 128-byte line and wider rows start on one.
 * gaib_cast_f32_fp8_rows: d_in dense fp32 [rows x len] -> d_q [rows x ld] (ld >= len, ld % 4 == 0, d_q 4-byte aligned) and
 * d_scale [rows].  scale[r] is exactly 2^k, k the smallest integer with amax(r) * 2^-k <= 448, clamped to [-126, 120]; amax is
 * taken over the row's finite elements; k = 0 for a row with no non-zero finite element.  The element stored is x * 2^-k (exact)
 * rounded to nearest, ties to even; a magnitude still above 448 saturates to +-448; a NaN stays a NaN of its sign; +-inf
 * becomes the NaN of its sign (the format has no infinity).  Pad bytes (columns len .. ld - 1) are written as 0.  One kernel,
 * no host wait, no allocation: legal inside a stream capture.
 * gaib_cast_fp8_f32_rows: the widening, dense [rows x len] output: out[r][c] = f32(q[r][c]) * scale[r]; both steps are exact.
 * gaib_spmm_fp8: gaib_spmm_ex over such a table -- flags GAIB_ACCUMULATE | GAIB_RELU, the five single-head weight kinds, square
 * and rectangular graphs, any len >= 1.  d_out is BIT-IDENTICAL to gaib_spmm_ex on the widened table (gaib_cast_fp8_f32_rows),
 * for every row, while w_e * scale[col_e] and the products stay normal fp32 numbers: the scale of an edge's column is multiplied
 * into the edge's weight -- an exact product that commutes with the rounding of w * x --, everything after the gather is the fp32
 * kernels' own (edge order, separate multiply and add, heavy threshold, the 16-wave combine, the ordered-chunk rule decided on
 * the fp32 sizes).  Where the product w_e * scale[col_e] or a term leaves the normal range (an under- or overflow the fp32 call on
 * the widened table would meet at another point), the results may differ.  Profile keys spmm_fp8_light / _heavy / _chunk.
 * gaib_spmm_gemm_fp8 / gaib_spmm_gemm2_fp8: gaib_spmm_gemm / gaib_spmm_gemm2 over such a table (the arguments of the bf16 _ld
 * calls with d_q, d_scale in place of the bf16 table): the route is the fp32 call's on the widened table, every route test made
 * on the fp32 sizes; d_agg (unless GAIB_AGG_SCRATCH) and d_out bit-identical to it under the same condition.  Profile key
 * spmm_gemm_fp8_fused.
 * Refused with GAIB_ERR_UNSUPPORTED, a message and nothing touched: a graph with a row map (a row class of a partition), a table
 * of 4 GB or more (buffer addressing only), a table not on a 16-byte boundary.  The calls take no head count: multi-head weights
 * have no fp8 form.  Two-table gathers and zero-suppressed tables have none either. */
int gaib_fp8_row_stride(int len, int64_t* ld);
int gaib_cast_f32_fp8_rows(gaib_ctx* ctx, int64_t rows, int len, const float* d_in, int64_t ld, uint8_t* d_q, float* d_scale);
int gaib_cast_fp8_f32_rows(gaib_ctx* ctx, int64_t rows, int len, int64_t ld, const uint8_t* d_q, const float* d_scale, float* d_out);
int gaib_spmm_fp8(gaib_ctx* ctx, gaib_graph* g, int weight_kind, const float* d_edge_w, int len, int64_t ld, const uint8_t* d_q,
                  const float* d_scale, float* d_out, int flags);
int gaib_spmm_gemm_fp8(gaib_ctx* ctx, gaib_graph* g, int weight_kind, const float* d_edge_w, int len_in, int64_t ld,
                       const uint8_t* d_q, const float* d_scale, float* d_agg, const float* d_W, int transW, int len_out,
                       float* d_out, int flags);
int gaib_spmm_gemm2_fp8(gaib_ctx* ctx, gaib_graph* g, int weight_kind, const float* d_edge_w, int len_in, int64_t ld,
                        const uint8_t* d_q, const float* d_scale, float* d_agg, const float* d_W, int transW, const float* d_rows2,
                        const float* d_W2, int len_out, float* d_out, int flags);
/* bf16 tables on the row classes of a vertex-range partition (the functions above keep their refusals; the capability has
 * names of its own).  d_in / d_in2 hold bf16 bits, everything else is fp32.
 * gaib_spmm_part_bf16: with d_in2 == NULL gaib_spmm_ex on a bf16 table (n_first is ignored), with d_in2 != NULL gaib_spmm_2t on
 * two bf16 tables (column ids >= n_first index d_in2); graphs with or without a row map; flags GAIB_ACCUMULATE | GAIB_RELU.
 * gaib_spmm_gemm_part_bf16: gaib_spmm_gemm_2t on bf16 tables (d_in2 may be NULL, d_rows2 / d_W2 both or NULL), with all of its
 * flags -- GAIB_RELU, GAIB_AGG_SCRATCH, GAIB_ACCUMULATE, GAIB_OVERLAPS_TRANSFER.  On a class graph a shape that
 * gaib_spmm_gemm_fusable says 0 to returns GAIB_ERR_UNSUPPORTED, exactly where the fp32 call does.
 * Every route decision is made on the fp32 sizes, and everything after the gather -- the row map, weights, CSR order with
 * separate multiply and add, the heavy threshold and its combine order, the GAIB_ACCUMULATE continuation, the product -- is the
 * fp32 class kernels' own: d_out (and d_agg unless GAIB_AGG_SCRATCH) are BIT-IDENTICAL to gaib_spmm_ex / gaib_spmm_2t /
 * gaib_spmm_gemm(2) / gaib_spmm_gemm_2t on the tables widened to fp32 (gaib_cast_bf16_f32), for bf16 tables aligned to 8 B and
 * d_out / d_agg to 16.  Tables of >= 4 GB in bf16 (either one) are gathered with 64-bit addresses. */
int gaib_spmm_part_bf16(gaib_ctx* ctx, gaib_graph* g, int weight_kind, const float* d_edge_w, int len, const uint16_t* d_in,
                        const uint16_t* d_in2, int64_t n_first, float* d_out, int flags);
int gaib_spmm_gemm_part_bf16(gaib_ctx* ctx, gaib_graph* g, int weight_kind, const float* d_edge_w, int len_in,
                             const uint16_t* d_in, const uint16_t* d_in2, int64_t n_first, float* d_agg, const float* d_W,
                             int transW, const float* d_rows2, const float* d_W2, int len_out, float* d_out, int flags);

/* ---- dense update: matmul -> sgemm_gpu -> cublasSgemm (math_functions.cu:321-343) --------
 * row-major C[M x N] = op(A)[M x K] . op(B)[K x N]  (+ C if accum).  fp32 MFMA. */
int gaib_sgemm(gaib_ctx* ctx, int transA, int transB, int64_t M, int64_t N, int64_t K,
               const float* d_A, const float* d_B, int accum, float* d_C);
/* flags = GAIB_ACCUMULATE | GAIB_RELU (activation fused into the epilogue) */
int gaib_sgemm_ex(gaib_ctx* ctx, int transA, int transB, int64_t M, int64_t N, int64_t K,
                  const float* d_A, const float* d_B, int flags, float* d_C);

/* ---- dense product on a bf16 table with exactly split fp32 weights (gemm_bf16.hip) ----
 * C[M x N] (=|+=) A . op(B), A = bf16 bits [M x K] at row stride lda (elements), B fp32 ([K x N], or [N x K] with transB),
 * C fp32 [M x N] dense; flags = GAIB_ACCUMULATE | GAIB_RELU as gaib_sgemm_ex.
 * op(B) is split ON THE DEVICE, on every call (weights change every step), into three bf16 planes: w0 = rne(B), w1 = rne(B - w0),
 * w2 = rne(B - w0 - w1), rne = gaib_cast_f32_bf16's rounding; w0 + w1 + w2 == B exactly.  The split is part of the kernel: no
 * host synchronisation, no workspace, safe inside gaib_capture_begin/end.  Every A[i][k] . w_t[k][j] is exact in fp32 and
 * enters an fp32 accumulator of the bf16 matrix cores: the result is a sum of 3 K exact terms (+ C when accumulating) in an
 * unspecified order -- the rounding of an fp32 product's accumulation, not bit-identical to any fp32 call; deterministic from
 * run to run (no atomics, no split over K).  Finite inputs only: a +-inf in the table meets zero residual terms and gives NaN
 * where fp32 gives +-inf.  |B| below about 2^-100 loses its low bits (the residuals underflow bf16's range).
 * Subnormal bf16 table entries, subnormal plane values, subnormal fp32 results and C inputs are all kept, not flushed (measured on
 * the MI355X: the bf16 MFMA takes 2^-133 x 2^100 to 2^-33).
 * Cover: 8 <= K <= 256, K % 8 == 0; 4 <= N <= 256, N % 4 == 0; lda >= K, lda % 8 == 0 (and lda <= 2^22); d_A_bf16 and d_C on
 * 16-byte boundaries; any M >= 0 (M == 0: GAIB_OK, nothing launched); option "gemm_bf16_kernel" = 1.  Anything else:
 * GAIB_ERR_UNSUPPORTED with nothing written -- the caller falls back to gaib_sgemm_ex.  Columns K .. lda - 1 of a row are
 * never read.  The table is read through per-tile buffer descriptors: 4 GB and more need no other path.
 * Profile: key "gemm_bf16", tag MxNxK; bytes 2 M K + 4 M N (1 + accum) + 4 K N, flops 2 M N K (the useful ones, not x 3). */
int gaib_gemm_bf16(gaib_ctx* ctx, int transB, int64_t M, int N, int K, int64_t lda, const uint16_t* d_A_bf16,
                   const float* d_B, int flags, float* d_C);
/* 1 when the call above would run (shape, stride and option "gemm_bf16_kernel" only; no pointer, no launch), else 0 */
int gaib_gemm_bf16_cover(gaib_ctx* ctx, int transB, int N, int K, int64_t lda);

/* weight gradient with the layer's d_relu folded in (d_relu_gpu on grad_in followed by matmul(transA),
 * gcn_layer.cpp:33-52): d_G <- d_G where d_mask > 0 else 0 (IN PLACE, what d_relu_gpu leaves behind) and
 * C[M x N] (=|+=) A^T . G for A [K x M], G / mask [K x N].  One pass over G instead of two. */
int gaib_sgemm_drelu(gaib_ctx* ctx, int64_t M, int64_t N, int64_t K, const float* d_A, float* d_G,
                     const float* d_mask, int accum, float* d_C);

/* ---- elementwise: relu_gpu / d_relu_gpu (math_functions.cu:242-268), dropout mask replay
 * d_dropout_gpu (:134-146) ---- */
int gaib_relu(gaib_ctx* ctx, int64_t n, const float* d_in, float* d_out);
int gaib_d_relu(gaib_ctx* ctx, int64_t n, const float* d_in_diff, const float* d_data,
                float* d_out_diff);
int gaib_dropout(gaib_ctx* ctx, int64_t n, float scale, float drop_rate, uint64_t seed,
                 const float* d_in, uint8_t* d_masks, float* d_out);
int gaib_d_dropout(gaib_ctx* ctx, int64_t n, float scale, const float* d_in,
                   const uint8_t* d_masks, float* d_out);
/* gaib_dropout with the mask seed in device memory: with s = *d_seed when the call's kernel runs on the context's stream, d_masks
 * and d_out hold the bits gaib_dropout(ctx, n, scale, drop_rate, s, ..) writes; behind the draw, in stream order, *d_seed becomes
 * s + 1 (mod 2^64) -- once per call, for n == 0 too (the host's `seed++`).  No host wait, no allocation: legal inside
 * gaib_capture_begin/end, and every replay draws the next seed.  d_out == d_in is allowed.  d_seed is always required and
 * 8-byte aligned (GAIB_ERR_INVALID before any launch otherwise); the rate lies in [0, 1).  d_in / d_out on 16 B and d_masks on
 * 4 B run 16-byte lanes, any other alignment one element per lane. */
int gaib_dropout_dev(gaib_ctx* ctx, int64_t n, float scale, float drop_rate, uint64_t* d_seed,
                     const float* d_in, uint8_t* d_masks, float* d_out);

/* bias_mv (include/utils/math_functions.hh:36; math_functions.cu:207-221): x[i, j] += b[j] for x [n x len] */
int gaib_bias_add(gaib_ctx* ctx, int64_t n, int len, float* d_x, const float* d_b);
/* reduce_sum (math_functions.hh:37-38; math_functions.cpp:246-262, .cu:224-238): a[j] = sum_i x[i, j], overwritten.
 * Deterministic (two levels in a fixed order; the reference's CUDA kernel adds into a[j] from all threads unguarded). */
int gaib_colsum(gaib_ctx* ctx, int64_t n, int len, const float* d_x, float* d_a);
/* rng_uniform_gpu / gpu_rng_uniform (math_functions.hh:156,174; math_functions.cu:39-50): r[i] uniform on [a, b) from the
 * library's counter RNG (element i of stream `seed`).  The reference draws cuRAND XORWOW numbers: streams differ. */
int gaib_rng_uniform(gaib_ctx* ctx, int64_t n, float a, float b, uint64_t seed, float* d_r);
/* csr2csc (math_functions.hh:45; cusparseCsr2cscEx2, math_functions.cu:345-358): the transpose of a general
 * [nrows x ncols] CSR matrix with 32-bit offsets, all arrays in device memory: d_rowptrT [ncols + 1], d_colidxT [nnz]
 * (row ids, ascending inside a column), d_valuesT [nnz] (d_values / d_valuesT may both be NULL: structure only).  Syncs. */
int gaib_csr2csc(gaib_ctx* ctx, int nrows, int ncols, int nnz, const float* d_values, const int* d_rowptr,
                 const int* d_colidx, float* d_valuesT, int* d_rowptrT, int* d_colidxT);

/* ---- loss / metrics: softmax_cross_entropy_gpu, d_softmax_cross_entropy_gpu,
 * masked_avg_loss_gpu, masked_accuracy_single (math_functions.cu:516-564,749-761,886-942) ---- */
int gaib_softmax_xent(gaib_ctx* ctx, int num_cls, int64_t begin, int64_t end,
                      const float* d_in, const uint8_t* d_masks, const uint8_t* d_labels,
                      float* d_loss, float* d_out);
int gaib_d_softmax_xent(gaib_ctx* ctx, int num_cls, int64_t begin, int64_t end,
                        const uint8_t* d_masks, const uint8_t* d_labels, const float* d_out,
                        float* d_diff);
/* multi-label head: sigmoid + cross entropy with [n x num_cls] 0/1 labels, its gradient, and the micro F1
 * that masked_accuracy_multi returns (src/layers/sigmoid_loss_layer.cpp:4-33, sigmoid_loss_layer.cu:4-17,
 * math_functions.cpp:517-521,553-559,580-621; math_functions.cu:583-637,944-1044).  Vertices of the range that
 * the mask excludes get loss 0; h_counts (optional) receives tp, fp, fn. */
int gaib_sigmoid_xent(gaib_ctx* ctx, int num_cls, int64_t begin, int64_t end,
                      const float* d_in, const uint8_t* d_masks, const uint8_t* d_labels,
                      float* d_loss, float* d_out);
int gaib_d_sigmoid_xent(gaib_ctx* ctx, int num_cls, int64_t begin, int64_t end,
                        const uint8_t* d_masks, const uint8_t* d_labels,
                        const float* d_out, float* d_diff);
int gaib_masked_f1_micro(gaib_ctx* ctx, int64_t begin, int64_t end, int num_cls,
                         const uint8_t* d_masks, const float* d_preds, const uint8_t* d_labels,
                         float* h_result, int64_t* h_counts);
int gaib_masked_avg_loss(gaib_ctx* ctx, int64_t begin, int64_t end, const uint8_t* d_masks,
                         const float* d_loss, float* h_result); /* syncs */
int gaib_masked_accuracy_single(gaib_ctx* ctx, int64_t begin, int64_t end, int num_cls,
                                const uint8_t* d_masks, const float* d_preds,
                                const uint8_t* d_labels, float* h_result); /* syncs */
/* The same reductions with the result left in DEVICE memory (d_result[0]; d_counts[3] = tp, fp, fn): no host wait,
 * so they can be part of a recorded sequence (gaib_capture_begin).  Block partials are added in the order of the
 * host forms: identical bits. */
int gaib_masked_avg_loss_dev(gaib_ctx* ctx, int64_t begin, int64_t end, const uint8_t* d_masks,
                             const float* d_loss, float* d_result);
int gaib_masked_accuracy_single_dev(gaib_ctx* ctx, int64_t begin, int64_t end, int num_cls,
                                    const uint8_t* d_masks, const float* d_preds,
                                    const uint8_t* d_labels, float* d_result);
int gaib_masked_f1_counts_dev(gaib_ctx* ctx, int64_t begin, int64_t end, int num_cls,
                              const uint8_t* d_masks, const float* d_preds, const uint8_t* d_labels,
                              uint64_t* d_counts);

/* ---- l2norm / d_l2norm (math_functions.cu:158-196) ---- */
int gaib_l2norm(gaib_ctx* ctx, int64_t n, int dim, const float* d_in, float* d_out);
int gaib_d_l2norm(gaib_ctx* ctx, int64_t n, int dim, const float* d_feat_in,
                  const float* d_grad_in, float* d_grad_out);

/* ---- optimizer: adam::update_gpu -> update_kernel (src/utilities/optimizer.cu:5-36).
 * The caller owns m/v state and the beta powers (optimizer.h:99-116). ---- */
int gaib_adam_step(gaib_ctx* ctx, int64_t n, const float* d_dW, float* d_W, float* d_m,
                   float* d_v, float alpha, float b1, float b2, float b1_t, float b2_t, float eps);
/* The same step with the beta powers in device memory: d_pow[0] = b1^t, d_pow[1] = b2^t are read by the step and
 * then advanced ON THE DEVICE (the host's `b1_t *= b1; b2_t *= b2`, optimizer.cpp:34-35 -- the same float products),
 * so a recorded step replays correctly.  Initialise d_pow to {b1, b2}. */
int gaib_adam_step_dev(gaib_ctx* ctx, int64_t n, const float* d_dW, float* d_W, float* d_m, float* d_v,
                       float alpha, float b1, float b2, float eps, float* d_pow);

/* ---- multi-GPU helpers (no reference counterpart) --------------------------
 * pack rows for the halo exchange: d_out[k,:] = d_in[d_idx[k],:] */
int gaib_gather_rows(gaib_ctx* ctx, int64_t n_idx, const int64_t* d_idx, int len,
                     const float* d_in, float* d_out);
/* the same for rows of width_bytes bytes (label rows: 1 byte single-class, one byte per class multi-label); any width >= 1,
 * no alignment beyond one byte asked of d_in or d_out */
int gaib_gather_rows_u8(gaib_ctx* ctx, int64_t n_idx, const int64_t* d_idx, int width_bytes, const uint8_t* d_in,
                        uint8_t* d_out);
/* out[dst_idx[k], :] = in[src_idx[k], :], dst rows distinct.  The halo plans pack with it in SOURCE order (src ascending):
 * a row that goes to several peers is read from HBM once (its repeats hit the cache) instead of once per peer. */
int gaib_gather_scatter_rows(gaib_ctx* ctx, int64_t n_idx, const int64_t* d_src_idx, const int64_t* d_dst_idx, int len,
                             const float* d_in, float* d_out);

/* ---- collectives of the vertex-range partitioned path ("halo_exchange(handle,D,buf)",
 * "allreduce(buf,n)"; 8e) -------------------------------------------------------------------------------------
 * One process per GPU.  The reference has no multi-GPU GNN; the partition scheme is its
 * PartitionedGraph::edgecut_induced_partition1D (src/partitioner/graph_partition.cc:128-178), the host pattern it uses
 * for multi-GPU work is one host thread per device with peer copies (src/triangle/multigpu_induced.cu:31-84).
 *
 * Transports:
 *   GAIB_COMM_RCCL  RCCL (ncclSend/ncclRecv groups, ncclAllReduce) on a communication stream; ONE GPU PER RANK
 *                   (RCCL refuses two ranks on one device: gaib_comm_init then fails on every rank); stream-ordered.
 *   GAIB_COMM_IPC   peer-to-peer pull through hipIpc handles published in POSIX shared memory (one node; xGMI
 *                   between GPUs, plain device copies when ranks share a GPU -- tests); host-synchronous hand-overs.
 *                   A send buffer above GAIB_IPC_CHUNK_BYTES (default 512 MiB) is cut into separately exported chunks
 *                   of whole rows (at most 64): hipIpcOpenMemHandle does not return for allocations above 2 GiB.  No
 *                   allocation above GAIB_IPC_EXPORT_LIMIT_BYTES (1.5 GiB) is exported: GAIB_ERR_UNSUPPORTED instead
 *                   (gaib_halo_reduce stages its partial rows in chunks the same way).  GAIB_COMM_DEBUG=1 prints the steps
 *                   of every exchange with time stamps on stderr.
 * gaib_comm_unique_id is called by ONE rank; the caller carries the GAIB_COMM_ID_BYTES to the other ranks (a file,
 * MPI, torch.distributed's store ...).  gaib_comm_init is collective.  Every collective below must be called by
 * every rank in the same order.  A rank that fails or does not arrive within GAIB_COMM_TIMEOUT_S (default 120 s)
 * makes the waiting ranks return GAIB_ERR_COMM instead of hanging. */
typedef struct gaib_comm gaib_comm;
typedef struct gaib_halo gaib_halo;
#define GAIB_COMM_ID_BYTES 128
#define GAIB_COMM_RCCL 0
#define GAIB_COMM_IPC 1
/* local and cheap: GAIB_OK if this process can use the transport at all (RCCL: librccl.so.1 loads and has every entry
 * point used here).  What the ranks agree on -- together with "every rank has a device of its own" -- BEFORE any of
 * them enters gaib_comm_init(GAIB_COMM_RCCL): ncclCommInitRank is collective and has no deadline. */
int gaib_comm_transport_available(int transport);
int gaib_comm_unique_id(int transport, void* h_id);
int gaib_comm_init(gaib_ctx* ctx, int rank, int nranks, const void* h_id, int transport, gaib_comm** out);
int gaib_comm_destroy(gaib_comm* comm);
int gaib_comm_rank(const gaib_comm* comm);
int gaib_comm_size(const gaib_comm* comm); /* RCCL: what ncclCommCount reports for the communicator that was built */
int gaib_comm_barrier(gaib_comm* comm); /* syncs the compute stream first */
/* in-place sum over ranks on the context's stream: the weight / alpha gradients of a layer (<= 256 KB each);
 * every rank ends with the same bits */
int gaib_allreduce_f32(gaib_comm* comm, float* d_buf, int64_t n);
/* host scalars (masked loss sums, accuracy counts): in-place sum over ranks, n <= 1024; syncs */
int gaib_allreduce_host_f64(gaib_comm* comm, double* h_buf, int n);
/* A halo plan: which of this rank's rows go to which peer and how many rows arrive from each peer.
 *   h_send_counts[r] rows go to rank r: their local row ids are send_idx[sum(h_send_counts[:r]) ...] (host or device
 *   array, copied); h_recv_counts[r] rows arrive from rank r; both 0 for the rank itself.  The table an exchange fills
 *   is [sum(h_recv_counts) x len], grouped by source rank in rank order -- the order of the halo column ids of
 *   gaib_graph_create_rect's column space after the owned rows.  Collective (create and destroy, in the same order
 *   on every rank); at most 8 plans alive per communicator, a destroyed plan's slot is reused.  One plan serves any
 *   mix of row lengths and directions: its buffers grow as needed and peers re-map them when they do. */
int gaib_halo_create(gaib_comm* comm, const int64_t* h_send_counts, const int64_t* send_idx, int idx_on_device,
                     const int64_t* h_recv_counts, gaib_halo** out);
int gaib_halo_destroy(gaib_halo* halo);
int64_t gaib_halo_rows(const gaib_halo* halo);      /* rows of the halo table */
int64_t gaib_halo_send_rows(const gaib_halo* halo); /* rows this rank packs per exchange */
int64_t gaib_halo_link_rows(const gaib_halo* halo); /* the most rows one peer pair moves per exchange, either direction:
                                                      * what one xGMI link carries (every pair has its own) */
int64_t gaib_halo_bytes_sent(const gaib_halo* halo);
/* how the plan's rows left so far: exchanges that ran the pack kernel, sends that went STRAIGHT from the caller's matrix, and the
 * number of peers whose send list is one run of consecutive rows (RCCL transport: such a peer is sent from d_rows itself; if
 * every peer is, the plan never packs -- the N-way cut of a graph whose ranges need all of each other's rows) */
int gaib_halo_send_stats(const gaib_halo* halo, int64_t* h_packs, int64_t* h_direct_sends, int* h_direct_peers);
/* one exchange = begin (pack the requested rows of d_rows [n_own x len] on the compute stream, start moving them)
 * ... independent work on the compute stream (the owned-column edges of the aggregation) ... end (the compute stream
 * continues only after the halo rows have arrived; *d_table stays valid until the next begin on this plan).
 * d_rows must stay valid and UNMODIFIED until gaib_halo_exchange_end: over RCCL a peer whose send list is one run of
 * consecutive rows is sent straight from d_rows on the communication stream (gaib_halo_send_stats), not from a packed
 * copy.  (A plan that mixes direct and packed peers still packs -- and reserves buffer space for -- all of its rows.) */
int gaib_halo_exchange_begin(gaib_halo* halo, int len, const float* d_rows);
int gaib_halo_exchange_end(gaib_halo* halo, const float** d_table);
/* An exchange in K time slices ("pieces", round 6): slice k of a peer pair's R rows is rows [R k / K, R (k + 1) / K) of
 * that pair's segment (gaib_halo_piece_slice: sender and receiver cut the same R the same way), slice k of EVERY pair
 * travels together (one ncclGroup / one round of peer pulls), so every link is busy throughout and piece k has landed after
 * ~(k + 1) / K of the exchange.  Between begin and end, gaib_halo_exchange_wait_piece(k) makes the compute stream wait for
 * piece k only (stream-ordered, the host does not wait): the caller's halo-column pass over piece k's columns
 * (gaib_graph_split_pieces with gaib_halo_piece_ranges) then runs while the later slices are still on the wire.
 * gaib_halo_exchange_end stays due after the last piece.  The table's layout does not change with K.
 * gaib_halo_set_pieces: 1 <= n_pieces <= 16, THE SAME ON EVERY RANK (the peer-to-peer transport checks it, RCCL would
 * mismatch its counts), not while an exchange is in flight; default 1.  gaib_halo_piece_ranges: the column ranges
 * [begin, end) of the table that piece k fills (at most one per peer; h_n = how many, at most cap). */
int gaib_halo_set_pieces(gaib_halo* halo, int n_pieces);
/* the library's choice for a partition of n_global vertices into `world` ranges, a function of figures every rank holds (so
 * the ranks agree without a collective): GAIB_HALO_PIECES if set (1 .. 16), else 4 from 131 072 rows per range, 2 from
 * 32 768, else 1.  make_partitioned_graph and dist.py set it on their plans. */
int gaib_halo_default_pieces(int64_t n_global, int world);
int gaib_halo_pieces(const gaib_halo* halo);
int gaib_halo_piece_slice(int64_t rows, int n_pieces, int piece, int64_t* h_lo, int64_t* h_hi); /* pure arithmetic, no device */
int gaib_halo_piece_ranges(const gaib_halo* halo, int piece, int cap, int64_t* h_begin, int64_t* h_end, int* h_n);
int gaib_halo_exchange_wait_piece(gaib_halo* halo, int piece, const float** d_table);
/* The same exchange carrying bf16 rows (raw bits) of `len` elements: 2 * len bytes per row -- through the same pack, chunks,
 * direct sends, pieces and pulls (a bf16 row of even len is byte for byte an fp32 row of len / 2; over RCCL it travels as len / 2
 * ncclFloat32 words), so gaib_halo_bytes_sent counts half of the fp32 exchange of the same plan and len.  d_rows (4-byte aligned)
 * stays valid and unmodified until the end, as above.  An odd len: GAIB_ERR_UNSUPPORTED, decided locally before any collective
 * step -- the same on every rank, no exchange is left pending.  An exchange is ended / waited for with the functions of the
 * element type it was begun with: the other type is GAIB_ERR_INVALID and leaves the exchange in flight.  The peer-to-peer
 * transport publishes the row bytes and the element size and refuses a mismatch between peers (bf16 tables on some ranks only). */
int gaib_halo_exchange_begin_bf16(gaib_halo* halo, int len, const uint16_t* d_rows);
int gaib_halo_exchange_end_bf16(gaib_halo* halo, const uint16_t** d_table);
int gaib_halo_exchange_wait_piece_bf16(gaib_halo* halo, int piece, const uint16_t** d_table);

/* the reverse of an exchange: d_halo_rows [halo rows x len] (the table's layout) holds this rank's partial sums for its
 * HALO vertices; they travel back to the owners, which add them to their own rows: d_rows[send_idx[k], :] += arrived[k, :],
 * peer by peer in rank order (deterministic).  The transposed aggregation of GAT backward on a partition: the term
 * p_(i->c) * grad_i of a row i that another rank owns.  Collective; not while an exchange of the same plan is in flight. */
int gaib_halo_reduce(gaib_halo* halo, int len, const float* d_halo_rows, float* d_rows);

/* ---- in-stream kernel timing (measurement only) -----------------------------------------------
 * When enabled, the aggregation entry points bracket each kernel launch with a HIP event pair
 * on the context's stream (no host sync).  gaib_prof_get syncs the stream and returns the launch
 * count and summed device time for a key: "spmm_light", "spmm_heavy", "spmm_sub", "sgemm". */
int gaib_prof_enable(gaib_ctx* ctx, int on);
int gaib_prof_reset(gaib_ctx* ctx);
int gaib_prof_get(gaib_ctx* ctx, const char* key, int64_t* h_count, double* h_total_ms);
/* the same plus the launches' ALGORITHMIC work as the call sites state it (bytes of the aggregation /
 * edge kernels, flops and operand bytes of the dense products; 0 where a site states none) and h_roof_ms = the time those
 * launches would take at the chip's roofs, per launch max(bytes / 8 TB/s, flops / 157.3 TFLOP/s).  gaib_prof_table: one text
 * line "key[@shape] count total_ms alg_bytes flops roof_ms" per key and launch shape that has records -- shape = the row width
 * of a gather kernel ("spmm_light@47"), M x N x K of a dense product ("sgemm@2449029x128x100") -- (at most cap bytes incl. the
 * terminating 0 are written; *h_needed = what the whole table takes); the epoch records of bench.py are built from it */
int gaib_prof_get_work(gaib_ctx* ctx, const char* key, int64_t* h_count, double* h_total_ms, double* h_bytes, double* h_flops,
                       double* h_roof_ms);
int gaib_prof_table(gaib_ctx* ctx, char* h_buf, size_t cap, size_t* h_needed);
/* heavy-row split of a graph at the context's current threshold: rows / edges handled by the
 * workgroup-per-row kernel, and the maximum degree */
/* locality of the vertex numbering: the share of (sampled) edges whose column id lies within 32 768 of the row id
 * (0 for rectangular graphs and graphs below 262 144 vertices).  The fused aggregation's tile supply follows it: from
 * 0.25 on, tiles are dealt XCD-affine in long chunks (option "spmm_tile_xcd" = -1), else off one global counter; the
 * affine form also requests a row's column ids one row ahead (option "spmm_prefetch_ids", default 1; same sums). */
int gaib_graph_locality(gaib_ctx* ctx, gaib_graph* g, float* h_near_frac);
int gaib_graph_stats(gaib_ctx* ctx, gaib_graph* g, int64_t* h_n_heavy, int64_t* h_heavy_edges,
                     int64_t* h_max_degree);

/* ---- bandwidth probes (measurement only) -------------------------------------------------------
 * gaib_probe_stream_copy: a 16-B-per-lane copy kernel of `bytes` bytes (rounded down to 16), `iters` launches
 *   on the context's stream between one HIP event pair; *h_gbs = (bytes read + bytes written) * iters / time.
 *   This is the chip's achievable streaming rate that bench.py reports next to the 8 TB/s spec figure
 *   (SURVEY.md 8d "confirm with a stream-copy kernel").
 * gaib_probe_peer_copy: hipMemcpyPeerAsync of `bytes` from device src_dev to device dst_dev, `iters` copies
 *   (and as many in the opposite direction at the same time on a second stream when bidir != 0);
 *   *h_gbs = bytes moved per direction * iters / time.  The xGMI link probe
 *   (template: /root/reference/src/test/test_nvlink.cu:37-77).  Needs two visible devices. */
int gaib_probe_stream_copy(gaib_ctx* ctx, size_t bytes, int iters, double* h_gbs);
int gaib_probe_peer_copy(int src_dev, int dst_dev, size_t bytes, int iters, int bidir, double* h_gbs);

/* ---- tuning knobs (benchmarks only; defaults are what ships) ----
 * "agg_zs" (default 1): 1 = the layer library's GCN backward pass gathers a relu-masked gradient of 128 columns from its
 * zero-suppressed image (gaib_pack_zs + gaib_spmm_gemm_zs: three lines per gathered row instead of four, the same bits); off
 * under "agg_bf16", on a partitioned graph, at other widths, on graphs without a packed route (gaib_spmm_gemm_zs_route), and for
 * SAGE's two-product backward until that form is measured faster than the dense one.  "agg_zs_paused" (readable; written by that library): 1 while
 * its guard gathers dense because too many rows of the gradient are over the packed row's capacity.
 * "agg_zs_wide" (default 0; needs "agg_zs" = 1): 1 = the GCN and SAGE backward passes also gather a relu-masked gradient of 256
 * columns packed (gaib_pack_zs_wide + gaib_spmm_gemm_zs / gaib_spmm_gemm2_zs on the K-slab route), same bits, same guard (counted
 * in row-slabs); off until it has been measured on the layer steps.
 * Two options are features rather than knobs: "agg_bf16" (default 0): 1 = the layer library's GCN and SAGE aggregations
 * (libgaib_gnn) gather from a bf16 copy of their table (gaib_cast_f32_bf16_rows at gaib_bf16_row_stride's stride +
 * gaib_spmm_bf16_ld / gaib_spmm_gemm_bf16_ld on whole graphs -- "spmm_bf16_pad" (default 1): 0 = always the dense stride;
 * "agg_bf16_ld_last" (readable; written by that library): the stride of the table it cast last --; GAT ignores
 * it and has "gat_bf16" instead; on a partitioned graph gaib_spmm_part_bf16 / gaib_spmm_gemm_part_bf16 over a bf16 halo exchange, odd widths in fp32);
 * "gemm_bf16" (default 0; needs "agg_bf16" = 1 to have any effect): 1 = where a SAGE layer on a whole graph runs its self term
 * as a separate accumulating product (256 -> 256, 128 -> 256 ...; the 100-wide input stays fp32: K % 8 != 0; gaib_spmm_gemm_fusable(.., 1) == 0) and
 * gaib_gemm_bf16_cover says 1, that product is gaib_gemm_bf16 on the bf16 table the aggregation has just cast instead of
 * gaib_sgemm_ex on the fp32 rows; "gemm_bf16_kernel" (default 1): 0 = gaib_gemm_bf16 refuses every call (GAIB_ERR_UNSUPPORTED),
 * gaib_gemm_bf16_cover says 0;
 * "gat_bf16" (default 0): 1 = the layer library's GAT aggregation casts h (forward) and grad (backward) into bf16 buffers of its
 * own and runs gaib_gat_forward_fused_bf16 / gaib_gat_backward_fused_bf16 where the one-sweep kernels apply (whole graphs), and
 * gaib_gat_forward_fused_drop_bf16 / gaib_gat_backward_fused_drop_bf16 where attention dropout stays in the sweep ("gat_fused_drop"
 * = 1); staged attention dropout runs on the fp32 tables; a partitioned GAT graph refuses the option;
 * "gat_fused_drop" (default 0; readable): 1 = the layer library's GAT aggregation, on a whole graph in the training phase with
 * attention dropout, runs gaib_gat_forward_fused_drop / gaib_gat_backward_fused_drop instead of the staged kernels and holds
 * neither the mask nor the dropped-attention array; the masks are those of the staged path, seed for seed; partitioned graphs
 * stay staged; with "gat_bf16" = 1 the _drop_bf16 calls run first;
 * "gat_fused_wide" (default 0; readable): 1 = gaib_gat_forward_fused / gaib_gat_backward_fused and their _drop forms run multi-head
 * rows wider than 128 columns as column slabs of the one-sweep kernels (gaib_gat_fused_slabs); the layer library keeps attention
 * dropout in the sweep there only with "gat_fused_drop" = 1 as well; the _bf16 / _drop_bf16 calls ("gat_bf16") run the same slabs; partitions stay as they are;
 * "drop_seed_dev" (default 0; readable): 1 = the layer library's feature dropout (dropout_gpu) and its staged GAT attention dropout
 * keep their mask seeds in device memory and draw with gaib_dropout_dev, so that a trainer can record an epoch under dropout; the
 * seeds are the host counters', call for call; read where a seed slot is first needed: set it before the first layer is built;
 * attention dropout kept in the one sweep ("gat_fused_drop" = 1) still takes its seed by value;
 * "spmm_bf16_layout" (0): gaib_spmm_bf16's lane layout, 0 = one row per wave, 4 / 8 =
 * sub-wave rows of 4 / 8 elements per lane.  Both readable with gaib_get_option.
 * "spmm_bf16_fuse_u" (0; benchmark only, readable): gathers a wave keeps in flight in the headline variant of the bf16 fused
 * kernel (row form, 8-row strip, buffer addressing, 65..128 columns): 0 = what ships, 16 / 32 = that depth.  Same bits.
 * "sampler_device" (default 0; readable): read by the trainer, not by the library: 1 = every sampled epoch's subgraph, feature
 * rows and label rows are built on the device (gaib_graph_induce, gaib_gather_rows, gaib_gather_rows_u8), 0 = on the host.
 * A third feature option: "agg_fp8" (default 0; readable): 1 = the layer library's GCN and SAGE aggregations of whole graphs gather
 * from an fp8 copy of their table with per-row scales (gaib_cast_f32_fp8_rows at gaib_fp8_row_stride's stride + gaib_spmm_fp8 /
 * gaib_spmm_gemm_fp8 / gaib_spmm_gemm2_fp8); setting it while "agg_bf16" is 1, or "agg_bf16" while it is 1, is GAIB_ERR_INVALID; a
 * graph with a halo refuses it; GAT ignores it. */
int gaib_set_option(gaib_ctx* ctx, const char* key, int64_t value);
/* what a record wants to name: "comm_reserve_cus" (CUs the fused kernel leaves to the transport: the EFFECTIVE figure -- option,
 * environment or the communicator's default, clamped; "comm_reserve_cus_raw": what the caller set, -1 = unset),
 * "spmm_fuse_cus", "spmm_flat_ring", "num_cus", "agg_bf16", "agg_fp8", "gat_bf16", "spmm_bf16_layout", "spmm_bf16_fuse_u",
 * "spmm_bf16_pad", "agg_bf16_ld_last", "agg_zs", "agg_zs_wide", "agg_zs_paused", "capturing", "gemm_bf16", "gemm_bf16_kernel",
 * "sampler_device", "gat_fused_drop", "gat_fused_wide", "drop_seed_dev" */
int gaib_get_option(gaib_ctx* ctx, const char* key, int64_t* h_value);

#ifdef __cplusplus
}
#endif
#endif /* GAIB_H */
