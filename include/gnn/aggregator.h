// include/gnn/aggregator.h -- the operator classes of the GNN layer path.
// init / aggregate / d_aggregate (/ update_weights) with the reference's signatures
// (include/gnn/aggregator.h:21-88); `in`/`out` are DEVICE pointers, `out` is fully overwritten.
// Each call lowers to gaib_spmm / gaib_gat_* (include/gaib.h) on the process context.
#pragma once
#include "lgraph.h"
#include "math_functions.hh"
#include "optimizer.h"

class aggregator {
 public:
  aggregator() : n(0), length(0), fuse_relu(false) {}
  // extension: bf16 feature tables (context option "agg_bf16" = 1, or GAIB_AGG_DTYPE=bf16): the GCN / SAGE aggregations
  // cast their table into a bf16 scratch and gather from there (gaib_spmm_bf16, gaib_spmm_gemm_bf16 where the product rides along; fp32 sums and output).  The scratch is
  // allocated on first use, which has to lie outside a capture (gaib_capture_*: the trainer records epoch 1 after running
  // epoch 0 eagerly).  GAT ignores the option (it has "gat_bf16", see GAT_Aggregator).  On a partitioned graph (halo) whose exchange can carry bf16 rows -- a halo plan,
  // or set_halo_bf16's callbacks -- the aggregations of even width run on bf16 tables too: the owned rows are cast once, the
  // exchange is begun from the scratch and the class kernels gather bf16 (gaib_spmm_part_bf16, gaib_spmm_gemm_part_bf16) -- the
  // one partition sequence of host/aggregators.cpp (partitioned<T>), which fp32 tables run through as well; odd
  // widths run in fp32 there; a halo with fp32 callbacks only refuses the option.
  static bool bf16_tables();
  // extension: fp8 feature tables with per-row scales (context option "agg_fp8" = 1, or GAIB_AGG_DTYPE=fp8; never together
  // with "agg_bf16"): on a whole graph the GCN / SAGE aggregations cast their table into a process-wide scratch -- e4m3 bytes
  // at gaib_fp8_row_stride's stride, a power-of-two scale per row -- and gather from there (gaib_spmm_fp8, gaib_spmm_gemm_fp8 /
  // gaib_spmm_gemm2_fp8 where the product rides along; fp32 sums and output): the fp32 layer on the rounded table.  The scratch
  // grows on first use, outside a capture, like the bf16 one.  A graph with a halo refuses the option; GAT ignores it.
  static bool fp8_tables();
  // extension: dense self products on that bf16 table (context option "gemm_bf16" = 1, or GAIB_GEMM_DTYPE=bf16; only under
  // bf16_tables()): where a SAGE layer on a whole graph runs its self term as a separate accumulating product and
  // gaib_gemm_bf16 covers the shape, the product multiplies the table the aggregation has just cast (weights split exactly
  // into three bf16 planes) instead of the fp32 rows.  Weight gradients, partitions, GCN and GAT keep their paths.
  static bool gemm_bf16_products();
  // extension: zero-suppressed gradient tables (context option "agg_zs", default 1).  The backward aggregation of a layer with
  // a relu gathers a table that is about half +0.0 (the d_relu has just masked it): aggregate_then_matmul packs such a table
  // of 128 columns into a process-wide scratch (gaib_pack_zs) and gathers from there (gaib_spmm_gemm_zs: the same bits).  The
  // scratch is allocated on first use, outside a capture, like the bf16 one.  Guard: the pack counts the rows over capacity
  // into a pinned host word that is read WITHOUT synchronising (a past step's value); above ZS_GUARD_SHARE of the rows the
  // aggregation gathers dense, packing every ZS_PROBE_EVERY-th call only to look at the count again (never inside a recording).
  // The guard's state is kept per gathered table.  Calls with a second product (SAGE) gather dense for now (ZS_TWO_PRODUCTS).
  // Option "agg_zs_wide" (default 0, GAIB_AGG_ZS_WIDE=1; only under zs_tables()): a masked gradient of 256 columns is packed
  // too (gaib_pack_zs_wide: one image per 128-column K-slab) and gathered on the K-slab route, GCN and SAGE alike (at that width
  // the self term is a separate dense product either way).  Same scratch, guard and cadence; the count is in row-slabs.
  static bool zs_tables();
  static bool zs_wide_tables();
  static bool zs_paused();
  void set_vlen(int vlen) { length = vlen; }
  // extension: the next aggregate() call clamps its output at 0 (the layer's relu_gpu fused
  // into the aggregation's store); cleared by that call
  void fuse_relu_once() { fuse_relu = true; }
  // extension: free what the operator allocated (nothing for GCN / SAGE; GAT: attention vectors, per-edge arrays,
  // partition tables, its Adam state).  See gconv_state::release.
  void release() {}

 protected:
  // extension shared by the GCN / SAGE operators: agg = Op.in followed by out = act(agg . op(W)) -- the
  // layers' "aggregate first" branches -- as ONE kernel (gaib_spmm_gemm: the product runs on the matrix
  // cores inside the aggregating wave).  W is [len x len_out], or [len_out x len] with transW.  keep_agg = false
  // lets the kernel skip the store of agg (still needs the buffer).  On a partitioned graph (halo exchange)
  // it runs as aggregation + matmul.
  // rows2 / W2 (both or neither): + rows2 . op(W2) in the same store (the self term of a SAGE layer)
  // relu_masked: `in` is a gradient the layer's d_relu has masked (see zs_tables)
  void aggregate_then_matmul(int kind, int len, Graph& g, const float* in, float* agg, bool keep_agg,
                             const float* W, bool transW, int len_out, float* out, bool relu,
                             const float* rows2 = NULL, const float* W2 = NULL, bool relu_masked = false);

  int n;
  int length;  // feature vector length
  bool fuse_relu;
};

// out[i,:] = sum_e (vd[i]*vd[col_e]) * in[col_e,:]; backward is the same operator (symmetric)
class GCN_Aggregator : public aggregator {
 public:
  void init(int length, int nv, int ne = 0, float lr = 0.01, float drop_rate = 0.);
  void aggregate(int len, Graph& g, const float* in, float* out);
  void d_aggregate(int len, Graph& g, const float* feat_in, const float* grad_in, float* grad_out);
  // aggregate / d_aggregate fused with the following matmul (see aggregator::aggregate_then_matmul)
  void aggregate_matmul(int len, Graph& g, const float* in, float* agg, bool keep_agg, const float* W,
                        bool transW, int len_out, float* out, bool relu);
  void d_aggregate_matmul(int len, Graph& g, const float* grad_in, float* agg, bool keep_agg, const float* W,
                          bool transW, int len_out, float* out, bool relu_masked = false);
};

// forward: mean over neighbours (1/deg(i)); backward: its transpose (1/deg(col_e))
class SAGE_Aggregator : public aggregator {
 public:
  void init(int length, int nv, int ne = 0, float lr = 0.01, float drop_rate = 0.);
  void aggregate(int len, Graph& g, const float* in, float* out);
  void d_aggregate(int len, Graph& g, const float* feat_in, const float* grad_in, float* grad_out);
  // out = act(mean(in) . op(W) + rows_self . op(W_self)): neighbour and self product of the layer in one kernel
  void aggregate_matmul(int len, Graph& g, const float* in, float* agg, bool keep_agg, const float* W,
                        bool transW, int len_out, float* out, bool relu, const float* rows_self = NULL,
                        const float* W_self = NULL);
  void d_aggregate_matmul(int len, Graph& g, const float* grad_in, float* agg, bool keep_agg, const float* W,
                          bool transW, int len_out, float* out, const float* rows_self = NULL,
                          const float* W_self = NULL, bool relu_masked = false);
};

// single-head attention: p = softmax_row(leaky_relu_0.2(a_l.h_i + a_r.h_j)); out = P h.
// d_aggregate: alpha gradients + P^T g; no gradient through the scores into h (Q18).
class GAT_Aggregator : public aggregator {
 public:
  GAT_Aggregator();
  void init(int length, int nv, int ne = 0, float lr = 0.01, float drop_rate = 0.);
  void aggregate(int len, Graph& g, const float* in, float* out);
  void d_aggregate(int len, Graph& g, const float* feat_in, const float* grad_in, float* grad_out);
  void update_weights(optimizer* opt);
  void release();
  // extension (BASELINE config "GAT 8-head"; the reference is single-head): h independent attentions
  // on the column slices of width length/h.  Call right after init().
  void set_num_heads(int h);
  int num_heads() const { return heads; }
  // extension: the next d_aggregate() may read the layer's forward output rows `out` (post-activation is fine as
  // long as grad_in went through the matching d_relu): it replaces the per-row sum_e p_e dp_e by <grad_i, out_i>
  void use_forward_output_once(const float* out) { fwd_out = out; fwd_out_given = true; }
  // attention dropout (score_drop > 0) is applied while training only, like the layers' feature dropout; the layer
  // passes its phase on before every forward
  void set_training(bool on) { training = on; }
  // device state (tests / checkpoints)
  float* alpha_l_ptr() { return d_alpha_l; }
  float* alpha_r_ptr() { return d_alpha_r; }
  float* alpha_lgrad_ptr() { return d_alpha_lgrad; }
  float* alpha_rgrad_ptr() { return d_alpha_rgrad; }
  float* norm_scores_ptr();  // (materialised on demand after a one-sweep forward, which keeps only row statistics)
  float* temp_scores_ptr() { return d_temp_scores; }  // NULL for 4, 8, 16 heads: not materialised either
  float* scores_ptr() { return NULL; }  // leaky_relu(temp_scores): not materialised by this backend
  float* norm_scores_grad_ptr() { return d_norm_scores_grad; }
  float* norm_scores_dropped_ptr() { return d_norm_scores_drop; }  // NULL unless a training forward dropped attention
  mask_t* attn_masks_ptr() { return d_attn_masks; }
  bool dropped_in_sweep() const { return drop_sweep_ran; }  // a training forward of this layer dropped inside the one sweep

 private:
  // the temp_scores array is kept where re-forming the score is not a gain: 1 or 2 heads (measured on the
  // reddit-shaped graph: 4.0 vs 4.7 ms for scores + softmax backward at 1 head, 10.5 vs 10.1 ms at 8 heads)
  bool needs_temp() const { return !(heads == 4 || heads == 8 || heads == 16); }
  float epsilon;    // LeakyReLU negative slope (0.2)
  // attention dropout: the normalised scores of a training forward are masked and rescaled (the reference's CUDA path,
  // graph_operations.h:326-331; its OpenMP path has the call commented out, gat_aggregator.cpp:78-79), and backward goes
  // through the SAME mask: dp_e is masked and rescaled before the softmax backward (d_dropout, graph_operations.h:376-377
  // -- the `_naive` form; the `_warp` form the reference launches has it commented out at :419-422), and the transposed
  // aggregation uses the dropped attention.  Masks from the library's counter RNG (gaib_dropout), one per (edge, head).
  float attn_drop, attn_scale;
  bool training, dropped_last;  // dropped_last: the last forward applied a mask (backward must take the staged path)
  float* d_norm_scores_drop;    // [ne][heads] p . mask . scale of the last training forward
  mask_t* d_attn_masks;         // [ne][heads]
  size_t drop_cap;
  uint64_t drop_seed;
  bool dropping() const { return attn_drop > 0.f && training; }
  // d_norm_scores -> d_norm_scores_drop (+ masks) under `seed`, or under *d_seed where that is given (gaib_dropout_dev, which
  // advances it); returns the latter
  const float* apply_attn_dropout(size_t n_scores, uint64_t seed, uint64_t* d_seed = NULL);
  // extension: the mask seed in device memory (context option "drop_seed_dev" = 1, or GAIB_DROP_SEED_DEV=1, set BEFORE the first
  // layer is built), so that a recorded epoch draws a new mask per replay.  Staged attention dropout only (gat_fused_drop = 0: the
  // one-sweep _drop kernels take their seed by value and the aggregator stays as it is): next_attn_dropout() is the staged
  // forward's `apply_attn_dropout(.., drop_seed++)`, with the counter in d_drop_seed -- one 8-byte slot per aggregator, made on
  // first use from drop_seed, released with the other device buffers -- where the option was on at that first use.
  const float* next_attn_dropout(size_t n_scores);
  uint64_t* d_drop_seed = NULL;
  int seed_dev = -1;  // -1: the options have not been read yet
  size_t num_edges;
  int heads;
  float *d_alpha_l, *d_alpha_r, *d_alpha_lgrad, *d_alpha_rgrad;
  float *d_temp_scores, *d_norm_scores, *d_norm_scores_grad, *d_norm_scores_t;
  const float* fwd_out;  // see use_forward_output_once
  bool fwd_out_given = false;  // ... was called (a rank WITHOUT rows passes NULL and must still take the path the others take)
  float* d_tbuf;         // output of the fused backward sweep (the layer aliases feat_in and grad_out)
  size_t tbuf_floats;
  // vertex-range partitions: the [owned | halo] column table, the transposed aggregation's output, padded row sums and
  // the column sums of g
  float *d_ptab, *d_pout, *d_prs, *d_pcs;
  size_t ptab_floats, pvec_floats;
  // ... and of the one-sweep path on a partition: the [owned | halo] tables of gradient rows and (rowdot, max, 1/sum) records
  float *d_pgrad, *d_prec;
  size_t pgrad_floats, prec_floats;
  bool part_fused_last;  // the last partition forward was the one-sweep kernel (row statistics only)
  void ensure_partition_buffers(Graph& g, int len);
  void aggregate_partition(int len, Graph& g, const float* in, float* out);
  void d_aggregate_partition(int len, Graph& g, const float* grad_in, float* grad_out);
  // one-sweep forward (gaib_gat_forward_fused): per (row, head) the softmax's maximum and 1 / sum
  float* d_row_stats;
  size_t stats_floats;
  bool stats_valid;   // the last forward kept statistics instead of the attention array
  Graph* last_graph;  // ... of this graph and input, should the array be asked for
  const float* last_in;
  int last_len;
  void materialise_scores();
  // extension: bf16 tables (context option "gat_bf16" = 1, or GAIB_GAT_DTYPE=bf16).  On a whole graph, without attention
  // dropout or with it kept in the sweep (gat_fused_drop: the _drop_bf16 calls under the same seeds, the fp32 _drop calls where
  // those do not apply), at a shape the one-sweep kernels cover (with gat_fused_wide also rows wider than 128 columns),
  // aggregate() casts `in` into d_hb16 and runs
  // gaib_gat_forward_fused_bf16; d_aggregate() then casts grad_in (process-wide scratch) and runs
  // gaib_gat_backward_fused_bf16 on the KEPT copy of h -- when that forward ran on bf16, the layer's forward output is at
  // hand and feat_in is the table that forward cast; in every other case the fp32 path runs as without the option.  The
  // layer then computes forward and backward of the fp32 layer on the rounded h and grad.  d_hb16 belongs to the aggregator:
  // it lives from a layer's forward to its backward while other layers run.  It grows on demand like d_tbuf, which has to
  // happen outside a capture.  A partitioned GAT graph refuses the option.  (norm_scores_ptr() after such a forward forms the
  // attention array from the fp32 `in`, like the staged path it serves: within the bf16 rounding of what the sweep used.)
  static bool gat_bf16_tables();
  uint16_t* d_hb16 = NULL;
  const uint16_t* cast_hb16(size_t elems, const float* in);
  size_t hb16_elems = 0;
  bool fwd_bf16 = false;  // the last forward ran on d_hb16 = bf16(last_in) over last_graph
  // extension: attention dropout inside the one sweep (context option "gat_fused_drop" = 1, or GAIB_GAT_FUSED_DROP=1).  On a
  // whole graph, in the training phase with attn_drop > 0, aggregate() runs gaib_gat_forward_fused_drop under seed = drop_seed++
  // -- the seed the staged path would have drawn, so both paths train through the same masks -- and keeps the row statistics
  // and that seed; neither d_norm_scores_drop nor d_attn_masks is allocated.  d_aggregate() runs gaib_gat_backward_fused_drop
  // under the kept seed when the layer's forward output is at hand and feat_in, graph and len are that forward's.  Where it
  // may not (gat_fused_bwd = 0, no forward output), the attention is materialised, mask and dropped attention are drawn AGAIN
  // with gaib_dropout under the kept seed -- the bits the sweep used -- and the staged pieces run.  Partitioned graphs stay
  // staged; bf16 tables (gat_bf16) are not used under dropout, with or without this option.
  static bool gat_fused_drop_option();
  // extension: multi-head rows wider than 128 columns in the one-sweep kernels, one column slab at a time (context option
  // "gat_fused_wide" = 1, or GAIB_GAT_WIDE=1, set BEFORE the layer is built).  Nothing changes in aggregate() / d_aggregate():
  // gaib_gat_forward_fused / gaib_gat_backward_fused accept the shape instead of answering GAIB_ERR_UNSUPPORTED, and every
  // fallback (gat_fused_bwd = 0, no forward output, norm_scores_ptr()) works from the full-width row statistics as at a narrow
  // shape.  Where the sweeps are expected to run -- the option, a shape with gaib_gat_fused_slabs >= 2, and either no attention
  // dropout or option "gat_fused_drop" = 1 as well (the _drop calls then accept the shape too) -- set_num_heads() does not hold
  // the [ne][heads] arrays; grow_edge_arrays() allocates them for the staged piece that first needs them, apply_attn_dropout()
  // mask and dropped attention.  Attention dropout without "gat_fused_drop", bf16 tables and partitions stay as they are at
  // these widths.
  bool wide_rows_expected() const;
  void grow_edge_arrays(size_t ne);
  bool drop_fused_last = false;  // the last forward was the dropped one sweep under drop_seed_last
  uint64_t drop_seed_last = 0;
  bool drop_sweep_ran = false;   // ... at least once (the trainer reports it)
  optimizer* alpha_opt;
};
