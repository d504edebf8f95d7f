// aggregators.cpp -- GCN / SAGE / GAT aggregators: each operator call is one or a few entries of
// the C ABI (include/gaib.h) on the process context.
#include "aggregator.h"
#include "host_util.h"

using gaib_host::OpTimer;
// edges aggregated so far by this process: one count of the graph's edges per aggregation call (BASELINE's
// "aggregated edges"; bench.py counts the same way)
static inline void count_edges(Graph& g) { gpu_context::add_aggregated_edges((uint64_t)g.sizeEdges()); }
static inline gaib_ctx* C() { return gpu_context::get(); }

static gaib_graph* dev(Graph& g) {
  if (!g.device_graph()) g.copy_to_gpu();
  return g.device_graph();
}
// a device buffer of the aggregator that only grows: `need` elements above `cap` -> free, allocate, remember (contents are lost).
// Returns whether it did.  (Two buffers that share one capacity: the first grows against a copy of it.)
template <class T>
static bool grow(T*& p, size_t& cap, size_t need) {
  if (need <= cap) return false;
  if (p) GAIB_OR_DIE(gaib_free(C(), p));
  p = gaib_host::dmalloc<T>(need);
  cap = need;
  return true;
}

// ---- bf16 feature tables (option agg_bf16) ------------------------------------------------------------------------------
bool aggregator::bf16_tables() { return gaib_host::option("agg_bf16") != 0; }
bool aggregator::gemm_bf16_products() { return gaib_host::option("gemm_bf16") != 0; }
// One process-wide scratch.  A buffer that has to grow is kept, not freed: a recorded epoch (gaib_exec) may still name it.
static uint16_t* g_bf16_tab = nullptr;
static size_t g_bf16_cap = 0;
static gaib_ctx* g_bf16_ctx = nullptr;
static std::vector<uint16_t*> g_bf16_retired;
static uint16_t* bf16_table(size_t elems) {
  if (g_bf16_ctx != C()) {  // a new process context (gpu_context::set): start a buffer on its device
    if (g_bf16_tab) g_bf16_retired.push_back(g_bf16_tab);
    g_bf16_tab = nullptr;
    g_bf16_cap = 0;
    g_bf16_ctx = C();
  }
  if (elems > g_bf16_cap) {
    if (g_bf16_tab) g_bf16_retired.push_back(g_bf16_tab);
    g_bf16_tab = nullptr;
    g_bf16_cap = 0;
    // (inside a capture gaib_malloc refuses: the run has to reserve the scratch before it records)
    GAIB_OR_DIE(gaib_malloc(C(), elems * sizeof(uint16_t), (void**)&g_bf16_tab));
    g_bf16_cap = elems;
  }
  return g_bf16_tab;
}

// the table of `rows` x `len` floats at `in` as bf16 bits in the scratch
static const uint16_t* to_bf16(size_t rows, int len, const float* in) {
  const size_t n = rows * (size_t)len;
  uint16_t* t = bf16_table(n);
  GAIB_OR_DIE(gaib_cast_f32_bf16(C(), (int64_t)n, in, t));
  return t;
}
// ... of a WHOLE graph `dg`, at the row stride the library's rule names for it (gaib_bf16_row_stride: odd widths line-aligned
// where that saves gathered lines; the strided cast is the one pass the cast is anyway).  *ld = that stride, which the caller
// hands to the _ld aggregation; option "agg_bf16_ld_last" reports it.  Partitions and GAT keep the dense stride (to_bf16 above).
static const uint16_t* to_bf16(gaib_graph* dg, int len, const float* in, int64_t* ld) {
  const size_t rows = (size_t)gaib_graph_nc(dg);
  GAIB_OR_DIE(gaib_bf16_row_stride(C(), dg, len, ld));
  uint16_t* t = bf16_table(rows * (size_t)*ld);
  GAIB_OR_DIE(gaib_cast_f32_bf16_rows(C(), (int64_t)rows, len, in, *ld, t));
  GAIB_OR_DIE(gaib_set_option(C(), "agg_bf16_ld_last", *ld));
  return t;
}
// bf16 tables on a vertex-range partition need an exchange that carries bf16 rows: a library plan (set_halo_plan) or bf16
// callbacks (set_halo_bf16).  A halo set with the fp32 callbacks alone (set_halo) cannot: refused as before.
static void no_bf16_halo(Graph& g) {
  if (!g.has_halo() || g.halo_carries_bf16()) return;
  fprintf(stderr, "GPU error: agg_bf16 (GAIB_AGG_DTYPE=bf16) on a graph with a halo (partitioned run) needs an exchange that "
          "carries bf16 rows: a halo plan (set_halo_plan) or bf16 callbacks (set_halo_bf16); this graph's halo was set with fp32 "
          "callbacks (set_halo)\n");
  exit(EXIT_FAILURE);
}
// does this aggregation of `len` columns run on bf16 tables?  Whole graphs: always under agg_bf16.  On a partition: even widths
// (an odd-width bf16 row is not a whole number of the 4-byte words the exchange moves: such an aggregation -- the 47-wide ones --
// runs on the fp32 path; the trainer's table line says so)
static bool bf16_for(Graph& g, int len) {
  if (!aggregator::bf16_tables()) return false;
  no_bf16_halo(g);
  return !g.has_halo() || len % 2 == 0;
}

// ---- fp8 feature tables with per-row scales (option agg_fp8) ---------------------------------------------------------------
bool aggregator::fp8_tables() { return gaib_host::option("agg_fp8") != 0; }
// One process-wide scratch holding the table ([rows x ld] bytes, rounded up to 256) and its row scales behind it.  Grown outside
// captures only and retired, not freed, like g_bf16_tab: a recorded epoch may still name a buffer that had to grow.
static uint8_t* g_fp8_tab = nullptr;
static size_t g_fp8_cap = 0;
static gaib_ctx* g_fp8_ctx = nullptr;
static std::vector<uint8_t*> g_fp8_retired;
static uint8_t* fp8_scratch(size_t bytes) {
  if (g_fp8_ctx != C()) {  // a new process context (gpu_context::set): start a buffer on its device
    if (g_fp8_tab) g_fp8_retired.push_back(g_fp8_tab);
    g_fp8_tab = nullptr;
    g_fp8_cap = 0;
    g_fp8_ctx = C();
  }
  if (bytes > g_fp8_cap) {
    if (g_fp8_tab) g_fp8_retired.push_back(g_fp8_tab);
    g_fp8_tab = nullptr;
    g_fp8_cap = 0;
    // (inside a capture gaib_malloc refuses: the run has to reserve the scratch before it records)
    GAIB_OR_DIE(gaib_malloc(C(), bytes, (void**)&g_fp8_tab));
    g_fp8_cap = bytes;
  }
  return g_fp8_tab;
}
struct Fp8Table {
  const uint8_t* q;
  const float* scale;
  int64_t ld;
};
// the table of a WHOLE graph `dg` (`len` floats per row at `in`) cast into the scratch at gaib_fp8_row_stride's stride
static Fp8Table to_fp8(gaib_graph* dg, int len, const float* in) {
  const size_t rows = (size_t)gaib_graph_nc(dg);
  Fp8Table t;
  GAIB_OR_DIE(gaib_fp8_row_stride(len, &t.ld));
  const size_t tab_bytes = (rows * (size_t)t.ld + 255) & ~(size_t)255;
  uint8_t* base = fp8_scratch(tab_bytes + rows * sizeof(float));
  float* scale = reinterpret_cast<float*>(base + tab_bytes);
  GAIB_OR_DIE(gaib_cast_f32_fp8_rows(C(), (int64_t)rows, len, in, t.ld, base, scale));
  t.q = base;
  t.scale = scale;
  return t;
}
// does this aggregation run on an fp8 table?  Whole graphs: always under agg_fp8.  A graph with a halo (partitioned run) has no
// exchange that carries fp8 rows with their scales and no row-class kernels: refused, never a silent fp32 path.
static bool fp8_for(Graph& g) {
  if (!aggregator::fp8_tables()) return false;
  if (g.has_halo()) {
    fprintf(stderr, "GPU error: agg_fp8 (GAIB_AGG_DTYPE=fp8) on a graph with a halo (partitioned run): fp8 feature tables are "
            "gathered on whole graphs only\n");
    exit(EXIT_FAILURE);
  }
  return true;
}

// ---- zero-suppressed gradient tables (option agg_zs) ---------------------------------------------------------------------
// Where the packed launch set (pack + heavy + fused) stops beating the dense one: the share of rows over capacity from which
// the layers gather dense.  An over-capacity row costs a dense 512-B gather that the wave waits for on top of its packed one.
// scripts/zs_aggregation.py sweeps the kept share of the gradient from 40 to 90 % on the products-shaped graph
// (profiles/zs/zs_gather_groups.json, LEDGER 10.4): packed wins by 1.13 ms at 50 % kept (0.02 % of the rows over capacity), by
// 0.65 ms at 60 % (3.5 %), by 0.15 ms at 62 % (7.3 %), loses 0.68 ms at 64 % (13.9 %) -- the two sets cross near 8.5 % of the rows.
// At 256 columns (agg_zs_wide) the pack counts over-capacity ROW-SLABS, two per row, and each slab launch has the economics of
// the 128-column launch set: the same share, of rows * 2.  A starting value -- the crossing has not been measured at this width
// (scripts/zs_wide.py reports it).
static const double ZS_GUARD_SHARE = 0.08;
static const unsigned ZS_PROBE_EVERY = 8;
// Two products (SAGE's backward: the self term rides along, the 2-row-strip kernel at 127 VGPRs with 10 spilled): the packed
// kernels exist and are bit-identical (gaib_spmm_gemm2_zs).  With the grouped expansion the packed call is the faster one at the
// kernel level (8.83 -> 8.14 ms at 50 % kept, pack included; LEDGER 10.4), but it has not been measured on the SAGE layer step in
// alternating pairs, and tests/test_gpu_zs.py holds SAGE to the dense gather: until both are settled SAGE gathers dense.
static const bool ZS_TWO_PRODUCTS = false;
bool aggregator::zs_tables() { return gaib_host::option("agg_zs") != 0; }
bool aggregator::zs_wide_tables() { return gaib_host::option("agg_zs_wide") != 0; }
bool aggregator::zs_paused() { return gaib_host::option("agg_zs_paused") != 0; }
// The guard's state is kept PER GATHERED TABLE (the layer's grad_in buffer): in a model, the count one layer's pack left behind
// says nothing about the next layer's gradient.  Each table has its own device counter and pinned host word.
static const int ZS_SLOTS = 16;  // tables watched at a time (a deeper model shares slots round robin: counts then mix)
struct ZsWatch {
  const float* table = nullptr;
  size_t counted_rows = 0;  // rows (256 columns: row-slabs) of the pack the slot's count belongs to (0: no pack yet)
  bool paused = false;
  unsigned since_probe = 0;
};
static struct {
  gaib_ctx* ctx = nullptr;
  unsigned gen = 0;  // gpu_context::generation() of ctx
  void* tab = nullptr;  // [cap_bytes]: rows x 384 B, or 2 x rows x 384 B for a table of 256 columns
  size_t cap_bytes = 0;
  uint32_t* d_over = nullptr;           // [ZS_SLOTS] the packs' counts of over-capacity rows ...
  volatile uint32_t* h_over = nullptr;  // [ZS_SLOTS] ... read back into pinned memory behind every pack
  ZsWatch watch[ZS_SLOTS];
  int n_watch = 0, next_evict = 0;
  std::vector<void*> retired;  // (a recorded epoch may still name a buffer that had to grow)
} g_zs;
// a new process context (gpu_context::set) -- told by its generation: it may sit at the address of the one it replaced, and the
// watch list of the old one (a table that was left paused and has since been freed) would keep "agg_zs_paused" at 1 for good
static bool zs_other_context() { return g_zs.ctx != C() || g_zs.gen != gpu_context::generation(); }
static void* zs_table(size_t bytes) {
  if (zs_other_context()) {  // start over on its device; no recorded sequence of the old context is alive (gaib_ctx_destroy)
    if (g_zs.h_over) GAIB_OR_DIE(gaib_host_free(C(), const_cast<uint32_t*>(g_zs.h_over)));
    if (g_zs.d_over) GAIB_OR_DIE(gaib_free(C(), g_zs.d_over));
    if (g_zs.tab) GAIB_OR_DIE(gaib_free(C(), g_zs.tab));
    for (void* p : g_zs.retired) GAIB_OR_DIE(gaib_free(C(), p));
    g_zs.retired.clear();
    g_zs.tab = nullptr;
    g_zs.cap_bytes = 0;
    g_zs.ctx = C();
    g_zs.gen = gpu_context::generation();
    g_zs.n_watch = g_zs.next_evict = 0;
    GAIB_OR_DIE(gaib_malloc(C(), sizeof(uint32_t) * ZS_SLOTS, (void**)&g_zs.d_over));
    void* h = nullptr;
    GAIB_OR_DIE(gaib_host_alloc(C(), sizeof(uint32_t) * ZS_SLOTS, &h));
    g_zs.h_over = static_cast<volatile uint32_t*>(h);
    for (int i = 0; i < ZS_SLOTS; i++) g_zs.h_over[i] = 0;
  }
  if (bytes > g_zs.cap_bytes) {
    if (g_zs.tab) g_zs.retired.push_back(g_zs.tab);
    g_zs.tab = nullptr;
    g_zs.cap_bytes = 0;
    // (inside a capture gaib_malloc refuses: the run has to reserve the scratch before it records)
    GAIB_OR_DIE(gaib_malloc(C(), bytes, &g_zs.tab));
    g_zs.cap_bytes = bytes;
  }
  return g_zs.tab;
}
static int zs_slot(const float* table) {
  for (int i = 0; i < g_zs.n_watch; i++)
    if (g_zs.watch[i].table == table) return i;
  int i;
  if (g_zs.n_watch < ZS_SLOTS) i = g_zs.n_watch++;
  else i = g_zs.next_evict++ % ZS_SLOTS;
  g_zs.watch[i] = ZsWatch();
  g_zs.watch[i].table = table;
  return i;
}
// pack `rows` x len (128, or 256: the wide image) floats at `in` into the scratch; the count of over-capacity rows (row-slabs)
// follows into the slot's pinned word
static const void* zs_pack(int slot, size_t rows, int len, const float* in) {
  const size_t slabs = (size_t)len / 128;
  void* t = zs_table(rows * slabs * 384);
  GAIB_OR_DIE(gaib_fill_f32(C(), 1, 0.f, reinterpret_cast<float*>(g_zs.d_over + slot)));
  if (len == 128) GAIB_OR_DIE(gaib_pack_zs(C(), (int64_t)rows, len, in, t, g_zs.d_over + slot));
  else GAIB_OR_DIE(gaib_pack_zs_wide(C(), (int64_t)rows, len, in, t, g_zs.d_over + slot));
  GAIB_OR_DIE(gaib_memcpy_d2h_async(C(), const_cast<uint32_t*>(g_zs.h_over + slot), g_zs.d_over + slot, sizeof(uint32_t)));
  g_zs.watch[slot].counted_rows = rows * slabs;
  return t;
}
// ("agg_zs_paused" reads 1 while ANY watched table is gathered dense by the guard)
static void zs_set_paused(int slot, bool p) {
  ZsWatch& w = g_zs.watch[slot];
  if (p == w.paused) return;
  w.paused = p;
  w.since_probe = 0;
  bool any = false;
  for (int i = 0; i < g_zs.n_watch; i++) any = any || g_zs.watch[i].paused;
  GAIB_OR_DIE(gaib_set_option(C(), "agg_zs_paused", any ? 1 : 0));
}

// ---- aggregation on a vertex-range partition ---------------------------------------------------------------------------------
// Written once on T, the element type of the gathered and exchanged table: float, or uint16_t = bf16 bits (agg_bf16, even len).
// What differs by type is this set of functions and nothing else: the exchange calls, the plain gather and the gather with the
// dense product(s) riding on it.  Both gathers run `dg` over `tab`, or -- tab2 given -- in one pass over [tab (n_first rows) | tab2].
static void halo_begin_t(Graph& g, int len, const float* tab) { g.halo_begin(len, tab); }
static void halo_begin_t(Graph& g, int len, const uint16_t* tab) { g.halo_begin_bf16(len, tab); }
static const float* halo_end_t(Graph& g, int len, const float*) { return g.halo_end(len); }
static const uint16_t* halo_end_t(Graph& g, int len, const uint16_t*) { return g.halo_end_bf16(len); }
static const float* halo_wait_t(Graph& g, int k, const float*) { return g.halo_wait_piece(k); }
static const uint16_t* halo_wait_t(Graph& g, int k, const uint16_t*) { return g.halo_wait_piece_bf16(k); }
static void gather_t(gaib_graph* dg, int kind, int len, const float* tab, const float* tab2, int64_t n_first, float* out, int fl) {
  if (tab2 || n_first > 0) GAIB_OR_DIE(gaib_spmm_2t(C(), dg, kind, NULL, len, tab, tab2, n_first, out, fl));
  else GAIB_OR_DIE(gaib_spmm_ex(C(), dg, kind, NULL, len, tab, out, fl));
}
static void gather_t(gaib_graph* dg, int kind, int len, const uint16_t* tab, const uint16_t* tab2, int64_t n_first, float* out, int fl) {
  GAIB_OR_DIE(gaib_spmm_part_bf16(C(), dg, kind, NULL, len, tab, tab2, n_first, out, fl));
}
// the dense half of aggregate_then_matmul: out = act(agg . op(W) [+ rows2 . op(W2)]), len_out columns
struct Product {
  float* agg;
  const float* W;
  int transW;
  const float *rows2, *W2;
  int len_out;
  float* out;
};
static void fused_t(gaib_graph* dg, int kind, int len, const float* tab, const float* tab2, int64_t n_first, const Product& p, int fl) {
  if (tab2 || n_first > 0)
    GAIB_OR_DIE(gaib_spmm_gemm_2t(C(), dg, kind, NULL, len, tab, tab2, n_first, p.agg, p.W, p.transW, p.rows2, p.W2, p.len_out, p.out, fl));
  else if (p.rows2)
    GAIB_OR_DIE(gaib_spmm_gemm2(C(), dg, kind, NULL, len, tab, p.agg, p.W, p.transW, p.rows2, p.W2, p.len_out, p.out, fl));
  else
    GAIB_OR_DIE(gaib_spmm_gemm(C(), dg, kind, NULL, len, tab, p.agg, p.W, p.transW, p.len_out, p.out, fl));
}
static void fused_t(gaib_graph* dg, int kind, int len, const uint16_t* tab, const uint16_t* tab2, int64_t n_first, const Product& p, int fl) {
  GAIB_OR_DIE(gaib_spmm_gemm_part_bf16(C(), dg, kind, NULL, len, tab, tab2, n_first, p.agg, p.W, p.transW, p.rows2, p.W2, p.len_out, p.out, fl));
}

// The halo-column half of a partitioned aggregation over `whole` (the mode's halo-column graph): in one pass after the whole
// exchange -- last(whole, table) --, or, where the exchange travels in K > 1 time slices (gaib_halo_set_pieces), piece by piece
// as the slices land: plain(piece k, table) in accumulate mode for every piece but the last non-empty one, which takes last()
// (the pass that carries the activation / the dense product).  Same terms per row, added piece by piece.  Ends the exchange.
template <class T, class Plain, class Last>
static void halo_half(Graph& g, gaib_graph* whole, int len, Plain plain, Last last) {
  const int K = g.halo_pieces(len);
  if (K <= 1) {
    last(whole, halo_end_t(g, len, (const T*)NULL));
    return;
  }
  int last_k = 0;
  for (int k = 0; k < K; k++)
    if (gaib_graph_ne(g.halo_piece_graph(k)) > 0) last_k = k;
  for (int k = 0; k < last_k; k++)
    if (gaib_graph_ne(g.halo_piece_graph(k)) > 0) plain(g.halo_piece_graph(k), halo_wait_t(g, k, (const T*)NULL));
  last(g.halo_piece_graph(last_k), halo_end_t(g, len, (const T*)NULL));  // (pieces behind last_k are empty: waiting for all of them costs nothing)
}

// One partitioned aggregation of the owned rows over `tab` (the owned table; the exchange is begun from it, so with bf16 tables
// nothing else may be cast into the scratch before it has ended: every path below ends it before it returns).  The work that needs
// no halo row runs while the halo rows are in flight (separate RCCL stream), the rest after they have arrived -- by row class
// (LearningGraph::partition_mode):
//   PART_SPLIT    owned-column edges of all rows meanwhile, halo-column edges added to the same rows after
//   PART_CLASSES  interior rows complete + the boundary rows' owned-column edges meanwhile, their halo-column edges after
//   PART_ONEPASS  interior rows complete meanwhile, the boundary rows in one pass over [owned | halo] after
// Partial sums go to `sums` through the plain gather.  final(graph, tab, tab2, n_first, extra) is the caller's pass that completes
// rows (it carries the activation / the dense product); extra = GAIB_ACCUMULATE where it continues partial sums,
// GAIB_OVERLAPS_TRANSFER while rows are on the wire.  Without halo-column edges the rows that could have had some are completed in
// flight: all owned rows (split), or -- classes, only if empty_boundary_class -- the boundary class, which is then empty.
template <class T, class Final>
static void partitioned(Graph& g, int kind, int len, const T* tab, float* sums, bool empty_boundary_class, Final final) {
  const T* const none = NULL;
  const int mode = g.partition_mode(len);
  halo_begin_t(g, len, tab);  // every rank joins every exchange, also one without halo edges
  if (mode != Graph::PART_SPLIT) {
    final(g.class_interior(), tab, none, 0, GAIB_OVERLAPS_TRANSFER);  // (the exchange is in flight: RCCL's kernels need CUs)
    if (mode != Graph::PART_CLASSES) {
      const T* halo = halo_end_t(g, len, none);
      final(g.class_boundary_full(), tab, halo, (int64_t)g.size(), 0);
      return;
    }
  }
  gaib_graph* half = mode == Graph::PART_SPLIT ? g.halo_graph() : g.class_boundary_halo();
  gaib_graph* meanwhile = mode == Graph::PART_SPLIT ? dev(g) : g.class_boundary_own();
  if (gaib_graph_ne(half) == 0) {  // (classes: no boundary row either)
    if (mode == Graph::PART_SPLIT || empty_boundary_class) final(meanwhile, tab, none, 0, GAIB_OVERLAPS_TRANSFER);
    halo_end_t(g, len, none);
    return;
  }
  // owned-column edges while the halo rows travel; the halo-column edges then continue the sums
  gather_t(meanwhile, kind, len, tab, none, 0, sums, 0);
  halo_half<T>(g, half, len, [&](gaib_graph* gh, const T* halo) { gather_t(gh, kind, len, halo, none, 0, sums, GAIB_ACCUMULATE); },
               [&](gaib_graph* gh, const T* halo) { final(gh, halo, none, 0, GAIB_ACCUMULATE); });
}

// the owned rows of a partitioned graph cast into the bf16 scratch ONCE: the owned-column passes gather from it and the exchange is
// begun FROM it (half the bytes packed and on the wire; over RCCL a contiguous send list is read straight from it)
static const uint16_t* owned_bf16(Graph& g, int len, const float* in) { return to_bf16((size_t)gaib_graph_nc(dev(g)), len, in); }

// One aggregation.  On a partition every pass is the plain gather: the final one adds the activation (it runs no kernel that
// yields CUs to the transport, so of `extra` it takes the accumulate bit alone), and an empty boundary class is still launched.
static void aggregate_rows(Graph& g, int kind, int len, const float* in, float* out, bool relu = false, bool count = true) {
  if (count) count_edges(g);
  const int act = relu ? GAIB_RELU : 0;
  const bool bf16 = bf16_for(g, len);
  const bool fp8 = fp8_for(g);
  if (g.has_halo()) {
    auto run = [&](auto tab) {
      partitioned(g, kind, len, tab, out, true, [&](gaib_graph* dg, decltype(tab) t, decltype(tab) t2, int64_t n_first, int extra) {
        gather_t(dg, kind, len, t, t2, n_first, out, act | (extra & GAIB_ACCUMULATE));
      });
    };
    if (bf16) run(owned_bf16(g, len, in));
    else run(in);
    return;
  }
  if (bf16) {
    gaib_graph* dg = dev(g);
    int64_t ld = len;
    const uint16_t* tab = to_bf16(dg, len, in, &ld);
    GAIB_OR_DIE(gaib_spmm_bf16_ld(C(), dg, kind, NULL, len, ld, tab, out, act));
    return;
  }
  if (fp8) {
    gaib_graph* dg = dev(g);
    const Fp8Table t = to_fp8(dg, len, in);
    GAIB_OR_DIE(gaib_spmm_fp8(C(), dg, kind, NULL, len, t.ld, t.q, t.scale, out, act));
    return;
  }
  GAIB_OR_DIE(gaib_spmm_ex(C(), dev(g), kind, NULL, len, in, out, act));
}

void aggregator::aggregate_then_matmul(int kind, int len, Graph& g, const float* in, float* agg, bool keep_agg,
                                       const float* W, bool transW, int len_out, float* out, bool relu,
                                       const float* rows2, const float* W2, bool relu_masked) {
  OpTimer t(OP_SPARSEMM);
  count_edges(g);
  const bool bf16 = bf16_for(g, len);
  const bool fp8 = fp8_for(g);
  const int act = relu ? GAIB_RELU : 0;
  const int flags = act | (keep_agg ? 0 : GAIB_AGG_SCRATCH);
  const Product prod{agg, W, transW ? 1 : 0, rows2, W2, len_out, out};
  if (g.has_halo()) {
    // the classes fill disjoint rows of ONE output: all of them take the fused kernel, or -- a shape it does not cover --
    // the aggregation runs class by class and the product(s) once over all rows
    if (g.partition_mode(len) != Graph::PART_SPLIT && !gaib_spmm_gemm_fusable(C(), kind, len, len_out, rows2 ? 1 : 0)) {
      aggregate_rows(g, kind, len, in, agg, false, false);
      GAIB_OR_DIE(gaib_sgemm_ex(C(), 0, transW ? 1 : 0, (int64_t)g.size(), len_out, len, agg, W, rows2 ? 0 : act, out));
      if (rows2)
        GAIB_OR_DIE(gaib_sgemm_ex(C(), 0, transW ? 1 : 0, (int64_t)g.size(), len_out, len, rows2, W2, GAIB_ACCUMULATE | act, out));
      return;
    }
    // every pass that completes rows carries the dense product(s); the partial sums continue in agg.  No boundary row: no launch.
    auto run = [&](auto tab) {
      partitioned(g, kind, len, tab, agg, false, [&](gaib_graph* dg, decltype(tab) t, decltype(tab) t2, int64_t n_first, int extra) {
        fused_t(dg, kind, len, t, t2, n_first, prod, flags | extra);
      });
    };
    if (bf16) run(owned_bf16(g, len, in));
    else run(in);
    return;
  }
  if (bf16) {
    // bf16 table: the fused kernel gathers from it -- the route (and the bits) of the fp32 branch below on the rounded table
    gaib_graph* dg = dev(g);
    int64_t ld = len;
    const uint16_t* tab = to_bf16(dg, len, in, &ld);
    // option gemm_bf16: the self rows ARE the table just cast and every dense route runs the self term as a separate
    // accumulating product (spmm.hip: two matrices that do not fit LDS together, the K-slab route, the unfused one) -- that
    // product on the bf16 table (gaib_gemm_bf16: exactly split weights), the neighbour half as before: both terms are then
    // "the fp32 layer on the rounded table"
    if (rows2 == in && gemm_bf16_products() && gaib_spmm_gemm_fusable(C(), kind, len, len_out, 1) == 0 &&
        gaib_gemm_bf16_cover(C(), transW ? 1 : 0, len_out, len, ld) == 1) {
      GAIB_OR_DIE(gaib_spmm_gemm_bf16_ld(C(), dg, kind, NULL, len, ld, tab, agg, W, transW ? 1 : 0, len_out, out, flags & ~GAIB_RELU));
      GAIB_OR_DIE(gaib_gemm_bf16(C(), transW ? 1 : 0, (int64_t)g.size(), len_out, len, ld, tab, W2, GAIB_ACCUMULATE | act, out));
      return;
    }
    if (rows2)
      GAIB_OR_DIE(gaib_spmm_gemm2_bf16_ld(C(), dg, kind, NULL, len, ld, tab, agg, W, transW ? 1 : 0, rows2, W2, len_out, out, flags));
    else
      GAIB_OR_DIE(gaib_spmm_gemm_bf16_ld(C(), dg, kind, NULL, len, ld, tab, agg, W, transW ? 1 : 0, len_out, out, flags));
    return;
  }
  if (fp8) {
    // fp8 table with row scales: the route (and the bits) of the fp32 branch below on the rounded table; ahead of the
    // zero-suppressed branch like bf16.  The self rows stay fp32 (option gemm_bf16 is inert without a bf16 table).
    gaib_graph* dg = dev(g);
    const Fp8Table t = to_fp8(dg, len, in);
    if (rows2)
      GAIB_OR_DIE(gaib_spmm_gemm2_fp8(C(), dg, kind, NULL, len, t.ld, t.q, t.scale, agg, W, transW ? 1 : 0, rows2, W2, len_out, out, flags));
    else
      GAIB_OR_DIE(gaib_spmm_gemm_fp8(C(), dg, kind, NULL, len, t.ld, t.q, t.scale, agg, W, transW ? 1 : 0, len_out, out, flags));
    return;
  }
  // (256 columns, option agg_zs_wide: the K-slab route, whose launches are one-product ones -- ZS_TWO_PRODUCTS concerns the
  // 128-column two-product kernel only)
  const bool zs_narrow = len == 128 && (!rows2 || ZS_TWO_PRODUCTS);
  if (relu_masked && (zs_narrow || len == 256) && zs_tables() && (len == 128 || zs_wide_tables())) {
    gaib_graph* dg = dev(g);
    const size_t rows = (size_t)gaib_graph_nc(dg);
    const size_t tab_bytes = rows * (size_t)(len / 128) * 384;
    const bool capturing = gaib_host::capturing();
    if (zs_other_context()) zs_table(0);
    // is there a packed route for this call?  Asked from the route information alone, before anything is packed or allocated (a
    // graph of short rows, a numbering with locality, a dense graph the ordered chunks take, a table of 4 GB: the dense call's
    // variants).  The query reads nothing through the image pointer: any 128-B aligned address stands for it.
    int route = gaib_spmm_gemm_zs_route(C(), dg, kind, len, in, g_zs.d_over, agg, rows2, len_out, out);
    if (route != GAIB_OK && route != GAIB_ERR_UNSUPPORTED) GAIB_OR_DIE(route);
    if (route == GAIB_OK && tab_bytes > g_zs.cap_bytes) {
      if (capturing) route = GAIB_ERR_UNSUPPORTED;  // (a recording that would have to grow the scratch: dense)
      else zs_table(tab_bytes);
    }
    if (route == GAIB_OK) {
      const int slot = zs_slot(in);
      ZsWatch& w = g_zs.watch[slot];
      // the guard looks at the count this table's last finished pack left behind (no synchronisation: a past step's value)
      if (w.counted_rows > 0) zs_set_paused(slot, (double)g_zs.h_over[slot] > ZS_GUARD_SHARE * (double)w.counted_rows);
      if (w.paused) {
        // a look at the count every ZS_PROBE_EVERY-th call -- never inside a recording: a recorded epoch of a paused table
        // gathers dense and packs nothing, whatever the call count was when it was recorded
        if (!capturing && ++w.since_probe % ZS_PROBE_EVERY == 0) zs_pack(slot, rows, len, in);
      } else {
        const void* tab = zs_pack(slot, rows, len, in);
        if (rows2)
          GAIB_OR_DIE(gaib_spmm_gemm2_zs(C(), dg, kind, NULL, len, in, tab, agg, W, transW ? 1 : 0, rows2, W2, len_out, out, flags));
        else
          GAIB_OR_DIE(gaib_spmm_gemm_zs(C(), dg, kind, NULL, len, in, tab, agg, W, transW ? 1 : 0, len_out, out, flags));
        return;
      }
    }
  }
  fused_t(dev(g), kind, len, in, (const float*)NULL, 0, prod, flags);
}

// ---- GCN ---------------------------------------------------------------------------------------
void GCN_Aggregator::aggregate_matmul(int len, Graph& g, const float* in, float* agg, bool keep_agg,
                                      const float* W, bool transW, int len_out, float* out, bool relu) {
  aggregate_then_matmul(GAIB_W_GCN, len, g, in, agg, keep_agg, W, transW, len_out, out, relu);
}
void GCN_Aggregator::d_aggregate_matmul(int len, Graph& g, const float* grad_in, float* agg, bool keep_agg,
                                        const float* W, bool transW, int len_out, float* out, bool relu_masked) {
  aggregate_then_matmul(GAIB_W_GCN, len, g, grad_in, agg, keep_agg, W, transW, len_out, out, false, NULL, NULL, relu_masked);
}
void SAGE_Aggregator::aggregate_matmul(int len, Graph& g, const float* in, float* agg, bool keep_agg,
                                       const float* W, bool transW, int len_out, float* out, bool relu,
                                       const float* rows_self, const float* W_self) {
  aggregate_then_matmul(GAIB_W_MEAN, len, g, in, agg, keep_agg, W, transW, len_out, out, relu, rows_self, W_self);
}
void SAGE_Aggregator::d_aggregate_matmul(int len, Graph& g, const float* grad_in, float* agg, bool keep_agg,
                                         const float* W, bool transW, int len_out, float* out,
                                         const float* rows_self, const float* W_self, bool relu_masked) {
  aggregate_then_matmul(GAIB_W_MEAN_T, len, g, grad_in, agg, keep_agg, W, transW, len_out, out, false, rows_self,
                        W_self, relu_masked);
}
void GCN_Aggregator::init(int l, int nv, int, float, float) {
  length = l;
  n = nv;
}
void GCN_Aggregator::aggregate(int len, Graph& g, const float* in, float* out) {
  OpTimer t(OP_SPARSEMM);
  aggregate_rows(g, GAIB_W_GCN, len, in, out, fuse_relu);
  fuse_relu = false;
}
// the normalised adjacency is symmetric, so the derivative is the same operator
void GCN_Aggregator::d_aggregate(int len, Graph& g, const float*, const float* grad_in, float* grad_out) {
  OpTimer t(OP_SPARSEMM);
  aggregate_rows(g, GAIB_W_GCN, len, grad_in, grad_out);
}

// ---- SAGE --------------------------------------------------------------------------------------
void SAGE_Aggregator::init(int l, int nv, int, float, float) {
  length = l;
  n = nv;
}
void SAGE_Aggregator::aggregate(int len, Graph& g, const float* in, float* out) {
  OpTimer t(OP_SPARSEMM);
  aggregate_rows(g, GAIB_W_MEAN, len, in, out, fuse_relu);
  fuse_relu = false;
}
void SAGE_Aggregator::d_aggregate(int len, Graph& g, const float*, const float* grad_in, float* grad_out) {
  OpTimer t(OP_SPARSEMM);
  aggregate_rows(g, GAIB_W_MEAN_T, len, grad_in, grad_out);
}

// ---- GAT ---------------------------------------------------------------------------------------
GAT_Aggregator::GAT_Aggregator()
    : epsilon(0.2f), attn_drop(0.f), attn_scale(1.f), training(true), dropped_last(false), d_norm_scores_drop(NULL),
      d_attn_masks(NULL), drop_cap(0), drop_seed(0xA77E0000ull), num_edges(0), heads(1), d_alpha_l(NULL), d_alpha_r(NULL), d_alpha_lgrad(NULL),
      d_alpha_rgrad(NULL), d_temp_scores(NULL), d_norm_scores(NULL),
      d_norm_scores_grad(NULL), d_norm_scores_t(NULL), fwd_out(NULL), d_tbuf(NULL), tbuf_floats(0), d_ptab(NULL), d_pout(NULL),
      d_prs(NULL), d_pcs(NULL), ptab_floats(0), pvec_floats(0), d_pgrad(NULL), d_prec(NULL), pgrad_floats(0), prec_floats(0),
      part_fused_last(false), d_row_stats(NULL), stats_floats(0), stats_valid(false),
      last_graph(NULL), last_in(NULL), last_len(0), alpha_opt(NULL) {}

void GAT_Aggregator::init(int l, int nv, int ne, float lr, float drop_rate) {
  length = l;
  n = nv;
  attn_drop = drop_rate;
  assert(attn_drop >= 0. && attn_drop < 1.);
  attn_scale = 1.f / (1.f - attn_drop);  // gat_aggregator.cpp:7
  num_edges = (size_t)ne;
  // alpha_l / alpha_r: Glorot over (l, 1) with seeds 2 and 3, as the reference's CPU path
  // (gat_aggregator.cpp:11-12)
  vec_t al, ar;
  init_glorot(l, 1, al, 2);
  init_glorot(l, 1, ar, 3);
  d_alpha_l = gaib_host::dmalloc<float>(l);
  d_alpha_r = gaib_host::dmalloc<float>(l);
  d_alpha_lgrad = gaib_host::dmalloc<float>(l);
  d_alpha_rgrad = gaib_host::dmalloc<float>(l);
  copy_float_device(l, al.data(), d_alpha_l);
  copy_float_device(l, ar.data(), d_alpha_r);
  GAIB_OR_DIE(gaib_fill_f32(C(), l, 0.f, d_alpha_lgrad));
  GAIB_OR_DIE(gaib_fill_f32(C(), l, 0.f, d_alpha_rgrad));
  d_temp_scores = gaib_host::dmalloc<float>(num_edges);
  d_norm_scores = gaib_host::dmalloc<float>(num_edges);
  d_norm_scores_grad = gaib_host::dmalloc<float>(num_edges);
  d_norm_scores_t = gaib_host::dmalloc<float>(num_edges);
  epsilon = 0.2f;
  alpha_opt = new adam(lr);
}

// d_norm_scores (the softmax of this forward) -> p . mask . scale in a buffer of its own: backward needs both the
// undropped attention (softmax backward) and the dropped one (d_dropout of dp, transposed aggregation)
const float* GAT_Aggregator::apply_attn_dropout(size_t n_scores, uint64_t seed, uint64_t* d_seed) {
  size_t masks_cap = drop_cap;  // (the pair shares one capacity)
  grow(d_attn_masks, masks_cap, n_scores);
  grow(d_norm_scores_drop, drop_cap, n_scores);
  OpTimer t(OP_DROPOUT);
  if (d_seed)
    GAIB_OR_DIE(gaib_dropout_dev(C(), (int64_t)n_scores, attn_scale, attn_drop, d_seed, d_norm_scores, d_attn_masks,
                                 d_norm_scores_drop));
  else
    GAIB_OR_DIE(gaib_dropout(C(), (int64_t)n_scores, attn_scale, attn_drop, seed, d_norm_scores, d_attn_masks,
                             d_norm_scores_drop));
  dropped_last = true;
  return d_norm_scores_drop;
}

// the staged forward's draw under the aggregator's next seed.  Option drop_seed_dev with attention dropout staged (gat_fused_drop
// = 0): the counter lives in d_drop_seed, made here on first use (outside any capture) from drop_seed, and gaib_dropout_dev
// advances it -- the host path's seeds, call for call; drop_seed keeps step with every call that runs.  Both options are read
// once, at that first use.
const float* GAT_Aggregator::next_attn_dropout(size_t n_scores) {
  if (seed_dev < 0) {
    seed_dev = gaib_host::drop_seed_dev_option() && !gat_fused_drop_option() ? 1 : 0;
    if (seed_dev) d_drop_seed = gaib_host::new_seed_slot(drop_seed);
  }
  if (!seed_dev) return apply_attn_dropout(n_scores, drop_seed++);
  const float* attn = apply_attn_dropout(n_scores, 0, d_drop_seed);
  if (!gaib_host::capturing()) drop_seed++;
  return attn;
}

void GAT_Aggregator::release() {
  gaib_ctx* c = C();
  float** owned[] = {&d_alpha_l, &d_alpha_r, &d_alpha_lgrad, &d_alpha_rgrad, &d_temp_scores, &d_norm_scores, &d_norm_scores_grad,
                     &d_norm_scores_t, &d_norm_scores_drop, &d_tbuf, &d_ptab, &d_pout, &d_prs, &d_pcs, &d_pgrad, &d_prec,
                     &d_row_stats};
  for (float** p : owned) {
    if (*p) GAIB_OR_DIE(gaib_free(c, *p));
    *p = NULL;
  }
  if (d_attn_masks) GAIB_OR_DIE(gaib_free(c, d_attn_masks));
  d_attn_masks = NULL;
  if (d_drop_seed) GAIB_OR_DIE(gaib_free(c, d_drop_seed));
  d_drop_seed = NULL;
  seed_dev = -1;
  if (d_hb16) GAIB_OR_DIE(gaib_free(c, d_hb16));
  d_hb16 = NULL;
  hb16_elems = 0;
  fwd_bf16 = false;
  drop_cap = tbuf_floats = ptab_floats = pvec_floats = pgrad_floats = prec_floats = stats_floats = 0;
  stats_valid = part_fused_last = dropped_last = drop_fused_last = false;
  last_graph = NULL;
  last_in = fwd_out = NULL;
  if (alpha_opt) {
    alpha_opt->reset();
    delete alpha_opt;
    alpha_opt = NULL;
  }
}

void GAT_Aggregator::set_num_heads(int h) {
  if (h < 1 || length % h != 0) {
    fprintf(stderr, "GAT_Aggregator::set_num_heads(%d): must divide the feature length %d\n", h, length);
    exit(EXIT_FAILURE);
  }
  if (h == heads) return;
  heads = h;
  float** arrays[] = {&d_norm_scores, &d_norm_scores_grad, &d_norm_scores_t};
  for (float** a : arrays) {
    float_free_device(*a);
    *a = gaib_host::dmalloc<float>(num_edges * heads);
  }
  // the temp_scores array only where the kernels do not form the pre-activation score again (see needs_temp)
  if (d_temp_scores) float_free_device(d_temp_scores);
  d_temp_scores = needs_temp() ? gaib_host::dmalloc<float>(num_edges * heads) : NULL;
  if (wide_rows_expected()) {
    // option gat_fused_wide at a shape it covers, without attention dropout or with it kept in the sweep (gat_fused_drop): the
    // one-sweep kernels keep row statistics only, so the [ne][heads] arrays are not held from here on; a staged piece that needs
    // them after all (a partition, gat_fused_fwd / gat_fused_bwd = 0, norm_scores_ptr()) allocates them then (grow_edge_arrays),
    // mask and dropped attention likewise (apply_attn_dropout)
    float** arrays[] = {&d_norm_scores, &d_norm_scores_grad, &d_norm_scores_t, &d_temp_scores};
    for (float** a : arrays) float_free_device(*a);
    num_edges = 0;
  }
}

bool GAT_Aggregator::wide_rows_expected() const {
  return gaib_host::option("gat_fused_wide") == 1 && (attn_drop == 0.f || gat_fused_drop_option()) && gaib_gat_fused_slabs(length, heads, NULL) >= 2;
}

// the [ne][heads] arrays of the staged kernels, for a graph of ne edges: grown where a graph is larger than the one the layer
// was built on (sampling -> full graph), allocated here in the first place where set_num_heads() did not (wide_rows_expected)
void GAT_Aggregator::grow_edge_arrays(size_t ne) {
  if (ne <= num_edges) return;
  num_edges = ne;
  float** arrays[] = {&d_norm_scores, &d_norm_scores_grad, &d_norm_scores_t};
  for (float** a : arrays) {
    float_free_device(*a);
    *a = gaib_host::dmalloc<float>(num_edges * heads);
  }
  if (d_temp_scores || needs_temp()) {
    float_free_device(d_temp_scores);
    d_temp_scores = gaib_host::dmalloc<float>(num_edges * heads);
  }
}

// ---- GAT on a vertex-range partition ("h halo rows for the scores, g halo rows for the transposed
// aggregation") ----
// forward: the halo rows of h arrive while the owned rows are copied into one column table [owned | halo]; scores,
// edge softmax and aggregation then run unchanged on the rank's rectangular graph over that column space.
// backward: the reverse edge of (i -> c) belongs to the rank that owns c, so instead of the reverse-edge permutation the
// rank's TRANSPOSED local structure is used: column sums of g (alpha_r gradient) are row sums over the transpose, and
// the gradient aggregation out_c = sum_i p_(i->c) grad_i is an SpMM over the transpose whose halo rows -- partial sums
// for vertices of other ranks -- travel back to their owners and are added there (gaib_halo_reduce).
void GAT_Aggregator::ensure_partition_buffers(Graph& g, int len) {
  const size_t nc = g.size() + g.gat_n_halo();
  grow_edge_arrays(g.sizeEdges());  // (a no-op unless set_num_heads() left them to the first use)
  size_t pout_cap = ptab_floats, pcs_cap = pvec_floats;  // (each pair shares one capacity)
  grow(d_pout, pout_cap, nc * len);
  grow(d_ptab, ptab_floats, nc * len);
  grow(d_pcs, pcs_cap, nc * heads);
  if (grow(d_prs, pvec_floats, nc * heads))
    GAIB_OR_DIE(gaib_fill_f32(C(), (int64_t)(nc * heads), 0.f, d_prs));  // rows of halo vertices stay 0
  if (!d_temp_scores) d_temp_scores = gaib_host::dmalloc<float>(num_edges * heads);  // the row-side backward reads it
}

void GAT_Aggregator::aggregate_partition(int len, Graph& g, const float* in, float* out) {
  const size_t n_own = g.size(), n_halo = g.gat_n_halo();
  ensure_partition_buffers(g, len);
  dropped_last = false;
  drop_fused_last = false;
  part_fused_last = false;
  // One sweep (gaib_gat_forward_fused_rect) where the shape allows: the chunks over owned columns run while the halo rows
  // of h are on the wire (phase 0), the rest and the per-row combination after they have arrived (phase 1); only the row
  // statistics are kept.  Otherwise (other widths, attention dropout, gat_fused_fwd = 0) the staged pieces.
  bool fused = false;
  {
    OpTimer t(OP_SCORE);
    g.halo_begin(len, in);
    GAIB_OR_DIE(gaib_memcpy_d2d(C(), d_ptab, in, sizeof(float) * n_own * len));
    if (!dropping() && g.gat_symmetric()) {  // (an asymmetric graph: the staged path, which walks the transposed structure)
      grow(d_row_stats, stats_floats, n_own * heads * 2);
      const int rc = gaib_gat_forward_fused_rect(C(), g.gat_full_graph(), len, heads, d_ptab, d_alpha_l, d_alpha_r, epsilon,
                                                 fuse_relu ? 1 : 0, out, d_row_stats, 0);
      if (rc == GAIB_OK) fused = true;
      else if (rc != GAIB_ERR_UNSUPPORTED) GAIB_OR_DIE(rc);
    }
    const float* halo = g.halo_end(len);
    if (n_halo) GAIB_OR_DIE(gaib_memcpy_d2d(C(), d_ptab + n_own * len, halo, sizeof(float) * n_halo * len));
    if (fused) {
      GAIB_OR_DIE(gaib_gat_forward_fused_rect(C(), g.gat_full_graph(), len, heads, d_ptab, d_alpha_l, d_alpha_r, epsilon,
                                              fuse_relu ? 1 : 0, out, d_row_stats, 1));
      fuse_relu = false;
      part_fused_last = true;
      return;
    }
    GAIB_OR_DIE(gaib_gat_scores_mh(C(), g.gat_full_graph(), len, heads, d_ptab, d_alpha_l, d_alpha_r, epsilon,
                                   d_temp_scores, NULL, d_norm_scores));
  }
  const float* attn = dropping() ? next_attn_dropout((size_t)g.sizeEdges() * heads) : d_norm_scores;
  OpTimer t(OP_SPARSEMM);
  GAIB_OR_DIE(gaib_spmm_mh(C(), g.gat_full_graph(), GAIB_W_EDGE, attn, heads, len, d_ptab, out,
                           fuse_relu ? GAIB_RELU : 0));
  fuse_relu = false;
}

void GAT_Aggregator::d_aggregate_partition(int len, Graph& g, const float* grad_in, float* grad_out) {
  const size_t n_own = g.size(), n_halo = g.gat_n_halo(), nc = n_own + n_halo;
  const int64_t ne = (int64_t)g.sizeEdges();
  gaib_graph *full = g.gat_full_graph(), *gt = g.gat_transposed_graph();
  const float* fwd = fwd_out;
  const bool fwd_given = fwd_out_given;
  fwd_out = NULL;
  fwd_out_given = false;
  ensure_partition_buffers(g, len);
  if (part_fused_last && fwd_given) {
    // the one-sweep backward on the rectangular graph: the owner of row i computes everything about i from i's own edge
    // list, given the halo vertices' h rows (d_ptab, from forward), grad rows and (rowdot, max, 1 / sum) records -- two
    // forward-direction exchanges, no transposed structure, no reverse exchange.  The chunks over owned columns run while
    // the grad rows are on the wire.
    OpTimer t(OP_ATTN);
    grow(d_pgrad, pgrad_floats, nc * len);
    grow(d_prec, prec_floats, nc * heads * 4);
    GAIB_OR_DIE(gaib_gat_backward_rec(C(), (int64_t)n_own, len, heads, grad_in, fwd, d_row_stats, d_prec));
    GAIB_OR_DIE(gaib_memcpy_d2d(C(), d_pgrad, grad_in, sizeof(float) * n_own * len));
    g.halo_begin(len, grad_in);
    const int rc = gaib_gat_backward_fused_rect(C(), full, len, heads, d_ptab, d_pgrad, d_prec, d_alpha_l, d_alpha_r, epsilon,
                                                grad_out, d_alpha_lgrad, d_alpha_rgrad, 0);
    const float* halo = g.halo_end(len);  // (every rank ends every exchange it began, whatever rc says)
    if (rc == GAIB_OK) {
      if (n_halo) GAIB_OR_DIE(gaib_memcpy_d2d(C(), d_pgrad + n_own * len, halo, sizeof(float) * n_halo * len));
      g.halo_begin(4 * heads, d_prec);
      halo = g.halo_end(4 * heads);
      if (n_halo) GAIB_OR_DIE(gaib_memcpy_d2d(C(), d_prec + n_own * heads * 4, halo, sizeof(float) * n_halo * heads * 4));
      GAIB_OR_DIE(gaib_gat_backward_fused_rect(C(), full, len, heads, d_ptab, d_pgrad, d_prec, d_alpha_l, d_alpha_r, epsilon,
                                               grad_out, d_alpha_lgrad, d_alpha_rgrad, 1));
      return;
    }
    // forward took the one-sweep path and backward may not (option gat_fused_bwd = 0 on every rank -- options are set per
    // process, the same on all): the exchange above was for nothing, the staged pieces below form the attention again
    if (rc != GAIB_ERR_UNSUPPORTED) GAIB_OR_DIE(rc);
  }
  if (part_fused_last) {  // forward kept statistics only and backward has no forward output to use: the attention, staged
    GAIB_OR_DIE(gaib_gat_scores_mh(C(), full, len, heads, d_ptab, d_alpha_l, d_alpha_r, epsilon, d_temp_scores, NULL,
                                   d_norm_scores));
    part_fused_last = false;
  }
  {
    OpTimer t(OP_SCORE);
    GAIB_OR_DIE(gaib_sddmm_mh(C(), full, len, heads, grad_in, d_ptab, d_norm_scores_grad));
    if (dropped_last)  // d(out)/d(p_e) = mask_e . scale . <grad_i, h_c>
      GAIB_OR_DIE(gaib_d_dropout(C(), ne * heads, attn_scale, d_norm_scores_grad, d_attn_masks, d_norm_scores_grad));
  }
  {
    OpTimer t(OP_ATTN);
    GAIB_OR_DIE(gaib_gat_softmax_bwd_rows(C(), full, heads, d_norm_scores, d_norm_scores_grad, d_temp_scores, epsilon,
                                          d_norm_scores_t /* g_e */, d_prs));
    GAIB_OR_DIE(gaib_edge_gather_perm(C(), ne, heads, g.gat_tperm(), d_norm_scores_t, d_norm_scores_grad));
    GAIB_OR_DIE(gaib_edge_rowsum(C(), gt, heads, d_norm_scores_grad, d_pcs));
    GAIB_OR_DIE(gaib_gat_alpha_grads(C(), (int64_t)nc, len, heads, d_ptab, d_prs, d_pcs, d_alpha_lgrad, d_alpha_rgrad));
  }
  {
    OpTimer t(OP_TRANSPOSE);
    GAIB_OR_DIE(gaib_edge_gather_perm(C(), ne, heads, g.gat_tperm(), dropped_last ? d_norm_scores_drop : d_norm_scores,
                                      d_norm_scores_grad));
  }
  OpTimer t(OP_SPARSEMM);
  GAIB_OR_DIE(gaib_spmm_mh(C(), gt, GAIB_W_EDGE, d_norm_scores_grad, heads, len, grad_in, d_pout, 0));
  GAIB_OR_DIE(gaib_memcpy_d2d(C(), grad_out, d_pout, sizeof(float) * n_own * len));
  GAIB_OR_DIE(gaib_halo_reduce(g.halo_plan(), len, d_pout + n_own * len, grad_out));
}

bool GAT_Aggregator::gat_fused_drop_option() { return gaib_host::option("gat_fused_drop") != 0; }
bool GAT_Aggregator::gat_bf16_tables() { return gaib_host::option("gat_bf16") != 0; }
// bf16 tables on a partitioned GAT graph would need a bf16 exchange of h, grad and record rows: refused, not served in fp32
static void no_gat_bf16_partition() {
  fprintf(stderr, "GPU error: gat_bf16 (GAIB_GAT_DTYPE=bf16) on a partitioned GAT graph: the one-sweep kernels over bf16 tables "
          "run on whole graphs only\n");
  exit(EXIT_FAILURE);
}

// h as bf16 bits in the aggregator's own buffer (kept for backward), grown on demand
const uint16_t* GAT_Aggregator::cast_hb16(size_t elems, const float* in) {
  grow(d_hb16, hb16_elems, elems);
  GAIB_OR_DIE(gaib_cast_f32_bf16(C(), (int64_t)elems, in, d_hb16));
  return d_hb16;
}

void GAT_Aggregator::aggregate(int len, Graph& g, const float* in, float* out) {
  count_edges(g);
  if (g.gat_full_graph() && gat_bf16_tables()) no_gat_bf16_partition();
  if (g.gat_full_graph()) {
    aggregate_partition(len, g, in, out);
    return;
  }
  if (g.has_halo()) {
    fprintf(stderr, "GAT_Aggregator: this partitioned graph was built without build_gat_structures()\n");
    exit(EXIT_FAILURE);
  }
  // dense graphs at 64 columns: scores, edge softmax and aggregation in ONE sweep; only the row statistics (maximum,
  // 1 / sum) are kept and backward forms the attention again -- no [ne][heads] array is written or read.  norm_scores_ptr()
  // materialises the attention on demand (tests, checkpoints).
  dropped_last = false;
  drop_fused_last = false;
  const bool drop_sweep = dropping() && gat_fused_drop_option();
  if (!dropping() || drop_sweep) grow(d_row_stats, stats_floats, (size_t)g.size() * heads * 2);
  if (drop_sweep) {
    // attention dropout inside the sweep (option gat_fused_drop): the masks of the staged path's next seed, no edge array
    OpTimer t(OP_SPARSEMM);
    // bf16 tables (option gat_bf16): the sweep gathers the aggregator's own bf16 copy of h; where that call does not apply the
    // fp32 sweep runs under the same seed, which advances once either way
    bool on_bf16 = false;
    int rc = GAIB_ERR_UNSUPPORTED;
    if (gat_bf16_tables()) {
      rc = gaib_gat_forward_fused_drop_bf16(C(), dev(g), len, heads, cast_hb16((size_t)g.size() * len, in), d_alpha_l, d_alpha_r,
                                            epsilon, fuse_relu ? 1 : 0, attn_drop, attn_scale, drop_seed, out, d_row_stats);
      on_bf16 = rc == GAIB_OK;
    }
    if (rc == GAIB_ERR_UNSUPPORTED)
      rc = gaib_gat_forward_fused_drop(C(), dev(g), len, heads, in, d_alpha_l, d_alpha_r, epsilon, fuse_relu ? 1 : 0, attn_drop,
                                       attn_scale, drop_seed, out, d_row_stats);
    if (rc == GAIB_OK) {
      drop_seed_last = drop_seed++;
      drop_fused_last = drop_sweep_ran = true;
      fuse_relu = false;
      fwd_bf16 = on_bf16;
      stats_valid = true;  // (the statistics are the undropped softmax's: materialise_scores() serves them as ever)
      last_graph = &g;
      last_in = in;
      last_len = len;
      return;
    }
    if (rc != GAIB_ERR_UNSUPPORTED) GAIB_OR_DIE(rc);  // UNSUPPORTED: the staged path draws this seed itself
  }
  if (!dropping()) {
    OpTimer t(OP_SPARSEMM);
    fwd_bf16 = false;
    int rc = GAIB_ERR_UNSUPPORTED;
    if (gat_bf16_tables()) {
      rc = gaib_gat_forward_fused_bf16(C(), dev(g), len, heads, cast_hb16((size_t)g.size() * len, in), d_alpha_l, d_alpha_r, epsilon,
                                       fuse_relu ? 1 : 0, out, d_row_stats);
      fwd_bf16 = rc == GAIB_OK;
    }
    if (rc == GAIB_ERR_UNSUPPORTED)
      rc = gaib_gat_forward_fused(C(), dev(g), len, heads, in, d_alpha_l, d_alpha_r, epsilon, fuse_relu ? 1 : 0, out,
                                  d_row_stats);
    if (rc == GAIB_OK) {
      fuse_relu = false;
      stats_valid = true;
      last_graph = &g;
      last_in = in;
      last_len = len;
      return;
    }
    if (rc != GAIB_ERR_UNSUPPORTED) GAIB_OR_DIE(rc);
  }
  stats_valid = false;
  fwd_bf16 = false;
  grow_edge_arrays(g.sizeEdges());  // a larger graph than the one the layer was built on (sampling -> full graph)
  {
    OpTimer t(OP_SCORE);
    // the leaky-relu output itself is not materialised (NULL): nothing downstream reads it
    // nor is the pre-activation score where backward can form its sign again (d_temp_scores stays NULL then)
    GAIB_OR_DIE(gaib_gat_scores_mh(C(), dev(g), len, heads, in, d_alpha_l, d_alpha_r, epsilon, d_temp_scores,
                                   NULL, d_norm_scores));
  }
  const float* attn = dropping() ? next_attn_dropout((size_t)g.sizeEdges() * heads) : d_norm_scores;
  OpTimer t(OP_SPARSEMM);
  GAIB_OR_DIE(gaib_spmm_mh(C(), dev(g), GAIB_W_EDGE, attn, heads, len, in, out, fuse_relu ? GAIB_RELU : 0));
  fuse_relu = false;
}

// feat_in and grad_out may be the same buffer (GAT_layer::backward passes out_temp for both):
// feat_in is last read by the alpha-gradient step, grad_out is first written by the final SpMM.
void GAT_Aggregator::d_aggregate(int len, Graph& g, const float* feat_in, const float* grad_in,
                                 float* grad_out) {
  count_edges(g);
  if (g.gat_full_graph() && gat_bf16_tables()) no_gat_bf16_partition();
  if (g.gat_full_graph()) {
    d_aggregate_partition(len, g, grad_in, grad_out);
    return;
  }
  if (drop_fused_last) {
    // forward dropped inside the sweep: backward through the same masks, formed again from the kept seed
    drop_fused_last = false;
    int rc = GAIB_ERR_UNSUPPORTED;
    if (fwd_out && stats_valid && feat_in == last_in && &g == last_graph && len == last_len) {
      OpTimer t(OP_ATTN);
      const size_t need = (size_t)g.size() * len;
      grow(d_tbuf, tbuf_floats, need);
      // bf16 tables: the kept copy of h is reused, one cast (of grad_in) is made (the guard above is the bf16 call's own)
      if (fwd_bf16)
        rc = gaib_gat_backward_fused_drop_bf16(C(), dev(g), len, heads, d_hb16, to_bf16(g.size(), len, grad_in), fwd_out, d_alpha_l,
                                               d_alpha_r, d_row_stats, epsilon, attn_drop, attn_scale, drop_seed_last, d_tbuf,
                                               d_alpha_lgrad, d_alpha_rgrad);
      if (rc == GAIB_ERR_UNSUPPORTED)
        rc = gaib_gat_backward_fused_drop(C(), dev(g), len, heads, feat_in, grad_in, fwd_out, d_alpha_l, d_alpha_r, d_row_stats,
                                          epsilon, attn_drop, attn_scale, drop_seed_last, d_tbuf, d_alpha_lgrad, d_alpha_rgrad);
      if (rc == GAIB_OK) {
        fwd_out = NULL;
        fwd_out_given = false;
        GAIB_OR_DIE(gaib_memcpy_d2d(C(), grad_out, d_tbuf, sizeof(float) * need));
        return;
      }
      if (rc != GAIB_ERR_UNSUPPORTED) GAIB_OR_DIE(rc);
    }
    // the sweep may not run (gat_fused_bwd = 0, no forward output): the attention array, then mask and dropped attention drawn
    // again under the kept seed -- the bits the forward sweep used -- and the staged pieces below
    materialise_scores();
    apply_attn_dropout((size_t)g.sizeEdges() * heads, drop_seed_last);
  }
  if (fwd_out && !dropped_last) {
    // one sweep over the edges instead of four (gaib_gat_backward_fused): needs the layer's forward output and an
    // output that does not alias feat_in (GAT_layer::backward passes out_temp for both) -> a scratch of its own
    OpTimer t(OP_ATTN);
    const size_t need = (size_t)g.size() * len;
    grow(d_tbuf, tbuf_floats, need);
    int rc = GAIB_ERR_UNSUPPORTED;
    // bf16 tables: the kept copy of h is reused, one cast (of grad_in) is made
    if (fwd_bf16 && stats_valid && feat_in == last_in && &g == last_graph && len == last_len)
      rc = gaib_gat_backward_fused_bf16(C(), dev(g), len, heads, d_hb16, to_bf16(g.size(), len, grad_in), fwd_out, d_alpha_l,
                                        d_alpha_r, d_row_stats, epsilon, d_tbuf, d_alpha_lgrad, d_alpha_rgrad);
    if (rc == GAIB_ERR_UNSUPPORTED)
      rc = gaib_gat_backward_fused(C(), dev(g), len, heads, feat_in, grad_in, fwd_out, d_alpha_l, d_alpha_r,
                                   stats_valid ? NULL : d_norm_scores, stats_valid ? d_row_stats : NULL, epsilon, d_tbuf,
                                   d_alpha_lgrad, d_alpha_rgrad);
    if (rc == GAIB_OK) {
      fwd_out = NULL;
      fwd_out_given = false;
      GAIB_OR_DIE(gaib_memcpy_d2d(C(), grad_out, d_tbuf, sizeof(float) * need));
      return;
    }
    if (rc != GAIB_ERR_UNSUPPORTED) GAIB_OR_DIE(rc);  // a real failure; UNSUPPORTED = this shape / graph takes the staged path
  }
  if (stats_valid) materialise_scores();  // (the staged kernels read the attention array)
  grow_edge_arrays(g.sizeEdges());        // (a no-op unless set_num_heads() left the arrays to the first use)
  {
    OpTimer t(OP_SCORE);
    GAIB_OR_DIE(gaib_sddmm_mh(C(), dev(g), len, heads, grad_in, feat_in, d_norm_scores_grad));
    if (dropped_last)  // d(out)/d(p_e) = mask_e . scale . <grad_i, h_c>; sum_e p_e dp_e is still <grad_i, out_i>
      GAIB_OR_DIE(gaib_d_dropout(C(), (int64_t)(g.sizeEdges() * heads), attn_scale, d_norm_scores_grad, d_attn_masks,
                                 d_norm_scores_grad));
  }
  {
    OpTimer t(OP_ATTN);
    // with the layer's forward output at hand the softmax backward is one pass over the edge arrays:
    // sum_e p_e dp_e == <grad_i, out_i> (out_i = sum_e p_e h_col; where relu cut out_i the gradient is 0 too)
    const float* fwd = fwd_out;
    fwd_out = NULL;
    fwd_out_given = false;
    // the pass that walks rev anyway also leaves the transposed attention p[rev(e)] in d_norm_scores_t, so the
    // gradient aggregation reads its weights linearly
    if (d_temp_scores)
      GAIB_OR_DIE(gaib_gat_softmax_bwd_alpha_ex(C(), dev(g), len, heads, feat_in, d_norm_scores, d_norm_scores_grad,
                                                d_temp_scores, epsilon, NULL, d_alpha_lgrad, d_alpha_rgrad,
                                                fwd ? grad_in : NULL, fwd, d_norm_scores_t));
    else
      GAIB_OR_DIE(gaib_gat_softmax_bwd_alpha_re(C(), dev(g), len, heads, feat_in, d_alpha_l, d_alpha_r, d_norm_scores,
                                                d_norm_scores_grad, epsilon, NULL, d_alpha_lgrad, d_alpha_rgrad,
                                                fwd ? grad_in : NULL, fwd, d_norm_scores_t));
  }
  if (dropped_last) {  // the gradient flows back along the DROPPED attention: its transpose replaces the undropped one
    OpTimer t2(OP_TRANSPOSE);
    GAIB_OR_DIE(gaib_edge_transpose_mh(C(), dev(g), heads, d_norm_scores_drop, d_norm_scores_t));
  }
  OpTimer t(OP_SPARSEMM);
  GAIB_OR_DIE(gaib_spmm_mh(C(), dev(g), GAIB_W_EDGE, d_norm_scores_t, heads, len, grad_in, grad_out, 0));
}

// the attention [ne][heads] of the last forward, for callers that want the array the one-sweep forward did not write
void GAT_Aggregator::materialise_scores() {
  if (!stats_valid || !last_graph) return;
  Graph& g = *last_graph;
  grow_edge_arrays(g.sizeEdges());
  GAIB_OR_DIE(gaib_gat_scores_mh(C(), dev(g), last_len, heads, last_in, d_alpha_l, d_alpha_r, epsilon, d_temp_scores, NULL,
                                 d_norm_scores));
  stats_valid = false;
}
float* GAT_Aggregator::norm_scores_ptr() {
  materialise_scores();
  return d_norm_scores;
}

void GAT_Aggregator::update_weights(optimizer*) {
  alpha_opt->update_gpu(length, d_alpha_lgrad, d_alpha_l);
  alpha_opt->update_gpu(length, d_alpha_rgrad, d_alpha_r);
}
