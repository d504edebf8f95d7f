// context.cpp -- process-wide device context + per-op timers of the host API.
#include <chrono>
#include <string>
#include "gpu_context.h"
#include "global.h"
#include "host_util.h"

std::map<char, double> time_ops;  // declared extern in include/gnn/global.h (reference: train.cpp:3)

static gaib_ctx* g_ctx = nullptr;
static bool g_sync_timers = false;
static gaib_comm* g_comm = nullptr;
static unsigned g_generation = 0;
unsigned gpu_context::generation() { return g_generation; }

static unsigned long long g_agg_edges = 0;
void gpu_context::add_aggregated_edges(unsigned long long n) { g_agg_edges += n; }
unsigned long long gpu_context::aggregated_edges() { return g_agg_edges; }
void gpu_context::set_comm(gaib_comm* comm) { g_comm = comm; }
gaib_comm* gpu_context::comm() { return g_comm; }

void gpu_context::check(int status, const char* what) {
  if (status == GAIB_OK) return;
  // reference convention: report and exit (include/utils/cutils.h:18-28,133-174)
  fprintf(stderr, "GPU error in %s: %s (status %d)\n", what, gaib_last_error(), status);
  exit(EXIT_FAILURE);
}

// "0" / "1" -> 0 / 1, anything else -> -1 (the 0|1 switches of the environment)
int gpu_context::parse_switch(const char* value) {
  if (!value || !value[0] || value[1]) return -1;
  return value[0] == '0' ? 0 : (value[0] == '1' ? 1 : -1);
}

void gpu_context::set(int device, void* hip_stream) {
  if (g_ctx) {
    gaib_ctx_destroy(g_ctx);
    g_ctx = nullptr;
  }
  check(gaib_ctx_create(device, hip_stream, &g_ctx), "gaib_ctx_create");
  g_generation++;
  const char* s = getenv("GAIB_SYNC_TIMERS");
  g_sync_timers = s && atoi(s) != 0;
  // development knobs for A/B runs of the drivers: GAIB_OPTS="key=value,key=value" -> gaib_set_option
  if (const char* o = getenv("GAIB_OPTS")) {
    std::string opts(o);
    size_t pos = 0;
    while (pos < opts.size()) {
      size_t end = opts.find(',', pos);
      if (end == std::string::npos) end = opts.size();
      const std::string kv = opts.substr(pos, end - pos);
      const size_t eq = kv.find('=');
      if (eq != std::string::npos) {
        check(gaib_set_option(g_ctx, kv.substr(0, eq).c_str(), atoll(kv.c_str() + eq + 1)), "gaib_set_option (GAIB_OPTS)");
        fprintf(stderr, "[gaib] option %s\n", kv.c_str());
      }
      pos = end + 1;
    }
  }
  // the precision of the aggregations' feature tables (GCN / SAGE): fp32 (default), bf16, or fp8 with per-row scales -- a
  // user-facing switch, so that a driver linked against the layer library gets narrow tables without code changes
  if (const char* d = getenv("GAIB_AGG_DTYPE")) {
    const std::string dt(d);
    if (dt != "fp32" && dt != "bf16" && dt != "fp8") {
      fprintf(stderr, "GAIB_AGG_DTYPE=%s: expected fp32, bf16 or fp8\n", d);
      exit(EXIT_FAILURE);
    }
    check(gaib_set_option(g_ctx, "agg_bf16", dt == "bf16" ? 1 : 0), "gaib_set_option (GAIB_AGG_DTYPE)");
    check(gaib_set_option(g_ctx, "agg_fp8", dt == "fp8" ? 1 : 0), "gaib_set_option (GAIB_AGG_DTYPE)");
  }
  // the dense self products of the SAGE layers under bf16 tables: fp32 rows (default) or the bf16 table with exactly split
  // weights (option gemm_bf16; without GAIB_AGG_DTYPE=bf16 there is no table and nothing changes)
  if (const char* d = getenv("GAIB_GEMM_DTYPE")) {
    const std::string dt(d);
    if (dt != "fp32" && dt != "bf16") {
      fprintf(stderr, "GAIB_GEMM_DTYPE=%s: expected fp32 or bf16\n", d);
      exit(EXIT_FAILURE);
    }
    check(gaib_set_option(g_ctx, "gemm_bf16", dt == "bf16" ? 1 : 0), "gaib_set_option (GAIB_GEMM_DTYPE)");
  }
  // relu-masked gradients of 256 columns gathered zero-suppressed on the K-slab route (option agg_zs_wide; off by default)
  if (const char* d = getenv("GAIB_AGG_ZS_WIDE")) {
    const std::string v(d);
    if (v != "0" && v != "1") {
      fprintf(stderr, "GAIB_AGG_ZS_WIDE=%s: expected 0 or 1\n", d);
      exit(EXIT_FAILURE);
    }
    check(gaib_set_option(g_ctx, "agg_zs_wide", v == "1" ? 1 : 0), "gaib_set_option (GAIB_AGG_ZS_WIDE)");
  }
  // sampled training (subg_size > 0): every epoch's subgraph, feature rows and label rows built on the device (option
  // sampler_device; off by default)
  if (const char* d = getenv("GAIB_SAMPLER_DEVICE")) {
    const int v = parse_switch(d);
    if (v < 0) {
      fprintf(stderr, "GAIB_SAMPLER_DEVICE=%s: expected 0 or 1\n", d);
      exit(EXIT_FAILURE);
    }
    check(gaib_set_option(g_ctx, "sampler_device", v), "gaib_set_option (GAIB_SAMPLER_DEVICE)");
  }
  // GAT with attention dropout (score_drop > 0): mask, forward and backward inside the one-sweep kernels (option gat_fused_drop;
  // off by default)
  if (const char* d = getenv("GAIB_GAT_FUSED_DROP")) {
    const int v = parse_switch(d);
    if (v < 0) {
      fprintf(stderr, "GAIB_GAT_FUSED_DROP=%s: expected 0 or 1\n", d);
      exit(EXIT_FAILURE);
    }
    check(gaib_set_option(g_ctx, "gat_fused_drop", v), "gaib_set_option (GAIB_GAT_FUSED_DROP)");
  }
  // dropout mask seeds in device memory (option drop_seed_dev; off by default): feature dropout and staged attention dropout
  // draw with gaib_dropout_dev, which lets the trainer record an epoch under dropout
  if (const char* d = getenv("GAIB_DROP_SEED_DEV")) {
    const int v = parse_switch(d);
    if (v < 0) {
      fprintf(stderr, "GAIB_DROP_SEED_DEV=%s: expected 0 or 1\n", d);
      exit(EXIT_FAILURE);
    }
    check(gaib_set_option(g_ctx, "drop_seed_dev", v), "gaib_set_option (GAIB_DROP_SEED_DEV)");
  }
  // GAT layers with multi-head rows wider than 128 columns (8 heads x 32, 8 x 64): the one-sweep kernels per column slab (option
  // gat_fused_wide; off by default)
  if (const char* d = getenv("GAIB_GAT_WIDE")) {
    const int v = parse_switch(d);
    if (v < 0) {
      fprintf(stderr, "GAIB_GAT_WIDE=%s: expected 0 or 1\n", d);
      exit(EXIT_FAILURE);
    }
    check(gaib_set_option(g_ctx, "gat_fused_wide", v), "gaib_set_option (GAIB_GAT_WIDE)");
  }
  // the same switch for GAT (option gat_bf16): its one-sweep forward and backward gather bf16 copies of h and grad
  if (const char* d = getenv("GAIB_GAT_DTYPE")) {
    const std::string dt(d);
    if (dt != "fp32" && dt != "bf16") {
      fprintf(stderr, "GAIB_GAT_DTYPE=%s: expected fp32 or bf16\n", d);
      exit(EXIT_FAILURE);
    }
    check(gaib_set_option(g_ctx, "gat_bf16", dt == "bf16" ? 1 : 0), "gaib_set_option (GAIB_GAT_DTYPE)");
  }
}

gaib_ctx* gpu_context::get() {
  if (!g_ctx) {
    int dev = 0;
    if (const char* e = getenv("GAIB_DEVICE")) dev = atoi(e);
    else if (const char* l = getenv("LOCAL_RANK")) {
      // rank -> device: round robin over the visible devices (more ranks than devices: a one-GPU box, peer-to-peer transport)
      int ndev = 0;
      check(gaib_device_count(&ndev), "gaib_device_count");
      dev = ndev > 0 ? atoi(l) % ndev : 0;
    }
    set(dev, nullptr);
  }
  return g_ctx;
}

void gpu_context::sync() { check(gaib_sync(get()), "gaib_sync"); }

static bool overlap_enabled() {
  static int on = -1;
  if (on < 0) {
    // opt-in: on MI355X the aggregation already saturates HBM and the wave slots, so running the
    // weight-gradient GEMM next to it measured no gain; kept for narrower graphs
    const char* e = getenv("GAIB_OVERLAP");
    on = (e && atoi(e) != 0) ? 1 : 0;
  }
  return on == 1;
}
void gpu_context::side_begin() {
  if (overlap_enabled()) check(gaib_side_begin(get()), "gaib_side_begin");
}
void gpu_context::side_end() {
  if (overlap_enabled()) check(gaib_side_end(get()), "gaib_side_end");
}
void gpu_context::side_wait() {
  if (overlap_enabled()) check(gaib_side_wait(get()), "gaib_side_wait");
}

namespace gaib_host {
static double now() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
OpTimer::OpTimer(char op) : op_(op), t0_(0) {
  if (g_sync_timers) {
    gpu_context::sync();
    t0_ = now();
  }
}
OpTimer::~OpTimer() {
  if (g_sync_timers) {
    gpu_context::sync();
    time_ops[op_] += now() - t0_;
  }
}
}  // namespace gaib_host
