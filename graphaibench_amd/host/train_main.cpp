// train_main.cpp -- full-batch GNN trainer on one MI355X with the reference's command line and log
// lines, so that scripts written for GraphAIBench's cpu_train_* / gpu_train_* binaries
// (scripts/run-sage-products.sh, README "Example: ./bin/cpu_train_gcn citeseer 10 2 softmax") work:
//
//   gpu_train_{gcn,sage,gat} data num_epochs num_threads type_loss [hidden(16) score_drop(0.)
//        feat_drop(0.) learning_rate(0.02) [num_layers(2) subg_size(0) val_interval(50) inductive(0)]]
//
// This is our own driver over the layer API of include/ (the reference's src/gnn/net.cpp cannot run as
// shipped: it exits right after loading the labels, net.cpp:150-154).  Control flow per epoch follows
// Model::train / forward_prop / backward_prop (net.cpp:361-419, 457-502, 580-615): gconv layers ->
// [l2norm -> dense for GAT] -> softmax loss; masks are the contiguous ranges of graph.meta.txt;
// GCN/GAT share one Adam instance across layers, GraphSAGE layers own theirs (quirk Q6).
// Architecture is a compile-time choice like in the reference: -DUSE_SAGE / -DUSE_GAT.
//
// One process per GPU (no reference counterpart): launched N times with RANK / WORLD_SIZE / LOCAL_RANK
// (torchrun's variables; GAIB_RANK / GAIB_WORLD override), GCN, GraphSAGE and GAT train on a vertex-range partition:
// every rank reads the (global) dataset, keeps the rows [lo, hi) of its range (include/gnn/partition.h), exchanges
// halo feature rows before every aggregation and sums the weight gradients before every optimizer step, all behind
// the C ABI (gaib_comm_* / gaib_halo_* / gaib_allreduce_f32; transport GAIB_COMM=rccl|ipc).  The run's ncclUniqueId
// travels from rank 0 to the others through the file GAIB_COMM_ID_FILE (default /dev/shm/gaib_id_<MASTER_PORT>).
// Loss / accuracy are all-reduced; rank 0 prints the reference's log lines.  Any rank that fails exits non-zero and
// the others follow (deadline in every wait).
// One command for N GPUs: GAIB_RANKS=N bin/gpu_train_gcn <the reference's arguments> -- the process then is a LAUNCHER
// (no GPU API is touched in it): it starts N copies of itself with RANK / WORLD_SIZE / LOCAL_RANK set and an id file of
// this launch, forwards rank 0's output, and when a rank exits non-zero (or GAIB_RANKS_DEADLINE_S passes) stops the
// others and exits non-zero -- one entry point drives all devices, as the reference's multi-GPU programs do from one
// main (src/triangle/multigpu_induced.cu:31-84); RCCL itself has no deadline for a peer that died.
#include <omp.h>
#include <algorithm>
#include <string>
#include <vector>
#include <fcntl.h>
#include <signal.h>
#include <sys/stat.h>
#include <sys/wait.h>
#include <time.h>
#include <unistd.h>
#include "partition.h"
#include "cutils.h"
#include "dense_layer.h"
#include "graph_conv_layer.h"
#include "host_util.h"
#include "l2norm_layer.h"
#include "math_functions.hh"
#include "reader.h"
#include "sampler.h"
#include "softmax_loss_layer.h"

#if defined(USE_GAT)
typedef GAT_layer gconv_t;
static const gnn_arch ARCH = gnn_arch::GAT;
static const char* ARCH_NAME = "Graph Attention Network";
#elif defined(USE_SAGE)
typedef SAGE_layer gconv_t;
static const gnn_arch ARCH = gnn_arch::SAGE;
static const char* ARCH_NAME = "GraphSAGE";
#else
typedef GCN_layer gconv_t;
static const gnn_arch ARCH = gnn_arch::GCN;
static const char* ARCH_NAME = "Graph Convolutional Network";
#endif

namespace {

struct Trainer {
  // configuration (positional CLI, net.cpp:13-64)
  std::string dataset;
  int num_epochs = 0, num_threads = 1, dim_hid = DEFAULT_SIZE_HID, num_layers = DEFAULT_NUM_LAYER;
  int subg_size = 0, val_interval = EVAL_INTERVAL, inductive = 0;
  float feat_drop = 0.f, score_drop = 0.f, lrate = DEFAULT_RATE_LEARN;
  bool use_dense = false, use_l2norm = false;
  // data
  Graph* graph = nullptr;
  int num_samples = 0, dim_init = 0, num_cls = 0;
  size_t train_begin = 0, train_end = 0, train_count = 0, val_begin = 0, val_end = 0, val_count = 0;
  size_t test_begin = 0, test_end = 0, test_count = 0;
  float* d_features = nullptr;
  label_t* d_labels = nullptr;
  mask_t *d_masks_train = nullptr, *d_masks_val = nullptr, *d_masks_test = nullptr;
  // sampling (GraphSAINT-style; net.cpp:156-176, 288-358)
  Graph* training_graph = nullptr;
  Sampler* sampler = nullptr;
  std::vector<Graph*> subgs;
  std::vector<mask_t> subg_masks;
  std::vector<float> feats_host;
  std::vector<label_t> labels_host;
  std::vector<mask_t> masks_train_host;
  int num_subgraphs = 1, subg_nv = 0;
  float* d_feats_subg = nullptr;
  label_t* d_labels_subg = nullptr;
  // option sampler_device (GAIB_SAMPLER_DEVICE=1): the subgraph, its feature rows and its label rows are built on the device
  bool sampler_device = false;
  std::vector<VertexSet> subg_sets;  // the sampled vertex sets of the round (device path: the subgraph is induced per epoch)
  int64_t* d_rows_subg = nullptr;    // [subg_size] the kept ids of the epoch's subgraph
  // network
  std::vector<gconv_t> layers;
  l2norm_layer* l2 = nullptr;
  dense_layer* dense = nullptr;
  loss_layer* loss = nullptr;  // softmax (single label) or sigmoid (multi label, argv[4])
  bool is_sigmoid = false;
  size_t label_width = 1;      // bytes of label per vertex: 1, or num_cls for multi-hot rows
  // one process per GPU
  int rank = 0, world = 1;
  gaib_comm* comm = nullptr;
  VertexRangePartition part;
  size_t g_train_begin = 0, g_train_end = 0, g_val_begin = 0, g_val_end = 0, g_test_begin = 0, g_test_end = 0;  // global
  bool root() const { return rank == 0; }
  // recorded epochs (HIP graphs, gaib_capture_*): forward + loss + metrics as one launch, backward + optimizer steps as
  // another.  For launch-bound models (the reference's shipped cora / citeseer: ~40 kernels of microseconds per epoch).
  bool graph_mode = false;
  gaib_exec *fw_exec = nullptr, *bw_exec = nullptr;
  char* d_metrics = nullptr;  // float loss, float accuracy, (8 bytes unused), uint64 tp, fp, fn
  char* h_metrics = nullptr;  // the same 40 bytes in pinned host memory, copied at the end of the forward recording
  static constexpr size_t METRICS_BYTES = 40;

  static int env_int(const char* a, const char* b, int dflt) {
    const char* v = getenv(a);
    if (!v && b) v = getenv(b);
    return v ? atoi(v) : dflt;
  }

  // rank 0 draws the communicator id and hands it to the other ranks through a file (one node)
  void init_comm() {
    rank = env_int("GAIB_RANK", "RANK", 0);
    world = env_int("GAIB_WORLD", "WORLD_SIZE", 1);
    if (world <= 1) return;
    const char* tr = getenv("GAIB_COMM");
    int transport = (tr && std::string(tr) == "ipc") ? GAIB_COMM_IPC : GAIB_COMM_RCCL;
    int ndev = 0;
    GAIB_OR_DIE(gaib_device_count(&ndev));
    if (!tr && world > ndev) {  // ranks share devices (a one-GPU box): RCCL refuses that, the peer-to-peer pull does not
      transport = GAIB_COMM_IPC;
      if (rank == 0) std::cerr << world << " ranks on " << ndev << " device(s): GAIB_COMM=ipc\n";
    }
    std::string path = getenv("GAIB_COMM_ID_FILE") ? getenv("GAIB_COMM_ID_FILE")
                                                  : std::string("/dev/shm/gaib_id_") +
                                                        (getenv("MASTER_PORT") ? getenv("MASTER_PORT") : "default");
    unsigned char id[GAIB_COMM_ID_BYTES];
    // a file left behind by a crashed run under the same name must not be taken for this run's id: rank 0 removes
    // the name before it draws the id, and the others ignore a file written well before they started (the launcher
    // -- GAIB_RANKS, bench.py -- gives every launch a name of its own, so this only matters for hand-started ranks)
    const time_t started = time(nullptr);
    if (rank == 0) {
      unlink(path.c_str());
      GAIB_OR_DIE(gaib_comm_unique_id(transport, id));
      const std::string tmp = path + ".tmp";
      FILE* f = fopen(tmp.c_str(), "wb");
      if (!f || fwrite(id, 1, sizeof(id), f) != sizeof(id)) {
        std::cerr << "cannot write " << tmp << "\n";
        exit(EXIT_FAILURE);
      }
      fclose(f);
      rename(tmp.c_str(), path.c_str());
    } else {
      const double deadline = omp_get_wtime() + 120.0;
      size_t got = 0;
      while (omp_get_wtime() < deadline) {
        struct stat st;
        FILE* f = (stat(path.c_str(), &st) == 0 && st.st_mtime + 60 >= started) ? fopen(path.c_str(), "rb") : nullptr;
        if (f) {
          got = fread(id, 1, sizeof(id), f);
          fclose(f);
          if (got == sizeof(id)) break;
        }
        usleep(2000);
      }
      if (got != sizeof(id)) {
        std::cerr << "rank " << rank << ": no communicator id at " << path << " after 120 s\n";
        exit(EXIT_FAILURE);
      }
    }
    GAIB_OR_DIE(gaib_comm_init(gpu_context::get(), rank, world, id, transport, &comm));
    if (rank == 0) unlink(path.c_str());  // gaib_comm_init is collective: everybody has read it
    gpu_context::set_comm(comm);
  }

  // intersect a global mask range with this rank's rows, in local row ids
  void local_range(size_t gb, size_t ge, size_t& b, size_t& e) const {
    const size_t lo = (size_t)part.lo, hi = (size_t)part.hi;
    const size_t x = std::max(gb, lo), y = std::min(ge, hi);
    b = x < y ? x - lo : 0;
    e = x < y ? y - lo : 0;
  }

  void parse(int argc, char** argv) {
    dataset = argv[1];
    num_epochs = atoi(argv[2]);
    num_threads = atoi(argv[3]);
    omp_set_num_threads(num_threads);
    is_sigmoid = std::string(argv[4]) == "sigmoid";  // train.cpp:20
    if (argc >= 6) dim_hid = atoi(argv[5]);
    if (argc >= 7) score_drop = atof(argv[6]);
    if (argc >= 8) feat_drop = atof(argv[7]);
    if (argc >= 9) lrate = atof(argv[8]);
    if (argc > 9) {
      assert(argc == 13);
      num_layers = atoi(argv[9]);
      subg_size = atoi(argv[10]);
      val_interval = atoi(argv[11]);
      inductive = atoi(argv[12]);
    }
    assert(num_layers >= 2);
    // l2norm + dense head for sampling and GAT (net.cpp:69-71)
    if (subg_size > 0 || ARCH == gnn_arch::GAT) use_l2norm = use_dense = true;
    if (subg_size > 0) inductive = 1;  // net.cpp:160
    // fp8 tables (GAIB_AGG_DTYPE=fp8, context option agg_fp8) take whole graphs: refused on more than one rank BEFORE the
    // communicator is built -- every rank reads the same environment and leaves alike, none waits in a collective
    const bool fp8 = aggregator::fp8_tables();
    if (fp8 && env_int("GAIB_WORLD", "WORLD_SIZE", 1) > 1) {
      std::cerr << "GAIB_AGG_DTYPE=fp8 (agg_fp8) runs on one GPU only: fp8 feature tables have no halo exchange and no row-class kernels\n";
      exit(EXIT_FAILURE);
    }
    init_comm();
    if (ARCH == gnn_arch::GAT) {
      // GAT's own tables: fp32, or bf16 with GAIB_GAT_DTYPE=bf16 (context option gat_bf16; whole graphs only)
      const int64_t gat16 = gaib_host::option("gat_bf16");
      if (gat16 && world > 1) {  // (every rank reads the same environment: refused before any collective)
        std::cerr << "GAIB_GAT_DTYPE=bf16 (gat_bf16) runs on one GPU only: the one-sweep GAT kernels over bf16 tables take whole graphs\n";
        exit(EXIT_FAILURE);
      }
      if (world == 1) std::cout << "GAT tables: " << (gat16 ? "bf16" : "fp32") << "\n";
    }
    // the aggregations' feature tables: fp32, or bf16 with GAIB_AGG_DTYPE=bf16 (context option agg_bf16; GCN / SAGE only -- GAT has GAIB_GAT_DTYPE / gat_bf16)
    const bool bf16 = aggregator::bf16_tables();
    if (world > 1) {
      // every rank reads the same environment; one that does not would exchange rows of another element size (the peer-to-peer
      // transport refuses that at the first exchange, RCCL would mismatch its counts): agree before anything is built
      double v[1] = {bf16 ? 1.0 : 0.0};
      GAIB_OR_DIE(gaib_allreduce_host_f64(comm, v, 1));
      if (v[0] != 0.0 && v[0] != (double)world) {
        std::cerr << "rank " << rank << ": GAIB_AGG_DTYPE differs between the ranks (" << (int)v[0] << " of " << world << " ask for bf16)\n";
        exit(EXIT_FAILURE);
      }
    }
    // (fp8 tables say so on a line of their own; GAT gathers fp32 whatever the option says)
    if (fp8 && root())
      std::cout << "[gaib] aggregation tables: " << (ARCH == gnn_arch::GAT ? "fp32 (fp8 asked; GAT gathers fp32)" : "fp8") << "\n";
    else if (root())
      std::cout << "aggregation tables: "
                << (bf16 ? (ARCH == gnn_arch::GAT ? "fp32 (bf16 asked; GAT gathers fp32)"
                                                  : (world > 1 ? "bf16 (odd widths on a partition: fp32)" : "bf16"))
                         : "fp32")
                << "\n";
    if (aggregator::gemm_bf16_products() && root()) std::cout << "dense self products: bf16 tables\n";
    if (world == 1 && !bf16 && !fp8 && ARCH != gnn_arch::GAT && root())
      std::cout << "relu-masked gradients of 128 columns are gathered " << (aggregator::zs_tables() ? "zero-suppressed (agg_zs = 1)" : "dense (agg_zs = 0)") << "\n";
    if (world == 1 && !bf16 && !fp8 && ARCH != gnn_arch::GAT && root() && aggregator::zs_wide_tables())
      std::cout << "relu-masked gradients of 256 columns are gathered " << (aggregator::zs_tables() ? "zero-suppressed (agg_zs_wide = 1)" : "dense (agg_zs = 0 overrides agg_zs_wide = 1)") << "\n";
    if (bf16 && world > 1 && ARCH == gnn_arch::GAT) {
      std::cerr << "GAIB_AGG_DTYPE=bf16 with GAT runs on one GPU only (GAT gathers fp32 tables; GCN and SAGE take bf16 tables on a partition)\n";
      exit(EXIT_FAILURE);
    }
    if (world > 1 && (subg_size > 0 || inductive)) {
      std::cerr << "subgraph sampling / inductive training run on one GPU only\n";
      exit(EXIT_FAILURE);
    }
  }

  // GAIB_REORDER=cm|bfs|degree (extension; the reference keeps the file's numbering, reader.cpp:414-457): the dataset under the
  // vertex numbering gaib_graph_reorder computes from the graph alone -- Cuthill-McKee / plain breadth-first levels from the
  // highest-degree vertex, or hubs first -- for files whose numbering has no locality.  Everything that is indexed by vertex is
  // permuted with it on the host, once: rows (columns relabelled and sorted again, so that every later step sees an ordinary
  // dataset), features, labels, masks -- inside each interval between the boundaries of the train / val / test ranges, which
  // therefore keep their vertex sets (see below).  Every rank does the same.
  void relabel(const char* how, std::vector<float>& feats, std::vector<label_t>& labels, std::vector<mask_t>& mtrain,
               std::vector<mask_t>& mval, std::vector<mask_t>& mtest) {
    const std::string m(how);
    if (m != "bfs" && m != "degree" && m != "cm") {
      std::cerr << "GAIB_REORDER=" << m << ": cm, bfs or degree\n";
      exit(EXIT_FAILURE);
    }
    const size_t n = graph->size(), ne = graph->sizeEdges();
    gaib_ctx* c = gpu_context::get();
    gaib_graph *g0 = nullptr, *g1 = nullptr;
    GAIB_OR_DIE(gaib_graph_create(c, (int64_t)n, (int64_t)ne, graph->row_start_host_ptr(), 32, graph->edge_dst_host_ptr(), 0, &g0));
    int64_t *d_no = nullptr, *d_on = nullptr;
    GAIB_OR_DIE(gaib_malloc(c, sizeof(int64_t) * n, (void**)&d_no));
    GAIB_OR_DIE(gaib_malloc(c, sizeof(int64_t) * n, (void**)&d_on));
    GAIB_OR_DIE(gaib_graph_reorder(c, g0, m == "cm" ? GAIB_ORDER_CM : (m == "bfs" ? GAIB_ORDER_BFS : GAIB_ORDER_DEGREE), &g1, d_no, d_on));
    std::vector<int64_t> no(n), on(n);
    GAIB_OR_DIE(gaib_memcpy_d2h(c, no.data(), d_no, sizeof(int64_t) * n));
    GAIB_OR_DIE(gaib_memcpy_d2h(c, on.data(), d_on, sizeof(int64_t) * n));
    GAIB_OR_DIE(gaib_free(c, d_no));
    GAIB_OR_DIE(gaib_free(c, d_on));
    GAIB_OR_DIE(gaib_graph_destroy(g0));
    GAIB_OR_DIE(gaib_graph_destroy(g1));
    // The loss layers divide by (end - begin) of the split's RANGE (softmax_loss_layer.cpp:31, quirk Q8), so the ranges
    // must keep their vertex sets: the new order is applied INSIDE each interval between two range boundaries (train / val /
    // test vertices stay where the file put them as a set; a dataset whose three ranges are all [0, n) is relabelled whole)
    {
      std::vector<size_t> cuts = {0, n, train_begin, train_end, val_begin, val_end, test_begin, test_end};
      for (auto& c2 : cuts) c2 = std::min(c2, n);
      std::sort(cuts.begin(), cuts.end());
      cuts.erase(std::unique(cuts.begin(), cuts.end()), cuts.end());
      std::vector<int64_t> on2(n);
      for (size_t s2 = 0; s2 + 1 < cuts.size(); s2++) {
        const size_t a = cuts[s2], b = cuts[s2 + 1];
        for (size_t v = a; v < b; v++) on2[v] = (int64_t)v;
        std::sort(on2.begin() + a, on2.begin() + b, [&](int64_t x, int64_t y) { return no[x] < no[y]; });
      }
      on.swap(on2);
      for (size_t k = 0; k < n; k++) no[on[k]] = (int64_t)k;
    }
    index_t* rp = graph->row_start_host_ptr();
    index_t* ci = graph->edge_dst_host_ptr();
    std::vector<index_t> rp2(n + 1, 0), ci2(ne);
    for (size_t k = 0; k < n; k++) rp2[k + 1] = rp2[k] + (rp[on[k] + 1] - rp[on[k]]);
#pragma omp parallel for schedule(dynamic, 256)
    for (size_t k = 0; k < n; k++) {
      const size_t v = (size_t)on[k];
      index_t* dst = ci2.data() + rp2[k];
      const size_t deg = rp[v + 1] - rp[v];
      for (size_t e = 0; e < deg; e++) dst[e] = (index_t)no[ci[rp[v] + e]];
      std::sort(dst, dst + deg);
    }
    std::copy(rp2.begin(), rp2.end(), rp);
    std::copy(ci2.begin(), ci2.end(), ci);
    auto rows = [&](auto& vec, size_t width) {
      typename std::remove_reference<decltype(vec)>::type out(vec.size());
      for (size_t k = 0; k < n; k++) std::copy(vec.begin() + (size_t)on[k] * width, vec.begin() + ((size_t)on[k] + 1) * width, out.begin() + k * width);
      vec.swap(out);
    };
    rows(feats, (size_t)dim_init);
    rows(labels, label_width);
    rows(mtrain, 1), rows(mval, 1), rows(mtest, 1);
    graph->degree_counting();
    if (root()) std::cout << "GAIB_REORDER=" << m << ": vertices relabelled (" << n << " vertices, " << ne << " edges)\n";
  }

  void load() {
    graph = new Graph(true);
    Reader reader(dataset);
    std::vector<float> feats;
    std::vector<label_t> labels;
    reader.bin_read_graph(graph);
    num_samples = graph->size();
    dim_init = reader.bin_read_features(feats);
    num_cls = reader.bin_read_vlabels(labels, !is_sigmoid);
    label_width = is_sigmoid ? (size_t)num_cls : 1;
    if (ARCH != gnn_arch::SAGE) graph->add_selfloop();  // net.cpp:96
    graph->degree_counting();
    if (root()) std::cout << "num_threads = " << num_threads << ", num_vertices = " << num_samples
              << ", num_edges = " << graph->sizeEdges() << ", num_layers = " << num_layers
              << ", \nnum_epochs = " << num_epochs << ", input_length = " << dim_init
              << ", hidden_length = " << dim_hid << ", num_classes = " << num_cls
              << ", \nfeat_drop = " << feat_drop << ", score_drop = " << score_drop << ", subg_size = " << subg_size
              << ", val_interval = " << val_interval << ", learning_rate = " << lrate << "\n";
    std::vector<mask_t> mtrain(num_samples), mval(num_samples), mtest(num_samples);
    train_count = reader.bin_read_masks("train", num_samples, train_begin, train_end, mtrain.data());
    val_count = reader.bin_read_masks("val", num_samples, val_begin, val_end, mval.data());
    test_count = reader.bin_read_masks("test", num_samples, test_begin, test_end, mtest.data());
    if (dim_init == 0) {
      std::cerr << "dataset has no features (feat_len = 0 in graph.meta.txt)\n";
      exit(1);
    }
    if (const char* ro = getenv("GAIB_REORDER"))
      if (*ro && std::string(ro) != "0") relabel(ro, feats, labels, mtrain, mval, mtest);
    g_train_begin = train_begin, g_train_end = train_end;
    g_val_begin = val_begin, g_val_end = val_end;
    g_test_begin = test_begin, g_test_end = test_end;
    if (world > 1) {
      // this rank's share: rows [lo, hi) of the global CSR, features / labels / masks of the same rows
      part = build_vertex_range_partition(num_samples, graph->row_start_host_ptr(), graph->edge_dst_host_ptr(), rank, world);
      if (ARCH == gnn_arch::GAT)  // the [owned | halo] column space and its transpose (include/gnn/partition.h)
        build_gat_structures(part, graph->row_start_host_ptr(), graph->edge_dst_host_ptr());
      Graph* global = graph;
      graph = make_partitioned_graph(part, comm);
      global->dealloc();
      delete global;
      const size_t lo = (size_t)part.lo, n_own = (size_t)part.n_own();
      feats.erase(feats.begin(), feats.begin() + lo * dim_init);
      feats.resize(n_own * dim_init);
      labels.erase(labels.begin(), labels.begin() + lo * label_width);
      labels.resize(n_own * label_width);
      auto cut = [&](std::vector<mask_t>& m) {
        m.erase(m.begin(), m.begin() + lo);
        m.resize(n_own);
      };
      cut(mtrain), cut(mval), cut(mtest);
      local_range(g_train_begin, g_train_end, train_begin, train_end);
      local_range(g_val_begin, g_val_end, val_begin, val_end);
      local_range(g_test_begin, g_test_end, test_begin, test_end);
      printf("rank %d of %d: rows [%lld, %lld), %zu owned-column + %zu halo-column edges, %lld halo rows in, %zu rows out "
             "per exchange\n", rank, world, (long long)part.lo, (long long)part.hi, part.colidx_own.size(),
             part.colidx_halo.size(), (long long)part.n_halo(), part.send_idx.size());
      fflush(stdout);
      num_samples = (int)n_own;
    }
    // transfer_data_to_device (net.cpp:206-227)
    float_malloc_device64((size_t)num_samples * dim_init, d_features);
    GAIB_OR_DIE(gaib_memcpy_h2d(gpu_context::get(), d_features, feats.data(), sizeof(float) * feats.size()));
    uint8_malloc_device(num_samples * label_width, d_labels);
    copy_uint8_device(num_samples * label_width, labels.data(), d_labels);
    copy_masks_device(num_samples, mtrain.data(), d_masks_train);
    copy_masks_device(num_samples, mval.data(), d_masks_val);
    copy_masks_device(num_samples, mtest.data(), d_masks_test);
    if (world == 1) {
      graph->alloc_on_device();
      graph->copy_to_gpu();
      graph->compute_vertex_data();
    }
    training_graph = graph;
    if (inductive) {
      training_graph = graph->generate_masked_graph(mtrain.data());
      training_graph->copy_to_gpu();
      training_graph->compute_vertex_data();
    }
    if (subg_size > 0) {
      if ((size_t)subg_size > train_count) {
        std::cerr << "subg_size " << subg_size << " exceeds the training set (" << train_count << ")\n";
        exit(1);
      }
      if (val_interval < num_epochs) {
        std::cout << "disabling validation for subgraph sampling on GPU\n";
        val_interval = num_epochs;
      }
      sampler_device = gaib_host::option("sampler_device") != 0;
      if (!sampler_device) {  // (the device path gathers from d_features / d_labels)
        feats_host = feats;
        labels_host = labels;
      }
      masks_train_host = mtrain;
      num_subgraphs = num_threads > 0 ? num_threads : 1;
      sampler = new Sampler(graph, training_graph, masks_train_host.data(), train_count);
      subgs.resize(num_subgraphs);
      for (auto& g : subgs) g = new Graph(true);
      if (!sampler_device) subg_masks.resize((size_t)num_samples * num_subgraphs);
      float_malloc_device64((size_t)subg_size * dim_init, d_feats_subg);
      uint8_malloc_device(subg_size * label_width, d_labels_subg);
      if (sampler_device) {
        subg_sets.resize(num_subgraphs);
        GAIB_OR_DIE(gaib_malloc(gpu_context::get(), sizeof(int64_t) * (size_t)subg_size, (void**)&d_rows_subg));
        std::cout << "subgraphs: built on the device\n";
      }
    }
  }

  // one epoch's subgraph: (re)sample num_subgraphs of them when none is left, then take one
  void subgraph_sampling(int& num_subg_remain) {
    if (num_subg_remain == 0) {
#pragma omp parallel for
      for (int sid = 0; sid < num_subgraphs; sid++) {
        VertexSet set;
        sampler->select_vertices(subg_size, set, (unsigned)omp_get_thread_num());  // seed = thread id, as net.cpp:298
        if (sampler_device) subg_sets[sid].swap(set);  // (induced on the device below, one per epoch)
        else sampler->generateSubgraph(set, &subg_masks[(size_t)sid * num_samples], subgs[sid]);
      }
      num_subg_remain = num_subgraphs;
    }
    const int sg_id = --num_subg_remain;
    Graph* sg = subgs[sg_id];
    if (sampler_device) {
      // one induce call (one 16-byte read-back), the normalisers, two row gathers from the tables already in HBM: no host copy
      // of features, labels or masks; nothing reads a subgraph's max_degree, so degree_counting() is not run
      sampler->generateSubgraphDevice(subg_sets[sg_id], sg, d_rows_subg);
      subg_nv = sg->size();
    } else {
      sg->degree_counting();
      subg_nv = sg->size();
      sg->copy_to_gpu();  // subgraphs of the self-looped full graph already carry their self loops
    }
    sg->compute_vertex_data();
    for (auto& l : layers) {
      l.update_dim_size(subg_nv);
      l.set_graph_ptr(sg);
    }
    if (use_l2norm) l2->update_dim_size(subg_nv);
    if (use_dense) dense->update_dim_size(subg_nv);
    loss->update_dim_size(subg_nv);
    if (sampler_device) {
      gaib_ctx* c = gpu_context::get();
      GAIB_OR_DIE(gaib_gather_rows(c, subg_nv, d_rows_subg, dim_init, d_features, d_feats_subg));
      GAIB_OR_DIE(gaib_gather_rows_u8(c, subg_nv, d_rows_subg, label_width, d_labels, d_labels_subg));
      layers[0].set_feat_in(d_feats_subg);
      loss->set_labels_ptr(d_labels_subg);
      return;
    }
    // features / labels of the kept vertices, in subgraph order
    const mask_t* mk = &subg_masks[(size_t)sg_id * num_samples];
    std::vector<float> f((size_t)subg_nv * dim_init);
    std::vector<label_t> lab((size_t)subg_nv * label_width);
    size_t k = 0;
    for (int v = 0; v < num_samples; v++)
      if (mk[v] == 1) {
        std::copy(&feats_host[(size_t)v * dim_init], &feats_host[(size_t)(v + 1) * dim_init], &f[k * dim_init]);
        std::copy(&labels_host[(size_t)v * label_width], &labels_host[(size_t)(v + 1) * label_width],
                  &lab[k * label_width]);
        k++;
      }
    assert((int)k == subg_nv);
    GAIB_OR_DIE(gaib_memcpy_h2d(gpu_context::get(), d_feats_subg, f.data(), sizeof(float) * f.size()));
    copy_uint8_device(subg_nv * label_width, lab.data(), d_labels_subg);
    layers[0].set_feat_in(d_feats_subg);
    loss->set_labels_ptr(d_labels_subg);
  }

  // evaluation always runs on the full graph (net.cpp:505-540)
  void use_full_graph() {
    for (auto& l : layers) {
      l.update_dim_size(num_samples);
      l.set_graph_ptr(graph);
    }
    if (use_l2norm) l2->update_dim_size(num_samples);
    if (use_dense) dense->update_dim_size(num_samples);
    loss->update_dim_size(num_samples);
    layers[0].set_feat_in(d_features);
    loss->set_labels_ptr(d_labels);
  }

  void construct() {
    if (root()) std::cout << "constructing neural network...\n";
    const int nv = subg_size > 0 ? subg_size : num_samples;  // buffers grow on demand (update_dim_size)
    for (int l = 0; l < num_layers - 1; l++)
      layers.push_back(gconv_t(l, nv, l == 0 ? dim_init : dim_hid, dim_hid, training_graph, true, lrate, feat_drop,
                               score_drop));
    layers.push_back(gconv_t(num_layers - 1, nv, dim_hid, use_dense ? dim_hid : num_cls, training_graph, false, lrate,
                             feat_drop, score_drop));
#if defined(USE_GAT)
    if (const char* hs = getenv("GAIB_GAT_HEADS")) {  // extension: multi-head attention (default 1 = reference)
      for (auto& l : layers) l.get_aggregator().set_num_heads(atoi(hs));
      std::cout << "GAT attention heads: " << atoi(hs) << "\n";
    }
    {
      // option gat_fused_wide (GAIB_GAT_WIDE=1): how the hidden layers' rows of dim_hid columns run -- the one-sweep kernels per
      // column slab where the shape rule gives slabs (whole graphs; under attention dropout only with option gat_fused_drop as
      // well, GAIB_GAT_FUSED_DROP=1: partitions, and dropout without that option, stay staged at these widths), else staged
      const int64_t wide = gaib_host::option("gat_fused_wide"), drop_sweep = gaib_host::option("gat_fused_drop");
      if (wide == 1 && root()) {
        const char* hs = getenv("GAIB_GAT_HEADS");
        int w = 0;
        const int S = gaib_gat_fused_slabs(dim_hid, hs ? atoi(hs) : 1, &w);
        if (S >= 2 && (score_drop == 0.f || drop_sweep == 1) && world == 1) std::cout << "GAT wide rows: one sweep, " << S << " slabs of " << w << "\n";
        else std::cout << "GAT wide rows: staged\n";
      }
    }
#endif
    if (use_l2norm) l2 = new l2norm_layer(nv, dim_hid);
    if (use_dense) dense = new dense_layer(nv, dim_hid, num_cls, lrate);
    layers[0].set_feat_in(d_features);
    // a full-batch run feeds layer 0 the same features over the same graph every epoch: where that layer aggregates
    // first, its aggregated input is computed by the first forward and kept (GAIB_CACHE_INPUT_AGG=0: re-aggregated
    // every epoch, as the reference does).  Not with sampling (the subgraph's features are copied into one buffer).
    const char* ca = getenv("GAIB_CACHE_INPUT_AGG");
    if (subg_size == 0 && feat_drop == 0.f && !(ca && atoi(ca) == 0)) layers[0].set_input_constant(true);
    if (is_sigmoid) loss = new sigmoid_loss_layer(nv, num_cls, d_labels);
    else loss = new softmax_loss_layer(nv, num_cls, d_labels);
  }

  void set_phase(net_phase p) {
    for (auto& l : layers) l.set_netphase(p);
    loss->set_netphase(p);
  }

  void forward_layers() {
    for (int l = 0; l < num_layers - 1; l++) layers[l].forward(layers[l + 1].get_feat_in());
    if (use_dense) {
      layers[num_layers - 1].forward(l2->get_feat_in());
      l2->forward(dense->get_feat_in());
      dense->forward(loss->get_feat_in());
    } else {
      layers[num_layers - 1].forward(loss->get_feat_in());
    }
  }

  // net.cpp:495-500: micro F1 on the sigmoid outputs, or argmax accuracy on the logits
  acc_t accuracy(size_t begin, size_t end, size_t count, mask_t* masks, label_t* labels) {
    if (is_sigmoid) return masked_accuracy_multi(begin, end, count, num_cls, masks, loss->get_feat_out(), labels);
    return masked_accuracy_single(begin, end, count, num_cls, masks, loss->get_feat_in(), labels);
  }

  acc_t forward_prop(acc_t& loss_value) {
    forward_layers();
    if (subg_size > 0) {  // every vertex of the subgraph is a training vertex (net.cpp:478-488)
      loss->forward(0, subg_nv, NULL);
      loss_value = loss->get_prediction_loss(0, subg_nv, subg_nv, NULL);
      return accuracy(0, subg_nv, subg_nv, NULL, d_labels_subg);
    }
    loss->forward(train_begin, train_end, d_masks_train);
    if (world > 1) return reduced_metrics(train_begin, train_end, g_train_end - g_train_begin, d_masks_train, &loss_value);
    loss_value = loss->get_prediction_loss(train_begin, train_end, train_count, d_masks_train);
    return accuracy(train_begin, train_end, train_count, d_masks_train, d_labels);
  }

  // partitioned run: this rank's part [b, e) of a global mask range of `global_len` vertices (masks are the contiguous
  // ranges of graph.meta.txt, Q5, so every vertex of the range counts).  Loss sum and hit / tp-fp-fn counts are summed
  // over the ranks; returns the accuracy (micro F1 for the sigmoid head), *loss_value = mean loss.
  acc_t reduced_metrics(size_t b, size_t e, size_t global_len, mask_t* masks, acc_t* loss_value) {
    gaib_ctx* c = gpu_context::get();
    double v[5] = {0, 0, 0, 0, 0};  // loss sum, hits, tp, fp, fn
    const double n_local = (double)(e - b);
    if (loss_value && e > b) v[0] = (double)loss->get_prediction_loss(b, e, e - b, masks) * n_local;
    if (e > b) {
      if (is_sigmoid) {
        float f1 = 0.f;
        int64_t cnt[3] = {0, 0, 0};
        GAIB_OR_DIE(gaib_masked_f1_micro(c, (int64_t)b, (int64_t)e, num_cls, masks, loss->get_feat_out(), d_labels, &f1, cnt));
        v[2] = (double)cnt[0], v[3] = (double)cnt[1], v[4] = (double)cnt[2];
      } else {
        v[1] = (double)masked_accuracy_single(b, e, e - b, num_cls, masks, loss->get_feat_in(), d_labels) * n_local;
      }
    }
    GAIB_OR_DIE(gaib_allreduce_host_f64(comm, v, 5));
    if (loss_value) *loss_value = (acc_t)(v[0] / (double)global_len);
    if (is_sigmoid) {  // f1_micro of the summed counts (math_functions.cpp:580-621)
      const double prec = v[2] + v[3] > 0 ? v[2] / (v[2] + v[3]) : 0., rec = v[2] + v[4] > 0 ? v[2] / (v[2] + v[4]) : 0.;
      return (acc_t)(prec + rec > 0 ? 2. * prec * rec / (prec + rec) : 0.);
    }
    return (acc_t)(v[1] / (double)global_len);
  }

  void backward_prop() {
    const size_t tb = subg_size > 0 ? 0 : train_begin, te = subg_size > 0 ? (size_t)subg_nv : train_end;
    mask_t* tm = subg_size > 0 ? NULL : d_masks_train;
    if (use_dense) {
      loss->backward(tb, te, tm, dense->get_grad_in());
      rescale_loss_grad(dense->get_grad_in(), tb, te);
      dense->backward(l2->get_grad_in());
      l2->backward(layers[num_layers - 1].get_grad_in());
      layers[num_layers - 1].backward(l2->get_feat_in(), layers[num_layers - 2].get_grad_in());
    } else {
      loss->backward(tb, te, tm, layers[num_layers - 1].get_grad_in());
      rescale_loss_grad(layers[num_layers - 1].get_grad_in(), tb, te);
      layers[num_layers - 1].backward(loss->get_feat_in(), layers[num_layers - 2].get_grad_in());
    }
    for (int l = num_layers - 2; l > 0; l--) layers[l].backward(layers[l + 1].get_feat_in(), layers[l - 1].get_grad_in());
    layers[0].backward(layers[1].get_feat_in(), NULL);
  }

  // the loss gradient is divided by (end - begin) of the range it was called on (softmax_loss_layer.cpp:31, Q8): a
  // rank's local share of the range -> the global range
  void rescale_loss_grad(float* grad, size_t b, size_t e) {
    if (world == 1 || e <= b) return;
    const float a = (float)((double)(e - b) / (double)(g_train_end - g_train_begin));
    GAIB_OR_DIE(gaib_scale_f32(gpu_context::get(), (int64_t)num_samples * num_cls, a, grad));
  }

  acc_t evaluate(const std::string& type) {
    set_phase(net_phase::TEST);
    if (subg_size > 0 || inductive) use_full_graph();
    forward_layers();
    const bool test = type == "test";
    const size_t b = test ? test_begin : val_begin, e = test ? test_end : val_end, c = test ? test_count : val_count;
    mask_t* m = test ? d_masks_test : d_masks_val;
    if (is_sigmoid) loss->forward(b, e, m);  // the F1 reads the sigmoid outputs (net.cpp:569-572)
    if (world > 1) return reduced_metrics(b, e, test ? g_test_end - g_test_begin : g_val_end - g_val_begin, m, NULL);
    return accuracy(b, e, c, m, d_labels);
  }

  // GAIB_EPOCH_GRAPH = 1: record the epoch wherever the run allows it; 0: never; unset: when it allows it AND the graph
  // is small enough to be launch bound (<= 4 M edges).  Not recorded: partitioned runs (the exchange waits on peers),
  // sampling / inductive runs (the graph changes per epoch), per-op synchronising timers and the side-stream option.
  // Dropout: a mask seed passed by value would be frozen in the recording, so a run with feat_drop > 0 or score_drop > 0 is
  // recorded only with option drop_seed_dev (GAIB_DROP_SEED_DEV=1), under which the layers keep their seeds in device memory
  // (gaib_dropout_dev: epoch 0 makes the slots call by call, the recording advances none, every replay draws the next) --
  // except GAT attention dropout kept in the one sweep (gat_fused_drop = 1), whose kernels take their seed by value.
  bool decide_graph_mode() const {
    const char* e = getenv("GAIB_EPOCH_GRAPH");
    if (e && atoi(e) == 0) return false;
    const char* st = getenv("GAIB_SYNC_TIMERS");
    const char* ov = getenv("GAIB_OVERLAP");
    const bool dropout = feat_drop != 0.f || score_drop != 0.f;
    const int64_t seeds_dev = dropout ? gaib_host::option("drop_seed_dev") : 0, drop_sweep = dropout ? gaib_host::option("gat_fused_drop") : 0;
    const bool sweep_by_value = ARCH == gnn_arch::GAT && score_drop != 0.f && drop_sweep == 1;
    const bool other = world == 1 && subg_size == 0 && !inductive && !(st && atoi(st)) && !(ov && atoi(ov)) && num_epochs > 1;
    const bool allowed = other && (!dropout || (seeds_dev == 1 && !sweep_by_value));
    if (e && atoi(e) != 0 && !allowed && root()) {
      if (other && seeds_dev == 1)
        std::cerr << "[gaib] GAIB_EPOCH_GRAPH=1 ignored: attention dropout in the one sweep (gat_fused_drop = 1) takes its mask "
                     "seed by value and is not recorded\n";
      else
        std::cerr << "[gaib] GAIB_EPOCH_GRAPH=1 ignored: partitioned, sampling, inductive, dropout or timer runs are not recorded\n";
    }
    if (!allowed) return false;
    return e ? true : graph->sizeEdges() <= ((size_t)1 << 22);
  }

  // the recorded forward: layers, loss, loss mean and accuracy (or F1 counts) left on the device, read-back to pinned memory
  void record_epoch(optimizer* opt) {
    gaib_ctx* c = gpu_context::get();
    GAIB_OR_DIE(gaib_malloc(c, METRICS_BYTES, (void**)&d_metrics));
    GAIB_OR_DIE(gaib_host_alloc(c, METRICS_BYTES, (void**)&h_metrics));
    GAIB_OR_DIE(gaib_capture_begin(c));
    forward_layers();
    loss->forward(train_begin, train_end, d_masks_train);
    GAIB_OR_DIE(gaib_masked_avg_loss_dev(c, (int64_t)train_begin, (int64_t)train_end, d_masks_train, loss->loss_buffer(),
                                         (float*)d_metrics));
    if (is_sigmoid)
      GAIB_OR_DIE(gaib_masked_f1_counts_dev(c, (int64_t)train_begin, (int64_t)train_end, num_cls, d_masks_train,
                                            loss->get_feat_out(), d_labels, (uint64_t*)(d_metrics + 16)));
    else
      GAIB_OR_DIE(gaib_masked_accuracy_single_dev(c, (int64_t)train_begin, (int64_t)train_end, num_cls, d_masks_train,
                                                  loss->get_feat_in(), d_labels, (float*)d_metrics + 1));
    GAIB_OR_DIE(gaib_memcpy_d2h_async(c, h_metrics, d_metrics, METRICS_BYTES));
    GAIB_OR_DIE(gaib_capture_end(c, &fw_exec));
    GAIB_OR_DIE(gaib_capture_begin(c));
    backward_prop();
    for (auto& l : layers) l.update_weight(opt);
    GAIB_OR_DIE(gaib_capture_end(c, &bw_exec));
    if (root())
      std::cerr << "[gaib] epochs recorded as HIP graphs: forward " << gaib_exec_nodes(fw_exec) << " nodes, backward + update "
                << gaib_exec_nodes(bw_exec) << " nodes\n";
  }

  acc_t recorded_metrics(acc_t& loss_value) const {
    loss_value = ((const float*)h_metrics)[0];
    if (!is_sigmoid) return ((const float*)h_metrics)[1];
    const uint64_t* cnt = (const uint64_t*)(h_metrics + 16);  // f1_micro of the counts (math_functions.cpp:580-621)
    const double tp = (double)cnt[0], fp = (double)cnt[1], fn = (double)cnt[2];
    const double prec = tp + fp > 0 ? tp / (tp + fp) : 0., rec = tp + fn > 0 ? tp / (tp + fn) : 0.;
    return (acc_t)(rec + prec > 0. ? 2. * (rec * prec) / (rec + prec) : 0.);
  }

  void train() {
    optimizer* opt = new adam(lrate);  // one instance for every layer's update_weight call (Q6)
    graph_mode = decide_graph_mode();
    if (gaib_host::option("drop_seed_dev") == 1 && root()) std::cerr << "[gaib] dropout mask seeds: device\n";
    if (graph_mode) {
      // the null stream cannot be recorded, and the beta powers of every Adam instance have to live on the device
      GAIB_OR_DIE(gaib_ctx_own_stream(gpu_context::get()));
      adam::keep_powers_on_device(true);
    }
    std::cout << "Start training...\n";
    double total = 0.0;
    int num_subg_remain = 0;
    unsigned long long edges_epoch = 0;  // edges aggregated by a steady-state epoch (the aggregators count per call)
    // GAIB_PROF_TABLE=k: in-stream timing of every library launch from epoch k on (default 1: epoch 0 allocates and builds
    // the graph's lazily made tables), printed after the run as "[gaib prof] key count total_ms alg_bytes flops roof_ms" --
    // what bench.py's epoch workloads build their roofline record from.  Not with recorded epochs (nothing is launched call by call).
    const char* pt = getenv("GAIB_PROF_TABLE");
    const int prof_from = (pt && *pt && !graph_mode) ? std::max(0, atoi(pt)) : -1;
    // GAIB_EPOCH_TIMES=k: only the epochs' train_time at full precision from epoch k on ("[gaib prof] epoch_seconds ..."), no
    // launch timing -- also for recorded epochs (a cora epoch is 0.2 ms: "0.000 s" in the reference's three decimals)
    const char* et = getenv("GAIB_EPOCH_TIMES");
    const int times_from = prof_from >= 0 ? prof_from : ((et && *et) ? std::max(0, atoi(et)) : -1);
    int prof_epochs = 0;
    std::vector<double> prof_epoch_s;  // the profiled epochs' train_time at full precision (the log line keeps the reference's 3 decimals)
    // GAIB_EPOCH_LOSSES=1: every epoch's train_loss / train_acc once more after the run with 9 significant digits
    // ("[gaib prof] epoch_losses ..." / "epoch_accs ..."): the log line keeps the reference's three decimals, which is all a
    // comparison of loss curves would otherwise see (bench.py's epoch parity holds the curve to 1e-4 relative)
    const bool exact_losses = getenv("GAIB_EPOCH_LOSSES") && atoi(getenv("GAIB_EPOCH_LOSSES")) != 0;
    std::vector<double> all_loss, all_acc;
    std::vector<double> subgraph_s;  // (GAIB_EPOCH_TIMES with sampling) seconds per epoch in subgraph_sampling
    // score_drop > 0 on GAT: which path the layers' training forwards of epoch 0 TOOK (asked of the aggregators, not predicted:
    // GAIB_GAT_FUSED_DROP=1 keeps a layer in the one-sweep kernels only where they cover its shape and graph), printed once
    bool drop_path_said = !(ARCH == gnn_arch::GAT && score_drop > 0.f && root());
    auto say_drop_path = [&]() {
      if (drop_path_said) return;
      drop_path_said = true;
#if defined(USE_GAT)
      size_t swept = 0;
      for (auto& l : layers) swept += l.get_aggregator().dropped_in_sweep() ? 1 : 0;
      std::cout << "GAT attention dropout: ";
      if (swept == layers.size()) std::cout << "one sweep\n";
      else if (swept == 0) std::cout << "staged\n";
      else std::cout << "one sweep in " << swept << " of " << layers.size() << " layers, staged in the others\n";
#endif
    };
    for (int itr = 0; itr < num_epochs; itr++) {
      if (itr == 1) say_drop_path();
      if (itr == prof_from) {
        GAIB_OR_DIE(gaib_prof_reset(gpu_context::get()));
        GAIB_OR_DIE(gaib_prof_enable(gpu_context::get(), 1));
      }
      if (prof_from >= 0 && itr >= prof_from) prof_epochs++;
      const unsigned long long edges_before = gpu_context::aggregated_edges();
      if (subg_size > 0) {
        // GAIB_EPOCH_TIMES: one wall time per epoch around the subgraph's construction, its device work waited for inside
        // the span ("[gaib prof] subgraph_seconds ...": the in-trainer measurement of option sampler_device, both settings)
        const bool timed = et && *et && itr >= times_from;
        const double ts = timed ? omp_get_wtime() : 0.0;
        subgraph_sampling(num_subg_remain);
        if (timed) {
          gpu_context::sync();
          subgraph_s.push_back(omp_get_wtime() - ts);
        }
      }
      std::cout << "Epoch " << std::setw(3) << itr << " ";
      set_phase(net_phase::TRAIN);
      acc_t train_loss = 0.0;
      acc_t train_acc = 0.0;
      double t0, t1, t2;
      if (graph_mode && itr >= 1) {
        // epoch 0 ran call by call (it allocates optimizer state and builds the graph's lazily made tables) and was
        // followed by the recording; from epoch 1 on an epoch is two graph launches
        gaib_ctx* c = gpu_context::get();
        // one host wait per epoch; the forward / backward split of the log line comes from events around the launches
        t0 = omp_get_wtime();
        GAIB_OR_DIE(gaib_exec_launch(c, fw_exec));
        GAIB_OR_DIE(gaib_exec_launch(c, bw_exec));
        gpu_context::sync();
        t2 = omp_get_wtime();
        train_acc = recorded_metrics(train_loss);  // copied to pinned memory at the end of the forward recording
        float fw_ms = 0.f, bw_ms = 0.f;
        GAIB_OR_DIE(gaib_exec_elapsed_ms(fw_exec, &fw_ms));
        GAIB_OR_DIE(gaib_exec_elapsed_ms(bw_exec, &bw_ms));
        t1 = t0 + (t2 - t0) * (fw_ms + bw_ms > 0.f ? fw_ms / (fw_ms + bw_ms) : 0.5);
      } else {
        t0 = omp_get_wtime();
        train_acc = forward_prop(train_loss);  // the loss read-back synchronises the stream
        t1 = omp_get_wtime();
        backward_prop();
        for (auto& l : layers) l.update_weight(opt);
        gpu_context::sync();
        t2 = omp_get_wtime();
      }
      // a replayed epoch runs no host code: what it aggregates is what its recording counted; call by call the last
      // epoch counts (epoch 0 also aggregates what layer 0 keeps afterwards)
      if (!(graph_mode && itr >= 1)) edges_epoch = gpu_context::aggregated_edges() - edges_before;
      if (graph_mode && itr == 0) {
        const unsigned long long b = gpu_context::aggregated_edges();
        record_epoch(opt);  // (outside the timed part of the epoch, before its log line ends)
        edges_epoch = gpu_context::aggregated_edges() - b;
      }
      const double fw = t1 - t0, bw = t2 - t1, epoch_time = fw + bw;
      total += epoch_time;
      if (times_from >= 0 && itr >= times_from) prof_epoch_s.push_back(epoch_time);
      if (exact_losses) {
        all_loss.push_back((double)train_loss);
        all_acc.push_back((double)train_acc);
      }
      std::cout << "train_loss " << std::setprecision(3) << std::fixed << train_loss << " train_acc " << train_acc << " ";
      if (itr % val_interval == 0 && itr != 0) {
        double tv0 = omp_get_wtime();
        acc_t val_acc = evaluate("val");
        double tv = omp_get_wtime() - tv0;
        std::cout << "val_acc " << std::setprecision(3) << std::fixed << val_acc << " ";
        std::cout << "time " << std::setprecision(3) << std::fixed << epoch_time + tv << " s (train_time " << epoch_time
                  << " val_time " << tv << ")\n";
        if (inductive && subg_size == 0)  // back to the training graph
          for (auto& l : layers) l.set_graph_ptr(training_graph);
      } else {
        std::cout << "train_time " << std::fixed << epoch_time << " s (fw " << fw << ", bw " << bw << ")\n";
      }
    }
    if (exact_losses && root()) {
      std::cout << "[gaib prof] epoch_losses" << std::scientific << std::setprecision(8);
      for (double v : all_loss) std::cout << " " << v;
      std::cout << "\n[gaib prof] epoch_accs";
      for (double v : all_acc) std::cout << " " << v;
      std::cout << std::fixed << std::setprecision(3) << "\n";
    }
    if (prof_from < 0 && !prof_epoch_s.empty() && root()) {
      std::cout << "[gaib prof] epoch_seconds";
      for (double t : prof_epoch_s) std::cout << " " << std::setprecision(7) << std::fixed << t;
      std::cout << std::setprecision(3) << "\n";
    }
    if (!subgraph_s.empty() && root()) {
      std::cout << "[gaib prof] subgraph_seconds";
      for (double t : subgraph_s) std::cout << " " << std::setprecision(7) << std::fixed << t;
      std::cout << std::setprecision(3) << "\n";
    }
    if (prof_from >= 0 && prof_epochs > 0) {
      gaib_ctx* c = gpu_context::get();
      GAIB_OR_DIE(gaib_prof_enable(c, 0));
      size_t need = 0;
      GAIB_OR_DIE(gaib_prof_table(c, NULL, 0, &need));
      std::string tab(need + 1, '\0');
      GAIB_OR_DIE(gaib_prof_table(c, &tab[0], tab.size(), &need));
      if (root()) {
        std::cout << "[gaib prof] epochs " << prof_epochs << "\n[gaib prof] epoch_seconds";
        for (double t : prof_epoch_s) std::cout << " " << std::setprecision(7) << std::fixed << t;
        std::cout << std::setprecision(3) << "\n";
        size_t a = 0;
        const std::string text(tab.c_str());
        while (a < text.size()) {
          size_t b = text.find('\n', a);
          if (b == std::string::npos) b = text.size();
          if (b > a) std::cout << "[gaib prof] " << text.substr(a, b - a) << "\n";
          a = b + 1;
        }
      }
      GAIB_OR_DIE(gaib_prof_reset(c));
    }
    say_drop_path();  // (a run of one epoch)
    std::cout << "Average training time per epoch: " << total / (double)num_epochs << " seconds. Throughput "
              << (double)num_epochs / total << " epoch/s\n";
    // added by this backend: the hot path's own metric (edges of the graph x aggregation calls of a steady-state
    // epoch, this rank's share; validation passes not counted)
    if (total > 0.0)
      std::cout << "Aggregated edges per epoch: " << edges_epoch << " (" << std::setprecision(2) << std::fixed
                << (double)edges_epoch * (double)num_epochs / total / 1e9 << " G aggregated edges/s)\n"
                << std::setprecision(3);  // (the lines that follow keep the reference's three decimals)
  }
};

void print_timers() {
  static const std::pair<char, const char*> names[] = {
      {OP_SPARSEMM, "AGGR"},   {OP_DENSEMM, "LINEAR"}, {OP_RELU, "RELU"},   {OP_DROPOUT, "DROPOUT"},
      {OP_LOSS, "LOSS"},       {OP_NORM, "NORM"},      {OP_SCORE, "SCORE"}, {OP_ATTN, "ATTN"},
      {OP_TRANSPOSE, "TRANSP"}};
  std::cout << "--------------------\n";
  for (auto& n : names) std::cout << n.second << " time: " << time_ops[n.first] << "\n";
  std::cout << "--------------------\n";
}

// GAIB_RANKS=N: this process only starts and supervises the ranks.  Nothing here may touch the GPU (a process that
// has initialised it must not fork ranks): plain fork + exec of this very binary, before any gaib_* call.
static pid_t g_rank_pids[64];
static int g_rank_n = 0;
extern "C" void launcher_on_signal(int sig) {  // the launcher is asked to stop: so are the ranks it started (and only those)
  for (int r = 0; r < g_rank_n; r++)
    if (g_rank_pids[r] > 0) kill(g_rank_pids[r], SIGTERM);
  _exit(128 + sig);
}

int launch_ranks(int n, char** argv) {
  if (n > 64) {
    fprintf(stderr, "GAIB_RANKS: at most 64 ranks\n");
    return 1;
  }
  // under a profiler the tool's preloaded library has initialised the GPU in THIS process before main: forking and
  // exec'ing ranks from it is the exec this pool forbids.  Refuse, and say what works.
  {
    const char* tool = getenv("ROCP_TOOL_LIBRARIES");
    const char* pre = getenv("LD_PRELOAD");
    const char* hsa = getenv("HSA_TOOLS_LIB");
    auto names_profiler = [](const char* v) { return v && (strstr(v, "rocprof") || strstr(v, "roctracer")); };
    if ((tool && *tool) || names_profiler(pre) || names_profiler(hsa)) {
      fprintf(stderr, "[launcher] GAIB_RANKS under a profiler (ROCP_TOOL_LIBRARIES / LD_PRELOAD / HSA_TOOLS_LIB name one): its "
                      "library touches the GPU before main, and such a process must not start rank programs.  Profile ONE "
                      "rank directly: RANK=r WORLD_SIZE=N LOCAL_RANK=r GAIB_COMM_ID_FILE=<shared path> rocprofv3 ... -- %s ...\n",
              argv[0]);
      return 2;
    }
  }
  // several ranks per device (more ranks than GPUs: tests, one-GPU boxes) move the rows over hipIpc handles, and the host
  // driver of this pool only supports the dmabuf kind
  setenv("HSA_ENABLE_IPC_MODE_LEGACY", "0", 0);
  const char* dl = getenv("GAIB_RANKS_DEADLINE_S");
  const double deadline_s = dl ? atof(dl) : 0.0;  // 0: none (training runs have no natural bound); a dead rank still ends the job
  char idfile[96], nbuf[16];
  snprintf(idfile, sizeof(idfile), "/dev/shm/gaib_id_%d_%ld", (int)getpid(), (long)time(nullptr));
  snprintf(nbuf, sizeof(nbuf), "%d", n);
  std::vector<pid_t> pids(n, -1);
  for (int r = 0; r < n; r++) {
    pid_t p = fork();
    if (p < 0) {
      perror("fork");
      for (int q = 0; q < r; q++) kill(pids[q], SIGKILL);
      return 1;
    }
    if (p == 0) {
      char rbuf[16];
      snprintf(rbuf, sizeof(rbuf), "%d", r);
      setenv("RANK", rbuf, 1);
      setenv("LOCAL_RANK", rbuf, 1);
      setenv("WORLD_SIZE", nbuf, 1);
      if (!getenv("GAIB_COMM_ID_FILE")) setenv("GAIB_COMM_ID_FILE", idfile, 1);
      unsetenv("GAIB_RANKS");
      execv("/proc/self/exe", argv);
      perror("execv");
      _exit(127);
    }
    pids[r] = p;
    g_rank_pids[r] = p;
    g_rank_n = r + 1;
  }
  signal(SIGTERM, launcher_on_signal);
  signal(SIGINT, launcher_on_signal);
  struct timespec t0;
  clock_gettime(CLOCK_MONOTONIC, &t0);
  int alive = n, rc = 0;
  while (alive > 0 && rc == 0) {
    int st = 0;
    pid_t p = waitpid(-1, &st, WNOHANG);
    if (p > 0) {
      for (int r = 0; r < n; r++)
        if (pids[r] == p) {
          pids[r] = -1;
          alive--;
          const int code = WIFEXITED(st) ? WEXITSTATUS(st) : 128 + WTERMSIG(st);
          if (code != 0) {
            fprintf(stderr, "[launcher] rank %d exited with %d: stopping the other ranks\n", r, code);
            rc = code;
          }
        }
      continue;
    }
    struct timespec t1;
    clock_gettime(CLOCK_MONOTONIC, &t1);
    if (deadline_s > 0 && (t1.tv_sec - t0.tv_sec) > deadline_s) {
      fprintf(stderr, "[launcher] GAIB_RANKS_DEADLINE_S = %.0f s passed: stopping the ranks\n", deadline_s);
      rc = 124;
    }
    usleep(20000);
  }
  if (rc) {  // exactly the children started above
    for (int r = 0; r < n; r++)
      if (pids[r] > 0) kill(pids[r], SIGTERM);
    for (int i = 0; i < 250 && alive > 0; i++) {
      int st;
      pid_t p = waitpid(-1, &st, WNOHANG);
      if (p > 0) {
        for (int r = 0; r < n; r++)
          if (pids[r] == p) pids[r] = -1, alive--;
      } else
        usleep(20000);
    }
    for (int r = 0; r < n; r++)
      if (pids[r] > 0) {
        kill(pids[r], SIGKILL);
        waitpid(pids[r], nullptr, 0);
      }
  }
  unlink(idfile);
  return rc;
}

}  // namespace

int main(int argc, char* argv[]) {
  if (const char* nr = getenv("GAIB_RANKS")) {
    if (atoi(nr) > 1 && !getenv("RANK") && !getenv("GAIB_RANK")) {
      // (what every rank would say in parse(), said once and before any rank is started)
      if (const char* dt = getenv("GAIB_AGG_DTYPE"))
        if (std::string(dt) == "fp8") {
          std::cerr << "GAIB_AGG_DTYPE=fp8 (agg_fp8) runs on one GPU only: fp8 feature tables have no halo exchange and no row-class kernels\n";
          return EXIT_FAILURE;
        }
      return launch_ranks(atoi(nr), argv);
    }
  }
  if (argc <= 4 || (argc > 9 && argc != 13)) {
    std::cout << "Usage: ./train data num_epochs num_threads type_loss "
              << "hidden(16) score_drop_rate(0.) feat_drop_rate(0.) "
              << "learnng_rate(0.01) num_layers(2) subg_size(0) val_interval(50) inductive(0)\n"
              << "Example: ./bin/gpu_train_gcn cora 10 2 softmax\n";
    exit(1);
  }
  std::cout << "Using " << ARCH_NAME << "\n";
  Trainer t;
  t.parse(argc, argv);
  if (!t.root()) std::cout.setstate(std::ios_base::failbit);  // rank 0 prints the log lines
  t.load();
  t.construct();
  double t1 = omp_get_wtime();
  t.train();
  double t2 = omp_get_wtime();
  std::cout << "Total training time (validation time included): " << t2 - t1 << " seconds\n";
  double tt1 = omp_get_wtime();
  acc_t test_acc = t.evaluate("test");
  double tt2 = omp_get_wtime();
  std::cout << "Test accuracy: " << test_acc << "  test time: " << tt2 - tt1 << " seconds\n";
  if (getenv("GAIB_SYNC_TIMERS") && atoi(getenv("GAIB_SYNC_TIMERS"))) print_timers();
  if (t.comm) {
    GAIB_OR_DIE(gaib_comm_barrier(t.comm));
    if (t.graph->halo_plan()) gaib_halo_destroy(t.graph->halo_plan());
    gaib_comm_destroy(t.comm);
  }
  return 0;
}
