// env.hh -- run configuration, output directory and param.txt, for the flags
// the link-sampling path reads.  Mirrors the reference's Env (src/env.hh):
// same defaults (ctor init list :305-483), same output-directory naming
// (:503-568), same param.txt keys (:577-619) and the network.dat symlink.
#pragma once
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace svinet {

class Env {
 public:
  struct Args {
    uint32_t n = 0, k = 0;
    std::string datfname = "network.dat";
    std::string label = "mmsb";
    bool batch = false, link_sampling = false;
    bool batch_gpu = false;             // -batch-gpu: -batch with its sweeps and pair likelihoods on the device (svils_batch_*)
    // -rnode / -rpair / -rpair -stratified: sampled-pair SVI of the exact model (MMSBInfer::infer, src/mmsbinfer.cc:459-740);
    // -nodelay: lambda learns from the first iteration (src/env.hh:487-490); -host-loops: the plain C++ loops instead of the device
    bool rnode = false, rpair = false, stratified = false, nodelay = false, host_loops = false;
    double scale = 1;                   // -scale (src/env.hh:357): only 1 is implemented
    // -infset: informative-set SVI (FastAMM::infer, src/fastamm.cc:549-672); -preprocess: its pass over the graph that writes
    // neighbors.bin (Network::set_neighborhood_sets, src/network.cc:558-686).  Both name the directory -infset (src/env.hh:523)
    bool infset = false, preprocess = false;
    double inf_epsilon = 0.0001;        // _inf_epsilon (src/fastamm.cc:18): library callers only
    // -snode: stratified random node SVI (FastAMM2::infer, src/fastamm2.cc:535-702; the reference starts it with
    // -stratified -rnode).  The constructor is -infset's; the chance of a non-link step is inf_epsilon, 0.5 there (:15)
    bool snode = false;
    // -sparse-graph (with -rnode / -rpair / -infset / -snode on the device): the handle keeps the graph as sorted adjacency
    // rows (svils_batch_create_sparse) and -n has no cap
    bool sparse_graph = false;
    // -orig: the full K x K blockmodel (MMSBInferOrig::batch_infer, src/mmsbinferorig.cc:212-294); -itype: its beta start
    // (0: init_beta1, > 0: init_beta2).  On the device unless -host-loops is given
    bool orig = false;
    // -clean-holdout (with -orig): both orientations of every held-out and validation pair are left out of training
    bool clean_holdout = false;
    int itype = 0;
    // -single: the single-membership stochastic blockmodel (SBM::batch_infer, src/sbm.cc:457-543).  On the device unless
    // -host-loops is given
    bool single = false;
    // -single-logl: -single with the lower bound after every iteration (logl.txt) and its two stop rules (sbm.hh)
    bool single_logl = false;
    bool findk = false;               // -findk: estimate the number of communities (FastInit, src/main.cc:321-327)
    bool gml = false, lcstats = false;  // -gml / -lcstats: link communities of a fitted model (MMSBGen, src/main.cc:307-318)
    bool ppc = false, gen = false;      // -ppc / -gen: posterior predictive checks, a network from the prior (MMSBGen, src/main.cc:268-303)
    int ppc_draws = 100;                // -ppc-draws (ppc_ndraws, src/env.hh:452)
    int ppc_save = 0;                   // -ppc-save <m>: the networks of the first m replicates
    bool ppc_mean = false;              // -ppc-mean: no parameter draws
    bool ppc_hops = false;              // -ppc-hops: the hop plot and the components of every list (svils_ppc_hops)
    bool ppc_orig = false;              // -ppc-orig: the -ppc mode for the K x K blockmodel of an -orig fit (gamma.txt, beta.txt)
    bool load = false;
    std::string location;
    bool val_load = false;
    std::string val_file_location;
    bool test_load = false;
    std::string test_file_location;
    bool init_comm = false;             // -init-communities <file>
    std::string init_comm_fname;
    double hol_ratio = 0.01;
    std::string eta_type = "uniform";
    uint32_t rfreq = 1;
    bool accuracy = false;
    bool logl = false;               // -logl: MMSBBatch writes the variational lower bound at every report (src/env.hh: logl)
    bool defer_init_gamma = false;  // library callers (host_api.Setup(host_gamma=False)): init_gamma2 is left to svils_init_gamma
    uint32_t max_iterations = 0;
    bool use_validation_stop = true;
    double rand_seed = 0;
    double link_thresh = 0.5;
    uint32_t lt_min_deg = 0;
    bool nmi = false;
    std::string ground_truth_fname;
    uint32_t nthreads = 0;
    bool strid = false;
    // extensions of this build (not in the reference)
    int device = 0;
    uint32_t sweep_batch = 0;   // sweeps enqueued per report chunk / between host polls; 0 = automatic (1, 2, 4, 8, then 16)
    std::string outdir_root;    // directory in which the output dir is created ("" = cwd)
    bool write_files = true;    // false: library use (bench / tests), nothing touches the disk
    // mini-batch mode of -link-sampling (include/svils.h, svils_step): 0 = full sweeps (the reference's loop)
    uint32_t minibatch = 0;     // nodes per mini-batch
    double tau0 = 1024, kappa = 0.9, nodetau0 = 1024, nodekappa = 0.5;   // src/env.hh:405-408
    int32_t sparse_after = 1000;   // the active-set branch needs _iter > this (src/linksampling.cc:634)
    // -gpus N: one process per GPU (forked by main), node-block sharding with RCCL exchanges inside
    // the device library (svils_sweep_sharded); rank 0 writes the files
    int gpus = 1, rank = 0;
    bool sharded = false;       // node-block sharding: set by -gpus N > 1, or by -sharded with one GPU (a communicator of one rank: the same code path)
    bool kshard = false;        // -kshard: shard the K columns over the ranks instead of the nodes
    // the ncclUniqueId travels from rank 0 to the others through pipes made before the fork: rank 0 holds the write
    // ends, rank r > 0 the read end of its own
    int comm_rfd = -1;
    std::vector<int> comm_wfds;
    std::vector<int> device_list;   // -device-list d0,d1,..: the HIP ordinal of every rank (default: device, device+1, ..)
    // link prediction from the final state (svils_link_prob / svils_predict_links): -predict-pairs <file>, -recommend <k>
    std::string predict_pairs_fname;
    int recommend = 0;              // top-k links per node written to recommendations.txt; 0 = none
    // where given links stand among their nodes' candidates (svils_rank_links): -rank-pairs <file>, -rank-heldout
    std::string rank_pairs_fname;
    bool rank_heldout = false;
    // -adamic-adar: the same pair lists scored and ranked by common neighbours, Adamic-Adar and resource allocation
    // (svils_nbr_score / svils_nbr_rank), the baselines beside the model's ranks
    bool adamic_adar = false;
  };

  explicit Env(const Args &a);
  ~Env();

  uint32_t n, k, t;
  double alpha;
  double heldout_ratio;
  double eta0, eta1;
  const double eta0_dense, eta1_dense, eta0_sparse, eta1_sparse;
  uint32_t reportfreq;
  double epsilon;
  uint32_t max_iterations;
  double seed;
  std::string eta_type;
  bool use_validation_stop;
  bool accuracy;
  bool logl;                         // -logl: read by MMSBBatch alone (approx_log_likelihood)
  bool defer_init_gamma;
  double link_thresh;
  uint32_t lt_min_deg;
  bool model_load;
  std::string gamma_location;
  bool load_heldout;
  std::string load_heldout_fname;
  bool load_test;
  std::string load_test_fname;
  bool use_init_communities;
  std::string init_communities_fname;
  bool nmi;
  std::string ground_truth_fname;
  std::string datfname, label;
  int gpus, rank;
  bool kshard, sharded;
  int comm_rfd;
  std::vector<int> comm_wfds;
  bool batch_mode, link_sampling, findk;
  bool batch_device;                 // -batch-gpu, and -rnode / -rpair / -infset / -snode without -host-loops: MMSBBatch drives a svils_batch handle
  bool randomnode, randompair, stratified, delaylearn;   // the sampled-pair engines (src/env.hh:485-501)
  bool sampled() const { return randomnode || randompair; }
  bool infset, preprocess;           // -infset / -preprocess (src/env.hh:325, :436)
  double inf_epsilon;                // the chance of a non-informative step (-snode: of a non-link step)
  bool snode;                        // -snode (FastAMM2)
  bool sparse_graph;                 // -sparse-graph: the device handle in sparse form; the number of pairs counted in 64 bits
  bool fastamm() const { return infset || snode; }   // the constructor both engines share (src/fastamm.cc:64-97)
  bool orig, orig_device;            // -orig; without -host-loops MMSBInferOrig drives a svils_orig handle
  int itype;                         // -itype (src/main.cc:193-194), read by -orig alone
  bool clean_holdout;                // -clean-holdout: -orig trains on no orientation of a held-out or validation pair
  bool single, single_device;        // -single; without -host-loops SBM drives a svils_sbm handle
  bool single_logl;                  // -single-logl: SBM writes the lower bound after every iteration and heeds its stop rules
  double sbm_alpha;                  // the Dirichlet prior of -single (src/env.hh:345)
  uint32_t s;                        // their mini-batch size n / 2 (src/env.hh:321; -rpair only)
  bool gml, lcstats;
  bool strid;
  volatile int terminate;
  // set by Network::set_env_variables
  uint64_t total_pairs;
  double ones_prob, zeros_prob;
  // extensions
  int device;
  uint32_t sweep_batch;
  bool write_files;
  uint32_t minibatch;
  double tau0, kappa, nodetau0, nodekappa;
  int32_t sparse_after;
  std::string predict_pairs_fname;   // -predict-pairs: pairs scored into link-prob.txt ("" = none)
  uint32_t recommend;                // -recommend: top-k links per node into recommendations.txt (0 = none)
  std::string rank_pairs_fname;      // -rank-pairs: pairs ranked into link-ranks.txt ("" = none)
  bool rank_heldout;                 // -rank-heldout: the held-out links ranked into heldout-ranks.txt
  bool adamic_adar;                  // -adamic-adar: link-nbr.txt / *-ranks-aa.txt / link-ranks-baselines.txt beside them

  static std::string prefix;
  static std::string file_str(const std::string &fname) { return prefix + fname; }
  static void plog(const std::string &s, const std::string &v);
  static void plog(const std::string &s, const char *v) { plog(s, std::string(v)); }
  static void plog(const std::string &s, double v);
  static void plog(const std::string &s, bool v);
  static void plog(const std::string &s, int v);
  static void plog(const std::string &s, uint32_t v);
  static void plog(const std::string &s, uint64_t v);

 private:
  static FILE *plogf_;
};

}  // namespace svinet
