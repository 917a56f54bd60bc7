#include "env.hh"

#include <sys/stat.h>
#include <unistd.h>

#include <cerrno>
#include <cstdlib>
#include <cstring>
#include <sstream>

namespace svinet {

std::string Env::prefix;
FILE *Env::plogf_ = nullptr;

void Env::plog(const std::string &s, const std::string &v) {
  if (!plogf_) return;
  fprintf(plogf_, "%s: %s\n", s.c_str(), v.c_str());
  fflush(plogf_);
}
void Env::plog(const std::string &s, double v) {
  if (!plogf_) return;
  fprintf(plogf_, "%s: %.9f\n", s.c_str(), v);
  fflush(plogf_);
}
void Env::plog(const std::string &s, bool v) {
  if (!plogf_) return;
  fprintf(plogf_, "%s: %s\n", s.c_str(), v ? "True" : "False");
  fflush(plogf_);
}
void Env::plog(const std::string &s, int v) {
  if (!plogf_) return;
  fprintf(plogf_, "%s: %d\n", s.c_str(), v);
  fflush(plogf_);
}
void Env::plog(const std::string &s, uint32_t v) {
  if (!plogf_) return;
  fprintf(plogf_, "%s: %d\n", s.c_str(), v);
  fflush(plogf_);
}
void Env::plog(const std::string &s, uint64_t v) {
  if (!plogf_) return;
  fprintf(plogf_, "%s: %" PRIu64 "\n", s.c_str(), v);
  fflush(plogf_);
}

Env::Env(const Args &a)
    : n(a.n), k(a.k), t(2),
      alpha((double)1 / a.k),
      heldout_ratio(a.hol_ratio),
      eta0(0), eta1(0),
      eta0_dense(4700.59), eta1_dense(0.77), eta0_sparse(0.97), eta1_sparse(6.33),
      reportfreq(a.rfreq),
      epsilon(1e-30),
      max_iterations(a.max_iterations),
      seed(a.rand_seed),
      eta_type(a.eta_type),
      use_validation_stop(a.use_validation_stop),
      accuracy(a.accuracy),
      logl(a.logl),
      defer_init_gamma(a.defer_init_gamma),
      link_thresh(a.link_thresh), lt_min_deg(a.lt_min_deg),
      model_load(a.load), gamma_location(a.location),
      load_heldout(a.val_load), load_heldout_fname(a.val_file_location),
      load_test(a.test_load), load_test_fname(a.test_file_location),
      use_init_communities(a.init_comm), init_communities_fname(a.init_comm_fname),
      nmi(a.nmi), ground_truth_fname(a.ground_truth_fname),
      datfname(a.datfname), label(a.label), gpus(a.gpus), rank(a.rank), kshard(a.kshard), sharded((a.sharded || a.gpus > 1) && !a.kshard), comm_rfd(a.comm_rfd), comm_wfds(a.comm_wfds),
      batch_mode(a.batch), link_sampling(a.link_sampling), findk(a.findk), batch_device((a.batch && a.batch_gpu) || ((a.rnode || a.rpair || a.infset || a.snode) && !a.host_loops)),
      randomnode(a.rnode), randompair(a.rpair), stratified(a.stratified), delaylearn((a.rnode || a.rpair) && !a.nodelay), infset(a.infset || a.preprocess), preprocess(a.preprocess), inf_epsilon(a.inf_epsilon), snode(a.snode), sparse_graph(a.sparse_graph), orig(a.orig), orig_device(a.orig && !a.host_loops), itype(a.itype), clean_holdout(a.clean_holdout), single(a.single), single_device(a.single && !a.host_loops), single_logl(a.single_logl), sbm_alpha(0.5), s(a.n / 2), gml(a.gml), lcstats(a.lcstats), strid(a.strid),
      terminate(0), total_pairs(0), ones_prob(0), zeros_prob(1),
      device(a.device), sweep_batch(a.sweep_batch), write_files(a.write_files),
      minibatch(a.minibatch), tau0(a.tau0), kappa(a.kappa), nodetau0(a.nodetau0), nodekappa(a.nodekappa),
      sparse_after(a.sparse_after), predict_pairs_fname(a.predict_pairs_fname), recommend((uint32_t)a.recommend),
      rank_pairs_fname(a.rank_pairs_fname), rank_heldout(a.rank_heldout), adamic_adar(a.adamic_adar) {
  if (!write_files) {
    if (plogf_) { fclose(plogf_); plogf_ = nullptr; }
    prefix.clear();
    return;
  }
  // output directory name, src/env.hh:503-568: "gml" for -gml; -lcstats names it like any run (no engine suffix unless
  // one was given)
  std::ostringstream sa;
  sa << "n" << n << "-" << "k" << k;
  if (label != "") sa << "-" << label;
  else if (datfname.length() > 3 && datfname.find("mmsb_gen.dat") == std::string::npos) {
    std::string q = datfname.substr(0, 2);
    if (q == "..") q = "xx";
    sa << "-" << q;
  }
  if (seed) sa << "-seed" << seed;
  if (batch_mode) { sa << "-batch"; if (!gml) reportfreq = 1; }   // the reference names no directory for -gml (the block is skipped)
  else if (single) sa << "-sbm";                                  // src/env.hh:521-522
  else if (infset) sa << "-infset";                               // src/env.hh:523
  else if (snode) sa << (a.nodelay ? "-Srnode" : "-SUrnode");     // what the reference names a -stratified -rnode run (:529-546)
  else if (link_sampling) sa << "-linksampling";
  else if (findk) sa << "-findk";
  else if (sampled()) {   // src/env.hh:529-546 (undirected is always set there: the dash is always written)
    sa << "-";
    if (stratified) sa << "S";
    if (delaylearn) sa << "U";
    if (randompair) sa << "rpair";
    if (randomnode) sa << "rnode";
  }
  else if (orig) sa << (a.nodelay ? "-" : "-U");   // the same branch: delaylearn is set unless -nodelay was given (src/env.hh:487-490)
  if (a.nthreads > 0) sa << "-T" << a.nthreads;
  if (orig && itype > 0) sa << "-i" << itype;      // src/env.hh:551-552 (read for -orig alone: the other engines keep their names)
  const std::string name = gml ? std::string("gml") : sa.str();
  prefix = a.outdir_root.empty() ? name : a.outdir_root + "/" + name;

  fprintf(stdout, "+ Output directory: %s\n", prefix.c_str());
  fflush(stdout);
  // Logger::setup_log_dir + setup_logfd (src/log.cc:86-127): create the dir, empty infer.log
  struct stat st;
  if (stat(prefix.c_str(), &st) != 0) {
    mkdir(prefix.c_str(), S_IRWXU | S_IRWXG | S_IROTH | S_IXOTH);
    if (stat(prefix.c_str(), &st) != 0) {
      fprintf(stderr, "Warning: could not create dir %s\n", prefix.c_str());
      exit(-1);
    }
  }
  FILE *lf = fopen(file_str("/infer.log").c_str(), "w");
  if (lf) { fprintf(stdout, "+ Writing log to %s\n", file_str("/infer.log").c_str()); fclose(lf); }
  if (plogf_) fclose(plogf_);
  plogf_ = fopen(file_str("/param.txt").c_str(), "w");
  if (!plogf_) {
    printf("cannot open param file:%s\n", strerror(errno));
    exit(-1);
  }
  plog("nodes", n);
  plog("groups", k);
  plog("t", t);
  plog("minibatch (rpair or stratified rpair options only)", (uint32_t)(n / 2));
  plog("mbsize", (uint32_t)1);
  plog("alpha", alpha);
  plog("sbm_alpha", alpha);
  plog("heldout_ratio", heldout_ratio);
  plog("precision_ratio", 0.001);
  plog("stratified", stratified);
  plog("delaylearn", delaylearn);
  plog("nolambda", false);
  plog("randomnode", randomnode);
  plog("gen", false);
  plog("undirected", true);
  plog("gap", false);
  plog("nthreads", a.nthreads);
  plog("stopthresh", 0.00001);
  plog("infthresh", 0.0);
  plog("randzeros", false);
  plog("benchmark", false);
  plog("max iterations", max_iterations);
  plog("seed", seed);
  plog("use validation stop", use_validation_stop);
  plog("gamma location", gamma_location);
  plog("link_thresh", link_thresh);
  plog("lt_min_deg", lt_min_deg);
  plog("epsilon", epsilon);
  plog("sets_mini_batch", (uint32_t)(n / 100));
  plog("use_init_communities", use_init_communities);
  plog("load_test_sets", false);
  plog("val_load", load_heldout);
  plog("val_file_location", load_heldout_fname);
  plog("test_load", load_test);
  plog("test_file_location", load_test_fname);
  plog("reportfreq", reportfreq);
  plog("eta_type", eta_type);
  if (minibatch || sampled() || fastamm()) {   // keys of this build (mini-batch mode, the sampled-pair engines), after the reference's
    if (minibatch) plog("link_sampling_minibatch_nodes", minibatch);
    plog("tau0", tau0);
    plog("kappa", kappa);
    plog("nodetau0", nodetau0);
    plog("nodekappa", nodekappa);
  }
  // network.dat symlink, src/env.hh:621-625
  std::string nd = file_str("/network.dat");
  unlink(nd.c_str());
  if (symlink(datfname.c_str(), nd.c_str()) < 0)
    fprintf(stderr, "warning: cannot symlink %s: %s\n", nd.c_str(), strerror(errno));
  unlink(file_str("/mutual.txt").c_str());
}

Env::~Env() {
  if (plogf_) { fclose(plogf_); plogf_ = nullptr; }
}

}  // namespace svinet
