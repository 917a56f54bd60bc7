#include "mmsbbatch.hh"

#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <set>
#include <sstream>

#include "util.hh"

namespace svinet {

namespace {

const double kNegInit = -2147483647.0;     // _max_t/_max_h/_max_v/_prev_h, src/mmsbinfer.cc:33-38
const uint32_t kOnlineIterations = 50;     // src/env.hh:415
const double kMeanChangeThresh = 0.00001;  // src/env.hh:337
const uint32_t kNoninfSetsize = 200;       // _noninf_setsize, src/fastamm.cc:18
const uint32_t kStratSets = 10;            // _m, src/fastamm2.cc:16: a non-link step takes n / 10 nodes

}  // namespace

MMSBBatch::MMSBBatch(Env &env, Network &network)
    : env_(env), network_(network), n_(env.n), k_(env.k),
      ones_prob_(env.ones_prob), zeros_prob_(env.zeros_prob),
      rng_((unsigned long)env.seed), gamma_rng_(rng_),
      gamma_((size_t)n_ * k_), gammanext_((size_t)n_ * k_, env.alpha),
      lambda_(2 * (size_t)k_), lambdanext_(2 * (size_t)k_),
      elogpi_((size_t)n_ * k_), elogbeta_(2 * (size_t)k_),
      max_t_(kNegInit), max_h_(kNegInit), max_v_(kNegInit), prev_h_(kNegInit),
      start_time_(time(0)) {
  fprintf(stdout, "+ initialization begin\n+ running inference on %d nodes\n", n_);
  Env::plog("inference n", n_);
  if (env_.fastamm()) {                                     // src/fastamm.cc:64-66, :85: the shuffle draws before the sampler
    Env::plog("inf_epsilon", env_.inf_epsilon);
    Env::plog("noninf_setsize", env_.snode ? n_ / kStratSets : kNoninfSetsize);
    shuffle_nodes();
    nodec_.assign(n_, 0);
  }
  init_heldout();
  printf("+ heldout sets created\n");
  if (env_.fastamm()) {
    init_gamma_lambda_infset();
  } else {
    init_gamma();
    for (uint32_t k = 0; k < k_; ++k) {                     // init_lambda, :389-397
      lambda_[2 * k] = lambdanext_[2 * k] = env.eta0;
      lambda_[2 * k + 1] = lambdanext_[2 * k + 1] = env.eta1;
    }
  }
  set_dir_exp();
  if (env_.batch_device) attach_device();
  if (env_.write_files) {
    // files the reference's constructor opens (:62-166); the ones this path never writes stay empty
    for (const char *f : {"/stats.txt", "/time.txt", "/convergence.txt", "/cmap.txt", "/training.txt",
                          "/training-edges.txt", "/logl.txt", "/modularity.txt"})
      fclose(open_or_die(Env::file_str(f), f + 1));
    if (env_.fastamm())                                     // src/fastamm.cc:99, :241 (PRECISION_SAMPLE is off: both stay empty)
      for (const char *f : {"/precision-pairs.txt", "/precision.txt"}) fclose(open_or_die(Env::file_str(f), f + 1));
    hf_ = open_or_die(Env::file_str("/heldout.txt"), "heldout");
    vf_ = open_or_die(Env::file_str("/validation.txt"), "validation");
    if (env_.logl) lf_ = open_or_die(Env::file_str("/logl.txt"), "logl");   // without -logl it stays the empty file above
  }
  Env::plog("network ones", network_.ones());
  Env::plog("network singles", network_.singles());
  heldout_likelihood();
  validation_likelihood(nullptr);
  if (env_.logl) approx_log_likelihood();                   // :174-175, src/fastamm.cc:289-290
  fprintf(stdout, "+ initialization end\n");
  fflush(stdout);
  start_time_ = time(0);
}

MMSBBatch::~MMSBBatch() {
  if (hf_) fclose(hf_);
  if (vf_) fclose(vf_);
  if (lf_) fclose(lf_);
  if (dev_) svils_batch_destroy(dev_);
}

// ---------------------------------------------------------------------------
// the device backend (include/svils.h: svils_batch_*)
// ---------------------------------------------------------------------------
void MMSBBatch::device_failed(const char *what, int rc) {
  if (strstr(svils_last_error(), "phi normaliser underflow")) {   // the host loops' error line and exit status (phis())
    fprintf(stderr, "error: %s\n", svils_last_error());
    exit(-1);
  }
  throw_svils(what, rc);
}

void MMSBBatch::attach_device() {
  // -sparse-graph: the handle's sparse form, without a cap on n (no sweep, no lower bound: main() refuses those beside it)
  const char *create = env_.sparse_graph ? "svils_batch_create_sparse" : "svils_batch_create";
  if (int rc = (env_.sparse_graph ? svils_batch_create_sparse : svils_batch_create)(env_.device, n_, k_, env_.alpha, env_.eta0, env_.eta1,
                                                                                     env_.epsilon, &dev_))
    device_failed(create, rc);
  std::set<Edge> links(network_.edges().begin(), network_.edges().end()), skip;
  for (const auto &it : heldout_map_) skip.insert(it.first);
  for (const auto &it : validation_map_) skip.insert(it.first);
  std::vector<uint32_t> l, s;
  for (const Edge &e : links) { l.push_back(e.first); l.push_back(e.second); }
  for (const Edge &e : skip) { s.push_back(e.first); s.push_back(e.second); }
  if (int rc = svils_batch_set_graph(dev_, l.data(), l.size() / 2, s.data(), s.size() / 2)) device_failed("svils_batch_set_graph", rc);
  if (int rc = svils_batch_set_state(dev_, gamma_.data(), lambda_.data())) device_failed("svils_batch_set_state", rc);
}

void MMSBBatch::fetch_state() {
  if (!dev_ || !host_stale_) return;
  if (int rc = svils_batch_get_state(dev_, gamma_.data(), lambda_.data())) device_failed("svils_batch_get_state", rc);
  host_stale_ = false;
}

std::vector<double> MMSBBatch::pair_likelihoods(const std::map<Edge, bool> &pairs) {
  std::vector<double> u(pairs.size());
  size_t i = 0;
  if (!dev_) {
    for (const auto &it : pairs) u[i++] = edge_likelihood(it.first.first, it.first.second, network_.y(it.first.first, it.first.second) ? 1 : 0);
    return u;
  }
  std::vector<uint32_t> pq(2 * pairs.size());
  std::vector<uint8_t> y(pairs.size());
  for (const auto &it : pairs) {
    pq[2 * i] = it.first.first;
    pq[2 * i + 1] = it.first.second;
    y[i++] = network_.y(it.first.first, it.first.second) ? 1 : 0;
  }
  if (int rc = svils_batch_pair_loglik(dev_, pq.data(), y.data(), pairs.size(), u.data())) device_failed("svils_batch_pair_loglik", rc);
  return u;
}

// ---------------------------------------------------------------------------
// held-out / validation sets (src/mmsbinfer.cc:205-329, src/mmsbinfer.hh:690-748)
// ---------------------------------------------------------------------------
bool MMSBBatch::edge_ok(const Edge &e, bool heldout_flag, bool stratified, int family) const {
  if (e.first == e.second) return false;
  if (heldout_flag) return true;                            // the held-out draw only rejects self pairs
  if (heldout_map_.count(e) || validation_map_.count(e)) return false;
  if (stratified && (int)network_.y(e.first, e.second) != family) return false;
  return true;
}

void MMSBBatch::get_random_edge(bool heldout_flag, bool stratified, int family, Edge &e) {
  if (!stratified || heldout_flag || family == 0) {
    do {
      uint32_t a = rng_.uniform_int(n_), b = rng_.uniform_int(n_);
      e = a < b ? Edge(a, b) : Edge(b, a);
    } while (!edge_ok(e, heldout_flag, stratified, family));
  } else {
    const std::vector<Edge> &edges = network_.edges();
    do {
      e = edges[rng_.uniform_int(network_.ones())];
    } while (!edge_ok(e, heldout_flag, stratified, family));
  }
}

void MMSBBatch::set_sample(int s, bool heldout) {
  if (env_.accuracy) return;
  std::map<Edge, bool> &map = heldout ? heldout_map_ : validation_map_;
  std::vector<uint32_t> &list = heldout ? heldout_edges_ : validation_edges_;
  int c0 = 0, c1 = 0;
  const int p = s / 2;
  while (c0 < p || c1 < p) {
    Edge e;
    if (c0 == p) get_random_edge(false, true, 1, e);        // enough non-links: draw links only
    else get_random_edge(heldout && !env_.fastamm(), false, 0, e);   // FastAMM's edge_ok always looks at both maps (src/fastamm.hh:592-613)
    const bool y = network_.y(e.first, e.second);
    if ((!y && c0 < p) || (y && c1 < p)) {
      (y ? c1 : c0)++;
      list.push_back(e.first);
      list.push_back(e.second);
      map[e] = true;
    }
  }
}

std::string MMSBBatch::edgelist_s(const std::vector<uint32_t> &pairs) const {
  std::ostringstream sa;
  const std::vector<uint32_t> &s2i = network_.seq2id();
  for (size_t i = 0; i + 1 < pairs.size(); i += 2) sa << s2i[pairs[i]] << "\t" << s2i[pairs[i + 1]] << "\n";
  return sa.str();
}

void MMSBBatch::init_heldout() {
  const int s = (int)(env_.heldout_ratio * network_.ones());
  set_sample(s, true);
  set_sample(s, false);
  Env::plog("heldout ratio", env_.heldout_ratio);
  Env::plog("heldout edges (1s and 0s)", (uint32_t)heldout_map_.size());
  if (!env_.write_files) return;
  // (FastAMM names them -pairs, src/fastamm.cc:87-97)
  FILE *f = open_or_die(Env::file_str(env_.fastamm() ? "/heldout-pairs.txt" : "/heldout-edges.txt"), "heldout edges");
  fprintf(f, "%s\n", edgelist_s(heldout_edges_).c_str());
  fclose(f);
  f = open_or_die(Env::file_str(env_.fastamm() ? "/validation-pairs.txt" : "/validation-edges.txt"), "validation edges");
  fprintf(f, "%s\n", edgelist_s(validation_edges_).c_str());
  fclose(f);
}

// ---------------------------------------------------------------------------
// gamma initialisation: gsl_ran_gamma(r, 100, 1/100) per cell (src/mmsbinfer.cc:372-387).
// GSL's sampler is Marsaglia-Tsang driven by its ziggurat Gaussian, whose tables are internal to
// GSL; this is the same Marsaglia-Tsang recipe over the same MT19937 stream but with a polar
// Box-Muller Gaussian, so the distribution matches and the stream does not (parity unpinned,
// SURVEY 8c).
// ---------------------------------------------------------------------------
void MMSBBatch::init_gamma() {
  for (size_t i = 0; i < gamma_.size(); ++i) gamma_[i] = gamma_rng_.gamma(100, 1. / 100);
}

void MMSBBatch::set_dir_exp() {                             // src/mmsbinfer.hh:563-580 (same as A5)
  for (uint32_t i = 0; i < n_; ++i) {
    const double *g = &gamma_[(size_t)i * k_];
    double s = 0;
    for (uint32_t k = 0; k < k_; ++k) s += g[k];
    const double ps = digamma(s);
    for (uint32_t k = 0; k < k_; ++k) elogpi_[(size_t)i * k_ + k] = digamma(g[k]) - ps;
  }
  set_elogbeta();
}

void MMSBBatch::set_elogbeta() {                            // set_dir_exp(_lambda, _Elogbeta)
  for (uint32_t k = 0; k < k_; ++k) {
    const double ps = digamma(lambda_[2 * k] + lambda_[2 * k + 1]);
    elogbeta_[2 * k] = digamma(lambda_[2 * k]) - ps;
    elogbeta_[2 * k + 1] = digamma(lambda_[2 * k + 1]) - ps;
  }
}

// lambda a step rho towards eta + scale lambdat (:613-631, src/fastamm.cc:604-616, src/fastamm2.cc:626-638); rho < 0: lambda waits
void MMSBBatch::blend_lambda(double rho, double scale, const std::vector<double> &lambdat) {
  if (!(rho >= 0)) return;
  for (uint32_t k = 0; k < k_; ++k) {
    lambda_[2 * k] = (1 - rho) * lambda_[2 * k] + rho * (env_.eta0 + scale * lambdat[2 * k]);
    lambda_[2 * k + 1] = (1 - rho) * lambda_[2 * k + 1] + rho * (env_.eta1 + scale * lambdat[2 * k + 1]);
  }
}

// ---------------------------------------------------------------------------
// PhiComp (src/mmsbinfer.hh:104-203): Jacobi-style fixed point of the two indicator vectors of
// one pair, at most 50 rounds, convergence tested on odd rounds against the vectors of two rounds ago
// ---------------------------------------------------------------------------
void MMSBBatch::phis(uint32_t p, uint32_t q, int y, double *phi1, double *phi2) const {
  const uint32_t K = k_;
  const double logeps = log(env_.epsilon);
  std::vector<double> buf(5 * (size_t)K);
  double *elogf = &buf[0], *old1 = &buf[K], *old2 = &buf[2 * K], *nx1 = &buf[3 * K], *nx2 = &buf[4 * K];
  for (uint32_t k = 0; k < K; ++k) {
    phi1[k] = phi2[k] = 1. / K;
    elogf[k] = elogbeta_[2 * k] * y + elogbeta_[2 * k + 1] * (1 - y);
    old1[k] = old2[k] = 0;
  }
  auto update = [&](const double *b, uint32_t c, double *next) {
    double s = 0;
    for (uint32_t k = 0; k < K; ++k) {
      const double u = y == 1 ? (1 - b[k]) * logeps : .0;
      next[k] = exp(elogpi_[(size_t)c * K + k] + elogf[k] * b[k] + u);
      s += next[k];
    }
    if (!(s > .0)) {
      fprintf(stderr, "error: phi normaliser underflow for pair (%u,%u)\n", p, q);   // reference: assert(s > .0)
      exit(-1);
    }
    for (uint32_t k = 0; k < K; ++k) next[k] /= s;
  };
  for (uint32_t i = 0; i < kOnlineIterations; ++i) {
    if (i % 2 == 0)
      for (uint32_t k = 0; k < K; ++k) { old1[k] = phi1[k]; old2[k] = phi2[k]; }
    update(phi2, p, nx1);
    update(phi1, q, nx2);
    double m1 = 0, m2 = 0;
    for (uint32_t k = 0; k < K; ++k) {
      m1 += fabs(nx1[k] - old1[k]);
      m2 += fabs(nx2[k] - old2[k]);
      phi1[k] = nx1[k];
      phi2[k] = nx2[k];
    }
    if (i % 2 == 0) continue;
    if (m1 / K < kMeanChangeThresh && m2 / K < kMeanChangeThresh) break;
  }
}

void MMSBBatch::sweep() {                                   // src/mmsbinfer.cc:846-889
  if (dev_) {
    if (int rc = svils_batch_sweep(dev_, 1)) device_failed("svils_batch_sweep", rc);
    host_stale_ = true;
    iter_++;
    return;
  }
  set_dir_exp();
  std::vector<double> phi1(k_), phi2(k_);
  for (uint32_t p = 0; p < n_; ++p)
    for (uint32_t q = p + 1; q < n_; ++q) {
      const Edge e(p, q);
      if (heldout_map_.count(e) || validation_map_.count(e)) continue;
      const int y = network_.y(p, q) ? 1 : 0;
      phis(p, q, y, phi1.data(), phi2.data());
      for (uint32_t k = 0; k < k_; ++k) {
        gammanext_[(size_t)p * k_ + k] += phi1[k];
        gammanext_[(size_t)q * k_ + k] += phi2[k];
        lambdanext_[2 * k + (y ? 0 : 1)] += phi1[k] * phi2[k];
      }
    }
  gamma_ = gammanext_;
  gammanext_.assign(gammanext_.size(), env_.alpha);
  lambda_ = lambdanext_;
  for (uint32_t k = 0; k < k_; ++k) { lambdanext_[2 * k] = env_.eta0; lambdanext_[2 * k + 1] = env_.eta1; }
  iter_++;
}

// ---------------------------------------------------------------------------
// -rnode / -rpair: MMSBInfer::infer (src/mmsbinfer.cc:459-740)
// ---------------------------------------------------------------------------
std::vector<uint32_t> MMSBBatch::node_pairs(uint32_t a) const {   // :1867-1876
  std::vector<uint32_t> out;
  for (uint32_t i = 0; i < n_; ++i) {
    if (i == a) continue;
    const Edge e = a < i ? Edge(a, i) : Edge(i, a);
    if (!edge_ok(e, false, false, 0)) continue;
    out.push_back(e.first);
    out.push_back(e.second);
  }
  return out;
}

MMSBBatch::Drawn MMSBBatch::draw() {
  Drawn d;
  const uint32_t it = drawn_++, mbsize = env_.s;             // _env.m = 1 (:483-485)
  d.family = family_;
  if (env_.randomnode) {                                     // get_subsample, :1931-1936
    d.node = rng_.uniform_int(n_);
    d.scale = (double)n_ / 2;                                // :576
  } else {
    do {                                                     // :1926-1930, :1941
      Edge e;
      get_random_edge(false, env_.stratified, family_, e);
      d.pairs.push_back(e.first);
      d.pairs.push_back(e.second);
    } while (d.pairs.size() / 2 < mbsize);
    double scale = (double)env_.total_pairs;                 // :566-568
    if (env_.stratified) scale = env_.total_pairs * (family_ ? ones_prob_ : zeros_prob_);
    d.scale = scale / mbsize;                                // :587, :631
  }
  d.rho_gamma = pow(env_.nodetau0 + 1 + (double)it / 100, -1 * env_.nodekappa);   // :584 with :18; _nodec[i] = the iteration
  if (!env_.delaylearn || (uint64_t)it * env_.s > env_.total_pairs) {               // :613
    if (!delay_reported_) {
      lambda_start_iter_ = it;
      Env::plog("learning lambda since (time)", (int)duration());
      Env::plog("learning lambda since (iter)", it);
      Env::plog("lambda start iter", lambda_start_iter_);
      delay_reported_ = true;
    }
    d.rho_lambda = pow(env_.tau0 + 1 + (it - lambda_start_iter_ + 1), -1 * env_.kappa);   // :622 with :17
  }
  if (env_.stratified) family_ = family_ ? 0 : 1;            // :682-683
  return d;
}

void MMSBBatch::step_host(const Drawn &d) {                  // :513-642, process() :1092-1190 with subsample_scale = 1
  set_dir_exp();
  const std::vector<uint32_t> pairs = env_.randomnode ? node_pairs(d.node) : d.pairs;
  std::vector<double> gammat((size_t)n_ * k_, 0.0), lambdat(2 * (size_t)k_, 0.0), phi1(k_), phi2(k_);
  for (size_t x = 0; x + 1 < pairs.size(); x += 2) {
    const uint32_t p = pairs[x], q = pairs[x + 1];
    const int y = network_.y(p, q) ? 1 : 0;
    phis(p, q, y, phi1.data(), phi2.data());
    for (uint32_t k = 0; k < k_; ++k) {
      gammat[(size_t)p * k_ + k] += phi1[k];
      gammat[(size_t)q * k_ + k] += phi2[k];
      lambdat[2 * k + (y ? 0 : 1)] += phi1[k] * phi2[k];
    }
  }
  for (size_t x = 0; x < gamma_.size(); ++x)
    gamma_[x] = (1 - d.rho_gamma) * gamma_[x] + d.rho_gamma * (env_.alpha + d.scale * gammat[x]);
  blend_lambda(d.rho_lambda, d.scale, lambdat);
}

// ---------------------------------------------------------------------------
// -infset: FastAMM (src/fastamm.cc).  _iter and _lambda_start_iter are never initialised there: both are 0 here
// ---------------------------------------------------------------------------
void MMSBBatch::shuffle_nodes() {                           // :506-511; gsl_ran_shuffle: i from n - 1 down, j = uniform_int(i + 1)
  shuffled_.resize(n_);
  for (uint32_t i = 0; i < n_; ++i) shuffled_[i] = i;
  for (uint32_t i = n_ - 1; i > 0; --i) std::swap(shuffled_[i], shuffled_[rng_.uniform_int(i + 1)]);
}

void MMSBBatch::init_gamma_lambda_infset() {                // :514-546 (k < 100 for gamma, k <= 100 for lambda)
  const double vg = k_ < 100 ? 1.0 : 100.0 / k_, vl = k_ <= 100 ? 1.0 : 100.0 / k_;
  for (size_t i = 0; i < gamma_.size(); ++i) gamma_[i] = gamma_rng_.gamma(100 * vg, 0.01);
  for (uint32_t k = 0; k < k_; ++k)
    for (uint32_t t = 0; t < 2; ++t) lambda_[2 * k + t] = lambdanext_[2 * k + t] = (t ? env_.eta1 : env_.eta0) + gamma_rng_.gamma(100 * vl, 0.01);
}

MMSBBatch::Star MMSBBatch::draw_star() {
  Star d;
  const uint32_t it = drawn_++;
  d.kind = rng_.uniform() < env_.inf_epsilon ? 1 : 0;       // gsl_ran_bernoulli (:574)
  const uint32_t a = d.start = rng_.uniform_int(n_);        // :917, :1054
  auto take = [&](uint32_t j, bool y) {
    d.partner.push_back(j);
    d.y.push_back(y ? 1 : 0);
  };
  auto ok = [&](uint32_t j) { return edge_ok(a < j ? Edge(a, j) : Edge(j, a), false, false, 0); };
  const std::vector<uint32_t> &zeros = network_.sparse_zeros(a);
  if (d.kind == 0) {                                        // opt_process: the links (:925-979), then the informative set (:988-1041)
    for (uint32_t j : network_.get_edges(a))
      if (ok(j)) take(j, true);
    for (uint32_t j : zeros)
      if (ok(j)) take(j, false);
    d.scale = (double)n_ / 2;                               // :587-588
  } else {                                                  // opt_process_noninf (:1062-1090)
    // inf_map.find(node)->second on a missing key reads as false with libstdc++: a node outside the informative set.
    // The reference walks on until it has 200 pairs, round the shuffled order again if need be (a node then listed
    // twice); here the walk ends after one lap, so that a partner is listed once
    std::set<uint32_t> inf(zeros.begin(), zeros.end());
    uint32_t q = (uint32_t)((int)((double)rng_.uniform_int(n_) / kNoninfSetsize)) * kNoninfSetsize;
    for (uint32_t seen = 0; seen < n_ && d.partner.size() < kNoninfSetsize; ++seen, q = (q + 1) % n_) {
      const uint32_t node = shuffled_[q];
      if (node == a || network_.y(a, node) || !ok(node) || inf.count(node)) continue;
      take(node, false);
    }
    d.scale = ((double)n_ * (double)n_) / (2 * env_.inf_epsilon * kNoninfSetsize);
  }
  // every row of the star moves with the step size of its own counter (:592-602); the counters are part of the draw
  d.rho_start = pow(env_.nodetau0 + 1 + nodec_[a], -1 * env_.nodekappa);
  nodec_[a]++;
  for (uint32_t j : d.partner) {
    d.rho_partner.push_back(pow(env_.nodetau0 + 1 + nodec_[j], -1 * env_.nodekappa));
    nodec_[j]++;
  }
  d.rho_lambda = pow(env_.tau0 + 1 + (it - lambda_start_iter_ + 1), -1 * env_.kappa);   // :605 (nolambda is never set here)
  return d;
}

// FPhiComp (src/fastamm.hh) normalises by log-sum-exp where PhiComp divides by the sum: the same fixed point at rounding
// level, so phis() above stands for both
void MMSBBatch::star_host(const Star &d) {
  const uint32_t a = d.start, K = k_;
  auto row_exp = [&](uint32_t i) {                          // set_dir_exp(a, _gamma, _Elogpi), :921, :943
    const double *g = &gamma_[(size_t)i * K];
    double s = 0;
    for (uint32_t k = 0; k < K; ++k) s += g[k];
    const double ps = digamma(s);
    for (uint32_t k = 0; k < K; ++k) elogpi_[(size_t)i * K + k] = digamma(g[k]) - ps;
  };
  set_elogbeta();                                           // :566
  row_exp(a);
  std::vector<double> ta(K, 0.0), tj(K), lambdat(2 * (size_t)K, 0.0), phi1(K), phi2(K);
  auto blend = [&](uint32_t i, double rho, const std::vector<double> &t) {   // :594-598
    for (uint32_t k = 0; k < K; ++k)
      gamma_[(size_t)i * K + k] = (1 - rho) * gamma_[(size_t)i * K + k] + rho * (env_.alpha + d.scale * t[k]);
  };
  for (size_t e = 0; e < d.partner.size(); ++e) {
    const uint32_t j = d.partner[e], p = std::min(a, j), q = std::max(a, j);
    const int y = d.y[e];
    row_exp(j);
    phis(p, q, y, phi1.data(), phi2.data());
    const std::vector<double> &pa = p == a ? phi1 : phi2, &pj = p == a ? phi2 : phi1;
    for (uint32_t k = 0; k < K; ++k) {
      ta[k] += pa[k];
      tj[k] = pj[k];
      lambdat[2 * k + (y ? 0 : 1)] += phi1[k] * phi2[k];
    }
    blend(j, d.rho_partner[e], tj);                         // a partner is listed once: its gammat is this pair's phi
  }
  blend(a, d.rho_start, ta);
  blend_lambda(d.rho_lambda, d.scale, lambdat);
}

// ---------------------------------------------------------------------------
// -snode: FastAMM2 (src/fastamm2.cc).  _iter and _lambda_start_iter are never initialised there: both are 0 here
// ---------------------------------------------------------------------------
MMSBBatch::Star MMSBBatch::draw_strat() {
  Star d;
  const uint32_t it = drawn_++;
  const double eps = env_.inf_epsilon;                      // 0.5 (:15)
  d.kind = rng_.uniform() < eps ? 1 : 0;                    // gsl_ran_bernoulli (:574)
  const uint32_t a = d.start = rng_.uniform_int(n_);        // :936, :1078
  auto ok = [&](uint32_t j) { return edge_ok(a < j ? Edge(a, j) : Edge(j, a), false, false, 0); };
  if (d.kind == 0) {                                        // opt_process: the links (:944-1000); no informative set (:1009)
    for (uint32_t j : network_.get_edges(a))
      if (ok(j)) {
        d.partner.push_back(j);
        d.y.push_back(1);
      }
    d.scale = (double)n_ / (2 * (1 - eps));                 // :591-592
  } else {                                                  // opt_process_noninf (:1101-1125)
    // The reference walks on until it has setsize nodes -- for ever when fewer qualify; here the walk ends after one
    // lap of the shuffled order, as -infset's does
    const uint32_t setsize = n_ / kStratSets;
    if (setsize) {
      uint32_t q = (uint32_t)((int)((double)rng_.uniform_int(n_) / setsize)) * setsize;
      for (uint32_t seen = 0; seen < n_ && d.partner.size() < setsize; ++seen, q = (q + 1) % n_) {
        const uint32_t node = shuffled_[q];
        if (node == a || network_.y(a, node) || !ok(node)) continue;
        d.partner.push_back(node);
        d.y.push_back(0);
      }
    }
    d.scale = ((double)n_ * kStratSets) / (2 * eps);
  }
  // one step size for all n rows: _nodec[i] is incremented for every i at every iteration (:606, :622)
  d.rho_start = pow(env_.nodetau0 + 1 + it, -1 * env_.nodekappa);
  d.rho_partner.assign(d.partner.size(), d.rho_start);
  d.rho_lambda = pow(env_.tau0 + 1 + (it - lambda_start_iter_ + 1), -1 * env_.kappa);   // :627 (nolambda is never set here)
  return d;
}

void MMSBBatch::strat_host(const Star &d) {
  const uint32_t a = d.start, K = k_;
  set_dir_exp();                                            // every row from the gamma the iteration began with
  std::vector<double> gammat((size_t)n_ * K, 0.0), lambdat(2 * (size_t)K, 0.0), phi1(K), phi2(K);
  std::vector<char> named(n_, 0);
  named[a] = 1;
  for (size_t e = 0; e < d.partner.size(); ++e) {
    const uint32_t j = d.partner[e], p = std::min(a, j), q = std::max(a, j);
    const int y = d.y[e];
    named[j] = 1;
    phis(p, q, y, phi1.data(), phi2.data());
    for (uint32_t k = 0; k < K; ++k) {
      gammat[(size_t)p * K + k] += phi1[k];
      gammat[(size_t)q * K + k] += phi2[k];
      lambdat[2 * k + (y ? 0 : 1)] += phi1[k] * phi2[k];
    }
  }
  const double rho = d.rho_start;
  for (uint32_t i = 0; i < n_; ++i)                         // :605-624: every row moves
    for (uint32_t k = 0; k < K; ++k) {
      double &g = gamma_[(size_t)i * K + k];
      g = named[i] ? (1 - rho) * g + rho * (env_.alpha + d.scale * gammat[(size_t)i * K + k]) : (1 - rho) * g + rho * env_.alpha;
    }
  blend_lambda(d.rho_lambda, d.scale, lambdat);
}

// -infset / -snode: a chunk of stars -- drawn, then run by the host loops or flattened once into the lists of one device call
void MMSBBatch::step_stars(uint32_t nsteps) {
  const bool strat = env_.snode;
  std::vector<Star> chunk(nsteps);
  for (Star &d : chunk) d = strat ? draw_strat() : draw_star();
  if (!dev_) {
    for (const Star &d : chunk) strat ? strat_host(d) : star_host(d);
  } else if (nsteps) {
    std::vector<uint32_t> start(nsteps), partner;
    std::vector<uint64_t> off(nsteps + 1, 0);
    std::vector<uint8_t> y;
    std::vector<double> rp, rs(nsteps), sc(nsteps), rl(nsteps);
    for (uint32_t s = 0; s < nsteps; ++s) {
      const Star &d = chunk[s];
      start[s] = d.start;
      partner.insert(partner.end(), d.partner.begin(), d.partner.end());
      y.insert(y.end(), d.y.begin(), d.y.end());
      rp.insert(rp.end(), d.rho_partner.begin(), d.rho_partner.end());
      off[s + 1] = partner.size();
      rs[s] = d.rho_start;
      sc[s] = d.scale;
      rl[s] = d.rho_lambda;
    }
    // -snode: rho_start carries the step's one rho_gamma, and rp is not handed over
    const char *call = strat ? "svils_batch_step_strat" : "svils_batch_step_star";
    if (int rc = strat ? svils_batch_step_strat(dev_, nsteps, start.data(), off.data(), partner.data(), y.data(), rs.data(), sc.data(), rl.data())
                       : svils_batch_step_star(dev_, nsteps, start.data(), off.data(), partner.data(), y.data(), rp.data(), rs.data(), sc.data(),
                                               rl.data()))
      device_failed(call, rc);
    host_stale_ = true;
  }
  iter_ += nsteps;
  if (keep_schedule_)
    for (Star &d : chunk) stars_.push_back(std::move(d));
}

void MMSBBatch::step(uint32_t nsteps) {
  if (env_.infset || env_.snode) return step_stars(nsteps);
  std::vector<Drawn> chunk(nsteps);
  for (Drawn &d : chunk) d = draw();
  if (!dev_) {
    for (const Drawn &d : chunk) step_host(d);
  } else if (nsteps) {
    std::vector<double> rg(nsteps), rl(nsteps);
    for (uint32_t s = 0; s < nsteps; ++s) { rg[s] = chunk[s].rho_gamma; rl[s] = chunk[s].rho_lambda; }
    if (env_.randomnode) {
      std::vector<uint32_t> nodes(nsteps);
      for (uint32_t s = 0; s < nsteps; ++s) nodes[s] = chunk[s].node;
      if (int rc = svils_batch_step_node(dev_, nsteps, nodes.data(), chunk[0].scale, rg.data(), rl.data())) device_failed("svils_batch_step_node", rc);
    } else {
      std::vector<uint64_t> off(nsteps + 1, 0);
      std::vector<uint32_t> pairs;
      std::vector<double> scale(nsteps);
      for (uint32_t s = 0; s < nsteps; ++s) {
        pairs.insert(pairs.end(), chunk[s].pairs.begin(), chunk[s].pairs.end());
        off[s + 1] = pairs.size() / 2;
        scale[s] = chunk[s].scale;
      }
      if (int rc = svils_batch_step_pairs(dev_, nsteps, off.data(), pairs.data(), scale.data(), rg.data(), rl.data()))
        device_failed("svils_batch_step_pairs", rc);
    }
    host_stale_ = true;
  }
  iter_ += nsteps;
  if (keep_schedule_)
    for (Drawn &d : chunk) schedule_.push_back(std::move(d));
}

int MMSBBatch::infer() {
  for (;;) {
    if (env_.max_iterations && iter_ > env_.max_iterations) {
      printf("+ Quitting: reached max iterations.\n");
      Env::plog("maxiterations reached", true);
      // The reference exits here without saving, MMSBInfer and FastAMM alike (src/fastamm.cc:559-563).  This build saves the
      // model, for -infset as for -rnode / -rpair and batch_infer(): a bounded run leaves usable output
      do_on_stop();
      return 0;
    }
    // drawing never depends on the state: everything up to the next report goes to the device in one call
    uint32_t todo = env_.reportfreq - iter_ % env_.reportfreq;
    if (env_.max_iterations) todo = std::min(todo, env_.max_iterations + 1 - iter_);
    step(todo);
    if (iter_ % env_.reportfreq == 0) {                      // :709-738
      if (report()) {
        do_on_stop();
        return 1;
      }
      printf("\riteration = %d took %d secs", iter_, duration());
      fflush(stdout);
      if (env_.terminate) {
        do_on_stop();
        env_.terminate = 0;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// likelihoods and the stop rule
// ---------------------------------------------------------------------------
double MMSBBatch::edge_likelihood(uint32_t p, uint32_t q, int y) const {
  const double *gp = &gamma_[(size_t)p * k_], *gq = &gamma_[(size_t)q * k_];
  double sp = 0, sq = 0;
  for (uint32_t k = 0; k < k_; ++k) { sp += gp[k]; sq += gq[k]; }
  double s = 0;
  if (y == 1) {
    for (uint32_t z = 0; z < k_; ++z)
      s += (gp[z] / sp) * (gq[z] / sq) * (lambda_[2 * z] / (lambda_[2 * z] + lambda_[2 * z + 1]));
  } else {
    for (uint32_t zp = 0; zp < k_; ++zp)
      for (uint32_t zq = 0; zq < k_; ++zq) {
        const double brate = zp == zq ? lambda_[2 * zp] / (lambda_[2 * zp] + lambda_[2 * zp + 1]) : env_.epsilon;
        s += (gp[zp] / sp) * (gq[zq] / sq) * (1 - brate);
      }
  }
  if (s < 1e-30) s = 1e-30;
  return log(s);
}

bool MMSBBatch::heldout_likelihood() {                      // src/mmsbinfer.cc:2086-2174
  if (env_.accuracy) return false;
  uint32_t k = 0, kzeros = 0, kones = 0;
  double s = 0, szeros = 0, sones = 0;
  const std::vector<double> us = pair_likelihoods(heldout_map_);
  size_t at = 0;
  for (const auto &it : heldout_map_) {
    const int y = network_.y(it.first.first, it.first.second) ? 1 : 0;
    const double u = us[at++];
    s += u;
    k++;
    if (y) { sones += u; kones++; } else { szeros += u; kzeros++; }
  }
  const double nshol = zeros_prob_ * (szeros / kzeros) + ones_prob_ * (sones / kones);
  const double row[10] = {(double)iter_, s / k, (double)k, szeros / kzeros, (double)kzeros, sones / kones,
                          (double)kones, zeros_prob_ * (szeros / kzeros), ones_prob_ * (sones / kones), nshol};
  rows_.insert(rows_.end(), row, row + 10);
  if (hf_) {
    fprintf(hf_, "%d\t%d\t%.9f\t%d\t%.9f\t%d\t%.9f\t%d\t%.9f\t%.9f\t%.9f\n", iter_, duration(), s / k, k,
            szeros / kzeros, kzeros, sones / kones, kones, row[7], row[8], nshol);
    fflush(hf_);
  }
  const double a = nshol;
  bool stop = false;
  int why = -1;
  if (iter_ > n_ || iter_ > 5000) {
    if (a > prev_h_ && prev_h_ != 0 && fabs((a - prev_h_) / prev_h_) < 0.00001) {
      stop = true;
      why = 0;
    } else if (a < prev_h_) {
      nh_++;
    } else if (a > prev_h_) {
      nh_ = 0;
    }
    if (a > max_h_) {
      double av = 0;
      validation_likelihood(&av);
      max_h_ = a;
      max_v_ = av;
      max_t_ = 0;
    }
    if (nh_ > 2) { why = 1; stop = true; }
  }
  prev_h_ = nshol;
  if (env_.write_files) {
    FILE *f = open_or_die(Env::file_str("/max.txt"), "max");
    fprintf(f, "%d\t%d\t%.5f\t%.5f\t%.5f\t%.5f\t%d\n", iter_, duration(), a, max_t_, max_h_, max_v_, why);
    fclose(f);
  }
  return env_.use_validation_stop && stop;
}

void MMSBBatch::validation_likelihood(double *av) {         // src/mmsbinfer.cc:2177-2224
  if (env_.accuracy) return;
  uint32_t k = 0, kzeros = 0, kones = 0;
  double s = 0, szeros = 0, sones = 0;
  const std::vector<double> us = pair_likelihoods(validation_map_);
  size_t at = 0;
  for (const auto &it : validation_map_) {
    const int y = network_.y(it.first.first, it.first.second) ? 1 : 0;
    const double u = us[at++];
    s += u;
    k++;
    if (y) { sones += u; kones++; } else { szeros += u; kzeros++; }
  }
  if (vf_) {
    fprintf(vf_, "%d\t%d\t%.5f\t%d\t%.5f\t%d\t%.5f\t%d\n", iter_, duration(), s / k, k, szeros / kzeros, kzeros,
            sones / kones, kones);
    fflush(vf_);
  }
  if (av) *av = s / k;
}

bool MMSBBatch::report() {                                  // src/mmsbinfer.cc:895-905
  if (!dev_) set_dir_exp();                                 // (the device forms Elogpi / Elogbeta at the head of its sweep)
  if (heldout_likelihood()) return true;                    // (the reference exits there: no row of logl.txt)
  validation_likelihood(nullptr);
  if (env_.logl) approx_log_likelihood();                   // :726-727, :914-915, src/fastamm.cc:668-669
  return false;
}

// ---------------------------------------------------------------------------
// -logl: the variational lower bound (src/mmsbinfer.cc:1948-2083, src/fastamm.cc:1129-1258)
// ---------------------------------------------------------------------------
double MMSBBatch::elbo(double *parts) {
  double out[4] = {0, 0, 0, 0};
  if (dev_) {
    if (int rc = svils_batch_elbo(dev_, out, nullptr, nullptr)) device_failed("svils_batch_elbo", rc);
  } else {
    set_dir_exp();
    const uint32_t K = k_;
    const double logeps = log(env_.epsilon);
    double G = 0, P = 0, N = 0;
    for (uint32_t k = 0; k < K; ++k) {                      // :1962-1982
      const double *l = &lambda_[2 * k], *e = &elogbeta_[2 * k];
      G += std::lgamma(env_.eta0 + env_.eta1) - (std::lgamma(env_.eta0) + std::lgamma(env_.eta1));
      G += (env_.eta0 - 1) * e[0] + (env_.eta1 - 1) * e[1];
      G -= std::lgamma(l[0] + l[1]) - (std::lgamma(l[0]) + std::lgamma(l[1]));
      G -= (l[0] - 1) * e[0] + (l[1] - 1) * e[1];
    }
    std::vector<double> phi1(K), phi2(K);
    for (uint32_t p = 0; p < n_; ++p)                       // :1984-2029
      for (uint32_t q = p + 1; q < n_; ++q) {
        const Edge e(p, q);
        if (heldout_map_.count(e) || validation_map_.count(e)) continue;
        const int y = network_.y(p, q) ? 1 : 0;
        phis(p, q, y, phi1.data(), phi2.data());
        const double *ep = &elogpi_[(size_t)p * K], *eq = &elogpi_[(size_t)q * K];
        double t = 0, s1 = 0, s2 = 0, spp = 0;
        for (uint32_t k = 0; k < K; ++k) {
          const double pp = phi1[k] * phi2[k];
          t += pp * (elogbeta_[2 * k] * y + elogbeta_[2 * k + 1] * (1 - y));
          s1 += phi1[k];
          s2 += phi2[k];
          spp += pp;
        }
        if (y == 1) t += logeps * (s1 * s2 - spp);          // the g != h double loop
        for (uint32_t k = 0; k < K; ++k) t += phi1[k] * ep[k] + phi2[k] * eq[k];
        for (uint32_t k = 0; k < K; ++k) {                  // 0 log 0 = 0
          if (phi1[k] > 0) t -= log(phi1[k]) * phi1[k];
          if (phi2[k] > 0) t -= log(phi2[k]) * phi2[k];
        }
        P += t;
      }
    for (uint32_t p = 0; p < n_; ++p) {                     // :2031-2056
      const double *g = &gamma_[(size_t)p * K], *ep = &elogpi_[(size_t)p * K];
      double se = 0, sg = 0, sl = 0, sge = 0;
      for (uint32_t k = 0; k < K; ++k) {
        se += ep[k];
        sg += g[k];
        sl += std::lgamma(g[k] < 1e-30 ? 1e-30 : g[k]);
        sge += (g[k] - 1) * ep[k];
      }
      N += std::lgamma(K * env_.alpha) - K * std::lgamma(env_.alpha) + (env_.alpha - 1) * se - (std::lgamma(sg) - sl) - sge;
    }
    out[0] = G + P + N;
    out[1] = G;
    out[2] = P;
    out[3] = N;
  }
  if (parts) memcpy(parts, out, sizeof out);
  return out[0];
}

double MMSBBatch::approx_log_likelihood() {
  const double s = elbo(nullptr);
  printf("approx. log likelihood = %f\n", s);
  logl_rows_.push_back((double)iter_);
  logl_rows_.push_back(s);
  const uint32_t dur = duration();
  if (lf_) {
    fprintf(lf_, "%d\t%d\t%.5f\n", iter_, dur, s);
    fflush(lf_);
  }
  const double w = s;                                       // :2062-2081
  if (env_.accuracy && (iter_ > n_ || iter_ > 5000))
    if (w > prev_w_ && prev_w_ != 0 && fabs((w - prev_w_) / prev_w_) < 0.00001 && env_.write_files) {
      FILE *f = open_or_die(Env::file_str("/done.txt"), "done");
      fprintf(f, "%d\t%d\t%.5f\n", iter_, dur, w);
      fclose(f);
    }
  prev_w_ = w;
  return s;
}

int MMSBBatch::batch_infer() {
  for (;;) {
    if (env_.max_iterations && iter_ > env_.max_iterations) {
      printf("+ Quitting: reached max iterations.\n");
      Env::plog("maxiterations reached", true);
      // the reference exits here without saving anything (src/mmsbinfer.cc:840-844); the model is
      // written so that a bounded run leaves usable output
      do_on_stop();
      return 0;
    }
    sweep();
    if (iter_ % env_.reportfreq == 0) {
      if (report()) {
        do_on_stop();
        return 1;
      }
      printf("\riteration = %d took %d secs", iter_, duration());
      fflush(stdout);
      if (env_.terminate) {
        do_on_stop();
        env_.terminate = 0;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// writers (src/mmsbinfer.cc:743-752, 932-1062)
// ---------------------------------------------------------------------------
void MMSBBatch::do_on_stop() {
  if (!env_.write_files) return;
  fetch_state();
  save_model();
  compute_and_log_groups();
}

void MMSBBatch::save_model() {
  FILE *gf = open_or_die(Env::file_str("/gamma.txt"), "gamma");
  const std::vector<uint32_t> &s2i = network_.seq2id();
  for (uint32_t i = 0; i < n_; ++i) {
    fprintf(gf, "%d\t%d\t", i, s2i[i]);
    for (uint32_t k = 0; k < k_; ++k) fprintf(gf, k == k_ - 1 ? "%.5f\n" : "%.5f\t", gamma_[(size_t)i * k_ + k]);
  }
  fclose(gf);
  FILE *lf = open_or_die(Env::file_str("/lambda.txt"), "lambda");
  for (uint32_t k = 0; k < k_; ++k) fprintf(lf, "%d\t%.5f\t%.5f\n", k, lambda_[2 * k], lambda_[2 * k + 1]);
  fclose(lf);
}

void MMSBBatch::compute_and_log_groups() {
  FILE *groupsf = open_or_die(Env::file_str("/groups.txt"), "groups");
  FILE *summaryf = open_or_die(Env::file_str("/summary.txt"), "summary", "a");
  FILE *commf = open_or_die(Env::file_str("/communities.txt"), "communities");
  const std::vector<uint32_t> &s2i = network_.seq2id();
  std::vector<double> epi((size_t)n_ * k_), beta(k_);
  for (uint32_t i = 0; i < n_; ++i) {
    double s = 0;
    for (uint32_t k = 0; k < k_; ++k) s += gamma_[(size_t)i * k_ + k];
    for (uint32_t k = 0; k < k_; ++k) epi[(size_t)i * k_ + k] = gamma_[(size_t)i * k_ + k] / s;
  }
  for (uint32_t k = 0; k < k_; ++k) beta[k] = lambda_[2 * k] / (lambda_[2 * k] + lambda_[2 * k + 1]);
  std::map<uint32_t, std::vector<uint32_t> > communities;
  std::vector<uint32_t> groups(n_, 0), nbrs;
  uint32_t unlikely = 0;
  for (uint32_t i = 0; i < n_; ++i) {
    const double *pi = &epi[(size_t)i * k_];
    fprintf(groupsf, "%d\t%d\t", i, s2i[i]);
    double max = .0;
    for (uint32_t j = 0; j < k_; ++j) {
      fprintf(groupsf, "%.3f\t", pi[j]);
      if (pi[j] > max) { max = pi[j]; groups[i] = j; }
    }
    fprintf(groupsf, "%d\n", groups[i]);
    // the links (i, m), m > i, in ascending m, from the adjacency list where the reference asks y(i, m) of all n: the same
    // links in the same order, each once -- the reader drops repeated pairs, so get_edges() lists a neighbour once
    nbrs.clear();
    for (uint32_t m : network_.get_edges(i))
      if (m > i) nbrs.push_back(m);
    std::sort(nbrs.begin(), nbrs.end());
    for (uint32_t m : nbrs) {
      const double *pm = &epi[(size_t)m * k_];
      // inner_prod_max (src/matrix.hh:459-476): largest term of sum_k pi_i pi_m beta over the sum
      double u = .0, s = .0;
      uint32_t max_k = 0;
      for (uint32_t k = 0; k < k_; ++k) {
        const double v = pi[k] * pm[k] * beta[k];
        s += v;
        if (v > u) { u = v; max_k = k; }
      }
      if (u / s < 0.5) { unlikely++; continue; }
      communities[max_k].push_back(i);
      communities[max_k].push_back(m);
    }
  }
  printf("unlikely = %d\n", unlikely);
  std::vector<int> sizes(k_, 0);
  for (uint32_t i = 0; i < n_; ++i) sizes[groups[i]]++;
  for (uint32_t k = 0; k < k_; ++k) fprintf(summaryf, "%d\t", sizes[k]);
  fprintf(summaryf, ":%d\n\n", unlikely);
  for (const auto &c : communities) {
    std::map<uint32_t, bool> uniq;
    for (uint32_t p : c.second)
      if (!uniq.count(p)) {
        fprintf(commf, "%d ", s2i[p]);
        uniq[p] = true;
      }
    fprintf(commf, "\n");
  }
  fclose(groupsf);
  fclose(summaryf);
  fclose(commf);
}

}  // namespace svinet
