#include "mmsbinferorig.hh"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "pairfiles.hh"
#include "util.hh"

namespace svinet {

namespace {

const uint32_t kOnlineIterations = 50;     // src/env.hh: online_iterations
const double kMeanChangeThresh = 0.00001;  // src/env.hh: meanchangethresh

}  // namespace

MMSBInferOrig::MMSBInferOrig(Env &env, Network &network, int itype)
    : env_(env), network_(network), n_(env.n), k_(env.k), itype_(itype),
      total_pairs_((double)env.n * (env.n - 1) / 2),          // undirected (:34-35)
      ones_prob_((double)network.ones() / ((double)env.n * (env.n - 1) / 2)),
      rng_((unsigned long)env.seed), gamma_rng_(rng_),
      gamma_((size_t)n_ * k_), beta_((size_t)k_ * k_),
      start_time_(time(0)) {
  fprintf(stdout, "+ mmsb orig initialization begin\n+ running inference on %d nodes\n", n_);
  Env::plog("inference n", n_);
  Env::plog("total pairs", total_pairs_);
  Env::plog("ones_prob", ones_prob_);
  Env::plog("zeros_prob", 1 - ones_prob_);
  Env::plog("itype", itype_);
  if (!env_.predict_pairs_fname.empty()) load_pairs_file(network_, "-predict-pairs", env_.predict_pairs_fname, &pp_ext_, &pp_seq_);
  if (!env_.rank_pairs_fname.empty()) load_pairs_file(network_, "-rank-pairs", env_.rank_pairs_fname, &rp_ext_, &rp_seq_);
  init_heldout();
  init_skip();
  printf("+ done heldout\n");
  init_gamma();
  if (itype_ == 0) init_beta1(); else init_beta2();
  printf("+ done initializing gamma, beta\n");
  if (env_.orig_device) attach_device();
  if (env_.write_files) {
    // files the reference's constructor opens (:86-128); the ones this path never writes stay empty
    for (const char *f : {"/stats.txt", "/time.txt", "/convergence.txt", "/logl.txt", "/modularity.txt"})
      fclose(open_or_die(Env::file_str(f), f + 1));
    if (env_.logl) lf_ = open_or_die(Env::file_str("/logl.txt"), "logl");
    hf_ = open_or_die(Env::file_str("/heldout.txt"), "heldout");
    vf_ = open_or_die(Env::file_str("/validation.txt"), "validation");
  }
  Env::plog("network ones", network_.ones());
  Env::plog("network singles", network_.singles());
  likelihood_row(heldout_map_, hf_, 0);      // :129-133
  likelihood_row(validation_map_, vf_, 1);
  rule_.enabled = env_.use_validation_stop;
  if (env_.logl) approx_log_likelihood();   // :135-137: the bound of the initial state (no rule can fire at the first row)
  fprintf(stdout, "+ mmsb initialization end\n");
  fflush(stdout);
  start_time_ = time(0);
}

MMSBInferOrig::~MMSBInferOrig() {
  if (hf_) fclose(hf_);
  if (vf_) fclose(vf_);
  if (lf_) fclose(lf_);
  if (dev_) svils_orig_destroy(dev_);
}

// ---------------------------------------------------------------------------
// the device backend (include/svils.h: svils_orig_*)
// ---------------------------------------------------------------------------
void MMSBInferOrig::attach_device() {
  if (int rc = svils_orig_create(env_.device, n_, k_, env_.alpha, &dev_)) throw_svils("svils_orig_create", rc);
  std::vector<uint32_t> l, s;
  for (const Edge &e : network_.edges()) {
    l.push_back(std::min(e.first, e.second));
    l.push_back(std::max(e.first, e.second));
  }
  for (const Edge &e : skip_) { s.push_back(e.first); s.push_back(e.second); }
  if (int rc = svils_orig_set_graph(dev_, l.data(), l.size() / 2, s.data(), s.size() / 2)) throw_svils("svils_orig_set_graph", rc);
  if (int rc = svils_orig_set_state(dev_, gamma_.data(), beta_.data())) throw_svils("svils_orig_set_state", rc);
}

void MMSBInferOrig::fetch_state() {
  if (!dev_ || !host_stale_) return;
  if (int rc = svils_orig_get_state(dev_, gamma_.data(), beta_.data())) throw_svils("svils_orig_get_state", rc);
  host_stale_ = false;
}

void MMSBInferOrig::set_state(const double *gamma, const double *beta) {
  if (dev_) {
    if (int rc = svils_orig_set_state(dev_, gamma, beta)) throw_svils("svils_orig_set_state", rc);
    host_stale_ = false;
  }
  gamma_.assign(gamma, gamma + gamma_.size());
  beta_.assign(beta, beta + beta_.size());
}

void MMSBInferOrig::skip_also(const std::vector<uint32_t> &pairs) {
  for (size_t i = 0; i + 1 < pairs.size(); i += 2) extra_skip_[Edge(pairs[i], pairs[i + 1])] = true;
}

// ---------------------------------------------------------------------------
// held-out / validation sets (:361-460): pairs are two uniform_int(n) draws kept in the order drawn; the held-out draw
// rejects self pairs only, the validation draw also a pair found in either map in that orientation
// ---------------------------------------------------------------------------
void MMSBInferOrig::set_sample(int s, bool heldout) {
  std::map<Edge, bool> &map = heldout ? heldout_map_ : validation_map_;
  std::vector<uint32_t> &list = heldout ? heldout_edges_ : validation_edges_;
  int c0 = 0, c1 = 0;
  const int p = s / 2;
  while (c0 < p || c1 < p) {
    Edge e;
    for (;;) {
      e.first = rng_.uniform_int(n_);
      e.second = rng_.uniform_int(n_);
      if (e.first == e.second) continue;
      if (!heldout && (heldout_map_.count(e) || validation_map_.count(e))) continue;
      break;
    }
    const bool y = network_.y(e.first, e.second);
    if ((!y && c0 < p) || (y && c1 < p)) {   // (a held-out pair drawn twice is listed twice, as there)
      (y ? c1 : c0)++;
      list.push_back(e.first);
      list.push_back(e.second);
      map[e] = true;
    }
  }
}

// The ordered pairs a sweep leaves out.  The reference: the held-out pairs in the orientation drawn, nothing else
// (:231-235).  -clean-holdout: both orientations of every held-out and every validation pair
void MMSBInferOrig::init_skip() {
  for (const auto &it : heldout_map_) skip_.insert(it.first);
  if (!env_.clean_holdout) return;
  for (const std::map<Edge, bool> *m : {&heldout_map_, &validation_map_})
    for (const auto &it : *m) {
      skip_.insert(it.first);
      skip_.insert(Edge(it.first.second, it.first.first));
    }
}

void MMSBInferOrig::init_heldout() {
  const int s = (int)(env_.heldout_ratio * network_.ones());
  set_sample(s, true);
  set_sample(s, false);
  Env::plog("heldout ratio", env_.heldout_ratio);
  Env::plog("heldout edges (1s and 0s)", (uint32_t)heldout_map_.size());
  if (!env_.write_files) return;
  for (int which = 0; which < 2; ++which) {   // edgelist_s (:589-598): sequence ids
    const std::vector<uint32_t> &list = which ? validation_edges_ : heldout_edges_;
    FILE *f = open_or_die(Env::file_str(which ? "/validation-edges.txt" : "/heldout-edges.txt"), which ? "validation edges" : "heldout edges");
    for (size_t i = 0; i + 1 < list.size(); i += 2) fprintf(f, "%d\t%d\n", list[i], list[i + 1]);
    fprintf(f, "\n");
    fclose(f);
  }
}

// ---------------------------------------------------------------------------
// starts (:157-209)
// ---------------------------------------------------------------------------
void MMSBInferOrig::init_gamma() {
  for (size_t i = 0; i < gamma_.size(); ++i) gamma_[i] = gamma_rng_.gamma(100, 1. / 100);
}

void MMSBInferOrig::init_beta1() {
  for (size_t i = 0; i < beta_.size(); ++i) {
    double b = (double)rng_.uniform_int(100) / 100;
    if (b > 0.99) b = 0.99;
    if (b <= 0.01) b = 0.01;
    beta_[i] = b;
  }
}

void MMSBInferOrig::init_beta2() {
  const double eta0 = total_pairs_ * ones_prob_ / k_;
  double eta1 = (total_pairs_ / (k_ * k_)) - eta0;
  if (eta1 < 0) eta1 = 1.0;
  for (uint32_t i = 0; i < k_; ++i)
    for (uint32_t j = 0; j < k_; ++j) beta_[(size_t)i * k_ + j] = i == j ? eta0 / (eta0 + eta1) : env_.epsilon;
}

// ---------------------------------------------------------------------------
// one sweep (:217-271)
// ---------------------------------------------------------------------------
// update_phis_until_conv (src/mmsbinferorig.hh:186-220) from 1 / K; returns the rounds run
uint32_t MMSBInferOrig::fixed_point(const double *ep, const double *eq, const double *lf, double *phi1, double *phi2, uint32_t p,
                                    uint32_t q) const {
  const uint32_t K = k_;
  std::vector<double> n1(K), n2(K), o1(K, 0.0), o2(K, 0.0);
  for (uint32_t g = 0; g < K; ++g) phi1[g] = phi2[g] = 1.0 / K;
  uint32_t rounds = 0;
  for (uint32_t i = 0; i < kOnlineIterations; ++i) {
    if (i % 2 == 0) { o1.assign(phi1, phi1 + K); o2.assign(phi2, phi2 + K); }
    double s1 = 0, s2 = 0;
    for (uint32_t g = 0; g < K; ++g) {                        // both from the old vectors, both with lf[g][h]
      double u1 = ep[g], u2 = eq[g];
      for (uint32_t h = 0; h < K; ++h) {
        u1 += lf[(size_t)g * K + h] * phi2[h];
        u2 += lf[(size_t)g * K + h] * phi1[h];
      }
      n1[g] = exp(u1);
      n2[g] = exp(u2);
      s1 += n1[g];
      s2 += n2[g];
    }
    if (!(s1 > 0) || !(s2 > 0)) {                             // the reference asserts here (:146)
      fprintf(stderr, "error: -orig: the normaliser of pair (%u, %u) is not > 0\n", p, q);
      exit(-1);
    }
    double v1 = 0, v2 = 0;
    for (uint32_t g = 0; g < K; ++g) {
      n1[g] /= s1;
      n2[g] /= s2;
      v1 += fabs(n1[g] - o1[g]);
      v2 += fabs(n2[g] - o2[g]);
    }
    std::copy(n1.begin(), n1.end(), phi1);
    std::copy(n2.begin(), n2.end(), phi2);
    rounds = i + 1;
    if (i % 2 == 0) continue;
    if (v1 / K < kMeanChangeThresh && v2 / K < kMeanChangeThresh) break;
  }
  return rounds;
}

// Elogpi of all rows: set_dir_exp (:601-622), psi of a cell clamped at 1e-30
std::vector<double> MMSBInferOrig::elogpi_rows() const {
  const uint32_t K = k_;
  std::vector<double> elogpi((size_t)n_ * K);
  for (uint32_t i = 0; i < n_; ++i) {
    const double *g = &gamma_[(size_t)i * K];
    double s = 0;
    for (uint32_t k = 0; k < K; ++k) s += g[k];
    const double ps = digamma(s);
    for (uint32_t k = 0; k < K; ++k) elogpi[(size_t)i * K + k] = digamma(g[k] < 1e-30 ? 1e-30 : g[k]) - ps;
  }
  return elogpi;
}

void MMSBInferOrig::sweep_host() {
  const uint32_t K = k_;
  const std::vector<double> elogpi = elogpi_rows();
  std::vector<double> l0((size_t)K * K), l1((size_t)K * K);
  for (size_t e = 0; e < l0.size(); ++e) {                    // compute_f gives exactly beta or 1 - beta (:159-172)
    l0[e] = log(1 - beta_[e]);
    l1[e] = log(beta_[e]);
  }
  std::vector<double> gnext((size_t)n_ * K, env_.alpha), num((size_t)K * K, 0.0), tot((size_t)K * K, 0.0);
  std::vector<double> phi1(K), phi2(K);
  rounds_total_ = 0;
  for (uint32_t p = 0; p < n_; ++p)
    for (uint32_t q = 0; q < n_; ++q) {
      if (p == q) continue;
      const Edge e(p, q);
      if (skip_.count(e) || extra_skip_.count(e)) continue;   // an ordered pair: init_skip
      const bool y = network_.y(p, q);
      const double *lf = y ? l1.data() : l0.data();
      const uint32_t rounds = fixed_point(&elogpi[(size_t)p * K], &elogpi[(size_t)q * K], lf, phi1.data(), phi2.data(), p, q);
      rounds_total_ += rounds;
      for (uint32_t g = 0; g < K; ++g) {
        gnext[(size_t)p * K + g] += phi1[g];
        gnext[(size_t)q * K + g] += phi2[g];
        for (uint32_t h = 0; h < K; ++h) {
          const double v = phi1[g] * phi2[h];
          if (y) num[(size_t)g * K + h] += v;
          tot[(size_t)g * K + h] += v;
        }
      }
    }
  gamma_.swap(gnext);
  for (size_t e = 0; e < beta_.size(); ++e) {
    beta_[e] = num[e] / tot[e];
    if (!(beta_[e] > 0 && beta_[e] < 1)) {
      fprintf(stderr, "error: -orig: block rate (%zu, %zu) left (0, 1) after sweep %u (the block saw only links or only non-links)\n",
              e / K, e % K, iter_ + 1);
      exit(-1);
    }
  }
}

void MMSBInferOrig::sweep() {
  if (dev_) {
    if (int rc = svils_orig_sweep(dev_, 1)) throw_svils("svils_orig_sweep", rc);
    host_stale_ = true;
  } else {
    sweep_host();
  }
  iter_++;
}

// ---------------------------------------------------------------------------
// likelihoods (:463-587)
// ---------------------------------------------------------------------------
double MMSBInferOrig::edge_likelihood(uint32_t p, uint32_t q, int y) const {
  const uint32_t K = k_;
  const double *gp = &gamma_[(size_t)p * K], *gq = &gamma_[(size_t)q * K];
  double sp = 0, sq = 0;
  for (uint32_t k = 0; k < K; ++k) { sp += gp[k]; sq += gq[k]; }
  double s = 0;
  for (uint32_t g = 0; g < K; ++g)
    for (uint32_t h = 0; h < K; ++h) {
      const double b = beta_[(size_t)g * K + h];
      s += (gp[g] / sp) * (gq[h] / sq) * (y ? b : 1 - b);
    }
  return log(s);   // no clamp (:583-586)
}

void MMSBInferOrig::likelihood_row(const std::map<Edge, bool> &pairs, FILE *f, int which) {
  std::vector<double> u(pairs.size());
  std::vector<uint32_t> pq;
  std::vector<uint8_t> y;
  for (const auto &it : pairs) {
    pq.push_back(it.first.first);
    pq.push_back(it.first.second);
    y.push_back(network_.y(it.first.first, it.first.second) ? 1 : 0);
  }
  if (dev_) {
    if (int rc = svils_orig_pair_loglik(dev_, pq.data(), y.data(), pairs.size(), u.data())) throw_svils("svils_orig_pair_loglik", rc);
  } else {
    for (size_t i = 0; i < u.size(); ++i) u[i] = edge_likelihood(pq[2 * i], pq[2 * i + 1], y[i]);
  }
  uint32_t k = 0, kzeros = 0, kones = 0;                      // summed in the map's order
  double s = .0, szeros = 0, sones = 0;
  for (size_t i = 0; i < u.size(); ++i) {
    s += u[i];
    k += 1;
    if (y[i]) { sones += u[i]; kones++; } else { szeros += u[i]; kzeros++; }
  }
  if (f) {
    fprintf(f, "%d\t%d\t%.5f\t%d\t%.5f\t%d\t%.5f\t%d\n", iter_, duration(), s / k, k, szeros / kzeros, kzeros, sones / kones, kones);
    fflush(f);
  }
  const double row[8] = {(double)which, (double)iter_, s / k, (double)k, szeros / kzeros, (double)kzeros, sones / kones, (double)kones};
  rows_.insert(rows_.end(), row, row + 8);
}

void MMSBInferOrig::report() {
  fetch_state();
  if (env_.write_files) compute_and_log_groups();
  likelihood_row(heldout_map_, hf_, 0);
  likelihood_row(validation_map_, vf_, 1);
  if (env_.logl && approx_log_likelihood()) stopped_ = true;   // :287-289
}

// ---------------------------------------------------------------------------
// the variational lower bound (:624-726 under GLOBALPHIS)
// ---------------------------------------------------------------------------
void MMSBInferOrig::elbo_host(double out[3], uint64_t *pairs, uint64_t *rounds) {
  const uint32_t K = k_;
  const std::vector<double> elogpi = elogpi_rows();
  std::vector<double> l0((size_t)K * K), l1((size_t)K * K), t0((size_t)K * K), t1((size_t)K * K);
  for (size_t e = 0; e < l0.size(); ++e) {
    l0[e] = log(1 - beta_[e]);
    l1[e] = log(beta_[e]);
    t0[e] = log((1 - beta_[e]) + 1e-10);                      // the reference's log(fd[g][h] + 1e-10) (:654)
    t1[e] = log(beta_[e] + 1e-10);
  }
  auto xlogx = [](double v) { return v > 0 ? v * log(v) : 0.0; };   // (log(phi) * phi there: NaN at an exact 0)
  std::vector<double> phi1(K), phi2(K);
  uint64_t np = 0, nr = 0;
  double P = 0;
  for (uint32_t p = 0; p < n_; ++p)
    for (uint32_t q = 0; q < n_; ++q) {
      if (p == q) continue;
      const Edge e(p, q);
      if (skip_.count(e) || extra_skip_.count(e)) continue;   // the pairs a sweep visits
      const bool y = network_.y(p, q);
      const double *ep = &elogpi[(size_t)p * K], *eq = &elogpi[(size_t)q * K], *tf = y ? t1.data() : t0.data();
      nr += fixed_point(ep, eq, y ? l1.data() : l0.data(), phi1.data(), phi2.data(), p, q);
      np++;
      double t = 0;
      for (uint32_t g = 0; g < K; ++g)
        for (uint32_t h = 0; h < K; ++h) t += phi1[g] * phi2[h] * tf[(size_t)g * K + h];
      for (uint32_t k = 0; k < K; ++k) t += phi1[k] * ep[k] + phi2[k] * eq[k];
      for (uint32_t k = 0; k < K; ++k) t -= xlogx(phi1[k]) + xlogx(phi2[k]);
      P += t;
    }
  double N = 0;
  const double a = env_.alpha;
  for (uint32_t p = 0; p < n_; ++p) {                         // :668-688
    const double *g = &gamma_[(size_t)p * K], *e = &elogpi[(size_t)p * K];
    double se = 0, sg = 0, sl = 0, sge = 0;
    for (uint32_t k = 0; k < K; ++k) {
      se += e[k];
      sg += g[k];
      sl += std::lgamma(g[k] < 1e-30 ? 1e-30 : g[k]);
      sge += (g[k] - 1) * e[k];
    }
    N += std::lgamma(K * a) - K * std::lgamma(a) + (a - 1) * se - (std::lgamma(sg) - sl) - sge;
  }
  out[0] = P + N;
  out[1] = P;
  out[2] = N;
  if (pairs) *pairs = np;
  if (rounds) *rounds = nr;
}

void MMSBInferOrig::elbo(double out[3], uint64_t *pairs, uint64_t *rounds) {
  if (dev_) {
    if (int rc = svils_orig_elbo(dev_, out)) throw_svils("svils_orig_elbo", rc);
    if (int rc = svils_orig_get_elbo_stats(dev_, pairs, rounds, nullptr, nullptr)) throw_svils("svils_orig_get_elbo_stats", rc);
  } else {
    elbo_host(out, pairs, rounds);
  }
}

bool MMSBInferOrig::approx_log_likelihood() {
  double o[3];
  elbo(o);
  const double s = o[0];
  printf("approx. log likelihood = %f\n", s);
  if (lf_) {
    fprintf(lf_, "%d\t%d\t%.5f\n", iter_, duration(), s);
    fflush(lf_);
  }
  logl_rows_.push_back((double)iter_);
  logl_rows_.push_back(s);
  const OrigStopRule::Verdict v = rule_.update(iter_, s);
  if (rule_.new_max && rows_.size() >= 16) {                  // the report's own rows (the reference recomputes and re-logs them)
    const double *h = &rows_[rows_.size() - 16], *vr = h + 8;
    for (int i = 0; i < 3; ++i) { max_h_[i] = h[2 + 2 * i]; max_v_[i] = vr[2 + 2 * i]; }
  }
  if (v == OrigStopRule::GO_ON) return false;
  if (env_.write_files) {
    if (v == OrigStopRule::STOP_DROP) {                       // :717-722
      FILE *f = open_or_die(Env::file_str("/max.txt"), "max");
      fprintf(f, "%d\t%d\t%f\t%f\t%f\t%f\t%f\t%f\t%f\n", iter_, duration(), rule_.max, max_h_[0], max_h_[1], max_h_[2], max_v_[0],
              max_v_[1], max_v_[2]);
      fclose(f);
    } else {                                                  // src/mmsbinfer.cc:2062-2081
      FILE *f = open_or_die(Env::file_str("/done.txt"), "done");
      fprintf(f, "%d\t%d\t%.5f\n", iter_, duration(), s);
      fclose(f);
    }
  }
  return true;
}

int MMSBInferOrig::batch_infer() {
  printf("+ Running MMSB Orig batch inference\n");
  const bool open_end = env_.max_iterations == 0 && env_.logl && rule_.enabled;   // a stop rule ends the run
  while ((open_end || iter_ < env_.max_iterations) && !env_.terminate && !stopped_) {
    sweep();
    printf("iteration = %d took %d secs\n", iter_, duration());
    fflush(stdout);
    if (iter_ % env_.reportfreq == 0) report();
  }
  fetch_state();
  if (env_.write_files) save_model();
  if (env_.write_files && dev_) run_queries();
  return 0;
}

// ---------------------------------------------------------------------------
// link queries of the final state (include/svils.h: svils_orig_link_prob / _predict_links / _rank_links)
// ---------------------------------------------------------------------------
void MMSBInferOrig::run_queries() {
  if (!pp_seq_.empty()) {
    std::vector<double> prob(pp_seq_.size() / 2);
    if (int rc = svils_orig_link_prob(dev_, pp_seq_.data(), prob.size(), prob.data())) throw_svils("svils_orig_link_prob", rc);
    write_link_prob(network_, pp_ext_, pp_seq_, prob);
  }
  if (env_.recommend) {
    const uint32_t k = env_.recommend;
    std::vector<uint32_t> ids((size_t)n_ * k);
    std::vector<double> sc((size_t)n_ * k);
    if (int rc = svils_orig_predict_links(dev_, nullptr, 0, k, ids.data(), sc.data())) throw_svils("svils_orig_predict_links", rc);
    write_recommendations(network_, n_, k, ids, sc, nullptr);
  }
  if (env_.rank_pairs_fname.empty() && !env_.rank_heldout) return;
  auto held_out = [&](uint32_t p, uint32_t q) {   // left out of training (both orientations are: -clean-holdout)
    const Edge e(p, q), r(q, p);
    return heldout_map_.count(e) || heldout_map_.count(r) || validation_map_.count(e) || validation_map_.count(r);
  };
  auto rank = [&](const char *fname, const std::vector<uint32_t> &seq, const std::vector<int> *ext) {
    const size_t m = seq.size() / 2;
    const std::vector<uint32_t> pairs = directed_pairs(seq, nullptr);
    std::vector<uint32_t> above(2 * m), tied(2 * m), ncand(2 * m);
    std::vector<double> sc(2 * m);
    if (int rc = svils_orig_rank_links(dev_, pairs.data(), 2 * m, above.data(), tied.data(), ncand.data(), sc.data()))
      throw_svils("svils_orig_rank_links", rc);
    return write_rank_file(network_, fname, seq, ext, above, tied, ncand, sc, held_out);
  };
  std::vector<uint32_t> ho;   // the y = 1 lines of heldout-edges.txt, then of validation-edges.txt, as listed
  if (env_.rank_heldout)
    for (const std::vector<uint32_t> *t : {&heldout_edges_, &validation_edges_})
      for (size_t i = 0; i + 1 < t->size(); i += 2)
        if (network_.y((*t)[i], (*t)[i + 1])) { ho.push_back((*t)[i]); ho.push_back((*t)[i + 1]); }
  RankSum model;
  if (!env_.rank_pairs_fname.empty()) model = rank("/link-ranks.txt", rp_seq_, &rp_ext_);
  if (env_.rank_heldout) model = rank("/heldout-ranks.txt", ho, nullptr);
  write_rank_summary(model);
}

// ---------------------------------------------------------------------------
// writers (:297-358)
// ---------------------------------------------------------------------------
void MMSBInferOrig::compute_and_log_groups() {
  FILE *groupsf = open_or_die(Env::file_str("/groups.txt"), "groups");
  FILE *summaryf = open_or_die(Env::file_str("/summary.txt"), "summary", "a");
  FILE *commf = open_or_die(Env::file_str("/communities.txt"), "communities");
  const std::vector<uint32_t> &s2i = network_.seq2id();
  std::vector<uint32_t> groups(n_, 0);
  for (uint32_t i = 0; i < n_; ++i) {
    const double *g = &gamma_[(size_t)i * k_];
    double s = 0;
    for (uint32_t k = 0; k < k_; ++k) s += g[k];
    fprintf(groupsf, "%d\t%d\t", i, s2i[i]);
    double max = .0;
    for (uint32_t j = 0; j < k_; ++j) {
      const double pi = g[j] / s;
      fprintf(groupsf, "%.3f\t", pi);
      if (pi > max) { max = pi; groups[i] = j; }
    }
    fprintf(groupsf, "%d\n", groups[i]);
  }
  std::vector<int> sizes(k_, 0);
  std::map<uint32_t, std::vector<uint32_t> > comm;
  for (uint32_t i = 0; i < n_; ++i) {
    sizes[groups[i]]++;
    comm[groups[i]].push_back(i);
  }
  for (uint32_t k = 0; k < k_; ++k) fprintf(summaryf, "%d\t", sizes[k]);
  fprintf(summaryf, "\n");
  for (const auto &c : comm) {
    fprintf(commf, "%d\t", c.first);
    for (uint32_t p : c.second) fprintf(commf, "%d ", p);
    fprintf(commf, "\n");
  }
  fclose(groupsf);
  fclose(summaryf);
  fclose(commf);
}

void MMSBInferOrig::save_model() {
  FILE *gf = open_or_die(Env::file_str("/gamma.txt"), "gamma");
  const std::vector<uint32_t> &s2i = network_.seq2id();
  for (uint32_t i = 0; i < n_; ++i) {
    fprintf(gf, "%d\t%d\t", i, s2i[i]);
    for (uint32_t k = 0; k < k_; ++k) fprintf(gf, k == k_ - 1 ? "%.5f\n" : "%.5f\t", gamma_[(size_t)i * k_ + k]);
  }
  fclose(gf);
  FILE *bf = open_or_die(Env::file_str("/beta.txt"), "beta");   // K lines of K values; 12 digits: the rates span many decades
  for (uint32_t g = 0; g < k_; ++g)
    for (uint32_t h = 0; h < k_; ++h) fprintf(bf, h == k_ - 1 ? "%.12g\n" : "%.12g\t", beta_[(size_t)g * k_ + h]);
  fclose(bf);
}

}  // namespace svinet
