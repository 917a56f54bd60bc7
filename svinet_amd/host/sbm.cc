#include "sbm.hh"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "util.hh"

namespace svinet {

namespace {

const uint32_t kMaxEstepPasses = 10;   // src/sbm.cc:470
const double kEstepThresh = 0.01;      // src/sbm.cc:481

// psi(x), x > 0: the recurrence up to x >= 10, then the asymptotic series with seven terms (error < 4e-17 there).  The
// E-step adds n - 1 multiples of Elogbeta, so the host loops take a psi as accurate as the device's
double psi(double x) {
  double r = 0;
  while (x < 10) { r -= 1 / x; x += 1; }
  const double f = 1 / (x * x);
  return r + std::log(x) - 0.5 / x -
         f * (1.0 / 12 - f * (1.0 / 120 - f * (1.0 / 252 - f * (1.0 / 240 - f * (1.0 / 132 - f * (691.0 / 32760 - f * (1.0 / 12)))))));
}

Edge ordered(uint32_t a, uint32_t b) { return a < b ? Edge(a, b) : Edge(b, a); }

}  // namespace

SBM::SBM(Env &env, Network &network)
    : env_(env), network_(network), n_(env.n), k_(env.k), rng_((unsigned long)env.seed), gamma_rng_(rng_),
      phi_((size_t)n_ * k_), gamma_(k_), lambda_(2 * ((size_t)k_ + 1)), eta_(2 * ((size_t)k_ + 1)), elogpi_(k_),
      elogbeta_(2 * ((size_t)k_ + 1)), start_time_(time(0)) {
  fprintf(stdout, "+ sbm initialization begin\n");
  fflush(stdout);
  Env::plog("inference n", n_);
  Env::plog("total pairs", (uint64_t)n_ * (n_ - 1) / 2);
  for (uint32_t k = 0; k < k_; ++k) {   // src/sbm.cc:50-56
    eta_[2 * k] = env.eta0;
    eta_[2 * k + 1] = env.eta1;
  }
  eta_[2 * k_] = 0.0001;
  eta_[2 * k_ + 1] = 1.0;
  init_heldout();
  skipped_.resize(n_);
  for (const SampleMap *m : {&heldout_map_, &validation_map_, &precision_map_})
    for (const auto &it : *m) {
      skipped_[it.first.first].push_back(it.first.second);
      skipped_[it.first.second].push_back(it.first.first);
    }
  printf("+ done heldout\n");
  init_state();
  printf("+ done initializing gamma, lambda\n");
  set_elog();
  printf("+ done Elogpi and Elogbeta\n");
  if (env_.single_device) attach_device();
  if (env_.write_files) {
    // files the reference's constructor opens (:97-139); the ones this path never writes stay empty
    for (const char *f : {"/time.txt", "/convergence.txt", "/precision.txt", "/logl.txt", "/modularity.txt"})
      fclose(open_or_die(Env::file_str(f), f + 1));
    hf_ = open_or_die(Env::file_str("/heldout.txt"), "heldout");
    vf_ = open_or_die(Env::file_str("/validation.txt"), "validation");
    if (env_.single_logl) lf_ = open_or_die(Env::file_str("/logl.txt"), "logl");
  }
  rule_.enabled = env_.use_validation_stop;
  Env::plog("network ones", network_.ones());
  Env::plog("network singles", network_.singles());
  printf("+ sbm initialization end\n");
  likelihood_row(heldout_map_, hf_, 0);      // :148-149
  likelihood_row(validation_map_, vf_, 1);
  fflush(stdout);
  start_time_ = time(0);
}

SBM::~SBM() {
  if (hf_) fclose(hf_);
  if (vf_) fclose(vf_);
  if (lf_) fclose(lf_);
  if (dev_) svils_sbm_destroy(dev_);
}

// ---------------------------------------------------------------------------
// the device backend (include/svils.h: svils_sbm_*)
// ---------------------------------------------------------------------------
void SBM::attach_device() {
  if (int rc = svils_sbm_create(env_.device, n_, k_, env_.sbm_alpha, eta_.data(), &dev_)) throw_svils("svils_sbm_create", rc);
  std::vector<uint32_t> l, s;
  for (const Edge &e : network_.edges()) {
    l.push_back(std::min(e.first, e.second));
    l.push_back(std::max(e.first, e.second));
  }
  for (const SampleMap *m : {&heldout_map_, &validation_map_, &precision_map_})
    for (const auto &it : *m) { s.push_back(it.first.first); s.push_back(it.first.second); }
  if (int rc = svils_sbm_set_graph(dev_, l.data(), l.size() / 2, s.data(), s.size() / 2)) throw_svils("svils_sbm_set_graph", rc);
  if (int rc = svils_sbm_set_state(dev_, phi_.data(), gamma_.data(), lambda_.data())) throw_svils("svils_sbm_set_state", rc);
}

void SBM::fetch_state() {
  if (!dev_ || !host_stale_) return;
  if (int rc = svils_sbm_get_state(dev_, phi_.data(), gamma_.data(), lambda_.data())) throw_svils("svils_sbm_get_state", rc);
  host_stale_ = false;
}

void SBM::set_state(const double *phi, const double *gamma, const double *lambda) {
  if (dev_) {
    if (int rc = svils_sbm_set_state(dev_, phi, gamma, lambda)) throw_svils("svils_sbm_set_state", rc);
    host_stale_ = false;
  }
  phi_.assign(phi, phi + phi_.size());
  gamma_.assign(gamma, gamma + gamma_.size());
  lambda_.assign(lambda, lambda + lambda_.size());
  set_elog();
}

// ---------------------------------------------------------------------------
// the three samples (:163-295, src/sbm.hh:310-350)
// ---------------------------------------------------------------------------
bool SBM::edge_ok(const Edge &e) const {
  return e.first != e.second && !heldout_map_.count(e) && !validation_map_.count(e) && !precision_map_.count(e);
}

// get_random_edge: a uniform pair of nodes, or a uniform link, that no sample holds yet
Edge SBM::random_edge(bool link) {
  Edge e;
  do {
    if (link) {
      const Edge &l = network_.edges()[rng_.uniform_int(network_.ones())];
      e = ordered(l.first, l.second);
    } else {
      const uint32_t a = rng_.uniform_int(n_), b = rng_.uniform_int(n_);
      e = ordered(a, b);
    }
  } while (!edge_ok(e));
  return e;
}

// `zeros` non-links and `ones` links: uniform pairs until the non-links are full (a link drawn meanwhile is taken while
// links are wanted), then uniform links
void SBM::set_sample(uint32_t zeros, uint32_t ones, SampleMap &map, std::vector<uint32_t> &list) {
  uint32_t c0 = 0, c1 = 0;
  while (c0 < zeros || c1 < ones) {
    const Edge e = random_edge(c0 == zeros);
    const bool y = network_.y(e.first, e.second);
    if ((!y && c0 < zeros) || (y && c1 < ones)) {
      (y ? c1 : c0)++;
      list.push_back(e.first);
      list.push_back(e.second);
      map[e] = true;
    }
  }
}

void SBM::init_heldout() {
  const uint32_t p = (uint32_t)((int)(env_.heldout_ratio * network_.ones()) / 2);
  const uint32_t prec1 = n_ > 100000 ? 1000 : 10, prec0 = n_ > 100000 ? 1000000 : 100;   // src/sbm.hh:369-379
  const uint64_t pairs = (uint64_t)n_ * (n_ - 1) / 2, need1 = 2 * (uint64_t)p + prec1, need0 = 2 * (uint64_t)p + prec0;
  if (network_.ones() < need1 || pairs - network_.ones() < need0) {   // the reference would draw for ever
    fprintf(stderr, "error: -single needs %llu links and %llu non-links for its held-out, validation and precision samples; the graph has "
                    "%u and %llu\n", (unsigned long long)need1, (unsigned long long)need0, network_.ones(),
            (unsigned long long)(pairs - network_.ones()));
    exit(-1);
  }
  set_sample(p, p, heldout_map_, heldout_pairs_);
  set_sample(p, p, validation_map_, validation_pairs_);
  set_sample(prec0, prec1, precision_map_, precision_pairs_);
  Env::plog("heldout ratio", env_.heldout_ratio);
  Env::plog("heldout pairs (1s and 0s)", (uint32_t)heldout_map_.size());
  Env::plog("precision links", prec1);
  Env::plog("precision nonlinks", prec0);
  Env::plog("precision pairs (1s and 0s)", (uint32_t)precision_map_.size());
  if (!env_.write_files) return;
  for (int which = 0; which < 2; ++which) {   // edgelist_s (:187-196): sequence ids, an empty line at the end
    const std::vector<uint32_t> &list = which ? validation_pairs_ : heldout_pairs_;
    FILE *f = open_or_die(Env::file_str(which ? "/validation-pairs.txt" : "/heldout-pairs.txt"), which ? "validation edges" : "heldout edges");
    for (size_t i = 0; i + 1 < list.size(); i += 2) fprintf(f, "%d\t%d\n", list[i], list[i + 1]);
    fprintf(f, "\n");
    fclose(f);
  }
}

// ---------------------------------------------------------------------------
// starts (:341-385): gamma, lambda, phi, in this order
// ---------------------------------------------------------------------------
void SBM::init_state() {
  const double v = 100.0 / k_, vl = k_ <= 100 ? 1.0 : 100.0 / k_;
  for (uint32_t k = 0; k < k_; ++k) gamma_[k] = gamma_rng_.gamma(100 * v, 0.01);
  for (size_t x = 0; x < lambda_.size(); ++x) lambda_[x] = gamma_rng_.gamma(100 * vl, 0.01);
  for (uint32_t i = 0; i < n_; ++i) {
    double *row = &phi_[(size_t)i * k_], s = 0;
    for (uint32_t k = 0; k < k_; ++k) s += row[k] = gamma_rng_.gamma(v * 100, 0.01);
    for (uint32_t k = 0; k < k_; ++k) row[k] /= s;
  }
}

// set_dir_exp (src/sbm.hh:177-207) of gamma and of the rows of lambda
void SBM::set_elog() {
  double sg = 0;
  for (uint32_t k = 0; k < k_; ++k) sg += gamma_[k];
  const double pg = psi(sg);
  for (uint32_t k = 0; k < k_; ++k) elogpi_[k] = psi(gamma_[k]) - pg;
  for (uint32_t k = 0; k <= k_; ++k) {
    const double ps = psi(lambda_[2 * k] + lambda_[2 * k + 1]);
    elogbeta_[2 * k] = psi(lambda_[2 * k]) - ps;
    elogbeta_[2 * k + 1] = psi(lambda_[2 * k + 1]) - ps;
  }
}

// ---------------------------------------------------------------------------
// one iteration on the host (:465-525): the reference's loops over all pairs
// ---------------------------------------------------------------------------
void SBM::estep_host() {
  const uint32_t K = k_;
  std::vector<double> a(K);
  std::vector<uint32_t> qs;
  std::vector<uint8_t> yv((size_t)n_), ok((size_t)n_), yq((size_t)n_);
  msums_.clear();
  passes_ = 0;
  for (uint32_t itr = 0; itr < kMaxEstepPasses; ++itr) {
    double msum = 0;
    for (uint32_t p = 0; p < n_; ++p) {
      uint32_t m = 0;   // the trained partners of p and their y (edge_ok and get_y, from the rows of p instead of per pair)
      qs.clear();
      std::fill(yv.begin(), yv.end(), 0);
      std::fill(ok.begin(), ok.end(), 1);
      ok[p] = 0;
      for (uint32_t q : skipped_[p]) ok[q] = 0;
      for (uint32_t q : network_.get_edges(p)) yv[q] = 1;
      for (uint32_t q = 0; q < n_; ++q)
        if (ok[q]) {
          qs.push_back(q);
          yq[m++] = yv[q];
        }
      // batch_update_phi (:414-435) with update_phi_helper (:437-454): every a[k] takes its partners in ascending order
      for (uint32_t k = 0; k < K; ++k) a[k] = elogpi_[k];
      for (uint32_t x = 0; x < m; ++x) {
        const double *pq = &phi_[(size_t)qs[x] * K];
        const int t = yq[x] ? 0 : 1;
        for (uint32_t k = 0; k < K; ++k) {
          a[k] += (1 - pq[k]) * elogbeta_[2 * K + t];
          a[k] += pq[k] * elogbeta_[2 * k + t];
        }
      }
      double mx = a[0];                    // lognormalize: exp(a - logsumexp a)
      for (uint32_t k = 1; k < K; ++k) mx = std::max(mx, a[k]);
      double s = 0;
      for (uint32_t k = 0; k < K; ++k) s += exp(a[k] - mx);
      const double lse = mx + log(s);
      double *row = &phi_[(size_t)p * K];
      for (uint32_t k = 0; k < K; ++k) {
        const double nw = exp(a[k] - lse);
        msum += fabs(row[k] - nw);
        row[k] = nw;
      }
    }
    msums_.push_back(msum);
    passes_++;
    if (msum < kEstepThresh) break;
  }
}

void SBM::mstep_host() {
  const uint32_t K = k_;
  for (uint32_t k = 0; k < K; ++k) {
    double s = 0;
    for (uint32_t i = 0; i < n_; ++i) s += phi_[(size_t)i * K + k];
    gamma_[k] = env_.sbm_alpha + s;
  }
  std::vector<double> sa(K + 1, 0.0), sb(K + 1, 0.0);
  std::vector<uint8_t> yv((size_t)n_), ok((size_t)n_);
  for (uint32_t i = 0; i < n_; ++i) {
    std::fill(yv.begin(), yv.end(), 0);
    std::fill(ok.begin(), ok.end(), 1);
    for (uint32_t q : skipped_[i]) ok[q] = 0;
    for (uint32_t q : network_.get_edges(i)) yv[q] = 1;
    for (uint32_t j = i + 1; j < n_; ++j) {
      if (!ok[j]) continue;
      const bool y = yv[j] != 0;
      const double *pi = &phi_[(size_t)i * K], *pj = &phi_[(size_t)j * K];
      for (uint32_t k = 0; k < K; ++k) {
        const double v = pi[k] * pj[k];
        (y ? sa : sb)[k] += v;
        (y ? sa : sb)[K] += 1 - v;           // summed over k (:512-515)
      }
    }
  }
  for (uint32_t k = 0; k <= K; ++k) {
    lambda_[2 * k] = eta_[2 * k] + sa[k];
    lambda_[2 * k + 1] = eta_[2 * k + 1] + sb[k];
  }
  set_elog();
}

void SBM::sweep() {
  if (dev_) {
    if (int rc = svils_sbm_sweep(dev_, 1)) throw_svils("svils_sbm_sweep", rc);
    double ms[SVILS_SBM_MAX_PASSES];
    if (int rc = svils_sbm_get_stats(dev_, &passes_, nullptr, ms)) throw_svils("svils_sbm_get_stats", rc);
    msums_.assign(ms, ms + passes_);
    host_stale_ = true;
  } else {
    estep_host();
    mstep_host();
  }
  const OrigStopRule::Verdict v = env_.single_logl ? approx_log_likelihood() : OrigStopRule::GO_ON;   // :528-530
  likelihood_row(heldout_map_, hf_, 0);       // :532-534
  likelihood_row(validation_map_, vf_, 1);
  if (v != OrigStopRule::GO_ON) {             // a rule ends the run (:914-936, :1222-1225)
    const SbmPrecision pr = compute_precision();
    const double s = logl_rows_.back();
    if (env_.write_files && v == OrigStopRule::STOP_DROP) {
      FILE *f = open_or_die(Env::file_str("/max.txt"), "max");   // a, t, v, max: the bound, 0, the validation mean, its maximum
      fprintf(f, "%d\t%d\t%.5f\t%.5f\t%.5f\t%.5f\t%d\t%d\t%d\t%d\n", iter_, duration(), s, 0.0, rows_[rows_.size() - 6], rule_.max, pr.c10,
              pr.c100, pr.c1000, 1);
      fclose(f);
    } else if (env_.write_files) {
      FILE *f = open_or_die(Env::file_str("/done.txt"), "done");
      fprintf(f, "%d\t%d\t%.5f\n", iter_, duration(), s);
      fclose(f);
    }
  }
  iter_++;
}

// ---------------------------------------------------------------------------
// the lower bound (:1133-1239) and its stop rules
// ---------------------------------------------------------------------------
void SBM::elbo_host(double out[4]) {
  const uint32_t K = k_;
  auto beta_term = [&](const std::vector<double> &p, uint32_t k) {   // :1144-1164
    return lgamma(p[2 * k] + p[2 * k + 1]) - (lgamma(p[2 * k]) + lgamma(p[2 * k + 1])) +
           ((p[2 * k] - 1) * elogbeta_[2 * k] + (p[2 * k + 1] - 1) * elogbeta_[2 * k + 1]);
  };
  double G = 0;
  for (uint32_t k = 0; k <= K; ++k) G += beta_term(eta_, k) - beta_term(lambda_, k);
  double P = 0;                                                      // :1166-1185
  std::vector<uint8_t> yv((size_t)n_), ok((size_t)n_);
  for (uint32_t p = 0; p < n_; ++p) {
    std::fill(yv.begin(), yv.end(), 0);
    std::fill(ok.begin(), ok.end(), 1);
    for (uint32_t q : skipped_[p]) ok[q] = 0;
    for (uint32_t q : network_.get_edges(p)) yv[q] = 1;
    const double *pp = &phi_[(size_t)p * K];
    for (uint32_t q = p + 1; q < n_; ++q) {
      if (!ok[q]) continue;
      const int t = yv[q] ? 0 : 1;
      const double *pq = &phi_[(size_t)q * K];
      double sum = 0;
      for (uint32_t k = 0; k < K; ++k) {
        sum += pp[k] * pq[k];
        P += pp[k] * pq[k] * elogbeta_[2 * k + t];
      }
      P += (1 - sum) * elogbeta_[2 * K + t];
    }
  }
  double N = 0;                                                      // :1187-1191 (an exact 0 adds 0)
  for (uint32_t i = 0; i < n_; ++i)
    for (uint32_t k = 0; k < K; ++k) {
      const double x = phi_[(size_t)i * K + k];
      if (x > 0) N += x * (elogpi_[k] - log(x));
    }
  double se = 0, sg = 0, slg = 0, sge = 0;                           // :1193-1213
  for (uint32_t k = 0; k < K; ++k) {
    se += elogpi_[k];
    sg += gamma_[k];
    slg += lgamma(gamma_[k] < 1e-30 ? 1e-30 : gamma_[k]);
    sge += (gamma_[k] - 1) * elogpi_[k];
  }
  G += lgamma(K * env_.sbm_alpha) - K * lgamma(env_.sbm_alpha) + (env_.sbm_alpha - 1) * se;
  G -= lgamma(sg) - slg;
  G -= sge;
  out[0] = (P + N) + G;
  out[1] = P;
  out[2] = N;
  out[3] = G;
}

void SBM::elbo(double out[4]) {
  if (dev_) {
    if (int rc = svils_sbmelbo(dev_, out)) throw_svils("svils_sbmelbo", rc);
  } else {
    elbo_host(out);
  }
}

OrigStopRule::Verdict SBM::approx_log_likelihood() {
  double o[4];
  elbo(o);
  const double s = o[0];
  printf("approx. log likelihood = %f\n", s);
  if (lf_) {
    fprintf(lf_, "%d\t%d\t%.5f\n", iter_, duration(), s);   // :1216
    fflush(lf_);
  }
  logl_rows_.push_back((double)iter_);
  logl_rows_.push_back(s);
  return verdict_ = rule_.update(iter_, s);
}

// ---------------------------------------------------------------------------
// compute_precision (:991-1060)
// ---------------------------------------------------------------------------
SbmPrecision sbm_rank_precision(const uint32_t *pairs, const double *score, const uint8_t *y, size_t m) {
  std::vector<size_t> order(m);
  for (size_t i = 0; i < m; ++i) order[i] = i;
  std::sort(order.begin(), order.end(), [&](size_t a, size_t b) {
    if (score[a] != score[b]) return score[a] > score[b];
    if (pairs[2 * a] != pairs[2 * b]) return pairs[2 * a] < pairs[2 * b];
    return pairs[2 * a + 1] < pairs[2 * b + 1];
  });
  SbmPrecision r;
  uint32_t hits = 0;
  for (size_t i = 0; i < m; ++i) {
    if (y[order[i]]) {
      hits++;
      if (i < 10) r.c10++;
      else if (i < 100) r.c100++;
      else if (i < 1000) r.c1000++;
    }
    if (i == 0 || (i + 1) % 1000 == 0) {
      r.curve.push_back((uint32_t)(i + 1));
      r.curve.push_back(hits);
    }
  }
  r.c100 += r.c10;
  r.c1000 += r.c100;
  return r;
}

SbmPrecision SBM::compute_precision() {
  const size_t m = precision_map_.size();
  std::vector<uint32_t> pq;
  std::vector<uint8_t> y, ones(m, 1);
  std::vector<double> u(m);
  for (const auto &it : precision_map_) {
    pq.push_back(it.first.first);
    pq.push_back(it.first.second);
    y.push_back(network_.y(it.first.first, it.first.second) ? 1 : 0);
  }
  if (dev_) {
    if (int rc = svils_sbm_pair_loglik(dev_, pq.data(), ones.data(), m, u.data())) throw_svils("svils_sbm_pair_loglik", rc);
  } else {
    for (size_t i = 0; i < m; ++i) u[i] = edge_likelihood2(pq[2 * i], pq[2 * i + 1], 1);
  }
  const SbmPrecision r = sbm_rank_precision(pq.data(), u.data(), y.data(), m);
  if (env_.write_files) {
    char buf[64];
    snprintf(buf, sizeof buf, "/hitcurve_%u.txt", hitcurve_id_++);
    FILE *hc = open_or_die(Env::file_str(buf), "hitcurve");
    for (size_t i = 0; i + 1 < r.curve.size(); i += 2) fprintf(hc, "%d\t%d\n", r.curve[i], r.curve[i + 1]);
    fclose(hc);
    FILE *pf = fopen(Env::file_str("/precision.txt").c_str(), "a");   // opened (and emptied) by the constructor
    if (!pf) {
      fprintf(stderr, "cannot open precision file\n");
      exit(-1);
    }
    fprintf(pf, "%d\t%d\t%d\t%d\t%d\n", iter_, duration(), r.c10, r.c100, r.c1000);
    fclose(pf);
  }
  return r;
}

// ---------------------------------------------------------------------------
// likelihoods (src/sbm.hh:284-308, src/sbm.cc:843-988)
// ---------------------------------------------------------------------------
double SBM::edge_likelihood2(uint32_t p, uint32_t q, int y) const {
  const uint32_t K = k_;
  const double *pp = &phi_[(size_t)p * K], *pq = &phi_[(size_t)q * K];
  double s = 0, sum = 0;
  for (uint32_t k = 0; k < K; ++k) {
    const double r = lambda_[2 * k] / (lambda_[2 * k] + lambda_[2 * k + 1]);
    s += pp[k] * pq[k] * (y ? r : 1 - r);
    sum += pp[k] * pq[k];
  }
  const double rK = lambda_[2 * K] / (lambda_[2 * K] + lambda_[2 * K + 1]);
  s += (1 - sum) * (y ? rK : 1 - rK);
  if (s < 1e-30) s = 1e-30;
  return log(s);
}

void SBM::likelihood_row(const SampleMap &pairs, FILE *f, int which) {
  std::vector<double> u(pairs.size());
  std::vector<uint32_t> pq;
  std::vector<uint8_t> y;
  for (const auto &it : pairs) {
    pq.push_back(it.first.first);
    pq.push_back(it.first.second);
    y.push_back(network_.y(it.first.first, it.first.second) ? 1 : 0);
  }
  if (dev_) {
    if (int rc = svils_sbm_pair_loglik(dev_, pq.data(), y.data(), pairs.size(), u.data())) throw_svils("svils_sbm_pair_loglik", rc);
  } else {
    for (size_t i = 0; i < u.size(); ++i) u[i] = edge_likelihood2(pq[2 * i], pq[2 * i + 1], y[i]);
  }
  uint32_t k = 0, kzeros = 0, kones = 0;                      // summed in the map's order
  double s = .0, szeros = 0, sones = 0;
  for (size_t i = 0; i < u.size(); ++i) {
    s += u[i];
    k += 1;
    if (y[i]) { sones += u[i]; kones++; } else { szeros += u[i]; kzeros++; }
  }
  const double zeros_prob = 0, ones_prob = 0;                 // never set by the reference's SBM: the weighted columns are 0
  if (f) {
    fprintf(f, "%d\t%d\t%.9f\t%d\t%.9f\t%d\t%.9f\t%d\t%.9f\t%.9f\t%.9f\n", iter_, duration(), s / k, k, szeros / kzeros, kzeros,
            sones / kones, kones, zeros_prob * (szeros / kzeros), ones_prob * (sones / kones),
            zeros_prob * (szeros / kzeros) + ones_prob * (sones / kones));
    fflush(f);
  }
  const double row[8] = {(double)which, (double)iter_, s / k, (double)k, szeros / kzeros, (double)kzeros, sones / kones, (double)kones};
  rows_.insert(rows_.end(), row, row + 8);
}

int SBM::batch_infer() {
  printf("Running batch inference\n");
  const bool open_end = env_.max_iterations == 0 && env_.single_logl && rule_.enabled;   // a stop rule ends the run
  while ((open_end || iter_ < env_.max_iterations) && !env_.terminate && verdict_ == OrigStopRule::GO_ON) {
    sweep();
    printf("iteration = %d took %d secs (%u E-step passes)\n", iter_, duration(), passes_);
    fflush(stdout);
  }
  if (env_.single_logl && verdict_ == OrigStopRule::GO_ON) compute_precision();   // the run ended at -max-iterations
  fetch_state();
  if (env_.write_files) save_model();
  return 0;
}

// ---------------------------------------------------------------------------
// save_model (:297-338)
// ---------------------------------------------------------------------------
void SBM::save_model() {
  FILE *pf = open_or_die(Env::file_str("/phi.txt"), "phi");
  const std::vector<uint32_t> &s2i = network_.seq2id();
  for (uint32_t i = 0; i < n_; ++i) {
    fprintf(pf, "%d\t%d\t", i, s2i[i]);
    for (uint32_t k = 0; k < k_; ++k) fprintf(pf, k == k_ - 1 ? "%.5f\n" : "%.5f\t", phi_[(size_t)i * k_ + k]);
  }
  fclose(pf);
  FILE *lf = open_or_die(Env::file_str("/lambda.txt"), "lambda");
  for (uint32_t k = 0; k <= k_; ++k) fprintf(lf, "%d\t%.5f\t%.5f\n", k, lambda_[2 * k], lambda_[2 * k + 1]);
  fclose(lf);
  FILE *gf = open_or_die(Env::file_str("/gamma.txt"), "gamma");
  for (uint32_t k = 0; k < k_; ++k) fprintf(gf, "%d\t%.5f\n", k, gamma_[k]);
  fclose(gf);
}

}  // namespace svinet
