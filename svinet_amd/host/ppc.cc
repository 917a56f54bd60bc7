// ppc.cc -- -ppc / -gen (src/mmsbgen.cc:43-71, 152-179, 286-362, 632-697, 730-742, 784-838).  See ppc.hh.
#include "ppc.hh"

#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "lcstats.hh"
#include "svils.h"
#include "util.hh"

namespace svinet {

void philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
  uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c0 = n0;
    c1 = (uint32_t)p1;
    c2 = n2;
    c3 = (uint32_t)p0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0;
  out[1] = c1;
  out[2] = c2;
  out[3] = c3;
}

namespace {

double to_uniform(uint32_t w0, uint32_t w1) { return (double)(((uint64_t)(w0 >> 5) << 26) | (uint64_t)(w1 >> 6)) * 0x1p-53; }

// the two uniforms of a block
void uniform_pair(uint32_t seed, uint32_t r, uint32_t a, uint32_t b, uint32_t stream, uint32_t block, double *u, double *v) {
  const uint32_t ctr[4] = {a, b, stream, block}, key[2] = {seed, r};
  uint32_t w[4];
  philox4x32_10(ctr, key, w);
  *u = to_uniform(w[0], w[1]);
  *v = to_uniform(w[2], w[3]);
}

}  // namespace

double gamma_variate(double shape, uint32_t seed, uint32_t r, uint32_t a, uint32_t b, uint32_t stream) {
  const double a1 = shape < 1.0 ? shape + 1.0 : shape;
  const double d = a1 - 1.0 / 3.0, c = 1.0 / std::sqrt(9.0 * d);
  double v;
  for (uint32_t t = 0;; ++t) {
    double u1, u2, u3, unused;
    uniform_pair(seed, r, a, b, stream, 2 * t, &u1, &u2);
    uniform_pair(seed, r, a, b, stream, 2 * t + 1, &u3, &unused);
    const double z = std::sqrt(-2.0 * std::log(1.0 - u1)) * std::cos(2.0 * M_PI * u2);
    v = 1.0 + c * z;
    if (v <= 0.0) continue;
    v = v * v * v;
    if (std::log(1.0 - u3) < 0.5 * z * z + d - d * v + d * std::log(v)) break;
  }
  double g = d * v;
  if (shape < 1.0) {
    double ub, unused;
    uniform_pair(seed, r, a, b, stream, 0xffffffffu, &ub, &unused);
    g *= std::pow(1.0 - ub, 1.0 / shape);
  }
  return g;
}

void dirichlet_rows(const double *gam, uint32_t n, uint32_t k, uint32_t seed, uint32_t r, double *pi) {
  for (uint32_t i = 0; i < n; ++i) {
    double *row = pi + (size_t)i * k;
    double s = 0.0;
    for (uint32_t j = 0; j < k; ++j) {
      row[j] = gamma_variate(gam[(size_t)i * k + j], seed, r, i, j, kPpcStreamPi);
      s += row[j];
    }
    for (uint32_t j = 0; j < k; ++j) row[j] = s > 0.0 ? row[j] / s : 1.0 / (double)k;
  }
}

void beta_draws(const double *lam, uint32_t k, uint32_t seed, uint32_t r, double *beta) {
  for (uint32_t j = 0; j < k; ++j) {
    const double g0 = gamma_variate(lam[2 * j], seed, r, j, 0, kPpcStreamBeta), g1 = gamma_variate(lam[2 * j + 1], seed, r, j, 1, kPpcStreamBeta);
    beta[j] = g0 / (g0 + g1);
  }
}

namespace {

// "%.5f" (digits = 5) of the reference's files, with one spelling of NaN whatever its sign
std::string fx(double x, int digits = 5) {
  if (std::isnan(x)) return "nan";
  char buf[64];
  snprintf(buf, sizeof buf, "%.*f", digits, x);
  return buf;
}

struct Scalars {
  uint64_t ones, maxdeg, triangles;
  double density, avgdeg, transitivity, clustering;
  double offdiag = NAN;   // -ppc-orig: joined links in blocks g != h / joined links
  std::vector<uint64_t> size;   // per community, or per block [k][k] (-ppc-orig)
  std::vector<double> logpe;
};

// mean and sample deviation in replicate order, z of obs (NaN where the deviation is 0) and the two-sided posterior
// predictive p-value min(1, 2 min(#{x >= obs}, #{x <= obs}) / R)
struct Moments {
  double mean = 0, sd = 0, z = NAN, p = NAN;
  Moments(const std::vector<double> &x, double obs) {
    const size_t R = x.size();
    if (!R) return;
    double s = 0;
    for (double v : x) s += v;
    mean = s / (double)R;
    double q = 0;
    for (double v : x) q += (v - mean) * (v - mean);
    sd = R > 1 ? std::sqrt(q / (double)(R - 1)) : 0.0;
    if (sd > 0) z = (obs - mean) / sd;
    size_t ge = 0, le = 0;
    for (double v : x) {
      ge += v >= obs;
      le += v <= obs;
    }
    p = std::min(1.0, 2.0 * (double)std::min(ge, le) / (double)R);
  }
};

// -ppc-hops: what svils_ppc_hops says of one list
struct Hops {
  double effdiam, meandist;
  uint64_t diameter, components, largest, isolated;
  std::vector<uint64_t> D;
};

// a row of summary.txt / hops-summary.txt: statistic, observed, replicate mean, deviation, two-sided posterior predictive p-value
std::string summary_row(const char *name, double obs, const std::vector<double> &x, int digits) {
  const Moments m(x, obs);
  return std::string(name) + "\t" + fx(obs, digits) + "\t" + fx(m.mean, digits) + "\t" + fx(m.sd, digits) + "\t" + fx(m.p) + "\n";
}

struct Handle {
  svils_ppc *h = nullptr;
  uint32_t n, k;
  bool blocks = false;   // the K x K kind is current
  Handle(int device, uint32_t n_, uint32_t k_, uint64_t cap) : n(n_), k(k_) {
    if (int rc = svils_ppc_create(device, n, k, cap, &h)) throw_svils("svils_ppc_create", rc);
  }
  ~Handle() { svils_ppc_destroy(h); }
  void params(const double *pi, const double *beta) {
    if (int rc = svils_ppc_set_params(h, pi, beta)) throw_svils("svils_ppc_set_params", rc);
    blocks = false;
  }
  void params_orig(const double *pi, const double *B) {
    if (int rc = svils_ppc_set_params_orig(h, pi, B)) throw_svils("svils_ppc_set_params_orig", rc);
    blocks = true;
  }
  Scalars stats() {
    if (int rc = svils_ppc_stats(h)) throw_svils("svils_ppc_stats", rc);
    uint64_t c[5];
    double v[2];
    Scalars s;
    s.size.resize(blocks ? (size_t)k * k : k);
    s.logpe.resize(s.size.size());
    if (int rc = svils_ppc_get_summary(h, c, v)) throw_svils("svils_ppc_get_summary", rc);
    if (blocks) {
      if (int rc = svils_ppc_get_blocks(h, s.size.data(), s.logpe.data())) throw_svils("svils_ppc_get_blocks", rc);
      uint64_t joined = 0, diag = 0;
      for (size_t t = 0; t < s.size.size(); ++t) {
        joined += s.size[t];
        if (t / k == t % k) diag += s.size[t];
      }
      if (joined) s.offdiag = (double)(joined - diag) / (double)joined;
    } else if (int rc = svils_ppc_get_communities(h, s.size.data(), s.logpe.data())) {
      throw_svils("svils_ppc_get_communities", rc);
    }
    s.ones = c[0];
    s.maxdeg = c[1];
    s.triangles = c[3];
    s.density = (double)c[0] / ((double)n * (n - 1) / 2.0);
    s.avgdeg = (double)(2 * c[0]) / (double)n;
    s.transitivity = v[0];
    s.clustering = v[1];
    return s;
  }
  Hops hops() {
    if (int rc = svils_ppc_hops(h)) throw_svils("svils_ppc_hops", rc);
    uint64_t c[6];
    double v[2];
    if (int rc = svils_ppc_get_hop_summary(h, c, v)) throw_svils("svils_ppc_get_hop_summary", rc);
    Hops s{v[0], v[1], c[1], c[2], c[3], c[4], std::vector<uint64_t>(c[5])};
    uint32_t levels = 0;
    if (int rc = svils_ppc_get_hops(h, &levels, s.D.data(), (uint32_t)s.D.size())) throw_svils("svils_ppc_get_hops", rc);
    return s;
  }
  std::vector<uint32_t> links() {
    uint64_t m = 0;
    if (int rc = svils_ppc_get_links(h, &m, nullptr, nullptr, nullptr)) throw_svils("svils_ppc_get_links", rc);
    std::vector<uint32_t> l(2 * m);
    if (int rc = svils_ppc_get_links(h, &m, l.data(), nullptr, nullptr)) throw_svils("svils_ppc_get_links", rc);
    return l;
  }
};

std::string row_of(const Scalars &s) {
  return std::to_string(s.ones) + "\t" + fx(s.density, 8) + "\t" + fx(s.avgdeg) + "\t" + std::to_string(s.maxdeg) + "\t" +
         std::to_string(s.triangles) + "\t" + fx(s.transitivity) + "\t" + fx(s.clustering) + "\n";
}

void write_file(const std::string &path, const std::string &text) {
  FILE *f = open_or_die(path, path.c_str());
  fwrite(text.data(), 1, text.size(), f);
  fclose(f);
}

void write_links(const std::string &path, const std::vector<uint32_t> &l) {   // draw_and_save (:686-695): sequence ids
  std::string t;
  for (size_t x = 0; x + 1 < l.size(); x += 2) t += std::to_string(l[x]) + "\t" + std::to_string(l[x + 1]) + "\n";
  write_file(path, t);
}

void make_dir(const std::string &d) { mkdir(d.c_str(), S_IRWXU | S_IRWXG | S_IROTH | S_IXOTH); }

// the list has room for eight times the observed links (and for 2^16): a fitted model draws about as many as it saw
uint64_t list_room(uint64_t observed) { return std::max<uint64_t>(8 * observed, 1u << 16); }

}  // namespace

int read_block_rates(const std::string &path, uint32_t k, double *B) {
  FILE *f = fopen(path.c_str(), "r");
  if (!f) {
    fprintf(stderr, "error: cannot open %s: %s\n", path.c_str(), strerror(errno));
    return -1;
  }
  std::string text;
  char buf[1 << 16];
  for (size_t m; (m = fread(buf, 1, sizeof buf, f)) > 0;) text.append(buf, m);
  fclose(f);
  uint32_t line = 0;
  for (size_t b = 0; b < text.size(); ++line) {
    size_t e = text.find('\n', b);
    if (e == std::string::npos) e = text.size();
    const std::string row = text.substr(b, e - b);
    b = e + 1;
    const char *c = row.c_str();
    uint32_t got = 0;
    for (;; ++got) {
      while (*c == ' ' || *c == '\t' || *c == '\r') ++c;
      if (!*c) break;
      char *end = nullptr;
      const double v = strtod(c, &end);
      if (end == c) {
        fprintf(stderr, "error: %s line %u: \"%.20s\" is not a number\n", path.c_str(), line + 1, c);
        return -1;
      }
      if (!(v >= 0.0 && v <= 1.0)) {
        fprintf(stderr, "error: %s line %u: the rate %g is not in [0, 1]\n", path.c_str(), line + 1, v);
        return -1;
      }
      if (line < k && got < k) B[(size_t)line * k + got] = v;
      c = end;
    }
    if (line >= k || got != k) {
      fprintf(stderr, "error: %s line %u holds %u values; -k %u wants %u lines of %u\n", path.c_str(), line + 1, got, k, k, k);
      return -1;
    }
  }
  if (line != k) {
    fprintf(stderr, "error: %s line %u is missing: %u lines, -k %u wants %u lines of %u\n", path.c_str(), line + 1, line, k, k, k);
    return -1;
  }
  return 0;
}

int run_ppc(Env &env, Network &network, const PpcOptions &opt) {
  const uint32_t n = env.n, K = env.k, R = opt.draws;
  LinkCommunities model(env, network);   // -gml's loader and checks
  std::vector<double> B;                 // -ppc-orig: the point estimate, the same for every replicate
  if (opt.orig) {
    B.resize((size_t)K * K);
    if (model.load_gamma() < 0 || read_block_rates("beta.txt", K, B.data()) < 0) return -1;
  } else if (model.load_model() < 0) {
    return -1;
  }
  const std::vector<double> &gam = model.gamma(), &lam = model.lambda();
  // estimate_all (:700-729): pi = gamma / sum in k order, beta = l0 / (l0 + l1)
  std::vector<double> pim((size_t)n * K), betam(K), pi, beta;
  for (uint32_t i = 0; i < n; ++i) {
    double s = 0;
    for (uint32_t j = 0; j < K; ++j) s += gam[(size_t)i * K + j];
    for (uint32_t j = 0; j < K; ++j) pim[(size_t)i * K + j] = gam[(size_t)i * K + j] / s;
  }
  if (!opt.orig)
    for (uint32_t j = 0; j < K; ++j) betam[j] = lam[2 * j] / (lam[2 * j] + lam[2 * j + 1]);
  const std::vector<Edge> &ed = network.edges();
  std::vector<uint32_t> links(2 * ed.size());
  for (size_t x = 0; x < ed.size(); ++x) {
    links[2 * x] = ed[x].first;
    links[2 * x + 1] = ed[x].second;
  }
  Handle h(env.device, n, K, list_room(ed.size()));
  // the observed network under the mean parameters
  if (opt.orig) h.params_orig(pim.data(), B.data()); else h.params(pim.data(), betam.data());
  if (int rc = svils_ppc_set_links(h.h, links.data(), ed.size())) throw_svils("svils_ppc_set_links", rc);
  const Scalars obs = h.stats();
  make_dir("ppc");
  write_file("ppc/obs.txt", row_of(obs));
  write_file("obs-ones.txt", fx(obs.density) + "\n");            // obs_ones, obs_avg_deg (:640-660)
  write_file("obs-avg-deg.txt", fx(obs.avgdeg) + "\n");
  write_file("obs-max-deg.txt", std::to_string(obs.maxdeg) + "\n");
  Hops obs_hops{};
  std::vector<Hops> rep_hops;
  if (opt.hops) {                                               // ppc_avg_deg's hop.ppc.tab (:340-380): exact here, nstat's is an estimate
    obs_hops = h.hops();
    std::string t;
    uint64_t c = 0;
    for (size_t l = 0; l < obs_hops.D.size(); ++l) {
      c += obs_hops.D[l];
      t += std::to_string(l) + "\t" + std::to_string(obs_hops.D[l]) + "\t" + std::to_string(c) + "\n";
    }
    write_file("ppc/obs-hops.txt", t);
    write_file("obs-hop.txt", fx(obs_hops.effdiam) + "\n");
  }
  std::vector<Scalars> rep;
  std::string rows, ones, avg, mx;
  if (!opt.mean) {
    pi.resize((size_t)n * K);
    beta.resize(K);
  }
  for (uint32_t r = 0; r < R; ++r) {
    printf("ppc draw: %u / %u\n", r, R);
    fflush(stdout);
    if (!opt.mean) {                                            // draw_all (:730-742), afresh for every replicate
      dirichlet_rows(gam.data(), n, K, opt.seed, r, pi.data());
      if (opt.orig) {
        h.params_orig(pi.data(), B.data());
      } else {
        beta_draws(lam.data(), K, opt.seed, r, beta.data());
        h.params(pi.data(), beta.data());
      }
    }
    if (int rc = svils_ppc_draw(h.h, opt.seed, r)) throw_svils("svils_ppc_draw", rc);
    rep.push_back(h.stats());
    const Scalars &s = rep.back();
    rows += row_of(s);
    ones += fx(s.density) + "\n";                               // ppc_ones, ppc_avg_deg (:339-362, :632-638)
    avg += fx(s.avgdeg) + "\n";
    mx += std::to_string(s.maxdeg) + "\n";
    if (opt.hops) rep_hops.push_back(h.hops());
    if (r < opt.save) {
      make_dir("ppc/" + std::to_string(r));
      write_links("ppc/" + std::to_string(r) + "/network.dat", h.links());
    }
  }
  write_file("ppc/rep.txt", rows);
  write_file("ppc/ppc-ones.txt", ones);
  write_file("ppc/ppc-avg-deg.txt", avg);
  write_file("ppc/ppc-max-deg.txt", mx);
  std::vector<double> x(R);
  if (opt.orig) {
    // per block, row-major: g, h, observed, replicate mean, deviation, z
    std::string bsz, bpe;
    for (uint32_t t = 0; t < K * K; ++t) {
      const std::string gh = std::to_string(t / K) + "\t" + std::to_string(t % K) + "\t";
      for (uint32_t r = 0; r < R; ++r) x[r] = (double)rep[r].size[t];
      const Moments ms(x, (double)obs.size[t]);
      bsz += gh + std::to_string(obs.size[t]) + "\t" + fx(ms.mean) + "\t" + fx(ms.sd) + "\t" + fx(ms.z) + "\n";
      for (uint32_t r = 0; r < R; ++r) x[r] = rep[r].logpe[t];
      const Moments mp(x, obs.logpe[t]);
      bpe += gh + fx(obs.logpe[t]) + "\t" + fx(mp.mean) + "\t" + fx(mp.sd) + "\t" + fx(mp.z) + "\n";
    }
    write_file("ppc/block_size.txt", bsz);
    write_file("ppc/block_logpe.txt", bpe);
  } else {
    // per community: k, observed, replicate mean, deviation, z (compute_lc_zscores, :286-320)
    std::string lsz, lpe, zsz, zpe;
    for (uint32_t k = 0; k < K; ++k) {
      for (uint32_t r = 0; r < R; ++r) x[r] = (double)rep[r].size[k];
      const Moments ms(x, (double)obs.size[k]);
      lsz += std::to_string(k) + "\t" + std::to_string(obs.size[k]) + "\t" + fx(ms.mean) + "\t" + fx(ms.sd) + "\t" + fx(ms.z) + "\n";
      zsz += std::to_string(k) + "\t" + fx(ms.z) + "\n";
      for (uint32_t r = 0; r < R; ++r) x[r] = rep[r].logpe[k];
      const Moments mp(x, obs.logpe[k]);
      lpe += std::to_string(k) + "\t" + fx(obs.logpe[k]) + "\t" + fx(mp.mean) + "\t" + fx(mp.sd) + "\t" + fx(mp.z) + "\n";
      zpe += std::to_string(k) + "\t" + fx(mp.z) + "\n";
    }
    write_file("ppc/lc_size.txt", lsz);
    write_file("ppc/lc_logpe.txt", lpe);
    write_file("ppc/lc_zscores_size.txt", zsz);
    write_file("ppc/lc_zscores_pe.txt", zpe);
  }
  // summary.txt: statistic, observed, replicate mean, deviation, two-sided posterior predictive p-value
  const struct { const char *name; double Scalars::*d; uint64_t Scalars::*u; int digits; } cols[] = {
      {"ones", nullptr, &Scalars::ones, 5},           {"density", &Scalars::density, nullptr, 8},
      {"avg_deg", &Scalars::avgdeg, nullptr, 5},      {"max_deg", nullptr, &Scalars::maxdeg, 5},
      {"triangles", nullptr, &Scalars::triangles, 5}, {"transitivity", &Scalars::transitivity, nullptr, 5},
      {"clustering", &Scalars::clustering, nullptr, 5},
      {"offdiag_share", &Scalars::offdiag, nullptr, 5}};   // -ppc-orig alone
  std::string sm;
  for (const auto &c : cols) {
    if (c.d == &Scalars::offdiag && !opt.orig) continue;
    auto val = [&](const Scalars &s) { return c.d ? s.*(c.d) : (double)(s.*(c.u)); };
    for (uint32_t r = 0; r < R; ++r) x[r] = val(rep[r]);
    sm += summary_row(c.name, val(obs), x, c.digits);
  }
  write_file("ppc/summary.txt", sm);
  if (opt.hops) {
    std::string eff, rh, hs;
    for (uint32_t r = 0; r < R; ++r) {
      const Hops &s = rep_hops[r];
      eff += fx(s.effdiam) + "\n";
      rh += std::to_string(r) + "\t" + fx(s.effdiam) + "\t" + std::to_string(s.diameter) + "\t" + fx(s.meandist) + "\t" +
            std::to_string(s.components) + "\t" + std::to_string(s.largest) + "\t" + std::to_string(s.isolated) + "\n";
    }
    write_file("ppc/ppc-hop.txt", eff);
    write_file("ppc/rep-hops.txt", rh);
    const struct { const char *name; double Hops::*d; uint64_t Hops::*u; } hcols[] = {
        {"effdiam", &Hops::effdiam, nullptr},       {"diameter", nullptr, &Hops::diameter}, {"meandist", &Hops::meandist, nullptr},
        {"components", nullptr, &Hops::components}, {"largest", nullptr, &Hops::largest},   {"isolated", nullptr, &Hops::isolated}};
    for (const auto &c : hcols) {
      auto val = [&](const Hops &s) { return c.d ? s.*(c.d) : (double)(s.*(c.u)); };
      for (uint32_t r = 0; r < R; ++r) x[r] = val(rep_hops[r]);
      hs += summary_row(c.name, val(obs_hops), x, 5);
    }
    write_file("ppc/hops-summary.txt", hs);
  }
  printf("+ wrote ppc/summary.txt (%u replicates)\n", R);
  return 0;
}

int run_gen(uint32_t n, uint32_t k, uint32_t seed, int device) {
  // MMSBGen::gen (:43-71): pi_i ~ Dirichlet(0.05), beta_k ~ Beta(eta0_gen, eta1_gen) (src/env.hh:371-378), one draw
  std::vector<double> gam((size_t)n * k, 0.05), lam(2 * (size_t)k), pi((size_t)n * k), beta(k);
  for (uint32_t j = 0; j < k; ++j) {
    lam[2 * j] = 4700.59;
    lam[2 * j + 1] = 0.77;
  }
  dirichlet_rows(gam.data(), n, k, seed, 0, pi.data());
  beta_draws(lam.data(), k, seed, 0, beta.data());
  Handle h(device, n, k, (uint64_t)n * (n - 1) / 2);
  h.params(pi.data(), beta.data());
  printf("Generating network of size %u x %u\n", n, n);
  fflush(stdout);
  if (int rc = svils_ppc_draw(h.h, seed, 0)) throw_svils("svils_ppc_draw", rc);
  const std::vector<uint32_t> l = h.links();
  printf("\nWriting network (ones:%zu)\n", l.size() / 2);
  make_dir("gen");
  write_links("gen/network_gen.dat", l);
  std::string g, b;                                             // save_model (:784-838)
  for (uint32_t i = 0; i < n; ++i) {
    g += std::to_string(i) + "\t" + std::to_string(i) + "\t";
    for (uint32_t j = 0; j < k; ++j) g += fx(pi[(size_t)i * k + j]) + (j + 1 == k ? "\n" : "\t");
  }
  for (uint32_t j = 0; j < k; ++j) b += std::to_string(j) + "\t" + fx(beta[j]) + "\n";
  write_file("gen/pi-gen.txt", g);
  write_file("gen/beta-gen.txt", b);
  printf("done\n");
  return 0;
}

}  // namespace svinet
