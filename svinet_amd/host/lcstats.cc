// lcstats.cc -- -gml / -lcstats (src/mmsbgen.cc:74-150, 181-285, 418-499, 911-961).  See lcstats.hh.
#include "lcstats.hh"

#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>

#include "fixedfmt.hh"
#include "svils.h"
#include "util.hh"

namespace svinet {

namespace {
// rows [0, n) formatted by row(i, RowOut &) in blocks on worker threads, written in order
template <class RowFn>
void write_text(const std::string &path, const char *what, uint32_t n, RowFn row) {
  FILE *f = open_or_die(path, what);
  const unsigned T = n < 4096 ? 1u : std::min(usable_cpus(), 16u);
  const uint32_t B = 4096;   // rows per block
  std::vector<std::string> buf(T);
  for (uint64_t w0 = 0; w0 < n; w0 += (uint64_t)T * B) {
    auto block = [&](unsigned t) {
      buf[t].clear();
      const uint64_t a = w0 + (uint64_t)t * B, b = std::min<uint64_t>(n, a + B);
      RowOut o(buf[t]);
      for (uint64_t i = a; i < b; ++i) row((uint32_t)i, o);
    };
    std::vector<std::thread> th;
    for (unsigned t = 1; t < T; ++t) th.emplace_back(block, t);
    block(0);
    for (auto &x : th) x.join();
    for (unsigned t = 0; t < T; ++t)
      if (!buf[t].empty() && fwrite(buf[t].data(), 1, buf[t].size(), f) != buf[t].size()) {
        printf("cannot write %s file:%s\n", what, strerror(errno));
        exit(-1);
      }
  }
  fclose(f);
}
}  // namespace

int read_text_rows(const std::string &path, uint32_t skip, uint32_t cols, uint32_t rows, double *out, double *lead) {
  FILE *f = fopen(path.c_str(), "rb");
  if (!f) {
    fprintf(stderr, "error: cannot read %s: %s\n", path.c_str(), strerror(errno));
    return -1;
  }
  std::string text;
  char chunk[1 << 16];
  size_t got;
  while ((got = fread(chunk, 1, sizeof chunk, f)) > 0) text.append(chunk, got);
  const bool bad = ferror(f);
  fclose(f);
  if (bad) {
    fprintf(stderr, "error: cannot read %s\n", path.c_str());
    return -1;
  }
  // lines as fgets sees them; each one ends in '\0' so that strtod stays inside it
  std::vector<size_t> start;
  for (size_t p = 0; p < text.size();) {
    start.push_back(p);
    const size_t e = text.find('\n', p);
    if (e == std::string::npos) break;
    text[e] = '\0';
    p = e + 1;
  }
  if (start.size() != rows) {
    fprintf(stderr, "error: %s has %zu rows, expected %u\n", path.c_str(), start.size(), rows);
    return -1;
  }
  const unsigned T = rows < 4096 ? 1u : std::min(usable_cpus(), 16u);
  std::vector<long> first_bad(T, -1);
  auto part = [&](unsigned t) {
    const uint64_t a = (uint64_t)rows * t / T, b = (uint64_t)rows * (t + 1) / T;
    for (uint64_t r = a; r < b; ++r) {
      const char *p = text.c_str() + start[r];
      uint32_t c = 0;
      for (; c < skip + cols; ++c) {
        char *q = nullptr;
        const double d = strtod(p, &q);
        if (q == p) break;
        p = q;
        if (c < skip) { if (lead) lead[r * skip + c] = d; }
        else out[r * cols + (c - skip)] = d;
      }
      if (c < skip + cols) {
        first_bad[t] = (long)r;
        return;
      }
    }
  };
  std::vector<std::thread> th;
  for (unsigned t = 1; t < T; ++t) th.emplace_back(part, t);
  part(0);
  for (auto &x : th) x.join();
  for (long r : first_bad)
    if (r >= 0) {
      fprintf(stderr, "error: %s: row %ld has fewer than %u numbers\n", path.c_str(), r + 1, skip + cols);
      return -1;
    }
  return 0;
}

LinkCommunities::LinkCommunities(Env &env, Network &network) : env_(env), network_(network), n_(env.n), k_(env.k) {}

LinkCommunities::~LinkCommunities() {
  if (h_) svils_lc_destroy(h_);
}

// MMSBGen::load_model (:74-150): "seq id g0 .. gK-1" rows, "k l0 l1" rows
int LinkCommunities::load_model(const std::string &dir) {
  if (load_gamma(dir) < 0) return -1;
  lambda_.assign(2 * (size_t)k_, 0.0);
  return read_text_rows(dir + "lambda.txt", 1, 2, k_, lambda_.data(), nullptr) < 0 ? -1 : 0;
}

int LinkCommunities::load_gamma(const std::string &dir) {
  fprintf(stderr, "+ Loading model\n");
  gamma_.assign((size_t)n_ * k_, 0.0);
  std::vector<double> lead(2 * (size_t)n_);
  if (read_text_rows(dir + "gamma.txt", 2, k_, n_, gamma_.data(), lead.data()) < 0) return -1;
  // the reference does not check the id column; a gamma.txt of another numbering would give wrong rows silently
  const std::vector<uint32_t> &s2i = network_.seq2id();
  for (uint32_t i = 0; i < n_; ++i)
    if (lead[2 * (size_t)i + 1] != (double)s2i[i]) {
      fprintf(stderr, "error: %sgamma.txt row %u names node %.0f; the network file numbers it %u (a model of another network?)\n",
              dir.c_str(), i + 1, lead[2 * (size_t)i + 1], s2i[i]);
      return -1;
    }
  return 0;
}

void LinkCommunities::run() {
  int rc = svils_lc_create(env_.device, n_, k_, &h_);
  if (rc) throw_svils("svils_lc_create", rc);
  const std::vector<Edge> &ed = network_.edges();
  std::vector<uint32_t> links(2 * ed.size());
  for (size_t x = 0; x < ed.size(); ++x) {
    links[2 * x] = ed[x].first;
    links[2 * x + 1] = ed[x].second;
  }
  if ((rc = svils_lc_set_graph(h_, links.data(), ed.size()))) throw_svils("svils_lc_set_graph", rc);
  if ((rc = svils_lc_set_model(h_, gamma_.data(), lambda_.data()))) throw_svils("svils_lc_set_model", rc);
  std::vector<double>().swap(gamma_);
  printf("+ Computing link communities\n");
  fflush(stdout);
  if ((rc = svils_lc_run(h_))) throw_svils("svils_lc_run", rc);
  group_.resize(n_);
  memb_.resize(n_);
  infl_.resize(n_);
  bridg_.resize(n_);
  degc_.resize((size_t)n_ * k_);
  cnodes_.resize(k_);
  csum_.resize(k_);
  cmax_.resize(k_);
  cargmax_.resize(k_);
  if ((rc = svils_lc_get_nodes(h_, group_.data(), bridg_.data(), memb_.data(), infl_.data()))) throw_svils("svils_lc_get_nodes", rc);
  if ((rc = svils_lc_get_degrees(h_, degc_.data()))) throw_svils("svils_lc_get_degrees", rc);
  if ((rc = svils_lc_get_communities(h_, cnodes_.data(), csum_.data(), cmax_.data(), cargmax_.data()))) throw_svils("svils_lc_get_communities", rc);
  if ((rc = svils_lc_get_links(h_, nullptr, nullptr, counts_))) throw_svils("svils_lc_get_links", rc);
  gml_.resize(3 * counts_[1]);
  if ((rc = svils_lc_get_gml(h_, nullptr, gml_.data()))) throw_svils("svils_lc_get_gml", rc);
  if ((rc = svils_lc_get_timing(h_, ms_))) throw_svils("svils_lc_get_timing", rc);
  svils_lc_destroy(h_);
  h_ = nullptr;
}

// Community::deg_stats: avg = s / m on the host, so an empty community prints what x86-64 prints for 0.0 / 0 ("-nan")
double LinkCommunities::avg(uint32_t k) const {
  const double s = (double)csum_[k];
  const double m = (double)cnodes_[k];
  return s / m;
}

void LinkCommunities::write_stats() const {
  const std::vector<uint32_t> &s2i = network_.seq2id();
  const uint32_t K = k_;
  // process_link_communities2 (:472-499)
  write_text(Env::file_str("/community_stats.txt"), "community stats", K, [&](uint32_t k, RowOut &o) {
    o.integer(k, '\t');
    o.fixed<5>(avg(k), '\t');
    o.fixed<5>((double)cmax_[k], '\t');
    o.integer(cargmax_[k], '\t');
    o.integer(s2i[cargmax_[k]], '\n');
  });
  printf("+ Computing bridgeness and influence\n");
  fflush(stdout);
  // bridgeness (:230-259)
  write_text(Env::file_str("/node_bridgeness.txt"), "node bridgeness", n_, [&](uint32_t i, RowOut &o) {
    const uint32_t g = group_[i];
    o.integer(i, '\t');
    o.integer(s2i[i], '\t');
    o.fixed<5>(bridg_[i], '\t');
    o.integer(infl_[i], '\t');
    o.integer(network_.deg(i), '\t');
    o.integer(cnodes_[g], '\t');
    o.fixed<5>(avg(g), '\t');
    o.fixed<5>((double)cmax_[g], '\t');
    o.integer(g, '\n');
  });
  // community_degrees (:261-285)
  write_text(Env::file_str("/node_influence.txt"), "node influence", n_, [&](uint32_t i, RowOut &o) {
    o.integer(i, '\t');
    o.integer(s2i[i], '\t');
    const uint32_t *row = &degc_[(size_t)i * K];
    for (uint32_t k = 0; k < K; ++k) o.integer(row[k], '\t');
    o.text("\n");
  });
  write_text(Env::file_str("/number_of_memberships.txt"), "number of memberships", n_, [&](uint32_t i, RowOut &o) {
    o.integer(i, '\t');
    o.integer(s2i[i], '\t');
    o.integer(memb_[i], '\n');
  });
}

// gml (:911-961)
void LinkCommunities::write_gml() const {
  const std::vector<uint32_t> &s2i = network_.seq2id();
  FILE *f = open_or_die(Env::file_str("/network.gml"), "gml");
  auto blocks = [&](uint64_t rows, auto row) {
    std::string s;
    for (uint64_t b0 = 0; b0 < rows; b0 += 65536) {
      s.clear();
      {
        RowOut o(s);
        for (uint64_t x = b0; x < std::min<uint64_t>(rows, b0 + 65536); ++x) row(x, o);
      }
      if (fwrite(s.data(), 1, s.size(), f) != s.size()) {
        printf("cannot write gml file:%s\n", strerror(errno));
        exit(-1);
      }
    }
  };
  fputs("graph\n[\n\tdirected 0\n", f);
  blocks(n_, [&](uint64_t x, RowOut &o) {
    const uint32_t i = (uint32_t)x;
    o.text("\tnode\n\t[\n\t\tid ");
    o.integer(i, '\n');
    o.text("\t\textid ");
    o.integer(s2i[i], '\n');
    o.text("\t\tgroup ");
    o.integer(group_[i], '\n');
    o.text("\t\tbridgeness ");
    o.fixed<5>(bridg_[i], '\n');
    o.text("\t\tinfluence ");
    o.integer(infl_[i], '\n');
    o.text("\t\tdegree ");
    o.integer(network_.deg(i), '\n');
    o.text("\t]\n");
  });
  blocks(counts_[1], [&](uint64_t x, RowOut &o) {   // (p asc, q asc): the reference's all-pairs loop
    o.text("\tedge\n\t[\n\t\tsource ");
    o.integer(gml_[3 * x], '\n');
    o.text("\t\ttarget ");
    o.integer(gml_[3 * x + 1], '\n');
    o.text("\t\tcolor ");
    o.integer(gml_[3 * x + 2], '\n');
    o.text("\t]\n");
  });
  fputs("]\n", f);
  fclose(f);
  printf("+ Done writing GML file. Visualize the communities using a tool such as Gephi.\n");
  fflush(stdout);
}

}  // namespace svinet
