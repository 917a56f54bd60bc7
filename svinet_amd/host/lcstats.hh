// lcstats.hh -- host side of `-gml` and `-lcstats`: the link communities of a fitted model.
//
// Same seam as the reference (src/mmsbgen.hh, used at src/main.cc:307-318):
//     MMSBGen mmsbgen(env, network, ppc);   mmsbgen.get_lc_stats();   /   mmsbgen.gml();
// The model files are read here (gamma.txt / lambda.txt of the working directory, MMSBGen::load_model, src/mmsbgen.cc:74-150),
// every per-node, per-link and per-community quantity is computed on the device through the svils_lc_* entry points of
// include/svils.h, and the files are written here in the reference's formats.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "env.hh"
#include "network.hh"
#include "util.hh"

struct svils_lc;

namespace svinet {

// Rows of a whitespace-separated text matrix, parsed by worker threads: every line must hold at least skip + cols numbers;
// the first skip go to lead[row][skip] (if non-null), the next cols to out[row][cols].  Exactly `rows` lines.  Returns 0,
// or -1 with a message on stderr.
int read_text_rows(const std::string &path, uint32_t skip, uint32_t cols, uint32_t rows, double *out, double *lead);

class LinkCommunities {
 public:
  LinkCommunities(Env &env, Network &network);
  ~LinkCommunities();

  // gamma.txt and lambda.txt of `dir` ("" = the working directory): n rows whose id column matches the reader's
  // numbering, k rows.  0, or -1 with a message on stderr.
  int load_model(const std::string &dir = "");
  int load_gamma(const std::string &dir = "");   // gamma.txt alone, with the same check (-ppc-orig: an -orig fit has no lambda.txt)
  void run();                 // the three device passes (throws SvilsError)
  // community_stats.txt, node_bridgeness.txt, node_influence.txt, number_of_memberships.txt into Env's directory
  void write_stats() const;
  void write_gml() const;     // network.gml (after write_stats: the reference's gml() calls get_lc_stats first)

  uint32_t n() const { return n_; }
  uint32_t k() const { return k_; }
  uint64_t unlikely() const { return counts_[0]; }
  uint64_t gml_edges() const { return counts_[1]; }
  uint64_t rechecked() const { return counts_[2]; }
  const double *timing_ms() const { return ms_; }
  // the loaded model, until run() hands gamma to the device: gamma [n][k], lambda [k][2] (ppc.cc reads it with this loader)
  const std::vector<double> &gamma() const { return gamma_; }
  const std::vector<double> &lambda() const { return lambda_; }

 private:
  double avg(uint32_t k) const;

  Env &env_;
  Network &network_;
  uint32_t n_, k_;
  std::vector<double> gamma_, lambda_;
  // results
  std::vector<uint32_t> group_, memb_, infl_, degc_, cnodes_, cmax_, cargmax_, gml_;
  std::vector<uint64_t> csum_;
  std::vector<double> bridg_;
  uint64_t counts_[3] = {0, 0, 0};
  double ms_[3] = {-1, -1, -1};
  svils_lc *h_ = nullptr;
};

}  // namespace svinet
