// findk.hh -- host side of `-findk`: the estimate of the number of communities.
//
// Same seam as the reference (src/fastinit.hh, used at src/main.cc:321-327):
//     FastInit fastinit(env, network, max_deg);   fastinit.batch_infer();
// The constructor does what the reference's does on the host (init_gamma, the held-out sample, the output files); every
// iteration's count, top-5 selection, likelihoods and groups run on the device through the svils_findk_* entry points of
// include/svils.h.  The padding draws of set_gamma stay here: they continue the one MT19937 stream in node order.
#pragma once
#include <cstdint>
#include <cstdio>
#include <ctime>
#include <map>
#include <string>
#include <vector>

#include "env.hh"
#include "network.hh"
#include "nmi.hh"
#include "rng.hh"
#include "util.hh"

struct svils_findk;

namespace svinet {

class FindK {
 public:
  static constexpr uint32_t S = 5;   // FastInit::_k
  // attach_device = false: the host-side state only (init_gamma and the held-out sample), no HIP device touched.
  // A failed svils_findk_* call throws SvilsError (util.hh), here and in step().
  FindK(Env &env, Network &network, bool attach_device = true);
  ~FindK();

  // the loop of batch_infer until the reference would exit(0): 0 after floor(log10 n) + 1 iterations, 1 when the
  // held-out stop rule fired
  int run();
  // one pass of the loop: 0 = an iteration with its groups, 1 = the stop rule fired (row written, no groups),
  // 2 = the loop was already over (nothing done)
  int step();

  uint32_t n() const { return n_; }
  uint32_t iter() const { return iter_; }
  const std::vector<uint32_t> &labels() const { return labels_; }   // [n][5], refreshed by step()
  const std::vector<double> &values() const { return values_; }
  const std::vector<uint32_t> &masks() const { return masks_; }     // [n] of the last groups
  const std::vector<uint32_t> &heldout_pairs() const { return held_; }   // [H][3] in map order
  const double *last_row() const { return row_; }                   // the 11 columns of the last heldout.txt row
  double training_ll() const { return training_ll_; }
  uint32_t unlikely() const { return unlikely_; }
  double pad_seconds() const { return pad_s_; }                      // host time of the padding draws of the last step
  uint32_t last_npad() const { return npad_; }
  svils_findk *handle() const { return h_; }

 private:
  void init_gamma();
  void init_heldout();
  bool edge_ok(const Edge &e) const;
  void get_random_edge(bool link, Edge &e);
  void attach();
  bool heldout_likelihood(const double sums[3]);   // true: stop
  void write_groups();
  uint32_t duration() const { return (uint32_t)(time(0) - start_time_); }

  Env &env_;
  Network &network_;
  uint32_t n_;
  GslMt19937 rng_;
  std::vector<uint32_t> labels_;
  std::vector<double> values_;
  std::map<Edge, bool> heldout_map_;
  std::vector<uint32_t> held_;
  std::vector<uint32_t> masks_;
  double total_pairs_, ones_prob_, zeros_prob_;
  uint32_t iter_ = 0;
  double prev_h_ = -2147483647, max_h_ = -2147483647;
  uint32_t nh_ = 0;
  bool done_ = false;
  double row_[11] = {};
  double training_ll_ = 0;
  uint32_t unlikely_ = 0;
  double pad_s_ = 0;
  uint32_t npad_ = 0;
  time_t start_time_;
  FILE *hf_ = nullptr, *uf_ = nullptr;
  Cover ground_truth_;
  std::vector<uint32_t> ext_order_;   // sequence ids in ascending order of their external ids
  svils_findk *h_ = nullptr;
};

}  // namespace svinet
