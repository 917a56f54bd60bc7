// mmsbbatch.hh -- the reference's `-batch` engine (BASELINE config 1).
//
// `svinet -file F -n N -k K -batch` in the reference constructs MMSBInfer and runs
// MMSBInfer::batch_infer() (src/main.cc:354-358): coordinate-ascent variational inference
// over ALL n(n-1)/2 pairs, on the CPU, single-threaded.  It is a different engine from the
// link-sampling hot path this repo accelerates (same flags, same output directory and file
// formats).  Two backends, chosen at construction by Env::batch_device:
//   host    (-batch)      the reference's loops restated, single-threaded, as plumbing;
//   device  (-batch-gpu)  every sweep and every pair likelihood through the svils_batch_* entry
//                         points of include/svils.h (csrc/svils_batch.hip); the samplers,
//                         init_gamma, the sums in std::map order, the stop rule and the writers
//                         stay here.  A failed svils_batch_* call throws SvilsError (util.hh); no
//                         HIP device is such a failure -- there is no fall-back to the host loops.
// It is NOT a fallback for `-link-sampling`: that path has no CPU route in this repo.
//
// -rnode / -rpair / -rpair -stratified (Env::sampled()) run MMSBInfer::infer() (src/mmsbinfer.cc:459-740) on the same
// object: the Robbins-Monro version of the same model, one mini-batch of pairs per iteration (infer(), step()).  The
// samplers, likelihoods, stop rule and writers are the ones above; the mini-batches are drawn here from the same MT19937
// stream (get_subsample, :1912-1945) and never depend on the state, so a whole report interval is drawn first and handed
// to the device in one call (svils_batch_step_node / svils_batch_step_pairs); -host-loops runs the restated loops instead.
//
// -infset (Env::infset) runs FastAMM::infer() (src/fastamm.cc:549-672) on the same object: informative-set sampling.  An
// iteration is a star -- a random start node with its links and its informative non-links (the set -preprocess wrote
// for it, Network::sparse_zeros), or with chance 1e-4 up to 200 non-informative non-links -- and moves only the rows of
// the star, each with the step size of its own counter.  What differs from the engines above is here (the node shuffle
// before the held-out sampler, init_gamma / init_lambda of :514-546, the draw, the restated step); the samplers, the
// fixed point, the likelihoods, the stop rule and the writers are the ones above.  A whole report interval is drawn
// first, counters and step sizes included, and handed to the device in one svils_batch_step_star call.
//
// -snode (Env::snode) runs FastAMM2::infer() (src/fastamm2.cc:535-702) on the same object: the stratified random node
// sampler.  The constructor is -infset's (the shuffle, the samplers, init_gamma / init_lambda, the -pairs files).  An
// iteration is a star again -- with chance 1/2 a random node and its links, else a random node and n / 10 of its
// non-links, a block of the shuffled order -- but EVERY row of gamma moves, with one step size: the rows of the star
// towards alpha + scale phi, all others towards alpha.  A report interval is drawn first and handed to the device in one
// svils_batch_step_strat call, which keeps the decay of the untouched rows as one factor per row.
//
// Seam mirrored:   MMSBInfer mmsb(env, network);  mmsb.batch_infer();
//
// Where the reference reads members it never initialises (`_iter`, `_ones_prob`,
// `_zeros_prob`: absent from the constructor, src/mmsbinfer.cc:8-41) this class uses 0 and
// the values Network::set_env_variables computes (the ones the authors' shipped run logged,
// example/n75-k4-mmsb-batch.tgz:param.txt).
#pragma once
#include <cstdint>
#include <cstdio>
#include <ctime>
#include <map>
#include <string>
#include <vector>

#include "env.hh"
#include "network.hh"
#include "rng.hh"
#include "svils.h"

namespace svinet {

class MMSBBatch {
 public:
  MMSBBatch(Env &env, Network &network);
  ~MMSBBatch();

  // Runs until the reference would exit: returns 0 when -max-iterations was reached, 1 when the
  // held-out stop rule fired (src/mmsbinfer.cc:2086-2174).
  int batch_infer();
  // one pass of the body of batch_infer()'s loop, without the report step (src/mmsbinfer.cc:846-889)
  void sweep();
  // the report step (:895-905); returns true when the stop rule fired
  bool report();
  void do_on_stop();                                      // :743-752
  // -logl: the variational lower bound of the current state, s = G + P + N (approx_log_likelihood, :1948-2056; the same
  // formula in src/fastamm.cc:1129-1232).  parts (may be null): s, G, P, N.  The device backend asks svils_batch_elbo; the
  // host loops run the restated sums with std::lgamma.  An entry of phi that is exactly 0 adds 0 (the reference: NaN)
  double elbo(double *parts);
  // ... printed, a row of logl.txt, and with -accuracy the rule that writes done.txt (:2058-2081; no shell-out to `mutual`)
  double approx_log_likelihood();
  const std::vector<double> &logl_rows() const { return logl_rows_; }   // [rows][2]: iter, s

  // the sampled-pair engines.  infer(): as batch_infer(), a report every reportfreq iterations
  int infer();
  // one drawn iteration: its start node (-rnode) or pair list, the factor of gammat / lambdat (scale, or scale / mbsize),
  // the step sizes (rho_lambda < 0: lambda waits, :613) and the family it was drawn from
  struct Drawn {
    uint32_t node = 0;
    std::vector<uint32_t> pairs;     // [m][2], p < q
    double scale = 0, rho_gamma = 0, rho_lambda = -1;
    int family = 0;
  };
  void step(uint32_t nsteps);                             // draws nsteps iterations, then runs them (:476-642)
  void keep_schedule(bool on) { keep_schedule_ = on; }   // library callers: every executed iteration stays in schedule()
  const std::vector<Drawn> &schedule() const { return schedule_; }
  // the pairs of a node's mini-batch (get_randomnode_edges, :1867-1876), [m][2]
  std::vector<uint32_t> node_pairs(uint32_t a) const;
  // -infset: one drawn iteration of FastAMM::infer -- the start node, kind 0 (its links and informative non-links,
  // opt_process) or 1 (non-informative non-links, opt_process_noninf), the partners in the reference's order with the
  // pair's y and the partner's step size, the start node's step size, scale and lambda's step size
  struct Star {
    uint32_t start = 0;
    int kind = 0;
    std::vector<uint32_t> partner;
    std::vector<uint8_t> y;
    std::vector<double> rho_partner;
    double rho_start = 0, scale = 0, rho_lambda = -1;
  };
  const std::vector<Star> &stars() const { return stars_; }               // with keep_schedule: every executed iteration
  const std::vector<uint32_t> &node_counts() const { return nodec_; }     // _nodec: times a node's row was moved
  const std::vector<uint32_t> &shuffled_nodes() const { return shuffled_; }

  uint32_t n() const { return n_; }
  uint32_t k() const { return k_; }
  uint32_t iter() const { return iter_; }
  std::vector<double> &gamma() { fetch_state(); return gamma_; }     // [n][k]
  std::vector<double> &lambda() { fetch_state(); return lambda_; }   // [k][2]
  const std::vector<uint32_t> &heldout_edges() const { return heldout_edges_; }         // [H][2], acceptance order
  const std::vector<uint32_t> &validation_edges() const { return validation_edges_; }   // [V][2]
  const std::vector<double> &heldout_rows() const { return rows_; }                     // [rows][10]
  // per-pair fixed point, PhiComp::update_phis_until_conv (src/mmsbinfer.hh:159-203)
  void phis(uint32_t p, uint32_t q, int y, double *phi1, double *phi2) const;
  double edge_likelihood(uint32_t p, uint32_t q, int y) const;                          // src/mmsbinfer.hh:634-668

 private:
  void attach_device();                                   // the svils_batch handle: graph, skip set, state
  void fetch_state();                                     // device backend: gamma_ / lambda_ follow the device
  [[noreturn]] void device_failed(const char *what, int rc);
  // edge_likelihood of every pair of a held-out map, in its order
  std::vector<double> pair_likelihoods(const std::map<Edge, bool> &pairs);
  void init_heldout();
  void set_sample(int s, bool heldout);
  void get_random_edge(bool heldout_flag, bool stratified, int family, Edge &e);
  bool edge_ok(const Edge &e, bool heldout_flag, bool stratified, int family) const;
  void init_gamma();
  void set_dir_exp();
  void set_elogbeta();                                    // Elogbeta of lambda_
  void blend_lambda(double rho, double scale, const std::vector<double> &lambdat);
  bool heldout_likelihood();
  void validation_likelihood(double *av);
  void save_model();
  void compute_and_log_groups();
  std::string edgelist_s(const std::vector<uint32_t> &pairs) const;
  uint32_t duration() const { return (uint32_t)(time(0) - start_time_); }

  Env &env_;
  Network &network_;
  uint32_t n_, k_;
  uint32_t iter_ = 0;
  double ones_prob_, zeros_prob_;
  GslMt19937 rng_;
  GammaSampler gamma_rng_;           // init_gamma's draws, over rng_
  std::map<Edge, bool> heldout_map_, validation_map_;
  std::vector<uint32_t> heldout_edges_, validation_edges_;
  std::vector<double> gamma_, gammanext_, lambda_, lambdanext_, elogpi_, elogbeta_;
  std::vector<double> rows_;
  double max_t_, max_h_, max_v_, prev_h_;
  uint32_t nh_ = 0;
  time_t start_time_;
  FILE *hf_ = nullptr, *vf_ = nullptr;
  FILE *lf_ = nullptr;               // logl.txt, open for rows under -logl alone
  double prev_w_ = -2147483647.0;    // _prev_w (src/mmsbinfer.cc:35)
  std::vector<double> logl_rows_;
  Drawn draw();                                           // get_subsample and the step sizes of iteration iter_ + drawn so far
  void step_host(const Drawn &d);
  int family_ = 0;                                        // _family, alternating under -stratified (:682-683)
  uint32_t drawn_ = 0;                                    // iterations drawn: the next one is number drawn_
  uint32_t lambda_start_iter_ = 0;
  bool delay_reported_ = false;
  bool keep_schedule_ = false;
  std::vector<Drawn> schedule_;
  // -infset (FastAMM, src/fastamm.cc)
  void shuffle_nodes();                                   // :506-511
  void init_gamma_lambda_infset();                        // :514-546
  Star draw_star();                                       // :574-605 with the lists of opt_process / opt_process_noninf
  // -snode (FastAMM2, src/fastamm2.cc).  A drawn iteration is a Star whose rho_start and every rho_partner are the one
  // step size of the iteration; kind 0: the links of the start node, 1: a block of its non-links
  Star draw_strat();                                      // :573-592 with the lists of opt_process / opt_process_noninf (:933-1165)
  void strat_host(const Star &d);                         // :565-640, the restated eager loops: all n rows move
  void star_host(const Star &d);                          // :565-616, the restated loops
  void step_stars(uint32_t nsteps);                       // -infset and -snode: draw a chunk, run it
  std::vector<uint32_t> shuffled_, nodec_;
  std::vector<Star> stars_;
  svils_batch *dev_ = nullptr;       // the device backend (null: host loops)
  bool host_stale_ = false;          // the device has swept since gamma_ / lambda_ were fetched
};

}  // namespace svinet
