// mmsbinferorig.hh -- the reference's `-orig` engine: the mixed-membership blockmodel of Airoldi et al. with a full
// K x K matrix of block rates, the only model of the package that can describe disassortative structure.
//
// `svinet -file F -n N -k K -orig` in the reference constructs MMSBInferOrig and runs MMSBInferOrig::batch_infer()
// (src/main.cc:330-334, src/mmsbinferorig.cc:212-294): coordinate ascent over every ORDERED pair (p, q), p != q, the
// fixed point of a pair being PhiComp2::update_phis_until_conv (src/mmsbinferorig.hh:110-226).  Two backends, chosen at
// construction by Env::orig_device:
//   device  (default)      every sweep and every pair likelihood through the svils_orig_* entry points of include/svils.h
//                          (csrc/svils_orig.hip); the samplers, the starts, the sums in std::map order and the writers
//                          stay here.  A failed svils_orig_* call throws SvilsError (util.hh); no HIP device is such a
//                          failure -- there is no fall-back to the host loops.
//   host    (-host-loops)  the reference's loops restated, single-threaded, as plumbing (what the CPU tests run).
//
// Seam mirrored:   MMSBInferOrig mmsb(env, network, itype);  mmsb.batch_infer();
//
// Quirks of the reference that are kept:
//   - training skips only the HELD-OUT map, and only in the orientation the pair was drawn in (:231-235): the reverse
//     orientation of a held-out pair and both orientations of the validation pairs are trained on.  -clean-holdout
//     (Env::clean_holdout) is this project's way out: the same draws, but both orientations of every held-out and every
//     validation pair are left out, on the device and in the host loops alike.  The link queries of a fitted state
//     (-predict-pairs, -recommend, -rank-pairs, -rank-heldout: run_queries) are offered with it only -- ranks of held-out
//     links the sweep has trained on would measure memorisation;
//   - both sides of a pair's update use L_y[g][h] with the other side's vector: the matrix is not transposed for the
//     second side (:129-137);
//   - the held-out and validation pairs are kept in the order drawn (no p < q), and the files list sequence ids.
// Departures, all forced:
//   - the reference's loop never ends and its stop rule is compiled out (:499-522): here -orig requires
//     -max-iterations N, runs N sweeps, then writes gamma.txt (this project's format) and beta.txt (K lines of K values) --
//     unless -logl is given: then the variational lower bound (elbo(), DESIGN.md section 4n: approx_log_likelihood,
//     :624-726 under GLOBALPHIS, of the CURRENT state over the visited pairs, with x log x for log(phi) phi) is written to
//     logl.txt after the constructor's rows and at every report, and OrigStopRule ends the run (the model is saved and the
//     queries run, as at the -max-iterations exit; the reference exits without saving);
//   - `_iter` is never initialised there; it starts at 0 here;
//   - the reference never seeds this engine; -seed is honoured here when given;
//   - the reference's printf of every beta entry is dropped;
//   - gsl_ran_gamma: the same Marsaglia-Tsang recipe as mmsbbatch.cc over the same MT19937 stream with a polar Box-Muller
//     Gaussian, so the distribution matches and the stream does not.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <ctime>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "env.hh"
#include "network.hh"
#include "rng.hh"
#include "svils.h"

namespace svinet {

// The stop rules of -orig -logl as a function of (iter, s), s the lower bound of a report.
//   drop  the reference's (:694-723): s > max remembers s (and the caller this report's rows) and clears nh; s < max with
//         iter > 10 counts nh up; nh > 3 ends the run (max.txt)
//   gain  the sibling's threshold (src/mmsbinfer.cc:2062-2081): s > prev, prev != 0 and |(s - prev) / prev| < 1e-5 ends the
//         run (done.txt) -- a loop on a shared machine must end
// enabled false (-no-stop): update() still tracks max and prev but never answers a stop.
struct OrigStopRule {
  enum Verdict { GO_ON = 0, STOP_DROP = 1, STOP_GAIN = 2 };
  bool enabled = true;
  double max = -1.7976931348623157e308, prev = 0;
  uint32_t nh = 0;
  bool new_max = false;   // the last update() raised max: the caller remembers the report's held-out and validation rows
  Verdict update(uint32_t iter, double s) {
    new_max = false;
    if (s > max) { max = s; nh = 0; new_max = true; }
    else if (s < max && iter > 10) nh++;
    const bool gain = s > prev && prev != 0 && fabs((s - prev) / prev) < 1e-5;
    prev = s;
    if (!enabled) return GO_ON;
    if (nh > 3) return STOP_DROP;
    return gain ? STOP_GAIN : GO_ON;
  }
};

class MMSBInferOrig {
 public:
  MMSBInferOrig(Env &env, Network &network, int itype);
  ~MMSBInferOrig();

  // env.max_iterations sweeps (0 with -logl: until a stop rule fires), a report every env.reportfreq of them, then gamma.txt
  // and beta.txt; returns 0
  int batch_infer();
  // The variational lower bound of the current state: total, P, N.  Device backend: svils_orig_elbo;
  // -host-loops: the loops restated.  pairs / rounds (either may be null): the visited pairs and their fixed-point rounds
  void elbo(double out[3], uint64_t *pairs = nullptr, uint64_t *rounds = nullptr);
  // approx_log_likelihood (:690-723): prints the bound, appends a row of logl.txt, drives the stop rule; true: end the run
  bool approx_log_likelihood();
  const std::vector<double> &logl_rows() const { return logl_rows_; }   // [rows][2]: iter, s
  OrigStopRule &stop_rule() { return rule_; }
  void sweep();    // one pass of :217-271 (iter() advances)
  // after the last sweep, device backend only: link-prob.txt, recommendations.txt, link-ranks.txt / heldout-ranks.txt and
  // link-ranks-summary.txt for the flags given, in the formats of pairfiles.hh, from the final state.  A score is
  // score(p, q) = pi_p^T beta pi_q in the listed orientation; the second direction's ranks use score(q, .)
  void run_queries();
  svils_orig *device() const { return dev_; }   // null: host loops
  void report();   // :276-290: groups.txt, communities.txt, summary.txt, a heldout.txt and a validation.txt row

  uint32_t n() const { return n_; }
  uint32_t k() const { return k_; }
  uint32_t iter() const { return iter_; }
  std::vector<double> &gamma() { fetch_state(); return gamma_; }   // [n][k]
  std::vector<double> &beta() { fetch_state(); return beta_; }     // [k][k]
  const std::vector<uint32_t> &heldout_edges() const { return heldout_edges_; }         // [H][2], as drawn
  const std::vector<uint32_t> &validation_edges() const { return validation_edges_; }   // [V][2]
  const std::vector<double> &rows() const { return rows_; }   // [rows][8]: which (0 held-out, 1 validation), iter, a, k, a0, k0, a1, k1
  uint64_t rounds_total() const { return rounds_total_; }     // rounds over all pairs of the last sweep
  double edge_likelihood(uint32_t p, uint32_t q, int y) const;   // :563-587, host
  // library callers: another start, gamma [n][k] and beta [k][k] (as svils_orig_set_state checks them on the device)
  void set_state(const double *gamma, const double *beta);
  // -host-loops only (tests): also skip these ordered pairs
  void skip_also(const std::vector<uint32_t> &pairs);

 private:
  void attach_device();
  void fetch_state();
  void init_heldout();
  void init_skip();
  void set_sample(int s, bool heldout);
  void init_gamma();
  void init_beta1();
  void init_beta2();
  std::vector<double> elogpi_rows() const;                // Elogpi [n][k] of gamma_ (sweep_host, elbo_host)
  void sweep_host();
  void elbo_host(double out[3], uint64_t *pairs, uint64_t *rounds);
  uint32_t fixed_point(const double *ep, const double *eq, const double *lf, double *phi1, double *phi2, uint32_t p, uint32_t q) const;
  void likelihood_row(const std::map<Edge, bool> &pairs, FILE *f, int which);
  void compute_and_log_groups();
  void save_model();
  uint32_t duration() const { return (uint32_t)(time(0) - start_time_); }

  Env &env_;
  Network &network_;
  uint32_t n_, k_;
  int itype_;
  uint32_t iter_ = 0;
  double total_pairs_, ones_prob_;
  GslMt19937 rng_;
  GammaSampler gamma_rng_;           // init_gamma's draws, over rng_
  std::map<Edge, bool> heldout_map_, validation_map_, extra_skip_;
  std::set<Edge> skip_;         // the ordered pairs a sweep leaves out (init_skip)
  std::vector<int> pp_ext_, rp_ext_;        // -predict-pairs / -rank-pairs: the ids as given, and as sequence ids
  std::vector<uint32_t> pp_seq_, rp_seq_;
  std::vector<uint32_t> heldout_edges_, validation_edges_;
  std::vector<double> gamma_, beta_, rows_;
  uint64_t rounds_total_ = 0;
  time_t start_time_;
  FILE *hf_ = nullptr, *vf_ = nullptr, *lf_ = nullptr;
  std::vector<double> logl_rows_;
  OrigStopRule rule_;
  double max_h_[3] = {0, 0, 0}, max_v_[3] = {0, 0, 0};   // the held-out / validation triples of the report at the maximum
  bool stopped_ = false;
  svils_orig *dev_ = nullptr;   // the device backend (null: host loops)
  bool host_stale_ = false;     // the device has swept since gamma_ / beta_ were fetched
};

}  // namespace svinet
