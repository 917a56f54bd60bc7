// sbm.hh -- the reference's `-single` engine: the single-membership stochastic blockmodel, the disjoint-community baseline
// of the package.
//
// `svinet -file F -n N -k K -single` in the reference constructs SBM and runs SBM::batch_infer() (src/main.cc:344-352,
// src/sbm.cc:457-543, src/sbm.hh): coordinate ascent over phi [n][K] (a node's distribution over the K groups), gamma [K]
// and lambda [K + 1][2] -- row K is the rate between different groups -- with a Gauss-Seidel E-step of at most 10 passes
// over the nodes and an M-step over all trained pairs.  include/svils.h (the svils_sbm section) has the written definition.
// Two backends, chosen at construction by Env::single_device:
//   device  (default)      every E-step, M-step and pair likelihood through the svils_sbm_* entry points (csrc/svils_sbm.hip):
//                          O((links + skipped pairs) K) per pass, at any n the memory holds.  The samplers, the starts, the
//                          sums of the likelihood rows in std::map order and the writers stay here.  A failed svils_sbm_* call
//                          throws SvilsError (util.hh); no HIP device is such a failure -- there is no fall-back to the host loops.
//   host    (-host-loops)  the reference's O(n^2 K) loops restated, single-threaded, as plumbing (what the CPU tests run).
//
// Seam mirrored:   SBM sbm(env, network);  sbm.batch_infer();
//
// The draws come in the reference's order from the one MT19937 stream: the held-out, the validation and the precision
// sample (10 links + 100 non-links; 1000 + 10^6 above n = 100 000), then gamma, lambda and phi.  A pair of any of the three
// samples is left out of training (edge_ok, src/sbm.hh:310-329).
//
// Quirks of the reference that are kept:
//   - row K of lambda sums (1 - phi_ik phi_jk) over k for every pair (src/sbm.cc:512-515), not 1 - sum_k;
//   - the three weighted columns of a heldout.txt / validation.txt row are 0: they are products with _ones_prob and
//     _zeros_prob, which SBM never sets (src/sbm.cc:11, :881-887);
//   - validation-pairs.txt is opened there and never written; here it lists the validation pairs as heldout-pairs.txt lists
//     the held-out ones.
// Departures, all forced:
//   - the reference's loop never ends, and its stop rule needs iter > 5000 on a value that is always 0 (src/sbm.cc:895): here
//     -single requires -max-iterations N, runs N iterations, then writes phi.txt, lambda.txt and gamma.txt in save_model's
//     formats (src/sbm.cc:297-338) -- unless -single-logl is given: then the variational lower bound (elbo(), DESIGN.md
//     section 4s: approx_log_likelihood, :1133-1239, compiled out there under GLOBALPHIS) is appended to logl.txt after the
//     M-step of every iteration, and the two rules of OrigStopRule (mmsbinferorig.hh) on it end the run: the bound below
//     its maximum at more than 3 reports with iter > 10 (max.txt in the ten columns of :926-932, t = 0, the bound in the
//     place of the held-out value that is always 0 there), or a relative gain below 1e-5 (done.txt).  -max-iterations is
//     then optional and still caps the run; -no-stop turns both rules off;
//   - compute_precision (:991-1060) is reached from the stop rule alone there; here a -single-logl run calls it when a rule
//     ends the run and when the run ends at -max-iterations: edge_likelihood2(p, q, 1) of the precision sample, ranked in
//     descending order -- ties by ascending pair, so the files are defined -- into precision.txt and hitcurve_<id>.txt;
//     an exact 0 of phi adds 0 to the bound's entropy (the reference gives NaN);
//   - a graph with too few links or non-links for the three samples is refused with a message (the reference draws for ever);
//   - network.gml is not written; without -single-logl neither are the lower bound, precision.txt and the hit curves;
//   - gsl_ran_gamma: the same Marsaglia-Tsang recipe as mmsbbatch.cc over the same MT19937 stream with a polar Box-Muller
//     Gaussian, so the distribution matches and the stream does not.
#pragma once
#include <cstdint>
#include <cstdio>
#include <ctime>
#include <map>
#include <vector>

#include "env.hh"
#include "mmsbinferorig.hh"   // OrigStopRule
#include "network.hh"
#include "rng.hh"
#include "svils.h"

namespace svinet {

// compute_precision's ranking (src/sbm.cc:1022-1056) on its own: pairs [m][2] with their scores and true y, ranked by
// descending score, ties by ascending pair.  c10 / c100 / c1000: the links among the first 10 / 100 / 1000 ranks
// (cumulative); curve: (rank, links so far) at rank 1 and at every 1000th
struct SbmPrecision {
  uint32_t c10 = 0, c100 = 0, c1000 = 0;
  std::vector<uint32_t> curve;   // [rows][2]
};
SbmPrecision sbm_rank_precision(const uint32_t *pairs, const double *score, const uint8_t *y, size_t m);

class SBM {
 public:
  SBM(Env &env, Network &network);
  ~SBM();

  // env.max_iterations iterations (0 with -single-logl: until a stop rule fires), a heldout.txt and a validation.txt row
  // after each, then the model files; returns 0
  int batch_infer();
  // one iteration (E-step, M-step, Elogpi / Elogbeta) and its two rows; with -single-logl the bound's row after the M-step
  // and, where a rule answers a stop, max.txt / done.txt and compute_precision; iter() advances
  void sweep();
  // The variational lower bound of the current state: total, P, N, G.  Device backend:
  // svils_sbmelbo; -host-loops: the reference's O(n^2 K) loops restated
  void elbo(double out[4]);
  // approx_log_likelihood (:1133-1239): prints the bound, appends a row of logl.txt, drives the stop rules; the verdict
  OrigStopRule::Verdict approx_log_likelihood();
  const std::vector<double> &logl_rows() const { return logl_rows_; }   // [rows][2]: iter, total
  OrigStopRule::Verdict stop_rule_verdict() const { return verdict_; }  // of the last row
  OrigStopRule &stop_rule() { return rule_; }                           // enabled unless -no-stop
  SbmPrecision compute_precision();                                     // :991-1060; with files: precision.txt, hitcurve_<id>.txt

  uint32_t n() const { return n_; }
  uint32_t k() const { return k_; }
  uint32_t iter() const { return iter_; }
  std::vector<double> &phi() { fetch_state(); return phi_; }       // [n][k]
  std::vector<double> &gamma() { fetch_state(); return gamma_; }   // [k]
  std::vector<double> &lambda() { fetch_state(); return lambda_; } // [k + 1][2]
  const std::vector<double> &eta() const { return eta_; }          // [k + 1][2]
  const std::vector<uint32_t> &heldout_pairs() const { return heldout_pairs_; }         // [H][2] p < q, as drawn
  const std::vector<uint32_t> &validation_pairs() const { return validation_pairs_; }
  const std::vector<uint32_t> &precision_pairs() const { return precision_pairs_; }
  // [rows][8]: which (0 held-out, 1 validation), iter, mean, count, mean of the non-links, count, mean of the links, count
  const std::vector<double> &rows() const { return rows_; }
  uint32_t passes() const { return passes_; }                      // passes of the last E-step
  const std::vector<double> &msums() const { return msums_; }      // msum of every pass of the last E-step
  double edge_likelihood2(uint32_t p, uint32_t q, int y) const;    // src/sbm.hh:284-308, host
  // library callers: another start, as svils_sbm_set_state checks it on the device
  void set_state(const double *phi, const double *gamma, const double *lambda);
  svils_sbm *device() const { return dev_; }                       // null: host loops

 private:
  typedef std::map<Edge, bool> SampleMap;
  void attach_device();
  void fetch_state();
  bool edge_ok(const Edge &e) const;
  Edge random_edge(bool link);
  void set_sample(uint32_t zeros, uint32_t ones, SampleMap &map, std::vector<uint32_t> &list);
  void init_heldout();
  void init_state();
  void set_elog();
  void estep_host();
  void mstep_host();
  void likelihood_row(const SampleMap &pairs, FILE *f, int which);
  void elbo_host(double out[4]);
  void save_model();
  uint32_t duration() const { return (uint32_t)(time(0) - start_time_); }

  Env &env_;
  Network &network_;
  uint32_t n_, k_;
  uint32_t iter_ = 0;
  GslMt19937 rng_;
  GammaSampler gamma_rng_;
  SampleMap heldout_map_, validation_map_, precision_map_;
  std::vector<uint32_t> heldout_pairs_, validation_pairs_, precision_pairs_;
  std::vector<std::vector<uint32_t> > skipped_;   // per node, its partners in the three samples (the host loops' edge_ok)
  std::vector<double> phi_, gamma_, lambda_, eta_, elogpi_, elogbeta_, rows_, msums_;
  uint32_t passes_ = 0;
  time_t start_time_;
  FILE *hf_ = nullptr, *vf_ = nullptr, *lf_ = nullptr;
  std::vector<double> logl_rows_;
  OrigStopRule rule_;
  OrigStopRule::Verdict verdict_ = OrigStopRule::GO_ON;
  uint32_t hitcurve_id_ = 0;
  svils_sbm *dev_ = nullptr;
  bool host_stale_ = false;   // the device has swept since phi_ / gamma_ / lambda_ were fetched
};

}  // namespace svinet
