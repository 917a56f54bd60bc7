// capi.cc -- C entry points over the host-side C++ classes, for Python
// (bench.py, tests) to obtain the product's own inputs for the C ABI of
// include/svils.h: graph reading, held-out sampling, gamma/lambda
// initialisation and the training-link list.  No device is touched here.
#include <chrono>
#include "fixedfmt.hh"
#include <cstring>
#include <memory>

#include "env.hh"
#include "findk.hh"
#include "svils.h"
#include "linksampling.hh"
#include "mmsbbatch.hh"
#include "mmsbinferorig.hh"
#include "network.hh"
#include "nmi.hh"
#include "ppc.hh"
#include "sbm.hh"

using namespace svinet;

// fn()'s result, or the svils_error of the svils_* call that failed in it
template <class Fn>
static int svils_rc(Fn fn) {
  try {
    return fn();
  } catch (const SvilsError &e) {
    return e.rc;
  }
}

extern "C" {

typedef struct {
  uint32_t n, k;
  double seed;
  double heldout_ratio;
  double link_thresh;
  uint32_t lt_min_deg;
  int32_t eta_type;        // 0 uniform, 1 fromdata, 2 sparse, 3 dense
  int32_t accuracy;
  int32_t defer_gamma;     // 1: no host init_gamma2 (the caller draws on the device: svih_init_links / svih_init_streams -> svils_init_gamma)
  int32_t batch_device;    // svih_batch_from_file: 1 = the device backend of the -batch engine (-batch-gpu), on `device`
  int32_t device;
  int32_t sampled;         // svih_batch_from_file: 0 = -batch; 1 -rnode, 2 -rpair, 3 -rpair -stratified (batch_device: on the device)
  int32_t nodelay;         // ... with -nodelay
  double tau0, kappa, nodetau0, nodekappa;   // their step sizes (svih_options_default: 1024, 0.9, 1024, 0.5)
  double inf_epsilon;      // svih_infset_from_file: the chance of a non-informative step (svih_options_default: 1e-4)
  int32_t logl;            // svih_batch_from_file / svih_infset_from_file: -logl, a row of the lower bound after the constructor and at every report
  int32_t sparse_graph;    // the sampled engines on the device: -sparse-graph (svils_batch_create_sparse, no cap on n)
} svih_options;

struct svih_setup {
  std::unique_ptr<Env> env;
  std::unique_ptr<Network> net;
  std::unique_ptr<LinkSampling> ls;
};

static svih_setup *make_setup(const svih_options *o, const char *path, const int32_t *pairs,
                              uint64_t nlines) {
  static const char *eta_names[] = {"uniform", "fromdata", "sparse", "dense"};
  Env::Args a;
  a.n = o->n;
  a.k = o->k;
  a.link_sampling = true;
  a.rand_seed = o->seed;
  a.hol_ratio = o->heldout_ratio;
  a.link_thresh = o->link_thresh;
  a.lt_min_deg = o->lt_min_deg;
  a.eta_type = eta_names[(o->eta_type >= 0 && o->eta_type < 4) ? o->eta_type : 0];
  a.accuracy = o->accuracy != 0;
  a.defer_init_gamma = o->defer_gamma != 0;
  a.write_files = false;
  svih_setup *s = new svih_setup();
  s->env.reset(new Env(a));
  s->net.reset(new Network(*s->env));
  if (path) {
    if (s->net->read(path) < 0) { delete s; return nullptr; }
  } else {
    s->net->read_pairs(pairs, nlines);
  }
  s->env->n = s->net->n() - s->net->singles();   // src/main.cc:291
  s->ls.reset(new LinkSampling(*s->env, *s->net, /*attach_device=*/false));
  return s;
}

void svih_options_default(svih_options *o, uint32_t n, uint32_t k) {
  memset(o, 0, sizeof *o);
  o->n = n; o->k = k; o->seed = 0; o->heldout_ratio = 0.01; o->link_thresh = 0.5;
  o->lt_min_deg = 0; o->eta_type = 0; o->accuracy = 0; o->defer_gamma = 0;
  o->batch_device = 0; o->device = 0;
  const Env::Args d;
  o->inf_epsilon = d.inf_epsilon;
  o->sampled = 0; o->nodelay = 0; o->tau0 = d.tau0; o->kappa = d.kappa; o->nodetau0 = d.nodetau0; o->nodekappa = d.nodekappa;
}
svih_setup *svih_setup_from_file(const char *path, const svih_options *o) { return make_setup(o, path, nullptr, 0); }
svih_setup *svih_setup_from_pairs(const int32_t *pairs, uint64_t nlines, const svih_options *o) {
  return make_setup(o, nullptr, pairs, nlines);
}
void svih_setup_free(svih_setup *s) { delete s; }

uint32_t svih_n(const svih_setup *s) { return s->ls->n(); }
uint32_t svih_k(const svih_setup *s) { return s->ls->k(); }
uint32_t svih_ones(const svih_setup *s) { return s->net->ones(); }
uint32_t svih_singles(const svih_setup *s) { return s->net->singles(); }
double svih_total_pairs(const svih_setup *s) { return s->ls->total_pairs(); }
double svih_ones_prob(const svih_setup *s) { return s->ls->ones_prob(); }
double svih_eta0(const svih_setup *s) { return s->env->eta0; }
double svih_eta1(const svih_setup *s) { return s->env->eta1; }
const uint32_t *svih_seq2id(const svih_setup *s) { return s->net->seq2id().data(); }
const double *svih_gamma(const svih_setup *s) { return s->ls->gamma().empty() ? nullptr : s->ls->gamma().data(); }   // null: defer_gamma
const double *svih_lambda(const svih_setup *s) { return s->ls->lambda().data(); }
uint64_t svih_nvalidation(const svih_setup *s) { return s->ls->validation_sorted().size() / 3; }
const uint32_t *svih_validation_sorted(const svih_setup *s) { return s->ls->validation_sorted().data(); }
const uint32_t *svih_validation_accept(const svih_setup *s) { return s->ls->validation_accept().data(); }
uint64_t svih_nlinks(svih_setup *s) { return s->ls->training_links().size() / 2; }
const uint32_t *svih_links(svih_setup *s) { return s->ls->training_links().data(); }
const uint32_t *svih_edges(const svih_setup *s) { return &s->net->edges()[0].first; }
// what svils_init_gamma takes (tests/test_gpu_init.py): the links in drawing order, the generator's states by jump-ahead
uint64_t svih_init_links(const svih_setup *s, uint32_t *out /* [ones][2] or null */) {
  std::vector<uint32_t> e;
  s->ls->init_links(&e);
  if (out) memcpy(out, e.data(), e.size() * sizeof(uint32_t));
  return e.size() / 2;
}
uint64_t svih_init_offset(const svih_setup *s) { return s->ls->init_offset(); }   // outputs drawn before init_gamma2 began
int svih_init_streams(const svih_setup *s, uint64_t nstreams, uint64_t per_stream, uint32_t *out /* [nstreams][624] */) {
  std::vector<uint32_t> st;
  if (!s->ls->init_streams(nstreams, per_stream, &st)) return -1;
  memcpy(out, st.data(), st.size() * sizeof(uint32_t));
  return 0;
}
uint32_t svih_deg(const svih_setup *s, uint32_t p) { return s->net->deg(p); }

// normalised mutual information of a communities.txt-style file against a ground-truth file in the
// "node<TAB>community ..." format of -nmi; < 0 when a file cannot be read
// jump-ahead of the random stream (rng.hh / mtjump.hh) against drawing: the `count` outputs from position `pos` on, once by
// GslMt19937::at(pos) and once by `pos` calls of get().  0: equal; 1: different; -1: the jump machinery is unavailable.
// out_ms (may be null): [0] time of the jump, [1] time of drawing up to pos.
int svih_mt_jump_check(unsigned long seed, uint64_t pos, uint32_t count, double *out_ms) {
  using clk = std::chrono::steady_clock;
  svinet::GslMt19937 a(seed), b(seed), j;
  const auto t0 = clk::now();
  if (!a.at(pos, &j)) return -1;
  const auto t1 = clk::now();
  for (uint64_t i = 0; i < pos; ++i) (void)b.get();
  const auto t2 = clk::now();
  if (out_ms) {
    out_ms[0] = std::chrono::duration<double, std::milli>(t1 - t0).count();
    out_ms[1] = std::chrono::duration<double, std::milli>(t2 - t1).count();
  }
  if (j.position() != pos || b.position() != pos) return 1;
  for (uint32_t i = 0; i < count; ++i)
    if (j.get() != b.get()) return 1;
  return j.position() == pos + count ? 0 : 1;
}

// the host random stream of -ppc / -gen (ppc.hh) for the tests: Philox4x32-10 of m counters ctr [m][4] under one key ->
// out [m][4], and the parameter draws of replicate r of seed
void svih_ppc_philox(const uint32_t *ctr, uint64_t m, const uint32_t *key, uint32_t *out) {
  for (uint64_t i = 0; i < m; ++i) philox4x32_10(ctr + 4 * i, key, out + 4 * i);
}
void svih_ppc_dirichlet(const double *gam, uint32_t n, uint32_t k, uint32_t seed, uint32_t r, double *pi) { dirichlet_rows(gam, n, k, seed, r, pi); }
void svih_ppc_beta(const double *lam, uint32_t k, uint32_t seed, uint32_t r, double *beta) { beta_draws(lam, k, seed, r, beta); }

double svih_nmi(const char *communities_path, const char *ground_truth_path) {
  Cover x, y;
  if (!read_cover_lines(communities_path, &x) || !read_cover_memberships(ground_truth_path, &y)) return -1.0;
  return lfk_nmi(y, x);
}

// ---- the -batch engine (host CPU), for the tests ----
struct svih_batch {
  std::unique_ptr<Env> env;
  std::unique_ptr<Network> net;
  std::unique_ptr<MMSBBatch> eng;
};

// neighbors non-null: the -infset engine with the informative sets of that file; snode: the -snode engine
static svih_batch *make_batch(const char *path, const svih_options *o, const char *neighbors, bool snode = false) {
  static const char *eta_names[] = {"uniform", "fromdata", "sparse", "dense"};
  Env::Args a;
  a.n = o->n;
  a.k = o->k;
  if (neighbors || snode) {
    a.infset = !snode;
    a.snode = snode;
    if (snode) a.rfreq = 100;
    a.host_loops = o->batch_device == 0;
    a.inf_epsilon = o->inf_epsilon;
    a.tau0 = o->tau0; a.kappa = o->kappa; a.nodetau0 = o->nodetau0; a.nodekappa = o->nodekappa;
  } else if (o->sampled) {
    a.rnode = o->sampled == 1;
    a.rpair = o->sampled >= 2;
    a.stratified = o->sampled == 3;
    a.nodelay = o->nodelay != 0;
    a.host_loops = o->batch_device == 0;
    a.rfreq = 100;
    a.tau0 = o->tau0; a.kappa = o->kappa; a.nodetau0 = o->nodetau0; a.nodekappa = o->nodekappa;
  } else {
    a.batch = true;
    a.batch_gpu = o->batch_device != 0;
  }
  a.device = o->device;
  a.logl = o->logl != 0;
  a.sparse_graph = o->sparse_graph != 0;   // (the all-pairs passes of such a handle answer SVILS_ERR_UNSUPPORTED: a sweep, the lower bound)
  a.rand_seed = o->seed;
  a.hol_ratio = o->heldout_ratio;
  a.eta_type = eta_names[(o->eta_type >= 0 && o->eta_type < 4) ? o->eta_type : 0];
  a.write_files = false;
  svih_batch *b = new svih_batch();
  b->env.reset(new Env(a));
  b->net.reset(new Network(*b->env));
  if (b->net->read(path) < 0) { delete b; return nullptr; }
  if (neighbors && b->net->load_neighborhood_sets(neighbors)) { delete b; return nullptr; }
  b->env->n = b->net->n() - b->net->singles();
  if (svils_rc([&] { b->eng.reset(new MMSBBatch(*b->env, *b->net)); return 0; })) {   // svils_last_error() keeps the library's text
    delete b;
    return nullptr;
  }
  b->eng->keep_schedule(o->sampled != 0 || neighbors || snode);
  return b;
}
svih_batch *svih_batch_from_file(const char *path, const svih_options *o) { return make_batch(path, o, nullptr); }
// the -infset engine (svih_batch_step steps it; its schedule: svih_batch_nstars / svih_batch_star)
svih_batch *svih_infset_from_file(const char *path, const char *neighbors, const svih_options *o) { return make_batch(path, o, neighbors); }
// the -snode engine (svih_batch_step steps it; its schedule is read as -infset's; o->inf_epsilon: the chance of a non-link step)
svih_batch *svih_snode_from_file(const char *path, const svih_options *o) { return make_batch(path, o, nullptr, true); }
// -preprocess: the informative sets of the graph of `path` (declared n nodes) into `out` in the reference's format; 0, or -1
int svih_preprocess(const char *path, uint32_t n, const char *out) {
  Env::Args a;
  a.n = n;
  a.k = 2;
  a.write_files = false;
  Env env(a);
  Network net(env);
  if (net.read(path) < 0) return -1;
  return net.write_neighborhood_sets(out) ? 0 : -1;
}
uint64_t svih_batch_nstars(const svih_batch *b) { return b->eng->stars().size(); }
// out[5]: start, kind, scale, rho_start, rho_lambda; returns the number of entries and with non-null arrays copies them
uint64_t svih_batch_star(const svih_batch *b, uint64_t i, double *out, uint32_t *partner, uint8_t *y, double *rho_partner) {
  const MMSBBatch::Star &d = b->eng->stars()[i];
  if (out) { out[0] = d.start; out[1] = d.kind; out[2] = d.scale; out[3] = d.rho_start; out[4] = d.rho_lambda; }
  const size_t m = d.partner.size();
  if (partner && m) memcpy(partner, d.partner.data(), m * sizeof(uint32_t));
  if (y && m) memcpy(y, d.y.data(), m);
  if (rho_partner && m) memcpy(rho_partner, d.rho_partner.data(), m * sizeof(double));
  return m;
}
const uint32_t *svih_batch_node_counts(const svih_batch *b) { return b->eng->node_counts().data(); }
const uint32_t *svih_batch_shuffled(const svih_batch *b) { return b->eng->shuffled_nodes().data(); }
// the sampled-pair engines: nsteps iterations (drawn, then run); the schedule of every executed iteration
int svih_batch_step(svih_batch *b, uint32_t nsteps) { return svils_rc([&] { b->eng->step(nsteps); return 0; }); }
uint64_t svih_batch_nschedule(const svih_batch *b) { return b->eng->schedule().size(); }
// out[5]: node, family, scale, rho_gamma, rho_lambda; returns the number of pairs of the iteration's mini-batch, and with
// pairs non-null copies them ([m][2]; -rnode: the pairs of the start node outside the held-out sets)
uint64_t svih_batch_schedule(const svih_batch *b, uint64_t i, double *out, uint32_t *pairs) {
  const MMSBBatch::Drawn &d = b->eng->schedule()[i];
  if (out) { out[0] = d.node; out[1] = d.family; out[2] = d.scale; out[3] = d.rho_gamma; out[4] = d.rho_lambda; }
  const std::vector<uint32_t> np = b->env->randomnode ? b->eng->node_pairs(d.node) : std::vector<uint32_t>();
  const std::vector<uint32_t> &pq = b->env->randomnode ? np : d.pairs;
  if (pairs && !pq.empty()) memcpy(pairs, pq.data(), pq.size() * sizeof(uint32_t));
  return pq.size() / 2;
}
double svih_batch_total_pairs(const svih_batch *b) { return (double)b->env->total_pairs; }
void svih_batch_free(svih_batch *b) { delete b; }
uint32_t svih_batch_n(const svih_batch *b) { return b->eng->n(); }
uint32_t svih_batch_iter(const svih_batch *b) { return b->eng->iter(); }
double *svih_batch_gamma(svih_batch *b) { return b->eng->gamma().data(); }
double *svih_batch_lambda(svih_batch *b) { return b->eng->lambda().data(); }
uint64_t svih_batch_nheldout(const svih_batch *b) { return b->eng->heldout_edges().size() / 2; }
const uint32_t *svih_batch_heldout(const svih_batch *b) { return b->eng->heldout_edges().data(); }
uint64_t svih_batch_nvalidation(const svih_batch *b) { return b->eng->validation_edges().size() / 2; }
const uint32_t *svih_batch_validation(const svih_batch *b) { return b->eng->validation_edges().data(); }
uint64_t svih_batch_nrows(const svih_batch *b) { return b->eng->heldout_rows().size() / 10; }
const double *svih_batch_rows(const svih_batch *b) { return b->eng->heldout_rows().data(); }
int svih_batch_sweep(svih_batch *b) { return svils_rc([&] { b->eng->sweep(); return 0; }); }   // < 0: a svils_error of the device backend
int svih_batch_report(svih_batch *b) { return svils_rc([&] { return b->eng->report() ? 1 : 0; }); }
// the variational lower bound of the current state: parts[4] = total, G, P, N (MMSBBatch::elbo); the rows -logl has written
int svih_batch_elbo(svih_batch *b, double *parts) { return svils_rc([&] { b->eng->elbo(parts); return 0; }); }
uint64_t svih_batch_nlogl(const svih_batch *b) { return b->eng->logl_rows().size() / 2; }
const double *svih_batch_logl(const svih_batch *b) { return b->eng->logl_rows().data(); }
double svih_batch_eta0(const svih_batch *b) { return b->env->eta0; }
double svih_batch_eta1(const svih_batch *b) { return b->env->eta1; }
double svih_batch_ones_prob(const svih_batch *b) { return b->env->ones_prob; }
const uint32_t *svih_batch_edges(const svih_batch *b) { return &b->net->edges()[0].first; }
uint32_t svih_batch_ones(const svih_batch *b) { return b->net->ones(); }

// ---- the -orig engine (MMSBInferOrig): on_device 0 = the host loops, 1 = svils_orig_* on `device` ----
struct svih_orig {
  std::unique_ptr<Env> env;
  std::unique_ptr<Network> net;
  std::unique_ptr<MMSBInferOrig> eng;
};
// clean_holdout: -clean-holdout (both orientations of every held-out and validation pair are left out of training)
static svih_orig *orig_from_file(const char *path, uint32_t n, uint32_t k, double seed, double heldout_ratio, int32_t itype,
                                 int32_t on_device, int32_t device, int32_t clean_holdout, int32_t logl) {
  Env::Args a;
  a.n = n;
  a.k = k;
  a.orig = true;
  a.itype = itype;
  a.host_loops = on_device == 0;
  a.clean_holdout = clean_holdout != 0;
  a.device = device;
  a.rand_seed = seed;
  a.hol_ratio = heldout_ratio;
  a.write_files = false;
  a.logl = logl != 0;
  svih_orig *b = new svih_orig();
  b->env.reset(new Env(a));
  b->net.reset(new Network(*b->env));
  if (b->net->read(path) < 0) { delete b; return nullptr; }
  b->env->n = b->net->n() - b->net->singles();
  if (svils_rc([&] { b->eng.reset(new MMSBInferOrig(*b->env, *b->net, itype)); return 0; })) {   // svils_last_error() keeps the library's text
    delete b;
    return nullptr;
  }
  return b;
}
svih_orig *svih_orig_from_file(const char *path, uint32_t n, uint32_t k, double seed, double heldout_ratio, int32_t itype,
                               int32_t on_device, int32_t device, int32_t clean_holdout) {
  return orig_from_file(path, n, k, seed, heldout_ratio, itype, on_device, device, clean_holdout, 0);
}
// logl: -logl (a row of the lower bound after the constructor's rows and at every report: svih_orig_logl_rows)
svih_orig *svih_orig_from_file_logl(const char *path, uint32_t n, uint32_t k, double seed, double heldout_ratio, int32_t itype,
                                    int32_t on_device, int32_t device, int32_t clean_holdout, int32_t logl) {
  return orig_from_file(path, n, k, seed, heldout_ratio, itype, on_device, device, clean_holdout, logl);
}
void svih_orig_free(svih_orig *b) { delete b; }
// the variational lower bound of the current state: out = total, P, N; stats = pairs visited, fixed-point rounds
int svih_orig_elbo(svih_orig *b, double *out, uint64_t *stats) {
  return svils_rc([&] { b->eng->elbo(out, stats, stats ? stats + 1 : nullptr); return 0; });
}
uint64_t svih_orig_nlogl_rows(const svih_orig *b) { return b->eng->logl_rows().size() / 2; }
const double *svih_orig_logl_rows(const svih_orig *b) { return b->eng->logl_rows().data(); }   // [rows][2]: iter, s
// tests: the stop rule of -orig -logl on its own.  state [4]: max, prev, nh, enabled (in and out); returns the verdict
// (0 go on, 1 the drop rule, 2 the gain rule)
int32_t svih_orig_stop_rule(double *state, uint32_t iter, double s) {
  OrigStopRule r;
  r.max = state[0];
  r.prev = state[1];
  r.nh = (uint32_t)state[2];
  r.enabled = state[3] != 0;
  const int32_t v = (int32_t)r.update(iter, s);
  state[0] = r.max;
  state[1] = r.prev;
  state[2] = (double)r.nh;
  return v;
}
uint32_t svih_orig_n(const svih_orig *b) { return b->eng->n(); }
uint32_t svih_orig_iter(const svih_orig *b) { return b->eng->iter(); }
int svih_orig_gamma(svih_orig *b, double *out) {
  return svils_rc([&] { memcpy(out, b->eng->gamma().data(), b->eng->gamma().size() * sizeof(double)); return 0; });
}
int svih_orig_beta(svih_orig *b, double *out) {
  return svils_rc([&] { memcpy(out, b->eng->beta().data(), b->eng->beta().size() * sizeof(double)); return 0; });
}
uint64_t svih_orig_nheldout(const svih_orig *b) { return b->eng->heldout_edges().size() / 2; }
const uint32_t *svih_orig_heldout(const svih_orig *b) { return b->eng->heldout_edges().data(); }
uint64_t svih_orig_nvalidation(const svih_orig *b) { return b->eng->validation_edges().size() / 2; }
const uint32_t *svih_orig_validation(const svih_orig *b) { return b->eng->validation_edges().data(); }
uint64_t svih_orig_nrows(const svih_orig *b) { return b->eng->rows().size() / 8; }
const double *svih_orig_rows(const svih_orig *b) { return b->eng->rows().data(); }
uint64_t svih_orig_rounds_total(const svih_orig *b) { return b->eng->rounds_total(); }
int svih_orig_sweep(svih_orig *b) { return svils_rc([&] { b->eng->sweep(); return 0; }); }   // < 0: a svils_error of the device backend
int svih_orig_report(svih_orig *b) { return svils_rc([&] { b->eng->report(); return 0; }); }
int svih_orig_set_state(svih_orig *b, const double *gamma, const double *beta) {
  return svils_rc([&] { b->eng->set_state(gamma, beta); return 0; });
}
void svih_orig_skip_also(svih_orig *b, const uint32_t *pairs, uint64_t m) { b->eng->skip_also(std::vector<uint32_t>(pairs, pairs + 2 * m)); }
const uint32_t *svih_orig_edges(const svih_orig *b) { return &b->net->edges()[0].first; }
uint32_t svih_orig_ones(const svih_orig *b) { return b->net->ones(); }
// the engine's svils_orig handle, for the link queries of include/svils.h (null: host loops); the engine keeps owning it
void *svih_orig_device(const svih_orig *b) { return b->eng->device(); }

// ---- the -single engine (SBM): on_device 0 = the host loops, 1 = svils_sbm_* on `device` ----
struct svih_sbm {
  std::unique_ptr<Env> env;
  std::unique_ptr<Network> net;
  std::unique_ptr<SBM> eng;
};
static svih_sbm *sbm_from_file(const char *path, uint32_t n, uint32_t k, double seed, double heldout_ratio, int32_t on_device,
                               int32_t device, int32_t logl, int32_t stop) {
  Env::Args a;
  a.n = n;
  a.k = k;
  a.single = true;
  a.single_logl = logl != 0;
  a.use_validation_stop = stop != 0;
  a.host_loops = on_device == 0;
  a.device = device;
  a.rand_seed = seed;
  a.hol_ratio = heldout_ratio;
  a.write_files = false;
  svih_sbm *b = new svih_sbm();
  b->env.reset(new Env(a));
  b->net.reset(new Network(*b->env));
  if (b->net->read(path) < 0) { delete b; return nullptr; }
  b->env->n = b->net->n() - b->net->singles();
  if (svils_rc([&] { b->eng.reset(new SBM(*b->env, *b->net)); return 0; })) {   // svils_last_error() keeps the library's text
    delete b;
    return nullptr;
  }
  return b;
}
svih_sbm *svih_sbm_from_file(const char *path, uint32_t n, uint32_t k, double seed, double heldout_ratio, int32_t on_device,
                             int32_t device) {
  return sbm_from_file(path, n, k, seed, heldout_ratio, on_device, device, 0, 1);
}
// logl: -single-logl (a row of the lower bound after the M-step of every sweep: svih_sbm_logl_rows); stop 0: -no-stop
svih_sbm *svih_sbm_from_file_logl(const char *path, uint32_t n, uint32_t k, double seed, double heldout_ratio, int32_t on_device,
                                  int32_t device, int32_t logl, int32_t stop) {
  return sbm_from_file(path, n, k, seed, heldout_ratio, on_device, device, logl, stop);
}
// the variational lower bound of the current state: out = total, P, N, G
int svih_sbm_elbo(svih_sbm *b, double *out) { return svils_rc([&] { b->eng->elbo(out); return 0; }); }
uint64_t svih_sbm_nlogl_rows(const svih_sbm *b) { return b->eng->logl_rows().size() / 2; }
const double *svih_sbm_logl_rows(const svih_sbm *b) { return b->eng->logl_rows().data(); }   // [rows][2]: iter, total
int32_t svih_sbm_stop_rule_verdict(const svih_sbm *b) { return (int32_t)b->eng->stop_rule_verdict(); }   // 0 go on, 1 drop, 2 gain
// tests: the engine's own stop rule (enabled unless -no-stop) fed a made-up row; the verdict.  Not a row of logl_rows
int32_t svih_sbm_feed_stop_rule(svih_sbm *b, uint32_t iter, double s) { return (int32_t)b->eng->stop_rule().update(iter, s); }
// compute_precision of the current state: out = c10, c100, c1000 (cumulative)
int svih_sbm_precision(svih_sbm *b, uint32_t *out) {
  return svils_rc([&] {
    const SbmPrecision r = b->eng->compute_precision();
    out[0] = r.c10; out[1] = r.c100; out[2] = r.c1000;
    return 0;
  });
}
// tests: the ranking of compute_precision on its own.  out = c10, c100, c1000; curve [2 * curve_cap]: (rank, links so far)
// rows; returns the curve's rows
uint64_t svih_sbm_rank_precision(const uint32_t *pairs, const double *score, const uint8_t *y, uint64_t m, uint32_t *out, uint32_t *curve,
                                 uint64_t curve_cap) {
  const SbmPrecision r = sbm_rank_precision(pairs, score, y, m);
  out[0] = r.c10; out[1] = r.c100; out[2] = r.c1000;
  for (size_t i = 0; i < r.curve.size() && i < 2 * curve_cap; ++i) curve[i] = r.curve[i];
  return r.curve.size() / 2;
}
void svih_sbm_free(svih_sbm *b) { delete b; }
uint32_t svih_sbm_n(const svih_sbm *b) { return b->eng->n(); }
uint32_t svih_sbm_iter(const svih_sbm *b) { return b->eng->iter(); }
uint32_t svih_sbm_passes(const svih_sbm *b) { return b->eng->passes(); }
const double *svih_sbm_msums(const svih_sbm *b) { return b->eng->msums().data(); }   // [passes]
// which 0: phi [n][k]; 1: gamma [k]; 2: lambda [k + 1][2]; 3: eta [k + 1][2]
int svih_sbm_state(svih_sbm *b, int32_t which, double *out) {
  return svils_rc([&] {
    const std::vector<double> &v = which == 0 ? b->eng->phi() : which == 1 ? b->eng->gamma() : which == 2 ? b->eng->lambda() : b->eng->eta();
    memcpy(out, v.data(), v.size() * sizeof(double));
    return 0;
  });
}
// which 0: the held-out pairs; 1: the validation pairs; 2: the precision pairs -- [count][2], p < q, as drawn
uint64_t svih_sbm_npairs(const svih_sbm *b, int32_t which) {
  return (which == 0 ? b->eng->heldout_pairs() : which == 1 ? b->eng->validation_pairs() : b->eng->precision_pairs()).size() / 2;
}
const uint32_t *svih_sbm_pairs(const svih_sbm *b, int32_t which) {
  return (which == 0 ? b->eng->heldout_pairs() : which == 1 ? b->eng->validation_pairs() : b->eng->precision_pairs()).data();
}
uint64_t svih_sbm_nrows(const svih_sbm *b) { return b->eng->rows().size() / 8; }
const double *svih_sbm_rows(const svih_sbm *b) { return b->eng->rows().data(); }
int svih_sbm_sweep(svih_sbm *b) { return svils_rc([&] { b->eng->sweep(); return 0; }); }   // < 0: a svils_error of the device backend
int svih_sbm_set_state(svih_sbm *b, const double *phi, const double *gamma, const double *lambda) {
  return svils_rc([&] { b->eng->set_state(phi, gamma, lambda); return 0; });
}
const uint32_t *svih_sbm_edges(const svih_sbm *b) { return &b->net->edges()[0].first; }
uint32_t svih_sbm_ones(const svih_sbm *b) { return b->net->ones(); }

// tests: how many of `count` values differ between the writers' fixed-point formatter (fixedfmt.hh) and printf's
// "%.5f" / "%.3f" -- the values come as they are, the test chooses them
uint64_t svih_fixed_format_mismatches(const double *v, uint64_t count) {
  uint64_t bad = 0;
  std::string a;
  char tmp[400];
  for (uint64_t i = 0; i < count; ++i) {
    a.clear();
    append_fixed<5>(a, v[i], '\t');
    snprintf(tmp, sizeof tmp, "%.5f\t", v[i]);
    bad += a != tmp;
    a.clear();
    append_fixed<3>(a, v[i], '\n');
    snprintf(tmp, sizeof tmp, "%.3f\n", v[i]);
    bad += a != tmp;
  }
  return bad;
}

// -findk through the host driver (findk.hh) in library mode: nothing is written to disk, the device work goes through the
// svils_findk_* entry points.  svih_findk_step: 0 = an iteration with groups, 1 = the stop rule fired, 2 = the loop is over.
struct svih_findk {
  std::unique_ptr<Env> env;
  std::unique_ptr<Network> net;
  std::unique_ptr<FindK> fk;
};

static svih_findk *make_findk(const svih_options *o, const char *path, const int32_t *pairs, uint64_t nlines, int device) {
  Env::Args a;
  a.n = o->n;
  a.k = o->k;
  a.findk = true;
  a.rand_seed = o->seed;
  a.hol_ratio = o->heldout_ratio;
  a.link_thresh = o->link_thresh;
  a.accuracy = o->accuracy != 0;
  a.device = device;
  a.write_files = false;
  svih_findk *s = new svih_findk();
  s->env.reset(new Env(a));
  s->net.reset(new Network(*s->env));
  if (path) {
    if (s->net->read(path) < 0) { delete s; return nullptr; }
  } else {
    s->net->read_pairs(pairs, nlines);
  }
  s->env->n = s->net->n() - s->net->singles();   // src/main.cc:291
  if (svils_rc([&] { s->fk.reset(new FindK(*s->env, *s->net)); return 0; })) {   // svils_last_error() keeps the library's text
    delete s;
    return nullptr;
  }
  return s;
}

svih_findk *svih_findk_from_file(const char *path, const svih_options *o, int device) { return make_findk(o, path, nullptr, 0, device); }
svih_findk *svih_findk_from_pairs(const int32_t *pairs, uint64_t nlines, const svih_options *o, int device) {
  return make_findk(o, nullptr, pairs, nlines, device);
}
void svih_findk_free(svih_findk *s) { delete s; }
int svih_findk_step(svih_findk *s) { return svils_rc([&] { return s->fk->step(); }); }
uint32_t svih_findk_n(const svih_findk *s) { return s->fk->n(); }
uint32_t svih_findk_iter(const svih_findk *s) { return s->fk->iter(); }
uint32_t svih_findk_unlikely(const svih_findk *s) { return s->fk->unlikely(); }
uint32_t svih_findk_npad(const svih_findk *s) { return s->fk->last_npad(); }
double svih_findk_pad_seconds(const svih_findk *s) { return s->fk->pad_seconds(); }
double svih_findk_training_ll(const svih_findk *s) { return s->fk->training_ll(); }
uint64_t svih_findk_nheldout(const svih_findk *s) { return s->fk->heldout_pairs().size() / 3; }
const uint32_t *svih_findk_heldout(const svih_findk *s) { return s->fk->heldout_pairs().data(); }
const uint32_t *svih_findk_seq2id(const svih_findk *s) { return s->net->seq2id().data(); }
void svih_findk_row(const svih_findk *s, double *row11) { memcpy(row11, s->fk->last_row(), 11 * sizeof(double)); }
void svih_findk_state(const svih_findk *s, uint32_t *labels, double *values, uint32_t *masks) {
  const FindK &f = *s->fk;
  if (labels) memcpy(labels, f.labels().data(), f.labels().size() * sizeof(uint32_t));
  if (values) memcpy(values, f.values().data(), f.values().size() * sizeof(double));
  if (masks) {
    if (f.masks().empty()) memset(masks, 0, (size_t)f.n() * sizeof(uint32_t));
    else memcpy(masks, f.masks().data(), f.masks().size() * sizeof(uint32_t));
  }
}
int svih_findk_timing(const svih_findk *s, double *ms4) { return svils_findk_get_timing(s->fk->handle(), ms4); }

}  // extern "C"
