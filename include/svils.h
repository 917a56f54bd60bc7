/*
 * svils.h -- C ABI of the MI355X link-sampling sweep engine (libsvils.so).
 *
 * The reference (premgopalan/svinet) has no plugin/FFI boundary: its only seam
 * for this path is the C++ class used at src/main.cc:337-342
 *
 *     LinkSampling ls(env, network);   // src/linksampling.cc:5-155
 *     ls.infer();                      // src/linksampling.cc:556-790
 *
 * This header is the boundary a maintainer would bind in its place: the host
 * keeps parsing, RNG, initialisation and file formats; the library owns the
 * device-resident state and runs the body of infer()'s `while (1)` loop
 * (phi pass :605-725, compute_mean_indicators :526-545, s3 pass :731-746,
 * lambda/swap/set_dir_exp/prune :748-761, validation_likelihood :966-1050
 * including its stop rule and annealing switch) as HIP kernels for gfx950.
 *
 * Conventions: plain C, no exceptions cross the boundary, every function
 * returns 0 on success or a negative svils_error; svils_last_error() gives
 * the text for the calling thread.  A handle is not thread-safe.  The caller
 * keeps ownership of every host buffer (copied in/out).  Indices are
 * uint32_t, reals are IEEE double, matrices are flat row-major with leading
 * dimension = number of columns.  There is NO CPU fallback: creating a handle
 * without a usable HIP device fails with SVILS_ERR_DEVICE.
 */
#ifndef SVILS_H
#define SVILS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SVILS_ABI_VERSION 8   /* 3: svils_config gained k_begin / k_total (K-sharded handles); 4: svils_comm_info; 5: community tags;
                                 6: work-balanced node blocks (svils_balance_node_blocks / svils_set_node_blocks), the node-block sweep
                                    with ONE row exchange (SVILS_PHASE_B_LIGHT / SVILS_PHASE_EXPAND_ALL, SVILS_BUF_GSTAGE);
                                 7: k up to SVILS_MAX_K_TOTAL (column-tiled handles above SVILS_MAX_K; K-sharded k_total up to it),
                                    getters that do not wait behind a stop the caller has seen ("After the stop");
                                 8: svils_init_gamma (init_gamma2 on the device); svils_set_option / svils_get_option / svils_option_table (every tunable in one documented table; nothing
                                    on a sweep path reads the environment); svils_gather_communities ends the no-wait window of "After the stop";
                                    (additive, same version) svils_link_prob / svils_predict_links: link prediction from the state;
                                    (additive, same version) svils_findk_*: -findk, the estimate of the number of communities;
                                    (additive, same version) svils_batch_*: -batch-gpu, all-pairs batch inference;
                                    (additive, same version) svils_batch_step_node / svils_batch_step_pairs: -rnode / -rpair, sampled-pair steps;
                                    (additive, same version) svils_batch_step_star / svils_batch_set_star_chain / svils_batch_get_expectations: -infset, informative-set steps;
                                    (additive, same version) svils_batch_elbo / svils_batch_set_elbo_tiles: -logl, the variational lower bound;
                                    (additive, same version) svils_batch_step_strat / svils_batch_get_lag: -snode, stratified random node steps;
                                    (additive, same version) svils_orig_*: -orig, the full K x K blockmodel over all ordered pairs;
                                    (additive, same version) svils_sbm_*: -single, the single-membership stochastic blockmodel;
                                    (additive, same version) svils_sbmelbo / svils_sbmelbo_get_timing: -single-logl, its variational lower bound;
                                    (additive, same version) svils_lc_*: -gml / -lcstats, the link communities of a fitted model;
                                    (additive, same version) svils_ppc_*: -ppc / -gen, networks drawn from a model and their statistics;
                                    (additive, same version) svils_ppc_hops / svils_ppc_get_hop*: -ppc-hops, the exact hop plot and components;
                                    (additive, same version) svils_ppc_set_params_orig / svils_ppc_get_blocks: -ppc-orig, the same checks of a K x K blockmodel;
                                    (additive, same version) svils_nbr_score / svils_nbr_rank: common-neighbour, Adamic-Adar and
                                    resource-allocation scores of pairs, the model-free baselines of svils_rank_links */

typedef enum {
  SVILS_OK = 0,
  SVILS_ERR_ARG = -1,      /* bad argument / call order                     */
  SVILS_ERR_DEVICE = -2,   /* no HIP device, HIP runtime error              */
  SVILS_ERR_NOMEM = -3,    /* host or device allocation failed              */
  SVILS_ERR_UNSUPPORTED = -4 /* e.g. k > SVILS_MAX_K_TOTAL                   */
} svils_error;

#define SVILS_MAX_K 2048         /* columns ONE set of kernels holds: a whole-row handle up to here, a K-sharded slice up to here */
/* k above SVILS_MAX_K (the reference has no limit short of its 16-bit community ids, src/linksampling.cc:635): svils_create
 * builds a COLUMN-TILED handle -- ceil(k / SVILS_MAX_K) slices of every row on the one device, the K-sharded layout with all
 * its "ranks" on one stream and their four exchanges summed in place.  Same results as a whole-row handle to rounding.  What
 * such a handle offers: svils_set_graph / set_validation / set_state (graph before the first sweep or likelihood row) /
 * sweep / synchronize / get_control / set_control / validation_row / get_rows / get_state / get_communities /
 * get_community_tags / get_sweep_stats / destroy; everything else (reports, test set, mini-batch steps, node blocks,
 * timing) answers SVILS_ERR_UNSUPPORTED.  Across GPUs the same k goes through K-sharded handles (k_total up to
 * SVILS_MAX_K_TOTAL, at most SVILS_MAX_K columns per rank). */
#define SVILS_MAX_K_TOTAL 65535
#define SVILS_MAX_TILES 32

typedef struct svils_handle svils_handle;

/* Everything the sweep needs from Env / Network / the LinkSampling ctor.
 * Replaces the Env& / Network& arguments of LinkSampling::LinkSampling
 * (src/linksampling.cc:5-33) for the fields the loop actually reads. */
typedef struct {
  uint32_t n;             /* env.n after singleton removal, src/main.cc:291          */
  uint32_t k;             /* env.k                                                   */
  uint64_t ones;          /* network.ones(): ALL links incl. held-out (anneal scale,
                             src/linksampling.cc:541-542)                            */
  double alpha;           /* env.alpha = 1/k, src/env.hh:344                         */
  double eta0, eta1;      /* Network::set_env_variables, src/network.cc:222-251      */
  double epsilon;         /* env.epsilon = 1e-30, src/env.hh:395                     */
  double link_thresh;     /* -link-thresh, src/linksampling.cc:672,708               */
  uint32_t lt_min_deg;    /* -lt-min-deg,  src/linksampling.cc:676-679,712-715       */
  uint32_t reportfreq;    /* env.reportfreq (1 under -link-sampling)                 */
  int32_t use_validation_stop; /* 0 with -no-stop, src/linksampling.cc:1044-1048     */
  double ones_prob;       /* _ones_prob,  src/linksampling.cc:49                     */
  double zeros_prob;      /* _zeros_prob, src/linksampling.cc:50                     */
  int32_t device;         /* HIP device ordinal                                      */
  /* node-block ownership for multi-GPU runs (one process per GPU): this
   * handle computes rows [node_begin, node_end); 0,n for a single GPU.     */
  uint32_t node_begin, node_end;
  /* rows allocated for the replicated n-by-k arrays (>= n; 0 = n).  A caller
   * that all-gathers equal node blocks sets world_size * block_rows.        */
  uint32_t n_alloc;
  /* the active-set branch is taken when _iter > sparse_after_iter: the constant 1000 of
   * src/linksampling.cc:634 (svils_config_default).  The revision that produced the runs shipped
   * under example/ behaved like 0, which is how the tests reproduce them. */
  int32_t sparse_after_iter;
  /* K-sharded handles (multi-GPU layout of DESIGN.md section 6): k_total != 0 means this handle holds the
   * columns [k_begin, k_begin + k) of k_total communities for ALL n nodes; alpha stays 1/k_total,
   * gamma / lambda are passed and returned as that column slice.  0: the handle holds every column. */
  uint32_t k_begin, k_total;
} svils_config;

/* fills the reference's defaults for a given n,k (alpha=1/k, eta=1,1, ...) */
int svils_config_default(svils_config *cfg, uint32_t n, uint32_t k);

int svils_create(const svils_config *cfg, svils_handle **out);
int svils_destroy(svils_handle *h);

/* Training links exactly as LinkSampling::assign_training_links leaves them
 * (src/linksampling.cc:493-523): [nlinks][2], p < q, sorted by p then by
 * adjacency order.  _training_links[p] (= 2 * training degree, quirk Q3) is
 * derived from the list.  Builds the device CSR. */
int svils_set_graph(svils_handle *h, const uint32_t *links, uint64_t nlinks);

/* Optional: capture the hipGraphs svils_sweep replays (1, 4, 8, 16 ... sweeps, up to max_sweeps) during set-up instead of
 * in the middle of the run (by itself svils_sweep launches eagerly until a handle has run 128 sweeps: a capture costs more
 * than a short run).  After svils_set_graph / svils_set_validation / svils_set_state.  The drop-in binary calls it from the
 * LinkSampling constructor, so that its default run -- 31 sweeps on ca-AstroPh -- replays graphs from the third chunk on. */
int svils_prepare_graphs(svils_handle *h, uint32_t max_sweeps);

/* Held-out pairs in std::map<Edge,bool> order (src/linksampling.cc:974-992):
 * [nv][3] = (p, q, y).  nv == 0 disables the likelihood/stop rule. */
int svils_set_validation(svils_handle *h, const uint32_t *pairs_y, uint64_t nv);

/* Test pairs of -load-test in std::map<Edge,bool> order (LinkSampling::load_test, src/linksampling.cc:1417-1450;
 * test_likelihood, :1147-1182): [nt][3] = (p, q, y), y = network.y(p, q).  Every report that does not end the run
 * (the stopping sweep leaves validation_likelihood through do_on_stop + exit, before test_likelihood is reached,
 * :777-781) also records a TEST row with the columns of the validation row, under the same row number; fetch them
 * with svils_get_test_rows or a report.  The caller has already taken the pairs out of the training links
 * (edge_ok, src/linksampling.hh:296-305).  Sweeps of a handle with a test set run as four launches (the three-launch
 * form of K <= 32 defers the stop rule to the next launch, too late to decide whether the test row exists).
 * nt == 0 removes the set.  Not for K-sharded handles.  Test rows share the row numbers of the validation rows: a handle
 * without a validation set (svils_set_validation with nv == 0) records neither (the reference always has one on this
 * path: its constructor samples it before anything else, src/linksampling.cc:84-109).  Calling it again re-uses the
 * device buffers (they grow when a larger set arrives; nothing accumulates). */
int svils_set_test(svils_handle *h, const uint32_t *pairs_y, uint64_t nt);
/* out[count][10]: the test rows of reports [first, first + count) (numbered like the validation rows); a report that
 * recorded none (the stopping sweep) reads as NaN.  Synchronises. */
int svils_get_test_rows(svils_handle *h, uint32_t first, uint32_t count, double *rows);

/* gamma [n][k], lambda [k][2] after init_gamma2/init_lambda (or -load);
 * converged [n] or NULL (= all 0, as at the top of infer(), :559).
 * Computes Elogpi / Elogbeta (set_dir_exp, src/linksampling.hh:170-187). */
int svils_set_state(svils_handle *h, const double *gamma, const double *lambda,
                    const uint32_t *converged);

/* init_gamma2 (src/linksampling.cc:374-401) ON THE DEVICE, bit for bit: instead of drawing the E x k uniforms on the host, adding
 * them into an n x k array and uploading it (svils_set_state), the caller hands over where its MT19937 stream stands and the
 * library regenerates the draws, normalises them per link and adds them into the gamma rows in the reference's order.
 *   edges      [nedges][2], p < q, EVERY link (held-out ones included) in the order the reference's loop visits them: p ascending,
 *              then the order of p's adjacency list -- link j consumes outputs [j k, (j + 1) k) of the stream
 *   mt_states  [nstreams][624] MT19937 states in canonical form (the next output is the first word of the next twist of the
 *              state; gsl_rng's mt[] with mti == 624): state s stands outputs_per_stream * s outputs behind state 0, which stands
 *              where the reference's generator stands when init_gamma2 starts (after the validation sampler's draws).
 *              host/mtjump.hh computes them by jump-ahead; streams x outputs_per_stream must cover nedges * k exactly once.
 *   lambda     [k][2] as for svils_set_state (init_lambda, src/linksampling.cc:364-372); the converged flags are zeroed.
 * Any handle: a node-block handle holds every row anyway; a K-sharded one (k_total columns drawn per link, its slice kept,
 * lambda = the slice's rows; svils_ksh_init_state follows as after svils_set_state) regenerates the whole stream on every
 * rank -- what a rank saves is the host's 2.9 s and its n x k_total array.  Needs 4 * nedges * k_total bytes of device scratch
 * for the duration of the call (24 GB at n = 1e6, k = 512; SVILS_ERR_NOMEM if it is not there: upload the state instead).
 * Replaces 2.9 s of host work + a 4.1 GB upload by ~0.1 s of host work (the states) + ~30 ms of device work at that size. */
int svils_init_gamma(svils_handle *h, const uint32_t *edges, uint64_t nedges, const uint32_t *mt_states, uint64_t nstreams,
                     uint64_t outputs_per_stream, const double *lambda);

/* Loop-carried scalars of infer()/validation_likelihood(). */
typedef struct {
  uint32_t iter;          /* _iter                                               */
  int32_t annealing;      /* _annealing_phase                                    */
  int32_t write_comm;     /* write_comm for the NEXT sweep                       */
  int32_t nh;             /* _nh                                                 */
  double prev_h;          /* _prev_h                                             */
  double max_h;           /* _max_h                                              */
  int32_t stopped;        /* 1 once the stop rule fired with use_validation_stop;
                             further sweeps are no-ops and the state is the one
                             do_on_stop() would have saved                       */
  int32_t why;            /* last `why` of validation_likelihood (:1007-1027)    */
  uint32_t sweeps_done;   /* sweeps executed since create                        */
  uint32_t rows;          /* validation rows recorded since create               */
  uint64_t links_dense, links_sparse, links_shortcut; /* c, d and the one-converged
                             count of the last sweep (:602,:726)                 */
} svils_control;

/* After the stop: once a control block or a report that says `stopped` has reached the caller (svils_get_control,
 * svils_report_fetch*), svils_get_control / get_state / get_rows / get_test_rows / get_communities / get_community_tags
 * no longer wait for the stream: whatever a pipelined caller still has in flight behind the stopping sweep are launches
 * that return at once, and the state they would wait for is already final. */
int svils_get_control(svils_handle *h, svils_control *out);   /* synchronises (but see "After the stop") */
/* only iter, annealing, write_comm, nh, prev_h, max_h are taken from `in` */
int svils_set_control(svils_handle *h, const svils_control *in);

/* validation_likelihood() on the current state WITHOUT the stop rule: the row
 * the constructor writes (src/linksampling.cc:149-150).
 * row[10] = iter, s/k, k, mean0, k0, mean1, k1, zeros_prob*mean0,
 *           ones_prob*mean1, a   (the columns of :996-1001 minus duration). */
int svils_validation_row(svils_handle *h, double *row10);

/* Enqueue `nsweeps` iterations of the loop body; asynchronous.  The stop
 * rule, the annealing switch and _iter++ run on the device, so no host
 * round trip is needed between sweeps.  At most 65536 * reportfreq sweeps per
 * call: the likelihood rows go to a ring of 65536 entries that the host drains
 * with svils_get_rows between calls. */
int svils_sweep(svils_handle *h, uint32_t nsweeps);
int svils_synchronize(svils_handle *h);

/* phases of a sweep / mini-batch step between exchange points (see "multi-GPU hooks" below) */
typedef enum { SVILS_PHASE_A = 0, SVILS_PHASE_B, SVILS_PHASE_C, SVILS_PHASE_D, SVILS_PHASE_EXPAND,
               SVILS_PHASE_B_LIGHT = 5, SVILS_PHASE_EXPAND_ALL = 6 } svils_phase;

/* ---- mini-batch mode (an ADDITION of this build; SURVEY 8f N4, BASELINE north_star) ----
 * The reference revision's -link-sampling loop is a deterministic full sweep with step size 1
 * (src/linksampling.cc:556-790); its stochastic engines (MMSBInfer::infer,
 * src/mmsbinfer.cc:564-641) sample node/pair mini-batches and blend with a Robbins-Monro step
 * (tau0 + t)^-kappa, per node and for lambda.  svils_step() is that scheme applied to the
 * link-sampling updates: one step processes the links of a WINDOW of `batch_nodes` consecutive
 * nodes (windows taken in cyclic order -- relabel the nodes randomly for unbiased batches),
 * scales the window sums to estimates of the full sums, and blends gamma rows of the window
 * (per-node step size from the node's own update count) and lambda (step size from the step
 * number).  With batch_nodes = 0 (all nodes) and kappa = 0 a step equals a full sweep.
 * Not a parity mode: the reference has no counterpart to compare against. */
typedef struct {
  uint32_t batch_nodes;   /* nodes per mini-batch; 0 = all nodes */
  /* step sizes, the reference's four constants (src/env.hh:399-408: 1024, 0.5, 1024, 0.9):
   * a node updated c times so far moves by (node_tau0 + c)^-node_kappa, lambda at step t by
   * (tau0 + t)^-kappa; tau >= 1, kappa in [0, 1], kappa = 0 = no damping */
  double node_tau0, node_kappa;
  double tau0, kappa;
  uint64_t seed;          /* offset of the first window in the cyclic order */
  /* node-block shards (svils_config node_begin/node_end): nodes per rank block (= n_alloc / world);
   * 0 on a single handle.  Every rank then takes the window at the SAME offset inside its own block,
   * so a global mini-batch is world x batch_nodes nodes; drive it with svils_step_phase(). */
  uint32_t shard_block;
} svils_stochastic;
void svils_stochastic_default(svils_stochastic *cfg, uint32_t batch_nodes);
/* Call after svils_create; allocates the extra accumulator. */
int svils_set_stochastic(svils_handle *h, const svils_stochastic *cfg);
/* Enqueue `nsteps` mini-batch steps; asynchronous; every step advances _iter, writes a
 * likelihood row when _iter % reportfreq == 0 and runs the stop rule, exactly as a sweep does. */
int svils_step(svils_handle *h, uint32_t nsteps);
/* One mini-batch step split at its exchange points, for node-block shards (one process per GPU):
 * A -> all-reduce SVILS_BUF_KVEC_A -> B -> all-gather, for every rank's window, the rows of
 * SVILS_BUF_GAMMA and SVILS_BUF_MPHI and the flag buffers -> EXPAND (Elogpi of the other ranks' window
 * rows from the gathered gamma) -> C -> all-reduce SVILS_BUF_KVEC_C -> D.  Phase A opens the step,
 * phase D closes it.  svils_step_window gives the window of the open (or next) step relative to a
 * rank's block: rows [r*shard_block + begin, r*shard_block + end) for every rank r. */
int svils_step_phase(svils_handle *h, svils_phase phase);
int svils_step_window(svils_handle *h, uint32_t *begin, uint32_t *end);

/* ---- pipelined reports --------------------------------------------------------------------------
 * The reference's loop reports after every sweep under -link-sampling (rfreq = 1, src/main.cc:149-153): a likelihood
 * row, max.txt, communities.txt (src/linksampling.cc:777-786).  Fetching that with svils_get_control / svils_get_rows /
 * svils_get_communities costs a stream synchronisation per report, i.e. per sweep.  A REPORT is the same data as a
 * snapshot taken in stream order: svils_report_enqueue() puts, behind the sweeps enqueued so far, one launch that packs
 * the control block, the likelihood rows [row_first, row_first + row_count) and (with_communities != 0) the community
 * bitmask of the last tagging sweep into a staging slot; a copy stream takes the slot to pinned host memory while the
 * compute stream goes on with the next sweeps.  The host collects it later (svils_report_fetch blocks until it has
 * landed; svils_report_ready does not block).  The caller names the rows because it knows them without asking the
 * device: every sweep whose _iter becomes a multiple of reportfreq records one (fewer only after the stop rule fired --
 * the fetched control block says how many really exist).  At most SVILS_REPORT_SLOTS reports may be outstanding, each
 * of at most SVILS_REPORT_MAX_ROWS rows.  Whole-graph handles only (a sharded run gathers its tags collectively). */
#define SVILS_REPORT_SLOTS 4
#define SVILS_REPORT_MAX_ROWS 64
int svils_report_enqueue(svils_handle *h, uint32_t row_first, uint32_t row_count, int with_communities, int *ticket);
int svils_report_ready(svils_handle *h, int ticket);     /* 1 = landed, 0 = not yet, < 0 = error */
/* ctrl: as svils_get_control at the snapshot; rows: [row_count][10], *nrows = how many of them exist
 * (min(ctrl.rows, row_first + row_count) - row_first); member: [n][k] as svils_get_communities, or NULL.  Frees the slot. */
int svils_report_fetch(svils_handle *h, int ticket, svils_control *ctrl, double *rows, uint32_t *nrows, uint8_t *member);
/* The communities of a report as (node, community) PAIRS -- what communities.txt is made of (src/linksampling.cc:882-917
 * walks the map community -> members) -- instead of the n x k byte matrix (n = 1e6, k = 512: 512 MB and a pass over it per
 * report, against ~1e6 pairs).  tags[2i] = node, tags[2i+1] = community, by ascending node (a node's communities in no
 * particular order).  svils_report_tag_count blocks until the report has landed and says how many pairs it holds (the slot
 * is kept); svils_report_fetch_tags is svils_report_fetch with the pairs in place of `member`: `cap` = room in pairs,
 * *ntags = pairs that exist; if they do not fit nothing is freed and SVILS_ERR_ARG comes back. */
int svils_report_tag_count(svils_handle *h, int ticket, uint64_t *ntags);
int svils_report_fetch_tags(svils_handle *h, int ticket, svils_control *ctrl, double *rows, uint32_t *nrows,
                            uint32_t *tags, uint64_t cap, uint64_t *ntags);
/* the TEST rows of the same report (svils_set_test): test_rows [row_count][10]; call it BEFORE svils_report_fetch (which
 * frees the slot); blocks until the report has landed.  *ntest = rows that exist: one per validation row, minus the one
 * of the stopping sweep. */
int svils_report_test_rows(svils_handle *h, int ticket, double *test_rows, uint32_t *ntest);

/* rows recorded by the in-loop validation_likelihood(): copies rows
 * [first, first+count) (as numbered since create) into out[count][10]. */
int svils_get_rows(svils_handle *h, uint32_t first, uint32_t count, double *rows);

/* save_model() inputs (src/linksampling.cc:804-837): gamma [n][k],
 * lambda [k][2]; any pointer may be NULL. */
int svils_get_state(svils_handle *h, double *gamma, double *lambda, uint32_t *converged);

/* communities of the last tagging sweep (src/linksampling.cc:704-717,882-917):
 * member[n][k] bytes, 1 = node p belongs on line k of communities.txt. */
int svils_get_communities(svils_handle *h, uint8_t *member);
/* the same as (node, community) pairs (see svils_report_fetch_tags); tags == NULL (cap 0): only the count */
int svils_get_community_tags(svils_handle *h, uint32_t *tags, uint64_t cap, uint64_t *ntags);

/* Derived device arrays for parity tests and integrators:
 * which = 0 Elogpi [n][k], 1 Elogbeta [k][2], 2 mphi [n][k],
 *         3 active_comms [n] (uint32), 4 training_links [n] (double),
 *         6 exp(Elogpi) [n][k] as the product-form phi pass reads it (handles on which option lpl_product reads 1). */
int svils_get_aux(svils_handle *h, int which, void *out);

/* ---- link prediction from the current state (an ADDITION of ABI 8; nothing on the sweep path changes) --------------------
 * link_prob(p, q) = sum_z pi_pz pi_qz beta_z, the reference's LinkSampling::link_prob (src/linksampling.hh:240-256) with
 * pi_p = gamma_p / sum_k gamma_pk (estimate_pi, :205-214) and beta_z = lambda_z0 / (lambda_z0 + lambda_z1)
 * (estimate_bernoulli_rate, :217-225; gsl_ran_bernoulli_pdf(1, u) = u).  The reference wires this quantity only to dead code:
 * auc() / biased_auc() / uniform_auc() (src/linksampling.cc:855-877, 1185-1226) sit behind create_test_precision_sets, which
 * its main.cc never sets, and behind load_test_sets(), which nothing calls.  For y = 1 the held-out likelihood already uses it:
 * edge_likelihood (:259-294) is log(max(link_prob, 1e-30)).
 * The calls enqueue on the handle's stream behind the sweeps already enqueued and synchronise before returning; they read
 * gamma, lambda and the training CSR and write nothing a sweep reads (a handle whose stop rule has fired and a mini-batch
 * handle between steps work the same way).  Device scratch is allocated on first use and freed by svils_destroy: at most
 * ~0.5 GB (queries go through in internal batches of 8192: 384 MB of partial top-k heaps, 64 MB of query rows, 24 MB of
 * results; pairs in batches of 2^20: 24 MB) plus 8 bytes per node and 4 bytes per CSR entry (a copy of the training CSR
 * with every row sorted, built on first use; the graph of a handle never changes).  Results are bitwise deterministic, and
 * a query's row does not depend on which other nodes are in the same call.
 * SVILS_ERR_ARG: no graph or state, a node id >= n, a pair with p == q, topk == 0 or > SVILS_PREDICT_MAX_TOPK.
 * SVILS_ERR_UNSUPPORTED: column-tiled handles (k > SVILS_MAX_K), K-sharded handles (k_total != 0), node-block handles. */
#define SVILS_PREDICT_MAX_TOPK 256
/* link_prob of pairs[npairs][2] (p != q, both < n) -> prob[npairs], in the reference's order of operations */
int svils_link_prob(svils_handle *h, const uint32_t *pairs, uint64_t npairs, double *prob);
/* The top-k links of each query node: nodes[nnodes] (NULL = all n nodes; nnodes is then 0 or n) -> ids[nnodes][topk],
 * scores[nnodes][topk].  Candidates of p: every node except p itself and p's training neighbours (held-out pairs ARE
 * candidates: finding them is the point).  Order: score descending, ties by ascending node id.  A node with fewer than topk
 * candidates has its remaining slots filled with id UINT32_MAX and score -1.0.  The scores are link_prob computed as
 * (sum_z (gamma_pz / sum gamma_p) beta_z gamma_qz) / sum gamma_q on the matrix cores (fp64), within a few ulps of
 * svils_link_prob's. */
int svils_predict_links(svils_handle *h, const uint32_t *nodes, uint32_t nnodes, uint32_t topk, uint32_t *ids, double *scores);
/* For every directed pair (p, q), pairs[npairs][2]: where q stands among the candidates of p.  Candidates of p are exactly
 * those of svils_predict_links: every node except p and p's training neighbours.  With s = the score svils_predict_links
 * computes for (p, q):
 *   above[i] = #{candidates c != q : score(p,c) >  s}
 *   tied[i]  = #{candidates c != q : score(p,c) == s}
 *   ncand[i] = #{candidates c != q}
 *   score[i] = s
 * q need not itself be a candidate (a training neighbour of p is ranked against the same set).  Any output pointer may be
 * NULL.  s and the scores it is compared with come from one device function on the matrix cores: score[i] is bitwise the
 * score svils_predict_links lists for q, q ties exactly with itself, and the counts agree exactly with those lists (q at
 * place j of p's list has above <= j <= above + tied).  A pair's result does not depend on which other pairs are in the call;
 * the counts of the candidate chunks are combined with integer atomics.  One query row per pair, in internal batches of 8192:
 * the call shares the query rows and the sorted CSR copy with svils_predict_links, keeps no heaps, and grows the scratch by
 * 24 bytes per row of a batch (q, s and the three counters: under 200 KB).
 * SVILS_ERR_ARG / SVILS_ERR_UNSUPPORTED: as for svils_link_prob. */
int svils_rank_links(svils_handle *h, const uint32_t *pairs, uint64_t npairs, uint32_t *above, uint32_t *tied, uint32_t *ncand,
                     double *score);

/* ---- neighbourhood scores: the model-free baselines of link ranks (an ADDITION of ABI 8; nothing on the sweep path changes) ----
 * score(p, q) = sum over the common TRAINING neighbours z of p and q, in ascending z, of w[deg z], deg = training degree:
 *   SVILS_NBR_CN  w = 1                  the number of common neighbours
 *   SVILS_NBR_AA  w = 1 / log(deg z)     Adamic-Adar: the reference's -adamic-adar (FastAMM::compute_adamic_adar_score,
 *                                        src/fastamm.cc:1486-1575), wired there to engines this build does not carry
 *   SVILS_NBR_RA  w = 1 / deg z          resource allocation
 * w is a table over the degrees 0 .. the largest training degree, w[0] = w[1] = 0 (a common neighbour of p != q has degree
 * >= 2), computed ON THE HOST as 1.0 / std::log((double)d) and 1.0 / (double)d, once per handle and measure, and uploaded:
 * a score is bitwise the sequential sum, in ascending z, of those doubles, so that equal scores are ties a caller can
 * restate.  CN scores and every count are exact integers.
 * The contract is that of svils_link_prob / svils_rank_links: the calls enqueue on the handle's stream behind what is there
 * and synchronise; they read the training CSR only and need a graph but NO state; any output pointer may be NULL; results
 * are bitwise deterministic and a pair's result does not depend on the other pairs of the call, on their order or on the
 * workgroup that served it.  Device scratch, allocated on first use and freed by svils_destroy: the sorted CSR copy shared
 * with svils_predict_links (4 bytes per CSR entry), 8 bytes per degree up to the largest for every measure used, 36 bytes
 * per pair of an internal batch of 65536 (2.4 MB), and for svils_nbr_rank one bitmap of n bits per workgroup, four
 * workgroups per CU: n / 8 x 1024 bytes on 256 CUs (128 MB at n = 10^6).
 * SVILS_ERR_ARG: a null handle, no graph, a node id >= n, a pair with p == q, an unknown measure.
 * SVILS_ERR_UNSUPPORTED: column-tiled handles (k > SVILS_MAX_K), K-sharded handles (k_total != 0), node-block handles. */
typedef enum { SVILS_NBR_CN = 0, SVILS_NBR_AA = 1, SVILS_NBR_RA = 2 } svils_nbr_measure;
/* pairs[npairs][2] (p != q, both < n) -> score[npairs], common[npairs] = the number of common training neighbours */
int svils_nbr_score(svils_handle *h, int measure, const uint32_t *pairs, uint64_t npairs, double *score, uint32_t *common);
/* svils_rank_links with this score in place of link_prob: for every directed pair (p, q), over the candidates c != q of p
 * (every node except p and p's training neighbours; q may itself be a training neighbour)
 *   above[i] = #{c : score(p,c) > s}, tied[i] = #{c : score(p,c) == s}, ncand[i] = #{c}, score[i] = s = score(p, q),
 * s bitwise that of svils_nbr_score.  Only the candidates two steps from p can score above zero: they are visited and
 * scored by the device function that computes s; the others score exactly 0 and are counted (they tie when s == 0). */
int svils_nbr_rank(svils_handle *h, int measure, const uint32_t *pairs, uint64_t npairs, uint32_t *above, uint32_t *tied,
                   uint32_t *ncand, double *score);

/* Evaluate the kernels' own special functions on a plain array (unit tests):
 * which = 0 digamma(x) [stands for gsl_sf_psi], 1 exp(x) for x <= 0, 2 1/x, 3 ln(x) for x >= 1. */
int svils_debug_eval(svils_handle *h, int which, const double *in, double *out, uint32_t n);

/* ---- measurement --------------------------------------------------------- */
enum {
  SVILS_KERNEL_PHI = 0, SVILS_KERNEL_REDUCE_SUM, SVILS_KERNEL_FINALIZE, SVILS_KERNEL_S3,
  SVILS_KERNEL_VALIDATION /* part of the tail kernel since ABI 2: never timed */,
  SVILS_KERNEL_REDUCE_S, SVILS_KERNEL_TAIL /* likelihood + lambda + stop rule */,
  SVILS_KERNEL_CLASSIFY /* stand-alone link classification (k <= 32; normally fused into the s3 launch) */,
  SVILS_KERNEL_EXCHANGE /* the RCCL collectives of svils_sweep_sharded */,
  SVILS_KERNEL_COUNT
};
/* mask: bit i set = bracket kernel i with hipEvents on the library's stream */
int svils_enable_timing(svils_handle *h, uint32_t kernel_mask);
/* sample only every `period`-th sweep of a svils_sweep() call (default 1 = every sweep): the
 * bracketed sweeps are launched eagerly, the others replay hipGraphs */
int svils_set_timing_period(svils_handle *h, uint32_t period);
/* synchronises; ms[i] = summed duration, launches[i] = launches timed since
 * the last svils_enable_timing call.  Arrays of SVILS_KERNEL_COUNT. */
int svils_get_timing(svils_handle *h, double *ms, uint64_t *launches);
const char *svils_kernel_name(int kernel);
/* How the links of sweeps [first, first+count) (numbered since create) were evaluated
 * (src/linksampling.cc:622-719; the c / d counters of :602,:726): out[count][3] =
 * full softmax, active-set softmax, O(1) shortcut.  The device keeps the last 4096 sweeps. */
int svils_get_sweep_stats(svils_handle *h, uint32_t first, uint32_t count, uint64_t *out);
/* The same three counts summed over exactly those sweeps whose phi launch was bracketed with
 * hipEvents since the last svils_enable_timing call: what the timed launches processed. */
int svils_get_timed_links(svils_handle *h, uint64_t *out3);

/* ---- multi-GPU hooks (one process per GPU; collectives stay with the caller) */
/* The sweep split at its exchange points.  Node-block ownership, whole sweeps (what svils_sweep_sharded issues itself):
 *   A            phi pass over the owned rows                  -> partial `sum[k]` in SVILS_BUF_KVEC_A
 *   B_LIGHT      mean indicators, s1 / s2 partials, tags and the UNSCALED new row of every owned node, written to this
 *                rank's slice of SVILS_BUF_GSTAGE ([world][bmax][ld]: slice r = the rows of rank r's block)
 *   -- exchange 1: all-reduce(SUM) KVEC_A; all-gather of the GSTAGE slices (in place: the send block IS slice `rank`)
 *   EXPAND_ALL   every row, owned or not: annealing scale ones / sum[k], gamma, Elogpi (digamma), the mean indicators of
 *                the other blocks m = (row - alpha) / (n - 1), prune() flags -- computed by every rank from the same
 *                bytes, so flags never cross the links and ONE n-by-k array does
 *   C            s3 pass over this rank's share of the links   -> SVILS_BUF_KVEC_C (s1, s2, s3)
 *   -- exchange 2: all-reduce(SUM) KVEC_C
 *   D            lambda, likelihood, stop rule, annealing switch (replicated)
 * Two exchange points in both phases of a run: the annealing scale is applied behind the row exchange (until ABI 5
 * `sum` had an exchange point of its own while annealing).  Mini-batch steps (svils_step_phase) keep the older split
 * A | B | EXPAND | C | D with the gamma / mphi / packed-flag rows of the windows exchanged in place.
 * svils_sweep() == A,B,C,D with no exchange. */
int svils_sweep_phase(svils_handle *h, svils_phase phase);

/* Node blocks.  Rank r of `world` owns the nodes [bounds[r], bounds[r + 1]); the handle of rank r is created with
 * svils_config.node_begin / node_end = that range.  svils_balance_node_blocks cuts [0, n) so that every block carries
 * the same WORK, not the same number of nodes ("balanced by sum of degree"): cost of a node = its CSR
 * entries (2 per training link it touches) + node_weight (per-node share of the finalise pass in units of one entry;
 * < 0 = the default 0.5).  The reference numbers nodes by first appearance (src/network.cc:10-116), so on its own
 * example graphs the hubs sit at the low ids: equal-count blocks give rank 0 of 8 on ca-AstroPh 2.96 x the mean number
 * of entries.  Pure host code (no device needed); every rank computes the same bounds from the same link list.
 * svils_set_node_blocks declares the blocks of ALL ranks to a handle (bounds[world + 1]; NULL = equal blocks of
 * ceil(n / world) nodes, what svils_comm_init assumes by itself), before or after svils_set_graph, before
 * svils_comm_init.  With caller-given bounds the s3 pass is cut by link count (equal runs of the link list) instead of
 * by node block, and mini-batch steps (which need equal blocks) are refused.  At most 64 ranks. */
int svils_balance_node_blocks(const uint32_t *links, uint64_t nlinks, uint32_t n, int world, double node_weight, uint32_t *bounds);
int svils_set_node_blocks(svils_handle *h, int rank, int world, const uint32_t *bounds);

typedef enum {
  SVILS_BUF_KVEC_A = 0,   /* double[k]   : sum (phase A -> all-reduce SUM)          */
  SVILS_BUF_KVEC_C,       /* double[3k]  : s1,s2,s3 (phase C -> all-reduce SUM)          */
  SVILS_BUF_GAMMA,        /* double[n_pad][ld] rows, all-gather by node block      */
  SVILS_BUF_ELOGPI,       /* double[n_pad][ld]  (re-derived by EXPAND; exchange optional) */
  SVILS_BUF_MPHI,         /* double[n_pad][ld]  (re-derived by EXPAND; exchange optional) */
  SVILS_BUF_CONV,         /* uint32[n_pad] new converged flags                      */
  SVILS_BUF_ACTIVE,       /* uint32[n_pad] active_comms                             */
  SVILS_BUF_AMASK,        /* uint64[n_pad][kw] active-set bitmask                   */
  SVILS_BUF_MEMBER,       /* uint64[n_pad][kw] community bitmask                    */
  SVILS_BUF_XFLAGS,       /* uint32[n_pad][2+2kw] new converged flag, active_comms and active-set
                             bitmask of every row, packed by phase B: all-gather THIS by node block
                             (instead of CONV/ACTIVE/AMASK); PHASE_EXPAND unpacks the others' rows
                             (mini-batch steps only since ABI 6) */
  SVILS_BUF_GSTAGE        /* double[world * bmax][ld]: staging of the row exchange of whole node-block sweeps; slice r
                             (bmax rows, bmax = the largest block) holds the unscaled new rows of rank r's block.
                             row_bytes = ld * 8, bytes = the whole buffer.  Exists once the blocks are declared. */
} svils_buffer;
/* device pointer + geometry of an exchange buffer (valid until destroy) */
int svils_device_buffer(svils_handle *h, svils_buffer which, void **dptr,
                        size_t *bytes, size_t *row_bytes);
/* the hipStream_t the library launches on, as void* */
int svils_stream(svils_handle *h, void **stream);

/* ---- native multi-GPU driver: one process per GPU, RCCL over xGMI ------------------------------
 * The reference has no distributed path; its one reduce analogue is the in-process sum of per-thread
 * partials in MMSBInfer::multithreaded_process (src/mmsbinfer.cc:1770-1827).  Here every process
 * creates its handle on its own GPU with the node block of its rank (svils_config node_begin / node_end =
 * [bounds[rank], bounds[rank + 1]) of svils_balance_node_blocks + svils_set_node_blocks; or, without them, the equal
 * blocks [rank*B, min(n, (rank+1)*B)), B = ceil(n/world) -- mini-batch steps also need n_alloc = world*B) and the
 * library issues the exchanges itself, on the handle's stream, between the phases of a sweep:
 *   phi pass -> light finalise -> {all-reduce(sum), all-gather(unscaled rows)} -> expand (scale, Elogpi, flags of every
 *   row) -> s3 pass -> all-reduce(s1,s2,s3) -> tail (replicated):
 * two exchange points per sweep in both phases of a run, nothing on the host looks at the control block, and runs of
 * sweeps -- collectives included -- replay as hipGraphs under svils_sweep's rule (eager until the handle has run 128
 * sweeps; option sharded_graphs = 0 keeps them eager; a capture that fails once leaves the handle eager).
 * The K-vector all-reduces run on the handle's stream.  When the n-by-k payload is large enough to be pipelined
 * (chunks on a communication stream of their own, each expanded while the next one travels) the row chunks use a
 * SECOND communicator, formed by the same ranks the first time it is needed (rank 0 draws another unique id and
 * broadcasts it over the first one): RCCL serialises the operations of one communicator, so sharing it would put
 * every K-vector all-reduce behind the broadcasts still in flight.
 * librccl is loaded at run time (dlopen) the first time one of these entry points is used. */
#define SVILS_COMM_ID_BYTES 128
/* rank 0: a fresh ncclUniqueId to hand to every rank (any transport: pipe, file, MPI, torch store) */
int svils_comm_unique_id(void *id128);
/* collective over all ranks: ncclCommInitRank on the handle's device */
int svils_comm_init(svils_handle *h, const void *id128, int rank, int world);
/* What the communicator of this handle looks like FROM RCCL'S SIDE (ncclCommCount / ncclCommUserRank /
 * ncclCommCuDevice / ncclGetVersion asked of the library that was bound, not echoed from svils_comm_init's
 * arguments): the evidence a launcher prints to show that N ranks on N devices really formed one communicator. */
typedef struct {
  int32_t nranks;        /* ncclCommCount                                                             */
  int32_t rank;          /* ncclCommUserRank                                                          */
  int32_t device;        /* ncclCommCuDevice: the HIP ordinal RCCL bound the communicator to          */
  int32_t version;       /* ncclGetVersion (e.g. 22203), -1 if the bound library has no such entry    */
  int32_t row_comm;      /* 1 once the second communicator (pipelined row exchange) exists            */
  char pci_bus_id[32];   /* hipDeviceGetPCIBusId of `device`                                          */
  char library[256];     /* path of the shared object the nccl* entry points were bound from          */
} svils_comm_info;
int svils_comm_query(svils_handle *h, svils_comm_info *out);
/* Enqueue `nsweeps` sharded sweeps (asynchronous, like svils_sweep).  Collective. */
int svils_sweep_sharded(svils_handle *h, uint32_t nsweeps);
/* Mini-batch steps (svils_set_stochastic with shard_block = B) over the node-block shards, the exchanges issued
 * here: per step all-reduce(sum) -> broadcasts of every rank's window rows (gamma, mphi, packed flags: world x
 * batch_nodes rows, not n) -> expand -> all-reduce(s1,s2,s3) -- "the K-vector lambda and touched gamma rows at
 * the global step".  svils_comm_init may come before or after svils_set_stochastic.  Collective, asynchronous. */
int svils_step_sharded(svils_handle *h, uint32_t nsteps);
/* all-gather of the community bitmasks before svils_get_communities on a sharded handle.  Collective. */
int svils_gather_communities(svils_handle *h);

/* ---- K-sharded sweeps: one process per GPU, every rank holds a column slice of all rows --------
 * The columns of a row are coupled in four places; each is a buffer of partials
 * that must be SUMmed over the ranks between two phases (tests/test_ksharded_protocol.py is the protocol):
 *   svils_set_state (slices) -> phase KINIT_ROWS -> SUM KSH_ROWX -> phase KINIT_EXPAND        (once)
 *   per sweep: phase KDEN -> SUM KSH_DEN -> phase KPHI -> SUM KSH_ROWX -> phase KFIN -> SUM KSH_Q2
 *              -> phase KLAMBDA -> SUM KSH_VDOT -> phase KSTOP
 * svils_sweep_ksharded does exactly that with RCCL all-reduces on the handle's stream (svils_comm_init
 * first; the node block of a K-sharded handle is [0, n)). */
typedef enum {
  SVILS_KPHASE_DEN = 0, SVILS_KPHASE_PHI = 1, SVILS_KPHASE_FIN = 2, SVILS_KPHASE_LAMBDA = 3, SVILS_KPHASE_STOP = 4,
  SVILS_KPHASE_INIT_ROWS = 5, SVILS_KPHASE_INIT_EXPAND = 6,
  SVILS_KPHASE_DENMAX = 7,  /* log-domain mode only: before DEN, followed by a MAX (not SUM) of SVILS_KSH_DMAX */
  /* not part of a sweep: the partial dot products of the held-out pairs alone, after svils_ksh_init_state or between two
   * sweeps -- what svils_validation_row launches on a K-sharded handle, for callers that SUM SVILS_KSH_VDOT themselves */
  SVILS_KPHASE_VDOT = 8
} svils_kphase;
typedef enum { SVILS_KSH_DEN = 0, SVILS_KSH_ROWX = 1, SVILS_KSH_Q2 = 2, SVILS_KSH_VDOT = 3, SVILS_KSH_DMAX = 4,
               /* link_thresh < 1/2 only (argmax tagging, src/linksampling.cc:704-717, src/matrix.hh:521-532): the lowest
                * column attaining the link's maximum, as a double; exchanged with MIN right after SVILS_KSH_DEN.  Such
                * handles always run the log-domain exchange (the maximum is what SVILS_KSH_DMAX carries). */
               SVILS_KSH_EARG = 5 } svils_ksh_buffer;
int svils_ksweep_phase(svils_handle *h, svils_kphase phase);
/* device pointer and length (doubles) of an exchange buffer */
int svils_ksh_buffer_ptr(svils_handle *h, svils_ksh_buffer which, void **dptr, size_t *ndoubles);
/* Log-domain denominators: the product form of the DEN / PHI phases underflows when max_k x_k < -745 for a link (memberships
 * concentrated on different communities at k_total >~ 740); this mode exchanges the per-link max first (phase DENMAX, MAX of
 * SVILS_KSH_DMAX) and sums e^(x - max).  On by default for k_total > 700.  on = 1 / 0 sets it, on < 0 returns the setting. */
int svils_ksh_log_domain(svils_handle *h, int on);
int svils_ksh_init_state(svils_handle *h);           /* collective: the two INIT phases around their all-reduce */
/* On a K-sharded handle svils_validation_row is collective too (partial dot products of the own columns, SUM of
 * SVILS_KSH_VDOT, the log terms in pair order); call it after svils_ksh_init_state or between two sweeps. */
/* save_model / communities of a sharded run (src/linksampling.cc:804-837,882-917): every rank hands `bytes`
 * bytes of host memory (its slice, padded to a common size) and receives world * bytes, rank by rank.
 * Staged through device memory, ncclAllGather on the handle's stream; synchronises.  Collective.
 * A handle without a communicator (world of one) copies send to recv. */
int svils_comm_allgather_host(svils_handle *h, const void *send, void *recv, size_t bytes);
int svils_sweep_ksharded(svils_handle *h, uint32_t nsweeps);   /* collective, asynchronous */
/* Mini-batch steps on a K-sharded handle (svils_set_stochastic with shard_block = 0: every rank holds all nodes and steps
 * through the SAME windows on its own columns).  The phases and exchanges are those of a sweep restricted to the window:
 * while a step is open svils_ksh_buffer_ptr returns the window's share of SVILS_KSH_DEN / DMAX / EARG (indexed by CSR entry
 * in this mode: the entries of the window's rows are one contiguous range) and of SVILS_KSH_ROWX.  With your own
 * collectives: svils_ksweep_phase in the order of a sweep; the first phase opens the step, SVILS_KPHASE_STOP closes it. */
int svils_step_ksharded(svils_handle *h, uint32_t nsteps);      /* collective, asynchronous */

/* ---- -findk: estimate the number of communities (an ADDITION of ABI 8; a handle of its own, nothing of svils_handle) ----
 * The reference's FastInit::batch_infer (src/fastinit.cc:240-289, dispatched at src/main.cc:321-327): label propagation
 * over a top-5 sparse gamma.  Every node holds 5 (label, value) slots, labels are node ids < n, slot 0's label is the
 * node's current label.  One iteration is
 *     svils_findk_count -> (host) padding draws for svils_findk_pad_requests -> svils_findk_apply -> svils_findk_report.
 * The padding draws stay on the host: they continue the reference's single MT19937 stream in node order (:217-225).
 * Without a HIP device every entry point answers SVILS_ERR_DEVICE ("no CPU path"); with one, a null handle SVILS_ERR_ARG. */
typedef struct svils_findk svils_findk;
/* alpha = 1 / k of -k (src/env.hh:344), link_thresh = -link-thresh; the state is [n][5] labels + values + pi on `device` */
int svils_findk_create(int device, uint32_t n, double alpha, double link_thresh, svils_findk **out);
int svils_findk_destroy(svils_findk *f);
/* links [nlinks][2] (p < q): every link, held-out ones included -- the training likelihood (:448-465) and the groups
 * (:291-414) run over all of them.  held_out[nlinks] (or null: none): 1 marks a link of the held-out set, left out of the
 * count (:258-271) and only there.  heldout_pairs [nheldout][3] (p, q, y) in the order of the reference's std::map
 * (heldout_likelihood, :511-543). */
int svils_findk_set_graph(svils_findk *f, const uint32_t *links, uint64_t nlinks, const uint8_t *held_out,
                          const uint32_t *heldout_pairs, uint64_t nheldout);
/* labels / values [n][5] (init_gamma, :178-190); pi follows (estimate_all_pi, src/fastinit.hh:460-476) */
int svils_findk_init_state(svils_findk *f, const uint32_t *labels, const double *values);
/* the count of one iteration (:258-271, Jacobi: every count reads the labels of the previous iteration) and every node's
 * top 5 of (count desc, label asc) -- the stable descending sort of set_gamma (:213-220).  *npad = nodes with 1 .. 4
 * distinct labels: they need 5 - ndistinct padding labels each. */
int svils_findk_count(svils_findk *f, uint32_t *npad);
/* those nodes in ascending order: nodes[npad], ndistinct[npad], labels [npad][4] (their counted labels, then UINT32_MAX) */
int svils_findk_pad_requests(svils_findk *f, uint32_t *nodes, uint32_t *ndistinct, uint32_t *labels);
/* set_gamma (:200-236) + estimate_all_pi: pads [npad][4], the first 5 - ndistinct of each row used, in
 * svils_findk_pad_requests order.  Counted slots get count + alpha, pads 2 alpha, nodes without a count keep their slots. */
int svils_findk_apply(svils_findk *f, const uint32_t *pads);
/* the likelihoods of the current state: *training_ll = mean edge_likelihood(p, q, 1) over all links (:448-465),
 * heldout_sums[3] = sums of edge_likelihood(p, q, y) over the held-out pairs: all, y = 0, y = 1 (:511-531).  Both are
 * fixed-order reductions (deterministic run to run, not the reference's sequential order).  With unlikely and masks
 * (both or neither): compute_and_log_groups (:291-414) -- *unlikely = directed link entries below link_thresh,
 * masks[n] = bit s set when slot s's label is a community of the node (the label 65535 is dropped, :341). */
int svils_findk_report(svils_findk *f, double *training_ll, double *heldout_sums, uint32_t *unlikely, uint32_t *masks);
/* labels / values / pi [n][5]; any may be null */
int svils_findk_get_state(svils_findk *f, uint32_t *labels, double *values, double *pi);
/* device milliseconds of the last count, apply, likelihoods and groups (hipEvent brackets; -1: not run yet) */
int svils_findk_get_timing(svils_findk *f, double ms[4]);

/* ---- -gml / -lcstats: link communities of a fitted model (an ADDITION of ABI 8; a handle of its own) -------------------
 * The reference's MMSBGen::get_lc_stats and MMSBGen::gml (src/mmsbgen.cc:181-193, 911-961; dispatched at src/main.cc:307-318):
 *   node pass  pi = gamma / s_i with s_i summed in k order (estimate_all, :700-729); group = the first strict maximum of
 *              pi from 0 (most_likely_group, src/mmsbgen.hh:112-123); bridgeness = (1 - sqrt(v K / (K - 1))) deg(i) with
 *              v = sum over k, in k order, of (pi - 1/K)^2 (bridgeness, :230-259)
 *   link pass  per link p < q: x_k = (pi_p[k] pi_q[k]) beta_k, beta_k = l0 / (l0 + l1) (estimate_beta, src/mmsbgen.hh:213-222);
 *              u / idx = the first strict maximum of x from 0, ratio = u / s, s the sum of x (inner_prod_max,
 *              src/matrix.hh:460-476).  The link joins community idx unless ratio < 0.5 (lc_current_draw_helper, :425-470)
 *              and is a GML edge unless ratio < 0.9 (gml, :936-954); a NaN ratio passes both.  s is summed in a fixed
 *              tree; links within 2 K DBL_EPSILON ratio of a threshold are decided again with s in k order, so every
 *              decision is the reference's
 *   counts     deg_c[i][k] = coloured links of community k at node i (Community, src/community.hh); per community the
 *              nodes with deg_c > 0, the sum of deg_c and the largest deg_c with its smallest node (deg_stats)
 * Any k >= 2.  Without a HIP device every entry point answers SVILS_ERR_DEVICE ("no CPU path"); with one, a null handle
 * SVILS_ERR_ARG. */
typedef struct svils_lc svils_lc;
/* device memory: pi [n][k] doubles (gamma is converted in place) and deg_c [n][k] uint32, plus O(n + links) */
int svils_lc_create(int device, uint32_t n, uint32_t k, svils_lc **out);
int svils_lc_destroy(svils_lc *h);
/* links [nlinks][2] with p < q < n, every link of the network (no held-out split), no repeats; any order (the GML list comes
 * out in (p, q) order, the per-link getters in this order) */
int svils_lc_set_graph(svils_lc *h, const uint32_t *links, uint64_t nlinks);
/* gamma [n][k], lambda [k][2]; svils_lc_run consumes the model: set it again before another run */
int svils_lc_set_model(svils_lc *h, const double *gamma, const double *lambda);
/* the three passes; synchronises */
int svils_lc_run(svils_lc *h);
/* after svils_lc_run (any pointer may be null): group / bridgeness / memberships (#k with deg_c > 0) / influence
 * (deg_c[i][group]) [n] */
int svils_lc_get_nodes(svils_lc *h, uint32_t *group, double *bridgeness, uint32_t *memberships, uint32_t *influence);
int svils_lc_get_degrees(svils_lc *h, uint32_t *deg_c);               /* [n][k] */
int svils_lc_get_pi(svils_lc *h, double *pi);                         /* [n][k] */
/* [k] each: nodes with deg_c > 0, the sum of deg_c, the largest deg_c and its smallest node (0 and 0 when empty) */
int svils_lc_get_communities(svils_lc *h, uint32_t *nodes, uint64_t *degsum, uint32_t *max, uint32_t *argmax);
/* per link in svils_lc_set_graph order: colour (idx) and flags (1: joins community idx, 2: GML edge, 4: decided by the
 * sequential recheck); counts[3] = links left out (ratio < 0.5), GML edges, rechecked links */
int svils_lc_get_links(svils_lc *h, uint32_t *colour, uint8_t *flags, uint64_t counts[3]);
/* the GML edges in (p, q) order: *count, and with edges non-null [count][3] (p, q, colour) */
int svils_lc_get_gml(svils_lc *h, uint64_t *count, uint32_t *edges);
/* device milliseconds of the last run's node pass, link pass (with the recheck) and counts (with the GML list); -1: not run */
int svils_lc_get_timing(svils_lc *h, double ms[3]);

/* ---- -batch-gpu: all-pairs batch variational inference (an ADDITION of ABI 8; a handle of its own) ---------------------
 * The reference's MMSBInfer::batch_infer (src/mmsbinfer.cc:833-930): coordinate ascent over ALL n (n - 1) / 2 pairs, the
 * exact model -link-sampling approximates.  One sweep is the loop body (:846-889):
 *   Elogpi / Elogbeta   set_dir_exp (src/mmsbinfer.hh:563-580) of gamma and lambda, on the device
 *   pair pass           every pair p < q outside the skip set: PhiComp::update_phis_until_conv (src/mmsbinfer.hh:104-203),
 *                       the Jacobi fixed point of the two indicator vectors from 1 / k, at most 50 rounds, the exit tested
 *                       on odd rounds (mean |new - old| < 1e-5 on both sides), normalised by the plain sum
 *   accumulation        gamma_next[p] += phi1, gamma_next[q] += phi2, lambda_next[k][y ? 0 : 1] += phi1[k] phi2[k] on top of
 *                       alpha and eta (:868-876): per-tile partial sums added in a fixed order, no floating-point atomics,
 *                       so a sweep is bitwise reproducible run to run
 * The device holds y(p, q) and the skip set as two n x n bit matrices: 2 * n * ceil(n / 32) * 4 bytes (256 MiB at
 * n = SVILS_BATCH_MAX_N).  Without a HIP device svils_batch_create answers SVILS_ERR_DEVICE ("no CPU path"); every other
 * entry point answers a null handle the same way, and SVILS_ERR_ARG with a device. */
#define SVILS_BATCH_MAX_K 256      /* the (W, V) table of the pair kernel ends here (svils_batch_variant) */
#define SVILS_BATCH_MAX_N 32768    /* bit matrices: 2 * n * ceil(n / 32) * 4 bytes = 256 MiB here; state 4 * n * k * 8 bytes */
typedef struct svils_batch svils_batch;
/* alpha, eta0, eta1, epsilon: src/env.hh:344-395 (epsilon in (0, 1)).  SVILS_ERR_ARG: n < 2, k < 2, a parameter <= 0;
 * SVILS_ERR_UNSUPPORTED: k > SVILS_BATCH_MAX_K or n > SVILS_BATCH_MAX_N (checked before any device call) */
int svils_batch_create(int device, uint32_t n, uint32_t k, double alpha, double eta0, double eta1, double epsilon,
                       svils_batch **out);
/* The same handle in SPARSE FORM, for the sampled engines (-rnode / -rpair / -infset / -snode) on graphs of any n the
 * memory holds: same arguments, contract and k limit, no SVILS_BATCH_MAX_N check (n < 2: SVILS_ERR_ARG; no room on the
 * device: SVILS_ERR_NOMEM, naming the buffer).  svils_batch_set_graph then keeps the links and the skip pairs as two
 * symmetric CSRs with ascending rows and 64-bit row offsets, on the host and on the device -- 8 (n + 1) + 8 * pairs bytes
 * each, nothing n x n anywhere -- with the same refusals in the same order.  The step kernels look a pair up by a
 * lower-bound search in a sorted row where the dense form reads a bit; everything else is the same code, and the two
 * forms give the same bits.  Every entry point works as on the dense form except the all-pairs
 * passes: svils_batch_sweep, svils_batch_elbo and svils_batch_set_elbo_tiles answer SVILS_ERR_UNSUPPORTED and touch
 * nothing.  State: 3 * n * k * 8 bytes at creation, and [ceil(n / G)][k] * 3 doubles (G = 64 / W pairs per wavefront)
 * from the first node step on (either form) */
int svils_batch_create_sparse(int device, uint32_t n, uint32_t k, double alpha, double eta0, double eta1, double epsilon,
                              svils_batch **out);
int svils_batch_destroy(svils_batch *h);
/* links [nlinks][2]: y(p, q) = 1 (Network::y); skip [nskip][2]: the held-out and validation pairs batch_infer leaves out
 * (:851-853).  Every pair has p < q < n; a self pair, p > q, a node >= n or a pair repeated inside its list: SVILS_ERR_ARG */
int svils_batch_set_graph(svils_batch *h, const uint32_t *links, uint64_t nlinks, const uint32_t *skip, uint64_t nskip);
/* gamma [n][k], lambda [k][2] (init_gamma / init_lambda, :372-397); every value > 0 */
int svils_batch_set_state(svils_batch *h, const double *gamma, const double *lambda);
int svils_batch_get_state(svils_batch *h, double *gamma, double *lambda);   /* either may be null; waits for the sweeps */
/* nsweeps passes of the loop body (:846-889), enqueued.  A pair whose normaliser is not > 0 (the reference's
 * assert(s > .0), src/mmsbinfer.hh:139) is counted on the device: the next call that waits for the device
 * (svils_batch_get_state, svils_batch_pair_loglik) then answers SVILS_ERR_UNSUPPORTED with "phi normaliser underflow" */
int svils_batch_sweep(svils_batch *h, uint32_t nsweeps);
/* edge_likelihood (src/mmsbinfer.hh:634-668) of m pairs (p, q, y) on the current state: out[i] = log(max(s, 1e-30)), s the
 * sum over z of pi_p pi_q beta_z for y = 1 and the k x k sum with epsilon off the diagonal for y = 0.  The caller adds them
 * (heldout_likelihood, src/mmsbinfer.cc:2086-2174, in its std::map order) */
int svils_batch_pair_loglik(svils_batch *h, const uint32_t *pairs, const uint8_t *y, uint64_t m, double *out);
/* of the last sweep, counted by the pair kernel: pairs visited, fixed-point rounds over all of them, the most rounds of one
 * pair, pairs whose normaliser underflowed (this one since the last svils_batch_set_state); any pointer may be null */
int svils_batch_get_stats(svils_batch *h, uint64_t *pairs_done, uint64_t *rounds_total, uint32_t *rounds_max,
                          uint64_t *underflow_pairs);
/* device milliseconds of the last sweep: Elogpi / Elogbeta, the pair pass, the reductions (hipEvent brackets; -1: none yet).
 * After a call of svils_batch_step_node / svils_batch_step_pairs / svils_batch_step_star / svils_batch_step_strat: ms[0] brackets all steps of that call, ms[1] = ms[2] = -1 */
int svils_batch_get_timing(svils_batch *h, double ms[3]);
/* the pair kernel's instantiation for k: a group of W lanes per pair, V values per lane, W * V >= k.  No device needed.
 * SVILS_ERR_ARG: k < 2 or a null pointer; SVILS_ERR_UNSUPPORTED: k > SVILS_BATCH_MAX_K */
int svils_batch_variant(uint32_t k, uint32_t *w, uint32_t *v);

/* ---- -rnode / -rpair: sampled-pair steps on the svils_batch handle (an ADDITION of ABI 8) -------------------------------
 * The reference's MMSBInfer::infer (src/mmsbinfer.cc:459-740): the Robbins-Monro version of the model batch_infer fits.
 * The caller draws the mini-batches (get_subsample, :1912-1945) and the step sizes; one step (:513-642, process()
 * :1092-1190) is
 *   Elogpi / Elogbeta   those of the current gamma and lambda
 *   pair pass           the fixed point of svils_batch_sweep for every pair of the mini-batch outside the skip set, y from
 *                       the bit matrix; gammat[p] += phi1, gammat[q] += phi2, lambdat[k][y ? 0 : 1] += phi1[k] phi2[k]
 *   gamma               for EVERY node i: gamma_i = (1 - rho_gamma) gamma_i + rho_gamma (alpha + scale gammat_i) (:578-600);
 *                       a node no pair touched moves towards alpha
 *   lambda              rho_lambda >= 0: lambda = (1 - rho_lambda) lambda + rho_lambda (eta + scale lambdat) (:613-637);
 *                       rho_lambda < 0: lambda is left bit for bit (the reference's delayed learning, :613)
 * nsteps steps are enqueued on the handle's stream in order and nothing waits for them; the getters do.  No
 * floating-point atomics: every sum has one owner and a fixed order, so a step is bitwise reproducible and the result does
 * not depend on how a run of steps is cut into calls.  Steps and sweeps may be mixed on one handle.
 * svils_batch_get_stats then covers all steps of the last call.  SVILS_ERR_ARG: a null array, rho_gamma outside (0, 1],
 * rho_lambda > 1, a scale that is not a positive number, no graph or no state.
 *
 * svils_batch_step_node: step s takes every pair (nodes[s], j), j != nodes[s], outside the skip set
 * (get_randomnode_edges, :1867-1876); the caller passes scale = n / 2.  Three launches per step. */
int svils_batch_step_node(svils_batch *h, uint32_t nsteps, const uint32_t *nodes, double scale, const double *rho_gamma,
                          const double *rho_lambda);
/* svils_batch_step_pairs: step s takes pairs[off[s] .. off[s + 1]) as given ([.][2], p < q < n); a pair listed twice
 * counts twice.  scale[s] is the reference's scale / mbsize (:566-568, :587, :631).  A listed pair of the skip set, a
 * self pair, p > q, a node >= n: SVILS_ERR_ARG, checked before anything is enqueued (the state is untouched).  Three
 * launches per step, two while lambda is left alone.  The lists travel through a pinned staging area: a call waits for
 * the previous call's copy (not for its steps) to have left it */
int svils_batch_step_pairs(svils_batch *h, uint32_t nsteps, const uint64_t *off, const uint32_t *pairs, const double *scale,
                           const double *rho_gamma, const double *rho_lambda);

/* ---- -infset: informative-set steps on the svils_batch handle (an ADDITION of ABI 8) -----------------------------------
 * The reference's FastAMM::infer (src/fastamm.cc:565-616) with opt_process / opt_process_noninf (:915-1126).  Step s is a
 * star: the start node a = start[s] and the entries off[s] .. off[s + 1) -- partner[e] = j, y[e] the pair's link bit,
 * rho_partner[e] the step size of row j.  One step:
 *   pair pass   every listed pair (a, j): the fixed point of svils_batch_sweep from the current Elogpi / Elogbeta
 *   gamma_j     (1 - rho_partner) gamma_j + rho_partner (alpha + scale[s] phi_j), Elogpi_j renewed
 *   gamma_a     (1 - rho_start[s]) gamma_a + rho_start[s] (alpha + scale[s] sum phi_a), Elogpi_a renewed
 *   lambda      rho_lambda[s] >= 0: (1 - rho_lambda) lambda + rho_lambda (eta + scale[s] (sum_{y=1} phi phi', sum_{y=0} phi phi')),
 *               Elogbeta renewed; rho_lambda[s] < 0: lambda and Elogbeta are left bit for bit
 * No other row of gamma is written.  A step without entries moves row a towards alpha and lambda towards eta (a start
 * node whose pairs are all held out).  The caller draws the stars and counts the times a node was touched, hence every
 * rho (:594).  The steps of a call run as a chain in ONE workgroup, step after step inside a launch (DESIGN.md section
 * 4h); a call cuts its chain into launches of at most 64 steps (svils_batch_set_star_chain: another length up to 1024; 0: the
 * default) and the result does not depend on where the cuts fall, nor on how the steps are cut into calls.  No
 * floating-point atomics.  Enqueued, nothing waits; svils_batch_get_stats / svils_batch_get_timing cover the call as for
 * the other steps; the lists travel through the pinned staging area of svils_batch_step_pairs.
 * SVILS_ERR_ARG, checked before anything is enqueued (the state is untouched): a null array, no graph or no state, a
 * node >= n, a partner equal to its step's start, a partner listed twice within a step, a listed pair of the skip set, a
 * y that disagrees with the graph, a rho outside (0, 1] (rho_lambda: > 1), a scale that is not a positive number */
int svils_batch_step_star(svils_batch *h, uint32_t nsteps, const uint32_t *start, const uint64_t *off, const uint32_t *partner,
                          const uint8_t *y, const double *rho_partner, const double *rho_start, const double *scale,
                          const double *rho_lambda);
/* steps per launch of the star chain: 1 .. SVILS_BATCH_STAR_CHAIN_MAX, 0 the default of 64; more: SVILS_ERR_ARG (a longer
 * chain is a longer kernel on a machine others share).  Results do not depend on it */
#define SVILS_BATCH_STAR_CHAIN_MAX 1024
int svils_batch_set_star_chain(svils_batch *h, uint32_t max_steps);
/* Elogpi [n][k] and Elogbeta [k][2] as the step kernels read them: those of the current gamma / lambda, renewed first if a
 * sweep or svils_batch_set_state came since the last step call (what the next step call would do), else the ones the steps
 * maintain row by row.  Waits for the stream.  Either pointer may be null.  SVILS_ERR_ARG: no state */
int svils_batch_get_expectations(svils_batch *h, double *elogpi, double *elogbeta);

/* ---- -snode: stratified random node steps on the svils_batch handle (an ADDITION of ABI 8) ------------------------------
 * The reference's FastAMM2::infer (src/fastamm2.cc:535-702) with opt_process / opt_process_noninf (:933-1165), the engine
 * behind `-stratified -rnode`.  Step s is a star as in svils_batch_step_star -- the start node a = start[s], the entries
 * off[s] .. off[s + 1) with partner[e] = j and y[e] the pair's link bit -- but EVERY row of gamma moves, with one step
 * size rho = rho_gamma[s]:
 *   Elogpi / Elogbeta   those of the current gamma and lambda
 *   pair pass           every listed pair (a, j): the fixed point of svils_batch_sweep
 *   listed rows and a   gamma_i = (1 - rho) gamma_i + rho (alpha + scale[s] gammat_i), gammat_j = phi_j, gammat_a = sum phi_a
 *   every other row     gamma_i = (1 - rho) gamma_i + rho alpha
 *   lambda              as svils_batch_step_star: rho_lambda[s] < 0 leaves lambda and Elogbeta bit for bit
 * The other rows are not written by the step.  gamma_i - alpha of such a row is multiplied by (1 - rho_s) at every step,
 * so the handle keeps, on the host, the running c = sum_s log1p(-rho_s) (one addition per step, in step order, whatever
 * the cut into calls) and per row the value c had when the row was last written; a row's true value is
 * alpha + (gamma_i - alpha) exp(c - c_i), and the step applies that factor to the rows it names as it reads them (a
 * factor of exactly 1 leaves the bits).  Every other entry point that reads or writes gamma (svils_batch_get_state,
 * _get_expectations, _sweep, _step_node, _step_pairs, _step_star, _pair_loglik, _elbo) first brings every row that is
 * behind to its true value in one elementwise launch; svils_batch_set_state starts the bookkeeping afresh.  No caller can
 * observe a stale row.  Two launches per step with entries (grid-wide pair pass, fixed-order tail), one without; Elogpi is
 * formed in registers and its buffer is not maintained (the next entry point that needs it renews it).  No floating-point
 * atomics; the result does not depend on how the steps are cut into calls.  A call between two steps that catches the rows
 * up (svils_batch_get_state, say) rounds them there: later results then agree with the uninterrupted run to rounding, not
 * bit for bit.  svils_batch_get_stats / svils_batch_get_timing cover the call as for the other steps.
 * SVILS_ERR_ARG, checked before anything is enqueued (the state and the bookkeeping are untouched): the cases of
 * svils_batch_step_star (it has no rho_partner), a rho_gamma outside (0, 1) -- 1 is refused: log1p(-1) has no value --
 * and a rho_lambda above 1 */
int svils_batch_step_strat(svils_batch *h, uint32_t nsteps, const uint32_t *start, const uint64_t *off, const uint32_t *partner,
                           const uint8_t *y, const double *rho_gamma, const double *scale, const double *rho_lambda);
/* rows of gamma whose stored value is behind their true value (c_i != c).  No device work.  SVILS_ERR_ARG: a null pointer */
int svils_batch_get_lag(svils_batch *h, uint64_t *rows_behind);

/* ---- -logl: the variational lower bound on the svils_batch handle (an ADDITION of ABI 8) ---------------------------------
 * The reference's approx_log_likelihood (src/mmsbinfer.cc:1948-2060, src/fastamm.cc:1129-1258) of the current state:
 * s = G + P + N with Elogpi / Elogbeta of the current gamma / lambda (those svils_batch_get_expectations would return),
 *   G   sum over k of lnGamma(eta0 + eta1) - lnGamma(eta0) - lnGamma(eta1) + sum_t (eta_t - 1) Elogbeta_kt
 *       - [lnGamma(lambda_k0 + lambda_k1) - sum_t lnGamma(lambda_kt)] - sum_t (lambda_kt - 1) Elogbeta_kt
 *   P   sum over every pair p < q outside the skip set, phi1 / phi2 the fixed point of svils_batch_sweep from 1 / k, of
 *       sum_k phi1 phi2 elogf + [y = 1] log(epsilon) (S1 S2 - sum_k phi1 phi2) + sum_k phi1 Elogpi_p + sum_k phi2 Elogpi_q
 *       - sum_k phi1 log phi1 - sum_k phi2 log phi2; an entry of phi that is exactly 0 adds 0 (the reference: NaN)
 *   N   sum over p of lnGamma(k alpha) - k lnGamma(alpha) + (alpha - 1) sum_k Elogpi_pk
 *       - [lnGamma(sum_k gamma_pk) - sum_k lnGamma(max(gamma_pk, 1e-30))] - sum_k (gamma_pk - 1) Elogpi_pk
 * parts: total, G, P, N.  pairs_done / rounds_total (either may be null): the pairs of the pass and their fixed-point rounds.
 * The pass has buffers and counters of its own: gamma, lambda, the expectations, svils_batch_get_stats and every later
 * sweep or step are as without it.  Sums in a fixed order, no floating-point atomics: bitwise reproducible, and the same
 * bits however svils_batch_set_elbo_tiles cuts the tiles into launches.  Waits for the device; svils_batch_get_timing
 * called next gives the pass's device ms in ms[0], ms[1] = ms[2] = -1.  SVILS_ERR_ARG: null parts, no graph or no state;
 * SVILS_ERR_UNSUPPORTED "phi normaliser underflow": a pair of the pass whose normaliser is not > 0 (parts untouched) */
int svils_batch_elbo(svils_batch *h, double parts[4], uint64_t *pairs_done, uint64_t *rounds_total);
/* tiles per launch of the pair pass of svils_batch_elbo: 1 .. 2048, 0 the default of 2048 (the sweep's bound); more:
 * SVILS_ERR_ARG.  Results do not depend on it */
int svils_batch_set_elbo_tiles(svils_batch *h, uint32_t tiles_per_launch);

/* ---- -orig: the full K x K blockmodel (an ADDITION of ABI 8; a handle of its own) ---------------------------------------
 * The reference's MMSBInferOrig::batch_infer (src/mmsbinferorig.cc:212-294; fixed point PhiComp2,
 * src/mmsbinferorig.hh:110-220): the mixed-membership blockmodel of Airoldi et al. with a K x K matrix beta of block
 * rates, coordinate ascent over every ORDERED pair (p, q), p != q.  One sweep: Elogpi = psi(max(gamma, 1e-30)) -
 * psi(row sum) (:601-622); for every ordered pair outside the skip list, from phi1 = phi2 = 1 / K, up to 50 rounds of
 *   next1[g] ~ exp(Elogpi_p[g] + sum_h L_y[g][h] phi2[h]),  next2[g] ~ exp(Elogpi_q[g] + sum_h L_y[g][h] phi1[h])
 * (L_1 = log beta, L_0 = log(1 - beta); both from the OLD vectors, L_y NOT transposed for the second side, normalised by
 * the plain sum), the old vectors saved at even rounds and the exit -- mean |next - old| < 1e-5 on both sides -- tested
 * at odd ones; then gamma_next[p] += phi1, gamma_next[q] += phi2 on top of alpha, num += y phi1 phi2^T, tot += phi1
 * phi2^T, and afterwards gamma = gamma_next, beta = num / tot.  The matrix-shaped parts run on v_mfma_f64_16x16x4_f64, a
 * wavefront owning 16 pairs (svinet_amd/csrc/svils_orig.hip).  No floating-point atomics: two runs
 * on the same device are bitwise equal and svils_orig_sweep(h, 3) equals three svils_orig_sweep(h, 1).
 * Bounded launches: a sweep is cut into launches of whole p rows whose phi vectors fill at most 256 MiB -- at most
 * max(n, 2^24 / KP) ordered pairs per launch, KP = 16 ceil(k / 16) -- so no launch grows with n^2.
 * Degenerate cases are counted, never asserted: a pair whose normaliser is not > 0 is counted; a beta entry outside (0, 1)
 * after the update (a block that saw only links or only non-links: num == tot bitwise, or num == 0) is counted and raises
 * a device flag -- sweeps already in the queue then leave the state alone, and the next call that waits
 * (svils_orig_get_state, svils_orig_pair_loglik) answers SVILS_ERR_UNSUPPORTED naming the cause; svils_orig_set_state
 * lowers the flag.  Without a HIP device svils_orig_create answers SVILS_ERR_DEVICE ("no CPU path"); every other entry
 * point answers a null handle the same way, and SVILS_ERR_ARG with a device. */
#define SVILS_ORIG_MAX_K 64                   /* the instantiations of the pair kernel end here (svils_orig_variant) */
#define SVILS_ORIG_MAX_N SVILS_BATCH_MAX_N    /* bit matrices for y and the skip list, as the batch handle's */
typedef struct svils_orig svils_orig;
/* SVILS_ERR_ARG: n < 2, k < 2, alpha <= 0; SVILS_ERR_UNSUPPORTED: k > SVILS_ORIG_MAX_K or n > SVILS_ORIG_MAX_N (checked
 * before any device call) */
int svils_orig_create(int device, uint32_t n, uint32_t k, double alpha, svils_orig **out);
int svils_orig_destroy(svils_orig *h);
/* links [nlinks][2], p < q < n: y(p, q) = y(q, p) = 1.  skip [nskip][2]: ORDERED pairs (p != q, either orientation; the
 * two orientations are separate entries) the sweep leaves out.  SVILS_ERR_ARG: a self pair, a node >= n, a link with
 * p > q, a pair repeated inside its list */
int svils_orig_set_graph(svils_orig *h, const uint32_t *links, uint64_t nlinks, const uint32_t *skip, uint64_t nskip);
/* p rows per launch from the next svils_orig_set_graph on: at most `rows` (never more than the bound above admits), 0 the
 * default.  Results agree to rounding whatever the value: a column sum of gamma is added launch by launch */
int svils_orig_set_launch_rows(svils_orig *h, uint32_t rows);
/* gamma [n][k], beta [k][k].  SVILS_ERR_ARG: a gamma that is negative or not finite, a beta outside (0, 1) */
int svils_orig_set_state(svils_orig *h, const double *gamma, const double *beta);
/* either may be null; waits for the sweeps.  With the degenerate flag up the state of the last applied sweep is still
 * copied out, then SVILS_ERR_UNSUPPORTED comes back */
int svils_orig_get_state(svils_orig *h, double *gamma, double *beta);
/* nsweeps sweeps, enqueued; nothing waits */
int svils_orig_sweep(svils_orig *h, uint32_t nsweeps);
/* edge_likelihood (:563-587) of pairs [m][2] (ordered, p != q) with y [m]: log sum_g sum_h pi_p[g] pi_q[h]
 * (y ? beta_gh : 1 - beta_gh), pi = gamma / row sum.  No clamp.  Waits */
int svils_orig_pair_loglik(svils_orig *h, const uint32_t *pairs, const uint8_t *y, uint64_t m, double *out);
/* of the last svils_orig_sweep call (all its sweeps): pairs visited, rounds over all pairs, most rounds of one pair, pairs
 * whose normaliser was not > 0; and since the last svils_orig_set_state: beta entries that left (0, 1).  Any pointer may
 * be null; waits */
int svils_orig_get_stats(svils_orig *h, uint64_t *pairs_done, uint64_t *rounds_total, uint32_t *rounds_max,
                         uint64_t *bad_normalisers, uint64_t *bad_betas);
/* device ms of the last sweep: Elogpi and the log tables, the pair pass, the reductions (-1 before the first sweep) */
int svils_orig_get_timing(svils_orig *h, double ms[3]);
/* ---- -orig -logl: the variational lower bound on the svils_orig handle (an ADDITION of ABI 8) ----------------------------
 * The reference's MMSBInferOrig::approx_log_likelihood (src/mmsbinferorig.cc:624-726, under GLOBALPHIS) of the CURRENT
 * state: s = P + N (beta is a point estimate, so it has no term), with Elogpi of the current gamma,
 * T1 = log(beta + 1e-10), T0 = log((1 - beta) + 1e-10),
 *   P   sum over every ordered pair (p, q), p != q, outside the skip list -- the pairs a sweep visits -- phi1 / phi2 the
 *       fixed point of svils_orig_sweep from 1 / k (the same kernel: the same rounds, the same exit rule), of
 *       sum_g sum_h phi1[g] phi2[h] T_y[g][h] + sum_k phi1[k] Elogpi_p[k] + sum_k phi2[k] Elogpi_q[k]
 *       - sum_k phi1[k] log phi1[k] - sum_k phi2[k] log phi2[k]; an entry of phi that is exactly 0 adds 0 (the reference: NaN)
 *   N   sum over p of lnGamma(k alpha) - k lnGamma(alpha) + (alpha - 1) sum_k Elogpi_pk
 *       - [lnGamma(sum_k gamma_pk) - sum_k lnGamma(max(gamma_pk, 1e-30))] - sum_k (gamma_pk - 1) Elogpi_pk
 * out: total, P, N.  The reference reads the phi vectors the last sweep stored (fixed points of the state before it) and
 * adds the held-out pairs no sweep visits with whatever their slots hold; here the fixed point is taken from the current
 * state over the visited pairs only, so the bound of a fresh state is defined.
 * The pass runs the sweep's pair kernel over the sweep's row cuts with a counter block, Elogpi and tables of its own, and
 * writes only that scratch and the phi buffers every sweep overwrites: gamma, beta, svils_orig_get_stats, the caches of
 * the link queries and every later sweep are bit for bit as without it.  No floating-point atomics; a partial sum belongs
 * to a piece of a row that depends on n alone and the partials are added in a fixed order: the three outputs are bitwise
 * equal from run to run, on two handles, and for every svils_orig_set_launch_rows value.  Waits for the device.
 * SVILS_ERR_ARG: a null handle or a null out, no graph or no state; SVILS_ERR_UNSUPPORTED: the degenerate flag is up (the
 * message of svils_orig_get_state), or "normaliser not > 0": a pair of the pass whose normaliser is not > 0 (out and the
 * state untouched); SVILS_ERR_DEVICE: no HIP device, as for the siblings. */
int svils_orig_elbo(svils_orig *h, double out[3]);
/* of the last svils_orig_elbo pass: pairs visited, rounds over all pairs, most rounds of one pair, pairs whose normaliser
 * was not > 0 (all 0 before the first pass).  Any pointer may be null; waits */
int svils_orig_get_elbo_stats(svils_orig *h, uint64_t *pairs_done, uint64_t *rounds_total, uint32_t *rounds_max,
                              uint64_t *bad_normalisers);
/* device ms of the last svils_orig_elbo pass: the whole pass, its pair launches (the first one's bracket includes Elogpi,
 * the tables and the node terms), its term launches (-1 before the first pass).  The sweep's events are as they were */
int svils_orig_get_elbo_timing(svils_orig *h, double ms[3]);
/* ---- link prediction from a fitted -orig state (an ADDITION of ABI 8; nothing a sweep reads is written) ------------------
 * score(p, c) = sum_g sum_h pi_p[g] beta[g][h] pi_c[h], pi_x = gamma_x / sum_k gamma_xk: the argument of the reference's
 * edge_likelihood(p, c, 1) (src/mmsbinferorig.cc:563-587).  beta is not symmetric in general, so score(p, c) != score(c, p):
 * "q among p's candidates" uses score(p, .), "p among q's candidates" uses score(q, .), and a scored pair (p, q) is scored
 * in the orientation given.
 * Candidates of p: every node c != p, except those where {p, c} is a link of the graph and NEITHER (p, c) NOR (c, p) is in
 * the handle's skip list (a pair left out of training in either orientation IS a candidate: finding those is the point --
 * the rule of svils_predict_links).  Note what the reference's own skip list is: a held-out pair in the orientation drawn
 * (:231-235); the reverse orientation and the validation pairs are trained on.  A caller that wants to rank held-out links
 * hands svils_orig_set_graph both orientations of every pair it holds out (the command line's -clean-holdout).
 * The contracts are those of svils_link_prob / svils_predict_links / svils_rank_links: nodes == NULL means all n nodes
 * (nnodes 0 or n); topk is 1 .. SVILS_PREDICT_MAX_TOPK; order is score descending, ties by ascending id; empty slots are
 * UINT32_MAX / -1.0; above, tied and ncand are counted over the candidates c != q (q itself need not be one); any output
 * pointer of svils_orig_rank_links may be NULL.  The calls enqueue on the handle's stream behind the sweeps already there
 * and synchronise; results are bitwise deterministic and a row does not depend on the other rows of the call.
 * All three calls get their scores from ONE device function (the 64 x 64 fp64 MFMA tile of svils_predict_links, fed with
 * pi_p^T beta -- summed over g ascending -- and pi): svils_orig_link_prob(p, q) and score[] of svils_orig_rank_links are
 * bitwise the score svils_orig_predict_links lists for q in p's row, and a node listed at place j has
 * above <= j <= above + tied.  Against a plain fp64 evaluation the score differs by rounding only (two dot products of at
 * most 64 positive terms: relative error below 2e-14).
 * The state is read as it is when the call runs: a copy of pi is rebuilt whenever svils_orig_set_state or svils_orig_sweep
 * came since it was built.
 * Device scratch, allocated on first use: pi, n x 16 ceil(k / 16) doubles (at most 16 MB; freed by svils_orig_destroy); one
 * bit matrix of the excluded pairs, adj & ~(skip | skip^T), n x ceil(n / 32) words (at most 128 MB; built once per graph,
 * freed by the next svils_orig_set_graph or svils_orig_destroy); and per internal batch of 8192 query rows at most 4 MB of
 * query rows, 384 MB of partial top-k heaps (svils_orig_predict_links only; 63 MB at topk = 10), 24 MB of results and 200 KB
 * of thresholds and counters (freed by svils_orig_destroy).
 * SVILS_ERR_ARG: a null handle, no graph or no state, a node id >= n, a pair with p == q, topk == 0 or
 * > SVILS_PREDICT_MAX_TOPK, a null array that is needed.  SVILS_ERR_UNSUPPORTED, with the message of svils_orig_get_state:
 * a state whose degenerate flag is up. */
/* score of pairs[npairs][2] (ordered, p != q, both < n) -> prob[npairs] */
int svils_orig_link_prob(svils_orig *h, const uint32_t *pairs, uint64_t npairs, double *prob);
/* the top-k candidates of each query node -> ids[nnodes][topk], scores[nnodes][topk] */
int svils_orig_predict_links(svils_orig *h, const uint32_t *nodes, uint32_t nnodes, uint32_t topk, uint32_t *ids, double *scores);
/* for every directed pair (p, q): above[i] = #{candidates c != q of p : score(p, c) > s}, tied[i] = #{... == s}, ncand[i] =
 * #{candidates c != q}, score[i] = s = score(p, q) */
int svils_orig_rank_links(svils_orig *h, const uint32_t *pairs, uint64_t npairs, uint32_t *above, uint32_t *tied, uint32_t *ncand,
                          double *score);
/* device ms of the last of these three calls, from behind the sweeps it waited for to its last kernel (hipEvents on the
 * handle's stream; a call of several internal batches includes the host's turn-round between them); -1 before the first */
int svils_orig_get_query_timing(svils_orig *h, double *ms);
/* host only: the instantiation of the pair kernel for k -- padded K, pairs per wavefront, 1 if the log tables live in LDS
 * (0: in registers).  SVILS_ERR_ARG: k < 2 or a null pointer; SVILS_ERR_UNSUPPORTED: k > SVILS_ORIG_MAX_K */
int svils_orig_variant(uint32_t k, uint32_t *padded_k, uint32_t *pairs_per_wave, uint32_t *tables_in_lds);

/* ---- -single: the single-membership stochastic blockmodel (an ADDITION of ABI 8; a handle of its own) --------------------
 * The reference's SBM::batch_infer (src/sbm.cc:457-543, src/sbm.hh).  State: phi [n][k] (rows sum to 1), gamma [k],
 * lambda [k + 1][2] (row k: the rate between different groups; column 0 counts links, column 1 non-links).  The trained
 * pairs T are all unordered pairs p != q that are not in the skip list.  One iteration:
 *   E-step   at most 10 passes; a pass takes p = 0 .. n - 1 in order (Gauss-Seidel: p reads the rows 0 .. p - 1 wrote in
 *            the same pass): a_k = Elogpi_k + sum over (p, q) in T of (1 - phi_qk) Elogbeta[K][y'] + phi_qk Elogbeta[k][y'],
 *            y' = 0 for a link and 1 for a non-link; phi_p = exp(a - logsumexp a); msum = sum_p sum_k |old - new|; the
 *            E-step ends after the first pass with msum < 0.01
 *   M-step   gamma_k = alpha + sum_i phi_ik; lambda_k0 = eta_k0 + sum over links of T of phi_ik phi_jk, lambda_k1 = eta_k1 +
 *            the same over non-links; row K: eta_K0 + sum over links sum_k (1 - phi_ik phi_jk), and over non-links; then
 *            Elogpi = psi(gamma_k) - psi(sum gamma), Elogbeta = psi(lambda_kt) - psi(lambda_k0 + lambda_k1)
 * The device never walks the n^2 pairs: with S the column sums of phi, the sum over all partners of p is S - phi_p, and
 * the links and the skipped pairs of p correct it, so a pass costs O((links + skips) k) and runs at
 * any n the memory holds.  All sums are fp64 in a fixed order (ascending partner within a row, ascending wavefront / block
 * across partials) and no floating-point atomic is used: results are bitwise equal from run to run, on two handles, for
 * every svils_sbm_set_launch_nodes value and for both chain forms, and svils_sbm_sweep(h, 3) equals three
 * svils_sbm_sweep(h, 1).  Without a HIP device svils_sbm_create answers SVILS_ERR_DEVICE ("no CPU path"); every other
 * entry point answers SVILS_ERR_DEVICE for a null handle there, SVILS_ERR_ARG where a device exists. */
#define SVILS_SBM_MAX_K 256
#define SVILS_SBM_MAX_PASSES 10               /* passes of one E-step (src/sbm.cc:470) */
typedef struct svils_sbm svils_sbm;
/* eta [k + 1][2], every entry > 0.  SVILS_ERR_ARG: n < 2, k < 2, alpha <= 0, a null pointer, an eta entry not > 0;
 * SVILS_ERR_UNSUPPORTED: k > SVILS_SBM_MAX_K (all checked before any device call) */
int svils_sbm_create(int device, uint32_t n, uint32_t k, double alpha, const double *eta, svils_sbm **out);
int svils_sbm_destroy(svils_sbm *h);
/* links [nlinks][2] with p < q < n, each once; skip [nskip][2]: pairs p < q < n left out of training, each once (a skipped
 * pair is a link exactly when it is listed in links).  Both are kept as symmetric CSRs with ascending rows and 64-bit
 * offsets.  The refusals (SVILS_ERR_ARG, the graph the handle had stays) are svils_batch_set_graph's */
int svils_sbm_set_graph(svils_sbm *h, const uint32_t *links, uint64_t nlinks, const uint32_t *skip, uint64_t nskip);
/* phi [n][k]: finite, >= 0, every row summing to 1 within 1e-9; gamma [k] > 0; lambda [k + 1][2] > 0.  Elogpi and Elogbeta
 * are formed on the device.  SVILS_ERR_ARG otherwise (the state the handle had stays) */
int svils_sbm_set_state(svils_sbm *h, const double *phi, const double *gamma, const double *lambda);
/* any pointer may be NULL.  Waits for the device */
int svils_sbm_get_state(svils_sbm *h, double *phi, double *gamma, double *lambda);
/* The E-step alone, from the stored gamma and lambda: at most max_passes (1 .. SVILS_SBM_MAX_PASSES) passes.  *passes:
 * the passes run; msum [max_passes]: msum of every pass run (the rest 0).  Either may be NULL.  Waits for the device */
int svils_sbm_estep(svils_sbm *h, uint32_t max_passes, uint32_t *passes, double *msum);
/* niter whole iterations (E-step of at most SVILS_SBM_MAX_PASSES passes, M-step, Elogpi / Elogbeta), queued without a
 * host round trip: the launches of all passes are queued, and those behind the end of an E-step return at once */
int svils_sbm_sweep(svils_sbm *h, uint32_t niter);
/* edge_likelihood2 (src/sbm.hh:284-308) of the current state: out[x] = log max(s, 1e-30), s = sum_k phi_pk phi_qk f_k +
 * (1 - sum_k phi_pk phi_qk) f_K, f = r or 1 - r by y[x], r_k = lambda_k0 / (lambda_k0 + lambda_k1).  Waits for the device */
int svils_sbm_pair_loglik(svils_sbm *h, const uint32_t *pairs, const uint8_t *y, uint64_t m, double *out);
/* passes of the last E-step; passes over the last svils_sbm_estep / svils_sbm_sweep call; msum [SVILS_SBM_MAX_PASSES] of
 * every pass of the last E-step (0 past its end).  Any pointer may be NULL.  Waits for the device */
int svils_sbm_get_stats(svils_sbm *h, uint32_t *passes_last, uint64_t *passes_call, double *msum);
/* device ms of the last call: the whole call; the chain launches of its last E-step (those behind its end included); the
 * M-step of its last iteration (-1 after svils_sbm_estep).  -1 before the first call */
int svils_sbm_get_timing(svils_sbm *h, double ms[3]);
/* nodes per launch of the chain kernel from the next call on; 0: the default, 2048 -- a launch stays a few milliseconds on
 * a shared device (DESIGN.md section 4r has the measurement).  The results do not depend on it, bit for bit */
int svils_sbm_set_launch_nodes(svils_sbm *h, uint32_t nodes);
/* plain != 0: the plain chain -- one wavefront, one node per turn, no look-ahead -- instead of the blocked one.  The same
 * bits; kept for the measurement of DESIGN.md section 4r */
int svils_sbm_set_plain_chain(svils_sbm *h, int plain);
/* host only: the lane mapping of the chain kernel for k -- a lane holds the columns lane, lane + 64, .. (*cols_per_lane of
 * them) of a row -- and *block_nodes = B, the consecutive nodes (= wavefronts of the workgroup) whose gathers overlap.
 * SVILS_ERR_ARG: k < 2 or a null pointer; SVILS_ERR_UNSUPPORTED: k > SVILS_SBM_MAX_K */
int svils_sbm_variant(uint32_t k, uint32_t *cols_per_lane, uint32_t *block_nodes);
/* -single-logl: the variational lower bound of the handle's CURRENT state -- phi, gamma, lambda and the Elogpi / Elogbeta
 * the handle keeps current (SBM::approx_log_likelihood, src/sbm.cc:1133-1239, compiled out there).
 * (An ADDITION of ABI 8.  The two names do not begin with svils_sbm_: that family's count is pinned.)
 * out = total, P, N, G with total = P + N + G.  E_1[k] = Elogbeta[k][0], E_0[k] = Elogbeta[k][1], k = 0 .. K:
 *   P  the sum over every trained pair p < q, y its link bit, of sum_k phi_pk phi_qk E_y[k] + (1 - sum_k phi_pk phi_qk) E_y[K]
 *      (the proper 1 - sum_k, not the M-step's row-K sum of 1 - phi_pk phi_qk over k)
 *   N  sum_p sum_k phi_pk (Elogpi_k - log phi_pk); an entry of phi that is exactly 0 adds 0 (the reference gives NaN)
 *   G  for k = 0 .. K: lnGamma(eta_k0 + eta_k1) - lnGamma(eta_k0) - lnGamma(eta_k1) + sum_t (eta_kt - 1) Elogbeta[k][t] minus
 *      the same expression in lambda_k; plus lnGamma(K alpha) - K lnGamma(alpha) + (alpha - 1) sum_k Elogpi_k -
 *      [lnGamma(sum gamma) - sum_k lnGamma(max(gamma_k, 1e-30))] - sum_k (gamma_k - 1) Elogpi_k
 * The device forms P from the sums a_k, b_k of phi_ik phi_jk over the trained links and non-links exactly as the M-step
 * forms them (P = sum_k D1_k a_k + sum_k D0_k b_k + n1 E_1[K] + n0 E_0[K], D_y,k = E_y[k] - E_y[K]) and N in a row kernel
 * that leaves one partial per piece of SVILS_SBMELBO_PIECE_ROWS rows (more where n exceeds 4096 pieces: the extent of a
 * piece depends on n alone); one block adds all partials in ascending order.  G is formed on the host inside the call,
 * from gamma, lambda, Elogpi and Elogbeta copied back.  O((n + links + skipped pairs) k).  All sums fp64 in a fixed order,
 * no floating-point atomic: the four outputs are bitwise equal from run to run, on two handles, for every
 * svils_sbm_set_launch_nodes value and for both chain forms.  The call changes nothing that a pass, an M-step,
 * svils_sbm_get_stats or svils_sbm_get_timing reads.  Waits for the device.
 * SVILS_ERR_ARG: a null handle, a null out, no graph or no state */
#define SVILS_SBMELBO_PIECE_ROWS 16
int svils_sbmelbo(svils_sbm *h, double out[4]);
/* device ms of the last svils_sbmelbo pass (its four kernels); -1 before the first */
int svils_sbmelbo_get_timing(svils_sbm *h, double ms[1]);

/* ---- -ppc / -gen: networks drawn from a model and their statistics (an ADDITION of ABI 8; a handle of its own) -----------
 * The device side of the reference's MMSBGen::gen (src/mmsbgen.cc:43-71) and MMSBGen::ppc (draw_and_save, :662-697, with
 * the statistics of :418-499 and :605-630).  GSL's random stream is not reproduced and cannot be: the draw is DEFINED here
 * (DESIGN.md section 4l), and every decision is that definition's, bit for bit, on any grid:
 *   random     Philox4x32-10, key (seed, r), counter (p, q, stream, block); the pair draw is stream 0, block 0, and
 *              u = ((w0 >> 5) 2^26 + (w1 >> 6)) 2^-53 from the first two output words
 *   link       for p < q: x_j = (pi_p[j] pi_q[j]) beta_j, s = sum of x_j in ascending j, y = (u < s).  No link is drawn
 *              through epsilon (the reference's generator draws none when the indicators differ, src/mmsbgen.hh:180).
 *              The tile kernel sums s on v_mfma_f64_16x16x4_f64; a pair whose tile sum lies within 2 K DBL_EPSILON s of
 *              u is decided again with the ascending sum (the recheck of svils_lc)
 *   colour     of a link: the first strict maximum x_max of x from 0; ratio = x_max / s; the link joins community
 *              colour unless ratio < 0.5 (lc_current_draw_helper, :425-470; a NaN ratio joins) -- the same rule for a
 *              drawn and for an observed list
 *   statistics of the current list: links, deg [n], the largest degree and its smallest node, tri [n] (triangles through
 *              a node), wedges = sum deg (deg - 1) / 2, transitivity = 3 T / wedges, the mean over nodes of
 *              tri_i / C(deg_i, 2) (0 where deg < 2); per community size_k (joined links) and logpe_k = sum of
 *              log x_max over them (the reference's edge_likelihood, :605-630), accumulated exactly in integer bins, so
 *              it depends on no order
 * n <= SVILS_PPC_MAX_N and 1 <= k <= SVILS_PPC_MAX_K, else SVILS_ERR_UNSUPPORTED before any device call.  Without a HIP
 * device every other entry point answers SVILS_ERR_DEVICE ("no CPU path"); with one, a null handle SVILS_ERR_ARG. */
#define SVILS_PPC_MAX_N 32768
#define SVILS_PPC_MAX_K 2048
typedef struct svils_ppc svils_ppc;
/* device memory: two bit matrices n x ceil(n / 64) words (at most 128 MB each), pi twice (n x k doubles, padded), and
 * max_links x 56 bytes of lists; max_links is the capacity of the link list */
int svils_ppc_create(int device, uint32_t n, uint32_t k, uint64_t max_links, svils_ppc **out);
int svils_ppc_destroy(svils_ppc *h);
/* pi [n][k]: every entry >= 0 and finite, every row summing to 1 within 1e-9; beta [k] in [0, 1]: else SVILS_ERR_ARG */
int svils_ppc_set_params(svils_ppc *h, const double *pi, const double *beta);
/* replicate r of seed becomes the current list.  More links than max_links: SVILS_ERR_NOMEM, the count is what
 * svils_ppc_get_draw_counts reports, and the current list and its statistics stay as they were */
int svils_ppc_draw(svils_ppc *h, uint32_t seed, uint32_t r);
/* the observed network becomes the current list: links [nlinks][2] with p < q < n, no repeats, any order */
int svils_ppc_set_links(svils_ppc *h, const uint32_t *links, uint64_t nlinks);
/* the statistics of the current list under the current parameters; synchronises */
int svils_ppc_stats(svils_ppc *h);
/* counts[2] = the links of the last svils_ppc_draw (also where it answered SVILS_ERR_NOMEM), the pairs it rechecked */
int svils_ppc_get_draw_counts(svils_ppc *h, uint64_t counts[2]);
/* the current list in (p, q) order: *count, and links [count][2]; after svils_ppc_stats colour [count] and joined [count] */
int svils_ppc_get_links(svils_ppc *h, uint64_t *count, uint32_t *links, uint32_t *colour, uint8_t *joined);
/* after svils_ppc_stats (any pointer may be null): deg [n], tri [n] */
int svils_ppc_get_nodes(svils_ppc *h, uint32_t *deg, uint32_t *tri);
/* after svils_ppc_stats: counts[5] = links, largest degree, its smallest node, triangles, wedges; values[2] = transitivity,
 * mean local clustering (transitivity is NaN without a wedge) */
int svils_ppc_get_summary(svils_ppc *h, uint64_t counts[5], double values[2]);
/* after svils_ppc_stats: size [k], logpe [k] (0 for an empty community, -inf where a joined link has x_max = 0) */
int svils_ppc_get_communities(svils_ppc *h, uint64_t *size, double *logpe);
/* device milliseconds of the last draw, of the last list / CSR build and of the last statistics; -1: not run */
int svils_ppc_get_timing(svils_ppc *h, double ms[3]);
/* tiles per launch of the draw (0: all in one launch); no result depends on it */
int svils_ppc_set_tile_batch(svils_ppc *h, uint32_t tiles_per_launch);

/* -ppc-orig: the same handle under the K x K blockmodel of svils_orig, the device side of the
 * reference's MMSBOrig::gen / draw_and_save (src/mmsborig.cc:25-116) taken marginally over its two indicators.  The random
 * numbers, the statistics that name no community and every other entry point (svils_ppc_draw, _set_links, _stats, _get_links,
 * _get_nodes, _get_summary, _get_draw_counts, _get_timing, _set_tile_batch, svils_ppc_hop*) are the ones above; what changes:
 *   link       for p < q: x_gh = (pi_p[g] pi_q[h]) B[g][h], s = ONE running fp64 sum of x_gh over g ascending and, within
 *              g, h ascending, nothing contracted; y = (u < s).  The smaller id indexes the rows of B (draw_and_save visits
 *              i < j with rate beta[z_i][z_j]).  For a diagonal B every off-diagonal term adds an exact zero: s, and with it
 *              the whole draw, is the assortative one's bit for bit.  The tile kernel sums sum_h aq_p[h] pi_q[h] with
 *              aq_p[h] = sum_g pi_p[g] B[g][h] (fma, g ascending); a pair whose tile sum lies within
 *              (K^2 + 2 K + 18) DBL_EPSILON s of u is decided again with the definition's sum, and counted
 *   block      of a link: the first strict maximum x_max of x in row-major (g, h) order from (0, 0); colour = g K + h;
 *              ratio = x_max / s, joined unless ratio < 0.5 (a NaN ratio joins)
 *   statistics in place of size_k / logpe_k: bsize[g][h] = the joined links of block (g, h), blogpe[g][h] = the sum of
 *              log x_max over them in the same exact bins (0 for an empty block, -inf where a joined link has x_max = 0)
 * pi as svils_ppc_set_params; B [k][k] row-major, every entry finite and in [0, 1] (else SVILS_ERR_ARG), not necessarily
 * symmetric.  A handle of k < 2 or k > SVILS_ORIG_MAX_K: SVILS_ERR_UNSUPPORTED before any device call.  The first call
 * allocates B and 38 x k^2 counters.  A handle may change kinds at will: the last svils_ppc_set_params* decides, and it
 * invalidates the statistics, not the list.  svils_ppc_get_communities answers SVILS_ERR_ARG while the K x K kind is
 * current, svils_ppc_get_blocks while the assortative one is. */
int svils_ppc_set_params_orig(svils_ppc *h, const double *pi, const double *B);
/* after svils_ppc_stats under the K x K kind: bsize [k][k], blogpe [k][k] (either may be null) */
int svils_ppc_get_blocks(svils_ppc *h, uint64_t *bsize, double *blogpe);

/* -ppc-hops: the exact hop plot and the components of the current list, an undirected simple graph
 * on n nodes.  d(s, v) is the BFS distance (infinite across components, d(s, s) = 0).
 *   D[h]       ordered pairs (s, v) with d(s, v) = h: D[0] = n, D[1] = 2 links (SNAP's hop plot counts the self pairs);
 *              levels = the largest finite distance + 1; C[h] = D[0] + .. + D[h]
 *   ecc [n]    the largest finite d(s, .), 0 for an isolated node;  comp [n]: the smallest node id of v's component
 *   counts[6]  reachable = C[levels - 1] - n, diameter = levels - 1, components, the size of the largest one, isolated
 *              (nodes of degree 0), levels
 *   values[2]  effdiam: the 90th percentile of the hop plot, linearly interpolated as SNAP's CalcEffDiam -- t = 0.9 C[levels - 1],
 *              h* the smallest h with C[h] >= t, 0 if h* = 0, else (h* - 1) + (t - C[h* - 1]) / (C[h*] - C[h* - 1]) in fp64, in this
 *              order, nothing contracted;  meandist = (sum of h D[h]) / reachable, NaN when nothing is reachable
 * All-sources BFS, bit-parallel over sources in passes of 64 x words sources, one launch per level, integer atomics alone:
 * every integer is exact and the same for any batch.  ceil(n / (64 words)) x levels launches: a long-diameter graph is slow.
 * The results belong to the list they were computed for: a successful svils_ppc_draw / svils_ppc_set_links invalidates them
 * (the getters answer SVILS_ERR_ARG until svils_ppc_hops runs again); a draw that answers SVILS_ERR_NOMEM keeps them.
 * svils_ppc_hops needs neither parameters nor svils_ppc_stats and changes nothing of theirs; it synchronises.  The first call
 * allocates three tables of n x words 64-bit words (6 MiB at n = 32768, words = 8). */
int svils_ppc_hops(svils_ppc *h);
/* *levels, and D[0 .. min(levels, cap)) */
int svils_ppc_get_hops(svils_ppc *h, uint32_t *levels, uint64_t *D, uint32_t cap);
/* ecc [n], comp [n]; either may be null */
int svils_ppc_get_hop_nodes(svils_ppc *h, uint32_t *ecc, uint32_t *comp);
int svils_ppc_get_hop_summary(svils_ppc *h, uint64_t counts[6], double values[2]);
/* words per node of a pass (1 .. 8, else SVILS_ERR_ARG) and levels queued between two reads of the level counter (>= 1);
 * 0 restores that default (8 and 8).  No result depends on it */
int svils_ppc_set_hop_batch(svils_ppc *h, uint32_t words, uint32_t levels_per_chunk);
/* ms[0]: device milliseconds of the last svils_ppc_hops, ms[1]: the kernel launches it queued; both -1 before the first run */
int svils_ppc_get_hop_timing(svils_ppc *h, double ms[2]);

/* ---- options -------------------------------------------------------------------------------------------------------
 * Every tunable of the library is a row of ONE table: key, the SVILS_* environment variable that sets its default, the
 * built-in default, until when it may be changed on a handle, and what it does -- svils_option_table() returns it as
 * tab-separated text (one row per line, a header line first; DESIGN.md section 9 prints it).  The environment is read
 * when svils_create runs and at no other time (SVILS_RCCL_LIBRARY: at the first svils_comm_init of the process);
 * svils_set_option changes one option of one handle afterwards -- options consumed by svils_create ("environment only")
 * or by svils_set_graph ("before svils_set_graph") answer SVILS_ERR_ARG once it is too late.  Values are decimal
 * integers as text.  The reference has one knob of this kind, its command line (src/env.hh:13-110); none of these changes
 * a result beyond rounding (tests/test_gpu_parity.py runs the A/B forms against the oracle). */
int svils_set_option(svils_handle *h, const char *key, const char *value);
int svils_get_option(svils_handle *h, const char *key, char *value, size_t cap);
const char *svils_option_table(void);

const char *svils_last_error(void);
int svils_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif
