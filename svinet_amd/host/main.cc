// svinet -- command line of the MI355X link-sampling build.
//
// Accepts the reference's flag set (src/main.cc:114-242, same spelling, same
// positional/order-sensitive semantics: e.g. -link-sampling resets rfreq to 1,
// so -rfreq must follow it).  Engines: -link-sampling (the MI355X path), -findk (the
// estimate of the number of communities, also on the device), -gml / -lcstats (the
// link communities of a fitted model's gamma.txt / lambda.txt, on the device) and the
// reference's small all-pairs CPU engine -batch (plumbing only), with
// -batch-gpu, -rnode, -rpair, -rpair -stratified, -infset (with its -preprocess pass) and -snode the same model on the device, and
// -orig, the blockmodel with a full K x K matrix of block rates (MMSBInferOrig), on the device as well (with -clean-holdout
// it answers the link-prediction flags too), and -single, the single-membership stochastic blockmodel (SBM), on the device
// too; the
// flags that select the reference's other engines are recognised and rejected
// with a message instead of being silently ignored.  -adamic-adar (src/main.cc:173), which
// the reference wires to two of those engines, is here an option of the link-prediction
// flags of -link-sampling runs.
#include <csignal>
#include <cerrno>
#include <sys/stat.h>
#include <sys/wait.h>
#include <unistd.h>
#include <cstdio>
#include <ctime>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "env.hh"
#include "findk.hh"
#include "lcstats.hh"
#include "ppc.hh"
#include "sbm.hh"
#include "linksampling.hh"
#include "mmsbbatch.hh"
#include "mmsbinferorig.hh"
#include "util.hh"
#include "network.hh"

using namespace svinet;

static Env *env_global = nullptr;

static void term_handler(int sig) {   // src/main.cc:29-40
  if (env_global) {
    printf("\nGot signal. Saving model and groups.\n");
    fflush(stdout);
    env_global->terminate = 1;
  } else {
    signal(sig, SIG_DFL);
    raise(sig);
  }
}

// -gpus N, parent process: the ranks it forked (-1 once reaped); signals are passed on to them
static std::vector<pid_t> g_kids;
static void forward_handler(int sig) {
  for (pid_t k : g_kids)
    if (k > 0) kill(k, sig);
}

// The single-GPU tool modes refuse the flags of the fitting paths.  Every flag a mode may refuse, in the order the checks
// name them: a mode reports the first one set among its own.
enum : unsigned { F_BATCH = 1, F_GPUS = 2, F_KSHARD = 4, F_SHARDED = 8, F_MINIBATCH = 16, F_PAIRS = 32, F_RECOMMEND = 64, F_K2048 = 128,
                  F_RANKPAIRS = 256, F_RANKHELDOUT = 512, F_ADAMIC = 1024, F_LINKSAMPLING = 2048, F_FINDK = 4096, F_GML = 8192,
                  F_LCSTATS = 16384, F_RNODE = 32768, F_RPAIR = 65536, F_STRATIFIED = 131072 };

struct ToolMode {
  unsigned refuses;   // F_* bits
  const char *fmt;    // the refusal: %1$s the mode's flag, %2$s the refused flag
};
static const ToolMode kLinkCommunities = {   // -gml / -lcstats: one pass over a saved model
    F_GPUS | F_KSHARD | F_SHARDED | F_MINIBATCH | F_PAIRS | F_RECOMMEND | F_RANKPAIRS | F_RANKHELDOUT | F_ADAMIC,
    "error: %2$s is not available with %1$s (a single-GPU pass over gamma.txt / lambda.txt)\n"};
static const ToolMode kPosterior = {         // -ppc / -gen: replicates of a saved model, or one network from the prior
    F_BATCH | F_LINKSAMPLING | F_FINDK | F_GML | F_LCSTATS | F_RNODE | F_RPAIR | F_STRATIFIED | F_GPUS | F_KSHARD | F_SHARDED |
        F_MINIBATCH | F_PAIRS | F_RECOMMEND | F_RANKPAIRS | F_RANKHELDOUT | F_ADAMIC,
    "error: %2$s is not available with %1$s (a single-GPU tool: it fits nothing)\n"};
static const ToolMode kHops = {              // -ppc-hops: one more call per list of a -ppc run, and nothing else
    F_BATCH | F_LINKSAMPLING | F_FINDK | F_GML | F_LCSTATS | F_RNODE | F_RPAIR | F_STRATIFIED | F_GPUS | F_KSHARD | F_SHARDED |
        F_MINIBATCH | F_PAIRS | F_RECOMMEND | F_RANKPAIRS | F_RANKHELDOUT | F_ADAMIC,
    "error: %1$s is not available with %2$s (it adds the hop plot and the components to a -ppc run: it fits nothing)\n"};
static const ToolMode kFindK = {             // -findk: whole iterations
    F_GPUS | F_KSHARD | F_SHARDED | F_MINIBATCH | F_PAIRS | F_RECOMMEND | F_RANKPAIRS | F_RANKHELDOUT | F_ADAMIC,
    "error: %2$s is not available with %1$s (a single-GPU run)\n"};
static const ToolMode kPrediction = {        // -predict-pairs / -recommend / -rank-pairs / -rank-heldout after a fit
    F_BATCH | F_GPUS | F_KSHARD | F_SHARDED | F_K2048,
    "error: %1$s is not available with %2$s (single-GPU -link-sampling runs with -k <= 2048 only)\n"};
static const ToolMode kBaselines = {         // -adamic-adar beside them: sums in ascending device id, which -minibatch relabels
    F_MINIBATCH,
    "error: %1$s is not available with %2$s (the relabelled device ids would change the order in which a score is summed)\n"};

static const ToolMode kSampled = {           // -rnode / -rpair: an engine of its own on one GPU
    F_BATCH | F_LINKSAMPLING | F_FINDK | F_GML | F_LCSTATS | F_GPUS | F_KSHARD | F_SHARDED | F_MINIBATCH | F_PAIRS | F_RECOMMEND |
        F_RANKPAIRS | F_RANKHELDOUT | F_ADAMIC,
    "error: %1$s is not available with %2$s (an engine of its own: single GPU, its own output directory)\n"};

static const ToolMode kInfset = {            // -infset / -preprocess: an engine of its own on one GPU
    F_BATCH | F_LINKSAMPLING | F_FINDK | F_GML | F_LCSTATS | F_RNODE | F_RPAIR | F_STRATIFIED | F_GPUS | F_KSHARD | F_SHARDED |
        F_MINIBATCH | F_PAIRS | F_RECOMMEND | F_RANKPAIRS | F_RANKHELDOUT | F_ADAMIC,
    "error: %1$s is not available with %2$s (an engine of its own: single GPU, its own output directory)\n"};

static const ToolMode kSnode = {             // -snode: an engine of its own on one GPU
    F_BATCH | F_LINKSAMPLING | F_FINDK | F_GML | F_LCSTATS | F_RNODE | F_RPAIR | F_STRATIFIED | F_GPUS | F_KSHARD | F_SHARDED |
        F_MINIBATCH | F_PAIRS | F_RECOMMEND | F_RANKPAIRS | F_RANKHELDOUT | F_ADAMIC,
    "error: %1$s is not available with %2$s (an engine of its own: single GPU, its own output directory)\n"};

// -orig: an engine of its own on one GPU.  The link-prediction flags are not in this table: -orig answers them from its final
// state (svils_orig_link_prob / _predict_links / _rank_links), under the conditions of orig_queries_refused below.
// -adamic-adar stays refused: the neighbourhood baselines need the training CSR of a -link-sampling handle
static const ToolMode kOrig = {
    F_BATCH | F_LINKSAMPLING | F_FINDK | F_GML | F_LCSTATS | F_RNODE | F_RPAIR | F_STRATIFIED | F_GPUS | F_KSHARD | F_SHARDED |
        F_MINIBATCH | F_ADAMIC,
    "error: %1$s is not available with %2$s (an engine of its own: single GPU, its own output directory)\n"};

// -single: an engine of its own on one GPU; its graph form is always the sparse one
static const ToolMode kSingle = {
    F_BATCH | F_LINKSAMPLING | F_FINDK | F_GML | F_LCSTATS | F_RNODE | F_RPAIR | F_STRATIFIED | F_GPUS | F_KSHARD | F_SHARDED |
        F_MINIBATCH | F_PAIRS | F_RECOMMEND | F_RANKPAIRS | F_RANKHELDOUT | F_ADAMIC,
    "error: %1$s is not available with %2$s (an engine of its own: single GPU, its own output directory)\n"};

static const ToolMode kSparseGraph = {       // -sparse-graph: the sparse form of the device graph of -rnode / -rpair / -infset / -snode
    F_BATCH | F_LINKSAMPLING | F_FINDK | F_GML | F_LCSTATS,
    "error: %1$s is not available with %2$s (it is the graph form of the sampled engines on the GPU: -rnode, -rpair, -infset, -snode; "
    "the all-pairs passes and the other tools keep the dense form)\n"};

// true (the refusal printed) when a flag `mode` refuses is set
static bool refused(const Env::Args &a, const ToolMode &mode, const char *flag) {
  const struct { unsigned bit; bool set; const char *name; } flags[] = {
      {F_BATCH, a.batch, "-batch"},
      {F_LINKSAMPLING, a.link_sampling, "-link-sampling"},
      {F_FINDK, a.findk, "-findk"},
      {F_GML, a.gml, "-gml"},
      {F_LCSTATS, a.lcstats, "-lcstats"},
      {F_RNODE, a.rnode, "-rnode"},
      {F_RPAIR, a.rpair, "-rpair"},
      {F_STRATIFIED, a.stratified, "-stratified"},
      {F_GPUS, a.gpus > 1, "-gpus N > 1"},
      {F_KSHARD, a.kshard, "-kshard"},
      {F_SHARDED, a.sharded, "-sharded"},
      {F_MINIBATCH, a.minibatch != 0, "-minibatch"},
      {F_PAIRS, !a.predict_pairs_fname.empty(), "-predict-pairs"},
      {F_RECOMMEND, a.recommend != 0, "-recommend"},
      {F_RANKPAIRS, !a.rank_pairs_fname.empty(), "-rank-pairs"},
      {F_RANKHELDOUT, a.rank_heldout, "-rank-heldout"},
      {F_ADAMIC, a.adamic_adar, "-adamic-adar"},
      {F_K2048, a.k > 2048, "-k > 2048"},
  };
  for (const auto &f : flags)
    if ((mode.refuses & f.bit) && f.set) {
      fprintf(stderr, mode.fmt, flag, f.name);
      return true;
    }
  return false;
}

// -predict-pairs / -recommend / -rank-pairs / -rank-heldout beside -orig: true (the refusal printed) unless -clean-holdout is
// given and the run is on the device.  The first flag set is the one named
static bool orig_queries_refused(const Env::Args &a) {
  const struct { bool set; const char *name; } q[] = {{!a.predict_pairs_fname.empty(), "-predict-pairs"}, {a.recommend != 0, "-recommend"},
                                                      {!a.rank_pairs_fname.empty(), "-rank-pairs"}, {a.rank_heldout, "-rank-heldout"}};
  for (const auto &f : q) {
    if (!f.set) continue;
    if (!a.clean_holdout) {
      fprintf(stderr,
              "error: %s beside -orig needs -clean-holdout: the reference's sweep trains on the reverse orientation of every held-out "
              "pair and on both orientations of the validation pairs, so ranks and scores of those links would measure memorisation\n",
              f.name);
      return true;
    }
    if (a.host_loops) {
      fprintf(stderr, "error: %s is not available with -orig -host-loops (the link queries run on the GPU; there is no host path)\n", f.name);
      return true;
    }
  }
  return false;
}

static void usage() {
  fprintf(stdout,
          "\nSVINET (MI355X link-sampling build): stochastic variational inference of undirected networks\n"
          "svinet [OPTIONS]\n"
          "\t-help\t\tusage\n\n"
          "\t-file <name>\tinput tab-separated file with a list of undirected links\n\n"
          "\t-n <N>\t\tnumber of nodes in network\n\n"
          "\t-k <K>\t\tnumber of communities\n\n"
          "\t-link-sampling\tinference using link sampling (the MI355X engine of this build)\n\n"
          "\t-batch\t\trun batch variational inference over all pairs (host CPU, small graphs)\n\n"
          "\t-batch-gpu\t-batch with every sweep and pair likelihood on the GPU: same output directory and files, -k <= 256,\n"
          "\t\t\t-n <= 32768.  Single GPU; without one the run fails (no fall-back to the host engine)\n\n"
          "\t-rnode\t\tstochastic variational inference of the model of -batch, one random node per iteration: the\n"
          "\t\t\tn - 1 pairs of the node are the mini-batch.  On the GPU (-k <= 256, -n <= 32768 unless -sparse-graph; without one the run fails);\n"
          "\t\t\ta report every 100 iterations unless -rfreq came before it; step sizes -tau0 -kappa -nodetau0 -nodekappa\n\n"
          "\t-rpair\t\tthe same with n / 2 random pairs per iteration; not with -rnode\n\n"
          "\t-stratified\twith -rpair: mini-batches alternate between non-links and links (with -rnode or alone: refused)\n\n"
          "\t-nodelay\twith -rnode / -rpair: learn lambda from the first iteration (default: once iterations x n / 2 exceed the\n"
          "\t\t\tnumber of pairs)\n\n"
          "\t-host-loops\twith -rnode / -rpair / -infset / -snode / -orig / -single: the host CPU loops instead of the GPU (small graphs)\n\n"
          "\t-sparse-graph\twith -rnode / -rpair / -infset / -snode on the GPU: the device keeps the links and the held-out pairs as\n"
          "\t\t\tsorted adjacency rows, not as n x n bit matrices, and -n has no limit but the memory (-k <= 256 stays).\n"
          "\t\t\tThe same results bit for bit where both forms run.  Refused beside -batch, -batch-gpu, -logl, -orig, -ppc,\n"
          "\t\t\t-ppc-orig, -gen, -link-sampling, -findk, -gml, -lcstats, -preprocess and -host-loops, and without an engine\n\n"
          "\t-snode\t\tinference using stratified random node sampling (the reference's -stratified -rnode): an iteration\n"
          "\t\t\ttakes a random node with its links or, as often, with n / 10 of its non-links, and moves every row.\n"
          "\t\t\tOn the GPU (-k <= 256, -n <= 32768 unless -sparse-graph; without one the run fails); a report every 100 iterations unless\n"
          "\t\t\t-rfreq came before it; step sizes -tau0 -kappa -nodetau0 -nodekappa\n\n"
          "\t-infset\t\tinference using informative set sampling: an iteration takes a random node, its links and the\n"
          "\t\t\tnon-links -preprocess chose for it (rarely: 200 other non-links) and moves only their rows.  Reads neighbors.bin\n"
          "\t\t\tof the working directory.  On the GPU, a report interval per launch chain (-k <= 256, -n <= 32768 unless -sparse-graph; without\n"
          "\t\t\tone the run fails); give -rfreq (default 1: a report after every iteration)\n\n"
          "\t-preprocess\tpreprocess to run informative set sampling: writes neighbors.bin (per node up to 100 two-hop\n"
          "\t\t\tnon-neighbours) into the run's output directory and exits; host CPU, threaded\n\n"
          "\t-orig\t\tthe mixed-membership blockmodel with a full K x K matrix of block rates (Airoldi et al.): batch\n"
          "\t\t\tvariational inference over all ordered pairs, on the GPU (-k <= 64, -n <= 32768; without one the run fails,\n"
          "\t\t\t-host-loops runs the host CPU loops).  Needs -max-iterations N: N sweeps, then gamma.txt and beta.txt.\n"
          "\t\t\t-itype 0 (default) starts beta at random, -itype 1 from the link density\n\n"
          "\t-single\t\tthe single-membership stochastic blockmodel (a node belongs to one of K groups): batch variational\n"
          "\t\t\tinference, on the GPU in O((links + held-out pairs) K) per pass (-k <= 256, any -n the memory holds; without a GPU\n"
          "\t\t\tthe run fails, -host-loops runs the host CPU loops over all pairs).  Needs -max-iterations N: N iterations, then\n"
          "\t\t\tphi.txt, lambda.txt and gamma.txt.  Refused beside every other engine or tool flag, -infset (the sampled variant\n"
          "\t\t\tis not implemented), -sparse-graph (the engine is always sparse), -logl, -gpus N > 1, -scale and the link queries\n\n"
          "\t-single-logl\t-single with its variational lower bound, on the GPU in O((n + links + held-out pairs) K): a row of logl.txt\n"
          "\t\t\tafter the M-step of every iteration, and two stop rules on it: the bound below its maximum at more than 3\n"
          "\t\t\titerations past iteration 10 (writes max.txt), or a relative gain below 1e-5 (writes done.txt).  Either ends\n"
          "\t\t\tthe run with the model saved, precision.txt and hitcurve_0.txt written, so -max-iterations is optional (if\n"
          "\t\t\tgiven it still caps the run); -no-stop turns both rules off and needs -max-iterations.  Refused with\n"
          "\t\t\teverything -single is refused with\n\n"
          "\t-clean-holdout\twith -orig: leave both orientations of every held-out and every validation pair out of training\n"
          "\t\t\t(the reference leaves out the held-out pairs alone, and only in the orientation drawn).  With it -orig answers\n"
          "\t\t\t-predict-pairs, -recommend, -rank-pairs and -rank-heldout from its final state, on the GPU: the score of\n"
          "\t\t\t(p, q) is pi_p^T beta pi_q in the listed orientation, the files are those of -link-sampling runs;\n"
          "\t\t\t-rank-heldout ranks the links of heldout-edges.txt, then those of validation-edges.txt\n\n"
          "\t-findk\t\testimate the number of communities (label propagation over a top-5 sparse gamma, on the GPU);\n"
          "\t\t\tpick -k for -link-sampling from the lines of its communities.txt.  Single GPU; -k only sets alpha = 1/k\n\n"
          "\t-gml\t\tgenerate a GML format file that visualizes link communities: reads gamma.txt and lambda.txt of the\n"
          "\t\t\tworking directory (the output directory of a fit) and writes gml/network.gml with the link-community\n"
          "\t\t\tstatistics (community_stats.txt, node_bridgeness.txt, node_influence.txt, number_of_memberships.txt).\n"
          "\t\t\tSingle GPU\n\n"
          "\t-lcstats\tthe link-community statistics of -gml without network.gml, into the run's output directory\n\n"
          "\t-ppc\t\tposterior predictive checks: reads gamma.txt and lambda.txt of the working directory, draws\n"
          "\t\t\t-ppc-draws <R> (default 100) networks from the fitted model on the GPU and writes under ppc/ the observed\n"
          "\t\t\tand replicated statistics (obs.txt, rep.txt: links, density, degrees, triangles, transitivity, clustering),\n"
          "\t\t\tper-community sizes and log-likelihoods with z-scores (lc_size.txt, lc_logpe.txt) and summary.txt with\n"
          "\t\t\tposterior predictive p-values.  Every replicate draws pi ~ Dirichlet(gamma), beta ~ Beta(lambda) afresh;\n"
          "\t\t\t-ppc-mean uses the posterior means instead; -ppc-save <m> writes ppc/<r>/network.dat of the first m.\n"
          "\t\t\tThe random stream is Philox4x32-10 keyed by -seed and the replicate, not the reference's GSL stream:\n"
          "\t\t\tthat one is not reproduced.  -n <= 32768, -k <= 2048, single GPU, no host route\n\n"
          "\t-ppc-orig\t-ppc for the K x K blockmodel of an -orig fit: reads gamma.txt and beta.txt (K lines of K rates) of the\n"
          "\t\t\tworking directory; every replicate draws pi_i ~ Dirichlet(gamma_i), the block rates are the fit's point\n"
          "\t\t\testimate; pair p < q is a link with probability pi_p' B pi_q.  The files of -ppc, with ppc/block_size.txt\n"
          "\t\t\tand ppc/block_logpe.txt (g, h, observed, mean, deviation, z for all K x K blocks) in place of the lc_*\n"
          "\t\t\tfiles, and one more row of ppc/summary.txt: offdiag_share, the joined links in blocks g != h over the\n"
          "\t\t\tjoined links.  2 <= -k <= 64.  Takes -ppc-draws, -ppc-mean, -ppc-save, -ppc-hops and -seed; refused beside\n"
          "\t\t\t-ppc, -gen, -orig and every flag -ppc refuses\n\n"
          "\t-ppc-hops\twith -ppc: the exact hop plot and the components of the observed network and of every replicate\n"
          "\t\t\t(all-sources BFS on the GPU): obs-hop.txt and ppc/ppc-hop.txt (effective diameters, the reference's\n"
          "\t\t\tnames), ppc/obs-hops.txt (h, pairs at distance h, cumulative), ppc/rep-hops.txt (r, effective diameter,\n"
          "\t\t\tdiameter, mean distance, components, largest component, isolated nodes) and ppc/hops-summary.txt in the\n"
          "\t\t\tcolumns of ppc/summary.txt.  One launch per BFS level: a long-diameter network is slow.  Refused\n"
          "\t\t\twithout -ppc, with -gen and with every fitting flag\n\n"
          "\t-gen\t\tgenerate a network from the model (-n, -k, -seed): pi ~ Dirichlet(0.05), beta ~ Beta(4700.59, 0.77);\n"
          "\t\t\twrites gen/network_gen.dat, gen/pi-gen.txt, gen/beta-gen.txt.  The same stream and limits as -ppc;\n"
          "\t\t\t-gen -orig, -disjoint and -gp are not implemented\n\n"
          "\t-load-validation <fname>\tuse the pairs in the file as the validation set for convergence\n\n"
          "\t-load <dir>\tresume from <dir>gamma.txt / <dir>lambda.txt\n\n"
          "\t-label\t\ttag output directory\n\n"
          "\t-rfreq\t\tset the frequency at which convergence is estimated (give it after -link-sampling)\n\n"
          "\t-max-iterations\tmaximum number of iterations (use with -no-stop to avoid stopping earlier)\n\n"
          "\t-no-stop\tdisable stopping criteria\n\n"
          "\t-seed\t\tset random generator seed\n\n"
          "\t-heldout-ratio, -link-thresh, -lt-min-deg, -eta-type, -accuracy\tas in the reference\n\n"
          "\t-logl\t\twith -batch, -batch-gpu, -rnode, -rpair, -infset and -snode: the variational lower bound after the\n"
          "\t\t\tinitialisation and at every report (a row of logl.txt; with -accuracy the convergence rule\n"
          "\t\t\tthat writes done.txt); on the device unless -batch or -host-loops is given.\n"
          "\t\t\tWith -orig: the bound of the K x K blockmodel, P + N of the current state over the pairs a sweep\n"
          "\t\t\tvisits (the reference reads the vectors of the sweep before and adds the held-out pairs), a row\n"
          "\t\t\tof logl.txt after the initialisation and at every report, and two stop rules on it: the bound\n"
          "\t\t\tbelow its maximum at more than 3 reports past iteration 10 (writes max.txt), or a relative gain\n"
          "\t\t\tbelow 1e-5 (writes done.txt).  Either ends the run with the model saved, so -orig -logl needs no\n"
          "\t\t\t-max-iterations (if given it still caps the run); -no-stop turns both rules off.  About one\n"
          "\t\t\tsweep's pair pass per row.  Accepted and without effect with every other mode\n\n"
          "\t-strid\t\tnode names are strings (writes str2id.txt)\n\n"
          "\t-nmi <file>\tground-truth communities (\"node<TAB>community ...\" per line): the normalised mutual\n"
          "\t\t\tinformation of every communities.txt against it is appended to mutual.txt\n\n"
          "\t-device <d>\tHIP device ordinal (default 0)\n\n"
          "\t-gpus <N>\t-link-sampling over N GPUs of this node: one process per GPU (devices d .. d+N-1), node-block\n"
          "\t\t\tsharding, RCCL all-reduce / all-gather over xGMI between the phases of a sweep\n\n"
          "\t\t\twith -minibatch <m>: every GPU steps through windows of m nodes of its own block; per step an all-reduce\n"
          "\t\t\tof the K-vectors and broadcasts of the touched gamma rows (svils_step_sharded)\n\n"
          "\t-device-list <d0,d1,..>\tthe HIP device ordinal of every rank of a -gpus N run (default: d, d+1, ..)\n\n"
          "\t-sharded\ttake the -gpus N code path with one GPU as well (a communicator of one rank)\n\n"
          "\t-kshard\t\twith -gpus N: shard the K communities over the N GPUs (every GPU holds K/N columns of all rows;\n"
          "\t\t\tper sweep four all-reduces of O(links) doubles instead of an all-gather of the rows) -- the\n"
          "\t\t\tlayout for large K (-link-thresh < 0.5 adds two exchanges of one double per link: the arg-max tagging rule);\n"
          "\t\t\twith -minibatch <m> every GPU steps through the same windows of m nodes on its own columns\n\n"
          "\t-sweep-batch <b>\tsweeps per report chunk (default 0 = automatic: 1, 2, 4, 8, then 16 sweeps per report;\n\t\t\t\treports are written while the device sweeps on)\n\n"
          "\t-sparse-after <i>\tthe active-set branch of the phi pass is used once the iteration count exceeds i\n"
          "\t\t\t(default 1000, the reference's constant)\n\n"
          "\t-predict-pairs <file>\tlink prediction: score the pairs of <file> (\"id<TAB>id\" lines of external ids) with\n"
          "\t\t\tthe final state's link probability sum_z pi_pz pi_qz beta_z; writes link-prob.txt (id, id, y, probability)\n\n"
          "\t-recommend <k>\tlink prediction: the k (1 .. 256) most probable links of every node that are not training links,\n"
          "\t\t\tfrom the final state; writes recommendations.txt (one line per node, groups.txt order).  Both flags\n"
          "\t\t\tbelong to single-GPU -link-sampling runs with -k <= 2048, and to -orig -clean-holdout runs\n\n"
          "\t-rank-pairs <file>\tlink prediction: where each pair of <file> (\"id<TAB>id\" lines of external ids) stands among the\n"
          "\t\t\tcandidates -recommend chooses from, in both directions; writes link-ranks.txt (id_p, id_q, y, score, mid-rank of q\n"
          "\t\t\tamong p's candidates and their count, the same for p among q's) and link-ranks-summary.txt (per-link AUC, MRR, hits@k)\n\n"
          "\t-rank-heldout\tthe same for the held-out links of the run (the y = 1 pairs of validation-edges.txt and, with -load-test,\n"
          "\t\t\tof test-edges.txt); writes heldout-ranks.txt and link-ranks-summary.txt.  Where -recommend is available\n\n"
          "\t-adamic-adar\twith -predict-pairs, -rank-pairs or -rank-heldout: the same pairs scored and ranked from the training\n"
          "\t\t\tgraph alone, by common neighbours, Adamic-Adar (sum of 1 / log degree over them) and resource allocation; writes\n"
          "\t\t\tlink-nbr.txt (id, id, y, common neighbours, Adamic-Adar), link-ranks-aa.txt / heldout-ranks-aa.txt (the ranks by\n"
          "\t\t\tAdamic-Adar) and link-ranks-baselines.txt (the summary line of the model, cn, aa and ra).  Not with -minibatch\n\n"
          "\t-minibatch <m>\tmini-batch mode of -link-sampling: one step = the links of m randomly chosen nodes,\n"
          "\t\t\tRobbins-Monro step sizes (-tau0 -kappa -nodetau0 -nodekappa; defaults 1024 0.9 1024 0.5);\n"
          "\t\t\tgive -rfreq <steps> after -link-sampling to evaluate the stop rule every <steps> steps\n\n");
  fflush(stdout);
}

int main(int argc, char **argv) {
  signal(SIGTERM, term_handler);
  Env::Args a;
  bool unsupported = false;
  std::string unsupported_flag;
  if (argc == 1) {
    usage();
    exit(-1);
  }
  auto need = [&](int i) {
    if (i + 1 > argc - 1) {
      fprintf(stderr, "+ insufficient arguments!\n");
      exit(-1);
    }
  };
  for (int i = 1; i <= argc - 1; ++i) {
    const char *f = argv[i];
    auto is = [&](const char *s) { return strcmp(f, s) == 0; };
    if (is("-help")) { usage(); exit(0); }
    else if (is("-force") || is("-online")) {}
    else if (is("-nodelay")) { a.nodelay = true; }
    else if (is("-rnode")) { a.rnode = true; if (a.rfreq == 1) a.rfreq = 100; }   // src/main.cc:141-163
    else if (is("-rpair")) { a.rpair = true; if (a.rfreq == 1) a.rfreq = 100; }
    else if (is("-stratified")) { a.stratified = true; if (a.rfreq == 1) a.rfreq = 100; }
    else if (is("-host-loops")) { a.host_loops = true; }
    else if (is("-sparse-graph")) { a.sparse_graph = true; }
    else if (is("-scale")) { need(i); a.scale = atof(argv[++i]); }
    else if (is("-file")) { need(i); a.datfname = argv[++i]; }
    else if (is("-batch")) { a.batch = true; a.link_sampling = false; a.rfreq = 1; }
    else if (is("-batch-gpu")) { a.batch = true; a.batch_gpu = true; a.link_sampling = false; a.rfreq = 1; }
    else if (is("-link-sampling")) { a.link_sampling = true; a.batch = false; a.rfreq = 1; }
    else if (is("-findk")) { a.findk = true; }
    else if (is("-gml")) { a.gml = true; }
    else if (is("-lcstats")) { a.lcstats = true; }
    else if (is("-load")) { need(i); a.load = true; a.location = argv[++i]; }
    else if (is("-load-validation")) { need(i); a.val_load = true; a.val_file_location = argv[++i]; }
    else if (is("-load-test")) { need(i); a.test_load = true; a.test_file_location = argv[++i]; }
    else if (is("-n")) { need(i); a.n = atoi(argv[++i]); }
    else if (is("-k")) { need(i); a.k = atoi(argv[++i]); }
    else if (is("-label")) { need(i); a.label = argv[++i]; }
    else if (is("-nthreads")) { need(i); a.nthreads = atoi(argv[++i]); }
    else if (is("-eta-type")) { need(i); a.eta_type = argv[++i]; }
    else if (is("-nmi")) { need(i); a.ground_truth_fname = argv[++i]; a.nmi = true; }
    else if (is("-rfreq")) { need(i); a.rfreq = atoi(argv[++i]); }
    else if (is("-accuracy")) { a.accuracy = true; }
    else if (is("-logl")) { a.logl = true; }                 // src/main.cc:221-222: read by MMSBBatch (-batch, -rnode, -rpair, -infset) and MMSBInferOrig (-orig)
    else if (is("-max-iterations")) { need(i); a.max_iterations = atoi(argv[++i]); }
    else if (is("-no-stop")) { a.use_validation_stop = false; }
    else if (is("-seed")) { need(i); a.rand_seed = atof(argv[++i]); }
    else if (is("-heldout-ratio")) { need(i); a.hol_ratio = atof(argv[++i]); }
    else if (is("-link-thresh")) { need(i); a.link_thresh = atof(argv[++i]); }
    else if (is("-lt-min-deg")) { need(i); a.lt_min_deg = atof(argv[++i]); }
    else if (is("-strid")) { a.strid = true; }
    else if (is("-device")) { need(i); a.device = atoi(argv[++i]); }
    else if (is("-gpus")) { need(i); a.gpus = atoi(argv[++i]); }
    else if (is("-device-list")) {
      need(i);
      a.device_list.clear();
      for (const char *p = argv[++i]; *p;) {
        char *e = nullptr;
        a.device_list.push_back((int)strtol(p, &e, 10));
        if (e == p) { fprintf(stderr, "error: -device-list wants d0,d1,...\n"); return -1; }
        p = *e == ',' ? e + 1 : e;
      }
    }
    else if (is("-kshard")) { a.kshard = true; }
    else if (is("-sharded")) { a.sharded = true; }
    else if (is("-sweep-batch")) { need(i); a.sweep_batch = atoi(argv[++i]); }
    else if (is("-outdir")) { need(i); a.outdir_root = argv[++i]; }
    else if (is("-sparse-after")) { need(i); a.sparse_after = atoi(argv[++i]); }
    else if (is("-minibatch")) { need(i); a.minibatch = atoi(argv[++i]); }
    else if (is("-tau0")) { need(i); a.tau0 = atof(argv[++i]); }
    else if (is("-kappa")) { need(i); a.kappa = atof(argv[++i]); }
    else if (is("-nodetau0")) { need(i); a.nodetau0 = atof(argv[++i]); }
    else if (is("-nodekappa")) { need(i); a.nodekappa = atof(argv[++i]); }
    else if (is("-predict-pairs")) { need(i); a.predict_pairs_fname = argv[++i]; }
    else if (is("-rank-pairs")) { need(i); a.rank_pairs_fname = argv[++i]; }
    else if (is("-rank-heldout")) { a.rank_heldout = true; }
    else if (is("-adamic-adar")) { a.adamic_adar = true; }
    else if (is("-recommend")) { need(i); a.recommend = atoi(argv[++i]); if (a.recommend == 0) a.recommend = -1; }
    else if (is("-init-communities")) { need(i); a.init_comm = true; a.init_comm_fname = argv[++i]; }   // src/main.cc:237-239
    else if (is("-orig")) { a.orig = true; }                   // src/main.cc:187-188
    else if (is("-clean-holdout")) { a.clean_holdout = true; }
    else if (is("-itype")) { need(i); a.itype = atoi(argv[++i]); }   // :193-194: read by -orig alone
    else if (is("-stopthresh") || is("-inf") || is("-groups-file")) {
      need(i); ++i;   // value flags of other engines: consumed, no effect on this path
    }
    else if (is("-snode")) { a.snode = true; if (a.rfreq == 1) a.rfreq = 100; }   // as -rnode (src/main.cc:141-163)
    else if (is("-infset")) { a.infset = true; }             // src/main.cc:189-190, :214-216: rfreq stays as it is
    else if (is("-preprocess")) { a.preprocess = true; }
    else if (is("-randzeros")) {}                            // ignored: the informative sets are the two-hop ones
    else if (is("-ppc")) { a.ppc = true; }                   // src/main.cc:131-132, :139-140
    else if (is("-gen")) { a.gen = true; }
    else if (is("-ppc-draws")) { need(i); a.ppc_draws = atoi(argv[++i]); }
    else if (is("-ppc-save")) { need(i); a.ppc_save = atoi(argv[++i]); }
    else if (is("-ppc-mean")) { a.ppc_mean = true; }
    else if (is("-ppc-hops")) { a.ppc_hops = true; }
    else if (is("-ppc-orig")) { a.ppc_orig = true; }
    else if (is("-single")) { a.single = true; }               // src/main.cc:191-192
    else if (is("-single-logl")) { a.single = a.single_logl = true; }   // -single with the lower bound and its stop rules
    else if (is("-gp") || is("-disjoint") ||
             is("-load-test-sets")) {
      unsupported = true;
      unsupported_flag = f;
    }
    // unknown flags are ignored, as in the reference
  }
  const bool sampled = a.rnode || a.rpair;
  const bool infset = a.infset || a.preprocess;
  const bool ppc_plain = a.ppc;
  if (a.ppc_orig) a.ppc = true;                          // -ppc-orig: the -ppc mode plus the K x K kind (it does not set -orig)
  if (a.single && !unsupported) {                        // -single (SBM::batch_infer): an engine of its own; refusals before anything is read
    const char *flag = a.single_logl ? "-single-logl" : "-single";   // the same table for both
    if (refused(a, kSingle, flag)) return 2;
    const struct { bool set; const char *name; } more[] = {
        {a.batch_gpu, "-batch-gpu"}, {a.infset, "-infset"}, {a.preprocess, "-preprocess"}, {a.snode, "-snode"}, {a.orig, "-orig"},
        {a.ppc_orig, "-ppc-orig"}, {a.ppc, "-ppc"}, {a.gen, "-gen"}, {a.sparse_graph, "-sparse-graph"}, {a.logl, "-logl"}, {a.load, "-load"},
        {a.val_load, "-load-validation"}, {a.test_load, "-load-test"}, {a.init_comm, "-init-communities"}, {a.scale != 1, "-scale"}};
    for (const auto &m : more)
      if (m.set) {
        fprintf(stderr, kSingle.fmt, flag, m.name);
        return 2;
      }
    if (a.max_iterations == 0 && !(a.single_logl && a.use_validation_stop)) {   // -single-logl: the stop rules of the bound end the run
      fprintf(stderr, "error: -single needs -max-iterations N: the reference's loop never ends and its stop rule cannot fire\n");
      return 2;
    }
    if (!a.host_loops && a.k > SVILS_SBM_MAX_K) {        // the limit of svils_sbm_create
      fprintf(stderr, "error: -single holds -k <= %d (SVILS_SBM_MAX_K) unless -host-loops is given; -k %u is refused\n", SVILS_SBM_MAX_K, a.k);
      return 2;
    }
  }
  if (a.sparse_graph && !unsupported) {                  // -sparse-graph: refusals before anything is read or created
    const struct { bool set; const char *name; } more[] = {   // (-batch-gpu first: it sets -batch too, and is the flag to name)
        {a.batch_gpu, "-batch-gpu"}, {a.logl, "-logl"}, {a.orig, "-orig"}, {a.ppc_orig, "-ppc-orig"}, {a.ppc, "-ppc"}, {a.gen, "-gen"},
        {a.preprocess, "-preprocess"}, {a.host_loops, "-host-loops"}};
    for (const auto &m : more)
      if (m.set) {
        fprintf(stderr, kSparseGraph.fmt, "-sparse-graph", m.name);
        return 2;
      }
    if (refused(a, kSparseGraph, "-sparse-graph")) return 2;
    if (!(sampled || a.infset || a.snode)) {
      fprintf(stderr, "error: -sparse-graph belongs to -rnode, -rpair, -infset or -snode runs (alone it selects no engine)\n");
      return 2;
    }
  }
  if (a.ppc_hops && !unsupported) {                      // -ppc-hops: beside -ppc alone; refusals before anything is read or created
    if (refused(a, kHops, "-ppc-hops")) return 2;
    const struct { bool set; const char *name; } more[] = {
        {a.gen, "-gen"}, {a.orig, "-orig"}, {a.infset, "-infset"}, {a.preprocess, "-preprocess"}, {a.batch_gpu, "-batch-gpu"},
        {a.load, "-load"}, {a.snode, "-snode"}};
    for (const auto &m : more)
      if (m.set) {
        fprintf(stderr, kHops.fmt, "-ppc-hops", m.name);
        return 2;
      }
    if (!a.ppc) {
      fprintf(stderr, "error: -ppc-hops belongs to -ppc runs (the hop plot and the components of the observed network and of every replicate)\n");
      return 2;
    }
  }
  if ((a.ppc || a.gen) && !unsupported) {                // -ppc / -gen (MMSBGen): refusals before anything is read or created
    const char *flag = a.ppc_orig ? "-ppc-orig" : a.gen ? "-gen" : "-ppc";
    if (a.ppc_orig && (a.gen || ppc_plain)) {
      fprintf(stderr, "error: -ppc-orig is not available with %s (it is the -ppc of a K x K blockmodel: gamma.txt and beta.txt of an -orig fit)\n",
              a.gen ? "-gen" : "-ppc");
      return 2;
    }
    if (a.ppc && a.gen) {
      fprintf(stderr, "error: -gen is not available with -ppc (one draws from the prior, the other from a fitted model)\n");
      return 2;
    }
    if (refused(a, kPosterior, flag)) return 2;
    const struct { bool set; const char *name; } more[] = {
        {a.orig, "-orig"}, {a.infset, "-infset"}, {a.preprocess, "-preprocess"}, {a.batch_gpu, "-batch-gpu"}, {a.load, "-load"},
        {a.snode, "-snode"}};
    for (const auto &m : more)
      if (m.set) {
        fprintf(stderr, kPosterior.fmt, flag, m.name);
        return 2;
      }
    if (a.ppc_orig && (a.k < 2 || a.k > SVILS_ORIG_MAX_K)) {   // the limits of svils_ppc_set_params_orig
      fprintf(stderr, "error: -ppc-orig holds 2 <= -k <= %d (SVILS_ORIG_MAX_K); -k %u is refused\n", SVILS_ORIG_MAX_K, a.k);
      return 2;
    }
    if (a.k < 1 || a.k > SVILS_PPC_MAX_K) {              // the limits of svils_ppc_create
      fprintf(stderr, "error: %s holds 1 <= -k <= %d (SVILS_PPC_MAX_K); -k %u is refused\n", flag, SVILS_PPC_MAX_K, a.k);
      return 2;
    }
    if (a.n < 2 || a.n > SVILS_PPC_MAX_N) {
      fprintf(stderr, "error: %s holds 2 <= -n <= %d (SVILS_PPC_MAX_N); -n %u is refused\n", flag, SVILS_PPC_MAX_N, a.n);
      return 2;
    }
    if (a.ppc && (a.ppc_draws < 1 || a.ppc_save < 0)) {
      fprintf(stderr, "error: -ppc-draws wants a count >= 1 and -ppc-save a count >= 0\n");
      return 2;
    }
    if (a.gen) {                                         // src/main.cc:268-280: no network is read
      try {
        return run_gen(a.n, a.k, (uint32_t)a.rand_seed, a.device) < 0 ? -1 : 0;
      } catch (const SvilsError &e) {
        fprintf(stderr, "error: %s\n", e.what());
        return -1;
      }
    }
    for (const char *m : {"gamma.txt", a.ppc_orig ? "beta.txt" : "lambda.txt"}) {
      FILE *f = fopen(m, "r");
      if (!f) {
        fprintf(stderr, "error: %s needs %s in the working directory (the output directory of a fit): %s\n", flag, m, strerror(errno));
        return 2;
      }
      fclose(f);
    }
    a.write_files = false;                               // everything goes under ppc/ of the working directory; no run directory
  }
  if (a.snode && !unsupported) {                         // -snode (FastAMM2): an engine of its own; refusals before anything is read
    if (refused(a, kSnode, "-snode")) return 2;
    const struct { bool set; const char *name; } more[] = {{a.infset, "-infset"}, {a.preprocess, "-preprocess"}, {a.orig, "-orig"}};
    for (const auto &m : more)
      if (m.set) {
        fprintf(stderr, kSnode.fmt, "-snode", m.name);
        return 2;
      }
    if (a.scale != 1) {
      fprintf(stderr, "error: -snode is not available with -scale other than 1 (subsampling of the non-links is not implemented)\n");
      return 2;
    }
    if (!a.host_loops && a.k > SVILS_BATCH_MAX_K) {      // the limits of svils_batch_create, before anything is read
      fprintf(stderr, "error: -snode holds -k <= %d (SVILS_BATCH_MAX_K); -k %u is refused\n", SVILS_BATCH_MAX_K, a.k);
      return 2;
    }
    if (!a.host_loops && !a.sparse_graph && a.n > SVILS_BATCH_MAX_N) {
      fprintf(stderr, "error: -snode holds -n <= %d (SVILS_BATCH_MAX_N) unless -sparse-graph is given; -n %u is refused\n", SVILS_BATCH_MAX_N, a.n);
      return 2;
    }
    a.inf_epsilon = 0.5;                                 // _inf_epsilon of FastAMM2 (src/fastamm2.cc:15)
  }
  if (infset && !unsupported) {                          // -infset / -preprocess (FastAMM): an engine of its own
    const char *flag = a.preprocess ? "-preprocess" : "-infset";
    if (refused(a, kInfset, flag)) return 2;
    if (a.scale != 1) {
      fprintf(stderr, "error: %s is not available with -scale other than 1 (subsampling of the non-links is not implemented)\n", flag);
      return 2;
    }
    if (!a.preprocess && !a.host_loops && a.k > SVILS_BATCH_MAX_K) {   // the limits of svils_batch_create, before anything is read
      fprintf(stderr, "error: -infset holds -k <= %d (SVILS_BATCH_MAX_K); -k %u is refused\n", SVILS_BATCH_MAX_K, a.k);
      return 2;
    }
    if (!a.preprocess && !a.host_loops && !a.sparse_graph && a.n > SVILS_BATCH_MAX_N) {
      fprintf(stderr, "error: -infset holds -n <= %d (SVILS_BATCH_MAX_N) unless -sparse-graph is given; -n %u is refused\n", SVILS_BATCH_MAX_N, a.n);
      return 2;
    }
  }
  if (a.orig && !unsupported) {                          // -orig (MMSBInferOrig): an engine of its own; refusals before anything is read or created
    if (refused(a, kOrig, "-orig")) return 2;
    if (orig_queries_refused(a)) return 2;
    const struct { bool set; const char *name; } more[] = {
        {a.batch_gpu, "-batch-gpu"}, {a.infset, "-infset"}, {a.preprocess, "-preprocess"}, {a.load, "-load"},
        {a.val_load, "-load-validation"}, {a.test_load, "-load-test"}, {a.init_comm, "-init-communities"}, {a.scale != 1, "-scale"}};
    for (const auto &m : more)
      if (m.set) {
        fprintf(stderr, kOrig.fmt, "-orig", m.name);
        return 2;
      }
    if (a.max_iterations == 0 && !(a.logl && a.use_validation_stop)) {   // -orig -logl: the stop rules of the bound end the run
      fprintf(stderr, "error: -orig needs -max-iterations N: the reference's loop never ends and its stop rule is compiled out\n");
      return 2;
    }
    if (!a.host_loops && a.k > SVILS_ORIG_MAX_K) {       // the limits of svils_orig_create
      fprintf(stderr, "error: -orig holds -k <= %d (SVILS_ORIG_MAX_K) unless -host-loops is given; -k %u is refused\n", SVILS_ORIG_MAX_K, a.k);
      return 2;
    }
    if (!a.host_loops && a.n > SVILS_ORIG_MAX_N) {
      fprintf(stderr, "error: -orig holds -n <= %d (SVILS_ORIG_MAX_N) unless -host-loops is given; -n %u is refused\n", SVILS_ORIG_MAX_N, a.n);
      return 2;
    }
  }
  if (a.clean_holdout && !a.orig) {                      // the other engines hold their pairs out in both orientations already
    fprintf(stderr, "error: -clean-holdout belongs to -orig runs (it changes which pairs the sweep of that engine leaves out)\n");
    return 2;
  }
  if (a.stratified && !sampled && !unsupported) {        // alone, or beside another engine: the reference's stratified engines
    unsupported = true;
    unsupported_flag = "-stratified";
  }
  if (unsupported || !(a.batch || a.link_sampling || a.findk || a.gml || a.lcstats || a.ppc || sampled || infset || a.orig || a.snode || a.single)) {
    fprintf(stderr,
            "svinet (MI355X build): only the -link-sampling and -batch engines are implemented here (and -findk, -gml, -lcstats)%s%s.\n"
            "Use the reference build for the other engines.\n",
            unsupported ? "; unsupported option " : "", unsupported ? unsupported_flag.c_str() : "");
    return 2;
  }
  if (sampled) {                                         // -rnode / -rpair / -rpair -stratified (MMSBInfer::infer)
    const char *flag = a.rnode ? "-rnode" : "-rpair";
    if (a.rnode && a.stratified) {
      fprintf(stderr, "error: -stratified -rnode is a different engine of the reference (FastAMM2) and is not implemented here under these flags: use -snode\n");
      return 2;
    }
    if (a.rnode && a.rpair) {
      fprintf(stderr, "error: -rnode is not available with -rpair (one engine per run)\n");
      return 2;
    }
    if (refused(a, kSampled, flag)) return 2;
    if (a.scale != 1) {
      fprintf(stderr, "error: %s is not available with -scale other than 1 (subsampling of the non-links is not implemented)\n", flag);
      return 2;
    }
    if (!a.host_loops && a.k > SVILS_BATCH_MAX_K) {      // the limits of svils_batch_create, before anything is read
      fprintf(stderr, "error: %s holds -k <= %d (SVILS_BATCH_MAX_K); -k %u is refused\n", flag, SVILS_BATCH_MAX_K, a.k);
      return 2;
    }
    if (!a.host_loops && !a.sparse_graph && a.n > SVILS_BATCH_MAX_N) {
      fprintf(stderr, "error: %s holds -n <= %d (SVILS_BATCH_MAX_N) unless -sparse-graph is given; -n %u is refused\n", flag, SVILS_BATCH_MAX_N, a.n);
      return 2;
    }
  }
  if (a.gml || a.lcstats) {
    const char *flag = a.lcstats ? "-lcstats" : "-gml";   // the reference runs -lcstats when both are given (src/main.cc:307-318)
    if (refused(a, kLinkCommunities, flag)) return 2;
    for (const char *m : {"gamma.txt", "lambda.txt"}) {   // the reference asserts on a missing model (src/mmsbgen.cc:79-81)
      FILE *f = fopen(m, "r");
      if (!f) {
        fprintf(stderr, "error: %s needs %s in the working directory (the output directory of a fit): %s\n", flag, m, strerror(errno));
        return 2;
      }
      fclose(f);
    }
    if (a.k < 2) {
      fprintf(stderr, "error: %s needs -k >= 2\n", flag);
      return 2;
    }
  }
  if (a.findk && refused(a, kFindK, "-findk")) return 2;
  if (a.batch_gpu) {                                     // the limits of svils_batch_create, before anything is read
    if (a.k > SVILS_BATCH_MAX_K) {
      fprintf(stderr, "error: -batch-gpu holds -k <= %d (SVILS_BATCH_MAX_K); -k %u is refused\n", SVILS_BATCH_MAX_K, a.k);
      return 2;
    }
    if (a.n > SVILS_BATCH_MAX_N) {
      fprintf(stderr, "error: -batch-gpu holds -n <= %d (SVILS_BATCH_MAX_N); -n %u is refused\n", SVILS_BATCH_MAX_N, a.n);
      return 2;
    }
  }
  if (a.adamic_adar) {                                   // baselines of link ranks (svils_nbr_score / svils_nbr_rank)
    if (refused(a, kPrediction, "-adamic-adar") || refused(a, kBaselines, "-adamic-adar")) return 2;
    if (!a.link_sampling || (a.predict_pairs_fname.empty() && a.rank_pairs_fname.empty() && !a.rank_heldout)) {
      fprintf(stderr, "error: -adamic-adar belongs to -link-sampling runs with -predict-pairs, -rank-pairs or -rank-heldout\n");
      return 2;
    }
  }
  if (!a.predict_pairs_fname.empty() || a.recommend) {   // link prediction (svils_link_prob / svils_predict_links)
    const char *flag = a.recommend ? "-recommend" : "-predict-pairs";
    if (a.recommend && (a.recommend < 1 || a.recommend > 256)) {
      fprintf(stderr, "error: -recommend wants a count of 1 .. 256 links per node\n");
      return 2;
    }
    if (refused(a, kPrediction, flag)) return 2;
    if (!a.predict_pairs_fname.empty()) {
      FILE *f = fopen(a.predict_pairs_fname.c_str(), "r");
      if (!f) {
        fprintf(stderr, "error: cannot read -predict-pairs file %s\n", a.predict_pairs_fname.c_str());
        return 2;
      }
      fclose(f);
    }
  }
  if (!a.rank_pairs_fname.empty() || a.rank_heldout) {   // ranks of given links (svils_rank_links)
    if (refused(a, kPrediction, a.rank_heldout ? "-rank-heldout" : "-rank-pairs")) return 2;
    if (!a.rank_pairs_fname.empty()) {
      FILE *f = fopen(a.rank_pairs_fname.c_str(), "r");
      if (!f) {
        fprintf(stderr, "error: cannot read -rank-pairs file %s\n", a.rank_pairs_fname.c_str());
        return 2;
      }
      fclose(f);
    }
  }
  if (a.kshard && !a.link_sampling) {
    fprintf(stderr, "error: -kshard belongs to -link-sampling runs\n");
    return -1;
  }
  if (a.n == 0 || a.k == 0) {
    fprintf(stderr, "error: -n and -k are required\n");
    return -1;
  }

  if (a.gpus < 1) {
    fprintf(stderr, "error: -gpus needs a positive count\n");
    return -1;
  }
  if (a.kshard && (uint32_t)a.gpus > a.k) {
    fprintf(stderr, "error: -kshard needs at least one community per GPU\n");
    return -1;
  }
  if (!a.device_list.empty() && (int)a.device_list.size() != a.gpus) {
    fprintf(stderr, "error: -device-list names %d devices for -gpus %d\n", (int)a.device_list.size(), a.gpus);
    return -1;
  }
  if (a.gpus == 1 && !a.device_list.empty()) a.device = a.device_list[0];

  // -gpus N: fork one process per GPU before anything touches the HIP runtime.  Every rank reads the
  // graph and runs the (seeded, deterministic) host-side initialisation itself; rank 0 owns the output
  // directory and the files, the others compute their node block (or column slice) only.  The communicator
  // id goes from rank 0 to rank r through a pipe made here.
  if (a.link_sampling && a.gpus > 1 && !a.gml && !a.lcstats) {
    // RCCL shares device buffers between the ranks' processes: the host driver of this GPU pool only supports dmabuf
    // IPC (without it: hipIpcGetMemHandle: invalid argument).  The runtime reads the variable when HIP is first
    // touched -- in the ranks, after the fork below; a value the user exported stays.
    setenv("HSA_ENABLE_IPC_MODE_LEGACY", "0", 0);
    std::vector<int> rfds((size_t)a.gpus, -1), wfds((size_t)a.gpus, -1);
    for (int r = 1; r < a.gpus; ++r) {
      int fd[2];
      if (pipe(fd)) { perror("pipe"); return -1; }
      rfds[r] = fd[0];
      wfds[r] = fd[1];
    }
    const int dev0 = a.device;
    for (int r = 0; r < a.gpus; ++r) {
      const pid_t pid = fork();
      if (pid < 0) {
        perror("fork");
        for (pid_t k : g_kids) kill(k, SIGKILL);
        return -1;
      }
      if (pid == 0) {
        g_kids.clear();
        a.rank = r;
        a.device = a.device_list.empty() ? dev0 + r : a.device_list[r];
        if (r > 0) a.write_files = false;
        for (int q = 1; q < a.gpus; ++q) {   // keep only the ends this rank uses
          if (r == 0) a.comm_wfds.push_back(wfds[q]); else close(wfds[q]);
          if (q == r) a.comm_rfd = rfds[q]; else close(rfds[q]);
        }
        goto run;
      }
      g_kids.push_back(pid);
    }
    for (int q = 1; q < a.gpus; ++q) { close(rfds[q]); close(wfds[q]); }
    // SIGTERM (the reference's "save the model" signal) and SIGINT go on to the ranks; they agree among themselves
    // at their next poll (LinkSampling::sweep_loop)
    signal(SIGTERM, forward_handler);
    signal(SIGINT, forward_handler);
    // reap in the order the ranks finish: the first one that fails takes the others with it, because they would
    // wait in a collective for ever; only pids not reaped yet are signalled
    int rc = 0;
    size_t left = g_kids.size();
    while (left) {
      int st = 0;
      const pid_t pid = waitpid(-1, &st, 0);
      if (pid < 0) {
        if (errno == EINTR) continue;
        break;
      }
      bool ours = false;
      for (pid_t &k : g_kids)
        if (k == pid) { k = -1; ours = true; }
      if (!ours) continue;
      --left;
      const int code = WIFEXITED(st) ? WEXITSTATUS(st) : 128 + (WIFSIGNALED(st) ? WTERMSIG(st) : 0);
      if (code != 0 && rc == 0) {
        rc = code;
        for (pid_t k : g_kids)
          if (k > 0) kill(k, SIGKILL);
      }
    }
    return rc;
  }
run:
  Env env(a);
  env_global = &env;
  Network network(env);
  timespec t_read0, t_read1;
  clock_gettime(CLOCK_MONOTONIC, &t_read0);
  if (network.read(a.datfname) < 0) {
    fprintf(stderr, "error reading %s; quitting\n", a.datfname.c_str());
    return -1;
  }
  clock_gettime(CLOCK_MONOTONIC, &t_read1);
  env.n = network.n() - network.singles();   // src/main.cc:291
  if (network.ones() == 0 || env.n < 2) {
    fprintf(stderr, "error: no links read from %s; quitting\n", a.datfname.c_str());
    return -1;
  }
  try {                                      // the device tools: a failed svils_* call ends the run here
    if (a.lcstats || a.gml) {                // src/main.cc:307-318, before -findk and the other engines
      if (a.lcstats) {
        printf("+ computing lc stats\n");
        unlink("ppc");                       // MMSBGen(env, network, true) makes ppc/ in the working directory
        mkdir("ppc", S_IRWXU | S_IRWXG | S_IROTH | S_IXOTH);
      } else {
        printf("+ generating GML file\n");
      }
      fflush(stdout);
      LinkCommunities lc(env, network);
      if (lc.load_model() < 0) return -1;
      lc.run();
      lc.write_stats();
      if (!a.lcstats) lc.write_gml();
      if (const char *tf = getenv("SVINET_TIMING_FILE")) {   // where the time went (tools/gml_bench.py)
        if (FILE *f = fopen(tf, "w")) {
          const double *ms = lc.timing_ms();
          fprintf(f, "{\"node_ms\": %.4f, \"link_ms\": %.4f, \"count_ms\": %.4f, \"links\": %u, \"unlikely\": %llu, "
                     "\"gml_edges\": %llu, \"rechecked\": %llu}\n", ms[0], ms[1], ms[2], network.ones(),
                  (unsigned long long)lc.unlikely(), (unsigned long long)lc.gml_edges(), (unsigned long long)lc.rechecked());
          fclose(f);
        }
      }
      exit(0);
    }
    if (a.ppc) {                             // src/main.cc:298-304
      printf("+ generating networks for posterior predictive checks\n");
      fflush(stdout);
      PpcOptions po;
      po.draws = (uint32_t)a.ppc_draws;
      po.seed = (uint32_t)a.rand_seed;
      po.save = (uint32_t)a.ppc_save;
      po.mean = a.ppc_mean;
      po.hops = a.ppc_hops;
      po.orig = a.ppc_orig;
      exit(run_ppc(env, network, po) < 0 ? 255 : 0);
    }
    if (a.findk) {                           // src/main.cc:321-327, before the other engines (-batch / -link-sampling only name the directory)
      FindK(env, network).run();
      exit(0);
    }
  } catch (const SvilsError &e) {
    fprintf(stderr, "error: %s\n", e.what());
    return -1;
  }
  if (a.preprocess) {                        // src/network.cc:148-151: <outdir>/neighbors.bin, then exit
    const std::string out = Env::file_str("/neighbors.bin");
    if (!network.write_neighborhood_sets(out)) {
      fprintf(stderr, "error: cannot write %s: %s\n", out.c_str(), strerror(errno));
      return -1;
    }
    printf("+ wrote %s\n", out.c_str());
    exit(0);
  }
  if (infset) {                              // src/network.cc:151-152, :689-696: neighbors.bin of the working directory
    const int rc = network.load_neighborhood_sets("neighbors.bin");
    if (rc == -1) {
      fprintf(stderr, "error: cannot find neighbors.bin from preprocessing the network\n");
      return -1;
    }
    if (rc) {
      fprintf(stderr, "error: neighbors.bin does not belong to this network (run -preprocess on the same file and -n)\n");
      return -1;
    }
  }
  if (a.orig) {                              // src/main.cc:330-334 (Airoldi et al.)
    printf("+ running mmsb orig inference\n");
    try {                                    // the device backend: a failed svils_orig_* call ends the run (no host fall-back)
      MMSBInferOrig mmsb(env, network, a.itype);
      mmsb.batch_infer();
    } catch (const SvilsError &e) {
      fprintf(stderr, "error: %s\n", e.what());
      return -1;
    }
    exit(0);
  }
  if (a.single) {                            // src/main.cc:344-352
    printf("+ running stochastic blockmodel inference\n");
    try {                                    // the device backend: a failed svils_sbm_* call ends the run (no host fall-back)
      SBM sbm(env, network);
      sbm.batch_infer();
    } catch (const SvilsError &e) {
      fprintf(stderr, "error: %s\n", e.what());
      return -1;
    }
    exit(0);
  }
  if (a.batch || sampled || infset || a.snode) {   // src/main.cc:354-358; -rnode / -rpair: :373-377; -infset: :361-366; -snode: :368-372
    printf(a.snode ? "+ running mmsb inference (with stratified random node option)\n" : infset ? "+ running mmsb inference (with infset network option)\n" : sampled ? "+ running mmsb inference\n" : "+ running mmsb batch inference\n");
    try {                                    // the device backends: a failed svils_batch_* call ends the run (no host fall-back)
      MMSBBatch mmsb(env, network);
      if (sampled || infset || a.snode) mmsb.infer(); else mmsb.batch_infer();
    } catch (const SvilsError &e) {
      fprintf(stderr, "error: %s\n", e.what());
      return -1;
    }
    exit(0);
  }
  LinkSampling ls(env, network);
  const int how = ls.infer();
  if (const char *tf = getenv("SVINET_TIMING_FILE")) {   // where the wall time went (bench.py's cli_end_to_end record)
    if (FILE *f = fopen(tf, "w")) {
      const LinkSampling::Timing &t = ls.timing();
      fprintf(f, "{\"read_s\": %.6f, \"ctor_s\": %.6f, \"graph_upload_s\": %.6f, \"sweeps_s\": %.6f, \"sweeps\": %u, \"chunks\": %u, "
                 "\"reports\": %u, \"communities_written\": %u, \"report_host_s\": %.6f, \"final_files_s\": %.6f, \"pipelined\": %s, "
                 "\"ended_by\": \"%s\"}\n",
              (double)(t_read1.tv_sec - t_read0.tv_sec) + 1e-9 * (double)(t_read1.tv_nsec - t_read0.tv_nsec), t.ctor_s, t.graph_upload_s,
              t.sweeps_t1 - t.sweeps_t0, t.sweeps, t.chunks, t.reports, t.communities_written, t.report_host_s, t.final_files_s,
              t.pipelined ? "true" : "false", how == 1 ? "stop rule" : "max iterations");
      fclose(f);
    }
  }
  exit(0);
}
