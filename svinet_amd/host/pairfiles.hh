// pairfiles.hh -- the pair lists the link-prediction flags read and the files they write, for both engines that answer
// them: LinkSampling (-link-sampling: svils_link_prob / svils_predict_links / svils_rank_links, and the neighbourhood
// baselines) and MMSBInferOrig (-orig -clean-holdout: svils_orig_link_prob / _predict_links / _rank_links).  The engine
// makes the library calls; the formats live here, once.
//
//   link-prob.txt            one line per -predict-pairs line, in input order: id_a, id_b, the network's y, the score
//   recommendations.txt      one line per node in groups.txt order: the node's id, then id and score of each of its
//                            -recommend best candidates; an empty slot reads -1 -1.000000000e+00
//   link-ranks.txt / heldout-ranks.txt (and their -aa namesakes): id_p, id_q, the network's y, the score of (p, q), the
//                            mid-rank of q among p's candidates (above + 1 + tied / 2, "%.3f") and their count, the same
//                            for p among q's
//   link-ranks-summary.txt   a header and one line of values over the directed pairs (p -> q, then q -> p, in file order) of
//                            the lines with y = 1 whose pair is held out; a direction without a candidate is left out.  The
//                            means are sequential double sums in that order
#pragma once
#include <cstdint>
#include <cstdio>
#include <functional>
#include <string>
#include <vector>

#include "network.hh"

namespace svinet {

// -predict-pairs / -rank-pairs: "id<TAB>id" lines of external ids, parsed like -load-test; an unknown id or a pair of one node
// ends the run (status 2)
void load_pairs_file(const Network &network, const char *flag, const std::string &fname, std::vector<int> *ext, std::vector<uint32_t> *seq);

// seq [m][2] sequence ids, ext [m][2] the ids as they were given, prob [m]
void write_link_prob(const Network &network, const std::vector<int> &ext, const std::vector<uint32_t> &seq, const std::vector<double> &prob);

// ids / sc [n][k] as svils_predict_links fills them; seq_of: the sequence id behind a listed id (null: the ids are sequence ids)
void write_recommendations(const Network &network, uint32_t n, uint32_t k, const std::vector<uint32_t> &ids, const std::vector<double> &sc,
                           const std::vector<uint32_t> *seq_of);

// the summary of one ranking: sequential sums over the directed pairs in file order
struct RankSum {
  uint64_t cnt = 0, h1 = 0, h10 = 0, h100 = 0;
  double auc = .0, mrr = .0, chance = .0;
  void add(uint32_t above, uint32_t tied, uint32_t ncand);
  void print(FILE *f) const;   // the line of values
};

// the directed pairs of a list seq [m][2]: (p, q), (q, p) per line -> [2m][2]; map: an id's relabelling (null: none)
std::vector<uint32_t> directed_pairs(const std::vector<uint32_t> &seq, const std::function<uint32_t(uint32_t)> &map);

// One rank file from the answers above / tied / ncand / sc [2m] to directed_pairs(seq); ext: the ids as they were given
// (null: the network's ids); held_out(p, q): whether the line counts towards the summary when y = 1; fname: the per-pair
// file under the output directory, "/name" (null: the summary only).  Returns the summary.
RankSum write_rank_file(const Network &network, const char *fname, const std::vector<uint32_t> &seq, const std::vector<int> *ext,
                        const std::vector<uint32_t> &above, const std::vector<uint32_t> &tied, const std::vector<uint32_t> &ncand,
                        const std::vector<double> &sc, const std::function<bool(uint32_t, uint32_t)> &held_out);

// link-ranks-summary.txt
void write_rank_summary(const RankSum &sum);

}  // namespace svinet
