// findk.cc -- -findk (src/fastinit.cc, src/fastinit.hh).  See findk.hh.
#include "findk.hh"

#include <algorithm>
#include <cerrno>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "svils.h"
#include "util.hh"

namespace svinet {

// FastInit::FastInit, src/fastinit.cc:8-156
FindK::FindK(Env &env, Network &network, bool attach_device)
    : env_(env), network_(network), n_(env.n), rng_(0), start_time_(time(0)) {
  // FastInit never calls gsl_rng_set: the default seed whatever -seed says (-seed still names the directory)
  // `_n * (_n - 1) / 2` in 32-bit unsigned arithmetic (:41-45); _ones_prob / _zeros_prob are never assigned in the
  // reference (fastinit.hh:121-122): defined here as LinkSampling defines them
  total_pairs_ = (double)((uint32_t)(n_ * (n_ - 1u)) / 2u);
  ones_prob_ = double(network_.ones()) / total_pairs_;
  zeros_prob_ = 1 - ones_prob_;
  printf("+ Estimating communities on input network with %d nodes\n", n_);
  Env::plog("inference n", n_);
  Env::plog("total pairs", total_pairs_);
  if (env_.write_files) {
    for (const char *f : {"/validation-edges.txt", "/training-edges.txt", "/stats.txt"}) fclose(open_or_die(Env::file_str(f), f + 1));
    uf_ = open_or_die(Env::file_str("/uncolored-links.txt"), "uncolored links");
  }
  init_gamma();
  if (env_.write_files) {
    for (const char *f : {"/time.txt", "/convergence.txt", "/cmap.txt", "/validation.txt", "/training.txt", "/logl.txt",
                          "/modularity.txt"})
      fclose(open_or_die(Env::file_str(f), f + 1));
    hf_ = open_or_die(Env::file_str("/heldout.txt"), "heldout");
  }
  Env::plog("network ones", network_.ones());
  Env::plog("network singles", network_.singles());
  start_time_ = time(0);
  init_heldout();
  if (env_.nmi) {   // Network::load_ground_truth / write_gt_communities (src/network.cc:252-307,508-525)
    if (!read_cover_memberships(env_.ground_truth_fname, &ground_truth_)) {
      fprintf(stderr, "error: cannot read ground truth file %s; check path; skipping file\n", env_.ground_truth_fname.c_str());
    } else if (env_.write_files) {
      FILE *f = open_or_die(Env::file_str("/ground_truth.txt"), "ground truth");
      FILE *g = open_or_die(Env::file_str("/ground_truth_community_sizes.txt"), "ground truth sizes");
      uint32_t c = 0;
      for (const auto &v : ground_truth_) {
        fprintf(g, "%d\t%ld\n", c++, (long)v.size());
        for (uint32_t id : v) fprintf(f, "%d ", id);
        fprintf(f, "\n");
      }
      fclose(f);
      fclose(g);
    }
  }
  ext_order_.resize(n_);
  for (uint32_t i = 0; i < n_; ++i) ext_order_[i] = i;
  const std::vector<uint32_t> &s2i = network_.seq2id();
  std::sort(ext_order_.begin(), ext_order_.end(), [&](uint32_t a, uint32_t b) { return s2i[a] < s2i[b]; });
  if (attach_device) attach();
}

FindK::~FindK() {
  if (h_) svils_findk_destroy(h_);
  if (hf_) fclose(hf_);
  if (uf_) fclose(uf_);
}

// init_gamma, :178-190
void FindK::init_gamma() {
  labels_.resize((size_t)n_ * S);
  values_.resize((size_t)n_ * S);
  for (uint32_t i = 0; i < n_; ++i) {
    labels_[(size_t)i * S] = i;
    values_[(size_t)i * S] = 1.0 + rng_.uniform();
    for (uint32_t j = 1; j < S; ++j) {
      labels_[(size_t)i * S + j] = (i + j) % n_;
      values_[(size_t)i * S + j] = rng_.uniform();
    }
  }
}

bool FindK::edge_ok(const Edge &e) const {   // src/fastinit.hh:478-488
  return e.first != e.second && heldout_map_.find(e) == heldout_map_.end();
}

void FindK::get_random_edge(bool link, Edge &e) {   // src/fastinit.hh:491-512
  if (!link) {
    do {
      uint32_t a = rng_.uniform_int(n_);
      uint32_t b = rng_.uniform_int(n_);
      e = a < b ? Edge(a, b) : Edge(b, a);
    } while (!edge_ok(e));
  } else {
    do {
      e = network_.edges()[rng_.uniform_int(network_.ones())];
    } while (!edge_ok(e));
  }
}

// init_heldout / set_heldout_sample, :467-508
void FindK::init_heldout() {
  const int s = env_.heldout_ratio * network_.ones();
  if (!env_.accuracy) {
    int c0 = 0, c1 = 0;
    const int p = s / 2;
    while (c0 < p || c1 < p) {
      Edge e;
      get_random_edge(c0 == p, e);
      const bool y = network_.y(e.first, e.second);
      if (!y && c0 < p) { c0++; heldout_map_[e] = true; }
      if (y && c1 < p) { c1++; heldout_map_[e] = true; }
    }
  }
  Env::plog("heldout ratio", env_.heldout_ratio);
  Env::plog("heldout edges (1s and 0s)", (uint32_t)heldout_map_.size());
  for (const auto &kv : heldout_map_) {
    held_.push_back(kv.first.first);
    held_.push_back(kv.first.second);
    held_.push_back(network_.y(kv.first.first, kv.first.second) ? 1u : 0u);
  }
  if (env_.write_files) {   // it prints _heldout_edges, which nothing fills
    FILE *f = open_or_die(Env::file_str("/heldout-edges.txt"), "heldout edges");
    fprintf(f, "\n");
    fclose(f);
  }
}

void FindK::attach() {
  int rc = svils_findk_create(env_.device, n_, env_.alpha, env_.link_thresh, &h_);
  if (rc) throw_svils("svils_findk_create", rc);
  const std::vector<Edge> &ed = network_.edges();
  std::vector<uint32_t> links(2 * ed.size());
  std::vector<uint8_t> held(ed.size(), 0);
  for (size_t x = 0; x < ed.size(); ++x) {
    links[2 * x] = ed[x].first;
    links[2 * x + 1] = ed[x].second;
    held[x] = heldout_map_.count(ed[x]) ? 1 : 0;
  }
  if ((rc = svils_findk_set_graph(h_, links.data(), ed.size(), held.data(), held_.data(), held_.size() / 3))) throw_svils("svils_findk_set_graph", rc);
  if ((rc = svils_findk_init_state(h_, labels_.data(), values_.data()))) throw_svils("svils_findk_init_state", rc);
}

int FindK::run() {
  int r;
  while ((r = step()) == 0) {}
  return r == 1 ? 1 : 0;
}

int FindK::step() {
  if (done_) return 2;
  if (iter_ > log10(n_)) {   // :246-249
    printf("+ Done\n");
    done_ = true;
    return 2;
  }
  // the count and the top 5 on the device, the padding draws here (:217-225), set_gamma + estimate_all_pi on the device
  uint32_t m = 0;
  int rc = svils_findk_count(h_, &m);
  if (rc) throw_svils("svils_findk_count", rc);
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<uint32_t> nodes(m), nd(m), lab(4 * (size_t)m), pads(4 * (size_t)m, 0);
  if ((rc = svils_findk_pad_requests(h_, nodes.data(), nd.data(), lab.data()))) throw_svils("svils_findk_pad_requests", rc);
  for (uint32_t x = 0; x < m; ++x) {
    const uint32_t *have = &lab[4 * (size_t)x];
    for (uint32_t j = nd[x]; j < S; ++j) {   // a draw already in the node's map is redrawn; earlier pads are not checked
      uint32_t k;
      do k = rng_.uniform_int(n_); while (std::find(have, have + nd[x], k) != have + nd[x]);
      pads[4 * (size_t)x + (j - nd[x])] = k;
    }
  }
  pad_s_ = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  npad_ = m;
  if ((rc = svils_findk_apply(h_, pads.data()))) throw_svils("svils_findk_apply", rc);
  double sums[3] = {0, 0, 0};
  masks_.resize(n_);
  if ((rc = svils_findk_report(h_, &training_ll_, sums, &unlikely_, masks_.data()))) throw_svils("svils_findk_report", rc);
  if ((rc = svils_findk_get_state(h_, labels_.data(), values_.data(), nullptr))) throw_svils("svils_findk_get_state", rc);
  printf("avg. link training likelihood = %.5f\n", training_ll_);
  iter_++;
  printf("iteration = %d took %d secs\n", iter_, duration());
  fflush(stdout);
  if (heldout_likelihood(sums)) {   // the stop exits before this iteration's groups are written (:545-567)
    done_ = true;
    return 1;
  }
  write_groups();
  return 0;
}

// heldout_likelihood, :511-567
bool FindK::heldout_likelihood(const double sums[3]) {
  uint32_t k = 0, kzeros = 0, kones = 0;
  for (size_t x = 0; x < held_.size() / 3; ++x) {
    k++;
    if (held_[3 * x + 2]) kones++; else kzeros++;
  }
  const double s = sums[0], szeros = sums[1], sones = sums[2];
  const double nshol = (zeros_prob_ * (szeros / kzeros)) + (ones_prob_ * (sones / kones));
  const double row[11] = {(double)iter_, (double)duration(), s / k, (double)k, szeros / kzeros, (double)kzeros, sones / kones,
                          (double)kones, zeros_prob_ * (szeros / kzeros), ones_prob_ * (sones / kones), nshol};
  memcpy(row_, row, sizeof row_);
  if (hf_) {
    fprintf(hf_, "%d\t%d\t%.9f\t%d\t%.9f\t%d\t%.9f\t%d\t%.9f\t%.9f\t%.9f\n", iter_, duration(), s / k, k, szeros / kzeros, kzeros,
            sones / kones, kones, zeros_prob_ * (szeros / kzeros), ones_prob_ * (sones / kones), nshol);
    fflush(hf_);
  }
  const double a = nshol;
  bool stop = false;
  if (a > prev_h_ && prev_h_ != 0 && fabs((a - prev_h_) / prev_h_) < 0.00001) stop = true;
  else if (a < prev_h_) nh_++;
  else if (a > prev_h_) nh_ = 0;
  if (a > max_h_) max_h_ = a;
  if (nh_ > 10) stop = true;
  prev_h_ = a;
  return stop;
}

// the files of compute_and_log_groups (:350-413) from the membership masks: nodes visited in ascending external id, so
// every community's members come out sorted; communities in ascending label
void FindK::write_groups() {
  if (uf_) {
    fprintf(uf_, "%d\n", unlikely_);
    fflush(uf_);
  }
  if (!env_.write_files) return;
  const std::vector<uint32_t> &s2i = network_.seq2id();
  std::vector<uint32_t> start((size_t)n_ + 1, 0);
  auto each = [&](uint32_t i, auto fn) {   // the distinct labels of node i's set bits
    const uint32_t mk = masks_[i];
    for (uint32_t b = 0; b < S; ++b) {
      if (!(mk >> b & 1)) continue;
      const uint32_t L = labels_[(size_t)i * S + b];
      bool seen = false;
      for (uint32_t c = 0; c < b; ++c) seen |= (mk >> c & 1) && labels_[(size_t)i * S + c] == L;
      if (!seen) fn(L);
    }
  };
  for (uint32_t i = 0; i < n_; ++i) each(i, [&](uint32_t L) { start[L + 1]++; });
  for (uint32_t L = 0; L < n_; ++L) start[L + 1] += start[L];
  std::vector<uint32_t> ids(start[n_]), at(start.begin(), start.end() - 1);
  for (uint32_t i : ext_order_) each(i, [&](uint32_t L) { ids[at[L]++] = s2i[i]; });
  std::string comm, size;
  Cover found;
  char buf[64];
  for (uint32_t L = 0; L < n_; ++L) {
    if (start[L + 1] == start[L]) continue;
    for (uint32_t x = start[L]; x < start[L + 1]; ++x) {
      comm.append(buf, (size_t)snprintf(buf, sizeof buf, "%d ", (int)ids[x]));
    }
    comm.push_back('\n');
    size.append(buf, (size_t)snprintf(buf, sizeof buf, "%d\t%ld\n", (int)L, (long)(start[L + 1] - start[L])));
    if (env_.nmi) found.emplace_back(ids.begin() + start[L], ids.begin() + start[L + 1]);
  }
  FILE *f = open_or_die(Env::file_str("/communities.txt"), "communities");
  fwrite(comm.data(), 1, comm.size(), f);
  fclose(f);
  f = open_or_die(Env::file_str("/communities_size.txt"), "communities size");
  fwrite(size.data(), 1, size.size(), f);
  fclose(f);
  fclose(open_or_die(Env::file_str("/aggregate.txt"), "aggregate"));   // _mcount is never filled
  if (env_.nmi && !ground_truth_.empty()) {
    // the reference runs `/usr/local/bin/mutual ground_truth.txt communities.txt >> mutual.txt` here (:381-412)
    FILE *mf = fopen(Env::file_str("/mutual.txt").c_str(), "a");
    if (mf) {
      fprintf(mf, "mutual3:\t%g\n", lfk_nmi(ground_truth_, found));
      fclose(mf);
    }
  }
}

}  // namespace svinet
