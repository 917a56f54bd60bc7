#include "pairfiles.hh"

#include <cstdlib>

#include "env.hh"
#include "fixedfmt.hh"
#include "util.hh"

namespace svinet {

void load_pairs_file(const Network &network, const char *flag, const std::string &fname, std::vector<int> *ext, std::vector<uint32_t> *seq) {
  FILE *f = fopen(fname.c_str(), "r");
  if (!f) {
    fprintf(stderr, "error: cannot read %s file %s\n", flag, fname.c_str());
    exit(2);
  }
  int a, b;
  while (fscanf(f, "%d %d", &a, &b) == 2) {
    uint32_t p, q;
    if (!network.id2seq((uint32_t)a, &p) || !network.id2seq((uint32_t)b, &q)) {
      fprintf(stderr, "error: %s: id %d or id %d not found in original network\n", flag, a, b);
      exit(2);
    }
    if (p == q) {
      fprintf(stderr, "error: %s: pair %d %d is one node\n", flag, a, b);
      exit(2);
    }
    ext->push_back(a);
    ext->push_back(b);
    seq->push_back(p);
    seq->push_back(q);
  }
  fclose(f);
}

void write_link_prob(const Network &network, const std::vector<int> &ext, const std::vector<uint32_t> &seq, const std::vector<double> &prob) {
  FILE *f = open_or_die(Env::file_str("/link-prob.txt"), "link-prob");
  for (size_t i = 0; i < prob.size(); ++i)
    fprintf(f, "%d\t%d\t%d\t%.9e\n", ext[2 * i], ext[2 * i + 1], network.y(seq[2 * i], seq[2 * i + 1]) ? 1 : 0, prob[i]);
  fclose(f);
}

void write_recommendations(const Network &network, uint32_t n, uint32_t k, const std::vector<uint32_t> &ids, const std::vector<double> &sc,
                           const std::vector<uint32_t> *seq_of) {
  const std::vector<uint32_t> &s2i = network.seq2id();
  FILE *f = open_or_die(Env::file_str("/recommendations.txt"), "recommendations");
  for (uint32_t i = 0; i < n; ++i) {
    fprintf(f, "%d", (int)s2i[i]);
    for (uint32_t j = 0; j < k; ++j) {
      const uint32_t q = ids[(size_t)i * k + j];
      if (q == 0xffffffffu) fprintf(f, "\t-1\t%.9e", sc[(size_t)i * k + j]);
      else fprintf(f, "\t%d\t%.9e", (int)s2i[seq_of ? (*seq_of)[q] : q], sc[(size_t)i * k + j]);
    }
    fprintf(f, "\n");
  }
  fclose(f);
}

void RankSum::add(uint32_t above, uint32_t tied, uint32_t ncand) {
  const double ahead_mid = (double)above + 0.5 * (double)tied;   // candidates ahead of the link, ties halved
  const uint64_t ahead = (uint64_t)above + tied;
  ++cnt;
  auc += 1.0 - ahead_mid / (double)ncand;
  mrr += 1.0 / (ahead_mid + 1.0);
  h1 += ahead < 1;
  h10 += ahead < 10;
  h100 += ahead < 100;
  chance += 10.0 / (double)ncand;
}

void RankSum::print(FILE *f) const {
  const double c = cnt ? (double)cnt : 1.0;
  fprintf(f, "%llu\t%.17g\t%.17g\t%.17g\t%.17g\t%.17g\t%.17g\n", (unsigned long long)cnt, auc / c, mrr / c, (double)h1 / c,
          (double)h10 / c, (double)h100 / c, chance / c);
}

std::vector<uint32_t> directed_pairs(const std::vector<uint32_t> &seq, const std::function<uint32_t(uint32_t)> &map) {
  const size_t m = seq.size() / 2;
  std::vector<uint32_t> pairs(4 * m);
  for (size_t i = 0; i < m; ++i) {
    pairs[4 * i] = pairs[4 * i + 3] = map ? map(seq[2 * i]) : seq[2 * i];
    pairs[4 * i + 1] = pairs[4 * i + 2] = map ? map(seq[2 * i + 1]) : seq[2 * i + 1];
  }
  return pairs;
}

RankSum write_rank_file(const Network &network, const char *fname, const std::vector<uint32_t> &seq, const std::vector<int> *ext,
                        const std::vector<uint32_t> &above, const std::vector<uint32_t> &tied, const std::vector<uint32_t> &ncand,
                        const std::vector<double> &sc, const std::function<bool(uint32_t, uint32_t)> &held_out) {
  const std::vector<uint32_t> &s2i = network.seq2id();
  const size_t m = seq.size() / 2;
  RankSum sum;
  std::string o;
  {
    RowOut out(o);
    char num[64];
    for (size_t i = 0; i < m; ++i) {
      const uint32_t p = seq[2 * i], q = seq[2 * i + 1];
      const bool y = network.y(p, q);
      out.integer(ext ? (*ext)[2 * i] : (long)s2i[p], '\t');
      out.integer(ext ? (*ext)[2 * i + 1] : (long)s2i[q], '\t');
      out.integer(y ? 1 : 0, '\t');
      snprintf(num, sizeof num, "%.9e\t", sc[2 * i]);
      out.text(num);
      for (size_t d = 2 * i; d < 2 * i + 2; ++d) {
        out.fixed<3>((double)above[d] + 0.5 * (double)tied[d] + 1.0, '\t');
        out.integer((long)ncand[d], d == 2 * i ? '\t' : '\n');
        if (y && held_out(p, q) && ncand[d] != 0) sum.add(above[d], tied[d], ncand[d]);
      }
    }
  }
  if (fname) {
    FILE *f = open_or_die(Env::file_str(fname), fname + 1);
    fwrite(o.data(), 1, o.size(), f);
    fclose(f);
  }
  return sum;
}

void write_rank_summary(const RankSum &sum) {
  FILE *f = open_or_die(Env::file_str("/link-ranks-summary.txt"), "link-ranks-summary");
  fprintf(f, "pairs\tauc\tmrr\thits1\thits10\thits100\tchance10\n");
  sum.print(f);
  fclose(f);
}

}  // namespace svinet
