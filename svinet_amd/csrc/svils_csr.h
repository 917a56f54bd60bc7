// svils_csr.h -- a list of node pairs as a symmetric CSR with ascending rows and 64-bit row offsets: the graph form of the
// sparse svils_batch handle (-sparse-graph) and of svils_sbm (-single).  Host code only.
#pragma once
#include "svils_handle.h"

namespace svils_impl {

struct HostCsr {
  std::vector<uint64_t> row;   // [n + 1]
  std::vector<uint32_t> col;
  bool has(uint32_t p, uint32_t q) const { return std::binary_search(col.begin() + row[p], col.begin() + row[p + 1], q); }
  void clear() {
    std::vector<uint64_t>().swap(row);
    std::vector<uint32_t>().swap(col);
  }
};

// One list of a *_set_graph call (`name`) as a symmetric CSR with ascending rows.  The refusals are the dense form's, in
// its order -- the first entry that is no pair p < q < n or repeats an earlier one -- with the repeat found after a sort
// of the entries before the first that is no pair.  The sorted list fills the rows in order: row r takes its partners
// below r while their rows are walked and those above r in its own, so no row is sorted again
inline int build_csr(const char *name, uint32_t n, const uint32_t *list, uint64_t cnt, const char *what, HostCsr &out) {
  uint64_t bad = cnt;
  for (uint64_t x = 0; x < cnt && bad == cnt; ++x)
    if (list[2 * x] >= list[2 * x + 1] || list[2 * x + 1] >= n) bad = x;
  std::vector<std::pair<uint64_t, uint64_t>> key((size_t)bad);   // (p, q) in one word, then the entry
  for (uint64_t x = 0; x < bad; ++x) key[x] = {((uint64_t)list[2 * x] << 32) | list[2 * x + 1], x};
  std::sort(key.begin(), key.end());
  uint64_t rep = cnt;   // equal pairs stand together in entry order: the first repeat is the least second of two neighbours
  for (uint64_t i = 1; i < bad; ++i)
    if (key[i].first == key[i - 1].first) rep = std::min(rep, key[i].second);
  if (rep < cnt)
    return fail(SVILS_ERR_ARG, "%s: %s %llu (%u, %u) is repeated", name, what, (unsigned long long)rep, list[2 * rep], list[2 * rep + 1]);
  if (bad < cnt)
    return fail(SVILS_ERR_ARG, "%s: %s %llu (%u, %u) is not a pair p < q < n = %u", name, what, (unsigned long long)bad, list[2 * bad],
                list[2 * bad + 1], n);
  out.row.assign((size_t)n + 1, 0);
  out.col.assign(2 * (size_t)cnt, 0);
  for (uint64_t x = 0; x < cnt; ++x) {
    ++out.row[list[2 * x] + 1];
    ++out.row[list[2 * x + 1] + 1];
  }
  for (uint32_t i = 0; i < n; ++i) out.row[i + 1] += out.row[i];
  std::vector<uint64_t> at(out.row.begin(), out.row.end() - 1);
  for (const auto &kx : key) {
    const uint32_t p = (uint32_t)(kx.first >> 32), q = (uint32_t)kx.first;
    out.col[at[p]++] = q;
    out.col[at[q]++] = p;
  }
  return 0;
}

}  // namespace svils_impl
