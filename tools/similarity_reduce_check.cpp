// tools/similarity_reduce_check.cpp — bnmf_similarity's finish (csrc/reduce_host.h: similarity_finish with con_canon64) as a stand-alone
// host program, so that it runs under the sanitizers without a device:
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread -Iinclude
//       -o similarity_reduce_check tools/similarity_reduce_check.cpp
//   similarity_reduce_check in.bin out.bin
// in.bin: int64 m, G, k, all; int32 members [m]; then, if all (the pass over all pairs ran), int32 nat [m][k] (places in the member list,
// -1 = none) and doubles nb [3][m][k], tum [3][m], all in member order.  out.bin, all doubles: neighbour_at [G][k], neighbour [3][G][k],
// tumour [3][G], then n_included, n_left_out, n_pairs, n_similar_pairs, n_isolated, mean_similarity, least_typical, least_typical_at; the
// same again with the three outputs NULL must give the same info (checked here).  tests/test_similarity_host.py builds it, runs it and
// holds out.bin to the numpy restatement bit for bit.
#include <cstdio>
#include "../bayesnmf_amd/csrc/reduce_host.h"

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::perror(argv[1]); return 2; }
  int64_t hd[4];
  if (std::fread(hd, 8, 4, f) != 4 || hd[0] < 2 || hd[1] < hd[0] || hd[2] < 0 || hd[2] > BNMF_SIM_MAX_K) { std::fprintf(stderr, "bad header\n"); return 2; }
  const long m = (long)hd[0], G = (long)hd[1]; const int k = (int)hd[2]; const bool all = hd[3] != 0;
  const size_t mk = (size_t)m * k, Gk = (size_t)G * k;
  std::vector<int> members(m);
  std::vector<int32_t> nat(all ? mk : 0);
  std::vector<double> nb(all ? 3 * mk : 0), tum(all ? 3 * (size_t)m : 0);
  auto get = [&](void* p, size_t size, size_t n) { return n == 0 || std::fread(p, size, n, f) == n; };   // (an empty vector has no address to read to)
  if (!get(members.data(), 4, members.size()) || !get(nat.data(), 4, nat.size()) || !get(nb.data(), 8, nb.size()) || !get(tum.data(), 8, tum.size())) {
    std::fprintf(stderr, "short input\n");
    return 2;
  }
  std::fclose(f);
  for (long i = 0; i < m; ++i) if (members[i] < 0 || members[i] >= G || (i && members[i] <= members[i - 1])) { std::fprintf(stderr, "bad member list\n"); return 2; }
  for (int32_t v : nat) if (v < -1 || v >= m) { std::fprintf(stderr, "bad neighbour\n"); return 2; }
  std::vector<int32_t> at(Gk);
  std::vector<double> ne(3 * Gk), tu(3 * (size_t)G);
  bnmf_similarity_info a, b;
  std::memset(&a, 0, sizeof a); std::memset(&b, 0, sizeof b);
  similarity_finish(members.data(), m, G, k, all ? nat.data() : nullptr, all ? nb.data() : nullptr, all ? tum.data() : nullptr, at.data(), ne.data(), tu.data(), &a);
  similarity_finish(members.data(), m, G, k, all ? nat.data() : nullptr, all ? nb.data() : nullptr, all ? tum.data() : nullptr, nullptr, nullptr, nullptr, &b);
  if (std::memcmp(&a, &b, sizeof a) != 0) { std::fprintf(stderr, "the info depends on the optional outputs\n"); return 1; }
  std::vector<double> out(at.begin(), at.end());
  out.insert(out.end(), ne.begin(), ne.end());
  out.insert(out.end(), tu.begin(), tu.end());
  for (double v : {(double)a.n_included, (double)a.n_left_out, (double)a.n_pairs, (double)a.n_similar_pairs, (double)a.n_isolated, a.mean_similarity,
                   a.least_typical, (double)a.least_typical_at}) out.push_back(v);
  FILE* o = std::fopen(argv[2], "wb");
  if (!o) { std::perror(argv[2]); return 2; }
  std::fwrite(out.data(), 8, out.size(), o);
  std::fclose(o);
  return 0;
}
