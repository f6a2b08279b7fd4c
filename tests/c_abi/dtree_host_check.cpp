// The decision tree's host logic (csrc/dtree_host.h) on its own, for a sanitizer build
// (tests/test_dtree_reference.py builds this with -fsanitize=address,undefined and compares the
// output with the Python restatement).
//   dtree_host_check split FILE   FILE: "impurity max_bins min_instances n d", then n rows of d
//                                 features and a label (hex floats).  Prints each feature's
//                                 thresholds and the root's best split.
//   dtree_host_check nodes FILE   FILE: "n_nodes d", then n_nodes rows "feature left right".
//                                 Prints whether prediction would accept the array.
//   dtree_host_check grow FILE    FILE: "impurity max_depth min_instances n d B", then per feature
//                                 its threshold count and thresholds (hex floats), then n rows of
//                                 d bins and a label.  Grows the whole tree in level order -- each
//                                 node's histogram counted here, the split and the node's growth
//                                 the header's -- and prints every node, doubles as hex floats.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <utility>
#include <vector>

#include "dtree_host.h"

using namespace eegfx;

static double read_double(FILE* f) {
  char tok[128];
  if (fscanf(f, "%127s", tok) != 1) {
    fprintf(stderr, "short file\n");
    exit(2);
  }
  return strtod(tok, nullptr);
}

static int run_split(FILE* f) {
  const int kind = (int)read_double(f), max_bins = (int)read_double(f);
  const int min_instances = (int)read_double(f);
  const int n = (int)read_double(f), d = (int)read_double(f);
  std::vector<double> X((size_t)n * d), y((size_t)n);
  for (int r = 0; r < n; ++r) {
    for (int c = 0; c < d; ++c) X[(size_t)r * d + c] = read_double(f);
    y[r] = read_double(f);
  }
  const int B = std::min(max_bins, n), T = B - 1;
  std::vector<int32_t> nthr((size_t)d);
  std::vector<std::vector<double>> thr((size_t)d);
  std::vector<uint32_t> hist((size_t)d * B * 2, 0);
  for (int c = 0; c < d; ++c) {
    std::vector<double> col((size_t)n);
    for (int r = 0; r < n; ++r) col[r] = X[(size_t)r * d + c];
    dtree::find_thresholds(col, T, &thr[c]);
    nthr[c] = (int32_t)thr[c].size();
    printf("thr %d:", c);
    for (double t : thr[c]) printf(" %a", t);
    printf("\n");
    for (int r = 0; r < n; ++r) {
      int bin = 0;
      for (double t : thr[c]) bin += t < X[(size_t)r * d + c];
      ++hist[((size_t)c * B + bin) * 2 + (y[r] == 1.0 ? 1 : 0)];
    }
  }
  const dtree::Best b = dtree::best_split(hist.data(), d, B, nullptr, nthr.data(), kind, min_instances);
  printf("root %d %d %a %a\n", b.feature, b.split, b.gain,
         dtree::impurity(kind, b.tot[0], b.tot[1]));
  return 0;
}

static int run_nodes(FILE* f) {
  const int n_nodes = (int)read_double(f), d = (int)read_double(f);
  std::vector<eegfx_tree_node> nodes((size_t)(n_nodes > 0 ? n_nodes : 0));
  for (auto& nd : nodes) {
    memset(&nd, 0, sizeof nd);
    nd.feature = (int32_t)read_double(f);
    nd.left = (int32_t)read_double(f);
    nd.right = (int32_t)read_double(f);
  }
  printf("valid %d\n", dtree::nodes_valid(nodes.data(), n_nodes, d) ? 1 : 0);
  return 0;
}

static int run_grow(FILE* f) {
  const int kind = (int)read_double(f), max_depth = (int)read_double(f);
  const int min_instances = (int)read_double(f);
  const int n = (int)read_double(f), d = (int)read_double(f), B = (int)read_double(f);
  const int T = B - 1;
  std::vector<int32_t> nthr((size_t)d);
  std::vector<double> thr((size_t)d * T, 0.0);
  for (int c = 0; c < d; ++c) {
    nthr[c] = (int32_t)read_double(f);
    if (nthr[c] < 0 || nthr[c] > T) return 2;
    for (int s = 0; s < nthr[c]; ++s) thr[(size_t)c * T + s] = read_double(f);
  }
  std::vector<int> bins((size_t)n * d), label((size_t)n);
  for (int r = 0; r < n; ++r) {
    for (int c = 0; c < d; ++c) {
      bins[(size_t)r * d + c] = (int)read_double(f);
      if (bins[(size_t)r * d + c] < 0 || bins[(size_t)r * d + c] >= B) return 2;
    }
    label[r] = read_double(f) == 1.0 ? 1 : 0;
  }
  struct Active {
    int32_t pos;
    int level;
    std::vector<int> rows;
  };
  std::vector<eegfx_tree_node> tree{eegfx_tree_node{1, -1, -1, -1, 0.0, 0.0, 0.0, 0.0}};
  std::deque<Active> queue;
  queue.push_back(Active{0, 0, {}});
  for (int r = 0; r < n; ++r) queue.front().rows.push_back(r);
  std::vector<uint32_t> hist((size_t)d * B * 2);
  while (!queue.empty()) {
    const Active a = std::move(queue.front());
    queue.pop_front();
    std::fill(hist.begin(), hist.end(), 0u);
    for (int r : a.rows)
      for (int c = 0; c < d; ++c) ++hist[((size_t)c * B + bins[(size_t)r * d + c]) * 2 + label[r]];
    const dtree::Best b =
        dtree::best_split(hist.data(), d, B, nullptr, nthr.data(), kind, min_instances);
    const dtree::Grown g =
        dtree::grow_node(&tree, a.pos, a.level, max_depth, b, thr.data(), T, kind);
    if (g.feature < 0) continue;
    Active child[2] = {Active{g.child[0], a.level + 1, {}}, Active{g.child[1], a.level + 1, {}}};
    for (int r : a.rows)
      child[bins[(size_t)r * d + g.feature] <= g.split ? 0 : 1].rows.push_back(r);
    for (Active& c : child)
      if (c.pos >= 0) queue.push_back(std::move(c));
  }
  for (const eegfx_tree_node& nd : tree)
    printf("%d %d %d %d %a %a %a %a\n", nd.id, nd.feature, nd.left, nd.right, nd.threshold,
           nd.predict, nd.impurity, nd.gain);
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[2], "r");
  if (!f) return 2;
  const int rc = strcmp(argv[1], "split") == 0 ? run_split(f)
                 : strcmp(argv[1], "nodes") == 0 ? run_nodes(f)
                 : strcmp(argv[1], "grow") == 0  ? run_grow(f) : 2;
  fclose(f);
  return rc;
}
