// The decision tree's host logic (csrc/dtree_host.h) on its own, for a sanitizer build
// (tests/test_dtree_reference.py builds this with -fsanitize=address,undefined and compares the
// output with the Python restatement).
//   dtree_host_check split FILE   FILE: "impurity max_bins min_instances n d", then n rows of d
//                                 features and a label (hex floats).  Prints each feature's
//                                 thresholds and the root's best split.
//   dtree_host_check nodes FILE   FILE: "n_nodes d", then n_nodes rows "feature left right".
//                                 Prints whether prediction would accept the array.
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
  const dtree::Best b = dtree::best_split(hist.data(), d, B, nthr.data(), kind, min_instances);
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

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[2], "r");
  if (!f) return 2;
  const int rc = strcmp(argv[1], "split") == 0 ? run_split(f)
                 : strcmp(argv[1], "nodes") == 0 ? run_nodes(f) : 2;
  fclose(f);
  return rc;
}
