// The random forest's host logic (csrc/rforest_host.h) on its own, for a sanitizer build
// (tests/test_rforest_reference.py builds this with -fsanitize=address,undefined and compares the
// output with the Python restatement).
//   rforest_host_check bag N TREES P SEED THREADS   one line per tree: its weights, then its sum
//   rforest_host_check fpn SUBSET TREES D           features per node
//   rforest_host_check reservoir D K SEED           the k features, in reservoir order
//   rforest_host_check group D K NODE_BYTES TREES SEED
//                                 the roots of TREES trees leave the queue group by group: one
//                                 line per group, "tree:features,..." per node
//   rforest_host_check split FILE  FILE: "impurity max_bins min_instances n d k", the k features
//                                 of the node, then n rows of d features, a label (hex floats)
//                                 and a weight.  Prints the node's best split.
//   rforest_host_check forest FILE FILE: "num_trees d", num_trees + 1 offsets, "n_nodes", then
//                                 n_nodes rows "feature left right".  Prints whether prediction
//                                 would accept the forest.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rforest_host.h"

using namespace eegfx;

static double read_double(FILE* f) {
  char tok[128];
  if (fscanf(f, "%127s", tok) != 1) {
    fprintf(stderr, "short file\n");
    exit(2);
  }
  return strtod(tok, nullptr);
}

static int run_bag(char** a) {
  const int64_t n = atoll(a[0]);
  const int trees = atoi(a[1]), P = atoi(a[2]);
  const int64_t seed = atoll(a[3]);
  const int threads = atoi(a[4]);
  std::vector<uint8_t> w((size_t)trees * n);
  std::vector<int64_t> sums((size_t)trees);
  if (!rforest::poisson_bag(n, trees, P, seed, w.data(), sums.data(), threads)) return 3;
  for (int t = 0; t < trees; ++t) {
    for (int64_t r = 0; r < n; ++r) printf("%d ", (int)w[(size_t)t * n + r]);
    printf("= %lld\n", (long long)sums[t]);
  }
  return 0;
}

static int run_group(char** a) {
  const int d = atoi(a[0]), k = atoi(a[1]);
  const int64_t node_bytes = atoll(a[2]);
  const int trees = atoi(a[3]);
  spark::JavaRandom rng(atoll(a[4]));
  std::deque<rforest::QNode> q;
  for (int t = 0; t < trees; ++t) q.push_back(rforest::QNode{t, 0, 0, t});
  std::vector<rforest::QNode> group;
  std::vector<int32_t> subsets;
  while (!q.empty()) {
    rforest::next_group(&q, &rng, d, k, k < d, node_bytes, &group, &subsets);
    if (group.empty()) return 3;
    for (size_t i = 0; i < group.size(); ++i) {
      printf("%d:", group[i].tree);
      for (int j = 0; j < (k < d ? k : 0); ++j) printf("%s%d", j ? "," : "", subsets[i * k + j]);
      printf(" ");
    }
    printf("\n");
  }
  return 0;
}

static int run_split(FILE* f) {
  const int kind = (int)read_double(f), max_bins = (int)read_double(f);
  const int min_instances = (int)read_double(f);
  const int n = (int)read_double(f), d = (int)read_double(f), k = (int)read_double(f);
  std::vector<int32_t> feat((size_t)k);
  for (auto& v : feat) v = (int32_t)read_double(f);
  std::vector<double> X((size_t)n * d), y((size_t)n);
  std::vector<uint32_t> w((size_t)n);
  for (int r = 0; r < n; ++r) {
    for (int c = 0; c < d; ++c) X[(size_t)r * d + c] = read_double(f);
    y[r] = read_double(f);
    w[r] = (uint32_t)read_double(f);
  }
  const int B = std::min(max_bins, n), T = B - 1;
  std::vector<int32_t> nthr((size_t)d);
  std::vector<std::vector<double>> thr((size_t)d);
  for (int c = 0; c < d; ++c) {
    std::vector<double> col((size_t)n);
    for (int r = 0; r < n; ++r) col[r] = X[(size_t)r * d + c];
    dtree::find_thresholds(col, T, &thr[c]);
    nthr[c] = (int32_t)thr[c].size();
  }
  std::vector<uint32_t> hist((size_t)k * B * 2, 0);
  for (int j = 0; j < k; ++j)
    for (int r = 0; r < n; ++r) {
      int bin = 0;
      for (double t : thr[feat[j]]) bin += t < X[(size_t)r * d + feat[j]];
      hist[((size_t)j * B + bin) * 2 + (y[r] == 1.0 ? 1 : 0)] += w[r];
    }
  const dtree::Best b =
      dtree::best_split(hist.data(), k, B, feat.data(), nthr.data(), kind, min_instances);
  printf("node %d %d %a %a\n", b.feature, b.split, b.gain,
         dtree::impurity(kind, b.tot[0], b.tot[1]));
  // the identity list is the decision tree's own selection (no list: feature j)
  if (k == d) {
    bool identity = true;
    for (int j = 0; j < k; ++j) identity = identity && feat[j] == j;
    if (identity) {
      const dtree::Best t =
          dtree::best_split(hist.data(), d, B, nullptr, nthr.data(), kind, min_instances);
      printf("same %d\n", t.feature == b.feature && t.split == b.split && t.gain == b.gain);
    }
  }
  return 0;
}

static int run_forest(FILE* f) {
  const int trees = (int)read_double(f), d = (int)read_double(f);
  std::vector<int32_t> offsets((size_t)(trees > 0 ? trees : 0) + 1);
  for (auto& o : offsets) o = (int32_t)read_double(f);
  const int n_nodes = (int)read_double(f);
  std::vector<eegfx_tree_node> nodes((size_t)(n_nodes > 0 ? n_nodes : 0));
  for (auto& nd : nodes) {
    memset(&nd, 0, sizeof nd);
    nd.feature = (int32_t)read_double(f);
    nd.left = (int32_t)read_double(f);
    nd.right = (int32_t)read_double(f);
  }
  printf("valid %d\n", rforest::forest_valid(nodes.data(), offsets.data(), trees, d) ? 1 : 0);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const char* mode = argv[1];
  if (strcmp(mode, "bag") == 0 && argc == 7) return run_bag(argv + 2);
  if (strcmp(mode, "group") == 0 && argc == 7) return run_group(argv + 2);
  if (strcmp(mode, "fpn") == 0 && argc == 5) {
    printf("%d\n", rforest::features_per_node(atoi(argv[2]), atoi(argv[3]), atoi(argv[4])));
    return 0;
  }
  if (strcmp(mode, "reservoir") == 0 && argc == 5) {
    const int d = atoi(argv[2]), k = atoi(argv[3]);
    std::vector<int32_t> res((size_t)k);
    rforest::reservoir(d, k, atoll(argv[4]), res.data());
    for (int v : res) printf("%d ", v);
    printf("\n");
    return 0;
  }
  if (argc != 3) return 2;
  FILE* f = fopen(argv[2], "r");
  if (!f) return 2;
  const int rc = strcmp(mode, "split") == 0 ? run_split(f)
                 : strcmp(mode, "forest") == 0 ? run_forest(f) : 2;
  fclose(f);
  return rc;
}
