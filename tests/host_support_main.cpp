// tests/host_support_main.cpp -- a stand-alone program over the host entry points of the bootstrap support (DESIGN.md section
// 23): dafs_host_tree_support, dafs_host_newick_support and dafs_host_support_table, for a sanitizer build on the CPU.
// test_bootstrap_cpu.py compiles it with dafs_amd/csrc/host_text.cpp and host_tree.cpp under -fsanitize=address,undefined and
// requires exit status 0 and an empty stderr.  The small trees, a deep chain, the refusals and the empty inputs are called,
// and everything returned is freed.  The formats and the counts are test_bootstrap_cpu.py's matter.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../include/dafs_hip.h"

// the library's error text lives in capi.cpp, which needs HIP: this program brings its own
static std::string g_error;
namespace dafs {
void set_last_error(const char* msg) { g_error = msg; }
}
extern "C" const char* dafs_hip_last_error(void) { return g_error.c_str(); }

static int failures = 0;
#define EXPECT(cond)                                                   \
  do {                                                                 \
    if (!(cond)) {                                                     \
      printf("%s:%d: %s is false\n", __FILE__, __LINE__, #cond);       \
      ++failures;                                                      \
    }                                                                  \
  } while (0)

static std::string take(char* text) {
  std::string s(text ? text : "<null>");
  dafs_host_free(text);
  return s;
}

// (((A,B),(C,D)),E) and ((A,B),((C,D),E)): the same unrooted tree
static const int32_t kLeft[9] = {-1, -1, -1, -1, -1, 0, 2, 5, 7}, kRight[9] = {-1, -1, -1, -1, -1, 1, 3, 6, 4};
static const int32_t kLeft2[9] = {-1, -1, -1, -1, -1, 0, 2, 6, 5}, kRight2[9] = {-1, -1, -1, -1, -1, 1, 3, 4, 7};
static const char* kNames[5] = {"A", "B", "C", "D", "E"};

static void support_counts() {
  int32_t support[9];
  std::vector<int32_t> rl, rr;
  for (int k = 0; k < 3; ++k) {
    rl.insert(rl.end(), k == 1 ? kLeft2 : kLeft, (k == 1 ? kLeft2 : kLeft) + 9);
    rr.insert(rr.end(), k == 1 ? kRight2 : kRight, (k == 1 ? kRight2 : kRight) + 9);
  }
  EXPECT(dafs_host_tree_support(5, kLeft, kRight, 3, rl.data(), rr.data(), support) == DAFS_HIP_OK);
  const int32_t want[9] = {-1, -1, -1, -1, -1, 3, 3, -1, -1};
  EXPECT(!memcmp(support, want, sizeof want));
  EXPECT(dafs_host_tree_support(5, kLeft2, kRight2, 3, rl.data(), rr.data(), support) == DAFS_HIP_OK);
  const int32_t want2[9] = {-1, -1, -1, -1, -1, 3, 3, 3, -1};
  EXPECT(!memcmp(support, want2, sizeof want2));
  EXPECT(dafs_host_tree_support(5, kLeft, kRight, 0, nullptr, nullptr, support) == DAFS_HIP_OK && support[5] == 0 && support[7] == -1);
  // one, two and three leaves: nothing to support
  const int32_t l1[1] = {-1}, l2[3] = {-1, -1, 0}, r2[3] = {-1, -1, 1}, l3[5] = {-1, -1, -1, 1, 3}, r3[5] = {-1, -1, -1, 2, 0};
  const int32_t* small_left[3] = {l1, l2, l3};
  const int32_t* small_right[3] = {l1, r2, r3};
  for (uint32_t n = 1; n <= 3; ++n) {
    int32_t s[5] = {7, 7, 7, 7, 7};
    EXPECT(dafs_host_tree_support(n, small_left[n - 1], small_right[n - 1], 1, small_left[n - 1], small_right[n - 1], s) == DAFS_HIP_OK);
    for (uint32_t v = 0; v < 2 * n - 1; ++v) EXPECT(s[v] == -1);
  }
  // refusals
  int32_t bad[9];
  memcpy(bad, kLeft, sizeof bad);
  bad[7] = 8;
  EXPECT(dafs_host_tree_support(5, bad, kRight, 1, kLeft, kRight, support) == DAFS_HIP_EINVAL);
  EXPECT(dafs_host_tree_support(5, kLeft, kRight, 1, bad, kRight, support) == DAFS_HIP_EINVAL && g_error.find("replicate 0") != std::string::npos);
  EXPECT(dafs_host_tree_support(0, kLeft, kRight, 1, kLeft, kRight, support) == DAFS_HIP_EINVAL);
  EXPECT(dafs_host_tree_support(5, nullptr, kRight, 1, kLeft, kRight, support) == DAFS_HIP_EINVAL);
  EXPECT(dafs_host_tree_support(5, kLeft, kRight, 1, nullptr, kRight, support) == DAFS_HIP_EINVAL);
  EXPECT(dafs_host_tree_support(5, kLeft, kRight, 1, kLeft, kRight, nullptr) == DAFS_HIP_EINVAL);
}

static void a_deep_chain() {
  const uint32_t n = 30000, T = 2 * n - 1;
  std::vector<int32_t> left(T, -1), right(T, -1), support(T, 0);
  std::vector<std::string> names(n);
  std::vector<const char*> c_names(n);
  for (uint32_t k = 0; k < n; ++k) { names[k] = "s" + std::to_string(k); c_names[k] = names[k].c_str(); }
  left[n] = 0;
  right[n] = 1;
  for (uint32_t t = 1; t + 1 < n; ++t) { left[n + t] = (int32_t)(n + t - 1); right[n + t] = (int32_t)(t + 1); }
  EXPECT(dafs_host_tree_support(n, left.data(), right.data(), 1, right.data(), left.data(), support.data()) == DAFS_HIP_OK);
  EXPECT(support[n] == 1 && support[T - 3] == 1 && support[T - 2] == -1 && support[T - 1] == -1 && support[0] == -1);
  char* text = nullptr;
  EXPECT(dafs_host_newick_support(n, c_names.data(), left.data(), right.data(), nullptr, support.data(), 1, &text) == DAFS_HIP_OK);
  const std::string line = take(text);
  EXPECT(line.size() > n && line.compare(line.size() - 3, 3, ");\n") == 0);
}

static void texts() {
  char* text = nullptr;
  const double length[9] = {0.1, 0.2, 0.3, 0.4, 0.5, 0.05, 0.06, 0.07, 0.0};
  const int32_t support[9] = {-1, -1, -1, -1, -1, 87, 40, -1, -1}, none[9] = {-1, -1, -1, -1, -1, -1, -1, -1, -1};
  EXPECT(dafs_host_newick_support(5, kNames, kLeft, kRight, length, support, 100, &text) == DAFS_HIP_OK);
  EXPECT(take(text) == "(((A:0.1,B:0.2)87:0.05,(C:0.3,D:0.4)40:0.06):0.07,E:0.5);\n");
  EXPECT(dafs_host_newick_support(5, kNames, kLeft, kRight, nullptr, none, 100, &text) == DAFS_HIP_OK);
  EXPECT(take(text) == "(((A,B),(C,D)),E);\n");
  const int32_t root_split[9] = {-1, -1, -1, -1, -1, 9, 5, 9, -1};
  EXPECT(dafs_host_newick_support(5, kNames, kLeft2, kRight2, nullptr, root_split, 10, &text) == DAFS_HIP_OK);
  EXPECT(take(text) == "((A,B)90,((C,D)50,E));\n");
  const int32_t one = -1;
  const int32_t leaf = -1;
  EXPECT(dafs_host_newick_support(1, kNames, &leaf, &leaf, nullptr, &one, 1, &text) == DAFS_HIP_OK);
  EXPECT(take(text) == "A;\n");
  EXPECT(dafs_host_newick_support(5, kNames, kLeft, kRight, nullptr, support, 0, &text) == DAFS_HIP_EINVAL && !text);
  EXPECT(dafs_host_newick_support(5, kNames, kLeft, kRight, nullptr, support, 50, &text) == DAFS_HIP_EINVAL && !text);
  EXPECT(dafs_host_newick_support(5, kNames, kLeft, kRight, nullptr, nullptr, 50, &text) == DAFS_HIP_EINVAL);
  EXPECT(dafs_host_newick_support(5, nullptr, kLeft, kRight, nullptr, support, 100, &text) == DAFS_HIP_EINVAL && !text);
  EXPECT(dafs_host_newick_support(5, kNames, kLeft, kRight, nullptr, support, 100, nullptr) == DAFS_HIP_EINVAL);
  EXPECT(dafs_host_newick_support(0, kNames, kLeft, kRight, nullptr, support, 100, &text) == DAFS_HIP_EINVAL && !text);

  EXPECT(dafs_host_support_table(5, kNames, kLeft, kRight, support, 100, 12345, DAFS_NJ_JC, &text) == DAFS_HIP_OK);
  EXPECT(take(text) == "# rows 5 replicates 100 seed 12345 model jc\n6\t87\t100\t87\t3\tC,D,E\n7\t40\t100\t40\t2\tC,D\n");
  EXPECT(dafs_host_support_table(5, kNames, kLeft2, kRight2, root_split, 10, ~0ull, DAFS_NJ_P, &text) == DAFS_HIP_OK);
  EXPECT(take(text) == "# rows 5 replicates 10 seed 18446744073709551615 model p\n6\t9\t10\t90\t3\tC,D,E\n7\t5\t10\t50\t2\tC,D\n");
  EXPECT(dafs_host_support_table(5, kNames, kLeft, kRight, none, 100, 1, DAFS_NJ_JC, &text) == DAFS_HIP_OK);
  EXPECT(take(text) == "# rows 5 replicates 100 seed 1 model jc\n");
  EXPECT(dafs_host_support_table(5, kNames, kLeft, kRight, support, 0, 1, DAFS_NJ_JC, &text) == DAFS_HIP_EINVAL && !text);
  EXPECT(dafs_host_support_table(5, kNames, kLeft, kRight, support, 50, 1, DAFS_NJ_JC, &text) == DAFS_HIP_EINVAL && !text);
  EXPECT(dafs_host_support_table(5, kNames, kLeft, kRight, support, 100, 1, 7, &text) == DAFS_HIP_EINVAL && !text);
  EXPECT(dafs_host_support_table(5, kNames, kLeft, kRight, nullptr, 100, 1, DAFS_NJ_JC, &text) == DAFS_HIP_EINVAL && !text);
  int32_t bad[9];
  memcpy(bad, kRight, sizeof bad);
  bad[5] = 0;
  EXPECT(dafs_host_support_table(5, kNames, kLeft, bad, support, 100, 1, DAFS_NJ_JC, &text) == DAFS_HIP_EINVAL && !text);
  for (int which = -1; which < 6; ++which) EXPECT(dafs_host_bootstrap_refusal(which) != nullptr);
  EXPECT(strlen(dafs_host_bootstrap_refusal(DAFS_BOOTSTRAP_NO_COLUMN)) > 0 && !strlen(dafs_host_bootstrap_refusal(4)));
}

int main() {
  support_counts();
  a_deep_chain();
  texts();
  if (failures) printf("%d checks failed\n", failures);
  return failures ? 1 : 0;
}
