// tests/host_transfer_main.cpp -- a stand-alone program over the host text helpers of the transfer bootstrap (DESIGN.md section
// 28): dafs_host_split_depth, dafs_host_transfer_percent, dafs_host_newick_transfer, dafs_host_transfer_table and
// dafs_host_transfer_refusal, for a sanitizer build on the CPU.  test_transfer_cpu.py compiles it with
// dafs_amd/csrc/host_text.cpp and host_tree.cpp under -fsanitize=address,undefined and requires exit status 0 and an empty
// stderr.  The small trees, a deep chain, the refusals and the empty inputs are called, and everything returned is freed.
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

static void depths_and_percent() {
  int32_t depth[9];
  EXPECT(dafs_host_split_depth(5, kLeft, kRight, depth) == DAFS_HIP_OK);
  const int32_t want[9] = {-1, -1, -1, -1, -1, 2, 2, -1, -1};
  EXPECT(!memcmp(depth, want, sizeof want));
  EXPECT(dafs_host_split_depth(5, kLeft2, kRight2, depth) == DAFS_HIP_OK);
  const int32_t want2[9] = {-1, -1, -1, -1, -1, 2, 2, 2, -1};
  EXPECT(!memcmp(depth, want2, sizeof want2));
  const int32_t leaf = -1;
  EXPECT(dafs_host_split_depth(1, &leaf, &leaf, depth) == DAFS_HIP_OK && depth[0] == -1);
  int32_t bad[9];
  memcpy(bad, kLeft, sizeof bad);
  bad[7] = 8;
  EXPECT(dafs_host_split_depth(5, bad, kRight, depth) == DAFS_HIP_EINVAL);
  EXPECT(dafs_host_split_depth(0, kLeft, kRight, depth) == DAFS_HIP_EINVAL);
  EXPECT(dafs_host_split_depth(5, nullptr, kRight, depth) == DAFS_HIP_EINVAL);
  EXPECT(dafs_host_split_depth(5, kLeft, kRight, nullptr) == DAFS_HIP_EINVAL);
  EXPECT(dafs_host_transfer_percent(0, 2, 1) == 100 && dafs_host_transfer_percent(1, 2, 1) == 0 && dafs_host_transfer_percent(1, 3, 1) == 50);
  EXPECT(dafs_host_transfer_percent(199, 2, 200) == 1 && dafs_host_transfer_percent(7, 5, 2) == 13);
  EXPECT(dafs_host_transfer_percent(65536ll * 8191, 8192, 65536) == 0 && dafs_host_transfer_percent(0, 8192, 65536) == 100);
  EXPECT(dafs_host_transfer_percent(0, 1, 5) == -1 && dafs_host_transfer_percent(0, 2, 0) == -1 && dafs_host_transfer_percent(3, 2, 2) == -1);
  EXPECT(dafs_host_transfer_percent(-1, 2, 2) == -1 && dafs_host_transfer_percent(0, 0x80000000u, 1) == -1);
  EXPECT(dafs_host_transfer_percent(INT64_MAX, 0x7FFFFFFFu, 0xFFFFFFFFu) == -1);  // above B (depth - 1), which still fits 64 bits
}

static void a_deep_chain() {
  const uint32_t n = 30000, T = 2 * n - 1;
  std::vector<int32_t> left(T, -1), right(T, -1), depth(T, 0);
  std::vector<int64_t> transfer(T, -1);
  std::vector<std::string> names(n);
  std::vector<const char*> c_names(n);
  for (uint32_t k = 0; k < n; ++k) { names[k] = "s" + std::to_string(k); c_names[k] = names[k].c_str(); }
  left[n] = 0;
  right[n] = 1;
  for (uint32_t t = 1; t + 1 < n; ++t) { left[n + t] = (int32_t)(n + t - 1); right[n + t] = (int32_t)(t + 1); }
  EXPECT(dafs_host_split_depth(n, left.data(), right.data(), depth.data()) == DAFS_HIP_OK);
  EXPECT(depth[n] == 2 && depth[n + n / 2 - 2] == (int32_t)(n / 2) && depth[T - 3] == 2 && depth[T - 2] == -1 && depth[T - 1] == -1 && depth[0] == -1);
  for (uint32_t v = n; v + 2 < T; ++v) transfer[v] = depth[v] - 1;  // B = 2: half of the most
  char* text = nullptr;
  EXPECT(dafs_host_newick_transfer(n, c_names.data(), left.data(), right.data(), nullptr, transfer.data(), 2, &text) == DAFS_HIP_OK);
  const std::string line = take(text);
  EXPECT(line.size() > n && line.compare(line.size() - 3, 3, ");\n") == 0 && line.find("s0,s1)50,s2)50,") != std::string::npos);
}

static void texts() {
  char* text = nullptr;
  const double length[9] = {0.1, 0.2, 0.3, 0.4, 0.5, 0.05, 0.06, 0.07, 0.0};
  const int32_t support[9] = {-1, -1, -1, -1, -1, 7, 9, -1, -1};
  const int64_t transfer[9] = {-1, -1, -1, -1, -1, 3, 1, -1, -1}, none[9] = {-1, -1, -1, -1, -1, -1, -1, -1, -1};
  EXPECT(dafs_host_newick_transfer(5, kNames, kLeft, kRight, length, transfer, 10, &text) == DAFS_HIP_OK);
  EXPECT(take(text) == "(((A:0.1,B:0.2)70:0.05,(C:0.3,D:0.4)90:0.06):0.07,E:0.5);\n");
  EXPECT(dafs_host_newick_transfer(5, kNames, kLeft, kRight, nullptr, none, 10, &text) == DAFS_HIP_OK);
  EXPECT(take(text) == "(((A,B),(C,D)),E);\n");
  const int64_t root_split[9] = {-1, -1, -1, -1, -1, 1, 5, 1, -1};
  EXPECT(dafs_host_newick_transfer(5, kNames, kLeft2, kRight2, nullptr, root_split, 10, &text) == DAFS_HIP_OK);
  EXPECT(take(text) == "((A,B)90,((C,D)50,E));\n");
  const int64_t one = -1;
  const int32_t leaf = -1;
  EXPECT(dafs_host_newick_transfer(1, kNames, &leaf, &leaf, nullptr, &one, 1, &text) == DAFS_HIP_OK);
  EXPECT(take(text) == "A;\n");
  EXPECT(dafs_host_newick_transfer(5, kNames, kLeft, kRight, nullptr, transfer, 0, &text) == DAFS_HIP_EINVAL && !text);
  EXPECT(dafs_host_newick_transfer(5, kNames, kLeft, kRight, nullptr, transfer, 2, &text) == DAFS_HIP_EINVAL && !text);  // 3 > 2 x 1
  const int64_t on_trivial[9] = {-1, -1, -1, -1, -1, 3, 1, 2, -1};
  EXPECT(dafs_host_newick_transfer(5, kNames, kLeft, kRight, nullptr, on_trivial, 10, &text) == DAFS_HIP_EINVAL && !text);
  EXPECT(dafs_host_newick_transfer(5, kNames, kLeft, kRight, nullptr, nullptr, 10, &text) == DAFS_HIP_EINVAL);
  EXPECT(dafs_host_newick_transfer(5, nullptr, kLeft, kRight, nullptr, transfer, 10, &text) == DAFS_HIP_EINVAL && !text);
  EXPECT(dafs_host_newick_transfer(5, kNames, kLeft, kRight, nullptr, transfer, 10, nullptr) == DAFS_HIP_EINVAL);
  EXPECT(dafs_host_newick_transfer(0, kNames, kLeft, kRight, nullptr, transfer, 10, &text) == DAFS_HIP_EINVAL && !text);

  EXPECT(dafs_host_transfer_table(5, kNames, kLeft, kRight, support, transfer, 10, 12345, DAFS_NJ_JC, &text) == DAFS_HIP_OK);
  EXPECT(take(text) == "# rows 5 replicates 10 seed 12345 model jc measure transfer\n6\t7\t10\t70\t3\tC,D,E\t2\t3\t70\n7\t9\t10\t90\t2\tC,D\t2\t1\t90\n");
  const int32_t support2[9] = {-1, -1, -1, -1, -1, 9, 5, 9, -1};
  EXPECT(dafs_host_transfer_table(5, kNames, kLeft2, kRight2, support2, root_split, 10, ~0ull, DAFS_NJ_P, &text) == DAFS_HIP_OK);
  EXPECT(take(text) ==
         "# rows 5 replicates 10 seed 18446744073709551615 model p measure transfer\n6\t9\t10\t90\t3\tC,D,E\t2\t1\t90\n7\t5\t10\t50\t2\tC,D\t2\t5\t50\n");
  const int32_t no_support[9] = {-1, -1, -1, -1, -1, -1, -1, -1, -1};
  EXPECT(dafs_host_transfer_table(5, kNames, kLeft, kRight, no_support, none, 10, 1, DAFS_NJ_JC, &text) == DAFS_HIP_OK);
  EXPECT(take(text) == "# rows 5 replicates 10 seed 1 model jc measure transfer\n");
  EXPECT(dafs_host_transfer_table(5, kNames, kLeft, kRight, support, transfer, 0, 1, DAFS_NJ_JC, &text) == DAFS_HIP_EINVAL && !text);
  EXPECT(dafs_host_transfer_table(5, kNames, kLeft, kRight, support, transfer, 2, 1, DAFS_NJ_JC, &text) == DAFS_HIP_EINVAL && !text);  // a count above B
  EXPECT(dafs_host_transfer_table(5, kNames, kLeft, kRight, support, transfer, 10, 1, 7, &text) == DAFS_HIP_EINVAL && !text);
  EXPECT(dafs_host_transfer_table(5, kNames, kLeft, kRight, support, nullptr, 10, 1, DAFS_NJ_JC, &text) == DAFS_HIP_EINVAL);
  EXPECT(dafs_host_transfer_table(5, kNames, kLeft, kRight, nullptr, transfer, 10, 1, DAFS_NJ_JC, &text) == DAFS_HIP_EINVAL && !text);
  EXPECT(dafs_host_transfer_table(5, kNames, kLeft, kRight, support, none, 10, 1, DAFS_NJ_JC, &text) == DAFS_HIP_EINVAL && !text);  // a count without a sum
  for (int which = -1; which < 3; ++which) EXPECT(dafs_host_transfer_refusal(which) != nullptr);
  EXPECT(strlen(dafs_host_transfer_refusal(DAFS_TRANSFER_NEEDS_REPLICATES)) > 0 && !strlen(dafs_host_transfer_refusal(1)));
}

int main() {
  depths_and_percent();
  a_deep_chain();
  texts();
  if (failures) printf("%d checks failed\n", failures);
  return failures ? 1 : 0;
}
