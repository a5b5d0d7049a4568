// tests/host_text_main.cpp -- a stand-alone program over the host text entry points of include/dafs_hip.h (and the two of
// host_tree.cpp), for a sanitizer build on the CPU: test_text_cpu.py compiles it with dafs_amd/csrc/host_text.cpp and
// host_tree.cpp under -fsanitize=address,undefined and requires exit status 0 and an empty stderr.  Every entry point is
// called on a few inputs, the refusals and the empty inputs included, and everything returned is freed.  What the calls
// return is checked only as far as a wrong answer would point at a memory error; the formats are test_text_cpu.py's matter.
#include <cmath>
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

static void names_and_blocks() {
  char* text = nullptr;
  const char* headers[] = {"a desc", "", "a", "  b\tx", " "};
  EXPECT(dafs_host_stockholm_names(5, headers, &text) == DAFS_HIP_OK);
  EXPECT(take(text) == "a\nseq2\na.2\nb\nseq5");
  EXPECT(dafs_host_stockholm_names(0, nullptr, &text) == DAFS_HIP_OK);
  EXPECT(take(text) == "");
  EXPECT(dafs_host_stockholm_names(2, nullptr, &text) == DAFS_HIP_EINVAL && !text);
  EXPECT(dafs_host_stockholm_names(1, headers, nullptr) == DAFS_HIP_EINVAL);
  EXPECT(dafs_host_pp_char(0.95) == '*' && dafs_host_pp_char(0.949999) == '9' && dafs_host_pp_char(0.0) == '0');

  const char* names[] = {"s1", "a_rather_long_name_of_a_sequence"};
  const char* rows[] = {"AC-G-", "A-UG-"};
  const double r0[] = {0.97, 0.5, 0.04}, r1[] = {0.96, 0.15, 0.25};
  const double* rel[] = {r0, r1};
  const double col[] = {0.965, 0.5, 0.15, 0.145, 0.0};
  const uint8_t rf[] = {1, 0, 1, 1, 0};
  EXPECT(dafs_host_stockholm_block("[ 0.5 s1 s2 ]", 2, 5, names, rows, rel, col, "(..).", rf, "2..2.", &text) == DAFS_HIP_OK);
  EXPECT(take(text).size() > 100);
  EXPECT(dafs_host_stockholm_block(nullptr, 1, 5, names, rows, rel, col, "(..).", nullptr, nullptr, &text) == DAFS_HIP_OK);
  EXPECT(take(text).find("#=GC PP_cons *5.1.\n//\n") != std::string::npos);
  // no rows, no columns
  EXPECT(dafs_host_stockholm_block(nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, "", nullptr, nullptr, &text) == DAFS_HIP_OK);
  EXPECT(take(text) == "# STOCKHOLM 1.0\n#=GC SS_cons \n#=GC PP_cons \n//\n");
  // an all-gap row needs no reliabilities
  const char* gap_rows[] = {"-----"};
  const double* no_rel[] = {nullptr};
  EXPECT(dafs_host_stockholm_block(nullptr, 1, 5, names, gap_rows, no_rel, col, ".....", nullptr, nullptr, &text) == DAFS_HIP_OK);
  dafs_host_free(text);
  // refused: a row of another width, a row with residues and no reliabilities, no bracket string
  EXPECT(dafs_host_stockholm_block(nullptr, 2, 4, names, rows, rel, col, "(..)", nullptr, nullptr, &text) == DAFS_HIP_EINVAL && !text);
  EXPECT(strstr(dafs_hip_last_error(), "columns") != nullptr);
  EXPECT(dafs_host_stockholm_block(nullptr, 1, 5, names, rows, no_rel, col, ".....", nullptr, nullptr, &text) == DAFS_HIP_EINVAL);
  EXPECT(dafs_host_stockholm_block(nullptr, 2, 5, names, rows, rel, col, nullptr, nullptr, nullptr, &text) == DAFS_HIP_EINVAL);
}

static void covariation() {
  const uint32_t X = DAFS_HIP_NONE;
  const uint32_t L = 8, n = 4;
  const char* rows[] = {"AGCAAUCU", "GGCA-UCC", "cacaaugg", "TGAA-TTA"};
  std::vector<uint8_t> code;
  for (const char* row : rows)
    for (uint32_t c = 0; c < L; ++c) code.push_back(dafs_host_cov_code(row[c]));
  EXPECT(code[0] == 0 && code[L + 4] == 4 && code[3 * L] == 3);
  const uint32_t ss[] = {7, 5, X, X, X, X, X, X}, best[] = {7, 6, 6, X, 1, 1, 2, 0};
  const double bs[] = {12.5, 3.25, 3.25, 0.0, -0.125, 1e-5, 3.25, 12.5}, be[] = {0.0, 0.04, 0.04, 0.0, 7.5, 0.05, 0.04, 0.0};
  const double ps[] = {12.5, 1 / 3.0, 0, 0, 0, 0, 0, 0}, pe[] = {0.0, -std::nan(""), 0, 0, 0, 0, 0, 0};
  const uint32_t pr[] = {4, 4, 0, 0, 0, 0, 0, 0}, pc[] = {3, 4, 0, 0, 0, 0, 0, 0}, pt[] = {3, 2, 0, 0, 0, 0, 0, 0};
  char* text = nullptr;
  EXPECT(dafs_host_covariation_table(n, L, code.data(), ss, best, bs, be, ps, pe, pr, pc, pt, &text) == DAFS_HIP_OK);
  EXPECT(take(text) == "1\t8\tss\t12.5\t0\t4\t3\t3\n2\t6\tss\t0.333333333\tnan\t4\t4\t2\n2\t7\tother\t3.25\t0.04\t4\t3\t2\n3\t7\tother\t3.25\t0.04\t4\t2\t2\n");
  EXPECT(dafs_host_cov_ss_cons(L, ss, pe, 0.05, &text) == DAFS_HIP_OK);
  EXPECT(take(text) == "2......2");
  // no columns; no rows
  EXPECT(dafs_host_covariation_table(0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &text) == DAFS_HIP_OK);
  EXPECT(take(text) == "");
  EXPECT(dafs_host_covariation_table(0, L, nullptr, ss, best, bs, be, ps, pe, pr, pc, pt, &text) == DAFS_HIP_OK);
  EXPECT(take(text).find("other\t3.25\t0.04\t0\t0\t0\n") != std::string::npos);
  EXPECT(dafs_host_cov_ss_cons(0, nullptr, nullptr, 0.05, &text) == DAFS_HIP_OK);
  EXPECT(take(text) == "");
  // refused: a partner column outside the alignment, a missing array
  const uint32_t far_ss[] = {8, X, X, X, X, X, X, X}, far_best[] = {7, 6, 6, X, 1, 1, 2, 9};
  EXPECT(dafs_host_covariation_table(n, L, code.data(), far_ss, best, bs, be, ps, pe, pr, pc, pt, &text) == DAFS_HIP_EINVAL && !text);
  EXPECT(dafs_host_covariation_table(n, L, code.data(), ss, far_best, bs, be, ps, pe, pr, pc, pt, &text) == DAFS_HIP_EINVAL);
  EXPECT(dafs_host_covariation_table(n, L, nullptr, ss, best, bs, be, ps, pe, pr, pc, pt, &text) == DAFS_HIP_EINVAL);
  EXPECT(dafs_host_cov_ss_cons(L, far_ss, pe, 0.05, &text) == DAFS_HIP_EINVAL && !text);
  EXPECT(dafs_host_cov_ss_cons(L, ss, nullptr, 0.05, &text) == DAFS_HIP_EINVAL);
}

static void pairwise_table() {
  const char* names[] = {"tRNA-1 desc", "b", "c_3"};
  const uint32_t x[] = {0, 0, 1}, y[] = {1, 2, 2};
  const double sim[] = {0.123456791, 1.00000001e-07, 0.0}, score[] = {-12.5, INFINITY, std::nan("")};
  const int64_t its[] = {37, 600, -1};
  char* text = nullptr;
  EXPECT(dafs_host_pairwise_table(3, x, y, 3, names, sim, score, its, &text) == DAFS_HIP_OK);
  EXPECT(take(text) == "1\t2\ttRNA-1 desc\tb\t0.123456791\t-12.5\t37\n1\t3\ttRNA-1 desc\tc_3\t1.00000001e-07\tinf\t600\n2\t3\tb\tc_3\t0\tnan\t-1\n");
  EXPECT(dafs_host_pairwise_table(0, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, &text) == DAFS_HIP_OK);
  EXPECT(take(text) == "");
  EXPECT(dafs_host_pairwise_table(3, x, y, 2, names, sim, score, its, &text) == DAFS_HIP_EINVAL && !text);  // y = 2 of two names
  EXPECT(dafs_host_pairwise_table(3, x, nullptr, 3, names, sim, score, its, &text) == DAFS_HIP_EINVAL);
}

static int parse_clean(const std::string& file, std::string& names, std::string& rows) {
  uint32_t n = 99;
  char *nm = nullptr, *rw = nullptr;
  int rc = dafs_host_seed_parse(file.data(), file.size(), &n, &nm, &rw);
  if (rc != DAFS_HIP_OK) {
    EXPECT(!nm && !rw);
    return rc;
  }
  names = take(nm);
  std::string raw = take(rw);
  std::vector<std::string> nv, rv;
  for (std::string* joined : {&names, &raw}) {
    std::vector<std::string>& v = joined == &names ? nv : rv;
    size_t b = 0;
    for (uint32_t k = 0; k < n; ++k) {
      const size_t e = joined->find('\n', b);
      v.push_back(joined->substr(b, e == std::string::npos ? e : e - b));
      b = e == std::string::npos ? joined->size() : e + 1;
    }
  }
  std::vector<const char*> np, rp;
  for (uint32_t k = 0; k < n; ++k) { np.push_back(nv[k].c_str()); rp.push_back(rv[k].c_str()); }
  rc = dafs_host_seed_clean(n, np.data(), rp.data(), &rw);
  if (rc == DAFS_HIP_OK) rows = take(rw);
  else EXPECT(!rw);
  return rc;
}

static void seeds() {
  std::string names, rows;
  EXPECT(parse_clean("# STOCKHOLM 1.0\r\n#=GF ID x\r\n\r\na  AC-GU.\r\nb  A--GUA\r\n#=GC SS_cons <<..>>\r\n\r\na ..CC\r\nb -GC.\r\n//\r\n# STOCKHOLM 1.0\r\nc AAAA\r\n//\r\n",
                     names, rows) == DAFS_HIP_OK);
  EXPECT(names == "a\nb" && rows == "ACGU--CC\nA-GUAGC-");
  EXPECT(parse_clean("[ 0.5 x y ]\n>SS_cons\n((..))--\n> x desc\nAC--\nGU-A\n>y\n-C-A\n\nGUA-", names, rows) == DAFS_HIP_OK);
  EXPECT(names == "x desc\ny" && rows == "AC-GU-A\n-CAGUA-");
  EXPECT(parse_clean(">   \nAC\n", names, rows) == DAFS_HIP_OK);  // a header of blanks only: an empty name
  EXPECT(names == "" && rows == "AC");
  const char* refused[][2] = {{"# STOCKHOLM 1.0\na ACGU\nb ACG\n//\n", "seed: rows of unequal length (a: 4 columns, b: 3)"},
                              {">a\nAC-U\n>b\nA*GU\n", "seed: row b holds '*', which is neither a letter nor a gap"},
                              {">a\nAC-U\n>b\n-..-\n", "seed: row b has no residues"},
                              {"", "seed: no rows"},
                              {"# STOCKHOLM 1.0\n//\n", "seed: no rows"},
                              {"just text\n", "seed: no rows"},
                              {"# STOCKHOLM 1.0\na AC GU\n//\n", "seed: line 2 is neither a #= annotation nor 'name row'"},
                              {">a\nAC\n>b\n", "seed: rows of unequal length (a: 2 columns, b: 0)"}};
  for (const auto& r : refused) {
    EXPECT(parse_clean(r[0], names, rows) == DAFS_HIP_EINVAL);
    EXPECT(std::string(dafs_hip_last_error()) == r[1]);
  }
  EXPECT(parse_clean(std::string(">a\nA\0C\n", 7), names, rows) == DAFS_HIP_EINVAL);  // a NUL byte would cut the row short
  uint32_t n = 0;
  char *nm = nullptr, *rw = nullptr;
  EXPECT(dafs_host_seed_parse(nullptr, 0, &n, &nm, &rw) == DAFS_HIP_OK && n == 0);  // no bytes at all
  EXPECT(take(nm) == "" && take(rw) == "");
  EXPECT(dafs_host_seed_parse(nullptr, 3, &n, &nm, &rw) == DAFS_HIP_EINVAL && !nm && !rw);
  EXPECT(dafs_host_seed_parse("x", 1, nullptr, &nm, &rw) == DAFS_HIP_EINVAL);
  EXPECT(dafs_host_seed_parse("x", 1, &n, &nm, nullptr) == DAFS_HIP_EINVAL && !nm);
  EXPECT(dafs_host_seed_clean(0, nullptr, nullptr, &rw) == DAFS_HIP_EINVAL && !rw);  // "seed: no rows"
  EXPECT(dafs_host_seed_clean(2, nullptr, nullptr, &rw) == DAFS_HIP_EINVAL);
  const char* one[] = {"a"};
  const char* empty[] = {""};
  EXPECT(dafs_host_seed_clean(1, one, empty, &rw) == DAFS_HIP_EINVAL);
  EXPECT(std::string(dafs_hip_last_error()) == "seed: row a has no residues");
}

static void estimates_and_packing() {
  const uint32_t lens[] = {100, 120, 77};
  EXPECT(dafs_host_family_bytes(0, nullptr) == 0);
  EXPECT(dafs_host_family_bytes(1, lens) == 4 + 8 * 100 * 100 + 64 * 100 + 4096);
  EXPECT(dafs_host_family_bytes(3, lens) > dafs_host_family_bytes(2, lens));
  EXPECT(dafs_host_node_bytes(0, 0) > 0 && dafs_host_node_bytes(5000, 5000) > dafs_host_node_bytes(5000, 2047));
  EXPECT(dafs_host_batch_bytes() == 16ull << 30);
  const uint64_t sizes[] = {2, 50, 2, 2, UINT64_MAX, UINT64_MAX, 1};
  uint32_t group[7] = {9, 9, 9, 9, 9, 9, 9};
  EXPECT(dafs_host_pack_greedy(7, sizes, 5, group) == DAFS_HIP_OK);
  const uint32_t want[] = {0, 1, 2, 2, 3, 4, 5};
  EXPECT(memcmp(group, want, sizeof want) == 0);
  EXPECT(dafs_host_pack_greedy(7, sizes, UINT64_MAX, group) == DAFS_HIP_OK && group[3] == 0 && group[4] == 1 && group[6] == 3);
  EXPECT(dafs_host_pack_greedy(0, nullptr, 5, nullptr) == DAFS_HIP_OK);
  EXPECT(dafs_host_pack_greedy(2, sizes, 5, nullptr) == DAFS_HIP_EINVAL);
}

static void tree_and_merge() {
  const float sim[] = {1.0f, 0.5f, 0.25f, 0.5f, 1.0f, 0.75f, 0.25f, 0.75f, 1.0f};
  float score[5];
  int32_t left[5], right[5];
  EXPECT(dafs_host_build_tree(3, sim, score, left, right) == DAFS_HIP_OK);
  EXPECT(left[3] == 1 && right[3] == 2 && left[0] == -1);
  EXPECT(dafs_host_build_tree(1, sim, score, left, right) == DAFS_HIP_OK);
  EXPECT(dafs_host_build_tree(0, sim, score, left, right) == DAFS_HIP_EINVAL);
  const uint32_t X = DAFS_HIP_NONE;
  const uint32_t lens[] = {3, 2}, z[] = {X, 0, X, 1, X}, bad_z[] = {1, 0, X, 1, X};
  uint32_t seed_col[2], res_col[5], width = 0;
  EXPECT(dafs_host_merge_added(2, 2, lens, z, seed_col, res_col, &width) == DAFS_HIP_OK && width == 5);
  EXPECT(dafs_host_merge_added(2, 2, lens, bad_z, seed_col, res_col, &width) == DAFS_HIP_EINVAL);
  EXPECT(dafs_host_merge_added(0, 0, nullptr, nullptr, nullptr, nullptr, &width) == DAFS_HIP_OK && width == 0);
}

int main() {
  names_and_blocks();
  covariation();
  pairwise_table();
  seeds();
  estimates_and_packing();
  tree_and_merge();
  dafs_host_free(nullptr);
  if (failures) printf("%d expectations failed\n", failures);
  return failures ? 1 : 0;
}
