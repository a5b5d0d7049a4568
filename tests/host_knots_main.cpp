// tests/host_knots_main.cpp -- a stand-alone program over the host entry points of DESIGN.md section 26
// (dafs_host_seed_clean_structure_levels, dafs_host_row_constraint_levels), for a sanitizer build on the CPU:
// test_seed_knots_cpu.py compiles it with dafs_amd/csrc/host_text.cpp and host_tree.cpp under -fsanitize=address,undefined and
// requires exit status 0 and an empty stderr.  The output buffers are exactly as large as the header says they must be, so a
// write past them is seen.  The formats and rules are test_seed_knots_cpu.py's matter.
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

static void reader() {
  const char* names[] = {"a", "b"};
  {  // a knot over two rows, one all-gap column that takes the '<' of a pair with it
    const char* rows[] = {"GAG.ACAC", "GAG-ACA-"};
    const size_t width = strlen(rows[0]);
    std::vector<uint32_t> ss(width);
    std::vector<uint8_t> level(width);
    uint32_t columns = 0;
    char* text = nullptr;
    EXPECT(dafs_host_seed_clean_structure_levels(2, names, rows, "(.[<)..]", ss.data(), level.data(), &columns, &text) == DAFS_HIP_EINVAL && !text);
    EXPECT(dafs_host_seed_clean_structure_levels(2, names, rows, "(.[<).>]", ss.data(), level.data(), &columns, &text) == DAFS_HIP_OK);
    EXPECT(take(text) == "GAGACAC\nGAGACA-" && columns == 7);
    EXPECT(ss[0] == 3 && ss[2] == 6 && ss[1] == DAFS_HIP_NONE && ss[3] == DAFS_HIP_NONE);
    EXPECT(level[0] == 0 && level[3] == 0 && level[2] == 1 && level[6] == 1 && level[1] == 0xFF && level[5] == 0xFF);
  }
  {  // one row, every group once and nested: all of level 0
    const char* rows[] = {"ACGUACGUACGUACGUACGUACGU"};
    std::vector<uint32_t> ss(24);
    std::vector<uint8_t> level(24);
    uint32_t columns = 0;
    char* text = nullptr;
    EXPECT(dafs_host_seed_clean_structure_levels(1, names, rows, "([{<AZ.,:_-~....za>}])..", ss.data(), level.data(), &columns, &text) == DAFS_HIP_OK);
    take(text);
    EXPECT(columns == 24 && ss[0] == 21 && ss[4] == 17 && ss[5] == 16 && level[5] == 0 && level[16] == 0 && level[22] == 0xFF);
  }
  {  // the refusals: five levels, unbalanced letters, a foreign character, a wrong length, null arguments
    const char* rows[] = {"ACGUACGUACGUACGUACG"};
    std::vector<uint32_t> ss(19);
    std::vector<uint8_t> level(19);
    uint32_t columns = 0;
    char* text = nullptr;
    const char* bad[] = {"(.[.{.<.A.).].}.>.a", "a..................", "A..................", "(.!..).............", "(.)"};
    for (const char* line : bad) {
      EXPECT(dafs_host_seed_clean_structure_levels(1, names, rows, line, ss.data(), level.data(), &columns, &text) == DAFS_HIP_EINVAL && !text);
      EXPECT(!g_error.empty());
    }
    EXPECT(g_error.find("3 columns") != std::string::npos);
    EXPECT(dafs_host_seed_clean_structure_levels(1, names, rows, nullptr, ss.data(), level.data(), &columns, &text) == DAFS_HIP_EINVAL);
    EXPECT(dafs_host_seed_clean_structure_levels(1, names, rows, "...................", ss.data(), nullptr, &columns, &text) == DAFS_HIP_EINVAL);
    EXPECT(dafs_host_seed_clean_structure_levels(0, nullptr, nullptr, "", ss.data(), level.data(), &columns, &text) == DAFS_HIP_EINVAL);
  }
}

static void constraints() {
  const uint32_t N = DAFS_HIP_NONE;
  const uint8_t F = 0xFF;
  {
    const uint8_t mask[] = {1, 1, 1, 1, 1, 1, 1};
    const uint32_t ss[] = {4, N, 6, N, N, N, N};
    const uint8_t level[] = {0, F, 1, F, 0, F, 1};
    std::vector<char> out(2 * 8);  // two strings of 7 characters and a NUL each
    EXPECT(dafs_host_row_constraint_levels(7, mask, ss, level, 2, "GAGACAC", out.data()) == DAFS_HIP_OK);
    EXPECT(std::string(out.data()) == "(?.?)?." && std::string(out.data() + 8) == ".?(?.?)");
    std::vector<char> four(4 * 8);
    EXPECT(dafs_host_row_constraint_levels(7, mask, ss, level, 4, "GAGACAC", four.data()) == DAFS_HIP_OK);
    EXPECT(std::string(four.data() + 16).empty() && std::string(four.data() + 24).empty());
    std::vector<char> one(8);
    EXPECT(dafs_host_row_constraint_levels(7, mask, ss, level, 1, "GAGACAC", one.data()) == DAFS_HIP_EINVAL);  // a level the call has not
    EXPECT(dafs_host_row_constraint_levels(7, mask, ss, nullptr, 1, "GAGACAC", one.data()) == DAFS_HIP_OK);     // NULL: all of level 0
    char plain[8];
    EXPECT(dafs_host_row_constraint(7, mask, ss, "GAGACAC", plain) == DAFS_HIP_OK && std::string(one.data()) == plain);
    EXPECT(dafs_host_row_constraint_levels(7, mask, ss, level, 0, "GAGACAC", out.data()) == DAFS_HIP_EINVAL);
    EXPECT(dafs_host_row_constraint_levels(7, mask, ss, level, 5, "GAGACAC", out.data()) == DAFS_HIP_EINVAL);
    EXPECT(dafs_host_row_constraint_levels(7, mask, ss, level, 2, "GAGACA", out.data()) == DAFS_HIP_EINVAL);
    EXPECT(dafs_host_row_constraint_levels(7, mask, ss, level, 2, "GAGACACA", out.data()) == DAFS_HIP_EINVAL);
    EXPECT(dafs_host_row_constraint_levels(7, mask, ss, level, 2, nullptr, out.data()) == DAFS_HIP_EINVAL);
  }
  {  // a row with gaps: three residues, strings of 3 + 1 bytes
    const uint8_t mask[] = {1, 0, 0, 0, 1, 0, 1};
    const uint32_t ss[] = {4, N, 6, N, N, N, N};
    const uint8_t level[] = {0, F, 1, F, 0, F, 1};
    std::vector<char> out(2 * 4);
    EXPECT(dafs_host_row_constraint_levels(7, mask, ss, level, 2, "GCC", out.data()) == DAFS_HIP_OK);
    EXPECT(std::string(out.data()) == "???" && std::string(out.data() + 4).empty());
  }
  {  // no columns, no residues
    char out[2] = {'x', 'x'};
    EXPECT(dafs_host_row_constraint_levels(0, nullptr, nullptr, nullptr, 2, "", out) == DAFS_HIP_OK && out[0] == 0 && out[1] == 0);
  }
}

int main() {
  reader();
  constraints();
  if (failures) printf("%d checks failed\n", failures);
  return failures ? 1 : 0;
}
