// tests/host_call_main.cpp -- a stand-alone program over dafs_amd/csrc/call_host.h, what the per-call entry points share on
// the host: the offset carver, the readers of the environment knobs, the structure check and the distance of one pair of rows
// (against dafs_host_nj_distances, to the bit).  test_bootstrap_cpu.py compiles it with dafs_amd/csrc/host_tree.cpp under
// -fsanitize=address,undefined, with no ROCm include path, and requires exit status 0 and an empty stderr.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../dafs_amd/csrc/call_host.h"

// the library's error text lives in capi.cpp, which needs HIP: this program brings its own
static std::string g_error;
namespace dafs {
void set_last_error(const char* msg) { g_error = msg; }
}

static int failures = 0;
#define EXPECT(cond)                                                   \
  do {                                                                 \
    if (!(cond)) {                                                     \
      printf("%s:%d: %s is false\n", __FILE__, __LINE__, #cond);       \
      ++failures;                                                      \
    }                                                                  \
  } while (0)

static void carver() {
  const size_t sizes[] = {1, 0, 255, 256, 257, 0, 100000, 4};
  dafs::carve cv;
  size_t sum = 0, end = 0;
  EXPECT(cv.bytes() == 0 && cv.reserve_bytes() == 256);
  for (size_t b : sizes) {
    const size_t at = cv.take(b);
    EXPECT(at % 256 == 0);
    EXPECT(at == end);  // right behind the piece before it: nothing overlaps, a piece of no bytes takes no room
    end = at + (b + 255) / 256 * 256;
    EXPECT(end >= at + b && end - (at + b) < 256);
    sum += (b + 255) / 256 * 256;
    EXPECT(cv.bytes() == sum && cv.bytes() == end);
  }
  EXPECT(cv.reserve_bytes() == sum + 256);
}

static uint64_t knob(const char* value, uint64_t lo, uint64_t hi, uint64_t fallback) {
  if (value) setenv("DAFS_TEST_KNOB", value, 1);
  else unsetenv("DAFS_TEST_KNOB");
  return dafs::env_uint("DAFS_TEST_KNOB", lo, hi, fallback);
}
static bool off(const char* value) {
  if (value) setenv("DAFS_TEST_KNOB", value, 1);
  else unsetenv("DAFS_TEST_KNOB");
  return dafs::env_off("DAFS_TEST_KNOB");
}

static void knobs() {
  EXPECT(knob(nullptr, 1, 32, 77) == 77);
  EXPECT(knob("", 1, 32, 77) == 77);
  EXPECT(knob("7", 1, 32, 77) == 7);
  EXPECT(knob("007", 1, 32, 77) == 7);
  EXPECT(knob("1", 1, 32, 77) == 1 && knob("32", 1, 32, 77) == 32);
  EXPECT(knob("0", 1, 32, 77) == 77 && knob("33", 1, 32, 77) == 77);
  EXPECT(knob("0", 0, 32, 77) == 0);
  for (const char* bad : {"12abc", " 7", "7 ", "+7", "-7", "abc", "0x10", "7.0", "18446744073709551616", "99999999999999999999999"})
    EXPECT(knob(bad, 0, UINT64_MAX, 77) == 77);
  EXPECT(knob("18446744073709551615", 0, UINT64_MAX, 77) == ULLONG_MAX);
  EXPECT(knob("18446744073709551615", 0, UINT64_MAX - 1, 77) == 77);
  EXPECT(!off(nullptr) && !off("") && off("0") && off("00") && !off("1") && !off("abc") && !off("0abc") && !off(" 0") && !off("-0"));
  auto real = [](const char* value) {
    setenv("DAFS_TEST_KNOB", value, 1);
    return dafs::env_double("DAFS_TEST_KNOB", 0.25);
  };
  EXPECT(real("0.5") == 0.5 && real("0") == 0.0 && real("-1") == 0.25 && real("abc") == 0.25 && real("") == 0.25);
  unsetenv("DAFS_TEST_KNOB");
  EXPECT(dafs::env_double("DAFS_TEST_KNOB", 0.25) == 0.25);
}

static void structures() {
  const uint32_t none = DAFS_HIP_NONE;
  std::vector<uint8_t> used(3, 9);  // the scratch comes in any state
  const uint32_t good[8] = {7, 5, none, none, none, none, none, none};
  EXPECT(dafs::structure_ok(good, 8, used) && used.size() == 8);
  const uint32_t empty[4] = {none, none, none, none};
  EXPECT(dafs::structure_ok(empty, 4, used) && dafs::structure_ok(empty, 0, used));
  const uint32_t self[4] = {none, 1, none, none}, back[4] = {none, none, 1, none}, symmetric[4] = {3, none, none, 0};
  EXPECT(!dafs::structure_ok(self, 4, used) && !dafs::structure_ok(back, 4, used) && !dafs::structure_ok(symmetric, 4, used));
  const uint32_t beyond[4] = {4, none, none, none}, far[4] = {none, none, none - 1, none};
  EXPECT(!dafs::structure_ok(beyond, 4, used) && !dafs::structure_ok(far, 4, used));
  const uint32_t shared_right[4] = {3, 3, none, none}, right_is_left[4] = {1, 2, none, none};
  EXPECT(!dafs::structure_ok(shared_right, 4, used) && !dafs::structure_ok(right_is_left, 4, used));
  EXPECT(dafs::structure_ok(good, 8, used));  // and the scratch of a refusal serves the next call
}

static void distances() {
  // a grid of (mism, comp) as the matrices of dafs_host_nj_distances: row 0 against every other row
  std::vector<uint32_t> comps = {0, 1, 2, 3, 4, 7, 100, 101, 1000, 1048576, 4000000000u};
  for (int model : {DAFS_NJ_P, DAFS_NJ_JC})
    for (uint32_t comp : comps) {
      std::vector<uint32_t> mism = {0, 1, comp / 4, comp / 2, comp - comp / 4, comp};
      for (uint64_t m = (3 * (uint64_t)comp) / 4; m < (3 * (uint64_t)comp) / 4 + 3; ++m) mism.push_back((uint32_t)(m ? m - 1 : 0));  // around 4m = 3c
      std::vector<uint32_t> kept;
      for (uint32_t m : mism)
        if (m <= comp) kept.push_back(m);
      const uint32_t n = (uint32_t)kept.size() + 1;
      std::vector<uint32_t> ident((size_t)n * n, 0), aligned((size_t)n * n, 0);
      for (uint32_t s = 1; s < n; ++s)
        for (size_t at : {(size_t)s, (size_t)s * n}) { aligned[at] = comp; ident[at] = comp - kept[s - 1]; }
      std::vector<double> dist((size_t)n * n, -1.0);
      EXPECT(dafs_host_nj_distances(n, ident.data(), aligned.data(), model, dist.data()) == DAFS_HIP_OK);
      for (uint32_t s = 1; s < n; ++s) {
        const double d = dafs::nj_pair_distance(model, kept[s - 1], comp);
        EXPECT(!memcmp(&d, &dist[s], 8) && !memcmp(&d, &dist[(size_t)s * n], 8));
        if (comp == 0) EXPECT(d == (model == DAFS_NJ_P ? 1.0 : 3.0));
        if (model == DAFS_NJ_JC && 4 * (uint64_t)kept[s - 1] >= 3 * (uint64_t)comp) EXPECT(d == 3.0);
        if (model == DAFS_NJ_JC) EXPECT(d >= 0.0 && d <= 3.0);
      }
      EXPECT(dist[0] == 0.0 && dist[(size_t)n * n - 1] == 0.0);
    }
  // the refusals stay with the entry point
  const uint32_t one = 1, two = 2;
  double d = 0.0;
  EXPECT(dafs_host_nj_distances(0, &one, &one, DAFS_NJ_JC, &d) == DAFS_HIP_EINVAL && g_error == "nj_distances: a missing argument");
  EXPECT(dafs_host_nj_distances(1, &one, &one, 7, &d) == DAFS_HIP_EINVAL && g_error == "nj_distances: unknown model");
  const uint32_t id2[4] = {0, two, two, 0}, al2[4] = {0, one, one, 0};
  double d2[4];
  EXPECT(dafs_host_nj_distances(2, id2, al2, DAFS_NJ_P, d2) == DAFS_HIP_EINVAL && g_error == "nj_distances: more identical columns than aligned ones");
  EXPECT(dafs::refuse("why") == DAFS_HIP_EINVAL && g_error == "why");
  EXPECT(dafs::mix64(0) == 0 && dafs::mix64(0x9E3779B97F4A7C15ull) == 0xE220A8397B1DCDAFull);  // splitmix64's first output from state 0
}

int main() {
  carver();
  knobs();
  structures();
  distances();
  if (failures) printf("%d checks failed\n", failures);
  return failures ? 1 : 0;
}
