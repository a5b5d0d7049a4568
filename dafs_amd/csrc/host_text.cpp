// dafs_amd/csrc/host_text.cpp -- the text formats and memory estimates of both drivers as C entry points (include/dafs_hip.h,
// "host text"): the Stockholm block, the --covariation, --pairwise-scores, --identity and --compare tables, the Newick line of --phylogeny, its bootstrap support and the table of --phylogeny-support,
// the seed reader of --seed, the estimates and the greedy chunking.  The C++ command line calls them directly and the Python driver through capi.py, so every byte and
// every formula is defined here once.  Host logic only: nothing here includes HIP or touches a device.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <new>
#include <set>
#include <sstream>
#include <string>
#include <utility>
#include <vector>

#include "../../include/dafs_hip.h"
#include "last_error.h"
#include "tree_support.h"

namespace {

char* copy_text(const std::string& s) {
  char* p = (char*)malloc(s.size() + 1);
  if (!p) throw std::bad_alloc();
  memcpy(p, s.c_str(), s.size() + 1);
  return p;
}

// the entry points' frame: the text of body() into *out; a std::string thrown by body() is a refusal
template <class F>
int text_out(char** out, F body) {
  if (!out) return DAFS_HIP_EINVAL;
  *out = nullptr;
  try {
    *out = copy_text(body());
    return DAFS_HIP_OK;
  } catch (const std::string& refusal) {
    dafs::set_last_error(refusal.c_str());
    return DAFS_HIP_EINVAL;
  } catch (const std::bad_alloc&) {
    return DAFS_HIP_ENOMEM;
  }
}

const std::string kBadArgument = "host text: invalid argument";

std::vector<std::string> strings(uint32_t n, const char* const* s) {
  std::vector<std::string> out(n);
  for (uint32_t k = 0; k < n; ++k) {
    if (!s || !s[k]) throw kBadArgument;
    out[k] = s[k];
  }
  return out;
}

std::string joined(const std::vector<std::string>& v) {
  std::string out;
  for (size_t k = 0; k < v.size(); ++k) out += (k ? "\n" : "") + v[k];
  return out;
}

// isspace() and isalpha() as the "C" locale has them, whatever locale the host process has set
const char kSpace[] = " \t\n\v\f\r";
bool is_space(char ch) { return memchr(kSpace, ch, sizeof kSpace - 1) != nullptr; }
bool is_alpha(char ch) { return (ch >= 'A' && ch <= 'Z') || (ch >= 'a' && ch <= 'z'); }

// Infernal's PP character: '*' for p >= 0.95, else the digit floor(p * 10 + 0.5), in double
char pp_char(double p) {
  if (p >= 0.95) return '*';
  return (char)('0' + (int)std::floor(p * 10.0 + 0.5));
}

// rows in stdout order: name, printed text and the reliabilities of its residues; col_rel per column ('.' where a column
// holds no residue).  Labels padded to the longest plus one.  tree_line nullptr: no "#=GF CC" line; rf: per column a seed
// column ('x') or an insert column ('.') of --seed, written as "#=GC RF" after PP_cons (nullptr: no RF line).  cov: the
// characters of "#=GC cov_SS_cons", written directly after PP_cons (nullptr: no such line, labels as wide as without it).
// row_ss: per row its own structure in the row's columns, written as "#=GR <name> SS" after its PP line (nullptr: no such lines).
std::string stockholm_block(const char* tree_line, const std::vector<std::string>& names, const std::vector<std::string>& rows,
                            const double* const* rel, const double* col_rel, uint32_t len, const std::string& ss, const uint8_t* rf,
                            const char* cov, const std::vector<std::string>* row_ss) {
  size_t width = std::max(std::string("#=GC SS_cons").size(), std::string("#=GC PP_cons").size());
  if (cov) width = std::max(width, std::string("#=GC cov_SS_cons").size());
  for (const std::string& nm : names) width = std::max(width, nm.size() + 8);  // "#=GR " + name + " PP"
  ++width;
  auto label = [&](const std::string& l) { return l + std::string(width - l.size(), ' '); };
  std::string out = "# STOCKHOLM 1.0\n";
  if (tree_line) out += "#=GF CC " + std::string(tree_line) + "\n";
  for (size_t r = 0; r < rows.size(); ++r) {
    out += label(names[r]) + rows[r] + "\n";
    std::string pp(rows[r].size(), '.');
    for (size_t c = 0, k = 0; c < rows[r].size(); ++c)
      if (rows[r][c] != '-') pp[c] = pp_char(rel[r][k++]);
    out += label("#=GR " + names[r] + " PP") + pp + "\n";
    if (row_ss) out += label("#=GR " + names[r] + " SS") + (*row_ss)[r] + "\n";
  }
  std::string cons(len, '.');
  for (size_t c = 0; c < len; ++c)
    for (const std::string& row : rows)
      if (row[c] != '-') { cons[c] = pp_char(col_rel[c]); break; }
  out += label("#=GC SS_cons") + ss + "\n" + label("#=GC PP_cons") + cons + "\n";
  if (cov) out += label("#=GC cov_SS_cons") + std::string(cov) + "\n";
  if (rf) {
    std::string line(len, '.');
    for (size_t c = 0; c < len; ++c)
      if (rf[c]) line[c] = 'x';
    out += label("#=GC RF") + line + "\n";
  }
  out += "//\n";
  return out;
}

// The merged alignment of a --seed-each run: all rows, then the PP lines of the rows that have values
// (rel[r] not null: the placed rows), SS_cons, PP_cons, RF.  PP_cons is the mean over those rows' values per column, a running
// double sum in row order, '.' where none of them has a residue; col_out (optional) receives the means, NaN for '.'.
std::string stockholm_block_merged(const std::vector<std::string>& names, const std::vector<std::string>& rows, const double* const* rel,
                                   uint32_t len, const std::string& ss, const uint8_t* rf, double* col_out) {
  size_t width = std::string("#=GC SS_cons").size();
  for (size_t r = 0; r < rows.size(); ++r) width = std::max(width, names[r].size() + (rel[r] ? 8 : 0));  // "#=GR " + name + " PP"
  ++width;
  auto label = [&](const std::string& l) { return l + std::string(width - l.size(), ' '); };
  std::string out = "# STOCKHOLM 1.0\n";
  for (size_t r = 0; r < rows.size(); ++r) out += label(names[r]) + rows[r] + "\n";
  std::vector<double> sum(len, 0.0);
  std::vector<uint32_t> cnt(len, 0);
  for (size_t r = 0; r < rows.size(); ++r) {
    if (!rel[r]) continue;
    std::string pp(len, '.');
    for (size_t c = 0, k = 0; c < len; ++c)
      if (rows[r][c] != '-') {
        const double v = rel[r][k++];
        pp[c] = pp_char(v);
        sum[c] += v;
        ++cnt[c];
      }
    out += label("#=GR " + names[r] + " PP") + pp + "\n";
  }
  std::string cons(len, '.'), line(len, '.');
  for (size_t c = 0; c < len; ++c) {
    const double mean = cnt[c] ? sum[c] / (double)cnt[c] : std::nan("");
    if (cnt[c]) cons[c] = pp_char(mean);
    if (col_out) col_out[c] = mean;
    if (rf[c]) line[c] = 'x';
  }
  out += label("#=GC SS_cons") + ss + "\n" + label("#=GC PP_cons") + cons + "\n" + label("#=GC RF") + line + "\n//\n";
  return out;
}

// --covariation
const double kCovEMax = 0.05;  // the cut of the table's `other` pairs: fixed (e_max moves cov_SS_cons only)

std::string fmt9d(double v) {
  if (std::isnan(v)) return "nan";
  char buf[64];
  snprintf(buf, sizeof buf, "%.9g", v);
  return buf;
}

// --seed: the seed alignment
std::vector<std::string> fields(const std::string& s) {
  std::vector<std::string> out;
  size_t b = s.find_first_not_of(kSpace);
  while (b != std::string::npos) {
    const size_t e = s.find_first_of(kSpace, b);
    out.push_back(s.substr(b, e == std::string::npos ? std::string::npos : e - b));
    b = e == std::string::npos ? e : s.find_first_not_of(kSpace, e);
  }
  return out;
}

// Stockholm when the first line is "# STOCKHOLM 1.0": the first alignment up to "//", interleaved blocks concatenated by
// name, '#' lines ignored, every other non-blank line "name row".  Otherwise aligned FASTA as `dafs` prints it: lines
// before the first '>' ignored, leading blanks of a name stripped, a record named SS_cons skipped, rows over several lines.
// structure (optional): the "#=GC SS_cons" lines of that first alignment concatenated in order, or the SS_cons record; *has says
// whether the file holds one.
void parse_seed(const std::string& text, std::vector<std::string>& names, std::vector<std::string>& rows, std::string* structure = nullptr,
                bool* has = nullptr) {
  if (text.find('\0') != std::string::npos) throw std::string("seed: the file holds a NUL byte");  // names and rows are C strings
  std::istringstream is(text);
  std::vector<std::string> lines;
  std::string ln;
  while (std::getline(is, ln)) {
    const size_t e = ln.find_last_not_of(kSpace);
    lines.push_back(e == std::string::npos ? std::string() : ln.substr(0, e + 1));
  }
  if (!lines.empty() && lines[0] == "# STOCKHOLM 1.0") {
    std::map<std::string, size_t> at;
    for (size_t k = 1; k < lines.size(); ++k) {
      const std::string& l = lines[k];
      if (l == "//") break;
      if (structure && l.compare(0, 4, "#=GC") == 0) {
        const std::vector<std::string> f = fields(l);
        if (f.size() >= 2 && f[1] == "SS_cons") {
          if (f.size() != 3) throw "seed: line " + std::to_string(k + 1) + " is not '#=GC SS_cons structure'";
          *structure += f[2];
          *has = true;
        }
      }
      if (l.empty() || l[0] == '#') continue;  // rstripped: a blank line is empty
      const std::vector<std::string> f = fields(l);
      if (f.size() != 2) throw "seed: line " + std::to_string(k + 1) + " is neither a #= annotation nor 'name row'";
      if (!at.count(f[0])) {
        at[f[0]] = names.size();
        names.push_back(f[0]);
        rows.push_back(std::string());
      }
      rows[at[f[0]]] += f[1];
    }
    return;
  }
  bool keep = false, in_ss = false;
  for (const std::string& l : lines) {
    if (!l.empty() && l[0] == '>') {
      const size_t b = l.find_first_not_of(kSpace, 1);
      const std::string nm = b == std::string::npos ? std::string() : l.substr(b);
      keep = nm != "SS_cons";
      in_ss = !keep && structure;
      if (in_ss) {
        if (*has) throw std::string("seed: more than one SS_cons record");
        *has = true;
      }
      if (keep) {
        names.push_back(nm);
        rows.push_back(std::string());
      }
    } else if (keep) {
      for (const std::string& f : fields(l)) rows.back() += f;
    } else if (in_ss) {
      for (const std::string& f : fields(l)) *structure += f;
    }
  }
}

// The pairs of a structure line: "()", "<>", "[]", "{}" each matched with its own kind, letters and ". , : _ - ~" unpaired.
// partner[c] = the other column of c's pair, DAFS_HIP_NONE for an unpaired column.
std::vector<uint32_t> structure_pairs(const std::string& st) {
  const std::string open = "(<[{", close = ")>]}", unpaired = ".,:_-~";
  std::vector<uint32_t> partner(st.size(), DAFS_HIP_NONE);
  std::vector<size_t> stack[4];
  for (size_t c = 0; c < st.size(); ++c) {
    const char ch = st[c];
    size_t k;
    if ((k = open.find(ch)) != std::string::npos) stack[k].push_back(c);
    else if ((k = close.find(ch)) != std::string::npos) {
      if (stack[k].empty()) throw "seed: SS_cons has a '" + std::string(1, ch) + "' at column " + std::to_string(c + 1) + " that closes nothing";
      partner[c] = (uint32_t)stack[k].back();
      partner[stack[k].back()] = (uint32_t)c;
      stack[k].pop_back();
    } else if (!is_alpha(ch) && unpaired.find(ch) == std::string::npos)
      throw "seed: SS_cons holds '" + std::string(1, ch) + "', which is neither a bracket, a letter nor one of \".,:_-~\"";
  }
  for (size_t k = 0; k < 4; ++k)
    if (!stack[k].empty()) throw "seed: SS_cons has a '" + std::string(1, open[k]) + "' at column " + std::to_string(stack[k].back() + 1) + " that is never closed";
  // all kinds merged: the pairs must nest
  std::vector<uint32_t> st_open;
  for (uint32_t c = 0; c < partner.size(); ++c) {
    if (partner[c] == DAFS_HIP_NONE) continue;
    if (partner[c] > c) st_open.push_back(c);
    else {
      if (st_open.back() != partner[c])
        throw "seed: the pairs of SS_cons cross (columns " + std::to_string(st_open.back() + 1) + " and " + std::to_string(partner[c] + 1) +
            " are open at column " + std::to_string(c + 1) + ")";
      st_open.pop_back();
    }
  }
  return partner;
}

// The pairs of a structure line that may cross: the groups "()", "[]", "{}", "<>" and then the letters
// 'A'..'Z' (upper case opens, the same letter in lower case closes), each matched last-in-first-out with itself; ". , : _ - ~"
// unpaired.  partner as structure_pairs gives it, group[c] the group of c's pair (0..29).  Nothing is said about crossing here.
const char kKnotOpen[] = "([{<", kKnotClose[] = ")]}>";
const uint32_t kKnotGroups = 30;

char knot_open_char(uint32_t g) { return g < 4 ? kKnotOpen[g] : (char)('A' + (g - 4)); }
char knot_close_char(uint32_t g) { return g < 4 ? kKnotClose[g] : (char)('a' + (g - 4)); }

std::vector<uint32_t> structure_pairs_groups(const std::string& st, std::vector<uint8_t>& group) {
  const std::string open = kKnotOpen, close = kKnotClose, unpaired = ".,:_-~";
  std::vector<uint32_t> partner(st.size(), DAFS_HIP_NONE);
  group.assign(st.size(), 0xFF);
  std::vector<size_t> stack[kKnotGroups];
  for (size_t c = 0; c < st.size(); ++c) {
    const char ch = st[c];
    size_t k;
    if ((k = open.find(ch)) != std::string::npos) stack[k].push_back(c);
    else if (ch >= 'A' && ch <= 'Z') stack[4 + (ch - 'A')].push_back(c);
    else if ((k = close.find(ch)) != std::string::npos || (ch >= 'a' && ch <= 'z')) {
      if (k == std::string::npos) k = 4 + (size_t)(ch - 'a');
      if (stack[k].empty()) throw "seed: SS_cons has a '" + std::string(1, ch) + "' at column " + std::to_string(c + 1) + " that closes nothing";
      partner[c] = (uint32_t)stack[k].back();
      partner[stack[k].back()] = (uint32_t)c;
      group[c] = group[stack[k].back()] = (uint8_t)k;
      stack[k].pop_back();
    } else if (unpaired.find(ch) == std::string::npos)
      throw "seed: SS_cons holds '" + std::string(1, ch) + "', which is neither a bracket, a letter nor one of \".,:_-~\"";
  }
  for (uint32_t k = 0; k < kKnotGroups; ++k)
    if (!stack[k].empty())
      throw "seed: SS_cons has a '" + std::string(1, knot_open_char(k)) + "' at column " + std::to_string(stack[k].back() + 1) + " that is never closed";
  return partner;
}

// The level of every group of a cleaned structure (ss: the partner at the left column of a pair; group: per column): group
// after group, a non-empty one goes to the lowest level at which none of its pairs crosses a pair already placed there.
// level[c]: the pair's level at both of its columns, 0xFF at unpaired ones.
void assign_levels(const std::vector<uint32_t>& ss, const std::vector<uint8_t>& group, uint8_t* level) {
  typedef std::pair<uint32_t, uint32_t> pr;
  std::vector<pr> placed[DAFS_HIP_MAX_LEVELS];
  for (size_t c = 0; c < ss.size(); ++c) level[c] = 0xFF;
  for (uint32_t g = 0; g < kKnotGroups; ++g) {
    std::vector<pr> mine;
    for (uint32_t c = 0; c < ss.size(); ++c)
      if (ss[c] != DAFS_HIP_NONE && group[c] == g) mine.push_back(pr(c, ss[c]));
    if (mine.empty()) continue;
    uint32_t lv = 0;
    for (; lv < DAFS_HIP_MAX_LEVELS; ++lv) {
      bool crosses = false;
      for (size_t a = 0; a < mine.size() && !crosses; ++a)
        for (size_t b = 0; b < placed[lv].size() && !crosses; ++b) {
          const uint32_t i = mine[a].first, j = mine[a].second, p = placed[lv][b].first, q = placed[lv][b].second;
          crosses = (p < i && i < q && q < j) || (i < p && p < j && j < q);
        }
      if (!crosses) break;
    }
    if (lv == DAFS_HIP_MAX_LEVELS)
      throw "seed: the '" + std::string(1, knot_open_char(g)) + "' '" + std::string(1, knot_close_char(g)) + "' pairs of SS_cons cross a pair of each of the " +
          std::to_string(DAFS_HIP_MAX_LEVELS) + " levels a structure may have";
    for (const pr& x : mine) {
      placed[lv].push_back(x);
      level[x.first] = level[x.second] = (uint8_t)lv;
    }
  }
}

// refuses an empty seed, rows of unequal length, a character that is neither a letter nor a gap ('.', '-') and a row without
// residues; drops the all-gap columns and writes every gap as '-'
// kept (optional): the columns that stay.
void clean_seed(const std::vector<std::string>& names, std::vector<std::string>& rows, std::vector<size_t>* kept = nullptr) {
  if (rows.empty()) throw std::string("seed: no rows");
  auto gap = [](char ch) { return ch == '.' || ch == '-'; };
  for (size_t r = 0; r < rows.size(); ++r) {
    if (rows[r].size() != rows[0].size())
      throw "seed: rows of unequal length (" + names[0] + ": " + std::to_string(rows[0].size()) + " columns, " + names[r] + ": " +
          std::to_string(rows[r].size()) + ")";
    bool residue = false;
    for (char ch : rows[r]) {
      if (!gap(ch) && !is_alpha(ch))
        throw "seed: row " + names[r] + " holds '" + std::string(1, ch) + "', which is neither a letter nor a gap";
      residue |= !gap(ch);
    }
    if (!residue) throw "seed: row " + names[r] + " has no residues";
  }
  std::vector<size_t> keep;  // not empty: every row has a residue
  for (size_t c = 0; c < rows[0].size(); ++c)
    for (const std::string& row : rows)
      if (!gap(row[c])) { keep.push_back(c); break; }
  for (std::string& row : rows) {
    std::string out;
    for (size_t c : keep) out += gap(row[c]) ? '-' : row[c];
    row.swap(out);
  }
  if (kept) kept->swap(keep);
}

// CONTRAfold's alphabet, case-insensitive "ACGU" (InferenceEngine constructor); everything else, T included, is its symbol 4
int fold_symbol(char ch) {
  switch (ch) {
    case 'A': case 'a': return 0;
    case 'C': case 'c': return 1;
    case 'G': case 'g': return 2;
    case 'U': case 'u': return 3;
    default: return 4;
  }
}

// per sequence of a file, in input order: the first whitespace-separated word of its header, "seq<k>" (k 1-based) for an
// empty one, ".2", ".3", ... appended to the second, third, ... occurrence of a name
std::vector<std::string> stockholm_names(const std::vector<std::string>& headers) {
  std::vector<std::string> out;
  std::map<std::string, int> seen;
  for (size_t k = 0; k < headers.size(); ++k) {
    const std::string& h = headers[k];
    size_t b = 0;
    while (b < h.size() && is_space(h[b])) ++b;
    size_t e = b;
    while (e < h.size() && !is_space(h[e])) ++e;
    const std::string nm = e > b ? h.substr(b, e - b) : "seq" + std::to_string(k + 1);
    const int c = ++seen[nm];
    out.push_back(c == 1 ? nm : nm + "." + std::to_string(c));
  }
  return out;
}

}  // namespace

extern "C" void dafs_host_free(void* p) { free(p); }

extern "C" char dafs_host_pp_char(double p) { return pp_char(p); }

extern "C" int dafs_host_stockholm_names(uint32_t n, const char* const* header_strs, char** names) {
  return text_out(names, [&]() { return joined(stockholm_names(strings(n, header_strs))); });
}

extern "C" int dafs_host_stockholm_block_rows(const char* tree_line, uint32_t n, uint32_t len, const char* const* names,
                                              const char* const* rows, const double* const* residue_rel, const double* col_rel,
                                              const char* ss, const uint8_t* rf, const char* cov, const char* const* row_ss, char** block) {
  return text_out(block, [&]() {
    const std::vector<std::string> nm = strings(n, names), rw = strings(n, rows);
    if (!ss || (len && !col_rel) || (n && !residue_rel)) throw kBadArgument;
    for (uint32_t r = 0; r < n; ++r) {
      if (rw[r].size() != len) throw "stockholm block: row " + nm[r] + " has " + std::to_string(rw[r].size()) + " columns, not " + std::to_string(len);
      if (!residue_rel[r] && rw[r] != std::string(len, '-')) throw kBadArgument;
    }
    std::vector<std::string> rs;
    if (row_ss) {
      rs = strings(n, row_ss);
      for (uint32_t r = 0; r < n; ++r) {
        if (rs[r].size() != len)
          throw "stockholm block: the structure of row " + nm[r] + " has " + std::to_string(rs[r].size()) + " columns, not " + std::to_string(len);
        for (uint32_t c = 0; c < len; ++c)
          if (rw[r][c] == '-' && rs[r][c] != '.')
            throw "stockholm block: the structure of row " + nm[r] + " has '" + std::string(1, rs[r][c]) + "' at gap column " + std::to_string(c + 1);
      }
    }
    return stockholm_block(tree_line, nm, rw, residue_rel, col_rel, len, ss, rf, cov, row_ss ? &rs : nullptr);
  });
}

extern "C" int dafs_host_stockholm_block(const char* tree_line, uint32_t n, uint32_t len, const char* const* names, const char* const* rows,
                                         const double* const* residue_rel, const double* col_rel, const char* ss, const uint8_t* rf,
                                         const char* cov, char** block) {
  return dafs_host_stockholm_block_rows(tree_line, n, len, names, rows, residue_rel, col_rel, ss, rf, cov, nullptr, block);
}

extern "C" int dafs_host_stockholm_block_merged(uint32_t n, uint32_t len, const char* const* names, const char* const* rows,
                                                const double* const* residue_rel, const char* ss, const uint8_t* rf, double* col_rel, char** block) {
  return text_out(block, [&]() {
    const std::vector<std::string> nm = strings(n, names), rw = strings(n, rows);
    if (!ss || (len && !rf) || (n && !residue_rel)) throw kBadArgument;
    if (strlen(ss) != len) throw "stockholm block: the structure has " + std::to_string(strlen(ss)) + " columns, not " + std::to_string(len);
    for (uint32_t r = 0; r < n; ++r)
      if (rw[r].size() != len) throw "stockholm block: row " + nm[r] + " has " + std::to_string(rw[r].size()) + " columns, not " + std::to_string(len);
    return stockholm_block_merged(nm, rw, residue_rel, len, ss, rf, col_rel);
  });
}

extern "C" const char* dafs_host_merged_refusal(void) {
  return "a merged alignment needs the seed's structure (--seed-structure, seed_ss): without it there is no structure to print";
}

extern "C" uint8_t dafs_host_cov_code(char ch) {
  switch (ch) {
    case 'A': case 'a': return 0;
    case 'C': case 'c': return 1;
    case 'G': case 'g': return 2;
    case 'U': case 'u': case 'T': case 't': return 3;
    default: return 4;
  }
}

extern "C" int dafs_host_cov_ss_cons(uint32_t len, const uint32_t* ss, const double* pair_e, double e_max, char** chars) {
  return text_out(chars, [&]() {
    if (len && (!ss || !pair_e)) throw kBadArgument;
    std::string out(len, '.');
    for (uint32_t c = 0; c < len; ++c) {
      if (ss[c] == DAFS_HIP_NONE) continue;
      if (ss[c] >= len) throw std::string("cov_SS_cons: a pair's right column is outside the alignment");
      if (pair_e[c] <= e_max) out[c] = out[ss[c]] = '2';
    }
    return out;
  });
}

extern "C" int dafs_host_covariation_table(uint32_t n, uint32_t L, const uint8_t* code, const uint32_t* ss, const uint32_t* best,
                                           const double* bscore, const double* be, const double* pscore, const double* pe,
                                           const uint32_t* prow, const uint32_t* pcan, const uint32_t* ptyp, char** table) {
  return text_out(table, [&]() {
    if (L && (!ss || !best || !bscore || !be || !pscore || !pe || !prow || !pcan || !ptyp || (n && !code))) throw kBadArgument;
    for (uint32_t c = 0; c < L; ++c)
      if ((ss[c] != DAFS_HIP_NONE && ss[c] >= L) || (best[c] != DAFS_HIP_NONE && best[c] >= L))
        throw std::string("covariation table: a partner column is outside the alignment");
    std::ostringstream os;
    std::set<std::pair<uint32_t, uint32_t> > cons;
    for (uint32_t c = 0; c < L; ++c) {
      if (ss[c] == DAFS_HIP_NONE) continue;
      cons.insert(std::make_pair(c, ss[c]));
      os << c + 1 << "\t" << ss[c] + 1 << "\tss\t" << fmt9d(pscore[c]) << "\t" << fmt9d(pe[c]) << "\t" << prow[c] << "\t" << pcan[c] << "\t" << ptyp[c] << "\n";
    }
    std::map<std::pair<uint32_t, uint32_t>, uint32_t> other;  // pair -> the first column that names it
    for (uint32_t c = 0; c < L; ++c) {
      if (best[c] == DAFS_HIP_NONE || !(be[c] <= kCovEMax)) continue;
      const std::pair<uint32_t, uint32_t> pr(std::min(c, best[c]), std::max(c, best[c]));
      if (!cons.count(pr) && !other.count(pr)) other[pr] = c;
    }
    for (const auto& kv : other) {
      const uint32_t c1 = kv.first.first, c2 = kv.first.second, c = kv.second;
      uint32_t cnt[4][4] = {{0}};
      uint32_t both = 0;
      for (uint32_t r = 0; r < n; ++r) {
        const uint8_t a = code[(size_t)r * L + c1], b = code[(size_t)r * L + c2];
        if (a < 4 && b < 4) { ++cnt[a][b]; ++both; }
      }
      const uint32_t six[6] = {cnt[0][3], cnt[3][0], cnt[2][1], cnt[1][2], cnt[2][3], cnt[3][2]};  // AU UA GC CG GU UG
      uint32_t canonical = 0, types = 0;
      for (uint32_t v : six) { canonical += v; types += v ? 1 : 0; }
      os << c1 + 1 << "\t" << c2 + 1 << "\tother\t" << fmt9d(bscore[c]) << "\t" << fmt9d(be[c]) << "\t" << both << "\t" << canonical << "\t" << types << "\n";
    }
    return os.str();
  });
}

extern "C" const char* dafs_host_alistat_refusal(int which) {
  switch (which) {
    case DAFS_ALISTAT_NO_PAIRWISE:
      return "identity statistics (--identity, identity) cannot be combined with pairwise alignments (--pairwise, pipeline.pairwise): they "
             "go with a run, several files or a seed";
    case DAFS_ALISTAT_NR_NEEDS_MERGED:
      return "a non-redundant subset (--seed-nr, nr) selects rows of the merged alignment: it needs --seed-merged / merged";
    case DAFS_ALISTAT_NR_THRESHOLD:
      return "the threshold of the non-redundant subset (--seed-nr, nr) is a number in (0, 1]";
    case DAFS_ALISTAT_TOO_MANY_ROWS:
      return "identity statistics (--identity, identity) hold the whole identity matrix for their summary: at most 32768 rows";
    default:
      return "";
  }
}

extern "C" const char* dafs_host_phylogeny_refusal(int which) {
  switch (which) {
    case DAFS_PHYLOGENY_NO_PAIRWISE:
      return "a neighbour-joining tree (--phylogeny, phylogeny) cannot be combined with pairwise alignments (--pairwise, pipeline.pairwise): "
             "it goes with a run, several files or a seed";
    case DAFS_PHYLOGENY_NO_SEED_EACH:
      return "a neighbour-joining tree (--phylogeny, phylogeny) cannot be combined with per-sequence placements (--seed-each, "
             "pipeline.add_each): it goes with a run, several files or --seed";
    case DAFS_PHYLOGENY_TOO_MANY_ROWS:
      return "a neighbour-joining tree (--phylogeny, phylogeny, --cov-tree nj) holds the whole distance matrix on the device: at most 16384 rows";
    case DAFS_PHYLOGENY_MODEL_NEEDS_TREE:
      return "--phylogeny-model needs --phylogeny";
    case DAFS_PHYLOGENY_UNKNOWN_MODEL:
      return "the distance model of the neighbour-joining tree (--phylogeny-model, phylogeny) is jc or p";
    case DAFS_PHYLOGENY_COV_TREE_NEEDS_NULL:
      return "the tree of the covariation null (--cov-tree, tree) needs the tree null (--cov-null tree, null=\"tree\")";
    case DAFS_PHYLOGENY_UNKNOWN_COV_TREE:
      return "the tree of the covariation null (--cov-tree, tree) is average or nj";
    default:
      return "";
  }
}

extern "C" const char* dafs_host_bootstrap_refusal(int which) {
  switch (which) {
    case DAFS_BOOTSTRAP_NEEDS_TREE:
      return "--phylogeny-bootstrap, --phylogeny-seed and --phylogeny-support (phylogeny_bootstrap) need --phylogeny (phylogeny)";
    case DAFS_BOOTSTRAP_COUNT:
      return "the number of bootstrap replicates (--phylogeny-bootstrap, phylogeny_bootstrap) is 1 to 65536";
    case DAFS_BOOTSTRAP_NEEDS_REPLICATES:
      return "--phylogeny-seed and --phylogeny-support need bootstrap replicates (--phylogeny-bootstrap)";
    case DAFS_BOOTSTRAP_NO_COLUMN:
      return "bootstrap replicates (--phylogeny-bootstrap, phylogeny_bootstrap) need one used column at least";
    default:
      return "";
  }
}

extern "C" const char* dafs_host_transfer_refusal(int which) {
  switch (which) {
    case DAFS_TRANSFER_NEEDS_REPLICATES:
      return "the transfer bootstrap (--phylogeny-transfer, phylogeny_transfer) needs bootstrap replicates (--phylogeny-bootstrap, phylogeny_bootstrap)";
    default:
      return "";
  }
}

namespace {

// (200 s + B) / (2 B) in integers: the share of the replicates in percent, halves rounded up
uint32_t support_percent(int32_t s, uint32_t B) { return (uint32_t)((200ull * (uint64_t)s + B) / (2ull * B)); }

// The two children of the root carry one split.  It is shown once: on the left child if that is a join, otherwise on the
// right child.  The node that stays silent, or UINT32_MAX.
uint32_t silent_root_child(uint32_t n, const int32_t* left, const int32_t* right) {
  if (n < 2) return UINT32_MAX;
  const uint32_t root = 2 * n - 2;
  return (uint32_t)left[root] >= n ? (uint32_t)right[root] : UINT32_MAX;
}

// per node the depth of its split, min(leaves below, the rest); -1 for the root and trivial splits (a well-formed tree)
std::vector<int32_t> split_depths(uint32_t n, const int32_t* left, const int32_t* right) {
  const uint32_t T = 2 * n - 1;
  std::vector<uint32_t> below(T, 1);
  std::vector<int32_t> depth(T, -1);
  for (uint32_t v = 0; v + 1 < T; ++v) {
    if (v >= n) below[v] = below[(uint32_t)left[v]] + below[(uint32_t)right[v]];
    const uint32_t d = std::min(below[v], n - below[v]);
    if (d >= 2) depth[v] = (int32_t)d;
  }
  return depth;
}

// the transfer bootstrap expectation in percent, halves rounded up like support_percent; what the
// sum cannot be for its split and B throws
uint32_t transfer_percent(const char* who, int64_t transfer, int32_t depth, uint32_t B) {
  if (depth < 2 || !B) throw std::string(who) + ": a transfer sum on a trivial split";
  const uint64_t most = (uint64_t)B * (uint64_t)(depth - 1);
  if (transfer < 0 || (uint64_t)transfer > most) throw std::string(who) + ": a transfer sum above replicates x (depth - 1)";
  return (uint32_t)((200ull * (most - (uint64_t)transfer) + most) / (2ull * most));
}

}  // namespace

extern "C" int32_t dafs_host_transfer_percent(int64_t transfer, uint32_t depth, uint32_t B) {
  if (depth < 2 || depth > 0x7FFFFFFFu || !B || transfer < 0 || (uint64_t)transfer > (uint64_t)B * (depth - 1)) return -1;
  return (int32_t)transfer_percent("transfer percent", transfer, (int32_t)depth, B);
}

extern "C" int dafs_host_split_depth(uint32_t n, const int32_t* left, const int32_t* right, int32_t* depth) {
  auto refuse = [](const std::string& why) { dafs::set_last_error(why.c_str()); return DAFS_HIP_EINVAL; };
  if (!n || !left || !right || !depth) return refuse("split depth: invalid argument");
  if (const char* bad = dafs::tree_malformed(n, left, right)) return refuse(std::string("split depth: ") + bad);
  try {
    const std::vector<int32_t> d = split_depths(n, left, right);
    std::copy(d.begin(), d.end(), depth);
  } catch (const std::bad_alloc&) {
    return DAFS_HIP_ENOMEM;
  }
  return DAFS_HIP_OK;
}

// The Newick line of a tree in the arrays of dafs_host_build_tree.  The walk keeps its own stack of
// (node, next step), so a chain of any depth uses none of the call stack.  support (or null) labels the joins (section 23).
// transfer (or null; section 28) labels them with the transfer bootstrap expectation instead, under the same root-child rule.
static int newick_text(uint32_t n, const char* const* names, const int32_t* left, const int32_t* right, const double* length,
                       const int32_t* support, uint32_t B, char** out, const int64_t* transfer = nullptr) {
  return text_out(out, [&]() {
    if (!n || !left || !right) throw kBadArgument;
    if ((support || transfer) && !B) throw std::string("newick: support values need the number of replicates");
    if (n > 0x7FFFFFFFu / 2) throw std::string("newick: too many leaves");
    const std::vector<std::string> nm = strings(n, names);
    const uint32_t T = 2 * n - 1;
    std::vector<uint8_t> is_child(T, 0);  // the checks of dafs_host_cluster_cut
    for (uint32_t i = 0; i < T; ++i) {
      if (i < n) {
        if (left[i] != -1 || right[i] != -1) throw std::string("newick: malformed tree (a leaf with a child)");
        continue;
      }
      const int64_t ch[2] = {left[i], right[i]};
      if (ch[0] == ch[1]) throw std::string("newick: malformed tree (a join of a node with itself)");
      for (int64_t c : ch) {
        if (c < 0 || c >= (int64_t)i) throw std::string("newick: malformed tree (a child that is not an earlier node)");
        if (is_child[c]) throw std::string("newick: malformed tree (a node that is a child twice)");
        is_child[c] = 1;
      }
    }
    auto quoted = [](const std::string& s) {
      bool plain = !s.empty();
      for (char ch : s)
        if (strchr("()[]':;,", ch) || is_space(ch)) plain = false;
      if (plain) return s;
      std::string q = "'";
      for (char ch : s) { q += ch; if (ch == '\'') q += '\''; }
      return q + "'";
    };
    const uint32_t silent = support || transfer ? silent_root_child(n, left, right) : UINT32_MAX;
    const std::vector<int32_t> depth = transfer ? split_depths(n, left, right) : std::vector<int32_t>();
    std::string text;
    std::vector<std::pair<uint32_t, uint8_t> > stack;
    stack.push_back(std::make_pair(T - 1, (uint8_t)0));
    while (!stack.empty()) {
      const uint32_t node = stack.back().first;
      const uint8_t step = stack.back().second++;
      if (node < n) {
        text += quoted(nm[node]);
      } else if (step == 0) {
        text += "(";
        stack.push_back(std::make_pair((uint32_t)left[node], (uint8_t)0));
        continue;
      } else if (step == 1) {
        text += ",";
        stack.push_back(std::make_pair((uint32_t)right[node], (uint8_t)0));
        continue;
      } else {
        text += ")";
        if (support && node != T - 1 && node != silent && support[node] >= 0) {
          if ((uint32_t)support[node] > B) throw std::string("newick: a support value above the number of replicates");
          text += std::to_string(support_percent(support[node], B));
        }
        if (transfer && node != T - 1 && node != silent && transfer[node] >= 0)
          text += std::to_string(transfer_percent("newick", transfer[node], depth[node], B));
      }
      if (length && node != T - 1) text += ":" + fmt9d(length[node]);
      stack.pop_back();
    }
    return text + ";\n";
  });
}

extern "C" int dafs_host_newick(uint32_t n, const char* const* names, const int32_t* left, const int32_t* right, const double* length,
                                char** out) {
  return newick_text(n, names, left, right, length, nullptr, 0, out);
}

extern "C" int dafs_host_newick_support(uint32_t n, const char* const* names, const int32_t* left, const int32_t* right, const double* length,
                                        const int32_t* support, uint32_t B, char** out) {
  if (!support) {
    dafs::set_last_error(kBadArgument.c_str());
    return DAFS_HIP_EINVAL;
  }
  return newick_text(n, names, left, right, length, support, B, out);
}

extern "C" int dafs_host_newick_transfer(uint32_t n, const char* const* names, const int32_t* left, const int32_t* right, const double* length,
                                         const int64_t* transfer, uint32_t B, char** out) {
  if (!transfer) {
    dafs::set_last_error(kBadArgument.c_str());
    return DAFS_HIP_EINVAL;
  }
  return newick_text(n, names, left, right, length, nullptr, B, out, transfer);
}

// Bootstrap support: per node of the main tree the number of replicate trees that hold its split
extern "C" int dafs_host_tree_support(uint32_t n, const int32_t* left, const int32_t* right, uint32_t B, const int32_t* rep_left,
                                      const int32_t* rep_right, int32_t* support) {
  auto refuse = [](const std::string& why) { dafs::set_last_error(why.c_str()); return DAFS_HIP_EINVAL; };
  if (!n || !left || !right || !support || (B && (!rep_left || !rep_right))) return refuse("tree support: invalid argument");
  if (const char* bad = dafs::tree_malformed(n, left, right)) return refuse(std::string("tree support: ") + bad);
  const size_t T = 2 * (size_t)n - 1;
  for (uint32_t k = 0; k < B; ++k)
    if (const char* bad = dafs::tree_malformed(n, rep_left + k * T, rep_right + k * T))
      return refuse("tree support: replicate " + std::to_string(k) + ": " + bad);
  try {
    dafs::support_counter counter(n, left, right);
    for (uint32_t k = 0; k < B; ++k) counter.add(rep_left + k * T, rep_right + k * T);
    counter.result(support);
  } catch (const std::bad_alloc&) {
    return DAFS_HIP_ENOMEM;
  }
  return DAFS_HIP_OK;
}

// The table of --phylogeny-support: one line per non-trivial split of the main tree, the leaves on the side without the first row
// transfer (or null; section 28): the header names the measure and every line gains depth, transfer and tbe
static int support_table_text(uint32_t n, const char* const* names, const int32_t* left, const int32_t* right, const int32_t* support,
                              const int64_t* transfer, uint32_t B, uint64_t seed, int model, char** out) {
  return text_out(out, [&]() {
    if (!n || !left || !right || !support || !B) throw kBadArgument;
    if (model != DAFS_NJ_P && model != DAFS_NJ_JC) throw std::string(dafs_host_phylogeny_refusal(DAFS_PHYLOGENY_UNKNOWN_MODEL));
    const std::vector<std::string> nm = strings(n, names);
    if (const char* bad = dafs::tree_malformed(n, left, right)) throw std::string("support table: ") + bad;
    const uint32_t T = 2 * n - 1, silent = silent_root_child(n, left, right);
    std::ostringstream os;
    const std::vector<int32_t> depth = transfer ? split_depths(n, left, right) : std::vector<int32_t>();
    os << "# rows " << n << " replicates " << B << " seed " << seed << " model " << (model == DAFS_NJ_JC ? "jc" : "p")
       << (transfer ? " measure transfer" : "") << "\n";
    // below[v]: the leaves below v in ascending order, kept only while a node above still needs them
    std::vector<std::vector<uint32_t> > below(T);
    for (uint32_t v = 0; v < T; ++v) {
      if (v < n) {
        below[v].assign(1, v);
      } else {
        std::vector<uint32_t>& a = below[(uint32_t)left[v]];
        std::vector<uint32_t>& b = below[(uint32_t)right[v]];
        below[v].resize(a.size() + b.size());
        std::merge(a.begin(), a.end(), b.begin(), b.end(), below[v].begin());
        std::vector<uint32_t>().swap(a);
        std::vector<uint32_t>().swap(b);
      }
      if (v + 1 == T || v == silent || support[v] < 0) continue;
      if ((uint32_t)support[v] > B) throw std::string("support table: a support value above the number of replicates");
      std::vector<uint32_t> side;
      if (below[v][0] != 0) {
        side = below[v];
      } else {  // the rest of the leaves
        size_t at = 0;
        for (uint32_t leaf = 0; leaf < n; ++leaf) {
          if (at < below[v].size() && below[v][at] == leaf) ++at;
          else side.push_back(leaf);
        }
      }
      os << v + 1 << "\t" << support[v] << "\t" << B << "\t" << support_percent(support[v], B) << "\t" << side.size() << "\t";
      for (size_t k = 0; k < side.size(); ++k) os << (k ? "," : "") << nm[side[k]];
      if (transfer) os << "\t" << depth[v] << "\t" << transfer[v] << "\t" << transfer_percent("transfer table", transfer[v], depth[v], B);
      os << "\n";
    }
    return os.str();
  });
}

extern "C" int dafs_host_support_table(uint32_t n, const char* const* names, const int32_t* left, const int32_t* right, const int32_t* support,
                                       uint32_t B, uint64_t seed, int model, char** out) {
  return support_table_text(n, names, left, right, support, nullptr, B, seed, model, out);
}

extern "C" int dafs_host_transfer_table(uint32_t n, const char* const* names, const int32_t* left, const int32_t* right, const int32_t* support,
                                        const int64_t* transfer, uint32_t B, uint64_t seed, int model, char** out) {
  if (!transfer) {
    dafs::set_last_error(kBadArgument.c_str());
    return DAFS_HIP_EINVAL;
  }
  return support_table_text(n, names, left, right, support, transfer, B, seed, model, out);
}

// Alignment statistics: the cell code, the summary and the tables of --identity and --identity-matrix
extern "C" uint8_t dafs_host_ali_code(char ch) {
  if (ch == '-' || ch == '.') return 5;
  if (!is_alpha(ch)) return 255;
  return dafs_host_cov_code(ch);  // A C G U/T 0..3, every other letter 4
}

namespace {

double pid_of(uint32_t ident, uint32_t den) { return (double)ident / (double)den; }

// (i1, d1) is more identical than (i2, d2): no floating point decides an order
bool more_identical(uint32_t i1, uint32_t d1, uint32_t i2, uint32_t d2) { return (uint64_t)i1 * d2 > (uint64_t)i2 * d1; }

}  // namespace

extern "C" int dafs_host_identity_summary(uint32_t n, const uint32_t* ident, const uint32_t* res, double* summary) {
  if (!n || !summary || (n > 1 && (!ident || !res))) return DAFS_HIP_EINVAL;
  summary[0] = summary[1] = summary[2] = std::nan("");
  if (n == 1) return DAFS_HIP_OK;
  for (uint32_t r = 0; r < n; ++r)
    if (!res[r]) return DAFS_HIP_EINVAL;
  double sum = 0.0;
  uint32_t lo_i = 0, lo_d = 0, hi_i = 0, hi_d = 0;
  for (uint32_t r = 0; r < n; ++r)
    for (uint32_t s = r + 1; s < n; ++s) {
      const uint32_t i = ident[(size_t)r * n + s], d = std::min(res[r], res[s]);
      sum += pid_of(i, d);
      if (!lo_d || more_identical(lo_i, lo_d, i, d)) { lo_i = i; lo_d = d; }
      if (!hi_d || more_identical(i, d, hi_i, hi_d)) { hi_i = i; hi_d = d; }
    }
  summary[0] = sum / (double)((uint64_t)n * (n - 1) / 2);
  summary[1] = pid_of(lo_i, lo_d);
  summary[2] = pid_of(hi_i, hi_d);
  return DAFS_HIP_OK;
}

extern "C" int dafs_host_identity_table(uint32_t n, uint32_t len, const char* const* names, const uint32_t* res, const double* weight,
                                        const uint32_t* nearest, const uint32_t* nearest_ident, const uint32_t* nearest_den,
                                        const double* summary, char** table) {
  return text_out(table, [&]() {
    const std::vector<std::string> nm = strings(n, names);
    if (!n || !res || !weight || !nearest || !nearest_ident || !nearest_den || !summary) throw kBadArgument;
    std::ostringstream os;
    os << "# rows " << n << " columns " << len << " average " << fmt9d(summary[0]) << " min " << fmt9d(summary[1]) << " max " << fmt9d(summary[2]) << "\n";
    for (uint32_t r = 0; r < n; ++r) {
      os << r + 1 << "\t" << nm[r] << "\t" << res[r] << "\t" << fmt9d(weight[r]) << "\t";
      if (nearest[r] == DAFS_HIP_NONE) {
        os << "0\t-\tnan\n";
        continue;
      }
      if (nearest[r] >= n || !nearest_den[r]) throw std::string("identity table: a nearest row is outside the alignment");
      os << nearest[r] + 1 << "\t" << nm[nearest[r]] << "\t" << fmt9d(pid_of(nearest_ident[r], nearest_den[r])) << "\n";
    }
    return os.str();
  });
}

extern "C" int dafs_host_identity_matrix_table(uint32_t n, const char* const* names, const uint32_t* res, const uint32_t* ident,
                                               const uint32_t* aligned, char** table) {
  return text_out(table, [&]() {
    const std::vector<std::string> nm = strings(n, names);
    if (!n || !res || !ident || !aligned) throw kBadArgument;
    std::ostringstream os;
    for (uint32_t r = 0; r < n; ++r)
      for (uint32_t s = r + 1; s < n; ++s) {
        const uint32_t den = std::min(res[r], res[s]);
        if (!den) throw std::string("identity matrix: a row without residues");
        const size_t at = (size_t)r * n + s;
        os << r + 1 << "\t" << s + 1 << "\t" << nm[r] << "\t" << nm[s] << "\t" << ident[at] << "\t" << aligned[at] << "\t" << den << "\t"
           << fmt9d(pid_of(ident[at], den)) << "\n";
      }
    return os.str();
  });
}

extern "C" int dafs_host_stockholm_weights(const char* block, uint32_t n, const char* const* names, const double* weight, char** out) {
  return text_out(out, [&]() {
    const std::vector<std::string> nm = strings(n, names);
    if (!block || (n && !weight)) throw kBadArgument;
    const std::string text(block);
    const std::string first = "# STOCKHOLM 1.0\n";
    if (text.compare(0, first.size(), first) != 0) throw std::string("stockholm weights: not a Stockholm block");
    size_t at = first.size();
    while (text.compare(at, 5, "#=GF ") == 0) {
      const size_t nl = text.find('\n', at);
      if (nl == std::string::npos) throw std::string("stockholm weights: not a Stockholm block");
      at = nl + 1;
    }
    std::string lines;
    for (uint32_t r = 0; r < n; ++r) {
      char buf[64];
      snprintf(buf, sizeof buf, "%.6f", weight[r]);
      lines += "#=GS " + nm[r] + " WT " + buf + "\n";
    }
    return text.substr(0, at) + lines + text.substr(at);
  });
}

extern "C" int dafs_host_stockholm_nr(const char* block, uint32_t n, const char* const* names, const uint8_t* kept, uint32_t nseed,
                                      double threshold, char** out) {
  return text_out(out, [&]() {
    const std::vector<std::string> nm = strings(n, names);
    if (!block || !kept || nseed > n) throw kBadArgument;
    const std::string text(block);
    const std::string first = "# STOCKHOLM 1.0\n";
    if (text.compare(0, first.size(), first) != 0) throw std::string("stockholm nr: not a Stockholm block");
    std::set<std::string> dropped;  // the labels of the lines that leave: the row's and its "#=GR <name> ..." lines
    uint32_t hits = 0;
    for (uint32_t r = 0; r < n; ++r) {
      if (r >= nseed && kept[r]) ++hits;
      if (!kept[r]) dropped.insert(nm[r]);
    }
    std::string res = first + "#=GF CC nr " + fmt9d(threshold) + " kept " + std::to_string(hits) + " of " + std::to_string(n - nseed) + " hits\n";
    for (size_t at = first.size(); at < text.size();) {
      size_t nl = text.find('\n', at);
      nl = nl == std::string::npos ? text.size() : nl + 1;
      const std::string line = text.substr(at, nl - at);
      at = nl;
      std::vector<std::string> f = fields(line);
      const bool gr = f.size() >= 2 && f[0] == "#=GR";
      if (!f.empty() && (gr ? dropped.count(f[1]) : (f[0][0] != '#' && dropped.count(f[0])))) continue;
      res += line;
    }
    return res;
  });
}

// --pairwise-scores: one line per pair
extern "C" int dafs_host_pairwise_table(uint64_t npairs, const uint32_t* x, const uint32_t* y, uint32_t nnames, const char* const* names,
                                        const double* sim, const double* score, const int64_t* iterations, char** table) {
  return text_out(table, [&]() {
    const std::vector<std::string> nm = strings(nnames, names);
    if (npairs && (!x || !y || !sim || !score || !iterations)) throw kBadArgument;
    std::ostringstream ts;
    for (uint64_t k = 0; k < npairs; ++k) {
      if (x[k] >= nnames || y[k] >= nnames) throw std::string("pairwise table: a pair names a sequence that is not there");
      ts << x[k] + 1 << "\t" << y[k] + 1 << "\t" << nm[x[k]] << "\t" << nm[y[k]] << "\t" << fmt9d(sim[k]) << "\t" << fmt9d(score[k]) << "\t"
         << iterations[k] << "\n";
    }
    return ts.str();
  });
}

// --cluster-table: one line per sequence, named by the Stockholm rule over the file's headers.  A cluster's join is found on
// the tree: the node whose leaves all carry the cluster's label and are as many as the cluster has members.
extern "C" int dafs_host_cluster_table(uint32_t n, const char* const* headers, const uint32_t* length, const uint32_t* labels,
                                       const float* score, const int32_t* left, const int32_t* right, const float* sim, char** table) {
  return text_out(table, [&]() {
    const std::vector<std::string> nm = stockholm_names(strings(n, headers));
    if (!n || !length || !labels || !score || !left || !right || !sim) throw kBadArgument;
    const std::string bad = "cluster table: the clusters are not those of a cut of this tree";
    std::vector<uint32_t> size(n, 0);
    for (uint32_t i = 0; i < n; ++i) {
      if (labels[i] >= n) throw bad;
      ++size[labels[i]];
    }
    const double nan = std::nan("");
    std::vector<double> join(n, nan);
    std::vector<uint8_t> found(n, 0);
    const uint32_t T = 2 * n - 1;
    std::vector<uint32_t> lab(T, DAFS_HIP_NONE), leaves(T, 1);  // per node: the one label of its leaves (or none), their number
    for (uint32_t i = 0; i < T; ++i) {
      if (i < n) {
        lab[i] = labels[i];
      } else {
        if (left[i] < 0 || right[i] < 0 || (uint32_t)left[i] >= i || (uint32_t)right[i] >= i) throw bad;
        leaves[i] = leaves[left[i]] + leaves[right[i]];
        if (lab[left[i]] != DAFS_HIP_NONE && lab[left[i]] == lab[right[i]]) lab[i] = lab[left[i]];
      }
      if (lab[i] != DAFS_HIP_NONE && leaves[i] == size[lab[i]]) {
        found[lab[i]] = 1;
        if (i >= n) join[lab[i]] = score[i];
      }
    }
    std::ostringstream ts;
    for (uint32_t i = 0; i < n; ++i) {
      if (!found[labels[i]]) throw bad;
      uint32_t best[2] = {DAFS_HIP_NONE, DAFS_HIP_NONE};  // inside, outside: the first of the most similar
      for (uint32_t j = 0; j < n; ++j) {
        if (j == i) continue;
        uint32_t& b = best[labels[j] == labels[i] ? 0 : 1];
        if (b == DAFS_HIP_NONE || sim[(size_t)i * n + j] > sim[(size_t)i * n + b]) b = j;
      }
      ts << i + 1 << "\t" << nm[i] << "\t" << length[i] << "\t" << labels[i] + 1 << "\t" << size[labels[i]] << "\t" << fmt9d(join[labels[i]]);
      for (uint32_t b : best) ts << "\t" << (b == DAFS_HIP_NONE ? 0 : b + 1) << "\t" << fmt9d(b == DAFS_HIP_NONE ? nan : (double)sim[(size_t)i * n + b]);
      ts << "\n";
    }
    return ts.str();
  });
}

// --seed-scores: one line per new sequence of a --seed-each run, named by the Stockholm rule over the file's headers; with
// --seed-structure four more columns, the sequence's structure support; with
// --seed-nearest two more: the nearest seed row and the identity to it
extern "C" int dafs_host_seed_table_nearest(uint32_t n, const char* const* headers, const uint32_t* length, const uint32_t* matched,
                                            const double* score, const int64_t* iterations, const uint32_t* both, const uint32_t* canonical,
                                            const uint32_t* half, const double* expected, const char* const* nearest_name,
                                            const double* identity, char** table) {
  return text_out(table, [&]() {
    const bool near = nearest_name || identity;
    if (near && n && (!nearest_name || !identity)) throw kBadArgument;
    const std::vector<std::string> nn = near ? strings(n, nearest_name) : std::vector<std::string>();
    const std::vector<std::string> nm = stockholm_names(strings(n, headers));
    if (n && (!length || !matched || !score || !iterations)) throw kBadArgument;
    const bool support = both || canonical || half || expected;
    if (support && n && (!both || !canonical || !half || !expected)) throw kBadArgument;
    std::ostringstream ts;
    for (uint32_t j = 0; j < n; ++j) {
      if (matched[j] > length[j]) throw std::string("seed table: more matched residues than residues");
      ts << j + 1 << "\t" << nm[j] << "\t" << length[j] << "\t" << matched[j] << "\t" << length[j] - matched[j] << "\t" << fmt9d(score[j]) << "\t"
         << iterations[j];
      if (support) {
        if (canonical[j] > both[j]) throw std::string("seed table: more canonical pairs than pairs");
        ts << "\t" << both[j] << "\t" << canonical[j] << "\t" << half[j] << "\t" << fmt9d(expected[j]);
      }
      if (near) ts << "\t" << nn[j] << "\t" << fmt9d(identity[j]);
      ts << "\n";
    }
    return ts.str();
  });
}

extern "C" int dafs_host_seed_table_support(uint32_t n, const char* const* headers, const uint32_t* length, const uint32_t* matched,
                                            const double* score, const int64_t* iterations, const uint32_t* both, const uint32_t* canonical,
                                            const uint32_t* half, const double* expected, char** table) {
  return dafs_host_seed_table_nearest(n, headers, length, matched, score, iterations, both, canonical, half, expected, nullptr, nullptr, table);
}

extern "C" int dafs_host_seed_table(uint32_t n, const char* const* headers, const uint32_t* length, const uint32_t* matched, const double* score,
                                    const int64_t* iterations, char** table) {
  return dafs_host_seed_table_support(n, headers, length, matched, score, iterations, nullptr, nullptr, nullptr, nullptr, table);
}

extern "C" int dafs_host_seed_parse(const char* text, size_t bytes, uint32_t* n, char** names, char** rows) {
  if (rows) *rows = nullptr;
  const int rc = text_out(names, [&]() {
    if (!n || !rows || (bytes && !text)) throw kBadArgument;
    std::vector<std::string> nm, rw;
    parse_seed(std::string(bytes ? text : "", bytes), nm, rw);
    const std::string names_text = joined(nm);
    *rows = copy_text(joined(rw));
    *n = (uint32_t)nm.size();
    return names_text;
  });
  if (rc != DAFS_HIP_OK && rows) {  // the names' copy failed after the rows'
    free(*rows);
    *rows = nullptr;
  }
  return rc;
}

extern "C" int dafs_host_seed_clean(uint32_t n, const char* const* names, const char* const* rows, char** cleaned) {
  return text_out(cleaned, [&]() {
    const std::vector<std::string> nm = strings(n, names);
    std::vector<std::string> rw = strings(n, rows);
    clean_seed(nm, rw);
    return joined(rw);
  });
}

// the seed with its consensus structure
extern "C" int dafs_host_seed_parse_structure(const char* text, size_t bytes, uint32_t* n, int* has_structure, char** names, char** rows,
                                              char** structure) {
  if (rows) *rows = nullptr;
  if (structure) *structure = nullptr;
  const int rc = text_out(names, [&]() {
    if (!n || !has_structure || !rows || !structure || (bytes && !text)) throw kBadArgument;
    std::vector<std::string> nm, rw;
    std::string st;
    bool has = false;
    parse_seed(std::string(bytes ? text : "", bytes), nm, rw, &st, &has);
    const std::string names_text = joined(nm);
    *rows = copy_text(joined(rw));
    *structure = copy_text(st);
    *n = (uint32_t)nm.size();
    *has_structure = has ? 1 : 0;
    return names_text;
  });
  if (rc != DAFS_HIP_OK) {  // a later copy failed after an earlier one
    if (rows) { free(*rows); *rows = nullptr; }
    if (structure) { free(*structure); *structure = nullptr; }
  }
  return rc;
}

extern "C" int dafs_host_seed_clean_structure(uint32_t n, const char* const* names, const char* const* rows, const char* structure,
                                              uint32_t* ss, uint32_t* columns, char** cleaned) {
  return text_out(cleaned, [&]() {
    if (!structure || !ss || !columns) throw kBadArgument;
    const std::vector<std::string> nm = strings(n, names);
    std::vector<std::string> rw = strings(n, rows);
    const size_t raw = rw.empty() ? 0 : rw[0].size();
    std::vector<size_t> kept;
    clean_seed(nm, rw, &kept);
    const std::string st = structure;
    if (st.size() != raw)
      throw "seed: SS_cons has " + std::to_string(st.size()) + " columns, the rows have " + std::to_string(raw);
    const std::vector<uint32_t> partner = structure_pairs(st);
    std::vector<uint32_t> now(raw, DAFS_HIP_NONE);  // raw column -> cleaned column
    for (size_t k = 0; k < kept.size(); ++k) now[kept[k]] = (uint32_t)k;
    for (size_t k = 0; k < kept.size(); ++k) {
      const uint32_t p = partner[kept[k]];
      // a pair that lost its right column reads NONE here; one that lost its left column is named by nothing any more
      ss[k] = p != DAFS_HIP_NONE && p > kept[k] ? now[p] : DAFS_HIP_NONE;
    }
    *columns = (uint32_t)kept.size();
    return joined(rw);
  });
}

// the seed with a consensus structure whose pairs may cross
extern "C" int dafs_host_seed_clean_structure_levels(uint32_t n, const char* const* names, const char* const* rows, const char* structure,
                                                     uint32_t* ss, uint8_t* level, uint32_t* columns, char** cleaned) {
  return text_out(cleaned, [&]() {
    if (!structure || !ss || !level || !columns) throw kBadArgument;
    const std::vector<std::string> nm = strings(n, names);
    std::vector<std::string> rw = strings(n, rows);
    const size_t raw = rw.empty() ? 0 : rw[0].size();
    std::vector<size_t> kept;
    clean_seed(nm, rw, &kept);
    const std::string st = structure;
    if (st.size() != raw)
      throw "seed: SS_cons has " + std::to_string(st.size()) + " columns, the rows have " + std::to_string(raw);
    std::vector<uint8_t> group_raw;
    const std::vector<uint32_t> partner = structure_pairs_groups(st, group_raw);
    std::vector<uint32_t> now(raw, DAFS_HIP_NONE);  // raw column -> cleaned column
    for (size_t k = 0; k < kept.size(); ++k) now[kept[k]] = (uint32_t)k;
    std::vector<uint32_t> out(kept.size(), DAFS_HIP_NONE);
    std::vector<uint8_t> group(kept.size(), 0xFF);
    for (size_t k = 0; k < kept.size(); ++k) {  // a pair that lost a column is dropped before the levels are assigned
      const uint32_t p = partner[kept[k]];
      if (p == DAFS_HIP_NONE || p < kept[k] || now[p] == DAFS_HIP_NONE) continue;
      out[k] = now[p];
      group[k] = group[now[p]] = group_raw[kept[k]];
    }
    std::vector<uint8_t> lv(kept.size() + 1);
    assign_levels(out, group, lv.data());
    for (size_t k = 0; k < kept.size(); ++k) { ss[k] = out[k]; level[k] = lv[k]; }
    *columns = (uint32_t)kept.size();
    return joined(rw);
  });
}

// The "#=GR <name> PP" lines of a Stockholm file's first alignment, over the columns the seed reader keeps
extern "C" int dafs_host_seed_pp(const char* text, size_t bytes, uint32_t* n, int* has_pp, char** pp) {
  return text_out(pp, [&]() {
    if (!n || !has_pp || (bytes && !text)) throw kBadArgument;
    const std::string all(bytes ? text : "", bytes);
    std::vector<std::string> nm, rw;
    parse_seed(all, nm, rw);
    std::map<std::string, std::string> of;  // name -> its PP characters, the blocks concatenated
    std::istringstream is(all);
    std::string ln;
    bool first = true, stockholm = false;
    size_t line = 0;
    while (std::getline(is, ln)) {
      ++line;
      const size_t e = ln.find_last_not_of(kSpace);
      ln = e == std::string::npos ? std::string() : ln.substr(0, e + 1);
      if (first) {
        stockholm = ln == "# STOCKHOLM 1.0";
        first = false;
      }
      if (!stockholm || ln == "//") break;
      if (ln.compare(0, 4, "#=GR") != 0) continue;
      const std::vector<std::string> f = fields(ln);
      if (f.size() < 3 || f[2] != "PP") continue;
      if (f.size() != 4) throw "seed: line " + std::to_string(line) + " is not '#=GR name PP characters'";
      of[f[1]] += f[3];
    }
    const size_t raw = rw.empty() ? 0 : rw[0].size();
    std::vector<size_t> kept;
    clean_seed(nm, rw, &kept);
    for (const auto& kv : of) {
      if (std::find(nm.begin(), nm.end(), kv.first) == nm.end()) throw "seed: the PP line of " + kv.first + " names no row";
      if (kv.second.size() != raw)
        throw "seed: the PP line of " + kv.first + " has " + std::to_string(kv.second.size()) + " columns, the rows have " + std::to_string(raw);
    }
    std::vector<std::string> out;
    for (const std::string& name : nm) {
      std::string row(kept.size(), '.');
      const auto it = of.find(name);
      if (it != of.end())
        for (size_t k = 0; k < kept.size(); ++k) row[k] = it->second[kept[k]];
      out.push_back(row);
    }
    *n = (uint32_t)nm.size();
    *has_pp = of.empty() ? 0 : 1;
    return joined(out);
  });
}

// Comparing two alignments: the refusals, the row matching and the tables of --compare,
// --compare-columns and --compare-matrix
extern "C" const char* dafs_host_compare_refusal(int which) {
  switch (which) {
    case DAFS_COMPARE_NEEDS_REF:
      return "comparing (--compare OUT, --compare-ref REF) needs both: where the table goes and the reference alignment";
    case DAFS_COMPARE_NEEDS_COMPARE:
      return "--compare-columns and --compare-matrix need --compare";
    case DAFS_COMPARE_NO_PAIRWISE:
      return "comparing (--compare, compare) cannot be combined with pairwise alignments (--pairwise, pipeline.pairwise): a pair of rows is no "
             "alignment of the reference's sequences";
    case DAFS_COMPARE_NEEDS_MERGED:
      return "comparing (--compare, compare) with --seed-each / add_each compares the merged alignment: it needs --seed-merged / merged";
    case DAFS_COMPARE_TOO_MANY_ROWS:
      return "the pair table of a comparison (--compare-matrix) holds the whole matrices: at most 16384 rows";
    default:
      return "";
  }
}

extern "C" int dafs_host_compare_match(uint32_t n_ref, const char* const* ref_names, uint32_t n_test, const char* const* test_names,
                                       uint32_t* count, uint32_t* ref_row, uint32_t* test_row) {
  char* unused = nullptr;
  const int rc = text_out(&unused, [&]() {
    if (!count || !ref_row || !test_row) throw kBadArgument;
    auto first_word = [](std::vector<std::string> v) {  // a Stockholm name: what a row of a Stockholm file is called
      for (std::string& h : v) {
        const std::vector<std::string> f = fields(h);
        h = f.empty() ? std::string() : f[0];
      }
      return v;
    };
    const std::vector<std::string> rn = first_word(strings(n_ref, ref_names)), tn = first_word(strings(n_test, test_names));
    std::map<std::string, uint32_t> at;
    for (uint32_t k = 0; k < n_test; ++k) {
      if (at.count(tn[k])) throw "compare: the name " + tn[k] + " is on two rows of the test alignment";
      at[tn[k]] = k;
    }
    std::set<std::string> seen;
    uint32_t m = 0;
    for (uint32_t k = 0; k < n_ref; ++k) {
      if (!seen.insert(rn[k]).second) throw "compare: the name " + rn[k] + " is on two rows of the reference alignment";
      const auto it = at.find(rn[k]);
      if (it == at.end()) continue;
      ref_row[m] = k;
      test_row[m] = it->second;
      ++m;
    }
    if (m < 2)
      throw "compare: the two alignments share " + std::to_string(m) + " row name" + (m == 1 ? "" : "s") + "; a comparison needs two at least";
    *count = m;
    return std::string();
  });
  free(unused);
  return rc;
}

namespace {
double quotient(uint64_t a, uint64_t b) { return b ? (double)a / (double)b : std::nan(""); }
}  // namespace

extern "C" int dafs_host_compare_table(uint32_t n, const char* const* names, uint32_t only_ref, uint32_t only_test, uint32_t len_r,
                                       uint32_t len_t, const uint32_t* residues, const uint64_t* shared, const uint64_t* refp,
                                       const uint64_t* testp, const uint64_t* total, const uint64_t* tc, const uint64_t* tp,
                                       const uint64_t* nref, const uint64_t* ntest, const uint64_t* pp_count, char** table) {
  return text_out(table, [&]() {
    const std::vector<std::string> nm = strings(n, names);
    if (!n || !residues || !shared || !refp || !testp || !total || !tc || (tp && (!nref || !ntest))) throw kBadArgument;
    std::ostringstream os;
    os << "# rows " << n << " only_ref " << only_ref << " only_test " << only_test << " columns_ref " << len_r << " columns_test " << len_t << "\n";
    os << "# pairs shared " << total[0] << " ref " << total[1] << " test " << total[2] << " sps " << fmt9d(quotient(total[0], total[1])) << " ppv "
       << fmt9d(quotient(total[0], total[2])) << "\n";
    os << "# columns reproduced " << tc[0] << " of " << tc[1] << " tc " << fmt9d(quotient(tc[0], tc[1])) << "\n";
    if (tp) {
      uint64_t t[3] = {0, 0, 0};
      for (uint32_t r = 0; r < n; ++r) { t[0] += tp[r]; t[1] += nref[r]; t[2] += ntest[r]; }
      os << "# structure tp " << t[0] << " ref " << t[1] << " test " << t[2] << " sensitivity " << fmt9d(quotient(t[0], t[1])) << " ppv "
         << fmt9d(quotient(t[0], t[2])) << " f " << fmt9d(quotient(2 * t[0], t[1] + t[2])) << "\n";
    }
    if (pp_count)
      for (uint32_t q = 0; q < 11; ++q)
        if (pp_count[q])
          os << "# pp " << "0123456789*"[q] << " " << pp_count[q] << " " << pp_count[11 + q] << " " << pp_count[22 + q] << " "
             << fmt9d(quotient(pp_count[22 + q], pp_count[11 + q])) << "\n";
    for (uint32_t r = 0; r < n; ++r) {
      os << r + 1 << "\t" << nm[r] << "\t" << residues[r] << "\t" << shared[r] << "\t" << refp[r] << "\t" << testp[r] << "\t"
         << fmt9d(quotient(shared[r], refp[r])) << "\t" << fmt9d(quotient(shared[r], testp[r]));
      if (tp) os << "\t" << tp[r] << "\t" << nref[r] << "\t" << ntest[r];
      os << "\n";
    }
    return os.str();
  });
}

extern "C" int dafs_host_compare_columns_table(uint32_t len_r, const uint32_t* k, const uint64_t* colref, const uint64_t* colshared,
                                               const uint8_t* reproduced, char** table) {
  return text_out(table, [&]() {
    if (!len_r || !k || !colref || !colshared || !reproduced) throw kBadArgument;
    std::ostringstream os;
    for (uint32_t c = 0; c < len_r; ++c)
      os << c + 1 << "\t" << k[c] << "\t" << colref[c] << "\t" << colshared[c] << "\t" << (reproduced[c] ? 1 : 0) << "\n";
    return os.str();
  });
}

extern "C" int dafs_host_compare_matrix_table(uint32_t n, const char* const* names, const uint32_t* pair_shared, const uint32_t* pair_refp,
                                              const uint32_t* pair_testp, char** table) {
  return text_out(table, [&]() {
    const std::vector<std::string> nm = strings(n, names);
    if (!n || !pair_shared || !pair_refp || !pair_testp) throw kBadArgument;
    std::ostringstream os;
    for (uint32_t r = 0; r < n; ++r)
      for (uint32_t s = r + 1; s < n; ++s) {
        const size_t at = (size_t)r * n + s;
        os << r + 1 << "\t" << s + 1 << "\t" << nm[r] << "\t" << nm[s] << "\t" << pair_shared[at] << "\t" << pair_refp[at] << "\t" << pair_testp[at]
           << "\t" << fmt9d(quotient(pair_shared[at], pair_refp[at])) << "\t" << fmt9d(quotient(pair_shared[at], pair_testp[at])) << "\n";
      }
    return os.str();
  });
}

extern "C" int dafs_host_fold_complementary(char a, char b) {
  const int x = fold_symbol(a), y = fold_symbol(b);
  return ((x == 0 && y == 3) || (x == 3 && y == 0) || (x == 2 && y == 3) || (x == 3 && y == 2) || (x == 1 && y == 2) || (x == 2 && y == 1)) ? 1 : 0;
}

extern "C" int dafs_host_row_constraint(uint32_t len, const uint8_t* mask_row, const uint32_t* ss, const char* residues, char* out) {
  if ((len && (!mask_row || !ss)) || !residues || !out) return DAFS_HIP_EINVAL;
  std::vector<uint32_t> rev(len);
  uint32_t k = 0;
  for (uint32_t c = 0; c < len; ++c) rev[c] = mask_row[c] ? k++ : DAFS_HIP_NONE;
  if (strnlen(residues, (size_t)k + 1) != k) return DAFS_HIP_EINVAL;
  for (uint32_t c = 0; c < len; ++c)
    if (ss[c] != DAFS_HIP_NONE && (ss[c] <= c || ss[c] >= len)) return DAFS_HIP_EINVAL;
  memset(out, '?', k);
  out[k] = 0;
  for (uint32_t c = 0; c < len; ++c) {
    if (ss[c] == DAFS_HIP_NONE) continue;
    const uint32_t i = rev[c], j = rev[ss[c]];
    if (i == DAFS_HIP_NONE || j == DAFS_HIP_NONE) continue;
    if (j - i < 4 || !dafs_host_fold_complementary(residues[i], residues[j])) continue;
    out[i] = '(';
    out[j] = ')';
  }
  return DAFS_HIP_OK;
}

// One constraint per level (DAFS::update_basepairing_probability, dafs.cpp:635-653): string k at
// out + k * (residues + 1).
extern "C" int dafs_host_row_constraint_levels(uint32_t len, const uint8_t* mask_row, const uint32_t* ss, const uint8_t* level, uint32_t nlevels,
                                               const char* residues, char* out) {
  if ((len && (!mask_row || !ss)) || !residues || !out || nlevels < 1 || nlevels > DAFS_HIP_MAX_LEVELS) return DAFS_HIP_EINVAL;
  std::vector<uint32_t> rev(len);
  uint32_t k = 0;
  for (uint32_t c = 0; c < len; ++c) rev[c] = mask_row[c] ? k++ : DAFS_HIP_NONE;
  if (strnlen(residues, (size_t)k + 1) != k) return DAFS_HIP_EINVAL;
  for (uint32_t c = 0; c < len; ++c) {
    if (ss[c] == DAFS_HIP_NONE) continue;
    if (ss[c] <= c || ss[c] >= len) return DAFS_HIP_EINVAL;
    if (level && (level[c] >= nlevels || level[ss[c]] != level[c])) return DAFS_HIP_EINVAL;
  }
  const size_t stride = (size_t)k + 1;
  for (uint32_t lv = 0; lv < nlevels; ++lv) {
    char* o = out + lv * stride;
    memset(o, '?', k);
    o[k] = 0;
    bool forced = false;
    for (uint32_t c = 0; c < len; ++c) {
      if (ss[c] == DAFS_HIP_NONE) continue;
      const uint32_t i = rev[c], j = rev[ss[c]];
      if (i == DAFS_HIP_NONE || j == DAFS_HIP_NONE) continue;
      if ((level ? level[c] : 0) != lv) {  // a pair of another level: both residues unpaired in this fold (dafs.cpp:650)
        o[i] = o[j] = '.';
        continue;
      }
      if (j - i < 4 || !dafs_host_fold_complementary(residues[i], residues[j])) continue;
      o[i] = '(';
      o[j] = ')';
      forced = true;
    }
    if (lv >= 1 && !forced) o[0] = 0;  // nothing to force at this level: the row is not folded for it
  }
  return DAFS_HIP_OK;
}

// ---------------------------------------------------------------------------------------------
// Device memory one family takes in phase 1, estimated from the stores' sizes (bytes): per pair its row pointers in both
// matching stores, its entries (as the pair kernels reserve them: 24 per shorter-sequence column and direction, col + val,
// the relaxed copy and the interleaved copy of the transforms) and its dense consistency tile; per sequence its base-pairing
// tile and rows; the similarity block.  Not counted: the folding kernels' workspaces and the resident nodes of the
// progressive phase, which hold only the open nodes (tools/time_batch.py reports their measured peak).
extern "C" uint64_t dafs_host_family_bytes(uint32_t n, const uint32_t* lens) {
  if (n && !lens) return 0;
  uint64_t b = 4 * (uint64_t)n * n;
  for (uint32_t x = 0; x < n; ++x) {
    const uint64_t lx = lens[x];
    b += 8 * lx * lx + 64 * lx + 4096;
    for (uint32_t y = x + 1; y < n; ++y) {
      const uint64_t ly = lens[y];
      b += 8 * (lx + ly + 2) + 2 * std::min(lx, ly) * 24 * 32 + 4 * lx * ly;
    }
  }
  return b;
}

// Device memory of one resident node of l1 x l2 columns (bytes), the bound capi_dd.cpp's nodes_open keeps, folding arrays
// included: per cell of the two base-pairing matrices 19 + 25 bytes, per cell of the alignment tables 26 bytes plus the
// padded sweep-order copies, traceback slots, row arrays and slack.
extern "C" uint64_t dafs_host_node_bytes(uint32_t len1, uint32_t len2) {
  const uint64_t l1 = len1, l2 = len2;
  return 44 * (l1 * l1 + l2 * l2) + 26 * (l1 + 1) * (l2 + 1) + 8 * (l1 + 63) * (l2 + 64) + 512 * (l1 + 1) * ((l2 + 2048) / 2048) + 128 * (l1 + l2) +
         (1 << 14);
}

// Device memory of one new sequence of a --seed-each run: the phase-1 stores of its family, the m seed
// sequences and itself, and its one node, the leaf against the seed's `seed_columns` columns, resident for the whole progressive
// phase of its chunk.
extern "C" uint64_t dafs_host_seed_each_bytes(uint32_t m, const uint32_t* seed_lens, uint32_t seed_columns, uint32_t new_len) {
  if (m && !seed_lens) return 0;
  std::vector<uint32_t> lens(seed_lens, seed_lens + m);
  lens.push_back(new_len);
  return dafs_host_family_bytes(m + 1, lens.data()) + dafs_host_node_bytes(new_len, seed_columns);
}

// per sub-batch or chunk, against the 288 GB of an MI355X.  A choice, not a measured limit.  Measured on 512 families of
// 5-15 sequences of 80-200 nt (profiles/r04_a_time_batch.json): phase-1 estimate 8.6 GB (one sub-batch), peak of the
// progressive phase's resident nodes 6.0 GB, which dafs_host_family_bytes does not count.
extern "C" uint64_t dafs_host_batch_bytes(void) { return 16ull << 30; }

// Device memory of one alignment of n_rows rows and len columns inside dafs_hip_consensus_structures (bytes), a bound that its
// carving checks for every chunk (capi_dd.cpp): the averaged matrix and the four tables of carve_nuss, 20 bytes a cell; the
// rows' ranks and residue columns, 8 bytes per row and column; the structure, the candidate counters and stack (16 bytes a
// column), the row arrays; then the constant part: the node and decoder descriptors and the score (644 bytes), the arrays'
// tails (88), and the 256-byte alignment of the alignment's eleven arrays and of a chunk's three shared ones plus its slack,
// which an alignment alone in its chunk carries all (under 3 900 bytes together).
extern "C" uint64_t dafs_host_structure_bytes(uint32_t n_rows, uint32_t len) {
  const uint64_t n = n_rows, l = len;
  return 20 * l * l + 8 * n * l + 24 * l + 8 * n + 16 * 256 + 1024;
}

// The same alignment inside dafs_hip_consensus_structures_levels.  On top: the level's own structure and
// the column keys (8 bytes a column) and the level bytes (1); the alignment's level descriptor, its per-level decoder
// descriptor and index, four flags and three more scores (under 200 bytes); the 256-byte alignment of its three more arrays
// and of a chunk's three more shared ones.
extern "C" uint64_t dafs_host_structure_levels_bytes(uint32_t n_rows, uint32_t len) {
  return dafs_host_structure_bytes(n_rows, len) + 12 * (uint64_t)len + 8 * 256 + 512;
}

// The same alignment inside dafs_hip_consensus_structures_auto with ncand candidates.  On top, per
// candidate: its structure (4 bytes a column and one entry more), its score, its decoder descriptor (72 bytes) and its row
// of the table at four levels (48), under 160 bytes together; the alignment's descriptor, S, the running sums, and the
// chosen candidates, T and n of four levels (under 300 bytes); the 256-byte alignment of its one more array and of a
// chunk's nine more shared ones.
extern "C" uint64_t dafs_host_structure_auto_bytes(uint32_t n_rows, uint32_t len, uint32_t ncand) {
  return dafs_host_structure_levels_bytes(n_rows, len) + (uint64_t)ncand * (4 * (uint64_t)len + 160) + 12 * 256 + 512;
}

// per chunk of dafs_hip_consensus_structures.  A choice, not a limit: 2 GiB hold some 3 500 pair alignments of 170 columns,
// a dozen times what the device keeps resident at once, and the buffer stays with the context.
extern "C" uint64_t dafs_host_structures_batch_bytes(void) { return 2ull << 30; }

// Device memory of one alignment of n_rows rows and len columns inside dafs_hip_alignment_reliabilities (bytes), a bound that its
// carving checks for every chunk (capi_reliability.cpp).  Per cell the mask byte, the column -> residue map and, for at most as
// many residues, the residue -> column map and the value (17 bytes) and the residue blocks' share (1/8); per row its descriptor
// and its last residue block (40); per column the structure, the three column outputs and the column blocks' share (under 25);
// the alignment's descriptor and last column block (48); then the 256-byte alignment of a chunk's twelve arrays plus its slack,
// which an alignment alone in its chunk carries all (under 3 400 bytes).
extern "C" uint64_t dafs_host_reliability_bytes(uint32_t n_rows, uint32_t len) {
  const uint64_t n = n_rows, l = len;
  return 18 * n * l + 40 * n + 25 * l + 64 + 4096;
}

// per chunk of dafs_hip_alignment_reliabilities.  A choice, not a limit: 1 GiB holds some 100 000 pair alignments of 170
// columns or 1 500 alignments of 33 rows and 1 000 columns, and the buffer stays with the context.
extern "C" uint64_t dafs_host_reliability_batch_bytes(void) { return 1ull << 30; }

// greedy, in input order: a group is closed before the item that would take it over max_bytes; an item over the budget
// is a group of its own
extern "C" int dafs_host_pack_greedy(uint32_t n, const uint64_t* sizes, uint64_t max_bytes, uint32_t* group_of) {
  if (n && (!sizes || !group_of)) return DAFS_HIP_EINVAL;
  uint32_t group = 0;
  uint64_t used = 0;
  for (uint32_t k = 0; k < n; ++k) {
    if (k && (used > max_bytes || sizes[k] > max_bytes - used)) {  // used + sizes[k] > max_bytes, without the overflow
      ++group;
      used = 0;
    }
    group_of[k] = group;
    used += sizes[k];
  }
  return DAFS_HIP_OK;
}

// The ranges of dafs_hip_similarity: dafs_host_pack_greedy's rule over the row-major pairs, each at the
// size dafs_hip_align_posteriors gives it before the launch -- 2 * min(len) * 24 entries of a 4-byte column and a 4-byte value,
// and its row pointers in both directions.  The launch's scratch planes belong to the launch, not to a pair, and are left out.
extern "C" int dafs_host_similarity_ranges(uint32_t n, const uint32_t* lens, uint64_t max_bytes, uint64_t* end, uint64_t cap,
                                           uint64_t* n_ranges) {
  if (!n_ranges || (n && !lens) || (cap && !end)) return DAFS_HIP_EINVAL;
  if (max_bytes == 0) max_bytes = dafs_host_batch_bytes();
  uint64_t ranges = 0, used = 0, held = 0, p = 0;
  for (uint32_t x = 0; x < n; ++x)
    for (uint32_t y = x + 1; y < n; ++y, ++p) {
      const uint64_t lx = lens[x], ly = lens[y];
      const uint64_t bytes = 2 * std::min(lx, ly) * 24 * 8 + 4 * (lx + ly + 2);
      if (held && (used > max_bytes || bytes > max_bytes - used || held == 0xFFFFFFFFull)) {  // close the range in front of this pair
        if (ranges < cap) end[ranges] = p;
        ++ranges;
        used = held = 0;
      }
      used += bytes;
      ++held;
    }
  if (held) {
    if (ranges < cap) end[ranges] = p;
    ++ranges;
  }
  *n_ranges = ranges;
  return DAFS_HIP_OK;
}
