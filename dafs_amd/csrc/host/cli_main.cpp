// dafs_amd/csrc/host/cli_main.cpp -- the `dafs [OPTIONS] FASTA` command line on top of libdafs_hip.so.
//
// Same flags, defaults and output format as the reference program (reference src/dafs.cpp:1603-1779
// for the options, :1781-1889 for the run, :495-511 and :1584-1601 for the output), with every
// numeric stage executed on the GPU through the C ABI: base-pairing posteriors, all-pairs matching
// posteriors, similarity, both consistency transforms, and per guide-tree node the averaging +
// dual-decomposition solve.  The host keeps what is inherently serial and tiny: option parsing,
// the guide tree, the alignment bookkeeping (project_alignment) and printing.  The guide tree, the Stockholm block, the
// --covariation and --pairwise-scores tables, the seed reader and the memory estimates are host code of the library
// (host_tree.cpp, host_text.cpp), shared with the Python driver.
//
// Differences from the reference, all forced by what its tree does not contain:
//   -s Boltzmann / -s Vienna and the RNAalifold term need ViennaRNA arithmetic: not available.
//      The default fold model here is CONTRAfold; asking for the others is an error.
//   --fold-decoder IPknot / --ipknot / -m 0 need an ILP solver: not available.  --fold-decoder Levels decodes a structure
//   with pseudoknots level by level instead, one level per entry of -T / -G.
// One addition: --devices a,b,... runs phase 1 (:1787-1827) as one process per listed GPU (dafs_hip_phase1_sharded, the
// shards all-gathered by RCCL); the processes are forked before anything touches a GPU, and the first one goes on alone.
#include <dlfcn.h>
#include <pthread.h>
#include <signal.h>
#include <sys/mman.h>
#include <sys/prctl.h>
#include <sys/wait.h>
#include <unistd.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <iostream>
#include <map>
#include <queue>
#include <sstream>
#include <string>
#include <system_error>
#include <vector>

#ifndef __HIP_PLATFORM_AMD__
#define __HIP_PLATFORM_AMD__ 1
#endif
#include <hip/hip_runtime_api.h>
#include <rccl/rccl.h>  // types and prototypes only: librccl is loaded when --devices asks for it (dlopen)

#include "../../../include/dafs_hip.h"
#include "types.h"

#define DAFS_VERSION "0.0.4-hip"
static const float kCutoff = 0.01f;  // reference CUTOFF (src/dafs.cpp:65)

namespace {

void check(int rc) {
  if (rc != DAFS_HIP_OK) throw dafs_hip_strerror(rc);
}

struct Options {
  int refinement = 0;
  float w = 4.0f, eta = 0.5f;
  int max_iter = 600;
  float fourway = 0.0f;
  int verbose = 0;
  std::string align_model = "ProbCons";
  float align_pct = 0.25f, align_th = 0.01f;
  std::string align_aux, fold_aux, save_align_aux, save_fold_aux;
  std::string fold_model = "CONTRAfold";
  bool fold_model_given = false;
  std::string fold_decoder = "Nussinov";
  float fold_pct = 0.25f;
  std::vector<float> fold_th{0.2f}, fold_th1;
  // -T auto / -G auto: the levels whose thresholds are chosen (0: the thresholds are given), the
  // candidates' weights (--auto-gammas) and thresholds 1 / (1 + gamma), and --fold-auto-table OUT
  uint32_t auto_levels = 0;
  std::vector<float> auto_gammas{1.0f, 2.0f, 4.0f, 8.0f, 16.0f, 32.0f}, auto_cand;
  std::string auto_table;
  bool no_alifold = false, ipknot = false, bp_update = false, bp_update1 = false;
  int device = 0;
  std::vector<int> devices;  // --devices: one process per entry for phase 1
  std::string stockholm;  // --stockholm FILE
  bool row_structures = false;  // --row-structures: a #=GR SS line per row of the Stockholm blocks
  std::string seed;       // --seed SEED: add FILE's sequences to this alignment
  bool seed_each = false;       // --seed-each: with --seed, every sequence of FILE added on its own
  std::string seed_scores;      // --seed-scores OUT
  std::string seed_merged;      // --seed-merged OUT: with --seed-each and --seed-structure, all placements in one Stockholm block
  bool seed_structure = false;  // --seed-structure: with --seed, the seed's SS_cons is fixed like its columns
  bool knots = false;           // --knots: the structures that are read may cross
  bool pairwise = false;  // --pairwise: every pair of FILE's sequences aligned as a two-sequence run
  std::string pairwise_scores;  // --pairwise-scores OUT
  std::string covariation;      // --covariation OUT
  uint32_t cov_shuffles = 100;  // --cov-shuffles K
  uint64_t cov_seed = 1;        // --cov-seed S
  bool cov_shuffles_given = false, cov_seed_given = false;
  int cov_null = DAFS_COV_NULL_SHUFFLE;  // --cov-null NAME
  bool cov_null_given = false;
  bool refinement_given = false;
  std::string identity;         // --identity OUT
  std::string identity_matrix;  // --identity-matrix OUT
  std::string phylogeny;        // --phylogeny OUT: the neighbour-joining tree of every printed alignment's rows, in Newick
  int phylogeny_model = DAFS_NJ_JC;  // --phylogeny-model jc|p
  bool phylogeny_model_given = false;
  uint32_t phylogeny_bootstrap = 0;  // --phylogeny-bootstrap B: replicates behind the support values of the tree (0: none)
  uint64_t phylogeny_seed = 12345;   // --phylogeny-seed S
  std::string phylogeny_support;     // --phylogeny-support OUT: the table of the splits
  bool phylogeny_bootstrap_given = false, phylogeny_seed_given = false;
  bool phylogeny_transfer = false;  // --phylogeny-transfer: the labels and the table show the transfer bootstrap
  bool cov_tree_nj = false;     // --cov-tree nj: the tree null evolves along the neighbour-joining tree
  bool cov_tree_given = false;
  bool seed_nearest = false;    // --seed-nearest: two more columns in --seed-scores
  double seed_nr = 0.0;         // --seed-nr T: --seed-merged holds the non-redundant block
  bool seed_nr_given = false;
  std::string describe;         // --describe ALIGNMENT: the alignment-only statistics of a finished alignment
  std::string compare;          // --compare OUT: every printed alignment against the reference
  std::string compare_ref;      // --compare-ref REF
  std::string compare_columns;  // --compare-columns OUT
  std::string compare_matrix;   // --compare-matrix OUT
  bool cluster_given = false;         // --cluster T: the one FILE cut into clusters at threshold T, each aligned
  double cluster = 0.0;
  bool cluster_count_given = false;   // --cluster-count K: the same cut into exactly K clusters
  uint32_t cluster_count = 0;
  bool cluster_min_size_given = false;
  uint32_t cluster_min_size = 1;      // --cluster-min-size M
  std::string cluster_table;          // --cluster-table OUT
  std::string cluster_tree;           // --cluster-tree OUT
  bool cluster_linkage_given = false;
  int cluster_linkage = 0;            // --cluster-linkage RULE: 0 the guide tree's own rule, else DAFS_LINKAGE_*
  bool cluster_score_given = false;
  int cluster_score = DAFS_SCORE_SEQUENCE;  // --cluster-score NAME
  bool cluster_weight_given = false;
  float cluster_weight = 0.5f;        // --cluster-structure-weight W
  std::string input;
  std::vector<std::string> inputs;  // every FILE argument; with two or more, one output block per file
};

const char* kHelp =
    "DAFS: dual decomposition for simultaneous aligning and folding RNA sequences (MI355X build).\n"
    "Usage:\n  dafs [OPTION...] FILE [FILE ...]\n"
    "  With several files every file is aligned as it would be alone; stdout holds one block per file, in argument\n"
    "  order: a line \"==> FILE <==\" and then that file's output.\n\n"
    "  -h, --help            Print usage\n"
    "      --version         Print version\n"
    "  -r, --refinement N    The number of iteration of the iterative refinment (default: 0)\n"
    "  -w, --weight arg      Weight of the expected accuracy score for secondary structures (default: 4.0)\n"
    "      --eta arg         Initial step width for the subgradient optimization (default: 0.5)\n"
    "  -m, --max-iter T      The maximum number of iteration of the subgradient optimization (default: 600)\n"
    "  -f, --fourway-pct arg Weight of four-way PCT (default: 0.0)\n"
    "  -v, --verbose arg     The level of verbose outputs (default: 0)\n"
    "      --device N        HIP device index (default: 0)\n"
    "      --devices A,B,... One process per listed HIP device for the posteriors and the consistency transform\n"
    "                        (shards exchanged over RCCL); the progressive alignment runs on the first\n"
    "      --stockholm FILE  Also write every printed alignment to FILE in Stockholm format, one block per input\n"
    "                        file, with per-residue (#=GR PP) and per-column (#=GC PP_cons) reliabilities\n"
    "      --row-structures  With --stockholm: after every row's #=GR PP line a #=GR SS line, the structure of that row alone\n"
    "                        (its own base-pairing probabilities after the consistency transform, decoded at the threshold\n"
    "                        of SS_cons), in the row's columns\n"
    "      --seed SEED       Add the sequences of the one FILE to the alignment SEED (Stockholm, or aligned FASTA\n"
    "                        as dafs prints it) without changing its columns; the output has no tree line, and\n"
    "                        --stockholm adds a #=GC RF line (x: seed column).  Not with -r, --bp-update, --devices,\n"
    "                        --align-aux, --fold-aux or --save-*-aux\n"
    "      --seed-each       With --seed: add every sequence of FILE on its own, as if it were the only one in FILE, from one\n"
    "                        shared computation of the posteriors: per sequence a line \"==> j <==\" (1-based, file order) and\n"
    "                        then what dafs --seed SEED prints for a file of that sequence alone; --stockholm writes one block\n"
    "                        per sequence.  Without it the new sequences of FILE inform one another\n"
    "      --seed-scores OUT With --seed-each: a tab-separated table, one line per new sequence:\n"
    "                        j name length matched inserted score iterations (residues in seed columns and in columns of\n"
    "                        their own; the objective and iterations of the sequence's node)\n"
    "                        With --seed-structure four more columns: pairs canonical half expected\n"
    "      --seed-merged OUT With --seed-each and --seed-structure: also write all placements as one alignment to OUT, one\n"
    "                        Stockholm block: the seed rows, then the new rows in file order, each placed as --seed-each places\n"
    "                        it; an insert block as wide as the widest insert there, new rows left-justified in it; #=GR PP for\n"
    "                        the new rows (each from its own placement), SS_cons the seed's, and a #=GC RF line.  OUT can be\n"
    "                        read again as a SEED\n"
    "      --seed-structure  With --seed (and --seed-each): the seed's consensus structure -- the #=GC SS_cons lines of a\n"
    "                        Stockholm seed, the SS_cons record of an aligned-FASTA seed -- is fixed like its columns: the seed\n"
    "                        rows are folded under it, nothing is decoded, and the printed SS_cons is the seed's with '.' at\n"
    "                        insert columns.  Not with --bp-update1, -T or -G\n"
    "      --knots           With --seed, --describe or --compare-ref: the structures that are read may cross.  Groups, in\n"
    "                        this order: () [] {} <>, then the letters A..Z (upper case opens, the same letter in lower case\n"
    "                        closes, as Rfam marks pseudoknots); each group is matched with itself, and group after group goes\n"
    "                        to the lowest of four levels at which it crosses no pair already there.  With --seed-structure\n"
    "                        every seed row is folded once per level, that level's pairs forced and the other levels' pairs\n"
    "                        unpaired, and a cell keeps the largest of its values; SS_cons prints () [] {} <> for levels 0..3.\n"
    "                        --describe prints \">SS_cons\" and the structure it read that way.  Without --knots such\n"
    "                        structures are refused and letters are unpaired\n"
    "      --pairwise        Align every pair of the one FILE's sequences (at least two) as two-sequence runs, the pairs\n"
    "                        in row-major order: per pair a line \"==> i j <==\" (1-based input indices) and then what\n"
    "                        dafs prints for a file of those two sequences; --stockholm writes one block per pair.\n"
    "                        Not with -r, --seed, --devices, --align-aux, --fold-aux or --save-*-aux\n"
    "      --pairwise-scores OUT  With --pairwise: a tab-separated table, one line per pair:\n"
    "                        i j name_i name_j similarity score iterations (the root node's objective and iterations)\n"
    "      --covariation OUT Also write the covariation statistics of every printed alignment to OUT, one tab-separated\n"
    "                        line per column pair: c1 c2 kind S E rows canonical types (columns 1-based; S: the G statistic\n"
    "                        with average-product correction, in nats; E: expected number of column pairs that reach S in\n"
    "                        column-shuffled alignments, a null that ignores phylogeny).  First the pairs of SS_cons (kind\n"
    "                        ss), then each column's best partner where it is no such pair and E <= 0.05 (kind other).\n"
    "                        With --stockholm a #=GC cov_SS_cons line marks the pairs with E <= 0.05.  Not with --pairwise\n"
    "      --cov-shuffles K  Shuffled alignments behind E (default: 100; 0: no E-values); needs --covariation\n"
    "      --cov-seed S      Seed of the shuffles (default: 1); needs --covariation\n"
    "      --cov-null NAME   The null behind E.  shuffle (default): every column permuted on its own, which ignores phylogeny.\n"
    "                        tree: the substitutions of every branch of a tree over the rows (average linkage of their\n"
    "                        identities), moved to other columns; K and S as above.  Needs --covariation\n"
    "      --cov-tree NAME   With --cov-null tree: the tree over the rows.  average (default): average linkage of their identities,\n"
    "                        which assumes a molecular clock.  nj: the neighbour-joining tree of --phylogeny (model jc), which does\n"
    "                        not; at most 16384 rows\n"
    "      --phylogeny OUT   Also write the neighbour-joining tree of every printed alignment's rows to OUT, one Newick line per\n"
    "                        alignment: \"(L:len,R:len)\" nested, the names those of --stockholm, lengths as %.9g (negative ones\n"
    "                        are kept), the root in the middle of the last edge joined; one row gives \"name;\".  The distances\n"
    "                        come from the identity counts of the rows (a letter outside ACGU counts as a difference); the\n"
    "                        joins run on the device.  At most 16384 rows.  Not with --pairwise or --seed-each\n"
    "      --phylogeny-model M  With --phylogeny: jc (default): Jukes-Cantor distances, capped at 3.0; p: the share of aligned\n"
    "                        columns that differ\n"
    "      --phylogeny-bootstrap B  With --phylogeny: B (1 to 65536) bootstrap replicates of every alignment, their columns drawn\n"
    "                        with replacement, their trees joined on the device; every join of the Newick line whose split has\n"
    "                        two rows or more on both sides then carries the share of the replicate trees that hold the split,\n"
    "                        in percent, as its label: \"(A:0.1,B:0.2)87:0.05\"\n"
    "      --phylogeny-seed S  Seed of the replicates (default: 12345); needs --phylogeny-bootstrap\n"
    "      --phylogeny-support OUT  With --phylogeny-bootstrap: also write the table of the splits to OUT, laid out as --phylogeny\n"
    "                        lays out its lines: \"# rows n replicates B seed S model M\", then per split, tab-separated:\n"
    "                        node support B percent size leaves (the rows on the side without the first row)\n"
    "      --phylogeny-transfer  With --phylogeny-bootstrap: the labels are the transfer bootstrap expectation in percent (how\n"
    "                        few rows would have to move for the replicate trees to hold the split) instead of the share of the\n"
    "                        replicate trees that hold it exactly, the table's header ends in \"measure transfer\" and every line\n"
    "                        gains depth transfer tbe\n"
    "      --identity OUT    Also write how similar the rows of every printed alignment are to OUT: the line\n"
    "                        \"# rows n columns len average A min B max C\" (pairwise identity over all row pairs), then one\n"
    "                        tab-separated line per row: r name residues weight nearest nearest_name pid (1-based rows; residues:\n"
    "                        cells that hold a letter; weight: position-based sequence weight; nearest: the most identical other\n"
    "                        row; pid: identical columns / the shorter of the two rows' residue counts).  With --stockholm the\n"
    "                        blocks gain #=GS <name> WT lines.  At most 32768 rows (the summary reads the whole identity\n"
    "                        matrix).  Not with --pairwise or --seed-each\n"
    "      --identity-matrix OUT  With --identity: one tab-separated line per row pair:\n"
    "                        r s name_r name_s identical aligned residues pid\n"
    "      --seed-nearest    With --seed-each and --seed-scores: two more columns at the end of the table, the seed row most\n"
    "                        identical to the new sequence in the seed's columns of its own placement, and that identity\n"
    "      --seed-nr T       With --seed-merged: OUT holds the non-redundant rows only: the seed rows, then, by descending score,\n"
    "                        every new row that is less than T (0 < T <= 1) identical, in the seed's columns, to every row kept\n"
    "                        before it; a line \"#=GF CC nr T kept K of M hits\" precedes the rows\n"
    "      --describe ALIGNMENT  No FILE: read a finished alignment (Stockholm or aligned FASTA, as --seed reads it, with its\n"
    "                        SS_cons if it has one) and write --identity / --identity-matrix and, if given, --covariation for\n"
    "                        it (--identity: at most 32768 rows); nothing is aligned and nothing is printed.  Only --device,\n"
    "                        the --phylogeny*, --cov-* and --compare* options go with it\n"
    "      --compare OUT     With --compare-ref REF: also write to OUT how far every printed alignment agrees with the\n"
    "                        reference alignment REF of the same sequences (read as --seed reads a seed, with its SS_cons if it\n"
    "                        has one).  The rows compared are the names in both.  Lines \"# rows ..\", \"# pairs shared S ref P\n"
    "                        test Q sps A ppv B\" (aligned residue pairs in both / in REF / in the alignment), \"# columns\n"
    "                        reproduced K of M tc C\", \"# structure ..\" when both have a structure, \"# pp class residues ref\n"
    "                        shared accuracy\" per PP class when the alignment has PP values (--describe of a Stockholm file with\n"
    "                        PP lines, --seed-merged), then per row: r name residues shared ref test sps ppv [tp nref ntest].\n"
    "                        With --seed-each it needs --seed-merged and compares the merged alignment in the seed's columns.\n"
    "                        Not with --pairwise\n"
    "      --compare-ref REF The reference alignment of --compare\n"
    "      --compare-columns OUT  With --compare: per column of REF: c residues pairs shared_pairs reproduced\n"
    "      --compare-matrix OUT   With --compare: per row pair: r s name_r name_s shared ref test sps ppv (at most 16384 rows)\n"
    "      --cluster T       The one FILE holds sequences of mixed origin: cluster them and align every cluster.  The similarity\n"
    "                        scores of all pairs (the alignment model's, with -a and -u) give the guide tree of the whole set; a\n"
    "                        join is kept when its score is >= T and every join below it is kept, and a cluster is the leaves of a\n"
    "                        maximal kept join, or a single sequence.  Clusters are numbered by their first member and keep the\n"
    "                        file's order.  Per cluster a line \"==> cluster c <==\" (1-based) and then what dafs prints for a file\n"
    "                        of that cluster's sequences; --stockholm, --covariation and --identity write one block or table per\n"
    "                        printed cluster.  With -f the clustering still reads the raw scores; -f acts inside each cluster's\n"
    "                        run.  Not with --seed*, --pairwise*, --describe, --devices, --compare*, --align-aux, --fold-aux or\n"
    "                        --save-*-aux\n"
    "      --cluster-count K Instead of --cluster T: exactly K clusters (1 <= K <= sequences in FILE), the joins made last undone\n"
    "      --cluster-min-size M  With --cluster or --cluster-count: clusters of fewer than M sequences are listed in the table\n"
    "                        but not aligned or printed (default: 1)\n"
    "      --cluster-table OUT  With --cluster or --cluster-count: a tab-separated table, one line per sequence:\n"
    "                        i name length cluster size join nearest_in sim_in nearest_out sim_out (join: the score of the\n"
    "                        cluster's top join; the most similar sequence inside and outside the cluster; 0 and nan for none)\n"
    "      --cluster-tree OUT   With --cluster or --cluster-count: the guide tree of the whole set, as dafs prints a tree line;\n"
    "                        its join scores are the values T chooses between\n"
    "      --cluster-linkage RULE  With --cluster or --cluster-count: the tree that is cut.  guide (default): the guide tree of\n"
    "                        the whole set; single, complete, average: that linkage of the similarity scores, joined on the\n"
    "                        device (a join scores the largest, the smallest or the size-weighted mean similarity between its\n"
    "                        two clusters).  --cluster-tree writes the tree that was cut\n"
    "      --cluster-score NAME  With --cluster or --cluster-count: the pair score that is clustered on.  sequence (default): the\n"
    "                        alignment model's similarity score; structure: the structural pair score, the base-pairing\n"
    "                        probabilities of both sequences (CONTRAfold, all sequences folded first) matched through the pair's\n"
    "                        matching probabilities, 0 .. 1; mix: sequence + W * (structure - sequence).  The table and the tree\n"
    "                        carry the chosen score; it works with every --cluster-linkage\n"
    "      --cluster-structure-weight W  With --cluster-score mix: the weight W of the structural score, 0 .. 1 (default: 0.5)\n"
    "\n Aligning options:\n"
    "  -a, --align-model arg Alignment model (value=CONTRAlign, ProbCons) (default: ProbCons)\n"
    "  -p, --align-pct arg   Weight of PCT for matching probabilities (default: 0.25)\n"
    "  -u, --align-th arg    Threshold for matching probabilities (default: 0.01)\n"
    "      --save-align-aux FILENAME  Write matching probability matrices in the --align-aux format\n"
    "\n Folding options:\n"
    "  -s, --fold-model arg  Folding model (value=CONTRAfold; Boltzmann and Vienna need ViennaRNA and are\n"
    "                        not available in this build) (default: CONTRAfold)\n"
    "      --fold-decoder arg Decoder for common secondary structure prediction (value=Nussinov, Levels) (default: Nussinov)\n"
    "                        Levels: a structure that may hold pseudoknots, decoded level by level, one level per entry of\n"
    "                        -T / -G (else of -t / -g), at most four: level 0 is the Nussinov decode at the first entry, level k\n"
    "                        the same decoder at entry k over the cells whose columns are still free and that cross a pair of\n"
    "                        every lower level.  Printed as () [] {} <>, in SS_cons and with --row-structures.  Each level is one\n"
    "                        of IPknot's given the lower ones, without its stacking constraints: not IPknot's optimum.  Not with\n"
    "                        --bp-update1 or --seed-structure.  The readers of --seed, --describe and --compare-ref take\n"
    "                        structures whose bracket kinds cross with --knots, so this output can be a seed again.\n"
    "                        With Nussinov only the first entry of -T / -G is used.  IPknot needs an ILP solver: not built.\n"
    "  -q, --fold-pct arg    Weight of PCT for base-pairing probabilities (default: 0.25)\n"
    "  -t, --fold-th arg     Threshold for base-pairing probabilities (default: 0.2)\n"
    "  -g, --gamma arg       Specify the threshold for base-pairing probabilities by 1/(gamma+1)\n"
    "      --no-alifold      No use of RNAalifold (always the case in this build)\n"
    "  -T, --fold-th1 arg    Threshold for base-pairing probabilities of the conclusive common secondary structures\n"
    "  -G, --gamma1 arg      ... specified by 1/(gamma+1)\n"
    "                        -T auto / -G auto: the threshold is chosen among the candidates 1/(gamma+1) of --auto-gammas by\n"
    "                        pseudo-expected accuracy: every candidate is decoded and valued against the averaged base-pairing\n"
    "                        matrix by F = 2T / (n + S) (T: the probability mass of its pairs, n: their number, S: the mass of\n"
    "                        the matrix; integers, no rounding decides), and the best stays; ties go to the higher threshold.\n"
    "                        With --fold-decoder Levels one auto per level (auto,auto: up to two levels, at most four): a level\n"
    "                        stays only if it raises F.  >SS_cons is the chosen structure.  Not mixed with numbers, not as -t / -g,\n"
    "                        not with --bp-update1 or --seed-structure; with Nussinov one entry\n"
    "      --auto-gammas LIST  With -T auto / -G auto: the candidates' weights, strictly increasing, positive, at most 16\n"
    "                        (default: 1,2,4,8,16,32)\n"
    "      --fold-auto-table OUT  With -T auto / -G auto: per printed alignment a line\n"
    "                        \"# alignment NAME columns L sum_p S\" (NAME: the first row's name in the --stockholm block) and one\n"
    "                        tab-separated line per decoded (level, candidate): level gamma threshold pairs tp f chosen (level\n"
    "                        0-based; tp and S in units of 2^-30; f: F of the levels kept below plus this candidate; chosen 0 / 1)\n"
    "                        With --stockholm every block gains \"#=GF CC SS_cons auto thresholds T0,T1|none f F\"\n"
    "      --bp-update       Re-estimate the base-pairing matrices of the last alignment step under the predicted structure\n"
    "      --bp-update1      The same for the conclusive common secondary structure\n"
    "      --fold-aux FILENAME        Load base-pairing probability matrices from FILENAME\n"
    "      --save-fold-aux FILENAME   Write base-pairing probability matrices in the --fold-aux format\n";

std::vector<float> parse_floats(const std::string& s) {  // cxxopts vector<float>: comma separated
  std::vector<float> v;
  std::stringstream ss(s);
  std::string item;
  while (std::getline(ss, item, ',')) v.push_back(std::stof(item));
  return v;
}

// "auto" or "auto,auto,...": the number of entries; 0 when the value does not name auto at all.  Mixed with numbers, or more
// than four entries: refused
uint32_t parse_auto(const std::string& opt, const std::string& s) {
  if (s.find("auto") == std::string::npos) return 0;
  uint32_t n = 0;
  std::stringstream ss(s);
  std::string item;
  while (std::getline(ss, item, ',')) {
    if (item != "auto") throw opt + ": auto cannot be mixed with numbers (every level's threshold is chosen, or none is)";
    ++n;
  }
  if (!s.empty() && s.back() == ',') throw opt + ": an empty entry";
  if (n < 1 || n > DAFS_HIP_MAX_LEVELS) throw opt + ": " + std::to_string(n) + " entries; one to four levels are decoded";
  return n;
}

Options parse(int argc, char** argv) {
  Options o;
  // long name -> (short char, takes value)
  const std::map<std::string, std::pair<char, bool> > spec = {
      {"help", {'h', false}}, {"version", {0, false}}, {"refinement", {'r', true}}, {"weight", {'w', true}}, {"eta", {0, true}},
      {"max-iter", {'m', true}}, {"fourway-pct", {'f', true}}, {"verbose", {'v', true}}, {"align-model", {'a', true}},
      {"align-pct", {'p', true}}, {"align-th", {'u', true}}, {"align-aux", {0, true}}, {"fold-model", {'s', true}},
      {"fold-decoder", {0, true}}, {"fold-pct", {'q', true}}, {"fold-th", {'t', true}}, {"gamma", {'g', true}},
      {"no-alifold", {0, false}}, {"fold-th1", {'T', true}}, {"gamma1", {'G', true}}, {"ipknot", {0, false}},
      {"bp-update", {0, false}}, {"bp-update1", {0, false}}, {"fold-aux", {0, true}}, {"save-align-aux", {0, true}},
      {"save-fold-aux", {0, true}}, {"device", {0, true}}, {"devices", {0, true}}, {"input", {0, true}},
      {"stockholm", {0, true}}, {"row-structures", {0, false}}, {"seed", {0, true}}, {"pairwise", {0, false}}, {"pairwise-scores", {0, true}},
      {"seed-each", {0, false}}, {"seed-scores", {0, true}}, {"seed-merged", {0, true}}, {"seed-structure", {0, false}}, {"knots", {0, false}},
      {"covariation", {0, true}}, {"cov-shuffles", {0, true}}, {"cov-seed", {0, true}}, {"cov-null", {0, true}}, {"identity", {0, true}},
      {"phylogeny", {0, true}}, {"phylogeny-model", {0, true}}, {"cov-tree", {0, true}},
      {"phylogeny-bootstrap", {0, true}}, {"phylogeny-seed", {0, true}}, {"phylogeny-support", {0, true}},
      {"phylogeny-transfer", {0, false}},
      {"identity-matrix", {0, true}}, {"seed-nearest", {0, false}}, {"seed-nr", {0, true}}, {"describe", {0, true}},
      {"compare", {0, true}}, {"compare-ref", {0, true}}, {"compare-columns", {0, true}}, {"compare-matrix", {0, true}},
      {"cluster", {0, true}}, {"cluster-count", {0, true}}, {"cluster-min-size", {0, true}}, {"cluster-table", {0, true}},
      {"cluster-tree", {0, true}}, {"cluster-linkage", {0, true}}, {"cluster-score", {0, true}}, {"cluster-structure-weight", {0, true}},
      {"auto-gammas", {0, true}}, {"fold-auto-table", {0, true}}};
  std::map<char, std::string> shorts;
  for (const auto& kv : spec)
    if (kv.second.first) shorts[kv.second.first] = kv.first;
  std::vector<float> gamma, gamma1;
  bool th_given = false, th1_given = false, auto_gammas_given = false;
  std::vector<std::string> given;  // every option as it was named, for --describe
  for (int i = 1; i < argc; ++i) {
    std::string arg = argv[i], name, value;
    bool have_value = false;
    if (arg.size() > 2 && arg[0] == '-' && arg[1] == '-') {
      const size_t eq = arg.find('=');
      name = arg.substr(2, eq == std::string::npos ? std::string::npos : eq - 2);
      if (eq != std::string::npos) { value = arg.substr(eq + 1); have_value = true; }
    } else if (arg.size() >= 2 && arg[0] == '-' && !(arg[1] >= '0' && arg[1] <= '9')) {
      if (!shorts.count(arg[1])) throw std::string("Unknown option: ") + arg;
      name = shorts[arg[1]];
      if (arg.size() > 2) { value = arg.substr(2); have_value = true; }
    } else {
      o.input = arg;
      o.inputs.push_back(arg);
      continue;
    }
    const auto it = spec.find(name);
    if (it == spec.end()) throw std::string("Unknown option: ") + arg;
    if (it->second.second && !have_value) {
      if (i + 1 >= argc) throw std::string("Option requires a value: ") + arg;
      value = argv[++i];
    }
    given.push_back(name);
    if (name == "help") { std::cout << kHelp << std::endl; exit(0); }
    else if (name == "version") { std::cout << "DAFS version " << DAFS_VERSION << std::endl; exit(0); }
    else if (name == "refinement") { o.refinement = std::stoi(value); o.refinement_given = true; }
    else if (name == "weight") o.w = std::stof(value);
    else if (name == "eta") o.eta = std::stof(value);
    else if (name == "max-iter") o.max_iter = std::stoi(value);
    else if (name == "fourway-pct") o.fourway = std::stof(value);
    else if (name == "verbose") o.verbose = std::stoi(value);
    else if (name == "align-model") o.align_model = value;
    else if (name == "align-pct") o.align_pct = std::stof(value);
    else if (name == "align-th") o.align_th = std::stof(value);
    else if (name == "align-aux") o.align_aux = value;
    else if (name == "fold-model") { o.fold_model = value; o.fold_model_given = true; }
    else if (name == "fold-decoder") o.fold_decoder = value;
    else if (name == "fold-pct") o.fold_pct = std::stof(value);
    else if ((name == "fold-th" || name == "gamma") && parse_auto("-t / -g", value))
      throw std::string("-t / -g: the threshold inside the dual-decomposition loop cannot be chosen automatically (-T auto / -G auto can)");
    else if (name == "fold-th") { o.fold_th = parse_floats(value); th_given = true; }
    else if (name == "gamma") gamma = parse_floats(value);
    else if (name == "no-alifold") o.no_alifold = true;
    else if ((name == "fold-th1" || name == "gamma1") && (o.auto_levels = parse_auto("-T / -G", value))) {}
    else if (name == "fold-th1") { o.fold_th1 = parse_floats(value); th1_given = true; o.auto_levels = 0; }
    else if (name == "gamma1") { gamma1 = parse_floats(value); o.auto_levels = 0; }
    else if (name == "auto-gammas") {
      size_t used = 0;
      o.auto_gammas.clear();
      std::stringstream gs(value);
      std::string item;
      while (std::getline(gs, item, ',')) {
        float g = 0.0f;
        try { g = std::stof(item, &used); } catch (const std::exception&) { used = 0; }
        if (used == 0 || used != item.size() || !std::isfinite(g) || !(g > 0.0f) || (!o.auto_gammas.empty() && !(g > o.auto_gammas.back())))
          throw std::string("--auto-gammas needs positive, strictly increasing weights");
        o.auto_gammas.push_back(g);
      }
      if (o.auto_gammas.empty() || o.auto_gammas.size() > DAFS_HIP_MAX_CANDIDATES || value.back() == ',')
        throw std::string("--auto-gammas needs one to sixteen weights");
      auto_gammas_given = true;
    }
    else if (name == "fold-auto-table") {
      if (value.empty()) throw std::string("--fold-auto-table needs a file name");
      o.auto_table = value;
    }
    else if (name == "ipknot") o.ipknot = true;
    else if (name == "bp-update") o.bp_update = true;
    else if (name == "bp-update1") o.bp_update1 = true;
    else if (name == "fold-aux") o.fold_aux = value;
    else if (name == "save-align-aux") o.save_align_aux = value;
    else if (name == "save-fold-aux") o.save_fold_aux = value;
    else if (name == "device") o.device = std::stoi(value);
    else if (name == "devices") {
      for (float d : parse_floats(value)) o.devices.push_back((int)d);
      if (o.devices.empty()) throw std::string("--devices needs at least one device index");
    }
    else if (name == "input") { o.input = value; o.inputs.push_back(value); }
    else if (name == "stockholm") {
      if (value.empty()) throw std::string("--stockholm needs a file name");
      o.stockholm = value;
    }
    else if (name == "row-structures") o.row_structures = true;
    else if (name == "seed") {
      if (value.empty()) throw std::string("--seed needs a file name");
      o.seed = value;
    }
    else if (name == "seed-each") o.seed_each = true;
    else if (name == "seed-structure") o.seed_structure = true;
    else if (name == "knots") o.knots = true;
    else if (name == "phylogeny-transfer") o.phylogeny_transfer = true;
    else if (name == "seed-scores") {
      if (value.empty()) throw std::string("--seed-scores needs a file name");
      o.seed_scores = value;
    }
    else if (name == "seed-merged") {
      if (value.empty()) throw std::string("--seed-merged needs a file name");
      o.seed_merged = value;
    }
    else if (name == "pairwise") o.pairwise = true;
    else if (name == "pairwise-scores") {
      if (value.empty()) throw std::string("--pairwise-scores needs a file name");
      o.pairwise_scores = value;
    }
    else if (name == "covariation") {
      if (value.empty()) throw std::string("--covariation needs a file name");
      o.covariation = value;
    }
    else if (name == "identity" || name == "identity-matrix" || name == "describe") {
      if (value.empty()) throw "--" + name + " needs a file name";
      (name == "identity" ? o.identity : name == "describe" ? o.describe : o.identity_matrix) = value;
    }
    else if (name == "phylogeny") {
      if (value.empty()) throw std::string("--phylogeny needs a file name");
      o.phylogeny = value;
    }
    else if (name == "phylogeny-model") {
      if (value == "jc") o.phylogeny_model = DAFS_NJ_JC;
      else if (value == "p") o.phylogeny_model = DAFS_NJ_P;
      else throw std::string(dafs_host_phylogeny_refusal(DAFS_PHYLOGENY_UNKNOWN_MODEL));
      o.phylogeny_model_given = true;
    }
    else if (name == "phylogeny-support") {
      if (value.empty()) throw std::string("--phylogeny-support needs a file name");
      o.phylogeny_support = value;
    }
    else if (name == "phylogeny-bootstrap" || name == "phylogeny-seed") {
      size_t used = 0;
      unsigned long long v = 0;
      try {
        if (value.empty() || value[0] < '0' || value[0] > '9') throw std::invalid_argument(value);
        v = std::stoull(value, &used, 10);
      } catch (const std::exception&) {
        used = 0;
      }
      if (name == "phylogeny-seed") {
        if (used == 0 || used != value.size()) throw std::string("--phylogeny-seed needs a non-negative integer");
        o.phylogeny_seed = v;
        o.phylogeny_seed_given = true;
      } else {
        if (used == 0 || used != value.size() || v < 1 || v > 65536) throw std::string(dafs_host_bootstrap_refusal(DAFS_BOOTSTRAP_COUNT));
        o.phylogeny_bootstrap = (uint32_t)v;
        o.phylogeny_bootstrap_given = true;
      }
    }
    else if (name == "cov-tree") {
      if (value == "average") o.cov_tree_nj = false;
      else if (value == "nj") o.cov_tree_nj = true;
      else throw std::string(dafs_host_phylogeny_refusal(DAFS_PHYLOGENY_UNKNOWN_COV_TREE));
      o.cov_tree_given = true;
    }
    else if (name == "compare" || name == "compare-ref" || name == "compare-columns" || name == "compare-matrix") {
      if (value.empty()) throw "--" + name + " needs a file name";
      (name == "compare" ? o.compare : name == "compare-ref" ? o.compare_ref : name == "compare-columns" ? o.compare_columns : o.compare_matrix) = value;
    }
    else if (name == "cluster") {
      size_t used = 0;
      try {
        o.cluster = std::stod(value, &used);
      } catch (const std::exception&) {
        used = 0;
      }
      if (used == 0 || used != value.size() || !std::isfinite(o.cluster)) throw std::string("--cluster needs a finite threshold");
      o.cluster_given = true;
    }
    else if (name == "cluster-count" || name == "cluster-min-size") {
      size_t used = 0;
      unsigned long long v = 0;
      try {
        if (value.empty() || value[0] < '0' || value[0] > '9') throw std::invalid_argument(value);
        v = std::stoull(value, &used, 10);
      } catch (const std::exception&) {
        used = 0;
      }
      if (used == 0 || used != value.size() || v < 1 || v > 0xFFFFFFFFull) throw "--" + name + " needs a positive integer";
      if (name == "cluster-count") { o.cluster_count = (uint32_t)v; o.cluster_count_given = true; }
      else { o.cluster_min_size = (uint32_t)v; o.cluster_min_size_given = true; }
    }
    else if (name == "cluster-table" || name == "cluster-tree") {
      if (value.empty()) throw "--" + name + " needs a file name";
      (name == "cluster-table" ? o.cluster_table : o.cluster_tree) = value;
    }
    else if (name == "cluster-linkage") {
      static const char* const rules[] = {"guide", "single", "complete", "average"};
      int code = -1;
      for (int r = 0; r < 4; ++r)
        if (value == rules[r]) code = r;
      if (code < 0) throw "--cluster-linkage: unknown rule '" + value + "' (guide, single, complete, average)";
      o.cluster_linkage = code;
      o.cluster_linkage_given = true;
    }
    else if (name == "cluster-score") {
      static const char* const scores[] = {"sequence", "structure", "mix"};  // the index is the library's DAFS_SCORE_* code
      int code = -1;
      for (int r = 0; r < 3; ++r)
        if (value == scores[r]) code = r;
      if (code < 0) throw "--cluster-score: unknown score '" + value + "' (sequence, structure, mix)";
      o.cluster_score = code;
      o.cluster_score_given = true;
    }
    else if (name == "cluster-structure-weight") {
      size_t used = 0;
      double w = 0.0;
      try {
        w = std::stod(value, &used);
      } catch (const std::exception&) {
        used = 0;
      }
      if (used == 0 || used != value.size() || !std::isfinite(w) || !(w >= 0.0 && w <= 1.0))
        throw std::string("--cluster-structure-weight needs a weight in 0 .. 1");
      o.cluster_weight = (float)w;
      o.cluster_weight_given = true;
    }
    else if (name == "seed-nearest") o.seed_nearest = true;
    else if (name == "seed-nr") {
      size_t used = 0;
      try {
        o.seed_nr = std::stod(value, &used);
      } catch (const std::exception&) {
        used = 0;
      }
      if (used == 0 || used != value.size() || !(o.seed_nr > 0.0 && o.seed_nr <= 1.0)) throw std::string(dafs_host_alistat_refusal(DAFS_ALISTAT_NR_THRESHOLD));
      o.seed_nr_given = true;
    }
    else if (name == "cov-null") {
      if (value == "shuffle") o.cov_null = DAFS_COV_NULL_SHUFFLE;
      else if (value == "tree") o.cov_null = DAFS_COV_NULL_TREE;
      else throw "--cov-null: unknown null '" + value + "' (shuffle, tree)";
      o.cov_null_given = true;
    }
    else if (name == "cov-shuffles" || name == "cov-seed") {
      size_t used = 0;
      unsigned long long v = 0;
      try {
        if (value.empty() || value[0] < '0' || value[0] > '9') throw std::invalid_argument(value);
        v = std::stoull(value, &used, 10);
      } catch (const std::exception&) {
        used = 0;
      }
      if (used == 0 || used != value.size() || (name == "cov-shuffles" && v > 0xFFFFFFFFull))
        throw "--" + name + " needs a non-negative integer";
      if (name == "cov-shuffles") { o.cov_shuffles = (uint32_t)v; o.cov_shuffles_given = true; }
      else { o.cov_seed = v; o.cov_seed_given = true; }
    }
  }
  if (o.cluster_given && o.cluster_count_given) throw std::string("--cluster and --cluster-count cut the same tree: give one of them");
  if (!o.cluster_given && !o.cluster_count_given) {
    if (o.cluster_min_size_given || !o.cluster_table.empty() || !o.cluster_tree.empty())
      throw std::string("--cluster-min-size, --cluster-table and --cluster-tree need --cluster or --cluster-count");
    if (o.cluster_linkage_given) throw std::string("--cluster-linkage needs --cluster or --cluster-count");
    if (o.cluster_score_given || o.cluster_weight_given) throw std::string("--cluster-score and --cluster-structure-weight need --cluster or --cluster-count");
  } else {  // the clusters are runs of their own: nothing that reads or writes one run's whole state, and one FILE to cut
    for (const std::string& g : given) {
      const bool other_mode = g.compare(0, 4, "seed") == 0 || g.compare(0, 8, "pairwise") == 0 || g.compare(0, 7, "compare") == 0 ||
                              g == "describe" || g == "devices";
      const bool aux = g == "align-aux" || g == "fold-aux" || g == "save-align-aux" || g == "save-fold-aux";
      if (other_mode || aux) throw "--cluster: --" + g + " cannot be combined with --cluster and --cluster-count";
    }
    if (o.inputs.size() != 1) throw std::string("--cluster needs exactly one input FILE");
  }
  if (o.cluster_weight_given && o.cluster_score != DAFS_SCORE_MIX) throw std::string("--cluster-structure-weight is the weight of --cluster-score mix");
  if (o.row_structures && o.stockholm.empty()) throw std::string("--row-structures needs --stockholm");
  if ((o.cov_shuffles_given || o.cov_seed_given) && o.covariation.empty()) throw std::string("--cov-shuffles and --cov-seed need --covariation");
  if (o.cov_null_given && o.covariation.empty()) throw std::string("--cov-null needs --covariation");
  if (o.cov_tree_given && (!o.cov_null_given || o.cov_null != DAFS_COV_NULL_TREE)) throw std::string(dafs_host_phylogeny_refusal(DAFS_PHYLOGENY_COV_TREE_NEEDS_NULL));
  if (o.phylogeny_model_given && o.phylogeny.empty()) throw std::string(dafs_host_phylogeny_refusal(DAFS_PHYLOGENY_MODEL_NEEDS_TREE));
  if ((o.phylogeny_bootstrap_given || o.phylogeny_seed_given || !o.phylogeny_support.empty()) && o.phylogeny.empty())
    throw std::string(dafs_host_bootstrap_refusal(DAFS_BOOTSTRAP_NEEDS_TREE));
  if ((o.phylogeny_seed_given || !o.phylogeny_support.empty()) && !o.phylogeny_bootstrap_given)
    throw std::string(dafs_host_bootstrap_refusal(DAFS_BOOTSTRAP_NEEDS_REPLICATES));
  if (o.phylogeny_transfer && !o.phylogeny_bootstrap_given) throw std::string(dafs_host_transfer_refusal(DAFS_TRANSFER_NEEDS_REPLICATES));
  if (o.pairwise && !o.phylogeny.empty()) throw std::string(dafs_host_phylogeny_refusal(DAFS_PHYLOGENY_NO_PAIRWISE));
  if (o.seed_each && !o.phylogeny.empty()) throw std::string(dafs_host_phylogeny_refusal(DAFS_PHYLOGENY_NO_SEED_EACH));
  if (o.pairwise && (!o.covariation.empty() || o.cov_shuffles_given || o.cov_seed_given))
    throw std::string("--pairwise: two rows carry no covariation; --covariation, --cov-shuffles and --cov-seed cannot be combined with --pairwise");
  if (!o.describe.empty()) {  // a finished alignment: nothing that aligns, and no FILE
    for (const std::string& g : given)
      if (g != "describe" && g != "identity" && g != "identity-matrix" && g != "covariation" && g != "cov-shuffles" && g != "cov-seed" && g != "cov-null" && g != "device" && g != "knots" &&
          g.compare(0, 9, "phylogeny") != 0 && g != "cov-tree" &&
          g.compare(0, 7, "compare") != 0)
        throw "--describe reads a finished alignment: --" + g + " cannot be combined with --describe";
    if (!o.inputs.empty()) throw std::string("--describe takes no FILE: the alignment is its argument");
    if (o.identity.empty() && o.covariation.empty() && o.compare.empty() && o.compare_ref.empty() && o.phylogeny.empty())
      throw std::string("--describe needs --identity or --covariation");
  }
  if (o.compare.empty() != o.compare_ref.empty()) throw std::string(dafs_host_compare_refusal(DAFS_COMPARE_NEEDS_REF));
  if ((!o.compare_columns.empty() || !o.compare_matrix.empty()) && o.compare.empty()) throw std::string(dafs_host_compare_refusal(DAFS_COMPARE_NEEDS_COMPARE));
  if (o.pairwise && !o.compare.empty()) throw std::string(dafs_host_compare_refusal(DAFS_COMPARE_NO_PAIRWISE));
  if (o.seed_each && !o.compare.empty() && o.seed_merged.empty()) throw std::string(dafs_host_compare_refusal(DAFS_COMPARE_NEEDS_MERGED));
  if (!o.identity_matrix.empty() && o.identity.empty()) throw std::string("--identity-matrix needs --identity");
  if (o.pairwise && !o.identity.empty()) throw std::string(dafs_host_alistat_refusal(DAFS_ALISTAT_NO_PAIRWISE));
  if (o.seed_each && !o.identity.empty()) throw std::string("--seed-each: --identity cannot be combined with --seed-each (--seed-nearest names each new sequence's nearest seed row)");
  if (o.seed_nearest && (!o.seed_each || o.seed_scores.empty())) throw std::string("--seed-nearest needs --seed-each and --seed-scores");
  if (o.seed_nr_given && o.seed_merged.empty()) throw std::string(dafs_host_alistat_refusal(DAFS_ALISTAT_NR_NEEDS_MERGED));
  if (!o.pairwise_scores.empty() && !o.pairwise) throw std::string("--pairwise-scores needs --pairwise");
  if (o.seed_each && o.seed.empty()) throw std::string("--seed-each needs --seed");
  if (!o.seed_scores.empty() && !o.seed_each) throw std::string("--seed-scores needs --seed-each");
  if (!o.seed_merged.empty() && !o.seed_each) throw std::string("--seed-merged needs --seed-each");
  if (!o.seed_merged.empty() && !o.seed_structure) throw std::string(dafs_host_merged_refusal());
  if (o.knots && o.seed.empty() && o.describe.empty() && o.compare_ref.empty())
    throw std::string("--knots says how structures are read: it needs --seed, --describe or --compare-ref");
  if ((auto_gammas_given || !o.auto_table.empty()) && !o.auto_levels) throw std::string("--auto-gammas and --fold-auto-table need -T auto or -G auto");
  if (o.auto_levels) {
    if (o.bp_update1) throw std::string("-T auto / -G auto: what the second decode of --bp-update1 would choose is undecided; they cannot be combined");
    if (o.seed_structure) throw std::string("--seed-structure: nothing is decoded; -T auto and -G auto cannot be combined with --seed-structure");
    if (o.fold_decoder == "Nussinov" && o.auto_levels > 1)
      throw std::string("--fold-decoder Nussinov decodes one level: -T auto / -G auto with " + std::to_string(o.auto_levels) + " entries needs --fold-decoder Levels");
    for (float g : o.auto_gammas) o.auto_cand.push_back(1.0 / (1.0 + g));  // the conversion of -G below
    for (size_t c = 1; c < o.auto_cand.size(); ++c)
      if (!(o.auto_cand[c] < o.auto_cand[c - 1])) throw std::string("--auto-gammas: two weights give the same threshold");
  }
  if (o.seed_structure) {  // the structure is the seed's: nothing is decoded, so nothing sets a decoder's threshold
    if (o.seed.empty()) throw std::string("--seed-structure needs --seed");
    if (o.bp_update1) throw std::string("--seed-structure: nothing is decoded; --bp-update1 cannot be combined with --seed-structure");
    if (th1_given || !gamma1.empty()) throw std::string("--seed-structure: nothing is decoded; -T and -G cannot be combined with --seed-structure");
  }
  if (o.pairwise) {  // every pair is a two-sequence run of its own: nothing that reads or writes one run's whole state
    if (o.refinement_given) throw std::string("--pairwise: -r cannot be combined with --pairwise");
    if (!o.seed.empty()) throw std::string("--pairwise: --seed cannot be combined with --pairwise");
    if (!o.devices.empty()) throw std::string("--pairwise: --devices cannot be combined with --pairwise (use --device)");
    if (!o.align_aux.empty() || !o.fold_aux.empty() || !o.save_align_aux.empty() || !o.save_fold_aux.empty())
      throw std::string("--pairwise: --align-aux, --fold-aux, --save-align-aux and --save-fold-aux cannot be combined with --pairwise");
    if (o.inputs.size() > 1) throw std::string("--pairwise needs exactly one input FILE");
  }
  if (!o.seed.empty()) {  // the seed's columns stay as they are: nothing may realign its rows
    if (o.refinement_given) throw std::string("--seed: -r would realign the seed's rows; it cannot be combined with --seed");
    if (o.bp_update) throw std::string("--seed: --bp-update cannot be combined with --seed (--bp-update1 can)");
    if (!o.devices.empty()) throw std::string("--seed: --devices cannot be combined with --seed (use --device)");
    if (!o.align_aux.empty() || !o.fold_aux.empty() || !o.save_align_aux.empty() || !o.save_fold_aux.empty())
      throw std::string("--seed: --align-aux, --fold-aux, --save-align-aux and --save-fold-aux cannot be combined with --seed");
    if (o.inputs.size() != 1) throw std::string("--seed needs exactly one FILE of new sequences");
  }
  if (o.inputs.size() > 1) {
    if (!o.align_aux.empty() || !o.fold_aux.empty() || !o.save_align_aux.empty() || !o.save_fold_aux.empty())
      throw std::string("--align-aux, --fold-aux, --save-align-aux and --save-fold-aux name one file each: they need a single input FILE");
    if (!o.devices.empty()) throw std::string("--devices shards one input: it needs a single input FILE");
  }
  // thresholds, reference src/dafs.cpp:1709-1750
  if (!th_given && !gamma.empty()) {
    o.fold_th = gamma;
    for (float& t : o.fold_th) t = 1.0 / (1.0 + t);
  }
  if (!th1_given) {
    if (!gamma1.empty()) {
      o.fold_th1 = gamma1;
      for (float& t : o.fold_th1) t = 1.0 / (1.0 + t);
    } else {
      o.fold_th1 = o.fold_th;
    }
  }
  if (o.auto_levels) o.fold_th1 = o.fold_th;  // not read: every decode chooses among auto_cand
  if (o.fold_decoder == "Levels" && !o.auto_levels) {  // one level per entry of -T / -G
    if (o.bp_update1)
      throw std::string("--fold-decoder Levels: --bp-update1 is not built for it (the reference folds again per level, under each level's constraint)");
    if (o.seed_structure) throw std::string("--seed-structure: nothing is decoded; --fold-decoder Levels cannot be combined with --seed-structure");
    if (o.fold_th1.empty() || o.fold_th1.size() > DAFS_HIP_MAX_LEVELS)
      throw std::string("--fold-decoder Levels: -T / -G hold " + std::to_string(o.fold_th1.size()) + " thresholds; one to four levels are decoded");
    for (size_t k = 1; k < o.fold_th1.size(); ++k)
      if (!(o.fold_th1[k] > 0.0f)) throw std::string("--fold-decoder Levels: the thresholds of the levels above the first must be positive");
  }
  if (o.input.empty() && o.describe.empty()) { std::cout << kHelp << std::endl; exit(0); }
  return o;
}

// ---------------------------------------------------------------------------------------------
typedef std::pair<float, std::pair<uint, uint> > node_t;

// DAFS::build_tree, reference src/dafs.cpp:446-492 (dafs_host_build_tree in the library; host code)
std::vector<node_t> build_tree(const std::vector<float>& sim, uint n0) {
  std::vector<float> score(2 * n0 - 1);
  std::vector<int32_t> left(2 * n0 - 1), right(2 * n0 - 1);
  check(dafs_host_build_tree(n0, sim.data(), score.data(), left.data(), right.data()));
  std::vector<node_t> tree(2 * n0 - 1);
  for (uint i = 0; i < 2 * n0 - 1; ++i) tree[i] = std::make_pair(score[i], std::make_pair((uint)left[i], (uint)right[i]));
  return tree;
}

void print_tree(std::ostream& os, const std::vector<node_t>& tree, const std::vector<Fasta>& fa, int i) {  // :495-511
  if (tree[i].second.first == -1u) { os << fa[i].name(); return; }
  os << "[ " << tree[i].first << " ";
  print_tree(os, tree, fa, tree[i].second.first);
  os << " ";
  print_tree(os, tree, fa, tree[i].second.second);
  os << " ]";
}

// DAFS::project_alignment, :766-825
void project_alignment(ALN& aln, const ALN& a1, const ALN& a2, const VU& z) {
  const uint L1 = (uint)a1[0].second.size(), L2 = (uint)a2[0].second.size();
  std::vector<int> c1, c2;  // per merged column: source column of aln1 / aln2, or -1
  uint k = 0;
  for (uint i = 0; i != L1; ++i) {
    if (z[i] != -1u) {
      while (k < z[i]) { c1.push_back(-1); c2.push_back((int)k++); }
      c1.push_back((int)i);
      c2.push_back((int)k++);
    } else {
      c1.push_back((int)i);
      c2.push_back(-1);
    }
  }
  while (k < L2) { c1.push_back(-1); c2.push_back((int)k++); }
  const size_t L = c1.size();
  aln.clear();
  for (const auto& row : a1) {
    std::vector<bool> m(L, false);
    for (size_t c = 0; c < L; ++c) m[c] = c1[c] >= 0 && row.second[c1[c]];
    aln.push_back(std::make_pair(row.first, m));
  }
  for (const auto& row : a2) {
    std::vector<bool> m(L, false);
    for (size_t c = 0; c < L; ++c) m[c] = c2[c] >= 0 && row.second[c2[c]];
    aln.push_back(std::make_pair(row.first, m));
  }
}

struct NodeJob {  // one node: its flattened child alignments and output buffers, and in / out pointing into them (moved, never copied)
  std::vector<uint32_t> s1, s2;
  std::vector<uint8_t> m1, m2;
  std::vector<float> px, py;  // --bp-update: re-estimated base-pairing matrices
  VU x, y, z;
  dafs_node_input in;
  dafs_node_output out;
};

// the `if (use_bp_update_)` blocks of align_alignments(ss, ...), :919-934, and of DAFS::run, :1863-1869: decode the averaged
// matrix, re-estimate it under that structure (update_basepairing_probability, :609-712)
void updated_bp(dafs_hip_ctx* ctx, uint32_t n, uint32_t len, const std::vector<uint32_t>& seq, const std::vector<uint8_t>& mask, float th,
                std::vector<float>& p) {
  VU ss(len);
  check(dafs_hip_consensus_structure(ctx, n, len, seq.data(), mask.data(), th, ss.data(), nullptr, nullptr));
  p.resize((size_t)len * len);
  check(dafs_hip_update_basepairing(ctx, n, len, seq.data(), mask.data(), ss.data(), p.data()));
}
void flatten(const ALN& a, std::vector<uint32_t>& s, std::vector<uint8_t>& m) {
  const size_t L = a[0].second.size();
  s.resize(a.size());
  m.resize(a.size() * L);
  for (size_t r = 0; r < a.size(); ++r) {
    s[r] = a[r].first;
    for (size_t c = 0; c < L; ++c) m[r * L + c] = a[r].second[c] ? 1 : 0;
  }
}

// The node that aligns the flattened alignments j.s1 / j.m1 (left) and j.s2 / j.m2 (right): sizes its output buffers and
// sets j.in and j.out.  bp_update: both base-pairing matrices re-estimated under the structure decoded from their averages
// (updated_bp), the top call of the recursion and refine() (align_alignments(ss, ...), :919-934).
void node_job(dafs_hip_ctx* ctx, NodeJob& j, bool bp_update, float th_s) {
  const uint32_t n1 = (uint32_t)j.s1.size(), n2 = (uint32_t)j.s2.size(), len1 = (uint32_t)(j.m1.size() / n1),
                 len2 = (uint32_t)(j.m2.size() / n2);
  j.x.resize(len1); j.y.resize(len2); j.z.resize(len1);
  j.in = dafs_node_input{n1, n2, len1, len2, j.s1.data(), j.s2.data(), j.m1.data(), j.m2.data(), nullptr, nullptr};
  if (bp_update) {
    updated_bp(ctx, n1, len1, j.s1, j.m1, th_s, j.px);
    updated_bp(ctx, n2, len2, j.s2, j.m2, th_s, j.py);
    j.in.p_x = j.px.data(); j.in.p_y = j.py.data();
  }
  j.out = dafs_node_output{j.x.data(), j.y.data(), j.z.data(), 0.0f, 0, 0, 0};
}

// align_alignments of a1 with a2 (:896-981) into out; returns the node's score
float solve_node(dafs_hip_ctx* ctx, const dafs_dd_params& prm, const ALN& a1, const ALN& a2, ALN& out, int verbose, bool bp_update) {
  NodeJob j;
  flatten(a1, j.s1, j.m1);
  flatten(a2, j.s2, j.m2);
  node_job(ctx, j, bp_update, prm.th_s);  // refine() goes through align_alignments(ss, ...) too
  check(dafs_hip_solve_nodes(ctx, 1, &j.in, &prm, &j.out));
  project_alignment(out, a1, a2, j.z);
  if (verbose >= 1) std::cerr << "Step: " << j.out.iterations << ", Violated: " << j.out.violated << std::endl;  // :1292
  return j.out.score;
}

// The resident-node rounds (dafs_hip_nodes_*; pipeline._solve_nodes is the Python twin).  A round is one call
// (dafs_hip_nodes_round): the open nodes advance, in opening order, while the nodes take_ready() returns (key, job) are set
// up and started beside them, and all of them stop together after the round's budget of microseconds, so a node that needs
// the full iteration budget does not hold back its level and the set-up of new nodes does not stand between two launches.
// take_ready() is called once per round, after the last round's finished nodes have gone to finish(key, job), which gets
// every node once, its result in job.out; -v prints its "Step:" line (:1292).  The rounds end when take_ready() returns
// nothing and no node is open.
void run_rounds(dafs_hip_ctx* ctx, const dafs_dd_params& prm, int verbose,
                const std::function<std::vector<std::pair<size_t, NodeJob> >()>& take_ready,
                const std::function<void(size_t, NodeJob&)>& finish) {
  const uint32_t round_us = getenv("DAFS_ROUND_US") ? (uint32_t)atoi(getenv("DAFS_ROUND_US")) : 2500u;
  struct Open { size_t key; uint32_t handle; NodeJob job; };
  std::vector<Open> open;
  while (true) {
    std::vector<std::pair<size_t, NodeJob> > ready = take_ready();
    const size_t n_old = open.size(), n_new = ready.size();
    if (!n_old && !n_new) break;
    // one entry more than the nodes: an empty list passes valid pointers too
    std::vector<dafs_node_input> in(n_new + 1);
    std::vector<uint32_t> handles(n_old + n_new + 1);
    std::vector<uint8_t> fin(n_old + n_new + 1, 0);
    for (size_t k = 0; k < n_old; ++k) handles[k] = open[k].handle;
    for (size_t b = 0; b < n_new; ++b) in[b] = ready[b].second.in;
    check(dafs_hip_nodes_round(ctx, (uint32_t)n_new, in.data(), handles.data() + n_old, (uint32_t)n_old, handles.data(), &prm, 0, round_us,
                               fin.data(), fin.data() + n_old));
    for (size_t b = 0; b < n_new; ++b) open.push_back(Open{ready[b].first, handles[n_old + b], std::move(ready[b].second)});
    std::vector<Open> still;
    for (size_t k = 0; k < open.size(); ++k) {
      if (!fin[k]) { still.push_back(std::move(open[k])); continue; }
      NodeJob& j = open[k].job;
      check(dafs_hip_nodes_result(ctx, open[k].handle, &j.out));
      if (verbose >= 1) std::cerr << "Step: " << j.out.iterations << ", Violated: " << j.out.violated << std::endl;  // :1292
      finish(open[k].key, j);
    }
    open.swap(still);
  }
  check(dafs_hip_nodes_close(ctx));
}

// --fold-aux reader, reference src/fold.cpp:230-259 ("> x" then "i j:p j:p ...", all 1-based)
void load_fold_aux(const std::string& file, const std::vector<Fasta>& fa, std::vector<BP>& bp) {
  std::ifstream is(file.c_str());
  if (!is.is_open()) throw strerror(errno);
  bp.assign(fa.size(), BP());
  for (size_t x = 0; x < fa.size(); ++x) bp[x].resize(fa[x].size());
  std::string s, t;
  uint x = 0, i, j;
  float p;
  while (std::getline(is, s)) {
    std::istringstream ss(s);
    if (!s.empty() && s[0] == '>') {
      ss >> t >> x;
      if (x < 1 || x > bp.size()) throw "fold-aux: sequence index out of range";
    } else {
      if (!(ss >> i) || x == 0) continue;
      if (i - 1 >= bp[x - 1].size()) bp[x - 1].resize(i);
      while (ss >> t)
        if (sscanf(t.c_str(), "%u:%f", &j, &p) == 2) bp[x - 1][i - 1].push_back(std::make_pair(j - 1, p));
    }
  }
  for (size_t k = 0; k < fa.size(); ++k)
    if (bp[k].size() != fa[k].size()) throw "fold-aux: row count does not match the sequence length";
}

void upload_bp(dafs_hip_ctx* ctx, const std::vector<BP>& bp) {
  std::vector<uint32_t> rowptr, col;
  std::vector<float> val;
  for (const BP& b : bp) {
    uint32_t n = 0;
    for (const SV& row : b) {
      rowptr.push_back(n);
      for (const auto& e : row) { col.push_back(e.first); val.push_back(e.second); ++n; }
    }
    rowptr.push_back(n);
  }
  check(dafs_hip_set_bp(ctx, rowptr.data(), col.data(), val.data()));
}

// writers in the formats the reference's readers accept (its own writers are compiled out,
// reference src/dafs.cpp:221-256); 1-based like load_bp / load_mp expect
void save_fold_aux(dafs_hip_ctx* ctx, const std::string& file, const std::vector<Fasta>& fa) {
  uint64_t nnz = 0, nrp = 0;
  check(dafs_hip_bp_result_size(ctx, 0, &nnz, &nrp));
  std::vector<uint32_t> rowptr(nrp), col(nnz);
  std::vector<float> val(nnz);
  check(dafs_hip_bp_fetch(ctx, 0, rowptr.data(), col.data(), val.data()));
  std::ofstream os(file.c_str());
  os.precision(9);
  size_t r = 0, e = 0;
  for (size_t x = 0; x < fa.size(); ++x) {
    os << "> " << x + 1 << std::endl;
    for (uint32_t i = 0; i < fa[x].size(); ++i) {
      os << i + 1;
      for (uint32_t k = rowptr[r + i]; k < rowptr[r + i + 1]; ++k) os << " " << col[e + k] + 1 << ":" << val[e + k];
      os << std::endl;
    }
    e += rowptr[r + fa[x].size()];
    r += fa[x].size() + 1;
  }
}
// --align-aux reader, reference src/align.cpp:204-246 ("> x y" then "i k:p k:p ...", all 1-based); the rows go to
// the device through dafs_hip_set_mp, which also lays out the transposes and computes the similarity scores
void load_align_aux(dafs_hip_ctx* ctx, const std::string& file, const std::vector<Fasta>& fa) {
  std::ifstream is(file.c_str());
  if (!is.is_open()) throw strerror(errno);
  const uint N = (uint)fa.size();
  std::vector<std::vector<std::vector<std::vector<std::pair<uint, float> > > > > mp(N);  // [x][y][i] -> (k, p)
  for (uint x = 0; x < N; ++x) {
    mp[x].resize(N);
    for (uint y = x + 1; y < N; ++y) mp[x][y].resize(fa[x].size());
  }
  std::string s, t;
  uint x = 0, y = 0;
  while (std::getline(is, s)) {
    if (s.empty()) continue;
    std::istringstream ss(s);
    if (s[0] == '>') {
      ss >> t >> x >> y;
      if (!(x < y && x >= 1 && y <= N)) throw "--align-aux: bad pair header";
    } else {
      uint i = 0, k = 0;
      float pr = 0;
      ss >> i;
      if (x == 0 || i < 1 || i > fa[x - 1].size()) throw "--align-aux: bad row index";
      while (ss >> t)
        if (sscanf(t.c_str(), "%u:%f", &k, &pr) == 2) {
          if (k < 1 || k > fa[y - 1].size()) throw "--align-aux: bad column index";
          mp[x - 1][y - 1][i - 1].push_back(std::make_pair(k - 1, pr));
        }
    }
  }
  std::vector<uint32_t> nnz, rowptr, col;
  std::vector<float> val;
  for (uint a = 0; a < N; ++a)
    for (uint b = a + 1; b < N; ++b) {
      uint32_t run = 0;
      rowptr.push_back(0);
      for (const auto& row : mp[a][b]) {
        for (const auto& e : row) { col.push_back(e.first); val.push_back(e.second); }
        run += (uint32_t)row.size();
        rowptr.push_back(run);
      }
      nnz.push_back(run);
    }
  if (col.empty()) { col.push_back(0); val.push_back(0.0f); }
  check(dafs_hip_set_mp(ctx, nnz.data(), rowptr.data(), col.data(), val.data()));
}

void save_align_aux(dafs_hip_ctx* ctx, const std::string& file, const std::vector<Fasta>& fa) {
  uint64_t np = 0, nnz = 0, nrp = 0;
  check(dafs_hip_mp_result_size(ctx, 0, &np, &nnz, &nrp));
  std::vector<uint32_t> px(np), py(np), cnt(np), rowptr(nrp), col(2 * nnz);
  std::vector<float> val(2 * nnz);
  check(dafs_hip_mp_fetch(ctx, 0, px.data(), py.data(), cnt.data(), rowptr.data(), col.data(), val.data()));
  std::ofstream os(file.c_str());
  os.precision(9);
  size_t r = 0, e = 0;
  for (uint64_t p = 0; p < np; ++p) {
    const uint32_t L1 = fa[px[p]].size(), L2 = fa[py[p]].size();
    os << "> " << px[p] + 1 << " " << py[p] + 1 << std::endl;
    for (uint32_t i = 0; i < L1; ++i) {
      os << i + 1;
      for (uint32_t k = rowptr[r + i]; k < rowptr[r + i + 1]; ++k) os << " " << col[e + k] + 1 << ":" << val[e + k];
      os << std::endl;
    }
    r += (size_t)L1 + 1 + L2 + 1;
    e += 2 * (size_t)cnt[p];
  }
}

// ---------------------------------------------------------------------------------------------
// The text formats -- the Stockholm block of --stockholm, the tables of --covariation and --pairwise-scores, the seed reader of
// --seed -- and the memory estimates of --pairwise are the library's (dafs_amd/csrc/host_text.cpp; the Python driver calls
// the same functions).  Here: the calls.

std::string take(char* text) {  // a text the library returned: copied and freed
  std::string s(text);
  dafs_host_free(text);
  return s;
}

void check_text(int rc) {  // a refusal of a host text function carries its own message
  if (rc == DAFS_HIP_EINVAL) throw std::string(dafs_hip_last_error());
  check(rc);
}

std::vector<const char*> c_strs(const std::vector<std::string>& v) {
  std::vector<const char*> p;
  for (const std::string& s : v) p.push_back(s.c_str());
  return p;
}

std::vector<std::string> lines_of(const std::string& joined, size_t n) {  // the n strings of a '\n'-joined list
  std::vector<std::string> out;
  for (size_t b = 0; out.size() < n;) {
    const size_t e = joined.find('\n', b);
    out.push_back(joined.substr(b, e == std::string::npos ? e : e - b));
    if (e == std::string::npos) break;
    b = e + 1;
  }
  return out;
}

std::vector<std::string> stockholm_names(const std::vector<std::string>& headers) {  // the Stockholm names of these headers
  char* text = nullptr;
  check_text(dafs_host_stockholm_names((uint32_t)headers.size(), c_strs(headers).data(), &text));
  return lines_of(take(text), headers.size());
}

// The chunks of items of these estimated device bytes: greedy in order under dafs_host_batch_bytes(), an item over the budget
// alone; [begin, end) each
std::vector<std::pair<size_t, size_t> > chunks(const std::vector<uint64_t>& bytes) {
  std::vector<uint32_t> chunk_of(bytes.size());
  check(dafs_host_pack_greedy((uint32_t)bytes.size(), bytes.data(), dafs_host_batch_bytes(), chunk_of.data()));
  std::vector<std::pair<size_t, size_t> > out;
  for (size_t k = 0; k < bytes.size(); ++k) {
    if (k == 0 || chunk_of[k] != chunk_of[k - 1]) out.push_back(std::make_pair(k, k));
    out.back().second = k + 1;
  }
  return out;
}

std::vector<uint8_t> cells_of(const std::vector<std::string>& rows) {
  const size_t L = rows.empty() ? 0 : rows[0].size();
  std::vector<uint8_t> cell(rows.size() * L);
  for (size_t r = 0; r < rows.size(); ++r)
    for (size_t c = 0; c < L; ++c) cell[r * L + c] = dafs_host_ali_code(rows[r][c]);
  return cell;
}

// The neighbour-joining tree of an alignment's rows (Context.alignment_tree is the Python twin): the
// identity counts, the distances under `model`, the joins on the device.  left, right, length: 2n-1 entries.
void nj_of(dafs_hip_ctx* ctx, int model, const std::vector<std::string>& rows, std::vector<int32_t>& left, std::vector<int32_t>& right,
           std::vector<double>& length) {
  const uint32_t n = (uint32_t)rows.size(), L = (uint32_t)rows[0].size();
  if (n > 16384) throw std::string(dafs_host_phylogeny_refusal(DAFS_PHYLOGENY_TOO_MANY_ROWS));
  const std::vector<uint8_t> cell = cells_of(rows);
  std::vector<uint32_t> ident((size_t)n * n), aligned((size_t)n * n);
  check(dafs_hip_alignment_identity(ctx, n, L, cell.data(), nullptr, nullptr, 0.0, nullptr, ident.data(), aligned.data(), nullptr, nullptr, nullptr,
                                    nullptr));
  std::vector<double> dist((size_t)n * n);
  check_text(dafs_host_nj_distances(n, ident.data(), aligned.data(), model, dist.data()));
  left.assign(2 * (size_t)n - 1, -1);
  right.assign(2 * (size_t)n - 1, -1);
  length.assign(2 * (size_t)n - 1, 0.0);
  check_text(dafs_hip_nj_tree(ctx, n, dist.data(), left.data(), right.data(), length.data()));
}

// --phylogeny: the Newick line of one printed alignment; names: the rows' Stockholm names.  With --phylogeny-bootstrap the joins
// carry their support and table is the text of --phylogeny-support; with --phylogeny-transfer both show
// the transfer bootstrap (section 28).
void phylogeny_of(dafs_hip_ctx* ctx, const Options& o, const std::vector<std::string>& names, const std::vector<std::string>& rows, std::string& newick,
                  std::string& table) {
  std::vector<int32_t> left, right;
  std::vector<double> length;
  nj_of(ctx, o.phylogeny_model, rows, left, right, length);
  const uint32_t n = (uint32_t)rows.size();
  char* text = nullptr;
  if (!o.phylogeny_bootstrap) {
    check_text(dafs_host_newick(n, c_strs(names).data(), left.data(), right.data(), length.data(), &text));
    newick = take(text);
    return;
  }
  const std::vector<uint8_t> cell = cells_of(rows);
  std::vector<int32_t> support(2 * (size_t)n - 1, -1);
  if (o.phylogeny_transfer) {
    std::vector<int64_t> transfer(2 * (size_t)n - 1, -1);
    check_text(dafs_hip_alignment_bootstrap_transfer(ctx, n, (uint32_t)rows[0].size(), cell.data(), nullptr, o.phylogeny_model, o.phylogeny_bootstrap,
                                                     o.phylogeny_seed, left.data(), right.data(), support.data(), nullptr, nullptr, transfer.data()));
    check_text(dafs_host_newick_transfer(n, c_strs(names).data(), left.data(), right.data(), length.data(), transfer.data(), o.phylogeny_bootstrap, &text));
    newick = take(text);
    check_text(dafs_host_transfer_table(n, c_strs(names).data(), left.data(), right.data(), support.data(), transfer.data(), o.phylogeny_bootstrap,
                                        o.phylogeny_seed, o.phylogeny_model, &text));
    table = take(text);
    return;
  }
  check_text(dafs_hip_alignment_bootstrap(ctx, n, (uint32_t)rows[0].size(), cell.data(), nullptr, o.phylogeny_model, o.phylogeny_bootstrap,
                                          o.phylogeny_seed, left.data(), right.data(), support.data(), nullptr, nullptr));
  check_text(dafs_host_newick_support(n, c_strs(names).data(), left.data(), right.data(), length.data(), support.data(), o.phylogeny_bootstrap, &text));
  newick = take(text);
  check_text(dafs_host_support_table(n, c_strs(names).data(), left.data(), right.data(), support.data(), o.phylogeny_bootstrap, o.phylogeny_seed,
                                     o.phylogeny_model, &text));
  table = take(text);
}

// --covariation: the statistics of one printed alignment (dafs_hip_alignment_covariation_null).
const double kCovEMax = 0.05;  // the cut of cov_SS_cons

// rows: the printed rows; ss: the structure.  tsv: the table of this alignment; chars: the cov_SS_cons characters.
void covariation_of(dafs_hip_ctx* ctx, const Options& o, const std::vector<std::string>& rows, const std::vector<uint32_t>& ss,
                    std::string& tsv, std::string& chars) {
  const uint32_t n = (uint32_t)rows.size(), L = (uint32_t)ss.size();
  std::vector<uint8_t> code((size_t)n * L);
  for (uint32_t r = 0; r < n; ++r)
    for (uint32_t c = 0; c < L; ++c) code[(size_t)r * L + c] = dafs_host_cov_code(rows[r][c]);
  std::vector<uint32_t> best(L), prow(L), pcan(L), ptyp(L);
  std::vector<double> bscore(L), be(L), pscore(L), pe(L);
  std::vector<int32_t> left, right;  // --cov-tree nj: the neighbour-joining tree of the rows (model jc); else the library's default
  if (o.cov_tree_nj && n >= 2) {
    std::vector<double> length;
    nj_of(ctx, DAFS_NJ_JC, rows, left, right, length);
  }
  const int rc = dafs_hip_alignment_covariation_null(ctx, n, L, code.data(), ss.data(), o.cov_shuffles, o.cov_seed, o.cov_null,
                                                     left.empty() ? nullptr : left.data(), right.empty() ? nullptr : right.data(),
                                                     nullptr, best.data(), bscore.data(), be.data(), pscore.data(), pe.data(), prow.data(),
                                                     pcan.data(), ptyp.data(), nullptr, nullptr);
  if (o.cov_null == DAFS_COV_NULL_TREE) check_text(rc);  // the tree null's refusals carry a message (a row without a base)
  else check(rc);
  char* text = nullptr;
  check_text(dafs_host_cov_ss_cons(L, ss.data(), pe.data(), kCovEMax, &text));
  chars = take(text);
  check_text(dafs_host_covariation_table(n, L, code.data(), ss.data(), best.data(), bscore.data(), be.data(), pscore.data(), pe.data(),
                                         prow.data(), pcan.data(), ptyp.data(), &text));
  tsv = take(text);
}

// --identity: how similar the rows of one printed alignment are (dafs_hip_alignment_identity, dafs_hip_alignment_weights;
// DESIGN.md section 18)
struct IdentityText {
  std::string table, matrix;    // the tables of --identity and --identity-matrix
  std::vector<double> weight;   // the WT lines of the Stockholm block
};

// names: the rows' Stockholm names; matrix: the pair table too
void identity_of(dafs_hip_ctx* ctx, const std::vector<std::string>& names, const std::vector<std::string>& rows, bool matrix, IdentityText& out) {
  const uint32_t n = (uint32_t)rows.size(), L = (uint32_t)rows[0].size();
  if (n > 32768) throw std::string(dafs_host_alistat_refusal(DAFS_ALISTAT_TOO_MANY_ROWS));  // the summary reads the whole matrix
  const std::vector<uint8_t> cell = cells_of(rows);
  std::vector<uint32_t> res(n), near(n), ni(n), nd(n), ident((size_t)n * n), aligned(matrix ? (size_t)n * n : 0);
  check(dafs_hip_alignment_identity(ctx, n, L, cell.data(), nullptr, nullptr, 0.0, res.data(), ident.data(), matrix ? aligned.data() : nullptr,
                                    near.data(), ni.data(), nd.data(), nullptr));
  out.weight.assign(n, 0.0);
  check(dafs_hip_alignment_weights(ctx, n, L, cell.data(), nullptr, out.weight.data()));
  double summary[3];
  check(dafs_host_identity_summary(n, ident.data(), res.data(), summary));
  char* text = nullptr;
  check_text(dafs_host_identity_table(n, L, c_strs(names).data(), res.data(), out.weight.data(), near.data(), ni.data(), nd.data(), summary, &text));
  out.table = take(text);
  if (matrix) {
    check_text(dafs_host_identity_matrix_table(n, c_strs(names).data(), res.data(), ident.data(), aligned.data(), &text));
    out.matrix = take(text);
  }
}

void write_tables(const std::string& option, const std::string& file, const std::vector<std::string>& tables, const std::vector<std::string>* headers) {
  std::ofstream os(file.c_str(), std::ios::binary);
  if (!os.is_open()) throw option + ": cannot open " + file;
  for (size_t k = 0; k < tables.size(); ++k) {
    if (headers) os << "==> " << (*headers)[k] << " <==\n";
    os << tables[k];
  }
  os.flush();
  if (!os) throw option + ": cannot write " + file;
}

void write_text(const std::string& option, const std::string& file, const std::string& text) { write_tables(option, file, {text}, nullptr); }

void write_identity(const Options& o, const std::vector<IdentityText>& idt, const std::vector<std::string>* headers) {
  std::vector<std::string> tables, matrices;
  for (const IdentityText& t : idt) { tables.push_back(t.table); matrices.push_back(t.matrix); }
  write_tables("--identity", o.identity, tables, headers);
  if (!o.identity_matrix.empty()) write_tables("--identity-matrix", o.identity_matrix, matrices, headers);
}

typedef std::vector<uint8_t> VL;  // per column the level of its pair, 0xFF at unpaired columns (DESIGN.md sections 25 and 26)

// --compare: a printed alignment against the reference of --compare-ref (dafs_hip_alignment_compare; DESIGN.md section 19;
// pipeline.compare is the Python twin)
struct CompareText {
  std::string table, columns, matrix;  // the tables of --compare, --compare-columns and --compare-matrix
};

// An alignment file as the seed reader reads it: names, cleaned rows, the structure over the cleaned columns if it has one
// (has_ss), and with pp the PP rows of a Stockholm file (left empty when it has no PP line)
// level (--knots): the structure may cross (dafs_host_seed_clean_structure_levels), and *level receives its pairs' levels
void read_alignment(const std::string& file, const std::string& option, std::vector<std::string>& names, std::vector<std::string>& rows, VU& ss,
                    bool& has_ss, std::vector<std::string>* pp = nullptr, VL* level = nullptr) {
  std::ifstream is(file.c_str(), std::ios::binary);
  if (!is.is_open()) throw option + ": cannot open " + file;
  const std::string text((std::istreambuf_iterator<char>(is)), std::istreambuf_iterator<char>());
  uint32_t n = 0;
  char *nm = nullptr, *rw = nullptr, *st = nullptr;
  int has = 0;
  check_text(dafs_host_seed_parse_structure(text.data(), text.size(), &n, &has, &nm, &rw, &st));
  names = lines_of(take(nm), n);
  rows = lines_of(take(rw), n);
  const std::string structure = take(st);
  has_ss = has != 0;
  if (has_ss) {
    ss.assign(rows.empty() ? 1 : rows[0].size() + 1, DAFS_HIP_NONE);
    uint32_t columns = 0;
    if (level) {
      level->assign(ss.size(), 0xFF);
      check_text(dafs_host_seed_clean_structure_levels(n, c_strs(names).data(), c_strs(rows).data(), structure.c_str(), ss.data(), level->data(),
                                                       &columns, &rw));
      level->resize(columns);
    } else {
      check_text(dafs_host_seed_clean_structure(n, c_strs(names).data(), c_strs(rows).data(), structure.c_str(), ss.data(), &columns, &rw));
    }
    rows = lines_of(take(rw), n);
    ss.resize(columns);
  } else {
    check_text(dafs_host_seed_clean(n, c_strs(names).data(), c_strs(rows).data(), &rw));
    rows = lines_of(take(rw), n);
  }
  if (pp) {
    int has_pp = 0;
    char* pt = nullptr;
    check_text(dafs_host_seed_pp(text.data(), text.size(), &n, &has_pp, &pt));
    const std::vector<std::string> got = lines_of(take(pt), n);
    if (has_pp) *pp = got;
  }
}

struct Reference {
  std::vector<std::string> names, rows;
  VU ss;
  bool has_ss = false;
};

// the reference of --compare-ref, read once
const Reference& reference_of(const Options& o) {
  static Reference ref;
  static bool loaded = false;
  if (!loaded) {
    VL level;  // --knots: the comparison reads the merged pairs
    read_alignment(o.compare_ref, "--compare-ref", ref.names, ref.rows, ref.ss, ref.has_ss, nullptr, o.knots ? &level : nullptr);
    loaded = true;
  }
  return ref;
}

// names: the rows' Stockholm names; ss: the alignment's structure or nullptr; use: its aligned columns or nullptr (all); pp:
// per row its PP characters ("" for a row without) or nullptr
void compare_of(dafs_hip_ctx* ctx, const Options& o, const std::vector<std::string>& names, const std::vector<std::string>& rows, const VU* ss,
                const uint8_t* use, const std::vector<std::string>* pp, CompareText& out) {
  const Reference& ref = reference_of(o);
  const uint32_t nr = (uint32_t)ref.names.size(), nt = (uint32_t)names.size();
  std::vector<uint32_t> ref_row(std::min(nr, nt) + 1), test_row(std::min(nr, nt) + 1);
  uint32_t n = 0;
  check_text(dafs_host_compare_match(nr, c_strs(ref.names).data(), nt, c_strs(names).data(), &n, ref_row.data(), test_row.data()));
  const bool matrix = !o.compare_matrix.empty(), both = ref.has_ss && ss;
  if (matrix && n > 16384) throw std::string(dafs_host_compare_refusal(DAFS_COMPARE_TOO_MANY_ROWS));
  std::vector<std::string> rr, tr, row_names;
  for (uint32_t k = 0; k < n; ++k) {
    rr.push_back(ref.rows[ref_row[k]]);
    tr.push_back(rows[test_row[k]]);
    const std::string& h = ref.names[ref_row[k]];
    const size_t b = h.find_first_not_of(" \t\n\v\f\r"), e = h.find_first_of(" \t\n\v\f\r", b);
    row_names.push_back(b == std::string::npos ? std::string() : h.substr(b, e == std::string::npos ? e : e - b));
  }
  const uint32_t len_r = (uint32_t)rr[0].size(), len_t = (uint32_t)tr[0].size();
  const std::vector<uint8_t> cell_r = cells_of(rr), cell_t = cells_of(tr);
  std::vector<uint8_t> classes;
  if (pp) {
    classes.assign((size_t)n * len_t, 255);
    const std::string chars = "0123456789*";
    for (uint32_t k = 0; k < n; ++k) {
      const std::string& line = (*pp)[test_row[k]];
      for (size_t c = 0; c < line.size() && c < len_t; ++c) {
        const size_t q = chars.find(line[c]);
        if (q != std::string::npos) classes[(size_t)k * len_t + c] = (uint8_t)q;
      }
    }
  }
  std::vector<uint32_t> residues(n), kc(len_r), md(len_t), ps, pr, pt;
  std::vector<uint64_t> shared(n), refp(n), testp(n), total(3), tc(2), colref(len_r), colshared(len_r), tp(n), nref(n), ntest(n), pp_count(33);
  std::vector<uint8_t> reproduced(len_r);
  if (matrix) {
    ps.resize((size_t)n * n);
    pr.resize((size_t)n * n);
    pt.resize((size_t)n * n);
  }
  dafs_compare_out c;
  memset(&c, 0, sizeof c);
  c.residues = residues.data(); c.shared = shared.data(); c.refp = refp.data(); c.testp = testp.data();
  c.total = total.data(); c.tc = tc.data(); c.k = kc.data(); c.m = md.data();
  c.colref = colref.data(); c.colshared = colshared.data(); c.reproduced = reproduced.data();
  if (matrix) { c.pair_shared = ps.data(); c.pair_refp = pr.data(); c.pair_testp = pt.data(); }
  if (pp) c.pp_count = pp_count.data();
  if (both) { c.tp = tp.data(); c.nref = nref.data(); c.ntest = ntest.data(); }
  check_text(dafs_hip_alignment_compare(ctx, n, len_r, len_t, cell_r.data(), cell_t.data(), nullptr, use, both ? ref.ss.data() : nullptr,
                                        both ? ss->data() : nullptr, pp ? classes.data() : nullptr, &c));
  char* text = nullptr;
  check_text(dafs_host_compare_table(n, c_strs(row_names).data(), nr - n, nt - n, len_r, len_t, residues.data(), shared.data(), refp.data(),
                                     testp.data(), total.data(), tc.data(), both ? tp.data() : nullptr, both ? nref.data() : nullptr,
                                     both ? ntest.data() : nullptr, pp ? pp_count.data() : nullptr, &text));
  out.table = take(text);
  check_text(dafs_host_compare_columns_table(len_r, kc.data(), colref.data(), colshared.data(), reproduced.data(), &text));
  out.columns = take(text);
  if (matrix) {
    check_text(dafs_host_compare_matrix_table(n, c_strs(row_names).data(), ps.data(), pr.data(), pt.data(), &text));
    out.matrix = take(text);
  }
}

void write_compare(const Options& o, const std::vector<CompareText>& cmp, const std::vector<std::string>* headers) {
  std::vector<std::string> tables, columns, matrices;
  for (const CompareText& t : cmp) { tables.push_back(t.table); columns.push_back(t.columns); matrices.push_back(t.matrix); }
  write_tables("--compare", o.compare, tables, headers);
  if (!o.compare_columns.empty()) write_tables("--compare-columns", o.compare_columns, columns, headers);
  if (!o.compare_matrix.empty()) write_tables("--compare-matrix", o.compare_matrix, matrices, headers);
}

// Everything one family (an input file, a cluster, a pair, a placement) produces: its text, printed as it is made or kept for
// the block the run prints later, and the side outputs that are wanted of it
enum : unsigned { kSto = 1, kCov = 2, kIdt = 4, kCmp = 8, kPhy = 16 };  // --stockholm, --covariation, --identity, --compare, --phylogeny

struct FamilyOut {
  unsigned wanted = 0;
  std::ostringstream text;
  std::ostream* os = &text;  // &text, or &std::cout
  std::string sto, cov, phy, phy_table, auto_table;
  IdentityText idt;
  CompareText cmp;
  FamilyOut() {}
  FamilyOut(const FamilyOut&) = delete;  // os points into the record
};

std::vector<FamilyOut> records(size_t n, unsigned wanted) {
  std::vector<FamilyOut> recs(n);
  for (FamilyOut& r : recs) r.wanted = wanted;
  return recs;
}

// the side outputs the options ask for; a mode that does not produce one of them clears its flag
unsigned wanted_of(const Options& o) {
  return (o.stockholm.empty() ? 0 : kSto) | (o.covariation.empty() ? 0 : kCov) | (o.identity.empty() ? 0 : kIdt) | (o.compare.empty() ? 0 : kCmp) |
         (o.phylogeny.empty() ? 0 : kPhy);
}

// The files of the wanted side outputs, one block or table per record in order; headers: a line "==> header <==" before every
// record's table (the Stockholm blocks carry none)
void write_outputs(const Options& o, unsigned wanted, const std::vector<FamilyOut>& recs, const std::vector<std::string>* headers) {
  std::vector<std::string> sto, cov, phy, phy_table;
  std::vector<IdentityText> idt;
  std::vector<CompareText> cmp;
  for (const FamilyOut& r : recs) { sto.push_back(r.sto); cov.push_back(r.cov); idt.push_back(r.idt); cmp.push_back(r.cmp); phy.push_back(r.phy); phy_table.push_back(r.phy_table); }
  if (wanted & kSto) write_tables("--stockholm", o.stockholm, sto, nullptr);
  if (wanted & kCov) write_tables("--covariation", o.covariation, cov, headers);
  if (wanted & kIdt) write_identity(o, idt, headers);
  if (wanted & kPhy) write_tables("--phylogeny", o.phylogeny, phy, headers);
  if ((wanted & kPhy) && !o.phylogeny_support.empty()) write_tables("--phylogeny-support", o.phylogeny_support, phy_table, headers);
  if (wanted & kCmp) write_compare(o, cmp, headers);
  if (!o.auto_table.empty()) {
    std::vector<std::string> tables;
    for (const FamilyOut& r : recs) tables.push_back(r.auto_table);
    write_tables("--fold-auto-table", o.auto_table, tables, headers);
  }
}

// ---------------------------------------------------------------------------------------------
// --seed: the seed alignment, read (Stockholm, or aligned FASTA as this program prints it) and checked
// by the library: names and rows without their all-gap columns, '-' for every gap
// ss (--seed-structure): also the seed's consensus structure over the cleaned columns; a seed without
// one is refused
// describe (--describe): the structure is optional -- without one ss comes back with every column unpaired
// level (--knots, with ss): the structure may cross, and *level receives its pairs' levels (empty when the file has no structure)
void read_seed(const std::string& file, std::vector<std::string>& names, std::vector<std::string>& rows, VU* ss = nullptr, bool describe = false,
               VL* level = nullptr) {
  std::ifstream is(file.c_str(), std::ios::binary);
  if (!is.is_open()) throw (describe ? "--describe: cannot open " : "--seed: cannot open ") + file;
  const std::string text((std::istreambuf_iterator<char>(is)), std::istreambuf_iterator<char>());
  uint32_t n = 0;
  char *nm = nullptr, *rw = nullptr, *st = nullptr;
  if (!ss) {
    check_text(dafs_host_seed_parse(text.data(), text.size(), &n, &nm, &rw));
    names = lines_of(take(nm), n);
    rows = lines_of(take(rw), n);
    check_text(dafs_host_seed_clean(n, c_strs(names).data(), c_strs(rows).data(), &rw));
    rows = lines_of(take(rw), n);
    return;
  }
  int has = 0;
  check_text(dafs_host_seed_parse_structure(text.data(), text.size(), &n, &has, &nm, &rw, &st));
  names = lines_of(take(nm), n);
  rows = lines_of(take(rw), n);
  const std::string structure = take(st);
  if (!has && describe) {
    check_text(dafs_host_seed_clean(n, c_strs(names).data(), c_strs(rows).data(), &rw));
    rows = lines_of(take(rw), n);
    ss->assign(rows[0].size(), DAFS_HIP_NONE);
    return;
  }
  if (!has) throw "--seed-structure: " + file + " holds no SS_cons";
  ss->assign(rows.empty() ? 1 : rows[0].size() + 1, DAFS_HIP_NONE);
  uint32_t columns = 0;
  if (level) {
    level->assign(ss->size(), 0xFF);
    check_text(dafs_host_seed_clean_structure_levels(n, c_strs(names).data(), c_strs(rows).data(), structure.c_str(), ss->data(), level->data(),
                                                     &columns, &rw));
    level->resize(columns);
  } else {
    check_text(dafs_host_seed_clean_structure(n, c_strs(names).data(), c_strs(rows).data(), structure.c_str(), ss->data(), &columns, &rw));
  }
  rows = lines_of(take(rw), n);
  ss->resize(columns);
}

// The seed of a run: its m rows over C columns as read_seed returns them, with --seed-structure its structure, and the rows
// taken apart into the ungapped sequences and the row-major mask of the cells that hold a residue
struct Seed {
  std::vector<std::string> names, rows;
  VU ss;
  VL level;            // --knots: the levels of ss's pairs, else empty
  uint32_t nlevels = 1;  // the levels in use
  std::vector<Fasta> fa;
  std::vector<uint8_t> mask;
  std::vector<uint32_t> lens;
  uint32_t m = 0, C = 0;
};

Seed load_seed(const Options& o) {
  Seed sd;
  read_seed(o.seed, sd.names, sd.rows, o.seed_structure ? &sd.ss : nullptr, false, o.seed_structure && o.knots ? &sd.level : nullptr);
  for (uint8_t lv : sd.level)
    if (lv != 0xFF) sd.nlevels = std::max(sd.nlevels, (uint32_t)lv + 1);
  sd.m = (uint32_t)sd.rows.size();
  sd.C = (uint32_t)sd.rows[0].size();
  sd.mask.assign((size_t)sd.m * sd.C, 0);
  for (uint32_t r = 0; r < sd.m; ++r) {
    std::string sq;
    for (uint32_t c = 0; c < sd.C; ++c)
      if (sd.rows[r][c] != '-') { sq += sd.rows[r][c]; sd.mask[(size_t)r * sd.C + c] = 1; }
    sd.fa.push_back(Fasta(sd.names[r], sq));
    sd.lens.push_back((uint32_t)sq.size());
  }
  return sd;
}

// --seed-structure: the folding constraints of a context that holds the seed's sequences and then k new ones -- every seed row
// under the seed's structure (dafs_host_row_constraint), nullptr (a free fold) for the new ones.  Without --seed-structure, empty.
// --knots: nlevels entries per sequence (dafs_host_row_constraint_levels), for dafs_hip_fold_posteriors_levels_begin.
struct Constraints {
  std::vector<std::string> text;
  std::vector<const char*> ptr;  // into text
  uint32_t nlevels = 0;          // --knots: the entries per sequence; 0: one, the plain call
  Constraints() {}
  Constraints(const Constraints&) = delete;
  Constraints(Constraints&&) = default;  // a moved vector keeps its strings where they are
};

Constraints seed_constraints(const Options& o, const Seed& sd, uint32_t k) {
  Constraints out;
  if (!o.seed_structure) return out;
  if (o.knots) {
    out.nlevels = sd.nlevels;
    for (uint32_t r = 0; r < sd.m; ++r) {
      const size_t stride = (size_t)sd.lens[r] + 1;
      std::vector<char> buf(stride * sd.nlevels);
      check(dafs_host_row_constraint_levels(sd.C, sd.mask.data() + (size_t)r * sd.C, sd.ss.data(), sd.level.data(), sd.nlevels,
                                            sd.fa[r].seq().c_str(), buf.data()));
      for (uint32_t lv = 0; lv < sd.nlevels; ++lv) out.text.push_back(buf.data() + lv * stride);
    }
    for (const std::string& s : out.text) out.ptr.push_back(s.c_str());
    out.ptr.resize((size_t)(sd.m + k) * sd.nlevels, nullptr);
    return out;
  }
  for (uint32_t r = 0; r < sd.m; ++r) {
    std::vector<char> buf(sd.lens[r] + 1);
    check(dafs_host_row_constraint(sd.C, sd.mask.data() + (size_t)r * sd.C, sd.ss.data(), sd.fa[r].seq().c_str(), buf.data()));
    out.text.push_back(buf.data());
  }
  for (const std::string& s : out.text) out.ptr.push_back(s.c_str());
  out.ptr.resize(sd.m + k, nullptr);
  return out;
}

// the seed's structure in the merged columns: insert columns unpaired
VU carry_structure(const VU& ss, const std::vector<uint32_t>& seed_col, uint32_t width) {
  VU out(width, DAFS_HIP_NONE);
  for (size_t c = 0; c < ss.size(); ++c)
    if (ss[c] != DAFS_HIP_NONE) out[seed_col[c]] = seed_col[ss[c]];
  return out;
}

// the levels of the seed's pairs in the merged columns (--knots; empty without): 0xFF at insert columns
VL carry_levels(const VL& level, const std::vector<uint32_t>& seed_col, uint32_t width) {
  if (level.empty()) return VL();
  VL out(width, 0xFF);
  for (size_t c = 0; c < level.size(); ++c) out[seed_col[c]] = level[c];
  return out;
}

// Where dafs_host_merge_added places k new sequences (lens; zs: each one's map onto the seed's columns, from its node) into
// the seed: the merged column of every seed column and of every new residue (one sequence after another), the merged width,
// and the RF mask (1: a seed column)
struct Placement {
  std::vector<uint32_t> seed_col, res_col;
  uint32_t width = 0;
  std::vector<uint8_t> rf;
};

Placement place(const Seed& sd, uint32_t k, const uint32_t* lens, const VU* zs) {
  Placement p;
  std::vector<uint32_t> z;
  for (uint32_t j = 0; j < k; ++j) z.insert(z.end(), zs[j].begin(), zs[j].end());
  p.seed_col.resize(sd.C);
  p.res_col.resize(z.size() ? z.size() : 1);
  check(dafs_host_merge_added(sd.C, k, lens, z.data(), p.seed_col.data(), p.res_col.data(), &p.width));
  p.rf.assign(p.width, 0);
  for (uint32_t c = 0; c < sd.C; ++c) p.rf[p.seed_col[c]] = 1;
  return p;
}

// the placed alignment: the k new rows (sequences new_first, new_first + 1, ...), then the seed rows (seed_first, ...)
ALN placed_rows(const Seed& sd, const Placement& p, uint32_t k, const uint32_t* lens, uint32_t new_first, uint32_t seed_first) {
  ALN aln;
  for (uint32_t j = 0, off = 0; j < k; off += lens[j], ++j) {
    std::vector<bool> msk(p.width, false);
    for (uint32_t i = 0; i < lens[j]; ++i) msk[p.res_col[off + i]] = true;
    aln.push_back(std::make_pair(new_first + j, msk));
  }
  for (uint32_t r = 0; r < sd.m; ++r) {
    std::vector<bool> msk(p.width, false);
    for (uint32_t c = 0; c < sd.C; ++c) msk[p.seed_col[c]] = sd.mask[(size_t)r * sd.C + c] != 0;
    aln.push_back(std::make_pair(seed_first + r, msk));
  }
  return aln;
}

// ---------------------------------------------------------------------------------------------
// --devices: the ranks of phase 1, one process per listed GPU.  The processes are forked before the first GPU call of
// the program (a process that has initialised the GPU must neither fork nor exec); rank 0 is the original process and
// the only one that goes on after phase 1.  What the ranks share is one anonymous mapping made before the fork.
struct RankShared {
  pthread_barrier_t barrier;
  ncclUniqueId nccl_id;  // written by rank 0, read by the others after a barrier
};

volatile sig_atomic_t g_child_count = 0;
pid_t g_child_pid[64];
volatile sig_atomic_t g_child_gone[64];

void on_sigchld(int) {  // a rank that fails takes the run down instead of leaving the others in a collective
  for (int k = 0; k < g_child_count; ++k) {
    if (g_child_gone[k]) continue;
    int st = 0;
    if (waitpid(g_child_pid[k], &st, WNOHANG) != g_child_pid[k]) continue;
    g_child_gone[k] = 1;
    if (!(WIFEXITED(st) && WEXITSTATUS(st) == 0)) {
      static const char msg[] = "dafs: a rank of --devices failed\n";
      if (write(2, msg, sizeof msg - 1) < 0) {}
      _exit(EXIT_FAILURE);  // the remaining ranks die with their parent (PR_SET_PDEATHSIG)
    }
  }
}

struct Ranks {
  uint32_t rank = 0, world = 1;
  RankShared* shared = nullptr;
  uint8_t* stage = nullptr;  // host staging area (only when a device is listed more than once)
  size_t stage_bytes = 0;
  void* lib = nullptr;
  ncclComm_t comm = nullptr;
  decltype(&ncclGetUniqueId) get_id = nullptr;
  decltype(&ncclCommInitRank) comm_init = nullptr;
  decltype(&ncclAllGather) all_gather = nullptr;
  decltype(&ncclCommDestroy) comm_destroy = nullptr;
  decltype(&ncclGetErrorString) err_string = nullptr;

  void fork_ranks(const std::vector<int>& devices) {
    world = (uint32_t)devices.size();
    if (world > 64) throw std::string("--devices: at most 64 devices");
    bool repeated = false;
    for (size_t a = 0; a < devices.size(); ++a)
      for (size_t b = 0; b < a; ++b) repeated |= devices[a] == devices[b];
    // RCCL refuses two ranks on one device; such a list (a rehearsal of the multi-process path on a single GPU) exchanges
    // its shards through a host staging area instead.  Untouched pages of the mapping cost nothing.
    if (repeated) stage_bytes = (size_t)sysconf(_SC_PHYS_PAGES) * (size_t)sysconf(_SC_PAGE_SIZE) / 4;
    const size_t head = 4096;
    static_assert(sizeof(RankShared) <= 4096, "the header page");
    void* m = mmap(nullptr, head + stage_bytes, PROT_READ | PROT_WRITE, MAP_SHARED | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
    if (m == MAP_FAILED) throw std::string("--devices: cannot map the shared area");
    shared = (RankShared*)m;
    stage = (uint8_t*)m + head;
    pthread_barrierattr_t at;
    pthread_barrierattr_init(&at);
    pthread_barrierattr_setpshared(&at, PTHREAD_PROCESS_SHARED);
    pthread_barrier_init(&shared->barrier, &at, world);
    std::cout.flush();
    std::cerr.flush();
    const pid_t parent = getpid();
    for (uint32_t r = 1; r < world; ++r) {
      const pid_t pid = fork();
      if (pid < 0) throw std::string("--devices: fork failed");
      if (pid == 0) {
        prctl(PR_SET_PDEATHSIG, SIGKILL);
        if (getppid() != parent) _exit(EXIT_FAILURE);  // the parent died before the prctl
        rank = r;
        g_child_count = 0;
        return;
      }
      g_child_pid[r - 1] = pid;
      g_child_gone[r - 1] = 0;
      g_child_count = (sig_atomic_t)r;
    }
    struct sigaction sa;
    memset(&sa, 0, sizeof sa);
    sa.sa_handler = on_sigchld;
    sa.sa_flags = SA_RESTART | SA_NOCLDSTOP;
    sigaction(SIGCHLD, &sa, nullptr);
    on_sigchld(0);  // a rank that died before the handler was in place
  }

  void barrier() { if (world > 1) pthread_barrier_wait(&shared->barrier); }

  void connect() {  // after dafs_hip_create: the communicator belongs to the context's device
    if (stage_bytes) return;
    lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!lib) throw std::string("--devices: cannot load librccl.so.1: ") + dlerror();
    get_id = (decltype(get_id))dlsym(lib, "ncclGetUniqueId");
    comm_init = (decltype(comm_init))dlsym(lib, "ncclCommInitRank");
    all_gather = (decltype(all_gather))dlsym(lib, "ncclAllGather");
    comm_destroy = (decltype(comm_destroy))dlsym(lib, "ncclCommDestroy");
    err_string = (decltype(err_string))dlsym(lib, "ncclGetErrorString");
    if (!get_id || !comm_init || !all_gather || !comm_destroy || !err_string) throw std::string("--devices: librccl.so.1 lacks an entry point");
    // RCCL announces itself on stdout when the communicator is made (version, host, library path): this program's
    // stdout is its result, so that goes to stderr
    std::cout.flush();
    fflush(stdout);
    const int keep = dup(1);
    if (keep >= 0) dup2(2, 1);
    ncclResult_t r0 = ncclSuccess, r1 = ncclSuccess;
    if (rank == 0) r0 = get_id(&shared->nccl_id);
    barrier();
    if (r0 == ncclSuccess) r1 = comm_init(&comm, (int)world, shared->nccl_id, (int)rank);
    fflush(stdout);
    if (keep >= 0) { dup2(keep, 1); close(keep); }
    nccl(r0);
    nccl(r1);
  }
  void disconnect() {
    if (comm) { comm_destroy(comm); comm = nullptr; }
  }
  void nccl(ncclResult_t r) {
    if (r != ncclSuccess) throw std::string("RCCL: ") + err_string(r);
  }
  void wait_ranks() {  // rank 0, at the end: every rank has left without an error
    sigset_t block, old;
    sigemptyset(&block);
    sigaddset(&block, SIGCHLD);
    sigprocmask(SIG_BLOCK, &block, &old);
    bool bad = false;
    for (int k = 0; k < g_child_count; ++k) {
      if (g_child_gone[k]) continue;
      int st = 0;
      if (waitpid(g_child_pid[k], &st, 0) == g_child_pid[k]) bad |= !(WIFEXITED(st) && WEXITSTATUS(st) == 0);
      g_child_gone[k] = 1;
    }
    sigprocmask(SIG_SETMASK, &old, nullptr);
    if (bad) throw std::string("a rank of --devices failed");
  }
};

// dafs_allgather_fn: ncclAllGather on the stream the library names; between two ranks of one device, host staging
int rank_allgather(void* user, const void* send, void* recv, size_t bytes, void* stream) {
  Ranks* rk = (Ranks*)user;
  if (rk->comm) {
    const ncclResult_t r = rk->all_gather(send, recv, bytes, ncclChar, rk->comm, (hipStream_t)stream);
    if (r != ncclSuccess) std::cerr << "RCCL: " << rk->err_string(r) << std::endl;
    return r == ncclSuccess ? 0 : 1;
  }
  if (bytes * rk->world > rk->stage_bytes) {
    std::cerr << "--devices: the host staging area is too small for " << bytes << " bytes per rank" << std::endl;
    return 1;
  }
  if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return 1;
  if (hipMemcpy(rk->stage + (size_t)rk->rank * bytes, send, bytes, hipMemcpyDeviceToHost) != hipSuccess) return 1;
  rk->barrier();
  if (hipMemcpy(recv, rk->stage, (size_t)rk->world * bytes, hipMemcpyHostToDevice) != hipSuccess) return 1;
  rk->barrier();  // nobody overwrites the area before everybody has read it
  return 0;
}

// --pairwise: the pairs of one chunk, whose two-sequence families a run of align_group gathers from the source context of
// the N sequences (dafs_hip_pairs_from) instead of computing its phase-1 inputs; per family its root node's score and
// iteration count come back in score / iterations
struct PairChunk {
  const dafs_hip_ctx* src = nullptr;
  std::vector<uint32_t> px, py;
  std::vector<float> score;
  std::vector<uint32_t> iterations;
};

struct Guard {  // the context of a run, destroyed however the run ends
  dafs_hip_ctx* c;
  ~Guard() { dafs_hip_destroy(c); }
};

void set_sequences(dafs_hip_ctx* ctx, const std::vector<Fasta>& fa) {
  std::vector<const char*> seqs;
  std::vector<uint32_t> lens;
  for (const Fasta& s : fa) { seqs.push_back(s.seq().c_str()); lens.push_back(s.size()); }
  check(dafs_hip_set_sequences(ctx, (uint32_t)fa.size(), seqs.data(), lens.data()));
}

// Phase 1 on this process (:1787-1827; the twin of pipeline._phase1_local) over the context's sequences fa, families
// [first[f], first[f + 1]): base-pairing probabilities (computed, or --fold-aux), and with two or more sequences the matching
// probabilities (computed, or --align-aux), -f, the similarity blocks into sim (one n x n block per family, one after
// another) and both consistency transforms.  The device folding is only started at the beginning: it keeps one workgroup
// per sequence busy, and the alignment posteriors and the matching-probability transform run beside it.
void phase1_local(dafs_hip_ctx* ctx, const Options& o, int align_model, const std::vector<Fasta>& fa, const std::vector<uint32_t>& first,
                  std::vector<float>& sim, const PairChunk* pc = nullptr, const std::vector<const char*>* constraints = nullptr,
                  uint32_t cons_levels = 0) {
  const uint N = (uint)fa.size(), F = (uint)first.size() - 1;
  bool folding = false;
  if (pc) {  // --pairwise: both raw stores and the similarity blocks gathered from the N-sequence source
    check(dafs_hip_pairs_from(ctx, pc->src, (uint32_t)pc->px.size(), pc->px.data(), pc->py.data()));
  } else if (!o.fold_aux.empty()) {
    std::vector<BP> bp;
    load_fold_aux(o.fold_aux, fa, bp);
    upload_bp(ctx, bp);
  } else if (constraints && cons_levels) {  // --knots: cons_levels constraints per sequence, the folds merged by _end
    check(dafs_hip_fold_posteriors_levels_begin(ctx, DAFS_FOLD_CONTRAFOLD, kCutoff, cons_levels, constraints->data()));
    folding = true;
  } else {  // constraints: per sequence its folding constraint, nullptr for a free fold (--seed-structure)
    check(dafs_hip_fold_posteriors_constrained_begin(ctx, DAFS_FOLD_CONTRAFOLD, kCutoff, constraints ? constraints->data() : nullptr));
    folding = true;
  }
  bool fold_saved = false;
  auto finish_folding = [&]() {
    if (folding) { check(dafs_hip_fold_posteriors_end(ctx)); folding = false; }
    if (!o.save_fold_aux.empty() && !fold_saved) { save_fold_aux(ctx, o.save_fold_aux, fa); fold_saved = true; }
  };
  if (N == 1) {
    finish_folding();
    return;
  }
  // matching probabilities, transposes, similarities (:1796-1819), PCTs (:1822-1827)
  if (pc) {}  // gathered by dafs_hip_pairs_from above
  else if (!o.align_aux.empty()) load_align_aux(ctx, o.align_aux, fa);
  else check(dafs_hip_align_posteriors(ctx, align_model, o.align_th, 0, 0));
  if (!o.save_align_aux.empty()) save_align_aux(ctx, o.save_align_aux, fa);
  if (o.fourway != 0.0f) {  // relax_fourway_consistency (:1808-1809): needs the base-pairing rows, replaces mp_ before sim_
    finish_folding();
    check(dafs_hip_fourway_consistency(ctx, o.fourway));
  }
  size_t sim_floats = 0;
  for (uint f = 0; f < F; ++f) sim_floats += (size_t)(first[f + 1] - first[f]) * (first[f + 1] - first[f]);
  sim.assign(sim_floats, 0.0f);
  check(dafs_hip_get_sim(ctx, sim.data()));
  check(dafs_hip_consistency_match(ctx, o.align_pct));
  finish_folding();
  check(dafs_hip_consistency_bp(ctx, o.fold_pct));
}

// the node parameters of the options (-w, --eta, -u, -t, -m)
dafs_dd_params dd_params_of(const Options& o) {
  dafs_dd_params prm;
  dafs_hip_dd_default_params(&prm);
  prm.w = o.w; prm.eta0 = o.eta; prm.th_a = o.align_th; prm.th_s = *std::min_element(o.fold_th.begin(), o.fold_th.end());
  prm.t_max = (uint32_t)o.max_iter;
  return prm;
}

// Many alignments as the library's batched calls take them: per alignment its rows and columns, then every alignment's
// sequence indices and row-major mask, one alignment after another
struct Packed {
  std::vector<uint32_t> n_rows, len, seq;
  std::vector<uint8_t> mask;
};

Packed pack(const std::vector<const ALN*>& alns) {
  Packed p;
  std::vector<uint32_t> rs;
  std::vector<uint8_t> rm;
  for (const ALN* a : alns) {
    flatten(*a, rs, rm);
    p.n_rows.push_back((uint32_t)a->size());
    p.len.push_back((uint32_t)(*a)[0].second.size());
    p.seq.insert(p.seq.end(), rs.begin(), rs.end());
    p.mask.insert(p.mask.end(), rm.begin(), rm.end());
  }
  return p;
}

// where each part of a flat result begins: part k of these lengths is [at[k], at[k + 1])
std::vector<size_t> starts_of(const std::vector<uint32_t>& len) {
  std::vector<size_t> at(1, 0);
  for (uint32_t l : len) at.push_back(at.back() + l);
  return at;
}

VU concat(const std::vector<VU>& parts) {
  VU all;
  for (const VU& p : parts) all.insert(all.end(), p.begin(), p.end());
  return all;
}

// Every decode of the command line goes through here: many alignments, laid out as the library takes them, at the decoder
// of --fold-decoder.  Nussinov: dafs_hip_consensus_structures at the first entry of -T / -G; level stays empty.  Levels:
// dafs_hip_consensus_structures_levels with one level per entry; level gets a byte per column.
// -T auto / -G auto: dafs_hip_consensus_structures_auto over the candidates of --auto-gammas, one level
// under Nussinov and up to one per entry under Levels; autos (optional) gets what every alignment's choice kept.
struct AutoInfo {
  uint32_t columns = 0;
  uint64_t sum_p = 0;
  std::vector<uint32_t> chosen, npairs, cand_pairs;  // [K], [K], [K * C]
  std::vector<uint64_t> tp, cand_tp;                 // [K], [K * C]
};

void decode_alignments(dafs_hip_ctx* ctx, const Options& o, const std::vector<uint32_t>& n_rows, const std::vector<uint32_t>& len,
                       const std::vector<uint32_t>& seq, const std::vector<uint8_t>& mask, VU& ss, VL& level, std::vector<AutoInfo>* autos = nullptr) {
  level.clear();
  if (o.auto_levels) {
    const size_t n = n_rows.size(), K = o.auto_levels, C = o.auto_cand.size();
    std::vector<uint32_t> chosen(n * K + 1), np(n * K + 1), cnp(n * K * C + 1);
    std::vector<uint64_t> sum(n + 1), tp(n * K + 1), ctp(n * K * C + 1);
    VL lv(ss.size(), 0xFF);
    check(dafs_hip_consensus_structures_auto(ctx, (uint32_t)n, n_rows.data(), len.data(), seq.data(), mask.data(), (uint32_t)K, (uint32_t)C,
                                             o.auto_cand.data(), ss.data(), lv.data(), nullptr, chosen.data(), sum.data(), tp.data(), np.data(),
                                             ctp.data(), cnp.data()));
    if (o.fold_decoder == "Levels") level.swap(lv);
    if (autos) {
      autos->assign(n, AutoInfo());
      for (size_t a = 0; a < n; ++a) {
        AutoInfo& au = (*autos)[a];
        au.columns = len[a];
        au.sum_p = sum[a];
        au.chosen.assign(chosen.begin() + a * K, chosen.begin() + (a + 1) * K);
        au.npairs.assign(np.begin() + a * K, np.begin() + (a + 1) * K);
        au.tp.assign(tp.begin() + a * K, tp.begin() + (a + 1) * K);
        au.cand_pairs.assign(cnp.begin() + a * K * C, cnp.begin() + (a + 1) * K * C);
        au.cand_tp.assign(ctp.begin() + a * K * C, ctp.begin() + (a + 1) * K * C);
      }
    }
    return;
  }
  if (o.fold_decoder != "Levels") {
    check(dafs_hip_consensus_structures(ctx, (uint32_t)n_rows.size(), n_rows.data(), len.data(), seq.data(), mask.data(), o.fold_th1[0], ss.data(), nullptr));
    return;
  }
  level.assign(ss.size(), 0xFF);
  check(dafs_hip_consensus_structures_levels(ctx, (uint32_t)n_rows.size(), n_rows.data(), len.data(), seq.data(), mask.data(),
                                             (uint32_t)o.fold_th1.size(), o.fold_th1.data(), ss.data(), level.data(), nullptr));
}

// The first decode of many final alignments in one library call: ss[k] of *alns[k], decoded over the rows in the order each
// holds them; level[k]: its levels, or empty (decode_alignments)
// autos (optional): with -T auto / -G auto what every alignment's choice kept, else left empty
void consensus_structures(dafs_hip_ctx* ctx, const Options& o, const std::vector<const ALN*>& alns, std::vector<VU>& ss, std::vector<VL>& level,
                          std::vector<AutoInfo>* autos = nullptr) {
  const Packed p = pack(alns);
  const std::vector<size_t> at = starts_of(p.len);
  VU all(at.back() ? at.back() : 1);
  VL lv;
  decode_alignments(ctx, o, p.n_rows, p.len, p.seq, p.mask, all, lv, autos);
  ss.clear();
  level.assign(alns.size(), VL());
  for (size_t k = 0; k < alns.size(); ++k) {
    ss.push_back(VU(all.begin() + at[k], all.begin() + at[k + 1]));
    if (!lv.empty()) level[k].assign(lv.begin() + at[k], lv.begin() + at[k + 1]);
  }
}

// The structure support of every row of many alignments in one library call (dafs_hip_structure_support): the rows of *alns[0]
// in the order it holds them, then those of *alns[1], ...
void structure_support(dafs_hip_ctx* ctx, const std::vector<const ALN*>& alns, const std::vector<VU>& ss, std::vector<uint32_t>& both,
                       std::vector<uint32_t>& canonical, std::vector<uint32_t>& half, std::vector<double>& expected) {
  const Packed p = pack(alns);
  const VU all = concat(ss);
  both.assign(p.seq.size(), 0); canonical.assign(p.seq.size(), 0); half.assign(p.seq.size(), 0); expected.assign(p.seq.size(), 0.0);
  check(dafs_hip_structure_support(ctx, (uint32_t)alns.size(), p.n_rows.data(), p.len.data(), p.seq.data(), p.mask.data(), all.data(), both.data(),
                                   canonical.data(), half.data(), expected.data()));
}

// --row-structures: the structure of every sequence of the context alone -- its one-row alignment decoded from the base-pairing
// store the progressive phase read, at the threshold of SS_cons -- all in one library call; indexed by sequence
// (row_level: per sequence its levels, or empty: decode_alignments)
std::vector<VU> row_structures(dafs_hip_ctx* ctx, const Options& o, const std::vector<Fasta>& fa, std::vector<VL>& row_level) {
  std::vector<uint32_t> n_rows(fa.size(), 1), len, seqs;
  for (const Fasta& s : fa) {
    seqs.push_back((uint32_t)seqs.size());
    len.push_back((uint32_t)s.size());
  }
  const std::vector<size_t> at = starts_of(len);
  const std::vector<uint8_t> mask(at.back() ? at.back() : 1, 1);
  VU all(at.back() ? at.back() : 1);
  VL lv;
  decode_alignments(ctx, o, n_rows, len, seqs, mask, all, lv);
  std::vector<VU> out;
  row_level.assign(seqs.size(), VL());
  for (size_t k = 0; k < seqs.size(); ++k) {
    out.push_back(VU(all.begin() + at[k], all.begin() + at[k + 1]));
    if (!lv.empty()) row_level[k].assign(lv.begin() + at[k], lv.begin() + at[k + 1]);
  }
  return out;
}

// The common secondary structure of a final alignment (:1857-1871; no RNAalifold term here), decoded over the rows in the
// order root holds them.  ss0: the first decode of the alignment where the caller has it already (consensus_structures over
// many alignments); without it the alignment is decoded here, as a batch of one, and level gets its levels (or stays empty).
VU final_structure(dafs_hip_ctx* ctx, const Options& o, const ALN& root, const VU* ss0, VL* level = nullptr, AutoInfo* au = nullptr) {
  std::vector<uint32_t> rs;
  std::vector<uint8_t> rm;
  flatten(root, rs, rm);
  const uint32_t L = (uint32_t)root[0].second.size();
  VU ss(L);
  if (ss0) ss = *ss0;
  else {
    std::vector<VU> one;
    std::vector<VL> one_level;
    std::vector<AutoInfo> one_auto;
    consensus_structures(ctx, o, {&root}, one, one_level, &one_auto);
    ss = one[0];
    if (level) *level = one_level[0];
    if (au && !one_auto.empty()) *au = one_auto[0];
  }
  if (o.bp_update1) {  // :1863-1869: re-estimate under the decoded structure, decode again (SparseNussinov::decode(p, ss, str))
    std::vector<float> p((size_t)L * L);
    check(dafs_hip_update_basepairing(ctx, (uint32_t)root.size(), L, rs.data(), rm.data(), ss.data(), p.data()));
    check(dafs_hip_nussinov_decode(ctx, o.fold_th1[0], 0.0f, L, p.data(), nullptr, ss.data(), nullptr));
  }
  return ss;
}

// The reliabilities of many final alignments and their final structures in one library call (dafs_hip_alignment_reliabilities),
// from the stores the progressive phase read (with --bp-update1 too: ss is the re-decoded one).  fa: the context's sequences.
// first_row_only: only the first row of every alignment is wanted (the placed row of --seed-merged); col is NaN then.
struct Reliability {
  std::vector<double> rel, col;  // the residues of the rows in the order the alignment held them at the call; per column
};
void reliabilities(dafs_hip_ctx* ctx, const std::vector<Fasta>& fa, const std::vector<const ALN*>& alns, const std::vector<VU>& ss,
                   bool first_row_only, std::vector<Reliability>& out) {
  const Packed p = pack(alns);
  const VU all_ss = concat(ss);
  std::vector<uint8_t> want;
  std::vector<uint32_t> residues;  // per alignment, over its rows
  for (const ALN* a : alns) {
    residues.push_back(0);
    for (size_t r = 0; r < a->size(); ++r) {
      want.push_back(r == 0 || !first_row_only ? 1 : 0);
      residues.back() += fa[(*a)[r].first].size();
    }
  }
  const std::vector<size_t> at = starts_of(residues), col_at = starts_of(p.len);
  std::vector<double> rel(at.back() ? at.back() : 1), col(all_ss.size() ? all_ss.size() : 1);
  check(dafs_hip_alignment_reliabilities(ctx, (uint32_t)alns.size(), p.n_rows.data(), p.len.data(), p.seq.data(), p.mask.data(), all_ss.data(),
                                         first_row_only ? want.data() : nullptr, -1, -1, rel.data(), col.data(), nullptr, nullptr, nullptr));
  out.assign(alns.size(), Reliability());
  for (size_t k = 0; k < alns.size(); ++k) {
    out[k].rel.assign(rel.begin() + at[k], rel.begin() + at[k + 1]);
    out[k].col.assign(col.begin() + col_at[k], col.begin() + col_at[k + 1]);
  }
}

// the rows of an alignment as text: residues in their columns, '-' elsewhere
std::vector<std::string> row_texts(const std::vector<Fasta>& fa, const ALN& aln) {
  std::vector<std::string> rows;
  for (const auto& row : aln) {
    const std::string& sq = fa[row.first].seq();
    std::string text(row.second.size(), '-');
    for (uint j = 0, k = 0; j != row.second.size(); ++j)
      if (row.second[j]) text[j] = sq[k++];
    rows.push_back(text);
  }
  return rows;
}

// 2 T / (n 2^30 + S) for display; 0 for a zero denominator
double pseudo_f(uint64_t t, uint64_t n, uint64_t S) {
  const double den = (double)n * 1073741824.0 + (double)S;
  return den > 0.0 ? 2.0 * (double)t / den : 0.0;
}

// --fold-auto-table: the header line and one line per decoded (level, candidate) of one alignment
std::string auto_table_of(const Options& o, const AutoInfo& au, const std::string& name) {
  const size_t K = au.chosen.size(), C = o.auto_cand.size();
  char buf[256];
  snprintf(buf, sizeof buf, "# alignment %s columns %u sum_p %llu\n", name.c_str(), au.columns, (unsigned long long)au.sum_p);
  std::string out = buf;
  uint64_t t_low = 0, n_low = 0;
  for (size_t k = 0; k < K; ++k) {
    for (size_t c = 0; c < C; ++c) {
      const uint64_t t = au.cand_tp[k * C + c], n = au.cand_pairs[k * C + c];
      snprintf(buf, sizeof buf, "%zu\t%g\t%g\t%llu\t%llu\t%.6f\t%d\n", k, (double)o.auto_gammas[c], (double)o.auto_cand[c], (unsigned long long)n,
               (unsigned long long)t, pseudo_f(t_low + t, n_low + n, au.sum_p), au.chosen[k] == c ? 1 : 0);
      out += buf;
    }
    if (au.chosen[k] == DAFS_HIP_NONE) break;  // the higher levels were not decoded
    t_low += au.tp[k];
    n_low += au.npairs[k];
  }
  return out;
}

// the "#=GF CC SS_cons auto ..." line of a block, behind its other #=GF lines
std::string with_auto_line(const Options& o, const AutoInfo& au, const std::string& block) {
  std::string line = "#=GF CC SS_cons auto thresholds ";
  uint64_t t = 0, n = 0;
  bool any = false;
  char buf[64];
  for (size_t k = 0; k < au.chosen.size() && au.chosen[k] != DAFS_HIP_NONE; ++k) {
    snprintf(buf, sizeof buf, "%s%g", any ? "," : "", (double)o.auto_cand[au.chosen[k]]);
    line += buf;
    any = true;
    t += au.tp[k];
    n += au.npairs[k];
  }
  if (!any) line += "none";
  snprintf(buf, sizeof buf, " f %.6f\n", pseudo_f(t, n, au.sum_p));
  line += buf;
  size_t at = block.find('\n') + 1;  // behind "# STOCKHOLM 1.0"
  while (block.compare(at, 5, "#=GF ") == 0) at = block.find('\n', at) + 1;
  return block.substr(0, at) + line + block.substr(at);
}

// The output of a final alignment with its final structure ss_final (:1876-1879, :1584-1601) on *out.os: ">SS_cons", the
// brackets, then the rows sorted by sequence index.  fa: the context's sequences, the family's from index first on, one per
// row.  What out.wanted asks for goes into out: the family's Stockholm block from rl (reliabilities, made while root held its
// rows in the present order) with tree_line (nullptr: no CC line), rf (nullptr: no RF line) and row_ss (--row-structures,
// nullptr without: per sequence of the context its own structure, row_structures, written as the block's #=GR SS lines); the
// covariation table, whose cov_SS_cons line joins the block; the identity tables, whose weights join the block; the comparison.
void finish_alignment(dafs_hip_ctx* ctx, const Options& o, const std::vector<Fasta>& fa, ALN& root, uint32_t first, FamilyOut& out,
                      const std::string* tree_line, const std::vector<uint8_t>* rf, const VU& ss_final, const Reliability& rl,
                      const std::vector<VU>* row_ss, const VL* level = nullptr, const std::vector<VL>* row_level = nullptr,
                      const AutoInfo* au = nullptr) {
  // au: with -T auto / -G auto what the alignment's choice kept (--fold-auto-table, the block's "#=GF CC SS_cons auto" line)
  if (au && au->chosen.empty()) au = nullptr;
  // level, row_level: the levels of ss_final and of the rows' structures under --fold-decoder Levels (null or empty: one kind of bracket)
  const uint32_t L = (uint32_t)root[0].second.size();
  std::vector<char> str(L + 1);
  dafs_hip_make_brackets_levels(L, ss_final.data(), level && !level->empty() ? level->data() : nullptr, str.data());
  std::map<uint32_t, size_t> rel_at;  // sequence -> its first residue in rl.rel
  size_t tot = 0;
  for (const auto& row : root) { rel_at[row.first] = tot; tot += fa[row.first].size(); }

  // output (:1876-1879, :1584-1601)
  std::sort(root.begin(), root.end());
  std::ostream& os = *out.os;
  os << ">SS_cons" << std::endl << str.data() << std::endl;
  const std::vector<std::string> rows = row_texts(fa, root);
  for (size_t r = 0; r < root.size(); ++r) os << "> " << fa[root[r].first].name() << std::endl << rows[r] << std::endl;
  std::string cov_chars;
  if (out.wanted & kCov) covariation_of(ctx, o, rows, ss_final, out.cov, cov_chars);
  std::vector<std::string> names;  // the printed rows' Stockholm names
  if ((out.wanted & (kSto | kIdt | kCmp | kPhy)) || (au && !o.auto_table.empty())) {
    std::vector<std::string> headers;
    for (size_t i = 0; i < root.size(); ++i) headers.push_back(fa[first + i].name());
    const std::vector<std::string> all_names = stockholm_names(headers);
    for (const auto& row : root) names.push_back(all_names[row.first - first]);
  }
  if (au && !o.auto_table.empty()) out.auto_table = auto_table_of(o, *au, names[0]);
  if (out.wanted & kIdt) identity_of(ctx, names, rows, !o.identity_matrix.empty(), out.idt);
  if (out.wanted & kPhy) phylogeny_of(ctx, o, names, rows, out.phy, out.phy_table);
  if (out.wanted & kCmp) compare_of(ctx, o, names, rows, &ss_final, nullptr, nullptr, out.cmp);
  if (out.wanted & kSto) {
    char* text = nullptr;
    std::vector<const double*> rr;
    for (const auto& row : root) rr.push_back(rl.rel.data() + rel_at[row.first]);
    std::vector<std::string> rss;  // each row's own structure in the row's columns
    for (size_t r = 0; row_ss && r < root.size(); ++r) {
      const VU& own = (*row_ss)[root[r].first];
      std::vector<char> buf(own.size() + 1);
      const VL* own_level = row_level && !row_level->empty() && !(*row_level)[root[r].first].empty() ? &(*row_level)[root[r].first] : nullptr;
      dafs_hip_make_brackets_levels((uint32_t)own.size(), own.data(), own_level ? own_level->data() : nullptr, buf.data());
      std::string line(rows[r].size(), '.');
      for (size_t c = 0, k = 0; c < line.size(); ++c)
        if (rows[r][c] != '-') line[c] = buf[k++];
      rss.push_back(line);
    }
    check_text(dafs_host_stockholm_block_rows(tree_line ? tree_line->c_str() : nullptr, (uint32_t)rows.size(), (uint32_t)rl.col.size(),
                                              c_strs(names).data(), c_strs(rows).data(), rr.data(), rl.col.data(), str.data(),
                                              rf ? rf->data() : nullptr, (out.wanted & kCov) ? cov_chars.c_str() : nullptr,
                                              row_ss ? c_strs(rss).data() : nullptr, &text));
    out.sto = take(text);
    if (au) out.sto = with_auto_line(o, *au, out.sto);
    if (out.wanted & kIdt) {  // --identity: the sequence weights as #=GS WT lines
      check_text(dafs_host_stockholm_weights(out.sto.c_str(), (uint32_t)names.size(), c_strs(names).data(), out.idt.weight.data(), &text));
      out.sto = take(text);
    }
  }
}

// rand() as a process that has not called it yet sees it: glibc's default generator is the one initstate(1, state, 128)
// sets up, and rand() returns random()
struct FreshRand {
  random_data rd;
  char state[128];
  FreshRand() {
    memset(&rd, 0, sizeof rd);
    memset(state, 0, sizeof state);
    initstate_r(1, state, sizeof state, &rd);
  }
  int next() {
    int32_t r = 0;
    random_r(&rd, &r);
    return (int)r;
  }
};

// The run of one or more families (members: indices into fams) on the context: phase 1 once over all of them, one guide
// tree per family, the progressive phase over the forest (the ready nodes of every family share each round), then per
// family the refinement, the common structure and the output into its record out[k] (finish_alignment): the text on
// *out[k]->os, and what out[k]->wanted asks for -- the same of every family of a group -- of the family's Stockholm block,
// covariation table, identity tables and weights, and comparison.
int align_group(dafs_hip_ctx* ctx, const Options& o, Ranks& rk, int align_model, const std::vector<std::vector<Fasta> >& fams,
                const std::vector<size_t>& members, const std::vector<FamilyOut*>& out, PairChunk* pc = nullptr) {
  const uint F = (uint)members.size();
  const bool sto = (out[0]->wanted & kSto) != 0;
  std::vector<Fasta> fa;         // every sequence of the group, family after family
  std::vector<uint32_t> first(1, 0);
  for (size_t f : members) {
    fa.insert(fa.end(), fams[f].begin(), fams[f].end());
    first.push_back((uint32_t)fa.size());
  }
  const uint N = (uint)fa.size();
  if (!pc) {  // dafs_hip_pairs_from sets the sequences and families itself
    set_sequences(ctx, fa);
    if (F > 1) check(dafs_hip_set_families(ctx, F, first.data()));
  }

  const bool sharded = !o.devices.empty() && N > 1;
  if (!sharded && rk.rank != 0) return 0;  // a single sequence: nothing to share

  // per family its guide tree (a family of one sequence: the leaf alone)
  std::vector<std::vector<node_t> > trees(F, std::vector<node_t>(1, std::make_pair(0.0f, std::make_pair(-1u, -1u))));
  if (sharded) {
    // phase 1 (:1787-1827) on rk.world ranks: every rank ends with the complete stores, rank 0 goes on alone
    rk.connect();
    check(dafs_hip_phase1_sharded(ctx, rk.rank, rk.world, align_model, o.align_th, o.align_pct, o.fold_pct, DAFS_FOLD_CONTRAFOLD, kCutoff, rank_allgather, &rk));
    rk.disconnect();
    if (rk.rank != 0) return 0;
    if (!o.save_fold_aux.empty()) save_fold_aux(ctx, o.save_fold_aux, fa);
    if (!o.save_align_aux.empty()) save_align_aux(ctx, o.save_align_aux, fa);
    std::vector<float> sim((size_t)N * N);
    check(dafs_hip_get_sim(ctx, sim.data()));
    trees[0] = build_tree(sim, N);
  } else {
    std::vector<float> sim;
    phase1_local(ctx, o, align_model, fa, first, sim, pc);
    size_t blk = 0;  // the guide trees (:1830) from the families' similarity blocks; a single sequence has none
    for (uint f = 0; N > 1 && f < F; ++f) {
      const uint n = first[f + 1] - first[f];
      trees[f] = build_tree(std::vector<float>(sim.begin() + blk, sim.begin() + blk + (size_t)n * n), n);
      blk += (size_t)n * n;
    }
  }
  for (uint f = 0; f < F; ++f) {
    const std::vector<Fasta>& ff = fams[members[f]];
    print_tree(*out[f]->os, trees[f], ff, (int)trees[f].size() - 1);
    *out[f]->os << std::endl;
  }

  // progressive alignment (:1838): every node whose children are ready is solved in the same batch
  const dafs_dd_params prm = dd_params_of(o);
  // The progressive loop below uses the alignment of a node and nothing else (dafs.cpp:896-912), except that the
  // score of the root seeds the iterative refinement and -v prints every node's iteration count (:1292): without
  // either, nodes with no consensus base pair may leave out their folding DPs
  // (dafs_dd_params::skip_uncoupled_folds).  The refinement itself compares scores.
  dafs_dd_params prm_prog = prm;
  prm_prog.skip_uncoupled_folds = (o.refinement == 0 && o.verbose == 0) ? 1 : 0;
  // The forest of the families' guide trees, one node array: family f's node i is tbase[f] + i, its leaf i the sequence
  // first[f] + i.  A node is ready when both of its children are done, whatever its family; the ready nodes of every
  // family share each round (run_rounds).
  std::vector<size_t> tbase(F + 1, 0);
  for (uint f = 0; f < F; ++f) tbase[f + 1] = tbase[f] + trees[f].size();
  std::vector<ALN> aln(tbase[F]);
  std::vector<bool> done(tbase[F], false), opened(tbase[F], false);
  for (uint f = 0; f < F; ++f)
    for (uint i = 0; i < first[f + 1] - first[f]; ++i) {
      aln[tbase[f] + i].push_back(std::make_pair(first[f] + i, std::vector<bool>(fa[first[f] + i].size(), true)));
      done[tbase[f] + i] = true;
    }
  std::vector<float> score(F, 0.0f);
  run_rounds(ctx, prm_prog, o.verbose, [&]() {
    std::vector<std::pair<size_t, NodeJob> > ready;
    for (uint f = 0; f < F; ++f) {
      const std::vector<node_t>& tree = trees[f];
      const size_t tb = tbase[f];
      for (uint i = first[f + 1] - first[f]; i < tree.size(); ++i) {
        const size_t l = tb + tree[i].second.first, r = tb + tree[i].second.second;
        if (done[tb + i] || opened[tb + i] || !done[l] || !done[r]) continue;
        opened[tb + i] = true;
        ready.emplace_back(tb + i, NodeJob());
        NodeJob& j = ready.back().second;
        flatten(aln[l], j.s1, j.m1);
        flatten(aln[r], j.s2, j.m2);
        node_job(ctx, j, o.bp_update && i == tree.size() - 1, prm.th_s);  // --bp-update: the top call of the recursion
      }
    }
    return ready;
  }, [&](size_t g, NodeJob& j) {
    const uint f = (uint)(std::upper_bound(tbase.begin(), tbase.end(), g) - tbase.begin()) - 1;
    const node_t& nd = trees[f][g - tbase[f]];
    const size_t l = tbase[f] + nd.second.first, r = tbase[f] + nd.second.second;
    project_alignment(aln[g], aln[l], aln[r], j.z);
    done[g] = true;
    ALN().swap(aln[l]);
    ALN().swap(aln[r]);
    if (g == tbase[f + 1] - 1) {
      score[f] = j.out.score;
      if (pc) { pc->score[f] = j.out.score; pc->iterations[f] = j.out.iterations; }
    }
  });
  for (uint f = 0; f < F; ++f) {
    ALN& root = aln[tbase[f + 1] - 1];
    float s = score[f];
    // iterative refinement (:1841-1855, refine :1539-1576; rand() is unseeded there too).  The draws come from a generator
    // of the family's own in the state rand() has at the start of a process, so that they are those of a run of its own
    // whatever else in the process (other families, the runtime's threads) calls rand()
    FreshRand rng;
    for (int it = 0; it < o.refinement && root.size() > 1; ++it) {
      VU group[2];
      do {
        group[0].clear();
        group[1].clear();
        for (uint i = 0; i != root.size(); ++i) group[rng.next() % 2].push_back(i);
      } while (group[0].empty() || group[1].empty());
      ALN part[2];
      for (uint g = 0; g != 2; ++g) {
        const uint n = (uint)group[g].size(), L = (uint)root[group[g][0]].second.size();
        part[g].resize(n);
        for (uint j = 0; j != n; ++j) part[g][j].first = root[group[g][j]].first;
        for (uint k = 0; k != L; ++k) {
          bool gap = true;
          for (uint j = 0; j != n; ++j) gap &= !root[group[g][j]].second[k];
          if (!gap)
            for (uint j = 0; j != n; ++j) part[g][j].second.push_back(root[group[g][j]].second[k]);
        }
      }
      ALN merged;
      const float sc = solve_node(ctx, prm, part[0], part[1], merged, o.verbose, o.bp_update);
      if (sc > s) { s = sc; root.swap(merged); }
    }
  }
  // the first decode of every family's final alignment in one call; with --row-structures, every row's own structure in another
  std::vector<const ALN*> roots;
  for (uint f = 0; f < F; ++f) roots.push_back(&aln[tbase[f + 1] - 1]);
  std::vector<VU> ss0;
  std::vector<VL> level0, row_level;
  std::vector<AutoInfo> autos;
  consensus_structures(ctx, o, roots, ss0, level0, &autos);
  std::vector<VU> row_ss;
  if (o.row_structures && sto) row_ss = row_structures(ctx, o, fa, row_level);
  // the annotation of all of them in one call, once every structure is final (-r and --bp-update1 are behind it)
  for (uint f = 0; f < F; ++f) ss0[f] = final_structure(ctx, o, *roots[f], &ss0[f]);
  std::vector<Reliability> rl(F);
  if (sto) reliabilities(ctx, fa, roots, ss0, false, rl);
  for (uint f = 0; f < F; ++f) {
    std::string tree_line;
    if (sto) {
      std::ostringstream tl;
      print_tree(tl, trees[f], fams[members[f]], (int)trees[f].size() - 1);
      tree_line = tl.str();
    }
    finish_alignment(ctx, o, fa, aln[tbase[f + 1] - 1], first[f], *out[f], &tree_line, nullptr, ss0[f], rl[f], row_ss.empty() ? nullptr : &row_ss,
                     &level0[f], &row_level, autos.empty() ? nullptr : &autos[f]);
  }
  return 0;
}

// a family's block of a run that prints several: the header line, then the family's text, which is not kept
void print_block(const std::string& header, FamilyOut& rec) {
  std::cout << "==> " << header << " <==" << std::endl << rec.text.str();
  rec.text.str(std::string());
}

// One node per new sequence against the seed, all count of them opened in the first round (run_rounds): fill(j, job) sets job
// j's left side (the new sequence's leaf) and right side (the seed's rows); finish as run_rounds calls it.
void placement_rounds(dafs_hip_ctx* ctx, const dafs_dd_params& prm, int verbose, size_t count, const std::function<void(size_t, NodeJob&)>& fill,
                      const std::function<void(size_t, NodeJob&)>& finish) {
  bool opened = false;
  run_rounds(ctx, prm, verbose, [&]() {
    std::vector<std::pair<size_t, NodeJob> > ready(opened ? 0 : count);
    for (size_t j = 0; j < ready.size(); ++j) {
      ready[j].first = j;
      fill(j, ready[j].second);
      node_job(ctx, ready[j].second, false, prm.th_s);
    }
    opened = true;
    return ready;
  }, finish);
}

// `dafs --seed SEED FILE` (pipeline.add is the Python twin).  The context holds the seed's m sequences
// in seed order and then FILE's k.  Phase 1 is a normal run's over all of them; one node per new sequence j, its leaf (left)
// against the seed (right), and all k go through the resident-node rounds together (placement_rounds); place() puts them into
// the seed; the structure is decoded over the rows new sequences, then seed rows, as in a run whose tree joins a leaf last.
int run_add(const Options& o, int align_model) {
  const Seed sd = load_seed(o);
  std::vector<Fasta> added;
  Fasta::load(added, o.input.c_str());
  if (added.empty()) throw "no sequences in the input";
  const uint32_t m = sd.m, k = (uint32_t)added.size();
  std::vector<Fasta> fa(sd.fa);
  fa.insert(fa.end(), added.begin(), added.end());

  dafs_hip_ctx* ctx = nullptr;
  check(dafs_hip_create(o.device, &ctx));
  Guard guard{ctx};
  set_sequences(ctx, fa);
  std::vector<float> sim;
  const Constraints cons = seed_constraints(o, sd, k);
  phase1_local(ctx, o, align_model, fa, {0, m + k}, sim, nullptr, o.seed_structure ? &cons.ptr : nullptr, cons.nlevels);

  dafs_dd_params prm = dd_params_of(o);
  prm.skip_uncoupled_folds = o.verbose == 0 ? 1 : 0;  // as the progressive loop of a run without -r
  std::vector<uint32_t> seed_idx(m), lens(k);
  for (uint32_t r = 0; r < m; ++r) seed_idx[r] = r;
  for (uint32_t j = 0; j < k; ++j) lens[j] = added[j].size();
  std::vector<VU> zs(k);
  placement_rounds(ctx, prm, o.verbose, k, [&](size_t j, NodeJob& jb) {
    jb.s1.assign(1, m + (uint32_t)j);
    jb.m1.assign(lens[j], 1);
    jb.s2 = seed_idx;
    jb.m2 = sd.mask;
  }, [&](size_t j, NodeJob& jb) { zs[j].swap(jb.z); });

  // the rows new sequences (file order), then seed rows (seed order)
  const Placement pl = place(sd, k, lens.data(), zs.data());
  ALN root = placed_rows(sd, pl, k, lens.data(), m, 0);
  std::vector<FamilyOut> recs = records(1, wanted_of(o));
  recs[0].os = &std::cout;
  std::vector<VU> row_ss;
  std::vector<VL> row_level;
  if (o.row_structures) row_ss = row_structures(ctx, o, fa, row_level);
  VU carried;  // --seed-structure: nothing is decoded
  if (o.seed_structure) carried = carry_structure(sd.ss, pl.seed_col, pl.width);
  VL level;
  AutoInfo au;
  const VU ss = final_structure(ctx, o, root, o.seed_structure ? &carried : nullptr, &level, &au);
  if (o.seed_structure) level = carry_levels(sd.level, pl.seed_col, pl.width);
  std::vector<Reliability> rl(1);
  if (recs[0].wanted & kSto) reliabilities(ctx, fa, {&root}, {ss}, false, rl);
  finish_alignment(ctx, o, fa, root, 0, recs[0], nullptr, &pl.rf, ss, rl[0], o.row_structures ? &row_ss : nullptr, &level, &row_level, &au);
  std::cout.flush();
  write_outputs(o, recs[0].wanted, recs, nullptr);
  return 0;
}

// `dafs --seed SEED --seed-each FILE` (pipeline.add_each is the Python twin): every sequence of FILE added
// to the seed as run_add adds a file of that sequence alone.  Phase 1 runs once in a source context over the seed's m sequences
// and then FILE's k: the folds and the posteriors of the pairs with a seed sequence on the left, no transform.  The new
// sequences go in chunks under dafs_host_batch_bytes() (dafs_host_seed_each_bytes each) through a second context, where
// dafs_hip_families_from gathers the chunk's families seed + [new]; then the transforms -- the matching transform for the pairs
// (seed, new) alone unless --stockholm's reliabilities read the seed-seed rows --, one node per family in shared rounds,
// run_add's placement per family and the structures of the chunk in one call.  No identity output and no comparison per family.
// --seed-merged: the placements' maps are kept, and after the last chunk place() puts all k into the seed at once (DESIGN.md
// section 17).
int run_add_each(const Options& o, int align_model) {
  const Seed sd = load_seed(o);
  std::vector<Fasta> added;
  Fasta::load(added, o.input.c_str());
  if (added.empty()) throw "no sequences in the input";
  const uint32_t m = sd.m, k = (uint32_t)added.size(), C = sd.C, n = m + 1;
  std::vector<uint32_t> lens(k);
  for (uint32_t j = 0; j < k; ++j) lens[j] = added[j].size();

  dafs_hip_ctx* src = nullptr;
  check(dafs_hip_create(o.device, &src));
  Guard src_guard{src};
  {
    std::vector<Fasta> all(sd.fa);
    all.insert(all.end(), added.begin(), added.end());
    set_sequences(src, all);
  }
  {  // --seed-structure: the seed rows under their constraints, the new sequences free, once for every chunk
    const Constraints cons = seed_constraints(o, sd, k);
    if (cons.nlevels) check(dafs_hip_fold_posteriors_levels_begin(src, DAFS_FOLD_CONTRAFOLD, kCutoff, cons.nlevels, cons.ptr.data()));
    else check(dafs_hip_fold_posteriors_constrained_begin(src, DAFS_FOLD_CONTRAFOLD, kCutoff, o.seed_structure ? cons.ptr.data() : nullptr));
  }
  // the pairs (x, y) with x < m are the first m (m + k) - m (m + 1) / 2 pair ids
  const int rc_align = dafs_hip_align_posteriors(src, align_model, o.align_th, 0, (uint64_t)m * (m + k) - (uint64_t)m * (m + 1) / 2);
  const int rc_fold = dafs_hip_fold_posteriors_end(src);
  check(rc_align);
  check(rc_fold);
  dafs_hip_ctx* ctx = nullptr;
  check(dafs_hip_create(o.device, &ctx));
  Guard guard{ctx};

  std::vector<uint64_t> bytes(k);
  for (uint32_t j = 0; j < k; ++j) bytes[j] = dafs_host_seed_each_bytes(m, sd.lens.data(), C, lens[j]);
  dafs_dd_params prm = dd_params_of(o);
  prm.skip_uncoupled_folds = o.verbose == 0 ? 1 : 0;  // as run_add
  const unsigned wanted = wanted_of(o) & ~(kIdt | kCmp | kPhy);
  const bool listed = !(wanted & kSto) && o.align_pct != 0.0f;  // the reliabilities of --stockholm read the seed-seed rows
  std::vector<uint32_t> matched(k, 0);
  std::vector<double> score(k, 0.0);
  std::vector<int64_t> iterations(k, 0);
  std::vector<uint32_t> sup_both(k, 0), sup_can(k, 0), sup_half(k, 0);  // --seed-structure: the support of each new sequence's row
  std::vector<double> sup_exp(k, 0.0);
  std::vector<uint32_t> near_row(k, DAFS_HIP_NONE);  // --seed-nearest: per new sequence its nearest seed row and the identity to it
  std::vector<double> near_pid(k, std::nan(""));
  std::vector<FamilyOut> recs = records(k, wanted);  // one per new sequence
  std::vector<std::string> headers;
  for (uint32_t j = 0; j < k; ++j) headers.push_back(std::to_string(j + 1));
  std::vector<VU> all_z(k);                     // --seed-merged: every placement's map, kept until the last chunk is done,
  std::vector<std::vector<double> > new_pp(k);  // and the residue values of its row in its own family
  for (const auto& chunk : chunks(bytes)) {
    const uint32_t j0 = (uint32_t)chunk.first, nf = (uint32_t)(chunk.second - chunk.first);
    // family f: the seed's sequences at f n .. f n + m - 1, the new one at f n + m
    std::vector<uint32_t> first(nf + 1), member;
    std::vector<Fasta> fa;
    for (uint32_t f = 0; f < nf; ++f) {
      first[f] = f * n;
      for (uint32_t r = 0; r < m; ++r) member.push_back(r);
      member.push_back(m + j0 + f);
      fa.insert(fa.end(), sd.fa.begin(), sd.fa.end());
      fa.push_back(added[j0 + f]);
    }
    first[nf] = nf * n;
    check(dafs_hip_families_from(ctx, src, nf, first.data(), member.data()));
    if (o.fourway != 0.0f) check(dafs_hip_fourway_consistency(ctx, o.fourway));
    check(dafs_hip_consistency_bp(ctx, o.fold_pct));
    if (listed) {  // the pairs (s, new) of every family: local id s n - s (s + 1) / 2 + m - s - 1
      std::vector<uint64_t> ids;
      for (uint32_t f = 0; f < nf; ++f)
        for (uint64_t s = 0; s < m; ++s) ids.push_back((uint64_t)f * ((uint64_t)n * m / 2) + s * n - s * (s + 1) / 2 + m - s - 1);
      check(dafs_hip_consistency_match_pairs(ctx, o.align_pct, ids.size(), ids.data()));
    } else {
      check(dafs_hip_consistency_match(ctx, o.align_pct));
    }

    std::vector<VU> zs(nf);
    placement_rounds(ctx, prm, o.verbose, nf, [&](size_t f, NodeJob& jb) {
      jb.s1.assign(1, (uint32_t)f * n + m);
      jb.m1.assign(lens[j0 + f], 1);
      jb.s2.resize(m);
      for (uint32_t r = 0; r < m; ++r) jb.s2[r] = (uint32_t)f * n + r;
      jb.m2 = sd.mask;
    }, [&](size_t f, NodeJob& jb) {
      score[j0 + f] = jb.out.score;
      iterations[j0 + f] = jb.out.iterations;
      zs[f].swap(jb.z);
    });

    // per family run_add's placement of its one map; the rows new sequence, then seed rows
    std::vector<Placement> pl;
    std::vector<ALN> roots;
    for (uint32_t f = 0; f < nf; ++f) {
      for (uint32_t z : zs[f]) matched[j0 + f] += z != DAFS_HIP_NONE ? 1 : 0;
      pl.push_back(place(sd, 1, &lens[j0 + f], &zs[f]));
      roots.push_back(placed_rows(sd, pl[f], 1, &lens[j0 + f], f * n + m, f * n));
    }
    std::vector<const ALN*> ptrs;
    for (const ALN& a : roots) ptrs.push_back(&a);
    std::vector<VU> ss;
    std::vector<VL> level(nf), row_level;
    std::vector<AutoInfo> autos;
    if (!o.seed_structure) {
      consensus_structures(ctx, o, ptrs, ss, level, &autos);
    } else {  // nothing is decoded: the seed's structure in every family's merged columns, and each row's support of it
      for (uint32_t f = 0; f < nf; ++f) ss.push_back(carry_structure(sd.ss, pl[f].seed_col, pl[f].width));
      for (uint32_t f = 0; f < nf; ++f) level[f] = carry_levels(sd.level, pl[f].seed_col, pl[f].width);
      std::vector<uint32_t> both, can, half;
      std::vector<double> expd;
      structure_support(ctx, ptrs, ss, both, can, half, expd);
      for (uint32_t f = 0; f < nf; ++f) {  // the new sequence is the first row of its alignment
        sup_both[j0 + f] = both[(size_t)f * n]; sup_can[j0 + f] = can[(size_t)f * n]; sup_half[j0 + f] = half[(size_t)f * n];
        sup_exp[j0 + f] = expd[(size_t)f * n];
      }
    }
    std::vector<VU> row_ss;
    if (o.row_structures) row_ss = row_structures(ctx, o, fa, row_level);
    for (uint32_t f = 0; f < nf; ++f) ss[f] = final_structure(ctx, o, roots[f], &ss[f]);
    // the annotation, once every structure is final: all rows of every family for --stockholm, or for --seed-merged alone the
    // new row of every family (the first), which reads the listed pairs only
    std::vector<Reliability> rl(nf);
    if ((wanted & kSto) || !o.seed_merged.empty()) reliabilities(ctx, fa, ptrs, ss, !(wanted & kSto), rl);
    for (uint32_t f = 0; !o.seed_merged.empty() && f < nf; ++f) {
      all_z[j0 + f] = zs[f];
      new_pp[j0 + f].assign(rl[f].rel.begin(), rl[f].rel.begin() + lens[j0 + f]);
    }
    for (uint32_t f = 0; f < nf; ++f) {
      finish_alignment(ctx, o, fa, roots[f], f * n, recs[j0 + f], nullptr, &pl[f].rf, ss[f], rl[f], o.row_structures ? &row_ss : nullptr,
                       &level[f], &row_level, autos.empty() ? nullptr : &autos[f]);
      print_block(headers[j0 + f], recs[j0 + f]);
      if (o.seed_nearest && matched[j0 + f]) {  // the printed rows (finish_alignment sorted them): the m seed rows, then the new one
        const std::vector<std::string> rows = row_texts(fa, roots[f]);
        const std::vector<uint8_t> cell = cells_of(rows);
        std::vector<uint8_t> cand(n, 1);
        cand[m] = 0;
        std::vector<uint32_t> near(n), ni(n), nd(n);
        check(dafs_hip_alignment_identity(ctx, n, pl[f].width, cell.data(), pl[f].rf.data(), cand.data(), 0.0, nullptr, nullptr, nullptr,
                                          near.data(), ni.data(), nd.data(), nullptr));
        near_row[j0 + f] = near[m];
        near_pid[j0 + f] = (double)ni[m] / (double)nd[m];
      }
    }
  }
  std::cout.flush();
  write_outputs(o, wanted, recs, &headers);
  if (!o.seed_merged.empty()) {  // all k placements in one alignment: the seed rows, then the new rows
    const Placement pl = place(sd, k, lens.data(), all_z.data());
    std::vector<std::string> row_headers, rows;
    std::vector<const double*> rr(m, nullptr);
    for (uint32_t r = 0; r < m; ++r) {
      row_headers.push_back(sd.names[r]);
      rows.push_back(std::string(pl.width, '-'));
      for (uint32_t c = 0; c < C; ++c) rows.back()[pl.seed_col[c]] = sd.rows[r][c];
    }
    for (uint32_t j = 0, off = 0; j < k; off += lens[j], ++j) {
      row_headers.push_back(added[j].name());
      rows.push_back(std::string(pl.width, '-'));
      const std::string& sq = added[j].seq();
      for (uint32_t i = 0; i < lens[j]; ++i) rows.back()[pl.res_col[off + i]] = sq[i];
      rr.push_back(new_pp[j].data());
    }
    const VU carried = carry_structure(sd.ss, pl.seed_col, pl.width);
    std::vector<char> brackets(pl.width + 1);
    const VL carried_level = carry_levels(sd.level, pl.seed_col, pl.width);
    dafs_hip_make_brackets_levels(pl.width, carried.data(), carried_level.empty() ? nullptr : carried_level.data(), brackets.data());
    const std::vector<std::string> names = stockholm_names(row_headers);
    char* text = nullptr;
    check_text(dafs_host_stockholm_block_merged(m + k, pl.width, c_strs(names).data(), c_strs(rows).data(), rr.data(), brackets.data(),
                                                pl.rf.data(), nullptr, &text));
    std::string block = take(text);
    if (!o.compare.empty()) {  // the merged alignment in the seed's columns, with the PP classes of its own block
      std::vector<std::string> pp(m, std::string());
      pp.resize(m + k, std::string(pl.width, '.'));
      for (uint32_t j = 0, off = 0; j < k; off += lens[j], ++j)
        for (uint32_t i = 0; i < lens[j]; ++i) pp[m + j][pl.res_col[off + i]] = dafs_host_pp_char(new_pp[j][i]);
      CompareText cmp;
      compare_of(ctx, o, names, rows, &carried, pl.rf.data(), &pp, cmp);
      write_compare(o, {cmp}, nullptr);
    }
    if (o.seed_nr_given) {  // the non-redundant rows: the rows with a residue in a seed column are compared
      std::vector<uint32_t> inc, pos(m + k, DAFS_HIP_NONE);
      std::vector<std::string> inc_rows;
      for (uint32_t r = 0; r < m + k; ++r)
        if (r < m || matched[r - m]) {
          pos[r] = (uint32_t)inc.size();
          inc.push_back(r);
          inc_rows.push_back(rows[r]);
        }
      const uint32_t ni = (uint32_t)inc.size();
      const std::vector<uint8_t> cell = cells_of(inc_rows);
      std::vector<uint32_t> red((size_t)ni * ((ni + 31) / 32));
      check(dafs_hip_alignment_identity(ctx, ni, pl.width, cell.data(), pl.rf.data(), nullptr, o.seed_nr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                        nullptr, red.data()));
      // the visiting order: the seed rows, then the new rows by descending score, ties in file order
      std::vector<uint32_t> hits(k), rank;
      for (uint32_t j = 0; j < k; ++j) hits[j] = j;
      std::stable_sort(hits.begin(), hits.end(), [&](uint32_t a, uint32_t b) { return score[a] > score[b]; });
      for (uint32_t r = 0; r < m; ++r) rank.push_back(r);
      for (uint32_t j : hits)
        if (pos[m + j] != DAFS_HIP_NONE) rank.push_back(pos[m + j]);
      std::vector<uint8_t> forced(ni, 0), kept_inc(ni), kept(m + k, 1);
      std::fill(forced.begin(), forced.begin() + m, 1);
      std::vector<uint32_t> by(ni);
      check_text(dafs_host_nr_select(ni, red.data(), rank.data(), forced.data(), kept_inc.data(), by.data()));
      for (uint32_t q = 0; q < ni; ++q) kept[inc[q]] = kept_inc[q];
      check_text(dafs_host_stockholm_nr(block.c_str(), m + k, c_strs(names).data(), kept.data(), m, o.seed_nr, &text));
      block = take(text);
    }
    write_text("--seed-merged", o.seed_merged, block);
  }
  if (!o.seed_scores.empty()) {
    std::vector<std::string> added_headers;
    for (const Fasta& s : added) added_headers.push_back(s.name());
    std::vector<std::string> near_name;  // --seed-nearest: the Stockholm names of the nearest seed rows
    if (o.seed_nearest) {
      const std::vector<std::string> seed_names = stockholm_names(sd.names);
      for (uint32_t j = 0; j < k; ++j) near_name.push_back(near_row[j] == DAFS_HIP_NONE ? "-" : seed_names[near_row[j]]);
    }
    char* text = nullptr;
    check_text(dafs_host_seed_table_nearest(k, c_strs(added_headers).data(), lens.data(), matched.data(), score.data(), iterations.data(),
                                            o.seed_structure ? sup_both.data() : nullptr, o.seed_structure ? sup_can.data() : nullptr,
                                            o.seed_structure ? sup_half.data() : nullptr, o.seed_structure ? sup_exp.data() : nullptr,
                                            o.seed_nearest ? c_strs(near_name).data() : nullptr, o.seed_nearest ? near_pid.data() : nullptr, &text));
    write_text("--seed-scores", o.seed_scores, take(text));
  }
  return 0;
}

// `dafs --pairwise FILE` (pipeline.pairwise is the Python twin).  Phase 1 runs once over FILE's N
// sequences in a source context, the folding beside the all-pairs posteriors and no transform; the pairs, row-major, go in
// chunks under dafs_host_batch_bytes() through a second context, where dafs_hip_pairs_from gathers a chunk's two-sequence
// families and align_group runs them as one batch of families.  Each pair prints "==> i j <==" and then what `dafs` prints
// for a file of its two sequences.  Of the side outputs a pair has its Stockholm block alone.
int run_pairwise(const Options& o, int align_model) {
  std::vector<Fasta> fa;
  Fasta::load(fa, o.input.c_str());
  if (fa.size() < 2) throw std::string("--pairwise needs at least two sequences in the input");
  const uint32_t N = (uint32_t)fa.size();
  dafs_hip_ctx* src = nullptr;
  check(dafs_hip_create(o.device, &src));
  Guard src_guard{src};
  set_sequences(src, fa);
  check(dafs_hip_fold_posteriors_begin(src, DAFS_FOLD_CONTRAFOLD, kCutoff));
  const int rc_align = dafs_hip_align_posteriors(src, align_model, o.align_th, 0, 0);
  const int rc_fold = dafs_hip_fold_posteriors_end(src);
  check(rc_align);
  check(rc_fold);
  std::vector<float> sim((size_t)N * N);
  check(dafs_hip_get_sim(src, sim.data()));
  dafs_hip_ctx* ctx = nullptr;
  check(dafs_hip_create(o.device, &ctx));
  Guard guard{ctx};

  std::vector<std::pair<uint32_t, uint32_t> > pairs;
  for (uint32_t x = 0; x < N; ++x)
    for (uint32_t y = x + 1; y < N; ++y) pairs.push_back(std::make_pair(x, y));
  std::vector<double> score(pairs.size(), 0.0);
  std::vector<int64_t> iterations(pairs.size(), 0);
  const unsigned wanted = wanted_of(o) & kSto;
  std::vector<FamilyOut> recs = records(pairs.size(), wanted);
  Ranks rk;  // one process
  // the chunks: greedy in pair order under the estimated device memory of each pair, its phase-1 stores and its root node,
  // which is resident for the whole chunk; a pair over the budget runs alone
  std::vector<uint64_t> bytes(pairs.size());
  for (size_t k = 0; k < pairs.size(); ++k) {
    const uint32_t l[2] = {(uint32_t)fa[pairs[k].first].size(), (uint32_t)fa[pairs[k].second].size()};
    bytes[k] = dafs_host_family_bytes(2, l) + dafs_host_node_bytes(l[0], l[1]);
  }
  for (const auto& chunk : chunks(bytes)) {
    const size_t p0 = chunk.first, n = chunk.second - chunk.first;
    PairChunk pc;
    pc.src = src;
    pc.score.assign(n, 0.0f);
    pc.iterations.assign(n, 0);
    std::vector<std::vector<Fasta> > fams;
    std::vector<size_t> members;
    std::vector<FamilyOut*> out;
    for (size_t j = 0; j < n; ++j) {
      pc.px.push_back(pairs[p0 + j].first);
      pc.py.push_back(pairs[p0 + j].second);
      fams.push_back({fa[pairs[p0 + j].first], fa[pairs[p0 + j].second]});
      members.push_back(j);
      out.push_back(&recs[p0 + j]);
    }
    align_group(ctx, o, rk, align_model, fams, members, out, &pc);
    for (size_t j = 0; j < n; ++j) {
      print_block(std::to_string(pairs[p0 + j].first + 1) + " " + std::to_string(pairs[p0 + j].second + 1), recs[p0 + j]);
      score[p0 + j] = pc.score[j];
      iterations[p0 + j] = pc.iterations[j];
    }
  }
  std::cout.flush();
  write_outputs(o, wanted, recs, nullptr);
  if (!o.pairwise_scores.empty()) {
    std::vector<uint32_t> px, py;
    std::vector<double> psim;
    std::vector<std::string> names;
    for (const Fasta& s : fa) names.push_back(s.name());
    for (const auto& pr : pairs) {
      px.push_back(pr.first);
      py.push_back(pr.second);
      psim.push_back(sim[(size_t)pr.first * N + pr.second]);
    }
    char* text = nullptr;
    check_text(dafs_host_pairwise_table(pairs.size(), px.data(), py.data(), N, c_strs(names).data(), psim.data(), score.data(), iterations.data(), &text));
    write_text("--pairwise-scores", o.pairwise_scores, take(text));
  }
  return 0;
}

// `dafs --cluster T FILE` (pipeline.cluster is the Python twin).  The similarity scores of all pairs come
// from dafs_hip_similarity, which walks the pairs in ranges under the library's budget and keeps no store; the guide tree of
// the whole set (with --cluster-linkage single, complete or average the linkage tree of dafs_hip_linkage_tree, DESIGN.md section
// 21) is cut by dafs_host_cluster_cut; the clusters of at least --cluster-min-size members are the families of
// align_group, as the FILEs of a run of several are: those of two or more sequences in sub-batches under
// dafs_host_batch_bytes() of dafs_host_family_bytes, a cluster of one sequence on the single-sequence path.  Each printed
// cluster is "==> cluster c <==" and then what `dafs` prints for a file of its sequences.
int run_cluster(const Options& o, int align_model) {
  std::vector<Fasta> fa;
  Fasta::load(fa, o.input.c_str());
  if (fa.empty()) throw "no sequences in the input";
  const uint32_t N = (uint32_t)fa.size();
  if (o.cluster_count_given && o.cluster_count > N)
    throw "--cluster-count: " + std::to_string(o.cluster_count) + " clusters asked of " + std::to_string(N) + " sequences";
  dafs_hip_ctx* ctx = nullptr;
  check(dafs_hip_create(o.device, &ctx));
  Guard guard{ctx};
  std::vector<float> sim((size_t)N * N, 1.0f);
  if (N > 1) {
    set_sequences(ctx, fa);
    if (o.cluster_score == DAFS_SCORE_SEQUENCE) {
      check(dafs_hip_similarity(ctx, align_model, o.align_th, 0, nullptr));
    } else {  // all sequences folded as phase 1 of a run folds them, then the pass with the scoring launch in it
      check(dafs_hip_fold_posteriors(ctx, DAFS_FOLD_CONTRAFOLD, kCutoff));
      check_text(dafs_hip_similarity_scored(ctx, align_model, o.align_th, 0, o.cluster_score, o.cluster_weight, nullptr));
    }
    check(dafs_hip_get_sim(ctx, sim.data()));  // the chosen matrix
  }
  std::vector<float> score(2 * N - 1);
  std::vector<int32_t> left(2 * N - 1), right(2 * N - 1);
  if (o.cluster_linkage == 0) check(dafs_host_build_tree(N, sim.data(), score.data(), left.data(), right.data()));
  else if (N == 1) { score[0] = 0.0f; left[0] = right[0] = -1; }  // the one-leaf tree
  else check_text(dafs_hip_linkage_tree(ctx, o.cluster_linkage, N, nullptr, score.data(), left.data(), right.data()));  // on the block the pass left on the device
  std::vector<uint32_t> labels(N);
  uint32_t K = 0;
  check_text(dafs_host_cluster_cut(N, score.data(), left.data(), right.data(), o.cluster_given ? DAFS_CLUSTER_THRESHOLD : DAFS_CLUSTER_COUNT,
                                   (float)o.cluster, o.cluster_count, labels.data(), &K));
  if (!o.cluster_table.empty()) {
    std::vector<std::string> headers;
    std::vector<uint32_t> lens;
    for (const Fasta& s : fa) { headers.push_back(s.name()); lens.push_back(s.size()); }
    char* text = nullptr;
    check_text(dafs_host_cluster_table(N, c_strs(headers).data(), lens.data(), labels.data(), score.data(), left.data(), right.data(), sim.data(), &text));
    write_text("--cluster-table", o.cluster_table, take(text));
  }
  if (!o.cluster_tree.empty()) {
    std::vector<node_t> tree(2 * N - 1);
    for (uint i = 0; i < 2 * N - 1; ++i) tree[i] = std::make_pair(score[i], std::make_pair((uint)left[i], (uint)right[i]));
    std::ostringstream tl;
    print_tree(tl, tree, fa, (int)tree.size() - 1);
    tl << std::endl;
    write_text("--cluster-tree", o.cluster_tree, tl.str());
  }
  // the clusters that are aligned, as the families of a run of several files
  std::vector<std::vector<Fasta> > all(K);
  for (uint32_t i = 0; i < N; ++i) all[labels[i]].push_back(fa[i]);
  std::vector<std::vector<Fasta> > fams;
  std::vector<std::string> headers;
  for (uint32_t c = 0; c < K; ++c)
    if (all[c].size() >= o.cluster_min_size) {
      fams.push_back(all[c]);
      headers.push_back("cluster " + std::to_string(c + 1));
    }
  const size_t P = fams.size();
  const unsigned wanted = wanted_of(o) & ~kCmp;
  std::vector<FamilyOut> recs = records(P, wanted);
  Ranks rk;  // one process
  auto group = [&](const std::vector<size_t>& members) {
    std::vector<FamilyOut*> out;
    for (size_t f : members) out.push_back(&recs[f]);
    align_group(ctx, o, rk, align_model, fams, members, out);
  };
  std::vector<size_t> batch;
  std::vector<uint64_t> bytes;
  for (size_t f = 0; f < P; ++f)
    if (fams[f].size() > 1) {
      std::vector<uint32_t> lens;
      for (const Fasta& s : fams[f]) lens.push_back(s.size());
      batch.push_back(f);
      bytes.push_back(dafs_host_family_bytes((uint32_t)lens.size(), lens.data()));
    }
  for (const auto& chunk : chunks(bytes)) group(std::vector<size_t>(batch.begin() + chunk.first, batch.begin() + chunk.second));
  for (size_t f = 0; f < P; ++f)
    if (fams[f].size() == 1) group({f});
  for (size_t f = 0; f < P; ++f) print_block(headers[f], recs[f]);
  std::cout.flush();
  write_outputs(o, wanted, recs, &headers);
  return 0;
}

// `dafs --describe ALIGNMENT` (pipeline.describe is the Python twin): the calls that read an alignment
// alone, on a finished alignment that the seed reader reads.  Nothing is aligned and nothing is printed.
int run_describe(const Options& o) {
  std::vector<std::string> headers, rows;
  VU ss;
  VL level;
  read_seed(o.describe, headers, rows, &ss, true, o.knots ? &level : nullptr);
  if (o.knots && !level.empty()) {  // the structure as it was read, each level with its own bracket kind
    std::vector<char> str(ss.size() + 1);
    dafs_hip_make_brackets_levels((uint32_t)ss.size(), ss.data(), level.data(), str.data());
    std::cout << ">SS_cons" << std::endl << str.data() << std::endl;
  }
  const std::vector<std::string> names = stockholm_names(headers);
  dafs_hip_ctx* ctx = nullptr;
  check(dafs_hip_create(o.device, &ctx));
  Guard guard{ctx};
  if (!o.identity.empty()) {
    IdentityText idt;
    identity_of(ctx, names, rows, !o.identity_matrix.empty(), idt);
    write_identity(o, {idt}, nullptr);
  }
  if (!o.phylogeny.empty()) {
    std::string newick, table;
    phylogeny_of(ctx, o, names, rows, newick, table);
    write_text("--phylogeny", o.phylogeny, newick);
    if (!o.phylogeny_support.empty()) write_text("--phylogeny-support", o.phylogeny_support, table);
  }
  if (!o.covariation.empty()) {
    std::string cov, chars;
    covariation_of(ctx, o, rows, ss, cov, chars);
    write_text("--covariation", o.covariation, cov);
  }
  if (!o.compare.empty()) {  // the file again: whether it has a structure, and its PP lines
    std::vector<std::string> h2, r2, pp;
    VU ss2;
    bool has_ss = false;
    VL level2;
    read_alignment(o.describe, "--describe", h2, r2, ss2, has_ss, &pp, o.knots ? &level2 : nullptr);
    CompareText cmp;
    compare_of(ctx, o, names, rows, has_ss ? &ss2 : nullptr, nullptr, pp.empty() ? nullptr : &pp, cmp);
    write_compare(o, {cmp}, nullptr);
  }
  return 0;
}

int run(const Options& o, Ranks& rk) {
  // ---- option checks mirroring parse_options (:1683-1763)
  int align_model;
  if (o.align_model == "ProbCons") align_model = DAFS_ALIGN_PROBCONS;
  else if (o.align_model == "CONTRAlign") align_model = DAFS_ALIGN_CONTRALIGN;
  else throw "Unknown alignment model: " + o.align_model;
  if (o.fold_aux.empty()) {
    if (o.fold_model == "Boltzmann" || o.fold_model == "Vienna")
      throw "Folding model " + o.fold_model + " needs ViennaRNA, which this build does not contain; use -s CONTRAfold or --fold-aux";
    if (o.fold_model != "CONTRAfold") throw "Unknown folding model: " + o.fold_model;
  }
  if ((o.fold_decoder != "Nussinov" && o.fold_decoder != "Levels") || o.ipknot)
    throw "Folding decoder IPknot needs an ILP solver, which this build does not contain; --fold-decoder Levels decodes pseudoknots level by level";
  if (o.max_iter <= 0) throw "-m 0 (exact ILP) needs an ILP solver, which this build does not contain";
  if ((o.bp_update || o.bp_update1) && !o.fold_aux.empty()) throw "--bp-update / --bp-update1 need a folding model (-s CONTRAfold), not --fold-aux";
  if (!o.devices.empty() && (!o.fold_aux.empty() || !o.align_aux.empty() || o.fourway != 0.0f))
    throw std::string("--devices shards the posterior models and the consistency transform; --fold-aux, --align-aux and -f run on one device (--device)");
  if (o.verbose >= 1) {
    if (!o.no_alifold) std::cerr << "note: RNAalifold is not available in this build; running as with --no-alifold" << std::endl;
    if (!o.fold_model_given && o.fold_aux.empty()) std::cerr << "note: default folding model is CONTRAfold in this build" << std::endl;
  }
  if (!o.describe.empty()) return rk.rank == 0 ? run_describe(o) : 0;
  if (!o.seed.empty()) return o.seed_each ? run_add_each(o, align_model) : run_add(o, align_model);
  if (o.pairwise) return run_pairwise(o, align_model);
  if (o.cluster_given || o.cluster_count_given) return run_cluster(o, align_model);

  // one family per input file
  const bool multi = o.inputs.size() > 1;
  std::vector<std::vector<Fasta> > fams(o.inputs.size());
  for (size_t f = 0; f < o.inputs.size(); ++f) {
    const std::string& file = o.inputs[f];
    try {
      Fasta::load(fams[f], file.c_str());
    } catch (const std::system_error& e) {
      if (multi) throw file + ": " + e.code().message();
      throw;
    }
    if (fams[f].empty()) {
      if (multi) throw file + ": no sequences in the input";
      throw "no sequences in the input";
    }
  }

  dafs_hip_ctx* ctx = nullptr;
  check(dafs_hip_create(o.devices.empty() ? o.device : o.devices[rk.rank], &ctx));
  Guard guard{ctx};

  // one record per input file, in input order; the files are written by the process that prints
  const unsigned wanted = wanted_of(o);
  std::vector<FamilyOut> recs = records(o.inputs.size(), wanted);
  if (!multi) {  // printed as it is made
    recs[0].os = &std::cout;
    align_group(ctx, o, rk, align_model, fams, {0}, {&recs[0]});
    if (rk.rank == 0) write_outputs(o, wanted, recs, nullptr);
    return 0;
  }
  // Several files: every file with two or more sequences in one batch (dafs_hip_set_families: shared launches, one guide
  // tree per family, the forest walked together); a file of one sequence takes the single-sequence path of a run of its
  // own (no pairs, no consistency transforms) on the same context.  Each block is what `dafs FILE` prints.
  std::vector<size_t> batch;
  for (size_t f = 0; f < fams.size(); ++f)
    if (fams[f].size() > 1) batch.push_back(f);
  auto names = [&](const std::vector<size_t>& members) {
    std::string s;
    for (size_t f : members) s += (s.empty() ? "" : ", ") + o.inputs[f];
    return s;
  };
  auto group = [&](const std::vector<size_t>& members) {
    std::vector<FamilyOut*> out;
    for (size_t f : members) out.push_back(&recs[f]);
    try {
      align_group(ctx, o, rk, align_model, fams, members, out);
    } catch (const char* str) {
      throw names(members) + ": " + str;
    } catch (const std::string& str) {
      throw names(members) + ": " + str;
    }
  };
  if (!batch.empty()) group(batch);
  for (size_t f = 0; f < fams.size(); ++f)
    if (fams[f].size() == 1) group({f});
  for (size_t f = 0; f < fams.size(); ++f) print_block(o.inputs[f], recs[f]);
  std::cout.flush();
  write_outputs(o, wanted, recs, &o.inputs);
  return 0;
}

}  // namespace

int main(int argc, char* argv[]) {
  try {
    const Options o = parse(argc, argv);
    Ranks rk;
    if (!o.devices.empty()) rk.fork_ranks(o.devices);  // before the first GPU call
    const int rc = run(o, rk);
    if (rk.rank == 0) rk.wait_ranks();
    return rc;
  } catch (const char* str) {
    std::cerr << str << std::endl;
  } catch (const std::string& str) {
    std::cerr << str << std::endl;
  } catch (const std::system_error& e) {
    std::cerr << e.what() << std::endl;
  } catch (const std::exception& e) {
    std::cerr << e.what() << std::endl;
  }
  return EXIT_FAILURE;
}
