// mvolps -- command-line front end over libmvolps_amd.so; counterpart of MVOLPS's main
// (/root/reference/2test.cpp:13-157): same flags, same dispatch on the file extension
// (2test.cpp:65-81), then initProblem (util.cpp:277-292) and branchAndBound (bs.cpp:54).
// Extra flags of this build: --repaired (reference_quirks = 0), --max-nodes N, --events FILE, --ranges FILE, --kkt FILE, --farkas FILE,
// --sift [K].
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "../../include/mvx_bnb.h"

namespace {
class InputParser { // InputParser.h:8-35
public:
  InputParser(int argc, char **argv) {
    for (int i = 1; i < argc; i++) tokens.push_back(std::string(argv[i]));
  }
  const std::string &getCMDOption(const std::string &option) const {
    auto itr = std::find(tokens.begin(), tokens.end(), option);
    if (itr != tokens.end() && ++itr != tokens.end()) return *itr;
    static const std::string empty("");
    return empty;
  }
  bool CMDOptionExists(const std::string &option) const { return std::find(tokens.begin(), tokens.end(), option) != tokens.end(); }

private:
  std::vector<std::string> tokens;
};
// --node-purge without a number (DESIGN.md "Cut purging in the tree (node_purge)": the smallest age limit of the CPU sweep
// whose work is not above that of no purge on any of its sets)
const long NODE_PURGE_DEFAULT = 1;
// --node-cliques without a number (DESIGN.md "Clique cuts in the tree (node_cliques)": the smallest K of the CPU sweep behind
// which a larger K no longer cuts the node counts of its instances)
const long NODE_CLIQUES_DEFAULT = 4;
} // namespace

int main(int argc, char **argv) {
  InputParser input(argc, argv);
  if (input.CMDOptionExists("-h") || input.CMDOptionExists("--help")) {
    std::cout << "Usage: mvolps [OPTION]\n"
              << "File input options:\n"
              << "  -f/--file [FILENAME.{mps|lp}]\n\n"
              << "  --events [FILE] write the B&B event stream (one line per event) to FILE\n"
              << "  --ranges [FILE] solve the root LP, write its sensitivity ranges (one line per row and column: activity ranges,\n"
              << "                  objective changes, allowable cost changes) to FILE, then run as without the flag\n"
              << "  --kkt [FILE]    solve the root LP, write its KKT check against the model (four lines KKT.PE, KKT.PB, KKT.DE, KKT.DB:\n"
              << "                  ae_max, its index, re_max, its index) to FILE, run the tree with every node LP checked, and append\n"
              << "                  the tree's summary (nodes checked, worst re_max per condition and its node); not with --best-window\n"
              << "  --farkas [FILE] solve the root LP; when it is infeasible write the proof (FARKAS.ROOT: found, row, side, dropped, rel of the\n"
              << "                  tableau side, rel of the model side, Lo or -Hi, de) to FILE, when it is unbounded its ray (RAY.ROOT: found,\n"
              << "                  variable, direction, blocking variables, rows of ae and re, dual, ae, re, slope); run the tree with every infeasible node LP\n"
              << "                  asked for its proof, and append the tree's totals; not with --best-window\n"
              << "  --sift [K]      solve the file's LP relaxation by sifting and stop: the columns that cannot rest at 0 form the first\n"
              << "                  working LP (column 1 when there is none), all others a device-resident pool that is priced whole\n"
              << "                  every round; at most K columns join per round (max(m, 64) without a number); prints the status, the\n"
              << "                  objective, the rounds, the columns appended and purged and the final width\n"
              << "Output verbosity options:\n"
              << "  -s/--silent\n  -v/--verbose\n  -d/--debug\n  -so/--solver-output\n\n"
              << "Algorithm strategy options:\n"
              << "  -vs [{0|1|2|3|4}]\n"
              << "    0. vars are picked on order\n"
              << "    1. vars are picked on fractional part closeness to 0.5\n"
              << "    2. vars are picked on greatest impact on obj. function\n"
              << "    3. vars are picked on the node LP's dual penalties (largest product of both sides)\n"
              << "    4. strong branching on the --sb-cands best penalty candidates (not with --best-window)\n"
              << "  -bs [{0|1}]\n"
              << "    0. nodes are picked for DFS (FIFO/queue)\n"
              << "    1. nodes are picked for best-FS (greatest z-value)\n"
              << "  -cm [{0|1}]\n"
              << "    0. disable cut generation\n"
              << "    1. generate Gomory mixed integer\n"
              << "    -cf [0...1]\n"
              << "      Percentage of generated cuts to be added per node\n"
              << "  --repaired      children keep the opposite bound, integrality within 1e-9, repaired GMI cuts\n"
              << "  --cut-select K  with --repaired -cm 1: 0 add the last cut, 1 add the -cf fraction of most effective cuts\n"
              << "  --best-window N with -bs 1: speculate on the top N open nodes per round (same tree; 0 = node at a time)\n"
              << "  --max-nodes N   stop after N loop iterations\n"
              << "  --sb-cands K    with -vs 4: candidates strong-branched per node (default 2)\n"
              << "  --sb-iters L    with -vs 4: pivot limit of each strong-branching child solve (default 4)\n"
              << "  --heur [{0|1|2}] with --repaired: primal rounding heuristic on every branching node's LP (on the device\n"
              << "                  up to 4096 columns, on the host beyond)\n"
              << "    0. off (default)\n"
              << "    1. round the LP values (away from the rows' locks) and keep the point when it is feasible\n"
              << "    2. as 1, then raise the columns greedily along the objective while every row allows it\n"
              << "  --rcfix         with --repaired (not with --best-window): once an incumbent exists, tighten the bounds of non-basic\n"
              << "                  integer columns from their reduced costs on every branching node; both children inherit them\n"
              << "  --prop [K]      with --repaired (not with --best-window): bound propagation over the model's rows, at most K rounds\n"
              << "                  (1..16; 8 without a number), on the root and on every child in front of its first solve\n"
              << "  --dive [R]      with --repaired (not with --best-window): LP diving heuristic at the root, R the rules as bits\n"
              << "                  (1 fractional, 2 locks, 4 vector length; 7 without a number); a better point becomes the incumbent\n"
              << "  --dive-freq F   with --dive: also dive at every branching node whose number F divides (default 0: the root only)\n"
              << "  --dive-depth D  with --dive: step limit of one dive (default 0: 4 n + 64)\n"
              << "  --pump [N]      with --repaired (not with --best-window): feasibility pump at the root, at most N distance LPs\n"
              << "                  (1..1000; 30 without a number), in front of the dives; a better point becomes the incumbent\n"
              << "  --pump-freq F   with --pump: also pump at every branching node whose number F divides (default 0: the root only)\n"
              << "  --pump-alpha A  with --pump: weight of the model's objective in the first distance LP (0..1, default 0; times 0.9\n"
              << "                  with every further LP)\n"
              << "  --cut-rounds [R] with --repaired: R rounds of GMI cuts on the root LP before the tree starts (1..64; 5 without a\n"
              << "                  number): per round the cuts of all fractional integer columns, the most effective first, none\n"
              << "                  nearly parallel to one already taken\n"
              << "  --cut-round-max K with --cut-rounds: most cuts one round appends (1..4096, default 32)\n"
              << "  --cut-maxpar P  with --cut-rounds: largest cosine between two cuts of a round (0 < P <= 1, default 0.9)\n"
              << "  --cut-families F with --cut-rounds: the cut families as bits (1..3, default 1): 1 GMI cuts, 2 clique cuts from the\n"
              << "                  conflict graph of the binary columns\n"
              << "  --cut-purge [A] with --cut-rounds: a cut row leaves the root LP again once it has been slack after A re-solves in a\n"
              << "                  row (1..64; 3 without a number)\n"
              << "  --polish [N]    with --repaired: every point that becomes the incumbent is first improved by a search over one- and\n"
              << "                  two-column unit moves, at most N of them (1..100000; 1000 without a number)\n"
              << "  --node-purge [A] with --repaired, not with --best-window: a cut row leaves both children of a branching node once it\n"
              << "                  has been slack at A branching nodes in a row on its path (1..64; 1 without a number)\n"
              << "  --node-cliques [K] with --repaired, not with --best-window: up to K violated cliques of the binary columns' conflict\n"
              << "                  graph are separated at every branching node and appended to both children (1..64; 4 without a number)\n"
              << "Help:\n  -h/--help\n";
    return 0;
  }
  mvx_term_out(MVX_OFF); // 2test.cpp:45
  const bool verbose = input.CMDOptionExists("-v") || input.CMDOptionExists("--verbose") || input.CMDOptionExists("-d") ||
                       input.CMDOptionExists("--debug");
  if (input.CMDOptionExists("-d") || input.CMDOptionExists("--debug") || input.CMDOptionExists("-so") ||
      input.CMDOptionExists("--solver-output"))
    mvx_term_out(MVX_ON);

  if (!(input.CMDOptionExists("-f") || input.CMDOptionExists("--file"))) {
    std::cout << "see ./mvolps -h for usage\n";
    return 0;
  }
  std::string fn = input.getCMDOption("-f");
  if (fn.empty()) fn = input.getCMDOption("--file");
  const size_t dot = fn.rfind('.');
  const std::string ext = dot == std::string::npos ? "" : fn.substr(dot);
  mvx_prob *prob = mvx_create_prob();
  if (ext == ".lp") {
    if (mvx_read_lp(prob, nullptr, fn.c_str())) std::exit(-1); // util.cpp:284-287
  } else if (ext == ".mps") {
    if (mvx_read_mps(prob, 2 /*GLP_MPS_FILE*/, nullptr, fn.c_str())) std::exit(-1); // util.cpp:290-292
  } else {
    std::cout << "Unrecognized filetype\n";
    return -1;
  }
  if (verbose) std::printf("%s\nProblem contains %d integer variables\n", mvx_version(), mvx_get_num_int(prob)); // util.cpp:278,298

  if (input.CMDOptionExists("--sift")) {
    // the LP relaxation by sifting (DESIGN.md "Sifting (sift)"): the columns that cannot rest at 0 are the first working set
    // (column 1 when there is none), every other column goes to the pool
    const int m = mvx_get_num_rows(prob), n = mvx_get_num_cols(prob);
    const std::string kopt = input.getCMDOption("--sift");
    mvx_sift_parm sp;
    mvx_init_sift_parm(&sp, m);
    if (!kopt.empty() && kopt[0] != '-') {
      sp.K = std::atoi(kopt.c_str());
      if (sp.K < 1) {
        std::fprintf(stderr, "Unknown parameter value for --sift\n");
        return -1;
      }
    }
    if (n < 1) {
      std::fprintf(stderr, "--sift: the model has no columns\n");
      return -1;
    }
    mvx_colpool *pool = mvx_pool_create(m);
    std::vector<int> ind((size_t)m + 1), pooled(1, 0);
    std::vector<double> val((size_t)m + 1), col((size_t)m + 1);
    auto to_pool = [&](int j) { // 0 when column j can rest at 0 and has joined the pool
      std::fill(col.begin(), col.end(), 0.0);
      const int len = mvx_get_mat_col(prob, j, ind.data(), val.data());
      for (int t = 1; t <= len; t++) col[(size_t)ind[(size_t)t]] = val[(size_t)t];
      const double obj = mvx_get_obj_coef(prob, j), lb = mvx_get_col_lb(prob, j), ub = mvx_get_col_ub(prob, j); // an absent bound is not read
      const int type = mvx_get_col_type(prob, j);
      return mvx_pool_add_cols(pool, 1, col.data(), &obj, &type, &lb, &ub, nullptr);
    };
    for (int j = 1; j <= n; j++)
      if (to_pool(j) == 0) pooled.push_back(j);
    if ((int)pooled.size() - 1 == n) { // every column can rest at 0: column 1 is the working set; the pool is built again without it
      mvx_pool_delete(pool);
      pool = mvx_pool_create(m);
      pooled.assign(1, 0);
      for (int j = 2; j <= n; j++)
        if (to_pool(j) == 0) pooled.push_back(j);
    }
    const int N = (int)pooled.size() - 1;
    if (N > 0 && mvx_del_cols(prob, N, pooled.data()) != 0) {
      std::fprintf(stderr, "--sift: the working LP could not be formed\n");
      return -1;
    }
    std::vector<int> where((size_t)N + 1, 0);
    mvx_sift_info info;
    const int rc = mvx_sift(prob, pool, nullptr, &sp, where.data(), &info);
    static const char *names[] = {"ROUND LIMIT", "UNDEFINED", "FEASIBLE", "INFEASIBLE (working LP only)", "NO FEASIBLE SOLUTION (working LP only)",
                                  "OPTIMAL", "UNBOUNDED"};
    std::printf("SIFT.RC %d\nSIFT.STATUS %s\nSIFT.OBJ %.17g\nSIFT.ROUNDS %d\nSIFT.APPENDED %lld\nSIFT.PURGED %lld\nSIFT.N_FINAL %d of %d\n", rc,
                names[info.end >= 0 && info.end <= 6 ? info.end : 1], mvx_get_obj_val(prob), info.rounds, info.appended, info.purged,
                info.n_final, n);
    mvx_pool_delete(pool);
    mvx_delete_prob(prob);
    return rc == 0 ? 0 : 1;
  }

  mvx_bnb_params params;
  mvx_bnb_default_params(&params);
  auto int_opt = [&](const char *flag, int lo, int hi, int *out) -> bool {
    if (!input.CMDOptionExists(flag)) return true;
    const int v = std::atoi(input.getCMDOption(flag).c_str());
    if (v < lo || v > hi) {
      std::fprintf(stderr, "Unknown parameter value for %s\n", flag);
      return false;
    }
    *out = v;
    return true;
  };
  if (!int_opt("-bs", 0, 1, &params.node_strat)) return -1; // 2test.cpp:92-104
  if (!int_opt("-vs", 0, 4, &params.var_strat)) return -1;  // 2test.cpp:106-121; 3 / 4 read the node LP
  if (!int_opt("--sb-cands", 0, 1 << 20, &params.sb_cands)) return -1;
  if (!int_opt("--sb-iters", 0, 1 << 30, &params.sb_iters)) return -1;
  if (!int_opt("--heur", 0, 2, &params.heur)) return -1;
  if (!int_opt("-cm", 0, 1, &params.cut_strat)) return -1;  // 2test.cpp:123-134
  if (input.CMDOptionExists("-cm")) {
    params.cut_chance = 1.0;
    if (input.CMDOptionExists("-cf")) {
      const double chance = std::atof(input.getCMDOption("-cf").c_str());
      if (!((chance <= 1.0) && (chance >= 0.0))) {
        std::fprintf(stderr, "Cut Frequency parameter must be in range [0.0, 1.0]\n");
        return -1;
      }
      params.cut_chance = chance; // stored, never read (util.cpp:259-261)
    }
  }
  if (input.CMDOptionExists("--repaired")) params.reference_quirks = 0;
  if (input.CMDOptionExists("--rcfix")) params.rc_fix = 1;
  if (input.CMDOptionExists("--prop")) {
    // the number is optional: the next token is K only when all of it is digits (another option or a file name is not)
    const std::string &k = input.getCMDOption("--prop");
    const bool numeric = !k.empty() && std::all_of(k.begin(), k.end(), [](char ch) { return ch >= '0' && ch <= '9'; });
    const long kv = numeric ? std::strtol(k.c_str(), nullptr, 10) : 8;
    params.prop = kv >= 1 && kv <= 16 ? (int)kv : -1;
    if (params.prop < 1) {
      std::fprintf(stderr, "Unknown parameter value for --prop\n");
      return -1;
    }
  }
  if (input.CMDOptionExists("--dive")) {
    // the number is optional, as for --prop
    const std::string &k = input.getCMDOption("--dive");
    const bool numeric = !k.empty() && std::all_of(k.begin(), k.end(), [](char ch) { return ch >= '0' && ch <= '9'; });
    const long kv = numeric ? std::strtol(k.c_str(), nullptr, 10) : 7;
    params.dive = kv >= 1 && kv <= 7 ? (int)kv : -1;
    if (params.dive < 1) {
      std::fprintf(stderr, "Unknown parameter value for --dive\n");
      return -1;
    }
  }
  if (!int_opt("--dive-freq", 0, 1 << 30, &params.dive_freq)) return -1;
  if (!int_opt("--dive-depth", 0, 1 << 30, &params.dive_depth)) return -1;
  if (input.CMDOptionExists("--pump")) {
    // the number is optional, as for --prop
    const std::string &k = input.getCMDOption("--pump");
    const bool numeric = !k.empty() && std::all_of(k.begin(), k.end(), [](char ch) { return ch >= '0' && ch <= '9'; });
    const long kv = numeric ? std::strtol(k.c_str(), nullptr, 10) : 30;
    params.pump = kv >= 1 && kv <= 1000 ? (int)kv : -1;
    if (params.pump < 1) {
      std::fprintf(stderr, "Unknown parameter value for --pump\n");
      return -1;
    }
  }
  if (!int_opt("--pump-freq", 0, 1 << 30, &params.pump_freq)) return -1;
  if (input.CMDOptionExists("--pump-alpha")) {
    char *end = nullptr;
    const std::string &k = input.getCMDOption("--pump-alpha");
    params.pump_alpha = std::strtod(k.c_str(), &end);
    if (k.empty() || *end != 0 || !(params.pump_alpha >= 0.0 && params.pump_alpha <= 1.0)) {
      std::fprintf(stderr, "Unknown parameter value for --pump-alpha\n");
      return -1;
    }
  }
  if (input.CMDOptionExists("--cut-rounds")) {
    // the number is optional, as for --prop
    const std::string &k = input.getCMDOption("--cut-rounds");
    const bool numeric = !k.empty() && std::all_of(k.begin(), k.end(), [](char ch) { return ch >= '0' && ch <= '9'; });
    const long kv = numeric ? std::strtol(k.c_str(), nullptr, 10) : 5;
    params.cut_rounds = kv >= 1 && kv <= 64 ? (int)kv : -1;
    if (params.cut_rounds < 1) {
      std::fprintf(stderr, "Unknown parameter value for --cut-rounds\n");
      return -1;
    }
  }
  if (!int_opt("--cut-round-max", 1, 4096, &params.cut_round_max)) return -1;
  if (input.CMDOptionExists("--cut-maxpar")) {
    char *end = nullptr;
    const std::string &k = input.getCMDOption("--cut-maxpar");
    params.cut_maxpar = std::strtod(k.c_str(), &end);
    if (k.empty() || *end != 0 || !(params.cut_maxpar > 0.0 && params.cut_maxpar <= 1.0)) {
      std::fprintf(stderr, "Unknown parameter value for --cut-maxpar\n");
      return -1;
    }
  }
  if (!int_opt("--cut-families", 1, 3, &params.cut_families)) return -1;
  if (input.CMDOptionExists("--cut-purge")) {
    // the number is optional, as for --cut-rounds
    const std::string &k = input.getCMDOption("--cut-purge");
    const bool numeric = !k.empty() && std::all_of(k.begin(), k.end(), [](char ch) { return ch >= '0' && ch <= '9'; });
    const long kv = numeric ? std::strtol(k.c_str(), nullptr, 10) : 3;
    params.cut_purge = kv >= 1 && kv <= 64 ? (int)kv : -1;
    if (params.cut_purge < 1) {
      std::fprintf(stderr, "Unknown parameter value for --cut-purge\n");
      return -1;
    }
  }
  if (input.CMDOptionExists("--polish")) {
    // the number is optional, as for --prop
    const std::string &k = input.getCMDOption("--polish");
    const bool numeric = !k.empty() && std::all_of(k.begin(), k.end(), [](char ch) { return ch >= '0' && ch <= '9'; });
    const long kv = numeric ? std::strtol(k.c_str(), nullptr, 10) : 1000;
    params.polish = kv >= 1 && kv <= 100000 ? (int)kv : -1;
    if (params.polish < 1) {
      std::fprintf(stderr, "Unknown parameter value for --polish\n");
      return -1;
    }
  }
  if (input.CMDOptionExists("--node-purge")) {
    // the number is optional, as for --cut-purge; what follows the flag and is neither a number nor the next flag is refused
    const std::string &k = input.getCMDOption("--node-purge");
    const bool numeric = !k.empty() && k.size() <= 3 && std::all_of(k.begin(), k.end(), [](char ch) { return ch >= '0' && ch <= '9'; });
    const long kv = numeric ? std::strtol(k.c_str(), nullptr, 10) : NODE_PURGE_DEFAULT;
    const bool absent = k.empty() || k[0] == '-'; // the next flag, or the end of the line
    params.node_purge = (numeric || absent) && kv >= 1 && kv <= 64 ? (int)kv : -1;
    if (params.node_purge < 1) {
      std::fprintf(stderr, "Unknown parameter value for --node-purge\n");
      return -1;
    }
  }
  if (input.CMDOptionExists("--node-cliques")) {
    // the number is optional, as for --node-purge
    const std::string &k = input.getCMDOption("--node-cliques");
    const bool numeric = !k.empty() && k.size() <= 3 && std::all_of(k.begin(), k.end(), [](char ch) { return ch >= '0' && ch <= '9'; });
    const long kv = numeric ? std::strtol(k.c_str(), nullptr, 10) : NODE_CLIQUES_DEFAULT;
    const bool absent = k.empty() || k[0] == '-'; // the next flag, or the end of the line
    params.node_cliques = (numeric || absent) && kv >= 1 && kv <= 64 ? (int)kv : -1;
    if (params.node_cliques < 1) {
      std::fprintf(stderr, "Unknown parameter value for --node-cliques\n");
      return -1;
    }
    if (params.reference_quirks != 0) {
      std::fprintf(stderr, "--node-cliques needs --repaired\n");
      return -1;
    }
  }
  if (input.CMDOptionExists("--cut-select")) params.cut_select = std::atoi(input.getCMDOption("--cut-select").c_str());
  if (input.CMDOptionExists("--window")) params.window = std::atoi(input.getCMDOption("--window").c_str());
  if (input.CMDOptionExists("--best-window")) params.best_window = std::atoi(input.getCMDOption("--best-window").c_str());
  if (input.CMDOptionExists("--max-nodes")) params.max_nodes = std::atoi(input.getCMDOption("--max-nodes").c_str());
  if (input.CMDOptionExists("--server"))
    std::fprintf(stderr, "--server: the ZeroMQ sink is not part of this build; use --events FILE for the same stream\n");

  if (input.CMDOptionExists("--ranges")) {
    const std::string &path = input.getCMDOption("--ranges");
    if (path.empty() || path[0] == '-') { // the end of the line, or the next flag
      std::fprintf(stderr, "Unknown parameter value for --ranges\n");
      return -1;
    }
    // the root LP as the tree will first solve it, on a copy: the run below starts from the handle as it was read
    mvx_prob *root = mvx_create_prob();
    mvx_copy_prob(root, prob, MVX_ON);
    if (!params.reference_quirks) mvx_bnb_integral_bounds(nullptr, root);
    mvx_simplex(root, nullptr);
    const size_t rows = (size_t)mvx_get_num_rows(root) + (size_t)mvx_get_num_cols(root) + 1;
    std::vector<double> val(rows * 6);
    std::vector<int> var(rows * 4);
    int rrc = mvx_ranges(root, val.data(), var.data());
    if (rrc == 0) rrc = mvx_bnb_print_ranges(nullptr, root, val.data(), var.data(), path.c_str());
    if (rrc != 0) std::fprintf(stderr, "--ranges: no report (%d): the root LP has no optimal basis, or %s cannot be written\n", rrc, path.c_str());
    mvx_delete_prob(root);
  }

  std::string kkt_path;
  if (input.CMDOptionExists("--kkt")) {
    kkt_path = input.getCMDOption("--kkt");
    if (kkt_path.empty() || kkt_path[0] == '-') { // the end of the line, or the next flag
      std::fprintf(stderr, "Unknown parameter value for --kkt\n");
      return -1;
    }
    if (params.best_window > 0) {
      std::fprintf(stderr, "--kkt is not supported with --best-window\n");
      return -1;
    }
    // the root LP as the tree will first solve it, on a copy: the run below starts from the handle as it was read
    mvx_prob *root = mvx_create_prob();
    mvx_copy_prob(root, prob, MVX_ON);
    if (!params.reference_quirks) mvx_bnb_integral_bounds(nullptr, root);
    mvx_simplex(root, nullptr);
    double val[8];
    int ind[8];
    const int krc = mvx_kkt(root, val, ind, nullptr, nullptr);
    FILE *out = krc == 0 ? std::fopen(kkt_path.c_str(), "w") : nullptr;
    if (out) {
      static const char *const cond[4] = {"PE", "PB", "DE", "DB"};
      for (int c = 0; c < 4; c++) std::fprintf(out, "KKT.%s %.17g %d %.17g %d\n", cond[c], val[2 * c], ind[2 * c], val[2 * c + 1], ind[2 * c + 1]);
      std::fclose(out);
      params.kkt = 1; // the tree's summary follows the root's lines
    } else { // nothing was written and nothing will be appended: the run goes on as without the flag
      std::fprintf(stderr, "--kkt: no report (%d): the root LP could not be checked, or %s cannot be written; the tree runs unchecked\n", krc,
                   kkt_path.c_str());
    }
    mvx_delete_prob(root);
  }

  std::string farkas_path;
  if (input.CMDOptionExists("--farkas")) {
    farkas_path = input.getCMDOption("--farkas");
    if (farkas_path.empty() || farkas_path[0] == '-') { // the end of the line, or the next flag
      std::fprintf(stderr, "Unknown parameter value for --farkas\n");
      return -1;
    }
    if (params.best_window > 0) {
      std::fprintf(stderr, "--farkas is not supported with --best-window\n");
      return -1;
    }
    // the root LP as the tree will first solve it, on a copy: the run below starts from the handle as it was read
    mvx_prob *root = mvx_create_prob();
    mvx_copy_prob(root, prob, MVX_ON);
    if (!params.reference_quirks) mvx_bnb_integral_bounds(nullptr, root);
    mvx_simplex(root, nullptr);
    double val[4] = {0.0, 0.0, 0.0, 0.0};
    int ind[4] = {0, 0, 0, 0};
    int rind[6] = {0, 0, 0, 0, 0, 0};
    const bool nofeas = mvx_get_status(root) == MVX_NOFEAS, unbnd = mvx_get_status(root) == MVX_UNBND;
    const int frc = nofeas ? mvx_farkas(root, val, ind, nullptr) : unbnd ? mvx_ray(root, val, rind, nullptr) : 0;
    FILE *out = frc == 0 ? std::fopen(farkas_path.c_str(), "w") : nullptr;
    if (out) {
      if (nofeas) std::fprintf(out, "FARKAS.ROOT %d %d %d %d %.17g %.17g %.17g %.17g\n", ind[0], ind[1], ind[2], ind[3], val[0], val[1], val[2], val[3]);
      if (unbnd)
        std::fprintf(out, "RAY.ROOT %d %d %d %d %d %d %.17g %.17g %.17g %.17g\n", rind[0], rind[1], rind[2], rind[3], rind[4], rind[5], val[0], val[1],
                     val[2], val[3]);
      std::fclose(out);
      params.farkas = 1; // the tree's totals follow the root's line
    } else { // nothing was written and nothing will be appended: the run goes on as without the flag
      std::fprintf(stderr, "--farkas: no report (%d): the root LP's proof could not be asked for, or %s cannot be written; the tree runs unchecked\n",
                   frc, farkas_path.c_str());
    }
    mvx_delete_prob(root);
  }

  mvx_bnb_result res;
  const int brc = mvx_branchAndBound(nullptr, prob, &params, &res);
  if (brc == -1) {
    std::fprintf(stderr, "-vs %d / --heur %d%s%s%s%s%s%s%s%s are not supported with these options (-vs 3 / 4: not with --best-window; --heur: only "
                 "with --repaired; --rcfix / --prop / --dive / --pump / --node-purge / --node-cliques: only with --repaired and without --best-window; --cut-rounds / --polish: only with --repaired)\n",
                 params.var_strat, params.heur, params.rc_fix ? " / --rcfix" : "", params.prop ? " / --prop" : "",
                 params.dive ? " / --dive" : "", params.pump ? " / --pump" : "", params.cut_rounds ? " / --cut-rounds" : "",
                 params.polish ? " / --polish" : "", params.node_purge ? " / --node-purge" : "",
                 params.node_cliques ? " / --node-cliques" : "");
    mvx_delete_prob(prob);
    return -1;
  }
  if (brc != 0)
    std::fprintf(stderr, "branch-and-bound stopped: the branching penalties, the heuristic, the propagation, a pump, a dive, the root cut rounds or the polishing could not be computed, or a purge could not be carried out (%d)\n", brc);
  if (input.CMDOptionExists("--events")) mvx_bnb_write_events(&res, input.getCMDOption("--events").c_str());
  mvx_bnb_print_tree(&res, nullptr); // bs.cpp:329-343
  std::vector<char> buf(64 + 64 * (size_t)res.n);
  mvx_bnb_solution_string(nullptr, prob, &res, buf.data(), (int)buf.size());
  std::printf("\n%s\n", buf.data()); // bs.cpp:345
  if (verbose) std::printf("Solution found after %d iterations (%lld pivots)\n", res.count, res.total_pivots);
  if (verbose && params.var_strat == 4) std::printf("Strong branching: %lld child LPs, %lld pivots\n", res.sb_lps, res.sb_pivots);
  if (verbose && params.heur > 0)
    std::printf("Rounding heuristic: %lld nodes, %lld feasible, %lld improved the incumbent%s\n", res.heur_calls, res.heur_found,
                res.heur_improved, res.incumbent_heur == 1 ? " (the final incumbent is one of them)" : "");
  if (verbose && params.rc_fix > 0)
    std::printf("Reduced-cost tightening: %lld nodes, %lld columns fixed, %lld tightened\n", res.rc_calls, res.rc_fixed, res.rc_tightened);
  if (verbose && params.prop > 0)
    std::printf("Bound propagation: %lld handles, %lld columns fixed, %lld tightened, %lld handles proved infeasible\n", res.prop_calls,
                res.prop_fixed, res.prop_tightened, res.prop_infeasible);
  if (verbose && params.dive > 0)
    std::printf("Diving: %lld nodes, %lld with a feasible point, %lld improved the incumbent, %lld child LPs, %lld pivots%s\n", res.dive_calls,
                res.dive_found, res.dive_improved, res.dive_lps, res.dive_pivots,
                res.incumbent_heur == 2 ? " (the final incumbent is one of them)" : "");
  if (verbose && params.pump > 0)
    std::printf("Feasibility pump: %lld nodes, %lld with a feasible point, %lld improved the incumbent, %lld distance LPs, %lld pivots%s\n",
                res.pump_calls, res.pump_found, res.pump_improved, res.pump_lps, res.pump_pivots,
                res.incumbent_heur == 3 ? " (the final incumbent is one of them)" : "");
  if (verbose && params.cut_rounds > 0)
    std::printf("Root cut rounds: %lld rounds, %lld cuts made, %lld rows appended, %lld LPs, %lld pivots, root LP %.10g -> %.10g\n",
                res.cutloop_rounds, res.cutloop_candidates, res.cutloop_rows, res.cutloop_lps, res.cutloop_pivots, res.cutloop_bound0,
                res.cutloop_bound);
  if (verbose && params.cut_rounds > 0 && (params.cut_families & 2))
    std::printf("Clique cuts: %lld conflicts, %lld violated cliques, %lld rows appended\n", res.cutloop_conflicts, res.cutloop_clique_cands,
                res.cutloop_clique_rows);
  if (verbose && params.cut_rounds > 0 && params.cut_purge > 0)
    std::printf("Cut purging: %lld rows purged, %lld live rows\n", res.cutloop_purged, res.cutloop_live_rows);
  if (verbose && params.polish > 0)
    std::printf("Incumbent polishing: %lld points, %lld moves, %lld came back better\n", res.polish_calls, res.polish_moves,
                res.polish_improved);
  if (verbose && params.node_purge > 0)
    std::printf("Tree cut purging: %lld children purged, %lld rows removed, at most %lld live cut rows on a node\n", res.node_purge_calls,
                res.node_purge_rows, res.node_cut_rows_peak);
  if (verbose && params.node_cliques > 0)
    std::printf("Node cliques: %lld conflicts, %lld nodes separated, %lld rows\n", res.node_clique_conflicts, res.node_clique_calls,
                res.node_clique_rows);
  if (params.kkt > 0) {
    static const char *const cond[4] = {"PE", "PB", "DE", "DB"};
    if (FILE *out = std::fopen(kkt_path.c_str(), "a")) {
      std::fprintf(out, "KKT.NODES %lld\n", res.kkt_nodes);
      for (int c = 0; c < 4; c++) std::fprintf(out, "KKT.TREE.%s %.17g %d\n", cond[c], res.kkt_re[c], res.kkt_oid[c]);
      std::fclose(out);
    } else {
      std::fprintf(stderr, "--kkt: the tree's summary could not be appended to %s\n", kkt_path.c_str());
    }
    if (verbose)
      std::printf("KKT check: %lld nodes, worst relative errors PE %.3g (node %d), PB %.3g (node %d), DE %.3g (node %d), DB %.3g (node %d)\n",
                  res.kkt_nodes, res.kkt_re[0], res.kkt_oid[0], res.kkt_re[1], res.kkt_oid[1], res.kkt_re[2], res.kkt_oid[2], res.kkt_re[3],
                  res.kkt_oid[3]);
  }
  if (params.farkas > 0) {
    if (FILE *out = std::fopen(farkas_path.c_str(), "a")) {
      std::fprintf(out, "FARKAS.NODES %lld\nFARKAS.PROVED %lld\nFARKAS.TABLEAU_ONLY %lld\nFARKAS.NONE %lld\nFARKAS.DROPPED %lld\n", res.farkas_nodes,
                   res.farkas_proved, res.farkas_tableau_only, res.farkas_none, res.farkas_dropped);
      std::fprintf(out, "FARKAS.REL_MIN %.17g %d\nFARKAS.DE_MAX %.17g %d\n", res.farkas_rel_min, res.farkas_rel_oid, res.farkas_de_max,
                   res.farkas_de_oid);
      std::fclose(out);
    } else {
      std::fprintf(stderr, "--farkas: the tree's totals could not be appended to %s\n", farkas_path.c_str());
    }
    if (verbose)
      std::printf("Farkas proofs: %lld infeasible nodes, %lld proved, %lld by the tableau only, %lld without, smallest rel %.3g (node %d), largest de %.3g (node %d)\n",
                  res.farkas_nodes, res.farkas_proved, res.farkas_tableau_only, res.farkas_none, res.farkas_rel_min, res.farkas_rel_oid,
                  res.farkas_de_max, res.farkas_de_oid);
  }
  const int limit = res.hit_limit || brc != 0;
  mvx_bnb_free_result(&res);
  mvx_delete_prob(prob);
  return limit ? -1 : 0;
}
