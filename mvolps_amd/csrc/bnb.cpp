// bnb.cpp -- branch-and-bound driver over the GLPK-shaped LP-engine table (include/mvx_bnb.h).
//
// Host-side mirror of MVOLPS's own control flow, same names and argument meaning:
//   MVOLP::NodeData        util.cpp:25-42     MVOLP::ParameterObj::pickNode/pickVar  util.cpp:154-230
//   printInfo              util.cpp:414-473   getFract                               util.cpp:11-23
//   generateCut3           gmi.cpp:11-117     CutPool::addToPool/addCutConstraint    cut.cpp:6-46
//   branchAndBound         bs.cpp:54-348      getParentOid / getBranchDirection      bs.cpp:26-52
// Every LP call goes through `mvx_lp_api`; with the default table that is the gfx950 engine.
#include <algorithm>
#include <chrono>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <future>
#include <limits>
#include <memory>
#include <set>
#include <unordered_map>
#include <unordered_set>
#include <utility>
#include <vector>

#include "../../include/mvx_bnb.h"
#include "sift_host.hpp"

extern "C" int mvx_classify_many(const mvx_prob *const *Ps, int count, int quirks, int *status, int *nviol, int *viol, double *xviol,
                                 int cap) __attribute__((weak));
extern "C" int mvx_branch_penalties_many(const mvx_prob *const *Ps, int count, const int *cols, const int *col_off, double tol,
                                         double *pen_down, double *pen_up, int *arg_down, int *arg_up) __attribute__((weak));
extern "C" int mvx_get_tableau(const mvx_prob *P, double *out) __attribute__((weak));
extern "C" int mvx_get_basis(const mvx_prob *P, int *head, int *nb, int *flag) __attribute__((weak));
extern "C" void mvx_init_smcp(mvx_smcp *parm) __attribute__((weak));
extern "C" int mvx_round_many(const mvx_prob *root, const mvx_prob *const *Ps, int count, int mode, double *obj, int *found, double *x)
    __attribute__((weak));
extern "C" int mvx_rc_tighten_many(const mvx_prob *const *Ps, int count, const double *cutoff, double tol, int *cnt, int *cols, double *lb,
                                   double *ub) __attribute__((weak));
extern "C" int mvx_tighten_cols_many(mvx_prob *const *Ps, int count, const int *off, const int *cols, const double *lb, const double *ub)
    __attribute__((weak));
extern "C" int mvx_propagate_many(const mvx_prob *root, const mvx_prob *const *Ps, int count, int max_rounds, int *infeasible, int *rounds,
                                  int *cnt, int *cols, double *lb, double *ub) __attribute__((weak));
extern "C" int mvx_set_col_bnds_many(mvx_prob *const *Ps, int count, const int *off, const int *cols, const double *lb, const double *ub)
    __attribute__((weak));
extern "C" int mvx_dive_pick_many(const mvx_prob *root, const mvx_prob *const *Ps, int count, const int *rules, int *nfrac, int *col, int *dir,
                                  double *val)
    __attribute__((weak));
extern "C" int mvx_set_obj_many(mvx_prob *const *Ps, int count, const double *c) __attribute__((weak));
extern "C" int mvx_pump_obj_many(const mvx_prob *root, const mvx_prob *const *Ps, int count, const double *xprev, const int *has_prev,
                                 const double *ab, int *info, double *xt, double *c) __attribute__((weak));

extern "C" int mvx_cut_scores(const mvx_prob *P, int k, const double *vals, double *dot, double *gram) __attribute__((weak));
extern "C" int mvx_add_cut_rows(mvx_prob *P, int k, const double *vals, const double *rhs) __attribute__((weak));
extern "C" int mvx_conflict_graph(const mvx_prob *model, unsigned long long *adj, long long *edges) __attribute__((weak));
extern "C" int mvx_polish_many(const mvx_prob *root, int count, double *x, int max_moves, double *obj, int *moves, int *ok)
    __attribute__((weak));
extern "C" int mvx_del_rows(mvx_prob *P, int nrs, const int *num) __attribute__((weak));
extern "C" int mvx_del_rows_many(mvx_prob *const *Ps, int count, const int *off, const int *rows) __attribute__((weak));
extern "C" const char *mvx_get_col_name(const mvx_prob *P, int j) __attribute__((weak));
extern "C" int mvx_clique_cuts_many(const mvx_prob *root, const mvx_prob *const *Ps, int count, int max_cuts, int *cnt, unsigned long long *q,
                                    double *sum) __attribute__((weak));
extern "C" int mvx_add_cut_rows_many(mvx_prob *const *Ps, int count, const int *off, const double *vals, const double *rhs)
    __attribute__((weak));
extern "C" int mvx_kkt_many(const mvx_prob *root, const mvx_prob *const *Ps, int count, double *val, int *ind) __attribute__((weak));
extern "C" int mvx_farkas_many(const mvx_prob *root, const mvx_prob *const *Ps, int count, double *val, int *ind) __attribute__((weak));

namespace {

struct CutContainer { // cut.h:7-13
  std::vector<int> inds;
  std::vector<double> vals;
  double lb = 0.0;
  int oid = 0;
};

class CutPool { // cut.h:15-23
public:
  explicit CutPool(const mvx_lp_api *api) : _api(api) {}
  int addToPool(CutContainer cut) { // cut.cpp:6-9
    _cuts.push_back(std::move(cut));
    return (int)_cuts.size();
  }
  // the pool keeps only what addCutConstraint can ever read: its last element (cut.cpp:20)
  void replaceLast(CutContainer cut) {
    if (_cuts.empty()) _cuts.push_back(std::move(cut));
    else _cuts.back() = std::move(cut);
  }
  int addCutConstraint(void *in, int cID = -1) { // cut.cpp:11-46
    if (_cuts.empty()) return -1;
    if (cID < 0) cID = (int)_cuts.size() - 1; // cut.cpp:20
    const int index = _api->add_rows(in, 1);
    const CutContainer &sel = _cuts.at((size_t)cID);
    _api->set_mat_row(in, index, (int)sel.inds.size() - 1, sel.inds.data(), sel.vals.data()); // cut.cpp:40
    _api->set_row_bnds(in, index, MVX_LO, sel.lb, 0);                                          // cut.cpp:43
    return cID;
  }
  // the best-bound window speculates a round's cut steps in key order and rolls the pool back to where its replay stopped
  struct Mark {
    size_t size = 0;
    CutContainer last;
  };
  Mark mark() const {
    Mark m;
    m.size = _cuts.size();
    if (!_cuts.empty()) m.last = _cuts.back();
    return m;
  }
  void rollback(const Mark &m) { // addToPool only appends, replaceLast only rewrites the last element
    _cuts.resize(m.size);
    if (!_cuts.empty()) _cuts.back() = m.last;
  }

private:
  const mvx_lp_api *_api;
  std::vector<CutContainer> _cuts;
};

double getFract(double x) { // util.cpp:11-23
  double intPart;
  double fractPart = std::modf(x, &intPart);
  if (fractPart < 0.0) fractPart += 1;
  return fractPart;
}

std::pair<int, std::vector<int>> printInfo(const mvx_lp_api *api, const void *prob, bool quirks) { // util.cpp:414-473
  const int cols = api->get_num_cols(prob);
  std::vector<int> violated;
  const int status = api->get_status(prob);
  if (status == MVX_NOFEAS || status == MVX_INFEAS || status == MVX_UNBND) return {-1, violated}; // util.cpp:424
  std::vector<double> xs;
  if (api->get_col_prim_all) { // one call instead of n through the table
    xs.resize((size_t)cols + 1);
    api->get_col_prim_all(prob, xs.data());
  }
  // this loop runs over every column of every node: trunc / round without a libm call per column (values beyond 2^52
  // are integers; |v - round(v)| = min(|f|, 1 - |f|) with f = v - trunc(v), exact wherever it is near the tolerance)
  auto trunc_of = [](double v) { return std::fabs(v) < 4503599627370496.0 ? (double)(long long)v : v; };
  for (int i = 1; i <= cols; i++) {
    const double v = xs.empty() ? api->get_col_prim(prob, i) : xs[(size_t)i];
    const double t = trunc_of(v);
    if (!quirks) {
      const double f = std::fabs(v - t);
      if ((f < 1.0 - f ? f : 1.0 - f) > 1e-9 && api->get_col_kind(prob, i) != MVX_CV) violated.push_back(i);
      continue;
    }
    if (v != 0 && api->get_obj_coef(prob, i) != 0) {            // util.cpp:437
      if (t != v && api->get_col_kind(prob, i) != MVX_CV) {     // util.cpp:443-444
        violated.push_back(i);
      }
    }
  }
  return {violated.empty() ? 1 : 0, violated};
}

// gmi.cpp:11-117.  oid stays -1 on rejection (gmi.cpp:20,25); on success the reference leaves it
// indeterminate and bs.cpp:252 treats it as "not -1", which is what 0 reproduces.
CutContainer generateCut3(const mvx_lp_api *api, const void *in, int j) {
  CutContainer result;
  double temp = 0.0; // uninitialised at gmi.cpp:13
  const int m = api->get_num_rows(in);
  const int n = api->get_num_cols(in);
  if (api->get_col_kind(in, j) != MVX_IV || api->get_col_stat(in, j) != MVX_BS) {
    result.oid = -1;
    return result;
  }
  std::vector<double> work((size_t)m + n + 1, 0.0), val2((size_t)n + 1, 0.0);
  std::vector<int> ind2((size_t)n + 1, 0);
  const int len = api->eval_tab_row(in, m + j, ind2.data(), val2.data()); // gmi.cpp:36
  double rhs = api->get_col_prim(in, j);                                   // gmi.cpp:37
  for (int i = 1; i <= len; i++) {
    const double val = val2[i];
    int kind;
    double ub;
    if (ind2[i] <= m) { // gmi.cpp:42-47
      kind = MVX_CV;
      ub = api->get_row_ub(in, ind2[i]);
    } else { // gmi.cpp:48-53
      const int curCol = ind2[i] - m;
      kind = api->get_col_kind(in, curCol);
      ub = api->get_col_ub(in, curCol);
    }
    const double fRhs = getFract(rhs); // the RUNNING rhs (gmi.cpp:55,73)
    const double fVal = getFract(val);
    if (kind == MVX_IV) temp = (fRhs >= fVal) ? fVal : (fRhs / (1.0 - fRhs)) * (1.0 - fVal);
    if (kind == MVX_CV) temp = (val >= 0.0) ? val : (fRhs / (1.0 - fRhs)) * (-1.0 * val);
    work[ind2[i]] = -1.0 * temp; // gmi.cpp:72
    rhs -= temp * ub;            // gmi.cpp:73
  }
  // gmi.cpp:81-89: back-substitution indexed by POSITION k in the row's non-zero list
  std::vector<double> rv((size_t)n + 1);
  std::vector<int> ri((size_t)n + 1);
  for (int i = 1; i <= m; i++) {
    // no shortcut for work[i] == 0: an earlier cut of this formula may have left inf / NaN coefficients in the
    // model (gmi.cpp:73 with absent bounds), and 0 * inf is NaN -- bs.cpp goes through every row, so does this
    const int len2 = api->get_mat_row(in, i, ri.data(), rv.data());
    const double wi = work[i];
    for (int k = 1; k <= len2; k++) work[m + k] += wi * rv[k];
  }
  result.inds.resize((size_t)n + 1);
  result.vals.resize((size_t)n + 1);
  result.inds[0] = 0;
  result.vals[0] = rhs;
  for (int i = 1; i <= n; i++) {
    result.inds[i] = i;
    result.vals[i] = work[m + i];
  }
  result.lb = rhs;
  result.oid = 0;
  return result;
}

// Repaired GMI -- see the derivation next to orc_generateCutGMI.
CutContainer generateCutGMI(const mvx_lp_api *api, const void *in, int j, double *efficacy) {
  CutContainer result;
  result.oid = -1;
  const int m = api->get_num_rows(in), n = api->get_num_cols(in);
  if (api->get_col_kind(in, j) == MVX_CV) return result;
  if (api->get_col_stat(in, j) != MVX_BS) return result;
  const double beta = api->get_col_prim(in, j);
  const double f0 = getFract(beta);
  if (f0 < 1e-6 || f0 > 1.0 - 1e-6) return result;
  std::vector<double> val2((size_t)n + 1, 0.0), work((size_t)m + n + 1, 0.0);
  std::vector<int> ind2((size_t)n + 1, 0);
  const int len = api->eval_tab_row(in, m + j, ind2.data(), val2.data());
  double rhs = 1.0;
  for (int t = 1; t <= len; t++) {
    const int k = ind2[t];
    const double alpha = val2[t];
    int stat;
    bool isint;
    double lo, up;
    if (k <= m) {
      stat = api->get_row_stat(in, k);
      isint = false;
      lo = api->get_row_lb(in, k);
      up = api->get_row_ub(in, k);
    } else {
      stat = api->get_col_stat(in, k - m);
      isint = api->get_col_kind(in, k - m) != MVX_CV;
      lo = api->get_col_lb(in, k - m);
      up = api->get_col_ub(in, k - m);
    }
    if (stat == MVX_NS) continue;      // fixed: y_j = 0
    if (stat == MVX_NF) return result; // free non-basic with a non-zero entry: no valid cut
    const double abar = (stat == MVX_NL) ? -alpha : alpha;
    double g;
    if (isint) {
      const double fj = getFract(abar);
      g = (fj <= f0) ? fj / f0 : (1.0 - fj) / (1.0 - f0);
    } else {
      g = (abar >= 0.0) ? abar / f0 : -abar / (1.0 - f0);
    }
    if (stat == MVX_NL) {
      work[k] += g;
      rhs += g * lo;
    } else {
      work[k] -= g;
      rhs -= g * up;
    }
  }
  std::vector<double> rv((size_t)n + 1);
  std::vector<int> ri((size_t)n + 1);
  for (int i = 1; i <= m; i++) {
    if (work[i] == 0.0) continue;
    const int len2 = api->get_mat_row(in, i, ri.data(), rv.data());
    for (int t = 1; t <= len2; t++) work[m + ri[t]] += work[i] * rv[t];
  }
  result.inds.resize((size_t)n + 1);
  result.vals.resize((size_t)n + 1);
  result.inds[0] = 0;
  result.vals[0] = rhs;
  double dot = 0.0, nrm = 0.0;
  for (int k = 1; k <= n; k++) {
    result.inds[k] = k;
    result.vals[k] = work[m + k];
    dot += result.vals[k] * api->get_col_prim(in, k);
    nrm += result.vals[k] * result.vals[k];
  }
  result.lb = rhs;
  if (!(nrm > 0.0)) return result;
  *efficacy = (rhs - dot) / std::sqrt(nrm);
  result.oid = 0;
  return result;
}

namespace MVOLP {
enum PruneType { INTG = 0, FEAS = 1, BNDS = 3, NONE = 4 }; // util.h:27

struct NodeData { // util.h:35-54
  NodeData(const mvx_lp_api *api, const void *parent, int &idCounter) : _api(api) { // util.cpp:25-37
    oid = idCounter;
    idCounter += 1;
    lowerBound = -std::numeric_limits<double>::infinity();
    upperBound = std::numeric_limits<double>::infinity();
    prob = _api->create_prob();
    _api->copy_prob(prob, parent, MVX_ON);
    inital = false;
  }
  // adopts `owned` instead of cloning it: the state a clone would have, without the device-to-device copy
  NodeData(const mvx_lp_api *api, void *owned, int &idCounter, bool /*adopt*/) : _api(api) {
    oid = idCounter;
    idCounter += 1;
    lowerBound = -std::numeric_limits<double>::infinity();
    upperBound = std::numeric_limits<double>::infinity();
    prob = owned;
    inital = false;
  }
  ~NodeData() {
    if (prob) _api->delete_prob(prob); // util.cpp:39-42
  }
  NodeData(const NodeData &) = delete;
  NodeData &operator=(const NodeData &) = delete;
  double upperBound, lowerBound;
  void *prob;
  bool inital;
  int oid;
  int repiv = -1; // window driver: pivots of the pop-time re-solve (bs.cpp:117) when it was done ahead, else -1
  // node_purge > 0: one age per row behind the caller's rows, ascending (255: a dead row, purged as a free row), and their number
  std::vector<unsigned char> age;
  int dead = 0;

private:
  const mvx_lp_api *_api;
};

// +1: compare bounds as a maximiser (bs.cpp:172,210 always do); -1: repaired mode on a minimisation problem
inline double sense_of(const mvx_lp_api *api, const void *prob, const mvx_bnb_params &p) {
  return (p.reference_quirks == 0 && api->get_obj_dir && api->get_obj_dir(prob) == MVX_MIN) ? -1.0 : 1.0;
}

class ParameterObj { // util.h:61-99
public:
  ParameterObj(const mvx_lp_api *api, const void *prob, const mvx_bnb_params &p)
      : _api(api), _prob(prob), _p(p), _sg(sense_of(api, prob, p)) {}
  double sense() const { return _sg; }
  bool IsCutEnabled() const { return _p.cut_strat != 0; }

  std::shared_ptr<NodeData> pickNode(const std::deque<std::shared_ptr<NodeData>> &problems, int &index) const { // util.cpp:154-188
    if (_p.node_strat == 0) { // "DFS" == FIFO
      index = 0;
      return problems.front();
    }
    index = 0;
    for (int i = 1; i < (int)problems.size(); i++)
      if (_sg * problems[(size_t)index]->upperBound < _sg * problems[(size_t)i]->upperBound) index = i; // first maximum
    return problems.at((size_t)index);
  }

  int pickVar(const std::vector<int> &vars) const { // util.cpp:190-230
    if (_p.var_strat == 0) return vars.front();
    if (_p.var_strat == 1) {
      // util.cpp:200-203 query _prob, the ROOT problem that is never solved
      double curBest = std::fabs(getFract(_api->get_col_prim(_prob, vars.front())) - 0.5);
      int index = vars.front();
      for (int i : vars) {
        const double cur = std::fabs(getFract(_api->get_col_prim(_prob, i)) - 0.5);
        if (cur < curBest) {
          curBest = cur;
          index = i;
        }
      }
      return index;
    }
    double bestCoef = 0.0;
    int index = vars.front(); // uninitialised in the reference when no coefficient is > 0
    for (int i : vars) {
      const double cur = _api->get_obj_coef(_prob, i);
      if (cur > bestCoef) {
        bestCoef = cur;
        index = i;
      }
    }
    return index;
  }

private:
  const mvx_lp_api *_api;
  const void *_prob;
  mvx_bnb_params _p;
  double _sg;
};
} // namespace MVOLP

int getBranchDirection(int oid) { // bs.cpp:43-52
  if (oid <= 1) return 0;
  return (oid % 2 == 0) ? 1 : 2;
}

struct Recorder {
  std::vector<int> parent, prune;
  std::vector<double> bound;
  std::vector<mvx_bnb_event> events;
  std::vector<mvx_bnb_event> *sink = nullptr; // window mode buffers events per node
  long long pivots = 0;
  void node(int oid, int pid) {
    if ((int)parent.size() <= oid) {
      parent.resize((size_t)oid + 1, 0);
      prune.resize((size_t)oid + 1, MVOLP::NONE);
      bound.resize((size_t)oid + 1, std::numeric_limits<double>::infinity());
    }
    parent[(size_t)oid] = pid;
  }
  void emit(int type, int oid, double f6, double f7, int f8, int pick) {
    mvx_bnb_event e;
    e.type = type;
    e.oid = oid;
    e.pid = parent[(size_t)oid]; // getParentOid, bs.cpp:26-33
    e.direction = getBranchDirection(oid);
    e.lp_bound = f6;
    e.sum_infeas = f7;
    e.n_violated = f8;
    e.pick = pick;
    (sink ? *sink : events).push_back(e);
  }
};

int solve(const mvx_lp_api *api, void *p, Recorder &rec) {
  const int before = api->get_it_cnt(p);
  const int rc = api->simplex(p, nullptr); // the reference ignores the return code
  rec.pivots += api->get_it_cnt(p) - before;
  return rc;
}

template <typename T>
T *dup(const std::vector<T> &v) {
  T *p = (T *)std::malloc(sizeof(T) * (v.empty() ? 1 : v.size()));
  if (!v.empty()) std::memcpy(p, v.data(), sizeof(T) * v.size());
  return p;
}

// A node's cuts through the engine's batch entry (mvx_lp_api.gmi_cuts): `cols` are the candidate columns (each one
// basic and integer, checked by the caller the way gmi.cpp:18-27 / the repaired filter do); returns one container per
// column, oid -1 where the engine found no cut.
static std::vector<CutContainer> cuts_via_engine(const mvx_lp_api *api, const void *a, bool repaired, const std::vector<int> &cols,
                                                 std::vector<double> *eff) {
  const int n = api->get_num_cols(a), k = (int)cols.size();
  std::vector<double> vals((size_t)k * (n + 1)), rhs((size_t)k);
  std::vector<int> ok((size_t)k, 0);
  std::vector<CutContainer> out((size_t)k);
  if (api->gmi_cuts(a, repaired ? 1 : 0, cols.data(), k, vals.data(), rhs.data(), ok.data()) != 0) {
    for (auto &c : out) c.oid = -1;
    return out;
  }
  std::vector<double> x;
  if (repaired) {
    x.resize((size_t)n + 1);
    for (int j = 1; j <= n; j++) x[(size_t)j] = api->get_col_prim(a, j);
  }
  for (int t = 0; t < k; t++) {
    CutContainer &c = out[(size_t)t];
    if (!ok[(size_t)t]) {
      c.oid = -1;
      continue;
    }
    const double *v = &vals[(size_t)t * (n + 1)];
    c.inds.resize((size_t)n + 1);
    c.vals.assign(v, v + n + 1);
    for (int j = 0; j <= n; j++) c.inds[(size_t)j] = j;
    c.lb = rhs[(size_t)t];
    c.oid = 0;
    if (repaired) { // efficacy as generateCutGMI computes it
      double dot = 0.0, nrm = 0.0;
      for (int j = 1; j <= n; j++) {
        dot += c.vals[(size_t)j] * x[(size_t)j];
        nrm += c.vals[(size_t)j] * c.vals[(size_t)j];
      }
      if (!(nrm > 0.0)) {
        c.oid = -1;
        continue;
      }
      if (eff) (*eff)[(size_t)t] = (c.lb - dot) / std::sqrt(nrm);
    }
  }
  return out;
}

// generateCutGMI's own rejections that need no tableau row (the rest is the engine's ok flag)
static bool gmi_candidate(const mvx_lp_api *api, const void *a, int j) {
  if (api->get_col_kind(a, j) == MVX_CV || api->get_col_stat(a, j) != MVX_BS) return false;
  const double f0 = getFract(api->get_col_prim(a, j));
  return !(f0 < 1e-6 || f0 > 1.0 - 1e-6);
}

// The lazy cut modes generate ONE cut per branching node (cut.cpp:20 only ever appends the last one): a window of 64
// nodes means 64 tableau-row reads and 64 O(m n) back-substitutions on the host, one node after the other, while the
// device idles -- that loop, not the LP solves, bounded the cut path (1.7 k nodes/s against 15 k without cuts).  Here the
// cuts of a whole round are made in one device pass (mvx_lp_api.gmi_cuts_many): for every node of the window that
// may branch, the column the host loop would settle on -- bug-compatible: the last basic integer column (gmi.cpp:18-27);
// repaired: the last column generateCutGMI would not reject out of hand -- and one launch pair for all of them.  Same
// bits as generateCut3 / generateCutGMI (tests/test_gpu_gmi.py); a node whose cut the engine rejects (ok = 0, zero
// norm) gets nullptr and goes through the host loop as before.
static std::vector<std::unique_ptr<CutContainer>> round_cuts(const mvx_lp_api *api, const std::vector<void *> &nodes, const std::vector<char> &wanted,
                                                              const mvx_bnb_params &prm, bool quirks) {
  std::vector<std::unique_ptr<CutContainer>> out(nodes.size());
  if (!api->gmi_cuts_many || prm.cut_strat == 0 || !prm.lazy_pool || (!quirks && prm.cut_select != 0)) return out;
  std::vector<const void *> ps;
  std::vector<int> cols;
  std::vector<size_t> slot;
  for (size_t w = 0; w < nodes.size(); w++) {
    if (!wanted[w]) continue;
    const void *a = nodes[w];
    const int na = api->get_num_cols(a);
    for (int j = na; j >= 1; j--) {
      const bool cand = quirks ? (api->get_col_kind(a, j) == MVX_IV && api->get_col_stat(a, j) == MVX_BS) : gmi_candidate(api, a, j);
      if (cand) {
        ps.push_back(a);
        cols.push_back(j);
        slot.push_back(w);
        break;
      }
    }
  }
  const int k = (int)ps.size();
  if (k < 2) return out; // a single cut: the host loop is as fast
  const int n = api->get_num_cols(ps[0]);
  std::vector<double> vals((size_t)k * (n + 1)), rhs((size_t)k);
  std::vector<int> ok((size_t)k, 0);
  const int grc = api->gmi_cuts_many(ps.data(), quirks ? 0 : 1, cols.data(), k, vals.data(), rhs.data(), ok.data());
  if (grc != 0) {
    if (std::getenv("MVX_BNB_TIMING")) std::fprintf(stderr, "round_cuts: gmi_cuts_many returned %d for %d cuts\n", grc, k);
    return out;
  }
  for (int t = 0; t < k; t++) {
    if (!ok[(size_t)t]) continue;
    const double *v = &vals[(size_t)t * (n + 1)];
    if (!quirks) { // generateCutGMI rejects a cut without coefficients
      double nrm = 0.0;
      for (int j = 1; j <= n; j++) nrm += v[j] * v[j];
      if (!(nrm > 0.0)) continue;
    }
    auto c = std::make_unique<CutContainer>();
    c->inds.resize((size_t)n + 1);
    c->vals.assign(v, v + n + 1);
    for (int j = 0; j <= n; j++) c->inds[(size_t)j] = j;
    c->lb = rhs[(size_t)t];
    c->oid = 0;
    out[slot[(size_t)t]] = std::move(c);
  }
  return out;
}

// Cut step of a branching node (bs.cpp:249-258), shared by both drivers: bug-compatible mode feeds the
// persistent pool and appends its last cut (cut.cpp:16-21); repaired mode appends this node's own GMI cuts,
// chosen by cut_select / -cf.
// Returns the number of rows appended; -1 when the bug-compatible path found its pool empty (nothing generated yet).
// `pre`: the one cut the lazy modes would generate for this node, already made by round_cuts (nullptr: make it here).
static double g_t_cut_scan = 0, g_t_cut_copy = 0, g_t_cut_add = 0; // MVX_BNB_TIMING: parts of add_node_cuts (window driver's thread only)
static double cut_now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static int add_node_cuts(const mvx_lp_api *api, void *a, const mvx_bnb_params &prm, bool quirks, CutPool &pool, const CutContainer *pre = nullptr) {
  if (prm.cut_strat == 0) return 0;
  const int na = api->get_num_cols(a);
  const bool dev = api->gmi_cuts != nullptr;
  if (quirks) {
    if (prm.lazy_pool) {
      // only the pool's LAST cut is ever added (cut.cpp:20): generate just that one
      const double t0 = cut_now();
      for (int j = na; j >= 1; j--) {
        if (api->get_col_kind(a, j) == MVX_IV && api->get_col_stat(a, j) == MVX_BS) {
          // one cut: the host loop (one row read, one back-substitution) is as fast as a device pass with its set-up
          const double t1 = cut_now();
          g_t_cut_scan += t1 - t0;
          pool.replaceLast(pre ? *pre : generateCut3(api, a, j));
          g_t_cut_copy += cut_now() - t1;
          break;
        }
      }
    } else if (dev) {
      std::vector<int> cols;
      for (int j = 1; j <= na; j++)
        if (api->get_col_kind(a, j) == MVX_IV && api->get_col_stat(a, j) == MVX_BS) cols.push_back(j); // gmi.cpp:18-27
      if (!cols.empty())
        for (auto &c : cuts_via_engine(api, a, false, cols, nullptr))
          if (c.oid != -1) pool.addToPool(std::move(c));
    } else {
      for (int j = 1; j <= na; j++) {
        CutContainer result = generateCut3(api, a, j);
        if (result.oid != -1) pool.addToPool(std::move(result));
      }
    }
    const double t2 = cut_now();
    const int rc = pool.addCutConstraint(a) < 0 ? -1 : 1;
    g_t_cut_add += cut_now() - t2;
    return rc;
  }
  std::vector<CutContainer> local;
  std::vector<double> eff;
  if (prm.cut_select == 0 && prm.lazy_pool && pre) {
    const double t1 = cut_now();
    local.push_back(*pre);
    eff.push_back(0.0);
    g_t_cut_copy += cut_now() - t1;
  } else if (prm.cut_select == 0 && prm.lazy_pool) {
    // only the last cut generated would be appended (cut.cpp:20): find it from the far end instead of
    // generating one cut per basic integer column (each is a tableau row read + an O(m n) back-substitution)
    for (int j = na; j >= 1 && local.empty(); j--) {
      double e = 0.0;
      CutContainer c = generateCutGMI(api, a, j, &e); // one cut: host loop (2 437 against 1 880 nodes/s through the device pass)
      if (c.oid != -1) {
        local.push_back(std::move(c));
        eff.push_back(e);
      }
    }
  } else if (dev) {
    std::vector<int> cols;
    for (int j = 1; j <= na; j++)
      if (gmi_candidate(api, a, j)) cols.push_back(j);
    if (!cols.empty()) {
      std::vector<double> e(cols.size(), 0.0);
      std::vector<CutContainer> all = cuts_via_engine(api, a, true, cols, &e);
      for (size_t t = 0; t < all.size(); t++)
        if (all[t].oid != -1) {
          local.push_back(std::move(all[t]));
          eff.push_back(e[t]);
        }
    }
  } else {
    for (int j = 1; j <= na; j++) {
      double e = 0.0;
      CutContainer c = generateCutGMI(api, a, j, &e);
      if (c.oid != -1) {
        local.push_back(std::move(c));
        eff.push_back(e);
      }
    }
  }
  if (local.empty()) return 0;
  int take = 1;
  if (prm.cut_select == 1) {
    take = (int)std::ceil(prm.cut_chance * (double)local.size());
    take = std::max(1, std::min(take, (int)local.size()));
  }
  std::vector<char> used(local.size(), 0);
  for (int t = 0; t < take; t++) {
    int best = -1;
    if (prm.cut_select == 0) best = (int)local.size() - 1; // cut.cpp:20: the last one
    else
      for (int q = 0; q < (int)local.size(); q++)
        if (!used[(size_t)q] && (best < 0 || eff[(size_t)q] > eff[(size_t)best])) best = q; // ties: first generated
    used[(size_t)best] = 1;
    const CutContainer &cc = local[(size_t)best];
    const double t2 = cut_now();
    const int index = api->add_rows(a, 1);
    api->set_mat_row(a, index, (int)cc.inds.size() - 1, cc.inds.data(), cc.vals.data());
    api->set_row_bnds(a, index, MVX_LO, cc.lb, 0);
    g_t_cut_add += cut_now() - t2;
  }
  return take;
}


// ---- branching on the node LP (var_strat 3 / 4, DESIGN.md "Branching on the node LP") ----

// The bounds the two children of a branching on `pick` at value `bound` get (bs.cpp:274,282; repaired mode keeps the
// opposite bound): S2 the down child, S3 the up child.  Every driver, strong branching and mvx_bnb_make_children use it.
// `a` is the branching node; the window driver's up child has adopted a's handle, so S3 may be `a` itself: the node's type
// and bounds are all read before the first write, and that order has to stay.
static void child_bounds(const mvx_lp_api *api, const void *a, int pick, double bound, bool quirks, void *S2, void *S3) {
  if (quirks) {
    api->set_col_bnds(S2, pick, MVX_UP, 0, std::floor(bound)); // bs.cpp:274
    api->set_col_bnds(S3, pick, MVX_LO, std::ceil(bound), 0);  // bs.cpp:282
    return;
  }
  const int t = api->get_col_type(a, pick);
  const double l = api->get_col_lb(a, pick), u = api->get_col_ub(a, pick);
  if (t == MVX_LO || t == MVX_DB || t == MVX_FX)
    api->set_col_bnds(S2, pick, (l == std::floor(bound)) ? MVX_FX : MVX_DB, l, std::floor(bound));
  else
    api->set_col_bnds(S2, pick, MVX_UP, 0, std::floor(bound));
  if (t == MVX_UP || t == MVX_DB || t == MVX_FX)
    api->set_col_bnds(S3, pick, (u == std::ceil(bound)) ? MVX_FX : MVX_DB, std::ceil(bound), u);
  else
    api->set_col_bnds(S3, pick, MVX_LO, std::ceil(bound), 0);
}

// One-step dual penalties of basic columns of one solved handle from its exported tableau and basis: the host twin of
// k_penalty, same tests, same division, same strict minimum over ascending positions -- the same bits.
static int host_penalties(const mvx_lp_api *api, const void *P, const int *cols, int count, double tol, double *pd, double *pu, int *ad,
                          int *au) {
  if (!P || count < 0 || (count > 0 && (!cols || !pd || !pu || !ad || !au))) return -1;
  const int m = api->get_num_rows(P), n = api->get_num_cols(P);
  for (int k = 0; k < count; k++)
    if (cols[k] < 1 || cols[k] > n) return -1;
  if (api->get_status(P) != MVX_OPT) return -3;
  if (count == 0) return 0;
  if (!api->get_tableau || !api->get_basis) return -5;
  std::vector<double> T((size_t)(m + 1) * (size_t)(n + 1));
  std::vector<int> head((size_t)m + 1), nb((size_t)n + 1), flag((size_t)n + 1);
  if (api->get_basis(P, head.data(), nb.data(), flag.data()) != 0 || api->get_tableau(P, T.data()) != 0) return -5;
  std::vector<int> rowof((size_t)n + 1, 0);
  for (int i = 1; i <= m; i++)
    if (head[(size_t)i] > m && head[(size_t)i] <= m + n) rowof[(size_t)(head[(size_t)i] - m)] = i;
  for (int k = 0; k < count; k++)
    if (rowof[(size_t)cols[k]] == 0) return -4;
  const double inf = std::numeric_limits<double>::infinity();
  const double *r0 = T.data();
  for (int k = 0; k < count; k++) {
    const double *ri = &T[(size_t)rowof[(size_t)cols[k]] * (size_t)(n + 1)];
    double bd = inf, bu = inf;
    int qd = 0, qu = 0;
    for (int q = 1; q <= n; q++) {
      const double e = ri[q];
      if (!(std::fabs(e) > tol)) continue;
      const int f = flag[(size_t)q];
      const bool inc = f == MVX_NL || f == MVX_NF, dec = f == MVX_NU || f == MVX_NF; // allowed directions s = +1 / -1
      const bool down = (inc && e < 0.0) || (dec && e > 0.0);
      const bool up = (inc && e > 0.0) || (dec && e < 0.0);
      if (!down && !up) continue;
      const double r = std::fabs(r0[q]) / std::fabs(e);
      if (down && r < bd) {
        bd = r;
        qd = q;
      }
      if (up && r < bu) {
        bu = r;
        qu = q;
      }
    }
    const double v = ri[0];
    const double fd = v - std::floor(v), fu = std::ceil(v) - v;
    pd[k] = qd ? fd * bd : inf;
    pu[k] = qu ? fu * bu : inf;
    ad[k] = qd;
    au[k] = qu;
  }
  return 0;
}

// pivot tolerance of the engine's default solve (mvx_init_smcp), passed to the penalty tests; an smcp with the defaults
static mvx_smcp default_smcp() {
  mvx_smcp p;
  p.msg_lev = 0;
  p.meth = 1;
  p.it_lim = -1;
  p.tol_bnd = p.tol_dj = p.tol_piv = 1e-9; // the engine's defaults (mvx.h)
  if (mvx_init_smcp) mvx_init_smcp(&p);
  return p;
}

inline double pen_score(double d, double u) { return std::max(d, 1e-6) * std::max(u, 1e-6); }

// What var_strat 3 / 4 decide for one branching node, and the strong-branching work it took (booked only if it branches).
struct Choice {
  int pick = 0;
  long long sb_lps = 0, sb_pivots = 0;
};

// Penalties of the basic candidates of several solved nodes: one branch_penalties_many call when the table has it, else
// the host twin per node.  Columns that are not basic (a fractional value at a fractional bound) keep 0 / 0.
static int penalties_of(const mvx_lp_api *api, const std::vector<const void *> &hs, const std::vector<std::vector<int>> &cands, double tol,
                        std::vector<std::vector<double>> &pd, std::vector<std::vector<double>> &pu) {
  const size_t K = hs.size();
  pd.assign(K, {});
  pu.assign(K, {});
  std::vector<const void *> ps;
  std::vector<int> cols, off(1, 0);
  std::vector<std::vector<size_t>> where(K);
  for (size_t t = 0; t < K; t++) {
    pd[t].assign(cands[t].size(), 0.0);
    pu[t].assign(cands[t].size(), 0.0);
    for (size_t k = 0; k < cands[t].size(); k++)
      if (api->get_col_stat(hs[t], cands[t][k]) == MVX_BS) {
        cols.push_back(cands[t][k]);
        where[t].push_back(k);
      }
    if (where[t].empty()) continue;
    ps.push_back(hs[t]);
    off.push_back((int)cols.size());
  }
  if (cols.empty()) return 0;
  std::vector<double> d(cols.size()), u(cols.size());
  std::vector<int> ad(cols.size()), au(cols.size());
  if (api->branch_penalties_many) {
    const int rc = api->branch_penalties_many(ps.data(), (int)ps.size(), cols.data(), off.data(), tol, d.data(), u.data(), ad.data(), au.data());
    if (rc != 0) return rc;
  } else {
    for (size_t p = 0; p < ps.size(); p++) {
      const int rc = host_penalties(api, ps[p], cols.data() + off[p], off[p + 1] - off[p], tol, d.data() + off[p], u.data() + off[p],
                                    ad.data() + off[p], au.data() + off[p]);
      if (rc != 0) return rc;
    }
  }
  size_t g = 0;
  for (size_t t = 0; t < K; t++)
    for (size_t k : where[t]) {
      pd[t][k] = d[g];
      pu[t][k] = u[g];
      g++;
    }
  return 0;
}

// Bytes of child tableaux one strong-branching batch may hold (MVX_SB_BUDGET_MB overrides; results do not depend on it).
static size_t sb_budget() {
  size_t mb = 4096;
  if (const char *e = std::getenv("MVX_SB_BUDGET_MB")) mb = (size_t)std::max(0, std::atoi(e));
  return mb << 20;
}

// `count` jobs in batches whose tableaux (`per_job` each) fit the strong-branching memory budget: advance(j0, j1) per batch,
// until one fails; its code.  Results do not depend on the cut.
template <typename F>
static int in_batches(const mvx_lp_api *api, const void *h0, size_t count, size_t per_job, F advance) {
  const size_t tab = (size_t)(api->get_num_rows(h0) + 1) * (size_t)(api->get_num_cols(h0) + 1) * 8;
  const size_t per = std::max<size_t>(1, std::min(count, sb_budget() / (per_job * tab + 1)));
  for (size_t j0 = 0; j0 < count; j0 += per) {
    const int rc = advance(j0, std::min(count, j0 + per));
    if (rc != 0) return rc;
  }
  return 0;
}

// hs solved together: simplex_batch where the table has it, else simplex per handle; the pivots of hs[k]
static std::vector<int> solve_counted(const mvx_lp_api *api, const std::vector<void *> &hs, const mvx_smcp *parm) {
  std::vector<int> pivots(hs.size());
  for (size_t k = 0; k < hs.size(); k++) pivots[k] = api->get_it_cnt(hs[k]);
  if (api->simplex_batch) api->simplex_batch(const_cast<void **>(hs.data()), (int)hs.size(), parm, nullptr);
  else
    for (void *h : hs) api->simplex(h, parm);
  for (size_t k = 0; k < hs.size(); k++) pivots[k] = api->get_it_cnt(hs[k]) - pivots[k];
  return pivots;
}

// var_strat 3 / 4 for a set of branching nodes: hs[t] solved (OPT), vars[t] its printInfo violated list (ascending).
// 3: the argmax of max(pen_down, 1e-6) * max(pen_up, 1e-6), ties to the lowest column.  4: the sb_cands best candidates by
// that score (same tie rule) are branched on clones with the drivers' own bounds, all their children solved by batched
// solves of at most sb_iters pivots each; each side's degradation is max(penalty, objective drop in the LP's own sense)
// (+inf for a NOFEAS child), scored by the same product.  The pick depends on each node's own LP only.
static int choose_many(const mvx_lp_api *api, const std::vector<const void *> &hs, const std::vector<std::vector<int>> &vars,
                       const mvx_bnb_params &prm, std::vector<Choice> &out) {
  const size_t K = hs.size();
  out.assign(K, Choice());
  if (K == 0) return 0;
  const mvx_smcp dflt = default_smcp();
  std::vector<std::vector<double>> pd, pu;
  const int rc = penalties_of(api, hs, vars, dflt.tol_piv, pd, pu);
  if (rc != 0) return rc;
  const bool quirks = prm.reference_quirks != 0;
  // candidates of each node in score order (descending, ties to the lower column: vars is ascending and the sort stable)
  std::vector<std::vector<size_t>> order(K);
  for (size_t t = 0; t < K; t++) {
    std::vector<size_t> &o = order[t];
    for (size_t k = 0; k < vars[t].size(); k++) o.push_back(k);
    std::stable_sort(o.begin(), o.end(), [&](size_t x, size_t y) { return pen_score(pd[t][x], pu[t][x]) > pen_score(pd[t][y], pu[t][y]); });
    if (!o.empty()) out[t].pick = vars[t][o.front()];
  }
  if (prm.var_strat != 4 || prm.sb_cands <= 0) return 0;
  // strong branching: children of the top candidates, solved in batches that fit the memory budget
  struct Job {
    size_t t, k;
    void *S2, *S3;
  };
  std::vector<Job> jobs;
  for (size_t t = 0; t < K; t++)
    for (size_t r = 0; r < order[t].size() && (int)r < prm.sb_cands; r++) jobs.push_back(Job{t, order[t][r], nullptr, nullptr});
  std::vector<double> dd(jobs.size()), du(jobs.size());
  mvx_smcp parm = dflt;
  parm.it_lim = std::max(0, prm.sb_iters);
  in_batches(api, hs[0], jobs.size(), 2, [&](size_t j0, size_t j1) {
    std::vector<void *> kids;
    for (size_t j = j0; j < j1; j++) {
      Job &jb = jobs[j];
      const void *a = hs[jb.t];
      const int col = vars[jb.t][jb.k];
      jb.S2 = api->create_prob();
      jb.S3 = api->create_prob();
      api->copy_prob(jb.S2, a, MVX_ON);
      api->copy_prob(jb.S3, a, MVX_ON);
      child_bounds(api, a, col, api->get_col_prim(a, col), quirks, jb.S2, jb.S3);
      kids.push_back(jb.S2);
      kids.push_back(jb.S3);
    }
    const std::vector<int> pivots = solve_counted(api, kids, &parm);
    for (size_t j = j0; j < j1; j++) {
      Job &jb = jobs[j];
      const void *a = hs[jb.t];
      const double lpsg = (api->get_obj_dir && api->get_obj_dir(a) == MVX_MIN) ? -1.0 : 1.0;
      const double z = api->get_obj_val(a);
      auto delta = [&](void *S, double pen) {
        if (api->get_status(S) == MVX_NOFEAS) return std::numeric_limits<double>::infinity();
        return std::max(pen, lpsg * (z - api->get_obj_val(S)));
      };
      dd[j] = delta(jb.S2, pd[jb.t][jb.k]);
      du[j] = delta(jb.S3, pu[jb.t][jb.k]);
      Choice &ch = out[jb.t];
      ch.sb_lps += 2;
      ch.sb_pivots += pivots[2 * (j - j0)] + pivots[2 * (j - j0) + 1];
      api->delete_prob(jb.S2);
      api->delete_prob(jb.S3);
    }
    return 0;
  });
  // best strong-branching score per node; ties to the lowest column
  std::vector<double> best(K, -1.0);
  for (size_t j = 0; j < jobs.size(); j++) {
    const Job &jb = jobs[j];
    const double sc = pen_score(dd[j], du[j]);
    const int col = vars[jb.t][jb.k];
    if (best[jb.t] < 0.0 || sc > best[jb.t] || (sc == best[jb.t] && col < out[jb.t].pick)) {
      best[jb.t] = sc;
      out[jb.t].pick = col;
    }
  }
  return 0;
}

// ---- the host model and the device-or-twin route (DESIGN.md "Host model, device flags and adoption") ----

struct RcEntry {
  int col;
  double lb, ub;
};
using RcList = std::vector<RcEntry>;

// The model the host twins work on, read from a handle through the table in one pass over its rows: rows 1..m0 with their
// non-zeros in ascending column order (and by column, ascending row), row and column bounds (+-inf where absent), which
// columns are integer and locked down / up by some row, and how many rows lock a column down / up.  `priced`: the table also
// has the objective and the column values of a solved handle, and c and sg are filled; the rounding family needs that part,
// propagation and the conflict graph do not.
struct HostModel {
  int m0 = 0, n = 0;
  bool priced = false;
  double sg = 1.0;
  std::vector<std::vector<std::pair<int, double>>> rows, cols; // rows[i-1]: (j, a_ij) ascending j; cols[j]: (i-1, a_ij) ascending i
  std::vector<double> rlo, rhi, clo, chi, c;
  std::vector<char> isint, dlock, ulock;
  std::vector<int> dl, ul; // rows that lock column j down / up
};

static double tab_bound(double b) { // the table reports an absent bound as -+DBL_MAX (GLPK)
  const double inf = std::numeric_limits<double>::infinity();
  return b <= -DBL_MAX ? -inf : b >= DBL_MAX ? inf : b;
}
static double round_tol(double b) { return 1e-9 * std::max(1.0, std::fabs(b)); } // a row bound's feasibility tolerance

// ---- sensitivity ranges (DESIGN.md "Sensitivity ranges (ranges)") ----

// What the ranges and their report read of a solved handle: the packed tableau, the basis and the bounds by variable number
struct RangeView {
  int m = 0, n = 0, maxdir = 1;
  std::vector<double> T, lb, ub; // T (m+1) x (n+1); lb / ub [m+n+1], +-inf when absent
  std::vector<int> head, nb, flag;
};

static bool has_view_accessors(const mvx_lp_api *api) {
  return api->get_tableau && api->get_basis && api->get_row_lb && api->get_row_ub && api->get_col_lb && api->get_col_ub && api->get_status &&
         api->get_num_rows && api->get_num_cols;
}

// the tableau, basis and bounds of a handle whatever its status (the table has the accessors: has_view_accessors); 0, or -2 when
// get_basis / get_tableau failed
static int read_tableau_view(const mvx_lp_api *api, const void *P, RangeView &V) {
  const int m = V.m = api->get_num_rows(P), n = V.n = api->get_num_cols(P);
  V.maxdir = (api->get_obj_dir && api->get_obj_dir(P) == MVX_MIN) ? 0 : 1;
  V.T.assign((size_t)(m + 1) * (size_t)(n + 1), 0.0);
  V.head.assign((size_t)m + 1, 0);
  V.nb.assign((size_t)n + 1, 0);
  V.flag.assign((size_t)n + 1, 0);
  if (api->get_basis(P, V.head.data(), V.nb.data(), V.flag.data()) != 0 || api->get_tableau(P, V.T.data()) != 0) return -2;
  V.lb.assign((size_t)m + n + 1, 0.0);
  V.ub.assign((size_t)m + n + 1, 0.0);
  for (int i = 1; i <= m; i++) {
    V.lb[(size_t)i] = tab_bound(api->get_row_lb(P, i));
    V.ub[(size_t)i] = tab_bound(api->get_row_ub(P, i));
  }
  for (int j = 1; j <= n; j++) {
    V.lb[(size_t)(m + j)] = tab_bound(api->get_col_lb(P, j));
    V.ub[(size_t)(m + j)] = tab_bound(api->get_col_ub(P, j));
  }
  return 0;
}

// 0; -2 an accessor is missing or failed; -3 the handle is not MVX_OPT
static int read_range_view(const mvx_lp_api *api, const void *P, RangeView &V) {
  if (!has_view_accessors(api)) return -2;
  if (api->get_status(P) != MVX_OPT) return -3;
  return read_tableau_view(api, P, V);
}

// The host twin of k_rangecols / k_rangefin / k_rangerows: the same tests, the same divisions, one walk over ascending rows
// (part A) and ascending positions (part B) with a strict compare -- the same bits.
static void host_ranges(const RangeView &V, double tol, double *val, int *var) {
  const int m = V.m, n = V.n;
  const size_t ldt = (size_t)n + 1;
  const double inf = std::numeric_limits<double>::infinity();
  std::fill(val, val + (size_t)(m + n + 1) * 6, 0.0);
  std::fill(var, var + (size_t)(m + n + 1) * 4, 0);
  const double *r0 = V.T.data();
  for (int q = 1; q <= n; q++) { // part A
    double tu = inf, td = inf;
    int iu = 0, id = 0;
    for (int i = 1; i <= m; i++) {
      const double e = V.T[(size_t)i * ldt + (size_t)q];
      const double ae = std::fabs(e);
      if (!(ae > tol)) continue;
      const double beta = V.T[(size_t)i * ldt];
      const double lb = V.lb[(size_t)V.head[(size_t)i]], ub = V.ub[(size_t)V.head[(size_t)i]];
      const double su = std::fmax(ub - beta, 0.0), sl = std::fmax(beta - lb, 0.0);
      const bool hu = ub != inf, hl = lb != -inf, pos = e > 0.0;
      if (pos ? hu : hl) {
        const double t = (pos ? su : sl) / ae;
        if (t < tu) {
          tu = t;
          iu = i;
        }
      }
      if (pos ? hl : hu) {
        const double t = (pos ? sl : su) / ae;
        if (t < td) {
          td = t;
          id = i;
        }
      }
    }
    const int k = V.nb[(size_t)q], f = V.flag[(size_t)q];
    const double d = std::fabs(r0[q]);
    const bool lo = f == MVX_NL || f == MVX_NF, hi = f == MVX_NU || f == MVX_NF;
    const bool cu = V.maxdir ? lo : hi, cd = V.maxdir ? hi : lo;
    const double none = d > 0.0 ? inf : 0.0;
    double *v = val + (size_t)k * 6;
    int *w = var + (size_t)k * 4;
    v[0] = td;
    v[1] = tu;
    v[2] = td == inf ? none : d * td;
    v[3] = tu == inf ? none : d * tu;
    v[4] = cd ? d : inf;
    v[5] = cu ? d : inf;
    w[0] = id ? V.head[(size_t)id] : 0;
    w[1] = iu ? V.head[(size_t)iu] : 0;
  }
  for (int i = 1; i <= m; i++) { // part B
    const double *ri = &V.T[(size_t)i * ldt];
    double bd = inf, bu = inf;
    int qd = 0, qu = 0;
    for (int q = 1; q <= n; q++) {
      const double e = ri[q];
      if (!(std::fabs(e) > tol)) continue;
      const int f = V.flag[(size_t)q];
      const bool inc = f == MVX_NL || f == MVX_NF, dec = f == MVX_NU || f == MVX_NF;
      const bool down = (inc && e < 0.0) || (dec && e > 0.0);
      const bool up = (inc && e > 0.0) || (dec && e < 0.0);
      if (!down && !up) continue;
      const double r = std::fabs(r0[q]) / std::fabs(e);
      if (down && r < bd) {
        bd = r;
        qd = q;
      }
      if (up && r < bu) {
        bu = r;
        qu = q;
      }
    }
    const int k = V.head[(size_t)i];
    const int vd = qd ? V.nb[(size_t)qd] : 0, vu = qu ? V.nb[(size_t)qu] : 0;
    double *v = val + (size_t)k * 6;
    int *w = var + (size_t)k * 4;
    v[4] = V.maxdir ? bd : bu;
    v[5] = V.maxdir ? bu : bd;
    w[2] = V.maxdir ? vd : vu;
    w[3] = V.maxdir ? vu : vd;
  }
}

// ---- KKT check (DESIGN.md "KKT check (kkt)") ----

// sum over k = 1..cnt of a(k) * v[k] in the order of mvx_price_cols' S: 64 chains, chain l taking k = l+1, l+65, ... ascending with
// fma from +0.0, combined by s[l] += s[l+h], h = 32 .. 1.  Zeros are not skipped
template <typename A>
static double kkt_chain_sum(int cnt, A a, const double *v) {
  double s[64];
  for (int l = 0; l < 64; l++) {
    double acc = 0.0;
    for (int k = l + 1; k <= cnt; k += 64) acc = std::fma(a(k), v[k], acc);
    s[l] = acc;
  }
  for (int h = 32; h >= 1; h >>= 1)
    for (int l = 0; l < h; l++) s[l] = s[l] + s[l + h];
  return s[0];
}

// a maximum with a strict compare over ascending indices: the lowest index among equals, 0 while the maximum is 0
struct KktMax {
  double v = 0.0;
  int i = 0;
  void see(double w, int k) {
    if (w > v) {
      v = w;
      i = k;
    }
  }
};

// The host twin of k_kkt_rows / k_kkt_cols / k_kkt_fin from numbers only: rows m x (n+1) dense (entry 0 of each unused), c[0..n],
// xs / dj [0..n], xr / lam [0..m], lb / ub / stat [0..m+n] by variable (+-inf where absent), sg +1 minimise / -1 maximise
static void kkt_host(int m, int n, const double *rows, const double *c, const double *xs, const double *xr, const double *lam, const double *dj,
                     const double *lb, const double *ub, const int *stat, double sg, double *val, int *ind, double *r_pe, double *r_de) {
  const size_t ldr = (size_t)n + 1;
  const double inf = std::numeric_limits<double>::infinity();
  KktMax mx[8];
  if (r_pe) r_pe[0] = 0.0;
  if (r_de) r_de[0] = 0.0;
  for (int i = 1; i <= m; i++) { // PE
    const double *ai = rows + (size_t)(i - 1) * ldr;
    const double s = kkt_chain_sum(n, [&](int j) { return ai[j]; }, xs);
    const double r = xr[i] - s, ae = std::fabs(r);
    if (r_pe) r_pe[i] = r;
    mx[0].see(ae, i);
    mx[1].see(ae / (1.0 + std::fabs(xr[i])), i);
  }
  for (int j = 1; j <= n; j++) { // DE
    const double t = kkt_chain_sum(m, [&](int i) { return rows[(size_t)(i - 1) * ldr + (size_t)j]; }, lam);
    const double r = (c[j] - t) - dj[j], ae = std::fabs(r);
    if (r_de) r_de[j] = r;
    mx[4].see(ae, j);
    mx[5].see(ae / (1.0 + std::fabs(c[j])), j);
  }
  for (int k = 1; k <= m + n; k++) { // PB, DB
    const double x = k <= m ? xr[k] : xs[k - m], d = k <= m ? lam[k] : dj[k - m];
    const double l = lb[k], u = ub[k];
    double ae = 0.0, re = 0.0;
    if (std::fabs(l) != inf && x < l) {
      ae = l - x;
      re = ae / (1.0 + std::fabs(l));
    } else if (std::fabs(u) != inf && x > u) {
      ae = x - u;
      re = ae / (1.0 + std::fabs(u));
    }
    mx[2].see(ae, k);
    mx[3].see(re, k);
    const double e = sg * d;
    double v;
    switch (stat[k]) {
      case MVX_NL: v = -e > 0.0 ? -e : 0.0; break;
      case MVX_NU: v = e > 0.0 ? e : 0.0; break;
      case MVX_NF: v = std::fabs(e); break;
      case MVX_NS: v = 0.0; break;
      default: v = std::fabs(d); break;
    }
    mx[6].see(v, k);
    mx[7].see(v / (1.0 + std::fabs(d)), k);
  }
  for (int t = 0; t < 8; t++) {
    val[t] = mx[t].v;
    ind[t] = mx[t].i;
  }
}

// The twin through the table: the model's rows, bounds and objective, and the four value vectors by the getters' own rule out of
// get_tableau and get_basis -- column 0 where a variable is basic, the bound its status names (0 for MVX_NF) where it is not;
// row 0 at a non-basic variable's position, 0 for a basic one.  0; -2 an accessor is missing or failed; -3 MVX_UNDEF
static int kkt_through_table(const mvx_lp_api *api, const void *P, double *val, int *ind, double *r_pe, double *r_de) {
  if (!api->get_mat_row || !api->get_obj_coef || !has_view_accessors(api)) return -2;
  if (api->get_status(P) == MVX_UNDEF) return -3; // every state a solve leaves behind will do
  RangeView V;
  const int rc = read_tableau_view(api, P, V);
  if (rc != 0) return rc;
  const int m = V.m, n = V.n;
  const size_t ldr = (size_t)n + 1;
  std::vector<double> rows((size_t)m * ldr, 0.0), c(ldr, 0.0), xs(ldr, 0.0), dj(ldr, 0.0), xr((size_t)m + 1, 0.0), lam((size_t)m + 1, 0.0);
  std::vector<int> stat((size_t)m + n + 1, 0), idx(ldr);
  std::vector<double> buf(ldr);
  for (int i = 1; i <= m; i++) {
    const int len = api->get_mat_row(P, i, idx.data(), buf.data());
    for (int k = 1; k <= len; k++) rows[(size_t)(i - 1) * ldr + (size_t)idx[(size_t)k]] = buf[(size_t)k];
  }
  for (int j = 1; j <= n; j++) c[(size_t)j] = api->get_obj_coef(P, j);
  auto put = [&](int k, double x, double d, int s) {
    (k <= m ? xr[(size_t)k] : xs[(size_t)(k - m)]) = x;
    (k <= m ? lam[(size_t)k] : dj[(size_t)(k - m)]) = d;
    stat[(size_t)k] = s;
  };
  for (int i = 1; i <= m; i++) put(V.head[(size_t)i], V.T[(size_t)i * ldr], 0.0, MVX_BS);
  for (int q = 1; q <= n; q++) {
    const int k = V.nb[(size_t)q], f = V.flag[(size_t)q];
    const double x = f == MVX_NL ? V.lb[(size_t)k] : f == MVX_NU ? V.ub[(size_t)k] : f == MVX_NS ? V.lb[(size_t)k] : 0.0;
    put(k, x, V.T[(size_t)q], f);
  }
  kkt_host(m, n, rows.data(), c.data(), xs.data(), xr.data(), lam.data(), dj.data(), V.lb.data(), V.ub.data(), stat.data(),
           V.maxdir ? -1.0 : 1.0, val, ind, r_pe, r_de);
  return 0;
}

// The rule's state for one tree: the route to the check (the table's kkt_many over `model`, the twin without the entry) and
// what the tree reports -- the nodes checked, the worst re_max per condition and the lowest oid it occurred at.
class KktCheck {
public:
  KktCheck(const mvx_lp_api *api, const void *model, int on) : _api(api), _model(model), _on(on > 0) {}
  bool on() const { return _on; }
  // val[8 t ..] of the solved handles hs; 0, or the failing call's code
  int compute(const std::vector<const void *> &hs, std::vector<double> &val) {
    val.assign(hs.size() * 8, 0.0);
    if (hs.empty()) return 0;
    std::vector<int> ind(hs.size() * 8, 0);
    if (_api->kkt_many) return _api->kkt_many(_model, hs.data(), (int)hs.size(), val.data(), ind.data());
    for (size_t t = 0; t < hs.size(); t++) {
      const int rc = kkt_through_table(_api, hs[t], &val[t * 8], &ind[t * 8], nullptr, nullptr);
      if (rc != 0) return rc;
    }
    return 0;
  }
  // a solved node books its result, in the order the serial loop meets the nodes
  void book(const double *val, int oid) {
    _nodes++;
    for (int c = 0; c < 4; c++) {
      const double re = val[2 * c + 1];
      if (re > _re[c] || (re == _re[c] && re > 0.0 && oid < _oid[c])) { // the lowest oid among equals, 0 while nothing is violated
        _re[c] = re;
        _oid[c] = oid;
      }
    }
  }
  void store(mvx_bnb_result *res) const {
    res->kkt_nodes = _nodes;
    for (int c = 0; c < 4; c++) {
      res->kkt_re[c] = _re[c];
      res->kkt_oid[c] = _oid[c];
    }
  }

private:
  const mvx_lp_api *_api;
  const void *_model;
  const bool _on;
  long long _nodes = 0;
  double _re[4] = {0.0, 0.0, 0.0, 0.0};
  int _oid[4] = {0, 0, 0, 0};
};

// ---- Farkas proof (DESIGN.md "Infeasibility and unboundedness proofs (farkas)") ----

constexpr double FARKAS_Z = 1e-9;   // a coefficient this small on a variable without the bound it needs is taken for zero
constexpr double FARKAS_REL = 1e-9; // a side proves when its rel exceeds this

// one side (lower: Lo, upper: Hi) of the interval rule: the sum of the finite terms, the sum of their absolute values, the terms
// that make the side infinite and those the zero rule dropped
struct FarkasSide {
  double sum = 0.0, act = 0.0;
  int inf = 0, drop = 0;
  void term(double f, double b) { // b: the bound this side takes of the variable
    if (std::fabs(b) == std::numeric_limits<double>::infinity()) {
      if (std::fabs(f) <= FARKAS_Z) drop++;
      else inf++;
      b = 0.0;
    }
    sum = std::fma(f, b, sum);
    act = std::fma(std::fabs(f), std::fabs(b), act);
  }
};

struct FarkasInterval {
  double lo, hi, rel_lo, rel_hi; // hi is Hi itself; rel_hi = -Hi / (1 + act_hi)
  int inf_lo, inf_hi, drop_lo, drop_hi;
};

// The interval rule I(f) over p = first..last, f(p) with bounds l(p), u(p): 64 chains, chain c taking p = first + c, first + c + 64,
// ... ascending with fma from +0.0, combined by s[c] += s[c+h], h = 32 .. 1; an exact zero takes part with the bound 0
template <typename F, typename L, typename U>
static FarkasInterval farkas_interval(int first, int last, F f, L l, U u) {
  FarkasSide lo[64], hi[64];
  for (int c = 0; c < 64; c++)
    for (int p = first + c; p <= last; p += 64) {
      const double fp = f(p);
      double bl = fp < 0.0 ? u(p) : l(p), bh = fp < 0.0 ? l(p) : u(p);
      if (fp == 0.0) bl = bh = 0.0;
      lo[c].term(fp, bl);
      hi[c].term(fp, bh);
    }
  for (int h = 32; h >= 1; h >>= 1)
    for (int c = 0; c < h; c++) {
      lo[c].sum = lo[c].sum + lo[c + h].sum; lo[c].act = lo[c].act + lo[c + h].act;
      hi[c].sum = hi[c].sum + hi[c + h].sum; hi[c].act = hi[c].act + hi[c + h].act;
      lo[c].inf += lo[c + h].inf; lo[c].drop += lo[c + h].drop;
      hi[c].inf += hi[c + h].inf; hi[c].drop += hi[c + h].drop;
    }
  const double ninf = -std::numeric_limits<double>::infinity();
  FarkasInterval r;
  r.lo = lo[0].sum; r.hi = hi[0].sum;
  r.inf_lo = lo[0].inf; r.inf_hi = hi[0].inf; r.drop_lo = lo[0].drop; r.drop_hi = hi[0].drop;
  r.rel_lo = r.inf_lo == 0 ? r.lo / (1.0 + lo[0].act) : ninf;
  r.rel_hi = r.inf_hi == 0 ? -r.hi / (1.0 + hi[0].act) : ninf;
  return r;
}

// The host twin of k_farkas_rows / k_farkas_pick / k_farkas_vars / k_farkas_cols / k_farkas_fin from numbers only: T (m+1) x (n+1) the
// tableau as get_tableau packs it (x_B(i) = sum_q T[i][q] x_N(q): eval_tab_row's alpha; row 0 and column 0 are not read), head[0..m]
// / nb[0..n] the basis, rows m x (n+1) dense, lb / ub [0..m+n] by variable.  y (nullable) [0..m]
static void farkas_host(int m, int n, const double *T, const int *head, const int *nb, const double *rows, const double *lb, const double *ub,
                        double *val, int *ind, double *y) {
  const size_t ldr = (size_t)n + 1;
  for (int t = 0; t < 4; t++) {
    val[t] = 0.0;
    ind[t] = 0;
  }
  if (y) std::fill(y, y + m + 1, 0.0);
  // 1. the tableau side: every row's form f^i over p = 0 (its basic variable, coefficient 1) and p = q (-alpha_iq)
  double best = FARKAS_REL;
  int bi = 0, bside = 0;
  for (int i = 1; i <= m; i++) {
    const double *Ti = T + (size_t)i * ldr;
    const FarkasInterval I = farkas_interval(
        0, n, [&](int p) { return p == 0 ? 1.0 : -Ti[p]; }, [&](int p) { return lb[(size_t)(p == 0 ? head[i] : nb[p])]; },
        [&](int p) { return ub[(size_t)(p == 0 ? head[i] : nb[p])]; });
    if (I.rel_lo > best) { best = I.rel_lo; bi = i; bside = 1; }
    if (I.rel_hi > best) { best = I.rel_hi; bi = i; bside = 2; }
  }
  if (bi == 0) return;
  // 2. the form by variable: y its part over the auxiliaries, z over the structurals
  std::vector<double> f((size_t)m + n + 1, 0.0), g((size_t)m + n + 1, 0.0);
  f[(size_t)head[bi]] = 1.0;
  for (int q = 1; q <= n; q++) f[(size_t)nb[q]] = -T[(size_t)bi * ldr + (size_t)q];
  // 3. the model side: w = A'y in the order of the KKT check's t_j, g = (y, -w)
  KktMax de;
  for (int r = 1; r <= m; r++) g[(size_t)r] = f[(size_t)r];
  for (int j = 1; j <= n; j++) {
    const double w = kkt_chain_sum(m, [&](int r) { return rows[(size_t)(r - 1) * ldr + (size_t)j]; }, f.data());
    const double gj = -w, z = f[(size_t)(m + j)];
    g[(size_t)(m + j)] = gj;
    de.see(std::fabs(gj - z) / (1.0 + std::fabs(z)), j);
  }
  const FarkasInterval I = farkas_interval(
      1, m + n, [&](int k) { return g[(size_t)k]; }, [&](int k) { return lb[(size_t)k]; }, [&](int k) { return ub[(size_t)k]; });
  const bool upper = I.rel_hi > I.rel_lo; // the lower side before the upper
  const double rel = upper ? I.rel_hi : I.rel_lo;
  const int inf = upper ? I.inf_hi : I.inf_lo;
  val[0] = best;
  val[1] = rel;
  val[2] = inf != 0 ? -std::numeric_limits<double>::infinity() : upper ? -I.hi : I.lo;
  val[3] = de.v;
  ind[0] = rel > FARKAS_REL ? 2 : 1;
  ind[1] = bi;
  ind[2] = bside;
  ind[3] = upper ? I.drop_hi : I.drop_lo;
  if (y) std::copy(f.begin(), f.begin() + m + 1, y);
}

// The twin through the table: tableau, basis and bounds as the ranges read them, the rows by get_mat_row.  0; -2 an accessor is
// missing or failed; -3 MVX_UNDEF
static int farkas_through_table(const mvx_lp_api *api, const void *P, double *val, int *ind, double *y) {
  if (!api->get_mat_row || !has_view_accessors(api)) return -2;
  if (api->get_status(P) == MVX_UNDEF) return -3;
  RangeView V;
  const int rc = read_tableau_view(api, P, V);
  if (rc != 0) return rc;
  const int m = V.m, n = V.n;
  const size_t ldr = (size_t)n + 1;
  std::vector<double> rows((size_t)m * ldr, 0.0), buf(ldr);
  std::vector<int> idx(ldr);
  for (int i = 1; i <= m; i++) {
    const int len = api->get_mat_row(P, i, idx.data(), buf.data());
    for (int k = 1; k <= len; k++) rows[(size_t)(i - 1) * ldr + (size_t)idx[(size_t)k]] = buf[(size_t)k];
  }
  farkas_host(m, n, V.T.data(), V.head.data(), V.nb.data(), rows.data(), V.lb.data(), V.ub.data(), val, ind, y);
  return 0;
}

// ---- the unbounded ray (same section of DESIGN.md) ----

constexpr double RAY_TOL = 1e-9; // the published dual must improve by more than this

// The host twin of k_ray_cols / k_ray_pick / k_ray_vars / k_ray_rows / k_ray_fin from numbers only: T (m+1) x (n+1) as get_tableau
// packs it (row 0 the published duals of the non-basic positions), head / nb / flag the basis, rows m x (n+1) dense, c[0..n], lb /
// ub [0..m+n] by variable, sg +1 minimise / -1 maximise.  val[4] = the dual, ae, re, the slope; ind[6] = found, the variable, the
// direction, the blocking variables, the rows of ae and re; d (nullable) [0..m+n]
static void ray_host(int m, int n, const double *T, const int *head, const int *nb, const int *flag, const double *rows, const double *c,
                     const double *lb, const double *ub, double sg, double *val, int *ind, double *d) {
  const size_t ldr = (size_t)n + 1;
  const double inf = std::numeric_limits<double>::infinity();
  for (int t = 0; t < 4; t++) val[t] = 0.0;
  for (int t = 0; t < 6; t++) ind[t] = 0;
  if (d) std::fill(d, d + m + n + 1, 0.0);
  // 1. the lowest position whose move improves the objective and that nothing in the tableau stops
  int qp = 0;
  double sp = 0.0;
  for (int q = 1; q <= n && qp == 0; q++) {
    const double e = sg * T[q];
    const int f = flag[q];
    double sigma = 0.0;
    if (e < -RAY_TOL && (f == MVX_NL || f == MVX_NF)) sigma = 1.0;
    else if (e > RAY_TOL && (f == MVX_NU || f == MVX_NF)) sigma = -1.0;
    if (sigma == 0.0) continue;
    const int k = nb[q];
    if (sigma > 0.0 ? ub[(size_t)k] != inf : lb[(size_t)k] != -inf) continue;
    bool open = true;
    for (int i = 1; i <= m && open; i++) {
      const double a = T[(size_t)i * ldr + (size_t)q], mv = sigma * a;
      if (std::fabs(a) <= FARKAS_Z) continue;
      open = mv > 0.0 ? ub[(size_t)head[i]] == inf : lb[(size_t)head[i]] == -inf;
    }
    if (open) {
      qp = q;
      sp = sigma;
    }
  }
  if (qp == 0) return;
  // 2. the ray by variable
  std::vector<double> r((size_t)m + n + 1, 0.0);
  r[(size_t)nb[qp]] = sp;
  for (int i = 1; i <= m; i++) r[(size_t)head[i]] = sp * T[(size_t)i * ldr + (size_t)qp];
  // 3. against the model: rho_r = dR_r - a_r dS in the order of the KKT check's s_i, the slope c dS, the bounds in the way
  KktMax ae, re;
  const double *ds = r.data() + m;
  for (int i = 1; i <= m; i++) {
    const double *ai = rows + (size_t)(i - 1) * ldr;
    const double rho = r[(size_t)i] - kkt_chain_sum(n, [&](int j) { return ai[j]; }, ds), a = std::fabs(rho);
    ae.see(a, i);
    re.see(a / (1.0 + std::fabs(r[(size_t)i])), i);
  }
  const double slope = kkt_chain_sum(n, [&](int j) { return c[j]; }, ds);
  int blocked = 0;
  for (int k = 1; k <= m + n; k++) {
    const double v = r[(size_t)k];
    if (std::fabs(v) <= FARKAS_Z) continue; // the zero rule
    if (v > 0.0 ? ub[(size_t)k] != inf : lb[(size_t)k] != -inf) blocked++;
  }
  val[0] = T[qp];
  val[1] = ae.v;
  val[2] = re.v;
  val[3] = slope;
  ind[0] = (sg * slope < 0.0 && re.v <= RAY_TOL && blocked == 0) ? 2 : 1;
  ind[1] = nb[qp];
  ind[2] = sp > 0.0 ? 1 : -1;
  ind[3] = blocked;
  ind[4] = ae.i;
  ind[5] = re.i;
  if (d) std::copy(r.begin(), r.end(), d);
  if (d) d[0] = 0.0;
}

// The twin through the table.  0; -2 an accessor is missing or failed; -3 MVX_UNDEF
static int ray_through_table(const mvx_lp_api *api, const void *P, double *val, int *ind, double *d) {
  if (!api->get_mat_row || !api->get_obj_coef || !has_view_accessors(api)) return -2;
  if (api->get_status(P) == MVX_UNDEF) return -3;
  RangeView V;
  const int rc = read_tableau_view(api, P, V);
  if (rc != 0) return rc;
  const int m = V.m, n = V.n;
  const size_t ldr = (size_t)n + 1;
  std::vector<double> rows((size_t)m * ldr, 0.0), buf(ldr), c(ldr, 0.0);
  std::vector<int> idx(ldr);
  for (int i = 1; i <= m; i++) {
    const int len = api->get_mat_row(P, i, idx.data(), buf.data());
    for (int k = 1; k <= len; k++) rows[(size_t)(i - 1) * ldr + (size_t)idx[(size_t)k]] = buf[(size_t)k];
  }
  for (int j = 1; j <= n; j++) c[(size_t)j] = api->get_obj_coef(P, j);
  ray_host(m, n, V.T.data(), V.head.data(), V.nb.data(), V.flag.data(), rows.data(), c.data(), V.lb.data(), V.ub.data(),
           V.maxdir ? -1.0 : 1.0, val, ind, d);
  return 0;
}

// The rule's state for one tree: the route to the proof (the table's farkas_many over `model`, the twin without the entry) and what
// the tree reports of its MVX_NOFEAS node LPs
class FarkasCheck {
public:
  FarkasCheck(const mvx_lp_api *api, const void *model, int on) : _api(api), _model(model), _on(on > 0) {}
  bool on() const { return _on; }
  // val[4 t ..], ind[4 t ..] of the handles hs; 0, or the failing call's code
  int compute(const std::vector<const void *> &hs, std::vector<double> &val, std::vector<int> &ind) {
    val.assign(hs.size() * 4, 0.0);
    ind.assign(hs.size() * 4, 0);
    if (hs.empty()) return 0;
    if (_api->farkas_many) return _api->farkas_many(_model, hs.data(), (int)hs.size(), val.data(), ind.data());
    for (size_t t = 0; t < hs.size(); t++) {
      const int rc = farkas_through_table(_api, hs[t], &val[t * 4], &ind[t * 4], nullptr);
      if (rc != 0) return rc;
    }
    return 0;
  }
  // a MVX_NOFEAS node books its result, in the order the serial loop meets the nodes
  void book(const double *val, const int *ind, int oid) {
    _nodes++;
    if (ind[0] == 2) {
      if (_proved == 0 || val[1] < _rel || (val[1] == _rel && oid < _rel_oid)) { // the lowest oid among equals
        _rel = val[1];
        _rel_oid = oid;
      }
      _proved++;
    } else if (ind[0] == 1) {
      _tableau_only++;
    } else {
      _none++;
    }
    if (ind[0] > 0) {
      if (ind[3] > 0) _dropped++;
      if (val[3] > _de || (val[3] == _de && val[3] > 0.0 && oid < _de_oid)) {
        _de = val[3];
        _de_oid = oid;
      }
    }
  }
  void store(mvx_bnb_result *res) const {
    res->farkas_nodes = _nodes;
    res->farkas_proved = _proved;
    res->farkas_tableau_only = _tableau_only;
    res->farkas_none = _none;
    res->farkas_dropped = _dropped;
    res->farkas_rel_min = _rel;
    res->farkas_de_max = _de;
    res->farkas_rel_oid = _rel_oid;
    res->farkas_de_oid = _de_oid;
  }

private:
  const mvx_lp_api *_api;
  const void *_model;
  const bool _on;
  long long _nodes = 0, _proved = 0, _tableau_only = 0, _none = 0, _dropped = 0;
  double _rel = 0.0, _de = 0.0;
  int _rel_oid = 0, _de_oid = 0;
};

// 0, or -2 when the table lacks an accessor of the rows, the bounds or the column kinds
static int read_host_model(const mvx_lp_api *api, const void *root, HostModel &M) {
  if (!api->get_mat_row || !api->get_row_lb || !api->get_row_ub || !api->get_col_lb || !api->get_col_ub || !api->get_col_kind) return -2;
  const int m0 = api->get_num_rows(root), n = api->get_num_cols(root);
  M.m0 = m0;
  M.n = n;
  M.rows.assign((size_t)m0, {});
  M.cols.assign((size_t)n + 1, {});
  M.rlo.resize((size_t)m0);
  M.rhi.resize((size_t)m0);
  M.clo.resize((size_t)n + 1);
  M.chi.resize((size_t)n + 1);
  M.isint.assign((size_t)n + 1, 0);
  M.dlock.assign((size_t)n + 1, 0);
  M.ulock.assign((size_t)n + 1, 0);
  M.dl.assign((size_t)n + 1, 0);
  M.ul.assign((size_t)n + 1, 0);
  std::vector<int> ind((size_t)n + 1);
  std::vector<double> val((size_t)n + 1);
  for (int i = 1; i <= m0; i++) {
    const int len = api->get_mat_row(root, i, ind.data(), val.data());
    auto &row = M.rows[(size_t)i - 1];
    for (int k = 1; k <= len; k++)
      if (val[(size_t)k] != 0.0) row.emplace_back(ind[(size_t)k], val[(size_t)k]);
    std::sort(row.begin(), row.end());
    const double lo = tab_bound(api->get_row_lb(root, i)), up = tab_bound(api->get_row_ub(root, i));
    M.rlo[(size_t)i - 1] = lo;
    M.rhi[(size_t)i - 1] = up;
    for (const auto &e : row) {
      M.cols[(size_t)e.first].emplace_back(i - 1, e.second);
      if ((e.second > 0.0 && std::isfinite(lo)) || (e.second < 0.0 && std::isfinite(up))) {
        M.dlock[(size_t)e.first] = 1;
        M.dl[(size_t)e.first]++;
      }
      if ((e.second > 0.0 && std::isfinite(up)) || (e.second < 0.0 && std::isfinite(lo))) {
        M.ulock[(size_t)e.first] = 1;
        M.ul[(size_t)e.first]++;
      }
    }
  }
  for (int j = 1; j <= n; j++) {
    M.clo[(size_t)j] = tab_bound(api->get_col_lb(root, j));
    M.chi[(size_t)j] = tab_bound(api->get_col_ub(root, j));
    M.isint[(size_t)j] = api->get_col_kind(root, j) != MVX_CV;
  }
  M.priced = api->get_obj_coef && api->get_status && (api->get_col_prim_all || api->get_col_prim);
  if (M.priced) {
    M.sg = (api->get_obj_dir && api->get_obj_dir(root) == MVX_MIN) ? -1.0 : 1.0;
    M.c.resize((size_t)n + 1);
    for (int j = 0; j <= n; j++) M.c[(size_t)j] = api->get_obj_coef(root, j);
  }
  return 0;
}

// The model of one handle, read on first use.  A tree owns one for its `model` handle and its rules borrow it.
struct LazyModel {
  const mvx_lp_api *api;
  const void *root;
  LazyModel(const mvx_lp_api *api_, const void *root_) : api(api_), root(root_) {}
  // 0 and the model, or the reader's code
  int get(const HostModel *&M) {
    if (!_ready) {
      const int rc = read_host_model(api, root, _M);
      if (rc != 0) return rc;
      _ready = true;
    }
    M = &_M;
    return 0;
  }

private:
  bool _ready = false;
  HostModel _M;
};

// One rule's route to its results: the table's batched entry while it accepts the model, the host twin (same bits) without the
// entry or, once the entry has answered -5 (the kernel's size limit), for the rest of the tree.  `device()` makes the call and
// unpacks its arrays, `twin(M)` loops over the handles; 0, or the failing call's code.  The flag is the rule's own.
class DeviceOrTwin {
public:
  template <typename D, typename T>
  int run(bool has_entry, LazyModel &lm, D device, T twin) {
    if (has_entry && _device) {
      const int rc = device();
      if (rc != -5) return rc;
      _device = false;
    }
    const HostModel *M = nullptr;
    const int rc = lm.get(M);
    if (rc != 0) return rc;
    return twin(*M);
  }

private:
  bool _device = true;
};

// lists[k] one behind the other: list k is entries off[k] .. off[k+1]-1
struct FlatLists {
  std::vector<int> off, cols;
  std::vector<double> lb, ub;
  explicit FlatLists(const std::vector<const RcList *> &lists) : off(1, 0) {
    for (const RcList *l : lists) {
      for (const RcEntry &e : *l) {
        cols.push_back(e.col);
        lb.push_back(e.lb);
        ub.push_back(e.ub);
      }
      off.push_back((int)cols.size());
    }
  }
};
static void list_out(const RcList &l, int *cnt, int *cols, double *lb, double *ub) {
  *cnt = (int)l.size();
  for (size_t k = 0; k < l.size(); k++) {
    cols[k] = l[k].col;
    lb[k] = l[k].lb;
    ub[k] = l[k].ub;
  }
}
static RcList list_in(int cnt, const int *cols, const double *lb, const double *ub) {
  RcList l;
  for (int k = 0; k < cnt; k++) l.push_back(RcEntry{cols[k], lb[k], ub[k]});
  return l;
}

// ---- primal rounding heuristic (heur 1 / 2, DESIGN.md "Primal rounding heuristic") ----

// The heuristic on one solved node (the host twin of k_round, same operations in the same order): x[0..n] gets the
// candidate, *obj its objective, *found whether it is feasible.
static int round_host(const mvx_lp_api *api, const HostModel &M, const void *P, int mode, double *obj, int *found, double *x) {
  if (!M.priced) return -2;
  const int n = M.n, m0 = M.m0;
  if (mode < 1 || mode > 2 || !obj || !found || !x || api->get_num_cols(P) != n) return -1;
  if (api->get_status(P) != MVX_OPT) return -3;
  std::vector<double> v((size_t)n + 1, 0.0);
  if (api->get_col_prim_all) api->get_col_prim_all(P, v.data());
  else
    for (int j = 1; j <= n; j++) v[(size_t)j] = api->get_col_prim(P, j);
  std::vector<double> xt((size_t)n + 1, 0.0), r((size_t)m0, 0.0);
  for (int j = 1; j <= n; j++) {
    const double vj = v[(size_t)j];
    double xr = vj;
    if (M.isint[(size_t)j]) {
      const double ri = std::rint(vj);
      if (std::fabs(vj - ri) <= 1e-9) xr = ri;
      else if (!M.dlock[(size_t)j]) xr = std::floor(vj);
      else if (!M.ulock[(size_t)j]) xr = std::ceil(vj);
      else xr = std::floor(vj + 0.5);
      const double lo = std::ceil(M.clo[(size_t)j]), hi = std::floor(M.chi[(size_t)j]);
      if (xr < lo) xr = lo;
      if (xr > hi) xr = hi;
    }
    xt[(size_t)j] = xr;
  }
  for (int i = 0; i < m0; i++) {
    double acc = 0.0;
    for (const auto &e : M.rows[(size_t)i])
      if (xt[(size_t)e.first] != 0.0) acc = acc + e.second * xt[(size_t)e.first];
    r[(size_t)i] = acc;
  }
  auto feasible = [&]() {
    for (int j = 1; j <= n; j++)
      if (!(M.clo[(size_t)j] <= xt[(size_t)j] && xt[(size_t)j] <= M.chi[(size_t)j])) return false;
    for (int i = 0; i < m0; i++) {
      const double lo = M.rlo[(size_t)i], hi = M.rhi[(size_t)i];
      if (!(r[(size_t)i] >= lo - round_tol(lo) && r[(size_t)i] <= hi + round_tol(hi))) return false;
    }
    return true;
  };
  bool ok = feasible();
  if (ok && mode == 2) {
    std::vector<int> order;
    for (int j = 1; j <= n; j++)
      if (M.isint[(size_t)j]) order.push_back(j);
    std::vector<double> key((size_t)n + 1, 0.0);
    for (int j : order) key[(size_t)j] = v[(size_t)j] - std::floor(v[(size_t)j]);
    std::sort(order.begin(), order.end(), [&](int p, int q) { return key[(size_t)p] > key[(size_t)q] || (key[(size_t)p] == key[(size_t)q] && p < q); });
    const double inf = std::numeric_limits<double>::infinity();
    for (int j : order) {
      const double sc = M.sg * M.c[(size_t)j];
      if (!(sc != 0.0)) continue;
      const double d = sc > 0.0 ? 1.0 : -1.0;
      double q = inf;
      for (const auto &e : M.cols[(size_t)j]) {
        const double da = d * e.second;
        const int i = e.first;
        if (da > 0.0 && std::isfinite(M.rhi[(size_t)i])) {
          const double hi = M.rhi[(size_t)i];
          q = std::min(q, ((hi + round_tol(hi)) - r[(size_t)i]) / da);
        } else if (da < 0.0 && std::isfinite(M.rlo[(size_t)i])) {
          const double lo = M.rlo[(size_t)i];
          q = std::min(q, ((r[(size_t)i] - lo) + round_tol(lo)) / -da);
        }
      }
      const double room = d > 0.0 ? std::floor(M.chi[(size_t)j]) - xt[(size_t)j] : xt[(size_t)j] - std::ceil(M.clo[(size_t)j]);
      const double tt = std::min(room, std::floor(q));
      if (!(tt > 0.0) || std::isinf(tt)) continue; // no room, or nothing limits the column
      const double step = d * tt;
      for (const auto &e : M.cols[(size_t)j]) r[(size_t)e.first] = r[(size_t)e.first] + step * e.second;
      xt[(size_t)j] = xt[(size_t)j] + step;
    }
    ok = feasible();
  }
  double sum = 0.0;
  for (int j = 1; j <= n; j++) sum = sum + M.c[(size_t)j] * xt[(size_t)j];
  *obj = sum + M.c[0];
  *found = ok ? 1 : 0;
  for (int j = 1; j <= n; j++) x[j] = xt[(size_t)j];
  return 0;
}

// One tree's heuristic: round_many (one call for a batch of nodes) when the table has it and the model fits the kernel,
// else the host twin on the tree's model.  Results depend on each node's own LP only.
struct HeurOut {
  double obj = 0.0;
  int found = 0;
  std::vector<double> x; // [0..n]
};

class Heuristic {
public:
  Heuristic(LazyModel &lm, int mode) : _lm(lm), _mode(mode) {}
  // hs: solved (OPT) nodes; 0, or the failing call's code
  int run(const std::vector<const void *> &hs, std::vector<HeurOut> &out) {
    const mvx_lp_api *api = _lm.api;
    const size_t K = hs.size(), row = (size_t)api->get_num_cols(_lm.root) + 1;
    out.assign(K, HeurOut());
    if (K == 0) return 0;
    return _route.run(
        api->round_many != nullptr, _lm,
        [&]() {
          std::vector<double> obj(K), x(K * row);
          std::vector<int> found(K);
          const int rc = api->round_many(_lm.root, hs.data(), (int)K, _mode, obj.data(), found.data(), x.data());
          for (size_t t = 0; t < K && rc == 0; t++) {
            out[t].obj = obj[t];
            out[t].found = found[t];
            out[t].x.assign(x.begin() + (long)(t * row), x.begin() + (long)((t + 1) * row));
          }
          return rc;
        },
        [&](const HostModel &M) {
          for (size_t t = 0; t < K; t++) {
            out[t].x.assign(row, 0.0);
            const int rc = round_host(api, M, hs[t], _mode, &out[t].obj, &out[t].found, out[t].x.data());
            if (rc != 0) return rc;
          }
          return 0;
        });
  }

private:
  LazyModel &_lm;
  int _mode;
  DeviceOrTwin _route;
};

// ---- incumbent polishing (polish, DESIGN.md "Incumbent polishing (polish)") ----

// The exchange search on one point against the model M (the host twin of k_lsact / k_lsmove / k_lsapply: the same test values in
// the same order).  The candidates of an iteration are walked singles first, then pairs by index(u), index(v), and one is taken
// only when its gain is strictly above the best so far: that is the tie rule.  A candidate that cannot win is not tested, which
// changes no result.  x[1..n] is edited in place when *ok comes back 1.
static int polish_host(const HostModel &M, double *x, int max_moves, double *obj, int *moves, int *ok) {
  if (!M.priced) return -2;
  const int n = M.n, m0 = M.m0;
  *obj = 0.0;
  *moves = 0;
  *ok = 0;
  std::vector<double> xt((size_t)n + 1, 0.0), r((size_t)m0, 0.0);
  for (int j = 1; j <= n; j++) {
    double v = x[j];
    if (M.isint[(size_t)j]) {
      const double ri = std::rint(v);
      if (!(std::fabs(v - ri) <= 1e-9)) return 0; // refused
      v = ri;
    }
    xt[(size_t)j] = v;
  }
  std::vector<double> lo_t((size_t)m0), hi_t((size_t)m0);
  for (int i = 0; i < m0; i++) {
    lo_t[(size_t)i] = M.rlo[(size_t)i] - round_tol(M.rlo[(size_t)i]);
    hi_t[(size_t)i] = M.rhi[(size_t)i] + round_tol(M.rhi[(size_t)i]);
  }
  auto inside = [&](int i, double t) { return t >= lo_t[(size_t)i] && t <= hi_t[(size_t)i]; };
  // the rounding heuristic's Activity and Feasible on xt
  auto feasible = [&](std::vector<double> &act) {
    for (int j = 1; j <= n; j++)
      if (!(M.clo[(size_t)j] <= xt[(size_t)j] && xt[(size_t)j] <= M.chi[(size_t)j])) return false;
    bool good = true;
    for (int i = 0; i < m0; i++) {
      double acc = 0.0;
      for (const auto &e : M.rows[(size_t)i])
        if (xt[(size_t)e.first] != 0.0) acc = acc + e.second * xt[(size_t)e.first];
      act[(size_t)i] = acc;
      good = good && inside(i, acc);
    }
    return good;
  };
  auto objective = [&]() {
    double sum = 0.0;
    for (int j = 1; j <= n; j++) sum = sum + M.c[(size_t)j] * xt[(size_t)j];
    return sum + M.c[0];
  };
  if (!feasible(r)) return 0; // refused
  const std::vector<double> x0 = xt;
  const double obj0 = objective();
  const int U = 2 * n;
  std::vector<char> adm((size_t)U, 0), ubad((size_t)m0, 0);
  std::vector<double> gain((size_t)U, 0.0), ru((size_t)m0, 0.0);
  auto col_of = [](int u) { return (u >> 1) + 1; };
  auto dir_of = [](int u) { return (u & 1) ? -1.0 : 1.0; };
  int taken = 0;
  while (taken < max_moves) {
    double gmax = 0.0; // the greatest gain of an admissible move: no pair gains more than g(u) + gmax
    for (int u = 0; u < U; u++) {
      const int j = col_of(u);
      const double d = dir_of(u), xn = xt[(size_t)j] + d;
      adm[(size_t)u] = M.isint[(size_t)j] && xn >= std::ceil(M.clo[(size_t)j]) && xn <= std::floor(M.chi[(size_t)j]);
      gain[(size_t)u] = M.sg * (d * M.c[(size_t)j]);
      if (adm[(size_t)u] && gain[(size_t)u] > gmax) gmax = gain[(size_t)u];
    }
    double best = 0.0;
    int bu = -1, bv = -1;
    for (int u = 0; u < U; u++) { // singles
      if (!adm[(size_t)u] || !(gain[(size_t)u] > best)) continue;
      const double d = dir_of(u);
      bool good = true;
      for (const auto &e : M.cols[(size_t)col_of(u)])
        if (!inside(e.first, r[(size_t)e.first] + d * e.second)) {
          good = false;
          break;
        }
      if (good) {
        best = gain[(size_t)u];
        bu = u;
      }
    }
    for (int u = 0; u < U; u++) { // pairs: the partner's column lies behind u's
      if (!adm[(size_t)u] || !(gain[(size_t)u] + gmax > best)) continue;
      const int ju = col_of(u);
      const double du = dir_of(u);
      ru = r;
      int nbad = 0;
      for (const auto &e : M.cols[(size_t)ju]) {
        const double t = r[(size_t)e.first] + du * e.second;
        ru[(size_t)e.first] = t;
        if (!inside(e.first, t)) {
          ubad[(size_t)e.first] = 1;
          nbad++;
        }
      }
      for (int v = 2 * ju; v < U; v++) {
        if (!adm[(size_t)v]) continue;
        const double g = gain[(size_t)u] + gain[(size_t)v];
        if (!(g > best)) continue;
        const double dv = dir_of(v);
        bool good = true;
        int mended = 0; // rows the single move u breaks that v touches: the others stay broken
        for (const auto &e : M.cols[(size_t)col_of(v)]) {
          if (!inside(e.first, ru[(size_t)e.first] + dv * e.second)) {
            good = false;
            break;
          }
          mended += ubad[(size_t)e.first];
        }
        if (good && mended == nbad) {
          best = g;
          bu = u;
          bv = v;
        }
      }
      if (nbad)
        for (const auto &e : M.cols[(size_t)ju]) ubad[(size_t)e.first] = 0;
    }
    if (bu < 0) break;
    for (const auto &e : M.cols[(size_t)col_of(bu)]) r[(size_t)e.first] = r[(size_t)e.first] + dir_of(bu) * e.second;
    xt[(size_t)col_of(bu)] = xt[(size_t)col_of(bu)] + dir_of(bu);
    if (bv >= 0) {
      for (const auto &e : M.cols[(size_t)col_of(bv)]) r[(size_t)e.first] = r[(size_t)e.first] + dir_of(bv) * e.second;
      xt[(size_t)col_of(bv)] = xt[(size_t)col_of(bv)] + dir_of(bv);
    }
    taken++;
  }
  *ok = 1;
  if (feasible(ru)) { // the freshly summed activities
    *obj = objective();
    *moves = taken;
  } else { // a tolerance edge: the entry point
    xt = x0;
    *obj = obj0;
  }
  for (int j = 1; j <= n; j++) x[j] = xt[(size_t)j];
  return 0;
}

// One tree's polishing: polish_many when the table has it, the twin on the tree's model without it or on -5.
class Polish {
public:
  Polish(LazyModel &lm, int cap) : _lm(lm), _cap(cap) {}
  // x[0..n] edited in place when *ok; 0, or the failing call's code
  int run(std::vector<double> &x, double *obj, int *moves, int *ok) {
    return _route.run(
        _lm.api->polish_many != nullptr, _lm, [&]() { return _lm.api->polish_many(_lm.root, 1, x.data(), _cap, obj, moves, ok); },
        [&](const HostModel &M) { return polish_host(M, x.data(), _cap, obj, moves, ok); });
  }

private:
  LazyModel &_lm;
  int _cap;
  DeviceOrTwin _route;
};

// ---- reduced-cost bound tightening (rc_fix, DESIGN.md "Reduced-cost tightening") ----

// The rule on one solved node from its exported tableau and basis (the host twin of k_rcfix: same tests, the same correctly
// rounded division): the changed columns in ascending order.
static int rc_tighten_host(const mvx_lp_api *api, const void *P, double B, double tol, RcList &out) {
  out.clear();
  if (!P) return -1;
  if (api->get_status(P) != MVX_OPT) return -3;
  if (!api->get_tableau || !api->get_basis || !api->get_col_kind || !api->get_col_lb || !api->get_col_ub) return -5;
  const int m = api->get_num_rows(P), n = api->get_num_cols(P);
  const double sg = (api->get_obj_dir && api->get_obj_dir(P) == MVX_MIN) ? -1.0 : 1.0;
  const double gap = sg * api->get_obj_val(P) - sg * B;
  const double gap2 = gap + 1e-9 * std::max(1.0, std::fabs(B));
  if (!(gap2 > 0.0)) return 0; // the node cannot beat the cutoff, or a NaN: no change
  std::vector<double> T((size_t)(m + 1) * (size_t)(n + 1));
  std::vector<int> head((size_t)m + 1), nb((size_t)n + 1), flag((size_t)n + 1);
  if (api->get_basis(P, head.data(), nb.data(), flag.data()) != 0 || api->get_tableau(P, T.data()) != 0) return -5;
  for (int q = 1; q <= n; q++) {
    const int j = nb[(size_t)q] - m;
    if (j < 1 || j > n || api->get_col_kind(P, j) == MVX_CV) continue;
    const int f = flag[(size_t)q];
    const double d = std::fabs(T[(size_t)q]);
    if ((f != MVX_NL && f != MVX_NU) || !(d > tol)) continue;
    const double lb = tab_bound(api->get_col_lb(P, j)), ub = tab_bound(api->get_col_ub(P, j));
    const double at = f == MVX_NL ? lb : ub;
    if (!(at == std::rint(at))) continue;
    const double room = std::ceil(gap2 / d) - 1.0;
    if (f == MVX_NL) {
      const double nu = at + room;
      if (nu < ub) out.push_back(RcEntry{j, lb, nu});
    } else {
      const double nl = at - room;
      if (nl > lb) out.push_back(RcEntry{j, nl, ub});
    }
  }
  std::sort(out.begin(), out.end(), [](const RcEntry &a, const RcEntry &b) { return a.col < b.col; });
  return 0;
}

// One tree's tightening: the lists of a batch of solved nodes through rc_tighten_many (one call) when the table has it, else
// the host twin per node; a batch of handles takes its lists through tighten_cols_many (one call), else set_col_bnds per
// entry.  A list depends on its node's LP and the cutoff only.
class RcFix {
public:
  explicit RcFix(const mvx_lp_api *api) : _api(api) {}
  long long calls = 0, fixed = 0, tightened = 0;
  // hs: solved (OPT) nodes, one cutoff for all of them; 0, or the failing call's code
  int compute(const std::vector<const void *> &hs, double cutoff, std::vector<RcList> &out) const {
    const size_t K = hs.size();
    out.assign(K, RcList());
    if (K == 0) return 0;
    if (_api->rc_tighten_many) {
      const size_t n = (size_t)_api->get_num_cols(hs[0]);
      std::vector<double> cut(K, cutoff), lb(K * n), ub(K * n);
      std::vector<int> cnt(K), cols(K * n);
      const int rc = _api->rc_tighten_many(hs.data(), (int)K, cut.data(), 1e-9, cnt.data(), cols.data(), lb.data(), ub.data());
      if (rc != 0) return rc;
      for (size_t t = 0; t < K; t++) out[t] = list_in(cnt[t], cols.data() + t * n, lb.data() + t * n, ub.data() + t * n);
      return 0;
    }
    for (size_t t = 0; t < K; t++) {
      const int rc = rc_tighten_host(_api, hs[t], cutoff, 1e-9, out[t]);
      if (rc != 0) return rc;
    }
    return 0;
  }
  // the node branches: its list is booked
  void book(const RcList &l) {
    calls++;
    for (const RcEntry &e : l) (e.lb == e.ub ? fixed : tightened)++;
  }
  // kids[k] takes *lists[k]
  int apply(const std::vector<void *> &kids, const std::vector<const RcList *> &lists) const {
    if (_api->tighten_cols_many) {
      const FlatLists f(lists);
      if (f.cols.empty()) return 0;
      return _api->tighten_cols_many(kids.data(), (int)kids.size(), f.off.data(), f.cols.data(), f.lb.data(), f.ub.data());
    }
    for (size_t k = 0; k < kids.size(); k++)
      for (const RcEntry &e : *lists[k]) _api->set_col_bnds(kids[k], e.col, e.lb == e.ub ? MVX_FX : MVX_DB, e.lb, e.ub);
    return 0;
  }
  void store(mvx_bnb_result *res) const {
    res->rc_calls = calls;
    res->rc_fixed = fixed;
    res->rc_tightened = tightened;
  }

private:
  const mvx_lp_api *_api;
};

// ---- node bound propagation (prop, DESIGN.md "Node bound propagation") ----

struct PropOut {
  int infeasible = 0, rounds = 0;
  RcList list; // the columns whose bounds changed, ascending; +-inf for an absent bound; empty when infeasible
};

// The propagation of one handle from its own column bounds (the host twin of k_prop: same tests, every product, sum and
// quotient rounded on its own, in the same order).
static int prop_host(const mvx_lp_api *api, const HostModel &M, const void *P, int max_rounds, PropOut &out) {
  const int n = M.n, m0 = M.m0;
  out = PropOut();
  if (!P || max_rounds < 1 || api->get_num_cols(P) != n) return -1;
  std::vector<double> l0((size_t)n + 1, 0.0), u0((size_t)n + 1, 0.0);
  for (int j = 1; j <= n; j++) {
    l0[(size_t)j] = tab_bound(api->get_col_lb(P, j));
    u0[(size_t)j] = tab_bound(api->get_col_ub(P, j));
  }
  std::vector<double> l = l0, u = u0, amin((size_t)m0), amax((size_t)m0);
  std::vector<int> kmins((size_t)m0), kmaxs((size_t)m0);
  for (int r = 0; r < max_rounds && !out.infeasible; r++) {
    out.rounds = r + 1;
    for (int i = 0; i < m0; i++) {
      double lmin = 0.0, lmax = 0.0;
      int kmin = 0, kmax = 0;
      for (const auto &e : M.rows[(size_t)i]) {
        const double v = e.second;
        const double bmin = v > 0.0 ? l[(size_t)e.first] : u[(size_t)e.first], bmax = v > 0.0 ? u[(size_t)e.first] : l[(size_t)e.first];
        if (std::isinf(bmin)) kmin++;
        else lmin = lmin + v * bmin;
        if (std::isinf(bmax)) kmax++;
        else lmax = lmax + v * bmax;
      }
      amin[(size_t)i] = lmin;
      amax[(size_t)i] = lmax;
      kmins[(size_t)i] = kmin;
      kmaxs[(size_t)i] = kmax;
      const double lo = M.rlo[(size_t)i], hi = M.rhi[(size_t)i];
      if ((kmin == 0 && std::isfinite(hi) && lmin > hi + round_tol(hi)) || (kmax == 0 && std::isfinite(lo) && lmax < lo - round_tol(lo)))
        out.infeasible = 1;
    }
    if (out.infeasible) break;
    bool changed = false;
    std::vector<double> nl = l, nu = u; // Jacobi: every candidate comes from the bounds the round started with
    for (int j = 1; j <= n; j++) {
      if (!M.isint[(size_t)j]) continue;
      const double lj = l[(size_t)j], uj = u[(size_t)j];
      double a = lj, b = uj;
      for (const auto &e : M.cols[(size_t)j]) {
        const int i = e.first;
        const double v = e.second;
        const int kmin = kmins[(size_t)i], kmax = kmaxs[(size_t)i];
        const double lo = M.rlo[(size_t)i], hi = M.rhi[(size_t)i];
        const double bmin = v > 0.0 ? lj : uj, bmax = v > 0.0 ? uj : lj;
        if (std::isfinite(hi) && (kmin == 0 || (kmin == 1 && std::isinf(bmin)))) {
          const double res = kmin == 0 ? amin[(size_t)i] - v * bmin : amin[(size_t)i];
          const double q = (hi - res) / v;
          if (std::isfinite(q)) {
            if (v > 0.0) {
              const double c = std::floor(q + round_tol(q));
              if (c < b) b = c;
            } else {
              const double c = std::ceil(q - round_tol(q));
              if (c > a) a = c;
            }
          }
        }
        if (std::isfinite(lo) && (kmax == 0 || (kmax == 1 && std::isinf(bmax)))) {
          const double res = kmax == 0 ? amax[(size_t)i] - v * bmax : amax[(size_t)i];
          const double q = (lo - res) / v;
          if (std::isfinite(q)) {
            if (v > 0.0) {
              const double c = std::ceil(q - round_tol(q));
              if (c > a) a = c;
            } else {
              const double c = std::floor(q + round_tol(q));
              if (c < b) b = c;
            }
          }
        }
      }
      if (a != lj || b != uj) {
        nl[(size_t)j] = a;
        nu[(size_t)j] = b;
        changed = true;
      }
      if (a > b) out.infeasible = 1;
    }
    l.swap(nl);
    u.swap(nu);
    if (!changed) break;
  }
  if (!out.infeasible)
    for (int j = 1; j <= n; j++)
      if (l[(size_t)j] != l0[(size_t)j] || u[(size_t)j] != u0[(size_t)j]) out.list.push_back(RcEntry{j, l[(size_t)j], u[(size_t)j]});
  return 0;
}

// hs[k] takes *lists[k] (+-inf for an absent bound): set_col_bnds_many (one call) when the table has it, else set_col_bnds per
// entry with the type the finite bounds give, FX where they meet.
static int apply_bound_lists(const mvx_lp_api *api, const std::vector<void *> &hs, const std::vector<const RcList *> &lists) {
  if (api->set_col_bnds_many) {
    const FlatLists f(lists);
    if (f.cols.empty()) return 0;
    return api->set_col_bnds_many(hs.data(), (int)hs.size(), f.off.data(), f.cols.data(), f.lb.data(), f.ub.data());
  }
  for (size_t k = 0; k < hs.size(); k++)
    for (const RcEntry &e : *lists[k]) {
      const bool has_l = std::isfinite(e.lb), has_u = std::isfinite(e.ub);
      api->set_col_bnds(hs[k], e.col, has_l && has_u ? (e.lb == e.ub ? MVX_FX : MVX_DB) : has_l ? MVX_LO : has_u ? MVX_UP : MVX_FR, e.lb, e.ub);
    }
  return 0;
}

// One tree's propagation: a batch of handles through propagate_many (one call) when the table has it and the model fits the
// kernel, else the host twin on the tree's model; the lists go on through set_col_bnds_many (one call), else
// set_col_bnds per entry.  A result depends on the handle's own bounds and the root's rows only.
class Prop {
public:
  Prop(LazyModel &lm, int max_rounds) : _api(lm.api), _lm(lm), _rounds(max_rounds) {}
  long long calls = 0, fixed = 0, tightened = 0, infeasible = 0;
  // 0, or the failing call's code (-2: neither propagate_many nor the twin's accessors)
  int compute(const std::vector<void *> &hs, std::vector<PropOut> &out) {
    const size_t K = hs.size();
    out.assign(K, PropOut());
    if (K == 0) return 0;
    return _route.run(
        _api->propagate_many != nullptr, _lm,
        [&]() {
          const size_t n = (size_t)_api->get_num_cols(_lm.root);
          std::vector<int> inf(K), rounds(K), cnt(K), cols(K * n + 1);
          std::vector<double> lb(K * n + 1), ub(K * n + 1);
          const int rc =
              _api->propagate_many(_lm.root, hs.data(), (int)K, _rounds, inf.data(), rounds.data(), cnt.data(), cols.data(), lb.data(), ub.data());
          for (size_t t = 0; t < K && rc == 0; t++) {
            out[t].infeasible = inf[t];
            out[t].rounds = rounds[t];
            out[t].list = list_in(cnt[t], cols.data() + t * n, lb.data() + t * n, ub.data() + t * n);
          }
          return rc;
        },
        [&](const HostModel &M) {
          for (size_t t = 0; t < K; t++) {
            const int rc = prop_host(_api, M, hs[t], _rounds, out[t]);
            if (rc != 0) return rc;
          }
          return 0;
        });
  }
  // the handles take their lists (a handle proved infeasible has none and keeps its bounds) and are booked
  int apply(const std::vector<void *> &hs, const std::vector<PropOut> &res) {
    for (const PropOut &o : res) {
      calls++;
      infeasible += o.infeasible;
      for (const RcEntry &e : o.list) (e.lb == e.ub ? fixed : tightened)++;
    }
    std::vector<const RcList *> lists;
    for (const PropOut &o : res) lists.push_back(&o.list);
    return apply_bound_lists(_api, hs, lists);
  }
  // compute + apply on a batch of children in front of their first solve
  int run(const std::vector<void *> &hs) {
    std::vector<PropOut> res;
    const int rc = compute(hs, res);
    if (rc != 0) return rc;
    return apply(hs, res);
  }
  void store(mvx_bnb_result *res) const {
    res->prop_calls = calls;
    res->prop_fixed = fixed;
    res->prop_tightened = tightened;
    res->prop_infeasible = infeasible;
  }

private:
  const mvx_lp_api *_api;
  LazyModel &_lm;
  int _rounds;
  DeviceOrTwin _route;
};

// ---- what the lockstep runners (dives, pumps) share ----

// the jobs of [j0, j1) that ended integral: one rounding call (mode 1) checks their LPs (job.cur) against the root's model and
// prices them with the root's objective; the results land in job.res
template <typename Job, typename Pred>
static int round_integral(Heuristic &round, std::vector<Job> &jobs, size_t j0, size_t j1, Pred integral) {
  std::vector<const void *> rh;
  std::vector<size_t> rj;
  for (size_t j = j0; j < j1; j++)
    if (integral(jobs[j])) {
      rh.push_back(jobs[j].cur);
      rj.push_back(j);
    }
  std::vector<HeurOut> got;
  const int rc = round.run(rh, got);
  if (rc != 0) return rc;
  for (size_t k = 0; k < rj.size(); k++) jobs[rj[k]].res = std::move(got[k]);
  return 0;
}

// ---- LP diving heuristic (dive, DESIGN.md "LP diving heuristic") ----

// What a rule picks on one solved node.
struct DivePick {
  int nfrac = 0, col = 0, dir = 0;
  double val = 0.0;
};

// The pick on one solved node (the host twin of k_divepick: same tests, every product rounded, the quotient correctly
// rounded): the smallest key in lexicographic order with the column last, so the lowest column wins a tie.
static int dive_pick_host(const mvx_lp_api *api, const HostModel &M, const void *P, int rule, DivePick &out) {
  if (!M.priced) return -2;
  const int n = M.n;
  out = DivePick();
  if (!P || (rule != 1 && rule != 2 && rule != 4) || api->get_num_cols(P) != n) return -1;
  if (api->get_status(P) != MVX_OPT) return -3;
  std::vector<double> v((size_t)n + 1, 0.0);
  if (api->get_col_prim_all) api->get_col_prim_all(P, v.data());
  else
    for (int j = 1; j <= n; j++) v[(size_t)j] = api->get_col_prim(P, j);
  double b1 = 0.0, b2 = 0.0;
  for (int j = 1; j <= n; j++) {
    if (!M.isint[(size_t)j]) continue;
    const double vj = v[(size_t)j];
    if (!(std::fabs(vj - std::rint(vj)) > 1e-9)) continue;
    const double fd = vj - std::floor(vj), fu = std::ceil(vj) - vj;
    const int near = fd <= fu ? 0 : 1;
    int dir = near;
    double k1 = 0.0, k2 = 0.0;
    if (rule == 1) {
      k1 = std::min(fd, fu);
    } else if (rule == 2) {
      const int dl = M.dl[(size_t)j], ul = M.ul[(size_t)j];
      dir = dl < ul ? 0 : ul < dl ? 1 : near;
      k1 = (double)std::min(dl, ul);
      k2 = dir ? fu : fd;
    } else {
      const double s = M.sg * M.c[(size_t)j];
      dir = s > 0.0 ? 0 : s < 0.0 ? 1 : near;
      k1 = (std::fabs(M.c[(size_t)j]) * (dir ? fu : fd)) / (double)(M.cols[(size_t)j].size() + 1);
    }
    if (out.nfrac == 0 || k1 < b1 || (k1 == b1 && k2 < b2)) { // columns ascend: a tie keeps the lower one
      b1 = k1;
      b2 = k2;
      out.col = j;
      out.dir = dir;
      out.val = vj;
    }
    out.nfrac++;
  }
  return 0;
}

// What the dives of one node gave: the best point of its rules (ties to the lower rule) and the work they took.
struct DiveOut {
  int found = 0;
  double obj = 0.0;
  std::vector<double> x; // [0..n] when found
  long long lps = 0, pivots = 0;
};

// One tree's dives.  run() takes solved (OPT) nodes and advances all their (node, rule) dives in lockstep: per round one
// pick call for the dives that stand on a fresh LP (dive_pick_many when the table has it and the model fits the kernel,
// else the twin), one clone each, one bound-list apply and one batched solve for all of them, and at the end one rounding
// call (mode 1) for the dives that ended integral.  No cutoff is used inside a dive: a result depends on its node's LP only.
class Dive {
public:
  Dive(LazyModel &lm, const mvx_bnb_params &prm) : Dive(lm, prm.dive, prm.dive_depth, prm.dive_freq) {}
  Dive(LazyModel &lm, int rules, int depth, int freq = 0)
      : _api(lm.api), _root(lm.root), _lm(lm), _rules(rules), _freq(freq), _depth(depth), _round(lm, 1) {}
  bool on() const { return _rules > 0; }
  // the root, and with dive_freq = F > 0 every node whose oid F divides
  bool selects(const MVOLP::NodeData &node) const { return _rules > 0 && (node.inital || (_freq > 0 && node.oid % _freq == 0)); }

  // the picks of (hs[k], rules[k]); 0, or the failing call's code
  int pick(const std::vector<const void *> &hs, const std::vector<int> &rules, std::vector<DivePick> &out) {
    const size_t K = hs.size();
    out.assign(K, DivePick());
    if (K == 0) return 0;
    return _route.run(
        _api->dive_pick_many != nullptr, _lm,
        [&]() {
          std::vector<int> nfrac(K), col(K), dir(K);
          std::vector<double> val(K);
          const int rc = _api->dive_pick_many(_root, hs.data(), (int)K, rules.data(), nfrac.data(), col.data(), dir.data(), val.data());
          for (size_t k = 0; k < K && rc == 0; k++) {
            out[k].nfrac = nfrac[k];
            out[k].col = col[k];
            out[k].dir = dir[k];
            out[k].val = val[k];
          }
          return rc;
        },
        [&](const HostModel &M) {
          for (size_t k = 0; k < K; k++) {
            const int rc = dive_pick_host(_api, M, hs[k], rules[k], out[k]);
            if (rc != 0) return rc;
          }
          return 0;
        });
  }

  // hs: solved (OPT) nodes; 0, or the failing call's code.  The dives are cut into batches that fit the strong-branching
  // memory budget (two tableaux per live dive); results do not depend on the cut.
  int run(const std::vector<const void *> &hs, std::vector<DiveOut> &out) {
    out.assign(hs.size(), DiveOut());
    if (hs.empty() || _rules <= 0) return 0;
    std::vector<Job> jobs;
    for (size_t t = 0; t < hs.size(); t++)
      for (int rule = 1; rule <= 4; rule <<= 1)
        if (_rules & rule) {
          Job jb;
          jb.node = t;
          jb.rule = rule;
          jb.cur = hs[t];
          jobs.push_back(jb);
        }
    const int rc = in_batches(_api, hs[0], jobs.size(), 2, [&](size_t j0, size_t j1) { return advance(jobs, j0, j1); });
    for (Job &jb : jobs) drop_cur(jb); // a failing call leaves clones behind
    if (rc != 0) return rc;
    // the node's result: its rules in ascending order, a strictly better point wins
    const double sg = (_api->get_obj_dir && _api->get_obj_dir(_root) == MVX_MIN) ? -1.0 : 1.0;
    for (Job &jb : jobs) {
      DiveOut &o = out[jb.node];
      o.lps += jb.lps;
      o.pivots += jb.pivots;
      if (jb.res.found && (!o.found || sg * jb.res.obj > sg * o.obj)) {
        o.found = 1;
        o.obj = jb.res.obj;
        o.x = std::move(jb.res.x);
      }
    }
    return 0;
  }

private:
  enum State { PICK, FLIP, INTEGRAL, ENDED }; // PICK: stands on a solved LP; FLIP: a side failed, the other one is next
  struct Job {
    size_t node = 0;
    int rule = 0;
    const void *cur = nullptr; // the node itself, or the dive's own clone
    bool owned = false;
    State state = PICK;
    int d = 0, col = 0, dir = 0;
    double val = 0.0;
    long long lps = 0, pivots = 0;
    HeurOut res;
  };
  void drop_cur(Job &jb) {
    if (jb.owned && jb.cur) _api->delete_prob(const_cast<void *>(jb.cur));
    jb.cur = nullptr;
    jb.owned = false;
  }
  // the bounds side `dir` of jb.col gives a clone of jb.cur; false when they cross
  bool side_bounds(const Job &jb, int dir, RcEntry &e) const {
    const double inf = std::numeric_limits<double>::infinity();
    const int t = _api->get_col_type(jb.cur, jb.col);
    const double l = (t == MVX_LO || t == MVX_DB || t == MVX_FX) ? _api->get_col_lb(jb.cur, jb.col) : -inf;
    const double u = t == MVX_FX ? l : (t == MVX_UP || t == MVX_DB) ? _api->get_col_ub(jb.cur, jb.col) : inf;
    e.col = jb.col;
    e.lb = dir ? std::ceil(jb.val) : l;
    e.ub = dir ? u : std::floor(jb.val);
    return e.lb <= e.ub;
  }

  int advance(std::vector<Job> &jobs, size_t j0, size_t j1) {
    const int n = _api->get_num_cols(_root);
    const int limit = _depth > 0 ? _depth : 4 * n + 64;
    for (;;) {
      // 1. the picks of the dives that stand on a fresh LP
      std::vector<const void *> ph;
      std::vector<int> pr;
      std::vector<size_t> pj;
      for (size_t j = j0; j < j1; j++)
        if (jobs[j].state == PICK) {
          ph.push_back(jobs[j].cur);
          pr.push_back(jobs[j].rule);
          pj.push_back(j);
        }
      std::vector<DivePick> picks;
      const int rc = pick(ph, pr, picks);
      if (rc != 0) return rc;
      for (size_t k = 0; k < pj.size(); k++) {
        Job &jb = jobs[pj[k]];
        if (picks[k].nfrac == 0) jb.state = INTEGRAL;
        else if (jb.d >= limit) jb.state = ENDED;
        else {
          jb.col = picks[k].col;
          jb.dir = picks[k].dir;
          jb.val = picks[k].val;
        }
      }
      // 2. one clone per live dive with its side's bounds; a side whose bounds cross fails without a solve
      std::vector<size_t> kj;
      std::vector<void *> kids;
      std::vector<RcList> lists;
      for (size_t j = j0; j < j1; j++) {
        Job &jb = jobs[j];
        if (jb.state != PICK && jb.state != FLIP) continue;
        RcEntry e{0, 0.0, 0.0};
        bool ok = side_bounds(jb, jb.dir, e);
        if (!ok && jb.state == PICK) {
          jb.state = FLIP;
          jb.dir = 1 - jb.dir;
          ok = side_bounds(jb, jb.dir, e);
        }
        if (!ok) {
          jb.state = ENDED; // infeasible
          continue;
        }
        void *kid = _api->create_prob();
        _api->copy_prob(kid, jb.cur, MVX_ON);
        kj.push_back(j);
        kids.push_back(kid);
        lists.push_back(RcList(1, e));
      }
      if (kids.empty()) break;
      std::vector<const RcList *> lp;
      for (const RcList &l : lists) lp.push_back(&l);
      int brc = apply_bound_lists(_api, kids, lp);
      // 3. one batched solve of the round's children, with the default parameters like a B&B child
      std::vector<int> pivots;
      if (brc == 0) pivots = solve_counted(_api, kids, nullptr);
      for (size_t k = 0; k < kids.size(); k++) {
        Job &jb = jobs[kj[k]];
        if (brc != 0) {
          _api->delete_prob(kids[k]);
          continue;
        }
        jb.lps++;
        jb.pivots += pivots[k];
        if (_api->get_status(kids[k]) == MVX_OPT) { // the child replaces cur
          drop_cur(jb);
          jb.cur = kids[k];
          jb.owned = true;
          jb.d++;
          jb.state = PICK;
        } else {
          _api->delete_prob(kids[k]);
          if (jb.state == PICK) { // the opposite side of the same column, once
            jb.state = FLIP;
            jb.dir = 1 - jb.dir;
          } else {
            jb.state = ENDED; // infeasible
          }
        }
      }
      if (brc != 0) return brc;
    }
    // 4. the dives that ended integral: rounded and checked against the root's model
    const int rc = round_integral(_round, jobs, j0, j1, [](const Job &jb) { return jb.state == INTEGRAL; });
    if (rc != 0) return rc;
    for (size_t j = j0; j < j1; j++) drop_cur(jobs[j]);
    return 0;
  }

  const mvx_lp_api *_api;
  const void *_root;
  LazyModel &_lm;
  int _rules, _freq, _depth;
  Heuristic _round;
  DeviceOrTwin _route;
};

// ---- feasibility pump (DESIGN.md "Feasibility pump") ----

// What the rounding and objective step gives on one solved node.
struct PumpStep {
  int nfrac = 0, moved = 0, stalled = 0, nnz = 0;
  std::vector<double> xt, c; // [0..n]
};

// The step on one solved node (the host twin of k_pumpobj: same tests, every operation rounded on its own): the rounding of the
// integer columns, the move of a repeated rounding, the distance slopes and the new objective in the node's own direction,
// c_j = a * (-sg * d_j) + (q * sqrt(nnz(d))) * c0_j.  The bounds are the node's own, the integer flags and c0 the root's.
static int pump_obj_host(const mvx_lp_api *api, const HostModel &M, const void *P, const double *xprev, int has_prev, double a, double q,
                         PumpStep &out) {
  if (!M.priced) return -2;
  const int n = M.n;
  if (!P || api->get_num_cols(P) != n || (has_prev && !xprev)) return -1;
  if (api->get_status(P) != MVX_OPT) return -3;
  std::vector<double> v((size_t)n + 1, 0.0), lo((size_t)n + 1, 0.0), hi((size_t)n + 1, 0.0);
  if (api->get_col_prim_all) api->get_col_prim_all(P, v.data());
  else
    for (int j = 1; j <= n; j++) v[(size_t)j] = api->get_col_prim(P, j);
  const double sg = (api->get_obj_dir && api->get_obj_dir(P) == MVX_MIN) ? -1.0 : 1.0;
  out = PumpStep();
  out.xt.assign((size_t)n + 1, 0.0);
  out.c.assign((size_t)n + 1, 0.0);
  std::vector<double> &xt = out.xt;
  bool differs = false;
  for (int j = 1; j <= n; j++) {
    if (!M.isint[(size_t)j]) continue;
    const double vj = v[(size_t)j];
    if (std::fabs(vj - std::rint(vj)) > 1e-9) out.nfrac++;
    const double L = std::ceil(tab_bound(api->get_col_lb(P, j))), U = std::floor(tab_bound(api->get_col_ub(P, j)));
    double x = std::floor(vj + 0.5); // round_host's nearest integer
    if (x < L) x = L;
    if (x > U) x = U;
    lo[(size_t)j] = L;
    hi[(size_t)j] = U;
    xt[(size_t)j] = x;
    if (has_prev && x != xprev[j]) differs = true;
  }
  const bool stall = has_prev && !differs;
  if (stall) {
    std::vector<double> sig((size_t)n + 1, -1.0);
    for (int j = 1; j <= n; j++) {
      if (!M.isint[(size_t)j]) continue;
      const double d = v[(size_t)j] - xt[(size_t)j], sd = std::fabs(d);
      if (!(sd > 0.0)) continue;
      const double xn = xt[(size_t)j] + (d > 0.0 ? 1.0 : -1.0);
      if (xn >= lo[(size_t)j] && xn <= hi[(size_t)j]) sig[(size_t)j] = sd;
    }
    for (int r = 0; r < 10; r++) {
      int win = 0;
      double bk = 0.0;
      for (int j = 1; j <= n; j++) // columns ascend: a tie keeps the lower one
        if (sig[(size_t)j] > bk) {
          bk = sig[(size_t)j];
          win = j;
        }
      if (!win) break;
      xt[(size_t)win] = xt[(size_t)win] + (v[(size_t)win] - xt[(size_t)win] > 0.0 ? 1.0 : -1.0);
      sig[(size_t)win] = -1.0;
      out.moved++;
    }
  }
  out.stalled = (stall && out.moved == 0) ? 1 : 0;
  std::vector<double> d((size_t)n + 1, 0.0);
  for (int j = 1; j <= n; j++) {
    if (!M.isint[(size_t)j]) continue;
    const double L = lo[(size_t)j], U = hi[(size_t)j], x = xt[(size_t)j];
    double dj;
    if (L == U) dj = 0.0;
    else if (x == L) dj = 1.0;
    else if (x == U) dj = -1.0;
    else {
      const double df = v[(size_t)j] - x;
      dj = df > 0.0 ? 1.0 : df < 0.0 ? -1.0 : 0.0;
    }
    d[(size_t)j] = dj;
    if (dj != 0.0) out.nnz++;
  }
  const double b = q * std::sqrt((double)out.nnz);
  for (int j = 1; j <= n; j++) {
    const double t1 = a * (-sg * d[(size_t)j]), t2 = b * M.c[(size_t)j];
    out.c[(size_t)j] = t1 + t2;
  }
  return 0;
}

// What the pump of one node gave: the point when it ended integral and the point checked out, the work, and how it ended.
struct PumpOut {
  int found = 0, end = 0; // end: MVX_PUMP_*
  double obj = 0.0;
  std::vector<double> x; // [0..n] when found
  long long lps = 0, pivots = 0;
};

// One tree's pumps.  run() takes solved (OPT) nodes and advances their pumps in lockstep: per round one rounding and
// objective step for the live pumps (pump_obj_many when the table has it and the model fits the kernel, else the twin), the
// history check on the host, one objective apply (set_obj_many, else set_obj_coef per changed column) and one batched solve,
// and at the end one rounding call (mode 1) for the pumps that ended integral.  Nothing of the incumbent enters: a result
// depends on its node's LP only.
class Pump {
public:
  Pump(LazyModel &lm, const mvx_bnb_params &prm) : Pump(lm, prm.pump, prm.pump_alpha, prm.pump_freq) {}
  Pump(LazyModel &lm, int iters, double alpha, int freq = 0)
      : _api(lm.api), _root(lm.root), _lm(lm), _iters(iters), _freq(freq), _alpha(alpha), _round(lm, 1) {}
  bool on() const { return _iters > 0; }
  // the root, and with pump_freq = F > 0 every node whose oid F divides
  bool selects(const MVOLP::NodeData &node) const { return _iters > 0 && (node.inital || (_freq > 0 && node.oid % _freq == 0)); }

  // the step on hs[k]; 0, or the failing call's code
  int step(const std::vector<const void *> &hs, const std::vector<const double *> &xprev, const std::vector<double> &ab,
           std::vector<PumpStep> &out) {
    const size_t K = hs.size();
    out.assign(K, PumpStep());
    if (K == 0) return 0;
    const int n = _api->get_num_cols(_root);
    const size_t row = (size_t)n + 1;
    return _route.run(
        _api->pump_obj_many != nullptr, _lm,
        [&]() {
          std::vector<double> xp(K * row, 0.0), xt(K * row), c(K * row);
          std::vector<int> hp(K), info(K * 4);
          for (size_t k = 0; k < K; k++) {
            hp[k] = xprev[k] ? 1 : 0;
            if (xprev[k]) std::memcpy(xp.data() + k * row, xprev[k], row * 8);
          }
          const int rc = _api->pump_obj_many(_root, hs.data(), (int)K, xp.data(), hp.data(), ab.data(), info.data(), xt.data(), c.data());
          for (size_t k = 0; k < K && rc == 0; k++) {
            out[k].nfrac = info[4 * k];
            out[k].moved = info[4 * k + 1];
            out[k].stalled = info[4 * k + 2];
            out[k].nnz = info[4 * k + 3];
            out[k].xt.assign(xt.begin() + k * row, xt.begin() + (k + 1) * row);
            out[k].c.assign(c.begin() + k * row, c.begin() + (k + 1) * row);
          }
          return rc;
        },
        [&](const HostModel &M) {
          for (size_t k = 0; k < K; k++) {
            const int rc = pump_obj_host(_api, M, hs[k], xprev[k], xprev[k] ? 1 : 0, ab[2 * k], ab[2 * k + 1], out[k]);
            if (rc != 0) return rc;
          }
          return 0;
        });
  }

  // hs: solved (OPT) nodes, left untouched; 0, or the failing call's code.  The pumps are cut into batches that fit the
  // strong-branching memory budget (one tableau per live pump); results do not depend on the cut.
  int run(const std::vector<const void *> &hs, std::vector<PumpOut> &out) {
    out.assign(hs.size(), PumpOut());
    if (hs.empty() || _iters <= 0) return 0;
    if (!_api->set_obj_many && !(_api->set_obj_coef && _api->get_obj_coef)) return -2;
    if (!_norm_ready) { // once per tree: the 2-norm of the root's objective, ascending j, plain adds
      if (!_api->get_obj_coef) return -2;
      const int n = _api->get_num_cols(_root);
      double sum = 0.0;
      for (int j = 1; j <= n; j++) {
        const double cj = _api->get_obj_coef(_root, j);
        sum = sum + cj * cj;
      }
      _norm = std::sqrt(sum);
      _norm_ready = true;
    }
    std::vector<Job> jobs(hs.size());
    const int rc = in_batches(_api, hs[0], jobs.size(), 1, [&](size_t j0, size_t j1) { return advance(hs, jobs, j0, j1); });
    for (Job &jb : jobs) drop(jb); // a failing call leaves clones behind
    if (rc != 0) return rc;
    for (size_t t = 0; t < jobs.size(); t++) {
      out[t].end = jobs[t].end;
      out[t].lps = jobs[t].lps;
      out[t].pivots = jobs[t].pivots;
      if (jobs[t].res.found) {
        out[t].found = 1;
        out[t].obj = jobs[t].res.obj;
        out[t].x = std::move(jobs[t].res.x);
      }
    }
    return 0;
  }

private:
  struct Job {
    void *cur = nullptr; // the pump's own clone of its node
    int k = 0, end = 0;  // LPs solved so far; 0 while the pump is live
    double alpha = 0.0;  // alpha_k
    std::vector<std::vector<double>> hist; // the roundings so far, the last one being xprev
    long long lps = 0, pivots = 0;
    HeurOut res;
  };
  void drop(Job &jb) {
    if (jb.cur) _api->delete_prob(jb.cur);
    jb.cur = nullptr;
  }
  // the objectives cs[k] applied to hs[k]
  int apply(const std::vector<void *> &hs, const std::vector<const std::vector<double> *> &cs) {
    const int n = _api->get_num_cols(_root);
    const size_t row = (size_t)n + 1;
    if (_api->set_obj_many) {
      std::vector<double> flat(hs.size() * row);
      for (size_t k = 0; k < hs.size(); k++) std::memcpy(flat.data() + k * row, cs[k]->data(), row * 8);
      return _api->set_obj_many(hs.data(), (int)hs.size(), flat.data()) == 0 ? 0 : -2;
    }
    for (size_t k = 0; k < hs.size(); k++)
      for (int j = 0; j <= n; j++)
        if (_api->get_obj_coef(hs[k], j) != (*cs[k])[(size_t)j]) _api->set_obj_coef(hs[k], j, (*cs[k])[(size_t)j]);
    return 0;
  }

  int advance(const std::vector<const void *> &nodes, std::vector<Job> &jobs, size_t j0, size_t j1) {
    for (size_t j = j0; j < j1; j++) {
      jobs[j].cur = _api->create_prob();
      _api->copy_prob(jobs[j].cur, nodes[j], MVX_ON);
      jobs[j].alpha = _alpha;
    }
    for (;;) {
      // 1. the step of the live pumps
      std::vector<const void *> sh;
      std::vector<const double *> sp;
      std::vector<double> ab;
      std::vector<size_t> sj;
      for (size_t j = j0; j < j1; j++) {
        Job &jb = jobs[j];
        if (jb.end) continue;
        sh.push_back(jb.cur);
        sp.push_back(jb.hist.empty() ? nullptr : jb.hist.back().data());
        ab.push_back(1.0 - jb.alpha);
        ab.push_back(_norm > 0.0 ? jb.alpha / _norm : 0.0);
        sj.push_back(j);
      }
      if (sh.empty()) break;
      std::vector<PumpStep> steps;
      int rc = step(sh, sp, ab, steps);
      if (rc != 0) return rc;
      // 2. how each goes on: integral, the limit, a stall, a cycle (the history is the host's), or the next LP
      std::vector<void *> gh;
      std::vector<const std::vector<double> *> gc;
      std::vector<size_t> gj;
      for (size_t k = 0; k < sj.size(); k++) {
        Job &jb = jobs[sj[k]];
        PumpStep &st = steps[k];
        if (st.nfrac == 0) jb.end = MVX_PUMP_INTEGRAL;
        else if (jb.k == _iters) jb.end = MVX_PUMP_LIMIT;
        else if (st.stalled) jb.end = MVX_PUMP_STALLED;
        else if (st.moved > 0 && std::find(jb.hist.begin(), jb.hist.end(), st.xt) != jb.hist.end()) jb.end = MVX_PUMP_CYCLE;
        if (jb.end) continue;
        jb.hist.push_back(st.xt);
        gh.push_back(jb.cur);
        gc.push_back(&st.c);
        gj.push_back(sj[k]);
      }
      if (gh.empty()) continue;
      // 3. one objective apply and one batched solve with the default parameters: the basis is primal feasible
      rc = apply(gh, gc);
      if (rc != 0) return rc;
      const std::vector<int> pivots = solve_counted(_api, gh, nullptr);
      for (size_t k = 0; k < gh.size(); k++) {
        Job &jb = jobs[gj[k]];
        jb.lps++;
        jb.pivots += pivots[k];
        jb.k++;
        jb.alpha = jb.alpha * 0.9;
        if (_api->get_status(gh[k]) != MVX_OPT) jb.end = MVX_PUMP_FAILED;
      }
    }
    // 4. the pumps that ended integral: rounded and checked against the root's model, priced with the root's objective
    const int rc = round_integral(_round, jobs, j0, j1, [](const Job &jb) { return jb.end == MVX_PUMP_INTEGRAL; });
    if (rc != 0) return rc;
    for (size_t j = j0; j < j1; j++) drop(jobs[j]);
    return 0;
  }

  const mvx_lp_api *_api;
  const void *_root;
  LazyModel &_lm;
  int _iters, _freq;
  double _alpha;
  Heuristic _round;
  DeviceOrTwin _route;
  bool _norm_ready = false;
  double _norm = 0.0;
};

// The counts of one point-finding rule (rounding, pump, dives), booked the way the serial loop meets the nodes.
struct RuleBook {
  long long calls = 0, found = 0, improved = 0, lps = 0, pivots = 0;
};

// ---- clique cuts in the tree (node_cliques, DESIGN.md "Clique cuts in the tree (node_cliques)") ----

// What the separation kept for one node: cnt member sets of W words each, in the twin's order.
struct CliqueOut {
  int cnt = 0;
  std::vector<unsigned long long> q;
};

// The rule's state for one tree: the conflict graph of `model`, taken once, the route to the separation (the table's
// clique_cuts_many while it accepts the model, the twin without it or once it has answered -5) and the counters.
class NodeCliques {
public:
  NodeCliques(const mvx_lp_api *api, const void *model, int K) : _api(api), _model(model), _K(K) {}
  bool on() const { return _K > 0 && _edges > 0; }
  // tree start: the graph through the table's conflict_graph, or through the twin without it or on -5.  0, or -2
  int start() {
    if (_K <= 0) return 0;
    _n = _api->get_num_cols(_model);
    _W = ((size_t)_n + 1 + 63) / 64;
    _adj.assign(((size_t)_n + 1) * _W, 0ULL);
    int rc = _api->conflict_graph ? _api->conflict_graph(_model, _adj.data(), &_edges) : -5;
    if (rc == -5) rc = mvx_bnb_conflict_graph(_api, _model, _adj.data(), &_edges);
    if (rc != 0) _edges = 0;
    return rc == 0 ? 0 : -2;
  }
  // the separation of the solved handles hs, one result each; 0, or the failing call's code
  int compute(const std::vector<const void *> &hs, std::vector<CliqueOut> &out) {
    const size_t count = hs.size(), per = (size_t)_K * _W;
    out.assign(count, CliqueOut());
    if (count == 0) return 0;
    std::vector<int> cnt(count, 0);
    std::vector<unsigned long long> q(count * per, 0ULL);
    std::vector<double> sum(count * (size_t)_K, 0.0);
    bool done = false;
    if (_api->clique_cuts_many && _device) {
      const int rc = _api->clique_cuts_many(_model, hs.data(), (int)count, _K, cnt.data(), q.data(), sum.data());
      if (rc == -5) _device = false;
      else if (rc != 0) return rc;
      else done = true;
    }
    if (!done)
      for (size_t t = 0; t < count; t++) {
        const int rc = mvx_bnb_clique_masks(_api, hs[t], _n, _adj.data(), _K, &cnt[t], &q[t * per], &sum[t * (size_t)_K]);
        if (rc != 0) return rc;
      }
    for (size_t t = 0; t < count; t++) {
      out[t].cnt = cnt[t];
      out[t].q.assign(q.begin() + (long)(t * per), q.begin() + (long)(t * per + (size_t)cnt[t] * _W));
    }
    return 0;
  }
  // a node that branches books its result
  void book(const CliqueOut &o) {
    _calls++;
    _rows += o.cnt;
  }
  // Child kids[t] takes the cliques *lists[t] (not empty) as rows -1 on Q >= -1, all children in one add_cut_rows_many call; on
  // -1, or without the entry, add_cut_rows handle by handle, and without that add_rows / set_mat_row / set_row_bnds row by row.
  // -2 is device memory: the rows are in every model, nothing is appended again.  With `ages` the rows enter the children's
  // age arrays at 0.
  void append(const std::vector<MVOLP::NodeData *> &kids, const std::vector<const CliqueOut *> &lists, bool ages) {
    if (kids.empty()) return;
    const size_t row = (size_t)_n + 1;
    std::vector<void *> hs;
    std::vector<int> off(1, 0);
    std::vector<double> vals, rhs;
    for (size_t t = 0; t < kids.size(); t++) {
      hs.push_back(kids[t]->prob);
      for (int c = 0; c < lists[t]->cnt; c++) {
        const size_t base = vals.size();
        vals.resize(base + row, 0.0);
        for (int j = 1; j <= _n; j++)
          if ((lists[t]->q[(size_t)c * _W + (size_t)j / 64] >> (j % 64)) & 1ULL) vals[base + (size_t)j] = -1.0;
        rhs.push_back(-1.0);
      }
      off.push_back((int)rhs.size());
    }
    const int rc = _api->add_cut_rows_many ? _api->add_cut_rows_many(hs.data(), (int)hs.size(), off.data(), vals.data(), rhs.data()) : -1;
    if (rc != 0 && rc != -2) {
      std::vector<int> inds(row);
      for (size_t j = 0; j < row; j++) inds[j] = (int)j;
      for (size_t t = 0; t < kids.size(); t++) {
        const int k = lists[t]->cnt;
        const double *v = vals.data() + (size_t)off[t] * row, *r = rhs.data() + off[t];
        const int arc = _api->add_cut_rows ? _api->add_cut_rows(hs[t], k, v, r) : -1;
        if (arc == 0 || arc == -2) continue;
        for (int c = 0; c < k; c++) {
          const int index = _api->add_rows(hs[t], 1);
          _api->set_mat_row(hs[t], index, _n, inds.data(), v + (size_t)c * row);
          _api->set_row_bnds(hs[t], index, MVX_LO, r[c], 0);
        }
      }
    }
    if (ages)
      for (size_t t = 0; t < kids.size(); t++) kids[t]->age.resize(kids[t]->age.size() + (size_t)lists[t]->cnt, 0);
  }
  void store(mvx_bnb_result *res) const {
    res->node_clique_conflicts = _edges;
    res->node_clique_calls = _calls;
    res->node_clique_rows = _rows;
  }

private:
  const mvx_lp_api *_api;
  const void *_model;
  const int _K;
  int _n = 0;
  size_t _W = 0;
  std::vector<unsigned long long> _adj;
  long long _edges = 0, _calls = 0, _rows = 0;
  bool _device = true;
};

// ---- what the three drivers share: the tree's state and what happens to a node once its LP is solved ----

// bs.cpp:229-233: the sum of the fractional parts of a solved node's violated columns
static double sum_infeas(const mvx_lp_api *api, const void *a, const std::vector<int> &vars) {
  double acc = 0;
  for (int i : vars)
    if (i != 0) acc += getFract(api->get_col_prim(a, i));
  return acc;
}

enum Verdict { STOP, INTEGER, INFEASIBLE, FATHOMED, BRANCH }; // STOP: the root ended the run (bs.cpp:139-149)

// One tree: the record, the incumbent and the counters.  The drivers differ in which nodes they solve together and when;
// what a solved node means for the tree is written here, once.
struct Tree {
  const mvx_lp_api *api;
  const mvx_bnb_params &prm;
  const bool quirks;
  const double sg; // sense_of
  const int n0;
  Recorder rec;
  int id = 1; // util.h:17
  double bestLower; // bs.cpp:90
  std::vector<double> xbest;
  int has_incumbent = 0, incumbent_oid = 0;
  int hit_limit = 0, count = 0, rc_out = 0;
  long long sb_lps = 0, sb_pivots = 0;
  RuleBook hbook, dbook, pbook;
  int incumbent_src = 0; // where the incumbent in hand came from: 0 a node's own LP, 1 the rounding heuristic, 2 a dive, 3 a pump
  LazyModel hm; // of `model`: the rows from before the root cut loop; the rules that read the model borrow it
  Polish pol;
  long long polish_calls = 0, polish_moves = 0, polish_improved = 0;
  bool failed = false; // a point could not be polished: the run ends with -2
  const int m0; // the rows of `model`: every row of a node behind them is a tree cut row (DESIGN.md "Cut purging in the tree")
  long long purge_calls = 0, purge_rows = 0, cut_rows_peak = 0;
  // MVX_BNB_WORK (a measurement aid, scripts/node_purge_profile.py): the sum over the solves that are booked of pivots x (live rows
  // of the handle + 1), the entries a dense pivot touches per column, printed to stderr when the tree ends
  const bool count_work = std::getenv("MVX_BNB_WORK") != nullptr;
  long long work = 0;
  void worked(const MVOLP::NodeData &nd, const void *h, long long pivots) {
    if (count_work && h) work += pivots * (long long)(api->get_num_rows(h) - nd.dead + 1);
  }

  Tree(const mvx_lp_api *api_, const void *prob, const mvx_bnb_params &p, const void *model = nullptr)
      : api(api_), prm(p), quirks(p.reference_quirks != 0), sg(MVOLP::sense_of(api_, prob, p)), n0(api_->get_num_cols(prob)),
        bestLower(-sg * std::numeric_limits<double>::infinity()), xbest((size_t)n0 + 1, 0.0), hm(api_, model ? model : prob), pol(hm, p.polish),
        m0(api_->get_num_rows(model ? model : prob)) {}

  std::shared_ptr<MVOLP::NodeData> root(const void *prob) { // bs.cpp:80
    auto S1 = std::make_shared<MVOLP::NodeData>(api, prob, id);
    S1->inital = true;
    if (prm.node_purge > 0) S1->age.assign((size_t)std::max(0, api->get_num_rows(prob) - m0), 0); // the root cut rounds' live rows
    rec.node(S1->oid, 0);
    return S1;
  }

  bool node_limit() {
    if (failed) return true;
    if (prm.max_nodes > 0 && count >= prm.max_nodes) hit_limit = 1;
    return hit_limit != 0;
  }

  // bs.cpp:210 fathoms a node whose bound does not beat the incumbent, ties included; a NaN bound is not fathomed
  bool beats(double obj) const { return !(sg * obj <= sg * bestLower); }

  // A node whose LP `h` holds solved, `status` from printInfo, `obj` its objective value: bound, label, event and incumbent
  // (bs.cpp:135-223).  On BRANCH nothing but the bound is booked yet.
  Verdict verdict(MVOLP::NodeData &node, const void *h, int status, double obj) {
    const size_t o = (size_t)node.oid;
    cut_rows_peak = std::max(cut_rows_peak, (long long)(api->get_num_rows(h) - m0 - node.dead));
    if (node.inital && status == -1) { // bs.cpp:139-143
      rec.prune[o] = MVOLP::FEAS;
      return STOP;
    }
    node.upperBound = obj; // bs.cpp:156
    rec.bound[o] = obj;
    if (status == 1) { // prune by integrality, bs.cpp:158-193
      rec.prune[o] = MVOLP::INTG;
      if (!node.inital) rec.emit(MVX_EV_INTEGER, node.oid, obj, 0.0, 0, 0);
      // the root: bs.cpp:144-149 leaves without the event and without recording the solution; repaired mode keeps it
      if (node.inital ? !quirks : sg * obj > sg * bestLower) {
        std::vector<double> x = xbest;
        const int na = api->get_num_cols(h);
        for (int i = 1; i <= na && i <= n0; i++) x[(size_t)i] = api->get_col_prim(h, i);
        adopt(0, obj, x, node.oid);
      }
      return node.inital ? STOP : INTEGER;
    }
    if (status == -1) { // bs.cpp:194-209
      rec.prune[o] = MVOLP::FEAS;
      rec.emit(MVX_EV_INFEASIBLE, node.oid, 0.0, 0.0, 0, 0);
      return INFEASIBLE;
    }
    if (!beats(obj)) { // bs.cpp:210-223
      rec.prune[o] = MVOLP::BNDS;
      rec.emit(MVX_EV_FATHOMED, node.oid, 0.0, 0.0, 0, 0);
      return FATHOMED;
    }
    return BRANCH;
  }

  // polish > 0: the point that has just become the incumbent is polished where the serial loop books it, whichever source it
  // came from; the source's decision and counters are those of the point as found.  A refused point (ok = 0) stays as booked.
  void polish_incumbent() {
    if (prm.polish <= 0 || failed) return;
    std::vector<double> x = xbest;
    double obj = 0.0;
    int moves = 0, ok = 0;
    if (pol.run(x, &obj, &moves, &ok) != 0) {
      rc_out = -2;
      failed = true;
      return;
    }
    polish_calls++;
    if (!ok) return;
    polish_moves += moves;
    if (sg * obj > sg * bestLower) polish_improved++;
    bestLower = obj;
    for (size_t j = 1; j < xbest.size(); j++) xbest[j] = x[j];
  }

  // The point x[1..] of objective `obj`, found at node `oid` by `source` (incumbent_src), becomes the incumbent and is polished.
  void adopt(int source, double obj, const std::vector<double> &x, int oid) {
    bestLower = obj;
    has_incumbent = 1;
    incumbent_oid = oid;
    incumbent_src = source;
    for (size_t j = 1; j < xbest.size() && j < x.size(); j++) xbest[j] = x[j];
    polish_incumbent();
  }
  // a rule's run on a node that branches: its work is booked, and its point is adopted when it is strictly better
  void book(RuleBook &b, int source, int found, double obj, const std::vector<double> &x, long long lps, long long pivots, int oid) {
    b.calls++;
    b.lps += lps;
    b.pivots += pivots;
    if (!found) return;
    b.found++;
    if (!(sg * obj > sg * bestLower)) return;
    b.improved++;
    adopt(source, obj, x, oid);
  }
  void book_heur(const HeurOut &h, int oid) { book(hbook, 1, h.found, h.obj, h.x, 0, 0, oid); }
  void book_dive(const DiveOut &d, int oid) { book(dbook, 2, d.found, d.obj, d.x, d.lps, d.pivots, oid); }
  void book_pump(const PumpOut &p, int oid) { book(pbook, 3, p.found, p.obj, p.x, p.lps, p.pivots, oid); }
  void book_choice(const Choice &c) {
    sb_lps += c.sb_lps;
    sb_pivots += c.sb_pivots;
  }
  void branched(const MVOLP::NodeData &node, double acc, int nviol, int pick) {
    rec.emit(MVX_EV_BRANCHED, node.oid, node.upperBound, acc, nviol, pick);
  }
  void children(const MVOLP::NodeData &node, const MVOLP::NodeData &S2, const MVOLP::NodeData &S3) { // bs.cpp:269-273
    rec.node(S2.oid, node.oid);
    rec.node(S3.oid, node.oid);
  }
  // the children's first solves have ended (bs.cpp:280,288,300-318)
  void candidates(MVOLP::NodeData &S2, double obj2, MVOLP::NodeData &S3, double obj3) {
    S2.upperBound = rec.bound[(size_t)S2.oid] = obj2;
    S3.upperBound = rec.bound[(size_t)S3.oid] = obj3;
    rec.emit(MVX_EV_CANDIDATE, S2.oid, obj2, 0.0, 0, 0);
    rec.emit(MVX_EV_CANDIDATE, S3.oid, obj3, 0.0, 0, 0);
  }
  // node_purge = A > 0, at a node that branches, in front of its cut step (host mirrors only): the ages of the node's tree cut
  // rows move on, and `out` takes the positions of the rows that leave both children.  false: the table cannot tell
  bool purge_ages(MVOLP::NodeData &node, const void *h, std::vector<int> &out) {
    out.clear();
    const int k = (int)node.age.size();
    if (prm.node_purge <= 0 || k == 0) return true;
    if (!api->get_row_stat || !api->set_row_bnds) return false;
    std::vector<int> basic((size_t)k, 0);
    for (int t = 0; t < k; t++)
      if (node.age[(size_t)t] != 255) basic[(size_t)t] = api->get_row_stat(h, m0 + 1 + t) == MVX_BS;
    out.resize((size_t)k);
    int nout = 0;
    mvx_bnb_purge_ages(k, basic.data(), prm.node_purge, node.age.data(), out.data(), &nout);
    out.resize((size_t)nout);
    return true;
  }
  // the rows the node's cut step has appended start at age 0; the children take the node's ages as they stand
  void purge_inherit(MVOLP::NodeData &node, const void *h, MVOLP::NodeData &S2, MVOLP::NodeData &S3) {
    if (prm.node_purge <= 0) return;
    node.age.resize((size_t)std::max(0, api->get_num_rows(h) - m0), 0);
    S2.age = node.age;
    S3.age = node.age;
    S2.dead = S3.dead = node.dead;
  }
  // Child kids[t] loses the rows at the positions *lists[t] of its age array (ascending, not empty), behind its branching bound
  // and in front of everything else that happens to it: all of them in one del_rows_many call; without the entry, or when it
  // fails, del_rows handle by handle; without that, or when it fails, each row becomes a free row (the same LP, not the same
  // bits), which stays where it is, dead.  Behind a deletion the child's ages are compacted as its rows are.
  void purge_children(const std::vector<MVOLP::NodeData *> &kids, const std::vector<const std::vector<int> *> &lists) {
    if (kids.empty()) return;
    std::vector<void *> hs;
    std::vector<int> off(1, 0), rows;
    for (size_t t = 0; t < kids.size(); t++) {
      hs.push_back(kids[t]->prob);
      for (int p : *lists[t]) rows.push_back(m0 + 1 + p);
      off.push_back((int)rows.size());
    }
    const bool all = api->del_rows_many && api->del_rows_many(hs.data(), (int)hs.size(), off.data(), rows.data()) == 0;
    for (size_t t = 0; t < kids.size(); t++) {
      MVOLP::NodeData &kid = *kids[t];
      const std::vector<int> &l = *lists[t];
      const int cnt = (int)l.size();
      bool deleted = all;
      if (!deleted && api->del_rows) {
        std::vector<int> num(1, 0);
        num.insert(num.end(), rows.begin() + off[t], rows.begin() + off[t + 1]);
        deleted = api->del_rows(kid.prob, cnt, num.data()) == 0;
      }
      if (deleted) {
        size_t w = 0, d = 0;
        for (size_t q = 0; q < kid.age.size(); q++) {
          if (d < l.size() && (size_t)l[d] == q) d++;
          else kid.age[w++] = kid.age[q];
        }
        kid.age.resize(w);
      } else {
        for (int p : l) {
          api->set_row_bnds(kid.prob, m0 + 1 + p, MVX_FR, 0.0, 0.0);
          kid.age[(size_t)p] = 255;
        }
        kid.dead += cnt;
      }
      purge_calls++;
      purge_rows += cnt;
    }
  }
  // a node is done (bs.cpp:326); true when a branching met the loop limit: bs.cpp:320-323 calls std::exit(-1), here the run stops
  bool counted(bool branching) {
    if (branching && count > prm.loop_limit) hit_limit = 1;
    count++;
    return hit_limit != 0;
  }

  static void store(const RuleBook &b, long long &calls, long long &found, long long &improved, long long *lps = nullptr,
                    long long *pivots = nullptr) {
    calls = b.calls;
    found = b.found;
    improved = b.improved;
    if (lps) *lps = b.lps;
    if (pivots) *pivots = b.pivots;
  }
  int finish(mvx_bnb_result *res, const RcFix *rcfix, const Prop *prop) const {
    std::memset(res, 0, sizeof(*res));
    res->n_nodes = id - 1;
    res->parent = dup(rec.parent);
    res->prune = dup(rec.prune);
    res->node_bound = dup(rec.bound);
    res->n_events = (int)rec.events.size();
    res->events = dup(rec.events);
    res->count = count;
    res->has_incumbent = has_incumbent;
    res->best_lower = bestLower;
    res->incumbent_oid = incumbent_oid;
    res->n = n0;
    res->x = dup(xbest);
    res->total_pivots = rec.pivots;
    res->hit_limit = hit_limit;
    res->sb_lps = sb_lps;
    res->sb_pivots = sb_pivots;
    store(hbook, res->heur_calls, res->heur_found, res->heur_improved);
    store(dbook, res->dive_calls, res->dive_found, res->dive_improved, &res->dive_lps, &res->dive_pivots);
    store(pbook, res->pump_calls, res->pump_found, res->pump_improved, &res->pump_lps, &res->pump_pivots);
    res->incumbent_heur = incumbent_src;
    res->polish_calls = polish_calls;
    res->polish_moves = polish_moves;
    res->polish_improved = polish_improved;
    if (rcfix) rcfix->store(res);
    if (prop) prop->store(res);
    res->node_purge_calls = purge_calls;
    res->node_purge_rows = purge_rows;
    res->node_cut_rows_peak = cut_rows_peak;
    if (count_work) std::fprintf(stderr, "bnb work: %lld\n", work);
    return rc_out;
  }
};

// The handles of the slots whose `mask` is set, from slot w0 on, go through `call(handles, slots, results)` together, and
// result k lands on its slot of `out`; the other slots keep what they hold.  Returns call's code.
template <typename R, typename F>
static int on_slots(const std::vector<void *> &hs, const std::vector<char> &mask, size_t w0, std::vector<R> &out, F call) {
  std::vector<const void *> sub;
  std::vector<size_t> slot;
  for (size_t w = w0; w < hs.size(); w++)
    if (mask[w]) {
      sub.push_back(hs[w]);
      slot.push_back(w);
    }
  std::vector<R> got;
  const int rc = call(sub, slot, got);
  if (rc != 0) return rc;
  for (size_t k = 0; k < slot.size(); k++) out[slot[k]] = std::move(got[k]);
  return 0;
}

// `model`: the handle whose rows 1..m0, bounds and objective the rules that read the model work on (rounding, propagation,
// dives, pump).  It is `prob` itself unless the root cut loop has appended rows to `prob`: a cut computed in floating point may
// be violated by a feasible point by more than those rules' margins, so they keep reading the model from before the cuts.
int branchAndBound(const mvx_lp_api *api, void *prob, const void *model, const mvx_bnb_params &prm, mvx_bnb_result *res) { // bs.cpp:54
  MVOLP::ParameterObj params(api, prob, prm);
  CutPool pool(api);
  Tree T(api, prob, prm, model);
  Recorder &rec = T.rec;
  std::deque<std::shared_ptr<MVOLP::NodeData>> leafContainer;
  leafContainer.push_back(T.root(prob));
  void *a = api->create_prob(); // bs.cpp:89
  Heuristic heur(T.hm, prm.heur);
  RcFix rcfix(api);
  Prop prop(T.hm, prm.prop);
  Dive dive(T.hm, prm);
  Pump pump(T.hm, prm);
  NodeCliques ncl(api, T.hm.root, prm.node_cliques);
  KktCheck kkt(api, T.hm.root, prm.kkt);
  FarkasCheck farkas(api, T.hm.root, prm.farkas);
  if (ncl.start() != 0) { // the graph could not be taken: the tree so far is the unsolved root
    T.rc_out = -2;
    leafContainer.clear();
  }

  while (!leafContainer.empty()) { // bs.cpp:96
    if (T.node_limit()) break;
    int index;
    std::shared_ptr<MVOLP::NodeData> node = params.pickNode(leafContainer, index); // bs.cpp:101
    api->erase_prob(a);                       // bs.cpp:114-115
    api->copy_prob(a, node->prob, MVX_OFF);   // bs.cpp:116
    {
      const long long piv0 = rec.pivots;
      solve(api, a, rec); // bs.cpp:117
      T.worked(*node, a, rec.pivots - piv0);
    }
    if (kkt.on()) { // kkt: the node's LP as solved, whatever its end status; nothing of the tree reads the result
      std::vector<double> kv;
      if (kkt.compute({a}, kv) != 0) {
        T.rc_out = -2;
        break;
      }
      kkt.book(kv.data(), node->oid);
    }
    if (farkas.on() && api->get_status(a) == MVX_NOFEAS) { // farkas: the proof of this verdict; nothing of the tree reads it
      std::vector<double> fv;
      std::vector<int> fi;
      if (farkas.compute({a}, fv, fi) != 0) {
        T.rc_out = -2;
        break;
      }
      farkas.book(fv.data(), fi.data(), node->oid);
    }
    const double obj = api->get_obj_val(a);
    rec.emit(MVX_EV_PREGNANT, node->oid, obj, 0.0, 0, 0); // bs.cpp:119-129

    auto ret = printInfo(api, a, T.quirks); // bs.cpp:135|151
    const std::vector<int> &vars = ret.second;
    const Verdict v = T.verdict(*node, a, ret.first, obj);
    if (v == STOP) break;
    leafContainer.erase(leafContainer.begin() + index); // bs.cpp:247
    if (v == BRANCH) {                                  // bs.cpp:224-324
      const double acc = sum_infeas(api, a, vars);
      // the rounding heuristic reads the node's LP as solved, in front of the cut step
      if (prm.heur > 0 && api->get_status(a) == MVX_OPT) {
        std::vector<HeurOut> ho;
        if (heur.run({a}, ho) != 0) {
          T.rc_out = -2;
          break;
        }
        T.book_heur(ho[0], node->oid);
      }
      // the pump starts from the node's LP as solved, behind the rounding heuristic and in front of the dives
      if (pump.selects(*node) && api->get_status(a) == MVX_OPT) {
        std::vector<PumpOut> pout;
        if (pump.run({a}, pout) != 0) {
          T.rc_out = -2;
          break;
        }
        T.book_pump(pout[0], node->oid);
      }
      // the dives start from the node's LP as solved, behind the rounding heuristic and in front of rc_fix and the cut step
      if (dive.selects(*node) && api->get_status(a) == MVX_OPT) {
        std::vector<DiveOut> dout;
        if (dive.run({a}, dout) != 0) {
          T.rc_out = -2;
          break;
        }
        T.book_dive(dout[0], node->oid);
      }
      // reduced-cost tightening against the incumbent in hand (a point the heuristic or a dive has just found counts), on the LP as
      // solved; the list goes to both children
      RcList rcl;
      if (prm.rc_fix > 0 && T.has_incumbent && api->get_status(a) == MVX_OPT) {
        std::vector<RcList> got;
        if (rcfix.compute({a}, T.bestLower, got) != 0) {
          T.rc_out = -2;
          break;
        }
        rcl = std::move(got[0]);
        rcfix.book(rcl);
      }
      // node_cliques: the violated cliques of the LP as solved, in front of the cut step; their rows go to both children
      CliqueOut ncq;
      if (ncl.on() && api->get_status(a) == MVX_OPT) {
        std::vector<CliqueOut> got;
        if (ncl.compute({a}, got) != 0) {
          T.rc_out = -2;
          break;
        }
        ncq = std::move(got[0]);
        ncl.book(ncq);
      }
      // var_strat 3 / 4 read the node's LP: they choose on it as solved, in front of the cut step
      int pick = 0;
      double bound = 0.0;
      if (prm.var_strat >= 3) {
        std::vector<Choice> ch;
        if (choose_many(api, {a}, {vars}, prm, ch) != 0) {
          T.rc_out = -2;
          break;
        }
        pick = ch[0].pick;
        bound = api->get_col_prim(a, pick);
        T.book_choice(ch[0]);
      }
      // node_purge: the ages move on in front of the cut step; the rows that have reached the limit leave both children
      std::vector<int> gone;
      if (!T.purge_ages(*node, a, gone)) {
        T.rc_out = -2;
        break;
      }
      add_node_cuts(api, a, prm, T.quirks, pool); // bs.cpp:249-258
      if (prm.var_strat < 3) {
        pick = params.pickVar(vars);         // bs.cpp:260
        bound = api->get_col_prim(a, pick); // bs.cpp:261
      }
      T.branched(*node, acc, (int)vars.size(), pick);

      auto S2 = std::make_shared<MVOLP::NodeData>(api, a, T.id); // bs.cpp:269-273
      auto S3 = std::make_shared<MVOLP::NodeData>(api, a, T.id);
      T.children(*node, *S2, *S3);
      child_bounds(api, a, pick, bound, T.quirks, S2->prob, S3->prob);
      T.purge_inherit(*node, a, *S2, *S3);
      if (!gone.empty()) T.purge_children({S2.get(), S3.get()}, {&gone, &gone});
      if (ncq.cnt > 0) ncl.append({S2.get(), S3.get()}, {&ncq, &ncq}, prm.node_purge > 0);
      // prop: both children behind their branching bound and the rc_fix list, in front of their first solve; whatever code
      // a failing call gives (no accessors, device memory, a refused list), the tree so far goes back with -2
      if ((!rcl.empty() && rcfix.apply({S2->prob, S3->prob}, {&rcl, &rcl}) != 0) || (prm.prop > 0 && prop.run({S2->prob, S3->prob}) != 0)) {
        T.rc_out = -2;
        break;
      }
      // bs.cpp:279 and :287 solve two independent clones; an engine with a batch entry runs them
      // side by side (identical results), otherwise one after the other as the reference does
      {
        const std::vector<int> pivs = solve_counted(api, {S2->prob, S3->prob}, nullptr);
        for (int piv : pivs) rec.pivots += piv;
        T.worked(*S2, S2->prob, pivs[0]);
        T.worked(*S3, S3->prob, pivs[1]);
      }
      leafContainer.push_back(S2); // bs.cpp:297-298
      leafContainer.push_back(S3);
      T.candidates(*S2, api->get_obj_val(S2->prob), *S3, api->get_obj_val(S3->prob));
    }
    if (T.counted(v == BRANCH)) break;
  }
  leafContainer.clear();
  api->delete_prob(a);
  const int rc = T.finish(res, &rcfix, &prop);
  ncl.store(res);
  kkt.store(res);
  farkas.store(res);
  return rc;
}

// Window mode: the front W nodes of the FIFO deque are solved together (one batched launch carries
// all of them), then bs.cpp's decisions are replayed in queue order.  With FIFO order children go to
// the back (bs.cpp:297-298) and no node is discarded unsolved, so the next W nodes the serial loop
// would pop are exactly the front W whatever their outcome: the tree, oids, events, pivot counts and
// incumbent are those of the node-at-a-time loop above.
int branchAndBoundWindow(const mvx_lp_api *api, void *prob, const void *model, const mvx_bnb_params &prm, mvx_bnb_result *res) {
  MVOLP::ParameterObj params(api, prob, prm);
  Tree T(api, prob, prm, model);
  Recorder &rec = T.rec;
  const bool quirks = T.quirks;
  std::deque<std::shared_ptr<MVOLP::NodeData>> leafContainer;
  leafContainer.push_back(T.root(prob));
  bool stop = false;
  Heuristic heur(T.hm, prm.heur);
  RcFix rcfix(api);
  Prop prop(T.hm, prm.prop);
  Dive dive(T.hm, prm);
  Pump pump(T.hm, prm);
  NodeCliques ncl(api, T.hm.root, prm.node_cliques);
  KktCheck kkt(api, T.hm.root, prm.kkt);
  FarkasCheck farkas(api, T.hm.root, prm.farkas);
  auto fail = [&]() { // whatever code a failing call gives, the tree so far goes back with -2
    T.rc_out = -2;
    stop = true;
  };
  if (ncl.start() != 0) fail(); // the graph could not be taken: the tree so far is the unsolved root

  struct Branch {
    size_t slot;
    std::shared_ptr<MVOLP::NodeData> S2, S3;
    int before2, before3;
    RcList rc; // rc_fix: the bound list both children take in front of their first solve
    std::vector<int> gone; // node_purge: the positions of the tree cut rows both children lose
    CliqueOut cliques;     // node_cliques: the rows both children take
  };
  // One round of the loop.  Its child solves (phase C) run on a worker thread while the main thread replays
  // the next window, whose nodes were solved rounds ago: a breadth-first queue is longer than the window
  // almost all the time.  Results do not depend on the overlap -- every LP is solved by the same calls on the
  // same state -- and the event stream is flushed round by round, in order.
  struct Round {
    std::vector<std::vector<mvx_bnb_event>> node_events;
    std::vector<Branch> branches;
    std::vector<void *> kids;
    std::vector<int> after1, repiv; // per kid: pivot count after its first solve; pivots of the re-solve done ahead (-1: none)
    std::vector<double> obj1;       // per kid: objective after its first solve (bs.cpp:280,288)
    std::future<void> fut;
    bool active = false;
  };
  // Rounds whose children are still being solved, oldest first.  Up to `depth` of them: while the slowest children of
  // one round finish (few batch slots busy), the next round's batch is already running on another batch context.
  std::deque<std::unique_ptr<Round>> flight;
  std::unordered_map<const void *, const Round *> inflight; // child handle -> the round that is solving it
  // Experiment knobs (off by default).  MVX_BNB_CHUNK=<c>: a replay's branchings leave as up to four rounds (chunks of at
  // least c branchings, in queue order), each one batched solve on its own worker; MVX_BNB_PREFIX=1: the next window
  // takes the queue's nodes only as far as their solves have ended, so one slow child holds back the nodes behind it in
  // its chunk and nothing else.  On the config-5 tree (a few tens of nodes wide, two thirds of a whole-round batch's
  // slot-launches idle behind its slowest LP: scripts/roundstats.py) this was measured SLOWER -- 2.86 s whole rounds,
  // 3.35 s with chunks of 8, 3.43 s with chunks of 2: more and smaller batches pay more fixed cost per batch, and the
  // dispatch of their tiny launches is what the GPU runs out of, not slots.  The wide tree does not care (104-117 ms).
  size_t depth = 2, chunk = (size_t)1 << 30;
  if (const char *e = std::getenv("MVX_BNB_DEPTH")) depth = (size_t)std::max(1, std::min(32, std::atoi(e)));
  if (const char *e = std::getenv("MVX_BNB_CHUNK")) chunk = (size_t)std::max(1, std::atoi(e));
  const bool prefix = std::getenv("MVX_BNB_PREFIX") && std::atoi(std::getenv("MVX_BNB_PREFIX")) != 0;
  CutPool pool(api); // persistent across nodes in bug-compatible mode (cut.h:15-23)
  const bool timing = std::getenv("MVX_BNB_TIMING") != nullptr;
  double tA = 0, tB = 0, tB_info = 0, tB_clone = 0, tB_cuts = 0, tB_rcuts = 0, tWait = 0;
  auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };

  // wait for a round's children, book their results, flush the round's events
  auto finalize = [&](Round &R) {
    if (!R.active) return;
    const double t0 = now();
    if (R.fut.valid()) R.fut.get();
    tWait += now() - t0;
    for (size_t b = 0; b < R.branches.size(); b++) {
      Branch &br = R.branches[b];
      const size_t k2 = 2 * b, k3 = 2 * b + 1;
      rec.pivots += (R.after1[k2] - br.before2) + (R.after1[k3] - br.before3);
      T.worked(*br.S2, br.S2->prob, R.after1[k2] - br.before2);
      T.worked(*br.S3, br.S3->prob, R.after1[k3] - br.before3);
      br.S2->repiv = R.repiv[k2];
      br.S3->repiv = R.repiv[k3];
      rec.sink = &R.node_events[br.slot];
      T.candidates(*br.S2, R.obj1[k2], *br.S3, R.obj1[k3]);
    }
    rec.sink = nullptr;
    for (auto &ne : R.node_events) rec.events.insert(rec.events.end(), ne.begin(), ne.end());
    for (void *k : R.kids) inflight.erase(k);
  };
  // rounds finish in the order they were started: the event stream is the serial one
  auto finalize_oldest = [&]() {
    if (flight.empty()) return;
    finalize(*flight.front());
    flight.pop_front();
  };
  auto finalize_through = [&](const Round *upto) {
    while (!flight.empty()) {
      const bool last = flight.front().get() == upto;
      finalize_oldest();
      if (last) break;
    }
  };

  while (!leafContainer.empty() && !stop) {
    if (T.node_limit()) break;
    double t0 = now();
    size_t W = std::min(leafContainer.size(), (size_t)prm.window);
    // The window may reach into the children that are still being solved: it ends in front of the first node whose
    // round has not finished (rounds are in queue order, so every older one has been booked by then), and waits
    // only when that node is the queue's head.  Same nodes in the same order as one by one -- only the grouping moves.
    for (size_t w = 0; w < W; w++) {
      auto it = inflight.find(leafContainer[w]->prob);
      if (it == inflight.end()) continue;
      const Round *R = it->second;
      if (prefix && w > 0 && R->fut.valid() && R->fut.wait_for(std::chrono::seconds(0)) != std::future_status::ready) {
        W = w;
        break;
      }
      finalize_through(R);
    }
    // A. solve the window (bs.cpp:114-117).  The reference copies the node's problem into the scratch
    // `a` and solves the copy; the node is discarded after this step either way, so its own clone is
    // solved in place here -- same state, one device-to-device clone fewer per node.  A node whose last
    // solve ended OPT, or whose re-solve was done ahead, goes through zero pivots and is not passed on.
    std::vector<void *> a(W), need;
    std::vector<int> before(W);
    for (size_t w = 0; w < W; w++) {
      a[w] = leafContainer[w]->prob;
      before[w] = api->get_it_cnt(a[w]);
      if (leafContainer[w]->repiv >= 0) continue;
      const int st = api->get_status(a[w]);
      if (st != MVX_OPT) need.push_back(a[w]);
    }
    if (!need.empty()) api->simplex_batch(need.data(), (int)need.size(), nullptr, nullptr); // none of them is in flight
    // kkt: the nodes this round has solved, in one call; booked by the replay for the nodes it reaches
    std::vector<double> kval;
    if (kkt.on() && kkt.compute(std::vector<const void *>(a.begin(), a.end()), kval) != 0) {
      fail();
      break;
    }
    // farkas: the nodes this round has left MVX_NOFEAS, in one call; booked by the replay for the nodes it reaches
    std::vector<double> fval;
    std::vector<int> fidx, fat(W, -1);
    if (farkas.on()) {
      std::vector<const void *> nofeas;
      for (size_t w = 0; w < W; w++)
        if (api->get_status(a[w]) == MVX_NOFEAS) {
          fat[w] = (int)nofeas.size();
          nofeas.push_back(a[w]);
        }
      if (farkas.compute(nofeas, fval, fidx) != 0) {
        fail();
        break;
      }
    }
    tA += now() - t0; t0 = now();
    // the lazy cut modes: the one cut of every node of the window that may branch, in one device pass (round_cuts);
    // printInfo of the window is taken ahead for that and reused by the replay
    std::vector<std::pair<int, std::vector<int>>> info;
    std::vector<std::unique_ptr<CutContainer>> pre;
    if (W >= 8) {
      // printInfo (util.cpp:414-473) of the whole window ahead of the replay, on a few threads: it reads every column
      // value of a node out of host mirrors that no cache holds yet (a window's nodes were solved rounds ago), ~15 us a
      // node when done one after the other inside the replay; the nodes are independent, the replay reuses the results
      info.resize(W);
      double ti = now();
      const size_t parts = std::min<size_t>(4, W / 4);
      std::vector<std::future<void>> fs;
      for (size_t part = 1; part < parts; part++)
        fs.push_back(std::async(std::launch::async, [&, part]() {
          for (size_t w = part * W / parts; w < (part + 1) * W / parts; w++) info[w] = printInfo(api, a[w], quirks);
        }));
      for (size_t w = 0; w < W / parts; w++) info[w] = printInfo(api, a[w], quirks);
      for (auto &f : fs) f.get();
      tB_info += now() - ti;
    }
    if (prm.cut_strat != 0 && prm.lazy_pool && api->gmi_cuts_many && !info.empty()) {
      std::vector<char> wanted(W, 0);
      for (size_t w = 0; w < W; w++) wanted[w] = info[w].first == 0; // neither infeasible nor integral: branches unless its bound prunes it
      const double ti = now();
      pre = round_cuts(api, a, wanted, prm, quirks);
      tB_cuts += now() - ti;
      tB_rcuts += now() - ti;
    }
    // var_strat 3 / 4, the heuristic and rc_fix work on the window ahead of the replay, each in one batched call over the slots
    // that qualify.  may[w]: node w is neither infeasible nor integral, so it branches unless its bound prunes it; opt[w]: and
    // its LP ended OPT.
    std::vector<char> may, opt;
    if (prm.var_strat >= 3 || prm.heur > 0 || prm.rc_fix > 0 || dive.on() || pump.on() || ncl.on()) {
      if (info.empty()) {
        info.resize(W);
        for (size_t w = 0; w < W; w++) info[w] = printInfo(api, a[w], quirks);
      }
      may.resize(W);
      opt.resize(W);
      for (size_t w = 0; w < W; w++) {
        may[w] = info[w].first == 0;
        opt[w] = may[w] && api->get_status(a[w]) == MVX_OPT;
      }
    }
    // var_strat 3 / 4: the choice of every node of the window that may branch, in one penalty call (and one strong-branching
    // batch).  It depends on the node's own LP only, so the replay takes the serial loop's picks; a node the replay then
    // prunes by bound has only cost work, and its strong-branching counts are not booked.
    std::vector<Choice> choice(may.size());
    if (prm.var_strat >= 3 && on_slots(a, may, 0, choice, [&](const auto &hs, const auto &slot, auto &got) {
          std::vector<std::vector<int>> vs;
          for (size_t w : slot) vs.push_back(info[w].second);
          return choose_many(api, hs, vs, prm, got);
        }) != 0) {
      fail();
      break;
    }
    // the rounding heuristic on every node of the window that may branch, in one call; booked by the replay for the nodes
    // that do branch, so the incumbent moves where the serial loop's does
    std::vector<HeurOut> hres(opt.size());
    if (prm.heur > 0 && on_slots(a, opt, 0, hres, [&](const auto &hs, const auto &, auto &got) { return heur.run(hs, got); }) != 0) {
      fail();
      break;
    }
    // the pumps of every selected node of the window that may branch, all in lockstep in one call; booked by the replay for
    // the nodes that do branch.  Nothing of the incumbent enters a pump, so a result is the serial loop's
    std::vector<char> psel(pump.on() ? W : 0);
    for (size_t w = 0; w < psel.size(); w++) psel[w] = opt[w] && pump.selects(*leafContainer[w]);
    std::vector<PumpOut> pres(psel.size());
    if (pump.on() && on_slots(a, psel, 0, pres, [&](const auto &hs, const auto &, auto &got) { return pump.run(hs, got); }) != 0) {
      fail();
      break;
    }
    // the dives of every selected node of the window that may branch, all in lockstep in one call; booked by the replay for
    // the nodes that do branch.  No cutoff enters a dive, so a result is the serial loop's
    std::vector<char> dsel(dive.on() ? W : 0);
    for (size_t w = 0; w < dsel.size(); w++) dsel[w] = opt[w] && dive.selects(*leafContainer[w]);
    std::vector<DiveOut> dres(dsel.size());
    if (dive.on() && on_slots(a, dsel, 0, dres, [&](const auto &hs, const auto &, auto &got) { return dive.run(hs, got); }) != 0) {
      fail();
      break;
    }
    // node_cliques: the separation of every node of the window that may branch, in one call; booked by the replay for the nodes
    // that do branch.  A result depends on the node's own LP and the model's graph only, so it is the serial loop's
    std::vector<CliqueOut> cres(ncl.on() ? W : 0);
    if (ncl.on() && on_slots(a, opt, 0, cres, [&](const auto &hs, const auto &, auto &got) { return ncl.compute(hs, got); }) != 0) {
      fail();
      break;
    }
    // rc_fix: the lists of every node of the window that may branch, in one call against the incumbent as it stands (none
    // yet: no call).  The replay uses a list only while the incumbent is the one it was computed with; once the replay has
    // moved the incumbent, the lists of the nodes from there on are computed again in one further call (rc_from).
    std::vector<RcList> rclist(opt.size());
    bool rc_have = false;
    double rc_cut = 0.0;
    auto rc_from = [&](size_t w0) {
      rc_have = true;
      rc_cut = T.bestLower;
      return on_slots(a, opt, w0, rclist, [&](const auto &hs, const auto &, auto &got) { return rcfix.compute(hs, T.bestLower, got); });
    };
    if (prm.rc_fix > 0 && T.has_incumbent && rc_from(0) != 0) {
      fail();
      break;
    }
    // B. replay in queue order
    Round cur;
    cur.node_events.resize(W);
    std::vector<Branch> &branches = cur.branches;
    size_t processed = 0;
    for (size_t w = 0; w < W; w++) {
      if (T.node_limit()) {
        stop = true;
        break;
      }
      std::shared_ptr<MVOLP::NodeData> node = leafContainer[w];
      void *aw = a[w];
      rec.sink = &cur.node_events[w];
      rec.pivots += (node->repiv >= 0) ? node->repiv : api->get_it_cnt(aw) - before[w];
      T.worked(*node, aw, (node->repiv >= 0) ? node->repiv : api->get_it_cnt(aw) - before[w]);
      processed++;
      if (kkt.on()) kkt.book(&kval[w * 8], node->oid);
      if (farkas.on() && fat[w] >= 0) farkas.book(&fval[(size_t)fat[w] * 4], &fidx[(size_t)fat[w] * 4], node->oid);
      const double obj = api->get_obj_val(aw);
      rec.emit(MVX_EV_PREGNANT, node->oid, obj, 0.0, 0, 0);
      double ti = now();
      auto ret = info.empty() ? printInfo(api, aw, quirks) : std::move(info[w]);
      tB_info += now() - ti;
      const std::vector<int> &vars = ret.second;
      const Verdict v = T.verdict(*node, aw, ret.first, obj);
      if (v == STOP) {
        stop = true;
        break;
      }
      if (v == BRANCH) {
        const double acc = sum_infeas(api, aw, vars);
        // cuts go onto the node's own problem (the serial driver's scratch copy `a`): both children inherit them.
        // The replay runs in queue order, so the persistent pool sees the nodes in bs.cpp's order.
        // bs.cpp:260-261 pick the variable and read its value behind the cut step; both are taken in front of it here: the
        // pick looks at the violated list and the root problem only, and appending a row leaves every other row's value
        // as it is -- but it marks the handle's solution mirrors stale, and reading one value afterwards is a device
        // export and a host round trip per branching node (~40 us, a tenth of the cut modes' run)
        if (prm.heur > 0 && opt[w]) T.book_heur(hres[w], node->oid);
        if (pump.on() && psel[w]) T.book_pump(pres[w], node->oid);
        if (dive.on() && dsel[w]) T.book_dive(dres[w], node->oid);
        RcList node_rc;
        if (prm.rc_fix > 0 && T.has_incumbent && opt[w]) {
          // no lists yet, or the incumbent has moved since they were computed
          if ((!rc_have || rc_cut != T.bestLower) && rc_from(w) != 0) {
            fail();
            break;
          }
          node_rc = std::move(rclist[w]);
          rcfix.book(node_rc);
        }
        CliqueOut node_cl;
        if (ncl.on() && opt[w]) {
          node_cl = std::move(cres[w]);
          ncl.book(node_cl);
        }
        const int pick = prm.var_strat >= 3 ? choice[w].pick : params.pickVar(vars);
        const double bound = api->get_col_prim(aw, pick);
        if (prm.var_strat >= 3) T.book_choice(choice[w]);
        std::vector<int> gone;
        if (!T.purge_ages(*node, aw, gone)) {
          fail();
          break;
        }
        ti = now();
        add_node_cuts(api, aw, prm, quirks, pool, pre.empty() ? nullptr : pre[w].get());
        tB_cuts += now() - ti;
        T.branched(*node, acc, (int)vars.size(), pick);
        Branch br;
        br.slot = w;
        // bs.cpp:269-273 clones the solved node twice.  The node itself is dropped at the end of this
        // round, so the second child takes over its problem object instead of cloning it (same state,
        // one device-to-device tableau copy fewer per branching).
        double tc = now();
        br.S2 = std::make_shared<MVOLP::NodeData>(api, aw, T.id); // even oid (R), then odd (L): bs.cpp:43-52
        tB_clone += now() - tc;
        br.S3 = std::make_shared<MVOLP::NodeData>(api, aw, T.id, true);
        node->prob = nullptr;
        T.children(*node, *br.S2, *br.S3);
        child_bounds(api, aw, pick, bound, quirks, br.S2->prob, br.S3->prob); // aw is S3's own handle by now
        br.before2 = api->get_it_cnt(br.S2->prob);
        br.before3 = api->get_it_cnt(br.S3->prob);
        br.rc = std::move(node_rc);
        T.purge_inherit(*node, aw, *br.S2, *br.S3);
        br.gone = std::move(gone);
        br.cliques = std::move(node_cl);
        branches.push_back(br);
        leafContainer.push_back(br.S2); // the queue order bs.cpp:297-298 gives them
        leafContainer.push_back(br.S3);
      }
      if (T.counted(v == BRANCH)) {
        stop = true;
        break;
      }
    }
    rec.sink = nullptr;
    // node_purge: every child of the round loses its parent's list of rows in one call, behind its branching bound and in front
    // of everything else
    if (prm.node_purge > 0) {
      std::vector<MVOLP::NodeData *> kids;
      std::vector<const std::vector<int> *> lists;
      for (const Branch &br : branches)
        if (!br.gone.empty()) {
          kids.push_back(br.S2.get());
          kids.push_back(br.S3.get());
          lists.push_back(&br.gone);
          lists.push_back(&br.gone);
        }
      T.purge_children(kids, lists);
    }
    // node_cliques: every child of the round takes its parent's cliques as rows in one call, behind the purge
    if (ncl.on()) {
      std::vector<MVOLP::NodeData *> kids;
      std::vector<const CliqueOut *> lists;
      for (const Branch &br : branches)
        if (br.cliques.cnt > 0) {
          kids.push_back(br.S2.get());
          kids.push_back(br.S3.get());
          lists.push_back(&br.cliques);
          lists.push_back(&br.cliques);
        }
      ncl.append(kids, lists, prm.node_purge > 0);
    }
    // rc_fix: every child of the round takes its parent's list in one call, behind its branching bound and in front of its
    // first solve
    if (prm.rc_fix > 0) {
      std::vector<void *> kids;
      std::vector<const RcList *> lists;
      for (const Branch &br : branches)
        if (!br.rc.empty()) {
          kids.push_back(br.S2->prob);
          kids.push_back(br.S3->prob);
          lists.push_back(&br.rc);
          lists.push_back(&br.rc);
        }
      if (!kids.empty() && rcfix.apply(kids, lists) != 0) fail();
    }
    // prop: every child of the round in one compute and one apply call, behind its branching bound and its rc_fix list, in
    // front of the round's batched solve.  A child's result depends on its own bounds only: the serial driver's
    if (prm.prop > 0 && !branches.empty() && T.rc_out == 0) {
      std::vector<void *> kids;
      for (const Branch &br : branches) {
        kids.push_back(br.S2->prob);
        kids.push_back(br.S3->prob);
      }
      if (prop.run(kids) != 0) fail();
    }
    tB += now() - t0;
    // C. every child of this round is an independent LP (bs.cpp:279,287): batched solves on worker threads; then, for
    // the children found infeasible (or unbounded), the re-solve bs.cpp:117 will ask for when they are
    // popped (it depends on nothing that happens in between), so that popping never has to solve.
    // The replay is cut into rounds of whole nodes: chunk k holds the events of its nodes and their branchings.
    {
      const size_t nb = branches.size();
      const size_t per = std::max(chunk, (nb + 3) / 4);
      const size_t nchunks = nb == 0 ? 1 : (nb + per - 1) / per;
      size_t ev_lo = 0;
      for (size_t ck = 0; ck < nchunks; ck++) {
        const size_t b_lo = ck * per, b_hi = std::min(nb, b_lo + per);
        const size_t ev_hi = (ck + 1 == nchunks) ? cur.node_events.size() : branches[b_hi - 1].slot + 1;
        auto part = std::make_unique<Round>();
        for (size_t e = ev_lo; e < ev_hi; e++) part->node_events.push_back(std::move(cur.node_events[e]));
        for (size_t bi = b_lo; bi < b_hi; bi++) {
          Branch br = branches[bi];
          br.slot -= ev_lo;
          part->kids.push_back(br.S2->prob);
          part->kids.push_back(br.S3->prob);
          part->branches.push_back(std::move(br));
        }
        ev_lo = ev_hi;
        part->active = true;
        while (flight.size() >= depth) finalize_oldest(); // at most `depth` rounds in flight; events stay in round order
        flight.push_back(std::move(part));
        Round *R = flight.back().get();
        if (R->kids.empty()) continue;
        for (void *k : R->kids) inflight.emplace(k, R);
        const size_t nk = R->kids.size();
        R->after1.assign(nk, 0);
        R->repiv.assign(nk, -1);
        R->obj1.assign(nk, 0.0);
        auto solve_range = [api, R](size_t lo, size_t hi) {
          if (hi <= lo) return;
          api->simplex_batch(R->kids.data() + lo, (int)(hi - lo), nullptr, nullptr);
          std::vector<void *> again;
          std::vector<size_t> idx;
          for (size_t k = lo; k < hi; k++) {
            R->after1[k] = api->get_it_cnt(R->kids[k]);
            R->obj1[k] = api->get_obj_val(R->kids[k]);
            const int st1 = api->get_status(R->kids[k]);
            if (st1 == MVX_NOFEAS || st1 == MVX_UNBND) { // a re-solve of these may pivot on (fresh devex weights)
              again.push_back(R->kids[k]);
              idx.push_back(k);
            }
          }
          if (!again.empty()) {
            api->simplex_batch(again.data(), (int)again.size(), nullptr, nullptr);
            for (size_t t = 0; t < idx.size(); t++) R->repiv[idx[t]] = api->get_it_cnt(again[t]) - R->after1[idx[t]];
          }
        };
        // a wide chunk goes through the engine's batch entry in two halves on two threads: the host side of one batch
        // (control-block uploads, polls, result mirrors) overlaps the kernels of the other
        const bool two = nk >= 32 && !std::getenv("MVX_BNB_ONE_WORKER");
        auto work = [solve_range, nk, two]() {
          if (!two) {
            solve_range(0, nk);
            return;
          }
          const size_t half = (nk / 2 + 1) & ~(size_t)1; // siblings stay together
          auto other = std::async(std::launch::async, solve_range, half, nk);
          solve_range(0, half);
          other.get();
        };
        if (prm.window > 1 && !std::getenv("MVX_BNB_SYNC")) R->fut = std::async(std::launch::async, work);
        else work();
      }
    }
    leafContainer.erase(leafContainer.begin(), leafContainer.begin() + (long)processed);
  }
  while (!flight.empty()) finalize_oldest();
  if (timing) {
    std::fprintf(stderr, "add_node_cuts: column scan %.1f ms, cut copy/generation %.1f ms, row append %.1f ms\n", g_t_cut_scan * 1e3, g_t_cut_copy * 1e3, g_t_cut_add * 1e3);
    g_t_cut_scan = g_t_cut_copy = g_t_cut_add = 0;
  }
  if (timing)
    std::fprintf(stderr, "bnb window timing: A %.1f ms  B %.1f ms (printInfo %.1f, clone %.1f, cuts %.1f of which the round's device pass %.1f)  waiting for child solves %.1f ms\n", tA * 1e3,
                 tB * 1e3, tB_info * 1e3, tB_clone * 1e3, tB_cuts * 1e3, tB_rcuts * 1e3, tWait * 1e3);
  leafContainer.clear();
  const int rc = T.finish(res, &rcfix, &prop);
  ncl.store(res);
  kkt.store(res);
  farkas.store(res);
  return rc;
}

// printInfo of a round's nodes: one mvx_lp_api.classify_many call when the engine has it (one device launch for all of
// them), else one printInfo per node.  xs[t] holds the values of node t's violated columns, in the order of its list --
// the bits get_col_prim returns, so the host sums (bs.cpp:229-233) and the branching bound (bs.cpp:261) are unchanged.
static void classify_round(const mvx_lp_api *api, const std::vector<void *> &hs, bool quirks, int n,
                           std::vector<std::pair<int, std::vector<int>>> &info, std::vector<std::vector<double>> &xs) {
  const size_t K = hs.size();
  info.assign(K, {});
  xs.assign(K, {});
  if (api->classify_many && K > 0) {
    const int cap = std::max(1, n);
    std::vector<int> st(K), nv(K), viol(K * (size_t)cap);
    std::vector<double> xv(K * (size_t)cap);
    const int rc = api->classify_many(hs.data(), (int)K, quirks ? 1 : 0, st.data(), nv.data(), viol.data(), xv.data(), cap);
    if (rc == 0) {
      for (size_t t = 0; t < K; t++) {
        const int *v = &viol[t * (size_t)cap];
        const double *x = &xv[t * (size_t)cap];
        info[t].first = st[t];
        info[t].second.assign(v, v + nv[t]);
        xs[t].assign(x, x + nv[t]);
      }
      return;
    }
    if (std::getenv("MVX_BNB_TIMING")) std::fprintf(stderr, "classify_round: classify_many returned %d for %zu nodes\n", rc, K);
  }
  for (size_t t = 0; t < K; t++) {
    info[t] = printInfo(api, hs[t], quirks);
    for (int i : info[t].second) xs[t].push_back(api->get_col_prim(hs[t], i));
  }
}

// Best-bound window (node_strat = 1, best_window > 1).  The serial loop pops the open node of largest sg * upperBound
// (pickNode's first maximum: ties go to the node inserted first), and its next pick depends on the bounds of the
// children it has just solved, so the pops cannot be batched the way FIFO's can.  Instead each round speculates: the top
// W open nodes S[0..W-1] are re-solved (bs.cpp:114-117), classified and -- those that would branch under the current
// incumbent -- cut and branched, and ALL their children solved in one batched call.  The replay then walks S in key
// order and commits S[j] with the serial logic as long as (a) S[j] is the argmax of the live open set, which now holds
// the children committed so far in this round, and (b) S[j]'s decision is the speculated one (an incumbent found
// earlier in the replay may prune it now, bs.cpp:210).  The first node that fails either test ends the round: it and
// the nodes behind it stay open, untouched (cut rows go onto a clone, never onto the node's handle), their children are
// deleted, and the persistent pool of the bug-compatible mode (bs.cpp:73, cut.cpp:16-21) is rolled back to the state
// the committed prefix left.  oids, parents, events, pivot counts and the incumbent are booked at commit, in the order
// the serial loop books them: the tree is the node-at-a-time one.
int branchAndBoundBest(const mvx_lp_api *api, void *prob, const void *model, const mvx_bnb_params &prm, mvx_bnb_result *res) {
  MVOLP::ParameterObj params(api, prob, prm);
  CutPool pool(api);
  Tree T(api, prob, prm, model);
  Recorder &rec = T.rec;
  const bool quirks = T.quirks;
  const double sg = T.sg;
  // the open set in pop order: (sg * upperBound descending, insertion ascending) is pickNode's first maximum over the
  // deque, whose order is insertion order (erase keeps it, children are pushed at the back).  A NaN bound sorts last.
  struct Open {
    double key;
    long long ins;
    std::shared_ptr<MVOLP::NodeData> node;
    bool operator<(const Open &o) const { return key != o.key ? key > o.key : ins < o.ins; }
  };
  std::set<Open> open;
  long long ins = 0;
  auto push = [&](const std::shared_ptr<MVOLP::NodeData> &nd) {
    const double k = sg * nd->upperBound;
    open.insert(Open{std::isnan(k) ? -std::numeric_limits<double>::infinity() : k, ins++, nd});
  };
  push(T.root(prob));
  long long rounds = 0, speculated = 0;
  bool stop = false;
  Heuristic heur(T.hm, prm.heur);
  const size_t W = (size_t)prm.best_window;
  const bool timing = std::getenv("MVX_BNB_TIMING") != nullptr;
  double tA = 0, tInfo = 0, tSpec = 0, tKids = 0, tReplay = 0;
  auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };

  struct Spec {
    std::shared_ptr<MVOLP::NodeData> node;
    bool branch = false;
    int pick = 0;
    double bound = 0.0;
    void *S2 = nullptr, *S3 = nullptr; // speculative children, no oid yet
    int before2 = 0, before3 = 0;
    bool marked = false; // pool state in front of this node's cut step
    CutPool::Mark mark;
  };
  std::vector<std::pair<int, std::vector<int>>> info;
  std::vector<std::vector<double>> xs;
  while (!open.empty() && !stop) {
    if (T.node_limit()) break;
    double t0 = now();
    std::vector<Spec> S;
    for (auto it = open.begin(); it != open.end() && S.size() < W; ++it) {
      S.emplace_back();
      S.back().node = it->node;
    }
    const size_t K = S.size();
    rounds++;
    speculated += (long long)K;
    std::vector<void *> hs(K);
    for (size_t j = 0; j < K; j++) hs[j] = S[j].node->prob;
    // A. the pop-time re-solve (bs.cpp:114-117) of every node of S that has not had it, in place: a node's handle is
    // only ever read after that (its cut rows and children are clones), so a node that stays open keeps its solve and
    // its pivot count (repiv) until it is committed.  A node whose last solve ended OPT goes through zero pivots.
    std::vector<void *> need;
    std::vector<int> before(K, 0);
    for (size_t j = 0; j < K; j++) {
      if (S[j].node->repiv >= 0) continue;
      before[j] = api->get_it_cnt(hs[j]);
      if (api->get_status(hs[j]) != MVX_OPT) need.push_back(hs[j]);
    }
    if (!need.empty()) api->simplex_batch(need.data(), (int)need.size(), nullptr, nullptr);
    for (size_t j = 0; j < K; j++)
      if (S[j].node->repiv < 0) S[j].node->repiv = api->get_it_cnt(hs[j]) - before[j];
    tA += now() - t0;
    t0 = now();
    classify_round(api, hs, quirks, T.n0, info, xs);
    tInfo += now() - t0;
    t0 = now();
    // B. speculate under the incumbent as it stands
    std::vector<char> wanted(K, 0);
    for (size_t j = 0; j < K; j++) wanted[j] = S[j].branch = info[j].first == 0 && T.beats(api->get_obj_val(hs[j]));
    // the rounding heuristic on every node speculated to branch, in one call; booked when the node commits, so that an
    // incumbent it finds enters the commit test of the nodes behind it
    std::vector<char> opt(prm.heur > 0 ? K : 0);
    for (size_t j = 0; j < opt.size(); j++) opt[j] = wanted[j] && api->get_status(hs[j]) == MVX_OPT;
    std::vector<HeurOut> hres(opt.size());
    if (prm.heur > 0 && on_slots(hs, opt, 0, hres, [&](const auto &sub, const auto &, auto &got) { return heur.run(sub, got); }) != 0) {
      T.rc_out = -2;
      break;
    }
    std::vector<std::unique_ptr<CutContainer>> pre = round_cuts(api, hs, wanted, prm, quirks);
    std::vector<void *> kids;
    for (size_t j = 0; j < K; j++) {
      Spec &sp = S[j];
      if (!sp.branch) continue;
      const std::vector<int> &vars = info[j].second;
      sp.pick = params.pickVar(vars); // bs.cpp:260-261, in front of the cut step (see the FIFO window)
      for (size_t k = 0; k < vars.size(); k++)
        if (vars[k] == sp.pick) {
          sp.bound = xs[j][k];
          break;
        }
      void *aw = hs[j];
      void *base = aw;
      if (prm.cut_strat != 0) { // bs.cpp:249-258 on a clone: the node itself stays as it is until it is committed
        base = api->create_prob();
        api->copy_prob(base, aw, MVX_ON);
        sp.mark = pool.mark();
        sp.marked = true;
        add_node_cuts(api, base, prm, quirks, pool, pre.empty() ? nullptr : pre[j].get());
      }
      sp.S2 = api->create_prob();
      api->copy_prob(sp.S2, base, MVX_ON);
      if (base != aw) {
        sp.S3 = base; // the cut clone becomes the second child: one clone fewer
      } else {
        sp.S3 = api->create_prob();
        api->copy_prob(sp.S3, aw, MVX_ON);
      }
      child_bounds(api, aw, sp.pick, sp.bound, quirks, sp.S2, sp.S3);
      sp.before2 = api->get_it_cnt(sp.S2);
      sp.before3 = api->get_it_cnt(sp.S3);
      kids.push_back(sp.S2);
      kids.push_back(sp.S3);
    }
    tSpec += now() - t0;
    t0 = now();
    if (!kids.empty()) api->simplex_batch(kids.data(), (int)kids.size(), nullptr, nullptr); // bs.cpp:279,287 for the round
    tKids += now() - t0;
    t0 = now();
    // C. replay in true best-bound order
    size_t j = 0;
    for (; j < K; j++) {
      if (T.node_limit()) {
        stop = true;
        break;
      }
      Spec &sp = S[j];
      if (open.begin()->node != sp.node) break; // a child committed in this round outranks it
      const int status = info[j].first;
      const std::vector<int> &vars = info[j].second;
      void *aw = hs[j];
      const double obj = api->get_obj_val(aw);
      if (status == 0 && T.beats(obj) != sp.branch) break; // pruned by an incumbent of this round
      std::shared_ptr<MVOLP::NodeData> node = sp.node;
      open.erase(open.begin());
      rec.pivots += node->repiv;
      rec.emit(MVX_EV_PREGNANT, node->oid, obj, 0.0, 0, 0);
      const Verdict v = T.verdict(*node, aw, status, obj); // BRANCH exactly when speculated so: the test above
      if (v == STOP) {
        stop = true;
        j++;
        break;
      }
      if (v == BRANCH) {
        double acc = 0;
        for (size_t k = 0; k < vars.size(); k++)
          if (vars[k] != 0) acc += getFract(xs[j][k]); // bs.cpp:229-233
        if (prm.heur > 0 && opt[j]) T.book_heur(hres[j], node->oid);
        T.branched(*node, acc, (int)vars.size(), sp.pick);
        auto S2 = std::make_shared<MVOLP::NodeData>(api, sp.S2, T.id, true); // even oid (R), then odd (L): bs.cpp:43-52
        auto S3 = std::make_shared<MVOLP::NodeData>(api, sp.S3, T.id, true);
        sp.S2 = sp.S3 = nullptr;
        T.children(*node, *S2, *S3);
        rec.pivots += (api->get_it_cnt(S2->prob) - sp.before2) + (api->get_it_cnt(S3->prob) - sp.before3);
        T.candidates(*S2, api->get_obj_val(S2->prob), *S3, api->get_obj_val(S3->prob));
        push(S2); // bs.cpp:297-298
        push(S3);
      }
      if (T.counted(v == BRANCH)) {
        stop = true;
        j++;
        break;
      }
    }
    // S[j..] stay open: drop their speculative children and undo their cut steps on the pool
    bool rolled = false;
    for (size_t r = j; r < K; r++) {
      Spec &sp = S[r];
      if (sp.marked && !rolled) {
        pool.rollback(sp.mark);
        rolled = true;
      }
      if (sp.S2) api->delete_prob(sp.S2);
      if (sp.S3) api->delete_prob(sp.S3);
      sp.S2 = sp.S3 = nullptr;
    }
    tReplay += now() - t0;
  }
  if (timing)
    std::fprintf(stderr, "bnb best window timing: %lld rounds, %lld speculated, %d committed: re-solve %.1f ms  classify %.1f ms  speculate %.1f ms  children %.1f ms  replay %.1f ms\n",
                 rounds, speculated, T.count, tA * 1e3, tInfo * 1e3, tSpec * 1e3, tKids * 1e3, tReplay * 1e3);
  open.clear();
  const int rc = T.finish(res, nullptr, nullptr);
  res->rounds = rounds;
  res->speculated = speculated;
  return rc;
}

// ---- the gfx950 engine's table ----
const mvx_lp_api g_hip_api = {
    []() -> void * { return mvx_create_prob(); },
    [](void *P) { mvx_erase_prob((mvx_prob *)P); },
    [](void *P) { mvx_delete_prob((mvx_prob *)P); },
    [](void *d, const void *s, int names) { mvx_copy_prob((mvx_prob *)d, (const mvx_prob *)s, names); },
    [](void *P, int nrs) { return mvx_add_rows((mvx_prob *)P, nrs); },
    [](void *P, int i, int len, const int *ind, const double *val) { mvx_set_mat_row((mvx_prob *)P, i, len, ind, val); },
    [](void *P, int i, int t, double lb, double ub) { mvx_set_row_bnds((mvx_prob *)P, i, t, lb, ub); },
    [](void *P, int j, int t, double lb, double ub) { mvx_set_col_bnds((mvx_prob *)P, j, t, lb, ub); },
    [](void *P, const void *parm) { return mvx_simplex((mvx_prob *)P, (const mvx_smcp *)parm); },
    [](const void *P) { return mvx_get_status((const mvx_prob *)P); },
    [](const void *P) { return mvx_get_obj_val((const mvx_prob *)P); },
    [](const void *P, int j) { return mvx_get_obj_coef((const mvx_prob *)P, j); },
    [](const void *P, int j) { return mvx_get_col_prim((const mvx_prob *)P, j); },
    [](const void *P) { return mvx_get_num_rows((const mvx_prob *)P); },
    [](const void *P) { return mvx_get_num_cols((const mvx_prob *)P); },
    [](const void *P, int j) { return mvx_get_col_kind((const mvx_prob *)P, j); },
    [](const void *P, int j) { return mvx_get_col_stat((const mvx_prob *)P, j); },
    [](const void *P, int i) { return mvx_get_row_stat((const mvx_prob *)P, i); },
    [](const void *P, int i) { return mvx_get_row_ub((const mvx_prob *)P, i); },
    [](const void *P, int i) { return mvx_get_row_lb((const mvx_prob *)P, i); },
    [](const void *P, int j) { return mvx_get_col_ub((const mvx_prob *)P, j); },
    [](const void *P, int j) { return mvx_get_col_lb((const mvx_prob *)P, j); },
    [](const void *P, int j) { return mvx_get_col_type((const mvx_prob *)P, j); },
    [](const void *P, int i, int *ind, double *val) { return mvx_get_mat_row((const mvx_prob *)P, i, ind, val); },
    [](const void *P, int k, int *ind, double *val) { return mvx_eval_tab_row((const mvx_prob *)P, k, ind, val); },
    [](const void *P) { return mvx_get_it_cnt((const mvx_prob *)P); },
    [](void **probs, int count, const void *parm, int *rcs) {
      return mvx_simplex_batch((mvx_prob **)probs, count, (const mvx_smcp *)parm, rcs);
    },
    [](const void *P) { return mvx_get_obj_dir((const mvx_prob *)P); },
    [](const void *P, int repaired, const int *cols, int count, double *vals, double *rhs, int *ok) {
      return mvx_gmi_cuts((const mvx_prob *)P, repaired, cols, count, vals, rhs, ok);
    },
    [](const void *const *Ps, int repaired, const int *cols, int count, double *vals, double *rhs, int *ok) {
      return mvx_gmi_cuts_many((const mvx_prob *const *)Ps, repaired, cols, count, vals, rhs, ok);
    },
    [](const void *P, double *x) { mvx_get_col_prim_all((const mvx_prob *)P, x); },
    // weak: a build of this driver against another engine (tests/tsan) need not define it -- the entry is then NULL
    mvx_classify_many ? +[](const void *const *Ps, int count, int quirks, int *status, int *nviol, int *viol, double *xviol, int cap) {
      return mvx_classify_many((const mvx_prob *const *)Ps, count, quirks, status, nviol, viol, xviol, cap);
    } : nullptr,
    mvx_get_tableau ? +[](const void *P, double *out) { return mvx_get_tableau((const mvx_prob *)P, out); } : nullptr,
    mvx_get_basis ? +[](const void *P, int *head, int *nb, int *flag) { return mvx_get_basis((const mvx_prob *)P, head, nb, flag); } : nullptr,
    mvx_branch_penalties_many ? +[](const void *const *Ps, int count, const int *cols, const int *col_off, double tol, double *pd, double *pu,
                                    int *ad, int *au) {
      return mvx_branch_penalties_many((const mvx_prob *const *)Ps, count, cols, col_off, tol, pd, pu, ad, au);
    } : nullptr,
    mvx_round_many ? +[](const void *root, const void *const *Ps, int count, int mode, double *obj, int *found, double *x) {
      return mvx_round_many((const mvx_prob *)root, (const mvx_prob *const *)Ps, count, mode, obj, found, x);
    } : nullptr,
    mvx_rc_tighten_many ? +[](const void *const *Ps, int count, const double *cutoff, double tol, int *cnt, int *cols, double *lb, double *ub) {
      return mvx_rc_tighten_many((const mvx_prob *const *)Ps, count, cutoff, tol, cnt, cols, lb, ub);
    } : nullptr,
    mvx_tighten_cols_many ? +[](void *const *Ps, int count, const int *off, const int *cols, const double *lb, const double *ub) {
      return mvx_tighten_cols_many((mvx_prob *const *)Ps, count, off, cols, lb, ub);
    } : nullptr,
    mvx_propagate_many ? +[](const void *root, const void *const *Ps, int count, int max_rounds, int *infeasible, int *rounds, int *cnt, int *cols,
                             double *lb, double *ub) {
      return mvx_propagate_many((const mvx_prob *)root, (const mvx_prob *const *)Ps, count, max_rounds, infeasible, rounds, cnt, cols, lb, ub);
    } : nullptr,
    mvx_set_col_bnds_many ? +[](void *const *Ps, int count, const int *off, const int *cols, const double *lb, const double *ub) {
      return mvx_set_col_bnds_many((mvx_prob *const *)Ps, count, off, cols, lb, ub);
    } : nullptr,
    mvx_dive_pick_many ? +[](const void *root, const void *const *Ps, int count, const int *rules, int *nfrac, int *col, int *dir, double *val) {
      return mvx_dive_pick_many((const mvx_prob *)root, (const mvx_prob *const *)Ps, count, rules, nfrac, col, dir, val);
    } : nullptr,
    [](void *P, int j, double coef) { mvx_set_obj_coef((mvx_prob *)P, j, coef); },
    mvx_set_obj_many ? +[](void *const *Ps, int count, const double *c) { return mvx_set_obj_many((mvx_prob *const *)Ps, count, c); } : nullptr,
    mvx_pump_obj_many ? +[](const void *root, const void *const *Ps, int count, const double *xprev, const int *has_prev, const double *ab,
                            int *info, double *xt, double *c) {
      return mvx_pump_obj_many((const mvx_prob *)root, (const mvx_prob *const *)Ps, count, xprev, has_prev, ab, info, xt, c);
    } : nullptr,
    mvx_cut_scores ? +[](const void *P, int k, const double *vals, double *dot, double *gram) {
      return mvx_cut_scores((const mvx_prob *)P, k, vals, dot, gram);
    } : nullptr,
    mvx_add_cut_rows ? +[](void *P, int k, const double *vals, const double *rhs) { return mvx_add_cut_rows((mvx_prob *)P, k, vals, rhs); }
                     : nullptr,
    mvx_conflict_graph ? +[](const void *model, unsigned long long *adj, long long *edges) {
      return mvx_conflict_graph((const mvx_prob *)model, adj, edges);
    } : nullptr,
    mvx_del_rows ? +[](void *P, int nrs, const int *num) { return mvx_del_rows((mvx_prob *)P, nrs, num); } : nullptr,
    mvx_polish_many ? +[](const void *root, int count, double *x, int max_moves, double *obj, int *moves, int *ok) {
      return mvx_polish_many((const mvx_prob *)root, count, x, max_moves, obj, moves, ok);
    } : nullptr,
    mvx_del_rows_many ? +[](void *const *Ps, int count, const int *off, const int *rows) {
      return mvx_del_rows_many((mvx_prob *const *)Ps, count, off, rows);
    } : nullptr,
    mvx_clique_cuts_many ? +[](const void *root, const void *const *Ps, int count, int max_cuts, int *cnt, unsigned long long *q, double *sum) {
      return mvx_clique_cuts_many((const mvx_prob *)root, (const mvx_prob *const *)Ps, count, max_cuts, cnt, q, sum);
    } : nullptr,
    mvx_add_cut_rows_many ? +[](void *const *Ps, int count, const int *off, const double *vals, const double *rhs) {
      return mvx_add_cut_rows_many((mvx_prob *const *)Ps, count, off, vals, rhs);
    } : nullptr,
    mvx_kkt_many ? +[](const void *root, const void *const *Ps, int count, double *val, int *ind) {
      return mvx_kkt_many((const mvx_prob *)root, (const mvx_prob *const *)Ps, count, val, ind);
    } : nullptr,
    mvx_farkas_many ? +[](const void *root, const void *const *Ps, int count, double *val, int *ind) {
      return mvx_farkas_many((const mvx_prob *)root, (const mvx_prob *const *)Ps, count, val, ind);
    } : nullptr,
};

} // namespace

extern "C" {

const mvx_lp_api *mvx_hip_lp_api(void) { return &g_hip_api; }

void mvx_bnb_default_params(mvx_bnb_params *p) {
  p->var_strat = 0;  // util.h:65
  p->node_strat = 0; // util.h:66
  p->cut_strat = 0;  // util.h:67
  p->cut_chance = 0.0;
  p->loop_limit = 200000; // bs.cpp:320
  p->max_nodes = 0;
  p->reference_quirks = 1;
  p->lazy_pool = 1;
  p->cut_select = 0;
  p->window = 64;
  p->best_window = 0;
  p->sb_cands = 2;
  p->sb_iters = 4;
  p->heur = 0;
  p->rc_fix = 0;
  p->prop = 0;
  p->dive = 0;
  p->dive_freq = 0;
  p->dive_depth = 0;
  p->pump = 0;
  p->pump_freq = 0;
  p->pump_alpha = 0.0;
  p->cut_rounds = 0;
  p->cut_round_max = 0;
  p->cut_maxpar = 0.0;
  p->cut_families = 0;
  p->cut_purge = 0;
  p->polish = 0;
  p->node_purge = 0;
  p->node_cliques = 0;
  p->kkt = 0;
  p->farkas = 0;
}

// Repaired mode's rule for an integer column whose bounds are not integers (legal input: LP and MPS files may carry them):
// the bounds are rounded inward, ceil(lb) and floor(ub), before the first solve, so every branching splits an integral range
// (no child with crossed bounds) and a repaired GMI cut measures an integer column from an integral bound.  Returns 0: every
// bound is integral already (nothing written), 1: some were rounded (written when `apply`), 2: a column's range holds no
// integer (the model is infeasible; the handle is left half edited).  Bounds that are integers come back as they went in.
static int integral_bounds(const mvx_lp_api *api, void *P, bool apply) {
  const int n = api->get_num_cols(P);
  int out = 0;
  for (int j = 1; j <= n; j++) {
    if (api->get_col_kind(P, j) == MVX_CV) continue;
    const int t = api->get_col_type(P, j);
    if (t == MVX_FR) continue;
    const double l = api->get_col_lb(P, j), u = api->get_col_ub(P, j);
    const bool has_l = t == MVX_LO || t == MVX_DB || t == MVX_FX, has_u = t == MVX_UP || t == MVX_DB;
    const double nl = has_l ? std::ceil(l) : l, nu = t == MVX_FX ? std::floor(l) : (has_u ? std::floor(u) : u);
    if ((!has_l || nl == l) && (t == MVX_FX ? nu == l : (!has_u || nu == u))) continue;
    if ((t == MVX_DB || t == MVX_FX) && nl > nu) return 2;
    out = 1;
    if (apply) api->set_col_bnds(P, j, (t == MVX_DB && nl == nu) ? MVX_FX : t, nl, nu);
  }
  return out;
}

int mvx_bnb_integral_bounds(const mvx_lp_api *api, void *prob) { return integral_bounds(api ? api : &g_hip_api, prob, true); }
int mvx_bnb_fractional_bounds(const mvx_lp_api *api, const void *prob) {
  return integral_bounds(api ? api : &g_hip_api, const_cast<void *>(prob), false);
}

static int run_driver(const mvx_lp_api *api, void *prob, const void *model, const mvx_bnb_params *params, mvx_bnb_result *res) {
  if (api->simplex_batch && params->node_strat == 0 && params->window > 1)
    return branchAndBoundWindow(api, prob, model, *params, res);
  if (api->simplex_batch && params->node_strat == 1 && params->best_window > 1) return branchAndBoundBest(api, prob, model, *params, res);
  return branchAndBound(api, prob, model, *params, res);
}

// ---- root cut rounds (DESIGN.md "Root cut rounds") ----

// dot[t] = sum_j v_tj x_j and gram[t][s] = sum_j v_tj v_sj, j ascending from +0.0, product and sum rounded separately (the
// efficacy loop of cuts_via_engine): the arithmetic k_cutgram repeats.  A product commutes, so the lower triangle is a copy.
static void cut_scores_host(const mvx_lp_api *api, const void *P, int k, const double *vals, double *dot, double *gram) {
  const int n = api->get_num_cols(P);
  const size_t row = (size_t)n + 1;
  std::vector<double> x(row, 0.0);
  for (int j = 1; j <= n; j++) x[(size_t)j] = api->get_col_prim(P, j);
  for (int t = 0; t < k; t++) {
    const double *vt = vals + (size_t)t * row;
    double d = 0.0;
    for (int j = 1; j <= n; j++) d += vt[j] * x[(size_t)j];
    dot[t] = d;
    for (int s = t; s < k; s++) {
      const double *vs = vals + (size_t)s * row;
      double g = 0.0;
      for (int j = 1; j <= n; j++) g += vt[j] * vs[j];
      gram[(size_t)t * (size_t)k + (size_t)s] = g;
      gram[(size_t)s * (size_t)k + (size_t)t] = g;
    }
  }
}

// Step 4 of a round, from numbers only: efficacy descending (ties to the lower index), a cut is taken when it is at most
// `maxpar` parallel to every cut taken before it, until K are taken or `budget` are.
static std::vector<int> cut_select(int k, const double *eff, const double *gram, int K, double maxpar, int budget) {
  std::vector<int> order((size_t)k), taken;
  for (int t = 0; t < k; t++) order[(size_t)t] = t;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return eff[a] > eff[b]; });
  for (int t : order) {
    if ((int)taken.size() >= K || (int)taken.size() >= budget) break;
    const double nt = std::sqrt(gram[(size_t)t * (size_t)k + (size_t)t]);
    bool ok = true;
    for (int s : taken) {
      const double ns = std::sqrt(gram[(size_t)s * (size_t)k + (size_t)s]);
      if (!(gram[(size_t)t * (size_t)k + (size_t)s] <= maxpar * (nt * ns))) {
        ok = false;
        break;
      }
    }
    if (ok) taken.push_back(t);
  }
  return taken;
}

// ---- clique cuts (cut_families bit 2, DESIGN.md "Clique cuts (cut_families)") ----

// The conflict graph of the binary columns of `P`, whose model is M (the host twin of k_conflict_rows / k_conflict: the
// activities are step 1 of prop_host at the handle's own bounds, every product and sum rounded on its own, and a pair's test
// adds the lower column's coefficient first).  adj: (n+1) x W words.
static int conflict_graph_host(const mvx_lp_api *api, const HostModel &M, const void *P, unsigned long long *adj, long long *edges) {
  const int n = M.n, m0 = M.m0;
  const size_t W = ((size_t)n + 1 + 63) / 64;
  std::vector<double> l((size_t)n + 1, 0.0), u((size_t)n + 1, 0.0);
  std::vector<char> inB((size_t)n + 1, 0);
  for (int j = 1; j <= n; j++) {
    l[(size_t)j] = tab_bound(api->get_col_lb(P, j));
    u[(size_t)j] = tab_bound(api->get_col_ub(P, j));
    inB[(size_t)j] = M.isint[(size_t)j] && l[(size_t)j] == 0.0 && u[(size_t)j] == 1.0;
  }
  std::fill(adj, adj + ((size_t)n + 1) * W, 0ULL);
  auto set = [&](int j, int k) {
    adj[(size_t)j * W + (size_t)k / 64] |= 1ULL << (k % 64);
    adj[(size_t)k * W + (size_t)j / 64] |= 1ULL << (j % 64);
  };
  std::vector<std::pair<int, double>> pos, neg;
  for (int i = 0; i < m0; i++) {
    double lmin = 0.0, lmax = 0.0;
    int kmin = 0, kmax = 0;
    for (const auto &e : M.rows[(size_t)i]) {
      const double v = e.second;
      const double bmin = v > 0.0 ? l[(size_t)e.first] : u[(size_t)e.first], bmax = v > 0.0 ? u[(size_t)e.first] : l[(size_t)e.first];
      if (std::isinf(bmin)) kmin++;
      else lmin = lmin + v * bmin;
      if (std::isinf(bmax)) kmax++;
      else lmax = lmax + v * bmax;
    }
    const double lo = M.rlo[(size_t)i], hi = M.rhi[(size_t)i];
    const bool upper = kmin == 0 && std::isfinite(hi), lower = kmax == 0 && std::isfinite(lo);
    if (!upper && !lower) continue;
    pos.clear();
    neg.clear();
    for (const auto &e : M.rows[(size_t)i])
      if (inB[(size_t)e.first]) (e.second > 0.0 ? pos : neg).push_back(e);
    if (upper) {
      const double thr = hi + round_tol(hi);
      for (size_t a = 0; a < pos.size(); a++) {
        const double first = lmin + pos[a].second;
        for (size_t b = a + 1; b < pos.size(); b++)
          if (first + pos[b].second > thr) set(pos[a].first, pos[b].first);
      }
    }
    if (lower) {
      const double thr = lo - round_tol(lo);
      for (size_t a = 0; a < neg.size(); a++) {
        const double first = lmax + neg[a].second;
        for (size_t b = a + 1; b < neg.size(); b++)
          if (first + neg[b].second < thr) set(neg[a].first, neg[b].first);
      }
    }
  }
  long long bits = 0;
  for (size_t w = 0; w < ((size_t)n + 1) * W; w++) bits += __builtin_popcountll(adj[w]);
  *edges = bits / 2;
  return 0;
}

// The separation, from numbers only: greedy maximal cliques around the LP point, one per seed, the violated ones kept once
// each, at most max_cuts.  A clique is its columns in ascending order.
static std::vector<std::vector<int>> clique_cuts(int n, const unsigned long long *adj, const double *x, int max_cuts) {
  const size_t W = ((size_t)n + 1 + 63) / 64;
  std::vector<int> order;
  for (int j = 1; j <= n; j++)
    for (size_t w = 0; w < W; w++)
      if (adj[(size_t)j * W + w]) {
        order.push_back(j);
        break;
      }
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return x[a] > x[b]; });
  std::vector<std::vector<int>> kept;
  std::vector<unsigned long long> mask(W);
  for (int seed : order) {
    if ((int)kept.size() >= max_cuts) break;
    if (!(x[seed] > 1e-6)) continue;
    std::copy(adj + (size_t)seed * W, adj + (size_t)(seed + 1) * W, mask.begin());
    std::vector<int> Q(1, seed);
    for (int c : order) {
      if (!((mask[(size_t)c / 64] >> (c % 64)) & 1ULL)) continue;
      Q.push_back(c);
      for (size_t w = 0; w < W; w++) mask[w] &= adj[(size_t)c * W + w];
    }
    std::sort(Q.begin(), Q.end());
    double s = 0.0;
    for (int j : Q) s = s + x[j];
    if (!(s - 1.0 > 1e-6)) continue;
    if (std::find(kept.begin(), kept.end(), Q) != kept.end()) continue;
    kept.push_back(std::move(Q));
  }
  return kept;
}

struct CutLoopOut {
  long long rounds = 0, candidates = 0, rows = 0, lps = 0, pivots = 0;
  long long conflicts = 0, clique_cands = 0, clique_rows = 0;
  long long purged = 0;
  double bound0 = 0.0, bound = 0.0;
  void store(mvx_bnb_result *res) const {
    res->cutloop_rounds = rounds;
    res->cutloop_candidates = candidates;
    res->cutloop_rows = rows;
    res->cutloop_lps = lps;
    res->cutloop_pivots = pivots;
    res->cutloop_bound0 = bound0;
    res->cutloop_bound = bound;
    res->cutloop_conflicts = conflicts;
    res->cutloop_clique_cands = clique_cands;
    res->cutloop_clique_rows = clique_rows;
    res->cutloop_purged = purged;
    res->cutloop_live_rows = rows - purged;
  }
};

// Coefficient-range safeguard of step 2: a cut whose largest |coefficient| is more than this many times its smallest non-zero
// one is not taken into a round.  Such a row carries cancellation noise (entries of 1e-15 where the exact cut has zeros) from
// a late-round tableau; in-tree cuts derived from tableaux that hold such rows kept a fixture tree from closing.  Over the
// general fixtures the ratios fall into two groups, up to 1.2e5 and from 3.4e14 on; 1e9 parts them, and is the relative size
// (1e-9) below which the driver's other rules treat a number as zero.
constexpr double CUT_MAX_RANGE = 1e9;

// The loop on `P`, edited in place: first solve, then up to R rounds of (candidates, scores, selection, append, re-solve).
// `families`: bit 1 the repaired GMI cuts, bit 2 clique cuts out of the conflict graph of `P` as it is handed in (0 means 1).
// `purge` = A (DESIGN.md "Cut purging (cut_purge)"): 0 no row leaves; otherwise a row this call appended is purged once its
// auxiliary variable has been basic after A consecutive re-solves -- through del_rows of the table, or, without it or when it
// fails, as a free row (the same LP), which stays where it is and is never looked at again.
// Returns 0; -2 when the table lacks an accessor or one of its calls failed.
static int cut_loop(const mvx_lp_api *api, void *P, int R, int K, double maxpar, int families, int purge, CutLoopOut &o) {
  if (!api->add_rows || !api->set_mat_row || !api->set_row_bnds || !api->simplex || !api->get_status || !api->get_obj_val ||
      !api->get_col_prim || !api->get_num_rows || !api->get_num_cols || !api->get_col_kind || !api->get_col_stat || !api->get_it_cnt ||
      !api->eval_tab_row || !api->get_mat_row)
    return -2;
  if (K == 0) K = 32;
  if (maxpar == 0.0) maxpar = 0.9;
  const int n = api->get_num_cols(P);
  const size_t row = (size_t)n + 1;
  const int budget = std::max(64, api->get_num_rows(P));
  if (families == 0) families = 1;
  // the conflict graph, once, from the rows the handle has before any cut: the table's entry, the twin without it or on -5
  std::vector<unsigned long long> adj;
  if (families & 2) {
    adj.assign(row * ((row + 63) / 64), 0ULL);
    LazyModel lm(api, P);
    if (DeviceOrTwin().run(
            api->conflict_graph != nullptr, lm, [&]() { return api->conflict_graph(P, adj.data(), &o.conflicts); },
            [&](const HostModel &M) { return conflict_graph_host(api, M, P, adj.data(), &o.conflicts); }) != 0)
      return -2;
  }
  auto solve_lp = [&]() {
    const int before = api->get_it_cnt(P);
    api->simplex(P, nullptr);
    o.pivots += api->get_it_cnt(P) - before;
    o.lps++;
  };
  solve_lp();
  o.bound0 = o.bound = api->get_obj_val(P);
  std::vector<int> inds(row);
  for (int j = 0; j <= n; j++) inds[(size_t)j] = j;
  if (purge > 0 && !api->get_row_stat) return -2;
  std::vector<int> live_row, live_age; // the live rows of the loop, ascending, and their ages
  for (int r = 1; r <= R && api->get_status(P) == MVX_OPT; r++) {
    // 1. candidates: the repaired cut of every column generateCutGMI would not reject out of hand
    std::vector<int> cols;
    for (int j = 1; j <= n; j++)
      if (gmi_candidate(api, P, j)) cols.push_back(j);
    if (cols.empty()) break; // the root LP is integral
    std::vector<double> x(row, 0.0);
    for (int j = 1; j <= n; j++) x[(size_t)j] = api->get_col_prim(P, j);
    // the GMI candidates first, the cliques of this LP point behind them: ties in efficacy go to the lower index
    const int kg = (families & 1) ? (int)cols.size() : 0;
    std::vector<std::vector<int>> cliques;
    if ((families & 2) && o.conflicts > 0) cliques = clique_cuts(n, adj.data(), x.data(), 4 * K);
    o.clique_cands += (long long)cliques.size();
    const int k = kg + (int)cliques.size();
    std::vector<double> vals((size_t)k * row, 0.0), rhs((size_t)k, 0.0);
    std::vector<int> ok((size_t)k, 0);
    for (size_t q = 0; q < cliques.size(); q++) {
      for (int j : cliques[q]) vals[((size_t)kg + q) * row + (size_t)j] = -1.0;
      rhs[(size_t)kg + q] = -1.0;
      ok[(size_t)kg + q] = 1;
    }
    if (kg > 0 && (!api->gmi_cuts || api->gmi_cuts(P, 1, cols.data(), kg, vals.data(), rhs.data(), ok.data()) != 0)) {
      for (int t = 0; t < kg; t++) {
        double e = 0.0;
        CutContainer c = generateCutGMI(api, P, cols[(size_t)t], &e);
        ok[(size_t)t] = c.oid != -1;
        if (!ok[(size_t)t]) continue;
        std::copy(c.vals.begin(), c.vals.end(), vals.begin() + (long)((size_t)t * row));
        rhs[(size_t)t] = c.lb;
      }
    }
    // 2. scores: efficacy at the LP point, as cuts_via_engine computes it
    std::vector<int> live;
    std::vector<double> eff((size_t)k, 0.0);
    for (int t = 0; t < k; t++) {
      if (!ok[(size_t)t]) continue;
      const double *v = &vals[(size_t)t * row];
      double dot = 0.0, nrm = 0.0, big = 0.0, small = std::numeric_limits<double>::infinity();
      for (int j = 1; j <= n; j++) {
        dot += v[j] * x[(size_t)j];
        nrm += v[j] * v[j];
        const double a = std::fabs(v[j]);
        if (a > big) big = a;
        if (a != 0.0 && a < small) small = a;
      }
      if (!(nrm > 0.0)) continue;
      o.candidates++;
      if (big > CUT_MAX_RANGE * small) continue;
      eff[(size_t)t] = (rhs[(size_t)t] - dot) / std::sqrt(nrm);
      if (eff[(size_t)t] > 1e-6) live.push_back(t);
    }
    std::stable_sort(live.begin(), live.end(), [&](int a, int b) { return eff[(size_t)a] > eff[(size_t)b]; });
    if (live.size() > (size_t)4 * (size_t)K) live.resize((size_t)4 * (size_t)K);
    const int C = (int)live.size();
    if (C == 0) break;
    // 3. the Gram matrix of the survivors
    std::vector<double> sv((size_t)C * row), se((size_t)C), sdot((size_t)C), gram((size_t)C * (size_t)C);
    for (int t = 0; t < C; t++) {
      std::copy(vals.begin() + (long)((size_t)live[(size_t)t] * row), vals.begin() + (long)((size_t)(live[(size_t)t] + 1) * row),
                sv.begin() + (long)((size_t)t * row));
      se[(size_t)t] = eff[(size_t)live[(size_t)t]];
    }
    if (!api->cut_scores || api->cut_scores(P, C, sv.data(), sdot.data(), gram.data()) != 0)
      cut_scores_host(api, P, C, sv.data(), sdot.data(), gram.data());
    // 4. selection
    const int left = budget - (int)live_row.size();
    std::vector<int> taken = cut_select(C, se.data(), gram.data(), K, maxpar, left);
    if (taken.empty()) break;
    // 5. append in taken order and re-solve (the dual simplex, warm)
    const int nt = (int)taken.size();
    std::vector<double> tv((size_t)nt * row), tr((size_t)nt);
    for (int t = 0; t < nt; t++) {
      std::copy(sv.begin() + (long)((size_t)taken[(size_t)t] * row), sv.begin() + (long)((size_t)(taken[(size_t)t] + 1) * row),
                tv.begin() + (long)((size_t)t * row));
      tr[(size_t)t] = rhs[(size_t)live[(size_t)taken[(size_t)t]]];
      if (live[(size_t)taken[(size_t)t]] >= kg) o.clique_rows++;
    }
    int arc = -1;
    if (api->add_cut_rows) arc = api->add_cut_rows(P, nt, tv.data(), tr.data());
    if (arc != 0 && arc != -2) // -2: device memory, the rows are in the model and the next solve starts from the slack basis
      for (int t = 0; t < nt; t++) {
        const int index = api->add_rows(P, 1);
        api->set_mat_row(P, index, n, inds.data(), &tv[(size_t)t * row]);
        api->set_row_bnds(P, index, MVX_LO, tr[(size_t)t], 0);
      }
    o.rows += nt;
    {
      const int m_now = api->get_num_rows(P);
      for (int t = 0; t < nt; t++) {
        live_row.push_back(m_now - nt + 1 + t);
        live_age.push_back(0);
      }
    }
    solve_lp();
    o.rounds++;
    if (api->get_status(P) == MVX_OPT) o.bound = api->get_obj_val(P);
    // 6. the purge: slack rows that have stayed slack for `purge` re-solves leave, in one call
    if (purge > 0 && api->get_status(P) == MVX_OPT) {
      std::vector<int> num(1, 0);
      for (size_t l = 0; l < live_row.size(); l++) {
        live_age[l] = api->get_row_stat(P, live_row[l]) == MVX_BS ? live_age[l] + 1 : 0;
        if (live_age[l] >= purge) num.push_back(live_row[l]);
      }
      const int cnt = (int)num.size() - 1;
      if (cnt > 0) {
        const bool deleted = api->del_rows && api->del_rows(P, cnt, num.data()) == 0;
        if (!deleted)
          for (int t = 1; t <= cnt; t++) api->set_row_bnds(P, num[(size_t)t], MVX_FR, 0.0, 0.0);
        // the purged rows are not live any more; behind a deletion the others move up
        size_t w = 0;
        int gone = 0;
        for (size_t l = 0; l < live_row.size(); l++) {
          if (live_age[l] >= purge) {
            gone++;
            continue;
          }
          live_row[w] = deleted ? live_row[l] - gone : live_row[l];
          live_age[w] = live_age[l];
          w++;
        }
        live_row.resize(w);
        live_age.resize(w);
        o.purged += cnt;
        // one more solve (no pivot behind a deletion): its pivots count, it is not one of the loop's LPs
        const int before = api->get_it_cnt(P);
        api->simplex(P, nullptr);
        o.pivots += api->get_it_cnt(P) - before;
        if (api->get_status(P) == MVX_OPT) o.bound = api->get_obj_val(P);
      }
    }
  }
  return 0;
}

int mvx_branchAndBound(const mvx_lp_api *api, void *prob, const mvx_bnb_params *params, mvx_bnb_result *res) {
  mvx_bnb_params dflt;
  if (!params) {
    mvx_bnb_default_params(&dflt);
    params = &dflt;
  }
  if (!api) api = &g_hip_api;
  // var_strat 3 / 4 are not (yet) in the speculative best-bound window: refused, not run with another rule
  // heur > 0 needs the repaired mode: bug-compatible mode reproduces bs.cpp, which has no heuristic
  if (params->var_strat < 0 || params->var_strat > 4 || (params->var_strat >= 3 && params->best_window > 0) || params->heur < 0 ||
      params->heur > 2 || (params->heur > 0 && params->reference_quirks != 0) || params->rc_fix < 0 || params->rc_fix > 1 ||
      // rc_fix: the bound argument needs the repaired mode's children and cuts; not (yet) in the best-bound window
      (params->rc_fix > 0 && (params->reference_quirks != 0 || params->best_window > 0)) ||
      // prop: children with both bounds kept, and not (yet) in the best-bound window either
      params->prop < 0 || params->prop > 16 || (params->prop > 0 && (params->reference_quirks != 0 || params->best_window > 0)) ||
      // dive: children with both bounds kept, and not (yet) in the best-bound window either
      params->dive < 0 || params->dive > 7 || params->dive_freq < 0 || params->dive_depth < 0 ||
      (params->dive > 0 && (params->reference_quirks != 0 || params->best_window > 0)) ||
      // pump: the same
      params->pump < 0 || params->pump > 1000 || params->pump_freq < 0 || !(params->pump_alpha >= 0.0 && params->pump_alpha <= 1.0) ||
      (params->pump > 0 && (params->reference_quirks != 0 || params->best_window > 0)) ||
      // root cut rounds: repaired cuts only; every single-GPU driver runs behind them
      params->cut_rounds < 0 || params->cut_rounds > 64 ||
      (params->cut_rounds > 0 && (params->reference_quirks != 0 || params->cut_round_max < 0 || params->cut_round_max > 4096 ||
                                  !(params->cut_maxpar == 0.0 || (params->cut_maxpar > 0.0 && params->cut_maxpar <= 1.0)) ||
                                  params->cut_families < 0 || params->cut_families > 3 || params->cut_purge < 0 ||
                                  params->cut_purge > 64)) ||
      // polish: the repaired mode's incumbent; every single-GPU driver
      params->polish < 0 || params->polish > 100000 || (params->polish > 0 && params->reference_quirks != 0) ||
      // node_purge: the repaired mode's own cut rows (the bug-compatible pool re-adds its cuts); not (yet) in the best-bound window
      params->node_purge < 0 || params->node_purge > 64 ||
      (params->node_purge > 0 && (params->reference_quirks != 0 || params->best_window > 0)) ||
      // node_cliques: rows on the repaired mode's children; not (yet) in the best-bound window
      params->node_cliques < 0 || params->node_cliques > 64 ||
      (params->node_cliques > 0 && (params->reference_quirks != 0 || params->best_window > 0)) ||
      // kkt: observation of every solved node, in both quirk modes; not (yet) in the best-bound window
      params->kkt < 0 || params->kkt > 1 || (params->kkt > 0 && params->best_window > 0) ||
      // farkas: observation of every node that ends MVX_NOFEAS, in both quirk modes; not (yet) in the best-bound window
      params->farkas < 0 || params->farkas > 1 || (params->farkas > 0 && params->best_window > 0)) {
    std::memset(res, 0, sizeof(*res));
    return -1;
  }
  if (params->reference_quirks == 0 && (params->prop > 0 || params->cut_rounds > 0 || integral_bounds(api, prob, false) != 0)) {
    // the caller's handle stays as it is: the tree runs on a copy with the rounded (and, with prop, propagated) bounds
    void *work = api->create_prob();
    api->copy_prob(work, prob, MVX_OFF);
    int rc = 0;
    // no integer in some column's range, or the propagation proves it: the root is infeasible, nothing to solve
    auto infeasible_root = [&](int prune) {
      Tree T(api, prob, *params);
      T.rec.node(T.id++, 0);
      T.rec.prune[1] = prune;
      T.finish(res, nullptr, nullptr);
    };
    // the tree behind the root cut loop (cut_rounds > 0): `work` takes the cuts, a copy from before them stays the model
    auto run_tree = [&]() {
      if (params->cut_rounds <= 0) return run_driver(api, work, work, params, res);
      void *model = api->create_prob();
      api->copy_prob(model, work, MVX_OFF);
      CutLoopOut lo;
      int r = cut_loop(api, work, params->cut_rounds, params->cut_round_max, params->cut_maxpar, params->cut_families, params->cut_purge,
                       lo);
      if (r != 0) {
        infeasible_root(MVOLP::NONE); // the loop could not run: the tree so far is the unsolved root
        r = -2;
      } else {
        r = run_driver(api, work, model, params, res);
      }
      lo.store(res);
      api->delete_prob(model);
      return r;
    };
    if (integral_bounds(api, work, true) == 2) {
      infeasible_root(MVOLP::FEAS);
    } else if (params->prop > 0) {
      // the root's own propagation, on the same copy: its list is applied before the first solve
      LazyModel root_model(api, work); // read before the root's bounds are final: the tree reads its own
      Prop root_prop(root_model, params->prop);
      std::vector<PropOut> got;
      if (root_prop.compute({work}, got) != 0) {
        infeasible_root(MVOLP::NONE); // nothing ran: the tree so far is the unsolved root
        rc = -2;
      } else if (got[0].infeasible) {
        root_prop.apply({work}, got);
        infeasible_root(MVOLP::FEAS);
        root_prop.store(res);
      } else {
        root_prop.apply({work}, got);
        rc = run_tree();
        res->prop_calls += root_prop.calls;
        res->prop_fixed += root_prop.fixed;
        res->prop_tightened += root_prop.tightened;
        res->prop_infeasible += root_prop.infeasible;
      }
    } else {
      rc = run_tree();
    }
    api->delete_prob(work);
    return rc;
  }
  return run_driver(api, prob, prob, params, res);
}

void mvx_bnb_free_result(mvx_bnb_result *res) {
  std::free(res->parent);
  std::free(res->prune);
  std::free(res->node_bound);
  std::free(res->events);
  std::free(res->x);
  std::memset(res, 0, sizeof(*res));
}

double mvx_getFract(double x) { return getFract(x); }

int mvx_generateCutGMI(const mvx_lp_api *api, const void *prob, int j, int *inds, double *vals, double *lb, double *efficacy) {
  double e = 0.0;
  CutContainer c = generateCutGMI(api ? api : &g_hip_api, prob, j, &e);
  if (c.oid == -1) return -1;
  std::memcpy(inds, c.inds.data(), c.inds.size() * sizeof(int));
  std::memcpy(vals, c.vals.data(), c.vals.size() * sizeof(double));
  *lb = c.lb;
  *efficacy = e;
  return 0;
}

int mvx_bnb_classify(const mvx_lp_api *api, const void *prob, const void *root, int quirks, int var_strat, double *out) {
  if (var_strat >= 3) return -1; // the node-LP rules need the penalties of the node's candidates (mvx_bnb_penalties)
  if (!api) api = &g_hip_api;
  auto ret = printInfo(api, prob, quirks != 0);
  mvx_bnb_params p;
  mvx_bnb_default_params(&p);
  p.var_strat = var_strat;
  MVOLP::ParameterObj params(api, root, p);
  out[0] = (double)ret.first;
  out[1] = api->get_obj_val(prob);
  out[2] = (double)ret.second.size();
  out[3] = sum_infeas(api, prob, ret.second);
  out[4] = ret.second.empty() ? 0.0 : (double)params.pickVar(ret.second);
  return 0;
}

int mvx_bnb_make_children(const mvx_lp_api *api, const void *a, int pick, int quirks, void *S2, void *S3) {
  if (!api) api = &g_hip_api;
  const double bound = api->get_col_prim(a, pick); // bs.cpp:261
  api->copy_prob(S2, a, MVX_ON);                   // NodeData(a), util.cpp:33-34
  api->copy_prob(S3, a, MVX_ON);
  child_bounds(api, a, pick, bound, quirks != 0, S2, S3);
  return 0;
}

int mvx_bnb_penalties(const mvx_lp_api *api, const void *prob, const int *cols, int count, double tol, double *pen_down, double *pen_up,
                      int *arg_down, int *arg_up) {
  return host_penalties(api ? api : &g_hip_api, prob, cols, count, tol, pen_down, pen_up, arg_down, arg_up);
}

int mvx_bnb_round(const mvx_lp_api *api, const void *prob, const void *root, int mode, double *obj, int *found, double *x) {
  if (!api) api = &g_hip_api;
  if (!prob || !root || mode < 1 || mode > 2 || !obj || !found || !x) return -1;
  HostModel M;
  const int rc = read_host_model(api, root, M);
  if (rc != 0) return rc;
  return round_host(api, M, prob, mode, obj, found, x);
}

int mvx_bnb_dive_pick(const mvx_lp_api *api, const void *prob, const void *root, int rule, int *nfrac, int *col, int *dir, double *val) {
  if (!api) api = &g_hip_api;
  if (!prob || !root || (rule != 1 && rule != 2 && rule != 4) || !nfrac || !col || !dir || !val) return -1;
  HostModel M;
  int rc = read_host_model(api, root, M);
  if (rc != 0) return rc;
  DivePick p;
  rc = dive_pick_host(api, M, prob, rule, p);
  if (rc != 0) return rc;
  *nfrac = p.nfrac;
  *col = p.col;
  *dir = p.dir;
  *val = p.val;
  return 0;
}

int mvx_bnb_dive(const mvx_lp_api *api, const void *prob, const void *root, int rules, int depth, double *obj, int *found, double *x,
                 long long *lps, long long *pivots) {
  if (!api) api = &g_hip_api;
  if (!prob || !root || rules < 1 || rules > 7 || depth < 0 || !obj || !found || !x || !lps || !pivots ||
      api->get_num_cols(prob) != api->get_num_cols(root))
    return -1;
  if (api->get_status(prob) != MVX_OPT) return -3;
  LazyModel lm(api, root);
  Dive dive(lm, rules, depth);
  std::vector<DiveOut> out;
  const int rc = dive.run({prob}, out);
  if (rc != 0) return rc;
  *obj = out[0].obj;
  *found = out[0].found;
  *lps = out[0].lps;
  *pivots = out[0].pivots;
  for (size_t j = 1; j < out[0].x.size(); j++) x[j] = out[0].x[j];
  return 0;
}

int mvx_bnb_pump_obj(const mvx_lp_api *api, const void *prob, const void *root, const double *xprev, int has_prev, const double *ab,
                     int *info, double *xt, double *c) {
  if (!api) api = &g_hip_api;
  if (!prob || !root || !ab || !info || !xt || !c || (has_prev && !xprev)) return -1;
  HostModel M;
  int rc = read_host_model(api, root, M);
  if (rc != 0) return rc;
  PumpStep st;
  rc = pump_obj_host(api, M, prob, xprev, has_prev ? 1 : 0, ab[0], ab[1], st);
  if (rc != 0) return rc;
  info[0] = st.nfrac; info[1] = st.moved; info[2] = st.stalled; info[3] = st.nnz;
  std::memcpy(xt, st.xt.data(), st.xt.size() * 8);
  std::memcpy(c, st.c.data(), st.c.size() * 8);
  return 0;
}

int mvx_bnb_pump(const mvx_lp_api *api, const void *prob, const void *root, int iters, double alpha, double *obj, int *found, double *x,
                 long long *lps, long long *pivots, int *end) {
  if (!api) api = &g_hip_api;
  if (!prob || !root || iters < 1 || iters > 1000 || !(alpha >= 0.0 && alpha <= 1.0) || !obj || !found || !x || !lps || !pivots || !end)
    return -1;
  if (api->get_num_cols(prob) != api->get_num_cols(root)) return -1;
  if (!api->get_status) return -2;
  if (api->get_status(prob) != MVX_OPT) return -3;
  LazyModel lm(api, root);
  Pump pump(lm, iters, alpha);
  std::vector<PumpOut> out;
  const int rc = pump.run(std::vector<const void *>(1, prob), out);
  if (rc != 0) return rc;
  *found = out[0].found;
  *obj = out[0].obj;
  *lps = out[0].lps;
  *pivots = out[0].pivots;
  *end = out[0].end;
  if (out[0].found) std::memcpy(x + 1, out[0].x.data() + 1, (size_t)api->get_num_cols(root) * 8);
  return 0;
}

int mvx_bnb_rc_tighten(const mvx_lp_api *api, const void *prob, double cutoff, double tol, int *cnt, int *cols, double *lb, double *ub) {
  if (!api) api = &g_hip_api;
  if (!prob || !cnt || !cols || !lb || !ub) return -1;
  RcList l;
  *cnt = 0;
  const int rc = rc_tighten_host(api, prob, cutoff, tol, l);
  if (rc != 0) return rc;
  list_out(l, cnt, cols, lb, ub);
  return 0;
}

int mvx_bnb_propagate(const mvx_lp_api *api, const void *prob, const void *root, int max_rounds, int *infeasible, int *rounds, int *cnt,
                      int *cols, double *lb, double *ub) {
  if (!api) api = &g_hip_api;
  if (!prob || !root || max_rounds < 1 || !infeasible || !rounds || !cnt || !cols || !lb || !ub) return -1;
  HostModel M;
  *infeasible = *rounds = *cnt = 0;
  int rc = read_host_model(api, root, M);
  if (rc != 0) return rc;
  PropOut out;
  rc = prop_host(api, M, prob, max_rounds, out);
  if (rc != 0) return rc;
  *infeasible = out.infeasible;
  *rounds = out.rounds;
  list_out(out.list, cnt, cols, lb, ub);
  return 0;
}

int mvx_bnb_cut_scores(const mvx_lp_api *api, const void *prob, int k, const double *vals, double *dot, double *gram) {
  if (!api) api = &g_hip_api;
  if (!prob || k < 1 || !vals || !dot || !gram || api->get_status(prob) != MVX_OPT) return -1;
  cut_scores_host(api, prob, k, vals, dot, gram);
  return 0;
}

int mvx_bnb_cut_select(int k, const double *eff, const double *gram, int K, double maxpar, int budget, int *taken, int *ntaken) {
  if (k < 0 || K < 1 || !(maxpar > 0.0 && maxpar <= 1.0) || budget < 0 || !ntaken || (k > 0 && (!eff || !gram || !taken))) return -1;
  std::vector<int> got = cut_select(k, eff, gram, K, maxpar, budget);
  for (size_t i = 0; i < got.size(); i++) taken[i] = got[i];
  *ntaken = (int)got.size();
  return 0;
}

int mvx_bnb_purge_ages(int k, const int *basic, int A, unsigned char *age, int *out, int *nout) {
  if (k < 0 || A < 1 || A > 64 || !nout || (k > 0 && (!basic || !age || !out))) return -1;
  int w = 0;
  for (int t = 0; t < k; t++) {
    if (age[t] == 255) continue; // a dead row
    if (!basic[t]) age[t] = 0;
    else if (age[t] < 254) age[t]++;
    if (age[t] >= A) out[w++] = t;
  }
  *nout = w;
  return 0;
}

int mvx_bnb_cut_loop_purge(const mvx_lp_api *api, void *prob, int rounds, int K, double maxpar, int families, int purge,
                           long long *counters, double *bounds) {
  if (!api) api = &g_hip_api;
  if (!prob || rounds < 1 || rounds > 64 || K < 0 || K > 4096 || !(maxpar == 0.0 || (maxpar > 0.0 && maxpar <= 1.0)) || families < 0 ||
      families > 3 || purge < 0 || purge > 64 || !counters || !bounds)
    return -1;
  CutLoopOut lo;
  const int rc = cut_loop(api, prob, rounds, K, maxpar, families, purge, lo);
  counters[0] = lo.rounds; counters[1] = lo.candidates; counters[2] = lo.rows; counters[3] = lo.lps; counters[4] = lo.pivots;
  counters[5] = lo.conflicts; counters[6] = lo.clique_cands; counters[7] = lo.clique_rows;
  counters[8] = lo.purged; counters[9] = lo.rows - lo.purged;
  bounds[0] = lo.bound0; bounds[1] = lo.bound;
  return rc;
}

int mvx_bnb_cut_loop_families(const mvx_lp_api *api, void *prob, int rounds, int K, double maxpar, int families, long long *counters,
                              double *bounds) {
  if (!counters) return -1;
  long long all[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  const int rc = mvx_bnb_cut_loop_purge(api, prob, rounds, K, maxpar, families, 0, all, bounds);
  if (rc != -1) std::copy(all, all + 8, counters);
  return rc;
}

int mvx_bnb_cut_loop(const mvx_lp_api *api, void *prob, int rounds, int K, double maxpar, long long *counters, double *bounds) {
  if (!counters) return -1;
  long long all[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const int rc = mvx_bnb_cut_loop_families(api, prob, rounds, K, maxpar, 1, all, bounds);
  if (rc != -1) std::copy(all, all + 5, counters);
  return rc;
}

int mvx_bnb_polish(const mvx_lp_api *api, const void *root, double *x, int max_moves, double *obj, int *moves, int *ok) {
  if (!api) api = &g_hip_api;
  if (!root || !x || !obj || !moves || !ok || max_moves < 1 || max_moves > 100000) return -1;
  HostModel M;
  const int rc = read_host_model(api, root, M);
  if (rc != 0) return rc;
  return polish_host(M, x, max_moves, obj, moves, ok);
}

int mvx_bnb_kkt_values(int m, int n, const double *rows, const double *c, const double *xs, const double *xr, const double *lam,
                       const double *dj, const double *lb, const double *ub, const int *stat, int dir, double *val, int *ind, double *r_pe,
                       double *r_de) {
  if (m < 1 || n < 1 || !rows || !c || !xs || !xr || !lam || !dj || !lb || !ub || !stat || !val || !ind || (dir != MVX_MIN && dir != MVX_MAX))
    return -1;
  kkt_host(m, n, rows, c, xs, xr, lam, dj, lb, ub, stat, dir == MVX_MIN ? 1.0 : -1.0, val, ind, r_pe, r_de);
  return 0;
}

int mvx_bnb_kkt(const mvx_lp_api *api, const void *prob, double *val, int *ind, double *r_pe, double *r_de) {
  if (!api) api = &g_hip_api;
  if (!prob || !val || !ind) return -1;
  return kkt_through_table(api, prob, val, ind, r_pe, r_de);
}

int mvx_bnb_farkas_values(int m, int n, const double *T, const int *head, const int *nb, const double *rows, const double *lb,
                          const double *ub, double *val, int *ind, double *y) {
  if (m < 1 || n < 1 || !T || !head || !nb || !rows || !lb || !ub || !val || !ind) return -1;
  farkas_host(m, n, T, head, nb, rows, lb, ub, val, ind, y);
  return 0;
}

int mvx_bnb_farkas(const mvx_lp_api *api, const void *prob, double *val, int *ind, double *y) {
  if (!api) api = &g_hip_api;
  if (!prob || !val || !ind) return -1;
  return farkas_through_table(api, prob, val, ind, y);
}

int mvx_bnb_ray(const mvx_lp_api *api, const void *prob, double *val, int *ind, double *d) {
  if (!api) api = &g_hip_api;
  if (!prob || !val || !ind) return -1;
  return ray_through_table(api, prob, val, ind, d);
}

int mvx_bnb_ranges(const mvx_lp_api *api, const void *prob, double *val, int *var) {
  if (!api) api = &g_hip_api;
  if (!prob || !val || !var) return -1;
  RangeView V;
  const int rc = read_range_view(api, prob, V);
  if (rc != 0) return rc;
  host_ranges(V, default_smcp().tol_piv, val, var);
  return 0;
}

// The host twin of k_addcols' pricing pass (DESIGN.md "Column append (add_cols)").  Image t, tableau row p: base + S, where
// S sums w_q * T[p][q] over the non-basic positions q that hold an auxiliary i (w_q = -cols[t][i]) in 64 chains -- chain l takes
// q = l+1, l+65, ... ascending, fma from +0.0, zero weights skipped -- the chains are combined by s[l] += s[l+h], h = 32 .. 1,
// and the base (obj[t] in row 0, the coefficient of the row's basic auxiliary below it, else 0) is added last.
int mvx_bnb_price_cols(const mvx_lp_api *api, const void *prob, int k, const double *cols, const double *obj, double *dj, double *img) {
  if (!api) api = &g_hip_api;
  if (!prob || k < 1 || !cols || !obj || !dj) return -1;
  if (!api->get_num_rows || !api->get_num_cols || !api->get_tableau || !api->get_basis) return -2;
  const int m = api->get_num_rows(prob), n = api->get_num_cols(prob);
  const size_t ldt = (size_t)n + 1, crow = (size_t)m + 1;
  std::vector<double> T((size_t)(m + 1) * ldt, 0.0);
  std::vector<int> head((size_t)m + 1, 0), nb((size_t)n + 1, 0), flag((size_t)n + 1, 0);
  if (api->get_basis(prob, head.data(), nb.data(), flag.data()) != 0 || api->get_tableau(prob, T.data()) != 0) return -2;
  std::vector<double> w((size_t)n + 1, 0.0);
  const int rows = img ? m + 1 : 1;
  for (int t = 0; t < k; t++) {
    const double *a = cols + (size_t)t * crow;
    for (int q = 1; q <= n; q++) w[(size_t)q] = nb[(size_t)q] <= m ? -a[(size_t)nb[(size_t)q]] : 0.0;
    for (int p = 0; p < rows; p++) {
      const double *Tp = T.data() + (size_t)p * ldt;
      double s[64];
      for (int l = 0; l < 64; l++) {
        double acc = 0.0;
        for (int q = l + 1; q <= n; q += 64)
          if (w[(size_t)q] != 0.0) acc = std::fma(w[(size_t)q], Tp[q], acc);
        s[l] = acc;
      }
      for (int h = 32; h >= 1; h >>= 1)
        for (int l = 0; l < h; l++) s[l] = s[l] + s[l + h];
      const double base = p == 0 ? obj[t] : (head[(size_t)p] <= m ? a[(size_t)head[(size_t)p]] : 0.0);
      const double v = base + s[0];
      if (img) img[(size_t)t * crow + (size_t)p] = v;
      if (p == 0) dj[t] = v;
    }
  }
  return 0;
}

// The host twins of mvx_pool_price, from numbers only (DESIGN.md "Sifting (sift)"; the loops are sift_host.hpp's): the reduced
// costs in the written order with the attractive rule, and the selection.
int mvx_bnb_pool_price_values(int m, int N, const double *cols, const double *obj, const int *type, const double *y, int dir, double tol,
                              double *dj, unsigned char *attractive) {
  if (m < 0 || N < 0 || !dj || (N > 0 && (!cols || !obj || !type)) || (m > 0 && !y) || (dir != MVX_MIN && dir != MVX_MAX)) return -1;
  const size_t crow = (size_t)m + 1;
  const double sgn = dir == MVX_MAX ? 1.0 : -1.0;
  dj[0] = 0.0;
  if (attractive) attractive[0] = 0;
  for (int j = 1; j <= N; j++) {
    const double d = mvx_sifting::price_one(m, cols + (size_t)(j - 1) * crow + 1, y, obj[j - 1]);
    dj[j] = d;
    if (attractive) attractive[j] = mvx_sifting::attractive(mvx_sifting::flag_of(type[j - 1]), d, sgn, tol) ? 1 : 0;
  }
  return 0;
}
int mvx_bnb_pool_select(int N, const double *dj, const unsigned char *attractive, const unsigned char *skip, int K, int *pick, int *npick) {
  if (N < 0 || K < 0 || !dj || !attractive || !npick || (K > 0 && !pick)) return -1;
  mvx_sifting::select(N, dj, attractive, skip, K, pick, npick);
  return 0;
}

int mvx_bnb_print_ranges(const mvx_lp_api *api, const void *prob, const double *val, const int *var, const char *path) {
  if (!api) api = &g_hip_api;
  if (!prob || !val || !var) return -1;
  RangeView V;
  const int rc = read_range_view(api, prob, V);
  if (rc != 0) return rc;
  const int m = V.m, n = V.n;
  std::vector<int> row((size_t)m + n + 1, 0), posn((size_t)m + n + 1, 0); // tableau row / non-basic position of a variable
  for (int i = 1; i <= m; i++) row[(size_t)V.head[(size_t)i]] = i;
  for (int q = 1; q <= n; q++) posn[(size_t)V.nb[(size_t)q]] = q;
  FILE *out = path ? std::fopen(path, "w") : stdout;
  if (!out) return -4;
  const bool named = api == &g_hip_api && mvx_get_col_name; // names live in the gfx950 engine's handles only
  for (int k = 1; k <= m + n; k++) {
    char name[64];
    const char *nm = (named && k > m) ? mvx_get_col_name((const mvx_prob *)prob, k - m) : nullptr;
    if (!nm) {
      std::snprintf(name, sizeof name, "%c%d", k <= m ? 'R' : 'C', k <= m ? k : k - m);
      nm = name;
    }
    const char *st = "B";
    double x = 0.0;
    if (row[(size_t)k]) {
      x = V.T[(size_t)row[(size_t)k] * ((size_t)n + 1)];
    } else {
      const int f = V.flag[(size_t)posn[(size_t)k]];
      st = f == MVX_NL ? "NL" : f == MVX_NU ? "NU" : f == MVX_NF ? "NF" : "NS";
      x = f == MVX_NL ? V.lb[(size_t)k] : f == MVX_NU ? V.ub[(size_t)k] : f == MVX_NS ? V.lb[(size_t)k] : 0.0;
    }
    const double *v = val + (size_t)k * 6;
    const int *w = var + (size_t)k * 4;
    std::fprintf(out, "%d %s %s %.17g %.17g %d %.17g %d %.17g %.17g %.17g %d %.17g %d\n", k, nm, st, x, v[0], w[0], v[1], w[1], v[2], v[3],
                 v[4], w[2], v[5], w[3]);
  }
  const bool bad = std::ferror(out) != 0;
  if (path) {
    if (std::fclose(out) != 0) return -4;
  } else {
    std::fflush(out);
  }
  return bad ? -4 : 0;
}

int mvx_bnb_conflict_graph(const mvx_lp_api *api, const void *model, unsigned long long *adj, long long *edges) {
  if (!api) api = &g_hip_api;
  if (!model || !adj || !edges) return -1;
  *edges = 0;
  HostModel M;
  const int rc = read_host_model(api, model, M);
  if (rc != 0) return rc;
  return conflict_graph_host(api, M, model, adj, edges);
}

int mvx_bnb_clique_cuts(int n, const unsigned long long *adj, const double *x, int max_cuts, double *vals, double *rhs, int *count) {
  if (n < 0 || max_cuts < 0 || !adj || !x || !count || (max_cuts > 0 && (!vals || !rhs))) return -1;
  const std::vector<std::vector<int>> got = clique_cuts(n, adj, x, max_cuts);
  const size_t row = (size_t)n + 1;
  for (size_t t = 0; t < got.size(); t++) {
    std::fill(vals + t * row, vals + (t + 1) * row, 0.0);
    for (int j : got[t]) vals[t * row + (size_t)j] = -1.0;
    rhs[t] = -1.0;
  }
  *count = (int)got.size();
  return 0;
}

int mvx_bnb_clique_masks(const mvx_lp_api *api, const void *prob, int n, const unsigned long long *adj, int max_cuts, int *cnt,
                         unsigned long long *q, double *sum) {
  if (!api) api = &g_hip_api;
  if (!prob || !adj || !cnt || !q || !sum || max_cuts < 1 || max_cuts > 64 || n < 0) return -1;
  if (!api->get_num_cols || !api->get_status || (!api->get_col_prim_all && !api->get_col_prim)) return -2;
  if (api->get_num_cols(prob) != n) return -1;
  if (api->get_status(prob) != MVX_OPT) return -3;
  const size_t W = ((size_t)n + 1 + 63) / 64;
  std::vector<double> x((size_t)n + 1, 0.0);
  if (api->get_col_prim_all) api->get_col_prim_all(prob, x.data());
  else
    for (int j = 1; j <= n; j++) x[(size_t)j] = api->get_col_prim(prob, j);
  const std::vector<std::vector<int>> got = clique_cuts(n, adj, x.data(), max_cuts);
  std::fill(q, q + (size_t)max_cuts * W, 0ULL);
  std::fill(sum, sum + max_cuts, 0.0);
  for (size_t t = 0; t < got.size(); t++) {
    double s = 0.0;
    for (int j : got[t]) {
      q[t * W + (size_t)j / 64] |= 1ULL << (j % 64);
      s = s + x[(size_t)j];
    }
    sum[t] = s;
  }
  *cnt = (int)got.size();
  return 0;
}

int mvx_bnb_node_cuts(const mvx_lp_api *api, void *a, const mvx_bnb_params *params) {
  if (!api) api = &g_hip_api;
  CutPool pool(api); // this node's cuts only: a caller that needs bs.cpp:73's pool across nodes keeps the order itself
  return add_node_cuts(api, a, *params, params->reference_quirks != 0, pool);
}

int mvx_printInfo(const mvx_lp_api *api, const void *prob, int quirks, int *violated, int *nviolated) {
  auto r = printInfo(api ? api : &g_hip_api, prob, quirks != 0);
  *nviolated = (int)r.second.size();
  for (size_t k = 0; k < r.second.size(); k++) violated[k] = r.second[k];
  return r.first;
}

int mvx_generateCut3(const mvx_lp_api *api, const void *prob, int j, int *inds, double *vals, double *lb) {
  CutContainer c = generateCut3(api ? api : &g_hip_api, prob, j);
  if (c.oid == -1) return -1;
  std::memcpy(inds, c.inds.data(), c.inds.size() * sizeof(int));
  std::memcpy(vals, c.vals.data(), c.vals.size() * sizeof(double));
  *lb = c.lb;
  return 0;
}

} // extern "C"
