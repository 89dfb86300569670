// sift_host.hpp -- the host side of sifting (DESIGN.md "Sifting (sift)") that needs neither a handle nor a device: the column
// pool's model layer (mvx_pool_create .. mvx_pool_get_col wrap it in capi.cpp) and the two loops mvx_pool_price is defined by
// (mvx_bnb_pool_price_values / mvx_bnb_pool_select wrap them in bnb.cpp).  Header-only and free of the engine's headers, so that
// a stand-alone program can run all of it under a sanitizer.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/mvx.h"

namespace mvx_sifting {

constexpr int POOL_LD_ALIGN = 64; // doubles: a pool column is a whole number of 512-byte wave rows

// the non-basic status a column of this bound type starts with, its bounds as the engine keeps them (+-inf when absent) and the
// value it rests at: the rules of mvx_set_col_bnds / mvx_add_dense_cols
inline int flag_of(int type) { return type == MVX_FR ? MVX_NF : type == MVX_LO || type == MVX_DB ? MVX_NL : type == MVX_UP ? MVX_NU : MVX_NS; }
inline void bounds_of(int type, double lb, double ub, double *olb, double *oub) {
  const double inf = HUGE_VAL;
  *olb = (type == MVX_LO || type == MVX_DB || type == MVX_FX) ? lb : -inf;
  *oub = (type == MVX_UP || type == MVX_DB) ? ub : type == MVX_FX ? lb : inf;
}
inline double rest_of(int flag, double lb, double ub) { return flag == MVX_NL || flag == MVX_NS ? lb : flag == MVX_NU ? ub : 0.0; }

// The host copy of a pool: column j = 1..N lies at cols[(j-1)*ldp .. ], model row i at entry i-1, zero behind row m.  The same
// image goes to the device, so the upload of a range of columns is one copy.
struct PoolHost {
  int m = 0, N = 0, ldp = 0;
  std::vector<double> cols, obj, lb, ub; // lb / ub as given
  std::vector<int> type, kind;
};

inline void pool_init(PoolHost &S, int m) {
  S = PoolHost();
  S.m = m;
  S.ldp = (m + POOL_LD_ALIGN - 1) / POOL_LD_ALIGN * POOL_LD_ALIGN;
}

// mvx_add_dense_cols' refusals plus the zero-rest rule; nothing is read behind a refusal's cause and nothing is written
inline bool pool_cols_ok(int m, int k, const double *cols, const double *obj, const int *type, const double *lb, const double *ub,
                         const int *kind) {
  if (k < 1 || !cols || !obj || !type || !lb || !ub) return false;
  const size_t crow = (size_t)m + 1;
  for (int t = 0; t < k; t++) {
    if (type[t] < MVX_FR || type[t] > MVX_FX) return false;
    if (std::isnan(obj[t]) || std::isnan(lb[t]) || std::isnan(ub[t])) return false;
    if (type[t] == MVX_DB && lb[t] > ub[t]) return false;
    if (kind && kind[t] != MVX_CV && kind[t] != MVX_IV) return false;
    for (int i = 1; i <= m; i++)
      if (std::isnan(cols[(size_t)t * crow + (size_t)i])) return false;
    double l, u;
    bounds_of(type[t], lb[t], ub[t], &l, &u);
    if (rest_of(flag_of(type[t]), l, u) != 0.0) return false; // the column cannot rest at zero
  }
  return true;
}

inline int pool_add(PoolHost &S, int k, const double *cols, const double *obj, const int *type, const double *lb, const double *ub,
                    const int *kind) {
  if (!pool_cols_ok(S.m, k, cols, obj, type, lb, ub, kind)) return -1;
  if ((long long)S.N + k > 0x7ffffff0LL) return -1;
  const size_t crow = (size_t)S.m + 1, ldp = (size_t)S.ldp, N0 = (size_t)S.N;
  S.cols.resize((N0 + (size_t)k) * ldp, 0.0);
  for (int t = 0; t < k; t++)
    if (S.m > 0) std::memcpy(&S.cols[(N0 + (size_t)t) * ldp], cols + (size_t)t * crow + 1, (size_t)S.m * 8);
  S.obj.insert(S.obj.end(), obj, obj + k);
  S.lb.insert(S.lb.end(), lb, lb + k);
  S.ub.insert(S.ub.end(), ub, ub + k);
  S.type.insert(S.type.end(), type, type + k);
  for (int t = 0; t < k; t++) S.kind.push_back(kind ? kind[t] : MVX_CV);
  S.N += k;
  return 0;
}

inline int pool_get(const PoolHost &S, int j, double *col, double *obj, int *type, double *lb, double *ub, int *kind) {
  if (j < 1 || j > S.N) return -1;
  const size_t t = (size_t)j - 1;
  if (col) {
    col[0] = 0.0;
    if (S.m > 0) std::memcpy(col + 1, &S.cols[t * (size_t)S.ldp], (size_t)S.m * 8);
  }
  if (obj) *obj = S.obj[t];
  if (type) *type = S.type[t];
  if (lb) *lb = S.lb[t];
  if (ub) *ub = S.ub[t];
  if (kind) *kind = S.kind[t];
  return 0;
}

// S_j + obj_j in the written order: 64 chains over the model rows, chain l taking i = l+1, l+65, ... ascending with
// fma(-a_i, y_i, acc) from +0.0 and skipping rows with y_i == 0; s[l] += s[l+h], h = 32 .. 1; obj added last.  a[i-1] is the
// coefficient of row i, y[i] its weight
inline double price_one(int m, const double *a, const double *y, double obj) {
  double s[64];
  for (int l = 0; l < 64; l++) {
    double acc = 0.0;
    for (int i = l + 1; i <= m; i += 64)
      if (y[i] != 0.0) acc = std::fma(-a[i - 1], y[i], acc);
    s[l] = acc;
  }
  for (int h = 32; h >= 1; h >>= 1)
    for (int l = 0; l < h; l++) s[l] = s[l] + s[l + h];
  return obj + s[0];
}

// the engine's primal pricing rule on a non-basic column of status `flag`: sgn +1 under MVX_MAX, -1 under MVX_MIN
inline bool attractive(int flag, double d, double sgn, double tol) {
  const double v = sgn * d;
  return flag == MVX_NL ? v > tol : flag == MVX_NU ? v < -tol : flag == MVX_NF ? std::fabs(d) > tol : false;
}

inline uint64_t abs_bits(double d) {
  uint64_t b;
  std::memcpy(&b, &d, 8);
  return b & 0x7fffffffffffffffULL;
}

// the min(K, #candidates) candidates of largest |dj| (by its bits), descending, ties to the lower column
inline void select(int N, const double *dj, const unsigned char *att, const unsigned char *skip, int K, int *pick, int *npick) {
  std::vector<int> c;
  for (int j = 1; j <= N; j++)
    if (att[j] && !(skip && skip[j])) c.push_back(j);
  const size_t kk = std::min(c.size(), (size_t)(K < 0 ? 0 : K));
  std::partial_sort(c.begin(), c.begin() + (long)kk, c.end(), [&](int a, int b) {
    const uint64_t ka = abs_bits(dj[a]), kb = abs_bits(dj[b]);
    return ka != kb ? ka > kb : a < b;
  });
  for (size_t t = 0; t < kk; t++) pick[t] = c[t];
  *npick = (int)kk;
}

} // namespace mvx_sifting
