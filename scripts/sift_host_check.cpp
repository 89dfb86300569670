// Stand-alone host check of sifting's device-free code (mvolps_amd/csrc/sift_host.hpp: the column pool's model layer and the two
// loops mvx_pool_price is defined by), meant to be built with a sanitizer and run on the CPU:
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all scripts/sift_host_check.cpp -o sift_host_check
// It walks every refusal, pools over 0, 1, 63..65 and 130 rows that grow in several calls, get_col with and without outputs, the
// pricing loop against a plain restatement, and the selection at K = 0, K > count, with skips, ties, zeros and denormals.
#include <cassert>
#include <cstdio>
#include <limits>
#include <random>

#include "../mvolps_amd/csrc/sift_host.hpp"

using namespace mvx_sifting;

int main() {
  std::mt19937_64 rng(7);
  std::normal_distribution<double> nd(0.0, 3.0);
  const double nan = std::numeric_limits<double>::quiet_NaN();
  long checks = 0;
  for (int m : {0, 1, 63, 64, 65, 130}) {
    PoolHost S;
    pool_init(S, m);
    const size_t crow = (size_t)m + 1;
    std::vector<double> all_cols, all_obj;
    std::vector<int> all_type;
    const int types[6] = {MVX_LO, MVX_UP, MVX_DB, MVX_FR, MVX_FX, MVX_DB};
    const double ubs[6] = {0.0, 0.0, 2.5, 0.0, 0.0, 0.0};
    for (int k : {1, 7, 300}) {
      std::vector<double> cols((size_t)k * crow), obj((size_t)k), lb((size_t)k, 0.0), ub((size_t)k);
      std::vector<int> type((size_t)k), kind((size_t)k);
      for (int t = 0; t < k; t++) {
        cols[(size_t)t * crow] = nan; // entry 0 is not read
        for (int i = 1; i <= m; i++) cols[(size_t)t * crow + (size_t)i] = (rng() % 3 == 0) ? 0.0 : nd(rng);
        obj[(size_t)t] = nd(rng);
        type[(size_t)t] = types[t % 6];
        ub[(size_t)t] = ubs[t % 6];
        kind[(size_t)t] = t % 2 ? MVX_IV : MVX_CV;
      }
      // refusals: nothing changes
      const int N0 = S.N;
      assert(pool_add(S, 0, cols.data(), obj.data(), type.data(), lb.data(), ub.data(), nullptr) == -1);
      assert(pool_add(S, k, nullptr, obj.data(), type.data(), lb.data(), ub.data(), nullptr) == -1);
      {
        std::vector<int> bad = type;
        bad[(size_t)k - 1] = 9;
        assert(pool_add(S, k, cols.data(), obj.data(), bad.data(), lb.data(), ub.data(), nullptr) == -1);
        std::vector<double> l2 = lb;
        bad = type;
        bad[0] = MVX_LO;
        l2[0] = 1.0; // cannot rest at zero
        assert(pool_add(S, k, cols.data(), obj.data(), bad.data(), l2.data(), ub.data(), nullptr) == -1);
        bad[0] = MVX_FX;
        l2[0] = 3.0;
        assert(pool_add(S, k, cols.data(), obj.data(), bad.data(), l2.data(), ub.data(), nullptr) == -1);
        bad[0] = MVX_UP;
        std::vector<double> u2 = ub;
        u2[0] = -2.0;
        assert(pool_add(S, k, cols.data(), obj.data(), bad.data(), lb.data(), u2.data(), nullptr) == -1);
        bad[0] = MVX_DB;
        l2[0] = 1.0;
        u2[0] = 4.0;
        assert(pool_add(S, k, cols.data(), obj.data(), bad.data(), l2.data(), u2.data(), nullptr) == -1);
        std::vector<int> k2 = kind;
        k2[0] = 7;
        assert(pool_add(S, k, cols.data(), obj.data(), type.data(), lb.data(), ub.data(), k2.data()) == -1);
        if (m > 0) {
          std::vector<double> c2 = cols;
          c2[crow - 1] = nan;
          assert(pool_add(S, k, c2.data(), obj.data(), type.data(), lb.data(), ub.data(), nullptr) == -1);
        }
      }
      assert(S.N == N0 && S.cols.size() == (size_t)N0 * (size_t)S.ldp);
      assert(pool_add(S, k, cols.data(), obj.data(), type.data(), lb.data(), ub.data(), (k == 7) ? nullptr : kind.data()) == 0);
      assert(S.N == N0 + k);
      all_cols.insert(all_cols.end(), cols.begin(), cols.end());
      all_obj.insert(all_obj.end(), obj.begin(), obj.end());
      all_type.insert(all_type.end(), type.begin(), type.end());
      checks += 12;
    }
    const int N = S.N;
    std::vector<double> col(crow);
    for (int j = 1; j <= N; j++) {
      double o, l, u;
      int ty, kd;
      assert(pool_get(S, j, col.data(), &o, &ty, &l, &u, &kd) == 0 && col[0] == 0.0);
      assert(std::memcmp(col.data() + 1, &all_cols[(size_t)(j - 1) * crow + 1], (size_t)m * 8) == 0);
      assert(std::memcmp(&o, &all_obj[(size_t)j - 1], 8) == 0 && ty == all_type[(size_t)j - 1]);
      assert(pool_get(S, j, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
    }
    assert(pool_get(S, 0, col.data(), nullptr, nullptr, nullptr, nullptr, nullptr) == -1 && pool_get(S, N + 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == -1);
    // pricing: y with zeros and signed zeros, y[0] not read
    std::vector<double> y((size_t)m + 1), dj((size_t)N + 1, 0.0);
    std::vector<unsigned char> att((size_t)N + 1, 0), skip((size_t)N + 1, 0);
    y[0] = nan;
    for (int i = 1; i <= m; i++) y[(size_t)i] = (rng() % 4 == 0) ? 0.0 : (rng() % 9 == 0) ? -0.0 : nd(rng);
    for (int j = 1; j <= N; j++) {
      const double d = price_one(m, S.cols.data() + (size_t)(j - 1) * (size_t)S.ldp, y.data(), S.obj[(size_t)j - 1]);
      long double ref = S.obj[(size_t)j - 1], mag = std::fabs(S.obj[(size_t)j - 1]);
      for (int i = 1; i <= m; i++) {
        ref -= (long double)all_cols[(size_t)(j - 1) * crow + (size_t)i] * y[(size_t)i];
        mag += std::fabs((long double)all_cols[(size_t)(j - 1) * crow + (size_t)i] * y[(size_t)i]);
      }
      assert(std::fabs((double)(d - ref)) <= (double)(((m + 63) / 64 + 9) * 1.2e-16L * mag));
      dj[(size_t)j] = d;
      att[(size_t)j] = attractive(flag_of(S.type[(size_t)j - 1]), d, j % 2 ? 1.0 : -1.0, 1e-9);
      skip[(size_t)j] = j % 5 == 0;
      checks++;
    }
    // ties, zeros and denormals among the candidates
    if (N > 20) {
      dj[3] = dj[11] = dj[17] = 4.0;
      dj[5] = 0.0, dj[6] = -0.0, dj[7] = 5e-324, dj[8] = -1e-320;
      for (int j : {3, 11, 17, 5, 6, 7, 8}) att[(size_t)j] = 1, skip[(size_t)j] = 0;
    }
    std::vector<int> pick((size_t)N + 1);
    for (int K : {0, 1, 7, N, N + 5}) {
      for (const unsigned char *sk : {(const unsigned char *)nullptr, (const unsigned char *)skip.data()}) {
        int np = -1;
        select(N, dj.data(), att.data(), sk, K, pick.data(), &np);
        int cnt = 0;
        for (int j = 1; j <= N; j++) cnt += att[(size_t)j] && !(sk && sk[j]);
        assert(np == std::min(K, cnt));
        for (int t = 0; t < np; t++) assert(att[(size_t)pick[(size_t)t]] && !(sk && sk[pick[(size_t)t]]));
        for (int t = 0; t + 1 < np; t++) {
          const uint64_t a = abs_bits(dj[(size_t)pick[(size_t)t]]), b = abs_bits(dj[(size_t)pick[(size_t)t + 1]]);
          assert(a > b || (a == b && pick[(size_t)t] < pick[(size_t)t + 1]));
        }
        checks += np + 1;
      }
    }
  }
  std::printf("sift_host_check: %ld checks passed\n", checks);
  return 0;
}
