// csrc/xcd_placement.h on the CPU (tests/test_xcd_placement_cpu.py): the placement table block -> tile of the remap kernels and the
// entry block (x, y) reads of it, over every tile grid 1..12 x 1..40, the four MDC_ORDER_* modes, rotation off and on, 1..40 frame
// groups.  Prints one "<check> ok" line per property, "FAIL ..." lines otherwise; exit status 1 on any failure.
#include "xcd_placement.h"

#include <cstdio>
#include <set>
#include <vector>

#include "xcd_placement_parent_tables.inc"

static int g_fail = 0;
#define EXPECT(cond, ...)          \
  do {                             \
    if (!(cond)) {                 \
      if (g_fail < 40) {           \
        std::printf("FAIL ");      \
        std::printf(__VA_ARGS__);  \
        std::printf("\n");         \
      }                            \
      g_fail++;                    \
    }                              \
  } while (0)

// The table as it was built before the rotation existed (tile_order of mdc_plan.hip, kept here word for word as the reference
// of "rotation off").
static void parent_bisect(int x0, int y0, int x1, int y1, int parts, int tx, std::vector<std::vector<int>>& out) {
  if (parts == 1) {
    std::vector<int> v;
    for (int y = y0; y < y1; y++)
      for (int x = x0; x < x1; x++) v.push_back(y * tx + x);
    out.push_back(v);
    return;
  }
  if (x1 - x0 > y1 - y0) {
    const int xm = x0 + (x1 - x0 + 1) / 2;
    parent_bisect(x0, y0, xm, y1, parts / 2, tx, out);
    parent_bisect(xm, y0, x1, y1, parts / 2, tx, out);
  } else {
    const int ym = y0 + (y1 - y0 + 1) / 2;
    parent_bisect(x0, y0, x1, ym, parts / 2, tx, out);
    parent_bisect(x0, ym, x1, y1, parts / 2, tx, out);
  }
}
static std::vector<int> parent_tile_order(int tx, int ty, int mode) {
  const int n = tx * ty;
  std::vector<std::vector<int>> per_xcd(8);
  if (mode == MDC_ORDER_BLOCKS2D && tx * ty >= 8) {
    per_xcd.clear();
    parent_bisect(0, 0, tx, ty, 8, tx, per_xcd);
  } else if (mode == MDC_ORDER_IDENTITY) {
    for (int t = 0; t < n; t++) per_xcd[t % 8].push_back(t);
  } else if (mode == MDC_ORDER_ROWS && ty >= 8) {
    int r = 0;
    for (int k = 0; k < 8; k++) {
      const int rows = ty / 8 + (k < ty % 8 ? 1 : 0);
      for (int y = r; y < r + rows; y++)
        for (int x = 0; x < tx; x++) per_xcd[k].push_back(y * tx + x);
      r += rows;
    }
  } else {
    const int per = (n + 7) / 8;
    for (int t = 0; t < n; t++) per_xcd[t / per].push_back(t);
  }
  size_t slots = 0;
  for (const auto& v : per_xcd) slots = std::max(slots, v.size());
  std::vector<int> order(slots * 8, -1);
  for (int k = 0; k < 8; k++)
    for (size_t j = 0; j < per_xcd[k].size(); j++) order[j * 8 + k] = per_xcd[k][j];
  return order;
}

// tiles that the blocks of residue k (one XCD) run in frame group y, in block order
static std::vector<int> share(const std::vector<int>& order, int k, int y, bool rot) {
  std::vector<int> v;
  for (int x = k; x < (int)order.size(); x += 8) {
    const int t = order[mdc::xcd_table_entry(x, y, rot)];
    if (t >= 0) v.push_back(t);
  }
  return v;
}

// does the share keep the mode's neighbourhood?
static bool neighbourhood(const std::vector<int>& v, int tx, int ty, int mode) {
  if (v.empty()) return true;
  const int n = tx * ty;
  if (mode == MDC_ORDER_IDENTITY) {  // every 8th tile, ascending
    for (size_t i = 1; i < v.size(); i++)
      if (v[i] != v[i - 1] + 8) return false;
    return true;
  }
  if (mode == MDC_ORDER_BLOCKS2D && n >= 8) {  // a full rectangle of the grid, row-major
    int x0 = tx, x1 = -1, y0 = ty, y1 = -1;
    for (int t : v) x0 = std::min(x0, t % tx), x1 = std::max(x1, t % tx), y0 = std::min(y0, t / tx), y1 = std::max(y1, t / tx);
    if ((size_t)(x1 - x0 + 1) * (y1 - y0 + 1) != v.size()) return false;
    size_t i = 0;
    for (int y = y0; y <= y1; y++)
      for (int x = x0; x <= x1; x++)
        if (v[i++] != y * tx + x) return false;
    return true;
  }
  for (size_t i = 1; i < v.size(); i++)  // bands, rows (and their fall-backs): a contiguous run
    if (v[i] != v[i - 1] + 1) return false;
  if (mode == MDC_ORDER_ROWS && ty >= 8) return v[0] % tx == 0 && v.size() % tx == 0;  // of whole tile rows
  return true;
}

int main() {
  const int modes[4] = {MDC_ORDER_BANDS, MDC_ORDER_ROWS, MDC_ORDER_IDENTITY, MDC_ORDER_BLOCKS2D};
  int f0 = g_fail;
  auto done = [&](const char* what) {
    if (g_fail == f0) std::printf("%s ok\n", what);
    f0 = g_fail;
  };

  // 1. the entry formula: a permutation of every row of 8, the identity when rotation is off
  for (int y = 0; y < 100; y++)
    for (int x = 0; x < 256; x++) {
      EXPECT(mdc::xcd_table_entry(x, y, false) == x, "entry(%d, %d, off)", x, y);
      const int e = mdc::xcd_table_entry(x, y, true);
      EXPECT(e == ((x & ~7) | ((x + y) & 7)), "entry(%d, %d, on) = %d", x, y, e);
    }
  done("entry formula");

  // 2. rotation off = the parent's table, entry for entry; 5 x 15 and 5 x 30 as literals
  for (int tx = 1; tx <= 12; tx++)
    for (int ty = 1; ty <= 40; ty++)
      for (int mode : modes) EXPECT(mdc::tile_order(tx, ty, mode, false) == parent_tile_order(tx, ty, mode), "rotation off differs from the parent: %d x %d mode %d", tx, ty, mode);
  done("rotation off is the parent's table");
  for (int m = 0; m < 4; m++) {
    EXPECT(mdc::tile_order(5, 15, m, false) == std::vector<int>(kParent5x15[m], kParent5x15[m] + kParent5x15Len[m]), "5 x 15 mode %d literal", m);
    EXPECT(mdc::tile_order(5, 30, m, false) == std::vector<int>(kParent5x30[m], kParent5x30[m] + kParent5x30Len[m]), "5 x 30 mode %d literal", m);
  }
  EXPECT(mdc::tile_order(5, 15, MDC_ORDER_BANDS) == mdc::tile_order(5, 15, MDC_ORDER_BANDS, false), "rotation is off by default");
  done("5x15 and 5x30 literals");

  long long cases = 0;
  int f_cover = 0, f_neigh = 0, f_even = 0, f_equal = 0, f_bands = 0;
  for (int tx = 1; tx <= 12; tx++)
    for (int ty = 1; ty <= 40; ty++)
      for (int mode : modes)
        for (int rot = 0; rot < 2; rot++) {
          const int n = tx * ty;
          const std::vector<int> order = mdc::tile_order(tx, ty, mode, rot != 0);
          const int nb = (int)order.size();
          int before_f = g_fail;
          EXPECT(nb > 0 && nb % 8 == 0, "%d x %d mode %d rot %d: %d entries", tx, ty, mode, rot, nb);
          if (mode == MDC_ORDER_BANDS || mode == MDC_ORDER_IDENTITY) EXPECT(nb == 8 * ((n + 7) / 8), "%d x %d mode %d rot %d: %d slots, not ceil(n/8)", tx, ty, mode, rot, nb / 8);
          // 3. the even split of the rotated bands: XCD k gets [k n / 8, (k+1) n / 8)
          if (mode == MDC_ORDER_BANDS && rot) {
            for (int k = 0; k < 8; k++) {
              const std::vector<int> v = share(order, k, 0, false);
              const int lo = k * n / 8, hi = (k + 1) * n / 8;
              EXPECT((int)v.size() == hi - lo && (v.empty() || (v.front() == lo && v.back() == hi - 1)), "%d x %d even split, XCD %d", tx, ty, k);
            }
          }
          f_even += g_fail - before_f;
          // 4. every group: every tile exactly once, -1 elsewhere; the shares keep the mode's neighbourhood
          std::vector<long long> total(8, 0);
          for (int y = 0; y < 40; y++) {
            before_f = g_fail;
            std::vector<int> hits(n, 0);
            int pads = 0;
            for (int x = 0; x < nb; x++) {
              const int e = mdc::xcd_table_entry(x, y, rot != 0);
              EXPECT(e >= 0 && e < nb, "%d x %d mode %d rot %d: block (%d, %d) reads entry %d of %d", tx, ty, mode, rot, x, y, e, nb);
              if (e < 0 || e >= nb) continue;
              const int t = order[e];
              EXPECT(t >= -1 && t < n, "tile %d of %d", t, n);
              if (t >= 0 && t < n) hits[t]++;
              else pads++;
            }
            bool once = pads == nb - n;
            for (int t = 0; t < n; t++) once = once && hits[t] == 1;
            EXPECT(once, "%d x %d mode %d rot %d group %d: not every tile exactly once", tx, ty, mode, rot, y);
            f_cover += g_fail - before_f;
            before_f = g_fail;
            for (int k = 0; k < 8; k++) {
              const std::vector<int> v = share(order, k, y, rot != 0);
              EXPECT(neighbourhood(v, tx, ty, mode), "%d x %d mode %d rot %d group %d XCD %d: neighbourhood lost", tx, ty, mode, rot, y, k);
              total[k] += (long long)v.size();
            }
            f_neigh += g_fail - before_f;
            // 5. per-XCD totals after G = y + 1 equal groups
            const int G = y + 1;
            const long long mx = *std::max_element(total.begin(), total.end()), mn = *std::min_element(total.begin(), total.end());
            if (rot) {
              before_f = g_fail;
              if (G % 8 == 0) EXPECT(mx == mn, "%d x %d mode %d, %d groups: totals %lld..%lld not equal", tx, ty, mode, G, mn, mx);
              f_equal += g_fail - before_f;
              before_f = g_fail;
              if (mode == MDC_ORDER_BANDS) EXPECT(mx - mn <= G % 8, "%d x %d bands, %d groups: totals %lld..%lld differ by more than %d", tx, ty, G, mn, mx, G % 8);
              f_bands += g_fail - before_f;
            }
            cases++;
          }
        }
  if (!f_even) std::printf("even split of the rotated bands ok\n");
  if (!f_cover) std::printf("every group covers every tile once ok\n");
  if (!f_neigh) std::printf("shares keep the neighbourhood ok\n");
  if (!f_equal) std::printf("equal totals at multiples of 8 groups ok\n");
  if (!f_bands) std::printf("band totals within groups mod 8 ok\n");
  f0 = g_fail;

  // 6. the headline numbers: 5 x 15 in bands of 10 leaves one XCD half idle; rotated, 4096 frames in groups of 96 are even to 0.25 %
  {
    const std::vector<int> off = mdc::tile_order(5, 15, MDC_ORDER_BANDS, false), on = mdc::tile_order(5, 15, MDC_ORDER_BANDS, true);
    EXPECT(off.size() == 80 && on.size() == 80, "5 x 15: 80 entries");
    EXPECT(share(off, 7, 3, false).size() == 5 && share(off, 0, 3, false).size() == 10, "5 x 15 off: 10/.../10/5");
    for (int fpb : {64, 96, 128}) {
      const int G = (4096 + fpb - 1) / fpb;
      std::vector<long long> work(8, 0);
      for (int y = 0; y < G; y++)
        for (int k = 0; k < 8; k++) work[k] += (long long)share(on, k, y, true).size() * std::min(fpb, 4096 - y * fpb);
      const long long mx = *std::max_element(work.begin(), work.end());
      EXPECT(mx * 8 * 400 <= 75ll * 4096 * 401, "5 x 15 rotated, %d frames per group: largest share %lld over the even %lld by more than 0.25 %%", fpb, mx, 75ll * 4096 / 8);
    }
  }
  done("headline shares");
  std::printf("%lld (grid, mode, rotation, group count) cases, %d failures\n", cases, g_fail);
  return g_fail ? 1 : 0;
}
