// Which XCD runs which output tile: the host-made placement table of the remap kernels (TilePlan::d_order, StripPlan::d_order) and the
// entry of it that block (x, y) of a launch reads, in a header both compilers take.  tests/native/xcd_placement_cpu.cpp
// (tests/test_xcd_placement_cpu.py) pins it on the CPU over every small tile grid.
//
// The dispatcher deals the blocks of a grid round-robin over the 8 XCDs in launch order; the table has a multiple of 8 entries
// (gridDim.x % 8 == 0), so block (x, y) runs on XCD x % 8 whatever its frame group y is, and XCD k runs the tiles of entries
// k, k+8, k+16, ...  Neighbouring tiles share source lines (halo rows, 128-byte lines straddling a tile border); they should meet in
// ONE XCD's L2.
//   MDC_ORDER_BANDS     row-major runs of tiles per XCD
//   MDC_ORDER_ROWS      whole tile rows per XCD, as even as the row count allows (no horizontal neighbours split)
//   MDC_ORDER_IDENTITY  entry b = tile b: neighbours land on different XCDs (diagnosis: worst case)
//   MDC_ORDER_BLOCKS2D  the tile grid cut into 8 rectangles by recursive bisection of the longer side (least shared halo
//                       perimeter between XCDs; the rectangles differ in size by up to one row / column)
// An XCD with fewer tiles than the largest share gets padding entries (-1): its blocks exit at once and the XCD idles while the
// others finish the frame group.  Without rotation every frame group hands the same XCD the same share, so the idle time adds up
// over the launch (75 tiles in bands of 10: 10/.../10/5).  With rotation (MDC_OPT_XCD_ROTATE) the blocks of XCD k read the
// entries of column (k + y) % 8 in frame group y: every XCD takes every share in turn, one share per group (its tiles still
// neighbours in one L2), and over 8 groups every XCD has run every tile once.
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>

#include "mdc_hip.h"

#if defined(__HIPCC__)
#define MDC_XCD_HD __host__ __device__ __forceinline__
#else
#define MDC_XCD_HD inline
#endif

namespace mdc {

constexpr int kXcds = 8;

// Entry of the placement table read by block x of frame group y.  x & ~7 is the block's slot (the table's row of 8), the low
// three bits its column; rotation shifts the column by the group index.  A permutation of every row for every y, so each group
// still covers every entry exactly once.
MDC_XCD_HD int xcd_table_entry(int x, int y, bool rotate) { return rotate ? ((x & ~(kXcds - 1)) | ((x + y) & (kXcds - 1))) : x; }

inline void xcd_bisect(int x0, int y0, int x1, int y1, int parts, int tx, std::vector<std::vector<int>>& out) {
  if (parts == 1) {
    std::vector<int> v;
    for (int y = y0; y < y1; y++)
      for (int x = x0; x < x1; x++) v.push_back(y * tx + x);
    out.push_back(v);
    return;
  }
  if (x1 - x0 > y1 - y0) {
    const int xm = x0 + (x1 - x0 + 1) / 2;
    xcd_bisect(x0, y0, xm, y1, parts / 2, tx, out);
    xcd_bisect(xm, y0, x1, y1, parts / 2, tx, out);
  } else {
    const int ym = y0 + (y1 - y0 + 1) / 2;
    xcd_bisect(x0, y0, x1, ym, parts / 2, tx, out);
    xcd_bisect(x0, ym, x1, y1, parts / 2, tx, out);
  }
}

// Placement table of a tx x ty tile grid: entry b = tile (row-major index) or -1, a multiple of 8 entries, column k = the share
// of one XCD.  rotate = false: the bands are runs of ceil(n/8) tiles, the last XCDs get what is left (or nothing).
// rotate = true: the bands are an even split, XCD k gets tiles [k n/8, (k+1) n/8) -- sizes differ by at most one, the
// slot count stays ceil(n/8); the other modes are the same table either way.
inline std::vector<int> tile_order(int tx, int ty, int mode, bool rotate = false) {
  const int n = tx * ty;
  std::vector<std::vector<int>> per_xcd(kXcds);
  if (mode == MDC_ORDER_BLOCKS2D && n >= kXcds) {
    per_xcd.clear();
    xcd_bisect(0, 0, tx, ty, kXcds, tx, per_xcd);
  } else if (mode == MDC_ORDER_IDENTITY) {
    for (int t = 0; t < n; t++) per_xcd[t % kXcds].push_back(t);
  } else if (mode == MDC_ORDER_ROWS && ty >= kXcds) {
    int r = 0;
    for (int k = 0; k < kXcds; k++) {
      const int rows = ty / kXcds + (k < ty % kXcds ? 1 : 0);
      for (int y = r; y < r + rows; y++)
        for (int x = 0; x < tx; x++) per_xcd[k].push_back(y * tx + x);
      r += rows;
    }
  } else if (rotate) {
    for (int k = 0; k < kXcds; k++)
      for (int t = (int)((long long)k * n / kXcds); t < (int)((long long)(k + 1) * n / kXcds); t++) per_xcd[k].push_back(t);
  } else {
    const int per = (n + kXcds - 1) / kXcds;
    for (int t = 0; t < n; t++) per_xcd[t / per].push_back(t);
  }
  size_t slots = 0;
  for (const auto& v : per_xcd) slots = std::max(slots, v.size());
  std::vector<int> order(slots * kXcds, -1);
  for (int k = 0; k < kXcds; k++)
    for (size_t j = 0; j < per_xcd[k].size(); j++) order[j * kXcds + k] = per_xcd[k][j];
  return order;
}

}  // namespace mdc
