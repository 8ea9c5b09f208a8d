// bpr_refresh_plan.h — which sorter a snapshot refresh (refresh_impl, bpr_refresh.hip) runs over its columns: the
// route, the workgroups per column, the template instantiation of every kernel on the way and the fallback of a
// column the binned sort gives up on.  Integer rules on the shape and the tuning knobs only: no HIP, no ctx
// (plain C++17; tests/test_refresh_plan_cpu.py pins it on the CPU through `bpr_test_refresh_plan`).
#pragma once
#include <stdint.h>

namespace bpr {

// what bpr_adaptive_refresh_info reports as the route
enum RefreshRoute {
  REFRESH_RADIX = 0,         // k_sort_sub: the in-LDS radix sort, sub workgroups per column + k_merge_runs when sub > 1
  REFRESH_BINNED = 1,        // k_sort_binned: one workgroup per column; k_sort_flagged behind it
  REFRESH_BINNED_SPLIT = 2,  // k_sort_binned_split (past 65,535 items its 17-bit-id form): G workgroups per column
  REFRESH_PARTIAL = 3,       // k_sort_partial: exact ends + bucketed middle; k_sort_flagged behind it
  REFRESH_DEVICE = 4,        // rocPRIM's device-wide radix sort over all columns at once
};
// who redoes a column the split binned sort flagged
enum RefreshFallback {
  REFRESH_FB_NONE = 0,
  REFRESH_FB_FLAGGED = 1,  // k_sort_flagged: the column fits one workgroup (I <= 36,864)
  REFRESH_FB_RADIX = 2,    // k_sort_sub over the flagged columns + k_merge_runs (sub = 2 | 4)
};

constexpr int64_t REFRESH_WG_MAX = 1024 * 36;       // keys one workgroup of the radix sort holds
constexpr int64_t REFRESH_BINNED_ONE_MAX = 1024 * 20;  // ... and one workgroup of the binned sort
constexpr int64_t REFRESH_ID16_MAX = 65535;         // 16-bit ids: k_sort_binned_split, k_sort_partial
constexpr int64_t REFRESH_ID17_MAX = 131071;        // 17-bit ids: the WIDE k_sort_binned_split
// the largest column the split binned sort takes by itself (binned_split = 0).  Past 65,535 items it is held to
// what was measured against radix + merge (profiles/binned_wide_sort.txt); a forced binned_split
// reaches the kernel up to REFRESH_ID17_MAX either way
constexpr int64_t REFRESH_BINNED_AUTO_MAX = 65535;

struct RefreshShape {
  int64_t I;
  int nf;                  // columns this call sorts (d, or this rank's share)
  bool split, part;        // _begin's side-stream sort; bpr_adaptive_refresh_part
  int tune_binned;         // bpr_set_tuning("binned_sort")
  int tune_binned_split;   // ... ("binned_split"): 0 by shape, else the workgroups per column asked for
  int tune_refresh_sub;    // ... ("refresh_sub"): 0 by shape, 1 | 2 | 4 forced
  int tune_partial;        // ... ("partial_snapshot")
  bool no_fast;            // BPR_NO_FAST_REFRESH is set
};

struct RefreshPlan {
  int route;      // RefreshRoute
  int sub;        // workgroups per column of the radix sort (the route's, or the fallback's)
  int64_t len;    // keys per radix workgroup, a multiple of 16
  int g;          // workgroups per column of the binned sort (0: not binned, 1: k_sort_binned)
  int sitems;     // SITEMS of k_sort_binned_split (g > 1)
  int items;      // ITEMS of the route's own kernel: k_sort_sub / k_sort_binned / k_sort_partial (0: none)
  int fallback;   // RefreshFallback (g > 1)
  int fb_items;   // ITEMS of the fallback's kernel
  bool wide;      // 17-bit ids
  bool partial;
};

inline int refresh_pick(int items, const int* steps, int n) {  // the smallest instantiation that holds `items`
  for (int k = 0; k < n - 1; ++k)
    if (items <= steps[k]) return steps[k];
  return steps[n - 1];
}

inline RefreshPlan plan_refresh(const RefreshShape& s) {
  RefreshPlan p = {};
  const int64_t I = s.I;
  const int force_sub = s.tune_refresh_sub;
  // One 1024-thread workgroup sorts a (sub-)column of <= 36 keys per thread in LDS.  Columns are
  // split over 2 or 4 workgroups — sorted runs merged pairwise by k_merge_runs — when they do not
  // fit, or when d workgroups would leave CUs idle and the pieces stay >= 5,000 keys (measured on
  // ML-20M, refresh + launch gaps per step: d=128 0.106 -> 0.095 ms with 2, d=64 0.100 -> 0.079 ms
  // with 4; d=256 and Netflix's 4.8 k-item columns are fastest unsplit).  A split refresh shares
  // the chip with the caller's kernels: it keeps the columns whole (fewer, longer workgroups and
  // no merge pass) whenever they fit.
  int sub = 1;
  while (sub < 4 && (I + sub - 1) / sub > REFRESH_WG_MAX) sub *= 2;
  if (!s.split)
    while (sub < 4 && s.nf * sub < 256 && I / (2 * sub) >= 5000) sub *= 2;
  if (force_sub == 1 || force_sub == 2 || force_sub == 4) sub = force_sub;
  // BINNED sort (r5): a column of <= 20,480 keys is ordered exactly by one workgroup in about a third of the radix
  // sort's time (k_sort_binned) — whole columns then beat split-and-merge on the idle chip too.  A _begin with
  // partial_snapshot on sorts partially instead — where a partial order exists (16-bit ids)
  const bool wants_partial = s.split && !s.part && s.tune_partial != 0 && I <= REFRESH_ID16_MAX;
  const bool binned_ok = s.tune_binned != 0 && !s.no_fast && force_sub == 0 && I >= 2048 && !wants_partial;
  // ... with G workgroups per column (k_sort_binned_split) when a column does not fit one workgroup's LDS:
  // 16-bit ids up to 65,535 items, 17-bit ids (its WIDE form) up to 131,071
  int g = 0, sitems = 0;
  const int64_t auto_max = s.tune_binned_split > 0 ? REFRESH_ID17_MAX : REFRESH_BINNED_AUTO_MAX;
  if (binned_ok && I <= auto_max) {
    if (s.tune_binned_split > 0) g = s.tune_binned_split;  // (tests, measurements)
    else if (I > REFRESH_BINNED_ONE_MAX) g = (int)((I * 106 / 100 + 20 * 1024 - 1) / (20 * 1024));
    else g = 1;  // (two workgroups per column on the idle chip were measured: 54.6 against 50.7 us per
                 // ML-20M refresh — every workgroup repeats the histogram passes)
    if (g > 1) {
      for (;; ++g) {  // the staged stretch (I / G keys + 6 % + a window) in 8 / 12 / 16 / 20 k entries
        const int64_t need = (I / g) * 106 / 100 + 64;
        sitems = need <= 8 * 1024 ? 8 : need <= 12 * 1024 ? 12 : need <= 16 * 1024 ? 16 : need <= 20 * 1024 ? 20 : 0;
        if (sitems != 0) break;
      }
    } else if (I > REFRESH_BINNED_ONE_MAX) {
      g = 0;  // (forced to one workgroup per column but the column does not fit: the radix sort)
    }
  }
  if (g == 1 || (g > 1 && I <= REFRESH_WG_MAX)) sub = 1;  // (the fallback of a flagged column: k_sort_flagged)
  int64_t len = (I + sub - 1) / sub;
  len = (len + 15) / 16 * 16;
  // PARTIAL order (r5): the split refresh of a column that one workgroup holds — the exact ends + a
  // bucketed middle, ~half the sort's work (k_sort_partial); everybody but k_stream gets the snapshot
  // completed on demand (snapshot_complete_impl)
  p.partial = s.split && !s.part && s.tune_partial != 0 && sub == 1 && len <= 1024 * 24 && I <= REFRESH_ID16_MAX &&
              I >= 2048 && !s.no_fast;
  p.sub = sub;
  p.len = len;
  p.g = g;
  p.sitems = sitems;
  p.wide = g > 1 && I > REFRESH_ID16_MAX;
  const int items = (int)((len + 1023) / 1024);
  static const int radix_steps[] = {6, 10, 12, 16, 20, 24, 28, 36};
  static const int partial_steps[] = {6, 10, 12, 16, 20, 24};
  static const int binned_steps[] = {6, 10, 16, 20};
  static const int flagged_steps[] = {10, 20, 28, 36};
  const bool radix_fits = len <= REFRESH_WG_MAX && !s.no_fast;
  if (p.partial) {
    p.route = REFRESH_PARTIAL;
    p.items = refresh_pick(items, partial_steps, 6);
  } else if (g == 1) {
    p.route = REFRESH_BINNED;
    p.items = refresh_pick(items, binned_steps, 4);
  } else if (g > 1) {
    p.route = REFRESH_BINNED_SPLIT;
    if (sub == 1) {
      p.fallback = REFRESH_FB_FLAGGED;
      p.fb_items = refresh_pick(items, flagged_steps, 4);
    } else if (radix_fits) {
      p.fallback = REFRESH_FB_RADIX;
      p.fb_items = refresh_pick(items, radix_steps, 8);
    }
  } else if (radix_fits) {
    p.route = REFRESH_RADIX;
    p.items = refresh_pick(items, radix_steps, 8);
  } else {
    p.route = REFRESH_DEVICE;
  }
  return p;
}

}  // namespace bpr
