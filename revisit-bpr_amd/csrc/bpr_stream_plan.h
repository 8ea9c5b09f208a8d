// bpr_stream_plan.h — how a STREAM launch (k_stream, bpr_stream.h) is laid out: which kernel, which "seen?"
// structure, block, grid, dynamic LDS, run length and — for the LDS tier — rows and tail zones.  Integer arithmetic
// on the shape and the tuning knobs only: no HIP, no bpr_ctx (plain C++17; tests/test_stream_plan_cpu.py pins it
// on the CPU).  launch_stream (bpr_stream_launch.hip) fills a StreamShape, supplies the occupancy between the two steps and
// launches what the StreamPlan says.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/bprcore.h"
#include "bpr_scored_plan.h"

namespace bpr {

constexpr int64_t STREAM_MAX_GRID = 65536;  // also the size of the per-block partials scratch
constexpr int LIST_CAP = 512;               // entries of a group's staged seen list (heavier users search the CSR in HBM)

// Dynamic LDS a workgroup of the LDS-tier kernel may declare at width d: the CU's 160 KiB less the kernel's static
// LDS (sigma: 4 d bytes rounded to the group layout, the loss reduction's 256 B, the ticket) and 256 B of slack.
inline size_t lds_tier_room(int d) { return 160 * 1024 - ((size_t)4 * (size_t)((d + 63) / 64 * 64) + 256 + 16 + 256); }

enum StreamSeen { STREAM_SEEN_CSR = 0, STREAM_SEEN_BITMAP = 1, STREAM_SEEN_LIST = 2 };  // == SEEN_* (bpr_device.h)
enum SeenForce { SEEN_BY_SHAPE = 0, FORCE_CSR = 1, FORCE_BITMAP = 2, FORCE_LIST = 3 };  // == bpr_set_tuning("seen")
enum StreamKernel { STREAM_PLAIN = 0, STREAM_LDS = 1 };                                 // k_stream<..., LDSHOT = false | true>

struct StreamShape {
  int64_t n, I;          // triples of the launch, item rows
  int d, G, E;
  int sampler;           // bpr_sampler_kind
  int64_t cap_groups;    // max_inflight (0: no cap)
  int run_len;           // bpr_set_stream_opts (0: by launch size)
  int force_seen;        // SeenForce
  int cus;               // CUs of the launch stream
  int64_t grid_cap;      // blocks of 256 threads a grid may have (BPR_MAX_BLOCKS, else STREAM_MAX_GRID)
  bool hot;              // a hot block is bound ...
  int hot_H;             // ... of this many rows
  int tune_hot_lds;      // bpr_set_hot_lds: LDS rows asked for (0: no LDS tier) ...
  bool tune_hot_lds_force;  // ... also for launches that do not fill the chip
  int tune_lds_block;    // bpr_set_tuning "lds_block" (0: by shape)
  int tune_lds_tail;     // bpr_set_tuning "lds_tail": percent of the triples dealt in short runs
  bool lds_allowed;      // the ctx's state admits the LDS tier (launch_stream)
};

struct StreamPlan {
  int kernel;            // StreamKernel
  int seen;              // StreamSeen
  unsigned block, grid;
  size_t shmem;          // dynamic LDS bytes
  int bm_words;          // words of a group's seen structure (StreamArgs::bm_words)
  int gpw_active;        // groups of a wave that work
  int run_len;
  int L;                 // LDS tier: delta rows in LDS (0: the plain kernel)
  int32_t tail1, tail2;  // LDS tier: first triple of the zones of runs of run_len / 2 and run_len / 4
};

// words of one group's seen bitmap (I bits; a multiple of 4: 16-byte LDS wipes)
inline int seen_words(int64_t I) { return (int)(((I + 31) / 32 + 3) / 4 * 4); }

// Step one — what the occupancy query needs: the plain kernel's block, "seen?" structure and dynamic LDS.
// A cap below one 256-thread block shrinks the block (whole waves), so max_inflight = 1 at G = 64 really is ONE
// wave walking the stream sequentially.
// "seen?" answers (bpr_device.h): the LDS bitmap (I bits per group) while a full 256-thread block's bitmaps fit
// 64 KiB (>= 2 blocks per CU at full width: I <= 65,536 for d <= 128, 131,072 above); larger item tables stage the
// user's sorted seen list in LDS instead (LIST_CAP entries per group).  bpr_set_tuning("seen", ...) forces a
// structure (tests, measurements); a forced bitmap shrinks the block to fit.
inline StreamPlan plan_stream_block(const StreamShape& s) {
  StreamPlan p = {};
  const int G = s.G;
  p.kernel = STREAM_PLAIN;
  p.block = 256;
  p.gpw_active = 64 / G;
  if (s.cap_groups > 0 && s.cap_groups * G < 256) {
    p.block = (unsigned)(((s.cap_groups * G + 63) / 64) * 64);
    if (s.cap_groups < 64 / G) p.gpw_active = (int)s.cap_groups;  // one wave, one group at work
  }
  const int words = seen_words(s.I);
  p.seen = STREAM_SEEN_CSR;
  if (s.sampler != BPR_NEG_GIVEN && s.force_seen != FORCE_CSR) {
    auto bm_bytes = [&] { return (size_t)(p.block / G) * words * sizeof(uint32_t); };
    if (s.force_seen == FORCE_LIST || (s.force_seen != FORCE_BITMAP && bm_bytes() > 64 * 1024)) {
      p.seen = STREAM_SEEN_LIST;
    } else {
      while (p.block > 64 && bm_bytes() > 64 * 1024) p.block /= 2;
      if (bm_bytes() <= 64 * 1024) {
        p.seen = STREAM_SEEN_BITMAP;
      } else {
        p.block = 256;
        p.seen = STREAM_SEEN_LIST;
      }
    }
  }
  p.bm_words = p.seen == STREAM_SEEN_BITMAP ? words : p.seen == STREAM_SEEN_LIST ? LIST_CAP : 0;
  p.shmem = (size_t)(p.block / G) * (size_t)p.bm_words * sizeof(uint32_t);
  return p;
}

// The LDS tier of the hot block (k_stream LDSHOT, bpr_hotlds.hip; bpr_set_hot_lds = rows asked for): ONE workgroup
// per CU — up to 1,024 threads, its groups' seen structures and an [L, d] fp32 delta block in LDS — persistent over
// its share of the runs.  Taken when the launch fills the chip at least twice (a smaller one is over when its slowest
// group is: the plain kernel's short runs win there) and the seen structures leave room for >= 8 rows.
// Overwrites p and returns true if taken.
inline bool plan_stream_lds(const StreamShape& s, StreamPlan& p) {
  if (!(s.tune_hot_lds > 0 && s.hot && s.lds_allowed && (s.sampler == BPR_NEG_GIVEN || s.force_seen != FORCE_CSR)))
    return false;
  // dynamic negatives score their candidates on the LIVE rows, WARP compares them with the positive there: a hot row
  // behind this workgroup's LDS delta is not one (and k_stream has no LDSHOT instantiation of those samplers)
  if (sampler_scored(s.sampler)) return false;
  const int G = s.G;
  unsigned block = s.E <= 4 ? 1024 : 512;  // (E >= 8: 64+ registers of rows per lane — two waves per SIMD)
  if (s.tune_lds_block > 0) block = std::min<unsigned>(block, (unsigned)s.tune_lds_block);
  if (s.cap_groups > 0 && s.cap_groups * G < block) block = (unsigned)(((s.cap_groups * G + 63) / 64) * 64);
  // the groups' seen structure beside the rows: the I-bit bitmaps while they leave 32 KB for rows, else (or forced)
  // the staged sorted lists (item tables past ~60 k items)
  const int words = seen_words(s.I);
  const size_t room = lds_tier_room(s.d);
  int seen = STREAM_SEEN_BITMAP;
  size_t bm_bytes = s.sampler == BPR_NEG_GIVEN ? 0 : (size_t)(block / G) * words * sizeof(uint32_t);
  if (s.sampler != BPR_NEG_GIVEN &&
      (s.force_seen == FORCE_LIST || (s.force_seen != FORCE_BITMAP && bm_bytes + 32 * 1024 > room))) {
    seen = STREAM_SEEN_LIST;
    bm_bytes = (size_t)(block / G) * LIST_CAP * sizeof(uint32_t);
  }
  const size_t row_bytes = sizeof(float) * (size_t)s.d + sizeof(uint32_t);
  int64_t L = bm_bytes < room ? (int64_t)((room - bm_bytes) / row_bytes) : 0;
  L = std::min<int64_t>(L, std::min<int64_t>(s.tune_hot_lds, s.hot_H));
  const int64_t per_block = (int64_t)(block / 64) * p.gpw_active;
  const bool fills = (s.n + 7) / 8 >= 2 * (int64_t)s.cus * per_block;
  if (L < 8 || !(fills || s.tune_hot_lds_force)) return false;
  p.kernel = STREAM_LDS;
  p.seen = s.sampler == BPR_NEG_GIVEN ? STREAM_SEEN_CSR : seen;
  p.block = block;
  p.run_len = s.run_len > 0 ? s.run_len : 8;  // (not the plain kernel's pick)
  // the last tickets of a persistent workgroup are short runs (k_stream: tail1 / tail2), whole wave-loads each
  // (zones hold whole wave-loads of runs: what is left of the chunk past the last whole wave-load of full runs
  // always goes in the shortest runs).  tests/hotlds_model.py::zones restates this.
  const int64_t len2 = std::max(1, p.run_len / 2), len3 = std::max(1, p.run_len / 4);
  const int64_t wl = (int64_t)p.run_len * p.gpw_active;  // triples of a wave-load of full runs
  int64_t t1 = (int64_t)((double)s.n * (1.0 - s.tune_lds_tail / 100.0)) / wl * wl;
  int64_t t2 = t1 + (int64_t)((double)(s.n - t1) * 0.6) / (len2 * p.gpw_active) * (len2 * p.gpw_active);
  if (s.tune_lds_tail <= 0) t1 = t2 = s.n / wl * wl;
  p.tail1 = (int32_t)t1;
  p.tail2 = (int32_t)t2;
  int64_t want = t1 / p.run_len + (t2 - t1) / len2 + (s.n - t2 + len3 - 1) / len3;
  if (s.cap_groups > 0 && want > s.cap_groups) want = s.cap_groups;
  p.grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(s.cus, (want + per_block - 1) / per_block));
  p.bm_words = s.sampler == BPR_NEG_GIVEN ? 0 : (seen == STREAM_SEEN_LIST ? LIST_CAP : words);
  p.L = (int)L;
  p.shmem = bm_bytes + (size_t)L * row_bytes;
  return true;
}

// Step two — the rest, given p = plan_stream_block(s) and occ = blocks of that kernel a CU holds at once.
// run_len 0 = by launch size.  A launch whose runs of 8 overfill the chip takes runs of 8 and a grid of ~1.5 runs
// per group (the hardware dispatcher balances the rest; measured: ML-20M 2,075 blocks 0.233 ms vs 0.24-0.25 for 1
// or >= 2 runs per group; Yelp 10,922 blocks 1.22 ms vs 1.31 ms with a persistent 2,048-block grid).  A smaller
// launch (Netflix-sized periods, a rank's share of a period at 8 ranks) is over when its slowest group is: the
// shortest runs of >= 4 triples that still fit the chip in ONE residency, one run per group
// (profiles/r03_sweep_small.txt: 40,704 triples d=64 0.0433 -> 0.0393 ms, 24,896 triples d=128 0.0550 -> 0.0413 ms;
// runs shorter than 4 re-load the user row too often).
inline StreamPlan plan_stream(const StreamShape& s, StreamPlan p, int occ) {
  if (plan_stream_lds(s, p)) return p;
  const int64_t per_block = (int64_t)(p.block / 64) * p.gpw_active;
  // groups the launch stream's CUs hold at once (occupancy of THIS instantiation x its CUs)
  const int64_t resident = (int64_t)occ * s.cus * per_block;
  p.run_len = s.run_len;
  if (p.run_len <= 0) {
    p.run_len = 8;
    // (max_inflight > 0 — what StreamTrainer passes — only changes this when the cap binds: the residency bound
    // is min(chip, cap))
    const int64_t room = s.cap_groups > 0 ? std::min<int64_t>(resident, s.cap_groups) : resident;
    if ((s.n + 7) / 8 < room) {
      p.run_len = 4;
      while (p.run_len < 8 && (s.n + p.run_len - 1) / p.run_len > room) ++p.run_len;
    }
  }
  const int64_t n_runs = (s.n + p.run_len - 1) / p.run_len;
  int64_t want = n_runs;
  if (s.cap_groups > 0 && want > s.cap_groups) want = s.cap_groups;
  int64_t nblk = (want + per_block - 1) / per_block;
  if ((s.cap_groups <= 0 || n_runs <= s.cap_groups) && n_runs > resident) nblk = (2 * nblk + 2) / 3;  // 1.5 runs per group
  const int64_t max_blk = std::min<int64_t>(s.grid_cap * (256 / p.block), STREAM_MAX_GRID);
  if (nblk > max_blk) nblk = max_blk;
  p.grid = (unsigned)(nblk < 1 ? 1 : nblk);
  return p;
}

}  // namespace bpr
