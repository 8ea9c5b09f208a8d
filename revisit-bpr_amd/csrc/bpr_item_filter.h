// bpr_item_filter.h — the item filter of the whole-catalogue serving kernels (k_topk, bpr_topk.hip; k_retrieve,
// bpr_retrieve.hip; k_sample, bpr_sample.hip; k_rank, bpr_rank.hip; k_neighbors, bpr_neighbors.hip), stated once: the layout, the word and bit of an item, "tile t is
// empty" and "the next non-empty tile of [t, t1)".  Plain C++17 on host and device (no HIP type, no intrinsic), so
// that a host program can pin it (tests/item_filter_plan_check.cpp, tests/rank_neighbors_filter_plan_check.cpp, and
// `bpr_test_filter_tiles` / `bpr_test_filter_words_from` for Python).
//
// Layout.  A filter over I items is a bitmap of uint32 words: bit `i & 31` of word `i >> 5` set means item i is
// eligible.  It is 4 * ceil(I / TOPK_TI) words long — a whole number of item tiles, a tile's FILTER_TILE_WORDS = 4
// words being one aligned 16-byte run — its start is 16-byte aligned, and bits at or past I are zero (the packer's
// duty: revisit_bpr/item_filter.py).  Item 0 is never eligible whatever its bit says; a filter over a table whose
// row 0 is a row (k_neighbors with first = 0) goes through the `_from` functions, whose lower bound is a parameter.
//
// One word per wave and tile.  After an item tile the 16 scores a lane holds of each of its two users are items
// 128 t + 32 w + 4 h + (q & 3) + 8 (q >> 2): all inside the aligned run 128 t + 32 w .. + 31 of wave w.  So a wave
// needs ONE word per tile, word 4 t + w, and the item's bit in it is the item's offset in the run.
//
// What the header never does is read a bit at or past I, or item 0's, as an item: filter_word clears them, and every
// function here goes through it.  A filter whose tail bits are set by mistake therefore ranks what a clean one ranks.
// A tile is empty when its four words, so cleared, are zero: a kernel that skips it loses nothing, because a walked
// tile without an eligible item counts nothing, appends nothing and adds (-inf, 0) to log_z's running (max, sum).
#pragma once
#include <stdint.h>

#include <type_traits>

#include "bpr_topk_plan.h"

#if defined(__HIPCC__)
#define BPR_FILTER_FN __host__ __device__ inline
#else
#define BPR_FILTER_FN inline
#endif

namespace bpr {

constexpr int FILTER_TILE_WORDS = TOPK_TI / 32;  // words of an item tile: one per wave
constexpr int FILTER_ALIGN = 16;                 // bytes: a tile's words are one aligned 16-byte run

static_assert(FILTER_TILE_WORDS == 4, "a wave of a tile covers one aligned run of 32 items");

// words of a filter over I items: whole tiles
BPR_FILTER_FN int64_t filter_words(int64_t I) { return FILTER_TILE_WORDS * ((I + TOPK_TI - 1) / TOPK_TI); }

// the word and the bit of item i
BPR_FILTER_FN int64_t filter_word_of(int64_t i) { return i >> 5; }
BPR_FILTER_FN int filter_bit_of(int64_t i) { return (int)(i & 31); }

// word wi of the filter with a lower bound that is a parameter: items 32 wi .. + 31, with the ids below `first` and
// the ids at or past N cleared.  The item tables have first = 1 (item 0 is the padding item); a table whose row 0 is
// a row like any other (k_neighbors over the user table, first = 0) keeps it.  wi < filter_words(N), first >= 0.
BPR_FILTER_FN uint32_t filter_word_from(const uint32_t* words, int64_t N, int64_t wi, int64_t first) {
  uint32_t v = words[wi];
  if (first == 1) {  // (the item tables' case in the words it had before there was a parameter: the same code)
    if (wi == 0) v &= ~1u;
  } else {
    const int64_t below = first - 32 * wi;  // ids of the word that are below first
    if (below > 0) v &= below >= 32 ? 0u : ~((1u << below) - 1u);
  }
  const int64_t left = N - 32 * wi;  // ids of the word that are below N
  if (left < 32) v &= left <= 0 ? 0u : (1u << left) - 1u;
  return v;
}

// the word of wave w of tile t, the tile test and the scan, with that lower bound
BPR_FILTER_FN uint32_t filter_wave_word_from(const uint32_t* words, int64_t N, int64_t t, int w, int64_t first) {
  return filter_word_from(words, N, FILTER_TILE_WORDS * t + w, first);
}

BPR_FILTER_FN bool filter_has_from(const uint32_t* words, int64_t N, int64_t i, int64_t first) {
  if (i < first || i < 0 || i >= N) return false;
  return (filter_word_from(words, N, filter_word_of(i), first) >> filter_bit_of(i)) & 1u;
}

BPR_FILTER_FN bool filter_tile_empty_from(const uint32_t* words, int64_t N, int64_t t, int64_t first) {
  uint32_t any = 0;
  for (int w = 0; w < FILTER_TILE_WORDS; ++w) any |= filter_wave_word_from(words, N, t, w, first);
  return any == 0;
}

BPR_FILTER_FN int64_t filter_next_tile_from(const uint32_t* words, int64_t N, int64_t t, int64_t t1, int64_t first) {
  while (t < t1 && filter_tile_empty_from(words, N, t, first)) ++t;
  return t < t1 ? t : t1;
}

// ---- the item tables: first = 1.
// word wi of the filter as the kernels read it: items 32 wi .. + 31, with item 0 and the items at or past I cleared.
// wi < filter_words(I).
BPR_FILTER_FN uint32_t filter_word(const uint32_t* words, int64_t I, int64_t wi) {
  return filter_word_from(words, I, wi, 1);
}

// the word of wave w of item tile t
BPR_FILTER_FN uint32_t filter_wave_word(const uint32_t* words, int64_t I, int64_t t, int w) {
  return filter_word(words, I, FILTER_TILE_WORDS * t + w);
}

// is item i eligible?  (any i: outside 1 .. I - 1 never)
BPR_FILTER_FN bool filter_has(const uint32_t* words, int64_t I, int64_t i) { return filter_has_from(words, I, i, 1); }

// tile t (items TOPK_TI t .. + TOPK_TI - 1) holds no eligible item.  t < ceil(I / TOPK_TI).
BPR_FILTER_FN bool filter_tile_empty(const uint32_t* words, int64_t I, int64_t t) {
  return filter_tile_empty_from(words, I, t, 1);
}

// the first tile of [t, t1) that is not empty, or t1.  t1 <= ceil(I / TOPK_TI).
BPR_FILTER_FN int64_t filter_next_tile(const uint32_t* words, int64_t I, int64_t t, int64_t t1) {
  return filter_next_tile_from(words, I, t, t1, 1);
}

// ---- a kernel's arguments with a filter behind them.  The FILT = false instantiation of a kernel takes its
// argument struct as it was, so that its kernarg segment, and with it its code, is what it was without the feature.
template <typename Args>
struct Filtered : Args {
  const uint32_t* filter;  // [filter_words(I)]
};
template <bool FILT, typename Args>
using MaybeFiltered = std::conditional_t<FILT, Filtered<Args>, Args>;

}  // namespace bpr
