// A stand-alone host program over revisit-bpr_amd/csrc/bpr_item_filter.h: tests/test_item_filter_cpu.py compiles it
// with the host compiler under -fsanitize=address,undefined and runs it.  The words of every case lie in a heap block
// of exactly filter_words(I) words, so a read past the filter is a sanitizer report.
//
// Without arguments: a sweep of its own — every function of the header against a loop over the items, for the sizes
// around a tile and a word and a few bit patterns.  Prints "<cases> cases, <n> failures".
// With "-": cases from standard input, one a line, "I w0 w1 ..." (hex words, exactly filter_words(I) of them); for
// each it prints four lines that the Python test holds against its numpy restatement:
//   has    one 0/1 per id -1 .. 32 * words (ids outside 1 .. I - 1 among them)
//   empty  one 0/1 per tile
//   next   filter_next_tile(t, t1) for every 0 <= t <= t1 <= tiles, t1 ascending, t ascending inside
//   at     word:bit of the ids 0, 1, 31, 32, 33, 127, 128, I - 1
// Exit status 0: all held.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "bpr_item_filter.h"

using namespace bpr;

static int failures = 0;
#define CHECK(c)                                                    \
  do {                                                              \
    if (!(c)) {                                                     \
      printf("FAILED line %d: %s\n", __LINE__, #c);                 \
      ++failures;                                                   \
    }                                                               \
  } while (0)

// a heap block of exactly n words, 16-byte aligned
struct Words {
  uint32_t* p;
  explicit Words(int64_t n) : p(static_cast<uint32_t*>(aligned_alloc(FILTER_ALIGN, (size_t)n * 4))) {}
  ~Words() { free(p); }
};

static void sweep_one(int64_t I, int pattern) {
  const int64_t nw = filter_words(I), tiles = nw / FILTER_TILE_WORDS;
  Words w(nw);
  for (int64_t j = 0; j < nw; ++j) {
    uint32_t v = 0;
    switch (pattern) {
      case 0: v = 0u; break;
      case 1: v = 0xFFFFFFFFu; break;                                  // tail bits and item 0's set on purpose
      case 2: v = 0x55555555u; break;
      case 3: v = (uint32_t)(2654435761u * (uint32_t)(j + 1)); break;  // (a hash: any bits)
      case 4: v = j / FILTER_TILE_WORDS == 0 ? 0u : 0xFFFFFFFFu; break;          // first tile empty
      case 5: v = j / FILTER_TILE_WORDS == tiles - 1 ? 0u : 0xFFFFFFFFu; break;  // last tile empty
      case 6: v = j / FILTER_TILE_WORDS == tiles / 2 ? 0u : 0xFFFFFFFFu; break;  // a middle tile empty
      case 7: v = j == 0 ? 1u : 0u; break;                                        // only item 0's bit
    }
    w.p[j] = v;
  }
  if (pattern == 8) {  // ONLY bits at or past I
    for (int64_t j = 0; j < nw; ++j) w.p[j] = 0u;
    for (int64_t i = I; i < 32 * nw; ++i) w.p[i >> 5] |= 1u << (i & 31);
  }
  CHECK(nw % FILTER_TILE_WORDS == 0 && tiles * TOPK_TI >= I && (tiles - 1) * TOPK_TI < I);
  // the restatement: a loop over the items
  std::vector<char> ok((size_t)(32 * nw), 0);
  for (int64_t i = 1; i < I; ++i) ok[(size_t)i] = (w.p[i / 32] >> (i % 32)) & 1u;
  for (int64_t i = -2; i < 32 * nw + 2; ++i) {
    const bool want = i >= 1 && i < I && ok[(size_t)i];
    CHECK(filter_has(w.p, I, i) == want);
    if (i >= 0) CHECK(filter_word_of(i) == i / 32 && filter_bit_of(i) == (int)(i % 32));
  }
  std::vector<char> empty((size_t)tiles, 1);
  for (int64_t i = 1; i < I; ++i)
    if (ok[(size_t)i]) empty[(size_t)(i / TOPK_TI)] = 0;
  for (int64_t t = 0; t < tiles; ++t) {
    CHECK(filter_tile_empty(w.p, I, t) == (bool)empty[(size_t)t]);
    for (int ww = 0; ww < FILTER_TILE_WORDS; ++ww) {
      const uint32_t word = filter_wave_word(w.p, I, t, ww);
      for (int b = 0; b < 32; ++b) CHECK(((word >> b) & 1u) == (uint32_t)ok[(size_t)(TOPK_TI * t + 32 * ww + b)]);
    }
  }
  for (int64_t t1 = 0; t1 <= tiles; ++t1)
    for (int64_t t = 0; t <= t1; ++t) {
      int64_t want = t;
      while (want < t1 && empty[(size_t)want]) ++want;
      CHECK(filter_next_tile(w.p, I, t, t1) == want);
    }
}

static int from_stdin() {
  static char line[1 << 16];
  while (fgets(line, sizeof line, stdin)) {
    char* at = line;
    const int64_t I = strtoll(at, &at, 10);
    if (I < 1) continue;
    const int64_t nw = filter_words(I), tiles = nw / FILTER_TILE_WORDS;
    Words w(nw);
    for (int64_t j = 0; j < nw; ++j) w.p[j] = (uint32_t)strtoul(at, &at, 16);
    printf("has ");
    for (int64_t i = -1; i <= 32 * nw; ++i) putchar(filter_has(w.p, I, i) ? '1' : '0');
    printf("\nempty ");
    for (int64_t t = 0; t < tiles; ++t) putchar(filter_tile_empty(w.p, I, t) ? '1' : '0');
    printf("\nnext");
    for (int64_t t1 = 0; t1 <= tiles; ++t1)
      for (int64_t t = 0; t <= t1; ++t) printf(" %lld", (long long)filter_next_tile(w.p, I, t, t1));
    printf("\nat");
    const int64_t ids[] = {0, 1, 31, 32, 33, 127, 128, I - 1};
    for (int64_t i : ids) printf(" %lld:%d", (long long)filter_word_of(i), filter_bit_of(i));
    printf("\n");
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && strcmp(argv[1], "-") == 0) return from_stdin();
  const int64_t Is[] = {1, 2, 31, 32, 33, 127, 128, 129, 255, 256, 257, 300, 384, 385, 4096, 4097, 20109};
  long cases = 0;
  for (int64_t I : Is)
    for (int pattern = 0; pattern <= 8; ++pattern) {
      sweep_one(I, pattern);
      ++cases;
    }
  static_assert(FILTER_TILE_WORDS * 32 == TOPK_TI, "a tile's words cover the tile");
  CHECK(filter_words(1) == 4 && filter_words(128) == 4 && filter_words(129) == 8 && filter_words(4097) == 132);
  CHECK(filter_words(((int64_t)1 << 31) - 1) == (int64_t)1 << 26);
  printf("%ld cases, %d failures\n", cases, failures);
  return failures != 0;
}
