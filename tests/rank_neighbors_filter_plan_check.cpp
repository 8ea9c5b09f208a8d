// A stand-alone host program over the `_from` functions of revisit-bpr_amd/csrc/bpr_item_filter.h (a filter whose
// lower bound is a parameter): tests/test_rank_neighbors_filter_cpu.py compiles it with the host compiler under
// -fsanitize=address,undefined and runs it.  The words of every case lie in a heap block of exactly filter_words(N)
// words, so a read past the filter is a sanitizer report.
//
// Without arguments: a sweep of its own — every `_from` function against a loop over the ids, for every (N, first)
// and a few bit patterns, and the first = 1 case against the functions without the parameter.  Prints
// "<cases> cases, <n> failures".
// With "-": cases from standard input, one a line, "N first w0 w1 ..." (hex words, exactly filter_words(N)); for
// each it prints one line, the words of filter_word_from in hex, that the Python test holds against numpy.
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

static void sweep_one(int64_t N, int64_t first, int pattern) {
  const int64_t nw = filter_words(N), tiles = nw / FILTER_TILE_WORDS;
  Words w(nw);
  for (int64_t j = 0; j < nw; ++j) {
    uint32_t v = 0;
    switch (pattern) {
      case 0: v = 0u; break;
      case 1: v = 0xFFFFFFFFu; break;  // tail bits and the bits below first set on purpose
      case 2: v = 0x55555555u; break;
      case 3: v = (uint32_t)(2654435761u * (uint32_t)(j + 1)); break;  // (a hash: any bits)
      case 4: v = j / FILTER_TILE_WORDS == tiles / 2 ? 0u : 0xFFFFFFFFu; break;  // a middle tile empty
      case 5: v = j == 0 ? 1u : 0u; break;                                        // only row 0's bit
    }
    w.p[j] = v;
  }
  std::vector<char> ok((size_t)(32 * nw), 0);
  for (int64_t i = first; i < N; ++i) ok[(size_t)i] = (w.p[i / 32] >> (i % 32)) & 1u;
  for (int64_t i = -2; i < 32 * nw + 2; ++i) {
    const bool want = i >= first && i >= 0 && i < N && ok[(size_t)i];
    CHECK(filter_has_from(w.p, N, i, first) == want);
    if (first == 1) CHECK(filter_has(w.p, N, i) == want);
  }
  std::vector<char> empty((size_t)tiles, 1);
  for (int64_t i = 0; i < N; ++i)
    if (ok[(size_t)i]) empty[(size_t)(i / TOPK_TI)] = 0;
  for (int64_t wi = 0; wi < nw; ++wi) {
    const uint32_t word = filter_word_from(w.p, N, wi, first);
    for (int b = 0; b < 32; ++b) CHECK(((word >> b) & 1u) == (uint32_t)ok[(size_t)(32 * wi + b)]);
    if (first == 1) CHECK(word == filter_word(w.p, N, wi));
  }
  for (int64_t t = 0; t < tiles; ++t) {
    CHECK(filter_tile_empty_from(w.p, N, t, first) == (bool)empty[(size_t)t]);
    if (first == 1) CHECK(filter_tile_empty(w.p, N, t) == (bool)empty[(size_t)t]);
    for (int ww = 0; ww < FILTER_TILE_WORDS; ++ww)
      CHECK(filter_wave_word_from(w.p, N, t, ww, first) == filter_word_from(w.p, N, FILTER_TILE_WORDS * t + ww, first));
  }
  for (int64_t t1 = 0; t1 <= tiles; ++t1)
    for (int64_t t = 0; t <= t1; ++t) {
      int64_t want = t;
      while (want < t1 && empty[(size_t)want]) ++want;
      CHECK(filter_next_tile_from(w.p, N, t, t1, first) == want);
      if (first == 1) CHECK(filter_next_tile(w.p, N, t, t1) == want);
    }
}

static int from_stdin() {
  static char line[1 << 16];
  while (fgets(line, sizeof line, stdin)) {
    char* at = line;
    const int64_t N = strtoll(at, &at, 10);
    if (N < 1) continue;
    const int64_t first = strtoll(at, &at, 10);
    const int64_t nw = filter_words(N);
    Words w(nw);
    for (int64_t j = 0; j < nw; ++j) w.p[j] = (uint32_t)strtoul(at, &at, 16);
    for (int64_t j = 0; j < nw; ++j) printf("%s%x", j ? " " : "", filter_word_from(w.p, N, j, first));
    printf("\n");
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && strcmp(argv[1], "-") == 0) return from_stdin();
  const int64_t Ns[] = {1, 2, 31, 32, 33, 127, 128, 129, 255, 256, 257, 300, 1000};
  const int64_t firsts[] = {0, 1, 5, 31, 32, 33, 128, 200, 5000};
  long cases = 0;
  for (int64_t N : Ns)
    for (int64_t first : firsts)
      for (int pattern = 0; pattern <= 5; ++pattern) {
        sweep_one(N, first, pattern);
        ++cases;
      }
  printf("%ld cases, %d failures\n", cases, failures);
  return failures != 0;
}
