// test_norm_swar.cpp — host check of the three word-wide ASCII helpers of the normalise pre-pass (csrc/utf8_swar.h:
// norm_ascii_lower, norm_ascii_dropped16, norm_ascii16) against the per-byte rules of norm_cp (csrc/normalize.h):
//   lower    c - 0x41 < 26 ? c + 0x20 : c, over every word of four bytes below 0x80 (128^4 words: every byte value at each
//            of the four positions with the other three running over all values);
//   dropped  (c < 0x20 && c != 9, 10, 13) || c == 0x7F, on the bytes below 0x80 of a 16-byte chunk (the caller masks the
//            others out: normalize.h, `starts & ascii16 & drop16`): every byte value at each of the 16 positions over
//            several backgrounds, and a few million seeded chunks of four mixes;
//   ascii    c < 0x80, on the same chunks.
// Built and run by tests/test_norm_swar.py (g++, no GPU).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>

#include "../../wordpiece_amd/csrc/utf8_swar.h"

static bool dropped_rule(uint32_t c) { return (c < 0x20u && c != 0x09u && c != 0x0au && c != 0x0du) || c == 0x7fu; }

static long chunks = 0;
static bool chunk_ok(const uint8_t (&b)[16], const char *what) {
  uint32_t w[5] = {0, 0, 0, 0, 0xffffffffu};  // (w[4], the word behind the chunk, is not looked at)
  std::memcpy(w, b, 16);
  uint32_t ascii = 0, drop = 0;
  for (int j = 0; j < 16; j++) {
    if (b[j] < 0x80u) ascii |= 1u << j;
    if (b[j] < 0x80u && dropped_rule(b[j])) drop |= 1u << j;
  }
  const uint32_t got_ascii = wp::norm_ascii16(w), got_drop = wp::norm_ascii_dropped16(w) & got_ascii;
  chunks++;
  if (got_ascii != ascii || got_drop != drop) {
    static int shown = 0;
    if (shown++ >= 4) return false;
    std::printf("MISMATCH (%s): chunk", what);
    for (int j = 0; j < 16; j++) std::printf(" %02x", b[j]);
    std::printf(": ascii %04x, expected %04x; dropped %04x, expected %04x\n", got_ascii, ascii, got_drop, drop);
    return false;
  }
  return true;
}

int main() {
  bool ok = true;
  // ---- lower: all 128^4 ASCII words
  uint32_t low[128];
  for (uint32_t c = 0; c < 128; c++) low[c] = c - 0x41u < 26u ? c + 0x20u : c;
  long words = 0, bad_words = 0;
  for (uint32_t b3 = 0; b3 < 128; b3++) {
    for (uint32_t b2 = 0; b2 < 128; b2++) {
      for (uint32_t b1 = 0; b1 < 128; b1++) {
        const uint32_t hi = (b3 << 24) | (b2 << 16) | (b1 << 8), hi_low = (low[b3] << 24) | (low[b2] << 16) | (low[b1] << 8);
        for (uint32_t b0 = 0; b0 < 128; b0++) {
          if (wp::norm_ascii_lower(hi | b0) != (hi_low | low[b0])) {
            if (bad_words++ < 4) {
              std::printf("MISMATCH (lower): %08x -> %08x, expected %08x\n", hi | b0, wp::norm_ascii_lower(hi | b0), hi_low | low[b0]);
            }
          }
          words++;
        }
      }
    }
  }
  ok = ok && bad_words == 0;
  // ---- dropped, ascii: every byte value at every position of the chunk, over backgrounds of each kind
  const uint8_t grounds[] = {0x61, 0x00, 0x09, 0x1f, 0x20, 0x7f, 0x80, 0xff};
  for (uint8_t g : grounds) {
    for (int pos = 0; pos < 16; pos++) {
      for (int c = 0; c < 256; c++) {
        uint8_t b[16];
        std::memset(b, g, 16);
        b[pos] = static_cast<uint8_t>(c);
        ok = chunk_ok(b, "single value") && ok;
      }
    }
  }
  // ---- seeded chunks: any byte; ASCII only; the values around the rule's edges; mostly letters with a few of those
  const uint8_t edges[] = {0x00, 0x01, 0x08, 0x09, 0x0a, 0x0b, 0x0c, 0x0d, 0x0e, 0x1e, 0x1f, 0x20, 0x21, 0x7e, 0x7f, 0x80, 0x81, 0x89,
                           0x8a, 0x8d, 0x9f, 0xa0, 0xff};
  std::mt19937 rnd(20261019);
  for (int it = 0; it < 4000000 && ok; it++) {
    uint8_t b[16];
    const unsigned mode = static_cast<unsigned>(it) & 3u;
    for (auto &c : b) {
      const uint32_t r = rnd();
      c = mode == 0   ? static_cast<uint8_t>(r)
          : mode == 1 ? static_cast<uint8_t>(r & 0x7fu)
          : mode == 2 ? edges[r % sizeof(edges)]
                      : ((r >> 8) % 5u == 0 ? edges[r % sizeof(edges)] : static_cast<uint8_t>(0x41u + (r >> 16) % 58u));
    }
    ok = chunk_ok(b, "seeded") && ok;
  }
  std::printf("%ld words lowered (%ld differ), %ld chunks checked: %s\n", words, bad_words, chunks, ok ? "ok" : "FAILED");
  return ok ? 0 : 1;
}
