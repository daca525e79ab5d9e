// spec_feed_fold.cpp -- the byte a folded feed computes at a cut (aha_amd/csrc/feed_fold.hpp: feedfold_byte, what kff_heads and
// kff_windows of scan_feedfold.hip are made of) against the host's statement of the folds (fold.hpp: fold2_bytes,
// fold3_bytes_with) on ctx || P as ONE buffer: for every sequence over the alphabet {a lead byte of two, a lead byte of three, a
// continuation byte, an ASCII letter} up to length 6 and every split of it into a context and a piece, every byte of the piece
// -- the first two are what kff_heads writes -- and every byte of the context -- what kff_windows writes -- for the simple, the
// BMP and the kana fold; then the same with only the last two bytes of the context in view, which is all kff_heads reads.  A
// stand-alone program (its own main; no GPU, no library): built with -fsanitize=address,undefined by
// tests/test_feed_fold_host.py, every buffer on the heap at its exact length, so an index the helper does not test first is a
// finding.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../aha_amd/csrc/feed_fold.hpp"

static int failures = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      if (failures++ < 20) fprintf(stderr, "line %d: %s\n", __LINE__, #cond); \
    }                                                            \
  } while (0)

typedef std::vector<uint8_t> Buf;

static aha::Fold3Tables tables(int mode) {
  if (mode == 4) return aha::Fold3Tables{aha::kFold2Table, aha::kFoldKIndex, aha::kFoldKLive};
  return aha::Fold3Tables{aha::kFold2Table, aha::kFold3Index, aha::kFold3Live};
}

// the fold of one buffer, on a heap copy of exactly its length
static Buf whole(int mode, const Buf &in) {
  Buf out(in);
  if (mode == 2)
    aha::fold2_bytes(out.data(), out.size());
  else
    aha::fold3_bytes_with(tables(mode), out.data(), out.size());
  return out;
}

static long checked = 0;

static void check_split(int mode, const Buf &seq, size_t cut) {
  const aha::Fold3Tables T = tables(mode);
  const Buf want = whole(mode, seq);
  // the context and the piece as buffers of their own: an index past either is out of bounds
  const Buf ctx(seq.begin(), seq.begin() + cut), piece(seq.begin() + cut, seq.end());
  const uint32_t lc = (uint32_t)ctx.size();
  const uint64_t L = piece.size();
  for (int64_t k = -(int64_t)lc; k < (int64_t)L; k++) {
    CHECK(aha::feedfold_byte(T, mode, ctx.data(), lc, piece.data(), L, k) == want[cut + k]);
    checked++;
  }
  // kff_heads: bytes 0 and 1 of the piece from the last two bytes of the context alone
  const size_t tail = cut < 2 ? cut : 2;
  const Buf last(ctx.end() - tail, ctx.end());
  for (int64_t k = 0; k < 2 && k < (int64_t)L; k++) {
    CHECK(aha::feedfold_byte(T, mode, last.data(), (uint32_t)tail, piece.data(), L, k) == want[cut + k]);
    checked++;
  }
}

int main() {
  // two live characters of each width, so that a fold that is applied shows: U+0416 (D0 96 -> D0 B6), U+1EC6 (E1 BB 86 -> E1 BB
  // 87) and, for the kana fold, U+3042 (E3 81 82 -> E3 82 A2)
  static const uint8_t kLead2[] = {0xD0, 0xC3}, kLead3[] = {0xE1, 0xE3, 0xEF}, kCont[] = {0x96, 0xBB, 0x86, 0x81, 0x82, 0xBC},
                       kAscii[] = {'A', 'z'};
  for (int mode = 2; mode <= 4; mode++) {
    for (size_t n = 0; n <= 6; n++) {
      // every sequence of n classes; the byte of a class is chosen by the position, so all of a class's bytes come up
      size_t total = 1;
      for (size_t i = 0; i < n; i++) total *= 4;
      for (size_t code = 0; code < total; code++) {
        for (size_t variant = 0; variant < 3; variant++) {
          Buf seq(n);
          size_t c = code;
          for (size_t i = 0; i < n; i++, c /= 4) {
            const size_t cls = c % 4, pick = i + variant;
            seq[i] = cls == 0 ? kLead2[pick % 2] : cls == 1 ? kLead3[pick % 3] : cls == 2 ? kCont[(2 * pick + variant) % 6] : kAscii[pick % 2];
          }
          for (size_t cut = 0; cut <= n; cut++) check_split(mode, seq, cut);
        }
      }
    }
  }
  // whole characters cut at every byte, where the expected bytes are known by heart
  {
    const Buf zhe = {0xD0, 0x96}, viet = {0xE1, 0xBB, 0x86}, hira = {0xE3, 0x81, 0x82};
    CHECK(whole(2, zhe) == (Buf{0xD0, 0xB6}));
    CHECK(whole(3, viet) == (Buf{0xE1, 0xBB, 0x87}) && whole(2, viet) == viet);
    CHECK(whole(4, hira) == (Buf{0xE3, 0x82, 0xA2}) && whole(3, hira) == hira);
    const aha::Fold3Tables T4 = tables(4);
    // the triple's last byte arrives alone: folded from the two context bytes
    CHECK(aha::feedfold_byte(T4, 4, hira.data(), 2, hira.data() + 2, 1, 0) == 0xA2);
    // its lead byte is still open at the piece's end: it passes through, and so does lead + one continuation byte
    CHECK(aha::feedfold_byte(T4, 4, nullptr, 0, hira.data(), 1, 0) == 0xE3);
    CHECK(aha::feedfold_byte(T4, 4, nullptr, 0, hira.data(), 2, 1) == 0x81);
  }
  if (failures) {
    fprintf(stderr, "spec_feed_fold: %d failures\n", failures);
    return 1;
  }
  printf("spec_feed_fold: ok (%ld bytes checked)\n", checked);
  return 0;
}
