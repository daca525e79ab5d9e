// token_rule.hpp -- where the tokens of a token call start (AHA_SELECT_TOKENS; DESIGN.md 4.14 "Tokens"), stated per 32-bit
// word of the position masks.  Host and device: the kernels of scan_tokens.hip and a stand-alone CPU program (tests/cpp/
// spec_token_rule.cpp) share this one definition.  Bit i of a word is position 32 w + i of the range's text.
//   select     a selected hit starts here
//   inside     a selected hit holds the byte ([start, end) of every selected hit)
//   doc_start  a document starts here
//   cont       the caller's byte is a UTF-8 continuation byte, (b & 0xC0) == 0x80
// A position starts a token iff a selected hit starts there, or it is not inside and a document starts there, its
// predecessor is inside, or -- unless gaps are single tokens -- its byte is no continuation byte.  The rule is bytewise and
// total: nothing about the text has to be valid.
#pragma once
#include <cstdint>

#ifndef AHA_HD
#if defined(__HIPCC__)
#define AHA_HD __host__ __device__
#else
#define AHA_HD
#endif
#endif

namespace aha {

// bit k = (byte k of the little-endian word w is a continuation byte), k in [0, 4)
AHA_HD inline uint32_t token_cont4(uint32_t w) {
  const uint32_t t = w & ~(w << 1) & 0x80808080u;  // 0x80 where bit 7 is set and bit 6 is clear
  return (((t >> 7) * 0x00204081u) >> 21) & 0xFu;
}

// the bits of word w that lie below nb (0 where the word starts at or behind nb)
AHA_HD inline uint32_t token_valid(uint64_t w, uint64_t nb) {
  const uint64_t p0 = w * 32;
  if (p0 >= nb) return 0u;
  return nb - p0 >= 32 ? ~0u : ~(~0u << (uint32_t)(nb - p0));
}

// A text that starts `head` bytes (below 32) in front of a word border of the loads that read it: the mask word is the last
// `head` bits of the loaded word in front (prev) and the first 32 - head bits of its own (cur)
AHA_HD inline uint32_t token_funnel(uint32_t prev, uint32_t cur, uint32_t head) {
  return (uint32_t)(((uint64_t)cur << 32 | prev) >> (32u - head));
}

// ---- the continuation bits of a text that may start anywhere.  The wide loads are aligned to the ADDRESS: corpus + head is
// the first 16-byte aligned address (head < 16; head = the text's length where it is shorter), text = corpus + head, na = the
// bytes from there on.  Loaded word j holds text positions [32 j, 32 j + 32); mask word w is token_funnel(loaded word w - 1,
// loaded word w, head), with token_cont_head in front of the first.  Nothing outside [corpus, corpus + head + na) is read.

// the 16 bits of the aligned piece at text position a (a multiple of 16): a whole piece by one 16-byte load, the bytes of the
// last, partial one singly
AHA_HD inline uint32_t token_cont16(const uint8_t *text, uint64_t a, uint64_t na) {
  if (a + 16 <= na) {
    uint32_t q[4];
    __builtin_memcpy(q, __builtin_assume_aligned(text + a, 16), 16);
    return token_cont4(q[0]) | token_cont4(q[1]) << 4 | token_cont4(q[2]) << 8 | token_cont4(q[3]) << 12;
  }
  uint32_t bits = 0;
  for (uint32_t k = 0; k < 16; k++)
    if (a + k < na && (text[a + k] & 0xC0u) == 0x80u) bits |= 1u << k;
  return bits;
}

AHA_HD inline uint32_t token_cont32(const uint8_t *text, uint64_t j, uint64_t na) {
  return token_cont16(text, j * 32, na) | token_cont16(text, j * 32 + 16, na) << 16;
}

// the head bytes, as the top bits of the loaded word in front of the first
AHA_HD inline uint32_t token_cont_head(const uint8_t *corpus, uint32_t head) {
  uint32_t bits = 0;
  for (uint32_t k = 0; k < head; k++)
    if ((corpus[k] & 0xC0u) == 0x80u) bits |= 1u << (32 - head + k);
  return bits;
}

// the token starts of one word.  inside_prev: bit 0 = the last position of the word in front is inside (0 for the first word);
// valid: token_valid of the word
AHA_HD inline uint32_t token_starts(uint32_t select, uint32_t inside, uint32_t doc_start, uint32_t inside_prev, uint32_t cont,
                                    bool gap_runs, uint32_t valid) {
  const uint32_t behind = inside << 1 | (inside_prev & 1u);  // p - 1 is inside
  const uint32_t lead = gap_runs ? 0u : ~cont;
  return (select | (~inside & (doc_start | behind | lead))) & valid;
}

}  // namespace aha
