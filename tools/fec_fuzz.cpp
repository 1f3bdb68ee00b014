// Hostile input to the protected-stream decoder, for a sanitizer build on the CPU (no GPU, no HIP runtime):
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/fec_fuzz.cpp
//       rdeic_amd/csrc/fec.cpp -o tools/fec_fuzz && tools/fec_fuzz          (one command line)
//
// Protects payloads of many sizes at many (nroots, depth), then drives rdeic_fec_decode over bit-flipped, byte-
// smashed, truncated, extended and length-lying copies, every buffer allocated at its exact size so that one byte
// read or written outside it is a sanitizer report. Checks the contract: a clean stream decodes to its payload; a
// stream with at most t byte errors per codeword decodes to its payload with exactly that many corrections; and
// whatever else happens, a status of 0 means the bytes are the original's (no silent wrong output). Prints its
// counts and exits 0; any sanitizer report or broken promise is a nonzero exit.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../include/rdeic_hip.h"

namespace {

uint64_t rng_state = 0x9e3779b97f4a7c15ull;
uint32_t rnd() {  // xorshift64*: the same streams on every run
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return (uint32_t)((rng_state * 0x2545f4914f6cdd1dull) >> 32);
}

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
      exit(1);                                                             \
    }                                                                      \
  } while (0)

struct Result {
  int rc;
  std::vector<uint8_t> out;
  rdeic_fec_stats st;
};

// exact-size heap copies of the input and the output: the sanitizer sees every byte outside them
Result decode(const std::vector<uint8_t>& in, size_t cap) {
  uint8_t* src = in.empty() ? nullptr : (uint8_t*)malloc(in.size());
  if (src) memcpy(src, in.data(), in.size());
  uint8_t* dst = cap ? (uint8_t*)malloc(cap) : nullptr;
  size_t n = 0;
  Result r;
  r.rc = rdeic_fec_decode(src, in.size(), dst, cap, &n, &r.st);
  CHECK(r.rc == 0 || r.rc == -74 || r.rc == -28 || r.rc == -22);
  CHECK(n <= cap && (r.rc == 0 || n == 0));
  r.out.assign(dst, dst + n);
  free(src);
  free(dst);
  return r;
}

}  // namespace

int main() {
  // block level, and the CRC's check value
  const uint8_t qr[16] = {32, 91, 11, 120, 209, 114, 220, 77, 67, 64, 236, 17, 236, 17, 236, 17};
  const uint8_t qr_par[10] = {196, 35, 39, 119, 235, 215, 231, 226, 93, 23};
  uint8_t par[64];
  CHECK(rdeic_rs_encode(qr, 16, 10, par) == 0 && memcmp(par, qr_par, 10) == 0);
  CHECK(rdeic_crc32((const uint8_t*)"123456789", 9) == 0xCBF43926u);
  CHECK(rdeic_rs_encode(qr, 16, 11, par) == -22 && rdeic_rs_encode(qr, 0, 10, par) == -22);
  CHECK(rdeic_rs_encode(qr, 246, 10, par) == -22 && rdeic_rs_encode(nullptr, 16, 10, par) == -22);

  const int roots[] = {2, 4, 16, 32, 64};
  const int depths[] = {1, 2, 4, 16, 255};
  long streams = 0, clean_ok = 0, repaired = 0, refused = 0, silent_ok = 0, lied = 0, cut = 0, trials = 0;
  for (int round = 0; round < 600; ++round) {
    const int nroots = roots[rnd() % 5], depth = depths[rnd() % 5], k = 255 - nroots, t = nroots / 2;
    size_t n;
    switch (rnd() % 6) {
      case 0: n = 0; break;
      case 1: n = 1 + rnd() % 3; break;
      case 2: n = (size_t)k * (1 + rnd() % 5) + (rnd() % 3) - 1; break;  // around a block boundary
      case 3: n = (size_t)k * depth + (rnd() % 3) - 1; break;            // around a group boundary
      default: n = rnd() % 9000; break;
    }
    if (n > 70000) n = 70000;
    std::vector<uint8_t> payload(n);
    for (auto& b : payload) b = (uint8_t)rnd();
    const size_t size = rdeic_fec_encoded_size(n, nroots, depth);
    const size_t ncw = (n + k - 1) / k;
    CHECK(size == 46 + n + nroots * ncw);
    std::vector<uint8_t> enc(size);
    if (size > 46) CHECK(rdeic_fec_encode(payload.data(), n, nroots, depth, enc.data(), size - 1) == -28);
    CHECK(rdeic_fec_encode(payload.empty() ? nullptr : payload.data(), n, nroots, depth, enc.data(), size) == 0);
    ++streams;

    Result r = decode(enc, n);
    CHECK(r.rc == 0 && r.out == payload && r.st.corrected == 0 && r.st.uncorrectable == 0);
    CHECK((size_t)r.st.codewords == ncw + 1);
    ++clean_ok;
    if (n > 0) CHECK(decode(enc, n - 1).rc == -28);

    // exactly t byte errors in every codeword, the header's 16 included: de-interleave by the format's own rule
    {
      std::vector<uint8_t> e = enc;
      long injected = 0;
      auto smash = [&](std::vector<size_t>& where, int count) {  // `count` distinct positions of one codeword
        for (int c = 0; c < count; ++c) {
          const size_t j = c + rnd() % (where.size() - c);
          std::swap(where[c], where[j]);
          e[where[c]] ^= (uint8_t)(1 + rnd() % 255);
          ++injected;
        }
      };
      std::vector<size_t> w(46);
      for (size_t i = 0; i < 46; ++i) w[i] = i;
      smash(w, 16);
      size_t base = 46;
      for (size_t first = 0; first < ncw; first += depth) {
        const size_t grp = ncw - first < (size_t)depth ? ncw - first : (size_t)depth;
        std::vector<std::vector<size_t>> cw(grp);
        std::vector<size_t> len(grp, 255);
        if (first + grp == ncw) len[grp - 1] = n - (ncw - 1) * k + nroots;
        size_t at = base;
        for (size_t j = 0; j < 255; ++j)
          for (size_t c = 0; c < grp; ++c)
            if (j < len[c]) cw[c].push_back(at++);
        for (size_t c = 0; c < grp; ++c) smash(cw[c], (int)len[c] < t ? (int)len[c] : t);
        base = at;
      }
      CHECK(base == size);
      Result q = decode(e, n);
      CHECK(q.rc == 0 && q.out == payload && q.st.corrected == injected && q.st.uncorrectable == 0);
      ++repaired;
    }

    // random corruption at mixed rates, truncation, extension, a header that lies about the length
    for (int v = 0; v < 12; ++v) {
      std::vector<uint8_t> e = enc;
      const uint32_t kind = rnd() % 6;
      if (kind <= 2) {  // bit flips: per-bit rate 1e-4 .. 5e-2
        const double rates[] = {1e-4, 1e-3, 5e-3, 1e-2, 2e-2, 5e-2};
        const double p = rates[rnd() % 6];
        for (size_t i = 0; i < e.size() * 8; ++i)
          if (rnd() < p * 4294967296.0) e[i / 8] ^= (uint8_t)(1u << (i % 8));
      } else if (kind == 3) {  // a burst of random bytes anywhere
        const size_t len = 1 + rnd() % (size_t)(2 * depth * t + 2), at = rnd() % e.size();
        for (size_t i = at; i < e.size() && i < at + len; ++i) e[i] = (uint8_t)rnd();
      } else if (kind == 4) {  // cut to any length (0 included) or extended
        if (rnd() % 4 == 0)
          e.resize(e.size() + 1 + rnd() % 300, 0xa5);
        else
          e.resize(rnd() % e.size());
        ++cut;
      } else {  // a valid header codeword announcing another length, roots or depth
        uint8_t h[14];
        memcpy(h, e.data(), 14);
        const uint32_t what = rnd() % 4;
        if (what == 0) {
          const uint32_t big = (uint32_t)n + 1 + rnd() % 100000;
          h[6] = (uint8_t)(big >> 24), h[7] = (uint8_t)(big >> 16), h[8] = (uint8_t)(big >> 8), h[9] = (uint8_t)big;
        } else if (what == 1) {
          h[6] = h[7] = h[8] = h[9] = 0xff;
        } else if (what == 2) {
          h[4] = (uint8_t)rnd();
        } else {
          h[5] = (uint8_t)rnd();
        }
        memcpy(e.data(), h, 14);
        CHECK(rdeic_rs_encode(h, 14, 32, e.data() + 14) == 0);
        ++lied;
      }
      const bool same = e == enc;
      Result q = decode(e, n);
      ++trials;
      if (q.rc == 0) {
        CHECK(q.out == payload);  // the contract: a clean status is the original's bytes
        if (!same) ++silent_ok;
      } else {
        CHECK(!same);
        ++refused;
      }
    }
  }
  // the calls' own arguments
  size_t n = 0;
  uint8_t b[64] = {0};
  CHECK(rdeic_fec_decode(b, 64, b, 64, nullptr, nullptr) == -22);
  CHECK(rdeic_fec_decode(nullptr, 64, b, 64, &n, nullptr) == -22);
  CHECK(rdeic_fec_decode(nullptr, 0, nullptr, 0, &n, nullptr) == -74);
  CHECK(rdeic_fec_decode(b, 45, b, 64, &n, nullptr) == -74);
  CHECK(rdeic_fec_encode(b, 8, 3, 1, b, 64) == -22 && rdeic_fec_encode(b, 8, 66, 1, b, 64) == -22);
  CHECK(rdeic_fec_encode(b, 8, 32, 0, b, 64) == -22 && rdeic_fec_encode(b, 8, 32, 256, b, 64) == -22);
  CHECK(rdeic_fec_encoded_size(8, 3, 1) == 0 && rdeic_fec_encoded_size(8, 32, 0) == 0);
  printf("fec_fuzz: %ld streams, %ld clean exact, %ld repaired at t errors in every codeword; %ld hostile trials "
         "(%ld length-lying headers, %ld cut or extended): %ld refused, %ld recovered exactly, 0 wrong\n",
         streams, clean_ok, repaired, trials, lied, cut, refused, silent_ok);
  CHECK(refused > 1000 && silent_ok > 500);
  return 0;
}
