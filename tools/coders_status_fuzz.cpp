// Hostile input to the host rANS decoder, for a sanitizer build on the CPU (no GPU, no HIP runtime):
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread \
//       tools/coders_status_fuzz.cpp rdeic_amd/csrc/coders.cpp -o tools/coders_status_fuzz && tools/coders_status_fuzz
//
// Encodes a batch of streams, then drives rdeic_rans_decode_batch_status over a few hundred bit-flipped and
// truncated copies of them in two stages, the way the isolating decompress does (status carried from stage to
// stage, threads on). Checks what the header promises: clean streams decode to their symbols, failed and skipped
// streams' rows are all zero, a failed stream stays failed, the call itself returns 0. Prints a count and exits 0;
// any sanitizer report or broken promise is a nonzero exit.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <cmath>
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

}  // namespace

int main() {
  // Gaussian-like tables: `levels` rows of widths 3 .. 3 + 4 (levels - 1) around a centre
  const int32_t levels = 8, max_len = 3 + 4 * (levels - 1), pmf_ld = max_len + 1, cdf_ld = max_len + 2;
  std::vector<float> pmf((size_t)levels * pmf_ld, 0.f);
  std::vector<int32_t> pmf_len(levels), offset(levels), cdf((size_t)levels * cdf_ld), cdf_len(levels);
  for (int32_t l = 0; l < levels; ++l) {
    const int32_t len = 3 + 4 * l, c = len / 2;
    const double sigma = 0.3 + 0.6 * l;
    double sum = 0;
    for (int32_t j = 0; j < len; ++j) sum += std::exp(-0.5 * (j - c) * (j - c) / (sigma * sigma));
    for (int32_t j = 0; j < len; ++j)
      pmf[(size_t)l * pmf_ld + j] = (float)(std::exp(-0.5 * (j - c) * (j - c) / (sigma * sigma)) / sum * (1.0 - 1e-4));
    pmf[(size_t)l * pmf_ld + len] = 1e-4f;  // the tail mass (bypass symbol)
    pmf_len[l] = len;
    offset[l] = -c;
  }
  CHECK(rdeic_build_gaussian_tables(pmf.data(), pmf_len.data(), levels, pmf_ld, cdf.data(), cdf_ld, cdf_len.data(),
                                    nullptr) == 0);

  const int32_t count = 6;
  const size_t n_per = 900, half = n_per / 2;
  std::vector<int32_t> idx(count * n_per), sym(count * n_per);
  for (size_t i = 0; i < idx.size(); ++i) {
    idx[i] = (int32_t)(rnd() % levels);
    const int32_t c = pmf_len[idx[i]] / 2;
    // mostly inside the table, now and then outside it (coded through the bypass nibbles)
    sym[i] = (rnd() % 50 == 0) ? (int32_t)(rnd() % 4001) - 2000 : (int32_t)(rnd() % (2 * c + 1)) - c;
  }
  const size_t cap = 4 * (n_per * 4 + 16);
  std::vector<uint8_t> enc(count * cap);
  std::vector<size_t> enc_len(count);
  CHECK(rdeic_rans_encode_batch(count, sym.data(), idx.data(), n_per, n_per, cdf.data(), cdf_ld, cdf_len.data(),
                                offset.data(), levels, enc.data(), cap, enc_len.data(), 2) == 0);

  // stage views: [count][half] index / symbol blocks, as the 20-stage loop hands them over
  std::vector<int32_t> idx_a(count * half), idx_b(count * half), out_a(count * half), out_b(count * half);
  for (int32_t i = 0; i < count; ++i)
    for (size_t j = 0; j < half; ++j) {
      idx_a[i * half + j] = idx[i * n_per + j];
      idx_b[i * half + j] = idx[i * n_per + half + j];
    }

  long rounds = 0, failed_streams = 0, clean_streams = 0, survived_corrupt = 0;
  for (int round = 0; round < 400; ++round) {
    std::vector<std::vector<uint8_t>> data(count);
    std::vector<int> touched(count, 0);
    std::vector<void*> handles(count, nullptr);
    for (int32_t i = 0; i < count; ++i) {
      data[i].assign(enc.begin() + i * cap, enc.begin() + i * cap + enc_len[i]);
      const uint32_t kind = (i == 0) ? 0 : rnd() % 5;  // stream 0 always stays clean
      if (kind == 1 || kind == 2) {                     // bit flips: a few, or many
        const size_t flips = kind == 1 ? 1 + rnd() % 4 : data[i].size() / 10;
        for (size_t f = 0; f < flips; ++f) data[i][rnd() % data[i].size()] ^= (uint8_t)(1u << (rnd() % 8));
        touched[i] = 1;
      } else if (kind == 3) {  // truncated to any length, 0 and odd ones included
        data[i].resize(rnd() % data[i].size());
        touched[i] = 1;
      } else if (kind == 4) {  // no decoder at all
        touched[i] = 2;
        continue;
      }
      handles[i] = rdeic_rans_dec_open(data[i].empty() ? nullptr : data[i].data(), data[i].size());
      CHECK(handles[i] != nullptr);
    }
    std::vector<int32_t> status(count, 0);
    for (auto& v : out_a) v = 0x5a5a5a5a;
    for (auto& v : out_b) v = 0x5a5a5a5a;
    CHECK(rdeic_rans_decode_batch_status(count, handles.data(), idx_a.data(), half, half, cdf.data(), cdf_ld,
                                         cdf_len.data(), offset.data(), levels, out_a.data(), 1 + round % 4,
                                         status.data()) == 0);
    const std::vector<int32_t> first = status;
    CHECK(rdeic_rans_decode_batch_status(count, handles.data(), idx_b.data(), half, half, cdf.data(), cdf_ld,
                                         cdf_len.data(), offset.data(), levels, out_b.data(), 1 + round % 4,
                                         status.data()) == 0);
    for (int32_t i = 0; i < count; ++i) {
      CHECK(status[i] == 0 || status[i] == -74 || status[i] == -22);
      if (first[i] != 0) CHECK(status[i] == first[i]);  // a failed stream stays failed
      const bool zero_a = touched[i] == 2 || first[i] != 0, zero_b = touched[i] == 2 || status[i] != 0;
      for (size_t j = 0; j < half; ++j) {
        if (zero_a) CHECK(out_a[i * half + j] == 0);
        if (zero_b) CHECK(out_b[i * half + j] == 0);
        if (!touched[i]) {
          CHECK(out_a[i * half + j] == sym[i * n_per + j]);
          CHECK(out_b[i * half + j] == sym[i * n_per + half + j]);
        }
      }
      if (touched[i] == 2) CHECK(status[i] == 0);  // skipped: its status is not written
      if (!touched[i]) {
        CHECK(status[i] == 0);
        ++clean_streams;
      } else if (status[i] != 0) {
        ++failed_streams;
      } else if (touched[i] == 1) {
        ++survived_corrupt;  // decoded to something: garbage symbols, but a clean status
      }
      if (handles[i]) rdeic_rans_dec_close(handles[i]);
    }
    ++rounds;
  }
  // the call's own arguments
  int32_t st = 0, o = 0, ix = 0;
  void* none = nullptr;
  CHECK(rdeic_rans_decode_batch_status(0, &none, &ix, 1, 1, cdf.data(), cdf_ld, cdf_len.data(), offset.data(), levels,
                                       &o, 1, &st) == -22);
  CHECK(rdeic_rans_decode_batch_status(1, &none, &ix, 1, 1, cdf.data(), cdf_ld, cdf_len.data(), offset.data(), levels,
                                       &o, 1, nullptr) == -22);
  CHECK(rdeic_rans_decode_batch_status(1, &none, &ix, 2, 1, cdf.data(), cdf_ld, cdf_len.data(), offset.data(), levels,
                                       &o, 1, &st) == -22);
  printf("coders_status_fuzz: %ld rounds, %ld clean streams exact, %ld corrupted streams failed, %ld decoded on\n",
         rounds, clean_streams, failed_streams, survived_corrupt);
  CHECK(failed_streams > 100 && clean_streams >= rounds);
  return 0;
}
