// Forward error correction for the RDEIC bitstream: Reed-Solomon over GF(2^8) with a CRC-32 of the payload,
// behind a header that is itself a codeword (DESIGN.md "Protected streams"). Host C++ beside the rANS coder:
// no HIP runtime, and a 2.5-129 KB stream costs far less here than one relay decode costs on the device.
//
// The code: field polynomial 0x11d, alpha = 2, generator g(x) = prod_{i=0}^{nroots-1} (x - alpha^i) (first root
// alpha^0, spacing 1), systematic: parity = m(x) x^nroots mod g(x), appended after the data, highest degree first.
// nroots even, 2..64; a codeword carries at most 255 - nroots data bytes and a shorter block is the shortened code
// (nothing is padded on the wire). The QR-code standard uses the same field, roots and byte order, which is what
// the known-answer test pins.
//
// The protected stream:
//   header codeword, 46 bytes : "RDF1", u8 nroots, u8 depth, u32be payload length, u32be CRC-32 of the payload,
//                               then 32 parity bytes (the code above with nroots = 32: 16 byte errors repaired)
//   body                      : the payload in blocks of k = 255 - nroots bytes (the last may be shorter), each a
//                               codeword of len + nroots bytes; codewords are taken `depth` at a time and the bytes
//                               of such a group go out round-robin (byte j of codeword 0, of codeword 1, ...,
//                               skipping a codeword that has ended)
// so its size is 46 + n + nroots * ceil(n / k).
//
// Every export is reentrant (the only shared data are the constant tables below) and bounds every access by the
// buffer sizes it was given, whatever the bytes announce.
#include <stdint.h>
#include <string.h>

#include "../../include/rdeic_hip.h"

#define RDEIC_OK 0
#define RDEIC_EINVAL (-22)
#define RDEIC_ENOSPC (-28)
#define RDEIC_EBADMSG (-74)

namespace {

constexpr int kMaxRoots = 64;
constexpr int kHdrData = 14, kHdrRoots = 32, kHdrLen = kHdrData + kHdrRoots;

struct Gf {
  uint8_t exp[512];  // alpha^i for i in 0..509 (two periods: a product's log sum needs no reduction)
  uint8_t log[256];
};

constexpr Gf make_gf() {
  Gf g{};
  unsigned x = 1;
  for (int i = 0; i < 255; ++i) {
    g.exp[i] = (uint8_t)x;
    g.log[x] = (uint8_t)i;
    x <<= 1;
    if (x & 0x100) x ^= 0x11d;
  }
  for (int i = 255; i < 512; ++i) g.exp[i] = g.exp[i - 255];
  g.log[0] = 0;  // never read: every use tests for zero first
  return g;
}

struct Crc {
  uint32_t t[256];
};

constexpr Crc make_crc() {
  Crc c{};
  for (uint32_t i = 0; i < 256; ++i) {
    uint32_t r = i;
    for (int b = 0; b < 8; ++b) r = (r >> 1) ^ ((r & 1) ? 0xedb88320u : 0u);
    c.t[i] = r;
  }
  return c;
}

constexpr Gf kGf = make_gf();
constexpr Crc kCrc = make_crc();

inline uint8_t gmul(uint8_t a, uint8_t b) { return (a && b) ? kGf.exp[kGf.log[a] + kGf.log[b]] : 0; }
inline uint8_t gdiv(uint8_t a, uint8_t b) { return a ? kGf.exp[kGf.log[a] + 255 - kGf.log[b]] : 0; }  // b != 0

uint32_t crc32(const uint8_t* p, size_t n) {
  uint32_t r = 0xffffffffu;
  for (size_t i = 0; i < n; ++i) r = kCrc.t[(r ^ p[i]) & 0xff] ^ (r >> 8);
  return r ^ 0xffffffffu;
}

bool roots_ok(int32_t nroots) { return nroots >= 2 && nroots <= kMaxRoots && (nroots & 1) == 0; }

// g(x), coefficients from x^nroots (g[0] = 1) down to x^0
void generator(int nroots, uint8_t* g) {
  g[0] = 1;
  for (int i = 0; i < nroots; ++i) {  // times (x + alpha^i); degree i before, i + 1 after
    const uint8_t r = kGf.exp[i];
    g[i + 1] = gmul(r, g[i]);
    for (int j = i; j >= 1; --j) g[j] ^= gmul(r, g[j - 1]);
  }
}

// parity[nroots] of data[n], n <= 255 - nroots
void rs_parity(const uint8_t* data, int n, int nroots, const uint8_t* g, uint8_t* par) {
  memset(par, 0, (size_t)nroots);
  for (int i = 0; i < n; ++i) {
    const uint8_t fb = (uint8_t)(data[i] ^ par[0]);
    if (fb) {
      const int lf = kGf.log[fb];
      for (int j = 0; j + 1 < nroots; ++j)
        par[j] = (uint8_t)(par[j + 1] ^ (g[j + 1] ? kGf.exp[lf + kGf.log[g[j + 1]]] : 0));
      par[nroots - 1] = g[nroots] ? kGf.exp[lf + kGf.log[g[nroots]]] : 0;
    } else {
      memmove(par, par + 1, (size_t)nroots - 1);
      par[nroots - 1] = 0;
    }
  }
}

// v * alpha^i for every syndrome index i: the syndromes of a codeword are then nroots independent table chains
struct MulAlpha {
  uint8_t t[kMaxRoots][256];
};

constexpr MulAlpha make_mul_alpha() {
  MulAlpha m{};
  for (int i = 0; i < kMaxRoots; ++i)
    for (int v = 1; v < 256; ++v) m.t[i][v] = kGf.exp[kGf.log[v] + i];
  return m;
}

constexpr MulAlpha kMulAlpha = make_mul_alpha();

// S_i = c(alpha^i), c[0] the coefficient of x^(n-1) (Horner, all i side by side). Returns whether any syndrome
// is nonzero.
bool syndromes(const uint8_t* c, int n, int nroots, uint8_t* s) {
  memset(s, 0, (size_t)nroots);
  for (int j = 0; j < n; ++j) {
    const uint8_t v = c[j];
    for (int i = 0; i < nroots; ++i) s[i] = (uint8_t)(kMulAlpha.t[i][s[i]] ^ v);
  }
  uint8_t any = 0;
  for (int i = 0; i < nroots; ++i) any |= s[i];
  return any != 0;
}

// Corrects c[n] (data and parity, n <= 255) in place. Returns the number of bytes corrected, or -1 when the word
// is uncorrectable (c is then left as it came): the locator's degree exceeds t, differs from the number of roots
// found, a root lies outside the shortened length, or the corrected word is no codeword after all.
int rs_correct(uint8_t* c, int n, int nroots) {
  uint8_t s[kMaxRoots];
  if (!syndromes(c, n, nroots, s)) return 0;
  const int t = nroots / 2;
  // Berlekamp-Massey: lam(x) = 1 + lam_1 x + ... with S_r + sum_{i=1}^{L} lam_i S_{r-i} = 0
  uint8_t lam[kMaxRoots + 1] = {1}, prev[kMaxRoots + 1] = {1}, tmp[kMaxRoots + 1];
  int L = 0, m = 1;
  uint8_t b = 1;
  for (int r = 0; r < nroots; ++r) {
    uint8_t d = s[r];
    for (int i = 1; i <= L; ++i) d ^= gmul(lam[i], s[r - i]);
    if (d == 0) {
      ++m;
      continue;
    }
    const uint8_t f = gdiv(d, b);
    if (2 * L <= r) {
      memcpy(tmp, lam, sizeof(lam));
      for (int i = 0; i + m <= nroots; ++i) lam[i + m] ^= gmul(f, prev[i]);
      L = r + 1 - L;
      memcpy(prev, tmp, sizeof(lam));
      b = d;
      m = 1;
    } else {
      for (int i = 0; i + m <= nroots; ++i) lam[i + m] ^= gmul(f, prev[i]);
      ++m;
    }
  }
  int deg = nroots;
  while (deg > 0 && lam[deg] == 0) --deg;
  if (L > t || deg != L) return -1;
  // Chien search over the whole field: position p (the coefficient of x^p) is in error when lam(alpha^-p) = 0
  int pos[kMaxRoots / 2], found = 0;
  int lg[kMaxRoots / 2 + 1];  // log of the term lam_i alpha^(-i p), stepped from p to p + 1 by -i (mod 255)
  for (int i = 1; i <= L; ++i) lg[i] = lam[i] ? kGf.log[lam[i]] : -1;
  for (int p = 0; p < 255; ++p) {
    uint8_t v = 1;
    for (int i = 1; i <= L; ++i) {
      if (lg[i] < 0) continue;
      v ^= kGf.exp[lg[i]];
      lg[i] -= i;
      if (lg[i] < 0) lg[i] += 255;
    }
    if (v == 0) {
      if (p >= n || found == L) return -1;  // outside the shortened length
      pos[found++] = p;
    }
  }
  if (found != L) return -1;
  // Forney: omega = S(x) lam(x) mod x^nroots; e = X omega(X^-1) / lam'(X^-1) (first root alpha^0)
  uint8_t om[kMaxRoots];
  for (int i = 0; i < nroots; ++i) {
    uint8_t v = 0;
    for (int j = 0; j <= i && j <= L; ++j) v ^= gmul(lam[j], s[i - j]);
    om[i] = v;
  }
  uint8_t val[kMaxRoots / 2];
  for (int k = 0; k < L; ++k) {
    const int xi = (255 - pos[k]) % 255;  // log of X^-1
    uint8_t num = 0, den = 0;
    for (int i = 0; i < nroots; ++i)
      if (om[i]) num ^= kGf.exp[(kGf.log[om[i]] + i * xi) % 255];
    for (int i = 1; i <= L; i += 2)
      if (lam[i]) den ^= kGf.exp[(kGf.log[lam[i]] + (i - 1) * xi) % 255];
    if (den == 0 || num == 0) return -1;
    val[k] = gmul(kGf.exp[pos[k]], gdiv(num, den));
  }
  for (int k = 0; k < L; ++k) c[n - 1 - pos[k]] ^= val[k];
  if (syndromes(c, n, nroots, s)) {  // belt and braces: never hand back a word that is no codeword
    for (int k = 0; k < L; ++k) c[n - 1 - pos[k]] ^= val[k];
    return -1;
  }
  return L;
}

// Where byte j of codeword c of a group goes: `g` codewords, all of `full` bytes but the last of `last` <= full.
inline size_t interleaved(int j, int c, int g, int last) {
  return j < last ? (size_t)j * g + c : (size_t)last * g + (size_t)(j - last) * (g - 1) + c;
}

struct Layout {
  size_t k, ncw, total;
};

// false when the size does not fit size_t
bool layout(size_t n, int nroots, Layout* l) {
  l->k = (size_t)(255 - nroots);
  l->ncw = n / l->k + (n % l->k ? 1 : 0);
  const size_t parity = l->ncw * (size_t)nroots;
  if (n > SIZE_MAX - kHdrLen || parity > SIZE_MAX - kHdrLen - n) return false;
  l->total = kHdrLen + n + parity;
  return true;
}

}  // namespace

extern "C" {

uint32_t rdeic_crc32(const uint8_t* data, size_t n) { return (data || n == 0) ? crc32(data, n) : 0; }

int rdeic_rs_encode(const uint8_t* data, int32_t n, int32_t nroots, uint8_t* parity_out) {
  if (!data || !parity_out || !roots_ok(nroots) || n < 1 || n > 255 - nroots) return RDEIC_EINVAL;
  uint8_t g[kMaxRoots + 1];
  generator(nroots, g);
  rs_parity(data, n, nroots, g, parity_out);
  return RDEIC_OK;
}

int rdeic_rs_decode(uint8_t* codeword, int32_t n_total, int32_t nroots, int32_t* corrected_out) {
  if (corrected_out) *corrected_out = 0;
  if (!codeword || !roots_ok(nroots) || n_total <= nroots || n_total > 255) return RDEIC_EINVAL;
  const int r = rs_correct(codeword, n_total, nroots);
  if (r < 0) return RDEIC_EBADMSG;
  if (corrected_out) *corrected_out = r;
  return RDEIC_OK;
}

size_t rdeic_fec_encoded_size(size_t n, int32_t nroots, int32_t depth) {
  Layout l;
  if (!roots_ok(nroots) || depth < 1 || depth > 255 || n > 0xffffffffull || !layout(n, nroots, &l)) return 0;
  return l.total;
}

int rdeic_fec_encode(const uint8_t* src, size_t n, int32_t nroots, int32_t depth, uint8_t* dst, size_t cap) {
  Layout l;
  if ((!src && n) || !dst || !roots_ok(nroots) || depth < 1 || depth > 255 || n > 0xffffffffull ||
      !layout(n, nroots, &l))
    return RDEIC_EINVAL;
  if (cap < l.total) return RDEIC_ENOSPC;
  uint8_t g[kMaxRoots + 1];
  const uint32_t crc = crc32(src, n);
  const uint8_t hdr[kHdrData] = {'R', 'D', 'F', '1', (uint8_t)nroots, (uint8_t)depth,
                                 (uint8_t)(n >> 24), (uint8_t)(n >> 16), (uint8_t)(n >> 8), (uint8_t)n,
                                 (uint8_t)(crc >> 24), (uint8_t)(crc >> 16), (uint8_t)(crc >> 8), (uint8_t)crc};
  memcpy(dst, hdr, kHdrData);
  generator(kHdrRoots, g);
  rs_parity(hdr, kHdrData, kHdrRoots, g, dst + kHdrData);
  generator(nroots, g);
  uint8_t* out = dst + kHdrLen;
  uint8_t par[kMaxRoots];
  for (size_t first = 0; first < l.ncw; first += (size_t)depth) {
    const int grp = (int)(l.ncw - first < (size_t)depth ? l.ncw - first : (size_t)depth);
    const size_t gdata = n - first * l.k < (size_t)grp * l.k ? n - first * l.k : (size_t)grp * l.k;
    const int last = (int)(gdata - (size_t)(grp - 1) * l.k) + nroots;  // the group's last codeword; the others have 255
    for (int c = 0; c < grp; ++c) {
      const uint8_t* blk = src + (first + c) * l.k;
      const int len = c == grp - 1 ? last - nroots : (int)l.k;
      rs_parity(blk, len, nroots, g, par);
      for (int j = 0; j < len; ++j) out[interleaved(j, c, grp, last)] = blk[j];
      for (int j = 0; j < nroots; ++j) out[interleaved(len + j, c, grp, last)] = par[j];
    }
    out += gdata + (size_t)grp * nroots;
  }
  return RDEIC_OK;
}

int rdeic_fec_decode(const uint8_t* src, size_t n, uint8_t* dst, size_t cap, size_t* out_len,
                     rdeic_fec_stats* stats) {
  if (out_len) *out_len = 0;
  if (stats) stats->codewords = stats->corrected = stats->uncorrectable = 0;
  if ((!src && n) || (!dst && cap) || !out_len) return RDEIC_EINVAL;
  if (n < (size_t)kHdrLen) return RDEIC_EBADMSG;
  rdeic_fec_stats st = {1, 0, 0};
  uint8_t hdr[kHdrLen];
  memcpy(hdr, src, kHdrLen);
  const int hc = rs_correct(hdr, kHdrLen, kHdrRoots);
  if (hc < 0) {
    st.uncorrectable = 1;
    if (stats) *stats = st;
    return RDEIC_EBADMSG;
  }
  st.corrected = hc;
  if (stats) *stats = st;
  const int nroots = hdr[4], depth = hdr[5];
  const size_t plen = ((size_t)hdr[6] << 24) | ((size_t)hdr[7] << 16) | ((size_t)hdr[8] << 8) | hdr[9];
  const uint32_t crc = ((uint32_t)hdr[10] << 24) | ((uint32_t)hdr[11] << 16) | ((uint32_t)hdr[12] << 8) | hdr[13];
  Layout l;
  if (memcmp(hdr, "RDF1", 4) != 0 || !roots_ok(nroots) || depth < 1 || !layout(plen, nroots, &l) || l.total != n)
    return RDEIC_EBADMSG;  // the announced length is now known to fit the input: plen < n
  if (cap < plen) return RDEIC_ENOSPC;
  const uint8_t* in = src + kHdrLen;
  uint8_t cw[255];
  for (size_t first = 0; first < l.ncw; first += (size_t)depth) {
    const int grp = (int)(l.ncw - first < (size_t)depth ? l.ncw - first : (size_t)depth);
    const size_t gdata = plen - first * l.k < (size_t)grp * l.k ? plen - first * l.k : (size_t)grp * l.k;
    const int last = (int)(gdata - (size_t)(grp - 1) * l.k) + nroots;
    for (int c = 0; c < grp; ++c) {
      const int tot = c == grp - 1 ? last : 255;
      for (int j = 0; j < tot; ++j) cw[j] = in[interleaved(j, c, grp, last)];
      const int r = rs_correct(cw, tot, nroots);
      ++st.codewords;
      if (r < 0)
        ++st.uncorrectable;
      else
        st.corrected += r;
      memcpy(dst + (first + c) * l.k, cw, (size_t)(tot - nroots));
    }
    in += gdata + (size_t)grp * nroots;
  }
  if (stats) *stats = st;
  if (st.uncorrectable || crc32(dst, plen) != crc) return RDEIC_EBADMSG;
  *out_len = plen;
  return RDEIC_OK;
}

}  // extern "C"
