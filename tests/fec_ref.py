"""The protected-stream format restated in plain Python from its description (DESIGN "Protected streams"), not from
rdeic_amd/csrc/fec.cpp: log / antilog tables of GF(2^8) with the polynomial 0x11d and alpha = 2, the generator
prod_{i<nroots} (x - alpha^i), parity by polynomial long division, the round-robin interleave, zlib's CRC-32.
It encodes, and it says from the byte positions of a corruption alone whether a stream is recoverable (no codeword
with more than nroots / 2 corrupted bytes); it holds no decoder."""
import struct
import zlib

EXP = [0] * 510
LOG = [0] * 256
_x = 1
for _i in range(255):
    EXP[_i] = EXP[_i + 255] = _x
    LOG[_x] = _i
    _x <<= 1
    if _x & 0x100:
        _x ^= 0x11d

HEADER_ROOTS, HEADER_BYTES = 32, 46


def mul(a, b):
    return EXP[LOG[a] + LOG[b]] if a and b else 0


def generator(nroots):
    """coefficients from x^nroots down to x^0"""
    g = [1]
    for i in range(nroots):
        root = EXP[i]
        g = [a ^ b for a, b in zip(g + [0], [0] + [mul(c, root) for c in g])]  # g * x + g * alpha^i
    return g


def parity(data, nroots):
    """remainder of data(x) * x^nroots divided by the generator, highest degree first"""
    g = generator(nroots)
    rem = list(data) + [0] * nroots
    for i in range(len(data)):
        lead = rem[i]
        if lead:
            for j in range(1, nroots + 1):
                rem[i + j] ^= mul(g[j], lead)
    return bytes(rem[len(data):])


def encoded_size(n, nroots):
    return HEADER_BYTES + n + nroots * (-(-n // (255 - nroots)))


def codeword_positions(n, nroots, depth):
    """For every codeword of the stream, the header's first: the stream offsets of its bytes, in codeword order."""
    k = 255 - nroots
    lens = [min(k, n - s) + nroots for s in range(0, n, k)]
    out = [list(range(HEADER_BYTES))]
    at = HEADER_BYTES
    for first in range(0, len(lens), depth):
        group = lens[first:first + depth]
        where = [[] for _ in group]
        for j in range(max(group)):
            for c, ln in enumerate(group):
                if j < ln:
                    where[c].append(at)
                    at += 1
        out += where
    assert at == encoded_size(n, nroots)
    return out


def protect(payload, nroots, depth):
    payload = bytes(payload)
    head = b"RDF1" + bytes([nroots, depth]) + struct.pack(">II", len(payload), zlib.crc32(payload) & 0xffffffff)
    out = bytearray(encoded_size(len(payload), nroots))
    out[:HEADER_BYTES] = head + parity(head, HEADER_ROOTS)
    k = 255 - nroots
    blocks = [payload[s:s + k] for s in range(0, len(payload), k)]
    for block, where in zip(blocks, codeword_positions(len(payload), nroots, depth)[1:]):
        for pos, byte in zip(where, block + parity(block, nroots)):
            out[pos] = byte
    return bytes(out)


def errors_per_codeword(clean, corrupted, nroots, depth, n):
    """the number of differing bytes in each codeword (the header's first) of two streams of one length"""
    assert len(clean) == len(corrupted) == encoded_size(n, nroots)
    return [sum(clean[p] != corrupted[p] for p in where) for where in codeword_positions(n, nroots, depth)]


def recoverable(clean, corrupted, nroots, depth, n):
    """Bounded-distance decoding repairs a stream exactly when no codeword holds more errors than it corrects: 16 for
    the header, nroots / 2 for the others. (Past that a decoder fails or, rarely, miscorrects; the CRC catches that.)"""
    if len(clean) != len(corrupted):
        return False
    errs = errors_per_codeword(clean, corrupted, nroots, depth, n)
    return errs[0] <= HEADER_ROOTS // 2 and all(e <= nroots // 2 for e in errs[1:])
