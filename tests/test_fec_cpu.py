"""Protected streams on the host (rdeic_amd/csrc/fec.cpp through rdeic_amd/fec.py): a known answer from outside the
project, the library against the plain-Python restatement of the format (tests/fec_ref.py) byte for byte, correction
at exactly t errors in every codeword and refusal at t + 1, the no-silent-wrong-output property over seeded random
corruption, bursts against the interleave depth, hostile input, and the codeword failure rate against the binomial
tail."""
import math
import struct

import numpy as np
import pytest

from rdeic_amd import _lib, fec
from tests import fec_ref

EBADMSG = -74


def _payload(n, seed):
    return np.random.default_rng(seed).integers(0, 256, size=n, dtype=np.uint8).tobytes()


def _smash(data, positions, rng):
    """XOR a nonzero random byte into every position: each one is a byte error for certain."""
    out = bytearray(data)
    for p in positions:
        out[p] ^= int(rng.integers(1, 256))
    return bytes(out)


# ------------------------------------------------------------------ 1. known answers
def test_known_answer_qr_code_block_and_crc_check_value():
    # the worked example of the QR-code literature (version 1-M: 16 data and 10 error-correction codewords); it pins
    # the field polynomial, the generator's roots and the byte order against something outside this project
    data = bytes([32, 91, 11, 120, 209, 114, 220, 77, 67, 64, 236, 17, 236, 17, 236, 17])
    want = bytes([196, 35, 39, 119, 235, 215, 231, 226, 93, 23])
    assert fec.rs_encode(data, 10) == want
    assert fec_ref.parity(data, 10) == want
    assert fec.crc32(b"123456789") == 0xCBF43926 and fec.crc32(b"") == 0
    # block level: 5 errors corrected in place, 6 refused
    rng = np.random.default_rng(3)
    word = data + want
    fixed, n = fec.rs_decode(_smash(word, rng.choice(26, 5, replace=False), rng), 10)
    assert fixed == word and n == 5
    assert fec.rs_decode(word, 10) == (word, 0)
    with pytest.raises(_lib.BitstreamError):
        fec.rs_decode(_smash(word, rng.choice(26, 6, replace=False), rng), 10)


# ------------------------------------------------------------------ 2. the library is the restatement
@pytest.mark.parametrize("nroots", [2, 16, 32, 64])
def test_encoder_equals_the_restatement_byte_for_byte(nroots):
    k = 255 - nroots
    for depth in (1, 4, 255):
        for n in (0, 1, k - 1, k, k + 1, 3 * k + 7):
            body = _payload(n, 1000 * nroots + n)
            params = fec.FecParams(nroots, depth)
            got = fec.protect(body, params)
            assert len(got) == 46 + n + nroots * math.ceil(n / k) == params.encoded_size(n)
            assert len(got) == _lib.load().rdeic_fec_encoded_size(n, nroots, depth)
            assert got == fec_ref.protect(body, nroots, depth), (nroots, depth, n)
            back, stats = fec.recover(got)
            assert back == body and stats == fec.FecStats(1 + math.ceil(n / k), 0, 0)
    assert fec.protect(b"", fec.FecParams(nroots, 1))[:6] == b"RDF1" + bytes([nroots, 1])


# ------------------------------------------------------------------ 3. / 4. t errors, t + 1 errors
CASES = [(2, 1, 3), (2, 255, 4), (16, 4, 9), (32, 4, 3), (32, 4, 10), (64, 1, 3), (64, 255, 5)]  # nroots, depth, blocks


@pytest.mark.parametrize("nroots,depth,blocks", CASES)
def test_t_errors_in_every_codeword_are_repaired(nroots, depth, blocks):
    n = (blocks - 1) * (255 - nroots) + 7  # the last codeword is a short one
    body = _payload(n, 7 * nroots + depth)
    clean = fec.protect(body, fec.FecParams(nroots, depth))
    rng = np.random.default_rng(nroots * 1000 + depth)
    where = fec_ref.codeword_positions(n, nroots, depth)
    assert len(where) == blocks + 1
    hits = list(rng.choice(where[0], 16, replace=False))  # the header codeword: 16 of its 46 bytes
    for cw in where[1:]:
        hits += list(rng.choice(cw, nroots // 2, replace=False))
    bad = _smash(clean, hits, rng)
    status, back, stats = fec.recover_status(bad)
    assert status == 0 and back == body
    assert stats == fec.FecStats(blocks + 1, len(hits), 0) and len(hits) == 16 + blocks * (nroots // 2)
    assert fec_ref.recoverable(clean, bad, nroots, depth, n)


@pytest.mark.parametrize("nroots,depth,blocks", CASES)
def test_one_codeword_with_t_plus_one_errors_is_refused(nroots, depth, blocks):
    n = (blocks - 1) * (255 - nroots) + 7
    body = _payload(n, 11 * nroots + depth)
    clean = fec.protect(body, fec.FecParams(nroots, depth))
    where = fec_ref.codeword_positions(n, nroots, depth)
    rng = np.random.default_rng(nroots * 77 + depth)
    for victim in range(len(where)):  # the header (17 errors), every full codeword, the short one
        t = 16 if victim == 0 else nroots // 2
        bad = _smash(clean, rng.choice(where[victim], t + 1, replace=False), rng)
        # (at nroots 2 two errors often look like one error elsewhere: the word is "corrected" to another codeword
        # and it is the CRC that refuses the stream. The status is what the contract is about.)
        status, back, stats = fec.recover_status(bad)
        assert status == EBADMSG and back == b"", (victim, stats)
        assert not fec_ref.recoverable(clean, bad, nroots, depth, n)
        with pytest.raises(fec.FecError) as e:
            fec.recover(bad)
        assert isinstance(e.value, _lib.BitstreamError) and isinstance(e.value, ValueError)
        assert e.value.code == EBADMSG and "0x" not in str(e.value)
        if nroots >= 16:
            assert stats.uncorrectable == 1 and (stats.codewords == 1) == (victim == 0)


# ------------------------------------------------------------------ 5. no silent wrong output
def test_status_zero_means_the_original_bytes():
    rng = np.random.default_rng(2024)
    rates = [1e-4, 1e-3, 3e-3, 1e-2, 2e-2, 5e-2, 0.2]
    streams = []
    for nroots, depth, n in [(2, 1, 500), (2, 3, 300), (4, 2, 900), (16, 1, 700), (16, 4, 1500), (32, 4, 1200),
                             (32, 1, 223), (64, 2, 600)]:
        body = _payload(n, n + nroots)
        streams.append((body, np.frombuffer(fec.protect(body, fec.FecParams(nroots, depth)), dtype=np.uint8)))
    trials = ok = refused = 0
    for trial in range(2400):
        body, clean = streams[trial % len(streams)]
        p = rates[(trial // len(streams)) % len(rates)]
        flips = rng.random((clean.size, 8)) < p
        bad = clean ^ np.packbits(flips, axis=1, bitorder="little")[:, 0]
        if trial % 5 == 4:  # and a stretch of random bytes on top
            a = int(rng.integers(0, clean.size))
            b = min(clean.size, a + int(rng.integers(1, 80)))
            bad[a:b] = rng.integers(0, 256, size=b - a, dtype=np.uint8)
        status, back, stats = fec.recover_status(bad.tobytes())
        trials += 1
        if status == 0:
            assert back == body, (trial, p, stats)  # the property
            ok += 1
        else:
            assert status == EBADMSG and back == b""
            refused += 1
    print(f"\n[fec safety] {trials} trials: {ok} recovered exactly, {refused} refused, 0 wrong")
    assert trials >= 2000 and ok > 300 and refused > 300  # both outcomes are well represented


# ------------------------------------------------------------------ 6. bursts
@pytest.mark.parametrize("depth", [4, 16])
def test_burst_of_depth_times_t_bytes_is_repaired_and_is_not_at_depth_one(depth):
    nroots, t = 32, 16
    n = 2 * depth * (255 - nroots)  # two full groups
    body = _payload(n, depth)
    clean = fec.protect(body, fec.FecParams(nroots, depth))
    burst = depth * t
    for start in (46, 46 + 37, 46 + depth * 255 - burst):  # group-aligned, odd, ending with the first group
        bad = _smash(clean, range(start, start + burst), np.random.default_rng(start))
        status, back, stats = fec.recover_status(bad)
        assert status == 0 and back == body and stats.corrected == burst and stats.uncorrectable == 0, start
        errs = fec_ref.errors_per_codeword(clean, bad, nroots, depth, n)
        assert max(errs) <= math.ceil(burst / depth) == t
    one = fec.protect(body, fec.FecParams(nroots, 1))
    bad = _smash(one, range(46 + 37, 46 + 37 + burst), np.random.default_rng(5))
    status, back, stats = fec.recover_status(bad)
    assert burst > t and status == EBADMSG and stats.uncorrectable >= 1


# ------------------------------------------------------------------ 7. hostile input
def test_hostile_input_gives_a_status():
    params = fec.FecParams(32, 4)
    body = _payload(1000, 9)
    clean = fec.protect(body, params)
    assert fec.recover_status(b"")[0] == EBADMSG
    for cut in (1, 45, 46, 47, 300, len(clean) - 1):  # the header alone (46) announces 1000 bytes that are not there
        status, back, stats = fec.recover_status(clean[:cut])
        assert status == EBADMSG and back == b"", cut
    assert fec.recover_status(clean + b"\x00")[0] == EBADMSG
    # a valid header codeword that announces more than the buffer holds, up to the largest length it can state
    for announced in (1001, 5000, 2 ** 31, 2 ** 32 - 1):
        head = clean[:6] + struct.pack(">I", announced) + clean[10:14]
        lying = head + fec_ref.parity(head, 32) + clean[46:]
        assert fec.recover_status(lying)[0] == EBADMSG, announced
    # corrected headers that state an impossible code: odd roots, too many, depth 0, another magic
    for patch in ((4, 31), (4, 66), (4, 0), (5, 0), (0, ord("X"))):
        head = bytearray(clean[:14])
        head[patch[0]] = patch[1]
        assert fec.recover_status(bytes(head) + fec_ref.parity(head, 32) + clean[46:])[0] == EBADMSG, patch
    # an empty payload is the 46 header bytes alone, and that is a stream
    empty = fec.protect(b"", params)
    assert len(empty) == 46 and fec.recover(empty) == (b"", fec.FecStats(1, 0, 0))
    # the calls' own arguments
    lib = _lib.load()
    assert lib.rdeic_fec_encoded_size(10, 3, 1) == 0 and lib.rdeic_fec_encoded_size(10, 32, 256) == 0
    assert lib.rdeic_fec_decode(None, 10, None, 0, None, None) == -22
    for bad in ((31, 1), (66, 1), (0, 1), (32, 0), (32, 256)):
        with pytest.raises(ValueError):
            fec.FecParams(*bad)
    with pytest.raises(fec.FecError, match="fewer than the 46"):
        fec.recover(b"abc")


# ------------------------------------------------------------------ 8. agreement with theory
def _tail(nroots, p):
    """P(Bin(255, q) > t): a full codeword holds more byte errors than the code corrects"""
    q, t = 1.0 - (1.0 - p) ** 8, nroots // 2
    return 1.0 - sum(math.comb(255, j) * q ** j * (1.0 - q) ** (255 - j) for j in range(t + 1))


def test_the_tails_are_the_ones_the_design_quotes():
    assert abs(_tail(32, 0.005) - 2.5e-2) < 0.1e-2 and abs(_tail(32, 0.01) - 0.77) < 0.01
    assert abs(_tail(64, 0.01) - 2.6e-3) < 0.1e-3 and abs(_tail(64, 0.02) - 0.84) < 0.01


@pytest.mark.parametrize("nroots,p", [(32, 0.005), (32, 0.01), (64, 0.02)])
def test_codeword_failure_rate_is_the_binomial_tail(nroots, p):
    codewords = 4000
    tail = _tail(nroots, p)
    assert 0.01 < tail < 0.99
    n = codewords * (255 - nroots)  # full codewords only
    body = _payload(n, nroots)
    clean = np.frombuffer(fec.protect(body, fec.FecParams(nroots, 4)), dtype=np.uint8)
    rng = np.random.default_rng(int(p * 1e4) + nroots)
    flips = rng.random((clean.size, 8)) < p  # i.i.d. bit flips, not the exact-count corruptor
    flips[:46] = False  # the header stays clean: an uncorrectable header would end the count at one codeword
    bad = clean ^ np.packbits(flips, axis=1, bitorder="little")[:, 0]
    status, _, stats = fec.recover_status(bad.tobytes())
    assert status == EBADMSG and stats.codewords == codewords + 1
    got = stats.uncorrectable / codewords
    sd = math.sqrt(tail * (1.0 - tail) / codewords)
    print(f"\n[fec theory] rs:{nroots} p={p}: failed {got:.4f} of {codewords} codewords, tail {tail:.4f}, "
          f"{(got - tail) / sd:+.2f} sd")
    assert abs(got - tail) <= 4.0 * sd
