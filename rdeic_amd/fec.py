"""Protected streams: Reed-Solomon + CRC-32 around a bitstream body (rdeic_amd/csrc/fec.cpp, DESIGN "Protected
streams"). The reference's fault-robustness study ends on "error correction should be applied at the bitstream level
using FEC codes"; this is that step. Host code: a body of 2.5-129 KB costs far less here than one relay decode.

    params = parse_fec("rs:32:4")        # 32 parity bytes per codeword (16 byte errors repaired), interleave depth 4
    data = protect(body, params)         # 46 + len + 32 * ceil(len / 223) bytes
    body, stats = recover(data)          # FecError (a BitstreamError) when the stream cannot be repaired or checked

Protection is never detected from the bytes: a magic number is no evidence on a noisy channel, so whoever decodes
says whether the stream is protected.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Tuple, Union

from . import _lib

HEADER_BYTES = 46


@dataclass(frozen=True)
class FecParams:
    """nroots parity bytes per codeword (even, 2..64: nroots / 2 byte errors repaired per codeword of at most 255
    bytes); codewords interleaved `depth` at a time (1..255: a burst of depth * nroots / 2 bytes is repaired)."""
    nroots: int
    depth: int = 1

    def __post_init__(self):
        if not (isinstance(self.nroots, int) and 2 <= self.nroots <= 64 and self.nroots % 2 == 0):
            raise ValueError(f"fec nroots {self.nroots!r}: an even number from 2 to 64")
        if not (isinstance(self.depth, int) and 1 <= self.depth <= 255):
            raise ValueError(f"fec depth {self.depth!r}: a number from 1 to 255")

    @property
    def spec(self) -> str:
        return f"rs:{self.nroots}:{self.depth}"

    def encoded_size(self, n: int) -> int:
        """46 + n + nroots * ceil(n / (255 - nroots))"""
        k = 255 - self.nroots
        return HEADER_BYTES + n + self.nroots * (-(-n // k))


@dataclass(frozen=True)
class FecStats:
    """codewords looked at (the header's included), bytes corrected, codewords that could not be corrected"""
    codewords: int
    corrected: int
    uncorrectable: int


class FecError(_lib.BitstreamError):
    """A protected stream that was not recovered. A decode failure like any other (BitstreamError); its text holds
    counts only, so two runs over the same bytes give the same text."""

    def __init__(self, code: int, stats: FecStats, nbytes: int):
        if stats.uncorrectable and stats.codewords == 1:
            why = "the header codeword is uncorrectable"
        elif stats.uncorrectable:
            why = f"{stats.uncorrectable} of {stats.codewords} codewords uncorrectable"
        elif nbytes < HEADER_BYTES:
            why = f"{nbytes} bytes are fewer than the {HEADER_BYTES} of the header codeword"
        else:
            why = "the header, the stream's length and the payload's CRC-32 do not agree"
        RuntimeError.__init__(self, f"rdeic_fec_decode failed: {code} ({why})")
        self.code = code
        self.stats = stats


def parse_fec(spec: str) -> FecParams:
    """"rs:NROOTS[:DEPTH]" -> FecParams (depth 1 by default). ValueError with the reason for anything else."""
    parts = spec.strip().split(":") if isinstance(spec, str) else []
    if len(parts) not in (2, 3) or parts[0] != "rs":
        raise ValueError(f"fec spec {spec!r}: expected rs:NROOTS[:DEPTH], e.g. rs:32 or rs:32:4")
    try:
        nums = [int(p) for p in parts[1:]]
    except ValueError:
        raise ValueError(f"fec spec {spec!r}: NROOTS and DEPTH are whole numbers (rs:NROOTS[:DEPTH])") from None
    try:
        return FecParams(*nums)
    except ValueError as e:
        raise ValueError(f"fec spec {spec!r}: {e}") from None


def as_params(fec: Union[None, str, FecParams]) -> Optional[FecParams]:
    """None, a spec string or FecParams -> None or FecParams (what the fec= arguments of the codec accept)."""
    if fec is None or isinstance(fec, FecParams):
        return fec
    return parse_fec(fec)


def _ro(data: bytes):
    return C.cast(C.c_char_p(data), C.c_void_p)


def crc32(data: bytes) -> int:
    data = bytes(data)
    return int(_lib.load().rdeic_crc32(_ro(data), len(data)))


def rs_encode(data: bytes, nroots: int) -> bytes:
    """The nroots parity bytes of one block of at most 255 - nroots bytes."""
    data = bytes(data)
    out = C.create_string_buffer(max(1, int(nroots)))
    _lib.check("rdeic_rs_encode", _lib.load().rdeic_rs_encode(_ro(data), len(data), nroots, out))
    return out.raw[:nroots]


def rs_decode(codeword: bytes, nroots: int) -> Tuple[bytes, int]:
    """One codeword (data then parity) -> (the corrected codeword, bytes corrected). BitstreamError when the word
    is uncorrectable."""
    buf = C.create_string_buffer(bytes(codeword), max(1, len(codeword)))
    n = C.c_int32(0)
    _lib.check("rdeic_rs_decode", _lib.load().rdeic_rs_decode(buf, len(codeword), nroots, C.byref(n)))
    return buf.raw[:len(codeword)], int(n.value)


def protect(body: bytes, params: Union[str, FecParams]) -> bytes:
    params = as_params(params)
    if params is None:
        raise ValueError("protect needs fec parameters")
    body = bytes(body)
    lib = _lib.load()
    size = int(lib.rdeic_fec_encoded_size(len(body), params.nroots, params.depth))
    if size == 0:
        raise ValueError(f"a payload of {len(body)} bytes cannot be protected")
    out = C.create_string_buffer(size)
    _lib.check("rdeic_fec_encode", lib.rdeic_fec_encode(_ro(body), len(body), params.nroots, params.depth, out, size))
    return out.raw


def recover_status(data: bytes) -> Tuple[int, bytes, FecStats]:
    """rdeic_fec_decode as it is: (status, payload, stats); the payload is b"" unless the status is 0."""
    data = bytes(data)
    cap = max(1, len(data))
    out = C.create_string_buffer(cap)
    n = C.c_size_t(0)
    st = _lib.FecStatsC()
    rc = int(_lib.load().rdeic_fec_decode(_ro(data), len(data), out, cap, C.byref(n), C.byref(st)))
    stats = FecStats(int(st.codewords), int(st.corrected), int(st.uncorrectable))
    return rc, (out.raw[:n.value] if rc == 0 else b""), stats


def recover(data: bytes) -> Tuple[bytes, FecStats]:
    rc, body, stats = recover_status(data)
    if rc != 0:
        raise FecError(rc, stats, len(data))
    return body, stats
