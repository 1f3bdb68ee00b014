"""CLIP byte-pair tokenizer: open_clip's SimpleTokenizer / tokenize restated (the reference calls
open_clip.tokenize in FrozenOpenCLIPEmbedder.forward, ldm/modules/encoders/modules.py:210-214).

    tokenize(texts, vocab_path=None, context=77) -> int64 [B, context]

SOT 49406, EOT 49407, zero padding, truncation to `context` with EOT forced last; text is html-unescaped,
whitespace-cleaned and lower-cased, split by the CLIP pattern, mapped through the byte-to-unicode table and merged
by the ranks of `bpe_simple_vocab_16e6.txt.gz` (lines 1 : 49152 - 256 - 2 + 1).

The vocabulary file is not shipped: pass its path (`vocab_path`, the CLIs' --clip_vocab, or the environment
variable RDEIC_CLIP_VOCAB). The empty text needs none: [49406, 49407, 0, ...].

Differences from open_clip, and status: open_clip cleans text with ftfy.fix_text before html.unescape; ftfy is
not a dependency here, so only html.unescape (twice, as open_clip) is applied. Text that ftfy would repair
(mojibake, odd unicode forms) therefore tokenizes differently. Parity with open_clip's tokenizer is UNPINNED:
no fixture of its output exists in this repository.
"""
from __future__ import annotations

import gzip
import html
import os
from functools import lru_cache
from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch

SOT, EOT = 49406, 49407
VOCAB_FILE = "bpe_simple_vocab_16e6.txt.gz"
VOCAB_ENV = "RDEIC_CLIP_VOCAB"
_PATTERN = r"""<\|startoftext\|>|<\|endoftext\|>|'s|'t|'re|'ve|'m|'ll|'d|[\p{L}]+|[\p{N}]|[^\s\p{L}\p{N}]+"""


@lru_cache()
def bytes_to_unicode() -> Dict[int, str]:
    """Byte -> printable unicode character (the GPT-2 table): printable latin-1 bytes map to themselves, the
    rest to 256 + n in order."""
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(ord("\xa1"), ord("\xac") + 1)) + \
        list(range(ord("\xae"), ord("\xff") + 1))
    cs = bs[:]
    n = 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return dict(zip(bs, (chr(c) for c in cs)))


def clean(text: str) -> str:
    text = html.unescape(html.unescape(text)).strip()
    return " ".join(text.split()).strip().lower()


class SimpleTokenizer:
    def __init__(self, vocab_path: str):
        import regex  # \p{L} / \p{N} classes: the stdlib `re` has none
        with gzip.open(vocab_path) as f:
            lines = f.read().decode("utf-8").split("\n")
        merges = [tuple(m.split()) for m in lines[1:49152 - 256 - 2 + 1]]
        merges = [m for m in merges if len(m) == 2]  # a short (toy) file ends before the slice does
        vocab = list(bytes_to_unicode().values())
        vocab = vocab + [v + "</w>" for v in vocab]
        vocab += ["".join(m) for m in merges]
        vocab += ["<|startoftext|>", "<|endoftext|>"]
        self.encoder = dict(zip(vocab, range(len(vocab))))
        self.ranks = dict(zip(merges, range(len(merges))))
        self.byte_encoder = bytes_to_unicode()
        self.cache = {"<|startoftext|>": "<|startoftext|>", "<|endoftext|>": "<|endoftext|>"}
        self.pat = regex.compile(_PATTERN, regex.IGNORECASE)

    def bpe(self, token: str) -> str:
        if token in self.cache:
            return self.cache[token]
        word: Tuple[str, ...] = tuple(token[:-1]) + (token[-1] + "</w>",)
        while len(word) > 1:
            pairs = set(zip(word, word[1:]))
            best = min(pairs, key=lambda p: self.ranks.get(p, float("inf")))
            if best not in self.ranks:
                break
            first, second = best
            out: List[str] = []
            i = 0
            while i < len(word):
                if i + 1 < len(word) and word[i] == first and word[i + 1] == second:
                    out.append(first + second)
                    i += 2
                else:
                    out.append(word[i])
                    i += 1
            word = tuple(out)
        res = " ".join(word)
        self.cache[token] = res
        return res

    def encode(self, text: str) -> List[int]:
        ids: List[int] = []
        for tok in self.pat.findall(clean(text)):
            tok = "".join(self.byte_encoder[b] for b in tok.encode("utf-8"))
            ids.extend(self.encoder[t] for t in self.bpe(tok).split(" "))
        return ids


@lru_cache(maxsize=4)
def _tokenizer(path: str) -> SimpleTokenizer:
    return SimpleTokenizer(path)


def resolve_vocab(vocab_path: Optional[str] = None) -> Optional[str]:
    return vocab_path or os.environ.get(VOCAB_ENV) or None


def tokenize(texts: Union[str, Sequence[str]], vocab_path: Optional[str] = None, context: int = 77) -> torch.Tensor:
    """Token ids [B, context] int64: SOT, the text's BPE ids, EOT, zeros; longer texts are cut to `context` with
    EOT as the last id. With the full vocabulary SOT / EOT are 49406 / 49407."""
    if isinstance(texts, str):
        texts = [texts]
    path = resolve_vocab(vocab_path)
    out = torch.zeros((len(texts), context), dtype=torch.int64)
    for i, text in enumerate(texts):
        if not isinstance(text, str):
            raise TypeError(f"tokenize expects strings, got {type(text).__name__}")
        body: List[int] = []
        if clean(text):
            if path is None:
                raise FileNotFoundError(
                    f"tokenizing a non-empty text needs CLIP's BPE vocabulary {VOCAB_FILE} (open_clip ships it); "
                    f"pass its path with --clip_vocab / vocab_path or set {VOCAB_ENV}")
            body = _tokenizer(path).encode(text)
        ids = [SOT] + body + [EOT]
        if len(ids) > context:
            ids = ids[:context]
            ids[-1] = EOT
        out[i, :len(ids)] = torch.tensor(ids, dtype=torch.int64)
    return out
