"""CLIP byte-level BPE tokenizer, pure Python (the tokenizer of the SD-v1-4 snapshot, ``<snapshot>/tokenizer``).

Equivalent to ``transformers.CLIPTokenizer(...)(text, padding="max_length", truncation=True, max_length=77)``, the call
the reference makes on the prompt before the text encoder (modeling/meta_arch/ldm_diffusers.py:219-243), without
depending on ``transformers``, ``regex`` or ``ftfy``:

* normalisation as transformers' path without ftfy: Unicode NFC, lower case, whitespace runs collapsed, stripped.
  ftfy's mojibake repair (``ftfy.fix_text``) is NOT reproduced: text that ftfy would rewrite (broken encodings,
  curly quotes it straightens, ...) may tokenize differently.  The empty prompt and plain text are unaffected;
* the split pattern ``<|startoftext|>|<|endoftext|>|'s|'t|'re|'ve|'m|'ll|'d|[\\p{L}]+|[\\p{N}]|[^\\s\\p{L}\\p{N}]+``
  (case-insensitive), with ``\\p{L}`` / ``\\p{N}`` from ``unicodedata.category``;
* every word's UTF-8 bytes mapped through ``bytes_to_unicode``, ``</w>`` appended to its last symbol, merges applied by
  rank;
* ``[bos] + ids[:max_length - 2] + [eos]``, padded with the pad id to ``max_length``.
"""
import json
import os
import unicodedata


def bytes_to_unicode():
    """The byte -> printable-character table of GPT-2 / CLIP byte-level BPE."""
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(ord("¡"), ord("¬") + 1)) + \
        list(range(ord("®"), ord("ÿ") + 1))
    cs = bs[:]
    n = 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return dict(zip(bs, (chr(c) for c in cs)))


_CONTRACTIONS = ("s", "t", "re", "ve", "m", "ll", "d")


def _is_letter(ch):
    return unicodedata.category(ch).startswith("L")


def _is_number(ch):
    return unicodedata.category(ch).startswith("N")


def split_words(text, specials=("<|startoftext|>", "<|endoftext|>")):
    """The matches of CLIP's pre-tokenisation pattern in ``text``, left to right (what ``regex.findall`` returns)."""
    out = []
    i, n = 0, len(text)
    while i < n:
        sp = next((s for s in specials if text.startswith(s, i)), None)
        if sp is not None:
            out.append(sp)
            i += len(sp)
            continue
        ch = text[i]
        if ch == "'":
            c = next((c for c in _CONTRACTIONS if text[i + 1:i + 1 + len(c)].lower() == c), None)
            if c is not None:
                out.append(text[i:i + 1 + len(c)])
                i += 1 + len(c)
                continue
        if _is_letter(ch):
            j = i + 1
            while j < n and _is_letter(text[j]):
                j += 1
        elif _is_number(ch):
            j = i + 1
        elif ch.isspace():
            i += 1
            continue
        else:
            j = i + 1
            while j < n and not (text[j].isspace() or _is_letter(text[j]) or _is_number(text[j])):
                j += 1
        out.append(text[i:j])
        i = j
    return out


def normalize(text):
    return " ".join(unicodedata.normalize("NFC", text).lower().split())


def _token_str(v):
    return v["content"] if isinstance(v, dict) else v


class CLIPTokenizer:
    """``CLIPTokenizer.from_dir(<snapshot>/tokenizer)``; ``tok(texts)`` -> list of id lists of length ``max_length``."""

    def __init__(self, vocab, merges, bos="<|startoftext|>", eos="<|endoftext|>", pad="<|endoftext|>",
                 unk="<|endoftext|>", max_length=77):
        self.encoder = dict(vocab)
        self.bpe_ranks = {tuple(m): r for r, m in enumerate(merges)}
        self.byte_encoder = bytes_to_unicode()
        self.max_length = int(max_length)
        for name, t in (("bos", bos), ("eos", eos), ("pad", pad), ("unk", unk)):
            if t not in self.encoder:
                raise ValueError(f"CLIPTokenizer: {name} token {t!r} is not in the vocabulary")
        self.bos_token, self.eos_token = bos, eos
        self.bos_id, self.eos_id, self.pad_id, self.unk_id = (self.encoder[t] for t in (bos, eos, pad, unk))
        self.specials = (bos, eos)
        self.cache = {bos: bos, eos: eos}
        if self.max_length < 2:
            raise ValueError(f"CLIPTokenizer: max_length {self.max_length} leaves no room for BOS / EOS")

    @classmethod
    def from_dir(cls, path):
        with open(os.path.join(path, "vocab.json"), encoding="utf-8") as f:
            vocab = json.load(f)
        with open(os.path.join(path, "merges.txt"), encoding="utf-8") as f:
            lines = f.read().split("\n")
        merges = [tuple(l.split()) for l in lines if l.strip() and not l.startswith("#version")]
        if any(len(m) != 2 for m in merges):
            raise ValueError(f"{path}/merges.txt: every merge line must hold two symbols")
        cfg = {}
        for name in ("tokenizer_config.json", "special_tokens_map.json"):   # the map wins where both name a token
            p = os.path.join(path, name)
            if os.path.exists(p):
                with open(p, encoding="utf-8") as f:
                    cfg.update({k: v for k, v in json.load(f).items() if v is not None})
        kw = {k: _token_str(cfg[k + "_token"]) for k in ("bos", "eos", "pad", "unk") if k + "_token" in cfg}
        ml = cfg.get("model_max_length", 77)
        if not isinstance(ml, int) or ml > 10 ** 6:   # transformers' "no limit" sentinel
            ml = 77
        return cls(vocab, merges, max_length=ml, **kw)

    def bpe(self, token):
        if token in self.cache:
            return self.cache[token]
        word = tuple(token[:-1]) + (token[-1] + "</w>",)
        while len(word) > 1:
            pairs = set(zip(word[:-1], word[1:]))
            best = min(pairs, key=lambda p: self.bpe_ranks.get(p, float("inf")))
            if best not in self.bpe_ranks:
                break
            first, second = best
            new = []
            i = 0
            while i < len(word):
                if i < len(word) - 1 and word[i] == first and word[i + 1] == second:
                    new.append(first + second)
                    i += 2
                else:
                    new.append(word[i])
                    i += 1
            word = tuple(new)
        self.cache[token] = word
        return word

    def encode(self, text):
        """Token ids of ``text`` without BOS / EOS / padding."""
        ids = []
        for w in split_words(normalize(text), self.specials):
            if w in self.specials:
                ids.append(self.encoder[w])
                continue
            token = "".join(self.byte_encoder[b] for b in w.encode("utf-8"))
            ids.extend(self.encoder.get(s, self.unk_id) for s in self.bpe(token))
        return ids

    def __call__(self, texts):
        """padding="max_length", truncation=True: one list of ``max_length`` ids per text."""
        if isinstance(texts, str):
            texts = [texts]
        out = []
        for t in texts:
            ids = [self.bos_id] + self.encode(t)[:self.max_length - 2] + [self.eos_id]
            out.append(ids + [self.pad_id] * (self.max_length - len(ids)))
        return out
