"""TEST INFRASTRUCTURE: write tests/golden/bpe_merges_subset.txt.gz, the stand-in for the CLIP BPE merges file that the
tokenizer tests read, so that they run from a clean checkout without the third-party file.

    python oracle/make_bpe_subset.py /path/to/bpe_simple_vocab_16e6.txt.gz

The subset keeps every merge the tokenizer looks up with success while it encodes the texts the tests tokenize, and every
merge whose joined token equals a token those texts produce; every other line becomes the same placeholder pair of
characters that no byte symbol maps to (it can never match a pair of a word, and its joined token collides with none).
Ranks and ids therefore stay those of the full file for these texts, and the file shrinks to a few kB.  The script checks
that the subset tokenizes every text exactly like the full file before it writes anything.
"""
from __future__ import annotations

import gzip
import io
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

import clip_fsar_amd.text as ctext  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "bpe_merges_subset.txt.gz")
PLACEHOLDER = "一"            # CJK code point: _byte_symbols() maps bytes to code points < 0x144 only


def test_texts():
    """Every text tests/test_text_n1.py tokenizes."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "text_cases.npz"))
    texts = list(json.loads(str(z["texts"])))
    texts += ["a photo of blasting sand", "a photo of hurling (sport)", "word " * 100]
    texts += ctext.prompts(["air drumming", "bowling", "cheerleading", "zumba", "yoga",
                            "busking", "unboxing", "ice skating", "side kick", "tap dancing"])
    return texts


class _Recorder(dict):
    """rank table that notes every pair it is asked for and holds"""

    def __init__(self, *a):
        super().__init__(*a)
        self.hits = set()

    def get(self, key, default=None):
        if key in self:
            self.hits.add(key)
        return super().get(key, default)


def main(src):
    texts = test_texts()
    full = ctext.ClipBpeTokenizer(src)
    full.rank = _Recorder(full.rank)
    want = full.tokenize(texts, truncate=True)
    lines = gzip.open(src).read().decode("utf-8").split("\n")
    merges = [tuple(l.split()) for l in lines[1:ctext.N_MERGES + 1]]
    id_to_tok = {i: t for t, i in full.ids.items()}
    needed = {"".join(m) for m in full.rank.hits} | {id_to_tok[int(i)] for i in np.unique(want)}
    keep = [m in full.rank.hits or "".join(m) in needed for m in merges]
    body = ["%s %s" % m if k else "%s %s" % (PLACEHOLDER, PLACEHOLDER) for m, k in zip(merges, keep)]
    text = "\n".join(["#version: 0.2 (test subset, oracle/make_bpe_subset.py)"] + body) + "\n"
    buf = io.BytesIO()
    with gzip.GzipFile(fileobj=buf, mode="wb", mtime=0) as f:       # mtime 0: the same bytes on every run
        f.write(text.encode("utf-8"))
    tmp = OUT + ".tmp"
    with open(tmp, "wb") as f:
        f.write(buf.getvalue())
    got = ctext.ClipBpeTokenizer(tmp).tokenize(texts, truncate=True)
    if not np.array_equal(got, want):
        os.remove(tmp)
        raise SystemExit("the subset tokenizes differently from the full merges file")
    os.replace(tmp, OUT)
    print("%s: %d of %d merges kept, %d bytes" % (OUT, sum(keep), len(merges), len(buf.getvalue())))


if __name__ == "__main__":
    main(sys.argv[1])
