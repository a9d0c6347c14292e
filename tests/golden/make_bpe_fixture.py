"""Writes the CLIP BPE fixture the tokenizer tests run on, from the reference's merge table (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_bpe_fixture.py

  clip_bpe_subset.txt.gz : the reference's assets/bpe_simple_vocab_16e6.txt.gz with every merge line that no
                           text below can reach replaced by an inert filler line ("Ā Ā": byte 0x00 twice, which
                           no text holds).  The kept merges stay at their line numbers, so ranks and token ids are
                           those of the full table; every merge the BPE loop can consult for these texts is kept
                           (its joined string is a run of the word's symbols), so their tokens are identical.
  clip_bpe_texts.npz     : the tokenizer tests' texts and the ids the reference's clip.tokenize gives them.

The script checks both claims: own tokenizer on the subset == own tokenizer on the full table == the reference.
"""
import gzip
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import ref_harness as rh  # noqa: E402
from clip_glass_amd import tokenizer as T  # noqa: E402

FILLER = "Ā Ā"
# tests/test_host.py::test_clip_tokenizer_matches_reference_known_answers
KNOWN_TEXTS = ["a wolf at night with the moon in the background", "A photo of  a CAT!!",
               "it's 42 degrees & sunny -- don't you think?", "naïve café façade", "x" * 10,
               "the quick brown fox jumps over the lazy dog, twice.", "&amp; html &lt;escapes&gt;", "word"]


def _runs(tok, text):
    """Every contiguous run of the BPE start symbols of every word of `text`, joined."""
    out = set()
    text = " ".join(T.html.unescape(T.html.unescape(text)).strip().split()).lower()
    for w in T._WORD.findall(text):
        w = "".join(tok.byte_to_char[b] for b in w.encode("utf-8"))
        syms = list(w[:-1]) + [w[-1] + "</w>"]
        for i in range(len(syms)):
            for j in range(i + 1, len(syms) + 1):
                out.add("".join(syms[i:j]))
    return out


def main():
    assert rh.available(), "needs the reference"
    full = os.path.join(rh.REF, "assets", "bpe_simple_vocab_16e6.txt.gz")
    fixture_texts = [str(t) for t in np.load(os.path.join(HERE, "clip_text_full.npz"))["texts"]]
    texts = KNOWN_TEXTS + fixture_texts
    tok = T.ClipTokenizer(full)
    keep = set()
    for t in texts:
        keep |= _runs(tok, t)
    lines = gzip.open(full).read().decode("utf-8").split("\n")
    last = 49152 - 256 - 2 + 1
    out = [lines[0]]
    for l in lines[1:last]:
        out.append(l if l.strip() and "".join(l.split()) in keep else FILLER)
    assert all(FILLER.split()[0] not in "".join(_runs(tok, t)) for t in texts)
    path = os.path.join(HERE, "clip_bpe_subset.txt.gz")
    with open(path, "wb") as f, gzip.GzipFile(fileobj=f, mode="wb", mtime=0) as g:
        g.write(("\n".join(out) + "\n").encode("utf-8"))
    sub = T.ClipTokenizer(path)
    known = KNOWN_TEXTS[:-1]
    ref = rh.load_reference()["clip_clip"].tokenize(known).numpy()
    np.testing.assert_array_equal(tok.tokenize(known), ref)
    np.testing.assert_array_equal(sub.tokenize(known), ref)
    np.testing.assert_array_equal(sub.tokenize(fixture_texts), tok.tokenize(fixture_texts))
    assert sub.encode("word " * 100) == tok.encode("word " * 100)
    np.savez(os.path.join(HERE, "clip_bpe_texts.npz"), texts=np.array(known), tokens=ref)
    print("kept %d of %d merges; %s %d bytes" % (sum(l != FILLER for l in out[1:]), len(out) - 1, path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
