"""The contract of include/wordpiece_amd_classify.h in plain Python: tokens, H, grams, word n-grams, the features of a
document, and logits / softmax in float64."""
import numpy as np

SPACES = frozenset(b" \n\r\t\x0b\x0c\x00")
EOS = b"</s>"
M32, M64 = 2 ** 32 - 1, 2 ** 64 - 1


def H(data):
    h = 2166136261
    for b in data:
        h = ((h ^ ((b - 256 if b >= 128 else b) & M32)) * 16777619) & M32
    return h


def tokens(doc):
    """the tokens of a document, "</s>" behind them"""
    out, cur = [], bytearray()
    for b in doc:
        if b in SPACES:
            if cur:
                out.append(bytes(cur))
            cur = bytearray()
        else:
            cur.append(b)
    return out + ([bytes(cur)] if cur else []) + [EOS]


def grams(token, minn, maxn):
    """the kept character n-grams of a token, in order of start and length"""
    w, out = b"<" + token + b">", []
    for i in range(len(w)):
        if w[i] & 0xC0 == 0x80:
            continue
        j = i
        for n in range(1, maxn + 1):
            if j >= len(w):
                break
            j += 1
            while j < len(w) and w[j] & 0xC0 == 0x80:
                j += 1
            if n >= minn and not (n == 1 and (i == 0 or j == len(w))):
                out.append(w[i:j])
    return out


def word_ngrams(toks, N, bucket):
    """the bucket indices of the word n-grams of a token list ("</s>" included)"""
    s = [H(t) - 2 ** 32 if H(t) >= 2 ** 31 else H(t) for t in toks]
    out = []
    for t in range(len(s)):
        h = s[t] & M64
        for j in range(t + 1, min(t + N, len(s))):
            h = (h * 116049371 + s[j]) & M64
            out.append(h % bucket)
    return out


class Model:
    def __init__(self, words, inp, outp, minn, maxn, word_ngrams, bucket):
        self.words, self.inp, self.outp = [bytes(w) for w in words], np.asarray(inp), np.asarray(outp, dtype=np.float64)  # (inp is widened row by row: it can be large)
        self.minn, self.maxn, self.N, self.bucket = minn, maxn, word_ngrams, bucket
        self.wid = {}
        for i, w in enumerate(self.words):
            self.wid.setdefault(w, i)

    def features(self, doc):
        toks, nw, f = tokens(doc), len(self.words), []
        for t in toks:
            if t in self.wid:
                f.append(self.wid[t])
            if self.maxn > 0 and t != EOS:
                f += [nw + H(g) % self.bucket for g in grams(t, self.minn, self.maxn)]
        if self.N > 1:
            f += [nw + h for h in word_ngrams(toks, self.N, self.bucket)]
        return f, len(toks), sum(t in self.wid for t in toks)

    def score(self, doc, keep=None, min_prob=0.0):
        """-> dict: F, S (the exact sum of the rows), logits, label, prob, reasons; all float64"""
        f = self.features(doc)[0]
        S = self.inp[f].astype(np.float64).sum(axis=0) if f else np.zeros(self.inp.shape[1])
        if not f:
            return dict(F=0, S=S, logits=np.zeros(len(self.outp)), label=-1, prob=0.0, reasons=1)
        logits = self.outp @ S / len(f)
        e = np.exp(logits - logits.max())
        label, prob = int(np.argmax(logits)), float(1.0 / e.sum())
        reasons = (2 if keep is not None and label not in keep else 0) | (4 if prob < min_prob else 0)
        return dict(F=len(f), S=S, logits=logits, label=label, prob=prob, reasons=reasons)
