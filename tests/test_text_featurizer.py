"""Featurizer numerics: pure-Python oracle vs native host path vs gfx950 kernel."""
import functools
import random

import numpy as np
import pytest
import torch

from fraud_detection_spark_kafka_llm_amd.data import fixtures
from fraud_detection_spark_kafka_llm_amd.ml.stopwords import ENGLISH
from fraud_detection_spark_kafka_llm_amd.ops import oracle as O
from fraud_detection_spark_kafka_llm_amd.ops import text as T

EDGE = ["", " ", "   ", "a", " a", "a ", "  a  b  ", "a\tb\nc", "don't stop", "İstanbul KELVIN K x",
        "UPPER lower MiXeD", "123 456 !!! ...", "été café \U0001F600 emoji", "the and of a an",
        "x" * 40, ("word " * 300).strip(), "ab  " * 50, fixtures.SCAM_SAMPLE, fixtures.BENIGN_SAMPLE]


def random_docs(n, seed=0, max_words=80):
    rng = random.Random(seed)
    vocab = ["hello", "the", "Suspect:", "Innocent:", "verify", "your", "social", "security", "number", "I'm",
             "please", "account", "Bank", "prize", "don't", "it's", "a", "and", "", "OK.", "x1", "café"]
    seps = [" ", " ", " ", "  ", "\n", "\t", ". ", ", "]
    out = []
    for _ in range(n):
        k = rng.randint(0, max_words)
        s = "".join(rng.choice(vocab) + rng.choice(seps) for _ in range(k))
        if rng.random() < 0.3:
            s = s.strip()
        out.append(s)
    return out


def csr_rows(res):
    ip, ix, v = res.csr()
    ip, ix, v = ip.cpu().numpy(), ix.cpu().numpy(), v.cpu().numpy()
    return [{int(a): float(b) for a, b in zip(ix[ip[i]:ip[i + 1]], v[ip[i]:ip[i + 1]])} for i in range(len(ip) - 1)]


def test_murmur_buckets():
    for w, b in fixtures.BUCKETS_10000.items():
        assert O.term_index(w, 10000) == b
    assert O.term_index("", 1 << 18) == 249180


def test_java_split_semantics():
    assert O.java_split_ws("") == [""]
    assert O.java_split_ws(" ") == []
    assert O.java_split_ws(" a") == ["", "a"]
    assert O.java_split_ws("a  b ") == ["a", "", "b"]
    assert O.java_split_ws("a\tb") == ["a", "b"]


def test_clean_text_rules():
    assert O.clean_text("Don't STOP-now 42\n!") == "dont stopnow "
    assert O.clean_text("İx K") == "ix k"


@pytest.mark.parametrize("clean", [True, False])
@pytest.mark.parametrize("stop", [True, False])
def test_native_cpu_matches_oracle(clean, stop):
    docs = EDGE + random_docs(300, seed=1)
    sw = list(ENGLISH) if stop else None
    spec = T.FeatureSpec(clean=clean, stopwords=sw, num_features=10007)
    res = T.featurize_score(T.PackedText.from_strings(docs), spec, want_csr=True, device="cpu")
    got = csr_rows(res)
    for d, g in zip(docs, got):
        s = O.clean_text(d) if clean else d
        toks = O.tokenize(s)
        if sw:
            toks = O.remove_stopwords(toks, sw)
        assert g == O.hashing_tf(toks, 10007), repr(d)[:80]


# the densest possible documents for the CSR scratch bound (csrc/scoring.h csr_slot: at most
# L / 2 + 2 distinct terms per L-byte document): distinct one-character tokens, a leading empty
# token, every parity of start offset
DENSE = ["".join(chr(c) + " " for c in range(33, 127)), " " + " ".join(chr(c) for c in range(33, 127)),
         "x", "", "a b", " " * 7 + "q", "\u00e9 \u00e8 \u00ea \u00eb \u00e0 " * 3]


@pytest.mark.parametrize("device", ["cpu", pytest.param("cuda:0", marks=pytest.mark.gpu)])
def test_densest_documents_fit_the_csr_scratch(device):
    docs = [d for k in range(3) for d in (DENSE[k % len(DENSE):] + DENSE[:k % len(DENSE)] + ["y" * (k + 1)])]
    spec = T.FeatureSpec(clean=False, stopwords=None, num_features=1 << 18)
    res = T.featurize_score(T.PackedText.from_strings(docs), spec, want_csr=True, device=device)
    got = csr_rows(res)
    for d, g in zip(docs, got):
        want = O.hashing_tf(O.tokenize(d), 1 << 18)
        assert g == want, repr(d)[:60]
        assert len(want) <= len(d.encode()) // 2 + 2


def test_vocab_mode_and_min_tf():
    docs = random_docs(200, seed=2)
    vocab = ["hello", "verify", "social", "security", "im", "dont", "please", "bank"]
    for min_tf in (1.0, 2.0, 0.1):
        spec = T.FeatureSpec(clean=True, stopwords=list(ENGLISH), vocab=vocab, min_tf=min_tf)
        got = csr_rows(T.featurize_score(T.PackedText.from_strings(docs), spec, want_csr=True, device="cpu"))
        for d, g in zip(docs, got):
            toks = O.remove_stopwords(O.tokenize(O.clean_text(d)), ENGLISH)
            assert g == O.count_vectorize(toks, vocab, min_tf), d


def test_binary_and_idf_scaling():
    docs = random_docs(50, seed=3)
    idf = np.random.default_rng(0).random(997)
    spec = T.FeatureSpec(clean=True, stopwords=list(ENGLISH), num_features=997, binary=True)
    got = csr_rows(T.featurize_score(T.PackedText.from_strings(docs), spec, idf=torch.from_numpy(idf),
                                     want_csr=True, device="cpu"))
    for d, g in zip(docs, got):
        toks = O.remove_stopwords(O.tokenize(O.clean_text(d)), ENGLISH)
        ref = {k: np.float32(v * idf[k]) for k, v in O.hashing_tf(toks, 997, binary=True).items()}
        assert g == pytest.approx({k: float(v) for k, v in ref.items()})


def test_lr_margin_matches_oracle():
    docs = random_docs(100, seed=4)
    rng = np.random.default_rng(1)
    w = rng.normal(size=1000)
    idf = rng.random(1000)
    spec = T.FeatureSpec(clean=True, stopwords=list(ENGLISH), num_features=1000)
    res = T.featurize_score(T.PackedText.from_strings(docs), spec, idf=torch.from_numpy(idf),
                            lr=T.LinearScorer(w, 0.25), device="cpu")
    for d, m in zip(docs, res.raw[:, 0].numpy()):
        x = O.pipeline_vector(d, ENGLISH, 1000, idf)
        assert m == pytest.approx(O.lr_margin(x, w, 0.25), rel=1e-12, abs=1e-12)


def random_forest_arrays(num_trees, num_features, depth, K, seed=0, cmp_less=False):
    rng = np.random.default_rng(seed)
    feat, thr, left, right, leaf, roots = [], [], [], [], [], []

    def build(d):
        i = len(feat)
        feat.append(-1); thr.append(0.0); left.append(-1); right.append(-1)
        leaf.append(rng.random(K).tolist())
        if d < depth and rng.random() < 0.85:
            feat[i] = int(rng.integers(0, num_features))
            thr[i] = float(rng.choice([0.0, 0.5, 1.5, 2.5, 3.7]))
            left[i] = build(d + 1)
            right[i] = build(d + 1)
        return i

    for _ in range(num_trees):
        roots.append(build(0))
    return T.TreeArrays(feat, thr, left, right, np.asarray(leaf), roots, rng.random(num_trees), K, cmp_less)


def host_tree_score(arrs, x, cmp_less):
    out = np.zeros(arrs.K)
    for t, r in enumerate(arrs.roots):
        i = r
        while arrs.feat[i] >= 0:
            v = x.get(int(arrs.feat[i]), 0.0)
            i = arrs.left[i] if (v < arrs.thr[i] if cmp_less else v <= arrs.thr[i]) else arrs.right[i]
        out += arrs.tree_weights[t] * arrs.leaf[i * arrs.K:(i + 1) * arrs.K]
    return out


@pytest.mark.parametrize("cmp_less", [False, True])
def test_tree_scoring_matches_oracle(cmp_less):
    docs = random_docs(60, seed=5)
    arrs = random_forest_arrays(70, 64, 5, 2, seed=2, cmp_less=cmp_less)
    spec = T.FeatureSpec(clean=True, stopwords=list(ENGLISH), num_features=64)
    res = T.featurize_score(T.PackedText.from_strings(docs), spec, trees=arrs, device="cpu")
    for d, r in zip(docs, res.raw.numpy()):
        x = O.pipeline_vector(d, ENGLISH, 64)
        np.testing.assert_allclose(r, host_tree_score(arrs, x, cmp_less), rtol=1e-12)


# ---------------------------------------------------------------- the kernels' LDS capacities
# csrc/text_kernels.hip: the streaming variant holds 4096 bytes and 1024 kept tokens per dialogue,
# the long-dialogue variant 65536 bytes and 16384 tokens with 16-bit token starts.
CAP_B, CAP_T, LONG_B, LONG_T = 4096, 1024, 65536, 16384


def _short_tokens(n, skip=()):
    """The first n lower-case tokens of 1, 2, 3 letters (a, b, .. z, aa, ab, ..) not in ``skip``."""
    import itertools
    import string

    out = []
    for k in (1, 2, 3):
        for t in itertools.product(string.ascii_lowercase, repeat=k):
            if "".join(t) not in skip:
                out.append("".join(t))
            if len(out) == n:
                return out
    raise ValueError(n)


def _run_head_tokens(n, num_features=1 << 18):
    """n short tokens that are no stop words and fall into n different buckets: after the sort
    every element is the head of its own run."""
    seen, out = set(), []
    for t in _short_tokens(n + 400, skip=set(ENGLISH)):
        b = O.term_index(t, num_features)
        if b not in seen:
            seen.add(b)
            out.append(t)
        if len(out) == n:
            return out
    raise ValueError(n)


# packed in this order: the start offsets take every value mod 4
CAPACITY = ["b " * 1024, "b " * 1025, ("b " * 1023).strip(),                   # kept tokens at the streaming cap
            " ".join(_short_tokens(1024)), " ".join(_short_tokens(1025)),      # 3,367 and 3,371 bytes
            "word " * 819 + "x", "word " * 819 + "xy", "word " * 819,          # 4096, 4097, 4095 bytes
            " " * 4096, " " * 2000 + "x", "12345", "123 456", "x" * 4096, "x" * 4097,
            "b " * 16384, "b " * 16385,                                        # tokens at the long cap
            "x" * 65534 + " y", "x" * 65535 + " y",                            # 65536 and 65537 bytes
            "abc K", "abc İ"]                                        # Kelvin sign, dotted capital I
# a multi-byte character across the 4-byte lane word and the 256-byte wave step
CAPACITY += [("a" * (250 + k)) + c + "b c" for k in range(8) for c in ("K", "İ")]
# every element a run head: a full-width (1024) sort, and one past the streaming table
CAPACITY += [" ".join(_run_head_tokens(1024)), " ".join(_run_head_tokens(1025))]
I_B1024, I_B1025, I_B1023, I_D1024, I_D1025, I_B16384, I_B16385, I_65536, I_65537 = 0, 1, 2, 3, 4, 14, 15, 16, 17
I_HEADS = len(CAPACITY) - 2
# (clean, stop words, num_features, binary)
CAP_SPECS = [(True, True, 1 << 18, False), (True, False, 10007, True), (False, False, 3, False), (False, True, 1, False)]


@functools.lru_cache(maxsize=None)
def _capacity_tokens(clean, stop):
    """The oracle's kept tokens of every CAPACITY document (computed once per mode)."""
    out = []
    for d in CAPACITY:
        toks = O.tokenize(O.clean_text(d) if clean else d)
        out.append(O.remove_stopwords(toks, ENGLISH) if stop else toks)
    return out


@functools.lru_cache(maxsize=None)
def _capacity_tf(k):
    clean, stop, F, binary = CAP_SPECS[k]
    return [O.hashing_tf(toks, F, binary) for toks in _capacity_tokens(clean, stop)]


def test_capacity_documents_stand_on_the_limits():
    """The inputs are what they claim: byte lengths, kept tokens and distinct terms at the caps."""
    nb = [len(d.encode()) for d in CAPACITY]
    assert [nb[i] for i in (3, 4, 5, 6, 7, 8, 12, 13)] == [3367, 3371, CAP_B, CAP_B + 1, CAP_B - 1, CAP_B, CAP_B,
                                                          CAP_B + 1]
    assert nb[I_65536] == LONG_B and nb[I_65537] == LONG_B + 1 and nb[I_B16384] == 2 * LONG_T
    offs = np.cumsum([0] + nb[:-1])
    assert {int(o) % 4 for o in offs} == {0, 1, 2, 3}
    for clean, stop in {(c, s) for c, s, _, _ in CAP_SPECS}:
        kept = [len(t) for t in _capacity_tokens(clean, stop)]
        assert [kept[i] for i in (I_B1023, I_B1024, I_B1025, I_B16384, I_B16385)] == [
            CAP_T - 1, CAP_T, CAP_T + 1, LONG_T, LONG_T + 1]
    toks = _capacity_tokens(True, False)
    assert [len(set(toks[i])) for i in (I_D1024, I_D1025)] == [len(toks[i]) for i in (I_D1024, I_D1025)] == [1024, 1025]
    tf = _capacity_tf(0)                    # clean, stop words, 2^18 buckets: every kept token its own term
    kept = _capacity_tokens(True, True)
    assert [len(kept[I_HEADS + j]) for j in (0, 1)] == [len(tf[I_HEADS + j]) for j in (0, 1)] == [1024, 1025]


@pytest.mark.parametrize("device", ["cpu", pytest.param("cuda:0", marks=pytest.mark.gpu)])
@pytest.mark.parametrize("k", range(len(CAP_SPECS)))
def test_capacity_documents_match_oracle(k, device):
    """Dialogues at 4095 / 4096 / 4097 and 65536 / 65537 bytes, 1023 / 1024 / 1025 and 16384 / 16385
    kept tokens, 1024 distinct terms, a token starting at byte 65535 and multi-byte characters across
    the load boundaries: the CSR rows are the oracle's term counts exactly, the values with an IDF
    vector float32(tf * idf[k]) exactly (host twin and kernel share csrc/scoring.h, so both are
    checked against the Python oracle, not against each other)."""
    clean, stop, F, binary = CAP_SPECS[k]
    spec = T.FeatureSpec(clean=clean, stopwords=list(ENGLISH) if stop else None, num_features=F, binary=binary)
    pt = T.PackedText.from_strings(CAPACITY)
    want = _capacity_tf(k)
    got = csr_rows(T.featurize_score(pt, spec, want_csr=True, device=device))
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, repr(CAPACITY[i])[:40])
    idf = np.random.default_rng(k).random(F) + 0.25
    got = csr_rows(T.featurize_score(pt, spec, idf=torch.from_numpy(idf), want_csr=True, device=device))
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == {t: float(np.float32(v * idf[t])) for t, v in w.items()}, (i, repr(CAPACITY[i])[:40])


@functools.lru_cache(maxsize=None)
def _capacity_lr(device):
    rng = np.random.default_rng(1)
    w, idf = rng.normal(size=1000), rng.random(1000)
    spec = T.FeatureSpec(clean=True, stopwords=list(ENGLISH), num_features=1000)
    res = T.featurize_score(T.PackedText.from_strings(CAPACITY), spec, idf=torch.from_numpy(idf),
                            lr=T.LinearScorer(w, 0.25), device=device)
    return res.raw.cpu()[:, 0].numpy(), w, idf


@pytest.mark.parametrize("device", ["cpu", pytest.param("cuda:0", marks=pytest.mark.gpu)])
def test_capacity_lr_margin_matches_oracle(device):
    """(tolerance of test_lr_margin_matches_oracle); the kernel's margins are the host's bit for bit."""
    got, w, idf = _capacity_lr(device)
    for d, m in zip(CAPACITY, got):
        x = O.pipeline_vector(d, ENGLISH, 1000, idf)
        assert m == pytest.approx(O.lr_margin(x, w, 0.25), rel=1e-12, abs=1e-12), repr(d)[:40]
    if device != "cpu":
        np.testing.assert_array_equal(got, _capacity_lr("cpu")[0])


@pytest.mark.parametrize("device", ["cpu", pytest.param("cuda:0", marks=pytest.mark.gpu)])
@pytest.mark.parametrize("K,cmp_less", [(1, False), (1, True), (2, True)])
def test_capacity_tree_scores_match_oracle(K, cmp_less, device):
    """One leaf value per node (the boosters) and strict comparisons: the host within the tolerance
    of test_tree_scoring_matches_oracle of the plain traversal, the kernel the host bit for bit."""
    arrs = random_forest_arrays(70, 64, 5, K, seed=2 + K, cmp_less=cmp_less)
    spec = T.FeatureSpec(clean=True, stopwords=list(ENGLISH), num_features=64)
    pt = T.PackedText.from_strings(CAPACITY)
    host = T.featurize_score(pt, spec, trees=arrs, device="cpu").raw
    assert host.shape == (len(CAPACITY), K)
    if device == "cpu":
        for d, r in zip(CAPACITY, host.numpy()):
            x = O.pipeline_vector(d, ENGLISH, 64)
            np.testing.assert_allclose(r, host_tree_score(arrs, x, cmp_less), rtol=1e-12)
    else:
        assert torch.equal(T.featurize_score(pt, spec, trees=arrs, device=device).raw.cpu(), host)


# ------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("clean", [True, False])
def test_gpu_capacity_statuses_and_fallbacks(clean):
    """Without host fallbacks the device leaves exactly the dialogues it cannot hold: over 65536
    raw bytes without a cut point, over 16384 kept tokens, and (without cleaning) non-ASCII ones;
    with fallbacks everything is the host's result bit for bit."""
    spec = T.FeatureSpec(clean=clean, stopwords=list(ENGLISH), num_features=1 << 18)
    pt = T.PackedText.from_strings(CAPACITY)
    idf = torch.rand(1 << 18, dtype=torch.float64)
    lr = T.LinearScorer(torch.randn(1 << 18, dtype=torch.float64).numpy(), -0.5)
    kept = _capacity_tokens(clean, True)
    want = []
    for d, toks in zip(CAPACITY, kept):
        raw = d.encode()
        if len(raw) > LONG_B or len(toks) > LONG_T:
            want.append(T.STATUS_TOO_LONG)
        else:
            want.append(T.STATUS_NEEDS_HOST if (not clean and max(raw, default=0) >= 0x80) else T.STATUS_OK)
    assert want[I_B16385] == want[I_65537] == T.STATUS_TOO_LONG and want.count(T.STATUS_TOO_LONG) == 2
    assert want.count(T.STATUS_NEEDS_HOST) == (0 if clean else 18)
    gpu = T.featurize_score(pt, spec, idf=idf, lr=lr, want_csr=True, device="cuda:0", fix_fallbacks=False)
    assert gpu.status.cpu().tolist() == want
    cpu = T.featurize_score(pt, spec, idf=idf, lr=lr, want_csr=True, device="cpu")
    gpu = T.featurize_score(pt, spec, idf=idf, lr=lr, want_csr=True, device="cuda:0")
    assert torch.equal(cpu.status, gpu.status.cpu()) and torch.equal(cpu.nnz, gpu.nnz.cpu())
    for a, b in zip(cpu.csr(), gpu.csr()):
        assert torch.equal(a, b.cpu())
    assert torch.equal(cpu.raw, gpu.raw.cpu())


@pytest.mark.gpu
@pytest.mark.parametrize("stop", [True, False])
@pytest.mark.parametrize("min_tf", [1.0, 0.1, 2.0])
def test_gpu_vocab_mode_matches_oracle(min_tf, stop):
    """CountVectorizerModel mode on the kernel against the oracle: absolute and fractional minTF
    (the fraction is of the tokens after stop-word removal), with the token-cap dialogues."""
    docs = random_docs(200, seed=12) + CAPACITY[:5]
    vocab = ["hello", "verify", "social", "security", "im", "dont", "please", "bank", "prize", "b", "zz", "the"]
    sw = list(ENGLISH) if stop else None
    spec = T.FeatureSpec(clean=True, stopwords=sw, vocab=vocab, min_tf=min_tf)
    got = csr_rows(T.featurize_score(T.PackedText.from_strings(docs), spec, want_csr=True, device="cuda:0"))
    for d, g in zip(docs, got):
        toks = O.tokenize(O.clean_text(d))
        if stop:
            toks = O.remove_stopwords(toks, ENGLISH)
        assert g == O.count_vectorize(toks, vocab, min_tf), repr(d)[:40]


@pytest.mark.gpu
@pytest.mark.parametrize("clean", [True, False])
def test_gpu_kernel_bitwise_equals_host(clean):
    docs = EDGE + random_docs(3000, seed=7, max_words=400)
    spec = T.FeatureSpec(clean=clean, stopwords=list(ENGLISH), num_features=1 << 18)
    pt = T.PackedText.from_strings(docs)
    idf = torch.rand(1 << 18, dtype=torch.float64)
    w = torch.randn(1 << 18, dtype=torch.float64)
    lr = T.LinearScorer(w.numpy(), -0.5)
    cpu = T.featurize_score(pt, spec, idf=idf, lr=lr, want_csr=True, device="cpu")
    gpu = T.featurize_score(pt, spec, idf=idf, lr=lr, want_csr=True, device="cuda:0")
    assert torch.equal(cpu.status, gpu.status.cpu())
    assert torch.equal(cpu.nnz, gpu.nnz.cpu())
    for a, b in zip(cpu.csr(), gpu.csr()):
        assert torch.equal(a, b.cpu())
    assert torch.equal(cpu.raw, gpu.raw.cpu())   # same fp64 summation order, no FMA


@pytest.mark.gpu
def test_gpu_tree_scoring_bitwise():
    docs = random_docs(2000, seed=8, max_words=200)
    arrs = random_forest_arrays(130, 4096, 6, 2, seed=3)
    spec = T.FeatureSpec(clean=True, stopwords=list(ENGLISH), num_features=4096)
    pt = T.PackedText.from_strings(docs)
    cpu = T.featurize_score(pt, spec, trees=arrs, device="cpu")
    gpu = T.featurize_score(pt, spec, trees=arrs, device="cuda:0")
    assert torch.equal(cpu.raw, gpu.raw.cpu())


@pytest.mark.gpu
def test_gpu_vocab_mode():
    docs = random_docs(500, seed=9)
    vocab = ["hello", "verify", "social", "security", "im", "dont", "please", "bank", "prize"]
    spec = T.FeatureSpec(clean=True, stopwords=list(ENGLISH), vocab=vocab, min_tf=2.0)
    pt = T.PackedText.from_strings(docs)
    cpu = T.featurize_score(pt, spec, want_csr=True, device="cpu")
    gpu = T.featurize_score(pt, spec, want_csr=True, device="cuda:0")
    for a, b in zip(cpu.csr(), gpu.csr()):
        assert torch.equal(a, b.cpu())


@pytest.mark.gpu
@pytest.mark.parametrize("scorer", ["lr", "trees"])
def test_gpu_long_dialogues_stay_on_device_and_match_host(scorer):
    """Dialogues over the streaming kernel's 4 KB capacity run on the long-dialogue kernel (64 KB,
    16K tokens); only larger ones reach the host path. Results are bitwise equal to the host."""
    rng = np.random.default_rng(3)
    words = ["bank", "verify", "account", "please", "the", "hello", "prize", "ssn", "x", "zebra"]
    docs = ["word " * 2000,                                   # 10 KB
            "a " * 3000,                                      # 1 token x 3000 (token cap, short text)
            " ".join(rng.choice(words, 6000)),                # ~33 KB
            " ".join(f"w{i}" for i in range(9000)),           # 9000 distinct tokens
            "z" * 70000,                                      # > 64 KB -> host
            fixtures.SCAM_SAMPLE] + random_docs(300, seed=4)
    pt = T.PackedText.from_strings(docs)
    F = 1 << 14
    spec = T.FeatureSpec(clean=True, stopwords=list(ENGLISH), num_features=F)
    idf = torch.rand(F, dtype=torch.float64)
    kw = dict(idf=idf)
    if scorer == "lr":
        kw["lr"] = T.LinearScorer(torch.randn(F, dtype=torch.float64).numpy(), 0.25)
    else:
        kw["trees"] = random_forest_arrays(40, F, 6, 2, seed=5)
    cpu = T.featurize_score(pt, spec, want_csr=True, device="cpu", **kw)
    gpu = T.featurize_score(pt, spec, want_csr=True, device="cuda:0", fix_fallbacks=False, **kw)
    st = gpu.status.cpu()
    assert st[:4].eq(T.STATUS_OK).all() and st[4] == T.STATUS_TOO_LONG   # only the 70 KB one left
    gpu = T.featurize_score(pt, spec, want_csr=True, device="cuda:0", **kw)
    assert torch.equal(cpu.nnz, gpu.nnz.cpu())
    for a, b in zip(cpu.csr(), gpu.csr()):
        assert torch.equal(a, b.cpu())
    assert torch.equal(cpu.raw, gpu.raw.cpu())
