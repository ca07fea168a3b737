"""Spark's NGram stage, fused into the featurize-and-score kernel: every expected value comes from
``oracle.ngrams`` plus the oracle's hashing / counting / murmur3; where bitwise equality between the
kernel and the host twin is claimed they are compared with each other in addition, never instead."""
import functools
import itertools
import json
import os
import random
import shutil
import string
import subprocess

import numpy as np
import pytest
import torch

from fraud_detection_spark_kafka_llm_amd import _build
from fraud_detection_spark_kafka_llm_amd.data import fixtures, synth
from fraud_detection_spark_kafka_llm_amd.ml import (IDF, CountVectorizer, DecisionTreeClassifier, Frame, HashingTF,
                                                     LogisticRegression, NGram, Pipeline, PipelineModel,
                                                     StopWordsRemover, TextColumn, TokenColumn, Tokenizer)
from fraud_detection_spark_kafka_llm_amd.ml.fused import match_chain
from fraud_detection_spark_kafka_llm_amd.ml.stopwords import ENGLISH
from fraud_detection_spark_kafka_llm_amd.ops import native
from fraud_detection_spark_kafka_llm_amd.ops import oracle as O
from fraud_detection_spark_kafka_llm_amd.ops import text as T

DEVICES = ["cpu", pytest.param("cuda:0", marks=pytest.mark.gpu)]
F = 10007

# the edge documents of test_text_featurizer.py
EDGE = ["", " ", "   ", "a", " a", "a ", "  a  b  ", "a\tb\nc", "don't stop", "İstanbul KELVIN K x",
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


def kept_tokens(d, clean, stop):
    toks = O.tokenize(O.clean_text(d) if clean else d)
    return O.remove_stopwords(toks, ENGLISH) if stop else toks


def grams(d, clean, stop, n):
    return O.ngrams(kept_tokens(d, clean, stop), n)


# ------------------------------------------------------------------------------ 1. oracle anchors
def test_oracle_anchors():
    assert O.ngrams(["Hi", "I", "heard", "about", "Spark"], 2) == ["Hi I", "I heard", "heard about", "about Spark"]
    for n in (2, 3, 5):
        toks = [f"t{i}" for i in range(n)]
        assert O.ngrams([], n) == []
        assert O.ngrams(toks[:n - 1], n) == []
        assert O.ngrams(toks, n) == [" ".join(toks)]
    toks = ["a", "", "b", "the", ""]
    assert O.ngrams(toks, 1) == toks
    assert O.ngrams(O.java_split_ws("a  b"), 2) == ["a ", " b"]       # empty tokens are tokens
    assert O.ngrams(["a", "", "", "b"], 3) == ["a  ", "  b"]
    with pytest.raises(ValueError):
        O.ngrams(toks, 0)


def test_ngram_stage_params():
    g = NGram(inputCol="words", outputCol="grams")
    assert g.getN() == 2 and NGram(n=3).getN() == 3
    for bad in (0, -1):
        with pytest.raises(ValueError):
            NGram(n=bad)
        with pytest.raises(ValueError):
            g.setN(bad)
    with pytest.raises(ValueError):
        T.FeatureSpec(ngram=T.NGRAM_MAX + 1)
    assert T.NGRAM_MAX == 8


# ------------------------------------------------------------------------------ 2. rows = oracle
def kept_exactly(k):
    """k kept tokens, each followed by one or two stop words: with stop-word removal the members of
    an n-gram are separated by removed tokens and fall into different 64-token batches of the pass
    that finds the tokens."""
    if k == 0:
        return "the is a"
    return "".join(f"q{string.ascii_lowercase[i % 26]}{'x' * (i % 3)}" + (" the " if i % 2 else " is a ")
                   for i in range(k))


@functools.lru_cache(maxsize=None)
def row_docs(n):
    ks = [0, 1, n - 1, n, n + 1, 63, 64, 65, 64 + n - 1, 127, 128, 129]
    toks = ["qrstu"[:k] for k in range(1, 6)]
    pairs = [f"{x} {y} {y}  {x}" for x, y in itertools.product(toks, toks)]     # joined lengths 3..11
    return (EDGE + random_docs(300, seed=1) + [kept_exactly(k) for k in ks]
            + ["a  b", "x  y   z    w  ", "  lead  and  trail  ", "gift  card   gift  card"]
            + ["gift\tcard\nwire\r\ntransfer  the\x0bb\x0cend", "\ta\n\nb\t"] + pairs)


def test_row_documents_are_what_they_claim():
    for n in (2, 3):
        ks = [0, 1, n - 1, n, n + 1, 63, 64, 65, 64 + n - 1, 127, 128, 129]
        for k in ks:
            d = kept_exactly(k)
            assert len(kept_tokens(d, True, True)) == k and len(kept_tokens(d, True, False)) >= max(2 * k, 3)
    lens = {len(g.encode()) % 4 for d in row_docs(2)[-25:] for g in grams(d, True, False, 2)}
    assert lens == {0, 1, 2, 3}


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("stop", [True, False])
@pytest.mark.parametrize("clean", [True, False])
@pytest.mark.parametrize("n", [2, 3])
def test_rows_equal_oracle(n, clean, stop, device):
    docs = row_docs(n)
    spec = T.FeatureSpec(clean=clean, stopwords=list(ENGLISH) if stop else None, num_features=F, ngram=n)
    pt = T.PackedText.from_strings(docs)
    res = T.featurize_score(pt, spec, want_csr=True, device=device)
    assert res.status.cpu().eq(T.STATUS_OK).all()
    got, ntok = csr_rows(res), res.ntok.cpu().tolist()
    for i, (d, g) in enumerate(zip(docs, got)):
        want = grams(d, clean, stop, n)
        assert g == O.hashing_tf(want, F), (i, repr(d)[:60])
        assert ntok[i] == len(want), (i, repr(d)[:60])
    if device != "cpu":
        host = T.featurize_score(pt, spec, want_csr=True, device="cpu")
        for a, b in zip(host.csr(), res.csr()):
            assert torch.equal(a, b.cpu())


# ------------------------------------------------------------------------------ 3. capacities
def _short_tokens(n):
    out = []
    for k in (1, 2, 3):
        for t in itertools.product(string.ascii_lowercase, repeat=k):
            if "".join(t) not in ENGLISH:
                out.append("".join(t))
            if len(out) == n:
                return out
    raise ValueError(n)


CAP = ["b " * 1024, "b " * 1025, "b " * 16384, "b " * 16385, " ".join(_short_tokens(1024)),
       "word " * 818 + "xy zw", "word " * 819 + "x", "word " * 819 + "xy"]          # 4095, 4096, 4097 bytes
# what the streaming kernel alone says, and the device path with the long-dialogue kernel
CAP_STREAM = [T.STATUS_OK, T.STATUS_TOO_LONG, T.STATUS_TOO_LONG, T.STATUS_TOO_LONG, T.STATUS_OK,
              T.STATUS_OK, T.STATUS_OK, T.STATUS_TOO_LONG]
CAP_DEVICE = [T.STATUS_OK, T.STATUS_OK, T.STATUS_OK, T.STATUS_TOO_LONG, T.STATUS_OK, T.STATUS_OK, T.STATUS_OK, T.STATUS_OK]


@functools.lru_cache(maxsize=None)
def _cap_want():
    return [O.hashing_tf(grams(d, True, True, 2), 1 << 18) for d in CAP]


def test_capacity_documents_stand_on_the_limits():
    assert [len(d.encode()) for d in CAP[5:]] == [4095, 4096, 4097]
    assert [len(kept_tokens(d, True, True)) for d in CAP[:5]] == [1024, 1025, 16384, 16385, 1024]
    want = _cap_want()
    assert want[0] == {O.term_index("b b", 1 << 18): 1023.0}
    assert len(set(grams(CAP[4], True, True, 2))) == 1023 and len(want[4]) > 1000     # a full-width sort


@pytest.mark.parametrize("device", DEVICES)
def test_capacities(device):
    spec = T.FeatureSpec(clean=True, stopwords=list(ENGLISH), num_features=1 << 18, ngram=2)
    pt = T.PackedText.from_strings(CAP)
    if device != "cpu":
        dev = torch.device(device)
        D = len(CAP)
        i32 = dict(dtype=torch.int32, device=dev)
        status = torch.full((D,), -1, **i32)
        out = (torch.zeros(D, **i32), torch.zeros(D, **i32), torch.zeros((D, 1), dtype=torch.float64, device=dev),
               status, torch.empty(1, **i32), torch.empty(1, dtype=torch.float32, device=dev))
        T._launch(native.lib(), pt.to(dev), spec, T._flags(spec, None, None, None, False), None, None, None, out, dev)
        assert status.cpu().tolist() == CAP_STREAM              # the streaming kernel on its own
        res = T.featurize_score(pt, spec, want_csr=True, device=device, fix_fallbacks=False)
        assert res.status.cpu().tolist() == CAP_DEVICE          # 16385 kept tokens are left to the host
    res = T.featurize_score(pt, spec, want_csr=True, device=device)
    assert res.status.cpu().eq(T.STATUS_OK).all()
    for i, (d, g, w) in enumerate(zip(CAP, csr_rows(res), _cap_want())):
        assert g == w, i
        assert len(g) <= len(d.encode()) // 2 + 2
    assert res.ntok.cpu().tolist() == [len(grams(d, True, True, 2)) for d in CAP]


# ------------------------------------------------------------------------------ 4. vocabulary mode
VOCAB = ["ab c", "a bc", "a b", "gift card", "b ", " b", "never seen", "abc", "ab", "c a", "zz top", "ab c a"]


@functools.lru_cache(maxsize=None)
def vocab_docs():
    rng = random.Random(5)
    words = ["a", "b", "c", "ab", "bc", "the", "gift", "card", "is", "", "abc"]
    docs = ["ab c a bc a b ab c a bc", "ab the c a is bc a the the b", "a  b  a  b", "abc", "ab c", "a b a b a b a b c",
            "gift card gift card gift the card", "", "the is", "AB, C! a-bc a.b", "ab c ab c", "a bc a bc", "ab the c ab"]
    docs += [" ".join(rng.choice(words) for _ in range(rng.randint(0, 30))) for _ in range(150)]
    return docs


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("stop", [True, False])
@pytest.mark.parametrize("min_tf", [1.0, 2.0, 0.25])
def test_vocabulary_mode(min_tf, stop, device):
    docs = vocab_docs()
    spec = T.FeatureSpec(clean=True, stopwords=list(ENGLISH) if stop else None, vocab=VOCAB, min_tf=min_tf, ngram=2)
    res = T.featurize_score(T.PackedText.from_strings(docs), spec, want_csr=True, device=device)
    seen = set()
    for i, (d, g) in enumerate(zip(docs, csr_rows(res))):
        want = O.count_vectorize(grams(d, True, stop, 2), VOCAB, min_tf)      # denominator: the n-gram count
        assert g == want, (i, d)
        seen |= set(want)
    if stop:                                   # "a" is a stop word: "ab the c" is the bigram "ab c", "a b" never forms
        assert VOCAB.index("ab c") in seen and not seen & {VOCAB.index("a bc"), VOCAB.index("a b")}
    else:
        assert {VOCAB.index(w) for w in ("ab c", "a bc", "a b")} <= seen
    assert not seen & {VOCAB.index(w) for w in ("never seen", "abc", "ab", "zz top", "ab c a")}


# ------------------------------------------------------------------------------ 5. keys and fit
@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("clean", [True, False])
def test_token_keys_are_ngram_keys(clean, device):
    docs = EDGE + random_docs(100, seed=3) + [kept_exactly(65), "b " * 1030]
    assert any(max(d.encode(), default=0) >= 0x80 for d in docs)       # without cleaning: the host redo
    spec = T.FeatureSpec(clean=clean, stopwords=list(ENGLISH), num_features=1, ngram=2)
    keys, ntok = T.token_keys(T.PackedText.from_strings(docs), spec, device)
    want = [[T.token_key(g) for g in grams(d, clean, True, 2)] for d in docs]
    assert ntok.cpu().tolist() == [len(w) for w in want]
    assert keys.cpu().tolist() == [k for w in want for k in w]
    pair = ("gift", "card")
    b = " ".join(pair).encode()
    k = (O.murmur3_x86_32(b, 42) << 32) | O.murmur3_x86_32(b, 0x9747B28C)
    assert T.token_key(" ".join(pair)) == (k - (1 << 64) if k >= (1 << 63) else k)


def _dialogue_frame(n=200, seed=21):
    pt, y = synth.generate(synth.SynthConfig(n=n, seed=seed))
    raw = TextColumn(pt.strings())
    return Frame({"dialogue": raw, "clean_text": TextColumn.cleaned_from(raw), "labels": y.numpy()})


def _materialised(frame, n=2):
    """The same frame with the NGram stage's input as plain token lists: nothing downstream fuses."""
    toks = [O.remove_stopwords(O.tokenize(s), ENGLISH) for s in frame.column("clean_text").strings]
    return frame.withColumn("filtered_words", TokenColumn(frame.column("clean_text"), tokens=toks))


def _vector_rows(vc):
    ip, ix, v = (t.cpu().numpy() for t in vc.csr())
    return [{int(a): float(b) for a, b in zip(ix[ip[i]:ip[i + 1]], v[ip[i]:ip[i + 1]])} for i in range(len(ip) - 1)]


def test_count_vectorizer_fit_over_ngram_lineage():
    df = _dialogue_frame()
    front = [Tokenizer(inputCol="clean_text", outputCol="words"),
             StopWordsRemover(inputCol="words", outputCol="filtered_words")]
    gram = NGram(n=2, inputCol="filtered_words", outputCol="grams")
    fused = df
    for s in front + [gram]:
        fused = s.transform(fused)
    host = gram.transform(_materialised(df))
    assert fused.column("grams").fusable and not host.column("grams").fusable
    assert fused.column("grams").tokens == host.column("grams").tokens
    assert host.column("grams").tokens[0] == O.ngrams(kept_tokens(df.column("dialogue").strings[0], True, True), 2)
    cv = CountVectorizer(inputCol="grams", outputCol="raw_features", vocabSize=300, minDF=2.0)
    a, b = cv.fit(fused), cv.fit(host)
    assert a.vocabulary == b.vocabulary and len(a.vocabulary) == 300
    assert all(w.count(" ") == 1 for w in a.vocabulary)
    rows = _vector_rows(a.transform(fused).column("raw_features"))
    assert rows == _vector_rows(b.transform(host).column("raw_features"))
    assert rows[0] == O.count_vectorize(host.column("grams").tokens[0], a.vocabulary)


# ------------------------------------------------------------------------------ 6. scores
def random_forest_arrays(num_trees, num_features, depth, K, seed=0, cmp_less=False):
    rng = np.random.default_rng(seed)
    feat, thr, left, right, leaf, roots = [], [], [], [], [], []

    def build(d):
        i = len(feat)
        feat.append(-1); thr.append(0.0); left.append(-1); right.append(-1)      # noqa: E702
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


def score_docs():
    return EDGE + random_docs(200, seed=4) + [kept_exactly(129), "b " * 1025]


@pytest.mark.parametrize("device", DEVICES)
def test_lr_margin_matches_oracle(device):
    docs = score_docs()
    rng = np.random.default_rng(1)
    w, idf = rng.normal(size=1000), rng.random(1000)
    spec = T.FeatureSpec(clean=True, stopwords=list(ENGLISH), num_features=1000, ngram=2)
    pt = T.PackedText.from_strings(docs)
    kw = dict(idf=torch.from_numpy(idf), lr=T.LinearScorer(w, 0.25))
    res = T.featurize_score(pt, spec, device=device, **kw)
    for d, m in zip(docs, res.raw.cpu()[:, 0].numpy()):
        x = {k: v * idf[k] for k, v in O.hashing_tf(grams(d, True, True, 2), 1000).items()}
        assert m == pytest.approx(O.lr_margin(x, w, 0.25), rel=1e-12, abs=1e-12), repr(d)[:40]
    if device != "cpu":
        assert torch.equal(res.raw.cpu(), T.featurize_score(pt, spec, device="cpu", **kw).raw)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("K,cmp_less", [(1, False), (1, True), (2, False), (2, True)])
def test_tree_scores(K, cmp_less, device):
    docs = score_docs()
    arrs = random_forest_arrays(70, 64, 5, K, seed=2 + K, cmp_less=cmp_less)
    spec = T.FeatureSpec(clean=True, stopwords=list(ENGLISH), num_features=64, ngram=2)
    pt = T.PackedText.from_strings(docs)
    host = T.featurize_score(pt, spec, trees=arrs, device="cpu").raw
    if device == "cpu":
        for d, r in zip(docs, host.numpy()):
            x = O.hashing_tf(grams(d, True, True, 2), 64)
            np.testing.assert_allclose(r, host_tree_score(arrs, x, cmp_less), rtol=1e-12)
    else:
        assert torch.equal(T.featurize_score(pt, spec, trees=arrs, device=device).raw.cpu(), host)


# ------------------------------------------------------------------------------ 7. pipeline
def _stages(tf, clf, n=2):
    out = [Tokenizer(inputCol="clean_text", outputCol="words"),
           StopWordsRemover(inputCol="words", outputCol="filtered_words")]
    terms = "filtered_words"
    if n is not None:
        out.append(NGram(n=n, inputCol=terms, outputCol="grams"))
        terms = "grams"
    tf.set("inputCol", terms)
    return out + [tf, IDF(inputCol="raw_features", outputCol="features"), clf]


def _hash_lr(n=2):
    return _stages(HashingTF(outputCol="raw_features", numFeatures=1 << 12),
                   LogisticRegression(featuresCol="features", labelCol="labels", maxIter=20, regParam=0.01), n)


def _cv_dt(n=2):
    return _stages(CountVectorizer(outputCol="raw_features", vocabSize=2000),
                   DecisionTreeClassifier(featuresCol="features", labelCol="labels", maxDepth=4), n)


def _staged(model, frame):
    """Stage by stage over materialised tokens: every stage runs its host path."""
    out = _materialised(frame)
    for s in model.stages[2:]:
        out = s.transform(out)
    return out


@pytest.mark.parametrize("make", [_hash_lr, _cv_dt])
def test_pipeline_fused_equals_staged(make, tmp_path):
    df = _dialogue_frame()
    model = Pipeline(stages=make()).fit(df)
    chain = match_chain(model.stages)
    assert chain is not None and chain[-1] == len(model.stages) and chain[5] is model.stages[2]
    fused, staged = model.transform(df), _staged(model, df)
    assert fused.column("grams").fusable and not staged.column("grams").fusable
    for col in ("raw_features", "features"):
        assert _vector_rows(fused.column(col)) == _vector_rows(staged.column(col)), col
    strings = df.column("dialogue").strings
    want = [O.ngrams(kept_tokens(s, True, True), 2) for s in strings[:20]]
    tf = model.stages[3]
    for g, row in zip(want, _vector_rows(fused.column("raw_features"))):
        assert row == (O.hashing_tf(g, 1 << 12) if isinstance(tf, HashingTF) else O.count_vectorize(g, tf.vocabulary))
    for col in ("rawPrediction", "probability", "prediction"):
        assert torch.equal(torch.as_tensor(fused.column(col)).cpu(), torch.as_tensor(staged.column(col)).cpu()), col
    fp = model.compile()
    assert fp.ngram == 2 and fp.spec(True).ngram == 2
    pred, prob, rp = fp.predict(strings, clean=True)
    assert torch.equal(pred.cpu(), torch.as_tensor(fused.column("prediction")).cpu())
    assert torch.equal(rp.cpu(), torch.as_tensor(fused.column("rawPrediction")).cpu())
    # Spark-layout round trip
    path = tmp_path / "m"
    model.write().overwrite().save(str(path))
    md = json.loads((path / "stages" / f"2_{model.stages[2].uid}" / "metadata" / "part-00000").read_text().splitlines()[0])
    assert md["class"] == "org.apache.spark.ml.feature.NGram"
    assert md["paramMap"]["n"] == 2 and md["paramMap"]["inputCol"] == "filtered_words"
    assert md["defaultParamMap"]["n"] == 2
    assert not (path / "stages" / f"2_{model.stages[2].uid}" / "data").exists()      # a data-less transformer
    again = PipelineModel.load(str(path))
    assert isinstance(again.stages[2], NGram) and again.stages[2].getN() == 2
    out = again.transform(df)
    for col in ("rawPrediction", "prediction"):
        assert torch.equal(torch.as_tensor(out.column(col)).cpu(), torch.as_tensor(fused.column(col)).cpu())
    assert torch.equal(again.compile().predict(strings)[0].cpu(), pred.cpu())


def test_unigram_pipeline_is_unchanged(tmp_path):
    """Without the stage nothing moves: the flags word of a spec that never heard of n-grams, and a
    saved pipeline without a trace of the stage."""
    spec = T.FeatureSpec(clean=True, stopwords=list(ENGLISH), num_features=1 << 12)
    lr = T.LinearScorer(np.zeros(1 << 12), 0.0)
    idf = torch.ones(1 << 12, dtype=torch.float64)
    word = T.FLAG_CLEAN | T.FLAG_WRITE_CSR | T.FLAG_IDF | T.FLAG_LR | T.FLAG_STOPWORDS
    assert T._flags(spec, idf, lr, None, True) == word
    assert T._flags(T.FeatureSpec(clean=True, stopwords=list(ENGLISH), num_features=1 << 12, ngram=1), idf, lr, None,
                    True) == word
    two = T._flags(T.FeatureSpec(clean=True, stopwords=list(ENGLISH), num_features=1 << 12, ngram=2), idf, lr, None, True)
    assert two == word | (1 << 16)
    eight = T.FeatureSpec(ngram=T.NGRAM_MAX)
    assert T._flags(eight, None, None, None, False) & ~T._flags(T.FeatureSpec(), None, None, None, False) == 7 << 16
    assert T._text_flags(spec) == T.FLAG_CLEAN | T.FLAG_STOPWORDS
    df = _dialogue_frame(120)
    model = Pipeline(stages=_hash_lr(None)).fit(df)
    assert model.compile().ngram == 1
    path = tmp_path / "uni"
    model.save(str(path))
    classes = []
    for i, s in enumerate(model.stages):
        text = (path / "stages" / f"{i}_{s.uid}" / "metadata" / "part-00000").read_text()
        assert "NGram" not in text and '"n"' not in text
        classes.append(json.loads(text.splitlines()[0])["class"].rsplit(".", 1)[1])
    assert classes == ["Tokenizer", "StopWordsRemover", "HashingTF", "IDFModel", "LogisticRegressionModel"]


# ------------------------------------------------------------------------------ 8. fallbacks
def test_wider_than_the_kernel_runs_on_the_host():
    n = T.NGRAM_MAX + 1
    df = _dialogue_frame(40)
    stages = [Tokenizer(inputCol="clean_text", outputCol="words"),
              StopWordsRemover(inputCol="words", outputCol="filtered_words"),
              NGram(n=n, inputCol="filtered_words", outputCol="grams"),
              HashingTF(inputCol="grams", outputCol="raw_features", numFeatures=F)]
    assert match_chain(stages) is None
    out = PipelineModel(stages).transform(df)
    assert not out.column("grams").fusable
    want = [O.hashing_tf(O.ngrams(kept_tokens(s, True, True), n), F) for s in df.column("dialogue").strings]
    assert _vector_rows(out.column("raw_features")) == want and any(want)
    with pytest.raises(ValueError):
        PipelineModel(stages).compile()


@pytest.mark.parametrize("device", DEVICES)
def test_dialogue_over_64k_finishes_on_the_host(device):
    docs = ["gift card wire " * 4700, "a short one here"]              # 70,500 bytes, cut points everywhere
    assert len(docs[0]) > T.LONG_DOC_BYTES
    spec = T.FeatureSpec(clean=True, stopwords=list(ENGLISH), num_features=F, ngram=2)
    pt = T.PackedText.from_strings(docs)
    if device != "cpu":
        left = T.featurize_score(pt, spec, want_csr=True, device=device, fix_fallbacks=False)
        assert left.status.cpu().tolist() == [T.STATUS_TOO_LONG, T.STATUS_OK]     # the segmented path declines
    res = T.featurize_score(pt, spec, want_csr=True, device=device)
    assert res.status.cpu().tolist() == [T.STATUS_OK, T.STATUS_OK]
    assert csr_rows(res) == [O.hashing_tf(grams(d, True, True, 2), F) for d in docs]


# ------------------------------------------------------------------------------ 9. streaming
@pytest.mark.gpu
def test_streaming_scorer_matches_fused_predict():
    from fraud_detection_spark_kafka_llm_amd.stream.gpu_worker import GpuScorer
    from fraud_detection_spark_kafka_llm_amd.stream.ring import PinnedRing

    df = _dialogue_frame()
    model = Pipeline(stages=_hash_lr()).fit(df)
    fp = model.compile("cuda:0")
    docs = list(df.column("dialogue").strings)
    docs = docs + random_docs(255 - len(docs), seed=6) + ["please verify your account number " * 150]   # ~5 KB
    assert len(docs) == 256 and 4096 < len(docs[-1]) < 6000
    ring = PinnedRing(slots=1, max_docs=256, max_bytes=1 << 20)
    ring.slots[0].fill(docs)
    gpu = GpuScorer(fp.spec(True), fp.idf.idf, fp.model.scorer(), "cuda:0", max_docs=256, max_bytes=1 << 20)
    raw = gpu.score_packed(ring.slots[0])
    pred, prob, rp = fp.predict(docs, clean=True)
    assert torch.equal(torch.from_numpy(raw), fp.run(docs, clean=True).raw.cpu())
    rp2, _, pred2 = fp.model.postprocess(torch.from_numpy(raw))
    assert torch.equal(rp2, rp.cpu()) and torch.equal(pred2, pred.cpu())
    x = O.hashing_tf(grams(docs[-1], True, True, 2), 1 << 12)
    lr = fp.model.scorer()
    want = O.lr_margin({k: v * fp.idf.idf[k] for k, v in x.items()}, lr.w, lr.b)
    assert raw[-1, 0] == pytest.approx(want, rel=1e-12, abs=1e-12)


# ------------------------------------------------------------------------------ 10. agent
def test_agent_names_bigrams(tmp_path):
    from fraud_detection_spark_kafka_llm_amd.serve.agent import ClassificationAgent
    from fraud_detection_spark_kafka_llm_amd.serve.llm import StubLLM

    df = _dialogue_frame()
    Pipeline(stages=_hash_lr()).fit(df).save(str(tmp_path / "m"))
    agent = ClassificationAgent(str(tmp_path / "m"), llm=StubLLM(), device="cpu")
    dialogue = df.column("dialogue").strings[0]
    words = agent.contributing_words(dialogue, n=10)
    own = set(grams(dialogue, True, True, 2))
    assert words and own
    for e in words:
        parts = e["word"].split("/")
        assert parts and all(p in own and p.count(" ") >= 1 for p in parts)
        assert all(O.term_index(p, agent.fused.dim) == e["feature"] for p in parts)


# ------------------------------------------------------------------------------ 11. sanitizer
@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                    reason="needs hipcc")
def test_ngram_host_twin_clean_under_asan_ubsan():
    exe = _build.build_selftest("ngram", sanitize=True)
    res = subprocess.run([str(exe)], env={**os.environ, **_build.SELFTEST_ENV}, capture_output=True, text=True,
                         timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "ngram selftest ok" in res.stdout
    assert "runtime error" not in res.stderr      # UBSan diagnostics
