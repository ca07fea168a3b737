"""Multi-class serving: C linear class scores in the fused featurize+score launch, through
``FusedPipeline(multiclass=True)``, the agent and the streaming scorers.

The contract (README "Multi-class serving"): for a dialogue's sorted unique terms ``u_j`` and fp64
values ``v_j``, ``x_j = (double)(float)v_j`` (the value the CSR scratch stores), lane ``l`` of 64 sums
``x_j * W[u_j, c]`` over ``j = l, l + 64, ...`` in ascending order (multiply, then add), the 64 partials
meet in the xor butterfly (offsets 32 .. 1) and ``b_c`` is added last. That is ``nb_score``'s order, so
the class scores are bitwise ``score_csr`` of the launch's own CSR. A scorer with ``exact=True`` (the
models' ``class_scorer()``) takes ``x_j = v_j`` instead: ``score_csr`` of the staged pipeline's fp64
feature column, which is what ``transform`` gives. Every equality here is bitwise.
"""
import functools
import json

import numpy as np
import pytest
import torch

from fraud_detection_spark_kafka_llm_amd.ml.linalg import VectorColumn
from fraud_detection_spark_kafka_llm_amd.ops import native, oracle, sparse
from fraud_detection_spark_kafka_llm_amd.ops import text as T

DEVICES = [pytest.param("cpu", id="host"), pytest.param("cuda:0", id="device", marks=pytest.mark.gpu)]
EDGE_TERMS = [0, 1, 63, 64, 65, 129]     # distinct terms: none, one lane, a full wave and its neighbours, three rounds
BATCHES = [1, 3, 4, 5, 257]              # either side of the 4-wave workgroup, and many workgroups
CLASSES = [2, 3, 8]
STOP = ["the"]


def bits(a) -> np.ndarray:
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def word(i: int) -> str:
    """Letters only (cleaning keeps them), never a stop word: 'q' + three base-26 digits."""
    return "q" + "".join(chr(97 + (i // 26 ** k) % 26) for k in range(3))


@functools.lru_cache(maxsize=None)
def pool(num_features: int, n: int = 420) -> tuple:
    """``n`` words whose HashingTF buckets differ, so a dialogue's distinct words are distinct terms."""
    out, seen = [], set()
    for i in range(26 ** 3):
        b = oracle.term_index(word(i), num_features)
        if b not in seen:
            seen.add(b)
            out.append(word(i))
            if len(out) == n:
                return tuple(out)
    raise AssertionError("not enough distinct buckets")


# ---------------------------------------------------------------------------------------------- NumPy contract
LANES = np.arange(64)


def lane_partials(terms: np.ndarray) -> np.ndarray:
    """64 lane-strided partial sums of ``terms [n, ...]``: lane l adds terms l, l + 64, ... in that order."""
    part = np.zeros((64,) + terms.shape[1:])
    for r in range(0, len(terms), 64):
        blk = terms[r:r + 64]
        part[:len(blk)] = part[:len(blk)] + blk
    return part


def butterfly(part: np.ndarray) -> np.ndarray:
    """Lane 0 of the xor butterfly over the 64 partials (offsets 32, 16, .., 1)."""
    for o in (32, 16, 8, 4, 2, 1):
        part = part + part[LANES ^ o]
    return part[0]


def class_scores_numpy(ip, ix, val, W, b, exact: bool = False) -> np.ndarray:
    """The contract over a CSR of the fp64 values ``v_j`` (or of their stored fp32 roundings)."""
    out = np.empty((len(ip) - 1, W.shape[1]))
    for d, (s, e) in enumerate(zip(ip[:-1], ip[1:])):
        x = val[s:e].astype(np.float64) if exact else val[s:e].astype(np.float32).astype(np.float64)
        out[d] = butterfly(lane_partials(x[:, None] * W[ix[s:e]])) + b
    return out


def csr_numpy(res) -> tuple:
    return tuple(t.cpu().numpy() for t in res.csr())


# ---------------------------------------------------------------------------------------------- 1. kernel = contract
def edge_doc(words, k: int, ngram: int) -> str:
    """A dialogue with exactly ``k`` distinct terms (``k`` distinct n-grams of distinct words)."""
    if k == 0:
        return "the the"
    return " ".join(words[: k + ngram - 1])


@functools.lru_cache(maxsize=None)
def config(name: str):
    """(spec, idf, texts) of a featurizer configuration; the first six dialogues hold EDGE_TERMS terms."""
    rng = np.random.default_rng(7)
    kw = dict(clean=True, stopwords=list(STOP))
    if name == "hash-idf":
        spec = T.FeatureSpec(num_features=1 << 14, **kw)
    elif name == "hash-binary":
        spec = T.FeatureSpec(num_features=1 << 14, binary=True, **kw)
    elif name == "vocab-mintf":
        spec = T.FeatureSpec(vocab=list(pool(1 << 14)[:300]), min_tf=0.005, **kw)
    elif name == "bigram":
        spec = T.FeatureSpec(num_features=1 << 16, ngram=2, **kw)
    else:
        raise KeyError(name)
    words = pool(1 << 14)
    texts = [edge_doc(words, k, spec.ngram) for k in EDGE_TERMS]
    while len(texts) < max(BATCHES):
        n = int(rng.integers(1, 300))
        src = words[:200] if rng.random() < 0.7 else words[180:330]     # some words outside the vocabulary
        toks = list(rng.choice(src, size=n)) + ["the"] * int(rng.integers(0, 3))
        texts.append(" ".join(rng.permutation(toks)).upper() if rng.random() < 0.2 else " ".join(rng.permutation(toks)))
    idf = None if name == "hash-binary" else torch.from_numpy(rng.random(spec.dim) * 3.0 + 0.25)
    return spec, idf, tuple(texts)


def class_scorer(dim: int, C: int, seed: int = 11) -> T.ClassLinearScorer:
    """Random signs and magnitudes over six decades: a wrong order of the adds shows in the low bits."""
    rng = np.random.default_rng(seed + C)
    W = rng.standard_normal((dim, C)) * 10.0 ** rng.uniform(-3, 3, size=(dim, C))
    return T.ClassLinearScorer(W, rng.standard_normal(C))


@functools.lru_cache(maxsize=None)
def host_reference(name: str, C: int):
    """The host twin's result for the whole batch and the NumPy contract over its CSR (computed once)."""
    spec, idf, texts = config(name)
    cs = class_scorer(spec.dim, C)
    host = T.featurize_score(T.PackedText.from_strings(list(texts)), spec, idf=idf, classes=cs, want_csr=True,
                             device="cpu")
    assert int((host.status != 0).sum()) == 0
    ip, ix, v = csr_numpy(host)
    return cs, host, class_scores_numpy(ip, ix, v, cs.W, cs.b)


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("C", CLASSES)
@pytest.mark.parametrize("name", ["hash-idf", "hash-binary", "vocab-mintf", "bigram"])
def test_class_scores_equal_the_contract(name, C, dev):
    spec, idf, texts = config(name)
    cs, host, ref = host_reference(name, C)
    assert host.nnz[: len(EDGE_TERMS)].tolist() == EDGE_TERMS
    if name == "vocab-mintf":       # the fractional minTF drops terms somewhere, and keeps the edge rows whole
        plain = T.featurize_score(T.PackedText.from_strings(list(texts)), T.FeatureSpec(
            clean=True, stopwords=list(STOP), vocab=spec.vocab), want_csr=True, device="cpu")
        assert int((plain.nnz > host.nnz).sum()) > 50
    assert host.raw.shape == (len(texts), C) and np.array_equal(bits(host.raw), bits(ref))
    for n in BATCHES:
        pt = T.PackedText.from_strings(list(texts[:n]))
        res = T.featurize_score(pt, spec, idf=idf, classes=cs, want_csr=True, device=dev)
        assert res.raw.shape == (n, C) and int((res.status != 0).sum()) == 0
        assert np.array_equal(bits(res.raw), bits(ref[:n])), f"batch of {n}: kernel != NumPy contract"
        assert np.array_equal(bits(res.raw), bits(host.raw[:n])), f"batch of {n}: kernel != host twin"
        ip, ix, v = res.csr()
        assert v.dtype == torch.float32
        again = sparse.score_csr(VectorColumn(spec.dim, ip, ix, v), cs)
        assert np.array_equal(bits(res.raw), bits(again)), f"batch of {n}: kernel != score_csr of its own CSR"
        bare = T.featurize_score(pt, spec, idf=idf, classes=cs, device=dev)        # no CSR written
        assert np.array_equal(bits(bare.raw), bits(res.raw))
        assert torch.equal(bare.nnz.cpu(), host.nnz[:n]) and torch.equal(bare.ntok.cpu(), host.ntok[:n])
    # exact=True: the fp64 values themselves, i.e. score_csr of the staged pipeline's fp64 feature column
    ex = T.ClassLinearScorer(cs.W, cs.b, exact=True)
    ip, ix, v64 = term_values(texts, spec, idf)
    want = class_scores_numpy(ip, ix, v64, cs.W, cs.b, exact=True)
    col = VectorColumn(spec.dim, torch.from_numpy(ip), torch.from_numpy(ix), torch.from_numpy(v64))
    assert np.array_equal(bits(sparse.score_csr(col, ex)), bits(want))
    res = T.featurize_score(T.PackedText.from_strings(list(texts)), spec, idf=idf, classes=ex, device=dev)
    assert np.array_equal(bits(res.raw), bits(want))
    assert np.array_equal(bits(want), bits(ref)) == (idf is None)      # without IDF the values are fp32-exact


def test_the_order_of_the_adds_matters_for_these_weights():
    """The cases above can tell a wrong order: a plain left-to-right sum differs in some row."""
    cs, host, ref = host_reference("hash-idf", 3)
    ip, ix, v = csr_numpy(host)
    seq = np.array([(v[s:e].astype(np.float64)[:, None] * cs.W[ix[s:e]]).sum(axis=0) + cs.b
                    for s, e in zip(ip[:-1], ip[1:])])
    assert not np.array_equal(bits(seq), bits(ref))


# ---------------------------------------------------------------------------------------------- 2. capacities
def exact_bytes(words, n: int, rng) -> str:
    s = " ".join(rng.choice(words, size=n // 4 + 8))[:n]
    return s[:-1] + "x" if s.endswith(" ") else s


@functools.lru_cache(maxsize=None)
def capacity_texts() -> tuple:
    rng = np.random.default_rng(23)
    words = pool(1 << 14)[:150]
    letters = "bcdefghij"
    texts = [exact_bytes(words, 4096, rng), exact_bytes(words, 4097, rng),
             " ".join(letters[i % 9] for i in range(1024)), " ".join(letters[i % 9] for i in range(1025)),
             exact_bytes(words, 70000, rng), "hello there", "", exact_bytes(words, 300, rng)]
    assert [len(t) for t in texts[:2]] == [4096, 4097] and len(texts[4]) > T.LONG_DOC_BYTES
    return tuple(texts)


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("ngram", [1, 2])
def test_long_dialogues_carry_class_scores(ngram, dev):
    """4096 / 4097 cleaned bytes and 1024 / 1025 kept tokens (the long-dialogue relaunch), one dialogue
    over 64 KB (the segmented path; with an NGram stage the host finish)."""
    texts = list(capacity_texts())
    spec = T.FeatureSpec(clean=True, stopwords=list(STOP), num_features=1 << 14, ngram=ngram)
    idf = torch.from_numpy(np.random.default_rng(3).random(spec.dim) + 0.5)
    cs = class_scorer(spec.dim, 3)
    host = T.featurize_score(T.PackedText.from_strings(texts), spec, idf=idf, classes=cs, want_csr=True, device="cpu")
    assert host.ntok[2:4].tolist() == [1024 - (ngram - 1), 1025 - (ngram - 1)]
    ip, ix, v = csr_numpy(host)
    ref = class_scores_numpy(ip, ix, v, cs.W, cs.b)
    assert np.array_equal(bits(host.raw), bits(ref))
    for want_csr in (False, True):
        res = T.featurize_score(T.PackedText.from_strings(texts), spec, idf=idf, classes=cs, want_csr=want_csr, device=dev)
        assert res.status.cpu().tolist() == [T.STATUS_OK] * len(texts)
        assert res.raw.shape == (len(texts), 3) and np.array_equal(bits(res.raw), bits(host.raw))
        assert torch.equal(res.nnz.cpu(), host.nnz)
    rp, rx, rv = csr_numpy(res)
    assert np.array_equal(rp, ip) and np.array_equal(rx, ix) and np.array_equal(rv, v)


# ---------------------------------------------------------------------------------------------- 3. existing modes
def term_values(texts, spec, idf) -> tuple:
    """(indptr, indices, fp64 values v_j = count (or 1) * idf) of the host featurizer: the counts come
    from a launch without IDF (exact integers in fp32), the product is taken here in fp64."""
    counts = T.featurize_score(T.PackedText.from_strings(list(texts)), spec, want_csr=True, device="cpu")
    ip, ix, c = csr_numpy(counts)
    v = c.astype(np.float64)
    return ip, ix, (v * idf.numpy()[ix] if idf is not None else v)


def stumps(dim: int, n_trees: int, K: int, seed: int = 5) -> T.TreeArrays:
    """``n_trees`` depth-1 trees over random features (more trees than lanes, so lanes hold two)."""
    rng = np.random.default_rng(seed)
    feat = np.full(3 * n_trees, -1, dtype=np.int32)
    thr = np.zeros(3 * n_trees)
    left = np.zeros(3 * n_trees, dtype=np.int32)
    right = np.zeros(3 * n_trees, dtype=np.int32)
    roots = np.arange(n_trees, dtype=np.int32) * 3
    words = pool(dim, min(200, dim // 2))
    feat[roots] = [oracle.term_index(w, dim) for w in rng.choice(words, size=n_trees)]
    thr[roots] = rng.uniform(0.2, 4.0, size=n_trees)
    left[roots], right[roots] = roots + 1, roots + 2
    leaf = rng.standard_normal((3 * n_trees, K)) * 10.0 ** rng.uniform(-3, 3, size=(3 * n_trees, K))
    return T.TreeArrays(feat, thr, left, right, leaf, roots, rng.uniform(0.1, 1.0, size=n_trees), K, cmp_less=False)


@pytest.mark.parametrize("dev", DEVICES)
def test_lr_and_tree_scores_are_the_fp64_order_they_were(dev):
    """``classes=None`` leaves the binary tails alone: the margin is the lane-order sum of the fp64 ``v_j w``
    (no rounding of ``v`` to fp32), the tree sums the lane-order sum of ``weight * leaf``."""
    spec, idf, texts = config("hash-idf")
    rng = np.random.default_rng(2)
    lr = T.LinearScorer(rng.standard_normal(spec.dim) * 10.0 ** rng.uniform(-3, 3, size=spec.dim), -0.375)
    assert T._flags(spec, idf, lr, None, False) & T.FLAG_CLASSES == 0
    assert T._flags(spec, idf, None, None, False, class_scorer(spec.dim, 2)) == \
        T._flags(spec, idf, None, None, False) | T.FLAG_CLASSES == T._flags(spec, idf, None, None, False) | (1 << 11)
    ip, ix, v = term_values(texts, spec, idf)
    margin = np.array([butterfly(lane_partials(v[s:e] * lr.w[ix[s:e]])) + lr.b for s, e in zip(ip[:-1], ip[1:])])
    pt = T.PackedText.from_strings(list(texts))
    res = T.featurize_score(pt, spec, idf=idf, lr=lr, device=dev)
    assert res.raw.shape == (len(texts), 1) and np.array_equal(bits(res.raw[:, 0]), bits(margin))
    v32 = v.astype(np.float32).astype(np.float64)
    rounded = np.array([butterfly(lane_partials(v32[s:e] * lr.w[ix[s:e]])) + lr.b for s, e in zip(ip[:-1], ip[1:])])
    assert not np.array_equal(bits(rounded), bits(margin))       # the two contracts differ, so this test can tell
    for K in (1, 2):
        tr = stumps(spec.dim, 70, K)
        sums = np.empty((len(texts), K))
        for d, (s, e) in enumerate(zip(ip[:-1], ip[1:])):
            x = dict(zip(ix[s:e].tolist(), v[s:e].tolist()))
            go_left = np.array([x.get(int(f), 0.0) <= t for f, t in zip(tr.feat[tr.roots], tr.thr[tr.roots])])
            leaves = np.where(go_left, tr.left[tr.roots], tr.right[tr.roots])
            sums[d] = butterfly(lane_partials(tr.tree_weights[:, None] * tr.leaf.reshape(-1, K)[leaves]))
        res = T.featurize_score(pt, spec, idf=idf, trees=tr, device=dev)
        assert res.raw.shape == (len(texts), K) and np.array_equal(bits(res.raw), bits(sums))


# ---------------------------------------------------------------------------------------------- 4. pipelines
WORDS = [[f"{name}{i}" for i in range(12)] for name in ("bank", "prize", "parcel")]
COMMON = [f"talk{i}" for i in range(40)]


@functools.lru_cache(maxsize=None)
def dialogues(C=3):
    """A synthetic dialogue frame of ``C`` kinds: common words and a few words of the row's own kind."""
    from fraud_detection_spark_kafka_llm_amd.ml import Frame, TextColumn

    rng = np.random.default_rng(41)
    n = 420
    y = rng.integers(0, C, size=n)
    texts = []
    for c in y:
        own = rng.choice(WORDS[c], size=rng.integers(1, 4))
        other = rng.choice(WORDS[(c + 1) % C], size=int(rng.random() < 0.15))
        words = np.concatenate([rng.choice(COMMON, size=rng.integers(8, 30)), own, other])
        texts.append(" ".join(rng.permutation(words)))
    raw = TextColumn(texts)
    df = Frame({"dialogue": raw, "clean_text": TextColumn.cleaned_from(raw), "labels": y.astype(np.float64)})
    return df.take_rows(np.arange(300)), df.take_rows(np.arange(300, n))


@functools.lru_cache(maxsize=None)
def pipeline_model(kind: str, C=3):
    from fraud_detection_spark_kafka_llm_amd.ml import (IDF, HashingTF, LogisticRegression, NaiveBayes, Pipeline,
                                                        StopWordsRemover, Tokenizer)

    last = NaiveBayes(featuresCol="features", labelCol="labels") if kind == "nb" else \
        LogisticRegression(featuresCol="features", labelCol="labels", regParam=0.01, maxIter=40,
                           family="multinomial" if kind == "mlr" else "auto")
    stages = [Tokenizer(inputCol="clean_text", outputCol="words"),
              StopWordsRemover(inputCol="words", outputCol="filtered_words"),
              HashingTF(inputCol="filtered_words", outputCol="raw_features", numFeatures=4096),
              IDF(inputCol="raw_features", outputCol="features"), last]
    return Pipeline(stages=stages).fit(dialogues(C)[0])


def column(frame, name) -> np.ndarray:
    c = frame.column(name)
    return (c.cpu().numpy() if isinstance(c, torch.Tensor) else np.asarray(c)).astype(np.float64)


def held_out_texts(C=3) -> list:
    return list(dialogues(C)[1].column("dialogue").strings)


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("kind", ["nb", "mlr"])
def test_multiclass_compile_equals_transform(kind, dev, monkeypatch):
    monkeypatch.setenv("FDX_DEVICE", dev)          # transform's single launch and postprocess on the same device
    model, test = pipeline_model(kind), dialogues()[1]
    assert model.stages[-1].numClasses == 3
    out = model.transform(test)
    fp = model.compile(device=dev, multiclass=True)
    pred, prob, rp = fp.predict(held_out_texts(), clean=True)
    assert rp.shape == prob.shape == (len(test), 3) and pred.shape == (len(test),)
    for name, got in (("rawPrediction", rp), ("probability", prob), ("prediction", pred)):
        assert np.array_equal(bits(got), bits(column(out, name))), name
    vc = out.column("features")                    # the lazy feature column, read after the fact
    assert np.array_equal(bits(rp), bits(sparse.score_csr(vc, model.stages[-1].class_scorer())))
    assert set(pred.cpu().tolist()) == {0.0, 1.0, 2.0}
    with pytest.raises(ValueError, match="3 classes"):
        model.compile(device=dev)
    with pytest.raises(ValueError, match="3 classes"):
        model.stages[-1].scorer()
    assert isinstance(model.stages[-1].serving_scorer(), T.ClassLinearScorer)


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("kind", ["nb", "mlr", "lr"])
def test_binary_models_serve_as_before_with_multiclass(kind, dev):
    model = pipeline_model(kind, 2)
    m = model.stages[-1]
    assert m.numClasses == 2 and isinstance(m.serving_scorer(), T.LinearScorer) and m.serving_scorer() is m.scorer()
    texts = held_out_texts(2)
    a = model.compile(device=dev).predict(texts, clean=True)
    b = model.compile(device=dev, multiclass=True).predict(texts, clean=True)
    for x, y in zip(a, b):
        assert x.shape == y.shape and np.array_equal(bits(x), bits(y))
    raw = model.compile(device=dev).run(texts, clean=True).raw.cpu().numpy()
    for x, y in zip(m.serving_postprocess(raw), m.postprocess_numpy(raw)):
        assert np.array_equal(bits(x), bits(y))


@pytest.mark.parametrize("dev", DEVICES)
def test_naive_bayes_thresholds_are_honoured(dev):
    from fraud_detection_spark_kafka_llm_amd.ml import PipelineModel

    base = pipeline_model("nb")
    texts = held_out_texts()
    plain = base.compile(device=dev, multiclass=True).predict(texts, clean=True)
    thr = [0.9, 1e-6, 0.9]                         # class 1 wins wherever its probability is not tiny
    nb = base.stages[-1].copy({"thresholds": thr})
    model = PipelineModel(list(base.stages[:-1]) + [nb])
    pred, prob, rp = model.compile(device=dev, multiclass=True).predict(texts, clean=True)
    assert np.array_equal(bits(rp), bits(plain[2])) and np.array_equal(bits(prob), bits(plain[1]))
    p = prob.cpu().numpy()
    want = np.argmax(p / np.asarray(thr), axis=1).astype(np.float64)
    assert np.array_equal(pred.cpu().numpy(), want) and not np.array_equal(want, plain[0].cpu().numpy())
    spred, conf = nb.serving_postprocess(rp.cpu().numpy())
    cpu_prob = nb.postprocess(rp.cpu())[1].numpy()
    assert np.array_equal(spred, nb.postprocess(rp.cpu())[2].numpy())
    assert np.array_equal(bits(conf), bits(cpu_prob[np.arange(len(texts)), spred.astype(int)]))


# ---------------------------------------------------------------------------------------------- 5. streaming
def slot_texts() -> list:
    """200 dialogues: the held-out ones, one over 4 KB (long-dialogue relaunch), one over 64 KB (segments)."""
    rng = np.random.default_rng(19)
    texts = (held_out_texts() * 2)[:200]
    vocab = COMMON + WORDS[0] + WORDS[2]
    texts[17] = " ".join(rng.choice(vocab, size=900))
    texts[101] = " ".join(rng.choice(vocab, size=12000))
    assert 4096 < len(texts[17]) <= T.LONG_DOC_BYTES < len(texts[101])
    return texts


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("kind", ["nb", "mlr"])
def test_streaming_scorer_carries_class_scores(kind, dev):
    from fraud_detection_spark_kafka_llm_amd.stream.gpu_worker import make_scorer
    from fraud_detection_spark_kafka_llm_amd.stream.ring import PinnedRing

    model = pipeline_model(kind)
    m = model.stages[-1]
    fp = model.compile(device=dev, multiclass=True)
    texts = slot_texts()
    want = fp.run(texts, clean=True).raw.cpu().numpy()
    assert want.shape == (200, 3)
    sc = make_scorer(fp.spec(True), fp.idf.idf, m.serving_scorer(), dev, max_docs=256, max_bytes=256 * 4096, depth=2)
    ring = PinnedRing(slots=2, max_docs=256, max_bytes=256 * 4096)
    assert ring.slots[0].fill(texts) == 200
    got = sc.score_packed(ring.slots[0])
    assert got.shape == (200, 3) and np.array_equal(bits(got), bits(want))
    # two slots in flight, collected in order
    assert ring.slots[1].fill(texts[::-1]) == 200
    sc.submit(ring.slots[0])
    sc.submit(ring.slots[1])
    assert sc.inflight == 2
    first, second = sc.collect()[1], sc.collect()[1]
    assert np.array_equal(bits(first), bits(want)) and np.array_equal(bits(second), bits(want[::-1]))
    pred, conf = m.serving_postprocess(first)
    _, prob, p = m.postprocess(torch.from_numpy(want))
    assert np.array_equal(pred, p.numpy()) and np.array_equal(bits(conf), bits(prob.numpy().max(axis=1)))


def test_scorers_reject_what_they_cannot_score():
    from fraud_detection_spark_kafka_llm_amd.stream.gpu_worker import GpuScorer, HostScorer

    spec = T.FeatureSpec(num_features=64)
    nine = T.ClassLinearScorer(np.zeros((64, 9)), np.zeros(9))
    with pytest.raises(ValueError, match="2 to 8 classes"):
        HostScorer(spec, None, nine, max_docs=4, max_bytes=1024).score_packed(_one_slot())
    with pytest.raises(TypeError):
        GpuScorer(spec, None, object(), "cpu")


def _one_slot():
    from fraud_detection_spark_kafka_llm_amd.stream.ring import PinnedRing

    ring = PinnedRing(slots=1, max_docs=4, max_bytes=1024, pin=False)
    ring.slots[0].fill(["hello there"])
    return ring.slots[0]


@pytest.mark.parametrize("dev", DEVICES)
def test_engine_and_agent_serve_three_classes(dev, tmp_path):
    from fraud_detection_spark_kafka_llm_amd.serve.agent import ClassificationAgent
    from fraud_detection_spark_kafka_llm_amd.serve.llm import StubLLM
    from fraud_detection_spark_kafka_llm_amd.stream import fake_kafka
    from fraud_detection_spark_kafka_llm_amd.stream.engine import StreamingEngine

    model = pipeline_model("nb")
    model.save(str(tmp_path / "m"))
    agent = ClassificationAgent(str(tmp_path / "m"), llm=StubLLM(), device=dev)
    texts = held_out_texts()
    labels = agent.predict_batch(texts)
    pred, prob, _ = (t.cpu().numpy() for t in model.compile(device="cpu", multiclass=True).predict(texts, clean=True))
    assert [r["prediction"] for r in labels] == pred.tolist() and {0.0, 1.0, 2.0} == set(pred.tolist())
    assert [r["confidence"] for r in labels] == prob.max(axis=1).tolist()
    i2 = int(np.flatnonzero(pred == 2.0)[0])
    one = agent.predict_and_get_label(texts[i2])
    assert one == {"prediction": 2.0, "confidence": float(prob[i2, 2])} == labels[i2]
    with pytest.raises((ValueError, NotImplementedError)):      # contributions stay binary-only
        agent.contributing_words(texts[0])
    # the engine over the in-memory broker
    url = f"memory://multiclass-{dev.replace(':', '-')}"
    broker = fake_kafka.broker_for(url)
    broker.create_topic("in", 3)
    p = fake_kafka.Producer({"bootstrap.servers": url})
    for i, t in enumerate(texts):
        p.produce("in", key=f"k{i}", value=json.dumps({"text": t}))
    c = fake_kafka.Consumer({"bootstrap.servers": url, "group.id": "g", "auto.offset.reset": "earliest",
                             "enable.auto.commit": False})
    c.subscribe(["in"])
    eng = StreamingEngine.from_agent(agent, c, fake_kafka.Producer({"bootstrap.servers": url}), "out", batch_max=32,
                                     max_latency_ms=1)
    st = eng.run(idle_timeout_s=0.3)
    assert st["messages"] == len(texts) and st["produced"] == len(texts) and st["delivery_errors"] == 0
    recs = {m.key(): json.loads(m.value()) for m in broker.messages("out")}
    for i, t in enumerate(texts):
        r = recs[f"k{i}".encode()]
        assert r["original_text"] == t
        assert (r["prediction"], r["confidence"]) == (labels[i]["prediction"], labels[i]["confidence"]), i
    got = c.committed([fake_kafka.TopicPartition("in", q) for q in range(3)])
    assert [tp.offset for tp in got] == [len(broker.topics["in"][q]) for q in range(3)]


# ---------------------------------------------------------------------------------------------- 6. errors
def native_call(spec, W, b, flags, lr_w=None, device="cpu"):
    """The binding itself, with outputs that would show a launch: status stays -1 if nothing ran."""
    pt = T.PackedText.from_strings(["hello there", "you won a prize"]).to(device)
    i32 = dict(dtype=torch.int32, device=device)
    C = W.shape[1] if W is not None and W.ndim == 2 else 1
    status = torch.full((2,), -1, **i32)
    out = (torch.zeros(1, **i32), torch.zeros(1, dtype=torch.float32, device=device), torch.zeros(2, **i32),
           torch.zeros(2, **i32), torch.zeros((2, max(C, 1)), dtype=torch.float64, device=device), status)
    try:
        native.lib().featurize_score(pt.data, pt.offsets, flags, spec.dim, None, None, 1.0, None, lr_w, 0.0, None, 1,
                                     *out, None, 0, None, W, b)
    finally:
        assert status.cpu().tolist() == [-1, -1], "a launch ran"


@pytest.mark.parametrize("dev", DEVICES)
def test_bad_class_scorers_raise_before_any_launch(dev):
    spec = T.FeatureSpec(clean=True, num_features=256)
    pt = T.PackedText.from_strings(["hello there"])
    good = class_scorer(256, 3)
    with pytest.raises(ValueError, match="one scorer per launch"):
        T.featurize_score(pt, spec, lr=T.LinearScorer(np.zeros(256), 0.0), classes=good, device=dev)
    with pytest.raises(ValueError, match="one scorer per launch"):
        T.featurize_score(pt, spec, trees=stumps(256, 2, 1), classes=good, device=dev)
    with pytest.raises(ValueError, match="2 to 8 classes"):
        T.featurize_score(pt, spec, classes=T.ClassLinearScorer(np.zeros((256, 9)), np.zeros(9)), device=dev)
    with pytest.raises(ValueError, match="longer than the feature space"):
        T.featurize_score(pt, spec, classes=class_scorer(257, 3), device=dev)
    # a model with fewer features than the TF stage is padded with rows of zeros, not refused
    short = T.featurize_score(pt, spec, classes=class_scorer(100, 3), device=dev)
    assert short.raw.shape == (1, 3) and int(short.status[0]) == 0
    # the binding checks for itself
    flags = T.FLAG_CLEAN | T.FLAG_CLASSES
    W = torch.zeros((256, 3), dtype=torch.float64, device=dev)
    b = torch.zeros(3, dtype=torch.float64, device=dev)
    with pytest.raises(RuntimeError, match="one scorer per launch"):
        native_call(spec, W, b, flags | T.FLAG_LR, lr_w=torch.zeros(256, dtype=torch.float64, device=dev), device=dev)
    with pytest.raises(RuntimeError, match="2 .. 8 classes"):
        native_call(spec, torch.zeros((256, 9), dtype=torch.float64, device=dev),
                    torch.zeros(9, dtype=torch.float64, device=dev), flags, device=dev)
    with pytest.raises(RuntimeError, match="fewer rows than the feature space"):
        native_call(spec, W[:255].contiguous(), b, flags, device=dev)
    with pytest.raises(RuntimeError, match="float64"):
        native_call(spec, W.to(torch.float32), b, flags, device=dev)
    with pytest.raises(RuntimeError, match="contiguous"):
        native_call(spec, torch.zeros((3, 256), dtype=torch.float64, device=dev).t(), b, flags, device=dev)
    with pytest.raises(RuntimeError, match="one entry per class"):
        native_call(spec, W, b[:2].contiguous(), flags, device=dev)
    with pytest.raises(RuntimeError, match="need W and b"):
        native_call(spec, None, None, flags, device=dev)
    with pytest.raises(RuntimeError, match="without the class-score flag"):
        native_call(spec, W, b, T.FLAG_CLEAN, device=dev)
