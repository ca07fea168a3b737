"""Classification agent (R-16): saved Spark-layout pipeline -> fused gfx950 scorer -> LLM explanation.

Same public surface as the reference's ``DeepSeekClassificationAgent``
(/root/reference/utils/agent_api.py:124-208): ``model``, ``analyzer``, ``historical_data``,
``preprocess_text``, ``predict_and_get_label``, ``classify_and_explain``,
``find_similar_historical_cases`` (and its batched form,
``find_similar_historical_cases_batch``). Differences:

* one fused kernel launch per call (the reference runs two Spark jobs per prediction);
* ``predict_batch`` scores a whole list in one launch (batch CSV tab, streaming);
* ``classify_and_explain`` can reuse an existing prediction, and passes ``temperature`` through;
* ``find_similar_historical_cases`` ranks historical dialogues by cosine similarity of their
  TF-IDF vectors (the reference returns the first ``n`` rows as a placeholder).

``confidence`` keeps the reference's meaning: P(class 1 = fraud), whatever the prediction. A
pipeline with more than two classes (NaiveBayes, multinomial logistic regression; the reference has
none) reports the probability of the predicted class instead.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from ..ml import Frame, PipelineModel, TextColumn
from ..ml.fused import FusedPipeline
from ..ops.sparse import score_csr
from ..ops.text import LinearScorer, PackedText, featurize_score
from ..utils.config import default_device
from ..utils.logging import get_logger
from .llm import Analyzer, make_llm

log = get_logger("agent")


class ClassificationAgent:
    def __init__(self, model_path: str, historical_data_path: Optional[str] = None, llm=None, device=None,
                 analyzer: Optional[Analyzer] = None):
        self.device = torch.device(device) if device is not None else default_device()
        self.model = PipelineModel.load(model_path)
        self.fused: FusedPipeline = self.model.compile(self.device, multiclass=True)
        self.analyzer = analyzer or Analyzer(llm if llm is not None else make_llm())
        self._historical: Optional[Frame] = None
        self._hist_index = None
        self._sim_index = None
        if historical_data_path:
            self.historical_data = Frame.read_csv(historical_data_path)

    # ------------------------------------------------------------------ historical data
    @property
    def historical_data(self) -> Optional[Frame]:
        return self._historical

    @historical_data.setter
    def historical_data(self, frame) -> None:
        if frame is not None and not isinstance(frame, Frame):
            frame = Frame.from_pandas(frame)
        self._historical = frame
        self._hist_index = None
        self._sim_index = None

    # ------------------------------------------------------------------ inference
    def preprocess_text(self, text: str) -> Frame:
        raw = TextColumn([text])
        return Frame({"dialogue": raw, "clean_text": TextColumn.cleaned_from(raw)})

    def predict_batch(self, texts: Sequence[str]) -> list:
        if not len(texts):
            return []
        texts = [t if t is not None else "" for t in texts]
        model = self.fused.model
        if model is not None and model.numClasses > 2:
            # class scores: the decision of the model's postprocess and the probability of the predicted
            # class, computed as the streaming engine computes them (serving_postprocess)
            raw = self.fused.run(texts, clean=True).raw.cpu().numpy()
            pred, conf = model.serving_postprocess(raw)
            return [{"prediction": float(a), "confidence": float(b)} for a, b in zip(pred, conf)]
        pred, prob, _ = self.fused.predict(texts, clean=True)
        pred = pred.cpu().numpy()
        p1 = prob[:, 1].cpu().numpy()
        return [{"prediction": float(a), "confidence": float(b)} for a, b in zip(pred, p1)]

    def predict_and_get_label(self, text: str) -> dict:
        try:
            return self.predict_batch([text])[0]
        except Exception as e:  # keep the reference's contract: prediction even if confidence fails
            log.error("prediction failed: %s", e)
            raise

    def find_similar_historical_cases(self, dialogue: str, n: int = 3):
        hd = self._historical
        if hd is None or hd.count() == 0 or "dialogue" not in hd:
            return None
        if self._hist_index is None:
            texts = [s or "" for s in (hd.column("dialogue").strings if isinstance(hd.column("dialogue"), TextColumn)
                                       else list(hd.column("dialogue")))]
            vc = self._features(texts)
            ip, ix, v = vc.csr()
            norms = torch.zeros(len(texts), dtype=torch.float64, device=v.device)
            row = torch.repeat_interleave(torch.arange(len(texts), device=v.device), ip[1:] - ip[:-1])
            norms.index_add_(0, row, v.double() * v.double())
            self._hist_index = (vc, torch.sqrt(norms))
        vc, norms = self._hist_index
        q = self._features([dialogue])
        qi, qx, qv = q.csr()
        w = np.zeros(q.size)
        w[qx.cpu().numpy()] = qv.cpu().double().numpy()
        qn = float(np.linalg.norm(w))
        if qn == 0:
            return hd.limit(n).collect()
        sims = score_csr(vc, LinearScorer(w, 0.0))[:, 0] / torch.clamp(norms * qn, min=1e-12)
        top = torch.argsort(sims, descending=True, stable=True)[:n].cpu().numpy()
        return hd.take_rows(top).collect()

    def find_similar_historical_cases_batch(self, dialogues: Sequence[str], n: int = 3, with_scores: bool = False):
        """``find_similar_historical_cases`` for a list of dialogues in one featurize launch and one
        exact top-k retrieval (``serve.similar.HistoricalIndex``): one list of historical rows per
        dialogue, best first, ties by historical row number; with ``with_scores`` a
        ``(cases, rows, sims)`` triple with the row numbers and cosine similarities as arrays
        ``[len(dialogues), min(n, N)]``. ``None`` under the single-query method's conditions."""
        hd = self._historical
        if hd is None or hd.count() == 0 or "dialogue" not in hd:
            return None
        if self._sim_index is None:
            from .similar import HistoricalIndex

            self._sim_index = HistoricalIndex(self.fused, hd)
        rows, sims = self._sim_index.query(list(dialogues), n)
        flat = hd.take_rows(rows.reshape(-1)).collect()
        k = rows.shape[1]
        cases = [flat[i * k:(i + 1) * k] for i in range(rows.shape[0])]
        return (cases, rows, sims) if with_scores else cases

    def _features(self, texts):
        fp = self.fused
        idf = fp.idf.idf_tensor(self.device) if fp.idf is not None else None
        res = featurize_score(PackedText.from_strings(texts), fp.spec(True), idf=idf, want_csr=True, device=self.device)
        ip, ix, v = res.csr()
        from ..ml.linalg import VectorColumn

        return VectorColumn(fp.dim, ip, ix, v.to(torch.float64))

    def contributing_words(self, dialogue: str, n: int = 10) -> list:
        """The words of ``dialogue`` that moved the classifier's class-1 score most: dicts with
        ``word``, ``feature``, ``value`` (the TF-IDF value) and ``contribution`` (the model's
        ``contributions``: TreeSHAP for tree models, ``w_f * x_f`` for logistic regression), by
        descending ``|contribution|``, ties by feature index. Only features present in the
        dialogue are listed. CountVectorizer features name their vocabulary word; HashingTF
        buckets name the dialogue's own filtered tokens (its n-grams behind an NGram stage) that
        hash there, joined with ``/``."""
        from ..ml.feature import CountVectorizerModel
        from ..ops import oracle

        fp = self.fused
        if fp.model is None:
            raise ValueError("pipeline has no classifier stage")
        vc = self._features([dialogue])
        _, ix, v = vc.csr()
        col = fp.model.contributions(vc)
        _, cx, cv = col.csr()
        contrib = dict(zip(cx.cpu().tolist(), cv.cpu().tolist()))
        items = [(f, x, contrib[f]) for f, x in zip(ix.cpu().tolist(), v.cpu().tolist()) if f in contrib]
        items.sort(key=lambda t: (-abs(t[2]), t[0]))
        if isinstance(fp.tf, CountVectorizerModel):
            words = {f: fp.tf.vocabulary[f] for f, _, _ in items}
        else:
            toks = oracle.tokenize(oracle.clean_text(dialogue))
            if fp.stopwords is not None:
                toks = oracle.remove_stopwords(toks, fp.stopwords)
            toks = oracle.ngrams(toks, fp.ngram)      # an NGram pipeline's terms are the n-grams
            buckets: dict = {}
            for t in dict.fromkeys(toks):
                buckets.setdefault(oracle.term_index(t, fp.dim), []).append(t)
            words = {f: "/".join(buckets.get(f, [])) for f, _, _ in items}
        return [{"word": words[f], "feature": int(f), "value": float(x), "contribution": float(c)}
                for f, x, c in items[:max(0, int(n))]]

    @staticmethod
    def evidence_paragraph(evidence: Sequence[dict]) -> str:
        listed = ", ".join(f"{e['word']!r} ({e['contribution']:+.4g})" for e in evidence)
        return ("\n\n        **Model Evidence**:\n"
                "        Words of this dialogue with their signed contribution to the classifier's fraud score "
                f"(positive pushes towards fraud, negative away from it), strongest first: {listed}")

    def insight_from_cases(self, dialogue: str, cases, temperature: float = 0.7) -> str:
        """The LLM's comparison of ``dialogue`` with the historical rows ``cases``."""
        cases_str = "\n".join(str(dict(r)) for r in cases)
        return self.analyzer.llm.generate(
            "Compare this new case with historical patterns:\n"
            f"New Case: {dialogue}\n\n"
            f"Historical Similar Cases:\n{cases_str}\n\n"
            "Identify any consistent patterns or anomalies.", temperature)

    def classify_and_explain(self, dialogue: str, temperature: float = 0.7, prediction: Optional[dict] = None,
                             with_history: bool = True, evidence: int = 0, cases=None) -> dict:
        """``cases``: historical rows already looked up for this dialogue (e.g. one element of
        ``find_similar_historical_cases_batch``); when given, no lookup is made."""
        res = prediction or self.predict_and_get_label(dialogue)
        words = self.contributing_words(dialogue, evidence) if evidence > 0 else None
        if words is None:
            analysis = self.analyzer.analyze_prediction(dialogue, res["prediction"], res["confidence"], temperature)
        else:
            prompt = self.analyzer.create_prompt(dialogue, res["prediction"], res["confidence"])
            analysis = self.analyzer.llm.generate(prompt + self.evidence_paragraph(words), temperature)
        insight = None
        if cases is not None or (with_history and self._historical is not None):
            if cases is None:
                cases = self.find_similar_historical_cases(dialogue)
            if cases:
                insight = self.insight_from_cases(dialogue, cases, temperature)
        out = {"prediction": res["prediction"], "confidence": res["confidence"], "analysis": analysis,
               "historical_insight": insight}
        if words is not None:
            out["evidence"] = words
        return out
