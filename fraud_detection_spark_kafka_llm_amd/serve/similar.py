"""Similar historical cases for a batch of dialogues: the historical dialogues' TF-IDF vectors as a
``SimIndex`` on the pipeline's device, queried with one featurize launch and one ``topk_cosine``
(csrc/sim_kernels.hip) per batch. Exact and deterministic: see ``ops.sparse.topk_cosine``."""
from __future__ import annotations

from typing import Sequence

import torch

from ..ml import Frame, TextColumn
from ..ml.fused import FusedPipeline
from ..ml.linalg import VectorColumn
from ..ops.sparse import SimIndex, sim_index, sim_limits, topk_cosine
from ..ops.text import PackedText, featurize_score


def featurize(fused: FusedPipeline, texts: Sequence[str]) -> VectorColumn:
    """TF-IDF vectors of ``texts`` by the pipeline's own fused featurizer (cleaning included)."""
    idf = fused.idf.idf_tensor(fused.device) if fused.idf is not None else None
    res = featurize_score(PackedText.from_strings(list(texts)), fused.spec(True), idf=idf, want_csr=True,
                          device=fused.device)
    ip, ix, v = res.csr()
    return VectorColumn(fused.dim, ip, ix, v.to(torch.float64))


class HistoricalIndex:
    def __init__(self, fused: FusedPipeline, frame: Frame, text_col: str = "dialogue", chunk: int = 65536):
        self.fused, self.frame = fused, frame
        col = frame.column(text_col)
        texts = [s or "" for s in (col.strings if isinstance(col, TextColumn) else list(col))]
        ips, ixs, vs, base = [torch.zeros(1, dtype=torch.int64, device=fused.device)], [], [], 0
        for a in range(0, len(texts), max(1, int(chunk))):
            ip, ix, v = featurize(fused, texts[a:a + chunk]).csr()
            ips.append(ip[1:] + base)
            ixs.append(ix)
            vs.append(v)
            base += int(ix.numel())
        cat = (lambda xs, dt: torch.cat(xs) if xs else torch.zeros(0, dtype=dt, device=fused.device))
        vc = VectorColumn(fused.dim, torch.cat(ips), cat(ixs, torch.int32), cat(vs, torch.float64))
        self.index: SimIndex = sim_index(vc)

    @classmethod
    def from_vectors(cls, fused: FusedPipeline, frame: Frame, vc: VectorColumn) -> "HistoricalIndex":
        """An index over already featurized historical dialogues (row ``i`` of ``vc`` = row ``i`` of ``frame``)."""
        self = cls.__new__(cls)
        self.fused, self.frame, self.index = fused, frame, sim_index(vc)
        return self

    def __len__(self) -> int:
        return self.index.rows

    def query(self, texts: Sequence[str], n: int = 3):
        """``(rows int64 [Q, min(n, N)], sims float64 [Q, min(n, N)])`` on the host, best first."""
        import numpy as np

        n = int(n)
        if not 1 <= n <= sim_limits()["k_max"]:
            raise ValueError(f"n must lie in 1 .. {sim_limits()['k_max']}")
        if not len(texts):
            kk = min(n, len(self))
            return np.zeros((0, kk), dtype=np.int64), np.zeros((0, kk), dtype=np.float64)
        rows, sims = topk_cosine(self.index, featurize(self.fused, [t or "" for t in texts]), n)
        return rows.cpu().numpy(), sims.cpu().numpy()

    def cases(self, texts: Sequence[str], n: int = 3) -> list:
        """The ``n`` most similar historical rows of every text, one list of ``Row`` per text."""
        rows, _ = self.query(texts, n)
        flat = self.frame.take_rows(rows.reshape(-1)).collect()
        k = rows.shape[1]
        return [flat[i * k:(i + 1) * k] for i in range(rows.shape[0])]
