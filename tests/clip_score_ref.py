"""torchmetrics' clip_score (functional/multimodal/clip_score.py: _clip_score_update + the mean and clamp of clip_score) restated in
numpy float64 from already projected features — torchmetrics is not installed here.  A plain helper module, like image_metrics_ref.py.

    img = img / ||img||;  txt = txt / ||txt||;  score_pair = 100 * sum(img * txt);  clip_score = max(mean(score_pair), 0)
"""
import numpy as np


def pair_scores(image_feats, text_feats) -> np.ndarray:
    i = np.asarray(image_feats, dtype=np.float64)
    t = np.asarray(text_feats, dtype=np.float64)
    i = i / np.linalg.norm(i, axis=-1, keepdims=True)
    t = t / np.linalg.norm(t, axis=-1, keepdims=True)
    return 100.0 * (i * t).sum(axis=-1)


def clip_score(image_feats, text_feats) -> float:
    return float(max(pair_scores(image_feats, text_feats).mean(), 0.0))
