"""numpy twin of geossl_eval_collect (csrc/eval_collect.hip): the per-row terms in fp32, each operation rounded on its
own as the kernel forms them, the sums in fp64.

    kind 0 (regression):       d = pred - target, a = |d|, s = d d
    kind 1 (BCE with logits):  z = pred, y = target, a = (max(z, 0) - z y) + log1p(exp(-|z|)), s = 0
"""
import numpy as np

REGRESSION, BCE = 0, 1


def terms(pred, target, kind):
    """-> (a, s) as float32 arrays [B]."""
    p, t = np.asarray(pred, dtype=np.float32).reshape(-1), np.asarray(target, dtype=np.float32).reshape(-1)
    assert p.shape == t.shape
    if kind == REGRESSION:
        d = (p - t).astype(np.float32)
        return np.abs(d), (d * d).astype(np.float32)
    if kind != BCE:
        raise ValueError("kind is 0 or 1")
    lin = (np.maximum(p, np.float32(0)) - (p * t).astype(np.float32)).astype(np.float32)
    soft = np.log1p(np.exp(-np.abs(p)).astype(np.float32)).astype(np.float32)
    return (lin + soft).astype(np.float32), np.zeros_like(p)


def collect(pred, target, kind, offset=0, out_pred=None, out_true=None, acc=None):
    """One launch: `acc` = [sum a, sum s, rows] (floats and an int; None: zeros) with this batch added; the rows
    [offset, offset + B) of the result arrays written in place.  -> acc."""
    a, s = terms(pred, target, kind)
    acc = [0.0, 0.0, 0] if acc is None else list(acc)
    acc[0] += float(a.astype(np.float64).sum())
    acc[1] += float(s.astype(np.float64).sum())
    acc[2] += int(a.size)
    B = a.size
    if out_pred is not None:
        out_pred[offset:offset + B] = np.asarray(pred, dtype=np.float32).reshape(-1)
    if out_true is not None:
        out_true[offset:offset + B] = np.asarray(target, dtype=np.float32).reshape(-1)
    return acc
