"""numpy restatement of the reference's L2 regulariser (modules/regularizers.py:11-18):

    target_weights = [tf.nn.l2_loss(w) for w in weights if not is_black(w.name)]
    l2_loss = sum(target_weights) * scale             tf.nn.l2_loss(w) = sum(w ** 2) / 2

``selected(name)`` plays ``not is_black(w.name)`` (sat_amd.params.is_l2_regularized for the
model's tensors; the blacklist works on TF names, which ours are not).  ``l2_loss64`` is the
float64 reference; ``l2_loss32`` evaluates the same formula in float32 as TF would (every square,
every tensor's sum, the halving, the sum over tensors and the scale rounded to float32): its
deviation from float64 on the same inputs, ``e32``, is float32 arithmetic's own error and sets the
tests' tolerances.  Nothing here runs on the GPU.
"""
import math

import numpy as np

F32 = np.float32


def l2_loss64(weights, scale, selected=lambda name: True) -> float:
    """float64: scale * sum over selected tensors of sum(w^2) / 2 (``scale`` as given)."""
    total = [math.fsum((np.asarray(w, np.float64).ravel() ** 2).tolist()) / 2.0
             for name, w in weights.items() if selected(name)]
    return math.fsum(total) * float(scale)


def l2_loss32(weights, scale, selected=lambda name: True) -> np.float32:
    """The same formula op by op in float32."""
    total = F32(0.0)
    for name, w in weights.items():
        if not selected(name):
            continue
        w = np.asarray(w, F32).ravel()
        sq = w * w
        assert sq.dtype == F32
        total = F32(total + F32(np.sum(sq, dtype=F32) / F32(2.0)))
    return F32(total * F32(scale))


def e32(weights, scale, selected=lambda name: True) -> float:
    """|float32 evaluation - float64 reference| on these inputs."""
    return abs(float(l2_loss32(weights, scale, selected)) - l2_loss64(weights, F32(scale), selected))


def grad64(w, g, grad_weight) -> np.ndarray:
    """g + grad_weight * w in float64 (the regulariser's gradient, scale * w, on top of g)."""
    return np.asarray(g, np.float64) + float(F32(grad_weight)) * np.asarray(w, np.float64)


def ulp32(x) -> np.ndarray:
    """One float32 ulp at |x| (of the float32 nearest to x)."""
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(F32)).astype(np.float64)
