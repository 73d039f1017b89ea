"""utils/ops.py of the reference: the helper the metrics need."""
import numpy as np


def onehot_encode(target):
    """One-hot rows (int32 [n, max(target) + 1]) of a label vector
    (utils/ops.py:42-51)."""
    labels = np.asarray(target).astype(np.int32).reshape(-1)
    out = np.zeros((labels.shape[0], int(labels.max()) + 1), dtype=np.int32)
    out[np.arange(labels.shape[0]), labels] = 1
    return out
