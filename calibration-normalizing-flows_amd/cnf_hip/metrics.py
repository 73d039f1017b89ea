"""Calibration scoring on the device: NLL, ECE, accuracy and the reliability
diagram of a probability matrix (the reference's utils/metrics.py:6-15, 35-80)
from one integer record of 4 + 3 * bins words (cnf_metrics, include/cnf.h):

    [0] n_rows  [1] n_invalid  [2] nll_fx  [3] n_correct
    [4 .. 4+bins) rows per bin   [4+bins .. 4+2*bins) conf_fx per bin
    [4+2*bins .. 4+3*bins) correct rows per bin

`*_fx` words are sums of rint(value * 2^32) with the value widened to double
first.  Every word is an integer sum, so records of batches or shards add word
by word (cnf_hip.dist.sharded_calibration_record) and the result does not
depend on how the rows were split.

`calibration_record` fills the record: one native launch for an fp32 tensor on
a ROCm device (the probabilities never leave the device), a torch restatement
of the same integer arithmetic for any other tensor (CPU tensors, gloo ranks,
float64 inputs).  `CalibrationSums` turns a record into float64 numbers on the
host with one copy of the record.
"""
import ctypes

import numpy as np
import torch

from . import _lib, engine

FX = 4294967296.0  # 2^32: the fixed-point scale of the *_fx words
MAX_ROWS = 1 << 26


def record_words(bins):
    bins = int(bins)
    if not 1 <= bins <= _lib.MAX_BINS:
        raise ValueError("bins must be 1..%d" % _lib.MAX_BINS)
    return 4 + 3 * bins


def _edges(bins):
    """The reference's bin edges, formed in double (metrics.py:57-61)."""
    width = 1. / bins
    return [i * width for i in range(bins + 1)]


def _torch_record(probs, y, bins, record):
    """The record of cnf_metrics as torch ops on any device: the same
    integer sums, on the values widened to double."""
    D = probs.shape[1]
    p = probs.detach().to(torch.float64)
    y = y.reshape(-1)
    finite = torch.isfinite(p).all(dim=1)
    in_range = (y >= 0) & (y < D)
    # p[y] selected by comparing the column index with the label
    cols = torch.arange(D, device=p.device).unsqueeze(0)
    py = torch.where(cols == y.unsqueeze(1), p, torch.zeros_like(p)).sum(dim=1)
    valid = finite & in_range
    valid = valid & (torch.where(valid, py, torch.ones_like(py)) + 1e-7 > 0)
    p, y, py = p[valid], y[valid], py[valid]
    pred = torch.argmax(p, dim=1)  # the first maximal index, as np.argmax
    conf = p.gather(1, pred.unsqueeze(1)).squeeze(1)
    hit = (pred == y).to(torch.int64)
    nll_fx = torch.round(-torch.log(py + 1e-7) * FX).to(torch.int64)
    conf_fx = torch.round(conf * FX).to(torch.int64)
    # bin i: edges[i] < conf <= edges[i + 1]
    edges = torch.tensor(_edges(bins), dtype=torch.float64, device=p.device)
    k = torch.bucketize(conf, edges, right=False)
    binned = (k >= 1) & (k <= bins)
    b = (k - 1)[binned]
    add = torch.zeros_like(record)
    add[0] = p.shape[0]
    add[1] = probs.shape[0] - p.shape[0]
    add[2] = nll_fx.sum()
    add[3] = hit.sum()
    add[4:4 + bins].index_add_(0, b, torch.ones_like(b))
    add[4 + bins:4 + 2 * bins].index_add_(0, b, conf_fx[binned])
    add[4 + 2 * bins:4 + 3 * bins].index_add_(0, b, hit[binned])
    record += add
    return record


def _labels_and_record(B, dev, y, bins, record):
    """(y, record) under the record rules every scoring call shares: int64
    labels on `dev`, one per row, at most 2^26 rows; a zeroed record when
    None, else a contiguous int64 [4 + 3 * bins] tensor on `dev`."""
    words = record_words(bins)
    if B > MAX_ROWS:
        raise ValueError("at most 2^26 rows per call (split the batch; records add)")
    y = torch.as_tensor(y).to(device=dev, dtype=torch.int64).reshape(-1)
    if y.shape[0] != B:
        raise ValueError("y must hold one label per row")
    if record is None:
        record = torch.zeros(words, dtype=torch.int64, device=dev)
    elif (record.dtype != torch.int64 or record.device != dev or record.numel() != words
          or not record.is_contiguous()):
        raise ValueError("record must be a contiguous int64 [%d] tensor on %s" % (words, dev))
    return y, record


def score_args(x, y, bins, record):
    """(y, bins, record) of a fused score call on the [B, D] ROCm tensor x (the
    *_score entry points, include/cnf.h), under calibration_record's rules;
    the record is added to."""
    y, record = _labels_and_record(x.shape[0], x.device, y, bins, record)
    return y.contiguous(), int(bins), record


def calibration_record(probs, y, bins=15, record=None):
    """ADD the calibration record of (probs [B, D], y [B]) into `record` (a
    zeroed int64 [4 + 3 * bins] tensor on probs' device when None) and return
    it.  A ROCm fp32 `probs` takes ONE native launch (cnf_metrics, on the
    current stream, graph-capturable); any other tensor the torch restatement."""
    record_words(bins)  # bins in range, before anything else is looked at
    bins = int(bins)
    if probs.dim() != 2 or not 2 <= probs.shape[1] <= _lib.MAX_DIM:
        raise ValueError("probs must be [B, D] with 2 <= D <= %d" % _lib.MAX_DIM)
    B, dev = probs.shape[0], probs.device
    y, record = _labels_and_record(B, dev, y, bins, record)
    if not (probs.is_cuda and probs.dtype == torch.float32):
        return _torch_record(probs, y, bins, record)
    probs = probs.detach().contiguous()
    y = y.contiguous()
    ops = engine._ops()
    if ops is not None:
        ops.metrics(probs, y, bins, record)
        engine.stats["torch_ops"] += 1
    else:
        with torch.cuda.device(dev):
            st = _lib.lib().cnf_metrics(engine._ptr(probs), engine._ptr(y),
                                        ctypes.c_int32(probs.shape[1]), ctypes.c_int32(bins),
                                        ctypes.c_int64(B), engine._ptr(record),
                                        ctypes.c_void_p(0), ctypes.c_size_t(0),
                                        engine._stream(dev))
        _lib.check("cnf_metrics", st)
    engine.stats["metrics"] += 1
    return record


class CalibrationSums:
    """Host view of a calibration record (one D2H copy of 4 + 3 * bins words);
    every value is float64."""

    def __init__(self, record, bins=None):
        if torch.is_tensor(record):
            record = record.detach().cpu().numpy()
        rec = np.asarray(record).astype(np.int64).reshape(-1)
        if bins is None:
            bins = (rec.size - 4) // 3
        bins = int(bins)
        if rec.size != record_words(bins):
            raise ValueError("a record of %d bins has %d words" % (bins, 4 + 3 * bins))
        self.record, self.bins = rec, bins
        self.n = int(rec[0])
        self.n_invalid = int(rec[1])
        self.n_correct = int(rec[3])
        self.bin_count = rec[4:4 + bins]
        self.bin_conf_fx = rec[4 + bins:4 + 2 * bins]
        self.bin_correct = rec[4 + 2 * bins:4 + 3 * bins]

    def _mean(self, num):
        return float(num) / self.n if self.n else float("nan")

    def nll(self):
        """mean(-log(p[y] + 1e-7)) (metrics.py:15); NaN when a row was invalid."""
        if self.n_invalid:
            return float("nan")
        return self._mean(float(self.record[2]) / FX)

    def accuracy(self):
        """metrics.py:80."""
        return self._mean(self.n_correct)

    def ece(self):
        """sum_b |acc_b - conf_b| * count_b / n (metrics.py:60-71), as
        sum_b |correct_b - conf_fx_b * 2^-32| / n."""
        gap = np.abs(self.bin_correct.astype(np.float64) - self.bin_conf_fx.astype(np.float64) / FX)
        return self._mean(gap.sum())

    def reliability(self):
        """(count, mean confidence, accuracy) per bin: the reliability
        diagram's arrays (NaN where a bin is empty)."""
        cnt = self.bin_count.astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            conf = self.bin_conf_fx.astype(np.float64) / FX / cnt
            acc = self.bin_correct.astype(np.float64) / cnt
        return self.bin_count.copy(), conf, acc

    def as_dict(self):
        return {"nll": self.nll(), "ece": self.ece(), "accuracy": self.accuracy(), "n": self.n}
