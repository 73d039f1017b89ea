"""The detection view of a calibrator (Ramos et al., Entropy 2018, 20, 208):
one-vs-rest log-likelihood ratios (the reference's utils/ops.py:54-66) and the
empirical cross-entropy curve over a grid of prior log-odds (the loops of
utils/visualization.py:431-571 around utils/metrics.py:18-32), computed from
per-column raw sums so that one pass over the B x cols ratios serves every
class's curve and the flattened (all classes together) curve:

    sums   [cols][2][P]  sum over the positives of softplus(-theta) / ln 2,
                         sum over the negatives of softplus(+theta) / ln 2,
                         theta = ln LR + ln(prior odds)
    counts [cols + 2]    positives per column, n_valid, n_invalid

Everything is float64 torch arithmetic on HOST tensors, in the log domain
(softplus(z) = max(z, 0) + log1p(exp(-|z|)), so +-inf and NaN ratios flow
through as log2(1 + ratio) carries them).  There is no device kernel for
these sums yet: a ROCm tensor is refused here, and the
drop-in functions of utils/ and calibrators.py copy device values to the host
first.  `EceCurveSums` turns the sums into curves with NumPy.
"""
import numpy as np
import torch

from . import _lib

LN2 = 0.6931471805599453094
MAX_PRIORS = 128  # points of one curve


def _host_only(t, what):
    if t.is_cuda:
        raise NotImplementedError(
            "%s: no device kernel serves the detection view yet; copy the tensor to the host"
            % what)


# ---- log-likelihood ratios ------------------------------------------------------
def log_likelihood_ratios(logits, priors):
    """One-vs-rest log-likelihood ratios [B, D] (float64, natural log) of the
    host tensor `logits` [B, D] under the class `priors` [D]:
    -log(sum_{i != c} priors_i / (1 - priors_c) * exp(x_i - x_c)), evaluated as
    (x_c - max) - log(S_c) + log1p(-priors_c) with S_c = sum_{i != c} priors_i
    exp(x_i - max) formed from an exclusive prefix plus an exclusive suffix
    sum: additions only (a dominant class does not cancel against a full row
    sum) and D exps per row instead of D^2."""
    _host_only(logits, "log_likelihood_ratios")
    if logits.dim() != 2 or not 2 <= logits.shape[1] <= _lib.MAX_DIM:
        raise ValueError("logits must be [B, D] with 2 <= D <= %d" % _lib.MAX_DIM)
    D = logits.shape[1]
    pr = torch.as_tensor(np.asarray(priors, dtype=np.float64) if not torch.is_tensor(priors)
                         else priors).to(dtype=torch.float64).reshape(-1)
    if pr.numel() != D:
        raise ValueError("priors must hold %d values" % D)
    x = logits.detach().to(torch.float64)
    t = x - x.max(dim=1, keepdim=True).values
    w = pr * torch.exp(t)
    zero = torch.zeros_like(w[:, :1])
    pre = torch.cat([zero, torch.cumsum(w, dim=1)[:, :-1]], dim=1)
    suf = torch.cat([zero, torch.cumsum(w.flip(1), dim=1)[:, :-1]], dim=1).flip(1)
    return t - torch.log(pre + suf) + torch.log1p(-pr)


# ---- curve sums -----------------------------------------------------------------
def prior_axis(range=(-2.5, 2.5), bins=100):
    """ECE_plot's axis of prior log10-odds (visualization.py:459)."""
    return np.linspace(range[0], range[1], num=bins)


def _theta(log10_odds, odds=None, priors=None):
    """(odds, priors, ln odds) of the axis, formed as the reference's loop
    forms them: odds = 10**t, prior = odds / (1 + odds), unless the caller
    knows them exactly."""
    t = np.asarray(log10_odds, dtype=np.float64).reshape(-1)
    if odds is None:
        odds = [10 ** v for v in t]  # scalar pow, as the loop's
    odds = np.asarray(odds, dtype=np.float64).reshape(-1)
    priors = odds / (1. + odds) if priors is None else \
        np.asarray(priors, dtype=np.float64).reshape(-1)
    if odds.size != t.size or priors.size != t.size:
        raise ValueError("odds and priors must hold one value per point of the axis")
    with np.errstate(divide="ignore"):
        return odds, priors, np.log(odds)


def _softplus(z):
    return torch.clamp(z, min=0) + torch.log1p(torch.exp(-z.abs()))


def ece_curve_raw(log_lr, y, n_labels, theta):
    """(sums [cols, 2, P] float64, counts [cols + 2] int64) of the host
    tensors log_lr [B, cols] and y [B] for theta [P] = ln(prior odds).  A row
    whose label lies outside [0, n_labels) counts in n_invalid and in nothing
    else."""
    _host_only(log_lr, "ece_curve_raw")
    log_lr = log_lr.detach().to(torch.float64)
    B, cols = log_lr.shape
    P = theta.numel()
    sums = torch.zeros(cols, 2, P, dtype=torch.float64)
    counts = torch.zeros(cols + 2, dtype=torch.int64)
    valid = (y >= 0) & (y < n_labels)
    counts[cols] = valid.sum()
    counts[cols + 1] = B - counts[cols]
    cidx = torch.arange(cols)
    zero = torch.zeros((), dtype=torch.float64)
    step = max(1, (1 << 22) // (cols * P))  # rows per pass: bounded temporaries
    for s in range(0, B, step):
        l, yy, ok = log_lr[s:s + step], y[s:s + step], valid[s:s + step]
        pos = (yy.unsqueeze(1) == cidx) & ok.unsqueeze(1)          # [b, cols]
        neg = ~pos & ok.unsqueeze(1)
        z = l.unsqueeze(2) + theta                                 # [b, cols, P]
        v = _softplus(torch.where(pos.unsqueeze(2), -z, z))
        sums[:, 0] += torch.where(pos.unsqueeze(2), v, zero).sum(dim=0)
        sums[:, 1] += torch.where(neg.unsqueeze(2), v, zero).sum(dim=0)
        counts[:cols] += pos.sum(dim=0)
    return sums / LN2, counts


def ece_curve_sums(log_lr, y, log10_odds, n_labels=None, odds=None, priors=None):
    """EceCurveSums of ln LR `log_lr` ([B, cols], or [B] for one column)
    against the labels `y` [B] over the axis `log10_odds` of prior
    log10-odds: element (r, c) is a positive iff y[r] == c.  `n_labels`
    (default: cols, or 2 for one column) bounds the valid labels; the binary
    form of ratios against a 0/1 target is one column, n_labels = 2 and
    y = 1 - target.  `odds` / `priors`: the prior odds and priors of the
    points when the caller holds them exactly (default: 10**log10_odds and
    odds / (1 + odds))."""
    if log_lr.dim() == 1:
        log_lr = log_lr.reshape(-1, 1)
    if log_lr.dim() != 2 or not 1 <= log_lr.shape[1] <= _lib.MAX_DIM:
        raise ValueError("log_lr must be [B, cols] with 1 <= cols <= %d" % _lib.MAX_DIM)
    B, cols = log_lr.shape
    if n_labels is None:
        n_labels = cols if cols > 1 else 2
    n_labels = int(n_labels)
    if n_labels < cols:
        raise ValueError("n_labels must be at least the number of columns")
    odds, priors, theta = _theta(log10_odds, odds, priors)
    if not 1 <= theta.size <= MAX_PRIORS:
        raise ValueError("the axis must hold 1..%d points" % MAX_PRIORS)
    y = torch.as_tensor(y).to(dtype=torch.int64).reshape(-1)
    if y.shape[0] != B:
        raise ValueError("y must hold one label per row")
    sums, counts = ece_curve_raw(log_lr, y, n_labels, torch.from_numpy(theta))
    return EceCurveSums(sums.numpy(), counts.numpy(), log10_odds, odds, priors)


class EceCurveSums:
    """Host view of the sums of an empirical cross-entropy curve; every value
    is float64.  `log10_odds` is the axis, `priors` the prior of each point."""

    def __init__(self, sums, counts, log10_odds, odds=None, priors=None):
        self.log10_odds = np.asarray(log10_odds, dtype=np.float64).reshape(-1)
        self.odds, self.priors, _ = _theta(self.log10_odds, odds, priors)
        self.sums = np.asarray(sums, dtype=np.float64)
        self.counts = np.asarray(counts).astype(np.int64).reshape(-1)
        self.cols = self.sums.shape[0]
        if self.sums.shape != (self.cols, 2, self.priors.size) or \
                self.counts.size != self.cols + 2:
            raise ValueError("sums must be [cols, 2, P] and counts [cols + 2]")
        self.n_pos = self.counts[:self.cols]
        self.n = int(self.counts[self.cols])
        self.n_invalid = int(self.counts[self.cols + 1])

    def _ece(self, pos, neg, n_pos, n_neg):
        """metrics.py:28-30 from the two sums; 0 / 0 is NaN, as there."""
        if self.n_invalid:
            return np.full(self.priors.shape, np.nan)
        with np.errstate(invalid="ignore", divide="ignore"):
            return self.priors / np.float64(n_pos) * pos + \
                (1 - self.priors) / np.float64(n_neg) * neg

    def curve(self, c):
        """The curve [P] of column c alone (ECE_plot of np.exp(LRs[:, c])
        against target == c)."""
        n_pos = int(self.n_pos[c])
        return self._ece(self.sums[c, 0], self.sums[c, 1], n_pos, self.n - n_pos)

    def curves(self):
        """[cols, P]: curve(c) of every column."""
        return np.stack([self.curve(c) for c in range(self.cols)])

    def flat(self):
        """The curve [P] of all columns scored together against the one-hot
        target (ECE_plot's flattened 2-D input)."""
        n_pos = int(self.n_pos.sum())
        return self._ece(self.sums[:, 0].sum(axis=0), self.sums[:, 1].sum(axis=0), n_pos,
                         self.n * self.cols - n_pos)

    def reference(self):
        """The curve of LR = 1 (ECE_plot's dotted line): a function of the
        prior alone."""
        with np.errstate(divide="ignore"):
            return self.priors * np.log2(1 + 1. / self.odds) + \
                (1 - self.priors) * np.log2(1 + self.odds)
