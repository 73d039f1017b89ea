"""Drop-in mirror of the reference's `utils` package for the scoring step:
`utils.metrics` (NLL, ECE, accuracy, empirical cross entropy) and the one
helper of `utils.ops` it needs (`onehot_encode`).  Out of scope: utils/data.py,
utils/visualization.py and the temperature optimiser of utils/ops.py."""
