"""The canonical-CSR check of the real library's entry points that take CSR arrays, once, for the stand-in libraries:
TEST INFRASTRUCTURE ONLY.  A message is `prefix` + the library's text (terse: without the place); None: nothing wrong."""

import numpy as np


def indptr_message(prefix, ip, cap=None, terse=False):
    """cap: the entries the index and value arrays can hold, where known."""
    if ip[0] != 0:
        return prefix + 'indptr[0] must be 0'
    d = np.diff(ip)
    if np.any(d < 0):
        return prefix + ('indptr decreases' if terse else 'indptr decreases at row %d' % int(np.argmax(d < 0)))
    if cap is not None and int(ip[-1]) > cap:
        return prefix + ("indptr's last entry (%d) is not the number of stored entries (the index and value "
                         'arrays hold at most %d)' % (int(ip[-1]), cap))
    return None


def columns_message(prefix, ip, ix, n_cols, terse=False):
    """Inside [0, n_cols) and strictly ascending in every row (ip has passed); the first row at fault is named."""
    rows = np.repeat(np.arange(len(ip) - 1), np.diff(ip))
    bad = (ix < 0) | (ix >= n_cols)
    if bad.any():
        return prefix + ('column index out of range' if terse else 'column index out of range in row %d' % int(rows[bad].min()))
    bad = (np.diff(ix) <= 0) & (rows[1:] == rows[:-1])
    if bad.any():
        return prefix + ('the columns of a row must ascend strictly' if terse else
                         'the columns of row %d must ascend strictly (no duplicates)' % int(rows[1:][bad].min()))
    return None


def message(prefix, ip, ix, n_cols, cap=None, terse=False):
    return indptr_message(prefix, ip, cap, terse) or columns_message(prefix, ip, ix, n_cols, terse)
