"""The piece of the reference's disco_theque/misc_utils.py that goes with the metrics: the bar-plot data of a result table.
Host NumPy on a handful of numbers, as the reference's."""
import warnings

import numpy as np

from .metrics import ci_wp


def bar_data(x_edges, x, y):
    """misc_utils.py:102-114: gather y into the bins of x -> (means, cis), one value per edge.  Sample i goes to the first bin whose edge
    is not below x[i] (x[i] <= x_edges[b]); a sample above the last edge raises ValueError, as the reference's list.index does.  The mean
    of a bin is np.nanmean and its confidence half-width metrics.ci_wp; an empty bin gives NaN for both, as there (NumPy's warnings
    about the empty bin are not passed on).  With speech_enhancement.results_io.batch_results' (R, K) arrays flattened, this is the
    data of the reference's bar plots: bar_data(edges, res['snr_in_cnv'].ravel(), res['snr_out'].ravel())."""
    x_edges = np.asarray(x_edges)
    bins = [[] for _ in range(len(x_edges))]
    for i in range(len(x)):
        bins[list(x[i] > x_edges).index(False)].append(y[i])
    means, cis = [], []
    with warnings.catch_warnings(), np.errstate(divide='ignore', invalid='ignore'):
        warnings.simplefilter('ignore', RuntimeWarning)
        for b in bins:
            means.append(np.nanmean(b))
            cis.append(ci_wp(b))
    return np.array(means), np.array(cis)
