"""Float64 restatement of the style-transfer posterior (include/flowtron_hip.h, style transfer; the reference's
inference_style_transfer.ipynb, the cells that form `mu_posterior` and sample from it), in plain numpy, written from the formulas:

    K utterances z_b [M][len_b],   ratio = K / lambd,   c = ratio / (ratio + 1)
    batch            mu[m][t] = c / K  sum_b z_b[m][t mod len_b]                     t < n_frames
    time_and_batch   mu[m]    = c / K  sum_b (1 / len_b) sum_{t < len_b} z_b[m][t]
    sample           out[s][m][t] = mu[m][t] + sigma eps[s][m][t]                    (time_and_batch: mu[m] at every t)

Beside every mean it returns the magnitude sum S the error bounds of the tests are built from: the same expression with |z|
in the place of z."""
import numpy as np

EPS24 = 2.0 ** -24


def shrink(K, lambd):
    ratio = K / float(lambd)
    return ratio / (ratio + 1.0)


def posterior_mean(zs, lambd, aggregation, n_frames=None):
    """zs: K arrays [M, len_b].  -> (mu, S) float64, [M, n_frames] for 'batch' and [M, 1] for 'time_and_batch'."""
    K = len(zs)
    c = shrink(K, lambd)
    zs = [np.asarray(z, np.float64) for z in zs]
    M = zs[0].shape[0]
    if aggregation == "batch":
        acc, mag = np.zeros((M, n_frames)), np.zeros((M, n_frames))
        t = np.arange(n_frames)
        for z in zs:
            tiled = z[:, t % z.shape[1]]
            acc += tiled
            mag += np.abs(tiled)
    elif aggregation == "time_and_batch":
        acc, mag = np.zeros((M, 1)), np.zeros((M, 1))
        for z in zs:
            acc[:, 0] += z.sum(axis=1) / z.shape[1]
            mag[:, 0] += np.abs(z).sum(axis=1) / z.shape[1]
    else:
        raise ValueError(aggregation)
    return c * acc / K, c * mag / K


def sample(mu, S, eps, sigma):
    """mu, S [M, n_frames] or [M, 1]; eps [n, M, n_frames] -> (out, S + |sigma eps|) float64 [n, M, n_frames]."""
    e = float(sigma) * np.asarray(eps, np.float64)
    return mu[None] + e, S[None] + np.abs(e)


def notebook_bound(S, K, aggregation, t_max):
    """What the notebook's own fp32 arithmetic may deviate from float64, per element: K - 1 (time_and_batch: also t_max - 1)
    summation terms in any order, plus the roundings of the division by the count, of ratio, of ratio + 1, of the product and
    of the quotient -- (K + 5) 2^-24 S, or (t_max + K + 5) 2^-24 S."""
    terms = K + 5 if aggregation == "batch" else t_max + K + 5
    return terms * EPS24 * S


def kernel_bound(ref, S):
    """The device result against float64: one rounding to fp32, plus slack for the float64 accumulation ((K + T) 2^-53 is far
    below 2^-45 at any size the tests use)."""
    return EPS24 * np.abs(ref) + 2.0 ** -45 * S
