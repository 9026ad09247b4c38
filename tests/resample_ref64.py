"""Float64 restatement of the resampler's definition (include/flowtron_hip.h, sample-rate conversion), in plain numpy and
independent of flowtron_amd.audio's tap builder: a loop over output samples.

    n_out = (n new + orig - 1) // orig,   base = 0.99 min(orig, new),   W = 6
    y[m]  = sum_{0 <= k < n} h(k / orig - m / new) x[k]
    h(t)  = (base / orig) sinc(base t) cos^2(pi base t / (2 W))  for |base t| < W, else 0;   sinc(u) = sin(pi u) / (pi u)

The argument base t is formed from the exact integer num = k new - m orig as base * num / (orig * new), and the window test
|base t| < W is the integer comparison 99 min(orig, new) |num| < 100 W orig new, so a tap depends on num alone."""
import math

import numpy as np

W = 6


def out_len(n, orig, new):
    return (n * new + orig - 1) // orig


def h64(num, orig, new):
    """h at t = num / (orig new) seconds."""
    mn = min(orig, new)
    if 99 * mn * abs(num) >= 100 * W * orig * new:
        return 0.0
    base = 0.99 * mn
    t = base * num / (orig * new)
    s = 1.0 if t == 0.0 else math.sin(math.pi * t) / (math.pi * t)
    return (base / orig) * s * math.cos(math.pi * t / (2 * W)) ** 2


def window(m, orig, new, cache=None):
    """The inputs under output m, whatever the signal's length: (k_lo, [h(k / orig - m / new) for k = k_lo ...]), every k whose
    tap is inside |base t| < W.  `cache` (a dict) keeps the taps by num."""
    reach = int(math.ceil(W * orig / (0.99 * min(orig, new)))) + 2
    centre = (m * orig) // new
    ks = [k for k in range(centre - reach, centre + reach + 1)
          if 99 * min(orig, new) * abs(k * new - m * orig) < 100 * W * orig * new]
    hs = []
    for k in ks:
        num = k * new - m * orig
        if cache is None:
            hs.append(h64(num, orig, new))
        else:
            if num not in cache:
                cache[num] = h64(num, orig, new)
            hs.append(cache[num])
    assert ks == list(range(ks[0], ks[-1] + 1))
    return ks[0], np.asarray(hs, dtype=np.float64)


def resample64(x, orig, new, round_taps=False):
    """x [n] -> (y [n_out] float64, sum_k |h x| [n_out]).  round_taps: the taps rounded to fp32 first (what the kernel multiplies
    by), the sums still in float64."""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    n_out = out_len(n, orig, new)
    y = np.zeros(n_out)
    mag = np.zeros(n_out)
    cache = {}
    for m in range(n_out):
        k_lo, h = window(m, orig, new, cache)
        if round_taps:
            h = h.astype(np.float32).astype(np.float64)
        a, b = max(k_lo, 0), min(k_lo + len(h), n)
        if a < b:
            prod = h[a - k_lo:b - k_lo] * x[a:b]
            y[m] = prod.sum()
            mag[m] = np.abs(prod).sum()
    return y, mag


def phase_table(orig, new):
    """The polyphase view of the same definition, from `window` alone: (taps float64 [new_g, K], first input offset [new_g],
    orig_g, new_g, K) where output m = q new_g + p reads x[q orig_g + offset[p] + i] against taps[p, i]."""
    g = math.gcd(orig, new)
    og, ng = orig // g, new // g
    rows = [window(p, orig, new) for p in range(ng)]
    K = max(len(h) for _, h in rows)
    taps = np.zeros((ng, K))
    for p, (_, h) in enumerate(rows):
        taps[p, :len(h)] = h
    return taps, np.asarray([k for k, _ in rows], dtype=np.int64), og, ng, K


def dc_gain(orig, new):
    """sum of every phase's taps: what a constant input is multiplied by, per phase [new_g]."""
    return phase_table(orig, new)[0].sum(axis=1)
