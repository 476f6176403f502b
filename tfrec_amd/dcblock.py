"""CPU restatement of the DC blocker (include/tfrec_amd.h: tfrec_amd_create_dc), in numpy and exact integers.
Written from the definition alone: nothing here calls the C library.

The blocker belongs to an input ROW and acts on x, the int16 value every format maps a stored component to (formats.to_x,
-8192 <= x <= 8191), at the context's input rate -- ahead of the input-rate tune, the resampling stage and everything behind them.

    windows   L = 512 complex samples; window w of a row covers samples [512 w, 512 (w + 1)), counted from the row's first submit
              or its last DC reset
    sums      S_I[w], S_Q[w] = the window's sums of x_I, x_Q                      (|S| <= 2^22)
    estimate  K = avg_windows (1 .. 4096), lo = max(0, w - K + 1), c = w - lo + 1, A = S[lo] + .. + S[w] per rail,
              d[w] = floor((2 A + 512 c) / (1024 c))   -- the mean over c windows, rounded half up; floor, not truncation
    apply     x' = clamp(x - d[w], -8192, 8191) per rail

Window w's own sum is part of A, so a row's first window is already corrected.  The state a row carries from submit to submit is
its last K window sums and its window count: `state` below, (sums int64 [m, 2] with m = min(count, K), count).

No window straddles a submit: a permitted submit of n_blocks blocks at the rate P / Q holds n_blocks 32768 P / Q complex samples;
n_blocks is a multiple of Q / gcd(Q, 64) (resample.permitted_blocks), which makes that k P 512 (64 / gcd(Q, 64)) -- so every submit is a
whole number of windows and the result does not depend on how a row is cut into submits (input_samples asserts it).
"""
from __future__ import annotations

import numpy as np

from . import formats, resample

L = 512
K_MAX = 4096
X_MIN, X_MAX = -8192, 8191


def input_samples(n_blocks: int, p: int = 1, q: int = 1) -> int:
    """resample.input_samples, with the argument above asserted: a permitted submit is a whole number of windows."""
    n = resample.input_samples(n_blocks, p, q) if (p, q) != (1, 1) else int(n_blocks) * 32768
    assert n % L == 0, "a permitted submit of %d blocks at %d/%d would cut a window" % (n_blocks, p, q)
    return n


def _check_k(k) -> int:
    k = int(k)
    if not 1 <= k <= K_MAX:
        raise ValueError("avg_windows %d outside [1, %d]" % (k, K_MAX))
    return k


def fresh_state():
    """A row before its first submit or after a DC reset."""
    return np.zeros((0, 2), dtype=np.int64), 0


def window_sums(x) -> np.ndarray:
    """x, interleaved int16 (I, Q) of a whole number of windows -> int64 [windows, 2]."""
    x = np.asarray(x, dtype=np.int16).reshape(-1, 2)
    assert len(x) % L == 0
    return x.astype(np.int64).reshape(-1, L, 2).sum(axis=1)


def estimate(sums, k, state=None):
    """This submit's window sums behind the carried state -> (d int16 [windows, 2], the state behind them)."""
    k = _check_k(k)
    ring, count = fresh_state() if state is None else state
    s = np.asarray(sums, dtype=np.int64).reshape(-1, 2)
    m = len(ring)
    assert m == min(count, k)
    allsum = np.concatenate([ring, s])
    cs = np.concatenate([np.zeros((1, 2), dtype=np.int64), np.cumsum(allsum, axis=0)])
    j = m + np.arange(len(s))  # the window's place in allsum; its absolute number is count + its place in s
    c = np.minimum(count + np.arange(len(s)) + 1, k)
    a = cs[j + 1] - cs[j + 1 - c]
    d = (2 * a + (L * c)[:, None]) // (2 * L * c)[:, None]  # numpy's // on int64 is floor division
    assert d.min(initial=0) >= X_MIN and d.max(initial=0) <= X_MAX
    return d.astype(np.int16), (allsum[max(0, len(allsum) - k):].copy(), count + len(s))


def apply(x, d) -> np.ndarray:
    """x (interleaved int16) and its windows' d [windows, 2] -> x', interleaved int16."""
    x = np.asarray(x, dtype=np.int16).reshape(-1, L, 2).astype(np.int32)
    d = np.asarray(d, dtype=np.int16).reshape(-1, 1, 2).astype(np.int32)
    assert len(x) == len(d)
    return np.clip(x - d, X_MIN, X_MAX).astype(np.int16).reshape(-1)


def dc_block(raw, fmt, k, state=None):
    """One submit's row of bytes in the format -> (x' interleaved int16, d int16 [windows, 2], the row's state behind it)."""
    x = formats.to_x(fmt, raw)
    d, state = estimate(window_sums(x), k, state)
    return apply(x, d), d, state


def dc_block_bruteforce(raw, fmt, k, state=None):
    """dc_block sample by sample in Python integers, with a floor division written out: what the vectorised form is tested
    against."""
    k = _check_k(k)
    ring, count = fresh_state() if state is None else state
    hist = [(int(a), int(b)) for a, b in ring]
    x = [int(v) for v in formats.to_x(fmt, raw)]
    assert len(x) % (2 * L) == 0
    out, ds = [], []
    for w0 in range(0, len(x), 2 * L):
        s = [0, 0]
        for i in range(L):
            s[0] += x[w0 + 2 * i]
            s[1] += x[w0 + 2 * i + 1]
        hist.append((s[0], s[1]))
        count += 1
        c = min(count, k)
        d = []
        for rail in range(2):
            num, den = 2 * sum(h[rail] for h in hist[-c:]) + L * c, 2 * L * c
            quo = abs(num) // den  # truncation of the magnitudes ...
            if num < 0:
                quo = -quo - (1 if abs(num) % den else 0)  # ... made a floor
            d.append(quo)
        ds.append(d)
        for i in range(L):
            for rail in range(2):
                out.append(min(X_MAX, max(X_MIN, x[w0 + 2 * i + rail] - d[rail])))
        hist = hist[-k:]
    return (np.array(out, dtype=np.int16), np.array(ds, dtype=np.int16).reshape(-1, 2),
            (np.array(hist, dtype=np.int64).reshape(-1, 2), count))
