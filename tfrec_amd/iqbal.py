"""CPU restatement of the IQ balancer (include/tfrec_amd.h: tfrec_amd_create_iq), in numpy and exact integers.
Written from the definition alone: nothing here calls the C library.

The balancer belongs to an input ROW, as the DC blocker does (dcblock.py), and acts behind it: on x' = clamp(x - d[w]), at the
context's input rate, ahead of the input-rate tune, the resampling stage and everything behind them.

    windows   those of the DC blocker: L = 512 complex samples, counted from the row's first submit or its last reset; d[w] is the
              blocker's estimate for window w, (0, 0) without a blocker
    moments   on the UNCLAMPED u = x - d[w]:  A[w] = sum u_I^2, B[w] = sum u_Q^2, C[w] = sum u_I u_Q        (A, B, |C| <= 2^37)
              -- from five raw sums of the window, S_I, S_Q, M_II, M_QQ, M_IQ:
                  A = M_II - 2 d_I S_I + 512 d_I^2,  B likewise,  C = M_IQ - d_I S_Q - d_Q S_I + 512 d_I d_Q
    sums      K = iq_windows (1 .. 4096), lo = max(0, w - K + 1); SA, SB, SC = the sums of A, B, C over windows lo .. w
    estimate  s = max(0, bitlen(max(SA, SB)) - 31); a, b, c = SA >> s, SB >> s, SC >> s (arithmetic);
              D = a b - c^2, r = isqrt(D) (the exact floor),
              t = floor((c 32768 + a) / (2 a)),  g = floor((a 32768 + r) / (2 r))                          (Q14: C / A, A / sqrt(AB - C^2))
              the identity t = 0, g = 16384 if a == 0, D <= 0, |t| > 4096, g < 12288 or g > 20480
    apply     on x':  I'' = I',  v = (Q' 16384 - t I' + 8192) >> 14,  Q'' = clamp((v g + 8192) >> 14, -8192, 8191)

The state a row carries from submit to submit is the DC blocker's (dcblock.py) and, for the balancer, its last K triples (A, B, C)
and its window count: (int64 [m, 3] with m = min(count, K), count).  No window straddles a submit (dcblock.input_samples), so the
result does not depend on how a row is cut into submits.
"""
from __future__ import annotations

import math

import numpy as np

from . import dcblock, formats

L = dcblock.L
K_MAX = 4096
X_MIN, X_MAX = dcblock.X_MIN, dcblock.X_MAX
T_MAX, G_MIN, G_MAX, G_ONE = 4096, 12288, 20480, 16384


def _check_k(k) -> int:
    k = int(k)
    if not 1 <= k <= K_MAX:
        raise ValueError("iq_windows %d outside [1, %d]" % (k, K_MAX))
    return k


def fresh_state():
    """A row's balancer before its first submit or after a reset."""
    return np.zeros((0, 3), dtype=np.int64), 0


def isqrt(d: int) -> int:
    """floor(sqrt(d)) for 0 <= d < 2^62 the way the kernel takes it: a double's square root, corrected in integers."""
    d = int(d)
    assert 0 <= d < 1 << 62
    r = int(math.sqrt(float(d)))
    while r * r > d:
        r -= 1
    while (r + 1) * (r + 1) <= d:
        r += 1
    return r


def raw_sums(x) -> np.ndarray:
    """x, interleaved int16 (I, Q) of a whole number of windows -> int64 [windows, 5]: S_I, S_Q, M_II, M_QQ, M_IQ."""
    x = np.asarray(x, dtype=np.int16).reshape(-1, 2).astype(np.int64)
    assert len(x) % L == 0
    i, q = x[:, 0].reshape(-1, L), x[:, 1].reshape(-1, L)
    return np.stack([i.sum(axis=1), q.sum(axis=1), (i * i).sum(axis=1), (q * q).sum(axis=1), (i * q).sum(axis=1)], axis=1)


def moments_of_sums(sums5, d) -> np.ndarray:
    """The five raw sums and d [windows, 2] -> int64 [windows, 3]: A, B, C of u = x - d."""
    s = np.asarray(sums5, dtype=np.int64).reshape(-1, 5)
    d = np.asarray(d, dtype=np.int64).reshape(-1, 2)
    assert len(s) == len(d)
    di, dq = d[:, 0], d[:, 1]
    a = s[:, 2] - 2 * di * s[:, 0] + L * di * di
    b = s[:, 3] - 2 * dq * s[:, 1] + L * dq * dq
    c = s[:, 4] - di * s[:, 1] - dq * s[:, 0] + L * di * dq
    return np.stack([a, b, c], axis=1)


def moments(x, d) -> np.ndarray:
    """x (interleaved int16) and its windows' d [windows, 2] -> int64 [windows, 3]: A, B, C, through the five raw sums."""
    return moments_of_sums(raw_sums(x), d)


def tg_of(sa: int, sb: int, sc: int) -> tuple:
    """(t, g) of one window's sums, in Python integers."""
    sa, sb, sc = int(sa), int(sb), int(sc)
    s = max(0, max(sa, sb).bit_length() - 31)
    a, b, c = sa >> s, sb >> s, sc >> s
    dd = a * b - c * c
    if a == 0 or dd <= 0:
        return 0, G_ONE
    r = isqrt(dd)
    t = (c * 32768 + a) // (2 * a)
    g = (a * 32768 + r) // (2 * r)
    if abs(t) > T_MAX or g < G_MIN or g > G_MAX:
        return 0, G_ONE
    return t, g


def estimate(abc, k, state=None):
    """This submit's moments behind the carried state -> (tg int16 [windows, 2], the state behind them)."""
    k = _check_k(k)
    ring, count = fresh_state() if state is None else state
    m3 = np.asarray(abc, dtype=np.int64).reshape(-1, 3)
    m = len(ring)
    assert m == min(count, k)
    allm = np.concatenate([ring, m3])
    cs = np.concatenate([np.zeros((1, 3), dtype=np.int64), np.cumsum(allm, axis=0)])
    j = m + np.arange(len(m3))
    c = np.minimum(count + np.arange(len(m3)) + 1, k)
    s = cs[j + 1] - cs[j + 1 - c]
    tg = np.array([tg_of(*row) for row in s.tolist()], dtype=np.int16).reshape(-1, 2)
    return tg, (allm[max(0, len(allm) - k):].copy(), count + len(m3))


def apply(xp, tg) -> np.ndarray:
    """x' (interleaved int16, within the rails) and its windows' (t, g) [windows, 2] -> x'', interleaved int16."""
    x = np.asarray(xp, dtype=np.int16).reshape(-1, L, 2).astype(np.int32)
    tg = np.asarray(tg, dtype=np.int16).reshape(-1, 1, 2).astype(np.int32)
    assert len(x) == len(tg)
    v = (x[:, :, 1] * 16384 - tg[:, :, 0] * x[:, :, 0] + 8192) >> 14
    out = x.copy()
    out[:, :, 1] = np.clip((v * tg[:, :, 1] + 8192) >> 14, X_MIN, X_MAX)
    return out.astype(np.int16).reshape(-1)


def iq_balance(raw, fmt, k_dc, k_iq, state=None):
    """One submit's row of bytes in the format -> (x'' interleaved int16, d int16 [windows, 2], tg int16 [windows, 2], the row's
    state behind it: (the DC blocker's, the balancer's)).  k_dc = 0: no DC blocker, d = 0."""
    dc_state, iq_state = (None, None) if state is None else state
    x = formats.to_x(fmt, raw)
    s5 = raw_sums(x)
    if int(k_dc):
        d, dc_state = dcblock.estimate(s5[:, :2], k_dc, dc_state)
        xp = dcblock.apply(x, d)
    else:
        d, xp = np.zeros((len(s5), 2), dtype=np.int16), np.asarray(x, dtype=np.int16).reshape(-1)
    tg, iq_state = estimate(moments_of_sums(s5, d), k_iq, iq_state)
    return apply(xp, tg), d, tg, (dc_state, iq_state)


def iq_balance_bruteforce(raw, fmt, k_dc, k_iq, state=None):
    """iq_balance sample by sample in Python integers: every sum is recomputed from the samples of the windows it covers (the
    state carries those samples, not their sums), the divisions are written out as floors of magnitudes, the square root is
    math.isqrt.  -> (x'', d, tg, state) with a state only this function reads."""
    k_iq = _check_k(k_iq)
    k_dc = int(k_dc)
    hist, count = ([], 0) if state is None else state  # hist: the last max(K_dc, K_iq) windows as (samples, d)
    hist = list(hist)
    x = [int(v) for v in formats.to_x(fmt, raw)]
    assert len(x) % (2 * L) == 0

    def floor_div(num, den):
        quo = abs(num) // den
        return quo if num >= 0 else -quo - (1 if abs(num) % den else 0)

    out, ds, tgs = [], [], []
    for w0 in range(0, len(x), 2 * L):
        win = [(x[w0 + 2 * i], x[w0 + 2 * i + 1]) for i in range(L)]
        count += 1
        d = [0, 0]
        if k_dc:
            c = min(count, k_dc)
            past = [h[0] for h in hist[len(hist) - (c - 1):]] if c > 1 else []
            for rail in range(2):
                tot = sum(smp[rail] for wn in past + [win] for smp in wn)
                d[rail] = floor_div(2 * tot + L * c, 2 * L * c)
        hist.append((win, (d[0], d[1])))
        c = min(count, k_iq)
        sa = sb = sc = 0
        for wn, dd in hist[-c:]:
            for i_, q_ in wn:
                ui, uq = i_ - dd[0], q_ - dd[1]
                sa += ui * ui
                sb += uq * uq
                sc += ui * uq
        s = max(0, max(sa, sb).bit_length() - 31)
        a, b, cc = sa >> s, sb >> s, floor_div(sc, 1 << s)
        det = a * b - cc * cc
        t, g = 0, G_ONE
        if a != 0 and det > 0:
            r = math.isqrt(det)
            t, g = floor_div(cc * 32768 + a, 2 * a), floor_div(a * 32768 + r, 2 * r)
            if abs(t) > T_MAX or g < G_MIN or g > G_MAX:
                t, g = 0, G_ONE
        ds.append(d)
        tgs.append((t, g))
        for i_, q_ in win:
            ip = min(X_MAX, max(X_MIN, i_ - d[0]))
            qp = min(X_MAX, max(X_MIN, q_ - d[1]))
            v = floor_div(qp * 16384 - t * ip + 8192, 16384)
            out.append(ip)
            out.append(min(X_MAX, max(X_MIN, floor_div(v * g + 8192, 16384))))
        hist = hist[-max(k_dc, k_iq, 1):]
    return (np.array(out, dtype=np.int16), np.array(ds, dtype=np.int16).reshape(-1, 2), np.array(tgs, dtype=np.int16).reshape(-1, 2),
            (hist, count))
