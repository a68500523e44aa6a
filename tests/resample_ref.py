"""Float64 numpy restatement of a2m.pats_audio.resample: band-limited interpolation with a
Kaiser-windowed sinc, from the published formulas only (resampy's filter parameters; neither
resampy nor librosa is a dependency, so parity with them is unpinned).

  g = gcd(sr_in, sr_out), P = sr_in / g, Q = sr_out / g, s = min(1, sr_out / sr_in), L = ceil(Z / s)
  output t sits at input position t P / Q:  n_t = (t P) div Q,  p_t = (t P) mod Q  (integers)
  y[t]   = sum_{k = -L+1 .. L} h_{p_t}[k] x[n_t + k]          x = 0 outside [0, n)
  h_p[k] = s rho sinc(s rho tau) w(s tau / Z),  tau = (p - k Q) / Q
  w(u)   = I0(beta sqrt(1 - u^2)) / I0(beta) for |u| < 1, else 0;  sinc(v) = sin(pi v) / (pi v)
  len(y) = ceil(n sr_out / sr_in)

|u| < 1 is decided in integers, |p - k Q| < Z max(P, Q) (the same inequality without a rounding),
so a tap exactly on the window's edge is zero whatever the last bit of s tau / Z is.

Shared by the CPU and GPU tests; the tests treat its outputs as read-only.
"""
import math

import numpy as np

# res_type -> (zero crossings Z, Kaiser beta, roll-off rho)
FILTERS = {'kaiser_best': (64, 14.769656459379492, 0.9475937167399596),
           'kaiser_fast': (16, 8.555504641634386, 0.85)}


def ratio(sr_in, sr_out):
    g = math.gcd(sr_in, sr_out)
    return sr_in // g, sr_out // g


def half_width(sr_in, sr_out, num_zeros):
    P, Q = ratio(sr_in, sr_out)
    return -(-num_zeros * max(P, Q) // Q)          # ceil(Z / s)


def num_samples(n, sr_in, sr_out):
    return -(-n * sr_out // sr_in)


def bank(sr_in, sr_out, res_type='kaiser_best'):
    """[Q, 2L] float64: row p holds h_p[k] for k = -L+1 .. L."""
    Z, beta, rho = FILTERS[res_type]
    P, Q = ratio(sr_in, sr_out)
    L = half_width(sr_in, sr_out, Z)
    s = min(1.0, sr_out / sr_in)
    num = np.arange(Q, dtype=np.int64)[:, None] - np.arange(-L + 1, L + 1, dtype=np.int64)[None, :] * Q
    tau = num / float(Q)
    u = s * tau / Z
    inside = np.abs(num) < Z * max(P, Q)
    w = np.where(inside, np.i0(beta * np.sqrt(np.maximum(0.0, 1.0 - u * u))) / np.i0(beta), 0.0)
    return s * rho * np.sinc(s * rho * tau) * w


def resample(x, sr_in, sr_out, res_type='kaiser_best', dtype=np.float64):
    """x [n] -> y [ceil(n sr_out / sr_in)], sums in `dtype` (float32: the GPU's arithmetic)."""
    x = np.asarray(x, dtype=dtype)
    P, Q = ratio(sr_in, sr_out)
    L = half_width(sr_in, sr_out, FILTERS[res_type][0])
    n_out = num_samples(x.size, sr_in, sr_out)
    if n_out == 0:
        return np.zeros(0, dtype)
    h = bank(sr_in, sr_out, res_type).astype(dtype)
    t = np.arange(n_out, dtype=np.int64)
    n_t, p_t = t * P // Q, t * P % Q
    idx = n_t[:, None] + np.arange(-L + 1, L + 1, dtype=np.int64)[None, :]
    xg = np.where((idx >= 0) & (idx < x.size), x[np.clip(idx, 0, x.size - 1)], dtype(0))
    return (h[p_t] * xg).sum(axis=1, dtype=dtype)


def tone(n_samples, sr, hz):
    return np.sin(2 * np.pi * hz * np.arange(n_samples) / float(sr))
