"""The arithmetic contract of the verification CNN in NumPy: what wb_verify_launch and
waldboost_amd.verification.Verifier.predict must return, bit for bit.

* fold: batch normalisation folded into the convolutions in float64, rounded to float32 once;
* every pre-activation is one float32 chain acc = b', acc = fmaf(x_k, w_k, acc), k ascending -- convolutions in (ky, kx,
  input channel) order, taps outside the window multiplied by zero, dense layers in flat-index order;
* ReLU is acc > 0 ? acc : +0; the pool is a 2x2 maximum with the last row / column of an odd size dropped; the flatten
  is (row, column, channel); the score is added last, one float32 add.

fmaf is the correctly rounded fused multiply-add: the product of two float32 is exact in float64; the float64 sum is
made round-to-odd with the exact error of TwoSum; one rounding to float32 follows (53 >= 24 + 2 bits, so the double
rounding is innocuous).  Only sums whose low 28 bits are zero can round differently from the plain float64 shortcut, so
only those take the long way."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

_LOW28 = np.int64(0x0FFFFFFF)


class _Chains:
    """One float32 fmaf chain per element of a float64 work buffer, stepped in place.  A product that is zero leaves its
    sum exact (and the sum's low bits zero): such elements are counted and not looked at again -- after a ReLU they are
    half of all."""

    def __init__(self, shape, start):
        self.acc = np.empty(shape)
        self.acc[...] = start
        self.p, self.s = np.empty(shape), np.empty(shape)
        self.low, self.r = np.empty(shape, np.int64), np.empty(shape, np.float32)
        np.copyto(self.r, self.acc, casting="same_kind")

    def step(self, x, w):
        """acc = fmaf(x, w, acc); x and w (float64 arrays holding float32 values) broadcast to the buffer."""
        acc, p, s, low, r = self.acc, self.p, self.s, self.low, self.r
        with np.errstate(all="ignore"):
            np.multiply(x, w, out=p)                   # exact: 24 + 24 bits
            np.add(p, acc, out=s)
            np.bitwise_and(s.view(np.int64), _LOW28, out=low)
            if np.count_nonzero(low) + (p.size - np.count_nonzero(p)) != p.size:
                at = np.nonzero((low == 0) & (p != 0.0))
                ps, cs, ss = p[at], acc[at], s[at]
                t = ss - ps                            # TwoSum: ss + err == ps + cs exactly
                err = (ps - (ss - t)) + (cs - t)
                inexact = np.isfinite(err) & (err != 0.0)
                # round to odd: these sums are even; the exact value lies between ss and its neighbour on err's side
                step = np.where((err > 0.0) == (ss > 0.0), 1, -1).astype(np.int64)
                s[at] = (ss.view(np.int64) + np.where(inexact, step, 0)).view(np.float64)
            np.copyto(r, s, casting="same_kind")
            np.copyto(acc, r)


def fmaf(a, b, c):
    """Correctly rounded float32 fma(a, b, c), elementwise with broadcasting."""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    shape = np.broadcast(a, b, c).shape
    chains = _Chains(shape or (1,), c)
    chains.step(a, b)
    return chains.r.reshape(shape)


def fmaf_shortcut(a, b, c):
    """What fmaf must NOT be: the float64 sum rounded twice."""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    return (a * b + c).astype(np.float32)


def fold(arrays, epsilon):
    """The 28 Keras arrays -> [(W', b')] * 4 + [dense0 kernel (F, 128), bias, dense1 kernel (128,), bias (1,)], float32."""
    layers = []
    for k in range(4):
        W, b, gamma, beta, mean, var = (np.asarray(a, np.float64) for a in arrays[6 * k:6 * k + 6])
        s = gamma / np.sqrt(var + np.float64(epsilon))
        layers.append(((W * s).astype(np.float32), ((b - mean) * s + beta).astype(np.float32)))
    return layers + [np.asarray(arrays[24], np.float32), np.asarray(arrays[25], np.float32),
                     np.asarray(arrays[26], np.float32).reshape(-1), np.asarray(arrays[27], np.float32).reshape(-1)]


def relu(x):
    return np.where(x > 0, x, np.float32(0.0)).astype(np.float32)


def _conv_chunk(x, W, b, pad_mode):
    """conv3x3 for a few windows, on [window][output channel][pixel] buffers (long contiguous inner loops)."""
    N, H, Wd, cin = x.shape
    cout = W.shape[3]
    xp = np.pad(x.astype(np.float64), ((0, 0), (1, 1), (1, 1), (0, 0)), mode=pad_mode)
    W64 = W.astype(np.float64)
    chains = _Chains((N, cout, H * Wd), b.astype(np.float64)[None, :, None])
    for ky in range(3):
        for kx in range(3):
            taps = np.ascontiguousarray(xp[:, ky:ky + H, kx:kx + Wd, :].transpose(3, 0, 1, 2)).reshape(cin, N, 1, H * Wd)
            for i in range(cin):
                chains.step(taps[i], W64[ky, kx, i][None, :, None])
    return np.ascontiguousarray(chains.r.reshape(N, cout, H, Wd).transpose(0, 2, 3, 1))


def conv3x3(x, W, b, pad_mode="constant"):
    """Pre-activations of a 3x3 "same" cross-correlation: out[y, x, o] = b[o] + sum in[y + ky - 1, x + kx - 1, i] *
    w[ky, kx, i, o], one chain per output in (ky, kx, i) order.  x (N, H, W, cin) float32."""
    x = np.asarray(x, np.float32)
    chunk = max(1, 65536 // (x.shape[1] * x.shape[2] * W.shape[3]))      # buffers of half a megabyte
    parts = [x[a:a + chunk] for a in range(0, x.shape[0], chunk)]
    if len(parts) <= 1:
        return _conv_chunk(x, W, b, pad_mode)
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:       # (NumPy releases the lock)
        return np.concatenate(list(pool.map(lambda part: _conv_chunk(part, W, b, pad_mode), parts)))


def pool2x2(x):
    N, H, Wd, C = x.shape
    h2, w2 = H // 2, Wd // 2
    return x[:, :2 * h2, :2 * w2].reshape(N, h2, 2, w2, 2, C).max(axis=(2, 4))


def dense(x, W, b):
    """Pre-activations b[j] + sum_k x[k] * W[k, j], k ascending.  x (N, K) float32, W (K, J)."""
    x64, W64 = np.asarray(x, np.float32).astype(np.float64), np.asarray(W, np.float32).astype(np.float64)
    chains = _Chains((x64.shape[0], W64.shape[1]), np.asarray(b, np.float32).astype(np.float64))
    for k in range(x64.shape[1]):
        chains.step(x64[:, k, None], W64[None, k])
    return chains.r


def forward(layers, X, scores):
    """cnn(X) + scores as float32 (N,).  layers: fold(...)'s list; X (N, m, n, C) float32 or uint8 (widened exactly)."""
    (w1, b1), (w2, b2), (w3, b3), (w4, b4), d0, c0, d1, c1 = layers
    a = np.asarray(X).astype(np.float32)
    a = relu(conv3x3(a, w1, b1))
    a = relu(conv3x3(a, w2, b2))
    a = pool2x2(a)
    a = relu(conv3x3(a, w3, b3))
    a = relu(conv3x3(a, w4, b4))
    h = relu(dense(a.reshape(a.shape[0], -1), d0, c0))
    y = dense(h, d1.reshape(-1, 1), c1)[:, 0]
    return (y + np.asarray(scores, np.float32).reshape(-1)).astype(np.float32)


def predict(arrays, epsilon, X, scores):
    return forward(fold(arrays, epsilon), X, scores)
