"""numpy restatements of the update phase's arithmetic as include/rsx.h writes it out (rsx_ppo_permutation, rsx_ppo_normalize,
rsx_adam_step), shared by tests/test_ppo_update_ref.py (no GPU) and tests/test_gpu_ppo_update.py."""
import math

import numpy as np

M32 = np.uint64(0xFFFFFFFF)
PERM_ROUNDS, DOM_PERM = 8, 8


def _u64(x):
    return np.asarray(x, dtype=np.uint64)


def philox_word0(c0, c1, c2, c3, k0, k1):
    """word 0 of philox4x32-7(counter = (c0, c1, c2, c3), key = (k0, k1)); every argument a uint64 array of 32-bit values (broadcast)"""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*(_u64(a) for a in (c0, c1, c2, c3, k0, k1)))
    for _ in range(7):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2   # (32 x 32 bits: no overflow in 64)
        h0, l0, h1, l1 = p0 >> np.uint64(32), p0 & M32, p1 >> np.uint64(32), p1 & M32
        c0, c1, c2, c3 = h1 ^ c1 ^ k0, l1, h0 ^ c3 ^ k1, l0
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c0


def perm_bits(n):
    bits = 8
    while (1 << bits) < n:
        bits += 1
    return bits


def feistel(x, bits, seed, update, epoch):
    """E(x) of rsx_ppo_permutation on the domain [0, 2^bits); x, seed, update, epoch broadcast against each other"""
    x, seed, update, epoch = np.broadcast_arrays(*(_u64(a) for a in (x, seed, update, epoch)))
    k0, k1, upd, ep = seed & M32, seed >> np.uint64(32), update & M32, epoch & M32
    wa = bits // 2
    wb = bits - wa
    a, b = x & np.uint64((1 << wa) - 1), x >> np.uint64(wa)
    for r in range(PERM_ROUNDS):
        f = philox_word0(b, ep, upd, np.uint64(DOM_PERM | (r << 8)), k0, k1)
        a, b = b, (a ^ f) & np.uint64((1 << wa) - 1)
        wa, wb = wb, wa
    return a | (b << np.uint64(wa))


def permute(idx, n, seed, update, epoch):
    """rows[idx] of rsx_ppo_permutation(n, seed, update, epoch): E applied until the value lies in [0, n) (cycle walking), at most
    2^bits - n + 1 times; idx and the three key parts broadcast against each other.  Returns int64."""
    bits = perm_bits(n)
    idx, seed, update, epoch = (np.array(a) for a in np.broadcast_arrays(*(_u64(a) for a in (idx, seed, update, epoch))))
    x = idx.copy()
    todo = np.ones(x.shape, dtype=bool)
    for _ in range((1 << bits) - n + 1):
        x[todo] = feistel(x[todo], bits, seed[todo], update[todo], epoch[todo])
        todo = x >= np.uint64(n)
        if not todo.any():
            break
    assert not todo.any(), "the walk did not end within its bound"
    return x.astype(np.int64)


def permutation(n, seed, update, epoch):
    """the whole rows [n] of rsx_ppo_permutation"""
    return permute(np.arange(n), n, seed, update, epoch)


def chunks(n, minibatches):
    """(lo, hi) of minibatch k of M: c = ceil(n / M) rows each, the last what is left"""
    c = -(-n // minibatches)
    return [(k * c, min((k + 1) * c, n)) for k in range(minibatches)]


def fixed_sum(x64, cap):
    """the reduction order of include/rsx.h on a float64 array: G = min(ceil(n / 256), cap) workgroups of 256 threads; thread j of
    workgroup w adds elements 256 w + j, + 256 G, ... from 0.0; the 64 lanes of a wave ascending from 0.0; the waves
    ((w0 + w1) + w2) + w3; the workgroups in order from 0.0.  (A thread without elements holds 0.0: padding with zeros restates it.)"""
    x64 = np.asarray(x64, dtype=np.float64).reshape(-1)
    n = x64.size
    G = min(-(-n // 256), cap)
    trips = -(-n // (256 * G))
    pad = np.zeros(trips * G * 256, dtype=np.float64)
    pad[:n] = x64
    pad = pad.reshape(trips, G, 4, 64)
    thread = np.zeros((G, 4, 64), dtype=np.float64)
    for k in range(trips):
        thread = thread + pad[k]
    wave = np.zeros((G, 4), dtype=np.float64)
    for lane in range(64):
        wave = wave + thread[:, :, lane]
    part = ((wave[:, 0] + wave[:, 1]) + wave[:, 2]) + wave[:, 3]
    total = np.float64(0.0)
    for g in range(G):
        total = total + part[g]
    return total


def normalize(adv, eps=1e-8):
    """rsx_ppo_normalize on a float32 array: (out, mean, std), all float32"""
    a = np.asarray(adv, dtype=np.float32).reshape(-1)
    x = a.astype(np.float64)
    n = np.float64(a.size)
    S, Q = fixed_sum(x, 128), fixed_sum(x * x, 128)
    mean64 = S / n
    var64 = (Q - S * mean64) / (n - np.float64(1.0))
    if var64 < 0.0:
        var64 = np.float64(0.0)
    mean, std = np.float32(mean64), np.float32(np.sqrt(var64))
    out = (a - mean) / (std + np.float32(eps))
    assert out.dtype == np.float32
    return out.reshape(np.shape(adv)), mean, std


def powi(b, t):
    """beta^t by squaring, in float64, the multiplications in rsx_adam_step's order"""
    r, b = np.float64(1.0), np.float64(b)
    while t > 0:
        if t & 1:
            r = r * b
        b = b * b
        t >>= 1
    return r


def clip_adam(p, g, m, v, t, lr, betas=(0.9, 0.999), eps=1e-8, max_norm=0.5):
    """one applied rsx_adam_step: p, g, m, v lists of three float32 arrays (actor | log_std | critic), t the step count this step
    carries (>= 1), lr a float32 value.  Returns (p, m, v) as new lists and the norm before the clip (float32)."""
    f32 = np.float32
    gcat = np.concatenate([np.asarray(x, dtype=f32).reshape(-1) for x in g]).astype(np.float64)
    norm = f32(np.sqrt(fixed_sum(gcat * gcat, 64)))
    coef = f32(1.0)
    if max_norm is not None and max_norm > 0.0:
        c = f32(max_norm) / (norm + f32(1e-6))
        coef = c if c < f32(1.0) else f32(1.0)
    b1, b2 = f32(betas[0]), f32(betas[1])
    omb1, omb2 = f32(np.float64(1.0) - np.float64(betas[0])), f32(np.float64(1.0) - np.float64(betas[1]))
    bc1, bc2 = np.float64(1.0) - powi(betas[0], t), np.float64(1.0) - powi(betas[1], t)
    step, s2 = f32(np.float64(f32(lr)) / bc1), f32(np.sqrt(bc2))
    P, Mo, V = [], [], []
    for pi, gi, mi, vi in zip(p, g, m, v):
        pi, gi, mi, vi = (np.asarray(x, dtype=f32) for x in (pi, gi, mi, vi))
        gc = gi * coef
        mn = b1 * mi + omb1 * gc
        vn = b2 * vi + (omb2 * gc) * gc
        pn = pi - step * (mn / (np.sqrt(vn) / s2 + f32(eps)))
        assert pn.dtype == f32 and mn.dtype == f32 and vn.dtype == f32
        P.append(pn); Mo.append(mn); V.append(vn)
    return P, Mo, V, norm


def chi2_quantile(p, df):
    """the p-quantile of the chi-square distribution with df degrees of freedom: bisection on the regularised lower incomplete gamma
    function (series for x < a + 1, continued fraction otherwise)"""
    a = 0.5 * df

    def cdf(x):
        x = 0.5 * x
        if x <= 0.0:
            return 0.0
        lg = math.lgamma(a)
        if x < a + 1.0:
            term = s = 1.0 / a
            k = a
            for _ in range(10000):
                k += 1.0
                term *= x / k
                s += term
                if abs(term) < abs(s) * 1e-17:
                    break
            return s * math.exp(-x + a * math.log(x) - lg)
        tiny = 1e-300
        b = x + 1.0 - a
        c, d = 1.0 / tiny, 1.0 / b
        h = d
        for i in range(1, 10000):
            an = -i * (i - a)
            b += 2.0
            d = an * d + b
            d = tiny if abs(d) < tiny else d
            c = b + an / c
            c = tiny if abs(c) < tiny else c
            d = 1.0 / d
            delta = d * c
            h *= delta
            if abs(delta - 1.0) < 1e-16:
                break
        return 1.0 - math.exp(-x + a * math.log(x) - lg) * h

    lo, hi = 0.0, float(df) + 100.0 * math.sqrt(2.0 * df) + 100.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if cdf(mid) < p:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)
