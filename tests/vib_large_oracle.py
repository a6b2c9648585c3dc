"""numpy restatement of k_vib_eigh_large (xequinet_amd/csrc/xeq_vib.hip): no test functions.

The same four phases in the kernel's operation order, vectorised over what the kernel spreads over its threads: Householder reduction
of the full symmetric matrix from the last row up, Q accumulated from the top-left corner and transposed, implicit-shift QL with the
running shift on (d, e) with every rotation applied to two rows of Q^T, then ranks, signs and the row permutation.  Sums over a vector
follow the kernel's pattern (thread t over the entries t, t + 256, ..., then the fixed tree over 256 partial sums); a column sum runs
top to bottom.  The kernel is built with contraction on, so its a * b + c may be one fused operation where this file rounds twice:
the two agree to rounding, not to the bit, and the tests bound both against numpy.linalg with the project's backward-error unit.
"""
import math

import numpy as np

THREADS = 256
MAX_ITER = 30       # XEQ_VIB_MAX_SWEEPS
EPS = 2.0 ** -52


def block_sum(x):
    """Thread t adds the entries t, t + 256, ... in order; then red[t] += red[t + o] for o = 128, 64, ..., 1."""
    red = np.zeros(THREADS)
    for start in range(0, len(x), THREADS):
        part = x[start : start + THREADS]
        red[: len(part)] += part
    o = THREADS // 2
    while o > 0:
        red[:o] += red[o : 2 * o]
        o //= 2
    return float(red[0])


def tridiagonalise(A):
    """(d, e, Qt): Qt A Qt^T = tridiag(d, e) with e[k] between k and k + 1 (e[m - 1] = 0); row i of Qt is column i of Q."""
    Z = np.array(A, dtype=np.float64)
    m = Z.shape[0]
    d, e = np.zeros(m), np.zeros(m)
    for i in range(m - 1, 0, -1):
        u = Z[i, :i].copy()
        sigma = block_sum(u[: i - 1] ** 2)
        f = u[i - 1]
        d[i] = Z[i, i]
        if not sigma > 0.0:
            e[i - 1] = f + sigma              # sigma is 0, or a NaN that must not be lost
            Z[i, i] = 0.0
            continue
        nrm2 = sigma + f * f
        g = -math.copysign(math.sqrt(nrm2), f)
        hh = nrm2 - f * g
        e[i - 1] = g
        u[i - 1] = f - g
        Z[i, :i] = u
        Z[i, i] = hh
        p = np.zeros(i)
        for k in range(i):
            p += Z[k, :i] * u[k]
        p /= hh
        kk = block_sum(u * p) / (2.0 * hh)
        q = p - kk * u
        L = np.outer(u, q)                    # entry (j, k) of the update: u_lo q_hi + q_lo u_hi with lo = min(j, k), hi = max(j, k)
        Z[:i, :i] -= L + L.T                  # (a sum of two rounded products commutes: symmetric to the bit)
    d[0] = Z[0, 0]
    Z[0, 0] = 1.0
    for i in range(1, m):
        hh = Z[i, i]
        if hh > 0.0:
            u = Z[i, :i].copy()
            acc = np.zeros(i)
            for k in range(i):
                acc += u[k] * Z[k, :i]
            acc /= hh
            Z[:i, :i] -= np.outer(u, acc)
        Z[i, :i] = 0.0
        Z[:i, i] = 0.0
        Z[i, i] = 1.0
    return d, e, np.ascontiguousarray(Z.T)


def ql(d, e, Zt):
    """In place; returns (iterations per eigenvalue, status)."""
    m = len(d)
    iters, status = [], 0
    fshift, tst1 = 0.0, 0.0
    for l in range(m):
        tst1 = max(tst1, abs(d[l]) + abs(e[l]))
        it = 0
        while True:
            small = np.nonzero(np.abs(e[l : m - 1]) <= EPS * tst1)[0]
            mm = l + int(small[0]) if len(small) else m - 1
            if mm == l:
                break
            if it == MAX_ITER:
                status = 1
                break
            it += 1
            el, g0, el1 = e[l], d[l], e[l + 1]
            p = (d[l + 1] - g0) / (2.0 * el)
            pr = p + math.copysign(math.hypot(p, 1.0), p)
            dl, dl1 = el / pr, el * pr
            h = g0 - dl
            d[l], d[l + 1] = dl, dl1
            d[l + 2 :] -= h
            fshift += h
            p = d[mm]
            c = c2 = c3 = 1.0
            s = s2 = 0.0
            carry = Zt[mm].copy()
            for i in range(mm - 1, l - 1, -1):
                c3, c2, s2 = c2, c, s
                ce, cp = c * e[i], c * p
                r = math.hypot(p, e[i])
                e[i + 1] = s * r
                s, c = e[i] / r, p / r
                p = c * d[i] - s * ce
                d[i + 1] = cp + s * (c * ce + s * d[i])
                zi = Zt[i]
                Zt[i + 1] = s * zi + c * carry
                carry = c * zi - s * carry
            Zt[l] = carry
            p = -s * s2 * c3 * el1 * el / dl1
            e[l] = s * p
            d[l] = c * p
        iters.append(it)
        if status:
            break
        d[l] += fshift
    return iters, status


def eigh(A):
    """(eigenvalues ascending, Vt with vector k in row k and its largest-magnitude component positive, iterations per eigenvalue,
    status): the output contract of xeq_vib_eigh_large."""
    d, e, Zt = tridiagonalise(A)
    iters, status = ql(d, e, Zt)
    m = len(d)
    if status or not np.isfinite(d).all():
        return d, Zt, iters, 1
    rank = np.array([int(((d < d[k]) | ((d == d[k]) & (np.arange(m) < k))).sum()) for k in range(m)])
    lead = np.abs(Zt).argmax(axis=1)                   # the first of equal magnitudes
    sign = np.where(Zt[np.arange(m), lead] < 0.0, -1.0, 1.0)
    w, Vt = np.empty(m), np.empty((m, m))
    w[rank] = d
    Vt[rank] = sign[:, None] * Zt
    return w, Vt, iters, 0
