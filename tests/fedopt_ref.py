"""Plain numpy reference for the server-optimizer step (csrc/fedopt.hip); no GPU.

server_opt_step is the definition of fh_server_opt_step (include/fedhip.h) on fp32 arrays, one
rounded operation per line: numpy's float32 +, -, *, / and sqrt are the IEEE correctly rounded
ones and keep denormals.  A NaN result is stored as the one quiet NaN 0x7FC00000.

tests/test_fedopt_ref_cpu.py pins it against hand-worked cases.
"""
import numpy as np

from robust_ref import QNAN_BITS, same_bits  # noqa: F401  (same_bits: re-exported)

MOMENTUM, ADAGRAD, ADAM, YOGI = range(4)
F = np.float32


def weighted_sum(rows, weights):
    """(((0 + w0*x0) + w1*x1) + ...): fh_fedavg_weighted_sum with accumulate = 0."""
    rows = np.asarray(rows, dtype=F)
    acc = np.zeros(rows.shape[1], dtype=F)
    for x, w in zip(rows, np.asarray(weights, dtype=F)):
        p = w * x
        acc = acc + p
    return acc


def canon(x):
    x = np.array(x, dtype=F)
    x.view(np.uint32)[np.isnan(x)] = QNAN_BITS
    return x


def server_opt_step(rule, rows, weights, g, m, v, server_lr, beta1, beta2, tau):
    """(g', m', v') fp32 [P].  rows [C, P] with weights [C], or weights None and rows [1, P]
    (or [P]): the row is the aggregate.  v may be None for MOMENTUM (returned as None)."""
    lr, b1, b2, tau = F(server_lr), F(beta1), F(beta2), F(tau)
    g, m = np.asarray(g, dtype=F), np.asarray(m, dtype=F)
    with np.errstate(all="ignore"):
        if weights is None:
            a = np.asarray(rows, dtype=F).reshape(-1, g.shape[0])
            assert a.shape[0] == 1
            a = a[0]
        else:
            a = weighted_sum(rows, weights)
        d = a - g
        omb1 = F(1.0) - b1
        omb2 = F(1.0) - b2
        bm = b1 * m
        if rule == MOMENTUM:
            mn = bm + d
            st = lr * mn
            gn = g + st
            return canon(gn), canon(mn), None
        v = np.asarray(v, dtype=F)
        od = omb1 * d
        mn = bm + od
        d2 = d * d
        if rule == ADAGRAD:
            vn = v + d2
        elif rule == ADAM:
            bv = b2 * v
            o2 = omb2 * d2
            vn = bv + o2
        else:
            t = v - d2
            s = np.where(t > 0, F(1.0), np.where(t < 0, F(-1.0), F(0.0))).astype(F)  # NaN: 0
            o2 = omb2 * d2
            os_ = o2 * s
            vn = v - os_
        rt = np.sqrt(vn)
        dn = rt + tau
        q = mn / dn
        st = lr * q
        gn = g + st
        for x in (a, d, mn, vn, rt, dn, q, st, gn):
            assert x.dtype == F
        return canon(gn), canon(mn), canon(vn)
