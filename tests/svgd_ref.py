"""fp64 numpy restatement of F23 (include/bnn_hip.h): the squared distances of the members, the median bandwidth, the RBF kernel
matrix and the two M x M matrices A, B of the direction d = A g + B theta that the optimiser subtracts -- SVGD (Liu & Wang 2016)
and kde-WGD (D'Angelo & Fortuin 2021).  tests/test_svgd_cpu.py ties it to the definition (phi with the kernel's gradient from
autograd); tests/test_gpu_svgd.py holds the kernels against it."""
import math

import numpy as np

MAX_MEMBERS = 64
CHUNK = 4096
CHAIN = 129
METHODS = ("svgd", "wgd")


def energy_scales(dataset_size, batch_size, prior_precision=1.0, temperature=1.0):
    """(s, tau'): grad U_j = s g_j + tau' theta_j."""
    return float(dataset_size) / (float(batch_size) * float(temperature)), float(prior_precision) / float(temperature)


def dist2(theta):
    """D2_ij = sum_p (theta_i[p] - theta_j[p])^2 from differences; exactly symmetric, the diagonal exactly 0."""
    theta = np.asarray(theta, dtype=np.float64)
    M = theta.shape[0]
    D2 = np.zeros((M, M))
    for i in range(M - 1):
        d = theta[i] - theta[i + 1:]
        D2[i, i + 1:] = D2[i + 1:, i] = (d * d).sum(axis=1)
    return D2


def bandwidth(D2, h=None):
    """(median of all M^2 entries, h): h = the given bandwidth or median / log(M + 1); h == 0 -> 1."""
    M = D2.shape[0]
    med = float(np.median(D2))
    hh = float(h) if h else med / math.log(M + 1)
    return med, (1.0 if hh == 0.0 else hh)


def kernel(D2, h):
    K = np.exp(-D2 / h)
    return K, K.sum(axis=1)


def coefficients(D2, s, tau, method="svgd", h=None):
    """(A, B, med, h, r) in fp64 from a matrix of squared distances."""
    assert method in METHODS
    M = D2.shape[0]
    med, hh = bandwidth(D2, h)
    K, r = kernel(D2, hh)
    I = np.eye(M)
    if method == "svgd":
        A = s * K / M
        B = (tau * K + (2.0 / hh) * (K - I * r[:, None])) / M
    else:
        A = s * I
        B = tau * I - (2.0 / hh) * (I - K / r[:, None])
    return A, B, med, hh, r


def terms(D2, s, tau, method="svgd", h=None):
    """The largest magnitude that enters each entry of A and of B (the scale of their rounding error)."""
    M = D2.shape[0]
    med, hh = bandwidth(D2, h)
    K, r = kernel(D2, hh)
    I = np.eye(M)
    if method == "svgd":
        return s * K / M, np.maximum(np.maximum(tau * K, (2.0 / hh) * K), (2.0 / hh) * I * r[:, None]) / M
    return s * I, np.maximum(np.maximum(tau * I, (2.0 / hh) * I), (2.0 / hh) * K / r[:, None])


def direction(theta, g, s, tau, method="svgd", h=None):
    """d = A g + B theta, [M, P] fp64."""
    theta, g = np.asarray(theta, dtype=np.float64), np.asarray(g, dtype=np.float64)
    A, B = coefficients(dist2(theta), s, tau, method, h)[:2]
    return A @ g + B @ theta


def chunks(stride):
    """bnn_svgd_chunks: ceil(stride / C), C = 64 min(CHUNK / 64, ceil(stride / 32768)) columns per chunk."""
    c = 64 * min(CHUNK // 64, -(-stride // 32768))
    return -(-stride // c)


def pair_index(i, j, M):
    """Where bnn_svgd_dist files pair (i, j), i < j."""
    return i * (2 * M - i - 1) // 2 + (j - i - 1)
