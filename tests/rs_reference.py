"""A numpy restatement of include/msig_rs.h's definition, written from the definition and sharing no code with the library or with
multimodalsignal_amd/resample.py: it takes the tap table `h` that FirResampler builds (or any other of 2 * half + 1 taps) and forms

    y[m] = sum over j of h[half + m M - j L] x[j],   j = max(0, ceil((m M - half) / L)) .. floor((m M + half) / L), ascending

for the outputs whose whole support lies inside the input, in float64 or in np.longdouble.  The sum is one multiply and one add per
tap in ascending j (numpy has no fused multiply-add), all outputs side by side."""
import numpy as np


def support(m, up, down, half):
    """(first, last) raw row of output m."""
    lo = m * down - half
    return max(0, -((-lo) // up)), (m * down + half) // up


def out_count_brute(n_in, up, down, half):
    """The outputs whose last raw row has arrived, counted one by one."""
    m = 0
    while support(m, up, down, half)[1] <= n_in - 1:
        m += 1
    return m


def resample(x, h, up, down, half, dtype=np.float64):
    """(n_out, cols) of a (n_in,) or (n_in, cols) input, n_out = out_count_brute(n_in), in `dtype`."""
    x = np.asarray(x).reshape(len(x), -1).astype(dtype)
    h = np.asarray(h).astype(dtype)
    assert h.shape == (2 * half + 1,)
    n = out_count_brute(x.shape[0], up, down, half)
    acc = np.zeros((n, x.shape[1]), dtype=dtype)
    if n == 0:
        return acc
    c = np.arange(n, dtype=np.int64) * down
    j0 = np.maximum(0, -((half - c) // up))
    j1 = (c + half) // up
    assert j1.max() <= x.shape[0] - 1
    for k in range(int((j1 - j0).max()) + 1):
        j = j0 + k
        live = j <= j1
        jj = np.where(live, j, 0)
        term = h[np.where(live, half + c - jj * up, 0)][:, None] * x[jj]
        acc = np.where(live[:, None], acc + term, acc)
    return acc


def holds(j, up, down, half, n_out):
    """The outputs among the first n_out whose support holds raw row j."""
    return [m for m in range(n_out) if support(m, up, down, half)[0] <= j <= support(m, up, down, half)[1]]
