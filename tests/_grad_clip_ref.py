"""numpy restatement of the global gradient norm and clip coefficient (include/kgat_hip.h, "global-norm gradient
clipping"): the fp64 reference, the worst-case bound of the fp32 kernel against it, and the kernel's own order of
additions replayed in fp32 (so that its bits can be predicted on the host)."""
import numpy as np

CHUNK = 4096      # elements per workgroup
LANES = 256       # threads per workgroup
WAVE = 64
U = 2.0 ** -24    # unit roundoff of fp32
CHAIN = CHUNK // LANES + 6 + 2   # fp32 additions a square passes through in `partials`: serial in the lane, the two trees


def gamma(k):
    return k * U / (1 - k * U)


def norm_bound(chain):
    """|norm - exact| / exact: every square is rounded once and passes through at most `chain` fp32 additions of
    positive terms, (1 + d)^(chain + 1) on the sum; the square root halves it; the double additions, the double square
    root and the rounding of the root to fp32 stay inside 2u."""
    return gamma(chain + 1) / 2 + 2 * U


def norm64(grads):
    return float(np.sqrt(sum(float((np.asarray(g, np.float64) ** 2).sum()) for g in grads)))


def coef_of(norm, max_norm):
    """The clip coefficient, in fp32 from the fp32 norm, as torch forms it (np.minimum keeps a NaN, as torch.clamp)."""
    return np.minimum(np.float32(max_norm) / (np.float32(norm) + np.float32(1e-6)), np.float32(1))


def _tree(v):
    """The workgroup's fixed tree over the last axis (256 lanes): shfl_down by 32 .. 1 in each wavefront, then
    (w0 + w1) + (w2 + w3).  The dtype of `v` is kept."""
    v = v.reshape(v.shape[:-1] + (LANES // WAVE, WAVE)).copy()
    off = WAVE // 2
    while off:
        v[..., :off] = v[..., :off] + v[..., off:2 * off]
        off //= 2
    w = v[..., 0]
    return (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])


def partials(grads):
    """One fp32 sum of squares per started chunk of every non-empty tensor, in the kernel's order: lane l owns elements
    1024 k + 4 l .. + 3 (k = 0..3) of its chunk and adds their squares serially, then the tree."""
    out = []
    for g in grads:
        g = np.asarray(g, np.float32).reshape(-1)
        if g.size == 0:
            continue
        nb = -(-g.size // CHUNK)
        x = np.zeros(nb * CHUNK, np.float32)
        x[:g.size] = g
        x = x.reshape(nb, CHUNK // 1024, LANES, 4)
        acc = np.zeros((nb, LANES), np.float32)
        for k in range(CHUNK // 1024):
            for j in range(4):
                acc = acc + x[:, k, :, j] * x[:, k, :, j]
        out.append(_tree(acc))
    return np.concatenate(out) if out else np.zeros(0, np.float32)


def finish(parts, max_norm):
    """(norm, coef) from the partials: thread t adds partials t, t + 256, ... in double, then the tree in double."""
    n = len(parts)
    rows = -(-n // LANES)
    x = np.zeros(max(rows, 1) * LANES, np.float64)
    x[:n] = parts
    acc = np.zeros(LANES, np.float64)
    for r in x.reshape(-1, LANES):
        acc = acc + r
    norm = np.float32(np.sqrt(_tree(acc)))
    return norm, coef_of(norm, max_norm)


def grad_norm(grads, max_norm):
    return finish(partials(grads), max_norm)
