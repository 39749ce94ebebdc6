"""float64 numpy restatement of the device input pipeline (csrc/pipeline.hip; utils/data_utils.py of the reference): mean and population
std per (block, channel) over all rows of the block's trials with std == 0 -> 1, z-score, the 9-tap Gaussian over time with half-sample
reflection (period 2 * len: ... c b a | a b c | c b a ...), then zero-pad / truncate to Tmax.  tests/test_pipeline_ref_cpu.py holds
smooth() to scipy.ndimage.gaussian_filter1d(mode="reflect", radius=4); the GPU tests use this restatement only."""
import numpy as np

RADIUS = 4


def taps(sigma):
    d = np.arange(-RADIUS, RADIUS + 1, dtype=np.float64)
    w = np.exp(-0.5 * d * d / (sigma * sigma))
    return w / w.sum()


def reflect(t, n):
    """index of sample t of the half-sample symmetric extension of n samples"""
    t = np.mod(t, 2 * n)
    return np.where(t < n, t, 2 * n - 1 - t)


def smooth(z, sigma):
    """z [len, C] float64 -> the filtered trial, same shape"""
    n = z.shape[0]
    w = taps(sigma)
    t = np.arange(n)
    out = np.zeros_like(z)
    for k in range(2 * RADIUS + 1):
        out += w[k] * z[reflect(t + k - RADIUS, n)]
    return out


def block_stats(trials, blocks, nblocks):
    """trials: list of [len, C] arrays; blocks: their block ids in [0, nblocks) -> (mean, std) float64 [nblocks, C]; a block without
    rows: mean 0, std 1"""
    C = trials[0].shape[1]
    mean, std = np.zeros((nblocks, C)), np.ones((nblocks, C))
    for b in range(nblocks):
        rows = [np.asarray(x, dtype=np.float64) for x, i in zip(trials, blocks) if i == b and x.shape[0] > 0]
        if not rows:
            continue
        x = np.concatenate(rows, axis=0)
        mean[b] = x.mean(axis=0)
        sd = np.sqrt(((x - mean[b]) ** 2).mean(axis=0))
        std[b] = np.where(sd == 0.0, 1.0, sd)
    return mean, std


def process_and_pad(trials, blocks, tmax, sigma=1.0):
    """-> float64 [n, tmax, C]; blocks as data_utils.process_and_pad takes them (any labels)"""
    _, inv = np.unique(np.asarray(blocks), return_inverse=True)
    mean, std = block_stats(trials, inv, int(inv.max()) + 1)
    out = np.zeros((len(trials), tmax, trials[0].shape[1]))
    for i, x in enumerate(trials):
        z = smooth((np.asarray(x, dtype=np.float64) - mean[inv[i]]) / std[inv[i]], sigma)
        n = min(tmax, z.shape[0])
        out[i, :n] = z[:n]
    return out
