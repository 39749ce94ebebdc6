"""Float64 restatement of the vector quantiser (include/franken_hip.h: fk_vq_assign, fk_vq_bwd, fk_vq_codebook_update) in numpy, and the
fixed inputs the CPU and GPU tests share.  Nothing here imports the library."""
import numpy as np

# (R, K, D) of the lookup tests: one row / one code, row and code tails, more than one workgroup (32 rows) and chunk (32 codes), every
# padded width (16, 32, 64, 128), K below / at / above a multiple of 32 and of 8 chunks
LOOKUP_CASES = [(1, 1, 4), (63, 33, 16), (65, 64, 16), (96, 7, 8), (257, 1000, 64), (300, 1031, 64), (513, 1024, 64), (130, 2050, 128)]
GAP = 1e-5            # rows whose float64 top-2 similarity gap is below this are not compared (fp32 dot error bound (D + 2) 2^-24 = 8e-6)


def lookup_inputs(R, K, D):
    """Gaussian rows scaled by U(0.1, 5), unit-norm Gaussian codes; float32 values (what both dtypes of the test start from)"""
    rng = np.random.default_rng(1000 * R + K + D)
    x = rng.standard_normal((R, D)) * rng.uniform(0.1, 5.0, (R, 1))
    codes = rng.standard_normal((K, D))
    codes /= np.linalg.norm(codes, axis=1, keepdims=True)
    return x.astype(np.float32), codes.astype(np.float32)


def normalize(v, eps=1e-12):
    v = np.asarray(v, dtype=np.float64)
    return v / np.maximum(np.linalg.norm(v, axis=-1, keepdims=True), eps)


def lookup(x, codes):
    """-> idx [R] (lowest index on a tie), gap [R] (best minus second-best similarity; inf for K = 1), xn [R, D], sims [R, K]"""
    xn = normalize(x)
    sims = xn @ np.asarray(codes, dtype=np.float64).T
    idx = sims.argmax(axis=1)                         # numpy: first maximum
    if sims.shape[1] > 1:
        top2 = np.partition(sims, -2, axis=1)[:, -2:]
        gap = top2[:, 1] - top2[:, 0]
    else:
        gap = np.full(sims.shape[0], np.inf)
    return idx, gap, xn, sims


def stats(xn, idx, K):
    counts = np.bincount(idx, minlength=K).astype(np.float64)
    sums = np.zeros((K, xn.shape[1]))
    np.add.at(sums, idx, xn)
    return counts, sums


def commit_sum(x, q):
    d = np.asarray(x, dtype=np.float64) - np.asarray(q, dtype=np.float64)
    return float((d * d).sum())


def backward(x, q, dq, d_commit, commitment_weight):
    x, q, dq = (np.asarray(t, dtype=np.float64) for t in (x, q, dq))
    return dq + d_commit * 2.0 * commitment_weight / x.size * (x - q)


def ema(embed, embed_avg, cluster_size, counts, sums, decay, eps, dead, seed=None):
    """-> (embed, embed_avg, cluster_size, dead mask) after one EMA step; dead codes take normalize(seed) when seed is given"""
    K = embed.shape[0]
    cs = decay * np.asarray(cluster_size, dtype=np.float64) + (1 - decay) * counts
    avg = decay * np.asarray(embed_avg, dtype=np.float64) + (1 - decay) * sums
    n = cs.sum()
    smoothed = (cs + eps) / (n + K * eps) * n
    emb = normalize(avg / smoothed[:, None])
    is_dead = cs < dead
    if seed is not None and is_dead.any():
        s = normalize(seed)
        emb[is_dead] = s[is_dead]
        avg[is_dead] = s[is_dead] * dead
        cs[is_dead] = dead
    return emb, avg, cs, is_dead


def kmeans_round(xn, means):
    """one Lloyd round on unit-norm rows -> (new means, idx, counts, smallest top-2 gap, mean best similarity)"""
    sims = xn @ means.T
    idx = sims.argmax(axis=1)
    top2 = np.partition(sims, -2, axis=1)[:, -2:]
    counts, sums = stats(xn, idx, means.shape[0])
    new = means.copy()
    live = counts > 0
    new[live] = normalize(sums[live] / counts[live, None])
    return new, idx, counts, float((top2[:, 1] - top2[:, 0]).min()), float(sims.max(axis=1).mean())


def planted(R=400, K=8, D=16, noise=0.05, seed=7):
    """K well-separated unit directions (signed coordinate axes) plus Gaussian noise; the initial means are the noisy directions
    themselves rotated slightly, so every round of the float64 Lloyd iteration has a top-2 gap far above 1e-4"""
    rng = np.random.default_rng(seed)
    dirs = np.zeros((K, D))
    dirs[np.arange(K), np.arange(K) * (D // K)] = 1.0
    lab = np.arange(R) % K
    x = (dirs[lab] + noise * rng.standard_normal((R, D))) * rng.uniform(0.5, 2.0, (R, 1))
    init = normalize(dirs + 0.2 * rng.standard_normal((K, D)))
    return x.astype(np.float32), init.astype(np.float32), lab


def planted_with_empty_cluster(j=5):
    """planted() with initial mean j pointing away from every row (minus the mean planted direction): no row ever selects it"""
    x, init, lab = planted()
    init = init.copy()
    dirs = np.zeros_like(init, dtype=np.float64)
    dirs[np.arange(init.shape[0]), np.arange(init.shape[0]) * (init.shape[1] // init.shape[0])] = 1.0
    init[j] = normalize(-dirs.sum(axis=0)).astype(np.float32)
    return x, init, j
