"""float64 numpy restatement of fmri_tta_agreement_f64 (include/fmri_hip.h), written from its definitions and from nothing else: explicit
loops over k for the sums, np.sort along k for the median, plain comparisons for the counts.  It does not import the package.  Also the
two data sets of tests/test_gpu_tta_agreement.py and tests/test_host_tta_agreement.py."""
import numpy as np

MAPS = ("mean", "variance", "entropy", "disagreement")
DYADIC = (0.0, 0.25, 0.5, 0.75, 1.0)


def agreement(stack, threshold=0.5, channels=1):
    """stack (K, ...) float64, channels last when channels > 1 -> dict of 'median', the four maps (each shaped like stack[0]) and
    'counts' (channels, 2K + 1) int64"""
    stack = np.asarray(stack)
    assert stack.dtype == np.float64 and stack.ndim >= 2 and stack.shape[0] >= 1
    K = stack.shape[0]
    srt = np.sort(stack, axis=0)
    median = (srt[(K - 1) // 2] + srt[K // 2]) / 2.0
    total = stack[0].copy()
    for k in range(1, K):
        total = total + stack[k]
    mean = total / float(K)
    sq = np.zeros(stack.shape[1:])
    for k in range(K):
        d = stack[k] - mean
        sq = sq + d * d
    variance = sq / float(K)
    p = np.minimum(np.maximum(mean, 0.0), 1.0)
    entropy = np.zeros(stack.shape[1:])
    inside = (p > 0.0) & (p < 1.0)
    pi = p[inside]
    entropy[inside] = -(pi * np.log2(pi) + (1.0 - pi) * np.log2(1.0 - pi))
    M = median > threshold
    differ = np.zeros(stack.shape[1:], dtype=np.int64)
    counts = np.zeros((channels, 2 * K + 1), dtype=np.int64)
    Mc = M.reshape(-1, channels)
    counts[:, 0] = Mc.sum(axis=0)
    for k in range(K):
        V = stack[k] > threshold
        differ += V != M
        Vc = V.reshape(-1, channels)
        counts[:, 1 + k] = Vc.sum(axis=0)
        counts[:, 1 + K + k] = (Vc & Mc).sum(axis=0)
    return {"median": median, "mean": mean, "variance": variance, "entropy": entropy, "disagreement": differ / float(K), "counts": counts}


def scores(counts):
    """(variant_dice (K, C), estimated_dice (C,), volume_cv (C,)) from counts (C, 2K + 1), element by element"""
    counts = np.asarray(counts)
    C, K = counts.shape[0], (counts.shape[1] - 1) // 2
    dice, est, cv = np.zeros((K, C)), np.zeros(C), np.zeros(C)
    for c in range(C):
        a = int(counts[c, 0])
        for k in range(K):
            b, i = int(counts[c, 1 + k]), int(counts[c, 1 + K + k])
            dice[k, c] = 1.0 if a + b == 0 else 2.0 * i / (a + b)
        est[c] = dice[:, c].mean()
        vols = counts[c, 1:1 + K].astype(np.float64)
        cv[c] = 0.0 if vols.mean() == 0 else vols.std() / vols.mean()
    return dice, est, cv


def dyadic_stack(K, nvox, C, seed):
    """values drawn uniformly from {0, .25, .5, .75, 1}: ties, values exactly on the threshold 0.5, even-K medians of exactly 0.5.  A
    variant keeps the element's own draw with probability 0.6 and takes a fresh one otherwise, so that the variants have something to
    agree on: every variant's set {v > 0.5} AND the consensus set {median > 0.5} hold about 40 % of the voxels at every K (with
    independent draws the consensus set of 64 variants would hold 6 % of them)"""
    rs = np.random.RandomState(seed)
    own = rs.randint(0, 5, size=(1, nvox, C))
    fresh = rs.randint(0, 5, size=(K, nvox, C))
    return np.asarray(DYADIC)[np.where(rs.rand(K, nvox, C) < 0.6, own, fresh)]


def smooth_stack(K, nvox, C, seed):
    """sigmoid-like fields in (0, 1): a slow wave per channel plus a per-variant perturbation, through a logistic"""
    rs = np.random.RandomState(seed)
    x = np.linspace(0.0, 6.0 * np.pi, nvox)[np.newaxis, :, np.newaxis]
    base = 2.5 * np.sin(x + np.arange(C)[np.newaxis, np.newaxis, :]) + 0.3 * rs.randn(1, nvox, C)
    return 1.0 / (1.0 + np.exp(-(base + 0.8 * rs.randn(K, nvox, C))))
